"""The kernels of the polynomial-preconditioned GMRES (csrc/das_poly.hpp) one by one on the device against longdouble restatements, with
the method of tests/test_gpu_idr_kernels.py: no mesh, no solver.  das_debug_poly_step runs the launch helpers the solver runs, on caller
data.  Every step variant: real root / first step of a pair / second step of a pair, each as the first, a middle and the last step of a
walk.  Bounds are derived (krylov_reference: an entry built from T terms |err| <= (T + 2) u sum|terms|), never tuned to what the kernels
give.  Every call runs twice for bitwise equality, every array sits in a sentinel guard band, what a step must not write (v always,
w always, prod on a last step, everything a variant has no business with) is compared with its copy, and what a variant must not READ
(poly and prod on a first step, w on a last real step) holds NaN.  Offsets 0 and 2 doubles from the allocation put every vector on a
16-byte boundary (16-byte path, with the element-wise last row when n is odd), offset 1 on an 8-byte one (element-wise path)."""
import numpy as np
import pytest

import krylov_reference as kr
from dafoam_amd import _capi
from krylov_reference import LD, SENTINEL

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")]

N_LIST = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 16 * 1024 + 1, 40000]
ILL_N = [17, 1025, 4097]
PAD = 5
REAL, PAIR_FIRST, PAIR_SECOND = 0, 1, 2
KIND_NAMES = {REAL: "real", PAIR_FIRST: "pair-first", PAIR_SECOND: "pair-second"}
POSITIONS = {"first": (1, 0), "middle": (0, 0), "last": (0, 1), "only": (1, 1)}


def dp(a):
    return _capi.dptr(a)


def banded(x, off):
    a = np.full(off + x.size + PAD, SENTINEL)
    a[off : off + x.size] = x
    return a


def run_step(n, kind, first, last, re, im, off, arrays):
    """two runs on copies of the five arrays; bitwise equal; returns the arrays after the step"""
    outs = []
    for _ in range(2):
        a = [x.copy() for x in arrays]
        _capi.check(_capi.lib().das_debug_poly_step(n, kind, first, last, re, im, off, a[0].size, *[dp(x) for x in a]))
        outs.append(a)
    for x, y in zip(*outs):
        assert x.tobytes() == y.tobytes(), "two runs on the same input differ bitwise"
    return outs[0]


def check_step(n, kind, pos, re, im, ill):
    first, last = POSITIONS[pos]
    v, w, prod, poly, tmp = (kr.vector(n, [71 + i, kind], ill) for i in range(5))
    nan = np.full(n, np.nan)
    if first:
        prod, poly = nan, nan  # the input of the walk is v; poly starts as zero without being read
    if kind == REAL and last:
        w = nan
    pin = (v if first else prod).astype(LD)
    m2 = re * re + im * im  # fp64, as the walk forms it
    want = {}  # index of the array -> (reference, magnitude, T)
    if kind == REAL:
        t = pin / LD(re)
        base = np.zeros(n, dtype=LD) if first else poly.astype(LD)
        want[3] = (base + t, np.abs(base) + np.abs(t), 2)
        if not last:
            t2 = w.astype(LD) / LD(re)
            want[2] = (pin - t2, np.abs(pin) + np.abs(t2), 2)
    elif kind == PAIR_FIRST:
        t1, t2 = LD(2.0 * re) * pin, w.astype(LD)
        want[4] = (t1 - t2, np.abs(t1) + np.abs(t2), 2)
        base = np.zeros(n, dtype=LD) if first else poly.astype(LD)
        want[3] = (base + (t1 - t2) / LD(m2), np.abs(base) + (np.abs(t1) + np.abs(t2)) / LD(m2), 3)
    elif not last:
        t2 = w.astype(LD) / LD(m2)
        want[2] = (pin - t2, np.abs(pin) + np.abs(t2), 2)
    worst = 0.0
    for off in (0, 1, 2):
        before = [banded(x, off) for x in (v, w, prod, poly, tmp)]
        after = run_step(n, kind, first, last, re, im, off, before)
        for i, (b, a) in enumerate(zip(before, after)):
            assert np.all(a[:off] == SENTINEL) and np.all(a[off + n :] == SENTINEL), f"guard band of array {i} overwritten"
            if i not in want:
                assert a.tobytes() == b.tobytes(), f"{KIND_NAMES[kind]} {pos}: array {i} must not be written"
                continue
            ref, mag, T = want[i]
            ok, ratio = kr.check_update(a[off : off + n], ref, mag, T)
            worst = max(worst, ratio)
            assert ok, (KIND_NAMES[kind], pos, n, off, i, ratio)
    return worst


@pytest.mark.parametrize("kind", [REAL, PAIR_FIRST, PAIR_SECOND], ids=lambda k: KIND_NAMES[k])
@pytest.mark.parametrize("n", N_LIST)
def test_root_steps(n, kind):
    for pos in POSITIONS:
        ratio = check_step(n, kind, pos, -1.375 if kind == REAL else 0.8125, 0.0 if kind == REAL else 1.1875, False)
        print(f"{KIND_NAMES[kind]} {pos} n={n}: max err / (u sum|terms|) = {ratio:.3g}")


@pytest.mark.parametrize("kind", [REAL, PAIR_FIRST, PAIR_SECOND], ids=lambda k: KIND_NAMES[k])
@pytest.mark.parametrize("n", ILL_N)
def test_root_steps_ill_scaled(n, kind):
    """|theta| from 1e-6 to 1e6 on vectors whose entries span twelve decades"""
    for scale in (1e-6, 1e-3, 1.0, 1e3, 1e6):
        for pos in POSITIONS:
            re, im = (-scale, 0.0) if kind == REAL else (0.6 * scale, 0.8 * scale)
            ratio = check_step(n, kind, pos, re, im, True)
            print(f"{KIND_NAMES[kind]} {pos} n={n} |theta|={scale:g}: max err / (u sum|terms|) = {ratio:.3g}")

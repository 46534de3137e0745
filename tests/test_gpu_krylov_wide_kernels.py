"""The 16-byte-load kernels of the delayed re-orthogonalisation (k_multidot2w, k_dcgs2w_update: the float basis, fp32 and split
storage) on the device against the longdouble restatements of tests/krylov_reference.py, with the bounds test_gpu_krylov_kernels.py
applies to the one-dword-per-lane kernels.  The launch helpers pick the path from the pointers and the leading dimension: an
allocation-aligned upload with n and ld multiples of 4 takes the 16-byte path (das_debug_krylov_wide_eligible tells), the same kind
of input with n + 1 rows takes the other one - both must meet the same bounds.  Shapes: n around the workgroup tiles of the two
kernels (1024 and 4096 rows), tight and padded leading dimensions, depths 1, 4, 5, 130 and 353 (the existing file stops at 129 / 9).
Last: the padded basis layout of the solver (rows of a float vector padded to a multiple of 4) in an adjoint solve whose n is no
multiple of 4."""
import ctypes as C

import numpy as np
import pytest

import krylov_reference as kr
from dafoam_amd import _capi
from krylov_reference import FP32, SPLIT

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")]

FMTS = [FP32, SPLIT]
FMT_ID = kr.FMT_NAMES.get
N_TILE = [4, 8, 1020, 1024, 1028, 4092, 4096, 4100, 8196]  # multiples of 4 around 1 and 2 tiles of 1024 and 4096 rows
N_LARGE = 2 ** 20 + 4
DEPTHS = [1, 4, 5, 130, 353]


def shapes():
    """every tile-boundary n at depth 5, every depth at n = 1028 and 4100, the large n at depth 5; well scaled, and ill scaled on a few"""
    out = [(n, 5, False) for n in N_TILE] + [(n, d, False) for n in (1028, 4100) for d in DEPTHS] + [(N_LARGE, 5, False)]
    out += [(1028, 5, True), (4100, 130, True), (4096, 353, True), (N_LARGE, 4, True)]
    return [pytest.param(n, d, ill, id=f"n{n}-d{d}" + ("-ill" if ill else "")) for n, d, ill in sorted(set(out))]


def vp(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def dp(a):
    return _capi.dptr(a)


def call(name, *args):
    _capi.check(getattr(_capi.lib(), name)(*args))


def eligible(n, fmt, ld):
    d, u = C.c_int(-1), C.c_int(-1)
    call("das_debug_krylov_wide_eligible", n, fmt, ld, C.byref(d), C.byref(u))
    return bool(d.value), bool(u.value)


def twice(fn):
    a, b = fn(), fn()
    assert a.tobytes() == b.tobytes(), "two runs on the same input differ bitwise"
    return a


def lds(n, fmt, aligned):
    """tight and padded; aligned: padded by 8 (the 16-byte path stays eligible), else by 3"""
    w = 2 * n if fmt == SPLIT else n
    return [w, w + (8 if aligned else 3)]


@pytest.fixture(autouse=True)
def wide_path_on():
    prev = C.c_int(0)
    call("das_debug_set_orth_wide", 1, C.byref(prev))
    yield
    call("das_debug_set_orth_wide", prev.value, None)


def dots2_case(n, K, ill, fmt, ld, want_wide):
    V = kr.vectors(n, K, 111, ill)
    v = kr.vector(n, [112, K], ill)
    B = kr.Basis(V, fmt, ld)
    assert eligible(n, fmt, ld)[0] == want_wide, "the inner products would not take the path this case is meant for"

    def run():
        out = np.zeros(2 * K)
        call("das_debug_krylov_dots2", n, K, fmt, vp(B.a), ld, dp(v), dp(out))
        return out

    got = twice(run)
    ref, mag = kr.ref_dots2(B, v)
    ok, ratio = kr.check_sum(got, ref, mag, n)
    print(f"multidot2 {'wide' if want_wide else 'scalar'} {kr.FMT_NAMES[fmt]} n={n} K={K} ld={ld}: max err / (u sum|xy|) = {ratio:.3g} (bound {n})")
    assert ok


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID)
@pytest.mark.parametrize("n,K,ill", shapes())
def test_multidot2_wide(n, K, ill, fmt):
    for ld in lds(n, fmt, True):
        dots2_case(n, K, ill, fmt, ld, True)
    # n + 1 rows, tight: the slots (ld = n + 1, split 2 n + 2 floats) and the lo half of a split slot are not 16-byte aligned
    dots2_case(n + 1, K, ill, fmt, lds(n + 1, fmt, False)[0], False)


def check_stored(B, slot, ref, mag, T, scale):
    st = B.slots()
    if B.fmt == FP32:
        return kr.check_fp32(st[slot, : B.n], ref)
    return kr.check_split(st[slot, : B.n], st[slot, B.n : 2 * B.n], ref, mag, T, scale)


def update_case(n, j, ill, fmt, ld, want_wide):
    V = kr.vectors(n, j + 1, 121, ill)
    v = kr.vector(n, [122, j], ill)
    sc = 0.25 * kr.vector(max(2 * j, 1), [123, j])
    gamma, ralpha = 0.8125 + 1e-3 * j, 1.0 / 0.73
    assert eligible(n, fmt, ld)[1] == want_wide, "the update would not take the path this case is meant for"
    B0 = kr.Basis(V, fmt, ld, extra_slots=2)
    (q, mq), (un, mu) = kr.ref_dcgs2_update(B0, j, sc, gamma, ralpha, v)

    def run():
        B = kr.Basis(V, fmt, ld, extra_slots=2)
        call("das_debug_krylov_dcgs2_update", n, j, fmt, vp(B.a), ld, B.nslots, dp(sc), gamma, ralpha, dp(v))
        return B.a

    B = kr.Basis(V, fmt, ld, extra_slots=2)
    B.a[:] = twice(run)
    w = B.width()
    assert np.array_equal(B.slots()[:j, :w], B0.slots()[:j, :w]), "the final basis vectors were modified"
    assert np.all(B.slots()[:, w:] == B.a.dtype.type(kr.SENTINEL)) and np.all(B.slots()[j + 2 :] == B.a.dtype.type(kr.SENTINEL)), "guard band overwritten"
    okq, rq = check_stored(B, j, q, mq, j + 1, ralpha)
    oku, ru = check_stored(B, j + 1, un, mu, j + 2, ralpha)
    print(f"dcgs2_update {'wide' if want_wide else 'scalar'} {kr.FMT_NAMES[fmt]} n={n} j={j} ld={ld}: q_j {rq:.3g}, u' {ru:.3g}")
    assert okq and oku


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID)
@pytest.mark.parametrize("n,j,ill", shapes())
def test_dcgs2_update_wide(n, j, ill, fmt):
    for ld in lds(n, fmt, True):
        update_case(n, j, ill, fmt, ld, True)
    update_case(n + 1, j, ill, fmt, lds(n + 1, fmt, False)[0], False)


def test_rows_not_a_multiple_of_four_on_the_wide_path():
    """fp32 storage with an aligned leading dimension and n = 4 m + 1, 2, 3: the 16-byte path with a partial last group of rows -
    the rows behind n (here: the sentinel) enter no sum and are not written"""
    for n in (5, 1026, 4099):
        ld = (n + 3) // 4 * 4 + 4
        dots2_case(n, 5, False, FP32, ld, True)
        update_case(n, 5, False, FP32, ld, True)


def test_switching_the_wide_path_off_selects_the_other_kernels():
    call("das_debug_set_orth_wide", 0, None)
    assert eligible(4096, SPLIT, 8192) == (False, False)
    dots2_case(4096, 5, False, SPLIT, 8192, False)
    update_case(4096, 5, False, SPLIT, 8192, False)
    call("das_debug_set_orth_wide", 1, None)
    assert eligible(4096, SPLIT, 8192) == (True, True)
    assert eligible(4096, kr.FP64, 4096) == (False, False)


def test_padded_split_basis_in_a_solve_whose_n_is_no_multiple_of_four():
    """The solver pads the rows of a float basis vector to a multiple of 4 (lo half n4 floats into a slot, slots 2 n4 apart), so that
    its basis always takes the 16-byte path; every other consumer of the basis goes through the same layout helpers.  An adjoint
    solve with n % 4 != 0: the split basis converges with the iteration count of the fp64 basis, psi agrees to 100 x the solve
    tolerance (the bound test_split_and_fp32_krylov_basis_storage uses for this comparison)."""
    from common import norm_states, options, relerr
    from dafoam_amd.meshgen import channel_case
    from dafoam_amd.pyDAFoam import PYDAFOAM
    from oracle import jacobian as J
    from oracle.foam_mesh import Geometry

    case = channel_case(11, 7, 5, perturb=0.0, lengths=(1.0, 0.2, 0.2), grading_y=2.0)
    g = Geometry(case.mesh)
    n = case.states.size
    assert n % 4 != 0, "this case is meant to have a vector length that is no multiple of 4"
    rhs = np.zeros(n)
    rhs[0 : 3 * g.nC : 3] = g.V
    rhs *= J.state_scales(case, g, norm_states(case))
    rtol = 1e-8
    out = {}
    for prec in ("fp64", "split", "fp32"):
        D = PYDAFOAM(options=options(case, adjEqnOption={"gmresRelTol": rtol, "gmresAbsTol": 1e-300, "gmresRestart": 800, "gmresMaxIters": 2000, "printInfo": 0},
                                     amd={"krylovBasisPrecision": prec}), case=case)
        psi, fail = D.solveAdjoint(rhs)
        info = D.ksp.info()
        out[prec] = dict(psi=psi, fail=fail, its=info["iters"], rel=info["res"] / info["res0"], basis=D.ksp.basisInfo())
        print(prec, "n", n, "iterations", info["iters"], "rel", info["res"] / info["res0"], D.ksp.basisInfo())
    n4 = (n + 3) // 4 * 4
    assert out["split"]["basis"]["split"] and out["split"]["basis"]["bytesPerVector"] == 8 * n4 and out["fp32"]["basis"]["bytesPerVector"] == 4 * n4
    assert out["fp64"]["basis"]["bytesPerVector"] == 8 * n
    for prec in ("fp64", "split", "fp32"):
        assert out[prec]["fail"] == 0 and out[prec]["rel"] <= rtol, (prec, out[prec]["rel"])
    assert out["split"]["its"] == out["fp64"]["its"], (out["split"]["its"], out["fp64"]["its"])
    assert relerr(out["split"]["psi"], out["fp64"]["psi"]) < 100 * rtol
    assert relerr(out["fp32"]["psi"], out["fp64"]["psi"]) < 100 * rtol

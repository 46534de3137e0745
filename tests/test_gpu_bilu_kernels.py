"""The kernels of the node-block ILU(0) preconditioner (dafoam_amd/csrc/das_bilu.hpp) on the device against their longdouble
restatements (tests/bilu_reference.py): no mesh, no solver.  The entries das_debug_bilu_* check a caller-made node structure on the
host and then run the numeric setup and the sweeps the solver runs.  Every stored block and node value is compared LOCALLY with the
derived bounds of bilu_reference (never tuned to what the kernels give), every operation is run twice for bitwise equality (fixed
summation order), the abort flag must stay 0, and out must be untouched wherever no nodeOut points.  The structures reach what no mesh
reaches: pass tails 0 .. 25 in both streams, empty nodes, late nodes, overlap copies of a two-block factor, un-owned rows, blocks that
need pivoting everywhere, exactly singular blocks, and a grid wide enough for the per-XCD ticket counters.  The achieved
max err / bound per kernel and storage format is printed by the last test (profiles/README.md holds a recorded table)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bilu_reference as br
from dafoam_amd import _capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")]

FIGURES = {}
WINDOW = (("window", 1),)  # diagScale = 1.75 on the rows below 3 n / 4 outside [n / 4, n / 2)


def rowlen_struct():
    g, blk = br.union(br.row_length_graph(1), br.mirror(br.row_length_graph(1)))
    return br.make(g, 3, blk=blk)


def multi_struct():
    g, blk = br.union(br.random_graph(17, 1), br.random_graph(9, 2))
    return br.make(g, 4, blk=blk, n_late=4, copies=3, n_unowned=5, late_late=2)


STRUCTS = {f"n{k}": (lambda k=k: br.make(br.random_graph(k, k), k, n_late=2 if k >= 8 else 0, n_unowned=3)) for k in br.NODE_COUNTS}
STRUCTS.update(rowlen=rowlen_struct, multi=multi_struct, wide=lambda: br.make(br.layered_graph(256, 4, 7), 7))


@functools.lru_cache(maxsize=None)
def struct(name):
    return STRUCTS[name]()


def args(S, kw):
    kw = dict(kw)
    if kw.pop("window", 0):
        kw.update(diagScale=1.75, exLo=S.n // 4, exHi=S.n // 2, end=3 * S.n // 4)
    return kw


@functools.lru_cache(maxsize=None)
def reference(name, kw=()):
    """(A, blocks, invD) of the longdouble restatement, computed once per structure and scatter variant"""
    S = struct(name)
    A, dropped = br.scatter(S, **args(S, kw))
    bv, invD, ns, kappa = br.factor(S, A)
    br.assert_tame(kappa)
    assert dropped == 0 and ns == 0
    return A, bv, invD


def record(op, fmt, res):
    for k, (ok, ratio) in res.items():
        FIGURES[(f"{op} {k}", fmt)] = max(FIGURES.get((f"{op} {k}", fmt), 0.0), ratio)
    return all(v[0] for v in res.values())


def device_factor(S, fp32=0, expect=0, **kw):
    d, keep = br.c_input(S, _capi, fp32=fp32, **kw)
    nN, nL, nU = S.nN, sum(S.nL(p) for p in range(S.nN)), sum(S.nU(p) for p in range(S.nN))
    F = br.Factor()
    F.Lptr, F.Uptr = np.zeros(nN + 1, dtype=np.int64), np.zeros(nN + 1, dtype=np.int64)
    F.Lcol, F.Ucol = np.zeros(nL, dtype=np.int32), np.zeros(nU, dtype=np.int32)
    vt = np.float32 if fp32 else np.float64
    F.Lval, F.Uval, F.invD = np.zeros(max(nL, 1) * 64, dtype=vt), np.zeros(max(nU, 1) * 64, dtype=vt), np.zeros(nN * 64)
    ns = C.c_int(-1)
    rc = _capi.lib().das_debug_bilu_factor(C.byref(d), F.Lptr.ctypes.data_as(_capi.c_ll_p), F.Uptr.ctypes.data_as(_capi.c_ll_p), F.Lcol.ctypes.data_as(_capi.c_int_p),
                                           F.Ucol.ctypes.data_as(_capi.c_int_p), F.Lval.ctypes.data_as(C.c_void_p), F.Uval.ctypes.data_as(C.c_void_p), _capi.dptr(F.invD),
                                           C.byref(ns))
    if expect:
        assert rc == expect, (rc, _capi.lib().das_last_error())
        return None
    _capi.check(rc)
    F.Lval, F.Uval, F.nshift = F.Lval[: nL * 64], F.Uval[: nU * 64], ns.value
    return F


def device_apply(S, B, ld=None, fp32=0, twice=1, **kw):
    """-> out (nrhs, ld), y, z (nN, 8, S_last) of the last group launched, info"""
    d, keep = br.c_input(S, _capi, fp32=fp32, **kw)
    nrhs, ld = B.shape[0], ld or S.n
    b = np.full((nrhs, max(ld, S.n)), 0.625)
    b[:, : S.n] = B
    out = np.full((nrhs, ld), br.SENTINEL)
    y, z = np.zeros(S.nN * 32), np.zeros(S.nN * 32)
    abort, info = C.c_int(-1), (C.c_int * 4)()
    _capi.check(_capi.lib().das_debug_bilu_apply(C.byref(d), nrhs, ld, _capi.dptr(b), _capi.dptr(out), twice, _capi.dptr(y), _capi.dptr(z), C.byref(abort), info))
    assert abort.value == 0, "a sweep ran into its spin limit"
    last = 1 if nrhs & 1 else (2 if nrhs % 4 == 2 else 4)
    return out, y[: S.nN * 8 * last].reshape(S.nN, 8, last), z[: S.nN * 8 * last].reshape(S.nN, 8, last), list(info)


def same(a, b):
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def factor_arrays(F):
    return F.Lptr, F.Uptr, F.Lcol, F.Ucol, F.Lval, F.Uval, F.invD


@functools.lru_cache(maxsize=None)
def checked_factor(name, fp32=0, kw=()):
    """the device factor of a structure (twice, bitwise equal); fp64: every block against the bounds; fp32: the rounded fp64 factor"""
    S = struct(name)
    F, F2 = device_factor(S, fp32, **args(S, kw)), device_factor(S, fp32, **args(S, kw))
    assert same(factor_arrays(F), factor_arrays(F2)) and F.nshift == F2.nshift == 0, "two factorisations of the same input differ"
    if fp32:
        assert br.check_fp32(checked_factor(name, 0, kw), F), "the float factor is not the rounded double factor"
    else:
        A, bv, invD = reference(name, kw)
        res = br.check_factor(S, A, F)
        print(f"factor {name} {dict(kw)}: max err / bound " + ", ".join(f"{k} {v[1]:.3g}" for k, v in res.items()))
        assert record("k_bilu_scatter + k_bilu_factor + k_bilu_pack", "fp64", res)
        got, ginv = br.decode(S, F)
        off = np.ones(len(bv), dtype=bool)
        off[S.bdiag] = False
        assert br.relerr(got[off], bv[off]) < 1e-9 and br.relerr(ginv, invD) < 1e-9
    return F


def check_apply(name, nrhs, fp32, ld=None, kw=(), env=""):
    S = struct(name)
    F = checked_factor(name, fp32, kw)
    B = br.rhs(S, nrhs, 51)
    out, y, z, info = device_apply(S, B, ld, fp32, **args(S, kw))
    assert same((out, y, z), device_apply(S, B, ld, fp32, **args(S, kw))[:3]), "two applications to the same input differ"
    last = y.shape[2]
    fmt = "fp32" if fp32 else "fp64"
    res = br.check_sweeps(S, F, B[nrhs - last :], y, z)
    print(f"sweeps {name} {fmt} nrhs={nrhs} ld={out.shape[1]} {env}grid={info[0]} perXcd={info[2]}: max err / bound y {res['y'][1]:.3g}, z {res['z'][1]:.3g}")
    assert record("k_bilu_sweep" + ("_m" if last > 1 else ""), fmt, res)
    assert br.check_out(S, z, out[nrhs - last :]), "out is not z where nodeOut points, or was written elsewhere"
    m = br.owned(S)
    assert np.all(out[:, : S.n][:, ~m] == br.SENTINEL) and np.all(out[:, S.n :] == br.SENTINEL)
    A, bv, invD = reference(name, kw)
    want = br.sweeps(S, bv, invD, B)[2]
    assert br.relerr(out[:, : S.n][:, m], want[:, m]) < (1e-2 if fp32 else 1e-9)
    if fp32:  # and against the longdouble solve with the stored float factor
        assert br.relerr(out[:, : S.n][:, m], br.sweeps(S, *br.decode(S, F), B)[2][:, m]) < 1e-9
    return out, y, z, info


# ---- 1. scatter, pad, factor, pack ------------------------------------------------------------------------------------------------------
VARIANTS = {"plain": (), "transpose": (("transpose", 1),), "shift": WINDOW, "transpose-shift": (("transpose", 1),) + WINDOW}


@pytest.mark.parametrize("name,kw", [pytest.param(n, kw, id=f"{n}-{v}") for n in STRUCTS for v, kw in VARIANTS.items() if n != "wide" or v in ("plain", "transpose-shift")])
def test_factor(name, kw):
    S = struct(name)
    if name == "rowlen":
        assert {S.nL(p) for p in range(S.nN)} >= set(br.ROW_LENGTHS) and {S.nU(p) for p in range(S.nN)} >= set(br.ROW_LENGTHS)
    if name == "multi":  # two maps, overlap copies, late nodes, late-late couplings (dropped without error), un-owned rows
        assert len(S.maps) == 2 and (S.nodeOut != S.nodeUnk).any() and S.late.sum() == 4 and S.n_late_late == 2 and S.unowned.size == 5
    checked_factor(name, 0, kw)
    checked_factor(name, 1, kw)


def test_coupling_outside_the_pattern_is_an_error_naming_the_count():
    S = br.make(br.random_graph(9, 2), 6, n_late=3, late_late=2, outside=3)
    assert br.scatter(S)[1] == 3
    device_factor(S, expect=-5)
    assert b"3 matrix entries fall outside the node pattern" in _capi.lib().das_last_error()


# ---- 2. the sweeps ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("nrhs", [1, 2, 4])
@pytest.mark.parametrize("name", list(STRUCTS))
def test_sweeps(name, nrhs, fp32):
    out, y, z, info = check_apply(name, nrhs, fp32)
    if name == "wide":
        assert info[0] >= 64, "the wide structure does not reach the grid of the per-XCD tickets"
        assert info[2] == (1 if info[3] == 8 else 0)
        print("wide structure: " + ("per-XCD ticket counters ran" if info[2] else "device-wide ticket counter ran: the device is partitioned, the per-XCD branch was NOT covered"))


@pytest.mark.parametrize("env", [{"DAS_BILU_WGS": "1"}, {"DAS_BILU_XCD": "0"}, {"DAS_BILU_WGS": "1", "DAS_BILU_XCD": "0"}], ids=["wgs1", "xcd0", "wgs1-xcd0"])
@pytest.mark.parametrize("name", ["n9", "n65", "rowlen", "multi", "wide"])
def test_launch_shape_does_not_change_a_bit(name, env, monkeypatch):
    S = struct(name)
    base = {nrhs: device_apply(S, br.rhs(S, nrhs, 51)) for nrhs in (1, 4)}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for nrhs in (1, 4):
        got = check_apply(name, nrhs, 0, env=f"{env} ")
        assert got[3][0] == (1 if "DAS_BILU_WGS" in env else base[nrhs][3][0]) and (got[3][2] == 0 or "DAS_BILU_XCD" not in env)
        assert same(got[:3], base[nrhs][:3]), "the launch shape changed the result"


@pytest.mark.parametrize("fp32", [0, 1], ids=["fp64", "fp32"])
@pytest.mark.parametrize("pad", [0, 3], ids=["ld=n", "ld=n+3"])
@pytest.mark.parametrize("nrhs", [3, 5, 7, 8])
def test_right_hand_side_groups(nrhs, pad, fp32):
    """groups of 4, 2, 1 and their column offsets: every column against the one-column sweep.  Both are float64 evaluations of the same
    two sweeps with the same stored factor, each within 1e-12 of the longdouble one on these inputs (CPU tier): 2e-12 apart at most"""
    for name in ("multi", "rowlen"):
        S = struct(name)
        out = check_apply(name, nrhs, fp32, ld=S.n + pad)[0]
        m = br.owned(S)
        B = br.rhs(S, nrhs, 51)
        for r in range(nrhs):
            one = device_apply(S, B[r : r + 1], fp32=fp32)[0]
            assert br.relerr(out[r, : S.n][m], one[0][m]) < 2e-12, r


# ---- 3. pivoting and the pivot shift ------------------------------------------------------------------------------------------------------
def test_pivoting_is_needed_everywhere():
    """every diagonal block of more than one unknown has its rows shifted and a leading entry of 1e-14: test_factor holds the inverses
    to 8^3 u kappa ||inv||; here: the same matrices without the row shift give another factor (the generator does what it says)"""
    S = struct("n17")
    A, _, _ = reference("n17")
    D = A[S.bdiag].astype(np.float64)
    big = [p for p in range(S.nN) if (S.nodeUnk[p] >= 0).sum() >= 2]
    assert big and all(np.abs(np.diag(D[p])[S.nodeUnk[p] >= 0]).max() < 2.0 < np.abs(D[p]).max() for p in big)
    for p in big:  # elimination in float64 without the row search misses the bound of the inverse
        ref, ns = br.inverse8(D[p])
        bad = br.inverse8(D[p], np.float64, pivot=False)[0]
        ninv = np.abs(ref).sum(axis=1).max()
        assert ns == 0 and np.abs(bad - ref).max() > 8 ** 3 * 2.0 ** -53 * np.abs(D[p]).sum(axis=1).max() * ninv * ninv


def test_pivot_shift():
    g, blk = br.union(br.random_graph(9, 1), br.random_graph(9, 2), br.random_graph(9, 3))
    S = br.make(g, 5, blk=blk, singular=(0, 9))
    sing = [int(S.pos[0]), int(S.pos[9])]
    A, _ = br.scatter(S)
    bv, invD, ns, kappa = br.factor(S, A)
    fy, fz = br.downstream(S, sing)
    assert ns == 2 and (~fz).sum() >= 9
    F, F2 = device_factor(S), device_factor(S)
    assert same(factor_arrays(F), factor_arrays(F2))
    assert F.nshift == F2.nshift == ns
    assert all(np.all(np.isfinite(a)) for a in (F.Lval, F.Uval, F.invD))
    assert record("k_bilu_factor away from the shifted pivots", "fp64", br.check_factor(S, A, F, nodes=np.flatnonzero(~fy)))
    for s in sing:
        res = br.check_shifted_inverse(A[S.bdiag[s]], F.invD.reshape(-1, 8, 8)[s])
        assert record("bilu_inverse8", "fp64", {"shifted": res})
    B = br.rhs(S, 1, 52)
    out, y, z, info = device_apply(S, B)
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(z)) and np.all(np.isfinite(out))
    assert all(v[0] for v in br.check_sweeps(S, F, B, y, z, nodes=np.flatnonzero(~fz)).values()) and br.check_out(S, z, out)
    m = np.zeros(S.n, dtype=bool)
    m[S.nodeOut[~fz][S.nodeOut[~fz] >= 0]] = True
    assert br.relerr(out[:, m], br.sweeps(S, bv, invD, B)[2][:, m]) < 1e-9


# ---- 4. argument checks -------------------------------------------------------------------------------------------------------------------
def test_invalid_structures_are_refused():
    S = br.make([[], [0], [0, 1]], 21, empty_nodes=[])
    L = _capi.lib()
    B = br.rhs(S, 1, 1)
    for name, override in br.bad_inputs(S):
        device_factor(S, expect=-1, **override)
        assert b"das_debug_bilu_factor" in L.das_last_error(), name
        with pytest.raises(_capi.DASError, match="error -1: das_debug_bilu_apply"):
            device_apply(S, B, **override)
    for bad in (dict(B=br.rhs(S, 1, 1), ld=S.n - 1), dict(B=np.zeros((9, S.n))), dict(B=np.zeros((0, S.n)))):
        with pytest.raises(_capi.DASError, match="error -1: das_debug_bilu_apply"):
            device_apply(S, **bad)
    assert all(v[0] for v in br.check_factor(S, br.scatter(S)[0], device_factor(S)).values())  # and the valid structure still goes through


def test_zzz_print_achieved_errors():
    print("\nachieved max err / bound per kernel and storage format (1 = the bound):")
    for (op, fmt), ratio in sorted(FIGURES.items()):
        print(f"  {op:<62s} {fmt:<5s} {ratio:9.3g}")
    assert all(r <= 1.0 for r in FIGURES.values())

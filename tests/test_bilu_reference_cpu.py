"""CPU tier of the node-block ILU kernel tests: (1) the restatements of tests/bilu_reference.py against a dense mpmath solve on tiny
structures whose pattern is complete (the incomplete factor is then the exact one); (2) the generators stay inside the cap on the
condition of the diagonal blocks, need pivoting, and let a float64 restatement reach 1e-12 of the longdouble one; (3) the comparison
functions ACCEPT that float64 restatement everywhere and REJECT every mutation listed below, each at the smallest place where it can be
expressed; (4) the argument checks of the C-ABI entries refuse every invalid structure before anything is launched (they need no
device: a launch on this tier would come back as another error code)."""
import ctypes as C

import mpmath
import numpy as np
import pytest

import bilu_reference as br
from dafoam_amd import _capi
from krylov_reference import LD

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")


def rowlen_struct():
    g, blk = br.union(br.row_length_graph(1), br.mirror(br.row_length_graph(1)))
    return br.make(g, 3, blk=blk)


def multi_struct():
    g, blk = br.union(br.random_graph(17, 1), br.random_graph(9, 2))
    return br.make(g, 4, blk=blk, n_late=4, copies=3, n_unowned=5, late_late=2)


def singular_struct():
    g, blk = br.union(br.random_graph(9, 1), br.random_graph(9, 2), br.random_graph(9, 3))
    return br.make(g, 5, blk=blk, singular=(0, 9))


STRUCTS = {"rowlen": rowlen_struct, "multi": multi_struct, "n9": lambda: br.make(br.random_graph(9, 9), 9, n_late=2, n_unowned=3)}
_cache = {}


def device64(name, **kw):
    """(S, A longdouble, float64 blocks, float64 invD, stored Factor): the float64 restatement standing in for the device"""
    key = (name, tuple(sorted(kw.items())))
    if key not in _cache:
        S = STRUCTS[name]()
        A, dropped = br.scatter(S, **kw)
        assert dropped == 0
        b64, i64, ns, _ = br.factor(S, br.scatter(S, dtype=np.float64, **kw)[0], np.float64)
        _cache[key] = (S, A, b64, i64, br.pack(S, b64, i64, ns))
    return _cache[key]


def all_ok(res):
    return all(v[0] for v in res.values())


# ---- 1. the restatement against a dense solve ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose,diagScale", [(0, 1.0), (1, 1.0), (0, 1.75), (1, 1.75)])
def test_restatement_solves_a_complete_pattern_exactly(transpose, diagScale):
    S = br.make([[], [0], [0, 1]], 21, empty_nodes=[], n_unowned=2)
    lo, hi, end = S.n // 4, S.n // 2, 3 * S.n // 4
    A, dropped = br.scatter(S, transpose, diagScale, lo, hi, end)
    bv, invD, ns, kappa = br.factor(S, A)
    assert dropped == 0 and ns == 0
    B = br.rhs(S, 2, 22)
    _, _, out = br.sweeps(S, bv, invD, B)
    own = np.flatnonzero(br.owned(S))
    loc = {g: k for k, g in enumerate(own)}
    with mpmath.workprec(200):
        M = mpmath.zeros(own.size)
        for row in own:
            for k in range(S.rp[row], S.rp[row + 1]):
                j = int(S.ci[k])
                if j in loc:
                    v = mpmath.mpf(float(S.val[k]))
                    if j == row and row < end and not (lo <= row < hi):
                        v *= mpmath.mpf(diagScale)
                    M[(loc[j], loc[row]) if transpose else (loc[row], loc[j])] = v
        for r in range(2):
            x = mpmath.lu_solve(M, mpmath.matrix([mpmath.mpf(float(B[r, g])) for g in own]))
            err = max(abs(mpmath.mpf(float(out[r, g])) - x[k]) for k, g in enumerate(own))
            assert err <= 1e-14 * max(abs(v) for v in x)  # out is rounded to float64: 2^-53 and a few longdouble roundings
    assert np.all(out[:, S.unowned] == br.SENTINEL)


def test_packed_layout_round_trip_and_position():
    blks = np.arange(9 * 64, dtype=np.float64).reshape(9, 8, 8)
    flat = br.pack_row(blks)
    assert np.array_equal(br.unpack_row(flat, 9), blks)
    # element (r, k) of block a = 8 pass + g sits at pass 512 + (((r >> 1) nb + g) 8 + k) 2 + (r & 1) with nb = blocks of the pass
    for a, r, k in [(0, 0, 0), (3, 5, 2), (7, 7, 7), (8, 0, 0), (8, 6, 3)]:
        ps, g = a >> 3, a & 7
        nb = min(8, 9 - 8 * ps)
        assert flat[ps * 512 + (((r >> 1) * nb + g) * 8 + k) * 2 + (r & 1)] == blks[a, r, k]


def test_inverse_needs_pivoting_and_shifts_like_the_kernel():
    D = br.diag_block(8, 5)
    inv, ns = br.inverse8(D)
    assert ns == 0 and np.abs((inv @ D.astype(LD)) - np.eye(8)).max() < 1e-17
    bad, _ = br.inverse8(D, pivot=False)
    assert abs(D[0, 0]) < 1e-13 and not np.abs((bad @ D.astype(LD)) - np.eye(8)).max() < 1e-6  # the tiny leading entry costs every digit
    Z = D.copy()
    Z[-1, :] = 0.0
    invz, ns = br.inverse8(Z)
    assert ns == 1 and np.all(np.isfinite(invz.astype(np.float64))) and invz[7, 7] == LD(1.0) / LD(1e-12)
    Z[-1, -1] = -1e-305
    invn, ns = br.inverse8(Z)
    assert ns == 1 and invn[7, 7] == LD(1.0) / LD(-1e-12)
    Z[-1, -1] = -0.0  # not below zero: the shift is positive
    assert br.inverse8(Z)[0][7, 7] == LD(1.0) / LD(1e-12)


# ---- 2. the generators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_generators_are_tame_and_float64_reaches_1e12(name):
    S, A, b64, i64, F = device64(name)
    bv, invD, ns, kappa = br.factor(S, A)
    br.assert_tame(kappa)
    assert ns == 0
    m = br.owned(S)
    B = br.rhs(S, 2, 31)
    assert br.relerr(br.sweeps(S, b64, i64, B, np.float64)[2][:, m], br.sweeps(S, bv, invD, B)[2][:, m]) < 1e-12
    if name == "rowlen":
        assert {S.nL(p) for p in range(S.nN)} >= set(br.ROW_LENGTHS) and {S.nU(p) for p in range(S.nN)} >= set(br.ROW_LENGTHS)
    if name == "multi":
        assert len(S.maps) == 2 and S.late.sum() == 4 and (S.nodeOut != S.nodeUnk).any() and S.n_late_late == 2 and S.unowned.size == 5
    assert any((S.nodeUnk[p] < 0).all() for p in range(S.nN)), "no empty node"
    # the generator alone, many seeds: condition of every reference diagonal block under the cap
    for seed in range(20):
        T = br.make(br.random_graph(17, seed, maxdeg=6), seed, n_late=2)
        br.assert_tame(br.factor(T, br.scatter(T)[0])[3])


def test_outside_couplings_are_counted_and_late_late_ones_are_not():
    S = br.make(br.random_graph(9, 2), 6, n_late=3, late_late=2, outside=3)
    assert (S.n_late_late, S.n_outside) == (2, 3) and br.scatter(S)[1] == 3 and br.scatter(S, transpose=1)[1] == 3


# ---- 3. the comparison functions accept float64 and reject the mutations -----------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STRUCTS))
@pytest.mark.parametrize("kw", [{}, {"transpose": 1}, {"diagScale": 1.75, "exLo": 20, "exHi": 50, "end": 90}], ids=["plain", "transpose", "shift"])
def test_float64_restatement_is_accepted(name, kw):
    S, A, b64, i64, F = device64(name, **kw)
    assert all_ok(br.check_factor(S, A, F))
    F32 = br.pack(S, b64, i64, 0, np.float32)
    assert br.check_fp32(F, F32)
    B = br.rhs(S, 4, 41)
    for fac in (F, F32):
        bw, iw = br.decode(S, fac)
        y, z, out = br.sweeps(S, bw.astype(np.float64), iw.astype(np.float64), B, np.float64)
        assert all_ok(br.check_sweeps(S, fac, B, y, z)) and br.check_out(S, z, out)


def test_dropped_skipped_and_swapped_blocks_are_rejected():
    S, A, b64, i64, F = device64("rowlen")
    B = br.rhs(S, 2, 42)
    y, z, _ = br.sweeps(S, b64, i64, B, np.float64)
    assert all_ok(br.check_sweeps(S, F, B, y, z))
    p9 = next(p for p in range(S.nN) if S.nL(p) == 9)
    q9 = next(p for p in range(S.nN) if S.nU(p) == 9)
    # one L block dropped from a row: by the factorisation (stored as zero) and by the sweep
    G = br.pack(S, b64, i64)
    G.Lval[G.Lptr[p9] * 64 : G.Lptr[p9] * 64 + 512].reshape(4, 8, 8, 2)[:, 3] = 0.0
    assert not br.check_factor(S, A, G)["L"][0]
    for first, last, name in ((3, 4, "one block"), (8, 9, "the last pass of a 9-block row")):
        yb = y.copy()
        for e in range(int(S.bptr[p9]) + first, int(S.bptr[p9]) + last):
            yb[p9] += b64[e] @ y[S.bcol[e]]
        assert not br.check_sweeps(S, F, B, yb, z)["y"][0], name
        zb = z.copy()
        for e in range(int(S.bdiag[q9]) + 1 + first, int(S.bdiag[q9]) + 1 + last):
            zb[q9] += i64[q9] @ (b64[e] @ z[S.bcol[e]])
        assert not br.check_sweeps(S, F, B, y, zb)["z"][0], name
    # two blocks of a pass swapped: in the full first pass, and in the one-block last pass against the pass before
    for stream, node, key in (("Lval", p9, "L"), ("Uval", S.nN - 1 - q9, "U")):
        ptr = F.Lptr if stream == "Lval" else F.Uptr
        G = br.pack(S, b64, i64)
        v = getattr(G, stream)[ptr[node] * 64 : ptr[node] * 64 + 512].reshape(4, 8, 8, 2)
        v[:, [0, 1]] = v[:, [1, 0]]
        assert not br.check_factor(S, A, G)[key][0]
        G = br.pack(S, b64, i64)
        w = getattr(G, stream)[ptr[node] * 64 : (ptr[node] + 9) * 64]
        w[:] = br.pack_row(br.unpack_row(w, 9)[[0, 1, 2, 3, 4, 5, 6, 8, 7]])
        assert not br.check_factor(S, A, G)[key][0]
    # the 9-block row packed as if its last pass were full (nb = 8 instead of 1)
    G = br.pack(S, b64, i64)
    last = b64[S.bptr[p9] + 8]
    G.Lval[(G.Lptr[p9] + 8) * 64 : (G.Lptr[p9] + 9) * 64] = 0.0
    for r in range(8):
        for k in range(8):
            i = (((r >> 1) * 8 + 0) * 8 + k) * 2 + (r & 1)
            if i < 64:
                G.Lval[(G.Lptr[p9] + 8) * 64 + i] = last[r, k]
    assert not br.check_factor(S, A, G)["L"][0]


def test_wrong_inverses_are_rejected():
    S, A, b64, i64, F = device64("n9")
    B = br.rhs(S, 1, 43)
    y, z, _ = br.sweeps(S, b64, i64, B, np.float64)
    p = next(p for p in range(S.nN) if (S.nodeUnk[p] >= 0).sum() >= 2)
    # invD transposed: stored so, and used so by the sweep
    G = br.pack(S, b64, i64)
    G.invD.reshape(-1, 8, 8)[p] = i64[p].T
    assert not br.check_factor(S, A, G)["invD"][0]
    zb = z.copy()
    zb[p] = i64[p].T @ np.linalg.solve(i64[p], z[p])
    assert not br.check_sweeps(S, F, B, y, zb)["z"][0]
    # the pivot search switched off
    bn, inn, _, _ = br.factor(S, br.scatter(S, dtype=np.float64)[0], np.float64, pivot=False)
    assert not br.check_factor(S, A, br.pack(S, bn, inn))["invD"][0]


def test_flipped_shift_sign_is_rejected():
    S = singular_struct()
    A, _ = br.scatter(S)
    bv, invD, ns, kappa = br.factor(S, A)
    sing = [int(S.pos[0]), int(S.pos[9])]
    br.assert_tame(kappa, skip=np.flatnonzero(br.downstream(S, sing)[0]))
    assert ns == 2 and invD[sing[0], 7, 7] > 0 > invD[sing[1], 7, 7]
    A64 = br.scatter(S, dtype=np.float64)[0]
    b64, i64, ns64, _ = br.factor(S, A64, np.float64)
    assert ns64 == 2 and np.all(np.isfinite(i64)) and np.all(np.isfinite(b64))
    fy, fz = br.downstream(S, sing)
    assert (~fz).sum() >= 9, "no node left that does not depend on a shifted pivot"
    assert all_ok(br.check_factor(S, A, br.pack(S, b64, i64, ns64), nodes=np.flatnonzero(~fy)))
    assert all_ok(br.check_factor(S, A, br.pack(S, b64, i64, ns64), nodes=sing))
    bf, inf_, nsf, _ = br.factor(S, A64, np.float64, flip_shift=True)
    assert nsf == 2
    for s in sing:  # the bound of an ordinary block is too wide at a shifted one (kappa 1e13) to tell the sign: the scaled one does
        D = A[S.bdiag[s]]
        assert br.check_shifted_inverse(D, i64[s])[0] and not br.check_shifted_inverse(D, inf_[s])[0]
        assert not br.check_shifted_inverse(D, i64[s].T)[0]


def test_exchanged_right_hand_sides_and_a_writing_copy_are_rejected():
    S, A, b64, i64, F = device64("multi")
    B = br.rhs(S, 4, 44)
    y, z, out = br.sweeps(S, b64, i64, B, np.float64)
    assert all_ok(br.check_sweeps(S, F, B, y, z)) and br.check_out(S, z, out)
    p = next(p for p in range(S.nN) if S.nL(p) > 0 and (S.nodeUnk[p] >= 0).any())
    for which in ("y", "z"):
        yb, zb = y.copy(), z.copy()
        v = yb if which == "y" else zb
        v[p][:, [1, 2]] = v[p][:, [2, 1]]
        assert not br.check_sweeps(S, F, B, yb, zb)[which][0]
    # an overlap copy writing out: the owner's value is replaced by the copy's (the other block's solution)
    c = next(p for p in range(S.nN) if (S.nodeOut[p] != S.nodeUnk[p]).any())
    ob = out.copy()
    m = S.nodeUnk[c] >= 0
    ob[:, S.nodeUnk[c][m]] = z[c][m].T
    assert not br.check_out(S, z, ob)
    ob = out.copy()
    ob[0, S.unowned[0]] = 1.0  # and an entry nobody owns written
    assert not br.check_out(S, z, ob)


def test_ignored_transpose_and_misplaced_shift_are_rejected():
    S, A, _, _, _ = device64("n9", transpose=1)
    bn, inn, _, _ = br.factor(S, br.scatter(S, transpose=1, dtype=np.float64, ignore_transpose=True)[0], np.float64)
    res = br.check_factor(S, A, br.pack(S, bn, inn))
    assert not res["L"][0] and not res["U"][0] and not res["invD"][0]
    kw = dict(diagScale=1.75, exLo=S.n // 4, exHi=S.n // 2, end=3 * S.n // 4)
    S, A, _, _, F = device64("n9", **kw)
    assert all_ok(br.check_factor(S, A, F))
    bn, inn, _, _ = br.factor(S, br.scatter(S, dtype=np.float64, shift_in_window=True, **kw)[0], np.float64)
    assert not br.check_factor(S, A, br.pack(S, bn, inn))["invD"][0]
    kw["end"] = 1 << 62  # and the end of the shifted rows ignored
    bn, inn, _, _ = br.factor(S, br.scatter(S, dtype=np.float64, **kw)[0], np.float64)
    assert not br.check_factor(S, A, br.pack(S, bn, inn))["invD"][0]


def test_truncated_fp32_value_is_rejected():
    S, A, b64, i64, F = device64("rowlen")
    F32 = br.pack(S, b64, i64, 0, np.float32)
    assert br.check_fp32(F, F32)
    for stream in ("Lval", "Uval"):
        G = br.pack(S, b64, i64, 0, np.float32)
        v, d = getattr(G, stream), getattr(F, stream)
        k = int(np.flatnonzero(np.abs(v.astype(np.float64)) > np.abs(d))[0])  # rounded away from zero: truncation differs
        v[k] = np.nextafter(v[k], np.float32(0.0))
        assert not br.check_fp32(F, G)


# ---- 4. the argument checks of the entries ---------------------------------------------------------------------------------------------
def test_entries_refuse_invalid_structures_before_any_launch():
    L = _capi.lib()
    S = br.make([[], [0], [0, 1]], 21, empty_nodes=[])
    nN, nnz = S.nN, int(S.bptr[-1])
    Lptr, Uptr = np.zeros(nN + 1, dtype=np.int64), np.zeros(nN + 1, dtype=np.int64)
    Lcol, Ucol = np.zeros(nnz, dtype=np.int32), np.zeros(nnz, dtype=np.int32)
    Lval, Uval, invD = np.zeros(nnz * 64), np.zeros(nnz * 64), np.zeros(nN * 64)
    nshift, abort, info = C.c_int(0), C.c_int(0), (C.c_int * 4)()
    b, out, y, z = br.rhs(S, 8, 1), np.zeros((8, S.n)), np.zeros(nN * 32), np.zeros(nN * 32)
    ip, lp, vp = _capi.c_int_p, _capi.c_ll_p, C.c_void_p

    def factor(d):
        return L.das_debug_bilu_factor(d, Lptr.ctypes.data_as(lp), Uptr.ctypes.data_as(lp), Lcol.ctypes.data_as(ip), Ucol.ctypes.data_as(ip),
                                       Lval.ctypes.data_as(vp), Uval.ctypes.data_as(vp), _capi.dptr(invD), C.byref(nshift))

    def apply(d, nrhs=1, ld=S.n, bb=b, oo=out):
        return L.das_debug_bilu_apply(d, nrhs, ld, None if bb is None else _capi.dptr(bb), None if oo is None else _capi.dptr(oo), 1, _capi.dptr(y), _capi.dptr(z),
                                      C.byref(abort), info)

    for name, override in br.bad_inputs(S):
        d, keep = br.c_input(S, _capi, **override)
        assert factor(C.byref(d)) == -1 and b"das_debug_bilu_factor" in L.das_last_error(), name
        assert apply(C.byref(d)) == -1 and b"das_debug_bilu_apply" in L.das_last_error(), name
    d, keep = br.c_input(S, _capi)
    assert factor(None) == -1 and apply(None) == -1
    assert apply(C.byref(d), nrhs=0) == -1 and apply(C.byref(d), nrhs=9) == -1 and apply(C.byref(d), ld=S.n - 1) == -1
    assert apply(C.byref(d), bb=None) == -1 and apply(C.byref(d), oo=None) == -1
    assert L.das_debug_bilu_factor(C.byref(d), None, Uptr.ctypes.data_as(lp), Lcol.ctypes.data_as(ip), Ucol.ctypes.data_as(ip), Lval.ctypes.data_as(vp),
                                   Uval.ctypes.data_as(vp), _capi.dptr(invD), C.byref(nshift)) == -1
    assert np.all(out == 0.0) and np.all(invD == 0.0)

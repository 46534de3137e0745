"""The coarse-space kernels of the two-level preconditioner (dafoam_amd/csrc/das_coarse.hpp: k_coarse_assemble, k_gj_pivot, k_gj_elim,
k_coarse_restrict, k_coarse_solve, k_coarse_prolong, k_az_build, k_az_apply) on the device against their restatements in
tests/coarse_reference.py: no mesh, no solver.  The entries das_debug_coarse_* check the caller-made structure on the host and then run
the launch sequences the solver runs.  Every entry is called twice for bitwise equality.  The inputs reach what no mesh reaches: 1 to
2048 aggregates (every trip count of the 256-stride loops, accs[2048] full), aggregates without a row cell and of one cell, cells of no
aggregate, columns on both sides of the field block, transposed storage, a scaled diagonal; pivots 256 rows below the diagonal, exact
inverses, singular matrices; aggregates of 0 .. 1000 cells around the 64-lane shuffle and the 256-thread stride; rows that touch 0 .. 64
aggregates and one that touches 65.

The poisoned restriction (test_correct_poisoned) is stated for what IEEE arithmetic gives: k_coarse_solve is a dense product, it
multiplies the NaN of the poisoned t by every entry of its column of Einv, zeros of a block-diagonal Einv included, and 0 x NaN is NaN -
so every u is non-finite, not only the coupled ones.  What is asserted: exactly the poisoned t is non-finite, u is what the float64
product of Einv with the device's own t gives (NaN where it gives NaN), and y is non-finite exactly at the field cells of an aggregate."""
import functools

import numpy as np
import pytest

import coarse_reference as cr
import krylov_reference as kr
from dafoam_amd import _capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")]
LD = cr.LD
RATIOS = {}


def twice(run):
    a, b = run(), run()
    assert a[0] == 0, _capi.lib().das_last_error()
    assert b[0] == 0 and all(cr.same(np.asarray(p), np.asarray(q)) for p, q in zip(a[1:], b[1:])), "two runs on the same input differ"
    return a[1:]


def record(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))
    print(f"{name}: achieved / bound = {ratio:.3g}")


def intact(g):
    return bool(np.all(g == g.dtype.type(cr.SENTINEL if g.dtype.kind == "f" else -7)))


# ---- assemble -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("off", [0, 5])
@pytest.mark.parametrize("nagg", cr.ASM_NAGG)
def test_assemble(nagg, off, transpose):
    """diagScale 1 and 0.5: bitwise the sequential float64 sum; 0.7: (T + 1) u sum |terms|; rows of aggregates without a row cell exactly 0"""
    c = cr.assemble_case(nagg, off, transpose)
    empty = np.setdiff1d(np.arange(nagg), c["aggRow"])
    for ds in (1.0, 0.5, 0.7):
        E, g = twice(lambda: cr.dev_assemble(_capi.lib(), c, ds))
        assert intact(g), "guard behind E"
        ref, mag, T = cr.ref_assemble(c, ds, LD)
        ok, ratio = cr.check_assemble(E, ref, mag, T)
        record(f"k_coarse_assemble diagScale {ds}", ratio)
        assert ok, f"diagScale {ds}: {ratio} of the bound"
        if ds != 0.7:
            assert cr.same(E, cr.ref_assemble(c, ds)[0]), f"diagScale {ds}: not the sequential sum in list and storage order"
        rows = E.T if transpose else E
        assert np.all(rows[empty] == 0.0) and not np.any(np.signbit(rows[empty]))
    if nagg >= 3:
        assert len(empty) >= 1 and np.count_nonzero(c["aggRow"] == nagg - 1) == 1


@pytest.mark.parametrize("transpose", [0, 1])
def test_assemble_moved_diagonal(transpose):
    """the twin differs only in which entry of one row is the diagonal: E differs in the entries those two positions feed, and nowhere else"""
    c = cr.assemble_case(257, 5, transpose)
    twin, fed = cr.move_diagonal(c)
    (E1, _), (E2, _) = twice(lambda: cr.dev_assemble(_capi.lib(), c, 0.5)), twice(lambda: cr.dev_assemble(_capi.lib(), twin, 0.5))
    assert cr.same(E1, cr.ref_assemble(c, 0.5)[0]) and cr.same(E2, cr.ref_assemble(twin, 0.5)[0])
    diff = set(zip(*np.nonzero(E1 != E2)))
    assert diff == set(fed), (diff, fed)


# ---- invert -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cr.INV_N)
def test_invert_exact(n):
    A = cr.invert_matrix(n, "exact")
    Inv, sing, g = twice(lambda: cr.dev_invert(_capi.lib(), A))
    assert sing == 0 and intact(g)
    assert cr.same(Inv, cr.exact_inverse(A))


@functools.lru_cache(maxsize=None)
def inverse_refs(n, kind):
    A = cr.invert_matrix(n, kind)
    ref = cr.gauss_jordan(A, LD)[0]
    return A, ref, cr.inverse_error(cr.gauss_jordan(A)[0], ref)


@pytest.mark.parametrize("kind", ["dominant", "permuted"])
@pytest.mark.parametrize("n", cr.INV_N)
def test_invert(n, kind):
    """e_dev <= 4 e_ref against the longdouble elimination with the same pivot rule; a missed pivot of "permuted" costs 1e3 and more"""
    A, ref, e_ref = inverse_refs(n, kind)
    Inv, sing, g = twice(lambda: cr.dev_invert(_capi.lib(), A))
    assert sing == 0 and intact(g) and np.all(np.isfinite(Inv))
    e_dev = cr.inverse_error(Inv, ref)
    ratio = e_dev / e_ref if e_ref > 0 else (0.0 if e_dev == 0 else np.inf)
    record(f"k_gj_pivot + k_gj_elim {kind} e_dev / e_ref", ratio)
    print(f"n = {n} {kind}: e_dev = {e_dev:.3g}, e_ref = {e_ref:.3g}")
    assert e_dev <= 4.0 * e_ref


@pytest.mark.parametrize("which", list(cr.singular_matrices()))
def test_invert_singular_flag(which):
    A, flag = cr.singular_matrices()[which]
    Inv, sing, g = twice(lambda: cr.dev_invert(_capi.lib(), A))
    assert sing == flag and intact(g)
    assert cr.gauss_jordan(A)[1] == flag


# ---- restrict, solve, prolong -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("set_", [1, 0])
@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("off", [0, 5])
def test_correct(off, kind, set_):
    c = cr.correct_case(off, kind)
    n, nagg = c["n"], c["nagg"]
    y0 = np.concatenate([kr.vector(n, [21, off]), np.full(7, cr.SENTINEL)])
    t, u, y = twice(lambda: cr.dev_correct(_capi.lib(), c, y0, set_))
    assert intact(t[nagg:]) and intact(u[nagg:]) and cr.guard_intact(y, n)
    t, u = t[:nagg], u[:nagg]
    ok, ratio = cr.check_restrict(t, *cr.ref_restrict(c))
    record(f"k_coarse_restrict {kind}", ratio)
    assert ok, ratio
    assert t[cr.COR_SIZES.index(0)] == 0.0 and t[cr.COR_SIZES.index(1)] == c["r"][off + np.flatnonzero(c["agg"] == cr.COR_SIZES.index(1))[0]]
    ok, ratio = cr.check_solve(u, c["Einv"], t)
    record(f"k_coarse_solve {kind}", ratio)
    assert ok, ratio
    assert cr.same(y, cr.ref_prolong(c, u, y0, set_))
    away = np.ones(n, dtype=bool)
    away[off + np.flatnonzero(c["agg"] >= 0)] = False
    assert away.sum() >= 40 + off + 7
    if set_:
        assert np.all(y[:n][away] == 0.0) and not np.any(np.signbit(y[:n][away]))
    else:
        assert cr.same(y[:n][away], y0[:n][away])


@pytest.mark.parametrize("set_", [1, 0])
def test_correct_poisoned(set_):
    """a NaN in one r entry of the 65-cell aggregate, block-diagonal Einv (see the head of the file for what IEEE makes of it)"""
    c = cr.correct_case(5, "well")
    n, off, nagg, agg = c["n"], c["off"], c["nagg"], c["agg"]
    I = cr.COR_SIZES.index(65)
    r = c["r"].copy()
    r[off + np.flatnonzero(agg == I)[64]] = np.nan
    Einv = np.zeros((nagg, nagg))
    for b in range(0, nagg, 3):
        Einv[b:b + 3, b:b + 3] = c["Einv"][b:b + 3, b:b + 3]
    y0 = np.concatenate([kr.vector(n, [22]), np.full(7, cr.SENTINEL)])
    t, u, y = twice(lambda: cr.dev_correct(_capi.lib(), c, y0, set_, r=r, Einv=Einv))
    t, u = t[:nagg], u[:nagg]
    assert not np.isfinite(t[I]) and np.all(np.isfinite(np.delete(t, I)))
    clean = cr.ref_restrict(c)
    assert cr.check_restrict(np.delete(t, I), *(np.delete(a, I) for a in clean))[0]
    with np.errstate(invalid="ignore"):
        u64 = np.array([np.sum(Einv[q] * t) for q in range(nagg)])
    assert np.array_equal(np.isfinite(u), np.isfinite(u64)) and not np.any(np.isfinite(u))
    live = np.zeros(n, dtype=bool)
    live[off + np.flatnonzero(agg >= 0)] = True
    assert not np.any(np.isfinite(y[:n][live])) and cr.guard_intact(y, n)
    assert cr.same(y[:n][~live], (np.zeros(n) if set_ else y0[:n])[~live])


# ---- the sparse A Z -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_vec", [True, False])
@pytest.mark.parametrize("off", [0, 5])
def test_az_build_and_apply(off, use_vec):
    c = cr.az_case(off)
    n = c["n"]
    rcnt, rptr, roa, rov, rovf = cr.ref_az_build(c)
    assert rovf == 0 and n % 256 and set(cr.AZ_TOUCH) <= set(rcnt.tolist())
    cap = int(rptr[-1]) + 5
    cnt, ptr, oa, ov, nnz, ovf, out = twice(lambda: cr.dev_az(_capi.lib(), c, use_vec, cap))
    assert ovf == 0 and nnz == rptr[-1]
    assert cr.same(cnt[:n], rcnt) and intact(cnt[n:]) and cr.same(ptr[: n + 1], rptr) and intact(ptr[n + 1:])
    assert cr.same(oa[:nnz], roa), "aggregates of a row: not in the order of their first appearance"
    assert cr.same(ov[:nnz], rov) and intact(ov[nnz:]) and intact(oa[nnz:])
    vec = c["vec"] if use_vec else None
    ref, mag, T = cr.ref_az_apply(rptr, roa, rov, c["u"], vec)
    ok, ratio = cr.check_az_apply(out[:n], ref, mag, T)
    record("k_az_apply " + ("v - (A Z) u" if use_vec else "(A Z) u"), ratio)
    assert ok and cr.guard_intact(out, n), ratio
    none = np.flatnonzero(rcnt == 0)
    assert len(none) and cr.same(out[:n][none], c["vec"][none] if use_vec else np.zeros(len(none)))


@pytest.mark.parametrize("off", [0, 5])
def test_az_overflow_at_65_aggregates(off):
    """the same matrix with one 64-aggregate row extended by a 65th: overflow, and nothing is written"""
    c = cr.az_case(off, extend=True)
    assert cr.ref_az_build(c)[4] == 1 and cr.ref_az_build(cr.az_case(off))[0][c["extended"]] == 64
    cnt, ptr, oa, ov, nnz, ovf, out = twice(lambda: cr.dev_az(_capi.lib(), c, True, 4096))
    assert ovf == 1 and nnz == -7
    assert intact(cnt) and intact(ptr) and intact(oa) and intact(ov) and intact(out)


def test_zzz_print_achieved_ratios(capsys):
    """the achieved max err / bound (1 = the bound; e_dev / e_ref: 4 = the bound) of everything that ran in this module"""
    with capsys.disabled():
        print("\n| kernel | max err / bound |\n|---|---|")
        for name in sorted(RATIOS):
            print(f"| {name} | {RATIOS[name]:.3g} |")
    assert all(r <= (4.0 if "e_ref" in name else 1.0) for name, r in RATIOS.items())

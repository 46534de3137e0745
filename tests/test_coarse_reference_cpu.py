"""CPU tier of tests/coarse_reference.py: the restatements of the coarse-space kernels against INDEPENDENT dense numpy (Z^T A Z,
numpy.linalg.inv, A @ Z), the generators against what the GPU tests rely on (the sizes, a pivot 256 rows below the diagonal, the cap on
the condition number, 64 against 65 aggregates in a row), the float64 restatements inside every stated bound and named wrong results
outside - so that a pass of tests/test_gpu_coarse_kernels.py means something - and every invalid input refused by the entries
das_debug_coarse_* with DAS_ERR_ARG before anything is launched (these run without a device)."""
import numpy as np
import pytest

import coarse_reference as cr
import graph_reference as gr
from dafoam_amd import _capi

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")
ARG = -1  # DAS_ERR_ARG
LD = cr.LD


def dense(n, rp, ci, v):
    A = np.zeros((n, n), dtype=LD)
    np.add.at(A, (gr.rows_of(rp), ci), v.astype(LD))
    return A


def indicator(agg, nagg, off, n):
    Z = np.zeros((n, nagg), dtype=LD)
    live = np.flatnonzero(agg >= 0)
    Z[off + live, agg[live]] = 1
    return Z


# ---- assemble -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transpose", [0, 1])
@pytest.mark.parametrize("nagg", [2, 257, 2048])
def test_assemble_against_dense_zt_a_z(nagg, transpose):
    c = cr.assemble_case(nagg, 5, transpose)
    n, off, N = c["n"], c["off"], c["N"]
    for ds in (1.0, 0.7):
        # the scale belongs to the entries, not to their sum: scale the diagonal entries one by one.  Dense products in float64 (BLAS):
        # the zeros of Z add nothing, so the error of an entry is that of its T terms in some order
        rows, cols = gr.rows_of(c["rp"]), c["ci"]
        A = np.zeros((n, n))
        np.add.at(A, (rows, cols), np.where(rows == cols, c["v"] * ds, c["v"]))
        E = indicator(c["aggRow"], nagg, off, n).astype(np.float64).T @ A @ indicator(c["aggCol"], nagg, off, n).astype(np.float64)
        ref, mag, T = cr.ref_assemble(c, ds, LD)
        if transpose:
            E = E.T
        assert np.all(np.abs(E.astype(LD) - ref) <= 4 * (T + 2) * LD(cr.U) * mag) and np.all(E[T == 0] == 0.0)
        ok, ratio = cr.check_assemble(cr.ref_assemble(c, ds)[0], ref, mag, T)
        assert ok and ratio <= 1.0, ratio


@pytest.mark.parametrize("off", [0, 5])
@pytest.mark.parametrize("nagg", cr.ASM_NAGG)
def test_assemble_generator(nagg, off):
    c = cr.assemble_case(nagg, off, 0)
    N, n, rp, ci = c["N"], c["n"], c["rp"], c["ci"]
    assert n == off + N + 7 and 2000 <= N <= 2200
    lens = np.diff(rp)
    assert lens.min() == 0 and lens.max() == 12
    assert np.any(ci >= off + N) and (off == 0 or np.any(ci < off))
    r, cc = c["aggRow"], c["aggCol"]
    assert 0.03 * N <= np.count_nonzero(r < 0) <= 0.06 * N and 0.04 * N <= np.count_nonzero(cc < 0) <= 0.06 * N and not np.any((r < 0) & (cc < 0))
    assert r.min() >= -1 and r.max() < nagg and cc.min() >= -1 and cc.max() < nagg
    I, J, k, dg = cr.assemble_terms(c)
    assert np.any(dg) and not np.all(dg)
    T = cr.ref_assemble(c, 1.0)[2]
    assert T.max() >= 2, "no aggregate pair with two terms: the order of a sum would not show"
    if nagg >= 3:
        assert len(np.setdiff1d(np.arange(nagg), r)) >= 1 and np.count_nonzero(r == nagg - 1) == 1
    if nagg > 256:
        assert np.any(J >= 256) and np.any(I >= 256)
    t = cr.assemble_case(nagg, off, 1)
    assert t["aggCol"] is t["aggRow"]


def test_assemble_rejects_a_wrong_stride_and_a_scaled_row():
    """named wrong results: the columns J >= 256 of a row left out (a stride that stops after one trip), and diagScale on every entry of
    the diagonal's row"""
    c = cr.assemble_case(513, 5, 0)
    ref, mag, T = cr.ref_assemble(c, 0.5, LD)
    good = cr.ref_assemble(c, 0.5)[0]
    bad = good.copy()
    bad[:, 256:] = 0.0
    assert cr.check_assemble(good, ref, mag, T)[0] and not cr.check_assemble(bad, ref, mag, T)[0]
    assert not cr.check_assemble(cr.ref_assemble(c, 1.0)[0], ref, mag, T)[0]
    twin, fed = cr.move_diagonal(c)
    E2 = cr.ref_assemble(twin, 0.5)[0]
    assert set(zip(*np.nonzero(good != E2))) == set(fed) and len(fed) == 2


# ---- invert -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dominant", "permuted", "exact"])
@pytest.mark.parametrize("n", cr.INV_N)
def test_elimination_against_numpy_inverse(n, kind):
    A = cr.invert_matrix(n, kind)
    Inv, sing, piv = cr.gauss_jordan(A)
    assert sing == 0 and np.linalg.cond(A) <= 1.0e4
    ref = np.linalg.inv(A)
    assert np.max(np.abs(Inv - ref)) <= 1.0e-11 * np.max(np.abs(ref))
    if kind == "permuted" and n >= 257:
        assert np.any(piv - np.arange(n) >= 256)
        # the search that stops after its first stride picks an entry of the 1e-3 R part and loses three digits and more
        a = np.abs(A[:, 0])
        assert np.argmax(a) >= 256 and a[:256].max() <= 1.0e-2 * a.max()
    if kind == "permuted" and n >= 2:
        assert np.any(piv != np.arange(n))
    if kind == "exact":
        assert cr.same(Inv, cr.exact_inverse(A)) and cr.same(cr.gauss_jordan(A, fused=True)[0], Inv)
        if n >= 3:
            assert np.any(piv != np.arange(n))


@pytest.mark.parametrize("kind", ["dominant", "permuted"])
@pytest.mark.parametrize("n", cr.INV_N[:-1])
def test_fused_elimination_stays_inside_four_e_ref(n, kind):
    """the device may fuse a - f b: a float64 restatement with every such update rounded once stays inside the bound of the GPU test
    (513 left out: two more longdouble eliminations of that size take 10 s)"""
    A = cr.invert_matrix(n, kind)
    ref = cr.gauss_jordan(A, LD)[0]
    e_ref, e_fused = cr.inverse_error(cr.gauss_jordan(A)[0], ref), cr.inverse_error(cr.gauss_jordan(A, fused=True)[0], ref)
    print(f"n = {n} {kind}: e_ref = {e_ref:.3g}, fused / e_ref = {e_fused / e_ref if e_ref else 0:.3g}")
    assert e_fused <= 4.0 * e_ref


def test_elimination_without_the_second_stride_is_rejected():
    """pivot search over the first 256 rows only, on "permuted" 257: at least 1e3 times the error of the restatement"""
    A = cr.invert_matrix(257, "permuted")
    ref = cr.gauss_jordan(A, LD)[0]
    e_ref = cr.inverse_error(cr.gauss_jordan(A)[0], ref)
    W = np.concatenate([A, np.eye(257)], axis=1)
    for k in range(257):
        pr = k + int(np.argmax(np.abs(W[k:k + 256, k])))
        W[[k, pr]] = W[[pr, k]]
        W[k] = W[k] / W[k, k]
        f = W[:, k].copy()
        f[k] = 0
        W -= f[:, None] * W[k][None, :]
    assert cr.inverse_error(W[:, 257:], ref) > 4.0 * e_ref


def test_singular_matrices():
    for which, (A, flag) in cr.singular_matrices().items():
        assert cr.gauss_jordan(A)[1] == flag and cr.gauss_jordan(A, LD)[1] == flag, which
        if flag and not np.any(np.isnan(A)):
            assert np.linalg.matrix_rank(A) < A.shape[0], which


# ---- restrict, solve, prolong -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("off", [0, 5])
def test_correct_against_dense_z(off, kind):
    c = cr.correct_case(off, kind)
    n, N, nagg, agg = c["n"], c["N"], c["nagg"], c["agg"]
    assert [int(np.count_nonzero(agg == q)) for q in range(nagg)] == cr.COR_SIZES and np.count_nonzero(agg < 0) == 40 and n == off + N + 7
    Z = indicator(agg, nagg, off, n)
    t, mag, T = cr.ref_restrict(c)
    assert np.all(np.abs(Z.T @ c["r"].astype(LD) - t) <= T * LD(2.0) ** -63 * mag) and list(T) == cr.COR_SIZES
    t64 = cr.restrict64(c)
    ok, ratio = cr.check_restrict(t64, t, mag, T)
    assert ok and ratio <= 1.0
    bad = t64.copy()
    q = cr.COR_SIZES.index(257)
    bad[q] -= c["r"][off + np.flatnonzero(agg == q)[256]]  # the 257th cell: the second trip of the 256-thread stride
    assert not cr.check_restrict(bad, t, mag, T)[0]
    u64 = c["Einv"] @ t64
    assert cr.check_solve(u64, c["Einv"], t64)[0]
    ubad = u64 - c["Einv"][:, -1] * t64[-1]
    assert not cr.check_solve(ubad, c["Einv"], t64)[0]
    y0 = np.concatenate([np.arange(1.0, n + 1.0), np.full(7, cr.SENTINEL)])
    for set_ in (0, 1):
        y = cr.ref_prolong(c, u64, y0, set_)
        assert cr.guard_intact(y, n)
        assert np.array_equal(y[:n], (0 if set_ else y0[:n]) + (Z @ u64.astype(LD)).astype(np.float64))


# ---- the sparse A Z -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 5])
def test_az_against_dense_a_z(off):
    c = cr.az_case(off)
    n, nagg = c["n"], c["nagg"]
    cnt, ptr, oa, ov, ovf = cr.ref_az_build(c)
    assert ovf == 0 and n % 256 and n > 256
    assert np.array_equal(cnt, c["touch"]) and set(cnt.tolist()) == set(cr.AZ_TOUCH)
    A = dense(n, c["rp"], c["ci"], c["v"])
    AZ = A @ indicator(c["agg"], nagg, off, n)
    S = np.zeros((n, nagg), dtype=LD)
    S[gr.rows_of(ptr), oa] = ov.astype(LD)
    rl = np.diff(c["rp"])
    assert np.all(np.abs(S - AZ) <= rl[:, None] * LD(2.0) ** -53 * (np.abs(A) @ indicator(c["agg"], nagg, off, n)))
    for i in range(n):
        assert len(set(oa[ptr[i]:ptr[i + 1]])) == cnt[i]
    # first appearance: the order differs from the ascending one, aggregates repeat, rows hold columns of no aggregate and outside the field
    assert any(np.any(np.diff(oa[ptr[i]:ptr[i + 1]]) < 0) for i in range(n))
    j = c["ci"].astype(np.int64) - off
    infield = (j >= 0) & (j < c["N"])
    assert np.any(~infield) and np.any(c["agg"][j[infield]] < 0)
    assert np.any((cnt == 0) & (rl > 0)) and np.any((cnt == 0) & (rl == 0)) and int(rl.sum()) > int(cnt.sum()) + 100
    for vec in (c["vec"], None):
        ref, mag, T = cr.ref_az_apply(ptr, oa, ov, c["u"], vec)
        dense_out = (0 if vec is None else vec.astype(LD)) - AZ @ c["u"].astype(LD) * (1 if vec is not None else -1)
        assert np.all(np.abs(dense_out - ref) <= (rl + 2) * LD(2.0) ** -52 * mag)
        o64 = cr.az_apply64(ptr, oa, ov, c["u"], vec)
        ok, ratio = cr.check_az_apply(o64, ref, mag, T)
        assert ok and ratio <= 1.0
        bad = o64.copy()
        i = int(np.flatnonzero(cnt == 64)[0])
        bad[i] += ov[ptr[i + 1] - 1] * c["u"][oa[ptr[i + 1] - 1]]  # the 64th aggregate of a row dropped
        assert not cr.check_az_apply(bad, ref, mag, T)[0]


@pytest.mark.parametrize("off", [0, 5])
def test_az_64_against_65_aggregates(off):
    c, x = cr.az_case(off), cr.az_case(off, extend=True)
    i = c["extended"]
    assert cr.ref_az_build(c)[0][i] == 64 and cr.ref_az_build(c)[4] == 0 and cr.ref_az_build(x)[4] == 1
    assert len(x["ci"]) == len(c["ci"]) + 1 and x["rp"][i + 1] == c["rp"][i + 1] + 1
    j = x["ci"][x["rp"][i]:x["rp"][i + 1]].astype(np.int64) - off
    j = j[(j >= 0) & (j < x["N"])]
    assert len(set(x["agg"][j][x["agg"][j] >= 0])) == 65


# ---- the entries refuse what they cannot index with -----------------------------------------------------------------------------------
def small():
    """5 unknowns, the field = the unknowns 1 .. 3, two aggregates"""
    rp = np.array([0, 2, 4, 5, 7, 8], dtype=np.int64)
    ci = np.array([0, 1, 1, 2, 2, 1, 3, 4], dtype=np.int32)
    v = np.arange(1.0, 9.0)
    agg = np.array([0, 1, -1], dtype=np.int32)
    return dict(nagg=2, N=3, off=1, n=5, rp=rp, ci=ci, v=v, aggRow=agg, aggCol=agg, agg=agg, transpose=0, Einv=np.eye(2), r=np.arange(1.0, 6.0),
                u=np.ones(2), vec=np.ones(5))


def bad_inputs(c, aggs):
    """(what, overrides) common to the entries with a field block (and a CSR structure when rp is among the keys asked for)"""
    out = [("nagg = 0", dict(nagg=0)), ("nagg = 2049", dict(nagg=2049)), ("nagg negative", dict(nagg=-1)), ("off + N > n", dict(N=5)), ("off + N > n", dict(off=3)),
           ("off negative", dict(off=-1)), ("N = 0", dict(N=0)), ("n = 0", dict(n=0))]
    for key in aggs:
        for what, val in [("agg = nagg", 2), ("agg = -2", -2)]:
            a = c[key].copy()
            a[1] = val
            out.append((f"{key}: {what}", {key: a}))
        out.append((f"{key}: null", {key: None}))
    return out


def bad_csr(c):
    out = []
    ci = c["ci"].copy(); ci[4] = 5; out.append(("column too large", dict(ci=ci)))
    ci = c["ci"].copy(); ci[4] = -1; out.append(("column negative", dict(ci=ci)))
    rp = c["rp"].copy(); rp[2] = 1; out.append(("rowptr decreases", dict(rp=rp)))
    rp = c["rp"].copy(); rp[0] = 1; out.append(("rowptr[0] != 0", dict(rp=rp)))
    return out + [("null rowptr", dict(rp=None)), ("null col", dict(ci=None)), ("null values", dict(v=None))]


def test_entries_refuse_invalid_input_before_any_launch():
    L = _capi.lib()
    c = small()

    def refused(rc, who, what):
        assert rc == ARG and who in L.das_last_error(), (who, what, rc, L.das_last_error())

    who = b"das_debug_coarse_assemble"
    for what, over in bad_inputs(c, ["aggRow", "aggCol"]) + bad_csr(c) + [("transpose = 2", dict(transpose=2))]:
        rc, E, g = cr.dev_assemble(L, c, 1.0, **over)
        refused(rc, who, what)
        assert np.all(E == cr.SENTINEL)
    refused(cr.dev_assemble(L, c, 1.0, null_E=True)[0], who, "null E")
    who = b"das_debug_coarse_invert"
    A = np.eye(3)
    for what, n in [("n = 0", 0), ("n = 2049", 2049), ("n negative", -1)]:
        refused(cr.dev_invert(L, A, n)[0], who, what)
    sing = cr.C.c_int(0)
    refused(L.das_debug_coarse_invert(3, None, cr._d(np.zeros(17)), cr.C.byref(sing)), who, "null Ein")
    refused(L.das_debug_coarse_invert(3, cr._d(A), None, cr.C.byref(sing)), who, "null Inv")
    refused(L.das_debug_coarse_invert(3, cr._d(A), cr._d(np.zeros(17)), None), who, "null singular")
    who = b"das_debug_coarse_correct"
    y0 = np.full(9, cr.SENTINEL)
    for what, over in bad_inputs(c, ["agg"]) + [("null Einv", dict(Einv=None)), ("null r", dict(r=None)), ("set = 2", dict(set_=2))]:
        set_ = over.pop("set_", 1)
        rc, t, u, y = cr.dev_correct(L, c, y0, set_, **over)
        refused(rc, who, what)
        assert np.all(y == cr.SENTINEL) and np.all(t == cr.SENTINEL)
    refused(cr.dev_correct(L, c, y0[:4], 1)[0], who, "y shorter than n")
    refused(L.das_debug_coarse_correct(2, 3, 1, 5, cr._i(c["agg"]), cr._d(c["Einv"]), cr._d(c["r"]), None, None, None, 9, 1), who, "null outputs")
    who = b"das_debug_coarse_az"
    for what, over in bad_inputs(c, ["agg"]) + bad_csr(c) + [("null u", dict(u=None))]:
        out = cr.dev_az(L, c, True, 16, **over)
        refused(out[0], who, what)
        assert out[5] == -7 and out[6] == -7 and np.all(out[7] == cr.SENTINEL)
    refused(cr.dev_az(L, c, True, 4)[0], who, "oa / ov shorter than the entries")     # the sparse A Z of small() holds 5 entries
    assert cr.ref_az_build(c)[1][-1] == 5
    refused(cr.dev_az(L, c, True, 0)[0], who, "cap = 0")
    refused(cr.dev_az(L, c, True, 16, guard=-1)[0], who, "out shorter than n")
    refused(L.das_debug_coarse_az(2, 5, cr._ll(c["rp"]), cr._i(c["ci"]), cr._d(c["v"]), 3, 1, cr._i(c["agg"]), None, None, None, None, 16, None, None, cr._d(c["u"]), None,
                                  None, 5), who, "null outputs")

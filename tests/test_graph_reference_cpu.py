"""CPU tier of tests/graph_reference.py: the restatements of the graph set-up, the filter and the pack against INDEPENDENT ones (a
dense boolean matrix, a brute-force double loop, a round trip), the generators against what they promise, a float64 restatement with
another summation order accepted by the product comparison, every named wrong result rejected - so that a pass of
tests/test_gpu_graph_kernels.py and tests/test_gpu_opmat_kernels.py means something - and every invalid input refused by the entries
das_debug_graph_* / das_debug_compact / das_debug_vecpack / das_debug_spmv_rows with DAS_ERR_ARG before anything is launched (these
run without a device)."""
import functools

import numpy as np
import pytest

import graph_reference as gr
import krylov_reference as kr
from dafoam_amd import _capi

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")
ARG = -1  # DAS_ERR_ARG


@functools.lru_cache(maxsize=None)
def transposed():
    n, rp, ci, lens = gr.transpose_pattern()
    return (n, rp, ci, lens) + gr.ref_transpose(rp, ci)[:2]


@functools.lru_cache(maxsize=None)
def packed(kind="well"):
    row0, nG, ntail, shift = gr.PACK_SHAPES[3]
    n, rp, ci, v, x = gr.pack_matrix(row0, nG, ntail, 3, kind, shift)
    built, cptr, chunks = gr.ref_pack(rp, ci, v, row0, nG)
    assert built
    return row0, nG, n, rp, ci, v, x, cptr, chunks


# ---- the restatements against independent ones ---------------------------------------------------------------------------------
def test_transpose_against_a_dense_boolean_matrix():
    n, rp, ci, lens, trp, tcol = transposed()
    D = np.zeros((n, n), dtype=bool)
    D[gr.rows_of(rp), ci] = True
    assert D.sum() == rp[-1], "the generator repeats an entry"
    assert np.all(np.diff(ci)[np.diff(gr.rows_of(rp)) == 0] > 0), "the columns of a row do not ascend strictly"
    for j in range(n):
        assert np.array_equal(tcol[trp[j]:trp[j + 1]], np.flatnonzero(D[:, j]))
    assert np.array_equal(np.diff(trp), lens) and lens[0] == 0 and lens[-1] == 0 and n % 4 and n % 16
    assert set(gr.TR_LENGTHS_SHORT + gr.TR_LENGTHS_LONG) <= set(lens.tolist()) and lens.max() > gr.SORT_MAX + 500


@pytest.mark.parametrize("which", ["none", "all", "every_other", "lane15", "lane0"])
def test_nets_against_a_brute_force_double_loop(which):
    n, rp, ci = gr.nets_pattern()
    keep = gr.nets_keeps(n, rp, ci)[which]
    cptr, crow, cpos, isStart = gr.ref_nets(rp, ci, keep)
    net = {int(r): q for q, r in enumerate(keep)}
    lists = []
    for j in range(n):
        lst = []
        for r in range(n):
            row = list(ci[rp[r]:rp[r + 1]])
            if j in row and r in net:
                lst.append((net[r], row.index(j)))
        lists.append(lst)
        assert [(int(a), int(b)) for a, b in zip(crow[cptr[j]:cptr[j + 1]], cpos[cptr[j]:cptr[j + 1]])] == lst
    assert [int(f) for f in isStart] == [1] + [0 if [a for a, _ in lists[j]] == [a for a, _ in lists[j - 1]] else 1 for j in range(1, n)]


def test_nets_generator_holds_the_named_cases():
    n, rp, ci = gr.nets_pattern()
    trp, tcol, _ = gr.ref_transpose(rp, ci)
    assert set(gr.NET_LENGTHS) <= set(np.diff(trp).tolist()) and n % 16
    K = gr.nets_keeps(n, rp, ci)
    cptr, crow, cpos, isStart = gr.ref_nets(rp, ci, K["all"])
    # both empty; identical lists; equal length and another last net
    assert list(isStart[:5]) == [1, 0, 1, 0, 1] and list(isStart[8:13]) == [1, 0, 1, 1, 0]
    assert cptr[4] - cptr[3] == cptr[5] - cptr[4] == 16 and np.array_equal(crow[cptr[3]:cptr[4]][:-1], crow[cptr[4]:cptr[5]][:-1])
    # the 16-lane prefix of column 8: only the last lane kept in two steps and nothing in the third; only lane 0 kept in three steps
    t8 = tcol[trp[8]:trp[9]]
    for which, lanes in (("lane15", [15, 31]), ("lane0", [0, 16, 32])):
        kept = np.isin(t8, K[which])
        assert list(np.flatnonzero(kept)) == lanes


def test_pack_round_trips_to_the_csr_rows():
    for row0, nG, ntail, shift in gr.PACK_SHAPES:
        n, rp, ci, v, x = gr.pack_matrix(row0, nG, ntail, 3, "ill", shift)
        built, cptr, chunks = gr.ref_pack(rp, ci, v, row0, nG)
        lens = np.diff(rp)[row0:row0 + 3 * nG:3]
        assert built and np.array_equal(np.diff(cptr), (lens + 15) // 16) and chunks.tobytes().__len__() == 448 * cptr[-1]
        for g, (cols, vals) in enumerate(gr.unpack(cptr, chunks, lens)):
            r = row0 + 3 * g
            assert np.array_equal(cols, ci[rp[r]:rp[r + 1]])
            for d in range(3):
                assert gr.same(vals[d], v[rp[r + d]:rp[r + d + 1]])
        # the pads: the last valid column again, +0.0 (all bits zero)
        for g in range(nG):
            if lens[g] % 16:
                last = chunks[cptr[g + 1] - 1]
                assert np.all(last["col"][lens[g] % 16:] == ci[rp[row0 + 3 * g + 1] - 1]) and not np.any(last["val"][:, lens[g] % 16:].view(np.uint64))
    lens_all = set()
    for row0, nG, ntail, shift in gr.PACK_SHAPES:
        lens_all |= {gr.PACK_LENGTHS[(g + shift) % 17] for g in range(nG)}
    assert lens_all == set(gr.PACK_LENGTHS)


def test_mismatch_generator_breaks_exactly_one_group():
    for g in (0, 20):
        for what in ("len", 0, 5, -1):
            n, rp, ci, v, x = gr.pack_matrix(5, 33, 14, 3, "well", 4, break_at=(g, what))
            assert not gr.ref_pack(rp, ci, v, 5, 33)[0]
            # every other group still shares its list
            for h in range(33):
                r = 5 + 3 * h
                ok = np.array_equal(ci[rp[r]:rp[r + 1]], ci[rp[r + 1]:rp[r + 2]]) and np.array_equal(ci[rp[r]:rp[r + 1]], ci[rp[r + 2]:rp[r + 3]])
                assert ok == (h != g)


# ---- the product comparison: accepts another order in float64, rejects the named wrong results ------------------------------------
@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("shape", gr.PACK_SHAPES)
def test_float64_restatement_in_another_order_is_accepted(shape, kind):
    row0, nG, ntail, shift = shape
    n, rp, ci, v, x = gr.pack_matrix(row0, nG, ntail, 3, kind, shift)
    built, cptr, chunks = gr.ref_pack(rp, ci, v, row0, nG)
    ref, mag, lens = gr.ref_product(rp, ci, v, x)
    y = gr.csr_product64(rp, ci, v, x)
    assert gr.check_product(y, ref, mag, lens)[0]
    y[row0:row0 + 3 * nG] = gr.pack_product64(cptr, chunks, x).reshape(-1)
    ok, ratio = gr.check_product(y, ref, mag, lens)
    assert ok and ratio <= 1.0 and np.all(y[lens == 0] == 0.0)


def test_wrong_packs_and_products_are_rejected():
    row0, nG, n, rp, ci, v, x, cptr, chunks = packed()
    ref, mag, lens = gr.ref_product(rp, ci, v, x)
    sl = slice(row0, row0 + 3 * nG)

    def ok(y_groups):
        return gr.check_product(np.asarray(y_groups).reshape(-1), ref[sl], mag[sl], lens[sl])[0]

    good = gr.pack_product64(cptr, chunks, x)
    assert ok(good)
    glen = lens[sl][::3]
    g = int(np.flatnonzero(glen % 16 == 1)[0])  # a group whose last chunk holds one entry and fifteen pads
    # nonzero pad values
    bad = chunks.copy()
    bad[cptr[g + 1] - 1]["val"][:, 5] = 1.0
    assert not gr.same(bad, chunks) and not ok(gr.pack_product64(cptr, bad, x))
    # value planes 1 and 2 swapped
    bad = chunks.copy()
    bad["val"][:, [1, 2], :] = chunks["val"][:, [2, 1], :]
    assert not gr.same(bad, chunks) and not ok(gr.pack_product64(cptr, bad, x))
    # the last chunk dropped from the product
    assert not ok(gr.pack_product64(cptr, chunks, x, skip_last_chunk_of=g))
    # a row0 shift of one: y of the group rows written one row further
    y = gr.csr_product64(rp, ci, v, x)
    assert gr.check_product(y, ref, mag, lens)[0]
    shifted = y.copy()
    shifted[row0 + 1:row0 + 3 * nG + 1] = good.reshape(-1)
    assert not gr.check_product(shifted, ref, mag, lens)[0]
    # one value truncated to fp32
    bad = chunks.copy()
    c = cptr[int(np.flatnonzero(glen == 280)[0])] + 3
    a = bad[c]["val"][1, 7]
    assert float(np.float32(a)) != a
    bad[c]["val"][1, 7] = np.float32(a)
    assert not ok(gr.pack_product64(cptr, bad, x))


@pytest.mark.parametrize("what", [np.nan, np.inf])
def test_foreign_pad_columns_show_only_with_a_poisoned_x(what):
    """Pad columns taken from the next group row with zero values: invisible with a finite x - the comparison ACCEPTS it - and the
    reason the poisoned x exists: there the comparison rejects it."""
    row0, nG, n, rp, ci, v, x, _, _ = packed()
    ci2, p, dirty = gr.poison_groups(row0, nG, rp, ci)
    built, cptr, chunks = gr.ref_pack(rp, ci2, v, row0, nG)
    assert built and 0 < dirty.sum() < n
    sl = slice(row0, row0 + 3 * nG)
    glen = np.diff(rp)[sl][::3]
    bad, hit = chunks.copy(), 0
    for g in range(nG - 1):
        if glen[g] % 16 and glen[g + 1] and not dirty[row0 + 3 * g]:
            bad[cptr[g + 1] - 1]["col"][glen[g] % 16:] = ci2[rp[row0 + 3 * g + 3]]
            hit += int(ci2[rp[row0 + 3 * g + 3]] == p)
    assert hit > 0 and not gr.same(bad, chunks), "no clean group is followed by a group that starts with the poisoned column"
    ref, mag, lens = gr.ref_product(rp, ci2, v, x)
    assert gr.check_product(gr.pack_product64(cptr, bad, x).reshape(-1), ref[sl], mag[sl], lens[sl])[0], "finite x: the wrong pads must be invisible"
    xp = x.copy()
    xp[p] = what
    assert gr.check_poisoned(gr.pack_product64(cptr, chunks, xp).reshape(-1), ref[sl], mag[sl], lens[sl], dirty[sl])[0]
    assert not gr.check_poisoned(gr.pack_product64(cptr, bad, xp).reshape(-1), ref[sl], mag[sl], lens[sl], dirty[sl])[0]
    # the scalar rows: the float64 restatement is accepted, a row that misses its poison is not
    y = gr.csr_product64(rp, ci2, v, xp)
    assert gr.check_poisoned(y, ref, mag, lens, dirty)[0]
    y[np.flatnonzero(dirty)[0]] = 0.0
    assert not gr.check_poisoned(y, ref, mag, lens, dirty)[0]


def test_poison_sits_behind_the_tails_of_clean_rows():
    """what makes the poisoned x bite: a clean group row whose chunk count leaves 1 or 2 chunks to the masked tail of k_spmv_vec3 is
    followed by a group whose first chunk holds the poisoned column, and a clean scalar row that ends inside a 64-entry step of
    k_spmv_wave is followed by a row that starts with it"""
    for row0, nG, ntail, shift in gr.PACK_SHAPES[1:5]:
        n, rp, ci, v, x = gr.pack_matrix(row0, nG, ntail, 3, "well", shift)
        ci2, p, dirty = gr.poison_groups(row0, nG, rp, ci)
        nch = (np.diff(rp)[row0:row0 + 3 * nG:3] + 15) // 16
        first = [ci2[rp[row0 + 3 * g]:rp[row0 + 3 * g + 1]][:16] for g in range(nG)]
        assert any(nch[g] % 4 in (1, 2) and not dirty[row0 + 3 * g] and p in first[g + 1] for g in range(nG - 1)), (row0, nG)
    row0, nG, ntail, shift = gr.PACK_SHAPES[3]
    n, rp, ci, v, x = gr.pack_matrix(row0, nG, ntail, 3, "well", shift)
    ci2, p, dirty = gr.poison_groups(row0, nG, rp, ci)
    rl, first = np.diff(rp), ci2[np.minimum(rp[:-1], len(ci2) - 1)]
    scalar = [i for i in range(n - 1) if not row0 <= i < row0 + 3 * nG and not row0 <= i + 1 < row0 + 3 * nG]
    assert any(rl[i] % 64 and not dirty[i] and rl[i + 1] and first[i + 1] == p for i in scalar)


# ---- the exact comparisons on the generators' data: each named wrong result differs ---------------------------------------------------
def test_wrong_scans_are_rejected():
    for n in gr.SCAN_N:
        cnt = gr.scan_counts(n, "random")
        out = gr.ref_scan(cnt)
        assert out[0] == 0 and out[-1] == cnt.astype(np.int64).sum() and np.array_equal(np.diff(out), cnt)
    cnt = gr.scan_counts(3073, "random")
    out = gr.ref_scan(cnt)
    bad = out.copy()
    bad[-1] = -7  # out[n] missing: the entry's fill value stays
    assert not gr.same(bad, out)
    bad = out.copy()
    bad[1024:2048] -= out[1024]  # the offset of the second block dropped
    assert out[1024] > 0 and not gr.same(bad, out)
    huge = gr.ref_scan(gr.scan_counts(3073, "huge"))
    assert huge[1024] > 2 ** 32 and huge[-1] > 2 ** 42 and gr.ref_scan(gr.scan_counts(1025, "zero"))[-1] == 0


def test_wrong_transposes_are_rejected():
    n, rp, ci, lens, trp, tcol = transposed()
    rng = np.random.default_rng(0)
    for L in (129, 2600):  # a row left in arrival order: below SORT_MAX (the network), above it (the single lane)
        j = int(np.flatnonzero(lens == L)[0])
        bad = tcol.copy()
        bad[trp[j]:trp[j + 1]] = rng.permutation(tcol[trp[j]:trp[j + 1]])
        assert not gr.same(bad, tcol)


def test_wrong_nets_are_rejected():
    n, rp, ci = gr.nets_pattern()
    cptr, crow, cpos, isStart = gr.ref_nets(rp, ci, gr.nets_keeps(n, rp, ci)["all"])
    bad = cpos.copy()
    bad[cptr[8]:cptr[9]] += 1
    assert not gr.same(bad, cpos)
    bad = crow.copy()
    bad[cptr[8] + 16:cptr[8] + 32] = crow[cptr[8] + 16:cptr[8] + 32][::-1]
    assert not gr.same(bad, crow)
    assert isStart[4] == 1 and isStart[10] == 1  # a comparison that stops one short of the last net gives 0 here
    bad = isStart.copy()
    bad[4] = 0
    assert not gr.same(bad, isStart)


def test_a_filter_with_greater_or_equal_is_rejected():
    n, rp, ci, v, bound = gr.filter_matrix()
    rows = gr.rows_of(rp)
    off = ci != rows
    assert np.any(off & (v == bound)) and np.any(off & (v == -bound)) and np.any(off & np.isnan(v)) and np.any(~off & np.isnan(v))
    assert np.any(~off & (np.abs(v) < bound)) and np.any(off & (v == 0) & np.signbit(v)) and np.any(~off & (v == 0) & np.signbit(v)) and n > 256
    for name, mask in gr.filter_masks(n).items():
        a, b = gr.ref_filter(rp, ci, v, bound, 1, mask), gr.ref_filter(rp, ci, v, bound, 1, mask, strict=False)
        assert not gr.same(a[0], b[0]) and len(a[1]) < len(b[1]), name
        kept_diag = int(np.sum(a[1] == gr.rows_of(a[0])))
        assert kept_diag == int(np.sum(~off & (True if mask is None else mask[ci] != 0))), "a diagonal below the bound must stay unless its column is un-owned"
        assert not np.any(np.isnan(a[2]) & (a[1] != gr.rows_of(a[0]))), "a NaN off the diagonal must go"
    assert np.sum(~off & (gr.filter_masks(n)["diag"][ci] == 0)) > 0


# ---- the entries refuse invalid input before anything is launched ---------------------------------------------------------------------
def small():
    """a 5 x 5 pattern with ascending rows, values and a vector"""
    rp = np.array([0, 2, 3, 3, 6, 9], dtype=np.int64)
    ci = np.array([0, 3, 1, 0, 2, 4, 0, 1, 2], dtype=np.int32)
    return 5, rp, ci, np.arange(1.0, 10.0), np.arange(1.0, 6.0)


def bad_structures(rp, ci, ascending):
    out = []
    r = rp.copy(); r[0] = 1; out.append(("rowptr[0] != 0", r, ci))
    r = rp.copy(); r[2] = 1; out.append(("rowptr decreases", r, ci))
    c = ci.copy(); c[4] = 5; out.append(("column too large", rp, c))
    c = ci.copy(); c[4] = -1; out.append(("column negative", rp, c))
    out.append(("null rowptr", None, ci))
    out.append(("null col", rp, None))
    if ascending:
        c = ci.copy(); c[0], c[1] = 3, 0; out.append(("columns descend", rp, c))
        c = ci.copy(); c[4] = 0; out.append(("column repeated", rp, c))
    return out


def test_entries_refuse_invalid_input_before_any_launch():
    L = _capi.lib()
    n, rp, ci, v, x = small()
    keep = np.array([3, 0], dtype=np.int64)

    def refused(rc, who, what):
        assert rc == ARG and who in L.das_last_error(), (who, what, rc, L.das_last_error())

    # scan
    cnt = np.array([1, 0, 2], dtype=np.int32)
    for what, rc in [("n = 0", gr.dev_scan(L, cnt, 0)[0]), ("n < 0", gr.dev_scan(L, cnt, -1)[0]), ("null", gr.dev_scan(L, None, 3)[0]),
                     ("negative count", gr.dev_scan(L, np.array([1, -1, 2], dtype=np.int32))[0])]:
        refused(rc, b"das_debug_graph_scan", what)
    assert L.das_debug_graph_scan(3, gr._i(cnt), None, None) == ARG
    # transpose and nets: the structure, ascending columns, a pattern without entries
    for what, r, c in bad_structures(rp, ci, True) + [("no entries", np.zeros(n + 1, dtype=np.int64), ci)]:
        cc = np.zeros(9, dtype=np.int32) if c is None else c
        refused(L.das_debug_graph_transpose(n, gr._ll(r), gr._i(c), gr._ll(np.zeros(n + 1, dtype=np.int64)), gr._i(np.zeros(9, dtype=np.int32))), b"das_debug_graph_transpose", what)
        if r is not None and c is not None:
            refused(gr.dev_nets(L, n, r, cc, keep)[0], b"das_debug_graph_nets", what)
    refused(gr.dev_transpose(L, 0, rp, ci)[0], b"das_debug_graph_transpose", "n = 0")
    refused(L.das_debug_graph_transpose(n, gr._ll(rp), gr._i(ci), None, None), b"das_debug_graph_transpose", "null output")
    for what, k, nk in [("kept row too large", np.array([3, 5], dtype=np.int64), None), ("kept row negative", np.array([-1, 2], dtype=np.int64), None),
                        ("kept row repeated", np.array([3, 0, 3], dtype=np.int64), None), ("nKeep negative", keep, -1), ("nKeep above n", keep, 6)]:
        refused(gr.dev_nets(L, n, rp, ci, k, nk)[0], b"das_debug_graph_nets", what)
    refused(L.das_debug_graph_nets(n, gr._ll(rp), gr._i(ci), 2, None, None, None, None, None, None), b"das_debug_graph_nets", "null pointers")
    refused(gr.dev_nets(L, 0, rp, ci, keep)[0], b"das_debug_graph_nets", "n = 0")
    # rows gather
    rows, dst, out = np.array([3, 0, 3], dtype=np.int64), np.array([0, 3, 5], dtype=np.int64), np.full(8, -7, dtype=np.int32)
    who = b"das_debug_graph_rows_gather"
    for what, r, c in bad_structures(rp, ci, False)[:5]:
        refused(L.das_debug_graph_rows_gather(3, gr._ll(rows), n, gr._ll(r), gr._i(c), gr._ll(dst), gr._i(out), 8), who, what)
    for what, rr, dd, ol in [("row too large", np.array([3, 5, 3], dtype=np.int64), dst, 8), ("row negative", np.array([3, -1, 3], dtype=np.int64), dst, 8),
                             ("dst negative", rows, np.array([0, -1, 5], dtype=np.int64), 8), ("row past the end of out", rows, np.array([0, 3, 6], dtype=np.int64), 8),
                             ("outLen = 0", rows, dst, 0)]:
        refused(L.das_debug_graph_rows_gather(3, gr._ll(rr), n, gr._ll(rp), gr._i(ci), gr._ll(dd), gr._i(out), ol), who, what)
    refused(L.das_debug_graph_rows_gather(0, gr._ll(rows), n, gr._ll(rp), gr._i(ci), gr._ll(dst), gr._i(out), 8), who, "nSel = 0")
    refused(L.das_debug_graph_rows_gather(3, None, n, gr._ll(rp), gr._i(ci), gr._ll(dst), None, 8), who, "null")
    assert np.all(out == -7)
    # filter
    for what, r, c in bad_structures(rp, ci, False):
        cc = np.zeros(9, dtype=np.int32) if c is None else c
        rc = L.das_debug_compact(n, gr._ll(r), gr._i(c), gr._d(v), 0.5, 1, None, gr._ll(np.zeros(n + 1, dtype=np.int64)), gr._i(cc), gr._d(np.zeros(9)), gr._ll(np.zeros(1, dtype=np.int64)))
        refused(rc, b"das_debug_compact", what)
    refused(gr.dev_compact(L, 0, rp, ci, v, 0.5, 1, None)[0], b"das_debug_compact", "n = 0")
    refused(gr.dev_compact(L, n, rp, ci, None, 0.5, 1, None)[0], b"das_debug_compact", "null values")
    refused(gr.dev_compact(L, n, rp, ci, v, 0.5, 2, None)[0], b"das_debug_compact", "useBound = 2")
    # pack: group rows [row0, row0 + 3 nG) inside [0, n), the structure, a data array that holds the chunks
    who = b"das_debug_vecpack"
    for what, row0, nG in [("row0 + 3 nG > n", 3, 1), ("row0 + 3 nG > n", 0, 2), ("row0 negative", -1, 1), ("nG = 0", 0, 0), ("nG negative", 0, -1), ("nG huge", 0, 2 ** 62)]:
        refused(gr.dev_vecpack(L, n, rp, ci, v, row0, nG, x, cap_chunks=4)[0], who, what)
    for what, r, c in bad_structures(rp, ci, False):
        if r is not None:
            refused(gr.dev_vecpack(L, n, r, c, v, 0, 1, x, cap_chunks=4)[0], who, what)
    refused(gr.dev_vecpack(L, 0, rp, ci, v, 0, 1, x, cap_chunks=4)[0], who, "n = 0")
    refused(gr.dev_vecpack(L, n, rp, ci, None, 0, 1, x, cap_chunks=4)[0], who, "null values")
    refused(gr.dev_vecpack(L, n, rp, ci, v, 0, 1, x, cap_chunks=0)[0], who, "data too short")
    refused(gr.dev_vecpack(L, n, rp, ci, v, 0, 1, x, guard=-1)[0], who, "y shorter than n")
    refused(L.das_debug_vecpack(n, gr._ll(rp), gr._i(ci), gr._d(v), 0, 1, None, None, None, 4 * 448, None, gr._d(x), None, n), who, "null outputs")
    # ghost-row product
    who = b"das_debug_spmv_rows"
    rows = np.array([3, 0, 2, 3], dtype=np.int32)
    for what, r, c in bad_structures(rp, ci, False):
        refused(L.das_debug_spmv_rows(4, gr._i(rows), n, gr._ll(r), gr._i(c), gr._d(v), gr._d(x), gr._d(np.zeros(4)), 4), who, what)
    for what, rr in [("row too large", np.array([3, 5, 2, 3], dtype=np.int32)), ("row negative", np.array([3, -1, 2, 3], dtype=np.int32))]:
        refused(gr.dev_spmv_rows(L, rr, n, rp, ci, v, x)[0], who, what)
    refused(gr.dev_spmv_rows(L, rows, 0, rp, ci, v, x)[0], who, "n = 0")
    refused(gr.dev_spmv_rows(L, rows, n, rp, ci, v, x, guard=-1)[0], who, "buf too short")
    refused(gr.dev_spmv_rows(L, rows, n, rp, ci, v, None)[0], who, "null x")
    refused(gr.dev_spmv_rows(L, rows, n, rp, ci, None, x)[0], who, "null values")
    refused(L.das_debug_spmv_rows(0, gr._i(rows), n, gr._ll(rp), gr._i(ci), gr._d(v), gr._d(x), gr._d(np.zeros(4)), 4), who, "nrows = 0")

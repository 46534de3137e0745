"""The graph set-up kernels (dafoam_amd/csrc/das_graph.hpp), the jacLowerBounds filter and the packed operator
(dafoam_amd/csrc/das_opmat.hpp) restated in plain numpy - integers in int64, products in np.longdouble - the generators of synthetic
structures that no mesh produces, and the comparisons:

  scan, transpose, nets, gathered rows, filter, pack layout:   EXACT (integers equal, values and bytes bitwise equal)
  a product row of T entries, any order, FMA or not:           |got - ref| <= T u sum |a x|   (krylov_reference.check_sum, u = 2^-53)
  a row of no entries:                                         exactly 0
  a poisoned x (one NaN or +Inf entry):                        the rows that hold the poisoned column are non-finite, every other row is
                                                               finite and inside its bound (a kernel that multiplies a foreign x entry
                                                               by a masked 0.0 shows here and nowhere else)

Used by tests/test_gpu_graph_kernels.py and tests/test_gpu_opmat_kernels.py (kernels on the device) and by
tests/test_graph_reference_cpu.py (the restatements against independent ones, the comparisons against named wrong results, and the
argument checks of the entries)."""
import ctypes as C

import numpy as np

import krylov_reference as kr

LD = kr.LD
SENTINEL = kr.SENTINEL
SORT_MAX = 2048          # das_graph.hpp: longer transposed rows are sorted by one lane
CHUNK = 16               # das_opmat.hpp VP_CHUNK
CHUNK_DT = np.dtype([("col", "<i4", (CHUNK,)), ("val", "<f8", (3, CHUNK))])
assert CHUNK_DT.itemsize == 448

SCAN_N = [1, 255, 256, 1023, 1024, 1025, 2048, 3073]
TR_LENGTHS_SHORT = [0, 1, 2, 3, 63, 64, 65, 128, 129]
TR_LENGTHS_LONG = [1024, 1025, 2047, 2048, 2049, 2600]
NET_LENGTHS = [0, 1, 15, 16, 17, 33]
PACK_LENGTHS = [0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 280]
SCALAR_LENGTHS = kr.ROW_LENGTHS + [31, 32, 33, 48, 49]
# (row0, nG, scalar rows after the pack, shift of the length list: the single groups hold 81 and 280 entries)
PACK_SHAPES = [(0, 1, 0, 13), (0, 16, 14, 0), (5, 17, 0, 0), (5, 33, 14, 4), (0, 33, 0, 0), (5, 1, 14, 16)]


# ---- restatements ---------------------------------------------------------------------------------------------------------------
def ref_scan(cnt):
    out = np.zeros(len(cnt) + 1, dtype=np.int64)
    out[1:] = np.cumsum(np.asarray(cnt, dtype=np.int64))
    return out


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def ref_transpose(rp, ci):
    """(trp, tcol, order): the transposed pattern with ascending rows; order[t] = the row-major entry behind transposed entry t"""
    n = len(rp) - 1
    rows, cols = rows_of(rp), np.asarray(ci, dtype=np.int64)
    order = np.lexsort((rows, cols))
    return ref_scan(np.bincount(cols, minlength=n)), rows[order].astype(np.int32), order


def ref_nets(rp, ci, keep):
    """(cptr, crow, cpos, isStart): per column j the nets (positions in keep) of the kept rows that hold j, in ascending ROW order,
    the position of j in each of those rows' ascending column lists, and isStart[j] = the net list differs from the one of j - 1"""
    n = len(rp) - 1
    net = np.full(n, -1, dtype=np.int64)
    net[np.asarray(keep, dtype=np.int64)] = np.arange(len(keep))
    trp, tcol, order = ref_transpose(rp, ci)
    kept = net[tcol] >= 0
    colOf = rows_of(trp)
    cptr = ref_scan(np.bincount(colOf[kept], minlength=n))
    crow = net[tcol][kept].astype(np.int32)
    cpos = (order - np.asarray(rp, dtype=np.int64)[tcol])[kept].astype(np.int32)
    isStart = np.ones(n, dtype=np.uint8)
    for j in range(1, n):
        isStart[j] = 0 if np.array_equal(crow[cptr[j]:cptr[j + 1]], crow[cptr[j - 1]:cptr[j]]) else 1
    return cptr, crow, cpos, isStart


def ref_rows_gather(rows, rp, ci, dst, out):
    out = out.copy()
    for q, r in enumerate(rows):
        out[dst[q]:dst[q] + rp[r + 1] - rp[r]] = ci[rp[r]:rp[r + 1]]
    return out


def ref_filter(rp, ci, v, bound, use_bound, owned=None, strict=True):
    """keep fabs(v) > bound (strictly) or the diagonal; an un-owned column is dropped even on the diagonal.  (nrp, nci, nv)"""
    rows = rows_of(rp)
    with np.errstate(invalid="ignore"):
        big = (np.abs(v) > bound) if strict else (np.abs(v) >= bound)
    keep = big | (ci == rows) if use_bound else np.ones(len(ci), dtype=bool)
    if owned is not None:
        keep = keep & (np.asarray(owned)[ci] != 0)
    return ref_scan(np.bincount(rows[keep], minlength=len(rp) - 1)), ci[keep].copy(), v[keep].copy()


def ref_pack(rp, ci, v, row0, nG):
    """(built, cptr, chunks): the group rows [row0, row0 + 3 nG) as chunks of 16 int32 columns + 3 x 16 doubles; the pad columns repeat
    the last valid column of the row, the pad values are +0.0.  built = False (and nothing else) when three rows do not share a list"""
    lens = np.zeros(nG, dtype=np.int64)
    for g in range(nG):
        r = row0 + 3 * g
        b = rp[r:r + 4]
        lens[g] = b[1] - b[0]
        if b[2] - b[1] != lens[g] or b[3] - b[2] != lens[g]:
            return False, None, None
        if not (np.array_equal(ci[b[0]:b[1]], ci[b[1]:b[2]]) and np.array_equal(ci[b[0]:b[1]], ci[b[2]:b[3]])):
            return False, None, None
    cptr = ref_scan((lens + CHUNK - 1) // CHUNK)
    chunks = np.zeros(cptr[-1], dtype=CHUNK_DT)
    for g in range(nG):
        r, L = row0 + 3 * g, lens[g]
        for c in range(cptr[g + 1] - cptr[g]):
            k = c * CHUNK + np.arange(CHUNK)
            ok = k < L
            kk = np.minimum(k, L - 1)
            ch = chunks[cptr[g] + c]
            ch["col"][:] = ci[rp[r] + kk]
            for d in range(3):
                ch["val"][d][:] = np.where(ok, v[rp[r + d] + kk], 0.0)
    return True, cptr, chunks


def unpack(cptr, chunks, lens):
    """the CSR rows behind a pack: per group the column list and the three value rows (the pads cut off by the row lengths)"""
    out = []
    for g, L in enumerate(lens):
        ch = chunks[cptr[g]:cptr[g + 1]]
        out.append((ch["col"].reshape(-1)[:L].copy(), np.stack([ch["val"][:, d, :].reshape(-1)[:L] for d in range(3)]) if len(ch) else np.zeros((3, 0))))
    return out


def ref_product(rp, ci, v, x):
    """(y, magnitude, row lengths) in longdouble"""
    Y, M, lens = kr.ref_csr_rows(rp, ci, v, np.asarray(x, dtype=np.float64)[None, :])
    return Y[0], M[0], lens


def pack_product64(cptr, chunks, x, skip_last_chunk_of=None):
    """what k_spmv_vec3 computes from a pack, in float64 and another order (chunk by chunk, pads included): nG x 3"""
    y = np.zeros((len(cptr) - 1, 3))
    for g in range(len(cptr) - 1):
        hi = cptr[g + 1] - (1 if skip_last_chunk_of == g else 0)
        for c in range(cptr[g], hi):
            with np.errstate(invalid="ignore"):
                y[g] += (chunks[c]["val"] * x[chunks[c]["col"]][None, :]).sum(axis=1)
    return y


def csr_product64(rp, ci, v, x, rows=None):
    """float64, strided over 16 lanes like the kernels and reduced by a tree: another order than the reference's"""
    rows = range(len(rp) - 1) if rows is None else rows
    y = np.zeros(len(rows))
    for q, i in enumerate(rows):
        with np.errstate(invalid="ignore"):
            p = v[rp[i]:rp[i + 1]] * x[ci[rp[i]:rp[i + 1]]]
            lanes = np.array([p[l::CHUNK].sum() for l in range(CHUNK)])
            while len(lanes) > 1:
                lanes = lanes[: len(lanes) // 2] + lanes[len(lanes) // 2:]
        y[q] = lanes[0]
    return y


# ---- comparisons ------------------------------------------------------------------------------------------------------------------
def same(a, b):
    """exact: same length, same type, same bytes"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def check_product(y, ref, mag, lens):
    """every row inside T u sum |a x| with T its length (an empty row: exactly 0).  -> (ok, achieved max err / bound)"""
    ok, _ = kr.check_sum(y, ref, mag, lens)
    err = np.abs(np.asarray(y, dtype=np.float64).astype(LD) - ref)
    return ok, kr._ratio(err, LD(kr.U) * mag * np.asarray(lens, dtype=LD))


def check_poisoned(y, ref_clean, mag_clean, lens, dirty):
    """dirty: mask of the rows that hold the poisoned column - they must be non-finite; the others finite and inside their bound
    (ref_clean, mag_clean: the reference with any finite value in place of the poison - the clean rows never read it)"""
    y = np.asarray(y, dtype=np.float64)
    clean = ~dirty
    ok, ratio = check_product(y[clean], ref_clean[clean], mag_clean[clean], lens[clean])
    return bool(ok and not np.any(np.isfinite(y[dirty]))), ratio


def guard_intact(a, n):
    return bool(np.all(a[n:] == a.dtype.type(SENTINEL)))


# ---- generators -------------------------------------------------------------------------------------------------------------------
def scan_counts(n, kind, seed=0):
    if kind == "zero":
        return np.zeros(n, dtype=np.int32)
    if kind == "huge":  # block sums and the total pass 2^32: nothing may be allocated by the total
        c = np.full(n, 2 ** 31 - 1, dtype=np.int32)
        c[::7] = 2 ** 31 - 2
        return c
    return np.random.default_rng([seed, n]).integers(0, 6, size=n).astype(np.int32)


def pattern_from_columns(n, col_rows):
    """row-major CSR (rowptr int64, col int32, columns strictly ascending) of the pattern whose COLUMN j holds the rows col_rows[j]"""
    cols = np.concatenate([np.full(len(r), j, dtype=np.int64) for j, r in enumerate(col_rows)])
    rows = np.concatenate([np.asarray(r, dtype=np.int64) for r in col_rows])
    order = np.lexsort((cols, rows))
    rp = ref_scan(np.bincount(rows, minlength=n))
    return rp, cols[order].astype(np.int32)


def transpose_pattern(seed=1):
    """n = 2603 (no multiple of 4 or 16): transposed rows (= dense columns) of 0, 1, 2, 3, 63, 64, 65, 128, 129 entries all over, one
    of 1024, 1025, 2047, 2048, 2049 and 2600 entries each, an empty first and an empty last one.  -> (n, rowptr, col, lengths)"""
    n = 2603
    rng = np.random.default_rng(seed)
    lens = [TR_LENGTHS_SHORT[(5 * j + 1) % len(TR_LENGTHS_SHORT)] for j in range(n)]
    for q, L in enumerate(TR_LENGTHS_LONG):
        lens[101 + 397 * q] = L
    lens[0] = lens[n - 1] = 0
    col_rows = [np.sort(rng.choice(n, size=L, replace=False)) for L in lens]
    rp, ci = pattern_from_columns(n, col_rows)
    assert rp[-1] <= 2e5 and set(TR_LENGTHS_SHORT + TR_LENGTHS_LONG) <= set(lens)
    return n, rp, ci, np.array(lens)


def nets_pattern(seed=2):
    """n = 157: transposed rows of 0, 1, 15, 16, 17 and 33 entries; neighbouring columns with identical lists (2, 3 and 8, 9), with
    equal length and another last row (3, 4 and 9, 10), both empty (0, 1 and 11, 12).  -> (n, rowptr, col)"""
    n = 157
    rng = np.random.default_rng(seed)

    def pick(L):
        return np.sort(rng.choice(n - 1, size=L, replace=False))  # row n - 1 is left for the "other last row" columns

    A, B = pick(16), pick(33)
    col_rows = [[], [], A, A, np.append(A[:-1], n - 1), pick(1), pick(15), pick(17), B, B, np.append(B[:-1], n - 1), [], []]
    while len(col_rows) < n:
        col_rows.append(pick(NET_LENGTHS[(3 * len(col_rows) + 1) % len(NET_LENGTHS)]))
    rp, ci = pattern_from_columns(n, col_rows)
    pos = np.arange(rp[-1]) - rp[rows_of(rp)]
    last = np.diff(rp)[rows_of(rp)] - 1
    assert np.any((pos == 0) & (last > 1)) and np.any((pos == last) & (last > 1)) and np.any((pos > 0) & (pos < last))
    return n, rp, ci


def nets_keeps(n, rp, ci):
    """the kept sets: none, all (net ids in descending row order), every other row, and - from the 33-entry column 8 - only the rows
    of lane 15 of its 16-entry steps (the third step keeps nothing) and only the rows of lane 0"""
    trp, tcol, _ = ref_transpose(rp, ci)
    t8 = tcol[trp[8]:trp[9]].astype(np.int64)
    assert len(t8) == 33
    return {"none": np.zeros(0, dtype=np.int64), "all": np.arange(n - 1, -1, -1, dtype=np.int64), "every_other": np.arange(0, n, 2, dtype=np.int64),
            "lane15": t8[[15, 31]], "lane0": t8[[32, 0, 16]]}


def values(size, seed, kind):
    """well: |a| in [1, 2) with random signs; ill: kr.vector spread over twelve orders like make_csr(ill=True)"""
    rng = np.random.default_rng(seed)
    if kind == "well":
        return np.where(rng.random(size) < 0.5, -1.0, 1.0) * (1.0 + rng.random(size))
    return kr.vector(size, [seed, 1] if np.ndim(seed) == 0 else list(seed) + [1]) * 10.0 ** (-12.0 * rng.random(size))


def assert_well(rp, ci, v, x):
    """every single product exceeds the bound of its row by many orders: a dropped, doubled or misplaced entry cannot hide"""
    _, mag, lens = ref_product(rp, ci, v, x)
    if len(v):
        assert np.min(np.abs(v)) * np.min(np.abs(x)) >= 1.0 and float(np.max(lens * kr.U * mag)) < 1e-9


def pack_matrix(row0, nG, ntail, seed, kind="well", shift=0, break_at=None):
    """n x n CSR with scalar rows [0, row0), group rows of PACK_LENGTHS[(g + shift) % 17] entries (three rows, one column list:
    unsorted, repeated columns) and ntail scalar rows of SCALAR_LENGTHS behind them.  break_at = (g, what): the rows of group g no
    longer share their list - what = "len" or a position (0, a lane != 0, -1 = last) whose column differs in one row.
    -> (n, rowptr, col, values, x)"""
    rng = np.random.default_rng([seed, row0, nG, ntail])
    n = row0 + 3 * nG + ntail
    lens = [SCALAR_LENGTHS[(3 * i + 2) % len(SCALAR_LENGTHS)] for i in range(row0)]
    glen = [PACK_LENGTHS[(g + shift) % len(PACK_LENGTHS)] for g in range(nG)]
    for g in range(nG):
        lens += [glen[g]] * 3
    lens += [SCALAR_LENGTHS[i % len(SCALAR_LENGTHS)] for i in range(ntail)]
    cols = []
    for i, L in enumerate(lens):
        g, d = divmod(i - row0, 3)
        if 0 <= g < nG and d > 0:
            cols.append(cols[-1].copy())
        else:
            c = rng.integers(0, n, size=L).astype(np.int32)
            if L >= 2:
                c[1] = c[0]
            cols.append(c)
    if break_at is not None:
        g, what = break_at
        r = row0 + 3 * g
        if what == "len":
            cols[r + 1] = cols[r + 1][:-1]
            lens[r + 1] -= 1
        else:
            d = 1 if what == 0 else 2
            cols[r + d][what] = (cols[r + d][what] + 1) % n
    rp = ref_scan(lens)
    ci = np.concatenate(cols).astype(np.int32) if rp[-1] else np.zeros(0, dtype=np.int32)
    v = values(int(rp[-1]), [seed, 7], kind)
    x = values(n, [seed, 8], "well") if kind == "well" else kr.vector(n, [seed, 8])
    if kind == "well":
        assert_well(rp, ci, v, x)
    return n, rp, ci, v, x


def poison(rp, ci, seed=0):
    """(ci', p, dirty): column p put at every third position of every other non-empty row (dirty = the rows that then hold it), and taken
    out of all others - so that every clean row is followed by a row whose first entries are poisoned: an unclamped tail reads them"""
    n = len(rp) - 1
    ci = ci.copy()
    p = int(np.random.default_rng(seed).integers(0, n))
    rows = rows_of(rp)
    pos = np.arange(len(ci)) - rp[rows]
    nonempty = np.flatnonzero(np.diff(rp) > 0)
    odd = np.zeros(n, dtype=bool)
    odd[nonempty[1::2]] = True
    ci[ci == p] = (p + 1) % n
    if n > 1:
        ci[odd[rows] & (pos % 3 == 0)] = p
    dirty = np.zeros(n, dtype=bool)
    dirty[rows[ci == p]] = True
    return ci, p, dirty


def poison_groups(row0, nG, rp, ci, seed=0):
    """the same for a pack matrix: whole groups are dirty or clean (three rows, one list), scalar rows as in poison()"""
    n = len(rp) - 1
    ci2, p, _ = poison(rp, ci, seed)
    for g in range(nG):  # the rows of a group share the list of its first row again
        r = row0 + 3 * g
        for d in (1, 2):
            ci2[rp[r + d]:rp[r + d + 1]] = ci2[rp[r]:rp[r + 1]]
    dirty = np.zeros(n, dtype=bool)
    dirty[rows_of(rp)[ci2 == p]] = True
    return ci2, p, dirty


def filter_matrix(seed=5):
    """n = 300 (two blocks of the one-thread-per-row kernels), bound 1e-3: in every row of four or more entries a diagonal below the
    bound (kept), |v| == bound with either sign (dropped), a NaN off the diagonal (dropped); a NaN ON a diagonal (kept), -0.0 off
    and on the diagonal.  -> (n, rowptr, col, values, bound)"""
    n, bound = 300, 1.0e-3
    rp, ci, v = kr.make_csr(n, seed)
    ci = ci.copy()
    for i in range(n):
        b, L = rp[i], rp[i + 1] - rp[i]
        ci[b:b + L][ci[b:b + L] == i] = (i + 1) % n
        if L >= 4:
            ci[b] = i
            v[b] = 1.0e-9 if i % 2 else -1.0e-9
            v[b + 1], v[b + 2], v[b + 3] = bound, -bound, np.nan
        if L >= 15:
            v[b + 5] = -0.0
            v[b + 6] = np.nextafter(bound, 1.0)
            v[b + 7] = np.nextafter(bound, 0.0)
        if L == 1:
            ci[b] = i
            v[b] = np.nan if i % 2 else -0.0
    return n, rp, ci, v, bound


def filter_masks(n):
    """null, a mask that keeps every diagonal's column... no mask keeps all; "some": every fifth column un-owned; "diag": the columns
    5 .. 49 un-owned, which drops their diagonals"""
    some = np.ones(n, dtype=np.uint8)
    some[::5] = 0
    diag = np.ones(n, dtype=np.uint8)
    diag[5:50] = 0
    return {"null": None, "some": some, "diag": diag}


# ---- the entries ------------------------------------------------------------------------------------------------------------------
def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _ll(a):
    return _p(a, C.POINTER(C.c_longlong))


def _i(a):
    return _p(a, C.POINTER(C.c_int))


def _d(a):
    return _p(a, C.POINTER(C.c_double))


def _u8(a):
    return _p(a, C.POINTER(C.c_ubyte))


def dev_scan(L, cnt, n=None):
    n = len(cnt) if n is None else n
    out, total = np.full(n + 1 if n > 0 else 1, -7, dtype=np.int64), C.c_longlong(-7)
    return L.das_debug_graph_scan(n, _i(cnt), _ll(out), C.byref(total)), out, total.value


def dev_transpose(L, n, rp, ci):
    trp, tcol = np.full(max(n, 0) + 1, -7, dtype=np.int64), np.full(max(len(ci), 1), -7, dtype=np.int32)
    return L.das_debug_graph_transpose(n, _ll(rp), _i(ci), _ll(trp), _i(tcol)), trp, tcol[: len(ci)]


def dev_nets(L, n, rp, ci, keep, nKeep=None):
    cap = max(len(ci), 1)
    cptr, crow, cpos = np.full(max(n, 0) + 1, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int32), np.full(cap, -7, dtype=np.int32)
    isStart, total = np.full(max(n, 1), 7, dtype=np.uint8), C.c_longlong(-7)
    rc = L.das_debug_graph_nets(n, _ll(rp), _i(ci), len(keep) if nKeep is None else nKeep, _ll(keep) if len(keep) else None, _ll(cptr), _i(crow), _i(cpos),
                                _u8(isStart), C.byref(total))
    t = max(total.value, 0)
    return rc, cptr, crow[:t], cpos[:t], isStart, total.value


def dev_rows_gather(L, rows, n, rp, ci, dst, out):
    out = out.copy()
    return L.das_debug_graph_rows_gather(len(rows), _ll(rows), n, _ll(rp), _i(ci), _ll(dst), _i(out), len(out)), out


def dev_compact(L, n, rp, ci, v, bound, use_bound, owned):
    cap = max(len(ci), 1)
    nrp, nci, nv, nnz = np.full(max(n, 0) + 1, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int32), np.full(cap, SENTINEL), C.c_longlong(-7)
    rc = L.das_debug_compact(n, _ll(rp), _i(ci), _d(v), bound, use_bound, _u8(owned), _ll(nrp), _i(nci), _d(nv), C.byref(nnz))
    t = max(nnz.value, 0)
    return rc, nrp, nci[:t], nv[:t]


def dev_vecpack(L, n, rp, ci, v, row0, nG, x, guard=7, cap_chunks=None):
    """-> (rc, built, cptr, chunks, nChunks, y): y holds n + guard entries, the sentinel in all of them on entry; cptr and the chunk
    bytes hold 0x5a where nothing was written"""
    cap = int(((np.diff(rp)[row0:row0 + 3 * nG:3] + CHUNK - 1) // CHUNK).sum()) if cap_chunks is None else cap_chunks
    cptr = np.full(min(max(nG, 0), 1 << 20) + 1, 0x5A5A5A5A, dtype=np.int64)
    data = np.full(max(cap, 1) * CHUNK_DT.itemsize, 0x5A, dtype=np.uint8)
    y = np.full(max(n, 0) + guard, SENTINEL)
    built, nch = C.c_int(-7), C.c_longlong(-7)
    rc = L.das_debug_vecpack(n, _ll(rp), _i(ci), _d(v), row0, nG, C.byref(built), _ll(cptr), _u8(data), cap * CHUNK_DT.itemsize, C.byref(nch), _d(x), _d(y), len(y))
    return rc, built.value, cptr, data, nch.value, y


def dev_spmv_rows(L, rows, n, rp, ci, v, x, guard=5):
    buf = np.full(len(rows) + guard, SENTINEL)
    return L.das_debug_spmv_rows(len(rows), _i(rows), n, _ll(rp), _i(ci), _d(v), _d(x), _d(buf), len(buf)), buf

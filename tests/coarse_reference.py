"""The coarse-space kernels of the two-level preconditioner (dafoam_amd/csrc/das_coarse.hpp: k_coarse_assemble, k_gj_pivot, k_gj_elim,
k_coarse_restrict, k_coarse_solve, k_coarse_prolong, k_az_build, k_az_apply) restated in plain numpy - integers in int64, every rounded
sum in np.longdouble next to a float64 restatement in the kernel's own order -, the generators of inputs that no mesh produces, and the
ctypes wrappers of the test-only entries das_debug_coarse_*.  u = 2^-53, T = the number of terms of a sum:

  E = Z^T A Z, diagScale 1 or 0.5 (the scale is exact):      bitwise equal to the sequential float64 sum in list and storage order
  E, diagScale 0.7 (the product may be fused into the add):  |E - E_ld| <= (T + 1) u sum |terms|
  E^-1, "exact" matrices:                                    bitwise the exact inverse
  E^-1, "dominant" / "permuted":                             e_dev <= 4 e_ref, e = max |Inv - Inv_ld| / max |Inv_ld|, e_ref that of the
                                                             float64 restatement of the same elimination (same pivot rule)
  t = Z^T r:                                                 |t - t_ld| <= T u sum |r|, an empty aggregate exactly 0
  u = Einv t:                                                |u - u_ld| <= nagg u sum |Einv t|, from the device's own t
  y = (y +) Z u:                                             bitwise, from the device's own u
  sparse A Z: cnt, ptr, nnz, oa (first appearance), ov:      exact / bitwise (adds only, storage order)
  out = v - (A Z) u:                                         |out - ref| <= (T + 1) u (|v_i| + sum |ov u|)

Used by tests/test_gpu_coarse_kernels.py (kernels on the device) and tests/test_coarse_reference_cpu.py (the restatements against
independent dense numpy, the generators against what they promise, the argument checks of the entries)."""
import ctypes as C
import functools

import numpy as np

import graph_reference as gr
import krylov_reference as kr

LD = kr.LD
U = kr.U
SENTINEL = gr.SENTINEL
values, same, guard_intact = gr.values, gr.same, gr.guard_intact
GUARD = 8        # das_coarse_debug.hpp COARSE_GUARD: entries behind every output that has no length argument
AZ_CAP = 64      # das_coarse.hpp
MAX_AGG = 2048

ASM_NAGG = [1, 2, 255, 256, 257, 513, 2048]
ASM_N = 2101
INV_N = [1, 2, 3, 64, 255, 256, 257, 513]
COR_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
AZ_TOUCH = [0, 1, 2, 63, 64]


# ---- E = Z^T A Z ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def assemble_case(nagg, off, transpose, seed=11):
    """-> dict(nagg, N, off, n, rp, ci, v, aggRow, aggCol, transpose).  n = off + N + 7 rows of 0 .. 12 entries, columns below off (off > 0)
    and at or above off + N, repeated columns, a diagonal in most field rows; about 5 % of the cells with aggRow = -1 and other 5 % with
    aggCol = -1; from three aggregates on: aggregate nagg // 2 without a row cell and the LAST aggregate with a single one (a row of four entries or more).  transpose = 1
    (the forward-mode preconditioner): aggCol IS aggRow."""
    rng = np.random.default_rng([seed, nagg, off])
    N, n = ASM_N, off + ASM_N + 7
    lens = rng.integers(0, 13, size=n)
    rp = gr.ref_scan(lens)
    ci = rng.integers(0, n, size=int(rp[-1])).astype(np.int32)
    for i in range(n):
        b, L = rp[i], lens[i]
        if L >= 4:
            ci[b + 1] = ci[b]                                  # the same column, so the same aggregate, twice in a row
            if i % 7 == 0:
                ci[b + 2] = off + N + i % 7
            if off > 0 and i % 5 == 0:
                ci[b + 3] = i % off
        if L >= 1 and off <= i < off + N and i % 6:
            ci[b + L // 2] = i                                 # the diagonal: j == c
    v = values(int(rp[-1]), [seed, 7, nagg], "well")
    base = rng.integers(0, nagg, size=N).astype(np.int32)
    aggRow = base.copy()
    single = -1
    if nagg >= 3:
        e, s = nagg // 2, nagg - 1
        aggRow[aggRow == e] = (e + 1) % (nagg - 1)
        aggRow[aggRow == s] = 0
        single = next(cell for cell in range(N // 3, N) if lens[off + cell] >= 4 and (off + cell) % 6)  # a row with entries and a diagonal
        aggRow[single] = s
    out = rng.permutation(N)
    out = out[out != single]
    aggRow[out[: N // 20]] = -1
    if transpose:
        aggCol = aggRow
    else:
        aggCol = base.copy()
        aggCol[out[N // 20: N // 10]] = -1
    return dict(nagg=nagg, N=N, off=off, n=n, rp=rp, ci=ci, v=v, aggRow=aggRow, aggCol=aggCol, transpose=transpose)


def assemble_terms(c):
    """the terms of E in the kernel's order - row cells in ascending order inside an aggregate, entries in storage order, which for one
    (I, J) is the storage order of the field rows -> (I, J, k, isDiag) per contributing entry"""
    off, N = c["off"], c["N"]
    rows = gr.rows_of(c["rp"])
    cell, j = rows - off, c["ci"].astype(np.int64) - off
    ok = (cell >= 0) & (cell < N) & (j >= 0) & (j < N)
    k = np.flatnonzero(ok)
    I, J = c["aggRow"][cell[k]], c["aggCol"][j[k]]
    keep = (I >= 0) & (J >= 0)
    k = k[keep]
    return I[keep].astype(np.int64), J[keep].astype(np.int64), k, (j[k] == cell[k])


def ref_assemble(c, diagScale, dtype=np.float64):
    """(E, magnitude, T) as the kernel stores E: E[I][J], transposed storage with transpose = 1.  dtype float64: the sequential sum the
    kernel computes when the scale is exact; longdouble: the reference"""
    nagg = c["nagg"]
    I, J, k, dg = assemble_terms(c)
    term = c["v"][k].astype(dtype)
    term = np.where(dg, term * dtype(diagScale), term)
    E, M, T = np.zeros((nagg, nagg), dtype=dtype), np.zeros((nagg, nagg), dtype=dtype), np.zeros((nagg, nagg), dtype=np.int64)
    np.add.at(E, (I, J), term)          # unbuffered: one add after the other, in the order given
    np.add.at(M, (I, J), np.abs(term))
    np.add.at(T, (I, J), 1)
    if c["transpose"]:
        E, M, T = E.T.copy(), M.T.copy(), T.T.copy()
    return E, M, T


def check_assemble(E, ref, mag, T):
    """|E - E_ld| <= (T + 1) u sum |terms| per entry; no term: exactly 0.  -> (ok, achieved / bound)"""
    err = np.abs(np.asarray(E, dtype=np.float64).astype(LD) - ref)
    bound = (T + 1).astype(LD) * LD(U) * mag
    ok = bool(np.all(np.isfinite(E)) and np.all(err <= bound) and np.all(E[T == 0] == 0.0))
    return ok, kr._ratio(err, bound)


def move_diagonal(c):
    """the twin of a case: in one field row the diagonal and another field column of a live aggregate change places.  -> (twin, the
    entries of E (as stored) that the two positions feed)"""
    off, N, rp, ci = c["off"], c["N"], c["rp"], c["ci"]
    for cell in range(N):
        if c["aggRow"][cell] < 0 or c["aggCol"][cell] < 0:
            continue
        b, e = rp[off + cell], rp[off + cell + 1]
        cols = ci[b:e].astype(np.int64) - off
        d = np.flatnonzero(cols == cell)
        o = [q for q in range(e - b) if 0 <= cols[q] < N and cols[q] != cell and c["aggCol"][cols[q]] not in (-1, c["aggCol"][cell])]
        if len(d) == 1 and o:
            p, q = b + d[0], b + o[0]
            ci2 = ci.copy()
            ci2[p], ci2[q] = ci[q], ci[p]
            I = int(c["aggRow"][cell])
            fed = [(I, int(c["aggCol"][cell])), (I, int(c["aggCol"][cols[o[0]]]))]
            if c["transpose"]:
                fed = [(b_, a_) for a_, b_ in fed]
            twin = dict(c)
            twin["ci"] = ci2
            return twin, fed
    raise AssertionError("no row with a diagonal and another live column")


# ---- E^-1 ---------------------------------------------------------------------------------------------------------------------------
def gauss_jordan(A, dtype=np.float64, fused=False):
    """the elimination of k_gj_pivot / k_gj_elim: per column the largest |a| from the diagonal down (lowest row on ties), rows swapped,
    the pivot row scaled by 1 / pivot, then a -= f b in every other row with f != 0.  fused (float64 only): every a - f b rounded once.
    -> (Inv, singular, pivot rows).  singular: a column without a positive |a| (zeros, NaN); Inv is then of no use"""
    n = A.shape[0]
    W = np.concatenate([np.asarray(A, dtype=np.float64).astype(dtype), np.eye(n, dtype=dtype)], axis=1)
    piv = np.zeros(n, dtype=np.int64)
    for k in range(n):
        a = np.abs(W[k:, k])
        best, pr = dtype(-1.0), k
        with np.errstate(invalid="ignore"):
            gt = a > best
        if np.any(gt):
            m = np.max(a[gt])
            pr = k + int(np.flatnonzero(gt & (a == m))[0])
            best = m
        if not best > 0:
            return W[:, n:], 1, piv
        piv[k] = pr
        ip = dtype(1.0) / W[pr, k]
        rk, rp_ = W[k].copy(), W[pr].copy()
        if pr != k:
            W[pr] = rk
        W[k] = rp_ * ip
        f = W[:, k].copy()
        f[k] = 0
        rows = np.flatnonzero(f != 0)
        if fused:
            W[rows] = (W[rows].astype(LD) - f[rows, None].astype(LD) * W[k][None, :].astype(LD)).astype(dtype)
        else:
            W[rows] -= f[rows, None] * W[k][None, :]
    return W[:, n:], 0, piv


def rotation(n):
    """the row permutation of "permuted": row i holds row (i - s) mod n, s = 256 from n = 257 on (the dominant entry of column 0 then sits
    256 rows below the diagonal: only the second stride of the pivot search meets it), else n // 2"""
    s = 256 if n >= 257 else n // 2
    return (np.arange(n) - s) % n


@functools.lru_cache(maxsize=None)
def invert_matrix(n, kind, seed=3):
    """dominant: D + 1e-3 R, |D_ii| in [1, 2), R standard normal.  permuted: its rows under rotation(n).  exact: P D L, P a random
    permutation, D_ii = 2^-depth(i), L unit lower with one or two entries +-1 per row left of the diagonal at columns of smaller depth
    (depth <= 6) - the pivot of every column is its own power of two, strictly the largest, and every operation is exact"""
    rng = np.random.default_rng([seed, n])
    if kind in ("dominant", "permuted"):
        A = np.diag(values(n, [seed, n, 1], "well")) + 1.0e-3 * rng.standard_normal((n, n))
        if kind == "permuted":
            A = A[rotation(n)]
            if n >= 257:
                piv = gauss_jordan(A)[2]
                assert np.any(piv - np.arange(n) >= 256), "no pivot in the second stride of the search"
        assert np.linalg.cond(A) <= 1.0e4
        return A
    assert kind == "exact"
    depth = np.zeros(n, dtype=np.int64)
    L = np.eye(n)
    for i in range(1, n):
        if i % 3 == 0:
            continue
        cand = np.flatnonzero(depth[:i] < 6)
        cols = rng.choice(cand, size=min(len(cand), 1 + i % 2), replace=False)
        L[i, cols] = rng.choice([-1.0, 1.0], size=len(cols))
        depth[i] = 1 + depth[cols].max()
    A = (np.diag(2.0 ** -depth.astype(np.float64)) @ L)[rng.permutation(n)]
    return A


def exact_inverse(A):
    """the inverse of an "exact" matrix: the longdouble elimination, checked to be exact (A Inv = I and Inv A = I without rounding) and
    to fit float64"""
    Inv, sing, _ = gauss_jordan(A, LD)
    n = A.shape[0]
    assert sing == 0 and np.array_equal(A.astype(LD) @ Inv, np.eye(n, dtype=LD)) and np.array_equal(Inv @ A.astype(LD), np.eye(n, dtype=LD))
    I64 = Inv.astype(np.float64)
    assert np.array_equal(I64.astype(LD), Inv)
    return I64


def inverse_error(Inv, ref):
    """max |Inv - ref| / max |ref| as a float"""
    return float(np.max(np.abs(np.asarray(Inv, dtype=np.float64).astype(LD) - ref)) / np.max(np.abs(ref)))


def singular_matrices():
    """small integers - 64 times an "exact" matrix, every pivot a power of two -, so the zeros are exact: the second of two equal rows
    becomes exactly zero when the first one is the pivot row.  The last one is regular"""
    base = 64.0 * invert_matrix(6, "exact")
    assert np.array_equal(base, np.round(base)) and np.abs(base).max() <= 64
    out = {}
    A = base.copy(); A[:, 0] = 0.0; out["zero first column"] = (A, 1)
    A = base.copy(); A[:, 5] = 0.0; out["zero last column"] = (A, 1)
    A = base.copy(); A[4] = A[2]; out["two equal rows"] = (A, 1)
    A = base.copy(); A[:, 3] = np.nan; out["a column of NaN"] = (A, 1)
    out["regular"] = (base, 0)
    return out


# ---- restrict, solve, prolong -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def correct_case(off, kind, seed=5):
    """one partition with aggregates of 0, 1, 63, 64, 65, 255, 256, 257 and 1000 cells (aggregate q has COR_SIZES[q] cells, scattered over
    the field) and 40 cells of no aggregate; n = off + N + 7.  -> dict(nagg, N, off, n, agg, Einv, r)"""
    rng = np.random.default_rng([seed, off])
    nagg = len(COR_SIZES)
    agg = np.concatenate([np.full(s, q, dtype=np.int32) for q, s in enumerate(COR_SIZES)] + [np.full(40, -1, dtype=np.int32)])
    agg = agg[rng.permutation(len(agg))]
    N = len(agg)
    n = off + N + 7
    Einv = values(nagg * nagg, [seed, 2], "well").reshape(nagg, nagg)
    r = kr.vector(n, [seed, 3, off], ill=(kind == "ill"))
    return dict(nagg=nagg, N=N, off=off, n=n, agg=agg, Einv=Einv, r=r)


def ref_restrict(c, r=None):
    """(t, sum |r|, T) in longdouble"""
    r = (c["r"] if r is None else r).astype(LD)
    nagg, off, agg = c["nagg"], c["off"], c["agg"]
    t, m, T = np.zeros(nagg, dtype=LD), np.zeros(nagg, dtype=LD), np.zeros(nagg, dtype=np.int64)
    live = np.flatnonzero(agg >= 0)
    np.add.at(t, agg[live], r[off + live])
    np.add.at(m, agg[live], np.abs(r[off + live]))
    np.add.at(T, agg[live], 1)
    return t, m, T


def restrict64(c):
    """float64, the kernel's order: thread q sums the cells q, q + 256, ... of the sorted list, wavefronts of 64 by a shuffle tree, then
    red[0] + red[1] + red[2] + red[3]"""
    r, off, agg = c["r"], c["off"], c["agg"]
    t = np.zeros(c["nagg"])
    for I in range(c["nagg"]):
        x = r[off + np.flatnonzero(agg == I)]
        lanes = np.zeros(256)
        for q in range(256):
            for val in x[q::256]:
                lanes[q] += val
        red = []
        for w in range(4):
            a = lanes[64 * w: 64 * w + 64].copy()
            o = 32
            while o:
                a[:o] = a[:o] + a[o:2 * o]
                o >>= 1
            red.append(a[0])
        t[I] = ((red[0] + red[1]) + red[2]) + red[3]
    return t


def check_restrict(t, ref, mag, T):
    err = np.abs(np.asarray(t, dtype=np.float64).astype(LD) - ref)
    bound = T.astype(LD) * LD(U) * mag
    ok = bool(np.all(np.isfinite(t)) and np.all(err <= bound) and np.all(np.asarray(t)[T == 0] == 0.0))
    return ok, kr._ratio(err, bound)


def check_solve(u, Einv, t):
    """|u - Einv t| <= nagg u sum |Einv t| with the t given (the device's own)"""
    P = Einv.astype(LD) * np.asarray(t, dtype=np.float64).astype(LD)[None, :]
    ref, mag = P.sum(axis=1), np.abs(P).sum(axis=1)
    err = np.abs(np.asarray(u, dtype=np.float64).astype(LD) - ref)
    bound = LD(Einv.shape[0]) * LD(U) * mag
    return bool(np.all(np.isfinite(u)) and np.all(err <= bound)), kr._ratio(err, bound)


def ref_prolong(c, u, y0, set_):
    """float64, one add per entry: y[off + cell] (+)= u[agg(cell)], 0.0 for a cell of no aggregate and outside the field.  ylen >= n:
    what lies behind n is left alone"""
    n, off, N, agg = c["n"], c["off"], c["N"], c["agg"]
    add = np.zeros(n)
    live = np.flatnonzero(agg >= 0)
    add[off + live] = np.asarray(u, dtype=np.float64)[agg[live]]
    y = y0.copy()
    with np.errstate(invalid="ignore"):
        y[:n] = add if set_ else y0[:n] + add
    return y


# ---- the sparse A Z ---------------------------------------------------------------------------------------------------------------
AZ_NAGG, AZ_N = 80, 320


@functools.lru_cache(maxsize=None)
def az_case(off, extend=False, seed=9):
    """n = off + 320 + 7 rows (no multiple of 256, two blocks); 80 aggregates, aggregate a = the cells a, a + 80, a + 160 and, for odd a,
    a + 240 (the even cells from 240 on have none).  Row i touches AZ_TOUCH[i % 5] = 0, 1, 2, 63 or 64 distinct aggregates: every one of
    them up to three times more, at other cells and interleaved with the first appearances of the later ones, with columns of no
    aggregate and columns outside the field in between.  extend: the last 64-aggregate row meets a 65th.
    -> dict(nagg, n, N, off, rp, ci, v, agg, u, vec, touch, extended)"""
    rng = np.random.default_rng([seed, off])
    nagg, N = AZ_NAGG, AZ_N
    n = off + N + 7
    agg = (np.arange(N) % nagg).astype(np.int32)
    agg[240::2] = -1
    dead = off + np.arange(240, N, 2)
    outside = np.concatenate([np.arange(off), off + N + np.arange(7)])
    rows, touch = [], np.zeros(n, dtype=np.int64)
    for i in range(n):
        m = AZ_TOUCH[i % len(AZ_TOUCH)]
        touch[i] = m
        order = rng.permutation(nagg)[:m]
        cols = []
        for q, a in enumerate(order):
            cols.append(off + a + 80 * int(rng.integers(0, 3)))
            for _ in range(int(rng.integers(0, 4)) if m < 63 or q % 9 == 0 else 0):   # repeats of what is already there
                b = order[int(rng.integers(0, q + 1))]
                cols.append(off + b + 80 * int(rng.integers(0, 3)))
            if q % 5 == 1:
                cols.append(int(rng.choice(dead)))
            if q % 7 == 2:
                cols.append(int(rng.choice(outside)))
        if m == 0 and i % 2:
            cols = [int(rng.choice(dead)), int(rng.choice(outside)), int(rng.choice(dead))]  # entries, none of them in an aggregate
        rows.append(cols)
    extended = max(i for i in range(n) if touch[i] == 64)
    if extend:
        used = set(int(agg[c - off]) for c in rows[extended] if off <= c < off + N and agg[c - off] >= 0)
        rows[extended] = rows[extended] + [off + min(set(range(nagg)) - used)]
    rp = gr.ref_scan([len(r) for r in rows])
    ci = np.concatenate([np.asarray(r, dtype=np.int32) for r in rows])
    v = values(int(rp[-1]), [seed, 1], "well")
    return dict(nagg=nagg, n=n, N=N, off=off, rp=rp, ci=ci, v=v, agg=agg, u=kr.vector(nagg, [seed, 2]), vec=kr.vector(n, [seed, 3]), touch=touch,
                extended=extended)


def ref_az_build(c):
    """(cnt, ptr, oa, ov, overflow): per row the aggregates of its field columns in the order of their first appearance, every sum in
    storage order in float64 (adds only: the kernel's value); a 65th aggregate of a row sets overflow and is left out"""
    n, off, N, rp, ci, v, agg = c["n"], c["off"], c["N"], c["rp"], c["ci"], c["v"], c["agg"]
    cnt, oa, ov, overflow = np.zeros(n, dtype=np.int32), [], [], 0
    for i in range(n):
        la, ls = [], []
        for k in range(rp[i], rp[i + 1]):
            j = int(ci[k]) - off
            if j < 0 or j >= N or agg[j] < 0:
                continue
            a = int(agg[j])
            if a not in la:
                if len(la) == AZ_CAP:
                    overflow = 1
                    continue
                la.append(a)
                ls.append(np.float64(0.0))
            q = la.index(a)
            ls[q] = ls[q] + v[k]
        cnt[i] = len(la)
        oa += la
        ov += ls
    return cnt, gr.ref_scan(cnt), np.asarray(oa, dtype=np.int32), np.asarray(ov, dtype=np.float64), overflow


def ref_az_apply(ptr, oa, ov, u, vec):
    """(out, magnitude, T) in longdouble: out = vec - (A Z) u, or (A Z) u with vec = None; magnitude = |vec_i| + sum |ov u|"""
    n = len(ptr) - 1
    rows = gr.rows_of(ptr)
    p = ov.astype(LD) * u.astype(LD)[oa]
    acc, mag = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    np.add.at(acc, rows, p)
    np.add.at(mag, rows, np.abs(p))
    if vec is None:
        return acc, mag, np.diff(ptr)
    return vec.astype(LD) - acc, np.abs(vec.astype(LD)) + mag, np.diff(ptr)


def check_az_apply(out, ref, mag, T):
    err = np.abs(np.asarray(out, dtype=np.float64).astype(LD) - ref)
    bound = (T + 1).astype(LD) * LD(U) * mag
    return bool(np.all(np.isfinite(out)) and np.all(err <= bound)), kr._ratio(err, bound)


def az_apply64(ptr, oa, ov, u, vec):
    """float64 in the kernel's order"""
    out = np.zeros(len(ptr) - 1)
    for i in range(len(out)):
        acc = 0.0
        for k in range(ptr[i], ptr[i + 1]):
            acc += ov[k] * u[oa[k]]
        out[i] = acc if vec is None else vec[i] - acc
    return out


# ---- the entries ------------------------------------------------------------------------------------------------------------------
_ll, _i, _d = gr._ll, gr._i, gr._d


def _c(a):
    return None if a is None else np.ascontiguousarray(a)


def dev_assemble(L, c, diagScale, null_E=False, **over):
    """-> (rc, E as nagg x nagg, the guard behind it); over: entries of the case replaced for this call"""
    a = dict(c, **over)
    nagg = a["nagg"]
    m = min(max(nagg, 1), MAX_AGG)
    E = np.full(m * m + GUARD, SENTINEL)
    rc = L.das_debug_coarse_assemble(nagg, a["N"], a["off"], a["n"], _ll(a["rp"]), _i(a["ci"]), _d(a["v"]), _i(a["aggRow"]), _i(a["aggCol"]), a["transpose"], diagScale,
                                     None if null_E else _d(E))
    return rc, E[: m * m].reshape(m, m), E[m * m:]


def dev_invert(L, A, n=None):
    """-> (rc, Inv, singular, guard)"""
    n = A.shape[0] if n is None else n
    m = min(max(n, 1), MAX_AGG)
    Inv, sing = np.full(m * m + GUARD, SENTINEL), C.c_int(-7)
    A = np.ascontiguousarray(A, dtype=np.float64)
    rc = L.das_debug_coarse_invert(n, _d(A), _d(Inv), C.byref(sing))
    return rc, Inv[: m * m].reshape(m, m), sing.value, Inv[m * m:]


def dev_correct(L, c, y0, set_, **over):
    """-> (rc, t, u, y): t and u with their guard, y as long as y0; over: entries of the case (r, Einv, ...) replaced for this call"""
    a = dict(c, **over)
    m = min(max(a["nagg"], 1), MAX_AGG)
    t, u, y = np.full(m + GUARD, SENTINEL), np.full(m + GUARD, SENTINEL), y0.copy()
    Einv = _c(a["Einv"])
    rc = L.das_debug_coarse_correct(a["nagg"], a["N"], a["off"], a["n"], _i(a["agg"]), _d(Einv), _d(a["r"]), _d(t), _d(u), _d(y), len(y), set_)
    return rc, t, u, y


def dev_az(L, c, use_vec, cap, guard=7, **over):
    """-> (rc, cnt, ptr, oa, ov, nnz, overflow, out): cnt and ptr with GUARD entries behind n and n + 1, oa and ov cap entries, out
    n + guard; integers prefilled with -7, doubles with the sentinel"""
    a = dict(c, **over)
    n = a["n"]
    m = min(max(n, 1), 1 << 20)
    cnt, ptr = np.full(m + GUARD, -7, dtype=np.int32), np.full(m + 1 + GUARD, -7, dtype=np.int64)
    oa, ov, out = np.full(max(cap, 1), -7, dtype=np.int32), np.full(max(cap, 1), SENTINEL), np.full(max(m + guard, 1), SENTINEL)
    nnz, ovf = C.c_longlong(-7), C.c_int(-7)
    rc = L.das_debug_coarse_az(a["nagg"], n, _ll(a["rp"]), _i(a["ci"]), _d(a["v"]), a["N"], a["off"], _i(a["agg"]), _i(cnt), _ll(ptr), _i(oa), _d(ov), cap,
                               C.byref(nnz), C.byref(ovf), _d(a["u"]), _d(a["vec"]) if use_vec else None, _d(out), m + guard)
    return rc, cnt, ptr, oa, ov, nnz.value, ovf.value, out

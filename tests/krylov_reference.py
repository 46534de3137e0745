"""The Krylov kernels of the GMRES engine restated in a few lines of numpy in np.longdouble, the inputs that make every position of
a vector count, and the comparison functions with their DERIVED bounds (u = 2^-53):

  sum of T products, any order, FMA or not:      |got - ref| <= T u sum_i |x_i y_i|
  updated entry built from T terms, scaled:      |got - ref| <= (T + 2) u |scale| (sum of the absolute values of the terms)
  split output hi, lo of x:                      |hi + lo - x| <= the bound above + max(2^-48 |x|, 2^-150)  and  hi == float32(hi + lo)
  fp32 output of x:                              float32(x) to one fp32 ulp

The references are computed from the STORED values a kernel reads (fp32 / split: the float arrays, widened), so that storage
rounding is not part of the error being judged.  Used by tests/test_gpu_krylov_kernels.py (kernels on the device) and by
tests/test_krylov_reference_cpu.py (the restatements against mpmath, and the comparison functions against wrong results)."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
FP64, FP32, SPLIT = 0, 1, 2
FMT_NAMES = {FP64: "fp64", FP32: "fp32", SPLIT: "split"}
SENTINEL = -6.0e30  # exactly representable neither matters nor is needed: it is compared after the cast to the array's type

# ---- shapes -------------------------------------------------------------------------------------------------------------------
# every tail and dispatch branch of the kernels: thread block 256, update block 512, MD_CHUNK 1024, MD2_CHUNK 4096, the row chunks
# of the TN product (rowsPerChunk 16 -> 32 at n = 16 * 1024 + 1; n = 40000: ceil(n / 1024) = 40 is no multiple of 16)
N_LIST = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025, 4095, 4096, 4097, 8193, 16 * 1024 - 1, 16 * 1024 + 1, 40000, 2 ** 20 + 1]
K_LIST = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 129]
J_LIST = [0, 1, 3, 4, 5, 8, 9]
S_LIST = [1, 2, 3, 4, 5, 6, 7, 8]
MAX_DOUBLES = 2e7


def nk_shapes():
    """(n, K): every n with K = 1, 5, 9 and every K with n = 17, 4097, 16 * 1024 + 1 (n K <= 2e7 doubles)"""
    out = []
    for n in N_LIST:
        for K in (1, 5, 9):
            out.append((n, K))
    for K in K_LIST:
        for n in (17, 4097, 16 * 1024 + 1):
            out.append((n, K))
    return sorted({p for p in out if p[0] * p[1] <= MAX_DOUBLES})


def nj_shapes():
    """(n, j) of the fused update: every n with j = 0, 5 and every j with n = 513, 1025"""
    out = [(n, j) for n in N_LIST for j in (0, 5)] + [(n, j) for j in J_LIST for n in (513, 1025)]
    return sorted({p for p in out if p[0] * (p[1] + 3) <= MAX_DOUBLES})


def ns_shapes():
    """(n, s) of the block kernels: every s with n = 65, 4097 and every n with s = 3, 8"""
    out = [(n, s) for n in (65, 4097) for s in S_LIST] + [(n, s) for n in N_LIST for s in (3, 8)]
    return sorted(set(out))


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def vector(n, seed, ill=False):
    """standard-normal entries pushed away from zero (|x| >= 0.5): a dropped or misplaced element is a unit-size error.
    ill: entries scaled 1 .. 1e-12 down the rows, vector normalised"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(n)
    x = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.5 + np.abs(z))
    if ill:
        x = x * 10.0 ** (-12.0 * np.arange(n) / max(n - 1, 1))
        x = x / np.linalg.norm(x)
    return x


def vectors(n, K, seed, ill=False):
    """K vectors of length n, distinct per vector (reading vector i + 1 for i is a unit-size error)"""
    return np.stack([vector(n, [seed, i], ill) for i in range(K)]) if K > 0 else np.zeros((0, n))


def split32(x):
    """hi = float32(x), lo = float32(x - hi): the split storage of a basis entry"""
    x = np.asarray(x, dtype=np.float64)
    hi = x.astype(np.float32)
    lo = (x - hi.astype(np.float64)).astype(np.float32)
    return hi, lo


class Basis:
    """K basis vectors in one of the storage formats of the solver, in a flat array with leading dimension ld and the sentinel in
    the padding.  hi(i): what the inner products read; full(i): what the updates read (hi + lo); both widened to longdouble."""

    def __init__(self, V, fmt, ld, extra_slots=0):
        V = np.asarray(V, dtype=np.float64)
        K, n = V.shape
        assert ld >= (2 * n if fmt == SPLIT else n)
        self.fmt, self.n, self.ld, self.K = fmt, n, ld, K
        self.nslots = K + extra_slots
        self.a = np.full(self.nslots * ld, SENTINEL, dtype=np.float64 if fmt == FP64 else np.float32)
        st = self.a.reshape(self.nslots, ld)
        if fmt == FP64:
            st[:K, :n] = V
        elif fmt == FP32:
            st[:K, :n] = V.astype(np.float32)
        else:
            hi, lo = split32(V)
            st[:K, :n] = hi
            st[:K, n : 2 * n] = lo

    def slots(self):
        return self.a.reshape(self.nslots, self.ld)

    def width(self):
        return 2 * self.n if self.fmt == SPLIT else self.n

    def hi(self, i):
        return self.slots()[i, : self.n].astype(LD)

    def lo(self, i):
        return self.slots()[i, self.n : 2 * self.n].astype(LD) if self.fmt == SPLIT else LD(0.0)

    def full(self, i):
        return self.hi(i) + self.lo(i)

    def guard_intact(self, written_slots):
        """the padding of every slot and every slot beyond the written ones still hold the sentinel"""
        st = self.slots()
        sent = self.a.dtype.type(SENTINEL)
        return bool(np.all(st[:, self.width() :] == sent) and np.all(st[written_slots:, :] == sent))


# ---- the operations, restated (every function returns (reference, magnitude) as longdouble arrays) -------------------------------
def ref_dot(x, y):
    p = np.asarray(x, dtype=LD) * np.asarray(y, dtype=LD)
    return p.sum(), np.abs(p).sum()


def ref_dots(B, m, x):
    """V_i^hi . x for i < m"""
    x = np.asarray(x, dtype=LD)
    r = [ref_dot(B.hi(i), x) for i in range(m)]
    return np.array([a for a, _ in r], dtype=LD), np.array([b for _, b in r], dtype=LD)


def ref_dots2(B, v):
    """[V^T u ; V^T v] with u = slot K - 1 (the inner products read the hi array)"""
    ru, mu = ref_dots(B, B.K, B.hi(B.K - 1))
    rv, mv = ref_dots(B, B.K, v)
    return np.concatenate([ru, rv]), np.concatenate([mu, mv])


def ref_multidot(B, m, w):
    r, g = ref_dots(B, m, w)
    ww, gw = ref_dot(w, w)
    return np.append(r, ww), np.append(g, gw)


def ref_combination(B, m, c, lo=True):
    """sum_i c_i V_i over the first m vectors (hi + lo)"""
    acc, mag = np.zeros(B.n, dtype=LD), np.zeros(B.n, dtype=LD)
    for i in range(m):
        t = LD(c[i]) * (B.full(i) if lo else B.hi(i))
        acc += t
        mag += np.abs(t)
    return acc, mag


def ref_multiaxpy(B, m, h, w, lo=True):
    """w - sum_i h_i V_i"""
    acc, mag = ref_combination(B, m, h, lo)
    w = np.asarray(w).astype(LD)
    return w - acc, np.abs(w) + mag


def ref_dcgs2_update(B, j, sc, gamma, ralpha, v, lo=True):
    """q_j = (u - Q s) ralpha, u' = (v - gamma u - Q c) ralpha with u = slot j; returns ((q, magq), (un, magun)), unscaled magnitudes"""
    u = B.full(j) if lo else B.hi(j)
    qs, ms = ref_combination(B, j, sc[:j], lo)
    qc, mc = ref_combination(B, j, sc[j : 2 * j], lo)
    v = np.asarray(v, dtype=LD)
    q = (u - qs) * LD(ralpha)
    un = (v - LD(gamma) * u - qc) * LD(ralpha)
    return (q, np.abs(u) + ms), (un, np.abs(v) + np.abs(LD(gamma) * u) + mc)


def ref_scale(a, x):
    r = LD(a) * np.asarray(x, dtype=LD)
    return r, np.abs(np.asarray(x, dtype=LD))


def ref_block_tn(V, W):
    """C[i, r] = V_i . W_r (rows of V and W are the vectors)"""
    K, s = V.shape[0], W.shape[0]
    C, M = np.zeros((K, s), dtype=LD), np.zeros((K, s), dtype=LD)
    Wl = W.astype(LD)
    for i in range(K):
        p = V[i].astype(LD)[None, :] * Wl
        C[i], M[i] = p.sum(axis=1), np.abs(p).sum(axis=1)
    return C, M


def ref_block_comb(V, C):
    """Y_r = sum_i V_i C[i, r]; returns (Y, magnitude), s x n"""
    K, n = V.shape
    s = C.shape[1]
    Y, M = np.zeros((s, n), dtype=LD), np.zeros((s, n), dtype=LD)
    for i in range(K):
        vi = V[i].astype(LD)
        for r in range(s):
            t = vi * LD(C[i, r])
            Y[r] += t
            M[r] += np.abs(t)
    return Y, M


def ref_block_nn_sub(V, C, W):
    Y, M = ref_block_comb(V, C)
    return W.astype(LD) - Y, np.abs(W.astype(LD)) + M


def ref_right_mult(W, T):
    """(W T)_c = sum_r W_r T[r, c]"""
    return ref_block_comb(W, T)


def ref_csr_rows(rp, ci, val, X):
    """Y_r[row] = sum over the row's entries of val x_r[col], row by row; X: s x n.  Returns (Y, magnitude, row lengths)"""
    n, s = len(rp) - 1, X.shape[0]
    Xl = X.astype(LD)
    Y, M = np.zeros((s, n), dtype=LD), np.zeros((s, n), dtype=LD)
    for i in range(n):
        b, e = rp[i], rp[i + 1]
        if e > b:
            p = val[b:e].astype(LD)[None, :] * Xl[:, ci[b:e]]
            Y[:, i], M[:, i] = p.sum(axis=1), np.abs(p).sum(axis=1)
    return Y, M, np.diff(rp)


ROW_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 280]


def make_csr(n, seed, last="empty", ill=False):
    """rows of length 0, 1, 15, 16, 17, 63, 64, 65, 280 mixed, an empty first row, repeated column indices in the rows, unsorted
    columns; last = "empty": an empty last row, "longest": the 280-entry row last.  Returns (rowptr int64, colidx int32, values)"""
    assert n >= 3
    rng = np.random.default_rng(seed)
    lens = [ROW_LENGTHS[(4 * i + 1) % len(ROW_LENGTHS)] for i in range(n)]
    lens[0] = 0
    lens[-1] = 0 if last == "empty" else 280
    if last != "empty":
        lens = [min(x, 65) for x in lens[:-1]] + [280]
    rp = np.zeros(n + 1, dtype=np.int64)
    rp[1:] = np.cumsum(lens)
    ci = rng.integers(0, n, size=rp[-1]).astype(np.int32)  # with replacement: repeated indices wherever a row is longer than a few
    for i in range(n):  # and at least one certain repeat in every row of two or more entries
        if lens[i] >= 2:
            ci[rp[i] + 1] = ci[rp[i]]
    val = vector(int(rp[-1]), [seed, 1])
    if ill:
        val = val * 10.0 ** (-12.0 * rng.random(val.size))
    return rp, ci, val


# ---- comparison: each returns (ok, achieved max err / (u magnitude)) -----------------------------------------------------------
def _ratio(err, unit):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(unit > 0, err / unit, np.where(err > 0, np.inf, 0.0))
    return float(np.max(r)) if np.size(r) else 0.0


def check_sum(got, ref, mag, T):
    """a sum of T products: |got - ref| <= T u mag (T scalar or per entry; an empty sum must be exactly zero)"""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    err = np.abs(got - ref)
    unit = LD(U) * mag
    ok = bool(np.all(np.isfinite(got)) and np.all(err <= np.asarray(T, dtype=LD) * unit))
    return ok, _ratio(err, unit)


def update_bound(mag, T, scale=1.0):
    return LD(T + 2) * LD(U) * abs(LD(scale)) * mag


def check_update(got, ref, mag, T, scale=1.0):
    """an entry built from T terms and scaled: |got - ref| <= (T + 2) u |scale| mag"""
    got = np.asarray(got, dtype=np.float64).astype(LD)
    err = np.abs(got - ref)
    ok = bool(np.all(np.isfinite(got)) and np.all(err <= update_bound(mag, T, scale)))
    return ok, _ratio(err, LD(U) * abs(LD(scale)) * mag)


def check_split(hi, lo, ref, mag, T, scale=1.0):
    """hi + lo against x = ref: the update bound + max(2^-48 |x|, 2^-150), and hi is the ROUNDED value: hi == float32(hi + lo) in fp64"""
    hi = np.asarray(hi, dtype=np.float32)
    lo = np.asarray(lo, dtype=np.float32)
    s64 = hi.astype(np.float64) + lo.astype(np.float64)
    err = np.abs(s64.astype(LD) - ref)
    bound = update_bound(mag, T, scale) + np.maximum(LD(2.0 ** -48) * np.abs(ref), LD(2.0 ** -150))
    ok = bool(np.all(np.isfinite(s64)) and np.all(err <= bound) and np.all(hi == s64.astype(np.float32)))
    return ok, _ratio(err, LD(U) * abs(LD(scale)) * mag)


def check_fp32(got, ref):
    """float32(x) to one fp32 ulp; the figure is the error in ulps"""
    got = np.asarray(got, dtype=np.float32)
    want = np.asarray(ref, dtype=np.float64).astype(np.float32)
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ok = bool(np.all(np.isfinite(got)) and np.all(err <= ulp))
    return ok, _ratio(err, ulp)

"""Plain restatements of the objective-function reductions (csrc/das_facefn.hpp, das_cellfn.hpp, das_meshquality.hpp, das_heatsource.hpp,
das_actuatordisk.hpp, das_reduce.hpp), the makers of their test inputs, the derived error bounds and the wrappers of the test-only
entries das_debug_reduce_* (test_reduce_reference_cpu.py checks this module without a GPU, test_gpu_reduce_kernels.py uses it on one).

Sums are math.fsum (the correctly rounded sum), exponentials np.longdouble, rn_term / rn_seed plain Python.

THE SUMMATION BOUND.  u = 2^-53.  A sum of terms t_i computed in floating point along a tree in which every leaf-to-root path passes at
most d additions satisfies |computed - exact| <= ((1 + u)^d - 1) sum |t_i|, taken here as d u sum |t_i| (the accumulators start at an
exact 0.0, so the first addition of every path is exact: (1 + u)^(d - 1) - 1 <= d u for every d that occurs).  d is counted from the
kernels:
  shuffle pairs (k_ks_expsum / k_rn_partial / k_cellfn_value / k_hs_partial / k_ad_dot_partial + their one-workgroup finals):
      stage 1: trips1 = ceil(n / (256 nb)) additions in the grid-stride loop of a thread, 6 shuffle steps (32, 16, .. 1), 2 LDS additions
               ((sh0 + sh1) + (sh2 + sh3));
      stage 2: trips2 = ceil(nb / 256) additions per thread, 6 shuffle steps, 2 LDS additions:   d = trips1 + trips2 + 16
  LDS-tree pairs (k_sv_dot / k_tangent_dot + k_group_sum): each stage ends in a 256-entry tree of 8 levels (128, 64, .. 1):
      stage 1: trips1 + 8;  stage 2 (k_group_sum over nb partials): ceil(nb / 256) + 8:           d = trips1 + trips2 + 16
  k_group_sum alone over cnt entries:                                                              d = ceil(cnt / 256) + 8
The error itself is formed without rounding of its own: fsum(terms + [-device]) is the correctly rounded value of exact - device.
Where the terms are products, the test inputs carry at most 24 significant bits, so that every product is exact in fp64 (contracted into
an fma or not) and the terms of the reference are the terms of the kernel; the residualNorm sum is judged on the device's own terms,
which are compared bit by bit first.

THE KS BOUND.  The kernel forms x_i = k a_i - m in fp64 (two roundings, or one where the compiler contracts), then exp.  Against
e_i = exp(k a_i - m) in longdouble with the exact m: |x_i(device) - x_i| <= delta_i = u (|k a_i| + |x_i|), so
  |t_i - e_i| <= e_i (expm1(delta_i) + E 2^-52 (1 + expm1(delta_i)))
where E is the error of the device's exp in ulps - NOT assumed: measured on the device, on the test's own arguments
(measure_exp_ulps: a launch in which every workgroup holds ONE argument next to entries whose exponential underflows to an exact 0, so
that its partial IS exp(x)).  The KS inputs draw from a palette of at most 1000 values so that every argument of a case can be measured
in two launches.  S then carries the sum of those term bounds plus the summation bound; a weight w_i = outer t_i / S two more roundings
and the relative error of S."""
import ctypes as C
import functools
import math

import numpy as np

U = 2.0 ** -53
SENT = -7.25                      # fill value of the output arrays: never a result of a test
CAP, SV_CAP, TD_BLOCKS = 1024, 512, 1024
SIZES = [1, 63, 64, 65, 255, 256, 257, 65536 + 1, 512 * 256 + 1, 1024 * 256, 1024 * 256 + 1, 3 * 1024 * 256 + 77]
SMALL = [n for n in SIZES if n <= 257]
EXP_UNDERFLOW = -746.0            # exp(x) rounds to an exact 0.0 in fp64 for x < -745.14


def ceil_div(a, b):
    return -(-a // b)


def blocks(n, cap=CAP):
    """the workgroups of a first stage: max(1, min(cap, ceil(n / 256)))"""
    return max(1, min(cap, ceil_div(n, 256)))


def depth(n, nb):
    """d of a two-stage pair (see the module docstring); nb = the workgroups of stage 1"""
    return ceil_div(n, 256 * nb) + ceil_div(nb, 256) + 16


def depth_group(cnt):
    return ceil_div(cnt, 256) + 8


def error_of(terms, dev):
    """exact sum - dev, correctly rounded"""
    return math.fsum(list(terms) + [-float(dev)])


def bound(d, terms):
    return d * U * math.fsum(np.abs(np.asarray(terms, dtype=np.float64)))


def by_block(x, nb, fill):
    """x as the grid-stride loops see it: [trip, workgroup, thread], padded with fill"""
    x = np.asarray(x)
    trips = ceil_div(len(x), 256 * nb)
    full = np.full(trips * nb * 256, fill, dtype=x.dtype)
    full[:len(x)] = x
    return full.reshape(trips, nb, 256)


def block_sums_exact(x, nb):
    """per-workgroup sums of integer-valued x, exact (int64)"""
    xi = np.asarray(x).astype(np.int64)
    assert np.all(xi == x)
    return by_block(xi, nb, 0).sum(axis=(0, 2))


# ---- input makers -----------------------------------------------------------------------------------------------------------------------
def counting(n):
    """x_i = i + 1: every partial sum is an integer below 2^53, so every summation order is exact"""
    return np.arange(1, n + 1, dtype=np.float64)


def small_ints(n, seed, lo=-9, hi=9):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=n).astype(np.float64)


def bits24(x):
    """x rounded to 24 significant bits: products of two such values are exact in fp64"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def mixed(n, seed):
    """random values of mixed sign over six decades, 24 significant bits"""
    rng = np.random.default_rng(seed)
    return bits24(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, size=n))


def ill_conditioned(n, seed):
    """large cancelling pairs plus small terms: sum |x| / |sum x| >= 1e8 (n >= 3); 24 significant bits"""
    rng = np.random.default_rng(seed)
    x = bits24(rng.uniform(0.5, 1.5, size=n) * 1e-4)
    big = bits24(rng.uniform(1.0, 2.0, size=n // 3) * 1e9)
    pos = rng.permutation(n)[:2 * (n // 3)]
    x[pos[0::2]] = big
    x[pos[1::2]] = -big
    return x


def condition(x):
    return math.fsum(np.abs(x)) / abs(math.fsum(x))


def duals(d, seed):
    """n dual numbers {value, tangent} as an (n, 2) array: the values are of magnitude 1e30, the tangents are d"""
    rng = np.random.default_rng(seed)
    R = np.empty((len(d), 2))
    R[:, 0] = rng.uniform(1.0, 2.0, size=len(d)) * 1e30 * rng.choice([-1.0, 1.0], size=len(d))
    R[:, 1] = d
    return R


# ---- KS ---------------------------------------------------------------------------------------------------------------------------------
def ks_palette(n, k, seed, where_max, count=1000, spread=30.0, base=1.0):
    """a[n] drawn from `count` values in [base, base + spread / |k|], the extreme (the maximum of k a) ONCE, at index where_max"""
    rng = np.random.default_rng(seed)
    pal = np.unique(rng.uniform(base, base + spread / abs(k), size=count))
    # the extreme is a multiple of 2^-20 and k has few bits, so that k a is exact there: under contraction exp would otherwise see the
    # POSITIVE argument k a - fl(k a), which no measuring launch can reproduce (exp_probe)
    top = math.ceil(pal[-1] * 2 ** 20 + 1) / 2 ** 20 if k > 0 else math.floor(pal[0] * 2 ** 20 - 1) / 2 ** 20
    assert float(k * 4).is_integer() and abs(k * 4) < 2 ** 10 and abs(top) < 2 ** 20  # a 12-bit k times a 40-bit a: exact
    rest = pal[:-1] if k > 0 else pal[1:]
    a = rng.choice(rest, size=n)
    a[where_max] = top
    return a


def wide_spread(n, k=2.0):
    """(a, k, alive): five entries with k (a - max) in [-24, 0] (fewer where n < 5), every other one below -800 - its exponential and its
    weight are an exact 0 in fp64"""
    rng = np.random.default_rng(9)
    a = 10.0 - (900.0 + 200.0 * rng.random(n)) / abs(k) * np.sign(k)
    alive = np.unique(np.array([0, 300, n // 2, n - 2, n - 1]) % n)
    a[alive] = 10.0 - 3.0 * np.arange(len(alive)) * np.sign(k)
    return a, k, alive


def ks_reference(a, k):
    """(m, e, S): m = max fl(k a_i) as the kernel forms it (fp64), e_i = exp(k a_i - m) and S = sum e_i in longdouble; an argument
    below EXP_UNDERFLOW counts as the exact 0 it is in fp64"""
    a = np.asarray(a, dtype=np.float64)
    m = float(np.max(k * a))
    x = np.longdouble(k) * a.astype(np.longdouble) - np.longdouble(m)
    e = np.where(x < EXP_UNDERFLOW, np.longdouble(0), np.exp(x))
    return m, e, e.sum(dtype=np.longdouble)


def ks_arguments(a, k, m):
    """the fp64 arguments the device may hand to exp: two roundings, and the contracted single rounding"""
    a = np.asarray(a, dtype=np.float64)
    two = k * a - m
    one = (np.longdouble(k) * a.astype(np.longdouble) - np.longdouble(m)).astype(np.float64)  # 64-bit product: the double rounding is below delta
    return np.unique(np.concatenate([two, one]))


def ks_term_bounds(a, k, m, e, E):
    """per-term bound on |t_i - e_i| (module docstring), longdouble"""
    L = np.longdouble
    ka = np.abs(L(k) * np.asarray(a, dtype=np.float64).astype(L))
    x = np.abs(L(k) * np.asarray(a, dtype=np.float64).astype(L) - L(m))
    grow = np.expm1(L(U) * (ka + x))
    return e * (grow + L(E) * L(2.0 ** -52) * (1 + grow))


def ks_sum_bound(n, a, k, m, e, E):
    nb = blocks(n)
    return float(ks_term_bounds(a, k, m, e, E).sum(dtype=np.longdouble) + np.longdouble(depth(n, nb) * U) * e.sum(dtype=np.longdouble) * (1 + 2 * E * 2.0 ** -52))


def ks_unshifted(a, k):
    """log(sum exp(k a)) / k without the shift, longdouble: representable while k a stays below 11000"""
    x = np.longdouble(k) * np.asarray(a, dtype=np.float64).astype(np.longdouble)
    return np.log(np.exp(x).sum(dtype=np.longdouble)) / np.longdouble(k)


def exp_probe(args):
    """the input of a measuring launch for at most 1023 arguments x <= 0: k = 1, workgroup b holds args[b] at its first thread, the last
    workgroup the maximum 0, every other entry -1e6 (its exponential is an exact 0): psum[b] = exp(args[b])"""
    args = np.asarray(args, dtype=np.float64)
    assert len(args) <= CAP - 1 and np.all(args <= 0.0)
    a = np.full(CAP * 256, -1.0e6)
    a[np.arange(len(args)) * 256] = args
    a[(CAP - 1) * 256] = 0.0
    return a


def measure_exp_ulps(L, args):
    """the largest error of the device's exp over args, in ulps of the result, against longdouble"""
    args = np.unique(np.asarray(args, dtype=np.float64))
    args = args[args >= -700.0]  # below: subnormal results or exact zeros, which the cases that have them assert directly
    worst = 0.0
    for i in range(0, len(args), CAP - 1):
        chunk = args[i:i + CAP - 1]
        rc, r = dev_ks(L, exp_probe(chunk), 1.0)
        assert rc == 0 and r["m"] == 0.0
        got = r["psum"][:len(chunk)]
        ref = np.exp(chunk.astype(np.longdouble))
        ulp = np.spacing(ref.astype(np.float64)).astype(np.longdouble)
        worst = max(worst, float(np.max(np.abs(got.astype(np.longdouble) - ref) / ulp)))
    return worst


# ---- residualNorm -----------------------------------------------------------------------------------------------------------------------
KIND_VEC, KIND_SCL, KIND_FACE = 0, 1, 2


def rn_layout():
    """all three block kinds with distinct weights, one of them zero, a flux block with nIF < nF and rows that fall in no block:
    [U 3 nC | p nC | gap 5 | nuTilda nC (weight 0) | phi nF | gap 3]"""
    nC, nF, nIF = 37, 130, 101
    blocks_ = [(0, KIND_VEC, 1.5), (3 * nC, KIND_SCL, -0.25), (4 * nC + 5, KIND_SCL, 0.0), (5 * nC + 5, KIND_FACE, 3.0)]
    return {"nC": nC, "nF": nF, "nIF": nIF, "blocks": blocks_, "n": 5 * nC + 5 + nF + 3}


def rn_tiled(n):
    """a layout of n rows for the sizes of the grid arithmetic: the proportions of rn_layout scaled to n (a gap of the last rows in no block)"""
    nC = max(1, n // 8)
    nF = max(0, n - 5 * nC - 3)
    nIF = (2 * nF) // 3
    blocks_ = [(0, KIND_VEC, 2.0), (3 * nC, KIND_SCL, -3.0), (4 * nC, KIND_SCL, 0.0), (5 * nC, KIND_FACE, 5.0)]
    return {"nC": nC, "nF": nF, "nIF": nIF, "blocks": blocks_, "n": n}


def rn_weight(lay, i):
    """(weight of row i, the row is an internal face of a flux block); the first block that holds the row, 0 where none does"""
    for off, kind, w in lay["blocks"]:
        length = 3 * lay["nC"] if kind == KIND_VEC else lay["nC"] if kind == KIND_SCL else lay["nF"]
        q = i - off
        if 0 <= q < length:
            return w, kind == KIND_FACE and q < lay["nIF"]
    return 0.0, False


def rn_term(lay, l1, i, R):
    w, ip = rn_weight(lay, i)
    return abs(w * R) if (l1 and not ip) else w * w * R * R


def rn_seed(lay, l1, i, R, F):
    w, ip = rn_weight(lay, i)
    if not l1:
        return w * w * R / F
    if ip:
        return 2.0 * w * w * R
    return abs(w) if R > 0.0 else -abs(w) if R < 0.0 else 0.0


def rn_rows(lay):
    """(weight per row, internal-flux flag per row) as arrays: rn_weight for every row at once"""
    w = np.zeros(lay["n"])
    ip = np.zeros(lay["n"], dtype=bool)
    taken = np.zeros(lay["n"], dtype=bool)
    for off, kind, wt in lay["blocks"]:
        length = 3 * lay["nC"] if kind == KIND_VEC else lay["nC"] if kind == KIND_SCL else lay["nF"]
        lo, hi = max(off, 0), min(off + length, lay["n"])
        if hi <= lo:
            continue
        sel = np.zeros(lay["n"], dtype=bool)
        sel[lo:hi] = True
        sel &= ~taken
        w[sel] = wt
        if kind == KIND_FACE:
            q = np.arange(lay["n"]) - off
            ip[sel & (q < lay["nIF"])] = True
        taken |= sel
    return w, ip


def rn_terms_np(lay, l1, R):
    """rn_term for every row, the same operations in the same order (test_reduce_reference_cpu.py: equal to the plain-Python loop bit by bit)"""
    w, ip = rn_rows(lay)
    sq = w * w * R * R
    return np.where(ip, sq, np.abs(w * R)) if l1 else sq


def rn_seeds_np(lay, l1, R, F, coef):
    w, ip = rn_rows(lay)
    if not l1:
        return coef * (w * w * R / F)
    return coef * np.where(ip, 2.0 * w * w * R, np.where(R > 0.0, np.abs(w), np.where(R < 0.0, -np.abs(w), 0.0)))


# ---- gathers ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cell_faces(nC=1000, nIF=2500, nF=3100, seed=3):
    """a cell-face list as the mesh holds it: per cell 0 to 9 entries; an entry is the face (the cell owns it) or the face with the top bit
    set (the cell is its neighbour); cf_other = the cell across (boundary faces f >= nIF: -1)"""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 10, size=nC)
    cnt[[0, 5, nC - 1]] = [0, 9, 9]
    ptr = np.zeros(nC + 1, dtype=np.int32)
    ptr[1:] = np.cumsum(cnt)
    face = rng.integers(0, nF, size=ptr[-1]).astype(np.int64)
    other = np.where(face < nIF, rng.integers(0, nC, size=ptr[-1]), -1).astype(np.int32)
    nei = (rng.random(ptr[-1]) < 0.4) & (face < nIF)
    enc = np.where(nei, face | 0x80000000, face).astype(np.uint32).view(np.int32)
    return nC, nIF, nF, ptr, enc, other


def owner_gather(ptr, enc, ft):
    """tc[c] = the sum of ft over the owned faces in list order, the additions one by one as the kernel makes them"""
    tc = np.zeros(len(ptr) - 1)
    for c in range(len(ptr) - 1):
        acc = 0.0
        for s in range(ptr[c], ptr[c + 1]):
            if enc[s] >= 0:
                acc += float(ft[enc[s]])
        tc[c] = acc
    return tc


def vm_gather(nIF, ptr, enc, other, colors, col, tc, seed, out):
    out = out.copy()
    for j in range(3 * (len(ptr) - 1)):
        if colors[j] != col:
            continue
        c = j // 3
        acc = float(tc[c])
        for s in range(ptr[c], ptr[c + 1]):
            if (int(enc[s]) & 0x7fffffff) < nIF:
                acc += float(tc[other[s]])
        out[j] = seed * acc
    return out


# ---- wrappers of the entries: every array goes down and comes back whole ------------------------------------------------------------------
def _d(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _i(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def _ll(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_longlong))


def _ub(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_ubyte))


def out_array(n, guard=8):
    return np.full(n + guard, SENT)


def guard_intact(a, n):
    return bool(np.all(a[n:] == SENT))


def same(a, b):
    """bitwise equality of two float arrays (NaN patterns and signed zeros included)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


def dev_ks(L, a, k, outer=1.0):
    a = np.ascontiguousarray(a, dtype=np.float64)
    ain, n = a.copy(), len(a)
    ms, pmax, psum, w, nb = out_array(2), out_array(CAP), out_array(CAP), out_array(n), C.c_int(-1)
    rc = L.das_debug_reduce_ks(n, _d(ain), k, outer, _d(ms), len(ms), _d(pmax), _d(psum), len(pmax), _d(w), len(w), C.byref(nb))
    return rc, {"m": ms[0], "S": ms[1], "ms": ms, "pmax": pmax, "psum": psum, "w": w, "nb": nb.value, "inputs": same(ain, a)}


def dev_group_sum(L, fv, group):
    fv = np.ascontiguousarray(fv, dtype=np.float64)
    fin, gin, out = fv.copy(), None if group is None else np.ascontiguousarray(group, dtype=np.uint8).copy(), out_array(2)
    rc = L.das_debug_reduce_group_sum(len(fv), _ub(gin), _d(fin), _d(out), len(out))
    return rc, {"out": out, "inputs": same(fin, fv) and (group is None or bool(np.all(gin == group)))}


def _dot(fn, first, second, cap, nout):
    first, second = np.ascontiguousarray(first, dtype=np.float64), np.ascontiguousarray(second, dtype=np.float64)
    f, s, part, out, nb = first.copy(), second.copy(), out_array(cap), out_array(nout), C.c_int(-1)
    rc = fn(len(second), _d(f), _d(s), _d(part), len(part), _d(out), len(out), C.byref(nb))
    return rc, {"out": out, "part": part, "nb": nb.value, "inputs": same(f, first) and same(s, second)}


def dev_tangent_dot(L, R, psi):
    return _dot(L.das_debug_reduce_tangent_dot, R, psi, TD_BLOCKS, 2)


def dev_ad_dot(L, R, psi):
    return _dot(L.das_debug_reduce_ad_dot, R, psi, CAP, 1)


def dev_sv_dot(L, a, b):
    return _dot(L.das_debug_reduce_sv_dot, a, b, SV_CAP, 2)


def dev_cellfn(L, cell, idx, data, square, mv, V, src, coef, sc, g):
    cell, idx = np.ascontiguousarray(cell, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int64)
    ci, ii, di, si, sci = cell.copy(), idx.copy(), None if data is None else data.copy(), src.copy(), None if sc is None else sc.copy()
    part, out, grad, nb = out_array(CAP), out_array(1), out_array(len(src)), C.c_int(-1)
    rc = L.das_debug_reduce_cellfn(len(cell), _i(ci), _ll(ii), _d(di), int(square), int(mv), len(V), _d(np.ascontiguousarray(V)), len(src), _d(si), coef, _d(part),
                                   len(part), _d(out), len(out), _d(sci), g, _d(grad), len(grad), C.byref(nb))
    ok = bool(np.all(ci == cell) and np.all(ii == idx)) and same(si, src) and (data is None or same(di, data)) and (sc is None or same(sci, sc))
    return rc, {"out": out, "part": part, "grad": grad, "nb": nb.value, "inputs": ok}


def dev_rn(L, lay, l1, R, F, coef):
    R = np.ascontiguousarray(R, dtype=np.float64)
    n, Rin = len(R), R.copy()
    off = np.array([b[0] for b in lay["blocks"]], dtype=np.int64)
    kind = np.array([b[1] for b in lay["blocks"]], dtype=np.int32)
    w = np.array([b[2] for b in lay["blocks"]], dtype=np.float64)
    term, part, ms, g, nb = out_array(n), out_array(CAP), out_array(2), out_array(n), C.c_int(-1)
    rc = L.das_debug_reduce_rn(n, len(off), _ll(off), _i(kind), _d(w), lay["nC"], lay["nF"], lay["nIF"], int(l1), _d(Rin), _d(term), len(term), _d(part), len(part),
                               _d(ms), len(ms), F, coef, _d(g), len(g), C.byref(nb))
    return rc, {"term": term, "part": part, "ms": ms, "sum": ms[1], "g": g, "nb": nb.value, "inputs": same(Rin, R)}


HS_SET, HS_FIELD = 0, 2


def dev_hs_sum(L, kind, V, s, psi, byV, power, vt):
    """s: the member mask (kind HS_SET) or the field (HS_FIELD)"""
    mem = np.ascontiguousarray(s, dtype=np.uint8).copy() if kind == HS_SET else None
    fld = np.ascontiguousarray(s, dtype=np.float64).copy() if kind == HS_FIELD else None
    pin, vin = None if psi is None else psi.copy(), None if vt is None else np.array([vt], dtype=np.float64)
    part, out, nb = out_array(CAP), out_array(1), C.c_int(-1)
    rc = L.das_debug_reduce_hs_sum(kind, len(V), _d(np.ascontiguousarray(V)), _ub(mem), _d(fld), _d(pin), int(byV), power, _d(vin), _d(part), len(part), _d(out),
                                   len(out), C.byref(nb))
    ok = (mem is None or bool(np.all(mem == s))) and (fld is None or same(fld, s)) and (psi is None or same(pin, psi)) and (vt is None or vin[0] == vt)
    return rc, {"out": out, "part": part, "nb": nb.value, "inputs": ok}


def dev_final(L, pair, dual, nb, part):
    """part: (nb,) or (nb, 2) [pair] doubles, one axis of 2 more for dual numbers"""
    part = np.ascontiguousarray(part, dtype=np.float64)
    pin, width = part.copy(), (2 if pair else 1) * (2 if dual else 1)
    out = out_array(width)
    rc = L.das_debug_reduce_final(int(pair), int(dual), nb, _d(pin), pin.size, _d(out), len(out))
    return rc, {"out": out, "width": width, "inputs": same(pin, part)}


def dev_owner_gather(L, ptr, enc, ft):
    p, e, f, tc = ptr.copy(), enc.copy(), ft.copy(), out_array(len(ptr) - 1)
    rc = L.das_debug_reduce_owner_gather(len(ptr) - 1, _i(p), _i(e), len(ft), _d(f), _d(tc), len(tc))
    return rc, {"tc": tc, "inputs": bool(np.all(p == ptr) and np.all(e == enc)) and same(f, ft)}


def dev_vm_gather(L, nIF, ptr, enc, other, colors, col, tc, seed, out):
    p, e, o, c, t, res = ptr.copy(), enc.copy(), other.copy(), colors.copy(), tc.copy(), out.copy()
    rc = L.das_debug_reduce_vm_gather(len(ptr) - 1, nIF, _i(p), _i(e), _i(o), _i(c), col, _d(t), seed, _d(res), len(res))
    return rc, {"out": res, "inputs": bool(np.all(p == ptr) and np.all(e == enc) and np.all(o == other) and np.all(c == colors)) and same(t, tc)}

"""The reductions every objective function ends in - k_ks_max / k_ks_max_final / k_ks_expsum / k_ks_sum_final / k_ks_weights, k_cellfn_value
/ k_cellfn_sum / k_cellfn_grad, k_rn_terms / k_rn_partial / k_rn_seeds, k_hs_partial / k_hs_final, k_ad_final, k_ad_dot_partial,
k_tangent_dot, k_sv_dot, k_group_sum - and the gathers k_mq_owner_gather / k_vm_gather on the device, one by one, against the restatements
of tests/reduce_reference.py: no mesh, no solver.  The entries das_debug_reduce_* run the launch helpers the solver runs.  The sizes are
the smallest that reach every trip count of the capped grids (reduce_reference.SIZES): wave and workgroup edges, 257 partials (the second
trip of every final), the caps 512 and 1024, the first element of the second trip, three trips with a ragged tail.  Integer-valued inputs
must come out EXACTLY, partial by partial; rounding inputs within d u sum |terms| with d counted from the kernels (the module docstring of
reduce_reference.py); the exponentials within that plus the device's exp error, which is measured here and not assumed.  Every call is
made twice for identical bits; every output carries a guard band, every partial array must hold exactly nb written entries, every input
must come back as it went."""
import functools
import math

import numpy as np
import pytest

import reduce_reference as rr
from dafoam_amd import _capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")]
LD = np.longdouble
ROUNDING_SIZES = [257, 65536 + 1, 512 * 256 + 1, 1024 * 256 + 1, 3 * 1024 * 256 + 77]
SECOND_TRIP = 1024 * 256


def lib():
    return _capi.lib()


def run2(call):
    """the call twice: both succeed, every output is the same bits, the inputs came back untouched"""
    (rc1, r1), (rc2, r2) = call(), call()
    assert rc1 == 0 and rc2 == 0, lib().das_last_error()
    for key, v in r1.items():
        assert rr.same(v, r2[key]) if isinstance(v, np.ndarray) else v == r2[key], f"{key} differs between two runs"
    assert r1["inputs"], "the device changed an input array"
    return r1


def written(part, nb):
    """exactly the first nb entries of a partial array were written"""
    return bool(np.all(part[:nb] != rr.SENT) and np.all(part[nb:] == rr.SENT))


# ---- KS ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2.0, -2.0])
@pytest.mark.parametrize("n", rr.SIZES)
def test_ks_of_equal_entries_counts_them(n, k):
    """all entries equal (k a exact): m = k a, every exponential is exp(0) = 1, S = n exactly, every partial is the count of its workgroup,
    every weight is 1 / n"""
    r = run2(lambda: rr.dev_ks(lib(), np.full(n, 0.375), k))
    nb = rr.blocks(n)
    assert r["nb"] == nb and written(r["pmax"], nb) and written(r["psum"], nb) and rr.guard_intact(r["ms"], 2) and rr.guard_intact(r["w"], n)
    assert r["m"] == k * 0.375 and np.all(r["pmax"][:nb] == k * 0.375)
    assert r["S"] == n and np.array_equal(r["psum"][:nb], rr.block_sums_exact(np.ones(n), nb).astype(np.float64))
    assert np.all(r["w"][:n] == 1.0 / n)


@functools.lru_cache(maxsize=None)
def exp_error(n, k, seed, where, base=1.0, spread=30.0):
    """E in ulps on every argument the case can hand to exp (two launches of 1023 arguments at the most)"""
    a = rr.ks_palette(n, k, seed, where, spread=spread, base=base)
    E = rr.measure_exp_ulps(lib(), rr.ks_arguments(a, k, float(np.max(k * a))))
    print(f"device exp on the arguments of n {n} k {k}: {E:.3f} ulp")
    return E


def check_ks(a, k, r, E, outer):
    """m bitwise, the partial maxima exact; S, its partials and the weights within the derived bound at the measured E"""
    n, nb = len(a), rr.blocks(len(a))
    m, e, S = rr.ks_reference(a, k)
    assert r["nb"] == nb and written(r["pmax"], nb) and written(r["psum"], nb) and rr.guard_intact(r["ms"], 2) and rr.guard_intact(r["w"], n)
    assert r["m"] == m, "m is not max(k a) bit by bit"
    assert np.array_equal(r["pmax"][:nb], rr.by_block(k * a, nb, -np.inf).max(axis=(0, 2)))
    tb = rr.ks_term_bounds(a, k, m, e, E)
    bS = rr.ks_sum_bound(n, a, k, m, e, E)
    errS = abs(float(LD(r["S"]) - S))
    print(f"n {n} k {k}: S error {errS:.3e} bound {bS:.3e} (E {E:.3f} ulp)")
    assert errS <= bS
    trips = rr.ceil_div(n, 256 * nb)
    eb, tbb = rr.by_block(e, nb, LD(0)).sum(axis=(0, 2)), rr.by_block(tb, nb, LD(0)).sum(axis=(0, 2))
    errP = np.abs(r["psum"][:nb].astype(LD) - eb)
    bP = tbb + LD((trips + 8) * rr.U) * (eb + tbb)
    print(f"   partials: worst error / bound {float(np.max(errP[bP > 0] / bP[bP > 0])):.3f}")
    assert np.all(errP <= bP)
    relS = LD(bS) / S
    wref = LD(outer) * e / S
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(e > 0, tb / e, LD(0))
    bW = np.abs(wref) * ((1 + rel) * LD(1 + rr.U) ** 2 / (1 - relS) - 1)
    errW = np.abs(r["w"][:n].astype(LD) - wref)
    print(f"   weights: worst error / bound {float(np.max(errW[e > 0] / bW[e > 0])):.3f}")
    assert np.all(errW <= bW)
    return m, S


KS_CASES = [(n, k, where) for n in (257, 65536 + 1, 1024 * 256, 1024 * 256 + 1, 3 * 1024 * 256 + 77) for k in (3.0, -0.75)
            for where in ("first", "last", "second trip") if where != "second trip" or n > SECOND_TRIP]


@pytest.mark.parametrize("n,k,where", KS_CASES)
def test_ks_soft_maximum_and_minimum(n, k, where):
    """k > 0 and k < 0 (a soft minimum); the extreme at index 0, at n - 1 (the tail element) and at the first element of the second trip"""
    at = {"first": 0, "last": n - 1, "second trip": SECOND_TRIP}[where]
    a = rr.ks_palette(n, k, 21, at)
    E = exp_error(n, k, 21, at)
    r = run2(lambda: rr.dev_ks(lib(), a, k, -2.5))
    check_ks(a, k, r, E, -2.5)
    assert int(np.argmax(np.abs(r["w"][:n]))) == at, "the largest weight does not sit on the extreme entry"


def test_ks_two_exact_ties_at_the_maximum():
    n, k = 65536 + 1, 3.0
    a = rr.ks_palette(n, k, 22, 5)
    a[n - 1] = a[5]
    r = run2(lambda: rr.dev_ks(lib(), a, k))
    m, S = check_ks(a, k, r, exp_error(n, k, 22, 5), 1.0)
    assert np.sum(k * a == m) == 2 and r["w"][5] == r["w"][n - 1] == np.max(r["w"][:n]) and float(S) > 2.0


@pytest.mark.parametrize("k", [2.0, -2.0])
@pytest.mark.parametrize("n", [65536 + 1, 3 * 1024 * 256 + 77])
def test_ks_spread_that_underflows(n, k):
    """k (a - max) < -800 for all but five entries: their exponentials and weights are EXACT zeros, S is the sum of the five"""
    a, k, alive = rr.wide_spread(n, k)
    m = float(np.max(k * a))
    E = rr.measure_exp_ulps(lib(), rr.ks_arguments(a[alive], k, m))
    r = run2(lambda: rr.dev_ks(lib(), a, k))
    check_ks(a, k, r, E, 1.0)
    dead = np.ones(n, dtype=bool)
    dead[alive] = False
    assert rr.same(r["w"][:n][dead], np.zeros(n - len(alive))), "a weight that must underflow is not an exact +0"
    nb = rr.blocks(n)
    empty = rr.by_block(~dead, nb, False).sum(axis=(0, 2)) == 0
    assert empty.sum() >= nb - 5 and rr.same(r["psum"][:nb][empty], np.zeros(empty.sum()))
    assert 1.0 <= r["S"] < 1.01


def test_ks_near_the_production_guard():
    """m + log S just under log(1e200) = 460.5, where location_ks_value stops: m = 449.4, log S <= log(65537) = 11.09"""
    n, k = 65536 + 1, 1.0
    a = rr.ks_palette(n, k, 23, 100, spread=19.4, base=430.0)
    r = run2(lambda: rr.dev_ks(lib(), a, k))
    check_ks(a, k, r, exp_error(n, k, 23, 100, 430.0, 19.4), 1.0)
    lg = r["m"] + math.log(r["S"])
    assert math.log(1e200) - 12.0 < lg <= math.log(1e200), lg


# ---- the sums on integer-valued inputs: exact, partial by partial -----------------------------------------------------------------------------
def exact_pair(r, terms, nb, scale=1.0):
    """the partials and the total of integer-valued terms"""
    assert r["nb"] == nb and written(r["part"], nb)
    assert np.array_equal(r["part"][:nb], rr.block_sums_exact(terms, nb).astype(np.float64)), "a partial sum is not the exact count"
    return scale * float(np.sum(np.asarray(terms).astype(np.int64)))


@pytest.mark.parametrize("n", rr.SIZES)
def test_dot_products_of_integers_are_exact(n):
    """k_tangent_dot + k_group_sum, k_ad_dot_partial + k_hs_final, k_sv_dot + k_group_sum; the dual numbers carry values of magnitude 1e30
    next to the tangents: a kernel that read .v for .d[0] would be off by 25 orders of magnitude"""
    d, psi = rr.small_ints(n, 1, 1, 1000), rr.small_ints(n, 2, -3, 3)
    R = rr.duals(d, 3)
    r = run2(lambda: rr.dev_tangent_dot(lib(), R, psi))
    used = rr.ceil_div(n, 256)
    assert r["nb"] == rr.TD_BLOCKS and written(r["part"], rr.TD_BLOCKS) and rr.guard_intact(r["out"], 2)
    assert rr.same(r["part"][min(used, 1024):1024], np.zeros(1024 - min(used, 1024))), "a workgroup without rows did not write an exact +0"
    assert r["out"][0] == exact_pair(r, d * psi, rr.TD_BLOCKS) and r["out"][1] == 0.0
    r = run2(lambda: rr.dev_ad_dot(lib(), R, psi))
    assert r["out"][0] == exact_pair(r, d * psi, min(rr.CAP, used)) and rr.guard_intact(r["out"], 1)
    r = run2(lambda: rr.dev_sv_dot(lib(), d, psi))
    assert r["out"][0] == exact_pair(r, d * psi, min(rr.SV_CAP, used)) and r["out"][1] == 0.0 and rr.guard_intact(r["out"], 2)


def test_tangent_dot_of_nothing_is_zero():
    r = run2(lambda: rr.dev_tangent_dot(lib(), np.zeros((0, 2)), np.zeros(0)))
    assert rr.same(r["part"][:1024], np.zeros(1024)) and rr.same(r["out"][:2], np.zeros(2)) and written(r["part"], 1024)


@pytest.mark.parametrize("n", rr.SIZES)
def test_group_sum_of_integers_is_exact(n):
    """a null group, all in group 0, all in group 1, alternating, and group 1 in the tail entry alone"""
    fv = rr.counting(n)
    total = n * (n + 1) // 2
    tail = np.zeros(n, dtype=np.uint8)
    tail[n - 1] = 1
    alt = (np.arange(n) % 2).astype(np.uint8)
    for name, g in (("null", None), ("zeros", np.zeros(n, dtype=np.uint8)), ("ones", np.ones(n, dtype=np.uint8)), ("alternating", alt), ("tail", tail)):
        r = run2(lambda: rr.dev_group_sum(lib(), fv, g))
        s1 = 0 if g is None else int(np.sum(fv[g == 1]))
        assert (r["out"][0], r["out"][1]) == (total - s1, s1) and rr.guard_intact(r["out"], 2), name


@pytest.mark.parametrize("l1", [0, 1])
@pytest.mark.parametrize("n", rr.SIZES)
def test_residual_norm_of_integers_is_exact(n, l1):
    """terms and seeds bit by bit against the restatement, the sum exact; L1: the seed of a row with R = 0 is an exact 0"""
    lay = rr.rn_tiled(n)
    R = rr.small_ints(n, 4)
    terms = rr.rn_terms_np(lay, l1, R)
    F = float(np.sum(terms)) if l1 else math.sqrt(float(np.sum(terms)))
    F = F if F != 0.0 else 1.0
    r = run2(lambda: rr.dev_rn(lib(), lay, l1, R, F, 0.5))
    nb = rr.blocks(n)
    assert rr.guard_intact(r["term"], n) and rr.guard_intact(r["g"], n) and r["ms"][0] == rr.SENT and rr.guard_intact(r["ms"], 2)
    assert rr.same(r["term"][:n], terms) and r["sum"] == exact_pair(r, terms, nb)
    assert rr.same(r["g"][:n], rr.rn_seeds_np(lay, l1, R, F, 0.5))
    if l1:
        w, ip = rr.rn_rows(lay)
        assert rr.same(r["g"][:n][(R == 0.0) & ~ip], np.zeros(np.sum((R == 0.0) & ~ip)))


@pytest.mark.parametrize("l1", [0, 1])
def test_residual_norm_on_every_block_kind(l1):
    """vector, scalar and flux block with nIF < nF, distinct weights with a zero one, rows that fall in no block; random R with zeros"""
    lay = rr.rn_layout()
    R = np.random.default_rng(6).standard_normal(lay["n"])
    R[::7] = 0.0
    terms = [rr.rn_term(lay, l1, i, R[i]) for i in range(lay["n"])]
    F = math.fsum(terms) if l1 else math.sqrt(math.fsum(terms))
    r = run2(lambda: rr.dev_rn(lib(), lay, l1, R, F, -1.5))
    n, nb = lay["n"], rr.blocks(lay["n"])
    assert rr.same(r["term"][:n], terms) and rr.same(r["g"][:n], [-1.5 * rr.rn_seed(lay, l1, i, R[i], F) for i in range(n)])
    err, bnd = abs(rr.error_of(terms, r["sum"])), rr.bound(rr.depth(n, nb), terms)
    print(f"residualNorm l1 {l1}: error {err:.3e} bound {bnd:.3e}")
    assert err <= bnd and written(r["part"], nb)


@pytest.mark.parametrize("n", rr.SIZES)
def test_cell_function_of_integers_is_exact(n):
    """x, and V x^2 with reference data; the gradient bit by bit, with the state scales and without, zeros where no term points"""
    rng = np.random.default_rng(7)
    nCells, nSrc = 97, n + 5
    cell, idx = ((np.arange(n) * 7) % nCells).astype(np.int32), rng.permutation(nSrc)[:n].astype(np.int64)
    V, src, data, sc = rr.small_ints(nCells, 1, 1, 4), rr.small_ints(nSrc, 2), rr.small_ints(n, 3), rr.small_ints(nSrc, 5, 1, 8)
    nb = rr.blocks(n)
    for dat, square, mv, scale in ((None, 0, 0, None), (data, 1, 1, sc), (data, 0, 1, None), (None, 1, 0, sc)):
        r = run2(lambda: rr.dev_cellfn(lib(), cell, idx, dat, square, mv, V, src, 0.5, scale, 0.25))
        x = src[idx] - (0.0 if dat is None else dat)
        wt = V[cell] if mv else np.ones(n)
        assert r["out"][0] == exact_pair(r, wt * (x * x if square else x), nb, 0.5) and rr.guard_intact(r["out"], 1)
        grad = np.zeros(nSrc)
        grad[idx] = 0.25 * wt * (2.0 * x if square else np.ones(n)) * (1.0 if scale is None else scale[idx])
        assert rr.same(r["grad"][:nSrc], grad) and rr.guard_intact(r["grad"], nSrc)


@pytest.mark.parametrize("n", rr.SIZES)
def test_heat_source_sums_of_integers_are_exact(n):
    """k_hs_partial<double> + k_hs_final<double>, field and cell-set kind: psi null and given, byV 0 and 1, vt null and given"""
    V, field, psi = rr.small_ints(n, 1, 1, 4), rr.small_ints(n, 2), rr.small_ints(n, 3, -3, 3)
    member = (np.arange(n) % 3 != 1).astype(np.uint8)
    nb = min(rr.CAP, rr.ceil_div(n, 256))
    for kind, s in ((rr.HS_FIELD, field), (rr.HS_SET, member)):
        sv = s.astype(np.float64)
        r = run2(lambda: rr.dev_hs_sum(lib(), kind, V, s, None, 0, 6.0, None))
        assert r["out"][0] == exact_pair(r, sv * V, nb) and rr.guard_intact(r["out"], 1)
        for byV in (0, 1):
            for vt in (None, 2.0):
                r = run2(lambda: rr.dev_hs_sum(lib(), kind, V, s, psi, byV, 6.0, vt))
                terms = (sv if vt is None else 6.0 * sv / vt) * (psi * (V if byV else 1.0))
                assert r["out"][0] == exact_pair(r, terms, nb), (kind, byV, vt)


@pytest.mark.parametrize("nb", [1, 255, 256, 257, 1024])
def test_second_stages_on_given_partials(nb):
    """k_hs_final<double / Dual<1>> and k_ad_final<double / Dual<1>> (two block sums with a barrier between them): integer tangents next to
    values of magnitude 1e30 - the tangent sums are exact, the value sums within the bound of one stage"""
    a, b = rr.small_ints(nb, 1, 1, 1000), rr.small_ints(nb, 2, -50, 50)
    va, vb = rr.duals(a, 3)[:, 0], rr.duals(b, 4)[:, 0]
    d = rr.ceil_div(nb, 256) + 8
    r = run2(lambda: rr.dev_final(lib(), 0, 0, nb, a))
    assert r["out"][0] == a.sum() and rr.guard_intact(r["out"], 1)
    r = run2(lambda: rr.dev_final(lib(), 1, 0, nb, np.stack([a, b], axis=1)))
    assert (r["out"][0], r["out"][1]) == (a.sum(), b.sum()) and rr.guard_intact(r["out"], 2)
    r = run2(lambda: rr.dev_final(lib(), 0, 1, nb, np.stack([va, a], axis=1)))
    assert r["out"][1] == a.sum() and rr.guard_intact(r["out"], 2)
    assert abs(rr.error_of(va, r["out"][0])) <= rr.bound(d, va)
    r = run2(lambda: rr.dev_final(lib(), 1, 1, nb, np.stack([np.stack([va, a], axis=1), np.stack([vb, b], axis=1)], axis=1)))
    assert (r["out"][1], r["out"][3]) == (a.sum(), b.sum()) and rr.guard_intact(r["out"], 4)
    for got, v in ((r["out"][0], va), (r["out"][2], vb)):
        err, bnd = abs(rr.error_of(v, got)), rr.bound(d, v)
        print(f"nb {nb}: value sum error {err:.3e} bound {bnd:.3e}")
        assert err <= bnd


# ---- the sums on rounding inputs: within d u sum |terms| --------------------------------------------------------------------------------------
@pytest.mark.parametrize("maker", [rr.mixed, rr.ill_conditioned])
@pytest.mark.parametrize("n", ROUNDING_SIZES)
def test_sums_round_within_the_derived_bound(n, maker):
    """every pair on values of mixed sign and on large cancelling pairs plus small terms (sum |x| / |sum x| >= 1e8); the inputs carry 24
    significant bits, so the products are exact and the bound is the summation's alone"""
    x = maker(n, 31)
    y = np.ones(n) if maker is rr.ill_conditioned else rr.bits24(np.random.default_rng(32).uniform(0.5, 2.0, size=n))  # ones: the pairs still cancel
    used = rr.ceil_div(n, 256)
    terms = x * y
    assert maker is rr.mixed or rr.condition(terms) >= 1e8
    checks = []
    R = rr.duals(x, 3)
    checks.append(("tangent_dot", run2(lambda: rr.dev_tangent_dot(lib(), R, y))["out"][0], rr.depth(n, rr.TD_BLOCKS)))
    checks.append(("ad_dot", run2(lambda: rr.dev_ad_dot(lib(), R, y))["out"][0], rr.depth(n, min(rr.CAP, used))))
    checks.append(("sv_dot", run2(lambda: rr.dev_sv_dot(lib(), x, y))["out"][0], rr.depth(n, min(rr.SV_CAP, used))))
    checks.append(("hs_sum", run2(lambda: rr.dev_hs_sum(lib(), rr.HS_FIELD, y, x, None, 0, 1.0, None))["out"][0], rr.depth(n, min(rr.CAP, used))))
    cell, idx = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int64)[::-1].copy()
    checks.append(("cellfn", run2(lambda: rr.dev_cellfn(lib(), cell, idx, None, 0, 1, y, x[::-1].copy(), 1.0, None, 1.0))["out"][0], rr.depth(n, rr.blocks(n))))
    for name, got, d in checks:
        err, bnd = abs(rr.error_of(terms, got)), rr.bound(d, terms)
        print(f"{name} n {n} {maker.__name__}: error {err:.3e} bound {bnd:.3e} (d {d})")
        assert err <= bnd, name
    alt = (np.arange(n) % 2).astype(np.uint8)
    out = run2(lambda: rr.dev_group_sum(lib(), x, alt))["out"]
    for g in (0, 1):
        err, bnd = abs(rr.error_of(x[alt == g], out[g])), rr.bound(rr.depth_group(n), x[alt == g])
        print(f"group_sum n {n} {maker.__name__} group {g}: error {err:.3e} bound {bnd:.3e}")
        assert err <= bnd


# ---- the gathers without atomics --------------------------------------------------------------------------------------------------------------
def test_owner_gather_adds_each_owned_face_once_in_list_order():
    nC, nIF, nF, ptr, enc, other = rr.cell_faces()
    for ft in (rr.small_ints(nF, 2), np.random.default_rng(8).standard_normal(nF)):
        r = run2(lambda: rr.dev_owner_gather(lib(), ptr, enc, ft))
        assert rr.same(r["tc"][:nC], rr.owner_gather(ptr, enc, ft)) and rr.guard_intact(r["tc"], nC)


def test_vm_gather_adds_the_neighbours_across_internal_faces():
    nC, nIF, nF, ptr, enc, other = rr.cell_faces()
    rng = np.random.default_rng(9)
    colors, tc, out = rng.integers(0, 5, size=3 * nC).astype(np.int32), rng.standard_normal(nC), rr.out_array(3 * nC)
    r = run2(lambda: rr.dev_vm_gather(lib(), nIF, ptr, enc, other, colors, 2, tc, -0.75, out))
    assert rr.same(r["out"], rr.vm_gather(nIF, ptr, enc, other, colors, 2, tc, -0.75, out))
    assert np.all(r["out"][:3 * nC][colors != 2] == rr.SENT) and np.all(r["out"][:3 * nC][colors == 2] != rr.SENT)

"""tests/reduce_reference.py without a GPU: the restatements against independent formulations (KS against the unshifted log-sum-exp, the
residualNorm terms against numpy.linalg.norm on weighted rows, the vectorised twins against the plain-Python loops bit by bit), the
input makers against what they promise, a float64 emulation of the kernels' own summation order against the derived bound (it passes;
a dropped, doubled or misplaced element does not), and the entries das_debug_reduce_* refusing every invalid input with DAS_ERR_ARG
before anything is launched (these run without a device)."""
import math

import numpy as np
import pytest

import reduce_reference as rr
from dafoam_amd import _capi

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")
ARG = -1  # DAS_ERR_ARG


def wave_tree(acc):
    """acc[..., 256] -> the workgroup's sum in the order of the shuffle kernels: per wave of 64 the steps 32 .. 1, then (s0 + s1) + (s2 + s3)"""
    w = acc.reshape(acc.shape[:-1] + (4, 64)).copy()
    for o in (32, 16, 8, 4, 2, 1):
        w[..., :o] = w[..., :o] + w[..., o:2 * o]
    s = w[..., 0]
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


def lds_tree(acc):
    w = acc.copy()
    for o in (128, 64, 32, 16, 8, 4, 2, 1):
        w[..., :o] = w[..., :o] + w[..., o:2 * o]
    return w[..., 0]


def emulate(x, nb, tree):
    """the two stages in float64 in the kernels' own order: (partials, total)"""
    v = rr.by_block(np.asarray(x, dtype=np.float64), nb, 0.0)
    acc = np.zeros(v.shape[1:])
    for t in range(v.shape[0]):
        acc = acc + v[t]
    part = tree(acc)
    p = rr.by_block(part, 1, 0.0)
    acc = np.zeros(256)
    for t in range(p.shape[0]):
        acc = acc + p[t, 0]
    return part, float(tree(acc))


@pytest.mark.parametrize("n", rr.SIZES)
def test_integer_inputs_stay_exact_in_every_partial_sum(n):
    """x_i = i + 1 and the small-integer products: the sum of the magnitudes stays below 2^53, so no order of additions rounds"""
    assert math.fsum(rr.counting(n)) == n * (n + 1) // 2 < 2 ** 53
    a, b = rr.small_ints(n, 1, 1, 1000), rr.small_ints(n, 2, -3, 3)
    assert np.sum(np.abs(a * b).astype(np.int64)) < 2 ** 53
    for cap, tree in ((rr.CAP, wave_tree), (rr.SV_CAP, lds_tree)):
        nb = rr.blocks(n, cap)
        part, total = emulate(rr.counting(n), nb, tree)
        assert total == n * (n + 1) // 2
        assert np.array_equal(part, rr.block_sums_exact(rr.counting(n), nb).astype(np.float64))


def test_block_arithmetic_reaches_every_trip_count():
    assert [rr.blocks(n) for n in rr.SIZES] == [1, 1, 1, 1, 1, 1, 2, 257, 513, 1024, 1024, 1024]
    assert [rr.blocks(n, rr.SV_CAP) for n in rr.SIZES[-4:]] == [512, 512, 512, 512]
    assert [rr.ceil_div(n, 256 * rr.blocks(n)) for n in rr.SIZES[-3:]] == [1, 2, 4]
    assert rr.ceil_div(rr.blocks(65537), 256) == 2 and rr.depth(786509, 1024) == 4 + 4 + 16 and rr.depth_group(257) == 10


@pytest.mark.parametrize("n", [257, 65537, 786509])
@pytest.mark.parametrize("maker", [rr.mixed, rr.ill_conditioned])
def test_kernel_order_in_float64_meets_the_derived_bound_and_a_wrong_sum_does_not(n, maker):
    x = maker(n, 11)
    for cap, tree in ((rr.CAP, wave_tree), (rr.SV_CAP, lds_tree)):
        nb = rr.blocks(n, cap)
        _, total = emulate(x, nb, tree)
        err, bnd = abs(rr.error_of(x, total)), rr.bound(rr.depth(n, nb), x)
        print(f"n {n} {maker.__name__}: error {err:.3e} bound {bnd:.3e}")
        assert err <= bnd
        k = int(np.argmin(np.abs(x)))  # the smallest entry dropped: still outside the bound on the mixed input
        if maker is rr.mixed:
            assert abs(rr.error_of(x, total - x[n - 1])) > bnd, "a dropped tail element hides inside the bound"
        assert x[k] != 0.0


@pytest.mark.parametrize("n", [3, 257, 65537, 786509])
def test_ill_conditioned_input_is_ill_conditioned(n):
    x = rr.ill_conditioned(n, 5)
    assert rr.condition(x) >= 1e8, rr.condition(x)
    assert np.array_equal(x, rr.bits24(x)) and np.array_equal(rr.mixed(n, 5), rr.bits24(rr.mixed(n, 5)))
    a, b = rr.mixed(n, 1), rr.mixed(n, 2)
    L = np.longdouble
    assert np.all((a.astype(L) * b.astype(L)).astype(np.float64).astype(L) == a.astype(L) * b.astype(L)), "a product of 24-bit values is not exact"


@pytest.mark.parametrize("k", [7.0, -3.0, 0.25])
def test_ks_restatement_is_the_unshifted_log_sum_exp(k):
    a = rr.ks_palette(5000, k, 3, 17)
    m, e, S = rr.ks_reference(a, k)
    assert m == float(np.max(k * a)) and int(np.argmax(k * a)) == 17 and np.sum(k * a == m) == 1
    F = (np.longdouble(m) + np.log(S)) / np.longdouble(k)
    assert abs(F - rr.ks_unshifted(a, k)) <= 1e-17 * abs(F)
    assert (F >= a.max()) if k > 0 else (F <= a.min())
    assert abs(float(e.max()) - 1.0) < 1e-14 and 1.0 <= S <= len(a)
    assert len(rr.ks_arguments(a, k, m)) <= 2 * 1000 and rr.ks_arguments(a, k, m).min() > -700.0


def test_wide_ks_input_really_underflows():
    a, k, alive = rr.wide_spread(65537)
    m, e, S = rr.ks_reference(a, k)
    x = k * a - m
    assert np.all((x[alive] >= -50.0)) and np.all(np.delete(x, alive) < -800.0)
    assert np.all(np.exp(np.delete(x, alive)) == 0.0), "fp64 exp does not underflow to an exact zero there"
    assert np.count_nonzero(e) == len(alive) and float(S) == pytest.approx(float(np.exp(x[alive].astype(np.longdouble)).sum()), rel=1e-15)


def test_exp_probe_isolates_one_argument_per_workgroup():
    args = -np.linspace(0.0, 700.0, 1023)
    a = rr.exp_probe(args)
    assert len(a) == 1024 * 256 and rr.blocks(len(a)) == 1024 and a.max() == 0.0
    v = rr.by_block(np.exp(a), 1024, 0.0)
    assert v.shape[0] == 1 and np.array_equal(v[0].sum(axis=1)[:1023], np.exp(args)) and np.all(np.count_nonzero(v[0], axis=1) == 1)


@pytest.mark.parametrize("l1", [0, 1])
def test_residual_norm_restatement(l1):
    lay = rr.rn_layout()
    rng = np.random.default_rng(4)
    R = rng.standard_normal(lay["n"])
    R[::7] = 0.0
    terms = [rr.rn_term(lay, l1, i, R[i]) for i in range(lay["n"])]
    assert rr.same(terms, rr.rn_terms_np(lay, l1, R))
    w, ip = rr.rn_rows(lay)
    assert sorted(set(w)) == [-0.25, 0.0, 1.5, 3.0] and ip.sum() == lay["nIF"] and np.sum(w == 0.0) == lay["nC"] + 8
    if l1:
        F = math.fsum(terms)
        assert F == pytest.approx(np.sum(np.abs(w * R)[~ip]) + np.sum((w * R)[ip] ** 2), rel=1e-13)
    else:
        F = math.sqrt(math.fsum(terms))
        assert F == pytest.approx(np.linalg.norm(w * R), rel=1e-13)
    seeds = [0.5 * rr.rn_seed(lay, l1, i, R[i], F) for i in range(lay["n"])]
    assert rr.same(seeds, rr.rn_seeds_np(lay, l1, R, F, 0.5))
    # the seeds are the derivative of F: central differences on a row of every kind (internal and boundary flux, a zero weight, no block)
    for i in (1, 3 * lay["nC"] + 2, 4 * lay["nC"] + 6, 5 * lay["nC"] + 5 + 3, 5 * lay["nC"] + 5 + lay["nIF"] + 1, lay["n"] - 1):
        if R[i] == 0.0:
            i -= 1
        h = 1e-6

        def value(Ri):
            t = [rr.rn_term(lay, l1, j, Ri if j == i else R[j]) for j in range(lay["n"])]
            return math.fsum(t) if l1 else math.sqrt(math.fsum(t))

        fd = (value(R[i] + h) - value(R[i] - h)) / (2 * h)
        assert rr.rn_seed(lay, l1, i, R[i], F) == pytest.approx(fd, rel=1e-6, abs=1e-9)
    if l1:
        assert all(rr.rn_seed(lay, 1, i, 0.0, F) == 0.0 for i in range(lay["n"]))


@pytest.mark.parametrize("n", [1, 65, 65537])
def test_tiled_residual_layout_covers_n_rows(n):
    lay = rr.rn_tiled(n)
    w, ip = rr.rn_rows(lay)
    assert len(w) == n and all((w[i], ip[i]) == rr.rn_weight(lay, i) for i in range(0, n, max(1, n // 500)))
    if n > 100:
        assert ip.any() and (w == 0.0).any() and set(w) == {2.0, -3.0, 0.0, 5.0} and w[-1] == 0.0


def test_gather_restatements():
    nC, nIF, nF, ptr, enc, other = rr.cell_faces()
    assert ptr[0] == 0 and ptr[1] == 0 and ptr[6] - ptr[5] == 9 and np.any(enc < 0) and np.any(enc >= 0)
    face = enc.view(np.uint32) & 0x7fffffff
    assert np.all(face < nF) and np.all(other[face < nIF] >= 0) and np.all(face[enc < 0] < nIF)
    ft = rr.small_ints(nF, 2)
    tc = rr.owner_gather(ptr, enc, ft)
    own = enc >= 0
    assert tc.sum() == ft[enc[own]].sum() and tc[0] == 0.0


def test_entries_refuse_invalid_input_before_a_launch():
    L = _capi.lib()
    ok = np.ones(4)
    assert rr.dev_ks(L, np.zeros(0), 1.0)[0] == ARG, "n = 0 has no KS aggregate"
    nb = rr.C.c_int(0)
    big = rr.out_array(rr.CAP)
    assert L.das_debug_reduce_ks(4, rr._d(ok), 1.0, 1.0, rr._d(big), 1, rr._d(big), rr._d(big), len(big), rr._d(big), len(big), rr.C.byref(nb)) == ARG
    assert L.das_debug_reduce_ks(4, rr._d(ok), 1.0, 1.0, rr._d(big), 2, rr._d(big), rr._d(big), 1023, rr._d(big), len(big), rr.C.byref(nb)) == ARG
    assert L.das_debug_reduce_ks(4, None, 1.0, 1.0, rr._d(big), 2, rr._d(big), rr._d(big), len(big), rr._d(big), len(big), rr.C.byref(nb)) == ARG
    assert L.das_debug_reduce_group_sum(4, None, rr._d(ok), rr._d(big), 1) == ARG and L.das_debug_reduce_group_sum(-1, None, rr._d(ok), rr._d(big), 2) == ARG
    assert rr.dev_sv_dot(L, np.zeros(0), np.zeros(0))[0] == ARG and rr.dev_ad_dot(L, np.zeros((0, 2)), np.zeros(0))[0] == ARG
    assert L.das_debug_reduce_sv_dot(4, rr._d(ok), rr._d(ok), rr._d(big), 511, rr._d(big), 2, rr.C.byref(nb)) == ARG
    assert L.das_debug_reduce_tangent_dot(2, rr._d(ok), rr._d(ok), rr._d(big), 1023, rr._d(big), 2, rr.C.byref(nb)) == ARG
    V, src = np.ones(3), np.ones(5)
    for cell, idx in (([0, 3], [0, 1]), ([0, -1], [0, 1]), ([0, 1], [0, 5]), ([0, 1], [2, 2])):
        assert rr.dev_cellfn(L, cell, idx, None, 0, 1, V, src, 1.0, None, 1.0)[0] == ARG, (cell, idx)
    lay = rr.rn_layout()
    assert rr.dev_rn(L, lay, 0, np.ones(4), 0.0, 1.0)[0] == ARG, "the L2Norm seeds at F = 0"
    assert rr.dev_rn(L, dict(lay, nIF=lay["nF"] + 1), 1, np.ones(4), 1.0, 1.0)[0] == ARG
    assert rr.dev_rn(L, dict(lay, blocks=[(0, 3, 1.0)]), 1, np.ones(4), 1.0, 1.0)[0] == ARG
    assert rr.dev_hs_sum(L, 1, V, np.ones(3), None, 0, 1.0, None)[0] == ARG, "cylinderSmooth reads cell centres"
    assert rr.dev_hs_sum(L, rr.HS_FIELD, V, np.ones(3), None, 0, 1.0, 2.0)[0] == ARG, "vt without psi"
    assert rr.dev_final(L, 0, 0, 1025, np.ones(1025))[0] == ARG and rr.dev_final(L, 1, 1, 4, np.ones(15))[0] == ARG
    ptr, enc = np.array([0, 2, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    assert rr.dev_owner_gather(L, ptr, enc, np.ones(2))[0] == ARG, "decreasing cf_ptr"
    ptr = np.array([0, 1, 2], dtype=np.int32)
    assert rr.dev_owner_gather(L, ptr, np.array([0, 2], dtype=np.int32), np.ones(2))[0] == ARG, "face out of range"
    other, colors = np.array([1, 2], dtype=np.int32), np.zeros(6, dtype=np.int32)
    assert rr.dev_vm_gather(L, 2, ptr, enc, other, colors, 0, np.ones(2), 1.0, rr.out_array(6))[0] == ARG, "neighbour out of range"
    assert rr.dev_vm_gather(L, 2, ptr, enc, np.array([1, 0], dtype=np.int32), colors, 0, np.ones(2), 1.0, rr.out_array(6)[:5])[0] == ARG, "out shorter than 3 nC"

"""CPU tier of the Krylov kernel tests: (1) the longdouble restatements of tests/krylov_reference.py against mpmath at 200 bits,
to the longdouble rounding level; (2) the comparison functions the GPU test uses must ACCEPT a plain fp64 numpy implementation at
every parametrised shape (well- and ill-scaled inputs) and must REJECT deliberately wrong results - last element dropped, last
chunk of 4096 dropped, basis vector K - 1 replaced by K - 2, lo array ignored in an update, one SpMV row shifted by one entry, hi
truncated instead of rounded - at every shape where the mistake is expressible, without allowance (well-scaled inputs: every entry
is >= 0.5 in magnitude, the smallest possible mistake, 0.25, is above the largest bound)."""
import mpmath
import numpy as np
import pytest

import krylov_reference as kr
from krylov_reference import FP32, FP64, LD, SPLIT

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")

NK = kr.nk_shapes()
NK_IDS = [f"n{n}-K{K}" for n, K in NK]
E64 = 2.0 ** -64


def mp(x):
    """exact conversion of a longdouble (64-bit mantissa) to mpmath"""
    m, e = np.frexp(LD(x))
    hi = np.floor(m * LD(2.0 ** 32))
    lo = (m * LD(2.0 ** 32) - hi) * LD(2.0 ** 32)
    return (mpmath.mpf(int(hi)) * 2 ** 32 + mpmath.mpf(int(lo))) * mpmath.mpf(2) ** (int(e) - 64)


def close(ld, exact, mag, T):
    return abs(mp(ld) - exact) <= (T + 2) * E64 * mag


@pytest.mark.parametrize("fmt", [FP64, FP32, SPLIT], ids=kr.FMT_NAMES.get)
@pytest.mark.parametrize("n,K", [(1, 1), (2, 2), (17, 5), (65, 3), (257, 4)])
def test_restatements_match_mpmath(n, K, fmt):
    with mpmath.workprec(200):
        B = kr.Basis(kr.vectors(n, K, 1), fmt, (2 * n if fmt == SPLIT else n) + 1, extra_slots=1)
        v = kr.vector(n, 2)
        st = B.slots().astype(np.float64)
        hi = [[mpmath.mpf(float(x)) for x in st[i, :n]] for i in range(K)]
        full = [[mpmath.mpf(float(st[i, k])) + (mpmath.mpf(float(st[i, n + k])) if fmt == SPLIT else 0) for k in range(n)] for i in range(K)]
        mv = [mpmath.mpf(float(x)) for x in v]
        # inner products (hi arrays) and their magnitudes
        ref, mag = kr.ref_dots2(B, v)
        for i in range(K):
            for r, y in ((0, hi[K - 1]), (1, mv)):
                ex = mpmath.fsum(a * b for a, b in zip(hi[i], y))
                mg = mpmath.fsum(abs(a * b) for a, b in zip(hi[i], y))
                assert close(ref[r * K + i], ex, mg, n) and close(mag[r * K + i], mg, mg, n)
        # w - sum h_i V_i and sum c_i V_i (hi + lo)
        h = kr.vector(K, 3)
        refa, maga = kr.ref_multiaxpy(B, K, h, v)
        refc, magc = kr.ref_combination(B, K, h)
        for k in range(n):
            terms = [mpmath.mpf(float(h[i])) * full[i][k] for i in range(K)]
            mg = mpmath.fsum(abs(t) for t in terms)
            assert close(refc[k], mpmath.fsum(terms), mg, K) and close(magc[k], mg, mg, K)
            assert close(refa[k], mv[k] - mpmath.fsum(terms), mg + abs(mv[k]), K + 1) and close(maga[k], mg + abs(mv[k]), mg + abs(mv[k]), K + 1)
        # the fused update with j = K - 1
        j = K - 1
        sc = 0.25 * kr.vector(max(2 * j, 1), 4)
        gam, ral = 0.8125, 1.0 / 0.73
        (q, mq), (un, mu) = kr.ref_dcgs2_update(B, j, sc, gam, ral, v)
        for k in range(n):
            ts = [mpmath.mpf(float(sc[i])) * full[i][k] for i in range(j)]
            tc = [mpmath.mpf(float(sc[j + i])) * full[i][k] for i in range(j)]
            u = full[j][k]
            mgq = abs(u) + mpmath.fsum(abs(t) for t in ts)
            mgu = abs(mv[k]) + abs(mpmath.mpf(gam) * u) + mpmath.fsum(abs(t) for t in tc)
            assert close(q[k], (u - mpmath.fsum(ts)) * mpmath.mpf(ral), mgq * abs(ral), j + 2) and close(mq[k], mgq, mgq, j + 2)
            assert close(un[k], (mv[k] - mpmath.mpf(gam) * u - mpmath.fsum(tc)) * mpmath.mpf(ral), mgu * abs(ral), j + 3) and close(mu[k], mgu, mgu, j + 3)


def test_block_and_csr_restatements_match_mpmath():
    with mpmath.workprec(200):
        n, K, s = 37, 5, 3
        V, W = kr.vectors(n, K, 5), kr.vectors(n, s, 6)
        Cm = kr.vector(K * s, 7).reshape(K, s)
        tn, mtn = kr.ref_block_tn(V, W)
        Y, mY = kr.ref_block_nn_sub(V, Cm, W)
        f = lambda x: mpmath.mpf(float(x))  # noqa: E731
        for i in range(K):
            for r in range(s):
                mg = mpmath.fsum(abs(f(a) * f(b)) for a, b in zip(V[i], W[r]))
                assert close(tn[i, r], mpmath.fsum(f(a) * f(b) for a, b in zip(V[i], W[r])), mg, n) and close(mtn[i, r], mg, mg, n)
        for r in range(s):
            for k in range(n):
                ts = [f(V[i, k]) * f(Cm[i, r]) for i in range(K)]
                mg = abs(f(W[r, k])) + mpmath.fsum(abs(t) for t in ts)
                assert close(Y[r, k], f(W[r, k]) - mpmath.fsum(ts), mg, K + 1) and close(mY[r, k], mg, mg, K + 1)
        rp, ci, val = kr.make_csr(50, 8, "longest")
        X = kr.vectors(50, 2, 9)
        Yc, mc, rl = kr.ref_csr_rows(rp, ci, val, X)
        assert rl[0] == 0 and rl[-1] == 280 and set(rl) >= {0, 1, 15, 16, 17, 63, 64, 65, 280}
        for i in range(50):
            for r in range(2):
                ts = [f(val[k]) * f(X[r, ci[k]]) for k in range(rp[i], rp[i + 1])]
                mg = mpmath.fsum(abs(t) for t in ts)
                assert close(Yc[r, i], mpmath.fsum(ts), mg, len(ts)) and close(mc[r, i], mg, mg, len(ts))
                assert len(ts) > 0 or (Yc[r, i] == 0 and mc[r, i] == 0)


# ---- the comparison functions: plain fp64 numpy accepted, mutations rejected -----------------------------------------------------
@pytest.mark.parametrize("ill", [False, True], ids=["well", "ill"])
@pytest.mark.parametrize("n,K", NK, ids=NK_IDS)
def test_plain_fp64_numpy_is_accepted(n, K, ill):
    V = kr.vectors(n, K, 11, ill)
    w = kr.vector(n, [12, K], ill)
    c = kr.vector(K, [13, K])
    for fmt in (FP64, FP32, SPLIT):
        B = kr.Basis(V, fmt, 2 * n if fmt == SPLIT else n)
        st = B.slots().astype(np.float64)
        hi = st[:, :n]
        full = hi + st[:, n:] if fmt == SPLIT else hi
        ref, mag = kr.ref_dots2(B, w)
        assert kr.check_sum(np.concatenate([hi @ hi[K - 1], hi @ w]), ref, mag, n)[0]
        ref, mag = kr.ref_multidot(B, K, w)
        assert kr.check_sum(np.append(hi @ w, w @ w), ref, mag, n)[0]
        ref, mag = kr.ref_combination(B, K, c)
        assert kr.check_sum(c @ full, ref, mag, K)[0]
        ref, mag = kr.ref_multiaxpy(B, K, c, w)
        got = w - c @ full
        assert kr.check_update(got, ref, mag, K + 1)[0]
        assert kr.check_split(*kr.split32(got), ref, mag, K + 1)[0]
        assert kr.check_fp32(got.astype(np.float32), ref)[0]


@pytest.mark.parametrize("n,K", NK, ids=NK_IDS)
def test_wrong_dots_and_combinations_are_rejected(n, K):
    V = kr.vectors(n, K, 11)
    w = kr.vector(n, [12, K])
    c = kr.vector(K, [13, K])
    for fmt in (FP64, FP32, SPLIT):
        B = kr.Basis(V, fmt, 2 * n if fmt == SPLIT else n)
        st = B.slots().astype(np.float64)
        hi = st[:, :n]
        full = hi + st[:, n:] if fmt == SPLIT else hi
        ref, mag = kr.ref_multidot(B, K, w)
        # last element dropped
        assert not kr.check_sum(np.append(hi[:, :-1] @ w[:-1], w[:-1] @ w[:-1]), ref, mag, n)[0]
        # last (partial or whole) chunk of 4096 dropped
        cut = 4096 * ((n - 1) // 4096)
        assert not kr.check_sum(np.append(hi[:, :cut] @ w[:cut], w[:cut] @ w[:cut]), ref, mag, n)[0]
        refc, magc = kr.ref_combination(B, K, c)
        refa, maga = kr.ref_multiaxpy(B, K, c, w)
        if K >= 2:
            # basis vector K - 1 replaced by K - 2
            sw = hi.copy()
            sw[K - 1] = sw[K - 2]
            assert not kr.check_sum(np.append(sw @ w, w @ w), ref, mag, n)[0]
            r2, m2 = kr.ref_dots2(B, w)
            assert not kr.check_sum(np.concatenate([sw @ hi[K - 1], sw @ w]), r2, m2, n)[0]
            fw = full.copy()
            fw[K - 1] = fw[K - 2]
            assert not kr.check_sum(c @ fw, refc, magc, K)[0]
            assert not kr.check_update(w - c @ fw, refa, maga, K + 1)[0]
        if fmt == SPLIT:
            # lo array ignored in an update
            assert not kr.check_update(w - c @ hi, refa, maga, K + 1)[0]
            assert not kr.check_sum(c @ hi, refc, magc, K)[0]
            (q, mq), (un, mu) = kr.ref_dcgs2_update(B, K - 1, 0.25 * np.tile(c, 2), 0.8125, 1.0 / 0.73, w)
            (qh, _), (uh, _) = kr.ref_dcgs2_update(B, K - 1, 0.25 * np.tile(c, 2), 0.8125, 1.0 / 0.73, w, lo=False)
            assert kr.check_split(*kr.split32(q.astype(np.float64)), q, mq, K, 1.0 / 0.73)[0] and not kr.check_split(*kr.split32(qh.astype(np.float64)), q, mq, K, 1.0 / 0.73)[0]
            assert kr.check_split(*kr.split32(un.astype(np.float64)), un, mu, K + 1, 1.0 / 0.73)[0] and not kr.check_split(*kr.split32(uh.astype(np.float64)), un, mu, K + 1, 1.0 / 0.73)[0]
        # hi truncated instead of rounded (the sum hi + lo is still right to 2^-48)
        good = (w - c @ full)
        hi_t = good.astype(np.float32)
        over = np.abs(hi_t.astype(np.float64)) > np.abs(good)
        hi_t[over] = np.nextafter(hi_t[over], np.float32(0.0))
        lo_t = (good - hi_t.astype(np.float64)).astype(np.float32)
        if np.any(over):  # expressible: at least one entry where rounding went away from zero
            assert not kr.check_split(hi_t, lo_t, refa, maga, K + 1)[0]


@pytest.mark.parametrize("last", ["empty", "longest"])
@pytest.mark.parametrize("s", kr.S_LIST)
def test_csr_product_accepted_and_shifted_row_rejected(s, last):
    import scipy.sparse as sp

    n = 333
    for ill in (False, True):
        rp, ci, val = kr.make_csr(n, 111, last, ill)
        X = kr.vectors(n, s, 112, ill)
        ref, mag, rl = kr.ref_csr_rows(rp, ci, val, X)
        A = sp.csr_matrix((val, ci, rp), shape=(n, n))
        assert kr.check_sum((A @ X.T).T, ref, mag, rl[None, :])[0]
    # one row shifted by one entry (well-scaled set): every non-empty row but the last of the matrix can shift
    rp, ci, val = kr.make_csr(n, 111, last)
    X = kr.vectors(n, s, 112)
    ref, mag, rl = kr.ref_csr_rows(rp, ci, val, X)
    good = np.array([[val[rp[i] : rp[i + 1]] @ X[r, ci[rp[i] : rp[i + 1]]] for i in range(n)] for r in range(s)])
    assert kr.check_sum(good, ref, mag, rl[None, :])[0]
    for i in range(n):
        if rl[i] > 0 and rp[i + 1] < rp[-1]:
            bad = good.copy()
            bad[:, i] = [val[rp[i] + 1 : rp[i + 1] + 1] @ X[r, ci[rp[i] + 1 : rp[i + 1] + 1]] for r in range(s)]
            assert not kr.check_sum(bad, ref, mag, rl[None, :])[0], i


@pytest.mark.parametrize("n,s", kr.ns_shapes(), ids=lambda v: str(v))
def test_block_products_accepted_and_wrong_column_rejected(n, s):
    K = 5
    for ill in (False, True):
        V, W = kr.vectors(n, K, 71, ill), kr.vectors(n, s, 72, ill)
        Cm = kr.vector(K * s, [83, K]).reshape(K, s)
        ref, mag = kr.ref_block_tn(V, W)
        assert kr.check_sum(V @ W.T, ref, mag, n)[0]
        refn, magn = kr.ref_block_nn_sub(V, Cm, W)
        assert kr.check_update(W - (V.T @ Cm).T, refn, magn, K + 1)[0]
    V, W = kr.vectors(n, K, 71), kr.vectors(n, s, 72)
    ref, mag = kr.ref_block_tn(V, W)
    refn, magn = kr.ref_block_nn_sub(V, Cm, W)
    if s >= 2:  # column r read for column r' (well-scaled set)
        Wx = W.copy()
        Wx[s - 1] = W[s - 2]
        assert not kr.check_sum(V @ Wx.T, ref, mag, n)[0]
        Cx = Cm.copy()
        Cx[:, s - 1] = Cm[:, s - 2]
        assert not kr.check_update(W - (V.T @ Cx).T, refn, magn, K + 1)[0]
    assert not kr.check_sum(V[:, :-1] @ W[:, :-1].T, ref, mag, n)[0]  # last row dropped

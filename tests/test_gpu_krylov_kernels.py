"""The Krylov kernels of the GMRES engine one by one on the device against their longdouble restatements (tests/krylov_reference.py):
no mesh, no solver.  The entries das_debug_krylov_* run the launch helpers the solver runs, on caller data.  Every operation is
compared with the derived bounds of krylov_reference (never tuned to what the kernels give), run twice for bitwise equality (the
kernels promise a fixed summation order) and checked for an untouched guard band around the range it may write.  The achieved
max err / (u magnitude) per operation and storage format is printed by the last test (profiles/README.md holds a recorded table)."""
import ctypes as C

import numpy as np
import pytest

import krylov_reference as kr
from dafoam_amd import _capi
from krylov_reference import FP32, FP64, LD, SPLIT

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")]

FMTS = [FP64, FP32, SPLIT]
FMT_ID = kr.FMT_NAMES.get
ILL_NK = [(17, 5), (1025, 9), (4097, 64), (16 * 1024 + 1, 9)]
FIGURES = {}


def record(op, fmt, ratio):
    key = (op, fmt if isinstance(fmt, str) else kr.FMT_NAMES[fmt])
    FIGURES[key] = max(FIGURES.get(key, 0.0), ratio)


def vp(a):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


def dp(a):
    return _capi.dptr(a)


def call(name, *args):
    _capi.check(getattr(_capi.lib(), name)(*args))


def twice(fn):
    """run fn (returns arrays) twice: the results must be bitwise equal; returns the first"""
    a, b = fn(), fn()
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two runs on the same input differ bitwise"
    return a if len(a) > 1 else a[0]


def lds(n, K, fmt):
    w = 2 * n if fmt == SPLIT else n
    return [w] if n * K > 2_000_000 else [w, w + 3]


def nk_cases():
    return [pytest.param(n, K, False, id=f"n{n}-K{K}") for n, K in kr.nk_shapes()] + [pytest.param(n, K, True, id=f"n{n}-K{K}-ill") for n, K in ILL_NK]


# ---- 1. fused two-vector inner products ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID)
@pytest.mark.parametrize("n,K,ill", nk_cases())
def test_multidot2(n, K, ill, fmt):
    V = kr.vectors(n, K, 11, ill)
    v = kr.vector(n, [12, K], ill)
    for ld in lds(n, K, fmt):
        B = kr.Basis(V, fmt, ld)

        def run():
            out = np.zeros(2 * K)
            call("das_debug_krylov_dots2", n, K, fmt, vp(B.a), ld, dp(v), dp(out))
            return out

        got = twice(run)
        ref, mag = kr.ref_dots2(B, v)
        ok, ratio = kr.check_sum(got, ref, mag, n)
        print(f"multidot2 {kr.FMT_NAMES[fmt]} n={n} K={K} ld={ld}: max err / (u sum|xy|) = {ratio:.3g} (bound {n})")
        record("k_multidot2 + k_reduce", fmt, ratio)
        assert ok


# ---- 2. fused update of the delayed re-orthogonalisation ------------------------------------------------------------------------
def check_stored(op, B, slot, ref, mag, T, scale):
    st = B.slots()
    if B.fmt == FP64:
        ok, ratio = kr.check_update(st[slot, : B.n], ref, mag, T, scale)
    elif B.fmt == FP32:
        ok, ratio = kr.check_fp32(st[slot, : B.n], ref)
        record(op + " (fp32 ulps)", B.fmt, ratio)
        return ok
    else:
        ok, ratio = kr.check_split(st[slot, : B.n], st[slot, B.n : 2 * B.n], ref, mag, T, scale)
    record(op, B.fmt, ratio)
    return ok


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID)
@pytest.mark.parametrize("n,j,ill", [pytest.param(n, j, False, id=f"n{n}-j{j}") for n, j in kr.nj_shapes()]
                         + [pytest.param(n, j, True, id=f"n{n}-j{j}-ill") for n, j in ((17, 5), (513, 9), (4097, 4))])
def test_dcgs2_update(n, j, ill, fmt):
    V = kr.vectors(n, j + 1, 21, ill)
    v = kr.vector(n, [22, j], ill)
    sc = 0.25 * kr.vector(max(2 * j, 1), [23, j])
    gamma, ralpha = 0.8125 + 1e-3 * j, 1.0 / 0.73
    for ld in lds(n, j + 3, fmt):
        B0 = kr.Basis(V, fmt, ld, extra_slots=2)
        (q, mq), (un, mu) = kr.ref_dcgs2_update(B0, j, sc, gamma, ralpha, v)

        def run():
            B = kr.Basis(V, fmt, ld, extra_slots=2)
            call("das_debug_krylov_dcgs2_update", n, j, fmt, vp(B.a), ld, B.nslots, dp(sc), gamma, ralpha, dp(v))
            return B.a

        B = kr.Basis(V, fmt, ld, extra_slots=2)
        B.a[:] = twice(run)
        w = B.width()
        assert np.array_equal(B.slots()[:j, :w], B0.slots()[:j, :w]), "the final basis vectors were modified"
        assert np.all(B.slots()[:, w:] == B.a.dtype.type(kr.SENTINEL)) and np.all(B.slots()[j + 2 :] == B.a.dtype.type(kr.SENTINEL)), "guard band overwritten"
        assert check_stored("k_dcgs2_update q_j", B, j, q, mq, j + 1, ralpha)
        assert check_stored("k_dcgs2_update u'", B, j + 1, un, mu, j + 2, ralpha)


# ---- 3. the cgs / mgs path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID)
@pytest.mark.parametrize("n,K,ill", nk_cases())
def test_multidot(n, K, ill, fmt):
    V = kr.vectors(n, K, 31, ill)
    w = kr.vector(n, [32, K], ill)
    for ld in lds(n, K, fmt):
        B = kr.Basis(V, fmt, ld)
        for m in sorted({K, 0}):

            def run():
                out = np.zeros(m + 1)
                call("das_debug_krylov_multidot", n, m, fmt, vp(B.a), ld, dp(w), dp(out))
                return out

            got = twice(run)
            ref, mag = kr.ref_multidot(B, m, w)
            ok, ratio = kr.check_sum(got, ref, mag, n)
            record("k_multidot + k_reduce", fmt, ratio)
            assert ok, (m, ratio)


@pytest.mark.parametrize("fmt", FMTS + ["fp32-float-w"], ids=lambda f: f if isinstance(f, str) else FMT_ID(f))
@pytest.mark.parametrize("n,K,ill", nk_cases())
def test_multiaxpy(n, K, ill, fmt):
    wfloat = fmt == "fp32-float-w"
    fmt = FP32 if wfloat else fmt
    V = kr.vectors(n, K, 41, ill)
    h = 0.25 * kr.vector(K, [42, K])
    pad = 5
    w0 = np.full(n + pad, kr.SENTINEL, dtype=np.float32 if wfloat else np.float64)
    w0[:n] = kr.vector(n, [43, K], ill)
    for ld in lds(n, K, fmt):
        B = kr.Basis(V, fmt, ld)

        def run():
            w = w0.copy()
            call("das_debug_krylov_multiaxpy", n, K, fmt, vp(B.a), ld, dp(h), int(wfloat), vp(w), w.size)
            return w

        got = twice(run)
        assert np.all(got[n:] == w0[n:]), "guard band overwritten"
        ref, mag = kr.ref_multiaxpy(B, K, h, w0[:n])
        if wfloat:
            ok, ratio = kr.check_fp32(got[:n], ref)
            record("k_multiaxpy float w (fp32 ulps)", fmt, ratio)
        else:
            ok, ratio = kr.check_update(got[:n], ref, mag, K + 1)
            record("k_multiaxpy", fmt, ratio)
        assert ok, ratio


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_ID)
@pytest.mark.parametrize("n,K,ill", nk_cases())
def test_lincomb(n, K, ill, fmt):
    V = kr.vectors(n, K, 51, ill)
    c = kr.vector(K, [52, K])
    for ld in lds(n, K, fmt):
        B = kr.Basis(V, fmt, ld)

        def run():
            y = np.full(n + 5, kr.SENTINEL)
            call("das_debug_krylov_lincomb", n, K, fmt, vp(B.a), ld, dp(c), dp(y), y.size)
            return y

        got = twice(run)
        assert np.all(got[n:] == kr.SENTINEL), "guard band overwritten"
        ref, mag = kr.ref_combination(B, K, c)
        ok, ratio = kr.check_sum(got[:n], ref, mag, K)
        record("k_lincomb", fmt, ratio)
        assert ok, ratio


SCALE_USES = {0: "double->double", 1: "double->float", 2: "double->split", 3: "split->double", 4: "float->double"}


@pytest.mark.parametrize("use", sorted(SCALE_USES), ids=SCALE_USES.get)
@pytest.mark.parametrize("ill", [False, True], ids=["well", "ill"])
@pytest.mark.parametrize("n", kr.N_LIST)
def test_scale_to(n, ill, use):
    a = 1.0 / 3.7
    xd = kr.vector(n, [61, use], ill)
    if use == 3:
        hi, lo = kr.split32(xd)
        x = np.concatenate([hi, lo])
        xl = hi.astype(LD) + lo.astype(LD)
    elif use == 4:
        x = xd.astype(np.float32)
        xl = x.astype(LD)
    else:
        x, xl = xd, xd.astype(LD)
    ny = (2 * n if use == 2 else n) + 5

    def run():
        y = np.full(ny, kr.SENTINEL, dtype=np.float32 if use in (1, 2) else np.float64)
        call("das_debug_krylov_scale_to", n, a, use, vp(x), vp(y), ny)
        return y

    y = twice(run)
    assert np.all(y[ny - 5 :] == y.dtype.type(kr.SENTINEL)), "guard band overwritten"
    ref, mag = kr.ref_scale(a, xl)
    if use == 1:
        ok, ratio = kr.check_fp32(y[:n], ref)
    elif use == 2:
        ok, ratio = kr.check_split(y[:n], y[n : 2 * n], ref, mag, 1, a)
    else:
        ok, ratio = kr.check_update(y[:n], ref, mag, 1, a)
    record("k_scale_to " + SCALE_USES[use] + (" (fp32 ulps)" if use == 1 else ""), "-", ratio)
    assert ok, ratio


# ---- 4. the block path -----------------------------------------------------------------------------------------------------------
def block(X, ld):
    """rows of X as the columns of a column-major block with leading dimension ld, sentinel in the padding"""
    a = np.full(X.shape[0] * ld, kr.SENTINEL)
    a.reshape(X.shape[0], ld)[:, : X.shape[1]] = X
    return a


def unblock(a, k, n, ld):
    st = a.reshape(k, ld)
    assert np.all(st[:, n:] == kr.SENTINEL), "guard band overwritten"
    return st[:, :n]


def block_cases():
    out = [(n, 5, s) for n, s in kr.ns_shapes()] + [(n, K, 8) for K in kr.K_LIST for n in (4097, 16 * 1024 + 1)] + [(257, K, 3) for K in kr.K_LIST]
    return [pytest.param(n, K, s, False, id=f"n{n}-K{K}-s{s}") for n, K, s in sorted(set(out)) if n * K <= kr.MAX_DOUBLES] + [
        pytest.param(n, K, s, True, id=f"n{n}-K{K}-s{s}-ill") for n, K, s in ((65, 5, 3), (4097, 65, 8), (16 * 1024 + 1, 9, 5))]


def block_lds(n, K):
    return [n] if n * K > 2_000_000 else [n, n + 1, n + 2]


@pytest.mark.parametrize("n,K,s,ill", block_cases())
def test_block_tn(n, K, s, ill):
    V, W = kr.vectors(n, K, 71, ill), kr.vectors(n, s, 72, ill)
    ref, mag = kr.ref_block_tn(V, W)
    for ld in block_lds(n, K):  # odd leading dimension: scalar loads of k_tsgemm_tn; even: the 16-byte loads
        Vb, Wb = block(V, ld), block(W, ld)

        def run():
            Cm = np.zeros(K * s)
            call("das_debug_krylov_block_tn", n, K, s, dp(Vb), ld, 0, dp(Wb), ld, dp(Cm))
            return Cm

        got = twice(run).reshape(K, s)
        ok, ratio = kr.check_sum(got, ref, mag, n)
        record("block_tn", "fp64", ratio)
        assert ok, (ld, ratio)


@pytest.mark.parametrize("n,K,s,ill", block_cases())
def test_block_nn_sub(n, K, s, ill):
    V, W = kr.vectors(n, K, 81, ill), kr.vectors(n, s, 82, ill)
    Cm = 0.25 * kr.vector(K * s, [83, K]).reshape(K, s)
    ref, mag = kr.ref_block_nn_sub(V, Cm, W)
    for ld in block_lds(n, K):
        Vb, Wb0 = block(V, ld), block(W, ld + 1)

        def run():
            Wb = Wb0.copy()
            call("das_debug_krylov_block_nn_sub", n, K, s, dp(Vb), ld, dp(np.ascontiguousarray(Cm.ravel())), dp(Wb), ld + 1)
            return Wb

        got = unblock(twice(run), s, n, ld + 1)
        ok, ratio = kr.check_update(got, ref, mag, K + 1)
        record("block_nn_sub", "fp64", ratio)
        assert ok, (ld, ratio)


@pytest.mark.parametrize("n,K,s,ill", block_cases())
def test_block_lincomb(n, K, s, ill):
    V = kr.vectors(n, K, 91, ill)
    Cm = kr.vector(K * s, [92, K]).reshape(K, s)
    ref, mag = kr.ref_block_comb(V, Cm)
    for ld in block_lds(n, K):
        Vb = block(V, ld)

        def run():
            Y = np.full(s * (ld + 2), kr.SENTINEL)
            call("das_debug_krylov_block_lincomb", n, K, s, dp(Vb), ld, dp(np.ascontiguousarray(Cm.ravel())), dp(Y), ld + 2)
            return Y

        got = unblock(twice(run), s, n, ld + 2)
        ok, ratio = kr.check_sum(got, ref, mag, K)
        record("k_block_lincomb", "fp64", ratio)
        assert ok, (ld, ratio)


@pytest.mark.parametrize("ill", [False, True], ids=["well", "ill"])
@pytest.mark.parametrize("n,s", kr.ns_shapes(), ids=lambda v: str(v))
def test_block_right_mult(n, s, ill):
    W = kr.vectors(n, s, 101, ill)
    T = np.triu(kr.vector(s * s, [102, s]).reshape(s, s))  # upper triangular like the inverse Cholesky factor
    ref, mag = kr.ref_right_mult(W, T)
    for ld in (n, n + 1):
        Wb0 = block(W, ld)

        def run():
            Wb = Wb0.copy()
            call("das_debug_krylov_block_right_mult", n, s, dp(Wb), ld, dp(np.ascontiguousarray(T.ravel())))
            return Wb

        got = unblock(twice(run), s, n, ld)
        ok, ratio = kr.check_sum(got, ref, mag, s)
        record("k_block_right_mult", "fp64", ratio)
        assert ok, (ld, ratio)


CSR_N = 333  # not a multiple of 16


@pytest.mark.parametrize("ill", [False, True], ids=["well", "ill"])
@pytest.mark.parametrize("last", ["empty", "longest"])
@pytest.mark.parametrize("s", kr.S_LIST)
def test_block_spmm(s, last, ill):
    rp, ci, val = kr.make_csr(CSR_N, 111, last, ill)
    X = kr.vectors(CSR_N, s, 112, ill)
    ref, mag, rowlen = kr.ref_csr_rows(rp, ci, val, X)
    for ld in (CSR_N, CSR_N + 1):
        Xb = block(X, ld)

        def run():
            Y = np.full(s * (ld + 3), kr.SENTINEL)
            call("das_debug_krylov_block_spmm", CSR_N, s, rp.ctypes.data_as(_capi.c_ll_p), ci.ctypes.data_as(_capi.c_int_p), dp(val), dp(Xb), ld, dp(Y), ld + 3)
            return Y

        got = unblock(twice(run), s, CSR_N, ld + 3)
        ok, ratio = kr.check_sum(got, ref, mag, rowlen[None, :])
        record("block_spmm", "fp64", ratio)
        assert ok, (ld, ratio)


@pytest.mark.parametrize("ill", [False, True], ids=["well", "ill"])
@pytest.mark.parametrize("last", ["empty", "longest"])
def test_spmv_wave(last, ill):
    """k_spmv_wave on an arbitrary CSR through das_mat_create_from_csr + das_mat_mult"""
    rp, ci, val = kr.make_csr(CSR_N, 121, last, ill)
    x = kr.vector(CSR_N, 122, ill)
    ref, mag, rowlen = kr.ref_csr_rows(rp, ci, val, x[None, :])
    h = C.c_void_p()
    call("das_mat_create_from_csr", CSR_N, rp.ctypes.data_as(_capi.c_ll_p), ci.ctypes.data_as(_capi.c_int_p), dp(val), C.byref(h))
    try:

        def run():
            y = np.full(CSR_N, kr.SENTINEL)
            call("das_mat_mult", h, dp(x), dp(y))
            return y

        got = twice(run)
    finally:
        _capi.lib().das_mat_destroy(h)
    ok, ratio = kr.check_sum(got, ref[0], mag[0], rowlen)
    record("k_spmv_wave", "fp64", ratio)
    assert ok, ratio


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    L = _capi.lib()
    n, K, s = 8, 2, 2
    V, v, out = np.ones(K * n), np.ones(n), np.zeros(2 * K)
    f32 = np.ones(2 * K * n, dtype=np.float32)
    bad = [
        L.das_debug_krylov_dots2(0, K, 0, vp(V), n, dp(v), dp(out)),
        L.das_debug_krylov_dots2(n, 0, 0, vp(V), n, dp(v), dp(out)),
        L.das_debug_krylov_dots2(n, K, 3, vp(V), n, dp(v), dp(out)),
        L.das_debug_krylov_dots2(n, K, 0, vp(V), n - 1, dp(v), dp(out)),
        L.das_debug_krylov_dots2(n, K, 2, vp(f32), 2 * n - 1, dp(v), dp(out)),
        L.das_debug_krylov_dots2(n, K, 0, None, n, dp(v), dp(out)),
        L.das_debug_krylov_dots2(n, K, 0, vp(V), n, None, dp(out)),
        L.das_debug_krylov_dcgs2_update(n, 1, 0, vp(V), n, 2, dp(v), 0.5, 1.0, dp(v)),   # needs slots 0 .. j + 1
        L.das_debug_krylov_dcgs2_update(n, -1, 0, vp(V), n, 2, dp(v), 0.5, 1.0, dp(v)),
        L.das_debug_krylov_multidot(n, -1, 0, vp(V), n, dp(v), dp(out)),
        L.das_debug_krylov_multiaxpy(n, K, 0, vp(V), n, dp(v), 0, vp(v.copy()), n - 1),
        L.das_debug_krylov_multiaxpy(n, K, 0, vp(V), n, dp(v), 1, vp(v.copy()), n),       # float w with an fp64 basis
        L.das_debug_krylov_lincomb(n, K, 0, vp(V), n, dp(v), dp(v.copy()), n - 1),
        L.das_debug_krylov_scale_to(n, 1.0, 5, vp(v), vp(v.copy()), n),
        L.das_debug_krylov_scale_to(n, 1.0, 2, vp(v), vp(f32), 2 * n - 1),
        L.das_debug_krylov_block_tn(n, K, 0, dp(V), n, 0, dp(V), n, dp(out)),
        L.das_debug_krylov_block_tn(n, K, 9, dp(V), n, 0, dp(V), n, dp(out)),
        L.das_debug_krylov_block_tn(n, K, s, dp(V), n - 1, 0, dp(V), n, dp(out)),
        L.das_debug_krylov_block_tn(n, K, s, dp(V), n, 0, None, n, dp(out)),
        L.das_debug_krylov_block_nn_sub(n, K, 9, dp(V), n, dp(out), dp(V.copy()), n),
        L.das_debug_krylov_block_right_mult(n, 9, dp(V.copy()), n, dp(out)),
        L.das_debug_krylov_block_lincomb(n, K, s, dp(V), n, dp(out), dp(V.copy()), n - 1),
    ]
    assert all(rc == -1 for rc in bad), bad  # DAS_ERR_ARG
    # even leading dimensions with the block at an odd offset: the 16-byte loads of k_tsgemm_tn would be misaligned
    assert L.das_debug_krylov_block_tn(n, 1, 1, dp(V), n, 1, dp(V), n, dp(out)) == -1 and b"16-byte" in L.das_last_error()
    rp = np.array([0, 1, 2], dtype=np.int64)
    ci = np.array([0, 2], dtype=np.int32)  # column 2 of a 2 x 2 matrix
    X, Y = np.ones(2), np.zeros(2)
    assert L.das_debug_krylov_block_spmm(2, 1, rp.ctypes.data_as(_capi.c_ll_p), ci.ctypes.data_as(_capi.c_int_p), dp(X), dp(X), 2, dp(Y), 2) == -1
    assert b"out of range" in L.das_last_error()
    # an odd offset with ODD leading dimensions takes the scalar loads and is fine
    Vo = np.concatenate([[kr.SENTINEL], kr.vector(9, 1)])
    Wo, Co = kr.vector(9, 2), np.zeros(1)
    call("das_debug_krylov_block_tn", 9, 1, 1, dp(Vo), 9, 1, dp(Wo), 9, dp(Co))
    ref, mag = kr.ref_dot(Vo[1:], Wo)
    assert kr.check_sum(Co, ref, mag, 9)[0]


def test_zzz_print_achieved_errors(capsys):
    """not an assertion: the achieved max err / (u magnitude) of everything that ran in this module"""
    with capsys.disabled():
        print("\n| operation | storage | max err / (u magnitude) |\n|---|---|---|")
        for (op, fmt), r in sorted(FIGURES.items()):
            print(f"| {op} | {fmt} | {r:.3g} |")

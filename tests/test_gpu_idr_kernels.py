"""The kernels of the IDR(s) solver (csrc/das_idr.hpp) one by one on the device against longdouble restatements, with the method of
tests/test_gpu_krylov_kernels.py: no mesh, no solver.  The entries das_debug_idr_* run the launch helpers the solver runs, on caller
data.  Bounds are derived (krylov_reference: a sum of T products |err| <= T u sum|x y|; an entry built from T terms |err| <= (T + 2) u
sum|terms|), never tuned to what the kernels give.  Every call runs twice for bitwise equality, everything a kernel may write sits in a
sentinel guard band, and what it must not touch is compared with its input.  Shapes: the grid arithmetic (256 rows per workgroup, 512
on the 16-byte path, MD_CHUNK 1024, more than one workgroup) and both load paths - leading dimension n and n + 3: an even one takes
the 16-byte path (with the element-wise last row when n is odd), an odd one the element-wise path.
The sums are judged against the STORED vector the kernel wrote (it sums the very values it stores), the vectors against exact arithmetic."""
import ctypes as C

import numpy as np
import pytest

import krylov_reference as kr
from dafoam_amd import _capi
from krylov_reference import LD, SENTINEL

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")]

N_LIST = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 16 * 1024 + 1, 40000]
S_LIST = [1, 2, 3, 4, 8]
K_LIST = sorted({k for s in S_LIST for k in (0, 1, s - 1) if k < s})  # 0, 1, 2, 3, 7
ILL_N = [17, 1025, 4097]
PAD = 5


def dp(a):
    return _capi.dptr(a)


def call(name, *args):
    _capi.check(getattr(_capi.lib(), name)(*args))


def twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two runs on the same input differ bitwise"
    return a


def columns(V, ld, extra=1):
    """K vectors as columns ld apart in a flat array, the padding and `extra` more columns filled with the sentinel"""
    K, n = V.shape
    a = np.full((K + extra) * ld, SENTINEL)
    a.reshape(K + extra, ld)[:K, :n] = V
    return a


def padded(v):
    a = np.full(v.size + PAD, SENTINEL)
    a[: v.size] = v
    return a


def cases(second, ill_second):
    return [pytest.param(n, q, False, id=f"n{n}-{q}") for n in N_LIST for q in second] + [pytest.param(n, q, True, id=f"n{n}-{q}-ill") for n in ILL_N for q in ill_second]


# ---- 1. the shadow space -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", N_LIST)
def test_shadow_fill_equals_the_host_hash_bitwise(n):
    for s, seed in ((1, 1), (8, 1), (3, 77)):
        for ld in (n, n + 3):
            def run(device):
                P = np.full((s + 1) * ld, SENTINEL)
                call("das_debug_idr_shadow", n, s, ld, seed, device, dp(P))
                return (P,)

            host = run(0)[0]
            dev = twice(lambda: run(1))[0]
            assert dev.tobytes() == host.tobytes()
            st = dev.reshape(s + 1, ld)
            assert np.all(st[:s, n:] == SENTINEL) and np.all(st[s] == SENTINEL), "guard band overwritten"
            assert np.all(np.abs(st[:s, :n]) < 1.0)


# ---- 2. y = a x + sum c_i V_i ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aliased", [False, True], ids=["separate", "inplace"])
@pytest.mark.parametrize("n,m,ill", cases(S_LIST, [3, 8]))
def test_combine(n, m, ill, aliased):
    V = kr.vectors(n, m, 61, ill)
    x = kr.vector(n, [62, m], ill)
    c = 0.5 * kr.vector(m, [63, m])
    a = -0.8125
    ref = LD(a) * x.astype(LD)
    mag = np.abs(ref)
    for i in range(m):
        t = LD(c[i]) * V[i].astype(LD)
        ref = ref + t
        mag = mag + np.abs(t)
    for ld in (n, n + 3):
        V0 = columns(V, ld)

        def run():
            Va, y = V0.copy(), np.full(n + PAD, SENTINEL)
            call("das_debug_idr_combine", n, m, a, dp(x), dp(Va), ld, Va.size, dp(c), 0 if aliased else -1, dp(y), y.size)
            return Va, y

        Va, y = twice(run)
        got = Va[:n] if aliased else y[:n]
        ok, ratio = kr.check_update(got, ref, mag, m + 1)
        print(f"k_idr_combine n={n} m={m} ld={ld} {'in place' if aliased else 'separate'}: max err / (u sum|terms|) = {ratio:.3g} (bound {m + 3})")
        assert ok, ratio
        if aliased:
            assert np.array_equal(Va[n:], V0[n:]), "the in-place combination touched more than column 0"
            assert np.all(y == SENTINEL)
        else:
            assert np.array_equal(Va, V0), "V was modified"
            assert np.all(y[n:] == SENTINEL), "guard band overwritten"


# ---- 3. the fused biorthogonalisation step -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k,ill", cases(K_LIST, [2, 7]))
def test_biortho_step(n, k, ill):
    Gv, Uv = kr.vectors(n, k + 1, 71, ill), kr.vectors(n, k + 1, 72, ill)
    r, x = kr.vector(n, [73, k], ill), kr.vector(n, [74, k], ill)
    coef = np.append(0.25 * kr.vector(max(k, 1), [75, k])[:k], 0.6875)
    beta = LD(coef[k])

    def exact(W, v, sign):
        """w' = W_k - sum alpha_j W_j and v + sign beta w', with the sums of the absolute values of their terms"""
        w, mw = W[k].astype(LD), np.abs(W[k].astype(LD))
        for j in range(k):
            t = LD(coef[j]) * W[j].astype(LD)
            w = w - t
            mw = mw + np.abs(t)
        return w, mw, v.astype(LD) + sign * beta * w, np.abs(v.astype(LD)) + np.abs(beta) * mw

    g, mg, rn, mr = exact(Gv, r, -1)
    u, mu, xn, mx = exact(Uv, x, +1)
    for ld in (n, n + 3):
        G0, U0 = columns(Gv, ld), columns(Uv, ld)

        def run():
            Ga, Ua, ra, xa, rr = G0.copy(), U0.copy(), padded(r), padded(x), np.zeros(1)
            call("das_debug_idr_biortho_step", n, k, dp(Ga), dp(Ua), ld, Ga.size, dp(coef), dp(ra), dp(xa), ra.size, dp(rr))
            return Ga, Ua, ra, xa, rr

        Ga, Ua, ra, xa, rr = twice(run)
        Gs, Us = Ga.reshape(k + 2, ld), Ua.reshape(k + 2, ld)
        figs = {}
        for name, got, ref, mag, T in (("g_k", Gs[k, :n], g, mg, k + 1), ("u_k", Us[k, :n], u, mu, k + 1), ("r", ra[:n], rn, mr, k + 2), ("x", xa[:n], xn, mx, k + 2)):
            ok, figs[name] = kr.check_update(got, ref, mag, T)
            assert ok, (name, figs[name])
        sref, smag = kr.ref_dot(ra[:n], ra[:n])
        ok, figs["r.r"] = kr.check_sum(rr, sref, smag, n)
        print(f"k_idr_biortho_step n={n} k={k} ld={ld}: max err / (u magnitude) " + ", ".join(f"{a} {b:.3g}" for a, b in figs.items()) + f" (bounds {k + 3}, {k + 3}, {k + 4}, {k + 4}, {n})")
        assert ok, figs["r.r"]
        for A, A0 in ((Ga, G0), (Ua, U0)):
            keep = np.ones(A.size, bool)
            if k > 0:
                keep[k * ld : k * ld + n] = False
            assert np.array_equal(A[keep], A0[keep]), "columns 0 .. k-1, the padding or the guard column were modified"
        if k == 0:
            assert np.array_equal(Ga, G0) and np.array_equal(Ua, U0)  # k = 0 is the plain r, x update
        assert np.all(ra[n:] == SENTINEL) and np.all(xa[n:] == SENTINEL), "guard band overwritten"


# ---- 4. the fused smoothing step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,s,ill", cases(S_LIST, [3, 8]))
def test_smooth_step(n, s, ill):
    Pv = kr.vectors(n, s, 81, ill)
    r, t, x, z = (kr.vector(n, [82 + i, s], ill) for i in range(4))
    omega = 0.71875
    rn, mr = r.astype(LD) - LD(omega) * t.astype(LD), np.abs(r.astype(LD)) + np.abs(LD(omega) * t.astype(LD))
    xn, mx = x.astype(LD) + LD(omega) * z.astype(LD), np.abs(x.astype(LD)) + np.abs(LD(omega) * z.astype(LD))
    for ld in (n, n + 3):
        P0 = columns(Pv, ld)

        def run():
            ra, xa, Pa, out = padded(r), padded(x), P0.copy(), np.zeros(s + 1)
            call("das_debug_idr_smooth_step", n, s, omega, dp(ra), dp(t), dp(xa), dp(z), ra.size, dp(Pa), ld, Pa.size, dp(out))
            return ra, xa, Pa, out

        ra, xa, Pa, out = twice(run)
        ok1, f1 = kr.check_update(ra[:n], rn, mr, 2)
        ok2, f2 = kr.check_update(xa[:n], xn, mx, 2)
        refs = [kr.ref_dot(Pv[i], ra[:n]) for i in range(s)] + [kr.ref_dot(ra[:n], ra[:n])]
        ok3, f3 = kr.check_sum(out, np.array([a for a, _ in refs], dtype=LD), np.array([b for _, b in refs], dtype=LD), n)
        print(f"k_idr_smooth_step n={n} s={s} ld={ld}: max err / (u magnitude) r {f1:.3g}, x {f2:.3g} (bound 4), sums {f3:.3g} (bound {n})")
        assert ok1 and ok2 and ok3, (f1, f2, f3)
        assert np.array_equal(Pa, P0), "P was modified"
        assert np.all(ra[n:] == SENTINEL) and np.all(xa[n:] == SENTINEL), "guard band overwritten"


def test_the_multi_dots_of_the_solver_are_the_existing_kernel():
    """P^T g_k (with g_k.g_k) and (r.t, t.t) go through launch_multidot with m = s and m = 1: the shapes IDR(s) uses, once more"""
    for n, m in ((1, 1), (4097, 1), (4097, 8), (40000, 4)):
        V, w = kr.vectors(n, m, 91), kr.vector(n, [92, m])
        B = kr.Basis(V, kr.FP64, n)
        out = np.zeros(m + 1)
        call("das_debug_krylov_multidot", n, m, kr.FP64, B.a.ctypes.data_as(C.c_void_p), n, dp(w), dp(out))
        ref, mag = kr.ref_multidot(B, m, w)
        ok, ratio = kr.check_sum(out, ref, mag, n)
        assert ok, ratio

"""CPU tier of amd.polyDegree (polynomial-preconditioned GMRES, csrc/das_poly_host.hpp): the roots of the GMRES polynomial from the
Hessenberg matrix of a d-step cycle (harmonic Ritz values, one representative per complex pair, modified Leja order) and the root walk
t = p(B) v in real arithmetic.  das_debug_poly_apply_host runs THE walk the device solver runs (poly_walk) on host vectors with callback
operator and preconditioner, so the device tier adds only the kernels of csrc/das_poly.hpp (tests/test_gpu_poly_kernels.py) and the
solver's bookkeeping (tests/test_gpu_poly_gmres.py).  Systems: the channel adjoints of tests/test_idrs_host_cpu.py with the oracle's ILU(0)."""
import ctypes as C

import numpy as np
import pytest

from common import relerr
from dafoam_amd import _capi
from dafoam_amd._capi import dptr
from dafoam_amd.meshgen import channel_case
from krylov_reference import LD, U
from test_idrs_host_cpu import System, wrap

DEGREES = [1, 2, 3, 4, 8, 16]


# ---- numpy restatements --------------------------------------------------------------------------------------------------------
def arnoldi(op, b, d):
    """d steps of Arnoldi (modified Gram-Schmidt, twice) from b: the unrotated (d + 1) x d Hessenberg matrix and |b|"""
    n = b.size
    V, H = np.zeros((d + 1, n)), np.zeros((d + 1, d))
    beta = np.linalg.norm(b)
    V[0] = b / beta
    for j in range(d):
        w = op(V[j])
        for _ in range(2):
            for i in range(j + 1):
                h = V[i] @ w
                H[i, j] += h
                w = w - h * V[i]
        H[j + 1, j] = np.linalg.norm(w)
        V[j + 1] = w / H[j + 1, j]
    return H, beta


def gmres_residual(H, beta):
    d = H.shape[1]
    e1 = np.zeros(d + 1)
    e1[0] = beta
    y = np.linalg.lstsq(H, e1, rcond=None)[0]
    return np.linalg.norm(e1 - H @ y)


def harmonic_ritz(H):
    d = H.shape[1]
    Hd = H[:d, :d]
    f = np.linalg.solve(Hd.T, np.eye(d)[:, d - 1])
    G = Hd.copy()
    G[:, d - 1] += H[d, d - 1] ** 2 * f
    return np.linalg.eigvals(G)


def roots_of(H):
    d = H.shape[1]
    re, im = np.full(16, np.nan), np.full(16, np.nan)
    m = _capi.lib().das_debug_poly_roots(d, dptr(np.ascontiguousarray(H)), dptr(re), dptr(im))
    assert m >= 0, _capi.lib().das_last_error()
    return re[:m].copy(), im[:m].copy()


def poly_apply(n, cA, cM, re, im, v):
    out = np.zeros(n)
    rc = _capi.lib().das_debug_poly_apply_host(n, C.cast(cA, C.c_void_p), C.cast(cM, C.c_void_p), None, re.size, dptr(re), dptr(im), dptr(np.ascontiguousarray(v)), dptr(out))
    assert rc == 0, _capi.lib().das_last_error()
    return out


def with_conjugates(re, im):
    out = []
    for a, b in zip(re, im):
        out += [complex(a, b)] + ([complex(a, -b)] if b != 0.0 else [])
    return np.array(out)


@pytest.fixture(scope="module")
def channel765():
    return System(channel_case(7, 6, 5), "volume")


@pytest.fixture(scope="module")
def channel12106():
    return System(channel_case(12, 10, 6), "volume")


def precond_operator(S):
    return lambda v: S.A @ S.pc(v)


# ---- roots --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DEGREES)
def test_roots_are_the_harmonic_ritz_values_in_modified_leja_order(channel765, d):
    S = channel765
    H, _ = arnoldi(precond_operator(S), S.rhs, d)
    re, im = roots_of(H)
    re2, im2 = roots_of(H)
    assert re.tobytes() == re2.tobytes() and im.tobytes() == im2.tobytes(), "two calls differ"
    assert re.size >= 1 and np.all(im >= 0.0) and np.all(np.isfinite(re)) and np.all(np.isfinite(im))
    got = with_conjugates(re, im)
    ref = harmonic_ritz(H)
    assert got.size == d  # real roots + 2 x pairs: every pair is represented once, by im > 0
    key = lambda z: (round(z.real, 9), round(z.imag, 9))  # noqa: E731
    gs, rs = np.array(sorted(got, key=key)), np.array(sorted(ref, key=key))
    err = np.max(np.abs(gs - rs) / np.abs(rs))
    print(f"d = {d}: {re.size} entries, {int(np.sum(im > 0))} pairs, max relative distance to numpy's harmonic Ritz values {err:.2e}")
    assert err <= 1e-10
    # modified Leja order
    z = re + 1j * im
    assert np.abs(z)[0] == np.max(np.abs(z))
    for i in range(1, z.size):
        placed = with_conjugates(re[:i], im[:i])
        with np.errstate(divide="ignore"):
            f = np.array([np.sum(np.log(np.abs(c - placed))) for c in z[i:]])
        assert f[0] >= np.max(f) - 1e-12 * max(1.0, np.max(np.abs(f[np.isfinite(f)]), initial=0.0)), (i, f)


def test_a_zero_harmonic_ritz_value_reports_the_fallback():
    """a rank-deficient Hessenberg matrix (zero first column): H_d^T H_d + h^2 e_d e_d^T is singular, a harmonic Ritz value is zero - no polynomial"""
    for H in (np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 1.0]]), np.array([[0.0], [0.0]]), np.array([[np.nan], [1.0]])):
        re, im = roots_of(H)
        assert re.size == 0


# ---- the host apply against the product formula in complex longdouble -------------------------------------------------------------
N_DENSE = 40


@pytest.fixture(scope="module")
def dense_system():
    """a normal 40 x 40 matrix with a prescribed spectrum: real eigenvalues in [0.5, 2] and complex pairs of modulus 0.6 .. 1.9 (condition
    number 4), B = Q D Q^T with Q orthogonal"""
    rng = np.random.default_rng(7)
    Q, _ = np.linalg.qr(rng.standard_normal((N_DENSE, N_DENSE)))
    D = np.zeros((N_DENSE, N_DENSE))
    for i, lam in enumerate(np.linspace(0.5, 2.0, 20)):
        D[i, i] = lam
    for q in range(10):
        a, b = 0.6 + 0.1 * q, 0.2 + 0.12 * q
        i = 20 + 2 * q
        D[i : i + 2, i : i + 2] = [[a, b], [-b, a]]
    B = Q @ D @ Q.T
    v = rng.standard_normal(N_DENSE)
    return B, v, wrap(lambda x: B @ x, N_DENSE), wrap(lambda x: x.copy(), N_DENSE)


def walk_with_running_bound(B, re, im, v):
    """the root walk restated in longdouble with a running bound of what fp64 evaluation may deviate by: an entry built from T terms errs
    by at most (T + 2) u sum|terms| (krylov_reference), a product B x of n terms by (n + 2) u |B| |x|, and input errors pass through
    |B| and the divisions"""
    n = v.size
    Bl, aB = B.astype(LD), np.abs(B.astype(LD))
    u = LD(U)

    def matvec(x, ex):
        return Bl @ x, aB @ ex + (n + 2) * u * (aB @ np.abs(x))

    prod, eprod = v.astype(LD), np.zeros(n, dtype=LD)
    poly, epoly = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for i in range(re.size):
        last = i == re.size - 1
        a, b = LD(re[i]), LD(im[i])
        if im[i] == 0.0:
            t = prod / a
            epoly = epoly + eprod / abs(a) + 4 * u * (np.abs(poly) + np.abs(t))
            poly = poly + t
            if not last:
                w, ew = matvec(prod, eprod)
                t2 = w / a
                eprod = eprod + ew / abs(a) + 4 * u * (np.abs(prod) + np.abs(t2))
                prod = prod - t2
        else:
            m2 = LD(re[i] * re[i] + im[i] * im[i])  # as the walk forms it, in fp64
            w, ew = matvec(prod, eprod)
            tmp = 2 * a * prod - w
            etmp = 2 * abs(a) * eprod + ew + 4 * u * (np.abs(2 * a * prod) + np.abs(w))
            t = tmp / m2
            epoly = epoly + etmp / m2 + 4 * u * (np.abs(poly) + np.abs(t))
            poly = poly + t
            if not last:
                w, ew = matvec(tmp, etmp)
                t2 = w / m2
                eprod = eprod + ew / m2 + 4 * u * (np.abs(prod) + np.abs(t2))
                prod = prod - t2
    return poly, epoly


def product_formula(B, re, im, v):
    """B^-1 (v - prod_i (I - B / theta_i) v) in complex longdouble; the solve by fp64 LU refined in longdouble (condition number 4)"""
    CL = np.clongdouble
    Bl = B.astype(CL)
    x = v.astype(CL)
    for th in with_conjugates(re, im):
        x = x - (Bl @ x) / CL(th)
    rhs = (v.astype(CL) - x)
    assert np.max(np.abs(rhs.imag)) <= 2.0 ** -50 * np.max(np.abs(rhs.real))  # conjugate pairs: the product is real
    rhs = rhs.real.astype(LD)
    Br = B.astype(LD)
    sol = np.zeros(v.size, dtype=LD)
    for _ in range(6):
        sol = sol + np.linalg.solve(B, (rhs - Br @ sol).astype(np.float64)).astype(LD)
    return sol


ROOT_SETS = {
    "d1-real": ([1.3], [0.0]),
    "d2-pair": ([0.9], [0.7]),
    "d4-real-last": ([1.9, 0.8, 0.6], [0.0, 0.9, 0.0]),
    "d4-pair-last": ([1.7, 0.6, 1.0], [0.0, 0.0, 0.5]),
    "d5-pair-last": ([1.6, 1.1, 0.7], [0.9, 0.0, 0.4]),
    "d5-real-last": ([1.0, 0.8, 1.4], [0.5, 0.9, 0.0]),
    "d16": ([2.0, 0.5, 1.2, 0.8, 1.6, 0.65, 1.0, 1.4, 0.9, 1.8, 0.55], [0.0, 0.0, 0.8, 0.0, 0.3, 0.4, 0.0, 0.0, 1.0, 0.6, 0.0]),
}


@pytest.mark.parametrize("name", list(ROOT_SETS))
def test_host_apply_equals_the_product_formula(dense_system, name):
    B, v, cA, cM = dense_system
    re, im = (np.array(x) for x in ROOT_SETS[name])
    got = poly_apply(N_DENSE, cA, cM, re, im, v)
    walk, bound = walk_with_running_bound(B, re, im, v)
    ref = product_formula(B, re, im, v)
    # the references' own error: longdouble against fp64 is 2^-11; a factor 8 for the complex arithmetic and the refined solve
    tol = bound + LD(2.0 ** -8) * np.max(bound)
    e1, e2 = np.abs(got.astype(LD) - ref), np.abs(walk - ref)
    print(f"{name}: max |twin - formula| / bound = {float(np.max(e1 / tol)):.3g}, max |longdouble walk - formula| / bound = {float(np.max(e2 / tol)):.3g}")
    assert np.all(np.isfinite(got)) and np.all(e1 <= tol)
    assert np.all(e2 <= LD(2.0 ** -8) * np.max(bound))  # the two references agree far inside the fp64 bound
    if name == "d1-real":
        assert np.array_equal(got, v / re[0])  # degree 1: exactly v / theta


# ---- the identity |b - B p(B) b| = GMRES(d) residual -----------------------------------------------------------------------------
@pytest.mark.parametrize("d", DEGREES)
@pytest.mark.parametrize("which", ["channel765", "channel12106"])
def test_polynomial_residual_equals_the_gmres_residual_of_its_cycle(request, which, d):
    S = request.getfixturevalue(which)
    op = precond_operator(S)
    H, beta = arnoldi(op, S.rhs, d)
    rho = gmres_residual(H, beta)
    re, im = roots_of(H)
    assert re.size >= 1
    t = poly_apply(S.n, S.cA, S.cM, re, im, S.rhs)
    got = np.linalg.norm(S.rhs - op(t))
    print(f"{which} d = {d}: |b - B p(B) b| = {got:.6e}, GMRES({d}) residual {rho:.6e}, relative difference {abs(got - rho) / rho:.2e}")
    assert abs(got - rho) <= 1e-9 * rho


# ---- a GMRES over B p(B) reaches the direct solution -----------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 8])
@pytest.mark.parametrize("which", ["channel765", "channel12106"])
def test_gmres_over_the_polynomial_operator_reaches_the_direct_solution(request, which, d):
    S = request.getfixturevalue(which)
    H, _ = arnoldi(precond_operator(S), S.rhs, d)
    re, im = roots_of(H)
    p = lambda v: poly_apply(S.n, S.cA, S.cM, re, im, v)  # noqa: E731
    op = lambda v: S.A @ S.pc(p(v))  # noqa: E731
    n, m = S.n, 80
    beta = np.linalg.norm(S.rhs)
    V, Hh = np.zeros((m + 1, n)), np.zeros((m + 1, m))
    V[0] = S.rhs / beta
    cols = 0
    for j in range(m):
        w = op(V[j])
        for _ in range(2):
            for i in range(j + 1):
                h = V[i] @ w
                Hh[i, j] += h
                w = w - h * V[i]
        Hh[j + 1, j] = np.linalg.norm(w)
        V[j + 1] = w / Hh[j + 1, j]
        cols = j + 1
        e1 = np.zeros(cols + 1)
        e1[0] = beta
        y = np.linalg.lstsq(Hh[: cols + 1, :cols], e1, rcond=None)[0]
        if np.linalg.norm(e1 - Hh[: cols + 1, :cols] @ y) <= 1e-10 * beta:
            break
    x = S.pc(p(V[:cols].T @ y))
    print(f"{which} d = {d}: {cols} columns, {cols * d} products, psi error {relerr(x, S.xd):.2e}, true rel {np.linalg.norm(S.rhs - S.A @ x) / beta:.2e}")
    assert cols < m and relerr(x, S.xd) <= 1e-7


def test_defaults():
    from dafoam_amd.pyDAFoam import DAOPTION

    assert DAOPTION().amd["polyDegree"] == 0

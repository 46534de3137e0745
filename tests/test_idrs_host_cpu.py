"""CPU tier of amd.krylovMethod "idrs": the IDR(s) iteration (idrs_loop in csrc/das_idr_host.hpp) is written once over a handful of vector
operations; das_debug_idrs_host runs THAT loop on host vectors with callback operator and preconditioner - so the small triangular
solves, the one-pass biorthogonalisation, the smoothing step, the true-residual check, the restart and the stagnation rule are tested
here, and the device solver adds only the kernels of csrc/das_idr.hpp (tests/test_gpu_idr_kernels.py)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from common import norm_states, relerr
from dafoam_amd import _capi
from dafoam_amd._capi import dptr
from dafoam_amd.meshgen import channel_case
from oracle import jacobian as J
from oracle import linear as OL
from oracle.foam_mesh import Geometry

APPLY = C.CFUNCTYPE(None, _capi.c_double_p, _capi.c_double_p, C.c_void_p)


def wrap(f, n):
    def cb(xp, yp, _u):
        x = np.ctypeslib.as_array(xp, shape=(n,))
        np.ctypeslib.as_array(yp, shape=(n,))[:] = f(x)

    return APPLY(cb)


class System:
    """the adjoint system of a channel with the oracle's ILU(0) in the [U, p, nuTilda] node permutation (the preconditioner of
    test_gmres_dr_loop_host_twin) and the sparse direct solution"""

    def __init__(self, case, rhs_kind):
        g = Geometry(case.mesh)
        sc = J.state_scales(case, g, norm_states(case))
        con = J.connectivity(case, g)
        col, _ = J.greedy_coloring(con)
        A = J.jacobian_colored(case, g, case.states, con, col, sc, mode="cs", lower_bound=0).tocsr()
        n, N = A.shape[0], g.nC
        perm = np.concatenate([np.array([3 * c, 3 * c + 1, 3 * c + 2, 3 * N + c, 4 * N + c]) for c in range(N)] + [np.arange(5 * N, n)])
        Ap = sp.csr_matrix(A[perm][:, perm])
        Ap.sort_indices()
        ilu = OL.ILU(Ap, fill=0)

        def pc(v):
            y = np.empty(n)
            y[perm] = ilu.solve(np.ascontiguousarray(v[perm]))
            return y

        if rhs_kind == "volume":
            rhs = np.zeros(n)
            rhs[0 : 3 * N : 3] = g.V
            rhs *= sc
        else:
            rhs = np.ones(n) * sc
        self.A, self.n, self.rhs, self.pc = A, n, rhs, pc
        self.xd = spla.spsolve(A.tocsc(), rhs)
        self.cA, self.cM = wrap(lambda v: A @ v, n), wrap(pc, n)

    def idrs(self, s, seed, rtol, maxit, atol=1e-300):
        x, hist, info, res = np.zeros(self.n), np.zeros(maxit + 8), np.zeros(4), np.zeros(2)
        fail = _capi.lib().das_debug_idrs_host(self.n, C.cast(self.cA, C.c_void_p), C.cast(self.cM, C.c_void_p), None, dptr(self.rhs), dptr(x), s, seed, rtol, atol, maxit,
                                               dptr(hist), hist.size, dptr(info), dptr(res))
        assert fail >= 0, _capi.lib().das_last_error()
        its = int(info[0])
        return dict(x=x, fail=fail, its=its, reason=int(info[1]), restarts=int(info[2]), breakdowns=int(info[3]), res0=res[0], res=res[1], hist=hist[: its + 1].copy())

    def full_gmres_iterations(self, rtol=1e-10):
        x, hist, info, res = np.zeros(self.n), np.zeros(2008), np.zeros(4), np.zeros(2)
        fail = _capi.lib().das_debug_gmres_dr_host(self.n, C.cast(self.cA, C.c_void_p), C.cast(self.cM, C.c_void_p), None, dptr(self.rhs), dptr(x), 600, 1, rtol, 1e-300, 2000,
                                                   dptr(hist), hist.size, dptr(info), dptr(res))
        assert fail == 0
        return int(info[0])


@pytest.fixture(scope="module")
def channel765():
    S = System(channel_case(7, 6, 5), "volume")
    S.it_full = S.full_gmres_iterations()
    return S


@pytest.fixture(scope="module")
def channel321():
    return System(channel_case(3, 2, 1, wall_function=True), "ones")


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_idrs_reaches_the_direct_solution_with_about_the_products_of_full_gmres(channel765, s, seed):
    """rtol 1e-10 on the 7 x 6 x 5 channel: return code 0, the TRUE relative residual within the tolerance, psi within 1e-8 of the sparse
    direct solve, and no more than 2 x (full GMRES iterations) + 10 operator products (prototype: 37-51 against 35)."""
    S = channel765
    R = S.idrs(s, seed, 1e-10, 2000)
    true_rel = np.linalg.norm(S.rhs - S.A @ R["x"]) / np.linalg.norm(S.rhs)
    print(f"IDR({s}) seed {seed}: {R['its']} products (full GMRES {S.it_full}), true rel {true_rel:.3e}, psi err {relerr(R['x'], S.xd):.3e}, restarts {R['restarts']}, breakdowns {R['breakdowns']}")
    assert R["fail"] == 0 and R["reason"] == 0
    assert true_rel <= 1e-10
    assert abs(R["res"] / R["res0"] - true_rel) <= 1e-3 * true_rel + 1e-16  # what the loop reports IS the true residual
    assert relerr(R["x"], S.xd) <= 1e-8
    assert R["its"] <= 2 * S.it_full + 10
    assert R["hist"].size == R["its"] + 1 and R["hist"][0] == R["res0"]  # one residual norm per product


def test_unreachable_tolerance_stops_on_stagnation(channel321):
    """gmresRelTol 1e-30 on the 59-unknown channel: the recurrence residual reaches what the true residual cannot; the loop restarts from
    the true residual and stops (reason 2) as soon as a restarted run does not halve it - well inside the budget, psi at direct-solve accuracy."""
    S = channel321
    for s in (1, 4):
        R = S.idrs(s, 1, 1e-30, 1000)
        print(f"IDR({s}): stopped after {R['its']} products, reason {R['reason']}, restarts {R['restarts']}, rel {R['res'] / R['res0']:.3e}, psi err {relerr(R['x'], S.xd):.3e}")
        assert R["reason"] == 2 and R["fail"] == 1 and R["restarts"] >= 1
        assert R["its"] <= 500
        assert relerr(R["x"], S.xd) <= 1e-8


def test_budget_counts_every_product_and_non_finite_input_ends_the_solve(channel765):
    """gmresMaxIters bounds the operator products, the closing true residual included; a non-finite right-hand side ends at once."""
    S = channel765
    calls = [0]
    cA = wrap(lambda v: (calls.__setitem__(0, calls[0] + 1), S.A @ v)[1], S.n)
    for maxit in (2, 7, 12):
        calls[0] = 0
        x, hist, info, res = np.zeros(S.n), np.zeros(maxit + 8), np.zeros(4), np.zeros(2)
        fail = _capi.lib().das_debug_idrs_host(S.n, C.cast(cA, C.c_void_p), C.cast(S.cM, C.c_void_p), None, dptr(S.rhs), dptr(x), 4, 1, 1e-10, 1e-300, maxit, dptr(hist),
                                               hist.size, dptr(info), dptr(res))
        assert fail == 1 and info[1] == 1 and info[0] == maxit
        assert calls[0] == maxit + 1  # + the residual of the start vector (x = 0), which no solver counts
        assert abs(res[1] - np.linalg.norm(S.rhs - S.A @ x)) <= 1e-12 * res[0]
    bad = S.rhs.copy()
    bad[3] = np.nan
    x, info, res = np.zeros(S.n), np.zeros(4), np.zeros(2)
    fail = _capi.lib().das_debug_idrs_host(S.n, C.cast(S.cA, C.c_void_p), C.cast(S.cM, C.c_void_p), None, dptr(bad), dptr(x), 4, 1, 1e-10, 1e-300, 100, None, 0, dptr(info),
                                           dptr(res))
    assert fail == 1 and info[1] == 3 and info[0] == 0


def sequential_cycle(A, pc, b, P):
    """one cycle of IDR(s) with biorthogonalisation as published (van Gijzen and Sonneveld, ACM TOMS 38, Algorithm 2; right-preconditioned),
    from x = 0: g_k is biorthogonalised against p_0 .. p_{k-1} ONE AFTER THE OTHER"""
    n, s = P.shape
    x, r = np.zeros(n), b.copy()
    G, U, M, om = np.zeros((n, s)), np.zeros((n, s)), np.eye(s), 1.0
    f = P.T @ r
    for k in range(s):
        c = np.linalg.solve(M[k:, k:], f[k:])
        v = pc(r - G[:, k:] @ c)
        U[:, k] = U[:, k:] @ c + om * v
        G[:, k] = A @ U[:, k]
        for i in range(k):
            alpha = P[:, i] @ G[:, k] / M[i, i]
            G[:, k] -= alpha * G[:, i]
            U[:, k] -= alpha * U[:, i]
        M[k:, k] = P[:, k:].T @ G[:, k]
        beta = f[k] / M[k, k]
        r -= beta * G[:, k]
        x += beta * U[:, k]
        f[k + 1 :] -= beta * M[k + 1 :, k]
        f[: k + 1] = 0.0
    v = pc(r)
    t = A @ v
    om = (t @ r) / (t @ t)
    rho = abs(t @ r) / (np.linalg.norm(t) * np.linalg.norm(r))
    if rho < 0.7:
        om *= 0.7 / rho
    return x + om * v, r - om * t, G


def test_one_cycle_equals_the_published_sequential_biorthogonalisation():
    """The loop takes d = P^T g_k in one pass and gets alpha by forward substitution with M; the published form uses k dependent inner
    products.  One cycle (s + 1 products, s = 4) on a random diagonally dominant 200 x 200 matrix with a Jacobi preconditioner: x and r
    agree to 1e-10, and P^T G is lower triangular to 1e-12 of its largest entry."""
    n, s = 200, 4
    rng = np.random.default_rng(7)
    A = rng.standard_normal((n, n)) / np.sqrt(n) + np.diag(4.0 + rng.random(n))
    b = rng.standard_normal(n)
    dinv = 1.0 / np.diag(A)
    cA, cM = wrap(lambda v: A @ v, n), wrap(lambda v: dinv * v, n)
    x, r, P, G, U = np.zeros(n), np.zeros(n), np.zeros(s * n), np.zeros(s * n), np.zeros(s * n)
    _capi.check(_capi.lib().das_debug_idr_cycle_host(n, C.cast(cA, C.c_void_p), C.cast(cM, C.c_void_p), None, dptr(b), dptr(x), s, 1, dptr(r), dptr(P), dptr(G), dptr(U)))
    P, G, U = P.reshape(s, n).T, G.reshape(s, n).T, U.reshape(s, n).T
    assert np.abs(P.T @ P - np.eye(s)).max() <= 1e-13  # the shadow space is orthonormal
    xs, rs, Gs = sequential_cycle(A, lambda v: dinv * v, b, P)
    print("x", relerr(x, xs), "r", relerr(r, rs), "recurrence vs true residual", relerr(r, b - A @ x))
    assert relerr(x, xs) <= 1e-10 and relerr(r, rs) <= 1e-10
    assert relerr(r, b - A @ x) <= 1e-10
    assert relerr(G, Gs) <= 1e-10 and relerr(G, A @ U) <= 1e-12
    PtG = P.T @ G
    assert np.abs(np.triu(PtG, 1)).max() <= 1e-12 * np.abs(PtG).max()
    assert np.abs(r).max() < np.abs(b).max()  # ... and the cycle did something


def test_shadow_space_is_a_deterministic_function_of_seed_row_and_column():
    L = _capi.lib()

    def shadow(n, s, seed, ld=None):
        ld = ld or n
        P = np.full(s * ld, 7.0)
        _capi.check(L.das_debug_idr_shadow(n, s, ld, seed, 0, dptr(P)))
        return P.reshape(s, ld)

    P1, P1b, P2 = shadow(1000, 8, 1), shadow(1000, 8, 1), shadow(1000, 8, 2)
    assert P1.tobytes() == P1b.tobytes()
    assert np.all(P1 != P2)
    assert np.all(np.abs(P1) < 1.0) and np.all(np.abs(P2) < 1.0)
    # uniform in (-1, 1): mean 0, variance 1/3 (8000 samples: 5 sigma), no two columns alike, entry (row, col) independent of n, s and ld
    assert abs(P1.mean()) < 5 * np.sqrt(1 / 3 / 8000) and abs(P1.var() - 1 / 3) < 0.03
    assert np.abs(np.corrcoef(P1)[np.triu_indices(8, 1)]).max() < 0.2
    Q = shadow(17, 3, 1, ld=20)
    assert np.array_equal(Q[:, :17], P1[:3, :17]) and np.all(Q[:, 17:] == 7.0)
    # two solves of the same system: identical bits
    n = 60
    rng = np.random.default_rng(3)
    A = rng.standard_normal((n, n)) / np.sqrt(n) + 3.0 * np.eye(n)
    b = rng.standard_normal(n)
    cA, cM = wrap(lambda v: A @ v, n), wrap(lambda v: v.copy(), n)
    out = []
    for _ in range(2):
        x, info = np.zeros(n), np.zeros(4)
        assert L.das_debug_idrs_host(n, C.cast(cA, C.c_void_p), C.cast(cM, C.c_void_p), None, dptr(b), dptr(x), 4, 1, 1e-10, 1e-300, 500, None, 0, dptr(info), None) == 0
        out.append((x.tobytes(), info[0]))
    assert out[0] == out[1]


def test_krylov_method_defaults_to_gmres_in_the_mirror_and_in_the_library():
    from common import options
    from dafoam_amd.pyDAFoam import DAOPTION
    from dafoam_amd.pyDASolvers import pyDASolvers

    d = DAOPTION()
    assert d.amd["krylovMethod"] == "gmres" and d.amd["idrShadowVectors"] == 4 and d.amd["idrSeed"] == 1
    case = channel_case(4, 4, 3)
    bare = {k: v for k, v in options(case).items() if k != "amd"}  # nothing pushed from the mirror: the library's own table
    s = pyDASolvers(b"DASimpleFoam -python", bare, case=case)
    buf = C.create_string_buffer(64)
    _capi.check(_capi.lib().das_get_option_string(s._h, b"amd.krylovMethod", buf, 64))
    assert buf.value == b"gmres"

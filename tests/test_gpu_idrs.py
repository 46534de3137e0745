"""GPU tier of amd.krylovMethod "idrs": IDR(s) through the whole adjoint path - the loop of csrc/das_idr_host.hpp (CPU tier:
tests/test_idrs_host_cpu.py) over the kernels of csrc/das_idr.hpp (tests/test_gpu_idr_kernels.py), the node-block ILU + coarse-space
preconditioner and the assembled operator - against the default solver and the sparse direct solve."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from common import norm_states, options, relerr
from dafoam_amd.meshgen import channel_case
from oracle import jacobian as J
from oracle.foam_mesh import Geometry

pytestmark = pytest.mark.gpu


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=options(case, **extra), case=case)


def oracle_matrix(case, g):
    sc = J.state_scales(case, g, norm_states(case))
    con = J.connectivity(case, g)
    col, _ = J.greedy_coloring(con)
    return sc, J.jacobian_colored(case, g, case.states, con, col, sc, mode="cs", lower_bound=0)


def volume_rhs(case, g):
    rhs = np.zeros(case.states.size)
    rhs[0 : 3 * g.nC : 3] = g.V
    return rhs * J.state_scales(case, g, norm_states(case))


@pytest.fixture(scope="module")
def converged_channel():
    """the case and right-hand side of test_gmres_deflated_restarting_matches_the_default_solver, with the default solver's answer"""
    from oracle.primal import solve_primal

    case = channel_case(10, 8, 6, perturb=0.0, lengths=(1.0, 0.2, 0.2), grading_y=2.0)
    g = Geometry(case.mesh)
    case.states, _ = solve_primal(case, g, max_iters=800, tol=1e-11)
    rhs = volume_rhs(case, g)
    base = {"gmresRelTol": 1e-10, "gmresAbsTol": 1e-300, "printInfo": 0, "gmresMaxIters": 1500, "gmresRestart": 1500}
    D = make(case, adjEqnOption=base)
    psi, fail = D.solveAdjoint(rhs)
    assert fail == 0
    return dict(case=case, rhs=rhs, base=base, psi=psi, it_full=D.ksp.info()["iters"], D=D)


def test_idrs_matches_the_default_solver_without_a_krylov_basis(converged_channel):
    """IDR(4) at rtol 1e-10: the default solver's psi to 1e-7, at most 2 x its iterations + 10 operator products (the cap of the GMRES-DR
    test; on the CPU with the oracle's ILU(0) the ratio was at most 1.2), 3 s + 5 <= 3 s + 8 work vectors of 8 n bytes, and no Krylov
    basis: basisInfo() is what a KSP that has never solved reports."""
    c = converged_channel
    n = c["rhs"].size
    D = make(c["case"], adjEqnOption=c["base"], amd={"krylovMethod": "idrs"})
    psi, fail = D.solveAdjoint(c["rhs"])
    info, st, idr = D.ksp.info(), D.ksp.status(), D.ksp.idrInfo()
    print("products: IDR(4)", info["iters"], "full GMRES iterations", c["it_full"], "rel", info["res"] / info["res0"], st, idr)
    assert fail == 0 and st["reason"] == 0 and info["res"] <= 1e-10 * info["res0"]
    assert relerr(psi, c["psi"]) <= 1e-7
    assert idr["s"] == 4 and idr["cycles"] >= 1
    assert idr["workVectors"] <= 3 * 4 + 8 and idr["workBytes"] == idr["workVectors"] * 8 * n
    assert D.ksp.history().size == info["iters"] + 1  # one residual norm per product
    # no basis was reserved or mapped: a KSP built the same way that never solved
    from dafoam_amd.pyDASolvers import KSP

    fresh = KSP().create()
    D.solverAD.createMLRKSPMatrixFree(D.dRdWTPC, fresh)
    assert D.ksp.basisInfo() == fresh.basisInfo() and fresh.basisInfo()["mappedGB"] == 0.0
    assert fresh.idrInfo()["cycles"] == 0 and fresh.idrInfo()["workVectors"] == 0
    assert info["iters"] <= 2 * c["it_full"] + 10, (info["iters"], c["it_full"])


def test_the_default_solver_is_untouched(converged_channel):
    """without the option: GMRES, idrInfo() empty, and the iteration count of the first default solve"""
    c = converged_channel
    assert c["D"].ksp.idrInfo()["cycles"] == 0 and c["D"].ksp.idrInfo()["workVectors"] == 0
    D = make(c["case"], adjEqnOption=c["base"])
    psi, fail = D.solveAdjoint(c["rhs"])
    assert fail == 0 and D.ksp.info()["iters"] == c["it_full"] and D.ksp.idrInfo()["cycles"] == 0
    assert relerr(psi, c["psi"]) <= 1e-9


def test_nonzero_initial_guess_ends_within_one_cycle(converged_channel):
    """useNonZeroInitGuess with the converged psi as the start.  The tolerances apply as they do for GMRES - relative to the residual of
    the START vector - so the absolute tolerance carries the level the first solve reached (1e-10 |b|): the solve has nothing left to do
    and must see that from the true residual of its start vector, within s + 2 products; a solve that ignored the guess would need
    about the 40 of the first one."""
    c = converged_channel
    bnorm = np.linalg.norm(c["rhs"])
    D = make(c["case"], adjEqnOption=dict(c["base"], useNonZeroInitGuess=1, gmresAbsTol=1e-10 * bnorm), amd={"krylovMethod": "idrs"})
    psi, fail = D.solveAdjoint(c["rhs"], psi0=c["psi"])
    info = D.ksp.info()
    print("products from the converged start", info["iters"], "res0", info["res0"], "res", info["res"], "|b|", bnorm)
    assert fail == 0 and info["iters"] <= 4 + 2
    assert info["res0"] <= 1.01e-10 * bnorm  # the start residual is the one of psi0, not |b|
    assert relerr(psi, c["psi"]) <= 1e-7


@pytest.mark.parametrize("s", [1, 8])
def test_shadow_space_sizes_against_the_direct_solve(s):
    case = channel_case(7, 6, 5)
    g = Geometry(case.mesh)
    sc, A = oracle_matrix(case, g)
    rhs = volume_rhs(case, g)
    ref = spla.spsolve(A.tocsc(), rhs)
    D = make(case, adjEqnOption={"gmresRelTol": 1e-10, "gmresAbsTol": 1e-300, "printInfo": 0}, amd={"krylovMethod": "idrs", "idrShadowVectors": s})
    psi, fail = D.solveAdjoint(rhs)
    print(f"IDR({s}):", D.ksp.info(), D.ksp.idrInfo())
    assert fail == 0 and relerr(psi, ref) <= 1e-7
    assert D.ksp.idrInfo()["s"] == s and D.ksp.idrInfo()["workVectors"] == 3 * s + 5


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 2, 1)])
def test_degenerate_meshes_are_solved_identically_every_time(dims):
    """a single cell / a handful of cells (s is clamped to n, the shadow space may span everything): psi against the direct solve, and four
    fresh solver objects in one process give one product count and bitwise identical psi"""
    case = channel_case(*dims, wall_function=True)
    g = Geometry(case.mesh)
    sc, A = oracle_matrix(case, g)
    rhs = np.ones(case.states.size) * sc
    ref = spla.spsolve(A.tocsc(), rhs)
    runs = []
    for rep in range(4):
        D = make(case, adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0}, jacLowerBounds={"dRdW": 0.0, "dRdWPC": 0.0}, amd={"krylovMethod": "idrs"})
        psi, fail = D.solveAdjoint(rhs)
        st = D.ksp.status()
        print(dims, "run", rep, D.ksp.info(), st, D.ksp.idrInfo())
        assert relerr(psi, ref) <= 1e-8 and st["reason"] in (0, 2)
        runs.append((D.ksp.info()["iters"], psi.tobytes()))
    assert len(set(runs)) == 1


def test_unreachable_tolerance_stops_on_stagnation():
    case = channel_case(3, 2, 1, wall_function=True)
    g = Geometry(case.mesh)
    sc, A = oracle_matrix(case, g)
    rhs = np.ones(case.states.size) * sc
    ref = spla.spsolve(A.tocsc(), rhs)
    D = make(case, adjEqnOption={"gmresRelTol": 1e-30, "gmresAbsTol": 1e-300, "gmresMaxIters": 1000, "printInfo": 0}, amd={"krylovMethod": "idrs"})
    psi, fail = D.solveAdjoint(rhs)
    info, st = D.ksp.info(), D.ksp.status()
    print(info, st, D.ksp.idrInfo())
    assert st["reason"] == 2 and info["iters"] < 1000 and fail == 1
    assert relerr(psi, ref) <= 1e-8


class DeviceVector:
    """n doubles on the device, through the HIP runtime the library itself has loaded"""

    def __init__(self, host):
        from dafoam_amd._capi import lib

        lib()
        # (another package may have brought a HIP runtime of its own into the process: the library's is the one that sees the device)
        cnt = C.c_int(0)
        for path in sorted({line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line}, key=lambda q: "site-packages" in q or "dist-packages" in q):
            self.hip = C.CDLL(path)
            if self.hip.hipGetDeviceCount(C.byref(cnt)) == 0 and cnt.value > 0:
                break
        self.n, self.p = host.size, C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.p), C.c_size_t(8 * self.n)) == 0
        assert self.hip.hipMemcpy(self.p, host.ctypes.data_as(C.c_void_p), C.c_size_t(8 * self.n), 1) == 0

    def to_host(self):
        out = np.empty(self.n)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.p, C.c_size_t(8 * self.n), 2) == 0
        return out

    def free(self):
        self.hip.hipFree(self.p)


def test_device_resident_solve_and_fixed_windows():
    """das_ksp_begin_device / advance / end with "idrs": the first advance runs the whole solve (same psi and product count as the
    host-array entry); a fixed-iteration window keeps GMRES silently and leaves the IDR(s) figures alone."""
    from dafoam_amd._capi import check, lib

    case = channel_case(7, 6, 5)
    g = Geometry(case.mesh)
    rhs = volume_rhs(case, g)
    D = make(case, adjEqnOption={"gmresRelTol": 1e-10, "gmresAbsTol": 1e-300, "printInfo": 0}, amd={"krylovMethod": "idrs"})
    psi, fail = D.solveAdjoint(rhs)
    its = D.ksp.info()["iters"]
    assert fail == 0
    L, h = lib(), D.solver._h
    D.solverAD.initializedRdWTMatrixFree()
    d_rhs, d_sol = DeviceVector(rhs), DeviceVector(np.full(rhs.size, 3.0))
    try:
        check(L.das_ksp_begin_device(h, D.ksp.handle, d_rhs.p, d_sol.p, 0))
        assert check(L.das_ksp_advance(h, D.ksp.handle, 3)) == 1
        assert check(L.das_ksp_advance(h, D.ksp.handle, 3)) == 1  # over: nothing runs twice
        assert check(L.das_ksp_end(h, D.ksp.handle)) == 0
        assert D.ksp.info()["iters"] == its and d_sol.to_host().tobytes() == psi.tobytes()
        before = D.ksp.idrInfo()
        check(L.das_ksp_run_fixed_device(h, D.ksp.handle, d_rhs.p, d_sol.p, 5))
        # (the delayed re-orthogonalisation reports the columns it has completed: one behind the steps of a window)
        assert 0 < D.ksp.info()["iters"] <= 5 and D.ksp.idrInfo() == before and D.ksp.basisInfo()["bytesPerVector"] == 8.0 * rhs.size
    finally:
        d_rhs.free()
        d_sol.free()
    D.solverAD.destroydRdWTMatrixFree()
    # ... and the next IDR(s) solve on this KSP is the first one again
    psi2, fail2 = D.solveAdjoint(rhs)
    assert fail2 == 0 and D.ksp.info()["iters"] == its and psi2.tobytes() == psi.tobytes()


def test_bad_options_raise():
    case = channel_case(3, 2, 1, wall_function=True)
    rhs = np.ones(case.states.size)
    with pytest.raises(Exception, match="krylovMethod"):
        make(case, amd={"krylovMethod": "bicg"}).solveAdjoint(rhs)
    for s in (0, 9):
        with pytest.raises(Exception, match="idrShadowVectors"):
            make(case, amd={"krylovMethod": "idrs", "idrShadowVectors": s}).solveAdjoint(rhs)
    with pytest.raises(Exception, match="gmresDeflation"):
        make(case, amd={"krylovMethod": "idrs", "gmresDeflation": 4}).solveAdjoint(rhs)

"""GPU tier of amd.polyDegree: polynomial-preconditioned GMRES through the whole adjoint path - the roots and the root walk of
csrc/das_poly_host.hpp (CPU tier: tests/test_poly_host_cpu.py) over the kernels of csrc/das_poly.hpp (tests/test_gpu_poly_kernels.py),
the node-block ILU + coarse-space preconditioner and the assembled operator - against the default solver and the sparse direct solve."""

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
    """the construction of tests/test_gpu_idrs.py: the 10 x 8 x 6 channel about its converged primal, rtol 1e-10, with the default solver's answer"""
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


@pytest.fixture(scope="module")
def poly4(converged_channel):
    c = converged_channel
    D = make(c["case"], adjEqnOption=c["base"], amd={"polyDegree": 4})
    psi, fail = D.solveAdjoint(c["rhs"])
    return dict(D=D, psi=psi, fail=fail)


def operator_product(D, x):
    """dRdW^T x through the matrix-free transposed product (the scaling of the adjoint system)"""
    y = np.zeros(x.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", D.getStates(), "residuals", "residual", np.ascontiguousarray(x), y)
    return y


def test_degree_4_matches_the_default_solver_with_fewer_columns(converged_channel, poly4):
    """d = 4 at rtol 1e-10: the default solver's psi to 1e-7 with a true residual inside the tolerance; columns <= 0.6 x and products <=
    2.5 x + 2 d of the default solver's iterations.  Columns are counted as the CPU prototype counted them (13 of 35 and 19 of 53 = 0.36-0.37
    with the oracle's ILU(0), products 1.5-1.6 x): the Arnoldi columns over B p(B), i.e. the basis, without the d columns of the generating
    cycle, whose products are counted; the margin is for the other preconditioner.  Measured on the MI355X with the node-block ILU + coarse
    space: 4 generating + 25 columns and 114 products against 44 iterations (0.57 and 2.59 x; all 29 columns would be 0.66).  The basis
    stays inside min(gmresRestart, ceil(maxIters / d) + d) columns (+ 2 slots)."""
    c, D, d = converged_channel, poly4["D"], 4
    n = c["rhs"].size
    info, st, pi, basis = D.ksp.info(), D.ksp.status(), D.ksp.polyInfo(), D.ksp.basisInfo()
    true_res = np.linalg.norm(c["rhs"] - operator_product(D, poly4["psi"]))
    print("polyDegree 4:", pi, "iters", info["iters"], "full GMRES iterations", c["it_full"], "true rel", true_res / info["res0"], st, "cycles", D.ksp.cycleLengths(), basis)
    assert poly4["fail"] == 0 and st["reason"] == 0
    assert info["res"] <= 1e-10 * info["res0"]  # (the true residual of the closing cycle, recomputed on the device)
    assert true_res <= 1.001e-10 * info["res0"]  # the same through the matrix-free product: other rounding, 1e-3 of the tolerance
    assert relerr(poly4["psi"], c["psi"]) <= 1e-7
    assert pi["degree"] == d and pi["generated"] == 1 and pi["fallback"] == 0
    assert sum(2 if im > 0 else 1 for _, im in pi["roots"]) == d and pi["nComplexPairs"] == sum(im > 0 for _, im in pi["roots"])
    assert pi["workVectors"] == 3 and pi["workBytes"] == 3 * 8 * n
    assert info["iters"] == pi["products"] and pi["generatingColumns"] == d
    assert D.ksp.history().size == d + pi["columns"] + 1 and sum(D.ksp.cycleLengths()) == d + pi["columns"]
    bound = min(c["base"]["gmresRestart"], -(-c["base"]["gmresMaxIters"] // d) + d)
    assert basis["mappedGB"] * 2**30 <= (bound + 2) * 8 * ((n + 3) // 4 * 4)
    assert pi["columns"] <= 0.6 * c["it_full"], (pi["columns"], c["it_full"])
    assert pi["products"] <= 2.5 * c["it_full"] + 2 * d, (pi["products"], c["it_full"])


def test_polynomial_residual_on_the_device_is_the_generating_cycle_s(converged_channel, poly4):
    """|b - B p(B) b| with p(B) b from the device apply and one more product through das_ksp_apply_pc and dRdW^T: the true residual the
    history holds at the end of the generating cycle (entry d), to a relative 1e-8"""
    from dafoam_amd._capi import check, dptr, lib

    c, D, d = converged_channel, poly4["D"], 4
    b = c["rhs"]
    t = np.zeros(b.size)
    D.solverAD.initializedRdWTMatrixFree()
    try:
        check(lib().das_debug_ksp_poly_apply(D.solver._h, D.ksp.handle, dptr(b), dptr(t)))
    finally:
        D.solverAD.destroydRdWTMatrixFree()
    got = np.linalg.norm(b - operator_product(D, D.ksp.applyPC(D.solver, t)))
    want = D.ksp.history()[d]
    print("|b - B p(B) b|", got, "history entry", want, "relative difference", abs(got - want) / want, "cycles", D.ksp.cycleLengths())
    assert D.ksp.cycleLengths()[0] == d
    assert abs(got - want) <= 1e-8 * want


def test_the_default_solver_is_untouched(converged_channel):
    c = converged_channel
    pi = c["D"].ksp.polyInfo()
    assert pi["degree"] == 0 and pi["workVectors"] == 0 and pi["workBytes"] == 0 and pi["roots"] == []
    D = make(c["case"], adjEqnOption=c["base"])
    psi, fail = D.solveAdjoint(c["rhs"])
    assert fail == 0 and D.ksp.info()["iters"] == c["it_full"]
    assert D.ksp.polyInfo()["degree"] == 0 and D.ksp.polyInfo()["workVectors"] == 0
    assert relerr(psi, c["psi"]) <= 1e-9


def test_restarted_solve_keeps_its_polynomial(converged_channel):
    c = converged_channel
    D = make(c["case"], adjEqnOption=dict(c["base"], gmresRestart=5), amd={"polyDegree": 4})
    psi, fail = D.solveAdjoint(c["rhs"])
    pi, lens = D.ksp.polyInfo(), D.ksp.cycleLengths()
    print("gmresRestart 5, d = 4:", pi, "cycles", lens, D.ksp.info())
    assert fail == 0 and D.ksp.status()["reason"] == 0 and relerr(psi, c["psi"]) <= 1e-7
    assert pi["generated"] == 1 and pi["degree"] == 4 and max(lens) <= 5 and lens[0] == 4


def test_the_budget_counts_operator_products(converged_channel):
    c = converged_channel
    D = make(c["case"], adjEqnOption=dict(c["base"], gmresMaxIters=20), amd={"polyDegree": 8})
    _, fail = D.solveAdjoint(c["rhs"])
    info, pi = D.ksp.info(), D.ksp.polyInfo()
    print("gmresMaxIters 20, d = 8:", info, pi, D.ksp.status())
    assert info["iters"] <= 20 and info["iters"] == pi["products"] and fail == 1 and D.ksp.status()["reason"] == 1


def test_nonzero_initial_guess_ends_at_once(converged_channel):
    """useNonZeroInitGuess with the converged psi and the absolute tolerance at the level the first solve reached (as in tests/test_gpu_idrs.py):
    nothing is left to do, within d + 2 products"""
    c, d = converged_channel, 4
    bnorm = np.linalg.norm(c["rhs"])
    D = make(c["case"], adjEqnOption=dict(c["base"], useNonZeroInitGuess=1, gmresAbsTol=1e-10 * bnorm), amd={"polyDegree": d})
    psi, fail = D.solveAdjoint(c["rhs"], psi0=c["psi"])
    info = D.ksp.info()
    print("products from the converged start", info["iters"], "res0", info["res0"], "res", info["res"], "|b|", bnorm)
    assert fail == 0 and info["iters"] <= d + 2
    assert info["res0"] <= 1.01e-10 * bnorm
    assert relerr(psi, c["psi"]) <= 1e-7


@pytest.fixture(scope="module")
def channel765():
    case = channel_case(7, 6, 5)
    g = Geometry(case.mesh)
    sc, A = oracle_matrix(case, g)
    rhs = volume_rhs(case, g)
    return case, rhs, spla.spsolve(A.tocsc(), rhs)


@pytest.mark.parametrize("d", [1, 3, 16])
def test_degrees_against_the_direct_solve(channel765, d):
    case, rhs, ref = channel765
    D = make(case, adjEqnOption={"gmresRelTol": 1e-10, "gmresAbsTol": 1e-300, "printInfo": 0}, amd={"polyDegree": d})
    psi, fail = D.solveAdjoint(rhs)
    pi = D.ksp.polyInfo()
    print(f"polyDegree {d}:", D.ksp.info(), pi, D.ksp.cycleLengths())
    assert fail == 0 and relerr(psi, ref) <= 1e-7
    assert pi["degree"] == d and pi["generated"] == 1


def test_bad_combinations_raise():
    case = channel_case(3, 2, 1, wall_function=True)
    rhs = np.ones(case.states.size)
    for d in (17, -1):
        with pytest.raises(Exception, match="polyDegree"):
            make(case, amd={"polyDegree": d}).solveAdjoint(rhs)
    with pytest.raises(Exception, match="polyDegree"):
        make(case, amd={"polyDegree": 4, "krylovMethod": "idrs"}).solveAdjoint(rhs)
    with pytest.raises(Exception, match="polyDegree"):
        make(case, amd={"polyDegree": 4, "gmresDeflation": 4}).solveAdjoint(rhs)
    with pytest.raises(Exception, match="polyDegree"):
        make(case, amd={"polyDegree": 4}).solveAdjoint(np.stack([rhs, 2.0 * rhs], axis=1))

"""variableVolSum, patchMean and variance objectives on the device: values, state-scaled dF/dW, boundary-value / field / volCoord
products and the errors, against the numpy restatement (tests/function_restatement.py)."""
import copy
import math

import numpy as np
import pytest

import function_restatement as FR
from common import norm_states, options
from dafoam_amd.meshgen import (bench_channel_case, channel_case, rho_channel_case, scalar_transport_case, simple_T_channel_case,
                                turbo_channel_case)
from oracle import functions as Fn
from oracle import jacobian as J
from oracle.foam_mesh import Geometry
from oracle.residual import residual

pytestmark = pytest.mark.gpu

# reference tests/runUnitTests_DAFunction.py:72-211, verbatim
UNIT_FUNCTIONS = {
    "PMean": {"type": "patchMean", "source": "patchToFace", "patches": ["inlet"], "varName": "p", "varType": "scalar", "index": 0, "scale": 1.0},
    "UMean": {"type": "patchMean", "source": "patchToFace", "patches": ["outlet"], "varName": "U", "varType": "vector", "index": 0, "scale": 1.0},
    "PVolSum": {"type": "variableVolSum", "source": "allCells", "varName": "p", "varType": "scalar", "index": 0, "isSquare": 0, "multiplyVol": 1,
                "divByTotalVol": 0, "scale": 1.0},
    "UVolSum": {"type": "variableVolSum", "source": "boxToCell", "min": [0.2, 0.2, 0.3], "max": [0.8, 0.8, 0.9], "varName": "U", "varType": "vector",
                "index": 0, "isSquare": 1, "multiplyVol": 0, "divByTotalVol": 1, "scale": 1.0},
    "PVar": {"type": "variance", "source": "allCells", "scale": 1.0, "mode": "field", "varName": "p", "varType": "scalar", "indices": [0],
             "useGeoWeight": True, "timeDependentRefData": False},
    "UOutVar": {"type": "variance", "source": "patchToFace", "patches": ["outlet"], "scale": 1.0, "mode": "surface", "varName": "U", "varType": "vector",
                "indices": [0], "useGeoWeight": True, "timeDependentRefData": False},
}


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=options(case, **extra), case=case)


def restated(case, g, fd, W, beta=None):
    t = fd["type"]
    if t == "variableVolSum":
        return FR.variable_vol_sum(case, g, W, fd, beta)
    if t == "patchMean":
        return FR.patch_mean(case, g, W, fd)
    return FR.variance(case, g, W, fd, case.ref_data)


def with_ref_data(case, g, seed=1):
    """<var>Data = a perturbed copy of the states (internal and boundary values)."""
    rng = np.random.default_rng(seed)
    W = case.states
    b = Fn._boundary_state(case, g, W)
    U, p = FR.cell_values(case, g, W, "U"), FR.cell_values(case, g, W, "p")
    case.ref_data = {
        "UData": {"internal": U * (1 + 0.05 * rng.standard_normal(U.shape)), "boundary": b["Ub"] * (1 + 0.05 * rng.standard_normal(b["Ub"].shape))},
        "pData": {"internal": p + 0.1 * np.abs(p).max() * rng.standard_normal(p.shape), "boundary": b["pb"] + 0.1 * np.abs(p).max() * rng.standard_normal(b["pb"].shape)},
    }
    return case


def unit_case(solver):
    if solver == "DASimpleFoam":
        case = channel_case(6, 5, 4, lengths=(1.0, 1.0, 1.2), wall_function=True, perturb=0.02)
    else:
        case = rho_channel_case(6, 5, 4, lengths=(1.0, 1.0, 1.2), perturb=0.02)
    return with_ref_data(case, Geometry(case.mesh))


@pytest.mark.parametrize("solver", ["DASimpleFoam", "DARhoSimpleFoam"])
def test_values_match_restatement_and_repeat_bitwise(solver):
    case = unit_case(solver)
    g = Geometry(case.mesh)
    D = make(case, function=UNIT_FUNCTIONS)
    for name, fd in UNIT_FUNCTIONS.items():
        Fo = restated(case, g, fd, case.states)
        F1, F2 = D.solver.calcFunction(name), D.solver.calcFunction(name)
        assert F1 == F2, name
        assert Fo != 0.0 and abs(F1 - Fo) <= 1e-12 * abs(Fo), (name, F1, Fo)
    # UVolSum divides by totalVol = 1 + the volume of ALL cells, not only the box's
    fd = UNIT_FUNCTIONS["UVolSum"]
    cells = FR.box_cells(g.C, fd["min"], fd["max"])
    assert 0 < cells.size < g.nC
    Ux = case.states[0 : 3 * g.nC : 3][cells]
    assert abs(D.solver.calcFunction("UVolSum") - (Ux * Ux).sum() / (1.0 + g.V.sum())) <= 1e-12 * abs(D.solver.calcFunction("UVolSum"))


@pytest.mark.parametrize("solver", ["DASimpleFoam", "DARhoSimpleFoam"])
def test_dFdW_matches_complex_step(solver):
    case = unit_case(solver)
    g = Geometry(case.mesh)
    W = case.states
    D = make(case, function=UNIT_FUNCTIONS)
    sc = J.state_scales(case, g, norm_states(case))
    for name, fd in UNIT_FUNCTIONS.items():
        dFo = Fn.gradient(lambda Wp: restated(case, g, fd, Wp), W, sc)
        dF = np.zeros(W.size)
        D.solverAD.calcJacTVecProduct("states", "stateVar", W, name, "function", np.array([1.5]), dF)
        assert np.abs(dF - 1.5 * dFo).max() <= 1e-10 * np.abs(1.5 * dFo).max(), name


def test_boundary_value_and_field_inputs():
    case = unit_case("DASimpleFoam")
    g = Geometry(case.mesh)
    W = case.states
    fns = {
        "UInMean": {"type": "patchMean", "source": "patchToFace", "patches": ["inlet"], "varName": "U", "varType": "vector", "index": 0, "scale": 2.0},
        "pOutVar": {"type": "variance", "source": "patchToFace", "patches": ["outlet"], "scale": 3.0, "mode": "surface", "varName": "p",
                    "varType": "scalar", "indices": [0], "useGeoWeight": 1, "timeDependentRefData": False},
        "BETA2": {"type": "variableVolSum", "source": "allCells", "varName": "betaFINuTilda", "varType": "scalar", "index": 0, "isSquare": 1, "scale": 0.7},
        "PVar": UNIT_FUNCTIONS["PVar"],
        "PVolSum": UNIT_FUNCTIONS["PVolSum"],
    }
    info = {"pv": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"},
            "pOut": {"type": "patchVar", "patches": ["outlet"], "varName": "p", "varType": "scalar"},
            "beta": {"type": "field", "fieldName": "betaFINuTilda", "fieldType": "scalar"}}
    D = make(case, function=fns, inputInfo=info)
    S = D.solverAD
    # patchMean of U_x on the fixedValue inlet: U_x,b = UMag cos(AoA), so dF/dUMag = scale cos(AoA), dF/dAoA = -scale UMag sin(AoA) pi/180
    x = np.array([10.0, 3.0])
    out = np.zeros(2)
    S.calcJacTVecProduct("pv", "patchVelocity", x, "UInMean", "function", np.ones(1), out)
    a = np.deg2rad(3.0)
    exp = np.array([2.0 * np.cos(a), -2.0 * 10.0 * np.sin(a) * np.pi / 180.0])
    assert np.abs(out - exp).max() <= 1e-10 * np.abs(exp).max()
    assert abs(S.calcFunction("UInMean") - 2.0 * 10.0 * np.cos(a)) <= 1e-12 * 20.0
    # variance of the boundary p on the fixedValue outlet: dF/dp_out = scale sum 2 |Sf| (p_out - d) / sum |Sf|
    pv = np.array([0.3])
    S.calcJacTVecProduct("pOut", "patchVar", pv, "pOutVar", "function", np.ones(1), out[:1])
    sel = np.nonzero(Fn._select(g, case, ["outlet"]))[0]
    A, d = g.bMagSf[sel], case.ref_data["pData"]["boundary"][sel]
    exp1 = 3.0 * (2.0 * A * (0.3 - d)).sum() / A.sum()
    assert abs(out[0] - exp1) <= 1e-10 * abs(exp1)
    for name in ("UInMean", "PVar", "PVolSum"):  # the inlet velocity and the cell-set functions do not read the outlet p
        S.calcJacTVecProduct("pOut", "patchVar", pv, name, "function", np.ones(1), out[:1])
        assert out[0] == 0.0, name
    for name in ("PVar", "PVolSum"):
        S.calcJacTVecProduct("pv", "patchVelocity", x, name, "function", np.ones(1), out)
        assert np.all(out == 0.0), name
    # field input: dF/dbeta = 2 scale V beta for the squared betaFINuTilda sum, 0 for the others
    beta = 1.0 + 0.2 * np.random.default_rng(3).standard_normal(g.nC)
    prod = np.zeros(g.nC)
    S.calcJacTVecProduct("beta", "field", beta, "BETA2", "function", np.ones(1), prod)
    exp = 2.0 * 0.7 * g.V * beta
    assert np.abs(prod - exp).max() <= 1e-13 * np.abs(exp).max()
    assert abs(S.calcFunction("BETA2") - FR.variable_vol_sum(case, g, W, fns["BETA2"], beta)) <= 1e-12 * S.calcFunction("BETA2")
    for name in ("PVar", "PVolSum", "UInMean"):
        S.calcJacTVecProduct("beta", "field", beta, name, "function", np.ones(1), prod)
        assert np.all(prod == 0.0), name


def moved_case(case, X):
    c = copy.copy(case)
    c.mesh = copy.deepcopy(case.mesh)
    c.mesh.points = X.reshape(-1, 3).copy()
    return c


def test_volcoord_products_match_central_differences():
    case = unit_case("DASimpleFoam")
    fns = {
        "PVolSum": UNIT_FUNCTIONS["PVolSum"],
        "PVolDiv": dict(UNIT_FUNCTIONS["PVolSum"], divByTotalVol=1, isSquare=1, scale=0.3),
        "UVolRef": dict(UNIT_FUNCTIONS["PVolSum"], varName="U", varType="vector", index=1, calcRefVar=1, ref=[0.02]),
        "PMean": UNIT_FUNCTIONS["PMean"],
        "UMean": UNIT_FUNCTIONS["UMean"],
        "PVar": UNIT_FUNCTIONS["PVar"],
    }
    D = make(case, function=fns, inputInfo={"x": {"type": "volCoord"}})
    S = D.solverAD
    X0 = np.zeros(S.getNLocalPoints() * 3)
    S.getOFMeshPoints(X0)
    rng = np.random.default_rng(5)
    h = 1e-6 * np.abs(X0).max()
    for name in ("PVolSum", "PVolDiv", "UVolRef", "PMean", "UMean"):
        prod = np.zeros(X0.size)
        S.calcJacTVecProduct("x", "volCoord", X0, name, "function", np.ones(1), prod)
        for _ in range(3):
            dX = rng.standard_normal(X0.size)
            vals = []
            for sgn in (1.0, -1.0):
                c = moved_case(case, X0 + sgn * h * dX)
                vals.append(restated(c, Geometry(c.mesh), fns[name], case.states))
            fd_ = (vals[0] - vals[1]) / (2 * h)
            assert abs(prod @ dX - fd_) <= 1e-6 * max(abs(fd_), 1e-12 * np.abs(prod).max() * np.abs(dX).max()), name
    with pytest.raises(Exception, match="variance"):
        S.calcJacTVecProduct("x", "volCoord", X0, "PVar", "function", np.ones(1), np.zeros(X0.size))


def linear_primal(case, g, sc, con, col):
    """The converged DAScalarTransportFoam primal: its residual is linear in T, so one sparse solve of the oracle's residual."""
    import scipy.sparse.linalg as spla

    W = case.states
    A = J.jacobian_colored(case, g, W, con, col, sc, mode="cs", lower_bound=0)  # A[j, i] = s_j dR_i/dW_j
    return W + sc * spla.spsolve(A.T.tocsc(), -residual(case, g, W))


def test_scalar_transport_config0_own_objective():
    """configs[0] with the reference's TVOL (tests/runRegTests_DAScalarTransportFoam.py:38-52, verbatim) and the TIn patchVar input on
    the inlet: dF/dW, the adjoint, and the adjoint total dTVOL/dTIn against a central difference of the oracle primal."""
    TVOL = {"type": "variableVolSum", "source": "allCells", "varName": "T", "varType": "scalar", "index": 0, "isSquare": 0, "divByTotalVol": 0,
            "scale": 1.0, "timeOp": "average", "nStepsFrac": 0.5}
    case = scalar_transport_case()
    g = Geometry(case.mesh)
    sc = J.state_scales(case, g, norm_states(case))
    con = J.connectivity(case, g)
    col, _ = J.greedy_coloring(con)
    case.states = linear_primal(case, g, sc, con, col)
    D = make(case, function={"TVOL": TVOL}, inputInfo={"TIn": {"type": "patchVar", "patches": ["inlet"], "varName": "T", "varType": "scalar"}},
             adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    W = case.states
    assert abs(D.solver.calcFunction("TVOL") - (g.V * W).sum()) <= 1e-12 * abs((g.V * W).sum())
    dF = np.zeros(W.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "TVOL", "function", np.ones(1), dF)
    dFo = Fn.gradient(lambda Wp: FR.variable_vol_sum(case, g, Wp, TVOL), W, sc)
    assert np.abs(dF - dFo).max() <= 1e-13 * np.abs(dFo).max()
    psi, fail = D.solveAdjoint(dF)
    assert fail == 0
    TIn0 = case.bcs["inlet"]["T"][1]
    out = np.zeros(1)
    D.solverAD.calcJacTVecProduct("TIn", "patchVar", np.array([TIn0]), "residual", "residual", psi, out)
    total = 0.0 - out[0]  # dF/dTIn = dF/dTIn|W - psi^T dR/dTIn
    h = 1e-3
    vals = []
    for sgn in (1.0, -1.0):
        c = copy.copy(case)
        c.bcs = copy.deepcopy(case.bcs)
        c.bcs["inlet"]["T"] = (case.bcs["inlet"]["T"][0], TIn0 + sgn * h)
        vals.append(FR.variable_vol_sum(c, g, linear_primal(c, g, sc, con, col), TVOL))
    cd = (vals[0] - vals[1]) / (2 * h)
    assert cd != 0.0 and abs(total - cd) <= 1e-6 * abs(cd), (total, cd)


def newton_primal(case, g, beta, W0, sc, con, col, ref, rtol=1e-11):
    """Zero the oracle residual at betaFINuTilda = beta (oracle.primal's SIMPLE step ignores beta): Newton steps with the complex-step
    Jacobian, from W0, until |R| <= rtol ref (ref = |R| of the initial, unconverged field)."""
    import scipy.sparse.linalg as spla

    cb = copy.copy(case)
    cb.beta_fi = beta
    W = W0.copy()
    for _ in range(20):
        R = residual(cb, g, W)
        if np.linalg.norm(R) <= rtol * ref:
            return W
        A = J.jacobian_colored(cb, g, W, con, col, sc, mode="cs", lower_bound=0)  # A[j, i] = s_j dR_i/dW_j
        W = W + sc * spla.spsolve(A.T.tocsc(), -R)
    raise AssertionError(f"Newton did not converge: |R| = {np.linalg.norm(R):.3e}, reference {ref:.3e}")


def test_field_inversion_end_to_end():
    """Field inversion: a variance of U (field mode, boxToCell) against data from the primal at another beta, and the regulariser
    sum V beta^2; the adjoint totals dF/dbeta in two random directions against central differences of the Newton-converged oracle
    primal."""
    from oracle.primal import solve_primal

    case = channel_case(6, 5, 4, perturb=0.0)
    g = Geometry(case.mesh)
    N = g.nC
    sc = J.state_scales(case, g, norm_states(case))
    con = J.connectivity(case, g)
    col, _ = J.greedy_coloring(con)
    ref = np.linalg.norm(residual(case, g, case.states))
    W1, _ = solve_primal(case, g, max_iters=800, tol=1e-11)
    rng = np.random.default_rng(11)
    beta_d = 1.0 + 0.2 * rng.standard_normal(N)
    beta0 = 1.0 + 0.1 * rng.standard_normal(N)
    Wd = newton_primal(case, g, beta_d, W1, sc, con, col, ref)
    W0 = newton_primal(case, g, beta0, W1, sc, con, col, ref)
    Ud = FR.cell_values(case, g, Wd, "U")
    case.ref_data = {"UData": {"internal": Ud, "boundary": np.zeros((g.nBF, 3))}}
    case.states = W0
    fns = {
        "UVAR": {"type": "variance", "source": "boxToCell", "min": [0.2, -1.0, -1.0], "max": [0.8, 1.0, 1.0], "scale": 1.0, "mode": "field",
                 "varName": "U", "varType": "vector", "indices": [0, 1, 2], "useGeoWeight": 1, "timeDependentRefData": False},
        "BREG": {"type": "variableVolSum", "source": "allCells", "varName": "betaFINuTilda", "varType": "scalar", "index": 0, "isSquare": 1,
                 "scale": 1.0},
    }
    D = make(case, function=fns, inputInfo={"beta": {"type": "field", "fieldName": "betaFINuTilda", "fieldType": "scalar"}},
             adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    S = D.solverAD
    S.setSolverInput("beta", "field", N, beta0)
    Rl = np.zeros(W0.size)
    S.getResiduals(Rl)
    totals = {}
    for name in fns:
        dFdW = np.zeros(W0.size)
        S.calcJacTVecProduct("states", "stateVar", W0, name, "function", np.ones(1), dFdW)
        if name == "BREG":
            assert not dFdW.any()
            psi = np.zeros(W0.size)
        else:
            psi, fail = D.solveAdjoint(dFdW)
            assert fail == 0
        dFdb, pRb = np.zeros(N), np.zeros(N)
        S.calcJacTVecProduct("beta", "field", beta0, name, "function", np.ones(1), dFdb)
        S.calcJacTVecProduct("beta", "field", beta0, "residual", "residual", psi, pRb)
        totals[name] = dFdb - pRb
    h = 1e-4
    for _ in range(2):
        d = rng.standard_normal(N)
        vals = {name: [] for name in fns}
        for sgn in (1.0, -1.0):
            b = beta0 + sgn * h * d
            W = newton_primal(case, g, b, W0, sc, con, col, ref)
            vals["UVAR"].append(FR.variance(case, g, W, fns["UVAR"], case.ref_data))
            vals["BREG"].append(FR.variable_vol_sum(case, g, W, fns["BREG"], b))
        for name in fns:
            cd = (vals[name][0] - vals[name][1]) / (2 * h)
            assert cd != 0.0 and abs(totals[name] @ d - cd) <= 1e-5 * abs(cd), (name, totals[name] @ d, cd)


@pytest.mark.parametrize("solver", ["DATurboFoam", "DASimpleFoamT"])
def test_new_kinds_on_turbo_and_passive_T(solver):
    """The boundary-value kinds read T on DATurboFoam (MRF) and on DASimpleFoam with the passive T field (inletOutlet outlet)."""
    if solver == "DATurboFoam":
        case = turbo_channel_case(6, 5, 4, wall_function=True, perturb=0.02)
    else:
        case = simple_T_channel_case(6, 5, 4, wall_function=True, perturb=0.02)
    g = Geometry(case.mesh)
    with_ref_data(case, g)
    fns = {
        "TMean": {"type": "patchMean", "source": "patchToFace", "patches": ["outlet"], "varName": "T", "varType": "scalar", "index": 0, "scale": 1.0},
        "TBotMean": {"type": "patchMean", "source": "patchToFace", "patches": ["bottom"], "varName": "T", "varType": "scalar", "index": 0,
                     "scale": 1.0, "calcRefVar": 1, "ref": [290.0]},
        "TVolSum": {"type": "variableVolSum", "source": "allCells", "varName": "T", "varType": "scalar", "index": 0, "isSquare": 1, "scale": 1e-3},
        "UMean": UNIT_FUNCTIONS["UMean"],
        "UOutVar": UNIT_FUNCTIONS["UOutVar"],
    }
    D = make(case, function=fns)
    W = case.states
    sc = J.state_scales(case, g, norm_states(case))
    for name, fd in fns.items():
        Fo = restated(case, g, fd, W)
        F = D.solver.calcFunction(name)
        assert Fo != 0.0 and abs(F - Fo) <= 1e-12 * abs(Fo), (name, F, Fo)
        dFo = Fn.gradient(lambda Wp: restated(case, g, fd, Wp), W, sc)
        dF = np.zeros(W.size)
        D.solverAD.calcJacTVecProduct("states", "stateVar", W, name, "function", np.ones(1), dF)
        assert np.abs(dF - dFo).max() <= 1e-10 * np.abs(dFo).max(), name  # (TBotMean: fixedValue wall T, dF/dW = 0 exactly)


def test_cell_set_value_at_200k_cells_is_exact_and_repeatable():
    case = bench_channel_case(80, 50, 50)
    fd = {"type": "variableVolSum", "source": "allCells", "varName": "p", "varType": "scalar", "index": 0, "scale": 1.0}
    D = make(case, function={"PV": fd})
    geo = D.solver.geometry()
    N = case.mesh.n_cells
    assert N == 200000
    p = case.states[3 * N : 4 * N]
    exact = math.fsum((geo["V"] * p).tolist())
    F1, F2 = D.solver.calcFunction("PV"), D.solver.calcFunction("PV")
    assert F1 == F2
    assert abs(F1 - exact) <= 1e-13 * abs(exact)


def test_errors_name_the_problem(capsys):
    case = channel_case(4, 4, 3)
    base = dict(UNIT_FUNCTIONS["PVolSum"])
    cases = [
        (dict(base, varName="rho"), "varName rho"),
        (dict(base, varType="tensor"), "varType tensor"),
        (dict(base, source="boxToCell"), "min and max"),
        (dict(UNIT_FUNCTIONS["PVar"], mode="probePoint"), "probePoint"),
        (dict(UNIT_FUNCTIONS["PVar"], timeDependentRefData=True), "timeDependentRefData"),
        ({k: v for k, v in UNIT_FUNCTIONS["UOutVar"].items() if k != "indices"}, "indices"),
        (dict(UNIT_FUNCTIONS["PVar"], varName="wallShearStress"), "wallShearStress"),
    ]
    for fd, msg in cases:
        with pytest.raises(Exception, match=msg):
            make(case, function={"F": fd})
    with pytest.raises(NotImplementedError):
        make(case, function={"F": {"type": "fieldMax", "varName": "p"}})
    D = make(case, function={"PVar": UNIT_FUNCTIONS["PVar"]})  # no 0/pData: value 0 with the reference's warning
    assert "WARNING" in capsys.readouterr().out
    assert D.solver.calcFunction("PVar") == 0.0
    dF = np.zeros(case.states.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", case.states, "PVar", "function", np.ones(1), dF)
    assert np.all(dF == 0.0)

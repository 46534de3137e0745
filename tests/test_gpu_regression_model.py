"""The regression models (the regressionModel option and the regressionPar input of DASimpleFoam) on the device, through the C-ABI and the
Python classes: the residual with a model active, the assembled coloured dRdW^T against the dense forward-mode Jacobian, the parameter
product [dR/dtheta]^T psi, the kernels alone on caller data, the adjoint solution and an end-to-end total derivative - against the numpy
restatement of the reference's text (tests/regression_model_restatement.py) with the oracle's Gauss gradients and residual.
Bounds (tests/README_regression.md): values 1e-12, tangents, Jacobian entries and products 1e-10 relative to the largest entry,
finite-difference checks 1e-6, fixed-order sums against math.fsum 1e-13, determinism: np.array_equal over two calls."""
import functools
import math

import numpy as np
import pytest

import regression_model_restatement as RM
from dafoam_amd import _capi
from dafoam_amd._capi import dptr
from dafoam_amd.meshgen import channel_case
from mixed_mesh import mixed
from oracle import jacobian as J
from oracle.foam_mesh import Geometry
from oracle.residual import simple_residual

pytestmark = pytest.mark.gpu
NORM = {"U": 10.0, "p": 50.0, "nuTilda": 1e-3, "phi": 1.0}
NOBOUND = {"dRdW": 0.0, "dRdWPC": 0.0}
MESHES = ("channel", "mixed")


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    o = {"solverName": "DASimpleFoam", "normalizeStates": dict(NORM), "adjEqnOption": {"printInfo": 0}}
    o.update(extra)
    return PYDAFOAM(options=o, case=case)


def reg(**models):
    return dict(active=True, **models)


def inputs_of(*names):
    return {n: {"type": "regressionPar", "components": ["solver"]} for n in names}


@functools.lru_cache(maxsize=None)
def flow(mesh):
    """(case, geometry, stirred states): the 6 x 5 x 4 channel (120 cells) and the mixed mesh (148 cells) - neither a multiple of a tile;
    shared, read-only"""
    case = channel_case(6, 5, 4) if mesh == "channel" else mixed("simple")
    return case, Geometry(case.mesh), RM.stirred_states(case)


def solver_with(mesh, names, models=None, **extra):
    """a solver with the named models of RM.MODELS active, their parameters set and the stirred states loaded"""
    case, g, W = flow(mesh)
    models = models or {n: RM.MODELS[n] for n in names}
    D = make(case, regressionModel=reg(**models), inputInfo=inputs_of(*names), **extra)
    pars = {n: RM.parameters(models[n], seed=k) for k, n in enumerate(names)}
    for n in names:
        D.solver.setSolverInput(n, "regressionPar", pars[n].size, pars[n])
    D.solver.updateOFFields(W)
    return D, pars


def clip_bounds(mesh, name):
    """bounds that the raw output of the model crosses on some cells of the mesh, on each side, and not on others"""
    case, g, W = flow(mesh)
    model = RM.MODELS[name]
    U, nuT, gU, gP, y = RM.flow_inputs(case, g, W)
    raw = RM.raw_output(model, RM.parameters(model), RM.features(model, U, nuT, case.nu, gU, gP, y))
    return float(np.quantile(raw, 0.25)), float(np.quantile(raw, 0.7))


# ---- 1: the residual ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_residual_features_and_output_against_restatement_and_oracle(mesh):
    case, g, W = flow(mesh)
    names = ("nn534", "rbf7")
    D, pars = solver_with(mesh, names)
    U, nuT, gU, gP, y = RM.flow_inputs(case, g, W)
    for n in names:
        feat, out = D.solver.getRegressionFeatures(n)
        fref = RM.features(RM.MODELS[n], U, nuT, case.nu, gU, gP, y)
        bref, mref = RM.beta(RM.MODELS[n], pars[n], fref)
        info = D.regressionModelInfo(n)
        print(mesh, n, "features", np.abs(feat - fref).max(), "output", np.abs(out - bref).max(), "range", bref.min(), bref.max(), info)
        assert np.abs(feat - fref).max() <= 1e-12 and np.abs(out - bref).max() <= 1e-12 and np.ptp(bref) > 1e-3
        assert [info["nNaN"], info["nInf"], info["nBounded"]] == RM.fail_counts(mref) == [0, 0, 0] and info["fail"] == 0
    R = D.getResiduals()
    ref = RM.restated_residual(case, g, W, [(RM.MODELS[n], pars[n]) for n in names])
    first = RM.restated_residual(case, g, W, [(RM.MODELS["nn534"], pars["nn534"])])
    plain = simple_residual(case, g, W)
    print(mesh, "residual", rel(R, ref), "last model against first", rel(first, ref), "against no model", rel(plain, ref))
    assert rel(R, ref) <= 1e-12
    # the last model wins, and the model moves the residual by orders more than the bound
    assert rel(first, ref) > 1e-6 and rel(plain, ref) > 1e-6
    R2 = D.getResiduals()
    assert np.array_equal(R, R2)


def test_residual_with_clipped_cells_and_exact_fail_counts():
    case, g, W = flow("mixed")
    lo, hi = clip_bounds("mixed", "nn534")
    model = RM.clipped(RM.MODELS["nn534"], lo, hi)
    D, pars = solver_with("mixed", ("nn534",), models={"nn534": model})
    bref, mref = RM.restated_beta(case, g, W, [(model, pars["nn534"])])
    nClip = int((mref != 0).sum())
    assert 10 < nClip < g.nC - 10  # on the restatement: some cells clip, many do not
    info = D.regressionModelInfo("nn534")
    _, out = D.solver.getRegressionFeatures("nn534")
    assert [info["nNaN"], info["nInf"], info["nBounded"]] == [0, 0, nClip] and info["fail"] == 1
    assert np.abs(out - bref).max() <= 1e-12 and np.array_equal(out[mref != 0], bref[mref != 0])
    assert rel(D.getResiduals(), RM.restated_residual(case, g, W, [(model, pars["nn534"])])) <= 1e-12


# ---- 2, 3: the assembled operator against the dense forward-mode Jacobian -----------------------------------------------------------------
@pytest.mark.parametrize("mesh,name", [("channel", "nn3"), ("mixed", "nn3"), ("channel", "nn3_nop")])
def test_assembled_dRdWT_against_dense_forward_mode_jacobian(mesh, name):
    """nn3 has PSoSS among its inputs: without p at levels 0 and 1 of nuTildaRes the assembled rows miss entries the forward mode has"""
    from dafoam_amd.pyDASolvers import Mat

    case, g, W = flow(mesh)
    D, pars = solver_with(mesh, (name,), jacLowerBounds=NOBOUND)
    n, N = W.size, g.nC
    Jd = np.zeros((n, n))  # column j = dR/dW (s o e_j), one dual-number residual pass each
    e, col = np.zeros(n), np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        D.solver.calcJacVecProduct(e, col)
        Jd[:, j] = col
        e[j] = 0.0
    D.solver.runColoring()
    M = Mat()
    D.solver.calcdRdWT(0, M, mode=1)
    A = M.to_scipy().toarray()  # rows = states
    scale = np.abs(Jd).max()
    err = np.abs(A - Jd.T).max() / scale
    dn_dp = np.abs(Jd[4 * N:5 * N, 3 * N:4 * N])
    print(mesh, name, "assembled against forward mode", err, "largest d nuTildaRes / dp", dn_dp.max() / scale, "entries", int((dn_dp > 0).sum()))
    assert err <= 1e-10
    if name == "nn3":
        assert dn_dp.max() / scale > 1e-8 and (dn_dp > 0).sum() > 2 * N  # the block a missing p entry would drop is live
    else:
        assert dn_dp.max() == 0.0
        D0 = make(case, jacLowerBounds=NOBOUND)
        D0.solver.runColoring()
        assert np.array_equal(D.solver.getColoring()[0], D0.solver.getColoring()[0])  # no feature reads grad(p): the colours of before
    # forward-mode columns against central differences of restatement + oracle
    sc = J.state_scales(case, g, NORM)
    rng = np.random.default_rng(2)
    v = rng.standard_normal(n)
    models = [(RM.MODELS[name], pars[name])]
    h = 1e-6
    fd = (RM.restated_residual(case, g, W + h * sc * v, models) - RM.restated_residual(case, g, W - h * sc * v, models)) / (2 * h)
    fd0 = (simple_residual(case, g, W + h * sc * v) - simple_residual(case, g, W - h * sc * v)) / (2 * h)
    nT = slice(4 * N, 5 * N)  # the model acts on the nuTildaRes rows alone: there the check has to resolve its share by an order at least
    Jv = Jd @ v
    print(mesh, name, "J v against central differences", rel(Jv, fd), "on nuTildaRes", rel(Jv[nT], fd[nT]), "the model's share there", rel(fd0[nT], fd[nT]))
    assert rel(Jv, fd) <= 1e-6 and rel(Jv[nT], fd[nT]) <= 1e-6 and rel(fd0[nT], fd[nT]) > 1e-5
    assert np.array_equal(fd0[:4 * N], fd[:4 * N]) and np.array_equal(fd0[5 * N:], fd[5 * N:])
    # a . (J v) = (J^T a) . v through the two products
    a = rng.standard_normal(n)
    Jv, JTa = np.zeros(n), np.zeros(n)
    D.solver.calcJacVecProduct(v, Jv)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "residuals", "residual", a, JTa)
    lhs, rhs = float(a @ Jv), float(JTa @ v)
    print(mesh, name, "a.(Jv)", lhs, "(J^T a).v", rhs)
    assert abs(lhs - rhs) <= 1e-10 * max(np.abs(a * Jv).max(), np.abs(JTa * v).max()) * math.sqrt(n)
    JTa2 = np.zeros(n)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "residuals", "residual", a, JTa2)
    assert np.array_equal(JTa, JTa2)


# ---- 4, 5: [dR/dtheta]^T psi ---------------------------------------------------------------------------------------------------------------
def dR_dbeta(case, g, W, beta):
    """d R / d beta_c: the residual is linear in betaFINuTilda, and row nuTildaRes_c alone reads beta_c"""
    import copy

    c1, c0 = copy.copy(case), copy.copy(case)
    c1.beta_fi, c0.beta_fi = beta + 1.0, beta
    d = simple_residual(c1, g, W) - simple_residual(c0, g, W)
    N = g.nC
    assert not d[:4 * N].any() and not d[5 * N:].any()
    return d[4 * N:5 * N]


@pytest.mark.parametrize("clip", [False, True], ids=["free", "clipped"])
@pytest.mark.parametrize("mesh", MESHES)
def test_parameter_product_of_the_3_network_against_the_restatement(mesh, clip):
    """psi . dR/dtheta_k = sum_c psi_c (dR_c / dbeta_c) dbeta_c / dtheta_k: the first factor from the oracle (exactly linear in beta), the
    second from central differences of the restatement in longdouble"""
    case, g, W = flow(mesh)
    model = RM.clipped(RM.MODELS["nn3"], *clip_bounds(mesh, "nn3")) if clip else RM.MODELS["nn3"]
    D, pars = solver_with(mesh, ("nn3",), models={"nn3": model})
    p = pars["nn3"]
    N = g.nC
    psi = np.random.default_rng(8).standard_normal(W.size)
    prod, prod2 = np.zeros(p.size), np.zeros(p.size)
    D.solverAD.calcJacTVecProduct("nn3", "regressionPar", p, "residuals", "residual", psi, prod)
    D.solverAD.calcJacTVecProduct("nn3", "regressionPar", p, "residuals", "residual", psi, prod2)
    U, nuT, gU, gP, y = RM.flow_inputs(case, g, W)
    feat = RM.features(model, U, nuT, case.nu, gU, gP, y)
    b, mask = RM.beta(model, p, feat)
    ref = RM.dbeta_dpar_fd(model, p, feat, psi[4 * N:5 * N] * dR_dbeta(case, g, W, b))
    print(mesh, "clipped cells", int((mask != 0).sum()), "product", prod, "err", rel(prod, ref))
    assert (0 < (mask != 0).sum() < N - 10) if clip else not mask.any()
    assert rel(prod, ref) <= 1e-10 and np.abs(ref).min() > 1e-6 * np.abs(ref).max()
    assert np.array_equal(prod, prod2)


@pytest.mark.parametrize("clip", [False, True], ids=["free", "clipped"])
def test_parameter_product_of_the_20_20_network_against_central_differences_of_the_device_residual(clip):
    """541 parameters: more than a workgroup of the backward kernel has threads; 120 cells: two tiles, the second partial"""
    mesh = "channel"
    case, g, W = flow(mesh)
    model = RM.clipped(RM.MODELS["nn2020"], *clip_bounds(mesh, "nn2020")) if clip else RM.MODELS["nn2020"]
    D, pars = solver_with(mesh, ("nn2020",), models={"nn2020": model})
    p = pars["nn2020"]
    assert p.size == 541
    psi = np.random.default_rng(9).standard_normal(W.size)
    prod = np.zeros(p.size)
    D.solverAD.calcJacTVecProduct("nn2020", "regressionPar", p, "residuals", "residual", psi, prod)
    info = D.regressionModelInfo("nn2020")
    assert (10 < info["nBounded"] < g.nC - 10) if clip else info["nBounded"] == 0
    fd = np.zeros(p.size)
    for k in range(p.size):
        h = 1e-5 * max(abs(p[k]), 1e-2)
        q = p.copy()
        q[k] = p[k] + h
        D.solver.setSolverInput("nn2020", "regressionPar", q.size, q)
        Rp = D.getResiduals()
        q[k] = p[k] - h
        D.solver.setSolverInput("nn2020", "regressionPar", q.size, q)
        fd[k] = psi @ (Rp - D.getResiduals()) / (2 * h)
    print("clipped cells", info["nBounded"], "err", rel(prod, fd), "largest", np.abs(fd).max())
    assert rel(prod, fd) <= 1e-6


def test_products_to_functions_and_a_model_that_is_overwritten_are_exact_zeros():
    case, g, W = flow("channel")
    fn = {"CD": {"type": "force", "source": "patchToFace", "patches": ["bottom", "top"], "directionMode": "fixedDirection", "direction": [1.0, 0.0, 0.0],
                 "scale": 2.0}}
    D, pars = solver_with("channel", ("nn3", "rbf1"), function=fn)
    out = np.ones(pars["nn3"].size)
    D.solverAD.calcJacTVecProduct("nn3", "regressionPar", pars["nn3"], "CD", "function", np.ones(1), out)
    assert not out.any()
    out[:] = 1.0
    D.solverAD.calcJacTVecProduct("nn3", "regressionPar", pars["nn3"], "residuals", "residual", np.ones(W.size), out)
    assert not out.any()  # rbf1, defined later, overwrites betaFINuTilda
    last = np.zeros(pars["rbf1"].size)
    D.solverAD.calcJacTVecProduct("rbf1", "regressionPar", pars["rbf1"], "residuals", "residual", np.ones(W.size), last)
    assert np.abs(last).min() > 0
    with pytest.raises(_capi.DASError, match="NOPE"):
        D.solverAD.calcJacTVecProduct("nn3", "regressionPar", pars["nn3"], "NOPE", "function", np.ones(1), out)


# ---- 6: the kernels alone ----------------------------------------------------------------------------------------------------------------
def debug_pair(model, par, feat, g):
    L = _capi.lib()
    sp = _capi.reg_spec(dict(model, nInputs=feat.shape[1]), with_names=False)
    n = feat.shape[0]
    b, m, out = np.zeros(n), np.zeros(n, dtype=np.uint8), np.zeros(par.size)
    import ctypes as C

    f = np.ascontiguousarray(feat)
    _capi.check(L.das_debug_reg_forward(C.byref(sp), dptr(par), par.size, n, dptr(f), dptr(b), m.ctypes.data_as(C.POINTER(C.c_ubyte))))
    _capi.check(L.das_debug_reg_backward(C.byref(sp), dptr(par), par.size, n, dptr(f), dptr(np.ascontiguousarray(g)), dptr(out)))
    return b, m.astype(np.int64), out


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_debug_pair_network_at_the_tile_edges(n):
    model = RM.clipped(RM.MODELS["nn534"], 0.8, 1.3)
    par = RM.parameters(model)
    rng = np.random.default_rng(n)
    feat, g = rng.random((n, 5)), rng.standard_normal(n)
    ref, mask = RM.beta(model, par, feat)
    b, m, out = debug_pair(model, par, feat, g * (mask == 0))
    b2, m2, out2 = debug_pair(model, par, feat, g * (mask == 0))
    fd = RM.dbeta_dpar_fd(model, par, feat, g)
    bias = math.fsum(g * (mask == 0)) * model["outputScale"]  # the output neuron's bias: d beta / d b = outputScale
    print(n, "cells, clipped", int((mask != 0).sum()), "beta", np.abs(b - ref).max(), "backward", rel(out, fd), "bias entry", out[-1], bias)
    assert np.abs(b - ref).max() <= 1e-12 and np.array_equal(m, mask)
    assert rel(out, fd) <= 1e-6 and abs(out[-1] - bias) <= 1e-13 * max(np.abs(g).sum(), 1e-300)
    assert np.array_equal(b, b2) and np.array_equal(out, out2)


def test_debug_pair_rbf_at_20001_cells_against_fsum():
    """313 tiles over 128 workgroups: every workgroup walks several tiles, the last tile holds 33 cells.  The per-cell terms of the one-RBF
    model in closed form, summed by math.fsum."""
    model = RM.MODELS["rbf1"]
    par = RM.parameters(model)
    n, nIn = 20001, 3
    rng = np.random.default_rng(20001)
    feat, g = rng.random((n, nIn)), rng.standard_normal(n)
    m_, s_, w = par[0:6:2], par[1:6:2], par[6]
    e = np.exp(-(((feat - m_) ** 2) / (2 * s_ * s_)).sum(1))
    ref_b = model["outputScale"] * (w * e + model["outputShift"])
    b, mask, out = debug_pair(model, par, feat, g)
    assert not mask.any() and np.abs(b - ref_b).max() <= 1e-12
    go = g * model["outputScale"]
    terms = [go * w * e * (feat[:, j] - m_[j]) ** q / s_[j] ** (q + 1) for j in range(nIn) for q in (1, 2)] + [go * e]
    for k, t in enumerate(terms):
        ref = math.fsum(t)
        print("parameter", k, out[k], ref, "relative to the sum of magnitudes", abs(out[k] - ref) / np.abs(t).sum())
        assert abs(out[k] - ref) <= 1e-13 * np.abs(t).sum()
    assert np.array_equal(out, debug_pair(model, par, feat, g)[2])


# ---- 7, 12: the adjoint --------------------------------------------------------------------------------------------------------------------
def test_adjoint_solution_with_a_model_against_a_dense_direct_solve():
    from dafoam_amd.pyDASolvers import Mat

    case, g, W = flow("channel")
    D, pars = solver_with("channel", ("nn3",), jacLowerBounds=NOBOUND, adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    rhs = np.random.default_rng(4).standard_normal(W.size)
    psi, fail = D.solveAdjoint(rhs)
    psi2, _ = D.solveAdjoint(rhs)
    M = Mat()
    D.solver.calcdRdWT(0, M, mode=1)
    ref = np.linalg.solve(M.to_scipy().toarray(), rhs)
    print("psi against the dense solve", rel(psi, ref))
    assert fail == 0 and rel(psi, ref) <= 1e-6
    assert np.array_equal(psi, psi2)


def test_inactive_option_is_bitwise_the_run_that_never_mentions_it():
    from dafoam_amd.pyDASolvers import Mat

    case, g, W = flow("channel")
    rhs = np.random.default_rng(6).standard_normal(W.size)
    got = []
    for extra in ({}, {"regressionModel": dict(active=False, m=RM.MODELS["nn3"])}):
        D = make(case, jacLowerBounds=NOBOUND, adjEqnOption={"gmresRelTol": 1e-10, "printInfo": 0}, **extra)
        D.solver.updateOFFields(W)
        psi, fail = D.solveAdjoint(rhs)
        M = Mat()
        D.solver.calcdRdWT(0, M, mode=1)
        A = M.to_scipy().tocsr()
        A.sort_indices()
        got.append((D.solver.getColoring()[0], A.indptr, A.indices, A.data, psi, D.getResiduals()))
        assert fail == 0
    for a, b in zip(*got):
        assert np.array_equal(a, b)


# ---- the other inputs pick the model up through the residual passes ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walled():
    """the 6 x 5 x 4 channel with walls at front and back (a point of a symmetry plane moved in z is treated differently by the volCoord
    product and by the oracle without any model: tests/actuator_disk_cases.py), stirred states, and nn3 - PoD reads the wall distance, PSoSS
    grad(p)"""
    case = channel_case(6, 5, 4, side_walls=True)
    return case, Geometry(case.mesh), RM.stirred_states(case), RM.MODELS["nn3"], RM.parameters(RM.MODELS["nn3"])


def walled_solver(with_model=True, **extra):
    case, g, W, model, p = walled()
    inputs = {"x": {"type": "volCoord"}, "UIn": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"},
              "UVec": {"type": "patchVar", "patches": ["inlet"], "varName": "U", "varType": "vector"},
              "nuIn": {"type": "patchVar", "patches": ["inlet"], "varName": "nuTilda", "varType": "scalar"}}
    if with_model:
        D = make(case, regressionModel=reg(nn3=model), inputInfo=dict(inputs, **inputs_of("nn3")), **extra)
        D.solver.setSolverInput("nn3", "regressionPar", p.size, p)
    else:
        D = make(case, inputInfo=inputs, **extra)
    D.solver.updateOFFields(W)
    return D


def volcoord_reference(psi, idx, with_model=True):
    """psi . dR/dX_j by central differences of restatement + oracle on the moved mesh (the wall distance stays, as in the library)"""
    import actuator_disk_restatement as AD

    case, g, W, model, p = walled()
    X0 = case.mesh.points.ravel()
    out = []
    for j in idx:
        h = 1e-7
        vals = []
        for sgn in (1.0, -1.0):
            X = X0.copy()
            X[j] += sgn * h
            gg = AD.FlowGeom(case.mesh, X.reshape(-1, 3))
            vals.append(psi @ (RM.restated_residual(case, gg, W, [(model, p)]) if with_model else simple_residual(case, gg, W)))
        out.append((vals[0] - vals[1]) / (2 * h))
    return np.array(out)


def sample_point_dofs(case):
    m = case.mesh
    boundary = set(int(q) for f in range(m.n_internal_faces, m.n_faces) for q in m.face_pts[m.face_ptr[f]:m.face_ptr[f + 1]])
    inner = [q for q in range(m.n_points) if q not in boundary]
    by = {pp.name: pp for pp in m.patches}
    wall = int(m.face_pts[m.face_ptr[by["bottom"].start + 5]])
    pts = [inner[0], inner[len(inner) // 2], inner[-1], wall]
    return [3 * q + k for q in pts for k in range(3)]


def volcoord_seeds(which):
    """full: on every row (there the model moves the product by 2e-6 of its largest entry only: the momentum rows of the wall points
    dominate); nuTilda: on the nuTildaRes rows alone, the rows the model acts on"""
    case, g, W, model, p = walled()
    psi = np.random.default_rng(21).standard_normal(W.size)
    if which == "nuTilda":
        psi[:4 * g.nC] = 0.0
        psi[5 * g.nC:] = 0.0
    return psi


@pytest.mark.parametrize("which", ["full", "nuTilda"])
def test_vol_coord_product_with_a_model_exact_mode(which):
    """the dual-metrics pass: k_reg_forward<Dual<1>, Dual<1>> - the wall distance of PoD carries no tangent (it is frozen), the gradients do"""
    case, g, W, model, p = walled()
    psi = volcoord_seeds(which)
    idx = sample_point_dofs(case)
    ref, ref0 = volcoord_reference(psi, idx), volcoord_reference(psi, idx, with_model=False)
    X0 = case.mesh.points.ravel().copy()
    prod, prod2, prod0 = np.zeros(X0.size), np.ones(X0.size), np.zeros(X0.size)
    D = walled_solver()
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod2)
    walled_solver(with_model=False).solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod0)
    scale = np.abs(prod).max()
    print("volCoord exact", which, ": err", np.abs(prod[idx] - ref).max() / scale, "the model's share", np.abs(ref - ref0).max() / scale, "product moved",
          np.abs(prod - prod0).max() / scale)
    assert np.abs(prod[idx] - ref).max() <= 1e-6 * scale and np.array_equal(prod, prod2)
    assert not np.array_equal(prod, prod0)
    if which == "nuTilda":  # on its own rows the model's share is orders above the bound: a pass without the model cannot meet it
        assert np.abs(ref - ref0).max() > 1e-3 * scale and np.abs(prod - prod0).max() > 1e-3 * scale


@pytest.mark.parametrize("which", ["full", "nuTilda"])
def test_vol_coord_product_with_a_model_difference_mode(which):
    """amd.volCoordMode fd: the mode differences the device residual itself.  It meets the 1e-6 of the finite-difference checks with both
    seeds (measured 4.3e-9 and 4.4e-10); on the nuTildaRes rows the model's share (0.41 of the largest entry) is asserted to be orders above"""
    case, g, W, model, p = walled()
    psi = volcoord_seeds(which)
    idx = sample_point_dofs(case)
    ref = volcoord_reference(psi, idx)
    X0 = case.mesh.points.ravel().copy()
    prod, prod0 = np.zeros(X0.size), np.zeros(X0.size)
    walled_solver(amd={"volCoordMode": "fd"}).solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod)
    walled_solver(with_model=False, amd={"volCoordMode": "fd"}).solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod0)
    err = np.abs(prod[idx] - ref) / np.abs(prod).max()
    print("volCoord fd", which, ": 95 %", np.percentile(err, 95), "max", err.max(), "product moved", np.abs(prod - prod0).max() / np.abs(prod).max())
    assert not np.array_equal(prod, prod0)
    assert err.max() <= 1e-6
    if which == "nuTilda":
        assert np.abs(prod - prod0).max() > 1e-3 * np.abs(prod).max()


def test_patch_velocity_and_patch_var_products_with_a_model():
    import copy

    case, g, W, model, p = walled()
    psi = np.random.default_rng(22).standard_normal(W.size)
    U0 = np.array(case.bcs["inlet"]["U"][1], dtype=float)
    n0 = float(case.bcs["inlet"]["nuTilda"][1])

    def restated(field, value, with_model=True):
        c = copy.copy(case)
        c.bcs = copy.deepcopy(case.bcs)
        c.bcs["inlet"][field] = (case.bcs["inlet"][field][0], value)
        return psi @ (RM.restated_residual(c, g, W, [(model, p)]) if with_model else simple_residual(c, g, W))

    def central(fun, x0, h):
        out = []
        for k in range(len(x0)):
            e = np.zeros(len(x0))
            e[k] = h[k]
            out.append((fun(x0 + e) - fun(x0 - e)) / (2 * h[k]))
        return np.array(out)

    def u_of(x):  # [UMag, AoA(deg)] -> the inlet vector: flow axis x, normal axis y
        a = x[1] * np.pi / 180.0
        return (x[0] * np.cos(a), x[0] * np.sin(a), U0[2])

    x_pv = np.array([float(np.hypot(U0[0], U0[1])), float(np.degrees(np.arctan2(U0[1], U0[0])))])
    cases = {
        "UIn": ("patchVelocity", x_pv, [1e-5, 1e-4], lambda x, m=True: restated("U", u_of(x), m)),
        "UVec": ("patchVar", U0.copy(), [1e-5] * 3, lambda x, m=True: restated("U", tuple(x), m)),
        "nuIn": ("patchVar", np.array([n0]), [1e-9], lambda x, m=True: restated("nuTilda", float(x[0]), m)),
    }
    D, D0 = walled_solver(), walled_solver(with_model=False)
    for name, (kind, x0, h, fun) in cases.items():
        ref, ref0 = central(fun, x0, h), central(lambda x: fun(x, False), x0, h)
        prod, prod2, prod0 = np.zeros(x0.size), np.ones(x0.size), np.zeros(x0.size)
        D.solverAD.calcJacTVecProduct(name, kind, x0, "residuals", "residual", psi, prod)
        D.solverAD.calcJacTVecProduct(name, kind, x0, "residuals", "residual", psi, prod2)
        D0.solverAD.calcJacTVecProduct(name, kind, x0, "residuals", "residual", psi, prod0)
        print(name, kind, "product", prod, "reference", ref, "without a model", prod0, "err", rel(prod, ref), "the model's share", rel(ref0, ref))
        assert rel(prod, ref) <= 1e-6 and np.array_equal(prod, prod2) and rel(prod0, ref0) <= 1e-6
        if name == "nuIn":
            # no feature reads a boundary value of nuTilda, and the production term is the only place beta enters: the derivative in the
            # inlet value is the one without a model (the two references differ by their own rounding, 2e-7)
            assert rel(prod, prod0) <= 1e-12
        else:
            assert rel(prod, prod0) > 1e-8


# ---- replaced cells in the reverse pass, and the models at the caps --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nn534", "rbf7"])
def test_debug_pair_with_a_nan_and_an_inf_cell_among_good_ones(name):
    """a cell whose output checkOutput replaced contributes exactly nothing: its g is zero and the reverse pass does not evaluate it"""
    model = dict(RM.MODELS[name], defaultOutputValue=0.75)
    par = RM.parameters(model)
    rng = np.random.default_rng(5)
    n, nIn = 70, len(model["inputNames"])
    feat, g = rng.random((n, nIn)), rng.standard_normal(n)
    # (an infinite feature leaves the output of a radial basis function finite - exp(-inf) = 0 - and the cell in place: NaN for both there;
    #  in the network the infinite feature turns into inf - inf = NaN on the way)
    feat[3, 1], feat[66, 0] = np.nan, (np.inf if name == "nn534" else np.nan)
    ref, mask = RM.beta(model, par, feat)
    b, m, out = debug_pair(model, par, feat, g * (mask == 0))
    good = mask == 0
    _, _, out_good = debug_pair(model, par, feat[good], g[good])
    print(name, "mask of the two cells", mask[3], mask[66], "beta there", b[3], b[66], "backward against the good cells alone", rel(out, out_good))
    assert np.array_equal(m, mask) and mask[3] != 0 and mask[66] != 0 and b[3] == 0.75 and b[66] == 0.75 and int((mask != 0).sum()) == 2
    assert np.isfinite(out).all() and rel(out, out_good) <= 1e-12 and np.abs(out_good).min() > 0


@pytest.mark.parametrize("which", ["wide", "deep", "rbf"])
def test_debug_pair_of_the_models_at_the_caps(which):
    """[32] x 4 with 8 inputs (3489 parameters), 6 layers, 64 RBFs with 8 inputs: the kernels with more than 64 KB of LDS, at 300 cells"""
    eight = dict(inputNames=["VoS"] * 8, inputShift=[0.0] * 8, inputScale=[1.0] * 8)
    model = {"wide": dict(RM.MODELS["nn3"], hiddenLayerNeurons=[32] * 4, activationFunction="tanh", **eight),
             "deep": dict(RM.MODELS["nn3"], hiddenLayerNeurons=[32, 32, 32, 20, 20, 8], activationFunction="sigmoid", **eight),
             "rbf": dict(RM.MODELS["rbf7"], nRBFs=64, **eight)}[which]
    par = RM.parameters(model, amp=0.3)
    rng = np.random.default_rng(6)
    n = 300
    feat, g = rng.random((n, 8)), rng.standard_normal(n)
    ref, mask = RM.beta(model, par, feat)
    b, m, out = debug_pair(model, par, feat, g)
    some = rng.choice(par.size, 6, replace=False)
    fd = np.array([RM.dbeta_dpar_fd(dict(model), par, feat[:20], g[:20], only=k) for k in some])
    _, _, out40 = debug_pair(model, par, feat[:20], g[:20])
    print(which, par.size, "parameters, beta", np.abs(b - ref).max(), "backward (6 parameters, 20 cells)", np.abs(out40[some] - fd).max() / np.abs(out40).max())
    assert not mask.any() and np.abs(b - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.abs(out40[some] - fd).max() <= 1e-6 * np.abs(out40).max() and np.isfinite(out).all()


# ---- 8: end to end -----------------------------------------------------------------------------------------------------------------------------
# noise floor of the CPU differences per parameter (see the docstring below) and the bar, ten times the floor
E2E_FLOOR = {0: 1.2e-12, 7: 6.4e-12, 18: 3.3e-12}


def test_total_derivative_of_the_drag_in_three_parameters_against_the_reconverged_primal():
    """dCD/dtheta_k = - psi^T dR/dtheta_k (device: Newton primal, solveAdjoint at gmresRelTol 1e-12, the regressionPar product) against central
    differences of the CPU primal of restatement + oracle re-converged at theta +- h (RM.CpuPrimal), h = 1e-4 max(|theta_k|, 1e-2).
    The CPU side was run first, at four steps (central differences):
      parameter 0   1e-2 -7.503692958e-06   1e-3 -7.503697133e-06   1e-4 -7.503696569e-06   1e-5 -7.503697691e-06
      parameter 7   1e-2 -2.353010282e-05   1e-3 -2.353009781e-05   1e-4 -2.353009714e-05   1e-5 -2.353010351e-05
      parameter 18  1e-2 -3.593104976e-04   1e-3 -3.592891044e-04   1e-4 -3.592888914e-04   1e-5 -3.592888882e-04
    Its noise floor is the scatter of the central difference between the steps 1e-4 and 1e-5 (for parameter 18 the truncation error is
    still 2e-10 at 1e-3 and gone at 1e-4): 1.2e-12, 6.4e-12 and 3.3e-12, i.e. 1.5e-7, 2.7e-7 and 9e-9 of the values.  The bar is that
    floor times ten, fixed in E2E_FLOOR.  Measured on an MI355X: adjoint totals -7.503697217e-06, -2.353009779e-05, -3.592888883e-04.
    The device primal starts in the Newton limit (amd.primalTau0 1e6; tests/README_regression.md says why)."""
    from oracle.functions import force

    case = channel_case(6, 5, 4, perturb=0.0)
    g = Geometry(case.mesh)
    fn = {"CD": {"type": "force", "source": "patchToFace", "patches": ["bottom", "top"], "directionMode": "fixedDirection", "direction": [1.0, 0.0, 0.0],
                 "scale": 2.0}}
    model = RM.MODELS["nn3"]
    p0 = RM.parameters(model)
    cpu = RM.CpuPrimal(case, g, model, p0, NORM)
    cd_of = lambda W: force(case, g, W, ["bottom", "top"], [1, 0, 0], 2.0)
    D = make(case, regressionModel=reg(nn3=model), inputInfo=inputs_of("nn3"), function=fn, adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0},
             amd={"primalTau0": 1.0e6})
    R0 = np.zeros(case.states.size)
    D.solver.getResiduals(R0)
    D.solver.setSolverInput("nn3", "regressionPar", p0.size, p0)
    fail, info = D.solver.solvePrimal(maxSteps=80, relTol=0.0, absTol=1e-12 * np.linalg.norm(R0))
    assert fail == 0, info
    W = D.getStates()
    f_dev, f_cpu = D.solver.calcFunction("CD"), cd_of(cpu.W0)
    print("CD device", f_dev, "CPU primal", f_cpu, "states", rel(W, cpu.W0))
    assert abs(f_dev - f_cpu) <= 1e-10 * abs(f_cpu)
    rhs = np.zeros(W.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "CD", "function", np.ones(1), rhs)
    psi, fail = D.solveAdjoint(rhs)
    prod = np.zeros(p0.size)
    D.solverAD.calcJacTVecProduct("nn3", "regressionPar", p0, "residuals", "residual", psi, prod)
    assert fail == 0
    for k, floor in E2E_FLOOR.items():
        dp = np.zeros(p0.size)
        dp[k] = 1e-4 * max(abs(p0[k]), 1e-2)
        fd = (cd_of(cpu.solve(p0 + dp)) - cd_of(cpu.solve(p0 - dp))) / (2 * dp[k])
        total = -prod[k]
        print("parameter", k, "adjoint total", total, "central differences of the CPU primal", fd, "bar", 10 * floor, "difference", abs(total - fd))
        assert fd != 0 and abs(total - fd) <= 10 * floor

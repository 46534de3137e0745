"""DASolidDisplacementFoam on the device: residual, Jacobians, products, colouring, the volCoord product of the residual, the objectives
vonMisesStressKS and variableVolSum (of D and of solid:rho) with their products, the adjoint, the Newton primal and a total derivative - against the numpy restatement (tests/solid_displacement_restatement.py) and its complex step.
Bars (those of tests/README_heat_transfer.md): 1e-12 relative for values, 1e-10 for derivative entries and products, 1e-4 for the
finite-difference dRdWTPC against exact entries, 1e-6 for an adjoint vector against an independent one."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import solid_displacement_restatement as S
from dafoam_amd._capi import DASError
from dafoam_amd.meshgen import solid_displacement_case
from solid_displacement_cases import KS_BOX, KS_COEFF, KS_SCALE, MATERIALS, MESHES, NORM, PASSES, solid_case, solid_functions, solid_options

pytestmark = pytest.mark.gpu

SC = NORM["D"]  # the state scale of every unknown


def make(case, passes=2, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=solid_options(passes, **extra), case=case)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def restated(mesh, material, passes):
    """(case, geometry, residual, D_s dRdW^T by the complex step) - computed once, shared, read-only"""
    case = solid_case(mesh, material)
    g = S.Geom(case.mesh)
    return case, g, S.residual(case, g, case.states, passes), sp.csr_matrix((S.jacobian(case, g, case.states, passes) * SC).T)


@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("material", sorted(MATERIALS))
@pytest.mark.parametrize("mesh", MESHES)
def test_residual(mesh, material, passes):
    case = solid_case(mesh, material)
    g = S.Geom(case.mesh)
    Ro = S.residual(case, g, case.states, passes)
    Sv = make(case, passes).solver
    n = case.states.size
    R, R2, Rp = np.zeros(n), np.ones(n), np.zeros(n)
    Sv.getResiduals(R)
    Sv.getResiduals(R2)
    print(mesh, material, passes, "residual", rel(R, Ro))
    assert np.array_equal(R, R2) and rel(R, Ro) <= 1e-12
    Sv.calcResiduals(1, Rp)
    assert np.array_equal(R, Rp)  # no PC variant of this residual


def test_residual_not_normalised_and_pass_count_is_read_at_residual_time():
    case = solid_case("mixed", "strain")
    g = S.Geom(case.mesh)
    D = make(case, 2, normalizeResiduals=["URes", "pRes"])
    R = np.zeros(case.states.size)
    D.solver.getResiduals(R)
    assert rel(R, S.residual(case, g, case.states, 2, normalized=False)) <= 1e-12
    D.solver.updateDAOption({"maxCorrectBCCalls": 20})
    D.solver.getResiduals(R)
    assert rel(R, S.residual(case, g, case.states, 20, normalized=False)) <= 1e-12


@pytest.mark.parametrize("mesh,material,passes", [("bump", "strain", 2), ("bump", "stress", 20), ("mixed", "strain", 20), ("mixed_renumbered", "strain", 2)])
def test_jacobians(mesh, material, passes):
    from dafoam_amd.pyDASolvers import Mat

    case, g, _, A = restated(mesh, material, passes)
    D = make(case, passes, jacLowerBounds={"dRdW": 0.0, "dRdWPC": 0.0})
    D.solver.runColoring()
    M = Mat()
    D.solver.calcdRdWT(0, M, mode=1)
    e = np.abs((M.to_scipy() - A).toarray()).max() / np.abs(A.data).max()
    Mp = Mat()
    D.solver.calcdRdWT(1, Mp)  # the reference's coloured finite differences
    efd = np.abs((Mp.to_scipy() - A).toarray()).max() / np.abs(A.data).max()
    print(mesh, material, passes, "dual", e, "FD", efd)
    assert e <= 1e-10 and efd <= 1e-4


@pytest.mark.parametrize("mesh,material,passes", [("bump", "strain", 2), ("mixed", "strain", 20)])
def test_products_and_dot_product_identity(mesh, material, passes):
    case, g, _, A = restated(mesh, material, passes)
    D = make(case, passes)
    n = case.states.size
    rng = np.random.default_rng(5)
    psi, v = rng.standard_normal(n), rng.standard_normal(n)
    prod, Jv = np.zeros(n), np.zeros(n)
    D.solverAD.calcJacTVecProduct("states", "stateVar", case.states, "residuals", "residual", psi, prod)
    D.solverAD.calcJacVecProduct(v, Jv)
    ref = np.imag(S.residual(case, g, case.states + 1e-30j * SC * v, passes)) / 1e-30
    print(mesh, material, passes, rel(prod, A @ psi), rel(Jv, ref))
    assert rel(prod, A @ psi) <= 1e-10 and rel(Jv, ref) <= 1e-10
    assert abs(psi @ Jv - prod @ v) <= 1e-10 * np.abs(psi * Jv).sum()


@pytest.mark.parametrize("mesh", ["bump432", "mixed_renumbered"])
def test_device_colouring_is_the_host_first_fit(mesh):
    case = solid_case(mesh, "strain")
    Dd, Dh = make(case), make(case, amd={"coloringOnDevice": 0})
    Dd.solver.runColoring()
    Dh.solver.runColoring()
    (cd, nd), (ch, nh) = Dd.solver.getColoring(), Dh.solver.getColoring()
    assert nd == nh and np.array_equal(cd, ch)


def sample_points(case):
    """an interior point, a corner, points of the two traction patches and of the fixed patch, and (mixed mesh) the apex of a pyramid"""
    m = case.mesh
    by = {p.name: p for p in m.patches}
    pts = {3 + 7 * (2 + 6 * 2), 0, int(m.face_pts[m.face_ptr[by["outlet"].start + 5]]), int(m.face_pts[m.face_ptr[by["top"].start + 3] + 1]),
           int(m.face_pts[m.face_ptr[by["inlet"].start + 2]])}
    if m.n_points > 210:
        pts.add(210)
    return sorted(pts)


@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_volcoord_product_of_the_residual(mesh):
    case, g, _, _ = restated(mesh, "strain", 2)
    D = make(case, 2, inputInfo={"x": {"type": "volCoord"}})
    n = case.states.size
    rng = np.random.default_rng(9)
    psi = rng.standard_normal(n)
    X0 = case.mesh.points.ravel().copy()
    prod = np.zeros(X0.size)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod)
    idx = [3 * p + k for p in sample_points(case) for k in range(3)]
    ref = []
    for j in idx:
        X = X0.astype(np.complex128)
        X[j] += 1e-30j
        ref.append(psi @ np.imag(S.residual(case, S.Geom(case.mesh, X.reshape(-1, 3)), case.states, 2)) / 1e-30)
    ref = np.array(ref)
    print(mesh, "volCoord", np.abs(prod[idx] - ref).max() / np.abs(prod).max())
    assert np.abs(ref).max() > 0 and np.abs(prod[idx] - ref).max() <= 1e-10 * np.abs(prod).max()


def test_variable_vol_sum_of_D():
    case, g, _, _ = restated("mixed", "strain", 2)
    fn = {"DY": {"type": "variableVolSum", "source": "allCells", "varName": "D", "varType": "vector", "index": 1, "isSquare": 0, "multiplyVol": 1,
                 "divByTotalVol": 0, "scale": 3.0}}
    Sv = make(case, 2, function=fn).solverAD
    ref = 3.0 * (g.V * case.states.reshape(-1, 3)[:, 1]).sum()
    v1, v2 = Sv.calcFunction("DY"), Sv.calcFunction("DY")
    assert v1 == v2 and abs(v1 - ref) <= 1e-12 * abs(ref)
    dF = np.zeros(case.states.size)
    Sv.calcJacTVecProduct("states", "stateVar", case.states, "DY", "function", np.ones(1), dF)
    exp = np.zeros((g.nC, 3))
    exp[:, 1] = 3.0 * g.V * SC
    assert rel(dF, exp.ravel()) <= 1e-10


def test_other_functions_and_outputs_are_refused_by_name():
    case = solid_case("bump", "strain")
    with pytest.raises(DASError, match="DASolidDisplacementFoam"):
        make(case, function={"F": {"type": "force", "source": "patchToFace", "patches": ["top"], "directionMode": "fixedDirection",
                                   "direction": [1.0, 0.0, 0.0], "scale": 1.0}})
    with pytest.raises(DASError, match="DASolidDisplacementFoam"):
        make(case, outputInfo={"q": {"type": "forceCouplingOutput", "patches": ["top"], "components": ["forceCoupling"], "pRef": 0.0}})
    with pytest.raises(DASError, match="DASolidDisplacementFoam"):
        make(case, fvSource={"s": {"type": "heatSource"}})
    with pytest.raises(DASError, match="DASolidDisplacementFoam"):
        make(case).solver.simpleIteration()


@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_adjoint_of_variable_vol_sum(mesh):
    case, g, _, A = restated(mesh, "strain", 2)
    fn = {"DX": {"type": "variableVolSum", "source": "allCells", "varName": "D", "varType": "vector", "index": 0, "isSquare": 1, "multiplyVol": 1,
                 "divByTotalVol": 0, "scale": 1e12}}
    D = make(case, 2, function=fn, adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    rhs = np.zeros(case.states.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", case.states, "DX", "function", np.ones(1), rhs)
    psi, fail = D.solveAdjoint(rhs)
    ref = spla.spsolve(A.tocsc(), rhs)
    e, r = np.linalg.norm(psi - ref) / np.linalg.norm(ref), np.linalg.norm(A @ psi - rhs) / np.linalg.norm(rhs)
    print(mesh, "psi", e, "true residual", r, "fail", fail)
    assert fail == 0 and e <= 1e-6 and r <= 1e-10


def test_newton_primal():
    """the problem is linear in D for a fixed number of passes: with a tight linear solve and no pseudo-time damping Newton is there in
    at most 3 steps"""
    case, g, R0, _ = restated("bump", "strain", 2)
    D = make(case, 2, amd={"primalTau0": 1e30, "primalTauMax": 1e30, "primalLinearTol": 1e-13, "primalLinearIters": 2000})
    fail, info = D.solver.solvePrimal(maxSteps=3, relTol=1e-10)
    W = D.getStates()
    print("Newton primal:", info["steps"], "steps,", info["res"] / info["res0"])
    assert fail == 0 and info["steps"] <= 3 and info["res"] <= 1e-10 * info["res0"]
    assert np.linalg.norm(S.residual(case, g, W, 2)) <= 1e-9 * np.linalg.norm(R0)


def test_newton_primal_refuses_a_singular_case():
    case = solid_displacement_case(4, 3, 3, D_bcs={"outlet": ("tractionDisplacement", (1e5, 0.0, 0.0), 0.0)})
    with pytest.raises(DASError, match="no patch carries a fixedValue D"):
        make(case).solver.solvePrimal()


# ---- the objectives: vonMisesStressKS (allCells, boxToCell), variableVolSum of D and of solid:rho (the mass) ------------------------------
def restated_function(case, g, name, passes):
    box = S.box_cells(g, *KS_BOX)
    if name == "VMS":
        return lambda D, gg=g: S.von_mises_ks(case, gg, D, passes, KS_SCALE, KS_COEFF)
    if name == "VMSBOX":
        return lambda D, gg=g: S.von_mises_ks(case, gg, D, passes, KS_SCALE, KS_COEFF, box)  # the set is chosen once, at definition
    if name == "MASS":
        return lambda D, gg=g: S.mass(case, gg) + 0.0 * D[0]
    return lambda D, gg=g: 3.0 * (gg.V * D.reshape(-1, 3)[:, 1]).sum()


@pytest.mark.parametrize("mesh,passes", [("bump", 2), ("mixed", 20)])
def test_functions_values_and_derivatives(mesh, passes):
    case, g, _, _ = restated(mesh, "strain", passes)
    D = make(case, passes, function=solid_functions(),
             inputInfo={"x": {"type": "volCoord"}, "Din": {"type": "patchVar", "patches": ["inlet"], "varName": "D", "varType": "vector"},
                        "pv": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"},
                        "beta": {"type": "field", "fieldName": "betaFINuTilda", "fieldType": "scalar"}})
    Sv = D.solverAD
    W, X0 = case.states, case.mesh.points.ravel().copy()
    idx = [3 * p + k for p in sample_points(case) for k in range(3)]
    for name in ("VMS", "VMSBOX", "MASS", "DY"):
        F = restated_function(case, g, name, passes)
        v1, v2 = Sv.calcFunction(name), Sv.calcFunction(name)
        ref = float(np.real(F(W.astype(np.complex128))))
        print(mesh, passes, name, "value", v1, abs(v1 - ref) / abs(ref))
        assert v1 == v2 and abs(v1 - ref) <= 1e-12 * abs(ref)
        dF, dF2 = np.zeros(W.size), np.ones(W.size)
        Sv.calcJacTVecProduct("states", "stateVar", W, name, "function", np.ones(1), dF)
        Sv.calcJacTVecProduct("states", "stateVar", W, name, "function", np.ones(1), dF2)
        assert np.array_equal(dF, dF2)
        if name == "MASS":
            assert np.all(dF == 0.0)  # no state reaches the mass
        else:
            refd = np.zeros(W.size)
            for j in range(W.size):
                Wp = W.astype(np.complex128)
                Wp[j] += 1e-30j
                refd[j] = SC * np.imag(F(Wp)) / 1e-30
            print(mesh, passes, name, "dFdW", np.abs(dF - refd).max() / np.abs(refd).max())
            assert np.abs(refd).max() > 0 and np.abs(dF - refd).max() <= 1e-10 * np.abs(refd).max()
        prod = np.zeros(X0.size)
        Sv.calcJacTVecProduct("x", "volCoord", X0, name, "function", np.ones(1), prod)
        refx = []
        for j in idx:
            X = X0.astype(np.complex128)
            X[j] += 1e-30j
            refx.append(np.imag(F(W.astype(np.complex128), gg=S.Geom(case.mesh, X.reshape(-1, 3)))) / 1e-30)
        refx = np.array(refx)
        print(mesh, passes, name, "volCoord", np.abs(prod[idx] - refx).max() / np.abs(prod).max())
        assert np.abs(refx).max() > 0 and np.abs(prod[idx] - refx).max() <= 1e-10 * np.abs(prod).max()
        # inputs that reach no objective of this solver: exact zeros
        z = np.ones(3)
        Sv.calcJacTVecProduct("Din", "patchVar", np.zeros(3), name, "function", np.ones(1), z)
        assert np.all(z == 0.0)
        z = np.ones(2)
        Sv.calcJacTVecProduct("pv", "patchVelocity", np.array([0.0, 0.0]), name, "function", np.ones(1), z)  # (magnitude 0: the inlet stays at 0)
        assert np.all(z == 0.0)
        z = np.ones(g.nC)
        Sv.calcJacTVecProduct("beta", "field", np.ones(g.nC), name, "function", np.ones(1), z)
        assert np.all(z == 0.0)


@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_adjoint_of_von_mises_ks(mesh):
    case, g, _, A = restated(mesh, "strain", 2)
    D = make(case, 2, function=solid_functions(), adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    rhs = np.zeros(case.states.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", case.states, "VMS", "function", np.ones(1), rhs)
    psi, fail = D.solveAdjoint(rhs)
    ref = spla.spsolve(A.tocsc(), rhs)
    e, r = np.linalg.norm(psi - ref) / np.linalg.norm(ref), np.linalg.norm(A @ psi - rhs) / np.linalg.norm(rhs)
    print(mesh, "VMS psi", e, "true residual", r, "fail", fail)
    assert fail == 0 and e <= 1e-6 and r <= 1e-10


def test_total_derivative_of_von_mises_ks_against_reconverged_primals():
    """dF/dX - psi^T dR/dX in one point-displacement direction against central differences of primals re-converged by the restatement
    (the problem is linear in D: one dense solve per mesh).  Step and bound of the wall-bump check of tests/test_gpu_parity.py: a
    relative step of 2.5e-4 of the cell size, 5e-5."""
    case, g, _, _ = restated("bump", "strain", 2)
    passes = 2

    def converged(gg):
        W0 = case.states
        J = S.jacobian(case, gg, W0, passes)
        return W0 - np.linalg.solve(J, S.residual(case, gg, W0, passes))

    D = make(case, passes, function=solid_functions(), inputInfo={"x": {"type": "volCoord"}},
             adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0},
             amd={"primalTau0": 1e30, "primalTauMax": 1e30, "primalLinearTol": 1e-13, "primalLinearIters": 2000})
    fail, info = D.solver.solvePrimal(maxSteps=3, relTol=1e-11)
    assert fail == 0
    W = D.getStates()
    assert rel(W, converged(g)) <= 1e-6
    X0 = case.mesh.points.ravel().copy()
    dFdW, gF, gR = np.zeros(W.size), np.zeros(X0.size), np.zeros(X0.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "VMS", "function", np.ones(1), dFdW)
    psi, fail = D.solveAdjoint(dFdW)
    assert fail == 0
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "VMS", "function", np.ones(1), gF)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, gR)
    m = case.mesh
    top = {p.name: p for p in m.patches}["top"]
    j = 3 * int(m.face_pts[m.face_ptr[top.start + 8]]) + 1  # a point of the loaded top patch, moved in y
    total = gF[j] - gR[j]
    h = 1e-5
    Fs = []
    for sgn in (1.0, -1.0):
        X = X0.copy()
        X[j] += sgn * h
        gg = S.Geom(m, X.reshape(-1, 3))
        Fs.append(S.von_mises_ks(case, gg, converged(gg), passes, KS_SCALE, KS_COEFF))
    fd = (Fs[0] - Fs[1]) / (2 * h)
    print("total derivative", total, "central difference", fd, "relative", abs(total - fd) / abs(fd))
    assert abs(total - fd) <= 5e-5 * abs(fd)

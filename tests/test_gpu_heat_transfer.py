"""DAHeatTransferFoam, the solid side of conjugate heat transfer, on the device: residual, Jacobians, products, colouring, adjoint, the
objectives wallHeatFlux and variableVolSum(T), the coupling output and input of discipline thermal with their products, the Newton primal
and the exchange loop of a composite wall between two solver instances - against the numpy restatement
(tests/heat_transfer_restatement.py) and its complex step.  Bars: 1e-12 relative for values, 1e-10 for derivative entries and products,
the finite-difference bar of tests/test_gpu_parity.py (1e-4 against exact entries) for dRdWTPC, 1e-6 for an adjoint vector or a device
primal against an independent one."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import heat_transfer_restatement as H
from dafoam_amd._capi import DASError
from dafoam_amd.meshgen import heat_transfer_case
from heat_transfer_cases import MATERIALS, MESHES, NORM, heat_case, heat_options, mixed_records
from test_heat_transfer_cpu import composite_wall

pytestmark = pytest.mark.gpu

SC = NORM["T"]  # the state scale of every unknown
OUT, INP = "thermalCouplingOutput", "thermalCoupling"


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=heat_options(case, **extra), case=case)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


@functools.lru_cache(maxsize=None)
def restated(mesh, material):
    """(case, geometry, residual, D_s dRdW^T by the complex step) - computed once, shared, read-only"""
    case = heat_case(mesh, material)
    g = H.Geom(case.mesh)
    Jm = H.jacobian_cs(lambda x: H.residual(case, g, x), case.states)
    return case, g, H.residual(case, g, case.states), sp.csr_matrix((Jm * SC).T)


def cs_gradient(fun, x, idx=None, h=1e-30):
    x = np.asarray(x, dtype=np.complex128)
    out = []
    for j in range(x.size) if idx is None else idx:
        xp = x.copy()
        xp[j] += 1j * h
        out.append(np.imag(fun(xp)) / h)
    return np.array(out)


# ---- 8: residual -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("material", sorted(MATERIALS))
@pytest.mark.parametrize("mesh", MESHES)
def test_residual(mesh, material):
    case, g, Ro, _ = restated(mesh, material)
    S = make(case).solver
    R, R2 = np.zeros(g.nC), np.ones(g.nC)
    S.getResiduals(R)
    S.getResiduals(R2)
    print(mesh, material, "residual", rel(R, Ro))
    assert np.array_equal(R, R2) and rel(R, Ro) <= 1e-12
    Rp = np.zeros(g.nC)
    S.calcResiduals(1, Rp)
    assert np.array_equal(R, Rp)  # no PC variant of this residual


def test_residual_not_normalised():
    case, g, _, _ = restated("mixed", "poly")
    S = make(case, normalizeResiduals=["URes", "pRes"]).solver
    R = np.zeros(g.nC)
    S.getResiduals(R)
    assert rel(R, H.residual(case, g, case.states, normalized=False)) <= 1e-12


# ---- 9: dRdWT (dual numbers) and dRdWTPC (finite differences) ----------------------------------------------------------------------
@pytest.mark.parametrize("material", sorted(MATERIALS))
@pytest.mark.parametrize("mesh", MESHES)
def test_jacobians(mesh, material):
    from dafoam_amd.pyDASolvers import Mat

    case, g, _, A = restated(mesh, material)
    D = make(case, jacLowerBounds={"dRdW": 0.0, "dRdWPC": 0.0})
    D.solver.runColoring()
    M = Mat()
    D.solver.calcdRdWT(0, M, mode=1)
    e = np.abs((M.to_scipy() - A).toarray()).max() / np.abs(A.data).max()
    Mp = Mat()
    D.solver.calcdRdWT(1, Mp)  # the reference's coloured finite differences
    efd = np.abs((Mp.to_scipy() - A).toarray()).max() / np.abs(A.data).max()
    print(mesh, material, "dual", e, "FD", efd)
    assert e <= 1e-10 and efd <= 1e-4


# ---- 10: J^T v, J v and the dot-product identity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,material", [("bump432", "poly"), ("mixed_renumbered", "poly"), ("bump", "const")])
def test_products_and_dot_product_identity(mesh, material):
    case, g, _, A = restated(mesh, material)
    D = make(case)
    rng = np.random.default_rng(5)
    psi, v = rng.standard_normal(g.nC), rng.standard_normal(g.nC)
    prod, Jv = np.zeros(g.nC), np.zeros(g.nC)
    D.solverAD.calcJacTVecProduct("states", "stateVar", case.states, "residuals", "residual", psi, prod)
    D.solverAD.calcJacVecProduct(v, Jv)
    ref = np.imag(H.residual(case, g, case.states + 1e-30j * SC * v)) / 1e-30
    print(mesh, material, rel(prod, A @ psi), rel(Jv, ref))
    assert rel(prod, A @ psi) <= 1e-10 and rel(Jv, ref) <= 1e-10
    assert abs(psi @ Jv - prod @ v) <= 1e-10 * np.abs(psi * Jv).sum()


# ---- 11: colouring -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["bump432", "mixed_renumbered"])
def test_device_colouring_is_the_host_first_fit(mesh):
    case = heat_case(mesh, "const")
    Dd, Dh = make(case), make(case, amd={"coloringOnDevice": 0})
    Dd.solver.runColoring()
    Dh.solver.runColoring()
    (cd, nd), (ch, nh) = Dd.solver.getColoring(), Dh.solver.getColoring()
    assert nd == nh and np.array_equal(cd, ch)


# ---- 12 - 14: objectives and the adjoint -------------------------------------------------------------------------------------------
WHF_PATCHES = ["bottom", "top"]  # a mixed and a fixedValue patch


def functions(by_unit_area=True):
    return {"HFX": {"type": "wallHeatFlux", "source": "patchToFace", "patches": list(WHF_PATCHES), "scale": 0.5, "byUnitArea": by_unit_area},
            "TVOL": {"type": "variableVolSum", "source": "allCells", "varName": "T", "varType": "scalar", "index": 0, "isSquare": 0,
                     "multiplyVol": 1, "divByTotalVol": 1, "scale": 2.0}}


def restated_function(case, g, name, mode="default", by_unit_area=True):
    if name == "HFX":
        return lambda T, gg=g, **kw: H.wall_heat_flux(case, gg, T, WHF_PATCHES, mode, by_unit_area, 0.5, **kw)
    return lambda T, gg=g, **kw: H.var_vol_sum(gg, T, scale=2.0, div_by_total_vol=True)


@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_adjoint(mesh):
    case, g, _, A = restated(mesh, "poly")
    D = make(case, function=functions(), adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    for name in ("HFX", "TVOL"):
        rhs = np.zeros(g.nC)
        D.solverAD.calcJacTVecProduct("states", "stateVar", case.states, name, "function", np.ones(1), rhs)
        dF = SC * cs_gradient(restated_function(case, g, name), case.states)
        assert rel(rhs, dF) <= 1e-10
        psi, fail = D.solveAdjoint(rhs)
        ref = spla.spsolve(A.tocsc(), rhs)
        e, r = np.linalg.norm(psi - ref) / np.linalg.norm(ref), np.linalg.norm(A @ psi - rhs) / np.linalg.norm(rhs)
        print(mesh, name, "psi", e, "true residual", r, "fail", fail)
        assert fail == 0 and e <= 1e-6 and r <= 1e-10


def sample_points(case):
    """an interior point, points of the function patches and of a corner, and (mixed mesh) the apex of a hex cut into pyramids"""
    m = case.mesh
    by = {p.name: p for p in m.patches}
    pts = {3 + 7 * (2 + 6 * 2), 0, int(m.face_pts[m.face_ptr[by["bottom"].start + 5]]), int(m.face_pts[m.face_ptr[by["top"].start + 3] + 1]),
           int(m.face_pts[m.face_ptr[by["inlet"].start + 2]])}
    if m.n_points > 210:
        pts.add(210)
    return sorted(pts)


@pytest.mark.parametrize("by_unit_area", [True, False])
@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_wall_heat_flux(mesh, mode, by_unit_area):
    case, g, _, _ = restated(mesh, "poly")
    D = make(case, function=functions(by_unit_area), wallDistanceMethod=mode,
             inputInfo={"x": {"type": "volCoord"}, "Ttop": {"type": "patchVar", "patches": ["top"], "varName": "T", "varType": "scalar"}})
    S = D.solverAD
    F = restated_function(case, g, "HFX", mode, by_unit_area)
    T = case.states
    v1, v2 = S.calcFunction("HFX"), S.calcFunction("HFX")
    assert v1 == v2 and abs(v1 - F(T)) <= 1e-12 * abs(F(T))
    dFdW = np.zeros(g.nC)
    S.calcJacTVecProduct("states", "stateVar", T, "HFX", "function", np.ones(1), dFdW)
    assert rel(dFdW, SC * cs_gradient(F, T)) <= 1e-10
    tan = np.zeros(1)
    S.calcJacTVecProduct("Ttop", "patchVar", np.array([300.0]), "HFX", "function", np.ones(1), tan)
    ref = np.imag(F(T, values={"top": 300.0 + 1e-30j})) / 1e-30
    assert ref != 0.0 and abs(tan[0] - ref) <= 1e-10 * abs(ref)
    X0 = case.mesh.points.ravel().copy()
    prod = np.zeros(X0.size)
    S.calcJacTVecProduct("x", "volCoord", X0, "HFX", "function", np.ones(1), prod)
    idx = [3 * p + k for p in sample_points(case) for k in range(3)]
    ref = cs_gradient(lambda X: F(T, gg=H.Geom(case.mesh, X.reshape(-1, 3))), X0, idx)
    print(mesh, mode, by_unit_area, "value", v1, "volCoord", np.abs(prod[idx] - ref).max() / np.abs(prod).max())
    assert np.abs(ref).max() > 0 and np.abs(prod[idx] - ref).max() <= 1e-10 * np.abs(prod).max()


@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_variable_vol_sum(mesh):
    case, g, _, _ = restated(mesh, "poly")
    S = make(case, function=functions()).solverAD
    F = restated_function(case, g, "TVOL")
    v = S.calcFunction("TVOL")
    assert abs(v - F(case.states)) <= 1e-12 * abs(v)
    dFdW = np.zeros(g.nC)
    S.calcJacTVecProduct("states", "stateVar", case.states, "TVOL", "function", np.ones(1), dFdW)
    assert rel(dFdW, SC * cs_gradient(F, case.states)) <= 1e-10


# ---- 15: thermalCouplingOutput, discipline thermal ---------------------------------------------------------------------------------
TC_PATCHES = ["top", "bottom", "inlet"]  # as the user lists them - not sorted; bottom is mixed, the others fixedValue


def tc_info(patches, typ=OUT):
    return {"type": typ, "patches": list(patches), "components": ["thermalCoupling"]}


@pytest.mark.parametrize("material", sorted(MATERIALS))
@pytest.mark.parametrize("mode", H.MODES)
@pytest.mark.parametrize("mesh", ["bump", "mixed_renumbered"])
def test_coupling_output_values(mesh, mode, material):
    case, g, _, _ = restated(mesh, material)
    S = make(case, discipline="thermal", wallDistanceMethod=mode, outputInfo={"q": tc_info(TC_PATCHES), "r": tc_info(TC_PATCHES[::-1])}).solver
    ref = H.coupling_output(case, g, case.states, TC_PATCHES, mode)
    n = 2 * H.selected_faces(case, TC_PATCHES).size
    assert S.getOutputSize("q", OUT) == n == ref.size
    a, b, c = np.zeros(n), np.ones(n), np.zeros(n)
    S.calcOutput("q", OUT, a)
    S.calcOutput("q", OUT, b)
    S.calcOutput("r", OUT, c)
    assert np.array_equal(a, b) and np.array_equal(a, c)  # repeatable; the order in which the patches are listed does not matter
    assert np.array_equal(a[: n // 2], ref[: n // 2]) and rel(a[n // 2 :], ref[n // 2 :]) <= 1e-12 and ref[n // 2 :].min() > 0


@pytest.mark.parametrize("mesh,mode", [("bump", "default"), ("mixed", "daCustom")])
def test_coupling_output_products(mesh, mode):
    case, g, _, _ = restated(mesh, "poly")
    D = make(case, discipline="thermal", wallDistanceMethod=mode, outputInfo={"q": tc_info(TC_PATCHES)},
             inputInfo={"x": {"type": "volCoord"}, "Ttop": {"type": "patchVar", "patches": ["top"], "varName": "T", "varType": "scalar"},
                        "beta": {"type": "field", "fieldName": "betaFINuTilda", "fieldType": "scalar"}})
    S = D.solverAD
    T = case.states
    n = 2 * H.selected_faces(case, TC_PATCHES).size
    X0 = case.mesh.points.ravel().copy()
    idx = [3 * p + k for p in sample_points(case) for k in range(3)]
    for seeds in np.random.default_rng(11).standard_normal((2, n)):
        F = lambda Tp, gg=g, **kw: seeds @ H.coupling_output(case, gg, Tp, TC_PATCHES, mode, **kw)  # noqa: E731
        prod = np.zeros(g.nC)
        S.calcJacTVecProduct("states", "stateVar", T, "q", OUT, seeds, prod)
        prod2 = np.zeros(g.nC)
        S.calcJacTVecProduct("states", "stateVar", T, "q", OUT, seeds, prod2)
        assert rel(prod, SC * cs_gradient(F, T)) <= 1e-10
        tan = np.zeros(1)
        S.calcJacTVecProduct("Ttop", "patchVar", np.array([300.0]), "q", OUT, seeds, tan)
        ref = np.imag(F(T, values={"top": 300.0 + 1e-30j})) / 1e-30
        assert ref != 0.0 and abs(tan[0] - ref) <= 1e-10 * abs(ref)
        pv = np.zeros(X0.size)
        S.calcJacTVecProduct("x", "volCoord", X0, "q", OUT, seeds, pv)
        ref = cs_gradient(lambda X: F(T, gg=H.Geom(case.mesh, X.reshape(-1, 3))), X0, idx)
        print(mesh, mode, "volCoord", np.abs(pv[idx] - ref).max() / np.abs(pv).max())
        assert np.abs(ref).max() > 0 and np.abs(pv[idx] - ref).max() <= 1e-10 * np.abs(pv).max()
        beta = np.ones(g.nC)
        S.calcJacTVecProduct("beta", "field", np.ones(g.nC), "q", OUT, seeds, beta)
        assert np.all(beta == 0.0)


# ---- 16: the thermalCoupling input --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corner_case():
    """bottom and outlet mixed: the cells along their common edge hold two coupled faces"""
    return heat_transfer_case(6, 5, 4, kappa_coeffs=MATERIALS["poly"]["kappa_coeffs"],
                              mixed_patches={"bottom": mixed_records(24), "outlet": mixed_records(20, seed=4)})


@pytest.mark.parametrize("mode", H.MODES)
def test_coupling_input_records_and_products(mode):
    case = corner_case()
    g = H.Geom(case.mesh)
    T = case.states
    patches = ["outlet", "bottom"]
    own = case.mesh.owner[H.selected_faces(case, patches)]
    assert np.unique(own).size < own.size  # corner cells
    D = make(case, discipline="thermal", wallDistanceMethod=mode, inputInfo={"in": tc_info(patches, INP)}, outputInfo={"q": tc_info(patches)},
             function={"HFX": {"type": "wallHeatFlux", "source": "patchToFace", "patches": ["bottom"], "scale": 1.0}})
    S = D.solverAD
    nF = own.size
    rng = np.random.default_rng(2)
    inp = np.concatenate([290.0 + 20.0 * rng.random(nF), H.coupling_output(case, g, T, patches, mode)[nF:] * (0.3 + 2.0 * rng.random(nF))])
    assert S.getInputSize("in", INP) == 2 * nF
    S.setSolverInput("in", INP, 2 * nF, inp)
    rec = H.coupling_records(case, g, T, patches, inp, mode)
    for nm in patches:
        ref, frac = S.getPatchMixedT(nm)
        assert np.array_equal(ref, rec[nm][0]) and rel(frac, rec[nm][1]) <= 1e-14
    R = np.zeros(g.nC)
    S.getResiduals(R)
    assert rel(R, H.residual(case, g, T, mixed=rec)) <= 1e-12

    # every product sets the input again, and with kappa(T_b) the fraction of a set reads the boundary temperature the records before it
    # give: `before` follows the records on the device from set to set
    before = rec
    psi = rng.standard_normal(g.nC)
    seeds_q = rng.standard_normal(2 * nF)
    targets = [("residuals", "residual", psi, lambda r: psi @ H.residual(case, g, T, mixed=r)),
               ("HFX", "function", np.ones(1), lambda r: H.wall_heat_flux(case, g, T, ["bottom"], mode, True, 1.0, mixed=r)),
               ("q", OUT, seeds_q, lambda r: seeds_q @ H.coupling_output(case, g, T, patches, mode, mixed=r))]
    for name, typ, seeds, fun in targets:
        prod = np.zeros(2 * nF)
        S.calcJacTVecProduct("in", INP, inp, name, typ, seeds, prod)
        ref = cs_gradient(lambda x: fun(H.coupling_records(case, g, T, patches, x, mode, mixed=before)), inp)
        before = H.coupling_records(case, g, T, patches, inp, mode, mixed=before)
        for nm in patches:
            assert rel(S.getPatchMixedT(nm)[1], before[nm][1]) <= 1e-14
        print(mode, typ, "product", rel(prod[:nF], ref[:nF]), rel(prod[nF:], ref[nF:]))
        assert np.abs(ref[:nF]).max() > 0 and np.abs(ref[nF:]).max() > 0
        assert rel(prod[:nF], ref[:nF]) <= 1e-10 and rel(prod[nF:], ref[nF:]) <= 1e-10
    # the same product twice from the same records: the same bits (a constant kappa makes the set idempotent)
    flat = heat_transfer_case(6, 5, 4, kappa=200.0, mixed_patches={"bottom": mixed_records(24), "outlet": mixed_records(20, seed=4)})
    S2 = make(flat, discipline="thermal", wallDistanceMethod=mode, inputInfo={"in": tc_info(patches, INP)}).solverAD
    p1, p2 = np.zeros(2 * nF), np.ones(2 * nF)
    S2.calcJacTVecProduct("in", INP, inp, "residuals", "residual", psi, p1)
    S2.calcJacTVecProduct("in", INP, inp, "residuals", "residual", psi, p2)
    assert np.array_equal(p1, p2) and p1.any()


# ---- 17: the Newton primal ----------------------------------------------------------------------------------------------------------
def test_newton_primal():
    case, g, R0, _ = restated("bump", "poly")
    D = make(case)
    fail, info = D.solver.solvePrimal(maxSteps=50, relTol=1e-10)
    W = D.getStates()
    print("Newton primal:", info["steps"], "steps,", info["res"] / info["res0"])
    assert fail == 0 and info["steps"] <= 50 and info["res"] <= 1e-10 * info["res0"]
    assert np.linalg.norm(H.residual(case, g, W)) <= 1e-9 * np.linalg.norm(R0)
    Tn, _ = H.newton(case, g, case.states)
    assert rel(W, Tn) <= 1e-6


def test_newton_primal_refuses_a_singular_case():
    case = heat_transfer_case(4, 3, 3, kappa=10.0, T_bcs={})
    with pytest.raises(DASError, match="no patch carries a fixedValue or mixed T"):
        make(case).solver.solvePrimal()


# ---- 18: the composite wall between two solver instances ----------------------------------------------------------------------------
def test_composite_wall_exchange_between_two_solvers():
    a, b, q, Ti = composite_wall()
    sides = []
    for case, patch in ((a, "outlet"), (b, "inlet")):
        D = make(case, discipline="thermal", wallDistanceMethod="daCustom", inputInfo={"in": tc_info([patch], INP)}, outputInfo={"out": tc_info([patch])},
                 function={"HFX": {"type": "wallHeatFlux", "source": "patchToFace", "patches": [patch], "scale": 1.0, "byUnitArea": True}})
        R = np.zeros(case.states.size)
        D.solver.getResiduals(R)
        sides.append((D.solver, patch, 1e-11 * np.linalg.norm(R)))
    (A, pa, tol_a), (B, pb, tol_b) = sides
    n = A.getOutputSize("out", OUT)
    assert n == B.getInputSize("in", INP) == 18
    out_a, out_b, last = np.zeros(n), np.zeros(n), None
    for n_exchanges in range(1, 21):
        A.calcOutput("out", OUT, out_a)
        B.setSolverInput("in", INP, n, out_a)
        assert B.solvePrimal(maxSteps=50, relTol=0.0, absTol=tol_b)[0] == 0
        B.calcOutput("out", OUT, out_b)
        A.setSolverInput("in", INP, n, out_b)
        assert A.solvePrimal(maxSteps=50, relTol=0.0, absTol=tol_a)[0] == 0
        now = np.concatenate([out_a[: n // 2], out_b[: n // 2]])
        if last is not None and np.abs(now - last).max() < 1e-10:
            break
        last = now
    else:
        pytest.fail("the exchange loop did not settle to 1e-10 K in 20 exchanges")
    Ti_dev = []
    for S, patch, case in ((A, pa, a), (B, pb, b)):
        ref, frac = S.getPatchMixedT(patch)
        W = np.zeros(case.states.size)
        S.getOFFields(W)
        pt = {p.name: p for p in case.mesh.patches}[patch]
        Ti_dev.append(frac * ref + (1.0 - frac) * W[case.mesh.owner[pt.start : pt.start + pt.size]])
    qa, qb = A.calcFunction("HFX"), B.calcFunction("HFX")
    print("exchanges", n_exchanges, "T_i", Ti_dev[0].mean(), Ti_dev[1].mean(), "analytic", Ti, "q", qa, qb, "analytic", q)
    for t in Ti_dev:
        assert np.abs(t - Ti).max() <= 1e-6 * 100.0
    assert abs(-qa - q) <= 1e-6 * q and abs(qb - q) <= 1e-6 * q and abs(qa + qb) <= 1e-6 * q

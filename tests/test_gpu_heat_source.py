"""The heat sources of DAHeatTransferFoam (the fvSource option, type heatSource) and the fvSourcePar input on the device: the field, the
residual, the unchanged state Jacobians, the parameter and the mesh products, updateOFMesh, the Newton primal with its energy balance and
an adjoint total derivative - against the numpy restatement (tests/heat_source_restatement.py) and its complex step.  Bars
(tests/README_heat_transfer.md): 1e-12 relative for values, 1e-10 for products, fields relative to their maximum; "bitwise" is
np.array_equal.  Notes: tests/README_heat_source.md."""
import functools
import math

import numpy as np
import pytest

import heat_source_restatement as HS
import heat_transfer_restatement as H
from heat_source_cases import ALL_SOURCES, SOURCE_A, SOURCE_B, geom, source_case, sources
from heat_transfer_cases import MESHES, NORM, heat_case, heat_options

pytestmark = pytest.mark.gpu

NAMES = ("mid_A", "tail_B", "head_C")
PAR_INPUTS = {"all_A": {"type": "fvSourcePar", "fvSourceName": "mid_A", "components": ["solver"]},
              "two_A": {"type": "fvSourcePar", "fvSourceName": "mid_A", "indices": [0, 6], "components": ["solver"]},
              "all_C": {"type": "fvSourcePar", "fvSourceName": "head_C", "components": ["solver"]},
              "x": {"type": "volCoord"}}
HFX_ALL = {"HFX": {"type": "wallHeatFlux", "source": "patchToFace", "patches": ["inlet", "outlet", "top", "bottom", "front", "back"], "scale": 1.0, "byUnitArea": False}}


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=heat_options(case, **extra), case=case)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def pars_of(name):
    e = ALL_SOURCES[name]
    return np.array(list(e["center"]) + list(e["axis"]) + [e["radius"], e["length"], e["power"]])


@functools.lru_cache(maxsize=None)
def restated(mesh):
    """(case, geometry, sources, field, residual with the field) - computed once, shared, read-only"""
    case, g, S = source_case(mesh), geom(mesh), sources(mesh)
    return case, g, S, np.real(S.field(g)), np.real(HS.residual(case, g, case.states, S))


# ---- the field ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES + ("box",))
def test_field_totals_and_repeatability(mesh):
    case, g, S, q, _ = restated(mesh)
    D = make(case, fvSource=dict(ALL_SOURCES))
    a, b = D.solver.getFvSource(), D.solver.getFvSource()
    info = {n: D.solver.heatSourceInfo(n) for n in NAMES}
    print(mesh, "field", rel(a, q), "sourceTotal", info["mid_A"]["sourceTotal"], "of", S.total_power())
    assert np.array_equal(a, b) and rel(a, q) <= 1e-12
    assert abs(info["mid_A"]["sourceTotal"] - S.total_power()) <= 1e-13 * S.total_power()
    for n in NAMES:
        Vt = float(np.real(S.entry_field(g, n)[1]))
        assert abs(info[n]["volumeTotal"] - Vt) <= 1e-13 * Vt
    if mesh == "box":  # 8 workgroups of partial sums: the two-stage sum against an exactly rounded one
        e = S.entries["mid_A"]
        s = HS.smooth_shape(g, e["pars"].real, e["eps"])
        assert abs(info["mid_A"]["volumeTotal"] - math.fsum(s * g.V)) <= 1e-13 * math.fsum(s * g.V)
        cells = S.entries["tail_B"]["cells"]
        assert abs(info["tail_B"]["volumeTotal"] - math.fsum(g.V[cells])) <= 1e-13 * math.fsum(g.V[cells])
    assert sorted(info["tail_B"]["cells"]) == sorted(S.entries["tail_B"]["cells"])
    assert info["head_C"]["snappedCell"] == S.entries["head_C"]["cell"]
    # the order of definition does not matter: the entries are walked by name
    D2 = make(case, fvSource={n: ALL_SOURCES[n] for n in reversed(NAMES)})
    assert np.array_equal(D2.solver.getFvSource(), a)


# ---- the residual ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_residual_with_sources_and_bitwise_without(mesh):
    case, g, S, q, Ro = restated(mesh)
    D = make(case, fvSource=dict(ALL_SOURCES))
    R, R2 = np.zeros(g.nC), np.ones(g.nC)
    D.solver.getResiduals(R)
    D.solver.calcResiduals(1, R2)
    print(mesh, "residual", rel(R, Ro))
    assert rel(R, Ro) <= 1e-12 and np.array_equal(R, R2)
    Du = make(case, fvSource=dict(ALL_SOURCES), normalizeResiduals=["URes", "pRes"])
    Ru = np.zeros(g.nC)
    Du.solver.getResiduals(Ru)
    assert rel(Ru, np.real(HS.residual(case, g, case.states, S, normalized=False))) <= 1e-12
    # no fvSource option, an empty one: the same bits, and those of the restatement without the term to 1e-12
    Ra, Rb = np.zeros(g.nC), np.zeros(g.nC)
    make(case).solver.getResiduals(Ra)
    make(case, fvSource={}).solver.getResiduals(Rb)
    assert np.array_equal(Ra, Rb) and rel(Ra, H.residual(case, g, case.states)) <= 1e-12 and not np.array_equal(Ra, R)


def test_state_jacobians_do_not_see_the_sources():
    from dafoam_amd.pyDASolvers import Mat

    case = source_case("mixed")
    out = []
    for fv in ({}, dict(ALL_SOURCES)):
        D = make(case, fvSource=fv, jacLowerBounds={"dRdW": 0.0, "dRdWPC": 0.0})
        D.solver.runColoring()
        M, Mp = Mat(), Mat()
        D.solver.calcdRdWT(0, M, mode=1)
        D.solver.calcdRdWT(1, Mp)
        psi = np.random.default_rng(5).standard_normal(case.states.size)
        prod = np.zeros(psi.size)
        D.solverAD.calcJacTVecProduct("states", "stateVar", case.states, "residuals", "residual", psi, prod)
        out.append((M.to_scipy().tocsr(), Mp.to_scipy().tocsr(), prod))
    for a, b in zip(out[0][:2], out[1][:2]):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    assert np.array_equal(out[0][0].data, out[1][0].data)  # dual numbers: the constant term leaves every tangent as it is
    assert np.array_equal(out[0][2], out[1][2])
    assert np.array_equal(out[0][1].data, out[1][1].data)  # the difference quotients of dRdWTPC are taken of the residual without the term


# ---- fvSourcePar ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("mesh", ["bump", "mixed_renumbered"])
def test_fv_source_par_products(mesh, normalized):
    case, g, S, _, _ = restated(mesh)
    extra = {} if normalized else {"normalizeResiduals": ["URes", "pRes"]}
    D = make(case, fvSource=dict(ALL_SOURCES), inputInfo=PAR_INPUTS, function=HFX_ALL, discipline="thermal",
             outputInfo={"q": {"type": "thermalCouplingOutput", "patches": ["top"], "components": ["thermalCoupling"]}}, **extra)
    A = D.solverAD
    psi = np.random.default_rng(7).standard_normal(g.nC)
    T = case.states

    def ref(name, idx):
        p0 = S.entries[name]["pars"]
        return np.array([np.imag(psi @ HS.residual(case, g, T, S, normalized=normalized, pars={name: p0 + 1e-30j * np.eye(9)[i]})) / 1e-30 for i in idx])

    p9, p9b, p2 = np.zeros(9), np.ones(9), np.zeros(2)
    A.calcJacTVecProduct("all_A", "fvSourcePar", pars_of("mid_A"), "residuals", "residual", psi, p9)
    A.calcJacTVecProduct("all_A", "fvSourcePar", pars_of("mid_A"), "residuals", "residual", psi, p9b)
    r9 = ref("mid_A", range(9))
    print(mesh, normalized, "A, nine parameters:", np.abs(p9 - r9) / np.abs(r9))
    assert np.array_equal(p9, p9b) and np.all(r9 != 0) and np.all(np.abs(p9 - r9) <= 1e-10 * np.abs(r9))
    A.calcJacTVecProduct("two_A", "fvSourcePar", pars_of("mid_A")[[0, 6]], "residuals", "residual", psi, p2)  # the reference's test: indices [0, 6]
    assert np.array_equal(p2, p9[[0, 6]])
    pc = np.ones(9)
    A.calcJacTVecProduct("all_C", "fvSourcePar", pars_of("head_C"), "residuals", "residual", psi, pc)
    rc = ref("head_C", range(9))
    print(mesh, normalized, "C:", np.abs(pc[3:] - rc[3:]) / np.abs(rc[3:]))
    assert np.all(pc[:3] == 0.0) and np.all(rc[:3] == 0.0) and np.all(np.abs(pc[3:] - rc[3:]) <= 1e-10 * np.abs(rc[3:]))
    for name, typ, seeds in (("HFX", "function", np.ones(1)), ("q", "thermalCouplingOutput", np.ones(A.getOutputSize("q", "thermalCouplingOutput")))):
        z = np.ones(9)
        A.calcJacTVecProduct("all_A", "fvSourcePar", pars_of("mid_A"), name, typ, seeds, z)
        assert np.all(z == 0.0)


def test_set_solver_input_moves_the_field_and_the_residual():
    case, g, S, q0, _ = restated("mixed")
    D = make(case, fvSource=dict(ALL_SOURCES), inputInfo=PAR_INPUTS)
    new = pars_of("mid_A") * np.array([1.1, 0.9, 1.2, 1.0, 2.0, 0.5, 1.3, 0.8, 1.7])
    D.set_solver_input({"all_A": new, "all_C": pars_of("head_C"), "two_A": new[[0, 6]], "x": case.mesh.points.ravel()})
    qn = np.real(S.field(g, {"mid_A": new}))
    R = np.zeros(g.nC)
    D.solver.getResiduals(R)
    f = D.solver.getFvSource()
    print("field", rel(f, qn), "moved by", rel(qn, q0))
    assert rel(f, qn) <= 1e-12 and rel(qn, q0) > 0.1
    assert rel(R, np.real(HS.residual(case, g, case.states, S, pars={"mid_A": new}))) <= 1e-12
    assert np.array_equal(D.solver.heatSourceInfo("mid_A")["pars"], new)
    D.solver.setSolverInput("two_A", "fvSourcePar", 2, pars_of("mid_A")[[0, 6]])
    assert np.array_equal(D.solver.heatSourceInfo("mid_A")["pars"][[0, 6]], pars_of("mid_A")[[0, 6]])


# ---- volCoord ---------------------------------------------------------------------------------------------------------------------------
def sample_points(case, S):
    """an interior, a patch, a corner and (mixed mesh) an apex point, a point of the snapped cell, and the far corner of the outlet, where
    every source is below 1e-30 of its peak"""
    m = case.mesh
    by = {p.name: p for p in m.patches}
    cell = S.entries["head_C"]["cell"]
    pts = {"interior": 3 + 7 * (2 + 6 * 2), "corner": 0, "patch": int(m.face_pts[m.face_ptr[by["bottom"].start + 5]]),
           "snapped": int(m.face_pts[m.face_ptr[int(np.nonzero(m.owner == cell)[0][0])]]), "far": int(np.argmax(m.points @ np.array([1.0, -1.0, -1.0])))}
    if m.n_points > 210:
        pts["apex"] = 210
    return pts


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_vol_coord_product_with_sources(mesh, normalized):
    case, g, S, _, _ = restated(mesh)
    extra = {} if normalized else {"normalizeResiduals": ["URes", "pRes"]}
    T = case.states
    psi = np.random.default_rng(9).standard_normal(g.nC)
    X0 = case.mesh.points.ravel().copy()
    pts = sample_points(case, S)
    idx = [3 * p + k for p in pts.values() for k in range(3)]

    def F(X, srcs, frozen=None):
        gg = H.Geom(case.mesh, X.reshape(-1, 3))
        return psi @ (HS.residual(case, gg, T, srcs, normalized=normalized, frozen=frozen) if srcs is not None else H.residual(case, gg, T, normalized=normalized))

    def cs(srcs, frozen=None):
        out = []
        for j in idx:
            X = X0.astype(np.complex128)
            X[j] += 1e-30j
            out.append(np.imag(F(X, srcs, frozen)) / 1e-30)
        return np.array(out)

    ref, ref0, ref_local = cs(S), cs(None), cs(S, frozen=g)
    D = make(case, fvSource=dict(ALL_SOURCES), inputInfo=PAR_INPUTS, **extra)
    prod, prod2 = np.zeros(X0.size), np.ones(X0.size)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod2)
    scale = np.abs(prod).max()
    err = np.abs(prod[idx] - ref).reshape(-1, 3).max(1) / scale
    print(mesh, normalized, "volCoord:", dict(zip(pts, err)), "the sources' share:", np.abs(ref - ref0).reshape(-1, 3).max(1) / scale)
    assert np.array_equal(prod, prod2) and np.abs(prod[idx] - ref).max() <= 1e-10 * scale
    # what a point does to the rows it cannot reach - through the total volumes and the snapped centre - is in the reference and not in a
    # pass with both frozen: a product without the rank-one terms cannot meet the bar.  (At the far corner every source has died away and
    # the point moves no total; the term is live at the points inside the sources.)
    gap = np.abs(ref - ref_local).reshape(-1, 3).max(1) / scale
    print("  of which through the totals and the snapped centre:", dict(zip(pts, gap)))
    assert gap[list(pts).index("interior")] > 1e-6 and gap[list(pts).index("snapped")] > 1e-6
    assert np.array_equal(ref[3 * list(pts).index("far"):][:3], ref0[3 * list(pts).index("far"):][:3])
    # the field is what it was
    assert rel(D.solver.getFvSource(), np.real(S.field(g))) <= 1e-12


def test_vol_coord_product_in_difference_mode():
    """amd.volCoordMode fd against the complex step of the restatement, at the bar of the difference mode (tests/test_gpu_functions_more.py:
    all entries within 5 % of the largest, 95 % within 1e-4)."""
    case, g, S, _, _ = restated("bump")
    T = case.states
    psi = np.random.default_rng(9).standard_normal(g.nC)
    X0 = case.mesh.points.ravel().copy()
    pts = sample_points(case, S)
    idx = [3 * p + k for p in pts.values() for k in range(3)]
    ref = []
    for j in idx:
        X = X0.astype(np.complex128)
        X[j] += 1e-30j
        ref.append(np.imag(psi @ HS.residual(case, H.Geom(case.mesh, X.reshape(-1, 3)), T, S)) / 1e-30)
    D = make(case, fvSource=dict(ALL_SOURCES), inputInfo=PAR_INPUTS, amd={"volCoordMode": "fd"})
    prod = np.zeros(X0.size)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod)
    err = np.abs(prod[idx] - np.array(ref)) / np.abs(prod).max()
    print("fd mode:", dict(zip(pts, err.reshape(-1, 3).max(1))))
    assert np.percentile(err, 95) <= 1e-4 and err.max() <= 5e-2
    assert rel(D.solver.getFvSource(), np.real(S.field(g))) <= 1e-12


def test_update_of_mesh_moves_the_field_and_keeps_the_choices():
    case, g, S, q0, _ = restated("mixed")
    D = make(case, fvSource=dict(ALL_SOURCES))
    m = case.mesh
    rng = np.random.default_rng(4)
    X = m.points + 0.004 * rng.standard_normal(m.points.shape) * np.array([1.0, 0.2, 0.1])
    before = D.solver.heatSourceInfo("tail_B")
    D.solver.updateOFMesh(np.ascontiguousarray(X.ravel()))
    g2 = H.Geom(m, X)
    q2 = np.real(S.field(g2))  # the cell set and the snapped cell of the first mesh, the metrics of the second
    after, snapped = D.solver.heatSourceInfo("tail_B"), D.solver.heatSourceInfo("head_C")
    f = D.solver.getFvSource()
    print("moved field", rel(f, q2), "moved by", rel(q2, q0), "totalV", before["volumeTotal"], "->", after["volumeTotal"])
    assert rel(f, q2) <= 1e-12 and rel(q2, q0) > 1e-3
    assert np.array_equal(before["cells"], after["cells"]) and before["volumeTotal"] != after["volumeTotal"]
    assert abs(after["volumeTotal"] - g2.V[S.entries["tail_B"]["cells"]].sum()) <= 1e-13 * after["volumeTotal"]
    assert snapped["snappedCell"] == S.entries["head_C"]["cell"] and rel(snapped["snappedCenter"], g2.C[snapped["snappedCell"]]) <= 1e-13
    R = np.zeros(g.nC)
    D.solver.getResiduals(R)
    assert rel(R, np.real(HS.residual(case, g2, case.states, S))) <= 1e-12


# ---- the primal, the energy balance and an adjoint total -------------------------------------------------------------------------------
AB = {"a": SOURCE_A, "b": SOURCE_B}


def test_newton_primal_conserves_the_power():
    case = heat_case("bump", "const")
    g = geom("bump")
    S = HS.Sources(g, AB)
    D = make(case, fvSource=dict(AB), function=HFX_ALL)
    R0 = np.zeros(g.nC)
    D.solver.getResiduals(R0)
    fail, info = D.solver.solvePrimal(maxSteps=50, relTol=1e-10)
    W = D.getStates()
    assert fail == 0 and info["res"] <= 1e-10 * info["res0"]
    res = np.linalg.norm(np.real(HS.residual(case, g, W, S))) / np.linalg.norm(R0)
    # the internal fluxes of the corrected Laplacian cancel in pairs and the boundary faces carry no correction: what the sources put in
    # leaves through the boundary, on a non-orthogonal mesh as well
    out = D.solver.calcFunction("HFX")
    P = S.total_power()
    print("primal:", info["steps"], "steps, residual of the restatement", res, " sum of wallHeatFlux", out, "+ powers", P, "=", out + P)
    assert res <= 1e-9
    assert abs(out + P) <= 1e-8 * P


def test_adjoint_total_derivative_of_the_heat_flux_in_the_source_parameters():
    """dHFX(top) / d(radius, power, center_x) of source a: -psi^T dR/dp with psi from solveAdjoint, against central differences of solvePrimal +
    calcFunction.  Per parameter the step is the one at which the two one-sided differences agree best, the bound ten times their disagreement."""
    case = heat_case("bump", "const")
    fn = {"HFX": {"type": "wallHeatFlux", "source": "patchToFace", "patches": ["top"], "scale": 1.0, "byUnitArea": False}}
    inputs = {"p": {"type": "fvSourcePar", "fvSourceName": "a", "indices": [6, 8, 0], "components": ["solver"]}}
    D = make(case, fvSource=dict(AB), function=fn, inputInfo=inputs, adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0})
    p0 = pars_of("mid_A")[[6, 8, 0]]

    def value(p):
        D.solver.setSolverInput("p", "fvSourcePar", 3, np.ascontiguousarray(p))
        fail, _ = D.solver.solvePrimal(maxSteps=50, relTol=1e-13)
        return D.solver.calcFunction("HFX")

    f0 = value(p0)
    fd, bound, step = np.zeros(3), np.zeros(3), np.zeros(3)
    for i in range(3):
        best = None
        for h in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6):
            dp = h * p0[i] * np.eye(3)[i]
            up, dn = (value(p0 + dp) - f0) / dp[i], (f0 - value(p0 - dp)) / dp[i]
            if best is None or abs(up - dn) < best[0]:
                best = (abs(up - dn), 0.5 * (up + dn), h)
        bound[i], fd[i], step[i] = 10.0 * best[0], best[1], best[2]
    assert value(p0) == f0
    W = D.getStates()
    rhs = np.zeros(W.size)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "HFX", "function", np.ones(1), rhs)
    psi, fail = D.solveAdjoint(rhs)
    prod = np.zeros(3)
    D.solverAD.calcJacTVecProduct("p", "fvSourcePar", p0, "residuals", "residual", psi, prod)
    total = -prod
    print("adjoint total", total, "central differences", fd, "relative steps", step, "bounds", bound, "difference", np.abs(total - fd))
    assert fail == 0 and np.all(fd != 0) and np.all(np.abs(total - fd) <= bound)


# ---- the option dictionary of the reference's unit test ---------------------------------------------------------------------------------
def test_the_reference_unit_test_dictionary_constructs_and_differentiates():
    """daOptions of the reference's tests/runUnitTests_DAHeatTransferFoam.py on heat_case("bump", "const"): its patch names replaced by
    this mesh's, its geometry scaled into the 1.0 x 0.2 x 0.1 box (y and z doubled), the rest as it stands - both fvSource entries, the
    fvSourcePar input with indices [0, 6], the wallHeatFlux function."""
    from dafoam_amd.pyDAFoam import PYDAFOAM

    case = heat_case("bump", "const")
    daOptions = {
        "designSurfaces": ["top", "bottom", "front"],
        "solverName": "DAHeatTransferFoam",
        "debug": True,
        "function": {"HFX": {"type": "wallHeatFlux", "source": "patchToFace", "patches": ["bottom"], "scale": 1}},
        "primalMinResTol": 1e-12,
        "fvSource": {
            "source1": {"type": "heatSource", "source": "cylinderToCell", "p1": [0.6, 0.11, 0.05], "p2": [1.0, 0.11, 0.05], "radius": 0.05, "power": 1000.0},
            "source2": {"type": "heatSource", "source": "cylinderSmooth", "center": [0.201, 0.112, 0.052], "axis": [1.0, 0.0, 0.0], "length": 0.4, "radius": 0.05,
                        "power": 1000.0, "eps": 0.01, "snapCenter2Cell": True},
        },
        "inputInfo": {"heat_source": {"type": "fvSourcePar", "fvSourceName": "source2", "indices": [0, 6], "components": ["solver", "function"]}},
        "normalizeStates": dict(NORM), "adjEqnOption": {"printInfo": 0},
    }
    D = PYDAFOAM(options=daOptions, case=case)
    g = geom("bump")
    S = HS.Sources(g, daOptions["fvSource"])
    val = np.array([0.3, 0.045])
    D.set_solver_input({"heat_source": val})
    p = S.entries["source2"]["pars"].copy()
    p[[0, 6]] = val
    assert rel(D.solver.getFvSource(), np.real(S.field(g, {"source2": p}))) <= 1e-12
    psi = np.random.default_rng(3).standard_normal(g.nC)
    prod = np.ones(2)
    D.solverAD.calcJacTVecProduct("heat_source", "fvSourcePar", val, "residuals", "residual", psi, prod)
    ref = [np.imag(psi @ HS.residual(case, g, case.states, S, pars={"source2": p + 1e-30j * np.eye(9)[i]})) / 1e-30 for i in (0, 6)]
    print("reference dictionary: product", prod, "complex step", ref)
    assert prod[0] == 0.0 and ref[0] == 0.0  # the centre of a snapped source is not read
    assert ref[1] != 0.0 and abs(prod[1] - ref[1]) <= 1e-10 * abs(ref[1])

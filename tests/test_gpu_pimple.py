"""DAPimpleFoam on the device: the residual with the time-derivative terms, the state Jacobians and the products that see them through
body_cell, the hand-written old-time product das_calc_drdwold_t_psi, the marching Newton primal and the time-accurate adjoint - against the
numpy restatement (tests/pimple_residual.py) and its complex step.  Bars (tests/README_actuator_disk.md): 1e-12 relative to the block's
maximum for values, 1e-10 for tangents and products; "bitwise" is np.array_equal.  Every measured number: tests/README_pimple.md.
Constructing the solver fails without the feature, so every case here does."""
import functools

import numpy as np
import pytest

import actuator_disk_restatement as AD
from dafoam_amd.meshgen import channel_case, pimple_case
from pimple_cases import DELTA_T, NORM, SCHEMES, blocks, geom, old_states, options, pimple_case_of, rel, scales, steady_case
from pimple_residual import ddt_coeffs, pimple_residual

pytestmark = pytest.mark.gpu

UNNORMALISED = {"normalizeResiduals": ["TRes"]}
GPU_MESHES = ("small", "mixed")  # 120 and 148 cells


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=options(**extra), case=case)


def at(D, mesh, ti):
    """the solver at the states of the case with the two old levels of tests/pimple_cases.py, at time index ti"""
    W0, W00 = old_states(mesh)
    D.solver.setTime(ti * DELTA_T, ti)
    D.solver.setOldTimeStates(W0, W00, ti)
    return steady_case(mesh).states, W0, W00


def columns(g, rng):
    """the U, p and nuTilda states of three cells, a face, and six random ones"""
    N = g.nC
    cells = (0, N // 2, N - 1)
    cols = [3 * c + k for c in cells for k in range(3)] + [3 * N + c for c in cells] + [4 * N + c for c in cells] + [5 * N + g.nIF // 2]
    return np.array(cols + list(rng.integers(0, 5 * N + g.nF, 6)))


def old_product_reference(case, g, W, W0, W00, ti, level, psi, s, cols, **kw):
    out = np.zeros(len(cols))
    for i, j in enumerate(cols):
        e = np.zeros(W.size, dtype=complex)
        e[j] = 1e-30j
        R = pimple_residual(case, g, W, W0 + e if level == 1 else W0, W00 + e if level == 2 else W00, time_index=ti, **kw)
        out[i] = s[j] * float(psi @ (np.imag(R) / 1e-30))
    return out


# ---- the residual ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("scheme,ti", SCHEMES)
@pytest.mark.parametrize("mesh", GPU_MESHES)
def test_residual(mesh, scheme, ti, normalized):
    case, g = pimple_case_of(mesh, scheme), geom(mesh)
    D = make(case, amd={"pcUpwindBlend": 0.5}, **({} if normalized else UNNORMALISED))
    W, W0, W00 = at(D, mesh, ti)
    kw = {} if normalized else dict(normalize=("TRes",))
    R, Rpc = np.zeros(W.size), np.zeros(W.size)
    D.solver.getResiduals(R)
    D.solver.calcResiduals(1, Rpc)
    ref, ref_pc = pimple_residual(case, g, W, W0, W00, time_index=ti, **kw), pimple_residual(case, g, W, W0, W00, time_index=ti, isPC=True, pc_blend=0.5, **kw)
    errs = {k: (rel(R[sl], ref[sl]), rel(Rpc[sl], ref_pc[sl])) for k, sl in blocks(g).items()}
    print(mesh, scheme, ti, "normalised" if normalized else "not normalised", errs)
    assert max(max(e) for e in errs.values()) <= 1e-12
    if (scheme, ti) == ("backward", 1):  # exactly Euler, whatever W00 holds
        De = make(pimple_case_of(mesh, "Euler"), **({} if normalized else UNNORMALISED))
        De.solver.setOldTimeStates(W0, None, 1)
        Re = np.zeros(W.size)
        De.solver.getResiduals(Re)
        assert np.array_equal(R, Re)


# ---- what the body gives for free -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", GPU_MESHES)
def test_state_products_and_jacobian_entries(mesh):
    from dafoam_amd.pyDASolvers import Mat

    case, g = pimple_case_of(mesh, "backward"), geom(mesh)
    D = make(case)
    W, W0, W00 = at(D, mesh, 3)
    s = scales(g)
    rng = np.random.default_rng(3)
    psi, v = rng.standard_normal(W.size), rng.standard_normal(W.size)
    Jv, JTpsi = np.zeros(W.size), np.zeros(W.size)
    D.solver.calcJacVecProduct(v, Jv)
    ref_Jv = np.imag(pimple_residual(case, g, W + 1e-30j * s * v, W0, W00, time_index=3)) / 1e-30
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "residuals", "residual", psi, JTpsi)
    errs = {k: rel(Jv[sl], ref_Jv[sl]) for k, sl in blocks(g).items()}
    dot = abs(float(v @ JTpsi) - float(psi @ ref_Jv)) / abs(float(psi @ ref_Jv))
    print(mesh, "dRdW v", errs, "v . dRdW^T psi against psi . dRdW v", dot)
    assert max(errs.values()) <= 1e-10 and dot <= 1e-10
    M = Mat().create()
    D.solver.calcdRdWT(0, M, mode=1)
    A = M.to_scipy().tocsr()
    cols = columns(g, rng)
    worst = 0.0
    for j in cols:
        e = np.zeros(W.size, dtype=complex)
        e[j] = 1e-30j
        col = s[j] * np.imag(pimple_residual(case, g, W + e, W0, W00, time_index=3)) / 1e-30
        worst = max(worst, rel(np.asarray(A[j].todense()).ravel(), col))
        assert abs(JTpsi[j] - float(psi @ col)) <= 1e-10 * np.abs(JTpsi).max()
    # the time derivative is in the entries: the diagonal of a U state carries c / dt = 1.5 / dt
    print(mesh, "entries of dRdWT at", len(cols), "columns", worst, "diagonal of U_x(0)", A[0, 0] / s[0], "c / dt", 1.5 / DELTA_T)
    assert worst <= 1e-10 and A[0, 0] / s[0] > 1.5 / DELTA_T


# ---- the old-time product -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize_states", [True, False])
@pytest.mark.parametrize("scheme,ti", SCHEMES)
@pytest.mark.parametrize("mesh", GPU_MESHES)
def test_old_time_product(mesh, scheme, ti, normalize_states):
    case, g = pimple_case_of(mesh, scheme), geom(mesh)
    D = make(case, **({} if normalize_states else {"normalizeStates": {}}))
    W, W0, W00 = at(D, mesh, ti)
    s = scales(g, NORM if normalize_states else None)
    rng = np.random.default_rng(5)
    psi = rng.standard_normal(W.size)
    cols = np.arange(W.size) if mesh == "small" else columns(g, rng)
    b = blocks(g)
    for level in (1, 2):
        a, a2 = np.zeros(W.size), np.ones(W.size)
        D.solverAD.calcdRdWOldTPsiAD(level, psi, a)
        D.solverAD.calcdRdWOldTPsiAD(level, psi, a2)
        assert np.array_equal(a, a2)
        if level == 2 and ddt_coeffs(scheme, ti)[2] == 0.0:
            assert not a.any()  # Euler, and backward at its first step
            continue
        ref = old_product_reference(case, g, W, W0, W00, ti, level, psi, s, cols)
        print(mesh, scheme, ti, "states scaled" if normalize_states else "states plain", "level", level, rel(a[cols], ref))
        assert np.abs(ref).max() > 0 and rel(a[cols], ref) <= 1e-10
        assert not a[b["p"]].any() and not a[b["phi"]].any()
        # seeds on the p and phi rows alone reach U0 through H, and only through H
        q = psi.copy()
        q[b["U"]] = 0.0
        q[b["nuTilda"]] = 0.0
        ah = np.zeros(W.size)
        D.solverAD.calcdRdWOldTPsiAD(level, q, ah)
        ucols = cols[cols < 3 * g.nC]
        refh = old_product_reference(case, g, W, W0, W00, ti, level, q, s, ucols)
        print("   seeds on p and phi only:", rel(ah[ucols], refh), "smallest |U0 entry|", np.abs(ah[b["U"]]).min())
        assert np.abs(ah[b["U"]]).min() > 0 and not ah[b["nuTilda"]].any() and rel(ah[ucols], refh) <= 1e-10


def test_old_time_product_not_normalised():
    case, g = pimple_case_of("mixed", "backward"), geom("mixed")
    D = make(case, **UNNORMALISED)
    W, W0, W00 = at(D, "mixed", 3)
    s = scales(g)
    rng = np.random.default_rng(8)
    psi = rng.standard_normal(W.size)
    cols = columns(g, rng)
    for level in (1, 2):
        a = np.zeros(W.size)
        D.solverAD.calcdRdWOldTPsiAD(level, psi, a)
        ref = old_product_reference(case, g, W, W0, W00, 3, level, psi, s, cols, normalize=("TRes",))
        print("not normalised, level", level, rel(a[cols], ref))
        assert rel(a[cols], ref) <= 1e-10


# ---- volCoord and patchVelocity ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walled():
    """channel_case(6, 5, 4) with walls at front and back: a corner point then moves on walls, not on a symmetry plane, whose points the
    product's dual metrics and the restatement treat differently (tests/actuator_disk_cases.py)"""
    case = channel_case(6, 5, 4, side_walls=True)
    case.solver_name, case.ddt_scheme, case.deltaT, case.n_steps = "DAPimpleFoam", "backward", DELTA_T, 6
    return case


def test_vol_coord_product():
    case = walled()
    m = case.mesh
    W = case.states
    rng = np.random.default_rng(9)
    W0, W00 = W * (1.0 + 0.05 * rng.standard_normal(W.size)), W * (1.0 + 0.05 * rng.standard_normal(W.size))
    psi = rng.standard_normal(W.size)
    by = {p.name: p for p in m.patches}
    boundary = set(int(p) for f in range(m.n_internal_faces, m.n_faces) for p in m.face_pts[m.face_ptr[f]:m.face_ptr[f + 1]])
    pts = {"corner": 0, "wall": int(m.face_pts[m.face_ptr[by["bottom"].start + 5]]),
           "interior": next(p for p in range(m.n_points // 2, m.n_points) if p not in boundary)}
    idx = [3 * p + k for p in pts.values() for k in range(3)]
    X0 = m.points.ravel().copy()
    ref = []
    for j in idx:
        X = X0.astype(np.complex128)
        X[j] += 1e-30j
        ref.append(np.imag(psi @ pimple_residual(case, AD.FlowGeom(m, X.reshape(-1, 3)), W.astype(np.complex128), W0, W00, time_index=3)) / 1e-30)
    ref = np.array(ref)
    D = make(case, inputInfo={"x": {"type": "volCoord"}}, amd={"volCoordMode": "dual"})
    D.solver.setTime(3 * DELTA_T, 3)
    D.solver.setOldTimeStates(W0, W00, 3)
    prod = np.zeros(X0.size)
    D.solverAD.calcJacTVecProduct("x", "volCoord", X0, "residuals", "residual", psi, prod)
    scale = np.abs(prod).max()
    err = np.abs(prod[idx] - ref).reshape(-1, 3).max(1) / scale
    print("volCoord:", dict(zip(pts, err)))
    assert np.abs(prod[idx] - ref).max() <= 1e-10 * scale


PATCHV = {"patchV": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y"}}


def test_patch_velocity_product():
    """dR / d[UMag, AoA] . psi against the complex step of the restatement in the patch value of the inlet velocity: d U_b / d UMag =
    (1, 0, 0) and d U_b / d AoA = UMag (0, 1, 0) pi / 180 at AoA = 0 (the limiter of linearUpwindV makes the residual non-linear in U_b:
    differences of a finite step do not meet the bar)"""
    mesh = "mixed"
    case, g = pimple_case_of(mesh, "backward"), geom(mesh)
    D = make(case, inputInfo=PATCHV)
    W, W0, W00 = at(D, mesh, 3)
    psi = np.random.default_rng(4).standard_normal(W.size)
    prod = np.zeros(2)
    D.solverAD.calcJacTVecProduct("patchV", "patchVelocity", np.array([10.0, 0.0]), "residual", "residual", psi, prod)
    inlet = next(p for p in case.mesh.patches if p.name == "inlet")
    sl = slice(inlet.start - g.nIF, inlet.start - g.nIF + inlet.size)
    ref = []
    for d in ((1.0, 0.0, 0.0), (0.0, 10.0 * np.pi / 180.0, 0.0)):
        dUb = np.zeros((g.nBF, 3), dtype=complex)
        dUb[sl] = 1e-30j * np.array(d)
        ref.append(psi @ np.imag(pimple_residual(case, g, W.astype(complex), W0, W00, time_index=3, dUb=dUb)) / 1e-30)
    ref = np.array(ref)
    print("patchVelocity:", prod, ref, np.abs(prod - ref) / np.abs(ref))
    assert np.all(np.abs(prod - ref) <= 1e-10 * np.abs(ref))


# ---- the marching primal ----------------------------------------------------------------------------------------------------------------
MARCH_DT = 5.0e-3
FORCE = lambda op, **kw: dict({"type": "force", "source": "patchToFace", "patches": ["bottom"], "directionMode": "fixedDirection", "direction": [1.0, 0.0, 0.0],
                               "scale": 1.0, "timeOp": op}, **kw)
FUNCTIONS = {"Favg": FORCE("average", nStepsFrac=1.0), "Ffinal": FORCE("final")}


@functools.lru_cache(maxsize=None)
def march_case(scheme):
    return pimple_case(8, 6, 5, ddt_scheme=scheme, deltaT=MARCH_DT, n_steps=6, perturb=0.0)


@functools.lru_cache(maxsize=None)
def marched(scheme):
    """(solver, series, info) of the 6-step march at relTol 1e-10 per step - computed once, shared, read-only"""
    D = make(march_case(scheme), function=FUNCTIONS, inputInfo=PATCHV, adjEqnOption={"gmresRelTol": 1e-12, "printInfo": 0}, primalMinResTol=1e-10)
    fail, info = D.solver.solvePrimal(maxSteps=80, relTol=1e-10)
    assert fail == 0, info
    return D, [D.solver.getTimeInstance(n) for n in range(7)], info


@pytest.mark.parametrize("scheme", ["Euler", "backward"])
def test_marching_primal_every_step_is_a_zero_of_the_restatement(scheme):
    case = march_case(scheme)
    g = AD.FlowGeom(case.mesh)
    D, series, info = marched(scheme)
    assert np.array_equal(series[0], case.states) and len(info["timeSteps"]) == 6
    for n in range(1, 7):
        first = np.linalg.norm(pimple_residual(case, g, series[n - 1], series[n - 1], series[max(n - 2, 0)], time_index=n))
        res = np.linalg.norm(pimple_residual(case, g, series[n], series[n - 1], series[max(n - 2, 0)], time_index=n)) / first
        st = info["timeSteps"][n - 1]
        print(scheme, "step", n, "Newton steps", st["steps"], "device", st["res"] / st["res0"], "restatement", res)
        assert st["res"] <= 1e-10 * st["res0"] and res <= 1e-9
        assert not np.array_equal(series[n], series[n - 1])
    if scheme == "backward":  # its first step is exactly the Euler step
        assert np.array_equal(series[1], marched("Euler")[1][1]) and not np.array_equal(series[2], marched("Euler")[1][2])
    vals = D.solver._functionTimeSteps["Ffinal"]
    assert D.solver.getTimeOpFuncVal("Ffinal") == vals[-1] and abs(D.solver.getTimeOpFuncVal("Favg") - sum(vals) / 6) <= 1e-14 * abs(vals[-1])


# ---- end to end: the time-accurate adjoint ----------------------------------------------------------------------------------------------
def diagonal_only(D):
    """calcdRdWOldTPsiAD without the H part: the diagonal scaling of psi in the U and nuTilda entries (normalised residuals)"""
    N = D._case.mesh.n_cells
    s = scales(AD.FlowGeom(D._case.mesh))

    def product(level, psi, out):
        c, c0, c00 = ddt_coeffs(D._case.ddt_scheme, D.solver._timeIndex)
        out[:] = 0.0
        for sl in (slice(0, 3 * N), slice(4 * N, 5 * N)):
            out[sl] = -((c0 if level == 1 else -c00) / MARCH_DT) * s[sl] * np.asarray(psi)[sl]

    return product


@pytest.mark.parametrize("scheme", ["Euler", "backward"])
def test_unsteady_adjoint_total_derivatives_in_the_inlet_velocity(scheme):
    """d(time-averaged force on the bottom wall) / d(inlet velocity) and d(final-time force) / d(inlet velocity) from solveUnsteadyAdjoint at
    gmresRelTol 1e-12, against central differences of the marching primal.  Protocol of tests/README_actuator_disk.md: relative steps
    1e-1 ... 1e-6, the step at which the two one-sided differences agree best, the bound ten times their disagreement.  An adjoint whose
    old-time product keeps only the diagonal misses that bound.  Measured (tests/README_pimple.md; adjoint total, central differences,
    bound, total without the H part):
      Euler    average 0.037113334877496      0.03711333487700555    1.32e-8  0.10446409255904528
      Euler    final   0.0011635401873996594  0.0011635401878529877  7.27e-9  0.03622401049151676
      backward average 0.019531355243947043   0.019531355242570318   5.91e-9  0.12984430756475546
      backward final   0.0011272774861146267  0.0011272774882824244  1.51e-9  0.03869938061183727"""
    D, series, _ = marched(scheme)
    W_start = series[0]
    x0 = np.array([10.0, 0.0])

    def values(U):
        D.solver.setSolverInput("patchV", "patchVelocity", 2, np.array([U, 0.0]))
        D.solver.updateOFFields(W_start)
        fail, info = D.solver.solvePrimal(maxSteps=80, relTol=1e-12)
        assert fail == 0, info
        return np.array([D.solver.getTimeOpFuncVal("Favg"), D.solver.getTimeOpFuncVal("Ffinal")])

    f0 = values(10.0)
    best = [None, None]
    for h in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6):
        up, dn = (values(10.0 * (1 + h)) - f0) / (10.0 * h), (f0 - values(10.0 * (1 - h))) / (10.0 * h)
        print("   step", h, "one-sided", up, dn)
        for k in range(2):
            if best[k] is None or abs(up[k] - dn[k]) < best[k][0]:
                best[k] = (abs(up[k] - dn[k]), 0.5 * (up[k] + dn[k]), h)
    assert np.all(np.abs(values(10.0) - f0) <= 1e-11 * np.abs(f0))
    for k, name in enumerate(("Favg", "Ffinal")):
        totals, fail = D.solveUnsteadyAdjoint([name], {"patchV": x0})
        total, fd, bound = totals["patchV"][0], best[k][1], 10.0 * best[k][0]
        print(scheme, name, "adjoint total", total, "central differences", fd, "relative step", best[k][2], "bound", bound, "difference", abs(total - fd))
        assert fail == 0 and fd != 0 and abs(total - fd) <= bound
        full = D.solverAD.calcdRdWOldTPsiAD
        D.solverAD.calcdRdWOldTPsiAD = diagonal_only(D)
        try:
            broken, _ = D.solveUnsteadyAdjoint([name], {"patchV": x0})
        finally:
            D.solverAD.calcdRdWOldTPsiAD = full
        print(scheme, name, "without the H part", broken["patchV"][0], "miss", abs(broken["patchV"][0] - fd), "bound", bound)
        assert abs(broken["patchV"][0] - fd) > bound

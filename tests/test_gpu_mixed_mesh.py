"""GPU tier (-m gpu) on pyramids, prisms and polyhedra: the device path on MIXED (tests/mixed_mesh.py: 148 cells with 5, 6, 10 and 16 faces,
triangles inside and on the boundary, up to 10 owned faces per cell, operator rows of 304 entries) and on its renumbered twin.  Every
test is the twin of a hex-block test of test_gpu_parity.py / test_gpu_functions*.py - the same calls, the same bounds - so a failure
here is a statement about cells that are no hexahedra.  The kernel BODIES on this mesh are checked without a GPU in
test_mixed_mesh_cpu.py; what only runs here is the launch code (k_grad_fp's second slot trip and tail tile, the graph kernels on rows of
304 entries, the colouring kernels on those nets, the level structure with interior late nodes, the geometry kernels' nv == 3 branch)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import function_restatement as FR
import function_restatement_more as FM
from common import blocks, norm_states, options, relerr
from mixed_mesh import mixed
from oracle import functions as Fn
from oracle import jacobian as J
from oracle import linear as OL
from oracle.foam_mesh import Geometry
from oracle.residual import residual

pytestmark = pytest.mark.gpu


def make(case, **extra):
    from dafoam_amd.pyDAFoam import PYDAFOAM

    return PYDAFOAM(options=options(case, **extra), case=case)


# the references are computed once per case and shared (read-only)
@functools.lru_cache(maxsize=None)
def geometry(*key):
    return Geometry(mixed(*key).mesh)


@functools.lru_cache(maxsize=None)
def oracle_mats(*key):
    case, g = mixed(*key), geometry(*key)
    sc = J.state_scales(case, g, norm_states(case))
    con = J.connectivity(case, g)
    col, _ = J.greedy_coloring(con)
    A = J.jacobian_colored(case, g, case.states, con, col, sc, mode="cs", lower_bound=0)
    return sc, con, col, A


def volume_rhs(key):
    g = geometry(*key)
    sc, _, _, A = oracle_mats(*key)
    rhs = np.zeros(A.shape[0])
    rhs[0 : 3 * g.nC : 3] = g.V
    return rhs * sc


def pc_setup(case, amd, **adj):
    from dafoam_amd.pyDASolvers import KSP, Mat

    D = make(case, amd=amd, adjEqnOption=dict({"printInfo": 0}, **adj))
    D.solver.runColoring()
    pc = Mat()
    D.solver.calcdRdWT(1, pc)
    ksp = KSP()
    D.solverAD.createMLRKSPMatrixFree(pc, ksp)
    return D, pc, ksp


def test_shape_of_the_mixed_mesh_reaches_the_paths_named_below():
    """148 cells = four full 32-cell tiles of k_grad_fp and a 20-cell tail (dual numbers: nine 16-cell tiles and a 4-cell tail); cells
    with more than 8 faces (second trip of the slot loop); more than 8 owned faces."""
    m = mixed().mesh
    nf = np.bincount(m.owner, minlength=m.n_cells) + np.bincount(m.neighbour, minlength=m.n_cells)
    assert m.n_cells == 148 and 148 % 32 == 20 and 148 % 16 == 4 and (nf > 8).sum() == 3 and nf.max() == 16
    assert np.bincount(m.owner, minlength=m.n_cells).max() == 10


def test_device_geometry_passes_equal_the_host_metrics_and_the_oracle():
    """Twin of test_device_geometry_passes_equal_the_host_metrics: k_geom_face (nv == 3 branch next to quads), k_geom_cell (5 to 16 faces)
    and k_geom_weights for moved points against the host metrics after updateOFMesh and against the oracle's Geometry."""
    case = mixed("simple", True)
    D = make(case, normalizeStates=norm_states(case))
    X = (case.mesh.points * np.array([1.0, 1.03, 0.98])).ravel()
    fg, cg = D.solver.deviceGeometry(X)
    geo0 = D.solver.geometry()
    D.solver.updateOFMesh(X)
    geo = D.solver.geometry()
    assert not np.array_equal(geo0["V"], geo["V"])
    moved = copy.copy(case.mesh)
    moved.points = X.reshape(-1, 3)
    go = Geometry(moved)
    nIF = case.mesh.n_internal_faces
    for ref in (geo, {"Sf": go.Sf.ravel(), "Cf": go.Cf.ravel(), "C": go.C.ravel(), "V": go.V, "w": go.w, "nonOrthDeltaCoeffs": go.nonOrthDeltaCoeffs,
                      "nonOrthCorr": go.nonOrthCorr.ravel(), "bDeltaCoeffs": go.bDeltaCoeffs}):
        assert relerr(fg[:, 0:3].ravel(), ref["Sf"]) < 1e-13 and relerr(fg[:, 9:12].ravel(), ref["Cf"]) < 1e-13
        assert relerr(cg[:, 0:3].ravel(), ref["C"]) < 1e-13 and relerr(cg[:, 3], ref["V"]) < 1e-13
        assert relerr(fg[:nIF, 4], ref["w"]) < 1e-12 and relerr(fg[:nIF, 5], ref["nonOrthDeltaCoeffs"]) < 1e-12
        assert np.abs(fg[:nIF, 6:9].ravel() - ref["nonOrthCorr"]).max() < 1e-12 and relerr(fg[nIF:, 5], ref["bDeltaCoeffs"]) < 1e-12
    assert np.array_equal(cg[:, 4], case.y_wall)  # frozen wall distance


@pytest.mark.parametrize("renumbered", [False, True])
@pytest.mark.parametrize("wall_function", [False, True])
@pytest.mark.parametrize("isPC", [0, 1])
def test_residual_parity_simplefoam(wall_function, isPC, renumbered):
    """Twin of test_residual_parity_simplefoam: every per-cell face loop (k_grad_fp, k_cell, k_face, k_pres) with trip counts 5, 6, 10, 16."""
    key = ("simple", wall_function, False, renumbered)
    case, g = mixed(*key), geometry(*key)
    D = make(case)
    R = np.zeros(case.states.size)
    D.solver.calcResiduals(isPC, R)
    Ro = residual(case, g, case.states, isPC=bool(isPC))
    for nm, sl in blocks(case, g):
        assert relerr(R[sl], Ro[sl]) < 1e-12, nm


@pytest.mark.parametrize("renumbered", [False, True])
def test_gradient_kernels_and_cell_face_split_agree(renumbered):
    """Twin of test_cell_face_split_kernels_equal_the_monolithic_cell_kernel, with the gradient launch switch as well: amd.gradFaceParallel
    0 (k_grad, one thread per cell) against 1 (k_grad_fp: eight lanes per cell, `s += 8` for the ninth face onward, a partial last tile;
    the renumbered twin scatters the neighbours across the tile borders), amd.cellFaceSplit 1 (k_fcoef / k_bcoef / k_cell2) against 0."""
    from dafoam_amd.pyDASolvers import Mat

    key = ("simple", True, False, renumbered)
    case, g = mixed(*key), geometry(*key)
    Ro = residual(case, g, case.states)
    out = {}
    for gfp, split in ((0, 0), (1, 0), (2, 0), (1, 1)):
        D = make(case, amd={"gradFaceParallel": gfp, "cellFaceSplit": split, "pcUpwindBlend": 0.5})
        R = np.zeros(case.states.size)
        D.solver.getResiduals(R)
        psi = np.random.default_rng(2).standard_normal(R.size)
        prod = np.zeros(R.size)
        D.solverAD.calcJacTVecProduct("states", "stateVar", case.states, "residuals", "residual", psi, prod)
        D.solver.runColoring()
        pc = Mat()
        D.solver.calcdRdWT(1, pc)
        out[(gfp, split)] = (R, prod, pc.to_scipy().tocsr())
        for nm, sl in blocks(case, g):
            assert relerr(R[sl], Ro[sl]) < 1e-12, (gfp, split, nm)
    base = out[(0, 0)]
    for k, o in out.items():
        assert relerr(o[0], base[0]) < 1e-13 and relerr(o[1], base[1]) < 1e-12, k
        assert abs(o[2] - base[2]).max() <= 1e-6 * abs(base[2]).max(), k  # finite differences of two summation orders


@pytest.mark.parametrize("gfp", [1, 2])
@pytest.mark.parametrize("wall_function", [False, True])
def test_drdwt_dual_matches_oracle_complex_step(wall_function, gfp):
    """Twin of test_drdwt_dual_matches_oracle_complex_step, default gradient launch and amd.gradFaceParallel 2 (k_grad_fp on dual numbers:
    nine 16-cell tiles and a 4-cell tail): rows of 304 entries through the graph kernels, 340-odd colours."""
    from dafoam_amd.pyDASolvers import Mat

    key = ("simple", wall_function)
    case, g = mixed(*key), geometry(*key)
    sc, con, col, A = oracle_mats(*key)
    D = make(case, jacLowerBounds={"dRdW": 0.0, "dRdWPC": 0.0}, amd={"gradFaceParallel": gfp})
    D.solver.runColoring()
    assert (D.solver.getConnectivity(0) != con).nnz == 0
    M = Mat()
    D.solver.calcdRdWT(0, M, mode=1)
    Ag = M.to_scipy()
    assert Ag.shape == A.shape
    assert np.abs((Ag - A).tocsr().data).max() <= 1e-10 * np.abs(A.data).max()
    Mp = Mat()
    D.solver.calcdRdWT(1, Mp, mode=1)
    P = J.jacobian_colored(case, g, case.states, J.connectivity(case, g, isPC=True), col, sc, mode="cs", isPC=True, lower_bound=0)
    assert np.abs((Mp.to_scipy() - P).tocsr().data).max() <= 1e-10 * np.abs(P.data).max()


def test_drdwt_pc_finite_difference_like_reference():
    """Twin of test_drdwt_pc_finite_difference_like_reference."""
    from dafoam_amd.pyDASolvers import Mat

    case, g = mixed(), geometry()
    sc = oracle_mats()[0]
    D = make(case)
    D.solver.runColoring()
    col, _ = D.solver.getColoring()
    M = Mat()
    D.solver.calcdRdWT(1, M)  # default: FD
    Pg = M.to_scipy()
    conp = J.connectivity(case, g, isPC=True)
    Po = J.jacobian_colored(case, g, case.states, conp, col.astype(np.int64), sc, mode="fd", isPC=True)
    assert np.abs((Pg - Po).tocsr().data).max() <= 1e-6 * np.abs(Po.data).max()
    Pex = J.jacobian_colored(case, g, case.states, conp, col.astype(np.int64), sc, mode="cs", isPC=True, lower_bound=0)
    assert np.abs((Pg - Pex).tocsr().data).max() <= 1e-4 * np.abs(Pex.data).max()
    assert Pg.nnz <= conp.nnz and np.all(Pg.diagonal() != 0)


@pytest.mark.parametrize("renumbered", [False, True])
def test_jac_t_vec_and_forward_jac_vec_products(renumbered):
    """Twins of test_jac_t_vec_product_and_dot_product_identity and test_forward_mode_jac_vec_product."""
    key = ("simple", False, False, renumbered)
    case, g = mixed(*key), geometry(*key)
    sc, con, col, A = oracle_mats(*key)
    W, n = case.states, A.shape[0]
    D = make(case)
    rng = np.random.default_rng(5)
    psi, v = rng.standard_normal(n), rng.standard_normal(n)
    prod = np.zeros(n)
    D.solverAD.calcJacTVecProduct("states", "stateVar", W, "residuals", "residual", psi, prod)
    assert relerr(prod, A @ psi) < 1e-11
    ref = residual(case, g, W + 1j * 1e-30 * (sc * v)).imag / 1e-30
    assert abs(psi @ ref - prod @ v) <= 1e-10 * abs(psi @ ref)
    Jv = np.zeros(n)
    D.solver.calcJacVecProduct(v, Jv)
    assert relerr(Jv, ref) < 1e-10
    assert abs(psi @ Jv - prod @ v) <= 1e-11 * np.linalg.norm(psi) * np.linalg.norm(Jv)


@pytest.mark.parametrize("kind", ["simple", "renumbered", "rho"])
def test_device_colourings_are_valid_and_the_first_fit_is_the_serial_one(kind):
    """Twins of test_device_coloring_is_the_serial_first_fit and test_speculative_device_coloring_is_valid_and_close_to_first_fit on nets
    of up to 304 columns and 340-odd colours (six 64-bit words of the per-net bitmaps).  The kernel's `m > 8` exit is not reachable from
    a mesh: the host cuts the column groups at 8 members (color_groups_from_flags) before the launch."""
    key = ("rho",) if kind == "rho" else ("simple", True, False, kind == "renumbered")
    case = mixed(*key)
    con = oracle_mats(*key)[1]
    Dd = make(case)
    Dd.solver.runColoring()
    cd, nd = Dd.solver.getColoring()
    assert (Dd.solver.getConnectivity(0) != con).nnz == 0
    assert cd.min() >= 0 and nd == cd.max() + 1 and J.validate_coloring(con, cd.astype(np.int64))
    Dh = make(case, amd={"coloringOnDevice": 0})
    Dh.solver.runColoring()
    ch, nh = Dh.solver.getColoring()
    assert nd == nh and np.array_equal(cd, ch)
    Ds = make(case, amd={"coloringAlgorithm": "speculative"})
    Ds.solver.runColoring()
    cs, ns = Ds.solver.getColoring()
    assert cs.min() >= 0 and ns == cs.max() + 1 and J.validate_coloring(con, cs.astype(np.int64))
    D2 = make(case, amd={"coloringAlgorithm": "speculative"})
    D2.solver.runColoring()
    assert np.array_equal(D2.solver.getColoring()[0], cs)
    assert ns <= 1.3 * nd + 8, (ns, nd)


def _check_level_order(S):
    nu = S["nodeUnk"]
    lev = np.repeat(np.arange(S["lvlPtr"].size - 1), np.diff(S["lvlPtr"]))
    for p in range(nu.shape[0]):
        cols = S["bcol"][S["bptr"][p] : S["bptr"][p + 1]]
        assert np.all(lev[cols[cols < p]] < lev[p]) and np.all(lev[cols[cols > p]] > lev[p])


@pytest.mark.parametrize("kind", ["simple", "renumbered", "rho"])
def test_node_block_ilu_apply_matches_oracle(kind):
    """Twin of test_node_block_ilu_apply_matches_oracle: late nodes of INTERIOR cells (4 to 10 owned faces) in the middle of the level
    structure, the late-late couplings dropped there."""
    key = ("rho",) if kind == "rho" else ("simple", False, False, kind == "renumbered")
    case = mixed(*key)
    D, pc, ksp = pc_setup(case, {"pcCoarseAggregates": 0})
    S = ksp.pcStructure()
    nu = S["nodeUnk"]
    P = pc.to_scipy().tocsr()
    n = P.shape[0]
    assert np.array_equal(np.sort(nu[nu >= 0]), np.arange(n))
    _check_level_order(S)
    x = np.random.default_rng(0).standard_normal(n)
    y = ksp.applyPC(D.solver, x)
    B = OL.NodeBlockILU.__new__(OL.NodeBlockILU)
    B.n, B.nu, B.bptr, B.bcol = n, nu, S["bptr"].astype(np.int64), S["bcol"].astype(np.int64)
    assert relerr(y, B.scalar_twin(P, node_order=np.argsort(S["natural"]))(x)) < 1e-9
    Bo = OL.NodeBlockILU(P, nu, S["bptr"], S["bcol"])
    assert relerr(y, Bo.solve(x)) < 1e-9
    nPrimary = int(np.sum(np.any((nu >= 0) & (nu < n - case.mesh.n_faces), axis=1)))
    assert Bo.dropped_pairs.size > 0 and np.all(S["natural"][Bo.dropped_pairs.ravel()] >= nPrimary)
    assert np.array_equal(y, ksp.applyPC(D.solver, x))


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4, 5, 6, 7])
def test_node_block_ilu_elimination_orders_match_oracle(order, monkeypatch):
    """Twin of test_node_block_ilu_elimination_orders_match_oracle."""
    from dafoam_amd import _capi

    monkeypatch.setenv("DAS_BILU_ORDER", str(order))
    case = mixed()
    D, pc, ksp = pc_setup(case, {"pcCoarseAggregates": 0, "pcStabilityLimit": 1e300})
    est, used = C.c_double(-1.0), C.c_int(-1)
    _capi.check(_capi.lib().das_ksp_get_pc_stability(ksp.handle, C.byref(est), C.byref(used)))
    assert used.value == order and 0.0 <= est.value < 1e12
    S = ksp.pcStructure()
    nu = S["nodeUnk"]
    P = pc.to_scipy().tocsr()
    n = P.shape[0]
    assert np.array_equal(np.sort(nu[nu >= 0]), np.arange(n))
    _check_level_order(S)
    x = np.random.default_rng(order).standard_normal(n)
    y = ksp.applyPC(D.solver, x)
    B = OL.NodeBlockILU.__new__(OL.NodeBlockILU)
    B.n, B.nu, B.bptr, B.bcol = n, nu, S["bptr"].astype(np.int64), S["bcol"].astype(np.int64)
    assert relerr(y, B.scalar_twin(P, node_order=np.argsort(S["natural"]))(x)) < 1e-9


@pytest.mark.parametrize("block,overlap,fill", [(64, 1, 1), (4096, 0, 0)])
def test_ras_ilu_apply_matches_oracle(block, overlap, fill):
    """Twin of test_ras_ilu_apply_matches_oracle: overlap rings that grow through pyramids and merged cells, 1 to 10 owned faces per cell."""
    case, g = mixed(), geometry()
    N, F = g.nC, g.nF
    D, pc, ksp = pc_setup(case, {"pcType": "ras", "pcCoarseAggregates": 0, "pcBlockCells": block, "pcFactorFP32": 0}, asmOverlap=overlap, pcFillLevel=fill)
    perm, off = ksp.blocks()
    n = perm.size
    assert sorted(perm.tolist()) == list(range(n)) and (off.size - 1 >= 2 or block > N)
    P = pc.to_scipy().tocsr()
    owned_faces = [[] for _ in range(N)]
    for f in range(F):
        owned_faces[g.own[f]].append(f)
    x = np.random.default_rng(0).standard_normal(n)
    y_o = np.zeros(n)
    for b in range(off.size - 1):
        core_states = perm[off[b] : off[b + 1]]
        core = np.zeros(N, bool)
        core[core_states[core_states < 3 * N] // 3] = True
        ext = core.copy()
        for _ in range(overlap):
            ext = ext | (g.cellCells @ ext.astype(np.int8) > 0)
        idx, own_mask = [], []
        for c in np.nonzero(ext)[0]:
            st = [3 * c, 3 * c + 1, 3 * c + 2, 3 * N + c, 4 * N + c] + [5 * N + f for f in owned_faces[c]]
            idx += st
            own_mask += [core[c]] * len(st)
        idx, own_mask = np.array(idx), np.array(own_mask)
        z = OL.ILU(P[idx][:, idx], fill=fill).solve(x[idx])
        y_o[idx[own_mask]] = z[own_mask]
    assert relerr(ksp.applyPC(D.solver, x), y_o) < 1e-9


@pytest.mark.parametrize("mode", ["additive", "deflated"])
def test_two_level_pc_apply(mode):
    """Twin of the apply part of test_two_level_pc_apply_and_iteration_gain: the aggregation of a ragged cell graph."""
    from dafoam_amd.pyDASolvers import Mat

    case, g = mixed(), geometry()
    N, nagg0 = g.nC, 6
    D, pc, ksp = pc_setup(case, {"pcCoarseAggregates": nagg0, "pcCoarseMode": mode})
    D.solverAD.initializedRdWTMatrixFree()
    nagg, agg = ksp.coarse(N)
    assert nagg == nagg0 and agg.min() == 0 and agg.max() == nagg0 - 1 and np.bincount(agg).min() >= N // nagg0 - 1
    P = pc.to_scipy().tocsr()
    n = P.shape[0]
    Z = sp.csr_matrix((np.ones(N), (3 * N + np.arange(N), agg)), shape=(n, nagg))
    Einv = np.linalg.inv((Z.T @ (P @ Z)).toarray())
    S = ksp.pcStructure()
    B = OL.NodeBlockILU(P, S["nodeUnk"], S["bptr"], S["bcol"])
    x = np.random.default_rng(1).standard_normal(n)
    cvec = Z @ (Einv @ (Z.T @ x))
    if mode == "additive":
        y_o = B.solve(x) + cvec
    else:
        Mop = Mat()
        D.solver.calcdRdWT(0, Mop, mode=1)
        y_o = B.solve(x - Mop.to_scipy() @ cvec) + cvec
    assert relerr(ksp.applyPC(D.solver, x), y_o) < 1e-9


@pytest.mark.parametrize("kind", ["mixed", "mixed_wall_function", "renumbered"])
def test_adjoint_vector_parity_simplefoam_with_the_default_options(kind):
    """Twin of test_adjoint_vector_parity_simplefoam / test_unstructured_renumbering_gpu with the LIBRARY's default options (no amd.*
    switch: node-block ILU, deflated coarse space, blended PC convection).  psi against a sparse direct solve of the oracle's complex-step
    dRdW^T, and - because cond_1 ~ 2.6e8 lets a loose psi bound hide a wrong operator - the true residual with the ORACLE's matrix."""
    from dafoam_amd.pyDAFoam import PYDAFOAM

    key = ("simple", kind == "mixed_wall_function", False, kind == "renumbered")
    case = mixed(*key)
    sc, con, col, A = oracle_mats(*key)
    rhs = volume_rhs(key)
    psi_o = spla.spsolve(A.tocsc(), rhs)
    D = PYDAFOAM(options={"solverName": case.solver_name, "normalizeStates": dict(norm_states(case)),
                          "adjEqnOption": {"gmresRelTol": 1e-12, "gmresMaxIters": 800, "printInfo": 0}}, case=case)
    psi, fail = D.solveAdjoint(rhs)
    info = D.ksp.info()
    e_psi, e_res = relerr(psi, psi_o), float(np.linalg.norm(A @ psi - rhs) / np.linalg.norm(rhs))
    print(f"{kind}: iters {info['iters']} psi rel err {e_psi:.2e} true residual {e_res:.2e}")
    assert fail == 0 and info["iters"] > 0
    assert e_psi <= 1e-6
    assert e_res <= 1e-10


@pytest.mark.parametrize("wall_function", [False, True])
def test_rhosimplefoam_residual_jacobian_adjoint(wall_function):
    """Twin of test_rhosimplefoam_residual_jacobian_adjoint (at the synthetic state): k_grad<..., true> and the compressible cell / face
    passes on 5 to 16 faces per cell."""
    from dafoam_amd.pyDASolvers import Mat

    key = ("rho", wall_function)
    case, g = mixed(*key), geometry(*key)
    D = make(case, adjEqnOption={"gmresRelTol": 1e-12, "gmresMaxIters": 800, "printInfo": 0}, jacLowerBounds={"dRdW": 0.0, "dRdWPC": 0.0})
    R = np.zeros(case.states.size)
    for pc in (0, 1):
        D.solver.calcResiduals(pc, R)
        Ro = residual(case, g, case.states, isPC=bool(pc))
        for nm, sl in blocks(case, g):
            assert relerr(R[sl], Ro[sl]) < 1e-11, (pc, nm)
    sc, con, col, A = oracle_mats(*key)
    D.solver.runColoring()
    assert (D.solver.getConnectivity(0) != con).nnz == 0
    M = Mat()
    D.solver.calcdRdWT(0, M, mode=1)
    assert np.abs((M.to_scipy() - A).tocsr().data).max() <= 1e-10 * np.abs(A.data).max()
    rhs = volume_rhs(key)
    psi, fail = D.solveAdjoint(rhs)
    e_psi, e_res = relerr(psi, spla.spsolve(A.tocsc(), rhs)), float(np.linalg.norm(A @ psi - rhs) / np.linalg.norm(rhs))
    print(f"rho wall_function={wall_function}: iters {D.ksp.info()['iters']} psi rel err {e_psi:.2e} true residual {e_res:.2e}")
    assert fail == 0 and e_psi <= 1e-6
    assert e_res <= 1e-10


SIDE = ["front", "back"]  # wall patches that hold triangles (side_walls=True)
FUNCTIONS = {
    "CD": {"type": "force", "source": "patchToFace", "patches": ["bottom", "top"] + SIDE, "directionMode": "fixedDirection", "direction": [1.0, 0.0, 0.0], "scale": 2.0},
    "PMean": {"type": "patchMean", "source": "patchToFace", "patches": SIDE, "varName": "p", "varType": "scalar", "index": 0, "scale": 1.0},
    "RMaxKS": {"type": "location", "source": "patchToFace", "patches": SIDE, "mode": "maxRadiusKS", "axis": [0.0, 0.0, 1.0], "center": [0.5, 0.5, 0.5],
               "coeffKS": 20.0, "scale": 1.0},
}


def test_functions_and_dFdW_on_wall_patches_with_triangles():
    """Twins of test_force_function_and_dFdW, of the patchMean cases of test_gpu_functions.py and of test_location_values_and_zero_state_
    derivatives, with side_walls=True so that the wall patches front / back hold the prism columns' triangles: k_fn_value / k_fn_grad
    (whose neighbour loop runs over 5 faces there) and the KS reduction k_ks_* on triangle faces."""
    from oracle.functions import force, force_gradient

    key = ("simple", True, True)
    case, g = mixed(*key), geometry(*key)
    W = case.states
    nv = np.diff(case.mesh.face_ptr)
    assert all(np.any(nv[p.start : p.start + p.size] == 3) for p in case.mesh.patches if p.name in SIDE)
    D = make(case, function=FUNCTIONS)
    sc = J.state_scales(case, g, norm_states(case))
    walls = FUNCTIONS["CD"]["patches"]
    ref = {"CD": (force(case, g, W, walls, [1, 0, 0], 2.0), force_gradient(case, g, W, walls, [1, 0, 0], 2.0, sc), 1e-12),
           "PMean": (FR.patch_mean(case, g, W, FUNCTIONS["PMean"]), Fn.gradient(lambda Wp: FR.patch_mean(case, g, Wp, FUNCTIONS["PMean"]), W, sc), 1e-12),
           "RMaxKS": (FM.location(case, g, W, FUNCTIONS["RMaxKS"], None), np.zeros(W.size), 1e-12)}
    for name, (Fo, dFo, tol) in ref.items():
        F1, F2 = D.solver.calcFunction(name), D.solver.calcFunction(name)
        assert F1 == F2 and Fo != 0.0 and abs(F1 - Fo) <= tol * abs(Fo), (name, F1, Fo)
        dF = np.ones(W.size)
        D.solverAD.calcJacTVecProduct("states", "stateVar", W, name, "function", np.array([1.0]), dF)
        if name == "RMaxKS":
            assert np.all(dF == 0.0)
        else:
            assert dFo.any() and np.abs(dF - dFo).max() <= 1e-10 * np.abs(dFo).max(), name


@pytest.mark.parametrize("mode", ["dual", "fd"])
def test_volcoord_full_product_vector_on_the_device(mode):
    """Twin of test_volcoord_full_product_vector_on_the_device, checks (1) to (4): single entries against difference quotients of the
    oracle on meshes with one moved point - the five apex points (only triangles touch them), points of the merged cells and of the
    prism columns, wall points - the contraction with a displacement field, bit-reproducibility, and the state left behind."""
    from oracle.functions import force

    case = mixed()
    W = case.states
    walls, d = ["bottom", "top"], [1.0, 0.0, 0.0]
    fns = {"CD": {"type": "force", "source": "patchToFace", "patches": walls, "directionMode": "fixedDirection", "direction": d, "scale": 1.0}}
    D = make(case, function=fns, amd={"volCoordMode": mode})
    S = D.solverAD
    mm = case.mesh
    n, nP, P3 = W.size, mm.n_points, 3 * mm.n_points
    rng = np.random.default_rng(3)
    seeds = rng.standard_normal(n)
    X0 = mm.points.ravel().copy()
    R0 = np.zeros(n)
    S.getResiduals(R0)
    assert S.getInputSize("x", "volCoord") == P3
    pR = np.zeros(P3)
    S.calcJacTVecProduct("x", "volCoord", X0, "residual", "residual", seeds, pR)
    info = S._volCoordInfo
    assert info["passes"] == (3 if mode == "dual" else 6) * info["colors"]
    pF = np.zeros(P3)
    S.calcJacTVecProduct("x", "volCoord", X0, "CD", "function", np.ones(1), pF)
    X, R1 = np.zeros(P3), np.zeros(n)
    S.getOFMeshPoints(X)
    S.getResiduals(R1)
    assert np.array_equal(X, X0) and np.array_equal(R0, R1)
    pR2 = np.zeros(P3)
    S.calcJacTVecProduct("x", "volCoord", X0, "residual", "residual", seeds, pR2)
    assert np.array_equal(pR, pR2)
    # the influence set of every point holds every cell that uses it (apex points: the six pyramids)
    inf = S.pointInfluence()
    steps = inf["steps"]
    touched = [set() for _ in range(nP)]
    for f in range(mm.n_faces):
        cells = {int(mm.owner[f])} | ({int(mm.neighbour[f])} if f < mm.n_internal_faces else set())
        for p in mm.face_pts[mm.face_ptr[f] : mm.face_ptr[f + 1]]:
            touched[p] |= cells
    for p in range(nP):
        assert touched[p] <= set(inf["cells"][inf["ptr"][p] : inf["ptr"][p + 1]].tolist()), p
    apex = list(range(nP - 5, nP))
    assert all(len(touched[p]) == 6 for p in apex)
    def patch_points(select):
        return np.unique(np.concatenate([mm.face_pts[mm.face_ptr[f] : mm.face_ptr[f + 1]] for pt in mm.patches if select(pt)
                                         for f in range(pt.start, pt.start + pt.size)]))

    # no point of a symmetry plane: basicSymmetry's snGradTransformDiag is |n_k|, a kink at n_k = 0 (all of `front`, and the middle row
    # of `back` faces for an odd ny, have such a component): tilting the face has two one-sided derivatives there - the device's dual
    # numbers take one, a central difference averages the two (test_dual_number_metrics_give_the_exact_mesh_derivative keeps the planes
    # planar for the same reason)
    sym_pts = patch_points(lambda pt: pt.type == "symmetry")
    inner_pts = np.setdiff1d(np.arange(nP - 5), sym_pts)
    wall_pts = np.setdiff1d(patch_points(lambda pt: pt.name in walls), sym_pts)
    pick = apex + list(rng.choice(inner_pts, 5, replace=False)) + list(rng.choice(wall_pts, 4, replace=False))
    scaleR, scaleF = np.abs(pR).max(), np.abs(pF).max()

    def oracle_fd(p, ax, h):
        vals = []
        for sgn in (1.0, -1.0):
            c2 = copy.copy(case)
            c2.mesh = copy.copy(mm)
            Xp = mm.points.copy()
            Xp[p, ax] += sgn * h
            c2.mesh.points = Xp
            g2 = Geometry(c2.mesh)
            vals.append(np.array([seeds @ residual(c2, g2, W), force(c2, g2, W, walls, d)]))
        return (vals[0] - vals[1]) / (2 * h)

    for p in pick:
        for ax in range(3):
            if mode == "fd":
                refR, refF = oracle_fd(p, ax, steps[p])
                tolr, tols = 1e-8, 1e-9
            else:
                refR, refF = oracle_fd(p, ax, 0.02 * steps[p])
                tolr, tols = 1e-5, 1e-6
            assert abs(pR[3 * p + ax] - refR) <= tolr * abs(refR) + tols * scaleR, (p, ax, pR[3 * p + ax], refR)
            assert abs(pF[3 * p + ax] - refF) <= tolr * abs(refF) + tols * scaleF, (p, ax, pF[3 * p + ax], refF)
    assert np.abs(pR.reshape(-1, 3)[apex]).max() > 0 and 0 < np.count_nonzero(pF) < P3
    Xr = mm.points
    dX = np.stack([0.3 * np.sin(3 * Xr[:, 1] / 0.2) * Xr[:, 0], 0.2 * Xr[:, 0] * (1 - Xr[:, 0]) + 0 * Xr[:, 1], 0.1 * np.cos(2 * Xr[:, 0])], axis=1).ravel()
    dirR = S.calcVolCoordDirectionalProduct(dX, "residual", "residual", seeds, eps=1e-6)
    assert abs(pR @ dX - dirR) <= (1e-6 if mode == "fd" else 1e-4) * np.abs(pR * dX).sum(), (pR @ dX, dirR)


@pytest.mark.parametrize("wall_function", [False, True])
def test_simple_sweeps_on_the_device_equal_the_oracle(wall_function):
    """Twin of part (a) of test_simple_sweeps_on_the_device_equal_the_oracle_and_reach_the_newton_fixed_point: k_simple_* and k_ldu_mv
    with 5 to 16 faces per cell, 1 and 3 sweeps against oracle.primal.simple_iteration."""
    from oracle.primal import simple_iteration

    key = ("simple", wall_function)
    case, g = mixed(*key), geometry(*key)
    Wo = [case.states.copy()]
    for _ in range(3):
        Wo.append(simple_iteration(case, g, Wo[-1]))
    for ns in (1, 3):
        D = make(case)
        info = D.solver.simpleIteration(ns, alphaP=0.3, linTol=1e-13)
        assert info["U"] > 0 and info["p"] > 0
        W = np.zeros(case.states.size)
        D.solver.getOFFields(W)
        for nm, sl in blocks(case, g):
            assert relerr(W[sl], Wo[ns][sl]) < 1e-9, (nm, ns)

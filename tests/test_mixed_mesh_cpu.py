"""CPU tier on pyramids, prisms and polyhedra (tests/mixed_mesh.py): the mixed-cell generator itself, the library's host code (metrics,
connectivity, colouring, node structure of the block ILU) and the kernel bodies through the host-emulation harness, each against the
face-based oracle.  Twins of the hex-block tests of test_host_cpu.py / test_oracle_cpu.py with the same bounds; no GPU compute here."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse.linalg as spla

from common import NORM_STATES, blocks, norm_states, options, relerr
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import channel_case, renumber_case, scalar_transport_case
from dafoam_amd.pyDASolvers import pyDASolvers
from mixed_mesh import MIXED, MIXED_RENUMBERED, mixed
from oracle import jacobian as J
from oracle import linear as OL
from oracle.foam_mesh import Geometry
from oracle.residual import residual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _emu():
    L = C.CDLL(os.path.join(ROOT, "tests", "hostemu", "libhostemu.so"))
    L.emu_residual.argtypes = [C.POINTER(das_case_t), _capi.c_double_p, C.c_longlong, C.c_int, _capi.c_double_p, _capi.c_double_p, _capi.c_double_p]
    return L


def _emu_res(case, W, isPC=0, d=None):
    cs = CaseStruct(case)
    n = W.size
    Rv, Rd = np.zeros(n), np.zeros(n)
    rc = _emu().emu_residual(cs.byref(), dptr(W), n, isPC, dptr(d) if d is not None else None, dptr(Rv), dptr(Rd))
    assert rc == 0
    return Rv, Rd


@functools.lru_cache(maxsize=None)
def geometry(kind="simple"):
    return Geometry(mixed(kind).mesh)


def _faces_per_cell(mesh):
    N = mesh.n_cells
    return np.bincount(mesh.owner, minlength=N) + np.bincount(mesh.neighbour, minlength=N)


def _interior_cells(mesh):
    inner = np.ones(mesh.n_cells, bool)
    inner[mesh.owner[mesh.n_internal_faces :]] = False
    return inner


# ---- the generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["simple", "rho", "scalar"])
def test_mixed_cell_generator_emits_a_valid_polymesh(kind):
    """Closed cells, positive volumes, OpenFOAM's face order, the patch table of the hex block, and the shape facts the later tests rely
    on: 5, 6, 10 and 16 faces per cell, triangles inside and on the boundary, an interior cell that owns >= 4 faces.  The weights and the
    non-orthogonality stay away from the clamps, so that no comparison sits on a non-smooth switch (conditions on the input)."""
    case = mixed(kind)
    base = {"simple": channel_case, "rho": channel_case, "scalar": scalar_transport_case}[kind](6, 5, 4)
    mesh, g = case.mesh, geometry(kind)
    N, F, nIF = mesh.n_cells, mesh.n_faces, mesh.n_internal_faces
    assert (N, F) == (148, 506) and mesh.face_ptr.size == F + 1 and mesh.face_ptr[-1] == mesh.face_pts.size
    clo = np.zeros((N, 3))
    np.add.at(clo, g.own, g.Sf)
    np.add.at(clo, g.nei, -g.Sf[:nIF])
    assert np.abs(clo).max() <= 1e-13 * g.magSf.max()
    # the same domain (up to the four warped `back` quads of the prism columns, now two flat triangles each)
    assert np.all(g.V > 0) and abs(g.V.sum() - Geometry(base.mesh).V.sum()) <= 1e-4 * g.V.sum()
    own, nei = mesh.owner[:nIF].astype(np.int64), mesh.neighbour.astype(np.int64)
    assert np.all(nei > own)
    key = own * N + nei
    assert np.all(np.diff(key) > 0)  # upper-triangular order and no cell pair twice
    assert np.all(np.einsum("ij,ij->i", g.Sf[:nIF], g.C[nei] - g.C[own]) > 0)  # owner -> neighbour
    assert [(p.name, p.type) for p in mesh.patches] == [(p.name, p.type) for p in base.mesh.patches]
    assert mesh.patches[0].start == nIF and all(a.start + a.size == b.start for a, b in zip(mesh.patches[:-1], mesh.patches[1:]))
    assert mesh.patches[-1].start + mesh.patches[-1].size == F
    nf = _faces_per_cell(mesh)
    assert {5, 6, 10, 16} <= set(nf.tolist()) and np.array_equal(np.bincount(nf)[[5, 6, 10, 16]], [46, 99, 2, 1])
    nv = np.diff(mesh.face_ptr)
    assert set(nv.tolist()) == {3, 4} and (nv[:nIF] == 3).sum() == 72 and (nv[nIF:] == 3).sum() == 8
    owned = np.bincount(mesh.owner, minlength=N)
    assert owned[_interior_cells(mesh)].max() >= 4 and {8, 9, 10} <= set(owned.tolist())
    assert 0.15 <= g.w.min() and g.w.max() <= 0.85
    assert (g.deltaCoeffs / g.nonOrthDeltaCoeffs).min() >= 0.2  # n.d / |d|: the 0.05 clamp of nonOrthDeltaCoeffs is never active
    if kind != "scalar":  # no two neighbours with the same velocity: U_N - U_P = 0 is the kink of the linearUpwindV limiter
        U = case.states[: 3 * N].reshape(N, 3)
        assert np.linalg.norm(U[nei] - U[own], axis=1).min() >= 1e-4 * np.linalg.norm(U, axis=1).max()
    assert np.isfinite(residual(case, g, case.states)).all()


def test_side_walls_put_triangles_on_wall_patches():
    mesh = mixed("simple", True, True).mesh
    nv = np.diff(mesh.face_ptr)
    tri_patches = {p.name for p in mesh.patches if np.any(nv[p.start : p.start + p.size] == 3)}
    assert tri_patches == {"front", "back"} and all(p.type == "wall" for p in mesh.patches if p.name in tri_patches)


def _renumber_case_hex_only(case, seed):
    """renumber_case as it was when every face had to have the same vertex count (the permutation, the orientation rule and the state
    blocks restated with a (F, k) face table) - the generalisation to ragged faces must not change a bit on hex cases."""
    m = case.mesh
    N, F, nIF = m.n_cells, m.n_faces, m.n_internal_faces
    new_of_old = np.random.default_rng(seed).permutation(N)
    o, n = new_of_old[m.owner[:nIF]], new_of_old[m.neighbour]
    flip = o > n
    no, nn = np.where(flip, n, o), np.where(flip, o, n)
    order = np.lexsort((nn, no))
    fp = m.face_pts.reshape(F, -1).copy()
    fp[:nIF][flip] = fp[:nIF][flip][:, ::-1]
    face_perm = np.concatenate([order, np.arange(nIF, F)])
    old_of_new = np.argsort(new_of_old)
    sign = np.ones(F)
    sign[:nIF] = np.where(flip[order], -1.0, 1.0)
    W = case.states
    if case.solver_name == "DASimpleFoam":
        W = np.concatenate([W[: 3 * N].reshape(N, 3)[old_of_new].ravel(), W[3 * N : 4 * N][old_of_new], W[4 * N : 5 * N][old_of_new], W[5 * N :][face_perm] * sign])
    else:
        W = W[old_of_new]
    return {"face_ptr": m.face_ptr, "face_pts": fp[face_perm].ravel(), "owner": np.concatenate([no[order], new_of_old[m.owner[nIF:]]]),
            "neighbour": nn[order], "states": W, "y_wall": None if case.y_wall is None else case.y_wall[old_of_new],
            "phi": None if case.phi is None else case.phi[face_perm] * sign, "T_old": None if case.T_old is None else case.T_old[old_of_new]}


@pytest.mark.parametrize("kind", ["simple", "scalar"])
def test_renumber_case_is_unchanged_on_hex_cases(kind):
    base = channel_case(6, 5, 4, wall_function=True) if kind == "simple" else scalar_transport_case(5, 4, 3)
    out, ref = renumber_case(base, seed=3), _renumber_case_hex_only(base, 3)
    for nm in ("face_ptr", "face_pts", "owner", "neighbour"):
        a = getattr(out.mesh, nm)
        assert a.dtype == np.int32 and np.array_equal(a, ref[nm]), nm
    assert np.array_equal(out.mesh.points, base.mesh.points)
    for nm in ("states", "y_wall", "phi", "T_old"):
        a = getattr(out, nm)
        assert (a is None and ref[nm] is None) or np.array_equal(a, ref[nm]), nm


@pytest.mark.parametrize("kind", ["simple", "rho", "scalar"])
def test_renumbered_mixed_mesh_has_the_permuted_residual(kind):
    """renumber_case on ragged faces: each flipped face has its own vertex slice reversed.  The oracle residual of the renumbered case is
    the residual of the original one, rows permuted (cells) / permuted and signed (faces)."""
    base = mixed(kind)
    case = renumber_case(base, seed=5)
    m0, m1 = base.mesh, case.mesh
    N, F, nIF = m0.n_cells, m0.n_faces, m0.n_internal_faces
    assert np.all(m1.neighbour > m1.owner[:nIF]) and np.array_equal(np.sort(np.diff(m1.face_ptr)), np.sort(np.diff(m0.face_ptr)))
    new_of_old = np.random.default_rng(5).permutation(N)
    old_of_new = np.argsort(new_of_old)
    g0, g1 = geometry(kind), Geometry(m1)
    assert np.abs(g1.V - g0.V[old_of_new]).max() <= 1e-15 * g0.V.max() and np.abs(g1.C - g0.C[old_of_new]).max() < 1e-15
    R0, R1 = residual(base, g0, base.states), residual(case, g1, case.states)
    if kind == "scalar":
        assert relerr(R1, R0[old_of_new]) < 1e-13
        return
    # old face of every new face, and its orientation, from the cell pair
    pair = {(int(a), int(b)): f for f, (a, b) in enumerate(zip(m0.owner[:nIF], m0.neighbour))}
    fold, sign = np.arange(F), np.ones(F)
    for f in range(nIF):
        a, b = int(old_of_new[m1.owner[f]]), int(old_of_new[m1.neighbour[f]])
        fold[f], sign[f] = (pair[(a, b)], 1.0) if (a, b) in pair else (pair[(b, a)], -1.0)
    nsc = (base.states.size - 3 * N - F) // N
    assert relerr(R1[: 3 * N].reshape(N, 3), R0[: 3 * N].reshape(N, 3)[old_of_new]) < 1e-13
    for b in range(nsc):
        assert relerr(R1[(3 + b) * N : (4 + b) * N], R0[(3 + b) * N : (4 + b) * N][old_of_new]) < 1e-13, b
    assert relerr(R1[(3 + nsc) * N :], R0[(3 + nsc) * N :][fold] * sign) < 1e-13
    if kind == "simple":
        assert np.array_equal(case.states, MIXED_RENUMBERED.states) and np.array_equal(m1.face_pts, MIXED_RENUMBERED.mesh.face_pts)


# ---- host code of the library vs the oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["simple", "rho"])
def test_mesh_metrics_connectivity_and_colouring_match_oracle_on_the_mixed_mesh(kind):
    """Twin of test_mesh_metrics_connectivity_and_colouring_match_oracle: geom_face's nv == 3 branch, every per-cell face loop of the
    host metrics and of the connectivity builder with 5, 10 and 16 faces, rows of 304 entries."""
    case, g = mixed(kind), geometry(kind)
    s = pyDASolvers((case.solver_name + " -python").encode(), options(case), case=case)
    geo = s.geometry()
    assert np.abs(geo["Sf"].reshape(-1, 3) - g.Sf).max() < 1e-15
    assert np.abs(geo["C"].reshape(-1, 3) - g.C).max() < 1e-13
    assert relerr(geo["V"], g.V) < 1e-13 and relerr(geo["w"], g.w) < 1e-13
    assert relerr(geo["nonOrthDeltaCoeffs"], g.nonOrthDeltaCoeffs) < 1e-12
    assert np.abs(geo["nonOrthCorr"].reshape(-1, 3) - g.nonOrthCorr).max() < 1e-11
    assert relerr(geo["bDeltaCoeffs"], g.bDeltaCoeffs) < 1e-12
    assert s.getNLocalAdjointStates() == case.states.size
    s.runColoring()
    for pc in (0, 1):
        assert (s.getConnectivity(pc) != J.connectivity(case, g, isPC=bool(pc))).nnz == 0
    col, nc = s.getColoring()
    con = J.connectivity(case, g)
    assert J.validate_coloring(con, col.astype(np.int64)) and nc == col.max() + 1
    if kind == "simple":
        assert np.diff(con.tocsr().indptr).max() == 304


# ---- kernel bodies through the host-emulation harness ----------------------------------------------------------------------
@pytest.mark.parametrize("wall_function", [False, True])
@pytest.mark.parametrize("isPC", [0, 1])
def test_kernel_bodies_match_oracle_simplefoam_on_the_mixed_mesh(wall_function, isPC):
    case = mixed("simple", wall_function)
    g = geometry()
    W = case.states
    Ro = residual(case, g, W, isPC=bool(isPC))
    Rv, _ = _emu_res(case, W, isPC)
    for nm, sl in blocks(case, g):
        assert relerr(Rv[sl], Ro[sl]) < 1e-12, nm
    v = np.random.default_rng(3).standard_normal(W.size) * J.state_scales(case, g, NORM_STATES)
    cs = residual(case, g, W + 1j * 1e-30 * v, isPC=bool(isPC)).imag / 1e-30
    _, Rd = _emu_res(case, W, isPC, v)
    for nm, sl in blocks(case, g):
        assert relerr(Rd[sl], cs[sl]) < 1e-10, nm


@pytest.mark.parametrize("wall_function", [False, True])
@pytest.mark.parametrize("isPC", [0, 1])
def test_kernel_bodies_match_oracle_rhosimplefoam_on_the_mixed_mesh(wall_function, isPC):
    case = mixed("rho", wall_function)
    g = geometry("rho")
    W = case.states
    Ro = residual(case, g, W, isPC=bool(isPC))
    Rv, _ = _emu_res(case, W, isPC)
    for nm, sl in blocks(case, g):
        assert relerr(Rv[sl], Ro[sl]) < 1e-11, nm
    v = np.random.default_rng(3).standard_normal(W.size) * J.state_scales(case, g, norm_states(case))
    cs = residual(case, g, W + 1j * 1e-30 * v, isPC=bool(isPC)).imag / 1e-30
    _, Rd = _emu_res(case, W, isPC, v)
    for nm, sl in blocks(case, g):
        assert relerr(Rd[sl], cs[sl]) < 1e-10, nm


def test_face_cell_split_of_the_cell_pass_equals_the_monolith_and_the_oracle_on_the_mixed_mesh():
    E = _emu()
    E.emu_set_pc_blend.argtypes = [C.c_double]
    E.emu_set_cell_split.argtypes = [C.c_int]
    try:
        for case in (mixed("simple", True), MIXED_RENUMBERED):
            g = Geometry(case.mesh)
            W = case.states
            v = np.random.default_rng(11).standard_normal(W.size) * J.state_scales(case, g, norm_states(case))
            for isPC, blend in ((0, 0.0), (1, 0.0), (1, 0.5)):
                E.emu_set_pc_blend(blend)
                E.emu_set_cell_split(0)
                R0, d0 = _emu_res(case, W, isPC, v)
                E.emu_set_cell_split(1)
                R1, d1 = _emu_res(case, W, isPC, v)
                Ro = residual(case, g, W, isPC=bool(isPC), pc_blend=blend if isPC else 1.0)
                for nm, sl in blocks(case, g):
                    assert relerr(R1[sl], R0[sl]) < 1e-13, (nm, isPC, blend)
                    assert relerr(d1[sl], d0[sl]) < 1e-12, (nm, isPC, blend)
                    assert relerr(R1[sl], Ro[sl]) < 1e-12, (nm, isPC, blend)
                assert not np.array_equal(R1, R0)  # the split really ran (different summation order)
    finally:
        E.emu_set_pc_blend(0.0)
        E.emu_set_cell_split(0)


# ---- node structure of the block ILU ---------------------------------------------------------------------------------------
def _structure(case):
    s = pyDASolvers((case.solver_name + " -python").encode(), options(case), case=case)
    s.runColoring()
    return s, s.pcStructure()


@pytest.mark.parametrize("kind", ["simple", "renumbered", "scalar"])
def test_pc_node_structure_levels_and_pattern_on_the_mixed_mesh(kind):
    """Twin of test_pc_node_structure_levels_and_pattern.  On hex blocks only boundary cells own more than three faces; here interior
    cells own 4 to 10, so late nodes (the face unknowns beyond a cell's first three) sit in the interior of the level structure."""
    case = MIXED_RENUMBERED if kind == "renumbered" else mixed(kind)
    s, S = _structure(case)
    nu, bptr, bcol, nat = S["nodeUnk"], S["bptr"], S["bcol"], S["natural"]
    n, nN = case.states.size, nu.shape[0]
    lev = np.repeat(np.arange(S["lvlPtr"].size - 1), np.diff(S["lvlPtr"]))
    assert np.array_equal(np.sort(nu[nu >= 0]), np.arange(n))  # every unknown in exactly one slot
    assert np.array_equal(np.sort(nat), np.arange(nN)) and lev.size == nN
    rows = np.repeat(np.arange(nN), np.diff(bptr))
    lower, upper = bcol < rows, bcol > rows
    assert np.all(lev[bcol[lower]] < lev[rows[lower]]) and np.all(nat[bcol[lower]] < nat[rows[lower]])
    assert np.all(lev[bcol[upper]] > lev[rows[upper]]) and np.all(nat[bcol[upper]] > nat[rows[upper]])
    node_of = np.empty(n, np.int64)
    node_of[nu[nu >= 0]] = np.nonzero(nu >= 0)[0]
    con = s.getConnectivity(1).tocoo()
    have = set(zip(rows.tolist(), bcol.tolist()))
    missing = [(a, b) for a, b in set(zip(node_of[con.row].tolist(), node_of[con.col].tolist())) if (a, b) not in have]
    if kind == "scalar":  # one unknown per cell, nodes of up to eight cells: no late nodes, nothing dropped
        assert not missing and (nu >= 0).sum(axis=1).max() == 8
        return
    nCellUnk = n - case.mesh.n_faces
    nPrimary = int(np.sum(np.any((nu >= 0) & (nu < nCellUnk), axis=1)))
    late = nat >= nPrimary
    assert all(late[a] and late[b] for a, b in missing)
    off = rows != bcol
    assert not np.any(late[rows[off]] & late[bcol[off]])  # no late node is coupled to another late node
    # late nodes of interior cells exist, and not only at the end of the level structure
    inner = _interior_cells(case.mesh)
    late_nodes = np.nonzero(late)[0]
    assert np.all(nu[late_nodes][nu[late_nodes] >= 0] >= nCellUnk)
    first_face = np.array([u[u >= 0][0] for u in nu[late_nodes]]) - nCellUnk
    inner_late = late_nodes[inner[case.mesh.owner[first_face]]]
    assert inner_late.size >= 5 and lev[inner_late].min() < lev.max()


@functools.lru_cache(maxsize=None)
def oracle_jacobian():
    case, g = MIXED, geometry()
    sc = J.state_scales(case, g, NORM_STATES)
    con = J.connectivity(case, g)
    col, _ = J.greedy_coloring(con)
    A = J.jacobian_colored(case, g, case.states, con, col, sc, mode="cs", lower_bound=0).tocsr()
    A.sort_indices()
    return A, sc


def test_host_node_block_ilu_matches_the_dense_block_restatement_on_the_mixed_mesh():
    """Twin of test_host_node_block_ilu_matches_the_dense_block_restatement on the node structure the library derives from the mixed mesh."""
    case, g = MIXED, geometry()
    A, sc = oracle_jacobian()
    n, N = A.shape[0], g.nC
    _, S = _structure(case)
    ref = OL.NodeBlockILU(A, S["nodeUnk"], S["bptr"].astype(np.int64), S["bcol"].astype(np.int64))
    K = OL.OmpKrylov(3)
    K.set_operator(A)
    assert K.set_pc_bilu(A, S) == 0
    b = np.random.default_rng(4).standard_normal(n)
    assert relerr(K.pc_solve(b), ref.solve(b)) < 1e-11
    rhs = np.zeros(n)
    rhs[0 : 3 * N : 3] = g.V
    rhs *= sc
    x, info = K.gmres(rhs, restart=200, max_iters=400, rel_tol=1e-11)
    assert info["fail"] == 0 and relerr(x, spla.spsolve(A.tocsc(), rhs)) < 1e-8

"""CPU tier: host logic of the product (mesh metrics, connectivity, colouring, option surface), the C-ABI
library (loads, exports every declared symbol, fails loudly without a GPU) and the kernel *bodies* run through
the host-emulation harness (tests/hostemu) against the oracle.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from common import NORM_STATES, NORM_STATES_RHO, blocks, norm_states, options, relerr, unrolled_maps
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import (channel_case, periodic_channel_case, renumber_case, rho_channel_case, scalar_transport_case, simple_T_channel_case,
                                turbo_channel_case, unroll_periodic_vector)
from dafoam_amd.pyDASolvers import pyDASolvers
from oracle import jacobian as J
from oracle.foam_mesh import Geometry
from oracle.residual import residual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAS_GPU = _capi.lib().das_device_count() > 0


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "dafoam_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(das_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_capi.declared_symbols()), declared ^ set(_capi.declared_symbols())
    L = C.CDLL(_capi.LIB_PATH)
    for name in declared:
        assert hasattr(L, name), name
    assert _capi.lib().das_version() >= 100


@pytest.mark.skipif(HAS_GPU, reason="only meaningful on a CPU-only host")
def test_compute_path_fails_loudly_without_gpu():
    case = channel_case(4, 4, 3)
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    with pytest.raises(_capi.DASError, match="no HIP device"):
        s.initSolver()
    with pytest.raises(_capi.DASError, match="das_init_solver has not been called"):
        s.getResiduals(np.zeros(s.getNLocalAdjointStates()))


@pytest.mark.parametrize("solver", ["DASimpleFoam", "DAScalarTransportFoam", "DARhoSimpleFoam"])
def test_mesh_metrics_connectivity_and_colouring_match_oracle(solver):
    case = {"DASimpleFoam": lambda: channel_case(7, 6, 5), "DAScalarTransportFoam": lambda: scalar_transport_case(6, 5, 4),
            "DARhoSimpleFoam": lambda: rho_channel_case(6, 5, 4)}[solver]()
    s = pyDASolvers((solver + " -python").encode(), options(case), case=case)
    g = Geometry(case.mesh)
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
    assert J.validate_coloring(J.connectivity(case, g), col.astype(np.int64)) and nc == col.max() + 1


def test_option_surface_and_type_checks():
    from dafoam_amd.pyDAFoam import DAOPTION, Error, PYDAFOAM

    d = DAOPTION()
    # defaults of the reference (dafoam/pyDAFoam.py:526-548, 390-392, 568-589, 608, 628)
    assert d.adjEqnOption["gmresRestart"] == 1000 and d.adjEqnOption["gmresRelTol"] == 1e-6
    assert d.adjEqnOption["pcFillLevel"] == 1 and d.adjEqnOption["asmOverlap"] == 1
    assert d.adjPartDerivFDStep == {"State": 1e-6} and d.jacLowerBounds["dRdWPC"] == 1e-30
    assert d.maxResConLv4JacPCMat["pRes"] == 2 and d.maxResConLv4JacPCMat["phiRes"] == 1
    assert d.adjStateOrdering == "state" and d.maxCorrectBCCalls == 2 and d.useConstrainHbyA is True
    case = channel_case(4, 4, 3)
    if not HAS_GPU:
        with pytest.raises(Exception):
            PYDAFOAM(options=options(case), case=case)  # init must fail loudly without a GPU
    with pytest.raises(Error):
        PYDAFOAM(options={"adjEqnOption": 3}, case=case)  # type mismatch (pyDAFoam.py:2029-2033)
    with pytest.raises(Error):
        PYDAFOAM(options={"noSuchOption": 1}, case=case)
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    with pytest.raises(_capi.DASError):
        s.updateDAOption({"adjStateOrdering": "cell"})  # the C-ABI itself only knows "state" ordering -> loud error
    # "cell" ordering at construction: handled by the Python mirror as a permutation (DAIndex.C:602-651)
    sc = pyDASolvers(b"DASimpleFoam -python", options(case, adjStateOrdering="cell"), case=case)
    perm = sc._perm
    N = case.mesh.n_cells
    assert sorted(perm.tolist()) == list(range(case.states.size))
    nown0 = int((case.mesh.owner == 0).sum())
    assert list(perm[:5]) == [0, 1, 2, 3 * N, 4 * N] and perm[5] == 5 * N + int(np.nonzero(case.mesh.owner == 0)[0][0]) and perm[5 + nown0] == 3
    xc = np.zeros(case.states.size)
    sc.getOFFields(xc)
    assert np.array_equal(xc, case.states[perm])
    v = C.c_double()
    _capi.check(_capi.lib().das_get_option_double(s._h, b"normalizeStates.U", C.byref(v)))
    assert v.value == 10.0
    x = np.zeros(s.getNLocalAdjointStates())
    s.getOFFields(x)
    assert np.array_equal(x, case.states)
    with pytest.raises(AssertionError):
        s.updateOFFields(np.zeros(3))  # invalid array size, like pyDASolvers.pyx:269


# ---- kernel bodies through the host-emulation harness ------------------------------------------------
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


@pytest.mark.parametrize("wall_function", [False, True])
@pytest.mark.parametrize("isPC", [0, 1])
def test_kernel_bodies_match_oracle_simplefoam(wall_function, isPC):
    case = channel_case(7, 7, 7, wall_function=wall_function)
    g = Geometry(case.mesh)
    W = case.states
    Ro = residual(case, g, W, isPC=bool(isPC))
    Rv, _ = _emu_res(case, W, isPC)
    for nm, sl in blocks(case, g):
        assert relerr(Rv[sl], Ro[sl]) < 1e-12, nm
    rng = np.random.default_rng(3)
    v = rng.standard_normal(W.size) * J.state_scales(case, g, NORM_STATES)
    cs = residual(case, g, W + 1j * 1e-30 * v, isPC=bool(isPC)).imag / 1e-30
    _, Rd = _emu_res(case, W, isPC, v)
    for nm, sl in blocks(case, g):
        assert relerr(Rd[sl], cs[sl]) < 1e-10, nm


def test_pc_upwind_blend_option_kernel_bodies_match_oracle():
    """amd.pcUpwindBlend (round 4): the PC residual with a partial second-order (linearUpwindV) correction - weight 0 is the
    reference's div(pc) = upwind, weight 1 the operator's scheme on the PC stencil.  Kernel bodies vs the oracle for both
    incompressible and compressible solvers, values and forward-mode tangents; the operator residual ignores the option."""
    E = _emu()
    E.emu_set_pc_blend.argtypes = [C.c_double]
    try:
        for case in (channel_case(7, 6, 5, wall_function=True), rho_channel_case(6, 6, 5)):
            g = Geometry(case.mesh)
            W = case.states
            sc = J.state_scales(case, g, norm_states(case))
            v = np.random.default_rng(5).standard_normal(W.size) * sc
            R_pc0, _ = _emu_res(case, W, 1)
            R_op, _ = _emu_res(case, W, 0)
            E.emu_set_pc_blend(0.35)
            Rv, Rd = _emu_res(case, W, 1, v)
            Ro = residual(case, g, W, isPC=True, pc_blend=0.35)
            cs = residual(case, g, W + 1j * 1e-30 * v, isPC=True, pc_blend=0.35).imag / 1e-30
            for nm, sl in blocks(case, g):
                assert relerr(Rv[sl], Ro[sl]) < 1e-12, nm
                assert relerr(Rd[sl], cs[sl]) < 1e-10, nm
            assert relerr(Rv, R_pc0) > 1e-6  # the option does something ...
            assert np.allclose(Rv, R_pc0 + 0.35 * (residual(case, g, W, isPC=True, pc_blend=1.0) - R_pc0), rtol=1e-9, atol=1e-9 * np.abs(Rv).max())  # ... linear in the weight
            assert np.array_equal(_emu_res(case, W, 0)[0], R_op)  # the operator residual does not see it
            E.emu_set_pc_blend(0.0)
    finally:
        E.emu_set_pc_blend(0.0)


def test_face_cell_split_of_the_cell_pass_equals_the_monolith_and_the_oracle():
    """Round 6 (north_star n1 / VERDICT round 5 item 4): body_cell split into a per-internal-face coefficient pass (body_fcoef), a
    per-boundary-face pass (body_bcoef) and a light per-cell pass (body_cell2).  Values and forward-mode tangents of the whole residual
    through the split equal the monolith's (rounding only) and the oracle's, for the operator residual and for the PC residual with a
    partial linearUpwindV correction, on the bump channel (all patch types, wall function) and on the NACA0012 O-grid."""
    from dafoam_amd.meshgen import naca0012_case

    E = _emu()
    E.emu_set_pc_blend.argtypes = [C.c_double]
    E.emu_set_cell_split.argtypes = [C.c_int]
    try:
        for case in (channel_case(7, 6, 5, wall_function=True), channel_case(6, 6, 6), naca0012_case(24, 8, 3, span=0.3, first_cell=1e-3)):
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
                assert not np.array_equal(R1, R0) or case.mesh.n_cells == 0  # the split really ran (different summation order)
    finally:
        E.emu_set_pc_blend(0.0)
        E.emu_set_cell_split(0)


def test_native_mesh_metrics_equal_the_numpy_input_geometry_and_the_swept_wing_is_a_valid_mesh():
    """Round 6: (a) das_mesh_metrics - the library's host geometry bodies for a bare mesh, what the input generators use from 1 M faces on -
    against the generators' numpy fan sums; (b) the swept / tapered wing segment of bench.py --naca-sweep / --naca-taper: positive volumes,
    owner -> neighbour face normals, the far field and the end planes where the unswept mesh has them, every layer its own chord."""
    from dafoam_amd.meshgen import _InputGeometry, naca0012_case

    for case in (channel_case(6, 5, 4), naca0012_case(24, 8, 3, span=0.3, first_cell=1e-3)):
        g = _InputGeometry(case.mesh)
        h = _InputGeometry.__new__(_InputGeometry)
        assert h._native(case.mesh)
        for nm, tol in (("Sf", 1e-13), ("Cf", 1e-13), ("C", 1e-12), ("V", 1e-12), ("w", 1e-9)):
            a, b = getattr(h, nm), getattr(g, nm)
            assert np.abs(a - b).max() <= tol * np.abs(b).max(), nm
    c0 = naca0012_case(40, 12, 6, span=1.2, first_cell=1e-3, perturb=0.0)
    c1 = naca0012_case(40, 12, 6, span=1.2, first_cell=1e-3, perturb=0.0, sweep_deg=25.0, taper=0.3)
    g1 = _InputGeometry(c1.mesh)
    nIF = c1.mesh.n_internal_faces
    assert np.all(g1.V > 0) and np.all(np.einsum("ij,ij->i", g1.Sf[:nIF], g1.C[c1.mesh.neighbour] - g1.C[c1.mesh.owner[:nIF]]) > 0)
    p0, p1 = c0.mesh.points, c1.mesh.points
    assert np.array_equal(p0[:, 2], p1[:, 2])                                         # the layers stay planes of constant z
    first = p0[:, 2] == 0.0
    assert np.allclose(p0[first], p1[first])                                           # the root section is the unswept one
    far = np.hypot(p0[:, 0] - 0.5, p0[:, 1]) > 19.0
    assert np.abs(p1[far] - p0[far]).max() < 0.05                                       # the far field (20 chords) hardly moves
    tip = slice(40 * 13 * 6, 40 * 13 * 6 + 40)                                          # the wall ring of the last layer of points
    chord_tip = p1[tip, 0].max() - p1[tip, 0].min()
    assert abs(chord_tip - 0.7) < 0.01 and abs(p1[tip, 0].min() - (0.25 - 0.25 * 0.7 + 1.2 * np.tan(np.deg2rad(25.0)))) < 0.01  # chord 0.7 about the swept quarter-chord line


def test_simple_sweep_bodies_equal_the_oracle_simple_iteration():
    """Round 6: the SIMPLE sweep of DASimpleFoam + SA (csrc/das_simple.hpp: momentum predictor with fvMatrix::relax, rAU /
    HbyA / constrainHbyA, pressure equation with one non-orthogonal corrector, phi = phiHbyA - flux, explicit p relaxation, U correction,
    SA transport + bound; reference DASimpleFoam.C:123-185, UEqnSimple.H, pEqnSimple.H, DASpalartAllmaras.C:386-405) - the per-entity
    bodies in host loops with serial Krylov solvers against the oracle's restatement with direct solves (oracle/primal.py), 1 and 3
    sweeps, on the bump channel (with and without the wall function) and on the NACA0012 O-grid."""
    from dafoam_amd.meshgen import naca0012_case
    from oracle.primal import simple_iteration

    E = _emu()
    E.emu_simple_iteration.argtypes = [C.POINTER(das_case_t), _capi.c_double_p, C.c_longlong, C.c_int, C.c_double, C.c_double, _capi.c_double_p]
    for case in (channel_case(7, 6, 5, perturb=0.0), channel_case(7, 6, 5, wall_function=True, perturb=0.0), naca0012_case(24, 8, 3, span=0.3, first_cell=1e-3, perturb=0.0)):
        g = Geometry(case.mesh)
        W = case.states.copy()
        oracle_states = [W]
        for _ in range(3):
            oracle_states.append(simple_iteration(case, g, oracle_states[-1]))
        cs = CaseStruct(case)
        for ns in (1, 3):
            out = np.zeros_like(W)
            assert E.emu_simple_iteration(cs.byref(), dptr(W), W.size, ns, 0.3, 1e-13, dptr(out)) == 0
            for nm, sl in blocks(case, g):
                assert relerr(out[sl], oracle_states[ns][sl]) < 1e-10, (nm, ns)


class _SimpleSolvers:
    """The inner solvers of the SIMPLE sweep (csrc/das_simple_host.hpp: simple_bicgstab, simple_pcg - the code the device driver runs, here
    over the harness's host operations) on random LDU matrices on the mesh of channel_case(4, 3, 3) (36 cells), and the same matrices
    assembled densely as body_ldu_row reads them: the owner's row takes up[f], the neighbour's row lo[f]."""

    def __init__(self):
        self.case = channel_case(4, 3, 3, perturb=0.0)
        mesh = self.case.mesh
        self.N, nIF = mesh.n_cells, mesh.n_internal_faces
        assert self.N == 36
        self.own, self.nei = np.asarray(mesh.owner[:nIF]), np.asarray(mesh.neighbour[:nIF])
        self.cs = CaseStruct(self.case)
        self.E = _emu()
        dp = _capi.c_double_p
        self.E.emu_simple_bicgstab.argtypes = [C.POINTER(das_case_t), dp, dp, dp, dp, dp, C.c_double, C.c_int]
        self.E.emu_simple_pcg.argtypes = [C.POINTER(das_case_t), dp, dp, dp, dp, dp, C.c_double, C.c_double, C.c_int]
        rng = np.random.default_rng(20240607)
        self.b = rng.standard_normal(self.N)
        # non-symmetric, |diag| > sum |off| per row
        up, lo = rng.uniform(-1.0, 1.0, nIF), rng.uniform(-1.0, 1.0, nIF)
        self.nonsym = (self._dominant_diag(up, lo, rng), up, lo)
        # symmetric with negative diagonal, -A positive definite (diagonally dominant): the shape of the pressure equation
        off = rng.uniform(-1.0, 1.0, nIF)
        self.sym = (-self._dominant_diag(off, off, rng), off, off.copy())

    def _dominant_diag(self, up, lo, rng):
        s = np.zeros(self.N)
        np.add.at(s, self.own, np.abs(up))
        np.add.at(s, self.nei, np.abs(lo))
        return s + rng.uniform(0.1, 1.0, self.N)

    def dense(self, ldu):
        diag, up, lo = ldu
        A = np.diag(diag)
        A[self.own, self.nei] = up
        A[self.nei, self.own] = lo
        return A

    def bicgstab(self, ldu, b, x0, tol, maxit):
        x = x0.copy()
        its = self.E.emu_simple_bicgstab(self.cs.byref(), dptr(ldu[0]), dptr(ldu[1]), dptr(ldu[2]), dptr(b), dptr(x), tol, maxit)
        return its, x

    def pcg(self, ldu, b, x0, sign, tol, maxit):
        x = x0.copy()
        its = self.E.emu_simple_pcg(self.cs.byref(), dptr(ldu[0]), dptr(ldu[1]), dptr(ldu[2]), dptr(b), dptr(x), sign, tol, maxit)
        return its, x


@pytest.fixture(scope="module")
def simple_solvers():
    return _SimpleSolvers()


def test_simple_bicgstab_equals_a_direct_solve(simple_solvers):
    S = simple_solvers
    A = S.dense(S.nonsym)
    assert np.all(np.abs(np.diag(A)) > np.abs(A - np.diag(np.diag(A))).sum(axis=1)) and not np.allclose(A, A.T)
    its, x = S.bicgstab(S.nonsym, S.b, np.zeros(S.N), 1e-13, 500)
    assert 0 < its < 500
    assert relerr(x, np.linalg.solve(A, S.b)) < 1e-10


def test_simple_pcg_with_sign_minus_one_equals_a_direct_solve(simple_solvers):
    S = simple_solvers
    A = S.dense(S.sym)
    assert np.array_equal(A, A.T) and np.all(np.diag(A) < 0) and np.linalg.eigvalsh(-A).min() > 0
    its, x = S.pcg(S.sym, S.b, np.zeros(S.N), -1.0, 1e-13, 500)
    assert 0 < its < 500
    assert relerr(x, np.linalg.solve(A, S.b)) < 1e-10


def test_simple_solvers_return_at_once_on_a_zero_right_hand_side(simple_solvers):
    S = simple_solvers
    zero = np.zeros(S.N)
    its, x = S.bicgstab(S.nonsym, zero, zero, 1e-13, 500)
    assert its == 0 and np.array_equal(x, zero)
    its, x = S.pcg(S.sym, zero, zero, -1.0, 1e-13, 500)
    assert its == 0 and np.array_equal(x, zero)


def test_simple_solvers_respect_the_iteration_cap(simple_solvers):
    S = simple_solvers
    A = S.dense(S.nonsym)
    _, xc = S.bicgstab(S.nonsym, S.b, np.zeros(S.N), 1e-13, 500)
    its, x1 = S.bicgstab(S.nonsym, S.b, np.zeros(S.N), 1e-13, 1)
    assert its == 1
    assert np.linalg.norm(S.b - A @ x1) > np.linalg.norm(S.b - A @ xc)
    A = S.dense(S.sym)
    _, xc = S.pcg(S.sym, S.b, np.zeros(S.N), -1.0, 1e-13, 500)
    its, x1 = S.pcg(S.sym, S.b, np.zeros(S.N), -1.0, 1e-13, 1)
    assert its == 1
    assert np.linalg.norm(S.b - A @ x1) > np.linalg.norm(S.b - A @ xc)


def test_seam_folded_cell_numbering_is_the_same_mesh_and_keeps_the_grid_sequencing_helpers_consistent():
    """Round 6 (naca0012_case(fold_seam=True), bench.py --naca-fold): the O-grid with the ring positions numbered 0, n-1, 1, n-2, ... - the
    same cells, geometry and state as the plain numbering under the permutation naca_ring_position decodes; ring neighbours are at most
    two ids apart (plain numbering: n - 1 across the seam); prolongation and extrusion commute with the permutation; the residual of the
    oracle is the same numbers."""
    from dafoam_amd.meshgen import _InputGeometry, extrude_naca_state, naca0012_case, naca_ring_position, prolong_naca_state

    nx, ny = 24, 8
    c0 = naca0012_case(nx, ny, 1, first_cell=1e-3, perturb=0.0)
    c1 = naca0012_case(nx, ny, 1, first_cell=1e-3, perturb=0.0, fold_seam=True)
    N = c0.mesh.n_cells
    ids = np.arange(N)
    old = naca_ring_position(ids, nx, True) + nx * (ids // nx)             # cell of c0 that cell `ids` of c1 is
    g0, g1 = _InputGeometry(c0.mesh), _InputGeometry(c1.mesh)
    assert np.abs(g1.C - g0.C[old]).max() < 1e-13 and np.abs(g1.V - g0.V[old]).max() < 1e-14
    assert np.allclose(c1.states[3 * N : 4 * N], c0.states[3 * N : 4 * N][old], rtol=0, atol=1e-13)
    nIF = c1.mesh.n_internal_faces
    ring = (c1.mesh.owner[:nIF] // nx) == (c1.mesh.neighbour // nx)
    assert np.abs(c1.mesh.owner[:nIF][ring].astype(int) - c1.mesh.neighbour[ring].astype(int)).max() <= 2
    ring0 = (c0.mesh.owner[:nIF] // nx) == (c0.mesh.neighbour // nx)
    assert np.abs(c0.mesh.owner[:nIF][ring0].astype(int) - c0.mesh.neighbour[ring0].astype(int)).max() == nx - 1
    R0 = residual(c0, Geometry(c0.mesh), c0.states)
    R1 = residual(c1, Geometry(c1.mesh), c1.states)
    assert relerr(R1[3 * N : 4 * N], R0[3 * N : 4 * N][old]) < 1e-11 and relerr(R1[: 3 * N].reshape(N, 3), R0[: 3 * N].reshape(N, 3)[old]) < 1e-11
    # grid sequencing: coarse folded -> fine folded equals the plain prolongation, permuted
    f0 = naca0012_case(2 * nx, 2 * ny, 1, first_cell=5e-4, perturb=0.0)
    f1 = naca0012_case(2 * nx, 2 * ny, 1, first_cell=5e-4, perturb=0.0, fold_seam=True)
    P0 = prolong_naca_state((nx, ny), c0.states, f0, (2 * nx, 2 * ny), first_cell=5e-4, coarse_first_cell=1e-3)
    P1 = prolong_naca_state((nx, ny), c1.states, f1, (2 * nx, 2 * ny), first_cell=5e-4, coarse_first_cell=1e-3, fold_seam=True)
    Nf = f0.mesh.n_cells
    idf = np.arange(Nf)
    oldf = naca_ring_position(idf, 2 * nx, True) + 2 * nx * (idf // (2 * nx))
    assert np.allclose(P1[3 * Nf : 4 * Nf], P0[3 * Nf : 4 * Nf][oldf], rtol=0, atol=1e-12)
    assert np.allclose(P1[: 3 * Nf].reshape(Nf, 3), P0[: 3 * Nf].reshape(Nf, 3)[oldf], rtol=0, atol=1e-12)
    # extrusion keeps the numbering layer by layer
    e1 = naca0012_case(nx, ny, 3, span=0.3, first_cell=1e-3, perturb=0.0, fold_seam=True, y_wall_section=c1.y_wall)
    W3 = extrude_naca_state(c1, c1.states, e1, (nx, ny, 3))
    assert np.array_equal(W3[3 * 3 * N : 4 * 3 * N], np.tile(c1.states[3 * N : 4 * N], 3))


def test_compressible_channel_prolongation_is_consistent():
    """Round 6 (grid sequencing of the DARhoSimpleFoam primal, dafoam_amd.meshgen.prolong_rho_channel_state): a coarse state prolonged to a
    mesh of the SAME size reproduces the cell fields; to a finer mesh it keeps their ranges, and the rebuilt mass flux is
    interpolate(rho) interpolate(U).Sf - on a uniform state exactly rho U.Sf on the internal faces."""
    from dafoam_amd.meshgen import _InputGeometry, prolong_rho_channel_state, rho_channel_case

    kw = dict(lengths=(2.0, 0.2, 0.2), grading_y=2.0)
    c = rho_channel_case(6, 4, 4, **kw)
    same = rho_channel_case(6, 4, 4, **kw)
    prolong_rho_channel_state(same, (6, 4, 4), {"dims": (6, 4, 4), "W": c.states})
    N = c.mesh.n_cells
    assert np.allclose(same.states[: 6 * N], c.states[: 6 * N], rtol=1e-12, atol=1e-12)
    f = rho_channel_case(12, 8, 8, **kw)
    prolong_rho_channel_state(f, (12, 8, 8), {"dims": (6, 4, 4), "W": c.states})
    Nf = f.mesh.n_cells
    for b in (3, 4, 5):  # p, T, nuTilda: finite, positive, within one coarse range of the coarse extremes (the outermost half cells extrapolate linearly)
        lo, hi = c.states[b * N : (b + 1) * N].min(), c.states[b * N : (b + 1) * N].max()
        v = f.states[b * Nf : (b + 1) * Nf]
        assert np.all(np.isfinite(v)) and v.min() > 0.0 and v.min() >= lo - (hi - lo) - 1e-9 * abs(lo) and v.max() <= hi + (hi - lo) + 1e-9 * abs(hi)
    u = rho_channel_case(5, 4, 3, **kw)
    Nu = u.mesh.n_cells
    W = u.states.copy()
    W[: 3 * Nu] = np.tile([30.0, 0.0, 0.0], Nu)
    W[3 * Nu : 4 * Nu], W[4 * Nu : 5 * Nu] = 101325.0, 300.0
    fu = rho_channel_case(10, 8, 6, **kw)
    prolong_rho_channel_state(fu, (10, 8, 6), {"dims": (5, 4, 3), "W": W})
    g = _InputGeometry(fu.mesh)
    rho = 101325.0 / (8314.47 / fu.thermo["molWeight"] * 300.0)
    nIF = fu.mesh.n_internal_faces
    phi = fu.states[6 * fu.mesh.n_cells :]
    assert np.allclose(phi[:nIF], rho * 30.0 * g.Sf[:nIF, 0], rtol=1e-12, atol=1e-12 * rho * 30.0 * np.abs(g.Sf[:, 0]).max())


def test_additive_schwarz_overlap_mask_of_a_rank():
    """Round 6: the sub-domain of a rank under adjEqnOption.asmOverlap (dafoam_amd.distributed.overlap_mask; reference PCASMSetOverlap,
    DALinearEqn.C:212-216) on the slab partition of the channel: overlap 0 = the owned unknowns; overlap k = owned + the states anchored at
    the cells within k face-neighbour rings (cell states at the cell, face fluxes at the face's owner cell), never a cut face; nested in k."""
    from dafoam_amd.distributed import SlabPartition, overlap_mask, state_table

    NX, NY, NZ = 8, 4, 3
    for rank in (0, 1):
        part = SlabPartition(NX, NY, NZ, rank, 2)
        case = channel_case(part.nxl, NY, NZ, x_range=(part.e0, part.e1, NX), lengths=(2.0, 0.2, 0.2), perturb=0.0)
        key, orank, owned = state_table(part, case.mesh)
        m = case.mesh
        N, F = m.n_cells, m.n_faces
        m0, m1, m2 = (overlap_mask(m, orank, rank, k) for k in (0, 1, 2))
        assert np.array_equal(m0, owned)
        assert np.all(m1[owned]) and np.all(m2[m1]) and m1.sum() > owned.sum() and m2.sum() > m1.sum()
        assert not np.any(m2[orank < 0])                                      # cut faces belong to nobody
        cell_owned = orank[3 * N : 4 * N] == rank
        own_f, nei = np.asarray(m.owner), np.asarray(m.neighbour)
        nIF = m.n_internal_faces
        ring1 = cell_owned.copy()
        ring1[own_f[:nIF][cell_owned[nei]]] = True
        ring1[nei[cell_owned[own_f[:nIF]]]] = True
        assert np.array_equal(m1[3 * N : 4 * N], ring1)                       # p block: exactly the owned cells + one ring
        assert np.array_equal(m1[: 3 * N].reshape(N, 3).all(axis=1), ring1)   # U block alike
        phi = m1[5 * N :]
        assert np.array_equal(phi[orank[5 * N :] >= 0], ring1[own_f][orank[5 * N :] >= 0])  # fluxes follow their owner cell


def test_kernel_bodies_match_oracle_scalar_transport():
    case = scalar_transport_case(8, 7, 6)
    g = Geometry(case.mesh)
    W = case.states
    Rv, _ = _emu_res(case, W)
    assert relerr(Rv, residual(case, g, W)) < 1e-13
    v = np.random.default_rng(0).standard_normal(W.size)
    _, Rd = _emu_res(case, W, 0, v)
    assert relerr(Rd, residual(case, g, W + 1j * 1e-30 * v).imag / 1e-30) < 1e-12


@pytest.mark.parametrize("kind", ["simple", "rho"])
def test_kernel_bodies_bc_value_tangent(kind):
    """dR/d(patch value): the dual-number BC seeds of the kernel bodies vs central differences of the oracle with the
    patch table perturbed (inlet U, outlet p / inletOutlet refValue, inlet nuTilda, inlet T)."""
    import copy
    case = channel_case(7, 6, 5, wall_function=True) if kind == "simple" else rho_channel_case(7, 6, 5)
    g = Geometry(case.mesh)
    W = case.states
    L = _emu()
    L.emu_residual_bc.argtypes = [C.POINTER(das_case_t), _capi.c_double_p, C.c_longlong, C.c_int, C.c_int, _capi.c_double_p, _capi.c_double_p]
    names = [p.name for p in case.mesh.patches]
    probes = [("inlet", "U", 0, np.array([0.8, 0.3, -0.2])), ("inlet", "nuTilda", 2, np.array([1.0, 0, 0])),
              ("outlet", "p", 1, np.array([1.0, 0, 0])), ("outlet", "U", 0, np.array([0.5, -0.4, 0.1]))]
    if kind == "rho":
        probes.append(("inlet", "T", 3, np.array([1.0, 0, 0])))
    for pname, field, fid, t in probes:
        code, v0 = case.bcs[pname][field]
        Rd = np.zeros(W.size)
        cs = CaseStruct(case)  # (kept alive: the struct points into arrays the wrapper owns)
        assert L.emu_residual_bc(cs.byref(), dptr(W), W.size, names.index(pname), fid, dptr(t), dptr(Rd)) == 0
        vmax = float(np.max(np.abs(v0)))
        h = 1e-4 * vmax if vmax > 0 else 1e-6
        Rpm = []
        for sgn in (1, -1):
            c2 = copy.copy(case)
            c2.bcs = copy.deepcopy(case.bcs)
            c2.bcs[pname][field] = (code, (np.asarray(v0, dtype=float) + sgn * h * t) if field == "U" else float(v0) + sgn * h * t[0])
            Rpm.append(residual(c2, g, W))
        fd = (Rpm[0] - Rpm[1]) / (2 * h)
        if code in (0, 2) and np.abs(fd).max() > 0:  # fixedValue / inletOutlet carry a value
            assert relerr(Rd, fd) < 1e-6, (pname, field)
        else:
            assert np.abs(Rd).max() == 0.0 and np.abs(fd).max() < 1e-9, (pname, field)


def test_unstructured_renumbering_invariance():
    """Random cell renumbering (faces re-sorted / re-oriented): the oracle residual is the permuted residual, the
    kernel bodies agree with the oracle on the renumbered mesh, and connectivity/colouring stay valid - nothing
    relies on the structured numbering of the generators."""
    base = channel_case(6, 5, 4, wall_function=True)
    case = renumber_case(base, seed=3)
    gb, g = Geometry(base.mesh), Geometry(case.mesh)
    assert np.all(case.mesh.neighbour > case.mesh.owner[: case.mesh.n_internal_faces])
    Rb, R = residual(base, gb, base.states), residual(case, g, case.states)
    N = g.nC
    # compare sorted per-block values (permutation invariant) and norms
    for nm, sl in blocks(case, g):
        assert relerr(np.sort(np.abs(R[sl])), np.sort(np.abs(Rb[sl]))) < 1e-11, nm
    Rv, _ = _emu_res(case, case.states)
    assert relerr(Rv, R) < 1e-12
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    s.runColoring()
    assert (s.getConnectivity(0) != J.connectivity(case, g)).nnz == 0
    col, nc = s.getColoring()
    assert J.validate_coloring(J.connectivity(case, g), col.astype(np.int64))


def test_coloring_cache_roundtrip_and_validation(tmp_path):
    """dRdWColoring_<nProcs>.bin cache (reference DAJacCon.C:1886-2019): written as a PETSc Vec, read back and
    validated; a file that does not validate against the connectivity is recomputed, a conflicting colouring handed
    to the C-ABI is rejected with the reference's message."""
    from dafoam_amd import petsc_io

    case = channel_case(6, 5, 4, wall_function=True)
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    s.runColoring(cacheDir=str(tmp_path))
    f = tmp_path / "dRdWColoring_1.bin"
    assert f.exists()
    col, nc = s.getColoring()
    assert np.array_equal(petsc_io.read_vec(str(f)), col.astype(np.float64))
    # a second solver picks the cached colours up (a permuted-but-valid colouring proves the file is what is used)
    perm = np.random.default_rng(0).permutation(nc)
    petsc_io.write_vec(str(f), perm[col].astype(np.float64))
    s2 = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    s2.runColoring(cacheDir=str(tmp_path))
    col2, nc2 = s2.getColoring()
    assert nc2 == nc and np.array_equal(col2, perm[col])
    g = Geometry(case.mesh)
    assert J.validate_coloring(J.connectivity(case, g), col2.astype(np.int64))
    # conflicting colours: rejected by the library; the cache path falls back to a fresh colouring
    bad = np.zeros(col.size, dtype=np.int32)
    with pytest.raises(_capi.DASError, match="Conflicting Colors Found"):
        _capi.check(_capi.lib().das_set_coloring(s2._h, bad.ctypes.data_as(_capi.c_int_p)))
    petsc_io.write_vec(str(f), bad.astype(np.float64))
    s3 = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    s3.runColoring(cacheDir=str(tmp_path))
    col3, _ = s3.getColoring()
    assert np.array_equal(col3, col) and np.array_equal(petsc_io.read_vec(str(f)), col.astype(np.float64))


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (1, 3, 1), (2, 2, 2)])
def test_degenerate_meshes(dims):
    """Edge cases: a single cell (no internal face at all), one row / one column of cells.  Oracle, kernel bodies,
    connectivity and colouring agree; with 8 or fewer cells every column conflicts with every other (n colours)."""
    case = channel_case(*dims, wall_function=True)
    g = Geometry(case.mesh)
    W = case.states
    Ro = residual(case, g, W)
    Rv, _ = _emu_res(case, W)
    assert np.abs(Rv - Ro).max() <= 1e-12 * np.abs(Ro).max()
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    s.runColoring()
    con = J.connectivity(case, g)
    assert (s.getConnectivity(0) != con).nnz == 0
    col, nc = s.getColoring()
    assert J.validate_coloring(con, col.astype(np.int64))
    if case.mesh.n_cells <= 3:
        assert nc == W.size


@pytest.mark.parametrize("sector", [None, (0.5, 0.12)])
def test_openfoam_boundary_cyclic_roundtrip(tmp_path, sector):
    """constant/polyMesh/boundary with a cyclic pair (neighbourPatch, transform translational / rotational): written and
    read back; the rotation tensor forwardT is recovered from rotationAxis / rotationCentre and the first face pair."""
    from dafoam_amd import foam_io

    c = periodic_channel_case(4, 3, 4, sector=sector)
    foam_io.write_polymesh(str(tmp_path), c.mesh)
    txt = open(tmp_path / "constant" / "polyMesh" / "boundary").read()
    assert "neighbourPatch  back;" in txt and ("rotational" if sector else "separationVector") in txt
    m = foam_io.read_polymesh(str(tmp_path))
    for p0, p1 in zip(c.mesh.patches, m.patches):
        assert (p0.name, p0.type, p0.neighbour, p0.start, p0.size) == (p1.name, p1.type, p1.neighbour, p1.start, p1.size)
        if p0.rotation is None:
            assert p1.rotation is None
        else:
            assert np.abs(p0.rotation - p1.rotation).max() < 1e-14


def test_openfoam_rotational_cyclic_off_origin_mixed_sign_axis(tmp_path):
    """A rotational cyclic pair whose axis has mixed-sign components and does not pass through the origin (a rigidly moved
    sector): rotationAxis / rotationCentre written by write_polymesh reproduce forwardT on reading."""
    from dafoam_amd import foam_io

    c = periodic_channel_case(4, 3, 4, sector=(0.5, 0.12))
    a = np.array([0.2, -0.1, 1.0]); a /= np.linalg.norm(a)
    th = 2.2
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R0 = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    c.mesh.points = c.mesh.points @ R0.T + np.array([0.3, -1.1, 2.0])
    for p in c.mesh.patches:
        if p.rotation is not None:
            p.rotation = R0 @ np.asarray(p.rotation).reshape(3, 3) @ R0.T
    foam_io.write_polymesh(str(tmp_path), c.mesh)
    txt = open(tmp_path / "constant" / "polyMesh" / "boundary").read()
    axis = np.array(re.search(r"rotationAxis\s+\(([^)]*)\)", txt).group(1).split(), dtype=float)
    assert (axis < -1e-6).any() and (axis > 1e-6).any()                      # the sign pattern survives
    centre = np.array(re.search(r"rotationCentre\s+\(([^)]*)\)", txt).group(1).split(), dtype=float)
    assert np.linalg.norm(centre) > 0.1
    m = foam_io.read_polymesh(str(tmp_path))
    for p0, p1 in zip(c.mesh.patches, m.patches):
        if p0.rotation is not None:
            assert np.abs(np.asarray(p0.rotation).reshape(3, 3) - p1.rotation).max() < 1e-12


def test_update_of_mesh_recomputes_metrics():
    """updateOFMesh (reference pyDASolvers.pyx:297-300): the library's fvMesh metrics after moving the points equal the
    oracle's geometry of the moved mesh; the wall distance stays frozen; getOFMeshPoints returns the new points."""
    import copy

    case = channel_case(6, 5, 4, wall_function=True)
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    moved = channel_case(6, 5, 4, wall_function=True, bump=0.13, skew=0.1)
    X = np.ascontiguousarray(moved.mesh.points.ravel())
    s.updateOFMesh(X)
    back = np.zeros(X.size)
    s.getOFMeshPoints(back)
    assert np.array_equal(back, X)
    geo = s.geometry()
    g = Geometry(moved.mesh)
    nIF = g.nIF
    assert relerr(geo["Sf"].reshape(-1, 3), np.concatenate([g.Sf[:nIF], g.bSf])) < 1e-13 and relerr(geo["V"], g.V) < 1e-13
    assert relerr(geo["w"], g.w) < 1e-13 and relerr(geo["nonOrthDeltaCoeffs"], g.nonOrthDeltaCoeffs) < 1e-13
    with pytest.raises(AssertionError):
        s.updateOFMesh(X[:-3])


def test_flow_aligned_force_directions():
    """directionMode parallelToFlow / normalToFlow (reference DAFunctionForce.C:45-61,92-113): direction and its AoA
    derivative from the patchVelocity input; any other mode is rejected with the reference's message."""
    case = channel_case(4, 3, 3)
    o = options(case, function={"CD": {"type": "force", "patches": ["bottom"], "directionMode": "parallelToFlow", "patchVelocityInputName": "pv"},
                                "CL": {"type": "force", "patches": ["bottom"], "directionMode": "normalToFlow", "patchVelocityInputName": "pv"}},
                inputInfo={"pv": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "z"}})
    s = pyDASolvers(b"DASimpleFoam -python", o, case=case)
    s._patchVelocity = [10.0, 30.0]
    a = np.pi / 6
    assert np.allclose(s._flow_direction(s._flowdir_fns["CD"]), [np.cos(a), 0.0, np.sin(a)])
    assert np.allclose(s._flow_direction(s._flowdir_fns["CL"]), [-np.sin(a), 0.0, np.cos(a)])
    h = 1e-6
    for nm in ("CD", "CL"):
        s._patchVelocity = [10.0, 30.0 + h]
        dp = s._flow_direction(s._flowdir_fns[nm])
        s._patchVelocity = [10.0, 30.0 - h]
        dm = s._flow_direction(s._flowdir_fns[nm])
        s._patchVelocity = [10.0, 30.0]
        assert np.allclose(s._flow_direction(s._flowdir_fns[nm], deriv=True), (dp - dm) / (2 * h), atol=1e-9)
    o["function"]["CD"]["directionMode"] = "sideways"
    with pytest.raises(_capi.DASError, match="directionMode for CD not valid"):
        pyDASolvers(b"DASimpleFoam -python", o, case=case)


def test_pydafoam_check_options():
    """PYDAFOAM._checkOptions (reference pyDAFoam.py:846-899): invalid option combinations are rejected with the
    reference's messages before any solver object exists."""
    from dafoam_amd.pyDAFoam import PYDAFOAM, Error

    case = channel_case(4, 3, 3)
    with pytest.raises(Error, match="function-CD-patches-wing is not valid"):
        PYDAFOAM(options=options(case, function={"CD": {"type": "force", "patches": ["wing"], "direction": [1.0, 0.0, 0.0]}}), case=case)
    with pytest.raises(Error, match="discipline: solid not supported"):
        PYDAFOAM(options=options(case, discipline="solid"), case=case)
    with pytest.raises(Error, match="useAD->mode only supports reverse, or forward"):
        PYDAFOAM(options=options(case, useAD={"mode": "fd"}), case=case)


def test_write_adjoint_fields(tmp_path):
    """writeAdjointFields (reference DASolver.C:4055-4160): psi as adjoint_<function>_<state> OpenFOAM fields, read back."""
    from dafoam_amd import foam_io

    case = channel_case(5, 4, 3, wall_function=True)
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    n = s.getNLocalAdjointStates()
    N, F = case.mesh.n_cells, case.mesh.n_faces
    psi = np.random.default_rng(0).standard_normal(n)
    files = s.writeAdjointFields("CD", 100, psi, caseDir=str(tmp_path))
    assert sorted(os.path.basename(f) for f in files) == ["adjoint_CD_U", "adjoint_CD_nuTilda", "adjoint_CD_p", "adjoint_CD_phi"]
    U, _ = foam_io.read_field(str(tmp_path / "100" / "adjoint_CD_U"), N, 3)
    p, _ = foam_io.read_field(str(tmp_path / "100" / "adjoint_CD_p"), N, 1)
    assert np.array_equal(U.ravel(), psi[: 3 * N]) and np.array_equal(p, psi[3 * N : 4 * N])
    txt = open(tmp_path / "100" / "adjoint_CD_phi").read()
    assert "surfaceScalarField" in txt and f"\n{case.mesh.n_internal_faces}\n" in txt
    with pytest.raises(AssertionError):
        s.writeAdjointFields("CD", 100, psi[:-1], caseDir=str(tmp_path))
    with pytest.raises(_capi.DASError, match="mode not valid"):
        s.calcPrimalResidualStatistics("bogus")


def test_petsc_binary_io_roundtrip_and_layout(tmp_path):
    """PETSc binary Vec/Mat (big-endian, classids 1211214 / 1211216 - SURVEY.md Appendix D)."""
    import scipy.sparse as sp

    from dafoam_amd import petsc_io as pio

    x = np.array([1.0, -2.5, 3.25])
    pv = tmp_path / "v.bin"
    pio.write_vec(pv, x)
    raw = pv.read_bytes()
    assert raw[:8] == (1211214).to_bytes(4, "big") + (3).to_bytes(4, "big") and len(raw) == 8 + 24
    assert raw[8:16] == np.array([1.0], dtype=">f8").tobytes()
    assert np.array_equal(pio.read_vec(pv), x)
    A = sp.random(7, 7, 0.4, random_state=0, format="csr") + sp.identity(7)
    pm = tmp_path / "m.bin"
    pio.write_mat(pm, A)
    hdr = np.frombuffer(pm.read_bytes()[:16], dtype=">i4")
    assert list(hdr) == [1211216, 7, 7, A.nnz]
    B = pio.read_mat(pm)
    assert (abs(A - B)).max() == 0.0
    assert pio.matdiff(pm, pm, verbose=False) and pio.vecdiff(pv, pv, verbose=False)
    pio.write_vec(tmp_path / "w.bin", x * (1 + 1e-3))
    assert not pio.vecdiff(pv, tmp_path / "w.bin", verbose=False)
    with pytest.raises(ValueError):
        pio.read_mat(pv)


@pytest.mark.parametrize("transport", ["const", "sutherland"])
@pytest.mark.parametrize("wall_function", [False, True])
@pytest.mark.parametrize("isPC", [0, 1])
def test_kernel_bodies_match_oracle_rhosimplefoam(wall_function, isPC, transport):
    """DARhoSimpleFoam (compressible) kernel bodies vs oracle/residual_rho.py: values and dual tangents; const transport
    and Sutherland's law with the modified-Eucken alpha (DAResidual::updateThermoVars, DAResidual.C:264-293)."""
    case = rho_channel_case(7, 6, 5, wall_function=wall_function, perturb=0.02)
    if transport == "sutherland":
        case.thermo = dict(case.thermo, transport="sutherland", As=1.4792e-06, Ts=116.0)
    g = Geometry(case.mesh)
    W = case.states
    Ro = residual(case, g, W, isPC=bool(isPC))
    Rv, _ = _emu_res(case, W, isPC)
    for nm, sl in blocks(case, g):
        assert relerr(Rv[sl], Ro[sl]) < 1e-11, nm
    v = np.random.default_rng(3).standard_normal(W.size) * J.state_scales(case, g, NORM_STATES_RHO)
    cs = residual(case, g, W + 1j * 1e-30 * v, isPC=bool(isPC)).imag / 1e-30
    _, Rd = _emu_res(case, W, isPC, v)
    for nm, sl in blocks(case, g):
        assert relerr(Rd[sl], cs[sl]) < 1e-10, nm


@pytest.mark.parametrize("variant", ["rho_mrf", "turbo", "turbo_nomrf", "turbo_transonic", "turbo_transonic_pc2"])
@pytest.mark.parametrize("isPC", [0, 1])
def test_kernel_bodies_match_oracle_turbofoam_and_mrf(variant, isPC):
    """DATurboFoam (SIMPLEC-consistent / transonic pEqn, "h" energy with viscous and MRF pressure work) and the MRF
    terms of DARhoSimpleFoam: kernel bodies vs oracle/residual_rho.py, values and dual tangents."""
    kw = {"rho_mrf": dict(solver_name="DARhoSimpleFoam"), "turbo": {}, "turbo_nomrf": dict(mrf=False),
          "turbo_transonic": dict(transonic=True), "turbo_transonic_pc2": dict(transonic=True)}[variant]
    case = turbo_channel_case(6, 5, 4, wall_function=True, perturb=0.02, **kw)
    if variant == "turbo_transonic_pc2":
        case.transonic_pc_option = 2
    g = Geometry(case.mesh)
    W = case.states
    Ro = residual(case, g, W, isPC=bool(isPC))
    Rv, _ = _emu_res(case, W, isPC)
    for nm, sl in blocks(case, g):
        assert relerr(Rv[sl], Ro[sl]) < 1e-11, nm
    v = np.random.default_rng(3).standard_normal(W.size) * J.state_scales(case, g, NORM_STATES_RHO)
    cs = residual(case, g, W + 1j * 1e-30 * v, isPC=bool(isPC)).imag / 1e-30
    _, Rd = _emu_res(case, W, isPC, v)
    for nm, sl in blocks(case, g):
        assert relerr(Rd[sl], cs[sl]) < 1e-10, nm


@pytest.mark.parametrize("isPC", [0, 1])
def test_simplefoam_with_T_field(isPC):
    """DASimpleFoam with the optional passive T field (DAResidualSimpleFoam.C:215-235, states [U|p|T|nuTilda|phi]):
    kernel bodies vs oracle (values, dual tangents), connectivity and colouring of the 5-block layout."""
    from common import norm_states

    case = simple_T_channel_case(6, 5, 4, wall_function=True, perturb=0.02)
    g = Geometry(case.mesh)
    W = case.states
    assert W.size == 6 * g.nC + g.nF
    Ro = residual(case, g, W, isPC=bool(isPC))
    Rv, _ = _emu_res(case, W, isPC)
    for nm, sl in blocks(case, g):
        assert relerr(Rv[sl], Ro[sl]) < 1e-12, nm
    v = np.random.default_rng(3).standard_normal(W.size) * J.state_scales(case, g, norm_states(case))
    cs = residual(case, g, W + 1j * 1e-30 * v, isPC=bool(isPC)).imag / 1e-30
    _, Rd = _emu_res(case, W, isPC, v)
    for nm, sl in blocks(case, g):
        assert relerr(Rd[sl], cs[sl]) < 1e-10, nm
    # the other residuals do not see T (passive scalar)
    W2 = W.copy()
    W2[4 * g.nC : 5 * g.nC] *= 1.01
    R2 = residual(case, g, W2, isPC=bool(isPC))
    b = dict(blocks(case, g))
    assert np.array_equal(R2[b["U"]], Ro[b["U"]]) and np.array_equal(R2[b["p"]], Ro[b["p"]]) and relerr(R2[b["T"]], Ro[b["T"]]) > 1e-6
    if not isPC:
        s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
        assert s.getNLocalAdjointStates() == W.size
        s.runColoring()
        for pc in (0, 1):
            assert (s.getConnectivity(pc) != J.connectivity(case, g, isPC=bool(pc))).nnz == 0
        col, _ = s.getColoring()
        assert J.validate_coloring(J.connectivity(case, g), col.astype(np.int64))


@pytest.mark.parametrize("wall_function", [False, True])
@pytest.mark.parametrize("isPC", [0, 1])
def test_cyclic_translational_vs_unrolled_oracle(wall_function, isPC):
    """Cyclic (coupled) patch pair, OpenFOAM cyclicFvPatch semantics for a translational pair: the paired cell acts as
    the neighbour of the boundary face (interpolation weights nbrDelta/(delta+nbrDelta), delta = own-centre -> image of
    the neighbour centre, corrected non-orthogonal flux), both faces keep their own phi state and phiRes row.
    Checked WITHOUT a cyclic oracle: the same periodic block unrolled three times is an ordinary mesh for the unchanged
    oracle, whose middle copy sees the periodic images as real neighbours - values and (periodic-consistent) tangents
    of every residual row incl. the cyclic faces' phiRes agree to round-off."""
    c1 = periodic_channel_case(6, 5, 5, wall_function=wall_function)
    c3 = periodic_channel_case(6, 5, 5, copies=3, wall_function=wall_function)
    idx, sgn = unrolled_maps(c1, c3)
    assert np.allclose(c3.states[idx] * sgn, c1.states, rtol=1e-12, atol=0.0)
    g1, g3 = Geometry(c1.mesh), Geometry(c3.mesh)
    ref = residual(c3, g3, c3.states, isPC=bool(isPC))[idx] * sgn
    Rv, _ = _emu_res(c1, c1.states, isPC)
    for nm, sl in blocks(c1, g1):
        assert relerr(Rv[sl], ref[sl]) < 1e-12, nm
    v = np.random.default_rng(1).standard_normal(c1.states.size) * J.state_scales(c1, g1, NORM_STATES)
    sl = {p.name: np.arange(p.start, p.start + p.size) for p in c1.mesh.patches}
    off = c1.states.size - c1.mesh.n_faces
    v[off + sl["front"]] = -v[off + sl["back"]]  # periodic-consistent direction: one flux per pair in the unrolled mesh
    v3 = unroll_periodic_vector(c1.mesh, c3.mesh, v, 3)
    cs = (residual(c3, g3, c3.states + 1e-30j * v3, isPC=bool(isPC)).imag / 1e-30)[idx] * sgn
    _, Rd = _emu_res(c1, c1.states, isPC, v)
    for nm, sl_ in blocks(c1, g1):
        assert relerr(Rd[sl_], cs[sl_]) < 1e-11, nm


@pytest.mark.parametrize("variant", ["simple", "simple_mrf", "rho", "turbo_mrf", "turbo_mrf_transonic"])
@pytest.mark.parametrize("isPC", [0, 1])
def test_cyclic_rotational_sector_vs_unrolled_oracle(variant, isPC):
    """Rotational cyclic pair (annular sector about the x axis, forwardT = Rx(-+dtheta)): neighbour-side velocities,
    gradients (Q G Q^T), HbyA, grad(p), Teff.U and the upwind offsets are rotated into this side's frame.  With MRF about
    the same axis, a rotating hub and DATurboFoam this is the compressor-passage configuration of the reference's
    turbo tests (tests/runRegTests_DATurboFoam*.py).  Reference: the unchanged oracle on the three-sector arc."""
    from common import norm_states

    sector = (0.5, 0.12)
    kw = {"simple": {}, "simple_mrf": dict(mrf_omega=15.0), "rho": dict(solver_name="DARhoSimpleFoam"),
          "turbo_mrf": dict(solver_name="DATurboFoam", mrf_omega=60.0),
          "turbo_mrf_transonic": dict(solver_name="DATurboFoam", mrf_omega=60.0, transonic=True)}[variant]
    c1 = periodic_channel_case(6, 5, 5, wall_function=True, sector=sector, **kw)
    c3 = periodic_channel_case(6, 5, 5, copies=3, wall_function=True, sector=sector, **kw)
    idx, sgn = unrolled_maps(c1, c3)
    assert np.allclose(c3.states[idx] * sgn, c1.states, rtol=1e-12, atol=0.0)
    g1, g3 = Geometry(c1.mesh), Geometry(c3.mesh)
    ref = residual(c3, g3, c3.states, isPC=bool(isPC))[idx] * sgn
    Rv, _ = _emu_res(c1, c1.states, isPC)
    for nm, sl in blocks(c1, g1):
        assert relerr(Rv[sl], ref[sl]) < 1e-11, nm
    v = np.random.default_rng(1).standard_normal(c1.states.size) * J.state_scales(c1, g1, norm_states(c1))
    sl = {p.name: np.arange(p.start, p.start + p.size) for p in c1.mesh.patches}
    off = c1.states.size - c1.mesh.n_faces
    v[off + sl["front"]] = -v[off + sl["back"]]
    v3 = unroll_periodic_vector(c1.mesh, c3.mesh, v, 3, dtheta=sector[1])
    cs = (residual(c3, g3, c3.states + 1e-30j * v3, isPC=bool(isPC)).imag / 1e-30)[idx] * sgn
    _, Rd = _emu_res(c1, c1.states, isPC, v)
    for nm, sl_ in blocks(c1, g1):
        assert relerr(Rd[sl_], cs[sl_]) < 1e-11, nm


def test_cyclic_connectivity_covers_every_dependency():
    """dRdWCon with a cyclic pair: the level rings run through the pair (the paired cell is a face neighbour, cyclic
    faces are coupled to two cells).  Every non-zero of the column-by-column forward-mode Jacobian of the kernel bodies
    lies inside the pattern, the colouring is valid and the mesh without the pair has a strictly smaller pattern."""
    c1 = periodic_channel_case(4, 3, 4, wall_function=True)
    s = pyDASolvers(b"DASimpleFoam -python", options(c1), case=c1)
    s.runColoring()
    con = s.getConnectivity(0).tocsr()
    n = c1.states.size
    dense = np.zeros((n, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        _, Rd = _emu_res(c1, c1.states, 0, e)
        dense[:, j] = Rd
    pat = np.asarray(con.todense()) != 0
    assert np.abs(np.where(pat, 0.0, dense)).max() == 0.0
    col, nc = s.getColoring()
    for r in range(n):
        cs = col[con.indices[con.indptr[r] : con.indptr[r + 1]]]
        assert np.unique(cs).size == cs.size
    plain = channel_case(4, 3, 4, wall_function=True)
    s2 = pyDASolvers(b"DASimpleFoam -python", options(plain), case=plain)
    s2.runColoring()
    assert s2.getConnectivity(0).nnz < con.nnz


def test_simplefoam_mrf_and_simplec():
    """DASimpleFoam with MRF (DAResidualSimpleFoam.C:139,182,245): kernel bodies vs oracle, values and dual tangents.
    SIMPLEC (`consistent`, :187-194) cancels identically in pRes and phiRes: interpolate(rAtU - rAU) snGrad(p) is added to
    phiHbyA and to the laplacian flux alike (linear interpolation is linear), which the oracle confirms to round-off -
    the kernels therefore need no rAtU for this solver."""
    case = channel_case(6, 5, 4, wall_function=True, perturb=0.02)
    g = Geometry(case.mesh)
    W = case.states
    R0 = residual(case, g, W)
    case.simple_consistent = True
    Rc = residual(case, g, W)
    assert np.abs(Rc - R0).max() <= 1e-12 * np.abs(R0).max()
    case.mrf = {"omega": (20.0, 0.0, 0.0), "origin": (0.0, -0.3, 0.0), "nonRotatingPatches": ["inlet", "outlet", "top"]}
    for isPC in (0, 1):
        Ro = residual(case, g, W, isPC=bool(isPC))
        assert relerr(Ro, R0) > 1e-3
        Rv, _ = _emu_res(case, W, isPC)
        for nm, sl in blocks(case, g):
            assert relerr(Rv[sl], Ro[sl]) < 1e-12, nm
        v = np.random.default_rng(3).standard_normal(W.size) * J.state_scales(case, g, NORM_STATES)
        cs = residual(case, g, W + 1j * 1e-30 * v, isPC=bool(isPC)).imag / 1e-30
        _, Rd = _emu_res(case, W, isPC, v)
        for nm, sl in blocks(case, g):
            assert relerr(Rd[sl], cs[sl]) < 1e-10, nm


def test_turbofoam_connectivity_and_coloring_host():
    """dRdWCon of DATurboFoam (DAStateInfoTurboFoam.C:82-119) from the C++ pattern builder equals the oracle's; the
    brute-force oracle Jacobian has no entry outside it (SIMPLEC, viscous-work and MRF terms stay inside the stencil)."""
    case = turbo_channel_case(5, 4, 4, wall_function=True, perturb=0.02)
    g = Geometry(case.mesh)
    s = pyDASolvers(b"DATurboFoam -python", options(case), case=case)
    s.runColoring()
    for pc in (0, 1):
        assert (s.getConnectivity(pc) != J.connectivity(case, g, isPC=bool(pc))).nnz == 0
    col, nc = s.getColoring()
    con = J.connectivity(case, g)
    assert J.validate_coloring(con, col.astype(np.int64))
    sc = J.state_scales(case, g, NORM_STATES_RHO)
    Jb = J.jacobian_bruteforce(case, g, case.states, sc)
    outside = np.where(np.asarray(con.T.todense()) != 0, 0.0, Jb)
    assert np.abs(outside).max() == 0.0


def test_turbofoam_mrf_terms_are_active():
    """The MRF / turbo switches change the residual blocks they should (guards against silently inactive branches)."""
    base = turbo_channel_case(5, 4, 4, mrf=False, solver_name="DARhoSimpleFoam", perturb=0.02)
    g = Geometry(base.mesh)
    W = base.states
    R0 = residual(base, g, W)
    mrf = turbo_channel_case(5, 4, 4, solver_name="DARhoSimpleFoam", perturb=0.02)
    tur = turbo_channel_case(5, 4, 4, mrf=False, perturb=0.02)
    trn = turbo_channel_case(5, 4, 4, mrf=False, transonic=True, perturb=0.02)
    Rm, Rt, Rn = residual(mrf, g, W), residual(tur, g, W), residual(trn, g, W)
    b = dict(blocks(base, g))
    assert relerr(Rm[b["U"]], R0[b["U"]]) > 1e-3 and relerr(Rm[b["phi"]], R0[b["phi"]]) > 1e-3  # Coriolis, relative flux
    assert np.array_equal(Rt[b["U"]], R0[b["U"]]) and np.array_equal(Rt[b["nuTilda"]], R0[b["nuTilda"]])
    assert relerr(Rt[b["T"]], R0[b["T"]]) > 1e-6  # viscous work
    assert relerr(Rt[b["p"]], R0[b["p"]]) > 1e-6 and relerr(Rn[b["p"]], Rt[b["p"]]) > 1e-6  # SIMPLEC form / transonic form
    # rotating hub: U_b = Omega x r on the included fixedValue wall shows up in the wall-adjacent momentum residual
    own_bottom = g.own[g.patch_slices()["bottom"].start + g.nIF : g.patch_slices()["bottom"].stop + g.nIF]
    assert np.abs((Rm - R0)[: 3 * g.nC].reshape(-1, 3)[own_bottom]).max() > 0


def test_openfoam_case_io_roundtrip(tmp_path):
    """constant/polyMesh + 0/ fields written and read back as OpenFOAM ASCII: mesh arrays bit-identical, BC table
    and cell states identical, oracle residual unchanged (boundary phi of the reader comes from the patch fields)."""
    from dafoam_amd import foam_io

    case = channel_case(5, 4, 3, wall_function=True)
    d = str(tmp_path / "case")
    foam_io.write_case(d, case)
    txt = open(os.path.join(d, "constant", "polyMesh", "boundary")).read()
    assert "startFace" in txt and "FoamFile" in txt
    back = foam_io.read_case(d, y_wall=case.y_wall)
    m0, m1 = case.mesh, back.mesh
    assert np.array_equal(m0.points, m1.points) and np.array_equal(m0.face_pts, m1.face_pts) and np.array_equal(m0.face_ptr, m1.face_ptr)
    assert np.array_equal(m0.owner, m1.owner) and np.array_equal(m0.neighbour, m1.neighbour)
    assert [(p.name, p.type, p.start, p.size) for p in m0.patches] == [(p.name, p.type, p.start, p.size) for p in m1.patches]
    for pt in m0.patches:
        for f in ("U", "p", "nuTilda", "nut"):
            a, b = case.bcs[pt.name][f], back.bcs[pt.name][f]
            assert a[0] == b[0] and (a[0] not in (0, 2) or np.allclose(np.atleast_1d(a[1]), np.atleast_1d(b[1]))), (pt.name, f)
    N, nIF = m0.n_cells, m0.n_internal_faces
    # the FULL state vector incl. the boundary-face fluxes (phi boundaryField written and parsed), and the oracle residual
    assert np.array_equal(case.states, back.states)
    from oracle.foam_mesh import Geometry
    from oracle.residual import residual

    assert np.array_equal(residual(case, Geometry(case.mesh), case.states), residual(back, Geometry(back.mesh), back.states))
    # without a phi file the boundary fluxes come from the patch velocities (createPhi); a uniform phi parses; restart-style
    # patch values (nonuniform / $internalField) are accepted where the patch type does not consume them
    os.remove(os.path.join(d, "0", "phi"))
    nophi = foam_io.read_case(d, y_wall=case.y_wall)
    assert np.abs(nophi.states[5 * N + nIF:]).max() > 0
    with open(os.path.join(d, "0", "phi"), "w") as f:
        f.write("FoamFile { version 2.0; format ascii; class surfaceScalarField; object phi; }\ninternalField uniform 0;\nboundaryField { }\n")
    assert np.all(foam_io.read_case(d, y_wall=case.y_wall).states[5 * N: 5 * N + nIF] == 0.0)
    assert foam_io._bc_entry({"type": "zeroGradient", "value": foam_io._parse_value("nonuniform List<scalar> 2 (1 2)", 1)}, False)[0] == 1
    with pytest.raises(NotImplementedError):
        foam_io._bc_entry({"type": "fixedValue", "value": foam_io._parse_value("$internalField", 1)}, False)
    with pytest.raises(NotImplementedError):
        foam_io._bc_entry({"type": "codedFixedValue"}, False)


def test_wall_distance_exact_finite_plate():
    """The reader's wall distance is the Euclidean distance to the nearest wall-face polygon: cells beside a
    finite wall do not collapse onto the wall's tangent plane."""
    from dafoam_amd.meshgen import _InputGeometry, wall_distance, wall_distance_exact

    case = channel_case(8, 4, 3)
    m = case.mesh
    g = _InputGeometry(m)
    for pt in m.patches:  # keep only the first half of the bottom wall as "wall": a finite plate
        if pt.type == "wall" and pt.name != "bottom":
            pt.type = "patch"
    bottom = next(pt for pt in m.patches if pt.name == "bottom")
    faces = np.arange(bottom.start, bottom.start + bottom.size)
    xmid = np.median(g.Cf[faces, 0])
    keep = faces[g.Cf[faces, 0] < xmid]
    keep = keep[: int(np.argmax(np.diff(keep) != 1)) + 1] if np.any(np.diff(keep) != 1) else keep  # a contiguous run = one patch
    y = wall_distance_exact(m, g.C, g.Cf, g.Sf)
    # brute force: distance to the plate polygon set = min over kept faces of the exact point-polygon distance
    import copy

    m2 = copy.copy(m)
    m2.patches = [copy.copy(pt) for pt in m.patches]
    # emulate the finite plate by comparing against a dense sampling of the kept faces
    from scipy.spatial import cKDTree

    samples = []
    for f in keep:
        v = m.points[m.face_pts[m.face_ptr[f]:m.face_ptr[f + 1]]]
        s, t = np.meshgrid(np.linspace(0, 1, 21), np.linspace(0, 1, 21))
        samples.append(((1 - s)[..., None] * ((1 - t)[..., None] * v[0] + t[..., None] * v[1]) + s[..., None] * ((1 - t)[..., None] * v[3] + t[..., None] * v[2])).reshape(-1, 3))
    d_samp, _ = cKDTree(np.concatenate(samples)).query(g.C)
    # restrict the library call to the plate
    bottom.type = "patch"
    assert np.all(np.diff(keep) == 1)
    m.patches.append(type(bottom)("plate", "wall", int(keep.min()), int(keep.size)))
    y = wall_distance_exact(m, g.C, g.Cf, g.Sf, k=keep.size)
    assert np.all(y <= d_samp + 1e-12) and np.all(y >= d_samp - 0.08 * d_samp.max())
    far = g.C[:, 0] > xmid + 0.2 * (g.C[:, 0].max() - xmid)
    yproj = wall_distance(m, g.C, g.Cf, g.Sf)
    assert np.any(yproj[far] < 0.5 * y[far])  # the projected distance underestimates beside the plate, the exact one does not


def test_naca0012_ogrid_generator():
    """BASELINE configs[1] mesh family: single-block O-grid around a closed NACA0012 with geometric wall-normal stretching
    and a merged branch cut (ordinary internal faces).  Closed cells, positive volumes, OpenFOAM face ordering, true wall
    distance; the kernel bodies (host emulation) match the oracle residual on it."""
    from dafoam_amd.meshgen import naca0012_case

    case = naca0012_case(48, 14, 1, first_cell=2e-3, radius=8.0, wall_function=True)
    m = case.mesh
    g = Geometry(m)
    N, nIF = m.n_cells, m.n_internal_faces
    assert N == 48 * 14 and [p.name for p in m.patches] == ["airfoil", "farfield", "front", "back"]
    acc = np.zeros((N, 3))
    np.add.at(acc, m.owner, g.Sf)
    np.subtract.at(acc, m.neighbour, g.Sf[:nIF])
    assert np.abs(acc).max() < 1e-12 * np.abs(g.Sf).max() and g.V.min() > 0
    assert np.all(m.owner[:nIF] < m.neighbour) and np.array_equal(np.lexsort((m.neighbour, m.owner[:nIF])), np.arange(nIF))
    wall = next(p for p in m.patches if p.name == "airfoil")
    first = np.abs(np.einsum("ij,ij->i", g.C[m.owner[wall.start:wall.start + wall.size]] - g.Cf[wall.start:wall.start + wall.size],
                             g.Sf[wall.start:wall.start + wall.size] / np.linalg.norm(g.Sf[wall.start:wall.start + wall.size], axis=1)[:, None]))
    assert np.allclose(case.y_wall[m.owner[wall.start:wall.start + wall.size]], first, rtol=0.05)  # wall cells: y = half the first cell height
    assert case.y_wall.max() > 5.0  # far-field cells see the Euclidean distance to the airfoil, not a tangent-plane projection
    W = case.states
    Ro = residual(case, g, W)
    Rv, _ = _emu_res(case, W, 0)
    for nm, sl in blocks(case, g):
        assert relerr(Rv[sl], Ro[sl]) < 1e-10, nm


def test_parity_tool_roundtrip_oracle(tmp_path):
    """tests/parity_from_dafoam_dump.py: this repo's own dumps in the reference's on-disk formats (OpenFOAM ASCII case,
    PETSc-binary dRdWT / dRdWTPC / colouring, adjoint_* fields) read back and compared - every block within tolerance."""
    import parity_from_dafoam_dump as P

    case_dir = P.write_self_dump(str(tmp_path), engine="oracle", dims=(5, 4, 3))
    ok, rows = P.compare(case_dir, str(tmp_path), engine="oracle", tol=1e-8, verbose=False)
    assert ok, [r for r in rows if not r[2]]
    assert any(r[0].startswith("psi[") for r in rows) and any("colouring" in r[0] for r in rows)


def test_pc_node_structure_levels_and_pattern():
    """Host side of the node-block ILU (das_bilu.hpp): every unknown sits in one slot, the node pattern holds every entry of
    the PC connectivity except late-late couplings, and the processing (level) order keeps all coupled nodes in their natural
    relative order - the condition under which the ticketed sweeps cannot deadlock and the factorisation equals the
    natural-order one."""
    case = channel_case(12, 10, 8, grading_y=1.5)
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    s.runColoring()
    S = s.pcStructure()
    nu, bptr, bcol, nat = S["nodeUnk"], S["bptr"], S["bcol"], S["natural"]
    n, nN = case.states.size, nu.shape[0]
    lev = np.repeat(np.arange(S["lvlPtr"].size - 1), np.diff(S["lvlPtr"]))
    assert np.array_equal(np.sort(nu[nu >= 0]), np.arange(n))
    assert np.array_equal(np.sort(nat), np.arange(nN)) and lev.size == nN
    rows = np.repeat(np.arange(nN), np.diff(bptr))
    lower, upper = bcol < rows, bcol > rows
    assert np.all(lev[bcol[lower]] < lev[rows[lower]]) and np.all(nat[bcol[lower]] < nat[rows[lower]])
    assert np.all(lev[bcol[upper]] > lev[rows[upper]]) and np.all(nat[bcol[upper]] > nat[rows[upper]])
    # pattern coverage: the PC connectivity, mapped to nodes
    node_of = np.empty(n, np.int64)
    node_of[nu[nu >= 0]] = np.nonzero(nu >= 0)[0]
    con = s.getConnectivity(1).tocoo()
    have = set(zip(rows.tolist(), bcol.tolist()))
    nPrimary = int(np.sum(np.any((nu >= 0) & (nu < n - case.mesh.n_faces), axis=1)))
    late = nat >= nPrimary
    missing = [(a, b) for a, b in set(zip(node_of[con.row].tolist(), node_of[con.col].tolist())) if (a, b) not in have]
    assert all(late[a] and late[b] for a, b in missing)


def test_amd_option_defaults_and_profile_helpers(tmp_path):
    """The MI355X-specific option table (mirror and library agree on the defaults that select the measured code paths), and
    the two host helpers around the PMC evidence: tools/pmc_summary.py and bench.pmc_traffic."""
    import importlib.util
    import json
    import subprocess
    import sys

    from dafoam_amd.pyDAFoam import DAOPTION

    d = DAOPTION()
    assert d.amd["gmresOrthogonalization"] == "dcgs2" and d.amd["pcType"] == "bilu" and d.amd["pcCoarseMode"] == "deflated" and d.amd["pcUpwindBlend"] == 0.5
    case = channel_case(4, 4, 3)
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    buf = C.create_string_buffer(64)
    if hasattr(_capi.lib(), "das_get_option_string"):
        _capi.check(_capi.lib().das_get_option_string(s._h, b"amd.gmresOrthogonalization", buf, 64))
        assert buf.value == b"dcgs2"
    # pmc_summary: two passes (one counter each), KB units, bytes = 2 x FETCH + WRITE
    for ctr, vals in (("FETCH_SIZE", (1000.0, 3000.0)), ("WRITE_SIZE", (100.0, 300.0))):
        dd = tmp_path / ctr / "host" / "1"
        dd.mkdir(parents=True)
        with open(dd / "pmc_counter_collection.csv", "w") as f:
            f.write('"Correlation_Id","Kernel_Name","Counter_Name","Counter_Value"\n')
            for i, v in enumerate(vals):
                f.write(f'{i},"k_a","{ctr}",{v}\n')
            f.write(f'9,"k_b","{ctr}",5.0\n')
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "pmc_summary.py"), str(tmp_path / "FETCH_SIZE"), str(tmp_path / "WRITE_SIZE")])
    summ = json.loads(out)
    assert summ["k_a"]["FETCH_SIZE_KB_avg"] == 2000.0 and summ["k_a"]["launches_WRITE_SIZE"] == 2
    assert summ["k_a"]["hbm_bytes_per_launch_corrected"] == (2 * 2000.0 + 200.0) * 1024.0
    # bench.pmc_traffic: the committed passes are reported only for the workload they were taken on
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t = bench.pmc_traffic(2091189176, "spmv")  # round 3: k_spmv_vec3 (packed U rows) + k_spmv_wave (scalar rows) per product
    assert t is not None and 2.2e10 < t < 3.2e10
    assert bench.pmc_traffic(12345, "spmv") is None and bench.pmc_traffic(2091189176, "no_such_kernel") is None


@pytest.mark.parametrize("variant", ["translational", "turbo_sector"])
@pytest.mark.parametrize("world", [2, 4])
def test_cyclic_aware_partition_extended_submesh_residuals(variant, world):
    """Multi-GPU partitioner with coupled cyclic pairs (BASELINE configs[4]: DATurboFoam, cyclic + MRF, 8 ranks): the ghost
    rings of extract_submesh run THROUGH the pairs, pairs whose two cells are in the extended set stay cyclic pairs of the
    sub-mesh (a pair may be split between ranks - the partner is then a ghost cell), the others are cut.  For every rank of
    an RCB partition the residual rows of the OWNED cells / faces evaluated on the extended sub-mesh (host-emulated kernel
    bodies, which carry the cyclic implementation) equal the rows of the undecomposed periodic case; the owned states
    partition the global vector.  With decomposeParDict.preservePatches (reference pyDAFoam.py:597-604) every pair lies on
    one rank."""
    from dafoam_amd.distributed import extract_submesh, preserve_patches, rcb_partition

    kw = {} if variant == "translational" else dict(sector=(0.5, 0.12), solver_name="DATurboFoam", mrf_omega=60.0)
    gcase = periodic_channel_case(8, 5, 6, wall_function=True, **kw)
    gg = Geometry(gcase.mesh)
    Rg, _ = _emu_res(gcase, gcase.states, 0)
    nx, ny, nz = 8, 5, 6
    cidx = np.arange(gcase.mesh.n_cells)
    ci, ck = cidx % nx, cidx // (nx * ny)
    sl = {p.name: np.arange(p.start, p.start + p.size) for p in gcase.mesh.patches}
    fo, bo = gcase.mesh.owner[sl["front"]], gcase.mesh.owner[sl["back"]]
    for mode in ("rcb", "split_pairs", "preserve"):
        if mode == "rcb":
            part = rcb_partition(gg.C, world)
        else:  # cut across the periodic direction: every pair is split between two ranks
            part = ((ck >= nz // 2).astype(np.int32) + (2 * (ci >= nx // 2).astype(np.int32) if world == 4 else 0)).astype(np.int32)
            assert np.all(part[fo] != part[bo])
            if mode == "preserve":
                part = preserve_patches(gcase, part, ["front", "back"])
                assert np.array_equal(part[fo], part[bo])
        seen = np.zeros(gcase.states.size, dtype=int)
        for rank in range(world):
            case, info = extract_submesh(gcase, part, rank)
            owned, key = info["owned"], info["key"]
            pf, pb = [p for p in case.mesh.patches if p.name in ("front", "back")]
            assert pf.size == pb.size and pf.type == pb.type == "cyclic"
            R, _ = _emu_res(case, case.states, 0)
            ref = Rg[key] * info["state_sign"]
            assert np.abs(R[owned] - ref[owned]).max() <= 1e-11 * np.abs(Rg).max(), (variant, world, mode, rank)
            seen[key[owned]] += 1
        assert np.all(seen == 1)


def test_field_input_betaFINuTilda_kernel_bodies_vs_oracle():
    """`field` input (reference DAInputField.C) betaFINuTilda - the field-inversion multiplier of the SA production term
    (DASpalartAllmaras.C:445-485): residual with a non-trivial field, and the tangent w.r.t. the field (the seeds of
    das_calc_dfield_product) against the oracle's complex step.  A residual row depends on the value of its own cell only."""
    case = channel_case(6, 5, 4, wall_function=True)
    g = Geometry(case.mesh)
    N = g.nC
    rng = np.random.default_rng(3)
    case.beta_fi = 1.0 + 0.3 * rng.standard_normal(N)
    Rv, _ = _emu_res(case, case.states, 0)
    Ro = residual(case, g, case.states)
    for nm, sl in blocks(case, g):
        assert relerr(Rv[sl], Ro[sl]) < 1e-12, nm
    c1 = channel_case(6, 5, 4, wall_function=True)
    assert relerr(Rv[4 * N : 5 * N], residual(c1, g, c1.states)[4 * N : 5 * N]) > 1e-3  # the field does act on nuTildaRes
    t = rng.standard_normal(N)
    L = _emu()
    L.emu_residual_field.argtypes = [C.POINTER(das_case_t), _capi.c_double_p, C.c_longlong, _capi.c_double_p, _capi.c_double_p]
    Rd = np.zeros(case.states.size)
    cs = CaseStruct(case)
    assert L.emu_residual_field(cs.byref(), dptr(case.states), case.states.size, dptr(t), dptr(Rd)) == 0
    import copy

    cc = copy.copy(case)
    cc.beta_fi = case.beta_fi + 1e-30j * t
    cs = residual(cc, g, case.states.astype(complex)).imag / 1e-30
    assert relerr(Rd, cs) < 1e-12
    assert np.all(Rd[: 4 * N] == 0.0) and np.all(Rd[5 * N :] == 0.0)  # only the cell's own nuTildaRes row


def _rows_of_cells(case, cells):
    """state-ordered rows owned by `cells`: their cell-centred rows and the phi rows of the faces they own"""
    m = case.mesh
    N, nF = m.n_cells, m.n_faces
    own = np.zeros(N, bool)
    own[cells] = True
    mask = []
    n = case.states.size
    ncellblocks = (n - nF - 3 * N) // N
    mask.append(np.repeat(own, 3))
    for _ in range(ncellblocks):
        mask.append(own)
    mask.append(own[np.asarray(m.owner)[:nF]])
    return np.concatenate(mask)


@pytest.mark.parametrize("kind", ["simple_wf", "rho", "turbo_cyclic"])
def test_point_influence_sets_cover_every_dependency_and_colouring_is_valid(kind):
    """Structure behind calcJacTVecProduct(volCoord -> ...): (1) brute force - moving ONE point changes no residual row outside
    the rows of its influence set (kernel bodies on the CPU, every point of a small mesh, all three axes); (2) two points of one
    colour have disjoint influence sets; (3) the steps are a fixed fraction of the smallest adjacent cell thickness."""
    import copy

    if kind == "simple_wf":
        case = channel_case(13, 11, 10, wall_function=True, bump=0.1, skew=0.05)
        name, norm = "DASimpleFoam", NORM_STATES
    elif kind == "rho":
        case = rho_channel_case(11, 10, 9, wall_function=True)
        name, norm = "DARhoSimpleFoam", NORM_STATES_RHO
    else:  # rotational cyclic pair + MRF: influence sets run through the pair
        case = periodic_channel_case(11, 10, 9, wall_function=True, sector=(0.5, 0.12), solver_name="DATurboFoam", mrf_omega=60.0)
        name, norm = "DATurboFoam", NORM_STATES_RHO
    s = pyDASolvers(f"{name} -python".encode(), options(case, normalizeStates=norm), case=case)
    I = s.pointInfluence()
    assert np.diff(I["ptr"]).max() < 0.25 * case.mesh.n_cells  # the sets are local: the brute-force check below discriminates
    P, N = case.mesh.n_points, case.mesh.n_cells
    assert I["colors"].min() >= 0 and I["nColors"] == I["colors"].max() + 1
    # (2) per colour, every cell is claimed by at most one point
    for c in range(I["nColors"]):
        pts = np.nonzero(I["colors"] == c)[0]
        cells = np.concatenate([I["cells"][I["ptr"][p]:I["ptr"][p + 1]] for p in pts])
        assert np.unique(cells).size == cells.size, f"colour {c}: overlapping influence sets"
    # (3)
    g = Geometry(case.mesh)
    assert np.all(I["steps"] > 0) and I["steps"].max() <= 1e-4 * np.cbrt(g.V.max()) * 1.0001
    # (1)
    W = case.states
    R0, _ = _emu_res(case, W)
    rng = np.random.default_rng(0)
    pts = rng.choice(P, 50, replace=False)
    with_two = pyDASolvers(f"{name} -python".encode(), options(case, normalizeStates=norm, amd={"volCoordRings": 2}), case=case).pointInfluence()
    escaped = 0
    for p in pts:
        inside = _rows_of_cells(case, I["cells"][I["ptr"][p]:I["ptr"][p + 1]])
        for ax in range(3):
            c2 = copy.copy(case)
            c2.mesh = copy.copy(case.mesh)
            X = np.array(case.mesh.points, dtype=np.float64).reshape(-1, 3).copy()
            X[p, ax] += 50.0 * I["steps"][p]
            c2.mesh.points = X
            R1, _ = _emu_res(c2, W)
            changed = R1 != R0
            assert not np.any(changed & ~inside), f"point {p} axis {ax}: a row outside the influence set changed"
            assert np.any(changed), f"point {p} axis {ax}: nothing changed"
            escaped += int(np.any(changed & ~_rows_of_cells(case, with_two["cells"][with_two["ptr"][p]:with_two["ptr"][p + 1]])))
    assert escaped > 0  # ... and three rings are needed: two-ring sets miss rows (the pRes table reaches level 3)


def test_case_discretisation_is_read_and_verified(tmp_path):
    """system/fvSolution is honoured (equation relaxation factors incl. quoted regular-expression keys, SIMPLE consistent /
    transonic), system/fvSchemes is verified against the ONE scheme set the kernels implement (the reference
    builds its operators through the run-time selected schemes of the case, DAResidualSimpleFoam.C:123-132): a case asking
    for anything else is rejected with the offending entries, not run with other numerics."""
    from dafoam_amd import foam_io

    case = channel_case(4, 3, 3, wall_function=True)
    case.relax = {"U": 0.8, "nuTilda": 0.6, "T": 1.0}
    case.simple_consistent = True
    d = str(tmp_path)
    foam_io.write_case(d, case)
    sch = foam_io.read_fv_schemes(d)
    assert sch["divSchemes"]["div(phi,U)"] == "bounded Gauss linearUpwindV grad(U)" and foam_io.check_schemes(sch) == []
    back = foam_io.read_case(d, y_wall=case.y_wall)
    assert back.relax["U"] == 0.8 and back.relax["nuTilda"] == 0.6 and back.simple_consistent and not back.transonic
    # the relaxation factor reaches the residual: the kernel bodies on the re-read case equal the oracle with the same factors
    g = Geometry(back.mesh)
    Rv, _ = _emu_res(back, back.states)
    assert relerr(Rv, residual(back, g, back.states)) < 1e-12
    c07 = channel_case(4, 3, 3, wall_function=True)
    assert relerr(_emu_res(c07, c07.states)[0], Rv) > 1e-3
    # a tutorial-style fvSolution: regular-expression keys, field relaxation of p present but not used by the residual
    with open(os.path.join(d, "system", "fvSolution"), "w") as f:
        f.write('FoamFile { version 2.0; format ascii; class dictionary; object fvSolution; }\n'
                'solvers { "(p|p_rgh)" { solver GAMG; tolerance 1e-8; } }\n'
                'SIMPLE { nNonOrthogonalCorrectors 0; consistent no; transonic yes; }\n'
                'relaxationFactors { fields { p 0.3; } equations { "(U|T|nuTilda)" 0.75; } } // comment\n')
    sol = foam_io.read_fv_solution(d)
    assert sol["relax"] == {"U": 0.75, "nuTilda": 0.75, "T": 0.75} and sol["relax_fields"] == {"p": 0.3} and sol["transonic"] and not sol["consistent"]
    # other schemes: rejected, with names
    text = open(os.path.join(d, "system", "fvSchemes")).read()
    with open(os.path.join(d, "system", "fvSchemes"), "w") as f:
        f.write(text.replace("div(phi,nuTilda) bounded Gauss upwind", "div(phi,nuTilda) bounded Gauss linearUpwind grad(nuTilda)")
                .replace("default Gauss linear corrected", "default Gauss linear limited 0.33"))
    with pytest.raises(NotImplementedError, match=r"divSchemes/div\(phi,nuTilda\).*laplacianSchemes/default"):
        foam_io.read_case(d, y_wall=case.y_wall)
    lax = foam_io.read_case(d, y_wall=case.y_wall, strict_schemes=False)
    assert len(lax.scheme_mismatches) == 2


def test_api_surface_methods_around_the_hot_path(tmp_path):
    """The small methods of the reference's pyDASolvers class a runScript / mphys_dafoam.py calls around solve_linear
    (pyDASolvers.pyx:198-206,283-303,320,361-410,464-468): distributed flags, calcOutput sizes, getOFField, getGlobalXvIndex,
    checkMesh with the checkMeshThreshold option, mesh-point and state files, primalBC."""
    case = channel_case(6, 5, 4, wall_function=True)
    opts = options(case, inputInfo={"aero_vol_coords": {"type": "volCoord", "components": ["solver", "function"]},
                                    "patchV": {"type": "patchVelocity", "patches": ["inlet"], "flowAxis": "x", "normalAxis": "y", "components": ["solver"]}},
                   primalBC={"U0": {"variable": "U", "patches": ["inlet"], "value": [12.0, 0.5, 0.0]}})
    s = pyDASolvers(b"DASimpleFoam -python", opts, case=case)
    N, P = case.mesh.n_cells, case.mesh.n_points
    assert s.hasVolCoordInput() == 1 and pyDASolvers(b"DASimpleFoam -python", options(case), case=case).hasVolCoordInput() == 0
    assert s.getInputDistributed("aero_vol_coords", "volCoord") == 1 and s.getInputDistributed("patchV", "patchVelocity") == 0
    assert s.getOutputDistributed("residual", "residual") == 1 and s.getOutputDistributed("CD", "function") == 0
    assert s.getInputSize("aero_vol_coords", "volCoord") == 3 * P and s.getGlobalXvIndex(7, 2) == 23
    U, p = np.zeros(3 * N), np.zeros(N)
    s.getOFField("U", "vector", U)
    s.getOFField("p", "scalar", p)
    assert np.array_equal(U, case.states[:3 * N]) and np.array_equal(p, case.states[3 * N:4 * N])
    with pytest.raises(_capi.DASError):
        s.getOFField("phi", "scalar", p)
    # checkMesh: the generated channel passes; a folded mesh and a tight threshold do not
    assert s.checkMesh() == 1 and s.meshQuality["incorrectlyOrientedFaces"] == 0 and 0 < s.meshQuality["maxNonOrth"] < 70
    tight = pyDASolvers(b"DASimpleFoam -python", options(case, checkMeshThreshold={"maxNonOrth": 0.5 * s.meshQuality["maxNonOrth"], "maxSkewness": 4.0,
                                                                                   "maxAspectRatio": 1000.0, "maxIncorrectlyOrientedFaces": 0}), case=case)
    assert tight.checkMesh() == 0
    # mesh points through files: write, move, read back
    s.caseDir = str(tmp_path)
    X0 = np.zeros(3 * P)
    s.getOFMeshPoints(X0)
    s.writeMeshPoints(X0 * 1.01, 3)
    s.readMeshPoints(3)
    X1 = np.zeros(3 * P)
    s.getOFMeshPoints(X1)
    assert np.allclose(X1, 1.01 * X0, rtol=1e-15)
    s.writeCurrentMeshPointsToConstant()
    s.writeFailedMesh()
    assert os.path.exists(os.path.join(str(tmp_path), "constant", "polyMesh", "points")) and os.path.exists(os.path.join(str(tmp_path), "9999", "polyMesh", "points"))
    # state files of a time directory
    from dafoam_amd import foam_io

    c2 = channel_case(6, 5, 4, wall_function=True, perturb=0.05, seed=3)
    foam_io.write_case(str(tmp_path), c2, time="100")
    s.readStateVars(100)
    W = np.zeros(case.states.size)
    s.getOFFields(W)
    assert np.array_equal(W[:5 * N], c2.states[:5 * N]) and np.array_equal(W[5 * N:], case.states[5 * N:])
    # time bookkeeping of the steady solvers
    s.setTime(500.0, 500)
    assert s.getLatestTime() == 500.0 and s.getDeltaT() == 1.0 and s.getdFScaling("CD") == 1.0 and s.getDdtSchemeOrder() == 1


def test_surface_families_for_geometry_and_warping_tools():
    """The family machinery pyGeo / IDWarp / mphys use around the solver (reference pyDAFoam.py:941-1125,1553-1800): basic
    families = patches with their unique points and faces in reduced numbering, the allSurfaces / allWalls / designSurfaces
    groups, surface coordinates and connectivity in the group's concatenated numbering, the triangulated surface for
    DVConstraints, mapVector between groups, and the hand-over to a warping object (setMesh / setSurfaceCoordinates)."""
    from dafoam_amd.pyDAFoam import PYDAFOAM, Error

    case = channel_case(5, 4, 3, wall_function=True, bump=0.1)
    D = PYDAFOAM(options=options(case, designSurfaces=["bottom"]), case=case, initSolver=False)
    m = case.mesh
    assert D.basicFamilies == sorted(p.name for p in m.patches) and sorted(D.wallList) == ["bottom", "top"]
    assert D.families["allWalls"] == sorted(D.families["bottom"] + D.families["top"]) and D.families["designSurfaces"] == D.families["bottom"]
    # coordinates + connectivity reproduce every wall face
    xs = D.getSurfaceCoordinates()
    conn, sizes = D.getSurfaceConnectivity()
    walls = [p for p in sorted(m.patches, key=lambda q: q.name) if p.type == "wall"]
    assert len(sizes) == sum(p.size for p in walls) and xs.shape == (D._getSurfaceSize("allWalls")[0], 3)
    c, k = 0, 0
    for p in walls:
        for f in range(p.start, p.start + p.size):
            ref = m.points[m.face_pts[m.face_ptr[f]:m.face_ptr[f + 1]]]
            assert np.array_equal(xs[conn[c:c + sizes[k]]], ref)
            c += sizes[k]
            k += 1
    # triangulated surface: the fan areas add up to the wall area
    p0, v1, v2 = D.getTriangulatedMeshSurface("bottom")
    g = Geometry(m)
    bot = next(p for p in m.patches if p.name == "bottom")
    area = 0.5 * np.linalg.norm(np.cross(np.array(v1), np.array(v2)), axis=1).sum()
    assert abs(area - np.linalg.norm(g.bSf[bot.start - g.nIF: bot.start - g.nIF + bot.size], axis=1).sum()) < 1e-12 * area
    # mapVector: allWalls -> designSurfaces keeps the bottom part, back again zero-fills the top part
    a = np.arange(xs.size, dtype=float).reshape(-1, 3)
    nb = D._getSurfaceSize("bottom")[0]
    low = D.mapVector(a, "allWalls", "designSurfaces")
    assert low.shape == (nb, 3) and np.array_equal(low, a[:nb])
    up = D.mapVector(low, "designSurfaces", "allWalls")
    assert np.array_equal(up[:nb], a[:nb]) and np.all(up[nb:] == 0)
    with pytest.raises(Error):
        D.addFamilyGroup("allWalls", ["bottom"])
    with pytest.raises(Error):
        D.addFamilyGroup("g", ["nonexistent"])
    D.addFamilyGroup("io", ["inlet", "outlet"])
    assert D._getSurfaceSize("io")[1] == 2 * 4 * 3

    # a warping object receives indices, surface definition and new surface coordinates
    class Warp:
        def setExternalMeshIndices(self, ind): self.ind = ind
        def setSurfaceDefinition(self, pts, conn, sizes): self.defn = (pts.copy(), list(conn), list(sizes))
        def setSurfaceCoordinates(self, pts): self.surf = pts.copy()

    w = Warp()
    D.setMesh(w)
    assert np.array_equal(w.ind, np.arange(3 * m.n_points)) and np.array_equal(w.defn[0], xs)
    D.setSurfaceCoordinates(low + 1.0, "designSurfaces")
    assert np.array_equal(w.surf[:nb], low + 1.0) and np.array_equal(w.surf[nb:], xs[nb:])
    D.setVolCoords(1.5 * m.points.ravel())
    assert np.array_equal(D.getSurfaceCoordinates(), 1.5 * xs)


@pytest.mark.parametrize("kind", ["simple_wf", "simple_T", "rho", "turbo_cyclic_mrf", "scalar"])
def test_dual_number_metrics_give_the_exact_mesh_derivative(kind):
    """The kernel bodies are templated on the scalar of the METRICS as well (csrc/das_kernels.hpp: DevMeshT<G>, das_geom.hpp
    bodies on Dual<1> points): with T = G = Dual<1> one pass gives dR/dX . dX exactly - the forward-mode counterpart of the
    reference's reverse sweep through the mesh metrics (DASolver.C:1690-1839 with DAInputVolCoord).  Checked against central
    differences of the same bodies on moved points, for every solver family.  The step is tiny on purpose: the residual is only
    piecewise smooth in the coordinates (the V-limiter of linearUpwindV, upwind switches) and a difference across a kink that
    lies 1e-4 cell sizes away is off by tens of per cent at that cell - the dual numbers give the derivative AT the point."""
    import copy

    if kind == "simple_wf":
        case = channel_case(6, 5, 4, wall_function=True, bump=0.1, skew=0.05)
    elif kind == "simple_T":
        case = simple_T_channel_case(6, 5, 4, wall_function=True)
    elif kind == "rho":
        case = rho_channel_case(6, 5, 4, wall_function=True)
    elif kind == "turbo_cyclic_mrf":
        case = periodic_channel_case(6, 5, 5, wall_function=True, sector=(0.5, 0.12), solver_name="DATurboFoam", mrf_omega=60.0)
    else:
        case = scalar_transport_case()
    L = _emu()
    L.emu_residual_geom.argtypes = [C.POINTER(das_case_t), _capi.c_double_p, C.c_longlong, _capi.c_double_p, _capi.c_double_p]
    W = case.states
    n = W.size
    X = np.array(case.mesh.points, dtype=np.float64)
    rng = np.random.default_rng(4)
    dX = rng.standard_normal(X.shape)
    if any(pt.type == "symmetry" for pt in case.mesh.patches):
        # the symmetry planes of the generators are z = const: keep them planar.  basicSymmetry's snGradTransformDiag is |n_k|, a
        # kink at n_k = 0 - tilting the plane has a one-sided derivative only (the dual numbers take the + side, a central
        # difference averages the two)
        dX[:, 2] = 0.0
    Rd = np.zeros(n)
    cs = CaseStruct(case)  # (kept alive: the struct points into arrays the wrapper owns)
    dXc = np.ascontiguousarray(dX.ravel())
    assert L.emu_residual_geom(cs.byref(), dptr(W), n, dptr(dXc), dptr(Rd)) == 0

    def fd(h):
        out = []
        for sgn in (1.0, -1.0):
            c2 = copy.copy(case)
            c2.mesh = copy.copy(case.mesh)
            c2.mesh.points = X + sgn * h * dX
            out.append(_emu_res(c2, W)[0])
        return (out[0] - out[1]) / (2 * h)

    g = Geometry(case.mesh)
    ref = fd(1e-6 * np.cbrt(g.V.min()))
    scale = np.abs(ref).max()
    err = np.abs(Rd - ref)
    assert scale > 0 and err.max() <= 1e-5 * scale and np.percentile(err, 95) <= 1e-7 * scale, (err.max(), np.percentile(err, 95), scale)


def test_strength_based_aggregates_follow_the_stretched_cells():
    """amd.pcCoarseAggregation "strength" (opt-in; csrc/das_mesh.cpp strength_aggregates): repeated pairwise matching along the
    strongest pressure-Laplacian coupling |Sf| / |d|.  On the NACA0012 O-grid (cells 10^2 .. 10^4 times longer than thick at the
    wall) the aggregates must run along the wall normal - the direction the slow pressure modes of the adjoint are smooth in
    (tools/naca_coarse_study.py: 763 -> 360 GMRES iterations with such aggregates, 530 with space-filling blocks) - be
    deterministic, cover every cell once and respect the requested maximum."""
    from dafoam_amd.meshgen import naca0012_case

    na, nn = 64, 24
    case = naca0012_case(na, nn, 1)
    s = pyDASolvers(b"DASimpleFoam -python", options(case), case=case)
    N = case.mesh.n_cells
    agg, agg2 = np.zeros(N, np.int32), np.zeros(N, np.int32)
    cnt, cnt2 = C.c_int(0), C.c_int(0)
    L = _capi.lib()
    assert L.das_debug_strength_aggregates(s._h, 64, agg.ctypes.data_as(_capi.c_int_p), C.byref(cnt)) == 0
    assert L.das_debug_strength_aggregates(s._h, 64, agg2.ctypes.data_as(_capi.c_int_p), C.byref(cnt2)) == 0
    assert np.array_equal(agg, agg2) and cnt.value == cnt2.value
    nA = cnt.value
    assert 16 < nA <= 64 and agg.min() == 0 and agg.max() == nA - 1 and np.unique(agg).size == nA
    # shape: extent in the wall-normal index j against the extent around the airfoil (i, periodic), cell = i + na j
    i, j = np.arange(N) % na, np.arange(N) // na
    ext_j = np.array([np.ptp(j[agg == a]) + 1 for a in range(nA)])
    ext_i = []
    for a in range(nA):
        ia = np.sort(np.unique(i[agg == a]))
        gaps = np.diff(np.concatenate([ia, [ia[0] + na]]))
        ext_i.append(na - gaps.max() + 1)  # smallest periodic window that holds them
    ext_i = np.array(ext_i)
    near_wall = np.array([j[agg == a].min() == 0 for a in range(nA)])
    assert near_wall.sum() >= 8 and np.median(ext_j[near_wall] / ext_i[near_wall]) >= 3.0, (ext_j[near_wall], ext_i[near_wall])
    # sizes are balanced within the factor pairwise matching gives
    sizes = np.bincount(agg)
    assert sizes.max() <= 8 * max(1, sizes.min()) or sizes.max() <= 2 * N // nA


def test_naca_grid_sequencing_helpers():
    """dafoam_amd.workloads / meshgen helpers of the NACA0012 primal (round 4): the level list, the prolongation of a section
    solution to the next finer O-grid (exact for fields that are constant, bounded by the coarse extrema, phi rebuilt from the
    interpolated velocity) and the spanwise extrusion of a one-layer state - whose residual, layer by layer, is the one-layer
    residual (up to the spanwise diffusion coefficient in the momentum diagonal, ~1e-5 relative, through the Rhie-Chow term)."""
    from dafoam_amd.meshgen import extrude_naca_state, naca0012_case, prolong_naca_state
    from dafoam_amd.workloads import naca_levels

    assert naca_levels(800, 250) == [(100, 31), (200, 62), (400, 125), (800, 250)]
    assert naca_levels(200, 63) == [(100, 31), (200, 63)]
    assert naca_levels(64, 20) == [(64, 20)]
    c = naca0012_case(48, 16, 1, first_cell=4e-4, perturb=0.0)
    f = naca0012_case(96, 32, 1, first_cell=2e-4, perturb=0.0)
    Nc, Nf = 48 * 16, 96 * 32
    Wc = c.states.copy()
    Wc[3 * Nc : 4 * Nc] = 7.0  # a constant pressure is reproduced exactly
    Wf = prolong_naca_state((48, 16), Wc, f, (96, 32), first_cell=2e-4, coarse_first_cell=4e-4)
    assert Wf.shape == f.states.shape and np.allclose(Wf[3 * Nf : 4 * Nf], 7.0)
    Uc, Uf = Wc[: 3 * Nc].reshape(Nc, 3), Wf[: 3 * Nf].reshape(Nf, 3)
    assert Uf[:, 0].max() <= Uc[:, 0].max() + 1e-12 and Uf[:, 0].min() >= Uc[:, 0].min() - 1e-12 and np.all(Uf[:, 2] == 0.0)
    assert np.all(Wf[4 * Nf : 5 * Nf] > 0.0)
    # the interpolated smooth field is close to the generator's own field on the fine mesh (same analytic profile)
    assert np.abs(Uf - f.states[: 3 * Nf].reshape(Nf, 3)).max() < 0.25 * np.abs(Uc).max()
    f3 = naca0012_case(96, 32, 3, span=0.3, first_cell=2e-4, perturb=0.0)
    W2 = naca0012_case(96, 32, 1, first_cell=2e-4, perturb=0.02).states  # a rough state: the identity must hold for any one-layer state
    f2 = naca0012_case(96, 32, 1, first_cell=2e-4, perturb=0.0)
    W3 = extrude_naca_state(f2, W2, f3, (96, 32, 3))
    R2 = residual(f2, Geometry(f2.mesh), W2)
    R3 = residual(f3, Geometry(f3.mesh), W3)
    N2, N3 = Nf, 3 * Nf
    for k in range(3):
        assert relerr(R3[3 * k * N2 : 3 * (k + 1) * N2], R2[: 3 * N2]) < 1e-8
        assert relerr(R3[3 * N3 + k * N2 : 3 * N3 + (k + 1) * N2], R2[3 * N2 : 4 * N2]) < 1e-4
        assert relerr(R3[4 * N3 + k * N2 : 4 * N3 + (k + 1) * N2], R2[4 * N2 : 5 * N2]) < 1e-8


def test_gmres_dr_loop_host_twin():
    """amd.gmresDeflation (round 4, opt-in): GMRES with deflated restarting.  The iteration (gmres_dr_loop in csrc/das_gmres_host.hpp) is
    written once over a handful of vector operations; das_debug_gmres_dr_host runs THAT loop on host vectors - so the least-squares
    bookkeeping with the dense carried-over block, the harmonic-Ritz restart (through the dense-eigen callback the mirror installs)
    and the restart logic are tested here, and the device solver adds only kernels the undeflated solver already uses.  Checked on
    the adjoint system of a small channel: (1) the host algebra of one restart keeps the Arnoldi-like relation
    A V_k = V_{k+1} Hbar_k and the residual; (2) GMRES-DR(12, 5) reaches the sparse direct solution with fewer iterations
    than GMRES(12) restarted (almost) plainly, and not many more than full GMRES; (3) a restart length above the iteration count reproduces
    full GMRES."""
    import scipy.sparse.linalg as spla

    from oracle import linear as OL

    L = _capi.lib()
    case = channel_case(7, 6, 5)
    g = Geometry(case.mesh)
    sc = J.state_scales(case, g, NORM_STATES)
    con = J.connectivity(case, g)
    col, _ = J.greedy_coloring(con)
    A = J.jacobian_colored(case, g, case.states, con, col, sc, mode="cs", lower_bound=0).tocsr()
    n, N = A.shape[0], g.nC
    perm = np.concatenate([np.array([3 * c, 3 * c + 1, 3 * c + 2, 3 * N + c, 4 * N + c]) for c in range(N)] + [np.arange(5 * N, n)])
    import scipy.sparse as sp

    Ap = sp.csr_matrix(A[perm][:, perm])
    Ap.sort_indices()
    ilu = OL.ILU(Ap, fill=0)

    def pc(v):
        y = np.empty(n)
        y[perm] = ilu.solve(np.ascontiguousarray(v[perm]))
        return y

    rhs = np.zeros(n)
    rhs[0 : 3 * N : 3] = g.V
    rhs *= sc
    xd = spla.spsolve(A.tocsc(), rhs)
    APPLY = C.CFUNCTYPE(None, _capi.c_double_p, _capi.c_double_p, C.c_void_p)

    def wrap(f):
        def cb(xp, yp, _u):
            x = np.ctypeslib.as_array(xp, shape=(n,))
            np.ctypeslib.as_array(yp, shape=(n,))[:] = f(x)
        return APPLY(cb)

    cA, cM = wrap(lambda v: A @ v), wrap(pc)

    def solve(m, k, maxit=2000, rtol=1e-10):
        x, hist, info, res = np.zeros(n), np.zeros(maxit + 8), np.zeros(4), np.zeros(2)
        fail = L.das_debug_gmres_dr_host(n, C.cast(cA, C.c_void_p), C.cast(cM, C.c_void_p), None, dptr(rhs), dptr(x), m, k, rtol, 1e-300, maxit, dptr(hist), hist.size,
                                         dptr(info), dptr(res))
        assert fail >= 0, _capi.lib().das_last_error()
        return x, fail, info, res

    # (1) one restart's host algebra on a real Arnoldi factorisation
    m, k = 24, 8
    V, H = np.zeros((n, m + 1)), np.zeros((m + 1, m))
    beta = np.linalg.norm(rhs)
    V[:, 0] = rhs / beta
    for j in range(m):
        w = A @ pc(V[:, j])
        for _ in range(2):
            h = V[:, : j + 1].T @ w
            w -= V[:, : j + 1] @ h
            H[: j + 1, j] += h
        H[j + 1, j] = np.linalg.norm(w)
        V[:, j + 1] = w / H[j + 1, j]
    c = np.zeros(m + 1)
    c[0] = beta
    rvec = c - H @ np.linalg.lstsq(H, c, rcond=None)[0]
    P1, Hn, cn = np.zeros((m + 1) * (k + 2)), np.zeros((k + 2) * (k + 1)), np.zeros(k + 2)
    kk = L.das_debug_gmres_dr_restart(m, k, dptr(np.ascontiguousarray(H)), dptr(rvec), dptr(P1), dptr(Hn), dptr(cn))
    assert k <= kk <= k + 1
    P1, Hn, cn = P1[: (m + 1) * (kk + 1)].reshape(m + 1, kk + 1), Hn[: (kk + 1) * kk].reshape(kk + 1, kk), cn[: kk + 1]
    Vn = V @ P1
    assert np.abs(P1.T @ P1 - np.eye(kk + 1)).max() < 1e-12
    AV = np.column_stack([A @ pc(Vn[:, q]) for q in range(kk)])
    assert np.abs(AV - Vn @ Hn).max() <= 1e-10 * np.abs(AV).max()
    assert np.abs(Vn @ cn - V @ rvec).max() <= 1e-12 * beta
    # (2) the loop: deflated vs plain restarting vs full GMRES
    x_full, f_full, i_full, _ = solve(600, 1)          # never restarts: full GMRES
    x_dr, f_dr, i_dr, r_dr = solve(12, 5)
    x_pl, f_pl, i_pl, r_pl = solve(12, 1, maxit=int(3 * i_dr[0]))  # k = 1 carries almost nothing: close to plain GMRES(12)
    print("iterations: full", i_full[0], " GMRES-DR(12, 5)", i_dr[0], "deflated restarts", i_dr[1], " GMRES-DR(12, 1)", i_pl[0], "rel", r_pl[1] / r_pl[0])
    assert f_full == 0 and f_dr == 0 and i_dr[1] >= 1 and i_dr[2] == 0
    assert relerr(x_full, xd) < 1e-7 and relerr(x_dr, xd) < 1e-7
    assert i_full[0] <= i_dr[0] <= 2.0 * i_full[0] + 10
    assert i_pl[0] > 1.15 * i_dr[0] or r_pl[1] > 1e-10 * r_pl[0]
    # (3) first cycle == full GMRES: same iterates as the oracle's GMRES (CGS2) while no restart happens
    xo, io = OL.gmres(lambda v: A @ v, rhs, pc, restart=600, max_iters=600, rel_tol=1e-10, abs_tol=1e-300)
    assert abs(io["iters"] - i_full[0]) <= 1


def test_bench_cpu_leg_guards():
    """bench.py's guards around the CPU legs (round 4: a 256-thread CPU leg on a 16-CPU quota did not finish in ten minutes and took
    the JSON line with it): a leg that overruns its deadline yields an error record naming the stage and marks the run for a hard exit
    after the line is printed; a leg that raises yields an error record; the thread count honours the affinity mask."""
    import importlib.util
    import time

    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench._with_deadline(lambda: {"value": 1.0}, 5.0, "fast leg") == {"value": 1.0} and not bench._OVERRUN
    out = bench._with_deadline(lambda: 1 / 0, 5.0, "failing leg")
    assert "ZeroDivisionError" in out["error"] and not bench._OVERRUN
    bench._CPU_STAGE[0] = "somewhere"
    out = bench._with_deadline(lambda: time.sleep(1.0) or {"value": 2.0}, 0.05, "slow leg")
    assert "slow leg" in out["error"] and "somewhere" in out["error"] and bench._OVERRUN == ["slow leg"]
    from oracle.linear import available_cpus

    assert 1 <= bench._cpu_threads() == available_cpus() <= len(os.sched_getaffinity(0))


def test_bench_passes_no_preconditioner_option_by_default(monkeypatch):
    """`bench.py` must pass no PC option the library would not pick itself.  With the default command line the
    `amd` dict of the options holds the Krylov memory budget only; the library's own defaults are the ones the wing needs
    (`amd.pcUpwindBlend 0.5`, deflated coarse mode - DAOPTION and the C++ Options agree); `--amd`, `--pc-blend`, `--coarse-mode`,
    `--solver` reach the options; the PMC traffic of the stated workload is found for the `roofline` objects."""
    import importlib.util
    import sys

    spec = importlib.util.spec_from_file_location("bench_mod3", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    o = bench.make_opts(a, 0, 1000, 1000, 1e-6)
    assert sorted(o["amd"]) == ["maxKrylovBytes"] and o["solverName"] == "DASimpleFoam" and a.workload == "naca" and a.naca == [200, 63, 160]
    monkeypatch.setattr(sys, "argv", ["bench.py", "--amd", "gradFaceParallel=0", "--amd", "krylovBasisPrecision=fp64", "--pc-blend", "0.2", "--coarse-mode", "additive",
                                      "--solver", "DARhoSimpleFoam"])
    a = bench.parse()
    o = bench.make_opts(a, 0, 1000, 1000, 1e-6)
    assert o["amd"]["gradFaceParallel"] == 0 and o["amd"]["krylovBasisPrecision"] == "fp64" and o["amd"]["pcUpwindBlend"] == 0.2 and o["amd"]["pcCoarseMode"] == "additive"
    assert o["solverName"] == "DARhoSimpleFoam" and "T" in o["normalizeStates"]
    from dafoam_amd.pyDAFoam import DAOPTION

    d = DAOPTION()
    assert d.amd["pcUpwindBlend"] == 0.5 and d.amd["pcCoarseMode"] == "deflated"
    assert bench.pmc_traffic(2112359800, "spmv") > 2.5e10 and bench.pmc_traffic(2112359800, "k_bilu_sweep_forward") > 1.0e10 and bench.pmc_traffic(1, "spmv") is None

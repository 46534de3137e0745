"""CPU tier of DASolidDisplacementFoam: the numpy restatement (tests/solid_displacement_restatement.py) checked on its own, the kernel bodies
body_solid_grad / body_solid_traction / body_solid run on the host (tests/hostemu/hostemu_solid.cpp) against it, the connectivity of the
C++ host code, and the host-side errors."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import solid_displacement_restatement as S
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import solid_displacement_case
from dafoam_amd.meshgen import BC_TRACTION, Patch
from dafoam_amd.pyDASolvers import pyDASolvers
from solid_displacement_cases import KS_BOX, KS_COEFF, KS_SCALE, MATERIALS, MESHES, PASSES, solid_case, solid_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = _capi.c_double_p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_solid.cpp through g++, as tests/test_heat_transfer_cpu.py builds its harness."""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    so = str(tmp_path_factory.mktemp("hostemu") / "libhostemu_solid.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-o", so, os.path.join(ROOT, "tests", "hostemu", "hostemu_solid.cpp"), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L = C.CDLL(so)
    L.emu_solid_residual.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, C.c_double]
    L.emu_solid_geom.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, C.c_int, dp, dp]
    return L


def emu_residual(L, case, D, passes, isPC=0, normalized=1, direction=None, vm=None, vm_scale=1.0):
    cs = CaseStruct(case)
    D = np.ascontiguousarray(D, dtype=np.float64)
    R, Rd = np.zeros(D.size), np.zeros(D.size)
    d = None if direction is None else np.ascontiguousarray(direction, dtype=np.float64)
    assert L.emu_solid_residual(cs.byref(), dptr(D), D.size, isPC, normalized, passes, dptr(d) if d is not None else None, dptr(R), dptr(Rd),
                                dptr(vm) if vm is not None else None, vm_scale) == 0
    return (R, Rd) if direction is not None else R


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


# ---- the restatement on its own ------------------------------------------------------------------------------------------------------
def test_restatement_linear_displacement_is_a_zero_on_an_orthogonal_box():
    """A patch carries one fixedValue, so the linear field is D = (0, 0, c z): constant on front / back (fixedValue there), zero normal
    gradient on the other four patches (zeroGradient there)."""
    L = (0.7, 0.3, 0.2)
    c = 1e-4
    case = solid_displacement_case(7, 4, 3, lengths=L, mapping=None,
                                   D_bcs={"front": ("fixedValue", (0.0, 0.0, 0.0)), "back": ("fixedValue", (0.0, 0.0, c * L[2]))})
    g = S.Geom(case.mesh)
    z = g.C[:, 2]
    zlo = g.Cf[g.nIF:][g.patch_slices()["front"], 2].mean()
    if zlo > 0.5 * L[2]:  # "front" is the high-z patch of this block
        case.bcs["front"], case.bcs["back"] = case.bcs["back"], case.bcs["front"]
    D = np.stack([0.0 * z, 0.0 * z, c * z], axis=1).ravel()
    mu, lam = S.lame(case.mechanical)
    R = S.residual(case, g, D)
    h = L[2] / 3
    bound = 1e-12 * (2 * mu + lam) * c / h
    print("max |DRes|:", np.abs(R).max(), "bound:", bound)
    assert np.abs(R).max() <= bound


@pytest.mark.parametrize("passes", PASSES)
def test_restatement_fd_and_complex_step_jacobians_agree(passes):
    case = solid_case("bump", "strain")
    g = S.Geom(case.mesh)
    D = case.states
    rng = np.random.default_rng(3)
    V = rng.standard_normal((D.size, 6)) * np.abs(D).max()
    for k in range(V.shape[1]):
        cs = np.imag(S.residual(case, g, D + 1e-30j * V[:, k], passes)) / 1e-30
        h = 1e-3
        fd = (S.residual(case, g, D + h * V[:, k], passes) - S.residual(case, g, D - h * V[:, k], passes)) / (2 * h)
        assert rel(fd, cs) <= 1e-6  # the residual is affine in D: the difference quotient carries rounding alone


def test_restatement_normalisation_is_the_cell_volume():
    case = solid_case("mixed", "strain")
    g = S.Geom(case.mesh)
    Rn, Ru = S.residual(case, g, case.states), S.residual(case, g, case.states, normalized=False)
    assert np.array_equal(Ru.reshape(-1, 3), Rn.reshape(-1, 3) * g.V[:, None])


def test_restatement_traction_balance_improves_with_the_pass_count():
    """uniaxial tension of an orthogonal bar with the consistent traction on the outlet: D = (eps x, -nu' eps y, -nu' eps z) of plane
    strain-free 3-D elasticity; the traction-balance error of the lagged boundary gradient falls with the pass count."""
    rho, E, nu = 7854.0, 2e11, 0.3
    sig = 1e6
    L = (1.0, 0.2, 0.1)
    case = solid_displacement_case(6, 4, 3, lengths=L, mapping=None, rho=rho, E=E, nu=nu,
                                   D_bcs={"inlet": ("fixedValue", (0.0, 0.0, 0.0)), "outlet": ("tractionDisplacement", (sig, 0.0, 0.0), 0.0)})
    g = S.Geom(case.mesh)
    eps = sig / E
    D = np.stack([eps * g.C[:, 0], -nu * eps * (g.C[:, 1] - 0.5 * L[1]), -nu * eps * (g.C[:, 2] - 0.5 * L[2])], axis=1).ravel()
    errs = [S.traction_balance(case, g, D, p) for p in (2, 20, 60)]
    print("uniaxial: traction-balance error after 2, 20, 60 passes:", errs)
    # the exact field is linear and shear-free: the normal part of the gradient is exact after one pass with the exact tangential gradD,
    # so the balance holds to rounding at every one of these counts (1e-12 of the traction, with a margin of 1e3 for the gradient sums)
    # and never grows; the rate is measured on a state that contracts, below
    assert all(e <= 1e-9 * sig for e in errs) and errs[0] >= errs[1] >= errs[2]


def test_restatement_traction_passes_contract_on_a_sheared_state():
    """The bump-channel test state (sheared, two traction patches, edge cells with two traction faces): the traction-balance error falls
    strictly over 2, 20 and 60 passes.  The rate per pass: below 1 (a contraction); the hand estimate for the tangential part on an
    orthogonal face is (mu + lambda) / (2 mu + lambda) = 0.71 at nu = 0.3, and nothing in the lagged update can be faster than its
    slowest component, so the band is 0.71 (less 5 % for the pre-asymptotic start) to 0.95."""
    case = solid_case("bump", "strain")
    g = S.Geom(case.mesh)
    errs = [S.traction_balance(case, g, case.states, p) for p in (2, 20, 60)]
    r1, r2 = (errs[1] / errs[0]) ** (1 / 18.0), (errs[2] / errs[1]) ** (1 / 40.0)
    print("bump: traction-balance error after 2, 20, 60 passes:", errs, "rate per pass:", r1, r2)
    assert errs[0] > errs[1] > errs[2]
    assert 0.67 <= r1 <= 0.95 and 0.67 <= r2 <= 0.95


# ---- the kernel bodies on the host -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("material", sorted(MATERIALS))
@pytest.mark.parametrize("mesh", MESHES)
def test_hostemu_values_and_tangents(emu, mesh, material, passes):
    case = solid_case(mesh, material)
    g = S.Geom(case.mesh)
    D = case.states
    Ro = S.residual(case, g, D, passes)
    rng = np.random.default_rng(11)
    v = rng.standard_normal(D.size) * np.abs(D).max()
    Jv = np.imag(S.residual(case, g, D + 1e-30j * v, passes)) / 1e-30
    res = {}
    for isPC in (0, 1):
        R, Rd = emu_residual(emu, case, D, passes, isPC, 1, v)
        res[isPC] = (R, Rd)
        print(mesh, material, passes, "isPC", isPC, "value", rel(R, Ro), "tangent", rel(Rd, Jv))
        assert rel(R, Ro) <= 1e-12 and rel(Rd, Jv) <= 1e-10
        assert np.array_equal(R, emu_residual(emu, case, D, passes, isPC, 1))  # the double and the dual pass give the same values
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])  # no PC variant of this residual


def test_hostemu_unnormalised_and_von_mises(emu):
    case = solid_case("mixed", "strain")
    g = S.Geom(case.mesh)
    D = case.states
    vm = np.zeros(g.nC)
    Ru = emu_residual(emu, case, D, 2, 0, 0, vm=vm)
    assert rel(Ru, S.residual(case, g, D, 2, normalized=False)) <= 1e-12
    assert rel(vm, S.von_mises(case, g, D, 2)) <= 1e-12


def _points_of_interest(case, g):
    """an interior, a wall, an edge and an apex (corner) point: by the number of boundary faces that use the point"""
    m = case.mesh
    cnt = np.zeros(m.n_points, int)
    fp = m.face_ptr
    for f in range(g.nIF, g.nF):
        cnt[m.face_pts[fp[f]:fp[f + 1]]] += 1
    npatch = np.zeros(m.n_points, int)
    for p in m.patches:
        seen = np.zeros(m.n_points, bool)
        for f in range(p.start, p.start + p.size):
            seen[m.face_pts[fp[f]:fp[f + 1]]] = True
        npatch += seen
    return [int(np.nonzero(npatch == k)[0][len(np.nonzero(npatch == k)[0]) // 2]) for k in (0, 1, 2, 3)]


@pytest.mark.parametrize("mesh", ("bump", "mixed"))
def test_hostemu_dual_metrics_against_the_complex_step(emu, mesh):
    case = solid_case(mesh, "strain")
    g = S.Geom(case.mesh)
    D = case.states
    scale = np.abs(S.residual(case, g, D, 2)).max()
    for pt in _points_of_interest(case, g):
        for k in range(3):
            dX = np.zeros(case.mesh.points.shape)
            dX[pt, k] = 1.0
            cs = np.imag(S.residual(case, S.Geom(case.mesh, case.mesh.points + 1e-30j * dX), D, 2)) / 1e-30
            Rd = np.zeros(D.size)
            assert emu.emu_solid_geom(CaseStruct(case).byref(), dptr(np.ascontiguousarray(D)), D.size, 2, dptr(np.ascontiguousarray(dX.ravel())), dptr(Rd)) == 0
            err = np.abs(Rd - cs).max() / max(np.abs(cs).max(), scale)
            print(mesh, "point", pt, "direction", k, err)
            assert err <= 1e-10


# ---- errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,value,word", [("rho", 0.0, "rho"), ("rho", -1.0, "rho"), ("E", 0.0, "E"), ("nu", 0.5, "nu"), ("nu", -1.0, "nu")])
def test_bad_material_is_refused_by_name(key, value, word):
    case = copy.copy(solid_case("bump", "strain"))
    case.mechanical = dict(case.mechanical, **{key: value})
    with pytest.raises(_capi.DASError, match=word) as e:
        CaseStruct(case)
    assert str(value) in str(e.value)
    # the C entry: the same refusal with the value in the message
    good = CaseStruct(solid_case("bump", "strain"))
    setattr(good.struct, {"rho": "solid_rho", "E": "solid_E", "nu": "solid_nu"}[key], value)
    L = _capi.lib()
    assert not L.das_create(good.byref())
    msg = L.das_last_error().decode()
    assert word in msg and "not %f" % value in msg  # std::to_string prints %f


def test_field_type_material_is_refused_by_name():
    case = copy.copy(solid_case("bump", "strain"))
    case.mechanical = dict(case.mechanical, E={"type": "field"})
    with pytest.raises(_capi.DASError, match="field"):
        CaseStruct(case)


def test_sharded_solver_is_refused():
    from dafoam_amd.distributed import extract_submesh
    with pytest.raises(NotImplementedError, match="DASolidDisplacementFoam"):
        extract_submesh(solid_case("bump", "strain"), np.zeros(120, int), 0)


def test_uniform_material_without_a_value_is_refused_by_name():
    case = copy.copy(solid_case("bump", "strain"))
    case.mechanical = dict(case.mechanical, nu={"type": "uniform"})
    with pytest.raises(_capi.DASError, match="mechanicalProperties nu"):
        CaseStruct(case)


def make(case, **opts):
    return pyDASolvers(b"DASolidDisplacementFoam -python", solid_options(2, **opts), case=case)


def test_bad_patch_fields_are_refused_by_name():
    L = _capi.lib()
    # a D patch code that is none of the four
    case = copy.copy(solid_case("bump", "strain"))
    case.bcs = dict(case.bcs, bottom={"D": (2, 0.0)})
    with pytest.raises(_capi.DASError, match="fixedValue, zeroGradient, symmetry or tractionDisplacement"):
        CaseStruct(case)
    cs = CaseStruct(solid_case("bump", "strain"))
    cs.keep["bc_D_code"][2] = 2
    assert not L.das_create(cs.byref())
    assert "fixedValue, zeroGradient, symmetry or tractionDisplacement" in L.das_last_error().decode()
    # a cyclic patch on this solver
    case = copy.copy(solid_case("bump", "strain"))
    case.mesh = copy.copy(case.mesh)
    case.mesh.patches = [Patch(p.name, "cyclic" if p.name in ("front", "back") else p.type, p.start, p.size,
                               {"front": "back", "back": "front"}.get(p.name), None) for p in case.mesh.patches]
    with pytest.raises(_capi.DASError, match="cyclic"):
        CaseStruct(case)
    cs = CaseStruct(solid_case("bump", "strain"))
    cs.keep["patch_type"][4] = 3
    assert not L.das_create(cs.byref())
    assert "cyclic" in L.das_last_error().decode() and "DASolidDisplacementFoam" in L.das_last_error().decode()
    # the traction code on a field of another solver
    from dafoam_amd.meshgen import heat_transfer_case
    cs = CaseStruct(heat_transfer_case(3, 3, 3, kappa=1.0))
    cs.keep["bc_T_code"][1] = BC_TRACTION
    assert not L.das_create(cs.byref())
    assert "tractionDisplacement" in L.das_last_error().decode()


@pytest.mark.parametrize("ftype,extra", [("force", {"patches": ["top"], "directionMode": "fixedDirection", "direction": [1.0, 0.0, 0.0]}),
                                         ("wallHeatFlux", {"patches": ["top"]}), ("massFlowRate", {"patches": ["outlet"]}),
                                         ("location", {"patches": ["top"], "mode": "maxRadius"}),
                                         ("patchMean", {"patches": ["top"], "varName": "D", "varType": "vector", "index": 0}),
                                         ("variance", {"mode": "field", "varName": "D", "varType": "vector", "indices": [0]})])
def test_other_function_types_are_refused_by_name(ftype, extra):
    with pytest.raises(_capi.DASError, match="DASolidDisplacementFoam"):
        make(solid_case("bump", "strain"), function={"F": dict({"type": ftype, "source": "patchToFace", "scale": 1.0}, **extra)})


def test_variable_vol_sum_of_an_unknown_variable_and_the_c_entries_refuse_by_name():
    case = solid_case("bump", "strain")
    with pytest.raises(_capi.DASError, match="DASolidDisplacementFoam"):
        make(case, function={"F": {"type": "variableVolSum", "source": "allCells", "varName": "T", "varType": "scalar", "scale": 1.0}})
    s = make(case)
    L = _capi.lib()
    ids = np.array([3], dtype=np.int32)
    d = np.array([1.0, 0.0, 0.0])
    assert L.das_define_face_function(s._h, b"F", b"force", ids.ctypes.data_as(_capi.c_int_p), None, 1, dptr(d), None, 1.0, 0.0) != 0
    assert "DASolidDisplacementFoam" in L.das_last_error().decode()
    assert L.das_define_force_coupling(s._h, b"q", ids.ctypes.data_as(_capi.c_int_p), 1, 0.0) != 0
    assert L.das_define_thermal_coupling(s._h, b"q", ids.ctypes.data_as(_capi.c_int_p), 1, 0) != 0
    cells = np.arange(4, dtype=np.int32)
    comps = np.array([0], dtype=np.int32)
    assert L.das_define_cell_function(s._h, b"F", b"variance", cells.ctypes.data_as(_capi.c_int_p), 4, b"D", comps.ctypes.data_as(_capi.c_int_p), 1, None, 0, 1.0, 0.0) != 0
    assert "DASolidDisplacementFoam" in L.das_last_error().decode()
    assert L.das_define_cell_function(s._h, b"F", b"variableVolSum", cells.ctypes.data_as(_capi.c_int_p), 4, b"p", comps.ctypes.data_as(_capi.c_int_p), 1, None, 0, 1.0, 0.0) != 0
    assert "DASolidDisplacementFoam" in L.das_last_error().decode()
    # vonMisesStressKS on another solver
    from dafoam_amd.meshgen import heat_transfer_case
    from heat_transfer_cases import heat_options
    hc = heat_transfer_case(3, 3, 3, kappa=1.0)
    with pytest.raises(_capi.DASError, match="vonMisesStressKS"):
        pyDASolvers(b"DAHeatTransferFoam -python", heat_options(hc, function={"F": {"type": "vonMisesStressKS", "source": "allCells", "scale": 1.0, "coeffKS": 1.0}}), case=hc)


def test_couplings_and_fv_source_are_refused_by_name():
    case = solid_case("bump", "strain")
    with pytest.raises(_capi.DASError, match="DASolidDisplacementFoam"):
        make(case, outputInfo={"q": {"type": "thermalCouplingOutput", "patches": ["top"], "components": ["thermalCoupling"]}})
    with pytest.raises(_capi.DASError, match="DASolidDisplacementFoam"):
        make(case, outputInfo={"q": {"type": "forceCouplingOutput", "patches": ["top"], "components": ["forceCoupling"], "pRef": 0.0}})
    with pytest.raises((_capi.DASError, NotImplementedError), match="DASolidDisplacementFoam"):
        make(case, inputInfo={"tin": {"type": "thermalCoupling", "patches": ["top"], "components": ["thermalCoupling"]}})
    with pytest.raises(_capi.DASError, match="DASolidDisplacementFoam"):
        make(case, fvSource={"s": {"type": "heatSource"}})
    with pytest.raises(_capi.DASError, match="DASolidDisplacementFoam"):
        make(case).simpleIteration()


# ---- the KS objective: its inputs and its summand ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("material", sorted(MATERIALS))
@pytest.mark.parametrize("mesh", MESHES)
def test_ks_loads_are_neither_the_maximum_nor_a_mean_and_the_summand_matches(emu, mesh, material, passes):
    case = solid_case(mesh, material)
    g = S.Geom(case.mesh)
    a = S.ks_summands(case, g, case.states, passes, KS_SCALE, KS_COEFF)
    print(mesh, material, passes, "coeffKS max(vm):", a.max())
    assert 5.0 <= a.max() <= 50.0  # a condition on the inputs (the issue's range), on the restatement's numbers
    box = S.box_cells(g, *KS_BOX)
    assert 0 < box.size < g.nC
    vm = np.zeros(g.nC)
    emu_residual(emu, case, case.states, passes, vm=vm, vm_scale=KS_SCALE)
    assert rel(KS_COEFF * vm, a) <= 1e-12
    # exp(coeffKS vm - max): the summand of the shifted sum
    assert rel(np.exp(KS_COEFF * vm - (KS_COEFF * vm).max()), np.exp(a - a.max())) <= 1e-10


# ---- the graph ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_connectivity_is_the_distance_two_pattern_times_3x3_and_the_colouring_is_valid(mesh):
    import scipy.sparse as sp

    case = solid_case(mesh, "strain")
    m = case.mesh
    s = make(case)
    N, nIF = m.n_cells, m.n_internal_faces
    assert s.getNLocalAdjointStates() == 3 * N == case.states.size
    s.runColoring()
    A = sp.coo_matrix((np.ones(nIF), (m.owner[:nIF], m.neighbour)), shape=(N, N)).tocsr()
    A = ((A + A.T + sp.identity(N)) > 0).astype(np.int32)
    cells = ((A @ A) > 0).astype(np.int8)  # DRes <- D at levels 0, 1, 2 (DAStateInfoSolidDisplacementFoam.C:69-75)
    want = sp.kron(cells, np.ones((3, 3), np.int8)).tocsr()  # states interleaved per cell
    for pc in (0, 1):
        assert (s.getConnectivity(pc) != want).nnz == 0
    col, nc = s.getColoring()
    assert nc == col.max() + 1
    for r in range(0, 3 * N, 3):  # no row reads two states of one colour (the three rows of a cell share their columns)
        cols = want.indices[want.indptr[r] : want.indptr[r + 1]]
        assert np.unique(col[cols]).size == cols.size

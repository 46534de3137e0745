"""CPU tier of DAHeatTransferFoam, the solid side of conjugate heat transfer: the numpy restatement (tests/heat_transfer_restatement.py)
checked on its own, the kernel bodies body_heat_grad / body_heat / body_facefn_solid / body_thermal_coupling_solid run on the host
(tests/hostemu/hostemu_heat.cpp) against it, connectivity and colouring of the C++ host code, the host-side errors, and the exchange loop
of a composite wall in numpy."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import heat_transfer_restatement as H
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import BC_FIXED_VALUE, BC_ZERO_GRADIENT, heat_transfer_case, with_mixed_T
from dafoam_amd.pyDASolvers import pyDASolvers
from heat_transfer_cases import MATERIALS, MESHES, heat_case, heat_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp, ip = _capi.c_double_p, _capi.c_int_p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_heat.cpp through g++, as tests/test_thermal_coupling_cpu.py builds its harness."""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    so = str(tmp_path_factory.mktemp("hostemu") / "libhostemu_heat.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-o", so, os.path.join(ROOT, "tests", "hostemu", "hostemu_heat.cpp"), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L = C.CDLL(so)
    L.emu_heat_residual.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, C.c_int, C.c_int, dp, dp, dp]
    L.emu_heat_geom.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, dp, dp]
    L.emu_heat_faces.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, ip, C.c_int, C.c_int, dp, dp]
    L.emu_heat_kappa.argtypes = [C.POINTER(das_case_t), C.c_int, dp, dp]
    return L


def emu_residual(L, case, T, isPC=0, normalized=1, direction=None):
    cs = CaseStruct(case)
    T = np.ascontiguousarray(T, dtype=np.float64)
    R, Rd = np.zeros(T.size), np.zeros(T.size)
    d = None if direction is None else np.ascontiguousarray(direction, dtype=np.float64)
    assert L.emu_heat_residual(cs.byref(), dptr(T), T.size, isPC, normalized, dptr(d) if d is not None else None, dptr(R), dptr(Rd)) == 0
    return (R, Rd) if direction is not None else R


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


# ---- 1-3: the restatement on its own -----------------------------------------------------------------------------------------------
def test_restatement_linear_profile_is_a_zero_on_an_orthogonal_box():
    L, dT, kappa = 0.7, 100.0, 200.0
    case = heat_transfer_case(7, 4, 3, lengths=(L, 0.3, 0.2), kappa=kappa, mapping=None,
                              T_bcs={"inlet": ("fixedValue", 400.0), "outlet": ("fixedValue", 400.0 - dT)})
    g = H.Geom(case.mesh)
    R = H.residual(case, g, 400.0 - dT * g.C[:, 0] / L)
    print("max |TRes| / (kappa dT / L^2):", np.abs(R).max() / (kappa * dT / L**2))
    assert np.abs(R).max() <= 1e-12 * kappa * dT / L**2


@pytest.mark.parametrize("material", sorted(MATERIALS))
def test_restatement_fd_and_complex_step_jacobians_agree(material):
    case = heat_case("bump", material)
    g = H.Geom(case.mesh)
    Jcs = H.jacobian_cs(lambda x: H.residual(case, g, x), case.states)
    Jfd = H.jacobian_fd(lambda x: H.residual(case, g, x), case.states)
    print("FD against complex step:", rel(Jfd, Jcs))
    assert rel(Jfd, Jcs) <= 1e-6


def test_restatement_normalisation_is_the_cell_volume():
    case = heat_case("mixed", "poly")
    g = H.Geom(case.mesh)
    Rn, Ru = H.residual(case, g, case.states), H.residual(case, g, case.states, normalized=False)
    assert np.array_equal(Ru, Rn * g.V)


# ---- 4: the kernel bodies on the host ----------------------------------------------------------------------------------------------
def test_kappa_horner_against_the_power_sum(emu):
    case = heat_case("bump", "poly")
    T = np.linspace(250.0, 450.0, 41)
    out = np.zeros(T.size)
    assert emu.emu_heat_kappa(CaseStruct(case).byref(), T.size, dptr(T), dptr(out)) == 0
    assert rel(out, H.kappa_of(case.kappa_coeffs, T)) <= 1e-14
    # the polynomial is live over the field of the test state: kappa(300) = 44, kappa(400) = 56 with the coefficients (20, 0.05, 1e-4)
    k = H.kappa_of(case.kappa_coeffs, case.states)
    assert k.max() / k.min() > 1.15


@pytest.mark.parametrize("material", sorted(MATERIALS))
@pytest.mark.parametrize("mesh", MESHES)
def test_hostemu_values_and_tangents(emu, mesh, material):
    case = heat_case(mesh, material)
    g = H.Geom(case.mesh)
    T = case.states
    Ro = H.residual(case, g, T)
    rng = np.random.default_rng(11)
    v = rng.standard_normal(T.size) * 10.0
    Jv = np.imag(H.residual(case, g, T + 1e-30j * v)) / 1e-30
    res = {}
    for isPC in (0, 1):
        R, Rd = emu_residual(emu, case, T, isPC, 1, v)
        res[isPC] = (R, Rd)
        print(mesh, material, "isPC", isPC, "value", rel(R, Ro), "tangent", rel(Rd, Jv))
        assert rel(R, Ro) <= 1e-12 and rel(Rd, Jv) <= 1e-10
        assert np.array_equal(R, emu_residual(emu, case, T, isPC, 1))  # the double and the dual pass give the same values
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])  # no PC variant of this residual
    Ru = emu_residual(emu, case, T, 0, 0)
    assert rel(Ru, H.residual(case, g, T, normalized=False)) <= 1e-12


def test_hostemu_mixed_at_fraction_0_and_1_is_zero_gradient_and_fixed_value(emu):
    base = heat_case("bump", "poly")
    n = {p.name: p.size for p in base.mesh.patches}["bottom"]
    plain = copy.copy(base)
    plain.bcs = copy.deepcopy(base.bcs)
    plain.mixed_T = {}
    for f, code, val in ((0.0, BC_ZERO_GRADIENT, 0.0), (1.0, BC_FIXED_VALUE, 305.0)):
        plain.bcs["bottom"]["T"] = (code, val)
        mixed = with_mixed_T(plain, "bottom", np.full(n, 305.0), np.full(n, f))
        assert np.array_equal(emu_residual(emu, mixed, base.states), emu_residual(emu, plain, base.states))


@pytest.mark.parametrize("material", sorted(MATERIALS))
def test_hostemu_dual_metrics_against_the_complex_step_in_the_points(emu, material):
    case = heat_case("mixed", material)
    m = case.mesh
    nx, ny, nz = 6, 5, 4
    bottom = {p.name: p for p in m.patches}["bottom"]
    wall_point = int(m.face_pts[m.face_ptr[bottom.start + 7]])
    points = {"interior": 3 + (nx + 1) * (2 + (ny + 1) * 2), "wall": wall_point, "apex": (nx + 1) * (ny + 1) * (nz + 1)}
    assert points["apex"] < m.n_points  # the first point mixed_cell_case added: the apex of a hex cut into pyramids
    cs = CaseStruct(case)
    T = np.ascontiguousarray(case.states)
    for name, p in points.items():
        dX = np.zeros((m.n_points, 3))
        dX[p] = (0.3, -0.5, 0.8)
        Rd = np.zeros(T.size)
        assert emu.emu_heat_geom(cs.byref(), dptr(T), T.size, dptr(np.ascontiguousarray(dX.ravel())), dptr(Rd)) == 0
        ref = np.imag(H.residual(case, H.Geom(m, m.points + 1e-30j * dX), T)) / 1e-30
        print(material, name, "point", p, rel(Rd, ref))
        assert np.abs(ref).max() > 0 and rel(Rd, ref) <= 1e-10


@pytest.mark.parametrize("material", sorted(MATERIALS))
@pytest.mark.parametrize("mesh", ("bump", "mixed_renumbered"))
def test_hostemu_wall_heat_flux_and_coupling_terms(emu, mesh, material):
    case = heat_case(mesh, material)
    g = H.Geom(case.mesh)
    T = np.ascontiguousarray(case.states)
    faces = np.ascontiguousarray(H.selected_faces(case, ["bottom", "inlet", "top"]), dtype=np.int32)
    nf = faces.size
    Tb, sn = H.patch_fields(case, g, T)
    for custom, mode in ((0, "default"), (1, "daCustom")):
        out, whf = np.zeros(2 * nf), np.zeros(nf)
        assert emu.emu_heat_faces(CaseStruct(case).byref(), dptr(T), T.size, faces.ctypes.data_as(ip), nf, custom, dptr(out), dptr(whf)) == 0
        assert rel(out, H.coupling_output(case, g, T, ["top", "inlet", "bottom"], mode)) <= 1e-12
        s = sn if not custom else (Tb - T[g.bcell]) / g.bDist
        assert rel(whf, (H.kappa_of(case.kappa_coeffs, Tb) * s)[faces - g.nIF]) <= 1e-12


# ---- 5: connectivity and colouring from the C++ host code --------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_connectivity_is_the_distance_two_pattern_and_the_colouring_is_valid(mesh):
    import scipy.sparse as sp

    case = heat_case(mesh, "const")
    m = case.mesh
    s = pyDASolvers(b"DAHeatTransferFoam -python", heat_options(case), case=case)
    assert s.getNLocalAdjointStates() == m.n_cells == case.states.size
    s.runColoring()
    N, nIF = m.n_cells, m.n_internal_faces
    A = sp.coo_matrix((np.ones(nIF), (m.owner[:nIF], m.neighbour)), shape=(N, N)).tocsr()
    A = ((A + A.T + sp.identity(N)) > 0).astype(np.int32)
    want = ((A @ A) > 0).astype(np.int8).tocsr()  # TRes <- T at levels 0, 1, 2 (DAStateInfoHeatTransferFoam.C:69-75)
    for pc in (0, 1):
        assert (s.getConnectivity(pc) != want).nnz == 0
    col, nc = s.getColoring()
    assert nc == col.max() + 1
    for r in range(N):  # no row reads two states of one colour
        cols = want.indices[want.indptr[r] : want.indptr[r + 1]]
        assert np.unique(col[cols]).size == cols.size


# ---- 6: host-side errors, each by name ----------------------------------------------------------------------------------------------
def make(case, **opts):
    return pyDASolvers(b"DAHeatTransferFoam -python", heat_options(case, **opts), case=case)


def test_error_kappa_coefficients():
    with pytest.raises(_capi.DASError, match="kappa or kappaCoeffs"):
        make(heat_transfer_case(3, 3, 3, kappa_coeffs=tuple(range(1, 10))))
    with pytest.raises(_capi.DASError, match="kappa or kappaCoeffs"):
        make(heat_transfer_case(3, 3, 3, kappa_coeffs=()))
    # the C entry itself refuses them as well
    cs = CaseStruct(heat_transfer_case(3, 3, 3, kappa=1.0))
    for n in (0, 9):
        cs.struct.n_kappa_coeffs = n
        assert not _capi.lib().das_create(cs.byref())
        msg = _capi.lib().das_last_error().decode()
        assert "kappa" in msg and "kappaCoeffs" in msg, msg


def test_error_fvsource():
    with pytest.raises(_capi.DASError, match="fvSource"):
        make(heat_case("bump", "const"), fvSource={"heat": {"type": "heatSource"}})
    make(heat_case("bump", "const"), fvSource={})  # an empty one is what the defaults carry


def test_error_coupling_needs_discipline_thermal():
    case = heat_case("bump", "const")
    out = {"out": {"type": "thermalCouplingOutput", "patches": ["bottom"], "components": ["thermalCoupling"]}}
    inp = {"in": {"type": "thermalCoupling", "patches": ["bottom"], "components": ["thermalCoupling"]}}
    for kw in (dict(outputInfo=out), dict(inputInfo=inp)):
        with pytest.raises(_capi.DASError, match="needs discipline thermal"):
            make(case, discipline="aero", **kw)
        with pytest.raises(_capi.DASError, match="needs discipline thermal"):
            make(case, **kw)  # aero is the default
        make(case, discipline="thermal", **kw)
    s = make(case, discipline="thermal", outputInfo=out, inputInfo=inp)
    n = {p.name: p.size for p in case.mesh.patches}["bottom"]
    assert s.getOutputSize("out", "thermalCouplingOutput") == 2 * n == s.getInputSize("in", "thermalCoupling")


def test_error_force_coupling_output():
    with pytest.raises(_capi.DASError, match="forceCouplingOutput needs a flow solver"):
        make(heat_case("bump", "const"), discipline="thermal",
             outputInfo={"f": {"type": "forceCouplingOutput", "patches": ["bottom"], "components": ["forceCoupling"], "pRef": 0.0}})


@pytest.mark.parametrize("ftype", ["force", "massFlowRate", "totalPressure", "patchMean", "variance", "location"])
def test_error_other_function_types(ftype):
    with pytest.raises(_capi.DASError, match=f"type {ftype} is not built for DAHeatTransferFoam"):
        make(heat_case("bump", "const"), function={"f": {"type": ftype, "source": "patchToFace", "patches": ["bottom"], "direction": [1.0, 0.0, 0.0], "scale": 1.0}})


def test_error_function_variable_and_c_entry():
    case = heat_case("bump", "const")
    with pytest.raises(_capi.DASError, match="varName p is not supported by this solver; supported: T"):
        make(case, function={"f": {"type": "variableVolSum", "source": "allCells", "varName": "p", "varType": "scalar", "scale": 1.0}})
    s = make(case, function={"q": {"type": "wallHeatFlux", "source": "patchToFace", "patches": ["bottom"], "scale": 1.0},
                             "v": {"type": "variableVolSum", "source": "allCells", "varName": "T", "varType": "scalar", "scale": 1.0}})
    ids = np.array([2], dtype=np.int32)
    rc = _capi.lib().das_define_face_function(s._h, b"m", b"massFlowRate", ids.ctypes.data_as(ip), None, 1, None, None, 1.0, 0.0)
    assert rc < 0 and "massFlowRate" in _capi.lib().das_last_error().decode()


def test_error_no_dirichlet_or_mixed_patch():
    case = heat_transfer_case(3, 3, 3, kappa=1.0, T_bcs={})
    with pytest.raises(_capi.DASError, match="no patch carries a fixedValue or mixed T"):
        make(case).solvePrimal()


def test_error_thermal_coupling_input_on_a_patch_that_is_not_mixed():
    with pytest.raises(_capi.DASError, match="patch top does not carry a mixed T patch field"):
        make(heat_case("bump", "const"), discipline="thermal", inputInfo={"in": {"type": "thermalCoupling", "patches": ["top"], "components": ["thermalCoupling"]}})


# ---- 7: the exchange loop of a composite wall, in numpy -----------------------------------------------------------------------------
def composite_wall():
    """A 3 x 3 x 3 slab (kappa 200, thickness 0.1, hot wall 400 at its inlet) against a 5 x 3 x 3 slab (kappa 1, thickness 0.05, cold wall 300 at
    its outlet); they meet at the first one's outlet and the second one's inlet, both mixed."""
    L1, L2, k1, k2 = 0.1, 0.05, 200.0, 1.0
    a = heat_transfer_case(3, 3, 3, lengths=(L1, 0.3, 0.3), kappa=k1, mapping=None, T_bcs={"inlet": ("fixedValue", 400.0)}, mixed_patches={"outlet": (350.0, 0.5)})
    b = heat_transfer_case(5, 3, 3, lengths=(L2, 0.3, 0.3), kappa=k2, mapping=None, T_bcs={"outlet": ("fixedValue", 300.0)}, mixed_patches={"inlet": (350.0, 0.5)})
    q = 100.0 / (L1 / k1 + L2 / k2)
    return a, b, q, 400.0 - q * L1 / k1


def test_exchange_loop_meets_the_composite_wall_answer():
    a, b, q, Ti = composite_wall()
    ga, gb = H.Geom(a.mesh), H.Geom(b.mesh)
    Ta, Tb = a.states.copy(), b.states.copy()
    rec_a, rec_b = dict(a.mixed_T), dict(b.mixed_T)
    mode = "daCustom"
    last, n_exchanges = None, 0
    for n_exchanges in range(1, 21):
        out_a = H.coupling_output(a, ga, Ta, ["outlet"], mode, mixed=rec_a)
        rec_b = H.coupling_records(b, gb, Tb, ["inlet"], out_a, mode)
        Tb, _ = H.newton(b, gb, Tb, mixed=rec_b)
        out_b = H.coupling_output(b, gb, Tb, ["inlet"], mode, mixed=rec_b)
        rec_a = H.coupling_records(a, ga, Ta, ["outlet"], out_b, mode)
        Ta, _ = H.newton(a, ga, Ta, mixed=rec_a)
        now = np.concatenate([out_a[: out_a.size // 2], out_b[: out_b.size // 2]])
        if last is not None and np.abs(now - last).max() < 1e-10:
            break
        last = now
    else:
        pytest.fail("the exchange loop did not settle to 1e-10 K in 20 exchanges")
    Ti_a = H.patch_fields(a, ga, Ta, mixed=rec_a)[0][ga.patch_slices()["outlet"]]
    Ti_b = H.patch_fields(b, gb, Tb, mixed=rec_b)[0][gb.patch_slices()["inlet"]]
    qa = H.wall_heat_flux(a, ga, Ta, ["outlet"], mode, True, mixed=rec_a)
    qb = H.wall_heat_flux(b, gb, Tb, ["inlet"], mode, True, mixed=rec_b)
    print("exchanges", n_exchanges, "T_i", Ti_a.mean(), Ti_b.mean(), "analytic", Ti, "q", qa, qb, "analytic", q)
    assert n_exchanges <= 20
    assert np.abs(Ti_a - Ti).max() <= 1e-9 * Ti and np.abs(Ti_b - Ti).max() <= 1e-9 * Ti
    assert abs(-qa - q) <= 1e-9 * q and abs(qb - q) <= 1e-9 * q


def test_error_sharded_solver():
    from dafoam_amd.distributed import extract_submesh

    case = heat_case("bump", "const")
    with pytest.raises(NotImplementedError, match="sharded .multi-rank. DAHeatTransferFoam solvers are not built"):
        extract_submesh(case, np.arange(case.mesh.n_cells) % 2, 0)

"""CPU tier of the heat sources of DAHeatTransferFoam (the fvSource option, type heatSource, and the fvSourcePar input): the numpy
restatement (tests/heat_source_restatement.py) on its own, the kernel body body_heat_source and body_heat with the src pointer run on the
host (tests/hostemu/hostemu_heat_source.cpp) against it, the membership rule of cylinderToCell, and the host-side errors by name.
Bounds (tests/README_heat_transfer.md): values 1e-12, tangents 1e-10 against the complex step of the restatement, fields relative to their
maximum; "bitwise" is np.array_equal."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import heat_source_restatement as HS
import heat_transfer_restatement as H
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import channel_case
from dafoam_amd.pyDASolvers import pyDASolvers
from heat_source_cases import ALL_SOURCES, B_CELLS, SOURCE_A, SOURCE_B, geom, source_case, sources
from heat_transfer_cases import MESHES, heat_case, heat_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = _capi.c_double_p
ALL_MESHES = MESHES + ("box",)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_heat_source.cpp through g++, as tests/test_heat_transfer_cpu.py builds its harness."""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    so = str(tmp_path_factory.mktemp("hostemu") / "libhostemu_heat_source.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-o", so, os.path.join(ROOT, "tests", "hostemu", "hostemu_heat_source.cpp"), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L = C.CDLL(so)
    L.emu_hs_shape.argtypes = [C.POINTER(das_case_t), dp, C.c_double, C.c_int, dp, dp, dp, dp]
    L.emu_hs_residual.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, C.c_int, dp, dp]
    # the harness of the residual without the term (tests/hostemu/hostemu_heat.cpp), for the bitwise comparison
    so0 = so.replace("heat_source", "heat")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-o", so0, os.path.join(ROOT, "tests", "hostemu", "hostemu_heat.cpp"), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L.plain = C.CDLL(so0)
    L.plain.emu_heat_residual.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, C.c_int, C.c_int, dp, dp, dp]
    return L


def emu_shape(L, case, pars, eps, cell=None, dpar=None, dX=None):
    n = case.mesh.n_cells
    sv, sd = np.zeros(n), np.zeros(n)
    arr = lambda a: None if a is None else dptr(np.ascontiguousarray(a, dtype=np.float64).ravel())
    assert L.emu_hs_shape(CaseStruct(case).byref(), arr(np.real(pars)), eps, -1 if cell is None else cell, arr(dpar), arr(dX), dptr(sv), dptr(sd)) == 0
    return sv, sd


# ---- the restatement on its own ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ALL_MESHES)
def test_restatement_integrates_to_the_powers_and_every_branch_is_live(mesh):
    g, S = geom(mesh), sources(mesh)
    q = S.field(g)
    total = float(np.real(q * g.V).sum())
    print(mesh, "sum q V", total, "powers", S.total_power())
    assert abs(total - S.total_power()) <= 1e-13 * S.total_power()
    e = S.entries["mid_A"]
    s = HS.smooth_shape(g, e["pars"].real, e["eps"])
    c = g.C - e["pars"][:3].real
    n = e["pars"][3:6].real / np.linalg.norm(e["pars"][3:6].real)
    A, R = np.linalg.norm(c * n, axis=1), np.linalg.norm(c - c * n, axis=1)
    assert (s == 1).any() and (A > 0.15).any() and (R > 0.04).any() and ((A > 0.15) & (R > 0.04)).any()
    # the projection reading n (c . n) is another field altogether: no 1e-12 test can pass with it
    sp = HS.smooth_shape(g, e["pars"].real, e["eps"], projection=True)
    assert np.abs(s - sp).max() > 0.8 * s.max()
    assert S.entries["tail_B"]["cells"].size == B_CELLS[mesh]


def test_restatement_complex_step_against_central_differences():
    g = geom("bump")
    S = sources("bump", ("mid_A",))
    p0 = S.entries["mid_A"]["pars"].real
    for i in range(9):
        dcs = np.imag(S.field(g, {"mid_A": p0 + 1e-30j * np.eye(9)[i]})) / 1e-30
        h = 1e-6 * max(abs(p0[i]), 1e-2)
        dfd = (S.field(g, {"mid_A": p0 + h * np.eye(9)[i]}) - S.field(g, {"mid_A": p0 - h * np.eye(9)[i]})) / (2 * h)
        print(HS.PAR_NAMES[i], rel(dfd, dcs))
        assert np.abs(dcs).max() > 0 and rel(dfd, dcs) <= 1e-6


# ---- body_heat_source on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_hostemu_shape_values_and_parameter_tangents(emu, mesh):
    case, g = source_case(mesh), geom(mesh)
    pars, eps = sources(mesh).entries["mid_A"]["pars"], SOURCE_A["eps"]
    ref = HS.smooth_shape(g, pars.real, eps)
    sv, _ = emu_shape(emu, case, pars, eps)
    print(mesh, "values", rel(sv, ref))
    assert rel(sv, ref) <= 1e-12
    for i in range(8):  # the power is no parameter of the shape
        v, d = emu_shape(emu, case, pars, eps, dpar=np.eye(9)[i])
        dcs = np.imag(HS.smooth_shape(g, pars + 1e-30j * np.eye(9)[i], eps)) / 1e-30
        print(mesh, HS.PAR_NAMES[i], rel(d, dcs))
        assert np.array_equal(v, sv) and np.abs(dcs).max() > 0 and rel(d, dcs) <= 1e-10


@pytest.mark.parametrize("mesh", MESHES)
def test_hostemu_shape_dual_metrics_and_the_snapped_cell(emu, mesh):
    case, g = source_case(mesh), geom(mesh)
    m = case.mesh
    e = sources(mesh).entries["head_C"]
    cell, pars, eps = e["cell"], e["pars"], e["eps"]
    sv, _ = emu_shape(emu, case, pars, eps, cell=cell)
    assert rel(sv, HS.smooth_shape(g, pars.real, eps, center=g.C[cell])) <= 1e-12 and sv[cell] == 1.0
    # the parameters of a snapped source: a finite, zero tangent in the snapped cell itself (A = R = 0), in every pass
    for i in range(3, 8):
        _, d = emu_shape(emu, case, pars, eps, cell=cell, dpar=np.eye(9)[i])
        assert np.isfinite(d).all() and d[cell] == 0.0
    nx, ny, nz = 6, 5, 4
    bottom = {p.name: p for p in m.patches}["bottom"]
    # a wall point, a point of the snapped cell (the first point of a face it owns), an interior point and the apex of a pyramid
    points = {"wall": int(m.face_pts[m.face_ptr[bottom.start + 7]]), "snapped": int(m.face_pts[m.face_ptr[int(np.nonzero(m.owner == cell)[0][0])]])}
    if mesh in ("bump", "mixed"):
        points["interior"] = 3 + (nx + 1) * (2 + (ny + 1) * 2)
    if mesh == "mixed":
        points["apex"] = (nx + 1) * (ny + 1) * (nz + 1)
    live = {None: 0, cell: 0}  # a point under cells with s = 1 moves nothing of a free source: count the tangents that are not zero
    for name, p in points.items():
        dX = np.zeros((m.n_points, 3))
        dX[p] = (0.3, -0.5, 0.8)
        gd = H.Geom(m, m.points + 1e-30j * dX)
        for snap in (None, cell):
            _, d = emu_shape(emu, case, pars, eps, cell=snap, dX=dX)
            ref = np.imag(HS.smooth_shape(gd, pars, eps, center=None if snap is None else gd.C[snap])) / 1e-30
            print(mesh, name, "point", p, "snapped" if snap is not None else "free", rel(d, ref))
            assert np.isfinite(d).all() and rel(d, ref) <= 1e-10
            live[snap] += int(np.abs(ref).max() > 0)
            if snap is not None:
                assert d[cell] == 0.0
    assert live[None] >= 1 and live[cell] >= 2


# ---- the residual with sources on the host -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_hostemu_residual_with_sources(emu, mesh):
    case, g, S = source_case(mesh), geom(mesh), sources(mesh)
    T = np.ascontiguousarray(case.states)
    q = np.ascontiguousarray(np.real(S.field(g)))
    cs = CaseStruct(case)
    for normalized in (1, 0):
        R, R0, Rn = np.zeros(T.size), np.zeros(T.size), np.zeros(T.size)
        assert emu.emu_hs_residual(cs.byref(), dptr(T), T.size, normalized, dptr(q), dptr(R)) == 0
        ref = HS.residual(case, g, T, S, normalized=bool(normalized))
        print(mesh, "normalized", normalized, rel(R, ref))
        assert rel(R, ref) <= 1e-12
        # without a source the src pointer is null and the row is, bit for bit, the residual without the term
        assert emu.emu_hs_residual(cs.byref(), dptr(T), T.size, normalized, None, dptr(R0)) == 0
        Rp = np.zeros(T.size)
        assert emu.plain.emu_heat_residual(cs.byref(), dptr(T), T.size, 0, normalized, None, dptr(Rp), dptr(np.zeros(T.size))) == 0
        assert np.array_equal(R0, Rp) and rel(R0, H.residual(case, g, T, normalized=bool(normalized))) <= 1e-12
        assert not np.array_equal(R0, R)
        z = np.zeros(T.size)
        assert emu.emu_hs_residual(cs.byref(), dptr(T), T.size, normalized, dptr(z), dptr(Rn)) == 0
        assert np.array_equal(Rn, R0)


# ---- the membership rule of cylinderToCell ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ALL_MESHES)
def test_cylinder_to_cell_membership_against_a_loop(mesh):
    g = geom(mesh)
    p1, p2, r = np.array(SOURCE_B["p1"]), np.array(SOURCE_B["p2"]), SOURCE_B["radius"]
    a = p2 - p1
    brute = []
    for c in range(g.nC):
        d = g.C[c] - p1
        mag = float(d @ a)
        if 0 < mag < a @ a and d @ d - mag * mag / (a @ a) < r * r:
            brute.append(c)
    cells = HS.cylinder_cells(g, p1, p2, r)
    assert list(cells) == brute and 0 < len(brute) == B_CELLS[mesh] < g.nC
    s = pyDASolvers("DAHeatTransferFoam -python", heat_options(source_case(mesh), fvSource={"b": SOURCE_B}), case=source_case(mesh))
    info = s.heatSourceInfo("b")
    assert list(info["cells"]) == brute and info["snappedCell"] is None


# ---- host-side errors, by name ------------------------------------------------------------------------------------------------------
def make(case, **opts):
    return pyDASolvers("DAHeatTransferFoam -python", heat_options(case, **opts), case=case)


def test_constructor_accepts_the_sources_and_snaps_to_the_cell():
    case = heat_case("bump", "const")
    s = make(case, fvSource=dict(ALL_SOURCES), inputInfo={"hs": {"type": "fvSourcePar", "fvSourceName": "mid_A", "indices": [0, 6], "components": ["solver"]}})
    assert s.getInputSize("hs", "fvSourcePar") == 2
    info = s.heatSourceInfo("head_C")
    assert info["snappedCell"] == sources("bump").entries["head_C"]["cell"]
    assert rel(info["snappedCenter"], geom("bump").C[info["snappedCell"]]) <= 1e-14
    assert np.array_equal(s.heatSourceInfo("mid_A")["pars"], sources("bump").entries["mid_A"]["pars"].real)
    assert s.heatSourceInfo("mid_A")["snappedCell"] is None
    s2 = make(case, fvSource={"a": SOURCE_A}, inputInfo={"hs": {"type": "fvSourcePar", "fvSourceName": "a"}})
    assert s2.getInputSize("hs", "fvSourcePar") == 9


@pytest.mark.parametrize("entry, words", [
    ({"type": "heatSource"}, "source"),
    ({"type": "heatSource", "source": "cylinderSmooth", "center": [0.4, 0.1, 0.05], "axis": [1, 0, 0], "radius": 0.04, "length": 0.3, "power": 1.0}, "eps"),
    ({"type": "heatSource", "source": "cylinderToCell", "p1": [0.3, 0.1, 0.05], "radius": 0.06, "power": 1.0}, "p2"),
    ({"type": "heatSource", "source": "cylinderAnnulusToCell", "p1": [0, 0, 0], "p2": [1, 0, 0], "radius": 0.1, "power": 1.0}, "cylinderAnnulusToCell"),
    ({"type": "actuatorDisk", "source": "cylinderAnnulusSmooth"}, "actuatorDisk"),
    (dict(SOURCE_B, p1=[3.0, 0.1, 0.05], p2=[4.0, 0.1, 0.05]), "no cell"),
    (dict(SOURCE_A, center=[0.43, 0.11, 0.5], snapCenter2Cell=1), "within a cell"),
    (dict(SOURCE_A, axis=[0.0, 0.0, 0.0]), "axis"),
])
def test_bad_entries_are_refused_by_name(entry, words):
    with pytest.raises(_capi.DASError, match="fvSource.*heat_1") as e:
        make(heat_case("bump", "const"), fvSource={"heat_1": entry})
    assert words in str(e.value)


def test_a_center_on_a_face_finds_two_cells_and_is_refused():
    case = heat_transfer_case_box()
    with pytest.raises(_capi.DASError, match="fvSource.*on_face.*2 was returned"):
        make(case, fvSource={"on_face": dict(SOURCE_A, center=[0.5, 0.125, 0.0625], snapCenter2Cell=1)})


def heat_transfer_case_box():
    from dafoam_amd.meshgen import heat_transfer_case

    return heat_transfer_case(4, 4, 4, lengths=(1.0, 0.2, 0.1), kappa=200.0, mapping=None)


def test_fv_source_par_errors_by_name():
    case = heat_case("bump", "const")
    src = {"a": SOURCE_A, "b": SOURCE_B}
    s = make(case, fvSource=src, inputInfo={"on_b": {"type": "fvSourcePar", "fvSourceName": "b"}, "nobody": {"type": "fvSourcePar", "fvSourceName": "zz"},
                                            "far": {"type": "fvSourcePar", "fvSourceName": "a", "indices": [0, 9]}})
    with pytest.raises(_capi.DASError, match=r"on_b.*fvSource\[b\].*cylinderToCell"):
        s.getInputSize("on_b", "fvSourcePar")
    with pytest.raises(_capi.DASError, match="fvSourceName zz.*fvSource"):
        s.getInputSize("nobody", "fvSourcePar")
    with pytest.raises(_capi.DASError, match=r"index 9 of fvSource\[a\]"):
        s.getInputSize("far", "fvSourcePar")
    # the C entries say the same on their own
    L = _capi.lib()
    idx = np.array([9], dtype=np.int32)
    one = np.ones(1)
    assert L.das_set_heat_source_pars(s._h, b"a", idx.ctypes.data_as(_capi.c_int_p), 1, dptr(one)) < 0
    assert "index 9 of fvSource a" in L.das_last_error().decode()
    idx[0] = 0
    assert L.das_set_heat_source_pars(s._h, b"b", idx.ctypes.data_as(_capi.c_int_p), 1, dptr(one)) < 0
    assert "fvSource b is a cylinderToCell source" in L.das_last_error().decode()
    assert L.das_set_heat_source_pars(s._h, b"zz", idx.ctypes.data_as(_capi.c_int_p), 1, dptr(one)) < 0
    assert "fvSource has no heat source zz" in L.das_last_error().decode()


def test_fv_source_on_a_flow_solver_is_refused_by_name():
    case = channel_case(4, 4, 3)
    opts = {"solverName": "DASimpleFoam", "adjEqnOption": {"printInfo": 0}}
    with pytest.raises(_capi.DASError, match=r"fvSource\[disk1\].*DASimpleFoam"):
        pyDASolvers("DASimpleFoam -python", dict(opts, fvSource={"disk1": {"type": "actuatorDisk"}}), case=case)
    with pytest.raises(_capi.DASError, match=r"fvSource\[heat\].*DASimpleFoam"):
        pyDASolvers("DASimpleFoam -python", dict(opts, fvSource={"heat": SOURCE_A}), case=case)
    s = pyDASolvers("DASimpleFoam -python", dict(opts, fvSource={}), case=case)
    pars = np.array(SOURCE_A["center"] + SOURCE_A["axis"] + [0.04, 0.3, 1.0])
    assert _capi.lib().das_define_heat_source(s._h, b"heat", b"cylinderSmooth", dptr(pars), 0.03, 0) < 0
    assert "fvSource" in _capi.lib().das_last_error().decode()

"""CPU tier of the actuator disks of DASimpleFoam (the fvSource option, type actuatorDisk, and the fvSourcePar input): the numpy
restatement (tests/actuator_disk_restatement.py) on its own, the kernel body body_actuator_disk and body_cell / body_cell2 with the src3
pointer run on the host (tests/hostemu/hostemu_actuator_disk.cpp) against it, the membership rule of cylinderAnnulusToCell, and the
refusals by name, through Python and the C entries.
Bounds (tests/README_heat_transfer.md): values 1e-12, tangents 1e-10 against the complex step of the restatement, fields relative to their
maximum; "bitwise" is np.array_equal."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import actuator_disk_restatement as AD
from actuator_disk_cases import ALL_DISKS, DISK_A, DISK_B, DISK_C, MESHES, disk_case, disks, geom, options
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import channel_case, heat_transfer_case, rho_channel_case, scalar_transport_case, simple_T_channel_case, turbo_channel_case
from dafoam_amd.pyDASolvers import pyDASolvers
from oracle.foam_mesh import Geometry
from oracle.residual import simple_residual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = _capi.c_double_p
UNNORMALISED = ("TRes",)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_actuator_disk.cpp through g++, as tests/test_heat_source_cpu.py builds its harness; and the harness of the
    residual as it stands (tests/hostemu/hostemu.cpp), for the bitwise comparison."""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    d = tmp_path_factory.mktemp("hostemu")
    libs = []
    for src in ("hostemu_actuator_disk.cpp", "hostemu.cpp"):
        so = str(d / ("lib" + src.replace(".cpp", ".so")))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                               "-o", so, os.path.join(ROOT, "tests", "hostemu", src), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
        libs.append(C.CDLL(so))
    L, L.plain = libs
    L.emu_ad_force.argtypes = [C.POINTER(das_case_t), C.c_int, dp, C.c_double, C.c_double, dp, dp, dp, dp, C.POINTER(C.c_int)]
    L.emu_ad_residual.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, C.c_int, C.c_int, dp, dp]
    L.plain.emu_residual.argtypes = [C.POINTER(das_case_t), dp, C.c_longlong, C.c_int, dp, dp, dp]
    L.plain.emu_set_cell_split.argtypes = [C.c_int]
    return L


def emu_force(L, case, e, pars=None, dpar=None, dX=None):
    """(f5 (n, 5), tangent (n, 5), degenerate cells) of the entry e of a Disks at the parameters pars"""
    n = case.mesh.n_cells
    fv, fd, deg = np.zeros((n, 5)), np.zeros((n, 5)), C.c_int(0)
    arr = lambda a: None if a is None else dptr(np.ascontiguousarray(a, dtype=np.float64).ravel())
    p = np.real(e["pars"] if pars is None else pars)
    assert L.emu_ad_force(CaseStruct(case).byref(), int(e["smooth"]), arr(p), e["eps"], 1.0 if e["rotDir"] == "left" else -1.0, arr(dpar), arr(dX), dptr(fv), dptr(fd),
                          C.byref(deg)) == 0
    return fv, fd, deg.value


def ref_force(g, e, pars=None):
    p = e["pars"] if pars is None else pars
    f, fa, fc, _, _ = AD.disk_force(g.C, p, e["eps"], e["rotDir"], e["smooth"])
    return np.column_stack([f, fa, fc])


# ---- the restatement on its own, and what the cases promise -------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_cases_every_branch_both_signs_no_cell_on_an_axis(mesh):
    g, S = geom(mesh), disks(mesh)
    for name in ("mid_A", "head_C"):
        e = S.entries[name]
        p = e["pars"].real
        f, fa, fc, rStar, rLen = AD.disk_force(g.C, p, e["eps"], e["rotDir"], True, scale=1.0)
        epsR = e["eps"] / (p[7] - p[6])
        inner, mid, outer = rStar < epsR, (rStar >= epsR) & (rStar <= 1 - epsR), rStar > 1 - epsR
        peak = np.abs(f).max()
        shares = [float(np.abs(f[m]).max() / peak) for m in (inner, mid, outer)]
        fp = AD.disk_force(g.C, p, e["eps"], e["rotDir"], True, scale=1.0, projection=True)[0]
        print(mesh, name, "cells per branch", inner.sum(), mid.sum(), outer.sum(), "peak share", shares, "min |r|", rLen.min(), "projection",
              np.abs(f - fp).max() / peak)
        # each branch holds cells whose force is far above the 1e-12 bound, relative to the peak
        assert min(shares) > 1e-3 and rLen.min() > 1e-4
        # the projection reading n (c . n) is another field altogether: no 1e-12 test can pass with it
        assert np.abs(f - fp).max() > 0.1 * peak
    assert S.entries["mid_A"]["rotDir"] != S.entries["head_C"]["rotDir"] == S.entries["tail_B"]["rotDir"]
    b = S.entries["tail_B"]
    assert 0 < b["cells"].size < g.nC
    rB = AD.disk_force(g.C[b["cells"]], b["pars"].real, 0.0, b["rotDir"], False)[4]
    assert rB.min() >= b["pars"][6].real
    # the thrust of C is the target, whatever scale says
    thrust = S.entry(g, "head_C")[1]
    print(mesh, "thrust of C", thrust, "scale", S.scale(g, "head_C"))
    assert abs(thrust - DISK_C["targetThrust"]) <= 1e-13 * DISK_C["targetThrust"]
    assert np.array_equal(S.entry(g, "head_C")[0], S.entry(g, "head_C", S.entries["head_C"]["pars"] + 5.0 * np.eye(13)[8])[0])


def test_restatement_complex_step_against_central_differences():
    g = geom("bump")
    for name in ("mid_A", "head_C"):
        S = disks("bump", (name,))
        p0 = S.entries[name]["pars"].real
        unread = 8 if name == "head_C" else 12
        for i in range(13):
            dcs = np.imag(S.field(g, {name: p0 + 1e-30j * np.eye(13)[i]})) / 1e-30
            h = 1e-6 * max(abs(p0[i]), 1e-2)
            dfd = np.real(S.field(g, {name: p0 + h * np.eye(13)[i]}) - S.field(g, {name: p0 - h * np.eye(13)[i]})) / (2 * h)
            if i == unread:
                assert not dcs.any() and not dfd.any()
                continue
            print(name, AD.PAR_NAMES[i], rel(dfd, dcs))
            assert np.abs(dcs).max() > 0 and rel(dfd, dcs) <= 1e-6


@pytest.mark.parametrize("mesh", MESHES)
def test_residual_variant_with_a_zero_field_has_the_bits_of_the_oracle(mesh):
    case = disk_case(mesh)
    go, W = Geometry(case.mesh), case.states
    for kw in (dict(), dict(normalize=UNNORMALISED), dict(isPC=True)):
        R0 = simple_residual(case, go, W, **kw)
        assert np.array_equal(R0, AD.simple_residual_with_source(case, go, W, **kw))
        assert np.array_equal(R0, AD.simple_residual_with_source(case, go, W, fvSource=np.zeros((go.nC, 3)), **kw))
    # the complex-safe metrics are the oracle's
    assert rel(AD.residual(case, geom(mesh), W), simple_residual(case, go, W)) <= 1e-13
    # the source reaches the p and phi rows through H, not only the U rows
    N = go.nC
    d = np.real(AD.residual(case, geom(mesh), W, disks(mesh)) - AD.residual(case, geom(mesh), W))
    assert np.abs(d[: 3 * N]).max() > 1.0 and np.abs(d[3 * N: 4 * N]).max() > 1e-3 and np.abs(d[5 * N:]).max() > 1e-3 and not d[4 * N: 5 * N].any()


# ---- body_actuator_disk on the host ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["flat", "bump", "mixed"])
def test_hostemu_force_values_and_parameter_tangents(emu, mesh):
    case, g, S = disk_case(mesh), geom(mesh), disks(mesh)
    for name in ("mid_A", "head_C"):
        e = S.entries[name]
        ref = ref_force(g, e)
        fv, _, deg = emu_force(emu, case, e)
        print(mesh, name, "values", rel(fv, ref))
        assert deg == 0 and rel(fv, ref) <= 1e-12
        for i in range(12):  # targetThrust is no parameter of the body: the sum that uses it is the kernels'
            v, d, _ = emu_force(emu, case, e, dpar=np.eye(13)[i])
            dcs = np.imag(ref_force(g, e, e["pars"] + 1e-30j * np.eye(13)[i])) / 1e-30
            print(mesh, name, AD.PAR_NAMES[i], rel(d, dcs))
            assert rel(v, ref) <= 1e-12 and np.abs(dcs).max() > 0 and np.isfinite(d).all() and rel(d, dcs) <= 1e-10
    # the Hoekstra form of cylinderAnnulusToCell on the cells of the set
    b = S.entries["tail_B"]
    fv, _, _ = emu_force(emu, case, b)
    refB = ref_force(g, b)
    assert rel(fv[b["cells"]], refB[b["cells"]]) <= 1e-12


@pytest.mark.parametrize("mesh", ["bump", "mixed"])
def test_hostemu_force_dual_metrics(emu, mesh):
    case, g, S = disk_case(mesh), geom(mesh), disks(mesh)
    m = case.mesh
    e = S.entries["mid_A"]
    near = int(np.argmax(np.abs(ref_force(g, e)[:, 3])))
    points = {"in_disk": int(m.face_pts[m.face_ptr[int(np.nonzero(m.owner == near)[0][0])]]), "corner": 0, "far_corner": m.n_points - 1 if mesh == "bump" else 20}
    live = 0
    for name, p in points.items():
        dX = np.zeros((m.n_points, 3))
        dX[p] = (0.3, -0.5, 0.8)
        gd = AD.FlowGeom(m, m.points + 1e-30j * dX)
        for dname in ("mid_A", "tail_B"):
            e = S.entries[dname]
            _, d, _ = emu_force(emu, case, e, dX=dX)
            ref = np.imag(ref_force(gd, e)) / 1e-30
            rows = slice(None) if e["smooth"] else e["cells"]
            scale = max(np.abs(ref[rows]).max(), 1e-300)
            print(mesh, name, dname, "point", p, float(np.abs(d[rows] - ref[rows]).max() / scale), "max", scale)
            assert np.isfinite(d[rows]).all()
            if np.abs(ref[rows]).max() > 0:
                live += 1
                assert np.abs(d[rows] - ref[rows]).max() <= 1e-10 * scale
            else:
                assert not d[rows].any()
    assert live >= 2


def test_hostemu_reports_a_cell_centre_on_the_axis(emu):
    case, g = disk_case("flat"), geom("flat")
    e = dict(disks("flat").entries["mid_A"])
    pars = e["pars"].real.copy()
    s = pyDASolvers("DASimpleFoam -python", options(), case=case)
    Cc = np.zeros(3 * g.nC)  # the library's own centres: the last bits decide
    _capi.check(_capi.lib().das_get_geometry(s._h, None, None, dptr(Cc), None, None, None, None, None))
    pars[0:3] = Cc[3 * 77: 3 * 77 + 3]
    _, _, deg = emu_force(emu, case, e, pars=pars)
    assert deg == 1


# ---- the residual with sources on the host -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["flat", "bump", "mixed"])
@pytest.mark.parametrize("split", [0, 1])
def test_hostemu_residual_with_sources(emu, mesh, split):
    case, g, S = disk_case(mesh), geom(mesh), disks(mesh)
    W = np.ascontiguousarray(case.states)
    q = np.ascontiguousarray(np.real(S.field(g)))
    cs = CaseStruct(case)
    for normalized in (1, 0):
        kw = {} if normalized else dict(normalize=UNNORMALISED)
        R, R0, Rn = np.zeros(W.size), np.zeros(W.size), np.zeros(W.size)
        assert emu.emu_ad_residual(cs.byref(), dptr(W), W.size, split, normalized, dptr(q), dptr(R)) == 0
        ref = np.real(AD.residual(case, g, W, S, **kw))
        N = g.nC
        blocks = {"U": slice(0, 3 * N), "p": slice(3 * N, 4 * N), "nuTilda": slice(4 * N, 5 * N), "phi": slice(5 * N, None)}
        errs = {k: rel(R[sl], ref[sl]) for k, sl in blocks.items()}
        print(mesh, "split", split, "normalized", normalized, errs)
        assert max(errs.values()) <= 1e-12
        # with the pointer null the rows are, bit for bit, those of the harness as it stands; a zero field changes no bit either
        assert emu.emu_ad_residual(cs.byref(), dptr(W), W.size, split, normalized, None, dptr(R0)) == 0
        assert emu.emu_ad_residual(cs.byref(), dptr(W), W.size, split, normalized, dptr(np.zeros((N, 3))), dptr(Rn)) == 0
        assert np.array_equal(Rn, R0) and not np.array_equal(R0, R)
        if normalized:
            Rp = np.zeros(W.size)
            emu.plain.emu_set_cell_split(split)
            try:
                assert emu.plain.emu_residual(cs.byref(), dptr(W), W.size, 0, None, dptr(Rp), None) == 0
            finally:
                emu.plain.emu_set_cell_split(0)
            assert np.array_equal(R0, Rp)


def test_hostemu_residual_with_sources_and_a_T_field(emu):
    """prm.hasT: states [U | p | T | nuTilda | phi]; body_cell with src3 set (the face / cell split does not serve this layout)"""
    case = simple_T_channel_case(10, 8, 6)
    g = AD.FlowGeom(case.mesh)
    S = AD.Disks(g, ALL_DISKS)
    W = np.ascontiguousarray(case.states)
    q = np.ascontiguousarray(np.real(S.field(g)))
    N = g.nC
    blocks = {"U": slice(0, 3 * N), "p": slice(3 * N, 4 * N), "T": slice(4 * N, 5 * N), "nuTilda": slice(5 * N, 6 * N), "phi": slice(6 * N, None)}
    cs = CaseStruct(case)
    for normalized in (1, 0):
        R, R0 = np.zeros(W.size), np.zeros(W.size)
        assert emu.emu_ad_residual(cs.byref(), dptr(W), W.size, 0, normalized, dptr(q), dptr(R)) == 0
        assert emu.emu_ad_residual(cs.byref(), dptr(W), W.size, 0, normalized, None, dptr(R0)) == 0
        ref = np.real(AD.residual(case, g, W, S, **({} if normalized else dict(normalize=UNNORMALISED))))
        errs = {k: rel(R[sl], ref[sl]) for k, sl in blocks.items()}
        print("T field, normalized", normalized, errs)
        assert max(errs.values()) <= 1e-12
        assert np.array_equal(R[blocks["T"]], R0[blocks["T"]]) and not np.array_equal(R[blocks["U"]], R0[blocks["U"]])
    assert emu.emu_ad_residual(cs.byref(), dptr(W), W.size, 1, 1, dptr(q), dptr(R)) != 0  # the split refuses a T field


# ---- the membership rule of cylinderAnnulusToCell -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", MESHES)
def test_annulus_membership_against_a_loop(mesh):
    g = geom(mesh)
    p1, p2, ri, ro = np.array(DISK_B["p1"]), np.array(DISK_B["p2"]), DISK_B["innerRadius"], DISK_B["outerRadius"]
    a = p2 - p1
    brute = []
    for c in range(g.nC):
        d = g.C[c].real - p1
        mag = float(d @ a)
        if 0 < mag < a @ a and ri * ri < d @ d - mag * mag / (a @ a) < ro * ro:
            brute.append(c)
    assert list(AD.annulus_cells(g, p1, p2, ri, ro)) == brute and 0 < len(brute) < g.nC
    s = pyDASolvers("DASimpleFoam -python", options(fvSource={"b": DISK_B}), case=disk_case(mesh))
    info = s.actuatorDiskInfo("b")
    assert list(info["cells"]) == brute and info["nCells"] == len(brute)
    assert rel(info["pars"][:10], disks(mesh).entries["tail_B"]["pars"].real[:10]) <= 1e-15


# ---- constructing, and the refusals by name -------------------------------------------------------------------------------------------
def make(case=None, **opts):
    return pyDASolvers("DASimpleFoam -python", options(**opts), case=case or disk_case("bump"))


def test_constructor_accepts_the_disks_and_the_inputs():
    s = make(fvSource=dict(ALL_DISKS), inputInfo={"two": {"type": "fvSourcePar", "fvSourceName": "mid_A", "indices": [0, 7], "components": ["solver"]},
                                                  "all": {"type": "fvSourcePar", "fvSourceName": "head_C"}})
    assert s.getInputSize("two", "fvSourcePar") == 2 and s.getInputSize("all", "fvSourcePar") == 13
    assert np.array_equal(s.actuatorDiskInfo("mid_A")["pars"], disks("bump").entries["mid_A"]["pars"].real)
    assert s.actuatorDiskInfo("mid_A")["nCells"] == disk_case("bump").mesh.n_cells and s.actuatorDiskInfo("mid_A")["cells"].size == 0
    # with a T field as well
    make(case=simple_T_channel_case(10, 8, 6), fvSource=dict(ALL_DISKS))


def test_the_reference_docstring_example_constructs():
    """DAFvSourceActuatorDisk.C:58-89, the geometry scaled into the 1.0 x 0.2 x 0.1 channel; the keys as they stand there (no adjustThrust,
    no targetThrust)."""
    fv = {"disk1": {"type": "actuatorDisk", "source": "cylinderAnnulusToCell", "p1": [0.3, 0.1, 0.05], "p2": [0.5, 0.1, 0.05], "innerRadius": 0.01,
                    "outerRadius": 0.08, "rotDir": "left", "scale": 1.0, "POD": 0.7},
          "disk2": {"type": "actuatorDisk", "source": "cylinderAnnulusSmooth", "center": [0.6, 0.1, 0.05], "direction": [1.0, 0.0, 0.0], "innerRadius": 0.01,
                    "outerRadius": 0.08, "rotDir": "right", "scale": 0.1, "POD": 1.0, "eps": 0.02, "expM": 1.0, "expN": 0.5}}
    s = make(fvSource=fv)
    assert s.actuatorDiskInfo("disk1")["nCells"] > 0 and s.actuatorDiskInfo("disk2")["pars"][8] == 0.1


@pytest.mark.parametrize("entry, words", [
    ({"type": "actuatorDisk"}, "source"),
    (dict(DISK_A, source="cylinderToCell"), "cylinderToCell not supported"),
    ({k: v for k, v in DISK_A.items() if k != "eps"}, "eps"),
    ({k: v for k, v in DISK_A.items() if k != "expM"}, "expM"),
    ({k: v for k, v in DISK_B.items() if k != "p2"}, "p2"),
    ({k: v for k, v in DISK_B.items() if k != "rotDir"}, "rotDir"),
    (dict(DISK_A, rotDir="up"), "rotDir not valid"),
    (dict(DISK_A, center=[0.4, 0.1]), "center needs 3"),
    (dict(DISK_A, direction=[0.0, 0.0, 0.0]), "direction"),
    (dict(DISK_A, eps=0.05), "eps"),
    (dict(DISK_B, p1=[3.0, 0.1, 0.05], p2=[4.0, 0.1, 0.05]), "no cell"),
    ({"type": "actuatorLine"}, "actuatorLine"),
    ({"type": "actuatorPoint"}, "actuatorPoint"),
    ({"type": "uniformPressureGradient"}, "uniformPressureGradient"),
    ({"type": "heatSource", "source": "cylinderSmooth"}, "heatSource"),
])
def test_bad_entries_are_refused_by_name(entry, words):
    with pytest.raises(_capi.DASError, match=r"fvSource.*disk_1") as e:
        make(fvSource={"disk_1": entry})
    assert words in str(e.value)


@pytest.mark.parametrize("solver, case_of, words", [
    ("DARhoSimpleFoam", lambda: rho_channel_case(4, 4, 3), "fvSourceEnergy"),
    ("DATurboFoam", lambda: turbo_channel_case(4, 4, 3), "DATurboFoam"),
    ("DAScalarTransportFoam", lambda: scalar_transport_case(4, 4, 3), "DAScalarTransportFoam"),
    ("DAHeatTransferFoam", lambda: heat_transfer_case(4, 4, 3, kappa=200.0), "actuatorDisk"),
])
def test_other_solvers_refuse_the_disks_by_name(solver, case_of, words):
    case = case_of()
    with pytest.raises(_capi.DASError, match=r"fvSource\[disk1\]") as e:
        pyDASolvers(f"{solver} -python", {"solverName": solver, "adjEqnOption": {"printInfo": 0}, "fvSource": {"disk1": DISK_A}}, case=case)
    assert words in str(e.value)
    # the C entries say the same on their own
    s = pyDASolvers(f"{solver} -python", {"solverName": solver, "adjEqnOption": {"printInfo": 0}}, case=case)
    L = _capi.lib()
    pars = np.array(DISK_A["center"] + DISK_A["direction"] + [0.01, 0.08, 1.0, 0.7, 1.0, 0.5, 0.0])
    assert L.das_define_actuator_disk(s._h, b"disk1", b"cylinderAnnulusSmooth", dptr(pars), b"left", 0.02, 0) < 0
    msg = L.das_last_error().decode()
    assert "fvSource" in msg and solver in msg
    assert L.das_get_fv_source_vector(s._h, dptr(np.zeros(3 * case.mesh.n_cells))) < 0 and "fvSource" in L.das_last_error().decode()


def test_sharded_solvers_refuse_the_disks_by_name():
    from dafoam_amd.distributed import refuse_fv_source

    refuse_fv_source({"fvSource": {}})
    refuse_fv_source({})
    with pytest.raises(_capi.DASError, match=r"fvSource\[a\].*sharded"):
        refuse_fv_source({"fvSource": {"a": DISK_A}})
    s = make(fvSource={"a": DISK_A})
    L = _capi.lib()
    mask = np.ones(disk_case("bump").states.size, dtype=np.uint8)
    assert L.das_set_owned_mask(s._h, mask.ctypes.data_as(C.POINTER(C.c_ubyte))) < 0
    assert "fvSource" in L.das_last_error().decode() and "sharded" in L.das_last_error().decode()
    s2 = make()
    assert L.das_set_owned_mask(s2._h, mask.ctypes.data_as(C.POINTER(C.c_ubyte))) == 0
    pars = np.array(DISK_A["center"] + DISK_A["direction"] + [0.01, 0.08, 1.0, 0.7, 1.0, 0.5, 0.0])
    assert L.das_define_actuator_disk(s2._h, b"a", b"cylinderAnnulusSmooth", dptr(pars), b"left", 0.02, 0) < 0
    assert "sharded" in L.das_last_error().decode()


def test_simple_iteration_refuses_while_a_disk_is_defined():
    s = make(fvSource={"a": DISK_A})
    assert _capi.lib().das_simple_iteration(s._h, 1, 0.3, 1e-6, 50, None) < 0
    msg = _capi.lib().das_last_error().decode()
    assert "das_simple_iteration" in msg and "fvSource" in msg


def test_fv_source_par_and_field_input_errors_by_name():
    s = make(fvSource={"a": DISK_A, "b": DISK_B},
             inputInfo={"on_b": {"type": "fvSourcePar", "fvSourceName": "b"}, "nobody": {"type": "fvSourcePar", "fvSourceName": "zz"},
                        "far": {"type": "fvSourcePar", "fvSourceName": "a", "indices": [0, 13]}, "neg": {"type": "fvSourcePar", "fvSourceName": "a", "indices": [-1]},
                        "fld": {"type": "field", "fieldName": "fvSource", "fieldType": "vector"}})
    with pytest.raises(_capi.DASError, match=r"on_b.*fvSource\[b\].*cylinderAnnulusToCell"):
        s.getInputSize("on_b", "fvSourcePar")
    with pytest.raises(_capi.DASError, match="fvSourceName zz.*fvSource"):
        s.getInputSize("nobody", "fvSourcePar")
    with pytest.raises(_capi.DASError, match=r"index 13 of fvSource\[a\]"):
        s.getInputSize("far", "fvSourcePar")
    with pytest.raises(_capi.DASError, match=r"index -1 of fvSource\[a\]"):
        s.getInputSize("neg", "fvSourcePar")
    with pytest.raises(_capi.DASError, match=r"fld.*fieldName fvSource"):
        s.setSolverInput("fld", "field", 3 * disk_case("bump").mesh.n_cells, np.zeros(3 * disk_case("bump").mesh.n_cells))
    # the C entries say the same on their own
    L = _capi.lib()
    idx = np.array([13], dtype=np.int32)
    one = np.ones(1)
    assert L.das_set_actuator_disk_pars(s._h, b"a", idx.ctypes.data_as(_capi.c_int_p), 1, dptr(one)) < 0
    assert "index 13 of fvSource a" in L.das_last_error().decode()
    idx[0] = 0
    assert L.das_set_actuator_disk_pars(s._h, b"b", idx.ctypes.data_as(_capi.c_int_p), 1, dptr(one)) < 0
    assert "fvSource b is a cylinderAnnulusToCell disk" in L.das_last_error().decode()
    assert L.das_set_actuator_disk_pars(s._h, b"zz", idx.ctypes.data_as(_capi.c_int_p), 1, dptr(one)) < 0
    assert "fvSource has no actuator disk zz" in L.das_last_error().decode()
    pars = np.array(DISK_A["center"] + DISK_A["direction"] + [0.01, 0.08, 1.0, 0.7, 1.0, 0.5, 0.0])
    assert L.das_define_actuator_disk(s._h, b"c", b"cylinderAnnulusSmooth", dptr(pars), b"up", 0.02, 0) < 0
    assert "rotDir not valid" in L.das_last_error().decode()
    assert L.das_define_actuator_disk(s._h, b"c", b"cylinderSmooth", dptr(pars), b"left", 0.02, 0) < 0
    assert "not supported" in L.das_last_error().decode()
    # a refused parameter leaves the disk as it was
    idx[0] = 7
    assert L.das_set_actuator_disk_pars(s._h, b"a", idx.ctypes.data_as(_capi.c_int_p), 1, dptr(np.array([0.005]))) < 0
    assert s.actuatorDiskInfo("a")["pars"][7] == DISK_A["outerRadius"]

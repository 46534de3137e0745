"""thermalCouplingOutput without a GPU: the numpy restatement (tests/thermal_coupling_restatement.py) against its own rules, against the
restated wallHeatFlux and against the oracle's patch-field formula, and the kernel body (body_thermal_coupling, csrc/das_kernels.hpp) run
on the host (tests/hostemu/hostemu_thermalcoupling.cpp) against the restatement."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import function_restatement_more as FM
import thermal_coupling_restatement as TC
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import BC_FIXED_VALUE, BC_ZERO_GRADIENT, channel_case, rho_channel_case, simple_T_channel_case, turbo_channel_case
from mixed_mesh import mixed
from oracle.foam_mesh import Geometry
from oracle.residual import bc_scalar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = "thermalCouplingOutput"


def build_case(which):
    """6 x 5 x 4 channels with wall functions on the walls, and the 148-cell pyramid / prism / polyhedron mesh as DARhoSimpleFoam."""
    if which == "mixed":
        return mixed("rho", wall_function=True)
    return {"simpleT": simple_T_channel_case, "rho": rho_channel_case, "turbo": turbo_channel_case}[which](6, 5, 4, wall_function=True, perturb=0.02)


def hot_wall(case):
    """The case with a fixedValue T on the bottom wall (the compressible channels come with adiabatic walls)."""
    c = copy.copy(case)
    c.bcs = copy.deepcopy(case.bcs)
    c.bcs["bottom"]["T"] = (BC_FIXED_VALUE, 320.0)
    return c


@pytest.fixture(scope="module")
def channel():
    case = build_case("simpleT")
    return case, Geometry(case.mesh)


# ---- the restatement's own rules -----------------------------------------------------------------------------------------------------
def test_size_rule(channel):
    case, g = channel
    # 6 x 5 x 4 cells: a wall has 6 x 4 faces, the inlet 5 x 4
    assert TC.size(case, ["bottom"]) == 2 * 6 * 4
    assert TC.size(case, ["inlet"]) == 2 * 5 * 4
    assert TC.size(case, ["inlet", "bottom"]) == 2 * (6 * 4 + 5 * 4)
    assert TC.output(case, g, case.states, ["inlet", "bottom"]).size == TC.size(case, ["inlet", "bottom"])


def test_patch_order_does_not_matter(channel):
    case, g = channel
    a = TC.output(case, g, case.states, ["inlet", "bottom"])
    b = TC.output(case, g, case.states, ["bottom", "inlet"])
    assert np.array_equal(a, b)
    # and the sorted order is the one used: each half starts with the bottom wall's
    nB, nF = 6 * 4, 6 * 4 + 5 * 4
    alone = TC.output(case, g, case.states, ["bottom"])
    assert np.array_equal(a[:nB], alone[:nB]) and np.array_equal(a[nF : nF + nB], alone[nB:])
    # the first half is T of the owner cells; bottom and inlet share a row of cells, whose T appears once per patch
    N = g.nC
    faces = TC.selected_faces(case, ["inlet", "bottom"])
    owners = case.mesh.owner[faces]
    assert np.array_equal(a[:nF], case.states[4 * N : 5 * N][owners])
    assert np.intersect1d(owners[:nB], owners[nB:]).size == 4


def test_bad_wall_distance_method_is_named(channel):
    case, g = channel
    with pytest.raises(ValueError, match="wallDistanceMethod: meshWave not supported! Options are: default and daCustom."):
        TC.output(case, g, case.states, ["bottom"], "meshWave")


@pytest.mark.parametrize("which", ["simpleT", "rho"])
@pytest.mark.parametrize("mode", TC.MODES)
def test_kappa_over_d_gives_the_wall_heat_flux(which, mode):
    """On a fixedValue wall  sum_f kappa/d (T_b - T_c) |Sf|  is the restated wallHeatFlux as the plain sum through the surface."""
    case = hot_wall(build_case(which))
    g = Geometry(case.mesh)
    W = case.states
    nF = TC.size(case, ["bottom"]) // 2
    kd = TC.output(case, g, W, ["bottom"], mode)[nF:]
    t = FM.thermal_boundary(case, g, W)
    sel = TC.selected_faces(case, ["bottom"]) - g.nIF
    dT = (t["xb"] - t["xc"])[sel] / (case.thermo["Cp"] if FM.is_compressible(case) else 1.0)
    total = (kd * dT * g.bMagSf[sel]).sum()
    ref = FM.wall_heat_flux(case, g, W, {"patches": ["bottom"], "byUnitArea": False, "scale": 1.0}, mode)
    print(f"{which} {mode}: sum kappa/d dT |Sf| = {total!r}, wallHeatFlux = {ref!r}, rel {abs(total - ref) / abs(ref):.2e}")
    assert ref != 0.0 and abs(total - ref) <= 1e-12 * abs(ref)


# ---- the mixed patch field and the fraction of the input ---------------------------------------------------------------------------------
def test_mixed_face_is_bc_scalar_at_both_ends():
    rng = np.random.default_rng(2)
    n = 40
    ref, xc, delta, phib = 300.0 + rng.standard_normal(n), 310.0 + rng.standard_normal(n), 50.0 + 10.0 * rng.random(n), rng.standard_normal(n)
    for f, code in ((1.0, BC_FIXED_VALUE), (0.0, BC_ZERO_GRADIENT)):
        mine = TC.mixed_face(ref, f * np.ones(n), xc, delta)
        theirs = bc_scalar(np.full(n, code), ref, xc, delta, phib)
        for a, b in zip(mine, theirs):
            assert np.array_equal(a, b)
    # in between: the value is the weighted mean, the gradient is (x_b - x_c) delta
    f = 0.1 + 0.8 * rng.random(n)
    xb, vic, vbc, gic, gbc = TC.mixed_face(ref, f, xc, delta)
    assert np.abs(xb - (f * ref + (1 - f) * xc)).max() <= 4 * np.finfo(float).eps * 320.0
    assert np.abs(gic * xc + gbc - (xb - xc) * delta).max() <= 1e-12 * np.abs((xb - xc) * delta).max()


@pytest.mark.parametrize("mode", TC.MODES)
def test_fraction_and_its_derivative(channel, mode):
    case, g = channel
    patches = ["inlet", "bottom"]
    nF = TC.size(case, patches) // 2
    W = case.states
    my_k = TC.output(case, g, W, patches, mode)[nF:]
    nk = my_k * (0.2 + 3.0 * np.random.default_rng(8).random(nF))  # fractions spread between 1/6 and 3/4
    f = TC.fraction(case, g, W, patches, nk, mode)
    assert f.min() > 0.15 and f.max() < 0.8 and f.max() - f.min() > 0.3
    assert np.abs(f - nk / (my_k + nk)).max() == 0.0
    h = 1e-30
    cs = TC.fraction(case, g, W, patches, nk + 1j * h * nk, mode).imag / (h * nk)  # every face reads its own nk only: one step does all
    d = TC.dfraction_dnk(case, g, W, patches, nk, mode)
    err = np.abs(d - cs).max() / np.abs(cs).max()
    print(f"{mode}: d fraction / d nk against the complex step, rel max err {err:.2e}")
    assert err <= 1e-13


# ---- the kernel body on the host ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_thermalcoupling.cpp through g++, as tests/test_force_coupling_cpu.py builds its harness."""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    so = str(tmp_path_factory.mktemp("hostemu") / "libhostemu_thermalcoupling.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-o", so, os.path.join(ROOT, "tests", "hostemu", "hostemu_thermalcoupling.cpp"),
                           os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L = C.CDLL(so)
    L.emu_thermal_coupling.argtypes = [C.POINTER(das_case_t), _capi.c_double_p, C.c_longlong, _capi.c_int_p, C.c_int, C.c_int, _capi.c_double_p,
                                       _capi.c_double_p, _capi.c_double_p, _capi.c_double_p]
    for fn, args in ((L.emu_bc_mixed, [C.c_int, _capi.c_double_p, _capi.c_double_p, C.c_double, C.c_double, _capi.c_double_p, _capi.c_double_p, _capi.c_double_p]),
                     (L.emu_bc_scalar, [C.c_int, C.c_int, _capi.c_double_p, _capi.c_double_p, _capi.c_double_p, _capi.c_double_p, _capi.c_double_p])):
        fn.argtypes, fn.restype = args, None
    return L


def test_device_mixed_field_is_bc_scalar_at_both_ends(emu):
    """bc_mixed (csrc/das_kernels.hpp) against bc_scalar of the same header at valueFraction 1 (fixedValue) and 0 (zeroGradient), bit for
    bit, for T itself and for the enthalpy Cp (T - Tref); in between against the restated mixed face."""
    rng = np.random.default_rng(2)
    n = 40
    ref, xc, delta, phib = 300.0 + rng.standard_normal(n), 310.0 + rng.standard_normal(n), 50.0 + 10.0 * rng.random(n), rng.standard_normal(n)
    Cp = 1005.0
    for scale, shift in ((1.0, 0.0), (Cp, FM.TREF)):
        x = scale * (xc - shift)
        for f, code in ((1.0, BC_FIXED_VALUE), (0.0, BC_ZERO_GRADIENT)):
            a, b = np.zeros((n, 5)), np.ones((n, 5))
            emu.emu_bc_mixed(n, dptr(ref), dptr(f * np.ones(n)), scale, shift, dptr(x), dptr(delta), dptr(a))
            emu.emu_bc_scalar(n, code, dptr(scale * (ref - shift)), dptr(x), dptr(delta), dptr(phib), dptr(b))
            assert np.array_equal(a, b), (scale, f)
        f = 0.1 + 0.8 * rng.random(n)
        a = np.zeros((n, 5))
        emu.emu_bc_mixed(n, dptr(ref), dptr(f), scale, shift, dptr(x), dptr(delta), dptr(a))
        r = np.stack(TC.mixed_face(scale * (ref - shift), f, x, delta), axis=1)
        assert np.abs(a - r).max() <= 4 * np.finfo(float).eps * np.abs(r).max()
        assert np.abs(a[:, 0] - scale * (f * ref + (1 - f) * xc - shift)).max() <= 1e-13 * np.abs(a[:, 0]).max()


def test_mixed_on_another_field_is_rejected_by_name():
    from dafoam_amd.meshgen import BC_MIXED

    case = build_case("simpleT")
    for field in ("U", "p", "nuTilda"):
        c = copy.copy(case)
        c.bcs = copy.deepcopy(case.bcs)
        c.bcs["bottom"][field] = (BC_MIXED, (0.0, 0.0, 0.0) if field == "U" else 0.0)
        with pytest.raises(_capi.DASError, match=f"patch bottom: the mixed patch field is built for T only, not for {field}"):
            CaseStruct(c)


def test_restated_T_row_is_the_oracle_row():
    """simple_T_rows (the T rows with face-by-face boundary values, which the products of the thermalCoupling input are checked against) is
    the oracle's T residual when the face values are the patch table's, and follows a changed table."""
    from oracle.residual import residual

    case = build_case("simpleT")
    g = Geometry(case.mesh)
    N = g.nC
    R0 = residual(case, g, case.states)[4 * N : 5 * N]
    for c, values in ((case, None), (TC.as_fixed_value(case, ["top"], [310.0]), {"top": 310.0})):
        R = residual(c, g, case.states)[4 * N : 5 * N]
        r = TC.simple_T_rows(TC.as_fixed_value(case, ["top"]) if values else case, g, case.states, values)
        assert np.abs(r.imag).max() == 0.0 and np.abs(r.real - R).max() <= 1e-12 * np.abs(R).max()
    assert np.abs(R - R0).max() > 1e-3 * np.abs(R0).max()


def body(emu, case, faces, mode, dirs):
    cs = CaseStruct(case)
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    out, fdot, whf = np.zeros(2 * faces.size), np.zeros(faces.size), np.zeros(faces.size)
    rc = emu.emu_thermal_coupling(cs.byref(), dptr(case.states), case.states.size, faces.ctypes.data_as(_capi.c_int_p), faces.size,
                                  int(mode == "daCustom"), dptr(np.ascontiguousarray(dirs)), dptr(out), dptr(fdot), dptr(whf))
    assert rc == 0
    return out, fdot, whf


@pytest.mark.parametrize("which", ["simpleT", "rho", "turbo", "mixed"])
@pytest.mark.parametrize("mode", TC.MODES)
def test_body_matches_restatement(emu, which, mode):
    case = hot_wall(build_case(which))
    patches = ["outlet", "inlet", "bottom", "front"]  # fixedValue, inletOutlet, wall-function and symmetry faces
    g = Geometry(case.mesh)
    faces = TC.selected_faces(case, patches)
    nF = faces.size
    dirs = np.random.default_rng(3).standard_normal((nF, 3))
    out, fdot, whf = body(emu, case, faces, mode, dirs)
    ref = TC.output(case, g, case.states, patches, mode)
    assert np.array_equal(out[:nF], ref[:nF])  # T of the owner cells: copied
    err = np.abs(out[nF:] - ref[nF:]).max() / np.abs(ref[nF:]).max()
    print(f"{which} {mode}: kappa / d of the body vs the restatement, max abs err / max = {err:.2e}")
    assert ref[nF:].min() > 0 and err <= 1e-12
    if mode == "daCustom" and which != "mixed":  # the perturbed hexahedra: the two distances differ
        assert np.abs(ref[nF:] / TC.output(case, g, case.states, patches, "default")[nF:] - 1.0).max() > 1e-6
    # the functional the derivative passes see is d[0] T_c + d[1] kappa / d
    dot = dirs[:, 0] * out[:nF] + dirs[:, 1] * out[nF:]
    assert np.abs(fdot - dot).max() <= 4 * np.finfo(float).eps * (np.abs(dirs[:, 0] * out[:nF]) + np.abs(dirs[:, 1] * out[nF:])).max()
    # and on the fixedValue wall kappa / d (T_b - T_c) is the wallHeatFlux summand of the device body
    t = FM.thermal_boundary(case, g, case.states)
    wall = np.isin(faces, TC.selected_faces(case, ["bottom"]))
    dT = (t["xb"] - t["xc"])[faces - g.nIF] / (case.thermo["Cp"] if FM.is_compressible(case) else 1.0)
    q = out[nF:] * dT
    assert np.abs(whf[wall]).max() > 0 and np.abs(q[wall] - whf[wall]).max() <= 1e-12 * np.abs(whf[wall]).max()


# ---- the host side of the library: definition, size and the errors that need no device --------------------------------------------------
def entry(patches):
    return {"type": OUT, "patches": list(patches), "components": ["thermalCoupling"]}  # reference dafoam/mphys/mphys_dafoam.py:888


def test_library_size_and_definition_errors():
    from common import options
    from dafoam_amd.meshgen import scalar_transport_case
    from dafoam_amd.pyDASolvers import pyDASolvers

    for which, patches in (("simpleT", ["inlet", "bottom"]), ("rho", ["inlet", "bottom"]), ("mixed", ["top", "inlet", "bottom"])):
        case = build_case(which)
        name = (case.solver_name + " -python").encode()
        S = pyDASolvers(name, options(case, outputInfo={"q": entry(patches)}, wallDistanceMethod="daCustom"), case=case)
        assert S.getOutputSize("q", OUT) == TC.size(case, patches)
        assert S.getOutputDistributed("q", OUT) == 1
        with pytest.raises(_capi.DASError, match="thermalCouplingOutput not defined: g"):
            S.getOutputSize("g", OUT)
        with pytest.raises(_capi.DASError, match="patch wing is not in the mesh"):
            pyDASolvers(name, options(case, outputInfo={"q": entry(["bottom", "wing"])}), case=case)
        with pytest.raises(_capi.DASError, match="needs patches"):
            pyDASolvers(name, options(case, outputInfo={"q": entry([])}), case=case)
        with pytest.raises(_capi.DASError, match="wallDistanceMethod: meshWave not supported! Options are: default and daCustom."):
            pyDASolvers(name, options(case, outputInfo={"q": entry(patches)}, wallDistanceMethod="meshWave"), case=case)
        with pytest.raises(_capi.DASError, match="discipline aero only"):
            pyDASolvers(name, options(case, outputInfo={"q": entry(patches)}, discipline="thermal"), case=case)
    for case in (channel_case(4, 4, 3), scalar_transport_case(4, 4, 3)):
        with pytest.raises(NotImplementedError, match="thermalCouplingOutput and the thermalCoupling input. is not built for solvers without a T field"):
            pyDASolvers((case.solver_name + " -python").encode(), options(case, outputInfo={"q": entry(["inlet"])}), case=case)

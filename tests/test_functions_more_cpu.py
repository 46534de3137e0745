"""totalPressureRatio, wallHeatFlux and location without a GPU: the numpy restatement (tests/function_restatement_more.py) against closed
forms, and the kernel body body_facefn (csrc/das_kernels.hpp) run on the host (tests/hostemu/hostemu_functions.cpp) against the restatement."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import function_restatement_more as FM
from common import norm_states
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import BC_FIXED_VALUE, channel_case, rho_channel_case, simple_T_channel_case
from oracle import functions as Fn
from oracle import jacobian as J
from oracle.foam_mesh import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TPR = {"type": "totalPressureRatio", "source": "patchToFace", "patches": ["inlet", "outlet"], "inletPatches": ["inlet"], "outletPatches": ["outlet"],
       "scale": 1.0}  # reference tests/runUnitTests_DAFunction.py:352-359, verbatim
WALLS = ["bottom", "top"]


# ---- the restatement against closed forms -------------------------------------------------------------------------------------
def test_total_pressure_ratio_of_a_uniform_flow_is_one():
    case = rho_channel_case(6, 5, 4, perturb=0.0)
    g = Geometry(case.mesh)
    N = g.nC
    W = case.states.copy()
    W[: 3 * N] = np.tile(case.bcs["inlet"]["U"][1], N)
    W[3 * N : 4 * N] = case.bcs["outlet"]["p"][1]
    W[4 * N : 5 * N] = case.bcs["inlet"]["T"][1]
    assert np.all(W[6 * N + g.nIF :][g.patch_slices()["outlet"]] > 0)  # outflow: the inletOutlet T is zero-gradient
    F = FM.total_pressure_ratio(case, g, W, TPR)
    assert abs(F - 1.0) <= 4 * np.finfo(float).eps  # the two area averages of one constant
    assert FM.total_pressure_ratio(case, g, W, dict(TPR, calcRefVar=1, ref=[0.5])) == (F - 0.5) ** 2
    assert abs(FM.total_pressure_ratio(case, g, case.states, TPR) - 1.0) > 1e-6  # the synthetic state is not uniform
    with pytest.raises(ValueError, match="inlet/outletPatches names are not in patches"):
        FM.total_pressure_ratio(case, g, W, dict(TPR, patches=["inlet", "outlet", "top"]))


@pytest.mark.parametrize("by_unit_area", [True, False])
def test_wall_heat_flux_of_a_linear_profile(by_unit_area):
    """T = Tw + G y over an orthogonal channel: the flux through the bottom wall is Cp alphaEff (Tw - T_c) / dy = -Cp (nu / Pr) G on every
    face (low-Re wall: nut_b = 0), whichever distance method."""
    case = simple_T_channel_case(6, 5, 4, bump=0.0, skew=0.0, perturb=0.0)
    # the generator still stretches z with x and y: put the points back on the lattice, so that the mesh is orthogonal
    case.mesh.points[:, 2] = np.repeat(np.linspace(0.0, 0.1, 4 + 1), (6 + 1) * (5 + 1))
    g = Geometry(case.mesh)
    N = g.nC
    Tw, G = case.bcs["bottom"]["T"][1], 150.0
    W = case.states.copy()
    W[4 * N : 5 * N] = Tw + G * g.C[:, 1]
    fd = {"type": "wallHeatFlux", "source": "patchToFace", "patches": ["bottom"], "scale": 2.0, "byUnitArea": by_unit_area}
    th = case.thermo
    q = -th["Cp"] * (case.nu / th["Pr"]) * G
    A = g.bMagSf[g.patch_slices()["bottom"]].sum()
    exact = 2.0 * q * (1.0 if by_unit_area else A)
    Fd, Fc = FM.wall_heat_flux(case, g, W, fd, "default"), FM.wall_heat_flux(case, g, W, fd, "daCustom")
    assert abs(Fd - exact) <= 1e-12 * abs(exact) and abs(Fc - exact) <= 1e-12 * abs(exact)
    # on a skewed mesh the two distance methods differ
    skewed = simple_T_channel_case(6, 5, 4, perturb=0.02)
    gs = Geometry(skewed.mesh)
    Fd, Fc = FM.wall_heat_flux(skewed, gs, skewed.states, fd, "default"), FM.wall_heat_flux(skewed, gs, skewed.states, fd, "daCustom")
    assert abs(Fd - Fc) > 1e-6 * abs(Fd)
    with pytest.raises(ValueError, match="foo not supported"):
        FM.wall_heat_flux(case, g, W, fd, "foo")
    plain = channel_case(6, 5, 4)
    with pytest.raises(ValueError, match="T field"):
        FM.wall_heat_flux(plain, Geometry(plain.mesh), plain.states, fd)


def test_ks_radius_approaches_the_largest_radius_from_above():
    case = channel_case(6, 5, 4)
    g = Geometry(case.mesh)
    fd = {"type": "location", "source": "patchToFace", "patches": WALLS, "mode": "maxRadiusKS", "axis": [0.0, 0.0, 1.0], "center": [0.5, 0.5, 0.5]}
    r = FM.location_radius(g, case, fd)
    assert r.size == 2 * 6 * 4
    prev = np.inf
    for k in (1.0, 10.0, 100.0, 400.0):
        F = FM.location(case, g, None, dict(fd, coeffKS=k))
        assert r.max() < F <= r.max() + np.log(r.size) / k and F < prev
        prev = F
    assert F - r.max() < 1e-2
    Fi = FM.location(case, g, None, dict(fd, mode="maxInverseRadiusKS", coeffKS=50.0))
    assert 1.0 / (r.min() + 1e-12) < Fi <= 1.0 / (r.min() + 1e-12) + np.log(r.size) / 50.0
    assert FM.location(case, g, None, dict(fd, mode="maxRadius")) == r.max()
    assert FM.location(case, g, None, dict(fd, mode="maxRadius", calcRefVar=1, ref=[0.3])) == (r.max() - 0.3) ** 2
    with pytest.raises(ValueError, match="too large"):
        FM.location(case, g, None, dict(fd, coeffKS=1e3))
    with pytest.raises(ValueError, match="mode: foo"):
        FM.location(case, g, None, dict(fd, mode="foo"))


def test_location_axis_product_is_component_wise():
    """axis = (1, 1, 0) / sqrt 2: the reference's diag(c) . axis is c o axis, not the projection (c . axis) axis."""
    case = channel_case(6, 5, 4)
    g = Geometry(case.mesh)
    fd = {"type": "location", "patches": WALLS, "mode": "maxRadius", "axis": [1.0, 1.0, 0.0], "center": [0.1, 0.05, 0.0]}
    c = g.Cf[g.nIF :][Fn._select(g, case, WALLS)] - np.array(fd["center"])
    a = 1.0 / np.sqrt(2.0)
    written = np.sqrt((c[:, 0] * (1 - a)) ** 2 + (c[:, 1] * (1 - a)) ** 2 + c[:, 2] ** 2)
    r = FM.location_radius(g, case, fd)
    assert np.abs(r - written).max() <= 1e-15 * written.max()
    proj = FM.location_radius(g, case, fd, projection=True)
    assert np.abs(proj - np.linalg.norm(np.cross(c, [a, a, 0.0]), axis=1)).max() <= 1e-14
    assert np.abs(r - proj).max() > 1e-2 * proj.max()
    assert abs(FM.location(case, g, None, fd) - written.max()) <= 1e-15 * written.max()


# ---- the kernel body on the host ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_functions.cpp through g++ with the flags build() gives hostemu.cpp (plus where the HIP headers are: the kernel
    headers include them for their __host__ __device__ qualifiers)."""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    so = str(tmp_path_factory.mktemp("hostemu") / "libhostemu_functions.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-o", so, os.path.join(ROOT, "tests", "hostemu", "hostemu_functions.cpp"), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L = C.CDLL(so)
    L.emu_facefn.argtypes = [C.POINTER(das_case_t), _capi.c_double_p, C.c_longlong, _capi.c_double_p, C.c_int, C.c_double, C.c_int, C.c_double,
                             _capi.c_double_p, _capi.c_int_p, C.c_int, _capi.c_double_p, _capi.c_double_p]
    return L


KIND_TPR, KIND_HFX, KIND_LOC, CUSTOM = 6, 7, 8, 16  # csrc/das_kernels.hpp DAS_FN_*; bit 4: daCustom / inverse radius


def body(emu, case, faces, kind, W, dW=None, bc=None, loc=None):
    """(values, tangents) of body_facefn on the faces; bc = (patch index, dT): a tangent of that patch's T value instead of a state direction."""
    cs = CaseStruct(case)
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    qv, qd = np.zeros(faces.size), np.zeros(faces.size)
    loc = np.ascontiguousarray(loc, dtype=np.float64) if loc is not None else None
    rc = emu.emu_facefn(cs.byref(), dptr(W), W.size, dptr(np.ascontiguousarray(dW)) if dW is not None else None, bc[0] if bc else -1,
                        bc[1] if bc else 0.0, kind, float(case.thermo.get("gamma", 1.4)), dptr(loc) if loc is not None else None,
                        faces.ctypes.data_as(_capi.c_int_p), faces.size, dptr(qv), dptr(qd))
    assert rc == 0
    return qv, qd


def faces_of(g, case, patches):
    return g.nIF + np.nonzero(Fn._select(g, case, patches))[0]


def hot_bottom(case):
    case.bcs["bottom"]["T"] = (BC_FIXED_VALUE, 320.0)
    return case


def check_function(emu, case, g, kind, fd, restated, weights, group=None):
    """F = sum w_f q_f (or the quotient of the two group sums) from the body's values, and its derivative along a random state direction
    from the body's tangents, against the restatement and its complex step."""
    W = case.states
    faces = faces_of(g, case, fd["patches"])
    v = np.random.default_rng(2).standard_normal(W.size) * J.state_scales(case, g, norm_states(case))
    q, dq = body(emu, case, faces, kind, W, v)
    if group is None:
        F, dF = (weights * q).sum(), (weights * dq).sum()
    else:
        S = [(weights * q)[group == k].sum() for k in (0, 1)]
        dS = [(weights * dq)[group == k].sum() for k in (0, 1)]
        F, dF = S[1] / S[0], dS[1] / S[0] - S[1] * dS[0] / S[0] ** 2
    Fo = restated(W)
    dFo = restated(W + 1j * 1e-30 * v).imag / 1e-30
    assert Fo != 0.0 and abs(F - Fo) <= 1e-12 * abs(Fo), (F, Fo)
    assert dFo != 0.0 and abs(dF - dFo) <= 1e-10 * abs(dFo), (dF, dFo)


def test_body_total_pressure_ratio_matches_restatement(emu):
    case = rho_channel_case(6, 5, 4, perturb=0.02)
    g = Geometry(case.mesh)
    sel = Fn._select(g, case, TPR["patches"])
    idx, so = np.nonzero(sel)[0], g.patch_slices()["outlet"]
    group = ((idx >= so.start) & (idx < so.stop)).astype(int)  # 0 inlet, 1 outlet
    assert set(group) == {0, 1}
    a = g.bMagSf[sel]
    w = a / np.where(group == 1, a[group == 1].sum(), a[group == 0].sum())
    check_function(emu, case, g, KIND_TPR, TPR, lambda W: FM.total_pressure_ratio(case, g, W, TPR), w, group)


@pytest.mark.parametrize("method", ["default", "daCustom"])
@pytest.mark.parametrize("which", ["simpleT", "rho"])
def test_body_wall_heat_flux_matches_restatement(emu, which, method):
    if which == "simpleT":
        case = simple_T_channel_case(6, 5, 4, wall_function=True, perturb=0.02)
    else:
        case = hot_bottom(rho_channel_case(6, 5, 4, wall_function=True, perturb=0.02))
    g = Geometry(case.mesh)
    fd = {"type": "wallHeatFlux", "source": "patchToFace", "patches": ["bottom"], "scale": 1.0}  # reference runUnitTests_DAFunction.py:66-71 on our wall
    kind = KIND_HFX | (CUSTOM if method == "daCustom" else 0)
    a = g.bMagSf[Fn._select(g, case, fd["patches"])]
    check_function(emu, case, g, kind, fd, lambda W: FM.wall_heat_flux(case, g, W, fd, method), a / a.sum())
    # the derivative in the wall's T value (a patchVar input), through the seeded boundary table
    W = case.states
    faces = faces_of(g, case, ["bottom"])
    pid = [p.name for p in case.mesh.patches].index("bottom")
    _, dq = body(emu, case, faces, kind, W, bc=(pid, 1.0))
    Tw = case.bcs["bottom"]["T"][1]
    dFo = FM.wall_heat_flux(case, g, W, fd, method, T_values={"bottom": Tw + 1j * 1e-30}).imag / 1e-30
    assert dFo != 0.0 and abs((a / a.sum() * dq).sum() - dFo) <= 1e-10 * abs(dFo)


def test_body_location_matches_restatement(emu):
    case = simple_T_channel_case(6, 5, 4, wall_function=True, perturb=0.02)
    g = Geometry(case.mesh)
    fd = {"type": "location", "patches": WALLS, "mode": "maxRadiusKS", "axis": [1.0, 1.0, 0.0], "center": [0.5, 0.5, 0.5]}
    loc = np.array([1.0 / np.sqrt(2.0), 1.0 / np.sqrt(2.0), 0.0] + fd["center"])
    faces = faces_of(g, case, WALLS)
    v = np.random.default_rng(2).standard_normal(case.states.size)
    r = FM.location_radius(g, case, fd)
    q, dq = body(emu, case, faces, KIND_LOC, case.states, v, loc=loc)
    assert np.abs(q - r).max() <= 1e-12 * r.max() and not dq.any()  # no state is read
    q, _ = body(emu, case, faces, KIND_LOC | CUSTOM, case.states, loc=loc)
    assert np.abs(q - 1.0 / (r + 1e-12)).max() <= 1e-12 * (1.0 / r).max()

"""forceCouplingOutput without a GPU: the numpy restatement (tests/force_coupling_restatement.py) against the force objective and its own
rules, and the vector form of the force body (body_force_vec, csrc/das_kernels.hpp) run on the host
(tests/hostemu/hostemu_forcecoupling.cpp) against the restatement."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import force_coupling_restatement as FC
from dafoam_amd import _capi
from dafoam_amd._capi import CaseStruct, das_case_t, dptr
from dafoam_amd.meshgen import channel_case, rho_channel_case
from mixed_mesh import mixed
from oracle import functions as Fn
from oracle.foam_mesh import Geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREF = 7.5


@pytest.fixture(scope="module")
def channel():
    case = channel_case(6, 5, 4, wall_function=True, perturb=0.02)
    return case, Geometry(case.mesh)


# ---- the restatement against the force objective and its own rules ---------------------------------------------------------------
@pytest.mark.parametrize("patches", [["bottom", "top"], ["bottom", "inlet"], ["outlet"]])
def test_nodal_forces_add_up_to_the_force_objective(channel, patches):
    """Handing F_f / nPoints_f to each of the nPoints_f points of a face loses nothing: per component, the nodal forces add up to
    oracle.functions.force along that axis minus pRef times the summed face vectors, to 1e-12 relative."""
    case, g = channel
    W = case.states
    f = FC.nodal_forces(case, g, W, patches, PREF).reshape(-1, 3)
    sel = Fn._select(g, case, patches)
    for d in range(3):
        expected = Fn.force(case, g, W, patches, np.eye(3)[d]) - PREF * g.bSf[sel][:, d].sum()
        print(f"{patches} component {d}: nodal sum {f[:, d].sum()!r} objective + shift {expected!r}")
        assert expected != 0.0 and abs(f[:, d].sum() - expected) <= 1e-12 * abs(expected)


def test_size_rule(channel):
    case, g = channel
    # 6 x 5 x 4 cells: a wall has 7 x 5 points, the inlet 6 x 5; the edge that bottom and inlet share has 5 points, counted on both
    assert FC.size(case, ["bottom"]) == 3 * 7 * 5
    assert FC.size(case, ["inlet"]) == 3 * 6 * 5
    assert FC.size(case, ["bottom", "top"]) == 3 * 2 * 7 * 5
    assert FC.size(case, ["bottom", "inlet"]) == 3 * (7 * 5 + 6 * 5)
    assert FC.nodal_forces(case, g, case.states, ["bottom", "inlet"], PREF).size == FC.size(case, ["bottom", "inlet"])


def test_patch_order_does_not_matter(channel):
    case, g = channel
    a = FC.nodal_forces(case, g, case.states, ["top", "bottom"], PREF)
    b = FC.nodal_forces(case, g, case.states, ["bottom", "top"], PREF)
    assert np.array_equal(a, b)
    # and the sorted order is the one used: the first half is the bottom wall's
    assert np.array_equal(a[: a.size // 2], FC.nodal_forces(case, g, case.states, ["bottom"], PREF))


def test_shared_points_appear_once_per_patch(channel):
    case, g = channel
    (n0, p0), (n1, p1) = FC.output_points(case, ["inlet", "bottom"])
    assert (n0, n1) == ("bottom", "inlet")
    assert np.all(np.diff(p0) > 0) and np.all(np.diff(p1) > 0)  # ascending inside a patch
    shared = np.intersect1d(p0, p1)
    assert shared.size == 5
    both = FC.nodal_forces(case, g, case.states, ["bottom", "inlet"], PREF).reshape(-1, 3)
    alone0 = FC.nodal_forces(case, g, case.states, ["bottom"], PREF).reshape(-1, 3)
    alone1 = FC.nodal_forces(case, g, case.states, ["inlet"], PREF).reshape(-1, 3)
    # each copy of a shared point receives its own patch's faces only: the two patches' outputs are simply concatenated
    assert np.array_equal(both, np.concatenate([alone0, alone1]))
    i0, i1 = np.searchsorted(p0, shared), np.searchsorted(p1, shared)
    assert np.abs(alone0[i0] - alone1[i1]).max() > 0


def test_pref_shift(channel):
    case, g = channel
    patches = ["bottom", "top"]
    f0 = FC.nodal_forces(case, g, case.states, patches, 0.0)
    f1 = FC.nodal_forces(case, g, case.states, patches, PREF)
    shift = FC.distribute(case, g, -PREF * g.bSf, patches)
    assert np.abs(shift).max() > 0 and np.abs(f1 - f0 - shift).max() <= 1e-13 * np.abs(f0).max()


# ---- the kernel body on the host ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_forcecoupling.cpp through g++ with the flags build() gives hostemu.cpp (plus where the HIP headers are: the
    kernel headers include them for their __host__ __device__ qualifiers)."""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    so = str(tmp_path_factory.mktemp("hostemu") / "libhostemu_forcecoupling.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-o", so, os.path.join(ROOT, "tests", "hostemu", "hostemu_forcecoupling.cpp"),
                           os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L = C.CDLL(so)
    L.emu_face_forces.argtypes = [C.POINTER(das_case_t), _capi.c_double_p, C.c_longlong, _capi.c_int_p, C.c_int, C.c_double, _capi.c_double_p,
                                  _capi.c_double_p, _capi.c_double_p]
    return L


def body(emu, case, faces, pRef, dirs):
    cs = CaseStruct(case)
    faces = np.ascontiguousarray(faces, dtype=np.int32)
    ff, fdot = np.zeros(3 * faces.size), np.zeros(faces.size)
    rc = emu.emu_face_forces(cs.byref(), dptr(case.states), case.states.size, faces.ctypes.data_as(_capi.c_int_p), faces.size, float(pRef),
                             dptr(np.ascontiguousarray(dirs)), dptr(ff), dptr(fdot))
    assert rc == 0
    return ff.reshape(-1, 3), fdot


def mixed_walls():
    """The pyramid / prism / polyhedron mesh with side walls; front and back carry triangles next to quadrilaterals."""
    return mixed("simple", side_walls=True), ["back", "bottom", "front"]


@pytest.mark.parametrize("which", ["hex", "rho", "mixed"])
def test_body_force_vec_matches_restatement(emu, which):
    if which == "mixed":
        case, patches = mixed_walls()
    else:
        case = (channel_case if which == "hex" else rho_channel_case)(6, 5, 4, wall_function=True, perturb=0.02)
        patches = ["bottom", "inlet", "outlet"]
    g = Geometry(case.mesh)
    faces = FC.selected_faces(case, patches)
    if which == "mixed":
        nv = np.diff(case.mesh.face_ptr)[faces]
        assert set(nv) >= {3, 4}, set(nv)
    dirs = np.random.default_rng(3).standard_normal((faces.size, 3))
    for pRef in (0.0, PREF if which != "rho" else 9.0e4):
        ff, fdot = body(emu, case, faces, pRef, dirs)
        ref = FC.face_forces(case, g, case.states, pRef)[faces - g.nIF]
        err = np.abs(ff - ref).max() / np.abs(ref).max()
        print(f"{which} pRef {pRef}: body_force_vec vs restatement, max abs err / max |F| = {err:.2e}")
        assert np.abs(ref).max() > 0 and err <= 1e-12
        # the scalar form is dir . the same components
        dot = (dirs * ff).sum(1)
        assert np.abs(fdot - dot).max() <= 4 * np.finfo(float).eps * np.abs(dirs * ff).sum(1).max()


# ---- the host side of the library: definition, size and the errors that need no device ------------------------------------------------
def test_library_size_and_definition_errors():
    from common import options
    from dafoam_amd.meshgen import scalar_transport_case
    from dafoam_amd.pyDASolvers import pyDASolvers

    out = "forceCouplingOutput"
    for case, patches in ((channel_case(6, 5, 4), ["inlet", "bottom"]), mixed_walls()):
        entry = {"type": out, "patches": patches, "components": ["forceCoupling"], "pRef": PREF}
        S = pyDASolvers(b"DASimpleFoam -python", options(case, outputInfo={"f": entry}), case=case)
        assert S.getOutputSize("f", out) == FC.size(case, patches)
        assert S.getOutputDistributed("f", out) == 1
        with pytest.raises(_capi.DASError, match="forceCouplingOutput not defined: g"):
            S.getOutputSize("g", out)
        with pytest.raises(_capi.DASError, match="needs pRef"):
            pyDASolvers(b"DASimpleFoam -python", options(case, outputInfo={"f": {k: v for k, v in entry.items() if k != "pRef"}}), case=case)
        with pytest.raises(_capi.DASError, match="patch wing is not in the mesh"):
            pyDASolvers(b"DASimpleFoam -python", options(case, outputInfo={"f": dict(entry, patches=["wing"])}), case=case)
        with pytest.raises(NotImplementedError, match="thermalCouplingOutput"):
            pyDASolvers(b"DASimpleFoam -python", options(case, outputInfo={"q": dict(entry, type="thermalCouplingOutput")}), case=case)
    scalar = scalar_transport_case(4, 4, 3)
    with pytest.raises(_capi.DASError, match="DAScalarTransportFoam has no p"):
        pyDASolvers(b"DAScalarTransportFoam -python", options(scalar, outputInfo={"f": dict(entry, patches=["inlet"])}), case=scalar)

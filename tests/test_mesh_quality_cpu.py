"""meshQualityKS and residualNorm without a GPU: the kernel bodies body_mesh_quality, rn_term and rn_seed (csrc/das_meshquality.hpp) run on the
host (tests/hostemu/hostemu_mesh_quality.cpp) against the numpy restatement (tests/mesh_quality_restatement.py).  Tolerances: values 1e-12,
tangents 1e-10 (DESIGN row f1c)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_quality_restatement as MQ
from common import blocks
from dafoam_amd import _capi
from dafoam_amd._capi import dptr
from dafoam_amd.meshgen import channel_case, rho_channel_case
from mixed_mesh import MIXED
from oracle.foam_mesh import Geometry
from oracle.residual import residual

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRIC_ID = {"faceOrthogonality": 0, "nonOrthoAngle": 1, "faceSkewness": 2}  # csrc/das_meshquality.hpp DAS_MQ_*
MESHES = {"channel": channel_case(6, 5, 4).mesh, "mixed": MIXED.mesh}
ip = _capi.c_int_p


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """tests/hostemu/hostemu_mesh_quality.cpp through g++ with the flags the other host emulations get"""
    rocm = os.environ.get("ROCM_PATH") or os.path.dirname(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")))
    so = str(tmp_path_factory.mktemp("hostemu") / "libhostemu_mesh_quality.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-fPIC", "-shared", "-I" + os.path.join(rocm, "include"), "-D__HIP_PLATFORM_AMD__",
                           "-o", so, os.path.join(ROOT, "tests", "hostemu", "hostemu_mesh_quality.cpp"), os.path.join(ROOT, "dafoam_amd", "csrc", "das_mesh.cpp")])
    L = C.CDLL(so)
    L.emu_mesh_quality.argtypes = [C.c_int, _capi.c_double_p, C.c_int, C.c_int, C.c_int, ip, ip, ip, ip, C.c_int, _capi.c_double_p, _capi.c_double_p,
                                   _capi.c_double_p]
    L.emu_residual_norm.argtypes = [C.c_longlong, _capi.c_double_p, C.c_int, _capi.c_ll_p, ip, _capi.c_double_p, C.c_longlong, C.c_longlong, C.c_longlong,
                                    C.c_int, C.c_double, C.c_double, _capi.c_double_p, _capi.c_double_p]
    return L


def body(emu, mesh, pts, metric, dX=None):
    """(a_f, tangents along dX) of body_mesh_quality over all faces"""
    i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1)
    fptr, fpts, own, nei = i32(mesh.face_ptr), i32(mesh.face_pts), i32(mesh.owner), i32(mesh.neighbour)
    a, da = np.zeros(mesh.n_faces), np.zeros(mesh.n_faces)
    rc = emu.emu_mesh_quality(pts.size // 3, dptr(pts), mesh.n_faces, mesh.n_internal_faces, mesh.n_cells, fptr.ctypes.data_as(ip), fpts.ctypes.data_as(ip),
                              own.ctypes.data_as(ip), nei.ctypes.data_as(ip), METRIC_ID[metric], dptr(np.ascontiguousarray(dX).reshape(-1)) if dX is not None else None,
                              dptr(a), dptr(da))
    assert rc == 0
    return a, da


def points_of(mesh, seed):
    return np.asarray(mesh.points, dtype=np.float64).reshape(-1, 3) if seed is None else MQ.jitter(mesh, seed)


def value_scale(g, metric):
    """The magnitude a per-face value is held against.  faceOrthogonality and faceSkewness: max(|a_f|, 1) - on an orthogonal face the
    skewness is the rounding residue of Cpf - r d, about 1e-17, which has no digit to compare, while its error is eps relative to the
    O(1) quotient |Cpf| / fd.  nonOrthoAngle: acos is ill-conditioned towards the clamp, an error e of the cosine becomes
    e (180 / pi) / sqrt(1 - val^2) degrees; the scale is that amplification, at least max(|a_f|, 1)."""
    a = np.abs(MQ.metric_values(g, metric))
    if metric != "nonOrthoAngle":
        return np.maximum(a, 1.0)
    v = np.clip(MQ.face_orthogonality(g), -MQ.BOUND, MQ.BOUND)
    return np.maximum(np.maximum(a, 1.0), (180.0 / np.pi) / np.sqrt(1.0 - v * v))


@pytest.mark.parametrize("seed", [None, 7, 8])
@pytest.mark.parametrize("metric", MQ.METRICS)
@pytest.mark.parametrize("name", list(MESHES))
def test_body_values_match_the_restatement(emu, name, metric, seed):
    mesh = MESHES[name]
    pts = points_of(mesh, seed)
    g = MQ.MeshGeometry(mesh, pts)
    assert g.V.min() > 0
    ref = MQ.metric_values(g, metric)
    a, _ = body(emu, mesh, pts, metric)
    err = np.abs(a - ref) / value_scale(g, metric)
    print(name, metric, seed, "max scaled error", err.max(), "range", ref.min(), ref.max())
    assert err.max() <= 1e-12
    if metric == "faceOrthogonality":
        assert np.all(a[mesh.n_internal_faces:] == 1.0)  # boundary faces: exactly 1
    if metric == "nonOrthoAngle":
        b = a[mesh.n_internal_faces:]  # boundary faces: the one constant acos(1 - 1e-6) in degrees
        assert np.all(b == b[0]) and abs(b[0] - np.arccos(MQ.BOUND) * 180.0 / np.pi) <= 1e-15


def check_jitter(g):
    """what the tangent comparisons need: no clamped internal face, no tie in the point maximum, no |sv| = 0"""
    _, sv_over_d, gap = MQ.face_skewness(g, details=True)
    assert g.V.real.min() > 0 and not MQ.clamped(g)[: g.nIF].any()
    assert gap.min() >= 1e-6 and sv_over_d.min() >= 1e-5, (gap.min(), sv_over_d.min())


@pytest.mark.parametrize("seed", [7, 8])
@pytest.mark.parametrize("metric", MQ.METRICS)
@pytest.mark.parametrize("name", list(MESHES))
def test_body_tangents_match_the_complex_step(emu, name, metric, seed):
    mesh = MESHES[name]
    pts = points_of(mesh, seed)
    check_jitter(MQ.MeshGeometry(mesh, pts))
    for dseed in (1, 2):
        dX = np.random.default_rng(dseed).standard_normal(pts.shape)
        h = 1e-30
        ref = MQ.metric_values(MQ.MeshGeometry(mesh, pts + 1j * h * dX), metric).imag / h
        _, da = body(emu, mesh, pts, metric, dX)
        err = np.abs(da - ref).max() / np.abs(ref).max()
        print(name, metric, seed, dseed, "tangent error relative to the largest", err)
        assert np.abs(ref).max() > 0 and err <= 1e-10


def test_clamped_and_boundary_faces_have_no_tangent(emu):
    """an orthogonal lattice: every internal face has orthogonality 1 > the bound, so nonOrthoAngle is the clamped constant there as on
    every boundary face, with tangent exactly 0 along any point direction; the orthogonality of a boundary face is the constant 1"""
    mesh = channel_case(4, 3, 3, bump=0.0, skew=0.0, perturb=0.0).mesh
    pts = np.asarray(mesh.points, dtype=np.float64).reshape(-1, 3).copy()
    pts[:, 2] = np.repeat(np.linspace(0.0, 0.1, 3 + 1), (4 + 1) * (3 + 1))  # the generator stretches z with x and y: back onto the lattice
    g = MQ.MeshGeometry(mesh, pts)
    assert g.V.min() > 0 and MQ.clamped(g)[: g.nIF].all()
    dX = np.random.default_rng(3).standard_normal(pts.shape)
    a, da = body(emu, mesh, pts, "nonOrthoAngle", dX)
    assert np.all(a == a[0]) and abs(a[0] - np.arccos(MQ.BOUND) * 180.0 / np.pi) <= 1e-15 and np.all(da == 0.0)
    a, da = body(emu, mesh, pts, "faceOrthogonality", dX)
    assert np.all(a[g.nIF:] == 1.0) and np.all(da[g.nIF:] == 0.0) and da[: g.nIF].any()


@pytest.mark.parametrize("mode", ["L2Norm", "L1Norm"])
@pytest.mark.parametrize("make", [channel_case, rho_channel_case])
def test_residual_norm_terms_and_seeds(emu, make, mode):
    """rn_term / rn_seed over every row against the restatement, the internal-phi quirk of L1Norm included, with calcRefVar's outer factor"""
    case = make(6, 5, 4)
    g = Geometry(case.mesh)
    bl = blocks(case, g)
    Rv = residual(case, g, case.states)
    Rv[5] = 0.0  # sign(0) = 0
    weights = {"URes": 2.0, "pRes": -3.0, "nuTildaRes": 0.5, "phiRes": 1.5, "TRes": 0.25, "kRes": 7.0}  # kRes: an extra key, ignored
    fd = {"type": "residualNorm", "resWeight": weights, "resMode": mode, "calcRefVar": 1, "ref": [0.3]}
    w, iphi = MQ.residual_rows(bl, weights, g.nIF)
    assert iphi.sum() == g.nIF
    F0 = MQ.residual_norm_of(Rv, w, iphi, dict(fd, calcRefVar=0))
    seeds = MQ.residual_norm_seeds(Rv, w, iphi, fd, seed=1.7)
    off = np.array([sl.start for _, sl in bl], dtype=np.int64)
    kind = np.array([0 if nm == "U" else 2 if nm == "phi" else 1 for nm, _ in bl], dtype=np.int32)  # KIND_VEC, KIND_FACE, KIND_SCL
    wb = np.array([weights[nm + "Res"] for nm, _ in bl])
    term, gv = np.zeros(Rv.size), np.zeros(Rv.size)
    coef = 1.7 * 2.0 * (F0 - 0.3)
    assert emu.emu_residual_norm(Rv.size, dptr(Rv), len(bl), off.ctypes.data_as(_capi.c_ll_p), kind.ctypes.data_as(ip), dptr(wb), g.nC, g.nF, g.nIF,
                                 int(mode == "L1Norm"), F0, coef, dptr(term), dptr(gv)) == 0
    tref = np.where(iphi | (mode == "L2Norm"), w * w * Rv * Rv, np.abs(w * Rv))
    assert np.abs(term - tref).max() <= 1e-12 * np.abs(tref).max()
    assert np.abs(gv - seeds).max() <= 1e-12 * np.abs(seeds).max() and gv[5] == 0.0
    if mode == "L1Norm":  # the quirk: an internal face of phiRes keeps the squared term, and its seed is 2 w^2 R
        f = bl[-1][1].start
        assert term[f] == 1.5 * 1.5 * Rv[f] * Rv[f] and abs(gv[f] - coef * 2.0 * 2.25 * Rv[f]) <= 1e-15 * abs(gv[f])
        b = f + g.nIF
        assert abs(term[b] - abs(1.5 * Rv[b])) <= 1e-15 * term[b]
    # the seeds are the derivative of the restated value: complex step along a random residual direction
    v = np.random.default_rng(4).standard_normal(Rv.size) * np.abs(Rv).mean()
    v[Rv == 0.0] = 0.0  # |w R| has a kink at R = 0 (wall rows of phiRes are exact zeros): the seed rule puts 0 there
    dF = MQ.residual_norm_of(Rv + 1e-30j * v, w, iphi, fd).imag / 1e-30
    assert abs(1.7 * dF - seeds @ v) <= 1e-10 * abs(1.7 * dF)
    with pytest.raises(ValueError, match="pRes"):
        MQ.residual_rows(bl, {k: x for k, x in weights.items() if k != "pRes"}, g.nIF)

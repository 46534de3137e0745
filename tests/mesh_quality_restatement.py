"""Plain-numpy restatement of the meshQualityKS and residualNorm functions (reference DAFunctionMeshQualityKS.C, DAFunctionResidualNorm.C),
written from the formulas of OpenFOAM v1812's polyMeshTools::faceOrthogonality / faceSkewness and from the reference's text; it calls none
of the library's bodies.  Everything here works on complex points (complex step: comparisons and arg-max on the real parts), so the
face and cell metrics are restated too instead of taken from oracle.foam_mesh.Geometry, which keeps real arrays.

R = ROOTVSMALL = 1e-150."""
import math

import numpy as np

R = 1e-150
BOUND = 1.0 - 1e-6
METRICS = ("faceOrthogonality", "nonOrthoAngle", "faceSkewness")


def _mag(v):
    return np.sqrt((v * v).sum(-1))  # not abs(): analytic in the components


def _cabs(z):
    return np.where(z.real >= 0, z, -z)


class MeshGeometry:
    """Sf, Cf, C, V of primitiveMesh::makeFaceCentresAndAreas / makeCellCentresAndVols from the points (real or complex)."""

    def __init__(self, mesh, points=None):
        pts = np.asarray(mesh.points if points is None else points).reshape(-1, 3)
        dt = pts.dtype
        self.mesh, self.pts = mesh, pts
        F, N, nIF = mesh.n_faces, mesh.n_cells, mesh.n_internal_faces
        self.nF, self.nC, self.nIF = F, N, nIF
        own, nei = mesh.owner.astype(np.int64), mesh.neighbour.astype(np.int64)
        self.own, self.nei = own, nei
        fp = mesh.face_ptr.astype(np.int64)
        nv = np.diff(fp)
        self.fp, self.nv, self.kmax = fp, nv, int(nv.max())
        fc = np.zeros((F, 3), dt)
        for s in range(self.kmax):
            m = nv > s
            fc[m] += pts[mesh.face_pts[fp[:-1][m] + s]]
        fc /= nv[:, None]
        sumN, sumA, sumAc = np.zeros((F, 3), dt), np.zeros(F, dt), np.zeros((F, 3), dt)
        for s in range(self.kmax):
            m = nv > s
            a = pts[mesh.face_pts[fp[:-1][m] + s]]
            b = pts[mesh.face_pts[fp[:-1][m] + (s + 1) % nv[m]]]
            n = np.cross(b - a, fc[m] - a)
            an = _mag(n)
            sumN[m] += n
            sumA[m] += an
            sumAc[m] += an[:, None] * (a + b + fc[m])
        Cf = sumAc / (3.0 * sumA[:, None])
        Sf = 0.5 * sumN
        tri = nv == 3
        if tri.any():
            i0, i1, i2 = (mesh.face_pts[fp[:-1][tri] + k] for k in range(3))
            Cf[tri] = (pts[i0] + pts[i1] + pts[i2]) / 3.0
            Sf[tri] = 0.5 * np.cross(pts[i1] - pts[i0], pts[i2] - pts[i0])
        self.Sf, self.Cf = Sf, Cf
        cnt = np.bincount(own, minlength=N) + np.bincount(nei, minlength=N)
        cEst = np.zeros((N, 3), dt)
        np.add.at(cEst, own, Cf)
        np.add.at(cEst, nei, Cf[:nIF])
        cEst /= cnt[:, None]
        pvo = (Sf * (Cf - cEst[own])).sum(1)
        pvn = (Sf[:nIF] * (cEst[nei] - Cf[:nIF])).sum(1)
        V3, C = np.zeros(N, dt), np.zeros((N, 3), dt)
        np.add.at(V3, own, pvo)
        np.add.at(V3, nei, pvn)
        np.add.at(C, own, pvo[:, None] * (0.75 * Cf + 0.25 * cEst[own]))
        np.add.at(C, nei, pvn[:, None] * (0.75 * Cf[:nIF] + 0.25 * cEst[nei]))
        self.C, self.V = C / V3[:, None], V3 / 3.0


def face_orthogonality(g):
    """internal: (d . Sf) / (|d| |Sf| + R), d = nei - own; boundary: exactly 1"""
    a = np.ones(g.nF, g.pts.dtype)
    d = g.C[g.nei] - g.C[g.own[: g.nIF]]
    a[: g.nIF] = (d * g.Sf[: g.nIF]).sum(1) / (_mag(d) * _mag(g.Sf[: g.nIF]) + R)
    return a


def clamped(g):
    """faces whose orthogonality the nonOrthoAngle clamp replaces by the bound"""
    return np.abs(face_orthogonality(g).real) > BOUND


def non_ortho_angle(g):
    """DAFunctionMeshQualityKS.C:112-135: val bounded to +-(1 - 1e-6) by assignment (a clamped face is a constant), acos in degrees"""
    v = face_orthogonality(g)
    v = np.where(v.real > BOUND, BOUND, v)
    v = np.where(v.real < -BOUND, -BOUND, v)
    return np.arccos(v) * 180.0 / np.pi


def face_skewness(g, details=False):
    """polyMeshTools::faceSkewness.  details: also |sv| / |d| and the relative gap between the two largest candidates of fd."""
    nIF = g.nIF
    Cpf = g.Cf - g.C[g.own]
    d = np.zeros_like(Cpf)
    d[:nIF] = g.C[g.nei] - g.C[g.own[:nIF]]
    n = g.Sf[nIF:] / (_mag(g.Sf[nIF:]) + R)[:, None]
    d[nIF:] = n * (n * Cpf[nIF:]).sum(1)[:, None]
    sv = Cpf - ((g.Sf * Cpf).sum(1) / ((g.Sf * d).sum(1) + R))[:, None] * d
    magSv = _mag(sv)
    svHat = sv / (magSv + R)[:, None]
    coef = np.where(np.arange(g.nF) < nIF, 0.2, 0.4)
    cand = np.full((g.nF, g.kmax + 1), -np.inf, g.pts.dtype)
    cand[:, 0] = coef * _mag(d) + R  # the floor term first, then the points in their stored order
    for s in range(g.kmax):
        m = g.nv > s
        p = g.pts[g.mesh.face_pts[g.fp[:-1][m] + s]]
        cand[m, s + 1] = _cabs((svHat[m] * (p - g.Cf[m])).sum(1))
    win = np.argmax(cand.real, axis=1)  # the first maximum
    fd = cand[np.arange(g.nF), win]
    a = magSv / fd
    if not details:
        return a
    top = np.sort(cand.real, axis=1)[:, ::-1]
    return a, (magSv / _mag(d)).real, (top[:, 0] - top[:, 1]) / top[:, 0]


def metric_values(g, metric):
    if metric == "faceOrthogonality":
        return face_orthogonality(g)
    if metric == "nonOrthoAngle":
        return non_ortho_angle(g)
    if metric == "faceSkewness":
        return face_skewness(g)
    raise ValueError("metric not valid! Options: faceOrthogonality, nonOrthoAngle, or faceSkewness")


def ks(a, k):
    """log(sum exp(k a)) / k in log space; real input: exactly rounded sum (math.fsum)"""
    x = k * np.asarray(a)
    m = x.real.max()
    e = np.exp(x - m)
    S = math.fsum(e) if not np.iscomplexobj(e) else e.sum()
    return (m + np.log(S)) / k


def _ref_var(fd, F0):
    return (F0 - np.atleast_1d(fd["ref"])[0]) ** 2 if int(fd.get("calcRefVar", 0)) else F0


def mesh_quality_ks(mesh, fd, points=None):
    """F of a meshQualityKS function dict at the points (default: the mesh's own).  scale is read and not applied."""
    return _ref_var(fd, ks(metric_values(MeshGeometry(mesh, points), fd["metric"]), float(fd["coeffKS"])))


def mesh_quality_gradient(mesh, fd, points=None, h=1e-30):
    """dF/dX for all 3 nP coordinates by complex step (small meshes only)"""
    X = np.asarray(mesh.points if points is None else points, dtype=np.float64).reshape(-1)
    out = np.zeros(X.size)
    for j in range(X.size):
        Xc = X.astype(np.complex128)
        Xc[j] += 1j * h
        out[j] = mesh_quality_ks(mesh, fd, Xc).imag / h
    return out


def jitter(mesh, seed, rel=0.1):
    """every point moved by rel h uniform(-1, 1), h the smallest edge of the mesh"""
    pts = np.asarray(mesh.points, dtype=np.float64).reshape(-1, 3)
    fp = mesh.face_ptr.astype(np.int64)
    h = np.inf
    for f in range(mesh.n_faces):
        v = pts[mesh.face_pts[fp[f] : fp[f + 1]]]
        h = min(h, np.linalg.norm(v - np.roll(v, -1, axis=0), axis=1).min())
    return pts + rel * h * np.random.default_rng(seed).uniform(-1.0, 1.0, pts.shape)


# ---- residualNorm ---------------------------------------------------------------------------------------------------------------------
def residual_rows(blocks, res_weight, nIF):
    """per row: the weight of its residual block (<state>Res; a missing one is an error, extra keys are ignored) and whether it is an
    internal face of phiRes.  blocks: ((state, slice), ...) as tests/common.blocks gives them."""
    n = max(sl.stop for _, sl in blocks)
    w, internal_phi = np.zeros(n), np.zeros(n, bool)
    for name, sl in blocks:
        if name + "Res" not in res_weight:
            raise ValueError(f"resWeight has no entry for {name}Res")
        w[sl] = float(res_weight[name + "Res"])
        if name == "phi":
            internal_phi[sl.start : sl.start + nIF] = True
    return w, internal_phi


def residual_norm_of(Rv, w, internal_phi, fd):
    """F from the residual vector.  L1Norm: the internal faces of phiRes still add w^2 R^2 (DAFunctionResidualNorm.C:146-149)."""
    mode = fd.get("resMode", "L2Norm")
    if mode == "L2Norm":
        F0 = np.sqrt((w * w * Rv * Rv).sum())
    elif mode == "L1Norm":
        t = np.where(internal_phi, w * w * Rv * Rv, _cabs(w * Rv))
        F0 = math.fsum(t) if not np.iscomplexobj(t) else t.sum()
    else:
        raise ValueError("resMode not supported")
    return _ref_var(fd, F0)


def residual_norm_seeds(Rv, w, internal_phi, fd, seed=1.0):
    """g = seed dF/dR: L2 w^2 R / F0; L1 |w| sign(R) (0 at R = 0), internal phi rows 2 w^2 R; times 2 (F0 - ref) under calcRefVar"""
    plain = dict(fd, calcRefVar=0)
    F0 = residual_norm_of(Rv, w, internal_phi, plain)
    outer = 2.0 * (F0 - np.atleast_1d(fd["ref"])[0]) if int(fd.get("calcRefVar", 0)) else 1.0
    if fd.get("resMode", "L2Norm") == "L2Norm":
        if F0 == 0.0:
            raise ValueError("the L2Norm is zero")
        g = w * w * Rv / F0
    else:
        g = np.where(internal_phi, 2.0 * w * w * Rv, np.abs(w) * np.sign(Rv))
    return seed * outer * g


def residual_norm(case, g, W, fd, blocks):
    from oracle.residual import residual

    w, ip = residual_rows(blocks, fd["resWeight"], g.nIF)
    return residual_norm_of(residual(case, g, W), w, ip, fd)

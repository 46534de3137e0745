"""numpy restatement of the reference's actuator disks, written from DAFvSourceActuatorDisk.C (:93-429 calcFvSource, :431-482 the 13
actuatorDiskPars, :484-560 the cell sets), OpenFOAM's cylinderAnnulusToCell and DAResidualSimpleFoam.C:141-147 - not from the kernel bodies:
  fvSource[c] = sum over the entries, in the order of their names, of f(c) = fAxial n + fCirc t           [force per unit volume]
  c = C - center, n = direction / |direction|; the axial part is the tensor diag(c) & n = c o n (component by component - NOT the
  projection n (c . n)), the radial part r = c - c o n; t = r x n (rotDir left) or n x r (right), normalised
  rPrime = |r| / outerRadius, hub = innerRadius / outerRadius, rStar = (rPrime - hub) / (1 - hub)
  cylinderAnnulusToCell   on a cell set chosen once (0 < d.a < a.a, innerRadius^2 < |d|^2 - (d.a)^2 / a.a < outerRadius^2; a = p2 - p1,
                          d = C - p1), center = (p1 + p2) / 2, direction = p2 - p1:
                          fAxial = rStar sqrt(1 - rStar) scale, fCirc = fAxial POD / pi / rPrime
  cylinderAnnulusSmooth   on every cell, epsR = eps / (outerRadius - innerRadius):
                          fR = rStar^expM (1 - rStar)^expN for epsR <= rStar <= 1 - epsR, else its value at the nearer end times
                          exp(-((rStar - end) / epsR)^2);  fAxial = scale fR exp(-|c o n|^2 / eps^2),
                          fCirc = fAxial POD / pi / (rPrime + 0.01 eps / outerRadius);
                          adjustThrust: scale = targetThrust / sum fAxial(scale = 1) V, pars[8] is not read
  UEqn = div(phi, U) + ... - fvSource: the matrix source gains V fvSource before relax(), so URes and H both carry it.
The residual is the oracle's simple_residual with that one term (simple_residual_with_source: a copy of oracle/residual.py:268-523, which
has no hook for a source; with a zero field it gives the oracle's bits).  Everything takes complex parameters and a FlowGeom at complex
points; the switches select on the real part."""
import numpy as np

import heat_transfer_restatement as H
from actuator_disk_residual import simple_residual_with_source

PAR_NAMES = ("center_x", "center_y", "center_z", "direction_x", "direction_y", "direction_z", "innerRadius", "outerRadius", "scale", "POD", "expM", "expN",
             "targetThrust")


class FlowGeom(H.Geom):
    """H.Geom (complex-safe metrics) with the boundary views the oracle's flow residual reads"""

    def __init__(self, mesh, points=None):
        super().__init__(mesh, points)
        self.nBF = self.nF - self.nIF
        self.bSf, self.bnf = self.Sf[self.nIF:], self.nf[self.nIF:]


def annulus_cells(g, p1, p2, innerRadius, outerRadius):
    """OpenFOAM cylinderAnnulusToCell on the cell centres of g (real parts: the set is a choice, not a function)"""
    p1, p2 = np.asarray(p1, float), np.asarray(p2, float)
    a = p2 - p1
    d = np.real(g.C) - p1
    m = d @ a
    aa = a @ a
    d2 = (d * d).sum(1) - m * m / aa
    return np.nonzero((m > 0) & (m < aa) & (d2 < outerRadius**2) & (d2 > innerRadius**2))[0]


def disk_force(C, pars, eps, rotDir, smooth, scale=None, projection=False):
    """(f (n, 3), fAxial, fCirc, rStar, |r|) at the cell centres C.  pars: the 13 parameters; scale overrides pars[8].  projection: the OTHER
    reading of the axial part, n (c . n) - what the reference does not do."""
    pars = np.asarray(pars)
    center, direction, inner, outer, POD, expM, expN = pars[0:3], pars[3:6], pars[6], pars[7], pars[9], pars[10], pars[11]
    scale = pars[8] if scale is None else scale
    n = direction / np.sqrt((direction * direction).sum())
    c = C - center
    ca = n * (c @ n)[:, None] if projection else c * n
    r = c - ca
    t = np.cross(r, n) if rotDir == "left" else np.cross(n, r)
    assert rotDir in ("left", "right"), "rotDir not valid"
    rLen, tLen = np.sqrt((r * r).sum(1)), np.sqrt((t * t).sum(1))
    rPrime, hub = rLen / outer, inner / outer
    rStar = (rPrime - hub) / (1.0 - hub)
    if not smooth:
        fAxial = rStar * np.sqrt(1.0 - rStar) * scale
        fCirc = fAxial * POD / np.pi / rPrime
    else:
        epsR = eps / (outer - inner)
        lo, hi = epsR, 1.0 - epsR
        x = np.real(rStar)
        mid = (x >= np.real(lo)) & (x <= np.real(hi))
        rs = np.where(mid, rStar, 0.5)  # pow is evaluated in the middle branch only, where 0 < rStar < 1
        fR = np.where(mid, rs**expM * (1.0 - rs) ** expN,
                      np.where(x < np.real(lo), lo**expM * (1.0 - lo) ** expN * np.exp(-((rStar - lo) ** 2) / epsR / epsR),
                               hi**expM * (1.0 - hi) ** expN * np.exp(-((rStar - hi) ** 2) / epsR / epsR)))
        fAxial = fR * scale * np.exp(-(ca * ca).sum(1) / eps / eps)
        fCirc = fAxial * POD / np.pi / (rPrime + 0.01 * eps / outer)
    f = fAxial[:, None] * n + fCirc[:, None] * (t / tLen[:, None])
    return f, fAxial, fCirc, rStar, rLen


class Disks:
    """The fvSource option at its definition: the cell sets are chosen from the geometry of that moment and kept."""

    def __init__(self, g0, fvSource):
        self.entries = {}
        for name in sorted(fvSource):
            e = dict(fvSource[name])
            if e["source"] == "cylinderAnnulusToCell":
                e["cells"] = annulus_cells(g0, e["p1"], e["p2"], e["innerRadius"], e["outerRadius"])
                assert e["cells"].size, name
                p1, p2 = np.array(e["p1"], float), np.array(e["p2"], float)
                e["pars"] = np.array(list((p1 + p2) / 2) + list(p2 - p1) + [e["innerRadius"], e["outerRadius"], e["scale"], e["POD"], 0, 0, 0], dtype=np.complex128)
                e["smooth"], e["eps"], e["adjustThrust"] = False, 0.0, 0
            else:
                assert e["source"] == "cylinderAnnulusSmooth", e["source"]
                e["pars"] = np.array(list(e["center"]) + list(e["direction"]) + [e.get(k, 0.0) for k in PAR_NAMES[6:]], dtype=np.complex128)
                e["smooth"], e["adjustThrust"] = True, int(e.get("adjustThrust", 0))
            self.entries[name] = e

    def unit_thrust(self, g, name, pars=None):
        """sum fAxial(scale = 1) V of a smooth disk: what adjustThrust divides targetThrust by"""
        e = self.entries[name]
        p = e["pars"] if pars is None else np.asarray(pars)
        return (disk_force(g.C, p, e["eps"], e["rotDir"], True, scale=1.0)[1] * g.V).sum()

    def scale(self, g, name, pars=None):
        e = self.entries[name]
        p = e["pars"] if pars is None else np.asarray(pars)
        return p[12] / self.unit_thrust(g, name, p) if e["adjustThrust"] else p[8]

    def entry(self, g, name, pars=None, frozen=None):
        """(f, thrustSourceSum, torqueSourceSum) of one entry at the metrics g; frozen: another geometry whose adjustThrust total is used
        instead of g's (what a pass that lets a point reach its own rows only can see)"""
        e = self.entries[name]
        p = e["pars"] if pars is None else np.asarray(pars)
        sc = self.scale(g if frozen is None else frozen, name, p)
        if e["smooth"]:
            f, fa, fc, _, _ = disk_force(g.C, p, e["eps"], e["rotDir"], True, scale=sc)
        else:
            cells = e["cells"]
            fs, fas, fcs, _, _ = disk_force(g.C[cells], p, 0.0, e["rotDir"], False, scale=sc)
            f, fa, fc = np.zeros((g.nC, 3), fs.dtype), np.zeros(g.nC, fs.dtype), np.zeros(g.nC, fs.dtype)
            f[cells], fa[cells], fc[cells] = fs, fas, fcs
        return f, (fa * g.V).sum(), (fc * g.V).sum()

    def field(self, g, pars=None, frozen=None):
        """fvSource (n, 3); pars: {name: parameters} replacing those of the entries named"""
        q = 0.0
        for name in self.entries:
            q = q + self.entry(g, name, (pars or {}).get(name), frozen)[0]
        return q


def residual(case, g, W, disks=None, normalize=("URes", "pRes", "TRes", "nuTildaRes", "phiRes"), pars=None, frozen=None, **kw):
    """R(W) of DASimpleFoam with the disks' source (disks None: without the term)"""
    q = None if disks is None else disks.field(g, pars, frozen)
    return simple_residual_with_source(case, g, W, fvSource=q, normalize=normalize, **kw)

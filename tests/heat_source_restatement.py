"""numpy restatement of the reference's heat sources, written from DAFvSourceHeatSource.C (:30-128 the definitions, :236-321 calcFvSource),
DAFvSource.C:128-154 (findGlobalSnappedCenter) and OpenFOAM's cylinderToCell / primitiveMesh::pointInCell - not from the kernel bodies:
  fvSource[c] = sum over the entries, in the order of their names, of q(c) [W/m^3]
  cylinderToCell   q = power / totalV on a cell set chosen once (0 < d.a < a.a, |d|^2 - (d.a)^2 / a.a < radius^2; a = p2 - p1, d = C - p1),
                   totalV the volume of the set at the current metrics
  cylinderSmooth   q = power s / sum s V;  c = C - center, n = axis / |axis|, the axial part is the tensor diag(c) & n = c o n (component
                   by component - NOT the projection n (c . n)), the radial part c - c o n;  s = sA sR, each 1 inside and
                   exp(-(overshoot / eps)^2) outside.  snapCenter2Cell: center = C of the cell that contained it at definition.
  TRes = laplacian(kappa, T) + fvSource per unit volume (DAResidualHeatTransferFoam.C:97-102), times V when TRes is not normalised.
Everything takes complex parameters and a Geom at complex points; the two switches select on the real part."""
import numpy as np

import heat_transfer_restatement as H

PAR_NAMES = ("center_x", "center_y", "center_z", "axis_x", "axis_y", "axis_z", "radius", "length", "power")


def cylinder_cells(g, p1, p2, radius):
    """OpenFOAM cylinderToCell on the cell centres of g (real parts: the set is a choice, not a function)"""
    p1, p2 = np.asarray(p1, float), np.asarray(p2, float)
    a = p2 - p1
    d = np.real(g.C) - p1
    m = d @ a
    aa = a @ a
    return np.nonzero((m > 0) & (m < aa) & ((d * d).sum(1) - m * m / aa < radius**2))[0]


def containing_cells(g, p):
    """primitiveMesh::pointInCell for every cell: p on the inner side of (or on) every face plane of the cell"""
    dots = ((np.asarray(p, float) - np.real(g.Cf)) * np.real(g.Sf)).sum(1)
    ok = np.ones(g.nC, bool)
    np.logical_and.at(ok, g.own, dots <= 0)
    np.logical_and.at(ok, g.nei, -dots[: g.nIF] <= 0)
    return np.nonzero(ok)[0]


def smooth_shape(g, pars, eps, center=None, projection=False):
    """s of cylinderSmooth; center overrides pars[0:3] (a snapped centre).  projection: the OTHER reading, n (c . n) - what the reference
    does not do; the tests use it to show that they tell the two apart."""
    pars = np.asarray(pars)
    ctr = pars[0:3] if center is None else np.asarray(center)
    axis, radius, length = pars[3:6], pars[6], pars[7]
    n = axis / np.sqrt((axis * axis).sum())
    c = g.C - ctr
    ca = n * (c @ n)[:, None] if projection else c * n
    cr = c - ca
    A, R = np.sqrt((ca * ca).sum(1)), np.sqrt((cr * cr).sum(1))
    dA, dR = A - length / 2.0, R - radius
    sA = np.where(np.real(dA) > 0, np.exp(-dA * dA / eps**2), 1.0)
    sR = np.where(np.real(dR) > 0, np.exp(-dR * dR / eps**2), 1.0)
    return sA * sR


class Sources:
    """The fvSource option at its definition: the cell sets and the snapped cells are chosen from the Geom of that moment and kept."""

    def __init__(self, g0, fvSource):
        self.entries = {}
        for name in sorted(fvSource):
            e = dict(fvSource[name])
            if e["source"] == "cylinderToCell":
                e["cells"] = cylinder_cells(g0, e["p1"], e["p2"], e["radius"])
                assert e["cells"].size, name
            else:
                e["pars"] = np.array(list(e["center"]) + list(e["axis"]) + [e["radius"], e["length"], e["power"]], dtype=np.complex128)
                e["cell"] = None
                if e.get("snapCenter2Cell"):
                    found = containing_cells(g0, e["center"])
                    assert found.size == 1, (name, found)
                    e["cell"] = int(found[0])
            self.entries[name] = e

    def total_power(self):
        return sum(float(np.real(e["pars"][8])) if "pars" in e else float(e["power"]) for e in self.entries.values())

    def entry_field(self, g, name, pars=None, frozen=None):
        """(q, Vt) of one entry at the metrics g; pars: other parameters than the entry's own; frozen: another Geom whose total volume and
        snapped centre are used instead of g's (what a pass that lets a point reach its own rows only can see)"""
        e = self.entries[name]
        gc = g if frozen is None else frozen
        if e["source"] == "cylinderToCell":
            s = np.zeros(g.nC)
            s[e["cells"]] = 1.0
            power = e["power"]
            sf = s
        else:
            p = e["pars"] if pars is None else np.asarray(pars)
            s = smooth_shape(g, p, e["eps"], center=None if e["cell"] is None else gc.C[e["cell"]])
            sf = s if frozen is None else smooth_shape(gc, p, e["eps"], center=None if e["cell"] is None else gc.C[e["cell"]])
            power = p[8]
        Vt = (sf * gc.V).sum()
        return power * s / Vt, Vt

    def field(self, g, pars=None, frozen=None):
        """fvSource; pars: {name: parameters} replacing those of the entries named"""
        q = 0.0
        for name in self.entries:
            q = q + self.entry_field(g, name, (pars or {}).get(name), frozen)[0]
        return q


def residual(case, g, T, sources, normalized=True, pars=None, frozen=None, **kw):
    q = sources.field(g, pars, frozen)
    return H.residual(case, g, T, normalized=True, **kw) + q if normalized else (H.residual(case, g, T, normalized=True, **kw) + q) * g.V

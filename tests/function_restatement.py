"""numpy restatement of the field-valued objectives (reference DAFunctionVariableVolSum.C, DAFunctionPatchMean.C,
DAFunctionVariance.C modes field / surface).  Every function takes the state vector W in "state" ordering and works with complex
W, so oracle.functions.gradient gives complex-step derivatives."""
import numpy as np

from common import blocks
from oracle.functions import _boundary_state, _select
from oracle.residual import BCTable, Ops, bc_scalar


def cell_values(case, g, W, var, beta=None):
    """(N,) or (N, 3) cell values of a state variable (or of the betaFINuTilda field)."""
    if var == "betaFINuTilda":
        return np.ones(g.nC) if beta is None else beta
    sl = dict(blocks(case, g))[var]
    v = W[sl]
    return v.reshape(-1, 3) if var == "U" else v


def box_cells(C, lo, hi):
    """boxToCell: the cells whose centre lies in the closed box [lo, hi]."""
    return np.nonzero(np.all((C >= np.asarray(lo)) & (C <= np.asarray(hi)), axis=1))[0]


def function_cells(g, fd):
    if fd.get("source", "allCells") == "allCells":
        return np.arange(g.nC)
    return box_cells(g.C, fd["min"], fd["max"])


def total_vol(g, fd):
    return 1.0 + g.V.sum() if int(fd.get("divByTotalVol", 0)) else 1.0


def variable_vol_sum(case, g, W, fd, beta=None):
    cells = function_cells(g, fd)
    q = cell_values(case, g, W, fd["varName"], beta)
    q = q[cells, int(fd.get("index", 0))] if fd["varType"] == "vector" else q[cells]
    if int(fd.get("isSquare", 0)):
        q = q * q
    w = g.V[cells] if int(fd.get("multiplyVol", 1)) else np.ones(cells.size)
    F = (float(fd.get("scale", 1.0)) * w * q).sum() / total_vol(g, fd)
    if int(fd.get("calcRefVar", 0)):
        F = (F - fd["ref"][0]) ** 2
    return F


def boundary_values(case, g, W, var):
    b = _boundary_state(case, g, W)
    if var == "T" and b["Tb"] is None:  # the passive T of DASimpleFoam: [U | p | T | nuTilda | phi]
        N = g.nC
        bt = BCTable(case, g, ("T",))
        phi_b = W[6 * N + g.nIF : 6 * N + g.nF]
        return bc_scalar(bt.code["T"], bt.val["T"], W[4 * N : 5 * N][Ops(g).bc], g.bDeltaCoeffs, phi_b)[0]
    return {"U": b["Ub"], "p": b["pb"], "T": b["Tb"]}[var]


def patch_mean(case, g, W, fd):
    sel = _select(g, case, fd["patches"])
    q = boundary_values(case, g, W, fd["varName"])
    q = q[sel, int(fd.get("index", 0))] if fd["varType"] == "vector" else q[sel]
    a = g.bMagSf[sel]
    F = (float(fd.get("scale", 1.0)) * a * q).sum() / a.sum()
    if int(fd.get("calcRefVar", 0)):
        F = (F - fd["ref"][0]) ** 2
    return F


def variance(case, g, W, fd, ref_data):
    """ref_data: FoamCase.ref_data ({"<var>Data": {"internal", "boundary"}}); no entry: 0 (isRefData_ == 0)."""
    var, vec = fd["varName"], fd["varType"] == "vector"
    d = ref_data.get(var + "Data")
    if d is None:
        return 0.0
    comps = list(fd["indices"]) if vec else [0]
    if fd["mode"] == "field":
        rows = function_cells(g, fd)
        q, dat, w = cell_values(case, g, W, var)[rows], np.asarray(d["internal"])[rows], g.V[rows]
    else:
        sel = _select(g, case, fd["patches"])
        rows = np.nonzero(sel)[0]  # boundary faces in face order = the patches in the mesh's order
        q, dat, w = boundary_values(case, g, W, var)[rows], np.asarray(d["boundary"])[rows], g.bMagSf[rows]
    if not vec:
        q, dat = q[:, None], dat[:, None]
    diff = q[:, comps] - dat[:, comps]
    geo = int(fd.get("useGeoWeight", 0))
    ww = np.repeat(w[:, None], len(comps), axis=1) if geo else np.ones(diff.shape)
    return (ww * float(fd.get("scale", 1.0)) * diff * diff).sum() / (ww.sum() if geo else diff.size)

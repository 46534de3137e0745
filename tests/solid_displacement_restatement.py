"""numpy restatement of the reference's structural solver DASolidDisplacementFoam, written from the reference's sources and OpenFOAM's
published operators - not from the kernel bodies:
  readMechanicalPropertiesSolidDisplacement.H:133-156  E / rho, mu = E / (2 (1 + nu)), lambda = nu E / ((1 + nu)(1 - 2 nu)), or
                                                       nu E / ((1 + nu)(1 - nu)) under planeStress
  DAResidualSolidDisplacementFoam.C:66-76   sigmaD = mu twoSymm(gradD) + lambda I tr(gradD); divSigmaExp = fvc::div(sigmaD - (2 mu + lambda)
                                            gradD); DEqn: d2dt2(D) == laplacian(2 mu + lambda, D) + divSigmaExp; DRes = DEqn & D, normalised
  DAResidualSolidDisplacementFoam.C:86      gradD = fvc::grad(D) (Gauss linear, with OpenFOAM's corrected boundary values
                                            G_c + n (snGrad(D) - n . G_c) on the non-coupled patches)
  tractionDisplacementFvPatchVectorField.C:89-117   the lagged gradient of the traction patch
  DASolver.C:2870 (updateStateBoundaryConditions)   maxCorrectBCCalls times: D.correctBoundaryConditions(), then gradD = fvc::grad(D)
  DAFunctionVonMisesStressKS.C:55-77        sigma = rho sigmaD, vm = scale sqrt(1.5 |dev sigma|^2), KS = log(sum exp(coeffKS vm)) / coeffKS
The reference carries the gradient of the traction patch from call to call; a residual that is a function of the states alone starts every
evaluation from the freshly constructed patch field (gradient 0, D_b = D_c, gradD of that), followed by exactly `passes` passes.
The steady d2dt2 is exactly zero.  M & D = (A D - b) / V with A = -laplacian matrix and b = V divSigmaExp, so
DRes = -(laplacian(2 mu + lambda, D) + divSigmaExp).  Everything takes complex D and points (the Geom of heat_transfer_restatement)."""
import numpy as np

from dafoam_amd.meshgen import BC_FIXED_VALUE, BC_SYMMETRY, BC_TRACTION, BC_ZERO_GRADIENT
from heat_transfer_restatement import Geom  # noqa: F401  (the metrics; re-exported)


def lame(mech):
    E = mech["E"] / mech["rho"]
    nu = mech["nu"]
    mu = E / (2.0 * (1.0 + nu))
    lam = nu * E / ((1.0 + nu) * (1.0 - nu)) if mech.get("planeStress", False) else nu * E / ((1.0 + nu) * (1.0 - 2.0 * nu))
    return mu, lam


def _patch_codes(case, g):
    nBF = g.nF - g.nIF
    code = np.full(nBF, BC_ZERO_GRADIENT)
    val, trac, pres = np.zeros((nBF, 3)), np.zeros((nBF, 3)), np.zeros(nBF)
    for p in case.mesh.patches:
        sl = g.patch_slices()[p.name]
        ent = case.bcs.get(p.name, {}).get("D", (BC_ZERO_GRADIENT, 0.0))
        code[sl] = ent[0]
        if ent[0] == BC_FIXED_VALUE:
            val[sl] = ent[1]
        elif ent[0] == BC_TRACTION:
            trac[sl], pres[sl] = ent[1], ent[2]
        else:
            assert ent[0] in (BC_ZERO_GRADIENT, BC_SYMMETRY), ent[0]
    return code, val, trac, pres


def _grad(g, D, Db):
    """fvc::grad(D), Gauss linear: G[c, i, j] = (1 / V) sum_f S_i D_j"""
    nIF = g.nIF
    oi, ni = g.own[:nIF], g.nei
    Df = g.w[:, None] * D[oi] + (1.0 - g.w[:, None]) * D[ni]
    G = np.zeros((g.nC, 3, 3), np.result_type(D, Db, g.Sf, np.float64))
    t = g.Sf[:nIF, :, None] * Df[:, None, :]
    np.add.at(G, oi, t)
    np.add.at(G, ni, -t)
    np.add.at(G, g.bcell, g.Sf[nIF:, :, None] * Db[:, None, :])
    return G / g.V[:, None, None]


def _bgrad(g, G, sn):
    """the boundary values of gradD: G_c + n (snGrad - n . G_c)"""
    n = g.nf[g.nIF:]
    Gc = G[g.bcell]
    return Gc + n[:, :, None] * (sn - np.einsum("fi,fij->fj", n, Gc))[:, None, :]


def fields(case, g, D, passes):
    """(G, Db, sn, Gb): the cell gradient, the boundary values and surface-normal gradients of D and the boundary values of gradD after
    `passes` passes of the traction patches from the freshly constructed patch field."""
    D = np.asarray(D).reshape(-1, 3)
    mu, lam = lame(case.mechanical)
    rho = case.mechanical["rho"]
    code, val, trac, pres = _patch_codes(case, g)
    n = g.nf[g.nIF:]
    Dc = D[g.bcell]
    dt = np.result_type(D, g.Sf, np.float64)
    Db, sn = np.array(Dc, dt), np.zeros(Dc.shape, dt)
    fx = code == BC_FIXED_VALUE
    Db[fx] = val[fx]
    sn[fx] = g.bDeltaCoeffs[fx, None] * (val[fx] - Dc[fx])
    sy = code == BC_SYMMETRY  # basicSymmetry: D_b = (D_c + transform(I - 2 n n, D_c)) / 2, snGrad = (transform(I - 2 n n, D_c) - D_c) deltaCoeff / 2
    nD = (n[sy] * Dc[sy]).sum(1)
    Db[sy] = Dc[sy] - n[sy] * nD[:, None]
    sn[sy] = -n[sy] * nD[:, None] * g.bDeltaCoeffs[sy, None]
    tr = code == BC_TRACTION
    G = _grad(g, D, Db)
    Gb = _bgrad(g, G, sn)
    for _ in range(int(passes)):
        B = Gb[tr]
        nt = n[tr]
        nA = mu * np.einsum("fi,fji->fj", nt, B) - (mu + lam) * np.einsum("fi,fij->fj", nt, B)
        gr = ((trac[tr] - pres[tr, None] * nt) / rho - nA - nt * (lam * np.trace(B, axis1=1, axis2=2))[:, None]) / (2.0 * mu + lam)
        sn[tr] = gr
        Db[tr] = Dc[tr] + gr / g.bDeltaCoeffs[tr, None]
        G = _grad(g, D, Db)
        Gb = _bgrad(g, G, sn)
    return G, Db, sn, Gb


def residual(case, g, D, passes=2, normalized=True):
    """DRes, interleaved as the states; normalized: DRes is listed in normalizeResiduals (per unit volume), else multiplied with V."""
    D = np.asarray(D).reshape(-1, 3)
    mu, lam = lame(case.mechanical)
    gam = 2.0 * mu + lam
    N, nIF = g.nC, g.nIF
    oi, ni = g.own[:nIF], g.nei
    G, Db, sn, Gb = fields(case, g, D, passes)

    def X(A):  # sigmaD - (2 mu + lambda) gradD
        return mu * (A + np.swapaxes(A, 1, 2)) + lam * np.trace(A, axis1=1, axis2=2)[:, None, None] * np.eye(3) - gam * A

    w = g.w[:, None, None]
    Xc = X(G)
    Xf = w * Xc[oi] + (1.0 - w) * Xc[ni]
    dflux = np.einsum("fi,fij->fj", g.Sf[:nIF], Xf)
    dfluxb = np.einsum("fi,fij->fj", g.Sf[nIF:], X(Gb))
    Gf = w * G[oi] + (1.0 - w) * G[ni]
    lflux = gam * g.magSf[:nIF, None] * (g.nonOrthDeltaCoeffs[:, None] * (D[ni] - D[oi]) + np.einsum("fi,fij->fj", g.nonOrthCorr, Gf))
    lfluxb = gam * g.bMagSf[:, None] * sn
    tot = np.zeros((N, 3), np.result_type(D, g.Sf, np.float64))
    np.add.at(tot, oi, lflux + dflux)
    np.add.at(tot, ni, -(lflux + dflux))
    np.add.at(tot, g.bcell, lfluxb + dfluxb)
    R = -tot / g.V[:, None]
    if not normalized:
        R = R * g.V[:, None]
    return R.ravel()


def von_mises(case, g, D, passes=2, scale=1.0):
    mu, lam = lame(case.mechanical)
    G = fields(case, g, D, passes)[0]
    sig = case.mechanical["rho"] * (mu * (G + np.swapaxes(G, 1, 2)) + lam * np.trace(G, axis1=1, axis2=2)[:, None, None] * np.eye(3))
    dev = sig - np.trace(sig, axis1=1, axis2=2)[:, None, None] * np.eye(3) / 3.0
    return scale * np.sqrt(1.5 * (dev * dev).sum((1, 2)))


def ks_summands(case, g, D, passes, scale, coeffKS, cells=None):
    """coeffKS vm of the cells of the set (what the reference exponentiates)"""
    vm = von_mises(case, g, D, passes, scale)
    return coeffKS * (vm if cells is None else vm[cells])


def von_mises_ks(case, g, D, passes, scale, coeffKS, cells=None):
    """log(sum exp(coeffKS vm)) / coeffKS, max-shifted (the reference's plain sum, rewritten so that it cannot overflow)"""
    a = ks_summands(case, g, D, passes, scale, coeffKS, cells)
    m = np.real(a).max()
    return (m + np.log(np.exp(a - m).sum())) / coeffKS


def box_cells(g, lo, hi):
    """boxToCell: the cells whose centre lies in the closed box"""
    C = np.real(g.C)
    return np.nonzero(np.all((C >= np.asarray(lo)) & (C <= np.asarray(hi)), axis=1))[0]


def mass(case, g, cells=None, scale=1.0):
    """variableVolSum of solid:rho with multiplyVol: scale sum rho V"""
    V = g.V if cells is None else g.V[cells]
    return scale * case.mechanical["rho"] * V.sum()


def traction_balance(case, g, D, passes):
    """max |n . sigma_b - (t - p n)| over the traction faces, sigma_b = rho sigmaD of the boundary gradD"""
    mu, lam = lame(case.mechanical)
    rho = case.mechanical["rho"]
    code, val, trac, pres = _patch_codes(case, g)
    Gb = fields(case, g, D, passes)[3]
    tr = code == BC_TRACTION
    n = g.nf[g.nIF:][tr]
    B = Gb[tr]
    sig = rho * (mu * (B + np.swapaxes(B, 1, 2)) + lam * np.trace(B, axis1=1, axis2=2)[:, None, None] * np.eye(3))
    err = np.einsum("fi,fij->fj", n, sig) - (trac[tr] - pres[tr, None] * n)
    return float(np.abs(err).max())


def jacobian(case, g, D, passes=2, normalized=True, h=1e-30):
    """dDRes/dD by the complex step, dense (test meshes only)"""
    D = np.asarray(D, dtype=np.float64).ravel()
    J = np.zeros((D.size, D.size))
    for j in range(D.size):
        Dp = D.astype(np.complex128)
        Dp[j] += 1j * h
        J[:, j] = residual(case, g, Dp, passes, normalized).imag / h
    return J

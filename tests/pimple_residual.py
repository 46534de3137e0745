"""The oracle's simple_residual (oracle/residual.py:268-523) with the time-derivative terms of DAPimpleFoam (reference
DAResidualPimpleFoam.C:94-227, DASpalartAllmaras.C:453): fvm::ddt(U) and fvm::ddt(nuTilda) enter the two matrices - the diagonal gains
c V / deltaT, the source V / deltaT (c0 x0 - c00 x00) - before UEqn.relax(1.0), so the dominance fix-up, A and H see them; the pressure equation is
DASimpleFoam's with phiHbyA = flux(HbyA) (no ddtCorr).  The oracle has no hook for this and is not edited, so this tests-side copy carries
it, the way tests/actuator_disk_residual.py carries its source term; everything else is the oracle's text, line for line, and its helpers
are the oracle's own.  Complex-safe in W, W0 and W00.  tests/test_pimple_cpu.py checks that c = c0 = c00 = 0 with the case's own relax
factor gives the oracle's bits on the four meshes of tests/actuator_disk_cases.py, and that W0 = W under Euler is the steady residual."""
import numpy as np

from dafoam_amd.meshgen import BC_FIXED_VALUE, BC_SYMMETRY, NUT_LOWRE_WALL, NUT_SPALDING_WALL, NUT_SYMMETRY
from oracle.residual import SA, SMALL, VSMALL, BCTable, Ops, _abs, _beta_fi, _max, _min, bc_scalar, bc_vector, dev2T, fv1_of, relax_diag, sadd, spalding_nut, unpack_simple


def ddt_coeffs(scheme, time_index):
    """(c, c0, c00) of fvm::ddt at constant deltaT: Euler 1, 1, 0; backward 1.5, 2, 0.5, and below time index 2 exactly Euler (OpenFOAM's
    deltaT0_() returns GREAT there and the three coefficients round to 1, 1, 0)."""
    if scheme == "backward" and time_index >= 2:
        return 1.5, 2.0, 0.5
    if scheme in ("Euler", "backward"):
        return 1.0, 1.0, 0.0
    raise ValueError(f"ddtScheme {scheme} not supported! Options: steadyState, Euler, or backward")


def pimple_residual(case, g, W, W0, W00=None, coeffs=None, time_index=1, relax_U=1.0, dUb=None, isPC=False, normalize=("URes", "pRes", "TRes", "nuTildaRes", "phiRes"), pc_blend=0.0,
                    use_constrain_hbya=True, return_parts=False):
    """W0, W00: the old-time state vectors in the layout of W (W00 None: not read, c00 must be 0); coeffs: (c, c0, c00), default those of
    case.ddt_scheme at time_index; relax_U: 1.0 as UEqn.relax(1.0) has it (None: the case's own factor, for the check against the oracle);
    dUb: (nBF, 3) added to the patch values of U, complex for the complex step in a boundary value (W complex then).
    R(W; W0, W00) for DASimpleFoam + Spalart-Allmaras in DAIndex 'state' ordering:
    [URes (3N, xyz interleaved) | pRes (N) | nuTildaRes (N) | phiRes (F, internal then boundary)]."""
    N, F, nIF, nBF = g.nC, g.nF, g.nIF, g.nBF
    ops = Ops(g)
    oi, ni, bcell = ops.oi, ops.ni, ops.bc
    U, p, nuT, phi = unpack_simple(W, N, F)
    c_, c0_, c00_ = ddt_coeffs(getattr(case, "ddt_scheme", "Euler"), time_index) if coeffs is None else coeffs
    U0, _, nuT0, _ = unpack_simple(W0, N, F)
    oldU, oldN = c0_ * U0, c0_ * nuT0
    if c00_ != 0.0:
        U00, _, nuT00, _ = unpack_simple(W00, N, F)
        oldU, oldN = oldU - c00_ * U00, oldN - c00_ * nuT00
    vdt = g.V / case.deltaT
    dt = np.result_type(W.dtype, oldU.dtype)
    nu = case.nu
    phi_i, phi_b = phi[:nIF], phi[nIF:]
    bt = BCTable(case, g, ("U", "p", "nuTilda", "nut"))
    if dUb is not None:
        bt.val["U"] = bt.val["U"] + dUb
    delta = g.bDeltaCoeffs
    V = g.V

    # ---- MRF (OpenFOAM MRFZone, one zone = the mesh; DAResidualSimpleFoam.C:139,182,245) and SIMPLEC (:187-194)
    from oracle.residual_rho import mrf_fields  # geometry-only helper shared with the compressible restatement

    mrf = mrf_fields(case, g)
    consistent = bool(getattr(case, "simple_consistent", False))
    if mrf is not None:  # correctBoundaryVelocity
        rot = mrf["incl"] & (bt.code["U"] == BC_FIXED_VALUE)
        bt.val["U"] = np.where(rot[:, None], mrf["vFb"], bt.val["U"])
    # ---- correctBoundaryConditions (DAResidualSimpleFoam.C:250-265, DASpalartAllmaras.C:235-243)
    Ub, UvIC, UvBC, UgIC, UgBC = bc_vector(bt.code["U"], bt.val["U"], U[bcell], delta, phi_b, g.bnf)
    pb, pvIC, pvBC, pgIC, pgBC = bc_scalar(bt.code["p"], bt.val["p"], p[bcell], delta, phi_b)
    nb, nvIC, nvBC, ngIC, ngBC = bc_scalar(bt.code["nuTilda"], bt.val["nuTilda"], nuT[bcell], delta, phi_b)

    # ---- correctNut (DASpalartAllmaras.C:215-233): nut = nuTilda*fv1(chi), then nut BCs
    chi = nuT / nu
    fv1 = fv1_of(chi)
    nut = nuT * fv1
    nut_b = nb * fv1_of(nb / nu)  # calculated patches
    cn = bt.code["nut"]
    nut_b = np.where(cn == NUT_LOWRE_WALL, 0.0 * nut_b, nut_b)
    nut_b = np.where(cn == NUT_SYMMETRY, nut[bcell], nut_b)
    wf = cn == NUT_SPALDING_WALL
    if wf.any():
        dU = U[bcell][wf] - Ub[wf]
        magUp = np.sqrt((dU * dU).sum(1) + 0.0)
        magGradU = magUp * delta[wf]
        ywf = np.abs(((g.Cf[nIF:][wf] - g.C[bcell][wf]) * g.bnf[wf]).sum(1))
        nw = spalding_nut(magUp, magGradU, ywf, nu)
        tmp = nut_b.astype(dt)
        tmp[wf] = nw
        nut_b = tmp
    nuEff = nu + nut
    nuEff_b = nu + nut_b

    # ---- gradients (Gauss linear) and their boundary values (GaussGrad::correctBoundaryConditions)
    gradU = ops.grad_vector(U, Ub)
    gradP = ops.grad_scalar(p, pb)
    snGradU_b = UgIC * U[bcell] + UgBC
    gUc = gradU[bcell]
    n_b = g.bnf
    ngU = np.einsum("fk,fkj->fj", n_b, gUc)
    gradU_b = gUc + n_b[:, :, None] * (snGradU_b - ngU)[:, None, :]

    # =================================================================== UEqn
    # fvm::div(phi,U) [bounded Gauss upwind weights; linearUpwindV explicit correction unless PC]
    wu = (np.real(phi_i) >= 0).astype(float)  # upwind weights = pos0(flux)
    lower = -wu * phi_i  # coefficient of owner value in neighbour's equation
    upper = lower + phi_i  # coefficient of neighbour value in owner's equation
    diag = sadd(oi, -lower, N) + sadd(ni, -upper, N)
    # bounded: - fvm::Sp(fvc::surfaceIntegrate(phi), U)
    sumPhi = ops.surface_sum(phi_i, phi_b)
    diag = diag - sumPhi
    iC = phi_b[:, None] * UvIC  # internalCoeffs (vector per boundary face)
    bC = -phi_b[:, None] * UvBC  # boundaryCoeffs
    src = np.zeros((N, 3), dtype=dt)
    conv_blend = float(pc_blend) if isPC else 1.0  # weight of the explicit linearUpwindV correction (PC: amd.pcUpwindBlend, default 0)
    if conv_blend > 0.0:
        pos = np.real(phi_i) > 0
        d_o = g.Cf[:nIF] - g.C[oi]
        d_n = g.Cf[:nIF] - g.C[ni]
        c_o = np.einsum("fi,fij->fj", d_o, gradU[oi])
        c_n = np.einsum("fi,fij->fj", d_n, gradU[ni])
        wl = g.w[:, None]
        m_o = (1.0 - wl) * (U[ni] - U[oi])
        m_n = wl * (U[oi] - U[ni])
        corr = np.where(pos[:, None], c_o, c_n)
        mx = np.where(pos[:, None], m_o, m_n)
        sfc = (corr * corr).sum(1)
        mxc = (corr * mx).sum(1)
        scale = np.where(
            np.real(sfc) > 0,
            np.where(np.real(mxc) < 0, 0.0 * mxc, np.where(np.real(sfc) > np.real(mxc), mxc / (sfc + VSMALL), 1.0 + 0 * mxc)),
            1.0 + 0 * mxc,
        )
        corr = corr * scale[:, None]
        fcorr = conv_blend * phi_i[:, None] * corr
        src = src - (sadd(oi, fcorr, N) - sadd(ni, fcorr, N))
    # - fvm::laplacian(nuEff, U)  (Gauss linear corrected)
    gam = ops.interp(nuEff) * g.magSf[:nIF]
    gam_b = nuEff_b * g.bMagSf
    cdiff = gam * g.nonOrthDeltaCoeffs
    upper = upper - cdiff
    lower = lower - cdiff
    diag = diag + sadd(oi, cdiff, N) + sadd(ni, cdiff, N)
    gradUf = ops.interp(gradU)
    fcorrL = gam[:, None] * np.einsum("fi,fij->fj", g.nonOrthCorr, gradUf)
    src = src + (sadd(oi, fcorrL, N) - sadd(ni, fcorrL, N))
    iC = iC - gam_b[:, None] * UgIC
    bC = bC + gam_b[:, None] * UgBC
    # - fvc::div(nuEff*dev2(T(grad(U))))  (explicit, Gauss linear)
    tau = nuEff[:, None, None] * dev2T(gradU)
    tau_b = nuEff_b[:, None, None] * dev2T(gradU_b)
    tf = np.einsum("fi,fij->fj", g.Sf[:nIF], ops.interp(tau))
    tb = np.einsum("fi,fij->fj", g.bSf, tau_b)
    src = src + ops.surface_sum(tf, tb)
    if mrf is not None:  # + MRF.DDt(U): source -= V (Omega x U)
        src = src - V[:, None] * np.cross(mrf["om"], U)
    # + fvm::ddt(U): before relax()
    diag = diag + c_ * vdt
    src = src + vdt[:, None] * oldU
    # UEqn.relax()
    D0 = diag
    sumOff = sadd(oi, _abs(upper), N) + sadd(ni, _abs(lower), N)
    alphaU = case.relax["U"] if relax_U is None else relax_U
    D = relax_diag(D0, sumOff, iC, bcell, alphaU, N)
    src = src + (D - D0)[:, None] * U
    # (UEqn & U) + grad(p)
    offU = sadd(oi, upper[:, None] * U[ni], N) + sadd(ni, lower[:, None] * U[oi], N)
    bdiag = sadd(bcell, iC, N)  # (N,3)
    bsrc = sadd(bcell, bC, N)
    URes = ((D[:, None] + bdiag) * U + offU - src - bsrc) / V[:, None] + gradP
    # A, H (fvMatrix::A/H with component-averaged boundary diagonal)
    avgb = bdiag.sum(1) / 3.0
    A = (D + avgb) / V
    H = ((avgb[:, None] - bdiag) * U - offU + src + bsrc) / V[:, None]
    rAU = 1.0 / A
    HbyA = rAU[:, None] * H

    # =================================================================== pEqn
    # boundary HbyA: extrapolated (zero-gradient; symmetry transform on symmetry patches),
    # constrainHbyA: U_b on non-assignable (fixedValue) patches (DAResidualSimpleFoam.C:163-178)
    cU = bt.code["U"]
    HbyA_b = HbyA[bcell].copy()
    symU = cU == BC_SYMMETRY
    if symU.any():
        hn = (HbyA_b[symU] * n_b[symU]).sum(1)[:, None]
        HbyA_b[symU] = HbyA_b[symU] - n_b[symU] * hn
    if use_constrain_hbya:
        fx = cU == BC_FIXED_VALUE
        HbyA_b[fx] = Ub[fx]
    phiHbyA_i = (ops.interp(HbyA) * g.Sf[:nIF]).sum(1)
    phiHbyA_b = (HbyA_b * g.bSf).sum(1)
    if mrf is not None:  # MRF.makeRelative(phiHbyA)
        phiHbyA_i = phiHbyA_i - mrf["rel_i"]
        phiHbyA_b = np.where(mrf["incl"], 0.0 * phiHbyA_b, phiHbyA_b - mrf["rel_b"])
    # (adjustPhi / setReference are no-ops: p has a fixedValue patch -> !p.needReference())
    gradPf = ops.interp(gradP)
    snGradP_i = g.nonOrthDeltaCoeffs * (p[ni] - p[oi]) + (g.nonOrthCorr * gradPf).sum(1)
    snGradP_b = pgIC * p[bcell] + pgBC
    rAtU = rAU
    if consistent:  # SIMPLEC: rAtU = 1/(1/rAU - H1), H1 = -sum(off-diagonal)/V
        H1 = -(sadd(oi, upper, N) + sadd(ni, lower, N)) / V
        rAtU = 1.0 / (A - H1)
        phiHbyA_i = phiHbyA_i + ops.interp(rAtU - rAU) * snGradP_i * g.magSf[:nIF]
        phiHbyA_b = phiHbyA_b + (rAtU - rAU)[bcell] * snGradP_b * g.bMagSf
    gp = ops.interp(rAtU) * g.magSf[:nIF]
    gp_b = rAtU[bcell] * g.bMagSf
    # fvm::laplacian(rAtU, p): flux() = upper*(pN - pO) + faceFluxCorrection ; boundary iC*p_c - bC
    flux_i = gp * snGradP_i
    flux_b = gp_b * snGradP_b
    # pRes = pEqn & p = (laplacian(rAU,p) - div(phiHbyA)) / V
    pRes = (ops.surface_sum(flux_i, flux_b) - ops.surface_sum(phiHbyA_i, phiHbyA_b)) / V
    # phiRes = phiHbyA - pEqn.flux() - phi
    phiRes = np.concatenate([phiHbyA_i - flux_i - phi_i, phiHbyA_b - flux_b - phi_b])

    # =================================================================== SA (DASpalartAllmaras.C:407-488)
    gradN = ops.grad_scalar(nuT, nb)
    y = case.y_wall
    k2y2 = (SA["kappa"] * y) ** 2
    skew = 0.5 * (gradU - np.swapaxes(gradU, 1, 2))
    Omega = np.sqrt(2.0) * np.sqrt((skew * skew).sum((1, 2)) + 0.0)
    fv2 = 1.0 - chi / (1.0 + chi * fv1)
    Stilda = _max(Omega + fv2 * nuT / k2y2, SA["Cs"] * Omega)
    r = _min(nuT / (_max(Stilda, SMALL + 0 * Stilda) * k2y2), 10.0 + 0 * Stilda)
    gg = r + SA["Cw2"] * (r**6 - r)
    fw = gg * ((1.0 + SA["Cw3"] ** 6) / (gg**6 + SA["Cw3"] ** 6)) ** (1.0 / 6.0)
    # div(phi,nuTilda): bounded Gauss upwind (same for PC)
    lo = -wu * phi_i
    up = lo + phi_i
    dN = sadd(oi, -lo, N) + sadd(ni, -up, N) - sumPhi
    iCn = phi_b * nvIC
    bCn = -phi_b * nvBC
    # - laplacian(DnuTildaEff, nuTilda)
    Dn = (nuT + nu) / SA["sigmaNut"]
    Dn_b = (nb + nu) / SA["sigmaNut"]
    gn = ops.interp(Dn) * g.magSf[:nIF]
    gn_b = Dn_b * g.bMagSf
    cd = gn * g.nonOrthDeltaCoeffs
    up = up - cd
    lo = lo - cd
    dN = dN + sadd(oi, cd, N) + sadd(ni, cd, N)
    dN = dN + c_ * vdt  # + fvm::ddt(nuTilda)
    fcn = gn * (g.nonOrthCorr * ops.interp(gradN)).sum(1)
    sN = sadd(oi, fcn, N) - sadd(ni, fcn, N)
    sN = sN + vdt * oldN
    iCn = iCn - gn_b * ngIC
    bCn = bCn + gn_b * ngBC
    offN = sadd(oi, up * nuT[ni], N) + sadd(ni, lo * nuT[oi], N)
    bdN = sadd(bcell, iCn, N)
    bsN = sadd(bcell, bCn, N)
    conv_diff = ((dN + bdN) * nuT + offN - sN - bsN) / V
    nuTildaRes = (
        conv_diff
        - SA["Cb2"] / SA["sigmaNut"] * (gradN * gradN).sum(1)
        - SA["Cb1"] * Stilda * nuT * _beta_fi(case, N)
        + SA["Cw1"] * fw * nuT / (y * y) * nuT
    )
    # (relax() leaves M & psi unchanged)

    # =================================================================== optional T field (DAResidualSimpleFoam.C:215-235)
    # TEqn = div(phi,T) - laplacian(alphaEff,T), alphaEff = nu/Pr + alphat, alphat = nut/Prt; bounded Gauss upwind /
    # Gauss linear corrected.  T is a passive scalar: no other residual depends on it.
    TRes = None
    if getattr(case, "has_T", False):
        Tt = W[4 * N : 5 * N]
        Pr, Prt = case.thermo["Pr"], case.thermo["Prt"]
        btT = BCTable(case, g, ("T",))
        Tb, TvIC, TvBC, TgIC, TgBC = bc_scalar(btT.code["T"], btT.val["T"], Tt[bcell], delta, phi_b)
        gradT = ops.grad_scalar(Tt, Tb)
        aEff = nu / Pr + nut / Prt
        aEff_b = nu / Pr + nut_b / Prt
        loT = -wu * phi_i
        upT = loT + phi_i
        dT = sadd(oi, -loT, N) + sadd(ni, -upT, N) - sumPhi
        ga = ops.interp(aEff) * g.magSf[:nIF]
        ga_b = aEff_b * g.bMagSf
        cdT = ga * g.nonOrthDeltaCoeffs
        upT, loT = upT - cdT, loT - cdT
        dT = dT + sadd(oi, cdT, N) + sadd(ni, cdT, N)
        fcT = ga * (g.nonOrthCorr * ops.interp(gradT)).sum(1)
        sT = sadd(oi, fcT, N) - sadd(ni, fcT, N)
        iCt = phi_b * TvIC - ga_b * TgIC
        bCt = -phi_b * TvBC + ga_b * TgBC
        offT = sadd(oi, upT * Tt[ni], N) + sadd(ni, loT * Tt[oi], N)
        TRes = ((dT + sadd(bcell, iCt, N)) * Tt + offT - sT - sadd(bcell, bCt, N)) / V
        if "TRes" not in normalize:
            TRes = TRes * V

    # ---- normalisation macros (DAMacroFunctions.H:28-51)
    if "URes" not in normalize:
        URes = URes * V[:, None]
    if "pRes" not in normalize:
        pRes = pRes * V
    if "nuTildaRes" not in normalize:
        nuTildaRes = nuTildaRes * V
    if "phiRes" in normalize:
        phiRes = phiRes / g.magSf
    R = np.concatenate([URes.ravel(), pRes, nuTildaRes, phiRes] if TRes is None else [URes.ravel(), pRes, TRes, nuTildaRes, phiRes])
    if return_parts:
        parts = dict(
            Ub=Ub, pb=pb, nuTildab=nb, nut=nut, nut_b=nut_b, gradU=gradU, gradP=gradP, gradN=gradN,
            D=D, A=A, H=H, rAU=rAU, HbyA=HbyA, phiHbyA=np.concatenate([phiHbyA_i, phiHbyA_b]),
            URes=URes, pRes=pRes, nuTildaRes=nuTildaRes, phiRes=phiRes, Stilda=Stilda, fw=fw,
        )
        return R, parts
    return R

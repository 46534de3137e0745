"""numpy restatement of totalPressureRatio (reference DAFunctionTotalPressureRatio.C:50-139), wallHeatFlux (DAFunctionWallHeatFlux.C:115-304,
fluid branches) and location (DAFunctionLocation.C:83-126, 153-295), written from those files.  Every function takes the state vector W in
"state" ordering and works with complex W, so oracle.functions.gradient gives complex-step derivatives; wall_heat_flux also takes complex
boundary values of T (T_values), for the derivative in a patchVar input."""
import numpy as np

from dafoam_amd.meshgen import NUT_LOWRE_WALL, NUT_SPALDING_WALL, NUT_SYMMETRY
from oracle.functions import _boundary_state, _select
from oracle.residual import BCTable, Ops, bc_scalar, bc_vector, fv1_of, spalding_nut

TREF = 298.15  # hConst enthalpy he = Cp (T - Tref)


def is_compressible(case):
    return case.solver_name in ("DARhoSimpleFoam", "DATurboFoam")


def calc_ref_var(F, fd):
    """DAFunction::calcRefVar (DAFunction.C:204-224) with one reference value."""
    return (F - fd["ref"][0]) ** 2 if int(fd.get("calcRefVar", 0)) else F


def total_pressure_ratio(case, g, W, fd, b=None):
    """TP_out / TP_in, TP the area average of p (1 + (gamma-1)/2 Ma^2)^(gamma/(gamma-1)), Ma^2 = (|U| / sqrt(gamma R T))^2, R = Cp - Cp/gamma."""
    inlet, outlet = fd["inletPatches"], fd["outletPatches"]
    for p in fd["patches"]:
        if p not in inlet and p not in outlet:
            raise ValueError("inlet/outletPatches names are not in patches")
    b = _boundary_state(case, g, W) if b is None else b  # (b: the boundary state of W, to share it among several functions)
    Cp, gamma = case.thermo["Cp"], float(case.thermo.get("gamma", 1.4))
    R = Cp - Cp / gamma
    UMag = np.sqrt((b["Ub"] * b["Ub"]).sum(1) + 0.0)
    Ma2 = (UMag / np.sqrt(gamma * R * b["Tb"])) ** 2
    pT = b["pb"] * (1.0 + 0.5 * (gamma - 1.0) * Ma2) ** (gamma / (gamma - 1.0))
    avg = []
    for names in (inlet, outlet):
        sel = _select(g, case, [p for p in fd["patches"] if p in names])
        a = g.bMagSf[sel]
        avg.append((pT[sel] * a / a.sum()).sum())
    return calc_ref_var(avg[1] / avg[0], fd)


def thermal_boundary(case, g, W, T_values=None):
    """Per boundary face: the energy variable x (T, or he = Cp (T - Tref) for the compressible solvers) in the near-wall cell and on the face,
    its patch-normal gradient from the patch field, and the boundary alphaEff (DATurbulenceModel::alphaEff: nu/Pr + nut/Prt, or
    mu/Pr + rho nut/Prt).  T_values: {patch: value} replaces the boundary value of T on those patches (may be complex)."""
    N, F, nIF = g.nC, g.nF, g.nIF
    bcell = Ops(g).bc
    rho = is_compressible(case)
    if not rho and not getattr(case, "has_T", False):
        raise ValueError("wallHeatFlux needs a T field")
    W = np.asarray(W)
    if T_values:
        W = W.astype(np.complex128)
    T = W[4 * N : 5 * N]
    U = W[: 3 * N].reshape(N, 3)
    nuT = W[5 * N : 6 * N]
    phi_b = W[6 * N + nIF : 6 * N + F]
    bt = BCTable(case, g, ("U", "p", "T", "nuTilda", "nut"))
    Tval = bt.val["T"].astype(W.dtype)
    for name, v in (T_values or {}).items():
        Tval[g.patch_slices()[name]] = v
    delta = g.bDeltaCoeffs
    th = case.thermo
    Cp, Pr, Prt = th["Cp"], th["Pr"], th["Prt"]
    if rho:
        from oracle.residual_rho import mrf_fields  # MRFZone::correctBoundaryVelocity on rotating fixedValue patches

        mrf = mrf_fields(case, g)
        if mrf is not None:
            bt.val["U"] = np.where((mrf["incl"] & (bt.code["U"] == 0))[:, None], mrf["vFb"], bt.val["U"])
    Ub = bc_vector(bt.code["U"], bt.val["U"], U[bcell], delta, phi_b, g.bnf)[0]
    pb = bc_scalar(bt.code["p"], bt.val["p"], W[3 * N : 4 * N][bcell], delta, phi_b)[0]
    if rho:
        assert th.get("transport", "const") == "const"
        xc = Cp * (T[bcell] - TREF)
        xb, _, _, gic, gbc = bc_scalar(bt.code["T"], Cp * (Tval - TREF), xc, delta, phi_b)
        Tb = xb / Cp + TREF
        rho_b = pb / ((8314.47 / th["molWeight"]) * Tb)
        nu_b = th["mu"] / rho_b
    else:
        xc = T[bcell]
        xb, _, _, gic, gbc = bc_scalar(bt.code["T"], Tval, xc, delta, phi_b)
        rho_b, nu_b = np.ones(g.nBF), case.nu * np.ones(g.nBF)
    # the boundary nut: calculated (nuTilda fv1), low-Re wall (0), symmetry (cell value), Spalding wall function
    nb = bc_scalar(bt.code["nuTilda"], bt.val["nuTilda"], nuT[bcell], delta, phi_b)[0]
    nut_b = nb * fv1_of(nb / nu_b)
    cn = bt.code["nut"]
    nut_b = np.where(cn == NUT_LOWRE_WALL, 0.0 * nut_b, nut_b)
    nu_c = case.nu if not rho else th["mu"] / (W[3 * N : 4 * N] / ((8314.47 / th["molWeight"]) * T))
    nut_c = nuT * fv1_of(nuT / nu_c)
    nut_b = np.where(cn == NUT_SYMMETRY, nut_c[bcell], nut_b)
    wf = cn == NUT_SPALDING_WALL
    if wf.any():
        dU = U[bcell][wf] - Ub[wf]
        magUp = np.sqrt((dU * dU).sum(1) + 0.0)
        ywf = np.abs(((g.Cf[nIF:][wf] - g.C[bcell][wf]) * g.bnf[wf]).sum(1))
        tmp = nut_b.astype(W.dtype)
        tmp[wf] = spalding_nut(magUp, magUp * delta[wf], ywf, nu_b[wf] if rho else case.nu)
        nut_b = tmp
    alphaEff_b = th["mu"] / Pr + rho_b * nut_b / Prt if rho else case.nu / Pr + nut_b / Prt
    return dict(xc=xc, xb=xb, snGrad=gic * xc + gbc, alphaEff_b=alphaEff_b, bcell=bcell)


def wall_heat_flux(case, g, W, fd, wall_distance_method="default", T_values=None, t=None):
    """scale sum w_f q_f: q = Cp alphaEff dT/dn (incompressible) or alphaEff dhe/dn (compressible); dn from the patch field's snGrad
    ("default") or (x_b - x_c) / |C_f - C_c| ("daCustom"); w = |Sf| / sum |Sf| (byUnitArea, the default) or |Sf|."""
    if wall_distance_method not in ("default", "daCustom"):
        raise ValueError(f"wallDistanceMethod: {wall_distance_method} not supported! Options are: default and daCustom.")
    t = thermal_boundary(case, g, W, T_values) if t is None else t  # (t: to share it among several functions of one W)
    if wall_distance_method == "default":
        dxdn = t["snGrad"]
    else:
        d = g.Cf[g.nIF :] - g.C[t["bcell"]]
        dxdn = (t["xb"] - t["xc"]) / np.sqrt((d * d).sum(1))
    q = t["alphaEff_b"] * dxdn * (1.0 if is_compressible(case) else case.thermo["Cp"])
    sel = _select(g, case, fd["patches"])
    a = g.bMagSf[sel]
    scale = float(fd.get("scale", 1.0))
    w = a / a.sum() if bool(fd.get("byUnitArea", True)) else a
    return calc_ref_var((scale * q[sel] * w).sum(), fd)


def location_radius(g, case, fd, projection=False):
    """Per selected face: |c - (c o axis)|, c = C_f - center.  The reference builds the tensor diag(c) and applies it to the axis
    (DAFunctionLocation.C:183-191), so "o" is the component-wise product; projection=True gives what the projection onto the axis would."""
    sel = _select(g, case, fd["patches"])
    axis = np.asarray(fd.get("axis", [1.0, 0.0, 0.0]), dtype=float)
    axis = axis / np.sqrt((axis * axis).sum())
    c = g.Cf[g.nIF :][sel] - np.asarray(fd.get("center", [0.0, 0.0, 0.0]), dtype=float)
    axial = np.outer(c @ axis, axis) if projection else c * axis
    cr = c - axial
    return np.sqrt((cr * cr).sum(1))


def location_terms(g, case, fd):
    """coeffKS a_f of the KS modes."""
    r = location_radius(g, case, fd)
    k = float(fd.get("coeffKS", 1.0))
    return k * r if fd["mode"] == "maxRadiusKS" else k / (r + 1e-12)


def max_radius_face(g, case, fd):
    """The face maxRadius keeps: the largest radius at definition, the first one on ties (DAFunctionLocation.C:83-126)."""
    return int(np.argmax(location_radius(g, case, fd)))


def location(case, g, W, fd, face=None):
    """W is not read.  face: the face of mode maxRadius (index among the selected faces), chosen on the mesh of the definition."""
    if int(fd.get("snapCenter2Cell", 0)):
        raise ValueError("snapCenter2Cell is not restated")
    mode = fd["mode"]
    if mode in ("maxRadiusKS", "maxInverseRadiusKS"):
        x = location_terms(g, case, fd)
        tot = np.exp(x).sum()
        if tot > 1e200:
            raise ValueError("KS function summation term too large! Reduce coeffKS!")
        F = np.log(tot) / float(fd.get("coeffKS", 1.0))
    elif mode == "maxRadius":
        F = location_radius(g, case, fd)[max_radius_face(g, case, fd) if face is None else face]
    else:
        raise ValueError(f"mode: {mode} not supported!")
    return calc_ref_var(F, fd)

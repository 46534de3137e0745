"""numpy restatement of the reference's conjugate heat transfer coupling, written from src/adjoint/DAOutput/DAOutputThermalCoupling.C and
src/adjoint/DAInput/DAInputThermalCoupling.C (discipline aero):
  output :40      the patches are sorted by name before anything else
  output :55-66   size = 2 x the faces of the patches
  output :79-92   entries [0, nF): T of the owner cell, patch by patch, each in face order
  output :94-211  entries [nF, 2 nF): kappa / d = Cp alphaEff_b deltaCoeff; deltaCoeff the patch's delta coefficient (wallDistanceMethod
                  default) or 1 / |C_f - C_c| (daCustom); Cp for the incompressible and for the enthalpy form of the compressible solvers
  input :76-93    refValue = the first half of the input, refGrad = 0
  input :95-222   valueFraction = nk / (myK + nk), nk the second half of the input, myK the second half of the output on the same face
The boundary state is the oracle's: thermal_boundary (tests/function_restatement_more.py) evaluates the patch fields and the boundary
alphaEff with the oracle's bc_scalar / bc_vector / spalding_nut, as oracle.functions._boundary_state does (which keeps no nut_b).  Works
with complex W, so complex steps through it give derivatives in the states; `bcs` replaces the case's patch table for the
(central-difference) derivatives in a patch value - the oracle's patch table holds real numbers."""
import copy

import numpy as np

from function_restatement_more import thermal_boundary

MODES = ("default", "daCustom")


def selected_faces(case, patches):
    """Mesh face indices in output order: the sorted patches, each in face order."""
    by_name = {q.name: q for q in case.mesh.patches}
    return np.concatenate([np.arange(by_name[nm].start, by_name[nm].start + by_name[nm].size) for nm in sorted(patches)])


def size(case, patches):
    return 2 * selected_faces(case, patches).size


def delta_coeffs(g, bcell, mode):
    """(nBF,): the delta coefficient of every boundary face under a wallDistanceMethod."""
    if mode not in MODES:
        raise ValueError(f"wallDistanceMethod: {mode} not supported! Options are: default and daCustom.")
    if mode == "default":
        return g.bDeltaCoeffs
    d = g.Cf[g.nIF :] - g.C[bcell]
    return 1.0 / np.sqrt((d * d).sum(1))


def face_terms(case, g, W, mode="default", bcs=None, T_values=None):
    """(T of the owner cell, kappa / d) of every boundary face.  T_values: {patch: boundary values of T, one per face or one for all} on
    fixedValue patches (may be complex) - how a mixed patch is restated, see mixed_T_values."""
    if bcs is not None:
        case = copy.copy(case)
        case.bcs = bcs
    t = thermal_boundary(case, g, W, T_values)
    N = g.nC
    Tc = np.asarray(W)[4 * N : 5 * N][t["bcell"]]
    return Tc, case.thermo["Cp"] * t["alphaEff_b"] * delta_coeffs(g, t["bcell"], mode)


def output(case, g, W, patches, mode="default", bcs=None, T_values=None):
    Tc, kd = face_terms(case, g, W, mode, bcs, T_values)
    sel = selected_faces(case, patches) - g.nIF
    return np.concatenate([Tc[sel], kd[sel]])


def fraction(case, g, W, patches, nk, mode="default"):
    """valueFraction of the faces of the patches for the neighbour's kappa / d `nk` (one per face, may be complex)."""
    my_k = output(case, g, W, patches, mode)[selected_faces(case, patches).size :]
    return nk / (my_k + nk)


def dfraction_dnk(case, g, W, patches, nk, mode="default"):
    """d valueFraction / d nk = myK / (myK + nk)^2, face by face (the fraction of one face reads the nk of that face only)."""
    my_k = output(case, g, W, patches, mode)[selected_faces(case, patches).size :]
    return my_k / (my_k + nk) ** 2


def mixed_face(ref, f, xc, delta):
    """mixedFvPatchField with refGrad = 0, as x_b = vic x_c + vbc, snGrad = gic x_c + gbc: (x_b, vic, vbc, gic, gbc).  The operations and
    their order are those of oracle.residual.bc_scalar, which is this at f = 1 (fixedValue) and f = 0 (zeroGradient)."""
    one = np.ones_like(xc)
    vic = (1.0 - f) * one
    vbc = f * ref
    gic = (-f * delta) * one
    gbc = f * delta * ref
    return vic * xc + vbc, vic, vbc, gic, gbc


def as_fixed_value(case, patches, values=None):
    """The case with a fixedValue T on the patches.  A mixed patch with refGrad = 0 is a fixedValue patch whose face values are
    T_b = f ref + (1 - f) T_c: then x_b is T_b and snGrad = f delta (ref - T_c) = delta (T_b - T_c), the two things a patch field hands to
    the equations.  So the oracle and the restatements see a mixed patch as this case with T_values = mixed_T_values(...)."""
    from dafoam_amd.meshgen import BC_FIXED_VALUE

    c = copy.copy(case)
    c.bcs = copy.deepcopy(case.bcs)
    for k, nm in enumerate(patches):
        c.bcs[nm]["T"] = (BC_FIXED_VALUE, 0.0 if values is None else float(values[k]))
    c.mixed_T = {}
    return c


def mixed_T_values(case, g, W, mixed):
    """{patch: T_b per face} of the mixed patches {patch: (refValue, valueFraction)} at the states W (all three may be complex)."""
    N = g.nC
    T = np.asarray(W)[4 * N : 5 * N]
    out = {}
    for nm, (ref, f) in mixed.items():
        p = {q.name: q for q in case.mesh.patches}[nm]
        Tc = T[case.mesh.owner[p.start : p.start + p.size]]
        out[nm] = f * ref + (1.0 - f) * Tc
    return out


def simple_T_rows(case, g, W, T_values):
    """The T rows of the DASimpleFoam residual with the passive T field (reference DAResidualSimpleFoam.C:215-235: div(phi, T) -
    laplacian(alphaEff, T), bounded Gauss upwind / Gauss linear corrected, divided by the cell volume as the normalised TRes is), with the
    boundary values of T given face by face on fixedValue patches (T_values, may be complex).  Per boundary face the equation receives
    phi_b x_b - alphaEff_b |Sf| snGrad with snGrad = delta (x_b - T_c) - which holds for every patch-field type of this project - and x_b
    enters the Gauss gradient of the non-orthogonal correction.  T is passive: no other row reads it."""
    from oracle.residual import BCTable, Ops, bc_scalar, fv1_of, sadd

    N, F, nIF = g.nC, g.nF, g.nIF
    ops = Ops(g)
    oi, ni, bcell = ops.oi, ops.ni, ops.bc
    W = np.asarray(W).astype(np.complex128)
    Tt, nuT, phi = W[4 * N : 5 * N], W[5 * N : 6 * N], W[6 * N : 6 * N + F]
    phi_i, phi_b = phi[:nIF], phi[nIF:]
    Pr, Prt = case.thermo["Pr"], case.thermo["Prt"]
    bt = BCTable(case, g, ("T",))
    Tval = bt.val["T"].astype(np.complex128)
    for name, v in (T_values or {}).items():
        Tval[g.patch_slices()[name]] = v
    delta = g.bDeltaCoeffs
    Tb = bc_scalar(bt.code["T"], Tval, Tt[bcell], delta, phi_b)[0]
    gradT = ops.grad_scalar(Tt, Tb)
    aEff = case.nu / Pr + nuT * fv1_of(nuT / case.nu) / Prt
    ga_b = thermal_boundary(case, g, W)["alphaEff_b"] * g.bMagSf
    wu = (np.real(phi_i) >= 0).astype(float)
    lo = -wu * phi_i
    up = lo + phi_i
    d = sadd(oi, -lo, N) + sadd(ni, -up, N) - ops.surface_sum(phi_i, phi_b)
    ga = ops.interp(aEff) * g.magSf[:nIF]
    cd = ga * g.nonOrthDeltaCoeffs
    up, lo = up - cd, lo - cd
    d = d + sadd(oi, cd, N) + sadd(ni, cd, N)
    fc = ga * (g.nonOrthCorr * ops.interp(gradT)).sum(1)
    sT = sadd(oi, fc, N) - sadd(ni, fc, N)
    off = sadd(oi, up * Tt[ni], N) + sadd(ni, lo * Tt[oi], N)
    boundary = phi_b * Tb - ga_b * (delta * (Tb - Tt[bcell]))
    return (d * Tt + off - sT + sadd(bcell, boundary, N)) / g.V

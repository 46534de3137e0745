"""ctypes binding of include/dafoam_amd.h (thin; no compute here).

The library is built in-tree by __graft_entry__.build() (hipcc --offload-arch=gfx950).  Import fails
loudly if the shared object is missing: there is no Python/CPU fallback for the compute path.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .meshgen import BC_MIXED, BC_TRACTION, FoamCase

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DAFOAM_AMD_LIB") or os.path.join(_HERE, "lib", "libdafoam_amd.so")  # (override: tuning builds)

SOLVER_IDS = {"DASimpleFoam": 0, "DAScalarTransportFoam": 1, "DARhoSimpleFoam": 2, "DATurboFoam": 3, "DAHeatTransferFoam": 4,
              "DASolidDisplacementFoam": 5, "DAPimpleFoam": 6}
DDT_SCHEMES = {"Euler": 0, "backward": 1}  # system/fvSchemes ddtSchemes.default of DAPimpleFoam
PATCH_TYPES = {"patch": 0, "wall": 1, "symmetry": 2, "cyclic": 3}

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)
c_ll_p = C.POINTER(C.c_longlong)


class das_case_t(C.Structure):
    _fields_ = [
        ("solver", C.c_int),
        ("n_points", C.c_int),
        ("n_faces", C.c_int),
        ("n_internal_faces", C.c_int),
        ("n_cells", C.c_int),
        ("n_patches", C.c_int),
        ("points", c_double_p),
        ("face_ptr", c_int_p),
        ("face_pts", c_int_p),
        ("owner", c_int_p),
        ("neighbour", c_int_p),
        ("patch_start", c_int_p),
        ("patch_size", c_int_p),
        ("patch_type", c_int_p),
        ("bc_U_code", c_int_p),
        ("bc_U_val", c_double_p),
        ("bc_p_code", c_int_p),
        ("bc_p_val", c_double_p),
        ("bc_nuTilda_code", c_int_p),
        ("bc_nuTilda_val", c_double_p),
        ("bc_nut_code", c_int_p),
        ("bc_T_code", c_int_p),
        ("bc_T_val", c_double_p),
        ("nu", C.c_double),
        ("relax_U", C.c_double),
        ("relax_nuTilda", C.c_double),
        ("relax_T", C.c_double),
        ("DT", C.c_double),
        ("deltaT", C.c_double),
        ("y_wall", c_double_p),
        ("phi_frozen", c_double_p),
        ("T_old", c_double_p),
        ("Cp", C.c_double),
        ("molWeight", C.c_double),
        ("mu", C.c_double),
        ("Pr", C.c_double),
        ("Prt", C.c_double),
        ("mrf_active", C.c_int),
        ("mrf_omega", C.c_double * 3),
        ("mrf_origin", C.c_double * 3),
        ("patch_mrf_rotating", c_int_p),
        ("transonic", C.c_int),
        ("transonic_pc_option", C.c_int),
        ("simple_has_T", C.c_int),
        ("patch_neighbour", c_int_p),
        ("patch_rotation", c_double_p),
        ("transport_sutherland", C.c_int),
        ("sutherland_As", C.c_double),
        ("sutherland_Ts", C.c_double),
        ("beta_fi_nuTilda", c_double_p),
        ("bc_T_mixed_ref", c_double_p),
        ("bc_T_mixed_frac", c_double_p),
        ("n_kappa_coeffs", C.c_int),
        ("kappa_coeffs", C.c_double * 8),
        ("solid_rho", C.c_double),
        ("solid_E", C.c_double),
        ("solid_nu", C.c_double),
        ("plane_stress", C.c_int),
        ("bc_D_code", c_int_p),
        ("bc_D_val", c_double_p),
        ("bc_D_traction", c_double_p),
        ("bc_D_pressure", c_double_p),
        ("ddt_scheme", C.c_int),
    ]


class das_bilu_debug_t(C.Structure):
    """input of the test-only entries das_debug_bilu_* (include/dafoam_amd.h)"""
    _fields_ = [
        ("nNodes", C.c_int),
        ("nLevels", C.c_int),
        ("nMaps", C.c_int),
        ("fp32", C.c_int),
        ("transpose", C.c_int),
        ("n", C.c_longlong),
        ("An", C.c_longlong),
        ("nodeUnk", c_int_p),
        ("nodeOut", c_int_p),
        ("late", C.POINTER(C.c_ubyte)),
        ("bptr", c_ll_p),
        ("bdiag", c_ll_p),
        ("bcol", c_int_p),
        ("lvlPtr", c_int_p),
        ("unkNode", c_int_p),
        ("unkSlot", C.POINTER(C.c_ubyte)),
        ("rp", c_ll_p),
        ("ci", c_int_p),
        ("val", c_double_p),
        ("diagScale", C.c_double),
        ("shiftExLo", C.c_longlong),
        ("shiftExHi", C.c_longlong),
        ("shiftEnd", C.c_longlong),
    ]


class das_reg_spec_t(C.Structure):
    """one entry of the regressionModel option (include/dafoam_amd.h); reg_spec() fills it and keeps its arrays alive"""
    _fields_ = [
        ("model_type", C.c_char_p),
        ("n_inputs", C.c_int),
        ("input_names", C.POINTER(C.c_char_p)),
        ("input_shift", c_double_p),
        ("input_scale", c_double_p),
        ("output_name", C.c_char_p),
        ("n_hidden_layers", C.c_int),
        ("hidden_layer_neurons", c_int_p),
        ("activation_function", C.c_char_p),
        ("leaky_coeff", C.c_double),
        ("n_rbfs", C.c_int),
        ("output_shift", C.c_double),
        ("output_scale", C.c_double),
        ("output_upper_bound", C.c_double),
        ("output_lower_bound", C.c_double),
        ("default_output_value", C.c_double),
    ]


def reg_spec(e, with_names=True):
    """das_reg_spec_t of a model dictionary with the reference's keys (modelType, inputNames, inputShift, inputScale, outputName,
    hiddenLayerNeurons, activationFunction, leakyCoeff, nRBFs, outputShift, outputScale, outputUpperBound, outputLowerBound,
    defaultOutputValue).  The arrays live as long as the returned structure."""
    sp = das_reg_spec_t()
    names = [str(n).encode() for n in e.get("inputNames", [])]
    sp._names = (C.c_char_p * max(len(names), 1))(*names)
    sp._shift = np.ascontiguousarray(e.get("inputShift", []), dtype=np.float64)
    sp._scale = np.ascontiguousarray(e.get("inputScale", []), dtype=np.float64)
    sp._hidden = np.ascontiguousarray(e.get("hiddenLayerNeurons", []), dtype=np.int32)
    sp.model_type = str(e.get("modelType", "")).encode()
    sp.n_inputs = len(names) if with_names else int(e["nInputs"] if "nInputs" in e else sp._shift.size)
    sp.input_names = C.cast(sp._names, C.POINTER(C.c_char_p)) if with_names else None
    sp.input_shift = sp._shift.ctypes.data_as(c_double_p)
    sp.input_scale = sp._scale.ctypes.data_as(c_double_p)
    sp.output_name = str(e["outputName"]).encode() if "outputName" in e else None
    sp.n_hidden_layers = int(sp._hidden.size)
    sp.hidden_layer_neurons = sp._hidden.ctypes.data_as(c_int_p)
    sp.activation_function = str(e.get("activationFunction", "")).encode()
    sp.leaky_coeff = float(e.get("leakyCoeff", 0.0))
    sp.n_rbfs = int(e.get("nRBFs", 0))
    sp.output_shift = float(e.get("outputShift", 0.0))
    sp.output_scale = float(e.get("outputScale", 1.0))
    sp.output_upper_bound = float(e.get("outputUpperBound", 1e30))
    sp.output_lower_bound = float(e.get("outputLowerBound", -1e30))
    sp.default_output_value = float(e.get("defaultOutputValue", 1.0))
    return sp


def _dp(a):
    return a.ctypes.data_as(c_double_p) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(c_int_p) if a is not None else None


class CaseStruct:
    """Keeps the numpy buffers alive next to the ctypes struct."""

    def __init__(self, case: FoamCase):
        m = case.mesh
        k = self.keep = {}
        k["points"] = np.ascontiguousarray(m.points, dtype=np.float64)
        k["face_ptr"] = np.ascontiguousarray(m.face_ptr, dtype=np.int32)
        k["face_pts"] = np.ascontiguousarray(m.face_pts, dtype=np.int32)
        k["owner"] = np.ascontiguousarray(m.owner, dtype=np.int32)
        k["neighbour"] = np.ascontiguousarray(m.neighbour, dtype=np.int32)
        P = len(m.patches)
        k["patch_start"] = np.array([p.start for p in m.patches], dtype=np.int32)
        k["patch_size"] = np.array([p.size for p in m.patches], dtype=np.int32)
        k["patch_type"] = np.array([PATCH_TYPES[p.type] for p in m.patches], dtype=np.int32)

        def table(field, vec=False):
            code = np.zeros(P, dtype=np.int32)
            val = np.zeros((P, 3) if vec else P, dtype=np.float64)
            present = False
            for i, p in enumerate(m.patches):
                ent = case.bcs.get(p.name, {}).get(field)
                if ent is None:
                    code[i] = 1  # zeroGradient
                    continue
                present = True
                if ent[0] == BC_MIXED and field != "T":
                    raise DASError(f"patch {p.name}: the mixed patch field is built for T only, not for {field}")
                code[i] = ent[0]
                val[i] = ent[1]
            return (code, np.ascontiguousarray(val)) if present else (None, None)

        k["bc_U_code"], k["bc_U_val"] = table("U", True)
        k["bc_p_code"], k["bc_p_val"] = table("p")
        k["bc_nuTilda_code"], k["bc_nuTilda_val"] = table("nuTilda")
        k["bc_nut_code"], _ = table("nut")
        k["bc_T_code"], k["bc_T_val"] = table("T")
        k["bc_T_mixed_ref"] = k["bc_T_mixed_frac"] = None
        if k["bc_T_code"] is not None and (k["bc_T_code"] == BC_MIXED).any():
            # refValue / valueFraction of the mixed patches, one entry per boundary face of the mesh
            k["bc_T_mixed_ref"], k["bc_T_mixed_frac"] = np.zeros(m.n_faces - m.n_internal_faces), np.zeros(m.n_faces - m.n_internal_faces)
            for i, p in enumerate(m.patches):
                if k["bc_T_code"][i] != BC_MIXED:
                    continue
                if p.name not in getattr(case, "mixed_T", {}):
                    raise DASError(f"patch {p.name}: T is mixed but FoamCase.mixed_T has no refValue / valueFraction for it")
                if any(np.shape(a) != (p.size,) for a in case.mixed_T[p.name]):
                    raise DASError(f"patch {p.name}: the refValue / valueFraction of the mixed T need one entry per face ({p.size})")
                sl = slice(p.start - m.n_internal_faces, p.start - m.n_internal_faces + p.size)
                k["bc_T_mixed_ref"][sl], k["bc_T_mixed_frac"][sl] = case.mixed_T[p.name]
        k["y_wall"] = None if case.y_wall is None else np.ascontiguousarray(case.y_wall, dtype=np.float64)
        k["phi_frozen"] = None if case.phi is None else np.ascontiguousarray(case.phi, dtype=np.float64)
        k["T_old"] = None if case.T_old is None else np.ascontiguousarray(case.T_old, dtype=np.float64)
        bfi = getattr(case, "beta_fi", None)
        k["beta_fi"] = None if bfi is None else np.ascontiguousarray(bfi, dtype=np.float64)
        s = self.struct = das_case_t()
        s.solver = SOLVER_IDS[case.solver_name]
        s.n_points, s.n_faces, s.n_internal_faces, s.n_cells, s.n_patches = (
            m.n_points,
            m.n_faces,
            m.n_internal_faces,
            m.n_cells,
            P,
        )
        for name in ("points", "bc_U_val", "bc_p_val", "bc_nuTilda_val", "bc_T_val", "y_wall", "phi_frozen", "T_old", "bc_T_mixed_ref", "bc_T_mixed_frac"):
            setattr(s, name, _dp(k[name]))
        for name in (
            "face_ptr", "face_pts", "owner", "neighbour", "patch_start", "patch_size", "patch_type",
            "bc_U_code", "bc_p_code", "bc_nuTilda_code", "bc_nut_code", "bc_T_code",
        ):
            setattr(s, name, _ip(k[name]))
        s.nu = case.nu
        s.relax_U = case.relax.get("U", 0.7)
        s.relax_nuTilda = case.relax.get("nuTilda", 0.7)
        s.relax_T = case.relax.get("T", 1.0)
        s.DT = case.DT
        s.deltaT = case.deltaT
        th = getattr(case, "thermo", None) or {}
        s.Cp, s.molWeight, s.mu, s.Pr, s.Prt = (th.get("Cp", 1005.0), th.get("molWeight", 28.96), th.get("mu", 1.8e-5), th.get("Pr", 0.7), th.get("Prt", 1.0))
        s.beta_fi_nuTilda = _dp(k["beta_fi"])
        s.transport_sutherland = 1 if th.get("transport", "const") == "sutherland" else 0
        s.sutherland_As, s.sutherland_Ts = th.get("As", 1.4792e-06), th.get("Ts", 116.0)
        mrf = getattr(case, "mrf", None)
        s.mrf_active = 1 if mrf else 0
        if mrf:
            for i in range(3):
                s.mrf_omega[i] = float(mrf["omega"][i])
                s.mrf_origin[i] = float(mrf.get("origin", (0.0, 0.0, 0.0))[i])
            k["patch_mrf_rotating"] = np.array([0 if p.name in mrf.get("nonRotatingPatches", ()) else 1 for p in m.patches], dtype=np.int32)
            s.patch_mrf_rotating = _ip(k["patch_mrf_rotating"])
        s.transonic = 1 if getattr(case, "transonic", False) else 0
        s.transonic_pc_option = int(getattr(case, "transonic_pc_option", 1))
        if any(p.type == "cyclic" for p in m.patches):
            pnames = [p.name for p in m.patches]
            k["patch_neighbour"] = np.array([pnames.index(p.neighbour) if p.type == "cyclic" else -1 for p in m.patches], dtype=np.int32)
            s.patch_neighbour = _ip(k["patch_neighbour"])
            if any(getattr(p, "rotation", None) is not None for p in m.patches):
                k["patch_rotation"] = np.ascontiguousarray(
                    [np.asarray(p.rotation, dtype=np.float64).reshape(9) if getattr(p, "rotation", None) is not None else np.eye(3).reshape(9)
                     for p in m.patches], dtype=np.float64)
                s.patch_rotation = _dp(k["patch_rotation"])
        if case.solver_name == "DAHeatTransferFoam":
            # constant/solidProperties: `kappa` is one coefficient, `kappaCoeffs` the polynomial in T
            coeffs = [float(x) for x in np.atleast_1d(getattr(case, "kappa_coeffs", None) if getattr(case, "kappa_coeffs", None) is not None else [])]
            if not 1 <= len(coeffs) <= 8:
                raise DASError(f"DAHeatTransferFoam needs kappa or kappaCoeffs with 1 to 8 coefficients, not {len(coeffs)}")
            s.n_kappa_coeffs = len(coeffs)
            for i, x in enumerate(coeffs):
                s.kappa_coeffs[i] = x
        if case.solver_name == "DASolidDisplacementFoam":
            # constant/mechanicalProperties (rho, E, nu: type uniform; planeStress) and the patch fields of D
            mp = getattr(case, "mechanical", None) or {}
            uniform = {}
            for nm in ("rho", "E", "nu"):
                ent = mp.get(nm)
                if isinstance(ent, dict):
                    if ent.get("type", "uniform") != "uniform":
                        raise DASError(f"DASolidDisplacementFoam: mechanicalProperties {nm} of type {ent.get('type')} is not built (only uniform is)")
                    ent = ent.get("value")
                if ent is None:
                    raise DASError(f"DASolidDisplacementFoam needs mechanicalProperties {nm} (a number, or type uniform with a value)")
                uniform[nm] = float(ent)
            rho, E, nu = uniform["rho"], uniform["E"], uniform["nu"]
            if not rho > 0.0:
                raise DASError(f"DASolidDisplacementFoam needs a positive rho, not {rho}")
            if not E > 0.0:
                raise DASError(f"DASolidDisplacementFoam needs a positive E, not {E}")
            if not -1.0 < nu < 0.5:
                raise DASError(f"DASolidDisplacementFoam needs nu inside (-1, 0.5), not {nu}")
            s.solid_rho, s.solid_E, s.solid_nu, s.plane_stress = rho, E, nu, 1 if mp.get("planeStress", False) else 0
            code = np.ones(P, dtype=np.int32)
            val, trac, pres = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P)
            for i, p in enumerate(m.patches):
                if p.type == "cyclic":
                    raise DASError(f"DASolidDisplacementFoam: patch {p.name} is cyclic - cyclic patches are not built for D")
                ent = case.bcs.get(p.name, {}).get("D")
                if ent is None:
                    continue
                code[i] = ent[0]
                if ent[0] == BC_TRACTION:
                    trac[i], pres[i] = ent[1], ent[2]
                elif ent[0] in (0, 1, 3):
                    val[i] = ent[1] if ent[0] == 0 else 0.0
                else:
                    raise DASError(f"DASolidDisplacementFoam: patch {p.name}: D is fixedValue, zeroGradient, symmetry or tractionDisplacement, not code {ent[0]}")
            k["bc_D_code"], k["bc_D_val"], k["bc_D_traction"], k["bc_D_pressure"] = code, val, trac, pres
            s.bc_D_code = _ip(code)
            s.bc_D_val, s.bc_D_traction, s.bc_D_pressure = _dp(val), _dp(trac), _dp(pres)
        s.simple_has_T = 1 if (case.solver_name in ("DASimpleFoam", "DAPimpleFoam") and getattr(case, "has_T", False)) else 0
        if case.solver_name == "DAPimpleFoam":
            scheme = getattr(case, "ddt_scheme", "Euler")
            if scheme not in DDT_SCHEMES:  # DASolver::getDdtSchemeOrder (DASolver.H:254-279)
                raise DASError(f"ddtScheme {scheme} not supported! Options: steadyState, Euler, or backward"
                               + (" (DAPimpleFoam is unsteady: Euler or backward)" if scheme == "steadyState" else ""))
            if getattr(case, "simple_consistent", False):
                raise DASError("DAPimpleFoam: simple_consistent is not built")
            s.ddt_scheme = DDT_SCHEMES[scheme]

    def byref(self):
        return C.byref(self.struct)


# every symbol include/dafoam_amd.h declares, with its signature
_VP = C.c_void_p
_SIGS = {
    "das_last_error": (C.c_char_p, []),
    "das_version": (C.c_int, []),
    "das_device_count": (C.c_int, []),
    "das_create": (_VP, [C.POINTER(das_case_t)]),
    "das_destroy": (None, [_VP]),
    "das_set_option_double": (C.c_int, [_VP, C.c_char_p, C.c_double]),
    "das_set_option_int": (C.c_int, [_VP, C.c_char_p, C.c_longlong]),
    "das_set_option_str": (C.c_int, [_VP, C.c_char_p, C.c_char_p]),
    "das_get_option_double": (C.c_int, [_VP, C.c_char_p, c_double_p]),
    "das_get_option_string": (C.c_int, [_VP, C.c_char_p, C.c_char_p, C.c_int]),
    "das_init_solver": (C.c_int, [_VP, C.c_int]),
    "das_get_n_local_adjoint_states": (C.c_longlong, [_VP]),
    "das_get_n_local_cells": (C.c_longlong, [_VP]),
    "das_get_n_global_cells": (C.c_longlong, [_VP]),
    "das_set_n_global_cells": (C.c_int, [_VP, C.c_longlong]),
    "das_get_n_local_points": (C.c_longlong, [_VP]),
    "das_get_n_local_faces": (C.c_longlong, [_VP]),
    "das_get_geometry": (C.c_int, [_VP] + [c_double_p] * 8),
    "das_update_of_fields": (C.c_int, [_VP, c_double_p]),
    "das_get_of_fields": (C.c_int, [_VP, c_double_p]),
    "das_get_residuals": (C.c_int, [_VP, c_double_p]),
    "das_calc_residuals": (C.c_int, [_VP, C.c_int, c_double_p]),
    "das_solve_primal": (C.c_int, [_VP, C.c_int, C.c_double, C.c_double, c_double_p, c_double_p, C.c_int]),
    "das_simple_iteration": (C.c_int, [_VP, C.c_int, C.c_double, C.c_double, C.c_int, c_double_p]),
    "das_run_coloring": (C.c_int, [_VP]),
    "das_update_of_mesh": (C.c_int, [_VP, c_double_p]),
    "das_get_of_mesh_points": (C.c_int, [_VP, c_double_p]),
    "das_set_coloring": (C.c_int, [_VP, c_int_p]),
    "das_debug_factor_block": (C.c_int, [C.c_int, c_ll_p, c_int_p, c_double_p, C.c_int, c_double_p, c_ll_p, c_int_p, c_int_p]),
    "das_debug_rcb": (C.c_int, [C.c_int, c_double_p, C.c_int, C.c_int, c_int_p]),
    "das_get_n_colors": (C.c_int, [_VP, C.c_int]),
    "das_get_con_nnz": (C.c_longlong, [_VP, C.c_int]),
    "das_get_con": (C.c_int, [_VP, C.c_int, c_ll_p, c_int_p]),
    "das_get_colors": (C.c_int, [_VP, C.c_int, c_int_p]),
    "das_calc_drdwt": (C.c_int, [_VP, C.c_int, C.c_int, C.POINTER(_VP)]),
    "das_mat_rows": (C.c_longlong, [_VP]),
    "das_mat_nnz": (C.c_longlong, [_VP]),
    "das_mat_export": (C.c_int, [_VP, c_ll_p, c_int_p, c_double_p]),
    "das_mat_mult": (C.c_int, [_VP, c_double_p, c_double_p]),
    "das_mat_create_from_csr": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, c_double_p, C.POINTER(_VP)]),
    "das_mat_destroy": (None, [_VP]),
    "das_initialize_drdwt_matrix_free": (C.c_int, [_VP]),
    "das_destroy_drdwt_matrix_free": (C.c_int, [_VP]),
    "das_op_nnz": (C.c_longlong, [_VP]),
    "das_op_format_bytes": (C.c_longlong, [_VP]),
    "das_op_export": (C.c_int, [_VP, c_ll_p, c_int_p, c_double_p]),
    "das_calc_drdwold_t_psi": (C.c_int, [_VP, C.c_int, c_double_p, c_double_p]),
    "das_set_old_time_fields": (C.c_int, [_VP, c_double_p, c_double_p]),
    "das_set_old_time_states": (C.c_int, [_VP, c_double_p, c_double_p, C.c_int]),
    "das_set_time_index": (C.c_int, [_VP, C.c_int]),
    "das_calc_jac_vec_product": (C.c_int, [_VP, c_double_p, c_double_p]),
    "das_set_patch_value": (C.c_int, [_VP, c_int_p, C.c_int, C.c_char_p, c_double_p]),
    "das_get_patch_value": (C.c_int, [_VP, C.c_int, C.c_char_p, c_double_p]),
    "das_set_field": (C.c_int, [_VP, C.c_char_p, c_double_p]),
    "das_get_field": (C.c_int, [_VP, C.c_char_p, c_double_p]),
    "das_calc_dfield_product": (C.c_int, [_VP, C.c_char_p, C.c_char_p, C.c_char_p, c_double_p, c_double_p]),
    "das_calc_dvolcoord_product": (C.c_int, [_VP, C.c_char_p, C.c_char_p, c_double_p, c_double_p, c_double_p]),
    "das_point_influence_build": (C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "das_point_influence_get": (C.c_int, [_VP, c_int_p, c_ll_p, c_int_p, c_double_p]),
    "das_debug_device_geometry": (C.c_int, [_VP, c_double_p, c_double_p, c_double_p]),
    "das_debug_strength_aggregates": (C.c_int, [_VP, C.c_int, c_int_p, C.POINTER(C.c_int)]),
    "das_calc_dbc_product": (C.c_int, [_VP, c_int_p, C.c_int, C.c_char_p, c_double_p, C.c_char_p, C.c_char_p, c_double_p, c_double_p]),
    "das_define_force_function": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, c_double_p, C.c_double]),
    "das_define_face_function": (C.c_int, [_VP, C.c_char_p, C.c_char_p, c_int_p, c_int_p, C.c_int, c_double_p, c_double_p, C.c_double, C.c_double]),
    "das_define_face_function_ex": (C.c_int, [_VP, C.c_char_p, C.c_char_p, c_int_p, c_int_p, C.c_int, c_double_p, c_double_p, C.c_double, C.c_double, C.c_int, C.c_double]),
    "das_define_location_function": (C.c_int, [_VP, C.c_char_p, C.c_char_p, c_int_p, C.c_int, c_double_p, c_double_p, C.c_double, C.c_int, C.c_double]),
    "das_define_patch_field_function": (C.c_int, [_VP, C.c_char_p, C.c_char_p, c_int_p, C.c_int, C.c_char_p, c_int_p, C.c_int, c_double_p, C.c_int, C.c_double, C.c_double]),
    "das_define_cell_function": (C.c_int, [_VP, C.c_char_p, C.c_char_p, c_int_p, C.c_int, C.c_char_p, c_int_p, C.c_int, c_double_p, C.c_int, C.c_double, C.c_double]),
    "das_define_von_mises_function": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double]),
    "das_define_mesh_quality_function": (C.c_int, [_VP, C.c_char_p, C.c_char_p, C.c_double, C.c_int, C.c_double]),
    "das_define_residual_norm_function": (C.c_int, [_VP, C.c_char_p, C.POINTER(C.c_char_p), c_double_p, C.c_int, C.c_char_p, C.c_int, C.c_double]),
    "das_calc_function": (C.c_int, [_VP, C.c_char_p, c_double_p]),
    "das_define_force_coupling": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, C.c_double]),
    "das_calc_force_coupling": (C.c_int, [_VP, C.c_char_p, c_double_p, C.c_int]),
    "das_define_thermal_coupling": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, C.c_int]),
    "das_calc_thermal_coupling": (C.c_int, [_VP, C.c_char_p, c_double_p, C.c_int]),
    "das_define_thermal_coupling_input": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, C.c_int]),
    "das_set_thermal_coupling_input": (C.c_int, [_VP, C.c_char_p, c_double_p, C.c_int]),
    "das_get_patch_mixed": (C.c_int, [_VP, C.c_int, c_double_p, c_double_p]),
    "das_calc_dthermal_coupling_product": (C.c_int, [_VP, C.c_char_p, C.c_char_p, C.c_char_p, c_double_p, c_double_p, C.c_int]),
    "das_define_heat_source": (C.c_int, [_VP, C.c_char_p, C.c_char_p, c_double_p, C.c_double, C.c_int]),
    "das_set_heat_source_pars": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, c_double_p]),
    "das_get_heat_source_info": (C.c_int, [_VP, C.c_char_p, c_double_p, c_double_p, c_double_p, c_int_p]),
    "das_get_heat_source_cells": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int]),
    "das_get_fv_source": (C.c_int, [_VP, c_double_p]),
    "das_calc_dfvsourcepar_product": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, C.c_char_p, C.c_char_p, c_double_p, c_double_p]),
    "das_define_actuator_disk": (C.c_int, [_VP, C.c_char_p, C.c_char_p, c_double_p, C.c_char_p, C.c_double, C.c_int]),
    "das_set_actuator_disk_pars": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, c_double_p]),
    "das_get_actuator_disk_info": (C.c_int, [_VP, C.c_char_p, c_double_p, c_double_p, c_int_p]),
    "das_get_actuator_disk_cells": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int]),
    "das_get_fv_source_vector": (C.c_int, [_VP, c_double_p]),
    "das_calc_dactuatordiskpar_product": (C.c_int, [_VP, C.c_char_p, c_int_p, C.c_int, C.c_char_p, C.c_char_p, c_double_p, c_double_p]),
    "das_define_regression_model": (C.c_int, [_VP, C.c_char_p, C.POINTER(das_reg_spec_t)]),
    "das_get_regression_n_parameters": (C.c_int, [_VP, C.c_char_p]),
    "das_set_regression_parameters": (C.c_int, [_VP, C.c_char_p, c_double_p, C.c_int]),
    "das_get_regression_parameters": (C.c_int, [_VP, C.c_char_p, c_double_p, C.c_int]),
    "das_get_regression_model_info": (C.c_int, [_VP, C.c_char_p, c_int_p, c_int_p, c_int_p]),
    "das_get_regression_features": (C.c_int, [_VP, C.c_char_p, c_double_p, c_double_p, c_ll_p]),
    "das_calc_dregressionpar_product": (C.c_int, [_VP, C.c_char_p, C.c_char_p, C.c_char_p, c_double_p, c_double_p]),
    "das_debug_reg_forward": (C.c_int, [C.POINTER(das_reg_spec_t), c_double_p, C.c_int, C.c_int, c_double_p, c_double_p, C.POINTER(C.c_ubyte)]),
    "das_debug_reg_backward": (C.c_int, [C.POINTER(das_reg_spec_t), c_double_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    "das_get_input_size": (C.c_int, [_VP, C.c_char_p, C.c_char_p]),
    "das_get_output_size": (C.c_int, [_VP, C.c_char_p, C.c_char_p]),
    "das_calc_jac_t_vec_product": (
        C.c_int,
        [_VP, C.c_char_p, C.c_char_p, c_double_p, C.c_char_p, C.c_char_p, c_double_p, c_double_p],
    ),
    "das_drdwt_mult_device": (C.c_int, [_VP, _VP, _VP]),
    "das_create_ml_rksp_matrix_free": (C.c_int, [_VP, _VP, C.POINTER(_VP)]),
    "das_solve_linear_eqn": (C.c_int, [_VP, _VP, c_double_p, c_double_p]),
    "das_solve_linear_eqn_block": (C.c_int, [_VP, _VP, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    "das_ksp_apply_pc": (C.c_int, [_VP, _VP, c_double_p, c_double_p]),
    "das_ksp_get_n_blocks": (C.c_int, [_VP]),
    "das_ksp_get_factor_nnz": (C.c_longlong, [_VP]),
    "das_ksp_get_n_ext": (C.c_longlong, [_VP]),
    "das_ksp_get_blocks": (C.c_int, [_VP, c_int_p, c_ll_p]),
    "das_pc_structure_build": (C.c_int, [_VP, c_int_p, c_ll_p, c_int_p, c_int_p]),
    "das_pc_structure_get": (C.c_int, [_VP, c_int_p, c_ll_p, c_int_p, c_int_p, c_int_p]),
    "das_ksp_get_pc_structure_sizes": (C.c_int, [_VP, c_int_p, c_ll_p, c_int_p]),
    "das_ksp_get_pc_structure": (C.c_int, [_VP, c_int_p, c_ll_p, c_int_p, c_int_p, c_int_p]),
    "das_ksp_get_info": (C.c_int, [_VP, c_int_p, c_double_p, c_double_p, c_double_p]),
    "das_ksp_get_history": (C.c_int, [_VP, c_double_p, C.c_int]),
    "das_ksp_get_cycle_lengths": (C.c_int, [_VP, c_int_p, C.c_int]),
    "das_ksp_get_basis_info": (C.c_int, [_VP, c_int_p, c_double_p, c_double_p]),
    "das_ksp_get_n_refine": (C.c_int, [_VP]),
    "das_set_dense_eig_callback": (C.c_int, [_VP]),
    "das_debug_gmres_dr_host": (C.c_int, [C.c_longlong, _VP, _VP, _VP, c_double_p, c_double_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_longlong, c_double_p, C.c_int,
                                          c_double_p, c_double_p]),
    "das_ksp_get_idr_info": (C.c_int, [_VP, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p, c_double_p]),
    "das_ksp_get_poly_info": (C.c_int, [_VP, c_int_p, c_int_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), c_int_p, c_int_p, c_int_p, c_double_p,
                                        c_int_p, c_double_p, c_double_p]),
    # test-only entries of amd.polyDegree (tests/test_poly_host_cpu.py, tests/test_gpu_poly_kernels.py, tests/test_gpu_poly_gmres.py)
    "das_debug_poly_roots": (C.c_int, [C.c_int, c_double_p, c_double_p, c_double_p]),
    "das_debug_poly_apply_host": (C.c_int, [C.c_longlong, _VP, _VP, _VP, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    "das_debug_poly_step": (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_longlong, C.c_longlong, c_double_p, c_double_p, c_double_p,
                                      c_double_p, c_double_p]),
    "das_debug_ksp_poly_apply": (C.c_int, [_VP, _VP, c_double_p, c_double_p]),
    "das_debug_idrs_host": (C.c_int, [C.c_longlong, _VP, _VP, _VP, c_double_p, c_double_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_longlong, c_double_p, C.c_int,
                                      c_double_p, c_double_p]),
    "das_debug_idr_cycle_host": (C.c_int, [C.c_longlong, _VP, _VP, _VP, c_double_p, c_double_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    # test-only entries (tests/test_gpu_idr_kernels.py): the IDR(s) kernels on caller data, never called by the bindings
    "das_debug_idr_shadow": (C.c_int, [C.c_longlong, C.c_int, C.c_longlong, C.c_int, C.c_int, c_double_p]),
    "das_debug_idr_combine": (C.c_int, [C.c_longlong, C.c_int, C.c_double, c_double_p, c_double_p, C.c_longlong, C.c_longlong, c_double_p, C.c_longlong, c_double_p,
                                        C.c_longlong]),
    "das_debug_idr_biortho_step": (C.c_int, [C.c_longlong, C.c_int, c_double_p, c_double_p, C.c_longlong, C.c_longlong, c_double_p, c_double_p, c_double_p, C.c_longlong,
                                             c_double_p]),
    "das_debug_idr_smooth_step": (C.c_int, [C.c_longlong, C.c_int, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, C.c_longlong, c_double_p, C.c_longlong,
                                            C.c_longlong, c_double_p]),
    "das_debug_gmres_dr_restart": (C.c_int, [C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "das_debug_block_chol": (C.c_int, [C.c_int, c_double_p, c_double_p, c_double_p]),
    "das_debug_block_lsq": (C.c_int, [C.c_int, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "das_ksp_get_status": (C.c_int, [_VP, c_int_p, c_int_p, c_int_p, c_int_p]),
    "das_ksp_get_pc_stability": (C.c_int, [_VP, C.POINTER(C.c_double), c_int_p]),
    "das_ksp_get_pc_subdomains": (C.c_int, [_VP, c_int_p, c_double_p]),
    "das_ksp_get_pc_node_out": (C.c_int, [_VP, c_int_p]),
    "das_mesh_metrics": (C.c_int, [C.c_int, c_double_p, C.c_int, C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "das_ksp_get_coarse": (C.c_int, [_VP, c_int_p]),
    "das_ksp_coarse_sparse_az_active": (C.c_int, [_VP]),
    "das_ksp_set_global_coarse": (C.c_int, [_VP, _VP, C.c_int, C.c_int, c_int_p]),
    "das_ksp_run_fixed_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int]),
    "das_ksp_begin_device": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int]),
    "das_ksp_advance": (C.c_int, [_VP, _VP, C.c_int]),
    "das_ksp_end": (C.c_int, [_VP, _VP]),
    "das_ksp_destroy": (None, [_VP]),
    "das_set_owned_mask": (C.c_int, [_VP, C.POINTER(C.c_ubyte)]),
    "das_comm_load_rccl": (C.c_int, []),
    "das_comm_unique_id": (C.c_int, [C.c_char_p]),
    "das_comm_init_rccl": (C.c_int, [_VP, C.c_int, C.c_int, C.c_char_p]),
    "das_comm_set_halo": (C.c_int, [_VP, C.c_int, c_int_p, c_ll_p, c_int_p, c_ll_p, c_int_p, C.c_longlong, c_int_p]),
    "das_set_exchange_cb": (C.c_int, [_VP, _VP, _VP]),
    "das_set_pc_overlap": (C.c_int, [_VP, C.POINTER(C.c_ubyte), C.c_int, c_ll_p, c_int_p, c_ll_p, c_int_p]),
    "das_set_gather_cb": (C.c_int, [_VP, _VP, _VP]),
    "das_comm_is_native": (C.c_int, [_VP]),
    "das_comm_reset": (C.c_int, [_VP]),
    "das_set_comm": (C.c_int, [_VP, _VP, _VP, _VP]),
    "das_set_stream": (C.c_int, [_VP, _VP]),
    "das_get_elapsed_clock_time": (C.c_double, [_VP]),
    "das_get_elapsed_cpu_time": (C.c_double, [_VP]),
    "das_timer_avg_ms": (C.c_double, [_VP, C.c_char_p]),
    "das_debug_orth_bench": (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "das_debug_orth_bench_split": (C.c_int, [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "das_debug_set_orth_wide": (C.c_int, [C.c_int, C.POINTER(C.c_int)]),
    "das_debug_krylov_wide_eligible": (C.c_int, [C.c_longlong, C.c_int, C.c_longlong, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    # test-only entries (tests/test_gpu_krylov_kernels.py): the Krylov kernels on caller data, never called by the bindings
    "das_debug_krylov_dots2": (C.c_int, [C.c_longlong, C.c_int, C.c_int, _VP, C.c_longlong, c_double_p, c_double_p]),
    "das_debug_krylov_dcgs2_update": (C.c_int, [C.c_longlong, C.c_int, C.c_int, _VP, C.c_longlong, C.c_int, c_double_p, C.c_double, C.c_double, c_double_p]),
    "das_debug_krylov_multidot": (C.c_int, [C.c_longlong, C.c_int, C.c_int, _VP, C.c_longlong, c_double_p, c_double_p]),
    "das_debug_krylov_multiaxpy": (C.c_int, [C.c_longlong, C.c_int, C.c_int, _VP, C.c_longlong, c_double_p, C.c_int, _VP, C.c_longlong]),
    "das_debug_krylov_lincomb": (C.c_int, [C.c_longlong, C.c_int, C.c_int, _VP, C.c_longlong, c_double_p, c_double_p, C.c_longlong]),
    "das_debug_krylov_scale_to": (C.c_int, [C.c_longlong, C.c_double, C.c_int, _VP, _VP, C.c_longlong]),
    "das_debug_krylov_block_tn": (C.c_int, [C.c_longlong, C.c_int, C.c_int, c_double_p, C.c_longlong, C.c_longlong, c_double_p, C.c_longlong, c_double_p]),
    "das_debug_krylov_block_nn_sub": (C.c_int, [C.c_longlong, C.c_int, C.c_int, c_double_p, C.c_longlong, c_double_p, c_double_p, C.c_longlong]),
    "das_debug_krylov_block_right_mult": (C.c_int, [C.c_longlong, C.c_int, c_double_p, C.c_longlong, c_double_p]),
    "das_debug_krylov_block_lincomb": (C.c_int, [C.c_longlong, C.c_int, C.c_int, c_double_p, C.c_longlong, c_double_p, c_double_p, C.c_longlong]),
    "das_debug_krylov_block_spmm": (C.c_int, [C.c_longlong, C.c_int, c_ll_p, c_int_p, c_double_p, c_double_p, C.c_longlong, c_double_p, C.c_longlong]),
    # test-only entries (tests/test_gpu_bilu_kernels.py): the node-block ILU(0) on a caller-made structure, never called by the bindings
    "das_debug_bilu_factor": (C.c_int, [C.POINTER(das_bilu_debug_t), c_ll_p, c_ll_p, c_int_p, c_int_p, _VP, _VP, c_double_p, c_int_p]),
    "das_debug_bilu_apply": (C.c_int, [C.POINTER(das_bilu_debug_t), C.c_int, C.c_longlong, c_double_p, c_double_p, C.c_int, c_double_p, c_double_p, c_int_p, c_int_p]),
    # test-only entries (tests/test_gpu_graph_kernels.py, tests/test_gpu_opmat_kernels.py): graph set-up, filter, packed operator and
    # ghost-row product on caller-made structures, never called by the bindings
    "das_debug_graph_scan": (C.c_int, [C.c_longlong, c_int_p, c_ll_p, c_ll_p]),
    "das_debug_graph_transpose": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, c_ll_p, c_int_p]),
    "das_debug_graph_nets": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, C.c_longlong, c_ll_p, c_ll_p, c_int_p, c_int_p, C.POINTER(C.c_ubyte), c_ll_p]),
    "das_debug_graph_rows_gather": (C.c_int, [C.c_longlong, c_ll_p, C.c_longlong, c_ll_p, c_int_p, c_ll_p, c_int_p, C.c_longlong]),
    "das_debug_compact": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, c_double_p, C.c_double, C.c_int, C.POINTER(C.c_ubyte), c_ll_p, c_int_p, c_double_p, c_ll_p]),
    "das_debug_vecpack": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, c_double_p, C.c_longlong, C.c_longlong, c_int_p, c_ll_p, C.POINTER(C.c_ubyte), C.c_longlong, c_ll_p,
                                    c_double_p, c_double_p, C.c_longlong]),
    "das_debug_spmv_rows": (C.c_int, [C.c_longlong, c_int_p, C.c_longlong, c_ll_p, c_int_p, c_double_p, c_double_p, c_double_p, C.c_longlong]),
    # test-only entries (tests/test_gpu_color_kernels.py): the colouring kernels on a caller-made pattern and kept-row list, never called
    # by the bindings
    "das_debug_color_firstfit": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, C.c_longlong, c_ll_p, c_int_p, C.c_longlong, c_int_p, c_int_p]),
    "das_debug_color_speculative": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, C.c_longlong, c_ll_p, C.c_int, c_int_p, C.c_longlong, c_int_p, c_int_p, c_int_p,
                                              c_int_p]),
    "das_debug_color_spec_round": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, C.c_longlong, c_ll_p, c_int_p, C.c_int, C.c_int, C.c_int, c_int_p, C.POINTER(C.c_ubyte),
                                             c_int_p, C.c_longlong, C.POINTER(C.c_ulonglong), C.c_longlong, C.POINTER(C.c_uint), c_int_p]),
    "das_debug_color_check": (C.c_int, [C.c_longlong, c_ll_p, c_int_p, C.c_longlong, c_ll_p, c_int_p, C.c_int, c_int_p]),
    # test-only entries (tests/test_gpu_reduce_kernels.py): the reductions of the objective functions and the two gathers on caller-made
    # arrays, never called by the bindings
    "das_debug_reduce_ks": (C.c_int, [C.c_longlong, c_double_p, C.c_double, C.c_double, c_double_p, C.c_longlong, c_double_p, c_double_p, C.c_longlong, c_double_p,
                                      C.c_longlong, c_int_p]),
    "das_debug_reduce_group_sum": (C.c_int, [C.c_longlong, C.POINTER(C.c_ubyte), c_double_p, c_double_p, C.c_longlong]),
    "das_debug_reduce_tangent_dot": (C.c_int, [C.c_longlong, c_double_p, c_double_p, c_double_p, C.c_longlong, c_double_p, C.c_longlong, c_int_p]),
    "das_debug_reduce_ad_dot": (C.c_int, [C.c_longlong, c_double_p, c_double_p, c_double_p, C.c_longlong, c_double_p, C.c_longlong, c_int_p]),
    "das_debug_reduce_sv_dot": (C.c_int, [C.c_longlong, c_double_p, c_double_p, c_double_p, C.c_longlong, c_double_p, C.c_longlong, c_int_p]),
    "das_debug_reduce_cellfn": (C.c_int, [C.c_longlong, c_int_p, c_ll_p, c_double_p, C.c_int, C.c_int, C.c_longlong, c_double_p, C.c_longlong, c_double_p, C.c_double,
                                          c_double_p, C.c_longlong, c_double_p, C.c_longlong, c_double_p, C.c_double, c_double_p, C.c_longlong, c_int_p]),
    "das_debug_reduce_rn": (C.c_int, [C.c_longlong, C.c_int, c_ll_p, c_int_p, c_double_p, C.c_longlong, C.c_longlong, C.c_longlong, C.c_int, c_double_p, c_double_p,
                                      C.c_longlong, c_double_p, C.c_longlong, c_double_p, C.c_longlong, C.c_double, C.c_double, c_double_p, C.c_longlong, c_int_p]),
    "das_debug_reduce_hs_sum": (C.c_int, [C.c_int, C.c_int, c_double_p, C.POINTER(C.c_ubyte), c_double_p, c_double_p, C.c_int, C.c_double, c_double_p, c_double_p,
                                          C.c_longlong, c_double_p, C.c_longlong, c_int_p]),
    "das_debug_reduce_final": (C.c_int, [C.c_int, C.c_int, C.c_int, c_double_p, C.c_longlong, c_double_p, C.c_longlong]),
    "das_debug_reduce_owner_gather": (C.c_int, [C.c_int, c_int_p, c_int_p, C.c_longlong, c_double_p, c_double_p, C.c_longlong]),
    "das_debug_reduce_vm_gather": (C.c_int, [C.c_int, C.c_int, c_int_p, c_int_p, c_int_p, c_int_p, C.c_int, c_double_p, C.c_double, c_double_p, C.c_longlong]),
    # test-only entries (tests/test_gpu_coarse_kernels.py): the coarse space of the two-level preconditioner on caller-made structures,
    # never called by the bindings
    "das_debug_coarse_assemble": (C.c_int, [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, c_ll_p, c_int_p, c_double_p, c_int_p, c_int_p, C.c_int, C.c_double,
                                            c_double_p]),
    "das_debug_coarse_invert": (C.c_int, [C.c_int, c_double_p, c_double_p, c_int_p]),
    "das_debug_coarse_correct": (C.c_int, [C.c_int, C.c_longlong, C.c_longlong, C.c_longlong, c_int_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                           C.c_longlong, C.c_int]),
    "das_debug_coarse_az": (C.c_int, [C.c_int, C.c_longlong, c_ll_p, c_int_p, c_double_p, C.c_longlong, C.c_longlong, c_int_p, c_int_p, c_ll_p, c_int_p, c_double_p,
                                      C.c_longlong, c_ll_p, c_int_p, c_double_p, c_double_p, c_double_p, C.c_longlong]),
    "das_timer_count": (C.c_longlong, [_VP, C.c_char_p]),
    "das_timer_reset": (None, [_VP]),
    "das_timer_enable": (None, [_VP, C.c_int]),
}

_lib = None


def declared_symbols():
    return sorted(_SIGS)


def lib():
    """Load libdafoam_amd.so (built in-tree); raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
                "dafoam_amd has no CPU fallback."
            )
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
        _install_dense_eig(L)
    return _lib


_DENSE_EIG_FN = C.CFUNCTYPE(C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p)
_dense_eig_keepalive = []


def _install_dense_eig(L):
    """The dense nonsymmetric eigen-solver of the deflated restart (amd.gmresDeflation): numpy.linalg.eig behind the callback the
    C-ABI asks for (the library itself carries no LAPACK; a C host would pass LAPACK's dgeev the same way)."""

    def eig(m, A, wr, wi, vr, vi):
        try:
            G = np.ctypeslib.as_array(A, shape=(m * m,)).reshape(m, m)
            w, v = np.linalg.eig(G)
            np.ctypeslib.as_array(wr, shape=(m,))[:] = w.real
            np.ctypeslib.as_array(wi, shape=(m,))[:] = w.imag
            np.ctypeslib.as_array(vr, shape=(m * m,))[:] = np.ascontiguousarray(v.T.real).ravel()
            np.ctypeslib.as_array(vi, shape=(m * m,))[:] = np.ascontiguousarray(v.T.imag).ravel()
            return 0
        except Exception:  # noqa: BLE001 - never raise through the C boundary
            return 1

    cb = _DENSE_EIG_FN(eig)
    _dense_eig_keepalive.append(cb)
    L.das_set_dense_eig_callback(C.cast(cb, C.c_void_p))


class DASError(RuntimeError):
    pass


def check(rc):
    if rc < 0:
        raise DASError(f"dafoam_amd error {rc}: {lib().das_last_error().decode()}")
    return rc


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)

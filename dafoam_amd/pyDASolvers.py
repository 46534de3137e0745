"""Host-side mirror of the reference's Cython boundary class ``pyDASolvers``
(reference src/pyDASolvers/pyDASolvers.pyx:117-482) for the adjoint hot path.

Same method names, argument meaning and error behaviour as the reference for the hot-path subset
(SURVEY.md section 8b); every method forwards to the C-ABI of include/dafoam_amd.h, which runs on the GPU.
PETSc is not part of this stack (north star: "no PETSc"): the ``Mat``/``Vec``/``KSP`` objects the reference's
callers create with petsc4py (reference dafoam/mphys/mphys_dafoam.py:468-475,519-529, dafoam/pyDAFoam.py:2132-2199)
are replaced by the light stand-ins below that expose the handful of methods those callers use.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from ._capi import CaseStruct, check, dptr, lib
from .meshgen import BC_MIXED, FoamCase


# ----------------------------------------------------------------------------- PETSc stand-ins
class Vec:
    """Stand-in for petsc4py.PETSc.Vec as used by pyDAFoam.array2Vec/vec2Array (pyDAFoam.py:2167-2199)."""

    def __init__(self, n=0):
        self.array = np.zeros(int(n), dtype=np.float64)

    @classmethod
    def createSeq(cls, n, bsize=1, comm=None):
        return cls(n)

    def setSizes(self, size, bsize=1):
        n = size[0] if isinstance(size, (tuple, list)) else size
        self.array = np.zeros(int(n), dtype=np.float64)

    def setFromOptions(self):
        pass

    def getOwnershipRange(self):
        return 0, self.array.size

    def getSize(self):
        return self.array.size

    def set(self, v):
        self.array[:] = v

    def zeroEntries(self):
        self.array[:] = 0.0

    def duplicate(self):
        return Vec(self.array.size)

    def copy(self, other=None):
        if other is None:
            o = Vec(self.array.size)
            o.array[:] = self.array
            return o
        other.array[:] = self.array
        return other

    def axpy(self, a, x):
        self.array += a * x.array

    def scale(self, a):
        self.array *= a

    def norm(self, norm_type=2):
        return float(np.linalg.norm(self.array))

    def assemblyBegin(self):
        pass

    def assemblyEnd(self):
        pass

    def __getitem__(self, i):
        return self.array[i]

    def __setitem__(self, i, v):
        self.array[i] = v

    def destroy(self):
        self.array = np.zeros(0)


class Mat:
    """Stand-in for the PETSc Mat dRdWT/dRdWTPC handle (device-resident CSR owned by the C-ABI)."""

    def __init__(self):
        self.handle = None

    def create(self, comm=None):
        return self

    def _set(self, h):
        self.destroy()
        self.handle = h

    def getSize(self):
        n = lib().das_mat_rows(self.handle)
        return n, n

    def getInfo(self):
        return {"nz_used": float(lib().das_mat_nnz(self.handle))}

    def to_scipy(self):
        import scipy.sparse as sp

        L = lib()
        n, nnz = L.das_mat_rows(self.handle), L.das_mat_nnz(self.handle)
        rp = np.empty(n + 1, np.int64)
        ci = np.empty(nnz, np.int32)
        v = np.empty(nnz, np.float64)
        check(L.das_mat_export(self.handle, rp.ctypes.data_as(_capi.c_ll_p), ci.ctypes.data_as(_capi.c_int_p), dptr(v)))
        return sp.csr_matrix((v, ci, rp), shape=(n, n))

    @staticmethod
    def from_scipy(A):
        """Device handle of a host CSR matrix (e.g. a dRdWTPC.bin read with petsc_io.read_mat: adjEqnOption.readPCMat)."""
        import scipy.sparse as sp

        A = sp.csr_matrix(A)
        A.sort_indices()
        rp, ci, v = A.indptr.astype(np.int64), A.indices.astype(np.int32), np.ascontiguousarray(A.data, dtype=np.float64)
        h = C.c_void_p()
        check(lib().das_mat_create_from_csr(A.shape[0], rp.ctypes.data_as(_capi.c_ll_p), ci.ctypes.data_as(_capi.c_int_p), dptr(v), C.byref(h)))
        m = Mat()
        m._set(h)
        return m

    def mult(self, x: Vec, y: Vec):
        check(lib().das_mat_mult(self.handle, dptr(x.array), dptr(y.array)))

    def destroy(self):
        if self.handle:
            lib().das_mat_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class KSP:
    """Stand-in for PETSc.KSP (created by the caller, configured by createMLRKSPMatrixFree)."""

    def __init__(self):
        self.handle = None
        self._tols = {}

    def create(self, comm=None):
        return self

    def setTolerances(self, rtol=None, atol=None, divtol=None, max_it=None):
        # mphys_dafoam.py:597-611 adjusts tolerances on the KSP; forwarded to adjEqnOption at solve time
        if rtol is not None:
            self._tols["adjEqnOption.gmresRelTol"] = float(rtol)
        if atol is not None:
            self._tols["adjEqnOption.gmresAbsTol"] = float(atol)
        if max_it is not None:
            self._tols["adjEqnOption.gmresMaxIters"] = int(max_it)

    def getIterationNumber(self):
        it = C.c_int(0)
        check(lib().das_ksp_get_info(self.handle, C.byref(it), None, None, None))
        return it.value

    def getResidualNorm(self):
        r = C.c_double(0)
        check(lib().das_ksp_get_info(self.handle, None, None, C.byref(r), None))
        return r.value

    def info(self):
        it, r0, r, sec = C.c_int(0), C.c_double(0), C.c_double(0), C.c_double(0)
        check(lib().das_ksp_get_info(self.handle, C.byref(it), C.byref(r0), C.byref(r), C.byref(sec)))
        return dict(iters=it.value, res0=r0.value, res=r.value, seconds=sec.value)

    def status(self):
        """How the last solve ended: dict(reason 0 tolerance | 1 gmresMaxIters | 2 breakdown / stagnation | 3 non-finite residual (IDR(s)), nBreakdown, nRefine,
        sweepGrid, sweepPerXcd)."""
        a = [C.c_int(0) for _ in range(4)]
        check(lib().das_ksp_get_status(self.handle, *[C.byref(x) for x in a]))
        return dict(reason=a[0].value, nBreakdown=a[1].value, nRefine=lib().das_ksp_get_n_refine(self.handle), sweepGrid=a[2].value,
                    sweepPerXcd=a[3].value)

    def blocks(self):
        L = lib()
        nb = check(L.das_ksp_get_n_blocks(self.handle))
        n = self._n
        perm = np.zeros(n, np.int32)
        off = np.zeros(nb + 1, np.int64)
        check(L.das_ksp_get_blocks(self.handle, perm.ctypes.data_as(_capi.c_int_p), off.ctypes.data_as(_capi.c_ll_p)))
        return perm, off

    def pcStructure(self):
        """Node structure of the default ("bilu") preconditioner: dict(nodeUnk[nNodes, 8], bptr, bcol, lvlPtr, natural)."""
        L = lib()
        nN, nB, nLv = C.c_int(0), C.c_longlong(0), C.c_int(0)
        check(L.das_ksp_get_pc_structure_sizes(self.handle, C.byref(nN), C.byref(nB), C.byref(nLv)))
        nu = np.empty(nN.value * 8, np.int32)
        bptr = np.empty(nN.value + 1, np.int64)
        bcol = np.empty(nB.value, np.int32)
        lvl = np.empty(nLv.value + 1, np.int32)
        nat = np.empty(nN.value, np.int32)
        ip = _capi.c_int_p
        check(L.das_ksp_get_pc_structure(self.handle, nu.ctypes.data_as(ip), bptr.ctypes.data_as(_capi.c_ll_p), bcol.ctypes.data_as(ip),
                                         lvl.ctypes.data_as(ip), nat.ctypes.data_as(ip)))
        out = np.empty(nN.value * 8, np.int32)
        check(L.das_ksp_get_pc_node_out(self.handle, out.ctypes.data_as(ip)))
        return dict(nodeUnk=nu.reshape(-1, 8), bptr=bptr, bcol=bcol, lvlPtr=lvl, natural=nat, nodeOut=out.reshape(-1, 8))

    def coarse(self, n_cells):
        """(nAgg, aggOfCell) of the two-level preconditioner's pressure coarse space (nAgg = 0: none)."""
        agg = np.full(n_cells, -1, np.int32)
        nagg = lib().das_ksp_get_coarse(self.handle, agg.ctypes.data_as(_capi.c_int_p))
        return nagg, agg

    def applyPC(self, solver, x):
        y = np.zeros_like(x)
        check(lib().das_ksp_apply_pc(solver._h, self.handle, dptr(np.ascontiguousarray(x)), dptr(y)))
        return y

    def history(self):
        buf = np.zeros(self.getIterationNumber() + 2)
        m = check(lib().das_ksp_get_history(self.handle, dptr(buf), buf.size))
        return buf[:m]

    def basisInfo(self):
        """Krylov basis of the last solve: dict(fp32 (compressed fp32 storage), split (hi + lo floats: inner products read hi only),
        mappedGB, bytesPerVector) - amd.krylovBasisPrecision."""
        f, mb, bv = C.c_int(0), C.c_double(0), C.c_double(0)
        check(lib().das_ksp_get_basis_info(self.handle, C.byref(f), C.byref(mb), C.byref(bv)))
        return dict(fp32=bool(f.value & 1), split=bool(f.value & 2), mappedGB=mb.value / 2**30, bytesPerVector=bv.value)

    def idrInfo(self):
        """IDR(s) of the last solve (amd.krylovMethod "idrs"): dict(s (as used), cycles, restarts, breakdowns, workVectors (3 s + 5: P, G, U,
        r, z, t, right-hand side, solution), workBytes (8 n each)); all 0 for a KSP that never ran it."""
        a = [C.c_int(0) for _ in range(5)]
        wb = C.c_double(0)
        check(lib().das_ksp_get_idr_info(self.handle, *[C.byref(x) for x in a], C.byref(wb)))
        return dict(s=a[0].value, cycles=a[1].value, restarts=a[2].value, breakdowns=a[3].value, workVectors=a[4].value, workBytes=wb.value)

    def polyInfo(self):
        """Polynomial preconditioning of the last solve (amd.polyDegree): dict(degree (as used; 0 = none), nComplexPairs, products (operator
        products: what info()["iters"] reports in this mode), columns (Arnoldi columns built after the generating cycle: the basis the option is
        about), generatingColumns (the columns of the generating cycle; the history holds one entry per column of both), generated, fallback (1: no usable roots, the solve ran
        without a polynomial), workVectors (3 once a polynomial was built), workBytes (8 n each), roots (the ordered roots as (re, im); a pair
        once, im > 0)); all 0 / empty for a KSP whose last solve ran without the option."""
        a = [C.c_int(0) for _ in range(6)]
        pr, co, gc, wb = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0), C.c_double(0)
        re, im = np.zeros(16), np.zeros(16)
        check(lib().das_ksp_get_poly_info(self.handle, C.byref(a[0]), C.byref(a[1]), C.byref(pr), C.byref(co), C.byref(gc), C.byref(a[2]), C.byref(a[3]), C.byref(a[4]), C.byref(wb),
                                          C.byref(a[5]), dptr(re), dptr(im)))
        return dict(degree=a[0].value, nComplexPairs=a[1].value, products=pr.value, columns=co.value, generatingColumns=gc.value, generated=a[2].value, fallback=a[3].value, workVectors=a[4].value,
                    workBytes=wb.value, roots=[(float(re[i]), float(im[i])) for i in range(a[5].value)])

    def cycleLengths(self):
        """Columns of every closed Arnoldi cycle of the last solve (all but the last equal gmresRestart, DALinearEqn.C:155)."""
        buf = np.zeros(max(1, self.getIterationNumber() + 2), np.int32)
        m = check(lib().das_ksp_get_cycle_lengths(self.handle, buf.ctypes.data_as(_capi.c_int_p), buf.size))
        return buf[:m].copy()

    def destroy(self):
        if self.handle:
            lib().das_ksp_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _flatten(prefix, obj, out):
    for k, v in obj.items():
        key = f"{prefix}.{k}" if prefix else k
        if isinstance(v, dict):
            _flatten(key, v, out)
        else:
            out[key] = v


# ----------------------------------------------------------------------------- pyDASolvers
class pyDASolvers:
    """GPU-backed replacement of the reference's ``pyDASolvers`` extension class.

    ``argsAll`` is the reference's command string (``b"DASimpleFoam -python"``, pyDAFoam.py:1425-1430); its first
    token must agree with ``pyOptions["solverName"]``.  The reference reads the mesh and fields from the OpenFOAM
    case in the working directory; here the same data arrives as a :class:`~dafoam_amd.meshgen.FoamCase`
    (``case=`` keyword or ``pyOptions["amdCase"]``).
    """

    def __init__(self, argsAll, pyOptions, case: FoamCase = None):
        if isinstance(argsAll, bytes):
            argsAll = argsAll.decode()
        self._args = argsAll
        case = case if case is not None else pyOptions.get("amdCase")
        if case is None:
            raise ValueError("pyDASolvers: a FoamCase is required (case= or pyOptions['amdCase'])")
        solver = argsAll.split()[0] if argsAll else case.solver_name
        if solver not in ("DASolvers", case.solver_name):
            raise ValueError(f"argsAll solver {solver} != case solver {case.solver_name}")
        self._case = case
        self._pimple = case.solver_name == "DAPimpleFoam"
        if self._pimple:
            self._pimple_checks(pyOptions if isinstance(pyOptions, dict) else {})
        self._fvSource = self._checked_fv_source(pyOptions.get("fvSource") if isinstance(pyOptions, dict) else None)
        self._cs = CaseStruct(case)
        L = lib()
        self._h = L.das_create(self._cs.byref())
        if not self._h:
            raise _capi.DASError(L.das_last_error().decode())
        self._inited = False
        self._device = int(pyOptions.get("amdDevice", 0)) if isinstance(pyOptions, dict) else 0
        # adjStateOrdering (reference DAIndex.C:188-397,518-661): the library works in "state" ordering; "cell"
        # ordering is provided at this boundary as a permutation of every state-length array
        self._perm = None
        if isinstance(pyOptions, dict) and pyOptions.get("adjStateOrdering", "state") == "cell":
            self._perm = self._cell_ordering_permutation()
        self.updateDAOption(pyOptions)
        self._inputInfo = dict(pyOptions.get("inputInfo") or {}) if isinstance(pyOptions, dict) else {}
        self._primalBC = dict(pyOptions.get("primalBC") or {}) if isinstance(pyOptions, dict) else {}
        self._checkMeshThreshold = dict(pyOptions.get("checkMeshThreshold") or {}) if isinstance(pyOptions, dict) else {}
        self._patchVelocity = [0.0, 0.0]  # DAGlobalVar::patchVelocity = [UMag, AoA(deg)], set by DAInputPatchVelocity::run
        self._flowdir_fns = {}
        self._wallDistanceMethod = pyOptions.get("wallDistanceMethod", "default") if isinstance(pyOptions, dict) else "default"
        self._discipline = pyOptions.get("discipline", "aero") if isinstance(pyOptions, dict) else "aero"
        self._define_functions(pyOptions.get("function") if isinstance(pyOptions, dict) else None)
        self._define_outputs(pyOptions.get("outputInfo") if isinstance(pyOptions, dict) else None)
        self._define_thermal_inputs()
        self._define_fv_sources()
        self._define_regression_models(pyOptions.get("regressionModel") if isinstance(pyOptions, dict) else None)
        if case.states is not None:  # FoamCase.states is always in "state" ordering (input data)
            check(lib().das_update_of_fields(self._h, dptr(np.ascontiguousarray(case.states, dtype=np.float64))))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().das_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- adjStateOrdering "cell" ----------------------------------------------------------------------
    def _cell_ordering_permutation(self):
        """perm[k] = index in "state" ordering of the k-th entry of the "cell" ordering: per cell its cell states
        (volVector, volScalar, model) followed by the phi of the faces it owns (DAIndex.C:602-651)."""
        m = self._case.mesh
        N, F = m.n_cells, m.n_faces
        layout = {"DASimpleFoam": (1, 3 if getattr(self._case, "has_T", False) else 2), "DAPimpleFoam": (1, 2), "DARhoSimpleFoam": (1, 3), "DATurboFoam": (1, 3),
                  "DAScalarTransportFoam": (0, 1), "DAHeatTransferFoam": (0, 1), "DASolidDisplacementFoam": (1, 0)}[self._case.solver_name]
        nvec, nscl = layout
        has_phi = self._case.solver_name not in ("DAScalarTransportFoam", "DAHeatTransferFoam", "DASolidDisplacementFoam")
        owned = [[] for _ in range(N)]
        if has_phi:
            for f in range(F):
                owned[m.owner[f]].append(f)
        perm = []
        for c in range(N):
            for v in range(nvec):
                perm += [3 * N * v + 3 * c + k for k in range(3)]
            for b in range(nscl):
                perm.append(3 * N * nvec + b * N + c)
            perm += [3 * N * nvec + nscl * N + f for f in owned[c]]
        return np.array(perm, dtype=np.int64)

    def _to_state(self, a):
        if self._perm is None:
            return a
        out = np.empty_like(a)
        out[self._perm] = a
        return out

    def _from_state(self, a_state, out):
        if self._perm is None:
            if out is not a_state:
                out[:] = a_state
        else:
            out[:] = a_state[self._perm]

    # -- lifecycle -------------------------------------------------------------------------
    def initSolver(self):
        check(lib().das_init_solver(self._h, self._device))
        self._inited = True

    def updateDAOption(self, pyOptions):
        """pyDASolvers.pyx:355; nested dict -> flattened "a.b" keys (values may be the reference's
        [type, value] pairs produced by pyDAFoam._getDefOptions, pyDAFoam.py:823-844)."""
        flat = {}
        opts = {k: (v[1] if isinstance(v, list) and len(v) == 2 and isinstance(v[0], type) else v) for k, v in pyOptions.items()}
        _flatten("", {k: v for k, v in opts.items() if not k.startswith("amdCase") and k not in ("function", "inputInfo", "outputInfo", "primalBC", "fvSource", "regressionModel")}, flat)
        if flat.get("adjStateOrdering") == "cell" and getattr(self, "_perm", None) is not None:
            flat.pop("adjStateOrdering")  # handled at this boundary (permutation); the library stays in "state" ordering
        L = lib()
        for k, v in flat.items():
            kb = k.encode()
            if isinstance(v, bool):
                check(L.das_set_option_int(self._h, kb, int(v)))
            elif isinstance(v, int):
                check(L.das_set_option_int(self._h, kb, v))
            elif isinstance(v, float):
                check(L.das_set_option_double(self._h, kb, v))
            elif isinstance(v, str):
                check(L.das_set_option_str(self._h, kb, v.encode()))
            elif isinstance(v, (list, tuple)) and all(isinstance(x, str) for x in v):
                check(L.das_set_option_str(self._h, kb, ",".join(v).encode()))
            # other option kinds (lists of numbers, ...) are not forwarded

    def printAllOptions(self):
        print("dafoam_amd options are held by the C-ABI; see DAOPTION for defaults")

    # -- sizes -------------------------------------------------------------------------------
    def getNLocalAdjointStates(self):
        return int(lib().das_get_n_local_adjoint_states(self._h))

    def getNLocalAdjointBoundaryStates(self):
        m = self._case.mesh
        nb = m.n_faces - m.n_internal_faces
        return {"DASimpleFoam": 6 if getattr(self._case, "has_T", False) else 5, "DAPimpleFoam": 5, "DARhoSimpleFoam": 6, "DATurboFoam": 6}.get(self._case.solver_name, 1) * nb

    def getNLocalCells(self):
        return int(lib().das_get_n_local_cells(self._h))

    def getNGlobalCells(self):
        return int(lib().das_get_n_global_cells(self._h))

    def getNLocalPoints(self):
        return int(lib().das_get_n_local_points(self._h))

    def getInputSize(self, inputName, inputType):
        if inputType == "patchVelocity":  # [UMag, AoA(deg)]  (reference DAInputPatchVelocity.H size() = 2)
            return 2
        if inputType == "patchVar":  # reference DAInputPatchVar.H: 1 (scalar) or 3 (vector)
            return 3 if self._input_entry(inputName, inputType)["varType"] == "vector" else 1
        if inputType == "field":  # reference DAInputField.H size(): the selected cells (here: all) x 1 for a scalar field
            self._field_entry(inputName)
            return self._case.mesh.n_cells
        if inputType == "thermalCoupling":  # reference DAInputThermalCoupling.C:52-63: two entries per face of the patches
            sizes = {p.name: p.size for p in self._case.mesh.patches}
            return 2 * sum(sizes[p] for p in self._input_entry(inputName, inputType)["patches"])
        if inputType == "volCoord":  # reference DAInputVolCoord.H size() = nLocalPoints * 3
            return self.getNLocalPoints() * 3
        if inputType == "fvSourcePar":  # reference DAInputFvSourcePar.H size() = indices.size()
            return len(self._fv_source_par_entry(inputName)[1])
        if inputType == "regressionPar":  # reference DAInputRegressionPar.H size() = nParameters(modelName); the entry is keyed by the model name
            return self._regression_par_entry(inputName)
        return check(lib().das_get_input_size(self._h, inputName.encode(), inputType.encode()))

    # -- boundary-value inputs (reference src/adjoint/DAInput/DAInputPatchVelocity.C, DAInputPatchVar.C) ---------
    def _input_entry(self, inputName, inputType):
        if inputName not in self._inputInfo:
            raise _capi.DASError(f"inputInfo has no entry {inputName}")
        e = self._inputInfo[inputName]
        if e.get("type") != inputType:
            raise _capi.DASError(f"inputInfo[{inputName}].type is {e.get('type')}, not {inputType}")
        if inputType == "patchVar" and e.get("varType") not in ("scalar", "vector"):
            raise _capi.DASError("varType not valid")
        return e

    def _field_entry(self, inputName):
        """inputInfo entry of a `field` input (reference DAInputField.C:33-86): fieldName, fieldType "scalar"; cellSetName /
        vector fields are not implemented here."""
        e = self._input_entry(inputName, "field")
        if e.get("fieldName") == "fvSource":
            raise _capi.DASError(f"inputInfo[{inputName}]: a field input with fieldName fvSource is not built (vector field inputs are not implemented; "
                                 "the fvSourcePar input drives the actuator disks)")
        if e.get("fieldType", "scalar") != "scalar":
            raise _capi.DASError("field input: only fieldType scalar is implemented")
        if "cellSetName" in e:
            raise _capi.DASError("field input: cellSetName is not implemented (the field covers all cells)")
        return e

    def getField(self, fieldName):
        out = np.zeros(self._case.mesh.n_cells)
        check(lib().das_get_field(self._h, fieldName.encode(), dptr(out)))
        return out

    def _patch_ids(self, entry):
        names = [p.name for p in self._case.mesh.patches]
        return np.array([names.index(p) for p in entry["patches"]], dtype=np.int32)

    def _patch_input_tangents(self, inputName, inputType, inputs):
        """(field, value[3], [tangent_i[3] for each input component])"""
        e = self._input_entry(inputName, inputType)
        if inputType == "patchVelocity":
            ax = {"x": 0, "y": 1, "z": 2}
            fi, ni = ax[e["flowAxis"]], ax[e["normalAxis"]]
            ids = self._patch_ids(e)
            cur = np.zeros(3)
            check(lib().das_get_patch_value(self._h, int(ids[0]), b"U", dptr(cur)))
            a = float(inputs[1]) * np.pi / 180.0
            val = cur.copy()
            val[fi], val[ni] = inputs[0] * np.cos(a), inputs[0] * np.sin(a)
            t_mag, t_aoa = np.zeros(3), np.zeros(3)
            t_mag[fi], t_mag[ni] = np.cos(a), np.sin(a)
            t_aoa[fi], t_aoa[ni] = -inputs[0] * np.sin(a) * np.pi / 180.0, inputs[0] * np.cos(a) * np.pi / 180.0
            return "U", val, [t_mag, t_aoa]
        name = e["varName"]
        if e["varType"] == "vector":
            return name, np.asarray(inputs, dtype=np.float64).copy(), [np.eye(3)[k].copy() for k in range(3)]
        return name, np.array([float(inputs[0]), 0.0, 0.0]), [np.array([1.0, 0.0, 0.0])]

    def setSolverInput(self, inputName, inputType, inputSize, inputs, seeds=None):
        """DAInput::run (reference pyDASolvers.pyx:164-182): assign the input to the solver.  (Forward-mode seeds
        belong to the reference's ADF build and are ignored here.)"""
        assert len(inputs) == inputSize, "invalid input array size!"
        if inputType == "stateVar":
            return self.updateOFFields(np.ascontiguousarray(inputs, dtype=np.float64))
        if inputType == "volCoord":
            # DAInputVolCoord::run (reference DAInputVolCoord.C:46-70): the input array is the point field; mesh.movePoints
            return self.updateOFMesh(inputs)
        if inputType == "field":
            # DAInputField::run (reference DAInputField.C:88-151): the input array IS the volScalarField (all cells; scalar fields)
            e = self._field_entry(inputName)
            return check(lib().das_set_field(self._h, e["fieldName"].encode(), dptr(np.ascontiguousarray(inputs, dtype=np.float64))))
        if inputType == "thermalCoupling":
            # DAInputThermalCoupling::run: refValue and, from the neighbour's kappa / d, the valueFraction of the mixed T patches
            self._input_entry(inputName, inputType)
            return check(lib().das_set_thermal_coupling_input(self._h, inputName.encode(), dptr(np.ascontiguousarray(inputs, dtype=np.float64)), inputSize))
        if inputType == "fvSourcePar":
            # DAInputFvSourcePar::run (reference DAInputFvSourcePar.C:75-140): heatSourcePars / actuatorDiskPars[indices] = input, then updateFvSource
            name, idx = self._fv_source_par_entry(inputName)
            setter = lib().das_set_actuator_disk_pars if self._is_actuator_disk(name) else lib().das_set_heat_source_pars
            return check(setter(self._h, name.encode(), idx.ctypes.data_as(_capi.c_int_p), idx.size, dptr(np.ascontiguousarray(inputs, dtype=np.float64))))
        if inputType == "regressionPar":
            # DAInputRegressionPar::run (reference DAInputRegressionPar.C:48-62): parameters[modelName] = input; the next residual sees them
            self._regression_par_entry(inputName)
            return check(lib().das_set_regression_parameters(self._h, inputName.encode(), dptr(np.ascontiguousarray(inputs, dtype=np.float64)), inputSize))
        if inputType not in ("patchVelocity", "patchVar"):
            raise _capi.DASError(f"inputType not supported on this path: {inputType}")
        field, val, _ = self._patch_input_tangents(inputName, inputType, inputs)
        ids = self._patch_ids(self._inputInfo[inputName])
        check(lib().das_set_patch_value(self._h, ids.ctypes.data_as(_capi.c_int_p), ids.size, field.encode(), dptr(np.ascontiguousarray(val))))
        if inputType == "patchVelocity":
            # DAGlobalVar::patchVelocity: the forces defined parallel / normal to the flow follow the new AoA
            self._patchVelocity = [float(inputs[0]), float(inputs[1])]
            for fname, meta in self._flowdir_fns.items():
                if meta["pv"] == inputName:
                    self._define_flowdir(fname)

    def getOutputSize(self, outputName, outputType):
        return check(lib().das_get_output_size(self._h, outputName.encode(), outputType.encode()))

    # -- states / residuals --------------------------------------------------------------------
    def updateOFFields(self, states):
        assert len(states) == self.getNLocalAdjointStates(), "invalid array size!"
        check(lib().das_update_of_fields(self._h, dptr(np.ascontiguousarray(self._to_state(states)))))

    def getOFFields(self, states):
        assert len(states) == self.getNLocalAdjointStates(), "invalid array size!"
        tmp = np.zeros(len(states)) if self._perm is not None else states
        check(lib().das_get_of_fields(self._h, dptr(tmp)))
        self._from_state(tmp, states)

    def getResiduals(self, residuals):
        assert len(residuals) == self.getNLocalAdjointStates(), "invalid input array size!"
        tmp = np.zeros(len(residuals)) if self._perm is not None else residuals
        check(lib().das_get_residuals(self._h, dptr(tmp)))
        self._from_state(tmp, residuals)

    def calcResiduals(self, isPC, residuals):
        assert len(residuals) == self.getNLocalAdjointStates(), "invalid input array size!"
        tmp = np.zeros(len(residuals)) if self._perm is not None else residuals
        check(lib().das_calc_residuals(self._h, int(isPC), dptr(tmp)))
        self._from_state(tmp, residuals)

    def updateStateBoundaryConditions(self):
        # boundary values are recomputed inline by every kernel from the state vector: nothing to do
        return None

    def getOFMeshPoints(self, points):
        assert len(points) == self.getNLocalPoints() * 3, "invalid array size!"
        check(lib().das_get_of_mesh_points(self._h, dptr(points)))

    def updateOFMesh(self, vol_coords):
        """pyDASolvers.pyx:297-300 (PYDAFOAM.setVolCoords, pyDAFoam.py:2111-2117): new point coordinates; the library
        recomputes the fvMesh metrics (the wall distance stays frozen).  Jacobians assembled earlier describe the old
        mesh and have to be rebuilt by the caller, as in the reference."""
        assert len(vol_coords) == self.getNLocalPoints() * 3, "invalid array size!"
        check(lib().das_update_of_mesh(self._h, dptr(np.ascontiguousarray(vol_coords, dtype=np.float64))))

    def calcVolCoordDirectionalProduct(self, dX, outputName, outputType, seeds, eps=1e-6):
        """seeds^T (dOutput/dX . dX) for ONE direction dX of the mesh points (e.g. the volume-mesh sensitivity of one
        FFD design variable), by a central difference of the geometry: two metric updates + two residual (or objective)
        evaluations on the device.  The reference returns the full product vector of calcJacTVecProduct(volCoord -> ...)
        from one reverse sweep of its AD tape (DASolver.C:1690-1839); without a tape the per-design-variable form is the
        one that maps to forward evaluations - the design variables of a shape optimisation are few.
        eps is relative to max|dX| (step = eps * characteristic point spacing / max|dX| is the caller's choice: here the
        points move by eps * dX)."""
        n3 = self.getNLocalPoints() * 3
        assert len(dX) == n3, "invalid array size!"
        X0 = np.zeros(n3)
        self.getOFMeshPoints(X0)
        dX = np.asarray(dX, dtype=np.float64)
        vals = []
        try:
            for sgn in (1.0, -1.0):
                self.updateOFMesh(X0 + sgn * eps * dX)
                if outputType == "residual":
                    R = np.zeros(self.getNLocalAdjointStates())
                    check(lib().das_get_residuals(self._h, dptr(R)))
                    vals.append(float(np.dot(self._to_state(np.asarray(seeds, dtype=np.float64)), R)))
                elif outputType == "function":
                    vals.append(float(seeds[0]) * self.calcFunction(outputName))
                else:
                    raise _capi.DASError(f"outputType not supported on this path: {outputType}")
        finally:
            self.updateOFMesh(X0)
        return (vals[0] - vals[1]) / (2.0 * eps)

    def pointInfluence(self):
        """Host-side structure of the volCoord product (no GPU needed): dict(colors[nPoints], nColors, ptr, cells, steps) - the
        cells whose residual rows can feel a point (CSR), a colouring of the points with pairwise disjoint sets, the
        central-difference step of every point."""
        nc, ne = C.c_int(0), C.c_longlong(0)
        check(lib().das_point_influence_build(self._h, C.byref(nc), C.byref(ne)))
        P = self.getNLocalPoints()
        col = np.zeros(P, np.int32)
        ptr = np.zeros(P + 1, np.int64)
        cells = np.zeros(ne.value, np.int32)
        h = np.zeros(P)
        check(lib().das_point_influence_get(self._h, col.ctypes.data_as(_capi.c_int_p), ptr.ctypes.data_as(_capi.c_ll_p),
                                            cells.ctypes.data_as(_capi.c_int_p), dptr(h)))
        return dict(colors=col, nColors=nc.value, ptr=ptr, cells=cells, steps=h)

    def deviceGeometry(self, points):
        """The metrics the DEVICE passes of the volCoord product compute for `points` (test aid): (fg[nF, 12], cg[nC, 5]) in the
        record layout of csrc/das_common.hpp (Sf, magSf, w, nod, corr, Cf | C, V, y)."""
        m = self._case.mesh
        fg = np.zeros(12 * m.n_faces)
        cg = np.zeros(5 * m.n_cells)
        check(lib().das_debug_device_geometry(self._h, dptr(np.ascontiguousarray(points, dtype=np.float64)), dptr(fg), dptr(cg)))
        return fg.reshape(-1, 12), cg.reshape(-1, 5)

    def geometry(self):
        """fvMesh metrics computed by the library (host side)."""
        m = self._case.mesh
        F, Fi, N = m.n_faces, m.n_internal_faces, m.n_cells
        out = dict(Sf=np.zeros(3 * F), Cf=np.zeros(3 * F), C=np.zeros(3 * N), V=np.zeros(N), w=np.zeros(Fi),
                   nonOrthDeltaCoeffs=np.zeros(Fi), nonOrthCorr=np.zeros(3 * Fi), bDeltaCoeffs=np.zeros(F - Fi))
        check(lib().das_get_geometry(self._h, *[dptr(out[k]) for k in
                                                ("Sf", "Cf", "C", "V", "w", "nonOrthDeltaCoeffs", "nonOrthCorr", "bDeltaCoeffs")]))
        return out

    # -- colouring / Jacobians -------------------------------------------------------------------
    def runColoring(self, cacheDir=None, nProcs=1, rank=0):
        """DASolver::runColoring (DASolver.C:708-745).  With cacheDir the colouring is kept like the reference keeps
        it, as a PETSc binary Vec `dRdWColoring_<nProcs>.bin` (`DAJacCon.C:1886-2019`; one file per rank here, suffix
        `_<rank>` when nProcs > 1): read + validated if present and of the right size, computed and written otherwise.
        A file that does not validate (different mesh) is recomputed, not trusted."""
        if cacheDir is None:
            return check(lib().das_run_coloring(self._h))
        import os

        from . import petsc_io

        name = f"dRdWColoring_{nProcs}" + (f"_{rank}" if nProcs > 1 else "") + ".bin"
        path = os.path.join(cacheDir, name)
        n = self.getNLocalAdjointStates()
        if os.path.exists(path):
            try:
                col = petsc_io.read_vec(path)
                if col.size == n and np.all(col == np.round(col)):
                    ci = np.ascontiguousarray(col, dtype=np.int32)
                    check(lib().das_set_coloring(self._h, ci.ctypes.data_as(_capi.c_int_p)))
                    return
            except (_capi.DASError, ValueError, OSError):
                pass  # stale / foreign cache: fall through and recompute
        check(lib().das_run_coloring(self._h))
        col, _ = self.getColoring()
        tmp = path + f".tmp{os.getpid()}"
        petsc_io.write_vec(tmp, col.astype(np.float64))
        os.replace(tmp, path)

    def getColoring(self):
        n = self.getNLocalAdjointStates()
        col = np.zeros(n, np.int32)
        check(lib().das_get_colors(self._h, 0, col.ctypes.data_as(_capi.c_int_p)))
        return col, check(lib().das_get_n_colors(self._h, 0))

    def getConnectivity(self, isPC=0):
        import scipy.sparse as sp

        n = self.getNLocalAdjointStates()
        nnz = check(lib().das_get_con_nnz(self._h, int(isPC)))
        rp = np.zeros(n + 1, np.int64)
        ci = np.zeros(nnz, np.int32)
        check(lib().das_get_con(self._h, int(isPC), rp.ctypes.data_as(_capi.c_ll_p), ci.ctypes.data_as(_capi.c_int_p)))
        return sp.csr_matrix((np.ones(nnz, np.int8), ci, rp), shape=(n, n))

    def pcStructure(self):
        """Node structure the default ("bilu") preconditioner would be factorised on, built on the host (no GPU needed):
        dict(nodeUnk[nNodes, 8], bptr, bcol, lvlPtr, natural, reach)."""
        L = lib()
        nN, nB, nLv, reach = C.c_int(0), C.c_longlong(0), C.c_int(0), C.c_int(0)
        check(L.das_pc_structure_build(self._h, C.byref(nN), C.byref(nB), C.byref(nLv), C.byref(reach)))
        nu = np.empty(nN.value * 8, np.int32)
        bptr = np.empty(nN.value + 1, np.int64)
        bcol = np.empty(nB.value, np.int32)
        lvl = np.empty(nLv.value + 1, np.int32)
        nat = np.empty(nN.value, np.int32)
        ip = _capi.c_int_p
        check(L.das_pc_structure_get(self._h, nu.ctypes.data_as(ip), bptr.ctypes.data_as(_capi.c_ll_p), bcol.ctypes.data_as(ip),
                                     lvl.ctypes.data_as(ip), nat.ctypes.data_as(ip)))
        return dict(nodeUnk=nu.reshape(-1, 8), bptr=bptr, bcol=bcol, lvlPtr=lvl, natural=nat, reach=reach.value)

    def calcdRdWT(self, isPC, dRdWT: Mat, mode=None):
        """pyDASolvers.pyx:237.  mode None: the reference's behaviour for the PC (coloured FD) and exact
        dual-number assembly for isPC=0."""
        if mode is None:
            mode = 0 if isPC else 1
        h = C.c_void_p()
        check(lib().das_calc_drdwt(self._h, int(isPC), int(mode), C.byref(h)))
        dRdWT._set(h)

    def initializedRdWTMatrixFree(self):
        check(lib().das_initialize_drdwt_matrix_free(self._h))

    def destroydRdWTMatrixFree(self):
        check(lib().das_destroy_drdwt_matrix_free(self._h))

    def calcJacTVecProduct(self, inputName, inputType, inputs, outputName, outputType, seeds, product):
        inputSize = self.getInputSize(inputName, inputType)
        outputSize = self.getOutputSize(outputName, outputType)
        assert len(inputs) == inputSize, "invalid input array size!"
        assert len(seeds) == outputSize, "invalid seed array size!"
        assert len(product) == inputSize, "invalid product array size!"
        seeds_s = np.ascontiguousarray(self._to_state(seeds)) if outputType == "residual" else seeds
        if inputType == "volCoord":
            # run(input) = movePoints, then the full product over all points from coloured central differences on the device
            X0 = np.zeros(inputSize)
            self.getOFMeshPoints(X0)
            if not np.array_equal(X0, np.asarray(inputs, dtype=np.float64)):
                self.updateOFMesh(inputs)
            info = np.zeros(4)
            check(lib().das_calc_dvolcoord_product(self._h, outputName.encode(), outputType.encode(),
                                                   dptr(np.ascontiguousarray(seeds_s, dtype=np.float64)), dptr(product), dptr(info)))
            self._volCoordInfo = dict(colors=int(info[0]), passes=int(info[1]), seconds=float(info[2]), build_seconds=float(info[3]))
            return
        if inputType == "thermalCoupling":
            # run(input), then forward-mode passes with the seeds in the mixed records and a per-face gather
            self.setSolverInput(inputName, inputType, inputSize, inputs)
            out = np.zeros(inputSize)
            check(lib().das_calc_dthermal_coupling_product(self._h, inputName.encode(), outputName.encode(), outputType.encode(),
                                                           dptr(np.ascontiguousarray(seeds_s, dtype=np.float64)), dptr(out), inputSize))
            product[:] = out
            return
        if inputType == "fvSourcePar":
            # run(input), then one forward-mode pass per selected parameter (das_calc_dfvsourcepar_product)
            self.setSolverInput(inputName, inputType, inputSize, inputs)
            name, idx = self._fv_source_par_entry(inputName)
            out = np.zeros(inputSize)
            prod = lib().das_calc_dactuatordiskpar_product if self._is_actuator_disk(name) else lib().das_calc_dfvsourcepar_product
            check(prod(self._h, name.encode(), idx.ctypes.data_as(_capi.c_int_p), idx.size, outputName.encode(), outputType.encode(),
                       dptr(np.ascontiguousarray(seeds_s, dtype=np.float64)), dptr(out)))
            product[:] = out
            return
        if inputType == "regressionPar":
            # run(input), then one dual pass for seeds . dR / d beta per cell and the reverse pass through the model (das_calc_dregressionpar_product)
            self.setSolverInput(inputName, inputType, inputSize, inputs)
            out = np.zeros(inputSize)
            check(lib().das_calc_dregressionpar_product(self._h, inputName.encode(), outputName.encode(), outputType.encode(),
                                                        dptr(np.ascontiguousarray(seeds_s, dtype=np.float64)), dptr(out)))
            product[:] = out
            return
        if inputType == "field":
            # run(input), then ONE forward-mode pass with a unit tangent on every cell (das_calc_dfield_product)
            # (DAHeatTransferFoam has no Spalart-Allmaras field to assign: nothing of it reads the input, the product is exact zeros)
            if self._case.solver_name not in ("DAHeatTransferFoam", "DASolidDisplacementFoam"):
                self.setSolverInput(inputName, inputType, inputSize, inputs)
            e = self._field_entry(inputName)
            check(lib().das_calc_dfield_product(self._h, e["fieldName"].encode(), outputName.encode(), outputType.encode(),
                                                dptr(np.ascontiguousarray(seeds_s, dtype=np.float64)), dptr(product)))
            return
        if inputType in ("patchVelocity", "patchVar"):
            # run(input), then one forward-mode pass per input component
            self.setSolverInput(inputName, inputType, inputSize, inputs)
            field, _, tangents = self._patch_input_tangents(inputName, inputType, inputs)
            ids = self._patch_ids(self._inputInfo[inputName])
            out = C.c_double(0.0)
            for i, t in enumerate(tangents):
                check(lib().das_calc_dbc_product(self._h, ids.ctypes.data_as(_capi.c_int_p), ids.size, field.encode(), dptr(np.ascontiguousarray(t)),
                                                 outputName.encode(), outputType.encode(), dptr(np.ascontiguousarray(seeds_s, dtype=np.float64)), C.byref(out)))
                product[i] = out.value
            meta = self._flowdir_fns.get(outputName) if outputType == "function" else None
            if meta is not None and inputType == "patchVelocity" and meta["pv"] == inputName:
                # the force direction itself depends on the AoA: F is linear in it, so dF/dAoA|dir = F(d') with the
                # unit vector of d' = dd/dAoA, times |d'| = pi/180
                dprime = self._flow_direction(meta, deriv=True)
                tmp = outputName + "__ddir"
                self._define_flowdir(outputName, name=tmp, direction=dprime * (180.0 / np.pi))
                product[1] += float(seeds[0]) * self.calcFunction(tmp) * (np.pi / 180.0)
            return
        tmp = np.zeros(len(product)) if self._perm is not None else product
        check(lib().das_calc_jac_t_vec_product(
            self._h, inputName.encode(), inputType.encode(), dptr(np.ascontiguousarray(self._to_state(inputs))), outputName.encode(),
            outputType.encode(), dptr(np.ascontiguousarray(seeds_s, dtype=np.float64)), dptr(tmp)))
        self._from_state(tmp, product)

    def calcJacVecProduct(self, v, product):
        """Forward-mode dR/dW (s o v) at the current states: one dual-number residual pass (no colouring, no matrix)."""
        n = self.getNLocalAdjointStates()
        assert len(v) == n, "invalid input array size!"
        assert len(product) == n, "invalid product array size!"
        tmp = np.zeros(n) if self._perm is not None else product
        check(lib().das_calc_jac_vec_product(self._h, dptr(np.ascontiguousarray(self._to_state(v))), dptr(tmp)))
        self._from_state(tmp, product)

    def calcdRdWOldTPsiAD(self, oldTimeLevel, psi, dRdWOldTPsi):
        assert len(psi) == self.getNLocalAdjointStates(), "invalid input array size!"
        assert len(dRdWOldTPsi) == self.getNLocalAdjointStates(), "invalid seed array size!"
        tmp = np.zeros(len(psi)) if self._perm is not None else dRdWOldTPsi
        check(lib().das_calc_drdwold_t_psi(self._h, int(oldTimeLevel), dptr(np.ascontiguousarray(self._to_state(psi))), dptr(tmp)))
        self._from_state(tmp, dRdWOldTPsi)

    def setOldTimeStates(self, W0, W00=None, timeIndex=None):
        """DAPimpleFoam: the state vectors of the two old time levels (the ordering of getOFFields) onto the device, with the time index
        the residual is evaluated at (default: the one of setTime).  W00 may be None where the scheme is Euler or timeIndex < 2.  Every
        residual, Jacobian and product evaluated afterwards is R(W; W0, W00)."""
        if not self._pimple:
            raise _capi.DASError(f"setOldTimeStates: old-time states only exist for DAPimpleFoam, not for {self._case.solver_name}")
        n = self.getNLocalAdjointStates()
        if np.size(W0) != n or (W00 is not None and np.size(W00) != n):
            raise _capi.DASError(f"setOldTimeStates: the old-time state vectors need {n} entries")
        ti = int(getattr(self, "_timeIndex", 1) if timeIndex is None else timeIndex)
        self._timeIndex = ti
        w0 = np.ascontiguousarray(self._to_state(np.asarray(W0, dtype=np.float64)))
        w00 = None if W00 is None else np.ascontiguousarray(self._to_state(np.asarray(W00, dtype=np.float64)))
        check(lib().das_set_old_time_states(self._h, dptr(w0), dptr(w00) if w00 is not None else None, ti))

    def setOldTimeFields(self, phi=None, T_old=None):
        check(lib().das_set_old_time_fields(self._h, dptr(np.ascontiguousarray(phi)) if phi is not None else None,
                                            dptr(np.ascontiguousarray(T_old)) if T_old is not None else None))

    # -- objective functions ------------------------------------------------------------------------
    def _define_functions(self, functions):
        """"function" option dict (reference pyDAFoam.py DAOPTION.function): the patch-integral types force (directionMode
        fixedDirection), moment, massFlowRate, totalPressure, totalTemperatureRatio, totalPressureRatio, wallHeatFlux and
        location are on this path, as are the field-valued variableVolSum, patchMean and variance and the whole-mesh meshQualityKS and
        residualNorm."""
        names = [p.name for p in self._case.mesh.patches]
        L = lib()
        for fname, fd in (functions or {}).items():
            ftype = fd.get("type")
            if self._case.solver_name == "DAHeatTransferFoam" and ftype not in ("wallHeatFlux", "variableVolSum"):
                raise _capi.DASError(f"function {fname}: type {ftype} is not built for DAHeatTransferFoam (wallHeatFlux and variableVolSum of T are)")
            if ftype == "vonMisesStressKS":
                # DAFunctionVonMisesStressKS.C: source allCells / boxToCell, scale, coeffKS (required, as the reference reads it)
                if self._case.solver_name != "DASolidDisplacementFoam":
                    raise _capi.DASError(f"function {fname}: type vonMisesStressKS needs DASolidDisplacementFoam, not {self._case.solver_name}")
                if "coeffKS" not in fd:
                    raise _capi.DASError(f"function {fname}: vonMisesStressKS needs coeffKS")
                cells = self._function_cells(fname, fd)
                flags, ref = (8, float(np.atleast_1d(fd["ref"])[0])) if int(fd.get("calcRefVar", 0)) else (0, 0.0)
                check(L.das_define_von_mises_function(self._h, fname.encode(), cells.ctypes.data_as(_capi.c_int_p), cells.size, float(fd.get("scale", 1.0)),
                                                      float(fd["coeffKS"]), flags, ref))
                continue
            if self._case.solver_name == "DASolidDisplacementFoam" and not (ftype == "variableVolSum" and fd.get("varName") in ("D", "solid:rho")):
                raise _capi.DASError(f"function {fname}: type {ftype}" + (f" of {fd.get('varName')}" if ftype == "variableVolSum" else "") +
                                     " is not built for DASolidDisplacementFoam (vonMisesStressKS and variableVolSum of D and of solid:rho are)")
            if ftype in ("variableVolSum", "patchMean", "variance"):
                self._define_field_function(fname, fd)
                continue
            if ftype in ("meshQualityKS", "residualNorm"):
                self._define_mesh_function(fname, fd)
                continue
            if ftype not in ("force", "moment", "massFlowRate", "totalPressure", "totalTemperatureRatio", "totalPressureRatio", "wallHeatFlux",
                             "location"):
                raise NotImplementedError(f"function type {ftype} is outside the GPU hot path")
            ids = np.array([names.index(p) for p in fd["patches"]], dtype=np.int32)
            # calcRefVar / ref (DAFunction.C:44-49, 204-224; steady: the one reference value)
            flags, ref = 0, 0.0
            if int(fd.get("calcRefVar", 0)):
                flags, ref = 8, float(np.atleast_1d(fd["ref"])[0])
            if ftype == "location":
                self._define_location(fname, fd, ids, flags, ref)
                continue
            dmode = fd.get("directionMode", "fixedDirection") if ftype == "force" else None
            if dmode in ("parallelToFlow", "normalToFlow"):
                # the direction follows the angle of attack of a patchVelocity input (DAFunctionForce.C:45-61,92-113)
                pv = fd["patchVelocityInputName"]
                e = self._input_entry(pv, "patchVelocity")
                ax = {"x": 0, "y": 1, "z": 2}
                self._flowdir_fns[fname] = dict(mode=dmode, fi=ax[e["flowAxis"]], ni=ax[e["normalAxis"]], ids=ids, scale=float(fd.get("scale", 1.0)), pv=pv)
                self._define_flowdir(fname)
                continue
            if ftype == "force" and dmode != "fixedDirection":
                raise _capi.DASError(f"directionMode for {fname} not valid!Options: fixedDirection, parallelToFlow, normalToFlow.")
            grp = None
            gamma = 0.0
            vecA = vecB = None
            if ftype == "force":
                vecA = np.ascontiguousarray(fd["direction"], dtype=np.float64)
            elif ftype == "moment":
                vecA = np.ascontiguousarray(fd["axis"], dtype=np.float64)
                vecB = np.ascontiguousarray(fd["center"], dtype=np.float64)
            elif ftype in ("totalTemperatureRatio", "totalPressureRatio"):
                if ftype == "totalPressureRatio" and self._case.solver_name not in ("DARhoSimpleFoam", "DATurboFoam"):
                    raise _capi.DASError(f"totalPressureRatio function {fname} needs a compressible solver, not {self._case.solver_name}")
                inl, out = fd["inletPatches"], fd["outletPatches"]
                for p in fd["patches"]:
                    if p not in inl and p not in out:
                        raise _capi.DASError("inlet/outletPatches names are not in patches")
                grp = np.array([1 if p in out else 0 for p in fd["patches"]], dtype=np.int32)
                gamma = float(self._case.thermo.get("gamma", 1.4))
            elif ftype == "wallHeatFlux":
                # DAFunctionWallHeatFlux.C:44-52: the distance method is the top-level option, byUnitArea the function's own key
                wdm = self._wallDistanceMethod
                if wdm not in ("default", "daCustom"):
                    raise _capi.DASError(f"wallDistanceMethod: {wdm} not supported! Options are: default and daCustom.")
                flags |= (1 if bool(fd.get("byUnitArea", True)) else 0) | (2 if wdm == "daCustom" else 0)
            if ftype in ("totalPressureRatio", "wallHeatFlux"):
                check(L.das_define_face_function_ex(
                    self._h, fname.encode(), ftype.encode(), ids.ctypes.data_as(_capi.c_int_p),
                    grp.ctypes.data_as(_capi.c_int_p) if grp is not None else None, ids.size, None, None, float(fd.get("scale", 1.0)), gamma, flags, ref))
                continue
            check(L.das_define_face_function(
                self._h, fname.encode(), ftype.encode(), ids.ctypes.data_as(_capi.c_int_p),
                grp.ctypes.data_as(_capi.c_int_p) if grp is not None else None, ids.size,
                dptr(vecA) if vecA is not None else None, dptr(vecB) if vecB is not None else None, float(fd.get("scale", 1.0)), gamma))

    def _define_location(self, fname, fd, ids, flags, ref):
        """location (DAFunctionLocation.C:19-127): mode is required; coeffKS 1, axis (1, 0, 0) and center (0, 0, 0) are the reference's
        defaults.  snapCenter2Cell is not implemented."""
        if int(fd.get("snapCenter2Cell", 0)):
            raise _capi.DASError(f"location function {fname}: snapCenter2Cell is not implemented")
        if "mode" not in fd:
            raise _capi.DASError(f"location function {fname}: mode is required")
        axis = np.ascontiguousarray(fd.get("axis", [1.0, 0.0, 0.0]), dtype=np.float64)
        center = np.ascontiguousarray(fd.get("center", [0.0, 0.0, 0.0]), dtype=np.float64)
        check(lib().das_define_location_function(self._h, fname.encode(), str(fd["mode"]).encode(), ids.ctypes.data_as(_capi.c_int_p), ids.size,
                                                 dptr(axis), dptr(center), float(fd.get("coeffKS", 1.0)), flags, ref))

    def _define_mesh_function(self, fname, fd):
        """meshQualityKS (DAFunctionMeshQualityKS.C: coeffKS and metric are required; includeProcPatches means nothing without processor
        patches) and residualNorm (DAFunctionResidualNorm.C: resWeight is required, resMode L2Norm by default).  Neither applies scale."""
        flags, ref = (8, float(np.atleast_1d(fd["ref"])[0])) if int(fd.get("calcRefVar", 0)) else (0, 0.0)
        if fd["type"] == "meshQualityKS":
            for key in ("coeffKS", "metric"):
                if key not in fd:
                    raise _capi.DASError(f"function {fname}: meshQualityKS needs {key}")
            check(lib().das_define_mesh_quality_function(self._h, fname.encode(), str(fd["metric"]).encode(), float(fd["coeffKS"]), flags, ref))
            return
        if not isinstance(fd.get("resWeight"), dict):
            raise _capi.DASError(f"function {fname}: residualNorm needs the dictionary resWeight")
        names = [str(k).encode() for k in fd["resWeight"]]
        weights = np.array([float(w) for w in fd["resWeight"].values()], dtype=np.float64)
        check(lib().das_define_residual_norm_function(self._h, fname.encode(), (C.c_char_p * len(names))(*names), dptr(weights), len(names),
                                                      str(fd.get("resMode", "L2Norm")).encode(), flags, ref))

    def _function_cells(self, fname, fd):
        """cellSources of a cell-set function (DAFunction.C): "allCells", or "boxToCell" = the cells whose centre lies in the
        closed box min/max.  Selected once, at definition (a later updateOFMesh does not reselect)."""
        src = fd.get("source", "allCells")
        N = self._case.mesh.n_cells
        if src == "allCells":
            return np.arange(N, dtype=np.int32)
        if src == "boxToCell":
            if "min" not in fd or "max" not in fd:
                raise _capi.DASError(f"function {fname}: boxToCell needs min and max")
            C = self.geometry()["C"].reshape(-1, 3)  # the library's cell centres (OpenFOAM's boxToCell tests mesh.C())
            lo, hi = np.asarray(fd["min"], dtype=np.float64), np.asarray(fd["max"], dtype=np.float64)
            return np.nonzero(np.all((C >= lo) & (C <= hi), axis=1))[0].astype(np.int32)
        raise _capi.DASError(f"function {fname}: source {src} not supported (allCells, boxToCell)")

    def _define_field_function(self, fname, fd):
        """variableVolSum (DAFunctionVariableVolSum.C), patchMean (DAFunctionPatchMean.C), variance (DAFunctionVariance.C; modes
        field and surface) with the reference's keys and defaults.  timeOp / nStepsFrac / timeOpMaxMode mean nothing for a
        steady solve and are ignored."""
        ftype = fd["type"]
        var = fd.get("varName")
        vtype = fd.get("varType")
        if ftype == "variance":
            mode = fd.get("mode")
            if mode not in ("field", "surface"):
                raise _capi.DASError(f"variance {fname}: mode {mode} is not supported (field, surface; probePoint is not implemented)")
            if fd.get("timeDependentRefData", False):
                raise _capi.DASError(f"variance {fname}: timeDependentRefData is not supported (steady solvers)")
            if var in ("wallShearStress", "wallHeatFlux"):
                raise _capi.DASError(f"variance {fname}: varName {var} is not supported")
        if vtype not in ("scalar", "vector"):
            raise _capi.DASError(f"function {fname}: varType {vtype} not supported! Options are: scalar or vector")
        if ftype == "variance":
            if vtype == "vector" and "indices" not in fd:
                raise _capi.DASError(f"variance {fname}: a vector variable needs indices")
            comps = [int(i) for i in fd["indices"]] if vtype == "vector" else [0]
        else:
            comps = [int(fd.get("index", 0))] if vtype == "vector" else [0]
        comps = np.array(comps, dtype=np.int32)
        if (vtype == "vector") != (var in ("U", "D")):
            raise _capi.DASError(f"function {fname}: varType {vtype} does not match varName {var}")
        flags = (int(fd.get("isSquare", 0)) and 1) | (int(fd.get("multiplyVol", 1)) and 2) | (int(fd.get("divByTotalVol", 0)) and 4)
        ref = 0.0
        if ftype != "variance" and int(fd.get("calcRefVar", 0)):
            flags |= 8
            ref = float(np.atleast_1d(fd["ref"])[0])
        if int(fd.get("useGeoWeight", 0)):
            flags |= 16
        scale = float(fd.get("scale", 1.0))
        data = None
        surface = ftype == "patchMean" or (ftype == "variance" and fd["mode"] == "surface")
        if ftype == "variance":
            d = self._case.ref_data.get(var + "Data")
            if d is None:
                print(f"WARNING! Can't find data files or can't find valid values in data files for the variance function {var}")
            else:
                m = self._case.mesh
                if surface:
                    rows = np.concatenate([np.arange(p.start, p.start + p.size) for p in self._patches_of(fd)]) - m.n_internal_faces
                    vals = np.asarray(d["boundary"], dtype=np.float64)[rows]
                else:
                    vals = np.asarray(d["internal"], dtype=np.float64)
                data = vals.reshape(vals.shape[0], -1)
        L = lib()
        if surface:
            ids = np.array([self._case.mesh.patches.index(p) for p in self._patches_of(fd)], dtype=np.int32)
            if data is not None:
                data = np.ascontiguousarray(data[:, comps] if vtype == "vector" else data[:, :1])
            check(L.das_define_patch_field_function(self._h, fname.encode(), ftype.encode(), ids.ctypes.data_as(_capi.c_int_p), ids.size, str(var).encode(),
                                                    comps.ctypes.data_as(_capi.c_int_p), comps.size, dptr(data) if data is not None else None, flags, scale, ref))
            return
        cells = self._function_cells(fname, fd)
        if data is not None:
            data = np.ascontiguousarray(data[cells][:, comps] if vtype == "vector" else data[cells][:, :1])
        check(L.das_define_cell_function(self._h, fname.encode(), ftype.encode(), cells.ctypes.data_as(_capi.c_int_p), cells.size, str(var).encode(),
                                         comps.ctypes.data_as(_capi.c_int_p), comps.size, dptr(data) if data is not None else None, flags, scale, ref))

    def _patches_of(self, fd):
        if fd.get("source", "patchToFace") != "patchToFace":
            raise _capi.DASError(f"source {fd.get('source')} not valid for a boundary-value function (patchToFace)")
        by_name = {p.name: p for p in self._case.mesh.patches}
        return [by_name[p] for p in fd["patches"]]

    def _flow_direction(self, meta, deriv=False):
        """force direction of parallelToFlow / normalToFlow at the current AoA (deriv: d/dAoA[deg])"""
        a = self._patchVelocity[1] * np.pi / 180.0
        d = np.zeros(3)
        ca, sa = (np.cos(a), np.sin(a)) if not deriv else (-np.sin(a) * np.pi / 180.0, np.cos(a) * np.pi / 180.0)
        if meta["mode"] == "parallelToFlow":
            d[meta["fi"]], d[meta["ni"]] = ca, sa
        else:
            d[meta["fi"]], d[meta["ni"]] = -sa, ca
        return d

    def _define_flowdir(self, fname, name=None, direction=None):
        meta = self._flowdir_fns[fname]
        d = np.ascontiguousarray(self._flow_direction(meta) if direction is None else direction, dtype=np.float64)
        ids = meta["ids"]
        check(lib().das_define_face_function(self._h, (name or fname).encode(), b"force", ids.ctypes.data_as(_capi.c_int_p), None, ids.size,
                                             dptr(d), None, meta["scale"], 0.0))

    def _define_outputs(self, outputInfo):
        """"outputInfo" option dict (reference pyDAFoam.py DAOPTION.outputInfo): the entries of type forceCouplingOutput
        ({"type", "patches", "components": ["forceCoupling"], "pRef"}, DAOutputForceCoupling.C:38-41) and thermalCouplingOutput
        ({"type", "patches", "components": ["thermalCoupling"]}, DAOutputThermalCoupling.C:38-53) are defined on the device.  The
        reference sorts the patches by name before anything else and reads pRef unconditionally; so does this.  The thermal output
        reads the options `discipline` and `wallDistanceMethod`; discipline aero is the fluid side (the flow solvers), discipline
        thermal the solid side (DAHeatTransferFoam)."""
        for oname, od in (outputInfo or {}).items():
            otype = od.get("type")
            if otype not in ("forceCouplingOutput", "thermalCouplingOutput"):
                raise NotImplementedError(f"outputInfo[{oname}]: output type {otype} is not built (forceCouplingOutput and "
                                          "thermalCouplingOutput are)")
            thermal = otype == "thermalCouplingOutput"
            what = f"outputInfo[{oname}]"
            if self._case.solver_name == "DASolidDisplacementFoam":
                raise _capi.DASError(f"{what}: {otype} is not built for DASolidDisplacementFoam (the reference has no coupling output on the solid displacement)")
            if not thermal and self._case.solver_name == "DAHeatTransferFoam":
                raise _capi.DASError(f"{what}: forceCouplingOutput needs a flow solver with a pressure field (DAHeatTransferFoam has no p)")
            if thermal:
                flags = self._thermal_coupling_checks(what)
            elif "pRef" not in od:
                raise _capi.DASError(f"{what}: forceCouplingOutput needs pRef")
            patches, ids = self._sorted_patch_ids(f"{what}: {otype}", od)
            if thermal:
                check(lib().das_define_thermal_coupling(self._h, oname.encode(), ids.ctypes.data_as(_capi.c_int_p), ids.size, flags))
            else:
                check(lib().das_define_force_coupling(self._h, oname.encode(), ids.ctypes.data_as(_capi.c_int_p), ids.size, float(od["pRef"])))

    def _thermal_coupling_checks(self, what):
        """What the reference's DAOutputThermalCoupling / DAInputThermalCoupling constructors read besides the patches: the options
        `wallDistanceMethod` and `discipline`; and the solver must carry T.  Returns the flags of the C entries."""
        sn = self._case.solver_name
        if sn == "DAHeatTransferFoam":  # the solid side: [T_nearwall, kappa(T_b) / d], DAOutputThermalCoupling.C:212-241
            wdm = self._wallDistanceMethod
            if wdm not in ("default", "daCustom"):
                raise _capi.DASError(f"wallDistanceMethod: {wdm} not supported! Options are: default and daCustom.")
            if self._discipline != "thermal":
                raise _capi.DASError(f"{what}: the thermal coupling of DAHeatTransferFoam needs discipline thermal (discipline {self._discipline} "
                                     "is the fluid side, built for the flow solvers)")
            return 2 if wdm == "daCustom" else 0
        if not (sn in ("DARhoSimpleFoam", "DATurboFoam") or (sn == "DASimpleFoam" and getattr(self._case, "has_T", False))):
            raise NotImplementedError(f"{what}: the thermal coupling (thermalCouplingOutput and the thermalCoupling input) is not built for "
                                      f"solvers without a T field ({sn} here; DASimpleFoam with T, DARhoSimpleFoam and DATurboFoam carry one)")
        wdm = self._wallDistanceMethod
        if wdm not in ("default", "daCustom"):
            raise _capi.DASError(f"wallDistanceMethod: {wdm} not supported! Options are: default and daCustom.")
        if self._discipline != "aero":
            raise _capi.DASError(f"{what}: the thermal coupling is built for discipline aero only (discipline {self._discipline}: the "
                                 "solid solver DAHeatTransferFoam is not)")
        return 2 if wdm == "daCustom" else 0

    def _sorted_patch_ids(self, what, entry):
        names = [p.name for p in self._case.mesh.patches]
        patches = sorted(entry.get("patches") or [])
        if not patches:
            raise _capi.DASError(f"{what} needs patches")
        for p in patches:
            if p not in names:
                raise _capi.DASError(f"{what}: patch {p} is not in the mesh (patches: {', '.join(names)})")
        return patches, np.array([names.index(p) for p in patches], dtype=np.int32)

    def _define_thermal_inputs(self):
        """The inputInfo entries of type thermalCoupling ({"type", "patches", "components"}, DAInputThermalCoupling.C:35-64): the patches are
        sorted by name, and each must carry a mixed T (meshgen.BC_MIXED) - the reference's refCast<mixedFvPatchField> aborts otherwise."""
        from .meshgen import BC_MIXED

        for iname, e in self._inputInfo.items():
            if not isinstance(e, dict) or e.get("type") != "thermalCoupling":
                continue
            what = f"inputInfo[{iname}]"
            flags = self._thermal_coupling_checks(what)
            patches, ids = self._sorted_patch_ids(what, e)
            for p in patches:
                if self._case.bcs[p].get("T", (None,))[0] != BC_MIXED:
                    raise _capi.DASError(f"{what}: patch {p} does not carry a mixed T patch field (the thermalCoupling input writes its "
                                         "refValue and valueFraction)")
            check(lib().das_define_thermal_coupling_input(self._h, iname.encode(), ids.ctypes.data_as(_capi.c_int_p), ids.size, flags))

    # -- heat sources: the fvSource option of DAHeatTransferFoam (reference DAFvSourceHeatSource.C) and the fvSourcePar input ----------
    _HEAT_SOURCE_KEYS = {"cylinderToCell": ("p1", "p2", "radius", "power"),
                         "cylinderSmooth": ("center", "axis", "radius", "length", "power", "eps")}

    def _checked_fv_source(self, fvSource):
        """The fvSource option as the constructor accepts it: empty anywhere; on DAHeatTransferFoam entries of type heatSource with source
        cylinderToCell or cylinderSmooth and the keys of that source.  Everything else is refused, and every message carries the word
        fvSource and the entry's name."""
        fvSource = dict(fvSource or {})
        sn = self._case.solver_name
        for name, e in fvSource.items():
            what = f"fvSource[{name}]"
            if sn == "DASimpleFoam":
                self._check_actuator_disk(what, e)
                continue
            if sn != "DAHeatTransferFoam":
                why = " (its fvSourceEnergy = fvSource . U is not built)" if sn == "DARhoSimpleFoam" else ""
                raise _capi.DASError(f"{what}: the fvSource option is not built for {sn}{why} (actuator disks run on DASimpleFoam, heat sources on "
                                     "DAHeatTransferFoam)")
            if not isinstance(e, dict):
                raise _capi.DASError(f"{what}: a dictionary is expected")
            if e.get("type") != "heatSource":
                raise _capi.DASError(f"{what}: type {e.get('type')} is not built (actuatorDisk, actuatorLine, actuatorPoint and uniformPressureGradient "
                                     "are momentum sources; DAHeatTransferFoam takes type heatSource)")
            if "source" not in e:
                raise _capi.DASError(f"{what}: the key source is missing (cylinderToCell or cylinderSmooth)")
            if e["source"] not in self._HEAT_SOURCE_KEYS:
                raise _capi.DASError(f"{what}: source: {e['source']} not supported! Options are: cylinderToCell and cylinderSmooth!")
            missing = [k for k in self._HEAT_SOURCE_KEYS[e["source"]] if k not in e]
            if missing:
                raise _capi.DASError(f"{what}: source {e['source']} needs the key(s) {', '.join(missing)}")
            for k, n in (("p1", 3), ("p2", 3), ("center", 3), ("axis", 3)):
                if k in e and k in self._HEAT_SOURCE_KEYS[e["source"]] and np.size(e[k]) != n:
                    raise _capi.DASError(f"{what}: {k} needs {n} components")
        return fvSource

    # -- actuator disks: the fvSource option of DASimpleFoam (reference DAFvSourceActuatorDisk.C) ------------------------------------------
    _ACTUATOR_DISK_KEYS = {"cylinderAnnulusToCell": ("p1", "p2", "innerRadius", "outerRadius", "rotDir", "scale", "POD"),
                           "cylinderAnnulusSmooth": ("center", "direction", "innerRadius", "outerRadius", "rotDir", "scale", "POD", "eps", "expM", "expN")}
    # adjustThrust and targetThrust may be left out (0 and 0.0): the reference's own docstring example has neither
    ACTUATOR_DISK_PAR_NAMES = ("center_x", "center_y", "center_z", "direction_x", "direction_y", "direction_z", "innerRadius", "outerRadius", "scale", "POD",
                               "expM", "expN", "targetThrust")

    def _check_actuator_disk(self, what, e):
        """One fvSource entry on DASimpleFoam: type actuatorDisk with source cylinderAnnulusToCell or cylinderAnnulusSmooth and the keys of
        that source.  Every message names the entry and the solver."""
        sn = self._case.solver_name
        if not isinstance(e, dict):
            raise _capi.DASError(f"{what}: a dictionary is expected ({sn})")
        t = e.get("type")
        if t == "heatSource":
            raise _capi.DASError(f"{what}: type heatSource is not built for {sn} (heat sources run on DAHeatTransferFoam; {sn} takes type actuatorDisk)")
        if t != "actuatorDisk":
            raise _capi.DASError(f"{what}: type {t} is not built for {sn} (actuatorLine, actuatorPoint and uniformPressureGradient are not implemented; "
                                 "type actuatorDisk is)")
        if "source" not in e:
            raise _capi.DASError(f"{what}: the key source is missing (cylinderAnnulusToCell or cylinderAnnulusSmooth; {sn})")
        if e["source"] not in self._ACTUATOR_DISK_KEYS:
            raise _capi.DASError(f"{what}: source: {e['source']} not supported! Options are: cylinderAnnulusToCell and cylinderAnnulusSmooth! ({sn})")
        missing = [k for k in self._ACTUATOR_DISK_KEYS[e["source"]] if k not in e]
        if missing:
            raise _capi.DASError(f"{what}: source {e['source']} needs the key(s) {', '.join(missing)} ({sn})")
        for k in ("p1", "p2", "center", "direction"):
            if k in self._ACTUATOR_DISK_KEYS[e["source"]] and np.size(e[k]) != 3:
                raise _capi.DASError(f"{what}: {k} needs 3 components ({sn})")
        if e["rotDir"] not in ("left", "right"):
            raise _capi.DASError(f"{what}: rotDir not valid: {e['rotDir']} (left or right; {sn})")

    def _define_actuator_disks(self):
        for name in sorted(self._fvSource):
            e = self._fvSource[name]
            if e["source"] == "cylinderAnnulusToCell":
                pars = np.array(list(e["p1"]) + list(e["p2"]) + [e["innerRadius"], e["outerRadius"], e["scale"], e["POD"]], dtype=np.float64)
                eps, adjust = 0.0, 0
            else:
                pars = np.array(list(e["center"]) + list(e["direction"]) + [e.get(k, 0.0) for k in self.ACTUATOR_DISK_PAR_NAMES[6:]], dtype=np.float64)
                eps, adjust = float(e["eps"]), int(bool(e.get("adjustThrust", 0)))
            check(lib().das_define_actuator_disk(self._h, name.encode(), e["source"].encode(), dptr(pars), e["rotDir"].encode(), eps, adjust))

    def actuatorDiskInfo(self, name):
        """What the reference prints per disk, and more: the 13 actuatorDiskPars, the effective scale (the adjusted one with adjustThrust),
        thrustSourceSum = sum fAxial V and torqueSourceSum = sum fCirc V, the thrust at scale 1, the size of the cell set and, for a
        cylinderAnnulusToCell disk, its cells."""
        pars, info, nc = np.zeros(13), np.zeros(4), C.c_int(0)
        check(lib().das_get_actuator_disk_info(self._h, name.encode(), dptr(pars), dptr(info), C.byref(nc)))
        n = check(lib().das_get_actuator_disk_cells(self._h, name.encode(), None, 0))
        cells = np.zeros(n, dtype=np.int32)
        if n:
            check(lib().das_get_actuator_disk_cells(self._h, name.encode(), cells.ctypes.data_as(_capi.c_int_p), n))
        return dict(pars=pars, scale=float(info[0]), thrustSourceSum=float(info[1]), torqueSourceSum=float(info[2]), unitThrust=float(info[3]),
                    nCells=nc.value, cells=cells)

    # -- regression models: the regressionModel option of DASimpleFoam (reference DARegression.C) and the regressionPar input -----------------
    _REGRESSION_KEYS = ("modelType", "inputNames", "outputName", "inputShift", "inputScale", "outputShift", "outputScale", "outputUpperBound",
                        "outputLowerBound", "defaultOutputValue")

    def _define_regression_models(self, opt):
        """The regressionModel option (reference DARegression.C:34-147): {"active": ..., modelName: {...}, ...}.  Inactive or absent: nothing
        is defined and nothing changes.  The models are defined in the order of the dictionary; every refusal names the model and the key."""
        self._regressionModels = []
        if not isinstance(opt, dict) or not opt.get("active"):
            return
        sn = self._case.solver_name
        if sn != "DASimpleFoam":
            raise _capi.DASError(f"regressionModel: the option is built for DASimpleFoam only, not for {sn}")
        # (a variableVolSum objective over betaFINuTilda is refused by das_define_regression_model itself: the functions are defined by now)
        for iname, e in self._inputInfo.items():
            if e.get("type") == "field" and e.get("fieldName") == "betaFINuTilda":
                raise _capi.DASError(f"regressionModel: inputInfo[{iname}] is a field input on betaFINuTilda; the model would overwrite it in every residual "
                                     "evaluation")
        for name, e in opt.items():
            if name == "active":
                continue
            what = f"regressionModel[{name}]"
            if not isinstance(e, dict):
                raise _capi.DASError(f"{what}: a dictionary is expected")
            missing = [k for k in self._REGRESSION_KEYS if k not in e]
            if missing:
                raise _capi.DASError(f"{what}: the key(s) {', '.join(missing)} are missing")
            n = len(e["inputNames"])
            for k in ("inputShift", "inputScale"):
                if np.size(e[k]) != n:
                    raise _capi.DASError(f"{what}: inputNames has different sizes than {k} ({n} names, {np.size(e[k])} values)")
            if e["modelType"] == "neuralNetwork":
                for k in ("hiddenLayerNeurons", "activationFunction"):
                    if k not in e:
                        raise _capi.DASError(f"{what}: modelType neuralNetwork needs the key {k}")
            elif e["modelType"] == "radialBasisFunction" and "nRBFs" not in e:
                raise _capi.DASError(f"{what}: modelType radialBasisFunction needs the key nRBFs")
            sp = _capi.reg_spec(e)
            check(lib().das_define_regression_model(self._h, name.encode(), C.byref(sp)))
            self._regressionModels.append(name)

    def _regression_par_entry(self, inputName):
        """The parameter count of the model an inputInfo entry of type regressionPar drives: the entry is keyed by the MODEL name
        (reference DAInputRegressionPar.C:48)."""
        self._input_entry(inputName, "regressionPar")
        if inputName not in self._regressionModels:
            raise _capi.DASError(f"inputInfo[{inputName}]: type regressionPar, but regressionModel has no active model {inputName} (the entry is keyed by "
                                 f"the model name; models: {', '.join(self._regressionModels) or 'none'})")
        return check(lib().das_get_regression_n_parameters(self._h, inputName.encode()))

    def regressionModelInfo(self, name):
        """nParameters, nInputs and modelType of a model and, once the solver is initialised, the number of cells whose output was NaN, Inf
        and out of bounds at the current states (the reference's fail flag: any of them non-zero)."""
        nPar, nIn, mt = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().das_get_regression_model_info(self._h, name.encode(), C.byref(nPar), C.byref(nIn), C.byref(mt)))
        fail = np.zeros(3, dtype=np.int64)
        if self._inited:
            check(lib().das_get_regression_features(self._h, name.encode(), None, None, fail.ctypes.data_as(_capi.c_ll_p)))
        return dict(nParameters=nPar.value, nInputs=nIn.value, modelType=("neuralNetwork", "radialBasisFunction")[mt.value], nNaN=int(fail[0]),
                    nInf=int(fail[1]), nBounded=int(fail[2]), fail=int(fail.any()))

    def getRegressionFeatures(self, name):
        """(features (nCells, nInputs), output (nCells,)) of a model at the current states: what the reference's writeFeatures writes."""
        nIn = C.c_int(0)
        check(lib().das_get_regression_model_info(self._h, name.encode(), None, C.byref(nIn), None))
        n = self._case.mesh.n_cells
        feat, out = np.zeros((n, nIn.value)), np.zeros(n)
        check(lib().das_get_regression_features(self._h, name.encode(), dptr(feat), dptr(out), None))
        return feat, out

    def getRegressionParameters(self, name):
        out = np.zeros(check(lib().das_get_regression_n_parameters(self._h, name.encode())))
        check(lib().das_get_regression_parameters(self._h, name.encode(), dptr(out), out.size))
        return out

    def _define_fv_sources(self):
        """the entries of the fvSource option: actuator disks on DASimpleFoam, heat sources on DAHeatTransferFoam"""
        return self._define_actuator_disks() if self._case.solver_name == "DASimpleFoam" else self._define_heat_sources()

    def _define_heat_sources(self):
        for name in sorted(self._fvSource):
            e = self._fvSource[name]
            if e["source"] == "cylinderToCell":
                pars = np.array(list(e["p1"]) + list(e["p2"]) + [e["radius"], e["power"]], dtype=np.float64)
                eps, snap = 0.0, 0
            else:
                pars = np.array(list(e["center"]) + list(e["axis"]) + [e["radius"], e["length"], e["power"]], dtype=np.float64)
                eps, snap = float(e["eps"]), int(bool(e.get("snapCenter2Cell", 0)))
            check(lib().das_define_heat_source(self._h, name.encode(), e["source"].encode(), dptr(pars), eps, snap))

    def _fv_source_par_entry(self, inputName):
        """(fvSourceName, indices) of an inputInfo entry of type fvSourcePar (reference DAInputFvSourcePar.C:38-72: all nine by default)."""
        e = self._input_entry(inputName, "fvSourcePar")
        name = e.get("fvSourceName")
        if name not in self._fvSource:
            raise _capi.DASError(f"inputInfo[{inputName}]: fvSourceName {name} is not an entry of the fvSource option")
        disk = self._fvSource[name].get("type") == "actuatorDisk"
        smooth, pars, nPar, kind = ("cylinderAnnulusSmooth", "actuatorDiskPars", 13, "an actuator disk") if disk else ("cylinderSmooth", "heatSourcePars", 9, "a heat source")
        if self._fvSource[name]["source"] != smooth:
            raise _capi.DASError(f"inputInfo[{inputName}]: fvSource[{name}] is a {self._fvSource[name]['source']} source; the fvSourcePar input drives the "
                                 f"{pars}, which exist for {smooth} sources only")
        idx = np.array(e.get("indices", list(range(nPar))), dtype=np.int32)  # DAInputFvSourcePar.C:45-48: all 13 of a disk by default
        if idx.size and (idx.min() < 0 or idx.max() >= nPar):
            raise _capi.DASError(f"inputInfo[{inputName}]: index {int(idx.max() if idx.max() >= nPar else idx.min())} of fvSource[{name}] is out of range "
                                 f"({kind} has {nPar} parameters)")
        return name, np.ascontiguousarray(idx)

    def _is_actuator_disk(self, name):
        return self._fvSource[name].get("type") == "actuatorDisk"

    def updateFvSource(self):
        """DAFvSource::updateFvSource: the field follows the parameters and the metrics at once here (das_set_heat_source_pars,
        das_update_of_mesh); nothing is left to do."""
        return None

    def getFvSource(self):
        """The fvSource field: [W/m^3], one value per cell, on DAHeatTransferFoam; the momentum source of the actuator disks [force per unit
        volume], (nCells, 3), on DASimpleFoam."""
        if self._case.solver_name == "DASimpleFoam":
            out = np.zeros((self._case.mesh.n_cells, 3))
            check(lib().das_get_fv_source_vector(self._h, dptr(out)))
            return out
        out = np.zeros(self._case.mesh.n_cells)
        check(lib().das_get_fv_source(self._h, dptr(out)))
        return out

    def heatSourceInfo(self, name):
        """What the reference prints per source, and more: the parameters, volumeTotal (the total volume of the source), sourceTotal (the sum
        of fvSource V over the whole field [W]), the snapped cell and its centre (None without snapCenter2Cell), the cells of a
        cylinderToCell source."""
        pars, vt, st, cell = np.zeros(9), C.c_double(0.0), C.c_double(0.0), C.c_int(-1)
        check(lib().das_get_heat_source_info(self._h, name.encode(), dptr(pars), C.byref(vt), C.byref(st), C.byref(cell)))
        n = check(lib().das_get_heat_source_cells(self._h, name.encode(), None, 0))
        cells = np.zeros(n, dtype=np.int32)
        if n:
            check(lib().das_get_heat_source_cells(self._h, name.encode(), cells.ctypes.data_as(_capi.c_int_p), n))
        center = None
        if cell.value >= 0:
            Cc = np.zeros(3 * self._case.mesh.n_cells)
            check(lib().das_get_geometry(self._h, None, None, dptr(Cc), None, None, None, None, None))
            center = Cc[3 * cell.value:3 * cell.value + 3].copy()
        return dict(pars=pars, volumeTotal=vt.value, sourceTotal=st.value, snappedCell=(cell.value if cell.value >= 0 else None), snappedCenter=center,
                    cells=cells)

    def getPatchMixedT(self, patchName):
        """(refValue, valueFraction) of the faces of a patch with a mixed T, as they stand on the solver."""
        names = [p.name for p in self._case.mesh.patches]
        if patchName not in names:
            raise _capi.DASError(f"patch {patchName} is not in the mesh (patches: {', '.join(names)})")
        n = self._case.mesh.patches[names.index(patchName)].size
        ref, frac = np.zeros(n), np.zeros(n)
        check(lib().das_get_patch_mixed(self._h, names.index(patchName), dptr(ref), dptr(frac)))
        return ref, frac

    def calcFunction(self, functionName):
        v = C.c_double(0.0)
        check(lib().das_calc_function(self._h, functionName.encode(), C.byref(v)))
        return v.value

    # -- Krylov ----------------------------------------------------------------------------------
    def createMLRKSPMatrixFree(self, jacPCMat: Mat, myKSP: KSP):
        h = C.c_void_p()
        check(lib().das_create_ml_rksp_matrix_free(self._h, jacPCMat.handle, C.byref(h)))
        myKSP.destroy()
        myKSP.handle = h
        myKSP._pc = jacPCMat  # keep the PC matrix alive as long as the KSP
        myKSP._n = self.getNLocalAdjointStates()

    def updateKSPPCMat(self, PCMat: Mat, myKSP: KSP):
        self.createMLRKSPMatrixFree(PCMat, myKSP)

    def solveLinearEqn(self, myKSP: KSP, rhsVec: Vec, solVec: Vec):
        L = lib()
        for k, v in myKSP._tols.items():
            (L.das_set_option_int if isinstance(v, int) else L.das_set_option_double)(self._h, k.encode(), v)
        if self._perm is None:
            return check(L.das_solve_linear_eqn(self._h, myKSP.handle, dptr(rhsVec.array), dptr(solVec.array)))
        rhs, sol = np.ascontiguousarray(self._to_state(rhsVec.array)), np.ascontiguousarray(self._to_state(solVec.array))
        rc = check(L.das_solve_linear_eqn(self._h, myKSP.handle, dptr(rhs), dptr(sol)))
        self._from_state(sol, solVec.array)
        return rc

    def solvePrimal(self, maxSteps=80, relTol=1e-8, absTol=0.0):
        """solvePrimal (reference pyDASolvers.pyx solvePrimal -> DASimpleFoam::solvePrimal, DASimpleFoam.C:123-185): converge
        the residuals from the current states.  Returns (fail, info) with info = dict(steps, linearIterations, res0, res,
        history); the converged states are read back with getOFFields / getStates."""
        if self._case.solver_name == "DAHeatTransferFoam" and not any(
                p.size > 0 and self._case.bcs.get(p.name, {}).get("T", (1, 0.0))[0] in (0, BC_MIXED) for p in self._case.mesh.patches):
            raise _capi.DASError("DAHeatTransferFoam: no patch carries a fixedValue or mixed T - the steady conduction problem is singular")
        if self._case.solver_name == "DASolidDisplacementFoam" and not any(
                p.size > 0 and self._case.bcs.get(p.name, {}).get("D", (1, 0.0))[0] == 0 for p in self._case.mesh.patches):
            raise _capi.DASError("DASolidDisplacementFoam: no patch carries a fixedValue D - the steady elastic problem is singular")
        if self._pimple:
            return self._solve_primal_unsteady(maxSteps, relTol, absTol)
        info4 = np.zeros(4)
        hist = np.zeros(int(maxSteps) + 2)
        rc = check(lib().das_solve_primal(self._h, int(maxSteps), float(relTol), float(absTol), dptr(info4), dptr(hist), hist.size))
        nst = int(info4[0])
        return rc, dict(steps=nst, linearIterations=int(info4[1]), res0=float(info4[2]), res=float(info4[3]), history=hist[: nst + 1].copy())

    # -- DAPimpleFoam: what is refused, the marching primal, the time operators and the time-accurate adjoint ------------------------------
    # the patch-integral types an incompressible solver without a T field can evaluate, and variableVolSum
    _PIMPLE_FUNCTIONS = ("force", "moment", "massFlowRate", "totalPressure", "location", "variableVolSum")

    def _pimple_checks(self, opt):
        """What DAPimpleFoam does not build is refused by name before anything is created."""
        case = self._case
        if getattr(case, "has_T", False):
            raise _capi.DASError("DAPimpleFoam: the T field is not built")
        if getattr(case, "mrf", None):
            raise _capi.DASError("DAPimpleFoam: MRF is not built")
        if any(p.type == "cyclic" for p in case.mesh.patches):
            raise _capi.DASError("DAPimpleFoam: cyclic patches are not built")
        if getattr(case, "simple_consistent", False):
            raise _capi.DASError("DAPimpleFoam: simple_consistent is not built")
        if case.ddt_scheme not in _capi.DDT_SCHEMES:
            raise _capi.DASError(f"ddtScheme {case.ddt_scheme} not supported! Options: steadyState, Euler, or backward")
        if opt.get("fvSource"):
            raise _capi.DASError(f"fvSource[{sorted(opt['fvSource'])[0]}]: the fvSource option is not built for DAPimpleFoam")
        if opt.get("regressionModel") and (opt["regressionModel"].get("active", True) if isinstance(opt["regressionModel"], dict) else True):
            raise _capi.DASError("regressionModel: the option is not built for DAPimpleFoam")
        if opt.get("outputInfo"):
            raise _capi.DASError(f"outputInfo[{sorted(opt['outputInfo'])[0]}]: coupling outputs are not built for DAPimpleFoam")
        for nm, e in (opt.get("inputInfo") or {}).items():
            if isinstance(e, dict) and e.get("type") in ("forceCoupling", "thermalCoupling", "thermalCouplingInput"):
                raise _capi.DASError(f"inputInfo[{nm}]: coupling inputs ({e.get('type')}) are not built for DAPimpleFoam")
        if (opt.get("dynamicMesh") or {}).get("active"):
            raise _capi.DASError("DAPimpleFoam: dynamicMesh is not built")
        if opt.get("runFPAdj") or opt.get("adjEqnSolMethod", "Krylov") != "Krylov":
            raise _capi.DASError("DAPimpleFoam: runFPAdj / adjEqnSolMethod fixedPoint is not built (the time-accurate adjoint is Krylov only)")
        for fname, fd in (opt.get("function") or {}).items():
            if fd.get("type") not in self._PIMPLE_FUNCTIONS:
                raise _capi.DASError(f"function {fname}: type {fd.get('type')} is not built for DAPimpleFoam (the patch-integral types and variableVolSum are)")
            if fd.get("timeOp", "final") not in ("final", "average"):
                raise _capi.DASError(f"function {fname}: timeOp {fd.get('timeOp')} is not built for DAPimpleFoam (final and average are)")
        self._functionDefs = {k: dict(v) for k, v in (opt.get("function") or {}).items()}

    def _time_op_range(self, functionName):
        """(timeOp, startIdx, endIdx) over the list of the marched steps: DASolver::getTimeOpRange (DASolver.C:404-422) - final: the
        whole list; average: the trailing window max(2, round(nStepsFrac (listEnd + 1))), nStepsFrac 0.2 unless the function sets it."""
        fd = self._functionDefs.get(functionName)
        if fd is None:
            raise _capi.DASError(f"functionName {functionName} not found!")
        op = fd.get("timeOp", "final")
        end = int(self._case.n_steps) - 1
        start = 0
        if op == "average":
            window = max(2, int(np.floor(float(fd.get("nStepsFrac", 0.2)) * (end + 1) + 0.5)))  # Foam::round: half away from zero
            start = max(0, end - window + 1)
        return op, start, end

    def getTimeInstance(self, n):
        """The states of time index n of the marched series (0: the start), the ordering of getOFFields."""
        series = getattr(self, "_series", None)
        if series is None or not 0 <= int(n) < len(series):
            raise _capi.DASError(f"getTimeInstance: time index {n} is not in the marched series (solvePrimal first)")
        return series[int(n)].copy()

    def _set_time_instance(self, n):
        """states and old-time states of time index n >= 1 from the series; before the start the flow is taken as steady: W(-1) = W(0)"""
        ser = self._series
        self.setOldTimeStates(ser[n - 1], ser[max(n - 2, 0)], n)  # one upload, with the index
        self.setTime(n * self.getDeltaT(), n)
        self.updateOFFields(ser[n])

    def _solve_primal_unsteady(self, maxSteps, relTol, absTol):
        """n_steps time steps, each the Newton solve of R(W; W0, W00) = 0 started from the step before; the series stays in memory"""
        n = self.getNLocalAdjointStates()
        W = np.zeros(n)
        self.getOFFields(W)
        self._series = [W.copy()]
        self._functionTimeSteps = {k: [] for k in self._functionDefs}
        infos, rc_all = [], 0
        for step in range(1, int(self._case.n_steps) + 1):
            self.setOldTimeStates(self._series[step - 1], self._series[max(step - 2, 0)], step)  # one upload, with the index
            self.setTime(step * self.getDeltaT(), step)
            info4 = np.zeros(4)
            hist = np.zeros(int(maxSteps) + 2)
            rc = check(lib().das_solve_primal(self._h, int(maxSteps), float(relTol), float(absTol), dptr(info4), dptr(hist), hist.size))
            rc_all = max(rc_all, rc)
            self.getOFFields(W)
            self._series.append(W.copy())
            for k in self._functionTimeSteps:
                self._functionTimeSteps[k].append(self.calcFunction(k))
            nst = int(info4[0])
            infos.append(dict(steps=nst, linearIterations=int(info4[1]), res0=float(info4[2]), res=float(info4[3]), history=hist[: nst + 1].copy()))
        last = infos[-1]
        return rc_all, dict(steps=sum(i["steps"] for i in infos), linearIterations=sum(i["linearIterations"] for i in infos), res0=infos[0]["res0"],
                            res=max(i["res"] for i in infos), history=last["history"], timeSteps=infos)

    def simpleIteration(self, nSweeps=1, alphaP=0.3, linTol=1e-12, maxLinIters=20000):
        """nSweeps iterations of the reference's own primal loop, SIMPLE (DASimpleFoam::solvePrimal, DASimpleFoam.C:123-185: UEqnSimple.H,
        pEqnSimple.H, DASpalartAllmaras::correct), on the device from the current states (das_simple_iteration); alphaP = the explicit
        pressure relaxation of fvSolution, linTol / maxLinIters = the inner solvers' settings.  Returns the inner iteration counts of the
        last sweep; the new states are read with getOFFields / getStates."""
        if self._case.solver_name == "DASolidDisplacementFoam":
            raise _capi.DASError("simpleIteration: the SIMPLE sweep is not built for DASolidDisplacementFoam (use solvePrimal)")
        info = np.zeros(3)
        check(lib().das_simple_iteration(self._h, int(nSweeps), float(alphaP), float(linTol), int(maxLinIters), dptr(info)))
        return dict(U=int(info[0]), p=int(info[1]), nuTilda=int(info[2]))

    def solveLinearEqnBlock(self, myKSP: KSP, rhs, sol):
        """Several adjoint systems with the same operator through ONE block GMRES (the reference loops solveLinearEqn over
        the objective functions, mphys_dafoam.py:478-481).  rhs, sol: (n, s) arrays, s <= 8; returns (fail, res0[s], res[s])."""
        L = lib()
        for k, v in myKSP._tols.items():
            (L.das_set_option_int if isinstance(v, int) else L.das_set_option_double)(self._h, k.encode(), v)
        rhs = np.asarray(rhs, dtype=np.float64)
        n, s = rhs.shape
        if self._perm is not None:
            rhs = np.stack([self._to_state(rhs[:, r]) for r in range(s)], axis=1)
        B = np.asfortranarray(rhs)
        X = np.zeros((n, s), order="F")
        r0, r1 = np.zeros(s), np.zeros(s)
        rc = check(L.das_solve_linear_eqn_block(self._h, myKSP.handle, int(s), B.ctypes.data_as(_capi.c_double_p), X.ctypes.data_as(_capi.c_double_p),
                                                dptr(r0), dptr(r1)))
        for r in range(s):
            if self._perm is None:
                sol[:, r] = X[:, r]
            else:
                self._from_state(np.ascontiguousarray(X[:, r]), sol[:, r])
        return rc, r0, r1

    # -- timing ----------------------------------------------------------------------------------
    def _state_blocks(self):
        """[(name, kind, offset, size)] of the DAIndex "state" ordering (reference DAIndex.C:188-258)."""
        m = self._case.mesh
        N, F = m.n_cells, m.n_faces
        names = {"DASimpleFoam": ["U", "p"] + (["T"] if getattr(self._case, "has_T", False) else []) + ["nuTilda", "phi"],
                 "DAPimpleFoam": ["U", "p", "nuTilda", "phi"],
                 "DARhoSimpleFoam": ["U", "p", "T", "nuTilda", "phi"], "DATurboFoam": ["U", "p", "T", "nuTilda", "phi"],
                 "DAScalarTransportFoam": ["T"], "DAHeatTransferFoam": ["T"], "DASolidDisplacementFoam": ["D"]}[self._case.solver_name]
        out, off = [], 0
        for nm in names:
            kind = "vec" if nm in ("U", "D") else ("face" if nm == "phi" else "scl")
            size = {"vec": 3 * N, "scl": N, "face": F}[kind]
            out.append((nm, kind, off, size))
            off += size
        return out

    def calcPrimalResidualStatistics(self, mode, writeRes=0):
        """DASolver::calcPrimalResidualStatistics (reference DASolver.C:745-946): norm2 / mean / max of every residual
        block at the current states; printed for mode "print", only computed for "calc".  Returns the numbers (the
        reference keeps them internal): {resName: {"norm2", "mean", "max"}, "totalResNorm2": ...}."""
        if mode not in ("print", "calc"):
            raise _capi.DASError("mode not valid")
        n = self.getNLocalAdjointStates()
        R = np.zeros(n)
        check(lib().das_get_residuals(self._h, dptr(R)))
        stats, tot = {}, 0.0
        if mode == "print":
            print("Printing Primal Residual Statistics.")
        for nm, kind, off, size in self._state_blocks():
            blk = R[off : off + size]
            if kind == "vec":
                blk = blk.reshape(-1, 3)
                st = {"norm2": np.sqrt((blk * blk).sum(0)), "mean": np.abs(blk).mean(0), "max": np.abs(blk).max(0)}
            else:
                st = {"norm2": float(np.sqrt((blk * blk).sum())), "mean": float(np.abs(blk).mean()), "max": float(np.abs(blk).max())}
            tot += float((blk * blk).sum())
            stats[nm + "Res"] = st
            if mode == "print":
                print(f"{nm} Residual Norm2: {st['norm2']}\n{nm} Residual Mean: {st['mean']}\n{nm} Residual Max: {st['max']}")
        stats["totalResNorm2"] = float(np.sqrt(tot))
        if mode == "print":
            print(f"Total Residual Norm2: {stats['totalResNorm2']}")
        return stats

    def writeAdjointFields(self, function, writeTime, psi, caseDir="."):
        """DASolver::writeAdjointFields (reference DASolver.C:4055-4160, pyDASolvers.pyx:470): psi as OpenFOAM fields
        adjoint_<function>_<state> under <caseDir>/<writeTime>/ (the reference writes into its case directory)."""
        from . import foam_io

        assert len(psi) == self.getNLocalAdjointStates(), "invalid array size!"
        psi_s = np.ascontiguousarray(self._to_state(np.asarray(psi, dtype=np.float64)))
        return foam_io.write_adjoint_fields(caseDir, self._case, function, writeTime, psi_s, self._state_blocks())

    # -- the rest of the reference's pyDASolvers surface that a runScript / mphys_dafoam.py touches around the hot path ------
    caseDir = "."  # where the IO methods read / write (the reference runs inside its case directory)

    def calcOutput(self, outputName, outputType, output):
        """pyDASolvers.pyx:204-206 -> DAOutput::run: the function value (1 entry), the residual vector (state ordering of the
        caller: adjStateOrdering), the nodal forces of a forceCouplingOutput or the [T, kappa / d] of a thermalCouplingOutput at the
        current states."""
        assert len(output) == self.getOutputSize(outputName, outputType), "invalid array size!"
        if outputType == "function":
            output[0] = self.calcFunction(outputName)
        elif outputType == "residual":
            R = np.zeros(self.getNLocalAdjointStates())
            self.getResiduals(R)
            output[:] = R
        elif outputType in ("forceCouplingOutput", "thermalCouplingOutput"):
            # DAOutputForceCoupling::run: [fx0, fy0, fz0, fx1, ...] over the points of the (sorted) patches; DAOutputThermalCoupling::run:
            # T of the owner cells, then kappa / d, over the faces of the (sorted) patches
            out = output if isinstance(output, np.ndarray) and output.dtype == np.float64 and output.flags["C_CONTIGUOUS"] else np.zeros(len(output))
            calc = lib().das_calc_force_coupling if outputType == "forceCouplingOutput" else lib().das_calc_thermal_coupling
            check(calc(self._h, outputName.encode(), dptr(out), len(out)))
            if out is not output:
                output[:] = out
        else:
            raise _capi.DASError(f"outputType not supported on this path: {outputType}")

    def hasVolCoordInput(self):
        """DASolver::hasVolCoordInput (DASolver.C:4149-4164): 1 if an inputInfo entry has type volCoord."""
        return int(any(isinstance(e, dict) and e.get("type") == "volCoord" for e in self._inputInfo.values()))

    def getInputDistributed(self, inputName, inputType):
        """DAInput*::distributed(): 1 for inputs that are partitioned over the ranks (DAInputStateVar.H:57, DAInputVolCoord.H:57; a
        field input says so itself, DAInputField.H:110-114), 0 for the global ones (patchVelocity, patchVar)."""
        if inputType in ("stateVar", "volCoord"):
            return 1
        if inputType == "thermalCoupling":  # DAInputThermalCoupling.H
            self._input_entry(inputName, inputType)
            return 1
        if inputType == "field":
            return int(self._field_entry(inputName).get("distributed", 1))
        if inputType in ("patchVelocity", "patchVar"):
            return 0
        raise _capi.DASError(f"inputType not supported on this path: {inputType}")

    def getOutputDistributed(self, outputName, outputType):
        """DAOutputResidual.H:59 (1), DAOutputFunction.H:76 (0), DAOutputForceCoupling.H (1), DAOutputThermalCoupling.H (1)."""
        if outputType == "residual":
            return 1
        if outputType in ("forceCouplingOutput", "thermalCouplingOutput"):
            self.getOutputSize(outputName, outputType)  # an unknown name is an error here as well
            return 1
        if outputType == "function":
            return 0
        raise _capi.DASError(f"outputType not supported on this path: {outputType}")

    def getOFField(self, fieldName, fieldType, field):
        """pyDASolvers.pyx:283-289: the internal field `fieldName` (a state of this solver) of the current states, cell by cell
        (vectors interleaved xyz)."""
        N = self.getNLocalCells()
        assert len(field) == (3 * N if fieldType == "vector" else N), "invalid array size!"
        W = np.zeros(self.getNLocalAdjointStates())
        check(lib().das_get_of_fields(self._h, dptr(W)))
        for nm, kind, off, size in self._state_blocks():
            if nm == fieldName and kind != "face":
                if (kind == "vec") != (fieldType == "vector"):
                    raise _capi.DASError(f"fieldType {fieldType} does not match field {fieldName}")
                field[:] = W[off : off + size]
                return
        raise _capi.DASError(f"field {fieldName} is not a cell-centred state of {self._case.solver_name}")

    def getOFFieldGlobal(self, fieldName, fieldType, field):
        """pyDASolvers.pyx:291-295 (the field gathered over all ranks): one domain here - the sharded wrapper owns the gather."""
        if self.getNGlobalCells() != self.getNLocalCells():
            raise _capi.DASError("getOFFieldGlobal on a sharded solver: gather through dafoam_amd.distributed")
        return self.getOFField(fieldName, fieldType, field)

    def getGlobalXvIndex(self, pointI, coordI):
        """DAIndex::getGlobalXvIndex (DAIndex.C:757-775): 3 * (global point) + coordinate; one domain: the local numbering."""
        assert 0 <= pointI < self.getNLocalPoints() and 0 <= coordI < 3
        return 3 * int(pointI) + int(coordI)

    def checkMesh(self):
        """DASolver::checkMesh -> DACheckMesh::run (DACheckMesh.C:49-77: OpenFOAM's checkGeometry with the thresholds of the
        checkMeshThreshold option): 1 = mesh quality passes.  Checked here on the library's metrics: cell volumes > 0, face
        orientation d.Sf > 0 (at most maxIncorrectlyOrientedFaces violations), non-orthogonality angle, skewness (distance of
        the face centre from the point where the line of centres meets the face, over |d|, OpenFOAM primitiveMeshTools::
        faceSkewness) and cell aspect ratio (primitiveMeshTools::cellClosedness) below the thresholds."""
        th = dict(maxAspectRatio=1000.0, maxNonOrth=70.0, maxSkewness=4.0, maxIncorrectlyOrientedFaces=0)
        th.update({k: (v[1] if isinstance(v, list) else v) for k, v in self._checkMeshThreshold.items()})
        g = self.geometry()
        m = self._case.mesh
        nIF, N = m.n_internal_faces, m.n_cells
        own, nei = np.asarray(m.owner), np.asarray(m.neighbour)
        Sf, Cf, Cc, V = g["Sf"].reshape(-1, 3), g["Cf"].reshape(-1, 3), g["C"].reshape(-1, 3), g["V"]
        self.meshQuality = q = {}
        q["minVolume"] = float(V.min())
        d = Cc[nei] - Cc[own[:nIF]]
        dn = np.einsum("ij,ij->i", d, Sf[:nIF])
        magd, magS = np.linalg.norm(d, axis=1), np.linalg.norm(Sf[:nIF], axis=1)
        q["incorrectlyOrientedFaces"] = int(np.count_nonzero(dn <= 0))
        cosang = np.clip(dn / np.maximum(magd * magS, 1e-300), -1.0, 1.0)
        q["maxNonOrth"] = float(np.degrees(np.arccos(cosang)).max()) if nIF else 0.0
        t = np.einsum("ij,ij->i", Cf[:nIF] - Cc[own[:nIF]], Sf[:nIF]) / np.where(dn != 0, dn, 1.0)
        sk = np.linalg.norm(Cf[:nIF] - (Cc[own[:nIF]] + t[:, None] * d), axis=1) / np.maximum(magd, 1e-300)
        q["maxSkewness"] = float(sk.max()) if nIF else 0.0
        sumMag = np.zeros((N, 3))
        absS = np.abs(Sf)
        for k in range(3):
            sumMag[:, k] = np.bincount(own, absS[:, k], N) + np.bincount(nei, absS[:nIF, k], N)
        lo = np.maximum(sumMag.min(axis=1), 1e-300)
        q["maxAspectRatio"] = float(np.maximum(sumMag.max(axis=1) / lo, sumMag.sum(axis=1) / 6.0 / np.maximum(V, 1e-300) ** (2.0 / 3.0)).max())
        ok = (q["minVolume"] > 0 and q["incorrectlyOrientedFaces"] <= th["maxIncorrectlyOrientedFaces"] and q["maxNonOrth"] <= th["maxNonOrth"]
              and q["maxSkewness"] <= th["maxSkewness"] and q["maxAspectRatio"] <= th["maxAspectRatio"])
        return int(ok)

    # time bookkeeping of the steady solvers (pyDASolvers.pyx:358,400-410,464): iterations play the role of time
    def setTime(self, time, timeIndex):
        self._time, self._timeIndex = float(time), int(timeIndex)
        if self._pimple:  # the ddt coefficients follow the time index (backward below 2 is Euler); the old states on the device stay
            check(lib().das_set_time_index(self._h, int(timeIndex)))

    def getDeltaT(self):
        return float(getattr(self._case, "deltaT", 1.0))

    def getEndTime(self):
        return float(getattr(self, "_endTime", getattr(self, "_time", 0.0)))

    def getLatestTime(self):
        return float(getattr(self, "_time", 0.0))

    def getPrevPrimalSolTime(self):
        return float(getattr(self, "_prevPrimalSolTime", getattr(self, "_time", 0.0)))

    def getDdtSchemeOrder(self):
        """1 (Euler) for the unsteady scalar transport residual, the steady solvers have no time derivative (DASolver::getDdtSchemeOrder);
        DAPimpleFoam: 1 for Euler, 2 for backward."""
        if self._pimple:
            return 2 if self._case.ddt_scheme == "backward" else 1
        return 1

    def getdFScaling(self, functionName, timeIdx=-1):
        """DASolver::getdFScaling: the weight of a time instance in a time-averaged objective; 1 for steady solvers.  DAPimpleFoam: the
        function's timeOp (final | average with nStepsFrac) over the marched series, timeIdx = time index - 1 (DASolver.C:454-482):
        average - 1 / window inside the trailing window, 0 before it; final - 1 at the last step and 0 before it.  DATimeOpFinal::dFScaling
        returns 1 at every index of the list, which is the derivative of the SUM over the steps, not of the final value (measured on the
        6-step channel of tests/test_gpu_pimple.py: 0.2227 = 6 x the average's 0.0371, against central differences 0.00116); what is built
        here is the derivative of what DATimeOpFinal::compute returns."""
        if not self._pimple:
            return 1.0
        op, i0, i1 = self._time_op_range(functionName)
        if not i0 <= int(timeIdx) <= i1:
            return 0.0
        if op == "final":
            return 1.0 if int(timeIdx) == i1 else 0.0
        return 1.0 / (i1 - i0 + 1)

    def getTimeOpFuncVal(self, functionName):
        """DASolver::getTimeOpFuncVal: the time-operated (final / averaged) objective; steady solvers: the value at the current states.
        DAPimpleFoam: DATimeOpFinal / DATimeOpAverage over the function values of the marched series (DASolver.C:424-451)."""
        if not self._pimple:
            return self.calcFunction(functionName)
        op, i0, i1 = self._time_op_range(functionName)
        vals = self._functionTimeSteps[functionName]
        if op == "final":
            return float(vals[i1])
        avg = 0.0
        for i in range(i0, i1 + 1):
            avg += vals[i]
        return float(avg / (i1 - i0 + 1))

    def updateBoundaryConditions(self, fieldName, fieldType):
        """pyDASolvers.pyx:364: boundary values are re-evaluated inline by every kernel from the states - nothing is stored."""
        return None

    def setPrimalBoundaryConditions(self, printInfo=1):
        """DASolver::setPrimalBoundaryConditions (DASolver.C:3790-4030): the primalBC option {name: {variable, patches, value}}
        written into the patch table (fixedValue / inletOutlet patches)."""
        for name, e in (self._primalBC or {}).items():
            if not isinstance(e, dict) or "variable" not in e:
                continue
            ids = np.ascontiguousarray(self._patch_ids(e), dtype=np.int32)
            val = np.ascontiguousarray(np.atleast_1d(np.asarray(e["value"], dtype=np.float64)))
            check(lib().das_set_patch_value(self._h, ids.ctypes.data_as(_capi.c_int_p), ids.size, str(e["variable"]).encode(), dptr(val)))
            if printInfo:
                print(f"primalBC {name}: {e['variable']} on {e['patches']} = {val.tolist()}")

    # mesh / state files (pyDASolvers.pyx:361,382-395 -> DASolver::readMeshPoints / writeMeshPoints / readStateVars)
    def _points_path(self, timeVal):
        import os

        return os.path.join(self.caseDir, ("%g" % timeVal) if timeVal is not None else "constant", "polyMesh", "points")

    def writeMeshPoints(self, points, timeVal):
        from . import foam_io

        assert len(points) == self.getNLocalPoints() * 3, "invalid array size!"
        foam_io.write_points(self._points_path(timeVal), np.asarray(points, dtype=np.float64).reshape(-1, 3))

    def readMeshPoints(self, timeVal):
        from . import foam_io

        self.updateOFMesh(np.ascontiguousarray(foam_io.read_points(self._points_path(timeVal)).ravel()))

    def writeCurrentMeshPointsToConstant(self):
        X = np.zeros(self.getNLocalPoints() * 3)
        self.getOFMeshPoints(X)
        self.writeMeshPoints(X, None)

    def writeFailedMesh(self):
        """DASolver::writeFailedMesh: the current points under the time directory 9999 for inspection (pyDAFoam.py:1240-1256)."""
        X = np.zeros(self.getNLocalPoints() * 3)
        self.getOFMeshPoints(X)
        self.writeMeshPoints(X, 9999)

    def readStateVars(self, timeVal, timeLevel=0):
        """DASolver::readStateVars (DASolver.C:3478-3600): the state fields of time directory timeVal -> the solver (timeLevel 0)."""
        import os

        from . import foam_io

        if timeLevel != 0:
            raise _capi.DASError("readStateVars: old-time levels are set through setOldTimeFields on this path")
        m = self._case.mesh
        N = m.n_cells
        tdir = os.path.join(self.caseDir, "%g" % timeVal)
        W = np.zeros(self.getNLocalAdjointStates())
        check(lib().das_get_of_fields(self._h, dptr(W)))
        for nm, kind, off, size in self._state_blocks():
            path = os.path.join(tdir, nm)
            if kind == "face" or not os.path.exists(path):
                continue  # phi is a derived field in a time directory written by a primal (kept as it is here)
            vals, _ = foam_io.read_field(path, N, 3 if kind == "vec" else 1)
            W[off : off + size] = np.asarray(vals, dtype=np.float64).ravel()
        check(lib().das_update_of_fields(self._h, dptr(W)))

    def getElapsedClockTime(self):
        return lib().das_get_elapsed_clock_time(self._h)

    def getElapsedCpuTime(self):
        return lib().das_get_elapsed_cpu_time(self._h)

    # -- not on the hot path -----------------------------------------------------------------------

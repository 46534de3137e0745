/*
 * dafoam_amd.h - C-ABI of the MI355X-native discrete-adjoint hot path.
 *
 * Drop-in boundary: these entry points are what the reference's Cython layer
 * (reference src/pyDASolvers/pyDASolvers.pyx:45-114 extern block, :117-482 class
 * pyDASolvers, wrapping src/pyDASolvers/DASolvers.H) would bind for the adjoint
 * path.  Conventions follow the reference: caller-owned
 * 1-D contiguous float64 buffers borrowed for the call and written in place;
 * strings are NUL-terminated char*; soft failures are integer returns; hard
 * failures return a negative code and set das_last_error() (the reference
 * aborts the process via OpenFOAM FatalError, e.g. DASolver.C:992-993).
 * No exceptions, no C++/torch types cross this boundary.
 *
 * PETSc objects of the reference API (Mat dRdWT / Mat dRdWTPC / KSP, created by the
 * Python caller in reference dafoam/mphys/mphys_dafoam.py:468-475,519-529) are
 * replaced by opaque device-resident handles das_mat_t / das_ksp_t.
 *
 * All compute entry points run on the GPU; they FAIL (return DAS_ERR_NO_DEVICE)
 * when no HIP device is present - there is no CPU fallback.
 */
#ifndef DAFOAM_AMD_H
#define DAFOAM_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define DAS_OK 0
#define DAS_ERR_ARG -1
#define DAS_ERR_NO_DEVICE -2
#define DAS_ERR_HIP -3
#define DAS_ERR_STATE -4
#define DAS_ERR_INTERNAL -5

/* solver ids (reference run-time selection by "solverName", DASolver.C:122-152) */
#define DAS_SOLVER_SIMPLEFOAM 0          /* DASimpleFoam + SpalartAllmaras */
#define DAS_SOLVER_SCALARTRANSPORTFOAM 1 /* DAScalarTransportFoam */
#define DAS_SOLVER_RHOSIMPLEFOAM 2       /* DARhoSimpleFoam + SpalartAllmaras (perfect gas, hConst, const transport) */
#define DAS_SOLVER_TURBOFOAM 3          /* DATurboFoam + SpalartAllmaras: SIMPLEC-consistent / transonic pEqn, "h" energy, MRF */
#define DAS_SOLVER_HEATTRANSFERFOAM 4   /* DAHeatTransferFoam: steady conduction in a solid, one cell state T, kappa constant or a polynomial in T */
#define DAS_SOLVER_SOLIDDISPLACEMENTFOAM 5 /* DASolidDisplacementFoam: steady linear-elastic solid, one cell vector state D, uniform rho, E, nu */
/* DAPimpleFoam + SpalartAllmaras: the unsteady incompressible solver.  DASimpleFoam's states [U | p | nuTilda | phi] and stencils; the
 * residual carries fvm::ddt(U) and fvm::ddt(nuTilda) (ddt_scheme Euler or backward at the constant deltaT) and UEqn.relax(1.0).  No T
 * field, MRF or cyclic patches: das_create returns NULL with the reason */
#define DAS_SOLVER_PIMPLEFOAM 6
#define DAS_IS_COMPRESSIBLE(s) ((s) == DAS_SOLVER_RHOSIMPLEFOAM || (s) == DAS_SOLVER_TURBOFOAM)

/* patch types */
#define DAS_PATCH_PATCH 0
#define DAS_PATCH_WALL 1
#define DAS_PATCH_SYMMETRY 2
#define DAS_PATCH_CYCLIC 3 /* coupled pair (translational or rotational): face k of the patch pairs with face k of patch_neighbour */

/* boundary-condition codes per patch and field */
#define DAS_MAX_KAPPA_COEFFS 8
#define DAS_BC_FIXED_VALUE 0
#define DAS_BC_ZERO_GRADIENT 1
#define DAS_BC_INLET_OUTLET 2
#define DAS_BC_SYMMETRY 3
#define DAS_BC_CYCLIC 4 /* placeholder code of coupled patches: no patch-field coefficients are evaluated */
/* T only: OpenFOAM's mixedFvPatchField with refGrad = 0 and a refValue and a valueFraction f of its own on every face,
 * x_b = f refValue + (1 - f) x_c, snGrad = f deltaCoeff (refValue - x_c) (bc_T_mixed_ref / bc_T_mixed_frac below); what the
 * thermalCoupling input of a conjugate heat transfer loop writes (reference DAInputThermalCoupling.C) */
#define DAS_BC_MIXED 5
/* D only: the reference's tractionDisplacement patch field (DAMisc/tractionDisplacement), a fixedGradient whose gradient
 * g = ((t - p n) / rho - n . (mu gradD_b^T - (mu + lambda) gradD_b) - n tr(gradD_b) lambda) / (2 mu + lambda) is lagged: the residual
 * runs the option maxCorrectBCCalls passes from g = 0 (bc_D_traction / bc_D_pressure below) */
#define DAS_BC_TRACTION 6
/* nut patch treatment (reference DAField.C:1155-1218, DAMisc/nutUSpaldingWallFunctionDF) */
#define DAS_NUT_CALCULATED 0
#define DAS_NUT_LOWRE_WALL 1
#define DAS_NUT_SPALDING_WALL 2
#define DAS_NUT_SYMMETRY 3

typedef struct das_solver das_solver_t; /* replaces Foam::DASolvers (DASolvers.H) */
typedef struct das_mat das_mat_t;       /* replaces PETSc Mat dRdWT / dRdWTPC */
typedef struct das_ksp das_ksp_t;       /* replaces PETSc KSP */

/* What the reference reads from the OpenFOAM case directory (constant/polyMesh, 0/,
 * constant/transportProperties, system/fvSolution) for this path, as plain arrays. */
typedef struct das_case {
    int solver; /* DAS_SOLVER_* */
    int n_points, n_faces, n_internal_faces, n_cells, n_patches;
    const double* points;  /* 3*n_points */
    const int* face_ptr;   /* n_faces+1 (CSR into face_pts) */
    const int* face_pts;   /* point ids */
    const int* owner;      /* n_faces */
    const int* neighbour;  /* n_internal_faces */
    const int* patch_start; /* n_patches, absolute face index */
    const int* patch_size;
    const int* patch_type; /* DAS_PATCH_* */
    /* per-patch BC tables; *_val: 3 doubles per patch for U, 1 otherwise */
    const int* bc_U_code;
    const double* bc_U_val;
    const int* bc_p_code;
    const double* bc_p_val;
    const int* bc_nuTilda_code;
    const double* bc_nuTilda_val;
    const int* bc_nut_code;
    const int* bc_T_code;
    const double* bc_T_val;
    double nu;
    double relax_U, relax_nuTilda, relax_T;
    double DT, deltaT;        /* DAScalarTransportFoam */
    const double* y_wall;     /* n_cells, frozen wall distance (may be NULL for ScalarTransport and HeatTransfer) */
    const double* phi_frozen; /* n_faces, DAScalarTransportFoam only */
    const double* T_old;      /* n_cells, DAScalarTransportFoam only */
    /* DARhoSimpleFoam thermophysicalProperties (reference DAResidual.C:179-293): Cp [J/kg/K], molWeight [kg/kmol],
     * mu [Pa s], Pr, Prt */
    double Cp, molWeight, mu, Pr, Prt;
    /* constant/MRFProperties, one zone covering the mesh (OpenFOAM MRFZone; used by DARhoSimpleFoam and DATurboFoam,
     * reference DAResidualRhoSimpleFoam.C:123,186, DAResidualTurboFoam.C:107,130,161,200): angular velocity vector
     * [rad/s], origin, and per patch 1 = the patch rotates with the zone (not listed in nonRotatingPatches) */
    int mrf_active;
    double mrf_omega[3], mrf_origin[3];
    const int* patch_mrf_rotating; /* n_patches, may be NULL when mrf_active == 0 */
    /* DATurboFoam: system/fvSolution SIMPLE.transonic and the reference option transonicPCOption (-1/0: keep
     * div(phid,p) in the PC, 1: drop it, 2: additionally phiRes = phi) */
    int transonic, transonic_pc_option;
    /* DASimpleFoam with the optional passive T field (reference DAResidualSimpleFoam.C:50-76,215-235; states
     * [U | p | T | nuTilda | phi], DAStateInfoSimpleFoam.C:118-131); Pr / Prt above are then transportProperties' */
    int simple_has_T;
    /* cyclic (coupled) patches, OpenFOAM cyclicFvPatch semantics: per patch the index of the paired patch (-1 for
     * ordinary patches; may be NULL if no patch is cyclic) and, for rotational pairs, the tensor forwardT (row-major 3x3
     * per patch) that carries neighbour-side vectors into this side's frame (cyclicPolyPatch::forwardT; identity /
     * NULL for translational pairs; the partner patch holds the transpose) */
    const int* patch_neighbour;
    const double* patch_rotation;
    /* thermophysicalProperties transport "sutherland" (reference DAResidual::updateThermoVars, DAResidual.C:264-293):
     * mu = As sqrt(T) / (1 + Ts / T), alpha = mu Cv (1.32 + 1.77 R / Cv) / Cp; 0 = "const" transport (mu, Pr above) */
    int transport_sutherland;
    double sutherland_As, sutherland_Ts;
    /* betaFINuTilda (n_cells, may be NULL = 1): the field-inversion multiplier of the Spalart-Allmaras production term
     * (reference DASpalartAllmaras.C betaFINuTilda_), the volScalarField a `field` input assigns (DAInputField.C:88-110) */
    const double* beta_fi_nuTilda;
    /* refValue and valueFraction of the patches whose bc_T_code is DAS_BC_MIXED: one entry per boundary face of the mesh (n_faces -
     * n_internal_faces, boundary-face order; the entries of other patches are not read).  NULL with such a patch: refValue 0, fraction 0. */
    const double* bc_T_mixed_ref;
    const double* bc_T_mixed_frac;
    /* DAHeatTransferFoam, constant/solidProperties (reference DAResidualHeatTransferFoam.C:40-53,105-132): the conductivity
     * kappa(T) = sum_k kappa_coeffs[k] T^k; `kappa` is one coefficient, `kappaCoeffs` up to DAS_MAX_KAPPA_COEFFS of them */
    int n_kappa_coeffs;
    double kappa_coeffs[DAS_MAX_KAPPA_COEFFS];
    /* DASolidDisplacementFoam, constant/mechanicalProperties (reference readMechanicalPropertiesSolidDisplacement.H): uniform density
     * rho [kg/m^3], Young's modulus E [Pa] and Poisson's ratio nu; E is normalised by rho, mu = (E / rho) / (2 (1 + nu)),
     * lambda = nu (E / rho) / ((1 + nu) (1 - 2 nu)), or nu (E / rho) / ((1 + nu) (1 - nu)) with plane_stress != 0.  rho <= 0, E <= 0 and
     * nu outside (-1, 0.5) return DAS_ERR_ARG with the value in the message */
    double solid_rho, solid_E, solid_nu;
    int plane_stress;
    /* per-patch tables of the state D: code (DAS_BC_FIXED_VALUE, DAS_BC_ZERO_GRADIENT, DAS_BC_SYMMETRY or DAS_BC_TRACTION), the
     * fixedValue (3 per patch), and the traction [Pa] (3 per patch) and pressure [Pa] (1 per patch) of a tractionDisplacement patch.
     * NULL code table: zeroGradient everywhere; NULL value tables: zeros.  A cyclic patch on this solver returns DAS_ERR_ARG */
    const int* bc_D_code;
    const double* bc_D_val;
    const double* bc_D_traction;
    const double* bc_D_pressure;
    /* DAPimpleFoam, system/fvSchemes ddtSchemes.default: 0 Euler, 1 backward (deltaT above is its constant time step) */
    int ddt_scheme;
} das_case_t;

const char* das_last_error(void);
int das_version(void);
/* number of visible HIP devices (0 on a CPU-only host; never fails) */
int das_device_count(void);

/* ---- construction / options ------------------------------------------------------------
 * das_create      <- pyDASolvers.__init__(argsAll, pyOptions)   pyDASolvers.pyx:134-153
 * das_init_solver <- pyDASolvers.initSolver()                    pyDASolvers.pyx:155 (DASolver::initSolver)
 * das_set_option_* <- pyDASolvers.updateDAOption(pyOptions)      pyDASolvers.pyx:355 (flattened "a.b" keys of DAOPTION,
 *                     reference dafoam/pyDAFoam.py:39-661; lists are comma-joined strings) */
das_solver_t* das_create(const das_case_t* c);
void das_destroy(das_solver_t* s);
int das_set_option_double(das_solver_t* s, const char* key, double v);
int das_set_option_int(das_solver_t* s, const char* key, long long v);
int das_set_option_str(das_solver_t* s, const char* key, const char* v);
int das_get_option_double(das_solver_t* s, const char* key, double* v);
/* a string option into buf (cap bytes, always terminated); returns the length of the value */
int das_get_option_string(das_solver_t* s, const char* key, char* buf, int cap);
int das_init_solver(das_solver_t* s, int device);

/* ---- sizes: getNLocalAdjointStates/getNLocalCells/getNGlobalCells/getNLocalPoints  pyDASolvers.pyx:305-317 */
long long das_get_n_local_adjoint_states(das_solver_t* s);
long long das_get_n_local_cells(das_solver_t* s);
long long das_get_n_global_cells(das_solver_t* s);
int das_set_n_global_cells(das_solver_t* s, long long nGlobal); /* sharded runs: set by the partitioner */
long long das_get_n_local_points(das_solver_t* s);
long long das_get_n_local_faces(das_solver_t* s);

/* das_update_of_mesh <- updateOFMesh(vol_coords)  pyDASolvers.pyx:297-300 (PYDAFOAM.setVolCoords, pyDAFoam.py:2111-2117):
 *   new point coordinates (3 * n_points); metrics are recomputed and re-uploaded, the wall distance stays frozen.
 * das_get_of_mesh_points <- getOFMeshPoints  pyDASolvers.pyx:278 */
int das_update_of_mesh(das_solver_t* s, const double* points);
int das_get_of_mesh_points(das_solver_t* s, double* points);
/* das_calc_dvolcoord_product <- calcJacTVecProduct(inputType "volCoord" -> outputType "residual" | "function")
 *   pyDASolvers.pyx:333-366 -> DASolver.C:1690-1839 with DAInput/DAInputVolCoord.C:33-70: the FULL product vector
 *   product[3 p + k] = sum_i seeds[i] dOutput_i/dX[p][k] over all mesh points, at the current states and points.  The reference
 *   gets it from one reverse sweep of its AD tape; here coloured forward-mode passes run entirely on the device: the points of a
 *   colour carry a unit tangent, metrics and residual follow as Dual<1> (exact; option amd.volCoordMode "fd": central
 *   differences; csrc/das_volcoord.hpp).  seeds: n states (residual) or 1 (function:
 *   any defined face function).  info4 (may be NULL) = {point colours, residual passes, seconds, build seconds}.
 * das_point_influence_build / _get: the host-side structure behind it (no GPU needed): point colours, the cells whose residual
 *   rows feel a point (CSR), the finite-difference step per point.
 * das_debug_device_geometry: the metrics the device passes produce for `points` (records of 12 / 5 doubles: FaceGeom, CellGeom of
 *   csrc/das_common.hpp), solver geometry untouched - test aid. */
int das_calc_dvolcoord_product(das_solver_t* s, const char* outputName, const char* outputType, const double* seeds, double* product /*3P*/,
                               double* info4);
int das_point_influence_build(das_solver_t* s, int* nColors, long long* nEntries);
int das_point_influence_get(das_solver_t* s, int* colors /*P*/, long long* ptr /*P+1*/, int* cells /*nEntries*/, double* steps /*P*/);
int das_debug_device_geometry(das_solver_t* s, const double* points /*3P*/, double* fg12 /*12F*/, double* cg5 /*5N*/);
/* das_debug_strength_aggregates: the aggregates of the pressure coarse space under option amd.pcCoarseAggregation "strength"
 *   (repeated pairwise matching along the strongest |Sf| / |d| coupling until at most maxAgg are left); host only - test aid. */
int das_debug_strength_aggregates(das_solver_t* s, int maxAgg, int* agg /*N*/, int* nAgg);
/* ---- host-side mesh geometry (fvMesh metrics; no GPU needed) - used by tests and input generators */
int das_get_geometry(das_solver_t* s, double* Sf /*3F*/, double* Cf /*3F*/, double* C /*3N*/, double* V /*N*/,
                     double* weights /*Fi*/, double* nonOrthDeltaCoeffs /*Fi*/, double* nonOrthCorr /*3Fi*/,
                     double* bDeltaCoeffs /*Fb*/);

/* fvMesh metrics of a bare polyhedral mesh (no case, no solver handle, no GPU): Sf / Cf per face, C / V per cell, linear interpolation
 * weights per internal face (may be NULL) - the synthetic-input generators of the bench use it at 2 M cells (numpy: 30 s) */
int das_mesh_metrics(int nPoints, const double* points, int nFaces, int nInternalFaces, int nCells, const int* facePtr, const int* facePts, const int* owner,
                     const int* neighbour, double* Sf /*3F*/, double* Cf /*3F*/, double* C /*3N*/, double* V /*N*/, double* weights /*Fi*/);

/* ---- state / residual access -------------------------------------------------------------
 * das_update_of_fields <- updateOFFields(states)   pyDASolvers.pyx:268   (DAField::stateVec2OFField)
 * das_get_of_fields    <- getOFFields(states)      pyDASolvers.pyx:273
 * das_get_residuals    <- getResiduals(residuals)  pyDASolvers.pyx:184   (DASolver.C:1157-1236; isPC=0)
 * das_calc_residuals   : same with explicit isPC (DAResidual::masterFunction, DAResidual.C:100-171) */
int das_update_of_fields(das_solver_t* s, const double* states);
int das_get_of_fields(das_solver_t* s, double* states);
int das_get_residuals(das_solver_t* s, double* residuals);
int das_calc_residuals(das_solver_t* s, int isPC, double* residuals);

/* ---- connectivity + colouring ------------------------------------------------------------
 * das_run_coloring <- runColoring()  pyDASolvers.pyx:161  (DASolver.C:708-743, DAJacCon, DAColoring)
 * Host graph work; needs no GPU.  The getters expose dRdWCon and the colour vector (the reference
 * writes them as dRdWCon.bin / dRdWColoring_<np>.bin, DAJacCon.C:1886-1975,2580-2586). */
/* das_solve_primal <- solvePrimal()  pyDASolvers.pyx (DASimpleFoam::solvePrimal, DASimpleFoam.C:123-185): converge the
 * residuals of the current states.  The reference iterates SIMPLE; its fixed point is R(W) = 0, which is solved here by a
 * pseudo-transient Newton-Krylov method built from the adjoint's own kernels (forward-mode operator, transposed node-block
 * ILU + coarse space; options amd.primalTau0 / primalLinearTol / primalLinearIters / primalPCLag; pseudo-time control
 * amd.primalTauMode "ser" | "ramp" (+ primalTauGrowth / GrowthMax / Max / Min, primalAcceptFactor, primalDampedSteps) and
 * amd.primalPseudoTimeFields "all" | "momentum" (cold starts: the term on the transport rows only)).  Returns 0 converged
 * (|R| <= max(relTol |R0|, absTol)) / 1 not converged; info4 = {Newton steps, GMRES iterations, |R0|, |R|}. */
int das_solve_primal(das_solver_t* s, int maxSteps, double relTol, double absTol, double* info4, double* hist, int histCap);
/* das_simple_iteration: nSweeps iterations of the reference's OWN primal loop - SIMPLE (DASimpleFoam::solvePrimal, DASimpleFoam.C:123-185:
 * UEqnSimple.H, pEqnSimple.H with nNonOrthogonalCorrectors 1, DASpalartAllmaras::correct) - on the device, from the current states:
 * relaxed momentum predictor, rAU / HbyA / constrainHbyA, pressure equation, phi = phiHbyA - flux, explicit p relaxation (alphaP =
 * fvSolution relaxationFactors.fields.p), U correction, SA transport + bound.  Inner solves: Jacobi-preconditioned BiCGStab (U, nuTilda) /
 * CG (p) to the relative tolerance linTol, at most maxLinIters iterations.  DASimpleFoam + SA without T field, MRF and cyclic pairs, one
 * rank.  info3 (optional) = inner iterations of the last sweep (U, p, nuTilda).  The Newton-Krylov das_solve_primal reaches the same
 * fixed point in far fewer steps; the sweeps reproduce the reference's iteration (and the oracle's, oracle/primal.py) sweep by sweep. */
int das_simple_iteration(das_solver_t* s, int nSweeps, double alphaP, double linTol, int maxLinIters, double* info3);
int das_run_coloring(das_solver_t* s);
/* das_set_coloring <- DAJacCon::readJacConColoring (DAJacCon.C:1980-2019): colours read back from a dRdWColoring_n.bin
 *                      cache; validated against the freshly built connectivity ("Conflicting Colors Found!" otherwise). */
int das_set_coloring(das_solver_t* s, const int* colors);
/* host-only profiling aid (no GPU needed): factorises one block-local CSR (sorted columns) exactly like a preconditioner
 * block - symbolic ILU(lfill), numeric, level schedules, entry streams - and returns the four phase times [s] */
int das_debug_factor_block(int nl, const long long* rowptr, const int* col, const double* val, int lfill, double* tim4, long long* nnzLU,
                           int* nLevelsL, int* nLevelsU);
/* host-only test aid (no GPU, no solver handle): the recursive coordinate bisection that cuts the "ras" blocks, the sub-domains,
 * the "rcb" aggregates and the colouring tiles, on n points centres[3 * i + axis].  mode 0: param parts of almost equal size,
 * out[i] = part of point i; mode 1: halving until a leaf holds at most param points, out[i] = leaf of point i */
int das_debug_rcb(int n, const double* centres, int mode, int param, int* out);
int das_get_n_colors(das_solver_t* s, int isPC);
long long das_get_con_nnz(das_solver_t* s, int isPC);
int das_get_con(das_solver_t* s, int isPC, long long* rowptr /*n+1*/, int* colidx /*nnz*/);
int das_get_colors(das_solver_t* s, int isPC, int* colors /*n*/);

/* ---- Jacobians ---------------------------------------------------------------------------
 * das_calc_drdwt <- calcdRdWT(isPC, Mat dRdWT)  pyDASolvers.pyx:237 (DASolver.C:948-1089, DAPartDeriv.C:350-473).
 *   mode: 0 = coloured one-sided finite differences (reference behaviour, step adjPartDerivFDStep.State),
 *         1 = coloured dual-number (forward-mode AD) perturbations - exact derivatives on the same colouring.
 *   Result: transposed CSR on the device, entry (j,i) = s_j dR_i/dW_j. */
int das_calc_drdwt(das_solver_t* s, int isPC, int mode, das_mat_t** out);
long long das_mat_rows(das_mat_t* m);
long long das_mat_nnz(das_mat_t* m);
int das_mat_export(das_mat_t* m, long long* rowptr, int* colidx, double* vals);
/* y = A x on host buffers (testing) */
int das_mat_mult(das_mat_t* m, const double* x, double* y);
/* device CSR handle from host arrays (reference: PETSc.Mat().load of dRdWTPC.bin under adjEqnOption.readPCMat,
 * dafoam/mphys/mphys_dafoam.py:469-471) */
int das_mat_create_from_csr(long long n, const long long* rowptr, const int* colidx, const double* vals, das_mat_t** out);
void das_mat_destroy(das_mat_t* m);

/* das_initialize_drdwt_matrix_free <- initializedRdWTMatrixFree()  pyDASolvers.pyx:253 (DASolver.C:1321-1351):
 *   the reference creates a PETSc MatShell whose MULT replays a CoDiPack reverse tape; here the operator is
 *   assembled once per call with dual numbers (mode 1, isPC=0 schemes) and applied as a device SpMV.
 * das_destroy_drdwt_matrix_free    <- destroydRdWTMatrixFree()      pyDASolvers.pyx:256 */
int das_initialize_drdwt_matrix_free(das_solver_t* s);
int das_destroy_drdwt_matrix_free(das_solver_t* s);
/* nnz of the assembled matrix-free operator (after the jacLowerBounds filter), -1 if not initialised */
long long das_op_nnz(das_solver_t* s);
/* bytes of matrix data one dRdW^T.psi product streams in the operator's storage format: vector-state rows packed as group
 * rows (one int32 column list + three fp64 value planes per 16 entries, csrc/das_opmat.hpp), scalar rows as CSR (12 B/entry) */
long long das_op_format_bytes(das_solver_t* s);
/* the operator of initializedRdWTMatrixFree as CSR arrays on the host (rowptr[n+1], colidx[das_op_nnz], vals[das_op_nnz]) */
int das_op_export(das_solver_t* s, long long* rowptr, int* colidx, double* vals);

/* ---- unsteady adjoint terms (DAScalarTransportFoam, BASELINE configs[0]) ---------------------------------------------
 * das_calc_drdwold_t_psi <- calcdRdWOldTPsiAD(oldTimeLevel, psi, dRdWOldTPsi)  pyDASolvers.pyx:240 (DASolver.C:1910-1969):
 *     D_s (dR/dW_old)^T psi for oldTimeLevel 1 (W0) or 2 (W00).  Euler ddt: dR/dT0 = -1/deltaT (per-volume residual),
 *     level 2 and steady solvers give zero.
 * das_set_old_time_fields: frozen flux and old-time temperature of the current time step (the reference re-reads them
 *     from disk, readStateVars DASolver.C:3193).
 * DAPimpleFoam: das_set_old_time_states puts the full state vectors of the two old time levels (n states each, "state" ordering) on
 *     the device and sets the time index the residual is evaluated at; W00 may be NULL where the scheme is Euler or timeIndex < 2 (it
 *     is not read there).  Every residual, Jacobian and product evaluated afterwards is R(W; W0, W00).  das_calc_drdwold_t_psi then
 *     gives D_s (dR/dW0)^T psi (level 1) and D_s (dR/dW00)^T psi (level 2; exact zeros for Euler and below time index 2) from one
 *     hand-written gather kernel: the diagonal of the U and nuTilda rows plus rAU c0 / deltaT times the transpose of the map
 *     HbyA -> (pRes, phiRes); bitwise the same on every call. */
int das_set_old_time_states(das_solver_t* s, const double* W0, const double* W00 /* or NULL */, int timeIndex);
/* das_set_time_index <- setTime(time, timeIndex) for DAPimpleFoam: the time index alone (it selects the ddt coefficients: backward
 *     below 2 is Euler); the old-time states on the device stay.  A residual that then needs W00 and has none returns DAS_ERR_STATE. */
int das_set_time_index(das_solver_t* s, int timeIndex);
int das_calc_drdwold_t_psi(das_solver_t* s, int oldTimeLevel, const double* psi, double* out);
int das_set_old_time_fields(das_solver_t* s, const double* phi_frozen /* n_faces or NULL */, const double* T_old /* n_cells or NULL */);

/* ---- objective functions (adjoint right-hand side producers) -----------------------------------------------
 * das_define_force_function <- the "function" option entry {type: force, patches, directionMode: fixedDirection,
 *     direction, scale} consumed by DAFunctionForce (reference src/adjoint/DAFunction/DAFunctionForce.C:20-77)
 * das_calc_function         <- calcFunction(functionName)  pyDASolvers.pyx (DAFunctionForce::calcFunction :79-158) */
/* das_calc_jac_vec_product <- the forward-mode (ADF build) directional derivative of the residuals, DASolver.C:1364-1441
 *                             run forward: product_i = sum_j dR_i/dW_j s_j v_j at the current states.  One dual-number
 *                             residual pass; no colouring and no matrix are involved. */
int das_calc_jac_vec_product(das_solver_t* s, const double* v, double* product);
/* Boundary-value design inputs.
 * das_set_patch_value   <- DAInputPatchVelocity::run / DAInputPatchVar::run (src/adjoint/DAInput/DAInputPatchVelocity.C:33-135):
 *                          assigns the (ref)value of fixedValue / inletOutlet patches; any other patch type is an error.
 *                          field: "U" (value[3]) | "p" | "nuTilda" | "T" (value[1]).
 * das_calc_dbc_product  <- calcJacTVecProduct(inputType = patchVelocity | patchVar) pyDASolvers.pyx:208-235:
 *                          product[0] = seeds^T (dOutput/d(patch value) . tangent), outputType "residual" (seeds: n,
 *                          host) or "function" (seeds: 1).  One forward-mode (dual number) pass. */
int das_set_patch_value(das_solver_t* s, const int* patch_ids, int npatch, const char* field, const double* value);
int das_get_patch_value(das_solver_t* s, int patch_id, const char* field, double* value);
/* `field` inputs (reference DAInputField.C: a design variable that IS a volScalarField; inputInfo type "field"):
 * fieldName "betaFINuTilda" (values[nCells]).  das_calc_dfield_product: product[c] = sum_i seeds[i] dR_i/dfield_c (outputType
 * "residual"; ONE forward-mode residual pass with a unit tangent on every cell - a residual row depends on the field value of
 * its own cell only) or 0 for the patch-integral functions (outputType "function"), i.e. calcJacTVecProduct(field -> ...)
 * of DASolver.C:1690-1839. */
int das_set_field(das_solver_t* s, const char* fieldName, const double* values);
int das_get_field(das_solver_t* s, const char* fieldName, double* values);
int das_calc_dfield_product(das_solver_t* s, const char* fieldName, const char* outputName, const char* outputType, const double* seeds,
                            double* product);
int das_calc_dbc_product(das_solver_t* s, const int* patch_ids, int npatch, const char* field, const double* tangent, const char* outputName,
                         const char* outputType, const double* seeds, double* product);
int das_define_force_function(das_solver_t* s, const char* name, const int* patch_ids, int npatch, const double* direction, double scale);
/* das_define_face_function <- the other patch-integral entries of the "function" option dict (pyDAFoam.py:100-200):
 *   type "force"                 vecA = direction (unit)                                   DAFunctionForce.C:79-158
 *        "moment"                vecA = axis (unit), vecB = center                         DAFunctionMoment.C:73-120
 *        "massFlowRate"          sum rho_b (U_b . S_f) * scale                             DAFunctionMassFlowRate.C:52-80
 *        "totalPressure"         area average of p_b + 0.5 rho_b |U_b|^2, * scale          DAFunctionTotalPressure.C:60-90
 *        "totalTemperatureRatio" TT_out / TT_in (area averages); patch_group[k] = 0 inlet, 1 outlet; gammaFn = the
 *                                thermophysicalProperties gamma, R = Cp - Cp/gamma         DAFunctionTotalTemperatureRatio.C:60-130
 * patch_group may be NULL for the non-ratio types.  Values and derivatives go through das_calc_function /
 * das_calc_jac_t_vec_product / das_calc_dbc_product like the force. */
int das_define_face_function(das_solver_t* s, const char* name, const char* type, const int* patch_ids, const int* patch_group, int npatch,
                             const double* vecA, const double* vecB, double scale, double gammaFn);
/* das_define_face_function_ex <- the same entries, plus the types that carry more options:
 *   type "totalPressureRatio"   TP_out / TP_in (area averages), TP = p_b (1 + 0.5 (gamma-1) Ma^2)^(gamma/(gamma-1)); groups, gammaFn and R
 *                               as for totalTemperatureRatio; no scale is applied            DAFunctionTotalPressureRatio.C:50-139
 *        "wallHeatFlux"         sum scale w_f q_f, q_f = alphaEff_b snGrad(he)_f (compressible) or Cp alphaEff_b snGrad(T)_f (DASimpleFoam
 *                               with the T field); w_f = |Sf| / sum |Sf| (flags & 1: byUnitArea) or |Sf|; snGrad from the patch field
 *                               (wallDistanceMethod default) or (x_b - x_c) / |C_f - C_c| (flags & 2: daCustom).  Solvers without a T
 *                               field return DAS_ERR_ARG                                    DAFunctionWallHeatFlux.C:115-304
 *                               DAHeatTransferFoam: q_f = kappa(T_b) snGrad(T)_f, same weights and flags (:229-261) - the only face
 *                               function of that solver, every other type returns DAS_ERR_ARG naming the type
 * flags & 8: calcRefVar, F <- (F - ref)^2, for these two types.  das_define_face_function(...) is
 * das_define_face_function_ex(..., flags = 1, ref = 0). */
int das_define_face_function_ex(das_solver_t* s, const char* name, const char* type, const int* patch_ids, const int* patch_group, int npatch,
                                const double* vecA, const double* vecB, double scale, double gammaFn, int flags, double ref);
/* das_define_location_function <- {type: location, mode, coeffKS, axis, center} (DAFunctionLocation.C:153-295) over the faces of the patches:
 *   r_f = |c - (c o axis)|, c = C_f - center, "o" the COMPONENT-WISE product as the reference writes it (not the projection onto the axis);
 *   mode "maxRadiusKS"         log(sum exp(coeffKS r_f)) / coeffKS
 *        "maxInverseRadiusKS"  log(sum exp(coeffKS / (r_f + 1e-12))) / coeffKS
 *        "maxRadius"           r of the face that has the largest radius at definition (first on ties; kept after das_update_of_mesh)
 * The KS sums are evaluated in log space, deterministically, over any number of faces; beyond the reference's guard (sum > 1e200)
 * das_calc_function returns DAS_ERR_ARG "KS function summation term too large! Reduce coeffKS!".  axis is normalised here.
 * flags & 8: calcRefVar.  State, boundary-value and field derivatives are exactly zero; das_calc_dvolcoord_product carries the
 * softmax weights through the dual-point metrics. */
int das_define_location_function(das_solver_t* s, const char* name, const char* mode, const int* patch_ids, int npatch, const double* axis,
                                 const double* center, double coeffKS, int flags, double ref);
/* das_define_mesh_quality_function <- {type: meshQualityKS, coeffKS, metric} (DAFunctionMeshQualityKS.C): log(sum exp(coeffKS a_f)) / coeffKS
 * over ALL faces of the mesh, internal and boundary; metric "faceOrthogonality" | "nonOrthoAngle" | "faceSkewness" (restated from OpenFOAM's
 * polyMeshTools, csrc/das_meshquality.hpp).  Log-space sum, deterministic, no 1e200 abort; no scale is applied.  flags & 8: calcRefVar.
 * Undecomposed DASimpleFoam, DARhoSimpleFoam, DATurboFoam and DAScalarTransportFoam; a mesh with cyclic patches is refused.  State,
 * boundary-value and field derivatives are exactly zero; das_calc_dvolcoord_product (amd.volCoordMode dual) carries the softmax weights
 * through the dual points and metrics. */
int das_define_mesh_quality_function(das_solver_t* s, const char* name, const char* metric, double coeffKS, int flags, double ref);
/* das_define_residual_norm_function <- {type: residualNorm, resWeight, resMode} (DAFunctionResidualNorm.C) on the residual das_calc_residuals
 * returns (isPC 0): resMode "L2Norm" sqrt(sum w_i^2 R_i^2) | "L1Norm" sum |w_i R_i|, where the internal faces of phiRes add w^2 R^2 in either
 * mode as in the reference.  resNames[k] = "<state>Res" carries weights[k]; every residual of the solver must be named, other names are
 * ignored.  flags & 8: calcRefVar.  No scale.  Every product entry treats such a function as the residual output seeded with dF/dR. */
int das_define_residual_norm_function(das_solver_t* s, const char* name, const char* const* resNames, const double* weights, int nw,
                                      const char* resMode, int flags, double ref);
/* das_define_patch_field_function <- the boundary-value entries of the "function" option dict (flow solvers):
 *   type "patchMean"  area average of component comps[0] of the boundary value of var, * scale   DAFunctionPatchMean.C:36-110
 *        "variance"   mode surface: sum w_f scale (b_f,i - d_f,i)^2 / W over the faces and the components comps[ncomp],
 *                     w_f = |Sf| (flags & 16: useGeoWeight) or 1, W = sum of w_f per component or the number of points
 *                                                                                             DAFunctionVariance.C
 * var: "U" (comps in 0..2), "p", "nuTilda", "T" (comps = {0}); the boundary value follows each patch's condition like the
 * residual's.  data[nfaces * ncomp] (variance: the reference values face-major over the patches in the given order; NULL = no
 * reference data: F = 0 with zero derivatives).  flags & 8: calcRefVar, F <- (F - ref)^2 (patchMean).  Values and derivatives
 * go through das_calc_function / das_calc_jac_t_vec_product / das_calc_dbc_product / das_calc_dvolcoord_product (patchMean) like
 * the face functions above; variance rejects the volCoord product.  Sharded solvers (owned-cell mask) return DAS_ERR_ARG. */
int das_define_patch_field_function(das_solver_t* s, const char* name, const char* type, const int* patch_ids, int npatch, const char* var,
                                    const int* comps, int ncomp, const double* data, int flags, double scale, double ref);
/* das_define_cell_function <- the cell-set entries of the "function" option dict (every solver):
 *   type "variableVolSum"  scale sum_c (V_c | 1) q_c^(1|2) / T over cells[ncells]; flags & 1 isSquare, & 2 multiplyVol,
 *                          & 4 divByTotalVol (T = 1 + the volume of ALL cells, else T = 1), & 8 calcRefVar (F <- (F - ref)^2)
 *                                                                                             DAFunctionVariableVolSum.C:43-135
 *        "variance"        mode field: sum w_t scale (q_t - d_t)^2 / W over (cell, component) terms, w = V_c (flags & 16:
 *                          useGeoWeight) or 1, W = sum of w or the number of terms            DAFunctionVariance.C
 * The cell set (allCells / boxToCell, chosen by the caller) is fixed here; the volumes follow das_update_of_mesh.
 * var: a cell state of the solver ("U", "p", "nuTilda", "T") or "betaFINuTilda" (variableVolSum on the SA solvers).
 * data[ncells * ncomp] (variance, cell-major; NULL = no reference data: F = 0).  The value is a two-stage deterministic reduction
 * (bitwise repeatable); dF/dW is one elementwise pass (no colouring); das_calc_dfield_product gives dF/dbeta for
 * var = betaFINuTilda (0 otherwise); das_calc_dbc_product gives 0; das_calc_dvolcoord_product differentiates the volumes
 * (variableVolSum; variance rejects it).  Sharded solvers (owned-cell mask) return DAS_ERR_ARG. */
int das_define_cell_function(das_solver_t* s, const char* name, const char* type, const int* cells, int ncells, const char* var, const int* comps,
                             int ncomp, const double* data, int flags, double scale, double ref);
/* das_define_von_mises_function <- the "function" entries of type vonMisesStressKS (DASolidDisplacementFoam only; DAFunctionVonMisesStressKS.C):
 *   F = log(sum_c exp(coeffKS vm_c)) / coeffKS over cells[ncells], vm_c = scale sqrt(1.5 |dev sigma|^2), sigma = rho (mu twoSymm(gradD) +
 *   lambda tr(gradD) I) with the cell gradD of the residual pass, traction passes included.  The sum runs max-shifted in log space (two
 *   deterministic stages); the reference's abort above 1e200 is not reproduced - wider than the reference.  flags & 8: calcRefVar.
 *   Derivatives: stateVar (reaches the face neighbours through gradD) and volCoord; patchVar, patchVelocity and field inputs give zeros.
 *   das_define_cell_function with var "solid:rho" (variableVolSum, DASolidDisplacementFoam only) sums the uniform density: the mass, whose
 *   state derivative is exactly zero. */
int das_define_von_mises_function(das_solver_t* s, const char* name, const int* cells, int ncells, double scale, double coeffKS, int flags, double ref);
int das_calc_function(das_solver_t* s, const char* name, double* value);
/* das_define_force_coupling <- the "outputInfo" option entry {type: forceCouplingOutput, patches, pRef} consumed by DAOutputForceCoupling
 *   (reference src/adjoint/DAOutput/DAOutputForceCoupling.C): the force S_f (p_b - pRef) + S_f . devRhoReff_b of every face of the patches,
 *   handed in equal shares to the points of the face.  The output lists the points patch by patch in the order of patch_ids (the reference
 *   sorts the patches by name, :41 - the caller does), inside a patch in ascending mesh-point index, as [fx0, fy0, fz0, fx1, ...]; a point
 *   that two of the patches share appears once per patch and each copy receives its own patch's faces only.  The size is
 *   das_get_output_size(name, "forceCouplingOutput") = 3 x points; it depends on the connectivity only (das_update_of_mesh keeps it).
 * das_calc_force_coupling   <- calcOutput(name, "forceCouplingOutput", output): n = that size.  No atomics: the same bits on every call.
 * Derivatives: outputType "forceCouplingOutput" with `size` seeds in das_calc_jac_t_vec_product (stateVar, state-scaled like a function),
 * das_calc_dbc_product, das_calc_dfield_product (zero: the forces do not read the field) and das_calc_dvolcoord_product
 * (amd.volCoordMode dual only).  DAScalarTransportFoam (no p) and sharded solvers (owned-cell mask) return DAS_ERR_ARG. */
int das_define_force_coupling(das_solver_t* s, const char* name, const int* patch_ids, int npatch, double pRef);
int das_calc_force_coupling(das_solver_t* s, const char* name, double* out, int n);
/* das_define_thermal_coupling <- the "outputInfo" option entry {type: thermalCouplingOutput, patches} consumed by DAOutputThermalCoupling
 *   (reference src/adjoint/DAOutput/DAOutputThermalCoupling.C, discipline aero): with nF the faces of the patches, taken in the order of
 *   patch_ids (the reference sorts the patches by name, :40 - the caller does) and in face order inside a patch, entries [0, nF) hold T of
 *   the owner cell of the face and entries [nF, 2 nF) hold kappa / d = Cp alphaEff_b deltaCoeff, alphaEff_b as in wallHeatFlux.  flags & 2:
 *   wallDistanceMethod daCustom (deltaCoeff = 1 / |C_f - C_c|) instead of the face's delta coefficient.  The size is
 *   das_get_output_size(name, "thermalCouplingOutput") = 2 nF.
 * das_calc_thermal_coupling   <- calcOutput(name, "thermalCouplingOutput", output): n = that size.  No atomics: the same bits on every call.
 *   DAHeatTransferFoam (discipline thermal, :212-241): kappa / d = kappa(T_b) deltaCoeff, everything else as above; the caller checks
 *   the discipline option (pyDASolvers: a coupling on DAHeatTransferFoam needs "thermal", one on a flow solver "aero").
 * Derivatives: outputType "thermalCouplingOutput", as for forceCouplingOutput above.  Solvers without a T field (DAScalarTransportFoam,
 * DASimpleFoam without T) and sharded solvers return DAS_ERR_ARG. */
int das_define_thermal_coupling(das_solver_t* s, const char* name, const int* patch_ids, int npatch, int flags);
int das_calc_thermal_coupling(das_solver_t* s, const char* name, double* out, int n);
/* das_define_thermal_coupling_input <- the "inputInfo" option entry {type: thermalCoupling, patches} consumed by DAInputThermalCoupling
 *   (reference src/adjoint/DAInput/DAInputThermalCoupling.C): the faces as for the output; every patch must carry a mixed T
 *   (DAS_BC_MIXED), where the reference's refCast aborts.  The size is 2 nF.
 * das_set_thermal_coupling_input    <- setSolverInput(name, "thermalCoupling", ...): in[k] becomes the refValue of face k and in[nF + k], the
 *   neighbour's kappa / d (nk), its valueFraction nk / (myK + nk), with myK this side's kappa / d (the second half of the output) at the
 *   current states, geometry and boundary values.  The fraction then stays as it is - a constant of the residual, of the Jacobians and of
 *   the volCoord products - until the input is set again.  (DAHeatTransferFoam with a kappa that varies with T: myK reads T_b, which the
 *   records of the moment give, so setting the same input twice does not give the same fraction twice.)
 * das_get_patch_mixed                   the refValue and valueFraction of the faces of one mixed patch, as they stand.
 * das_calc_dthermal_coupling_product <- calcJacTVecProduct(name, "thermalCoupling", inputs, outputName, outputType, seeds, product) after
 *   the input has been set: product = [d output / d input]^T seeds (n = 2 nF), outputType "residual" (seeds: one per state), "function"
 *   (one seed), "thermalCouplingOutput" (one per entry).  d valueFraction / d nk = myK / (myK + nk)^2 is part of
 *   it.  Forward-mode passes and a per-face gather over the transposed structure of dRdW: no atomics, the same bits on every call. */
int das_define_thermal_coupling_input(das_solver_t* s, const char* name, const int* patch_ids, int npatch, int flags);
int das_set_thermal_coupling_input(das_solver_t* s, const char* name, const double* in, int n);
int das_get_patch_mixed(das_solver_t* s, int patch, double* refValue, double* valueFraction);
int das_calc_dthermal_coupling_product(das_solver_t* s, const char* inputName, const char* outputName, const char* outputType, const double* seeds,
                                       double* product, int n);

/* Heat sources of DAHeatTransferFoam: the fvSource option, entries of type heatSource (reference DAFvSourceHeatSource.C:30-321), and the
 * fvSourcePar input (DAInputFvSourcePar.C:38-140).  TRes = laplacian(kappa, T) + fvSource (DAResidualHeatTransferFoam.C:90-102), fvSource
 * [W/m^3] the sum of the sources in the order of their names.  The field depends on the metrics and the parameters only: it is computed when
 * a source is defined, when parameters are set and by das_update_of_mesh, never per residual evaluation.  Two-stage sums in a fixed order,
 * no atomics: the same bits on every call.
 * das_define_heat_source      kind "cylinderToCell": pars = p1(3), p2(3), radius, power (8 values); the cells with 0 < d.a < a.a and
 *   |d|^2 - (d.a)^2 / a.a < radius^2 (a = p2 - p1, d = C - p1) are chosen now and kept, q = power / (their volume, at the current metrics);
 *   an empty set is an error.  kind "cylinderSmooth": pars = the nine heatSourcePars center(3), axis(3), radius, length, power, and eps;
 *   q = power s / sum s V with s of :258-293 (the axial part is the component-wise product of C - center and the unit axis).
 *   snapCenter2Cell: the one cell that contains center is found now (none or several: an error) and center is C of that cell from then on.
 * das_set_heat_source_pars    heatSourcePars[indices[k]] = values[k] of a cylinderSmooth source, then the field again (updateFvSource).
 * das_get_heat_source_info    the parameters (cylinderToCell: p1, p2, radius, |p2 - p1|, power), the total volume of the source, the
 *   total sum fvSource V of the whole field [W] and the snapped cell (-1: none); any output may be NULL.
 * das_get_heat_source_cells   the cell set of a cylinderToCell source (at most cap entries are written); returns its size.
 * das_get_fv_source           the field, one value per cell (zeros while no source is defined).
 * das_calc_dfvsourcepar_product <- calcJacTVecProduct(name, "fvSourcePar", ...): product[k] = seeds . d output / d heatSourcePars[indices[k]].
 *   outputType "residual": one forward pass per index with dual-number parameters (s and the total volume are dual; the residual body is
 *   not run, d TRes / d p = d fvSource / d p); "function" and the coupling outputs: exact zeros, nothing of them reads the source.  The
 *   centre of a snapped source is not read: exact zeros for indices 0-2.
 * Every other solver and a sharded solver return DAS_ERR_ARG with a message that names fvSource; so do an unknown source name, an index
 * outside 0-8 and parameters asked of a cylinderToCell source. */
int das_define_heat_source(das_solver_t* s, const char* name, const char* kind, const double* pars, double eps, int snapCenter2Cell);
int das_set_heat_source_pars(das_solver_t* s, const char* name, const int* indices, int n, const double* values);
int das_get_heat_source_info(das_solver_t* s, const char* name, double* pars9, double* volumeTotal, double* sourceTotal, int* snappedCell);
int das_get_heat_source_cells(das_solver_t* s, const char* name, int* cells, int cap);
int das_get_fv_source(das_solver_t* s, double* out);
int das_calc_dfvsourcepar_product(das_solver_t* s, const char* name, const int* indices, int n, const char* outputName, const char* outputType,
                                  const double* seeds, double* product);

/* Actuator disks of DASimpleFoam: the fvSource option, entries of type actuatorDisk (reference DAFvSourceActuatorDisk.C:36-500), and the
 * fvSourcePar input for them.  UEqn = div(phi, U) + ... - fvSource (DAResidualSimpleFoam.C:141-147): the source is part of the matrix
 * source, so it reaches URes and, through H, HbyA, phiHbyA, pRes and phiRes; dR/dW changes with it.  fvSource [force per unit volume] is
 * the sum of the disks in the order of their names.  Like the heat sources the field depends on the metrics and the parameters only: it is
 * computed when a disk is defined, when parameters are set and by das_update_of_mesh, never per residual evaluation; two-stage sums in a
 * fixed order, no atomics.
 * das_define_actuator_disk     kind "cylinderAnnulusToCell": pars = p1(3), p2(3), innerRadius, outerRadius, scale, POD (10 values); the cells
 *   with 0 < d.a < a.a and innerRadius^2 < |d|^2 - (d.a)^2 / a.a < outerRadius^2 (a = p2 - p1, d = C - p1) are chosen now and kept; an
 *   empty set is an error.  kind "cylinderAnnulusSmooth": pars = the 13 actuatorDiskPars center(3), direction(3), innerRadius, outerRadius,
 *   scale, POD, expM, expN, targetThrust, and eps; adjustThrust: scale = targetThrust / sum fAxial(scale = 1) V, pars[8] is not read.
 *   rotDir "left" or "right".  The axial part of C - center is the component-wise product with the unit direction, as in the reference.
 *   A cell centre on the axis of a disk (the reference divides by zero there) is an error, here and whenever the field is recomputed.
 * das_set_actuator_disk_pars   actuatorDiskPars[indices[k]] = values[k] of a cylinderAnnulusSmooth disk, then the field again.
 * das_get_actuator_disk_info   the 13 parameters (cylinderAnnulusToCell: center = (p1 + p2) / 2, direction = p2 - p1), info4 = {effective
 *   scale, thrustSourceSum = sum fAxial V, torqueSourceSum = sum fCirc V, the thrust at scale 1 (adjustThrust)}, and the size of the cell
 *   set (a smooth disk: all cells); any output may be NULL.
 * das_get_actuator_disk_cells  the cell set of a cylinderAnnulusToCell disk (at most cap entries are written); returns its size.
 * das_get_fv_source_vector     the field, three components per cell (zeros while no disk is defined).
 * das_calc_dactuatordiskpar_product <- calcJacTVecProduct(name, "fvSourcePar", ...): product[k] = seeds . d output / d actuatorDiskPars[
 *   indices[k]].  outputType "residual": one forward pass per index - the parameters, the field and the adjustThrust total in dual
 *   numbers, then the whole residual once with that tangent on the source and none elsewhere (the factor rAU of H depends on the states:
 *   the U, p and phi rows all carry it); "function" and the coupling outputs: exact zeros.  Index 8 with adjustThrust and index 12
 *   without are not read: exact zeros.
 * das_simple_iteration refuses while a disk is defined (the SIMPLE sweep has no source term); das_solve_primal runs with disks.
 * Every other solver and a sharded solver return DAS_ERR_ARG with a message that names fvSource; so do an unknown disk name, an index
 * outside 0-12 and parameters asked of a cylinderAnnulusToCell disk. */
int das_define_actuator_disk(das_solver_t* s, const char* name, const char* kind, const double* pars, const char* rotDir, double eps, int adjustThrust);
int das_set_actuator_disk_pars(das_solver_t* s, const char* name, const int* indices, int n, const double* values);
int das_get_actuator_disk_info(das_solver_t* s, const char* name, double* pars13, double* info4, int* nCells);
int das_get_actuator_disk_cells(das_solver_t* s, const char* name, int* cells, int cap);
int das_get_fv_source_vector(das_solver_t* s, double* out);
int das_calc_dactuatordiskpar_product(das_solver_t* s, const char* name, const int* indices, int n, const char* outputName, const char* outputType,
                                      const double* seeds, double* product);

/* Regression models of DASimpleFoam: the regressionModel option and the regressionPar input (reference DARegression.C:164-773,
 * DAInputRegressionPar.C).  A neural network or a sum of radial basis functions is evaluated in every cell from local flow features and
 * writes betaFINuTilda as part of every residual evaluation (kernels: csrc/das_regression.hpp): the residual, dRdW^T (assembled, coloured),
 * every product and the Newton primal see it.  The models run in the order of their definition; the last one wins.
 * das_define_regression_model    one entry of the option.  model_type "neuralNetwork" | "radialBasisFunction"; input_names out of VoS, PoD,
 *   chiSA, pGradStream, PSoSS, SCurv, UOrth, each followed by (f + input_shift) * input_scale; output_name "betaFINuTilda";
 *   activation_function "sigmoid" | "tanh" | "relu" (with leaky_coeff).  Caps, refused by name: DAS_REG_MAX_INPUTS 8, DAS_REG_MAX_LAYERS 6
 *   hidden layers, DAS_REG_MAX_WIDTH 32 neurons per layer, DAS_REG_MAX_RBFS 64, DAS_REG_MAX_PARAMS 4096, DAS_REG_MAX_MODELS 4, and DAS_REG_MAX_LDS 160 KB per workgroup of either kernel
 *   (backward: inputs + 2 x hidden neurons + 1 rows of 512 bytes).
 *   Refused by name as well: externalTensorFlow, the features KoU2, ReWall, TauoK, CoP and every *_dt, another output_name, another
 *   solver, a sharded solver, a `field` input or a variableVolSum objective on betaFINuTilda and das_simple_iteration while a model is
 *   defined.  The parameters start at zero, as in the reference.  A model of the same name is replaced.
 *   pGradStream or PSoSS among the inputs of any model: nuTildaRes lists p at levels 0 and 1 and the colouring is done again.
 * das_get_regression_n_parameters  the parameter count (DARegression::nParameters), or a negative error code.
 * das_set/get_regression_parameters  the parameter vector in the reference's order (n must be the count); setting bumps the operator epoch.
 * das_get_regression_model_info  nParameters, nInputs, modelType (0 network, 1 RBF); any output may be NULL.
 * das_get_regression_features    at the current states: the features (nCells x nInputs, shifted and scaled), the model's output after the
 *   bounds (nCells) and fail3 = the number of cells that were NaN, Inf and out of bounds (the reference's fail flag is "any of them
 *   non-zero"); any output may be NULL.
 * das_calc_dregressionpar_product <- calcJacTVecProduct(name, "regressionPar", ...): product[k] = seeds . d output / d parameter k.
 *   "residual": one dual-number residual pass with a unit tangent on betaFINuTilda of every cell that kept its value (g_c = seeds . dR /
 *   d beta_c), then the hand-written reverse pass through the model, reduced over cells x parameters in a fixed order (no atomics, the
 *   same bits on every call).  "function" and the coupling outputs: exact zeros.  A model whose output a later model overwrites: zeros.
 * das_debug_reg_forward / _backward  TEST ONLY: k_reg_forward / k_reg_backward on caller-supplied features (nCells x n_inputs) with no
 *   mesh; forward gives beta (after the bounds) and the mask per cell (bit 0 NaN, 1 Inf, 2 bounded); backward gives
 *   out[k] = sum_c g[c] d beta_c / d parameter k without the bounds (the caller zeroes g on the cells it wants masked). */
typedef struct das_reg_spec {
    const char* model_type;
    int n_inputs;
    const char* const* input_names; /* may be NULL in the debug entries */
    const double* input_shift;
    const double* input_scale;
    const char* output_name;
    int n_hidden_layers;
    const int* hidden_layer_neurons;
    const char* activation_function;
    double leaky_coeff;
    int n_rbfs;
    double output_shift, output_scale, output_upper_bound, output_lower_bound, default_output_value;
} das_reg_spec_t;
int das_define_regression_model(das_solver_t* s, const char* name, const das_reg_spec_t* spec);
int das_get_regression_n_parameters(das_solver_t* s, const char* name);
int das_set_regression_parameters(das_solver_t* s, const char* name, const double* values, int n);
int das_get_regression_parameters(das_solver_t* s, const char* name, double* values, int n);
int das_get_regression_model_info(das_solver_t* s, const char* name, int* nParameters, int* nInputs, int* modelType);
int das_get_regression_features(das_solver_t* s, const char* name, double* features, double* output, long long* fail3);
int das_calc_dregressionpar_product(das_solver_t* s, const char* name, const char* outputName, const char* outputType, const double* seeds,
                                    double* product);
int das_debug_reg_forward(const das_reg_spec_t* spec, const double* par, int nPar, int nCells, const double* features, double* beta, unsigned char* mask);
int das_debug_reg_backward(const das_reg_spec_t* spec, const double* par, int nPar, int nCells, const double* features, const double* g, double* out);

/* das_calc_jac_t_vec_product <-calcJacTVecProduct(inputName,inputType,inputs,outputName,outputType,seeds,product)
 *   pyDASolvers.pyx:208-235 (DASolver.C:1690-1839).  Supported pair on this path: inputType "stateVar",
 *   outputType "residual": product = D_s (dR/dW)^T seeds  (normalizeJacTVecProduct, DASolver.C:1443-1553);
 *   outputType "function" (outputName = function name, one seed): product = seed * D_s dF/dW  (mphys_dafoam.py:746-801). */
int das_get_input_size(das_solver_t* s, const char* inputName, const char* inputType);
int das_get_output_size(das_solver_t* s, const char* outputName, const char* outputType);
int das_calc_jac_t_vec_product(das_solver_t* s, const char* inputName, const char* inputType, const double* inputs,
                               const char* outputName, const char* outputType, const double* seeds, double* product);
/* same product on device buffers (no copies; used by bench.py); d_x,d_y: n doubles in HBM */
int das_drdwt_mult_device(das_solver_t* s, const double* d_x, double* d_y);

/* ---- Krylov solve ------------------------------------------------------------------------
 * das_create_ml_rksp_matrix_free <- createMLRKSPMatrixFree(Mat jacPCMat, KSP ksp) pyDASolvers.pyx:259
 *     (DASolver.C:1102-1119 -> DALinearEqn::createMLRKSP, DALinearEqn.C:28-339): right-preconditioned
 *     restarted GMRES, PC = block (additive-Schwarz-like) ILU(pcFillLevel) of jacPCMat.
 * das_solve_linear_eqn <- solveLinearEqn(KSP, Vec rhs, Vec sol) pyDASolvers.pyx:265 (DALinearEqn.C:341-437);
 *     returns 0 converged / 1 failed by the reference's gmresTolDiff rule (:422-434), <0 on error. */
int das_create_ml_rksp_matrix_free(das_solver_t* s, das_mat_t* pc, das_ksp_t** ksp);
int das_solve_linear_eqn(das_solver_t* s, das_ksp_t* ksp, const double* rhs, double* sol);
/* das_solve_linear_eqn_block: nrhs (1..8) adjoint systems with the same operator through ONE block GMRES (the reference
 *     loops solveLinearEqn over the objective functions, mphys_dafoam.py:478-481): dRdW^T is streamed once per iteration
 *     for all systems, the block orthogonalisation runs as tall-skinny fp64 MFMA GEMMs.  rhs / sol: column-major n x nrhs;
 *     res0 / res (optional, nrhs each): initial / final residual norms.  Returns 1 if any system fails the reference rule. */
int das_solve_linear_eqn_block(das_solver_t* s, das_ksp_t* ksp, int nrhs, const double* rhs, double* sol, double* res0, double* res);
/* preconditioner introspection (tests): y = M^{-1} x on host buffers; block layout of the additive-Schwarz PC:
 * perm[n] = global state index at each permuted position, block_off[nBlocks+1] offsets into perm */
int das_ksp_apply_pc(das_solver_t* s, das_ksp_t* ksp, const double* x, double* y);
int das_ksp_get_n_blocks(das_ksp_t* ksp);
/* nnz(L+U) summed over all (overlapping) blocks and total extended unknowns of the preconditioner */
long long das_ksp_get_factor_nnz(das_ksp_t* ksp);
long long das_ksp_get_n_ext(das_ksp_t* ksp);
int das_ksp_get_blocks(das_ksp_t* ksp, int* perm, long long* block_off);
/* node structure of the default preconditioner (amd.pcType "bilu": one node-block ILU(0) of jacPCMat per GPU, the
 * reference's ASM+ILU stack DALinearEqn.C:199-299 with one sub-domain per rank): nodes of 8 unknown slots in processing
 * (level) order, nodeUnk[8 nNodes] = state index or -1, block CSR bptr[nNodes+1]/bcol[nBlocks] over node positions,
 * lvlPtr[nLevels+1], natural[nNodes] = index of the node in the natural (cell-by-cell) order.  das_pc_structure_* build it on the host without a GPU (tests), das_ksp_get_pc_structure* return
 * the one a KSP was factorised on. */
int das_pc_structure_build(das_solver_t* s, int* nNodes, long long* nBlocks, int* nLevels, int* reach);
int das_pc_structure_get(das_solver_t* s, int* nodeUnk, long long* bptr, int* bcol, int* lvlPtr, int* natural);
int das_ksp_get_pc_structure_sizes(das_ksp_t* ksp, int* nNodes, long long* nBlocks, int* nLevels);
int das_ksp_get_pc_structure(das_ksp_t* ksp, int* nodeUnk, long long* bptr, int* bcol, int* lvlPtr, int* natural);
/* nodeOut[nNodes * 8]: the unknown every slot WRITES: nodeUnk, or -1 for the overlap copies of a multi-block factorisation (amd.pcSubdomains) */
int das_ksp_get_pc_node_out(das_ksp_t* ksp, int* nodeOut);
int das_ksp_get_info(das_ksp_t* ksp, int* iters, double* res0, double* res, double* seconds);
int das_ksp_get_history(das_ksp_t* ksp, double* hist, int cap);
/* Krylov basis of the last solve (amd.krylovBasisPrecision): *fp32 = bit 0: plain fp32 storage, bit 1: split storage (hi + lo floats, the
 * inner products read the hi array only); device bytes mapped so far; bytes per stored basis vector */
int das_ksp_get_basis_info(das_ksp_t* ksp, int* fp32, double* mappedBytes, double* bytesPerVector);
/* columns of every closed Arnoldi cycle of the last solveLinearEqn (reference: KSPGMRESSetRestart, DALinearEqn.C:155 - every cycle
 * but the last holds exactly gmresRestart columns); writes min(cap, count) entries, returns the count */
int das_ksp_get_cycle_lengths(das_ksp_t* ksp, int* lens, int cap);
/* number of Gram-Schmidt refinement passes of the last solve (KSP_GMRES_CGS_REFINE_IFNEEDED, DALinearEqn.C:160); with
 * amd.gmresOrthogonalization "dcgs2": the number of explicit projections (exhausted Krylov space / lost orthogonality) */
int das_ksp_get_n_refine(das_ksp_t* ksp);
/* amd.gmresDeflation = k > 0 (opt-in; round 4, not yet measured on the device): GMRES with deflated restarting (GMRES-DR; PETSc's
 * counterpart is KSPDGMRES, not the reference's default KSPGMRES of DALinearEqn.C:28-339): gmresRestart basis vectors, k harmonic
 * Ritz vectors carried across restarts.  The dense m x m eigenproblem of a restart goes through a process-wide callback
 * fn(m, A row-major, wr, wi, vr, vi) -> 0 (eigenvector e in vr / vi [e m, e m + m)); das_debug_gmres_dr_restart exposes the host
 * algebra of one restart to the CPU tier (returns the number of kept vectors, which never splits a complex pair). */
int das_set_dense_eig_callback(void* fn);
int das_debug_gmres_dr_restart(int m, int kwant, const double* Hbar, const double* rvec, double* P1, double* Hnew, double* cnew);
/* host algebra of the block solve for the CPU tier, all matrices row-major.  das_debug_block_chol: the Cholesky step of CholQR, G (sv x sv
 * Gram matrix) -> L (lower triangular, G = L L^T; a non-positive pivot is replaced by a tiny one) and T = L^-T (upper triangular).
 * das_debug_block_lsq: the block-Hessenberg least squares min |[S0; 0] - Hbar Y| of a cycle of at most m block columns, fed ncols <= m
 * columns as the solver feeds them.  S0: sv x sv.  Hc, Hc2 (the two Gram-Schmidt passes, summed inside): ncols slabs of m sv x sv, slab j
 * holds the (j+1) sv rows of block column j in its first rows.  S: ncols slabs of sv x sv (upper triangular sub-diagonal blocks).  Out:
 * Y (ncols sv x sv) and res (sv: the recurrence residual norm of every right-hand side after the last column). */
int das_debug_block_chol(int sv, const double* G, double* L, double* T);
int das_debug_block_lsq(int sv, int m, int ncols, const double* S0, const double* Hc, const double* Hc2, const double* S, double* Y, double* res);
/* the deflated-restart iteration itself on HOST vectors (operator A and preconditioner M as callbacks fn(x, y, user)): the very loop the
 * device solver runs, for the CPU tier; info4 = {iterations, deflated restarts, plain restarts, breakdowns}, res2 = {|r0|, |r|} */
int das_debug_gmres_dr_host(long long n, void* A, void* M, void* user, const double* b, double* x, int m, int kdef, double rtol, double atol,
                            long long maxIts, double* hist, int histCap, double* info4, double* res2);
/* amd.krylovMethod "idrs" (opt-in): IDR(s) with biorthogonalisation (van Gijzen and Sonneveld, ACM TOMS 38, 2011) instead of GMRES in
 * das_solve_linear_eqn and das_ksp_begin_device / advance / end - 3 s + O(1) work vectors whatever the iteration count, no Krylov basis
 * (amd.idrShadowVectors s = 1 .. 8, amd.idrSeed).  adjEqnOption.gmresMaxIters bounds the operator products (the true-residual ones
 * included), das_ksp_get_info's iters is their number and the history holds one residual norm per product; the reported residual is
 * always the true one.  The solve is not resumable step by step: the first das_ksp_advance after das_ksp_begin_device runs all of it and
 * returns 1.  Fixed-iteration windows and the Newton primal's inner solves keep GMRES; a sharded solve, or amd.gmresDeflation > 0, is an
 * error.  das_ksp_get_status: reason 2 = a restarted run did not halve the true residual, 3 = non-finite residual (fail flag set).
 * das_ksp_get_idr_info: s as used (clamped to n), completed cycles, restarts from the true residual and breakdowns of the last IDR(s)
 * solve; the work vectors the path holds (3 s + 5: P, G, U, r, z, t, right-hand side, solution) and their bytes (8 n each); all 0 for a KSP
 * that never ran it */
int das_ksp_get_idr_info(das_ksp_t* ksp, int* s, int* cycles, int* restarts, int* breakdowns, int* workVectors, double* workBytes);
/* the IDR(s) iteration itself on HOST vectors from x = 0 (operator A and preconditioner M as callbacks fn(x, y, user)): the very loop the
 * device solver runs, for the CPU tier; info4 = {products, stop reason, restarts, breakdowns}, res2 = {|r0|, |r|} (true residuals) */
int das_debug_idrs_host(long long n, void* A, void* M, void* user, const double* b, double* x, int s, int seed, double rtol, double atol, long long maxIts,
                        double* hist, int histCap, double* info4, double* res2);
/* exactly one cycle (s + 1 products) of that loop from x = 0 and the state it leaves: x, the recurrence residual r (n), the orthonormal
 * shadow space P and the spaces G, U (column-major n x s) */
int das_debug_idr_cycle_host(long long n, void* A, void* M, void* user, const double* b, double* x, int s, int seed, double* r, double* P, double* G,
                             double* U);
/* test-only entries of the IDR(s) kernels (tests/test_gpu_idr_kernels.py): caller data up, the solver's launch helpers, data down.
 * shadow: P (s columns, ld apart) = the raw hash of (seed, row, column); device = 0 fills it on the host (no GPU needed) */
int das_debug_idr_shadow(long long n, int s, long long ld, int seed, int device, double* P);
/* k_idr_combine: y[0..n) = a x + sum_{i < m} c_i V_i, V = m columns ld apart in an array of vlen entries; yoff >= 0: y = V + yoff (in
 * place; y, ylen unused), else y is an array of ylen >= n entries.  V is copied back in both cases */
int das_debug_idr_combine(long long n, int m, double a, const double* x, double* V, long long ld, long long vlen, const double* c, long long yoff, double* y,
                          long long ylen);
/* k_idr_biortho_step + k_reduce: step k on G, U (glen entries each, columns ld apart), r, x (vlen >= n entries each), coef = [alpha (k);
 * beta]; *rr = r.r afterwards.  All four arrays are copied back */
int das_debug_idr_biortho_step(long long n, int k, double* G, double* U, long long ld, long long glen, const double* coef, double* r, double* x,
                               long long vlen, double* rr);
/* k_idr_smooth_step + k_reduce: r -= omega t, x += omega z on r, x (vlen >= n entries each), P = s columns ld apart in plen entries;
 * out[0..s) = P^T r, out[s] = r.r afterwards.  r, x and P are copied back */
int das_debug_idr_smooth_step(long long n, int s, double omega, double* r, const double* t, double* x, const double* z, long long vlen, double* P,
                              long long ld, long long plen, double* out);
/* amd.polyDegree = d (opt-in, 0 = off, 1 .. 16): polynomial-preconditioned GMRES.  With B = A M^-1 (M^-1: the whole preconditioner) the
 * first Arnoldi cycle of a solve is closed after d columns; the roots of its GMRES residual polynomial - the harmonic Ritz values, in
 * modified Leja order, a complex pair once - define p of degree d - 1, and every later column is w = B p(B) v: d operator products with
 * nothing but element-wise updates between them; a cycle closes with x += M^-1 p(B) (V y).  A generating cycle that ends early, or roots
 * that are unusable (zero, not finite, no dense eigen-solver callback: das_set_dense_eig_callback), leave the solve without a polynomial
 * (degree 0, fallback 1).  adjEqnOption.gmresMaxIters bounds the operator products (polynomial, closing steps and true residuals included;
 * a column the budget does not cover is not started), gmresRestart the basis columns; das_ksp_get_info's iters is the number of
 * products, the history keeps one entry per column.  das_ksp_get_status: reason 3 = non-finite residual (fail flag set).  Fixed-iteration
 * windows and the Newton primal's inner solves ignore the option; amd.krylovMethod "idrs", amd.gmresDeflation > 0, a block solve, a
 * sharded solve or a degree outside 0 .. 16 is an error.
 * das_ksp_get_poly_info: the last solve's degree as used, complex pairs, operator products, Arnoldi columns built AFTER the generating
 * cycle (the basis the option is about; with a polynomial they are columns of B p(B)), the columns of the generating cycle itself (the
 * history holds one entry per column of both), whether a polynomial was generated, the fallback flag, the work vectors (3 once a polynomial was built) and their bytes (8 n each), and the ordered roots (re, im: room for 16
 * entries each; nRoots of them are written); all 0 for a KSP whose last solve ran without the option */
int das_ksp_get_poly_info(das_ksp_t* ksp, int* degree, int* nComplexPairs, long long* products, long long* columns, long long* generatingColumns, int* generated,
                          int* fallback, int* workVectors, double* workBytes, int* nRoots, double* re, double* im);
/* test-only entries of amd.polyDegree.  roots: the ordered roots of a (d + 1) x d unrotated Hessenberg matrix (row-major); returns the
 * number of entries written to re / im (real roots and pairs, a pair by its member with im > 0), 0 = fallback (no usable polynomial) */
int das_debug_poly_roots(int d, const double* Hbar, double* re, double* im);
/* out = p(B) v on HOST vectors, B = A M^-1 with A and M^-1 as callbacks fn(x, y, user): the root walk the device solver runs */
int das_debug_poly_apply_host(long long n, void* A, void* M, void* user, int nroots, const double* re, const double* im, const double* v, double* out);
/* one root step through the solver's launch helper on caller data: kind 0 = real root (poly (+)= prod / re; unless last: prod -= w / re),
 * 1 = first step of a pair (tmp = 2 re prod - w; poly (+)= tmp / (re^2 + im^2)), 2 = second step of a pair (prod -= w / (re^2 + im^2);
 * nothing is launched when last).  first: prod is read from v, poly is not read.  Every array has len entries with its vector in
 * [off, off + n); the device copies keep the offset (odd off: element-wise path).  All five arrays are copied back */
int das_debug_poly_step(long long n, int kind, int first, int last, double re, double im, long long off, long long len, double* v, double* w, double* prod, double* poly,
                        double* tmp);
/* out = p(B) v on the device with the roots of this KSP's last solve (after initializedRdWTMatrixFree) */
int das_debug_ksp_poly_apply(das_solver_t* s, das_ksp_t* ksp, const double* v, double* out);
/* how the last solve ended: reason 0 = tolerance met (KSP_CONVERGED_RTOL/ATOL), 1 = gmresMaxIters reached (KSP_DIVERGED_ITS),
 * 2 = stopped on stagnation after a Krylov breakdown / at the attainable accuracy (PETSc: KSP_CONVERGED_HAPPY_BREAKDOWN /
 * KSP_DIVERGED_BREAKDOWN; the reference's failure flag is still the tolerance rule of DALinearEqn.C:422-434);
 * nBreakdown = happy breakdowns detected, nSweepGrid / sweepPerXcd = launch shape of the preconditioner sweeps */
int das_ksp_get_status(das_ksp_t* ksp, int* reason, int* nBreakdown, int* nSweepGrid, int* sweepPerXcd);
/* Stability estimate of the incomplete factorisation, max |(LU)^-1 P e - e| on two test vectors (amd.pcStabilityLimit; -1: not computed),
 * and the elimination order of the cells the check settled on (0 mesh numbering, 1 reverse Cuthill-McKee = jacMatReOrdering "rcm",
 * 2 Cuthill-McKee, 3 mesh numbering backwards, 4 / 5 along / against the mean flow; -1: no check).  A factorisation above the limit is
 * rebuilt with the next order, rank by rank.  The reference's PETSc ILU has no such check; its MatFactorInfo shift (DALinearEqn.C:270-272)
 * only replaces zero pivots. */
int das_ksp_get_pc_stability(das_ksp_t* ksp, double* estimate, int* orderUsed);
/* amd.pcSubdomains K (default -1: 4 from 1 M cells on): restricted additive Schwarz INSIDE the rank - K node-block ILUs on recursive-coordinate-
 * bisection blocks of the cells plus adjEqnOption.asmOverlap rings, each with its own elimination order, merged into one level structure so
 * that one pair of sweeps runs them together (the reference reaches several sub-domains per device only through more MPI ranks,
 * DALinearEqn.C:212-216).  Returns K (1: one factorisation, -1: null handle); orders[K] / estimates[K] are optional. */
int das_ksp_get_pc_subdomains(das_ksp_t* ksp, int* orders, double* estimates);
/* two-level preconditioner (amd.pcCoarseAggregates / pcCoarseField / pcCoarseMode): number of aggregates of the
 * piecewise-constant pressure coarse space (0 = none) and, optionally, the aggregate of every cell (-1 = not owned) */
int das_ksp_get_coarse(das_ksp_t* ksp, int* aggOfCell);
/* 1 if the deflated coarse correction of this KSP takes A (Z u) from the precomputed sparse A Z (amd.pcCoarseSparseAZ, round 5), 0 if it runs
 * a full operator product per apply - test aid */
int das_ksp_coarse_sparse_az_active(das_ksp_t* ksp);
/* multi-GPU: ONE coarse space over all ranks instead of one per rank (the reference's ASM level couples the sub-domains through
 * its overlap, DALinearEqn.C:199-216; a per-rank coarse space lets the iteration count grow with the number of GPUs).
 * Collective over the installed communication.  naggGlobal <= 2048: size of the global coarse operator; aggOffset: position of
 * this rank's aggregates; aggRowGlobal[nLocalCells]: global aggregate of every local cell, owned (= aggOffset + local id) and
 * ghost (the owner rank's numbering), -1 = none.  Returns 0, or 1 if the coarse operator is singular (no correction). */
int das_ksp_set_global_coarse(das_solver_t* s, das_ksp_t* ksp, int naggGlobal, int aggOffset, const int* aggRowGlobal);
/* run exactly `iters` GMRES iterations on device-resident rhs/sol (bench.py "step"); no convergence exit */
int das_ksp_run_fixed_device(das_solver_t* s, das_ksp_t* ksp, const double* d_rhs, double* d_sol, int iters);
/* the same solve advanced in pieces on device-resident rhs/sol (bench.py times a window of iterations deep inside an
 * Arnoldi cycle): begin -> advance(n) ... -> end.  advance returns 1 once the solve is over (never in `fixed` mode),
 * end closes the open cycle (x += M^-1 V y, true residual) and returns the solveLinearEqn fail code. */
int das_ksp_begin_device(das_solver_t* s, das_ksp_t* ksp, const double* d_rhs, double* d_sol, int fixed);
int das_ksp_advance(das_solver_t* s, das_ksp_t* ksp, int iters);
int das_ksp_end(das_solver_t* s, das_ksp_t* ksp);
void das_ksp_destroy(das_ksp_t* k);

/* ---- multi-GPU sharding (one process per GPU; reference: MPI domain decomposition, one OpenFOAM sub-domain per rank) ----
 * The solver instance holds the rank's EXTENDED sub-mesh (owned cells + ghost layers).  owned[j] != 0 marks the
 * states/residuals this rank owns (DAIndex ordering of the extended mesh).  With a mask set:
 *   - assembled matrices keep only columns (residuals) owned by this rank (rows = all extended states),
 *   - the preconditioner is built on owned cells only,
 *   - after every operator product the halo callback is invoked on the device vector so that ghost-row
 *     contributions can be sent to their owner ranks and added there (then zeroed locally),
 *   - every fused dot-product result (device buffer of n doubles) goes through the all-reduce callback.
 * Callbacks run on the stream given to das_set_stream (pass the communication library's current stream). */
typedef void (*das_halo_cb)(double* d_vec, void* user);
typedef void (*das_allreduce_cb)(double* d_buf, int n, void* user);
int das_set_owned_mask(das_solver_t* s, const unsigned char* owned /* n states */);
int das_set_comm(das_solver_t* s, das_halo_cb halo, das_allreduce_cb allreduce, void* user);
/* Native transport set-up, step 1 (local, not collective): dlopen the RCCL PyTorch already loaded and bind its symbols.
 * All ranks exchange the return code (torch.distributed MIN all-reduce) BEFORE any of them calls the collective
 * das_comm_init_rccl: a rank without RCCL must not leave its peers blocked in ncclCommInitRank. */
int das_comm_load_rccl(void);
/* Native transport (no host code in the iteration loop): RCCL point-to-point halo reduction overlapped with the owned-row
 * product + in-stream ncclAllReduce of the Gram-Schmidt dots.  Reference: PETSc VecScatter of the MPIAIJ off-diagonal
 * block in MatMult and MPI_Allreduce in VecMDot (KSPGMRES, DALinearEqn.C:341-437).
 *   das_comm_unique_id   rank 0: 128-byte RCCL id, distributed by the host side (bootstrap only)
 *   das_comm_init_rccl   every rank: communicator on the solver's device
 *   das_comm_set_halo    the halo plan: peers[npeers]; sendIdx[sendOff[i]..sendOff[i+1]) = extended rows held for peer i
 *                        (evaluated first, sent); recvIdx[...] = my owned rows peer i holds as ghosts, in its send order;
 *                        ghostIdx[nGhost] = all local ghost rows (zeroed after the reduction)
 *   das_set_exchange_cb  host-staged transport of the same plan (gloo tests on single-GPU boxes) */
typedef void (*das_exchange_cb)(double* d_send, double* d_recv, void* user);
int das_comm_unique_id(char* out128);
int das_comm_init_rccl(das_solver_t* s, int rank, int world, const char* id128);
int das_comm_set_halo(das_solver_t* s, int npeers, const int* peers, const long long* sendOff, const int* sendIdx, const long long* recvOff,
                      const int* recvIdx, long long nGhost, const int* ghostIdx);
int das_set_exchange_cb(das_solver_t* s, das_exchange_cb cb, void* user);
/* Additive-Schwarz overlap of the preconditioner across ranks - adjEqnOption.asmOverlap, reference DALinearEqn.C:212-216
 * (PCASMSetOverlap; PETSc's default restricted variant): pcMask[state] != 0 for the unknowns of this rank's sub-domain solve (owned +
 * overlap rings of ghost cells); per peer of das_comm_set_halo (same order) the owned states it needs (ovSend) and the overlap ghost
 * states it owns (ovRecv, in its send order).  Call before calcdRdWT(1) / createMLRKSPMatrixFree.  pcMask NULL: no overlap.
 * das_set_gather_cb: host-staged transport of the gather (gloo tests on single-GPU boxes). */
int das_set_pc_overlap(das_solver_t* s, const unsigned char* pcMask /* n states */, int npeers, const long long* ovSendOff, const int* ovSendIdx,
                       const long long* ovRecvOff, const int* ovRecvIdx);
int das_set_gather_cb(das_solver_t* s, das_exchange_cb cb, void* user);
int das_comm_is_native(das_solver_t* s);
/* drop the native communicator again (all ranks fall back to the callback transport together) */
int das_comm_reset(das_solver_t* s);
int das_set_stream(das_solver_t* s, void* hip_stream);

/* ---- timing (getElapsedClockTime/getElapsedCpuTime pyDASolvers.pyx:332-336) and kernel timers */
double das_get_elapsed_clock_time(das_solver_t* s);
double das_get_elapsed_cpu_time(das_solver_t* s);
/* average duration [ms] of the named kernel family measured with HIP events on the launch stream since
 * the last reset: "spmv", "pc", "residual" ; returns <0 if never launched */
double das_timer_avg_ms(das_solver_t* s, const char* name);
/* tuning hook (tools/orth_bench.py): average ms of the two kernels of the delayed re-orthogonalisation (inner products with
 * `rows` rows per thread; update with `unroll` basis vectors in flight and `rpt` rows per thread) on synthetic vectors of
 * length n against K basis vectors; -1 for a variant that is not compiled in */
int das_debug_orth_bench(long long n, int K, int reps, int rows, int unroll, int rpt, double* ms_dots, double* ms_update);
/* the same for the float basis in the solver's layout (fmt 1 = fp32, 2 = split): variant 0 = the one-dword-per-lane kernels,
   1 = the 16-byte-load kernels (rows and rpt count groups of 4 rows per lane), 2 = 1 with non-temporal loads */
int das_debug_orth_bench_split(long long n, int K, int reps, int fmt, int variant, int rows, int unroll, int rpt, double* ms_dots, double* ms_update);
/* 16-byte-load path of the float basis on / off for the later launches of this process (tests, timing tool) */
int das_debug_set_orth_wide(int on, int* previous);
/* does a basis of this shape, uploaded by das_debug_krylov_dots2 / _dcgs2_update, take the 16-byte-load kernels? */
int das_debug_krylov_wide_eligible(long long n, int fmt, long long ld, int* dots, int* update);
/* ---- TEST-ONLY entries (tests/test_gpu_krylov_kernels.py).  Nothing in the product path calls them and no binding should: they exist
 * so that every Krylov kernel of the GMRES engine can be compared with a high-precision reference on caller data, one kernel at a
 * time.  They need the device but no solver handle: host arrays are uploaded, the launch helper THE SOLVER USES is run on the null
 * stream, the result is downloaded.  Bad arguments (sizes <= 0, s outside 1..8, a leading dimension below n, null pointers) return
 * DAS_ERR_ARG with a message.
 * Basis storage `fmt`: 0 = fp64 (V: double, slot stride ld >= n), 1 = fp32 (V: float, ld >= n), 2 = split (V: float, slot = hi
 * array followed by the lo array n floats further, ld >= 2 n).  Arrays that a kernel writes are uploaded and downloaded whole, so
 * that the caller can put a sentinel around the written range and find it untouched. */
/* k_multidot2 + k_reduce: out[0..K) = V^T u, out[K..2K) = V^T v with u = slot K - 1 (split: its hi array) */
int das_debug_krylov_dots2(long long n, int K, int fmt, const void* V, long long ld, const double* v, double* out);
/* k_dcgs2_update on slots 0..j+1 of V (nslots >= j + 2 slots, in place): sc = [s (j); c (j)] */
int das_debug_krylov_dcgs2_update(long long n, int j, int fmt, void* V, long long ld, int nslots, const double* sc, double gamma, double ralpha,
                                  const double* v);
/* k_multidot + k_reduce: out[0..m) = V^T w, out[m] = w.w (m >= 0; fp32 and split read the hi array) */
int das_debug_krylov_multidot(long long n, int m, int fmt, const void* V, long long ld, const double* w, double* out);
/* k_multiaxpy: w -= sum_i h_i V_i in place on wlen >= n entries (wfloat: w is float, fp32 basis only) */
int das_debug_krylov_multiaxpy(long long n, int m, int fmt, const void* V, long long ld, const double* h, int wfloat, void* w, long long wlen);
/* k_lincomb: y[0..n) = sum_i c_i V_i, y holds ylen >= n entries */
int das_debug_krylov_lincomb(long long n, int m, int fmt, const void* V, long long ld, const double* c, double* y, long long ylen);
/* k_scale_to, y = a x: use 0 double -> double, 1 double -> float, 2 double -> split (lo at y + n), 3 split -> double (lo at x + n),
 * 4 float -> double; y holds ylen >= n (use 2: 2 n) entries of its type */
int das_debug_krylov_scale_to(long long n, double a, int use, const void* x, void* y, long long ylen);
/* block_tn (k_tsgemm_tn + k_tsgemm_reduce): C (K x s row-major) = V^T W; the block V starts voff doubles into the uploaded array
 * (voff + K ldv doubles); even leading dimensions with an odd voff are rejected (16-byte loads) */
int das_debug_krylov_block_tn(long long n, int K, int s, const double* V, long long ldv, long long voff, const double* W, long long ldw, double* C);
/* block_nn_sub (k_tsgemm_nn_sub): W -= V C in place */
int das_debug_krylov_block_nn_sub(long long n, int K, int s, const double* V, long long ldv, const double* C, double* W, long long ldw);
/* k_block_right_mult: W <- W T (T: s x s row-major) in place */
int das_debug_krylov_block_right_mult(long long n, int s, double* W, long long ldw, const double* T);
/* k_block_lincomb: Y_r = sum_i V_i C[i s + r] */
int das_debug_krylov_block_lincomb(long long n, int K, int s, const double* V, long long ldv, const double* C, double* Y, long long ldy);
/* block_spmm (k_block_to_rows<S> + k_spmm_wave<S>, S = 2, 4 or 8 chosen from s): Y_r = A X_r for a square CSR matrix */
int das_debug_krylov_block_spmm(long long n, int s, const long long* rowptr, const int* colidx, const double* vals, const double* X, long long ldx,
                                double* Y, long long ldy);
/* ---- TEST-ONLY entries (tests/test_gpu_bilu_kernels.py): the node-block ILU(0) preconditioner on a caller-made node structure and
 * scalar CSR matrix, kernel by kernel.  No mesh, no solver handle; the numeric setup and the sweeps THE SOLVER USES run on the null
 * stream.  The structure is checked on the host before anything is launched, and DAS_ERR_ARG is returned for a null pointer (nodeOut
 * alone may be null: nodeOut = nodeUnk), sizes <= 0, An > n, and for anything that is not a valid level-ordered structure: bptr not
 * monotone, block columns of a row not ascending, out of range or without the diagonal at bdiag, a pattern that is not symmetric,
 * lvlPtr not covering [0, nNodes], an entry J < p of row p with level(J) >= level(p), slots >= 8, unkNode outside [-1, nNodes), CSR
 * columns >= An, nodeUnk / nodeOut outside [-1, n).  Matrix entries outside the node pattern that are not late-late couplings stay the
 * DAS_ERR_INTERNAL of the solver's setup. */
typedef struct {
    int nNodes, nLevels, nMaps; /* nodes in processing order, levels, (unkNode, unkSlot) maps (one per block of a multi-block factor) */
    int fp32, transpose;        /* factor stored as float; factorise the transposed matrix */
    long long n, An;            /* length of a vector of unknowns; rows (= columns) of the CSR matrix, An <= n */
    const int* nodeUnk;         /* nNodes*8: unknown of a slot or -1 */
    const int* nodeOut;         /* nNodes*8 or null: where the slot's solution is written, -1 for an overlap copy */
    const unsigned char* late;  /* nNodes */
    const long long* bptr;      /* nNodes+1 */
    const long long* bdiag;     /* nNodes: position of the diagonal block */
    const int* bcol;            /* bptr[nNodes] */
    const int* lvlPtr;          /* nLevels+1 */
    const int* unkNode;         /* nMaps*An: node of an unknown or -1 */
    const unsigned char* unkSlot; /* nMaps*An */
    const long long* rp;        /* An+1 */
    const int* ci;
    const double* val;
    double diagScale;           /* diagonal entries of the rows below shiftEnd outside [shiftExLo, shiftExHi) are multiplied by it */
    long long shiftExLo, shiftExHi, shiftEnd;
} das_bilu_debug_t;
/* k_bilu_scatter, k_bilu_pad_diag, k_bilu_factor, k_bilu_pack: Lptr / Uptr (nNodes+1; U rows by q = nNodes-1-p), Lcol / Ucol, the
 * packed Lval / Uval (64 per block, per pass of nb <= 8 blocks [qq][g][k][2]; float if fp32 else double), invD (nNodes*64) and the
 * number of shifted pivots */
int das_debug_bilu_factor(const das_bilu_debug_t* in, long long* Lptr, long long* Uptr, int* Lcol, int* Ucol, void* Lval, void* Uval, double* invD,
                          int* nshift);
/* the same setup, then k_bilu_reset + k_bilu_sweep (nrhs = 1) or bilu_apply_multi (nrhs = 2..8: groups of 4, 2, 1), twice if `twice`;
 * b, out column-major nrhs x ld, ld >= n; out is uploaded before every application, so entries nothing writes keep the caller's
 * values.  y, z (nNodes*8*4 doubles each): the work vectors of the LAST group launched, [(node*8+slot)*S + r] with S = 4, 2 or 1 its
 * width.  info = {launchGrid, launchSleep, launchPerXcd, xcdProbe} */
int das_debug_bilu_apply(const das_bilu_debug_t* in, int nrhs, long long ld, const double* b, double* out, int twice, double* y, double* z,
                         int* abortFlag, int* info);
/* ---- TEST-ONLY entries (tests/test_gpu_graph_kernels.py, tests/test_gpu_opmat_kernels.py): the graph set-up kernels of the colouring
 * input, the jacLowerBounds filter, the packed operator and the ghost-row product on caller-made CSR structures, kernel by kernel.  No
 * mesh, no solver handle; the launch sequences THE SOLVER USES run on the null stream.  These kernels index with what they are given,
 * so everything is checked on the host before anything is launched, and DAS_ERR_ARG is returned for a null pointer, a size <= 0,
 * rowptr[0] != 0, a decreasing rowptr, a column or row index outside [0, n), columns of a row that do not ascend strictly (transpose
 * and nets), a pattern without entries (transpose and nets), kept rows out of range or repeated, row0 + 3 nG > n, and an output array
 * too short for what is written.  All matrices are n x n.  Arrays that a kernel writes into at caller-given places (out, y, buf) are
 * uploaded and downloaded whole, so that the caller can put a sentinel around the written range and find it untouched. */
/* device_exclusive_scan (k_scan_block_sums, k_scan_apply): out[0..n] = exclusive prefix of the counts (>= 0), *total = out[n] */
int das_debug_graph_scan(long long n, const int* cnt, long long* out, long long* total);
/* device_transpose (k_tr_count, scan, k_tr_fill, k_sort_rows): trp (n+1), tcol (nnz) = the transposed pattern, rows ascending */
int das_debug_graph_transpose(long long n, const long long* rowptr, const int* col, long long* trp, int* tcol);
/* device_transpose, then device_build_nets (k_net_count, scan, k_net_fill, k_group_flags) for the kept rows keep[0..nKeep) (net q = row
 * keep[q]; nKeep = 0 is allowed): cptr (n+1), crow / cpos (*total <= nnz entries: the nets of a column in ascending row order and the
 * position of the column in each of those rows), isStart (n) */
int das_debug_graph_nets(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, long long* cptr, int* crow, int* cpos,
                         unsigned char* isStart, long long* total);
/* k_rows_gather: out[dst[q] ..] = the columns of row rows[q], q < nSel; out holds outLen entries */
int das_debug_graph_rows_gather(long long nSel, const long long* rows, long long n, const long long* rowptr, const int* col, const long long* dst, int* out,
                                long long outLen);
/* filter_compact (k_count_keep, k_compact): the entries with |v| > bound (if useBound) or on the diagonal, of the columns with
 * owned[col] != 0 (owned may be null: all); nrp (n+1), nci / nv (*nnzOut <= nnz entries) */
int das_debug_compact(long long n, const long long* rowptr, const int* col, const double* vals, double bound, int useBound, const unsigned char* owned,
                      long long* nrp, int* nci, double* nv, long long* nnzOut);
/* vecpack_build (k_vecpack_count, k_vecpack_fill) of the group rows [row0, row0 + 3 nG): *built = 0 when the three rows of a group do
 * not share their column list (nothing else is written), else cptr (nG+1), data (*nChunks chunks of 448 bytes; dataCap bytes must hold
 * them) and, unless x is null, launch_spmv over the whole matrix (k_spmv_vec3 + k_spmv_wave on the rows before and after the pack) into
 * y[0..n), y holding ylen >= n entries */
int das_debug_vecpack(long long n, const long long* rowptr, const int* col, const double* vals, long long row0, long long nG, int* built, long long* cptr,
                      unsigned char* data, long long dataCap, long long* nChunks, const double* x, double* y, long long ylen);
/* k_spmv_rows_to_buf: buf[k] = A[rows[k], :] . x, k < nrows; buf holds buflen >= nrows entries */
int das_debug_spmv_rows(long long nrows, const int* rows, long long n, const long long* rowptr, const int* col, const double* vals, const double* x, double* buf,
                        long long buflen);
/* ---- TEST-ONLY entries (tests/test_gpu_color_kernels.py): the colouring kernels (csrc/das_color.hpp) on a caller-made n x n CSR
 * pattern (columns of a row strictly ascending) and the kept rows keep[0..nKeep) (net q = row keep[q], nKeep >= 1).  No mesh, no solver
 * handle; everything runs on the null stream.  The structures the kernels index with (column -> nets with positions, groups, net ->
 * columns) are derived from the pattern with the helpers THE SOLVER USES (device_transpose, device_build_nets, color_groups_from_flags,
 * k_rows_gather).  Everything is checked on the host before anything is launched, and DAS_ERR_ARG is returned for everything
 * das_debug_graph_nets refuses, for n >= 2^31, nKeep < 1, a colour outside [-1, 64 W), W < 1 or above what the LDS of k_spec_conflict
 * holds (160 words at most; fewer if the device says so), S < 1, a spread that is neither -1 nor >= 1, a negative round and an output
 * array too short for what is written. */
/* color_firstfit_run (k_color_firstfit, the bitmaps doubled from 8 words on overflow) as the graph path of the solver runs it: *rc = 1
 * and colors[0..n), *W = the bitmap words that sufficed; *rc = 0 (gave up) or -1 (watchdog) and nothing else.  colors holds colorsLen
 * >= n entries */
int das_debug_color_firstfit(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, int* colors, long long colorsLen,
                             int* rc, int* W);
/* color_speculative_run: spread = -1 is the rule of the solver (1.25 x the longest net, DAS_COLOR_SPREAD), spread >= 1 is taken as it
 * is.  *ok = 1: colors[0..n), *rounds, *S and *W of the run that succeeded; *ok = 0: the bitmaps cannot be widened any further */
int das_debug_color_speculative(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, int spread, int* colors,
                                long long colorsLen, int* ok, int* rounds, int* S, int* W);
/* one round from the final colours colorsIn (-1 = none): k_spec_netbits, k_spec_assign (-> tent), k_spec_conflict(0) (-> lose),
 * k_spec_commit (-> colorsOut, *left), k_spec_netbits (-> F, nKeep x W words), *overflow = a column found no colour below 64 W.  tent,
 * lose and colorsOut hold outLen >= n entries, F holds FLen >= nKeep W */
int das_debug_color_spec_round(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, const int* colorsIn, int S, int W,
                               int round, int* tent, unsigned char* lose, int* colorsOut, long long outLen, unsigned long long* F, long long FLen,
                               unsigned* left, int* overflow);
/* k_spec_conflict with check = 1 alone: *invalid = 1 if two columns of a net share a colour or a column of a net has none */
int das_debug_color_check(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, const int* colors, int W, int* invalid);
/* ---- TEST-ONLY entries (tests/test_gpu_reduce_kernels.py): the two-stage fixed-order reductions the objective functions end in, and
 * the two gathers without atomics, on caller-made arrays.  No mesh, no solver handle; each entry runs THE LAUNCH HELPER THE SOLVER RUNS
 * (csrc/das_facefn.hpp, das_cellfn.hpp, das_meshquality.hpp, das_heatsource.hpp, das_actuatordisk.hpp, das_reduce.hpp) on the null
 * stream.  Every array that is not const - input or output - is uploaded whole and downloaded whole: the caller finds its inputs as
 * the device left them and puts sentinels behind the written range of an output (its length is an argument).  *nb = the workgroups of
 * the first stage: the first *nb entries of a partial array are written.  Everything is checked on the host before anything is
 * launched; DAS_ERR_ARG for a null pointer (where null is not named as allowed), a size outside its range (n < 2^31), an index a
 * kernel would read out of range with, and an array too short. */
/* launch_ks_max, launch_ks_expsum, launch_ks_weights: ms = {m, S} (msLen >= 2), pmax / psum = the partials of the two stages (partLen >=
 * 1024 each), w[t] = outer exp(k a_t - m) / S (wLen >= n); n >= 1 */
int das_debug_reduce_ks(long long n, double* a, double k, double outer, double* ms, long long msLen, double* pmax, double* psum, long long partLen, double* w,
                        long long wLen, int* nb);
/* launch_group_sum: out2[g] = the sum of fv over group g (group null: all in group 0); cnt >= 0, outLen >= 2 */
int das_debug_reduce_group_sum(long long cnt, unsigned char* group, double* fv, double* out2, long long outLen);
/* launch_tangent_dot: out2[0] = sum_i psi_i R[2 i + 1] (R: n dual numbers {value, tangent}), all 1024 partials written; n >= 0, partLen
 * >= 1024, outLen >= 2 */
int das_debug_reduce_tangent_dot(long long n, double* R, double* psi, double* part, long long partLen, double* out2, long long outLen, int* nb);
/* launch_ad_dot: the same product through k_ad_dot_partial + k_hs_final; n >= 1, partLen >= 1024, outLen >= 1 */
int das_debug_reduce_ad_dot(long long n, double* R, double* psi, double* part, long long partLen, double* out, long long outLen, int* nb);
/* launch_sv_dot: out2[0] = a . b; n >= 1, partLen >= 512, outLen >= 2 */
int das_debug_reduce_sv_dot(long long n, double* a, double* b, double* part, long long partLen, double* out2, long long outLen, int* nb);
/* launch_cellfn_value: out[0] = coef sum_t w_t g(src[idx_t] - data_t) (data null: 0; w_t = V[cell_t] with mv, g = x^2 with square);
 * launch_cellfn_grad with the factor g and the scales sc (nSrc entries, or null) into grad, whose first nSrc entries the entry zeroes
 * (gradLen >= nSrc).  idx entries are distinct; partLen >= 1024 */
int das_debug_reduce_cellfn(long long nt, int* cell, long long* idx, double* data, int square, int mv, long long nCells, const double* V, long long nSrc, double* src,
                            double coef, double* part, long long partLen, double* out, long long outLen, double* sc, double g, double* grad, long long gradLen, int* nb);
/* launch_rn_sum, launch_rn_seeds on nblocks <= 8 residual blocks {off, kind (0 vector 3 nC, 1 scalar nC, 2 face nF), w}: term[i]
 * (termLen >= n), ms[1] = their sum (msLen >= 2, ms[0] untouched), g[i] = coef dF/dR_i at the given F (gLen >= n; L2Norm: F != 0) */
int das_debug_reduce_rn(long long n, int nblocks, const long long* off, const int* kind, const double* w, long long nC, long long nF, long long nIF, int l1, double* R,
                        double* term, long long termLen, double* part, long long partLen, double* ms, long long msLen, double F, double coef, double* g, long long gLen,
                        int* nb);
/* launch_hs_sum<double> for kind 0 (cylinderToCell: member[nC]) and 2 (field[nC]) on cells of volume V[c]: psi null: sum s V; else
 * sum (vt ? power s / vt[0] : s) psi (byV ? V : 1); partLen >= 1024 */
int das_debug_reduce_hs_sum(int kind, int nC, const double* V, unsigned char* member, double* field, double* psi, int byV, double power, double* vt, double* part,
                            long long partLen, double* out, long long outLen, int* nb);
/* the second stages on caller-made partials, 1 <= nb <= 1024: pair = 0 launch_hs_final (nb entries -> out[0]), pair = 1 launch_ad_final
 * (nb pairs -> out[0], out[1]); dual = 1: every entry is a dual number {value, tangent}, two doubles */
int das_debug_reduce_final(int pair, int dual, int nb, double* part, long long partLen, double* out, long long outLen);
/* launch_mq_owner_gather: tc[c] = the sum of ft over the faces cell c owns (cf_face >= 0) in the order of its list; ft holds nFt entries */
int das_debug_reduce_owner_gather(int nC, int* cf_ptr, int* cf_face, long long nFt, double* ft, double* tc, long long tcLen);
/* launch_vm_gather: out[j] = seed (tc[c] + sum of tc over the neighbours across internal faces), c = j / 3, for the states j < 3 nC
 * with colors[j] == col; every other entry of out is left as it is (outLen >= 3 nC) */
int das_debug_reduce_vm_gather(int nC, int nIF, int* cf_ptr, int* cf_face, int* cf_other, int* colors, int col, double* tc, double seed, double* out, long long outLen);
/* ---- TEST-ONLY entries (tests/test_gpu_coarse_kernels.py): the coarse space of the two-level preconditioner (csrc/das_coarse.hpp) on
 * caller-made structures, kernel by kernel.  No mesh, no solver handle; the launch sequences THE SOLVER USES run on the null stream.
 * These kernels index with what they are given, so everything is checked on the host before anything is launched, and DAS_ERR_ARG is
 * returned for a null pointer, a size <= 0, nagg outside 1 .. 2048, rowptr[0] != 0, a decreasing rowptr, a column outside [0, n), an
 * aggregate outside [-1, nagg), a field block [off, off + N) that does not lie in [0, n), and an output array too short for what is
 * written.  All matrices are n x n CSR; the field is the unknowns off .. off + N - 1.  An output array WITHOUT a length argument (E, Inv,
 * t, u, cnt, ptr) holds 8 entries more than are written; every output is uploaded and downloaded whole, so that the caller can put a
 * sentinel behind the written range and find it untouched. */
/* coarse_sort_cells of aggRow, coarse_assemble (E = 0, k_coarse_assemble): E[I][J] (nagg x nagg, J x nagg + I with transpose = 1) = the
 * sum of the field-block entries a_ij, i in row aggregate I (aggRow, N cells), j in column aggregate J (aggCol), a diagonal entry
 * (j == i) times diagScale */
int das_debug_coarse_assemble(int nagg, long long N, long long off, long long n, const long long* rowptr, const int* col, const double* vals, const int* aggRow,
                              const int* aggCol, int transpose, double diagScale, double* E);
/* coarse_invert (k_gj_pivot, k_gj_elim per column): Inv = Ein^-1 (n x n, n <= 2048), *singular = 1 when a pivot column holds no
 * nonzero (Inv is then of no use) */
int das_debug_coarse_invert(int n, const double* Ein, double* Inv, int* singular);
/* coarse_sort_cells, coarse_restrict_solve (k_coarse_restrict, k_coarse_solve), k_coarse_prolong: t = Z^T r (nagg), u = Einv t (nagg),
 * y[off + c] = u[agg(c)] and 0 elsewhere (set = 1) or y[off + c] += u[agg(c)] (set = 0); r holds n entries, y ylen >= n */
int das_debug_coarse_correct(int nagg, long long N, long long off, long long n, const int* agg, const double* Einv, const double* r, double* t, double* u, double* y,
                             long long ylen, int set);
/* coarse_az_build (k_az_build pass 0, prefix sum, pass 1), then k_az_apply: cnt (n), ptr (n + 1), oa / ov (*nnz entries of the cap
 * that they hold) = the sparse A Z, per row the aggregates in the order of their first appearance; out[0..n) = v - (A Z) u, or (A Z) u
 * with v null; u holds nagg entries, out outlen >= n.  A row that touches more than 64 aggregates: *overflow = 1 and nothing else is
 * written (no pass 1, no apply), else *overflow = 0 */
int das_debug_coarse_az(int nagg, long long n, const long long* rowptr, const int* col, const double* vals, long long N, long long off, const int* agg, int* cnt,
                        long long* ptr, int* oa, double* ov, long long cap, long long* nnz, int* overflow, const double* u, const double* v, double* out,
                        long long outlen);
long long das_timer_count(das_solver_t* s, const char* name);
void das_timer_reset(das_solver_t* s);
void das_timer_enable(das_solver_t* s, int on);

#ifdef __cplusplus
}
#endif
#endif

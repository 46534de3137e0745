// Case parameters shared by the device driver and the host-emulation test harness.
#pragma once
#include "das_kernels.hpp"

namespace das {

struct RegSet;

struct CaseParams {
    int solver = DAS_SOLVER_SIMPLEFOAM;
    double nu = 1.5e-5, relax_U = 0.7, relax_nuTilda = 0.7, relax_T = 1.0, DT = 0.01, deltaT = 1.0;
    double Cp = 1005.0, molWeight = 28.96, mu = 1.8e-5, Pr = 0.7, Prt = 1.0;
    int mrf = 0, transonic = 0, transonicPC = 1, hasT = 0, sutherland = 0;
    int hasCyclic = 0;  // the mesh has coupled (cyclic) patch pairs
    double As = 1.4792e-06, Ts = 116.0;
    double om[3] = {0, 0, 0}, org[3] = {0, 0, 0};
    std::vector<double> phi_frozen, T_old;
    // `field` inputs (reference DAInputField.C): betaFINuTilda per cell; the pointers are what the kernels read (device memory
    // in the library, the host vector in the test harness), null = field absent (= 1) / no tangent
    std::vector<double> beta_fi;
    const double* betaFI_ptr = nullptr;
    const double* dBetaFI_ptr = nullptr;
    // regression models of DASimpleFoam (das_regression.hpp): the active models, null = none - then every code path is the one without
    // the option; regSeed: the dual pass of das_calc_dregressionpar_product (unit tangent on beta after the bounds)
    const RegSet* reg = nullptr;
    int regSeed = 0;
    // DAHeatTransferFoam: kappa(T) = sum_k kappa[k] T^k (constant/solidProperties kappa / kappaCoeffs)
    int nKappa = 0;
    double kappa[DAS_MAX_KAPPA_COEFFS] = {0, 0, 0, 0, 0, 0, 0, 0};
    // DASolidDisplacementFoam, constant/mechanicalProperties: rho, E, nu, planeStress and the Lame coefficients per unit density; the
    // pointer is what the traction kernel reads (device memory in the library, the host vector in the test harness)
    double solidRho = 1.0, solidE = 0.0, solidNu = 0.0, solidMu = 0.0, solidLambda = 0.0;
    int planeStress = 0, nTrac = 0;
    const int* tracCells_ptr = nullptr;
    // DAPimpleFoam: DASimpleFoam's layout, stencils and kernels with the fvm::ddt terms of body_cell and relax(1.0).  `solver` reads
    // DAS_SOLVER_SIMPLEFOAM with pimple = 1, so every path written for that layout serves it; what it cannot serve is refused by name.
    // ddtScheme: 0 Euler, 1 backward; timeIndex: the step the residual is evaluated at (backward below 2 is Euler); W0 / W00: what the
    // kernels read (device memory in the library, the host vectors in the test harness)
    int pimple = 0, ddtScheme = 0, timeIndex = 1;
    const double* W0_ptr = nullptr;
    const double* W00_ptr = nullptr;
    // the ddt coefficients (c, c0, c00) of the time index as it stands: backwardDdtScheme with deltaT0 = deltaT; below index 2 its deltaT0 is
    // GREAT and the three round to exactly 1, 1, 0
    void ddt_coeffs(double& c, double& c0, double& c00) const {
        const bool second = ddtScheme == 1 && timeIndex >= 2;
        c = second ? 1.5 : 1.0;
        c0 = second ? 2.0 : 1.0;
        c00 = second ? 0.5 : 0.0;
    }
    void from_case(const das_case_t* c) {
        solver = c->solver;
        if (solver == DAS_SOLVER_PIMPLEFOAM) {
            solver = DAS_SOLVER_SIMPLEFOAM;
            pimple = 1;
            DAS_CHECK(c->ddt_scheme == 0 || c->ddt_scheme == 1, DAS_ERR_ARG, "DAPimpleFoam: ddt_scheme is 0 (Euler) or 1 (backward), not " + std::to_string(c->ddt_scheme));
            DAS_CHECK(c->deltaT > 0.0, DAS_ERR_ARG, "DAPimpleFoam needs a positive deltaT, not " + std::to_string(c->deltaT));
            DAS_CHECK(!c->simple_has_T, DAS_ERR_ARG, "DAPimpleFoam: the T field is not built");
            DAS_CHECK(!c->mrf_active, DAS_ERR_ARG, "DAPimpleFoam: MRF is not built");
            for (int p = 0; p < c->n_patches; p++)
                DAS_CHECK(c->patch_type[p] != DAS_PATCH_CYCLIC, DAS_ERR_ARG, "DAPimpleFoam: cyclic patches are not built");
            ddtScheme = c->ddt_scheme;
        }
        if (solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM) {
            DAS_CHECK(c->solid_rho > 0.0, DAS_ERR_ARG, "DASolidDisplacementFoam needs a positive rho, not " + std::to_string(c->solid_rho));
            DAS_CHECK(c->solid_E > 0.0, DAS_ERR_ARG, "DASolidDisplacementFoam needs a positive E, not " + std::to_string(c->solid_E));
            DAS_CHECK(c->solid_nu > -1.0 && c->solid_nu < 0.5, DAS_ERR_ARG,
                      "DASolidDisplacementFoam needs nu inside (-1, 0.5), not " + std::to_string(c->solid_nu));
            solidRho = c->solid_rho; solidE = c->solid_E; solidNu = c->solid_nu; planeStress = c->plane_stress != 0;
            solid_lame(solidRho, solidE, solidNu, planeStress, solidMu, solidLambda);
        }
        if (solver == DAS_SOLVER_HEATTRANSFERFOAM) {
            DAS_CHECK(c->n_kappa_coeffs >= 1 && c->n_kappa_coeffs <= DAS_MAX_KAPPA_COEFFS, DAS_ERR_ARG,
                      "DAHeatTransferFoam needs kappa or kappaCoeffs with 1 to " + std::to_string(DAS_MAX_KAPPA_COEFFS) + " coefficients, not " +
                          std::to_string(c->n_kappa_coeffs));
            nKappa = c->n_kappa_coeffs;
            for (int k = 0; k < nKappa; k++) kappa[k] = c->kappa_coeffs[k];
        }
        nu = c->nu;
        relax_U = c->relax_U;
        relax_nuTilda = c->relax_nuTilda;
        relax_T = c->relax_T;
        DT = c->DT;
        deltaT = c->deltaT;
        if (solver != DAS_SOLVER_SCALARTRANSPORTFOAM) {
            mrf = c->mrf_active != 0;
            for (int k = 0; k < 3; k++) { om[k] = c->mrf_omega[k]; org[k] = c->mrf_origin[k]; }
            DAS_CHECK(!mrf || c->patch_mrf_rotating, DAS_ERR_ARG, "MRF needs the per-patch rotating flags");
        }
        for (int p = 0; p < c->n_patches; p++) hasCyclic = hasCyclic || c->patch_type[p] == DAS_PATCH_CYCLIC;
        hasT = (solver == DAS_SOLVER_SIMPLEFOAM) && c->simple_has_T != 0;
        if (hasT) {
            Pr = c->Pr; Prt = c->Prt;
            DAS_CHECK(Pr > 0 && Prt > 0, DAS_ERR_ARG, "DASimpleFoam with a T field needs positive Pr, Prt");
            DAS_CHECK(c->bc_T_code != nullptr, DAS_ERR_ARG, "DASimpleFoam with a T field needs the T patch table");
        }
        if (DAS_IS_COMPRESSIBLE(solver)) {
            transonic = (solver == DAS_SOLVER_TURBOFOAM) && c->transonic != 0;
            transonicPC = c->transonic_pc_option;
            Cp = c->Cp; molWeight = c->molWeight; mu = c->mu; Pr = c->Pr; Prt = c->Prt;
            DAS_CHECK(Cp > 0 && molWeight > 0 && mu > 0 && Pr > 0 && Prt > 0, DAS_ERR_ARG, "DARhoSimpleFoam/DATurboFoam need positive Cp, molWeight, mu, Pr, Prt");
            sutherland = c->transport_sutherland != 0;
            if (sutherland) {
                As = c->sutherland_As; Ts = c->sutherland_Ts;
                DAS_CHECK(As > 0 && Ts >= 0, DAS_ERR_ARG, "sutherland transport needs As > 0, Ts >= 0");
            }
        }
        if (c->beta_fi_nuTilda) beta_fi.assign(c->beta_fi_nuTilda, c->beta_fi_nuTilda + c->n_cells);
        if (c->phi_frozen) phi_frozen.assign(c->phi_frozen, c->phi_frozen + c->n_faces);
        if (c->T_old) T_old.assign(c->T_old, c->T_old + c->n_cells);
        if (solver == DAS_SOLVER_SCALARTRANSPORTFOAM)
            DAS_CHECK(!phi_frozen.empty() && !T_old.empty(), DAS_ERR_ARG, "DAScalarTransportFoam needs phi_frozen and T_old");
    }
};

inline ResParams make_params(const CaseParams& cp, const Options& opt, int isPC) {
    ResParams p;
    p.nu = cp.nu;
    p.alphaU = cp.pimple ? 1.0 : cp.relax_U;  // DAPimpleFoam: UEqn.relax(1.0), whatever fvSolution says
    p.alphaN = cp.relax_nuTilda;
    p.DT = cp.DT;
    p.deltaT = cp.deltaT;
    p.isPC = isPC;
    p.convBlend = isPC ? opt.getd("amd.pcUpwindBlend") : 1.0;
    p.constrainHbyA = (int)opt.geti("useConstrainHbyA");
    p.normU = opt.list_has("normalizeResiduals", "URes");
    p.normP = opt.list_has("normalizeResiduals", "pRes");
    p.normN = opt.list_has("normalizeResiduals", "nuTildaRes");
    p.normPhi = opt.list_has("normalizeResiduals", "phiRes");
    p.normT = opt.list_has("normalizeResiduals", "TRes");
    const bool rho = DAS_IS_COMPRESSIBLE(cp.solver) || cp.hasT;  // layouts with a T block
    p.offP = 3;
    p.offT = rho ? 4 : 0;
    p.offN = rho ? 5 : 4;
    p.offPhi = rho ? 6 : 5;
    p.hasT = cp.hasT;
    p.gradFaceParallel = (int)opt.geti_or("amd.gradFaceParallel", 1);
    // the face / cell split of the cell pass (body_fcoef + body_bcoef + body_cell2) serves DASimpleFoam + SA without T field, MRF and cyclic pairs
    p.cellFaceSplit = (int)opt.geti_or("amd.cellFaceSplit", 0) && cp.solver == DAS_SOLVER_SIMPLEFOAM && !cp.hasT && !cp.mrf && !cp.hasCyclic && !cp.reg && !cp.pimple;
    p.Cp = cp.Cp;
    p.Rgas = 8314.47 / cp.molWeight;  // Foam::constant::thermodynamic::RR / molWeight
    p.mu = cp.mu;
    p.Pr = cp.Pr;
    p.Prt = cp.Prt;
    p.sutherland = cp.sutherland;
    p.As = cp.As;
    p.Ts = cp.Ts;
    {
        const double Cv = p.Cp - p.Rgas;  // modified Eucken: alpha = mu Cv (1.32 + 1.77 R / Cv) / Cp
        p.alphaFac = cp.sutherland ? Cv * (1.32 + 1.77 * p.Rgas / Cv) / p.Cp : 1.0 / cp.Pr;
    }
    p.turbo = cp.solver == DAS_SOLVER_TURBOFOAM;
    p.transonic = cp.transonic;
    p.transonicPC = cp.transonicPC;
    p.mrf = cp.mrf;
    p.wTU = nullptr;
    p.betaFI = cp.betaFI_ptr;
    p.dBetaFI = cp.dBetaFI_ptr;
    p.betaReg = nullptr;  // set by the residual evaluation once k_reg_forward has written the array of the pass
    p.solid = cp.solver == DAS_SOLVER_HEATTRANSFERFOAM;
    p.nKappa = cp.nKappa;
    for (int k = 0; k < DAS_MAX_KAPPA_COEFFS; k++) p.kappa[k] = cp.kappa[k];
    p.sRho = cp.solidRho; p.sMu = cp.solidMu; p.sLam = cp.solidLambda;
    p.normD = opt.list_has("normalizeResiduals", "DRes");
    p.nPass = (int)opt.geti("maxCorrectBCCalls");  // read at residual time: the passes of the tractionDisplacement gradient
    p.nTrac = cp.nTrac;
    p.tracCells = cp.tracCells_ptr;
    for (int k = 0; k < 3; k++) { p.om[k] = cp.om[k]; p.org[k] = cp.org[k]; }
    p.ddt = cp.pimple;
    cp.ddt_coeffs(p.ddtC, p.ddtC0, p.ddtC00);
    p.W0 = cp.W0_ptr;
    p.W00 = cp.W00_ptr;
    return p;
}

inline DevMesh host_view(const Mesh& m) {
    DevMesh d;
    d.nC = m.nC; d.nF = m.nF; d.nIF = m.nIF;
    d.fg = m.fg.data(); d.cg = m.cg.data();
    d.cf_ptr = m.cf_ptr.data(); d.cf_face = m.cf_face.data(); d.cf_other = m.cf_other.data();
    d.owner = m.owner.data(); d.neigh = m.neighbour.data();
    d.bpatch = m.bface_patch.data(); d.bc = m.bc.data();
    d.mixed = m.mixed.empty() ? nullptr : m.mixed.data();
    d.cyc = m.cyc_face.data();
    return d;
}

}  // namespace das

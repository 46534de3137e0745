// TEST HARNESS ONLY (never linked into libdafoam_amd.so, never used by the product path).
// Runs the DAPimpleFoam residual bodies (body_grad, body_cell with the DDT flag, body_face, body_pres) and the hand-written old-time
// product body_drdwold (csrc/das_kernels.hpp) - the bodies the kernels k_cell<.., DDT> and k_drdwold wrap - in plain host loops, so that the
// CPU-only test tier can check them against the numpy restatement (tests/test_pimple_cpu.py).  A DASimpleFoam case runs body_cell with the
// flag off: the rows are then, bit for bit, those of tests/hostemu/hostemu.cpp.
#include "../../dafoam_amd/csrc/das_case.hpp"

using namespace das;

template <class T, class OLD = double>
static void eval(const DevMesh& m, const ResParams& prm, const T* W, T* R, std::vector<T>& rAU) {
    const long long N = m.nC;
    std::vector<T> nut(N), gU(9 * N), gP(3 * N), gN(3 * N), gH(3 * N), HbyA(3 * N), q(m.nF);
    rAU.assign(N, T(0.0));
    for (int k = 0; k < m.nC; k++) body_grad<T, false>(k, m, prm, W, nut.data(), gU.data(), gP.data(), gN.data(), gH.data());
    for (int k = 0; k < m.nC; k++) {  // DDT as eval_residual picks it: by prm.ddt
        if (prm.ddt) body_cell<T, false, double, false, true, OLD>(k, m, prm, W, nut.data(), gU.data(), gP.data(), gN.data(), gH.data(), R, rAU.data(), HbyA.data());
        else body_cell<T, false, double>(k, m, prm, W, nut.data(), gU.data(), gP.data(), gN.data(), gH.data(), R, rAU.data(), HbyA.data());
    }
    for (int f = 0; f < m.nF; f++) body_face<T, false>(f, m, prm, W, nut.data(), gP.data(), rAU.data(), HbyA.data(), q.data(), R);
    for (int k = 0; k < m.nC; k++) body_pres<T, false>(k, m, prm, q.data(), R);
}

static ResParams params_of(const das_case_t* c, CaseParams& cp, const double* W0, const double* W00, int timeIndex, int isPC, double pcBlend, int normalized) {
    cp.from_case(c);
    if (cp.solver != DAS_SOLVER_SIMPLEFOAM || cp.hasT) throw std::runtime_error("a DAPimpleFoam or DASimpleFoam case without a T field expected");
    cp.timeIndex = timeIndex;
    cp.W0_ptr = W0;
    cp.W00_ptr = W00;
    Options opt;
    opt.d["amd.pcUpwindBlend"] = pcBlend;
    if (!normalized) opt.s["normalizeResiduals"] = "TRes";
    return make_params(cp, opt, isPC);
}

// R(W; W0, W00) at the time index.  dW0 / dW00 (either may be null): tangents of the old states - one dual pass, its tangent part -> Rd
// (this pass exists here only: the library never differentiates with respect to the old states)
extern "C" int emu_pimple_residual(const das_case_t* c, const double* W, long long n, const double* W0, const double* W00, int timeIndex, int isPC,
                                   double pcBlend, int normalized, const double* dW0, const double* dW00, double* Rv, double* Rd) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        ResParams prm = params_of(c, cp, W0, W00, timeIndex, isPC, pcBlend, normalized);
        const DevMesh m = host_view(mesh);
        if (dW0 || dW00) {
            if (!prm.ddt) throw std::runtime_error("old-state tangents need a DAPimpleFoam case");
            // the old states as dual numbers behind the same pointers: body_cell<.., OLD = Dual<1>> is instantiated here and nowhere else
            std::vector<Dual<1>> Wd(n), W0d(n), W00d(n), R(n), rAU;
            for (long long i = 0; i < n; i++) {
                Wd[i] = Dual<1>(W[i]);
                W0d[i] = Dual<1>(W0[i]);
                W00d[i] = Dual<1>(W00 ? W00[i] : 0.0);
                if (dW0) W0d[i].d[0] = dW0[i];
                if (dW00) W00d[i].d[0] = dW00[i];
            }
            prm.W0 = (const double*)W0d.data();
            prm.W00 = (const double*)W00d.data();
            eval<Dual<1>, Dual<1>>(m, prm, Wd.data(), R.data(), rAU);
            for (long long i = 0; i < n; i++) { Rv[i] = R[i].v; Rd[i] = R[i].d[0]; }
        } else {
            std::vector<double> rAU;
            eval<double>(m, prm, W, Rv, rAU);
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_pimple_residual: %s\n", e.what());
        return -1;
    }
}

// out = scale o [dR/dW0]^T psi (level 1) or scale o [dR/dW00]^T psi (level 2) through body_drdwold, as das_calc_drdwold_t_psi launches it:
// rAU from one residual pass, zeros in the p and phi entries
extern "C" int emu_pimple_drdwold(const das_case_t* c, const double* W, long long n, const double* W0, const double* W00, int timeIndex, int level, int normalized,
                                  const double* scale, const double* psi, double* out) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        const ResParams prm = params_of(c, cp, W0, W00, timeIndex, 0, 0.0, normalized);
        if (!prm.ddt) throw std::runtime_error("a DAPimpleFoam case expected");
        const DevMesh m = host_view(mesh);
        std::vector<double> R(n), rAU;
        eval<double>(m, prm, W, R.data(), rAU);
        double cc, c0, c00;
        cp.ddt_coeffs(cc, c0, c00);
        const double coef = (level == 1 ? c0 : -c00) / cp.deltaT;
        for (long long i = 0; i < n; i++) out[i] = 0.0;
        if (coef == 0.0) return 0;
        for (int k = 0; k < m.nC; k++) body_drdwold(k, m, prm, coef, rAU.data(), psi, scale, out);
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_pimple_drdwold: %s\n", e.what());
        return -1;
    }
}

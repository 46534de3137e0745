// TEST HARNESS ONLY (never linked into libdafoam_amd.so, never used by the product path).
// Runs the face-function body that the HIP kernels k_fn_value / k_fn_tangent / k_fn_grad / k_fn_dual wrap (body_facefn,
// csrc/das_kernels.hpp) in a plain host loop, so that the CPU-only test tier can check it against the numpy restatement
// (tests/test_functions_more_cpu.py).
#include "../../dafoam_amd/csrc/das_case.hpp"

using namespace das;

template <class T, bool RHO>
static void facefn_on(const DevMesh& m, const ResParams& prm, const std::vector<T>& W, int kind, double gammaFn, double RFn, const double* loc,
                      const int* faces, int nf, T* q) {
    const long long N = m.nC;
    std::vector<T> nut(N), gU(9 * N), gP(3 * N), gN(3 * N), gH(3 * N), TU(3 * N);
    for (int c = 0; c < m.nC; c++) body_grad<T, RHO>(c, m, prm, W.data(), nut.data(), gU.data(), gP.data(), gN.data(), gH.data(), TU.data());
    const double dir[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < nf; k++) q[k] = body_facefn<T, RHO>(faces[k], m, prm, W.data(), nut.data(), gU.data(), kind, dir, gammaFn, RFn, loc);
}

// qv[k] = body_facefn<double>(faces[k]); with a state direction dW, or a tangent of the boundary value of T on one patch (bcPatch >= 0),
// also qd[k] = the tangent of body_facefn<Dual<1>>.  loc = axis (unit), center (location), may be null for the other kinds.
extern "C" int emu_facefn(const das_case_t* c, const double* Win, long long n, const double* dW, int bcPatch, double dTval, int kind, double gammaFn,
                          const double* loc, const int* faces, int nf, double* qv, double* qd) {
    try {
        Mesh mesh;
        mesh.build(c);
        CaseParams cp;
        cp.from_case(c);
        Options opt;
        const ResParams prm = make_params(cp, opt, 0);
        const bool rho = DAS_IS_COMPRESSIBLE(cp.solver);
        const double RFn = cp.Cp - cp.Cp / gammaFn;
        for (int k = 0; k < nf; k++)
            if (faces[k] < mesh.nIF || faces[k] >= mesh.nF) throw std::runtime_error("not a boundary face");
        std::vector<double> W(Win, Win + n);
        if (rho) facefn_on<double, true>(host_view(mesh), prm, W, kind, gammaFn, RFn, loc, faces, nf, qv);
        else facefn_on<double, false>(host_view(mesh), prm, W, kind, gammaFn, RFn, loc, faces, nf, qv);
        if (!dW && bcPatch < 0) return 0;
        if (bcPatch >= 0) mesh.bc[bcPatch].dT_val = dTval;
        std::vector<Dual<1>> Wd(n), q(nf);
        for (long long i = 0; i < n; i++) { Wd[i] = Dual<1>(Win[i]); Wd[i].d[0] = dW ? dW[i] : 0.0; }
        if (rho) facefn_on<Dual<1>, true>(host_view(mesh), prm, Wd, kind, gammaFn, RFn, loc, faces, nf, q.data());
        else facefn_on<Dual<1>, false>(host_view(mesh), prm, Wd, kind, gammaFn, RFn, loc, faces, nf, q.data());
        for (int k = 0; k < nf; k++) qd[k] = q[k].d[0];
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_facefn: %s\n", e.what());
        return -1;
    }
}

// TEST HARNESS ONLY (never linked into libdafoam_amd.so, never used by the product path).
// Runs the DAS_HD bodies of csrc/das_regression.hpp - the ones k_reg_forward and k_reg_backward wrap - in plain host loops, with double and
// with dual-number scalars, so that the CPU-only test tier can check them against the numpy restatement
// (tests/test_regression_model_cpu.py).  The work arrays the kernels keep in LDS columns are plain arrays here (stride 1).
// Built with -DEMU_REG_MAIN it is a stand-alone program that walks the parameter indexing of a [5, 3, 4] network and of the cap-sized
// models (for a run under -fsanitize=address,undefined).
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../dafoam_amd/csrc/das_case.hpp"
#include "../../dafoam_amd/csrc/das_regression.hpp"

using namespace das;

// ispec = {type, nIn, nLayers, nRBF, act, feat[8], width[6]}; dspec = {shift[8], scale[8], leaky, outShift, outScale, upper, lower, dflt}
static RegView view_of(const int* is, const double* ds, const double* par) {
    RegView v;
    memset(&v, 0, sizeof(v));
    v.type = is[0]; v.nIn = is[1]; v.nLayers = is[2]; v.nRBF = is[3]; v.act = is[4];
    if (v.nIn < 1 || v.nIn > DAS_REG_MAX_INPUTS || v.nLayers > DAS_REG_MAX_LAYERS || v.nRBF > DAS_REG_MAX_RBFS) throw std::runtime_error("model beyond the caps");
    for (int k = 0; k < DAS_REG_MAX_INPUTS; k++) { v.feat[k] = is[5 + k]; v.shift[k] = ds[k]; v.scale[k] = ds[8 + k]; }
    for (int l = 0; l < DAS_REG_MAX_LAYERS; l++) {
        v.width[l] = is[13 + l];
        if (l < v.nLayers && (v.width[l] < 1 || v.width[l] > DAS_REG_MAX_WIDTH)) throw std::runtime_error("layer beyond the caps");
    }
    v.leaky = ds[16]; v.outShift = ds[17]; v.outScale = ds[18]; v.upper = ds[19]; v.lower = ds[20]; v.dflt = ds[21];
    v.nPar = reg_n_parameters(v);
    v.par = par;
    return v;
}

extern "C" int emu_reg_n_parameters(const int* is, const double* ds) {
    try { return view_of(is, ds, nullptr).nPar; } catch (const std::exception& e) { fprintf(stderr, "emu_reg_n_parameters: %s\n", e.what()); return -1; }
}

// the features (N x nIn) of N cells from U (3 N), nuTilda (N), gradU (9 N), gradP (3 N) and y (N); with tangents (dU ... dgP, all or none)
// their forward tangents -> dfeat
extern "C" int emu_reg_features(const int* is, const double* ds, int N, double nu, const double* U, const double* nuT, const double* gU, const double* gP,
                                const double* y, const double* dU, const double* dN, const double* dgU, const double* dgP, double* feat, double* dfeat) {
    try {
        typedef Dual<1> D;
        const RegView v = view_of(is, ds, nullptr);
        ResParams prm{};
        prm.nu = nu;
        prm.offN = 4;  // [U | p | nuTilda]
        std::vector<CellGeom> cg(N);
        for (int c = 0; c < N; c++) cg[c].y = y[c];
        if (dU) {
            std::vector<D> W(5 * (size_t)N, D(0.0)), g(9 * (size_t)N), p(3 * (size_t)N);
            for (int i = 0; i < 3 * N; i++) { W[i].v = U[i]; W[i].d[0] = dU[i]; p[i].v = gP[i]; p[i].d[0] = dgP[i]; }
            for (int i = 0; i < N; i++) { W[4 * (size_t)N + i].v = nuT[i]; W[4 * (size_t)N + i].d[0] = dN[i]; }
            for (int i = 0; i < 9 * N; i++) { g[i].v = gU[i]; g[i].d[0] = dgU[i]; }
            D f[DAS_REG_MAX_INPUTS];
            for (int c = 0; c < N; c++) {
                reg_features<D, double>(v, c, N, prm, cg.data(), W.data(), g.data(), p.data(), f, 1);
                for (int k = 0; k < v.nIn; k++) { feat[(size_t)c * v.nIn + k] = f[k].v; dfeat[(size_t)c * v.nIn + k] = f[k].d[0]; }
            }
        } else {
            std::vector<double> W(5 * (size_t)N, 0.0);
            for (int i = 0; i < 3 * N; i++) W[i] = U[i];
            for (int i = 0; i < N; i++) W[4 * (size_t)N + i] = nuT[i];
            for (int c = 0; c < N; c++) reg_features<double, double>(v, c, N, prm, cg.data(), W.data(), gU, gP, feat + (size_t)c * v.nIn, 1);
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_reg_features: %s\n", e.what());
        return -1;
    }
}

// beta and the mask of N cells from their features, as k_reg_forward does it.  dfeat (N x nIn, may be null): forward tangents of the
// features -> dbeta.  seed: the tangent is set after the bounds instead, 1 on the cells that kept their value.
extern "C" int emu_reg_forward(const int* is, const double* ds, const double* par, int N, const double* feat, const double* dfeat, int seed, double* beta,
                               double* dbeta, unsigned char* mask) {
    try {
        typedef Dual<1> D;
        const RegView v = view_of(is, ds, par);
        const int rows = reg_forward_rows(v);
        if (dbeta) {
            std::vector<D> a0(rows), a1(rows);
            for (int c = 0; c < N; c++) {
                for (int k = 0; k < v.nIn; k++) { a0[k].v = feat[(size_t)c * v.nIn + k]; a0[k].d[0] = dfeat ? dfeat[(size_t)c * v.nIn + k] : 0.0; }
                int m;
                D b = reg_check_output<D>(v, reg_eval<D>(v, par, a0.data(), a1.data(), 1), m);
                if (seed) b = MkSeed<D>::make(val(b), m ? 0.0 : 1.0);
                beta[c] = b.v; dbeta[c] = b.d[0]; mask[c] = (unsigned char)m;
            }
        } else {
            std::vector<double> a0(rows), a1(rows);
            for (int c = 0; c < N; c++) {
                for (int k = 0; k < v.nIn; k++) a0[k] = feat[(size_t)c * v.nIn + k];
                int m;
                beta[c] = reg_check_output<double>(v, reg_eval<double>(v, par, a0.data(), a1.data(), 1), m);
                mask[c] = (unsigned char)m;
            }
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_reg_forward: %s\n", e.what());
        return -1;
    }
}

// out[k] = sum_c g[c] d beta_c / d par_k (no bounds: the caller zeroes g where it wants a cell masked), the cells in their order
extern "C" int emu_reg_backward(const int* is, const double* ds, const double* par, int N, const double* feat, const double* g, double* out) {
    try {
        const RegView v = view_of(is, ds, par);
        std::vector<double> act(reg_act_rows(v)), dlt(reg_delta_rows(v));
        for (int k = 0; k < v.nPar; k++) out[k] = 0.0;
        for (int c = 0; c < N; c++) {
            for (int k = 0; k < v.nIn; k++) act[k] = feat[(size_t)c * v.nIn + k];
            reg_backprop(v, par, g[c] * v.outScale, act.data(), dlt.data(), 1);
            for (int k = 0; k < v.nPar; k++) out[k] += reg_param_term(reg_param_rows(v, par, k), act.data(), dlt.data(), 0, 1);
        }
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "emu_reg_backward: %s\n", e.what());
        return -1;
    }
}

#ifdef EMU_REG_MAIN
// every parameter of the model decoded and used once, forward and backward, on a few cells: an index beyond an array shows under the
// address sanitiser.  The arrays have exactly the sizes the helpers report.
static int walk(const char* what, int type, int nIn, int nLayers, const int* widths, int nRBF, int act) {
    int is[19] = {type, nIn, nLayers, nRBF, act};
    double ds[22];
    for (int k = 0; k < 8; k++) { is[5 + k] = k % 7; ds[k] = 0.1 * k; ds[8 + k] = 1.0 + 0.05 * k; }
    for (int l = 0; l < 6; l++) is[13 + l] = l < nLayers ? widths[l] : 0;
    ds[16] = 0.1; ds[17] = 0.2; ds[18] = 1.5; ds[19] = 1e30; ds[20] = -1e30; ds[21] = 1.0;
    const int nPar = emu_reg_n_parameters(is, ds);
    if (nPar < 1) return 1;
    std::vector<double> par(nPar), out(nPar);
    for (int k = 0; k < nPar; k++) par[k] = 0.3 + 0.01 * ((k * 7919) % 101);
    const int N = 5;
    std::vector<double> feat((size_t)N * nIn), g(N), beta(N);
    std::vector<unsigned char> mask(N);
    for (size_t i = 0; i < feat.size(); i++) feat[i] = 0.05 * (double)(i % 13) - 0.2;
    for (int c = 0; c < N; c++) g[c] = 1.0 + c;
    if (emu_reg_forward(is, ds, par.data(), N, feat.data(), nullptr, 0, beta.data(), nullptr, mask.data())) return 1;
    if (emu_reg_backward(is, ds, par.data(), N, feat.data(), g.data(), out.data())) return 1;
    double s = 0.0;
    for (int k = 0; k < nPar; k++) s += out[k];
    printf("%s: %d parameters, beta[0] = %.15g, sum of the gradient = %.15g\n", what, nPar, beta[0], s);
    return !(s == s);
}
int main() {
    const int a[3] = {5, 3, 4}, b[6] = {32, 32, 32, 32, 0, 0}, c[6] = {8, 8, 8, 8, 8, 8};
    int bad = 0;
    bad |= walk("[5, 3, 4] tanh, 3 inputs", DAS_REG_NN, 3, 3, a, 0, DAS_REG_TANH);
    bad |= walk("[32, 32, 32, 32] relu, 8 inputs", DAS_REG_NN, DAS_REG_MAX_INPUTS, 4, b, 0, DAS_REG_RELU);
    bad |= walk("six layers of 8 sigmoid, 1 input", DAS_REG_NN, 1, DAS_REG_MAX_LAYERS, c, 0, DAS_REG_SIGMOID);
    bad |= walk("64 RBFs, 8 inputs", DAS_REG_RBF, DAS_REG_MAX_INPUTS, 0, c, DAS_REG_MAX_RBFS, 0);
    return bad;
}
#endif

// Regression models of DASimpleFoam (the regressionModel option and the regressionPar input; reference DARegression.C:164-773,
// DASpalartAllmaras.C:601-622, DAInputRegressionPar.C): a small neural network or a sum of radial basis functions, evaluated in every
// cell from local flow features, writes betaFINuTilda as part of every residual evaluation.
//   features   (f + inputShift) * inputScale of VoS, PoD, chiSA, pGradStream, PSoSS, SCurv, UOrth (reg_feature), from the states and from the
//              gradient arrays of the gradient launch; gU[3 i + j] = d_i U_j is OpenFOAM's gradU[i][j]
//   model      reg_eval: the parameter order, the activations and the output handling of DARegression::compute
//   bounds     reg_check_output: DARegression::checkOutput - NaN / Inf -> defaultOutputValue, values beyond the bounds clipped; a replaced
//              or clipped cell carries a zero tangent (the assignment of a constant)
//   backward   out[k] = sum_c g[c] d beta_c / d theta_k (reg_backprop + reg_param_term): the hand-written reverse pass
// The bodies are DAS_HD and take their per-cell work arrays with a stride: LDS columns on the device ([row][thread]: neighbouring threads
// on neighbouring banks), plain arrays in the host harness (tests/hostemu/hostemu_regression.cpp).
// A mag() of an exactly zero vector or tensor is dsqrt(0) of das_dual.hpp: the value 0 with a ZERO tangent (the derivative of the square
// root at 0 is taken as 0, not as infinity), like every other dsqrt of the library.
#pragma once
#include "das_kernels.hpp"

namespace das {

// caps, checked when a model is defined (das_define_regression_model); they size the LDS of the kernels below
#define DAS_REG_MAX_INPUTS 8
#define DAS_REG_MAX_LAYERS 6
#define DAS_REG_MAX_WIDTH 32
#define DAS_REG_MAX_RBFS 64
#define DAS_REG_MAX_PARAMS 4096
#define DAS_REG_MAX_MODELS 4

enum { DAS_REG_NN = 0, DAS_REG_RBF = 1 };
enum { DAS_REG_SIGMOID = 0, DAS_REG_TANH = 1, DAS_REG_RELU = 2 };
enum { DAS_REG_VOS = 0, DAS_REG_POD, DAS_REG_CHISA, DAS_REG_PGRADSTREAM, DAS_REG_PSOSS, DAS_REG_SCURV, DAS_REG_UORTH };
enum { DAS_REG_NAN = 1, DAS_REG_INF = 2, DAS_REG_BOUNDED = 4 };  // bits of the per-cell mask of reg_check_output

struct RegView {
    int type, nIn, nLayers, nRBF, act, nPar;
    int feat[DAS_REG_MAX_INPUTS];
    double shift[DAS_REG_MAX_INPUTS], scale[DAS_REG_MAX_INPUTS];
    int width[DAS_REG_MAX_LAYERS];
    double leaky, outShift, outScale, upper, lower, dflt;
    const double* par;  // nPar values (device memory in the library)
};
// the active models in the order of the option dictionary: the last one to write betaFINuTilda wins
struct RegSet {
    int n = 0;
    RegView v[DAS_REG_MAX_MODELS];
};

DAS_HD int reg_n_parameters(const RegView& v) {  // DARegression::nParameters, DARegression.C:664-699
    if (v.type == DAS_REG_RBF) return v.nRBF * (2 * v.nIn + 1);
    int n = v.nIn * v.width[0];
    for (int l = 1; l < v.nLayers; l++) n += v.width[l] * v.width[l - 1];
    n += v.width[v.nLayers - 1];
    for (int l = 0; l < v.nLayers; l++) n += v.width[l];
    return n + 1;
}
DAS_HD int reg_hidden_total(const RegView& v) {
    int h = 0;
    for (int l = 0; l < v.nLayers; l++) h += v.width[l];
    return h;
}
// rows of one activation buffer of the forward pass / of the two arrays of the backward pass
DAS_HD int reg_forward_rows(const RegView& v) {
    int a = v.nIn;
    if (v.type == DAS_REG_NN)
        for (int l = 0; l < v.nLayers; l++) a = v.width[l] > a ? v.width[l] : a;
    return a;
}
DAS_HD int reg_act_rows(const RegView& v) { return v.nIn + (v.type == DAS_REG_NN ? reg_hidden_total(v) : 0); }
DAS_HD int reg_delta_rows(const RegView& v) { return v.type == DAS_REG_NN ? reg_hidden_total(v) + 1 : v.nRBF; }

template <class T>
DAS_HD T reg_mag3(const T* a) { return dsqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// one input feature of one cell, before shift and scale (DARegression.C:182-285)
template <class T, class G>
DAS_HD T reg_feature(int id, const T* U, const T& nc, double nu, const T* g, const T* gP, const G& y) {
    if (id == DAS_REG_VOS) {  // mag(skew(gradU)) / (mag(symm(gradU)) + mag(skew(gradU)) + 1e-16)
        T so(0.0), ss(0.0);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const T a = 0.5 * (g[3 * i + j] - g[3 * j + i]), s = 0.5 * (g[3 * i + j] + g[3 * j + i]);
                so += a * a;
                ss += s * s;
            }
        const T mo = dsqrt(so), ms = dsqrt(ss);
        return mo / (ms + mo + 1e-16);
    }
    if (id == DAS_REG_POD) {  // P / (D + P + 1e-16) of the SA model (getTurbProdOverDestruct), with the functions of body_cell
        T Stilda, fw;
        sa_stilda_fw<T, G>(nc, T(nu), g, y, Stilda, fw);
        const T P = SA_CB1 * Stilda * nc;
        const T q = nc / y;
        const T D = SA_CW1 * fw * (q * q);
        return P / (D + P + 1e-16);
    }
    if (id == DAS_REG_CHISA) return nc / (nu + nc + 1e-16);
    if (id == DAS_REG_PGRADSTREAM) {  // (U & gradP) / (mag(U) mag(gradP) + mag(U & gradP) + 1e-16)
        const T d = U[0] * gP[0] + U[1] * gP[1] + U[2] * gP[2];
        return d / (reg_mag3<T>(U) * reg_mag3<T>(gP) + dabs(d) + 1e-16);
    }
    if (id == DAS_REG_PSOSS) {  // mag(gradP) / (mag(gradP) + mag(3 cmptAv(U & diag(gradU))) + 1e-16); cmptAv of a scalar is the identity
        const T mp = reg_mag3<T>(gP);
        const T s = U[0] * g[0] + U[1] * g[4] + U[2] * g[8];
        return mp / (mp + dabs(3.0 * s) + 1e-16);
    }
    T a[3], b[3];  // a = U & gradU, b = gradU & U
#pragma unroll
    for (int j = 0; j < 3; j++) {
        a[j] = U[0] * g[j] + U[1] * g[3 + j] + U[2] * g[6 + j];
        b[j] = g[3 * j] * U[0] + g[3 * j + 1] * U[1] + g[3 * j + 2] * U[2];
    }
    if (id == DAS_REG_SCURV) {  // mag(U & gradU) / (mag(U & U) + mag(U & gradU) + 1e-16)
        const T ma = reg_mag3<T>(a);
        return ma / (dabs(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]) + ma + 1e-16);
    }
    // UOrth: mag(U & gradU & U) / (mag(U) mag(gradU & U) + mag(U & gradU & U) + 1e-16)
    const T s = dabs(a[0] * U[0] + a[1] * U[1] + a[2] * U[2]);
    return s / (reg_mag3<T>(U) * reg_mag3<T>(b) + s + 1e-16);
}

// the features of cell c into f[k * stride], shifted and scaled
template <class T, class G>
DAS_HD void reg_features(const RegView& v, int c, long long N, const ResParams& prm, const CellGeomT<G>* cg, const T* W, const T* gU, const T* gP, T* f,
                         int stride) {
    const T U[3] = {W[3LL * c], W[3LL * c + 1], W[3LL * c + 2]};
    const T nc = W[prm.offN * N + c];
    T g[9], p[3];
#pragma unroll
    for (int k = 0; k < 9; k++) g[k] = gU[9LL * c + k];
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = gP[3LL * c + k];
    for (int k = 0; k < v.nIn; k++) f[k * stride] = (reg_feature<T, G>(v.feat[k], U, nc, prm.nu, g, p, cg[c].y) + v.shift[k]) * v.scale[k];
}

template <class T>
DAS_HD T reg_activation(const RegView& v, const T& z) {
    if (v.act == DAS_REG_SIGMOID) return 1.0 / (1.0 + dexp(-z));
    if (v.act == DAS_REG_TANH) {
        const T e = dexp(-2.0 * z);
        return (1.0 - e) / (1.0 + e);
    }
    return val(z) < 0.0 ? v.leaky * z : z;
}

// outputScale (out + outputShift) of one cell.  a0 holds the features on entry; a0 / a1 (reg_forward_rows entries each) take the layers
// in turn.  The parameters run as in DARegression::compute: per neuron its weights, then its bias; the output neuron last.
template <class T>
DAS_HD T reg_eval(const RegView& v, const double* par, T* a0, T* a1, int stride) {
    T out(0.0);
    if (v.type == DAS_REG_NN) {
        T *in = a0, *nx = a1;
        int k = 0, nPrev = v.nIn;
        for (int l = 0; l < v.nLayers; l++) {
            for (int i = 0; i < v.width[l]; i++) {
                T z(0.0);
                for (int j = 0; j < nPrev; j++) z += in[j * stride] * par[k++];
                z += par[k++];
                nx[i * stride] = reg_activation<T>(v, z);
            }
            T* t = in; in = nx; nx = t;
            nPrev = v.width[l];
        }
        for (int j = 0; j < nPrev; j++) out += in[j * stride] * par[k++];
        out += par[k];
    } else {
        const int dP = 2 * v.nIn + 1;
        for (int i = 0; i < v.nRBF; i++) {
            T e(0.0);
            for (int j = 0; j < v.nIn; j++) {
                const T d = a0[j * stride] - par[dP * i + 2 * j];
                e += (d * d) / (2.0 * par[dP * i + 2 * j + 1] * par[dP * i + 2 * j + 1]);
            }
            out += par[dP * i + dP - 1] * dexp(-e);
        }
    }
    return v.outScale * (out + v.outShift);
}

// DARegression::checkOutput on one cell, in its order; mask: which of the three conditions were met.  A replaced or clipped value is a
// constant: no tangent.
template <class T>
DAS_HD T reg_check_output(const RegView& v, T b, int& mask) {
    mask = 0;
    if (!(val(b) == val(b))) { b = T(v.dflt); mask |= DAS_REG_NAN; }
    if (val(b) - val(b) != 0.0 && val(b) == val(b)) { b = T(v.dflt); mask |= DAS_REG_INF; }
    if (val(b) > v.upper) { b = T(v.upper); mask |= DAS_REG_BOUNDED; }
    if (val(b) < v.lower) { b = T(v.lower); mask |= DAS_REG_BOUNDED; }
    return b;
}

// ---- the reverse pass of one cell.  act: reg_act_rows rows (the features, then for a network the outputs of every hidden layer);
// dlt: reg_delta_rows rows - a network: gOut d out / d z of every hidden neuron (z: its sum before the activation), then gOut itself for
// the output neuron; radial basis functions: gOut e_i.  gOut = g outputScale.  The features are in act on entry.
DAS_HD void reg_backprop(const RegView& v, const double* par, double gOut, double* act, double* dlt, int stride) {
    if (gOut == 0.0) {
        // a cell that contributes nothing - its output was replaced (NaN, Inf) or clipped, so the tape holds a constant and g is zero - is
        // not evaluated at all: its features may be NaN or Inf, and 0 x NaN would poison the sums of every parameter.  Zero rows instead.
        const int na = reg_act_rows(v), nd = reg_delta_rows(v);
        for (int k = 0; k < na; k++) act[k * stride] = 0.0;
        for (int k = 0; k < nd; k++) dlt[k * stride] = 0.0;
        return;
    }
    if (v.type == DAS_REG_RBF) {
        const int dP = 2 * v.nIn + 1;
        for (int i = 0; i < v.nRBF; i++) {
            double e = 0.0;
            for (int j = 0; j < v.nIn; j++) {
                const double d = act[j * stride] - par[dP * i + 2 * j];
                e += (d * d) / (2.0 * par[dP * i + 2 * j + 1] * par[dP * i + 2 * j + 1]);
            }
            dlt[i * stride] = gOut * exp(-e);
        }
        return;
    }
    // forward: the activations of every layer are kept; dlt takes the derivative of the activation meanwhile
    int k = 0, nPrev = v.nIn, inRow = 0, outRow = v.nIn, dRow = 0;
    for (int l = 0; l < v.nLayers; l++) {
        for (int i = 0; i < v.width[l]; i++) {
            double z = 0.0;
            for (int j = 0; j < nPrev; j++) z += act[(inRow + j) * stride] * par[k++];
            z += par[k++];
            double a, da;
            if (v.act == DAS_REG_SIGMOID) { a = 1.0 / (1.0 + exp(-z)); da = a * (1.0 - a); }
            else if (v.act == DAS_REG_TANH) { const double e = exp(-2.0 * z); a = (1.0 - e) / (1.0 + e); da = 4.0 * e / ((1.0 + e) * (1.0 + e)); }
            else { a = z < 0.0 ? v.leaky * z : z; da = z < 0.0 ? v.leaky : 1.0; }
            act[(outRow + i) * stride] = a;
            dlt[(dRow + i) * stride] = da;
        }
        inRow = outRow;
        outRow += v.width[l];
        dRow += v.width[l];
        nPrev = v.width[l];
    }
    // k: the first parameter of the output neuron; dRow: its row
    dlt[dRow * stride] = gOut;
    int nNext = 1, nextRow = dRow, nextPar = k;
    for (int l = v.nLayers - 1; l >= 0; l--) {
        const int w = v.width[l], row = nextRow - w;
        for (int i = 0; i < w; i++) {
            double s = 0.0;
            for (int n = 0; n < nNext; n++) s += dlt[(nextRow + n) * stride] * par[nextPar + n * (w + 1) + i];
            dlt[(row + i) * stride] *= s;
        }
        nNext = w;
        nextRow = row;
        nextPar -= w * ((l > 0 ? v.width[l - 1] : v.nIn) + 1);
    }
}

// parameter k decoded once: its term of a cell is  dlt[drow] x (kind 0: 1 | kind 1: act[arow] | kind 2: c0 (act[arow] - c1) | kind 3: c0 (act[arow] - c1)^2)
struct RegParamRows {
    int kind, arow, drow;
    double c0, c1;
};
DAS_HD RegParamRows reg_param_rows(const RegView& v, const double* par, int k) {
    RegParamRows r;
    r.c0 = 0.0; r.c1 = 0.0; r.arow = 0;
    if (v.type == DAS_REG_RBF) {
        const int dP = 2 * v.nIn + 1, i = k / dP, q = k - i * dP;
        r.drow = i;
        if (q == dP - 1) { r.kind = 0; return r; }
        const int j = q >> 1;
        const double m = par[dP * i + 2 * j], s = par[dP * i + 2 * j + 1], w = par[dP * i + dP - 1];
        r.arow = j;
        r.c1 = m;
        if (q & 1) { r.kind = 3; r.c0 = w / (s * s * s); }
        else { r.kind = 2; r.c0 = w / (s * s); }
        return r;
    }
    int p0 = 0, nPrev = v.nIn, inRow = 0, dRow = 0;
    for (int l = 0; l <= v.nLayers; l++) {
        const int w = l < v.nLayers ? v.width[l] : 1;
        const int cnt = w * (nPrev + 1);
        if (k < p0 + cnt || l == v.nLayers) {
            const int q = k - p0, i = q / (nPrev + 1), j = q - i * (nPrev + 1);
            r.drow = dRow + i;
            r.kind = j < nPrev ? 1 : 0;
            r.arow = inRow + (j < nPrev ? j : 0);
            return r;
        }
        p0 += cnt;
        inRow += nPrev;
        dRow += w;
        nPrev = w;
    }
    return r;
}
DAS_HD double reg_param_term(const RegParamRows& r, const double* act, const double* dlt, int cl, int stride) {
    const double d = dlt[r.drow * stride + cl];
    if (r.kind == 0) return d;
    const double a = act[r.arow * stride + cl];
    if (r.kind == 1) return d * a;
    const double x = a - r.c1;
    return r.kind == 2 ? d * (r.c0 * x) : d * (r.c0 * (x * x));
}

}  // namespace das

#ifdef __HIPCC__
#include "das_heatsource.hpp"

namespace das {

#define DAS_REG_FWD_THREADS 64  // one wave per workgroup: 2 x reg_forward_rows LDS columns per thread
#define DAS_REG_BWD_TILE 64     // cells per tile of the backward kernel
#define DAS_REG_BWD_THREADS 256
#define DAS_REG_BWD_MAX_BLOCKS 128
#define DAS_REG_MAX_LDS (160 * 1024)  // LDS of a gfx950 compute unit: the most one workgroup can have; checked when a model is defined

template <class T>
inline size_t reg_forward_lds(const RegView& v) { return (size_t)v.nPar * sizeof(double) + 2 * (size_t)reg_forward_rows(v) * DAS_REG_FWD_THREADS * sizeof(T); }
inline size_t reg_backward_lds(const RegView& v) { return (size_t)(reg_act_rows(v) + reg_delta_rows(v)) * DAS_REG_BWD_TILE * sizeof(double); }

// beta[c] of one model.  The parameters are staged in LDS once per workgroup (uniform reads afterwards: broadcasts); the activations of a
// thread are two LDS columns, [row][thread].  featIn != null: the features (nC x nIn, shifted and scaled) are read from it and neither
// the mesh nor the states are touched (das_debug_reg_forward).  seed (dual passes only): the tangent of beta is set AFTER the bounds,
// 1 on the cells that kept their value and 0 on the replaced and clipped ones (das_calc_dregressionpar_product).  featOut (nC x nIn)
// and maskOut (nC) are optional.
template <class T, class G>
__global__ __launch_bounds__(DAS_REG_FWD_THREADS) void k_reg_forward(RegView v, int nC, const CellGeomT<G>* __restrict__ cg, ResParams prm, const T* __restrict__ W,
                                                                      const T* __restrict__ gU, const T* __restrict__ gP, const double* __restrict__ featIn,
                                                                      int seed, T* __restrict__ beta, double* __restrict__ featOut,
                                                                      unsigned char* __restrict__ maskOut) {
    extern __shared__ double reg_sh[];
    double* const par = reg_sh;
    const int rows = reg_forward_rows(v);
    T* const a0 = reinterpret_cast<T*>(reg_sh + v.nPar) + threadIdx.x;
    T* const a1 = a0 + rows * DAS_REG_FWD_THREADS;
    for (int k = threadIdx.x; k < v.nPar; k += DAS_REG_FWD_THREADS) par[k] = v.par[k];
    __syncthreads();
    const int c = blockIdx.x * DAS_REG_FWD_THREADS + threadIdx.x;
    if (c >= nC) return;
    if (featIn)
        for (int k = 0; k < v.nIn; k++) a0[k * DAS_REG_FWD_THREADS] = T(featIn[(long long)c * v.nIn + k]);
    else
        reg_features<T, G>(v, c, nC, prm, cg, W, gU, gP, a0, DAS_REG_FWD_THREADS);
    if (featOut)
        for (int k = 0; k < v.nIn; k++) featOut[(long long)c * v.nIn + k] = val(a0[k * DAS_REG_FWD_THREADS]);
    int mask;
    T b = reg_check_output<T>(v, reg_eval<T>(v, par, a0, a1, DAS_REG_FWD_THREADS), mask);
    if (seed) b = MkSeed<T>::make(val(b), mask ? 0.0 : 1.0);
    beta[c] = b;
    if (maskOut) maskOut[c] = (unsigned char)mask;
}

// the three fail counts, stage 1: part[3 b + q] = cells of block b (grid-stride) with bit q of the mask set; k_reg_count_final adds them
__global__ __launch_bounds__(256) void k_reg_count(int nC, const unsigned char* __restrict__ mask, double* __restrict__ part) {
    double cnt[3] = {0.0, 0.0, 0.0};
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nC; c += gridDim.x * blockDim.x) {
        const int m = mask[c];
#pragma unroll
        for (int q = 0; q < 3; q++) cnt[q] += (m >> q) & 1;
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
        if (q) __syncthreads();  // the LDS slots of the sum before are read before the next one writes them
        const double t = hs_block_sum<double>(cnt[q]);
        if (threadIdx.x == 0) part[3 * blockIdx.x + q] = t;
    }
}
__global__ __launch_bounds__(256) void k_reg_count_final(int nb, const double* __restrict__ part, double* __restrict__ out3) {
    double cnt[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nb; i += 256)
#pragma unroll
        for (int q = 0; q < 3; q++) cnt[q] += part[3 * i + q];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        if (q) __syncthreads();
        const double t = hs_block_sum<double>(cnt[q]);
        if (threadIdx.x == 0) out3[q] = t;
    }
}

// part[b nPar + k] = sum over the cells of the tiles of workgroup b of g[c] d beta_c / d theta_k.  Per tile: the first DAS_REG_BWD_TILE
// threads run the reverse pass of one cell each and leave the layer inputs and the deltas in LDS ([row][cell]); then every thread owns
// the parameters k = tid, tid + 256, ... and walks the cells of the tile in their order.  The tiles of a workgroup are fixed by the grid,
// the grid by nC: the same bits on every call.  No per-cell gradient array exists anywhere.
__global__ __launch_bounds__(DAS_REG_BWD_THREADS) void k_reg_backward(RegView v, int nC, const CellGeom* __restrict__ cg, ResParams prm, const double* __restrict__ W,
                                                                       const double* __restrict__ gU, const double* __restrict__ gP,
                                                                       const double* __restrict__ featIn, const double* __restrict__ g,
                                                                       double* __restrict__ part) {
    extern __shared__ double reg_sh[];
    constexpr int TC = DAS_REG_BWD_TILE, NQ = DAS_REG_MAX_PARAMS / DAS_REG_BWD_THREADS;
    double* const act = reg_sh;
    double* const dlt = reg_sh + reg_act_rows(v) * TC;
    double acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[q] = 0.0;
    const int nTiles = (nC + TC - 1) / TC;
    for (int t = blockIdx.x; t < nTiles; t += gridDim.x) {
        const int c0 = t * TC, nT = min(TC, nC - c0);
        if ((int)threadIdx.x < nT) {
            const int c = c0 + threadIdx.x;
            if (featIn)
                for (int k = 0; k < v.nIn; k++) act[k * TC + threadIdx.x] = featIn[(long long)c * v.nIn + k];
            else
                reg_features<double, double>(v, c, nC, prm, cg, W, gU, gP, act + threadIdx.x, TC);
            reg_backprop(v, v.par, g[c] * v.outScale, act + threadIdx.x, dlt + threadIdx.x, TC);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NQ; q++) {
            const int k = threadIdx.x + q * DAS_REG_BWD_THREADS;
            if (k < v.nPar) {
                const RegParamRows r = reg_param_rows(v, v.par, k);
                double a = acc[q];
                for (int cl = 0; cl < nT; cl++) a += reg_param_term(r, act, dlt, cl, TC);
                acc[q] = a;
            }
        }
        __syncthreads();  // the tile is read before the next one overwrites it
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const int k = threadIdx.x + q * DAS_REG_BWD_THREADS;
        if (k < v.nPar) part[(long long)blockIdx.x * v.nPar + k] = acc[q];
    }
}
// out[k] = the partials of the nb workgroups in their order
__global__ __launch_bounds__(256) void k_reg_backward_final(int nb, int nPar, const double* __restrict__ part, double* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nPar) return;
    double acc = 0.0;
    for (int b = 0; b < nb; b++) acc += part[(long long)b * nPar + k];
    out[k] = acc;
}

}  // namespace das
#endif

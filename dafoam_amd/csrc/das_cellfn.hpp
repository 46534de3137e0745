// Cell-set objectives (reference DAFunctionVariableVolSum.C, DAFunctionVariance.C mode "field"): F = coef * sum_t w_t g(x_t) over
// the terms t of a fixed cell set, one term per (cell, component):
//   x_t = src[idx_t] - d_t      src = the states (or the betaFINuTilda field), d_t = reference data (variance; 0 otherwise)
//   g   = x^2 (isSquare / variance) or x
//   w_t = V_cell (multiplyVol / useGeoWeight) or 1
// coef = scale / (totalVol | sum of weights | number of terms) is set by the host from the current metrics.
#pragma once
#include "das_common.hpp"
#include "das_dual.hpp"
#include "das_kernels.hpp"

namespace das {

#define DAS_CELLFN_MAX_BLOCKS 1024

struct CellFnView {
    long long nt;
    const int* cell;        // nt: the cell of each term
    const long long* idx;   // nt: index of the term's value in src
    const double* data;     // nt: reference values, may be null
    int square, mv;
};

DAS_HD inline double cellfn_x(const CellFnView& f, const double* src, long long t) { return src[f.idx[t]] - (f.data ? f.data[t] : 0.0); }

// value, stage 1: per-workgroup partial sums (grid-stride loop over the terms, wave64 shuffles, 4 waves through LDS); the grid size
// depends on nt only, so the partials - and the final sum - are the same bits on every call
__global__ __launch_bounds__(256) void k_cellfn_value(CellFnView f, const CellGeom* __restrict__ cg, const double* __restrict__ src, double* __restrict__ part) {
    double acc = 0.0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < f.nt; t += (long long)gridDim.x * blockDim.x) {
        const double x = cellfn_x(f, src, t);
        acc += (f.mv ? cg[f.cell[t]].V : 1.0) * (f.square ? x * x : x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// value, stage 2: ONE workgroup adds the nb partials in a fixed order; out[0] = coef * sum
__global__ __launch_bounds__(256) void k_cellfn_sum(int nb, const double* __restrict__ part, double coef, double* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = coef * ((sh[0] + sh[1]) + (sh[2] + sh[3]));
}
// gradient: out[idx_t] = g * w_t * dg/dx * sc[idx_t]   (g = seed x coef x outer derivative; sc = state scales or null).  The terms
// of one function address distinct entries, so the stores do not collide; the caller zeroes out first.
__global__ __launch_bounds__(256) void k_cellfn_grad(CellFnView f, const CellGeom* __restrict__ cg, const double* __restrict__ src, const double* __restrict__ sc,
                                                     double g, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= f.nt) return;
    const long long i = f.idx[t];
    const double dx = f.square ? 2.0 * cellfn_x(f, src, t) : 1.0;
    out[i] = g * (f.mv ? cg[f.cell[t]].V : 1.0) * dx * (sc ? sc[i] : 1.0);
}
// ---- launch helpers: the grid arithmetic, once.  part holds DAS_CELLFN_MAX_BLOCKS entries -----------------------------------------------
static inline int cellfn_blocks(long long nt) { return std::max(1, std::min(DAS_CELLFN_MAX_BLOCKS, nblk(nt, 256))); }
// out[0] = coef sum_t w_t g(x_t); part[0 .. cellfn_blocks(f.nt)) = the per-workgroup sums
static void launch_cellfn_value(hipStream_t st, const CellFnView& f, const CellGeom* cg, const double* src, double coef, double* part, double* out) {
    const int nb = cellfn_blocks(f.nt);
    hipLaunchKernelGGL(k_cellfn_value, dim3(nb), dim3(256), 0, st, f, cg, src, part);
    hipLaunchKernelGGL(k_cellfn_sum, dim3(1), dim3(256), 0, st, nb, (const double*)part, coef, out);
}
// f.nt > 0; the caller zeroes out
static void launch_cellfn_grad(hipStream_t st, const CellFnView& f, const CellGeom* cg, const double* src, const double* sc, double g, double* out) {
    hipLaunchKernelGGL(k_cellfn_grad, dim3(nblk(f.nt, 256)), dim3(256), 0, st, f, cg, src, sc, g, out);
}
// volCoord product (dual-point pass): per-cell tangent t_c = a V_c'  (the -N/T^2 part of divByTotalVol over all cells; a = 0 clears)
__global__ __launch_bounds__(256) void k_vc_cellfn_all(int nC, const CellGeomT<Dual<1>>* __restrict__ cg, double a, double* __restrict__ tc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < nC) tc[c] = a * cg[c].V.d[0];
}
// ... plus b g(x_t) V_c' on the cells of the set (multiplyVol; one term per cell)
__global__ __launch_bounds__(256) void k_vc_cellfn_terms(CellFnView f, const CellGeomT<Dual<1>>* __restrict__ cg, const double* __restrict__ src, double b,
                                                         double* __restrict__ tc) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= f.nt) return;
    const int c = f.cell[t];
    const double x = cellfn_x(f, src, t);
    tc[c] += b * (f.square ? x * x : x) * cg[c].V.d[0];
}

// ---- vonMisesStressKS of DASolidDisplacementFoam (reference DAFunctionVonMisesStressKS.C): F = log(sum_t exp(coeffKS vm_t)) / coeffKS
// over the cells of the set, vm_t = solid_von_mises of the cell gradient gradD of the residual pass (traction passes included).  The sum
// runs max-shifted in log space through the two-stage kernels of das_facefn.hpp (k_ks_max ... k_ks_weights) on the compact array a[t].
// a[t] = vm of cell[t]
__global__ __launch_bounds__(256) void k_vm_terms(long long nt, const int* __restrict__ cell, ResParams prm, const double* __restrict__ gD, double scale,
                                                  double* __restrict__ a) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nt) a[t] = solid_von_mises<double>(prm, gD + 9LL * cell[t], scale);
}
// wc[cell[t]] = wt[t]: the softmax weights per cell (the caller zeroes wc; the cells of a set are distinct)
__global__ __launch_bounds__(256) void k_vm_cell_weights(long long nt, const int* __restrict__ cell, const double* __restrict__ wt, double* __restrict__ wc) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < nt) wc[cell[t]] = wt[t];
}
// tc[c] = wc[c] x the tangent of vm_c (dual-number gradD: a state colour, or the dual points of the volCoord pass); 0 outside the set
__global__ __launch_bounds__(256) void k_vm_tangent(int nC, ResParams prm, const Dual<1>* __restrict__ gD, double scale, const double* __restrict__ wc,
                                                    double* __restrict__ tc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nC) return;
    const double w = wc[c];
    tc[c] = w == 0.0 ? 0.0 : w * solid_von_mises<Dual<1>>(prm, gD + 9LL * c, scale).d[0];
}
// dFdW of one colour, a gather without atomics: state j = 3 c + q of colour col receives tc of its cell and of the face neighbours -
// vm reads D at levels 0 and 1, and the distance-2 colouring leaves one state of a colour in the stencil of a cell
__global__ __launch_bounds__(256) void k_vm_gather(DevMesh m, const int* __restrict__ colors, int col, const double* __restrict__ tc, double seed,
                                                   double* __restrict__ out) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 3LL * m.nC || colors[j] != col) return;
    const int c = (int)(j / 3);
    double acc = tc[c];
    for (int s = m.cf_ptr[c]; s < m.cf_ptr[c + 1]; s++)
        if ((m.cf_face[s] & 0x7fffffff) < m.nIF) acc += tc[m.cf_other[s]];
    out[j] = seed * acc;
}
// reads m.nC, m.nIF, m.cf_ptr, m.cf_face, m.cf_other
static void launch_vm_gather(hipStream_t st, const DevMesh& m, const int* colors, int col, const double* tc, double seed, double* out) {
    hipLaunchKernelGGL(k_vm_gather, dim3(nblk(3LL * m.nC, 256)), dim3(256), 0, st, m, colors, col, tc, seed, out);
}

}  // namespace das

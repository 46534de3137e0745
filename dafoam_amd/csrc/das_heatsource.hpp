// Heat sources of DAHeatTransferFoam (reference DAFvSourceHeatSource.C:236-321, the fvSource option with type heatSource):
//   fvSource[c] = sum_k q_k(c),  q_k(c) = power_k s_k(c) / Vt_k,  Vt_k = sum_c s_k(c) V_c          [W/m^3]
//   cylinderToCell   s = 1 on a fixed cell set (chosen once, at definition), 0 elsewhere
//   cylinderSmooth   s = body_heat_source (das_kernels.hpp); with snapCenter2Cell the centre is C of a fixed cell
// The field is a function of the metrics and of the parameters only - never of the states - so it is computed when a source is defined,
// when its parameters are set and when the mesh moves, and the residual kernel k_heat just reads it (DevMeshT::src).
// One global sum per source: two stages, the grid size fixed by the cell count, wave64 shuffles, four waves through LDS, ONE workgroup
// adds the partials in a fixed order - no atomics, the same bits on every call.  Dual<1> sums send the tangent through the same tree.
#pragma once
#include "das_common.hpp"
#include "das_dual.hpp"
#include "das_kernels.hpp"

namespace das {

#define DAS_HS_CYLINDERTOCELL 0
#define DAS_HS_CYLINDERSMOOTH 1
#define DAS_HS_FIELD 2  // s = field[c]: the sum of an existing field times V (sourceTotal)
#define DAS_HS_MAX_BLOCKS 1024

template <class P>  // P: the scalar of the parameters (Dual<1> in the fvSourcePar passes)
struct HsView {
    int kind;
    const unsigned char* member;  // cylinderToCell: 1 on the cells of the set
    const double* field;          // DAS_HS_FIELD
    P center[3], axis[3], radius, length, power;
    double eps;
    int snapCell;  // >= 0: the centre is C of this cell at the metrics of the launch, held fixed (no tangent) within the launch
};

DAS_HD double hs_tangent(double) { return 0.0; }
DAS_HD double hs_tangent(const Dual<1>& a) { return a.d[0]; }
DAS_HD void hs_make(double v, double, double& r) { r = v; }
DAS_HD void hs_make(double v, double d, Dual<1>& r) { r.v = v; r.d[0] = d; }

// s_k(c) in R
template <class R, class P, class G>
DAS_HD R hs_shape(const HsView<P>& v, const CellGeomT<G>* cg, int c) {
    if (v.kind == DAS_HS_CYLINDERTOCELL) return R(v.member[c] ? 1.0 : 0.0);
    if (v.kind == DAS_HS_FIELD) return R(v.field[c]);
    P ctr[3] = {v.center[0], v.center[1], v.center[2]};
    if (v.snapCell >= 0)
        for (int i = 0; i < 3; i++) ctr[i] = P(val(cg[v.snapCell].C[i]));
    return body_heat_source<R, P, G>(ctr, v.axis, v.radius, v.length, v.eps, cg[c].C);
}

__device__ inline double hs_wave_sum(double a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
    return a;
}
__device__ inline Dual<1> hs_wave_sum(Dual<1> a) {
    a.v = hs_wave_sum(a.v);
    a.d[0] = hs_wave_sum(a.d[0]);
    return a;
}
// the sum over the 256 threads of the workgroup, valid on thread 0
template <class R>
__device__ inline R hs_block_sum(R acc) {
    acc = hs_wave_sum(acc);
    __shared__ double sh[4][2];
    if ((threadIdx.x & 63) == 0) { sh[threadIdx.x >> 6][0] = val(acc); sh[threadIdx.x >> 6][1] = hs_tangent(acc); }
    __syncthreads();
    R r;
    hs_make((sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]), (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]), r);
    return r;
}

// stage 1: part[block] = sum over the block's cells (grid-stride) of
//   psi == null:  s_c V_c                                              (Vt; sum V over a set; sum field V)
//   psi != null:  psi_c nrm_c x_c,  nrm_c = V_c (byV) or 1,  x_c = power s_c / vt[0] (vt != null: the source q_c) or s_c
template <class R, class P, class G>
__global__ __launch_bounds__(256) void k_hs_partial(HsView<P> v, int nC, const CellGeomT<G>* __restrict__ cg, const double* __restrict__ psi, int byV,
                                                    const R* __restrict__ vt, R* __restrict__ part) {
    R acc(0.0);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nC; c += gridDim.x * blockDim.x) {
        const R s = hs_shape<R, P, G>(v, cg, c);
        if (!psi) acc += s * R(cg[c].V);
        else acc += (vt ? R(v.power) * s / vt[0] : s) * (psi[c] * (byV ? val(cg[c].V) : 1.0));
    }
    acc = hs_block_sum<R>(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// stage 2: ONE workgroup adds the nb partials in a fixed order
template <class R>
__global__ __launch_bounds__(256) void k_hs_final(int nb, const R* __restrict__ part, R* __restrict__ out) {
    R acc(0.0);
    for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
    acc = hs_block_sum<R>(acc);
    if (threadIdx.x == 0) out[0] = acc;
}
// ---- launch helpers: the grid arithmetic, once.  part holds DAS_HS_MAX_BLOCKS entries of R; n >= 1 -------------------------------------
static inline int hs_blocks(long long n) { return std::min(nblk(n, 256), DAS_HS_MAX_BLOCKS); }
template <class R>
static void launch_hs_final(hipStream_t st, int nb, const R* part, R* out) {
    hipLaunchKernelGGL((k_hs_final<R>), dim3(1), dim3(256), 0, st, nb, part, out);
}
// out[0] = the two-stage sum over all cells; part[0 .. hs_blocks(nC)) = the per-workgroup sums
template <class R, class P, class G>
static void launch_hs_sum(hipStream_t st, const HsView<P>& v, int nC, const CellGeomT<G>* cg, const double* psi, int byV, const R* vt, R* part, R* out) {
    const int nb = hs_blocks(nC);
    hipLaunchKernelGGL((k_hs_partial<R, P, G>), dim3(nb), dim3(256), 0, st, v, nC, cg, psi, byV, vt, part);
    launch_hs_final<R>(st, nb, (const R*)part, out);
}
// src[c] (+)= power s_c / vt[0]: the first source stores, the later ones add
template <class R, class P, class G>
__global__ __launch_bounds__(256) void k_hs_apply(HsView<P> v, int nC, const CellGeomT<G>* __restrict__ cg, const R* __restrict__ vt, int first, R* __restrict__ src) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nC) return;
    const R q = R(v.power) * hs_shape<R, P, G>(v, cg, c) / vt[0];
    src[c] = first ? q : src[c] + q;
}
// volCoord product: what the coloured passes cannot see of one source (v: its frozen form), on the per-cell tangent array -
//   beta (s_c V_c)' on every cell           (the total Vt, beta = -(power / Vt^2) sum psi s nrm)
//   sum_j gamma_j C_j' on the snapped cell  (the snapped centre, gamma_j = sum psi nrm dq / dcenter_j)
// exact mode: the tangents of the dual metrics
__global__ __launch_bounds__(256) void k_hs_vc_rank1(HsView<double> v, int nC, const CellGeomT<Dual<1>>* __restrict__ cg, int snapCell, double beta, double g0,
                                                     double g1, double g2, double* __restrict__ tc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nC) return;
    const Dual<1> sv = hs_shape<Dual<1>, double, Dual<1>>(v, cg, c) * cg[c].V;
    double t = beta * sv.d[0];
    if (c == snapCell) t += g0 * cg[c].C[0].d[0] + g1 * cg[c].C[1].d[0] + g2 * cg[c].C[2].d[0];
    tc[c] += t;
}
// difference mode: the same functional at the metrics of one side, added with the sign of the side (beta and gamma carry it)
__global__ __launch_bounds__(256) void k_hs_fd_rank1(HsView<double> v, int nC, const CellGeom* __restrict__ cg, int snapCell, double beta, double g0, double g1,
                                                     double g2, double* __restrict__ tc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nC) return;
    double t = beta * (hs_shape<double, double, double>(v, cg, c) * cg[c].V);
    if (c == snapCell) t += g0 * cg[c].C[0] + g1 * cg[c].C[1] + g2 * cg[c].C[2];
    tc[c] += t;
}
__global__ __launch_bounds__(256) void k_hs_add(int n, const double* __restrict__ a, double* __restrict__ b) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] += a[i];
}

}  // namespace das

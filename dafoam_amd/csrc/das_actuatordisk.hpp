// Actuator disks of DASimpleFoam (reference DAFvSourceActuatorDisk.C:93-429, the fvSource option with type actuatorDisk):
//   fvSource[c] = sum_k f_k(c)   [force per unit volume; the U equation carries - fvSource, DAResidualSimpleFoam.C:141-147]
//   cylinderAnnulusToCell  f = body_actuator_disk(smooth = 0) on a fixed cell set (chosen once, at definition), 0 elsewhere
//   cylinderAnnulusSmooth  f = body_actuator_disk(smooth = 1) on every cell; with adjustThrust scale = targetThrust / sum fAxial(scale = 1) V
// Like the heat sources (das_heatsource.hpp) the field is a function of the metrics and of the parameters only: it is computed when a
// disk is defined, when its parameters are set and when the mesh moves, and the cell kernels just read it (DevMeshT::src3).  The sums are
// the two-stage fixed-order sums of das_heatsource.hpp (hs_block_sum, k_hs_final): no atomics, the same bits on every call, Dual<1>
// through the same tree.  The scale stays on the device between the sum and the field: no host round trip inside a refresh.
#pragma once
#include "das_heatsource.hpp"

namespace das {

template <class P>  // P: the scalar of the parameters (Dual<1> in the fvSourcePar passes)
struct AdView {
    int smooth, adjustThrust;
    const unsigned char* member;  // cylinderAnnulusToCell: 1 on the cells of the set; null for a smooth disk
    P center[3], direction[3], innerRadius, outerRadius, scale, POD, expM, expN, targetThrust;
    double eps, rotSign;
};

// f[0..4] of disk v at cell c with the given scale; returns 1 where the reference would divide by zero
template <class R, class P, class G>
DAS_HD int ad_eval(const AdView<P>& v, const R& scale, const CellGeomT<G>* cg, int c, R* f) {
    if (v.member && !v.member[c]) {
#pragma unroll
        for (int i = 0; i < 5; i++) f[i] = R(0.0);
        return 0;
    }
    return body_actuator_disk<R, P, G>(v.smooth, v.center, v.direction, v.innerRadius, v.outerRadius, scale, v.POD, v.expM, v.expN, v.eps, v.rotSign, cg[c].C, f);
}

// stage 1 of two sums at once: part[2 b] = sum fAxial V, part[2 b + 1] = sum fCirc V over the cells of block b (grid-stride);
// scale == null: at scale 1 (the total that adjustThrust divides by)
template <class R, class P, class G>
__global__ __launch_bounds__(256) void k_ad_partial(AdView<P> v, int nC, const CellGeomT<G>* __restrict__ cg, const R* __restrict__ scale, R* __restrict__ part) {
    R thrust(0.0), torque(0.0);
    const R sc = scale ? scale[0] : R(1.0);
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < nC; c += gridDim.x * blockDim.x) {
        R f[5];
        ad_eval<R, P, G>(v, sc, cg, c, f);
        thrust += f[3] * R(cg[c].V);
        torque += f[4] * R(cg[c].V);
    }
    thrust = hs_block_sum<R>(thrust);
    __syncthreads();  // the LDS slots of the first sum are read before the second writes them
    torque = hs_block_sum<R>(torque);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = thrust; part[2 * blockIdx.x + 1] = torque; }
}
// stage 2: ONE workgroup adds the nb pairs in a fixed order
template <class R>
__global__ __launch_bounds__(256) void k_ad_final(int nb, const R* __restrict__ part, R* __restrict__ out2) {
    R thrust(0.0), torque(0.0);
    for (int i = threadIdx.x; i < nb; i += 256) { thrust += part[2 * i]; torque += part[2 * i + 1]; }
    thrust = hs_block_sum<R>(thrust);
    __syncthreads();
    torque = hs_block_sum<R>(torque);
    if (threadIdx.x == 0) { out2[0] = thrust; out2[1] = torque; }
}
// the effective scale: the parameter, or with adjustThrust targetThrust over the thrust at scale 1 (unit2[0])
template <class R, class P>
__global__ void k_ad_scale(AdView<P> v, const R* __restrict__ unit2, R* __restrict__ scale) {
    if (blockIdx.x == 0 && threadIdx.x == 0) scale[0] = v.adjustThrust ? R(v.targetThrust) / unit2[0] : R(v.scale);
}
// src3[3 c + k] (+)= f_k: the first disk stores, the later ones add; bad[0] = 1 where a cell centre sits on the axis
template <class R, class P, class G>
__global__ __launch_bounds__(256) void k_ad_apply(AdView<P> v, int nC, const CellGeomT<G>* __restrict__ cg, const R* __restrict__ scale, int first,
                                                  R* __restrict__ src3, int* __restrict__ bad) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nC) return;
    R f[5];
    if (ad_eval<R, P, G>(v, scale[0], cg, c, f)) bad[0] = 1;
#pragma unroll
    for (int k = 0; k < 3; k++) src3[3LL * c + k] = first ? f[k] : src3[3LL * c + k] + f[k];
}
// stage 1 of seeds . (tangent of a dual residual); k_hs_final<double> finishes it
__global__ __launch_bounds__(256) void k_ad_dot_partial(long long n, const double* __restrict__ psi, const Dual<1>* __restrict__ Rd, double* __restrict__ part) {
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) acc += psi[i] * Rd[i].d[0];
    acc = hs_block_sum<double>(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
// ---- launch helpers: the grid arithmetic, once (hs_blocks of das_heatsource.hpp).  part holds 2 DAS_HS_MAX_BLOCKS entries of R for the
// pair of sums, DAS_HS_MAX_BLOCKS doubles for the dot product; n >= 1
template <class R>
static void launch_ad_final(hipStream_t st, int nb, const R* part, R* out2) {
    hipLaunchKernelGGL((k_ad_final<R>), dim3(1), dim3(256), 0, st, nb, part, out2);
}
template <class R, class P, class G>
static void launch_ad_sums(hipStream_t st, const AdView<P>& v, int nC, const CellGeomT<G>* cg, const R* scale, R* part, R* out2) {
    const int nb = hs_blocks(nC);
    hipLaunchKernelGGL((k_ad_partial<R, P, G>), dim3(nb), dim3(256), 0, st, v, nC, cg, scale, part);
    launch_ad_final<R>(st, nb, (const R*)part, out2);
}
// out[0] = sum_i psi_i Rd_i.d[0]
static void launch_ad_dot(hipStream_t st, long long n, const double* psi, const Dual<1>* Rd, double* part, double* out) {
    const int nb = hs_blocks(n);
    hipLaunchKernelGGL(k_ad_dot_partial, dim3(nb), dim3(256), 0, st, n, psi, Rd, part);
    launch_hs_final<double>(st, nb, (const double*)part, out);
}
// volCoord product: what the coloured passes cannot see of an adjustThrust disk - the total S = sum fAxial(scale = 1) V moves with every
// cell.  beta = - (scale / S) (seeds . dR / dscale) multiplies (fAxial_1 V)' of every cell, on the per-cell tangent array.
// exact mode: the tangents of the dual metrics
template <class P>
__global__ __launch_bounds__(256) void k_ad_vc_rank1(AdView<P> v, int nC, const CellGeomT<Dual<1>>* __restrict__ cg, double beta, double* __restrict__ tc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nC) return;
    Dual<1> f[5];
    ad_eval<Dual<1>, P, Dual<1>>(v, Dual<1>(1.0), cg, c, f);
    tc[c] += beta * (f[3] * cg[c].V).d[0];
}
// difference mode: the same functional at the metrics of one side (beta carries the sign of the side)
template <class P>
__global__ __launch_bounds__(256) void k_ad_fd_rank1(AdView<P> v, int nC, const CellGeom* __restrict__ cg, double beta, double* __restrict__ tc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nC) return;
    double f[5];
    ad_eval<double, P, double>(v, 1.0, cg, c, f);
    tc[c] += beta * (f[3] * cg[c].V);
}

}  // namespace das

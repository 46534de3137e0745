// The small fixed-order reductions that several subsystems share: the one-workgroup group sum that finishes the per-face objective
// functions and the two dot products below, the seeds . dR product of the boundary-input derivatives, and the dot product of the inner
// Krylov solvers of the SIMPLE sweeps.  All three reduce 256 accumulators through an LDS tree; no atomics, the same bits on every call.
#pragma once
#include "das_common.hpp"
#include "das_dual.hpp"

namespace das {

#define DAS_TANGENT_DOT_BLOCKS 1024
#define DAS_SV_DOT_MAX_BLOCKS 512

// out2[g] = sum of fv[k] over the entries of group g (group == nullptr: everything is group 0); one workgroup, fixed order
__global__ __launch_bounds__(256) void k_group_sum(long long cnt, const unsigned char* __restrict__ group, const double* __restrict__ fv, double* __restrict__ out2) {
    __shared__ double sh[2][256];
    double a0 = 0.0, a1 = 0.0;
    for (long long k = threadIdx.x; k < cnt; k += 256) {
        const double v = fv[k];
        if (group && group[k]) a1 += v; else a0 += v;
    }
    sh[0][threadIdx.x] = a0; sh[1][threadIdx.x] = a1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sh[0][threadIdx.x] += sh[0][threadIdx.x + o]; sh[1][threadIdx.x] += sh[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out2[0] = sh[0][0]; out2[1] = sh[1][0]; }
}
// part[b] = sum over the block's rows of psi_i * dR_i  (dR = tangent part of a dual residual); k_group_sum adds the parts
__global__ __launch_bounds__(256) void k_tangent_dot(long long n, const Dual<1>* __restrict__ R, const double* __restrict__ psi, double* __restrict__ part) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) acc += psi[i] * R[i].d[0];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
// small vector kernel of the inner Krylov solvers (host scalars; the sweeps are the reference's primal, not the fast path)
__global__ __launch_bounds__(256) void k_sv_dot(long long n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ part) {
    __shared__ double sh[256];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) acc += a[i] * b[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// ---- launch helpers: the grid arithmetic, once ------------------------------------------------------------------------------------------
// out2 holds two entries
static void launch_group_sum(hipStream_t st, long long cnt, const unsigned char* group, const double* fv, double* out2) {
    hipLaunchKernelGGL(k_group_sum, dim3(1), dim3(256), 0, st, cnt, group, fv, out2);
}
// out2[0] = sum_i psi_i R_i.d[0] (out2[1] = 0); part holds DAS_TANGENT_DOT_BLOCKS entries, all of them written (a workgroup without rows writes 0)
static void launch_tangent_dot(hipStream_t st, long long n, const Dual<1>* R, const double* psi, double* part, double* out2) {
    hipLaunchKernelGGL(k_tangent_dot, dim3(DAS_TANGENT_DOT_BLOCKS), dim3(256), 0, st, n, R, psi, part);
    launch_group_sum(st, (long long)DAS_TANGENT_DOT_BLOCKS, nullptr, part, out2);
}
static inline int sv_dot_blocks(long long n) { return (int)std::min<long long>(DAS_SV_DOT_MAX_BLOCKS, (n + 255) / 256); }
// out2[0] = a . b (out2[1] = 0); part holds DAS_SV_DOT_MAX_BLOCKS entries, the first sv_dot_blocks(n) are written; n >= 1
static void launch_sv_dot(hipStream_t st, long long n, const double* a, const double* b, double* part, double* out2) {
    const int nb = sv_dot_blocks(n);
    hipLaunchKernelGGL(k_sv_dot, dim3(nb), dim3(256), 0, st, n, a, b, part);
    launch_group_sum(st, (long long)nb, nullptr, part, out2);
}

}  // namespace das

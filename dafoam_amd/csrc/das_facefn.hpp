// KS aggregate of a face set (reference DAFunctionLocation.C:163-253, modes maxRadiusKS / maxInverseRadiusKS):
//   F = log( sum_f exp(k a_f) ) / k          k = coeffKS, a_f = the per-face quantity (body_facefn kind 8)
// evaluated in log space so that no exponential can overflow:
//   m = max_f k a_f ;  S = sum_f exp(k a_f - m)  (1 <= S <= nf) ;  F = (m + log S) / k
// and its derivative weights, the softmax  dF/da_f = exp(k a_f - m) / S.
// Both passes are two-stage like k_cellfn_value + k_cellfn_sum: per-workgroup partials over a grid that depends on the number of
// faces only, then ONE workgroup combines them in a fixed order - the value is the same bits on every call, and the face set may be
// as large as the mesh's boundary.
#pragma once
#include "das_common.hpp"

namespace das {

#define DAS_FACEFN_MAX_BLOCKS 1024

// stage 1 of the maximum: part[b] = max over the block's faces of k a_f
__global__ __launch_bounds__(256) void k_ks_max(long long n, const double* __restrict__ a, double k, double* __restrict__ part) {
    double acc = -1.79769313486231570e308;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) acc = fmax(acc, k * a[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = fmax(acc, __shfl_down(acc, o, 64));
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
// stage 2 of the maximum: ONE workgroup, ms[0] = m
__global__ __launch_bounds__(256) void k_ks_max_final(int nb, const double* __restrict__ part, double* __restrict__ ms) {
    double acc = -1.79769313486231570e308;
    for (int i = threadIdx.x; i < nb; i += 256) acc = fmax(acc, part[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = fmax(acc, __shfl_down(acc, o, 64));
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ms[0] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}
// stage 1 of the sum: part[b] = sum over the block's faces of exp(k a_f - m), m = ms[0]
__global__ __launch_bounds__(256) void k_ks_expsum(long long n, const double* __restrict__ a, double k, const double* __restrict__ ms, double* __restrict__ part) {
    const double m = ms[0];
    double acc = 0.0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) acc += exp(k * a[t] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// stage 2 of the sum: ONE workgroup adds the nb partials in a fixed order, ms[1] = S
__global__ __launch_bounds__(256) void k_ks_sum_final(int nb, const double* __restrict__ part, double* __restrict__ ms) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += 256) acc += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) ms[1] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// w_f = outer exp(k a_f - m) / S : the effective per-face weights of the derivative passes (outer = dF/dF0 of calcRefVar, else 1)
__global__ __launch_bounds__(256) void k_ks_weights(long long n, const double* __restrict__ a, double k, const double* __restrict__ ms, double outer,
                                                    double* __restrict__ w) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) w[t] = outer * exp(k * a[t] - ms[0]) / ms[1];
}

// ---- launch helpers: the grid arithmetic of the KS reduction, once.  part holds DAS_FACEFN_MAX_BLOCKS entries, ms two ({m, S}) --------
static inline int ks_blocks(long long n) { return std::max(1, std::min(DAS_FACEFN_MAX_BLOCKS, nblk(n, 256))); }
// ms[0] = max_t k a_t; part[0 .. ks_blocks(n)) = the per-workgroup maxima
static void launch_ks_max(hipStream_t st, long long n, const double* a, double k, double* part, double* ms) {
    const int nb = ks_blocks(n);
    hipLaunchKernelGGL(k_ks_max, dim3(nb), dim3(256), 0, st, n, a, k, part);
    hipLaunchKernelGGL(k_ks_max_final, dim3(1), dim3(256), 0, st, nb, (const double*)part, ms);
}
// ms[1] = the fixed-order sum of nb partials (the second stage of the exponential sum and of residualNorm)
static void launch_ks_sum_final(hipStream_t st, int nb, const double* part, double* ms) {
    hipLaunchKernelGGL(k_ks_sum_final, dim3(1), dim3(256), 0, st, nb, part, ms);
}
// ms[1] = sum_t exp(k a_t - ms[0]); part[0 .. ks_blocks(n)) = the per-workgroup sums
static void launch_ks_expsum(hipStream_t st, long long n, const double* a, double k, double* part, double* ms) {
    const int nb = ks_blocks(n);
    hipLaunchKernelGGL(k_ks_expsum, dim3(nb), dim3(256), 0, st, n, a, k, (const double*)ms, part);
    launch_ks_sum_final(st, nb, part, ms);
}
// the whole sequence: {m, S} -> ms through one partial buffer
static void launch_ks_reduce(hipStream_t st, long long n, const double* a, double k, double* part, double* ms) {
    launch_ks_max(st, n, a, k, part, ms);
    launch_ks_expsum(st, n, a, k, part, ms);
}
static void launch_ks_weights(hipStream_t st, long long n, const double* a, double k, const double* ms, double outer, double* w) {
    hipLaunchKernelGGL(k_ks_weights, dim3(nblk(n, 256)), dim3(256), 0, st, n, a, k, ms, outer, w);
}

}  // namespace das

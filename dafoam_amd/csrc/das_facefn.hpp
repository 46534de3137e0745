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

}  // namespace das

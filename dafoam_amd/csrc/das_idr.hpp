// Vector kernels of the IDR(s) solver (amd.krylovMethod "idrs", das_idr_host.hpp): the shadow-space fill (k_idr_shadow), the
// linear combination that builds v and u_k (k_idr_combine), the fused biorthogonalisation + residual / solution update
// (k_idr_biortho_step), the fused smoothing update with the projections of the new residual (k_idr_smooth_step), and the launch
// helpers that hold their grid arithmetic.  The inner products P^T g_k and (r.t, t.t) are launch_multidot of das_krylov.hpp.
// All vectors fp64, all sums fp64 in a fixed order: per-block partials, then k_reduce; no atomics.  Nothing here knows a solver handle.
// Loads and stores: a lane owns W consecutive rows.  W = 2 (one 16-byte access per vector and lane) needs every pointer 16-byte
// aligned and an even leading dimension (idr_wide_ok); the last row of an odd n goes element-wise in the same launch.  Everything
// else runs W = 1.  The two paths sum the rows in different orders; each is deterministic.
#pragma once
#include <cstdint>
#include <initializer_list>

#include "das_idr_host.hpp"
#include "das_krylov.hpp"

namespace das {

// rows [k, k + cnt) of a vector, cnt in 0 .. W: absent rows read as zero and are not written
template <int W>
__device__ __forceinline__ void idr_ld(const double* p, long long k, int cnt, double (&v)[W]) {
    if (W == 2 && cnt == 2) {
        const f64x2 a = *reinterpret_cast<const f64x2*>(p + k);
        v[0] = a.x; v[W - 1] = a.y;
        return;
    }
#pragma unroll
    for (int e = 0; e < W; e++) v[e] = e < cnt ? p[k + e] : 0.0;
}
template <int W>
__device__ __forceinline__ void idr_st(double* p, long long k, int cnt, const double (&v)[W]) {
    if (W == 2 && cnt == 2) {
        *reinterpret_cast<f64x2*>(p + k) = f64x2{v[0], v[W - 1]};
        return;
    }
#pragma unroll
    for (int e = 0; e < W; e++) if (e < cnt) p[k + e] = v[e];
}
// first row and number of rows of this lane
template <int W>
__device__ __forceinline__ long long idr_rows(long long n, int& cnt) {
    const long long k = ((long long)blockIdx.x * 256 + threadIdx.x) * W;
    cnt = k >= n ? 0 : (int)(n - k < W ? n - k : W);
    return k;
}
// sum over the workgroup (256 lanes), stored by lane 0; red: 4 doubles of LDS
__device__ __forceinline__ void idr_block_sum(double v, double* red, double* dst) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) *dst = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
}

// P[col ld + row] = idr_shadow_entry(seed, row, col)
__global__ __launch_bounds__(256) void k_idr_shadow(long long n, int s, unsigned seed, double* __restrict__ P, long long ld) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    for (int q = 0; q < s; q++) P[(long long)q * ld + k] = idr_shadow_entry(seed, k, q);
}
// y = a x + sum_{i < m} c_i V_i  (m <= IDR_MAX_S).  y may be column 0 of V (the in-place u_k): a lane reads all of its rows before it
// writes any - so neither y nor V is __restrict__
template <int W>
__global__ __launch_bounds__(256) void k_idr_combine(long long n, int m, double a, const double* __restrict__ x, const double* V, long long ldv,
                                                     const double* __restrict__ c, double* y) {
    int cnt;
    const long long k = idr_rows<W>(n, cnt);
    if (cnt == 0) return;
    double acc[W], v[W];
    idr_ld<W>(x, k, cnt, acc);
#pragma unroll
    for (int e = 0; e < W; e++) acc[e] *= a;
    for (int i = 0; i < m; i++) {
        const double ci = c[i];
        idr_ld<W>(V + (long long)i * ldv, k, cnt, v);
#pragma unroll
        for (int e = 0; e < W; e++) acc[e] += ci * v[e];
    }
    idr_st<W>(y, k, cnt, acc);
}
// step k of a cycle, fused: g_k -= sum_{j < k} alpha_j g_j, u_k -= sum_{j < k} alpha_j u_j, r -= beta g_k, x += beta u_k, and this
// block's part of r.r in partial[blockIdx].  coef = [alpha_0 .. alpha_{k-1}, beta].  Reads 2 k + 4 vectors, writes 4; k = 0 is the plain
// r, x update.
template <int W>
__global__ __launch_bounds__(256) void k_idr_biortho_step(long long n, int k, double* __restrict__ G, double* __restrict__ U, long long ld,
                                                          const double* __restrict__ coef, double* __restrict__ r, double* __restrict__ x,
                                                          double* __restrict__ partial) {
    __shared__ double red[4];
    int cnt;
    const long long row = idr_rows<W>(n, cnt);
    double rr = 0.0;
    if (cnt > 0) {
        double g[W], u[W], v[W], rv[W], xv[W];
        idr_ld<W>(G + (long long)k * ld, row, cnt, g);
        idr_ld<W>(U + (long long)k * ld, row, cnt, u);
        for (int j = 0; j < k; j++) {
            const double aj = coef[j];
            idr_ld<W>(G + (long long)j * ld, row, cnt, v);
#pragma unroll
            for (int e = 0; e < W; e++) g[e] -= aj * v[e];
            idr_ld<W>(U + (long long)j * ld, row, cnt, v);
#pragma unroll
            for (int e = 0; e < W; e++) u[e] -= aj * v[e];
        }
        const double beta = coef[k];
        idr_ld<W>(r, row, cnt, rv);
        idr_ld<W>(x, row, cnt, xv);
#pragma unroll
        for (int e = 0; e < W; e++) { rv[e] -= beta * g[e]; xv[e] += beta * u[e]; }
        if (k > 0) {
            idr_st<W>(G + (long long)k * ld, row, cnt, g);
            idr_st<W>(U + (long long)k * ld, row, cnt, u);
        }
        idr_st<W>(r, row, cnt, rv);
        idr_st<W>(x, row, cnt, xv);
#pragma unroll
        for (int e = 0; e < W; e++) rr += rv[e] * rv[e];  // absent rows hold zero
    }
    idr_block_sum(rr, red, partial + blockIdx.x);
}
// the smoothing update, fused: r -= omega t, x += omega z, and this block's part of P_i . r (i < s) in partial[i nb + blockIdx] and of
// r.r in partial[s nb + blockIdx].  The lane's rows of the new r stay in registers across the columns of P.
template <int W>
__global__ __launch_bounds__(256) void k_idr_smooth_step(long long n, int s, double omega, double* __restrict__ r, const double* __restrict__ t,
                                                         double* __restrict__ x, const double* __restrict__ z, const double* __restrict__ P, long long ldp,
                                                         double* __restrict__ partial, int nb) {
    __shared__ double red[4];
    int cnt;
    const long long row = idr_rows<W>(n, cnt);
    double rv[W], v[W];
#pragma unroll
    for (int e = 0; e < W; e++) rv[e] = 0.0;
    if (cnt > 0) {
        double xv[W];
        idr_ld<W>(r, row, cnt, rv);
        idr_ld<W>(t, row, cnt, v);
#pragma unroll
        for (int e = 0; e < W; e++) rv[e] -= omega * v[e];
        idr_ld<W>(x, row, cnt, xv);
        idr_ld<W>(z, row, cnt, v);
#pragma unroll
        for (int e = 0; e < W; e++) xv[e] += omega * v[e];
        idr_st<W>(r, row, cnt, rv);
        idr_st<W>(x, row, cnt, xv);
    }
    for (int i = 0; i <= s; i++) {
        double a = 0.0;
        if (i < s) {
            if (cnt > 0) {
                idr_ld<W>(P + (long long)i * ldp, row, cnt, v);
#pragma unroll
                for (int e = 0; e < W; e++) a += v[e] * rv[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < W; e++) a += rv[e] * rv[e];
        }
        idr_block_sum(a, red, partial + (long long)i * nb + blockIdx.x);
    }
}

// ---- launch helpers ---------------------------------------------------------------------------------------------------------
// the one place that holds the grid arithmetic: the solver (IdrDeviceOps) and the test-only entries das_debug_idr_* run the SAME launches
static inline bool idr_wide_ok(long long n, long long ld, std::initializer_list<const void*> ptrs) {
    if (n < 2 || (ld & 1)) return false;
    uintptr_t a = 0;
    for (const void* p : ptrs) a |= (uintptr_t)p;
    return (a & 15) == 0;
}
static inline int idr_nb(long long n, bool wide) { return nblk(wide ? (n + 1) / 2 : n, 256); }
// doubles of the partial-sum array one solve needs (the fused kernels and the multi-dots against P)
static inline size_t idr_partial_size(long long n, int s) { return std::max((size_t)(s + 1) * idr_nb(n, false), multidot_partial_size(n, s)); }
static void launch_idr_shadow(hipStream_t st, long long n, int s, unsigned seed, double* P, long long ld) {
    hipLaunchKernelGGL(k_idr_shadow, dim3(nblk(n, 256)), dim3(256), 0, st, n, s, seed, P, ld);
}
// y = a x + sum_{i < m} c_i V_i; c on the device; y may be V (column 0)
static void launch_idr_combine(hipStream_t st, long long n, int m, double a, const double* x, const double* V, long long ldv, const double* c, double* y) {
    if (idr_wide_ok(n, ldv, {x, V, y})) hipLaunchKernelGGL(k_idr_combine<2>, dim3(idr_nb(n, true)), dim3(256), 0, st, n, m, a, x, V, ldv, c, y);
    else hipLaunchKernelGGL(k_idr_combine<1>, dim3(idr_nb(n, false)), dim3(256), 0, st, n, m, a, x, V, ldv, c, y);
}
// out[0] = r.r after the fused step k (coef = [alpha (k); beta] on the device)
static void launch_idr_biortho_step(hipStream_t st, long long n, int k, double* G, double* U, long long ld, const double* coef, double* r, double* x,
                                    double* partial, double* out) {
    const bool wide = idr_wide_ok(n, ld, {G, U, r, x});
    const int nb = idr_nb(n, wide);
    if (wide) hipLaunchKernelGGL(k_idr_biortho_step<2>, dim3(nb), dim3(256), 0, st, n, k, G, U, ld, coef, r, x, partial);
    else hipLaunchKernelGGL(k_idr_biortho_step<1>, dim3(nb), dim3(256), 0, st, n, k, G, U, ld, coef, r, x, partial);
    hipLaunchKernelGGL(k_reduce, dim3(1), dim3(256), 0, st, nb, (const double*)partial, out);
}
// out[0..s) = P^T r, out[s] = r.r after the fused smoothing update
static void launch_idr_smooth_step(hipStream_t st, long long n, int s, double omega, double* r, const double* t, double* x, const double* z, const double* P,
                                   long long ldp, double* partial, double* out) {
    const bool wide = idr_wide_ok(n, ldp, {r, t, x, z, P});
    const int nb = idr_nb(n, wide);
    if (wide) hipLaunchKernelGGL(k_idr_smooth_step<2>, dim3(nb), dim3(256), 0, st, n, s, omega, r, t, x, z, P, ldp, partial, nb);
    else hipLaunchKernelGGL(k_idr_smooth_step<1>, dim3(nb), dim3(256), 0, st, n, s, omega, r, t, x, z, P, ldp, partial, nb);
    hipLaunchKernelGGL(k_reduce, dim3(s + 1), dim3(256), 0, st, nb, (const double*)partial, out);
}

}  // namespace das

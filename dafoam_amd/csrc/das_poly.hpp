// Vector kernels of the polynomial-preconditioned GMRES (amd.polyDegree, das_poly_host.hpp): the element-wise updates between the
// operator products of t = p(B) v, fused so that a root step is ONE pass over its vectors, and the launch helpers that hold their grid
// arithmetic.
//   k_poly_real         poly (+)= prod / c;  prod = prod - w / c              (real root theta: c = theta, w = B prod)
//   k_poly_pair_first   tmp = twoa prod - w;  poly (+)= tmp / c                (pair a +- i b: twoa = 2 a, c = a^2 + b^2, w = B prod)
//   k_poly_pair_second  prod = prod - w / c                                    (w = B tmp)
// True fp64 divisions (one rounding each, as the host twin; the kernels stay bound by their loads and stores).
// FIRST: prod is still the input vector v - it is read through `pin` and never written, and poly is not read (it starts as zero): no
// copy and no zero fill before the walk.  LAST (real step): the prod update is skipped, w is not read; the second pair step of a
// last pair is not launched at all.  `pin` and `pout` are the same vector except on the first step (a lane reads its rows before it
// writes them: neither is __restrict__).
// All vectors fp64; no sums, no atomics.  Nothing here knows a solver handle.  Loads and stores as in das_idr.hpp: a lane owns W
// consecutive rows, W = 2 (one 16-byte access per vector and lane) needs every pointer 16-byte aligned (idr_wide_ok), the last row of an
// odd n goes element-wise in the same launch; everything else runs W = 1.
#pragma once
#include "das_idr.hpp"
#include "das_poly_host.hpp"

namespace das {

template <int W, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_poly_real(long long n, double c, const double* pin, const double* __restrict__ w, double* __restrict__ poly, double* pout) {
    int cnt;
    const long long k = idr_rows<W>(n, cnt);
    if (cnt == 0) return;
    double p[W], q[W];
    idr_ld<W>(pin, k, cnt, p);
    if (FIRST) {
#pragma unroll
        for (int e = 0; e < W; e++) q[e] = p[e] / c;
    } else {
        idr_ld<W>(poly, k, cnt, q);
#pragma unroll
        for (int e = 0; e < W; e++) q[e] += p[e] / c;
    }
    idr_st<W>(poly, k, cnt, q);
    if (LAST) return;
    double wv[W];
    idr_ld<W>(w, k, cnt, wv);
#pragma unroll
    for (int e = 0; e < W; e++) p[e] -= wv[e] / c;
    idr_st<W>(pout, k, cnt, p);
}
template <int W, bool FIRST>
__global__ __launch_bounds__(256) void k_poly_pair_first(long long n, double twoa, double c, const double* __restrict__ pin, const double* __restrict__ w,
                                                         double* __restrict__ poly, double* __restrict__ tmp) {
    int cnt;
    const long long k = idr_rows<W>(n, cnt);
    if (cnt == 0) return;
    double p[W], wv[W], q[W];
    idr_ld<W>(pin, k, cnt, p);
    idr_ld<W>(w, k, cnt, wv);
#pragma unroll
    for (int e = 0; e < W; e++) p[e] = twoa * p[e] - wv[e];
    if (FIRST) {
#pragma unroll
        for (int e = 0; e < W; e++) q[e] = p[e] / c;
    } else {
        idr_ld<W>(poly, k, cnt, q);
#pragma unroll
        for (int e = 0; e < W; e++) q[e] += p[e] / c;
    }
    idr_st<W>(tmp, k, cnt, p);
    idr_st<W>(poly, k, cnt, q);
}
template <int W>
__global__ __launch_bounds__(256) void k_poly_pair_second(long long n, double c, const double* pin, const double* __restrict__ w, double* pout) {
    int cnt;
    const long long k = idr_rows<W>(n, cnt);
    if (cnt == 0) return;
    double p[W], wv[W];
    idr_ld<W>(pin, k, cnt, p);
    idr_ld<W>(w, k, cnt, wv);
#pragma unroll
    for (int e = 0; e < W; e++) p[e] -= wv[e] / c;
    idr_st<W>(pout, k, cnt, p);
}

// ---- launch helpers ---------------------------------------------------------------------------------------------------------
// the one place that holds the grid arithmetic: the solver (PolyDeviceOps) and the test-only entry das_debug_poly_step run the SAME launches.
// v: the input of the walk (read while `first`), prod / poly / tmp: the three work vectors, w: the operator product of the step
static void launch_poly_real(hipStream_t st, long long n, bool first, bool last, double c, const double* v, const double* w, double* poly, double* prod) {
    const double* pin = first ? v : prod;
    const bool wide = last ? idr_wide_ok(n, 0, {pin, poly}) : idr_wide_ok(n, 0, {pin, w, poly, prod});
    const dim3 grid(idr_nb(n, wide)), block(256);
#define DAS_POLY_REAL(F, L)                                                                                     \
    do {                                                                                                        \
        if (wide) hipLaunchKernelGGL((k_poly_real<2, F, L>), grid, block, 0, st, n, c, pin, w, poly, prod);     \
        else hipLaunchKernelGGL((k_poly_real<1, F, L>), grid, block, 0, st, n, c, pin, w, poly, prod);          \
    } while (0)
    if (first && last) DAS_POLY_REAL(true, true);
    else if (first) DAS_POLY_REAL(true, false);
    else if (last) DAS_POLY_REAL(false, true);
    else DAS_POLY_REAL(false, false);
#undef DAS_POLY_REAL
}
static void launch_poly_pair_first(hipStream_t st, long long n, bool first, double twoa, double c, const double* v, const double* prod, const double* w, double* poly,
                                   double* tmp) {
    const double* pin = first ? v : prod;
    const bool wide = idr_wide_ok(n, 0, {pin, w, poly, tmp});
    const dim3 grid(idr_nb(n, wide)), block(256);
    if (first) {
        if (wide) hipLaunchKernelGGL((k_poly_pair_first<2, true>), grid, block, 0, st, n, twoa, c, pin, w, poly, tmp);
        else hipLaunchKernelGGL((k_poly_pair_first<1, true>), grid, block, 0, st, n, twoa, c, pin, w, poly, tmp);
    } else {
        if (wide) hipLaunchKernelGGL((k_poly_pair_first<2, false>), grid, block, 0, st, n, twoa, c, pin, w, poly, tmp);
        else hipLaunchKernelGGL((k_poly_pair_first<1, false>), grid, block, 0, st, n, twoa, c, pin, w, poly, tmp);
    }
}
// (never for the last pair of a walk: its prod is not needed)
static void launch_poly_pair_second(hipStream_t st, long long n, bool first, double c, const double* v, const double* w, double* prod) {
    const double* pin = first ? v : prod;
    const bool wide = idr_wide_ok(n, 0, {pin, w, prod});
    const dim3 grid(idr_nb(n, wide)), block(256);
    if (wide) hipLaunchKernelGGL(k_poly_pair_second<2>, grid, block, 0, st, n, c, pin, w, prod);
    else hipLaunchKernelGGL(k_poly_pair_second<1>, grid, block, 0, st, n, c, pin, w, prod);
}

}  // namespace das

// Krylov vector kernels of the GMRES engine: the inner products against the basis (k_multidot, the fused two-right-hand-side
// k_multidot2 of the delayed re-orthogonalisation and its 16-byte-load variant k_multidot2w), the basis updates (k_multiaxpy,
// k_dcgs2_update, k_dcgs2w_update), k_lincomb, k_scale_to, and the launch helpers that hold their grid arithmetic.  The basis is
// stored as fp64, fp32 or split (float hi + float lo); all sums are fp64.  Nothing here knows a solver handle.
#pragma once
#include "das_common.hpp"

namespace das {

// partial[i*nb + blk] = sum over this block's chunk of V_i . w   (i < m); last slot (i == m) = w . w
// Split storage of the Krylov basis (amd.krylovBasisPrecision "split"): a basis entry x is kept as hi = (float)x and lo = (float)(x - hi) in
// TWO float arrays (8 bytes per entry like fp64; hi + lo carries 48 mantissa bits).  The inner-product pass of the delayed
// re-orthogonalisation reads only the hi array (4 bytes per entry), the update pass reads and writes both - every consumer that builds
// vectors (updates, the solution update, the preconditioner input) uses hi + lo, so the Arnoldi relation holds to 2^-48, while the
// Gram-Schmidt coefficients carry fp32-level errors, which only cost orthogonality (1e-7).  Kernels below take the lo array as an optional
// pointer next to a float basis: null = plain fp32 storage (amd.krylovBasisPrecision "fp32").
// (VT: storage type of the Krylov basis - double, or float for the compressed basis of amd.krylovBasisPrecision; all sums in fp64)
#define MD_CHUNK 1024
template <class VT>
__global__ __launch_bounds__(256) void k_multidot(long long n, int m, const VT* __restrict__ V, long long ldv, const double* __restrict__ w,
                                                  double* __restrict__ partial, int nb) {
    __shared__ double red[4];
    long long base = (long long)blockIdx.x * MD_CHUNK;
    double wr[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        long long k = base + threadIdx.x + 256 * t;
        wr[t] = k < n ? w[k] : 0.0;
    }
    for (int i = 0; i <= m; i++) {
        double s = 0.0;
        if (i < m) {
            const VT* vi = V + (long long)i * ldv;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                long long k = base + threadIdx.x + 256 * t;
                if (k < n) s += (double)vi[k] * wr[t];
            }
        } else {
#pragma unroll
            for (int t = 0; t < 4; t++) s += wr[t] * wr[t];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) partial[(long long)i * nb + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_reduce(int nb, const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double red[4];
    const double* p = partial + (long long)blockIdx.x * nb;
    double s = 0.0;
    for (int k = threadIdx.x; k < nb; k += 256) s += p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
// w -= sum_i h_i V_i
template <class VT, class WT>
__global__ __launch_bounds__(256) void k_multiaxpy(long long n, int m, const VT* __restrict__ V, long long ldv, const double* __restrict__ h,
                                                   WT* __restrict__ w, const float* __restrict__ Vlo = nullptr) {
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double s = (double)w[k];
    if (Vlo) for (int i = 0; i < m; i++) s -= h[i] * ((double)V[(long long)i * ldv + k] + (double)Vlo[(long long)i * ldv + k]);
    else for (int i = 0; i < m; i++) s -= h[i] * (double)V[(long long)i * ldv + k];
    w[k] = (WT)s;
}
// The reduce-scatter that ends a step of k_multidot2 and k_multidot2w: the wave's 8 sums acc[2 ii + r] (basis vector i0 + ii against
// right-hand side r) end up one per lane group g = lane >> 3, whose first lane stores it to partial[(r K + i) nbw + slot].
// (g comes from the caller, which computes it before its loads as it always did: derived from lane in here, it costs the
// k_multidot2w<2 | 4> instantiations one more SGPR each.)
__device__ __forceinline__ void multidot2_reduce_scatter(const double (&acc)[8], int lane, int g, int i0, int K, double* __restrict__ partial, long long nbw,
                                                         long long slot) {
    double a4[4], a2[2], a1;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const double snd = (g & 4) ? acc[i] : acc[i + 4], keep = (g & 4) ? acc[i + 4] : acc[i];
        a4[i] = keep + __shfl_xor(snd, 32, 64);
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const double snd = (g & 2) ? a4[i] : a4[i + 2], keep = (g & 2) ? a4[i + 2] : a4[i];
        a2[i] = keep + __shfl_xor(snd, 16, 64);
    }
    {
        const double snd = (g & 1) ? a2[0] : a2[1], keep = (g & 1) ? a2[1] : a2[0];
        a1 = keep + __shfl_xor(snd, 8, 64);
    }
    a1 += __shfl_xor(a1, 1, 64);
    a1 += __shfl_xor(a1, 2, 64);
    a1 += __shfl_xor(a1, 4, 64);  // lane group g: the wave's sum number g = 2 ii + r
    const int i = i0 + (g >> 1);
    if ((lane & 7) == 0 && i < K) partial[((long long)(g & 1) * K + i) * nbw + slot] = a1;
}
// Two right-hand sides against K basis vectors in ONE pass over the basis (the fused inner products of the delayed
// re-orthogonalisation, gmres_iter_dcgs2): partial[(r K + i) nbw + slot] = this wave's part of V_i . (r == 0 ? u : v).
// A thread keeps MD2_ROWS rows of u and v in registers (16: 5.9 TB/s, 8: 5.6, 4: 4.7 on synthetic vectors, tools/orth_bench.py); four basis vectors at a time give 8 sums per lane, which one
// reduce-scatter over the wave (10 exchanges for 8 sums instead of 48) leaves in the 8 lane groups.
#ifndef MD2_ROWS
#define MD2_ROWS 16
#endif
template <int ROWS, bool FULL, class QT, class VT>
__device__ __forceinline__ void multidot2_body(long long n, int K, const QT* __restrict__ V, long long ldv, const VT* __restrict__ u,
                                               const double* __restrict__ v, double* __restrict__ partial, long long nbw) {
    const int lane = threadIdx.x & 63, g = lane >> 3;
    const long long base = (long long)blockIdx.x * (256 * ROWS) + threadIdx.x;
    const long long slot = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    double ur[ROWS], vr[ROWS];
#pragma unroll
    for (int t = 0; t < ROWS; t++) {
        const long long k = FULL ? base + 256 * t : min(base + 256 * t, n - 1);  // clamped loads, masked below: no branches
        const double m = (FULL || base + 256 * t < n) ? 1.0 : 0.0;
        ur[t] = m * (double)u[k];
        vr[t] = m * v[k];
    }
    for (int i0 = 0; i0 < K; i0 += 4) {
        double acc[8], x[4][ROWS];
        // all 4 x ROWS loads are issued before the first use (written as two loops: the scheduler otherwise trades the
        // loads in flight for registers and waits after every load)
#pragma unroll
        for (int ii = 0; ii < 4; ii++) {
            const QT* vi = V + (long long)min(i0 + ii, K - 1) * ldv;
#pragma unroll
            for (int t = 0; t < ROWS; t++) x[ii][t] = (double)vi[FULL ? base + 256 * t : min(base + 256 * t, n - 1)];  // ur, vr are zero beyond n
        }
#pragma unroll
        for (int ii = 0; ii < 4; ii++) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int t = 0; t < ROWS; t++) {
                a += x[ii][t] * ur[t];
                b += x[ii][t] * vr[t];
            }
            acc[2 * ii] = a;
            acc[2 * ii + 1] = b;
        }
        multidot2_reduce_scatter(acc, lane, g, i0, K, partial, nbw, slot);
    }
}
template <int ROWS, class QT, class VT>
__global__ __launch_bounds__(256) void k_multidot2(long long n, int K, const QT* __restrict__ V, long long ldv, const VT* __restrict__ u,
                                                   const double* __restrict__ v, double* __restrict__ partial, long long nbw) {
    if ((long long)(blockIdx.x + 1) * (256 * ROWS) <= n) multidot2_body<ROWS, true, QT, VT>(n, K, V, ldv, u, v, partial, nbw);
    else multidot2_body<ROWS, false, QT, VT>(n, K, V, ldv, u, v, partial, nbw);
}
// The fused update of the delayed re-orthogonalisation, one pass over the basis: with Q = the j final vectors, u = slot j
// (projected once), v = the operator applied to u:   q_j = (u - Q s) / alpha  -> slot j,
//                                                     u' = (v - gamma u - Q c) / alpha -> slot j + 1
#ifndef DCGS2_UNROLL
#define DCGS2_UNROLL 4
#endif
#ifndef DCGS2_RPT
#define DCGS2_RPT 2
#endif
template <int UNROLL, int RPT, class VT>
__global__ __launch_bounds__(256) void k_dcgs2_update(long long n, int j, VT* __restrict__ V, long long ldv, const double* __restrict__ sc,
                                                      double gamma, double ralpha, const double* __restrict__ v, float* __restrict__ Vlo = nullptr) {
    const long long k0 = ((long long)blockIdx.x * RPT) * blockDim.x + threadIdx.x;  // rows k0 + r * blockDim.x
    const double* s = sc;
    const double* c = sc + j;
    double as[RPT], ac[RPT];
    long long kk[RPT];
#pragma unroll
    for (int r = 0; r < RPT; r++) { as[r] = 0.0; ac[r] = 0.0; kk[r] = min(k0 + (long long)r * blockDim.x, n - 1); }
    int i = 0;
    for (; i + UNROLL <= j; i += UNROLL) {
        double q[UNROLL][RPT];
#pragma unroll
        for (int t = 0; t < UNROLL; t++)
#pragma unroll
            for (int r = 0; r < RPT; r++) q[t][r] = (double)V[(long long)(i + t) * ldv + kk[r]];
        if (Vlo) {
#pragma unroll
            for (int t = 0; t < UNROLL; t++)
#pragma unroll
                for (int r = 0; r < RPT; r++) q[t][r] += (double)Vlo[(long long)(i + t) * ldv + kk[r]];
        }
#pragma unroll
        for (int t = 0; t < UNROLL; t++)
#pragma unroll
            for (int r = 0; r < RPT; r++) { as[r] += s[i + t] * q[t][r]; ac[r] += c[i + t] * q[t][r]; }
    }
    for (; i < j; i++)
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            const double q = (double)V[(long long)i * ldv + kk[r]] + (Vlo ? (double)Vlo[(long long)i * ldv + kk[r]] : 0.0);
            as[r] += s[i] * q; ac[r] += c[i] * q;
        }
#pragma unroll
    for (int r = 0; r < RPT; r++) {
        const long long k = k0 + (long long)r * blockDim.x;
        if (k >= n) continue;
        const double u = (double)V[(long long)j * ldv + k] + (Vlo ? (double)Vlo[(long long)j * ldv + k] : 0.0);
        const double qj = (u - as[r]) * ralpha, un = (v[k] - gamma * u - ac[r]) * ralpha;
        const VT qh = (VT)qj, uh = (VT)un;
        V[(long long)j * ldv + k] = qh;
        V[(long long)(j + 1) * ldv + k] = uh;
        if (Vlo) { Vlo[(long long)j * ldv + k] = (float)(qj - (double)qh); Vlo[(long long)(j + 1) * ldv + k] = (float)(un - (double)uh); }
    }
}
// ---- 16-byte-load variants of the two kernels above for the float basis (fp32 and split storage) -------------------------------
// A lane owns groups of 4 consecutive rows and reads the hi (and lo) floats of a group as ONE 16-byte load: 1 KiB per wave
// instruction, a quarter of the load instructions of the one-dword-per-lane kernels.  The vector's start is uniform and stepped by
// ldv from vector to vector; the lane's part of the address is a 32-bit byte offset computed once (n < 2^30).  A workgroup whose
// rows all exist (FULL) uses the 16-byte loads and stores; the last one goes element by element with clamped loads (row n - 1 of the
// same vector: real data, never the padding behind row n) and masked sums / stores.  They need 16-byte aligned V, Vlo, u, v and
// ldv % 4 == 0 (orth_wide_ok); everything else runs the kernels above.  Sums in fp64 as above; only the order of the rows differs.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
template <bool FULL, bool NT>
__device__ __forceinline__ f32x4 ld_group(const float* __restrict__ vec, const unsigned (&bo)[4]) {
    const char* b = reinterpret_cast<const char*>(vec);
    if (FULL) {
        const f32x4* p = reinterpret_cast<const f32x4*>(b + bo[0]);
        return NT ? __builtin_nontemporal_load(p) : *p;
    }
    f32x4 r;
    r.x = *reinterpret_cast<const float*>(b + bo[0]);
    r.y = *reinterpret_cast<const float*>(b + bo[1]);
    r.z = *reinterpret_cast<const float*>(b + bo[2]);
    r.w = *reinterpret_cast<const float*>(b + bo[3]);
    return r;
}
// byte offsets of the 4 rows of the group that starts at row k (clamped to row n - 1 unless FULL)
template <bool FULL>
__device__ __forceinline__ void group_offsets(long long k, long long n, unsigned (&bo)[4]) {
#pragma unroll
    for (int e = 0; e < 4; e++) bo[e] = (unsigned)((FULL ? k + e : min(k + e, n - 1)) * 4);
}
// R4 groups of 4 rows per lane (group t of a lane starts at row 4 (256 (R4 blockIdx + t) + threadIdx)); partial sums as k_multidot2
template <int R4, bool FULL, bool NT>
__device__ __forceinline__ void multidot2w_body(long long n, int K, const float* __restrict__ V, long long ldv, const float* __restrict__ u,
                                                const double* __restrict__ v, double* __restrict__ partial, long long nbw) {
    const int lane = threadIdx.x & 63, g = lane >> 3;
    const long long base = ((long long)blockIdx.x * (256 * R4) + threadIdx.x) * 4;
    const long long slot = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    unsigned bo[R4][4];
    float ur[R4][4];
    double vr[R4][4];
#pragma unroll
    for (int t = 0; t < R4; t++) {
        const long long k = base + 1024LL * t;
        group_offsets<FULL>(k, n, bo[t]);
        const f32x4 uu = ld_group<FULL, false>(u, bo[t]);
        ur[t][0] = uu.x; ur[t][1] = uu.y; ur[t][2] = uu.z; ur[t][3] = uu.w;
        if (FULL) {
            const f64x2 a = *reinterpret_cast<const f64x2*>(v + k), b = *reinterpret_cast<const f64x2*>(v + k + 2);
            vr[t][0] = a.x; vr[t][1] = a.y; vr[t][2] = b.x; vr[t][3] = b.y;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const bool in = k + e < n;
                vr[t][e] = in ? v[min(k + e, n - 1)] : 0.0;
                ur[t][e] = in ? ur[t][e] : 0.f;
            }
        }
    }
    const float* v0 = V;  // start of vector i0 (uniform)
    for (int i0 = 0; i0 < K; i0 += 4, v0 += 4 * ldv) {
        f32x4 x[4][R4];
        double acc[8];
        // all 4 x R4 loads are issued before the first use (two loops, as in multidot2_body)
#pragma unroll
        for (int ii = 0; ii < 4; ii++) {
            const float* vi = v0 + (long long)min(ii, K - 1 - i0) * ldv;  // beyond K - 1: vector K - 1 again, its sums are not stored
#pragma unroll
            for (int t = 0; t < R4; t++) x[ii][t] = ld_group<FULL, NT>(vi, bo[t]);
        }
#pragma unroll
        for (int ii = 0; ii < 4; ii++) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int t = 0; t < R4; t++) {
                const double x0 = (double)x[ii][t].x, x1 = (double)x[ii][t].y, x2 = (double)x[ii][t].z, x3 = (double)x[ii][t].w;
                a += x0 * (double)ur[t][0]; b += x0 * vr[t][0];
                a += x1 * (double)ur[t][1]; b += x1 * vr[t][1];
                a += x2 * (double)ur[t][2]; b += x2 * vr[t][2];
                a += x3 * (double)ur[t][3]; b += x3 * vr[t][3];
            }
            acc[2 * ii] = a;
            acc[2 * ii + 1] = b;
        }
        multidot2_reduce_scatter(acc, lane, g, i0, K, partial, nbw, slot);
    }
}
template <int R4, bool NT>
__global__ __launch_bounds__(256) void k_multidot2w(long long n, int K, const float* __restrict__ V, long long ldv, const float* __restrict__ u,
                                                    const double* __restrict__ v, double* __restrict__ partial, long long nbw) {
    if ((long long)(blockIdx.x + 1) * (1024 * R4) <= n) multidot2w_body<R4, true, NT>(n, K, V, ldv, u, v, partial, nbw);
    else multidot2w_body<R4, false, NT>(n, K, V, ldv, u, v, partial, nbw);
}
// the fused update with RPT4 groups of 4 rows per lane and UNROLL basis vectors (hi and lo: 2 x UNROLL x RPT4 16-byte loads) in flight
template <int UNROLL, int RPT4, bool FULL, bool NT>
__device__ __forceinline__ void dcgs2w_body(long long n, int j, float* __restrict__ V, long long ldv, const double* __restrict__ sc, double gamma,
                                            double ralpha, const double* __restrict__ v, float* __restrict__ Vlo) {
    const long long base = ((long long)blockIdx.x * (256 * RPT4) + threadIdx.x) * 4;
    const double* s = sc;
    const double* c = sc + j;
    unsigned bo[RPT4][4];
    double as[RPT4][4], ac[RPT4][4];
#pragma unroll
    for (int r = 0; r < RPT4; r++) {
        group_offsets<FULL>(base + 1024LL * r, n, bo[r]);
#pragma unroll
        for (int e = 0; e < 4; e++) { as[r][e] = 0.0; ac[r][e] = 0.0; }
    }
    const float* h0 = V;    // start of vector i (uniform), hi and lo
    const float* l0 = Vlo;
    for (int i = 0; i < j; i += UNROLL, h0 += UNROLL * ldv, l0 += (Vlo ? UNROLL * ldv : 0)) {
        f32x4 qh[UNROLL][RPT4], ql[UNROLL][RPT4];
        // beyond j - 1: vector j - 1 again with zero coefficients (never slot j, which this kernel writes)
#pragma unroll
        for (int t = 0; t < UNROLL; t++) {
            const float* hv = h0 + (long long)min(t, j - 1 - i) * ldv;
#pragma unroll
            for (int r = 0; r < RPT4; r++) qh[t][r] = ld_group<FULL, NT>(hv, bo[r]);
        }
        if (Vlo) {
#pragma unroll
            for (int t = 0; t < UNROLL; t++) {
                const float* lv = l0 + (long long)min(t, j - 1 - i) * ldv;
#pragma unroll
                for (int r = 0; r < RPT4; r++) ql[t][r] = ld_group<FULL, NT>(lv, bo[r]);
            }
        }
#pragma unroll
        for (int t = 0; t < UNROLL; t++) {
            const bool in = i + t < j;
            const double st = in ? s[min(i + t, j - 1)] : 0.0, ct = in ? c[min(i + t, j - 1)] : 0.0;
#pragma unroll
            for (int r = 0; r < RPT4; r++) {
                double q[4] = {(double)qh[t][r].x, (double)qh[t][r].y, (double)qh[t][r].z, (double)qh[t][r].w};
                if (Vlo) { q[0] += (double)ql[t][r].x; q[1] += (double)ql[t][r].y; q[2] += (double)ql[t][r].z; q[3] += (double)ql[t][r].w; }
#pragma unroll
                for (int e = 0; e < 4; e++) { as[r][e] += st * q[e]; ac[r][e] += ct * q[e]; }
            }
        }
    }
    float* uh = V + (long long)j * ldv;
    float* nh = uh + ldv;
    float* ul = Vlo ? Vlo + (long long)j * ldv : nullptr;
    float* nl = Vlo ? ul + ldv : nullptr;
#pragma unroll
    for (int r = 0; r < RPT4; r++) {
        const long long k = base + 1024LL * r;
        if (k >= n) continue;
        const f32x4 u4 = ld_group<FULL, false>(uh, bo[r]);
        double u[4] = {(double)u4.x, (double)u4.y, (double)u4.z, (double)u4.w}, vv[4];
        if (Vlo) {
            const f32x4 l4 = ld_group<FULL, false>(ul, bo[r]);
            u[0] += (double)l4.x; u[1] += (double)l4.y; u[2] += (double)l4.z; u[3] += (double)l4.w;
        }
        if (FULL) {
            const f64x2 a = *reinterpret_cast<const f64x2*>(v + k), b = *reinterpret_cast<const f64x2*>(v + k + 2);
            vv[0] = a.x; vv[1] = a.y; vv[2] = b.x; vv[3] = b.y;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) vv[e] = v[min(k + e, n - 1)];
        }
        float qh[4], qlo[4], nhh[4], nlo[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double qj = (u[e] - as[r][e]) * ralpha, un = (vv[e] - gamma * u[e] - ac[r][e]) * ralpha;
            qh[e] = (float)qj; nhh[e] = (float)un;
            qlo[e] = (float)(qj - (double)qh[e]); nlo[e] = (float)(un - (double)nhh[e]);
        }
        if (FULL) {
            *reinterpret_cast<f32x4*>(uh + k) = f32x4{qh[0], qh[1], qh[2], qh[3]};
            *reinterpret_cast<f32x4*>(nh + k) = f32x4{nhh[0], nhh[1], nhh[2], nhh[3]};
            if (Vlo) {
                *reinterpret_cast<f32x4*>(ul + k) = f32x4{qlo[0], qlo[1], qlo[2], qlo[3]};
                *reinterpret_cast<f32x4*>(nl + k) = f32x4{nlo[0], nlo[1], nlo[2], nlo[3]};
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (k + e >= n) continue;
                uh[k + e] = qh[e]; nh[k + e] = nhh[e];
                if (Vlo) { ul[k + e] = qlo[e]; nl[k + e] = nlo[e]; }
            }
        }
    }
}
template <int UNROLL, int RPT4, bool NT>
__global__ __launch_bounds__(256) void k_dcgs2w_update(long long n, int j, float* __restrict__ V, long long ldv, const double* __restrict__ sc,
                                                       double gamma, double ralpha, const double* __restrict__ v, float* __restrict__ Vlo) {
    if ((long long)(blockIdx.x + 1) * (1024 * RPT4) <= n) dcgs2w_body<UNROLL, RPT4, true, NT>(n, j, V, ldv, sc, gamma, ralpha, v, Vlo);
    else dcgs2w_body<UNROLL, RPT4, false, NT>(n, j, V, ldv, sc, gamma, ralpha, v, Vlo);
}
// y = sum_i c_i V_i
template <class VT>
__global__ __launch_bounds__(256) void k_lincomb(long long n, int m, const VT* __restrict__ V, long long ldv, const double* __restrict__ c,
                                                 double* __restrict__ y, const float* __restrict__ Vlo = nullptr) {
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    double s = 0.0;
    if (Vlo) for (int i = 0; i < m; i++) s += c[i] * ((double)V[(long long)i * ldv + k] + (double)Vlo[(long long)i * ldv + k]);
    else for (int i = 0; i < m; i++) s += c[i] * (double)V[(long long)i * ldv + k];
    y[k] = s;
}
// y = a x; xlo: x is stored split (x = x + xlo); ylo: y is stored split (y = (TO) value, ylo = the fp32 rest)
template <class TI, class TO>
__global__ void k_scale_to(long long n, double a, const TI* __restrict__ x, TO* __restrict__ y, const float* __restrict__ xlo = nullptr,
                           float* __restrict__ ylo = nullptr) {
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double val = a * ((double)x[k] + (xlo ? (double)xlo[k] : 0.0));
    const TO yh = (TO)val;
    y[k] = yh;
    if (ylo) ylo[k] = (float)(val - (double)yh);
}
// ---- launch helpers of the Krylov vector kernels --------------------------------------------------------------------------
// The one place that holds the grid arithmetic of these kernels: they take (stream, n, ...) and no solver handle, so that the
// solver (gmres_iter_t, gmres_iter_dcgs2, DrDeviceOps) and the test-only entries das_debug_krylov_* run the SAME launches.
static inline size_t multidot_partial_size(long long n, int m) { return (size_t)(m + 1) * nblk(n, MD_CHUNK); }
// out[0..m) = V^T w, out[m] = w.w
template <class VT>
static void launch_multidot(hipStream_t st, long long n, int m, const VT* V, long long ldv, const double* w, double* partial, double* out) {
    const int nb = nblk(n, MD_CHUNK);
    hipLaunchKernelGGL(k_multidot, dim3(nb), dim3(256), 0, st, n, m, V, ldv, w, partial, nb);
    hipLaunchKernelGGL(k_reduce, dim3(m + 1), dim3(256), 0, st, nb, (const double*)partial, out);
}
template <int ROWS>
static inline long long multidot2_nbw(long long n) { return 4LL * nblk(n, 256 * ROWS); }
// Shapes of the 16-byte-load kernels (k_multidot2w, k_dcgs2w_update) and whether the launch helpers pick them for an eligible
// float basis.  MEASURED ON THE FLOAT INSTANTIATIONS (split layout, n = 16 172 600, K = 150 and 352) with das_debug_orth_bench_split /
// tools/orth_bench.py --split - not inherited from the fp64 shapes above; the table is in profiles/orth_wide_loads_split_basis.md.
// At K = 352: inner products 3.81 ms (4.30 with k_multidot2<16, float>), non-temporal loads 0.4 ms better than plain ones (u, v stay in
// the cache); update 7.67 ms (8.95 with k_dcgs2_update<4, 2, float>), plain loads better than non-temporal ones.
#ifndef MD2W_R4
#define MD2W_R4 4  // groups of 4 rows per lane of the inner products (16 rows: 184 VGPRs, 2 waves per SIMD)
#endif
#ifndef MD2W_NT
#define MD2W_NT 1  // non-temporal loads of the basis stream in the inner products
#endif
#ifndef DCGS2W_UNROLL
#define DCGS2W_UNROLL 4  // basis vectors in flight in the update
#endif
#ifndef DCGS2W_RPT4
#define DCGS2W_RPT4 2  // groups of 4 rows per lane of the update (8 rows x 4 vectors x hi, lo: 220 VGPRs, 2 waves per SIMD)
#endif
#ifndef DCGS2W_NT
#define DCGS2W_NT 0  // non-temporal loads of the basis stream in the update
#endif
#ifndef ORTH_WIDE_DEFAULT
#define ORTH_WIDE_DEFAULT 1
#endif
static int g_orth_wide = ORTH_WIDE_DEFAULT;  // das_debug_set_orth_wide: the tests and the timing tool run both paths of one build
// the 16-byte path of the float basis: every pointer 16-byte aligned, vectors a multiple of 16 bytes apart, 32-bit byte offsets in a vector
static inline bool orth_wide_ok(long long n, const void* V, const void* Vlo, long long ldv, const void* u, const void* v) {
    return n >= 4 && n < (1LL << 30) && (ldv & 3) == 0 && ((((uintptr_t)V | (uintptr_t)Vlo | (uintptr_t)u | (uintptr_t)v) & 15) == 0);
}
static inline long long multidot2w_nbw(long long n, int r4) { return 4LL * nblk(n, 1024 * r4); }
static inline size_t multidot2_partial_size(long long n, int K) {
    return (size_t)2 * K * (size_t)std::max(multidot2_nbw<MD2_ROWS>(n), multidot2w_nbw(n, MD2W_R4));
}
// the inner-product pass alone (the tuning hook times it for several ROWS)
template <int ROWS, class VT>
static void launch_multidot2_pass(hipStream_t st, long long n, int K, const VT* V, long long ldv, const VT* u, const double* v, double* partial) {
    hipLaunchKernelGGL((k_multidot2<ROWS, VT, VT>), dim3(nblk(n, 256 * ROWS)), dim3(256), 0, st, n, K, V, ldv, u, v, partial, multidot2_nbw<ROWS>(n));
}
// out[0..K) = V^T u, out[K..2K) = V^T v
template <int R4, bool NT>
static void launch_multidot2w_pass(hipStream_t st, long long n, int K, const float* V, long long ldv, const float* u, const double* v, double* partial) {
    hipLaunchKernelGGL((k_multidot2w<R4, NT>), dim3(nblk(n, 1024 * R4)), dim3(256), 0, st, n, K, V, ldv, u, v, partial, multidot2w_nbw(n, R4));
}
// the one-dword-per-lane update alone, whatever the basis is eligible for (the tuning hook times it next to the wide one)
template <int UNROLL, int RPT, class VT>
static void launch_dcgs2_update_pass(hipStream_t st, long long n, int j, VT* V, long long ldv, const double* sc, double gamma, double ralpha,
                                     const double* v, float* Vlo) {
    hipLaunchKernelGGL((k_dcgs2_update<UNROLL, RPT, VT>), dim3(nblk(n, 256 * RPT)), dim3(256), 0, st, n, j, V, ldv, sc, gamma, ralpha, v, Vlo);
}
template <int UNROLL, int RPT4, bool NT>
static void launch_dcgs2w_update(hipStream_t st, long long n, int j, float* V, long long ldv, const double* sc, double gamma, double ralpha,
                                 const double* v, float* Vlo) {
    hipLaunchKernelGGL((k_dcgs2w_update<UNROLL, RPT4, NT>), dim3(nblk(n, 1024 * RPT4)), dim3(256), 0, st, n, j, V, ldv, sc, gamma, ralpha, v, Vlo);
}
template <class VT>
static void launch_multidot2(hipStream_t st, long long n, int K, const VT* V, long long ldv, const VT* u, const double* v, double* partial, double* out) {
    if constexpr (std::is_same<VT, float>::value) {
        if (g_orth_wide && orth_wide_ok(n, V, nullptr, ldv, u, v)) {
            launch_multidot2w_pass<MD2W_R4, MD2W_NT != 0>(st, n, K, V, ldv, u, v, partial);
            hipLaunchKernelGGL(k_reduce, dim3(2 * K), dim3(256), 0, st, (int)multidot2w_nbw(n, MD2W_R4), (const double*)partial, out);
            return;
        }
    }
    launch_multidot2_pass<MD2_ROWS, VT>(st, n, K, V, ldv, u, v, partial);
    hipLaunchKernelGGL(k_reduce, dim3(2 * K), dim3(256), 0, st, (int)multidot2_nbw<MD2_ROWS>(n), (const double*)partial, out);
}
template <int UNROLL, int RPT, class VT>
static void launch_dcgs2_update(hipStream_t st, long long n, int j, VT* V, long long ldv, const double* sc, double gamma, double ralpha, const double* v,
                                float* Vlo) {
    if constexpr (std::is_same<VT, float>::value) {
        if (g_orth_wide && orth_wide_ok(n, V, Vlo, ldv, nullptr, v)) {
            launch_dcgs2w_update<DCGS2W_UNROLL, DCGS2W_RPT4, DCGS2W_NT != 0>(st, n, j, V, ldv, sc, gamma, ralpha, v, Vlo);
            return;
        }
    }
    launch_dcgs2_update_pass<UNROLL, RPT, VT>(st, n, j, V, ldv, sc, gamma, ralpha, v, Vlo);
}
template <class VT, class WT>
static void launch_multiaxpy(hipStream_t st, long long n, int m, const VT* V, long long ldv, const double* h, WT* w, const float* Vlo) {
    hipLaunchKernelGGL(k_multiaxpy, dim3(nblk(n, 256)), dim3(256), 0, st, n, m, V, ldv, h, w, Vlo);
}
template <class VT>
static void launch_lincomb(hipStream_t st, long long n, int m, const VT* V, long long ldv, const double* c, double* y, const float* Vlo) {
    hipLaunchKernelGGL(k_lincomb, dim3(nblk(n, 256)), dim3(256), 0, st, n, m, V, ldv, c, y, Vlo);
}
template <class TI, class TO>
static void launch_scale_to(hipStream_t st, long long n, double a, const TI* x, TO* y, const float* xlo, float* ylo) {
    hipLaunchKernelGGL(k_scale_to, dim3(nblk(n, 256)), dim3(256), 0, st, n, a, x, y, xlo, ylo);
}

}  // namespace das

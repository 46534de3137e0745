// Coarse space of the two-level preconditioner (amd.pcCoarseAggregates, amd.pcCoarseMode): the kernels that assemble E = Z^T P Z, invert it,
// restrict / solve / prolong per apply and build the sparse A Z of the deflated mode, and the launch sequences the solver runs with them.
// In a header of their own so that the test-only entries of das_coarse_debug.hpp can run them without a solver handle.
#pragma once
#include <algorithm>
#include <vector>

#include "das_common.hpp"

namespace das {

// ---- two-level correction: piecewise-constant coarse space on one scalar cell field (the pressure) ---------------------
// The incomplete factorisation alone leaves the smooth pressure modes to the Krylov method: the iteration count of the
// adjoint solve grows linearly with the number of cells along the domain (measured ~4.2 x nx for the bench channels).  A
// Nicolaides-type coarse space - one unknown per aggregate of cells, acting on the p / pRes entries only - removes that
// growth: M^-1 = ILU^-1 + Z E^-1 Z^T (additive) or ILU^-1 (I - A Z E^-1 Z^T) + Z E^-1 Z^T (deflated, A-DEF1), with
// E = Z^T P Z assembled from jacPCMat on the device and inverted on the host (nAgg <= 2048).
// E[I][J] = sum of the field-block entries a_ij with i in aggregate I, j in aggregate J - DETERMINISTIC (the
// atomicAdd version summed in arrival order, so E - and with it every iterate - differed in the last bits from run to run):
// one workgroup per row aggregate I walks the rows of its cells in list order; thread t owns the target columns J = t (mod 256)
// and is the only one that ever adds to them (LDS row of nagg doubles), so every E[I][J] is summed in the same order every time.
// aggRow: aggregate of a ROW cell (owned and - multi-GPU, global coarse space - ghost cells), aggCol: aggregate of a COLUMN
// cell (owned residuals only: the matrix holds no other columns); cellsAll / aptrAll: the row cells sorted by aggregate.
__global__ __launch_bounds__(256) void k_coarse_assemble(int nagg, const long long* __restrict__ aptrAll, const int* __restrict__ cellsAll, long long N,
                                                         long long off, const long long* __restrict__ rp, const int* __restrict__ ci,
                                                         const double* __restrict__ v, const int* __restrict__ aggCol, double* __restrict__ E,
                                                         int transpose, double diagScale) {
    __shared__ double accs[2048];
    const int I = blockIdx.x, t = threadIdx.x;
    const long long q0 = aptrAll[I], q1 = aptrAll[I + 1];
    if (q0 == q1) return;  // no row cell of this aggregate on this rank: the row of E stays zero here
    for (int J = t; J < nagg; J += 256) accs[J] = 0.0;
    for (long long q = q0; q < q1; q++) {
        const long long c = cellsAll[q];
        const long long row = off + c;
        for (long long k = rp[row]; k < rp[row + 1]; k++) {
            const long long j = (long long)ci[k] - off;
            if (j < 0 || j >= N) continue;
            const int J = aggCol[j];
            if (J >= 0 && (J & 255) == t) accs[J] += (j == c) ? v[k] * diagScale : v[k];
        }
    }
    for (int J = t; J < nagg; J += 256) E[transpose ? (long long)J * nagg + I : (long long)I * nagg + J] = accs[J];
}
// dense inverse of the coarse operator by Gauss-Jordan with partial pivoting on the device (n <= 2048): per pivot column
// one single-workgroup kernel (pivot search, row swap, row scaling) and one elimination kernel (one workgroup per row)
__global__ __launch_bounds__(256) void k_gj_pivot(int n, int k, double* __restrict__ E, double* __restrict__ Inv, int* __restrict__ singular) {
    __shared__ double bv[256];
    __shared__ int bi[256];
    double best = -1.0;
    int br = k;
    for (int r = k + threadIdx.x; r < n; r += 256) { const double a = fabs(E[(long long)r * n + k]); if (a > best) { best = a; br = r; } }
    bv[threadIdx.x] = best; bi[threadIdx.x] = br;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o && (bv[threadIdx.x + o] > bv[threadIdx.x] || (bv[threadIdx.x + o] == bv[threadIdx.x] && bi[threadIdx.x + o] < bi[threadIdx.x]))) {
            bv[threadIdx.x] = bv[threadIdx.x + o]; bi[threadIdx.x] = bi[threadIdx.x + o];
        }
        __syncthreads();
    }
    const int pr = bi[0];
    if (!(bv[0] > 0.0)) { if (threadIdx.x == 0) *singular = 1; return; }
    const double ip = 1.0 / E[(long long)pr * n + k];
    __syncthreads();
    for (int q = threadIdx.x; q < n; q += 256) {
        const double ek = E[(long long)k * n + q], ep = E[(long long)pr * n + q];
        const double ik = Inv[(long long)k * n + q], ipr = Inv[(long long)pr * n + q];
        if (pr != k) { E[(long long)pr * n + q] = ek; Inv[(long long)pr * n + q] = ik; }
        E[(long long)k * n + q] = ep * ip;
        Inv[(long long)k * n + q] = ipr * ip;
    }
}
__global__ __launch_bounds__(256) void k_gj_elim(int n, int k, double* __restrict__ E, double* __restrict__ Inv) {
    const int r = blockIdx.x;
    if (r == k) return;
    __shared__ double fs;
    if (threadIdx.x == 0) fs = E[(long long)r * n + k];
    __syncthreads();
    const double f = fs;
    if (f == 0.0) return;
    for (int q = threadIdx.x; q < n; q += 256) {
        E[(long long)r * n + q] -= f * E[(long long)k * n + q];
        Inv[(long long)r * n + q] -= f * Inv[(long long)k * n + q];
    }
}
// t[I] = sum of r over the field entries of aggregate I (cells sorted by aggregate: deterministic, one workgroup each)
__global__ __launch_bounds__(256) void k_coarse_restrict(const long long* __restrict__ aptr, const int* __restrict__ cells, long long off,
                                                         const double* __restrict__ r, double* __restrict__ t) {  // t: first OWN aggregate
    __shared__ double red[4];
    const int I = blockIdx.x;
    double acc = 0.0;
    for (long long q = aptr[I] + threadIdx.x; q < aptr[I + 1]; q += 256) acc += r[off + cells[q]];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) t[I] = red[0] + red[1] + red[2] + red[3];
}
__global__ void k_coarse_solve(int nagg, const double* __restrict__ Einv, const double* __restrict__ t, double* __restrict__ u) {
    const int I = blockIdx.x * blockDim.x + threadIdx.x;
    if (I >= nagg) return;
    double acc = 0.0;
    for (int J = 0; J < nagg; J++) acc += Einv[(long long)I * nagg + J] * t[J];
    u[I] = acc;
}
// y[field entry of cell c] (+)= u[agg(c)]; `set`: y is zero elsewhere (the deflation vector), else accumulate
__global__ void k_coarse_prolong(long long N, long long n, long long off, const int* __restrict__ agg, const double* __restrict__ u,
                                 double* __restrict__ y, int set) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long c = i - off;
    const double add = (c >= 0 && c < N && agg[c] >= 0) ? u[agg[c]] : 0.0;
    y[i] = set ? add : y[i] + add;
}

// A Z for the deflated coarse mode: row i of the operator summed over the field-block columns of every aggregate.  One thread per
// row, entries in storage order (deterministic); a row whose field columns touch more than AZ_CAP aggregates sets `overflow` (the
// caller then keeps the full operator product).  pass 0: counts -> cnt[i]; pass 1: fills (ptr from the prefix sum of the counts)
constexpr int AZ_CAP = 64;  // (round 5: 12 overflowed on the wing - RCB boxes next to the wall are 4 cells thick spanwise, a 7-cell stencil meets 3 x 3 x 2 of them)
__global__ __launch_bounds__(256) void k_az_build(long long n, const long long* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ v,
                                                  long long N, long long off, const int* __restrict__ agg, int pass, int* __restrict__ cnt,
                                                  const long long* __restrict__ ptr, int* __restrict__ oa, double* __restrict__ ov, int* __restrict__ overflow) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int la[AZ_CAP];
    double ls[AZ_CAP];
    int m = 0;
    for (long long k = rp[i]; k < rp[i + 1]; k++) {
        const long long j = (long long)ci[k] - off;
        if (j < 0 || j >= N) continue;
        const int a = agg[j];
        if (a < 0) continue;
        int q = 0;
        while (q < m && la[q] != a) q++;
        if (q == m) {
            if (m == AZ_CAP) { *overflow = 1; continue; }
            la[m] = a; ls[m] = 0.0; m++;
        }
        ls[q] += v[k];
    }
    if (pass == 0) { cnt[i] = m; return; }
    const long long b = ptr[i];
    for (int q = 0; q < m; q++) { oa[b + q] = la[q]; ov[b + q] = ls[q]; }
}
// out = v - (A Z) u   (v == nullptr: out = (A Z) u - several ranks reduce the ghost rows before the subtraction)
__global__ __launch_bounds__(256) void k_az_apply(long long n, const long long* __restrict__ ptr, const int* __restrict__ oa, const double* __restrict__ ov,
                                                  const double* __restrict__ u, const double* __restrict__ v, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double acc = 0.0;
    for (long long k = ptr[i]; k < ptr[i + 1]; k++) acc += ov[k] * u[oa[k]];
    out[i] = v ? v[i] - acc : acc;
}

// ---- the launch sequences of the coarse space: the solver (das_device.hip) and the test-only entries (das_coarse_debug.hpp) run these ----
// the cells that belong to an aggregate (agg[c] in [0, nagg), -1: none) sorted by aggregate, cells of one aggregate in ascending order:
// aptr (nagg + 1 offsets), cells (aptr[nagg] cell ids)
static void coarse_sort_cells(long long N, int nagg, const int* agg, std::vector<long long>& aptr, std::vector<int>& cells) {
    aptr.assign((size_t)nagg + 1, 0);
    for (long long c = 0; c < N; c++) if (agg[c] >= 0) aptr[agg[c] + 1]++;
    for (int a = 0; a < nagg; a++) aptr[a + 1] += aptr[a];
    cells.resize((size_t)aptr[nagg]);
    std::vector<long long> pos(aptr.begin(), aptr.end() - 1);
    for (long long c = 0; c < N; c++) if (agg[c] >= 0) cells[pos[agg[c]]++] = (int)c;
}
// E (nagg x nagg, device) = 0, then k_coarse_assemble: one workgroup per row aggregate
static void coarse_assemble(int nagg, const long long* aptrAll, const int* cellsAll, long long N, long long off, const long long* rp, const int* ci, const double* v,
                            const int* aggCol, double* E, int transpose, double diagScale, hipStream_t st) {
    DAS_HIP(hipMemsetAsync(E, 0, (size_t)nagg * nagg * sizeof(double), st));
    hipLaunchKernelGGL(k_coarse_assemble, dim3(nagg), dim3(256), 0, st, nagg, aptrAll, cellsAll, N, off, rp, ci, v, aggCol, E, transpose, diagScale);
}
// Inv = E^-1 by Gauss-Jordan with partial pivoting (E is overwritten; E, Inv: n x n on the device, sing: one int on the device).
// Returns the singular flag: 1 = a pivot column without a nonzero (or with NaN only) - Inv then holds nothing of use.  Waits for the stream.
static int coarse_invert(int n, double* E, double* Inv, int* sing, hipStream_t st) {
    {
        std::vector<double> I0((size_t)n * n, 0.0);
        for (int i = 0; i < n; i++) I0[(size_t)i * n + i] = 1.0;
        DAS_HIP(hipMemcpy(Inv, I0.data(), I0.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    DAS_HIP(hipMemsetAsync(sing, 0, sizeof(int), st));
    for (int kk = 0; kk < n; kk++) {
        hipLaunchKernelGGL(k_gj_pivot, dim3(1), dim3(256), 0, st, n, kk, E, Inv, sing);
        hipLaunchKernelGGL(k_gj_elim, dim3(n), dim3(256), 0, st, n, kk, E, Inv);
    }
    int hs = 0;
    DAS_HIP(hipMemcpyAsync(&hs, sing, sizeof(int), hipMemcpyDeviceToHost, st));
    DAS_HIP(hipStreamSynchronize(st));
    return hs;
}
// t[aggOff + I] = Z^T r for the nagg aggregates of this rank, then u = Einv t over all naggG aggregates; `between` runs between the two
// launches (several ranks: the all-reduce of t)
template <class F>
static void coarse_restrict_solve(int nagg, const long long* aptr, const int* cells, long long off, const double* r, int naggG, int aggOff, const double* Einv,
                                  double* t, double* u, hipStream_t st, F&& between) {
    if (nagg > 0) hipLaunchKernelGGL(k_coarse_restrict, dim3(nagg), dim3(256), 0, st, aptr, cells, off, r, t + aggOff);
    between();
    hipLaunchKernelGGL(k_coarse_solve, dim3(nblk(naggG, 64)), dim3(64), 0, st, naggG, Einv, t, u);
}
static void coarse_restrict_solve(int nagg, const long long* aptr, const int* cells, long long off, const double* r, int naggG, int aggOff, const double* Einv,
                                  double* t, double* u, hipStream_t st) {
    coarse_restrict_solve(nagg, aptr, cells, off, r, naggG, aggOff, Einv, t, u, st, [] {});
}
// the sparse A Z of an n-row CSR operator: pass 0 (counts), the prefix sum on the host, pass 1 (fill).  anyOverflow(flag) -> flag agreed
// by all ranks (one rank: the flag itself).  Returns false - and runs no pass 1 - when a row touches more than AZ_CAP aggregates.
template <class F>
static bool coarse_az_build(long long n, const long long* rp, const int* ci, const double* v, long long N, long long off, const int* agg, DevBuf<int>& cnt,
                            DevBuf<long long>& ptr, DevBuf<int>& oa, DevBuf<double>& ov, long long& nnz, hipStream_t st, F&& anyOverflow) {
    DevBuf<int> ovf(1);
    if (cnt.n < (size_t)n) cnt.alloc((size_t)n);
    DAS_HIP(hipMemsetAsync(ovf.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_az_build, dim3(nblk(n, 256)), dim3(256), 0, st, n, rp, ci, v, N, off, agg, 0, cnt.p, (const long long*)nullptr, (int*)nullptr, (double*)nullptr,
                       ovf.p);
    DAS_HIP(hipStreamSynchronize(st));
    if (anyOverflow(ovf.to_host()[0])) return false;
    std::vector<int> h((size_t)n);
    cnt.download(h.data(), (size_t)n);
    std::vector<long long> hp((size_t)n + 1, 0);
    for (long long i = 0; i < n; i++) hp[i + 1] = hp[i] + h[i];
    nnz = hp[n];
    ptr.upload(hp);
    if (oa.n < (size_t)std::max<long long>(1, nnz)) oa.alloc((size_t)std::max<long long>(1, nnz));
    if (ov.n < (size_t)std::max<long long>(1, nnz)) ov.alloc((size_t)std::max<long long>(1, nnz));
    hipLaunchKernelGGL(k_az_build, dim3(nblk(n, 256)), dim3(256), 0, st, n, rp, ci, v, N, off, agg, 1, cnt.p, ptr.p, oa.p, ov.p, ovf.p);
    DAS_HIP(hipStreamSynchronize(st));
    return true;
}

}  // namespace das

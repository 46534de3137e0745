// Bodies of the test-only entries das_debug_idr_* (tests/test_gpu_idr_kernels.py): they upload the caller's arrays, run the launch
// helpers the IDR(s) solver runs (null stream) and download the result.  Nothing in the product path calls them.
#pragma once
#include "das_idr.hpp"
#include "das_krylov_debug.hpp"

namespace das {

static void idr_check_shape(const std::string& who, long long n, int s, long long ld) {
    DAS_CHECK(n > 0 && s >= 1 && s <= IDR_MAX_S, DAS_ERR_ARG, who + ": n > 0 and 1 to 8 columns");
    DAS_CHECK(ld >= n, DAS_ERR_ARG, who + ": leading dimension below n");
}
// P (s columns, ld apart) = the raw hash; device = 0: the host side of the hash, no GPU needed
static void debug_idr_shadow(long long n, int s, long long ld, unsigned seed, bool device, double* P) {
    if (!device) {
        for (int q = 0; q < s; q++) for (long long i = 0; i < n; i++) P[(size_t)q * ld + i] = idr_shadow_entry(seed, i, q);
        return;
    }
    const DevBuf<double> dP = krylov_up<double>(P, (size_t)s * ld);
    krylov_run([&] { launch_idr_shadow(0, n, s, seed, dP.p, ld); }, dP, P, (size_t)s * ld);
}
// y = a x + sum_{i < m} c_i V_i on V (m columns, ld apart, vlen entries); yoff >= 0: y = V + yoff (in place), else y is its own array of ylen entries
static void debug_idr_combine(long long n, int m, double a, const double* x, double* V, long long ld, long long vlen, const double* c, long long yoff, double* y,
                              long long ylen) {
    const DevBuf<double> dx = krylov_up<double>(x, n), dV = krylov_up<double>(V, (size_t)vlen), dc = krylov_up<double>(c, m);
    if (yoff >= 0) {
        krylov_run([&] { launch_idr_combine(0, n, m, a, dx.p, dV.p, ld, dc.p, dV.p + yoff); }, dV, V, (size_t)vlen);
        return;
    }
    const DevBuf<double> dy = krylov_up<double>(y, (size_t)ylen);
    krylov_run([&] { launch_idr_combine(0, n, m, a, dx.p, dV.p, ld, dc.p, dy.p); }, dy, y, (size_t)ylen);
    dV.download(V, (size_t)vlen);
}
// the fused step k on G, U (glen entries each, columns ld apart), r, x (vlen entries each); coef = [alpha (k); beta]; rr = r.r
static void debug_idr_biortho_step(long long n, int k, double* G, double* U, long long ld, long long glen, const double* coef, double* r, double* x, long long vlen,
                                   double* rr) {
    const DevBuf<double> dG = krylov_up<double>(G, (size_t)glen), dU = krylov_up<double>(U, (size_t)glen), dc = krylov_up<double>(coef, (size_t)k + 1);
    const DevBuf<double> dr = krylov_up<double>(r, (size_t)vlen), dx = krylov_up<double>(x, (size_t)vlen), partial(idr_partial_size(n, 1)), dout(1);
    krylov_run([&] { launch_idr_biortho_step(0, n, k, dG.p, dU.p, ld, dc.p, dr.p, dx.p, partial.p, dout.p); }, dout, rr, 1);
    dG.download(G, (size_t)glen); dU.download(U, (size_t)glen); dr.download(r, (size_t)vlen); dx.download(x, (size_t)vlen);
}
// the fused smoothing update on r, x (vlen entries each) with t, z (n) and P (s columns, ld apart, plen entries); out[0..s) = P^T r, out[s] = r.r
static void debug_idr_smooth_step(long long n, int s, double omega, double* r, const double* t, double* x, const double* z, long long vlen, double* P, long long ld,
                                  long long plen, double* out) {
    const DevBuf<double> dr = krylov_up<double>(r, (size_t)vlen), dx = krylov_up<double>(x, (size_t)vlen), dt = krylov_up<double>(t, n), dz = krylov_up<double>(z, n);
    const DevBuf<double> dP = krylov_up<double>(P, (size_t)plen), partial(idr_partial_size(n, s)), dout((size_t)s + 1);
    krylov_run([&] { launch_idr_smooth_step(0, n, s, omega, dr.p, dt.p, dx.p, dz.p, dP.p, ld, partial.p, dout.p); }, dout, out, (size_t)s + 1);
    dr.download(r, (size_t)vlen); dx.download(x, (size_t)vlen); dP.download(P, (size_t)plen);
}

}  // namespace das

// IDR(s), the short-recurrence Krylov solver of amd.krylovMethod "idrs": the shadow-space hash, the iteration written once over a small
// set of vector operations (idrs_loop<Ops>) and its host twin (IdrHostOps).  Host C++ only - no device, no solver handle, no global
// state: the CPU tier runs this very code (das_debug_idrs_host, das_debug_idr_cycle_host, das_debug_idr_shadow).
//
// ---- IDR(s) (opt-in: amd.krylovMethod "idrs"; van Gijzen and Sonneveld, ACM TOMS 38 (2011), Algorithm 2: "IDR(s) with biorthogonalisation") --
// Full GMRES keeps one basis vector per iteration and orthogonalises against all of them; the basis is what limits the mesh size on one
// GPU and the Gram-Schmidt passes are most of an iteration at depth.  IDR(s) forces the residuals into a sequence of nested subspaces
// G_{j+1} = (I - omega_j A)(G_j intersected with the null space of P^T) with a FIXED shadow space P (n x s): s + 1 operator products take
// the residual from G_j into G_{j+1}, and the work vectors are x, r, z, t, P, G, U - 3 s + O(1) of them whatever the iteration count.
// Right preconditioning: every direction is built as u = omega M^-1 v + U c and mapped by g = A u, so x += beta u needs no
// back-transformation and r stays the residual of the original system.  One cycle:
//   f = P^T r
//   for k = 0 .. s-1:  solve M[k:, k:] c = f[k:];  v = r - G[:, k:] c;  u_k = omega M^-1 v + U[:, k:] c;  g_k = A u_k
//                      biorthogonalise: alpha = M[:k, :k]^-1 (P^T g_k)[:k],  g_k -= G[:, :k] alpha,  u_k -= U[:, :k] alpha,
//                      M[k:, k] = P[:, k:]^T g_k;  beta = f_k / M[k, k];  r -= beta g_k;  x += beta u_k;  f[k+1:] -= beta M[k+1:, k]
//   smoothing step:    t = A M^-1 r;  omega = t.r / t.t, enlarged to 0.7 / rho of it when rho = |t.r| / (|t| |r|) < 0.7 ("maintaining
//                      convergence", Sleijpen and van der Vorst);  r -= omega t;  x += omega M^-1 r
// The published algorithm biorthogonalises g_k against p_0 .. p_{k-1} one after the other (k dependent inner products); here d = P^T g_k
// is taken in ONE pass and alpha follows by forward substitution with the lower triangular M = P^T G - the same numbers up to rounding
// (the CPU tier compares a cycle with the sequential form), one host synchronisation instead of k.  Vector passes of an inner step:
// v (s - k + 2), u_k (s - k + 2), P^T g_k (s + 1), the fused update (2 k + 8) <= 3 s + 13; of a smoothing step: s + 8.
// Safeguards (all here, so that the CPU tier tests them): the recurrence residual is never trusted - when it meets the target, and when
// the budget ends, b - A x is computed; a true residual above the target restarts from x with G = U = 0, M = I, omega = 1 and the next
// seed, and a restarted run that does not halve the true residual ends the solve on stagnation (reason 2, as the GMRES path); M[k, k]
// zero or non-finite, a vanishing t.t or omega restart with a new seed (nBreakdown); a non-finite residual ends the solve (reason 3).
// Every operator product - the true-residual ones included - is counted and bounded by maxIts, and leaves one entry in the history.
// At size it has been run once (profiles/README.md): on the 2 M-cell wing, whose GMRES residual history has a plateau of 250 iterations,
// IDR(4) did NOT converge inside the reference's 1000-product budget (true residual 2.2 |r0|, peaks of 1e3 |r0| on the way) - the option
// is for systems without such a plateau until that is understood.  Reference role: the reference (PETSc KSPGMRES through DALinearEqn.C)
// has no counterpart; the default stays GMRES.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "das_gmres_host.hpp"

#if defined(__HIPCC__)
#define DAS_IDR_HD __host__ __device__
#else
#define DAS_IDR_HD
#endif

namespace das {
constexpr int IDR_MAX_S = 8;

// entry (row, col) of the raw shadow space: a pure function of (seed, row, col) - a 64-bit mix (the finaliser of splitmix64) of the three
// counters, its upper 52 bits taken to a uniform value in (-1, 1).  Integer arithmetic, one exact conversion and exact scalings by powers of two:
// the device fill (k_idr_shadow) and the host twin give identical bits.
DAS_IDR_HD inline double idr_shadow_entry(unsigned seed, long long row, int col) {
    uint64_t z = (uint64_t)row * 0x9E3779B97F4A7C15ull + ((uint64_t)(unsigned)col << 40) * 0xD1B54A32D192ED03ull + ((uint64_t)seed + 1u) * 0x8CB92BA72F3D8DD7ull;
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double u = ((double)(z >> 12) + 0.5) * 0x1p-52;  // (0, 1): 2^-53 .. 1 - 2^-53
    return 2.0 * u - 1.0;
}

// reason: 0 tolerance met (true residual), 1 budget, 2 stagnation (a restarted run did not halve the true residual), 3 non-finite residual
struct IdrResult { long long its = 0; double res0 = 0, res = 0; int reason = 0, cycles = 0, nRestarts = 0, nBreakdown = 0; };

// The iteration itself.  Ops: shadow(s, seed) [P = the hash, columns orthonormalised]; reset_spaces() [G = U = 0]; project_r(f) [f[0..s) =
// P^T r]; inner_vec(k, c, omega) [v = r - G[:, k:] c, u_k = omega M^-1 v + U[:, k:] c, g_k = A u_k; c holds s - k entries];
// dots_g(k, d, gg) [d[0..s) = P^T g_k, gg = g_k.g_k]; biortho_step(k, alpha, beta) [g_k -= G[:, :k] alpha, u_k -= U[:, :k] alpha,
// r -= beta g_k, x += beta u_k; returns r.r]; smooth_vec() [z = M^-1 r, t = A z]; dots_t(tr, tt) [t.r, t.t];
// smooth_step(omega, f) [r -= omega t, x += omega z, f = P^T r; returns r.r]; true_residual() [r = b - A x, returns |r|].
// On entry r holds the true residual of the start vector and beta0 its norm, which hist already ends with.
template <class Ops>
inline IdrResult idrs_loop(Ops& ops, int s, unsigned seed, double beta0, double target, long long maxIts, std::vector<double>& hist) {
    IdrResult out;
    out.res0 = out.res = beta0;
    if (!std::isfinite(beta0)) { out.reason = 3; return out; }
    if (beta0 <= target) return out;
    out.reason = 1;
    if (maxIts < 2) return out;  // no room for one step and the product that confirms it
    const long long recIts = maxIts - 1;  // products the recurrence may spend: the last one belongs to the closing true residual
    double M[IDR_MAX_S][IDR_MAX_S], f[IDR_MAX_S + 1], c[IDR_MAX_S], d[IDR_MAX_S + 1], alpha[IDR_MAX_S + 1];
    double omega = 1.0, rn = beta0, runStart = beta0;
    bool fresh = true, restartedRun = false;
    for (;;) {
        if (fresh) {
            ops.shadow(s, seed);
            ops.reset_spaces();
            for (int i = 0; i < s; i++) for (int j = 0; j < s; j++) M[i][j] = i == j ? 1.0 : 0.0;
            omega = 1.0;
            ops.project_r(f);
            fresh = false;
        }
        bool close = false, breakdown = false;
        for (int k = 0; k < s && !close; k++) {
            for (int i = k; i < s; i++) {  // M[k:, k:] c = f[k:], M lower triangular
                double a = f[i];
                for (int j = k; j < i; j++) a -= M[i][j] * c[j - k];
                c[i - k] = a / M[i][i];
            }
            bool ok = true;
            for (int i = 0; i < s - k; i++) ok = ok && std::isfinite(c[i]);
            if (!ok) { breakdown = close = true; break; }
            ops.inner_vec(k, c, omega);
            out.its++;
            double gg = 0.0;
            ops.dots_g(k, d, gg);
            for (int i = 0; i < k; i++) {  // alpha = M[:k, :k]^-1 d[:k]
                double a = d[i];
                for (int j = 0; j < i; j++) a -= M[i][j] * alpha[j];
                alpha[i] = a / M[i][i];
            }
            for (int i = k; i < s; i++) {
                double a = d[i];
                for (int j = 0; j < k; j++) a -= M[i][j] * alpha[j];
                M[i][k] = a;
            }
            if (!std::isfinite(gg)) { out.reason = 3; hist.push_back(gg); out.res = gg; return out; }
            if (!(std::isfinite(M[k][k]) && M[k][k] != 0.0)) { hist.push_back(rn); breakdown = close = true; break; }
            const double beta = f[k] / M[k][k];
            const double rr = ops.biortho_step(k, alpha, beta);
            f[k] = 0.0;
            for (int i = k + 1; i < s; i++) f[i] -= beta * M[i][k];
            rn = std::sqrt(std::max(rr, 0.0));
            hist.push_back(std::isfinite(rr) ? rn : rr);
            if (!std::isfinite(rr)) { out.reason = 3; out.res = rr; return out; }
            if (rn <= target || out.its >= recIts) close = true;
        }
        if (!close) {  // the smoothing step into the next subspace
            ops.smooth_vec();
            out.its++;
            double tr = 0.0, tt = 0.0;
            ops.dots_t(tr, tt);
            if (!std::isfinite(tr) || !std::isfinite(tt)) { out.reason = 3; hist.push_back(tt); out.res = tt; return out; }
            if (tt > 0.0 && tr != 0.0) {
                omega = tr / tt;
                const double rho = std::fabs(tr) / (std::sqrt(tt) * rn);
                if (rho < 0.7) omega *= 0.7 / rho;
            } else omega = 0.0;
            if (!(std::isfinite(omega) && omega != 0.0)) { hist.push_back(rn); breakdown = close = true; }
            else {
                const double rr = ops.smooth_step(omega, f);
                rn = std::sqrt(std::max(rr, 0.0));
                hist.push_back(std::isfinite(rr) ? rn : rr);
                if (!std::isfinite(rr)) { out.reason = 3; out.res = rr; return out; }
                out.cycles++;
                if (rn <= target || out.its >= recIts) close = true;
            }
        }
        if (!close) continue;
        // the recurrence met the target, broke down or used the budget: what counts is b - A x
        if (breakdown) out.nBreakdown++;
        const double tn = ops.true_residual();
        out.its++;
        hist.push_back(tn);
        out.res = tn;
        if (!std::isfinite(tn)) { out.reason = 3; return out; }
        if (tn <= target) { out.reason = 0; return out; }
        if (restartedRun && tn > 0.5 * runStart) { out.reason = 2; return out; }
        if (out.its >= recIts) { out.reason = 1; return out; }
        restartedRun = true; runStart = tn; rn = tn;
        seed++;
        out.nRestarts++;
        fresh = true;
    }
}

// host twin of the vector operations (CPU tier): operator and preconditioner through callbacks, plain loops.  Columns of P, G, U are n apart.
struct IdrHostOps {
    long long n; das_host_apply_fn A, M; void* user;
    const double* b; double* x;
    int s = 0;
    std::vector<double> P, G, U, r, z, t, rrec;  // rrec: the recurrence residual the last true_residual() replaced
    void shadow(int s_, unsigned seed) {
        s = s_;
        P.assign((size_t)s * n, 0.0);
        for (int q = 0; q < s; q++) for (long long i = 0; i < n; i++) P[(size_t)q * n + i] = idr_shadow_entry(seed, i, q);
        std::vector<double> Gm((size_t)s * s), L((size_t)s * s), T((size_t)s * s), row(s);
        for (int pass = 0; pass < 2; pass++) {  // CholQR twice: P <- P L^-T with P^T P = L L^T
            for (int a = 0; a < s; a++) for (int q = 0; q < s; q++) { double v = 0.0; for (long long i = 0; i < n; i++) v += P[(size_t)a * n + i] * P[(size_t)q * n + i]; Gm[(size_t)a * s + q] = v; }
            chol_upper_inverse(s, Gm.data(), L.data(), T.data());
            for (long long i = 0; i < n; i++) {
                for (int q = 0; q < s; q++) row[q] = P[(size_t)q * n + i];
                for (int q = 0; q < s; q++) { double v = 0.0; for (int a = 0; a <= q; a++) v += row[a] * T[(size_t)a * s + q]; P[(size_t)q * n + i] = v; }
            }
        }
    }
    void reset_spaces() { G.assign((size_t)s * n, 0.0); U.assign((size_t)s * n, 0.0); }
    void project_r(double* f) const { for (int q = 0; q < s; q++) { double a = 0.0; for (long long i = 0; i < n; i++) a += P[(size_t)q * n + i] * r[i]; f[q] = a; } }
    void inner_vec(int k, const double* c, double omega) {
        for (long long i = 0; i < n; i++) { double a = r[i]; for (int q = k; q < s; q++) a -= c[q - k] * G[(size_t)q * n + i]; t[i] = a; }
        M(t.data(), z.data(), user);
        double* uk = U.data() + (size_t)k * n;
        for (long long i = 0; i < n; i++) { double a = omega * z[i]; for (int q = k; q < s; q++) a += c[q - k] * U[(size_t)q * n + i]; uk[i] = a; }
        A(uk, G.data() + (size_t)k * n, user);
    }
    void dots_g(int k, double* d, double& gg) const {
        const double* gk = G.data() + (size_t)k * n;
        for (int q = 0; q < s; q++) { double a = 0.0; for (long long i = 0; i < n; i++) a += P[(size_t)q * n + i] * gk[i]; d[q] = a; }
        gg = 0.0; for (long long i = 0; i < n; i++) gg += gk[i] * gk[i];
    }
    double biortho_step(int k, const double* alpha, double beta) {
        double* gk = G.data() + (size_t)k * n;
        double* uk = U.data() + (size_t)k * n;
        double rr = 0.0;
        for (long long i = 0; i < n; i++) {
            double g = gk[i], u = uk[i];
            for (int j = 0; j < k; j++) { g -= alpha[j] * G[(size_t)j * n + i]; u -= alpha[j] * U[(size_t)j * n + i]; }
            gk[i] = g; uk[i] = u;
            r[i] -= beta * g; x[i] += beta * u;
            rr += r[i] * r[i];
        }
        return rr;
    }
    void smooth_vec() { M(r.data(), z.data(), user); A(z.data(), t.data(), user); }
    void dots_t(double& tr, double& tt) const { tr = tt = 0.0; for (long long i = 0; i < n; i++) { tr += t[i] * r[i]; tt += t[i] * t[i]; } }
    double smooth_step(double omega, double* f) {
        double rr = 0.0;
        for (long long i = 0; i < n; i++) { r[i] -= omega * t[i]; x[i] += omega * z[i]; rr += r[i] * r[i]; }
        project_r(f);
        return rr;
    }
    double true_residual() {
        rrec = r;
        A(x, r.data(), user);
        double a = 0.0;
        for (long long i = 0; i < n; i++) { r[i] = b[i] - r[i]; a += r[i] * r[i]; }
        return std::sqrt(a);
    }
};
}  // namespace das

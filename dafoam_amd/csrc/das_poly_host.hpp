// Host algebra of the polynomial-preconditioned GMRES (amd.polyDegree = d, 1 .. 16; Loe and Morgan, "Toward efficient polynomial
// preconditioning for GMRES", 2022; Embree, Loe and Morgan on the ordering of the roots).  With B = A M^-1 the Krylov operator becomes
// B p(B), p the polynomial of degree d - 1 whose residual polynomial 1 - t p(t) = prod_i (1 - t / theta_i) is the one a d-step GMRES
// cycle produced: its roots theta_i are the harmonic Ritz values of that cycle.  This is a minimum-residual polynomial of the actual
// operator - it needs no contraction, unlike a Neumann / Richardson polynomial in I - A M^-1.
// Here: the roots from the (d + 1) x d Hessenberg matrix (poly_roots_host), and the root walk t = p(B) v in real arithmetic, written ONCE
// over a small set of vector operations (poly_walk): the device solver (PolyDeviceOps, das_device.hip, kernels of das_poly.hpp) and the
// host twin of the CPU tier (PolyHostOps, das_debug_poly_apply_host) run the same walk.  No HIP in this header.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "das_gmres_host.hpp"

namespace das {

static const int POLY_MAX_DEGREE = 16;

// Ordered roots of the GMRES polynomial of a d-step cycle.  Hbar: the unrotated (d + 1) x d Hessenberg matrix, row-major with leading
// dimension ld.  The harmonic Ritz values are the eigenvalues of H_d + h_{d+1,d}^2 H_d^-T e_d e_d^T (dense eigen-solver callback, as in
// gmres_dr_restart_host).  A complex pair is kept once, by its member with positive imaginary part, and stands for two consecutive
// roots.  Order: modified Leja - the first root has the largest modulus, each next one maximises sum_i log|theta - theta_i| over the
// roots already placed (conjugates included); ties go to the lower index of the eigen-solver's output.
// Returns the number of entries written to re / im (> 0; real roots + pairs, nPairs of them pairs), or 0: no usable polynomial
// (no callback or it failed, H_d singular, a root zero or not finite, pairs that do not match) - the caller runs without one.
inline int poly_roots_host(das_dense_eig_fn eig, int d, const double* Hbar, int ld, double* re, double* im, int* nPairs) {
    if (nPairs) *nPairs = 0;
    if (!eig || d < 1 || d > POLY_MAX_DEGREE) return 0;
    for (int i = 0; i <= d; i++) for (int j = 0; j < d; j++) if (!std::isfinite(Hbar[(size_t)i * ld + j])) return 0;
    std::vector<double> Hm((size_t)d * d), f;
    for (int i = 0; i < d; i++) for (int j = 0; j < d; j++) Hm[(size_t)i * d + j] = Hbar[(size_t)i * ld + j];
    if (!dr_solve_transposed_last(d, Hm, f)) return 0;
    const double h = Hbar[(size_t)d * ld + (d - 1)];
    for (int i = 0; i < d; i++) {
        if (!std::isfinite(f[i])) return 0;
        Hm[(size_t)i * d + (d - 1)] += h * h * f[i];
    }
    std::vector<double> wr(d, 0.0), wi(d, 0.0), vr((size_t)d * d), vi((size_t)d * d);
    if (eig(d, Hm.data(), wr.data(), wi.data(), vr.data(), vi.data()) != 0) return 0;
    // one representative per pair
    std::vector<double> cr, ci;
    int nreal = 0, npos = 0, nneg = 0;
    for (int i = 0; i < d; i++) {
        if (!std::isfinite(wr[i]) || !std::isfinite(wi[i]) || (wr[i] == 0.0 && wi[i] == 0.0)) return 0;
        if (wi[i] < 0.0) { nneg++; continue; }
        if (wi[i] > 0.0) npos++; else nreal++;
        cr.push_back(wr[i]); ci.push_back(wi[i]);
    }
    if (npos != nneg || nreal + 2 * npos != d) return 0;
    const int m = (int)cr.size();
    std::vector<char> placed(m, 0);
    std::vector<int> order;
    for (int step = 0; step < m; step++) {
        int best = -1;
        double bestv = 0.0;
        for (int c = 0; c < m; c++) {
            if (placed[c]) continue;
            double v;
            if (step == 0) v = std::hypot(cr[c], ci[c]);
            else {
                v = 0.0;
                for (int q : order) {
                    v += std::log(std::hypot(cr[c] - cr[q], ci[c] - ci[q]));
                    if (ci[q] != 0.0) v += std::log(std::hypot(cr[c] - cr[q], ci[c] + ci[q]));
                }
            }
            if (best < 0 || v > bestv) { best = c; bestv = v; }  // (strict: a tie keeps the lower index; a NaN never wins)
        }
        placed[best] = 1;
        order.push_back(best);
    }
    for (int i = 0; i < m; i++) { re[i] = cr[order[i]]; im[i] = ci[order[i]]; }
    if (nPairs) *nPairs = npos;
    return m;
}
// degree of the polynomial's residual polynomial: real roots + 2 x pairs
inline int poly_degree_of(int nroots, const double* im) {
    int d = 0;
    for (int i = 0; i < nroots; i++) d += im[i] != 0.0 ? 2 : 1;
    return d;
}

// t = p(B) v by the ordered roots, in real arithmetic: prod = v, poly = 0, then per root
//   real theta:               poly += prod / theta;                                   unless last: prod -= (B prod) / theta
//   pair a +- i b, m2 = |.|^2: tmp = 2 a prod - B prod; poly += tmp / m2;              unless last: prod -= (B tmp) / m2
// - degree - 1 products of B, nothing but element-wise updates between them (true divisions: degree 1 gives v / theta exactly).
// Ops: product(fromTmp, first) [w = B x, x = tmp | prod, or the input v while `first`]; real_step(first, last, theta)
// [poly (+)= prod / theta; unless last: prod -= w / theta]; pair_first(first, twoa, m2) [tmp = twoa prod - w; poly (+)= tmp / m2];
// pair_second(first, m2) [prod -= w / m2].  `first`: prod is still the input v (read-only) and poly is not read: no copy, no zero fill.
inline void poly_pair_coef(double re, double im, double& twoa, double& m2) { twoa = 2.0 * re; m2 = re * re + im * im; }
template <class Ops>
inline void poly_walk(Ops& ops, int nroots, const double* re, const double* im) {
    for (int i = 0; i < nroots; i++) {
        const bool first = i == 0, last = i == nroots - 1;
        if (im[i] == 0.0) {
            if (!last) ops.product(false, first);
            ops.real_step(first, last, re[i]);
        } else {
            double twoa, m2;
            poly_pair_coef(re[i], im[i], twoa, m2);
            ops.product(false, first);
            ops.pair_first(first, twoa, m2);
            if (!last) { ops.product(true, first); ops.pair_second(first, m2); }
        }
    }
}

// the walk on host vectors with callback operator A and preconditioner M (y = M^-1 x): the CPU tier's twin of the device apply
struct PolyHostOps {
    long long n; das_host_apply_fn A, M; void* user;
    const double* v;
    std::vector<double> prod, poly, tmp, z, w;
    PolyHostOps(long long n_, das_host_apply_fn A_, das_host_apply_fn M_, void* user_, const double* v_)
        : n(n_), A(A_), M(M_), user(user_), v(v_), prod(n_, 0.0), poly(n_, 0.0), tmp(n_, 0.0), z(n_, 0.0), w(n_, 0.0) {}
    void product(bool fromTmp, bool first) {
        M(fromTmp ? tmp.data() : (first ? v : prod.data()), z.data(), user);
        A(z.data(), w.data(), user);
    }
    void real_step(bool first, bool last, double th) {
        const double* p = first ? v : prod.data();
        for (long long i = 0; i < n; i++) {
            const double pv = p[i];
            poly[i] = first ? pv / th : poly[i] + pv / th;
            if (!last) prod[i] = pv - w[i] / th;
        }
    }
    void pair_first(bool first, double twoa, double m2) {
        const double* p = first ? v : prod.data();
        for (long long i = 0; i < n; i++) {
            const double t = twoa * p[i] - w[i];
            tmp[i] = t;
            poly[i] = first ? t / m2 : poly[i] + t / m2;
        }
    }
    void pair_second(bool first, double m2) {
        const double* p = first ? v : prod.data();
        for (long long i = 0; i < n; i++) prod[i] = p[i] - w[i] / m2;
    }
};

}  // namespace das

// Dense host algebra of the GMRES solvers (restarted, deflated restarting, block): Givens updates of the Hessenberg least squares, back
// substitution, the deflated-restart iteration and its host twin, the Cholesky step of CholQR.  Host C++
// only - no device, no solver handle, no global state: the CPU tier runs this very code (das_debug_gmres_dr_*, das_debug_block_*).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "das_error.hpp"

namespace das {
// a new basis vector whose norm is below this fraction of the norm of the operator image it was projected from is
// rounding noise (the rounding errors of the projection itself are ~1e-16 of that norm, at any problem size: they are
// componentwise): the Krylov space is exhausted - happy breakdown
constexpr double GMRES_BREAKDOWN_TOL = 1e-13;

// Givens rotation (c, s) that takes (a, b) to (d, 0); returns d
inline double givens(double a, double b, double& c, double& s) {
    const double d = std::hypot(a, b);
    c = d > 0 ? a / d : 1.0; s = d > 0 ? b / d : 0.0;
    return d;
}
// Givens update of Hessenberg column `col` (H (m+1) x m row-major, entries H[0..col+1][col] already set) and of g; returns the recurrence residual norm
inline double gmres_rotate_column(std::vector<double>& H, std::vector<double>& cs, std::vector<double>& sn, std::vector<double>& g, int m, int col) {
    for (int i = 0; i < col; i++) {
        const double a = H[(size_t)i * m + col], b2 = H[(size_t)(i + 1) * m + col];
        H[(size_t)i * m + col] = cs[i] * a + sn[i] * b2;
        H[(size_t)(i + 1) * m + col] = -sn[i] * a + cs[i] * b2;
    }
    H[(size_t)col * m + col] = givens(H[(size_t)col * m + col], H[(size_t)(col + 1) * m + col], cs[col], sn[col]);
    H[(size_t)(col + 1) * m + col] = 0.0;
    g[col + 1] = -sn[col] * g[col];
    g[col] = cs[col] * g[col];
    return std::fabs(g[col + 1]);
}
// back substitution R y = g: R upper triangular K x K, row-major, leading dimension ldr; entry (i, r) of g and y at [i * stride + r] (y may be g)
inline void back_substitute(int K, const double* R, int ldr, int nrhs, int stride, const double* g, double* y) {
    for (int r = 0; r < nrhs; r++)
        for (int i = K - 1; i >= 0; i--) {
            double a = g[(size_t)i * stride + r];
            for (int q = i + 1; q < K; q++) a -= R[(size_t)i * ldr + q] * y[(size_t)q * stride + r];
            y[(size_t)i * stride + r] = a / R[(size_t)i * ldr + i];
        }
}

// ---- GMRES with deflated restarting (opt-in: amd.gmresDeflation = k > 0; Morgan, SIAM J. Sci. Comput. 24 (2002) "GMRES-DR") ------------
// A restart of length m (adjEqnOption.gmresRestart) keeps the k harmonic Ritz vectors of smallest magnitude: the next cycle starts from
// the (k+1)-dimensional subspace span{harmonic Ritz vectors, residual}, for which an Arnoldi-like relation A M^-1 V_k = V_{k+1} Hbar_k
// holds with a DENSE leading block, and continues Arnoldi from there.  Why (round 4, CPU prototype tools/gmres_dr_study.py): the residual
// history of the airfoil adjoint is a plateau of hundreds of iterations followed by a fast drop - plain restarting inside the plateau
// stalls (GMRES(100): 0.81 after 1500 iterations where full GMRES needs 302), deflated restarting needs 354-379 with 101-151 basis
// vectors.  The basis is what limits the mesh size on one GPU (1000 vectors = 125 GB at 2 M cells).  Reference role: PETSc offers the
// same idea as KSPDGMRES; the reference's default stays the undeflated solver, and so does this library's.
// Orthogonalisation: classical Gram-Schmidt, always two passes.  The dense eigenproblem of the m x m harmonic matrix is solved through a
// callback (das_set_dense_eig_callback; the Python mirror installs numpy.linalg.eig) - the library carries no LAPACK.
typedef int (*das_dense_eig_fn)(int m, const double* A_rowmajor, double* wr, double* wi, double* vr_colmajor, double* vi_colmajor);
// least-squares bookkeeping of min |c - Hbar y|: Qt (accumulated rotations), R = Qt Hbar, gt = Qt c
struct DrLsq {
    int m = 0;
    std::vector<double> Qt, R, gt;
    void reset(int m_, const std::vector<double>& c) {
        m = m_;
        Qt.assign((size_t)(m + 1) * (m + 1), 0.0);
        for (int i = 0; i <= m; i++) Qt[(size_t)i * (m + 1) + i] = 1.0;
        R.assign((size_t)(m + 1) * m, 0.0);
        gt = c;
    }
    // append column `col` of Hbar whose entries 0..nr-1 may be non-zero; eliminates everything below the diagonal
    double add_column(int col, int nr, const double* h) {
        const int ld = m + 1;
        std::vector<double> t(nr, 0.0);
        for (int i = 0; i < nr; i++) { double a = 0.0; for (int q = 0; q < nr; q++) a += Qt[(size_t)i * ld + q] * h[q]; t[i] = a; }
        for (int r = nr - 1; r > col; r--) {  // rotate rows (r-1, r) so that t[r] = 0
            const double a = t[r - 1], b = t[r];
            const double d = std::hypot(a, b);
            if (d == 0.0) continue;
            const double cc = a / d, ss = b / d;
            t[r - 1] = d; t[r] = 0.0;
            for (int q = 0; q < nr; q++) {
                const double x = Qt[(size_t)(r - 1) * ld + q], y = Qt[(size_t)r * ld + q];
                Qt[(size_t)(r - 1) * ld + q] = cc * x + ss * y; Qt[(size_t)r * ld + q] = -ss * x + cc * y;
            }
            // (earlier columns of R are zero in rows >= col: nothing to rotate there; later columns do not exist yet)
            const double gx = gt[r - 1], gy = gt[r];
            gt[r - 1] = cc * gx + ss * gy; gt[r] = -ss * gx + cc * gy;
        }
        for (int i = 0; i < nr; i++) R[(size_t)i * m + col] = t[i];
        return std::fabs(gt[col + 1]);
    }
    void solve(int j, std::vector<double>& y) const { y.assign(j, 0.0); back_substitute(j, R.data(), m, 1, 1, gt.data(), y.data()); }
};
// dense LU solve (partial pivoting) of A^T f = e_last, A row-major n x n (destroyed)
inline bool dr_solve_transposed_last(int n, std::vector<double> A, std::vector<double>& f) {
    // work on T = A^T
    std::vector<double> T((size_t)n * n);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) T[(size_t)i * n + j] = A[(size_t)j * n + i];
    f.assign(n, 0.0); f[n - 1] = 1.0;
    for (int c = 0; c < n; c++) {
        int p = c; double best = std::fabs(T[(size_t)c * n + c]);
        for (int r = c + 1; r < n; r++) if (std::fabs(T[(size_t)r * n + c]) > best) { best = std::fabs(T[(size_t)r * n + c]); p = r; }
        if (best == 0.0) return false;
        if (p != c) { for (int q = 0; q < n; q++) std::swap(T[(size_t)c * n + q], T[(size_t)p * n + q]); std::swap(f[c], f[p]); }
        for (int r = c + 1; r < n; r++) {
            const double l = T[(size_t)r * n + c] / T[(size_t)c * n + c];
            if (l == 0.0) continue;
            for (int q = c; q < n; q++) T[(size_t)r * n + q] -= l * T[(size_t)c * n + q];
            f[r] -= l * f[c];
        }
    }
    back_substitute(n, T.data(), n, 1, 1, f.data(), f.data());
    return true;
}
// host part of a deflated restart (also exported for the CPU tier: das_debug_gmres_dr_restart).  In: Hbar ((m+1) x m row-major), the
// residual vector rvec = c - Hbar y in the basis V_{m+1}, the wanted k.  Out: kk (k or k +- 1: a complex pair is never split), P1
// ((m+1) x (kk+1) row-major, orthonormal columns: the new basis is V P1), Hnew ((kk+1) x kk row-major), cnew (kk+1).
inline int gmres_dr_restart_host(das_dense_eig_fn eig, int m, int k, const std::vector<double>& Hb, const std::vector<double>& rvec, int& kk,
                                 std::vector<double>& P1, std::vector<double>& Hnew, std::vector<double>& cnew) {
    DAS_CHECK(eig, DAS_ERR_STATE, "amd.gmresDeflation needs a dense eigen-solver callback (das_set_dense_eig_callback; the Python mirror installs numpy's)");
    std::vector<double> Hm((size_t)m * m), f;
    for (int i = 0; i < m; i++) for (int j = 0; j < m; j++) Hm[(size_t)i * m + j] = Hb[(size_t)i * m + j];
    if (!dr_solve_transposed_last(m, Hm, f)) return -1;
    const double h2 = Hb[(size_t)m * m + (m - 1)] * Hb[(size_t)m * m + (m - 1)];
    std::vector<double> Gm = Hm;
    for (int i = 0; i < m; i++) Gm[(size_t)i * m + (m - 1)] += h2 * f[i];
    std::vector<double> wr(m), wi(m), vr((size_t)m * m), vi((size_t)m * m);
    if (eig(m, Gm.data(), wr.data(), wi.data(), vr.data(), vi.data()) != 0) return -1;
    std::vector<int> idx(m);
    for (int i = 0; i < m; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int a, int b) { const double ma = std::hypot(wr[a], wi[a]), mb = std::hypot(wr[b], wi[b]); return ma < mb || (ma == mb && a < b); });
    // real basis of the invariant subspace of the k smallest harmonic Ritz values; a conjugate pair contributes (Re v, Im v) once
    std::vector<std::vector<double>> cols;
    std::vector<char> used(m, 0);
    for (int q = 0; q < m && (int)cols.size() < k; q++) {
        const int e = idx[q];
        if (used[e]) continue;
        used[e] = 1;
        std::vector<double> re(m), im(m);
        double imax = 0.0;
        for (int i = 0; i < m; i++) { re[i] = vr[(size_t)e * m + i]; im[i] = vi[(size_t)e * m + i]; imax = std::max(imax, std::fabs(im[i])); }
        cols.push_back(re);
        if (std::fabs(wi[e]) > 0.0 && imax > 0.0) {
            cols.push_back(im);
            for (int q2 = q + 1; q2 < m; q2++) {  // its conjugate is the same two vectors
                const int e2 = idx[q2];
                if (!used[e2] && wr[e2] == wr[e] && wi[e2] == -wi[e]) { used[e2] = 1; break; }
            }
        }
    }
    kk = (int)cols.size();
    if (kk > m - 1) { cols.resize(m - 1); kk = m - 1; }
    // orthonormalise (modified Gram-Schmidt, twice) -> Pk (m x kk); drop numerically dependent columns
    std::vector<std::vector<double>> Q;
    for (auto& v : cols) {
        for (int pass = 0; pass < 2; pass++)
            for (auto& q : Q) { double d = 0.0; for (int i = 0; i < m; i++) d += q[i] * v[i]; for (int i = 0; i < m; i++) v[i] -= d * q[i]; }
        double nv = 0.0; for (int i = 0; i < m; i++) nv += v[i] * v[i];
        nv = std::sqrt(nv);
        if (!(nv > 1e-10)) continue;
        for (int i = 0; i < m; i++) v[i] /= nv;
        Q.push_back(v);
    }
    kk = (int)Q.size();
    if (kk == 0) return -1;
    // P1 = [ [Pk; 0], rvec orthogonalised against it and normalised ]
    P1.assign((size_t)(m + 1) * (kk + 1), 0.0);
    for (int c = 0; c < kk; c++) for (int i = 0; i < m; i++) P1[(size_t)i * (kk + 1) + c] = Q[c][i];
    std::vector<double> rv = rvec;
    for (int pass = 0; pass < 2; pass++)
        for (int c = 0; c < kk; c++) { double d = 0.0; for (int i = 0; i < m; i++) d += Q[c][i] * rv[i]; for (int i = 0; i < m; i++) rv[i] -= d * Q[c][i]; }
    double nr = 0.0; for (int i = 0; i <= m; i++) nr += rv[i] * rv[i];
    nr = std::sqrt(nr);
    if (!(nr > 0.0)) return -1;
    for (int i = 0; i <= m; i++) P1[(size_t)i * (kk + 1) + kk] = rv[i] / nr;
    // Hnew = P1^T Hbar Pk, cnew = P1^T rvec
    std::vector<double> HP((size_t)(m + 1) * kk, 0.0);
    for (int i = 0; i <= m; i++) for (int c = 0; c < kk; c++) { double a = 0.0; for (int q = 0; q < m; q++) a += Hb[(size_t)i * m + q] * Q[c][q]; HP[(size_t)i * kk + c] = a; }
    Hnew.assign((size_t)(kk + 1) * kk, 0.0);
    for (int r = 0; r <= kk; r++) for (int c = 0; c < kk; c++) { double a = 0.0; for (int i = 0; i <= m; i++) a += P1[(size_t)i * (kk + 1) + r] * HP[(size_t)i * kk + c]; Hnew[(size_t)r * kk + c] = a; }
    cnew.assign(kk + 1, 0.0);
    for (int r = 0; r <= kk; r++) { double a = 0.0; for (int i = 0; i <= m; i++) a += P1[(size_t)i * (kk + 1) + r] * rvec[i]; cnew[r] = a; }
    return 0;
}

// The iteration itself, written once over a small set of vector operations (Ops): the device solver below and the host twin of the CPU
// tier (das_debug_gmres_dr_host) run THIS loop - what the CPU tests check is what the GPU executes, up to the kernels behind Ops, all of
// which the undeflated solver already uses.  Ops: n; start(beta) [v_0 = r / beta]; arnoldi(j, h, ww, hn) [w = A M^-1 v_j orthogonalised
// against v_0..v_j by two classical Gram-Schmidt passes: h[0..j] the summed coefficients, ww = |A M^-1 v_j|^2, hn = |w| afterwards,
// v_{j+1} = w / hn if hn > 0]; update(j, y) [x += M^-1 (V_j y)]; true_residual() [r = b - A x, returns |r|]; compress(m, kk, P1)
// [V[:, 0..kk] = V[:, 0..m] P1].  eig: the dense eigen-solver of the restart.
struct DrResult { long long its = 0; double res0 = 0, res = 0; int nBreakdown = 0, nRestarts = 0, nDeflated = 0; };
template <class Ops>
inline DrResult gmres_dr_loop(Ops& ops, das_dense_eig_fn eig, int m, int kdef, double beta0, double target, long long maxIts, std::vector<double>& hist) {
    DrResult out;
    out.res0 = beta0;
    kdef = std::max(1, std::min(kdef, m - 2));
    std::vector<double> Hb((size_t)(m + 1) * m, 0.0), c(m + 1, 0.0), y, rvec(m + 1), hcol(m + 2), h(m + 2), P1, Hnew, cnew;
    DrLsq L;
    int j0 = 0;  // vectors 0..j0 of the basis and the leading (j0+1) x j0 block of Hbar are in place
    bool first = true;
    double beta = beta0;
    while (beta > target && out.its < maxIts) {
        if (first) {
            ops.start(beta);
            std::fill(Hb.begin(), Hb.end(), 0.0);
            std::fill(c.begin(), c.end(), 0.0);
            c[0] = beta;
            j0 = 0;
            first = false;
        }
        L.reset(m, c);
        for (int col = 0; col < j0; col++) {  // the dense block carried over the restart
            for (int i = 0; i <= j0; i++) hcol[i] = Hb[(size_t)i * m + col];
            L.add_column(col, j0 + 1, hcol.data());
        }
        int j = j0;
        double res = beta;
        for (; j < m && out.its < maxIts;) {
            double ww = 0.0, hn = 0.0;
            ops.arnoldi(j, h.data(), ww, hn);
            if (!(hn > GMRES_BREAKDOWN_TOL * std::sqrt(std::max(ww, 0.0)))) { hn = 0.0; out.nBreakdown++; }
            for (int i = 0; i <= j; i++) { hcol[i] = h[i]; Hb[(size_t)i * m + j] = h[i]; }
            hcol[j + 1] = hn; Hb[(size_t)(j + 1) * m + j] = hn;
            res = L.add_column(j, j + 2, hcol.data());
            out.its++;
            hist.push_back(res);
            j++;
            if (res <= target || hn == 0.0) break;
        }
        L.solve(j, y);
        ops.update(j, y.data());
        beta = ops.true_residual();  // one operator product per cycle: the recurrence is checked against it
        hist.back() = beta;
        if (beta <= target || out.its >= maxIts) break;
        const bool recurrenceOk = std::fabs(res - beta) <= 1e-6 * beta0 + 1e-3 * beta;
        if (j < m || !recurrenceOk) { first = true; out.nRestarts++; continue; }  // breakdown / early exit / drifted recurrence: plain restart
        // ---- deflated restart: rvec = c - Hbar y, harmonic Ritz vectors, compression of the basis
        for (int i = 0; i <= m; i++) { double a = c[i]; for (int q = 0; q < m; q++) a -= Hb[(size_t)i * m + q] * y[q]; rvec[i] = a; }
        int kk = 0;
        if (gmres_dr_restart_host(eig, m, kdef, Hb, rvec, kk, P1, Hnew, cnew) != 0) { first = true; out.nRestarts++; continue; }
        ops.compress(m, kk, P1.data());
        std::fill(Hb.begin(), Hb.end(), 0.0);
        for (int r = 0; r <= kk; r++) for (int q = 0; q < kk; q++) Hb[(size_t)r * m + q] = Hnew[(size_t)r * kk + q];
        std::fill(c.begin(), c.end(), 0.0);
        for (int r = 0; r <= kk; r++) c[r] = cnew[r];
        j0 = kk;
        out.nDeflated++;
    }
    out.res = beta;
    return out;
}

// host twin of the vector operations (CPU tier): operator and preconditioner through callbacks, plain loops
typedef void (*das_host_apply_fn)(const double* x, double* y, void* user);
struct DrHostOps {
    long long n; das_host_apply_fn A, M; void* user;
    const double* b; double* x;
    std::vector<double> V, w, z, r;
    int m;
    void start(double beta) { for (long long i = 0; i < n; i++) V[i] = r[i] / beta; }
    void arnoldi(int j, double* h, double& ww, double& hn) {
        M(V.data() + (size_t)j * n, z.data(), user);
        A(z.data(), w.data(), user);
        ww = 0.0; for (long long i = 0; i < n; i++) ww += w[i] * w[i];
        std::vector<double> h1(j + 1), h2(j + 1);
        for (int pass = 0; pass < 2; pass++) {
            std::vector<double>& hp = pass ? h2 : h1;
            for (int q = 0; q <= j; q++) { double a = 0.0; const double* v = V.data() + (size_t)q * n; for (long long i = 0; i < n; i++) a += v[i] * w[i]; hp[q] = a; }
            for (int q = 0; q <= j; q++) { const double* v = V.data() + (size_t)q * n; for (long long i = 0; i < n; i++) w[i] -= hp[q] * v[i]; }
        }
        for (int q = 0; q <= j; q++) h[q] = h1[q] + h2[q];
        double a = 0.0; for (long long i = 0; i < n; i++) a += w[i] * w[i];
        hn = std::sqrt(a);
        if (hn > GMRES_BREAKDOWN_TOL * std::sqrt(ww)) for (long long i = 0; i < n; i++) V[(size_t)(j + 1) * n + i] = w[i] / hn;
    }
    void update(int j, const double* y) {
        std::fill(w.begin(), w.end(), 0.0);
        for (int q = 0; q < j; q++) { const double* v = V.data() + (size_t)q * n; for (long long i = 0; i < n; i++) w[i] += y[q] * v[i]; }
        M(w.data(), z.data(), user);
        for (long long i = 0; i < n; i++) x[i] += z[i];
    }
    double true_residual() {
        A(x, r.data(), user);
        double a = 0.0;
        for (long long i = 0; i < n; i++) { r[i] = b[i] - r[i]; a += r[i] * r[i]; }
        return std::sqrt(a);
    }
    void compress(int mm, int kk, const double* P1) {
        std::vector<double> Vn((size_t)(kk + 1) * n, 0.0);
        for (int c = 0; c <= kk; c++)
            for (int q = 0; q <= mm; q++) { const double p = P1[(size_t)q * (kk + 1) + c]; if (p == 0.0) continue; const double* v = V.data() + (size_t)q * n; double* o = Vn.data() + (size_t)c * n; for (long long i = 0; i < n; i++) o[i] += p * v[i]; }
        std::copy(Vn.begin(), Vn.end(), V.begin());
    }
};

// Cholesky G = L L^T of the sv x sv Gram matrix of CholQR (row-major; a non-positive pivot = a column that lost all its new content:
// replaced by a tiny one) and T = L^-T (upper triangular): Q = W T
inline void chol_upper_inverse(int sv, const double* G, double* L, double* T) {
    std::fill(L, L + (size_t)sv * sv, 0.0);
    double gmax = 0.0;
    for (int i = 0; i < sv; i++) gmax = std::max(gmax, G[(size_t)i * sv + i]);
    for (int j = 0; j < sv; j++) {
        double d = G[(size_t)j * sv + j];
        for (int q = 0; q < j; q++) d -= L[(size_t)j * sv + q] * L[(size_t)j * sv + q];
        if (!(d > 1e-28 * gmax)) d = std::max(1e-28 * gmax, 1e-300);
        L[(size_t)j * sv + j] = std::sqrt(d);
        for (int i = j + 1; i < sv; i++) {
            double a = G[(size_t)i * sv + j];
            for (int q = 0; q < j; q++) a -= L[(size_t)i * sv + q] * L[(size_t)j * sv + q];
            L[(size_t)i * sv + j] = a / L[(size_t)j * sv + j];
        }
    }
    std::fill(T, T + (size_t)sv * sv, 0.0);
    for (int c = 0; c < sv; c++)  // solve L^T t_c = e_c  (upper triangular system, backward)
        for (int i = sv - 1; i >= 0; i--) {
            double a = (i == c) ? 1.0 : 0.0;
            for (int q = i + 1; q < sv; q++) a -= L[(size_t)q * sv + i] * T[(size_t)q * sv + c];
            T[(size_t)i * sv + c] = a / L[(size_t)i * sv + i];
        }
}

// least squares of block GMRES, min |[S0; 0] - Hbar Y| for sv right-hand sides at once: Hbar is block Hessenberg ((m+1)sv x m sv, sv
// sub-diagonals), reduced to the upper triangular H by Givens rotations that are applied to the right-hand sides G as they are generated
struct BlockLsq {
    int m = 0, sv = 0;
    std::vector<double> H, G;          // row-major: (m+1)sv x m sv, (m+1)sv x sv
    std::vector<double> rc, rs, hcol;  // rotation (col q, step u); the column being rotated
    // new cycle: the residual block is V_0 S0 (S0 sv x sv row-major)
    void reset(int m_, int sv_, const double* S0) {
        m = m_; sv = sv_;
        const int ms = m * sv;
        H.assign((size_t)(ms + sv) * ms, 0.0); G.assign((size_t)(ms + sv) * sv, 0.0);
        rc.resize((size_t)ms * sv); rs.resize((size_t)ms * sv);
        for (int i = 0; i < sv; i++) for (int r = 0; r < sv; r++) G[(size_t)i * sv + r] = S0[(size_t)i * sv + r];
    }
    // block Hessenberg column j: rows 0..K-1 (K = (j+1) sv) from the projections Hc + Hc2 (K x sv), rows K..K+sv-1 = S (upper triangular)
    void add_column(int j, const double* Hc, const double* Hc2, const double* S) {
        const int K = (j + 1) * sv, ms = m * sv;
        for (int c = 0; c < sv; c++) {
            const int q = j * sv + c;
            hcol.assign((size_t)K + sv, 0.0);
            for (int i = 0; i < K; i++) hcol[i] = Hc[(size_t)i * sv + c] + Hc2[(size_t)i * sv + c];
            for (int i = 0; i <= c; i++) hcol[K + i] = S[(size_t)i * sv + c];
            for (int qq = 0; qq < q; qq++)          // earlier rotations, in the order they were generated
                for (int u = sv - 1; u >= 0; u--) {
                    const int a = qq + u, b2 = qq + u + 1;
                    if (b2 >= K + sv) continue;
                    const double cc = rc[(size_t)qq * sv + u], ss = rs[(size_t)qq * sv + u];
                    const double x = hcol[a], y = hcol[b2];
                    hcol[a] = cc * x + ss * y; hcol[b2] = -ss * x + cc * y;
                }
            for (int u = sv - 1; u >= 0; u--) {     // eliminate the s sub-diagonal entries of this column
                const int a = q + u, b2 = q + u + 1;
                double cc, ss;
                hcol[a] = givens(hcol[a], hcol[b2], cc, ss); hcol[b2] = 0.0;
                rc[(size_t)q * sv + u] = cc; rs[(size_t)q * sv + u] = ss;
                for (int r = 0; r < sv; r++) {
                    const double gx = G[(size_t)a * sv + r], gy = G[(size_t)b2 * sv + r];
                    G[(size_t)a * sv + r] = cc * gx + ss * gy; G[(size_t)b2 * sv + r] = -ss * gx + cc * gy;
                }
            }
            for (int i = 0; i <= q; i++) H[(size_t)i * ms + q] = hcol[i];
        }
    }
    // recurrence residual norm of every right-hand side after column j
    void residuals(int j, double* res) const {
        const int K = (j + 1) * sv;
        for (int r = 0; r < sv; r++) { double a = 0.0; for (int i = K; i < K + sv; i++) a += G[(size_t)i * sv + r] * G[(size_t)i * sv + r]; res[r] = std::sqrt(a); }
    }
    // Y (j sv x sv row-major) of the first j block columns: H Y = G
    void solve(int j, double* Y) const { back_substitute(j * sv, H.data(), m * sv, sv, sv, G.data(), Y); }
};
}  // namespace das

// Stand-alone check of csrc/das_poly_host.hpp for a host sanitizer build (no GPU, no Python):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/poly_host_check.cpp -o poly_host_check && ./poly_host_check
// A small dense system, d = 1, 2, 3 steps of Arnoldi, the roots of the GMRES polynomial through a built-in eigen routine for 1 x 1,
// 2 x 2 and 3 x 3 matrices, the host root walk, and the identity |b - B p(B) b| = GMRES(d) residual.  Exit status 0 = all held.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../dafoam_amd/csrc/das_poly_host.hpp"

namespace {
const int N = 7;
double Bm[N][N];
void applyB(const double* x, double* y, void*) { for (int i = 0; i < N; i++) { double a = 0; for (int j = 0; j < N; j++) a += Bm[i][j] * x[j]; y[i] = a; } }
void applyI(const double* x, double* y, void*) { for (int i = 0; i < N; i++) y[i] = x[i]; }

// eigenvalues of a 1 x 1, 2 x 2 or 3 x 3 real matrix (row-major); the eigenvectors are not needed by the roots and stay zero
void quad(double tr, double det, double* wr, double* wi) {
    const double disc = tr * tr / 4 - det;
    if (disc >= 0) { const double s = std::sqrt(disc); wr[0] = tr / 2 + s; wr[1] = tr / 2 - s; wi[0] = wi[1] = 0; }
    else { const double s = std::sqrt(-disc); wr[0] = wr[1] = tr / 2; wi[0] = s; wi[1] = -s; }
}
int small_eig(int m, const double* A, double* wr, double* wi, double* vr, double* vi) {
    for (int i = 0; i < m * m; i++) vr[i] = vi[i] = 0.0;
    if (m == 1) { wr[0] = A[0]; wi[0] = 0; return 0; }
    if (m == 2) { quad(A[0] + A[3], A[0] * A[3] - A[1] * A[2], wr, wi); return 0; }
    if (m != 3) return 1;
    // t^3 - c2 t^2 + c1 t - c0: one real root by bisection, the other two from the deflated quadratic
    const double c2 = A[0] + A[4] + A[8];
    const double c1 = A[0] * A[4] - A[1] * A[3] + A[0] * A[8] - A[2] * A[6] + A[4] * A[8] - A[5] * A[7];
    const double c0 = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    auto f = [&](double t) { return ((t - c2) * t + c1) * t - c0; };
    double lo = -1.0, hi = 1.0;
    while (f(lo) > 0) lo *= 2;
    while (f(hi) < 0) hi *= 2;
    for (int it = 0; it < 200; it++) { const double mid = 0.5 * (lo + hi); if (f(mid) < 0) lo = mid; else hi = mid; }
    const double r = 0.5 * (lo + hi);
    wr[0] = r; wi[0] = 0;
    quad(c2 - r, r * r - c2 * r + c1, wr + 1, wi + 1);  // t^2 - (c2 - r) t + (r^2 - c2 r + c1)
    return 0;
}
double norm(const std::vector<double>& v) { double a = 0; for (double x : v) a += x * x; return std::sqrt(a); }
}  // namespace

int main() {
    for (int i = 0; i < N; i++) for (int j = 0; j < N; j++) Bm[i][j] = (i == j ? 1.5 + 0.1 * i : 0.0) + 0.3 * std::sin(1.0 + 3 * i + 7 * j) + (j == i + 1 ? 0.6 : 0.0) - (i == j + 1 ? 0.6 : 0.0);
    std::vector<double> b(N);
    for (int i = 0; i < N; i++) b[i] = 1.0 / (1 + i) - 0.4;
    int bad = 0;
    for (int d = 1; d <= 3; d++) {
        // Arnoldi, modified Gram-Schmidt twice
        std::vector<std::vector<double>> V(d + 1, std::vector<double>(N));
        std::vector<double> H((size_t)(d + 1) * d, 0.0), w(N);
        const double beta = norm(b);
        for (int i = 0; i < N; i++) V[0][i] = b[i] / beta;
        for (int j = 0; j < d; j++) {
            applyB(V[j].data(), w.data(), nullptr);
            for (int pass = 0; pass < 2; pass++)
                for (int q = 0; q <= j; q++) { double h = 0; for (int i = 0; i < N; i++) h += V[q][i] * w[i]; H[(size_t)q * d + j] += h; for (int i = 0; i < N; i++) w[i] -= h * V[q][i]; }
            H[(size_t)(j + 1) * d + j] = norm(w);
            for (int i = 0; i < N; i++) V[j + 1][i] = w[i] / H[(size_t)(j + 1) * d + j];
        }
        // GMRES(d) residual: Givens on a copy
        std::vector<double> R = H, cs(d), sn(d), g(d + 1, 0.0);
        g[0] = beta;
        double rho = beta;
        for (int j = 0; j < d; j++) rho = das::gmres_rotate_column(R, cs, sn, g, d, j);
        double re[das::POLY_MAX_DEGREE], im[das::POLY_MAX_DEGREE];
        int npairs = 0;
        const int m = das::poly_roots_host(small_eig, d, H.data(), d, re, im, &npairs);
        if (m == 0 || das::poly_degree_of(m, im) != d) { std::printf("d = %d: no roots (%d)\n", d, m); bad++; continue; }
        das::PolyHostOps ops(N, applyB, applyI, nullptr, b.data());
        das::poly_walk(ops, m, re, im);
        std::vector<double> r(N);
        applyB(ops.poly.data(), r.data(), nullptr);
        for (int i = 0; i < N; i++) r[i] = b[i] - r[i];
        const double got = norm(r);
        std::printf("d = %d: %d root entries, %d pairs, |b - B p(B) b| = %.15e, GMRES(%d) residual %.15e, relative difference %.2e\n", d, m, npairs, got, d, rho, std::fabs(got - rho) / rho);
        if (!(std::fabs(got - rho) <= 1e-9 * rho)) bad++;
    }
    // the fallbacks: a singular H_d, a non-finite entry, no callback
    const double Hz[6] = {0, 1, 0, 1, 0, 1}, Hn[2] = {NAN, 1.0}, Hok[2] = {2.0, 1.0};
    double re[das::POLY_MAX_DEGREE], im[das::POLY_MAX_DEGREE];
    if (das::poly_roots_host(small_eig, 2, Hz, 2, re, im, nullptr) != 0) bad++;
    if (das::poly_roots_host(small_eig, 1, Hn, 1, re, im, nullptr) != 0) bad++;
    if (das::poly_roots_host(nullptr, 1, Hok, 1, re, im, nullptr) != 0) bad++;
    if (das::poly_roots_host(small_eig, 1, Hok, 1, re, im, nullptr) != 1 || re[0] != 2.5) bad++;  // (h11^2 + h21^2) / h11
    std::printf(bad ? "FAILED (%d)\n" : "all checks held\n", bad);
    return bad ? 1 : 0;
}

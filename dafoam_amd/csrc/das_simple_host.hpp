// The SIMPLE sweep of das_simple_iteration and its inner Krylov solvers, written once over a small set of operations (simple_sweep<Ops>,
// simple_bicgstab<Ops>, simple_pcg<Ops>).  Host C++ only - no device code, no solver handle, no global state: das_device.hip supplies
// SimpleDeviceOps (kernel launches on the solver's stream), the test harness SimpleHostOps (host loops over the same das_simple.hpp
// bodies), and the CPU tier runs this very code.  Only the summation order of dot() differs between the two.
// Ops holds the mesh, ResParams, the storage and the choice of gradient kernel; the loops see the vectors as opaque double* (the member
// SimpleVecs v) and hand them back to Ops:
//   solvers, over the N cells:  ldu_mv(A, x, y, sign) [y = sign A x];  lin(y, a, x, b, z) [y = a x + b z];  bicg_p(p, r, beta, om, v)
//     [p = r + beta (p - om v)];  divdiag(out, in, diag, sign) [out = in / (sign diag)];  bicg_x(x, alpha, ph, om, sh, r, s, t)
//     [x += alpha ph + om sh, r = s - om t];  dot(a, b);  copy(dst, src, count);  zero(x, count)
//   sweep steps on the vectors of v:  grads_and_records(W) [nut, gU, gP, gN, fc, brec of the state W];  ueqn();  offdiag(W, cdIdx);
//     gather3(k) / scatter3(k) [component k of U: W -> x, dg, b / x -> Wn];  hbya();  pface();  peqn();  gradp();  flux();
//     relax(alphaP);  correct();  saeqn();  bound() [x -> nuTilda of Wn, DAUtility::boundVar]
#pragma once
#include <cmath>

namespace das {

// LDU matrix: per-cell diagonal, per-internal-face off-diagonals (row owner takes up[f], row neighbour lo[f]: body_ldu_row)
struct SimpleLdu { const double* diag; const double* up; const double* lo; };
struct SimpleIters { int U = 0, p = 0, nuTilda = 0; };  // inner iterations of one sweep

// every vector of one sweep (value-initialise).  n states, N cells, F faces, nIF internal faces; Wp / WnNu / WnPhi point into W / Wn
struct SimpleVecs {
    long long n, N, F, nIF;
    double *W, *Wp, *Wn, *WnNu, *WnPhi, *nut, *gU, *gP, *gN, *fc, *brec;  // the state and what grads_and_records fills: set by Ops
    double *D, *bd, *sb, *rhsU, *up, *lo, *rAU, *HbyA, *phiH, *gpf, *cp, *pbc, *dp, *rp, *x, *b, *dg, *pn, *phiN, *gPn;
    double *r, *r0, *p, *v, *s, *t, *ph, *sh;  // Krylov work (N each)
};
// take(count) returns storage for count doubles that the caller keeps alive; n = 0: the Krylov work alone
template <class Take>
inline void simple_alloc(SimpleVecs& v, long long n, long long N, long long F, long long nIF, Take take) {
    v.n = n; v.N = N; v.F = F; v.nIF = nIF;
    v.r = take(N); v.r0 = take(N); v.p = take(N); v.v = take(N); v.s = take(N); v.t = take(N); v.ph = take(N); v.sh = take(N);
    if (!n) return;
    v.Wn = take(n); v.D = take(N); v.bd = take(3 * N); v.sb = take(3 * N); v.rhsU = take(3 * N); v.up = take(nIF); v.lo = take(nIF); v.rAU = take(N); v.HbyA = take(3 * N);
    v.phiH = take(F); v.gpf = take(F); v.cp = take(nIF); v.pbc = take(4 * (F - nIF > 1 ? F - nIF : 1)); v.dp = take(N); v.rp = take(N); v.x = take(N); v.b = take(N);
    v.dg = take(N); v.pn = take(N); v.phiN = take(F); v.gPn = take(3 * N);
}

// Jacobi-preconditioned BiCGStab (convection-diffusion systems) on the LDU matrix; x holds the start vector; returns the iterations done
template <class Ops>
inline int simple_bicgstab(Ops& ops, const SimpleLdu& A, const double* b, double* x, double tol, int maxit) {
    const SimpleVecs& w = ops.v;
    ops.ldu_mv(A, x, w.r, 1.0);
    ops.lin(w.r, 1.0, b, -1.0, w.r);
    ops.copy(w.r0, w.r, w.N);
    ops.zero(w.p, w.N); ops.zero(w.v, w.N);
    const double bn = std::sqrt(ops.dot(b, b)) + 1e-300;
    double rho = 1.0, alpha = 1.0, om = 1.0;
    for (int it = 1; it <= maxit; it++) {
        if (std::sqrt(ops.dot(w.r, w.r)) <= tol * bn) return it - 1;
        const double rho1 = ops.dot(w.r0, w.r);
        if (rho1 == 0.0 || !std::isfinite(rho1)) return it - 1;  // breakdown: keep the iterate (right-hand sides that vanish to rounding end here)
        const double beta = (rho1 / rho) * (alpha / om);
        ops.bicg_p(w.p, w.r, beta, om, w.v);
        ops.divdiag(w.ph, w.p, A.diag, 1.0);
        ops.ldu_mv(A, w.ph, w.v, 1.0);
        alpha = rho1 / ops.dot(w.r0, w.v);
        ops.lin(w.s, 1.0, w.r, -alpha, w.v);
        if (std::sqrt(ops.dot(w.s, w.s)) <= tol * bn) {  // converged at the half step
            ops.lin(x, 1.0, x, alpha, w.ph);
            return it;
        }
        ops.divdiag(w.sh, w.s, A.diag, 1.0);
        ops.ldu_mv(A, w.sh, w.t, 1.0);
        om = ops.dot(w.t, w.s) / ops.dot(w.t, w.t);
        ops.bicg_x(x, alpha, w.ph, om, w.sh, w.r, w.s, w.t);
        rho = rho1;
    }
    return maxit;
}
// Jacobi-preconditioned conjugate gradients on sign * A (the pressure equation: A symmetric negative definite, sign = -1)
template <class Ops>
inline int simple_pcg(Ops& ops, const SimpleLdu& A, double sign, const double* b, double* x, double tol, int maxit) {
    const SimpleVecs& w = ops.v;
    ops.ldu_mv(A, x, w.r, 1.0);
    ops.lin(w.r, sign, b, -sign, w.r);
    const double bn = std::sqrt(ops.dot(b, b)) + 1e-300;
    double rz = 0.0;
    for (int it = 1; it <= maxit; it++) {
        if (std::sqrt(ops.dot(w.r, w.r)) <= tol * bn) return it - 1;
        ops.divdiag(w.ph, w.r, A.diag, sign);  // z
        const double rz1 = ops.dot(w.r, w.ph);
        if (it == 1) ops.copy(w.p, w.ph, w.N);
        else ops.lin(w.p, 1.0, w.ph, rz1 / rz, w.p);
        rz = rz1;
        ops.ldu_mv(A, w.p, w.v, sign);  // q = sign A p
        const double alpha = rz / ops.dot(w.p, w.v);
        ops.lin(x, 1.0, x, alpha, w.p);
        ops.lin(w.r, 1.0, w.r, -alpha, w.v);
    }
    return maxit;
}

// One SIMPLE iteration on ops.v.W (reference DASimpleFoam.C:123-185).  alphaP: explicit pressure relaxation; linTol: relative tolerance
// of the inner solves; maxLinUN / maxLinP: their iteration caps (momentum and nuTilda / pressure)
template <class Ops>
inline SimpleIters simple_sweep(Ops& ops, double alphaP, double linTol, int maxLinUN, int maxLinP) {
    const SimpleVecs& v = ops.v;
    SimpleIters its;
    // ---- momentum predictor (UEqnSimple.H)
    ops.grads_and_records(v.W);
    ops.ueqn(); ops.offdiag(v.W, 0);
    ops.copy(v.Wn, v.W, v.n);
    for (int k = 0; k < 3; k++) {
        ops.gather3(k);
        its.U += simple_bicgstab(ops, SimpleLdu{v.dg, v.up, v.lo}, v.b, v.x, linTol, maxLinUN);
        ops.scatter3(k);
    }
    // ---- pressure corrector (pEqnSimple.H)
    ops.hbya(); ops.pface();
    ops.copy(v.gPn, v.gP, 3 * v.N); ops.copy(v.pn, v.Wp, v.N);
    for (int corr = 0; corr < 2; corr++) {  // nNonOrthogonalCorrectors 1
        ops.peqn();
        its.p += simple_pcg(ops, SimpleLdu{v.dp, v.cp, v.cp}, -1.0, v.rp, v.pn, linTol, maxLinP);
        ops.gradp();
    }
    ops.flux(); ops.relax(alphaP); ops.gradp(); ops.correct();
    ops.copy(v.WnPhi, v.phiN, v.F);
    // ---- SA transport at the updated U / phi (DASpalartAllmaras::correct)
    ops.grads_and_records(v.Wn);
    ops.saeqn(); ops.offdiag(v.Wn, 1);
    ops.copy(v.x, v.WnNu, v.N);
    its.nuTilda += simple_bicgstab(ops, SimpleLdu{v.dg, v.up, v.lo}, v.b, v.x, linTol, maxLinUN);
    ops.bound();
    ops.copy(v.W, v.Wn, v.n);
    return its;
}

}  // namespace das

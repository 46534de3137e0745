// meshQualityKS and residualNorm (reference DAFunctionMeshQualityKS.C, DAFunctionResidualNorm.C): the two objective functions whose terms
// run over the whole mesh instead of over a patch or a cell set.
//
// meshQualityKS:  F = log( sum_f exp(k a_f) ) / k over ALL faces, internal and boundary, a_f one of three per-face metrics.  The reference
// takes them from OpenFOAM's polyMeshTools::faceOrthogonality / faceSkewness, which is not vendored: body_mesh_quality restates them from
// OpenFOAM v1812 (not machine-checked against a build of it).  R = ROOTVSMALL, own / nei = cell centres, Sf / Cf = face area vector / centre:
//   faceOrthogonality  internal: d = nei - own, a = (d . Sf) / (|d| |Sf| + R);  boundary: exactly 1
//   nonOrthoAngle      that value clamped to [-(1 - 1e-6), 1 - 1e-6] (DAFunctionMeshQualityKS.C:117-129; a clamped face is the constant
//                      bound: tangent exactly 0), a = acos(val) 180 / pi
//   faceSkewness       internal: Cpf = Cf - own, d = nei - own, sv = Cpf - ((Sf . Cpf) / ((Sf . d) + R)) d, svHat = sv / (|sv| + R),
//                      fd = max(0.2 |d| + R, max over the face's points p of |svHat . (p - Cf)|), a = |sv| / fd
//                      boundary: the same with n = Sf / (|Sf| + R), d = n (n . Cpf) and 0.4 |d| in place of 0.2 |d|
//                      The maximum takes the floor term first, then the points in their stored order; the first maximum wins and the
//                      tangent follows the winner.  |sv| = 0 exactly: the tangent of |sv| is 0 (dsqrt).
// The body is templated on the scalar of points and metrics like geom_face: double for the value, Dual<1> in the mesh-sensitivity product,
// where k_mq_metric writes (softmax weight of the base mesh) x (tangent of a_f) and k_mq_owner_gather adds the faces a cell owns into the
// per-cell array k_vc_gather consumes.  The KS reduction is the two-stage fixed-order one of das_facefn.hpp.  No atomics.
//
// residualNorm:  L2Norm F = sqrt( sum_i w_i^2 R_i^2 ), L1Norm F = sum_i |w_i R_i| over all residual rows, w_i the weight of the row's
// residual block.  The internal faces of phiRes contribute w^2 R^2 in EITHER mode: the reference's loop over them has no mode switch
// (DAFunctionResidualNorm.C:146-149) - kept.  k_rn_terms forms the terms, k_rn_partial + k_ks_sum_final add them in a fixed order;
// k_rn_seeds forms g = coef dF/dR, the seed vector of the existing  input -> residual  products.
#pragma once
#include "das_geom.hpp"
#include "das_jaccon.hpp"
#include "das_kernels.hpp"
#ifdef __HIPCC__
#include "das_facefn.hpp"
#endif

namespace das {

#define DAS_MQ_ORTHO 0
#define DAS_MQ_NONORTHO 1
#define DAS_MQ_SKEW 2

DAS_HD double dacos(double a) { return acos(a); }
template <int K>
DAS_HD Dual<K> dacos(const Dual<K>& a) {
    Dual<K> r;
    r.v = acos(a.v);
    const double g = -1.0 / sqrt(1.0 - a.v * a.v);
#pragma unroll
    for (int k = 0; k < K; k++) r.d[k] = g * a.d[k];
    return r;
}

template <class S>
DAS_HD S mq_dot(const S* a, const S* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// a_f of face f (S: double, or Dual<1> when the points and the metrics carry tangents); P is read by faceSkewness only
template <class S>
DAS_HD S body_mesh_quality(int f, const GeomTopo& t, const S* __restrict__ P, const FaceGeomT<S>* __restrict__ fg, const CellGeomT<S>* __restrict__ cg,
                           int metric) {
    const FaceGeomT<S>& g = fg[f];
    const S* own = cg[t.owner[f]].C;
    const bool internal = f < t.nIF;
    if (metric != DAS_MQ_SKEW) {
        S v(1.0);
        if (internal) {
            const S* nei = cg[t.neigh[f]].C;
            const S d[3] = {nei[0] - own[0], nei[1] - own[1], nei[2] - own[2]};
            v = mq_dot(d, g.Sf) / (dsqrt(mq_dot(d, d)) * g.magSf + DAS_ROOTVSMALL);
        }
        if (metric == DAS_MQ_ORTHO) return v;
        const double bound = 1.0 - 1e-6;
        if (val(v) > bound) v = S(bound);
        if (val(v) < -bound) v = S(-bound);
        return dacos(v) * 180.0 / 3.14159265358979323846;
    }
    const S Cpf[3] = {g.Cf[0] - own[0], g.Cf[1] - own[1], g.Cf[2] - own[2]};
    S d[3];
    if (internal) {
        const S* nei = cg[t.neigh[f]].C;
        for (int k = 0; k < 3; k++) d[k] = nei[k] - own[k];
    } else {
        const S im = 1.0 / (g.magSf + DAS_ROOTVSMALL);
        const S n[3] = {g.Sf[0] * im, g.Sf[1] * im, g.Sf[2] * im};
        const S nc = mq_dot(n, Cpf);
        for (int k = 0; k < 3; k++) d[k] = n[k] * nc;
    }
    const S r = mq_dot(g.Sf, Cpf) / (mq_dot(g.Sf, d) + DAS_ROOTVSMALL);
    const S sv[3] = {Cpf[0] - r * d[0], Cpf[1] - r * d[1], Cpf[2] - r * d[2]};
    const S magSv = dsqrt(mq_dot(sv, sv));
    const S is = 1.0 / (magSv + DAS_ROOTVSMALL);
    const S svHat[3] = {sv[0] * is, sv[1] * is, sv[2] * is};
    S fd = (internal ? 0.2 : 0.4) * dsqrt(mq_dot(d, d)) + DAS_ROOTVSMALL;
    for (int i = t.face_ptr[f]; i < t.face_ptr[f + 1]; i++) {
        const S* p = P + 3 * (long long)t.face_pts[i];
        const S e[3] = {p[0] - g.Cf[0], p[1] - g.Cf[1], p[2] - g.Cf[2]};
        const S c = dabs(mq_dot(svHat, e));
        if (val(c) > val(fd)) fd = c;  // the first maximum wins
    }
    return magSv / fd;
}

// what a pass stores per face: the value, or in the dual pass the tangent times the weight of the face
DAS_HD double mq_store(double a, const double*, int) { return a; }
DAS_HD double mq_store(const Dual<1>& a, const double* __restrict__ w, int f) { return w[f] * a.d[0]; }

#ifdef __HIPCC__
// one thread per face: out[f] = a_f (S = double; w unused) or w_f a_f' (S = Dual<1>)
template <class S>
__global__ __launch_bounds__(256) void k_mq_metric(GeomTopo t, const S* __restrict__ P, const FaceGeomT<S>* __restrict__ fg, const CellGeomT<S>* __restrict__ cg,
                                                   int metric, const double* __restrict__ w, double* __restrict__ out) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < t.nF) out[f] = mq_store(body_mesh_quality<S>(f, t, P, fg, cg, metric), w, f);
}
// tc[c] = sum of ft over the faces cell c owns, in the order of its face list (every face has one owner: each ft is added once)
__global__ __launch_bounds__(256) void k_mq_owner_gather(int nC, const int* __restrict__ cf_ptr, const int* __restrict__ cf_face, const double* __restrict__ ft,
                                                         double* __restrict__ tc) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nC) return;
    double acc = 0.0;
    for (int s = cf_ptr[c]; s < cf_ptr[c + 1]; s++) {
        const int fe = cf_face[s];
        if (fe >= 0) acc += ft[fe];  // fe < 0: the cell is the face's neighbour
    }
    tc[c] = acc;
}
#endif  // __HIPCC__

// ---- residualNorm ---------------------------------------------------------------------------------------------------------------------
struct RnRows {  // the residual blocks in DAIndex "state" ordering (as RowLayout holds them) with their weights
    int nb;
    long long off[8];
    int kind[8];
    long long nC, nF, nIF;
    double w[8];
    int l1;  // resMode L1Norm
};
// the weight of row i; internalPhi: the row is an internal face of a surface-flux block
DAS_HD double rn_row_weight(const RnRows& r, long long i, bool& internalPhi) {
    internalPhi = false;
    for (int b = 0; b < r.nb; b++) {
        const long long len = r.kind[b] == KIND_VEC ? 3 * r.nC : r.kind[b] == KIND_SCL ? r.nC : r.nF;
        const long long q = i - r.off[b];
        if (q >= 0 && q < len) {
            internalPhi = r.kind[b] != KIND_VEC && r.kind[b] != KIND_SCL && q < r.nIF;
            return r.w[b];
        }
    }
    return 0.0;
}
DAS_HD double rn_term(const RnRows& r, long long i, double R) {
    bool ip;
    const double w = rn_row_weight(r, i, ip);
    return (r.l1 && !ip) ? fabs(w * R) : w * w * R * R;
}
// dF/dR_i up to the common factor: L2 w^2 R / F;  L1 |w| sign(R) (0 at R = 0), internal phi rows 2 w^2 R
DAS_HD double rn_seed(const RnRows& r, long long i, double R, double F) {
    bool ip;
    const double w = rn_row_weight(r, i, ip);
    if (!r.l1) return w * w * R / F;
    if (ip) return 2.0 * w * w * R;
    return R > 0.0 ? fabs(w) : R < 0.0 ? -fabs(w) : 0.0;
}
#ifdef __HIPCC__
__global__ __launch_bounds__(256) void k_rn_terms(long long n, RnRows r, const double* __restrict__ R, double* __restrict__ term) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) term[i] = rn_term(r, i, R[i]);
}
__global__ __launch_bounds__(256) void k_rn_seeds(long long n, RnRows r, const double* __restrict__ R, double F, double coef, double* __restrict__ g) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] = coef * rn_seed(r, i, R[i], F);
}
// stage 1 of the sum: part[b] = the block's share of sum_i term_i (grid-stride, fixed order); k_ks_sum_final adds the partials
__global__ __launch_bounds__(256) void k_rn_partial(long long n, const double* __restrict__ term, double* __restrict__ part) {
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) acc += term[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ double sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// ---- launch helpers (ks_blocks, launch_ks_sum_final: das_facefn.hpp).  part holds DAS_FACEFN_MAX_BLOCKS entries, ms two ----------------
// term[i] = the term of row i, ms[1] = their fixed-order sum; part[0 .. ks_blocks(n)) = the per-workgroup sums
static void launch_rn_sum(hipStream_t st, long long n, const RnRows& r, const double* R, double* term, double* part, double* ms) {
    const int nb = ks_blocks(n);
    hipLaunchKernelGGL(k_rn_terms, dim3(nblk(n, 256)), dim3(256), 0, st, n, r, R, term);
    hipLaunchKernelGGL(k_rn_partial, dim3(nb), dim3(256), 0, st, n, (const double*)term, part);
    launch_ks_sum_final(st, nb, part, ms);
}
static void launch_rn_seeds(hipStream_t st, long long n, const RnRows& r, const double* R, double F, double coef, double* g) {
    hipLaunchKernelGGL(k_rn_seeds, dim3(nblk(n, 256)), dim3(256), 0, st, n, r, R, F, coef, g);
}
static void launch_mq_owner_gather(hipStream_t st, int nC, const int* cf_ptr, const int* cf_face, const double* ft, double* tc) {
    hipLaunchKernelGGL(k_mq_owner_gather, dim3(nblk(nC, 256)), dim3(256), 0, st, nC, cf_ptr, cf_face, ft, tc);
}

#endif  // __HIPCC__

}  // namespace das

// forceCouplingOutput (reference src/adjoint/DAOutput/DAOutputForceCoupling.C): the force of every face of the named patches,
//   F_f = S_f (p_b - pRef) + S_f . devRhoReff_b      (body_force_vec, das_kernels.hpp),
// handed in equal shares F_f / nPoints_f to the points of the face (:142-191).  The output lists the points patch by patch (the patches
// sorted by name, :41), in ascending mesh-point index inside a patch (:194-201), as [fx0, fy0, fz0, fx1, ...] (:207-214); a point that
// two of the patches share appears once per patch, and each copy receives its own patch's faces only.
// Three kernels, no atomics: the value is the same bits on every call.
//   k_fc_face_force  one thread per face slot: F_f -> ff[3 k ..]
//   k_fc_nodal       one thread per output point: sum over its face slots (CSR, ascending slot) of F_f / nPoints_f
//   k_fc_seed_dir    one thread per face slot: d_f = (sum of the seeds of its output points) / nPoints_f.  With these directions and
//                    unit weights  seeds . output = sum_f d_f . F_f  - a force functional with a per-face direction, which is what
//                    k_fn_grad / k_fn_tangent / k_fn_dual differentiate.
#pragma once
#include "das_kernels.hpp"

namespace das {

template <bool RHO>
__global__ __launch_bounds__(256) void k_fc_face_force(DevMesh m, ResParams prm, const double* __restrict__ W, const double* nut, const double* gU,
                                                       int nf, const int* __restrict__ faces, double pRef, double* __restrict__ ff) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nf) return;
    double F[3];
    body_force_vec<double, RHO>(faces[k], m, prm, W, nut, gU, pRef, F);
    ff[3LL * k] = F[0]; ff[3LL * k + 1] = F[1]; ff[3LL * k + 2] = F[2];
}
// ptr / slot: output point -> face slots; fptr: face slot -> its output points, fptr[k + 1] - fptr[k] = nPoints_f
__global__ __launch_bounds__(256) void k_fc_nodal(int nOut, const int* __restrict__ ptr, const int* __restrict__ slot, const int* __restrict__ fptr,
                                                  const double* __restrict__ ff, double* __restrict__ out) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= nOut) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int q = ptr[o]; q < ptr[o + 1]; q++) {
        const int k = slot[q];
        const double n = (double)(fptr[k + 1] - fptr[k]);
        a0 += ff[3LL * k] / n; a1 += ff[3LL * k + 1] / n; a2 += ff[3LL * k + 2] / n;
    }
    out[3LL * o] = a0; out[3LL * o + 1] = a1; out[3LL * o + 2] = a2;
}
// ptr / opt: face slot -> its output points (ptr[k + 1] - ptr[k] = nPoints_f)
__global__ __launch_bounds__(256) void k_fc_seed_dir(int nf, const int* __restrict__ ptr, const int* __restrict__ opt, const double* __restrict__ seeds,
                                                     double* __restrict__ dir) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nf) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int q = ptr[k]; q < ptr[k + 1]; q++) {
        const long long o = opt[q];
        a0 += seeds[3 * o]; a1 += seeds[3 * o + 1]; a2 += seeds[3 * o + 2];
    }
    const double n = (double)(ptr[k + 1] - ptr[k]);
    dir[3LL * k] = a0 / n; dir[3LL * k + 1] = a1 / n; dir[3LL * k + 2] = a2 / n;
}

}  // namespace das

// thermalCouplingOutput (reference src/adjoint/DAOutput/DAOutputThermalCoupling.C, discipline aero): what the fluid side of a conjugate
// heat transfer loop sends out.  With nF the faces of the named patches (the patches sorted by name, :40, each in face order):
//   out[k]      = T of the owner cell of face k                      (:79-92)
//   out[nF + k] = kappa / d = Cp alphaEff_b deltaCoeff on face k      (:94-211; body_thermal_coupling, das_kernels.hpp)
// The output: two kernels, no atomics - every entry is one plain store of one thread, the same bits on every call.
//   k_tc_values    one thread per face slot fills its entry of both halves
//   k_tc_seed_dir  one thread per face slot: d_f = (seeds[k], seeds[nF + k], 0).  With these directions and unit weights
//                  seeds . output = sum_f (d_f[0] T_c + d_f[1] kappa / d)  - the face functional of kind DAS_FN_THERMALCOUPLING, which is
//                  what k_fn_grad / k_fn_tangent / k_fn_dual differentiate.
// thermalCoupling input (reference src/adjoint/DAInput/DAInputThermalCoupling.C): what the fluid side takes in, written into the per-face
// records {refValue, valueFraction, d refValue, d valueFraction} of the mixed T patches (DevMeshT::mixed):
//   k_tc_set_mixed   refValue = in[k] (:76-93), valueFraction = nk / (myK + nk) with nk = in[nF + k] and myK the kappa / d k_tc_values
//                    has just written for the same face (:95-222); the fraction then stays as it is until the input is set again
//   k_tc_seed_mixed  the forward-mode seed of one derivative pass: d refValue or d valueFraction of the listed face slots
//   k_tc_gather      per listed face slot, sum over the rows r that read T of its owner cell (the transposed structure of dRdW) of
//                    psi_r dR_r: [d R / d refValue_f]^T psi, one thread per face in the order of the structure - no atomics
#pragma once
#include "das_kernels.hpp"

namespace das {

template <bool RHO, bool SOLID = false>
__global__ __launch_bounds__(256) void k_tc_values(DevMesh m, ResParams prm, const double* __restrict__ W, const double* nut, int nf,
                                                   const int* __restrict__ faces, int custom, double* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nf) return;
    double Tnear, kd;
    if constexpr (SOLID) body_thermal_coupling_solid<double>(faces[k], m, prm, W, custom != 0, Tnear, kd);  // discipline thermal
    else body_thermal_coupling<double, RHO>(faces[k], m, prm, W, nut, custom != 0, Tnear, kd);
    out[k] = Tnear;
    out[(long long)nf + k] = kd;
}
__global__ __launch_bounds__(256) void k_tc_seed_dir(int nf, const double* __restrict__ seeds, double* __restrict__ dir) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nf) return;
    dir[3LL * k] = seeds[k]; dir[3LL * k + 1] = seeds[(long long)nf + k]; dir[3LL * k + 2] = 0.0;
}

__global__ __launch_bounds__(256) void k_tc_set_mixed(int nf, const int* __restrict__ faces, int nIF, const double* __restrict__ in,
                                                      const double* __restrict__ myK, double* __restrict__ mixed) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nf) return;
    double* mx = mixed + 4LL * (faces[k] - nIF);
    const double nk = in[(long long)nf + k];
    mx[0] = in[k]; mx[1] = nk / (myK[k] + nk); mx[2] = 0.0; mx[3] = 0.0;
}
// sel: the face slots of the pass (null: all nf of them); which: 2 = d refValue, 3 = d valueFraction
__global__ __launch_bounds__(256) void k_tc_seed_mixed(int cnt, const int* __restrict__ sel, const int* __restrict__ faces, int nIF, int which, double v,
                                                       double* __restrict__ mixed) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cnt) return;
    mixed[4LL * (faces[sel ? sel[q] : q] - nIF) + which] = v;
}
// colOff: the index of T of cell 0 among the states; trp / tcol: state j -> the residual rows that read it
__global__ __launch_bounds__(256) void k_tc_gather(int cnt, const int* __restrict__ sel, const int* __restrict__ faces, const int* __restrict__ owner,
                                                   long long colOff, const long long* __restrict__ trp, const int* __restrict__ tcol,
                                                   const double* __restrict__ psi, const Dual<1>* __restrict__ Rd, double* __restrict__ out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cnt) return;
    const int k = sel[q];
    const long long j = colOff + owner[faces[k]];
    double acc = 0.0;
    for (long long e = trp[j]; e < trp[j + 1]; e++) acc += psi[tcol[e]] * Rd[tcol[e]].d[0];
    out[k] = acc;
}

}  // namespace das

// MI355X device driver of the adjoint hot path: kernel launches, coloured Jacobian assembly (dual numbers / FD),
// transposed-CSR SpMV (dRdW^T psi), restricted-additive-Schwarz + ILU(k) preconditioner (one workgroup per block, block
// vector in LDS), the on-device restarted GMRES, objective/boundary-input derivatives, exported through the C-ABI of
// include/dafoam_amd.h.  gfx950 only.  The dense host algebra of the GMRES solvers (no device code) is in das_gmres_host.hpp.
//
// Reference orchestration being replaced (file:line):
//   DASolver::calcdRdWT                         src/adjoint/DASolver/DASolver.C:948-1089
//   DAPartDeriv::calcPartDerivMat/perturbStates/setPartDerivMat  src/adjoint/DAPartDeriv/DAPartDeriv.C:42-208,350-473
//   DASolver::dRdWTMatVecMultFunction           src/adjoint/DASolver/DASolver.C:1364-1409
//   DASolver::calcJacTVecProduct                src/adjoint/DASolver/DASolver.C:1690-1839
//   DALinearEqn::createMLRKSP / solveLinearEqn  src/adjoint/DALinearEqn/DALinearEqn.C:28-437
#include <algorithm>
#include <cmath>
#include <ctime>
#include <functional>
#include <numeric>
#include <thread>

#include "das_case.hpp"
#include "das_jaccon.hpp"
#include "das_bilu.hpp"
#include "das_rcb.hpp"
#include "das_comm.hpp"
#include "das_krylov.hpp"
#include "das_gmres_host.hpp"
#include "das_block.hpp"
#include "das_krylov_debug.hpp"
#include "das_idr.hpp"
#include "das_idr_debug.hpp"
#include "das_poly.hpp"
#include "das_poly_debug.hpp"
#include "das_bilu_debug.hpp"
#include "das_graph_debug.hpp"
#include "das_coarse.hpp"
#include "das_coarse_debug.hpp"
#include "das_color.hpp"
#include "das_color_debug.hpp"
#include "das_opmat.hpp"
#include "das_graph.hpp"
#include "das_volcoord.hpp"
#include "das_cellfn.hpp"
#include "das_facefn.hpp"
#include "das_meshquality.hpp"
#include "das_forcecoupling.hpp"
#include "das_thermalcoupling.hpp"
#include "das_heatsource.hpp"
#include "das_actuatordisk.hpp"
#include "das_regression.hpp"
#include "das_reduce.hpp"
#include "das_reduce_debug.hpp"
#include "das_simple.hpp"
#include "das_simple_host.hpp"

#include <omp.h>

namespace das {

// =====================================================================================================
// kernel wrappers around the templated bodies
// =====================================================================================================
// (Round 3, measured and dropped - profiles/r03m_tile_launch_order_2M_rejected.log: a tile launch order for these kernels - cells
// grouped into compact RCB tiles, natural order inside, XCD-aware block -> tile mapping so that one XCD's L2 sees one region.  With
// tiles of individually sorted cells every kernel got 25-40 % slower (13-cell runs: partial lines); with 64-cell memory runs as the
// unit the assembly of dRdWT took 1.26 s against 1.19 s in the natural order.  The k+-1 neighbours that miss the 4 MB L2 are served
// by the 256 MB Infinity Cache; the kernels already run at ~5.5 TB/s of their FETCH_SIZE traffic.)
template <class T, bool RHO, class G = double>
__global__ __launch_bounds__(256) void k_grad(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, T* nut, T* gU, T* gP, T* gN, T* gH) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_grad<T, RHO>(c, m, prm, W, nut, gU, gP, gN, gH, (T*)prm.wTU);
}
// Round 5 (north_star: "owner/neighbour gather staged through LDS, wavefront segmented reductions for cell accumulation"): the Gauss
// gradients face-parallel.  A workgroup owns CPB consecutive cells; EIGHT lanes per cell, lane (cell, slot) evaluates face slot `slot`
// (slot + 8, ... for polyhedra) - the dependent chain cf_face -> face record -> neighbour state of the one-thread-per-cell kernel runs
// for all faces of a cell at once (its six-trip loop was the latency of k_grad: ~1.3 GB moved in 0.45 ms, neither bandwidth nor ALU).
//   stage 1  the states [U | p | nuTilda] of the CPB cells are staged in LDS (coalesced); a face whose other cell lies in the tile reads it
//            from there (the +-1 neighbours along the numbering), everyone else from global memory
//   stage 2  every lane writes its 15 products S_f (x) {U_f, p_f, nuTilda_f} to LDS, [cell][slot][quantity]
//   stage 3  segmented reduction: the 15 x CPB sums over the 8 slots, in slot order (deterministic), scaled by 1 / V and written to
//            gradU / gradP / gradN with consecutive threads on consecutive addresses (the old kernel stored with a 72-byte lane stride)
// DASimpleFoam without the T field and double metrics (the benchmark path); every other variant keeps k_grad.  amd.gradFaceParallel 0 = off.
template <class T, int CPB>
__global__ __launch_bounds__(CPB * 8) void k_grad_fp(DevMesh m, ResParams prm, const T* __restrict__ W, T* __restrict__ nut, T* __restrict__ gU,
                                                     T* __restrict__ gP, T* __restrict__ gN) {
    extern __shared__ double sh_raw[];
    T* const tile = reinterpret_cast<T*>(sh_raw);   // [5][CPB]
    T* const part = tile + 5 * CPB;                 // [CPB][8][15]
    const long long N = m.nC;
    const int c0 = blockIdx.x * CPB;
    const int nT = min(CPB, m.nC - c0);
    for (int i = threadIdx.x; i < 5 * CPB; i += CPB * 8) {
        const int q = i / CPB, cl = i - q * CPB;
        if (cl < nT) tile[i] = q < 3 ? W[3LL * (c0 + cl) + q] : W[(q == 3 ? prm.offP : prm.offN) * N + c0 + cl];
    }
    __syncthreads();
    const int cl = threadIdx.x >> 3, slot = threadIdx.x & 7, c = c0 + cl;
    T acc[15];
#pragma unroll
    for (int q = 0; q < 15; q++) acc[q] = T(0.0);
    if (cl < nT) {
        const T Uc[3] = {tile[cl], tile[CPB + cl], tile[2 * CPB + cl]};
        const T pc = tile[3 * CPB + cl], nc = tile[4 * CPB + cl];
        const T nut_c = nc * fv1_of<T>(nc / T(prm.nu));
        if (slot == 0) nut[c] = nut_c;
        T gH[3];  // (no energy-like scalar on this path)
        for (int s = m.cf_ptr[c] + slot; s < m.cf_ptr[c + 1]; s += 8)
            grad_face<T, false, double>(c, s, m, prm, W, Uc, pc, T(0.0), nc, nut_c, false, acc, acc + 9, acc + 12, gH, tile, c0, CPB);
    }
#pragma unroll
    for (int q = 0; q < 15; q++) part[(cl * 8 + slot) * 15 + q] = acc[q];  // [cell][slot][quantity]: a lane's 15 values are contiguous (stride 15: no bank conflicts)
    __syncthreads();
    for (int o = threadIdx.x; o < 15 * CPB; o += CPB * 8) {
        // output o of the tile: gradU entries first (9 per cell, cell-major like the global array), then gradP, then gradN
        int q, oc;
        T* dst;
        if (o < 9 * CPB) { oc = o / 9; q = o - 9 * oc; dst = gU + 9LL * c0 + o; }
        else if (o < 12 * CPB) { const int r = o - 9 * CPB; oc = r / 3; q = 9 + r - 3 * oc; dst = gP + 3LL * c0 + r; }
        else { const int r = o - 12 * CPB; oc = r / 3; q = 12 + r - 3 * oc; dst = gN + 3LL * c0 + r; }
        if (oc >= nT) continue;
        // (round 5, first layout [quantity][cell][slot]: neighbouring threads read 2 KB apart - every lane of a group on one bank; the dual-number
        //  variant ran at 0.98 ms against 0.57 for k_grad, profiles/r06e_*.  Here neighbouring threads read neighbouring quantities.)
        const T* ps = part + oc * 8 * 15 + q;
        T sum = ps[0];
#pragma unroll
        for (int t = 1; t < 8; t++) sum += ps[15 * t];
        *dst = sum * (1.0 / m.cg[c0 + oc].V);
    }
}
// SRC: with the momentum source of the actuator disks (m.src3 set); the kernels without it are the ones of before
// DDT: with the fvm::ddt terms of DAPimpleFoam (prm.ddt, prm.W0 / prm.W00 set); the same holds
template <class T, bool RHO, class G = double, bool SRC = false, bool DDT = false>
__global__ __launch_bounds__(256) void k_cell(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, const T* nut, const T* gU, const T* gP,
                                              const T* gN, const T* gH, T* R, T* rAU, T* HbyA) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_cell<T, RHO, G, SRC, DDT>(c, m, prm, W, nut, gU, gP, gN, gH, R, rAU, HbyA, (const T*)prm.wTU);
}
// DAPimpleFoam: s o [dR/dW0]^T psi or s o [dR/dW00]^T psi (body_drdwold); one thread per cell, the p and phi entries are the caller's zeros
__global__ __launch_bounds__(256) void k_drdwold(DevMesh m, ResParams prm, double coef, const double* __restrict__ rAU, const double* __restrict__ psi,
                                                 const double* __restrict__ scale, double* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_drdwold(c, m, prm, coef, rAU, psi, scale, out);
}
// Round 6: the cell pass of DASimpleFoam split the finite-volume way (das_kernels.hpp body_fcoef / body_bcoef / body_cell2): every
// internal face evaluated ONCE by its own thread (the monolithic k_cell evaluates it from both sides inside a serial six-trip loop that
// nothing hides at one wave per SIMD), six scalars per face handed to a light per-cell pass.
template <class T>
__global__ __launch_bounds__(256) void k_fcoef(DevMesh m, ResParams prm, const T* __restrict__ W, const T* __restrict__ nut, const T* __restrict__ gU,
                                               const T* __restrict__ gN, T* __restrict__ fc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < m.nIF) body_fcoef<T>(f, m, prm, W, nut, gU, gN, fc);
}
template <class T>
__global__ __launch_bounds__(256) void k_bcoef(DevMesh m, ResParams prm, const T* __restrict__ W, const T* __restrict__ nut, const T* __restrict__ gU,
                                               T* __restrict__ brec) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < m.nF - m.nIF) body_bcoef<T>(b, m, prm, W, nut, gU, brec);
}
template <class T, bool SRC = false>
__global__ __launch_bounds__(256) void k_cell2(DevMesh m, ResParams prm, const T* __restrict__ W, const T* __restrict__ nut, const T* __restrict__ gU,
                                               const T* __restrict__ gP, const T* __restrict__ gN, const T* __restrict__ fc, const T* __restrict__ brec,
                                               T* __restrict__ R, T* __restrict__ rAU, T* __restrict__ HbyA) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_cell2<T, SRC>(c, m, prm, W, nut, gU, gP, gN, fc, brec, R, rAU, HbyA);
}
template <class T, bool RHO, class G = double>
__global__ __launch_bounds__(256) void k_face(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, const T* nut, const T* gP, const T* rAU,
                                              const T* HbyA, T* q, T* R) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < m.nF) body_face<T, RHO>(f, m, prm, W, nut, gP, rAU, HbyA, q, R);
}
template <class T, bool RHO, class G = double>
__global__ __launch_bounds__(256) void k_pres(DevMeshT<G> m, ResParams prm, const T* q, T* R) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_pres<T, RHO>(c, m, prm, q, R);
}
// face-integral objectives: value (atomic sums per group), forward-mode tangent, coloured dual-number gradient scatter
// (deterministic: per-face / per-block values first, then ONE workgroup sums them in a fixed order - the atomicAdd versions of
//  round 2 summed in arrival order)
template <bool RHO, bool SOLID = false>
__global__ __launch_bounds__(256) void k_fn_value(DevMesh m, ResParams prm, const double* __restrict__ W, const double* nut, const double* gU,
                                                  FaceFnView fn, double* __restrict__ fv) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= fn.nf) return;
    double dir[3] = {0.0, 0.0, 0.0};
    if (fn.dir) { dir[0] = fn.dir[3 * k]; dir[1] = fn.dir[3 * k + 1]; dir[2] = fn.dir[3 * k + 2]; }
    fv[k] = fn.w[k] * facefn_of<double, RHO, SOLID>(fn.faces[k], m, prm, W, nut, gU, fn.kind, dir, fn.gammaFn, fn.RFn, fn.loc, fn.pRef);
}
// (the group sum of the per-face summands: k_group_sum, das_reduce.hpp)
// tangent of the objective for seeded boundary values (dF/d(BC value), one forward pass): per-face summands
template <bool RHO, bool SOLID = false>
__global__ __launch_bounds__(256) void k_fn_tangent(DevMesh m, ResParams prm, const Dual<1>* __restrict__ W, const Dual<1>* nut, const Dual<1>* gU,
                                                    FaceFnView fn, double seed, double* __restrict__ fv) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= fn.nf) return;
    double dir[3] = {0.0, 0.0, 0.0};
    if (fn.dir) { dir[0] = fn.dir[3 * k]; dir[1] = fn.dir[3 * k + 1]; dir[2] = fn.dir[3 * k + 2]; }
    Dual<1> v = facefn_of<Dual<1>, RHO, SOLID>(fn.faces[k], m, prm, W, nut, gU, fn.kind, dir, fn.gammaFn, fn.RFn, fn.loc, fn.pRef);
    fv[k] = seed * fn.w[k] * v.d[0];
}
// the derivative of q_f w.r.t. the (unique) state of colour `col` in the stencil of face f (cell c and its face
// neighbours: U, p, (T), nuTilda) is accumulated into dFdW
template <bool RHO, bool SOLID = false>
__global__ __launch_bounds__(256) void k_fn_grad(DevMesh m, ResParams prm, const Dual<1>* __restrict__ W, const Dual<1>* nut, const Dual<1>* gU,
                                                 FaceFnView fn, double seed, const int* __restrict__ colors, int col, double* dFdW) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= fn.nf) return;
    double dir[3] = {0.0, 0.0, 0.0};
    if (fn.dir) { dir[0] = fn.dir[3 * k]; dir[1] = fn.dir[3 * k + 1]; dir[2] = fn.dir[3 * k + 2]; }
    const int f = fn.faces[k];
    Dual<1> v = facefn_of<Dual<1>, RHO, SOLID>(f, m, prm, W, nut, gU, fn.kind, dir, fn.gammaFn, fn.RFn, fn.loc, fn.pRef);
    if (v.d[0] == 0.0) return;
    const double g = seed * fn.w[k] * v.d[0];
    const long long N = m.nC;
    const int c = m.owner[f];
    if constexpr (SOLID) {  // the one-block layout [T]: the summand of a face reads T of its owner cell alone
        if (colors[c] == col) atomicAdd(&dFdW[c], g);
        return;
    }
    const int nsc = prm.offPhi - 3;  // scalar cell blocks after U (p, [T], nuTilda)
    auto try_cell = [&](int x) -> bool {
        for (int q = 0; q < 3; q++) if (colors[3LL * x + q] == col) { atomicAdd(&dFdW[3LL * x + q], g); return true; }
        for (int b = 0; b < nsc; b++) if (colors[(3 + b) * N + x] == col) { atomicAdd(&dFdW[(3 + b) * N + x], g); return true; }
        return false;
    };
    if (try_cell(c)) return;
    for (int s = m.cf_ptr[c]; s < m.cf_ptr[c + 1]; s++) {
        int o = m.cf_other[s];
        if (o >= 0 && try_cell(o)) return;
    }
}

template <class T, class G = double>
__global__ __launch_bounds__(256) void k_gradT(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, const double* phiF, T* gT) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_gradT<T>(c, m, prm, W, phiF, gT);
}
template <class T, class G = double>
__global__ __launch_bounds__(256) void k_T(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, const double* phiF, const double* Told,
                                           const T* gT, T* R) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_T<T>(c, m, prm, W, phiF, Told, gT, R);
}

// DAHeatTransferFoam: Gauss gradient of T, then TRes = laplacian(kappa(T), T) (body_heat_grad / body_heat); one thread per cell
template <class T, class G = double>
__global__ __launch_bounds__(256) void k_heat_grad(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, T* gT) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_heat_grad<T>(c, m, prm, W, gT);
}
template <class T, class G = double>
__global__ __launch_bounds__(256) void k_heat(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, const T* gT, T* R) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_heat<T>(c, m, prm, W, gT, R);
}

// DASolidDisplacementFoam (body_solid_grad / body_solid_traction / body_solid): the Gauss gradient of D with the pass-0 boundary values
// over all cells, the lagged tractionDisplacement passes over the compact list of the cells that own a traction face (they overwrite
// gradD of those cells and leave the final g per traction face), then DRes; one thread per cell, no atomics
template <class T, class G = double>
__global__ __launch_bounds__(256) void k_solid_grad(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, T* gD) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_solid_grad<T>(c, m, prm, W, gD);
}
template <class T, class G = double>
__global__ __launch_bounds__(256) void k_solid_traction(DevMeshT<G> m, ResParams prm, T* gD, T* gTr) {
    int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < prm.nTrac) body_solid_traction<T>(k, m, prm, gD, gTr);
}
template <class T, class G = double>
__global__ __launch_bounds__(256) void k_solid(DevMeshT<G> m, ResParams prm, const T* __restrict__ W, const T* gD, const T* gTr, T* R) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_solid<T>(c, m, prm, W, gD, gTr, R);
}
// the gradient passes of DASolidDisplacementFoam into wk.gU (9 per cell) and wk.gTr (3 per boundary face)
template <class T, class G, class WK>
static void launch_solid_grad(const DevMeshT<G>& dm, const ResParams& prm, const T* W, WK& wk, hipStream_t st) {
    DAS_CHECK(prm.nPass >= 1, DAS_ERR_ARG, "DASolidDisplacementFoam needs maxCorrectBCCalls >= 1, not " + std::to_string(prm.nPass));
    const size_t nBF3 = 3 * (size_t)std::max(1, dm.nF - dm.nIF);
    if (wk.gTr.n != nBF3) wk.gTr.alloc(nBF3);
    hipLaunchKernelGGL((k_solid_grad<T, G>), dim3(nblk(dm.nC, 256)), dim3(256), 0, st, dm, prm, W, wk.gU.p);
    if (prm.nTrac > 0) hipLaunchKernelGGL((k_solid_traction<T, G>), dim3(nblk(prm.nTrac, 256)), dim3(256), 0, st, dm, prm, wk.gU.p, wk.gTr.p);
}

template <class T>
struct ResWork {
    DevBuf<T> nut, gU, gP, gN, gH, rAU, HbyA, q, gT, TU;
    DevBuf<T> gTr;  // DASolidDisplacementFoam: the tractionDisplacement gradient, 3 per boundary face (allocated on first use)
    DevBuf<T> fc, brec;  // face / cell split of the cell pass: 6 scalars per internal face, 13 per boundary face (allocated on first use)
    DevBuf<T> beta;      // regression models: betaFINuTilda per cell as k_reg_forward wrote it (allocated on first use)
    void ensure(int solver, long long N, long long F) {
        if (solver == DAS_SOLVER_SIMPLEFOAM || DAS_IS_COMPRESSIBLE(solver)) {
            if (nut.n != (size_t)N) {
                nut.alloc(N); gU.alloc(9 * N); gP.alloc(3 * N); gN.alloc(3 * N); rAU.alloc(N); HbyA.alloc(3 * N); q.alloc(F);
            }
            if (gH.n != (size_t)(3 * N)) gH.alloc(3 * N);  // compressible he / the optional T field of DASimpleFoam
            if (solver == DAS_SOLVER_TURBOFOAM && TU.n != (size_t)(3 * N)) TU.alloc(3 * N);
        } else if (solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM) {
            if (gU.n != (size_t)(9 * N)) gU.alloc(9 * N);  // gradD
        } else if (gT.n != (size_t)(3 * N)) gT.alloc(3 * N);
    }
    // work array referenced through ResParams (DATurboFoam)
    ResParams bind(int solver, long long N, long long F, ResParams prm) {
        ensure(solver, N, F);
        prm.wTU = TU.p;
        return prm;
    }
};

// one k_reg_forward launch (das_regression.hpp); its LDS follows the model: the parameters and two activation columns per thread
template <class T, class G>
static void launch_reg_forward(const RegView& v, int nC, const CellGeomT<G>* cg, const ResParams& prm, const T* W, const T* gU, const T* gP, const double* featIn,
                               int seed, T* beta, double* featOut, unsigned char* maskOut, hipStream_t st) {
    const size_t lds = reg_forward_lds<T>(v);
    if (lds > 64 * 1024) { DAS_HIP(hipFuncSetAttribute((const void*)k_reg_forward<T, G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); }
    hipLaunchKernelGGL((k_reg_forward<T, G>), dim3(nblk(nC, DAS_REG_FWD_THREADS)), dim3(DAS_REG_FWD_THREADS), lds, st, v, nC, cg, prm, W, gU, gP, featIn, seed, beta,
                       featOut, maskOut);
}

// the gradient launch of DASimpleFoam: face-parallel k_grad_fp where it applies (no T field, double metrics, amd.gradFaceParallel), else k_grad
template <class T, class G>
static void launch_grad_simple(const DevMeshT<G>& dm, const ResParams& prm, const T* W, ResWork<T>& wk, hipStream_t st) {
    if constexpr (std::is_same<G, double>::value) {
        // measured at 2 M cells (profiles/r06e_*, r06f_*; rocprofv3 averages over 540 launches): fp64 states 448 -> 348 us (-22 %); dual numbers
        // 568 -> 613 us (979 with the first LDS layout): the 16-byte scalars double the LDS traffic of the transposition and halve the cells per
        // workgroup - the dual-number passes keep k_grad (amd.gradFaceParallel 2 forces the face-parallel kernel for them as well)
        if (prm.gradFaceParallel && !prm.hasT && (sizeof(T) == 8 || prm.gradFaceParallel >= 2)) {
            constexpr int CPB = sizeof(T) > 8 ? 16 : 32;  // dual numbers: 16 cells per workgroup (LDS: 5 x CPB + 120 x CPB scalars)
            const size_t shBytes = (size_t)(5 * CPB + 15 * CPB * 8) * sizeof(T);
            hipLaunchKernelGGL((k_grad_fp<T, CPB>), dim3(nblk(dm.nC, CPB)), dim3(CPB * 8), shBytes, st, dm, prm, W, wk.nut.p, wk.gU.p, wk.gP.p, wk.gN.p);
            return;
        }
    }
    hipLaunchKernelGGL((k_grad<T, false, G>), dim3(nblk(dm.nC, 256)), dim3(256), 0, st, dm, prm, W, wk.nut.p, wk.gU.p, wk.gP.p, wk.gN.p, wk.gH.p);
}

// one residual evaluation R(W): DAResidual::masterFunction (reference DAResidual.C:100-171)
template <class T, class G = double>
static void eval_residual(const DevMeshT<G>& dm, const CaseParams& cp, const ResParams& prm_in, const T* W, T* R, ResWork<T>& wk,
                          const double* d_phiF, const double* d_Told, hipStream_t st) {
    ResParams prm = wk.bind(cp.solver, dm.nC, dm.nF, prm_in);
    const int B = 256;
    if (cp.solver == DAS_SOLVER_SIMPLEFOAM) {
        launch_grad_simple<T, G>(dm, prm, W, wk, st);
        if (cp.reg) {  // regression models: betaFINuTilda of this pass, in its scalar; one launch per model, the last one wins
            if (wk.beta.n != (size_t)dm.nC) wk.beta.alloc(dm.nC);
            for (int k = 0; k < cp.reg->n; k++)
                launch_reg_forward<T, G>(cp.reg->v[k], dm.nC, dm.cg, prm, W, (const T*)wk.gU.p, (const T*)wk.gP.p, nullptr, cp.regSeed, wk.beta.p, nullptr, nullptr, st);
            prm.betaReg = wk.beta.p;
        }
        bool split = false;
        if constexpr (std::is_same<G, double>::value) {
            if (prm.cellFaceSplit) {
                split = true;
                const long long nBF = dm.nF - dm.nIF;
                if (wk.fc.n != (size_t)DAS_FC_N * dm.nIF) wk.fc.alloc((size_t)DAS_FC_N * dm.nIF);
                if (wk.brec.n != (size_t)DAS_BREC_N * nBF) wk.brec.alloc((size_t)DAS_BREC_N * nBF);
                if (dm.nIF > 0) hipLaunchKernelGGL((k_fcoef<T>), dim3(nblk(dm.nIF, B)), dim3(B), 0, st, dm, prm, W, (const T*)wk.nut.p, (const T*)wk.gU.p, (const T*)wk.gN.p, wk.fc.p);
                if (nBF > 0) hipLaunchKernelGGL((k_bcoef<T>), dim3(nblk(nBF, B)), dim3(B), 0, st, dm, prm, W, (const T*)wk.nut.p, (const T*)wk.gU.p, wk.brec.p);
                if (dm.src3)
                    hipLaunchKernelGGL((k_cell2<T, true>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, (const T*)wk.nut.p, (const T*)wk.gU.p, (const T*)wk.gP.p,
                                       (const T*)wk.gN.p, (const T*)wk.fc.p, (const T*)wk.brec.p, R, wk.rAU.p, wk.HbyA.p);
                else
                    hipLaunchKernelGGL((k_cell2<T>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, (const T*)wk.nut.p, (const T*)wk.gU.p, (const T*)wk.gP.p,
                                       (const T*)wk.gN.p, (const T*)wk.fc.p, (const T*)wk.brec.p, R, wk.rAU.p, wk.HbyA.p);
            }
        }
        if (prm.ddt) {  // DAPimpleFoam (no split path, no disks)
            DAS_CHECK(prm.W0 && (prm.ddtC00 == 0.0 || prm.W00), DAS_ERR_STATE, "DAPimpleFoam: the old-time states have not been set (setOldTimeStates)");
            hipLaunchKernelGGL((k_cell<T, false, G, false, true>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, wk.nut.p, wk.gU.p, wk.gP.p, wk.gN.p,
                               (const T*)wk.gH.p, R, wk.rAU.p, wk.HbyA.p);
        } else if (!split && dm.src3)
            hipLaunchKernelGGL((k_cell<T, false, G, true>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, wk.nut.p, wk.gU.p, wk.gP.p, wk.gN.p,
                               (const T*)wk.gH.p, R, wk.rAU.p, wk.HbyA.p);
        else if (!split)
            hipLaunchKernelGGL((k_cell<T, false, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, wk.nut.p, wk.gU.p, wk.gP.p, wk.gN.p,
                               (const T*)wk.gH.p, R, wk.rAU.p, wk.HbyA.p);
        hipLaunchKernelGGL((k_face<T, false, G>), dim3(nblk(dm.nF, B)), dim3(B), 0, st, dm, prm, W, wk.nut.p, wk.gP.p, wk.rAU.p, wk.HbyA.p, wk.q.p, R);
        hipLaunchKernelGGL((k_pres<T, false, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, wk.q.p, R);
    } else if (DAS_IS_COMPRESSIBLE(cp.solver)) {
        hipLaunchKernelGGL((k_grad<T, true, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, wk.nut.p, wk.gU.p, wk.gP.p, wk.gN.p, wk.gH.p);
        hipLaunchKernelGGL((k_cell<T, true, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, wk.nut.p, wk.gU.p, wk.gP.p, wk.gN.p,
                           (const T*)wk.gH.p, R, wk.rAU.p, wk.HbyA.p);
        hipLaunchKernelGGL((k_face<T, true, G>), dim3(nblk(dm.nF, B)), dim3(B), 0, st, dm, prm, W, wk.nut.p, wk.gP.p, wk.rAU.p, wk.HbyA.p, wk.q.p, R);
        hipLaunchKernelGGL((k_pres<T, true, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, wk.q.p, R);
    } else if (cp.solver == DAS_SOLVER_HEATTRANSFERFOAM) {
        hipLaunchKernelGGL((k_heat_grad<T, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, wk.gT.p);
        hipLaunchKernelGGL((k_heat<T, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, (const T*)wk.gT.p, R);
    } else if (cp.solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM) {
        launch_solid_grad<T, G>(dm, prm, W, wk, st);
        hipLaunchKernelGGL((k_solid<T, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, (const T*)wk.gU.p, (const T*)wk.gTr.p, R);
    } else {
        hipLaunchKernelGGL((k_gradT<T, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, d_phiF, wk.gT.p);
        hipLaunchKernelGGL((k_T<T, G>), dim3(nblk(dm.nC, B)), dim3(B), 0, st, dm, prm, W, d_phiF, d_Told, wk.gT.p, R);
    }
    DAS_HIP(hipGetLastError());
}

// =====================================================================================================
// coloured assembly kernels
// =====================================================================================================
// seeds: W_j + eps s_j for the K colours [c0, c0+K)   (reference DAPartDeriv::perturbStates :42-107 with AD seeds)
template <int K>
__global__ void k_seed(long long n, const double* __restrict__ W, const int* __restrict__ colors, const double* __restrict__ scale, int c0,
                       Dual<K>* Wd) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    Dual<K> w(W[j]);
    int c = colors[j] - c0;
    if (c >= 0 && c < K) w.d[c] = scale[j];
    Wd[j] = w;
}
__global__ void k_lift(long long n, const double* __restrict__ W, Dual<1>* Wd) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) Wd[j] = Dual<1>(W[j]);
}
// W + eps (s o v): tangent = s_j v_j (forward-mode directional derivative dR/dW . (s o v))
__global__ void k_seed_dir(long long n, const double* __restrict__ W, const double* __restrict__ scale, const double* __restrict__ v, Dual<1>* Wd) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    Dual<1> w(W[j]);
    w.d[0] = scale[j] * v[j];
    Wd[j] = w;
}
__global__ void k_tangent_out(long long n, const Dual<1>* __restrict__ R, double* out) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) out[j] = R[j].d[0];
}
__global__ void k_perturb(long long n, const double* __restrict__ W, const int* __restrict__ colors, const double* __restrict__ scale, int c,
                          double delta, double* Wp) {
    long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    Wp[j] = W[j] + (colors[j] == c ? delta * scale[j] : 0.0);
}
// setPartDerivMat (reference DAPartDeriv.C:109-208): after the residual pass of one colour, every column j of that colour
// fills its own transposed row - the residuals listed there depend on j, and j is their unique column of this colour.
// 16 lanes per column; no scatter map, no search.
__global__ __launch_bounds__(256) void k_scatter_dual(long long cnt, const Dual<1>* __restrict__ R, const int* __restrict__ cols,
                                                      const long long* __restrict__ trp, const int* __restrict__ tcol, double* __restrict__ vals) {
    const long long q = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (q >= cnt) return;
    const int j = cols[q];
    for (long long k = trp[j] + (threadIdx.x & 15); k < trp[j + 1]; k += 16) vals[k] = R[tcol[k]].d[0];
}
__global__ __launch_bounds__(256) void k_scatter_fd(long long cnt, const double* __restrict__ R, const double* __restrict__ R0, double rdelta,
                                                    const int* __restrict__ cols, const long long* __restrict__ trp, const int* __restrict__ tcol,
                                                    double* __restrict__ vals) {
    const long long q = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (q >= cnt) return;
    const int j = cols[q];
    for (long long k = trp[j] + (threadIdx.x & 15); k < trp[j + 1]; k += 16) {
        const int i = tcol[k];
        vals[k] = (R[i] - R0[i]) * rdelta;
    }
}

// =====================================================================================================
// linear algebra kernels (the operator product y = A x and the jacLowerBounds filter: das_opmat.hpp)
// =====================================================================================================
__global__ void k_axpby(long long n, double a, const double* __restrict__ x, double b, double* __restrict__ y) {
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) y[k] = a * x[k] + b * y[k];
}
__global__ void k_mul(long long n, const double* __restrict__ s, double* __restrict__ y) {
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) y[k] *= s[k];
}

// ---- Newton primal helpers ------------------------------------------------------------------------------------------------
__global__ void k_extract_diag(long long n, const long long* __restrict__ rp, const int* __restrict__ ci, const double* __restrict__ v, double* __restrict__ d,
                               long long exLo, long long exHi, long long end) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a = 0.0;
    if (i < end && !(i >= exLo && i < exHi))
        for (long long k = rp[i]; k < rp[i + 1]; k++) if (ci[k] == i) { a = v[k]; break; }
    d[i] = a;
}
__global__ void k_add_diag_prod(long long n, double a, const double* __restrict__ d, const double* __restrict__ x, double* __restrict__ y) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] += a * d[i] * x[i];
}
// Wn = W + omega * s o dw, with the SA working variable kept non-negative
__global__ void k_newton_update(long long n, long long n0, long long n1, double omega, const double* __restrict__ W, const double* __restrict__ scale,
                                const double* __restrict__ dw, double* __restrict__ Wn) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double w = W[i] + omega * scale[i] * dw[i];
    if (i >= n0 && i < n1 && w < 1e-14) w = 1e-14;
    Wn[i] = w;
}

// ---- RAS/ILU(k) apply: one workgroup per (overlapping) additive-Schwarz block -------------------------------------
// Restricted additive Schwarz: the block solves on its extended (core + overlap) unknowns and writes back only the
// core part (PETSc's default PC_ASM_RESTRICT, reference DALinearEqn.C:199-216).
//
// MI355X design of the triangular solves: level scheduling has O(10^3) levels of only a few rows each, so the cost is
// the dependent-latency chain per level, not bandwidth.  Therefore
//   * the block's work vector lives in LDS (<= 160 KiB) - dependent reads are LDS reads;
//   * the factor is stored as ONE entry stream per block sorted by (level, row): {value fp64, row u16, col u16}; a level
//     is a contiguous range of the stream, every thread owns the entries e = tid (mod T) and applies
//     x[row] -= val * x[col] with an LDS fp64 atomic (rows of a level are independent, so only same-row partial
//     sums collide);
//   * U rows are pre-divided by their pivot and x is scaled by 1/pivot once before the backward sweep, so each level
//     needs exactly one workgroup barrier;
//   * entry loads do not depend on x: each thread keeps its next PF entries in registers (software prefetch), so the
//     HBM/L2 latency is overlapped with the barriers of the preceding levels.
#ifndef PC_THREADS
#define PC_THREADS 1024
#endif
#ifndef PC_PF
#define PC_PF 8
#endif
struct PCView {
    int nBlocks;
    const long long* boff;     // nBlocks+1: offset of the block's (extended) unknowns
    const int* gidx;           // extended position -> global state index (gather)
    const int* gout;           // extended position -> global state index if owned by the block's core, else -1
    const double* invd;        // 1/pivot per extended position
    // L and U entry streams (values fp64 or fp32: `svalf` is used when factor32 is set)
    int factor32;
    const double* sval[2];
    const float* svalf[2];
    const unsigned* srowcol[2];  // row | col << 16 (block-local)
    const long long* slev[2];    // level pointers into the streams (absolute entry offsets), concatenated per block
    const long long* slevOff[2]; // nBlocks+1 offsets into slev
    double* xglob;             // global scratch when a block does not fit into LDS
};

// x[row] -= v * x[col] for one entry per lane (LDS fp64 atomic: rows of a level are independent, only partial sums of
// the same row collide).  PC_SEGREDUCE=1 (default): DPP segmented pre-reduction over 16-lane rows before the atomics -
// 3.96 -> 2.38 ms per apply (an earlier shuffle-based pre-reduction, which goes through the LDS crossbar, was slower).
#ifndef PC_SEGREDUCE
#define PC_SEGREDUCE 1
#endif
// DPP lane moves inside a row of 16 lanes (row_shr:n = 0x110+n, row_shl:1 = 0x101); lanes without a source keep `old`
template <int CTRL>
__device__ __forceinline__ unsigned dpp_u32(unsigned v, unsigned old) {
    return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
template <bool USE_LDS>
__device__ __forceinline__ void ras_apply_entry(double* xw, double v, unsigned rc, bool valid) {
#if PC_SEGREDUCE
    // The entries of a level are sorted by row, so the lanes of a wave hit one or two rows: 64 same-address LDS atomics
    // serialise in the LDS bank.  Segmented sum over the 16 lanes of a DPP row first (4 row_shr steps, VALU only); only
    // the last lane of every run of equal rows touches LDS: <= 4 + #rows atomics per wave instead of 64.
    const unsigned key = valid ? (rc & 0xffffu) : (0x10000u + (threadIdx.x & 63u));
    double val = valid ? -v * xw[rc >> 16] : 0.0;
    unsigned k;
    double w;
    k = dpp_u32<0x111>(key, 0xffffffffu); w = dpp_f64<0x111>(val); if (k == key) val += w;
    k = dpp_u32<0x112>(key, 0xffffffffu); w = dpp_f64<0x112>(val); if (k == key) val += w;
    k = dpp_u32<0x114>(key, 0xffffffffu); w = dpp_f64<0x114>(val); if (k == key) val += w;
    k = dpp_u32<0x118>(key, 0xffffffffu); w = dpp_f64<0x118>(val); if (k == key) val += w;
    const unsigned knext = dpp_u32<0x101>(key, 0xffffffffu);  // row_shl:1: the key of the next lane (none for lane 15)
    if (valid && knext != key) {
        if (USE_LDS) __hip_atomic_fetch_add(&xw[key], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else atomicAdd(&xw[key], val);
    }
#else
    if (!valid) return;
    const double contrib = -v * xw[rc >> 16];
#ifdef PC_EXP_NOATOMIC
    xw[rc & 0xffffu] = contrib;  // timing experiment only (wrong results)
#else
    if (USE_LDS) __hip_atomic_fetch_add(&xw[rc & 0xffffu], contrib, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else atomicAdd(&xw[rc & 0xffffu], contrib);
#endif
#endif
}

// One triangular sweep over a block's level-sorted entry stream.  Software pipeline over LEVELS: slot d of a
// compile-time ring of PC_PF slots holds this thread's entry of level lv0+d; after consuming it the slot is refilled
// with the entry of level lv0+d+PC_PF.  Everything in the loop body is straight-line code: the host splits levels
// into pieces of <= PC_THREADS entries (one entry per thread per level) and the level list is padded with empty
// levels, so the refill loads are UNCONDITIONAL (clamped address + validity flag).  This matters on CDNA: a load
// inside a conditional forces the compiler's s_waitcnt insertion to assume it may not have been issued, which
// degrades every later wait to vmcnt(0) and serialises the prefetch ring.
// 32-bit-lane loads of the factor values: an fp64 value travels as two dwords (lo, hi).  With global_load_dwordx2 in
// the ring the compiler's s_waitcnt insertion emits vmcnt(1..4) inside the steady-state loop (a drain of the ring on
// every trip); with dword loads only it emits the exact vmcnt(2*PF-2) / vmcnt(3*PF-3) - inspected in the gfx950 ISA.
template <class VT> struct RingVal;
template <> struct RingVal<float> {
    unsigned a;
    __device__ __forceinline__ void load(const float* __restrict__ p, int e) { a = __float_as_uint(p[e]); }
    __device__ __forceinline__ double get() const { return (double)__uint_as_float(a); }
    __device__ __forceinline__ void clear() { a = 0u; }
};
template <> struct RingVal<double> {
    unsigned lo, hi;
    __device__ __forceinline__ void load(const double* __restrict__ p, int e) {
        const unsigned* __restrict__ q = reinterpret_cast<const unsigned*>(p);
        lo = q[2 * (long long)e];
        hi = q[2 * (long long)e + 1];
    }
    __device__ __forceinline__ double get() const { return __hiloint2double((int)hi, (int)lo); }
    __device__ __forceinline__ void clear() { lo = 0u; hi = 0u; }
};

template <bool USE_LDS, class VT>
__device__ __forceinline__ void ras_sweep(const VT* __restrict__ sval, const unsigned* __restrict__ src, const long long* __restrict__ lev,
                                          long long l0, long long l1, double* xw, int* lvl) {
    const long long ebeg = lev[l0];
    const int nptr = (int)(l1 - l0);
    const int NL = nptr - 1;
    const int eend = (int)(lev[l1 - 1] - ebeg);
    if (eend <= 0) return;  // uniform
    const int NLpad = ((NL + PC_PF - 1) / PC_PF) * PC_PF;
    // level pointers -> LDS (relative to the block's first entry), padded with empty levels
    for (int k = threadIdx.x; k < NLpad + PC_PF + 1; k += PC_THREADS) lvl[k] = k < nptr ? (int)(lev[l0 + k] - ebeg) : eend;
    __syncthreads();
    const VT* __restrict__ bv = sval + ebeg;
    const unsigned* __restrict__ br = src + ebeg;
    const int tid = (int)threadIdx.x;
    RingVal<VT> sv[PC_PF];
    unsigned sr[PC_PF];
    bool sok[PC_PF];  // validity lives in its own (load-independent) flag: no ALU touches a loaded register before use
#pragma unroll
    for (int d = 0; d < PC_PF; d++) { sv[d].clear(); sr[d] = 0u; sok[d] = false; }
    // The ring is primed by a first trip that only refills (all slots invalid) instead of a separate prologue: the
    // compiler's s_waitcnt insertion merges the pending-load state of every loop entry, and a prologue whose loads are
    // scheduled in a different order than the steady state degrades the header waits to (almost) vmcnt(0).
    for (int lv0 = -PC_PF; lv0 < NLpad; lv0 += PC_PF) {
#pragma unroll
        for (int d = 0; d < PC_PF; d++) {
            const int lq = lv0 + d + PC_PF;
            // consume, then refill the same slot: the refill loads target the registers the next trip reads, so no
            // register copies (which would need s_waitcnt vmcnt(0)) appear on the loop back-edge
            ras_apply_entry<USE_LDS>(xw, sv[d].get(), sr[d], sok[d]);
            const int ee = lvl[lq] + tid;
            sok[d] = ee < lvl[lq + 1];
            const int ec = ee < eend ? ee : eend - 1;
            sv[d].load(bv, ec);
            sr[d] = br[ec];
#ifndef PC_EXP_NOBARRIER
            __syncthreads();
#endif
        }
    }
}

template <bool USE_LDS>
__global__ __launch_bounds__(PC_THREADS) void k_ras_apply(PCView P, const double* __restrict__ b, double* __restrict__ out, int maxLev) {
    extern __shared__ double xs[];
    const int blk = blockIdx.x;
    const long long o0 = P.boff[blk];
    const int nloc = (int)(P.boff[blk + 1] - o0);
    int* lvl = (int*)xs;                                   // level pointers (+ padding levels), padded to 8 bytes
    double* xlds = xs + ((maxLev + 2 * PC_PF + 4) >> 1);
    double* xw = USE_LDS ? xlds : P.xglob + o0;
    for (int i = threadIdx.x; i < nloc; i += PC_THREADS) xw[i] = b[P.gidx[o0 + i]];
    __syncthreads();
    if (P.factor32) ras_sweep<USE_LDS, float>(P.svalf[0], P.srowcol[0], P.slev[0], P.slevOff[0][blk], P.slevOff[0][blk + 1], xw, lvl);
    else ras_sweep<USE_LDS, double>(P.sval[0], P.srowcol[0], P.slev[0], P.slevOff[0][blk], P.slevOff[0][blk + 1], xw, lvl);
    for (int i = threadIdx.x; i < nloc; i += PC_THREADS) xw[i] *= P.invd[o0 + i];
    __syncthreads();
    if (P.factor32) ras_sweep<USE_LDS, float>(P.svalf[1], P.srowcol[1], P.slev[1], P.slevOff[1][blk], P.slevOff[1][blk + 1], xw, lvl);
    else ras_sweep<USE_LDS, double>(P.sval[1], P.srowcol[1], P.slev[1], P.slevOff[1][blk], P.slevOff[1][blk + 1], xw, lvl);
    for (int i = threadIdx.x; i < nloc; i += PC_THREADS) {
        int g = P.gout[o0 + i];
        if (g >= 0) out[g] = xw[i];
    }
}

// =====================================================================================================
// host-side objects
// =====================================================================================================
struct Mat {
    long long n = 0, nnz = 0;
    DevBuf<long long> rowptr;
    DevBuf<int> col;
    DevBuf<double> val;
    VecPack vp;  // packed vector rows of the Krylov operator (das_opmat.hpp); empty for every other matrix
};

struct KernelTimer {
    struct Rec { double ms = 0; long long cnt = 0; std::vector<std::pair<hipEvent_t, hipEvent_t>> pending; };
    std::map<std::string, Rec> recs;
    bool on = false;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        DAS_HIP(hipEventCreate(&e));
        return e;
    }
    void begin(const char* name, hipStream_t st, hipEvent_t& a) {
        if (!on) return;
        a = get();
        DAS_HIP(hipEventRecord(a, st));
    }
    void end(const char* name, hipStream_t st, hipEvent_t a) {
        if (!on) return;
        hipEvent_t b = get();
        DAS_HIP(hipEventRecord(b, st));
        recs[name].pending.push_back({a, b});
    }
    void resolve() {
        for (auto& kv : recs) {
            for (auto& pr : kv.second.pending) {
                DAS_HIP(hipEventSynchronize(pr.second));
                float ms = 0;
                DAS_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
                kv.second.ms += ms;
                kv.second.cnt++;
                pool.push_back(pr.first);
                pool.push_back(pr.second);
            }
            kv.second.pending.clear();
        }
    }
    void reset() { resolve(); for (auto& kv : recs) { kv.second.ms = 0; kv.second.cnt = 0; } }
};

struct ConDev {  // device copy of a JacCon (assembly maps + transposed structure)
    bool ready = false;
    bool onDevice = false;  // transposed structure generated on the device (das_graph.hpp): the host JacCon holds none
    DevBuf<long long> t_rowptr;
    DevBuf<int> cl_cols;
    DevBuf<int> t_col;
};

struct BlockILU {
    long long n = 0, next = 0;
    int nBlocks = 0;
    long long fnnz = 0;
    int maxLocal = 0;  // largest number of unknowns in one block
    DevBuf<long long> boff, slev[2], slevOff[2];
    DevBuf<int> gidx, gout;
    DevBuf<unsigned> srowcol[2];
    DevBuf<double> sval[2], invd, xw;
    DevBuf<float> svalf[2];
    bool factor32 = false;
    PCView view;
    int maxLevels = 0;
    bool useLDS = false;
    double setup_seconds = 0;
    std::vector<int> h_core_perm;           // host copies for introspection (tests)
    std::vector<long long> h_core_off;
};

}  // namespace das

using namespace das;

struct das_mat {
    Mat m;
};

struct das_ksp {
    das_mat* pcmat = nullptr;
    BlockILU pc;      // amd.pcType "ras": restricted additive Schwarz + scalar ILU(k) blocks in LDS
    NodeILU bilu;     // amd.pcType "bilu" (default): global node-block ILU(0), sync-free sweeps (das_bilu.hpp)
    bool useBilu = false;
    bool pcTranspose = false;   // factorise jacPCMat^T (forward system of the Newton primal)
    double pcDiagScale = 1.0;   // 1 + 1/tau on the diagonal (pseudo-transient shift)
    long long shiftExLo = 0, shiftExHi = 0, shiftEnd = (long long)1 << 62;  // ... on the rows below shiftEnd outside [shiftExLo, shiftExHi)
    struct CoarsePC {
        bool active = false, deflated = false;
        bool global = false;        // multi-GPU: ONE coarse space over all ranks (das_ksp_set_global_coarse), else per rank
        int nagg = 0;               // aggregates of this rank's owned cells
        int naggG = 0, aggOff = 0;  // size of the coarse operator and the first own aggregate in it (single rank: nagg, 0)
        long long off = 0, N = 0;
        DevBuf<int> agg;            // per cell: aggregate in the coarse operator for OWNED cells, -1 otherwise (prolongation, columns of E)
        DevBuf<int> aggRow;         // per cell: aggregate for owned AND ghost cells (rows of E); single rank: same as agg
        DevBuf<int> cells, cellsAll;
        DevBuf<long long> aptr, aptrAll;  // own aggregates (restriction) / all aggregates with local row cells (assembly)
        DevBuf<double> Einv, t, u, c, rr;
        std::vector<int> h_agg;     // local aggregate of every cell (-1: not owned), as handed out by das_ksp_get_coarse
        // deflated mode, single rank, assembled operator: A Z as a sparse n x nagg matrix (rows hold the few aggregates their p-columns
        // touch), so that the A-DEF1 term A (Z u) costs one pass over ~1.2 entries per row instead of a full operator product
        DevBuf<long long> azPtr;
        DevBuf<int> azAgg;
        DevBuf<double> azVal;
        long long azOpId = -1;  // id of the operator A Z was built from (das_solver::opId; rebuilt when the operator is re-assembled)
        long long azEpoch = -1, azNnz = 0;
        bool azReady = false, azFailed = false;
    } coarse;
    int restart = 0;
    VmBuf<double> V;  // Krylov basis: up to 129 GB (reference default restart at 2 M cells) - mapped chunk by chunk through the VM API
    long long Vn = 0; // vector length the basis was reserved for
    // compressed basis (amd.krylovBasisPrecision, gmres_ws): the basis vectors are STORED in fp32 (half the bytes of the two Gram-Schmidt
    // passes, which are most of an iteration at depth > 150), all inner products / updates / the Hessenberg matrix stay fp64
    bool vf32 = false;
    // split storage: slot j of V holds [hi_j (n floats) | lo_j (n floats)] - the 8 n bytes an fp64 vector takes, so the range, its on-demand
    // mapping and its single mapper thread are exactly those of the fp64 basis (round 5: a first version kept the lo halves in a SECOND
    // virtual range with its own mapper; two of five 2 M-cell runs lost the Arnoldi relation after ~800 vectors - recurrence 2.5e-9, true
    // residual 5.4e-5, profiles/r06f_*, r06j_* - which the single-range layout has not shown); vf32 is set as well
    bool split = false;
    DevBuf<double> ustage;  // fp64 copy of the basis vector the preconditioner is applied to (fp32 basis only)
    DevBuf<double> w, z, r, xdev, bdev, partial, hdev, rich_r, rich_d;
    // amd.pcSubdomains K > 1 (single rank): restricted additive Schwarz INSIDE the GPU - K node-block ILUs on RCB blocks of the cells (+
    // asmOverlap rings), every block with its own elimination order, merged into ONE level structure (bilu_setup_multi): `bilu` holds it
    int nSub = 1;
    std::vector<int> subOrder;      // elimination order of every block
    std::vector<double> subEst;     // stability estimate of every block's own factorisation
    int pcOrder = -1;  // elimination order of the node-block ILU (bilu_build_structure); -1: adjEqnOption.jacMatReOrdering
    int pcOrderUsed = -1;  // ... the order the stability check settled on
    double pcStability = -1.0;  // stability estimate of the factorisation (-1: not computed)
    bool rasOverlap = false;  // restricted additive Schwarz across ranks: the factorisation covers owned + overlap unknowns (setup_node_ilu)
    DevBuf<double> pcin;      // ... its input: a copy of the vector with the overlap entries gathered from their owners
    std::unique_ptr<struct GmresRun> run;
    std::unique_ptr<struct BlockWork> block;
    int polyD = 0;  // amd.polyDegree as the current solve runs it (gmres_ws)
    std::unique_ptr<struct PolyWork> poly;  // amd.polyDegree > 0: the roots of the GMRES polynomial and its three work vectors (first use)
    std::unique_ptr<struct IdrWork> idr;  // amd.krylovMethod "idrs": the 3 s + O(1) work vectors, allocated once per KSP (idr_ws)
    std::vector<double> block_res0, block_res;
    int iters = 0, nrefine = 0, reason = 0, nBreakdown = 0;
    double res0 = 0, res = 0, seconds = 0;
    std::vector<double> hist;
    std::vector<int> cycleLens;  // columns of every closed Arnoldi cycle of the last solve (das_ksp_get_cycle_lengths)
};

struct das_solver {
    Mesh mesh;
    CaseParams cp;
    Options opt;
    int device = -1;
    bool inited = false;
    long long n = 0;
    Stencil st_full, st_pc;
    JacCon con_full, con_pc;
    std::vector<int> colors;
    int nColors = 0;
    bool colored = false;
    // device mesh
    DevBuf<FaceGeom> d_fg;
    DevBuf<CellGeom> d_cg;
    DevBuf<int> d_cf_ptr, d_cf_face, d_cf_other, d_owner, d_neigh, d_bpatch, d_cyc;
    DevBuf<PatchBC> d_bc;
    DevBuf<double> d_mixed;  // Mesh::mixed (the per-face records of the mixed T patches), when there are any
    DevBuf<int> d_tracCells;  // Mesh::trac_cells (DASolidDisplacementFoam), when there are any
    DevBuf<double> d_phiF, d_Told;
    DevBuf<double> d_W0, d_W00;  // DAPimpleFoam: the old-time state vectors (das_set_old_time_states)
    std::vector<double> h_W0, h_W00;
    // rAU of the last old-time product and what it was computed at: the two levels of one adjoint step share one residual pass
    DevBuf<double> d_rAUold;
    std::vector<double> rAUold_states;
    long long rAUold_epoch = -1, rAUold_geom = -1;
    DevMesh dm;
    DevBuf<double> d_W, d_R, d_R0, d_Wp, d_scale, d_tmp1, d_tmp2;
    DevBuf<int> d_colors;
    std::vector<double> h_W, h_scale;
    ResWork<double> wk;
    ResWork<Dual<1>> wk1;
    DevBuf<Dual<1>> d_Wd, d_Rd;
    ConDev cd[2];
    std::unique_ptr<das_mat> op;  // matrix-free operator (dual-number assembled dRdW^T)
    std::vector<double> op_states;  // the states (and geometry version) the operator was assembled at
    long long op_geom = -1;
    struct FaceFn {  // a face-integral objective (see body_facefn)
        int kind = DAS_FN_FORCE;
        bool ratio = false;  // F = S[1] / S[0] over the two face groups (totalTemperatureRatio), else F = S[0] + S[1]
        double gammaFn = 1.4, RFn = 287.0;
        std::vector<int> faces;
        std::vector<unsigned char> group;
        std::vector<double> w0, dir;  // base weights (nf), directions (3 nf, force/moment only)
        DevBuf<int> d_faces;
        DevBuf<unsigned char> d_group;
        DevBuf<double> d_w0, d_weff, d_dir, d_fv;  // d_fv: per-face summands of the last value / tangent pass
        bool uploaded = false;
        // definition (kept so that the geometry-dependent weights / directions can be rebuilt after updateOFMesh)
        bool isMoment = false;
        double vecA[3] = {0, 0, 0}, vecB[3] = {0, 0, 0}, scale = 1.0;
        long long geomVersion = -1;
        // patchMean / variance (surface): calcRefVar F <- (F - ref)^2; variance weights |Sf| (useGeoWeight) or 1, over their
        // sum or the number of reference points; no reference data: all weights 0
        bool refVar = false, geoWeight = false, hasData = true;
        double ref = 0.0;
        int ncomp = 1;
        // wallHeatFlux: byUnitArea (area average) or the plain sum; location: axis / center, the KS modes (F = log sum exp(coeffKS a_f) /
        // coeffKS, das_facefn.hpp; d_ks = {m, S} of the last value, d_kpart = the block partials) or maxRadius (one face, chosen at definition)
        bool byUnitArea = true, ks = false;
        double coeffKS = 1.0, loc[6] = {1, 0, 0, 0, 0, 0};
        DevBuf<double> d_ks, d_kpart;
        double pRef = 0.0;  // the reference pressure of the forces (the internal function of a ForceCoupling; 0 for the objectives)
        FaceFnView view(const double* w) const {
            return FaceFnView{d_faces.p, d_group.p, w, dir.empty() ? nullptr : d_dir.p, (int)faces.size(), kind, gammaFn, RFn,
                              {loc[0], loc[1], loc[2], loc[3], loc[4], loc[5]}, pRef};
        }
    };
    std::map<std::string, FaceFn> functions;
    // a forceCouplingOutput (das_forcecoupling.hpp): nodal forces on the points of the patches.  The topology (which points, which
    // faces feed them) depends on the connectivity only: das_update_of_mesh leaves it alone.  `fn` is the force functional
    // seeds . output = sum_f d_f . F_f of the derivative passes: kind force, unit weights, the directions d_f written on the device
    // by k_fc_seed_dir (never rebuilt from the geometry: it is no moment and has no fixed direction).
    struct ForceCoupling {
        std::vector<int> patches;  // in output order (the caller sorts them by name)
        int nOut = 0;              // output points (a point shared by two patches counts twice); the output has 3 nOut entries
        std::vector<int> ptPtr, ptSlot;      // output point -> face slots, ascending
        std::vector<int> fcPtr, fcPt;        // face slot -> output points (fcPtr[k + 1] - fcPtr[k] = the points of the face)
        DevBuf<int> d_ptPtr, d_ptSlot, d_fcPtr, d_fcPt;
        DevBuf<double> d_ff, d_out, d_seeds;
        FaceFn fn;
        bool uploaded = false;
    };
    std::map<std::string, ForceCoupling> forceCouplings;
    // a thermalCouplingOutput (das_thermalcoupling.hpp): [T of the owner cells, kappa / d] over the faces of the patches.  `fn` lists the
    // faces and is the functional seeds . output of the derivative passes: kind thermalCoupling, unit weights, d_f = the two seeds of the
    // face, written on the device by k_tc_seed_dir.
    struct ThermalCoupling {
        std::vector<int> patches;  // in output order (the caller sorts them by name)
        DevBuf<double> d_out, d_seeds;
        FaceFn fn;
        bool uploaded = false;
        std::vector<double> in;  // a thermalCoupling input: what was set last (empty before the first time); d_out then holds the myK used
    };
    // the outputs, and the thermalCoupling inputs (reference DAInputThermalCoupling.C): the same faces and kernels, on mixed T patches
    std::map<std::string, ThermalCoupling> thermalCouplings, thermalInputs;
    struct CellFn {  // a cell-set objective (see das_cellfn.hpp)
        bool variance = false, square = false, multiplyVol = true, divByTotalVol = false, refVar = false, geoWeight = false, hasData = true;
        bool field = false;  // src = betaFINuTilda instead of the states
        double scale = 1.0, ref = 0.0;
        double coef = 0.0, totalVol = 1.0;  // from the metrics of geomVersion
        long long geomVersion = -1;
        std::vector<int> cell;
        std::vector<long long> idx;
        std::vector<double> data;
        DevBuf<int> d_cell;
        DevBuf<long long> d_idx;
        DevBuf<double> d_data, d_part, d_unit;  // d_unit: betaFINuTilda = 1 while no field has been set
        // DASolidDisplacementFoam: constSrc = variableVolSum of solid:rho (src = the uniform density, a `field`-like source no state
        // reaches); vmKS = vonMisesStressKS over the cell set (k_vm_terms + the KS kernels of das_facefn.hpp)
        bool constSrc = false, vmKS = false;
        double coeffKS = 1.0;
        DevBuf<double> d_a, d_ks, d_kpart, d_wt, d_wc;  // vm per term, {m, S}, partials, softmax weights per term and per cell
        bool uploaded = false;
        CellFnView view() const {
            return CellFnView{(long long)cell.size(), d_cell.p, d_idx.p, data.empty() ? nullptr : d_data.p, (int)square, (int)multiplyVol};
        }
    };
    std::map<std::string, CellFn> cellFunctions;
    struct MeshFn {  // a function over the whole mesh (das_meshquality.hpp): meshQualityKS, or residualNorm
        std::string name;
        bool residualNorm = false, refVar = false;
        double ref = 0.0;
        int metric = DAS_MQ_ORTHO;  // meshQualityKS
        double coeffKS = 1.0;
        double w[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // residualNorm: the weight of every residual block, in the order of the row layout
        bool l1 = false;
        // d_a: a_f per face / the term per row; d_w: the softmax weights per face; d_ks = {m, S} of the last value, d_kpart = the block
        // partials; d_X: the points of xGeom (faceSkewness reads them)
        DevBuf<double> d_a, d_w, d_ks, d_kpart, d_X;
        long long xGeom = -1;
    };
    std::map<std::string, MeshFn> meshFunctions;
    // heat sources of DAHeatTransferFoam (the fvSource option; das_heatsource.hpp).  The map keeps them in name order, the order of the
    // reference's toc() walk, so the accumulation does not depend on the order of definition.
    struct HeatSource {
        int kind = DAS_HS_CYLINDERSMOOTH;
        // cylinderSmooth: heatSourcePars = center(3), axis(3), radius, length, power; cylinderToCell: p1(3), p2(3), radius, |p2 - p1|, power
        double pars[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        double eps = 0.0;
        int snapCell = -1;         // snapCenter2Cell: the cell found at definition (the centre follows its C), -1 otherwise
        std::vector<int> members;  // cylinderToCell: the cell set, chosen at definition and kept
        DevBuf<unsigned char> d_member;
        double volumeTotal = 0.0;  // Vt at the current metrics and parameters
    };
    std::map<std::string, HeatSource> heatSources;
    DevBuf<double> d_src, d_hsVt;       // fvSource per cell (allocated with the first source); Vt per source + the total of the field
    DevBuf<Dual<1>> d_hsPart, d_hsVtD;  // partial sums of either scalar type; dual sums of the parameter passes
    double hsSourceTotal = 0.0;         // sum_c fvSource_c V_c
    // actuator disks of DASimpleFoam (the fvSource option, type actuatorDisk; das_actuatordisk.hpp), in name order like the heat sources
    struct ActuatorDisk {
        int smooth = 1, adjustThrust = 0;
        // the 13 actuatorDiskPars: center(3), direction(3), innerRadius, outerRadius, scale, POD, expM, expN, targetThrust
        // (cylinderAnnulusToCell: center = (p1 + p2) / 2, direction = p2 - p1; expM, expN and targetThrust are not read)
        double pars[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        double eps = 0.0, rotSign = 1.0;
        std::vector<int> members;  // cylinderAnnulusToCell: the cell set, chosen at definition and kept
        DevBuf<unsigned char> d_member;
        double scale = 0.0, thrustSum = 0.0, torqueSum = 0.0, unitThrust = 0.0;  // at the current metrics and parameters
    };
    std::map<std::string, ActuatorDisk> actuatorDisks;
    DevBuf<double> d_src3, d_adSums;  // fvSource (3 per cell, allocated with the first disk); per disk: unit sums(2), scale, sums(2)
    DevBuf<Dual<1>> d_adPart, d_adD;  // partial sums of either scalar type; the sums and the scale of a dual pass
    DevBuf<int> d_adBad;              // set where a cell centre sits on the axis of a disk
    // regression models of DASimpleFoam (the regressionModel option; das_regression.hpp) in the order of their definition, the order of
    // the option dictionary: the last one to write betaFINuTilda wins.  regSet is what CaseParams::reg points at while one is defined.
    struct RegModel {
        std::string name, type;
        std::vector<std::string> inputs;
        RegView v;
        std::vector<double> par;
        DevBuf<double> d_par;
    };
    std::vector<std::unique_ptr<RegModel>> regModels;
    RegSet regSet;
    DevBuf<double> d_regFeat, d_regBeta, d_regPart, d_regOut;  // features and output of one model (read-back), partials and result of the backward kernel
    DevBuf<unsigned char> d_regMask;
    bool reg_needs_p() const {  // pGradStream and PSoSS read grad(p): nuTildaRes then depends on p at levels 0 and 1
        for (const auto& m : regModels)
            for (int k = 0; k < m->v.nIn; k++)
                if (m->v.feat[k] == DAS_REG_PGRADSTREAM || m->v.feat[k] == DAS_REG_PSOSS) return true;
        return false;
    }
    int colorRounds = 0;       // rounds of the speculative device colouring (0: another algorithm ran)
    DevBuf<double> d_betaFI, d_dBetaFI;  // `field` input betaFINuTilda and its tangent (das_set_field / das_calc_dfield_product)
    long long geomVersion = 0;  // bumped by das_update_of_mesh
    // mesh-sensitivity product (das_volcoord.hpp): point influence sets + colours (topology only: built once), device copies
    struct VolCoord {
        PointInfluence inf;
        bool built = false, uploaded = false;
        double relStep = 0.0;
        long long hGeom = -1;  // geometry version the steps h were computed for
        DevBuf<long long> d_ptr;
        DevBuf<int> d_cells, d_cpoints, d_face_ptr, d_face_pts, d_bad, d_fnPtr, d_fnIdx;
        DevBuf<double> d_h, d_X0, d_X, d_Rp, d_Rm, d_seeds, d_tc, d_out, d_fvp, d_fvm;
        DevBuf<FaceGeom> d_fg0;
        DevBuf<CellGeom> d_cg0;
        double buildSeconds = 0.0, seconds = 0.0;
    } vc;
    // everything else the Jacobian depends on besides the states and the geometry: patch values, old-time fields, options
    // (normalizeStates, residual / discretisation switches).  Every setter bumps the epoch; a cached operator is only
    // reused by calcJacTVecProduct when its epoch is current
    long long opEpoch = 0, op_epoch = -1;
    long long nGlobalCells = 0; // sharded runs (das_set_n_global_cells); 0 = single domain
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::vector<unsigned char> owned;  // per state; empty = single-domain
    DevBuf<unsigned char> d_owned;
    // additive-Schwarz overlap (das_set_pc_overlap; adjEqnOption.asmOverlap, reference DALinearEqn.C:212-216): the unknowns of this rank's
    // sub-domain solve = owned + `asmOverlap` rings of ghost cells; empty = the owned unknowns (block-Jacobi across ranks)
    std::vector<unsigned char> pcMask;
    DevBuf<unsigned char> d_pcMask;
    long long opId = 0;  // bumped whenever the assembled operator is created or destroyed (caches keyed on it)
    struct FwdOp {  // Newton primal: the Krylov operator is (dR/dW S + D / tau) applied matrix-free by one dual-number residual pass
        bool on = false;
        double invTau = 0.0;
        DevBuf<double> diag;  // D = diag(dR/dW S), taken from jacPCMat
    } fwd;
    HaloPlan halo;  // native halo reduction / all-reduce (das_comm.hpp); the two callbacks below are the legacy host transport
    das_halo_cb halo_cb = nullptr;
    das_allreduce_cb allreduce_cb = nullptr;
    void* comm_user = nullptr;
    KernelTimer timer;
    NodeILU pcStruct;  // das_pc_structure_build (host-only introspection)
    double t0_wall = 0;
    std::clock_t t0_cpu = 0;
};

static thread_local std::string g_err;
static int fail(const std::exception& e) {
    g_err = e.what();
    const Error* de = dynamic_cast<const Error*>(&e);
    return de ? de->code : DAS_ERR_INTERNAL;
}
#define DAS_TRY try {
#define DAS_CATCH \
    }             \
    catch (const std::exception& e) { return fail(e); }

static void need_init(das_solver* s) {
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    DAS_CHECK(s->inited, DAS_ERR_STATE, "das_init_solver has not been called (or failed): no GPU path available");
}
// the fvSource field from the metrics on the device and the parameters as they stand (nothing to do without a source or a device);
// check: wait for the totals, keep them and refuse a total volume that is zero or not finite
static void refresh_heat_sources(das_solver* s, bool check);
// the same for the actuator disks of DASimpleFoam (check: also refuse a cell centre on the axis of a disk)
static void refresh_actuator_disks(das_solver* s, bool check);
// the views of the regression models (das_solver::regSet) from the models as they stand, their parameters on the device once there is one
static void reg_sync(das_solver* s);

// sum of a small device buffer over the ranks: the native all-reduce in stream order, else the legacy host callback (single rank: nothing)
static void rank_allreduce(das_solver* s, double* p, long long cnt, hipStream_t st) {
    if (!(s->halo.active && s->halo.allreduce(p, (int)cnt, st)) && s->allreduce_cb) s->allreduce_cb(p, (int)cnt, s->comm_user);
}
// a flag the ranks must agree on: true everywhere as soon as it is true on one rank (one rank alone: the flag itself)
static bool rank_any(das_solver* s, bool flag) {
    if (!(s->halo.active || s->allreduce_cb)) return flag;
    DevBuf<double> f(1);
    const double fv = flag ? 1.0 : 0.0;
    DAS_HIP(hipMemcpyAsync(f.p, &fv, sizeof(double), hipMemcpyHostToDevice, s->stream));
    rank_allreduce(s, f.p, 1, s->stream);
    DAS_HIP(hipStreamSynchronize(s->stream));
    return f.to_host()[0] > 0.5;
}
// y = a x + b y on the solver's stream (len: number of entries, s->n if not given)
static void axpby(das_solver* s, double a, const double* x, double b, double* y, long long len = -1) {
    const long long n = len < 0 ? s->n : len;
    hipLaunchKernelGGL(k_axpby, dim3(nblk(n, 256)), dim3(256), 0, s->stream, n, a, x, b, y);
}

// state scaling s_j (reference DAPartDeriv.C:210-315, DASolver.C:2356-2455)
static void compute_scales(das_solver* s) {
    s->h_scale.assign(s->n, 1.0);
    for (const StateDef& sd : s->st_full.states) {
        const double v = s->opt.getd_or("normalizeStates." + sd.name, 1.0);
        for (long long k = 0; k < sd.size; k++)
            s->h_scale[sd.offset + k] = sd.kind == KIND_FACE ? v * s->mesh.fg[k].magSf : v;
    }
    if (s->inited) s->d_scale.upload(s->h_scale);
}

// ---- graph set-up on the device (das_graph.hpp): transposed structures and colouring input from the host's row-major pattern
static bool graph_on_device(das_solver* s) {
    if (!s->inited) return false;
    return s->opt.geti_or("amd.graphOnDevice", 1) != 0;
}
static void upload_pattern(const JacCon& j, DevPattern& P) {
    P.n = j.n; P.nnz = j.nnz;
    P.rowptr.upload(j.rowptr);
    P.col.upload(j.col.data(), j.col.size());
}
// transposed structure of pattern isPC into s->cd[isPC]; `keepRowMajor`: hand the uploaded row-major pattern back (colouring)
static void device_build_con(das_solver* s, int isPC, DevPattern* keepRowMajor = nullptr) {
    ConDev& c = s->cd[isPC ? 1 : 0];
    const JacCon& j = isPC ? s->con_pc : s->con_full;
    DevPattern local;
    DevPattern& P = keepRowMajor ? *keepRowMajor : local;
    upload_pattern(j, P);
    device_transpose(P, c.t_rowptr, c.t_col, s->stream);
    c.onDevice = true;
}

// longest chain c_1 < c_2 < ... of cells in which consecutive cells are at most two face-neighbour rings apart: a lower bound of the
// dependent chain of the data-flow first-fit colouring in column order (columns conflict over even longer distances)
static long long cell_chain_depth(const Mesh& m) {
    std::vector<int> depth(m.nC, 0);
    long long best = 0;
    for (int c = 0; c < m.nC; c++) {
        int d = 0;
        for (int q = m.cf_ptr[c]; q < m.cf_ptr[c + 1]; q++) {
            const int n1 = m.cf_other[q];
            if (n1 < 0) continue;
            if (n1 < c) d = std::max(d, depth[n1]);
            for (int r = m.cf_ptr[n1]; r < m.cf_ptr[n1 + 1]; r++) {
                const int n2 = m.cf_other[r];
                if (n2 >= 0 && n2 < c) d = std::max(d, depth[n2]);
            }
        }
        depth[c] = d + 1;
        best = std::max<long long>(best, d + 1);
    }
    return best;
}

// preset != nullptr: colours read from a dRdWColoring file (reference DAJacCon::readJacConColoring :1980-2019) - they
// are validated against the connectivity exactly like the reference does (DAColoring::validateColoring)
static void ensure_coloring(das_solver* s, const int* preset = nullptr) {
    if (s->colored && !preset) return;
    double t = wall_seconds();
    s->st_full = make_stencil(s->cp.solver, s->mesh.nC, s->mesh.nF, s->opt, false, s->cp.hasT != 0, s->reg_needs_p());
    s->st_pc = make_stencil(s->cp.solver, s->mesh.nC, s->mesh.nF, s->opt, true, s->cp.hasT != 0, s->reg_needs_p());
    double t1 = wall_seconds();
    s->con_full.build(s->mesh, s->st_full);
    s->con_pc.build(s->mesh, s->st_pc);
    double t2 = wall_seconds();
    // without a device the transposed structures (no colours needed) are built by a second host thread beside the colouring; with
    // a device they are generated there (das_graph.hpp).  (Measured and dropped: building the preconditioner's pattern in that
    // thread beside the device colouring - the prune and the upload of the operator pattern slowed down by as much as was
    // gained, 8.98 -> 9.80 s: the host phases are memory-bound, profiles/r03y_setup_phases_2M.log.)
    const bool devGraph = graph_on_device(s);
    std::exception_ptr tErr;
    std::thread transposer([&]() {
        if (devGraph) return;
        try { s->con_full.build_transpose(); s->con_pc.build_transpose(); } catch (...) { tErr = std::current_exception(); }
    });
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{transposer};
    for (int k = 0; k < 2; k++) { s->cd[k].ready = false; s->cd[k].onDevice = false; }
    DevPattern fullRowMajor;
    bool fullTransposed = false;
    if (preset) {
        s->colors.assign(preset, preset + s->n);
        int mx = -1;
        for (long long j = 0; j < s->n; j++) {
            DAS_CHECK(s->colors[j] >= 0 && s->colors[j] < 65535, DAS_ERR_ARG, "colour out of range in the supplied colouring");
            mx = std::max(mx, s->colors[j]);
        }
        s->nColors = mx + 1;
    } else {
        {
            std::vector<double> ctr(3 * (size_t)s->mesh.nC);
            for (int c = 0; c < s->mesh.nC; c++) for (int d = 0; d < 3; d++) ctr[3 * (size_t)c + d] = s->mesh.cg[c].C[d];
            // on a GPU box the serial first-fit runs as a data-flow kernel (das_color.hpp); without a device (CPU tests) or with
            // amd.coloringOnDevice = 0 the host variants of das_jaccon.cpp run
            ColorDeviceFn fn = nullptr;
            if (s->inited && s->opt.geti("amd.coloringOnDevice"))
                fn = [s](long long nn, const std::vector<long long>& keep, const std::vector<long long>& cptr, const uvector<int>& crow,
                         const uvector<int>& cpos, const std::vector<long long>& rowptr, const uvector<int>& col, std::vector<int>& colors) {
                    // amd.coloringAlgorithm "firstfit" (default): the serial first-fit as a data-flow kernel over net bitmaps (the
                    // host's serial colours, bit for bit); "speculative": rounds of speculate / detect / retry over the same bitmaps
                    // (order-independent, ~20 % more colours; kept for patterns whose index order gives no wavefront parallelism)
                    const bool spec = s->opt.gets_or("amd.coloringAlgorithm", "firstfit") == "speculative";
                    const bool ok = spec ? color_speculative_device(nn, keep, cptr, crow, rowptr, col, colors, s->stream, &s->colorRounds)
                                         : color_firstfit_device(nn, keep, cptr, crow, cpos, rowptr, col, colors, s->stream);
                    if (!ok) fprintf(stderr, "[dafoam_amd] device colouring gave up (too many colours or a timeout): host first-fit instead\n");
                    return ok;
                };
            // device graph path: the kept rows come from the host's dominance pruning; the transposed full pattern, the
            // column -> net incidence (with positions) and the groups are derived on the device, then the same first-fit kernel
            ColorGraphFn gfn = nullptr;
            {
                const bool spec = s->opt.gets_or("amd.coloringAlgorithm", "firstfit") == "speculative";
                if (devGraph && s->opt.geti("amd.coloringOnDevice") && !spec)
                    gfn = [s, &fullRowMajor, &fullTransposed](long long nn, const std::vector<long long>& keep, std::vector<int>& colors) {
                        const bool dbg = getenv("DAS_DEBUG_TIMING") != nullptr;
                        double tq = wall_seconds();
                        auto lap = [&](const char* what) { if (dbg) { double t2 = wall_seconds(); fprintf(stderr, "[dafoam_amd]     device graph: %s %.2f s\n", what, t2 - tq); tq = t2; } };
                        hipStream_t st = s->stream;
                        device_build_con(s, 0, &fullRowMajor);
                        fullTransposed = true;
                        lap("upload + transpose of the full pattern");
                        ConDev& c = s->cd[0];
                        const long long nKeep = (long long)keep.size();
                        std::vector<int> netOfRow((size_t)nn, -1);
                        for (long long q = 0; q < nKeep; q++) netOfRow[keep[q]] = (int)q;
                        DevBuf<int> d_net, d_crow, d_cpos;
                        d_net.upload(netOfRow);
                        DevBuf<long long> d_cptr;
                        DevBuf<unsigned char> d_start;
                        device_build_nets(nn, c.t_rowptr.p, c.t_col.p, d_net.p, fullRowMajor.rowptr.p, fullRowMajor.col.p, d_cptr, d_crow, d_cpos, d_start, st);
                        std::vector<unsigned char> isStart = d_start.to_host();
                        const std::vector<long long> gstart = color_groups_from_flags(nn, isStart);
                        lap("nets, positions, groups");
                        // a numbering whose lower-numbered 2-ring neighbours chain through (nearly) all cells - an O-grid whose ring j+1
                        // starts next to the END of ring j - serialises the data-flow sweep (2 M-cell NACA0012: 63 s until the watchdog
                        // fired, round 3): estimated on the cell graph BEFORE the launch, such meshes go straight to the speculative rounds
                        const bool autoAlg = s->opt.gets("amd.coloringAlgorithm") == "auto";
                        const long long depth = autoAlg ? cell_chain_depth(s->mesh) : 0;
                        const bool deep = autoAlg && depth > std::max<long long>(20000, s->mesh.nC / 50);
                        if (s->opt.geti("debug") && autoAlg) fprintf(stderr, "[dafoam_amd] colouring: dependency depth of the cell numbering ~%lld (%d cells) -> %s\n", depth, s->mesh.nC, deep ? "speculative rounds" : "data-flow first-fit");
                        const int rc = deep ? -1 : color_firstfit_run(nn, nKeep, gstart, d_cptr.p, d_crow.p, d_cpos.p, colors, st);
                        lap(deep ? "dependency-depth estimate" : "first-fit kernel");
                        bool ok = rc == 1;
                        if (rc == -1) {
                            // the watchdog stopped the data-flow sweep (a numbering without wavefront parallelism): the
                            // order-independent rounds over the same bitmaps; net -> columns = the kept rows of the pattern
                            const JacCon& jc = s->con_full;
                            std::vector<long long> krp((size_t)nKeep + 1, 0);
                            long long maxNet = 0;
                            for (long long q = 0; q < nKeep; q++) {
                                const long long len = jc.rowptr[keep[q] + 1] - jc.rowptr[keep[q]];
                                krp[q + 1] = krp[q] + len;
                                maxNet = std::max(maxNet, len);
                            }
                            DevBuf<long long> d_krp, d_keep;
                            d_krp.upload(krp); d_keep.upload(keep);
                            DevBuf<int> d_kcol((size_t)std::max<long long>(1, krp[nKeep]));
                            hipLaunchKernelGGL(k_rows_gather, dim3((unsigned)((nKeep + 3) / 4)), dim3(256), 0, st, nKeep, d_keep.p, fullRowMajor.rowptr.p, fullRowMajor.col.p,
                                               d_krp.p, d_kcol.p);
                            DAS_HIP(hipGetLastError());
                            ok = color_speculative_run(nn, nKeep, maxNet, d_cptr.p, d_crow.p, d_krp.p, d_kcol.p, colors, st, &s->colorRounds);
                            lap("speculative rounds");
                        }
                        fullRowMajor.rowptr.release(); fullRowMajor.col.release();
                        if (!ok) fprintf(stderr, "[dafoam_amd] device colouring gave up (too many colours or a timeout): host first-fit instead\n");
                        return ok;
                    };
            }
            s->nColors = d2_coloring(s->con_full, s->colors, ctr.data(), fn, gfn);
        }
    }
    double t3 = wall_seconds();
    DAS_CHECK(validate_coloring(s->con_full, s->colors), DAS_ERR_INTERNAL, "Conflicting Colors Found!");
    double t4 = wall_seconds();
    transposer.join();
    if (tErr) std::rethrow_exception(tErr);
    s->con_full.build_colour_lists(s->colors);
    s->con_pc.build_colour_lists(s->colors);
    if (devGraph) {
        if (!fullTransposed) device_build_con(s, 0);
        device_build_con(s, 1);
    }
    if (s->opt.geti("debug"))
        fprintf(stderr, "[dafoam_amd] runColoring: patterns %.2f s, colouring %.2f s, validate %.2f s, wait for the second thread + colour lists %.2f s\n",
                t2 - t1, t3 - t2, t4 - t3, wall_seconds() - t4);
    s->colored = true;
    if (s->opt.geti("debug"))
        fprintf(stderr, "[dafoam_amd] dRdWCon: n=%lld nnz=%lld (PC %lld) colours=%d  %.2f s\n", s->n, s->con_full.nnz, s->con_pc.nnz,
                s->nColors, wall_seconds() - t);
}

static ConDev& ensure_con_dev(das_solver* s, int isPC) {
    ensure_coloring(s);
    ConDev& c = s->cd[isPC ? 1 : 0];
    if (!c.ready) {
        const JacCon& j = isPC ? s->con_pc : s->con_full;
        c.cl_cols.upload(j.cl_cols);
        if (c.onDevice) {
            if (!c.t_col.p) device_build_con(s, isPC);  // released after an assembly (amd.keepAssemblyMaps 0): generated again
        } else {
            c.t_rowptr.upload(j.t_rowptr);
            c.t_col.upload(j.t_col.data(), j.t_col.size());
        }
        s->d_colors.upload(s->colors);
        c.ready = true;
    }
    return c;
}

static void spmv(das_solver* s, const Mat& A, const double* x, double* y) {
    hipEvent_t ev = nullptr;
    // sharded: ghost rows first (their contributions travel to the owner ranks while the owned rows are computed)
    if (s->halo.active) s->halo.begin(A, x, s->stream);
    s->timer.begin("spmv", s->stream, ev);
    launch_spmv(s->stream, A.n, A.rowptr.p, A.col.p, A.val.p, A.vp, x, y);
    s->timer.end("spmv", s->stream, ev);
    if (s->halo.active) {
        hipEvent_t eh = nullptr;
        s->timer.begin("halo", s->stream, eh);
        s->halo.finish(y, s->stream);
        s->timer.end("halo", s->stream, eh);
    } else if (s->halo_cb) {  // legacy transport: the whole halo reduction in a host callback
        hipEvent_t eh = nullptr;
        s->timer.begin("halo", s->stream, eh);
        s->halo_cb(y, s->comm_user);
        s->timer.end("halo", s->stream, eh);
    }
}

// ---- coloured assembly: DAPartDeriv::calcPartDerivMat (reference DAPartDeriv.C:350-473) -----------------------
static das_mat* assemble(das_solver* s, int isPC, int mode) {
    need_init(s);
    ConDev& c = ensure_con_dev(s, isPC);
    const JacCon& jc = isPC ? s->con_pc : s->con_full;
    const long long n = s->n;
    ResParams prm = make_params(s->cp, s->opt, isPC);
    // amd.pcUpwindBlend > 0: the PC residual carries the linearUpwindV correction, i.e. grad(U) of the upwind cell - URes then reaches U two
    // rings away and the PC pattern must keep that level.  Through src -> HbyA the correction also enters pRes / phiRes one
    // ring beyond their PC levels (2 / 1): those derivatives are NOT in the reduced pattern; the coloured differences fold them into
    // in-pattern entries of the same colour - an accepted approximation of the PRECONDITIONER matrix only, the operator
    // dRdW^T always uses the full tables
    // A user table with URes < 2 gets the reference's upwind div(pc) back (weight 0) with a warning instead of an error.
    if (isPC && prm.convBlend > 0.0 && s->cp.solver != DAS_SOLVER_SCALARTRANSPORTFOAM && s->cp.solver != DAS_SOLVER_HEATTRANSFERFOAM && s->cp.solver != DAS_SOLVER_SOLIDDISPLACEMENTFOAM && s->opt.geti("maxResConLv4JacPCMat.URes") < 2) {
        static bool warned = false;
        if (!warned) fprintf(stderr, "[dafoam_amd] warning: amd.pcUpwindBlend %.3g needs maxResConLv4JacPCMat.URes >= 2 (the second-order correction reaches two cell rings); "
                                     "the PC matrix is assembled with the upwind div(pc) (weight 0) instead\n", prm.convBlend);
        warned = true;
        prm.convBlend = 0.0;
    }
    DevBuf<double> vals(jc.nnz);
    vals.zero();
    const int B = 256;
    hipStream_t st = s->stream;
    if (mode == 1) {
        if (s->d_Wd.n != (size_t)n) { s->d_Wd.alloc(n); s->d_Rd.alloc(n); }
        for (int col = 0; col < s->nColors; col++) {
            hipLaunchKernelGGL(k_seed<1>, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_W.p, s->d_colors.p, s->d_scale.p, col, s->d_Wd.p);
            eval_residual<Dual<1>>(s->dm, s->cp, prm, s->d_Wd.p, s->d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
            const long long q0 = jc.cl_ptr[col], cnt = jc.cl_ptr[col + 1] - q0;
            if (cnt > 0)
                hipLaunchKernelGGL(k_scatter_dual, dim3(nblk(cnt, 16)), dim3(B), 0, st, cnt, s->d_Rd.p, c.cl_cols.p + q0, c.t_rowptr.p, c.t_col.p, vals.p);
        }
    } else {
        const double delta = s->opt.getd("adjPartDerivFDStep.State");
        if (s->d_R0.n != (size_t)n) { s->d_R0.alloc(n); s->d_Wp.alloc(n); }
        // the heat sources do not depend on the states: the difference quotients are taken of the residual without them, so that the
        // term does not cost the difference its low digits and the matrix has the bits it has without a source
        DevMesh dmJ = s->dm;
        dmJ.src = nullptr;
        eval_residual<double>(dmJ, s->cp, prm, s->d_W.p, s->d_R0.p, s->wk, s->d_phiF.p, s->d_Told.p, st);
        for (int col = 0; col < s->nColors; col++) {
            hipLaunchKernelGGL(k_perturb, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_W.p, s->d_colors.p, s->d_scale.p, col, delta, s->d_Wp.p);
            eval_residual<double>(dmJ, s->cp, prm, s->d_Wp.p, s->d_R.p, s->wk, s->d_phiF.p, s->d_Told.p, st);
            const long long q0 = jc.cl_ptr[col], cnt = jc.cl_ptr[col + 1] - q0;
            if (cnt > 0)
                hipLaunchKernelGGL(k_scatter_fd, dim3(nblk(cnt, 16)), dim3(B), 0, st, cnt, s->d_R.p, s->d_R0.p, 1.0 / delta, c.cl_cols.p + q0,
                                   c.t_rowptr.p, c.t_col.p, vals.p);
        }
    }
    DAS_HIP(hipGetLastError());
    // jacLowerBounds filter + compaction (reference DAPartDeriv.C:192-201; default bound 1e-30 drops exact zeros)
    double bound = s->opt.getd(isPC ? "jacLowerBounds.dRdWPC" : "jacLowerBounds.dRdW");
    std::unique_ptr<das_mat> out(new das_mat);
    Mat& M = out->m;
    M.n = n;
    const bool masked = !s->owned.empty();
    // columns kept on a sharded rank: the owned residuals; the PC matrix also keeps the residuals of the Schwarz overlap
    const unsigned char* colMask = !masked ? (const unsigned char*)nullptr : ((isPC && !s->pcMask.empty()) ? s->d_pcMask.p : s->d_owned.p);
    const bool useBound = !(bound < 1.0e-16);
    if (!useBound && !masked) {
        M.nnz = jc.nnz;
        if (c.onDevice) {
            M.rowptr.alloc((size_t)n + 1);
            M.col.alloc((size_t)std::max<long long>(1, jc.nnz));
            DAS_HIP(hipMemcpyAsync(M.rowptr.p, c.t_rowptr.p, (n + 1) * sizeof(long long), hipMemcpyDeviceToDevice, st));
            DAS_HIP(hipMemcpyAsync(M.col.p, c.t_col.p, jc.nnz * sizeof(int), hipMemcpyDeviceToDevice, st));
        } else {
            M.rowptr.upload(jc.t_rowptr);
            M.col.upload(jc.t_col.data(), jc.t_col.size());
        }
        M.val = std::move(vals);
    } else {
        M.nnz = filter_compact(n, c.t_rowptr.p, c.t_col.p, vals.p, bound, useBound, colMask, M.rowptr, M.col, M.val, st);
    }
    DAS_HIP(hipStreamSynchronize(st));
    // the per-colour scatter lists and the transposed structure are only needed during assembly: at 2 M cells they hold
    // ~40 GB of HBM that the Krylov basis can use (they are re-uploaded from the host copies by the next assembly)
    if (!s->opt.geti("amd.keepAssemblyMaps")) {
        c.cl_cols.release(); c.t_col.release(); c.t_rowptr.release();
        c.ready = false;
    }
    return out.release();
}

// ---- RAS + ILU(k) setup (host, OpenMP over blocks; one-off per PC matrix) ----------------------------------------
// Mirrors the reference's PC stack (DALinearEqn.C:199-299): additive Schwarz with overlap `asmOverlap` (here: cell
// rings around an RCB sub-domain, restricted variant) and ILU(`pcFillLevel`) sub-solves with a non-zero pivot shift.
// Unknowns are ordered cell-by-cell inside a block (cf. adjStateOrdering "cell", DAIndex.C:602-651), which the oracle
// study in DESIGN.md section 6 shows to be the better ILU ordering for this system.
#include "das_ilu_host.hpp"  // BlockFactor, ilu_symbolic, factor_local

// host threads of a preconditioner set-up: every block touches ~100 MB of fresh host memory; beyond a few dozen threads the kernel's
// page-fault / mmap paths serialise (measured on the 256-core MI355X host), hence the cap amd.setupThreads
static int pc_setup_threads(das_solver* s) { return (int)std::max<long long>(1, std::min<long long>(das::host_threads(), s->opt.geti("amd.setupThreads"))); }

static void setup_block_ilu(das_solver* s, das_ksp* k) {
    double t0 = wall_seconds();
    const Mat& A = k->pcmat->m;
    const long long n = A.n;
    std::vector<long long> rp = A.rowptr.to_host();
    uvector<int> ci(A.col.n);  // uninitialised: filled by the download (no serial zero-fill of GB-sized buffers)
    uvector<double> av(A.val.n);
    A.col.download(ci.data(), ci.size());
    A.val.download(av.data(), av.size());
    const Mesh& m = s->mesh;
    const long long bc = std::max<long long>(64, s->opt.geti("amd.pcBlockCells"));
    const int overlap = (int)std::max<long long>(0, s->opt.geti("adjEqnOption.asmOverlap"));
    const int lfill = (int)std::max<long long>(0, s->opt.geti("adjEqnOption.pcFillLevel"));
    // compact sub-domains by recursive coordinate bisection of the cell centres (the reference decomposes with
    // scotch, pyDAFoam.py:597-604; RCB gives comparable compact blocks without a graph library)
    // multi-GPU: only cells owned by this rank take part (block-Jacobi across ranks, like the reference's one
    // ASM sub-domain per MPI rank); a cell is owned iff its first cell-state is owned
    const std::vector<char> cellOwned = cells_of_mask(m, s->st_full.states, s->owned);
    long long nOwnedStates = n;
    if (!s->owned.empty()) {
        nOwnedStates = 0;
        for (unsigned char o : s->owned) nOwnedStates += o ? 1 : 0;
    }
    std::vector<int> cellOrder;
    cellOrder.reserve(m.nC);
    for (int c = 0; c < m.nC; c++) if (cellOwned[c]) cellOrder.push_back(c);
    std::vector<long long> cboff;
    rcb_leaves(cellOrder, [&](int c, int d) { return m.cg[c].C[d]; }, bc, cboff);
    const int nB = (int)cboff.size() - 1;
    for (int b = 0; b < nB; b++) std::sort(cellOrder.begin() + cboff[b], cellOrder.begin() + cboff[b + 1]);
    std::vector<std::vector<int>> owned(m.nC);
    bool hasFace = false;
    for (const StateDef& sd : s->st_full.states) if (sd.kind == KIND_FACE) hasFace = true;
    if (hasFace) for (int f = 0; f < m.nF; f++) owned[m.owner[f]].push_back(f);

    std::vector<BlockFactor> BF(nB);
    std::string err;
    const double t_prep = wall_seconds();
    const int nthr = pc_setup_threads(s);
#pragma omp parallel num_threads(nthr)
    {
        std::vector<int> cmark(m.nC, -1);
        std::vector<int> loc(n, -1);
        std::vector<int> ext, frontier, nxt;
        std::vector<long long> lrp;
        std::vector<int> lci;
        std::vector<double> lv;
        std::vector<std::pair<int, double>> row;
        std::vector<long long> where;
        std::vector<int> lev;
#pragma omp for schedule(dynamic, 1)
        for (int b = 0; b < nB; b++) {
            try {
                BlockFactor& F = BF[b];
                // core + overlap rings of cells
                ext.clear();
                frontier.clear();
                for (long long q = cboff[b]; q < cboff[b + 1]; q++) { int c = cellOrder[q]; cmark[c] = b; ext.push_back(c); frontier.push_back(c); }
                const size_t ncore = ext.size();
                for (int ring = 0; ring < overlap; ring++) {
                    nxt.clear();
                    for (int c : frontier)
                        for (int q = m.cc_ptr[c]; q < m.cc_ptr[c + 1]; q++) {
                            int y = m.cc[q];
                            if (cmark[y] != b && cellOwned[y]) { cmark[y] = b; ext.push_back(y); nxt.push_back(y); }
                        }
                    frontier.swap(nxt);
                }
                // mark core membership: core cells are the first ncore entries of ext; sort all ext cells
                std::vector<char> isCore(ext.size(), 0);
                {
                    std::vector<std::pair<int, char>> tmp(ext.size());
                    for (size_t q = 0; q < ext.size(); q++) tmp[q] = {ext[q], (char)(q < ncore)};
                    std::sort(tmp.begin(), tmp.end());
                    for (size_t q = 0; q < ext.size(); q++) { ext[q] = tmp[q].first; isCore[q] = tmp[q].second; }
                }
                // unknown list, cell by cell
                for (size_t q = 0; q < ext.size(); q++) {
                    long long c = ext[q];
                    auto push = [&](long long g) {
                        if (!s->owned.empty() && !s->owned[g]) return;  // e.g. cut-patch faces of the extended mesh
                        F.gidx.push_back((int)g);
                        F.gout.push_back(isCore[q] ? (int)g : -1);
                    };
                    for (const StateDef& sd : s->st_full.states) {
                        if (sd.kind == KIND_VEC) for (int k2 = 0; k2 < 3; k2++) push(sd.offset + 3 * c + k2);
                        else if (sd.kind == KIND_SCL) push(sd.offset + c);
                    }
                    for (const StateDef& sd : s->st_full.states)
                        if (sd.kind == KIND_FACE) for (int f : owned[c]) push(sd.offset + f);
                }
                const int nl = (int)F.gidx.size();
                for (int p = 0; p < nl; p++) loc[F.gidx[p]] = p;
                // local matrix (block-restricted rows of dRdWTPC), sorted columns
                lrp.assign(nl + 1, 0);
                lci.clear();
                lv.clear();
                for (int p = 0; p < nl; p++) {
                    int g = F.gidx[p];
                    row.clear();
                    for (long long q = rp[g]; q < rp[g + 1]; q++) {
                        int lc = loc[ci[q]];
                        if (lc >= 0) row.push_back({lc, av[q]});
                    }
                    std::sort(row.begin(), row.end());
                    for (auto& e : row) { lci.push_back(e.first); lv.push_back(e.second); }
                    lrp[p + 1] = (long long)lci.size();
                }
                for (int p = 0; p < nl; p++) loc[F.gidx[p]] = -1;
                factor_local(nl, lrp, lci, lv, lfill, F, where, lev, nullptr);
                F.nnzLU = (long long)F.fci.size();
                std::vector<long long>().swap(F.frp); std::vector<long long>().swap(F.fdiag); std::vector<int>().swap(F.fci);
                std::vector<double>().swap(F.fv); std::vector<int>().swap(F.Lrows); std::vector<int>().swap(F.Urows);
            } catch (const std::exception& e) {
#pragma omp critical
                err = e.what();
            }
        }
    }
    DAS_CHECK(err.empty(), DAS_ERR_INTERNAL, "block ILU setup failed: " + err);
    const double t_fact = wall_seconds();
    // concatenate the per-block streams (offsets by prefix sums, copies in parallel)
    BlockILU& P = k->pc;
    std::vector<long long> boff(nB + 1, 0), eoff[2], loff[2], slev[2], slevOff[2];
    long long next = 0, fnnz = 0;
    int maxLocal = 0, maxLv = 0, nshift = 0;
    for (int t = 0; t < 2; t++) { eoff[t].assign(nB + 1, 0); loff[t].assign(nB + 1, 0); }
    P.h_core_off.assign(1, 0);
    for (int b = 0; b < nB; b++) {
        const BlockFactor& F = BF[b];
        const int nl = (int)F.gidx.size();
        boff[b + 1] = boff[b] + nl;
        maxLocal = std::max(maxLocal, nl);
        nshift += F.nshift;
        fnnz += F.nnzLU;
        long long ncore = 0;
        for (int g : F.gout) ncore += g >= 0 ? 1 : 0;
        P.h_core_off.push_back(P.h_core_off.back() + ncore);
        for (int t = 0; t < 2; t++) {
            eoff[t][b + 1] = eoff[t][b] + (long long)F.sval[t].size();
            loff[t][b + 1] = loff[t][b] + (long long)F.slev[t].size();
            maxLv = std::max<int>(maxLv, (int)F.slev[t].size() - 1);
        }
    }
    next = boff[nB];
    std::vector<int> gidx(next), gout(next);
    std::vector<double> invd(next);
    P.h_core_perm.assign(P.h_core_off.back(), 0);
    for (int t = 0; t < 2; t++) { slev[t].resize(loff[t][nB]); slevOff[t] = loff[t]; }
#pragma omp parallel for schedule(dynamic, 1) num_threads(das::host_threads())
    for (int b = 0; b < nB; b++) {
        BlockFactor& F = BF[b];
        std::copy(F.gidx.begin(), F.gidx.end(), gidx.begin() + boff[b]);
        std::copy(F.gout.begin(), F.gout.end(), gout.begin() + boff[b]);
        std::copy(F.invd.begin(), F.invd.end(), invd.begin() + boff[b]);
        long long pc = P.h_core_off[b];
        for (int g : F.gout) if (g >= 0) P.h_core_perm[pc++] = g;
        for (int t = 0; t < 2; t++)
            for (size_t q = 0; q < F.slev[t].size(); q++) slev[t][loff[t][b] + q] = eoff[t][b] + F.slev[t][q];
    }
    DAS_CHECK((long long)P.h_core_perm.size() == nOwnedStates, DAS_ERR_INTERNAL, "block cores do not cover all owned states exactly once");
    P.n = n; P.next = next; P.nBlocks = nB; P.fnnz = fnnz; P.maxLevels = maxLv; P.maxLocal = maxLocal;
    P.boff.upload(boff); P.gidx.upload(gidx); P.gout.upload(gout); P.invd.upload(invd);
    // mixed precision: the factors of the (approximate) preconditioner may be stored in fp32 - the operator, the
    // Krylov vectors and the block work vector stay fp64 (amd.pcFactorFP32; SURVEY.md section 7 "hard parts")
    P.factor32 = s->opt.geti("amd.pcFactorFP32") != 0;
    // the entry streams (GBs) go from the per-block vectors straight into their slice of the device buffers: no
    // concatenated host copy (its serial first-touch used to cost seconds)
    for (int t = 0; t < 2; t++) {
        const size_t tot = (size_t)eoff[t][nB];
        if (P.factor32) { P.svalf[t].alloc(tot); P.sval[t].release(); }
        else { P.sval[t].alloc(tot); P.svalf[t].release(); }
        P.srowcol[t].alloc(tot);
        P.slev[t].upload(slev[t]); P.slevOff[t].upload(slevOff[t]);
    }
    {
        std::vector<float> f32;
        for (int b = 0; b < nB; b++) {
            BlockFactor& F = BF[b];
            for (int t = 0; t < 2; t++) {
                const size_t cnt = F.sval[t].size();
                if (!cnt) continue;
                if (P.factor32) {
                    f32.assign(F.sval[t].begin(), F.sval[t].end());
                    DAS_HIP(hipMemcpy(P.svalf[t].p + eoff[t][b], f32.data(), cnt * sizeof(float), hipMemcpyHostToDevice));
                } else {
                    DAS_HIP(hipMemcpy(P.sval[t].p + eoff[t][b], F.sval[t].data(), cnt * sizeof(double), hipMemcpyHostToDevice));
                }
                DAS_HIP(hipMemcpy(P.srowcol[t].p + eoff[t][b], F.src[t].data(), cnt * sizeof(unsigned), hipMemcpyHostToDevice));
            }
            F = BlockFactor();
        }
    }
    P.useLDS = (size_t)maxLocal * sizeof(double) + (size_t)(maxLv + 2 * PC_PF + 8) * sizeof(int) + 16 <= 160 * 1024;
    if (!P.useLDS) P.xw.alloc(next);
    else DAS_HIP(hipFuncSetAttribute((const void*)k_ras_apply<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    P.view.nBlocks = nB; P.view.boff = P.boff.p; P.view.gidx = P.gidx.p; P.view.gout = P.gout.p; P.view.invd = P.invd.p;
    P.view.factor32 = P.factor32 ? 1 : 0;
    for (int t = 0; t < 2; t++) { P.view.sval[t] = P.sval[t].p; P.view.svalf[t] = P.svalf[t].p; P.view.srowcol[t] = P.srowcol[t].p; P.view.slev[t] = P.slev[t].p; P.view.slevOff[t] = P.slevOff[t].p; }
    P.view.xglob = P.xw.p;
    P.setup_seconds = wall_seconds() - t0;
    if (s->opt.geti("debug"))
        fprintf(stderr, "[dafoam_amd] RAS(overlap %d)+ILU(%d): %d blocks, n_ext=%lld (%.2fx), nnz(LU)=%lld, max block %d unknowns (%s), max levels %d, "
                        "%d shifted pivots, %.2f s (download+partition %.2f, factorise %.2f, streams+upload %.2f)\n", overlap, lfill, nB, next,
                (double)next / n, fnnz, maxLocal, P.useLDS ? "LDS" : "global", maxLv, nshift, P.setup_seconds, t_prep - t0, t_fact - t_prep,
                wall_seconds() - t_fact);
}

// reach (in cell rings, measured between the cells that own the unknowns) of the PC connectivity: level lv of a residual,
// +1 if the level lists a face state (the face of a ring-lv cell may be owned by its neighbour), +1 for a face residual
// (anchored at either adjacent cell, owned by one of them)
static int pc_stencil_reach(das_solver* s) {
    ensure_coloring(s);
    int reach = 0;
    for (size_t b = 0; b < s->st_pc.states.size(); b++)
        for (size_t lv = 0; lv < s->st_pc.levels[b].size(); lv++) {
            const unsigned mask = s->st_pc.levels[b][lv];
            if (!mask) continue;
            bool faceState = false;
            for (size_t q = 0; q < s->st_pc.states.size(); q++) if ((mask >> q & 1u) && s->st_pc.states[q].kind == KIND_FACE) faceState = true;
            reach = std::max<int>(reach, (int)lv + (faceState ? 1 : 0) + (s->st_pc.states[b].kind == KIND_FACE ? 1 : 0));
        }
    return reach;
}

// adjEqnOption.jacMatReOrdering (DALinearEqn.C:82-83,238-290): ordering of the unknowns inside the sub-domain ILU.
// "natural" = the mesh's cell numbering, "rcm" = reverse Cuthill-McKee of the cell graph; the others are rejected.
static bool pc_ordering_rcm(das_solver* s) {
    const std::string& o = s->opt.gets("adjEqnOption.jacMatReOrdering");
    DAS_CHECK(o == "natural" || o == "rcm", DAS_ERR_ARG, "adjEqnOption.jacMatReOrdering \"" + o + "\" is not implemented (natural | rcm)");
    return o == "rcm";
}

// mean velocity direction (elimination orders 4 ... 7: along / against the flow); x if there is no velocity state
static void pc_flow_direction(das_solver* s, double* dir) {
    dir[0] = 1.0; dir[1] = 0.0; dir[2] = 0.0;
    if (!s->st_full.states.empty() && s->st_full.states[0].kind == KIND_VEC && s->h_W.size() == (size_t)s->n) {
        const StateDef& u = s->st_full.states[0];
        double m[3] = {0, 0, 0};
        for (long long c = 0; c < u.size / 3; c++) for (int q = 0; q < 3; q++) m[q] += s->h_W[u.offset + 3 * c + q];
        const double nm = std::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
        if (nm > 0.0) for (int q = 0; q < 3; q++) dir[q] = m[q] / nm;
    }
}

// several ranks: the sub-domain of this rank = its owned unknowns, or - asmOverlap > 0 - those plus the overlap rings (das_set_pc_overlap)
static const std::vector<unsigned char>& pc_mask(das_solver* s, das_ksp* k) { return (s->pcMask.empty() || k->pcTranspose) ? s->owned : s->pcMask; }
// the elimination order the options ask for (orders: das_bilu.hpp)
static int pc_configured_order(das_solver* s, das_ksp* k) { return k->pcOrder >= 0 ? k->pcOrder : (pc_ordering_rcm(s) ? 1 : 0); }
// a DEEP order: levels >> nodes^(1/3) - e.g. reverse Cuthill-McKee of a thin far-field block, 23755 levels for 270 k nodes where ~500 are normal
static bool pc_order_is_deep(int levels, int nodes) { return (double)levels > 30.0 * std::cbrt((double)std::max(1, nodes)); }
static const char* rank_label() { return getenv("RANK") ? getenv("RANK") : "0"; }

// what every node-block ILU set-up (das_bilu.hpp) takes from the solver: stencil reach, set-up threads, flow direction, factor precision
struct BiluInputs {
    const Mat& A;
    int reach, nthr;
    bool fp32, debug;
    double dir[3];
    BiluInputs(das_solver* s, das_ksp* k)
        : A(k->pcmat->m), reach(pc_stencil_reach(s)), nthr(pc_setup_threads(s)), fp32(s->opt.geti("amd.pcFactorFP32") != 0), debug(s->opt.geti("debug") != 0) { pc_flow_direction(s, dir); }
};
// global node-block ILU(0): one incomplete factorisation of dRdWTPC over `mask`'s unknowns in elimination order `order`
static void factorise_node_ilu(das_solver* s, das_ksp* k, NodeILU& P, const std::vector<unsigned char>& mask, int order) {
    const BiluInputs in(s, k);
    bilu_setup(s->mesh, s->st_full.states, s->n, mask, in.reach, in.fp32, in.A.n, in.A.rowptr.p, in.A.col.p, in.A.val.p, s->stream,
               P, in.debug, in.nthr, order, k->pcTranspose, k->pcDiagScale, k->shiftExLo, k->shiftExHi, k->shiftEnd, in.dir);
}
// what every node-block ILU set-up ends with: k->bilu holds the factorisation of nBlocks sub-domains, set up since t0
static void pc_finish_bilu(das_solver* s, das_ksp* k, double t0, int nBlocks, bool rasOverlap) {
    k->useBilu = true;
    k->rasOverlap = rasOverlap;
    if (k->rasOverlap && k->pcin.n != (size_t)s->n) k->pcin.alloc(s->n);
    k->pc.setup_seconds = wall_seconds() - t0;
    k->pc.nBlocks = nBlocks;
    k->pc.fnnz = (k->bilu.nL + k->bilu.nU + k->bilu.nNodes) * (long long)BILU_NB2;
    k->pc.next = (long long)k->bilu.nNodes * BILU_NB;
}

// Stability estimate of the incomplete factorisation: max |(LU)^-1 P e - e| over the sub-domain's unknowns for e = ones and for a +-1
// pattern.  O(1) for a usable factorisation (it is ||I - M^-1 P|| on two vectors), 1e10 and more when the triangular recurrences of an
// ILU of a not diagonally dominant matrix grow exponentially (Chow & Saad 1997, "Experimental study of ILU preconditioners for
// indefinite matrices": the ||(LU)^-1 e|| test) - which the blended second-order PC matrix (amd.pcUpwindBlend) does for some elimination
// orders: round 6, 403 k-cell wing, sectors without overlap and 8 index blocks: M^-1 amplifies by 1e16, GMRES makes no progress.
static double pc_stability_estimate(das_solver* s, das_ksp* k, NodeILU& F, const std::vector<unsigned char>& mask) {
    const long long n = s->n;
    const Mat& P = k->pcmat->m;
    std::vector<double> e(n), z(n);
    DevBuf<double> de(n), dw(n), dz(n);
    double est = 0.0;
    long long worst = -1;
    for (int trial = 0; trial < 2; trial++) {
        for (long long i = 0; i < n; i++) {
            const bool in = mask.empty() || mask[i];
            unsigned long long hsh = (unsigned long long)i * 0x9E3779B97F4A7C15ull;
            hsh ^= hsh >> 29;
            e[i] = !in ? 0.0 : (trial == 0 ? 1.0 : ((hsh & 1ull) ? 1.0 : -1.0));
        }
        de.upload(e);
        hipLaunchKernelGGL(k_spmv_wave, SPMV_GRID(P.n), dim3(256), 0, s->stream, P.n, P.rowptr.p, P.col.p, P.val.p, (const double*)de.p, dw.p);
        dz.zero();
        bilu_apply(F, dw.p, dz.p, s->stream);
        DAS_HIP(hipStreamSynchronize(s->stream));
        z = dz.to_host();
        const int* nu = F.h_nodeUnk.data();
        for (size_t q = 0; q < F.h_nodeUnk.size(); q++) {
            const int gi = nu[q];
            if (gi < 0) continue;
            const double d = std::fabs(z[gi] - e[gi]);
            if (d > est || d != d) worst = gi;
            est = (d > est || d != d) ? (d != d ? 1e300 : d) : est;
        }
    }
    if (worst >= 0 && getenv("DAS_PC_STAB")) {  // where the worst entry sits (state, cell / face centre, frozen wall distance)
        for (const StateDef& sd : s->st_full.states) {
            if (worst < sd.offset || worst >= sd.offset + sd.size) continue;
            const long long ent = (worst - sd.offset) / (sd.kind == KIND_VEC ? 3 : 1);
            const double* C = sd.kind == KIND_FACE ? s->mesh.fg[ent].Cf : s->mesh.cg[ent].C;
            fprintf(stderr, "[dafoam_amd] rank %s: worst entry of the stability test: state %s entity %lld at (%.4g %.4g %.4g)%s\n", rank_label(),
                    sd.name.c_str(), ent, C[0], C[1], C[2], (!s->owned.empty() && !s->owned[worst]) ? " (overlap ring)" : "");
        }
    }
    return est;
}

// Factorise `mask`'s unknowns into F with an elimination order chosen by the stability estimate (amd.pcStabilityLimit > 0; else the configured
// order, no estimate).  Candidates: the configured order, then amd.pcOrderCandidates.  pickMin: every candidate is factorised and the one
// with the smallest estimate kept (sub-domains of an additive-Schwarz preconditioner: their triangular recurrences blow up or not, and
// transport information well or badly, depending on the direction the elimination crosses them - round 6: 403 k-cell wing on 8 ranks, outer
// blocks next to the wake: 1e8 ... 1e27 in one order, 1e2 in another; 2 M cells on 4 ranks: 691 iterations with the smallest-estimate
// orders, > 1000 with reverse Cuthill-McKee everywhere); otherwise the first candidate below the limit.  Local to the rank: no collective.
static void choose_order_and_factorise(das_solver* s, das_ksp* k, NodeILU& F, const std::vector<unsigned char>& mask, bool pickMin, int& orderUsed, double& estimate,
                                       bool earlyAccept = true) {
    const int configured = pc_configured_order(s, k);
    const double limit = s->opt.getd("amd.pcStabilityLimit");
    if (!(limit > 0.0)) {
        F = NodeILU();
        factorise_node_ilu(s, k, F, mask, configured);
        orderUsed = -1; estimate = -1.0;
        return;
    }
    std::vector<int> cand{configured};
    {
        std::string lst = s->opt.gets("amd.pcOrderCandidates");
        if (getenv("DAS_BILU_ORDER_LIST")) { lst = getenv("DAS_BILU_ORDER_LIST"); cand.clear(); }
        for (size_t q = 0; q < lst.size(); q++)
            if (lst[q] >= '0' && lst[q] <= '7') { const int o = lst[q] - '0'; if (std::find(cand.begin(), cand.end(), o) == cand.end()) cand.push_back(o); }
        if (cand.empty()) cand.push_back(configured);
    }
    if (getenv("DAS_BILU_PICK_MIN")) pickMin = atoi(getenv("DAS_BILU_PICK_MIN")) != 0;
    const double good = s->opt.getd("amd.pcStabilityGood");  // pickMin: an estimate this small ends the search
    // every evaluated candidate: (order, estimate, dependency levels).  The levels matter for sub-domains: the merged structure of
    // amd.pcSubdomains runs max(levels over the blocks) dependent hops - one block in a deep order (round 6, 2 M cells, K = 6 / 8: a
    // Cuthill-McKee order of a thin block) leaves thousands of levels with a handful of nodes each: 108 - 151 ms per apply instead of 6.
    // Among the candidates below the limit only those within 1.5 x the shallowest compete for the smallest estimate.
    struct Cand { int o; double est; int levels; };
    std::vector<Cand> seen;
    int last = -1;
    for (size_t attempt = 0; attempt < cand.size(); attempt++) {
        const int o = cand[attempt];
        F = NodeILU();
        factorise_node_ilu(s, k, F, mask, o);
        const double est = pc_stability_estimate(s, k, F, mask);
        last = o;
        seen.push_back({o, est, F.nLevels});
        if (s->opt.geti("debug") || getenv("DAS_PC_STAB") || (est > limit && !pickMin))
            fprintf(stderr, "[dafoam_amd] rank %s: preconditioner stability estimate max|(LU)^-1 P e - e| = %.3e with elimination order %d, %d levels (limit %.1e)%s\n",
                    rank_label(), est, o, F.nLevels, limit, (est > limit && !pickMin) ? ": unstable, trying another order" : "");
        const bool deep = pc_order_is_deep(F.nLevels, F.nNodes);  // (never accepted early)
        // (earlyAccept false - the sub-domains of a multi-rank solve: every candidate is evaluated; 403 k cells on 8 ranks: 722 iterations, with the
        //  early accept 867)
        if (est <= limit && (!pickMin || (earlyAccept && est <= good && !deep))) break;
    }
    bool anyOk = false;
    for (const Cand& c : seen) anyOk = anyOk || c.est <= limit;
    int minLv = 1 << 30;
    for (const Cand& c : seen) if (!anyOk || c.est <= limit) minLv = std::min(minLv, c.levels);
    int best = seen.back().o;
    double bestEst = 1e300;
    if (!pickMin && seen.back().est <= limit) bestEst = seen.back().est;  // first stable candidate (the loop stopped there)
    else
        for (const Cand& c : seen)
            if ((!anyOk || c.est <= limit) && (double)c.levels <= 1.5 * minLv && c.est < bestEst) { best = c.o; bestEst = c.est; }
    if (last != best) {
        F = NodeILU();
        factorise_node_ilu(s, k, F, mask, best);
    }
    if (bestEst > limit)
        fprintf(stderr, "[dafoam_amd] rank %s: no elimination order passes the stability limit; keeping order %d (estimate %.3e)\n", rank_label(), best, bestEst);
    orderUsed = best; estimate = bestEst;
}

// ONE node-block ILU over this rank's unknowns.  byEstimate (the adjoint): the elimination order is chosen by the stability estimate - a
// sub-domain of a multi-rank solve takes the order with the smallest estimate, one rank alone the first stable one; else (the Newton primal,
// which factorises again and again) the configured order
static void setup_node_ilu(das_solver* s, das_ksp* k, bool byEstimate) {
    const double t0 = wall_seconds();
    if (byEstimate) {
        choose_order_and_factorise(s, k, k->bilu, pc_mask(s, k), !s->owned.empty(), k->pcOrderUsed, k->pcStability, /*earlyAccept*/ s->owned.empty());
        if (k->pcOrderUsed >= 0) k->pcOrder = k->pcOrderUsed;
    } else {
        factorise_node_ilu(s, k, k->bilu, pc_mask(s, k), pc_configured_order(s, k));
    }
    pc_finish_bilu(s, k, t0, 1, !s->pcMask.empty() && !k->pcTranspose && s->halo.ovActive);
}

// amd.pcSubdomains: K > 1 sub-domain factorisations inside this rank (single-rank adjoint solves only); -1 = automatic: 4 from 1 M cells
static long long pc_subdomain_count(das_solver* s) {
    long long K = s->opt.geti("amd.pcSubdomains");
    if (!s->owned.empty()) return 1;
    if (K < 0) K = s->mesh.nC >= 1000000 ? 4 : 1;
    return std::max<long long>(1, std::min<long long>(K, 16));
}

// fn(unknown, cell) for every unknown with the cell it belongs to: cell states their cell, face states the face's owner cell
template <class Fn>
static void for_each_unknown_with_cell(das_solver* s, Fn fn) {
    const Mesh& m = s->mesh;
    for (const StateDef& sd : s->st_full.states) {
        if (sd.kind == KIND_VEC) { for (int c = 0; c < m.nC; c++) for (int q = 0; q < 3; q++) fn(sd.offset + 3LL * c + q, c); }
        else if (sd.kind == KIND_SCL) { for (int c = 0; c < m.nC; c++) fn(sd.offset + c, c); }
        else { for (long long f = 0; f < m.nF; f++) fn(sd.offset + f, m.owner[f]); }
    }
}

// Restricted additive Schwarz inside one GPU: K blocks of the cells by recursive coordinate bisection of the cell centres (K = 4 on a wing:
// the quadrants around the section, whole spanwise columns), each + adjEqnOption.asmOverlap rings of cells; one node-block ILU per block
// with its own elimination order (choose_order_and_factorise, smallest estimate), merged into ONE level structure (bilu_setup_multi): one pair
// of sweeps runs the K blocks together - max(levels) dependent hops, every level K times as wide - and only the owner block's copy of an
// overlap unknown writes the result.  (First version, K sweep pairs on K streams + a combine pass: 8.3 ms per apply at 2 M cells against
// 6.4 ms for the single factorisation - profiles/r07m_*, r07n_*.)
static bool setup_subdomain_ilus(das_solver* s, das_ksp* k, int K) {
    const double t0 = wall_seconds();
    const Mesh& m = s->mesh;
    const long long N = m.nC, n = s->n;
    // ---- RCB of the cell centres
    std::vector<int> cells(N), blockOf(N, 0);
    std::iota(cells.begin(), cells.end(), 0);
    rcb_parts(cells, [&](int c, int d) { return m.cg[c].C[d]; }, K, blockOf);
    // ---- unknown -> block (cell states: the cell's block; face states: the owner cell's)
    std::vector<unsigned char> subOf(n, 0);
    for_each_unknown_with_cell(s, [&](long long g, int c) { subOf[g] = (unsigned char)blockOf[c]; });
    const int overlap = (int)std::max<long long>(0, s->opt.geti("adjEqnOption.asmOverlap"));
    std::vector<std::vector<unsigned char>> masks(K);
    k->subOrder.assign(K, -1);
    k->subEst.assign(K, -1.0);
    for (int b = 0; b < K; b++) {
        std::vector<unsigned char> cellIn(N, 0), grown;
        for (long long c = 0; c < N; c++) cellIn[c] = blockOf[c] == b;
        for (int ring = 0; ring < overlap; ring++) {
            grown = cellIn;
            for (long long c = 0; c < N; c++) if (cellIn[c]) for (int q = m.cc_ptr[c]; q < m.cc_ptr[c + 1]; q++) grown[m.cc[q]] = 1;
            cellIn.swap(grown);
        }
        masks[b].assign(n, 0);
        for_each_unknown_with_cell(s, [&](long long g, int c) { masks[b][g] = cellIn[c]; });
        // the block's own factorisation: only to choose its elimination order (smallest stability estimate); released again
        NodeILU F;
        choose_order_and_factorise(s, k, F, masks[b], true, k->subOrder[b], k->subEst[b]);
        if (k->subOrder[b] < 0) k->subOrder[b] = pc_configured_order(s, k);
        if (s->opt.geti("debug") || getenv("DAS_PC_STAB"))
            fprintf(stderr, "[dafoam_amd] sub-domain %d of %d: %d nodes, %d levels, elimination order %d, stability estimate %.3e\n", b, K, F.nNodes, F.nLevels, k->subOrder[b], k->subEst[b]);
        // a block whose best order is still DEEP (levels >> nodes^(1/3): coordinate-bisection blocks that cut the grid lines of a swept wing
        // diagonally - round 6: 2489 ... 16618 levels for 540 k nodes, 13.9 ms per apply and more iterations than the single factorisation)
        // makes the merged structure slow: the caller falls back to ONE factorisation
        if (pc_order_is_deep(F.nLevels, F.nNodes) && s->opt.geti("amd.pcSubdomains") < 0) {
            fprintf(stderr, "[dafoam_amd] sub-domain %d of %d needs %d dependency levels for %d nodes: the blocks do not suit this mesh, one factorisation instead "
                            "(amd.pcSubdomains K > 1 forces the blocks)\n", b, K, F.nLevels, F.nNodes);
            k->subOrder.clear(); k->subEst.clear();
            return false;
        }
    }
    // ---- ONE merged level structure for the K blocks
    {
        const BiluInputs in(s, k);
        std::vector<const std::vector<unsigned char>*> mp;
        for (int b = 0; b < K; b++) mp.push_back(&masks[b]);
        k->bilu = NodeILU();
        bilu_setup_multi(s->mesh, s->st_full.states, n, mp, k->subOrder, subOf, in.reach, in.fp32, in.A.n, in.A.rowptr.p, in.A.col.p, in.A.val.p, s->stream, k->bilu,
                         in.debug, in.nthr, in.dir);
    }
    k->nSub = K;
    k->pcOrderUsed = k->subOrder[0];
    k->pcStability = 0.0;
    for (double e : k->subEst) k->pcStability = std::max(k->pcStability, e);
    pc_finish_bilu(s, k, t0, K, false);
    if (s->opt.geti("debug") || getenv("DAS_PC_STAB"))
        fprintf(stderr, "[dafoam_amd] %d sub-domains merged: %d nodes, %d levels (%.0f nodes per level)\n", K, k->bilu.nNodes, k->bilu.nLevels, (double)k->bilu.nNodes / std::max(1, k->bilu.nLevels));
    return true;
}

// E = Z^T P Z and its dense inverse for a coarse space of naggG aggregates of which [aggOff, aggOff + C.nagg) are this rank's;
// aggRowG[cell] = aggregate of every local cell that belongs to one (owned cells: aggOff + local id; multi-GPU ghost cells: the
// owner rank's numbering; -1: none).  With naggG > C.nagg the contributions of all ranks are summed (all-reduce) and every
// rank inverts the same matrix.
static void coarse_build_operator(das_solver* s, das_ksp* k, int naggG, int aggOff, const std::vector<int>& aggRowG) {
    das_ksp::CoarsePC& C = k->coarse;
    C.active = false;
    DAS_CHECK(naggG >= C.nagg && naggG <= 2048, DAS_ERR_ARG, "coarse space: at most 2048 aggregates in total (dense inverse)");
    const long long N = C.N;
    std::vector<int> aggOwn(N, -1);
    for (long long c = 0; c < N; c++) if (C.h_agg[c] >= 0) aggOwn[c] = aggOff + C.h_agg[c];
    std::vector<long long> aptrAll;
    std::vector<int> cellsAll;
    coarse_sort_cells(N, naggG, aggRowG.data(), aptrAll, cellsAll);
    C.naggG = naggG; C.aggOff = aggOff; C.global = naggG > C.nagg;
    C.azOpId = -1; C.azReady = false;  // the sparse A Z of the deflated mode belongs to the old aggregates
    C.agg.upload(aggOwn); C.aggRow.upload(aggRowG); C.cellsAll.upload(cellsAll); C.aptrAll.upload(aptrAll);
    DevBuf<double> E((size_t)naggG * naggG);
    const Mat& P = k->pcmat->m;
    // rows: cells of every aggregate present on this rank (transposed storage: rows = states); columns: owned residual cells
    coarse_assemble(naggG, C.aptrAll.p, C.cellsAll.p, N, C.off, P.rowptr.p, P.col.p, P.val.p, k->pcTranspose ? C.aggRow.p : C.agg.p, E.p, k->pcTranspose ? 1 : 0,
                    (C.off < k->shiftEnd && !(C.off >= k->shiftExLo && C.off < k->shiftExHi)) ? k->pcDiagScale : 1.0, s->stream);
    if (C.global) {
        DAS_CHECK(!k->pcTranspose, DAS_ERR_ARG, "global coarse space: adjoint preconditioner only");
        rank_allreduce(s, E.p, naggG * naggG, s->stream);
    }
    // E^-1 on the device (Gauss-Jordan, partial pivoting)
    {
        if (C.Einv.n < (size_t)naggG * naggG) C.Einv.alloc((size_t)naggG * naggG);
        DevBuf<int> sing(1);
        if (coarse_invert(naggG, E.p, C.Einv.p, sing.p, s->stream)) return;  // singular coarse operator: no coarse correction
    }
    C.t.alloc(naggG); C.u.alloc(naggG);
    C.active = true;
}

// coarse space of the two-level preconditioner (amd.pcCoarseAggregates: 0 = off, -1 = automatic): RCB aggregates of the owned
// cells, E = Z^T P Z on the entries of the scalar cell field amd.pcCoarseField ("p") of jacPCMat
static void setup_coarse(das_solver* s, das_ksp* k) {
    das_ksp::CoarsePC& C = k->coarse;
    C.active = false;
    long long want = s->opt.geti("amd.pcCoarseAggregates");
    if (want == 0) return;
    const std::string field = s->opt.gets("amd.pcCoarseField");
    const StateDef* sd = nullptr;
    for (const StateDef& q : s->st_full.states) if (q.name == field && q.kind == KIND_SCL) sd = &q;
    if (!sd) return;  // no such field in this solver (e.g. DAScalarTransportFoam has no p)
    const Mesh& m = s->mesh;
    const long long N = m.nC;
    std::vector<int> owned;
    owned.reserve(N);
    for (long long c = 0; c < N; c++) if (s->owned.empty() || s->owned[sd->offset + c]) owned.push_back((int)c);
    if (owned.size() < 64) return;
    if (want < 0) want = std::min<long long>(1024, std::max<long long>(16, (long long)owned.size() / 2048));
    int nagg = (int)std::min<long long>(want, std::min<long long>(2048, (long long)owned.size() / 4));
    if (nagg < 2) return;
    std::vector<int> agg(N, -1);
    const bool byStrength = s->opt.gets("amd.pcCoarseAggregation") == "strength";
    DAS_CHECK(byStrength || s->opt.gets("amd.pcCoarseAggregation") == "rcb", DAS_ERR_ARG, "amd.pcCoarseAggregation: rcb | strength");
    if (byStrength) {
        // aggregates along the strongest pressure-Laplacian couplings (das_mesh.cpp): at most nagg of them
        std::vector<unsigned char> mask;
        if (!s->owned.empty()) { mask.resize(N); for (long long c = 0; c < N; c++) mask[c] = s->owned[sd->offset + c]; }
        nagg = strength_aggregates(m, s->owned.empty() ? nullptr : &mask, nagg, agg);
        if (nagg < 2) return;
    } else {
        // recursive coordinate bisection into nagg parts of (almost) equal size
        rcb_parts(owned, [&](int c, int d) { return m.cg[c].C[d]; }, nagg, agg);
    }
    std::vector<long long> aptr;
    std::vector<int> cells;
    coarse_sort_cells(N, nagg, agg.data(), aptr, cells);
    C.nagg = nagg; C.off = sd->offset; C.N = N; C.h_agg = agg;
    C.cells.upload(cells); C.aptr.upload(aptr);
    C.deflated = s->opt.gets("amd.pcCoarseMode") == "deflated";
    if (C.deflated) { C.c.alloc(s->n); C.rr.alloc(s->n); }
    // per-rank coarse operator (replaced by das_ksp_set_global_coarse when the ranks agree on one global coarse space)
    coarse_build_operator(s, k, nagg, 0, agg);
    if (C.active && s->opt.geti("debug")) fprintf(stderr, "[dafoam_amd] coarse space: %d aggregates on field %s (%s)\n", nagg, field.c_str(), C.deflated ? "deflated" : "additive");
}
// u = E^-1 Z^T r  (global coarse space: the restricted residual of every rank lands in its own slots, one small all-reduce)
static void coarse_solve(das_solver* s, das_ksp* k, const double* r) {
    das_ksp::CoarsePC& C = k->coarse;
    if (C.global) DAS_HIP(hipMemsetAsync(C.t.p, 0, (size_t)C.naggG * sizeof(double), s->stream));
    coarse_restrict_solve(C.nagg, C.aptr.p, C.cells.p, C.off, r, C.naggG, C.aggOff, C.Einv.p, C.t.p, C.u.p, s->stream,
                          [&] { if (C.global) rank_allreduce(s, C.t.p, C.naggG, s->stream); });
}

static void pc_apply(das_solver* s, das_ksp* k, const double* b, double* x) {
    hipEvent_t ev = nullptr;
    s->timer.begin("pc", s->stream, ev);
    if (k->useBilu) {
        if (k->rasOverlap) {
            // restricted additive Schwarz (reference: PCASM, overlap asmOverlap, PC_ASM_RESTRICT): the sub-domain solve sees the vector on
            // owned + overlap unknowns (overlap entries gathered from their owner ranks), only the owned part of its result is kept
            DAS_HIP(hipMemcpyAsync(k->pcin.p, b, (size_t)s->n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
            s->halo.gather_overlap(k->pcin.p, s->stream);
            bilu_apply(k->bilu, k->pcin.p, x, s->stream);
            s->halo.zero_overlap(x, s->stream);
        } else {
            bilu_apply(k->bilu, b, x, s->stream);
        }
        s->timer.end("pc", s->stream, ev);
        return;
    }
    const int mlv = k->pc.maxLevels;
    const size_t lvlBytes = (size_t)((mlv + 2 * PC_PF + 4) >> 1) * sizeof(double);
    if (k->pc.useLDS)
        hipLaunchKernelGGL(k_ras_apply<true>, dim3(k->pc.nBlocks), dim3(PC_THREADS), lvlBytes + (size_t)k->pc.maxLocal * sizeof(double), s->stream,
                           k->pc.view, b, x, mlv);
    else
        hipLaunchKernelGGL(k_ras_apply<false>, dim3(k->pc.nBlocks), dim3(PC_THREADS), lvlBytes, s->stream, k->pc.view, b, x, mlv);
    s->timer.end("pc", s->stream, ev);
}

// ---- restarted right-preconditioned GMRES on the device (reference DALinearEqn.C:28-339 settings) -----------------
// Orthogonalisation: classical Gram-Schmidt, fused multi-dot (one pass over the basis), refined by a second pass if
// needed (the reference uses KSP_GMRES_CGS_REFINE_IFNEEDED, DALinearEqn.C:160), or modified Gram-Schmidt when
// adjEqnOption.useMGSO is set (DALinearEqn.C:162-167).  Givens rotations on the host.  The solve is a small state
// machine (begin / step / end) so that a caller can advance it a given number of iterations (bench.py times a window of
// iterations deep inside a cycle).
// polyD > 0 (amd.polyDegree applies to this solve): gmresMaxIters bounds operator products, a column holds polyD of them - never more
// basis than min(gmresRestart, ceil(maxIters / polyD) + polyD) columns, and no address range beyond it
static void gmres_ws(das_solver* s, das_ksp* k, int polyD = 0) {
    const long long n = s->n;
    long long restart = std::min<long long>(s->opt.geti("adjEqnOption.gmresRestart"), s->opt.geti("adjEqnOption.gmresMaxIters"));
    k->polyD = polyD;
    if (polyD > 0) restart = std::min<long long>(s->opt.geti("adjEqnOption.gmresRestart"), (std::max<long long>(s->opt.geti("adjEqnOption.gmresMaxIters"), 1) + polyD - 1) / polyD + polyD);
    const long long budget = s->opt.geti_or("amd.maxKrylovBytes", (long long)(32.0 * 1024 * 1024 * 1024));
    const long long nr = (n + 3) / 4 * 4;  // fp64 elements a basis vector occupies at most (float storage pads its rows to a multiple of 4: basis_ld)
    const long long maxVec = std::max<long long>(3, budget / (8 * nr));  // vectors the budget holds (restart + 2 of them are needed)
    restart = std::max<long long>(1, std::min<long long>(restart, maxVec - 2));
    // the basis: address range for the larger of this restart and what the reference's default restart (1000) would need inside
    // the budget - reserved ONCE, so that a later solve with another restart never frees and re-allocates it; physical memory is
    // mapped while the iteration advances (VmBuf::ensure in gmres_map_basis)
    long long wantVec = std::max<long long>(restart + 2, std::min<long long>(maxVec, 1002));
    // the over-reservation is free only on the virtual-memory path (>= 4 GB, VmBuf::reserve); below that the range is one hipMalloc of
    // real memory: then exactly what this restart needs (~2.8 GB per KSP on small cases otherwise)
    if ((size_t)wantVec * (size_t)nr * sizeof(double) < ((size_t)4 << 30) || getenv("DAS_NO_VMM") || polyD > 0) wantVec = restart + 2;
    if (k->V.n < (size_t)((restart + 2) * nr) || k->Vn != n) {
        k->V.reserve((size_t)(wantVec * nr));  // (sized for fp64 vectors whatever the storage type of this solve: switching needs no new range)
        k->Vn = n;
    }
    {   // storage type of the basis.  "auto" (default): split (hi + lo floats) for the delayed re-orthogonalisation when the basis is >= 1 GB,
        // else fp64; the tolerance does not enter (split storage keeps 48 mantissa bits per entry: the parity tests solve to 1e-10 .. 1e-12
        // with it); always fp64 for modified Gram-Schmidt, deflated restarting and the Newton primal's inner solves
        const std::string prec = s->opt.gets_or("amd.krylovBasisPrecision", "auto");
        DAS_CHECK(prec == "auto" || prec == "fp64" || prec == "fp32" || prec == "split", DAS_ERR_ARG, "amd.krylovBasisPrecision: auto | fp64 | split | fp32");
        const bool eligible = s->opt.geti("adjEqnOption.useMGSO") == 0 && !s->fwd.on;
        // "fp32" storage alone (round 5, measured on the 2 M-cell wing, profiles/r06c_*): the recurrence follows the fp64 run to four
        // digits for 900 iterations, but the recomputed true residual of the closing cycle is 2.5e-4 |r0| instead of 5e-7 - the rounding of
        // every stored vector violates the Arnoldi relation by eps32 |h_{j+1,j} y_j|, and the plateau of this adjoint makes |y| ~ 1e3-1e4.
        // It stays an explicit option for short, well-conditioned solves.  (A bf16 COPY for the inner products, second attempt,
        // profiles/r06d_*, r06e_*: the preconditioned operator is close to the identity on the Krylov vectors, so the first projection
        // must be accurate relative to a remainder of a few per cent of the vector - 2e-3 errors of the coefficients trip the
        // lost-orthogonality safeguard at the third step and the solve falls back to the four-pass scheme.)  What works is "split":
        // hi + lo floats, inner products on hi (fp32-accurate coefficients), everything else on hi + lo.
        // "auto" = split for the delayed re-orthogonalisation when the basis is >= 1 GB (the Gram-Schmidt passes then dominate), else fp64.
        const bool dcgs2 = s->opt.gets("amd.gmresOrthogonalization") == "dcgs2" && s->opt.geti("adjEqnOption.useMGSO") == 0;
        bool big = (size_t)(restart + 2) * (size_t)n * 8 >= ((size_t)1 << 30);
        // several ranks: n (owned + ghost rows) differs from rank to rank, but the storage type fixes the recurrence target (recTarget)
        // every rank compares the SAME all-reduced residual with - the ranks must agree on it or they disagree on closing a cycle
        // (ADVICE round 5): split everywhere as soon as one rank's basis is that large
        big = rank_any(s, big);
        k->split = eligible && (prec == "split" || (prec == "auto" && dcgs2 && big));
        k->vf32 = k->split || (eligible && prec == "fp32");
        if (k->vf32 && k->ustage.n != (size_t)n) k->ustage.alloc(n);
    }
    if (k->restart != restart || k->w.n != (size_t)n) {
        k->restart = (int)restart;
        k->w.alloc(n); k->z.alloc(n); k->r.alloc(n); k->xdev.alloc(n); k->bdev.alloc(n);
        k->z.zero();  // multi-GPU: ghost entries are never written by the PC and must stay zero
        k->partial.alloc(std::max<size_t>(multidot_partial_size(n, (int)restart + 1), multidot2_partial_size(n, (int)restart + 2)));
        k->hdev.alloc(4 * (restart + 3));
    }
}
// distance between consecutive basis vectors in elements of the storage type (split: hi and lo floats of a vector are adjacent)
// float storage: the rows of a vector are padded to a multiple of 4 (n4), so that every slot and every lo half starts 16-byte aligned
// and the 16-byte-load kernels always apply (orth_wide_ok); nothing reads or relies on the padding
static inline long long basis_n4(das_solver* s) { return (s->n + 3) / 4 * 4; }
static inline long long basis_ld(das_solver* s, das_ksp* k) { return k->split ? 2 * basis_n4(s) : (k->vf32 ? basis_n4(s) : s->n); }
// basis slots [0, nvec) are about to be written / read: map them (a no-op once mapped; milliseconds per new 2 GB chunk)
// the helper thread of the buffer maps 64 vectors ahead of the iteration; the solver waits only if it catches up
// false: the device cannot hold that many vectors (gmres_advance then closes the cycle: the mapped part is the restart length)
static inline bool gmres_map_basis(das_solver* s, das_ksp* k, long long nvec) {
    const long long per = basis_ld(s, k) / (k->vf32 ? 2 : 1);  // fp64 elements of the range one basis vector occupies
    // (amd.polyDegree: nothing is mapped beyond the column bound of gmres_ws, also in a range an earlier solve reserved)
    const long long ahead = k->polyD > 0 ? std::min<long long>(nvec + 64, (long long)k->restart + 2) : nvec + 64;
    k->V.request((size_t)(ahead * per));
    return k->V.try_ensure((size_t)(nvec * per));
}
// slot j of the basis in its storage type
template <class VT>
static inline VT* basis_slot(das_solver* s, das_ksp* k, long long j) { return reinterpret_cast<VT*>(k->V.p) + j * basis_ld(s, k); }
// the lo half of slot j (split storage), or null
static inline float* basis_lo(das_solver* s, das_ksp* k, long long j) { return k->split ? reinterpret_cast<float*>(k->V.p) + j * basis_ld(s, k) + basis_n4(s) : nullptr; }

// dev_out[0..m) = V^T w (V = m vectors of stride n starting at Vbase), dev_out[m] = w.w; summed over the ranks
template <class VT>
static void multidot_dev(das_solver* s, das_ksp* k, const VT* Vbase, int m, const double* w, double* dev_out) {
    launch_multidot<VT>(s->stream, s->n, m, Vbase, basis_ld(s, k), w, k->partial.p, dev_out);
    rank_allreduce(s, dev_out, m + 1, s->stream);
}
// h[0..m) = V^T w, h[m] = w.w  (device result in k->hdev, copied to host)
template <class VT = double>
static void multidot(das_solver* s, das_ksp* k, int m, const double* w, double* h_host) {
    multidot_dev<VT>(s, k, basis_slot<VT>(s, k, 0), m, w, k->hdev.p);
    DAS_HIP(hipMemcpyAsync(h_host, k->hdev.p, (m + 1) * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
}

static void apply_operator(das_solver* s, const double* x, double* y);

// deflated coarse mode: is the sparse A Z of the CURRENT operator available?  Built on first use per operator (two passes over the
// assembled CSR, one thread per row: tens of milliseconds once, against one operator product saved in every iteration); only for the
// single-rank assembled operator - several ranks (ghost rows + halo reduction), the matrix-free forward-mode operator and the Newton
// primal's shifted operator keep the full product.  amd.pcCoarseSparseAZ 0 switches it off.
static bool coarse_az_ready(das_solver* s, das_ksp* k) {
    das_ksp::CoarsePC& C = k->coarse;
    if (!s->op || s->fwd.on) return false;
    if (s->opt.geti_or("amd.pcCoarseSparseAZ", 1) == 0) return false;
    const Mat& A = s->op->m;
    // keyed on the operator's id, not its address: solveAdjoint destroys and re-creates the operator per solve and the allocator may hand
    // back the same address
    if (C.azOpId == s->opId && C.azEpoch == s->op_epoch) return C.azReady;
    C.azOpId = s->opId; C.azEpoch = s->op_epoch; C.azReady = false; C.azFailed = false;
    const long long n = s->n;
    hipStream_t st = s->stream;
    DevBuf<int> cnt(n);
    // (several ranks: all of them take the same path - the fallback is a collective operator product)
    const bool built = coarse_az_build(n, A.rowptr.p, A.col.p, A.val.p, C.N, C.off, C.agg.p, cnt, C.azPtr, C.azAgg, C.azVal, C.azNnz, st,
                                       [&](int ovfAny) { return rank_any(s, ovfAny != 0) ? 1 : 0; });
    if (!built) {
        C.azFailed = true;
        fprintf(stderr, "[dafoam_amd] deflated coarse mode: a row of the operator touches more than %d aggregates - keeping the full operator product per apply\n", AZ_CAP);
        return false;
    }
    if (s->opt.geti("debug")) fprintf(stderr, "[dafoam_amd] deflated coarse mode: sparse A Z with %lld entries (%.2f per row)\n", C.azNnz, (double)C.azNnz / (double)n);
    C.azReady = true;
    return true;
}

// z = M^{-1} v: the factorisation, wrapped in globalPCIters x localPCIters Richardson sweeps on jacPCMat when the
// options ask for more than one (reference DALinearEqn.C:173-205, 237-260: KSPRICHARDSON around ASM and around the
// sub-domain ILU; with one sub-domain per GPU both iterate the same stationary scheme, so l x g sweeps in total)
static long long pc_sweeps(das_solver* s) { return std::max<long long>(1, s->opt.geti("adjEqnOption.globalPCIters")) * std::max<long long>(1, s->opt.geti("adjEqnOption.localPCIters")); }
static void pc_apply_full(das_solver* s, das_ksp* k, const double* v, double* z) {
    const long long sweeps = pc_sweeps(s);
    const long long n = s->n;
    das_ksp::CoarsePC& C = k->coarse;
    if (C.active) {
        hipEvent_t ev = nullptr;
        s->timer.begin("coarse", s->stream, ev);
        coarse_solve(s, k, v);
        if (C.deflated && (s->op || s->fwd.on)) {
            // A-DEF1: z = ILU^-1 (v - A c) + c,  c = Z E^-1 Z^T v
            hipLaunchKernelGGL(k_coarse_prolong, dim3(nblk(n, 256)), dim3(256), 0, s->stream, C.N, n, C.off, C.agg.p, C.u.p, C.c.p, 1);
            if (coarse_az_ready(s, k)) {
                // A c = (A Z) u with the precomputed sparse A Z: ~1.2 entries per row instead of the whole operator
                if (s->halo.active || s->halo_cb) {
                    // several ranks: (A_ext Z) u on all extended rows, the ghost rows reduced to their owners like an operator product
                    hipLaunchKernelGGL(k_az_apply, dim3(nblk(n, 256)), dim3(256), 0, s->stream, n, C.azPtr.p, C.azAgg.p, C.azVal.p, C.u.p, (const double*)nullptr, C.rr.p);
                    if (s->halo.active) s->halo.reduce_vector(C.rr.p, s->stream);
                    else s->halo_cb(C.rr.p, s->comm_user);
                    axpby(s, 1.0, v, -1.0, C.rr.p);
                } else {
                    hipLaunchKernelGGL(k_az_apply, dim3(nblk(n, 256)), dim3(256), 0, s->stream, n, C.azPtr.p, C.azAgg.p, C.azVal.p, C.u.p, v, C.rr.p);
                }
                s->timer.end("coarse", s->stream, ev);
            } else {
                s->timer.end("coarse", s->stream, ev);
                apply_operator(s, C.c.p, C.rr.p);
                axpby(s, 1.0, v, -1.0, C.rr.p);
            }
            pc_apply(s, k, C.rr.p, z);
            axpby(s, 1.0, C.c.p, 1.0, z);
        } else {
            s->timer.end("coarse", s->stream, ev);
            pc_apply(s, k, v, z);
            hipLaunchKernelGGL(k_coarse_prolong, dim3(nblk(n, 256)), dim3(256), 0, s->stream, C.N, n, C.off, C.agg.p, C.u.p, z, 0);
        }
    } else {
        pc_apply(s, k, v, z);
    }
    if (sweeps <= 1) return;
    if (k->rich_r.n != (size_t)n) { k->rich_r.alloc(n); k->rich_d.alloc(n); k->rich_d.zero(); }
    const Mat& P = k->pcmat->m;
    for (long long it = 1; it < sweeps; it++) {
        hipLaunchKernelGGL(k_spmv_wave, SPMV_GRID(P.n), dim3(256), 0, s->stream, P.n, P.rowptr.p, P.col.p, P.val.p, z, k->rich_r.p);
        axpby(s, 1.0, v, -1.0, k->rich_r.p);  // r = v - P z
        pc_apply(s, k, k->rich_r.p, k->rich_d.p);
        axpby(s, 1.0, k->rich_d.p, 1.0, z);
    }
}

// Z[:, r] = M^{-1} V[:, r] for sv columns (column-major, leading dimension n).  The node-block sweeps take all columns at once
// (bilu_apply_multi: tickets, row extents, factor blocks and dependency polls shared by the systems; the factor is streamed once
// per group of 4); the coarse correction stays per column (0.14 ms each).  Richardson sweeps / the deflated coarse form / the
// round-1 RAS preconditioner fall back to the column loop.
static void pc_apply_block(das_solver* s, das_ksp* k, const double* V, double* Z, int sv) {
    const long long n = s->n;
    const long long sweeps = pc_sweeps(s);
    das_ksp::CoarsePC& C = k->coarse;
    const bool batched = k->useBilu && sweeps <= 1 && !(C.active && C.deflated) && sv > 1 && s->opt.geti("amd.blockBatchedPC") != 0;
    if (!batched) {
        for (int r = 0; r < sv; r++) pc_apply_full(s, k, V + (size_t)r * n, Z + (size_t)r * n);
        return;
    }
    hipEvent_t ev = nullptr;
    s->timer.begin("pc", s->stream, ev);
    bilu_apply_multi(k->bilu, V, Z, n, sv, s->stream);
    s->timer.end("pc", s->stream, ev);
    if (C.active)
        for (int r = 0; r < sv; r++) {
            coarse_solve(s, k, V + (size_t)r * n);
            hipLaunchKernelGGL(k_coarse_prolong, dim3(nblk(n, 256)), dim3(256), 0, s->stream, C.N, n, C.off, C.agg.p, C.u.p, Z + (size_t)r * n, 0);
        }
}

// y = (Krylov operator) x: the assembled dRdW^T (adjoint), or - Newton primal - (dR/dW S + D/tau) x by ONE forward-mode pass
static void apply_operator(das_solver* s, const double* x, double* y) {
    if (!s->fwd.on) { spmv(s, s->op->m, x, y); return; }
    const long long n = s->n;
    const int B = 256;
    hipStream_t st = s->stream;
    hipEvent_t ev = nullptr;
    s->timer.begin("jvp", st, ev);
    ResParams prm = make_params(s->cp, s->opt, 0);
    if (s->d_Wd.n != (size_t)n) { s->d_Wd.alloc(n); s->d_Rd.alloc(n); }
    hipLaunchKernelGGL(k_seed_dir, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_W.p, s->d_scale.p, x, s->d_Wd.p);
    eval_residual<Dual<1>>(s->dm, s->cp, prm, s->d_Wd.p, s->d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
    hipLaunchKernelGGL(k_tangent_out, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_Rd.p, y);
    if (s->fwd.invTau != 0.0) hipLaunchKernelGGL(k_add_diag_prod, dim3(nblk(n, B)), dim3(B), 0, st, n, s->fwd.invTau, s->fwd.diag.p, x, y);
    s->timer.end("jvp", st, ev);
}

struct GmresRun {
    bool open = false;        // inside an Arnoldi cycle
    bool fixed = false;       // no convergence exit (bench)
    int m = 0, j = 0;
    bool memWarned = false;
    long long its = 0, maxIts = 0;
    double beta = 0, target = 0, rtol = 0, atol = 0, t0 = 0;
    double recTarget = 0;     // what the RECURRENCE residual is driven to: the target (fp64 basis), 0.98 x the target with the split basis
                              // (Arnoldi relation to 2^-48: a margin for the recomputed true residual), half of it with the fp32 basis,
                              // whose recurrence tracks the true residual only to ~1e-7 |r0| - so that the recomputed TRUE residual of
                              // the closing cycle lands below the target instead of opening another cycle (and another plateau)
    const double* d_rhs = nullptr;
    double* d_x = nullptr;
    std::vector<double> H, cs, sn, g, hh, h2, y;
    // delayed re-orthogonalisation (gmres_iter_dcgs2)
    bool dcgs2 = false;
    int pend = 0;                 // slot of the pending (once projected, not normalised) vector = number of final basis vectors
    std::vector<double> Hraw, h1; // unrotated Hessenberg matrix; first-projection coefficients of the pending vector
    // breakdown / stagnation control (gmres_advance): a cycle closed by a Krylov breakdown, by lost orthogonality or by a
    // recurrence residual the recomputed true residual does not confirm must make progress; two such cycles in a row that
    // do not halve the true residual end the solve (PETSc, which the reference runs - DALinearEqn.C:341-437 - leaves the
    // iteration at a breakdown as well: KSP_CONVERGED_HAPPY_BREAKDOWN / KSP_DIVERGED_BREAKDOWN)
    bool earlyClose = false;      // the open cycle was closed before the basis was full and before maxIts
    bool safeOrth = false;        // after lost orthogonality: the following cycles use the two-pass scheme ("cgs")
    bool stalled = false;
    int nonImproving = 0, nBreakdown = 0;
    double betaStart = 0;         // true residual norm at the start of the open cycle
    // polynomial preconditioning (amd.polyDegree = polyD > 0, das_poly_host.hpp): the first cycle is closed after polyD columns (cap) and
    // gives the polynomial; from then on a column is w = B p(B) v (polyOn).  prods counts operator products - what gmresMaxIters bounds
    // and das_ksp_get_info reports in this mode; its stays the number of Arnoldi columns
    int cap = 0;                  // columns at which the open cycle is closed: m, or polyD for the generating cycle
    int polyD = 0;
    bool polyGen = false, polyTried = false, polyOn = false, budgetOut = false, nonFinite = false;
    long long prods = 0;
};
// the GMRES polynomial of a KSP (amd.polyDegree): ordered roots (a pair once, im > 0), the work vectors of the root walk, and the figures
// of the last solve (das_ksp_get_poly_info)
struct PolyWork {
    long long n = 0;
    DevBuf<double> prod, poly, tmp;  // allocated when the first polynomial is built, never without one
    int nroots = 0;
    double re[POLY_MAX_DEGREE] = {0}, im[POLY_MAX_DEGREE] = {0};
    int degree = 0, nPairs = 0, generated = 0, fallback = 0;
    long long products = 0, columns = 0, genColumns = 0;  // columns: Arnoldi columns after the generating cycle's genColumns
    int work_vectors() const { return prod.n ? 3 : 0; }
};
// amd.polyDegree, validated at every solve: the degree this solve runs with.  Fixed-iteration bench windows and the Newton primal's
// inner solves keep plain GMRES silently; IDR(s), deflated restarting or several ranks on top are errors
static int poly_degree(das_solver* s, bool fixed) {
    const long long d = s->opt.geti("amd.polyDegree");
    DAS_CHECK(d >= 0 && d <= POLY_MAX_DEGREE, DAS_ERR_ARG, "amd.polyDegree " + std::to_string(d) + " is outside 0 .. 16");
    if (d == 0 || fixed || s->fwd.on) return 0;
    DAS_CHECK(s->opt.gets("amd.krylovMethod") != "idrs", DAS_ERR_ARG, "amd.polyDegree > 0 belongs to GMRES: not with amd.krylovMethod \"idrs\"");
    DAS_CHECK(!s->halo.active && !s->halo_cb, DAS_ERR_ARG, "amd.polyDegree > 0 is single-rank (run the sharded solve without it)");
    DAS_CHECK(s->opt.geti_or("amd.gmresDeflation", 0) <= 0, DAS_ERR_ARG, "amd.gmresDeflation > 0 cannot be combined with amd.polyDegree > 0");
    return (int)d;
}
static bool gmres_trace() { static const bool on = [] { const char* e = getenv("DAS_GMRES_TRACE"); return e && *e && *e != '0'; }(); return on; }

static void gmres_true_residual(das_solver* s, das_ksp* k, GmresRun& G, bool haveGuess) {
    const long long n = s->n;
    hipStream_t st = s->stream;
    if (haveGuess) {
        apply_operator(s, G.d_x, k->r.p);
        G.prods++;
        axpby(s, 1.0, G.d_rhs, -1.0, k->r.p);
    } else {
        DAS_HIP(hipMemsetAsync(G.d_x, 0, n * sizeof(double), st));
        DAS_HIP(hipMemcpyAsync(k->r.p, G.d_rhs, n * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    multidot(s, k, 0, k->r.p, G.hh.data());
    G.beta = std::sqrt(G.hh[0]);
}

// what every solve starts with: workspace, a fresh GmresRun with the options read, the true residual of the start vector, the target.
// `deflated`: run_gmres_dr - fp64 basis, no Hessenberg arrays (gmres_dr_loop keeps its own), the cycle lengths are left alone
static GmresRun& gmres_begin(das_solver* s, das_ksp* k, const double* d_rhs, double* d_x, bool fixed, bool deflated = false, int polyD = 0) {
    need_init(s);
    DAS_CHECK(s->op || s->fwd.on, DAS_ERR_STATE, "initializedRdWTMatrixFree() must be called before solveLinearEqn()");
    if (deflated) DAS_CHECK(!s->halo.active && !s->halo_cb, DAS_ERR_ARG, "amd.gmresDeflation is single-rank (the restart's small dense algebra is not replicated across ranks yet)");
    gmres_ws(s, k, polyD);
    if (deflated) { k->vf32 = false; k->split = false; }  // the deflated solver keeps its (short) basis in fp64
    if (k->useBilu) bilu_clear_abort(k->bilu, s->stream);
    if (!k->run) k->run.reset(new GmresRun);
    GmresRun& G = *k->run;
    const int m = k->restart;
    G = GmresRun();
    if (deflated) DAS_CHECK(m >= 4, DAS_ERR_ARG, "amd.gmresDeflation needs gmresRestart >= 4");
    G.m = m; G.fixed = fixed; G.d_rhs = d_rhs; G.d_x = d_x;
    G.cap = m; G.polyD = std::min(polyD, m);  // (a restart shorter than the degree gives a polynomial of the restart's degree)
    if (polyD > 0) {
        if (!k->poly) k->poly.reset(new PolyWork);
        PolyWork& P = *k->poly;
        P.nroots = 0; P.degree = 0; P.nPairs = 0; P.generated = 0; P.fallback = 0; P.products = 0; P.columns = 0; P.genColumns = 0;
    } else if (k->poly && !fixed && !deflated) {
        k->poly.reset();  // a solve without the option: what a KSP that never ran it reports (a bench window leaves the figures alone)
    }
    G.maxIts = s->opt.geti("adjEqnOption.gmresMaxIters");
    G.rtol = s->opt.getd("adjEqnOption.gmresRelTol"); G.atol = s->opt.getd("adjEqnOption.gmresAbsTol");
    G.hh.assign(2 * (m + 2), 0.0); G.h2.assign(2 * (m + 2), 0.0);
    if (!deflated) {
        G.H.assign((size_t)(m + 1) * m, 0.0); G.cs.assign(m, 0.0); G.sn.assign(m, 0.0); G.g.assign(m + 1, 0.0); G.y.assign(m, 0.0);
        const std::string& orth = s->opt.gets("amd.gmresOrthogonalization");
        DAS_CHECK(orth == "dcgs2" || orth == "cgs", DAS_ERR_ARG, "amd.gmresOrthogonalization \"" + orth + "\" is not one of dcgs2 | cgs");
        G.dcgs2 = orth == "dcgs2" && s->opt.geti("adjEqnOption.useMGSO") == 0;
        if (G.dcgs2) { G.Hraw.assign((size_t)(m + 1) * m, 0.0); G.h1.assign(m + 2, 0.0); }
        else if (G.polyD > 0) G.Hraw.assign((size_t)(m + 1) * m, 0.0);  // the generating cycle keeps its unrotated Hessenberg matrix
        k->cycleLens.clear();
    }
    k->nrefine = 0; k->hist.clear();
    G.t0 = wall_seconds();
    gmres_true_residual(s, k, G, s->opt.geti("adjEqnOption.useNonZeroInitGuess") != 0);
    k->res0 = G.beta;
    k->hist.push_back(G.beta);
    G.target = std::max(G.rtol * G.beta, G.atol);
    if (!deflated) G.recTarget = k->split ? 0.98 * G.target : (k->vf32 ? 0.5 * G.target : G.target);
    return G;
}
// reference failure rule (DALinearEqn.C:422-434): 1 = failed, the residual misses BOTH tolerances by more than the factor `diff` (gmresTolDiff)
static int gmres_failed(double res, double res0, double rtol, double atol, double diff) {
    const double absRatio = res / atol, relRatio = res0 > 0 ? res / res0 / rtol : 0.0;
    return (relRatio > diff && absRatio > diff) ? 1 : 0;
}
// what every solve ends with: wait for the stream, then the abort flag of the preconditioner sweeps
static void gmres_finish_check(das_solver* s, das_ksp* k) {
    DAS_HIP(hipStreamSynchronize(s->stream));
    if (k->useBilu) DAS_CHECK(!bilu_aborted(k->bilu, s->stream), DAS_ERR_INTERNAL, "preconditioner sweep timed out (bounded spin)");
}
static void gmres_cycle_start(das_solver* s, das_ksp* k) {
    GmresRun& G = *k->run;
    const long long n = s->n;
    DAS_CHECK(gmres_map_basis(s, k, 3), DAS_ERR_INTERNAL, "GMRES: no device memory for three Krylov vectors (" + k->V.workerError + ")");
    if (k->vf32) launch_scale_to(s->stream, n, 1.0 / G.beta, (const double*)k->r.p, basis_slot<float>(s, k, 0), (const float*)nullptr, basis_lo(s, k, 0));
    else launch_scale_to(s->stream, n, 1.0 / G.beta, (const double*)k->r.p, (double*)k->V.p, (const float*)nullptr, (float*)nullptr);
    std::fill(G.g.begin(), G.g.end(), 0.0);
    G.g[0] = G.beta;
    G.j = 0;
    G.pend = 0;
    G.open = true;
    G.earlyClose = false;
    G.betaStart = G.beta;
    G.polyGen = G.polyD > 0 && !G.polyTried;  // the first cycle of the solve gives the polynomial
    G.polyTried = true;
    G.cap = G.polyGen ? G.polyD : G.m;
}
// the basis vector in slot j as the fp64 input of the preconditioner (fp32 basis: converted into the staging vector)
template <class VT>
static const double* basis_as_double(das_solver* s, das_ksp* k, long long j) {
    if (sizeof(VT) == sizeof(double)) return reinterpret_cast<const double*>(basis_slot<VT>(s, k, j));
    launch_scale_to(s->stream, s->n, 1.0, (const VT*)basis_slot<VT>(s, k, j), (double*)k->ustage.p, (const float*)basis_lo(s, k, j), (float*)nullptr);
    return k->ustage.p;
}
static das_dense_eig_fn g_dense_eig = nullptr;  // das_set_dense_eig_callback: the restart of GMRES-DR and the roots of the GMRES polynomial
// ---- the polynomial apply t = p(B) v on the device: poly_walk of das_poly_host.hpp over the kernels of das_poly.hpp ----------------
// v must be none of k->z, k->w (the scratch of the products) and is not written; the result is P.poly
namespace {
struct PolyDeviceOps {
    das_solver* s; das_ksp* k; PolyWork* P; const double* v;
    void product(bool fromTmp, bool first) {
        pc_apply_full(s, k, fromTmp ? P->tmp.p : (first ? v : P->prod.p), k->z.p);
        apply_operator(s, k->z.p, k->w.p);
    }
    void real_step(bool first, bool last, double th) { launch_poly_real(s->stream, s->n, first, last, th, v, k->w.p, P->poly.p, P->prod.p); }
    void pair_first(bool first, double twoa, double m2) { launch_poly_pair_first(s->stream, s->n, first, twoa, m2, v, P->prod.p, k->w.p, P->poly.p, P->tmp.p); }
    void pair_second(bool first, double m2) { launch_poly_pair_second(s->stream, s->n, first, m2, v, k->w.p, P->prod.p); }
};
}  // namespace
static void poly_apply_device(das_solver* s, das_ksp* k, const double* v) {
    PolyWork& P = *k->poly;
    PolyDeviceOps ops{s, k, &P, v};
    poly_walk(ops, P.nroots, P.re, P.im);
}
// the roots of the generating cycle (j = polyD columns, unrotated Hessenberg matrix in G.Hraw) and the work vectors; no usable roots:
// the solve goes on without a polynomial and reports the fallback
static void poly_generate(das_solver* s, das_ksp* k, int j) {
    GmresRun& G = *k->run;
    PolyWork& P = *k->poly;
    P.nroots = poly_roots_host(g_dense_eig, j, G.Hraw.data(), G.m, P.re, P.im, &P.nPairs);
    if (P.nroots == 0) {
        P.fallback = 1; P.nPairs = 0;
        if (s->opt.geti("debug")) fprintf(stderr, "[dafoam_amd] amd.polyDegree %d: no usable harmonic Ritz values (or no dense eigen-solver callback) - this solve runs without the polynomial\n", j);
        return;
    }
    if (P.n != s->n || !P.prod.n) { P.n = s->n; P.prod.alloc(s->n); P.poly.alloc(s->n); P.tmp.alloc(s->n); }
    P.degree = j; P.generated = 1;
    G.polyOn = true;
}
// the ONE place where the Krylov operator meets the preconditioner: z = M^-1 p(B) v (p = 1 without a polynomial) in k->z, then
// w = A z unless w is null (the closing step of a cycle).  v is none of k->z, k->w.  Counts the operator products
static void gmres_precond_product(das_solver* s, das_ksp* k, const double* v, double* w) {
    GmresRun& G = *k->run;
    const double* t = v;
    if (G.polyOn) {
        poly_apply_device(s, k, v);
        t = k->poly->poly.p;
        G.prods += k->poly->degree - 1;
    }
    pc_apply_full(s, k, t, k->z.p);
    if (w) { apply_operator(s, k->z.p, w); G.prods++; }
}
// one Arnoldi step; returns the recurrence residual norm
template <class VT>
static double gmres_iter_dcgs2(das_solver* s, das_ksp* k);
template <class VT>
static double gmres_iter_t(das_solver* s, das_ksp* k) {
    GmresRun& G = *k->run;
    if (G.dcgs2 && !G.safeOrth) return gmres_iter_dcgs2<VT>(s, k);
    const long long n = s->n;
    const int B = 256, m = G.m, j = G.j;
    hipStream_t st = s->stream;
    const bool alwaysRefine = s->opt.geti("amd.cgsAlwaysRefine") != 0;
    const bool mgs = s->opt.geti("adjEqnOption.useMGSO") != 0;
    std::vector<double>&H = G.H, &hh = G.hh, &h2 = G.h2, &cs = G.cs, &sn = G.sn, &g = G.g;
    VT* const Vb = basis_slot<VT>(s, k, 0);
    const long long ld = basis_ld(s, k);
    gmres_precond_product(s, k, basis_as_double<VT>(s, k, j), k->w.p);
    double hn;
    std::fill(h2.begin(), h2.end(), 0.0);
    if (mgs) {
        // modified Gram-Schmidt: j+1 dependent (dot, axpy) pairs, coefficients stay on the device until the end
        double* hcol = k->hdev.p + (m + 2);
        for (int i = 0; i <= j; i++) {
            multidot_dev<VT>(s, k, Vb + (long long)i * ld, 1, k->w.p, k->hdev.p);
            DAS_HIP(hipMemcpyAsync(hcol + i, k->hdev.p, sizeof(double), hipMemcpyDeviceToDevice, st));
            launch_multiaxpy(st, n, 1, (const VT*)(Vb + (long long)i * ld), ld, (const double*)k->hdev.p, (double*)k->w.p, (const float*)basis_lo(s, k, i));
        }
        multidot_dev<VT>(s, k, Vb, 0, k->w.p, k->hdev.p);
        DAS_HIP(hipMemcpyAsync(hcol + j + 1, k->hdev.p, sizeof(double), hipMemcpyDeviceToDevice, st));
        DAS_HIP(hipMemcpyAsync(hh.data(), hcol, (j + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
        DAS_HIP(hipStreamSynchronize(st));
        hn = std::sqrt(std::max(hh[j + 1], 0.0));
    } else {
        // classical Gram-Schmidt, one fused pass: h = V^T w and w.w; refinement only if needed (reference:
        // KSP_GMRES_CGS_REFINE_IFNEEDED, DALinearEqn.C:160): refine when the projected vector keeps less than half
        // of its squared norm, i.e. ||w - V h||^2 (= w.w - h.h) < h.h
        multidot<VT>(s, k, j + 1, k->w.p, hh.data());
        launch_multiaxpy(st, n, j + 1, (const VT*)Vb, ld, (const double*)k->hdev.p, (double*)k->w.p, (const float*)basis_lo(s, k, 0));
        double hsq = 0.0;
        for (int i = 0; i <= j; i++) hsq += hh[i] * hh[i];
        const double ww = hh[j + 1];
        const double est = ww - hsq;
        if (alwaysRefine || !(est > hsq) || !(est > 0.0)) {
            multidot<VT>(s, k, j + 1, k->w.p, h2.data());
            launch_multiaxpy(st, n, j + 1, (const VT*)Vb, ld, (const double*)k->hdev.p, (double*)k->w.p, (const float*)basis_lo(s, k, 0));
            double hn2;
            multidot<VT>(s, k, 0, k->w.p, &hn2);
            hn = std::sqrt(std::max(hn2, 0.0));
            k->nrefine++;
        } else {
            hn = std::sqrt(est);
        }
    }
    if (!mgs && !(hn > GMRES_BREAKDOWN_TOL * std::sqrt(std::max(hh[j + 1], 0.0)))) { hn = 0.0; G.nBreakdown++; }  // happy breakdown (hh[j+1] = |A M^-1 v_j|^2)
    for (int i = 0; i <= j; i++) H[(size_t)i * m + j] = hh[i] + h2[i];
    H[(size_t)(j + 1) * m + j] = hn;
    if (G.polyGen) for (int i = 0; i <= j + 1; i++) G.Hraw[(size_t)i * m + j] = H[(size_t)i * m + j];
    if (hn > 0.0) launch_scale_to(st, n, 1.0 / hn, (const double*)k->w.p, Vb + (long long)(j + 1) * ld, (const float*)nullptr, basis_lo(s, k, j + 1));
    gmres_rotate_column(H, cs, sn, g, m, j);
    G.its++;
    G.j++;
    const double res = std::fabs(g[G.j]);
    k->hist.push_back(res);
    if (hn == 0.0) { G.j = -G.j; G.earlyClose = true; }  // happy breakdown: close the cycle (sign marks it)
    return res;
}
static double gmres_iter(das_solver* s, das_ksp* k) { return k->vf32 ? gmres_iter_t<float>(s, k) : gmres_iter_t<double>(s, k); }
// One step of GMRES with classical Gram-Schmidt and DELAYED re-orthogonalisation (DCGS2; Bielich, Langou, Thomas,
// Swirydowicz, Yamazaki, Boman, "Low-synch Gram-Schmidt with delayed reorthogonalization for Krylov solvers", 2022).
// The reference's CGS with refinement (DALinearEqn.C:160) reads the basis four times per iteration here (it refines at
// nearly every step: the right-preconditioned operator is close to the identity on the current vector, so the first
// projection removes most of the norm).  DCGS2 produces the same basis with TWO reads: the second projection of the newest
// vector and the first projection of the next Krylov vector share their inner products and their update.
//
// State: Q = [q_0 .. q_{j-1}] final; u (slot j) = B q_{j-1} - Q h1, projected once, not normalised (B = A M^-1).
//   v = B u
//   [s; uu] = [Q u]^T u,  [t; uv] = [Q u]^T v                       one pass over the basis (k_multidot2)
//   alpha^2 = uu - s.s ;  column j-1 of H = [h1 + s ; alpha]         (B q_{j-1} = Q (h1 + s) + alpha q_j)
//   q_j = (u - Q s) / alpha
//   B q_j = (v - B Q s) / alpha = (v - Q (H_jj s) - q_j alpha s_{j-1}) / alpha     (Arnoldi relation for B Q)
//   gamma = q_j.(B q_j) + s_{j-1} = (uv - s.t) / alpha^2
//   u' = B q_j - [Q q_j] h1' = (v - gamma u - Q (t - gamma s)) / alpha,  h1' = [(t - H_jj s) / alpha ; gamma - s_{j-1}]
//   q_j and u' come out of one more pass over the basis (k_dcgs2_update).
// The Hessenberg column (and with it the residual norm) of a step is known one step later; a solve that stops after k
// columns has applied the operator k + 1 times.
template <class VT>
static double gmres_iter_dcgs2(das_solver* s, das_ksp* k) {
    GmresRun& G = *k->run;
    const long long n = s->n;
    const int m = G.m, j = G.pend;
    hipStream_t st = s->stream;
    VT* const Vb = basis_slot<VT>(s, k, 0);
    const long long ld = basis_ld(s, k);
    VT* u = Vb + (long long)j * ld;
    gmres_precond_product(s, k, basis_as_double<VT>(s, k, j), k->w.p);
    const int K = j + 1;
    launch_multidot2<VT>(st, n, K, (const VT*)Vb, ld, (const VT*)u, (const double*)k->w.p, k->partial.p, k->hdev.p);
    rank_allreduce(s, k->hdev.p, 2 * K, st);
    std::vector<double>& o = G.hh;
    DAS_HIP(hipMemcpyAsync(o.data(), k->hdev.p, 2 * K * sizeof(double), hipMemcpyDeviceToHost, st));
    DAS_HIP(hipStreamSynchronize(st));
    const double* sv = o.data();
    const double* tv = o.data() + K;
    const double uu = sv[j], uv = tv[j];
    double ss = 0.0, stt = 0.0;
    for (int i = 0; i < j; i++) { ss += sv[i] * sv[i]; stt += sv[i] * tv[i]; }
    double al2 = uu - ss, num = uv - stt;  // |u - Q s|^2 and (u - Q s).v by Pythagoras - accurate while s is small against u
    // |B q_{j-1}|^2 = |h1|^2 + u.u: the scale the pending vector is measured against (breakdown rule)
    double normBq2 = uu;
    for (int i = 0; i < j; i++) normBq2 += G.h1[i] * G.h1[i];
    bool explicitProj = false;
    if (j > 0 && !(ss <= 1e-2 * uu)) {
        if (gmres_trace()) fprintf(stderr, "[dafoam_amd] dcgs2 step %d: s.s / u.u = %.3e > 1e-2: explicit projection, cycle closes\n", j, ss / uu);
        // the first projection left a large component in span(Q): u is (nearly) rounding noise - the Krylov space is exhausted or
        // orthogonality was lost - and uu - s.s cancels.  Rare; pay one extra pass: c = u - Q s explicitly, then c.c and c.v
        double* dsc = k->hdev.p + 2 * (m + 3);
        DAS_HIP(hipMemcpyAsync(dsc, sv, j * sizeof(double), hipMemcpyHostToDevice, st));
        if (k->split) {
            // u is stored split: project its fp64 value (staging vector) with the hi + lo basis, store it split again
            const double* ud = basis_as_double<VT>(s, k, j);
            launch_multiaxpy(st, n, j, (const VT*)Vb, ld, (const double*)dsc, const_cast<double*>(ud), (const float*)basis_lo(s, k, 0));
            launch_scale_to(st, n, 1.0, ud, u, (const float*)nullptr, basis_lo(s, k, j));
        } else {
            launch_multiaxpy(st, n, j, (const VT*)Vb, ld, (const double*)dsc, u, (const float*)nullptr);
        }
        launch_multidot2<VT>(st, n, 1, (const VT*)u, ld, (const VT*)u, (const double*)k->w.p, k->partial.p, k->hdev.p);  // K = 1: the leading dimension is not used
        rank_allreduce(s, k->hdev.p, 2, st);
        double cc[2] = {0.0, 0.0};
        DAS_HIP(hipMemcpyAsync(cc, k->hdev.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
        DAS_HIP(hipStreamSynchronize(st));
        al2 = cc[0]; num = cc[1];
        explicitProj = true;
        k->nrefine++;
    }
    // happy breakdown: what is left of B q_{j-1} after the projections is rounding noise (GMRES_BREAKDOWN_TOL).  The column
    // is completed with a ZERO sub-diagonal - the recurrence residual drops to zero - and the cycle is closed; whether the
    // solve is over is decided on the recomputed true residual (gmres_advance)
    if (G.polyD > 0 && !std::isfinite(al2)) { G.nonFinite = true; return al2; }  // (gmres_advance ends the solve: reason 3)
    const bool breakdown = !(al2 > GMRES_BREAKDOWN_TOL * GMRES_BREAKDOWN_TOL * normBq2);
    const double al = breakdown ? 0.0 : std::sqrt(al2);
    double res = k->hist.back();
    if (j == 0) {
        DAS_CHECK(!breakdown, DAS_ERR_INTERNAL, "GMRES: the start vector of an Arnoldi cycle is not finite (preconditioner or operator returned NaN)");
        G.g[0] = G.beta * al;  // slot 0 holds r / beta, alpha = 1 up to rounding
    } else {
        const int col = j - 1;
        for (int i = 0; i < j; i++) G.Hraw[(size_t)i * m + col] = G.H[(size_t)i * m + col] = G.h1[i] + (breakdown ? 0.0 : sv[i]);
        G.Hraw[(size_t)j * m + col] = G.H[(size_t)j * m + col] = al;
        res = gmres_rotate_column(G.H, G.cs, G.sn, G.g, m, col);
        G.its++;
        G.j = j;
        k->hist.push_back(res);
        // happy breakdown, or the explicit projection above (orthogonality lost: the lagged recurrence below would divide by
        // a small alpha and multiply the rounding errors of s): close the cycle (sign marks it), restart from the true
        // residual; the cycles after lost orthogonality run the two-pass scheme
        if (breakdown || explicitProj) {
            if (breakdown) G.nBreakdown++; else G.safeOrth = true;
            G.j = -G.j; G.earlyClose = true;
            return res;
        }
        const bool stop = !G.fixed && (res <= G.recTarget || G.its >= G.maxIts);
        if (stop || G.j >= G.cap) return res;        // the cycle is closed by the caller: no further basis vector needed
    }
    const double gam = num / al2;
    // coefficients of the fused update: s, then c = t - gamma s
    std::vector<double>& co = G.h2;
    for (int i = 0; i < j; i++) { co[i] = sv[i]; co[j + i] = tv[i] - gam * sv[i]; }
    double* dco = k->hdev.p + 2 * (m + 3);
    if (j > 0) DAS_HIP(hipMemcpyAsync(dco, co.data(), 2 * j * sizeof(double), hipMemcpyHostToDevice, st));
    launch_dcgs2_update<DCGS2_UNROLL, DCGS2_RPT, VT>(st, n, j, Vb, ld, (const double*)dco, gam, 1.0 / al, (const double*)k->w.p, basis_lo(s, k, 0));
    // first-projection coefficients of the new pending vector: (t - H_jj s) / alpha, gamma - s_{j-1}
    for (int i = 0; i < j; i++) {
        double a = tv[i];
        for (int q = std::max(0, i - 1); q < j; q++) a -= G.Hraw[(size_t)i * m + q] * sv[q];
        G.h1[i] = a / al;
    }
    G.h1[j] = gam - (j > 0 ? sv[j - 1] : 0.0);
    G.pend = j + 1;
    return res;
}
// back substitution, x += M^{-1} (V y), true residual
template <class VT>
static void gmres_cycle_end_t(das_solver* s, das_ksp* k) {
    GmresRun& G = *k->run;
    const long long n = s->n;
    const int B = 256, m = G.m, j = std::abs(G.j);
    hipStream_t st = s->stream;
    back_substitute(j, G.H.data(), m, 1, 1, G.g.data(), G.y.data());
    DAS_HIP(hipMemcpyAsync(k->hdev.p, G.y.data(), j * sizeof(double), hipMemcpyHostToDevice, st));
    // V y: into k->w, or - the polynomial's products use k->w - into k->r, which the true residual below rewrites anyway
    double* const vy = G.polyOn ? k->r.p : k->w.p;
    launch_lincomb(st, n, j, (const VT*)basis_slot<VT>(s, k, 0), basis_ld(s, k), (const double*)k->hdev.p, vy, (const float*)basis_lo(s, k, 0));
    gmres_precond_product(s, k, vy, nullptr);
    axpby(s, 1.0, k->z.p, 1.0, G.d_x);
    const double recRes = k->hist.back();
    gmres_true_residual(s, k, G, true);
    if (G.polyGen) {  // the generating cycle: a polynomial only from a cycle that ran its polyD columns without a breakdown
        if (j == G.polyD && !G.earlyClose) poly_generate(s, k, j);
        G.polyGen = false;
    }
    k->hist.back() = G.beta;
    k->cycleLens.push_back(j);
    G.open = false;
    if (gmres_trace()) {
        double ymax = 0.0;
        for (int i = 0; i < j; i++) ymax = std::max(ymax, std::fabs(G.y[i]));
        fprintf(stderr, "[dafoam_amd] GMRES cycle closed after %d columns (its %lld): recurrence |r| %.6e, true |r| %.6e (|r0| %.3e), max |y| %.3e, explicit projections %d, basis %s%s\n",
                j, G.its, recRes, G.beta, k->res0, ymax, k->nrefine, k->split ? "split" : (k->vf32 ? "fp32" : "fp64"), G.safeOrth ? ", two-pass scheme from here" : "");
    }
}
static void gmres_cycle_end(das_solver* s, das_ksp* k) {
    if (k->vf32) gmres_cycle_end_t<float>(s, k); else gmres_cycle_end_t<double>(s, k);
}
// advance by up to `nsteps` iterations (cycles are opened / closed as needed); returns true when the solve is over
static bool gmres_over(const GmresRun& G) { return !G.fixed && !G.open && (G.beta <= G.target || G.its >= G.maxIts || G.stalled || G.budgetOut || G.nonFinite); }
static bool gmres_advance(das_solver* s, das_ksp* k, long long nsteps) {
    GmresRun& G = *k->run;
    for (long long t = 0; t < nsteps; t++) {
        if (gmres_over(G)) return true;
        if (G.beta == 0.0) return true;
        if (G.polyD > 0) {
            // gmresMaxIters bounds operator products: a column (polyD of them once the polynomial is there) is started only if the budget
            // also covers closing its cycle (the polynomial in x += M^-1 p(B) V y, and the true residual); the delayed scheme completes the
            // first column of a cycle with its second product
            const long long per = G.polyOn ? k->poly->degree : 1, closing = per;
            const bool lagged = G.dcgs2 && !G.safeOrth;
            if (G.prods + (!G.open && lagged ? 2 : 1) * per + closing > G.maxIts) {
                if (G.open) gmres_cycle_end(s, k);
                G.budgetOut = true;
                return true;
            }
        }
        if (!G.open) gmres_cycle_start(s, k);
        // the step writes basis slots up to (pending vector) + 2: map them; if the device has no memory left for them the cycle
        // ends here - the mapped part of the basis is the restart length from now on
        // (a cycle of m columns holds m + 1 basis vectors - with the delayed scheme the pending vector of the last step sits in slot
        // m and nothing is written behind it - so the request never exceeds the restart + 2 slots gmres_ws reserved: round 4 asked
        // for pend + 3 = restart + 3 at the last step of a cycle and closed every malloc-path cycle one column early)
        const long long wantSlots = std::min<long long>(((G.dcgs2 && !G.safeOrth) ? G.pend : G.j) + 3, (long long)G.cap + 2);
        if (!gmres_map_basis(s, k, wantSlots)) {
            if (k->V.workerError.empty())
                k->V.workerError = "request for " + std::to_string(wantSlots) + " basis vectors beyond the reserved range of " + std::to_string(k->V.n / (size_t)std::max<long long>(1, s->n)) + " (internal)";
            DAS_CHECK(G.j >= 1, DAS_ERR_INTERNAL, "GMRES: the Krylov basis cannot grow beyond its first vectors (" + k->V.workerError + ")");
            if (!G.memWarned) fprintf(stderr, "[dafoam_amd] GMRES restarts after %d vectors: %s\n", G.j, k->V.workerError.c_str());
            G.memWarned = true;
            gmres_cycle_end(s, k);
            t--;  // no iteration was done in this pass of the loop
            continue;
        }
        const double res = gmres_iter(s, k);
        if (G.polyD > 0 && (G.nonFinite || !std::isfinite(res))) {
            // a non-finite value out of the operator, the preconditioner or the polynomial: x keeps the last closed cycle's update
            if (G.nonFinite) k->hist.push_back(res);  // (the step returned before it recorded anything)
            G.nonFinite = true; G.open = false;
            return true;
        }
        const bool stop = !G.fixed && (res <= G.recTarget || G.its >= G.maxIts);
        if (G.j < 0 || G.j >= G.cap || stop) {
            // a cycle that ends on a breakdown / lost orthogonality, or on a recurrence residual below the target, should
            // leave a TRUE residual below the target.  If it does not, the next cycle works on the rounding level of this
            // system; it may still gain (iterative refinement), but two such cycles in a row that do not halve the true
            // residual mean the attainable accuracy is reached: stop instead of spending gmresMaxIters on one-step cycles
            const bool judged = G.earlyClose || (res <= G.recTarget && G.its < G.maxIts);
            gmres_cycle_end(s, k);
            if (!G.fixed && judged && G.beta > G.target) {
                if (G.beta < 0.5 * G.betaStart) G.nonImproving = 0;
                else if (++G.nonImproving >= 2) G.stalled = true;
            }
        }
    }
    return gmres_over(G);
}
static int gmres_end(das_solver* s, das_ksp* k) {
    GmresRun& G = *k->run;
    if (G.open) gmres_cycle_end(s, k);
    gmres_finish_check(s, k);
    k->iters = (int)(G.polyD > 0 ? G.prods : G.its);
    k->nBreakdown = G.nBreakdown;
    k->res = k->hist.back();
    k->reason = G.nonFinite ? 3 : (G.beta <= G.target ? 0 : (G.stalled ? 2 : 1));
    k->seconds = wall_seconds() - G.t0;
    if (G.polyD > 0) {
        k->poly->products = G.prods;
        k->poly->genColumns = k->cycleLens.empty() ? G.its : std::min<long long>(G.its, k->cycleLens[0]);
        k->poly->columns = G.its - k->poly->genColumns;
        if (s->opt.geti("debug")) fprintf(stderr, "[dafoam_amd] polynomial GMRES (degree %d%s): %lld products, %lld columns, |r| %.3e -> %.3e (reason %d)\n", k->poly->degree, k->poly->fallback ? ", fallback" : "", G.prods, G.its, k->res0, k->res, k->reason);
        if (G.nonFinite) return 1;  // a non-finite residual never passes the tolerance rule
    }
    return gmres_failed(k->res, k->res0, G.rtol, G.atol, s->opt.getd("adjEqnOption.gmresTolDiff"));
}

// ---- GMRES with deflated restarting (amd.gmresDeflation): gmres_dr_loop of das_gmres_host.hpp over the device's vector operations; dense-eigen callback
namespace {
struct DrDeviceOps {
    das_solver* s; das_ksp* k; GmresRun* G; int kdefMax;
    DevBuf<double> scratch, Cdev;
    void start(double beta) {
        launch_scale_to(s->stream, s->n, 1.0 / beta, (const double*)k->r.p, (double*)k->V.p, (const float*)nullptr, (float*)nullptr);
    }
    void arnoldi(int j, double* h, double& ww, double& hn) {
        const long long n = s->n;
        hipStream_t st = s->stream;
        pc_apply_full(s, k, k->V.p + (long long)j * n, k->z.p);
        apply_operator(s, k->z.p, k->w.p);
        multidot(s, k, j + 1, k->w.p, G->hh.data());
        launch_multiaxpy(st, n, j + 1, (const double*)k->V.p, n, (const double*)k->hdev.p, (double*)k->w.p, (const float*)nullptr);
        multidot(s, k, j + 1, k->w.p, G->h2.data());
        launch_multiaxpy(st, n, j + 1, (const double*)k->V.p, n, (const double*)k->hdev.p, (double*)k->w.p, (const float*)nullptr);
        double hn2 = 0.0;
        multidot(s, k, 0, k->w.p, &hn2);
        k->nrefine++;
        for (int i = 0; i <= j; i++) h[i] = G->hh[i] + G->h2[i];
        ww = G->hh[j + 1];
        hn = std::sqrt(std::max(hn2, 0.0));
        if (hn > GMRES_BREAKDOWN_TOL * std::sqrt(std::max(ww, 0.0)))
            launch_scale_to(st, n, 1.0 / hn, (const double*)k->w.p, (double*)k->V.p + (long long)(j + 1) * n, (const float*)nullptr, (float*)nullptr);
    }
    void update(int j, const double* y) {
        const long long n = s->n;
        hipStream_t st = s->stream;
        DAS_HIP(hipMemcpyAsync(k->hdev.p, y, j * sizeof(double), hipMemcpyHostToDevice, st));
        DAS_HIP(hipStreamSynchronize(st));  // y is the caller's host vector
        launch_lincomb(st, n, j, (const double*)k->V.p, n, (const double*)k->hdev.p, (double*)k->w.p, (const float*)nullptr);
        pc_apply_full(s, k, k->w.p, k->z.p);
        axpby(s, 1.0, k->z.p, 1.0, G->d_x);
    }
    double true_residual() { gmres_true_residual(s, k, *G, true); return G->beta; }
    void compress(int m, int kk, const double* P1) {
        const long long n = s->n;
        hipStream_t st = s->stream;
        if (scratch.n < (size_t)(kk + 1) * n) scratch.alloc((size_t)(kdefMax + 2) * n);
        if (Cdev.n < (size_t)(m + 1) * 8) Cdev.alloc((size_t)(m + 1) * 8);
        std::vector<double> Cblk;
        for (int c0 = 0; c0 <= kk; c0 += 8) {  // Vnew[:, c0 : c0 + sv) = V[:, 0 : m + 1) P1[:, c0 : c0 + sv)
            const int sv = std::min(8, kk + 1 - c0);
            Cblk.assign((size_t)(m + 1) * sv, 0.0);
            for (int i = 0; i <= m; i++) for (int r = 0; r < sv; r++) Cblk[(size_t)i * sv + r] = P1[(size_t)i * (kk + 1) + c0 + r];
            DAS_HIP(hipMemcpyAsync(Cdev.p, Cblk.data(), Cblk.size() * sizeof(double), hipMemcpyHostToDevice, st));
            launch_block_lincomb(st, n, m + 1, sv, k->V.p, n, Cdev.p, scratch.p + (long long)c0 * n, n);
            DAS_HIP(hipStreamSynchronize(st));  // Cblk / Cdev are reused by the next group
        }
        DAS_HIP(hipMemcpyAsync(k->V.p, scratch.p, (size_t)(kk + 1) * n * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
};
}  // namespace

static int run_gmres_dr(das_solver* s, das_ksp* k, const double* d_rhs, double* d_x, int kdef) {
    GmresRun& G = gmres_begin(s, k, d_rhs, d_x, /* fixed */ false, /* deflated */ true);
    const int m = G.m;
    DAS_CHECK(gmres_map_basis(s, k, m + 2), DAS_ERR_INTERNAL, "GMRES-DR: no device memory for the basis (" + k->V.workerError + ")");
    DrDeviceOps ops{s, k, &G, std::max(1, std::min(kdef, m - 2))};
    const DrResult R = gmres_dr_loop(ops, g_dense_eig, m, kdef, G.beta, G.target, G.maxIts, k->hist);
    gmres_finish_check(s, k);
    G.its = R.its;
    k->iters = (int)R.its;
    k->nBreakdown = R.nBreakdown;
    k->res = R.res;
    k->reason = R.res <= G.target ? 0 : 1;
    k->seconds = wall_seconds() - G.t0;
    if (s->opt.geti("debug")) fprintf(stderr, "[dafoam_amd] GMRES-DR(%d, %d): %lld iterations, %d deflated restarts, %d plain restarts, |r| %.3e -> %.3e\n", m, kdef, R.its, R.nDeflated, R.nRestarts, R.res0, R.res);
    return gmres_failed(k->res, k->res0, G.rtol, G.atol, s->opt.getd("adjEqnOption.gmresTolDiff"));
}

static bool idr_selected(das_solver* s, bool fixed);
static int run_idrs(das_solver* s, das_ksp* k, const double* d_rhs, double* d_x);
static int run_gmres(das_solver* s, das_ksp* k, const double* d_rhs, double* d_x, int fixed_iters) {
    const int polyD = poly_degree(s, fixed_iters > 0);  // opt-in: amd.polyDegree
    if (idr_selected(s, fixed_iters > 0)) return run_idrs(s, k, d_rhs, d_x);  // opt-in: amd.krylovMethod "idrs"
    {   // opt-in: deflated restarting (never for the fixed-iteration bench windows, the Newton primal's inner solves or several ranks)
        const long long kdef = s->opt.geti_or("amd.gmresDeflation", 0);
        if (kdef > 0 && fixed_iters <= 0 && !s->fwd.on && s->opt.geti("adjEqnOption.gmresRestart") < s->opt.geti("adjEqnOption.gmresMaxIters")) {
            if (!s->halo.active && !s->halo_cb) return run_gmres_dr(s, k, d_rhs, d_x, (int)kdef);
            static bool told = false;  // several ranks: the plain restarted solver (the comment promised this, the code threw)
            if (!told) fprintf(stderr, "[dafoam_amd] amd.gmresDeflation is single-rank: this sharded solve runs the undeflated GMRES\n");
            told = true;
        }
    }
    gmres_begin(s, k, d_rhs, d_x, fixed_iters > 0, /* deflated */ false, polyD);
    if (fixed_iters > 0) gmres_advance(s, k, fixed_iters);
    else while (!gmres_advance(s, k, 1 << 20)) {}
    return gmres_end(s, k);
}

// ---- block (multi right-hand-side) GMRES: s adjoints through one Krylov solve (das_block.hpp) ----------------------------
// Right-preconditioned block GMRES with block size s = number of right-hand sides: block Arnoldi with block classical
// Gram-Schmidt applied twice, CholQR2 for the new basis block, the block-Hessenberg least squares by Givens rotations on
// the host, unpreconditioned residual norms per right-hand side, restart when the basis memory is exhausted.  The
// convergence rule is the reference's per system (DALinearEqn.C:320-324, 422-434): every column has to meet
// max(rtol ||b_r||, atol).  dRdW^T is streamed once per iteration for all s vectors (SpMM), V^T W and W -= V H run on
// the matrix cores as tall-skinny fp64 GEMMs; the preconditioner is applied column by column.
struct BlockWork {
    DevBuf<double> V, W, Z, R, Xr, partial, Cdev, Tdev;
    int s = 0, m = 0;
};
// C_host (K x sv, row-major) = V^T W  (V: K vectors, W: sv vectors, both column-major with leading dimension n)
static void block_tn(das_solver* s, BlockWork& bw, const double* V, int K, const double* W, int sv, double* C_host) {
    const size_t need = tsgemm_partial_size(K);
    if (bw.partial.n < need) bw.partial.alloc(need);
    if (bw.Cdev.n < (size_t)K * sv) bw.Cdev.alloc((size_t)K * sv + 1024);
    launch_tsgemm_tn(s->stream, s->n, K, sv, V, s->n, W, s->n, bw.partial.p, bw.Cdev.p);
    DAS_HIP(hipMemcpyAsync(C_host, bw.Cdev.p, (size_t)K * sv * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
}
// W -= V C  (C = K x sv on the host)
static void block_nn_sub(das_solver* s, BlockWork& bw, const double* V, int K, const double* C_host, double* W, int sv) {
    if (bw.Cdev.n < (size_t)K * sv) bw.Cdev.alloc((size_t)K * sv + 1024);
    DAS_HIP(hipMemcpyAsync(bw.Cdev.p, C_host, (size_t)K * sv * sizeof(double), hipMemcpyHostToDevice, s->stream));
    launch_tsgemm_nn_sub(s->stream, s->n, K, sv, V, s->n, bw.Cdev.p, W, s->n);
}
// W = Q S with Q^T Q = I (CholQR applied twice); S (sv x sv upper triangular, row-major) returned on the host
static void block_cholqr2(das_solver* s, BlockWork& bw, double* W, int sv, std::vector<double>& S) {
    std::vector<double> G((size_t)sv * sv), L((size_t)sv * sv), T((size_t)sv * sv), S1((size_t)sv * sv, 0.0), S2((size_t)sv * sv, 0.0);
    if (bw.Tdev.n < 64) bw.Tdev.alloc(64);
    for (int pass = 0; pass < 2; pass++) {
        block_tn(s, bw, W, sv, W, sv, G.data());
        chol_upper_inverse(sv, G.data(), L.data(), T.data());
        DAS_HIP(hipMemcpyAsync(bw.Tdev.p, T.data(), (size_t)sv * sv * sizeof(double), hipMemcpyHostToDevice, s->stream));
        launch_block_right_mult(s->stream, s->n, sv, W, s->n, bw.Tdev.p);
        std::vector<double>& Sp = pass == 0 ? S1 : S2;
        for (int i = 0; i < sv; i++) for (int j = i; j < sv; j++) Sp[(size_t)i * sv + j] = L[(size_t)j * sv + i];  // L^T
    }
    S.assign((size_t)sv * sv, 0.0);  // W = Q2 S2 S1
    for (int i = 0; i < sv; i++) for (int j = i; j < sv; j++) { double a = 0.0; for (int q = i; q <= j; q++) a += S2[(size_t)i * sv + q] * S1[(size_t)q * sv + j]; S[(size_t)i * sv + j] = a; }
}
// ---- IDR(s) (amd.krylovMethod "idrs"): idrs_loop of das_idr_host.hpp over the device's vector operations (das_idr.hpp) ---------------
// No Krylov basis: the path never calls gmres_ws, never reserves or maps k->V.  Its vectors - P, G, U (n x s each), r, z, t and the
// device copies of the right-hand side and the solution - are allocated once per KSP and reused by later solves.
struct IdrWork {
    int s = 0;
    long long n = 0;
    DevBuf<double> P, G, U, partial, coef, sums;
    BlockWork bw;  // scratch of block_cholqr2 (the orthonormalisation of P)
    // last solve (das_ksp_get_idr_info)
    int cycles = 0, restarts = 0, breakdowns = 0;
    // a solve opened by das_ksp_begin_device and not run yet
    bool pending = false;
    const double* d_rhs = nullptr;
    double* d_x = nullptr;
    int rc = 0;
    int work_vectors() const { return 3 * s + 5; }  // P, G, U; r, z, t; rhs and solution on the device
};
// amd.krylovMethod, validated at every solve: true when this solve runs IDR(s).  Fixed-iteration bench windows and the Newton primal's
// inner solves keep GMRES silently; several ranks, or deflated restarting on top, are errors
static bool idr_selected(das_solver* s, bool fixed) {
    const std::string& meth = s->opt.gets("amd.krylovMethod");
    DAS_CHECK(meth == "gmres" || meth == "idrs", DAS_ERR_ARG, "amd.krylovMethod \"" + meth + "\" is not one of gmres | idrs");
    if (meth != "idrs") return false;
    const long long sv = s->opt.geti("amd.idrShadowVectors");
    DAS_CHECK(sv >= 1 && sv <= IDR_MAX_S, DAS_ERR_ARG, "amd.idrShadowVectors " + std::to_string(sv) + " is outside 1 .. 8");
    if (fixed || s->fwd.on) return false;
    DAS_CHECK(!s->halo.active && !s->halo_cb, DAS_ERR_ARG, "amd.krylovMethod \"idrs\" is single-rank (run the sharded solve with \"gmres\")");
    DAS_CHECK(s->opt.geti_or("amd.gmresDeflation", 0) <= 0, DAS_ERR_ARG, "amd.gmresDeflation > 0 belongs to GMRES: not with amd.krylovMethod \"idrs\"");
    return true;
}
// the work vectors of the IDR(s) path (the ones it shares with the GMRES path are re-allocated by gmres_ws when that runs next: restart = 0)
static IdrWork& idr_ws(das_solver* s, das_ksp* k) {
    const long long n = s->n;
    const int sv = (int)std::min<long long>(s->opt.geti("amd.idrShadowVectors"), n);
    if (!k->idr) k->idr.reset(new IdrWork);
    IdrWork& I = *k->idr;
    if (I.s != sv || I.n != n) {
        I.s = sv; I.n = n;
        I.P.alloc((size_t)sv * n); I.G.alloc((size_t)sv * n); I.U.alloc((size_t)sv * n);
        I.partial.alloc(idr_partial_size(n, sv)); I.coef.alloc(4 * IDR_MAX_S); I.sums.alloc(IDR_MAX_S + 2);
    }
    if (k->w.n != (size_t)n || k->z.n != (size_t)n || k->r.n != (size_t)n || k->xdev.n != (size_t)n || k->bdev.n != (size_t)n) {
        k->restart = 0;
        k->w.alloc(n); k->z.alloc(n); k->r.alloc(n); k->xdev.alloc(n); k->bdev.alloc(n);
        k->z.zero();  // the preconditioner's output stays a vector of its own, zero-initialised (as in gmres_ws)
    }
    return I;
}
namespace {
struct IdrDeviceOps {
    das_solver* s; das_ksp* k; IdrWork* I;
    const double* d_rhs; double* d_x;
    double hc[4 * IDR_MAX_S], hs[IDR_MAX_S + 2];  // host side of coef / sums: rewritten only after the synchronisation that follows their use
    void get_sums(int cnt) {
        DAS_HIP(hipMemcpyAsync(hs, I->sums.p, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        DAS_HIP(hipStreamSynchronize(s->stream));
    }
    void shadow(int sv, unsigned seed) {
        launch_idr_shadow(s->stream, s->n, sv, seed, I->P.p, s->n);
        std::vector<double> S;
        block_cholqr2(s, I->bw, I->P.p, sv, S);
    }
    void reset_spaces() {
        DAS_HIP(hipMemsetAsync(I->G.p, 0, (size_t)I->s * s->n * sizeof(double), s->stream));
        DAS_HIP(hipMemsetAsync(I->U.p, 0, (size_t)I->s * s->n * sizeof(double), s->stream));
    }
    void project_r(double* f) {
        launch_multidot<double>(s->stream, s->n, I->s, I->P.p, s->n, k->r.p, I->partial.p, I->sums.p);
        get_sums(I->s);
        std::copy(hs, hs + I->s, f);
    }
    void inner_vec(int kk, const double* c, double omega) {
        const long long n = s->n;
        hipStream_t st = s->stream;
        const int m = I->s - kk;
        for (int i = 0; i < m; i++) { hc[i] = -c[i]; hc[IDR_MAX_S + i] = c[i]; }
        DAS_HIP(hipMemcpyAsync(I->coef.p, hc, 2 * IDR_MAX_S * sizeof(double), hipMemcpyHostToDevice, st));
        double* uk = I->U.p + (long long)kk * n;
        double* gk = I->G.p + (long long)kk * n;
        launch_idr_combine(st, n, m, 1.0, k->r.p, gk, n, I->coef.p, k->w.p);                // v = r - G[:, k:] c
        pc_apply_full(s, k, k->w.p, k->z.p);
        launch_idr_combine(st, n, m, omega, k->z.p, uk, n, I->coef.p + IDR_MAX_S, uk);      // u_k = omega z + U[:, k:] c, in place
        apply_operator(s, uk, gk);
    }
    void dots_g(int kk, double* d, double& gg) {
        launch_multidot<double>(s->stream, s->n, I->s, I->P.p, s->n, I->G.p + (long long)kk * s->n, I->partial.p, I->sums.p);
        get_sums(I->s + 1);
        std::copy(hs, hs + I->s, d);
        gg = hs[I->s];
    }
    double biortho_step(int kk, const double* alpha, double beta) {
        double* h = hc + 2 * IDR_MAX_S;
        for (int j = 0; j < kk; j++) h[j] = alpha[j];
        h[kk] = beta;
        DAS_HIP(hipMemcpyAsync(I->coef.p + 2 * IDR_MAX_S, h, (size_t)(kk + 1) * sizeof(double), hipMemcpyHostToDevice, s->stream));
        launch_idr_biortho_step(s->stream, s->n, kk, I->G.p, I->U.p, s->n, I->coef.p + 2 * IDR_MAX_S, k->r.p, d_x, I->partial.p, I->sums.p);
        get_sums(1);
        return hs[0];
    }
    void smooth_vec() {
        pc_apply_full(s, k, k->r.p, k->z.p);
        apply_operator(s, k->z.p, k->w.p);
    }
    void dots_t(double& tr, double& tt) {
        launch_multidot<double>(s->stream, s->n, 1, k->r.p, s->n, k->w.p, I->partial.p, I->sums.p);
        get_sums(2);
        tr = hs[0]; tt = hs[1];
    }
    double smooth_step(double omega, double* f) {
        launch_idr_smooth_step(s->stream, s->n, I->s, omega, k->r.p, k->w.p, d_x, k->z.p, I->P.p, s->n, I->partial.p, I->sums.p);
        get_sums(I->s + 1);
        std::copy(hs, hs + I->s, f);
        return hs[I->s];
    }
    double norm_r() {
        launch_multidot<double>(s->stream, s->n, 0, k->r.p, s->n, k->r.p, I->partial.p, I->sums.p);
        get_sums(1);
        return std::sqrt(std::max(hs[0], 0.0));
    }
    double true_residual() {
        apply_operator(s, d_x, k->r.p);
        axpby(s, 1.0, d_rhs, -1.0, k->r.p);
        return norm_r();
    }
};
}  // namespace

static int run_idrs(das_solver* s, das_ksp* k, const double* d_rhs, double* d_x) {
    need_init(s);
    DAS_CHECK(s->op, DAS_ERR_STATE, "initializedRdWTMatrixFree() must be called before solveLinearEqn()");
    IdrWork& I = idr_ws(s, k);
    if (k->useBilu) bilu_clear_abort(k->bilu, s->stream);
    const long long n = s->n;
    const double t0 = wall_seconds();
    const double rtol = s->opt.getd("adjEqnOption.gmresRelTol"), atol = s->opt.getd("adjEqnOption.gmresAbsTol");
    const long long maxIts = s->opt.geti("adjEqnOption.gmresMaxIters");
    IdrDeviceOps ops{s, k, &I, d_rhs, d_x};
    double beta0;
    if (s->opt.geti("adjEqnOption.useNonZeroInitGuess") != 0) beta0 = ops.true_residual();
    else {
        DAS_HIP(hipMemsetAsync(d_x, 0, n * sizeof(double), s->stream));
        DAS_HIP(hipMemcpyAsync(k->r.p, d_rhs, n * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        beta0 = ops.norm_r();
    }
    k->nrefine = 0; k->hist.clear(); k->cycleLens.clear();
    k->hist.push_back(beta0);
    const double target = std::max(rtol * beta0, atol);
    const IdrResult R = idrs_loop(ops, I.s, (unsigned)s->opt.geti("amd.idrSeed"), beta0, target, maxIts, k->hist);
    gmres_finish_check(s, k);
    I.cycles = R.cycles; I.restarts = R.nRestarts; I.breakdowns = R.nBreakdown;
    k->iters = (int)R.its;
    k->nBreakdown = R.nBreakdown;
    k->res0 = R.res0;
    k->res = R.res;
    k->reason = R.reason;
    k->seconds = wall_seconds() - t0;
    if (s->opt.geti("debug")) fprintf(stderr, "[dafoam_amd] IDR(%d): %lld products, %d cycles, %d restarts, %d breakdowns, |r| %.3e -> %.3e (reason %d)\n", I.s, R.its, R.cycles, R.nRestarts, R.nBreakdown, R.res0, R.res, R.reason);
    if (R.reason == 3) return 1;  // a non-finite residual never passes the tolerance rule
    return gmres_failed(k->res, k->res0, rtol, atol, s->opt.getd("adjEqnOption.gmresTolDiff"));
}

static void block_spmm(das_solver* s, BlockWork& bw, const Mat& A, const double* X, double* Y, int sv) {
    launch_block_to_rows(s->stream, s->n, sv, X, s->n, bw.Xr.p);
    hipEvent_t ev = nullptr;
    s->timer.begin("spmm", s->stream, ev);
    launch_spmm_wave(s->stream, A.n, sv, A.rowptr.p, A.col.p, A.val.p, bw.Xr.p, Y, s->n);
    s->timer.end("spmm", s->stream, ev);
}

static int run_block_gmres(das_solver* s, das_ksp* k, int sv, const double* d_B, double* d_X) {
    need_init(s);
    DAS_CHECK(s->op, DAS_ERR_STATE, "initializedRdWTMatrixFree() must be called before solveLinearEqn()");
    DAS_CHECK(sv >= 1 && sv <= 8, DAS_ERR_ARG, "block solve: 1 to 8 right-hand sides");
    DAS_CHECK(!s->halo.active && !s->halo_cb, DAS_ERR_ARG, "the block solve is single-rank (shard the right-hand sides across solves instead)");
    const Mat& A = s->op->m;
    const long long n = s->n;
    hipStream_t st = s->stream;
    const long long budget = s->opt.geti_or("amd.maxKrylovBytes", (long long)(32.0 * 1024 * 1024 * 1024));
    const long long maxIts = s->opt.geti("adjEqnOption.gmresMaxIters");
    long long m = std::min<long long>(s->opt.geti("adjEqnOption.gmresRestart"), maxIts);
    m = std::max<long long>(1, std::min<long long>(m, std::min<long long>(budget / (8 * n * sv) - 1, 4000 / sv)));
    if (!k->block) k->block.reset(new BlockWork);
    BlockWork& bw = *k->block;
    if (bw.s != sv || bw.m != (int)m || bw.V.n != (size_t)((m + 1) * sv) * n) {
        bw.s = sv; bw.m = (int)m;
        bw.V.alloc((size_t)((m + 1) * sv) * n);
        bw.W.alloc((size_t)sv * n); bw.Z.alloc((size_t)sv * n); bw.R.alloc((size_t)sv * n); bw.Xr.alloc((size_t)8 * n);
        bw.Z.zero();
    }
    const double rtol = s->opt.getd("adjEqnOption.gmresRelTol"), atol = s->opt.getd("adjEqnOption.gmresAbsTol");
    const double t0 = wall_seconds();
    const int B = 256;
    const int ms = (int)m * sv;
    BlockLsq lsq;
    std::vector<double> S, Hc, Hc2, Y((size_t)ms * sv), res0(sv), res(sv), target(sv);
    auto col_norms = [&](const double* Rblk, std::vector<double>& out) {
        std::vector<double> Gm((size_t)sv * sv);
        block_tn(s, bw, Rblk, sv, Rblk, sv, Gm.data());
        for (int r = 0; r < sv; r++) out[r] = std::sqrt(std::max(Gm[(size_t)r * sv + r], 0.0));
    };
    DAS_HIP(hipMemsetAsync(d_X, 0, (size_t)sv * n * sizeof(double), st));
    DAS_HIP(hipMemcpyAsync(bw.R.p, d_B, (size_t)sv * n * sizeof(double), hipMemcpyDeviceToDevice, st));
    col_norms(bw.R.p, res0);
    for (int r = 0; r < sv; r++) { target[r] = std::max(rtol * res0[r], atol); res[r] = res0[r]; }
    k->hist.clear();
    k->hist.push_back(*std::max_element(res0.begin(), res0.end()));
    long long its = 0;
    auto all_done = [&]() { for (int r = 0; r < sv; r++) if (res[r] > target[r]) return false; return true; };
    while (!all_done() && its < maxIts) {
        // ---- new cycle: R = V_0 S0
        DAS_HIP(hipMemcpyAsync(bw.V.p, bw.R.p, (size_t)sv * n * sizeof(double), hipMemcpyDeviceToDevice, st));
        block_cholqr2(s, bw, bw.V.p, sv, S);
        lsq.reset((int)m, sv, S.data());
        int j = 0;
        for (; j < m && its < maxIts; j++) {
            double* Vj = bw.V.p + (size_t)j * sv * n;
            pc_apply_block(s, k, Vj, bw.Z.p, sv);
            block_spmm(s, bw, A, bw.Z.p, bw.W.p, sv);
            const int K = (j + 1) * sv;
            Hc.assign((size_t)K * sv, 0.0); Hc2.assign((size_t)K * sv, 0.0);
            block_tn(s, bw, bw.V.p, K, bw.W.p, sv, Hc.data());
            block_nn_sub(s, bw, bw.V.p, K, Hc.data(), bw.W.p, sv);
            block_tn(s, bw, bw.V.p, K, bw.W.p, sv, Hc2.data());      // second Gram-Schmidt pass (block CGS2)
            block_nn_sub(s, bw, bw.V.p, K, Hc2.data(), bw.W.p, sv);
            double* Vn = bw.V.p + (size_t)(j + 1) * sv * n;
            DAS_HIP(hipMemcpyAsync(Vn, bw.W.p, (size_t)sv * n * sizeof(double), hipMemcpyDeviceToDevice, st));
            block_cholqr2(s, bw, Vn, sv, S);
            lsq.add_column(j, Hc.data(), Hc2.data(), S.data());
            its++;
            lsq.residuals(j, res.data());
            k->hist.push_back(*std::max_element(res.begin(), res.end()));
            if (all_done()) { j++; break; }
        }
        // ---- x += M^-1 (V Y),  R Y = G  (upper triangular, K x K)
        const int K = j * sv;
        lsq.solve(j, Y.data());
        if (bw.Cdev.n < (size_t)K * sv) bw.Cdev.alloc((size_t)K * sv + 1024);
        DAS_HIP(hipMemcpyAsync(bw.Cdev.p, Y.data(), (size_t)K * sv * sizeof(double), hipMemcpyHostToDevice, st));
        launch_block_lincomb(st, n, K, sv, bw.V.p, n, bw.Cdev.p, bw.W.p, n);
        pc_apply_block(s, k, bw.W.p, bw.Z.p, sv);
        axpby(s, 1.0, bw.Z.p, 1.0, d_X, (long long)sv * n);
        // true residuals
        block_spmm(s, bw, A, d_X, bw.R.p, sv);
        axpby(s, 1.0, d_B, -1.0, bw.R.p, (long long)sv * n);
        col_norms(bw.R.p, res);
        k->hist.back() = *std::max_element(res.begin(), res.end());
    }
    gmres_finish_check(s, k);
    k->iters = (int)its;
    k->seconds = wall_seconds() - t0;
    k->block_res0 = res0; k->block_res = res;
    k->res0 = *std::max_element(res0.begin(), res0.end());
    k->res = *std::max_element(res.begin(), res.end());
    const double diff = s->opt.getd("adjEqnOption.gmresTolDiff");
    int failed = 0;
    for (int r = 0; r < sv; r++) if (gmres_failed(res[r], res0[r], rtol, atol, diff)) failed = 1;  // per system
    return failed;
}

// ---- Newton-Krylov primal (survey row f4: the step before the adjoint, reference DASimpleFoam.C:123-185 solvePrimal) -----------
// The reference iterates SIMPLE (UEqn -> pEqn -> turbulence) until the residuals of DAResidualSimpleFoam fall below
// primalMinResTol.  Its fixed point is R(W) = 0 for exactly the residual this library evaluates, so the MI355X primal solves
// R(W) = 0 with the machinery of the adjoint: pseudo-transient Newton, every step (dR/dW S + D/tau) dw = -R by GMRES with
//   * the operator applied matrix-free by ONE forward-mode (dual-number) residual pass (no assembled Jacobian),
//   * the preconditioner = node-block ILU(0) of jacPCMat^T (coloured FD, diagonal scaled by 1 + 1/tau) + the pressure coarse
//     space - the adjoint's preconditioner with transposed blocks, rebuilt every `pcLag` steps,
//   * tau from switched evolution relaxation (tau = tau0 ||R0|| / ||R||), a backtracking update that keeps nuTilda >= 0.
// Verified against the oracle's SIMPLE fixed point (tests): same W* to 1e-6.
struct NewtonInfo { int steps = 0, linIters = 0, pcBuilds = 0; double res0 = 0, res = 0, seconds = 0; std::vector<double> hist; };

static double device_norm2(das_solver* s, das_ksp* k, const double* x) {
    double h = 0.0;
    multidot_dev(s, k, x, 0, x, k->hdev.p);
    DAS_HIP(hipMemcpyAsync(&h, k->hdev.p, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return std::sqrt(std::max(h, 0.0));
}

static int run_newton_primal(das_solver* s, int maxSteps, double relTol, double absTol, NewtonInfo& info) {
    need_init(s);
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SIMPLEFOAM || DAS_IS_COMPRESSIBLE(s->cp.solver) || s->cp.solver == DAS_SOLVER_HEATTRANSFERFOAM ||
                  s->cp.solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM,
              DAS_ERR_ARG, "the Newton primal needs a flow solver, DAHeatTransferFoam or DASolidDisplacementFoam");
    if (s->cp.solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM) {
        // without a fixedValue patch a rigid translation of D changes nothing: the steady elastic problem is singular
        bool anchored = false;
        for (int p = 0; p < (int)s->mesh.bc.size(); p++) anchored = anchored || (s->mesh.patch_size[p] > 0 && s->mesh.bc[p].U_code == DAS_BC_FIXED_VALUE);
        DAS_CHECK(anchored, DAS_ERR_ARG, "DASolidDisplacementFoam: no patch carries a fixedValue D - the steady elastic problem is singular");
    }
    if (s->cp.solver == DAS_SOLVER_HEATTRANSFERFOAM) {
        // pure zeroGradient boundaries leave T undetermined up to a constant: the steady conduction problem is singular
        bool anchored = false;
        for (int p = 0; p < (int)s->mesh.bc.size(); p++) {
            const int code = s->mesh.bc[p].T_code;
            anchored = anchored || (s->mesh.patch_size[p] > 0 && (code == DAS_BC_FIXED_VALUE || code == DAS_BC_MIXED));
        }
        DAS_CHECK(anchored, DAS_ERR_ARG, "DAHeatTransferFoam: no patch carries a fixedValue or mixed T - the steady conduction problem is singular");
    }
    DAS_CHECK(!s->halo.active && !s->halo_cb, DAS_ERR_ARG, "the Newton primal is single-rank");
    const long long n = s->n;
    const int B = 256;
    hipStream_t st = s->stream;
    const double t0 = wall_seconds();
    const double tau0 = s->opt.getd("amd.primalTau0"), linTol = s->opt.getd("amd.primalLinearTol");
    const int pcLag = (int)std::max<long long>(1, s->opt.geti("amd.primalPCLag"));
    const double serExp = s->opt.getd("amd.primalSERExponent");
    const long long linIters = s->opt.geti("amd.primalLinearIters");
    const bool ramp = s->opt.gets("amd.primalTauMode") == "ramp";
    // WHERE the pseudo-time term acts (amd.primalPseudoTimeFields).  "all" (default, round 2): every row.  "momentum": the transported
    // cell fields (U, T, nuTilda) only - implicit under-relaxation of the transport equations, the pressure and the face fluxes follow
    // algebraically, as in a coupled pressure-based solver.  Measured with the host-emulated kernel bodies and exact Jacobians on the
    // NACA0012 O-grid (round 4, tools/naca_newton_cpu_twin.py): from a COLD start the term on the pressure rows makes the pseudo-time
    // evolution itself unstable beyond tau ~ 3 (a disturbance grows ~1.3x per step until it explodes; with the line search the
    // residual just wanders), without it the residual falls monotonically while tau ramps up.  From a start CLOSE to the solution (a
    // prolonged coarse solution) it is the other way round: "all" + switched evolution relaxation crosses the unstable range in a
    // few steps, the unshifted pressure rows of "momentum" make every small-tau system as hard as the tau = inf one.
    const bool ptMomentum = s->opt.gets("amd.primalPseudoTimeFields") == "momentum";
    long long pLo = 0, pHi = 0, phiLo = (long long)1 << 62;
    for (const StateDef& q : s->st_full.states) {
        if (q.name == "p") { pLo = q.offset; pHi = q.offset + q.size; }
        if (q.name == "phi") phiLo = q.offset;
    }
    const double growth = s->opt.getd("amd.primalTauGrowth"), growthMax = s->opt.getd("amd.primalTauGrowthMax"), tauMax = s->opt.getd("amd.primalTauMax");
    const double acceptFactor = s->opt.getd("amd.primalAcceptFactor"), tauMin = s->opt.getd("amd.primalTauMin");
    const bool rejectDamped = ramp && s->opt.gets("amd.primalDampedSteps") == "reject";
    int nRejected = 0;
    double tauPC = 0.0;
    ensure_coloring(s);
    // Krylov options of the inner solves (restored afterwards)
    const Options saved = s->opt;
    s->opt.i["adjEqnOption.gmresMaxIters"] = linIters;
    s->opt.i["adjEqnOption.gmresRestart"] = linIters;
    s->opt.d["adjEqnOption.gmresRelTol"] = linTol;
    s->opt.d["adjEqnOption.gmresAbsTol"] = 1e-300;
    s->opt.i["adjEqnOption.useNonZeroInitGuess"] = 0;
    struct Restore { das_solver* s; Options o; ~Restore() { s->opt = o; s->fwd.on = false; } } restore{s, saved};
    const StateDef* sdN = nullptr;
    for (const StateDef& q : s->st_full.states) if (q.name == "nuTilda") sdN = &q;
    const long long n0 = sdN ? sdN->offset : 0, n1 = sdN ? sdN->offset + sdN->size : 0;
    ResParams prm = make_params(s->cp, s->opt, 0);
    DevBuf<double> Rc(n), Rn(n), Wn(n), rhs(n), dw(n);  // Rc: residual at the current states (s->d_R is scratch of the FD assembly)
    std::unique_ptr<das_ksp> k;
    std::unique_ptr<das_mat> P;
    auto residual_at = [&](const double* W, double* R) { eval_residual<double>(s->dm, s->cp, prm, W, R, s->wk, s->d_phiF.p, s->d_Told.p, st); };
    // a scratch KSP just for norms before the first preconditioner exists
    std::unique_ptr<das_ksp> scratch(new das_ksp);
    scratch->partial.alloc(multidot_partial_size(n, 1));
    scratch->hdev.alloc(8);
    residual_at(s->d_W.p, Rc.p);
    double rn = device_norm2(s, scratch.get(), Rc.p);
    info = NewtonInfo();
    info.res0 = rn;
    info.hist.push_back(rn);
    double tau = tau0;
    int sincePC = pcLag;
    for (int step = 0; step < maxSteps && rn > std::max(relTol * info.res0, absTol); step++) {
        if (!(rn == rn)) break;
        if (sincePC >= pcLag) {
            // jacPCMat at the current states (coloured FD), transposed node-block ILU with the pseudo-transient diagonal
            // ONE Krylov object for the whole run: only its preconditioner is rebuilt - the basis (a mapped virtual range at
            // >= 4 GB) and the work vectors stay (round 4: ~160 create / map / unmap cycles of the basis at 200 k cells ended in a
            // device memory fault, and the re-mapping was pure overhead)
            if (k) { k->pcmat = nullptr; DAS_HIP(hipStreamSynchronize(st)); }
            P.reset(assemble(s, 1, 0));
            if (!k) k.reset(new das_ksp);
            k->pcmat = P.get();
            k->pcTranspose = true;
            k->pcDiagScale = 1.0 + 1.0 / tau;
            tauPC = tau;
            if (ptMomentum) { k->shiftExLo = pLo; k->shiftExHi = pHi; k->shiftEnd = phiLo; }
            setup_node_ilu(s, k.get(), /*byEstimate*/ false);
            setup_coarse(s, k.get());
            if (s->fwd.diag.n != (size_t)n) s->fwd.diag.alloc(n);
            hipLaunchKernelGGL(k_extract_diag, dim3(nblk(n, B)), dim3(B), 0, st, n, P->m.rowptr.p, P->m.col.p, P->m.val.p, s->fwd.diag.p, k->shiftExLo,
                               k->shiftExHi, k->shiftEnd);
            sincePC = 0;
            info.pcBuilds++;
        }
        sincePC++;
        s->fwd.on = true;
        s->fwd.invTau = 1.0 / tau;
        launch_scale_to(st, n, -1.0, (const double*)Rc.p, (double*)rhs.p, (const float*)nullptr, (float*)nullptr);
        run_gmres(s, k.get(), rhs.p, dw.p, 0);
        s->fwd.on = false;
        info.linIters += k->iters;
        // backtracking: accept the first step that does not blow the residual up.  amd.primalDampedSteps "reject" (ramp mode): a
        // step that needs damping is NOT taken at all - the pseudo-time step is halved and the step recomputed (a damped Newton
        // update of a strongly under-relaxed system is a poor direction; rejecting keeps the iteration on the pseudo-time path),
        // unless tau has already reached its floor amd.primalTauMin, where the damped update is the last resort
        double omega = 1.0, rnew = rn;
        const int maxHalvings = (rejectDamped && tau > tauMin) ? 1 : 8;
        for (int ls = 0; ls < maxHalvings; ls++) {
            hipLaunchKernelGGL(k_newton_update, dim3(nblk(n, B)), dim3(B), 0, st, n, n0, n1, omega, s->d_W.p, s->d_scale.p, dw.p, Wn.p);
            residual_at(Wn.p, Rn.p);
            rnew = device_norm2(s, k.get(), Rn.p);
            if (rnew == rnew && rnew < acceptFactor * rn) break;
            if (ls + 1 < maxHalvings) omega *= 0.5;
        }
        const bool accepted = rnew == rnew && rnew < acceptFactor * rn;
        if (ramp && !accepted) {
            // no (damped) update is acceptable: the step is rejected, the pseudo-time step cut, the preconditioner rebuilt
            tau = std::max(tauMin, tau * (rejectDamped ? 0.5 : 0.1));
            if (tau < 0.25 * tauPC || tau > 4.0 * tauPC) sincePC = pcLag;
            info.steps = step + 1;
            info.hist.push_back(rn);
            if (s->opt.geti("debug")) fprintf(stderr, "[dafoam_amd] Newton primal step %d: REJECTED (|R| would be %.3e, %d GMRES iterations), tau -> %.2e\n", step + 1, rnew, k->iters, tau);
            if (++nRejected > 40) break;  // the pseudo-time path is lost
            continue;
        }
        DAS_HIP(hipMemcpyAsync(s->d_W.p, Wn.p, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        DAS_HIP(hipMemcpyAsync(Rc.p, Rn.p, n * sizeof(double), hipMemcpyDeviceToDevice, st));
        // a preconditioner built for a much smaller tau is rebuilt early
        // "ser": switched evolution relaxation on the INITIAL residual (tau = tau0 (|R0|/|R|)^p - fine when the start is close,
        // e.g. a prolonged coarse solution); "ramp": the CFL ramp of implicit RANS solvers - tau grows by at least `growth` per
        // full step (a start far from the solution first RAISES the residual norm while the boundary layers form: tying tau to
        // |R0|/|R| would shrink it there), by the residual drop (^p) when that is larger, and shrinks with a damped update
        const double tauNew = !ramp ? std::min(1e12, tau0 * std::pow(info.res0 / std::max(rnew, 1e-300), serExp))
                                    : std::min(tauMax, tau * (omega == 1.0 ? std::max(growth, std::min(growthMax, std::pow(rn / std::max(rnew, 1e-300), serExp))) : std::max(omega, 0.25)));
        if (tauNew > 4.0 * tauPC || tauNew < 0.25 * tauPC) sincePC = pcLag;
        tau = std::max(tauMin, tauNew);
        rn = rnew;
        info.steps = step + 1;
        info.hist.push_back(rn);
        if (s->opt.geti("debug")) fprintf(stderr, "[dafoam_amd] Newton primal step %d: |R| %.3e (omega %.3f, %d GMRES iterations, tau %.2e)\n", step + 1, rn, omega, k->iters, tau);
    }
    DAS_HIP(hipStreamSynchronize(st));
    s->h_W = s->d_W.to_host();
    info.res = rn;
    info.seconds = wall_seconds() - t0;
    return (rn <= std::max(relTol * info.res0, absTol)) ? 0 : 1;
}

// =====================================================================================================
// C-ABI
// =====================================================================================================
extern "C" {

const char* das_last_error(void) { return g_err.c_str(); }
int das_version(void) { return 100; }
int das_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

das_solver_t* das_create(const das_case_t* c) {
    try {
        DAS_CHECK(c, DAS_ERR_ARG, "null case");
        std::unique_ptr<das_solver> s(new das_solver);
        s->t0_wall = wall_seconds();
        s->t0_cpu = std::clock();
        s->cp.from_case(c);
        s->mesh.build(c);
        s->opt.s["solverName"] = c->solver == DAS_SOLVER_PIMPLEFOAM ? "DAPimpleFoam" : c->solver == DAS_SOLVER_SIMPLEFOAM ? "DASimpleFoam" : (c->solver == DAS_SOLVER_RHOSIMPLEFOAM ? "DARhoSimpleFoam" : (c->solver == DAS_SOLVER_TURBOFOAM ? "DATurboFoam" : (c->solver == DAS_SOLVER_HEATTRANSFERFOAM ? "DAHeatTransferFoam" : (c->solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM ? "DASolidDisplacementFoam" : "DAScalarTransportFoam"))));
        s->st_full = make_stencil(s->cp.solver, s->mesh.nC, s->mesh.nF, s->opt, false, s->cp.hasT != 0, s->reg_needs_p());
        s->n = s->st_full.n;
        s->h_W.assign(s->n, 0.0);
        compute_scales(s.get());
        return s.release();
    } catch (const std::exception& e) {
        fail(e);
        return nullptr;
    }
}
void das_destroy(das_solver_t* s) {
    if (!s) return;
    if (s->stream && s->own_stream) (void)hipStreamDestroy(s->stream);
    delete s;
}
int das_set_option_double(das_solver_t* s, const char* key, double v) {
    DAS_TRY
    DAS_CHECK(s && key, DAS_ERR_ARG, "null argument");
    { auto it = s->opt.d.find(key); if (it == s->opt.d.end() || it->second != v || s->opt.i.count(key)) s->opEpoch++; }
    s->opt.d[key] = v;
    s->opt.i.erase(key);
    if (std::string(key).rfind("normalizeStates.", 0) == 0) compute_scales(s);
    return DAS_OK;
    DAS_CATCH
}
int das_set_option_int(das_solver_t* s, const char* key, long long v) {
    DAS_TRY
    DAS_CHECK(s && key, DAS_ERR_ARG, "null argument");
    std::string k(key);
    if (s->opt.d.count(k) && !s->opt.i.count(k)) return das_set_option_double(s, key, (double)v);
    { auto it = s->opt.i.find(k); if (it == s->opt.i.end() || it->second != v) s->opEpoch++; }
    s->opt.i[k] = v;
    if (k.rfind("maxResConLv4JacPCMat.", 0) == 0) s->colored = false;
    return DAS_OK;
    DAS_CATCH
}
int das_set_option_str(das_solver_t* s, const char* key, const char* v) {
    DAS_TRY
    DAS_CHECK(s && key && v, DAS_ERR_ARG, "null argument");
    std::string k(key);
    if (k == "adjStateOrdering") DAS_CHECK(std::string(v) == "state", DAS_ERR_ARG, "adjStateOrdering: only \"state\" is implemented");
    { auto it = s->opt.s.find(k); if (it == s->opt.s.end() || it->second != v) s->opEpoch++; }
    s->opt.s[k] = v;
    return DAS_OK;
    DAS_CATCH
}
int das_get_option_double(das_solver_t* s, const char* key, double* v) {
    DAS_TRY
    DAS_CHECK(s && key && v, DAS_ERR_ARG, "null argument");
    *v = s->opt.getd(key);
    return DAS_OK;
    DAS_CATCH
}
// a string option into buf (cap bytes, always terminated); returns the length of the value
int das_get_option_string(das_solver_t* s, const char* key, char* buf, int cap) {
    DAS_TRY
    DAS_CHECK(s && key && buf && cap > 0, DAS_ERR_ARG, "null argument");
    const std::string& v = s->opt.gets(key);
    const size_t m = std::min(v.size(), (size_t)cap - 1);
    std::copy(v.begin(), v.begin() + m, buf);
    buf[m] = 0;
    return (int)v.size();
    DAS_CATCH
}

int das_init_solver(das_solver_t* s, int device) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    int nd = das_device_count();
    DAS_CHECK(nd > 0, DAS_ERR_NO_DEVICE, "no HIP device visible: the dafoam_amd compute path is GPU-only (no CPU fallback)");
    DAS_CHECK(device >= 0 && device < nd, DAS_ERR_ARG, "device index out of range");
    DAS_HIP(hipSetDevice(device));
    s->device = device;
    DAS_HIP(hipStreamCreate(&s->stream));
    s->own_stream = true;
    if (!s->owned.empty()) s->d_owned.upload(s->owned);
    if (!s->cp.beta_fi.empty()) { s->d_betaFI.upload(s->cp.beta_fi); s->cp.betaFI_ptr = s->d_betaFI.p; }
    const Mesh& m = s->mesh;
    s->d_fg.upload(m.fg); s->d_cg.upload(m.cg);
    s->d_cf_ptr.upload(m.cf_ptr); s->d_cf_face.upload(m.cf_face); s->d_cf_other.upload(m.cf_other);
    s->d_owner.upload(m.owner);
    if (m.nIF) s->d_neigh.upload(m.neighbour);
    s->d_bpatch.upload(m.bface_patch);
    s->d_cyc.upload(m.cyc_face);
    s->d_bc.upload(m.bc);
    if (!s->cp.phi_frozen.empty()) s->d_phiF.upload(s->cp.phi_frozen);
    if (!s->cp.T_old.empty()) s->d_Told.upload(s->cp.T_old);
    if (!s->h_W0.empty()) { s->d_W0.upload(s->h_W0); s->cp.W0_ptr = s->d_W0.p; }
    if (!s->h_W00.empty()) { s->d_W00.upload(s->h_W00); s->cp.W00_ptr = s->d_W00.p; }
    s->dm = DevMesh{m.nC, m.nF, m.nIF, s->d_fg.p, s->d_cg.p, s->d_cf_ptr.p, s->d_cf_face.p, s->d_cf_other.p, s->d_owner.p, s->d_neigh.p,
                    s->d_bpatch.p, s->d_bc.p, s->d_cyc.p};
    if (!m.mixed.empty()) { s->d_mixed.upload(m.mixed); s->dm.mixed = s->d_mixed.p; }
    if (!m.trac_cells.empty()) {  // DASolidDisplacementFoam: the compact list the traction passes run over
        s->d_tracCells.upload(m.trac_cells);
        s->cp.tracCells_ptr = s->d_tracCells.p;
        s->cp.nTrac = (int)m.trac_cells.size();
    }
    s->d_W.upload(s->h_W);
    s->d_R.alloc(s->n);
    s->d_tmp1.alloc(s->n);
    s->d_tmp2.alloc(s->n);
    s->inited = true;
    compute_scales(s);
    refresh_heat_sources(s, true);
    refresh_actuator_disks(s, true);
    if (!s->regModels.empty()) reg_sync(s);
    return DAS_OK;
    DAS_CATCH
}

long long das_get_n_local_adjoint_states(das_solver_t* s) { return s ? s->n : -1; }
long long das_get_n_local_cells(das_solver_t* s) { return s ? s->mesh.nC : -1; }
long long das_get_n_global_cells(das_solver_t* s) { return s ? (s->nGlobalCells > 0 ? s->nGlobalCells : (long long)s->mesh.nC) : -1; }
// sharded runs: the cell count of the whole (undecomposed) mesh, set by the partitioner
int das_set_n_global_cells(das_solver_t* s, long long nGlobal) {
    DAS_TRY
    DAS_CHECK(s && nGlobal > 0, DAS_ERR_ARG, "bad argument");
    s->nGlobalCells = nGlobal;
    return DAS_OK;
    DAS_CATCH
}
long long das_get_n_local_points(das_solver_t* s) { return s ? s->mesh.nP : -1; }
long long das_get_n_local_faces(das_solver_t* s) { return s ? s->mesh.nF : -1; }

// DASolver::updateOFMesh (reference pyDASolvers.pyx:297-300): new point coordinates -> fvMesh metrics recomputed, the
// device copies refreshed.  Matrices assembled before the call keep describing the old mesh (the caller rebuilds them,
// like the reference after setVolCoords); the frozen wall distance is kept (DASpalartAllmaras.C:94).
int das_update_of_mesh(das_solver_t* s, const double* points) {
    DAS_TRY
    DAS_CHECK(s && points, DAS_ERR_ARG, "null argument");
    Mesh& m = s->mesh;
    std::vector<double> y(m.nC);
    for (int c = 0; c < m.nC; c++) y[c] = m.cg[c].y;
    m.points.assign(points, points + 3 * (size_t)m.nP);
    m.compute_geometry(y.data());
    s->geomVersion++;
    if (s->inited) {
        DAS_HIP(hipStreamSynchronize(s->stream));
        s->d_fg.upload(m.fg);
        s->d_cg.upload(m.cg);
    }
    compute_scales(s);
    refresh_heat_sources(s, true);  // Vt, the volume of a cell set and a snapped centre follow the metrics; the set and the cell stay
    refresh_actuator_disks(s, true);  // the field and an adjustThrust scale follow the metrics; a cell set stays
    return DAS_OK;
    DAS_CATCH
}
int das_get_of_mesh_points(das_solver_t* s, double* points) {
    DAS_TRY
    DAS_CHECK(s && points, DAS_ERR_ARG, "null argument");
    std::copy(s->mesh.points.begin(), s->mesh.points.end(), points);
    return DAS_OK;
    DAS_CATCH
}
// metrics of a bare mesh, no solver handle (input generators: dafoam_amd/meshgen.py at bench sizes)
int das_mesh_metrics(int nPoints, const double* points, int nFaces, int nInternalFaces, int nCells, const int* facePtr, const int* facePts, const int* owner,
                     const int* neighbour, double* Sf, double* Cf, double* C, double* V, double* weights) {
    DAS_TRY
    DAS_CHECK(points && facePtr && facePts && owner && neighbour && Sf && Cf && C && V, DAS_ERR_ARG, "null argument");
    mesh_metrics_only(nPoints, points, nFaces, nInternalFaces, nCells, facePtr, facePts, owner, neighbour, Sf, Cf, C, V, weights);
    return DAS_OK;
    DAS_CATCH
}
int das_get_geometry(das_solver_t* s, double* Sf, double* Cf, double* C, double* V, double* w, double* nod, double* corr, double* bdc) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    const Mesh& m = s->mesh;
    for (int f = 0; f < m.nF; f++) {
        const FaceGeom& g = m.fg[f];
        for (int k = 0; k < 3; k++) { if (Sf) Sf[3 * f + k] = g.Sf[k]; if (Cf) Cf[3 * f + k] = g.Cf[k]; }
        if (f < m.nIF) {
            if (w) w[f] = g.w;
            if (nod) nod[f] = g.nod;
            if (corr) for (int k = 0; k < 3; k++) corr[3 * f + k] = g.corr[k];
        } else if (bdc) bdc[f - m.nIF] = g.nod;
    }
    for (int c = 0; c < m.nC; c++) {
        if (C) for (int k = 0; k < 3; k++) C[3 * c + k] = m.cg[c].C[k];
        if (V) V[c] = m.cg[c].V;
    }
    return DAS_OK;
    DAS_CATCH
}

int das_update_of_fields(das_solver_t* s, const double* states) {
    DAS_TRY
    DAS_CHECK(s && states, DAS_ERR_ARG, "null argument");
    s->h_W.assign(states, states + s->n);
    if (s->inited) s->d_W.upload(s->h_W);
    return DAS_OK;
    DAS_CATCH
}
int das_get_of_fields(das_solver_t* s, double* states) {
    DAS_TRY
    DAS_CHECK(s && states, DAS_ERR_ARG, "null argument");
    std::copy(s->h_W.begin(), s->h_W.end(), states);
    return DAS_OK;
    DAS_CATCH
}
int das_calc_residuals(das_solver_t* s, int isPC, double* residuals) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(residuals, DAS_ERR_ARG, "null argument");
    ResParams prm = make_params(s->cp, s->opt, isPC);
    hipEvent_t ev = nullptr;
    s->timer.begin("residual", s->stream, ev);
    eval_residual<double>(s->dm, s->cp, prm, s->d_W.p, s->d_R.p, s->wk, s->d_phiF.p, s->d_Told.p, s->stream);
    s->timer.end("residual", s->stream, ev);
    DAS_HIP(hipMemcpyAsync(residuals, s->d_R.p, s->n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return DAS_OK;
    DAS_CATCH
}
int das_get_residuals(das_solver_t* s, double* residuals) { return das_calc_residuals(s, 0, residuals); }

// =====================================================================================================
// SIMPLE sweeps on the device (das_simple.hpp; reference DASimpleFoam.C:123-185, UEqnSimple.H, pEqnSimple.H, DASpalartAllmaras.C:386-405)
// =====================================================================================================
__global__ __launch_bounds__(256) void k_simple_ueqn(DevMesh m, ResParams prm, const double* __restrict__ W, const double* gP, const double* fc, const double* brec, double* D,
                                                     double* bd, double* sb, double* rhs) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_simple_ueqn(c, m, prm, W, gP, fc, brec, D, bd, sb, rhs);
}
__global__ __launch_bounds__(256) void k_simple_offdiag(DevMesh m, ResParams prm, const double* __restrict__ W, const double* fc, int cdIdx, double* up, double* lo) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < m.nIF) body_simple_offdiag(f, m, prm, W, fc, cdIdx, up, lo);
}
__global__ __launch_bounds__(256) void k_ldu_mv(DevMesh m, const double* __restrict__ diag, const double* __restrict__ up, const double* __restrict__ lo,
                                                const double* __restrict__ x, double* __restrict__ y, double sign) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) y[c] = sign * body_ldu_row(c, m, diag, up, lo, x);
}
__global__ __launch_bounds__(256) void k_simple_hbya(DevMesh m, const double* __restrict__ Us, const double* D, const double* bd, const double* sb, const double* up,
                                                     const double* lo, double* rAU, double* HbyA) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_simple_hbya(c, m, Us, D, bd, sb, up, lo, rAU, HbyA);
}
__global__ __launch_bounds__(256) void k_simple_pface(DevMesh m, ResParams prm, const double* __restrict__ Wn, const double* nut, const double* rAU, const double* HbyA,
                                                      double* phiH, double* gpf, double* cp, double* pbc) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < m.nF) body_simple_pface(f, m, prm, Wn, nut, rAU, HbyA, phiH, gpf, cp, pbc);
}
__global__ __launch_bounds__(256) void k_simple_peqn(DevMesh m, const double* phiH, const double* gpf, const double* cp, const double* pbc, const double* gradP, double* dp,
                                                     double* rhs) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_simple_peqn(c, m, phiH, gpf, cp, pbc, gradP, dp, rhs);
}
__global__ __launch_bounds__(256) void k_simple_gradp(DevMesh m, const double* __restrict__ pcell, const double* pbc, double* gradP) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_simple_gradp(c, m, pcell, pbc, gradP);
}
__global__ __launch_bounds__(256) void k_simple_flux(DevMesh m, const double* __restrict__ pn, const double* gradP, const double* phiH, const double* gpf, const double* cp,
                                                     const double* pbc, double* phiOut) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < m.nF) body_simple_flux(f, m, pn, gradP, phiH, gpf, cp, pbc, phiOut);
}
__global__ __launch_bounds__(256) void k_simple_saeqn(DevMesh m, ResParams prm, const double* __restrict__ W, const double* gU, const double* gN, const double* fc,
                                                      const double* brec, double* diag, double* rhs) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < m.nC) body_simple_saeqn(c, m, prm, W, gU, gN, fc, brec, diag, rhs);
}
__global__ __launch_bounds__(256) void k_simple_correct(long long N, int offP, const double* __restrict__ HbyA, const double* rAU, const double* gradP, const double* pRel,
                                                        double* Wn) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < N) body_sv_correct(c, N, offP, HbyA, rAU, gradP, pRel, Wn);
}
// small vector kernels of the inner Krylov solvers (host scalars; the sweeps are the reference's primal, not the fast path); their dot
// product is k_sv_dot of das_reduce.hpp
__global__ __launch_bounds__(256) void k_sv_lin(long long n, double* y, double a, const double* x, double b, const double* z) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) body_sv_lin(i, y, a, x, b, z);
}
__global__ __launch_bounds__(256) void k_sv_bicg_p(long long n, double* p, const double* r, double beta, double om, const double* v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) body_sv_bicg_p(i, p, r, beta, om, v);
}
__global__ __launch_bounds__(256) void k_sv_divdiag(long long n, double* out, const double* in, const double* diag, double sign) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) body_sv_divdiag(i, out, in, diag, sign);
}
__global__ __launch_bounds__(256) void k_sv_bicg_x(long long n, double* x, double alpha, const double* ph, double om, const double* sh, double* r, const double* s, const double* t) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) body_sv_bicg_x(i, x, alpha, ph, om, sh, r, s, t);
}
__global__ __launch_bounds__(256) void k_sv_gather3(long long n, const double* W, int k, const double* D, const double* bd, const double* rhs3, double* x, double* dg, double* b) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) body_sv_gather3(c, W, k, D, bd, rhs3, x, dg, b);
}
__global__ __launch_bounds__(256) void k_sv_scatter3(long long n, const double* x, int k, double* W) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n) body_sv_scatter3(c, x, k, W);
}
__global__ __launch_bounds__(256) void k_sv_relax(long long n, double* pn, const double* pold, double alpha) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) body_sv_relax(i, pn, pold, alpha);
}
__global__ __launch_bounds__(256) void k_sv_bound(long long n, const double* x, double lo, double* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) body_sv_bound(i, x, lo, out);
}

// device storage of one run of sweeps: the vectors of SimpleVecs and the partial sums of the dot product
struct SimpleWork {
    std::vector<DevBuf<double>> store;
    DevBuf<double> part{DAS_SV_DOT_MAX_BLOCKS}, red{2};
    double* take(long long cnt) { store.emplace_back((size_t)cnt); return store.back().p; }
};
static double sv_dot(hipStream_t st, SimpleWork& w, long long n, const double* a, const double* b) {
    launch_sv_dot(st, n, a, b, w.part.p, w.red.p);
    double h[2];
    DAS_HIP(hipMemcpyAsync(h, w.red.p, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    DAS_HIP(hipStreamSynchronize(st));
    return h[0];
}
// the operations of simple_sweep / simple_bicgstab / simple_pcg (das_simple_host.hpp) as kernel launches on the solver's stream
extern "C++" struct SimpleDeviceOps {  // (a member template inside the C-ABI block)
    const DevMesh& dm;
    ResParams prm;
    ResWork<double>& wk;
    hipStream_t st;
    SimpleWork w;
    SimpleVecs v{};
    SimpleDeviceOps(das_solver* s) : dm(s->dm), prm(s->wk.bind(s->cp.solver, s->dm.nC, s->dm.nF, make_params(s->cp, s->opt, 0))), wk(s->wk), st(s->stream) {
        const long long N = dm.nC, F = dm.nF, nIF = dm.nIF, nBF = F - nIF;
        if (wk.fc.n != (size_t)DAS_FC_N * nIF) wk.fc.alloc((size_t)DAS_FC_N * nIF);
        if (wk.brec.n != (size_t)DAS_BREC_N * nBF) wk.brec.alloc((size_t)DAS_BREC_N * nBF);
        simple_alloc(v, s->n, N, F, nIF, [&](long long cnt) { return w.take(cnt); });
        v.W = s->d_W.p; v.Wp = v.W + prm.offP * N; v.WnNu = v.Wn + prm.offN * N; v.WnPhi = v.Wn + prm.offPhi * N;
        v.nut = wk.nut.p; v.gU = wk.gU.p; v.gP = wk.gP.p; v.gN = wk.gN.p; v.fc = wk.fc.p; v.brec = wk.brec.p;
    }
    template <class K, class... A>
    void launch(K k, long long cnt, A... a) { hipLaunchKernelGGL(k, dim3(nblk(cnt, 256)), dim3(256), 0, st, a...); }
    void ldu_mv(const SimpleLdu& A, const double* x, double* y, double sign) { launch(k_ldu_mv, v.N, dm, A.diag, A.up, A.lo, x, y, sign); }
    void lin(double* y, double a, const double* x, double b, const double* z) { launch(k_sv_lin, v.N, v.N, y, a, x, b, z); }
    void bicg_p(double* p, const double* r, double beta, double om, const double* vv) { launch(k_sv_bicg_p, v.N, v.N, p, r, beta, om, vv); }
    void divdiag(double* out, const double* in, const double* diag, double sign) { launch(k_sv_divdiag, v.N, v.N, out, in, diag, sign); }
    void bicg_x(double* x, double alpha, const double* ph, double om, const double* sh, double* r, const double* s, const double* t) { launch(k_sv_bicg_x, v.N, v.N, x, alpha, ph, om, sh, r, s, t); }
    double dot(const double* a, const double* b) { return sv_dot(st, w, v.N, a, b); }
    void copy(double* dst, const double* src, long long cnt) { DAS_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(double), hipMemcpyDeviceToDevice, st)); }
    void zero(double* x, long long cnt) { if (cnt) DAS_HIP(hipMemset(x, 0, cnt * sizeof(double))); }
    void grads_and_records(const double* W) {
        launch_grad_simple<double, double>(dm, prm, W, wk, st);
        if (v.nIF > 0) launch(k_fcoef<double>, v.nIF, dm, prm, W, v.nut, v.gU, v.gN, v.fc);
        if (v.F > v.nIF) launch(k_bcoef<double>, v.F - v.nIF, dm, prm, W, v.nut, v.gU, v.brec);
    }
    void ueqn() { launch(k_simple_ueqn, v.N, dm, prm, v.W, v.gP, v.fc, v.brec, v.D, v.bd, v.sb, v.rhsU); }
    void offdiag(const double* W, int cdIdx) { if (v.nIF > 0) launch(k_simple_offdiag, v.nIF, dm, prm, W, v.fc, cdIdx, v.up, v.lo); }
    void gather3(int k) { launch(k_sv_gather3, v.N, v.N, v.W, k, v.D, v.bd, v.rhsU, v.x, v.dg, v.b); }
    void scatter3(int k) { launch(k_sv_scatter3, v.N, v.N, v.x, k, v.Wn); }
    void hbya() { launch(k_simple_hbya, v.N, dm, v.Wn, v.D, v.bd, v.sb, v.up, v.lo, v.rAU, v.HbyA); }
    void pface() { launch(k_simple_pface, v.F, dm, prm, v.Wn, v.nut, v.rAU, v.HbyA, v.phiH, v.gpf, v.cp, v.pbc); }
    void peqn() { launch(k_simple_peqn, v.N, dm, v.phiH, v.gpf, v.cp, v.pbc, v.gPn, v.dp, v.rp); }
    void gradp() { launch(k_simple_gradp, v.N, dm, v.pn, v.pbc, v.gPn); }
    void flux() { launch(k_simple_flux, v.F, dm, v.pn, v.gPn, v.phiH, v.gpf, v.cp, v.pbc, v.phiN); }
    void relax(double alphaP) { launch(k_sv_relax, v.N, v.N, v.pn, v.Wp, alphaP); }
    void correct() { launch(k_simple_correct, v.N, v.N, prm.offP, v.HbyA, v.rAU, v.gPn, v.pn, v.Wn); }
    void saeqn() { launch(k_simple_saeqn, v.N, dm, prm, v.Wn, v.gU, v.gN, v.fc, v.brec, v.dg, v.b); }
    void bound() { launch(k_sv_bound, v.N, v.N, v.x, 1e-16, v.WnNu); }  // DAUtility::boundVar
};

// nSweeps SIMPLE iterations on the solver's states (DASimpleFoam + SA without T field, MRF, cyclic pairs; single rank).  alphaP: explicit
// pressure relaxation (fvSolution relaxationFactors.fields.p), linTol / maxLin: relative tolerance and iteration cap of the inner solves
// (the reference's fvSolution solvers; tight values reproduce the oracle's direct solves).  info[3] = inner iterations (U, p, nuTilda)
// of the last sweep.
static void run_simple_sweeps(das_solver* s, int nSweeps, double alphaP, double linTol, int maxLin, double* info) {
    need_init(s);
    DAS_CHECK(s->cp.solver != DAS_SOLVER_SOLIDDISPLACEMENTFOAM, DAS_ERR_ARG, "the SIMPLE sweeps are not built for DASolidDisplacementFoam (use das_solve_primal)");
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SIMPLEFOAM && !s->cp.hasT && !s->cp.mrf && !s->cp.hasCyclic, DAS_ERR_ARG,
              "SIMPLE sweeps serve DASimpleFoam + SA without T field, MRF and cyclic pairs");
    DAS_CHECK(!s->halo.active && !s->halo_cb && s->owned.empty(), DAS_ERR_ARG, "the SIMPLE sweeps are single-rank");
    SimpleDeviceOps ops(s);
    SimpleIters its;
    for (int sw = 0; sw < nSweeps; sw++) its = simple_sweep(ops, alphaP, linTol, maxLin, maxLin);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipStreamSynchronize(s->stream));
    s->h_W = s->d_W.to_host();
    if (info) { info[0] = its.U; info[1] = its.p; info[2] = its.nuTilda; }
}

int das_simple_iteration(das_solver_t* s, int nSweeps, double alphaP, double linTol, int maxLinIters, double* info3) {
    DAS_TRY
    DAS_CHECK(s && nSweeps >= 0 && alphaP > 0.0 && linTol > 0.0 && maxLinIters > 0, DAS_ERR_ARG, "das_simple_iteration: bad argument");
    DAS_CHECK(!s->cp.pimple, DAS_ERR_ARG, "DAPimpleFoam: simpleIteration is not built (the SIMPLE sweep is steady); use das_solve_primal per time step");
    DAS_CHECK(s->actuatorDisks.empty(), DAS_ERR_ARG,
              "das_simple_iteration: the SIMPLE sweep does not carry the fvSource actuator disks (its U equation has no source term); use das_solve_primal");
    DAS_CHECK(s->regModels.empty(), DAS_ERR_ARG,
              "das_simple_iteration: the SIMPLE sweep does not evaluate the regressionModel (its nuTilda equation reads no betaFINuTilda); use das_solve_primal");
    run_simple_sweeps(s, nSweeps, alphaP, linTol, maxLinIters, info3);
    return DAS_OK;
    DAS_CATCH
}

// solvePrimal (reference pyDASolvers.pyx solvePrimal -> DASimpleFoam::solvePrimal, DASimpleFoam.C:123-185): converge
// R(W) = 0 from the current states; returns 0 converged / 1 not converged; info4 = {steps, GMRES iterations, |R0|, |R|}
int das_solve_primal(das_solver_t* s, int maxSteps, double relTol, double absTol, double* info4, double* hist, int histCap) {
    DAS_TRY
    NewtonInfo inf;
    const int rc = run_newton_primal(s, maxSteps, relTol, absTol, inf);
    if (info4) { info4[0] = inf.steps; info4[1] = inf.linIters; info4[2] = inf.res0; info4[3] = inf.res; }
    if (hist) for (int i = 0; i < histCap && i < (int)inf.hist.size(); i++) hist[i] = inf.hist[i];
    return rc;
    DAS_CATCH
}
int das_run_coloring(das_solver_t* s) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    ensure_coloring(s);
    return DAS_OK;
    DAS_CATCH
}
// host-only profiling aid: factorise one local CSR exactly like a preconditioner block and report the phase times
int das_debug_factor_block(int nl, const long long* rp, const int* ci, const double* val, int lfill, double* tim4, long long* nnzLU,
                           int* nLevelsL, int* nLevelsU) {
    DAS_TRY
    DAS_CHECK(nl > 0 && rp && ci && val && tim4, DAS_ERR_ARG, "null argument");
    std::vector<long long> lrp(rp, rp + nl + 1), where;
    std::vector<int> lci(ci, ci + rp[nl]), lev;
    std::vector<double> lv(val, val + rp[nl]);
    BlockFactor F;
    for (int k = 0; k < 4; k++) tim4[k] = 0.0;
    factor_local(nl, lrp, lci, lv, lfill, F, where, lev, tim4);
    if (nnzLU) *nnzLU = (long long)F.fci.size();
    if (nLevelsL) *nLevelsL = (int)F.Llev.size() - 1;
    if (nLevelsU) *nLevelsU = (int)F.Ulev.size() - 1;
    return DAS_OK;
    DAS_CATCH
}
// host-only test aid: the recursive coordinate bisection (das_rcb.hpp) of n points, centres[3 * i + axis].  mode 0: param parts,
// out[i] = part of point i; mode 1: leaves of at most param points, out[i] = leaf of point i
int das_debug_rcb(int n, const double* centres, int mode, int param, int* out) {
    DAS_TRY
    DAS_CHECK(n >= 0 && (centres || n == 0) && (out || n == 0) && (mode == 0 || mode == 1) && param >= 1, DAS_ERR_ARG, "bad argument");
    std::vector<int> idx(n);
    std::iota(idx.begin(), idx.end(), 0);
    auto centre = [&](int i, int d) { return centres[3LL * i + d]; };
    if (mode == 0) {
        std::vector<int> partOf(n, -1);
        rcb_parts(idx, centre, param, partOf);
        std::copy(partOf.begin(), partOf.end(), out);
    } else {
        std::vector<long long> leafOff;
        rcb_leaves(idx, centre, param, leafOff);
        for (size_t l = 0; l + 1 < leafOff.size(); l++) for (long long q = leafOff[l]; q < leafOff[l + 1]; q++) out[idx[q]] = (int)l;
    }
    return DAS_OK;
    DAS_CATCH
}
int das_set_coloring(das_solver_t* s, const int* colors) {
    DAS_TRY
    DAS_CHECK(s && colors, DAS_ERR_ARG, "null argument");
    s->colored = false;
    ensure_coloring(s, colors);
    return DAS_OK;
    DAS_CATCH
}
int das_get_n_colors(das_solver_t* s, int isPC) {
    DAS_TRY
    DAS_CHECK(s && s->colored, DAS_ERR_STATE, "runColoring() has not been called");
    return s->nColors;
    DAS_CATCH
}
long long das_get_con_nnz(das_solver_t* s, int isPC) {
    try {
        DAS_CHECK(s && s->colored, DAS_ERR_STATE, "runColoring() has not been called");
        return isPC ? s->con_pc.nnz : s->con_full.nnz;
    } catch (const std::exception& e) { return fail(e); }
}
int das_get_con(das_solver_t* s, int isPC, long long* rowptr, int* colidx) {
    DAS_TRY
    DAS_CHECK(s && s->colored && rowptr && colidx, DAS_ERR_STATE, "runColoring() has not been called");
    const JacCon& j = isPC ? s->con_pc : s->con_full;
    std::copy(j.rowptr.begin(), j.rowptr.end(), rowptr);
    std::copy(j.col.begin(), j.col.end(), colidx);
    return DAS_OK;
    DAS_CATCH
}
int das_get_colors(das_solver_t* s, int isPC, int* colors) {
    DAS_TRY
    DAS_CHECK(s && s->colored && colors, DAS_ERR_STATE, "runColoring() has not been called");
    std::copy(s->colors.begin(), s->colors.end(), colors);
    return DAS_OK;
    DAS_CATCH
}

int das_calc_drdwt(das_solver_t* s, int isPC, int mode, das_mat_t** out) {
    DAS_TRY
    DAS_CHECK(out, DAS_ERR_ARG, "null output");
    DAS_CHECK(isPC == 0 || isPC == 1, DAS_ERR_ARG, "isPC not supported! Options are: 0 (for dRdWT) and 1 (for dRdWTPC).");
    DAS_CHECK(mode == 0 || mode == 1, DAS_ERR_ARG, "mode must be 0 (finite difference) or 1 (dual number)");
    *out = assemble(s, isPC, mode);
    return DAS_OK;
    DAS_CATCH
}
long long das_mat_rows(das_mat_t* m) { return m ? m->m.n : -1; }
long long das_mat_nnz(das_mat_t* m) { return m ? m->m.nnz : -1; }
int das_mat_export(das_mat_t* m, long long* rowptr, int* colidx, double* vals) {
    DAS_TRY
    DAS_CHECK(m && rowptr && colidx && vals, DAS_ERR_ARG, "null argument");
    m->m.rowptr.download(rowptr, m->m.n + 1);
    m->m.col.download(colidx, m->m.nnz);
    m->m.val.download(vals, m->m.nnz);
    return DAS_OK;
    DAS_CATCH
}
int das_mat_mult(das_mat_t* m, const double* x, double* y) {
    DAS_TRY
    DAS_CHECK(m && x && y, DAS_ERR_ARG, "null argument");
    DevBuf<double> dx(m->m.n), dy(m->m.n);
    dx.upload(x, m->m.n);
    launch_spmv(0, m->m.n, m->m.rowptr.p, m->m.col.p, m->m.val.p, VecPack(), dx.p, dy.p);  // the plain CSR product, whatever pack the matrix carries
    DAS_HIP(hipDeviceSynchronize());
    dy.download(y, m->m.n);
    return DAS_OK;
    DAS_CATCH
}
// a matrix read from a file (reference: PETSc.Mat().load of dRdWTPC.bin when adjEqnOption.readPCMat is set,
// mphys_dafoam.py:469-471,520-522) -> device CSR handle
int das_mat_create_from_csr(long long n, const long long* rowptr, const int* colidx, const double* vals, das_mat_t** out) {
    DAS_TRY
    DAS_CHECK(n > 0 && rowptr && colidx && vals && out, DAS_ERR_ARG, "bad argument");
    DAS_CHECK(das_device_count() > 0, DAS_ERR_NO_DEVICE, "no HIP device visible");
    std::unique_ptr<das_mat> m(new das_mat);
    m->m.n = n;
    m->m.nnz = rowptr[n];
    m->m.rowptr.upload(rowptr, n + 1);
    m->m.col.upload(colidx, m->m.nnz);
    m->m.val.upload(vals, m->m.nnz);
    *out = m.release();
    return DAS_OK;
    DAS_CATCH
}
void das_mat_destroy(das_mat_t* m) { delete m; }

int das_initialize_drdwt_matrix_free(das_solver_t* s) {
    DAS_TRY
    need_init(s);
    s->op.reset(assemble(s, 0, (int)s->opt.geti("amd.jacMode")));
    s->opId++;
    // the Krylov operator: vector-state rows repacked as group rows (das_opmat.hpp); amd.opPackVector 0 keeps the plain CSR
    {
        const StateDef& s0 = s->st_full.states[0];
        if (s->opt.geti_or("amd.opPackVector", 1) != 0 && s0.kind == KIND_VEC) {
            Mat& M = s->op->m;
            const bool ok = vecpack_build(M.vp, s0.size / 3, s0.offset, M.rowptr.p, M.col.p, M.val.p, s->stream);
            if (s->opt.geti("debug"))
                fprintf(stderr, "[dafoam_amd] operator vector rows %s: %lld group rows, %lld chunks, %.2f GB\n",
                        ok ? "packed" : "NOT packed (rows of a cell differ)", M.vp.nGroups, M.vp.nChunks, M.vp.bytes() / 1e9);
        }
    }
    s->op_states = s->h_W;
    s->op_geom = s->geomVersion;
    s->op_epoch = s->opEpoch;
    return DAS_OK;
    DAS_CATCH
}
int das_destroy_drdwt_matrix_free(das_solver_t* s) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    s->op.reset();
    s->opId++;
    return DAS_OK;
    DAS_CATCH
}

int das_calc_drdwold_t_psi(das_solver_t* s, int oldTimeLevel, const double* psi, double* out) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(psi && out, DAS_ERR_ARG, "null argument");
    DAS_CHECK(oldTimeLevel == 1 || oldTimeLevel == 2, DAS_ERR_ARG, "oldTimeLevel must be 1 (W0) or 2 (W00)");
    const long long n = s->n;
    if (s->cp.pimple) {
        double c, c0, c00;
        s->cp.ddt_coeffs(c, c0, c00);
        const double coef = (oldTimeLevel == 1 ? c0 : -c00) / s->cp.deltaT;
        if (coef == 0.0) {  // Euler, or backward below time index 2: no W00 in the residual
            std::fill(out, out + n, 0.0);
            return DAS_OK;
        }
        // rAU of the current states: one residual pass (its R goes to the scratch), kept for as long as the states, the geometry, the
        // options and the old-time states stand - level 2 of an adjoint step reuses the pass of level 1; then the gather
        hipStream_t st = s->stream;
        ResParams prm = make_params(s->cp, s->opt, 0);
        const bool kept = s->d_rAUold.n == (size_t)s->dm.nC && s->rAUold_epoch == s->opEpoch && s->rAUold_geom == s->geomVersion &&
                          s->rAUold_states.size() == s->h_W.size() && std::memcmp(s->rAUold_states.data(), s->h_W.data(), n * sizeof(double)) == 0;
        if (!kept) {
            eval_residual<double>(s->dm, s->cp, prm, s->d_W.p, s->d_tmp2.p, s->wk, s->d_phiF.p, s->d_Told.p, st);
            if (s->d_rAUold.n != (size_t)s->dm.nC) s->d_rAUold.alloc(s->dm.nC);
            DAS_HIP(hipMemcpyAsync(s->d_rAUold.p, s->wk.rAU.p, (size_t)s->dm.nC * sizeof(double), hipMemcpyDeviceToDevice, st));
            s->rAUold_states = s->h_W;
            s->rAUold_epoch = s->opEpoch;
            s->rAUold_geom = s->geomVersion;
        }
        DAS_HIP(hipMemcpyAsync(s->d_tmp1.p, psi, n * sizeof(double), hipMemcpyHostToDevice, st));
        DAS_HIP(hipMemsetAsync(s->d_tmp2.p, 0, n * sizeof(double), st));
        hipLaunchKernelGGL(k_drdwold, dim3(nblk(s->dm.nC, 256)), dim3(256), 0, st, s->dm, prm, coef, (const double*)s->d_rAUold.p, (const double*)s->d_tmp1.p,
                           (const double*)s->d_scale.p, s->d_tmp2.p);
        DAS_HIP(hipGetLastError());
        DAS_HIP(hipMemcpyAsync(out, s->d_tmp2.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
        DAS_HIP(hipStreamSynchronize(st));
        return DAS_OK;
    }
    if (s->cp.solver != DAS_SOLVER_SCALARTRANSPORTFOAM || oldTimeLevel == 2) {
        std::fill(out, out + n, 0.0);  // steady residuals / Euler scheme: no W00 dependence
        return DAS_OK;
    }
    // R_i = ((V/dt)(T_i - T0_i) + ...)/V (normalised) -> dR_i/dT0_j = -delta_ij/dt (x V if TRes is not normalised)
    DAS_HIP(hipMemcpyAsync(s->d_tmp1.p, psi, n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    std::vector<double> coef(n);
    const bool norm = s->opt.list_has("normalizeResiduals", "TRes");
    for (long long j = 0; j < n; j++) coef[j] = -s->h_scale[j] / s->cp.deltaT * (norm ? 1.0 : s->mesh.cg[j].V);
    s->d_tmp2.upload(coef);
    hipLaunchKernelGGL(k_mul, dim3(nblk(n, 256)), dim3(256), 0, s->stream, n, s->d_tmp2.p, s->d_tmp1.p);
    DAS_HIP(hipMemcpyAsync(out, s->d_tmp1.p, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return DAS_OK;
    DAS_CATCH
}
int das_set_old_time_states(das_solver_t* s, const double* W0, const double* W00, int timeIndex) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    DAS_CHECK(s->cp.pimple, DAS_ERR_ARG, "old-time states only exist for DAPimpleFoam");
    DAS_CHECK(W0, DAS_ERR_ARG, "null W0");
    DAS_CHECK(timeIndex >= 1, DAS_ERR_ARG, "timeIndex counts the time steps from 1, not " + std::to_string(timeIndex));
    DAS_CHECK(W00 || !(s->cp.ddtScheme == 1 && timeIndex >= 2), DAS_ERR_ARG, "the backward scheme at time index " + std::to_string(timeIndex) + " needs W00");
    s->cp.timeIndex = timeIndex;
    s->h_W0.assign(W0, W0 + s->n);
    if (W00) s->h_W00.assign(W00, W00 + s->n);
    if (s->inited) {
        s->d_W0.upload(s->h_W0); s->cp.W0_ptr = s->d_W0.p;
        if (W00) { s->d_W00.upload(s->h_W00); s->cp.W00_ptr = s->d_W00.p; }
    }
    s->opEpoch++;
    return DAS_OK;
    DAS_CATCH
}
int das_set_time_index(das_solver_t* s, int timeIndex) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    DAS_CHECK(s->cp.pimple, DAS_ERR_ARG, "the time index only selects ddt coefficients for DAPimpleFoam");
    DAS_CHECK(timeIndex >= 1, DAS_ERR_ARG, "timeIndex counts the time steps from 1, not " + std::to_string(timeIndex));
    if (s->cp.timeIndex != timeIndex) {
        s->cp.timeIndex = timeIndex;
        s->opEpoch++;
    }
    return DAS_OK;
    DAS_CATCH
}
int das_set_old_time_fields(das_solver_t* s, const double* phi_frozen, const double* T_old) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SCALARTRANSPORTFOAM, DAS_ERR_ARG, "old-time fields only exist for DAScalarTransportFoam");
    if (phi_frozen) s->cp.phi_frozen.assign(phi_frozen, phi_frozen + s->mesh.nF);
    if (T_old) s->cp.T_old.assign(T_old, T_old + s->mesh.nC);
    if (s->inited) { s->d_phiF.upload(s->cp.phi_frozen); s->d_Told.upload(s->cp.T_old); }
    s->opEpoch++;
    return DAS_OK;
    DAS_CATCH
}

// ---- shared by the host paths of the objective functions ----------------------------------------------------------------------
extern "C++" {  // templates: not under the C linkage of the entry points around them
// f with the compressible switch as a compile-time tag: f(SolverTag<true, false>{}) or f(SolverTag<false, false>{})
template <bool RHO, bool SOLID>
struct SolverTag { static constexpr bool value = RHO, solid = SOLID; };  // value: the compressible switch; solid: DAHeatTransferFoam's layout [T]
template <class F>
static void with_rho(bool rho, F&& f) {
    if (rho) f(SolverTag<true, false>{});
    else f(SolverTag<false, false>{});
}
// the two launches of a function pass: the gradient fields of W into wk (k_grad; not for location, which reads no state: grad = false),
// then the per-face kernel - `face` launches it and takes the same tag
template <class T, class G, class F>
static void launch_grad_and_faces(hipStream_t st, bool rho, const DevMeshT<G>& dm, const ResParams& prm, const T* W, ResWork<T>& wk, bool grad, F&& face) {
    if (prm.solid) {  // DAHeatTransferFoam: the face functions read T of the owner cell and the patch field - no gradient pass
        face(SolverTag<false, true>{});
        return;
    }
    with_rho(rho, [&](auto R) {
        if (grad) hipLaunchKernelGGL((k_grad<T, decltype(R)::value, G>), dim3(nblk(dm.nC, 256)), dim3(256), 0, st, dm, prm, W, wk.nut.p, wk.gU.p, wk.gP.p, wk.gN.p, wk.gH.p);
        face(R);
    });
}
}  // extern "C++"
// calcRefVar (DAFunction::calcRefVar): F = (F0 - ref)^2, dF/dF0 = 2 (F0 - ref); without it F = F0
static double ref_var_value(bool refVar, double ref, double F0) { return refVar ? (F0 - ref) * (F0 - ref) : F0; }
static double ref_var_outer(bool refVar, double ref, double F0) { return refVar ? 2.0 * (F0 - ref) : 1.0; }
static void need_flow_solver(das_solver* s) {
    DAS_CHECK(s->cp.solver != DAS_SOLVER_SOLIDDISPLACEMENTFOAM, DAS_ERR_ARG,
              "face functions and coupling outputs are not built for DASolidDisplacementFoam (variableVolSum of D is)");
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SIMPLEFOAM || DAS_IS_COMPRESSIBLE(s->cp.solver), DAS_ERR_ARG, "function needs a flow solver");
}
// the derivative passes of a face function that is already defined: the flow solvers, and DAHeatTransferFoam (wallHeatFlux, thermal coupling)
static void need_face_function_solver(das_solver* s) {
    if (s->cp.solver != DAS_SOLVER_HEATTRANSFERFOAM) need_flow_solver(s);
}

// geometry-dependent part of a face function: per-face weights (scale, area fractions) and directions (moment arms)
static void build_function_geometry(das_solver* s, das_solver::FaceFn& fn) {
    const size_t nf = fn.faces.size();
    double area[2] = {0.0, 0.0};
    for (size_t k = 0; k < nf; k++) area[fn.group[k]] += s->mesh.fg[fn.faces[k]].magSf;
    DAS_CHECK(!fn.ratio || (area[0] > 0 && area[1] > 0), DAS_ERR_ARG, "inlet/outletPatches names are not in patches");
    fn.w0.resize(nf);
    if (fn.kind == DAS_FN_FORCE) fn.dir.resize(3 * nf);
    for (size_t k = 0; k < nf; k++) {
        const FaceGeom& g = s->mesh.fg[fn.faces[k]];
        if (fn.kind == DAS_FN_FORCE) {
            if (!fn.isMoment) for (int d = 0; d < 3; d++) fn.dir[3 * k + d] = fn.vecA[d];
            else {  // (r x F) . axis = F . (axis x r),  r = Cf - center
                const double r[3] = {g.Cf[0] - fn.vecB[0], g.Cf[1] - fn.vecB[1], g.Cf[2] - fn.vecB[2]};
                fn.dir[3 * k] = fn.vecA[1] * r[2] - fn.vecA[2] * r[1];
                fn.dir[3 * k + 1] = fn.vecA[2] * r[0] - fn.vecA[0] * r[2];
                fn.dir[3 * k + 2] = fn.vecA[0] * r[1] - fn.vecA[1] * r[0];
            }
            fn.w0[k] = fn.scale;
        } else if (fn.kind == DAS_FN_MASSFLOW) fn.w0[k] = fn.scale;
        else if (fn.kind == DAS_FN_TOTALPRESSURE) fn.w0[k] = fn.scale * g.magSf / area[0];  // area average, DAFunctionTotalPressure.C:77
        else if (DAS_FN_BASE(fn.kind) == DAS_FN_PATCHMEAN) fn.w0[k] = fn.scale * g.magSf / area[0];  // DAFunctionPatchMean.C:55-80
        else if (DAS_FN_BASE(fn.kind) == DAS_FN_VARIANCE)  // DAFunctionVariance.C: geoWeightTotal adds |Sf| once per component
            fn.w0[k] = !fn.hasData ? 0.0 : fn.geoWeight ? fn.scale * g.magSf / (fn.ncomp * area[0]) : fn.scale / (double)(fn.ncomp * nf);
        else if (DAS_FN_BASE(fn.kind) == DAS_FN_WALLHEATFLUX)  // DAFunctionWallHeatFlux.C:264-295: area average, or the total through the surface
            fn.w0[k] = fn.byUnitArea ? fn.scale * g.magSf / area[0] : fn.scale * g.magSf;
        else if (DAS_FN_BASE(fn.kind) == DAS_FN_LOCATION) fn.w0[k] = 1.0;  // the value pass stores a_f itself
        else fn.w0[k] = g.magSf / area[fn.group[k]];                                          // TTIn / TTOut, TPIn / TPOut area averages
    }
    fn.geomVersion = s->geomVersion;
    fn.uploaded = false;
}

// the faces of the patches, in patch order -> fn.faces / fn.group (group 1: patch_group[k] != 0; all 0 when patch_group is null)
static void collect_patch_faces(das_solver* s, const int* patch_ids, const int* patch_group, int npatch, das_solver::FaceFn& fn) {
    for (int k = 0; k < npatch; k++) {
        const int p = patch_ids[k];
        DAS_CHECK(p >= 0 && p < s->mesh.nPatch, DAS_ERR_ARG, "patch id out of range");
        DAS_CHECK(s->mesh.patch_type[p] != DAS_PATCH_CYCLIC, DAS_ERR_ARG, "functions cannot be defined on cyclic patches");
        const unsigned char grp = (patch_group && patch_group[k]) ? 1 : 0;
        for (int q = 0; q < s->mesh.patch_size[p]; q++) {
            fn.faces.push_back(s->mesh.patch_start[p] + q);
            fn.group.push_back(grp);
        }
    }
}
// the tail of every face-function definition; needFaces: an empty face list is an error that names the function
static void register_face_function(das_solver* s, const char* name, das_solver::FaceFn&& fn, bool needFaces) {
    DAS_CHECK(!needFaces || !fn.faces.empty(), DAS_ERR_ARG, "the patches of function " + std::string(name) + " have no faces");
    build_function_geometry(s, fn);
    s->cellFunctions.erase(name);
    s->meshFunctions.erase(name);
    s->functions[name] = std::move(fn);
}

// ---- objective functions (reference "function" option dict).  Face functions (das_define_face_function[_ex]): DAFunctionForce,
//      DAFunctionMoment, DAFunctionMassFlowRate, DAFunctionTotalPressure, DAFunctionTotalTemperatureRatio, DAFunctionTotalPressureRatio,
//      DAFunctionWallHeatFlux; das_define_location_function: DAFunctionLocation; das_define_patch_field_function / das_define_cell_function:
//      DAFunctionPatchMean, DAFunctionVariance, DAFunctionVariableVolSum -------------------------------------------------------------
int das_define_face_function(das_solver_t* s, const char* name, const char* type, const int* patch_ids, const int* patch_group, int npatch,
                             const double* vecA, const double* vecB, double scale, double gammaFn) {
    return das_define_face_function_ex(s, name, type, patch_ids, patch_group, npatch, vecA, vecB, scale, gammaFn, 1, 0.0);
}
int das_define_face_function_ex(das_solver_t* s, const char* name, const char* type, const int* patch_ids, const int* patch_group, int npatch,
                                const double* vecA, const double* vecB, double scale, double gammaFn, int flags, double ref) {
    DAS_TRY
    DAS_CHECK(s && name && type && patch_ids && npatch > 0, DAS_ERR_ARG, "bad argument");
    const std::string ty = type;
    if (s->cp.solver == DAS_SOLVER_HEATTRANSFERFOAM) {  // the solid: kappa(T_b) snGrad(T) on the one-block layout (body_facefn_solid)
        DAS_CHECK(ty == "wallHeatFlux", DAS_ERR_ARG, "function type " + ty + " (function " + name + ") is not built for DAHeatTransferFoam; wallHeatFlux and variableVolSum of T are");
        DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "DAHeatTransferFoam functions run on an undecomposed solver (sharded solvers are not supported)");
        das_solver::FaceFn fn;
        fn.kind = DAS_FN_WALLHEATFLUX | ((flags & 2) ? DAS_FN_ALT_BIT : 0);
        fn.byUnitArea = (flags & 1) != 0;
        collect_patch_faces(s, patch_ids, nullptr, npatch, fn);
        fn.scale = scale;
        fn.refVar = (flags & 8) != 0;
        fn.ref = ref;
        register_face_function(s, name, std::move(fn), false);
        return DAS_OK;
    }
    DAS_CHECK(ty != "wallHeatFlux" || DAS_IS_COMPRESSIBLE(s->cp.solver) || (s->cp.solver == DAS_SOLVER_SIMPLEFOAM && s->cp.hasT), DAS_ERR_ARG,
              std::string("wallHeatFlux function ") + name + " needs a T field (DASimpleFoam with T, DARhoSimpleFoam, DATurboFoam)");
    need_flow_solver(s);
    das_solver::FaceFn fn;
    if (ty == "force" || ty == "moment") fn.kind = DAS_FN_FORCE;
    else if (ty == "massFlowRate") fn.kind = DAS_FN_MASSFLOW;
    else if (ty == "totalPressure") fn.kind = DAS_FN_TOTALPRESSURE;
    else if (ty == "totalTemperatureRatio") { fn.kind = DAS_FN_TOTALTEMPERATURE; fn.ratio = true; }
    else if (ty == "totalPressureRatio") { fn.kind = DAS_FN_TOTALPRESSURERATIO; fn.ratio = true; }
    else if (ty == "wallHeatFlux") { fn.kind = DAS_FN_WALLHEATFLUX | ((flags & 2) ? DAS_FN_ALT_BIT : 0); fn.byUnitArea = (flags & 1) != 0; }
    else throw Error(DAS_ERR_ARG, "function type not implemented on the GPU path: " + ty);
    if (fn.kind == DAS_FN_FORCE) {
        DAS_CHECK(vecA, DAS_ERR_ARG, "force / moment need a direction / axis");
        const double mag = std::sqrt(vecA[0] * vecA[0] + vecA[1] * vecA[1] + vecA[2] * vecA[2]);
        // reference DAFunctionForce.C:60-66 / DAFunctionMoment.C: the direction (axis) has unit length
        DAS_CHECK(std::fabs(mag - 1.0) <= 1.0e-8, DAS_ERR_ARG, std::string("the magnitude of the direction parameter in ") + name + " is not 1.0!");
        DAS_CHECK(ty == "force" || vecB, DAS_ERR_ARG, "moment needs a center");
    }
    if (fn.ratio) {
        DAS_CHECK(DAS_IS_COMPRESSIBLE(s->cp.solver), DAS_ERR_ARG, ty + " needs a compressible solver");
        DAS_CHECK(patch_group, DAS_ERR_ARG, ty + " needs the inlet (0) / outlet (1) group of every patch");
        DAS_CHECK(gammaFn > 1.0, DAS_ERR_ARG, ty + " needs gamma > 1");
        fn.gammaFn = gammaFn;
        fn.RFn = s->cp.Cp - s->cp.Cp / gammaFn;  // DAFunctionTotalTemperatureRatio.C:98
    }
    collect_patch_faces(s, patch_ids, fn.ratio ? patch_group : nullptr, npatch, fn);
    fn.isMoment = ty == "moment";
    fn.scale = fn.kind == DAS_FN_TOTALPRESSURERATIO ? 1.0 : scale;  // DAFunctionTotalPressureRatio.C applies no scale
    // calcRefVar (DAFunction::calcRefVar) of the kinds this entry adds; the earlier kinds keep their meaning under das_define_face_function
    fn.refVar = (flags & 8) && (fn.kind == DAS_FN_TOTALPRESSURERATIO || DAS_FN_BASE(fn.kind) == DAS_FN_WALLHEATFLUX);
    fn.ref = ref;
    for (int d = 0; d < 3; d++) { fn.vecA[d] = vecA ? vecA[d] : 0.0; fn.vecB[d] = vecB ? vecB[d] : 0.0; }
    register_face_function(s, name, std::move(fn), false);  // no faces: defined all the same, as before the entry points shared this tail
    return DAS_OK;
    DAS_CATCH
}
// location (reference DAFunctionLocation.C): mode maxRadiusKS / maxInverseRadiusKS / maxRadius over the faces of the patches.  The axis is
// normalised here (:40-46).  maxRadius keeps the ONE face that has the largest radius now (the first on ties, :83-126); a later
// das_update_of_mesh does not choose again.  flags & 8: calcRefVar.  No scale is applied (:153-295).
int das_define_location_function(das_solver_t* s, const char* name, const char* mode, const int* patch_ids, int npatch, const double* axis,
                                 const double* center, double coeffKS, int flags, double ref) {
    DAS_TRY
    DAS_CHECK(s && name && mode && patch_ids && npatch > 0 && axis && center, DAS_ERR_ARG, "bad argument");
    need_flow_solver(s);
    const std::string md = mode;
    DAS_CHECK(md == "maxRadiusKS" || md == "maxInverseRadiusKS" || md == "maxRadius", DAS_ERR_ARG,
              "mode: " + md + " not supported! Options are: maxRadiusKS, maxInverseRadiusKS, maxRadius");
    const double mag = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    DAS_CHECK(mag > 0.0, DAS_ERR_ARG, std::string("the axis of location function ") + name + " has zero length");
    das_solver::FaceFn fn;
    fn.kind = DAS_FN_LOCATION | (md == "maxInverseRadiusKS" ? DAS_FN_ALT_BIT : 0);
    fn.ks = md != "maxRadius";
    fn.coeffKS = coeffKS;
    DAS_CHECK(!fn.ks || coeffKS != 0.0, DAS_ERR_ARG, std::string("coeffKS of location function ") + name + " is zero");
    for (int d = 0; d < 3; d++) { fn.loc[d] = axis[d] / mag; fn.loc[3 + d] = center[d]; }
    fn.refVar = (flags & 8) != 0;
    fn.ref = ref;
    collect_patch_faces(s, patch_ids, nullptr, npatch, fn);
    if (!fn.ks) {  // maxRadius: of the collected faces, the first of the largest radius
        int best = -1;
        double maxR = -100000.0;
        for (int f : fn.faces) {
            const double r = location_radius<double>(s->mesh.fg[f], fn.loc, false);
            if (r > maxR) { maxR = r; best = f; }
        }
        fn.faces.clear();
        if (best >= 0) fn.faces.push_back(best);
        fn.group.resize(fn.faces.size());
    }
    register_face_function(s, name, std::move(fn), true);
    return DAS_OK;
    DAS_CATCH
}
int das_define_force_function(das_solver_t* s, const char* name, const int* patch_ids, int npatch, const double* direction, double scale) {
    return das_define_face_function(s, name, "force", patch_ids, nullptr, npatch, direction, nullptr, scale, 0.0);
}
// ---- field-valued objectives (reference DAFunctionVariableVolSum.C, DAFunctionPatchMean.C, DAFunctionVariance.C) ----------
// variable id of a cell state (0 U, 1 p, 2 nuTilda, 3 T) and whether this solver has it; "betaFINuTilda" is 4 (cell sets only)
static int field_var_id(das_solver* s, const char* var, bool allowField) {
    const std::string v = var ? var : "";
    const bool flow = s->cp.solver == DAS_SOLVER_SIMPLEFOAM || DAS_IS_COMPRESSIBLE(s->cp.solver);
    const bool hasT = DAS_IS_COMPRESSIBLE(s->cp.solver) || s->cp.hasT || s->cp.solver == DAS_SOLVER_SCALARTRANSPORTFOAM || s->cp.solver == DAS_SOLVER_HEATTRANSFERFOAM;
    const std::string supported = std::string(flow ? "U, p, nuTilda" : "") + (hasT ? (flow ? ", T" : "T") : "") + (allowField && flow ? ", betaFINuTilda" : "");
    int id = -1;
    if (s->cp.solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM) {  // the one vector state D sits where U sits in the flow layouts
        DAS_CHECK(v == "D" || (v == "solid:rho" && allowField), DAS_ERR_ARG,
                  "varName " + v + " is not supported by DASolidDisplacementFoam; supported: D" + (allowField ? ", solid:rho" : ""));
        return v == "D" ? 0 : 4;  // solid:rho: the uniform density, a source no state reaches (the slot of the `field` sources)
    }
    if (v == "U" && flow) id = 0;
    else if (v == "p" && flow) id = 1;
    else if (v == "nuTilda" && flow) id = 2;
    else if (v == "T" && hasT) id = 3;
    else if (v == "betaFINuTilda" && flow && allowField) id = 4;
    DAS_CHECK(!(id == 4 && !s->regModels.empty()), DAS_ERR_ARG,
              "varName betaFINuTilda: a regressionModel is active and writes betaFINuTilda from the states in every residual evaluation; an objective over it "
              "would depend on the states, which is not built");
    DAS_CHECK(id >= 0, DAS_ERR_ARG, "varName " + v + " is not supported by this solver; supported: " + supported);
    return id;
}
static void check_comps(int vid, const int* comps, int ncomp) {
    DAS_CHECK(comps && ncomp >= 1 && ncomp <= 3, DAS_ERR_ARG, "1 to 3 components expected");
    int mask = 0;
    for (int i = 0; i < ncomp; i++) {
        DAS_CHECK(comps[i] >= 0 && comps[i] < (vid == 0 ? 3 : 1), DAS_ERR_ARG, "component index out of range for this varType");
        DAS_CHECK(!((mask >> comps[i]) & 1), DAS_ERR_ARG, "repeated component index");
        mask |= 1 << comps[i];
    }
}
int das_define_patch_field_function(das_solver_t* s, const char* name, const char* type, const int* patch_ids, int npatch, const char* var,
                                    const int* comps, int ncomp, const double* data, int flags, double scale, double ref) {
    DAS_TRY
    DAS_CHECK(s && name && type && patch_ids && npatch > 0, DAS_ERR_ARG, "bad argument");
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "patchMean / variance functions run on an undecomposed solver");
    need_flow_solver(s);
    const std::string ty = type;
    DAS_CHECK(ty == "patchMean" || ty == "variance", DAS_ERR_ARG, "patch field function type not valid: " + ty);
    const int vid = field_var_id(s, var, false);
    check_comps(vid, comps, ncomp);
    DAS_CHECK(ty == "variance" || ncomp == 1, DAS_ERR_ARG, "patchMean takes one component");
    das_solver::FaceFn fn;
    int mask = 0;
    for (int i = 0; i < ncomp; i++) mask |= 1 << comps[i];
    fn.kind = DAS_FN_FIELD_KIND(ty == "patchMean" ? DAS_FN_PATCHMEAN : DAS_FN_VARIANCE, vid, mask);
    collect_patch_faces(s, patch_ids, nullptr, npatch, fn);
    fn.scale = scale;
    fn.refVar = ty == "patchMean" && (flags & 8);
    fn.ref = ref;
    fn.geoWeight = (flags & 16) != 0;
    fn.ncomp = ncomp;
    if (ty == "variance") {  // the reference values of face k go into its direction slot: dir[3 k + component]
        fn.hasData = data != nullptr;
        fn.dir.assign(3 * fn.faces.size(), 0.0);
        if (data)
            for (size_t k = 0; k < fn.faces.size(); k++)
                for (int i = 0; i < ncomp; i++) fn.dir[3 * k + comps[i]] = data[k * ncomp + i];
    }
    register_face_function(s, name, std::move(fn), true);
    return DAS_OK;
    DAS_CATCH
}
int das_define_cell_function(das_solver_t* s, const char* name, const char* type, const int* cells, int ncells, const char* var, const int* comps,
                             int ncomp, const double* data, int flags, double scale, double ref) {
    DAS_TRY
    DAS_CHECK(s && name && type && (cells || ncells == 0) && ncells >= 0, DAS_ERR_ARG, "bad argument");
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "variableVolSum / variance functions run on an undecomposed solver");
    const std::string ty = type;
    DAS_CHECK(ty == "variableVolSum" || ty == "variance", DAS_ERR_ARG, "cell function type not valid: " + ty);
    DAS_CHECK(s->cp.solver != DAS_SOLVER_SOLIDDISPLACEMENTFOAM || ty == "variableVolSum", DAS_ERR_ARG,
              "function type " + ty + " (function " + name + ") is not built for DASolidDisplacementFoam; variableVolSum of D is");
    const int vid = field_var_id(s, var, ty == "variableVolSum");
    check_comps(vid, comps, ncomp);
    DAS_CHECK(ty == "variance" || ncomp == 1, DAS_ERR_ARG, "variableVolSum takes one component");
    das_solver::CellFn fn;
    fn.variance = ty == "variance";
    fn.field = vid == 4;
    fn.constSrc = fn.field && s->cp.solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM;
    fn.square = fn.variance || (flags & 1);
    fn.multiplyVol = fn.variance ? (flags & 16) != 0 : (flags & 2) != 0;
    fn.divByTotalVol = !fn.variance && (flags & 4);
    fn.refVar = !fn.variance && (flags & 8);
    fn.geoWeight = fn.variance && (flags & 16);
    fn.hasData = !fn.variance || data != nullptr;
    fn.scale = scale;
    fn.ref = ref;
    const ResParams prm = make_params(s->cp, s->opt, 0);
    const long long N = s->mesh.nC;
    const long long off = vid == 1 ? prm.offP * N : vid == 2 ? prm.offN * N : vid == 3 ? prm.offT * N : 0;
    for (int k = 0; k < ncells; k++) {
        const int c = cells[k];
        DAS_CHECK(c >= 0 && c < s->mesh.nC, DAS_ERR_ARG, "cell index out of range");
        for (int i = 0; i < ncomp; i++) {
            fn.cell.push_back(c);
            fn.idx.push_back(vid == 0 ? 3LL * c + comps[i] : off + c);
        }
    }
    {  // one term per state: the gradient scatter stores without collisions
        std::vector<unsigned char> seen(N, 0);
        for (int k = 0; k < ncells; k++) { DAS_CHECK(!seen[cells[k]], DAS_ERR_ARG, "repeated cell in the cell set"); seen[cells[k]] = 1; }
    }
    if (fn.variance && data) fn.data.assign(data, data + fn.cell.size());
    s->functions.erase(name);
    s->meshFunctions.erase(name);
    s->cellFunctions[name] = std::move(fn);
    return DAS_OK;
    DAS_CATCH
}
int das_define_von_mises_function(das_solver_t* s, const char* name, const int* cells, int ncells, double scale, double coeffKS, int flags, double ref) {
    DAS_TRY
    DAS_CHECK(s && name && cells && ncells > 0, DAS_ERR_ARG, "vonMisesStressKS: a non-empty cell set is expected");
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM, DAS_ERR_ARG,
              std::string("function type vonMisesStressKS (function ") + name + ") is built for DASolidDisplacementFoam only");
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "vonMisesStressKS runs on an undecomposed solver (sharded solvers are not supported)");
    DAS_CHECK(coeffKS != 0.0, DAS_ERR_ARG, std::string("coeffKS of vonMisesStressKS function ") + name + " is zero");
    das_solver::CellFn fn;
    fn.vmKS = true;
    fn.coeffKS = coeffKS;
    fn.scale = scale;
    fn.refVar = (flags & 8) != 0;
    fn.ref = ref;
    std::vector<unsigned char> seen(s->mesh.nC, 0);
    for (int k = 0; k < ncells; k++) {
        const int c = cells[k];
        DAS_CHECK(c >= 0 && c < s->mesh.nC, DAS_ERR_ARG, "cell index out of range");
        DAS_CHECK(!seen[c], DAS_ERR_ARG, "repeated cell in the cell set");
        seen[c] = 1;
        fn.cell.push_back(c);
        fn.idx.push_back(3LL * c);
    }
    s->functions.erase(name);
    s->meshFunctions.erase(name);
    s->cellFunctions[name] = std::move(fn);
    return DAS_OK;
    DAS_CATCH
}
static das_solver::CellFn* find_cell_function(das_solver* s, const char* name) {
    auto it = s->cellFunctions.find(name ? name : "");
    if (it == s->cellFunctions.end()) return nullptr;
    das_solver::CellFn& fn = it->second;
    if (fn.geomVersion != s->geomVersion) {  // the cell set is fixed; its weights follow the metrics
        const Mesh& m = s->mesh;
        double norm = 1.0;
        if (fn.variance) {
            norm = (double)fn.cell.size();
            if (fn.geoWeight) { norm = 0.0; for (int c : fn.cell) norm += m.cg[c].V; }
        } else if (fn.divByTotalVol) {
            for (int c = 0; c < m.nC; c++) norm += m.cg[c].V;  // totalVol starts at 1 (DAFunctionVariableVolSum.C:60-70)
        }
        fn.totalVol = norm;
        fn.coef = (!fn.hasData || fn.cell.empty()) ? 0.0 : fn.scale / norm;
        fn.geomVersion = s->geomVersion;
    }
    if (!fn.uploaded && s->inited) {
        fn.d_cell.upload(fn.cell);
        fn.d_idx.upload(fn.idx);
        if (!fn.data.empty()) fn.d_data.upload(fn.data);
        fn.d_part.alloc(DAS_CELLFN_MAX_BLOCKS);
        fn.uploaded = true;
    }
    return &fn;
}
// the values the terms read: the states or the betaFINuTilda field (1 everywhere until das_set_field; the solver's field state
// is left as it is)
static const double* cell_function_src(das_solver* s, das_solver::CellFn& fn) {
    if (!fn.field) return s->d_W.p;
    if (!fn.constSrc && !s->cp.beta_fi.empty()) return s->d_betaFI.p;
    if (fn.d_unit.n != (size_t)s->mesh.nC) fn.d_unit.upload(std::vector<double>(s->mesh.nC, fn.constSrc ? s->cp.solidRho : 1.0));
    return fn.d_unit.p;
}
// vonMisesStressKS: gradD of the residual pass (traction passes included) into s->wk.gU, vm of the terms into fn.d_a, then the
// max-shifted two-stage KS sum of das_facefn.hpp; {m, S} stay in fn.d_ks for the weights.  F0 = (m + log S) / coeffKS.  The reference
// aborts when its plain sum of exponentials passes 1e200; the log-space sum has no such limit and none is imposed (wider than the reference).
static double vm_ks_value(das_solver* s, das_solver::CellFn& fn) {
    const long long nt = (long long)fn.cell.size();
    DAS_CHECK(nt > 0, DAS_ERR_ARG, "vonMisesStressKS: the cell set is empty");
    const ResParams prm = s->wk.bind(s->cp.solver, s->dm.nC, s->dm.nF, make_params(s->cp, s->opt, 0));
    launch_solid_grad<double, double>(s->dm, prm, (const double*)s->d_W.p, s->wk, s->stream);
    if (fn.d_ks.n != 2) fn.d_ks.alloc(2);
    if (fn.d_kpart.n != DAS_FACEFN_MAX_BLOCKS) fn.d_kpart.alloc(DAS_FACEFN_MAX_BLOCKS);
    if (fn.d_a.n != (size_t)nt) { fn.d_a.alloc(nt); fn.d_wt.alloc(nt); }
    if (fn.d_wc.n != (size_t)s->mesh.nC) fn.d_wc.alloc(s->mesh.nC);
    hipLaunchKernelGGL(k_vm_terms, dim3(nblk(nt, 256)), dim3(256), 0, s->stream, nt, (const int*)fn.d_cell.p, prm, (const double*)s->wk.gU.p, fn.scale, fn.d_a.p);
    launch_ks_reduce(s->stream, nt, (const double*)fn.d_a.p, fn.coeffKS, fn.d_kpart.p, fn.d_ks.p);
    DAS_HIP(hipGetLastError());
    double ms[2];
    DAS_HIP(hipMemcpyAsync(ms, fn.d_ks.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return (ms[0] + std::log(ms[1])) / fn.coeffKS;
}
// the per-cell weights g dF/dvm_c of the derivative passes into fn.d_wc (0 outside the set); g = seed x dF/dF0 of calcRefVar
static void vm_ks_cell_weights(das_solver* s, das_solver::CellFn& fn, double seed) {
    const double outer = seed * ref_var_outer(fn.refVar, fn.ref, vm_ks_value(s, fn));
    const long long nt = (long long)fn.cell.size();
    launch_ks_weights(s->stream, nt, (const double*)fn.d_a.p, fn.coeffKS, (const double*)fn.d_ks.p, outer, fn.d_wt.p);
    DAS_HIP(hipMemsetAsync(fn.d_wc.p, 0, (size_t)s->mesh.nC * sizeof(double), s->stream));
    hipLaunchKernelGGL(k_vm_cell_weights, dim3(nblk(nt, 256)), dim3(256), 0, s->stream, nt, (const int*)fn.d_cell.p, (const double*)fn.d_wt.p, fn.d_wc.p);
    DAS_HIP(hipGetLastError());
}
// product_j = seed s_j dF/dW_j of vonMisesStressKS: per colour one dual-number gradient pass and a gather over the cell and its face
// neighbours (k_vm_gather), no atomics
static void vm_ks_gradient(das_solver* s, das_solver::CellFn& fn, double seed, double* product) {
    ensure_con_dev(s, 0);
    vm_ks_cell_weights(s, fn, 1.0);
    const ResParams prm = s->wk1.bind(s->cp.solver, s->dm.nC, s->dm.nF, make_params(s->cp, s->opt, 0));
    const long long n = s->n;
    if (s->d_Wd.n != (size_t)n) { s->d_Wd.alloc(n); s->d_Rd.alloc(n); }
    DAS_HIP(hipMemsetAsync(s->d_tmp2.p, 0, n * sizeof(double), s->stream));
    const int B = 256;
    for (int col = 0; col < s->nColors; col++) {
        hipLaunchKernelGGL(k_seed<1>, dim3(nblk(n, B)), dim3(B), 0, s->stream, n, s->d_W.p, s->d_colors.p, s->d_scale.p, col, s->d_Wd.p);
        launch_solid_grad<Dual<1>, double>(s->dm, prm, (const Dual<1>*)s->d_Wd.p, s->wk1, s->stream);
        hipLaunchKernelGGL(k_vm_tangent, dim3(nblk(s->dm.nC, B)), dim3(B), 0, s->stream, s->dm.nC, prm, (const Dual<1>*)s->wk1.gU.p, fn.scale, (const double*)fn.d_wc.p, s->d_tmp1.p);
        launch_vm_gather(s->stream, s->dm, (const int*)s->d_colors.p, col, (const double*)s->d_tmp1.p, seed, s->d_tmp2.p);
    }
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(product, s->d_tmp2.p, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
}
// F0 = coef sum_t w_t g(x_t) (before calcRefVar)
static double cell_function_base_value(das_solver* s, das_solver::CellFn& fn) {
    if (fn.vmKS) return vm_ks_value(s, fn);
    if (fn.coef == 0.0) return 0.0;
    launch_cellfn_value(s->stream, fn.view(), (const CellGeom*)s->d_cg.p, cell_function_src(s, fn), fn.coef, fn.d_part.p, s->d_tmp1.p);
    DAS_HIP(hipGetLastError());
    double v = 0.0;
    DAS_HIP(hipMemcpyAsync(&v, s->d_tmp1.p, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return v;
}
// dF/dF0: 2 (F0 - ref) under calcRefVar (DAFunction::calcRefVar), else 1
static double cell_function_outer(das_solver* s, das_solver::CellFn& fn) {
    return ref_var_outer(fn.refVar, fn.ref, fn.refVar ? cell_function_base_value(s, fn) : 0.0);  // the value pass runs only where it is read
}
// out[0..len) = 0, then seed dF/dsrc_i (x s_i for the states) on the entries of the terms
static void cell_function_gradient(das_solver* s, das_solver::CellFn& fn, double seed, bool stateScaled, double* out, long long len) {
    const double g = seed * cell_function_outer(s, fn) * fn.coef;
    DAS_HIP(hipMemsetAsync(s->d_tmp2.p, 0, len * sizeof(double), s->stream));
    if (g != 0.0 && !fn.cell.empty())
        launch_cellfn_grad(s->stream, fn.view(), (const CellGeom*)s->d_cg.p, cell_function_src(s, fn),
                           stateScaled ? (const double*)s->d_scale.p : (const double*)nullptr, g, s->d_tmp2.p);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(out, s->d_tmp2.p, len * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
}
static das_solver::FaceFn& get_function(das_solver* s, const char* name) {
    auto it = s->functions.find(name ? name : "");
    DAS_CHECK(it != s->functions.end(), DAS_ERR_ARG, std::string("function not defined: ") + (name ? name : "(null)"));
    das_solver::FaceFn& fn = it->second;
    if (fn.geomVersion != s->geomVersion) build_function_geometry(s, fn);
    if (!fn.uploaded) {
        fn.d_faces.upload(fn.faces);
        fn.d_group.upload(fn.group);
        fn.d_w0.upload(fn.w0);
        fn.d_weff.alloc(fn.w0.size());
        if (!fn.dir.empty()) fn.d_dir.upload(fn.dir);
        fn.uploaded = true;
    }
    return fn;
}
// group sums S[0], S[1] of w0_f q_f at the current states (k_grad + k_fn_value)
static void function_sums(das_solver* s, das_solver::FaceFn& fn, double S[2]) {
    const bool rho = DAS_IS_COMPRESSIBLE(s->cp.solver);
    const int B = 256, nf = (int)fn.faces.size();
    if (fn.d_fv.n != (size_t)nf) fn.d_fv.alloc(nf);
    if (DAS_FN_BASE(fn.kind) == DAS_FN_LOCATION) {  // geometry only: no gradients, no states
        hipLaunchKernelGGL((k_fn_value<false>), dim3(nblk(nf, B)), dim3(B), 0, s->stream, s->dm, make_params(s->cp, s->opt, 0), s->d_W.p, (const double*)nullptr,
                           (const double*)nullptr, fn.view(fn.d_w0.p), fn.d_fv.p);
        if (fn.ks) { DAS_HIP(hipGetLastError()); S[0] = S[1] = 0.0; return; }  // the KS reduction reads fn.d_fv (location_ks_value)
    } else {
        const ResParams prm = s->wk.bind(s->cp.solver, s->dm.nC, s->dm.nF, make_params(s->cp, s->opt, 0));
        launch_grad_and_faces(s->stream, rho, s->dm, prm, (const double*)s->d_W.p, s->wk, true, [&](auto R) {
            hipLaunchKernelGGL((k_fn_value<decltype(R)::value, decltype(R)::solid>), dim3(nblk(nf, B)), dim3(B), 0, s->stream, s->dm, prm, s->d_W.p, s->wk.nut.p, s->wk.gU.p, fn.view(fn.d_w0.p), fn.d_fv.p);
        });
    }
    launch_group_sum(s->stream, (long long)nf, (const unsigned char*)fn.d_group.p, (const double*)fn.d_fv.p, s->d_tmp1.p);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(S, s->d_tmp1.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
}
// the KS aggregate F0 = (m + log S) / coeffKS of the per-face values (das_facefn.hpp); {m, S} stay in fn.d_ks for k_ks_weights.
// The reference stops when its running sum of exp(coeffKS a_f) passes 1e200 (DAFunctionLocation.C:195-199); the sum only grows, so
// that is the total m + log S passing log(1e200) - the same guard, with no exponential that could overflow.
static double location_ks_value(das_solver* s, das_solver::FaceFn& fn) {
    double unused[2];
    function_sums(s, fn, unused);  // a_f -> fn.d_fv
    const long long nf = (long long)fn.faces.size();
    if (fn.d_ks.n != 2) { fn.d_ks.alloc(2); fn.d_kpart.alloc(DAS_FACEFN_MAX_BLOCKS); }
    launch_ks_reduce(s->stream, nf, (const double*)fn.d_fv.p, fn.coeffKS, fn.d_kpart.p, fn.d_ks.p);
    DAS_HIP(hipGetLastError());
    double ms[2];
    DAS_HIP(hipMemcpyAsync(ms, fn.d_ks.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    const double lg = ms[0] + std::log(ms[1]);
    DAS_CHECK(lg <= std::log(1e200), DAS_ERR_ARG, "KS function summation term too large! Reduce coeffKS!");
    return lg / fn.coeffKS;
}
// the function before calcRefVar: the sum or the quotient of the group sums, or the KS aggregate
static double function_base_value(das_solver* s, das_solver::FaceFn& fn) {
    if (fn.ks) return location_ks_value(s, fn);
    double S[2];
    function_sums(s, fn, S);
    return fn.ratio ? S[1] / S[0] : S[0] + S[1];
}
// effective per-face weights of the derivative passes: the base weights, times the quotient rule for ratio functions
static void function_effective_weights(das_solver* s, das_solver::FaceFn& fn) {
    if (DAS_FN_BASE(fn.kind) == DAS_FN_LOCATION) {  // dF/da_f: the softmax of the KS modes, 1 on the one face of maxRadius
        const double F0 = function_base_value(s, fn);
        const double outer = ref_var_outer(fn.refVar, fn.ref, F0);
        const long long nf = (long long)fn.faces.size();
        if (fn.ks) {
            launch_ks_weights(s->stream, nf, (const double*)fn.d_fv.p, fn.coeffKS, (const double*)fn.d_ks.p, outer, fn.d_weff.p);
            DAS_HIP(hipGetLastError());
        } else {
            fn.d_weff.upload(std::vector<double>(fn.w0.size(), outer));
        }
        return;
    }
    if (!fn.refVar && !fn.ratio) {  // F = S0 + S1: the base weights, no sums needed
        DAS_HIP(hipMemcpyAsync(fn.d_weff.p, fn.d_w0.p, fn.w0.size() * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        return;
    }
    double S[2], c[2];  // c[g] = dF/dS_g
    function_sums(s, fn, S);
    if (!fn.ratio) {  // F = (S - ref)^2: dF = 2 (S - ref) dS
        c[0] = c[1] = ref_var_outer(true, fn.ref, S[0] + S[1]);
    } else if (fn.refVar) {  // F = (S1 / S0 - ref)^2; written out, not as the plain quotient rule times a: the rounding differs
        const double a = ref_var_outer(true, fn.ref, S[1] / S[0]);
        c[0] = -a * S[1] / (S[0] * S[0]);
        c[1] = a / S[0];
    } else {  // F = S1 / S0
        c[0] = -S[1] / (S[0] * S[0]);
        c[1] = 1.0 / S[0];
    }
    std::vector<double> w(fn.w0.size());
    for (size_t k = 0; k < w.size(); k++) w[k] = fn.w0[k] * c[fn.group[k]];
    fn.d_weff.upload(w);
}
// ---- meshQualityKS and residualNorm (reference DAFunctionMeshQualityKS.C, DAFunctionResidualNorm.C; kernels: das_meshquality.hpp) ----
static GeomTopo device_geom_topo(das_solver* s);
static RowLayout residual_row_layout(das_solver* s);
static das_solver::MeshFn* find_mesh_function(das_solver* s, const char* name) {
    auto it = s->meshFunctions.find(name ? name : "");
    return it == s->meshFunctions.end() ? nullptr : &it->second;
}
static void need_mesh_function_solver(das_solver* s, const std::string& type, const char* name) {
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SIMPLEFOAM || DAS_IS_COMPRESSIBLE(s->cp.solver) || s->cp.solver == DAS_SOLVER_SCALARTRANSPORTFOAM, DAS_ERR_ARG,
              "function type " + type + " (function " + name + ") is built for DASimpleFoam, DARhoSimpleFoam, DATurboFoam and DAScalarTransportFoam");
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, type + " function " + name + " runs on an undecomposed solver (sharded solvers are not supported)");
}
static void register_mesh_function(das_solver* s, const char* name, das_solver::MeshFn&& fn) {
    fn.name = name;
    s->functions.erase(name);
    s->cellFunctions.erase(name);
    s->meshFunctions.erase(name);
    s->meshFunctions.emplace(name, std::move(fn));
}
// meshQualityKS: the KS aggregate of a per-face mesh-quality metric over ALL faces.  flags & 8: calcRefVar.  No scale is applied (the
// reference's calcFunction multiplies by none).  Cyclic patches are refused: OpenFOAM treats their faces as coupled, with the neighbour's
// centre, which body_mesh_quality does not.
int das_define_mesh_quality_function(das_solver_t* s, const char* name, const char* metric, double coeffKS, int flags, double ref) {
    DAS_TRY
    DAS_CHECK(s && name && metric, DAS_ERR_ARG, "bad argument");
    need_mesh_function_solver(s, "meshQualityKS", name);
    const std::string mt = metric;
    DAS_CHECK(mt == "faceOrthogonality" || mt == "nonOrthoAngle" || mt == "faceSkewness", DAS_ERR_ARG,
              "metric not valid! Options: faceOrthogonality, nonOrthoAngle, or faceSkewness");
    DAS_CHECK(coeffKS != 0.0, DAS_ERR_ARG, std::string("coeffKS of meshQualityKS function ") + name + " is zero");
    for (int p = 0; p < s->mesh.nPatch; p++)
        DAS_CHECK(s->mesh.patch_type[p] != DAS_PATCH_CYCLIC, DAS_ERR_ARG,
                  std::string("meshQualityKS function ") + name + ": the mesh has cyclic patches, whose faces OpenFOAM treats as coupled; that is not built");
    das_solver::MeshFn fn;
    fn.metric = mt == "faceOrthogonality" ? DAS_MQ_ORTHO : mt == "nonOrthoAngle" ? DAS_MQ_NONORTHO : DAS_MQ_SKEW;
    fn.coeffKS = coeffKS;
    fn.refVar = (flags & 8) != 0;
    fn.ref = ref;
    register_mesh_function(s, name, std::move(fn));
    return DAS_OK;
    DAS_CATCH
}
// residualNorm: resNames[k] = "<state>Res" with weights[k]; every residual block of the solver must be among them, other names are
// ignored (the reference's unit test passes TRes to a case without T).  resMode L2Norm | L1Norm.  flags & 8: calcRefVar.  No scale.
int das_define_residual_norm_function(das_solver_t* s, const char* name, const char* const* resNames, const double* weights, int nw, const char* resMode,
                                      int flags, double ref) {
    DAS_TRY
    DAS_CHECK(s && name && resMode && (nw == 0 || (resNames && weights)) && nw >= 0, DAS_ERR_ARG, "bad argument");
    need_mesh_function_solver(s, "residualNorm", name);
    const std::string md = resMode;
    DAS_CHECK(md == "L2Norm" || md == "L1Norm", DAS_ERR_ARG, "resMode not supported! options are L2Norm or L1Norm (function " + std::string(name) + ": " + md + ")");
    const Stencil stn = make_stencil(s->cp.solver, s->mesh.nC, s->mesh.nF, s->opt, false, s->cp.hasT != 0, s->reg_needs_p());
    DAS_CHECK(stn.states.size() <= 8, DAS_ERR_INTERNAL, "more than 8 state blocks");
    das_solver::MeshFn fn;
    fn.residualNorm = true;
    fn.l1 = md == "L1Norm";
    for (size_t b = 0; b < stn.states.size(); b++) {
        const std::string res = stn.states[b].name + "Res";
        int at = -1;
        for (int k = 0; k < nw; k++) if (res == resNames[k]) at = k;
        DAS_CHECK(at >= 0, DAS_ERR_ARG, std::string("residualNorm function ") + name + ": resWeight has no entry for " + res);
        fn.w[b] = weights[at];
    }
    fn.refVar = (flags & 8) != 0;
    fn.ref = ref;
    register_mesh_function(s, name, std::move(fn));
    return DAS_OK;
    DAS_CATCH
}
// a_f of all faces at the current metrics -> fn.d_a, then the max-shifted two-stage KS sum; {m, S} stay in fn.d_ks for k_ks_weights.
// F0 = (m + log S) / coeffKS.  The reference aborts when its plain sum of exponentials passes 1e200; the log-space sum has no such limit
// and none is imposed (as for vonMisesStressKS).
static double mesh_quality_value(das_solver* s, das_solver::MeshFn& fn) {
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, std::string(fn.residualNorm ? "residualNorm" : "meshQualityKS") + " function " + fn.name + " runs on an undecomposed solver (sharded solvers are not supported)");
    const Mesh& m = s->mesh;
    const GeomTopo t = device_geom_topo(s);
    const long long nF = m.nF;
    if (fn.xGeom != s->geomVersion) { fn.d_X.upload(m.points.data(), 3 * (size_t)m.nP); fn.xGeom = s->geomVersion; }
    if (fn.d_a.n != (size_t)nF) { fn.d_a.alloc(nF); fn.d_w.alloc(nF); }
    if (fn.d_ks.n != 2) { fn.d_ks.alloc(2); fn.d_kpart.alloc(DAS_FACEFN_MAX_BLOCKS); }
    hipLaunchKernelGGL(k_mq_metric<double>, dim3(nblk(nF, 256)), dim3(256), 0, s->stream, t, (const double*)fn.d_X.p, (const FaceGeom*)s->d_fg.p,
                       (const CellGeom*)s->d_cg.p, fn.metric, (const double*)nullptr, fn.d_a.p);
    launch_ks_reduce(s->stream, nF, (const double*)fn.d_a.p, fn.coeffKS, fn.d_kpart.p, fn.d_ks.p);
    DAS_HIP(hipGetLastError());
    double ms[2];
    DAS_HIP(hipMemcpyAsync(ms, fn.d_ks.p, 2 * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return (ms[0] + std::log(ms[1])) / fn.coeffKS;
}
// the per-face weights seed dF/da_f of the volCoord product -> fn.d_w (the softmax of the base mesh; calcRefVar's outer derivative included)
static void mesh_quality_weights(das_solver* s, das_solver::MeshFn& fn, double seed) {
    const double outer = seed * ref_var_outer(fn.refVar, fn.ref, mesh_quality_value(s, fn));
    const long long nF = s->mesh.nF;
    launch_ks_weights(s->stream, nF, (const double*)fn.d_a.p, fn.coeffKS, (const double*)fn.d_ks.p, outer, fn.d_w.p);
    DAS_HIP(hipGetLastError());
}
static RnRows residual_norm_rows(das_solver* s, const das_solver::MeshFn& fn) {
    const RowLayout L = residual_row_layout(s);
    RnRows r{};
    r.nb = L.nb;
    for (int b = 0; b < L.nb; b++) { r.off[b] = L.off[b]; r.kind[b] = L.kind[b]; r.w[b] = fn.w[b]; }
    r.nC = s->mesh.nC; r.nF = s->mesh.nF; r.nIF = s->mesh.nIF;
    r.l1 = fn.l1 ? 1 : 0;
    return r;
}
// F0 of residualNorm on the residual das_calc_residuals returns at the current states (isPC 0, normalizeResiduals as configured); the
// residual stays in s->d_R for k_rn_seeds
static double residual_norm_value(das_solver* s, das_solver::MeshFn& fn) {
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, std::string(fn.residualNorm ? "residualNorm" : "meshQualityKS") + " function " + fn.name + " runs on an undecomposed solver (sharded solvers are not supported)");
    const long long n = s->n;
    const ResParams prm = make_params(s->cp, s->opt, 0);
    eval_residual<double>(s->dm, s->cp, prm, s->d_W.p, s->d_R.p, s->wk, s->d_phiF.p, s->d_Told.p, s->stream);
    if (fn.d_a.n != (size_t)n) fn.d_a.alloc(n);
    if (fn.d_ks.n != 2) { fn.d_ks.alloc(2); fn.d_kpart.alloc(DAS_FACEFN_MAX_BLOCKS); }
    launch_rn_sum(s->stream, n, residual_norm_rows(s, fn), (const double*)s->d_R.p, fn.d_a.p, fn.d_kpart.p, fn.d_ks.p);
    DAS_HIP(hipGetLastError());
    double sum = 0.0;
    DAS_HIP(hipMemcpyAsync(&sum, fn.d_ks.p + 1, sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return fn.l1 ? sum : std::sqrt(sum);
}
// d_g[i] = seed dF/dR_i at the current states (device array of s->n entries): the seeds of the  input -> residual  products
static void residual_norm_seeds(das_solver* s, das_solver::MeshFn& fn, double seed, double* d_g) {
    const double F0 = residual_norm_value(s, fn);
    DAS_CHECK(fn.l1 || F0 != 0.0, DAS_ERR_ARG, "residualNorm function " + fn.name + ": the L2Norm is zero, where it has no derivative");
    const double coef = seed * ref_var_outer(fn.refVar, fn.ref, F0);
    launch_rn_seeds(s->stream, (long long)s->n, residual_norm_rows(s, fn), (const double*)s->d_R.p, F0, coef, d_g);
    DAS_HIP(hipGetLastError());
}
// The product of a residualNorm function from any input is the existing  input -> residual  product with the seeds g = seed dF/dR:
// (ot, seeds) become ("residual", g).  g is formed on the device and comes down once (the product entries take host seeds).
static void residual_norm_redirect(das_solver* s, const char* outputName, std::string& ot, const double*& seeds, std::vector<double>& g) {
    if (ot != "function") return;
    das_solver::MeshFn* mf = find_mesh_function(s, outputName);
    if (!mf || !mf->residualNorm) return;
    g.resize(s->n);
    residual_norm_seeds(s, *mf, seeds[0], s->d_tmp2.p);
    DAS_HIP(hipMemcpyAsync(g.data(), s->d_tmp2.p, s->n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    ot = "residual";
    seeds = g.data();
}
int das_calc_function(das_solver_t* s, const char* name, double* value) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(value, DAS_ERR_ARG, "null output");
    if (das_solver::MeshFn* mf = find_mesh_function(s, name)) {
        *value = ref_var_value(mf->refVar, mf->ref, mf->residualNorm ? residual_norm_value(s, *mf) : mesh_quality_value(s, *mf));
        return DAS_OK;
    }
    if (das_solver::CellFn* cf = find_cell_function(s, name)) {
        *value = ref_var_value(cf->refVar, cf->ref, cell_function_base_value(s, *cf));
        return DAS_OK;
    }
    das_solver::FaceFn& fn = get_function(s, name);
    *value = ref_var_value(fn.refVar, fn.ref, function_base_value(s, fn));
    return DAS_OK;
    DAS_CATCH
}
static void face_function_gradient(das_solver* s, das_solver::FaceFn& fn, double seed, double* product);
// product_j = seed * s_j dF/dW_j : coloured forward-mode gradient of the objective (one k_grad + one k_force per colour)
static void function_gradient(das_solver* s, const char* name, double seed, double* product) {
    need_init(s);
    if (das_solver::MeshFn* mf = find_mesh_function(s, name)) {  // meshQualityKS reads the points alone: dF/dW = 0 exactly, no pass
        DAS_CHECK(!mf->residualNorm, DAS_ERR_INTERNAL, "residualNorm takes the residual product");
        std::fill(product, product + s->n, 0.0);
        return;
    }
    if (das_solver::CellFn* cf = find_cell_function(s, name)) {  // local and analytic: one elementwise pass, no colouring
        if (cf->field) std::fill(product, product + s->n, 0.0);
        else if (cf->vmKS) vm_ks_gradient(s, *cf, seed, product);
        else cell_function_gradient(s, *cf, seed, true, product, s->n);
        return;
    }
    das_solver::FaceFn& fn = get_function(s, name);
    if (DAS_FN_BASE(fn.kind) == DAS_FN_LOCATION) {  // geometry only: dF/dW = 0 exactly, no coloured pass
        std::fill(product, product + s->n, 0.0);
        return;
    }
    face_function_gradient(s, fn, seed, product);
}
// the coloured passes of function_gradient for a face function whose device arrays are in place
static void face_function_gradient(das_solver* s, das_solver::FaceFn& fn, double seed, double* product) {
    ensure_con_dev(s, 0);
    function_effective_weights(s, fn);
    ResParams prm = s->wk1.bind(s->cp.solver, s->dm.nC, s->dm.nF, make_params(s->cp, s->opt, 0));
    const bool rho = DAS_IS_COMPRESSIBLE(s->cp.solver);
    const long long n = s->n;
    if (s->d_Wd.n != (size_t)n) { s->d_Wd.alloc(n); s->d_Rd.alloc(n); }
    DAS_HIP(hipMemsetAsync(s->d_tmp2.p, 0, n * sizeof(double), s->stream));
    const int B = 256, nf = (int)fn.faces.size();
    for (int col = 0; col < s->nColors; col++) {
        hipLaunchKernelGGL(k_seed<1>, dim3(nblk(n, B)), dim3(B), 0, s->stream, n, s->d_W.p, s->d_colors.p, s->d_scale.p, col, s->d_Wd.p);
        launch_grad_and_faces(s->stream, rho, s->dm, prm, (const Dual<1>*)s->d_Wd.p, s->wk1, true, [&](auto R) {
            hipLaunchKernelGGL((k_fn_grad<decltype(R)::value, decltype(R)::solid>), dim3(nblk(nf, B)), dim3(B), 0, s->stream, s->dm, prm, s->d_Wd.p, s->wk1.nut.p, s->wk1.gU.p, fn.view(fn.d_weff.p), seed, s->d_colors.p, col, s->d_tmp2.p);
        });
    }
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(product, s->d_tmp2.p, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
}

// ---- forceCouplingOutput (reference DAOutputForceCoupling.C; layout and kernels: das_forcecoupling.hpp) --------------------------
static bool is_force_coupling(const std::string& outputType) { return outputType == "forceCouplingOutput"; }
static void need_force_coupling_solver(das_solver* s) {
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SIMPLEFOAM || DAS_IS_COMPRESSIBLE(s->cp.solver), DAS_ERR_ARG,
              "forceCouplingOutput needs a flow solver with a pressure field (DAScalarTransportFoam has no p)");
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "forceCouplingOutput runs on an undecomposed solver (sharded solvers are not supported)");
}
int das_define_force_coupling(das_solver_t* s, const char* name, const int* patch_ids, int npatch, double pRef) {
    DAS_TRY
    DAS_CHECK(s && name && patch_ids && npatch > 0, DAS_ERR_ARG, "bad argument");
    need_force_coupling_solver(s);
    const Mesh& m = s->mesh;
    das_solver::ForceCoupling fc;
    das_solver::FaceFn& fn = fc.fn;
    fc.fcPtr.push_back(0);
    for (int k = 0; k < npatch; k++) {
        const int p = patch_ids[k];
        DAS_CHECK(p >= 0 && p < m.nPatch, DAS_ERR_ARG,
                  "forceCouplingOutput " + std::string(name) + ": patch id " + std::to_string(p) + " is not in the mesh (" + std::to_string(m.nPatch) + " patches)");
        DAS_CHECK(m.patch_type[p] != DAS_PATCH_CYCLIC, DAS_ERR_ARG, "forceCouplingOutput cannot be defined on cyclic patches");
        const int f0 = m.patch_start[p], f1 = f0 + m.patch_size[p];
        // the distinct points of the patch's faces, ascending: this patch's share of the output (DAOutputForceCoupling.C:194-201)
        std::vector<int> pts(m.face_pts.begin() + m.face_ptr[f0], m.face_pts.begin() + m.face_ptr[f1]);
        std::sort(pts.begin(), pts.end());
        pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
        for (int f = f0; f < f1; f++) {
            fn.faces.push_back(f);
            for (int q = m.face_ptr[f]; q < m.face_ptr[f + 1]; q++)
                fc.fcPt.push_back(fc.nOut + (int)(std::lower_bound(pts.begin(), pts.end(), m.face_pts[q]) - pts.begin()));
            fc.fcPtr.push_back((int)fc.fcPt.size());
        }
        fc.nOut += (int)pts.size();
        fc.patches.push_back(p);
    }
    const int nf = (int)fn.faces.size();
    DAS_CHECK(nf > 0, DAS_ERR_ARG, "the patches of forceCouplingOutput " + std::string(name) + " have no faces");
    // output point -> face slots: filled slot by slot, so every list is ascending - the order k_fc_nodal adds in
    fc.ptPtr.assign(fc.nOut + 1, 0);
    for (int o : fc.fcPt) fc.ptPtr[o + 1]++;
    for (int o = 0; o < fc.nOut; o++) fc.ptPtr[o + 1] += fc.ptPtr[o];
    fc.ptSlot.resize(fc.fcPt.size());
    std::vector<int> pos(fc.ptPtr.begin(), fc.ptPtr.end() - 1);
    for (int k = 0; k < nf; k++)
        for (int q = fc.fcPtr[k]; q < fc.fcPtr[k + 1]; q++) fc.ptSlot[pos[fc.fcPt[q]]++] = k;
    fn.kind = DAS_FN_FORCE;
    fn.pRef = pRef;
    fn.group.assign(nf, 0);
    fn.w0.assign(nf, 1.0);
    fn.dir.assign(3 * (size_t)nf, 0.0);
    s->forceCouplings[name] = std::move(fc);
    return DAS_OK;
    DAS_CATCH
}
// the device arrays of the internal face function of a coupling output (unit weights; the directions are written per product)
static void upload_coupling_functional(das_solver* s, das_solver::FaceFn& fn) {
    fn.d_faces.upload(fn.faces);
    fn.d_group.upload(fn.group);
    fn.d_w0.upload(fn.w0);
    fn.d_weff.alloc(fn.w0.size());
    fn.d_dir.upload(fn.dir);
    fn.geomVersion = s->geomVersion;
    fn.uploaded = true;
}
static das_solver::ForceCoupling& get_force_coupling(das_solver* s, const char* name, bool device = true) {
    auto it = s->forceCouplings.find(name ? name : "");
    DAS_CHECK(it != s->forceCouplings.end(), DAS_ERR_ARG, std::string("forceCouplingOutput not defined: ") + (name ? name : "(null)"));
    need_force_coupling_solver(s);
    das_solver::ForceCoupling& fc = it->second;
    if (device && !fc.uploaded) {
        das_solver::FaceFn& fn = fc.fn;
        upload_coupling_functional(s, fn);
        fc.d_ptPtr.upload(fc.ptPtr); fc.d_ptSlot.upload(fc.ptSlot);
        fc.d_fcPtr.upload(fc.fcPtr); fc.d_fcPt.upload(fc.fcPt);
        fc.d_ff.alloc(3 * fn.faces.size());
        fc.d_out.alloc(3 * (size_t)fc.nOut);
        fc.d_seeds.alloc(3 * (size_t)fc.nOut);
        fc.uploaded = true;
    }
    return fc;
}
// seeds (3 nOut, host) -> the per-face directions of the force functional seeds . output = sum_f d_f . F_f; returns that functional
static das_solver::FaceFn& force_coupling_functional(das_solver* s, const char* name, const double* seeds) {
    das_solver::ForceCoupling& fc = get_force_coupling(s, name);
    const int nf = (int)fc.fn.faces.size();
    DAS_HIP(hipMemcpyAsync(fc.d_seeds.p, seeds, 3 * (size_t)fc.nOut * sizeof(double), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_fc_seed_dir, dim3(nblk(nf, 256)), dim3(256), 0, s->stream, nf, (const int*)fc.d_fcPtr.p, (const int*)fc.d_fcPt.p, (const double*)fc.d_seeds.p,
                       fc.fn.d_dir.p);
    DAS_HIP(hipGetLastError());
    return fc.fn;
}
int das_calc_force_coupling(das_solver_t* s, const char* name, double* out, int n) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(out, DAS_ERR_ARG, "null output");
    das_solver::ForceCoupling& fc = get_force_coupling(s, name);
    DAS_CHECK(n == 3 * fc.nOut, DAS_ERR_ARG,
              "forceCouplingOutput " + std::string(name) + " has " + std::to_string(3 * fc.nOut) + " entries (3 per point), not " + std::to_string(n));
    const bool rho = DAS_IS_COMPRESSIBLE(s->cp.solver);
    const int B = 256, nf = (int)fc.fn.faces.size();
    const ResParams prm = s->wk.bind(s->cp.solver, s->dm.nC, s->dm.nF, make_params(s->cp, s->opt, 0));
    launch_grad_and_faces(s->stream, rho, s->dm, prm, (const double*)s->d_W.p, s->wk, true, [&](auto R) {
        hipLaunchKernelGGL((k_fc_face_force<decltype(R)::value>), dim3(nblk(nf, B)), dim3(B), 0, s->stream, s->dm, prm, s->d_W.p, s->wk.nut.p, s->wk.gU.p, nf,
                           (const int*)fc.fn.d_faces.p, fc.fn.pRef, fc.d_ff.p);
    });
    hipLaunchKernelGGL(k_fc_nodal, dim3(nblk(fc.nOut, B)), dim3(B), 0, s->stream, fc.nOut, (const int*)fc.d_ptPtr.p, (const int*)fc.d_ptSlot.p, (const int*)fc.d_fcPtr.p,
                       (const double*)fc.d_ff.p, fc.d_out.p);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(out, fc.d_out.p, 3 * (size_t)fc.nOut * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return DAS_OK;
    DAS_CATCH
}

// ---- thermalCouplingOutput (reference DAOutputThermalCoupling.C; layout and kernels: das_thermalcoupling.hpp) ---------------------
static void need_thermal_coupling_solver(das_solver* s) {
    DAS_CHECK(DAS_IS_COMPRESSIBLE(s->cp.solver) || (s->cp.solver == DAS_SOLVER_SIMPLEFOAM && s->cp.hasT) || s->cp.solver == DAS_SOLVER_HEATTRANSFERFOAM, DAS_ERR_ARG,
              "thermalCouplingOutput needs a solver that carries a T field (DASimpleFoam with T, DARhoSimpleFoam, DATurboFoam)");
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "thermalCouplingOutput runs on an undecomposed solver (sharded solvers are not supported)");
}
// the faces of an output (input: the patches must carry a mixed T, where the reference's refCast aborts);
// flags & 2: wallDistanceMethod daCustom (the bit das_define_face_function_ex gives wallHeatFlux)
static int define_thermal_coupling(das_solver_t* s, const char* name, const int* patch_ids, int npatch, int flags, bool input) {
    DAS_TRY
    DAS_CHECK(s && name && patch_ids && npatch > 0, DAS_ERR_ARG, "bad argument");
    need_thermal_coupling_solver(s);
    const Mesh& m = s->mesh;
    const std::string what = std::string(input ? "thermalCoupling input " : "thermalCouplingOutput ") + name;
    das_solver::ThermalCoupling tc;
    das_solver::FaceFn& fn = tc.fn;
    for (int k = 0; k < npatch; k++) {
        const int p = patch_ids[k];
        DAS_CHECK(p >= 0 && p < m.nPatch, DAS_ERR_ARG, what + ": patch id " + std::to_string(p) + " is not in the mesh (" + std::to_string(m.nPatch) + " patches)");
        DAS_CHECK(m.patch_type[p] != DAS_PATCH_CYCLIC, DAS_ERR_ARG, what + " cannot be defined on cyclic patches");
        DAS_CHECK(!input || m.bc[p].T_code == DAS_BC_MIXED, DAS_ERR_ARG, what + ": patch id " + std::to_string(p) + " does not carry a mixed T patch field");
        for (int q = 0; q < m.patch_size[p]; q++) fn.faces.push_back(m.patch_start[p] + q);
        tc.patches.push_back(p);
    }
    const size_t nf = fn.faces.size();
    DAS_CHECK(nf > 0, DAS_ERR_ARG, "the patches of " + what + " have no faces");
    fn.kind = DAS_FN_THERMALCOUPLING | ((flags & 2) ? DAS_FN_ALT_BIT : 0);
    fn.group.assign(nf, 0);
    fn.w0.assign(nf, 1.0);
    fn.dir.assign(3 * nf, 0.0);
    (input ? s->thermalInputs : s->thermalCouplings)[name] = std::move(tc);
    return DAS_OK;
    DAS_CATCH
}
int das_define_thermal_coupling(das_solver_t* s, const char* name, const int* patch_ids, int npatch, int flags) {
    return define_thermal_coupling(s, name, patch_ids, npatch, flags, false);
}
int das_define_thermal_coupling_input(das_solver_t* s, const char* name, const int* patch_ids, int npatch, int flags) {
    return define_thermal_coupling(s, name, patch_ids, npatch, flags, true);
}
static das_solver::ThermalCoupling& get_thermal_coupling(das_solver* s, const char* name, bool device = true, bool input = false) {
    auto& table = input ? s->thermalInputs : s->thermalCouplings;
    auto it = table.find(name ? name : "");
    DAS_CHECK(it != table.end(), DAS_ERR_ARG, std::string(input ? "thermalCoupling input not defined: " : "thermalCouplingOutput not defined: ") + (name ? name : "(null)"));
    need_thermal_coupling_solver(s);
    das_solver::ThermalCoupling& tc = it->second;
    if (device && !tc.uploaded) {
        upload_coupling_functional(s, tc.fn);
        tc.d_out.alloc(2 * tc.fn.faces.size());
        tc.d_seeds.alloc(2 * tc.fn.faces.size());
        tc.uploaded = true;
    }
    return tc;
}
// [T of the owner cells, kappa / d] of the faces of tc at the current states -> tc.d_out
static void thermal_coupling_values(das_solver* s, das_solver::ThermalCoupling& tc) {
    const int B = 256, nf = (int)tc.fn.faces.size();
    const ResParams prm = s->wk.bind(s->cp.solver, s->dm.nC, s->dm.nF, make_params(s->cp, s->opt, 0));
    // the gradient pass fills nut of the cells, which a symmetry-type nut patch reads
    launch_grad_and_faces(s->stream, DAS_IS_COMPRESSIBLE(s->cp.solver), s->dm, prm, (const double*)s->d_W.p, s->wk, true, [&](auto R) {
        hipLaunchKernelGGL((k_tc_values<decltype(R)::value, decltype(R)::solid>), dim3(nblk(nf, B)), dim3(B), 0, s->stream, s->dm, prm, s->d_W.p, s->wk.nut.p, nf,
                           (const int*)tc.fn.d_faces.p, (int)DAS_FN_ALT(tc.fn.kind), tc.d_out.p);
    });
    DAS_HIP(hipGetLastError());
}
int das_calc_thermal_coupling(das_solver_t* s, const char* name, double* out, int n) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(out, DAS_ERR_ARG, "null output");
    das_solver::ThermalCoupling& tc = get_thermal_coupling(s, name);
    const int nf = (int)tc.fn.faces.size();
    DAS_CHECK(n == 2 * nf, DAS_ERR_ARG,
              "thermalCouplingOutput " + std::string(name) + " has " + std::to_string(2 * nf) + " entries (2 per face), not " + std::to_string(n));
    thermal_coupling_values(s, tc);
    DAS_HIP(hipMemcpyAsync(out, tc.d_out.p, 2 * (size_t)nf * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return DAS_OK;
    DAS_CATCH
}
// DAInputThermalCoupling::run: in[k] -> refValue, in[nF + k] = the neighbour's kappa / d -> valueFraction = nk / (myK + nk), myK this side's
// kappa / d at the current states, geometry and boundary values (those from before this call, like the reference's alphaEff field)
int das_set_thermal_coupling_input(das_solver_t* s, const char* name, const double* in, int n) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(in, DAS_ERR_ARG, "null input");
    das_solver::ThermalCoupling& tc = get_thermal_coupling(s, name, true, true);
    const int nf = (int)tc.fn.faces.size();
    DAS_CHECK(n == 2 * nf, DAS_ERR_ARG,
              "thermalCoupling input " + std::string(name) + " has " + std::to_string(2 * nf) + " entries (2 per face), not " + std::to_string(n));
    for (int k = 0; k < nf; k++)
        DAS_CHECK(in[nf + k] >= 0.0, DAS_ERR_ARG, "thermalCoupling input " + std::string(name) + ": a negative kappa / d of the neighbour (entry " + std::to_string(nf + k) + ")");
    thermal_coupling_values(s, tc);
    DAS_HIP(hipMemcpyAsync(tc.d_seeds.p, in, 2 * (size_t)nf * sizeof(double), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_tc_set_mixed, dim3(nblk(nf, 256)), dim3(256), 0, s->stream, nf, (const int*)tc.fn.d_faces.p, s->dm.nIF, (const double*)tc.d_seeds.p,
                       (const double*)(tc.d_out.p + nf), s->d_mixed.p);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(s->mesh.mixed.data(), s->d_mixed.p, s->mesh.mixed.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    tc.in.assign(in, in + n);
    s->opEpoch++;
    return DAS_OK;
    DAS_CATCH
}
// refValue and valueFraction of the faces of a patch with a mixed T, as they stand (size: the faces of the patch)
int das_get_patch_mixed(das_solver_t* s, int patch, double* refValue, double* valueFraction) {
    DAS_TRY
    DAS_CHECK(s && refValue && valueFraction, DAS_ERR_ARG, "null argument");
    const Mesh& m = s->mesh;
    DAS_CHECK(patch >= 0 && patch < m.nPatch, DAS_ERR_ARG, "patch id out of range");
    DAS_CHECK(m.bc[patch].T_code == DAS_BC_MIXED, DAS_ERR_ARG, "patch id " + std::to_string(patch) + " does not carry a mixed T patch field");
    for (int k = 0; k < m.patch_size[patch]; k++) {
        const size_t bf = (size_t)(m.patch_start[patch] - m.nIF + k);
        refValue[k] = m.mixed[4 * bf];
        valueFraction[k] = m.mixed[4 * bf + 1];
    }
    return DAS_OK;
    DAS_CATCH
}

// ---- both coupling outputs, as the derivative products and das_get_output_size see them ------------------------------------------
static bool is_coupling(const std::string& outputType) { return outputType == "forceCouplingOutput" || outputType == "thermalCouplingOutput"; }
// the number of entries; an unknown name or a solver the output does not run on is an error
static int coupling_size(das_solver* s, const std::string& outputType, const char* name) {
    if (is_force_coupling(outputType)) return 3 * get_force_coupling(s, name, false).nOut;
    return 2 * (int)get_thermal_coupling(s, name, false).fn.faces.size();
}
// seeds (host, one per entry) -> the face functional seeds . output of the derivative passes, its per-face directions set on the device
static das_solver::FaceFn& coupling_functional(das_solver* s, const std::string& outputType, const char* name, const double* seeds) {
    if (is_force_coupling(outputType)) return force_coupling_functional(s, name, seeds);
    das_solver::ThermalCoupling& tc = get_thermal_coupling(s, name);
    const int nf = (int)tc.fn.faces.size();
    DAS_HIP(hipMemcpyAsync(tc.d_seeds.p, seeds, 2 * (size_t)nf * sizeof(double), hipMemcpyHostToDevice, s->stream));
    hipLaunchKernelGGL(k_tc_seed_dir, dim3(nblk(nf, 256)), dim3(256), 0, s->stream, nf, (const double*)tc.d_seeds.p, tc.fn.d_dir.p);
    DAS_HIP(hipGetLastError());
    return tc.fn;
}

long long das_op_nnz(das_solver_t* s) { return (s && s->op) ? s->op->m.nnz : -1; }
// the operator initializedRdWTMatrixFree assembled, as CSR on the host (bench.py: the CPU baseline multiplies the SAME matrix)
int das_op_export(das_solver_t* s, long long* rowptr, int* colidx, double* vals) {
    DAS_TRY
    DAS_CHECK(s && s->op, DAS_ERR_STATE, "initializedRdWTMatrixFree() has not been called");
    DAS_CHECK(rowptr && colidx && vals, DAS_ERR_ARG, "null argument");
    const Mat& M = s->op->m;
    M.rowptr.download(rowptr, M.n + 1);
    M.col.download(colidx, M.nnz);
    M.val.download(vals, M.nnz);
    return DAS_OK;
    DAS_CATCH
}
// bytes of matrix data one dRdW^T.psi product streams in the operator's storage format (packed vector rows + CSR scalar rows)
long long das_op_format_bytes(das_solver_t* s) {
    if (!s || !s->op) return -1;
    const Mat& M = s->op->m;
    if (!M.vp.ready) return 12LL * M.nnz + 8LL * (M.n + 1);
    return M.vp.bytes() + 12LL * (M.nnz - M.vp.csrEntries) + 8LL * (M.n - 3 * M.vp.nGroups + 1);
}

// ---- boundary-value inputs (reference DAInputPatchVelocity.C:33-135, DAInputPatchVar.C) ---------------------------
static int bc_field_id(const char* field) {
    std::string f = field ? field : "";
    if (f == "U" || f == "D") return 0;  // (D of DASolidDisplacementFoam rides in the U slots of the patch table)
    if (f == "p") return 1;
    if (f == "nuTilda") return 2;
    if (f == "T") return 3;
    throw Error(DAS_ERR_ARG, "patch field not supported: " + f);
}
static void check_patches(das_solver* s, const int* patches, int np) {
    DAS_CHECK(patches && np > 0, DAS_ERR_ARG, "no patches given");
    for (int i = 0; i < np; i++) DAS_CHECK(patches[i] >= 0 && patches[i] < s->mesh.nPatch, DAS_ERR_ARG, "patch id out of range");
}
int das_set_patch_value(das_solver_t* s, const int* patches, int np, const char* field, const double* value) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(value, DAS_ERR_ARG, "null value");
    check_patches(s, patches, np);
    const int fid = bc_field_id(field);
    for (int i = 0; i < np; i++) {
        PatchBC& b = s->mesh.bc[patches[i]];
        const int code = fid == 0 ? b.U_code : fid == 1 ? b.p_code : fid == 2 ? b.nuTilda_code : b.T_code;
        // the reference accepts fixedValue and inletOutlet patches only (DAInputPatchVelocity.C:84-131)
        DAS_CHECK(code == DAS_BC_FIXED_VALUE || code == DAS_BC_INLET_OUTLET, DAS_ERR_ARG,
                  "patch type not valid! only support fixedValue or inletOutlet");
        if (fid == 0) for (int k = 0; k < 3; k++) b.U_val[k] = value[k];
        else if (fid == 1) b.p_val = value[0];
        else if (fid == 2) b.nuTilda_val = value[0];
        else b.T_val = value[0];
    }
    DAS_HIP(hipStreamSynchronize(s->stream));
    s->d_bc.upload(s->mesh.bc);
    s->opEpoch++;
    return DAS_OK;
    DAS_CATCH
}
int das_get_patch_value(das_solver_t* s, int patch, const char* field, double* value) {
    DAS_TRY
    DAS_CHECK(s && value, DAS_ERR_ARG, "null argument");
    check_patches(s, &patch, 1);
    const int fid = bc_field_id(field);
    const PatchBC& b = s->mesh.bc[patch];
    if (fid == 0) for (int k = 0; k < 3; k++) value[k] = b.U_val[k];
    else value[0] = fid == 1 ? b.p_val : fid == 2 ? b.nuTilda_val : b.T_val;
    return DAS_OK;
    DAS_CATCH
}
// product = seeds^T (dOutput/d(patch value) . tangent): ONE forward-mode pass of the residual (or of the objective)
// with the tangent seeded in the patch table -- the scalar-input counterpart of the coloured state Jacobian.
int das_calc_dbc_product(das_solver_t* s, const int* patches, int np, const char* field, const double* tangent, const char* outputName,
                         const char* outputType, const double* seeds, double* product) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(tangent && outputType && seeds && product, DAS_ERR_ARG, "null argument");
    check_patches(s, patches, np);
    const int fid = bc_field_id(field);
    std::string ot = outputType;
    std::vector<double> rnSeeds;  // a residualNorm function: the residual product with the seeds dF/dR
    residual_norm_redirect(s, outputName, ot, seeds, rnSeeds);
    const bool isFC = is_coupling(ot);
    DAS_CHECK(ot == "residual" || ot == "function" || isFC, DAS_ERR_ARG, "outputType not supported on this path: " + ot);
    if (isFC) (void)coupling_size(s, ot, outputName);  // an unknown name fails before the patch table is touched
    std::vector<PatchBC> bc = s->mesh.bc;
    for (int i = 0; i < np; i++) {
        PatchBC& b = bc[patches[i]];
        if (fid == 0) for (int k = 0; k < 3; k++) b.dU_val[k] = tangent[k];
        else if (fid == 1) b.dp_val = tangent[0];
        else if (fid == 2) b.dnuTilda_val = tangent[0];
        else b.dT_val = tangent[0];
    }
    const long long n = s->n;
    const int B = 256;
    hipStream_t st = s->stream;
    DAS_HIP(hipStreamSynchronize(st));
    s->d_bc.upload(bc);
    struct Restore {
        das_solver* s;
        ~Restore() { (void)hipStreamSynchronize(s->stream); s->d_bc.upload(s->mesh.bc); }
    } restore{s};
    ResParams prm = make_params(s->cp, s->opt, 0);
    const bool rho = DAS_IS_COMPRESSIBLE(s->cp.solver);
    if (s->d_Wd.n != (size_t)n) { s->d_Wd.alloc(n); s->d_Rd.alloc(n); }
    hipLaunchKernelGGL(k_lift, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_W.p, s->d_Wd.p);  // states carry no tangent
    DAS_HIP(hipMemsetAsync(s->d_tmp1.p, 0, sizeof(double), st));
    if (ot == "residual") {
        eval_residual<Dual<1>>(s->dm, s->cp, prm, s->d_Wd.p, s->d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
        DAS_HIP(hipMemcpyAsync(s->d_tmp2.p, seeds, n * sizeof(double), hipMemcpyHostToDevice, st));
        DevBuf<double> part(DAS_TANGENT_DOT_BLOCKS);
        launch_tangent_dot(st, n, (const Dual<1>*)s->d_Rd.p, (const double*)s->d_tmp2.p, part.p, s->d_tmp1.p);
        DAS_HIP(hipStreamSynchronize(st));  // part goes out of scope
    } else if (!isFC && find_cell_function(s, outputName)) {
        // variableVolSum reads no boundary value.  vonMisesStressKS does - vm of a boundary cell follows a fixedValue D through the cell
        // gradD - and its zero here is the convention the function layer was specified with, NOT the derivative
        product[0] = 0.0;
        return DAS_OK;
    } else if (!isFC && (find_mesh_function(s, outputName) || DAS_FN_BASE(get_function(s, outputName).kind) == DAS_FN_LOCATION)) {  // geometry only
        product[0] = 0.0;
        return DAS_OK;
    } else {
        // coupling outputs: the functional seeds . output (its directions carry the seeds: the seed of the pass is 1)
        das_solver::FaceFn& fn = isFC ? coupling_functional(s, ot, outputName, seeds) : get_function(s, outputName);
        const double fnSeed = isFC ? 1.0 : seeds[0];
        function_effective_weights(s, fn);
        DAS_HIP(hipMemsetAsync(s->d_tmp1.p, 0, sizeof(double), st));  // function_sums used the scratch
        prm = s->wk1.bind(s->cp.solver, s->dm.nC, s->dm.nF, prm);
        const int nf = (int)fn.faces.size();
        if (fn.d_fv.n != (size_t)nf) fn.d_fv.alloc(nf);
        launch_grad_and_faces(st, rho, s->dm, prm, (const Dual<1>*)s->d_Wd.p, s->wk1, true, [&](auto R) {
            hipLaunchKernelGGL((k_fn_tangent<decltype(R)::value, decltype(R)::solid>), dim3(nblk(nf, B)), dim3(B), 0, st, s->dm, prm, s->d_Wd.p, s->wk1.nut.p, s->wk1.gU.p, fn.view(fn.d_weff.p), fnSeed, fn.d_fv.p);
        });
        launch_group_sum(st, (long long)nf, nullptr, (const double*)fn.d_fv.p, s->d_tmp1.p);
    }
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(product, s->d_tmp1.p, sizeof(double), hipMemcpyDeviceToHost, st));
    DAS_HIP(hipStreamSynchronize(st));
    return DAS_OK;
    DAS_CATCH
}

// ---- thermalCoupling input -> residual | function | thermalCouplingOutput: product = [d output / d input]^T seeds (2 nF entries) ---------------
// The input reaches the solver through refValue_f = in[k] and valueFraction_f = nk / (myK + nk), nk = in[nF + k]:
//   product[k]      = seeds . d output / d refValue_f
//   product[nF + k] = seeds . d output / d valueFraction_f  x  myK / (myK + nk)^2,   myK as it was when the input was set.
// Forward-mode passes with the seed in the mixed records (bc_mixed carries it).  A function or a thermalCouplingOutput reads the record of a face
// in the summand of that face only: one pass per kind of seed with all faces seeded, the per-face tangents are the derivatives.  The
// residual: a face acts on the rows that read T of its owner cell, so faces whose owner cells' T states have the same
// colour do not share a row and are seeded together; faces that share an owner cell (corner cells) are told apart by their rank in
// the cell.  After each pass k_tc_gather adds psi_r dR_r over the rows of the owner's T column, face by face: no atomics.
int das_calc_dthermal_coupling_product(das_solver_t* s, const char* inputName, const char* outputName, const char* outputType, const double* seeds,
                                       double* product, int n) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(outputType && seeds && product, DAS_ERR_ARG, "null argument");
    std::string ot = outputType;
    std::vector<double> rnSeeds;  // a residualNorm function: the residual product with the seeds dF/dR
    residual_norm_redirect(s, outputName, ot, seeds, rnSeeds);
    const bool isFC = ot == "thermalCouplingOutput";
    DAS_CHECK(ot == "residual" || ot == "function" || isFC, DAS_ERR_ARG, "outputType not supported on this path: " + ot);
    das_solver::ThermalCoupling& tc = get_thermal_coupling(s, inputName, true, true);
    const int nf = (int)tc.fn.faces.size(), B = 256;
    DAS_CHECK(n == 2 * nf, DAS_ERR_ARG, "thermalCoupling input " + std::string(inputName ? inputName : "") + " has " + std::to_string(2 * nf) + " entries, not " + std::to_string(n));
    DAS_CHECK((int)tc.in.size() == 2 * nf, DAS_ERR_ARG, "thermalCoupling input " + std::string(inputName ? inputName : "") + " has not been set");
    if (isFC) (void)coupling_size(s, ot, outputName);
    std::fill(product, product + n, 0.0);
    if (ot == "function") {  // cell-set functions and location read no boundary value of T
        if (find_cell_function(s, outputName) || find_mesh_function(s, outputName)) return DAS_OK;
        if (DAS_FN_BASE(get_function(s, outputName).kind) == DAS_FN_LOCATION) return DAS_OK;
    }
    hipStream_t st = s->stream;
    const long long ns = s->n;
    const int* faces = (const int*)tc.fn.d_faces.p;
    struct Restore {  // whatever happens, the records carry no tangent afterwards
        das_solver* s;
        ~Restore() { (void)hipStreamSynchronize(s->stream); s->d_mixed.upload(s->mesh.mixed); }
    } restore{s};
    ResParams prm = make_params(s->cp, s->opt, 0);
    const bool rho = DAS_IS_COMPRESSIBLE(s->cp.solver);
    if (s->d_Wd.n != (size_t)ns) { s->d_Wd.alloc(ns); s->d_Rd.alloc(ns); }
    hipLaunchKernelGGL(k_lift, dim3(nblk(ns, B)), dim3(B), 0, st, ns, s->d_W.p, s->d_Wd.p);  // states carry no tangent
    std::vector<double> dOut[2] = {std::vector<double>(nf, 0.0), std::vector<double>(nf, 0.0)};  // d / d refValue_f, d / d valueFraction_f
    if (ot == "residual") {
        ConDev& c = ensure_con_dev(s, 0);
        const long long colOff = (long long)prm.offT * s->mesh.nC;
        // groups: (colour of the owner's T state, rank of the face among the input's faces of that cell)
        std::map<std::pair<int, int>, std::vector<int>> groups;
        std::map<int, int> seen;
        for (int k = 0; k < nf; k++) {
            const int cell = s->mesh.owner[tc.fn.faces[k]];
            groups[{s->colors[colOff + cell], seen[cell]++}].push_back(k);
        }
        DAS_HIP(hipMemcpyAsync(s->d_tmp2.p, seeds, ns * sizeof(double), hipMemcpyHostToDevice, st));
        DevBuf<double> d_face((size_t)nf);
        DevBuf<int> d_sel((size_t)nf);
        for (int which = 2; which <= 3; which++) {
            for (const auto& grp : groups) {
                const int cnt = (int)grp.second.size();
                DAS_HIP(hipMemcpyAsync(d_sel.p, grp.second.data(), cnt * sizeof(int), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_tc_seed_mixed, dim3(nblk(cnt, B)), dim3(B), 0, st, cnt, (const int*)d_sel.p, faces, s->dm.nIF, which, 1.0, s->d_mixed.p);
                eval_residual<Dual<1>>(s->dm, s->cp, prm, s->d_Wd.p, s->d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
                hipLaunchKernelGGL(k_tc_gather, dim3(nblk(cnt, B)), dim3(B), 0, st, cnt, (const int*)d_sel.p, faces, (const int*)s->d_owner.p, colOff,
                                   (const long long*)c.t_rowptr.p, (const int*)c.t_col.p, (const double*)s->d_tmp2.p, (const Dual<1>*)s->d_Rd.p, d_face.p);
                hipLaunchKernelGGL(k_tc_seed_mixed, dim3(nblk(cnt, B)), dim3(B), 0, st, cnt, (const int*)d_sel.p, faces, s->dm.nIF, which, 0.0, s->d_mixed.p);
                DAS_HIP(hipGetLastError());
                DAS_HIP(hipStreamSynchronize(st));  // d_sel is written again by the next group
            }
            DAS_HIP(hipMemcpy(dOut[which - 2].data(), d_face.p, nf * sizeof(double), hipMemcpyDeviceToHost));
        }
    } else {
        das_solver::FaceFn& fn = isFC ? coupling_functional(s, ot, outputName, seeds) : get_function(s, outputName);
        const double fnSeed = isFC ? 1.0 : seeds[0];
        function_effective_weights(s, fn);
        prm = s->wk1.bind(s->cp.solver, s->dm.nC, s->dm.nF, prm);
        const int nfn = (int)fn.faces.size();
        if (fn.d_fv.n != (size_t)nfn) fn.d_fv.alloc(nfn);
        std::map<int, int> slotOf;  // mesh face -> slot of the input
        for (int k = 0; k < nf; k++) slotOf[tc.fn.faces[k]] = k;
        std::vector<double> fv(nfn);
        for (int which = 2; which <= 3; which++) {
            hipLaunchKernelGGL(k_tc_seed_mixed, dim3(nblk(nf, B)), dim3(B), 0, st, nf, (const int*)nullptr, faces, s->dm.nIF, which, 1.0, s->d_mixed.p);
            launch_grad_and_faces(st, rho, s->dm, prm, (const Dual<1>*)s->d_Wd.p, s->wk1, true, [&](auto R) {
                hipLaunchKernelGGL((k_fn_tangent<decltype(R)::value, decltype(R)::solid>), dim3(nblk(nfn, B)), dim3(B), 0, st, s->dm, prm, s->d_Wd.p, s->wk1.nut.p, s->wk1.gU.p, fn.view(fn.d_weff.p), fnSeed, fn.d_fv.p);
            });
            hipLaunchKernelGGL(k_tc_seed_mixed, dim3(nblk(nf, B)), dim3(B), 0, st, nf, (const int*)nullptr, faces, s->dm.nIF, which, 0.0, s->d_mixed.p);
            DAS_HIP(hipGetLastError());
            DAS_HIP(hipMemcpyAsync(fv.data(), fn.d_fv.p, nfn * sizeof(double), hipMemcpyDeviceToHost, st));
            DAS_HIP(hipStreamSynchronize(st));
            for (int q = 0; q < nfn; q++) {  // in slot order of the function: a fixed order
                auto it = slotOf.find(fn.faces[q]);
                if (it != slotOf.end()) dOut[which - 2][it->second] += fv[q];
            }
        }
    }
    std::vector<double> myK(nf);
    DAS_HIP(hipMemcpy(myK.data(), tc.d_out.p + nf, nf * sizeof(double), hipMemcpyDeviceToHost));
    for (int k = 0; k < nf; k++) {
        const double nk = tc.in[nf + k], sum = myK[k] + nk;
        product[k] = dOut[0][k];
        product[nf + k] = dOut[1][k] * (myK[k] / (sum * sum));
    }
    return DAS_OK;
    DAS_CATCH
}

// ---- `field` inputs (reference DAInputField.C): betaFINuTilda ----------------------------------------------------
static void check_field(const char* name) {
    DAS_CHECK(name && std::string(name) == "betaFINuTilda", DAS_ERR_ARG,
              std::string("field input: fieldName \"") + (name ? name : "") + "\" is not implemented (betaFINuTilda is)");
}
int das_set_field(das_solver_t* s, const char* fieldName, const double* values) {
    DAS_TRY
    DAS_CHECK(s && values, DAS_ERR_ARG, "null argument");
    check_field(fieldName);
    DAS_CHECK(s->cp.solver != DAS_SOLVER_SCALARTRANSPORTFOAM && s->cp.solver != DAS_SOLVER_HEATTRANSFERFOAM && s->cp.solver != DAS_SOLVER_SOLIDDISPLACEMENTFOAM,
              DAS_ERR_ARG, "betaFINuTilda needs a Spalart-Allmaras solver");
    DAS_CHECK(s->regModels.empty(), DAS_ERR_ARG, "field input betaFINuTilda: a regressionModel is active and would overwrite the field in every residual evaluation");
    s->cp.beta_fi.assign(values, values + s->mesh.nC);
    if (s->inited) {
        DAS_HIP(hipStreamSynchronize(s->stream));
        s->d_betaFI.upload(s->cp.beta_fi);
        s->cp.betaFI_ptr = s->d_betaFI.p;
    }
    s->opEpoch++;
    return DAS_OK;
    DAS_CATCH
}
int das_get_field(das_solver_t* s, const char* fieldName, double* values) {
    DAS_TRY
    DAS_CHECK(s && values, DAS_ERR_ARG, "null argument");
    check_field(fieldName);
    for (int c = 0; c < s->mesh.nC; c++) values[c] = s->cp.beta_fi.empty() ? 1.0 : s->cp.beta_fi[c];
    return DAS_OK;
    DAS_CATCH
}
// product_c = seeds . dR/d(field_c): every residual row depends on the field value of its own cell only, so ONE dual pass
// with a unit tangent on all cells carries every derivative, and product_c = seed of the cell's nuTildaRes row x its tangent
__global__ void k_field_product(long long N, long long offN, const Dual<1>* __restrict__ R, const double* __restrict__ seeds, double* __restrict__ out) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (c < N) out[c] = seeds[offN + c] * R[offN + c].d[0];
}
int das_calc_dfield_product(das_solver_t* s, const char* fieldName, const char* outputName, const char* outputType, const double* seeds,
                            double* product) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(outputType && seeds && product, DAS_ERR_ARG, "null argument");
    check_field(fieldName);
    DAS_CHECK(s->regModels.empty(), DAS_ERR_ARG, "field input betaFINuTilda: a regressionModel is active and overwrites the field in every residual evaluation");
    std::string ot = outputType;
    std::vector<double> rnSeeds;  // a residualNorm function: the residual product with the seeds dF/dR
    residual_norm_redirect(s, outputName, ot, seeds, rnSeeds);
    DAS_CHECK(ot == "residual" || ot == "function" || is_coupling(ot), DAS_ERR_ARG, "outputType not supported on this path: " + ot);
    const long long N = s->mesh.nC, n = s->n;
    if (s->cp.solver == DAS_SOLVER_SCALARTRANSPORTFOAM || s->cp.solver == DAS_SOLVER_HEATTRANSFERFOAM || s->cp.solver == DAS_SOLVER_SOLIDDISPLACEMENTFOAM) {
        // no Spalart-Allmaras production term: nothing of these solvers reads the field - exact zeros (an unknown output still fails by name)
        if (is_coupling(ot)) (void)coupling_size(s, ot, outputName);
        else if (ot == "function" && !find_cell_function(s, outputName) && !find_mesh_function(s, outputName)) (void)get_function(s, outputName);
        std::fill(product, product + N, 0.0);
        return DAS_OK;
    }
    if (is_coupling(ot)) {  // like the patch-integral functions: the coupling outputs do not see the production term
        (void)coupling_size(s, ot, outputName);
        std::fill(product, product + N, 0.0);
        return DAS_OK;
    }
    if (ot == "function") {
        das_solver::CellFn* cf = find_cell_function(s, outputName);
        if (!cf && !find_mesh_function(s, outputName)) (void)get_function(s, outputName);  // the patch-integral functions do not see the production term
        if (cf && cf->field) cell_function_gradient(s, *cf, seeds[0], false, product, N);  // dF/dbeta_c, unscaled like the field itself
        else std::fill(product, product + N, 0.0);
        return DAS_OK;
    }
    hipStream_t st = s->stream;
    const int B = 256;
    if (s->cp.beta_fi.empty()) { s->cp.beta_fi.assign(N, 1.0); s->d_betaFI.upload(s->cp.beta_fi); s->cp.betaFI_ptr = s->d_betaFI.p; }
    if (s->d_dBetaFI.n != (size_t)N) { std::vector<double> one(N, 1.0); s->d_dBetaFI.upload(one); }
    struct Restore { das_solver* s; ~Restore() { s->cp.dBetaFI_ptr = nullptr; } } restore{s};
    s->cp.dBetaFI_ptr = s->d_dBetaFI.p;
    ResParams prm = make_params(s->cp, s->opt, 0);
    if (s->d_Wd.n != (size_t)n) { s->d_Wd.alloc(n); s->d_Rd.alloc(n); }
    hipLaunchKernelGGL(k_lift, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_W.p, s->d_Wd.p);  // states carry no tangent
    eval_residual<Dual<1>>(s->dm, s->cp, prm, s->d_Wd.p, s->d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
    DAS_HIP(hipMemcpyAsync(s->d_tmp2.p, seeds, n * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_field_product, dim3(nblk(N, B)), dim3(B), 0, st, N, (long long)prm.offN * N, s->d_Rd.p, s->d_tmp2.p, s->d_tmp1.p);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(product, s->d_tmp1.p, N * sizeof(double), hipMemcpyDeviceToHost, st));
    DAS_HIP(hipStreamSynchronize(st));
    return DAS_OK;
    DAS_CATCH
}

// ---- mesh-sensitivity product over all points (das_volcoord.hpp) -----------------------------------------------------
static GeomTopo device_geom_topo(das_solver* s) {
    das_solver::VolCoord& v = s->vc;
    const Mesh& m = s->mesh;
    if (v.d_face_ptr.n != m.face_ptr.size()) { v.d_face_ptr.upload(m.face_ptr); v.d_face_pts.upload(m.face_pts); v.d_bad.alloc(1); }
    GeomTopo t;
    t.nC = m.nC; t.nF = m.nF; t.nIF = m.nIF;
    t.face_ptr = v.d_face_ptr.p; t.face_pts = v.d_face_pts.p;
    t.owner = s->d_owner.p; t.neigh = s->d_neigh.p;
    t.cf_ptr = s->d_cf_ptr.p; t.cf_face = s->d_cf_face.p;
    t.bpatch = s->d_bpatch.p; t.cyc = s->d_cyc.p; t.bc = s->d_bc.p;
    return t;
}
// the three metric passes on the device: points X -> s->d_fg / s->d_cg (frozen wall distance kept)
static void device_geometry(das_solver* s, const GeomTopo& t, const double* X) {
    const int B = 256;
    hipStream_t st = s->stream;
    hipLaunchKernelGGL(k_geom_face<double>, dim3(nblk(t.nF, B)), dim3(B), 0, st, t, X, s->d_fg.p);
    hipLaunchKernelGGL(k_geom_cell<double>, dim3(nblk(t.nC, B)), dim3(B), 0, st, t, (const FaceGeom*)s->d_fg.p, s->d_cg.p, s->vc.d_bad.p);
    hipLaunchKernelGGL(k_geom_weights<double>, dim3(nblk(t.nF, B)), dim3(B), 0, st, t, (const CellGeom*)s->d_cg.p, s->d_fg.p);
}
static void ensure_point_influence(das_solver* s) {
    das_solver::VolCoord& v = s->vc;
    const int rings = (int)s->opt.geti("amd.volCoordRings");
    const double rel = s->opt.getd("amd.volCoordRelStep");
    DAS_CHECK(rings >= 1 && rel > 0, DAS_ERR_ARG, "amd.volCoordRings >= 1 and amd.volCoordRelStep > 0 expected");
    if (!(v.built && v.inf.rings == rings)) {  // topology only: survives mesh updates
        const double t0 = wall_seconds();
        build_point_influence(s->mesh, rings, (int)s->opt.geti("amd.setupThreads"), v.inf);
        v.built = true;
        v.uploaded = false;
        v.hGeom = -1;
        v.buildSeconds = wall_seconds() - t0;
    }
    if (v.relStep != rel || v.hGeom != s->geomVersion) {
        point_steps(s->mesh, rel, v.inf.h);
        v.relStep = rel;
        v.hGeom = s->geomVersion;
        if (s->inited) v.d_h.upload(v.inf.h);
    }
    if (s->inited && !v.uploaded) {
        v.d_ptr.upload(v.inf.ptr);
        v.d_cells.upload(v.inf.cells);
        v.d_cpoints.upload(v.inf.cpoints);
        v.d_h.upload(v.inf.h);
        v.uploaded = true;
    }
}
// debug / test aid: the metrics the DEVICE passes produce for `points`, without touching the solver's geometry
int das_debug_device_geometry(das_solver_t* s, const double* points, double* fg12, double* cg5) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(points && fg12 && cg5, DAS_ERR_ARG, "null argument");
    static_assert(sizeof(FaceGeom) == 12 * sizeof(double) && sizeof(CellGeom) == 5 * sizeof(double), "geometry records are plain doubles");
    const Mesh& m = s->mesh;
    das_solver::VolCoord& v = s->vc;
    const GeomTopo t = device_geom_topo(s);
    DAS_HIP(hipStreamSynchronize(s->stream));
    v.d_fg0.alloc(m.nF); v.d_cg0.alloc(m.nC);
    DAS_HIP(hipMemcpy(v.d_fg0.p, s->d_fg.p, m.nF * sizeof(FaceGeom), hipMemcpyDeviceToDevice));
    DAS_HIP(hipMemcpy(v.d_cg0.p, s->d_cg.p, m.nC * sizeof(CellGeom), hipMemcpyDeviceToDevice));
    v.d_X.upload(points, 3 * (size_t)m.nP);
    DAS_HIP(hipMemsetAsync(v.d_bad.p, 0, sizeof(int), s->stream));
    device_geometry(s, t, v.d_X.p);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipStreamSynchronize(s->stream));
    DAS_HIP(hipMemcpy(fg12, s->d_fg.p, m.nF * sizeof(FaceGeom), hipMemcpyDeviceToHost));
    DAS_HIP(hipMemcpy(cg5, s->d_cg.p, m.nC * sizeof(CellGeom), hipMemcpyDeviceToHost));
    DAS_HIP(hipMemcpy(s->d_fg.p, v.d_fg0.p, m.nF * sizeof(FaceGeom), hipMemcpyDeviceToDevice));
    DAS_HIP(hipMemcpy(s->d_cg.p, v.d_cg0.p, m.nC * sizeof(CellGeom), hipMemcpyDeviceToDevice));
    v.d_fg0.release(); v.d_cg0.release();
    return DAS_OK;
    DAS_CATCH
}
// host-side (no GPU needed): the aggregates amd.pcCoarseAggregation "strength" would use for at most maxAgg aggregates
int das_debug_strength_aggregates(das_solver_t* s, int maxAgg, int* agg, int* nAgg) {
    DAS_TRY
    DAS_CHECK(s && agg && nAgg && maxAgg >= 1, DAS_ERR_ARG, "bad argument");
    std::vector<int> a;
    *nAgg = strength_aggregates(s->mesh, nullptr, maxAgg, a);
    std::copy(a.begin(), a.end(), agg);
    return DAS_OK;
    DAS_CATCH
}
// host-side structure of the product (no GPU needed): sizes, then colours / influence sets / steps
int das_point_influence_build(das_solver_t* s, int* nColors, long long* nEntries) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    ensure_point_influence(s);
    if (nColors) *nColors = s->vc.inf.nColors;
    if (nEntries) *nEntries = (long long)s->vc.inf.cells.size();
    return DAS_OK;
    DAS_CATCH
}
int das_point_influence_get(das_solver_t* s, int* colors, long long* ptr, int* cells, double* steps) {
    DAS_TRY
    DAS_CHECK(s && s->vc.built, DAS_ERR_STATE, "das_point_influence_build has not been called");
    const PointInfluence& I = s->vc.inf;
    if (colors) std::copy(I.color.begin(), I.color.end(), colors);
    if (ptr) std::copy(I.ptr.begin(), I.ptr.end(), ptr);
    if (cells) std::copy(I.cells.begin(), I.cells.end(), cells);
    if (steps) std::copy(I.h.begin(), I.h.end(), steps);
    return DAS_OK;
    DAS_CATCH
}
// ---- shared by the two modes of the product -----------------------------------------------------------------------------------
// cell -> slots of its function faces, as CSR
static void function_face_slots(const Mesh& m, const das_solver::FaceFn& fn, std::vector<int>& cptr, std::vector<int>& cidx) {
    const int nf = (int)fn.faces.size();
    cptr.assign(m.nC + 1, 0);
    cidx.resize(nf);
    for (int k = 0; k < nf; k++) cptr[m.owner[fn.faces[k]] + 1]++;
    for (int c = 0; c < m.nC; c++) cptr[c + 1] += cptr[c];
    std::vector<int> pos(cptr.begin(), cptr.end() - 1);
    for (int k = 0; k < nf; k++) cidx[pos[m.owner[fn.faces[k]]]++] = k;
}
// where the residual rows of each state block start (k_vc_rows / k_vc_rows_dual)
static RowLayout residual_row_layout(das_solver* s) {
    const Stencil stn = make_stencil(s->cp.solver, s->mesh.nC, s->mesh.nF, s->opt, false, s->cp.hasT != 0, s->reg_needs_p());
    DAS_CHECK(stn.states.size() <= 8, DAS_ERR_INTERNAL, "more than 8 state blocks");
    RowLayout L{};
    L.nb = (int)stn.states.size();
    for (int b = 0; b < L.nb; b++) { L.off[b] = stn.states[b].offset; L.kind[b] = (int)stn.states[b].kind; }
    return L;
}
// ---- heat sources of DAHeatTransferFoam (reference DAFvSourceHeatSource.C; kernels: das_heatsource.hpp) -----------------------------
static void need_heat_source_solver(das_solver* s) {
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    DAS_CHECK(s->cp.solver != DAS_SOLVER_SOLIDDISPLACEMENTFOAM, DAS_ERR_ARG, "the fvSource option is not built for DASolidDisplacementFoam");
    DAS_CHECK(s->cp.solver == DAS_SOLVER_HEATTRANSFERFOAM, DAS_ERR_ARG,
              "the fvSource heat sources (and the fvSourcePar input) are built for DAHeatTransferFoam only: no fvSource on a flow solver or on DAScalarTransportFoam");
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "the fvSource heat sources run on an undecomposed solver (sharded solvers are not supported)");
}
static das_solver::HeatSource& get_heat_source(das_solver* s, const char* name) {
    auto it = s->heatSources.find(name ? name : "");
    DAS_CHECK(it != s->heatSources.end(), DAS_ERR_ARG, std::string("fvSource has no heat source ") + (name ? name : "(null)"));
    return it->second;
}
extern "C++" {
template <class P>
static HsView<P> heat_source_view(const das_solver::HeatSource& h) {
    HsView<P> v;
    v.kind = h.kind; v.member = h.d_member.p; v.field = nullptr;
    for (int i = 0; i < 3; i++) { v.center[i] = P(h.pars[i]); v.axis[i] = P(h.pars[3 + i]); }
    v.radius = P(h.pars[6]); v.length = P(h.pars[7]); v.power = P(h.pars[8]);
    v.eps = h.eps; v.snapCell = h.snapCell;
    return v;
}
// out[0] = the two-stage sum of k_hs_partial / k_hs_final over all cells
template <class R, class P, class G>
static void heat_source_sum(das_solver* s, const HsView<P>& v, const CellGeomT<G>* cg, const double* psi, int byV, const R* vt, R* out) {
    if (s->d_hsPart.n < (size_t)DAS_HS_MAX_BLOCKS) s->d_hsPart.alloc(DAS_HS_MAX_BLOCKS);
    launch_hs_sum<R, P, G>(s->stream, v, s->mesh.nC, cg, psi, byV, vt, reinterpret_cast<R*>(s->d_hsPart.p), out);
}
}  // extern "C++"
static void refresh_heat_sources(das_solver* s, bool check) {
    if (s->heatSources.empty() || !s->inited) return;
    const int nC = s->mesh.nC, K = (int)s->heatSources.size();
    if (s->d_src.n != (size_t)nC) s->d_src.alloc(nC);
    if (s->d_hsVt.n < (size_t)K + 1) s->d_hsVt.alloc(K + 1);
    s->dm.src = s->d_src.p;
    const CellGeom* cg = s->d_cg.p;
    int k = 0;
    for (auto& e : s->heatSources) {
        das_solver::HeatSource& h = e.second;
        if (h.kind == DAS_HS_CYLINDERTOCELL && h.d_member.n != (size_t)nC) {
            std::vector<unsigned char> mask(nC, 0);
            for (int c : h.members) mask[c] = 1;
            h.d_member.upload(mask);
        }
        const HsView<double> v = heat_source_view<double>(h);
        heat_source_sum<double, double, double>(s, v, cg, nullptr, 0, nullptr, s->d_hsVt.p + k);
        hipLaunchKernelGGL((k_hs_apply<double, double, double>), dim3(nblk(nC, 256)), dim3(256), 0, s->stream, v, nC, cg, (const double*)(s->d_hsVt.p + k), (int)(k == 0),
                           s->d_src.p);
        k++;
    }
    HsView<double> fv{};
    fv.kind = DAS_HS_FIELD; fv.field = s->d_src.p; fv.snapCell = -1;
    heat_source_sum<double, double, double>(s, fv, cg, nullptr, 0, nullptr, s->d_hsVt.p + K);
    DAS_HIP(hipGetLastError());
    if (!check) return;
    std::vector<double> tot(K + 1);
    DAS_HIP(hipMemcpyAsync(tot.data(), s->d_hsVt.p, (K + 1) * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    k = 0;
    for (auto& e : s->heatSources) {
        DAS_CHECK(std::isfinite(tot[k]) && tot[k] != 0.0, DAS_ERR_ARG,
                  "fvSource " + e.first + ": the total volume of the heat source is " + std::to_string(tot[k]) + " (zero or not finite): the source reaches no cell");
        e.second.volumeTotal = tot[k++];
    }
    s->hsSourceTotal = tot[K];
}
// sum_c psi_c nrm_c dq_c / dpars[idx] of one cylinderSmooth source: one forward pass with Dual<1> parameters on the double mesh (s_c and
// Vt are dual; the residual body is not run: dR_c / dp = dq_c / dp, times V_c in the unnormalised row).  unsnap: a snapped centre is
// taken as the parameter it replaces, at its current place
static double heat_source_par_pass(das_solver* s, const das_solver::HeatSource& h, int idx, const double* d_psi, bool unsnap) {
    typedef Dual<1> D;
    HsView<D> v = heat_source_view<D>(h);
    if (unsnap && h.snapCell >= 0) {
        for (int i = 0; i < 3; i++) v.center[i] = D(s->mesh.cg[h.snapCell].C[i]);
        v.snapCell = -1;
    }
    D& p = idx < 3 ? v.center[idx] : (idx < 6 ? v.axis[idx - 3] : (idx == 6 ? v.radius : (idx == 7 ? v.length : v.power)));
    p.d[0] = 1.0;
    if (s->d_hsVtD.n < 2) s->d_hsVtD.alloc(2);
    const int byV = make_params(s->cp, s->opt, 0).normT ? 0 : 1;
    heat_source_sum<D, D, double>(s, v, (const CellGeom*)s->d_cg.p, nullptr, 0, nullptr, s->d_hsVtD.p);
    heat_source_sum<D, D, double>(s, v, (const CellGeom*)s->d_cg.p, d_psi, byV, (const D*)s->d_hsVtD.p, s->d_hsVtD.p + 1);
    DAS_HIP(hipGetLastError());
    D r;
    DAS_HIP(hipMemcpyAsync(&r, s->d_hsVtD.p + 1, sizeof(D), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return r.d[0];
}

// das_define_heat_source <- one entry of the fvSource option, type heatSource (DAFvSourceHeatSource.C:30-128)
int das_define_heat_source(das_solver_t* s, const char* name, const char* kind, const double* pars, double eps, int snapCenter2Cell) {
    DAS_TRY
    need_heat_source_solver(s);
    DAS_CHECK(name && kind && pars, DAS_ERR_ARG, "fvSource: null argument");
    const std::string nm = name, kd = kind, what = "fvSource " + nm;
    const Mesh& m = s->mesh;
    das_solver::HeatSource h;
    if (kd == "cylinderToCell") {
        // OpenFOAM's cylinderToCell on the cell centres of this moment: between the two end planes and within the radius of the axis
        h.kind = DAS_HS_CYLINDERTOCELL;
        const double* p1 = pars;
        const double* p2 = pars + 3;
        const double radius = pars[6], a[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
        const double aa = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
        DAS_CHECK(aa > 0.0 && radius > 0.0 && std::isfinite(pars[7]), DAS_ERR_ARG, what + ": cylinderToCell needs p1 != p2, radius > 0 and a finite power");
        for (int c = 0; c < m.nC; c++) {
            const double d[3] = {m.cg[c].C[0] - p1[0], m.cg[c].C[1] - p1[1], m.cg[c].C[2] - p1[2]};
            const double mg = d[0] * a[0] + d[1] * a[1] + d[2] * a[2];
            if (mg > 0.0 && mg < aa && (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - mg * mg / aa < radius * radius) h.members.push_back(c);
        }
        DAS_CHECK(!h.members.empty(), DAS_ERR_ARG, what + ": cylinderToCell selects no cell (an empty set cannot carry the power)");
        for (int i = 0; i < 6; i++) h.pars[i] = pars[i];
        h.pars[6] = radius; h.pars[7] = std::sqrt(aa); h.pars[8] = pars[7];
    } else if (kd == "cylinderSmooth") {
        h.kind = DAS_HS_CYLINDERSMOOTH;
        for (int i = 0; i < 9; i++) h.pars[i] = pars[i];
        h.eps = eps;
        DAS_CHECK(eps > 0.0, DAS_ERR_ARG, what + ": cylinderSmooth needs eps > 0");
        DAS_CHECK(pars[3] * pars[3] + pars[4] * pars[4] + pars[5] * pars[5] > 0.0, DAS_ERR_ARG, what + ": cylinderSmooth needs a non-zero axis");
        if (snapCenter2Cell) {
            // primitiveMesh::findCell as DAUtility::myFindCell calls it: the cells whose face planes all have the point on their inner side
            int found = 0;
            for (int c = 0; c < m.nC; c++) {
                bool in = true;
                for (int q = m.cf_ptr[c]; q < m.cf_ptr[c + 1] && in; q++) {
                    const int fe = m.cf_face[q], f = fe & 0x7fffffff;
                    const FaceGeom& g = m.fg[f];
                    const double dot = (pars[0] - g.Cf[0]) * g.Sf[0] + (pars[1] - g.Cf[1]) * g.Sf[1] + (pars[2] - g.Cf[2]) * g.Sf[2];
                    in = (fe < 0 ? -dot : dot) <= 0.0;
                }
                if (in) { found++; h.snapCell = c; }
            }
            DAS_CHECK(found == 1, DAS_ERR_ARG,
                      what + ": snapCenter2Cell: there should be only one cell found while " + std::to_string(found)
                          + " was returned. Please adjust center such that it is located completely within a cell in the mesh domain. The center should not be "
                            "outside of the mesh domain or on a mesh face");
        }
    } else {
        DAS_CHECK(false, DAS_ERR_ARG, what + ": source: " + kd + " not supported! Options are: cylinderToCell and cylinderSmooth!");
    }
    s->heatSources.erase(nm);
    s->heatSources.emplace(nm, std::move(h));
    refresh_heat_sources(s, true);
    return DAS_OK;
    DAS_CATCH
}
// das_set_heat_source_pars <- DAInputFvSourcePar::run (DAInputFvSourcePar.C:75-140): heatSourcePars[indices[k]] = values[k], then updateFvSource
int das_set_heat_source_pars(das_solver_t* s, const char* name, const int* indices, int n, const double* values) {
    DAS_TRY
    need_heat_source_solver(s);
    DAS_CHECK(indices && values && n >= 0, DAS_ERR_ARG, "fvSourcePar: null argument");
    das_solver::HeatSource& h = get_heat_source(s, name);
    DAS_CHECK(h.kind == DAS_HS_CYLINDERSMOOTH, DAS_ERR_ARG,
              std::string("fvSourcePar: fvSource ") + name + " is a cylinderToCell source; heatSourcePars exist for cylinderSmooth sources only");
    for (int k = 0; k < n; k++)
        DAS_CHECK(indices[k] >= 0 && indices[k] < 9, DAS_ERR_ARG,
                  std::string("fvSourcePar: index ") + std::to_string(indices[k]) + " of fvSource " + name + " is out of range (a heat source has 9 parameters)");
    for (int k = 0; k < n; k++) h.pars[indices[k]] = values[k];
    DAS_CHECK(h.pars[3] * h.pars[3] + h.pars[4] * h.pars[4] + h.pars[5] * h.pars[5] > 0.0, DAS_ERR_ARG, std::string("fvSource ") + name + ": cylinderSmooth needs a non-zero axis");
    refresh_heat_sources(s, true);
    return DAS_OK;
    DAS_CATCH
}
int das_get_heat_source_info(das_solver_t* s, const char* name, double* pars9, double* volumeTotal, double* sourceTotal, int* snappedCell) {
    DAS_TRY
    need_heat_source_solver(s);
    const das_solver::HeatSource& h = get_heat_source(s, name);
    if (pars9) std::copy(h.pars, h.pars + 9, pars9);
    if (volumeTotal) *volumeTotal = h.volumeTotal;
    if (sourceTotal) *sourceTotal = s->hsSourceTotal;
    if (snappedCell) *snappedCell = h.snapCell;
    return DAS_OK;
    DAS_CATCH
}
// the cells of a cylinderToCell source (cap entries at most are written); returns their number
int das_get_heat_source_cells(das_solver_t* s, const char* name, int* cells, int cap) {
    DAS_TRY
    need_heat_source_solver(s);
    const das_solver::HeatSource& h = get_heat_source(s, name);
    if (cells) std::copy(h.members.begin(), h.members.begin() + std::min((size_t)std::max(cap, 0), h.members.size()), cells);
    return (int)h.members.size();
    DAS_CATCH
}
int das_get_fv_source(das_solver_t* s, double* out) {
    DAS_TRY
    need_heat_source_solver(s);
    need_init(s);
    DAS_CHECK(out, DAS_ERR_ARG, "null argument");
    if (s->heatSources.empty()) { std::fill(out, out + s->mesh.nC, 0.0); return DAS_OK; }
    DAS_HIP(hipMemcpyAsync(out, s->d_src.p, (size_t)s->mesh.nC * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return DAS_OK;
    DAS_CATCH
}
// das_calc_dfvsourcepar_product <- calcJacTVecProduct(name, "fvSourcePar", ...) after the input has been set: product[k] =
// seeds . d output / d heatSourcePars[indices[k]].  No function and no coupling output reads the source: exact zeros without a pass.  The
// first three parameters of a snapped source are not read either.
int das_calc_dfvsourcepar_product(das_solver_t* s, const char* name, const int* indices, int n, const char* outputName, const char* outputType,
                                  const double* seeds, double* product) {
    DAS_TRY
    need_heat_source_solver(s);
    need_init(s);
    DAS_CHECK(indices && outputType && seeds && product && n >= 0, DAS_ERR_ARG, "fvSourcePar: null argument");
    const das_solver::HeatSource& h = get_heat_source(s, name);
    DAS_CHECK(h.kind == DAS_HS_CYLINDERSMOOTH, DAS_ERR_ARG,
              std::string("fvSourcePar: fvSource ") + name + " is a cylinderToCell source; heatSourcePars exist for cylinderSmooth sources only");
    for (int k = 0; k < n; k++)
        DAS_CHECK(indices[k] >= 0 && indices[k] < 9, DAS_ERR_ARG,
                  std::string("fvSourcePar: index ") + std::to_string(indices[k]) + " of fvSource " + name + " is out of range (a heat source has 9 parameters)");
    std::string ot = outputType;
    std::vector<double> rnSeeds;  // a residualNorm function: the residual product with the seeds dF/dR
    residual_norm_redirect(s, outputName, ot, seeds, rnSeeds);
    DAS_CHECK(ot == "residual" || ot == "function" || is_coupling(ot), DAS_ERR_ARG, "outputType not supported on this path: " + ot);
    if (ot != "residual") {
        if (is_coupling(ot)) (void)coupling_size(s, ot, outputName);
        else if (!find_cell_function(s, outputName) && !find_mesh_function(s, outputName)) (void)get_function(s, outputName);
        std::fill(product, product + n, 0.0);
        return DAS_OK;
    }
    DevBuf<double> d_psi;
    d_psi.upload(seeds, (size_t)s->n);
    for (int k = 0; k < n; k++) product[k] = (h.snapCell >= 0 && indices[k] < 3) ? 0.0 : heat_source_par_pass(s, h, indices[k], d_psi.p, false);
    return DAS_OK;
    DAS_CATCH
}

// The volCoord product and the heat sources.  A point moves the source of EVERY cell through the total Vt, and a snapped centre moves with
// its cell - neither fits the colouring, which lets a point reach the rows of its own influence set only.  Inside the coloured passes both
// are therefore frozen data; what they add is rank one per source and goes onto the per-cell tangents before the gather, as
// k_vc_cellfn_all does for divByTotalVol:
//   beta = -(power / Vt^2) sum_c psi_c s_c nrm_c   multiplies (s_c V_c)' of every cell          (nrm_c = 1, or V_c unnormalised)
//   gamma_j = sum_c psi_c nrm_c dq_c / dcenter_j   multiplies C_j' of the snapped cell          (the fvSourcePar pass, unsnapped)
// view: the source with its centre where it is now and no snapped cell - the frozen form the passes evaluate
struct HsRank1 { HsView<double> view; int snapCell; double beta, gamma[3]; };
static void heat_source_rank1_terms(das_solver* s, const double* d_psi, int byV, std::vector<HsRank1>& terms) {
    for (auto& e : s->heatSources) {
        const das_solver::HeatSource& h = e.second;
        HsRank1 r{heat_source_view<double>(h), h.snapCell, 0.0, {0.0, 0.0, 0.0}};
        heat_source_sum<double, double, double>(s, r.view, (const CellGeom*)s->d_cg.p, d_psi, byV, nullptr, s->d_hsVt.p);
        double S = 0.0;
        DAS_HIP(hipMemcpyAsync(&S, s->d_hsVt.p, sizeof(double), hipMemcpyDeviceToHost, s->stream));
        DAS_HIP(hipStreamSynchronize(s->stream));
        r.beta = -h.pars[8] / (h.volumeTotal * h.volumeTotal) * S;
        if (h.snapCell >= 0) {
            for (int j = 0; j < 3; j++) {
                r.gamma[j] = heat_source_par_pass(s, h, j, d_psi, true);
                r.view.center[j] = s->mesh.cg[h.snapCell].C[j];
            }
            r.view.snapCell = -1;
        }
        terms.push_back(r);
    }
}

// ---- actuator disks of DASimpleFoam (reference DAFvSourceActuatorDisk.C; kernels: das_actuatordisk.hpp) -----------------------------
static void need_actuator_disk_solver(das_solver* s) {
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    DAS_CHECK(s->cp.solver != DAS_SOLVER_SOLIDDISPLACEMENTFOAM, DAS_ERR_ARG, "the fvSource option is not built for DASolidDisplacementFoam");
    DAS_CHECK(!s->cp.pimple, DAS_ERR_ARG, "DAPimpleFoam: fvSource is not built");
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SIMPLEFOAM, DAS_ERR_ARG,
              "the fvSource actuator disks are built for DASimpleFoam only: not for DARhoSimpleFoam (its fvSourceEnergy = fvSource . U is not built), DATurboFoam, "
              "DAScalarTransportFoam or DAHeatTransferFoam");
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "the fvSource actuator disks run on an undecomposed solver (sharded solvers are not supported)");
}
static das_solver::ActuatorDisk& get_actuator_disk(das_solver* s, const char* name) {
    auto it = s->actuatorDisks.find(name ? name : "");
    DAS_CHECK(it != s->actuatorDisks.end(), DAS_ERR_ARG, std::string("fvSource has no actuator disk ") + (name ? name : "(null)"));
    return it->second;
}
static void check_actuator_disk_pars(const das_solver::ActuatorDisk& a, const std::string& what) {
    const double* p = a.pars;
    DAS_CHECK(p[3] * p[3] + p[4] * p[4] + p[5] * p[5] > 0.0, DAS_ERR_ARG, what + ": the direction (p2 - p1) must not be zero");
    DAS_CHECK(p[7] > p[6] && p[6] >= 0.0, DAS_ERR_ARG, what + ": 0 <= innerRadius < outerRadius is needed");
    for (int i = 0; i < 13; i++) DAS_CHECK(std::isfinite(p[i]), DAS_ERR_ARG, what + ": a parameter is not finite");
    if (a.smooth) DAS_CHECK(a.eps > 0.0 && 2.0 * a.eps < p[7] - p[6], DAS_ERR_ARG, what + ": cylinderAnnulusSmooth needs 0 < eps < (outerRadius - innerRadius) / 2");
}
extern "C++" {
template <class P>
static AdView<P> actuator_disk_view(const das_solver::ActuatorDisk& a) {
    AdView<P> v;
    v.smooth = a.smooth; v.adjustThrust = a.adjustThrust; v.member = a.smooth ? nullptr : a.d_member.p;
    for (int i = 0; i < 3; i++) { v.center[i] = P(a.pars[i]); v.direction[i] = P(a.pars[3 + i]); }
    v.innerRadius = P(a.pars[6]); v.outerRadius = P(a.pars[7]); v.scale = P(a.pars[8]); v.POD = P(a.pars[9]);
    v.expM = P(a.pars[10]); v.expN = P(a.pars[11]); v.targetThrust = P(a.pars[12]);
    v.eps = a.eps; v.rotSign = a.rotSign;
    return v;
}
// the parameter idx of a dual view
static Dual<1>& actuator_disk_par(AdView<Dual<1>>& v, int idx) {
    if (idx < 3) return v.center[idx];
    if (idx < 6) return v.direction[idx - 3];
    Dual<1>* rest[7] = {&v.innerRadius, &v.outerRadius, &v.scale, &v.POD, &v.expM, &v.expN, &v.targetThrust};
    return *rest[idx - 6];
}
// out2 = {sum fAxial V, sum fCirc V} at the scale scale[0] (null: 1) through k_ad_partial / k_ad_final
template <class R, class P, class G>
static void actuator_disk_sums(das_solver* s, const AdView<P>& v, const CellGeomT<G>* cg, const R* scale, R* out2) {
    if (s->d_adPart.n < (size_t)2 * DAS_HS_MAX_BLOCKS) s->d_adPart.alloc((size_t)2 * DAS_HS_MAX_BLOCKS);
    launch_ad_sums<R, P, G>(s->stream, v, s->mesh.nC, cg, scale, reinterpret_cast<R*>(s->d_adPart.p), out2);
}
// the whole field of the disks views[0..K) into src3 (3 nC); work: 5 slots per disk {unit sums(2), scale, sums(2)}; withSums: the
// thrust and torque sums at the effective scale as well
template <class R, class P, class G>
static void actuator_disk_field(das_solver* s, const std::vector<AdView<P>>& views, const CellGeomT<G>* cg, R* work, R* src3, bool withSums) {
    const int nC = s->mesh.nC;
    if (s->d_adBad.n < 1) { s->d_adBad.alloc(1); DAS_HIP(hipMemsetAsync(s->d_adBad.p, 0, sizeof(int), s->stream)); }
    for (size_t k = 0; k < views.size(); k++) {
        R* w = work + 5 * k;
        if (views[k].adjustThrust) actuator_disk_sums<R, P, G>(s, views[k], cg, (const R*)nullptr, w);
        hipLaunchKernelGGL((k_ad_scale<R, P>), dim3(1), dim3(64), 0, s->stream, views[k], (const R*)w, w + 2);
        hipLaunchKernelGGL((k_ad_apply<R, P, G>), dim3(nblk(nC, 256)), dim3(256), 0, s->stream, views[k], nC, cg, (const R*)(w + 2), (int)(k == 0), src3, s->d_adBad.p);
        if (withSums) actuator_disk_sums<R, P, G>(s, views[k], cg, (const R*)(w + 2), w + 3);
    }
}
}  // extern "C++"
static void refresh_actuator_disks(das_solver* s, bool check) {
    if (s->actuatorDisks.empty() || !s->inited) return;
    const int nC = s->mesh.nC, K = (int)s->actuatorDisks.size();
    if (s->d_src3.n != (size_t)3 * nC) s->d_src3.alloc((size_t)3 * nC);
    if (s->d_adSums.n < (size_t)5 * K) s->d_adSums.alloc((size_t)5 * K);
    DAS_HIP(hipMemsetAsync(s->d_adSums.p, 0, (size_t)5 * K * sizeof(double), s->stream));
    s->dm.src3 = s->d_src3.p;
    std::vector<AdView<double>> views;
    for (auto& e : s->actuatorDisks) {
        das_solver::ActuatorDisk& a = e.second;
        if (!a.smooth && a.d_member.n != (size_t)nC) {
            std::vector<unsigned char> mask(nC, 0);
            for (int c : a.members) mask[c] = 1;
            a.d_member.upload(mask);
        }
        views.push_back(actuator_disk_view<double>(a));
    }
    if (s->d_adBad.n < 1) s->d_adBad.alloc(1);
    DAS_HIP(hipMemsetAsync(s->d_adBad.p, 0, sizeof(int), s->stream));
    actuator_disk_field<double, double, double>(s, views, (const CellGeom*)s->d_cg.p, s->d_adSums.p, s->d_src3.p, true);
    DAS_HIP(hipGetLastError());
    if (!check) return;
    std::vector<double> w((size_t)5 * K);
    int bad = 0;
    DAS_HIP(hipMemcpyAsync(w.data(), s->d_adSums.p, w.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipMemcpyAsync(&bad, s->d_adBad.p, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    int k = 0;
    for (auto& e : s->actuatorDisks) {
        das_solver::ActuatorDisk& a = e.second;
        a.unitThrust = w[5 * k]; a.scale = w[5 * k + 2]; a.thrustSum = w[5 * k + 3]; a.torqueSum = w[5 * k + 4];
        DAS_CHECK(!a.adjustThrust || (std::isfinite(a.scale) && a.unitThrust != 0.0), DAS_ERR_ARG,
                  "fvSource " + e.first + ": adjustThrust: the thrust at scale 1 is " + std::to_string(a.unitThrust) + " (zero or not finite): the disk reaches no cell");
        k++;
    }
    DAS_CHECK(!bad, DAS_ERR_ARG,
              "fvSource actuatorDisk: a cell centre sits on the axis of a disk (its radial part is exactly zero): the reference divides by zero there; move the "
              "centre off the cell centres");
}

// das_define_actuator_disk <- one entry of the fvSource option, type actuatorDisk (DAFvSourceActuatorDisk.C:36-92 the cell set, :431-500 the
// parameters)
int das_define_actuator_disk(das_solver_t* s, const char* name, const char* kind, const double* pars, const char* rotDir, double eps, int adjustThrust) {
    DAS_TRY
    need_actuator_disk_solver(s);
    DAS_CHECK(name && kind && pars && rotDir, DAS_ERR_ARG, "fvSource: null argument");
    const std::string nm = name, kd = kind, rd = rotDir, what = "fvSource " + nm;
    const Mesh& m = s->mesh;
    das_solver::ActuatorDisk a;
    DAS_CHECK(rd == "left" || rd == "right", DAS_ERR_ARG, what + ": rotDir not valid: " + rd + " (left or right)");
    a.rotSign = rd == "left" ? 1.0 : -1.0;
    if (kd == "cylinderAnnulusToCell") {
        // pars = p1(3), p2(3), innerRadius, outerRadius, scale, POD.  OpenFOAM's cylinderAnnulusToCell on the cell centres of this moment:
        // between the two end planes and between the two radii of the axis
        a.smooth = 0;
        const double* p1 = pars;
        const double* p2 = pars + 3;
        const double ax[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
        const double aa = ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2], ir2 = pars[6] * pars[6], or2 = pars[7] * pars[7];
        for (int i = 0; i < 3; i++) { a.pars[i] = 0.5 * (p1[i] + p2[i]); a.pars[3 + i] = ax[i]; }
        for (int i = 6; i < 10; i++) a.pars[i] = pars[i];
        check_actuator_disk_pars(a, what);
        for (int c = 0; c < m.nC; c++) {
            const double d[3] = {m.cg[c].C[0] - p1[0], m.cg[c].C[1] - p1[1], m.cg[c].C[2] - p1[2]};
            const double mg = d[0] * ax[0] + d[1] * ax[1] + d[2] * ax[2];
            if (mg > 0.0 && mg < aa) {
                const double d2 = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) - mg * mg / aa;
                if (d2 < or2 && d2 > ir2) a.members.push_back(c);
            }
        }
        DAS_CHECK(!a.members.empty(), DAS_ERR_ARG, what + ": cylinderAnnulusToCell selects no cell (an empty set carries no force)");
    } else if (kd == "cylinderAnnulusSmooth") {
        a.smooth = 1;
        for (int i = 0; i < 13; i++) a.pars[i] = pars[i];
        a.eps = eps;
        a.adjustThrust = adjustThrust ? 1 : 0;
        check_actuator_disk_pars(a, what);
    } else {
        DAS_CHECK(false, DAS_ERR_ARG, what + ": source: " + kd + " not supported! Options are: cylinderAnnulusToCell and cylinderAnnulusSmooth!");
    }
    // a disk that cannot be evaluated is not kept, and a refused redefinition leaves the earlier disk of that name as it was
    auto old = s->actuatorDisks.extract(nm);
    s->actuatorDisks.emplace(nm, std::move(a));
    try {
        refresh_actuator_disks(s, true);
    } catch (...) {
        s->actuatorDisks.erase(nm);
        if (!old.empty()) s->actuatorDisks.insert(std::move(old));
        if (s->actuatorDisks.empty()) s->dm.src3 = nullptr;
        else try { refresh_actuator_disks(s, false); } catch (...) {}
        throw;
    }
    return DAS_OK;
    DAS_CATCH
}
// das_set_actuator_disk_pars <- DAInputFvSourcePar::run (DAInputFvSourcePar.C:75-140): actuatorDiskPars[indices[k]] = values[k], then updateFvSource
int das_set_actuator_disk_pars(das_solver_t* s, const char* name, const int* indices, int n, const double* values) {
    DAS_TRY
    need_actuator_disk_solver(s);
    DAS_CHECK(indices && values && n >= 0, DAS_ERR_ARG, "fvSourcePar: null argument");
    das_solver::ActuatorDisk& a = get_actuator_disk(s, name);
    DAS_CHECK(a.smooth, DAS_ERR_ARG,
              std::string("fvSourcePar: fvSource ") + name + " is a cylinderAnnulusToCell disk; actuatorDiskPars exist for cylinderAnnulusSmooth disks only");
    for (int k = 0; k < n; k++)
        DAS_CHECK(indices[k] >= 0 && indices[k] < 13, DAS_ERR_ARG,
                  std::string("fvSourcePar: index ") + std::to_string(indices[k]) + " of fvSource " + name + " is out of range (an actuator disk has 13 parameters)");
    das_solver::ActuatorDisk trial;
    trial.smooth = 1; trial.eps = a.eps;
    std::copy(a.pars, a.pars + 13, trial.pars);
    for (int k = 0; k < n; k++) trial.pars[indices[k]] = values[k];
    check_actuator_disk_pars(trial, std::string("fvSource ") + name);
    // parameters whose field cannot be evaluated (a cell centre on the axis, no thrust at scale 1) are not kept either
    double before[13];
    std::copy(a.pars, a.pars + 13, before);
    std::copy(trial.pars, trial.pars + 13, a.pars);
    try {
        refresh_actuator_disks(s, true);
    } catch (...) {
        std::copy(before, before + 13, a.pars);
        try { refresh_actuator_disks(s, false); } catch (...) {}
        throw;
    }
    return DAS_OK;
    DAS_CATCH
}
// info4 = {the effective scale, thrustSourceSum, torqueSourceSum, the thrust at scale 1 (adjustThrust; 0 otherwise)}
int das_get_actuator_disk_info(das_solver_t* s, const char* name, double* pars13, double* info4, int* nCells) {
    DAS_TRY
    need_actuator_disk_solver(s);
    const das_solver::ActuatorDisk& a = get_actuator_disk(s, name);
    if (pars13) std::copy(a.pars, a.pars + 13, pars13);
    if (info4) { info4[0] = a.scale; info4[1] = a.thrustSum; info4[2] = a.torqueSum; info4[3] = a.unitThrust; }
    if (nCells) *nCells = a.smooth ? s->mesh.nC : (int)a.members.size();
    return DAS_OK;
    DAS_CATCH
}
// the cells of a cylinderAnnulusToCell disk (cap entries at most are written); returns their number (a smooth disk: 0, it has no set)
int das_get_actuator_disk_cells(das_solver_t* s, const char* name, int* cells, int cap) {
    DAS_TRY
    need_actuator_disk_solver(s);
    const das_solver::ActuatorDisk& a = get_actuator_disk(s, name);
    if (cells) std::copy(a.members.begin(), a.members.begin() + std::min((size_t)std::max(cap, 0), a.members.size()), cells);
    return (int)a.members.size();
    DAS_CATCH
}
int das_get_fv_source_vector(das_solver_t* s, double* out) {
    DAS_TRY
    need_actuator_disk_solver(s);
    need_init(s);
    DAS_CHECK(out, DAS_ERR_ARG, "null argument");
    if (s->actuatorDisks.empty()) { std::fill(out, out + 3 * (size_t)s->mesh.nC, 0.0); return DAS_OK; }
    DAS_HIP(hipMemcpyAsync(out, s->d_src3.p, 3 * (size_t)s->mesh.nC * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return DAS_OK;
    DAS_CATCH
}

// The dual-metrics residual with NO point seeded: the metrics of the solver lifted to Dual<1> with zero tangents.  It is the vehicle of
// fvSourcePar -> residual: the residual is affine in the source field but the factor (rAU in HbyA, phiHbyA, pRes, phiRes) depends on the
// states, so the tangent of the field is pushed through the whole residual body rather than added to the U rows.
struct AdDualResidual {
    typedef Dual<1> D;
    DevBuf<D> d_XD, d_Wd, d_Rd, d_src3D, d_work;
    DevBuf<FaceGeomT<D>> d_fgD;
    DevBuf<CellGeomT<D>> d_cgD;
    DevBuf<double> d_X0, d_psi, d_part, d_out;
    DevMeshT<D> dmD;
    ResParams prm0;
    void init(das_solver* s, const double* seeds) {
        const Mesh& m = s->mesh;
        const GeomTopo t = device_geom_topo(s);
        hipStream_t st = s->stream;
        const int B = 256;
        const size_t n3 = 3 * (size_t)m.nP;
        d_XD.alloc(n3); d_Wd.alloc((size_t)s->n); d_Rd.alloc((size_t)s->n); d_src3D.alloc(3 * (size_t)m.nC); d_work.alloc(5 * s->actuatorDisks.size());
        d_fgD.alloc((size_t)m.nF); d_cgD.alloc((size_t)m.nC);
        d_X0.upload(m.points.data(), n3);
        d_psi.upload(seeds, (size_t)s->n);
        d_part.alloc(DAS_HS_MAX_BLOCKS); d_out.alloc(1);
        DAS_HIP(hipMemsetAsync(s->vc.d_bad.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_points_lift, dim3(nblk((long long)n3, B)), dim3(B), 0, st, (long long)n3, (const double*)d_X0.p, d_XD.p);
        hipLaunchKernelGGL(k_cell_y, dim3(nblk(m.nC, B)), dim3(B), 0, st, m.nC, (const CellGeom*)s->d_cg.p, d_cgD.p);
        hipLaunchKernelGGL(k_lift, dim3(nblk(s->n, B)), dim3(B), 0, st, s->n, s->d_W.p, d_Wd.p);
        hipLaunchKernelGGL(k_geom_face<D>, dim3(nblk(t.nF, B)), dim3(B), 0, st, t, (const D*)d_XD.p, d_fgD.p);
        hipLaunchKernelGGL(k_geom_cell<D>, dim3(nblk(t.nC, B)), dim3(B), 0, st, t, (const FaceGeomT<D>*)d_fgD.p, d_cgD.p, s->vc.d_bad.p);
        hipLaunchKernelGGL(k_geom_weights<D>, dim3(nblk(t.nF, B)), dim3(B), 0, st, t, (const CellGeomT<D>*)d_cgD.p, d_fgD.p);
        dmD.nC = m.nC; dmD.nF = m.nF; dmD.nIF = m.nIF;
        dmD.fg = d_fgD.p; dmD.cg = d_cgD.p;
        dmD.cf_ptr = s->dm.cf_ptr; dmD.cf_face = s->dm.cf_face; dmD.cf_other = s->dm.cf_other;
        dmD.owner = s->dm.owner; dmD.neigh = s->dm.neigh; dmD.bpatch = s->dm.bpatch; dmD.bc = s->dm.bc; dmD.cyc = s->dm.cyc; dmD.mixed = s->dm.mixed;
        dmD.src3 = d_src3D.p;
        prm0 = make_params(s->cp, s->opt, 0);
    }
    // seeds . dR / d(parameter idx of the disk `name`); unitScale: d / d(the effective scale) instead, whatever sets it (the rank-one
    // factor of the volCoord product)
    double pass(das_solver* s, const std::string& name, int idx, bool unitScale) {
        hipStream_t st = s->stream;
        std::vector<AdView<D>> views;
        for (auto& e : s->actuatorDisks) {
            AdView<D> v = actuator_disk_view<D>(e.second);
            if (e.first == name) {
                if (unitScale) { v.adjustThrust = 0; v.scale = D(e.second.scale); v.scale.d[0] = 1.0; }
                else actuator_disk_par(v, idx).d[0] = 1.0;
            }
            views.push_back(v);
        }
        actuator_disk_field<D, D, double>(s, views, (const CellGeom*)s->d_cg.p, d_work.p, d_src3D.p, false);
        eval_residual<D, D>(dmD, s->cp, prm0, d_Wd.p, d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
        launch_ad_dot(st, (long long)s->n, (const double*)d_psi.p, (const D*)d_Rd.p, d_part.p, d_out.p);
        DAS_HIP(hipGetLastError());
        double r = 0.0;
        DAS_HIP(hipMemcpyAsync(&r, d_out.p, sizeof(double), hipMemcpyDeviceToHost, st));
        DAS_HIP(hipStreamSynchronize(st));
        return r;
    }
};

// das_calc_dactuatordiskpar_product <- calcJacTVecProduct(name, "fvSourcePar", ...) after the input has been set: product[k] =
// seeds . d output / d actuatorDiskPars[indices[k]].  No function and no coupling output reads the source: exact zeros without a pass.
// Neither does anything read scale (index 8) with adjustThrust, or targetThrust (12) without.
int das_calc_dactuatordiskpar_product(das_solver_t* s, const char* name, const int* indices, int n, const char* outputName, const char* outputType,
                                      const double* seeds, double* product) {
    DAS_TRY
    need_actuator_disk_solver(s);
    need_init(s);
    DAS_CHECK(indices && outputType && seeds && product && n >= 0, DAS_ERR_ARG, "fvSourcePar: null argument");
    const das_solver::ActuatorDisk& a = get_actuator_disk(s, name);
    DAS_CHECK(a.smooth, DAS_ERR_ARG,
              std::string("fvSourcePar: fvSource ") + name + " is a cylinderAnnulusToCell disk; actuatorDiskPars exist for cylinderAnnulusSmooth disks only");
    for (int k = 0; k < n; k++)
        DAS_CHECK(indices[k] >= 0 && indices[k] < 13, DAS_ERR_ARG,
                  std::string("fvSourcePar: index ") + std::to_string(indices[k]) + " of fvSource " + name + " is out of range (an actuator disk has 13 parameters)");
    std::string ot = outputType;
    std::vector<double> rnSeeds;  // a residualNorm function: the residual product with the seeds dF/dR
    residual_norm_redirect(s, outputName, ot, seeds, rnSeeds);
    DAS_CHECK(ot == "residual" || ot == "function" || is_coupling(ot), DAS_ERR_ARG, "outputType not supported on this path: " + ot);
    if (ot != "residual") {
        if (is_coupling(ot)) (void)coupling_size(s, ot, outputName);
        else if (!find_cell_function(s, outputName) && !find_mesh_function(s, outputName)) (void)get_function(s, outputName);
        std::fill(product, product + n, 0.0);
        return DAS_OK;
    }
    AdDualResidual dr;
    dr.init(s, seeds);
    for (int k = 0; k < n; k++) {
        const bool unread = (indices[k] == 8 && a.adjustThrust) || (indices[k] == 12 && !a.adjustThrust);
        product[k] = unread ? 0.0 : dr.pass(s, name, indices[k], false);
    }
    return DAS_OK;
    DAS_CATCH
}

// The volCoord product and the disks.  The coloured passes recompute the field from the dual (or moved) C and V with the effective scale
// of every disk frozen; an adjustThrust disk adds the rank-one term of its total afterwards (k_ad_vc_rank1 / k_ad_fd_rank1).
struct AdRank1 { AdView<double> view; double beta; };
static void actuator_disk_volcoord_setup(das_solver* s, const double* seeds /* host */, std::vector<AdView<double>>& frozen, std::vector<AdRank1>& terms) {
    std::vector<std::string> adj;
    for (auto& e : s->actuatorDisks) {
        AdView<double> v = actuator_disk_view<double>(e.second);
        if (e.second.adjustThrust) adj.push_back(e.first);
        v.adjustThrust = 0;
        v.scale = e.second.scale;
        frozen.push_back(v);
    }
    if (adj.empty()) return;
    AdDualResidual dr;
    dr.init(s, seeds);
    for (const std::string& nm : adj) {
        const das_solver::ActuatorDisk& a = s->actuatorDisks[nm];
        const double gamma = dr.pass(s, nm, -1, true);
        terms.push_back(AdRank1{actuator_disk_view<double>(a), -(a.scale / a.unitThrust) * gamma});
    }
}

// the end of a product: the vector and the bad-volume flag come down, the timing goes into info4
static void finish_volcoord(das_solver* s, const double* d_out, double* product, const char* badMessage, double t0, long long passes, double* info4) {
    das_solver::VolCoord& v = s->vc;
    int bad = 0;
    DAS_HIP(hipMemcpyAsync(&bad, v.d_bad.p, sizeof(int), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipMemcpyAsync(product, d_out, 3 * (size_t)s->mesh.nP * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    DAS_CHECK(!bad, DAS_ERR_INTERNAL, badMessage);
    v.seconds = wall_seconds() - t0;
    if (info4) { info4[0] = v.inf.nColors; info4[1] = (double)passes; info4[2] = v.seconds; info4[3] = v.buildSeconds; }
}

// exact mode of the product (amd.volCoordMode "dual", the default): Dual<1> points -> Dual<1> metrics -> Dual<1> residual
static void volcoord_product_dual(das_solver* s, das_solver::FaceFn* fn, bool areaAvg, const double* cN, const double* cA, const double* seeds,
                                  double* product, double* info4, das_solver::CellFn* cfn = nullptr, das_solver::MeshFn* mq = nullptr) {
    typedef Dual<1> D;
    const Mesh& m = s->mesh;
    das_solver::VolCoord& v = s->vc;
    const PointInfluence& I = v.inf;
    const GeomTopo t = device_geom_topo(s);
    hipStream_t st = s->stream;
    const int B = 256;
    const long long n = s->n;
    const size_t n3 = 3 * (size_t)m.nP;
    const bool isFn = fn != nullptr, isCell = cfn != nullptr, isMq = mq != nullptr;
    const bool rho = DAS_IS_COMPRESSIBLE(s->cp.solver);
    // meshQualityKS: the linearised functional sum_f w_f a_f, w = seed x the softmax weights of the base mesh; k_mq_metric<Dual<1>> stores
    // w_f a_f' per face (d_fvd), k_mq_owner_gather adds the faces a cell owns into d_tc
    if (isMq) mesh_quality_weights(s, *mq, seeds[0]);
    // cell-set functions (variableVolSum): F0 = N / T with N = coef T sum_S w g, T = totalVol, so dF/dV_c = dF/dF0 ( [c in S, multiplyVol]
    // scale g_c / T - [divByTotalVol] F0 / T ): cellA multiplies V_c' on every cell, cellB g_c V_c' on the cells of the set
    double cellA = 0.0, cellB = 0.0;
    const bool isVm = isCell && cfn->vmKS;  // vonMisesStressKS: the linearised functional sum_c w_c vm_c on the dual metrics
    if (isVm) {
        vm_ks_cell_weights(s, *cfn, seeds[0]);
    } else if (isCell) {
        const double F0 = cell_function_base_value(s, *cfn);
        const double outer = seeds[0] * ref_var_outer(cfn->refVar, cfn->ref, F0);
        cellA = cfn->divByTotalVol ? -outer * F0 / cfn->totalVol : 0.0;
        cellB = cfn->multiplyVol ? outer * cfn->coef : 0.0;
    }
    DevBuf<double> d_X0, d_out(n3), d_tc((size_t)m.nC), d_seeds, d_fvd;
    DevBuf<D> d_XD(n3), d_Wd((size_t)n), d_Rd;
    DevBuf<FaceGeomT<D>> d_fgD((size_t)m.nF);
    DevBuf<CellGeomT<D>> d_cgD((size_t)m.nC);
    DevBuf<int> d_fnPtr, d_fnIdx;
    d_X0.upload(m.points.data(), n3);
    DAS_HIP(hipMemsetAsync(d_out.p, 0, n3 * sizeof(double), st));
    DAS_HIP(hipMemsetAsync(v.d_bad.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_points_lift, dim3(nblk((long long)n3, B)), dim3(B), 0, st, (long long)n3, (const double*)d_X0.p, d_XD.p);
    hipLaunchKernelGGL(k_cell_y, dim3(nblk(m.nC, B)), dim3(B), 0, st, m.nC, (const CellGeom*)s->d_cg.p, d_cgD.p);
    hipLaunchKernelGGL(k_lift, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_W.p, d_Wd.p);  // states carry no tangent
    DevMeshT<D> dmD;
    dmD.nC = m.nC; dmD.nF = m.nF; dmD.nIF = m.nIF;
    dmD.fg = d_fgD.p; dmD.cg = d_cgD.p;
    dmD.cf_ptr = s->dm.cf_ptr; dmD.cf_face = s->dm.cf_face; dmD.cf_other = s->dm.cf_other;
    dmD.owner = s->dm.owner; dmD.neigh = s->dm.neigh; dmD.bpatch = s->dm.bpatch; dmD.bc = s->dm.bc; dmD.cyc = s->dm.cyc; dmD.mixed = s->dm.mixed;
    ResParams prm0 = make_params(s->cp, s->opt, 0);
    RowLayout L{};
    int nf = 0;
    if (isMq) {
        d_fvd.alloc((size_t)m.nF);
    } else if (isCell) {
    } else if (!isFn) {
        L = residual_row_layout(s);
        d_Rd.alloc((size_t)n);
        d_seeds.upload(seeds, (size_t)n);
    } else {
        need_face_function_solver(s);
        nf = (int)fn->faces.size();
        d_fvd.alloc((size_t)nf);
        std::vector<int> cptr, cidx;
        function_face_slots(m, *fn, cptr, cidx);
        d_fnPtr.upload(cptr); d_fnIdx.upload(cidx);
    }
    // heat sources (residual rows only): the totals and a snapped centre are frozen inside the coloured passes (the dual src array carries
    // the local tangent through C_c and V_c of the cell itself) and come back as rank-one terms - heat_source_rank1_terms
    std::vector<HsRank1> hsTerms;
    DevBuf<D> d_srcD, d_vtD;
    if (!isMq && !isCell && !isFn && !s->heatSources.empty()) {
        heat_source_rank1_terms(s, d_seeds.p, prm0.normT ? 0 : 1, hsTerms);
        std::vector<D> vt;
        for (auto& e : s->heatSources) vt.push_back(D(e.second.volumeTotal));
        d_vtD.upload(vt);
        d_srcD.alloc((size_t)m.nC);
        dmD.src = d_srcD.p;
    }
    // actuator disks (residual rows only): the effective scales are frozen inside the coloured passes; an adjustThrust disk comes back
    // as a rank-one term - actuator_disk_volcoord_setup
    std::vector<AdView<double>> adFrozen;
    std::vector<AdRank1> adTerms;
    DevBuf<D> d_src3D, d_adWork;
    if (!isMq && !isCell && !isFn && !s->actuatorDisks.empty()) {
        actuator_disk_volcoord_setup(s, seeds, adFrozen, adTerms);
        d_src3D.alloc(3 * (size_t)m.nC);
        d_adWork.alloc(5 * adFrozen.size());
        dmD.src3 = d_src3D.p;
    }
    const double t0 = wall_seconds();
    long long passes = 0;
    for (int col = 0; col < I.nColors; col++) {
        const int np = I.cptr[col + 1] - I.cptr[col];
        if (np == 0) continue;
        const int* pts = v.d_cpoints.p + I.cptr[col];
        for (int axis = 0; axis < 3; axis++) {
            hipLaunchKernelGGL(k_points_seed, dim3(nblk(np, B)), dim3(B), 0, st, np, pts, axis, 1.0, d_XD.p);
            hipLaunchKernelGGL(k_geom_face<D>, dim3(nblk(t.nF, B)), dim3(B), 0, st, t, (const D*)d_XD.p, d_fgD.p);
            hipLaunchKernelGGL(k_geom_cell<D>, dim3(nblk(t.nC, B)), dim3(B), 0, st, t, (const FaceGeomT<D>*)d_fgD.p, d_cgD.p, v.d_bad.p);
            hipLaunchKernelGGL(k_geom_weights<D>, dim3(nblk(t.nF, B)), dim3(B), 0, st, t, (const CellGeomT<D>*)d_cgD.p, d_fgD.p);
            if (isMq) {
                hipLaunchKernelGGL(k_mq_metric<D>, dim3(nblk(t.nF, B)), dim3(B), 0, st, t, (const D*)d_XD.p, (const FaceGeomT<D>*)d_fgD.p, (const CellGeomT<D>*)d_cgD.p,
                                   mq->metric, (const double*)mq->d_w.p, d_fvd.p);
                launch_mq_owner_gather(st, m.nC, t.cf_ptr, t.cf_face, (const double*)d_fvd.p, d_tc.p);
            } else if (isVm) {
                const ResParams prm = s->wk1.bind(s->cp.solver, s->dm.nC, s->dm.nF, prm0);
                launch_solid_grad<D, D>(dmD, prm, (const D*)d_Wd.p, s->wk1, st);
                hipLaunchKernelGGL(k_vm_tangent, dim3(nblk(m.nC, B)), dim3(B), 0, st, m.nC, prm, (const D*)s->wk1.gU.p, cfn->scale, (const double*)cfn->d_wc.p, d_tc.p);
            } else if (isCell) {
                hipLaunchKernelGGL(k_vc_cellfn_all, dim3(nblk(m.nC, B)), dim3(B), 0, st, m.nC, (const CellGeomT<D>*)d_cgD.p, cellA, d_tc.p);
                if (cellB != 0.0 && !cfn->cell.empty())
                    hipLaunchKernelGGL(k_vc_cellfn_terms, dim3(nblk((long long)cfn->cell.size(), B)), dim3(B), 0, st, cfn->view(), (const CellGeomT<D>*)d_cgD.p,
                                       cell_function_src(s, *cfn), cellB, d_tc.p);
            } else if (!isFn) {
                for (size_t k = 0; k < hsTerms.size(); k++)
                    hipLaunchKernelGGL((k_hs_apply<D, double, D>), dim3(nblk(m.nC, B)), dim3(B), 0, st, hsTerms[k].view, m.nC, (const CellGeomT<D>*)d_cgD.p,
                                       (const D*)(d_vtD.p + k), (int)(k == 0), d_srcD.p);
                if (!adFrozen.empty()) actuator_disk_field<D, double, D>(s, adFrozen, (const CellGeomT<D>*)d_cgD.p, d_adWork.p, d_src3D.p, false);
                eval_residual<D, D>(dmD, s->cp, prm0, d_Wd.p, d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
                hipLaunchKernelGGL(k_vc_rows_dual, dim3(nblk(m.nC, B)), dim3(B), 0, st, s->dm, L, (const double*)d_seeds.p, (const D*)d_Rd.p, d_tc.p);
                for (const AdRank1& r : adTerms)
                    hipLaunchKernelGGL((k_ad_vc_rank1<double>), dim3(nblk(m.nC, B)), dim3(B), 0, st, r.view, m.nC, (const CellGeomT<D>*)d_cgD.p, r.beta, d_tc.p);
                for (const HsRank1& r : hsTerms)
                    hipLaunchKernelGGL(k_hs_vc_rank1, dim3(nblk(m.nC, B)), dim3(B), 0, st, r.view, m.nC, (const CellGeomT<D>*)d_cgD.p, r.snapCell, r.beta, r.gamma[0],
                                       r.gamma[1], r.gamma[2], d_tc.p);
            } else {
                const ResParams prm = s->wk1.bind(s->cp.solver, s->dm.nC, s->dm.nF, prm0);
                const bool isLoc = DAS_FN_BASE(fn->kind) == DAS_FN_LOCATION;  // the linearised functional sum w_eff a_f; no state is read
                const FaceFnView fv = fn->view(isLoc ? fn->d_weff.p : fn->d_w0.p);
                launch_grad_and_faces(st, rho, dmD, prm, (const D*)d_Wd.p, s->wk1, !isLoc, [&](auto R) {
                    hipLaunchKernelGGL((k_fn_dual<decltype(R)::value, decltype(R)::solid>), dim3(nblk(nf, B)), dim3(B), 0, st, dmD, prm, (const D*)d_Wd.p, (const D*)s->wk1.nut.p, (const D*)s->wk1.gU.p, fv,
                                       (int)fn->isMoment, fn->vecA[0], fn->vecA[1], fn->vecA[2], fn->vecB[0], fn->vecB[1], fn->vecB[2], (int)areaAvg, cN[0], cN[1], cA[0], cA[1], d_fvd.p);
                });
                hipLaunchKernelGGL(k_vc_fn_cells_dual, dim3(nblk(m.nC, B)), dim3(B), 0, st, m.nC, (const int*)d_fnPtr.p, (const int*)d_fnIdx.p, seeds[0],
                                   (const double*)d_fvd.p, d_tc.p);
            }
            hipLaunchKernelGGL(k_points_seed, dim3(nblk(np, B)), dim3(B), 0, st, np, pts, axis, 0.0, d_XD.p);
            hipLaunchKernelGGL(k_vc_gather, dim3(nblk(np, 4)), dim3(256), 0, st, np, pts, (const long long*)v.d_ptr.p, (const int*)v.d_cells.p,
                               (const double*)d_tc.p, (const double*)nullptr, axis, d_out.p);
            passes++;
        }
        DAS_HIP(hipGetLastError());
    }
    finish_volcoord(s, d_out.p, product, "non-positive cell volume in the volCoord product", t0, passes, info4);
}

// calcJacTVecProduct(volCoord -> residual | function), reference DASolver.C:1690-1839 + DAInputVolCoord: the full product vector
// (3 nPoints) at the current states and points.  info4 (optional) = {colours, residual passes, seconds of the passes, seconds of
// the one-off influence / colouring build}
int das_calc_dvolcoord_product(das_solver_t* s, const char* outputName, const char* outputType, const double* seeds, double* product,
                               double* info4) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(outputType && seeds && product, DAS_ERR_ARG, "null argument");
    std::string ot = outputType;
    std::vector<double> rnSeeds;  // a residualNorm function: the residual product with the seeds dF/dR
    residual_norm_redirect(s, outputName, ot, seeds, rnSeeds);
    DAS_CHECK(ot == "residual" || ot == "function" || is_coupling(ot), DAS_ERR_ARG, "outputType not supported on this path: " + ot);
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "the volCoord product runs on an undecomposed mesh (sharded solvers: use calcVolCoordDirectionalProduct)");
    if (is_coupling(ot)) {
        // the functional seeds . output through the dual-point metrics (forces: S_f carries the tangent, so the pRef S_f term is included;
        // thermal coupling: the delta coefficient of either wallDistanceMethod and the wall distance of a wall function do)
        (void)coupling_size(s, ot, outputName);
        DAS_CHECK(s->opt.gets_or("amd.volCoordMode", "dual") == "dual", DAS_ERR_ARG,
                  "the volCoord product of a " + ot + " needs amd.volCoordMode dual (fd is not implemented for it)");
        das_solver::FaceFn& fn = coupling_functional(s, ot, outputName, seeds);
        const double one = 1.0, zero2[2] = {0.0, 0.0};
        ensure_point_influence(s);
        volcoord_product_dual(s, &fn, false, zero2, zero2, &one, product, info4);
        return DAS_OK;
    }
    const Mesh& m = s->mesh;
    const bool isFn = ot == "function";
    if (isFn) {
        if (das_solver::MeshFn* mf = find_mesh_function(s, outputName)) {  // meshQualityKS: the softmax-weighted face tangents on the dual metrics
            DAS_CHECK(s->opt.gets_or("amd.volCoordMode", "dual") == "dual", DAS_ERR_ARG,
                      "the volCoord product of meshQualityKS function " + mf->name + " needs amd.volCoordMode dual (fd is not implemented for it)");
            ensure_point_influence(s);
            volcoord_product_dual(s, nullptr, false, nullptr, nullptr, seeds, product, info4, nullptr, mf);
            return DAS_OK;
        }
        if (das_solver::CellFn* cf = find_cell_function(s, outputName)) {
            DAS_CHECK(!cf->variance, DAS_ERR_ARG, std::string("volCoord input is not supported for the variance function ") + outputName);
            ensure_point_influence(s);
            volcoord_product_dual(s, nullptr, false, nullptr, nullptr, seeds, product, info4, cf);
            return DAS_OK;
        }
    }
    das_solver::FaceFn* fn = nullptr;
    if (isFn) fn = &get_function(s, outputName);
    DAS_CHECK(!fn || DAS_FN_BASE(fn->kind) != DAS_FN_VARIANCE, DAS_ERR_ARG, std::string("volCoord input is not supported for the variance function ") + outputName);
    // area-averaged functions: coefficients of the linearised functional (k_fn_area_avg) from the group sums at the base mesh
    double cN[2] = {0.0, 0.0}, cA[2] = {0.0, 0.0};
    const int base = isFn ? DAS_FN_BASE(fn->kind) : -1;
    const bool isLoc = base == DAS_FN_LOCATION;
    // functions whose weights carry |Sf| (the area averages; wallHeatFlux also as the plain sum scale |Sf| q)
    const bool areaAvg = isFn && (fn->kind == DAS_FN_TOTALPRESSURE || fn->kind == DAS_FN_TOTALTEMPERATURE || base == DAS_FN_PATCHMEAN
                                  || base == DAS_FN_TOTALPRESSURERATIO || base == DAS_FN_WALLHEATFLUX);
    if (isLoc) function_effective_weights(s, *fn);  // location: the linearised functional sum w_eff a_f (softmax weights at the base mesh)
    if (areaAvg) {
        double S[2], A[2] = {0.0, 0.0};
        function_sums(s, *fn, S);  // S_g = sum of w0 q: totalPressure scale N0 / A0 (one group), ratio functions N_g / A_g
        for (size_t q = 0; q < fn->faces.size(); q++) A[fn->group[q]] += m.fg[fn->faces[q]].magSf;
        if (!fn->ratio) {
            const double outer = ref_var_outer(fn->refVar, fn->ref, S[0] + S[1]);
            if (base == DAS_FN_WALLHEATFLUX && !fn->byUnitArea) {  // F = scale sum |Sf| q
                cN[0] = outer * fn->scale;
            } else {
                cN[0] = outer * fn->scale / A[0];
                cA[0] = -outer * S[0] / A[0];
            }
        } else {
            const double F0 = S[1] / S[0];  // F0 = (N1 / A1) / (N0 / A0)
            const double F = ref_var_outer(fn->refVar, fn->ref, F0) * F0;
            cN[1] = F / (S[1] * A[1]); cA[1] = -F / A[1];
            cN[0] = -F / (S[0] * A[0]); cA[0] = F / A[0];
        }
    }
    ensure_point_influence(s);
    {
        const std::string mode = s->opt.gets_or("amd.volCoordMode", "dual");
        DAS_CHECK(mode == "dual" || mode == "fd", DAS_ERR_ARG, "amd.volCoordMode: dual | fd");
        if (mode == "dual") {
            volcoord_product_dual(s, fn, areaAvg, cN, cA, seeds, product, info4);
            return DAS_OK;
        }
    }
    das_solver::VolCoord& v = s->vc;
    const PointInfluence& I = v.inf;
    const GeomTopo t = device_geom_topo(s);
    hipStream_t st = s->stream;
    const int B = 256;
    const long long n = s->n;
    const size_t n3 = 3 * (size_t)m.nP;
    v.d_X0.upload(m.points.data(), n3);
    v.d_X.upload(m.points.data(), n3);
    v.d_out.alloc(n3);
    v.d_tc.alloc(m.nC);
    DAS_HIP(hipMemsetAsync(v.d_out.p, 0, n3 * sizeof(double), st));
    DAS_HIP(hipMemsetAsync(v.d_bad.p, 0, sizeof(int), st));
    v.d_fg0.alloc(m.nF); v.d_cg0.alloc(m.nC);
    DAS_HIP(hipMemcpyAsync(v.d_fg0.p, s->d_fg.p, m.nF * sizeof(FaceGeom), hipMemcpyDeviceToDevice, st));
    DAS_HIP(hipMemcpyAsync(v.d_cg0.p, s->d_cg.p, m.nC * sizeof(CellGeom), hipMemcpyDeviceToDevice, st));
    // whatever happens below, the solver's metrics are the unperturbed ones afterwards
    struct Restore {
        das_solver* s;
        ~Restore() {
            das_solver::VolCoord& v = s->vc;
            (void)hipStreamSynchronize(s->stream);
            (void)hipMemcpy(s->d_fg.p, v.d_fg0.p, s->mesh.nF * sizeof(FaceGeom), hipMemcpyDeviceToDevice);
            (void)hipMemcpy(s->d_cg.p, v.d_cg0.p, s->mesh.nC * sizeof(CellGeom), hipMemcpyDeviceToDevice);
            v.d_fg0.release(); v.d_cg0.release(); v.d_Rp.release(); v.d_Rm.release(); v.d_seeds.release();
            v.d_X.release(); v.d_X0.release(); v.d_tc.release(); v.d_fvp.release(); v.d_fvm.release();
            if (fn) fn->uploaded = false;  // moment arms were recomputed from perturbed face centres: re-upload the host copy
            try { refresh_heat_sources(s, false); } catch (...) {}  // the source field of the unperturbed metrics
            try { refresh_actuator_disks(s, false); } catch (...) {}
        }
        das_solver::FaceFn* fn;
    } restore{s, (fn && fn->isMoment) ? fn : nullptr};
    const bool rho = DAS_IS_COMPRESSIBLE(s->cp.solver);
    ResParams prm0 = make_params(s->cp, s->opt, 0);
    RowLayout L{};
    int nf = 0;
    if (!isFn) {
        L = residual_row_layout(s);
        v.d_Rp.alloc(n); v.d_Rm.alloc(n);
        v.d_seeds.upload(seeds, n);
    } else {
        need_face_function_solver(s);
        nf = (int)fn->faces.size();
        v.d_fvp.alloc(nf); v.d_fvm.alloc(nf);
        std::vector<int> cptr, cidx;
        function_face_slots(m, *fn, cptr, cidx);
        v.d_fnPtr.upload(cptr); v.d_fnIdx.upload(cidx);
    }
    std::vector<HsRank1> hsTerms;
    DevBuf<double> d_vt0, d_tc2;
    double sideSign = 1.0;
    if (!isFn && !s->heatSources.empty()) {
        heat_source_rank1_terms(s, v.d_seeds.p, prm0.normT ? 0 : 1, hsTerms);
        std::vector<double> vt;
        for (auto& e : s->heatSources) vt.push_back(e.second.volumeTotal);
        d_vt0.upload(vt);
        d_tc2.alloc((size_t)m.nC);
    }
    // actuator disks: as in the exact mode - the scales frozen in the moved-mesh fields, the rank-one terms side by side in d_tc2
    std::vector<AdView<double>> adFrozen;
    std::vector<AdRank1> adTerms;
    DevBuf<double> d_adWork;
    if (!isFn && !s->actuatorDisks.empty()) {
        actuator_disk_volcoord_setup(s, seeds, adFrozen, adTerms);
        d_adWork.alloc(5 * adFrozen.size());
        if (!adTerms.empty()) d_tc2.alloc((size_t)m.nC);
    }
    const bool rank1 = !hsTerms.empty() || !adTerms.empty();
    auto output_pass = [&](double* Rout, double* fvOut) {
        if (!isFn) {
            if (!adFrozen.empty()) actuator_disk_field<double, double, double>(s, adFrozen, (const CellGeom*)s->d_cg.p, d_adWork.p, s->d_src3.p, false);
            for (const AdRank1& r : adTerms)
                hipLaunchKernelGGL((k_ad_fd_rank1<double>), dim3(nblk(m.nC, B)), dim3(B), 0, st, r.view, m.nC, (const CellGeom*)s->d_cg.p, sideSign * r.beta, d_tc2.p);
            // the source field of the moved mesh with the totals and a snapped centre frozen, as in the exact mode; their rank-one terms
            // are collected side by side (+ and -) in d_tc2
            for (size_t k = 0; k < hsTerms.size(); k++) {
                hipLaunchKernelGGL((k_hs_apply<double, double, double>), dim3(nblk(m.nC, B)), dim3(B), 0, st, hsTerms[k].view, m.nC, (const CellGeom*)s->d_cg.p,
                                   (const double*)(d_vt0.p + k), (int)(k == 0), s->d_src.p);
                hipLaunchKernelGGL(k_hs_fd_rank1, dim3(nblk(m.nC, B)), dim3(B), 0, st, hsTerms[k].view, m.nC, (const CellGeom*)s->d_cg.p, hsTerms[k].snapCell,
                                   sideSign * hsTerms[k].beta, sideSign * hsTerms[k].gamma[0], sideSign * hsTerms[k].gamma[1], sideSign * hsTerms[k].gamma[2], d_tc2.p);
            }
            eval_residual<double>(s->dm, s->cp, prm0, s->d_W.p, Rout, s->wk, s->d_phiF.p, s->d_Told.p, st);
            return;
        }
        if (isLoc) {
            hipLaunchKernelGGL((k_fn_value<false>), dim3(nblk(nf, B)), dim3(B), 0, st, s->dm, prm0, s->d_W.p, (const double*)nullptr, (const double*)nullptr,
                               fn->view(fn->d_weff.p), fvOut);
            return;
        }
        const ResParams prm = s->wk.bind(s->cp.solver, s->dm.nC, s->dm.nF, prm0);
        if (fn->isMoment)
            hipLaunchKernelGGL(k_fn_moment_dir, dim3(nblk(nf, B)), dim3(B), 0, st, nf, (const int*)fn->d_faces.p, (const FaceGeom*)s->d_fg.p, fn->vecA[0], fn->vecA[1],
                               fn->vecA[2], fn->vecB[0], fn->vecB[1], fn->vecB[2], fn->d_dir.p);
        launch_grad_and_faces(st, rho, s->dm, prm, (const double*)s->d_W.p, s->wk, true, [&](auto R) {
            if (areaAvg) hipLaunchKernelGGL((k_fn_area_avg<decltype(R)::value, decltype(R)::solid>), dim3(nblk(nf, B)), dim3(B), 0, st, s->dm, prm, s->d_W.p, s->wk.nut.p, s->wk.gU.p, fn->view(fn->d_w0.p), cN[0], cN[1], cA[0], cA[1], fvOut);
            else hipLaunchKernelGGL((k_fn_value<decltype(R)::value, decltype(R)::solid>), dim3(nblk(nf, B)), dim3(B), 0, st, s->dm, prm, s->d_W.p, s->wk.nut.p, s->wk.gU.p, fn->view(fn->d_w0.p), fvOut);
        });
    };
    const double t0 = wall_seconds();
    long long passes = 0;
    for (int col = 0; col < I.nColors; col++) {
        const int np = I.cptr[col + 1] - I.cptr[col];
        if (np == 0) continue;
        const int* pts = v.d_cpoints.p + I.cptr[col];
        for (int axis = 0; axis < 3; axis++) {
            if (rank1) DAS_HIP(hipMemsetAsync(d_tc2.p, 0, (size_t)m.nC * sizeof(double), st));
            for (int side = 0; side < 2; side++) {
                sideSign = side == 0 ? 1.0 : -1.0;
                hipLaunchKernelGGL(k_move_points, dim3(nblk(np, B)), dim3(B), 0, st, np, pts, (const double*)v.d_h.p, side == 0 ? 1.0 : -1.0, axis,
                                   (const double*)v.d_X0.p, v.d_X.p);
                device_geometry(s, t, v.d_X.p);
                output_pass(side == 0 ? v.d_Rp.p : v.d_Rm.p, side == 0 ? v.d_fvp.p : v.d_fvm.p);
                passes++;
            }
            hipLaunchKernelGGL(k_move_points, dim3(nblk(np, B)), dim3(B), 0, st, np, pts, (const double*)v.d_h.p, 0.0, axis, (const double*)v.d_X0.p, v.d_X.p);
            if (!isFn) {
                hipLaunchKernelGGL(k_vc_rows, dim3(nblk(m.nC, B)), dim3(B), 0, st, s->dm, L, (const double*)v.d_seeds.p, (const double*)v.d_Rp.p,
                                   (const double*)v.d_Rm.p, v.d_tc.p);
                if (rank1) hipLaunchKernelGGL(k_hs_add, dim3(nblk(m.nC, B)), dim3(B), 0, st, m.nC, (const double*)d_tc2.p, v.d_tc.p);
            } else
                hipLaunchKernelGGL(k_vc_fn_cells, dim3(nblk(m.nC, B)), dim3(B), 0, st, m.nC, (const int*)v.d_fnPtr.p, (const int*)v.d_fnIdx.p, seeds[0],
                                   (const double*)v.d_fvp.p, (const double*)v.d_fvm.p, v.d_tc.p);
            hipLaunchKernelGGL(k_vc_gather, dim3(nblk(np, 4)), dim3(256), 0, st, np, pts, (const long long*)v.d_ptr.p, (const int*)v.d_cells.p,
                               (const double*)v.d_tc.p, (const double*)v.d_h.p, axis, v.d_out.p);
        }
        DAS_HIP(hipGetLastError());
    }
    finish_volcoord(s, v.d_out.p, product, "a perturbed mesh of the volCoord product has a non-positive cell volume (amd.volCoordRelStep too large?)", t0,
                    passes, info4);
    return DAS_OK;
    DAS_CATCH
}

int das_get_input_size(das_solver_t* s, const char* inputName, const char* inputType) {
    DAS_TRY
    DAS_CHECK(s && inputType, DAS_ERR_ARG, "null argument");
    DAS_CHECK(std::string(inputType) == "stateVar", DAS_ERR_ARG, std::string("inputType not supported on this path: ") + inputType);
    return (int)s->n;
    DAS_CATCH
}
int das_get_output_size(das_solver_t* s, const char* outputName, const char* outputType) {
    DAS_TRY
    DAS_CHECK(s && outputType, DAS_ERR_ARG, "null argument");
    if (std::string(outputType) == "function") return 1;
    if (is_coupling(outputType)) return coupling_size(s, outputType, outputName);
    DAS_CHECK(std::string(outputType) == "residual", DAS_ERR_ARG, std::string("outputType not supported on this path: ") + outputType);
    return (int)s->n;
    DAS_CATCH
}
int das_calc_jac_t_vec_product(das_solver_t* s, const char* inputName, const char* inputType, const double* inputs, const char* outputName,
                               const char* outputType, const double* seeds, double* product) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(inputType && outputType && inputs && seeds && product, DAS_ERR_ARG, "null argument");
    DAS_CHECK(std::string(inputType) == "stateVar", DAS_ERR_ARG, "calcJacTVecProduct: only stateVar inputs are implemented on the GPU path");
    // a residualNorm function: dR/dW^T g with the seeds g = seed dF/dR formed on the device at the assigned states (k_rn_seeds)
    das_solver::MeshFn* rn = std::string(outputType) == "function" ? find_mesh_function(s, outputName) : nullptr;
    if (rn && !rn->residualNorm) rn = nullptr;
    if (!rn && std::string(outputType) == "function") {
        // dFdW^T * seed, state-scaled (reference DASolver.C:1690-1839 with DAOutputFunction, normalizeJacTVecProduct :1443-1553)
        s->h_W.assign(inputs, inputs + s->n);
        s->d_W.upload(s->h_W);
        function_gradient(s, outputName, seeds[0], product);
        return DAS_OK;
    }
    if (is_coupling(outputType)) {
        // d(seeds . output)/dW, state-scaled like the function branch: the coloured passes on the functional seeds . output
        const std::string ot = outputType;
        (void)coupling_size(s, ot, outputName);
        s->h_W.assign(inputs, inputs + s->n);
        s->d_W.upload(s->h_W);
        face_function_gradient(s, coupling_functional(s, ot, outputName, seeds), 1.0, product);
        return DAS_OK;
    }
    DAS_CHECK(rn || std::string(outputType) == "residual", DAS_ERR_ARG,
              "calcJacTVecProduct: only (stateVar -> residual | function | forceCouplingOutput | thermalCouplingOutput) is implemented on the GPU path");
    // DAInputStateVar::run assigns the inputs to the states (reference DASolver.C:1690-1839)
    // the operator initializedRdWTMatrixFree built is reused when it was assembled at these very states (the reference
    // replays its tape; re-assembling all colours for one product would cost ~nColors residual passes)
    const bool reuse = s->op && s->op_geom == s->geomVersion && s->op_epoch == s->opEpoch && s->op_states.size() == (size_t)s->n && (int)s->opt.geti("amd.jacMode") == 1
                       && std::memcmp(s->op_states.data(), inputs, s->n * sizeof(double)) == 0;
    s->h_W.assign(inputs, inputs + s->n);
    s->d_W.upload(s->h_W);
    std::unique_ptr<das_mat> A;
    if (!reuse) A.reset(assemble(s, 0, 1));
    if (rn) {
        residual_norm_seeds(s, *rn, seeds[0], s->d_tmp1.p);
    } else {
        DAS_HIP(hipMemcpyAsync(s->d_tmp1.p, seeds, s->n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    spmv(s, reuse ? s->op->m : A->m, s->d_tmp1.p, s->d_tmp2.p);
    DAS_HIP(hipMemcpyAsync(product, s->d_tmp2.p, s->n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    DAS_HIP(hipStreamSynchronize(s->stream));
    return DAS_OK;
    DAS_CATCH
}
// product_i = sum_j dR_i/dW_j s_j v_j : ONE forward-mode residual pass, no colouring, no matrix (the untransposed
// companion of dRdW^T psi; exact, so  a.(J v) == (J^T a).v  holds to round-off and checks colouring + scatter maps)
int das_calc_jac_vec_product(das_solver_t* s, const double* v, double* product) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(v && product, DAS_ERR_ARG, "null argument");
    const long long n = s->n;
    const int B = 256;
    hipStream_t st = s->stream;
    ResParams prm = make_params(s->cp, s->opt, 0);
    if (s->d_Wd.n != (size_t)n) { s->d_Wd.alloc(n); s->d_Rd.alloc(n); }
    DAS_HIP(hipMemcpyAsync(s->d_tmp1.p, v, n * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_seed_dir, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_W.p, s->d_scale.p, s->d_tmp1.p, s->d_Wd.p);
    eval_residual<Dual<1>>(s->dm, s->cp, prm, s->d_Wd.p, s->d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
    hipLaunchKernelGGL(k_tangent_out, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_Rd.p, s->d_tmp2.p);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipMemcpyAsync(product, s->d_tmp2.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
    DAS_HIP(hipStreamSynchronize(st));
    return DAS_OK;
    DAS_CATCH
}
int das_drdwt_mult_device(das_solver_t* s, const double* d_x, double* d_y) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(s->op, DAS_ERR_STATE, "initializedRdWTMatrixFree() has not been called");
    spmv(s, s->op->m, d_x, d_y);
    return DAS_OK;
    DAS_CATCH
}

int das_create_ml_rksp_matrix_free(das_solver_t* s, das_mat_t* pc, das_ksp_t** ksp) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(pc && ksp, DAS_ERR_ARG, "null argument");
    std::unique_ptr<das_ksp> k(new das_ksp);
    k->pcmat = pc;
    const std::string pcType = s->opt.gets("amd.pcType");
    DAS_CHECK(pcType == "bilu" || pcType == "ras", DAS_ERR_ARG, "amd.pcType must be \"bilu\" or \"ras\"");
    if (pcType == "bilu") {
        if (getenv("DAS_BILU_ORDER")) k->pcOrder = atoi(getenv("DAS_BILU_ORDER"));
        const long long K = pc_subdomain_count(s);
        if (!(K > 1 && setup_subdomain_ilus(s, k.get(), (int)K))) setup_node_ilu(s, k.get(), /*byEstimate*/ true);
    } else setup_block_ilu(s, k.get());
    setup_coarse(s, k.get());
    *ksp = k.release();
    return DAS_OK;
    DAS_CATCH
}
int das_solve_linear_eqn(das_solver_t* s, das_ksp_t* ksp, const double* rhs, double* sol) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(ksp && rhs && sol, DAS_ERR_ARG, "null argument");
    const int polyD = poly_degree(s, false);
    if (idr_selected(s, false)) idr_ws(s, ksp);  // (never the Krylov basis)
    else gmres_ws(s, ksp, polyD);
    ksp->bdev.upload(rhs, s->n);
    ksp->xdev.upload(sol, s->n);
    int rc = run_gmres(s, ksp, ksp->bdev.p, ksp->xdev.p, 0);
    ksp->xdev.download(sol, s->n);
    if (s->opt.geti("adjEqnOption.printInfo"))
        fprintf(stderr, "Main iteration %d KSP Residual norm %14.12e %.2f s\n", ksp->iters, ksp->res, ksp->seconds);
    return rc;
    DAS_CATCH
}
// block solve: nrhs right-hand sides (host, column-major n x nrhs) through ONE block GMRES; res0/res (optional) return
// the initial / final residual norm of every system
int das_solve_linear_eqn_block(das_solver_t* s, das_ksp_t* ksp, int nrhs, const double* rhs, double* sol, double* res0, double* res) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(ksp && rhs && sol && nrhs >= 1, DAS_ERR_ARG, "bad argument");
    DAS_CHECK(poly_degree(s, false) == 0, DAS_ERR_ARG, "amd.polyDegree > 0 is not available for a block (multi-right-hand-side) solve");
    DevBuf<double> dB((size_t)nrhs * s->n), dX((size_t)nrhs * s->n);
    dB.upload(rhs, (size_t)nrhs * s->n);
    int rc = run_block_gmres(s, ksp, nrhs, dB.p, dX.p);
    dX.download(sol, (size_t)nrhs * s->n);
    for (int r = 0; r < nrhs; r++) { if (res0) res0[r] = ksp->block_res0[r]; if (res) res[r] = ksp->block_res[r]; }
    if (s->opt.geti("adjEqnOption.printInfo"))
        fprintf(stderr, "Block solve (%d systems): iteration %d max KSP Residual norm %14.12e %.2f s\n", nrhs, ksp->iters, ksp->res, ksp->seconds);
    return rc;
    DAS_CATCH
}
int das_ksp_apply_pc(das_solver_t* s, das_ksp_t* ksp, const double* x, double* y) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(ksp && x && y, DAS_ERR_ARG, "null argument");
    DevBuf<double> dx(s->n), dy(s->n);
    dx.upload(x, s->n);
    DAS_HIP(hipDeviceSynchronize());
    dy.zero();
    pc_apply_full(s, ksp, dx.p, dy.p);
    gmres_finish_check(s, ksp);
    dy.download(y, s->n);
    return DAS_OK;
    DAS_CATCH
}
// node structure of the "bilu" preconditioner (host only, no GPU needed): sizes, then the arrays in processing order
static void copy_pc_structure(const NodeILU& P, int* nodeUnk, long long* bptr, int* bcol, int* lvlPtr, int* natural) {
    if (natural) std::copy(P.h_natural.begin(), P.h_natural.end(), natural);
    if (nodeUnk) std::copy(P.h_nodeUnk.begin(), P.h_nodeUnk.end(), nodeUnk);
    if (bptr) std::copy(P.h_bptr.begin(), P.h_bptr.end(), bptr);
    if (bcol) std::copy(P.h_bcol.begin(), P.h_bcol.end(), bcol);
    if (lvlPtr) std::copy(P.h_lvlPtr.begin(), P.h_lvlPtr.end(), lvlPtr);
}
int das_pc_structure_build(das_solver_t* s, int* nNodes, long long* nBlocks, int* nLevels, int* reach) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    const int rch = pc_stencil_reach(s);
    const std::vector<char> cellOwned = cells_of_mask(s->mesh, s->st_full.states, s->owned);
    std::vector<int> unkNode, bcol;
    std::vector<unsigned char> unkSlot;
    std::vector<long long> bptr, bdiag;
    bilu_build_structure(s->mesh, s->st_full.states, s->n, s->owned, cellOwned, rch, s->pcStruct, unkNode, unkSlot, bptr, bdiag, bcol, pc_setup_threads(s), pc_ordering_rcm(s));
    if (nNodes) *nNodes = s->pcStruct.nNodes;
    if (nBlocks) *nBlocks = s->pcStruct.nnzB;
    if (nLevels) *nLevels = s->pcStruct.nLevels;
    if (reach) *reach = rch;
    return DAS_OK;
    DAS_CATCH
}
int das_pc_structure_get(das_solver_t* s, int* nodeUnk, long long* bptr, int* bcol, int* lvlPtr, int* natural) {
    DAS_TRY
    DAS_CHECK(s && s->pcStruct.nNodes > 0, DAS_ERR_STATE, "das_pc_structure_build has not been called");
    copy_pc_structure(s->pcStruct, nodeUnk, bptr, bcol, lvlPtr, natural);
    return DAS_OK;
    DAS_CATCH
}
int das_ksp_get_pc_structure_sizes(das_ksp_t* ksp, int* nNodes, long long* nBlocks, int* nLevels) {
    DAS_TRY
    DAS_CHECK(ksp && ksp->useBilu, DAS_ERR_STATE, "the KSP does not hold a node-block ILU preconditioner (amd.pcType \"bilu\")");
    if (nNodes) *nNodes = ksp->bilu.nNodes;
    if (nBlocks) *nBlocks = ksp->bilu.nnzB;
    if (nLevels) *nLevels = ksp->bilu.nLevels;
    return DAS_OK;
    DAS_CATCH
}
int das_ksp_get_pc_structure(das_ksp_t* ksp, int* nodeUnk, long long* bptr, int* bcol, int* lvlPtr, int* natural) {
    DAS_TRY
    DAS_CHECK(ksp && ksp->useBilu, DAS_ERR_STATE, "the KSP does not hold a node-block ILU preconditioner (amd.pcType \"bilu\")");
    copy_pc_structure(ksp->bilu, nodeUnk, bptr, bcol, lvlPtr, natural);
    return DAS_OK;
    DAS_CATCH
}
// nodeOut[nNodes * 8]: the unknown a slot WRITES (= nodeUnk, or -1 for the overlap copies of a multi-block factorisation, amd.pcSubdomains)
int das_ksp_get_pc_node_out(das_ksp_t* ksp, int* nodeOut) {
    DAS_TRY
    DAS_CHECK(ksp && ksp->useBilu && nodeOut, DAS_ERR_STATE, "the KSP does not hold a node-block ILU preconditioner (amd.pcType \"bilu\")");
    const std::vector<int>& src = ksp->bilu.h_nodeOut.empty() ? ksp->bilu.h_nodeUnk : ksp->bilu.h_nodeOut;
    std::copy(src.begin(), src.end(), nodeOut);
    return DAS_OK;
    DAS_CATCH
}
int das_ksp_get_n_blocks(das_ksp_t* ksp) { return ksp ? ksp->pc.nBlocks : -1; }
long long das_ksp_get_factor_nnz(das_ksp_t* ksp) { return ksp ? ksp->pc.fnnz : -1; }
long long das_ksp_get_n_ext(das_ksp_t* ksp) { return ksp ? ksp->pc.next : -1; }
int das_ksp_get_blocks(das_ksp_t* ksp, int* perm, long long* block_off) {
    DAS_TRY
    DAS_CHECK(ksp && perm && block_off, DAS_ERR_ARG, "null argument");
    DAS_CHECK(!ksp->useBilu, DAS_ERR_STATE, "das_ksp_get_blocks describes the \"ras\" preconditioner; use das_ksp_get_pc_structure");
    std::copy(ksp->pc.h_core_perm.begin(), ksp->pc.h_core_perm.end(), perm);
    std::copy(ksp->pc.h_core_off.begin(), ksp->pc.h_core_off.end(), block_off);
    return DAS_OK;
    DAS_CATCH
}
int das_ksp_get_info(das_ksp_t* k, int* iters, double* res0, double* res, double* seconds) {
    DAS_TRY
    DAS_CHECK(k, DAS_ERR_ARG, "null ksp");
    if (iters) *iters = k->iters;
    if (res0) *res0 = k->res0;
    if (res) *res = k->res;
    if (seconds) *seconds = k->seconds;
    return DAS_OK;
    DAS_CATCH
}
// dense nonsymmetric eigen-solver used by the deflated restart (amd.gmresDeflation): fn(m, A row-major, wr, wi, vr, vi) with the
// eigenvector of eigenvalue e in vr / vi [e * m .. e * m + m) (real / imaginary parts); returns 0 on success.  Process-wide.
int das_set_dense_eig_callback(void* fn) { g_dense_eig = (das_dense_eig_fn)fn; return DAS_OK; }
// host algebra of one deflated restart (CPU tier: checked against the numpy restatement): Hbar (m+1) x m row-major, rvec (m+1);
// outputs sized for k + 1: P1 (m+1) x (kk+1), Hnew (kk+1) x kk, cnew (kk+1) - all row-major; returns kk (< 0 on failure)
int das_debug_gmres_dr_restart(int m, int kwant, const double* Hbar, const double* rvec, double* P1, double* Hnew, double* cnew) {
    DAS_TRY
    DAS_CHECK(m >= 2 && kwant >= 1 && Hbar && rvec && P1 && Hnew && cnew, DAS_ERR_ARG, "bad argument");
    std::vector<double> Hb(Hbar, Hbar + (size_t)(m + 1) * m), rv(rvec, rvec + m + 1), p, h, c;
    int kk = 0;
    if (gmres_dr_restart_host(g_dense_eig, m, kwant, Hb, rv, kk, p, h, c) != 0) return -1;
    std::copy(p.begin(), p.end(), P1); std::copy(h.begin(), h.end(), Hnew); std::copy(c.begin(), c.end(), cnew);
    return kk;
    DAS_CATCH
}
// Cholesky step of CholQR on the host (CPU tier): G sv x sv row-major -> L (lower triangular), T = L^-T
int das_debug_block_chol(int sv, const double* G, double* L, double* T) {
    DAS_TRY
    DAS_CHECK(sv >= 1 && G && L && T, DAS_ERR_ARG, "bad argument");
    chol_upper_inverse(sv, G, L, T);
    return DAS_OK;
    DAS_CATCH
}
// the block-Hessenberg least squares fed as run_block_gmres feeds it (CPU tier; layout: include/dafoam_amd.h)
int das_debug_block_lsq(int sv, int m, int ncols, const double* S0, const double* Hc, const double* Hc2, const double* S, double* Y, double* res) {
    DAS_TRY
    DAS_CHECK(sv >= 1 && m >= 1 && ncols >= 1 && ncols <= m && S0 && Hc && Hc2 && S && Y && res, DAS_ERR_ARG, "bad argument");
    BlockLsq lsq;
    lsq.reset(m, sv, S0);
    const size_t blk = (size_t)m * sv * sv;
    for (int j = 0; j < ncols; j++) lsq.add_column(j, Hc + j * blk, Hc2 + j * blk, S + (size_t)j * sv * sv);
    lsq.residuals(ncols - 1, res);
    lsq.solve(ncols, Y);
    return DAS_OK;
    DAS_CATCH
}
// the deflated-restart iteration (gmres_dr_loop, the loop the device solver runs) on host vectors with callback operator / preconditioner:
// CPU tier.  info4 = {iterations, deflated restarts, plain restarts, breakdowns}; returns the reference's fail flag
int das_debug_gmres_dr_host(long long n, void* A, void* M, void* user, const double* b, double* x, int m, int kdef, double rtol, double atol,
                            long long maxIts, double* hist, int histCap, double* info4, double* res2) {
    DAS_TRY
    DAS_CHECK(n > 0 && A && M && b && x && m >= 4, DAS_ERR_ARG, "bad argument");
    DrHostOps ops{n, (das_host_apply_fn)A, (das_host_apply_fn)M, user, b, x, std::vector<double>((size_t)(m + 2) * n, 0.0), std::vector<double>(n), std::vector<double>(n), std::vector<double>(n), m};
    std::fill(x, x + n, 0.0);
    const double beta0 = ops.true_residual();
    std::vector<double> h{beta0};
    const double target = std::max(rtol * beta0, atol);
    const DrResult R = gmres_dr_loop(ops, g_dense_eig, m, kdef, beta0, target, maxIts, h);
    if (hist) for (int i = 0; i < histCap && i < (int)h.size(); i++) hist[i] = h[i];
    if (info4) { info4[0] = (double)R.its; info4[1] = R.nDeflated; info4[2] = R.nRestarts; info4[3] = R.nBreakdown; }
    if (res2) { res2[0] = R.res0; res2[1] = R.res; }
    return gmres_failed(R.res, beta0, rtol, atol, 1e2);
    DAS_CATCH
}
// IDR(s) of the last solve of this KSP (amd.krylovMethod "idrs"): s as used (clamped to n), completed cycles, restarts from the true
// residual, breakdowns; the work vectors the path holds (3 s + 5: P, G, U, r, z, t, right-hand side, solution) and their bytes (8 n each).
// cycles = 0 and workVectors = 0: this KSP has not run IDR(s)
int das_ksp_get_idr_info(das_ksp_t* k, int* sv, int* cycles, int* restarts, int* breakdowns, int* workVectors, double* workBytes) {
    DAS_TRY
    DAS_CHECK(k, DAS_ERR_ARG, "null ksp handle");
    const IdrWork* I = k->idr.get();
    if (sv) *sv = I ? I->s : 0;
    if (cycles) *cycles = I ? I->cycles : 0;
    if (restarts) *restarts = I ? I->restarts : 0;
    if (breakdowns) *breakdowns = I ? I->breakdowns : 0;
    if (workVectors) *workVectors = I ? I->work_vectors() : 0;
    if (workBytes) *workBytes = I ? (double)I->work_vectors() * 8.0 * (double)I->n : 0.0;
    return DAS_OK;
    DAS_CATCH
}
static IdrHostOps idr_host_ops(long long n, void* A, void* M, void* user, const double* b, double* x) {
    return IdrHostOps{n, (das_host_apply_fn)A, (das_host_apply_fn)M, user, b, x, 0, {}, {}, {}, std::vector<double>(n), std::vector<double>(n), std::vector<double>(n), {}};
}
// the IDR(s) iteration (idrs_loop, the loop the device solver runs) on host vectors with callback operator / preconditioner, from x = 0:
// CPU tier.  info4 = {products, stop reason (0 tolerance, 1 budget, 2 stagnation, 3 non-finite residual), restarts, breakdowns}, res2 = {|r0|, |r|}
// (true residuals); returns the fail flag
int das_debug_idrs_host(long long n, void* A, void* M, void* user, const double* b, double* x, int sv, int seed, double rtol, double atol, long long maxIts,
                        double* hist, int histCap, double* info4, double* res2) {
    DAS_TRY
    DAS_CHECK(n > 0 && A && M && b && x && sv >= 1 && sv <= IDR_MAX_S, DAS_ERR_ARG, "bad argument (1 to 8 shadow vectors)");
    IdrHostOps ops = idr_host_ops(n, A, M, user, b, x);
    std::fill(x, x + n, 0.0);
    const double beta0 = ops.true_residual();
    std::vector<double> h{beta0};
    const IdrResult R = idrs_loop(ops, (int)std::min<long long>(sv, n), (unsigned)seed, beta0, std::max(rtol * beta0, atol), maxIts, h);
    if (hist) for (int i = 0; i < histCap && i < (int)h.size(); i++) hist[i] = h[i];
    if (info4) { info4[0] = (double)R.its; info4[1] = R.reason; info4[2] = R.nRestarts; info4[3] = R.nBreakdown; }
    if (res2) { res2[0] = R.res0; res2[1] = R.res; }
    return R.reason == 3 ? 1 : gmres_failed(R.res, beta0, rtol, atol, 1e2);
    DAS_CATCH
}
// exactly one cycle (s + 1 products) of the same loop from x = 0, and the state it leaves: x, the recurrence residual r, the orthonormal
// shadow space P and the spaces G, U (n x s each, column-major) - what the CPU tier compares with the published sequential form
int das_debug_idr_cycle_host(long long n, void* A, void* M, void* user, const double* b, double* x, int sv, int seed, double* r, double* P, double* G, double* U) {
    DAS_TRY
    DAS_CHECK(n > 0 && A && M && b && x && r && P && G && U && sv >= 1 && sv <= IDR_MAX_S && sv <= n, DAS_ERR_ARG, "bad argument (1 to min(8, n) shadow vectors)");
    IdrHostOps ops = idr_host_ops(n, A, M, user, b, x);
    std::fill(x, x + n, 0.0);
    const double beta0 = ops.true_residual();
    std::vector<double> h{beta0};
    const IdrResult R = idrs_loop(ops, sv, (unsigned)seed, beta0, 0.0, (long long)sv + 2, h);  // budget: one cycle and the closing true residual
    DAS_CHECK(R.its == sv + 2 && R.cycles == 1, DAS_ERR_INTERNAL, "the cycle did not complete (breakdown)");
    std::copy(ops.rrec.begin(), ops.rrec.end(), r);
    std::copy(ops.P.begin(), ops.P.end(), P); std::copy(ops.G.begin(), ops.G.end(), G); std::copy(ops.U.begin(), ops.U.end(), U);
    return DAS_OK;
    DAS_CATCH
}
// test-only entries of the IDR(s) kernels (bodies: das_idr_debug.hpp; layouts: include/dafoam_amd.h)
int das_debug_idr_shadow(long long n, int sv, long long ld, int seed, int device, double* P) {
    DAS_TRY
    DAS_CHECK(P, DAS_ERR_ARG, "null argument");
    idr_check_shape("das_debug_idr_shadow", n, sv, ld);
    debug_idr_shadow(n, sv, ld, (unsigned)seed, device != 0, P);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_idr_combine(long long n, int m, double a, const double* x, double* V, long long ld, long long vlen, const double* c, long long yoff, double* y,
                          long long ylen) {
    DAS_TRY
    DAS_CHECK(x && V && c && (yoff >= 0 || y), DAS_ERR_ARG, "null argument");
    DAS_CHECK(n > 0 && m >= 0 && m <= IDR_MAX_S && ld >= n && vlen >= (long long)std::max(m - 1, 0) * ld + n, DAS_ERR_ARG, "das_debug_idr_combine: bad shape");
    DAS_CHECK(yoff >= 0 ? yoff + n <= vlen : ylen >= n, DAS_ERR_ARG, "das_debug_idr_combine: the output does not fit");
    debug_idr_combine(n, m, a, x, V, ld, vlen, c, yoff, y, ylen);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_idr_biortho_step(long long n, int kk, double* G, double* U, long long ld, long long glen, const double* coef, double* r, double* x, long long vlen,
                               double* rr) {
    DAS_TRY
    DAS_CHECK(G && U && coef && r && x && rr, DAS_ERR_ARG, "null argument");
    DAS_CHECK(n > 0 && kk >= 0 && kk < IDR_MAX_S && ld >= n && glen >= (long long)kk * ld + n && vlen >= n, DAS_ERR_ARG, "das_debug_idr_biortho_step: bad shape");
    debug_idr_biortho_step(n, kk, G, U, ld, glen, coef, r, x, vlen, rr);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_idr_smooth_step(long long n, int sv, double omega, double* r, const double* t, double* x, const double* z, long long vlen, double* P, long long ld,
                              long long plen, double* out) {
    DAS_TRY
    DAS_CHECK(r && t && x && z && P && out, DAS_ERR_ARG, "null argument");
    idr_check_shape("das_debug_idr_smooth_step", n, sv, ld);
    DAS_CHECK(vlen >= n && plen >= (long long)(sv - 1) * ld + n, DAS_ERR_ARG, "das_debug_idr_smooth_step: bad shape");
    debug_idr_smooth_step(n, sv, omega, r, t, x, z, vlen, P, ld, plen, out);
    return DAS_OK;
    DAS_CATCH
}
// ---- amd.polyDegree: the figures of the last solve, and the test-only entries (bodies: das_poly_host.hpp, das_poly_debug.hpp) --------
int das_ksp_get_poly_info(das_ksp_t* k, int* degree, int* nComplexPairs, long long* products, long long* columns, long long* generatingColumns, int* generated,
                          int* fallback, int* workVectors, double* workBytes, int* nRoots, double* re, double* im) {
    DAS_TRY
    DAS_CHECK(k, DAS_ERR_ARG, "null ksp handle");
    const PolyWork* P = k->poly.get();
    if (degree) *degree = P ? P->degree : 0;
    if (nComplexPairs) *nComplexPairs = P ? P->nPairs : 0;
    if (products) *products = P ? P->products : 0;
    if (columns) *columns = P ? P->columns : 0;
    if (generatingColumns) *generatingColumns = P ? P->genColumns : 0;
    if (generated) *generated = P ? P->generated : 0;
    if (fallback) *fallback = P ? P->fallback : 0;
    if (workVectors) *workVectors = P ? P->work_vectors() : 0;
    if (workBytes) *workBytes = P ? (double)P->work_vectors() * 8.0 * (double)P->n : 0.0;
    if (nRoots) *nRoots = P ? P->nroots : 0;
    for (int i = 0; P && i < P->nroots; i++) { if (re) re[i] = P->re[i]; if (im) im[i] = P->im[i]; }
    return DAS_OK;
    DAS_CATCH
}
// the ordered roots of a (d + 1) x d Hessenberg matrix (row-major): the number of entries written (real roots and pairs), 0 = fallback
int das_debug_poly_roots(int d, const double* Hbar, double* re, double* im) {
    DAS_TRY
    DAS_CHECK(d >= 1 && d <= POLY_MAX_DEGREE && Hbar && re && im, DAS_ERR_ARG, "bad argument (degree 1 to 16)");
    return poly_roots_host(g_dense_eig, d, Hbar, d, re, im, nullptr);
    DAS_CATCH
}
// out = p(B) v, B = A M^-1 as callbacks, by the root walk the device solver runs (poly_walk) on host vectors
int das_debug_poly_apply_host(long long n, void* A, void* M, void* user, int nroots, const double* re, const double* im, const double* v, double* out) {
    DAS_TRY
    DAS_CHECK(n > 0 && A && M && re && im && v && out && nroots >= 1 && nroots <= POLY_MAX_DEGREE, DAS_ERR_ARG, "bad argument (1 to 16 roots)");
    DAS_CHECK(poly_degree_of(nroots, im) <= POLY_MAX_DEGREE, DAS_ERR_ARG, "the degree (real roots + 2 x pairs) is above 16");
    for (int i = 0; i < nroots; i++) DAS_CHECK(im[i] >= 0.0 && (re[i] != 0.0 || im[i] != 0.0), DAS_ERR_ARG, "a root is zero, or a pair is not given by its member with im > 0");
    PolyHostOps ops(n, (das_host_apply_fn)A, (das_host_apply_fn)M, user, v);
    poly_walk(ops, nroots, re, im);
    std::copy(ops.poly.begin(), ops.poly.end(), out);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_poly_step(long long n, int kind, int first, int last, double re, double im, long long off, long long len, double* v, double* w, double* prod, double* poly,
                        double* tmp) {
    DAS_TRY
    DAS_CHECK(v && w && prod && poly && tmp, DAS_ERR_ARG, "null argument");
    DAS_CHECK(n > 0 && off >= 0 && len >= off + n && kind >= POLY_STEP_REAL && kind <= POLY_STEP_PAIR_SECOND, DAS_ERR_ARG, "das_debug_poly_step: bad shape or kind");
    debug_poly_step(n, kind, first != 0, last != 0, re, im, off, len, v, w, prod, poly, tmp);
    return DAS_OK;
    DAS_CATCH
}
// out = p(B) v on the device with the roots of this KSP's last solve (operator and preconditioner as that solve had them)
int das_debug_ksp_poly_apply(das_solver_t* s, das_ksp_t* k, const double* v, double* out) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(k && v && out, DAS_ERR_ARG, "null argument");
    DAS_CHECK(s->op, DAS_ERR_STATE, "initializedRdWTMatrixFree() must be called first");
    DAS_CHECK(k->poly && k->poly->nroots > 0 && k->poly->n == s->n && k->w.n == (size_t)s->n && k->z.n == (size_t)s->n, DAS_ERR_STATE, "this KSP's last solve built no polynomial (amd.polyDegree)");
    DevBuf<double> dv(s->n);
    dv.upload(v, s->n);
    DAS_HIP(hipDeviceSynchronize());
    if (k->useBilu) bilu_clear_abort(k->bilu, s->stream);
    poly_apply_device(s, k, dv.p);
    gmres_finish_check(s, k);
    k->poly->poly.download(out, s->n);
    return DAS_OK;
    DAS_CATCH
}
int das_ksp_get_n_refine(das_ksp_t* k) { return k ? k->nrefine : -1; }
int das_ksp_get_status(das_ksp_t* k, int* reason, int* nBreakdown, int* nSweepGrid, int* sweepPerXcd) {
    DAS_TRY
    DAS_CHECK(k, DAS_ERR_ARG, "null ksp handle");
    if (reason) *reason = k->reason;
    if (nBreakdown) *nBreakdown = k->nBreakdown;
    if (nSweepGrid) *nSweepGrid = k->useBilu ? k->bilu.launchGrid : 0;
    if (sweepPerXcd) *sweepPerXcd = k->useBilu ? k->bilu.launchPerXcd : 0;
    return DAS_OK;
    DAS_CATCH
}
// stability estimate of the factorisation (max |(LU)^-1 P e - e|; -1: not computed - amd.pcStabilityLimit 0) and the elimination order the
// check settled on (0 mesh numbering, 1 reverse Cuthill-McKee, 2 Cuthill-McKee, 3 mesh numbering backwards; -1: no check)
int das_ksp_get_pc_stability(das_ksp_t* k, double* estimate, int* orderUsed) {
    DAS_TRY
    DAS_CHECK(k, DAS_ERR_ARG, "null ksp handle");
    if (estimate) *estimate = k->pcStability;
    if (orderUsed) *orderUsed = k->pcOrderUsed;
    return DAS_OK;
    DAS_CATCH
}
// sub-domains of the factorisation inside this rank (amd.pcSubdomains): returns K (1: one factorisation); orders[K] / estimates[K] optional
int das_ksp_get_pc_subdomains(das_ksp_t* k, int* orders, double* estimates) {
    if (!k) return -1;
    for (int b = 0; b < k->nSub && k->nSub > 1; b++) {
        if (orders) orders[b] = k->subOrder[b];
        if (estimates) estimates[b] = k->subEst[b];
    }
    return k->nSub;
}
// 1 if the last preconditioner applies of this KSP took the A-DEF1 term A (Z u) from the precomputed sparse A Z (k_az_build / k_az_apply), 0 if
// they ran a full operator product (amd.pcCoarseSparseAZ 0, no assembled operator, build failed), -1: null handle
int das_ksp_coarse_sparse_az_active(das_ksp_t* k) { return k ? (k->coarse.active && k->coarse.deflated && k->coarse.azReady ? 1 : 0) : -1; }
// coarse space of the two-level preconditioner: number of aggregates (0 = none); aggOfCell[nCells] (optional) = aggregate or -1
int das_ksp_get_coarse(das_ksp_t* k, int* aggOfCell) {
    if (!k || !k->coarse.active) return 0;
    if (aggOfCell) std::copy(k->coarse.h_agg.begin(), k->coarse.h_agg.end(), aggOfCell);
    return k->coarse.nagg;
}
// multi-GPU: replace the per-rank coarse spaces by ONE coarse space over all ranks.  Every rank passes the size of the global
// coarse operator, the position of its own aggregates in it and, per local cell (owned AND ghost), the global aggregate (-1:
// none).  Collective: E = Z^T P Z is summed over the ranks (all-reduce through the installed communication) and inverted by
// every rank; afterwards a preconditioner apply costs one all-reduce of naggGlobal doubles.
int das_ksp_set_global_coarse(das_solver_t* s, das_ksp_t* k, int naggGlobal, int aggOffset, const int* aggRowGlobal) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(k && aggRowGlobal, DAS_ERR_ARG, "null argument");
    das_ksp::CoarsePC& C = k->coarse;
    DAS_CHECK(C.N > 0 && !C.h_agg.empty(), DAS_ERR_STATE, "the preconditioner of this KSP has no coarse space (amd.pcCoarseAggregates)");
    DAS_CHECK(aggOffset >= 0 && aggOffset + C.nagg <= naggGlobal, DAS_ERR_ARG, "aggregate offset out of range");
    std::vector<int> rows(aggRowGlobal, aggRowGlobal + C.N);
    for (long long c = 0; c < C.N; c++) {
        DAS_CHECK(rows[c] >= -1 && rows[c] < naggGlobal, DAS_ERR_ARG, "global aggregate id out of range");
        if (C.h_agg[c] >= 0) DAS_CHECK(rows[c] == aggOffset + C.h_agg[c], DAS_ERR_ARG, "owned cells must carry offset + local aggregate");
    }
    coarse_build_operator(s, k, naggGlobal, aggOffset, rows);
    if (C.active) return DAS_OK;
    // singular global coarse operator (every rank sees the same summed matrix, so every rank lands here): fall back to the
    // per-rank coarse spaces that were in place before the call (the failed build must not leave the
    // preconditioner without any coarse correction)
    coarse_build_operator(s, k, C.nagg, 0, C.h_agg);
    return 1;
    DAS_CATCH
}
int das_ksp_get_history(das_ksp_t* k, double* hist, int cap) {
    DAS_TRY
    DAS_CHECK(k && hist, DAS_ERR_ARG, "null argument");
    int m = std::min<int>(cap, (int)k->hist.size());
    std::copy(k->hist.begin(), k->hist.begin() + m, hist);
    return m;
    DAS_CATCH
}
int das_ksp_get_basis_info(das_ksp_t* k, int* fp32, double* mappedBytes, double* bytesPerVector) {
    DAS_TRY
    DAS_CHECK(k, DAS_ERR_ARG, "null argument");
    if (fp32) *fp32 = ((k->vf32 && !k->split) ? 1 : 0) | (k->split ? 2 : 0);
    if (mappedBytes) *mappedBytes = (double)k->V.mappedBytes;
    if (bytesPerVector) *bytesPerVector = k->vf32 ? (double)((k->Vn + 3) / 4 * 4) * (k->split ? 8.0 : 4.0) : (double)k->Vn * 8.0;  // basis_ld
    return DAS_OK;
    DAS_CATCH
}
int das_ksp_get_cycle_lengths(das_ksp_t* k, int* lens, int cap) {
    DAS_TRY
    DAS_CHECK(k && (lens || cap == 0), DAS_ERR_ARG, "null argument");
    int m = std::min<int>(cap, (int)k->cycleLens.size());
    std::copy(k->cycleLens.begin(), k->cycleLens.begin() + m, lens);
    return (int)k->cycleLens.size();
    DAS_CATCH
}
int das_ksp_run_fixed_device(das_solver_t* s, das_ksp_t* ksp, const double* d_rhs, double* d_sol, int iters) {
    DAS_TRY
    DAS_CHECK(ksp && d_rhs && d_sol && iters > 0, DAS_ERR_ARG, "bad argument");
    return run_gmres(s, ksp, d_rhs, d_sol, iters);
    DAS_CATCH
}
// the same solve as a state machine on device-resident rhs/sol: begin, advance by n iterations (returns 1 once the solve
// is over: converged or gmresMaxIters reached; never in `fixed` mode), end (closes the cycle, returns the fail code)
int das_ksp_begin_device(das_solver_t* s, das_ksp_t* ksp, const double* d_rhs, double* d_sol, int fixed) {
    DAS_TRY
    DAS_CHECK(ksp && d_rhs && d_sol, DAS_ERR_ARG, "bad argument");
    const int polyD = poly_degree(s, fixed != 0);
    if (ksp->idr) ksp->idr->pending = false;
    if (idr_selected(s, fixed != 0)) {  // IDR(s) is not resumable step by step: the first das_ksp_advance runs the whole solve
        need_init(s);
        IdrWork& I = idr_ws(s, ksp);
        I.pending = true; I.d_rhs = d_rhs; I.d_x = d_sol; I.rc = 0;
        ksp->run.reset();
        return DAS_OK;
    }
    gmres_begin(s, ksp, d_rhs, d_sol, fixed != 0, /* deflated */ false, polyD);
    return DAS_OK;
    DAS_CATCH
}
int das_ksp_advance(das_solver_t* s, das_ksp_t* ksp, int iters) {
    DAS_TRY
    DAS_CHECK(ksp && iters > 0, DAS_ERR_STATE, "das_ksp_begin_device has not been called");
    if (ksp->idr && !ksp->run && ksp->idr->d_x) {
        IdrWork& I = *ksp->idr;
        if (I.pending) { I.pending = false; I.rc = run_idrs(s, ksp, I.d_rhs, I.d_x); }
        return 1;
    }
    DAS_CHECK(ksp->run, DAS_ERR_STATE, "das_ksp_begin_device has not been called");
    return gmres_advance(s, ksp, iters) ? 1 : 0;
    DAS_CATCH
}
int das_ksp_end(das_solver_t* s, das_ksp_t* ksp) {
    DAS_TRY
    DAS_CHECK(ksp, DAS_ERR_STATE, "das_ksp_begin_device has not been called");
    if (ksp->idr && !ksp->run && ksp->idr->d_x) {
        IdrWork& I = *ksp->idr;
        if (I.pending) { I.pending = false; I.rc = run_idrs(s, ksp, I.d_rhs, I.d_x); }
        I.d_rhs = nullptr; I.d_x = nullptr;
        return I.rc;
    }
    DAS_CHECK(ksp->run, DAS_ERR_STATE, "das_ksp_begin_device has not been called");
    return gmres_end(s, ksp);
    DAS_CATCH
}
void das_ksp_destroy(das_ksp_t* k) { delete k; }

// ---- regression models of DASimpleFoam (reference DARegression.C, DAInputRegressionPar.C; kernels: das_regression.hpp) ---------------
// the option entry -> the view the kernels read (par stays null); every refusal names what it refuses
static RegView reg_view_from_spec(const std::string& what, const das_reg_spec_t* sp, bool needNames, std::vector<std::string>* names) {
    DAS_CHECK(sp && sp->model_type, DAS_ERR_ARG, what + ": null model description");
    RegView v;
    memset(&v, 0, sizeof(v));
    const std::string mt = sp->model_type;
    DAS_CHECK(mt != "externalTensorFlow", DAS_ERR_ARG,
              what + ": modelType externalTensorFlow is not built (the model runs in a Python callback outside the residual pass); neuralNetwork and radialBasisFunction are");
    DAS_CHECK(mt == "neuralNetwork" || mt == "radialBasisFunction", DAS_ERR_ARG,
              what + ": modelType " + mt + " not supported. Options are: neuralNetwork and radialBasisFunction");
    v.type = mt == "neuralNetwork" ? DAS_REG_NN : DAS_REG_RBF;
    DAS_CHECK(sp->n_inputs >= 1 && sp->n_inputs <= DAS_REG_MAX_INPUTS, DAS_ERR_ARG,
              what + ": " + std::to_string(sp->n_inputs) + " inputNames; 1 to DAS_REG_MAX_INPUTS = " + std::to_string(DAS_REG_MAX_INPUTS) + " are supported");
    v.nIn = sp->n_inputs;
    DAS_CHECK(sp->input_shift && sp->input_scale, DAS_ERR_ARG, what + ": inputShift and inputScale are needed, one value per inputName");
    static const char* const kNames[] = {"VoS", "PoD", "chiSA", "pGradStream", "PSoSS", "SCurv", "UOrth"};
    for (int k = 0; k < v.nIn; k++) {
        v.shift[k] = sp->input_shift[k];
        v.scale[k] = sp->input_scale[k];
        if (!needNames && !sp->input_names) continue;
        DAS_CHECK(sp->input_names && sp->input_names[k], DAS_ERR_ARG, what + ": null inputName");
        const std::string in = sp->input_names[k];
        DAS_CHECK(!(in.size() > 3 && in.compare(in.size() - 3, 3, "_dt") == 0), DAS_ERR_ARG,
                  what + ": inputName " + in + " is a time derivative; the *_dt features are not built (the solvers here are steady)");
        DAS_CHECK(in != "KoU2" && in != "ReWall" && in != "TauoK", DAS_ERR_ARG,
                  what + ": inputName " + in + " needs the turbulent kinetic energy k, which the Spalart-Allmaras model does not carry; it is not built");
        DAS_CHECK(in != "CoP", DAS_ERR_ARG, what + ": inputName CoP needs a face interpolation of nuTilda outside the stencil of nuTildaRes; it is not built");
        int id = -1;
        for (int q = 0; q < 7; q++) if (in == kNames[q]) id = q;
        DAS_CHECK(id >= 0, DAS_ERR_ARG, what + ": inputName " + in + " not supported. Options are: VoS, PoD, chiSA, pGradStream, PSoSS, SCurv, UOrth");
        v.feat[k] = id;
        if (names) names->push_back(in);
    }
    if (needNames || sp->output_name)
        DAS_CHECK(sp->output_name && std::string(sp->output_name) == "betaFINuTilda", DAS_ERR_ARG,
                  what + ": outputName " + (sp->output_name ? sp->output_name : "(null)") + " is not built; betaFINuTilda is");
    if (v.type == DAS_REG_NN) {
        DAS_CHECK(sp->n_hidden_layers >= 1 && sp->n_hidden_layers <= DAS_REG_MAX_LAYERS && sp->hidden_layer_neurons, DAS_ERR_ARG,
                  what + ": " + std::to_string(sp->n_hidden_layers) + " hidden layers; 1 to DAS_REG_MAX_LAYERS = " + std::to_string(DAS_REG_MAX_LAYERS) + " are supported");
        v.nLayers = sp->n_hidden_layers;
        for (int l = 0; l < v.nLayers; l++) {
            DAS_CHECK(sp->hidden_layer_neurons[l] >= 1 && sp->hidden_layer_neurons[l] <= DAS_REG_MAX_WIDTH, DAS_ERR_ARG,
                      what + ": hiddenLayerNeurons " + std::to_string(sp->hidden_layer_neurons[l]) + "; 1 to DAS_REG_MAX_WIDTH = " + std::to_string(DAS_REG_MAX_WIDTH) +
                          " neurons per layer are supported");
            v.width[l] = sp->hidden_layer_neurons[l];
        }
        const std::string af = sp->activation_function ? sp->activation_function : "";
        DAS_CHECK(af == "sigmoid" || af == "tanh" || af == "relu", DAS_ERR_ARG, what + ": activationFunction " + af + " not valid. Options are: sigmoid, tanh, and relu");
        v.act = af == "sigmoid" ? DAS_REG_SIGMOID : (af == "tanh" ? DAS_REG_TANH : DAS_REG_RELU);
        v.leaky = v.act == DAS_REG_RELU ? sp->leaky_coeff : 0.0;
    } else {
        DAS_CHECK(sp->n_rbfs >= 1 && sp->n_rbfs <= DAS_REG_MAX_RBFS, DAS_ERR_ARG,
                  what + ": nRBFs " + std::to_string(sp->n_rbfs) + "; 1 to DAS_REG_MAX_RBFS = " + std::to_string(DAS_REG_MAX_RBFS) + " are supported");
        v.nRBF = sp->n_rbfs;
    }
    v.nPar = reg_n_parameters(v);
    DAS_CHECK(v.nPar <= DAS_REG_MAX_PARAMS, DAS_ERR_ARG,
              what + ": " + std::to_string(v.nPar) + " parameters; at most DAS_REG_MAX_PARAMS = " + std::to_string(DAS_REG_MAX_PARAMS) + " are supported");
    // the LDS of the two kernels follows the model: what a workgroup may hold bounds it, here and not at the first launch
    const size_t ldsB = reg_backward_lds(v), ldsF = reg_forward_lds<Dual<1>>(v);
    DAS_CHECK(ldsB <= DAS_REG_MAX_LDS && ldsF <= DAS_REG_MAX_LDS, DAS_ERR_ARG,
              what + ": the model needs " + std::to_string(std::max(ldsB, ldsF)) + " bytes of LDS per workgroup (inputs + 2 x hidden neurons + 1 rows of " +
                  std::to_string(DAS_REG_BWD_TILE * sizeof(double)) + " bytes in the backward kernel); at most DAS_REG_MAX_LDS = " + std::to_string(DAS_REG_MAX_LDS) +
                  " are supported");
    v.outShift = sp->output_shift; v.outScale = sp->output_scale;
    v.upper = sp->output_upper_bound; v.lower = sp->output_lower_bound; v.dflt = sp->default_output_value;
    return v;
}
static void need_regression_solver(das_solver* s) {
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    DAS_CHECK(!s->cp.pimple, DAS_ERR_ARG, "DAPimpleFoam: regressionModel is not built");
    DAS_CHECK(s->cp.solver == DAS_SOLVER_SIMPLEFOAM, DAS_ERR_ARG,
              "the regressionModel option is built for DASimpleFoam only: not for " + s->opt.gets("solverName"));
    DAS_CHECK(s->owned.empty(), DAS_ERR_ARG, "the regression models run on an undecomposed solver (sharded solvers are not supported)");
}
static das_solver::RegModel& get_regression_model(das_solver* s, const char* name, int* index = nullptr) {
    for (size_t k = 0; k < s->regModels.size(); k++)
        if (name && s->regModels[k]->name == name) { if (index) *index = (int)k; return *s->regModels[k]; }
    throw Error(DAS_ERR_ARG, std::string("regressionModel has no model ") + (name ? name : "(null)"));
}
static void reg_sync(das_solver* s) {
    s->regSet.n = (int)s->regModels.size();
    for (int k = 0; k < s->regSet.n; k++) {
        das_solver::RegModel& m = *s->regModels[k];
        if (s->inited) { DAS_HIP(hipStreamSynchronize(s->stream)); m.d_par.upload(m.par); }
        m.v.par = m.d_par.p;
        s->regSet.v[k] = m.v;
    }
    s->cp.reg = s->regSet.n ? &s->regSet : nullptr;
    s->opEpoch++;
}
int das_define_regression_model(das_solver_t* s, const char* name, const das_reg_spec_t* spec) {
    DAS_TRY
    need_regression_solver(s);
    DAS_CHECK(name && *name, DAS_ERR_ARG, "regressionModel: a model needs a name");
    const std::string what = std::string("regressionModel ") + name;
    std::unique_ptr<das_solver::RegModel> m(new das_solver::RegModel);
    m->v = reg_view_from_spec(what, spec, true, &m->inputs);
    m->name = name;
    m->type = spec->model_type;
    m->par.assign(m->v.nPar, 0.0);
    DAS_CHECK(s->cp.beta_fi.empty(), DAS_ERR_ARG, what + ": a `field` input betaFINuTilda has been set; the model would overwrite it in every residual evaluation");
    for (const auto& e : s->cellFunctions)
        DAS_CHECK(!e.second.field, DAS_ERR_ARG,
                  what + ": the objective " + e.first + " reads betaFINuTilda; with a model active it would depend on the states, which is not built");
    const bool hadP = s->reg_needs_p();
    int at = -1;
    for (size_t k = 0; k < s->regModels.size(); k++) if (s->regModels[k]->name == name) at = (int)k;
    DAS_CHECK(at >= 0 || (int)s->regModels.size() < DAS_REG_MAX_MODELS, DAS_ERR_ARG,
              what + ": at most DAS_REG_MAX_MODELS = " + std::to_string(DAS_REG_MAX_MODELS) + " models are supported");
    if (at >= 0) s->regModels[at] = std::move(m);
    else s->regModels.push_back(std::move(m));
    reg_sync(s);
    if (s->reg_needs_p() != hadP) s->colored = false;  // the connectivity of nuTildaRes changed: new patterns, new colours
    return DAS_OK;
    DAS_CATCH
}
int das_get_regression_n_parameters(das_solver_t* s, const char* name) {
    DAS_TRY
    need_regression_solver(s);
    return get_regression_model(s, name).v.nPar;
    DAS_CATCH
}
int das_set_regression_parameters(das_solver_t* s, const char* name, const double* values, int n) {
    DAS_TRY
    need_regression_solver(s);
    das_solver::RegModel& m = get_regression_model(s, name);
    DAS_CHECK(values && n == m.v.nPar, DAS_ERR_ARG,
              std::string("regressionPar ") + name + ": " + std::to_string(n) + " values given, the model has " + std::to_string(m.v.nPar) + " parameters");
    m.par.assign(values, values + n);
    reg_sync(s);
    return DAS_OK;
    DAS_CATCH
}
int das_get_regression_parameters(das_solver_t* s, const char* name, double* values, int n) {
    DAS_TRY
    need_regression_solver(s);
    const das_solver::RegModel& m = get_regression_model(s, name);
    DAS_CHECK(values && n == m.v.nPar, DAS_ERR_ARG,
              std::string("regressionPar ") + name + ": room for " + std::to_string(n) + " values, the model has " + std::to_string(m.v.nPar) + " parameters");
    std::copy(m.par.begin(), m.par.end(), values);
    return DAS_OK;
    DAS_CATCH
}
int das_get_regression_model_info(das_solver_t* s, const char* name, int* nParameters, int* nInputs, int* modelType) {
    DAS_TRY
    need_regression_solver(s);
    const das_solver::RegModel& m = get_regression_model(s, name);
    if (nParameters) *nParameters = m.v.nPar;
    if (nInputs) *nInputs = m.v.nIn;
    if (modelType) *modelType = m.v.type;
    return DAS_OK;
    DAS_CATCH
}
// the three counts of a mask array: the two-stage fixed-order sum
static void reg_fail_counts(int nC, const unsigned char* d_mask, DevBuf<double>& d_part, long long* fail3, hipStream_t st) {
    const int nb = (int)std::min<long long>(nblk(nC, 256), 256);
    if (d_part.n < 3 * (size_t)nb + 3) d_part.alloc(3 * (size_t)nb + 3);
    hipLaunchKernelGGL(k_reg_count, dim3(nb), dim3(256), 0, st, nC, d_mask, d_part.p);
    hipLaunchKernelGGL(k_reg_count_final, dim3(1), dim3(256), 0, st, nb, (const double*)d_part.p, d_part.p + 3 * (size_t)nb);
    DAS_HIP(hipGetLastError());
    double h[3];
    DAS_HIP(hipMemcpyAsync(h, d_part.p + 3 * (size_t)nb, sizeof(h), hipMemcpyDeviceToHost, st));
    DAS_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < 3; q++) fail3[q] = (long long)h[q];
}
int das_get_regression_features(das_solver_t* s, const char* name, double* features, double* output, long long* fail3) {
    DAS_TRY
    need_regression_solver(s);
    need_init(s);
    const das_solver::RegModel& m = get_regression_model(s, name);
    const int nC = s->mesh.nC;
    hipStream_t st = s->stream;
    const ResParams prm = s->wk.bind(s->cp.solver, nC, s->mesh.nF, make_params(s->cp, s->opt, 0));
    launch_grad_simple<double, double>(s->dm, prm, s->d_W.p, s->wk, st);
    if (s->d_regFeat.n != (size_t)nC * m.v.nIn) s->d_regFeat.alloc((size_t)nC * m.v.nIn);
    if (s->d_regBeta.n != (size_t)nC) { s->d_regBeta.alloc(nC); s->d_regMask.alloc(nC); }
    launch_reg_forward<double, double>(m.v, nC, s->dm.cg, prm, s->d_W.p, (const double*)s->wk.gU.p, (const double*)s->wk.gP.p, nullptr, 0, s->d_regBeta.p,
                                       s->d_regFeat.p, s->d_regMask.p, st);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipStreamSynchronize(st));
    if (features) s->d_regFeat.download(features, (size_t)nC * m.v.nIn);
    if (output) s->d_regBeta.download(output, nC);
    if (fail3) reg_fail_counts(nC, s->d_regMask.p, s->d_regPart, fail3, st);
    return DAS_OK;
    DAS_CATCH
}
// out[k] = sum_c g[c] d beta_c / d theta_k on the device: k_reg_backward over a grid fixed by nC, then the partials in their order
static void launch_reg_backward(const RegView& v, int nC, const CellGeom* cg, const ResParams& prm, const double* W, const double* gU, const double* gP,
                                const double* featIn, const double* g, DevBuf<double>& d_part, double* d_out, hipStream_t st) {
    const int nb = (int)std::min<long long>(nblk(nC, DAS_REG_BWD_TILE), DAS_REG_BWD_MAX_BLOCKS);
    if (d_part.n < (size_t)nb * v.nPar) d_part.alloc((size_t)nb * v.nPar);
    const size_t lds = reg_backward_lds(v);
    if (lds > 64 * 1024) { DAS_HIP(hipFuncSetAttribute((const void*)k_reg_backward, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); }
    hipLaunchKernelGGL(k_reg_backward, dim3(nb), dim3(DAS_REG_BWD_THREADS), lds, st, v, nC, cg, prm, W, gU, gP, featIn, g, d_part.p);
    hipLaunchKernelGGL(k_reg_backward_final, dim3(nblk(v.nPar, 256)), dim3(256), 0, st, nb, v.nPar, (const double*)d_part.p, d_out);
    DAS_HIP(hipGetLastError());
}
int das_calc_dregressionpar_product(das_solver_t* s, const char* name, const char* outputName, const char* outputType, const double* seeds, double* product) {
    DAS_TRY
    need_regression_solver(s);
    need_init(s);
    DAS_CHECK(outputType && seeds && product, DAS_ERR_ARG, "null argument");
    int at = -1;
    const das_solver::RegModel& m = get_regression_model(s, name, &at);
    std::string ot = outputType;
    std::vector<double> rnSeeds;  // a residualNorm function: the residual product with the seeds dF/dR
    residual_norm_redirect(s, outputName, ot, seeds, rnSeeds);
    DAS_CHECK(ot == "residual" || ot == "function" || is_coupling(ot), DAS_ERR_ARG, "outputType not supported on this path: " + ot);
    if (ot != "residual") {  // no function and no coupling output reads the production term: exact zeros (an unknown output still fails by name)
        if (is_coupling(ot)) (void)coupling_size(s, ot, outputName);
        else if (!find_cell_function(s, outputName) && !find_mesh_function(s, outputName)) (void)get_function(s, outputName);
        std::fill(product, product + m.v.nPar, 0.0);
        return DAS_OK;
    }
    if (at + 1 != (int)s->regModels.size()) {  // a later model overwrites this one's output: the residual does not see it
        std::fill(product, product + m.v.nPar, 0.0);
        return DAS_OK;
    }
    hipStream_t st = s->stream;
    const int B = 256;
    const long long N = s->mesh.nC, n = s->n;
    // step 1: g_c = seeds . dR / d beta_c - one dual pass, the unit tangent set by k_reg_forward after the bounds (zero on clipped cells)
    struct Restore { das_solver* s; ~Restore() { s->cp.regSeed = 0; } } restore{s};
    s->cp.regSeed = 1;
    const ResParams prm = make_params(s->cp, s->opt, 0);
    if (s->d_Wd.n != (size_t)n) { s->d_Wd.alloc(n); s->d_Rd.alloc(n); }
    hipLaunchKernelGGL(k_lift, dim3(nblk(n, B)), dim3(B), 0, st, n, s->d_W.p, s->d_Wd.p);  // states carry no tangent
    eval_residual<Dual<1>>(s->dm, s->cp, prm, s->d_Wd.p, s->d_Rd.p, s->wk1, s->d_phiF.p, s->d_Told.p, st);
    DAS_HIP(hipMemcpyAsync(s->d_tmp2.p, seeds, n * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_field_product, dim3(nblk(N, B)), dim3(B), 0, st, N, (long long)prm.offN * N, s->d_Rd.p, s->d_tmp2.p, s->d_tmp1.p);
    // step 2: the reverse pass through the model at the same states (the gradients in double)
    const ResParams prmD = s->wk.bind(s->cp.solver, N, s->mesh.nF, prm);
    launch_grad_simple<double, double>(s->dm, prmD, s->d_W.p, s->wk, st);
    if (s->d_regOut.n < (size_t)m.v.nPar) s->d_regOut.alloc(m.v.nPar);
    launch_reg_backward(m.v, (int)N, s->dm.cg, prmD, s->d_W.p, s->wk.gU.p, s->wk.gP.p, nullptr, s->d_tmp1.p, s->d_regPart, s->d_regOut.p, st);
    DAS_HIP(hipMemcpyAsync(product, s->d_regOut.p, m.v.nPar * sizeof(double), hipMemcpyDeviceToHost, st));
    DAS_HIP(hipStreamSynchronize(st));
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reg_forward(const das_reg_spec_t* spec, const double* par, int nPar, int nCells, const double* features, double* beta, unsigned char* mask) {
    DAS_TRY
    RegView v = reg_view_from_spec("das_debug_reg_forward", spec, false, nullptr);
    DAS_CHECK(par && features && beta && nCells >= 1 && nPar == v.nPar, DAS_ERR_ARG,
              "das_debug_reg_forward: bad argument (the model has " + std::to_string(v.nPar) + " parameters)");
    DevBuf<double> d_par, d_feat, d_beta((size_t)nCells);
    DevBuf<unsigned char> d_mask((size_t)nCells);
    d_par.upload(par, nPar);
    d_feat.upload(features, (size_t)nCells * v.nIn);
    v.par = d_par.p;
    launch_reg_forward<double, double>(v, nCells, nullptr, ResParams{}, nullptr, nullptr, nullptr, d_feat.p, 0, d_beta.p, nullptr, d_mask.p, 0);
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipDeviceSynchronize());
    d_beta.download(beta, nCells);
    if (mask) d_mask.download(mask, nCells);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reg_backward(const das_reg_spec_t* spec, const double* par, int nPar, int nCells, const double* features, const double* g, double* out) {
    DAS_TRY
    RegView v = reg_view_from_spec("das_debug_reg_backward", spec, false, nullptr);
    DAS_CHECK(par && features && g && out && nCells >= 1 && nPar == v.nPar, DAS_ERR_ARG,
              "das_debug_reg_backward: bad argument (the model has " + std::to_string(v.nPar) + " parameters)");
    DevBuf<double> d_par, d_feat, d_g, d_part, d_out((size_t)nPar);
    d_par.upload(par, nPar);
    d_feat.upload(features, (size_t)nCells * v.nIn);
    d_g.upload(g, nCells);
    v.par = d_par.p;
    launch_reg_backward(v, nCells, nullptr, ResParams{}, nullptr, nullptr, nullptr, d_feat.p, d_g.p, d_part, d_out.p, 0);
    DAS_HIP(hipDeviceSynchronize());
    d_out.download(out, nPar);
    return DAS_OK;
    DAS_CATCH
}

int das_set_owned_mask(das_solver_t* s, const unsigned char* owned) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    if (!owned) { s->owned.clear(); return DAS_OK; }
    DAS_CHECK(s->regModels.empty(), DAS_ERR_ARG, "the regression models run on an undecomposed solver (sharded solvers are not supported)");
    DAS_CHECK(s->actuatorDisks.empty(), DAS_ERR_ARG, "the fvSource actuator disks run on an undecomposed solver (sharded solvers are not supported)");
    s->owned.assign(owned, owned + s->n);
    if (s->inited) s->d_owned.upload(s->owned);
    return DAS_OK;
    DAS_CATCH
}
int das_set_comm(das_solver_t* s, das_halo_cb halo, das_allreduce_cb allreduce, void* user) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    s->halo_cb = halo;
    s->allreduce_cb = allreduce;
    s->comm_user = user;
    return DAS_OK;
    DAS_CATCH
}
// ---- native communication (das_comm.hpp) ---------------------------------------------------------------------------
// rank 0 creates the RCCL unique id (128 bytes); the host side distributes it (bootstrap only)
// step 1 of the native set-up, LOCAL (no collective inside): bind RCCL.  The ranks agree on the result before any of them
// enters the collective ncclCommInitRank - a rank that cannot load the library must not leave the others blocked there
int das_comm_load_rccl(void) {
    DAS_TRY
    rccl().load();
    return DAS_OK;
    DAS_CATCH
}
int das_comm_unique_id(char* out128) {
    DAS_TRY
    DAS_CHECK(out128, DAS_ERR_ARG, "null argument");
    rccl().load();
    ncclUniqueId id;
    DAS_NCCL(rccl().GetUniqueId(&id));
    static_assert(sizeof(id) == 128, "ncclUniqueId size");
    std::memcpy(out128, &id, sizeof(id));
    return DAS_OK;
    DAS_CATCH
}
int das_comm_init_rccl(das_solver_t* s, int rank, int world, const char* id128) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(id128 && world >= 1 && rank >= 0 && rank < world, DAS_ERR_ARG, "bad argument");
    rccl().load();
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    DAS_HIP(hipSetDevice(s->device));
    if (s->halo.comm) { (void)rccl().CommDestroy(s->halo.comm); s->halo.comm = nullptr; }  // re-install: no leaked communicator
    DAS_NCCL(rccl().CommInitRank(&s->halo.comm, world, id, rank));
    s->halo.rank = rank;
    s->halo.world = world;
    s->halo.ensure_streams();
    return DAS_OK;
    DAS_CATCH
}
// host-staged transport of the same plan (gloo tests on single-GPU boxes): cb(d_send, d_recv) moves the packed segments
int das_set_exchange_cb(das_solver_t* s, das_exchange_cb cb, void* user) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    s->halo.exchange_cb = cb;
    s->halo.cb_user = user;
    return DAS_OK;
    DAS_CATCH
}
// the halo plan: per peer the extended rows I hold for it (send, evaluated first) and my owned rows it holds as ghosts
// (recv, in the peer's send order); ghostIdx = all local ghost rows (zeroed after the reduction)
int das_comm_set_halo(das_solver_t* s, int npeers, const int* peers, const long long* sendOff, const int* sendIdx, const long long* recvOff,
                      const int* recvIdx, long long nGhost, const int* ghostIdx) {
    DAS_TRY
    need_init(s);
    DAS_CHECK(npeers >= 0 && (npeers == 0 || (peers && sendOff && recvOff)), DAS_ERR_ARG, "bad argument");
    HaloPlan& H = s->halo;
    H.peers.assign(peers, peers + npeers);
    H.sendOff.assign(1, 0);
    H.recvOff.assign(1, 0);
    if (npeers) { H.sendOff.assign(sendOff, sendOff + npeers + 1); H.recvOff.assign(recvOff, recvOff + npeers + 1); }
    H.nSend = H.sendOff.back(); H.nRecv = H.recvOff.back(); H.nGhost = nGhost;
    for (long long k = 0; k < H.nSend; k++) DAS_CHECK(sendIdx[k] >= 0 && sendIdx[k] < s->n, DAS_ERR_ARG, "send index out of range");
    for (long long k = 0; k < H.nRecv; k++) DAS_CHECK(recvIdx[k] >= 0 && recvIdx[k] < s->n, DAS_ERR_ARG, "recv index out of range");
    if (H.nSend) { H.sendIdx.upload(sendIdx, H.nSend); H.sendBuf.alloc(H.nSend); }
    if (H.nRecv) { H.recvIdx.upload(recvIdx, H.nRecv); H.recvBuf.alloc(H.nRecv); }
    if (nGhost) H.ghostIdx.upload(ghostIdx, nGhost);
    H.ensure_streams();
    H.active = true;
    return DAS_OK;
    DAS_CATCH
}
// additive-Schwarz overlap across ranks (adjEqnOption.asmOverlap; reference DALinearEqn.C:212-216, PCASMSetOverlap): pcMask[state] != 0 for
// the unknowns of this rank's sub-domain solve (owned + overlap rings; a superset of the owned mask), and per peer of the halo plan (same
// peer order as das_comm_set_halo) the owned states it needs from me (ovSend) and my overlap ghost states it owns (ovRecv, in its send
// order).  Call before calcdRdWT(1) / createMLRKSPMatrixFree: the PC matrix keeps the residual columns of the overlap, the factorisation
// covers them, every apply gathers the overlap entries of its input first and keeps the owned part of its result (restricted variant).
// pcMask == NULL switches the overlap off (block-Jacobi across ranks).
int das_set_pc_overlap(das_solver_t* s, const unsigned char* pcMask, int npeers, const long long* ovSendOff, const int* ovSendIdx, const long long* ovRecvOff,
                       const int* ovRecvIdx) {
    DAS_TRY
    need_init(s);
    HaloPlan& H = s->halo;
    if (!pcMask) { s->pcMask.clear(); H.ovActive = false; return DAS_OK; }
    DAS_CHECK(!s->owned.empty(), DAS_ERR_STATE, "das_set_pc_overlap: das_set_owned_mask first");
    DAS_CHECK(H.active && npeers == (int)H.peers.size() && (npeers == 0 || (ovSendOff && ovRecvOff)), DAS_ERR_ARG, "das_set_pc_overlap: the peer list is that of das_comm_set_halo");
    s->pcMask.assign(pcMask, pcMask + s->n);
    for (long long i = 0; i < s->n; i++) DAS_CHECK(!s->owned[i] || s->pcMask[i], DAS_ERR_ARG, "das_set_pc_overlap: the sub-domain must contain every owned unknown");
    s->d_pcMask.upload(s->pcMask);
    H.ovSendOff.assign(1, 0);
    H.ovRecvOff.assign(1, 0);
    if (npeers) { H.ovSendOff.assign(ovSendOff, ovSendOff + npeers + 1); H.ovRecvOff.assign(ovRecvOff, ovRecvOff + npeers + 1); }
    H.nOvSend = H.ovSendOff.back(); H.nOvRecv = H.ovRecvOff.back();
    for (long long q = 0; q < H.nOvSend; q++) DAS_CHECK(ovSendIdx[q] >= 0 && ovSendIdx[q] < s->n && s->owned[ovSendIdx[q]], DAS_ERR_ARG, "das_set_pc_overlap: send entries are owned states");
    for (long long q = 0; q < H.nOvRecv; q++)
        DAS_CHECK(ovRecvIdx[q] >= 0 && ovRecvIdx[q] < s->n && !s->owned[ovRecvIdx[q]] && s->pcMask[ovRecvIdx[q]], DAS_ERR_ARG, "das_set_pc_overlap: recv entries are overlap ghost states");
    if (H.nOvSend) { H.ovSendIdx.upload(ovSendIdx, H.nOvSend); H.ovSendBuf.alloc(H.nOvSend); }
    if (H.nOvRecv) { H.ovRecvIdx.upload(ovRecvIdx, H.nOvRecv); H.ovRecvBuf.alloc(H.nOvRecv); }
    H.ovActive = true;
    return DAS_OK;
    DAS_CATCH
}
// host-staged transport of the overlap gather (gloo tests on single-GPU boxes): cb(d_send, d_recv) moves the packed segments
int das_set_gather_cb(das_solver_t* s, das_exchange_cb cb, void* user) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    s->halo.gather_cb = cb;
    s->halo.gather_user = user;
    return DAS_OK;
    DAS_CATCH
}
int das_comm_is_native(das_solver_t* s) { return (s && s->halo.comm) ? 1 : 0; }
// drop a native communicator again (the ranks agreed to use the callback transport instead)
int das_comm_reset(das_solver_t* s) {
    DAS_TRY
    DAS_CHECK(s, DAS_ERR_ARG, "null solver handle");
    if (s->halo.comm) { (void)rccl().CommDestroy(s->halo.comm); s->halo.comm = nullptr; }
    return DAS_OK;
    DAS_CATCH
}

int das_set_stream(das_solver_t* s, void* hip_stream) {
    DAS_TRY
    need_init(s);
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    s->stream = (hipStream_t)hip_stream;
    s->own_stream = false;
    return DAS_OK;
    DAS_CATCH
}

// One timed shape of the two tuning entries below (das_debug_orth_bench*): they name n, K, reps, j = K - 1, the basis V (leading dimension ld, lo array or null),
// u = its slot K - 1, w, sc and the empty buffer partial, which every inner-product shape sizes for its own slots.
#define DAS_DOT(VT, R) do { if (rows == R) { partial.alloc((size_t)2 * K * multidot2_nbw<R>(n)); \
    *ms_dots = orth_bench_ms(reps, [&] { launch_multidot2_pass<R, VT>(0, n, K, V.p, ld, u, w.p, partial.p); }); } } while (0)
#define DAS_UPD(VT, U, R) do { if (unroll == U && rpt == R) \
    *ms_update = orth_bench_ms(reps, [&] { launch_dcgs2_update_pass<U, R, VT>(0, n, j, V.p, ld, sc.p, 0.5, 1.0, w.p, lo); }); } while (0)
#define DAS_DOTW(R, NT) do { if (rows == R) { partial.alloc((size_t)2 * K * multidot2w_nbw(n, R)); \
    *ms_dots = orth_bench_ms(reps, [&] { launch_multidot2w_pass<R, NT>(0, n, K, V.p, ld, u, w.p, partial.p); }); } } while (0)
#define DAS_UPDW(U, R, NT) do { if (unroll == U && rpt == R) \
    *ms_update = orth_bench_ms(reps, [&] { launch_dcgs2w_update<U, R, NT>(0, n, j, V.p, ld, sc.p, 0.5, 1.0, w.p, lo); }); } while (0)
#define DAS_WIDE(NT) do { DAS_DOTW(1, NT); DAS_DOTW(2, NT); DAS_DOTW(4, NT); \
    DAS_UPDW(2, 1, NT); DAS_UPDW(4, 1, NT); DAS_UPDW(8, 1, NT); DAS_UPDW(2, 2, NT); DAS_UPDW(4, 2, NT); } while (0)
// Tuning hook (tools/orth_bench.py): times the two kernels of the delayed re-orthogonalisation on synthetic vectors of length n
// against K basis vectors, for the compiled variants (rows per thread of the inner products; unroll / rows per thread of
// the update).  No solver handle: it only needs the device.
int das_debug_orth_bench(long long n, int K, int reps, int rows, int unroll, int rpt, double* ms_dots, double* ms_update) {
    DAS_TRY
    DAS_CHECK(n > 0 && K > 1 && reps > 0 && ms_dots && ms_update, DAS_ERR_ARG, "das_debug_orth_bench: bad arguments");
    const long long ld = n;
    DevBuf<double> V((size_t)(K + 2) * ld), w(n), partial, sc(2 * (size_t)K);
    V.zero(); w.zero(); sc.zero();
    float* lo = nullptr;
    const double* u = V.p + (long long)(K - 1) * ld;
    *ms_dots = -1.0; *ms_update = -1.0;
    const int j = K - 1;
    DAS_DOT(double, 4); DAS_DOT(double, 8); DAS_DOT(double, 16);
    DAS_UPD(double, 4, 1); DAS_UPD(double, 8, 1); DAS_UPD(double, 16, 1); DAS_UPD(double, 4, 2); DAS_UPD(double, 8, 2); DAS_UPD(double, 4, 4);
    DAS_UPD(double, 8, 4);
    return DAS_OK;
    DAS_CATCH
}

// The same for the float basis the solver runs by default (tools/orth_bench.py --split): synthetic buffers in the solver's layout
// (fmt 2 = split: ld = 2 n4, lo n4 floats into a slot; fmt 1 = fp32: ld = n4, no lo array; n4 = n rounded up to a multiple of 4).
// variant 0: the one-dword-per-lane kernels (rows 4 | 8 | 16; unroll, rpt as above); 1: the 16-byte-load kernels (rows = groups of 4
// rows per lane 1 | 2 | 4; (unroll, rpt) = (vectors in flight, groups of 4 rows per lane)); 2: the same with non-temporal loads.
// rows = 0 / unroll = 0 skips that kernel; a combination that is not compiled returns -1 ms.
int das_debug_orth_bench_split(long long n, int K, int reps, int fmt, int variant, int rows, int unroll, int rpt, double* ms_dots, double* ms_update) {
    DAS_TRY
    DAS_CHECK(n > 0 && n < (1LL << 30) && K > 1 && reps > 0 && ms_dots && ms_update, DAS_ERR_ARG, "das_debug_orth_bench_split: bad arguments");
    DAS_CHECK((fmt == KRY_FP32 || fmt == KRY_SPLIT) && variant >= 0 && variant <= 2, DAS_ERR_ARG, "das_debug_orth_bench_split: fmt 1 | 2, variant 0 | 1 | 2");
    const long long n4 = (n + 3) / 4 * 4, ld = fmt == KRY_SPLIT ? 2 * n4 : n4;
    DevBuf<float> V((size_t)(K + 2) * ld);
    DevBuf<double> w(n4), partial, sc(2 * (size_t)K);
    V.zero(); w.zero(); sc.zero();
    float* lo = fmt == KRY_SPLIT ? V.p + n4 : nullptr;
    const float* u = V.p + (long long)(K - 1) * ld;
    *ms_dots = -1.0; *ms_update = -1.0;
    const int j = K - 1;
    if (variant == 0) {
        DAS_DOT(float, 4); DAS_DOT(float, 8); DAS_DOT(float, 16);
        DAS_UPD(float, 4, 1); DAS_UPD(float, 8, 1); DAS_UPD(float, 4, 2); DAS_UPD(float, 8, 2); DAS_UPD(float, 4, 4);
    }
    if (variant == 1) DAS_WIDE(false);
    if (variant == 2) DAS_WIDE(true);
    return DAS_OK;
    DAS_CATCH
}
#undef DAS_DOT
#undef DAS_UPD
#undef DAS_DOTW
#undef DAS_UPDW
#undef DAS_WIDE
// the 16-byte-load path of the float basis on (1) / off (0) for every later launch of this process; *previous: what it was.  The tests
// and the timing tool run both paths of one build with it; the solver never calls it.
int das_debug_set_orth_wide(int on, int* previous) {
    if (previous) *previous = g_orth_wide;
    g_orth_wide = on ? 1 : 0;
    return DAS_OK;
}
// would das_debug_krylov_dots2 / das_debug_krylov_dcgs2_update on a basis of this shape (their uploads are allocation-aligned) run the
// 16-byte-load kernels?  The launch helpers' own predicate on stand-in pointers.
int das_debug_krylov_wide_eligible(long long n, int fmt, long long ld, int* dots, int* update) {
    DAS_TRY
    DAS_CHECK(dots && update, DAS_ERR_ARG, "das_debug_krylov_wide_eligible: null pointer");
    const float* base = reinterpret_cast<const float*>((uintptr_t)1 << 20);
    const bool f = fmt == KRY_FP32 || fmt == KRY_SPLIT;
    *dots = (f && g_orth_wide && orth_wide_ok(n, base, nullptr, ld, base + ld, base)) ? 1 : 0;
    *update = (f && g_orth_wide && orth_wide_ok(n, base, fmt == KRY_SPLIT ? base + n : nullptr, ld, nullptr, base)) ? 1 : 0;
    return DAS_OK;
    DAS_CATCH
}

// Test-only entries (tests/test_gpu_krylov_kernels.py): every Krylov kernel of the GMRES engine on caller data through the launch
// helpers the solver uses.  No solver handle, nothing in the product path calls them.
int das_debug_krylov_dots2(long long n, int K, int fmt, const void* V, long long ld, const double* v, double* out) {
    DAS_TRY
    krylov_check_basis("das_debug_krylov_dots2", n, K, fmt, V, ld);
    DAS_CHECK(v && out, DAS_ERR_ARG, "das_debug_krylov_dots2: null pointer");
    if (fmt == KRY_FP64) debug_krylov_dots2<double>(n, K, V, ld, v, out);
    else debug_krylov_dots2<float>(n, K, V, ld, v, out);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_dcgs2_update(long long n, int j, int fmt, void* V, long long ld, int nslots, const double* sc, double gamma, double ralpha,
                                  const double* v) {
    DAS_TRY
    DAS_CHECK(j >= 0, DAS_ERR_ARG, "das_debug_krylov_dcgs2_update: j must not be negative");
    krylov_check_basis("das_debug_krylov_dcgs2_update", n, nslots, fmt, V, ld);
    DAS_CHECK(nslots >= j + 2, DAS_ERR_ARG, "das_debug_krylov_dcgs2_update: the basis needs slots 0 .. j + 1");
    DAS_CHECK(v && (sc || j == 0), DAS_ERR_ARG, "das_debug_krylov_dcgs2_update: null pointer");
    if (fmt == KRY_FP64) debug_krylov_dcgs2_update<double>(n, j, false, V, ld, nslots, sc, gamma, ralpha, v);
    else debug_krylov_dcgs2_update<float>(n, j, fmt == KRY_SPLIT, V, ld, nslots, sc, gamma, ralpha, v);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_multidot(long long n, int m, int fmt, const void* V, long long ld, const double* w, double* out) {
    DAS_TRY
    DAS_CHECK(m >= 0, DAS_ERR_ARG, "das_debug_krylov_multidot: m must not be negative");
    krylov_check_basis("das_debug_krylov_multidot", n, std::max(m, 1), fmt, m > 0 ? V : (const void*)w, ld);
    DAS_CHECK(w && out, DAS_ERR_ARG, "das_debug_krylov_multidot: null pointer");
    if (fmt == KRY_FP64) debug_krylov_multidot<double>(n, m, V, ld, w, out);
    else debug_krylov_multidot<float>(n, m, V, ld, w, out);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_multiaxpy(long long n, int m, int fmt, const void* V, long long ld, const double* h, int wfloat, void* w, long long wlen) {
    DAS_TRY
    krylov_check_basis("das_debug_krylov_multiaxpy", n, m, fmt, V, ld);
    DAS_CHECK(h && w, DAS_ERR_ARG, "das_debug_krylov_multiaxpy: null pointer");
    DAS_CHECK(wlen >= n, DAS_ERR_ARG, "das_debug_krylov_multiaxpy: w shorter than n");
    DAS_CHECK(!wfloat || fmt == KRY_FP32, DAS_ERR_ARG, "das_debug_krylov_multiaxpy: a float w goes with the fp32 basis only");
    if (fmt == KRY_FP64) debug_krylov_multiaxpy<double, double>(n, m, false, V, ld, h, w, wlen);
    else if (wfloat) debug_krylov_multiaxpy<float, float>(n, m, false, V, ld, h, w, wlen);
    else debug_krylov_multiaxpy<float, double>(n, m, fmt == KRY_SPLIT, V, ld, h, w, wlen);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_lincomb(long long n, int m, int fmt, const void* V, long long ld, const double* c, double* y, long long ylen) {
    DAS_TRY
    krylov_check_basis("das_debug_krylov_lincomb", n, m, fmt, V, ld);
    DAS_CHECK(c && y, DAS_ERR_ARG, "das_debug_krylov_lincomb: null pointer");
    DAS_CHECK(ylen >= n, DAS_ERR_ARG, "das_debug_krylov_lincomb: y shorter than n");
    if (fmt == KRY_FP64) debug_krylov_lincomb<double>(n, m, false, V, ld, c, y, ylen);
    else debug_krylov_lincomb<float>(n, m, fmt == KRY_SPLIT, V, ld, c, y, ylen);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_scale_to(long long n, double a, int use, const void* x, void* y, long long ylen) {
    DAS_TRY
    DAS_CHECK(n > 0, DAS_ERR_ARG, "das_debug_krylov_scale_to: n must be positive");
    DAS_CHECK(use >= 0 && use <= 4, DAS_ERR_ARG, "das_debug_krylov_scale_to: use is 0 (double -> double), 1 (double -> float), 2 (double -> split), 3 (split -> double) or 4 (float -> double)");
    DAS_CHECK(x && y, DAS_ERR_ARG, "das_debug_krylov_scale_to: null pointer");
    DAS_CHECK(ylen >= (use == 2 ? 2 * n : n), DAS_ERR_ARG, "das_debug_krylov_scale_to: y shorter than n (split: 2 n)");
    if (use == 0) debug_krylov_scale_to<double, double>(n, a, false, false, x, y, ylen);
    else if (use == 1) debug_krylov_scale_to<double, float>(n, a, false, false, x, y, ylen);
    else if (use == 2) debug_krylov_scale_to<double, float>(n, a, false, true, x, y, ylen);
    else if (use == 3) debug_krylov_scale_to<float, double>(n, a, true, false, x, y, ylen);
    else debug_krylov_scale_to<float, double>(n, a, false, false, x, y, ylen);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_block_tn(long long n, int K, int s, const double* V, long long ldv, long long voff, const double* W, long long ldw, double* C) {
    DAS_TRY
    krylov_check_block("das_debug_krylov_block_tn", n, K, s);
    DAS_CHECK(V && W && C, DAS_ERR_ARG, "das_debug_krylov_block_tn: null pointer");
    DAS_CHECK(ldv >= n && ldw >= n && voff >= 0, DAS_ERR_ARG, "das_debug_krylov_block_tn: leading dimension below n or negative offset");
    debug_krylov_block_tn(n, K, s, V, ldv, voff, W, ldw, C);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_block_nn_sub(long long n, int K, int s, const double* V, long long ldv, const double* C, double* W, long long ldw) {
    DAS_TRY
    krylov_check_block("das_debug_krylov_block_nn_sub", n, K, s);
    DAS_CHECK(V && W && C, DAS_ERR_ARG, "das_debug_krylov_block_nn_sub: null pointer");
    DAS_CHECK(ldv >= n && ldw >= n, DAS_ERR_ARG, "das_debug_krylov_block_nn_sub: leading dimension below n");
    debug_krylov_block_nn_sub(n, K, s, V, ldv, C, W, ldw);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_block_right_mult(long long n, int s, double* W, long long ldw, const double* T) {
    DAS_TRY
    krylov_check_block("das_debug_krylov_block_right_mult", n, 1, s);
    DAS_CHECK(W && T, DAS_ERR_ARG, "das_debug_krylov_block_right_mult: null pointer");
    DAS_CHECK(ldw >= n, DAS_ERR_ARG, "das_debug_krylov_block_right_mult: leading dimension below n");
    debug_krylov_block_right_mult(n, s, W, ldw, T);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_block_lincomb(long long n, int K, int s, const double* V, long long ldv, const double* C, double* Y, long long ldy) {
    DAS_TRY
    krylov_check_block("das_debug_krylov_block_lincomb", n, K, s);
    DAS_CHECK(V && C && Y, DAS_ERR_ARG, "das_debug_krylov_block_lincomb: null pointer");
    DAS_CHECK(ldv >= n && ldy >= n, DAS_ERR_ARG, "das_debug_krylov_block_lincomb: leading dimension below n");
    debug_krylov_block_lincomb(n, K, s, V, ldv, C, Y, ldy);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_krylov_block_spmm(long long n, int s, const long long* rp, const int* ci, const double* val, const double* X, long long ldx, double* Y,
                                long long ldy) {
    DAS_TRY
    krylov_check_block("das_debug_krylov_block_spmm", n, 1, s);
    DAS_CHECK(rp && X && Y, DAS_ERR_ARG, "das_debug_krylov_block_spmm: null pointer");
    DAS_CHECK(ldx >= n && ldy >= n, DAS_ERR_ARG, "das_debug_krylov_block_spmm: leading dimension below n");
    DAS_CHECK(rp[0] == 0, DAS_ERR_ARG, "das_debug_krylov_block_spmm: rowptr[0] must be 0");
    for (long long i = 0; i < n; i++) DAS_CHECK(rp[i + 1] >= rp[i], DAS_ERR_ARG, "das_debug_krylov_block_spmm: rowptr decreases");
    const long long nnz = rp[n];
    DAS_CHECK(nnz == 0 || (ci && val), DAS_ERR_ARG, "das_debug_krylov_block_spmm: null pointer");
    for (long long k = 0; k < nnz; k++) DAS_CHECK(ci[k] >= 0 && ci[k] < n, DAS_ERR_ARG, "das_debug_krylov_block_spmm: column index out of range");
    debug_krylov_block_spmm(n, s, rp, ci, val, X, ldx, Y, ldy);
    return DAS_OK;
    DAS_CATCH
}

// Test-only entries (tests/test_gpu_bilu_kernels.py): the node-block ILU(0) on a caller-made structure through the numeric setup and
// the sweeps the solver uses (das_bilu_debug.hpp).  The structure is checked on the host before anything is launched.
int das_debug_bilu_factor(const das_bilu_debug_t* in, long long* Lptr, long long* Uptr, int* Lcol, int* Ucol, void* Lval, void* Uval, double* invD,
                          int* nshift) {
    DAS_TRY
    bilu_debug_check("das_debug_bilu_factor", in);
    DAS_CHECK(Lptr && Uptr && Lcol && Ucol && Lval && Uval && invD && nshift, DAS_ERR_ARG, "das_debug_bilu_factor: null pointer");
    debug_bilu_factor(*in, Lptr, Uptr, Lcol, Ucol, Lval, Uval, invD, nshift);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_bilu_apply(const das_bilu_debug_t* in, int nrhs, long long ld, const double* b, double* out, int twice, double* y, double* z,
                         int* abortFlag, int* info) {
    DAS_TRY
    bilu_debug_check("das_debug_bilu_apply", in);
    DAS_CHECK(nrhs >= 1 && nrhs <= 8, DAS_ERR_ARG, "das_debug_bilu_apply: 1 to 8 right-hand sides");
    DAS_CHECK(ld >= in->n, DAS_ERR_ARG, "das_debug_bilu_apply: leading dimension below n");
    DAS_CHECK(b && out && y && z && abortFlag && info, DAS_ERR_ARG, "das_debug_bilu_apply: null pointer");
    debug_bilu_apply(*in, nrhs, ld, b, out, twice, y, z, abortFlag, info);
    return DAS_OK;
    DAS_CATCH
}

// Test-only entries (tests/test_gpu_graph_kernels.py, tests/test_gpu_opmat_kernels.py): the graph set-up, the jacLowerBounds filter, the
// packed operator and the ghost-row product on caller-made structures through the helpers the solver uses (das_graph_debug.hpp).
// Everything a kernel would index with is checked on the host before anything is launched.
#define DAS_GRAPH_DEVICE(who) DAS_CHECK(das_device_count() > 0, DAS_ERR_NO_DEVICE, std::string(who) + ": no HIP device visible")
int das_debug_graph_scan(long long n, const int* cnt, long long* out, long long* total) {
    DAS_TRY
    const std::string who = "das_debug_graph_scan";
    graph_check_sizes(who, n);
    DAS_CHECK(cnt && out && total, DAS_ERR_ARG, who + ": null pointer");
    for (long long i = 0; i < n; i++) DAS_CHECK(cnt[i] >= 0, DAS_ERR_ARG, who + ": negative count");
    DAS_GRAPH_DEVICE(who);
    debug_graph_scan(n, cnt, out, total);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_graph_transpose(long long n, const long long* rowptr, const int* col, long long* trp, int* tcol) {
    DAS_TRY
    const std::string who = "das_debug_graph_transpose";
    graph_check_sizes(who, n);
    DAS_CHECK(rowptr && col && trp && tcol, DAS_ERR_ARG, who + ": null pointer");
    graph_check_csr(who, n, rowptr, col, n, true);
    DAS_CHECK(rowptr[n] > 0, DAS_ERR_ARG, who + ": a pattern without entries");
    DAS_GRAPH_DEVICE(who);
    debug_graph_transpose(n, rowptr, col, trp, tcol);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_graph_nets(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, long long* cptr, int* crow, int* cpos,
                         unsigned char* isStart, long long* total) {
    DAS_TRY
    const std::string who = "das_debug_graph_nets";
    graph_check_sizes(who, n);
    DAS_CHECK(rowptr && col && cptr && crow && cpos && isStart && total && (keep || nKeep == 0), DAS_ERR_ARG, who + ": null pointer");
    graph_check_csr(who, n, rowptr, col, n, true);
    DAS_CHECK(rowptr[n] > 0, DAS_ERR_ARG, who + ": a pattern without entries");
    DAS_CHECK(nKeep >= 0 && nKeep <= n, DAS_ERR_ARG, who + ": nKeep outside [0, n]");
    {
        std::vector<unsigned char> seen((size_t)n, 0);
        for (long long q = 0; q < nKeep; q++) {
            DAS_CHECK(keep[q] >= 0 && keep[q] < n, DAS_ERR_ARG, who + ": kept row out of range");
            DAS_CHECK(!seen[keep[q]], DAS_ERR_ARG, who + ": kept row repeated");
            seen[keep[q]] = 1;
        }
    }
    DAS_GRAPH_DEVICE(who);
    debug_graph_nets(n, rowptr, col, nKeep, keep, cptr, crow, cpos, isStart, total);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_graph_rows_gather(long long nSel, const long long* rows, long long n, const long long* rowptr, const int* col, const long long* dst, int* out,
                                long long outLen) {
    DAS_TRY
    const std::string who = "das_debug_graph_rows_gather";
    graph_check_sizes(who, n);
    DAS_CHECK(nSel > 0 && outLen > 0, DAS_ERR_ARG, who + ": sizes must be positive");
    DAS_CHECK(rows && rowptr && dst && out, DAS_ERR_ARG, who + ": null pointer");
    graph_check_csr(who, n, rowptr, col, n, false);
    for (long long q = 0; q < nSel; q++) {
        DAS_CHECK(rows[q] >= 0 && rows[q] < n, DAS_ERR_ARG, who + ": row index out of range");
        DAS_CHECK(dst[q] >= 0 && dst[q] <= outLen - (rowptr[rows[q] + 1] - rowptr[rows[q]]), DAS_ERR_ARG, who + ": a gathered row does not fit into out");
    }
    DAS_GRAPH_DEVICE(who);
    debug_graph_rows_gather(nSel, rows, n, rowptr, col, dst, out, outLen);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_compact(long long n, const long long* rowptr, const int* col, const double* vals, double bound, int useBound, const unsigned char* owned,
                      long long* nrp, int* nci, double* nv, long long* nnzOut) {
    DAS_TRY
    const std::string who = "das_debug_compact";
    graph_check_sizes(who, n);
    DAS_CHECK(rowptr && nrp && nci && nv && nnzOut, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(useBound == 0 || useBound == 1, DAS_ERR_ARG, who + ": useBound is 0 or 1");
    graph_check_csr(who, n, rowptr, col, n, false);
    DAS_CHECK(rowptr[n] == 0 || vals, DAS_ERR_ARG, who + ": null pointer");
    DAS_GRAPH_DEVICE(who);
    debug_compact(n, rowptr, col, vals, bound, useBound != 0, owned, nrp, nci, nv, nnzOut);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_vecpack(long long n, const long long* rowptr, const int* col, const double* vals, long long row0, long long nG, int* built, long long* cptr,
                      unsigned char* data, long long dataCap, long long* nChunks, const double* x, double* y, long long ylen) {
    DAS_TRY
    const std::string who = "das_debug_vecpack";
    graph_check_sizes(who, n);
    DAS_CHECK(nG > 0, DAS_ERR_ARG, who + ": sizes must be positive");
    DAS_CHECK(rowptr && built && cptr && data && nChunks && (!x || y), DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(row0 >= 0 && nG <= n && row0 <= n - 3 * nG, DAS_ERR_ARG, who + ": the group rows [row0, row0 + 3 nG) do not lie in [0, n)");
    DAS_CHECK(!x || ylen >= n, DAS_ERR_ARG, who + ": y shorter than n");
    graph_check_csr(who, n, rowptr, col, n, false);
    DAS_CHECK(rowptr[n] == 0 || vals, DAS_ERR_ARG, who + ": null pointer");
    long long need = 0;
    for (long long g = 0; g < nG; g++) need += (rowptr[row0 + 3 * g + 1] - rowptr[row0 + 3 * g] + VP_CHUNK - 1) / VP_CHUNK;
    DAS_CHECK(dataCap >= need * VP_CHUNK_BYTES, DAS_ERR_ARG, who + ": data holds fewer bytes than the chunks of the group rows");
    DAS_GRAPH_DEVICE(who);
    debug_vecpack(n, rowptr, col, vals, row0, nG, built, cptr, data, nChunks, x, y, ylen);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_spmv_rows(long long nrows, const int* rows, long long n, const long long* rowptr, const int* col, const double* vals, const double* x, double* buf,
                        long long buflen) {
    DAS_TRY
    const std::string who = "das_debug_spmv_rows";
    graph_check_sizes(who, n);
    DAS_CHECK(nrows > 0, DAS_ERR_ARG, who + ": sizes must be positive");
    DAS_CHECK(rows && rowptr && x && buf, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(buflen >= nrows, DAS_ERR_ARG, who + ": buf shorter than nrows");
    graph_check_csr(who, n, rowptr, col, n, false);
    DAS_CHECK(rowptr[n] == 0 || vals, DAS_ERR_ARG, who + ": null pointer");
    for (long long k = 0; k < nrows; k++) DAS_CHECK(rows[k] >= 0 && rows[k] < n, DAS_ERR_ARG, who + ": row index out of range");
    DAS_GRAPH_DEVICE(who);
    debug_spmv_rows(nrows, rows, n, rowptr, col, vals, x, buf, buflen);
    return DAS_OK;
    DAS_CATCH
}
// Test-only entries (tests/test_gpu_color_kernels.py): the colouring kernels on a caller-made pattern and kept-row list; the device
// structures are derived with the helpers the solver uses (das_color_debug.hpp).  Everything is checked on the host before anything is
// launched.
static void color_check_input(const std::string& who, long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep) {
    graph_check_sizes(who, n);
    DAS_CHECK(rowptr && col && keep, DAS_ERR_ARG, who + ": null pointer");
    graph_check_csr(who, n, rowptr, col, n, true);
    DAS_CHECK(rowptr[n] > 0, DAS_ERR_ARG, who + ": a pattern without entries");
    DAS_CHECK(nKeep >= 1 && nKeep <= n, DAS_ERR_ARG, who + ": nKeep outside [1, n]");
    std::vector<unsigned char> seen((size_t)n, 0);
    for (long long q = 0; q < nKeep; q++) {
        DAS_CHECK(keep[q] >= 0 && keep[q] < n, DAS_ERR_ARG, who + ": kept row out of range");
        DAS_CHECK(!seen[keep[q]], DAS_ERR_ARG, who + ": kept row repeated");
        seen[keep[q]] = 1;
    }
}
static void color_check_width(const std::string& who, int W) {
    DAS_CHECK(W >= 1 && W <= SPEC_MAXW, DAS_ERR_ARG, who + ": W outside 1 .. 160 (the LDS of k_spec_conflict holds no more)");
}
static void color_check_colors(const std::string& who, long long n, const int* colors, int W) {
    DAS_CHECK(colors, DAS_ERR_ARG, who + ": null pointer");
    for (long long j = 0; j < n; j++) DAS_CHECK(colors[j] >= -1 && colors[j] < 64 * W, DAS_ERR_ARG, who + ": colour outside [-1, 64 W)");
}
int das_debug_color_firstfit(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, int* colors, long long colorsLen,
                             int* rc, int* W) {
    DAS_TRY
    const std::string who = "das_debug_color_firstfit";
    color_check_input(who, n, rowptr, col, nKeep, keep);
    DAS_CHECK(colors && rc && W, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(colorsLen >= n, DAS_ERR_ARG, who + ": colors shorter than n");
    DAS_GRAPH_DEVICE(who);
    debug_color_firstfit(n, rowptr, col, nKeep, keep, colors, rc, W);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_color_speculative(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, int spread, int* colors,
                                long long colorsLen, int* ok, int* rounds, int* S, int* W) {
    DAS_TRY
    const std::string who = "das_debug_color_speculative";
    color_check_input(who, n, rowptr, col, nKeep, keep);
    DAS_CHECK(colors && ok && rounds && S && W, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(colorsLen >= n, DAS_ERR_ARG, who + ": colors shorter than n");
    DAS_CHECK(spread == -1 || spread >= 1, DAS_ERR_ARG, who + ": the spread is -1 (the rule) or at least 1");
    DAS_CHECK(spread <= 32 * SPEC_MAXW, DAS_ERR_ARG, who + ": a spread whose first bitmaps exceed the LDS of k_spec_conflict");
    DAS_GRAPH_DEVICE(who);
    debug_color_speculative(n, rowptr, col, nKeep, keep, spread, colors, ok, rounds, S, W);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_color_spec_round(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, const int* colorsIn, int S, int W,
                               int round, int* tent, unsigned char* lose, int* colorsOut, long long outLen, unsigned long long* F, long long FLen,
                               unsigned* left, int* overflow) {
    DAS_TRY
    const std::string who = "das_debug_color_spec_round";
    color_check_input(who, n, rowptr, col, nKeep, keep);
    color_check_width(who, W);
    DAS_CHECK(S >= 1, DAS_ERR_ARG, who + ": S must be at least 1");
    DAS_CHECK(round >= 0, DAS_ERR_ARG, who + ": negative round");
    color_check_colors(who, n, colorsIn, W);
    DAS_CHECK(tent && lose && colorsOut && F && left && overflow, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(outLen >= n, DAS_ERR_ARG, who + ": tent / lose / colorsOut shorter than n");
    DAS_CHECK(FLen >= nKeep * W, DAS_ERR_ARG, who + ": F shorter than nKeep W");
    DAS_GRAPH_DEVICE(who);
    debug_color_spec_round(n, rowptr, col, nKeep, keep, colorsIn, S, W, round, tent, lose, colorsOut, F, left, overflow);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_color_check(long long n, const long long* rowptr, const int* col, long long nKeep, const long long* keep, const int* colors, int W, int* invalid) {
    DAS_TRY
    const std::string who = "das_debug_color_check";
    color_check_input(who, n, rowptr, col, nKeep, keep);
    color_check_width(who, W);
    color_check_colors(who, n, colors, W);
    DAS_CHECK(invalid, DAS_ERR_ARG, who + ": null pointer");
    DAS_GRAPH_DEVICE(who);
    debug_color_check(n, rowptr, col, nKeep, keep, colors, W, invalid);
    return DAS_OK;
    DAS_CATCH
}
// Test-only entries (tests/test_gpu_reduce_kernels.py): the reductions of the objective functions and the two gathers on caller-made
// arrays through the launch helpers the solver uses (das_reduce_debug.hpp).  Everything is checked on the host before anything is launched.
#define DAS_REDUCE_MAX_N (1LL << 31)
int das_debug_reduce_ks(long long n, double* a, double k, double outer, double* ms, long long msLen, double* pmax, double* psum, long long partLen, double* w,
                        long long wLen, int* nb) {
    DAS_TRY
    const std::string who = "das_debug_reduce_ks";
    DAS_CHECK(n >= 1 && n < DAS_REDUCE_MAX_N, DAS_ERR_ARG, who + ": n outside [1, 2^31) (an empty set has no KS aggregate)");
    DAS_CHECK(a && ms && pmax && psum && w && nb, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(msLen >= 2 && partLen >= DAS_FACEFN_MAX_BLOCKS && wLen >= n, DAS_ERR_ARG, who + ": ms shorter than 2, a partial array shorter than 1024 or w shorter than n");
    DAS_GRAPH_DEVICE(who);
    debug_reduce_ks(n, a, k, outer, ms, msLen, pmax, psum, partLen, w, wLen, nb);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reduce_group_sum(long long cnt, unsigned char* group, double* fv, double* out2, long long outLen) {
    DAS_TRY
    const std::string who = "das_debug_reduce_group_sum";
    DAS_CHECK(cnt >= 0 && cnt < DAS_REDUCE_MAX_N, DAS_ERR_ARG, who + ": cnt outside [0, 2^31)");
    DAS_CHECK(fv && out2, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(outLen >= 2, DAS_ERR_ARG, who + ": out2 shorter than 2");
    DAS_GRAPH_DEVICE(who);
    debug_reduce_group_sum(cnt, group, fv, out2, outLen);
    return DAS_OK;
    DAS_CATCH
}
static void reduce_check_dot(const std::string& who, long long n, long long nMin, const void* a, const void* b, const void* part, long long partLen, long long partMin,
                             const void* out, long long outLen, long long outMin, const int* nb) {
    DAS_CHECK(n >= nMin && n < DAS_REDUCE_MAX_N, DAS_ERR_ARG, who + ": n out of range");
    DAS_CHECK(a && b && part && out && nb, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(partLen >= partMin && outLen >= outMin, DAS_ERR_ARG, who + ": the partial array or the output is too short");
}
int das_debug_reduce_tangent_dot(long long n, double* R, double* psi, double* part, long long partLen, double* out2, long long outLen, int* nb) {
    DAS_TRY
    const std::string who = "das_debug_reduce_tangent_dot";
    reduce_check_dot(who, n, 0, R, psi, part, partLen, DAS_TANGENT_DOT_BLOCKS, out2, outLen, 2, nb);
    DAS_GRAPH_DEVICE(who);
    debug_reduce_dual_dot(0, n, R, psi, part, partLen, out2, outLen, nb);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reduce_ad_dot(long long n, double* R, double* psi, double* part, long long partLen, double* out, long long outLen, int* nb) {
    DAS_TRY
    const std::string who = "das_debug_reduce_ad_dot";
    reduce_check_dot(who, n, 1, R, psi, part, partLen, DAS_HS_MAX_BLOCKS, out, outLen, 1, nb);
    DAS_GRAPH_DEVICE(who);
    debug_reduce_dual_dot(1, n, R, psi, part, partLen, out, outLen, nb);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reduce_sv_dot(long long n, double* a, double* b, double* part, long long partLen, double* out2, long long outLen, int* nb) {
    DAS_TRY
    const std::string who = "das_debug_reduce_sv_dot";
    reduce_check_dot(who, n, 1, a, b, part, partLen, DAS_SV_DOT_MAX_BLOCKS, out2, outLen, 2, nb);
    DAS_GRAPH_DEVICE(who);
    debug_reduce_sv_dot(n, a, b, part, partLen, out2, outLen, nb);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reduce_cellfn(long long nt, int* cell, long long* idx, double* data, int square, int mv, long long nCells, const double* V, long long nSrc, double* src,
                            double coef, double* part, long long partLen, double* out, long long outLen, double* sc, double g, double* grad, long long gradLen, int* nb) {
    DAS_TRY
    const std::string who = "das_debug_reduce_cellfn";
    DAS_CHECK(nt >= 1 && nt < DAS_REDUCE_MAX_N && nCells >= 1 && nCells < DAS_REDUCE_MAX_N && nSrc >= 1 && nSrc < DAS_REDUCE_MAX_N, DAS_ERR_ARG, who + ": sizes outside [1, 2^31)");
    DAS_CHECK(cell && idx && V && src && part && out && grad && nb, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(partLen >= DAS_CELLFN_MAX_BLOCKS && outLen >= 1 && gradLen >= nSrc, DAS_ERR_ARG, who + ": part shorter than 1024, out empty or grad shorter than nSrc");
    std::vector<unsigned char> seen((size_t)nSrc, 0);
    for (long long t = 0; t < nt; t++) {
        DAS_CHECK(cell[t] >= 0 && cell[t] < nCells, DAS_ERR_ARG, who + ": cell out of range");
        DAS_CHECK(idx[t] >= 0 && idx[t] < nSrc, DAS_ERR_ARG, who + ": idx out of range");
        DAS_CHECK(!seen[idx[t]], DAS_ERR_ARG, who + ": idx repeated (the terms of a function address distinct entries)");
        seen[idx[t]] = 1;
    }
    DAS_GRAPH_DEVICE(who);
    debug_reduce_cellfn(nt, cell, idx, data, square, mv, nCells, V, nSrc, src, coef, part, partLen, out, outLen, sc, g, grad, gradLen, nb);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reduce_rn(long long n, int nblocks, const long long* off, const int* kind, const double* w, long long nC, long long nF, long long nIF, int l1, double* R,
                        double* term, long long termLen, double* part, long long partLen, double* ms, long long msLen, double F, double coef, double* g, long long gLen,
                        int* nb) {
    DAS_TRY
    const std::string who = "das_debug_reduce_rn";
    DAS_CHECK(n >= 1 && n < DAS_REDUCE_MAX_N, DAS_ERR_ARG, who + ": n outside [1, 2^31)");
    DAS_CHECK(nblocks >= 0 && nblocks <= 8, DAS_ERR_ARG, who + ": 0 to 8 residual blocks");
    DAS_CHECK(off && kind && w && R && term && part && ms && g && nb, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(nC >= 0 && nF >= 0 && nIF >= 0 && nIF <= nF && nC < DAS_REDUCE_MAX_N && nF < DAS_REDUCE_MAX_N, DAS_ERR_ARG, who + ": bad nC / nF / nIF");
    DAS_CHECK(termLen >= n && gLen >= n && partLen >= DAS_FACEFN_MAX_BLOCKS && msLen >= 2, DAS_ERR_ARG, who + ": an output array is too short");
    DAS_CHECK(l1 || F != 0.0, DAS_ERR_ARG, who + ": the L2Norm seeds divide by F");
    RnRows r{};
    r.nb = nblocks;
    for (int b = 0; b < nblocks; b++) {
        DAS_CHECK(kind[b] == KIND_VEC || kind[b] == KIND_SCL || kind[b] == KIND_FACE, DAS_ERR_ARG, who + ": kind is 0 (vector), 1 (scalar) or 2 (face)");
        r.off[b] = off[b]; r.kind[b] = kind[b]; r.w[b] = w[b];
    }
    r.nC = nC; r.nF = nF; r.nIF = nIF;
    r.l1 = l1 ? 1 : 0;
    DAS_GRAPH_DEVICE(who);
    debug_reduce_rn(n, r, R, term, termLen, part, partLen, ms, msLen, F, coef, g, gLen, nb);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reduce_hs_sum(int kind, int nC, const double* V, unsigned char* member, double* field, double* psi, int byV, double power, double* vt, double* part,
                            long long partLen, double* out, long long outLen, int* nb) {
    DAS_TRY
    const std::string who = "das_debug_reduce_hs_sum";
    DAS_CHECK(kind == DAS_HS_FIELD || kind == DAS_HS_CYLINDERTOCELL, DAS_ERR_ARG, who + ": kind is 0 (cylinderToCell) or 2 (field): the kinds that read volumes only");
    DAS_CHECK(nC >= 1, DAS_ERR_ARG, who + ": nC must be positive");
    DAS_CHECK(V && part && out && nb && (kind == DAS_HS_FIELD ? field != nullptr : member != nullptr), DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(!vt || psi, DAS_ERR_ARG, who + ": vt is read only with psi");
    DAS_CHECK(partLen >= DAS_HS_MAX_BLOCKS && outLen >= 1, DAS_ERR_ARG, who + ": part shorter than 1024 or out empty");
    DAS_GRAPH_DEVICE(who);
    debug_reduce_hs_sum(kind, nC, V, member, field, psi, byV, power, vt, part, partLen, out, outLen, nb);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reduce_final(int pair, int dual, int nb, double* part, long long partLen, double* out, long long outLen) {
    DAS_TRY
    const std::string who = "das_debug_reduce_final";
    DAS_CHECK(nb >= 1 && nb <= DAS_HS_MAX_BLOCKS, DAS_ERR_ARG, who + ": nb outside 1 .. 1024");
    DAS_CHECK(part && out, DAS_ERR_ARG, who + ": null pointer");
    const long long per = (dual ? 2 : 1), cnt = (pair ? 2 : 1);
    DAS_CHECK(partLen >= cnt * per * nb && outLen >= cnt * per && partLen % per == 0 && outLen % per == 0, DAS_ERR_ARG, who + ": part or out too short (or an odd count of dual halves)");
    DAS_GRAPH_DEVICE(who);
    if (dual) debug_reduce_final<Dual<1>>(pair, nb, part, partLen, out, outLen);
    else debug_reduce_final<double>(pair, nb, part, partLen, out, outLen);
    return DAS_OK;
    DAS_CATCH
}
static void reduce_check_cell_faces(const std::string& who, int nC, const int* cf_ptr, const int* cf_face) {
    DAS_CHECK(nC >= 1, DAS_ERR_ARG, who + ": nC must be positive");
    DAS_CHECK(cf_ptr && cf_face, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(cf_ptr[0] == 0, DAS_ERR_ARG, who + ": cf_ptr[0] != 0");
    for (int c = 0; c < nC; c++) DAS_CHECK(cf_ptr[c + 1] >= cf_ptr[c], DAS_ERR_ARG, who + ": decreasing cf_ptr");
}
int das_debug_reduce_owner_gather(int nC, int* cf_ptr, int* cf_face, long long nFt, double* ft, double* tc, long long tcLen) {
    DAS_TRY
    const std::string who = "das_debug_reduce_owner_gather";
    reduce_check_cell_faces(who, nC, cf_ptr, cf_face);
    DAS_CHECK(ft && tc && nFt >= 1 && tcLen >= nC, DAS_ERR_ARG, who + ": null pointer, no face values or tc shorter than nC");
    for (int s = 0; s < cf_ptr[nC]; s++) DAS_CHECK(cf_face[s] < nFt, DAS_ERR_ARG, who + ": face out of range");
    DAS_GRAPH_DEVICE(who);
    debug_reduce_owner_gather(nC, cf_ptr, cf_face, nFt, ft, tc, tcLen);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_reduce_vm_gather(int nC, int nIF, int* cf_ptr, int* cf_face, int* cf_other, int* colors, int col, double* tc, double seed, double* out, long long outLen) {
    DAS_TRY
    const std::string who = "das_debug_reduce_vm_gather";
    reduce_check_cell_faces(who, nC, cf_ptr, cf_face);
    DAS_CHECK(cf_other && colors && tc && out, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(nIF >= 0 && outLen >= 3LL * nC, DAS_ERR_ARG, who + ": negative nIF or out shorter than 3 nC");
    for (int s = 0; s < cf_ptr[nC]; s++)
        if ((cf_face[s] & 0x7fffffff) < nIF) DAS_CHECK(cf_other[s] >= 0 && cf_other[s] < nC, DAS_ERR_ARG, who + ": neighbour of an internal face out of range");
    DAS_GRAPH_DEVICE(who);
    debug_reduce_vm_gather(nC, nIF, cf_ptr, cf_face, cf_other, colors, col, tc, seed, out, outLen);
    return DAS_OK;
    DAS_CATCH
}
// Test-only entries (tests/test_gpu_coarse_kernels.py): the coarse space of the two-level preconditioner on caller-made structures
// through the helpers the solver uses (das_coarse.hpp, das_coarse_debug.hpp).  Everything a kernel would index with is checked on the
// host before anything is launched.
int das_debug_coarse_assemble(int nagg, long long N, long long off, long long n, const long long* rowptr, const int* col, const double* vals, const int* aggRow,
                              const int* aggCol, int transpose, double diagScale, double* E) {
    DAS_TRY
    const std::string who = "das_debug_coarse_assemble";
    coarse_check_nagg(who, nagg);
    coarse_check_field(who, N, off, n);
    DAS_CHECK(rowptr && aggRow && aggCol && E, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(transpose == 0 || transpose == 1, DAS_ERR_ARG, who + ": transpose is 0 or 1");
    graph_check_csr(who, n, rowptr, col, n, false);
    DAS_CHECK(rowptr[n] == 0 || vals, DAS_ERR_ARG, who + ": null pointer");
    coarse_check_agg(who, N, nagg, aggRow);
    coarse_check_agg(who, N, nagg, aggCol);
    DAS_GRAPH_DEVICE(who);
    debug_coarse_assemble(nagg, N, off, n, rowptr, col, vals, aggRow, aggCol, transpose, diagScale, E);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_coarse_invert(int n, const double* Ein, double* Inv, int* singular) {
    DAS_TRY
    const std::string who = "das_debug_coarse_invert";
    DAS_CHECK(n >= 1 && n <= COARSE_MAX_AGG, DAS_ERR_ARG, who + ": n outside 1 .. 2048");
    DAS_CHECK(Ein && Inv && singular, DAS_ERR_ARG, who + ": null pointer");
    DAS_GRAPH_DEVICE(who);
    debug_coarse_invert(n, Ein, Inv, singular);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_coarse_correct(int nagg, long long N, long long off, long long n, const int* agg, const double* Einv, const double* r, double* t, double* u, double* y,
                             long long ylen, int set) {
    DAS_TRY
    const std::string who = "das_debug_coarse_correct";
    coarse_check_nagg(who, nagg);
    coarse_check_field(who, N, off, n);
    DAS_CHECK(Einv && r && t && u && y, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(ylen >= n && ylen < (1LL << 31), DAS_ERR_ARG, who + ": y shorter than n");
    DAS_CHECK(set == 0 || set == 1, DAS_ERR_ARG, who + ": set is 0 or 1");
    coarse_check_agg(who, N, nagg, agg);
    DAS_GRAPH_DEVICE(who);
    debug_coarse_correct(nagg, N, off, n, agg, Einv, r, t, u, y, ylen, set);
    return DAS_OK;
    DAS_CATCH
}
int das_debug_coarse_az(int nagg, long long n, const long long* rowptr, const int* col, const double* vals, long long N, long long off, const int* agg, int* cnt,
                        long long* ptr, int* oa, double* ov, long long cap, long long* nnz, int* overflow, const double* u, const double* v, double* out,
                        long long outlen) {
    DAS_TRY
    const std::string who = "das_debug_coarse_az";
    coarse_check_nagg(who, nagg);
    coarse_check_field(who, N, off, n);
    DAS_CHECK(rowptr && cnt && ptr && oa && ov && nnz && overflow && u && out, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(outlen >= n && outlen < (1LL << 31), DAS_ERR_ARG, who + ": out shorter than n");
    graph_check_csr(who, n, rowptr, col, n, false);
    DAS_CHECK(rowptr[n] == 0 || vals, DAS_ERR_ARG, who + ": null pointer");
    coarse_check_agg(who, N, nagg, agg);
    bool over = false;
    const long long need = coarse_az_count(n, rowptr, col, N, off, agg, over);
    DAS_CHECK(cap >= 1 && cap < (1LL << 31) && (over || cap >= need), DAS_ERR_ARG, who + ": oa / ov hold fewer than the entries of the sparse A Z");
    DAS_GRAPH_DEVICE(who);
    debug_coarse_az(nagg, n, rowptr, col, vals, N, off, agg, cnt, ptr, oa, ov, cap, nnz, overflow, u, v, out, outlen);
    return DAS_OK;
    DAS_CATCH
}
#undef DAS_GRAPH_DEVICE

double das_get_elapsed_clock_time(das_solver_t* s) { return s ? wall_seconds() - s->t0_wall : -1.0; }
double das_get_elapsed_cpu_time(das_solver_t* s) { return s ? (double)(std::clock() - s->t0_cpu) / CLOCKS_PER_SEC : -1.0; }
double das_timer_avg_ms(das_solver_t* s, const char* name) {
    try {
        if (!s || !name) return -1.0;
        s->timer.resolve();
        auto it = s->timer.recs.find(name);
        if (it == s->timer.recs.end() || it->second.cnt == 0) return -1.0;
        return it->second.ms / it->second.cnt;
    } catch (const std::exception& e) { fail(e); return -1.0; }
}
long long das_timer_count(das_solver_t* s, const char* name) {
    try {
        if (!s || !name) return -1;
        s->timer.resolve();
        auto it = s->timer.recs.find(name);
        return it == s->timer.recs.end() ? 0 : it->second.cnt;
    } catch (const std::exception& e) { fail(e); return -1; }
}
void das_timer_reset(das_solver_t* s) { if (s) { try { s->timer.reset(); } catch (...) {} } }
void das_timer_enable(das_solver_t* s, int on) { if (s) s->timer.on = on != 0; }

}  // extern "C"

// Bodies of the test-only entries das_debug_color_* (tests/test_gpu_color_kernels.py): the colouring kernels of das_color.hpp -
// k_color_firstfit, k_spec_assign, k_spec_conflict, k_spec_commit, k_spec_netbits - on a caller-made pattern and kept-row list: no
// mesh, no solver handle.  The caller hands over the row-major pattern and the kept rows only; the structures the kernels index with
// (column -> nets with positions, groups, net -> columns) are DERIVED with the helpers the solver runs - device_transpose,
// device_build_nets, color_groups_from_flags, k_rows_gather - so that the waiting kernel can never be given a cpos that disagrees with
// its nets.  Everything is CHECKED ON THE HOST first (DAS_ERR_ARG before the first device call); everything runs on the null stream.
// Nothing in the product path calls them.
#pragma once
#include "das_color.hpp"
#include "das_graph_debug.hpp"

namespace das {

struct ColorDebugGraph {
    DevPattern P;
    DevBuf<long long> trp, cptr, krp, keep;
    DevBuf<int> tcol, net, crow, cpos, kcol;
    DevBuf<unsigned char> start;
    std::vector<long long> gstart;
    long long maxNet = 0;
};
// as the graph path of ensure_coloring derives them (das_device.hip)
static void color_debug_graph(long long n, const long long* rp, const int* ci, long long nKeep, const long long* keep, ColorDebugGraph& G) {
    debug_graph_transposed(n, rp, ci, G.P, G.trp, G.tcol);
    std::vector<int> netOfRow((size_t)n, -1);
    for (long long q = 0; q < nKeep; q++) netOfRow[keep[q]] = (int)q;
    G.net.upload(netOfRow);
    device_build_nets(n, G.trp.p, G.tcol.p, G.net.p, G.P.rowptr.p, G.P.col.p, G.cptr, G.crow, G.cpos, G.start, 0);
    krylov_debug_sync();
    G.gstart = color_groups_from_flags(n, G.start.to_host());
    std::vector<long long> krp((size_t)nKeep + 1, 0);
    for (long long q = 0; q < nKeep; q++) {
        const long long len = rp[keep[q] + 1] - rp[keep[q]];
        krp[q + 1] = krp[q] + len;
        G.maxNet = std::max(G.maxNet, len);
    }
    G.krp.upload(krp);
    G.keep.upload(keep, (size_t)nKeep);
    G.kcol.alloc((size_t)std::max<long long>(1, krp[nKeep]));
    hipLaunchKernelGGL(k_rows_gather, dim3((unsigned)((nKeep + 3) / 4)), dim3(256), 0, 0, nKeep, G.keep.p, G.P.rowptr.p, G.P.col.p, G.krp.p, G.kcol.p);
    krylov_debug_sync();
}
static void debug_color_firstfit(long long n, const long long* rp, const int* ci, long long nKeep, const long long* keep, int* colors, int* rc, int* W) {
    ColorDebugGraph G;
    color_debug_graph(n, rp, ci, nKeep, keep, G);
    std::vector<int> c;
    int w = 0;
    *rc = color_firstfit_run(n, nKeep, G.gstart, G.cptr.p, G.crow.p, G.cpos.p, c, 0, &w);
    *W = w;
    if (*rc == 1) std::copy(c.begin(), c.end(), colors);
}
static void debug_color_speculative(long long n, const long long* rp, const int* ci, long long nKeep, const long long* keep, int spread, int* colors, int* ok,
                                    int* rounds, int* S, int* W) {
    ColorDebugGraph G;
    color_debug_graph(n, rp, ci, nKeep, keep, G);
    std::vector<int> c;
    int r = 0, s = 0, w = 0;
    *ok = color_speculative_run(n, nKeep, G.maxNet, G.cptr.p, G.crow.p, G.krp.p, G.kcol.p, c, 0, &r, spread, &s, &w) ? 1 : 0;
    *rounds = r; *S = s; *W = w;
    if (*ok) std::copy(c.begin(), c.end(), colors);
}
// the buffers of a SpecView around caller-given final colours
struct ColorDebugSpec {
    DevBuf<int> colors, tent;
    DevBuf<unsigned char> lose;
    DevBuf<unsigned> ctrl;
    DevBuf<unsigned long long> F;
    SpecView V;
    unsigned gNet;
    ColorDebugSpec(const ColorDebugGraph& G, long long n, long long nKeep, const int* colorsIn, int W, const std::string& who)
        : colors(krylov_up<int>(colorsIn, (size_t)n)), tent((size_t)n), lose((size_t)n), ctrl(4), F((size_t)nKeep * W) {
        DAS_CHECK(spec_conflict_prepare(W), DAS_ERR_ARG, who + ": W above what the LDS of k_spec_conflict holds on this device");
        DAS_HIP(hipMemset(tent.p, 0xff, (size_t)n * sizeof(int)));
        lose.zero(); ctrl.zero(); F.zero();
        V = SpecView{n, nKeep, G.cptr.p, G.crow.p, G.krp.p, G.kcol.p, W, F.p, colors.p, tent.p, lose.p, ctrl.p};
        gNet = (unsigned)((nKeep + 3) / 4);
    }
};
static void debug_color_spec_round(long long n, const long long* rp, const int* ci, long long nKeep, const long long* keep, const int* colorsIn, int S, int W,
                                   int round, int* tent, unsigned char* lose, int* colorsOut, unsigned long long* F, unsigned* left, int* overflow) {
    ColorDebugGraph G;
    color_debug_graph(n, rp, ci, nKeep, keep, G);
    ColorDebugSpec D(G, n, nKeep, colorsIn, W, "das_debug_color_spec_round");
    const size_t ldsBits = (size_t)4 * W * sizeof(unsigned long long);
    hipLaunchKernelGGL(k_spec_netbits, dim3(D.gNet), dim3(256), ldsBits, 0, D.V);
    hipLaunchKernelGGL(k_spec_assign, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, 0, D.V, S, (unsigned)round);
    krylov_debug_sync();
    D.tent.download(tent, (size_t)n);
    hipLaunchKernelGGL(k_spec_conflict, dim3(D.gNet), dim3(256), spec_conflict_lds(W), 0, D.V, 0);
    krylov_debug_sync();
    D.lose.download(lose, (size_t)n);
    hipLaunchKernelGGL(k_spec_commit, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, D.V);
    krylov_debug_sync();
    D.colors.download(colorsOut, (size_t)n);
    hipLaunchKernelGGL(k_spec_netbits, dim3(D.gNet), dim3(256), ldsBits, 0, D.V);
    krylov_debug_sync();
    D.F.download(F, (size_t)nKeep * W);
    unsigned ctrl[4] = {0, 0, 0, 0};
    D.ctrl.download(ctrl, 4);
    *left = ctrl[0];
    *overflow = ctrl[1] ? 1 : 0;
}
static void debug_color_check(long long n, const long long* rp, const int* ci, long long nKeep, const long long* keep, const int* colorsIn, int W, int* invalid) {
    ColorDebugGraph G;
    color_debug_graph(n, rp, ci, nKeep, keep, G);
    ColorDebugSpec D(G, n, nKeep, colorsIn, W, "das_debug_color_check");
    hipLaunchKernelGGL(k_spec_conflict, dim3(D.gNet), dim3(256), spec_conflict_lds(W), 0, D.V, 1);
    krylov_debug_sync();
    unsigned ctrl[4] = {0, 0, 0, 0};
    D.ctrl.download(ctrl, 4);
    *invalid = ctrl[2] ? 1 : 0;
}

}  // namespace das

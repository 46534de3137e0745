// Bodies of the test-only entries das_debug_krylov_* (tests/test_gpu_krylov_kernels.py) and the timing helper of the tuning
// entries das_debug_orth_bench*.  The bodies upload the caller's arrays, run the launch helpers the solver runs (null stream) and
// download the result.  Nothing in the product path calls them.  Basis formats: 0 = fp64, 1 = fp32, 2 = split (float hi, the lo
// array n floats further inside a slot).
#pragma once
#include "das_krylov.hpp"
#include "das_block.hpp"

namespace das {

enum { KRY_FP64 = 0, KRY_FP32 = 1, KRY_SPLIT = 2 };
static void krylov_check_basis(const std::string& who, long long n, long long nvec, int fmt, const void* V, long long ld) {
    DAS_CHECK(n > 0 && nvec > 0, DAS_ERR_ARG, who + ": sizes must be positive");
    DAS_CHECK(fmt == KRY_FP64 || fmt == KRY_FP32 || fmt == KRY_SPLIT, DAS_ERR_ARG, who + ": fmt is 0 (fp64), 1 (fp32) or 2 (split)");
    DAS_CHECK(V, DAS_ERR_ARG, who + ": null basis");
    DAS_CHECK(ld >= (fmt == KRY_SPLIT ? 2 * n : n), DAS_ERR_ARG, who + ": leading dimension below n (split: below 2 n)");
}
static void krylov_check_block(const std::string& who, long long n, int K, int sv) {
    DAS_CHECK(n > 0 && K > 0, DAS_ERR_ARG, who + ": sizes must be positive");
    DAS_CHECK(sv >= 1 && sv <= 8, DAS_ERR_ARG, who + ": 1 to 8 right-hand sides");
}
static void krylov_debug_sync() {
    DAS_HIP(hipGetLastError());
    DAS_HIP(hipStreamSynchronize(0));
}
template <class VT>
static float* krylov_lo(VT* V, long long n, bool split) { return split ? reinterpret_cast<float*>(V) + n : nullptr; }
// the first cnt entries of a host array on the device (never a null device pointer: an empty array gets one entry)
template <class T>
static DevBuf<T> krylov_up(const void* h, size_t cnt) {
    DevBuf<T> d(std::max<size_t>(cnt, 1));
    d.upload((const T*)h, cnt);
    return d;
}
// run the launch, wait for it, and copy the first cnt entries of res back to the host array
template <class T, class F>
static void krylov_run(F&& launch, const DevBuf<T>& res, void* h, size_t cnt) {
    launch();
    krylov_debug_sync();
    res.download((T*)h, cnt);
}

template <class VT>
static void debug_krylov_dots2(long long n, int K, const void* V, long long ld, const double* v, double* out) {
    const DevBuf<VT> dV = krylov_up<VT>(V, (size_t)K * ld);
    const DevBuf<double> dv = krylov_up<double>(v, n), partial(multidot2_partial_size(n, K)), dout((size_t)2 * K);
    krylov_run([&] { launch_multidot2<VT>(0, n, K, dV.p, ld, dV.p + (long long)(K - 1) * ld, dv.p, partial.p, dout.p); }, dout, out, (size_t)2 * K);
}
template <class VT>
static void debug_krylov_dcgs2_update(long long n, int j, bool split, void* V, long long ld, int nslots, const double* sc, double gamma, double ralpha,
                                      const double* v) {
    const DevBuf<VT> dV = krylov_up<VT>(V, (size_t)nslots * ld);
    const DevBuf<double> dsc = krylov_up<double>(sc, (size_t)2 * j), dv = krylov_up<double>(v, n);
    krylov_run([&] { launch_dcgs2_update<DCGS2_UNROLL, DCGS2_RPT, VT>(0, n, j, dV.p, ld, dsc.p, gamma, ralpha, dv.p, krylov_lo(dV.p, n, split)); }, dV, V,
               (size_t)nslots * ld);
}
template <class VT>
static void debug_krylov_multidot(long long n, int m, const void* V, long long ld, const double* w, double* out) {
    const DevBuf<VT> dV = krylov_up<VT>(V, (size_t)m * ld);
    const DevBuf<double> dw = krylov_up<double>(w, n), partial(multidot_partial_size(n, m)), dout((size_t)m + 1);
    krylov_run([&] { launch_multidot<VT>(0, n, m, dV.p, ld, dw.p, partial.p, dout.p); }, dout, out, (size_t)m + 1);
}
template <class VT, class WT>
static void debug_krylov_multiaxpy(long long n, int m, bool split, const void* V, long long ld, const double* h, void* w, long long wlen) {
    const DevBuf<VT> dV = krylov_up<VT>(V, (size_t)m * ld);
    const DevBuf<double> dh = krylov_up<double>(h, m);
    const DevBuf<WT> dw = krylov_up<WT>(w, (size_t)wlen);
    krylov_run([&] { launch_multiaxpy<VT, WT>(0, n, m, dV.p, ld, dh.p, dw.p, krylov_lo(dV.p, n, split)); }, dw, w, (size_t)wlen);
}
template <class VT>
static void debug_krylov_lincomb(long long n, int m, bool split, const void* V, long long ld, const double* c, double* y, long long ylen) {
    const DevBuf<VT> dV = krylov_up<VT>(V, (size_t)m * ld);
    const DevBuf<double> dc = krylov_up<double>(c, m), dy = krylov_up<double>(y, (size_t)ylen);
    krylov_run([&] { launch_lincomb<VT>(0, n, m, dV.p, ld, dc.p, dy.p, krylov_lo(dV.p, n, split)); }, dy, y, (size_t)ylen);
}
// xsplit / ysplit: the lo array sits n floats after the hi array, as in a basis slot
template <class TI, class TO>
static void debug_krylov_scale_to(long long n, double a, bool xsplit, bool ysplit, const void* x, void* y, long long ylen) {
    const DevBuf<TI> dx = krylov_up<TI>(x, (size_t)(xsplit ? 2 * n : n));
    const DevBuf<TO> dy = krylov_up<TO>(y, (size_t)ylen);
    krylov_run([&] { launch_scale_to<TI, TO>(0, n, a, dx.p, dy.p, krylov_lo(dx.p, n, xsplit), krylov_lo(dy.p, n, ysplit)); }, dy, y, (size_t)ylen);
}
static void debug_krylov_block_tn(long long n, int K, int s, const double* V, long long ldv, long long voff, const double* W, long long ldw, double* C) {
    const DevBuf<double> dV = krylov_up<double>(V, (size_t)(voff + (long long)K * ldv)), dW = krylov_up<double>(W, (size_t)s * ldw);
    const DevBuf<double> partial(tsgemm_partial_size(K)), dC((size_t)K * s);
    krylov_run([&] { launch_tsgemm_tn(0, n, K, s, dV.p + voff, ldv, dW.p, ldw, partial.p, dC.p); }, dC, C, (size_t)K * s);
}
static void debug_krylov_block_nn_sub(long long n, int K, int s, const double* V, long long ldv, const double* C, double* W, long long ldw) {
    const DevBuf<double> dV = krylov_up<double>(V, (size_t)K * ldv), dW = krylov_up<double>(W, (size_t)s * ldw), dC = krylov_up<double>(C, (size_t)K * s);
    krylov_run([&] { launch_tsgemm_nn_sub(0, n, K, s, dV.p, ldv, dC.p, dW.p, ldw); }, dW, W, (size_t)s * ldw);
}
static void debug_krylov_block_right_mult(long long n, int s, double* W, long long ldw, const double* T) {
    const DevBuf<double> dW = krylov_up<double>(W, (size_t)s * ldw), dT = krylov_up<double>(T, (size_t)s * s);
    krylov_run([&] { launch_block_right_mult(0, n, s, dW.p, ldw, dT.p); }, dW, W, (size_t)s * ldw);
}
static void debug_krylov_block_lincomb(long long n, int K, int s, const double* V, long long ldv, const double* C, double* Y, long long ldy) {
    const DevBuf<double> dV = krylov_up<double>(V, (size_t)K * ldv), dC = krylov_up<double>(C, (size_t)K * s), dY = krylov_up<double>(Y, (size_t)s * ldy);
    krylov_run([&] { launch_block_lincomb(0, n, K, s, dV.p, ldv, dC.p, dY.p, ldy); }, dY, Y, (size_t)s * ldy);
}
static void debug_krylov_block_spmm(long long n, int s, const long long* rp, const int* ci, const double* val, const double* X, long long ldx, double* Y,
                                    long long ldy) {
    const size_t nnz = (size_t)rp[n];
    const DevBuf<long long> drp = krylov_up<long long>(rp, (size_t)n + 1);
    const DevBuf<int> dci = krylov_up<int>(ci, nnz);
    const DevBuf<double> dval = krylov_up<double>(val, nnz), dX = krylov_up<double>(X, (size_t)s * ldx), dY = krylov_up<double>(Y, (size_t)s * ldy);
    const DevBuf<double> dXr((size_t)n * spmm_width(s));
    krylov_run([&] {
        launch_block_to_rows(0, n, s, dX.p, ldx, dXr.p);
        launch_spmm_wave(0, n, s, drp.p, dci.p, dval.p, dXr.p, dY.p, ldy);
    }, dY, Y, (size_t)s * ldy);
}

// ---- timing of the tuning entries das_debug_orth_bench* (tools/orth_bench.py) ---------------------------------------------
struct BenchEvent {
    hipEvent_t e = nullptr;
    BenchEvent() { DAS_HIP(hipEventCreate(&e)); }
    ~BenchEvent() { (void)hipEventDestroy(e); }
    BenchEvent(const BenchEvent&) = delete;
    BenchEvent& operator=(const BenchEvent&) = delete;
};
// milliseconds per launch on the null stream: one warm-up launch, then reps timed ones (the events go on the error path too)
template <class F>
static double orth_bench_ms(int reps, F&& launch) {
    BenchEvent e0, e1;
    launch();  // warm-up
    DAS_HIP(hipEventRecord(e0.e, 0));
    for (int r = 0; r < reps; r++) launch();
    DAS_HIP(hipEventRecord(e1.e, 0));
    DAS_HIP(hipEventSynchronize(e1.e));
    DAS_HIP(hipGetLastError());
    float ms = 0.f;
    DAS_HIP(hipEventElapsedTime(&ms, e0.e, e1.e));
    return (double)ms / reps;
}

}  // namespace das

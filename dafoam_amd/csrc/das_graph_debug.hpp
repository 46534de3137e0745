// Bodies of the test-only entries das_debug_graph_*, das_debug_compact, das_debug_vecpack and das_debug_spmv_rows
// (tests/test_gpu_graph_kernels.py, tests/test_gpu_opmat_kernels.py): the graph set-up of das_graph.hpp, the jacLowerBounds filter and
// the packed operator of das_opmat.hpp and the ghost-row product of das_comm.hpp on caller-made structures - no mesh, no solver handle.
// These kernels index with what they are given, so everything is CHECKED ON THE HOST first (graph_check_*: DAS_ERR_ARG before the first
// device call); then the helpers the solver runs are run on the null stream: device_exclusive_scan, device_transpose, device_build_nets,
// filter_compact, vecpack_build, launch_spmv.  Nothing in the product path calls them.
#pragma once
#include "das_comm.hpp"
#include "das_graph.hpp"
#include "das_krylov_debug.hpp"
#include "das_opmat.hpp"

namespace das {

static void graph_check_sizes(const std::string& who, long long n) {
    DAS_CHECK(n > 0, DAS_ERR_ARG, who + ": sizes must be positive");
    DAS_CHECK(n < (1LL << 31), DAS_ERR_ARG, who + ": n must be below 2^31");
}
// a CSR structure of n rows with columns in [0, ncols): rowptr[0] = 0, rowptr monotone, fewer than 2^31 entries, columns in range and,
// if asked for, strictly ascending inside a row
static void graph_check_csr(const std::string& who, long long n, const long long* rp, const int* ci, long long ncols, bool ascending) {
    DAS_CHECK(rp, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(rp[0] == 0, DAS_ERR_ARG, who + ": rowptr[0] must be 0");
    for (long long i = 0; i < n; i++) DAS_CHECK(rp[i + 1] >= rp[i], DAS_ERR_ARG, who + ": rowptr decreases");
    DAS_CHECK(rp[n] < (1LL << 31), DAS_ERR_ARG, who + ": too many entries");
    DAS_CHECK(rp[n] == 0 || ci, DAS_ERR_ARG, who + ": null pointer");
    for (long long i = 0; i < n; i++)
        for (long long k = rp[i]; k < rp[i + 1]; k++) {
            DAS_CHECK(ci[k] >= 0 && ci[k] < ncols, DAS_ERR_ARG, who + ": column index out of range");
            DAS_CHECK(!ascending || k == rp[i] || ci[k - 1] < ci[k], DAS_ERR_ARG, who + ": the columns of a row must ascend strictly");
        }
}

static void debug_graph_scan(long long n, const int* cnt, long long* out, long long* total) {
    const DevBuf<int> dc = krylov_up<int>(cnt, (size_t)n);
    const DevBuf<long long> dout((size_t)n + 1);
    *total = device_exclusive_scan(n, dc.p, dout.p, 0);
    krylov_debug_sync();
    dout.download(out, (size_t)n + 1);
}
// the row-major pattern on the device and its transposed structure
static void debug_graph_transposed(long long n, const long long* rp, const int* ci, DevPattern& P, DevBuf<long long>& trp, DevBuf<int>& tcol) {
    P.n = n; P.nnz = rp[n];
    P.rowptr.upload(rp, (size_t)n + 1);
    P.col.upload(ci, (size_t)P.nnz);
    device_transpose(P, trp, tcol, 0);
    krylov_debug_sync();
}
static void debug_graph_transpose(long long n, const long long* rp, const int* ci, long long* trp, int* tcol) {
    DevPattern P;
    DevBuf<long long> dtrp;
    DevBuf<int> dtcol;
    debug_graph_transposed(n, rp, ci, P, dtrp, dtcol);
    dtrp.download(trp, (size_t)n + 1);
    dtcol.download(tcol, (size_t)P.nnz);
}
static void debug_graph_nets(long long n, const long long* rp, const int* ci, long long nKeep, const long long* keep, long long* cptr, int* crow, int* cpos,
                             unsigned char* isStart, long long* total) {
    DevPattern P;
    DevBuf<long long> dtrp, dcptr;
    DevBuf<int> dtcol, dnet, dcrow, dcpos;
    DevBuf<unsigned char> dstart;
    debug_graph_transposed(n, rp, ci, P, dtrp, dtcol);
    std::vector<int> netOfRow((size_t)n, -1);
    for (long long q = 0; q < nKeep; q++) netOfRow[keep[q]] = (int)q;
    dnet.upload(netOfRow);
    const long long tot = device_build_nets(n, dtrp.p, dtcol.p, dnet.p, P.rowptr.p, P.col.p, dcptr, dcrow, dcpos, dstart, 0);
    krylov_debug_sync();
    dcptr.download(cptr, (size_t)n + 1);
    dcrow.download(crow, (size_t)tot);
    dcpos.download(cpos, (size_t)tot);
    dstart.download(isStart, (size_t)n);
    *total = tot;
}
static void debug_graph_rows_gather(long long nSel, const long long* rows, long long n, const long long* rp, const int* ci, const long long* dst, int* out,
                                    long long outLen) {
    const DevBuf<long long> drows = krylov_up<long long>(rows, (size_t)nSel), drp = krylov_up<long long>(rp, (size_t)n + 1), ddst = krylov_up<long long>(dst, (size_t)nSel);
    const DevBuf<int> dci = krylov_up<int>(ci, (size_t)rp[n]), dout = krylov_up<int>(out, (size_t)outLen);
    krylov_run([&] { hipLaunchKernelGGL(k_rows_gather, dim3((unsigned)((nSel + 3) / 4)), dim3(256), 0, 0, nSel, drows.p, drp.p, dci.p, ddst.p, dout.p); }, dout, out,
               (size_t)outLen);
}
static void debug_compact(long long n, const long long* rp, const int* ci, const double* v, double bound, bool useBound, const unsigned char* owned, long long* nrp,
                          int* nci, double* nv, long long* nnzOut) {
    const size_t nnz = (size_t)rp[n];
    const DevBuf<long long> drp = krylov_up<long long>(rp, (size_t)n + 1);
    const DevBuf<int> dci = krylov_up<int>(ci, nnz);
    const DevBuf<double> dv = krylov_up<double>(v, nnz);
    DevBuf<unsigned char> down;
    if (owned) down.upload(owned, (size_t)n);
    DevBuf<long long> dnrp;
    DevBuf<int> dnci;
    DevBuf<double> dnv;
    const long long kept = filter_compact(n, drp.p, dci.p, dv.p, bound, useBound, owned ? down.p : (const unsigned char*)nullptr, dnrp, dnci, dnv, 0);
    krylov_debug_sync();
    dnrp.download(nrp, (size_t)n + 1);
    dnci.download(nci, (size_t)kept);
    dnv.download(nv, (size_t)kept);
    *nnzOut = kept;
}
static void debug_vecpack(long long n, const long long* rp, const int* ci, const double* v, long long row0, long long nG, int* built, long long* cptr,
                          unsigned char* data, long long* nChunks, const double* x, double* y, long long ylen) {
    const size_t nnz = (size_t)rp[n];
    const DevBuf<long long> drp = krylov_up<long long>(rp, (size_t)n + 1);
    const DevBuf<int> dci = krylov_up<int>(ci, nnz);
    const DevBuf<double> dv = krylov_up<double>(v, nnz);
    VecPack P;
    *built = vecpack_build(P, nG, row0, drp.p, dci.p, dv.p, 0) ? 1 : 0;
    krylov_debug_sync();
    if (!*built) return;
    P.cptr.download(cptr, (size_t)nG + 1);
    P.data.download(data, (size_t)P.nChunks * VP_CHUNK_BYTES);
    *nChunks = P.nChunks;
    if (!x) return;
    const DevBuf<double> dx = krylov_up<double>(x, (size_t)n), dy = krylov_up<double>(y, (size_t)ylen);
    krylov_run([&] { launch_spmv(0, n, drp.p, dci.p, dv.p, P, dx.p, dy.p); }, dy, y, (size_t)ylen);
}
static void debug_spmv_rows(long long nrows, const int* rows, long long n, const long long* rp, const int* ci, const double* v, const double* x, double* buf,
                            long long buflen) {
    const size_t nnz = (size_t)rp[n];
    const DevBuf<int> drows = krylov_up<int>(rows, (size_t)nrows), dci = krylov_up<int>(ci, nnz);
    const DevBuf<long long> drp = krylov_up<long long>(rp, (size_t)n + 1);
    const DevBuf<double> dv = krylov_up<double>(v, nnz), dx = krylov_up<double>(x, (size_t)n), dbuf = krylov_up<double>(buf, (size_t)buflen);
    krylov_run([&] { hipLaunchKernelGGL(k_spmv_rows_to_buf, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, 0, nrows, drows.p, drp.p, dci.p, dv.p, dx.p, dbuf.p); },
               dbuf, buf, (size_t)buflen);
}

}  // namespace das

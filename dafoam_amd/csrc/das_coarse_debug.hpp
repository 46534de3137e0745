// Bodies of the test-only entries das_debug_coarse_* (tests/test_gpu_coarse_kernels.py): the coarse space of the two-level preconditioner
// (das_coarse.hpp) on caller-made structures - no mesh, no solver handle.  These kernels index with what they are given, so everything is
// CHECKED ON THE HOST first (coarse_check_*: DAS_ERR_ARG before the first device call); then the helpers the solver runs are run on the
// null stream: coarse_sort_cells, coarse_assemble, coarse_invert, coarse_restrict_solve, k_coarse_prolong, coarse_az_build, k_az_apply.
// Every output array without a length argument holds COARSE_GUARD entries more than are written; outputs are uploaded and downloaded
// whole, so that the caller finds its sentinel behind the written range.  Nothing in the product path calls them.
#pragma once
#include "das_coarse.hpp"
#include "das_graph_debug.hpp"

namespace das {

constexpr int COARSE_GUARD = 8;
constexpr int COARSE_MAX_AGG = 2048;  // accs[2048] of k_coarse_assemble, the dense inverse

static void coarse_check_nagg(const std::string& who, int nagg) {
    DAS_CHECK(nagg >= 1 && nagg <= COARSE_MAX_AGG, DAS_ERR_ARG, who + ": nagg outside 1 .. 2048");
}
// the field block [off, off + N) inside the n unknowns
static void coarse_check_field(const std::string& who, long long N, long long off, long long n) {
    graph_check_sizes(who, n);
    DAS_CHECK(N > 0, DAS_ERR_ARG, who + ": sizes must be positive");
    DAS_CHECK(off >= 0 && N <= n && off <= n - N, DAS_ERR_ARG, who + ": the field block [off, off + N) does not lie in [0, n)");
}
static void coarse_check_agg(const std::string& who, long long N, int nagg, const int* agg) {
    DAS_CHECK(agg, DAS_ERR_ARG, who + ": null pointer");
    for (long long c = 0; c < N; c++) DAS_CHECK(agg[c] >= -1 && agg[c] < nagg, DAS_ERR_ARG, who + ": aggregate outside [-1, nagg)");
}
// what k_az_build counts: the distinct aggregates among the field columns of every row (at most AZ_CAP are kept).  -> the entries of
// the sparse A Z; overflow = some row touches more than AZ_CAP
static long long coarse_az_count(long long n, const long long* rp, const int* ci, long long N, long long off, const int* agg, bool& overflow) {
    long long nnz = 0;
    overflow = false;
    std::vector<int> seen;
    for (long long i = 0; i < n; i++) {
        seen.clear();
        for (long long k = rp[i]; k < rp[i + 1]; k++) {
            const long long j = (long long)ci[k] - off;
            if (j < 0 || j >= N || agg[j] < 0) continue;
            if (std::find(seen.begin(), seen.end(), agg[j]) != seen.end()) continue;
            if ((int)seen.size() == AZ_CAP) { overflow = true; continue; }
            seen.push_back(agg[j]);
        }
        nnz += (long long)seen.size();
    }
    return nnz;
}

static void debug_coarse_assemble(int nagg, long long N, long long off, long long n, const long long* rp, const int* ci, const double* v, const int* aggRow,
                                  const int* aggCol, int transpose, double diagScale, double* E) {
    std::vector<long long> aptr;
    std::vector<int> cells;
    coarse_sort_cells(N, nagg, aggRow, aptr, cells);
    const size_t nnz = (size_t)rp[n], elen = (size_t)nagg * nagg + COARSE_GUARD;
    const DevBuf<long long> daptr = krylov_up<long long>(aptr.data(), aptr.size()), drp = krylov_up<long long>(rp, (size_t)n + 1);
    const DevBuf<int> dcells = krylov_up<int>(cells.data(), cells.size()), dci = krylov_up<int>(ci, nnz), dcol = krylov_up<int>(aggCol, (size_t)N);
    const DevBuf<double> dv = krylov_up<double>(v, nnz), dE = krylov_up<double>(E, elen);
    krylov_run([&] { coarse_assemble(nagg, daptr.p, dcells.p, N, off, drp.p, dci.p, dv.p, dcol.p, dE.p, transpose, diagScale, 0); }, dE, E, elen);
}
static void debug_coarse_invert(int n, const double* Ein, double* Inv, int* singular) {
    const size_t len = (size_t)n * n + COARSE_GUARD;
    const DevBuf<double> dE = krylov_up<double>(Ein, (size_t)n * n), dInv = krylov_up<double>(Inv, len);
    const DevBuf<int> sing(1);
    *singular = coarse_invert(n, dE.p, dInv.p, sing.p, 0);
    krylov_debug_sync();
    dInv.download(Inv, len);
}
static void debug_coarse_correct(int nagg, long long N, long long off, long long n, const int* agg, const double* Einv, const double* r, double* t, double* u,
                                 double* y, long long ylen, int set) {
    std::vector<long long> aptr;
    std::vector<int> cells;
    coarse_sort_cells(N, nagg, agg, aptr, cells);
    const size_t glen = (size_t)nagg + COARSE_GUARD;
    const DevBuf<long long> daptr = krylov_up<long long>(aptr.data(), aptr.size());
    const DevBuf<int> dcells = krylov_up<int>(cells.data(), cells.size()), dagg = krylov_up<int>(agg, (size_t)N);
    const DevBuf<double> dEinv = krylov_up<double>(Einv, (size_t)nagg * nagg), dr = krylov_up<double>(r, (size_t)n), dt = krylov_up<double>(t, glen),
                         du = krylov_up<double>(u, glen), dy = krylov_up<double>(y, (size_t)ylen);
    krylov_run([&] {
        coarse_restrict_solve(nagg, daptr.p, dcells.p, off, dr.p, nagg, 0, dEinv.p, dt.p, du.p, 0);
        hipLaunchKernelGGL(k_coarse_prolong, dim3(nblk(n, 256)), dim3(256), 0, 0, N, n, off, dagg.p, du.p, dy.p, set);
    }, dy, y, (size_t)ylen);
    dt.download(t, glen);
    du.download(u, glen);
}
static void debug_coarse_az(int nagg, long long n, const long long* rp, const int* ci, const double* v, long long N, long long off, const int* agg, int* cnt,
                            long long* ptr, int* oa, double* ov, long long cap, long long* nnz, int* overflow, const double* u, const double* vec, double* out,
                            long long outlen) {
    const size_t nz = (size_t)rp[n];
    const DevBuf<long long> drp = krylov_up<long long>(rp, (size_t)n + 1);
    const DevBuf<int> dci = krylov_up<int>(ci, nz), dagg = krylov_up<int>(agg, (size_t)N);
    const DevBuf<double> dv = krylov_up<double>(v, nz);
    DevBuf<int> dcnt = krylov_up<int>(cnt, (size_t)n + COARSE_GUARD), doa = krylov_up<int>(oa, (size_t)cap);
    DevBuf<long long> dptr = krylov_up<long long>(ptr, (size_t)n + 1 + COARSE_GUARD);
    DevBuf<double> dov = krylov_up<double>(ov, (size_t)cap);
    long long nn = 0;
    const bool built = coarse_az_build(n, drp.p, dci.p, dv.p, N, off, dagg.p, dcnt, dptr, doa, dov, nn, 0, [](int f) { return f; });
    krylov_debug_sync();
    *overflow = built ? 0 : 1;
    if (!built) return;
    // (the buffers held what was needed, so coarse_az_build allocated none anew; the prefix sum was uploaded over the first n + 1 offsets)
    dcnt.download(cnt, (size_t)n + COARSE_GUARD);
    dptr.download(ptr, (size_t)n + 1 + COARSE_GUARD);
    doa.download(oa, (size_t)cap);
    dov.download(ov, (size_t)cap);
    *nnz = nn;
    const DevBuf<double> du = krylov_up<double>(u, (size_t)nagg), dvec = krylov_up<double>(vec, vec ? (size_t)n : 0), dout = krylov_up<double>(out, (size_t)outlen);
    krylov_run([&] { hipLaunchKernelGGL(k_az_apply, dim3(nblk(n, 256)), dim3(256), 0, 0, n, dptr.p, doa.p, dov.p, du.p, vec ? dvec.p : (const double*)nullptr, dout.p); },
               dout, out, (size_t)outlen);
}

}  // namespace das

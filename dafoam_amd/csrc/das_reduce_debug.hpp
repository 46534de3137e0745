// Bodies of the test-only entries das_debug_reduce_* (tests/test_gpu_reduce_kernels.py): the two-stage fixed-order reductions every
// objective function ends in - the KS sequence, the cell-set sum, the residualNorm sum, the heat-source and actuator-disk totals, the
// group sum and the seeds . dR products - and the two gathers without atomics, on caller-made arrays: no mesh, no solver handle.  Each
// body runs THE LAUNCH HELPER THE SOLVER RUNS (das_facefn.hpp, das_cellfn.hpp, das_meshquality.hpp, das_heatsource.hpp,
// das_actuatordisk.hpp, das_reduce.hpp) on the null stream.  Every array - input or output - is uploaded whole and downloaded whole, so
// that the caller finds its inputs untouched and the sentinels it put behind the written range intact.  The arguments are checked on the
// host before the first device call (das_device.hip).  Nothing in the product path calls them.
#pragma once
#include "das_actuatordisk.hpp"
#include "das_cellfn.hpp"
#include "das_facefn.hpp"
#include "das_heatsource.hpp"
#include "das_krylov_debug.hpp"
#include "das_meshquality.hpp"
#include "das_reduce.hpp"

namespace das {

// a host array of len entries mirrored on the device (null: no array); back() copies the device's state over the host's
template <class T>
struct ReduceArr {
    DevBuf<T> d;
    void* h;
    size_t len;
    ReduceArr(void* h_, long long len_) : d(krylov_up<T>(h_, h_ ? (size_t)len_ : 0)), h(h_), len(h_ ? (size_t)len_ : 0) {}
    T* p() const { return h ? d.p : nullptr; }
    void back() const { d.download((T*)h, len); }
};

static void debug_reduce_ks(long long n, double* a, double k, double outer, double* ms, long long msLen, double* pmax, double* psum, long long partLen, double* w,
                            long long wLen, int* nb) {
    const ReduceArr<double> da(a, n), dms(ms, msLen), dpm(pmax, partLen), dps(psum, partLen), dw(w, wLen);
    launch_ks_max(0, n, da.p(), k, dpm.p(), dms.p());
    launch_ks_expsum(0, n, da.p(), k, dps.p(), dms.p());
    launch_ks_weights(0, n, da.p(), k, dms.p(), outer, dw.p());
    krylov_debug_sync();
    da.back(); dms.back(); dpm.back(); dps.back(); dw.back();
    *nb = ks_blocks(n);
}
static void debug_reduce_group_sum(long long cnt, unsigned char* group, double* fv, double* out2, long long outLen) {
    const ReduceArr<unsigned char> dg(group, cnt);
    const ReduceArr<double> dfv(fv, cnt), dout(out2, outLen);
    launch_group_sum(0, cnt, dg.p(), dfv.d.p, dout.p());
    krylov_debug_sync();
    dg.back(); dfv.back(); dout.back();
}
// which: 0 = launch_tangent_dot, 1 = launch_ad_dot (R: n Dual<1> as pairs {v, d[0]})
static void debug_reduce_dual_dot(int which, long long n, double* R, double* psi, double* part, long long partLen, double* out, long long outLen, int* nb) {
    const ReduceArr<Dual<1>> dR(R, n);
    const ReduceArr<double> dpsi(psi, n), dpart(part, partLen), dout(out, outLen);
    if (which == 0) launch_tangent_dot(0, n, dR.d.p, dpsi.d.p, dpart.p(), dout.p());
    else launch_ad_dot(0, n, dpsi.d.p, dR.d.p, dpart.p(), dout.p());
    krylov_debug_sync();
    dR.back(); dpsi.back(); dpart.back(); dout.back();
    *nb = which == 0 ? DAS_TANGENT_DOT_BLOCKS : hs_blocks(n);
}
static void debug_reduce_sv_dot(long long n, double* a, double* b, double* part, long long partLen, double* out2, long long outLen, int* nb) {
    const ReduceArr<double> da(a, n), db(b, n), dpart(part, partLen), dout(out2, outLen);
    launch_sv_dot(0, n, da.p(), db.p(), dpart.p(), dout.p());
    krylov_debug_sync();
    da.back(); db.back(); dpart.back(); dout.back();
    *nb = sv_dot_blocks(n);
}
static void debug_reduce_cellfn(long long nt, int* cell, long long* idx, double* data, int square, int mv, long long nCells, const double* V, long long nSrc, double* src,
                                double coef, double* part, long long partLen, double* out, long long outLen, double* sc, double g, double* grad, long long gradLen,
                                int* nb) {
    std::vector<CellGeom> cg((size_t)nCells);
    for (long long c = 0; c < nCells; c++) {
        cg[c].C[0] = cg[c].C[1] = cg[c].C[2] = 0.0;
        cg[c].V = V[c];
        cg[c].y = 0.0;
    }
    DevBuf<CellGeom> dcg((size_t)nCells);
    dcg.upload(cg);
    const ReduceArr<int> dcell(cell, nt);
    const ReduceArr<long long> didx(idx, nt);
    const ReduceArr<double> ddata(data, nt), dsrc(src, nSrc), dpart(part, partLen), dout(out, outLen), dsc(sc, nSrc), dgrad(grad, gradLen);
    const CellFnView f{nt, dcell.p(), didx.p(), ddata.p(), square, mv};
    launch_cellfn_value(0, f, dcg.p, dsrc.p(), coef, dpart.p(), dout.p());
    DAS_HIP(hipMemsetAsync(dgrad.p(), 0, (size_t)nSrc * sizeof(double), 0));  // as cell_function_gradient zeroes the product
    launch_cellfn_grad(0, f, dcg.p, dsrc.p(), dsc.p(), g, dgrad.p());
    krylov_debug_sync();
    dcell.back(); didx.back(); ddata.back(); dsrc.back(); dpart.back(); dout.back(); dsc.back(); dgrad.back();
    *nb = cellfn_blocks(nt);
}
static void debug_reduce_rn(long long n, const RnRows& r, double* R, double* term, long long termLen, double* part, long long partLen, double* ms, long long msLen,
                            double F, double coef, double* g, long long gLen, int* nb) {
    const ReduceArr<double> dR(R, n), dterm(term, termLen), dpart(part, partLen), dms(ms, msLen), dg(g, gLen);
    launch_rn_sum(0, n, r, dR.p(), dterm.p(), dpart.p(), dms.p());
    launch_rn_seeds(0, n, r, dR.p(), F, coef, dg.p());
    krylov_debug_sync();
    dR.back(); dterm.back(); dpart.back(); dms.back(); dg.back();
    *nb = ks_blocks(n);
}
// launch_hs_sum<double> for the kinds that need volumes only
static void debug_reduce_hs_sum(int kind, int nC, const double* V, unsigned char* member, double* field, double* psi, int byV, double power, double* vt, double* part,
                                long long partLen, double* out, long long outLen, int* nb) {
    std::vector<CellGeom> cg((size_t)nC);
    for (int c = 0; c < nC; c++) {
        cg[c].C[0] = cg[c].C[1] = cg[c].C[2] = 0.0;
        cg[c].V = V[c];
        cg[c].y = 0.0;
    }
    DevBuf<CellGeom> dcg((size_t)nC);
    dcg.upload(cg);
    const ReduceArr<unsigned char> dmem(member, nC);
    const ReduceArr<double> dfield(field, nC), dpsi(psi, nC), dvt(vt, 1), dpart(part, partLen), dout(out, outLen);
    HsView<double> v{};
    v.kind = kind;
    v.member = dmem.p();
    v.field = dfield.p();
    v.power = power;
    v.snapCell = -1;
    launch_hs_sum<double, double, double>(0, v, nC, (const CellGeom*)dcg.p, dpsi.p(), byV, (const double*)dvt.p(), dpart.p(), dout.p());
    krylov_debug_sync();
    dmem.back(); dfield.back(); dpsi.back(); dvt.back(); dpart.back(); dout.back();
    *nb = hs_blocks(nC);
}
// the second stages on caller-made partials: pair = 0 launch_hs_final (nb entries), pair = 1 launch_ad_final (nb pairs); R = double or Dual<1>
template <class R>
static void debug_reduce_final(int pair, int nb, double* part, long long partDoubles, double* out, long long outLen) {
    const size_t per = sizeof(R) / sizeof(double);
    const ReduceArr<R> dpart(part, (long long)(partDoubles / per)), dout(out, (long long)(outLen / per));
    if (pair) launch_ad_final<R>(0, nb, (const R*)dpart.p(), dout.p());
    else launch_hs_final<R>(0, nb, (const R*)dpart.p(), dout.p());
    krylov_debug_sync();
    dpart.back(); dout.back();
}
static void debug_reduce_owner_gather(int nC, int* cf_ptr, int* cf_face, long long nFt, double* ft, double* tc, long long tcLen) {
    const ReduceArr<int> dptr(cf_ptr, (long long)nC + 1), dface(cf_face, cf_ptr[nC]);
    const ReduceArr<double> dft(ft, nFt), dtc(tc, tcLen);
    launch_mq_owner_gather(0, nC, dptr.p(), dface.d.p, dft.d.p, dtc.p());
    krylov_debug_sync();
    dptr.back(); dface.back(); dft.back(); dtc.back();
}
static void debug_reduce_vm_gather(int nC, int nIF, int* cf_ptr, int* cf_face, int* cf_other, int* colors, int col, double* tc, double seed, double* out,
                                   long long outLen) {
    const ReduceArr<int> dptr(cf_ptr, (long long)nC + 1), dface(cf_face, cf_ptr[nC]), dother(cf_other, cf_ptr[nC]), dcol(colors, 3LL * nC);
    const ReduceArr<double> dtc(tc, nC), dout(out, outLen);
    DevMesh m{};  // only what k_vm_gather reads
    m.nC = nC;
    m.nIF = nIF;
    m.cf_ptr = dptr.p();
    m.cf_face = dface.d.p;
    m.cf_other = dother.d.p;
    launch_vm_gather(0, m, dcol.p(), col, dtc.p(), seed, dout.p());
    krylov_debug_sync();
    dptr.back(); dface.back(); dother.back(); dcol.back(); dtc.back(); dout.back();
}

}  // namespace das

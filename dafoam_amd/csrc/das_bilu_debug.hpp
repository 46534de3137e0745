// Bodies of the test-only entries das_debug_bilu_* (tests/test_gpu_bilu_kernels.py): the node-block ILU(0) of das_bilu.hpp on a
// caller-made node structure and scalar CSR matrix - no mesh, no solver handle.  The structure is CHECKED ON THE HOST first (the sweeps
// wait on their dependencies: a structure that is not a valid level order must be refused, never tried), then the code the solver runs
// is run on the null stream: bilu_numeric (scatter, pad, factor, pack, bilu_launch_shape), bilu_apply, bilu_apply_multi.  Nothing in the
// product path calls them.
#pragma once
#include "das_bilu.hpp"

namespace das {

// everything but null pointers and sizes, which the callers of this check first: DAS_ERR_ARG for whatever is not a level-ordered
// symmetric node pattern with in-range maps
static void bilu_debug_validate(const std::string& who, const das_bilu_debug_t& d) {
    const int nN = d.nNodes;
    auto bad = [&](bool cond, const char* what) { DAS_CHECK(!cond, DAS_ERR_ARG, who + ": " + what); };
    bad(d.bptr[0] != 0, "bptr[0] must be 0");
    for (int p = 0; p < nN; p++) bad(d.bptr[p + 1] < d.bptr[p], "bptr decreases");
    bad(d.bptr[nN] >= (1LL << 40), "too many blocks");
    // levels: lvlPtr covers [0, nNodes]
    bad(d.lvlPtr[0] != 0 || d.lvlPtr[d.nLevels] != nN, "lvlPtr must cover [0, nNodes]");
    for (int l = 0; l < d.nLevels; l++) bad(d.lvlPtr[l + 1] < d.lvlPtr[l], "lvlPtr decreases");
    std::vector<int> level(nN);
    for (int l = 0; l < d.nLevels; l++) for (int p = d.lvlPtr[l]; p < d.lvlPtr[l + 1]; p++) level[p] = l;
    for (int p = 0; p < nN; p++) {
        const long long rb = d.bptr[p], re = d.bptr[p + 1], rd = d.bdiag[p];
        bad(rd < rb || rd >= re, "bdiag outside its row");
        for (long long e = rb; e < re; e++) {
            const int J = d.bcol[e];
            bad(J < 0 || J >= nN, "block column out of range");
            bad(e > rb && d.bcol[e - 1] >= J, "block columns of a row must ascend");
        }
        bad(d.bcol[rd] != p, "bdiag does not point at the diagonal block");
    }
    for (int p = 0; p < nN; p++)
        for (long long e = d.bptr[p]; e < d.bptr[p + 1]; e++) {
            const int J = d.bcol[e];
            if (J == p) continue;
            const int* jb = d.bcol + d.bptr[J];
            const int* je = d.bcol + d.bptr[J + 1];
            bad(!std::binary_search(jb, je, p), "the node pattern is not symmetric");
            bad(J < p && level[J] >= level[p], "a dependency does not lie in an earlier level");
        }
    for (long long i = 0; i < (long long)nN * BILU_NB; i++) {
        bad(d.nodeUnk[i] < -1 || d.nodeUnk[i] >= d.n, "nodeUnk out of range");
        if (d.nodeOut) bad(d.nodeOut[i] < -1 || d.nodeOut[i] >= d.n, "nodeOut out of range");
    }
    for (long long i = 0; i < (long long)d.nMaps * d.An; i++) {
        bad(d.unkNode[i] < -1 || d.unkNode[i] >= nN, "unkNode out of range");
        bad(d.unkSlot[i] >= BILU_NB, "unkSlot must be below 8");
    }
    bad(d.rp[0] != 0, "rowptr[0] must be 0");
    for (long long i = 0; i < d.An; i++) bad(d.rp[i + 1] < d.rp[i], "rowptr decreases");
    const long long nnz = d.rp[d.An];
    bad(nnz > 0 && !(d.ci && d.val), "null pointer");
    for (long long k = 0; k < nnz; k++) bad(d.ci[k] < 0 || d.ci[k] >= d.An, "CSR column out of range");
}

// null pointers and sizes, then the structure
static void bilu_debug_check(const std::string& who, const das_bilu_debug_t* d) {
    DAS_CHECK(d, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK(d->nNodes > 0 && d->nLevels > 0 && d->nMaps > 0 && d->n > 0 && d->An > 0, DAS_ERR_ARG, who + ": sizes must be positive");
    DAS_CHECK(d->nNodes < (1 << 27) && d->An <= d->n && d->n < (1LL << 31), DAS_ERR_ARG, who + ": sizes out of range (An <= n < 2^31)");
    DAS_CHECK(d->nodeUnk && d->late && d->bptr && d->bdiag && d->bcol && d->lvlPtr && d->unkNode && d->unkSlot && d->rp, DAS_ERR_ARG, who + ": null pointer");
    DAS_CHECK((d->fp32 == 0 || d->fp32 == 1) && (d->transpose == 0 || d->transpose == 1), DAS_ERR_ARG, who + ": fp32 and transpose are 0 or 1");
    bilu_debug_validate(who, *d);
}

// the checked structure as the NodeILU that bilu_build_structure would leave, then the solver's numeric setup
static void bilu_debug_setup(const das_bilu_debug_t& d, NodeILU& P) {
    const int nN = d.nNodes;
    const std::vector<long long> bptr(d.bptr, d.bptr + nN + 1), bdiag(d.bdiag, d.bdiag + nN);
    const std::vector<int> bcol(d.bcol, d.bcol + bptr[nN]);
    std::vector<std::vector<int>> unkNode(d.nMaps);
    std::vector<std::vector<unsigned char>> unkSlot(d.nMaps);
    BiluStructRef S{&bptr, &bdiag, &bcol, {}, {}};
    for (int q = 0; q < d.nMaps; q++) {
        unkNode[q].assign(d.unkNode + q * d.An, d.unkNode + (q + 1) * d.An);
        unkSlot[q].assign(d.unkSlot + q * d.An, d.unkSlot + (q + 1) * d.An);
    }
    for (int q = 0; q < d.nMaps; q++) { S.unkNode.push_back(&unkNode[q]); S.unkSlot.push_back(&unkSlot[q]); }
    P.n = d.n; P.nNodes = nN; P.nLevels = d.nLevels; P.nnzB = bptr[nN]; P.nPrimary = nN;
    for (int p = 0; p < nN; p++) P.maxRow = std::max(P.maxRow, (int)(bptr[p + 1] - bptr[p]));
    P.h_nodeUnk.assign(d.nodeUnk, d.nodeUnk + (size_t)nN * BILU_NB);
    if (d.nodeOut) P.h_nodeOut.assign(d.nodeOut, d.nodeOut + (size_t)nN * BILU_NB);
    P.h_late.assign(d.late, d.late + nN);
    P.h_lvlPtr.assign(d.lvlPtr, d.lvlPtr + d.nLevels + 1);
    P.h_bptr = bptr; P.h_bcol = bcol;
    const size_t nnz = (size_t)d.rp[d.An];
    DevBuf<long long> d_rp(d.An + 1);
    DevBuf<int> d_ci(std::max<size_t>(nnz, 1));
    DevBuf<double> d_av(std::max<size_t>(nnz, 1));
    d_rp.upload(d.rp, (size_t)d.An + 1); d_ci.upload(d.ci, nnz); d_av.upload(d.val, nnz);
    bilu_numeric(d.n, S, d.fp32 != 0, d.An, d_rp.p, d_ci.p, d_av.p, 0, P, false, d.transpose != 0, d.diagScale, d.shiftExLo, d.shiftExHi, d.shiftEnd, wall_seconds());
}

static void debug_bilu_factor(const das_bilu_debug_t& d, long long* Lptr, long long* Uptr, int* Lcol, int* Ucol, void* Lval, void* Uval, double* invD, int* nshift) {
    NodeILU P;
    bilu_debug_setup(d, P);
    const size_t nN = (size_t)d.nNodes;
    P.Lptr.download(Lptr, nN + 1); P.Uptr.download(Uptr, nN + 1);
    P.Lcol.download(Lcol, (size_t)P.nL); P.Ucol.download(Ucol, (size_t)P.nU);
    if (d.fp32) { P.Lvalf.download((float*)Lval, (size_t)P.nL * BILU_NB2); P.Uvalf.download((float*)Uval, (size_t)P.nU * BILU_NB2); }
    else { P.Lval.download((double*)Lval, (size_t)P.nL * BILU_NB2); P.Uval.download((double*)Uval, (size_t)P.nU * BILU_NB2); }
    P.invD.download(invD, nN * BILU_NB2);
    *nshift = P.nshift;
}

// S of the last group that bilu_apply_multi launches for nrhs right-hand sides (groups of 4, then 2, then 1)
static int bilu_debug_last_group(int nrhs) { return (nrhs & 1) ? 1 : ((nrhs & 3) == 2 ? 2 : 4); }

static void debug_bilu_apply(const das_bilu_debug_t& d, int nrhs, long long ld, const double* b, double* out, int twice, double* y, double* z, int* abortFlag,
                             int* info) {
    NodeILU P;
    bilu_debug_setup(d, P);
    const size_t len = (size_t)nrhs * ld;
    DevBuf<double> db(len), dout(len);
    db.upload(b, len);
    for (int rep = 0; rep < (twice ? 2 : 1); rep++) {
        dout.upload(out, len);  // the caller's sentinels again: a second application that did nothing would leave them
        if (nrhs == 1) bilu_apply(P, db.p, dout.p, 0);
        else bilu_apply_multi(P, db.p, dout.p, ld, nrhs, 0);
        DAS_HIP(hipGetLastError());
        DAS_HIP(hipStreamSynchronize(0));
    }
    dout.download(out, len);
    const int S = bilu_debug_last_group(nrhs);
    const size_t nw = (size_t)d.nNodes * BILU_NB * S;
    (S == 1 ? P.y : P.ym).download(y, nw);
    (S == 1 ? P.z : P.zm).download(z, nw);
    *abortFlag = bilu_aborted(P, 0) ? 1 : 0;
    info[0] = P.launchGrid; info[1] = P.launchSleep; info[2] = P.launchPerXcd; info[3] = bilu_xcd_probe(0);
}

}  // namespace das

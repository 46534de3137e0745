"""The node-block ILU(0) preconditioner (dafoam_amd/csrc/das_bilu.hpp) restated in plain numpy, generators of synthetic node
structures that reach the branches no mesh reaches, and the comparison functions with their DERIVED bounds (u = 2^-53, first order).

Every comparison is LOCAL: a stored block or node value is compared with what the values THE DEVICE STORED for its inputs give in
np.longdouble, so that one wrong row cannot hide in a norm and an ill-conditioned neighbour cannot excuse it:

  L_pJ   = (A_pJ - sum_{M<J} L_pM U_MJ) invD_J     |err| <= (T + 10) u (|A| + sum |L||U|) |invD|,  T = 8 #M + 1
  U_pJ   =  A_pJ - sum_{M<p} L_pM U_MJ             |err| <= (T + 10) u (|A| + sum |L||U|)
  invD_p = inverse of D_p = A_pp - sum L_pM U_Mp   |err| <= 8^3 u kappa_inf(D_p) ||inv||_inf + |inv| dD |inv|,  dD = (T + 10) u (|A| + sum |L||U|)
  y_p    = b_p - sum L_pJ y_J                      |err| <= (T + 1) u (|b| + sum |L||y|),  T = 8 nE + 1
  z_p    = invD_p (y_p - sum U_pJ z_J)             |err| <= (T + 10) u |invD| (|y| + sum |U||z|)
  out[nodeOut] == z bitwise, every other entry of out untouched;  float factor == float32(double factor) bitwise.

(8 #M products and as many subtractions make A - sum L U, 8 more products the multiplication with invD; a sum of T products in any
order, fused or not, is within T u of the sum of their magnitudes.)  The functions are generic in the number type: dtype = LD is the
reference, dtype = np.float64 the stand-in for the device that tests/test_bilu_reference_cpu.py mutates.  Used by
tests/test_gpu_bilu_kernels.py and tests/test_bilu_reference_cpu.py."""
import numpy as np

from krylov_reference import LD, U, vector

NB = 8
SENTINEL = -6.0e30
OFF_SCALE = 0.1     # the off-diagonal blocks of a block row sum to about this (times the entries, 0.5 .. 3): the incomplete factor stays tame
KAPPA_CAP = 50.0    # cap on kappa_inf of every diagonal block of the reference factor (asserted by factor(); see diag_block)
TINY_LEAD = 4e-14   # leading entry of a row-permuted diagonal block: 1e-14 of its large entries
ROW_LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 25]
NODE_COUNTS = [1, 2, 7, 8, 9, 17, 64, 65]


class Struct:
    """a node structure in processing order, its (unkNode, unkSlot) maps and the scalar CSR matrix that goes with it"""

    def row(self, p):
        return self.bcol[self.bptr[p] : self.bptr[p + 1]]

    def nL(self, p):
        return int(self.bdiag[p] - self.bptr[p])

    def nU(self, p):
        return int(self.bptr[p + 1] - self.bdiag[p] - 1)

    def find(self, p, J):
        r = self.row(p)
        k = int(np.searchsorted(r, J))
        return int(self.bptr[p]) + k if k < r.size and r[k] == J else -1


# ---- generators of node graphs (lists of predecessors in natural order) -----------------------------------------------------------
def random_graph(nN, seed, maxdeg=3, window=12):
    rng = np.random.default_rng(seed)
    return [sorted(rng.choice(np.arange(max(0, i - window), i), size=min(i, int(rng.integers(0, maxdeg + 1))), replace=False).tolist()) for i in range(nN)]


def row_length_graph(seed):
    """every length of ROW_LENGTHS as the number of predecessors of some node; mirror() of it has them as successors"""
    rng = np.random.default_rng(seed)
    at = {0: 0, 2: 1, 8: 7, 10: 8, 12: 9, 18: 15, 20: 16, 22: 17, 30: 25}  # node: predecessors
    lower = []
    for i in range(32):
        t = at.get(i, int(rng.integers(0, min(i, 2) + 1)))
        lower.append(sorted(rng.choice(i, size=t, replace=False).tolist()) if t else [])
    return lower


def mirror(lower):
    """the same graph with the node order reversed: predecessors become successors"""
    N = len(lower)
    out = [[] for _ in range(N)]
    for i, pre in enumerate(lower):
        for j in pre:
            out[N - 1 - j].append(N - 1 - i)
    return [sorted(x) for x in out]


def union(*graphs):
    """disjoint union; returns (lower, block id of every node)"""
    lower, blk, off = [], [], 0
    for b, g in enumerate(graphs):
        lower += [[j + off for j in pre] for pre in g]
        blk += [b] * len(g)
        off += len(g)
    return lower, np.array(blk)


def layered_graph(per_level, n_levels, seed, deg=3):
    """per_level mutually independent nodes per level, each coupled to `deg` nodes of the level before"""
    rng = np.random.default_rng(seed)
    lower = [[] for _ in range(per_level)]
    for l in range(1, n_levels):
        for _ in range(per_level):
            lower.append(sorted(((l - 1) * per_level + rng.choice(per_level, size=deg, replace=False)).tolist()))
    return lower


def diag_block(m, seed, permute=True):
    """m x m: 4 I + 0.3 R with |R_ij| >= 0.5 (well conditioned), rows shifted by one so that every diagonal entry is one of the small
    ones, and the leading entry set to 1e-14 of the large ones: without row pivoting the first elimination step loses every digit"""
    W = 4.0 * np.eye(m) + 0.3 * vector(m * m, seed).reshape(m, m)
    if permute and m >= 2:
        W = np.roll(W, -1, axis=0)
        W[0, 0] = TINY_LEAD
    return W


def make(lower, seed, blk=None, n_late=0, copies=0, n_unowned=0, late_late=0, outside=0, permute=True, full_nodes=(), empty_nodes=None, singular=()):
    """The structure and matrix of a node graph.  blk: block of every node (edges stay inside a block); n_late: late nodes appended,
    coupled to primary nodes only; copies: so many nodes of block 0 get an overlap copy in block 1 (same unknowns, nodeOut = -1)
    coupled to nodes of block 1; n_unowned: unknowns in no node; late_late / outside: matrix entries between uncoupled late nodes
    (dropped by design) / uncoupled primary nodes (an error); singular: natural nodes without predecessors whose diagonal block gets
    an exactly singular last row: zeros for the first of them, -1e-305 in the last column for the others."""
    rng = np.random.default_rng(seed)
    lower = [list(x) for x in lower]
    n0 = len(lower)
    blk = np.zeros(n0, dtype=int) if blk is None else np.asarray(blk)
    nblocks = int(blk.max()) + 1 if copies == 0 else 2
    late0 = [0] * n0
    for _ in range(n_late):
        b = int(rng.integers(0, int(blk.max()) + 1))
        cand = [i for i in range(n0) if blk[i] == b]
        lower.append(sorted(rng.choice(cand, size=min(len(cand), int(rng.integers(1, 4))), replace=False).tolist()))
        late0.append(1)
        blk = np.append(blk, b)
    copy_of = {}
    if copies:
        own = rng.choice([i for i in range(n0) if blk[i] == 0], size=copies, replace=False)
        cand = [i for i in range(n0) if blk[i] == 1]
        for o in own:
            lower.append(sorted(rng.choice(cand, size=min(len(cand), 2), replace=False).tolist()))
            late0.append(0)
            blk = np.append(blk, 1)
            copy_of[len(lower) - 1] = int(o)
    nN = len(lower)
    # levels by longest path, processing order = level order (stable)
    level = np.zeros(nN, dtype=int)
    for i in range(nN):
        assert all(j < i for j in lower[i])
        level[i] = 1 + max((level[j] for j in lower[i]), default=-1)
    order = np.lexsort((np.arange(nN), level))
    pos = np.empty(nN, dtype=int)
    pos[order] = np.arange(nN)
    S = Struct()
    S.nN, S.level, S.natural, S.pos = nN, level[order], order, pos
    S.lvlPtr = np.concatenate([[0], np.cumsum(np.bincount(level, minlength=level.max() + 1))]).astype(np.int32)
    rows = [{p} for p in range(nN)]
    for i in range(nN):
        for j in lower[i]:
            rows[pos[i]].add(int(pos[j]))
            rows[pos[j]].add(int(pos[i]))
    rows = [sorted(r) for r in rows]
    S.bptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    S.bcol = np.concatenate(rows).astype(np.int32)
    S.bdiag = np.array([S.bptr[p] + rows[p].index(p) for p in range(nN)], dtype=np.int64)
    S.late = np.array([late0[i] for i in order], dtype=np.uint8)
    S.blk = blk[order]
    # slots: 0 .. 8 occupied per node, anywhere in the node; an empty node where there is room for one
    occ = [sorted(rng.choice(NB, size=int(rng.integers(1, NB + 1)), replace=False).tolist()) for _ in range(nN)]
    for i in full_nodes:
        occ[i] = list(range(NB))
    for i in singular:
        occ[i] = list(range(NB))
        assert not lower[i]
    for i in ([nN // 2] if nN >= 3 else []) if empty_nodes is None else empty_nodes:
        if i not in copy_of.values() and i not in singular:
            occ[i] = []
    for c, o in copy_of.items():
        occ[c] = occ[o]
    n_own = sum(len(occ[i]) for i in range(nN) if i not in copy_of)
    S.n = n = max(n_own + n_unowned, 1)
    ids = rng.permutation(n)
    S.unowned = np.sort(ids[n_own:])
    unk0 = np.full((nN, NB), -1, dtype=np.int32)
    k = 0
    for i in range(nN):
        if i not in copy_of:
            unk0[i, occ[i]] = ids[k : k + len(occ[i])]
            k += len(occ[i])
    for c, o in copy_of.items():
        unk0[c] = unk0[o]
    S.nodeUnk = unk0[order]
    S.nodeOut = S.nodeUnk.copy()
    for c in copy_of:
        S.nodeOut[pos[c]] = -1
    S.has_copies = bool(copy_of)
    overlap = np.zeros(n, dtype=bool)
    for c in copy_of:
        overlap[unk0[c][unk0[c] >= 0]] = True
    S.maps = []
    for q in range(nblocks):
        un, us = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        for p in range(nN):
            if nblocks == 1 or S.blk[p] == q:
                for s in range(NB):
                    if S.nodeUnk[p, s] >= 0:
                        un[S.nodeUnk[p, s]], us[S.nodeUnk[p, s]] = p, s
        S.maps.append((un, us))
    # the scalar matrix: a dense coupling of the occupied slots of every coupled node pair
    I, Jc, V = [], [], []
    for p in range(nN):
        nat = int(order[p])
        own = copy_of.get(nat, nat)
        up = S.nodeUnk[p][S.nodeUnk[p] >= 0]
        if up.size == 0:
            continue
        D = diag_block(up.size, [seed, 1, own], permute)
        if own in singular:
            D[-1, :] = 0.0
            if own != singular[0]:
                D[-1, -1] = -1e-305
        I.append(np.repeat(up, up.size)); Jc.append(np.tile(up, up.size)); V.append(D.ravel())
        for J in rows[p]:
            uj = S.nodeUnk[J][S.nodeUnk[J] >= 0]
            if J == p or uj.size == 0:
                continue
            ii, jj = np.repeat(up, uj.size), np.tile(uj, up.size)
            keep = ~(overlap[ii] & overlap[jj])
            vv = vector(ii.size, [seed, 2, p, J]) * (OFF_SCALE / (len(rows[p]) - 1))
            I.append(ii[keep]); Jc.append(jj[keep]); V.append(vv[keep])
    S.n_late_late = S.n_outside = 0
    for kind, cnt in (("late", late_late), ("out", outside)):
        pool = [p for p in range(nN) if S.late[p] == (kind == "late") and (S.nodeUnk[p] >= 0).any() and (S.nodeUnk[p] == S.nodeOut[p]).all()]
        pairs = [(a, b) for a in pool for b in pool if a != b and S.blk[a] == S.blk[b] and S.find(a, b) < 0]
        assert cnt == 0 or pairs, "no uncoupled pair of this kind"
        for t in range(cnt):
            a, b = pairs[int(rng.integers(0, len(pairs)))]
            pairs.remove((a, b))
            i, j = S.nodeUnk[a][S.nodeUnk[a] >= 0][0], S.nodeUnk[b][S.nodeUnk[b] >= 0][0]
            I.append(np.array([i])); Jc.append(np.array([j])); V.append(np.array([1.5 + t]))
            if kind == "late":
                S.n_late_late += 1
            else:
                S.n_outside += 1
    for u in S.unowned:  # rows and columns nobody owns: ignored by the scatter
        cols = rng.choice(n, size=min(n, 3), replace=False)
        I.append(np.full(cols.size, u)); Jc.append(cols); V.append(vector(cols.size, [seed, 3, int(u)]))
        I.append(cols); Jc.append(np.full(cols.size, u)); V.append(vector(cols.size, [seed, 4, int(u)]))
    I = np.concatenate(I) if I else np.zeros(0, dtype=np.int64)
    Jc = np.concatenate(Jc) if Jc else np.zeros(0, dtype=np.int64)
    V = np.concatenate(V) if V else np.zeros(0)
    _, first = np.unique(I.astype(np.int64) * n + Jc, return_index=True)  # an entry met twice (a copy's diagonal block) is kept once
    I, Jc, V = I[first], Jc[first], V[first]
    S.rp = np.concatenate([[0], np.cumsum(np.bincount(I, minlength=n))]).astype(np.int64)
    S.ci, S.val = Jc.astype(np.int32), np.ascontiguousarray(V, dtype=np.float64)
    return S


# ---- the kernels, restated ----------------------------------------------------------------------------------------------------------
def scatter(S, transpose=0, diagScale=1.0, exLo=0, exHi=0, end=1 << 62, dtype=LD, ignore_transpose=False, shift_in_window=False):
    """k_bilu_scatter + k_bilu_pad_diag: (blocks (nnzB, 8, 8), dropped).  The two flags are the mutations of the CPU tier."""
    bval = np.zeros((int(S.bptr[-1]), NB, NB), dtype=dtype)
    dropped = 0
    rows = np.repeat(np.arange(S.n), np.diff(S.rp))
    for un, us in S.maps:
        for row, j, v in zip(rows, S.ci, S.val):
            I0, J0 = un[row], un[j]
            if I0 < 0 or J0 < 0:
                continue
            tr = transpose and not ignore_transpose
            I, J, r, c = (J0, I0, us[j], us[row]) if tr else (I0, J0, us[row], us[j])
            e = S.find(I, J)
            if e < 0:
                dropped += 0 if (S.late[I] and S.late[J]) else 1
                continue
            shifted = row < end and (shift_in_window or not (exLo <= row < exHi))
            bval[e, r, c] = dtype(v) * dtype(diagScale) if (j == row and shifted) else dtype(v)
    for p in range(S.nN):
        for k in range(NB):
            if S.nodeUnk[p, k] < 0:
                bval[S.bdiag[p], k, k] = 1.0
    return bval, dropped


def inverse8(a, dtype=LD, pivot=True, flip_shift=False):
    """bilu_inverse8: Gauss-Jordan with row pivoting; a pivot with |pv| <= 1e-300 (or NaN) becomes +-1e-12, - only for pv < 0"""
    a = np.array(a, dtype=dtype)
    b = np.eye(NB, dtype=dtype)
    nshift = 0
    for k in range(NB):
        pr = k + int(np.argmax(np.abs(a[k:, k]))) if pivot else k
        a[[k, pr]], b[[k, pr]] = a[[pr, k]], b[[pr, k]]
        pv = a[k, k]
        if not abs(pv) > 1e-300:
            pv = dtype(-1e-12 if (pv < 0) != flip_shift else 1e-12)
            a[k, k] = pv
            nshift += 1
        rk, rkb = a[k] / pv, b[k] / pv
        f = a[:, k].copy()
        f[k] = 0
        a, b = a - np.outer(f, rk), b - np.outer(f, rkb)
        a[k], b[k] = rk, rkb
    return b, nshift


def factor(S, bval, dtype=LD, **inv_args):
    """k_bilu_factor level by level = row by row in processing order: (blocks with L, D, U in place, invD, nshift, kappa of every D)"""
    bval = np.array(bval, dtype=dtype)
    invD = np.zeros((S.nN, NB, NB), dtype=dtype)
    nshift, kappa = 0, np.zeros(S.nN)
    for p in range(S.nN):
        for e in range(int(S.bptr[p]), int(S.bdiag[p])):
            J = int(S.bcol[e])
            bval[e] = bval[e] @ invD[J]
            for f in range(int(S.bdiag[J]) + 1, int(S.bptr[J + 1])):
                pos = S.find(p, int(S.bcol[f]))
                if pos >= 0:
                    bval[pos] -= bval[e] @ bval[f]
        D = bval[S.bdiag[p]]
        invD[p], ns = inverse8(D, dtype, **inv_args)
        nshift += ns
        kappa[p] = float(np.abs(D).sum(axis=1).max() * np.abs(invD[p]).sum(axis=1).max())
    return bval, invD, nshift, kappa


def assert_tame(kappa, skip=()):
    k = np.delete(kappa, list(skip))
    assert k.size == 0 or k.max() <= KAPPA_CAP, f"kappa_inf of a diagonal block {k.max():.3g} above the cap {KAPPA_CAP}"


def stream_ptrs(S):
    Lptr = np.concatenate([[0], np.cumsum([S.nL(p) for p in range(S.nN)])]).astype(np.int64)
    Uptr = np.concatenate([[0], np.cumsum([S.nU(S.nN - 1 - q) for q in range(S.nN)])]).astype(np.int64)
    return Lptr, Uptr


def pack_row(blks):
    """(nE, 8, 8) -> the packed stream of the row: passes of nb <= 8 blocks, inside a pass [qq][g][k][2], row r = 2 qq + rr"""
    out = []
    for a0 in range(0, len(blks), NB):
        sub = blks[a0 : a0 + NB]
        out.append(sub.reshape(len(sub), 4, 2, NB).transpose(1, 0, 3, 2).ravel())
    return np.concatenate(out) if out else np.zeros(0, dtype=blks.dtype)


def unpack_row(flat, nE):
    out = np.zeros((nE, NB, NB), dtype=flat.dtype)
    for a0 in range(0, nE, NB):
        nb = min(NB, nE - a0)
        out[a0 : a0 + nb] = flat[a0 * 64 : (a0 + nb) * 64].reshape(4, nb, NB, 2).transpose(1, 0, 3, 2).reshape(nb, NB, NB)
    return out


class Factor:
    """what das_debug_bilu_factor returns"""


def pack(S, bval, invD, nshift=0, dtype=np.float64):
    """k_bilu_pack<dtype>"""
    F = Factor()
    F.Lptr, F.Uptr = stream_ptrs(S)
    F.Lcol = np.concatenate([S.row(p)[: S.nL(p)] for p in range(S.nN)]).astype(np.int32)
    F.Ucol = np.concatenate([S.row(p)[S.nL(p) + 1 :] for p in range(S.nN - 1, -1, -1)]).astype(np.int32)
    b = np.asarray(bval).astype(dtype)
    F.Lval = np.concatenate([pack_row(b[S.bptr[p] : S.bdiag[p]]) for p in range(S.nN)] + [np.zeros(0, dtype=dtype)])
    F.Uval = np.concatenate([pack_row(b[S.bdiag[p] + 1 : S.bptr[p + 1]]) for p in range(S.nN - 1, -1, -1)] + [np.zeros(0, dtype=dtype)])
    F.invD, F.nshift = np.asarray(invD).astype(np.float64).reshape(-1), nshift
    return F


def decode(S, F):
    """the stored factor back in the block layout of the structure (diagonal blocks left zero), widened to longdouble; the pointers
    and columns must be exactly those the structure implies"""
    Lptr, Uptr = stream_ptrs(S)
    assert np.array_equal(F.Lptr, Lptr) and np.array_equal(F.Uptr, Uptr), "Lptr / Uptr"
    assert np.array_equal(F.Lcol, np.concatenate([S.row(p)[: S.nL(p)] for p in range(S.nN)])), "Lcol"
    assert np.array_equal(F.Ucol, np.concatenate([S.row(p)[S.nL(p) + 1 :] for p in range(S.nN - 1, -1, -1)])), "Ucol"
    bval = np.zeros((int(S.bptr[-1]), NB, NB), dtype=LD)
    for p in range(S.nN):
        q = S.nN - 1 - p
        bval[S.bptr[p] : S.bdiag[p]] = unpack_row(F.Lval[Lptr[p] * 64 : Lptr[p + 1] * 64], S.nL(p))
        bval[S.bdiag[p] + 1 : S.bptr[p + 1]] = unpack_row(F.Uval[Uptr[q] * 64 : Uptr[q + 1] * 64], S.nU(p))
    return bval, F.invD.reshape(S.nN, NB, NB).astype(LD)


def rhs(S, nrhs, seed):
    return np.stack([vector(S.n, [seed, r]) for r in range(nrhs)])


def sweeps(S, bval, invD, B, dtype=LD):
    """k_bilu_sweep / k_bilu_sweep_m: y, z (nN, 8, nrhs) and out (nrhs, n) with the sentinel where nothing is written"""
    nrhs = B.shape[0]
    y, z = np.zeros((S.nN, NB, nrhs), dtype=dtype), np.zeros((S.nN, NB, nrhs), dtype=dtype)
    bp = np.where(S.nodeUnk[:, :, None] >= 0, B.T[np.maximum(S.nodeUnk, 0)], 0.0).astype(dtype)
    for p in range(S.nN):
        acc = np.zeros((NB, nrhs), dtype=dtype)
        for e in range(int(S.bptr[p]), int(S.bdiag[p])):
            acc += bval[e].astype(dtype) @ y[S.bcol[e]]
        y[p] = bp[p] - acc
    for p in range(S.nN - 1, -1, -1):
        acc = np.zeros((NB, nrhs), dtype=dtype)
        for e in range(int(S.bdiag[p]) + 1, int(S.bptr[p + 1])):
            acc += bval[e].astype(dtype) @ z[S.bcol[e]]
        z[p] = invD[p].astype(dtype) @ (y[p] - acc)
    out = np.full((nrhs, S.n), SENTINEL)
    m = S.nodeOut >= 0
    out[:, S.nodeOut[m]] = z[m].astype(np.float64).T
    return y, z, out


# ---- comparison: each returns (ok, achieved max err / bound) ------------------------------------------------------------------------
def _judge(err, bound, got):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    ok = bool(np.all(np.isfinite(np.asarray(got, dtype=np.float64))) and np.all(err <= bound))
    return ok, float(np.max(r)) if np.size(r) else 0.0


def _merge(results):
    return all(r[0] for r in results), max([r[1] for r in results], default=0.0)


def check_factor(S, A, F, nodes=None):
    """every L and U block and every inverse of the nodes (default: all) against the stored blocks they were made of.  A: the
    blocks of the reference scatter.  Returns {"L": (ok, ratio), "U": ..., "invD": ...}"""
    bv, invD = decode(S, F)
    A = np.asarray(A, dtype=LD)
    res = {"L": [], "U": [], "invD": []}
    for p in (range(S.nN) if nodes is None else nodes):
        for e in range(int(S.bptr[p]), int(S.bptr[p + 1])):
            J = int(S.bcol[e])
            acc, mag, cnt = A[e].copy(), np.abs(A[e]), 0
            for e2 in range(int(S.bptr[p]), min(e, int(S.bdiag[p]))):  # common M < min(J, p): L_pM stored, U_MJ stored
                f = S.find(int(S.bcol[e2]), J)
                if f >= 0:
                    acc -= bv[e2] @ bv[f]
                    mag += np.abs(bv[e2]) @ np.abs(bv[f])
                    cnt += 1
            T = NB * cnt + 1
            if J < p:
                ref, bound = acc @ invD[J], LD((T + 10) * U) * (mag @ np.abs(invD[J]))
                res["L"].append(_judge(np.abs(bv[e] - ref), bound, bv[e]))
            elif J > p:
                res["U"].append(_judge(np.abs(bv[e] - acc), LD((T + 10) * U) * mag, bv[e]))
            else:
                ref, _ = inverse8(acc, LD)
                ninv = np.abs(ref).sum(axis=1).max()
                kap = np.abs(acc).sum(axis=1).max() * ninv
                bound = LD(NB ** 3 * U) * kap * ninv + np.abs(ref) @ (LD((T + 10) * U) * mag) @ np.abs(ref)
                res["invD"].append(_judge(np.abs(invD[p] - ref), bound, invD[p]))
    return {k: _merge(v) for k, v in res.items()}


def check_shifted_inverse(D, invD):
    """The inverse of a block whose last row is exactly singular (make(singular=...); the node has no predecessors, so D = A_pp is
    exact).  The row is never a multiplier, so the kernel inverts D_s = D with D[7, 7] = +-1e-12 (- only below zero) = R D', R =
    diag(1, ..., 1, 1e-12): the row scaling only scales column 7 of the inverse, inv(D_s) = inv(D') inv(R).  The bound of an ordinary
    block, 8^3 u kappa_inf(D') ||inv(D')||_inf, therefore holds column by column with column 7 scaled by 1e12; taken with kappa(D_s) it
    would be 1e12 times wider on every column and could not tell the sign of the shift."""
    D = np.asarray(D, dtype=LD)
    assert not np.abs(D[7, :7]).any() and abs(D[7, 7]) <= 1e-300
    ref, ns = inverse8(D, LD)
    R = np.ones(NB, dtype=LD)
    R[7] = LD(1e-12)
    Dp = D.copy()
    Dp[7, 7] = -1.0 if D[7, 7] < 0 else 1.0
    ninv = np.abs(ref * R[None, :]).sum(axis=1).max()
    bound = LD(NB ** 3 * U) * np.abs(Dp).sum(axis=1).max() * ninv * ninv / R[None, :] * np.ones((NB, 1), dtype=LD)
    invD = np.asarray(invD, dtype=np.float64).astype(LD)
    return _judge(np.abs(invD - ref), bound, invD)


def check_sweeps(S, F, B, y, z, nodes=None):
    """y, z (nN, 8, nrhs) as stored by the device against the stored factor and the stored values of the dependencies.
    Returns {"y": (ok, ratio), "z": ...}"""
    bv, invD = decode(S, F)
    y, z = np.asarray(y, dtype=np.float64).astype(LD), np.asarray(z, dtype=np.float64).astype(LD)
    bp = np.where(S.nodeUnk[:, :, None] >= 0, B.T[np.maximum(S.nodeUnk, 0)], 0.0).astype(LD)
    res = {"y": [], "z": []}
    for p in (range(S.nN) if nodes is None else nodes):
        acc, mag = np.zeros_like(y[p]), np.zeros_like(y[p])
        for e in range(int(S.bptr[p]), int(S.bdiag[p])):
            acc += bv[e] @ y[S.bcol[e]]
            mag += np.abs(bv[e]) @ np.abs(y[S.bcol[e]])
        T = NB * S.nL(p) + 1
        res["y"].append(_judge(np.abs(y[p] - (bp[p] - acc)), LD((T + 1) * U) * (np.abs(bp[p]) + mag), y[p]))
        acc, mag = np.zeros_like(y[p]), np.zeros_like(y[p])
        for e in range(int(S.bdiag[p]) + 1, int(S.bptr[p + 1])):
            acc += bv[e] @ z[S.bcol[e]]
            mag += np.abs(bv[e]) @ np.abs(z[S.bcol[e]])
        T = NB * S.nU(p) + 1
        res["z"].append(_judge(np.abs(z[p] - invD[p] @ (y[p] - acc)), LD((T + 10) * U) * (np.abs(invD[p]) @ (np.abs(y[p]) + mag)), z[p]))
    return {k: _merge(v) for k, v in res.items()}


def check_out(S, z, out):
    """out (nrhs, ld): out[nodeOut] == z bitwise, every other entry still the sentinel"""
    want = np.full(out.shape, SENTINEL)
    m = S.nodeOut >= 0
    want[:, S.nodeOut[m]] = np.asarray(z, dtype=np.float64)[m].T
    return want.tobytes() == np.ascontiguousarray(out).tobytes()


def check_fp32(F64, F32):
    """the float factor is the rounded double factor, block for block in place; columns, pointers and invD identical"""
    return bool(F32.Lval.dtype == np.float32 and F32.Uval.dtype == np.float32
                and F32.Lval.tobytes() == F64.Lval.astype(np.float32).tobytes() and F32.Uval.tobytes() == F64.Uval.astype(np.float32).tobytes()
                and all(np.array_equal(getattr(F32, k), getattr(F64, k)) for k in ("Lptr", "Uptr", "Lcol", "Ucol"))
                and F32.invD.tobytes() == F64.invD.tobytes() and F32.nshift == F64.nshift)


def relerr(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), LD(1e-300)))


def downstream(S, bad):
    """nodes whose factor row, y or z depend on a node of `bad` (themselves included): (factor / y, z)"""
    fy = np.zeros(S.nN, dtype=bool)
    fy[list(bad)] = True
    for p in range(S.nN):
        fy[p] |= fy[S.row(p)[: S.nL(p)]].any()
    fz = fy.copy()
    for p in range(S.nN - 1, -1, -1):
        fz[p] |= fz[S.row(p)[S.nL(p) + 1 :]].any()
    return fy, fz


def owned(S):
    """mask of the entries of a vector of unknowns that some nodeOut names"""
    m = np.zeros(S.n, dtype=bool)
    m[S.nodeOut[S.nodeOut >= 0]] = True
    return m


# ---- the C-ABI input ----------------------------------------------------------------------------------------------------------------
def c_input(S, capi, fp32=0, transpose=0, diagScale=1.0, exLo=0, exHi=0, end=1 << 62, **override):
    """das_bilu_debug_t of the structure (returns (struct, keep-alive list)); override: replacement arrays / scalars by field name"""
    a = dict(nodeUnk=np.ascontiguousarray(S.nodeUnk.reshape(-1), dtype=np.int32),
             nodeOut=np.ascontiguousarray(S.nodeOut.reshape(-1), dtype=np.int32) if S.has_copies else None,
             late=np.ascontiguousarray(S.late, dtype=np.uint8), bptr=np.ascontiguousarray(S.bptr, dtype=np.int64),
             bdiag=np.ascontiguousarray(S.bdiag, dtype=np.int64), bcol=np.ascontiguousarray(S.bcol, dtype=np.int32),
             lvlPtr=np.ascontiguousarray(S.lvlPtr, dtype=np.int32),
             unkNode=np.ascontiguousarray(np.concatenate([m[0] for m in S.maps]), dtype=np.int32),
             unkSlot=np.ascontiguousarray(np.concatenate([m[1] for m in S.maps]), dtype=np.uint8),
             rp=np.ascontiguousarray(S.rp, dtype=np.int64), ci=np.ascontiguousarray(S.ci, dtype=np.int32), val=np.ascontiguousarray(S.val, dtype=np.float64))
    sc = dict(nNodes=S.nN, nLevels=len(S.lvlPtr) - 1, nMaps=len(S.maps), fp32=fp32, transpose=transpose, n=S.n, An=S.n, diagScale=diagScale,
              shiftExLo=exLo, shiftExHi=exHi, shiftEnd=end)
    for k, v in override.items():
        (a if k in a else sc)[k] = v
    d = capi.das_bilu_debug_t()
    for k, v in sc.items():
        setattr(d, k, v)
    types = dict(d._fields_)
    for k, v in a.items():
        setattr(d, k, v.ctypes.data_as(types[k]) if v is not None else None)
    return d, a


def bad_inputs(S3):
    """(name, override) of every structure das_debug_bilu_* must refuse with DAS_ERR_ARG; S3: make([[], [0], [0, 1]], ...), 3 nodes, all coupled"""
    assert S3.nN == 3 and S3.bptr[-1] == 9
    i32, i64 = (lambda *x: np.array(x, dtype=np.int32)), (lambda *x: np.array(x, dtype=np.int64))

    def changed(a, k, v):
        a = a.copy().reshape(-1)
        a[k] = v
        return a

    out = [("bptr not monotone", dict(bptr=i64(0, 6, 3, 9))),
           ("bptr[0] not 0", dict(bptr=i64(1, 3, 6, 9))),
           ("columns not ascending", dict(bcol=i32(0, 2, 1, 0, 1, 2, 0, 1, 2))),
           ("column out of range", dict(bcol=i32(0, 1, 3, 0, 1, 2, 0, 1, 2))),
           ("negative column", dict(bcol=i32(-1, 1, 2, 0, 1, 2, 0, 1, 2))),
           ("diagonal not at bdiag", dict(bdiag=i64(0, 3, 8))),
           ("bdiag outside its row", dict(bdiag=i64(0, 4, 9))),
           ("pattern not symmetric", dict(bptr=i64(0, 3, 6, 8), bcol=i32(0, 1, 2, 0, 1, 2, 1, 2), bdiag=i64(0, 4, 7))),
           ("lvlPtr does not reach nNodes", dict(lvlPtr=i32(0, 1, 2, 2))),
           ("lvlPtr does not start at 0", dict(lvlPtr=i32(1, 1, 2, 3))),
           ("lvlPtr decreases", dict(lvlPtr=i32(0, 2, 1, 3))),
           ("coupled nodes in one level", dict(lvlPtr=i32(0, 2, 3), nLevels=2)),
           ("slot index 8", dict(unkSlot=changed(S3.maps[0][1], 0, 8))),
           ("unkNode = nNodes", dict(unkNode=changed(S3.maps[0][0], 0, 3))),
           ("unkNode below -1", dict(unkNode=changed(S3.maps[0][0], 0, -2))),
           ("CSR column = An", dict(ci=changed(S3.ci, 0, S3.n))),
           ("negative CSR column", dict(ci=changed(S3.ci, 0, -1))),
           ("rowptr decreases", dict(rp=changed(S3.rp, 1, S3.rp[2] + 1))),
           ("unknown = n", dict(nodeUnk=changed(S3.nodeUnk, 0, S3.n))),
           ("nodeOut = n", dict(nodeOut=changed(S3.nodeOut, 0, S3.n))),
           ("An above n", dict(n=S3.n - 1)),
           ("no nodes", dict(nNodes=0)), ("no levels", dict(nLevels=0)), ("no maps", dict(nMaps=0)), ("fp32 = 2", dict(fp32=2))]
    out += [(f"null {k}", {k: None}) for k in ("nodeUnk", "late", "bptr", "bdiag", "bcol", "lvlPtr", "unkNode", "unkSlot", "rp", "ci", "val")]
    return out

"""CPU tier of tests/color_reference.py: the restatements of the colouring against INDEPENDENT ones (a dense boolean conflict matrix
and linear scans; the host library's serial sweep on a mesh), the generators against what they promise, the speculative restatement
valid and within 1000 rounds on every generator, every named wrong result rejected - so that a pass of
tests/test_gpu_color_kernels.py means something - and every invalid input refused by the entries das_debug_color_* with DAS_ERR_ARG
before anything is launched (these run without a device)."""
import ctypes as C

import numpy as np
import pytest

import color_reference as cr
import graph_reference as gr
from common import options
from dafoam_amd import _capi

ARG = -1  # DAS_ERR_ARG


# ---- the restatements against independent ones -----------------------------------------------------------------------------------
def dense_conflicts(n, rp, ci, keep):
    D = np.zeros((len(keep), n), dtype=bool)
    for q, r in enumerate(keep):
        D[q, ci[rp[r]:rp[r + 1]]] = True
    A = (D.astype(np.int32).T @ D.astype(np.int32)) > 0
    np.fill_diagonal(A, False)
    return A


def brute_firstfit(A):
    colors = np.full(len(A), -1)
    for j in range(len(A)):
        taken = set(colors[:j][A[j, :j]])
        colors[j] = min(c for c in range(len(A) + 1) if c not in taken)
    return colors


def brute_speculative(A, S, W):
    """the rule on the conflict matrix, colours searched by linear scans; None on overflow"""
    n = len(A)
    colors, rnd = np.full(n, -1), 0
    while np.any(colors < 0):
        tent = np.full(n, -1)
        for j in np.flatnonzero(colors < 0):
            taken = set(colors[A[j] & (colors >= 0)])
            start = cr.spec_hash(int(j), rnd) % S
            order = list(range(start, S)) + list(range(0, start)) + list(range(S, 64 * W))
            pick = [c for c in order if c not in taken][:1]
            if not pick:
                return None
            tent[j] = pick[0]
        open_ = colors < 0
        for j in np.flatnonzero(open_):
            rivals = A[j, :j] & open_[:j] & (tent[:j] == tent[j])
            if not np.any(rivals):
                colors[j] = tent[j]
        rnd += 1
    return colors, rnd


@pytest.mark.parametrize("name", ["groups", "crowded", "by_net_count", "width10"])
def test_first_fit_against_a_dense_boolean_matrix(name):
    n, rp, ci, keep = cr.pattern(name)
    assert np.array_equal(cr.firstfit_of(name), brute_firstfit(dense_conflicts(n, rp, ci, keep)))
    assert cr.valid(rp, ci, keep, cr.firstfit_of(name))


@pytest.mark.parametrize("name,S", [("groups", None), ("crowded", None), ("crowded", 8), ("crowded", 64), ("by_net_count", None), ("width10", None)])
def test_speculative_against_a_dense_boolean_matrix(name, S):
    n, rp, ci, keep = cr.pattern(name)
    colors, rounds, W, _ = cr.speculative_of(name, S)
    S = cr.spread_rule(rp, keep) if S is None else S
    assert W == cr.width_rule(S)
    got = brute_speculative(dense_conflicts(n, rp, ci, keep), S, W)
    assert got is not None and np.array_equal(got[0], colors) and got[1] == rounds


def test_valid_against_a_dense_boolean_matrix():
    n, rp, ci, keep = cr.pattern("crowded")
    A = dense_conflicts(n, rp, ci, keep)
    rng = np.random.default_rng(0)
    good = cr.firstfit_of("crowded")
    seen = set()
    for trial in range(200):
        c = good.copy()
        if trial:
            c[rng.integers(0, n)] = rng.integers(-1, good.max() + 1)
        ok = bool(np.all(c >= 0)) and not np.any(A & (c[:, None] == c[None, :]))
        assert cr.valid(rp, ci, keep, c) == ok
        seen.add(ok)
    assert seen == {True, False}


def test_first_fit_is_the_host_librarys_serial_sweep_on_a_mesh():
    """all rows as nets: dominated rows add no constraint, so the library's kept rows give the same colours"""
    from dafoam_amd.meshgen import channel_case
    from dafoam_amd.pyDASolvers import pyDASolvers

    case = channel_case(6, 5, 4)
    s = pyDASolvers(b"DASimpleFoam -python", options(case, amd={"coloringOnDevice": 0}), case=case)
    s.runColoring()
    col, nc = s.getColoring()
    con = s.getConnectivity(0).tocsr()
    con.sort_indices()
    n = con.shape[0]
    rp, ci = con.indptr.astype(np.int64), con.indices.astype(np.int32)
    ref = cr.ref_firstfit(rp, ci, np.arange(n, dtype=np.int64))
    assert nc == ref.max() + 1 and np.array_equal(np.asarray(col, dtype=np.int32), ref)


# ---- the generators hold what they promise -------------------------------------------------------------------------------------------
def net_lengths(rp, keep):
    return np.diff(rp)[keep]


def net_counts(n, rp, ci, keep):
    return np.array([len(c) for c in cr.nets_of(rp, ci, keep)[1]])


@pytest.mark.parametrize("name", cr.PATTERNS + ["long_net"])
def test_generators_are_wellformed_and_small(name):
    n, rp, ci, keep = cr.pattern(name)
    assert len(rp) == n + 1 and rp[0] == 0 and rp[-1] == len(ci) and n <= 5000 and len(ci) <= 2e5
    assert rp.dtype == np.int64 and ci.dtype == np.int32 and keep.dtype == np.int64
    assert np.all(np.diff(ci)[np.diff(gr.rows_of(rp)) == 0] > 0), "the columns of a row do not ascend strictly"
    assert ci.min() >= 0 and ci.max() < n and len(set(keep.tolist())) == len(keep) >= 1 and keep.min() >= 0 and keep.max() < n


def test_generators_hold_the_named_cases():
    n, rp, ci, keep = cr.pattern("by_net_count")
    cnt = net_counts(n, rp, ci, keep)
    assert set(cr.COL_NETS) <= set(cnt.tolist()) and list(cnt[:3]) == [0, 0, 0] and cnt[-1] == 0 and len(keep) % 4 == 1
    assert set(gr.rows_of(rp).tolist()) - set(keep.tolist()), "no entry outside the kept rows"
    n, rp, ci, keep = cr.pattern("by_net_length")
    assert set(cr.NET_LENGTHS) == set(net_lengths(rp, keep).tolist()) and net_lengths(rp, keep)[-1] == 129 and len(keep) % 4 == 2
    # groups: runs of identical lists, cut at 8 by color_groups_from_flags; behind each a column that differs in one net
    n, rp, ci, keep, first = cr.groups()
    _, colnets = cr.nets_of(rp, ci, keep)
    for L, j0 in zip(cr.RUNS, first):
        assert all(colnets[j0 + i] == colnets[j0] for i in range(L)) and (j0 == 0 or colnets[j0 - 1] != colnets[j0])
        odd = colnets[j0 + L]
        assert len(odd) == len(colnets[j0]) and len(set(odd) ^ set(colnets[j0])) == 2
    assert len(keep) % 4 == 2
    for K in cr.CLIQUES:
        n, rp, ci, keep = cr.pattern(f"clique{K}")
        assert net_lengths(rp, keep).tolist() == [K, 2] and cr.firstfit_of(f"clique{K}").max() + 1 == K
    assert [cr.firstfit_width(cr.firstfit_of(f"clique{K}")) for K in cr.CLIQUES] == [8, 8, 16, 32]
    # the band: column j shares a net with j-1 .. j-3, so the dependency chain runs through every column
    n, rp, ci, keep = cr.pattern("chain")
    nets, colnets = cr.nets_of(rp, ci, keep)
    assert n == 2000 and len(keep) % 4 == 1
    for j in range(1, n):
        assert {i for q in colnets[j] for i in nets[q] if i < j} == set(range(max(0, j - 3), j))
    n, rp, ci, keep = cr.pattern("random")
    assert n == 3000 and 25 <= net_lengths(rp, keep).mean() <= 35 and len(keep) % 4
    # widths and spreads
    for name, S, W in [("width10", 312, 10), ("long_net", 2125, 67), ("by_net_length", 750, 24)]:
        n, rp, ci, keep = cr.pattern(name)
        assert cr.spread_rule(rp, keep) == S and cr.width_rule(S) == W
    assert {S for _, S in cr.SPREADS} >= {1, 8, 63, 64, 65, 127, 128, 129}
    for name, S in cr.SPREADS:
        colors, rounds, W, _ = cr.speculative_of(name, S)
        if name != "random":  # more colours than the spread offers; the clique of 513 overflows 8 words
            assert colors.max() >= S
        assert W == (16 if name == "clique513" else 8) and cr.width_rule(S) == 8
        n, rp, ci, keep = cr.pattern(name)
        starts = {cr.spec_hash(j, 0) % S for j in range(n)}
        assert S < 127 or {63, 64, 65} <= starts, "no start on either side of the first word boundary"


@pytest.mark.parametrize("name,S", [(p, None) for p in cr.PATTERNS + ["long_net"]] + cr.SPREADS)
def test_speculative_restatement_is_valid_and_needs_few_rounds(name, S):
    n, rp, ci, keep = cr.pattern(name)
    colors, rounds, W, states = cr.speculative_of(name, S)
    assert cr.valid(rp, ci, keep, colors) and rounds <= 1000 and len(states) == rounds and colors.max() < 64 * W
    assert cr.valid(rp, ci, keep, cr.firstfit_of(name))
    left = [int(np.sum(s < 0)) for s in states]
    assert all(a > b for a, b in zip([n] + left, left)), "a round that commits nothing"


# ---- named wrong results are rejected ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,swap", [("a hash with another constant", {"mul": 2654435769}), ("start ignored", {"use_start": False}),
                                       ("the higher index wins", {"winner": max}), ("a loser decided by its first net only", {"nets_checked": "first"})])
def test_wrong_speculative_rules_are_rejected(what, swap):
    hit = 0
    for name in ("by_net_count", "crowded", "width10", "groups"):
        n, rp, ci, keep = cr.pattern(name)
        nets, colnets = cr.nets_of(rp, ci, keep)
        S = cr.spread_rule(rp, keep)
        good = cr.ref_spec_round(nets, colnets, np.full(n, -1, dtype=np.int32), S, cr.width_rule(S), 0)
        bad = cr.ref_spec_round(nets, colnets, np.full(n, -1, dtype=np.int32), S, cr.width_rule(S), 0, dict(cr.RULE, **swap))
        assert not gr.same(good[2], bad[2]), (what, name)
        hit += 1
        if "first net" in what:  # such a round commits two columns of one net with one colour
            assert not cr.valid(rp, ci, keep, np.where(bad[2] < 0, np.arange(n) + 10000, bad[2]))
    assert hit == 4


def test_a_group_coloured_as_if_it_had_nine_members_is_rejected():
    """the kernel colours at most 8 members per group: a run of 9 left uncut has a ninth member that nothing colours"""
    n, rp, ci, keep, first = cr.groups()
    good = cr.firstfit_of("groups")
    for L in (9, 16, 17):
        bad = good.copy()
        bad[first[cr.RUNS.index(L)] + 8] = -1
        assert not gr.same(bad, good) and not cr.valid(rp, ci, keep, bad)
    # and members that take ONE colour as if they did not exclude each other
    bad = good.copy()
    j0 = first[cr.RUNS.index(9)]
    bad[j0 + 8] = bad[j0]
    assert not gr.same(bad, good) and not cr.valid(rp, ci, keep, bad)


def test_a_conflict_hidden_in_the_65th_column_of_a_net_is_rejected():
    n, rp, ci, keep = cr.pattern("by_net_length")
    for good in (cr.firstfit_of("by_net_length"), cr.speculative_of("by_net_length")[0]):
        for q in (7, len(keep) - 1):  # the net of 600 columns, the last one (129)
            cols = ci[rp[keep[q]]:rp[keep[q] + 1]]
            bad = good.copy()
            bad[cols[64]] = good[cols[3]]
            assert cr.valid(rp, ci, keep, good) and not cr.valid(rp, ci, keep, bad)


def test_netbits_restatement():
    n, rp, ci, keep = cr.pattern("width10")
    colors, rounds, W, states = cr.speculative_of("width10")
    nets, _ = cr.nets_of(rp, ci, keep)
    F = cr.ref_netbits(nets, states[0], W).reshape(len(keep), W)
    for q in range(len(keep)):
        bits = {w * 64 + b for w in range(W) for b in range(64) if (int(F[q, w]) >> b) & 1}
        assert bits == {int(states[0][j]) for j in nets[q] if states[0][j] >= 0}


# ---- the entries refuse invalid input before anything is launched ---------------------------------------------------------------------
def test_entries_refuse_invalid_input_before_any_launch():
    from test_graph_reference_cpu import bad_structures, small

    L = _capi.lib()
    n, rp, ci, _, _ = small()
    keep = np.array([3, 0], dtype=np.int64)
    colors = np.array([0, 1, -1, 2, 511], dtype=np.int32)

    def calls(n=n, rp=rp, ci=ci, keep=keep, nKeep=None, colors=colors, S=4, W=8, rnd=0, spread=-1, guard=5, f_guard=3):
        nk = len(keep) if nKeep is None else nKeep
        return [(b"das_debug_color_firstfit", lambda: cr.dev_firstfit(L, n, rp, ci, keep, nk, guard)[0]),
                (b"das_debug_color_speculative", lambda: cr.dev_speculative(L, n, rp, ci, keep, spread, nk, guard)[0]),
                (b"das_debug_color_spec_round", lambda: L.das_debug_color_spec_round(n, gr._ll(rp), gr._i(ci), nk, gr._ll(keep), gr._i(colors), S, W, rnd, gr._i(np.zeros(16, dtype=np.int32)),
                                                                             gr._u8(np.zeros(16, dtype=np.uint8)), gr._i(np.zeros(16, dtype=np.int32)), max(n, 0) + guard,
                                                                             cr._u64(np.zeros(4096, dtype=np.uint64)), max(nk, 0) * max(W, 0) + f_guard, C.byref(C.c_uint()),
                                                                             C.byref(C.c_int()))),
                (b"das_debug_color_check", lambda: L.das_debug_color_check(n, gr._ll(rp), gr._i(ci), nk, gr._ll(keep), gr._i(colors), W, C.byref(C.c_int())))]

    def refused(which, what, **kw):
        for who, call in calls(**kw):
            if which is None or any(w in who for w in which):
                rc = call()
                assert rc == ARG and who in L.das_last_error(), (who, what, rc, L.das_last_error())

    # what das_debug_graph_nets refuses
    for what, r, c in bad_structures(rp, ci, True) + [("no entries", np.zeros(n + 1, dtype=np.int64), ci)]:
        refused(None, what, rp=r, ci=c)
    refused(None, "n = 0", n=0)
    refused(None, "n < 0", n=-3)
    refused(None, "n = 2^31", n=2 ** 31)
    for what, k in [("kept row too large", np.array([3, 5], dtype=np.int64)), ("kept row negative", np.array([-1, 2], dtype=np.int64)),
                    ("kept row repeated", np.array([3, 0, 3], dtype=np.int64))]:
        refused(None, what, keep=k)
    for what, nk in [("nKeep = 0", 0), ("nKeep negative", -1), ("nKeep above n", 6)]:
        refused(None, what, keep=np.array([3, 0, 1, 2, 4, 4], dtype=np.int64), nKeep=nk)
    refused(None, "null keep", keep=None, nKeep=2)
    # colours, widths, spreads, rounds
    for what, c in [("colour 64 W", np.array([0, 1, 512, 2, 3], dtype=np.int32)), ("colour -2", np.array([0, -2, 1, 2, 3], dtype=np.int32)), ("null colours", None)]:
        refused([b"round", b"check"], what, colors=c)
    for W in (0, -1, 161, 1024, 2 ** 30):
        refused([b"round", b"check"], f"W = {W}", W=W, colors=np.zeros(5, dtype=np.int32))
    for S in (0, -1):
        refused([b"round"], f"S = {S}", S=S)
    refused([b"round"], "negative round", rnd=-1)
    for spread in (0, -2, 5121, 2 ** 30):
        refused([b"speculative"], f"spread = {spread}", spread=spread)
    # outputs too short or null
    refused([b"firstfit", b"speculative", b"round"], "outputs shorter than n", guard=-1)
    refused([b"round"], "F shorter than nKeep W", f_guard=-1)
    a = (n, gr._ll(rp), gr._i(ci), 2, gr._ll(keep))
    for who, call in [(b"das_debug_color_firstfit", lambda: L.das_debug_color_firstfit(*a, None, 5, None, None)),
                      (b"das_debug_color_speculative", lambda: L.das_debug_color_speculative(*a, -1, None, 5, None, None, None, None)),
                      (b"das_debug_color_spec_round", lambda: L.das_debug_color_spec_round(*a, gr._i(colors), 4, 8, 0, None, None, None, 5, None, 16, None, None)),
                      (b"das_debug_color_check", lambda: L.das_debug_color_check(*a, gr._i(colors), 8, None))]:
        assert call() == ARG and who in L.das_last_error(), (who, "null outputs")

"""The colouring kernels (dafoam_amd/csrc/das_color.hpp: k_color_firstfit, k_spec_assign, k_spec_conflict, k_spec_commit,
k_spec_netbits) restated in plain Python - sets, sorted lists and dictionaries; no bitmaps, no groups, no tickets, no lanes - the
generators of patterns that no mesh produces, and the wrappers of the entries das_debug_color_*.  Everything is integer arithmetic:
every comparison is EXACT.

  first-fit     columns in ascending order, each takes the smallest colour that no lower-numbered column sharing a kept row holds
  speculative   round by round: every uncoloured column j picks, with start = hash(j, round) % S, the first free colour in [start, S),
                else the first free colour below start, else the first free colour at or beyond S (none below 64 W: overflow - the width
                doubles and the whole run starts again); in every net, per colour, the lowest index among the tentative holders wins, and
                a column that loses in any one of its nets stays uncoloured; W = max(8, (2 S + 63) / 64), S = max(8, 1.25 x longest net)

Used by tests/test_gpu_color_kernels.py (kernels on the device) and tests/test_color_reference_cpu.py (the restatements against a dense
brute force and the host library, the generators against what they promise, named wrong results rejected, the argument checks)."""
import ctypes as C
import functools
from bisect import bisect_left

import numpy as np

import graph_reference as gr

M32 = 0xFFFFFFFF
RULE = {"mul": 2654435761, "use_start": True, "winner": min, "nets_checked": None}  # das_color.hpp; the CPU tier swaps one item at a time


# ---- the structure ---------------------------------------------------------------------------------------------------------------
def nets_of(rp, ci, keep):
    """(nets, colnets): the ascending columns of every kept row, and per column the tuple of the nets (positions in keep) that hold it,
    in the order of keep"""
    n = len(rp) - 1
    nets = [[int(c) for c in ci[rp[r]:rp[r + 1]]] for r in keep]
    colnets = [[] for _ in range(n)]
    for q, cols in enumerate(nets):
        for j in cols:
            colnets[j].append(q)
    return nets, [tuple(c) for c in colnets]


def valid(rp, ci, keep, colors):
    """brute force: no kept row holds two columns of one colour, no column is left without one"""
    if len(colors) != len(rp) - 1 or any(int(c) < 0 for c in colors):
        return False
    for r in keep:
        seen = set()
        for j in ci[rp[r]:rp[r + 1]]:
            if int(colors[j]) in seen:
                return False
            seen.add(int(colors[j]))
    return True


# ---- first-fit --------------------------------------------------------------------------------------------------------------------
def ref_firstfit(rp, ci, keep):
    nets, colnets = nets_of(rp, ci, keep)
    colors = []
    for j in range(len(rp) - 1):
        taken = set()
        for q in colnets[j]:
            for i in nets[q]:
                if i >= j:
                    break
                taken.add(colors[i])
        c = 0
        while c in taken:
            c += 1
        colors.append(c)
    return np.array(colors, dtype=np.int32)


def firstfit_width(colors):
    """the bitmap words of the first-fit run that holds these colours: 8, doubled while a colour lies at or beyond 64 W"""
    W = 8
    while int(np.max(colors)) >= 64 * W:
        W *= 2
    return W


# ---- speculative rounds -----------------------------------------------------------------------------------------------------------
def spec_hash(j, rnd, mul=RULE["mul"]):
    x = (j * mul + rnd * 40503) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def spread_rule(rp, keep):
    longest = max([int(rp[r + 1] - rp[r]) for r in keep] + [0])
    return max(8, longest + longest // 4)


def width_rule(S):
    return max(8, (2 * S + 63) // 64)


def ref_spec_round(nets, colnets, colors, S, W, rnd, rule=RULE):
    """one round from the final colours `colors` (-1 = none).  -> (tent, lose, colours after the commit, left, overflow)"""
    n, cap = len(colnets), 64 * W
    held = [{int(colors[j]) for j in cols if colors[j] >= 0} for cols in nets]
    tent = np.full(n, -1, dtype=np.int32)
    overflow = False
    free_of = {}  # columns with the same nets see the same free colours: computed once per round
    for j in range(n):
        if colors[j] >= 0:
            continue
        free = free_of.get(colnets[j])
        if free is None:
            taken = set().union(*[held[q] for q in colnets[j]])
            free = free_of[colnets[j]] = [c for c in range(cap) if c not in taken]
        start = spec_hash(j, rnd, rule["mul"]) % S if rule["use_start"] else 0
        i = bisect_left(free, start)
        if i < len(free) and free[i] < S:
            tent[j] = free[i]
        elif i > 0:
            tent[j] = free[0]
        elif i < len(free):
            tent[j] = free[i]
        else:
            overflow = True
    lose = np.zeros(n, dtype=np.uint8)
    for q, cols in enumerate(nets):
        holders = {}
        for j in cols:
            if colors[j] < 0 and tent[j] >= 0:
                holders.setdefault(int(tent[j]), []).append(j)
        for c, js in holders.items():
            for j in js:
                if j != rule["winner"](js) and (rule["nets_checked"] is None or q == colnets[j][0]):
                    lose[j] = 1
    out = np.array(colors, dtype=np.int32)
    won = (out < 0) & (tent >= 0) & (lose == 0)
    out[won] = tent[won]
    return tent, lose, out, int(np.sum(out < 0)), overflow


def ref_netbits(nets, colors, W):
    """what k_spec_netbits leaves: per net the set of the final colours of its columns as W words of 64 bits"""
    F = np.zeros((len(nets), W), dtype=np.uint64)
    for q, cols in enumerate(nets):
        for j in cols:
            if colors[j] >= 0:
                F[q, colors[j] // 64] |= np.uint64(1 << (int(colors[j]) % 64))
    return F.reshape(-1)


def ref_speculative(rp, ci, keep, S=None, rule=RULE, states=None):
    """-> (colours, rounds, W); states (a list) receives the colours after every round of the run that succeeded"""
    nets, colnets = nets_of(rp, ci, keep)
    S = spread_rule(rp, keep) if S is None else S
    W = width_rule(S)
    while True:
        colors, rnd, left = np.full(len(rp) - 1, -1, dtype=np.int32), 0, 1
        if states is not None:
            del states[:]
        while left:
            _, _, colors, left, overflow = ref_spec_round(nets, colnets, colors, S, W, rnd, rule)
            rnd += 1
            if overflow:
                break
            if states is not None:
                states.append(colors)
        if not overflow:
            return colors, rnd, W
        W *= 2


# ---- generators: (n, rowptr, col, keep) -------------------------------------------------------------------------------------------
COL_NETS = [0, 1, 63, 64, 65, 130]
NET_LENGTHS = [1, 63, 64, 65, 129, 600]
RUNS = [1, 2, 3, 7, 8, 9, 16, 17]
CLIQUES = [511, 512, 513, 1025]


def _keep(k):
    return np.arange(k, dtype=np.int64)


def by_net_count(seed=11):
    """n = 211, kept rows 0 .. 200 (201 = 4 x 50 + 1): columns of 0, 1, 63, 64, 65 and 130 nets, three neighbouring columns without a
    net in front and one at the end, entries in rows that are not kept"""
    n, nK = 211, 201
    rng = np.random.default_rng(seed)
    col_rows = []
    for j in range(n):
        cnt = 0 if j < 3 or j == n - 1 else COL_NETS[j % len(COL_NETS)]
        rows = list(np.sort(rng.choice(nK, size=cnt, replace=False)))
        if j % 5 == 0:
            rows.append(nK + j % (n - nK))
        col_rows.append(rows)
    rp, ci = gr.pattern_from_columns(n, col_rows)
    return n, rp, ci, _keep(nK)


def by_net_length(seed=12):
    """n = 700, 42 kept rows (4 x 10 + 2) of 1, 63, 64, 65 and 129 columns in turn, one of 600, the LAST one of 129; rows 42 .. are not
    kept"""
    n, nK = 700, 42
    rng = np.random.default_rng(seed)
    lens = [NET_LENGTHS[q % 5] for q in range(nK)]
    lens[7], lens[nK - 1] = 600, 129
    rows = [np.sort(rng.choice(n, size=L, replace=False)) for L in lens] + [np.sort(rng.choice(n, size=9, replace=False)) for _ in range(nK, 60)]
    rows += [np.zeros(0, dtype=np.int64)] * (n - len(rows))
    rp = gr.ref_scan([len(r) for r in rows])
    return n, rp, np.concatenate(rows).astype(np.int32), _keep(nK)


def groups(seed=13):
    """runs of 1, 2, 3, 7, 8, 9, 16 and 17 neighbouring columns with one net list each; behind every run a column whose list differs
    from the run's in its last net only.  n = 75, kept rows 0 .. 69 (4 x 17 + 2).  -> (..., first column of every run)"""
    n, nK = 75, 70
    rng = np.random.default_rng(seed)
    col_rows, first = [], []
    for L in RUNS:
        A = np.sort(rng.choice(nK - 1, size=5, replace=False))
        first.append(len(col_rows))
        col_rows += [A] * L + [np.append(A[:-1], nK - 1)]
    col_rows += [np.sort(rng.choice(n, size=4, replace=False)) for _ in range(n - len(col_rows))]
    rp, ci = gr.pattern_from_columns(n, col_rows)
    return n, rp, ci, _keep(nK), first


def clique(K):
    """one net of the columns 0 .. K-1 (exactly K colours), one of the two columns behind them; row 2 is not kept"""
    n = K + 2
    rows = [np.arange(K), np.array([K, K + 1]), np.array([0, K])] + [np.zeros(0, dtype=np.int64)] * (n - 3)
    return n, gr.ref_scan([len(r) for r in rows]), np.concatenate(rows).astype(np.int32), _keep(2)


def chain(n=2000):
    """net r = the columns r .. r+3: column j shares a net with j-1 .. j-3 and waits for them - dependency depth n; 1997 nets"""
    rows = [np.arange(r, r + 4) for r in range(n - 3)] + [np.zeros(0, dtype=np.int64)] * 3
    return n, gr.ref_scan([len(r) for r in rows]), np.concatenate(rows).astype(np.int32), _keep(n - 3)


def random_sparse(seed=14):
    """n = 3000, rows of 20 .. 40 random columns, two of three rows kept (1999 nets)"""
    n = 3000
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, size=int(rng.integers(20, 41)), replace=False)) for _ in range(n)]
    keep = np.array([r for r in range(n - 2) if r % 3], dtype=np.int64)
    return n, gr.ref_scan([len(r) for r in rows]), np.concatenate(rows).astype(np.int32), keep


def width10(seed=15):
    """a longest net of 250 columns: S = 312, W = 10 - of the 8 lanes of a column in k_spec_assign two own two words, six own one.
    n = 400, 31 nets"""
    n = 400
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, size=250, replace=False))] + [np.sort(rng.choice(n, size=40, replace=False)) for _ in range(30)]
    rows += [np.zeros(0, dtype=np.int64)] * (n - len(rows))
    return n, gr.ref_scan([len(r) for r in rows]), np.concatenate(rows).astype(np.int32), _keep(31)


def crowded(seed=16):
    """a net of 100 columns and 21 of 30 over n = 160: more colours than a forced spread of 1, 8, 63, 64 or 65 offers, so that the
    columns run out of [0, S)"""
    n = 160
    rng = np.random.default_rng(seed)
    rows = [np.arange(30, 130)] + [np.sort(rng.choice(n, size=30, replace=False)) for _ in range(21)]
    rows += [np.zeros(0, dtype=np.int64)] * (n - len(rows))
    return n, gr.ref_scan([len(r) for r in rows]), np.concatenate(rows).astype(np.int32), _keep(22)


def long_net():
    """one net of 1700 columns: S = 2125, W = 67 - more than 64 KiB of LDS in k_spec_conflict"""
    return clique(1700)


@functools.lru_cache(maxsize=None)
def pattern(name):
    """every generator by name, groups() without its list of runs"""
    if name.startswith("clique"):
        return clique(int(name[6:]))
    return {"by_net_count": by_net_count, "by_net_length": by_net_length, "groups": lambda: groups()[:4], "chain": chain, "random": random_sparse,
            "width10": width10, "crowded": crowded, "long_net": long_net}[name]()


PATTERNS = ["by_net_count", "by_net_length", "groups"] + [f"clique{K}" for K in CLIQUES] + ["chain", "random", "width10", "crowded"]
# (pattern, forced spread): more colours than S (the branch "[0, S) is full"), widening on overflow (a clique of 513 with 8 words), starts
# on both sides of a word boundary
SPREADS = [("crowded", S) for S in (1, 8, 63, 64, 65)] + [("clique513", 1), ("clique513", 65)] + [("random", S) for S in (127, 128, 129)]


@functools.lru_cache(maxsize=None)
def firstfit_of(name):
    n, rp, ci, keep = pattern(name)
    return ref_firstfit(rp, ci, keep)


@functools.lru_cache(maxsize=None)
def speculative_of(name, S=None):
    """(colours, rounds, W, the colours after every round)"""
    n, rp, ci, keep = pattern(name)
    states = []
    return ref_speculative(rp, ci, keep, S, states=states) + (states,)


# ---- the entries ------------------------------------------------------------------------------------------------------------------
def _u32(a):
    return gr._p(a, C.POINTER(C.c_uint))


def _u64(a):
    return gr._p(a, C.POINTER(C.c_ulonglong))


def _cap(n):
    """entries to allocate for an n that may be absurd (the entry refuses it before it touches the array)"""
    return min(max(n, 0), 1 << 20)


def dev_firstfit(L, n, rp, ci, keep, nKeep=None, guard=5):
    """-> (return code of the entry, colours, rc of color_firstfit_run, W); the colours hold n + guard entries, -7 on entry (a negative guard hands over a
    length below n)"""
    colors, rc, W = np.full(_cap(n) + max(guard, 0), -7, dtype=np.int32), C.c_int(-7), C.c_int(-7)
    e = L.das_debug_color_firstfit(n, gr._ll(rp), gr._i(ci), len(keep) if nKeep is None else nKeep, gr._ll(keep), gr._i(colors), max(n, 0) + guard, C.byref(rc),
                                   C.byref(W))
    return e, colors, rc.value, W.value


def dev_speculative(L, n, rp, ci, keep, spread=-1, nKeep=None, guard=5):
    """-> (return code, colours, ok, rounds, S, W)"""
    colors = np.full(_cap(n) + max(guard, 0), -7, dtype=np.int32)
    ok, rounds, S, W = C.c_int(-7), C.c_int(-7), C.c_int(-7), C.c_int(-7)
    e = L.das_debug_color_speculative(n, gr._ll(rp), gr._i(ci), len(keep) if nKeep is None else nKeep, gr._ll(keep), spread, gr._i(colors), max(n, 0) + guard,
                                      C.byref(ok), C.byref(rounds), C.byref(S), C.byref(W))
    return e, colors, ok.value, rounds.value, S.value, W.value


def dev_spec_round(L, n, rp, ci, keep, colors, S, W, rnd, guard=5, f_guard=3):
    """-> (return code, tent, lose, colours, F, left, overflow); the arrays hold guard (F: f_guard) entries more than are written, the
    lengths handed over say so - a negative guard hands over a length that is too short"""
    m = _cap(n) + max(guard, 0)
    tent, lose, out = np.full(m, -7, dtype=np.int32), np.full(m, 7, dtype=np.uint8), np.full(m, -7, dtype=np.int32)
    F = np.full(max(len(keep) * max(W, 0) + max(f_guard, 0), 1), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    left, over = C.c_uint(7), C.c_int(-7)
    e = L.das_debug_color_spec_round(n, gr._ll(rp), gr._i(ci), len(keep), gr._ll(keep), gr._i(colors), S, W, rnd, gr._i(tent), gr._u8(lose), gr._i(out),
                                     max(n, 0) + guard, _u64(F), len(keep) * max(W, 0) + f_guard, C.byref(left), C.byref(over))
    return e, tent, lose, out, F, left.value, over.value


def dev_check(L, n, rp, ci, keep, colors, W):
    """-> (return code, invalid)"""
    bad = C.c_int(-7)
    return L.das_debug_color_check(n, gr._ll(rp), gr._i(ci), len(keep), gr._ll(keep), gr._i(colors), W, C.byref(bad)), bad.value

"""The colouring kernels (dafoam_amd/csrc/das_color.hpp: k_color_firstfit, k_spec_assign, k_spec_conflict, k_spec_commit,
k_spec_netbits) on the device against their restatements in tests/color_reference.py: no mesh, no solver.  The entries
das_debug_color_* check the caller-made pattern on the host, derive the device structures with the helpers the solver uses and then run
what the solver runs.  Every result is EXACT - colours, rounds, widths, tentative colours, losers, bitmaps - and every full run is made
twice for identical output.  The patterns reach what no mesh reaches: columns without a net and with up to 130, nets of 1 to 1700
columns, groups on both sides of the cut at 8, cliques that need the last bit of the last bitmap word and one colour more, a dependency
chain through every column, spreads below the colour count and on word boundaries, bitmaps of 10 and of 67 words.  No test comes near the
watchdog or the spin limit of the data-flow kernel: the longest dependency chain has 2000 links."""
import functools

import numpy as np
import pytest

import color_reference as cr
import graph_reference as gr
from dafoam_amd import _capi

pytestmark = pytest.mark.gpu


def err():
    return _capi.lib().das_last_error()


def guard_intact(a, n):
    """the entries behind the n that an entry may write still hold the wrappers' fill value"""
    return bool(np.all(a[n:] == -7))


@pytest.mark.parametrize("name", cr.PATTERNS + ["long_net"])
def test_first_fit_is_the_serial_sweep(name):
    """return code 1, the colours of the serial first-fit, the bitmap width that holds them (8 words, doubled on overflow), twice"""
    n, rp, ci, keep = cr.pattern(name)
    ref = cr.firstfit_of(name)
    runs = [cr.dev_firstfit(_capi.lib(), n, rp, ci, keep) for _ in range(2)]
    for e, colors, rc, W in runs:
        assert e == 0, err()
        assert rc == 1 and W == cr.firstfit_width(ref), (rc, W)
        assert gr.same(colors[:n], ref) and guard_intact(colors, n)
    assert gr.same(runs[0][1], runs[1][1])


@pytest.mark.parametrize("name,S", [(p, None) for p in cr.PATTERNS] + cr.SPREADS)
def test_speculative_run_is_the_restatement(name, S):
    """colours, rounds, spread and width equal the restatement's, the result is valid by the brute force, twice"""
    n, rp, ci, keep = cr.pattern(name)
    ref, rounds, W, _ = cr.speculative_of(name, S)
    runs = [cr.dev_speculative(_capi.lib(), n, rp, ci, keep, -1 if S is None else S) for _ in range(2)]
    for e, colors, ok, r, s, w in runs:
        assert e == 0, err()
        assert ok == 1 and (r, s, w) == (rounds, cr.spread_rule(rp, keep) if S is None else S, W), (ok, r, s, w, rounds, W)
        assert gr.same(colors[:n], ref) and guard_intact(colors, n)
        assert cr.valid(rp, ci, keep, colors[:n])
    assert gr.same(runs[0][1], runs[1][1])


def test_long_net_is_coloured_or_given_up_loudly():
    """one net of 1700 columns asks for 67 bitmap words, 67 KiB of LDS in k_spec_conflict: the restatement's result, or ok = 0 where the
    device cannot hold the width - never ok = 1 with an invalid colouring"""
    n, rp, ci, keep = cr.pattern("long_net")
    ref, rounds, W, _ = cr.speculative_of("long_net")
    assert W == 67
    runs = [cr.dev_speculative(_capi.lib(), n, rp, ci, keep) for _ in range(2)]
    for e, colors, ok, r, s, w in runs:
        assert e == 0, err()
        print(f"long net: ok {ok}, rounds {r}, S {s}, W {w}")
        assert ok in (0, 1) and s == 2125
        if ok:
            assert cr.valid(rp, ci, keep, colors[:n])
            assert (r, w) == (rounds, W) and gr.same(colors[:n], ref)
        else:
            assert np.all(colors == -7), "a run that gave up wrote colours"
    assert runs[0][2:] == runs[1][2:] and gr.same(runs[0][1], runs[1][1])


@functools.lru_cache(maxsize=None)
def round_case(name, S, at):
    """(the pattern, the final colours before round `at` of the restatement's run, S, W)"""
    n, rp, ci, keep = cr.pattern(name)
    _, rounds, W, states = cr.speculative_of(name, S)
    assert at < rounds
    before = np.full(n, -1, dtype=np.int32) if at == 0 else states[at - 1]
    assert at == 0 or 0 < np.sum(before < 0) < n
    return n, rp, ci, keep, before, cr.spread_rule(rp, keep) if S is None else S, W


@pytest.mark.parametrize("name,S,at", [("by_net_count", None, 0), ("by_net_count", None, 7), ("by_net_length", None, 0), ("by_net_length", None, 1),
                                       ("groups", None, 0), ("groups", None, 2), ("width10", None, 0), ("width10", None, 1), ("crowded", 8, 0), ("crowded", 8, 40),
                                       ("crowded", 64, 5), ("clique513", 65, 100), ("random", 128, 0), ("random", 128, 3), ("chain", None, 1)])
def test_one_round_kernel_by_kernel(name, S, at):
    """k_spec_netbits, k_spec_assign, k_spec_conflict, k_spec_commit, k_spec_netbits from round 0 and from a half-finished state of the
    restatement: tent, lose, the colours, left, F and the overflow flag"""
    n, rp, ci, keep, before, S, W = round_case(name, S, at)
    nets, colnets = cr.nets_of(rp, ci, keep)
    tent, lose, after, left, overflow = cr.ref_spec_round(nets, colnets, before, S, W, at)
    e, dtent, dlose, dafter, dF, dleft, dover = cr.dev_spec_round(_capi.lib(), n, rp, ci, keep, before, S, W, at)
    assert e == 0, err()
    assert gr.same(dtent[:n], tent), "k_spec_assign: tentative colours"
    assert gr.same(dlose[:n], lose), "k_spec_conflict: losers"
    assert gr.same(dafter[:n], after) and dleft == left, "k_spec_commit: colours / columns left"
    assert gr.same(dF[:len(keep) * W], cr.ref_netbits(nets, after, W)), "k_spec_netbits"
    assert dover == int(overflow) == 0
    assert guard_intact(dtent, n) and guard_intact(dafter, n) and np.all(dlose[n:] == 7) and np.all(dF[len(keep) * W:] == np.uint64(0x5A5A5A5A5A5A5A5A))


def test_one_round_that_overflows():
    """a clique of 513 in 8 words with 512 colours taken: the last column finds none - overflow, no tentative colour, still left"""
    n, rp, ci, keep = cr.pattern("clique513")
    before = np.arange(n, dtype=np.int32)
    before[[512, 513, 514]] = -1
    nets, colnets = cr.nets_of(rp, ci, keep)
    tent, lose, after, left, overflow = cr.ref_spec_round(nets, colnets, before, 65, 8, 3)
    assert overflow and tent[512] == -1 and left >= 1
    e, dtent, dlose, dafter, dF, dleft, dover = cr.dev_spec_round(_capi.lib(), n, rp, ci, keep, before, 65, 8, 3)
    assert e == 0, err()
    assert dover == 1 and dleft == left and gr.same(dtent[:n], tent) and gr.same(dlose[:n], lose) and gr.same(dafter[:n], after)
    assert gr.same(dF[:2 * 8], cr.ref_netbits(nets, after, 8))


def checked(name, colors, W):
    n, rp, ci, keep = cr.pattern(name)
    e, bad = cr.dev_check(_capi.lib(), n, rp, ci, keep, np.ascontiguousarray(colors, dtype=np.int32), W)
    assert e == 0, err()
    assert bad == (0 if cr.valid(rp, ci, keep, colors) else 1), "the device's validity pass disagrees with the brute force"
    return bad


@pytest.mark.parametrize("name", ["by_net_length", "by_net_count", "width10", "clique512"])
def test_validity_pass_accepts_valid_colourings(name):
    colors, _, W, _ = cr.speculative_of(name)
    assert checked(name, colors, W) == 0
    ff = cr.firstfit_of(name)
    assert checked(name, ff, max(W, cr.firstfit_width(ff))) == 0


@pytest.mark.parametrize("what", ["positions 3 and 70", "positions 3 and 70 of the last net", "colour 64 W - 1 twice", "one uncoloured column"])
def test_validity_pass_flags_an_invalid_colouring(what):
    """by_net_length: 42 nets (the last workgroup holds two), the net of 600 columns and the LAST net of 129"""
    n, rp, ci, keep = cr.pattern("by_net_length")
    good, _, W, _ = cr.speculative_of("by_net_length")
    bad = good.copy()
    q = len(keep) - 1 if "last" in what else 7
    cols = ci[rp[keep[q]]:rp[keep[q] + 1]]
    assert len(keep) % 4 and len(cols) > 70
    if what.startswith("positions"):
        bad[cols[70]] = good[cols[3]]
    elif what.startswith("colour"):
        assert good.max() < 64 * W - 1
        bad[cols[5]] = bad[cols[100]] = 64 * W - 1
    else:
        bad[cols[70]] = -1
    assert checked("by_net_length", good, W) == 0 and checked("by_net_length", bad, W) == 1

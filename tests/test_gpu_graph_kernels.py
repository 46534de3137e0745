"""The graph set-up kernels of the colouring input (dafoam_amd/csrc/das_graph.hpp: k_scan_block_sums, k_scan_apply, k_tr_count,
k_tr_fill, k_sort_rows, k_net_count, k_net_fill, k_group_flags, k_rows_gather) and the jacLowerBounds filter (k_count_keep, k_compact,
das_opmat.hpp) on the device against their restatements in tests/graph_reference.py: no mesh, no solver.  The entries das_debug_graph_*
and das_debug_compact check the caller-made structure on the host and then run the launch sequences the solver runs.  Every result is
EXACT - integers equal, values bitwise equal - and every entry is called twice for bitwise equality (atomics decide the arrival order of
the transpose; the sort must undo it).  The structures reach what no mesh reaches: empty transposed rows, rows on both sides of the
SORT_MAX = 2048 branch, scans with a ragged tail across the 1024 blocks and totals beyond 2^32, a 16-lane prefix that keeps only its
last lane, only its first or nothing, neighbouring columns with equal, nearly equal and empty net lists."""
import functools

import numpy as np
import pytest

import graph_reference as gr
from dafoam_amd import _capi

pytestmark = pytest.mark.gpu


def twice(run):
    a, b = run(), run()
    assert a[0] == 0, _capi.lib().das_last_error()
    assert b[0] == 0 and all(gr.same(np.asarray(p), np.asarray(q)) for p, q in zip(a[1:], b[1:])), "two runs on the same input differ"
    return a[1:]


@pytest.mark.parametrize("kind", ["random", "zero", "huge"])
@pytest.mark.parametrize("n", gr.SCAN_N)
def test_exclusive_scan(n, kind):
    cnt = gr.scan_counts(n, kind)
    out, total = twice(lambda: gr.dev_scan(_capi.lib(), cnt))
    ref = gr.ref_scan(cnt)
    assert gr.same(out, ref) and total == ref[-1]


@functools.lru_cache(maxsize=None)
def transposed_on_device():
    n, rp, ci, lens = gr.transpose_pattern()
    return (n, rp, ci, lens) + tuple(twice(lambda: gr.dev_transpose(_capi.lib(), n, rp, ci)))


def test_transpose_offsets():
    n, rp, ci, lens, trp, tcol = transposed_on_device()
    assert gr.same(trp, gr.ref_transpose(rp, ci)[0])


@pytest.mark.parametrize("L", gr.TR_LENGTHS_SHORT + gr.TR_LENGTHS_LONG)
def test_transposed_rows_ascend(L):
    """every transposed row of L entries: the network in LDS up to SORT_MAX, the single lane beyond"""
    n, rp, ci, lens, trp, tcol = transposed_on_device()
    rtrp, rtcol, _ = gr.ref_transpose(rp, ci)
    assert gr.same(trp, rtrp)
    hit = 0
    for j in np.flatnonzero(lens == L):
        assert gr.same(tcol[trp[j]:trp[j + 1]], rtcol[trp[j]:trp[j + 1]]), f"transposed row {j} of {L} entries"
        hit += 1
    assert hit > 0


def test_transpose_whole():
    n, rp, ci, lens, trp, tcol = transposed_on_device()
    assert gr.same(tcol, gr.ref_transpose(rp, ci)[1])


@pytest.mark.parametrize("which", ["none", "all", "every_other", "lane15", "lane0"])
def test_nets_positions_and_group_flags(which):
    n, rp, ci = gr.nets_pattern()
    keep = gr.nets_keeps(n, rp, ci)[which]
    cptr, crow, cpos, isStart, total = twice(lambda: gr.dev_nets(_capi.lib(), n, rp, ci, keep))
    rcptr, rcrow, rcpos, rstart = gr.ref_nets(rp, ci, keep)
    assert total == rcptr[-1] and gr.same(cptr, rcptr)
    assert gr.same(crow, rcrow), "nets of a column: wrong ids or not in ascending row order"
    assert gr.same(cpos, rcpos), "position of the column inside the net's ascending column list"
    assert gr.same(isStart, rstart)


def test_nets_on_the_long_rows():
    """the nets over the transpose pattern: columns of up to 2600 nets, many 16-entry steps per column"""
    n, rp, ci, lens = gr.transpose_pattern()
    keep = np.arange(1, n, 3, dtype=np.int64)
    cptr, crow, cpos, isStart, total = twice(lambda: gr.dev_nets(_capi.lib(), n, rp, ci, keep))
    rcptr, rcrow, rcpos, rstart = gr.ref_nets(rp, ci, keep)
    assert total == rcptr[-1] and gr.same(cptr, rcptr) and gr.same(crow, rcrow) and gr.same(cpos, rcpos) and gr.same(isStart, rstart)


def test_rows_gather():
    """rows repeated, empty rows, a count that is no multiple of the four rows of a block, rows longer than a wavefront; the gaps
    between the gathered rows and the end of out keep the sentinel"""
    n, rp, ci, lens = gr.transpose_pattern()
    rl = np.diff(rp)
    rows = np.concatenate([np.flatnonzero(rl == 0)[:2], [int(np.argmax(rl)), 7, 7, n - 1, 0, int(np.argmax(rl))], np.arange(100, 113)]).astype(np.int64)
    assert len(rows) % 4 and rl.max() > 64
    dst = np.zeros(len(rows), dtype=np.int64)
    dst[1:] = np.cumsum(rl[rows] + 3)[:-1]  # three sentinels between two rows
    out = np.full(int(dst[-1] + rl[rows[-1]] + 5), -7, dtype=np.int32)
    (got,) = twice(lambda: gr.dev_rows_gather(_capi.lib(), rows, n, rp, ci, dst, out))
    assert gr.same(got, gr.ref_rows_gather(rows, rp, ci, dst, out))


@pytest.mark.parametrize("mask", ["null", "some", "diag"])
@pytest.mark.parametrize("use_bound", [0, 1])
def test_filter_and_compaction(use_bound, mask):
    """|v| == bound goes, a diagonal below the bound stays, a NaN off the diagonal goes, -0.0 keeps its sign, an un-owned column goes
    even on the diagonal: rowptr, columns and values bitwise"""
    n, rp, ci, v, bound = gr.filter_matrix()
    owned = gr.filter_masks(n)[mask]
    nrp, nci, nv = twice(lambda: gr.dev_compact(_capi.lib(), n, rp, ci, v, bound, use_bound, owned))
    rrp, rci, rv = gr.ref_filter(rp, ci, v, bound, use_bound, owned)
    assert gr.same(nrp, rrp) and gr.same(nci, rci) and gr.same(nv, rv)

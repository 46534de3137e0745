"""CPU tier: the recursive coordinate bisection every partition of the library comes from (csrc/das_rcb.hpp: the "ras" blocks, the
amd.pcSubdomains blocks, the "rcb" aggregates, the colouring tiles), through das_debug_rcb, against a numpy statement of the rule
written here: a range is cut across its widest axis (the lowest axis wins a tie of extents) in the order (coordinate, index).  The
numpy version SORTS every range with np.lexsort and cuts the sorted range - no selection algorithm - so the two agree only if the
set on each side of every cut is what the total order says.  The whole output array is compared, not its validity."""
import ctypes as C

import numpy as np
import pytest

from dafoam_amd import _capi
from dafoam_amd._capi import dptr


def _sort_range(idx, X, b, e):
    """idx[b:e] sorted by (coordinate on the widest axis of the range, index); an empty range has no widest axis and nothing to sort"""
    seg = idx[b:e]
    if seg.size == 0:
        return
    ext = X[seg].max(axis=0) - X[seg].min(axis=0)
    ax = 0
    for d in (1, 2):
        if ext[d] > ext[ax]:
            ax = d
    idx[b:e] = seg[np.lexsort((seg, X[seg, ax]))]


def ref_parts(X, K):
    n = X.shape[0]
    idx, out = np.arange(n), np.full(n, -1, np.int32)

    def rec(b, e, a0, na):
        if na == 1:
            out[idx[b:e]] = a0
            return
        nl = na // 2
        mid = b + (e - b) * nl // na
        _sort_range(idx, X, b, e)
        rec(b, mid, a0, nl)
        rec(mid, e, a0 + nl, na - nl)

    rec(0, n, 0, K)
    return out


def ref_leaves(X, max_leaf):
    n = X.shape[0]
    idx, out = np.arange(n), np.full(n, -1, np.int32)
    starts = []

    def rec(b, e):
        if e - b <= max_leaf:
            starts.append(b)
            return
        mid = (b + e) // 2
        _sort_range(idx, X, b, e)
        rec(b, mid)
        rec(mid, e)

    rec(0, n)
    assert starts == sorted(starts)  # leaves are numbered by ascending start
    for leaf, (b, e) in enumerate(zip(starts, starts[1:] + [n])):
        out[idx[b:e]] = leaf
    return out


def lib_rcb(X, mode, param):
    X = np.ascontiguousarray(X, np.float64)
    out = np.full(X.shape[0], -7, np.int32)
    _capi.check(_capi.lib().das_debug_rcb(X.shape[0], dptr(X), mode, param, out.ctypes.data_as(_capi.c_int_p)))
    return out


def _grid():
    """4 x 3 x 2 cell centres: almost every comparison on an axis is a tie"""
    x, y, z = np.meshgrid(np.arange(4) + 0.5, np.arange(3) + 0.5, np.arange(2) + 0.5, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)


def _tied_extents(first, second):
    """17 points: axes `first` < `second` have exactly the same extent (1), the third a smaller one - the lower axis must win"""
    X = np.random.default_rng(17).uniform(0.0, 1.0, (17, 3))
    third = 3 - first - second
    X[:, third] *= 0.5
    for ax in (first, second):
        X[2 + ax, ax], X[9 + ax, ax] = 0.0, 1.0
    assert X[:, first].max() - X[:, first].min() == X[:, second].max() - X[:, second].min() == 1.0
    return X


POINTS = {
    "grid_4x3x2": _grid(),
    "identical_24": np.full((24, 3), 0.25),
    "tie_xy_17": _tied_extents(0, 1),
    "tie_yz_17": _tied_extents(1, 2),
    "three": np.array([[0.3, 0.0, 0.0], [0.1, 0.0, 0.0], [0.2, 0.0, 0.0]]),
    "one": np.array([[1.0, 2.0, 3.0]]),
    "random_1000": np.random.default_rng(1000).standard_normal((1000, 3)),
}
PARTS = [(name, K) for name in ("grid_4x3x2", "identical_24", "tie_xy_17", "tie_yz_17") for K in (2, 3, 5, 7)]
PARTS += [("three", 5), ("three", 2), ("one", 1), ("one", 2), ("random_1000", 16)]
LEAVES = [(name, L) for name in ("grid_4x3x2", "identical_24", "tie_xy_17", "tie_yz_17") for L in (1, 5, 24, 100)]
LEAVES += [("three", 1), ("one", 1), ("random_1000", 64)]


@pytest.mark.parametrize("name,K", PARTS)
def test_rcb_parts_match_the_sorted_statement(name, K):
    X = POINTS[name]
    ref = ref_parts(X, K)
    assert np.array_equal(lib_rcb(X, 0, K), ref)
    # (what the rule gives: sizes differ by at most one when K <= n; K > n leaves parts empty, and every point still has one)
    sizes = np.bincount(ref, minlength=K)
    assert sizes.sum() == X.shape[0] and (K > X.shape[0] or sizes.max() - sizes.min() <= 1)


@pytest.mark.parametrize("name,max_leaf", LEAVES)
def test_rcb_leaves_match_the_sorted_statement(name, max_leaf):
    X = POINTS[name]
    ref = ref_leaves(X, max_leaf)
    assert np.array_equal(lib_rcb(X, 1, max_leaf), ref)
    assert np.bincount(ref).max() <= max_leaf


def test_rcb_ties_are_decided_as_stated():
    """the two facts a sorted restatement could share with the code by accident, stated directly: identical points are cut by index, and of two
    axes with the same extent the lower one is cut"""
    assert np.array_equal(lib_rcb(POINTS["identical_24"], 0, 2), np.repeat([0, 1], 12).astype(np.int32))
    for name, ax in (("tie_xy_17", 0), ("tie_yz_17", 1)):
        X = POINTS[name]
        part = lib_rcb(X, 0, 2)
        assert X[part == 0, ax].max() <= X[part == 1, ax].min() and (part == 0).sum() == 8


def test_rcb_rejects_bad_arguments():
    X, out = POINTS["three"], np.zeros(3, np.int32)
    L = _capi.lib()
    for mode, param in ((0, 0), (1, 0), (2, 1), (-1, 1)):
        assert L.das_debug_rcb(3, dptr(np.ascontiguousarray(X)), mode, param, out.ctypes.data_as(_capi.c_int_p)) != 0
    assert L.das_debug_rcb(-1, dptr(np.ascontiguousarray(X)), 0, 2, out.ctypes.data_as(_capi.c_int_p)) != 0
    assert L.das_debug_rcb(3, None, 0, 2, out.ctypes.data_as(_capi.c_int_p)) != 0

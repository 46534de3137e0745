"""The packed operator (dafoam_amd/csrc/das_opmat.hpp: k_vecpack_count, k_vecpack_fill, k_spmv_vec3, and k_spmv_wave on the scalar rows
around the pack) and the ghost-row product k_spmv_rows_to_buf (das_comm.hpp) on the device against tests/graph_reference.py: no mesh, no
solver.  das_debug_vecpack runs vecpack_build and launch_spmv as the solver does.  The pack's offsets, chunk count and BYTES equal the
reference layout (pad columns = the last valid column of the row, pad values +0.0); every product row lies inside T u sum |a x| with T its
length (the derived bound of test_spmv_wave), a row of no entries is exactly 0, every y inside [0, n) is written and nothing beyond; a
group whose rows do not share their list makes built = 0 and writes nothing; and with one NaN or +Inf in x exactly the rows that hold that
column are non-finite - a tail that multiplies a foreign x entry by its masked 0.0 shows only there.  Group rows of 0 .. 280 entries sit
on the 16 / 64 / 80 boundaries of the chunk and VP_UNROLL loops, the pack starts at row 0 or 5 and ends at n or before scalar rows.
Every entry is called twice for bitwise equality.  The achieved max err / bound is printed by the last test (profiles/README.md holds a
recorded table)."""
import ctypes as C

import numpy as np
import pytest

import graph_reference as gr
import krylov_reference as kr
from dafoam_amd import _capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="np.longdouble has no 64-bit mantissa on this platform: no reference")]

FIGURES = {}
POISONS = {"nan": np.nan, "inf": np.inf}


def record(op, kind, ratio):
    FIGURES[(op, kind)] = max(FIGURES.get((op, kind), 0.0), ratio)


def twice(run):
    a, b = run(), run()
    assert a[0] == 0, _capi.lib().das_last_error()
    assert b[0] == 0 and all(gr.same(np.asarray(p), np.asarray(q)) for p, q in zip(a[1:], b[1:])), "two runs on the same input differ"
    return a[1:]


def pack_on_device(n, rp, ci, v, row0, nG, x):
    built, cptr, data, nch, y = twice(lambda: gr.dev_vecpack(_capi.lib(), n, rp, ci, v, row0, nG, x))
    return built, cptr, data, nch, y


@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("shape", gr.PACK_SHAPES)
def test_pack_layout_and_product(shape, kind):
    row0, nG, ntail, shift = shape
    n, rp, ci, v, x = gr.pack_matrix(row0, nG, ntail, 3, kind, shift)
    built, cptr, data, nch, y = pack_on_device(n, rp, ci, v, row0, nG, x)
    rbuilt, rcptr, rchunks = gr.ref_pack(rp, ci, v, row0, nG)
    assert built == 1 and rbuilt and nch == rcptr[-1] and gr.same(cptr, rcptr)
    assert data[: 448 * nch].tobytes() == rchunks.tobytes(), "chunk bytes: columns, value planes, pad columns or pad values"
    assert np.all(data[448 * nch:] == 0x5A)
    ref, mag, lens = gr.ref_product(rp, ci, v, x)
    assert not np.any(y[:n] == gr.SENTINEL), "a row of y was not written"
    assert gr.guard_intact(y, n), "y was written beyond n"
    assert np.all(y[:n][lens == 0] == 0.0)
    sl = slice(row0, row0 + 3 * nG)
    scalar = np.ones(n, dtype=bool)
    scalar[sl] = False
    ok_p, r_p = gr.check_product(y[:n][sl], ref[sl], mag[sl], lens[sl])
    ok_s, r_s = gr.check_product(y[:n][scalar], ref[scalar], mag[scalar], lens[scalar])
    print(f"k_spmv_vec3 {r_p:.3g}, k_spmv_wave around the pack {r_s:.3g} of the bound")
    record("k_spmv_vec3", kind, r_p)
    record("k_spmv_wave around the pack", kind, r_s)
    assert ok_p and ok_s, (r_p, r_s)


def test_pack_only_without_x():
    row0, nG, ntail, shift = gr.PACK_SHAPES[3]
    n, rp, ci, v, x = gr.pack_matrix(row0, nG, ntail, 3, "ill", shift)
    built, cptr, data, nch, y = pack_on_device(n, rp, ci, v, row0, nG, None)
    rbuilt, rcptr, rchunks = gr.ref_pack(rp, ci, v, row0, nG)
    assert built == 1 and gr.same(cptr, rcptr) and data[: 448 * nch].tobytes() == rchunks.tobytes() and np.all(y == gr.SENTINEL)


@pytest.mark.parametrize("what", ["len", 0, 5, -1])
@pytest.mark.parametrize("g", [0, 20])
def test_rows_that_do_not_share_their_list_are_not_packed(g, what):
    """lengths differ; one column differs at position 0, at a position of a lane != 0, at the last position; in group 0 and in a
    group of the second workgroup: built = 0 and nothing is written"""
    n, rp, ci, v, x = gr.pack_matrix(5, 33, 14, 3, "well", 4, break_at=(g, what))
    built, cptr, data, nch, y = pack_on_device(n, rp, ci, v, 5, 33, x)
    assert built == 0 and nch == -7 and np.all(cptr == 0x5A5A5A5A) and np.all(data == 0x5A) and np.all(y == gr.SENTINEL)


@pytest.mark.parametrize("poison", sorted(POISONS))
@pytest.mark.parametrize("shape", gr.PACK_SHAPES[1:5])
def test_poisoned_x_reaches_only_the_rows_that_hold_its_column(shape, poison):
    row0, nG, ntail, shift = shape
    n, rp, ci, v, x = gr.pack_matrix(row0, nG, ntail, 3, "well", shift)
    ci2, p, dirty = gr.poison_groups(row0, nG, rp, ci)
    assert 0 < dirty.sum() < n
    ref, mag, lens = gr.ref_product(rp, ci2, v, x)
    xp = x.copy()
    xp[p] = POISONS[poison]
    built, cptr, data, nch, y = pack_on_device(n, rp, ci2, v, row0, nG, xp)
    assert built == 1 and gr.guard_intact(y, n)
    ok, ratio = gr.check_poisoned(y[:n], ref, mag, lens, dirty)
    record("packed product, poisoned x", poison, ratio)
    assert ok, (ratio, np.flatnonzero(~np.isfinite(y[:n]) != dirty))


def scalar_matrix(kind):
    """rows of SCALAR_LENGTHS entries, 37 of them and a 38th empty one: unsorted, repeated columns"""
    lens = [gr.SCALAR_LENGTHS[(5 * i + 3) % len(gr.SCALAR_LENGTHS)] for i in range(37)] + [0]
    rp = gr.ref_scan(lens)
    rng = np.random.default_rng(17)
    n = len(lens)
    ci = rng.integers(0, n, size=rp[-1]).astype(np.int32)
    v = gr.values(int(rp[-1]), [17, 7], kind)
    x = gr.values(n, [17, 8], "well") if kind == "well" else kr.vector(n, [17, 8])
    if kind == "well":
        gr.assert_well(rp, ci, v, x)
    assert set(gr.SCALAR_LENGTHS) <= set(lens)
    return n, rp, ci, v, x


def mat_mult(n, rp, ci, v, x):
    """k_spmv_wave through das_mat_create_from_csr + das_mat_mult"""
    L = _capi.lib()
    h = C.c_void_p()
    _capi.check(L.das_mat_create_from_csr(n, gr._ll(rp), gr._i(ci), gr._d(v), C.byref(h)))
    try:
        def run():
            y = np.full(n, gr.SENTINEL)
            return L.das_mat_mult(h, gr._d(x), gr._d(y)), y

        (y,) = twice(run)
    finally:
        L.das_mat_destroy(h)
    return y


@pytest.mark.parametrize("poison", sorted(POISONS))
def test_spmv_wave_poisoned_x(poison):
    n, rp, ci, v, x = scalar_matrix("well")
    ci2, p, dirty = gr.poison(rp, ci)
    assert 0 < dirty.sum() < n
    ref, mag, lens = gr.ref_product(rp, ci2, v, x)
    xp = x.copy()
    xp[p] = POISONS[poison]
    ok, ratio = gr.check_poisoned(mat_mult(n, rp, ci2, v, xp), ref, mag, lens, dirty)
    record("k_spmv_wave, poisoned x", poison, ratio)
    assert ok, ratio


ROWS = np.array([3, 37, 3, 0, 36, 12, 12, 12, 37, 5, 1, 2, 4, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
                 33, 34, 35, 37], dtype=np.int32)  # 43 rows: repeats, the empty row 37 three times, no multiple of 16


@pytest.mark.parametrize("kind", ["well", "ill"])
def test_spmv_rows_to_buf(kind):
    n, rp, ci, v, x = scalar_matrix(kind)
    assert len(ROWS) % 16 and rp[38] == rp[37]
    (buf,) = twice(lambda: gr.dev_spmv_rows(_capi.lib(), ROWS, n, rp, ci, v, x))
    ref, mag, lens = gr.ref_product(rp, ci, v, x)
    assert gr.guard_intact(buf, len(ROWS)) and not np.any(buf[: len(ROWS)] == gr.SENTINEL)
    assert np.all(buf[: len(ROWS)][lens[ROWS] == 0] == 0.0)
    ok, ratio = gr.check_product(buf[: len(ROWS)], ref[ROWS], mag[ROWS], lens[ROWS])
    record("k_spmv_rows_to_buf", kind, ratio)
    assert ok, ratio


@pytest.mark.parametrize("poison", sorted(POISONS))
def test_spmv_rows_to_buf_poisoned_x(poison):
    n, rp, ci, v, x = scalar_matrix("well")
    ci2, p, dirty = gr.poison(rp, ci)
    ref, mag, lens = gr.ref_product(rp, ci2, v, x)
    xp = x.copy()
    xp[p] = POISONS[poison]
    (buf,) = twice(lambda: gr.dev_spmv_rows(_capi.lib(), ROWS, n, rp, ci2, v, xp))
    ok, ratio = gr.check_poisoned(buf[: len(ROWS)], ref[ROWS], mag[ROWS], lens[ROWS], dirty[ROWS])
    record("k_spmv_rows_to_buf, poisoned x", poison, ratio)
    assert ok and gr.guard_intact(buf, len(ROWS)), ratio


def test_zzz_print_achieved_errors(capsys):
    """the achieved max err / bound (T u sum |a x|, 1 = the bound) of everything that ran in this module"""
    with capsys.disabled():
        print("\n| kernel | values | max err / bound |\n|---|---|---|")
        for (op, kind), r in sorted(FIGURES.items()):
            print(f"| {op} | {kind} | {r:.3g} |")
    assert all(r <= 1.0 for r in FIGURES.values())

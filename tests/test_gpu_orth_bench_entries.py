"""The two tuning entries das_debug_orth_bench / das_debug_orth_bench_split: every shape tools/orth_bench.py walks (the lists of
dafoam_amd/orth_bench_shapes.py, which the tool imports as well) runs and reports a positive time for the kernel that was asked for
and -1 for the other one; a shape that is not compiled reports -1 for both; bad arguments are refused.  n = 4099 is no multiple of
4 and makes two workgroups of both the 4096-row and the 1024-row tiles.  Nothing is asserted about the times beyond their sign."""
import ctypes as C

import pytest

from dafoam_amd import _capi
from dafoam_amd import orth_bench_shapes as S

pytestmark = pytest.mark.gpu

N, K, REPS = 4099, 5, 1
DAS_OK, DAS_ERR_ARG = 0, -1


def fp64(rows, unroll, rpt, n=N, k=K, reps=REPS):
    d, u = C.c_double(0.0), C.c_double(0.0)
    rc = _capi.lib().das_debug_orth_bench(n, k, reps, rows, unroll, rpt, C.byref(d), C.byref(u))
    return rc, d.value, u.value


def split(fmt, variant, rows, unroll, rpt, n=N, k=K, reps=REPS):
    d, u = C.c_double(0.0), C.c_double(0.0)
    rc = _capi.lib().das_debug_orth_bench_split(n, k, reps, fmt, variant, rows, unroll, rpt, C.byref(d), C.byref(u))
    return rc, d.value, u.value


def dots_ok(res):
    rc, d, u = res
    assert rc == DAS_OK and d > 0 and u == -1, res


def update_ok(res):
    rc, d, u = res
    assert rc == DAS_OK and d == -1 and u > 0, res


def test_fp64_shapes():
    for rows in S.FP64_DOTS:
        dots_ok(fp64(rows, 0, 0))
    for unroll, rpt in S.FP64_UPD:
        update_ok(fp64(0, unroll, rpt))
    assert set(S.FP64_DOTS_QUICK) <= set(S.FP64_DOTS) and set(S.FP64_UPD_QUICK) <= set(S.FP64_UPD)


@pytest.mark.parametrize("variant", sorted(S.VARIANT), ids=S.VARIANT.get)
@pytest.mark.parametrize("fmt", [1, 2], ids=["fp32", "split"])
def test_split_shapes(fmt, variant):
    dots, upd = S.split_shapes(variant)
    for rows in dots:
        dots_ok(split(fmt, variant, rows, 0, 0))
    for unroll, rpt in upd:
        update_ok(split(fmt, variant, 0, unroll, rpt))


def test_shape_not_compiled():
    assert fp64(3, 0, 0) == (DAS_OK, -1, -1)
    assert fp64(0, 3, 3) == (DAS_OK, -1, -1)
    for fmt in (1, 2):
        for variant in S.VARIANT:
            assert split(fmt, variant, 3, 0, 0) == (DAS_OK, -1, -1)
            assert split(fmt, variant, 0, 3, 3) == (DAS_OK, -1, -1)


def test_bad_arguments():
    assert fp64(16, 4, 2, k=1)[0] == DAS_ERR_ARG
    assert fp64(16, 4, 2, reps=0)[0] == DAS_ERR_ARG
    assert split(2, 1, 4, 4, 2, k=1)[0] == DAS_ERR_ARG
    assert split(2, 1, 4, 4, 2, reps=0)[0] == DAS_ERR_ARG
    assert split(0, 1, 4, 4, 2)[0] == DAS_ERR_ARG
    assert split(2, 3, 4, 4, 2)[0] == DAS_ERR_ARG

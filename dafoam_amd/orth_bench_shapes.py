"""The shapes tools/orth_bench.py times through das_debug_orth_bench / das_debug_orth_bench_split - kept here, once, so that the
tool and tests/test_gpu_orth_bench_entries.py walk the same lists.  Inner products: rows per thread (scalar kernels) or groups of 4
rows per lane (wide kernels); update: (unroll, rows per thread) or (unroll, groups of 4 rows per lane)."""
FP64_DOTS = (4, 8, 16)
FP64_UPD = ((4, 1), (8, 1), (16, 1), (4, 2), (8, 2), (4, 4), (8, 4))
FP64_DOTS_QUICK, FP64_UPD_QUICK = (16,), ((4, 2),)  # the shapes the solver runs
SCALAR_DOTS, SCALAR_UPD = (8, 16), ((4, 1), (8, 1), (4, 2), (8, 2), (4, 4))
WIDE_DOTS, WIDE_UPD = (1, 2, 4), ((2, 1), (4, 1), (8, 1), (2, 2), (4, 2))
VARIANT = {0: "scalar", 1: "wide", 2: "wide-nt"}  # variant argument of das_debug_orth_bench_split


def split_shapes(variant):
    """(inner-product shapes, update shapes) of a variant of das_debug_orth_bench_split"""
    return (SCALAR_DOTS, SCALAR_UPD) if variant == 0 else (WIDE_DOTS, WIDE_UPD)

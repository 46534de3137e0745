"""Dev tool (GPU): the two kernels of the delayed re-orthogonalisation (k_multidot2, k_dcgs2_update) on synthetic vectors -
variants of rows per thread / unroll, no mesh and no setup.  Prints ms and TB/s per variant.
Default: the fp64 instantiations (8 (K + 2) n bytes per kernel).  --split / --fp32: the float instantiations the solver runs on its
compressed basis, in the solver's layout - the one-dword-per-lane kernels ("scalar") and the 16-byte-load kernels ("wide", "wide-nt" =
with non-temporal loads) side by side with the fp64 numbers; bytes counted: 4 per basis entry for the inner products (hi only), 8
(split) or 4 (fp32) for the update."""
import argparse, ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16172600)
ap.add_argument("--K", type=int, nargs="+", default=[150, 352])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--split", action="store_true", help="time the split (hi + lo floats) instantiations beside the fp64 ones")
ap.add_argument("--fp32", action="store_true", help="time the plain fp32 instantiations (no lo array) beside the fp64 ones")
ap.add_argument("--quick", action="store_true", help="fp64: only the default shapes")
a = ap.parse_args()
import __graft_entry__ as ge
ge.build()
from dafoam_amd import _capi
L = _capi.lib()
from dafoam_amd import orth_bench_shapes as S
FP64_DOTS = S.FP64_DOTS_QUICK if a.quick else S.FP64_DOTS
FP64_UPD = S.FP64_UPD_QUICK if a.quick else S.FP64_UPD
VARIANT = S.VARIANT


def line(K, what, ms, gb):
    if ms > 0:
        print(f"K {K:4d} {what:44s}: {ms:7.3f} ms  {gb / ms:6.2f} TB/s", flush=True)


for K in a.K:
    gb = 8.0 * (K + 2) * a.n / 1e9
    for rows in FP64_DOTS:
        d, u = C.c_double(-1), C.c_double(-1)
        _capi.check(L.das_debug_orth_bench(a.n, K, a.reps, rows, 0, 0, C.byref(d), C.byref(u)))
        line(K, f"fp64 k_multidot2<{rows}>", d.value, gb)
    for unroll, rpt in FP64_UPD:
        d, u = C.c_double(-1), C.c_double(-1)
        _capi.check(L.das_debug_orth_bench(a.n, K, a.reps, 0, unroll, rpt, C.byref(d), C.byref(u)))
        line(K, f"fp64 k_dcgs2_update<{unroll},{rpt}>", u.value, gb)
    for fmt, name, on in ((2, "split", a.split), (1, "fp32", a.fp32)):
        if not on:
            continue
        gb_d = 4.0 * (K + 2) * a.n / 1e9  # 4 B per basis entry (K vectors), u and v on top
        gb_u = (8.0 if fmt == 2 else 4.0) * (K + 2) * a.n / 1e9
        for variant in VARIANT:
            dots, upd = S.split_shapes(variant)
            for rows in dots:
                d, u = C.c_double(-1), C.c_double(-1)
                _capi.check(L.das_debug_orth_bench_split(a.n, K, a.reps, fmt, variant, rows, 0, 0, C.byref(d), C.byref(u)))
                line(K, f"{name} {VARIANT[variant]} multidot2 rows/lane {rows if variant == 0 else 4 * rows}", d.value, gb_d)
            for unroll, rpt in upd:
                d, u = C.c_double(-1), C.c_double(-1)
                _capi.check(L.das_debug_orth_bench_split(a.n, K, a.reps, fmt, variant, 0, unroll, rpt, C.byref(d), C.byref(u)))
                line(K, f"{name} {VARIANT[variant]} dcgs2_update unroll {unroll} rows/lane {rpt if variant == 0 else 4 * rpt}", u.value, gb_u)

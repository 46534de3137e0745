// Bodies of the test-only entries das_debug_poly_* (tests/test_poly_host_cpu.py, tests/test_gpu_poly_kernels.py): the roots and the
// host twin of the polynomial apply need no GPU; das_debug_poly_step uploads the caller's arrays, runs the launch helpers the solver
// runs (null stream) and downloads the result.  Nothing in the product path calls them.
#pragma once
#include "das_poly.hpp"
#include "das_krylov_debug.hpp"

namespace das {

enum { POLY_STEP_REAL = 0, POLY_STEP_PAIR_FIRST = 1, POLY_STEP_PAIR_SECOND = 2 };
// one root step on caller data.  Every array has len entries and its vector in [off, off + n): the device copy keeps that offset, so an
// odd off puts the vector on an 8-byte boundary (element-wise path), an even one on a 16-byte boundary (16-byte path).  theta = re + i im
// gives the coefficients exactly as the root walk forms them.  All five arrays are copied back.
static void debug_poly_step(long long n, int kind, bool first, bool last, double re, double im, long long off, long long len, double* v, double* w, double* prod,
                            double* poly, double* tmp) {
    const DevBuf<double> dv = krylov_up<double>(v, (size_t)len), dw = krylov_up<double>(w, (size_t)len), dprod = krylov_up<double>(prod, (size_t)len);
    const DevBuf<double> dpoly = krylov_up<double>(poly, (size_t)len), dtmp = krylov_up<double>(tmp, (size_t)len);
    double twoa = 0.0, c = re;
    if (kind != POLY_STEP_REAL) poly_pair_coef(re, im, twoa, c);
    if (kind == POLY_STEP_REAL) launch_poly_real(0, n, first, last, c, dv.p + off, dw.p + off, dpoly.p + off, dprod.p + off);
    else if (kind == POLY_STEP_PAIR_FIRST) launch_poly_pair_first(0, n, first, twoa, c, dv.p + off, dprod.p + off, dw.p + off, dpoly.p + off, dtmp.p + off);
    else if (!last) launch_poly_pair_second(0, n, first, c, dv.p + off, dw.p + off, dprod.p + off);
    krylov_debug_sync();
    dv.download(v, (size_t)len); dw.download(w, (size_t)len); dprod.download(prod, (size_t)len); dpoly.download(poly, (size_t)len); dtmp.download(tmp, (size_t)len);
}

}  // namespace das

"""CPU tier: the dense host algebra of the GMRES solvers (csrc/das_gmres_host.hpp) against numpy.  The block solve's least squares
(BlockLsq, through das_debug_block_lsq) and the Cholesky step of its CholQR (chol_upper_inverse, through das_debug_block_chol) are
the code run_block_gmres runs; the failure rule (gmres_failed in csrc/das_device.hip) is checked by
test_host_cpu.py::test_gmres_dr_loop_host_twin through the return value of das_debug_gmres_dr_host.  Bounds: u = 2^-53 times the size
and the condition number numpy reports, with a factor 8 for the modest constant of the backward-error bounds (Givens QR, Cholesky)
plus numpy's own rounding."""
import numpy as np
import pytest

from dafoam_amd import _capi
from dafoam_amd._capi import dptr

U = 2.0 ** -53
SEED = 20261018


def _upper(rng, sv):
    """upper triangular, diagonal in [1, 2]: what CholQR returns for a block of full rank"""
    S = np.triu(0.3 * rng.standard_normal((sv, sv)), 1)
    S[np.diag_indices(sv)] = rng.uniform(1.0, 2.0, sv)
    return S


def _block_case(sv, m, ncols):
    """random projection blocks of ncols block columns in the layout of das_debug_block_lsq, and the block Hessenberg matrix they mean"""
    rng = np.random.default_rng([SEED, sv, m, ncols])
    S0 = _upper(rng, sv)
    Hc, Hc2, S = np.zeros((ncols, m * sv, sv)), np.zeros((ncols, m * sv, sv)), np.zeros((ncols, sv, sv))
    H = np.zeros(((ncols + 1) * sv, ncols * sv))
    for j in range(ncols):
        K = (j + 1) * sv
        Hc[j, :K] = 0.3 * rng.standard_normal((K, sv))
        Hc2[j, :K] = 1e-8 * rng.standard_normal((K, sv))  # the second Gram-Schmidt pass corrects the first
        S[j] = _upper(rng, sv)
        H[:K, j * sv : K] = Hc[j, :K] + Hc2[j, :K]
        H[K : K + sv, j * sv : K] = S[j]
    return S0, Hc, Hc2, S, H


BLOCK_CASES = [(sv, m, ncols) for sv in (1, 2, 3, 8) for m, ncols in ((1, 1), (2, 2), (5, 5), (5, 3))]


def test_block_lsq_matches_numpy_lstsq():
    L = _capi.lib()
    rows, ok = [], True
    for sv, m, ncols in BLOCK_CASES:
        S0, Hc, Hc2, S, H = _block_case(sv, m, ncols)
        kappa = np.linalg.cond(H)
        assert kappa <= 1e3, (sv, m, ncols, kappa)
        Y, res = np.zeros((ncols * sv, sv)), np.zeros(sv)
        assert L.das_debug_block_lsq(sv, m, ncols, dptr(S0), dptr(Hc), dptr(Hc2), dptr(S), dptr(Y), dptr(res)) == 0, L.das_last_error()
        N = (ncols + 1) * sv
        rhs = np.zeros((N, sv))
        rhs[:sv] = S0
        for r in range(sv):
            y_np = np.linalg.lstsq(H, rhs[:, r], rcond=None)[0]
            ey, by = np.linalg.norm(Y[:, r] - y_np), 8 * N * U * kappa * np.linalg.norm(y_np)
            er, br = abs(res[r] - np.linalg.norm(rhs[:, r] - H @ y_np)), 8 * N * U * np.linalg.norm(S0[:, r])
            rows.append(f"sv {sv} m {m} ncols {ncols} rhs {r}: kappa {kappa:.2e}  Y {ey:.2e} / {by:.2e}  res {er:.2e} / {br:.2e}")
            ok = ok and ey <= by and er <= br
    if not ok:
        print("\n".join(rows))
    assert ok


@pytest.mark.parametrize("sv", [1, 3, 8])
def test_chol_upper_inverse(sv):
    rng = np.random.default_rng([SEED, sv])
    W = rng.standard_normal((50, sv))
    G = W.T @ W
    Lo, T = np.zeros((sv, sv)), np.zeros((sv, sv))
    assert _capi.lib().das_debug_block_chol(sv, dptr(G), dptr(Lo), dptr(T)) == 0
    gmax = np.abs(G).max()
    e1, e2 = np.abs(Lo @ Lo.T - G).max(), np.abs(Lo.T @ T - np.eye(sv)).max()
    print(f"sv {sv}: |L L^T - G| {e1:.2e} / {8 * sv * U * gmax:.2e}   |L^T T - I| {e2:.2e} / {8 * sv * U * np.linalg.cond(Lo):.2e}")
    assert np.all(np.triu(Lo, 1) == 0.0) and np.all(np.tril(T, -1) == 0.0)
    assert e1 <= 8 * sv * U * gmax
    assert e2 <= 8 * sv * U * np.linalg.cond(Lo)


def test_chol_upper_inverse_replaces_a_lost_column():
    """a column without content (zero column of W): its pivot is replaced by sqrt(1e-28 gmax), everything stays finite"""
    sv = 3
    W = np.random.default_rng([SEED, 0]).standard_normal((50, sv))
    W[:, 1] = 0.0
    G = W.T @ W
    Lo, T = np.zeros((sv, sv)), np.zeros((sv, sv))
    assert _capi.lib().das_debug_block_chol(sv, dptr(G), dptr(Lo), dptr(T)) == 0
    assert Lo[1, 1] == np.sqrt(1e-28 * np.diag(G).max())
    assert np.all(np.isfinite(Lo)) and np.all(np.isfinite(T))

"""The DAHeatTransferFoam test cases of tests/test_heat_transfer_cpu.py and tests/test_gpu_heat_transfer.py: the bump-mapped channel
(non-orthogonal, so the correction term is live) at 6 x 5 x 4 (120 cells: one workgroup with a tail) and 9 x 8 x 6 (432: a full workgroup
plus a tail), the pyramid / prism / polyhedron mesh of tests/mixed_mesh.py (148 cells) and its renumbered twin; inlet fixedValue 400, top
fixedValue 300, bottom mixed with per-face refValue in [290, 310] and valueFraction in [0.2, 0.8], the rest zeroGradient; kappa = 200 or
kappaCoeffs (20, 0.05, 1e-4) - three terms, kappa = 44 at 300 K and 56 at 400 K.  Cached: treat the cases as read-only."""
import functools

import numpy as np

from dafoam_amd.meshgen import heat_transfer_case, mixed_cell_case, renumber_case
from mixed_mesh import DIMS, MERGES, PRISM_COLUMNS, PYRAMIDS

MESHES = ("bump", "bump432", "mixed", "mixed_renumbered")
MATERIALS = {"const": dict(kappa=200.0), "poly": dict(kappa_coeffs=(20.0, 0.05, 1e-4))}
NORM = {"T": 300.0}


def mixed_records(n, seed=3):
    rng = np.random.default_rng(seed)
    return 290.0 + 20.0 * rng.random(n), 0.2 + 0.6 * rng.random(n)


@functools.lru_cache(maxsize=None)
def heat_case(mesh="bump", material="poly"):
    if mesh == "mixed_renumbered":
        return renumber_case(heat_case("mixed", material), seed=5)
    if mesh == "mixed":
        return mixed_cell_case(heat_case("bump", material), pyramids=PYRAMIDS, merges=MERGES, prism_columns=PRISM_COLUMNS)
    nx, ny, nz = DIMS if mesh == "bump" else (9, 8, 6)
    return heat_transfer_case(nx, ny, nz, mixed_patches={"bottom": mixed_records(nx * nz)}, **MATERIALS[material])


def heat_options(case, **extra):
    o = {"solverName": "DAHeatTransferFoam", "normalizeStates": dict(NORM), "adjEqnOption": {"printInfo": 0}}
    o.update(extra)
    return o

"""The DAPimpleFoam cases of tests/test_pimple_cpu.py and tests/test_gpu_pimple.py, and what both tiers share: the DASimpleFoam channels
of the other suites with the solver name, the ddt scheme and the time step set, old-time states that differ from the states in every
entry, the state scales and the blocks of the layout [U | p | nuTilda | phi].
  small  channel_case(6, 5, 4)   120 cells      bump   channel_case(10, 8, 6)   480 cells: two workgroups      mixed   the pyramid / prism /
  polyhedron mesh of tests/mixed_mesh.py, 148 cells
Cached: treat the cases as read-only."""
import copy
import functools

import numpy as np

from dafoam_amd.meshgen import channel_case
from mixed_mesh import mixed
from oracle.foam_mesh import Geometry

MESHES = ("small", "bump", "mixed")
NORM = {"U": 10.0, "p": 50.0, "nuTilda": 1e-3, "phi": 1.0}
DELTA_T = 2.0e-3
# (scheme, time index): Euler, backward at its first step (exactly Euler) and backward with both old levels
SCHEMES = (("Euler", 1), ("backward", 1), ("backward", 3))


@functools.lru_cache(maxsize=None)
def steady_case(mesh):
    if mesh == "mixed":
        return mixed("simple")
    return channel_case(6, 5, 4) if mesh == "small" else channel_case(10, 8, 6)


@functools.lru_cache(maxsize=None)
def pimple_case_of(mesh, scheme="Euler", deltaT=DELTA_T, n_steps=6):
    case = copy.copy(steady_case(mesh))
    case.solver_name, case.ddt_scheme, case.deltaT, case.n_steps = "DAPimpleFoam", scheme, deltaT, n_steps
    return case


@functools.lru_cache(maxsize=None)
def geom(mesh):
    return Geometry(steady_case(mesh).mesh)


@functools.lru_cache(maxsize=None)
def old_states(mesh):
    """(W0, W00): the states with every entry moved by a few per cent, two independent draws"""
    W = steady_case(mesh).states
    rng = np.random.default_rng(11)
    return W * (1.0 + 0.05 * rng.standard_normal(W.size)), W * (1.0 + 0.05 * rng.standard_normal(W.size))


def blocks(g):
    N = g.nC
    return {"U": slice(0, 3 * N), "p": slice(3 * N, 4 * N), "nuTilda": slice(4 * N, 5 * N), "phi": slice(5 * N, None)}


def scales(g, norm=NORM):
    """s_j of normalizeStates: the value for cell states, value x |S_f| for phi; ones without the option"""
    N = g.nC
    if not norm:
        return np.ones(5 * N + g.nF)
    return np.concatenate([np.full(3 * N, norm["U"]), np.full(N, norm["p"]), np.full(N, norm["nuTilda"]), norm["phi"] * g.magSf])


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300))


def options(**extra):
    o = {"solverName": "DAPimpleFoam", "normalizeStates": dict(NORM), "adjEqnOption": {"printInfo": 0}}
    o.update(extra)
    return o

"""The standard pyramid / prism / polyhedron test mesh of tests/test_mixed_mesh_cpu.py and tests/test_gpu_mixed_mesh.py: the 6 x 5 x 4
bump channel with five hexes cut into pyramids, three merge groups (a pair in x, a 2 x 2 x 1 slab, a pair in z) and two prism columns -
148 cells with 5, 6, 10 and 16 faces, 80 triangles (8 on front / back; more with side walls), up to 10 owned faces per cell."""
import functools

from dafoam_amd.meshgen import channel_case, mixed_cell_case, renumber_case, rho_channel_case, scalar_transport_case

DIMS = (6, 5, 4)
PYRAMIDS = ((1, 1, 1), (3, 2, 2), (0, 0, 0), (5, 4, 3), (2, 3, 1))
MERGES = (((3, 0, 0), (4, 0, 0)), ((0, 3, 2), (1, 3, 2), (0, 4, 2), (1, 4, 2)), ((4, 2, 0), (4, 2, 1)))
PRISM_COLUMNS = ((2, 1), (5, 0))


def mixed_of(case):
    return mixed_cell_case(case, pyramids=PYRAMIDS, merges=MERGES, prism_columns=PRISM_COLUMNS)


@functools.lru_cache(maxsize=None)
def mixed(kind="simple", wall_function=False, side_walls=False, renumbered=False):
    """kind: "simple" (DASimpleFoam), "rho" (DARhoSimpleFoam), "scalar" (DAScalarTransportFoam).  Cached: treat the case as read-only."""
    if renumbered:
        return renumber_case(mixed(kind, wall_function, side_walls), seed=5)
    if kind == "simple":
        return mixed_of(channel_case(*DIMS, wall_function=wall_function, side_walls=side_walls))
    if kind == "rho":
        return mixed_of(rho_channel_case(*DIMS, wall_function=wall_function))
    assert kind == "scalar"
    return mixed_of(scalar_transport_case(*DIMS))


MIXED = mixed()
MIXED_RENUMBERED = mixed(renumbered=True)

"""The actuator disks of tests/test_actuator_disk_cpu.py and tests/test_gpu_actuator_disk.py, on four DASimpleFoam channels (1.0 x 0.2 x 0.1):
  flat   channel_case(10, 8, 6) without the bump mapping (480 cells: two workgroups)      bump   the same with the bump mapping
  mixed  the pyramid / prism / polyhedron mesh of tests/mixed_mesh.py (148 cells)         box    16 x 13 x 10 (2080 cells: 9 workgroups of
                                                                                                 partial sums) for the reductions
  A  cylinderAnnulusSmooth, direction (1, 0.3, -0.2), rotDir left, adjustThrust 0
  B  cylinderAnnulusToCell along x, rotDir right
  C  cylinderAnnulusSmooth, another tilted direction, rotDir right, adjustThrust 1 (scale is computed, pars[8] is not read)
bump_walls / mixed_walls: bump and mixed with walls instead of the symmetry planes at front and back, for the volCoord products - a point on a
symmetry plane moved in z is treated differently by the product's dual metrics and by the restatement (4907.426 against 4906.989 at point 0
of bump WITHOUT any disk, through the host emulation as well): that is not the disks' business, so those tests move points of walls.
The names are chosen so that the sorted order (C, A, B) is not the order of insertion.  tests/test_actuator_disk_cpu.py checks on every
mesh that the three radial branches and both rotDir signs are live, that B's set is not empty, that no cell centre sits on an axis and that
the projection reading of the axial part is another field altogether.  Cached: treat the cases as read-only."""
import functools

import actuator_disk_restatement as AD
from dafoam_amd.meshgen import channel_case
from mixed_mesh import mixed

DISK_A = dict(type="actuatorDisk", source="cylinderAnnulusSmooth", center=[0.45, 0.11, 0.048], direction=[1.0, 0.3, -0.2], innerRadius=0.01, outerRadius=0.08,
              rotDir="left", scale=200.0, POD=0.7, eps=0.02, expM=1.0, expN=0.5, adjustThrust=0, targetThrust=0.0)
DISK_B = dict(type="actuatorDisk", source="cylinderAnnulusToCell", p1=[0.22, 0.1, 0.05], p2=[0.62, 0.1, 0.05], innerRadius=0.015, outerRadius=0.07,
              rotDir="right", scale=150.0, POD=0.9)
DISK_C = dict(DISK_A, center=[0.62, 0.09, 0.055], direction=[1.0, -0.25, 0.15], rotDir="right", scale=1.0e9, POD=1.1, expM=1.3, expN=0.6, adjustThrust=1,
              targetThrust=0.05)
ALL_DISKS = {"mid_A": DISK_A, "tail_B": DISK_B, "head_C": DISK_C}
NAMES = ("mid_A", "tail_B", "head_C")
MESHES = ("flat", "bump", "mixed", "box")
NORM = {"U": 10.0, "p": 50.0, "nuTilda": 1e-3, "phi": 1.0}


@functools.lru_cache(maxsize=None)
def disk_case(mesh):
    if mesh in ("mixed", "mixed_walls"):
        return mixed("simple", side_walls=mesh == "mixed_walls")
    if mesh == "bump_walls":
        return channel_case(10, 8, 6, side_walls=True)
    if mesh == "box":
        return channel_case(16, 13, 10)
    return channel_case(10, 8, 6, bump=0.0, skew=0.0) if mesh == "flat" else channel_case(10, 8, 6)


@functools.lru_cache(maxsize=None)
def geom(mesh):
    return AD.FlowGeom(disk_case(mesh).mesh)


@functools.lru_cache(maxsize=None)
def disks(mesh, names=NAMES):
    return AD.Disks(geom(mesh), {n: ALL_DISKS[n] for n in names})


def options(**extra):
    o = {"solverName": "DASimpleFoam", "normalizeStates": dict(NORM), "adjEqnOption": {"printInfo": 0}}
    o.update(extra)
    return o

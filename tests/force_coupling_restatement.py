"""numpy restatement of the reference's forceCouplingOutput (src/adjoint/DAOutput/DAOutputForceCoupling.C), written from that file:
  :41       the patches are sorted by name before anything else
  :43-56    size = 3 x sum over the patches of the distinct mesh points of the patch's faces (a point on two patches counts twice)
  :107-116  face force = Sf (p_b - pRef) + Sf . devRhoReff_b
  :142-191  every face gives force / nPointsOfFace to each of its points, patch by patch
  :194-201  inside a patch the points come out in ascending mesh-point index
  :207-214  layout [fx0, fy0, fz0, fx1, ...]
The boundary state and the sign convention are the oracle's (oracle.functions._boundary_state / _face_forces).  Works with complex W, so
complex steps through it give derivatives in the states; `bcs` replaces the case's patch table for the (central-difference) derivatives in a
patch value - the oracle's patch table holds real numbers."""
import copy

import numpy as np

from oracle.functions import _boundary_state, _face_forces


def patch_points(mesh, name):
    """Ascending distinct mesh points of the faces of one patch."""
    p = {q.name: q for q in mesh.patches}[name]
    ptr = mesh.face_ptr
    return np.unique(mesh.face_pts[ptr[p.start] : ptr[p.start + p.size]])


def output_points(case, patches):
    """[(patch name, its points)] in output order."""
    return [(nm, patch_points(case.mesh, nm)) for nm in sorted(patches)]


def size(case, patches):
    return 3 * sum(pts.size for _, pts in output_points(case, patches))


def face_forces(case, g, W, pRef, bcs=None):
    """(nBF, 3): the force of every boundary face, pressure shifted by pRef.  bcs: a replacement of case.bcs."""
    if bcs is not None:
        case = copy.copy(case)
        case.bcs = bcs
    b = _boundary_state(case, g, W)
    return _face_forces(g, b) - g.bSf * pRef


def distribute(case, g, ff, patches):
    """Nodal forces (3 x points, interleaved) from the per-face forces ff (nBF, 3)."""
    m = case.mesh
    ptr, fpts = m.face_ptr, m.face_pts
    by_name = {q.name: q for q in m.patches}
    out = []
    for nm, pts in output_points(case, patches):
        p = by_name[nm]
        acc = np.zeros((pts.size, 3), dtype=ff.dtype)
        for f in range(p.start, p.start + p.size):
            mine = fpts[ptr[f] : ptr[f + 1]]
            share = ff[f - g.nIF] / mine.size
            for q in np.searchsorted(pts, mine):
                acc[q] += share
        out.append(acc)
    return np.concatenate(out).ravel()


def nodal_forces(case, g, W, patches, pRef, bcs=None):
    return distribute(case, g, face_forces(case, g, W, pRef, bcs), patches)


def selected_faces(case, patches):
    """Mesh face indices in slot order: the sorted patches, each in face order."""
    by_name = {q.name: q for q in case.mesh.patches}
    return np.concatenate([np.arange(by_name[nm].start, by_name[nm].start + by_name[nm].size) for nm in sorted(patches)])

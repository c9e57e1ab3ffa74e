"""Host restatement of the heat sources for the tests ("Heat sources"), on top of tests/thermal_ref.py (corners,
face areas), tests/stack_ref.py (the workgroup sums) and tests/sampling_ref.py (the owner rule by brute force), with every
sum in the order the device states.  numpy contracts nothing, so every decision and every value is the same bit for bit.

Meshes come as (xy, tri, ...) tuples in flat order with ``mesh_layer`` the layer of each; a source is (layer, polygon (n, 2)).
 1. centroid of face f: cx = ((x1 + x2) + x3) / 3, cy likewise, corners as thermal_ref.corners.
 2. coverage: f belongs to a mesh of the source's layer and the centroid is inside by the even-odd rule -- the edge from
    (xj, yj), the previous vertex (cyclic), to (xi, yi) crosses when (yi > cy) != (yj > cy) and
    cx < (xj - xi) * (cy - yi) / (yj - yi) + xi; inside when the number of crossings is odd.
 3. list: the covered faces ascending; A_s = stack_ref.mesh_sum of their areas (thermal_ref.face_area) in list order.
 4. fallback for an empty list: q = the polygon's vertex mean (summed in vertex order from 0.0, divided by n); the list is
    the one face that owns q among the faces of the layer (sampling_ref.owners); none: ValueError.
 5. load of one column: per vertex acc = 0, over its faces ascending and the sources of each face ascending
    acc = acc + ((area_f / A_s) * p_s) / 3; then b_v = b_v + acc.
 6. footprint temperature: ambient + mesh_sum over the list of (area_f / A_s) * mean_f."""
from __future__ import annotations

import numpy as np

import stack_ref as K
import thermal_ref as T


def centroids(xy, tri) -> np.ndarray:
    """(n_tri, 2): definition 1."""
    c = T.corners(tri)
    return ((xy[c[:, 0]] + xy[c[:, 1]]) + xy[c[:, 2]]) / 3


def inside(polygon, cx, cy) -> np.ndarray:
    """The even-odd rule of definition 2 for the points (cx, cy), elementwise."""
    polygon = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
    crossings = np.zeros(np.shape(cx), dtype=np.int64)
    for i in range(len(polygon)):
        (xi, yi), (xj, yj) = polygon[i], polygon[i - 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            crossings += ((yi > cy) != (yj > cy)) & (cx < (xj - xi) * (cy - yi) / (yj - yi) + xi)
    return crossings % 2 == 1


def coverage(meshes, mesh_layer, sources) -> np.ndarray:
    """(n_source, n_tri) bool: definition 2."""
    xy, tri, face_mesh, _voff, _toff = T.flatten(meshes)
    cen = centroids(xy, tri)
    face_layer = np.asarray(mesh_layer, dtype=np.int64)[face_mesh]
    out = np.zeros((len(sources), len(tri)), dtype=bool)
    for s, (layer, polygon) in enumerate(sources):
        out[s] = (face_layer == layer) & inside(polygon, cen[:, 0], cen[:, 1])
    return out


def vertex_mean(polygon) -> tuple:
    polygon = np.asarray(polygon, dtype=np.float64).reshape(-1, 2)
    sx = sy = 0.0
    for x, y in polygon:
        sx = sx + x
        sy = sy + y
    return sx / len(polygon), sy / len(polygon)


def fallback(meshes, mesh_layer, layer, polygon) -> int:
    """The owner face of the polygon's vertex mean among the faces of ``layer`` (definition 4), -1 for none."""
    return int(K.R.owners(K.board_of(meshes, mesh_layer), layer, np.array([vertex_mean(polygon)]))[0])


def lists(meshes, mesh_layer, sources):
    """(ptr (n + 1,), face, fallback flags (n,) bool): definitions 3 and 4.  ValueError for a source that lies on no face."""
    cover = coverage(meshes, mesh_layer, sources)
    ptr, face, flags = [0], [], []
    for s, (layer, polygon) in enumerate(sources):
        mine = np.flatnonzero(cover[s])
        flags.append(len(mine) == 0)
        if len(mine) == 0:
            owner = fallback(meshes, mesh_layer, layer, polygon)
            if owner < 0:
                raise ValueError(f"source {s} lies on no face of layer {layer}")
            mine = np.array([owner], dtype=np.int64)
        face.append(mine)
        ptr.append(ptr[-1] + len(mine))
    return (np.asarray(ptr, dtype=np.int64), np.concatenate(face).astype(np.int64) if face else np.zeros(0, np.int64),
            np.asarray(flags, dtype=bool))


def areas(face_area, ptr, face) -> np.ndarray:
    """A_s of every source: definition 3."""
    return np.array([K.mesh_sum(face_area[face[ptr[s]:ptr[s + 1]]]) for s in range(len(ptr) - 1)])


def weights(face_area, ptr, face, A) -> np.ndarray:
    """area_f / A_s of every list entry."""
    return face_area[face] / np.repeat(A, np.diff(ptr))


def load(n_pot: int, tri, face_area, ptr, face, A, power) -> np.ndarray:
    """Definition 5 for one column, ``power`` (n_source,): what is added to b."""
    per_face: dict = {}
    for s in range(len(ptr) - 1):                            # ascending s: the sources of a face come out ascending
        for f in face[ptr[s]:ptr[s + 1]]:
            per_face.setdefault(int(f), []).append(s)
    c = T.corners(tri)
    acc = np.zeros(int(n_pot))
    for f in sorted(per_face):                               # ascending f: the faces of a vertex come in ascending order
        for s in per_face[f]:
            term = ((face_area[f] / A[s]) * power[s]) / 3
            for v in c[f]:
                acc[v] = acc[v] + term
    return acc


def footprint_temperature(tri, face_area, ptr, face, A, theta, ambient: float) -> np.ndarray:
    """Definition 6 for one column ``theta`` (n_pot,): T_s of every source."""
    c = T.corners(tri)
    mean = ((theta[c[:, 0]] + theta[c[:, 1]]) + theta[c[:, 2]]) / 3
    out = np.zeros(len(ptr) - 1)
    for s in range(len(ptr) - 1):
        mine = face[ptr[s]:ptr[s + 1]]
        out[s] = ambient + K.mesh_sum((face_area[mine] / A[s]) * mean[mine])
    return out


class Restated:
    """Everything of a set of sources on a board, computed once: lists, flags, areas."""

    def __init__(self, meshes, mesh_layer, sources):
        self.xy, self.tri, _fm, self.voff, self.toff = T.flatten(meshes)
        self.face_area = T.face_area(self.xy, self.tri)
        self.ptr, self.face, self.fallback = lists(meshes, mesh_layer, sources)
        self.A = areas(self.face_area, self.ptr, self.face)
        self.counts = np.diff(self.ptr)

    def load(self, n_pot, power) -> np.ndarray:
        """(k, n_pot) for ``power`` (k, n_source)."""
        return np.stack([load(n_pot, self.tri, self.face_area, self.ptr, self.face, self.A, p) for p in np.atleast_2d(power)])

    def temperature(self, theta, ambient: float) -> np.ndarray:
        return np.stack([footprint_temperature(self.tri, self.face_area, self.ptr, self.face, self.A, th, ambient)
                         for th in np.atleast_2d(theta)])

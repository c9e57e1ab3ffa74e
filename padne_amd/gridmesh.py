"""The grid mesher: first meshes of polygons with holes, on the device ("Grid mesher").

The reference meshes with CGAL (``mesh.py:662-795``, out of scope).  :class:`GridMesher` is not a replacement for it: it is
isosurface stuffing on a uniform lattice -- sign of every lattice vertex by the even-odd rule, cuts on the lattice edges the
boundary crosses, lattice vertices close to a cut snapped onto the boundary, the mixed triangles clipped
(``csrc/polymesh.hip``, ``padne_polymesh_create``).  What it does not do, and what follows from that:

* corners of the polygon are cut off at the scale of the spacing; no vertex is placed on them;
* a feature narrower than about one cell is lost.  That shows only as a mesh in several pieces (``crumbs``) or as a seed
  point far from every vertex; both raise :class:`padne_amd.mesh.MeshingException`;
* faces along the boundary may be obtuse, so the stiffness matrix has positive off-diagonal entries there (the ``|cot|``
  caveat of the README applies);
* the spacing is uniform unless ``graded=True``: then the interior is coarsened by a balanced quadtree over the lattice's
  cells, by the variable-density fields of ``Mesher.Config`` (``padne_polymesh_create_graded``; DESIGN.md, "Graded grid
  mesher").  ``minimum_angle`` and ``distance_map_quantization`` are accepted and ignored either way;
* one GPU.

``refine_meshes`` and the adaptive loops of the solver improve such a first mesh where the error estimate asks.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional, Sequence

import numpy as np

from . import mesh, structured

LOWER = "lower maximum_size (or the spacing)"


class _Ring:
    """``.coords`` of a ring, closed as shapely closes it (the first vertex repeated at the end)."""

    def __init__(self, coords):
        pts = [(float(x), float(y)) for x, y in coords]
        if len(pts) > 1 and pts[0] != pts[-1]:
            pts.append(pts[0])
        self.coords = pts


class Polygon:
    """An exterior ring and hole rings, with the two attributes of shapely's Polygon that meshers read:
    ``.exterior.coords`` and ``.interiors``.  ``structured.Shapes.of(Polygon(...))`` is a layer's shape."""

    def __init__(self, exterior, holes=()):
        self.exterior = _Ring(exterior)
        self.interiors = tuple(_Ring(hole) for hole in holes)

    def contains_xy(self, x, y) -> bool:
        return bool(_inside(_segments(rings_of(self)), np.array([float(x)]), np.array([float(y)]))[0])


def rings_of(poly) -> list:
    """The rings of ``poly`` (a ``structured.Rect``, or anything with ``.exterior.coords`` and ``.interiors``) as (n, 2)
    arrays, the exterior first, a closing duplicate vertex dropped."""
    if isinstance(poly, structured.Rect):
        raw = [[(poly.x0, poly.y0), (poly.x1, poly.y0), (poly.x1, poly.y1), (poly.x0, poly.y1)]]
    elif hasattr(poly, "exterior") and hasattr(poly, "interiors"):
        raw = [list(poly.exterior.coords)] + [list(ring.coords) for ring in poly.interiors]
    else:
        raise mesh.MeshingException(f"GridMesher cannot mesh {type(poly).__name__}: it takes a Rect, or an object with "
                                    ".exterior.coords and .interiors")
    rings = []
    for ring in raw:
        r = np.array([(float(p[0]), float(p[1])) for p in ring], dtype=np.float64).reshape(-1, 2)
        if len(r) > 1 and np.array_equal(r[0], r[-1]):
            r = r[:-1]
        if len(r) < 3:
            raise ValueError("a ring needs at least 3 distinct vertices")
        if not np.isfinite(r).all():
            raise ValueError("a coordinate of a ring is not finite")
        rings.append(r)
    return rings


def _segments(rings) -> np.ndarray:
    return np.concatenate([np.concatenate([np.roll(r, 1, axis=0), r], axis=1) for r in rings])


def _inside(seg, x, y) -> np.ndarray:
    """The even-odd rule of the kernels, for the host checks (seeds)."""
    cx, cy = np.asarray(x, dtype=np.float64)[:, None], np.asarray(y, dtype=np.float64)[:, None]
    xj, yj, xi, yi = seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        cross = ((yi > cy) != (yj > cy)) & (cx < (xj - xi) * (cy - yi) / (yj - yi) + xi)
    return (cross.sum(axis=1) & 1) == 1


def _polygon_area(rings) -> float:
    total = 0.0
    for k, r in enumerate(rings):
        a = 0.5 * abs(float(np.sum(r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1])))
        total += a if k == 0 else -a
    return total


def _face_components(n_vert: int, tri: np.ndarray):
    """(number of connected components, the component of every face), labelled with scipy on the fetched arrays.  Faces are
    connected through shared edges: two pieces that touch in one vertex are two components."""
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    t = tri.astype(np.int64)
    u, v = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    key = np.minimum(u, v) * n_vert + np.maximum(u, v)
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    a, b = order[:-1][same] // 3, order[1:][same] // 3
    graph = sp.coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(len(t), len(t)))
    n, face_label = csgraph.connected_components(graph, directed=False)
    return n, face_label


def _device_engine(polygons, h, snap):
    from . import _hip, solver
    return _hip.polymesh(solver.get_context(), polygons, h, snap)


def _device_engine_graded(polygons, h, snap, thresholds, seeds):
    from . import _hip, solver
    return _hip.polymesh_graded(solver.get_context(), polygons, h, snap, thresholds, seeds)


MAX_LEVEL = 5           # padne_polymesh_create_graded takes at most 6 levels, 0 to 5


def graded_thresholds(h: float, factor: float, min_distance: float, max_distance: float, max_level: int = MAX_LEVEL) -> list:
    """The thresholds ``t`` of ``padne_polymesh_create_graded``, in cells of spacing ``h``.  The size is to grow linearly from
    ``maximum_size`` at ``min_distance`` from the boundary to ``factor * maximum_size`` at ``max_distance``; a leaf of level l
    has ``2^l`` times the size, so level ``l >= 1`` exists while ``2^l <= factor`` and ``l <= max_level`` and needs the
    distance ``dist_l = min_distance + (2^l - 1) / (factor - 1) * (max_distance - min_distance)``.  A cell at Chebyshev
    distance d from a cell the boundary touches is at least ``(d - 1) h`` from the boundary, hence
    ``t[l] = max(t[l - 1] + 2^(l - 1), 1 + ceil(dist_l / h))``; the first term keeps the quadtree balanced.  ``factor < 2``
    gives ``[0]``: the uniform mesh."""
    t = [0]
    level = 1
    while 2 ** level <= factor and level <= max_level:
        dist = min_distance + (2 ** level - 1) / (factor - 1) * (max_distance - min_distance)
        cells = 1 + math.ceil(dist / h)
        if not cells < 2 ** 30:
            raise ValueError(f"level {level} would start {dist / h:g} cells from the boundary: the spacing is too small for "
                             "these variable-density distances")
        t.append(max(t[-1] + 2 ** (level - 1), cells))
        level += 1
    return t


class GridMesher:
    """``poly_to_mesh(poly, seed_points)`` for ``solver.solve(prob, mesher=GridMesher(config))``, and
    ``polys_to_meshes(polys, seed_points)``, which meshes a batch in one device call.

    ``config``: a ``mesh.Mesher.Config``; only ``maximum_size`` is read, the spacing is ``maximum_size / sqrt(2)`` so that the
    longest lattice edge is ``maximum_size`` (an edge next to the boundary may reach ``(1 + 2 snap) maximum_size``).
    ``minimum_angle`` and the variable-density fields are accepted and ignored (the latter unless ``graded``).  ``spacing``
    overrides the lattice spacing;
    seeds are then held to ``sqrt(2) spacing``.  ``snap`` in (0, 1/2).  ``area_tolerance``: when given, mesh area over polygon
    area must lie within ``1 +- area_tolerance`` (no default).  ``crumbs``: ``"raise"`` when the mesh has more than one
    connected component, ``"drop"`` to keep the component with the most faces (the lowest label on a tie).
    ``engine``: what computes the lattice work, ``(polygons, h, snap) -> [(xy, tri, kind)]``; the device by default -- the
    tests hand in their host restatement of the kernels.

    ``graded=True`` (off by default) coarsens the interior: a balanced quadtree over the cells the boundary does not touch,
    leaves of ``2^l x 2^l`` cells, right-isosceles faces.  ``variable_size_maximum_factor``, ``variable_density_min_distance``
    and ``variable_density_max_distance`` of the config give the thresholds (:func:`graded_thresholds`); levels are powers of
    two, so the reference's default factor 3 gives one level, and ``max_level`` (0 to 5) caps them.  Distances are counted in
    cells (Chebyshev), not Euclidean.  Seeds are fine spots: the cell of a seed stays at level 0 and the levels grow away from
    it as from the boundary.  ``distance_map_quantization`` and ``minimum_angle`` stay ignored.  The engine is then called as
    ``(polygons, h, snap, thresholds, seeds) -> [(xy, tri, kind, cells_per_level)]``.

    ``last_report``: per polygon of the last call a dict with ``lattice`` (nx, ny), ``vertices`` {"lattice", "snapped",
    "cut"}, ``faces``, ``area_ratio`` and ``components`` (before any crumbs were dropped); with ``graded`` also
    ``thresholds`` and ``cells_per_level``, the lattice's cells by level.
    """

    def __init__(self, config: Optional[mesh.Mesher.Config] = None, *, spacing: Optional[float] = None, snap: float = 0.25,
                 area_tolerance: Optional[float] = None, crumbs: str = "raise", engine=None, graded: bool = False,
                 max_level: int = MAX_LEVEL):
        self.config = config if config is not None else mesh.Mesher.Config()
        if spacing is not None and not (spacing > 0 and math.isfinite(spacing)):
            raise ValueError(f"spacing must be positive, got {spacing}")
        if not 0 < snap < 0.5:
            raise ValueError(f"snap must lie in (0, 1/2), got {snap}")
        if crumbs not in ("raise", "drop"):
            raise ValueError(f"crumbs must be 'raise' or 'drop', got {crumbs!r}")
        if area_tolerance is not None and not area_tolerance > 0:
            raise ValueError(f"area_tolerance must be positive, got {area_tolerance}")
        self.spacing, self.snap, self.area_tolerance, self.crumbs = spacing, float(snap), area_tolerance, crumbs
        if not (isinstance(max_level, (int, np.integer)) and not isinstance(max_level, bool) and 0 <= max_level <= MAX_LEVEL):
            raise ValueError(f"max_level must be an integer from 0 to {MAX_LEVEL}, got {max_level!r}")
        self.graded, self.max_level = bool(graded), int(max_level)
        self.engine = engine if engine is not None else (_device_engine_graded if self.graded else _device_engine)
        self.last_report: list = []

    def _sizes(self):
        """(lattice spacing, how far a seed may be from the nearest vertex)."""
        if self.spacing is not None:
            return float(self.spacing), math.sqrt(2.0) * float(self.spacing)
        if self.config.maximum_size == 0:
            raise mesh.MeshingException("GridMesher needs a maximum_size above 0, or a spacing: the lattice is uniform")
        return self.config.maximum_size / math.sqrt(2.0), float(self.config.maximum_size)

    def thresholds(self) -> list:
        """The thresholds of the levels at this mesher's spacing (``[0]`` when it is not graded)."""
        if not self.graded:
            return [0]
        h, _reach = self._sizes()
        c = self.config
        return graded_thresholds(h, c.variable_size_maximum_factor, c.variable_density_min_distance,
                                 c.variable_density_max_distance, self.max_level)

    def poly_to_mesh(self, poly, seed_points: Iterable = ()) -> mesh.Mesh:
        return self.polys_to_meshes([poly], seed_points)[0]

    def polys_to_meshes(self, polys: Sequence, seed_points: Iterable = ()) -> list:
        h, reach = self._sizes()
        polygons = [rings_of(poly) for poly in polys]
        self.last_report = []
        if not polygons:
            return []
        seeds = np.array([(p.x, p.y) if hasattr(p, "x") else (p[0], p[1]) for p in seed_points], dtype=np.float64).reshape(-1, 2)
        meshes = []
        if self.graded:
            if not np.isfinite(seeds).all():
                raise ValueError("a seed point is not finite")
            t = self.thresholds()
            for k, (rings, (xy, tri, kind, cells)) in enumerate(zip(polygons, self.engine(polygons, h, self.snap, t, seeds))):
                meshes.append(self._checked(k, rings, np.asarray(xy), np.asarray(tri), np.asarray(kind), seeds, h, reach,
                                            {"thresholds": list(t), "cells_per_level": [int(c) for c in cells]}))
            return meshes
        for k, (rings, (xy, tri, kind)) in enumerate(zip(polygons, self.engine(polygons, h, self.snap))):
            meshes.append(self._checked(k, rings, np.asarray(xy), np.asarray(tri), np.asarray(kind), seeds, h, reach))
        return meshes

    def _checked(self, k, rings, xy, tri, kind, seeds, h, reach, extra=None) -> mesh.Mesh:
        pts = np.concatenate(rings)
        nx = int(math.ceil(pts[:, 0].max() / h)) + 1 - (int(math.floor(pts[:, 0].min() / h)) - 1) + 1
        ny = int(math.ceil(pts[:, 1].max() / h)) + 1 - (int(math.floor(pts[:, 1].min() / h)) - 1) + 1
        report = {"lattice": (nx, ny), "vertices": {"lattice": int((kind == 0).sum()), "snapped": int((kind == 1).sum()),
                                                    "cut": int((kind == 2).sum())},
                  "faces": len(tri), "area_ratio": 0.0, "components": 0, **(extra or {})}
        self.last_report.append(report)
        if len(tri) == 0:
            raise mesh.MeshingException(f"polygon {k}: no lattice vertex of spacing {h:g} lies inside it, the mesh has no face; {LOWER}")
        a, b, c = xy[tri[:, 0]], xy[tri[:, 1]], xy[tri[:, 2]]
        area = 0.5 * ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))
        report["area_ratio"] = float(area.sum() / _polygon_area(rings))
        n_comp, face_label = _face_components(len(xy), tri)
        report["components"] = n_comp
        if n_comp > 1:
            if self.crumbs == "raise":
                raise mesh.MeshingException(f"polygon {k}: the mesh falls into {n_comp} pieces, a feature is narrower than about "
                                            f"one cell of spacing {h:g}; {LOWER}, or pass crumbs='drop' to keep the largest piece")
            sizes = np.bincount(face_label)
            tri = tri[face_label == int(np.argmax(sizes))]
            keep = np.zeros(len(xy), dtype=bool)
            keep[tri.reshape(-1)] = True
            number = np.cumsum(keep) - 1
            xy, kind, tri = xy[keep], kind[keep], number[tri].astype(np.int32)
        if self.area_tolerance is not None and abs(report["area_ratio"] - 1.0) > self.area_tolerance:
            raise mesh.MeshingException(f"polygon {k}: mesh area over polygon area is {report['area_ratio']:.6f}, outside "
                                        f"1 +- {self.area_tolerance:g}; {LOWER}")
        if len(seeds):
            inside = seeds[_inside(_segments(rings), seeds[:, 0], seeds[:, 1])]
            if len(inside):
                import scipy.spatial
                dist, _ = scipy.spatial.cKDTree(xy).query(inside)
                if (dist > reach).any():
                    worst = inside[int(np.argmax(dist))]
                    raise mesh.MeshingException(f"polygon {k}: the seed point ({worst[0]:g}, {worst[1]:g}) lies inside it but "
                                                f"{dist.max():g} from the nearest mesh vertex (more than {reach:g}): the copper "
                                                f"around it was lost; {LOWER}")
        return mesh.Mesh(np.ascontiguousarray(xy), np.ascontiguousarray(tri, dtype=np.int32))

"""The graded grid mesher restated in numpy ("Graded grid mesher"): the specification of the bits of
``padne_polymesh_create_graded``.  It builds on ``gridmesh_ref.mesh_polygon``: steps 1 to 4 (lattice, sign, cuts, snap) are
that function's, and so is every face of a level 0 cell.

  plain     a cell (ci, cj) of the lattice's (nx - 1) x (ny - 1) cells is plain when its four corners have state +; a seed
            (x, y) makes the cell (floor(x / h) - i0, floor(y / h) - j0) not plain when that cell is in the lattice; cells
            outside the lattice are not plain;
  distance  d(c) = the Chebyshev distance, in cells, from c to the nearest cell that is not plain, capped at t[n_level - 1];
  level     of a cell: the largest l < n_level such that the block of 2^l x 2^l cells that contains it -- aligned at global
            cell indices, (i0 + ci) and (j0 + cj) rounded down to multiples of 2^l by floor division -- lies wholly in the
            lattice and min d over it is at least t[l].  Such a block is a leaf.  t[0] = 0, t[l] >= t[l - 1] + 2^(l - 1);
  faces     a level 0 cell emits what it emits in the uniform mesh.  Of a leaf of level l >= 1 only the anchor (lower left)
            cell emits, from the leaf's corners v00, v10, v11, v01: a side hangs when the cell across it (at the anchor's end of
            the side) has a lower level; no side hangs: (v00, v10, v11), (v00, v11, v01); otherwise with the centre lattice
            vertex c and the ring v00, [mid S], v10, [mid E], v11, [mid N], v01, [mid W] (a midpoint on a hanging side only):
            (c, ring[k], ring[k + 1]) cyclically from v00;
  numbers   the slots some face names in ascending slot order, the faces in cell order, a leaf's at its anchor cell.

Every vertex of a leaf is a corner of a plain cell, which the uniform mesh names too: the graded mesh is the uniform mesh with
the two faces of every cell of a leaf taken out, the leaf's faces put in where its anchor cell's two faces stood, and the
vertices no face names any more dropped."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import gridmesh_ref as G

MAX_LEVELS = 6
SIDES = ("S", "E", "N", "W")


def check_thresholds(t):
    t = [int(x) for x in t]
    if not 1 <= len(t) <= MAX_LEVELS or t[0] != 0:
        raise ValueError("1 to 6 thresholds, the first of them 0")
    for l in range(1, len(t)):
        if t[l] < t[l - 1] + 2 ** (l - 1):
            raise ValueError("t[l] >= t[l - 1] + 2^(l - 1)")
    return t


def plain_cells(m, seeds=()):
    i0, j0, nx, ny = m.lattice
    plus = m.state == G.PLUS
    plain = plus[:-1, :-1] & plus[:-1, 1:] & plus[1:, 1:] & plus[1:, :-1]
    for x, y in np.asarray(seeds, dtype=np.float64).reshape(-1, 2):
        if not (math.isfinite(x) and math.isfinite(y)):
            raise ValueError("a seed is not finite")
        fi, fj = np.floor(x / m.h) - i0, np.floor(y / m.h) - j0
        if 0 <= fi < nx - 1 and 0 <= fj < ny - 1:
            plain[int(fj), int(fi)] = False
    return plain


def distance(plain, cap):
    """Chebyshev distance to the nearest cell that is not plain (cells outside count as not plain), capped: grown ring by
    ring from the cells that are not plain."""
    rows, cols = plain.shape
    d = np.full((rows, cols), cap, dtype=np.int32)
    if cap == 0:
        return d
    reached = np.ones((rows + 2 * cap, cols + 2 * cap), dtype=bool)
    reached[cap:cap + rows, cap:cap + cols] = ~plain
    inner = (slice(cap, cap + rows), slice(cap, cap + cols))
    done = np.zeros((rows, cols), dtype=bool)
    for k in range(cap):
        new = reached[inner] & ~done
        d[new] = k
        done |= new
        grown = reached.copy()
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                grown[1:-1, 1:-1] |= reached[1 + dj:reached.shape[0] - 1 + dj, 1 + di:reached.shape[1] - 1 + di]
        reached = grown
    return d


def levels(d, i0, j0, t):
    rows, cols = d.shape
    level = np.zeros((rows, cols), dtype=np.int8)
    for l in range(1, len(t)):
        s = 2 ** l
        a0, b0 = (-i0) % s, (-j0) % s                   # the first aligned block: (i0 + a0) % s == 0, with floor division
        nbx, nby = (cols - a0) // s, (rows - b0) // s
        if nbx <= 0 or nby <= 0:
            continue
        block = d[b0:b0 + nby * s, a0:a0 + nbx * s].reshape(nby, s, nbx, s).min(axis=(1, 3))
        ok = np.repeat(np.repeat(block >= t[l], s, axis=0), s, axis=1)
        level[b0:b0 + nby * s, a0:a0 + nbx * s][ok] = l
    return level


def mesh_polygon_graded(poly, h, thresholds, seeds=(), snap=0.25, uniform=None):
    """Returns a namespace: xy, tri, kind as ``mesh_polygon``; ``uniform`` that mesh; ``plain``, ``d``, ``level`` per cell;
    ``cells_per_level``; ``leaves`` [(ci, cj, l, mask)] with bit k of mask set when side SIDES[k] hangs; ``leaf_face`` (one
    flag per face) and ``leaf_tri_ij`` (k, 3, 2), the corners of the leaves' faces as lattice indices."""
    t = check_thresholds(thresholds)
    m = uniform if uniform is not None else G.mesh_polygon(poly, h, snap)
    i0, j0, nx, ny = m.lattice
    plain = plain_cells(m, seeds)
    d = distance(plain, t[-1])
    level = levels(d, i0, j0, t)
    cells_per_level = np.bincount(level.reshape(-1), minlength=len(t)).astype(np.int64)
    if not level.any():
        return SimpleNamespace(xy=m.xy, tri=m.tri, kind=m.kind, uniform=m, plain=plain, d=d, level=level, leaves=[],
                               cells_per_level=cells_per_level, leaf_face=np.zeros(len(m.tri), dtype=bool),
                               leaf_tri_ij=np.zeros((0, 3, 2), dtype=np.int64), lattice=m.lattice)

    # ---- the uniform mesh's number of every unsnapped + lattice vertex, by its exact coordinates
    X = (i0 + np.arange(nx)).astype(np.float64) * m.h
    Y = (j0 + np.arange(ny)).astype(np.float64) * m.h
    vid = np.full((ny, nx), -1, dtype=np.int64)
    lat = np.flatnonzero(m.kind == 0)
    li = np.rint(m.xy[lat, 0] / m.h).astype(np.int64) - i0
    lj = np.rint(m.xy[lat, 1] / m.h).astype(np.int64) - j0
    assert np.array_equal(X[li], m.xy[lat, 0]) and np.array_equal(Y[lj], m.xy[lat, 1])
    vid[lj, li] = lat

    # ---- where the two faces of every plain cell stand in the uniform mesh
    n = len(m.xy)
    key = (m.tri[:, 0].astype(np.int64) * n + m.tri[:, 1]) * n + m.tri[:, 2]
    order = np.argsort(key, kind="stable")

    def lower_face_of(ci, cj):
        n00, n10, n11, n01 = vid[cj, ci], vid[cj, ci + 1], vid[cj + 1, ci + 1], vid[cj + 1, ci]
        assert (np.stack([n00, n10, n11, n01]) >= 0).all()
        want = (n00 * n + n10) * n + n11
        at = order[np.searchsorted(key[order], want)]
        assert np.array_equal(key[at], want)
        assert np.array_equal(m.tri[at + 1], np.stack([n00, n11, n01], axis=1))
        return at

    cj_all, ci_all = np.nonzero(level > 0)
    gone = lower_face_of(ci_all, cj_all)
    keep = np.ones(len(m.tri), dtype=bool)
    keep[gone] = keep[gone + 1] = False

    # ---- the leaves
    padded = np.zeros((ny + 1, nx + 1), dtype=np.int8)              # level 0 round the lattice's cells
    padded[1:ny, 1:nx] = level

    def level_at(ci, cj):
        return int(padded[cj + 1, ci + 1])
    leaves, new_faces, new_at, new_ij = [], [], [], []
    for cj, ci in zip(cj_all.tolist(), ci_all.tolist()):
        l = int(level[cj, ci])
        s = 2 ** l
        if (i0 + ci) % s or (j0 + cj) % s:
            continue
        hang = [level_at(ci, cj - 1) < l, level_at(ci + s, cj) < l, level_at(ci, cj + s) < l, level_at(ci - 1, cj) < l]
        mask = sum(1 << k for k in range(4) if hang[k])
        leaves.append((ci, cj, l, mask))
        v00, v10, v11, v01 = (ci, cj), (ci + s, cj), (ci + s, cj + s), (ci, cj + s)
        if mask == 0:
            faces = [(v00, v10, v11), (v00, v11, v01)]
        else:
            half = s // 2
            mids = [(ci + half, cj), (ci + s, cj + half), (ci + half, cj + s), (ci, cj + half)]
            ring = []
            for k, corner in enumerate((v00, v10, v11, v01)):
                ring.append(corner)
                if hang[k]:
                    ring.append(mids[k])
            c = (ci + half, cj + half)
            faces = [(c, ring[k], ring[(k + 1) % len(ring)]) for k in range(len(ring))]
        (at,) = lower_face_of(np.array([ci]), np.array([cj]))
        for f in faces:
            ids = [int(vid[p[1], p[0]]) for p in f]
            assert min(ids) >= 0
            new_faces.append(ids)
            new_at.append(at)
            new_ij.append(f)

    # ---- faces in cell order (a leaf's where its anchor's stood), vertices in slot order
    old = np.flatnonzero(keep)
    faces = np.concatenate([m.tri[old].astype(np.int64), np.array(new_faces, dtype=np.int64).reshape(-1, 3)])
    at = np.concatenate([old, np.array(new_at, dtype=np.int64)])
    sub = np.concatenate([np.zeros(len(old), dtype=np.int64), np.arange(len(new_at))])
    is_leaf = np.concatenate([np.zeros(len(old), dtype=bool), np.ones(len(new_at), dtype=bool)])
    by = np.lexsort((sub, at))
    faces, is_leaf = faces[by], is_leaf[by]
    used = np.zeros(n, dtype=bool)
    used[faces.reshape(-1)] = True
    number = np.cumsum(used) - used
    return SimpleNamespace(xy=np.ascontiguousarray(m.xy[used]), tri=number[faces].astype(np.int32).reshape(-1, 3),
                           kind=np.ascontiguousarray(m.kind[used]), uniform=m, plain=plain, d=d, level=level, leaves=leaves,
                           cells_per_level=cells_per_level, leaf_face=is_leaf,
                           leaf_tri_ij=np.array(new_ij, dtype=np.int64).reshape(-1, 3, 2), lattice=m.lattice)


def host_thresholds(h, factor, dmin, dmax, max_level=5):
    """The thresholds ``GridMesher(graded=True)`` forms, restated: level l >= 1 exists while 2^l <= factor and l <= max_level;
    dist_l = dmin + (2^l - 1) / (factor - 1) * (dmax - dmin); t[l] = max(t[l - 1] + 2^(l - 1), 1 + ceil(dist_l / h))."""
    t = [0]
    l = 1
    while 2 ** l <= factor and l <= max_level:
        dist = dmin + (2 ** l - 1) / (factor - 1) * (dmax - dmin)
        t.append(max(t[-1] + 2 ** (l - 1), 1 + math.ceil(dist / h)))
        l += 1
    return t


def boundary_edges(xy, tri):
    """The boundary half-edges (directed edges without a twin) as a set of coordinate pairs."""
    t = np.asarray(tri, dtype=np.int64)
    u, v = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    n = len(xy)
    twinless = ~np.isin(v * n + u, u * n + v)
    return {(tuple(xy[a]), tuple(xy[b])) for a, b in zip(u[twinless].tolist(), v[twinless].tolist())}

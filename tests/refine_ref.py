"""Host restatement of the refinement rule ("Refinement"): 4-triangle longest-edge refinement with conforming
closure, in numpy, for the tests.  Nothing here calls the library.  All meshes of a call are one batch: vertices and faces
are numbered globally in mesh order, edges are the distinct keys lo * n_vert + hi in ascending order."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np


@dataclass
class Edges:
    lo: np.ndarray            # (n_edges,) global vertex, lo < hi
    hi: np.ndarray
    of_face: np.ndarray       # (n_tri, 3): the edge of corner c, (tri[f, c], tri[f, (c + 1) % 3])
    uses: np.ndarray          # (n_edges,) corners on the edge: 1 = boundary, 2 = interior
    d: np.ndarray             # (n_edges,) squared length, from lo to hi
    longest: np.ndarray       # (n_tri,) the corner of the face's longest edge


@dataclass
class Refined:
    meshes: list              # per mesh (points (n, 2) float64, triangles (k, 3) int32, mesh-local)
    parents: list             # per mesh (k,) int32: the parent face, mesh-local
    midpoint_ends: list       # per mesh (n_new, 2) int32: the (lo, hi) ends of every new vertex, mesh-local
    edges: Edges
    marks_flagged: np.ndarray  # (n_edges,) bool: the edges of the flagged faces
    marks: np.ndarray          # (n_edges,) bool: after the closure
    sweeps: int


def flatten(meshes):
    """[(points, triangles)] -> (xy, global tri int64, voff, toff)."""
    voff = np.concatenate([[0], np.cumsum([len(p) for p, _ in meshes])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(t) for _, t in meshes])]).astype(np.int64)
    xy = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p, _ in meshes]) if meshes else np.zeros((0, 2))
    tri = (np.concatenate([np.asarray(t, dtype=np.int64).reshape(-1, 3) + voff[i] for i, (_, t) in enumerate(meshes)])
           if meshes else np.zeros((0, 3), dtype=np.int64))
    return xy, tri, voff, toff


def edges_of(xy, tri) -> Edges:
    n_vert = len(xy)
    u, v = tri, tri[:, [1, 2, 0]]
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    if (lo == hi).any():
        raise ValueError("a face names a vertex twice")
    keys, inv, uses = np.unique((lo * n_vert + hi).reshape(-1), return_inverse=True, return_counts=True)
    inv = inv.reshape(-1, 3)
    forward = np.bincount(inv.reshape(-1), weights=(u < v).reshape(-1), minlength=len(keys))
    if (uses > 2).any() or (forward > 1).any() or (uses - forward > 1).any():
        raise ValueError("Non-manifold mesh")
    e_lo, e_hi = keys // max(n_vert, 1), keys % max(n_vert, 1)
    dx, dy = xy[e_hi, 0] - xy[e_lo, 0], xy[e_hi, 1] - xy[e_lo, 1]
    d = dx * dx + dy * dy
    best = np.zeros(len(tri), dtype=np.int64)
    rows = np.arange(len(tri))
    for c in (1, 2):
        dc, db = d[inv[:, c]], d[inv[rows, best]]
        better = (dc > db) | ((dc == db) & (inv[:, c] < inv[rows, best]))
        best = np.where(better, c, best)
    return Edges(e_lo, e_hi, inv, uses, d, best)


def close_marks(E: Edges, marks):
    """The least fixed point by whole sweeps over all faces (each sweep reads the marks of the sweep before).  Returns
    (marks, sweeps that changed something)."""
    marks = marks.copy()
    rows = np.arange(len(E.of_face))
    longest_edge = E.of_face[rows, E.longest] if len(rows) else np.zeros(0, dtype=np.int64)
    sweeps = 0
    while True:
        want = marks[E.of_face].any(axis=1) & ~marks[longest_edge]
        if not want.any():
            return marks, sweeps
        marks[longest_edge[want]] = True
        sweeps += 1


def close_marks_worklist(E: Edges, marks):
    """The same fixed point in another order: one face at a time from a stack, the last face first, each face seeing every
    mark made so far."""
    marks = marks.copy()
    faces_of = [[] for _ in range(len(marks))]
    for f, row in enumerate(E.of_face):
        for e in row:
            faces_of[e].append(f)
    stack = list(range(len(E.of_face)))
    while stack:
        f = stack.pop()
        e_long = E.of_face[f, E.longest[f]]
        if marks[E.of_face[f]].any() and not marks[e_long]:
            marks[e_long] = True
            stack.extend(faces_of[e_long])
    return marks


def refine(meshes, flags) -> Refined:
    """One round on ``meshes`` = [(points, triangles)] with ``flags`` = one boolean array per mesh."""
    xy, tri, voff, toff = flatten(meshes)
    flag = np.concatenate([np.asarray(f, dtype=bool).reshape(-1) for f in flags]) if len(flags) else np.zeros(0, dtype=bool)
    assert len(flag) == len(tri)
    n_mesh = len(meshes)
    E = edges_of(xy, tri)
    n_edges = len(E.lo)
    marks0 = np.zeros(n_edges, dtype=bool)
    marks0[E.of_face[flag].reshape(-1)] = True
    marks, sweeps = close_marks(E, marks0)
    # new vertices: one per marked edge, behind the old vertices of its mesh, in ascending edge number
    scan = np.concatenate([[0], np.cumsum(marks)]).astype(np.int64)
    edge_mesh = np.searchsorted(voff, E.lo, side="right") - 1
    eoff = np.searchsorted(E.lo, voff, side="left")                  # a mesh's edges are contiguous
    before = scan[eoff]                                               # marked edges of the meshes in front
    nv = np.diff(voff)
    new_local = nv[edge_mesh] + scan[:-1] - before[edge_mesh] if n_edges else np.zeros(0, dtype=np.int64)
    mid = 0.5 * (xy[E.lo] + xy[E.hi])
    # children
    rows = np.arange(len(tri))
    face_mesh = np.searchsorted(toff, rows, side="right") - 1
    L = E.longest
    base = voff[face_mesh]
    a, b, c = (tri[rows, (L + k) % 3] - base for k in range(3))
    eab, ebc, eca = (E.of_face[rows, (L + k) % 3] for k in range(3))
    mab, mbc, mca = marks[eab], marks[ebc], marks[eca]
    assert not ((mbc | mca) & ~mab).any()                             # the closure's fixed point
    m, p, q = new_local[eab], new_local[ebc], new_local[eca]
    t0, t1, t2 = (tri[:, k] - base for k in range(3))
    slots = np.zeros((len(tri), 4, 3), dtype=np.int64)
    live = np.zeros((len(tri), 4), dtype=bool)

    def put(slot, on, x, y, z):
        slots[on, slot, 0], slots[on, slot, 1], slots[on, slot, 2] = x[on], y[on], z[on]
        live[on, slot] = True

    put(0, ~mab, t0, t1, t2)
    put(0, mab & mca, a, m, q)
    put(0, mab & ~mca, a, m, c)
    put(1, mab & mca, q, m, c)
    put(2, mab & mbc, m, b, p)
    put(2, mab & ~mbc, m, b, c)
    put(3, mab & mbc, m, p, c)
    children = slots.reshape(-1, 3)[live.reshape(-1)]
    parent = np.repeat(rows, 4)[live.reshape(-1)]
    choff = np.concatenate([[0], np.cumsum(live.sum(axis=1))]).astype(np.int64)
    assert (live.sum(axis=1) == 1 + mab.astype(int) + mbc + mca).all()
    out_meshes, parents, ends = [], [], []
    for i in range(n_mesh):
        on = slice(eoff[i], eoff[i + 1])
        sel = np.flatnonzero(marks[on]) + eoff[i]
        pts = np.concatenate([xy[voff[i]:voff[i + 1]], mid[sel]])
        lo_c, hi_c = choff[toff[i]], choff[toff[i + 1]]
        out_meshes.append((pts, children[lo_c:hi_c].astype(np.int32)))
        parents.append((parent[lo_c:hi_c] - toff[i]).astype(np.int32))
        ends.append(np.stack([E.lo[sel] - voff[i], E.hi[sel] - voff[i]], axis=1).astype(np.int32))
    return Refined(out_meshes, parents, ends, E, marks0, marks, sweeps)


def signed_areas(points, triangles):
    p, t = np.asarray(points), np.asarray(triangles)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])) / 2


def smallest_angle(points, triangles) -> float:
    p, t = np.asarray(points), np.asarray(triangles)
    best = np.inf
    for k in range(3):
        o, u, v = p[t[:, k]], p[t[:, (k + 1) % 3]] - p[t[:, k]], p[t[:, (k + 2) % 3]] - p[t[:, k]]
        del o
        cross = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        dot = (u * v).sum(axis=1)
        best = min(best, float(np.abs(np.arctan2(cross, dot)).min()))
    return best

"""Host restatement of the field sampler for the tests (DESIGN.md "Sampling"): the owner rule by brute force over ALL faces
of the layer -- no bins, no index --, the potential by the written formula, and the owner's J and p with the arithmetic of
the face kernels.  The same orient() arithmetic as the device (no fused multiply-add in numpy), so every containment
decision and every value is the same bit for bit."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

CHUNK = 1 << 24          # point x face pairs evaluated at a time


@dataclass
class Board:
    """Meshes in the sampler's flat order (layer by layer, each layer's meshes in LayerSolution order)."""
    xy: np.ndarray         # (n_vert, 2) all vertices
    tri: np.ndarray        # (n_tri, 3) corners as GLOBAL vertex indices
    toff: np.ndarray       # (n_mesh + 1,) first face of each mesh
    voff: np.ndarray       # (n_mesh + 1,)
    sigma: np.ndarray      # (n_mesh,)
    layer_of: np.ndarray   # (n_mesh,)
    V: np.ndarray          # (n_vert,)

    def faces_of(self, layer: int) -> np.ndarray:
        """Global indices of the layer's faces, ascending."""
        return np.concatenate([np.arange(self.toff[m], self.toff[m + 1]) for m in range(len(self.sigma))
                               if self.layer_of[m] == layer] or [np.zeros(0, np.int64)]).astype(np.int64)

    def mesh_of(self, face):
        return np.searchsorted(self.toff, face, side="right") - 1


def board(meshes, potentials) -> Board:
    """``meshes``: (xy, tri, sigma, layer) in flat order; ``potentials``: one array per mesh."""
    voff = np.concatenate([[0], np.cumsum([len(m[0]) for m in meshes])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes])]).astype(np.int64)
    xy = np.concatenate([np.asarray(m[0], np.float64).reshape(-1, 2) for m in meshes] or [np.zeros((0, 2))])
    tri = np.concatenate([np.asarray(m[1], np.int64).reshape(-1, 3) + o for m, o in zip(meshes, voff)] or [np.zeros((0, 3), np.int64)])
    return Board(xy=xy, tri=tri, toff=toff, voff=voff, sigma=np.array([m[2] for m in meshes], np.float64),
                 layer_of=np.array([m[3] for m in meshes], np.int64),
                 V=np.concatenate([np.asarray(p, np.float64) for p in potentials] or [np.zeros(0)]))


def board_of_solution(sol) -> Board:
    meshes, pots = [], []
    for li, (layer, ls) in enumerate(zip(sol.problem.layers, sol.layer_solutions)):
        for msh, zf in zip(ls.meshes, ls.potentials):
            meshes.append((msh.points, msh.triangles, layer.conductance, li))
            pots.append(zf.values)
    return board(meshes, pots)


def orient(ax, ay, bx, by, px, py):
    """(b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x), elementwise, in that order."""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def edge_side(b: Board, i, k, qx, qy):
    """The side of q of the edge (i, k) as its face runs it: orient from the lower global vertex P to the higher Q, negated
    where the face runs it from Q to P.  i, k: (F,) global vertices; qx, qy: (P, 1); returns (P, F)."""
    fwd = i < k
    P, Q = np.where(fwd, i, k), np.where(fwd, k, i)
    o = orient(b.xy[P, 0], b.xy[P, 1], b.xy[Q, 0], b.xy[Q, 1], qx, qy)
    return np.where(fwd, o, -o)


def sides(b: Board, faces, q):
    """(o_a, o_b, o_c), each (len(q), len(faces)): the sides of the edges opposite corners a = tri[0], b = tri[1], c = tri[2]."""
    t = b.tri[faces]
    qx, qy = q[:, 0:1], q[:, 1:2]
    return (edge_side(b, t[:, 1], t[:, 2], qx, qy), edge_side(b, t[:, 2], t[:, 0], qx, qy),
            edge_side(b, t[:, 0], t[:, 1], qx, qy))


def contains(oa, ob, oc):
    return (((oa >= 0) & (ob >= 0) & (oc >= 0)) | ((oa <= 0) & (ob <= 0) & (oc <= 0))) & ~((oa == 0) & (ob == 0) & (oc == 0))


def owners(b: Board, layer: int, q) -> np.ndarray:
    """The owner of every point: the lowest global face of the layer that contains it, -1 for none.  Brute force."""
    q = np.asarray(q, np.float64).reshape(-1, 2)
    faces = b.faces_of(layer)
    out = np.full(len(q), -1, np.int64)
    if not len(faces):
        return out
    step = max(1, CHUNK // len(faces))
    for lo in range(0, len(q), step):
        inside = contains(*sides(b, faces, q[lo:lo + step]))
        first = inside.argmax(axis=1)                      # the first True: the lowest face
        out[lo:lo + step] = np.where(inside.any(axis=1), faces[first], -1)
    return out


def containing_counts(b: Board, layer: int, q) -> np.ndarray:
    """How many faces of the layer contain each point (1 inside a face, 2 on an edge, the fan at a vertex)."""
    q = np.asarray(q, np.float64).reshape(-1, 2)
    faces = b.faces_of(layer)
    out = np.zeros(len(q), np.int64)
    step = max(1, CHUNK // max(len(faces), 1))
    for lo in range(0, len(q), step):
        out[lo:lo + step] = contains(*sides(b, faces, q[lo:lo + step])).sum(axis=1)
    return out


def face_values(b: Board, faces):
    """(J (n, 2), p (n,)) of the given global faces: -sigma grad V and sigma |grad V|^2 with the face gradient of
    compute_triangle_gradient, corners visited as (tri[2], tri[0], tri[1])."""
    t = b.tri[faces]
    c1, c2, c3 = t[:, 2], t[:, 0], t[:, 1]
    x1, y1, x2, y2, x3, y3 = b.xy[c1, 0], b.xy[c1, 1], b.xy[c2, 0], b.xy[c2, 1], b.xy[c3, 0], b.xy[c3, 1]
    f1, f2, f3 = b.V[c1], b.V[c2], b.V[c3]

    def interp(x, y):
        D = (y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3)
        l1 = ((y2 - y3) * (x - x3) + (x3 - x2) * (y - y3)) / D
        l2 = ((y3 - y1) * (x - x3) + (x1 - x3) * (y - y3)) / D
        l3 = 1 - l1 - l2
        return l1 * f1 + l2 * f2 + l3 * f3
    with np.errstate(divide="ignore", invalid="ignore"):
        gx = interp(x1 + 1, y1) - f1
        gy = interp(x1, y1 + 1) - f1
    s = b.sigma[b.mesh_of(faces)]
    jx, jy = gx * s, gy * s
    return np.stack([-s * gx, -s * gy], axis=1), jx * gx + jy * gy


def sample(b: Board, layer: int, q):
    """(face (n,) global or -1, V (n,), J (n, 2), p (n,)) with NaN where there is no owner."""
    q = np.asarray(q, np.float64).reshape(-1, 2)
    face = owners(b, layer, q)
    n = len(q)
    V, J, p = np.full(n, np.nan), np.full((n, 2), np.nan), np.full(n, np.nan)
    hit = np.flatnonzero(face >= 0)
    if len(hit):
        f = face[hit]
        t = b.tri[f]
        qx, qy = q[hit, 0], q[hit, 1]
        oa, ob, oc = (edge_side(b, t[:, 1], t[:, 2], qx, qy), edge_side(b, t[:, 2], t[:, 0], qx, qy),
                      edge_side(b, t[:, 0], t[:, 1], qx, qy))
        s = (oa + ob) + oc
        V[hit] = ((oa / s) * b.V[t[:, 0]] + (ob / s) * b.V[t[:, 1]]) + (oc / s) * b.V[t[:, 2]]
        J[hit], p[hit] = face_values(b, f)
    return face, V, J, p


def raster_points(x0, y0, dx, dy, width, height) -> np.ndarray:
    """Pixel centres (height * width, 2), row j column i at j * width + i, by the stated expression."""
    xs = x0 + (np.arange(width) + 0.5) * dx
    ys = y0 + (np.arange(height) + 0.5) * dy
    return np.stack([np.tile(xs, height), np.repeat(ys, width)], axis=1)


# ---- point sets ------------------------------------------------------------------------------------------------------

def layer_vertices(b: Board, layer: int) -> np.ndarray:
    return np.concatenate([np.arange(b.voff[m], b.voff[m + 1]) for m in range(len(b.sigma)) if b.layer_of[m] == layer]
                          or [np.zeros(0, np.int64)]).astype(np.int64)


def special_points(b: Board, layer: int):
    """(every vertex, every edge midpoint, every face centroid) of the layer."""
    t = b.tri[b.faces_of(layer)]
    mids = np.concatenate([(b.xy[t[:, e]] + b.xy[t[:, (e + 1) % 3]]) / 2 for e in range(3)])
    cent = (b.xy[t[:, 0]] + b.xy[t[:, 1]] + b.xy[t[:, 2]]) / 3
    return b.xy[layer_vertices(b, layer)], mids, cent


def box_points(b: Board, layer: int, n: int, seed: int, grow: float = 0.2) -> np.ndarray:
    """Seeded random points in the bounding box of the layer's vertices grown by ``grow``."""
    pts = b.xy[layer_vertices(b, layer)]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    return np.random.default_rng(seed).uniform(lo - grow * (hi - lo), hi + grow * (hi - lo), size=(n, 2))


def interior_edges(b: Board, layer: int) -> np.ndarray:
    """(n, 2) global vertex pairs of the edges shared by two faces of the layer."""
    t = b.tri[b.faces_of(layer)]
    e = np.concatenate([np.stack([t[:, k], t[:, (k + 1) % 3]], axis=1) for k in range(3)])
    e.sort(axis=1)
    uniq, count = np.unique(e, axis=0, return_counts=True)
    return uniq[count == 2]


def on_edge_points(b: Board, layer: int, n: int, seed: int) -> np.ndarray:
    """Random convex combinations of the two ends of random interior edges, rounded as they fall."""
    rng = np.random.default_rng(seed)
    e = interior_edges(b, layer)
    pick = e[rng.integers(0, len(e), size=n)]
    w = rng.uniform(0.0, 1.0, size=(n, 1))
    return w * b.xy[pick[:, 0]] + (1 - w) * b.xy[pick[:, 1]]


# ---- what a point set holds (from the restatement's own answers) ------------------------------------------------------

def boundary_loops(b: Board, layer: int):
    """(edges (n, 2) global vertex pairs, loop (n,)): the edges that belong to one face only, labelled by the closed loop
    (connected component of the boundary) they lie on.  A mesh with a hole has two loops or more."""
    t = b.tri[b.faces_of(layer)]
    e = np.concatenate([np.stack([t[:, k], t[:, (k + 1) % 3]], axis=1) for k in range(3)])
    e.sort(axis=1)
    uniq, count = np.unique(e, axis=0, return_counts=True)
    edges = uniq[count == 1]
    root = {}

    def find(v):
        while root.setdefault(v, v) != v:
            root[v] = root[root[v]]
            v = root[v]
        return v
    for p, q in edges.tolist():
        root[find(p)] = find(q)
    label = np.array([find(p) for p in edges[:, 0].tolist()], dtype=np.int64)
    return edges, label


def in_a_hole(b: Board, layer: int, q) -> np.ndarray:
    """True for the points that lie inside two or more boundary loops of one mesh (even-odd rule per loop, a ray towards
    +x): inside the outline and inside a hole's rim.  Meant for points the rule gave no owner."""
    q = np.asarray(q, np.float64).reshape(-1, 2)
    edges, label = boundary_loops(b, layer)
    out = np.zeros(len(q), dtype=bool)
    if not len(edges) or not len(q):
        return out
    x1, y1, x2, y2 = b.xy[edges[:, 0], 0], b.xy[edges[:, 0], 1], b.xy[edges[:, 1], 0], b.xy[edges[:, 1], 1]
    px, py = q[:, 0:1], q[:, 1:2]
    with np.errstate(divide="ignore", invalid="ignore"):
        straddles = (y1 > py) != (y2 > py)
        crosses = straddles & (px < x1 + (py - y1) * (x2 - x1) / (y2 - y1))
    mesh_of_edge = np.searchsorted(b.voff, edges[:, 0], side="right") - 1
    for m in np.unique(mesh_of_edge):
        loops = np.unique(label[mesh_of_edge == m])
        inside = np.stack([crosses[:, label == k].sum(axis=1) % 2 == 1 for k in loops], axis=1)
        out |= inside.sum(axis=1) >= 2
    return out


def census(b: Board, layer: int, q) -> dict:
    """How many points of q are inside one face, on an edge (two faces contain them), at a vertex (three or more), outside
    the bounding box of the layer's vertices, and in a hole."""
    q = np.asarray(q, np.float64).reshape(-1, 2)
    counts = containing_counts(b, layer, q)
    pts = b.xy[layer_vertices(b, layer)]
    beyond = ((q < pts.min(axis=0)) | (q > pts.max(axis=0))).any(axis=1)
    return {"inside": int((counts == 1).sum()), "edge": int((counts == 2).sum()), "vertex": int((counts >= 3).sum()),
            "outside": int(((counts == 0) & beyond).sum()), "hole": int(in_a_hole(b, layer, q[counts == 0]).sum())}

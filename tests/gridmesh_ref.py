"""The grid mesher restated in numpy ("Grid mesher"): the specification of the bits of csrc/polymesh.hip.

One polygon = a list of rings (exterior, then holes), each an (n, 2) array without a closing duplicate.  Every expression
below is rounded as written; the device evaluates the same expressions in the same order (-ffp-contract=off).

  lattice   i0 = floor(xmin / h) - 1, nx = ceil(xmax / h) + 1 - i0 + 1 vertices per row, rows likewise; x_i = (i0 + i) * h;
  segments  segment k of a ring runs from vertex k - 1 (cyclic) P = (xj, yj) to vertex k Q = (xi, yi); it belongs to band j
            when min(yj, yi) <= Y[j + 1] and max(yj, yi) >= Y[j].  Row j and the edges that start in it read band j only;
  sign      + when the number of segments with (yi > cy) != (yj > cy) and cx < (xj - xi) * (cy - yi) / (yj - yi) + xi is odd;
  cut       of an edge A -> B (E, N, NE from A) whose ends differ in sign, against P -> Q: r = B - A, s = Q - P, w = P - A,
            den = rx * sy - ry * sx, t = (wx * sy - wy * sx) / den, u = (wx * ry - wy * rx) / den; it meets when den != 0 and
            0 <= t <= 1 and 0 <= u <= 1; the cut's t is the least such t when A is +, the greatest when B is +, 0.5 when
            there is none; the cut lies at A + t * r;
  snap      the six directions in the order E, N, NE, W, S, SW; the cut of a direction at c, d2 = dx * dx + dy * dy from the
            vertex to c, l2 = rx * rx + ry * ry of its edge; a candidate when d2 < (snap * snap) * l2; the vertex moves to
            the candidate of least d2, the lowest direction on a tie, and becomes 0; a cut lives while both its ends are not 0;
  faces     see faces_of below; references are slots: lattice vertex v = j * nx + i is slot v, the cut of family f on the edge
            that starts at v is slot nv + 3 * v + f; the slots some face names are numbered in ascending slot order.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

PLUS, ZERO, MINUS = 1, 0, -1
# (di, dj) of B from A for the families E, N, NE
FAMILY = ((1, 0), (0, 1), (1, 1))
# the six directions of a vertex: (di, dj) of the edge's owner A from the vertex, the family, whether the vertex is the A end
DIRECTIONS = ((0, 0, 0, True), (0, 0, 1, True), (0, 0, 2, True), (-1, 0, 0, False), (0, -1, 1, False), (-1, -1, 2, False))
# corner k of the lower and the upper triangle of a cell as (di, dj) from v00, and edge k (corner k -> corner k + 1) as
# (the corner that owns it, the family)
TRIANGLES = ((((0, 0), (1, 0), (1, 1)), ((0, 0), (1, 1), (0, 2))),
             (((0, 0), (1, 1), (0, 1)), ((0, 2), (2, 0), (0, 1))))


def rings_of(poly):
    out = []
    for ring in poly:
        r = np.ascontiguousarray(ring, dtype=np.float64).reshape(-1, 2)
        if len(r) > 1 and np.array_equal(r[0], r[-1]):
            r = r[:-1]
        out.append(r)
    return out


def lattice_of(rings, h):
    pts = np.concatenate(rings)
    i0 = int(math.floor(pts[:, 0].min() / h)) - 1
    j0 = int(math.floor(pts[:, 1].min() / h)) - 1
    nx = int(math.ceil(pts[:, 0].max() / h)) + 1 - i0 + 1
    ny = int(math.ceil(pts[:, 1].max() / h)) + 1 - j0 + 1
    return i0, j0, nx, ny


def segments_of(rings):
    """(n, 4): xj, yj, xi, yi."""
    return np.concatenate([np.concatenate([np.roll(r, 1, axis=0), r], axis=1) for r in rings])


def inside(seg, cx, cy):
    """The even-odd rule of csrc/sources.hip for points cx, cy (any shape) over the segments seg (n, 4)."""
    cx, cy = np.asarray(cx, dtype=np.float64)[..., None], np.asarray(cy, dtype=np.float64)[..., None]
    xj, yj, xi, yi = seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        cross = ((yi > cy) != (yj > cy)) & (cx < (xj - xi) * (cy - yi) / (yj - yi) + xi)
    return (cross.sum(axis=-1) & 1) == 1


def mesh_polygon(poly, h, snap=0.25):
    """Steps 1 to 6.  Returns a namespace: xy (n, 2) float64, tri (k, 3) int32, kind (n,) int32 (0 lattice, 1 snapped, 2 cut),
    and the lattice (i0, j0, nx, ny), the signs, states and cut parameters for the tests."""
    rings = rings_of(poly)
    h = float(h)
    i0, j0, nx, ny = lattice_of(rings, h)
    seg = segments_of(rings)
    X = (i0 + np.arange(nx + 1)).astype(np.float64) * h
    Y = (j0 + np.arange(ny + 1)).astype(np.float64) * h
    ylo, yhi = np.minimum(seg[:, 1], seg[:, 3]), np.maximum(seg[:, 1], seg[:, 3])
    bands = [seg[(ylo <= Y[j + 1]) & (yhi >= Y[j])] for j in range(ny)]

    # ---- sign
    sign = np.empty((ny, nx), dtype=np.int8)
    for j in range(ny):
        sign[j] = np.where(inside(bands[j], X[:nx], np.full(nx, Y[j])), PLUS, MINUS)

    # ---- cuts: t[f][j][i] of the edge of family f that starts at (i, j), -1.0 where there is none
    T = np.full((3, ny, nx), -1.0)
    for j in range(ny - 1):
        s = bands[j]
        px, py, sx, sy = s[:, 0], s[:, 1], s[:, 2] - s[:, 0], s[:, 3] - s[:, 1]
        for f, (di, dj) in enumerate(FAMILY):
            n = nx - di
            ax, ay = X[:n, None], Y[j]
            rx, ry = X[di:di + n, None] - ax, Y[j + dj] - ay
            a_plus = sign[j, :n] == PLUS
            differ = sign[j, :n] != sign[j + dj, di:di + n]
            den = rx * sy - ry * sx
            wx, wy = px - ax, py - ay
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (wx * sy - wy * sx) / den
                u = (wx * ry - wy * rx) / den
            ok = (den != 0) & (t >= 0) & (t <= 1) & (u >= 0) & (u <= 1)
            least = np.where(ok, t, np.inf).min(axis=1, initial=np.inf)
            greatest = np.where(ok, t, -np.inf).max(axis=1, initial=-np.inf)
            best = np.where(a_plus, least, greatest)
            best = np.where(np.isfinite(best), best, 0.5)
            T[f, j, :n] = np.where(differ, best, -1.0)

    # ---- the position of every cut
    AX, AY = np.broadcast_to(X[None, :nx], (ny, nx)), np.broadcast_to(Y[:ny, None], (ny, nx))
    CX, CY, L2 = np.zeros((3, ny, nx)), np.zeros((3, ny, nx)), np.zeros((3, ny, nx))
    for f, (di, dj) in enumerate(FAMILY):
        rx = np.broadcast_to((X[di:di + nx] - X[:nx])[None, :], (ny, nx))
        ry = np.broadcast_to((Y[dj:dj + ny] - Y[:ny])[:, None], (ny, nx))
        CX[f], CY[f], L2[f] = AX + T[f] * rx, AY + T[f] * ry, rx * rx + ry * ry

    # ---- snap
    snap2 = snap * snap
    best_d2 = np.full((ny, nx), np.inf)
    PX, PY = AX.copy(), AY.copy()
    snapped = np.zeros((ny, nx), dtype=bool)
    for (di, dj, f, _is_a) in DIRECTIONS:
        # the owner of the edge of vertex (i, j) is (i + di, j + dj): shift the owner's arrays onto the vertex
        t = np.full((ny, nx), -1.0)
        cx, cy, l2 = np.zeros((ny, nx)), np.zeros((ny, nx)), np.zeros((ny, nx))
        dst = (slice(-dj, ny), slice(-di, nx))
        src = (slice(0, ny + dj), slice(0, nx + di))
        t[dst], cx[dst], cy[dst], l2[dst] = T[f][src], CX[f][src], CY[f][src], L2[f][src]
        dx, dy = cx - AX, cy - AY
        d2 = dx * dx + dy * dy
        take = (t >= 0) & (d2 < snap2 * l2) & (d2 < best_d2)
        best_d2 = np.where(take, d2, best_d2)
        PX, PY = np.where(take, cx, PX), np.where(take, cy, PY)
        snapped |= take
    state = np.where(snapped, ZERO, sign).astype(np.int8)

    # ---- faces, as slots
    nv = nx * ny
    V = np.arange(nv).reshape(ny, nx)
    cells = (slice(0, ny - 1), slice(0, nx - 1))
    face_slots, face_count = [], []
    for corners, edges in TRIANGLES:
        at = [(slice(dj, ny - 1 + dj), slice(di, nx - 1 + di)) for di, dj in corners]
        st = np.stack([state[a] for a in at])
        ref = np.stack([V[a] for a in at])
        px, py = np.stack([PX[a] for a in at]), np.stack([PY[a] for a in at])
        cref = np.stack([nv + 3 * V[at[o]] + f for o, f in edges])
        cx, cy = np.stack([CX[f][at[o]] for o, f in edges]), np.stack([CY[f][at[o]] for o, f in edges])
        band = [bands[j] for j in range(ny - 1)]
        slots, count = faces_of(st, ref, px, py, cref, cx, cy, band)
        face_slots.append(slots)
        face_count.append(count)
    slots = np.stack(face_slots, axis=2)            # (ny - 1, nx - 1, 2 triangles, 2 pieces, 3)
    count = np.stack(face_count, axis=2)            # (ny - 1, nx - 1, 2 triangles)
    keep = np.arange(2)[None, None, None, :] < count[..., None]
    faces = slots[keep]                             # cell order, lower triangle first, the pieces in order

    # ---- numbering
    used = np.zeros(4 * nv, dtype=bool)
    used[faces.reshape(-1)] = True
    number = np.cumsum(used) - used
    tri = number[faces].astype(np.int32).reshape(-1, 3)
    slot = np.flatnonzero(used)
    xy = np.empty((len(slot), 2))
    kind = np.empty(len(slot), dtype=np.int32)
    lat = slot < nv
    xy[lat, 0], xy[lat, 1] = PX.reshape(-1)[slot[lat]], PY.reshape(-1)[slot[lat]]
    kind[lat] = np.where(snapped.reshape(-1)[slot[lat]], 1, 0)
    c = slot[~lat] - nv
    xy[~lat, 0] = CX.reshape(3, -1)[c % 3, c // 3]
    xy[~lat, 1] = CY.reshape(3, -1)[c % 3, c // 3]
    kind[~lat] = 2
    return SimpleNamespace(xy=xy, tri=tri, kind=kind, lattice=(i0, j0, nx, ny), sign=sign, state=state, T=T, h=h, snap=snap,
                           segments=seg)


def faces_of(st, ref, px, py, cref, cx, cy, band):
    """The pieces of a grid of lattice triangles.  Everything has a leading axis of 3 corners (edges: edge k runs from corner
    k to corner k + 1) and the shape (rows, columns) behind it; band[row] holds the segments the three-0 rule tests.

      no + corner          nothing, except three 0 corners whose centroid ((x0 + x1) + x2) / 3 is inside: the triangle;
      no - corner          the triangle (c0, c1, c2);
      one +, two -         with + first (p, q, r): (p, cut pq, cut rp);
      one +, one 0, one -  with + first: (p, q, cut rp) when q is 0, (p, cut pq, r) when r is 0;
      two +, one -         with - last (p, q, r): d1 = |cut qr - p|^2, d2 = |cut rp - q|^2 (dx * dx + dy * dy); d1 <= d2:
                           (p, q, cut qr), (p, cut qr, cut rp); otherwise (p, q, cut rp), (q, cut qr, cut rp).
    Returns slots (rows, columns, 2, 3) and the count (rows, columns)."""
    n_plus, n_minus = (st == PLUS).sum(axis=0), (st == MINUS).sum(axis=0)
    rows, cols = n_plus.shape
    first_plus = np.argmax(st == PLUS, axis=0)
    first_minus = np.argmax(st == MINUS, axis=0)
    rot = np.where((n_plus == 2) & (n_minus == 1), (first_minus + 1) % 3, first_plus)
    rot = np.where((n_plus >= 1) & (n_minus >= 1), rot, 0)
    order = (rot[None] + np.arange(3)[:, None, None]) % 3

    def turned(a):
        return np.take_along_axis(a, order, axis=0)
    st, ref, px, py, cref, cx, cy = (turned(a) for a in (st, ref, px, py, cref, cx, cy))
    p, q, r = ref
    cpq, cqr, crp = cref
    slots = np.zeros((rows, cols, 2, 3), dtype=np.int64)
    count = np.zeros((rows, cols), dtype=np.int64)

    def put(where, n, first, second=None):
        count[where] = n
        for k in range(3):
            slots[..., 0, k][where] = first[k][where]
            if second is not None:
                slots[..., 1, k][where] = second[k][where]

    # three 0 corners
    zeros = (n_plus == 0) & (n_minus == 0)
    if zeros.any():
        gx, gy = ((px[0] + px[1]) + px[2]) / 3, ((py[0] + py[1]) + py[2]) / 3
        inside_c = np.zeros((rows, cols), dtype=bool)
        for j in np.flatnonzero(zeros.any(axis=1)):
            inside_c[j] = inside(band[j], gx[j], gy[j])
        put(zeros & inside_c, 1, (p, q, r))
    put((n_plus >= 1) & (n_minus == 0), 1, (p, q, r))
    put((n_plus == 1) & (n_minus == 2), 1, (p, cpq, crp))
    one = (n_plus == 1) & (n_minus == 1)
    put(one & (st[1] == ZERO), 1, (p, q, crp))
    put(one & (st[2] == ZERO), 1, (p, cpq, r))
    two = (n_plus == 2) & (n_minus == 1)
    ex, ey = cx[1] - px[0], cy[1] - py[0]
    fx, fy = cx[2] - px[1], cy[2] - py[1]
    d1, d2 = ex * ex + ey * ey, fx * fx + fy * fy
    put(two & (d1 <= d2), 2, (p, q, cqr), (p, cqr, crp))
    put(two & ~(d1 <= d2), 2, (p, q, crp), (q, cqr, crp))
    return slots, count


# ---- what the tests measure -------------------------------------------------------------------------------------------------

def signed_areas(xy, tri):
    a, b, c = xy[tri[:, 0]], xy[tri[:, 1]], xy[tri[:, 2]]
    return 0.5 * ((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))


def polygon_area(poly):
    """Exterior minus holes (shoelace)."""
    total = 0.0
    for k, r in enumerate(rings_of(poly)):
        a = 0.5 * abs(np.sum(r[:, 0] * np.roll(r[:, 1], -1) - np.roll(r[:, 0], -1) * r[:, 1]))
        total += a if k == 0 else -a
    return total


def components(n_vert, tri):
    """(the number of components, the component of every face); faces are connected through shared edges."""
    import scipy.sparse as sp
    import scipy.sparse.csgraph as csgraph
    t = np.asarray(tri, dtype=np.int64)
    if len(t) == 0:
        return 0, np.zeros(0, dtype=np.int64)
    u, v = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    key = np.minimum(u, v) * n_vert + np.maximum(u, v)
    order = np.argsort(key, kind="stable")
    same = key[order][1:] == key[order][:-1]
    a, b = order[:-1][same] // 3, order[1:][same] // 3
    g = sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(len(t), len(t)))
    return csgraph.connected_components(g, directed=False)


def smallest_angle(xy, tri):
    p = xy[tri]
    best = np.inf
    for k in range(3):
        a, b, c = p[:, k], p[:, (k + 1) % 3], p[:, (k + 2) % 3]
        u, v = b - a, c - a
        cosv = (u * v).sum(axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
        best = min(best, float(np.degrees(np.arccos(np.clip(cosv, -1.0, 1.0))).min()))
    return best


def longest_edge(xy, tri):
    p = xy[tri]
    return max(float(np.linalg.norm(p[:, k] - p[:, (k + 1) % 3], axis=1).max()) for k in range(3))


def boundary_vertices(tri):
    """The vertices on a boundary half-edge: a directed edge without a twin."""
    t = np.asarray(tri, dtype=np.int64)
    u, v = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)
    n = int(t.max()) + 1
    twinless = ~np.isin(v * n + u, u * n + v)
    return np.unique(np.concatenate([u[twinless], v[twinless]]))


def distance_to_segments(seg, pts):
    """The least distance of every point to the segments, in extended precision."""
    p = np.asarray(pts, dtype=np.longdouble)[:, None, :]
    a, b = seg[None, :, 0:2].astype(np.longdouble), seg[None, :, 2:4].astype(np.longdouble)
    ab = b - a
    t = np.clip(((p - a) * ab).sum(axis=2) / (ab * ab).sum(axis=2), 0, 1)
    d = p - (a + t[..., None] * ab)
    return np.sqrt((d * d).sum(axis=2)).min(axis=1)


# ---- the shapes of the tests -------------------------------------------------------------------------------------------------

def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=np.float64)


def rotated(ring, angle, shift=(0.0, 0.0)):
    c, s = math.cos(angle), math.sin(angle)
    r = np.asarray(ring, dtype=np.float64)
    return np.stack([c * r[:, 0] - s * r[:, 1] + shift[0], s * r[:, 0] + c * r[:, 1] + shift[1]], axis=1)


def ngon(n, radius, centre=(0.0, 0.0), phase=0.0):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([centre[0] + radius * np.cos(a), centre[1] + radius * np.sin(a)], axis=1)


def star(points=10, r_out=4.0, r_in=2.0, centre=(0.13, -0.21)):
    a = 0.1 + np.pi * np.arange(2 * points) / points
    rad = np.where(np.arange(2 * points) % 2 == 0, r_out, r_in)
    return np.stack([centre[0] + rad * np.cos(a), centre[1] + rad * np.sin(a)], axis=1)


def ell(a=6.0, b=4.0, w=1.7, shift=(0.11, 0.23)):
    r = np.array([[0, 0], [a, 0], [a, w], [w, w], [w, b], [0, b]], dtype=np.float64)
    return r + np.asarray(shift)


def trace(width_in_cells, h):
    """The trace of the issue: rect(0, 0, 12, w) rotated 0.37 rad and shifted by 0.07."""
    return rotated(rect(0, 0, 12, width_in_cells * h), 0.37, (0.07, 0.07))


def seven_shapes(h):
    """name -> polygon (a list of rings), the seven shapes of the issue at spacing h."""
    return {
        "rect_off": [rect(0.13, 0.21, 7.31, 3.47)],
        "rect_on": [rect(0, 0, 10, 4)],
        "rect_rotated": [rotated(rect(0, 0, 8, 3), 0.3, (0.05, 0.02))],
        "ell": [ell()],
        "gon96_hole48": [ngon(96, 5.0, (0.17, 0.09)), ngon(48, 2.0, (0.31, -0.12), 0.05)],
        "star": [star()],
        "trace3": [trace(3.0, h)],
    }


def random_shapes(seed, n=150):
    """Rotated rectangles, n-gons with a hole and L shapes, seeded."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        which = k % 3
        angle, shift = rng.uniform(0, np.pi), rng.uniform(-1, 1, 2)
        if which == 0:
            out.append([rotated(rect(0, 0, rng.uniform(3, 8), rng.uniform(2, 5)), angle, shift)])
        elif which == 1:
            m = int(rng.integers(5, 40))
            R = rng.uniform(2.5, 5)
            out.append([ngon(m, R, shift, angle), ngon(int(rng.integers(4, 20)), rng.uniform(0.8, 0.45 * R),
                                                       shift + rng.uniform(-0.2, 0.2, 2), angle / 2)])
        else:
            out.append([rotated(ell(rng.uniform(4, 7), rng.uniform(3.5, 6), rng.uniform(1.5, 2.5), (0.0, 0.0)), angle, shift)])
    return out

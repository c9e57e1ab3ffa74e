"""The connectivity pre-pass restated in numpy and plain Python: the specification of the bits of csrc/connectivity.hip
(``padne_polygons_locate``) and of the graph of ``padne_amd.solver.compute_connectivity``.  Written from the rule, not from
the kernel or the solver.

The rule.  Polygons as ``padne_polymesh_create`` takes them (a list of rings each, the exterior first, no closing
duplicate, orientation free).  Every polygon has a group (its layer), ascending over the batch; every query point has a
group and meets the polygons of its own group only.

  segments  for every ring vertex i, from the previous vertex of the same ring (cyclic) (xj, yj) to (xi, yi);
  crossing  (yi > py) != (yj > py) and px < (xj - xi) * (py - yi) / (yj - yi) + xi, every operation rounded on its own
            (numpy does; the kernel is compiled with -ffp-contract=off); inside when the crossings over all rings are odd;
  boundary  on when for some segment (xi - xj) * (py - yj) - (yi - yj) * (px - xj) == 0 and min(xi, xj) <= px <= max(xi, xj)
            and min(yi, yj) <= py <= max(yi, yj);
  kind      2 when on, else 1 when inside, else 0 (:func:`classify`);
  box       the exact least and greatest coordinates of the polygon's ring vertices, closed; :func:`locate` gives kind 0 to
            a query outside it without asking :func:`classify`;
  output    CSR over the queries, the hits (kind != 0) of a query in ascending polygon number.

The boundary test carries no tolerance: it is exact at every ring vertex, on axis-parallel segments and wherever the two
products are exact; a point computed onto a slanted segment is in general not seen as on it.
"""
import numpy as np


def segments_of(rings):
    """(n, 4): xj, yj, xi, yi."""
    return np.concatenate([np.concatenate([np.roll(r, 1, axis=0), r], axis=1)
                           for r in (np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings)])


def classify(rings, px, py):
    """The kind of every point (px[k], py[k]) against the polygon ``rings``: int32, 0 outside, 1 inside, 2 on the boundary.
    The box is not asked."""
    seg = segments_of(rings)
    px, py = np.asarray(px, dtype=np.float64).reshape(-1, 1), np.asarray(py, dtype=np.float64).reshape(-1, 1)
    xj, yj, xi, yi = seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cross = ((yi > py) != (yj > py)) & (px < (xj - xi) * (py - yi) / (yj - yi) + xi)
        on = (((xi - xj) * (py - yj) - (yi - yj) * (px - xj) == 0.0) & (np.minimum(xi, xj) <= px) & (px <= np.maximum(xi, xj))
              & (np.minimum(yi, yj) <= py) & (py <= np.maximum(yi, yj)))
    inside = (cross.sum(axis=1) & 1) == 1
    return np.where(on.any(axis=1), 2, np.where(inside, 1, 0)).astype(np.int32)


def box_of(rings):
    pts = np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 2) for r in rings])
    return pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()


def in_box(box, px, py):
    return (px >= box[0]) & (px <= box[2]) & (py >= box[1]) & (py <= box[3])


def locate(polygons, groups, points, point_groups):
    """(hit_ptr (n + 1,) int64, hit_poly int32, hit_kind int32), as ``_hip.locate_polygons``; ValueError where
    ``padne_polygons_locate`` refuses with PADNE_E_INVALID."""
    groups = np.asarray(groups).reshape(-1)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    point_groups = np.asarray(point_groups).reshape(-1)
    if len(groups) != len(polygons) or len(point_groups) != len(pts):
        raise ValueError("one group per polygon and per point")
    if (groups < 0).any() or (point_groups < 0).any():
        raise ValueError("a group is not negative")
    if (np.diff(groups) < 0).any():
        raise ValueError("the groups of the polygons must be ascending")
    if not np.isfinite(pts).all():
        raise ValueError("a query point is not finite")
    for poly in polygons:
        if len(poly) == 0:
            raise ValueError("a polygon has at least its exterior ring")
        for ring in poly:
            r = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
            if len(r) < 3:
                raise ValueError("a ring has at least 3 vertices")
            if not np.isfinite(r).all():
                raise ValueError("a coordinate is not finite")
    found = []                                                # (query, polygon, kind)
    for p, poly in enumerate(polygons):
        mine = np.flatnonzero(point_groups == groups[p])
        if len(mine) == 0:
            continue
        mine = mine[in_box(box_of(poly), pts[mine, 0], pts[mine, 1])]
        if len(mine) == 0:
            continue
        kind = classify(poly, pts[mine, 0], pts[mine, 1])
        found.extend((int(q), p, int(k)) for q, k in zip(mine, kind) if k != 0)
    found.sort()
    count = np.bincount(np.array([f[0] for f in found], dtype=np.int64), minlength=len(pts)) if found else np.zeros(len(pts), dtype=np.int64)
    hit_ptr = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    return hit_ptr, np.array([f[1] for f in found], dtype=np.int32), np.array([f[2] for f in found], dtype=np.int32)


def locate_by_layer(polygons, groups, points, point_groups):
    """:func:`locate`, a group at a time with the box test of all its (point, polygon) pairs in one array operation: the
    same result, for boards with thousands of polygons (scripts/connectivity.py times it)."""
    groups = np.asarray(groups).reshape(-1)
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    point_groups = np.asarray(point_groups).reshape(-1)
    boxes = np.array([box_of(poly) for poly in polygons], dtype=np.float64).reshape(-1, 4)
    qs, ps, ks = [], [], []
    for g in np.unique(groups):
        mine, polys = np.flatnonzero(point_groups == g), np.flatnonzero(groups == g)
        if len(mine) == 0:
            continue
        x, y = pts[mine, 0][:, None], pts[mine, 1][:, None]
        b = boxes[polys]
        cand = (x >= b[:, 0]) & (x <= b[:, 2]) & (y >= b[:, 1]) & (y <= b[:, 3])
        for col in np.flatnonzero(cand.any(axis=0)):
            who = mine[cand[:, col]]
            kind = classify(polygons[polys[col]], pts[who, 0], pts[who, 1])
            qs.append(who[kind != 0])
            ps.append(np.full(int((kind != 0).sum()), polys[col], dtype=np.int64))
            ks.append(kind[kind != 0])
    if not qs:
        return np.zeros(len(pts) + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    q, p, k = np.concatenate(qs), np.concatenate(ps), np.concatenate(ks)
    order = np.lexsort((p, q))
    hit_ptr = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=len(pts)))]).astype(np.int64)
    return hit_ptr, p[order].astype(np.int32), k[order].astype(np.int32)


# ---- the graph ---------------------------------------------------------------------------------------------------------------

def connected_pairs(network_nodes, has_source):
    """``network_nodes[n]``: the nodes (any hashable, here (layer_i, geom_i)) the connections of network n touch;
    ``has_source[n]``.  All nodes of a network are joined, those of a network with a source are roots; returns
    (the set of nodes reachable from a root, the set of roots).  Breadth first, on adjacency sets."""
    neighbours, roots = {}, set()
    for nodes, source in zip(network_nodes, has_source):
        nodes = list(nodes)
        for a in nodes:
            neighbours.setdefault(a, set()).update(nodes)
        if source:
            roots.update(nodes)
    seen, todo = set(roots), list(roots)
    while todo:
        a = todo.pop()
        for b in neighbours[a]:
            if b not in seen:
                seen.add(b)
                todo.append(b)
    return seen, roots


def kept_networks(network_nodes, connected):
    """The indices of the networks none of whose nodes is outside ``connected`` (a network that touches nothing stays)."""
    return [n for n, nodes in enumerate(network_nodes) if all(a in connected for a in nodes)]


def board_nodes(polygons_by_layer, networks):
    """``polygons_by_layer[l]``: the polygons (lists of rings) of layer l; ``networks``: per network a list of connections
    ``(layer_i, x, y)``.  Returns per network, per connection, the list of ((layer_i, geom_i), kind) it touches, by
    :func:`locate` over the whole board."""
    polygons = [poly for layer in polygons_by_layer for poly in layer]
    groups = [l for l, layer in enumerate(polygons_by_layer) for _ in layer]
    first = np.concatenate([[0], np.cumsum([len(layer) for layer in polygons_by_layer])])
    conns = [c for net in networks for c in net]
    hit_ptr, hit_poly, hit_kind = locate(polygons, groups, [(c[1], c[2]) for c in conns], [c[0] for c in conns])
    out, q = [], 0
    for net in networks:
        of_net = []
        for layer_i, _x, _y in net:
            of_net.append([((layer_i, int(hit_poly[k] - first[layer_i])), int(hit_kind[k])) for k in range(hit_ptr[q], hit_ptr[q + 1])])
            q += 1
        out.append(of_net)
    return out


# ---- boards as plain data: for the graph tests and tests/golden/make_connectivity_golden.py -------------------------------------
# A board is (polygons_by_layer, networks): networks[n] = {"has_source": bool, "connections": [(layer_i, x, y), ...]}.

def fixture_board():
    """``pruned_board_problem()`` of tests/test_connectivity_host.py as plain data (a test holds the two together)."""
    import gridmesh_ref as G
    front = [[G.ell(6.0, 4.0, 1.7, (0.11, 0.23)), G.ngon(24, 0.4, (1.0, 1.1))], [G.rect(7.0, 0.2, 9.0, 1.7)], [G.rect(7.0, 2.3, 9.0, 3.8)],
             [G.rect(9.6, 2.3, 11.0, 3.8)], [G.rect(9.5, 0.5, 9.6, 0.6)], [G.rect(11.5, 0.2, 12.5, 1.2)]]
    back = [[G.rect(0.3, 0.4, 5.7, 1.6)], [G.rect(6.5, 0.4, 9.0, 1.6)]]
    networks = [{"has_source": True, "connections": [(0, 5.8, 0.9), (0, 0.9, 3.9)]},
                {"has_source": False, "connections": [(0, 3.0, 1.0), (1, 3.0, 1.0)]},
                {"has_source": False, "connections": [(0, 3.0, 1.2), (0, 8.0, 1.0)]},
                {"has_source": False, "connections": [(0, 8.0, 3.0), (0, 10.0, 3.0)]},
                {"has_source": False, "connections": [(0, 11.5, 0.2), (0, 5.0, 0.5)]}]
    return [front, back], networks


RANDOM_BOARD_SEEDS = tuple(range(40))


def random_board(seed):
    """3 layers of 5 to 30 rectangles and n-gons with disjoint interiors, one per cell of a 6 x 6 grid of 4 x 4 cells; some
    fill their cell, so that diagonal neighbours share a ring vertex and side neighbours a side: a point there touches
    two to four polygons.  3 to 12 networks of 2 or 3 connections, with and without a source, the connections drawn from
    centres of polygons, ring vertices and empty space (left of the grid)."""
    import gridmesh_ref as G
    rng = np.random.default_rng(1000 + seed)
    layers = []
    for _layer in range(3):
        cells = rng.permutation(36)[:int(rng.integers(5, 31))]
        polys = []
        for cell in np.sort(cells):
            x0, y0 = 4.0 * (cell % 6), 4.0 * (cell // 6)
            which = rng.uniform()
            if which < 0.35:
                polys.append([G.rect(x0, y0, x0 + 4.0, y0 + 4.0)])
            elif which < 0.7:
                a, b = rng.uniform(0.2, 1.5, 2)
                polys.append([G.rect(x0 + a, y0 + b, x0 + 4.0 - b, y0 + 4.0 - a)])
            else:
                polys.append([G.ngon(int(rng.integers(3, 13)), rng.uniform(0.5, 1.9), (x0 + 2.0, y0 + 2.0), rng.uniform(0, 1))])
        layers.append(polys)
    networks = []
    for _net in range(int(rng.integers(3, 13))):
        conns = []
        for _c in range(int(rng.integers(2, 4))):
            layer_i = int(rng.integers(0, 3))
            poly = layers[layer_i][int(rng.integers(0, len(layers[layer_i])))]
            which = rng.uniform()
            if which < 0.5:
                x, y = np.mean(poly[0], axis=0)
            elif which < 0.85:
                x, y = poly[0][int(rng.integers(0, len(poly[0])))]
            else:
                x, y = rng.uniform(-3.0, -1.0), rng.uniform(0.0, 24.0)
            conns.append((layer_i, float(x), float(y)))
        networks.append({"has_source": bool(rng.uniform() < 0.4), "connections": conns})
    return layers, networks


def board_graph(board):
    """(connected pairs sorted, kept network indices) of a plain board by :func:`locate`, :func:`connected_pairs` and
    :func:`kept_networks`."""
    layers, networks = board
    per_conn = board_nodes(layers, [net["connections"] for net in networks])
    network_nodes = [[node for of_conn in of_net for node, _kind in of_conn] for of_net in per_conn]
    connected, _roots = connected_pairs(network_nodes, [net["has_source"] for net in networks])
    return sorted(connected), kept_networks(network_nodes, connected)


def reference_graph(ref, board):
    """The same by the reference's own ``ConnectivityGraph.create_from_problem``, ``find_connected_layer_geom_indices`` and
    ``filter_dead_networks`` (``ref``: the namespace of ``oracle.ref_loader.load_reference()``) on duck-typed objects: a tree
    whose ``query`` returns every index of the layer, geoms whose ``intersects`` / ``contains`` are :func:`classify`'s kinds.
    This holds the graph and the filter to the reference, not the predicate."""
    layers, networks = board

    class Geom:
        def __init__(self, rings):
            self.rings = rings

        def intersects(self, point):
            return bool(classify(self.rings, [point.x], [point.y])[0] != 0)

        def contains(self, point):
            return bool(classify(self.rings, [point.x], [point.y])[0] == 1)

    class Layer:
        def __init__(self, polys):
            self.geoms = tuple(Geom(p) for p in polys)

    class Tree:
        def __init__(self, n):
            self.n = n

        def query(self, _point):
            return list(range(self.n))

    class Point:
        def __init__(self, x, y):
            self.x, self.y = x, y

    class Connection:
        def __init__(self, layer, x, y):
            self.layer, self.point = layer, Point(x, y)

    class Network:
        def __init__(self, connections, has_source):
            self.connections, self.has_source = connections, has_source

    class Problem:
        pass

    prob = Problem()
    prob.layers = [Layer(polys) for polys in layers]
    prob.networks = [Network([Connection(prob.layers[l], x, y) for l, x, y in net["connections"]], net["has_source"]) for net in networks]
    trees = [Tree(len(layer.geoms)) for layer in prob.layers]
    graph = ref.solver.ConnectivityGraph.create_from_problem(prob, trees)
    connected = ref.solver.find_connected_layer_geom_indices(graph)
    kept = ref.solver.filter_dead_networks(prob, trees, connected)
    return sorted((int(l), int(g)) for l, g in connected), [n for n, net in enumerate(prob.networks) if any(net is k for k in kept)]

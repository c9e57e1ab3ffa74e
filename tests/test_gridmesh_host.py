"""The grid mesher on the host: tests/gridmesh_ref.py (the numpy restatement of csrc/polymesh.hip, the specification of the
bits) held to the properties a first mesh must have, ``padne_amd.gridmesh.GridMesher``'s own checks run on the restatement's
arrays, and the physics of a rotated strip through the checker's assembly and direct solve.  No GPU."""
import math

import numpy as np
import pytest

import gridmesh_ref as G
from oracle import padne_oracle as O
from padne_amd import GridMesher, Polygon, gridmesh, mesh, problem, structured

EPS = 2.0 ** -53
SNAP = 0.25


def host_engine(polygons, h, snap):
    out = []
    for rings in polygons:
        m = G.mesh_polygon(rings, h, snap)
        out.append((m.xy, m.tri, m.kind))
    return out


def host_mesher(**kw):
    return GridMesher(engine=host_engine, **kw)


def on_boundary_bound(poly, h):
    """How far a cut may lie from the polygon's segments.  The cut is c = A + t r, t = N / den with N = wx sy - wy sx and
    den = rx sy - ry sx, every operand a rounded difference.  With e = 2^-53: N carries at most 6 e |w| |s|, den at most
    6 e |r| |s|, and |den| = |r| |s| sin(theta), theta the angle between the edge and the segment.  An error dt of t moves c
    by |r| dt along the edge, that is by |r| dt sin(theta) off the segment's line: 6 e (|w| + |r|), and the quotient, the
    product and the sum that make c add 3 e |c|.  The same figure divided by sin(theta) bounds how far past a segment's end a
    crossing can be that rounding still accepts (0 <= u <= 1).  |w| <= the lattice's diagonal, |r| <= sqrt(2) h, |c| <= the
    largest coordinate; theta is at least the smallest angle between a segment and the three lattice directions that is not
    exactly 0 (parallel pairs have den == 0 and never meet).  16 covers 6 + 6 + 3."""
    rings = G.rings_of(poly)
    seg = G.segments_of(rings)
    pts = np.concatenate(rings)
    diag = float(np.hypot(np.ptp(pts[:, 0]) + 2 * h, np.ptp(pts[:, 1]) + 2 * h))
    big = float(np.abs(pts).max()) + h
    ang = np.arctan2(seg[:, 3] - seg[:, 1], seg[:, 2] - seg[:, 0])
    sines = np.abs(np.sin(ang[:, None] - np.array([0.0, math.pi / 2, math.pi / 4])[None, :]))
    sin_min = float(sines[sines > 1e-12].min())
    return 16 * EPS * (diag + math.sqrt(2) * h + big) / sin_min


def hold(poly, h, snap=SNAP):
    """Every property of the issue's list on one mesh of the restatement; returns it with its area ratio and smallest angle."""
    m = G.mesh_polygon(poly, h, snap)
    assert m.xy.dtype == np.float64 and m.tri.dtype == np.int32 and m.kind.dtype == np.int32
    mesh.check_manifold(len(m.xy), m.tri)
    area = G.signed_areas(m.xy, m.tri)
    assert area.min() > 0
    assert G.components(len(m.xy), m.tri)[0] == 1
    assert G.longest_edge(m.xy, m.tri) <= math.sqrt(2) * (1 + 2 * snap) * h
    rim = G.boundary_vertices(m.tri)
    assert set(m.kind[rim].tolist()) <= {1, 2}
    assert G.distance_to_segments(m.segments, m.xy[rim]).max() <= on_boundary_bound(poly, h)
    assert np.array_equal(np.unique(m.tri), np.arange(len(m.xy)))          # no unused vertex
    return m, float(area.sum() / G.polygon_area(poly)), G.smallest_angle(m.xy, m.tri)


@pytest.mark.parametrize("h", [0.5, 0.25])
@pytest.mark.parametrize("name", list(G.seven_shapes(0.5)))
def test_the_seven_shapes(name, h):
    _m, ratio, angle = hold(G.seven_shapes(h)[name], h)
    print(name, h, "area ratio", ratio, "smallest angle", angle)


def test_a_seeded_sweep_of_random_shapes():
    ratios, angles = [], []
    for k, poly in enumerate(G.random_shapes(7)):
        _m, ratio, angle = hold(poly, 0.5 if k % 2 else 0.25)
        ratios.append(ratio)
        angles.append(angle)
    print("area ratio", min(ratios), "to", max(ratios), "smallest angle", min(angles))


@pytest.mark.parametrize("h", [0.5, 0.25])
def test_a_rectangle_on_lattice_lines_is_meshed_exactly(h):
    """Sides on lattice lines: the closed interval of the cut and the centroid rule for three 0 corners.  Two faces in
    every cell of the rectangle, none outside, the area exactly 40."""
    m = G.mesh_polygon([G.rect(0, 0, 10, 4)], h)
    nx, ny = round(10 / h), round(4 / h)
    assert len(m.tri) == 2 * nx * ny
    centroid = m.xy[m.tri].mean(axis=1)
    cell = np.floor(centroid[:, 0] / h).astype(int) + nx * np.floor(centroid[:, 1] / h).astype(int)
    assert centroid[:, 0].min() > 0 and centroid[:, 0].max() < 10 and centroid[:, 1].min() > 0 and centroid[:, 1].max() < 4
    assert np.array_equal(np.bincount(cell, minlength=nx * ny), np.full(nx * ny, 2))
    assert G.signed_areas(m.xy, m.tri).sum() == 40.0
    assert len(m.xy) == (nx + 1) * (ny + 1) and not (m.kind == 2).any()


def test_two_runs_and_ring_orientation():
    """Two runs: the same bits.  Rings turned round: the same signs, so the same faces and kinds; a segment run from its other
    end rounds a cut's parameter differently, so the coordinates agree to rounding only."""
    poly = G.seven_shapes(0.5)["gon96_hole48"]
    a, again, b = G.mesh_polygon(poly, 0.5), G.mesh_polygon(poly, 0.5), G.mesh_polygon([poly[0][::-1], poly[1][::-1]], 0.5)
    assert np.array_equal(a.xy, again.xy) and np.array_equal(a.tri, again.tri) and np.array_equal(a.kind, again.kind)
    assert np.array_equal(a.sign, b.sign) and np.array_equal(a.tri, b.tri) and np.array_equal(a.kind, b.kind)
    assert np.abs(a.xy - b.xy).max() <= on_boundary_bound(poly, 0.5)


# ---- GridMesher's own checks, on the restatement's arrays ---------------------------------------------------------------------

def thin_trace():
    return Polygon(G.rotated(G.rect(0, 0, 12, 0.4), 0.37, (0.07, 0.07)))


def test_a_trace_narrower_than_a_cell_raises_for_components():
    with pytest.raises(mesh.MeshingException, match="maximum_size"):
        host_mesher(spacing=0.5).poly_to_mesh(thin_trace())


def test_crumbs_drop_keeps_one_component():
    mesher = host_mesher(spacing=0.5, crumbs="drop")
    m = mesher.poly_to_mesh(thin_trace())
    assert mesher.last_report[0]["components"] > 1
    mesh.check_manifold(len(m.points), m.triangles)
    assert G.components(len(m.points), m.triangles)[0] == 1
    assert np.array_equal(np.unique(m.triangles), np.arange(len(m.points)))


def test_a_polygon_smaller_than_a_cell_raises():
    with pytest.raises(mesh.MeshingException, match="maximum_size"):
        host_mesher(spacing=0.5).poly_to_mesh(structured.Rect(0.1, 0.1, 0.4, 0.4))


def test_a_lost_seed_raises():
    """An L whose arm is thinner than a cell, dropped as a crumb or never meshed: the seed in it is far from every vertex."""
    arm = Polygon([(0, 0), (4, 0), (4, 3), (3.9, 3), (3.9, 10), (3.7, 10), (3.7, 3), (0, 3)])
    seed = mesh.Point(3.8, 9.5)
    assert arm.contains_xy(seed.x, seed.y)
    with pytest.raises(mesh.MeshingException, match="seed"):
        host_mesher(spacing=0.5, crumbs="drop").poly_to_mesh(arm, [seed])
    host_mesher(spacing=0.5, crumbs="drop").poly_to_mesh(arm, [mesh.Point(1.0, 1.0), mesh.Point(50.0, 50.0)])


def test_bad_arguments_raise():
    square = [(0, 0), (2, 0), (2, 2), (0, 2)]
    with pytest.raises(mesh.MeshingException, match="maximum_size"):
        host_mesher(config=mesh.Mesher.Config(maximum_size=0.0)).poly_to_mesh(Polygon(square))
    for kw in ({"snap": 0.0}, {"snap": 0.5}, {"spacing": 0.0}, {"spacing": -1.0}, {"crumbs": "keep"}, {"area_tolerance": 0.0}):
        with pytest.raises(ValueError):
            host_mesher(**kw)
    with pytest.raises(ValueError):
        host_mesher(spacing=0.5).poly_to_mesh(Polygon([(0, 0), (1, 0), (0, 0)]))
    with pytest.raises(ValueError):
        host_mesher(spacing=0.5).poly_to_mesh(Polygon([(0, 0), (1, 0), (1, float("nan"))]))
    with pytest.raises(mesh.MeshingException):
        host_mesher(spacing=0.5).poly_to_mesh(structured.Annulus(0, 0, 1, 2))
    with pytest.raises(mesh.MeshingException, match="area"):
        host_mesher(spacing=0.5, area_tolerance=1e-6).poly_to_mesh(Polygon(G.star()))


def test_polygon_rect_report_and_the_default_spacing():
    """A closing duplicate is dropped, a Rect is its four corners, the default spacing is maximum_size / sqrt(2)."""
    ring = G.ell()
    closed = Polygon(np.concatenate([ring, ring[:1]]), holes=[G.ngon(12, 0.5, (1.0, 1.0))])
    assert closed.exterior.coords[0] == closed.exterior.coords[-1] and len(closed.interiors) == 1
    mesher = host_mesher(config=mesh.Mesher.Config(maximum_size=0.5, minimum_angle=33.0))
    got = mesher.polys_to_meshes([closed, structured.Rect(0, 0, 10, 4)])
    want = [G.mesh_polygon([ring, G.ngon(12, 0.5, (1.0, 1.0))], 0.5 / math.sqrt(2.0)), G.mesh_polygon([G.rect(0, 0, 10, 4)], 0.5 / math.sqrt(2.0))]
    for g, w, rep in zip(got, want, mesher.last_report):
        assert np.array_equal(g.points, w.xy) and np.array_equal(g.triangles, w.tri)
        assert rep["lattice"] == w.lattice[2:] and rep["components"] == 1 and rep["faces"] == len(w.tri)
        assert rep["vertices"] == {"lattice": int((w.kind == 0).sum()), "snapped": int((w.kind == 1).sum()), "cut": int((w.kind == 2).sum())}
        assert 0.9 < rep["area_ratio"] < 1.1
    layer = problem.Layer(shape=structured.Shapes.of(closed), name="F.Cu", conductance=1.0)
    assert layer.geoms == (closed,)
    assert gridmesh.GridMesher is GridMesher


# ---- physics -----------------------------------------------------------------------------------------------------------------

ANGLE, SHIFT = 0.3, (0.137, 0.291)


def rotated_strip_problem():
    """``strip_problem()`` of tests/test_gpu_parity.py, rotated by 0.3 rad and shifted off the lattice: the same nodes and
    elements, the layer a Polygon, every connection's point moved with it."""
    from test_gpu_parity import strip_problem
    old = strip_problem()
    layer = problem.Layer(shape=structured.Shapes.of(Polygon(G.rotated(G.rect(0, 0, 10, 1), ANGLE, SHIFT))), name="F.Cu", conductance=1.0)
    nets = []
    for net in old.networks:
        cons = []
        for c in net.connections:
            (p,) = G.rotated(np.array([[c.point.x, c.point.y]]), ANGLE, SHIFT)
            cons.append(problem.Connection(layer=layer, point=mesh.Point(float(p[0]), float(p[1])), node_id=c.node_id))
        nets.append(problem.Network(connections=cons, elements=net.elements))
    return problem.Problem(layers=[layer], networks=nets)


def along_the_strip(points):
    """The coordinate along the strip's axis, from 0 to 10."""
    c, s = math.cos(ANGLE), math.sin(ANGLE)
    return c * (points[:, 0] - SHIFT[0]) + s * (points[:, 1] - SHIFT[1])


def test_the_rotated_strip_is_linear_by_the_direct_solve():
    """The checker's assembly and direct solve on the restatement's mesh: V linear along the axis within the 0.05 that
    test_linear_rectangle_end_to_end takes from the reference's own test."""
    prob = rotated_strip_problem()
    (m,) = host_mesher(config=mesh.Mesher.Config(maximum_size=0.2)).polys_to_meshes(
        prob.layers[0].geoms, [c.point for n in prob.networks for c in n.connections])
    ids = {}
    nets = []
    for net in prob.networks:
        cons = [(0, c.point.x, c.point.y, ids.setdefault(c.node_id, len(ids))) for c in net.connections]
        els = [("V", ids.setdefault(e.p, len(ids)), ids.setdefault(e.n, len(ids)), e.voltage) for e in net.elements]
        nets.append({"connections": cons, "elements": els})
    n_vert = len(m.points)
    n2g, extra, internal = O.node_indexer_create({0: m.points}, {0: np.arange(n_vert)}, n_vert, nets)
    ground = O.find_best_ground_node_index(nets, n2g)
    L, r = O.assemble_system([(m.points, m.triangles, 1.0)], internal, O.globalise_elements(nets, n2g, extra), ground)
    v, _gc, res = O.solve_system(L, r)
    assert res < 1e-9
    err = np.abs(v[:n_vert] - along_the_strip(m.points) / 10.0).max()
    print("rotated strip:", n_vert, "vertices, largest deviation from linear", err)
    assert err < 0.05

"""The graded grid mesher on the host: tests/gridmesh_graded_ref.py (the numpy restatement of the rule, the specification of
the bits of ``padne_polymesh_create_graded``) held to the properties a graded mesh must have, on fixtures that are themselves
held to produce every leaf template; ``GridMesher(graded=True)``'s thresholds, report, checks and refusals with the
restatement as its engine.  No GPU."""
import functools
import math

import numpy as np
import pytest

import gridmesh_graded_ref as GG
import gridmesh_ref as G
from padne_amd import GridMesher, Polygon, gridmesh, mesh, structured

SPACINGS = (0.5, 0.25)
NEGATIVE_RECT = [G.rect(-43.3, -31.7, -3.3, -1.7)]          # 40 x 30, every coordinate negative
# inside a plain cell; outside the lattice; exactly on lattice lines of both spacings; in a cell the boundary already touches
NEGATIVE_SEEDS = [(-20.13, -15.21), (100.0, 100.0), (-10.0, -8.0), (-43.2, -31.6)]
SHAPE_SEEDS = [(3.03, 1.26), (-50.0, 7.0), (2.0, 1.5), (0.14, 0.22)]


def threshold_sets(h):
    return [[0, 2, 4], [0, 5, 8, 13], GG.host_thresholds(h, 3.0, 0.5, 3.0)]


@functools.lru_cache(maxsize=None)
def uniform_of(name, h):
    if name == "negative":
        return NEGATIVE_RECT, G.mesh_polygon(NEGATIVE_RECT, h)
    if name.startswith("random"):
        poly = G.random_shapes(7)[int(name[6:])]
        return poly, G.mesh_polygon(poly, h)
    poly = G.seven_shapes(h)[name]
    return poly, G.mesh_polygon(poly, h)


def fixtures():
    """(name, h, thresholds, seeds) of every mesh the properties are held on."""
    out = []
    for h in SPACINGS:
        for t in threshold_sets(h):
            for name in G.seven_shapes(h):
                out.append((name, h, tuple(t), ()))
            out.append(("negative", h, tuple(t), ()))
            out.append(("negative", h, tuple(t), tuple(NEGATIVE_SEEDS)))
        for name in G.seven_shapes(h):
            out.append((name, h, (0, 2, 4), tuple(SHAPE_SEEDS)))
    for k in range(150):
        h = 0.5 if k % 2 else 0.25
        out.append((f"random{k}", h, tuple(threshold_sets(h)[k % 3]), ()))
    return out


@functools.lru_cache(maxsize=None)
def graded_of(name, h, t, seeds):
    poly, uniform = uniform_of(name, h)
    return poly, GG.mesh_polygon_graded(poly, h, list(t), list(seeds), uniform=uniform)


def hold(poly, g, t):
    """Every property of the issue's list on one graded mesh of the restatement."""
    u = g.uniform
    i0, j0, nx, ny = g.lattice
    assert g.xy.dtype == np.float64 and g.tri.dtype == np.int32 and g.kind.dtype == np.int32
    mesh.check_manifold(len(g.xy), g.tri)
    area = G.signed_areas(g.xy, g.tri)
    assert area.min() > 0
    assert G.components(len(g.xy), g.tri)[0] == 1
    assert np.array_equal(np.unique(g.tri), np.arange(len(g.xy)))          # no unused vertex
    # no hanging node: the boundary is the uniform mesh's, edge by edge
    assert GG.boundary_edges(g.xy, g.tri) == GG.boundary_edges(u.xy, u.tri)
    # sums of different triangles round differently; the difference is rounding alone
    total, want = float(area.sum()), float(G.signed_areas(u.xy, u.tri).sum())
    assert abs(total - want) <= 1e-12 * want
    # the distance and the levels: d is 0 exactly on the cells that are not plain, levels need their threshold
    assert np.array_equal(g.d == 0, ~g.plain) and g.d.max() <= t[-1]
    assert all((g.d[g.level == l] >= t[l]).all() for l in range(len(t)))
    # balance: cells that share a side differ by at most one level, and a leaf side borders at most two leaves
    lev = g.level.astype(np.int64)
    assert np.abs(np.diff(lev, axis=0)).max() <= 1 and np.abs(np.diff(lev, axis=1)).max() <= 1
    cj, ci = np.mgrid[0:ny - 1, 0:nx - 1]
    s = 2 ** lev
    leaf = np.full((ny + 1, nx + 1), -1, dtype=np.int64)
    leaf[1:ny, 1:nx] = (((j0 + cj) // s) * s - j0) * nx + ((i0 + ci) // s) * s - i0
    for (ai, aj, l, mask) in g.leaves:
        w = 2 ** l
        assert (g.level[aj:aj + w, ai:ai + w] == l).all() and g.plain[aj:aj + w, ai:ai + w].all()
        sides = (leaf[aj, ai + 1:ai + w + 1], leaf[aj + 1:aj + w + 1, ai + w + 1], leaf[aj + w + 1, ai + 1:ai + w + 1],
                 leaf[aj + 1:aj + w + 1, ai])
        for k, across in enumerate(sides):
            assert len(np.unique(across)) <= 2
            assert (len(np.unique(across)) == 2) == bool(mask >> k & 1)
    assert sum(4 ** l for (_i, _j, l, _m) in g.leaves) == int((g.level > 0).sum())
    assert int(g.cells_per_level.sum()) == (nx - 1) * (ny - 1)
    # every face of a leaf is right-isosceles and counter-clockwise, in exact lattice arithmetic
    p = g.leaf_tri_ij
    assert len(p) == int(g.leaf_face.sum())
    if len(p):
        e = np.stack([p[:, (k + 1) % 3] - p[:, k] for k in range(3)], axis=1)
        l2 = np.sort((e * e).sum(axis=2), axis=1)
        assert (l2[:, 0] > 0).all() and np.array_equal(l2[:, 0], l2[:, 1]) and np.array_equal(l2[:, 2], 2 * l2[:, 0])
        assert (e[:, 0, 0] * e[:, 1, 1] - e[:, 0, 1] * e[:, 1, 0] > 0).all()
        assert set(g.kind[g.tri[g.leaf_face]].reshape(-1).tolist()) == {0}


def test_every_fixture_holds_and_the_fixtures_reach_every_template():
    """The properties on every fixture; and over the set, leaves with each of the 16 hang masks and at every level of every
    threshold set, so that a change of the fixtures cannot hide a template."""
    masks, levels_seen, most = set(), {}, {}
    for name, h, t, seeds in fixtures():
        poly, g = graded_of(name, h, t, seeds)
        hold(poly, g, t)
        masks |= {m for (_i, _j, _l, m) in g.leaves}
        levels_seen.setdefault(t, set()).update(l for (_i, _j, l, _m) in g.leaves)
        if name == "negative" and not seeds:
            most[(h, t)] = (len(g.uniform.tri), len(g.tri))
    print("hang masks", sorted(masks))
    print("faces of the 40 x 30 rectangle, uniform and graded", most)
    assert masks == set(range(16))
    for t, seen in levels_seen.items():
        assert seen == set(range(1, len(t))), (t, seen)


def test_the_seeds_are_fine_spots():
    """A seed in the lattice takes its cell to level 0 (on a lattice line: the cell above and to the right of it, by the
    floor); one outside changes nothing; the mesh without seeds is coarser."""
    for h in SPACINGS:
        _poly, bare = graded_of("negative", h, (0, 2, 4), ())
        _poly, g = graded_of("negative", h, (0, 2, 4), tuple(NEGATIVE_SEEDS))
        i0, j0, nx, ny = g.lattice
        cells = [(math.floor(x / h) - i0, math.floor(y / h) - j0) for x, y in NEGATIVE_SEEDS]
        assert not 0 <= cells[1][0] < nx - 1
        assert cells[2] == (round(-10.0 / h) - i0, round(-8.0 / h) - j0)
        for k in (0, 2):
            ci, cj = cells[k]
            assert bare.plain[cj, ci] and not g.plain[cj, ci] and g.level[cj, ci] == 0 and bare.level[cj, ci] > 0
            assert (g.level[cj - 1:cj + 2, ci - 1:ci + 2] == 0).all()          # t[1] = 2: the ring round it too
        assert not bare.plain[cells[3][1], cells[3][0]]
        assert len(g.tri) > len(bare.tri)
        _poly, outside_only = graded_of("negative", h, (0, 2, 4), (NEGATIVE_SEEDS[1],))
        assert np.array_equal(outside_only.tri, bare.tri) and np.array_equal(outside_only.xy, bare.xy)


def test_one_level_is_the_uniform_mesh_exactly():
    for h in SPACINGS:
        for name, poly in G.seven_shapes(h).items():
            u = G.mesh_polygon(poly, h)
            g = GG.mesh_polygon_graded(poly, h, [0], SHAPE_SEEDS)
            assert np.array_equal(g.xy.view(np.int64), u.xy.view(np.int64)) and np.array_equal(g.tri, u.tri)
            assert np.array_equal(g.kind, u.kind) and g.tri.dtype == u.tri.dtype


def test_the_rectangle_loses_about_half_its_faces_under_the_default_ramp():
    """The 40 x 30 rectangle at h = 0.25 with the default ramp (factor 3: one level): the figure of the issue's prototype is
    13 557 -> 7 123 faces at the default spacing; here the same ramp on the fixtures' lattice."""
    t = tuple(GG.host_thresholds(0.25, 3.0, 0.5, 3.0))
    _poly, g = graded_of("negative", 0.25, t, ())
    print("faces", len(g.uniform.tri), "->", len(g.tri), "cells per level", g.cells_per_level.tolist())
    assert len(g.tri) < 0.6 * len(g.uniform.tri)


# ---- the thresholds ------------------------------------------------------------------------------------------------------------

def test_the_threshold_formula_on_hand_computed_cases():
    """By hand.  Default config (factor 3, 0.5 to 3.0): one level, dist_1 = 0.5 + 1/2 * 2.5 = 1.75; at h = 0.5 that is
    3.5 cells, ceil 4, t[1] = 5; at h = 0.25 7 cells, t[1] = 8.  Factor 8, 0.5 to 4.0, h = 0.25: dist = 0.5 + (1, 3, 7) / 7 *
    3.5 = 1.0, 2.0, 4.0 -> 1 + (4, 8, 16) = 5, 9, 17.  Factor 8 with dmin = 0, dmax = 0.7, h = 1: dist = 0.1, 0.3, 0.7 ->
    1 + 1 = 2 each, and the balance term takes over: 2, 2 + 2 = 4, 4 + 4 = 8."""
    assert gridmesh.graded_thresholds(0.5, 3.0, 0.5, 3.0) == [0, 5]
    assert gridmesh.graded_thresholds(0.25, 3.0, 0.5, 3.0) == [0, 8]
    assert gridmesh.graded_thresholds(0.25, 8.0, 0.5, 4.0) == [0, 5, 9, 17]
    assert gridmesh.graded_thresholds(1.0, 8.0, 0.0, 0.7) == [0, 2, 4, 8]
    assert gridmesh.graded_thresholds(0.25, 8.0, 0.5, 4.0, max_level=2) == [0, 5, 9]
    assert gridmesh.graded_thresholds(0.25, 8.0, 0.5, 4.0, max_level=0) == [0]
    assert gridmesh.graded_thresholds(0.25, 1.999, 0.5, 4.0) == [0] and gridmesh.graded_thresholds(0.25, 1.0, 0.5, 4.0) == [0]
    assert len(gridmesh.graded_thresholds(0.25, 1000.0, 0.5, 4.0)) == 6          # capped at level 5
    for args in ((0.5, 3.0, 0.5, 3.0), (0.25, 8.0, 0.5, 4.0), (1.0, 8.0, 0.0, 0.7), (0.3, 64.0, 0.1, 0.2)):
        t = gridmesh.graded_thresholds(*args)
        assert t == GG.host_thresholds(*args) and GG.check_thresholds(t) == t
    cfg = mesh.Mesher.Config(maximum_size=0.5 * math.sqrt(2.0))
    assert GridMesher(cfg, graded=True).thresholds() == GG.host_thresholds(cfg.maximum_size / math.sqrt(2.0), 3.0, 0.5, 3.0)
    assert GridMesher(cfg).thresholds() == [0]


# ---- GridMesher(graded=True) on the restatement ---------------------------------------------------------------------------------

CALLS = []


def host_engine_graded(polygons, h, snap, thresholds, seeds):
    CALLS.append((h, snap, list(thresholds), np.array(seeds)))
    out = []
    for rings in polygons:
        g = GG.mesh_polygon_graded(rings, h, thresholds, seeds, snap)
        out.append((g.xy, g.tri, g.kind, g.cells_per_level))
    return out


def host_mesher(**kw):
    return GridMesher(engine=host_engine_graded, graded=True, **kw)


def test_the_mesher_hands_thresholds_and_seeds_to_the_engine_and_reports_the_levels():
    cfg = mesh.Mesher.Config(maximum_size=0.25 * math.sqrt(2.0), variable_size_maximum_factor=8.0,
                             variable_density_min_distance=0.5, variable_density_max_distance=4.0)
    mesher = host_mesher(config=cfg)
    seeds = [mesh.Point(x, y) for x, y in NEGATIVE_SEEDS]
    del CALLS[:]
    (m, small) = mesher.polys_to_meshes([Polygon(NEGATIVE_RECT[0]), structured.Rect(0.1, 0.2, 1.3, 1.4)], seeds)
    (h, snap, t, got_seeds), = CALLS
    assert t == [0, 5, 9, 17] and snap == 0.25 and np.array_equal(got_seeds, np.array(NEGATIVE_SEEDS))
    want = GG.mesh_polygon_graded(NEGATIVE_RECT, h, t, NEGATIVE_SEEDS)
    assert np.array_equal(m.points, want.xy) and np.array_equal(m.triangles, want.tri)
    rep, rep_small = mesher.last_report
    assert rep["thresholds"] == t and rep["cells_per_level"] == want.cells_per_level.tolist()
    assert all(c > 0 for c in rep["cells_per_level"]) and rep["faces"] == len(want.tri) < len(want.uniform.tri)
    assert rep["components"] == 1 and abs(rep["area_ratio"] - 1.0) < 0.01
    assert rep_small["cells_per_level"][1:] == [0, 0, 0] and len(small.triangles) > 0          # too small for any block
    # every seed inside the copper within the reach the uniform mesher holds them to
    inside = [s for s in NEGATIVE_SEEDS if Polygon(NEGATIVE_RECT[0]).contains_xy(*s)]
    assert len(inside) == 3
    for x, y in inside:
        assert np.hypot(m.points[:, 0] - x, m.points[:, 1] - y).min() <= cfg.maximum_size
    assert host_mesher(config=cfg).polys_to_meshes([]) == []


def test_a_factor_below_two_and_max_level_zero_give_the_uniform_mesh():
    poly = Polygon(G.ell())
    u = G.mesh_polygon([G.ell()], 0.25)
    for kw in ({"config": mesh.Mesher.Config(maximum_size=0.25 * math.sqrt(2.0), variable_size_maximum_factor=1.9)},
               {"spacing": 0.25, "max_level": 0}):
        mesher = host_mesher(**kw)
        m = mesher.poly_to_mesh(poly, [mesh.Point(1.0, 1.0)])
        assert np.array_equal(m.points, u.xy) and np.array_equal(m.triangles, u.tri)
        assert mesher.last_report[0]["thresholds"] == [0] and mesher.last_report[0]["cells_per_level"] == [u.state[:-1, :-1].size]


def test_the_uniform_mesher_is_unchanged():
    """``graded=False`` (the default): the engine is called with (polygons, h, snap) and the report has no new key."""
    seen = []

    def engine(polygons, h, snap):
        seen.append((h, snap))
        return [(m.xy, m.tri, m.kind) for m in (G.mesh_polygon(p, h, snap) for p in polygons)]
    mesher = GridMesher(spacing=0.5, engine=engine)
    mesher.poly_to_mesh(Polygon(G.ell()), [mesh.Point(1.0, 1.0)])
    assert seen == [(0.5, 0.25)] and mesher.graded is False
    assert set(mesher.last_report[0]) == {"lattice", "vertices", "faces", "area_ratio", "components"}


def test_graded_errors():
    square = Polygon([(0, 0), (8, 0), (8, 8), (0, 8)])
    for kw in ({"max_level": -1}, {"max_level": 6}, {"max_level": 1.5}, {"max_level": True}, {"snap": 0.5}, {"spacing": 0.0}):
        with pytest.raises(ValueError):
            host_mesher(**kw)
    with pytest.raises(mesh.MeshingException, match="maximum_size"):
        host_mesher(config=mesh.Mesher.Config(maximum_size=0.0)).poly_to_mesh(square)
    with pytest.raises(ValueError, match="finite"):
        host_mesher(spacing=0.5).poly_to_mesh(square, [(float("nan"), 1.0)])
    with pytest.raises(ValueError, match="spacing is too small"):
        host_mesher(spacing=1e-12).poly_to_mesh(square)
    # a seed the copper around which was lost is still refused, and so is a mesh in pieces
    arm = Polygon([(0, 0), (4, 0), (4, 3), (3.9, 3), (3.9, 10), (3.7, 10), (3.7, 3), (0, 3)])
    with pytest.raises(mesh.MeshingException, match="seed"):
        host_mesher(spacing=0.5, crumbs="drop").poly_to_mesh(arm, [mesh.Point(3.8, 9.5)])
    with pytest.raises(mesh.MeshingException, match="pieces"):
        host_mesher(spacing=0.5).poly_to_mesh(Polygon(G.rotated(G.rect(0, 0, 12, 0.4), 0.37, (0.07, 0.07))))
    # the restatement refuses what the entry refuses
    for t in ([], [1, 2], [0, 0], [0, 1, 2], [0, 2, 3], [0, 1, 2, 4, 8, 16, 32]):
        with pytest.raises(ValueError):
            GG.mesh_polygon_graded([G.rect(0, 0, 4, 4)], 0.5, t)
    with pytest.raises(ValueError):
        GG.mesh_polygon_graded([G.rect(0, 0, 4, 4)], 0.5, [0, 2], [(1.0, float("inf"))])

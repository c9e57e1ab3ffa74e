"""The connectivity pre-pass on the device (needs an MI355X): ``padne_polygons_locate`` against tests/connectivity_ref.py
exactly in hit_ptr, hit_poly and hit_kind, two calls, queries one at a time, the pool's guarded mode, the refusals, and
``compute_connectivity`` / ``prepare_board`` / ``solver.solve(..., prune=True)`` on the board whose undriven pad stops the
unpruned solve."""
import warnings

import numpy as np
import pytest

import connectivity_ref as R
import gridmesh_ref as G
from padne_amd import GridMesher, _hip, mesh, solver
from test_connectivity_host import (CONNECTED, KEPT, MAXIMUM_SIZE, direct_solve, hand_pruned_problem, host_mesher, pruned_board_problem,
                                    same_meshes)
from test_device_memory import three_ways
from test_gridmesh import potentials, sawtooth

pytestmark = pytest.mark.gpu

REL_TOL = 1e-8          # the project's bar, as in tests/test_gridmesh.py


def batch():
    """(polygons, groups, points, point_groups).  Group 0 has no polygon, group 1 one, group 2 130 (three chunks of 64, the last
    2 wide): 126 unit squares on a 14 x 9 grid, neighbours sharing sides and corners, the 600-segment sawtooth, the 96-gon with
    its 48-gon hole, a triangle, a rotated rectangle; group 3 has no polygon.  300 queries: 75 workgroups of four."""
    squares = [[G.rect(float(i), float(j), i + 1.0, j + 1.0)] for j in range(9) for i in range(14)]
    saw = [sawtooth() + np.array([0.0, 20.0])]
    gon = [G.ngon(96, 5.0, (30.17, 5.09)), G.ngon(48, 2.0, (30.31, 4.88), 0.05)]
    tri = [np.array([[20.0, 0.0], [24.0, 0.0], [20.0, 3.0]])]
    rot = [G.rotated(G.rect(0, 0, 8, 3), 0.3, (40.05, 0.02))]
    polygons = [[G.rect(0.0, 0.0, 3.0, 2.0)]] + squares[:70] + [saw, gon] + squares[70:] + [tri, rot]
    groups = [1] + [2] * 130
    assert len(polygons) == 131 and len(R.segments_of(saw)) > 600
    rng = np.random.default_rng(5)
    pts = []
    pts += [(i + 0.5, j + 0.25) for i, j in rng.integers(0, 9, (40, 2))]                             # interiors of squares
    pts += [(float(i), float(j)) for i, j in rng.integers(0, 10, (40, 2))]                            # shared corners: 1, 2 or 4 hits
    pts += [(i + 0.5, float(j)) for i, j in rng.integers(1, 9, (20, 2))]                              # shared sides: 2 hits
    pts += [(float(i), j + 0.75) for i, j in rng.integers(1, 9, (20, 2))]
    pts += [tuple(p) for p in gon[0][::8]] + [tuple(p) for p in gon[1][::8]]                          # ring vertices: 12 + 6
    pts += [tuple(p) for p in saw[0][::40]] + [tuple(p) for p in rot[0]] + [tuple(p) for p in tri[0]]  # 16 + 4 + 3
    pts += [(30.31, 4.88), (30.9, 5.3), (29.5, 4.2)]                                                  # in the hole
    pts += [(30.17, 9.0), (27.0, 5.0), (33.5, 6.0), (26.0, 1.0), (34.3, 9.2)]                         # in the 96-gon; in its box only
    pts += [(15.0, 20.05), (15.0, 21.75), (0.0, 20.5), (7.5, 20.1), (29.99, 21.0)]                    # sawtooth: in, between teeth, on a side
    pts += [(22.0, 0.0), (20.0, 1.5), (23.0, 2.5), (21.0, 1.0), (22.0, 1.5)]                          # triangle: on, on, in the box, in, on the slant
    pts += [(41.0, 1.0), (40.2, 2.9), (47.0, 0.3), (44.0, 2.5)]                                       # rotated rectangle: in and in its box only
    pts += [(100.0, 100.0), (-5.0, 3.0), (50.0, -8.0)]                                                # outside every box
    special = len(pts)
    pts += [tuple(p) for p in rng.uniform((-1.0, -1.0), (49.0, 23.0), (300 - special - 8, 2))]
    pts += pts[:8]                                                                                    # duplicates
    pts = np.array(pts, dtype=np.float64)
    assert pts.shape == (300, 2)
    point_groups = np.full(300, 2, dtype=np.int32)
    point_groups[5::9] = 1                  # against the one rectangle of group 1
    point_groups[7::31] = 0                 # a group in front of every polygon
    point_groups[11::37] = 3                # a group behind every polygon
    return polygons, np.array(groups, dtype=np.int32), pts, point_groups


@pytest.fixture(scope="module")
def expected():
    polygons, groups, pts, point_groups = batch()
    want = R.locate(polygons, groups, pts, point_groups)
    per_query = np.diff(want[0])
    kinds = np.bincount(want[2], minlength=3)
    print("hits", len(want[1]), "by kind", kinds.tolist(), "most hits of a query", per_query.max(), "queries without", int((per_query == 0).sum()))
    # the batch does what the docstring says: two to four hits, both kinds, both halves of every decision
    assert per_query.max() == 4 and (per_query == 2).any() and (per_query == 0).sum() > 30 and kinds[1] > 50 and kinds[2] > 80
    assert set(want[1].tolist()) >= {0, 71, 72, 129, 130}
    return want


def assert_same(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w)


def test_locate_against_the_restatement_and_twice(ctx, expected):
    polygons, groups, pts, point_groups = batch()
    got = _hip.locate_polygons(ctx, polygons, groups, pts, point_groups)
    assert_same(got, expected)
    assert_same(_hip.locate_polygons(ctx, polygons, groups, pts, point_groups), expected)
    for q in range(len(pts)):                               # a query's hits in ascending polygon number
        assert (np.diff(got[1][got[0][q]:got[0][q + 1]]) > 0).all()


def test_queries_one_at_a_time_give_the_rows_of_the_batch(ctx, expected):
    polygons, groups, pts, point_groups = batch()
    hit_ptr, hit_poly, hit_kind = expected
    for q in list(range(0, 300, 7)) + [299]:
        one = _hip.locate_polygons(ctx, polygons, groups, pts[q:q + 1], point_groups[q:q + 1])
        assert one[0].tolist() == [0, hit_ptr[q + 1] - hit_ptr[q]]
        assert np.array_equal(one[1], hit_poly[hit_ptr[q]:hit_ptr[q + 1]]) and np.array_equal(one[2], hit_kind[hit_ptr[q]:hit_ptr[q + 1]])


def test_no_queries_no_polygons_and_no_hit(ctx):
    polygons, groups, pts, point_groups = batch()
    hit_ptr, hit_poly, hit_kind = _hip.locate_polygons(ctx, polygons, groups, np.zeros((0, 2)), [])
    assert hit_ptr.tolist() == [0] and len(hit_poly) == 0 and len(hit_kind) == 0
    hit_ptr, hit_poly, hit_kind = _hip.locate_polygons(ctx, [], [], pts[:5], point_groups[:5])
    assert hit_ptr.tolist() == [0] * 6 and len(hit_poly) == 0 and len(hit_kind) == 0
    hit_ptr, hit_poly, hit_kind = _hip.locate_polygons(ctx, polygons, groups, [(100.0, 100.0), (3.5, 3.5)], [2, 3])
    assert hit_ptr.tolist() == [0, 0, 0] and len(hit_poly) == 0


def test_the_batch_under_the_guarded_allocator(ctx, switches):
    polygons, groups, pts, point_groups = batch()
    three_ways(ctx, switches, lambda: list(_hip.locate_polygons(ctx, polygons, groups, pts, point_groups)))


def test_refusals(ctx):
    square = [G.rect(0, 0, 2, 2)]
    pts = [(1.0, 1.0)]
    for polygons, groups, points, point_groups in (
            ([[G.rect(0, 0, 2, 2)[:2]]], [0], pts, [0]),                                    # a ring of two vertices
            ([[np.array([[0, 0], [1, 0], [1, np.inf]])]], [0], pts, [0]),                   # a coordinate that is not finite
            ([square], [0], [(np.nan, 1.0)], [0]), ([square], [0], [(1.0, -np.inf)], [0]),  # a query that is not finite
            ([square, square], [1, 0], pts, [0]),                                           # groups not ascending
            ([square], [-1], pts, [0]), ([square], [0], pts, [-1]),                         # a negative group
            ([[]], [0], pts, [0]),                                                          # a polygon without a ring
            ([square], [0, 0], pts, [0]), ([square], [0], pts, [0, 0]), ([square], [2 ** 31], pts, [0])):
        with pytest.raises(ValueError):
            _hip.locate_polygons(ctx, polygons, groups, points, point_groups)
    assert ctx._lib.padne_polygons_locate_destroy(None) == 0
    assert _hip.locate_polygons(ctx, [square], [0], pts, [0])[2].tolist() == [1]           # the context still works


# ---- the board -------------------------------------------------------------------------------------------------------------------

def device_mesher(**kw):
    return GridMesher(mesh.Mesher.Config(maximum_size=MAXIMUM_SIZE), **kw)


def test_connectivity_and_prepare_board_on_the_device_equal_the_host_engines(ctx):
    prob = pruned_board_problem()
    got, want = solver.compute_connectivity(prob), solver.compute_connectivity(prob, locate=R.locate)
    assert got == want and got.connected == CONNECTED
    for mode in ("skip", "mesh"):
        dev = solver.prepare_board(prob, mesher=device_mesher(), disconnected=mode)
        host = solver.prepare_board(prob, mesher=host_mesher(), locate=R.locate, disconnected=mode)
        same_meshes(dev.meshes, host.meshes)
        assert dev.mesh_index_to_layer_index == host.mesh_index_to_layer_index and dev.connectivity == host.connectivity
        assert [prob.networks.index(n) for n in dev.filtered_networks] == KEPT
        for d, h in zip(dev.disconnected_meshes_by_layer, host.disconnected_meshes_by_layer):
            same_meshes(d, h)
        assert dev.skipped == host.skipped
    assert [len(d) for d in dev.disconnected_meshes_by_layer] == [2, 1] and [s[:2] for s in dev.skipped] == [(0, 4)]


def test_solve_with_prune(ctx):
    prob = pruned_board_problem()
    with pytest.raises(mesh.MeshingException, match="no face"):
        solver.solve(prob, mesher=device_mesher(), prune=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        sol = solver.solve(prob, mesher=device_mesher(), prune=True)
        by_hand = solver.solve(hand_pruned_problem(), mesher=device_mesher())
        board = solver.prepare_board(prob, mesher=device_mesher(), disconnected="mesh")
        shown = solver.solve_meshed(prob, board.meshes, board.mesh_index_to_layer_index, filtered_networks=board.filtered_networks,
                                    disconnected_meshes_by_layer=board.disconnected_meshes_by_layer)
    assert sol.solver_info.residual_norm < 1e-9
    got = potentials(sol)
    v, n_vert, _off, res, _L = direct_solve(prob, board.meshes, board.mesh_index_to_layer_index, board.filtered_networks)
    err = np.abs(got - v[:n_vert]).max() / np.abs(v[:n_vert]).max()
    print("pruned board:", n_vert, "vertices, relative deviation from the direct solve", err, "drop", np.ptp(got), "residual", res)
    assert len(got) == n_vert and res < 1e-9 and np.ptp(got) > 0.5
    assert err <= REL_TOL
    assert np.array_equal(got.view(np.int64), potentials(by_hand).view(np.int64))            # bit for bit the hand-pruned Problem
    assert [len(ls.meshes) for ls in sol.layer_solutions] == [3, 1]
    assert [len(ls.disconnected_meshes) for ls in sol.layer_solutions] == [0, 0]
    assert len(shown.layer_solutions[0].disconnected_meshes) == 2 and len(shown.layer_solutions[1].disconnected_meshes) == 1
    assert np.array_equal(potentials(shown).view(np.int64), got.view(np.int64))


def test_solve_currents_with_prune(ctx):
    """One wrapper: the resistor of network 4 ends on geom 5, which nothing else touches, and carries no current."""
    prob = pruned_board_problem()
    with pytest.raises(mesh.MeshingException, match="no face"):
        solver.solve_currents(prob, mesher=device_mesher())
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        _sol, report = solver.solve_currents(prob, mesher=device_mesher(), prune=True)
    assert len(report.elements) == 4                                    # network 3, on dead copper, is not solved
    source = abs(report.elements[prob.networks[0].elements[0]]["current"])
    dangling = abs(report.elements[prob.networks[4].elements[0]]["current"])
    print("source current", source, "through the dangling resistor", dangling)
    assert source > 0.1 and dangling <= 1e-8 * source

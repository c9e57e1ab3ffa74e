"""The graded grid mesher on the device (needs an MI355X): ``padne_polymesh_create_graded`` against
tests/gridmesh_graded_ref.py bit for bit in xy, tri and kind (and the cells per level), a batch with seeds against its polygons
one at a time, two calls, one level against ``padne_polymesh_create``, a row of three workgroups, the refusals, the pool's
guarded mode, and ``solver.solve(prob, mesher=GridMesher(config, graded=True))`` on an L-shaped pour with an antipad."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import gridmesh_graded_ref as GG
import gridmesh_ref as G
from oracle import padne_oracle as O
from padne_amd import GridMesher, Polygon, _hip, mesh, problem, solver, structured
from test_device_memory import three_ways
from test_gridmesh_graded_host import NEGATIVE_RECT, NEGATIVE_SEEDS, SHAPE_SEEDS

pytestmark = pytest.mark.gpu

REL_TOL = 1e-8          # the bar of the existing parity tests (tests/test_load_cases.py)


def assert_same(got, want):
    xy, tri, kind, cells = got
    assert xy.dtype == np.float64 and tri.dtype == np.int32 and kind.dtype == np.int32 and cells.dtype == np.int64
    assert xy.shape == want.xy.shape and tri.shape == want.tri.shape
    assert np.array_equal(tri, want.tri) and np.array_equal(kind, want.kind)
    assert np.array_equal(xy.view(np.int64), want.xy.view(np.int64))
    assert np.array_equal(cells, want.cells_per_level)


@pytest.mark.parametrize("h", [0.5, 0.25])
def test_the_seven_shapes_bit_for_bit(ctx, h):
    shapes = G.seven_shapes(h)
    got = _hip.polymesh_graded(ctx, list(shapes.values()), h, 0.25, [0, 2, 4])
    levels = set()
    for name, g in zip(shapes, got):
        want = GG.mesh_polygon_graded(shapes[name], h, [0, 2, 4])
        print(name, h, want.lattice[2:], len(want.xy), "vertices", len(want.tri), "faces, uniform", len(want.uniform.tri),
              "cells per level", want.cells_per_level.tolist())
        assert_same(g, want)
        levels |= {l for (_i, _j, l, _m) in want.leaves}
    assert levels == ({1, 2} if h == 0.25 else {1})         # (at 0.5 no shape is wide enough for a block of 4 x 4 with d >= 4)


def mixed_batch():
    """The 40 x 30 rectangle at negative coordinates, a polygon too small for any block of cells, the 96-gon with the
    48-gon; the seeds of the rectangle and of the shapes together, so that some fall into every lattice, some into none."""
    return [NEGATIVE_RECT, [G.rect(0.1, 0.2, 1.3, 1.4)], G.seven_shapes(0.5)["gon96_hole48"]], 0.5, NEGATIVE_SEEDS + SHAPE_SEEDS


BATCH_THRESHOLDS = ((0, 2, 4), (0, 5, 8, 13), (0, 1, 3, 7))


@functools.lru_cache(maxsize=None)
def batch_reference(t):
    polys, h, seeds = mixed_batch()
    return [GG.mesh_polygon_graded(p, h, list(t), seeds) for p in polys]


def test_the_batches_reach_every_template():
    """Over the three threshold sets the batch below holds leaves with each of the 16 hang masks."""
    assert {m for t in BATCH_THRESHOLDS for w in batch_reference(t) for (_i, _j, _l, m) in w.leaves} == set(range(16))


@pytest.mark.parametrize("t", BATCH_THRESHOLDS)
def test_a_mixed_batch_with_seeds_bit_for_bit_twice_and_one_at_a_time(ctx, t):
    polys, h, seeds = mixed_batch()
    want = batch_reference(t)
    assert max(w.lattice[2] * w.lattice[3] for w in want) <= 100 * 100
    assert {l for (_i, _j, l, _m) in want[0].leaves} == set(range(1, len(t))) and not want[1].leaves and len(want[1].tri) > 0
    assert len({m for w in want for (_i, _j, _l, m) in w.leaves}) >= 10          # most of the 16 templates in one call
    bare = GG.mesh_polygon_graded(polys[0], h, list(t), uniform=want[0].uniform)
    assert len(bare.tri) < len(want[0].tri) < len(want[0].uniform.tri)              # the seeds refined, the levels coarsened
    got = _hip.polymesh_graded(ctx, polys, h, 0.25, list(t), seeds)
    again = _hip.polymesh_graded(ctx, polys, h, 0.25, list(t), seeds)
    for g, a, w, p in zip(got, again, want, polys):
        assert_same(g, w)
        assert_same(a, w)
        (alone,) = _hip.polymesh_graded(ctx, [p], h, 0.25, list(t), seeds)
        assert_same(alone, w)


def test_six_levels_with_the_least_thresholds(ctx):
    """The most levels the entry takes, each threshold the least the balance allows: one leaf of 32 x 32 cells in the middle
    of a square, every level round it."""
    poly, t = [G.rect(0.2, 0.2, 48.8, 48.8)], [0, 1, 3, 7, 15, 31]
    want = GG.mesh_polygon_graded(poly, 0.5, t)
    assert want.lattice[2] * want.lattice[3] <= 101 * 101 and (want.cells_per_level > 0).all()
    assert want.cells_per_level[5] == 32 * 32
    (got,) = _hip.polymesh_graded(ctx, [poly], 0.5, 0.25, t)
    assert_same(got, want)


def test_a_row_longer_than_two_workgroups(ctx):
    """More than 512 lattice vertices in a row: leaves of 4 x 4 cells straddle the 256-vertex chunks of the row kernels, and
    a second polygon follows in the batch."""
    polys = [[G.rotated(G.rect(0.1, 0.3, 149.3, 4.4), 0.004, (0.05, 0.02))], [G.rect(0.1, 0.3, 5.3, 2.7)]]
    seeds = [(60.01, 2.3), (120.9, 2.6)]
    want = [GG.mesh_polygon_graded(p, 0.25, [0, 2, 4], seeds) for p in polys]
    nx = want[0].lattice[2]
    assert nx > 2 * 256 and nx % 256 != 0 and nx * want[0].lattice[3] <= 2 * 100 * 100
    i0 = want[0].lattice[0]
    for edge in (256, 512):                  # a leaf of level 2 across each chunk edge
        assert any(l == 2 and ci < edge < ci + 4 for (ci, _cj, l, _m) in want[0].leaves), (edge, i0)
    for g, w in zip(_hip.polymesh_graded(ctx, polys, 0.25, 0.25, [0, 2, 4], seeds), want):
        assert_same(g, w)


def test_one_level_is_the_uniform_call_bit_for_bit(ctx):
    polys, h, seeds = mixed_batch()
    for g, u in zip(_hip.polymesh_graded(ctx, polys, h, 0.25, [0], seeds), _hip.polymesh(ctx, polys, h)):
        assert np.array_equal(g[0].view(np.int64), u[0].view(np.int64)) and np.array_equal(g[1], u[1]) and np.array_equal(g[2], u[2])
        assert g[0].dtype == u[0].dtype and g[1].dtype == u[1].dtype and g[2].dtype == u[2].dtype and len(g[3]) == 1
    nx, ny = G.mesh_polygon(polys[0], h).lattice[2:]
    assert _hip.polymesh_graded(ctx, polys, h)[0][3].tolist() == [(nx - 1) * (ny - 1)]


def test_argument_errors(ctx):
    square = [G.rect(0, 0, 8, 8)]
    for t, seeds in (([], []), ([0, 1, 3, 7, 15, 31, 63], []), ([1, 2], []), ([0, 0], []), ([0, 2, 3], []), ([0, 1, 3, 6], []),
                     ([0, 2], [(1.0, float("nan"))]), ([0, 2], [(float("inf"), 1.0)]), ([0, 2.5], []), ([0, 2 ** 31], [])):
        with pytest.raises(ValueError):
            _hip.polymesh_graded(ctx, [square], 0.5, 0.25, t, seeds)
    # what the uniform entry refuses
    for polys, h, snap in (([[G.rect(0, 0, 2, 2)[:2]]], 0.5, 0.25), ([square], 0.0, 0.25), ([square], 0.5, 0.5), ([], 0.5, 0.25)):
        with pytest.raises(ValueError):
            _hip.polymesh_graded(ctx, polys, h, snap, [0, 2])
    # null pointers where a count is positive, through the entry itself
    prp, rp, xy = np.array([0, 1], dtype=np.int64), np.array([0, 4], dtype=np.int64), np.ascontiguousarray(square[0])
    t, seed = np.array([0, 2], dtype=np.int32), np.array([[1.0, 1.0]])
    nv, nt = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)

    def call(threshold, n_seed, seed_xy, out=True):
        handle = C.c_void_p()
        rc = ctx._lib.padne_polymesh_create_graded(ctx._h, 1, _hip._ptr(prp, _hip._PI64), _hip._ptr(rp, _hip._PI64),
                                                   _hip._ptr(xy, _hip._PF64), 0.5, 0.25, 2, threshold, n_seed, seed_xy,
                                                   _hip._ptr(nv, _hip._PI64), _hip._ptr(nt, _hip._PI64), None,
                                                   C.byref(handle) if out else None)
        assert handle.value is None or rc == 0
        if handle.value is not None:
            ctx._lib.padne_polymesh_destroy(handle)
        return rc
    assert call(_hip._ptr(t, _hip._PI32), 1, _hip._ptr(seed, _hip._PF64)) == 0           # (level_cells_out may be NULL)
    assert call(_hip._ptr(t, _hip._PI32), 0, None) == 0
    for args in ((None, 0, None), (_hip._ptr(t, _hip._PI32), 1, None), (_hip._ptr(t, _hip._PI32), 0, None, False)):
        with pytest.raises(ValueError):
            _hip._check(call(*args))


def test_the_batch_under_the_guarded_allocator(ctx, switches):
    polys, h, seeds = mixed_batch()
    three_ways(ctx, switches, lambda: [list(m) for m in _hip.polymesh_graded(ctx, polys, h, 0.25, [0, 2, 4, 8], seeds)])


# ---- solve ---------------------------------------------------------------------------------------------------------------------

SCALE = 4.0


def pour_problem():
    """The L-shaped pour with a round antipad over a rectangle of tests/test_gridmesh.py, four times the size, so that the
    arms are wide enough for leaves; a current source across the L instead of the voltage source, so that the drop between its
    terminals depends on the mesh."""
    k = SCALE
    pour = Polygon(G.ell(6.0 * k, 4.0 * k, 1.7 * k, (0.11, 0.23)), holes=[G.ngon(24, 0.4 * k, (1.0 * k, 1.1 * k))])
    top = problem.Layer(shape=structured.Shapes.of(pour), name="F.Cu", conductance=2.0)
    bottom = problem.Layer(shape=structured.Shapes.of(structured.Rect(0.3 * k, 0.4 * k, 5.7 * k, 1.6 * k)), name="B.Cu", conductance=1.5)

    def P(x, y):
        return mesh.Point(x * k, y * k)
    a, b = problem.Connection(layer=top, point=P(5.8, 0.9)), problem.Connection(layer=top, point=P(0.9, 3.9))
    c, d = problem.Connection(layer=top, point=P(3.0, 1.0)), problem.Connection(layer=bottom, point=P(3.0, 1.0))
    e, f = problem.Connection(layer=bottom, point=P(0.6, 0.8)), problem.Connection(layer=top, point=P(0.6, 0.8))
    nets = [problem.Network(connections=[a, b], elements=[problem.CurrentSource(f=b.node_id, t=a.node_id, current=1.0)]),
            problem.Network(connections=[c, d], elements=[problem.Resistor(a=c.node_id, b=d.node_id, resistance=0.01)]),
            problem.Network(connections=[e, f], elements=[problem.Resistor(a=e.node_id, b=f.node_id, resistance=0.02)])]
    return problem.Problem(layers=[top, bottom], networks=nets)


def potentials(sol):
    return np.concatenate([zf.values for ls in sol.layer_solutions for zf in ls.potentials])


def solved(prob, mesher):
    """(potentials of solver.solve, relative deviation from the direct solve on the same meshes, the mesher's report)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        meshes, layer_of = solver.mesh_problem(prob, mesher=mesher)
        report = list(mesher.last_report)
        sol = solver.solve(prob, mesher=mesher)
    assert [len(m.points) for m in meshes] == [len(m.points) for ls in sol.layer_solutions for m in ls.meshes]
    board = solver.index_board(prob, meshes, layer_of)
    with board.assembled() as (L, r):
        v, _gc, res = O.solve_system(L.tocsr(), r)
    n_vert = len(board.vindex)
    got = potentials(sol)
    assert res < 1e-9
    return got, np.abs(got - v[:n_vert]).max() / np.abs(v[:n_vert]).max(), report, meshes


def test_solve_on_the_graded_pour_against_the_direct_solve_and_the_uniform_mesh(ctx):
    prob = pour_problem()
    cfg = mesh.Mesher.Config(maximum_size=0.3)                  # the reference's default ramp: factor 3, one level
    graded = GridMesher(cfg, graded=True)
    got, err, report, meshes = solved(prob, graded)
    # the meshes are the restatement's, seeds and all; the last layer meshed is the bottom rectangle
    h = 0.3 / np.sqrt(2.0)
    seeds = [(c.point.x, c.point.y) for n in prob.networks for c in n.connections if c.layer is prob.layers[1]]
    want = GG.mesh_polygon_graded([G.rect(0.3 * SCALE, 0.4 * SCALE, 5.7 * SCALE, 1.6 * SCALE)], h, graded.thresholds(), seeds)
    assert np.array_equal(meshes[1].points, want.xy) and np.array_equal(meshes[1].triangles, want.tri)
    assert report[0]["cells_per_level"] == want.cells_per_level.tolist() and report[0]["cells_per_level"][1] > 0
    from padne_amd import gridmesh
    seeds = [(c.point.x, c.point.y) for n in prob.networks for c in n.connections if c.layer is prob.layers[0]]
    want = GG.mesh_polygon_graded(gridmesh.rings_of(prob.layers[0].geoms[0]), h, graded.thresholds(), seeds)
    assert np.array_equal(meshes[0].points, want.xy) and np.array_equal(meshes[0].triangles, want.tri)
    assert any(l >= 1 for (_i, _j, l, _m) in want.leaves) and len(want.tri) < len(want.uniform.tri)
    print("the pour's cells per level", want.cells_per_level.tolist(), "the rectangle's", report[0]["cells_per_level"])
    uniform, err_u, _rep, meshes_u = solved(prob, GridMesher(cfg))
    assert sum(len(m.triangles) for m in meshes) < sum(len(m.triangles) for m in meshes_u)
    print("graded pour:", [len(m.points) for m in meshes], "vertices", [len(m.triangles) for m in meshes], "faces; uniform",
          [len(m.points) for m in meshes_u], "vertices", [len(m.triangles) for m in meshes_u], "faces")
    print("relative deviation from the direct solve: graded", err, "uniform", err_u)
    print("drop between the terminals: graded", repr(np.ptp(got)), "uniform", repr(np.ptp(uniform)),
          "relative difference", abs(np.ptp(got) - np.ptp(uniform)) / np.ptp(uniform))
    assert np.ptp(got) > 0
    assert err <= REL_TOL

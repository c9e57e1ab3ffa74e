"""The grid mesher on the device (needs an MI355X): ``padne_polymesh_create`` against tests/gridmesh_ref.py bit for bit in
xy, tri and kind, a batch against its polygons one at a time, two calls, the pool's guarded mode, and
``solver.solve(prob, mesher=GridMesher(...))`` on a rotated strip and on an L-shaped pour with a hole."""
import warnings

import numpy as np
import pytest

import gridmesh_ref as G
from oracle import padne_oracle as O
from padne_amd import GridMesher, Polygon, _hip, mesh, problem, solver, structured
from test_device_memory import three_ways
from test_gridmesh_host import along_the_strip, rotated_strip_problem

pytestmark = pytest.mark.gpu

REL_TOL = 1e-8          # the bar of the existing parity tests (tests/test_load_cases.py)


def sawtooth(n_teeth=300, x1=30.0):
    """A strip whose upper side is a sawtooth of 2 * n_teeth segments between y = 1.6 and y = 1.9: at h = 0.5 all of them in
    the band [1.5, 2.0], which then spans several LDS chunks of 256."""
    x = np.linspace(x1, 0.0, 2 * n_teeth + 1)
    y = np.where(np.arange(2 * n_teeth + 1) % 2 == 0, 1.6, 1.9)
    return np.concatenate([[[0.0, 0.1], [x1, 0.1]], np.stack([x, y], axis=1)])


def mixed_batch():
    """(polygons, h): a polygon that covers one row of lattice vertices, one smaller than a cell (no face at all), the
    sawtooth, a hole inside one cell that touches no lattice vertex and crosses only a diagonal, the 96-gon with the 48-gon."""
    return [[G.rect(0.1, 0.3, 5.3, 0.7)],
            [G.rect(0.1, 0.1, 0.4, 0.4)],
            [sawtooth()],
            [G.rect(0.2, 0.2, 4.8, 3.8), G.rect(1.05, 1.2, 1.3, 1.45)],
            G.seven_shapes(0.5)["gon96_hole48"]], 0.5


def assert_same(got, want):
    xy, tri, kind = got
    assert xy.dtype == np.float64 and tri.dtype == np.int32 and kind.dtype == np.int32
    assert xy.shape == want.xy.shape and tri.shape == want.tri.shape
    assert np.array_equal(tri, want.tri) and np.array_equal(kind, want.kind)
    assert np.array_equal(xy.view(np.int64), want.xy.view(np.int64))


@pytest.mark.parametrize("h", [0.5, 0.25])
def test_the_seven_shapes_bit_for_bit(ctx, h):
    shapes = G.seven_shapes(h)
    got = _hip.polymesh(ctx, list(shapes.values()), h)
    for name, g in zip(shapes, got):
        want = G.mesh_polygon(shapes[name], h)
        print(name, h, want.lattice[2:], len(want.xy), "vertices", len(want.tri), "faces")
        assert_same(g, want)


def test_a_mixed_batch_bit_for_bit_twice_and_one_at_a_time(ctx):
    polys, h = mixed_batch()
    want = [G.mesh_polygon(p, h) for p in polys]
    assert len(want[1].tri) == 0 and len(want[0].tri) > 0
    assert max(w.lattice[2] * w.lattice[3] for w in want) <= 100 * 100
    seg = want[2].segments
    assert ((np.minimum(seg[:, 1], seg[:, 3]) >= 1.5) & (np.maximum(seg[:, 1], seg[:, 3]) <= 2.0)).sum() >= 600
    assert (want[3].sign[2:-2, 2:-2] == G.PLUS).all()                       # the hole changed no sign
    got = _hip.polymesh(ctx, polys, h)
    again = _hip.polymesh(ctx, polys, h)
    for g, a, w, p in zip(got, again, want, polys):
        assert_same(g, w)
        assert_same(a, w)
        (alone,) = _hip.polymesh(ctx, [p], h)
        assert_same(alone, w)


def test_another_snap_and_an_odd_spacing(ctx):
    polys = [G.seven_shapes(0.5)["star"], G.seven_shapes(0.5)["rect_rotated"]]
    for h, snap in ((0.37, 0.1), (0.61, 0.45)):
        for g, p in zip(_hip.polymesh(ctx, polys, h, snap), polys):
            assert_same(g, G.mesh_polygon(p, h, snap))


def test_a_row_longer_than_a_workgroup(ctx):
    """600 lattice vertices in a row: three workgroups per row, each staging the band for itself; the last one 88 wide."""
    polys = [[G.rotated(G.rect(0.1, 0.3, 149.3, 1.4), 0.004, (0.05, 0.02))], [G.rect(0.1, 0.3, 5.3, 0.7)]]
    want = G.mesh_polygon(polys[0], 0.25)
    assert want.lattice[2] > 2 * 256 and want.lattice[2] % 256 != 0 and want.lattice[2] * want.lattice[3] <= 100 * 100
    for g, p in zip(_hip.polymesh(ctx, polys, 0.25), polys):
        assert_same(g, G.mesh_polygon(p, 0.25))


def test_argument_errors(ctx):
    square = [G.rect(0, 0, 2, 2)]
    for polys, h, snap in (([[G.rect(0, 0, 2, 2)[:2]]], 0.5, 0.25), ([[np.array([[0, 0], [1, 0], [1, np.inf]])]], 0.5, 0.25),
                           ([square], 0.0, 0.25), ([square], -1.0, 0.25), ([square], 0.5, 0.0), ([square], 0.5, 0.5),
                           ([square], 1e-6, 0.25), ([], 0.5, 0.25)):
        with pytest.raises(ValueError):
            _hip.polymesh(ctx, polys, h, snap)
    assert ctx._lib.padne_polymesh_destroy(None) == 0


def test_the_batch_under_the_guarded_allocator(ctx, switches):
    polys, h = mixed_batch()
    three_ways(ctx, switches, lambda: [list(m) for m in _hip.polymesh(ctx, polys, h)])


def potentials(sol):
    return np.concatenate([zf.values for ls in sol.layer_solutions for zf in ls.potentials])


def test_solve_on_the_rotated_strip(ctx):
    prob = rotated_strip_problem()
    mesher = GridMesher(mesh.Mesher.Config(maximum_size=0.2))
    with warnings.catch_warnings():
        warnings.simplefilter("error", solver.SolverWarning)
        sol = solver.solve(prob, mesher=mesher)
    ls = sol.layer_solutions[0]
    msh, pot = ls.meshes[0], ls.potentials[0]
    want = G.mesh_polygon(gridmesh_rings(prob.layers[0].geoms[0]), 0.2 / np.sqrt(2.0))
    assert np.array_equal(msh.points, want.xy) and np.array_equal(msh.triangles, want.tri)
    assert mesher.last_report[0]["components"] == 1 and mesher.last_report[0]["lattice"] == want.lattice[2:]
    err = np.abs(pot.values - along_the_strip(msh.points) / 10.0).max()
    print("rotated strip:", len(msh.points), "vertices, largest deviation from linear", err)
    assert err < 0.05
    assert sol.solver_info.residual_norm < 1e-9


def gridmesh_rings(poly):
    from padne_amd import gridmesh
    return gridmesh.rings_of(poly)


def pour_problem():
    """An L-shaped pour with a round antipad and a rectangle on a second layer, a via between them, a source across the L."""
    pour = Polygon(G.ell(6.0, 4.0, 1.7, (0.11, 0.23)), holes=[G.ngon(24, 0.4, (1.0, 1.1))])
    top = problem.Layer(shape=structured.Shapes.of(pour), name="F.Cu", conductance=2.0)
    bottom = problem.Layer(shape=structured.Shapes.of(structured.Rect(0.3, 0.4, 5.7, 1.6)), name="B.Cu", conductance=1.5)
    P = mesh.Point
    a, b = problem.Connection(layer=top, point=P(5.8, 0.9)), problem.Connection(layer=top, point=P(0.9, 3.9))
    c, d = problem.Connection(layer=top, point=P(3.0, 1.0)), problem.Connection(layer=bottom, point=P(3.0, 1.0))
    e, f = problem.Connection(layer=bottom, point=P(0.6, 0.8)), problem.Connection(layer=top, point=P(0.6, 0.8))
    nets = [problem.Network(connections=[a, b], elements=[problem.VoltageSource(p=a.node_id, n=b.node_id, voltage=1.0)]),
            problem.Network(connections=[c, d], elements=[problem.Resistor(a=c.node_id, b=d.node_id, resistance=0.01)]),
            problem.Network(connections=[e, f], elements=[problem.Resistor(a=e.node_id, b=f.node_id, resistance=0.02)])]
    return problem.Problem(layers=[top, bottom], networks=nets)


def test_solve_on_an_l_shaped_pour_with_a_hole_against_the_direct_solve(ctx):
    prob = pour_problem()
    mesher = GridMesher(mesh.Mesher.Config(maximum_size=0.3))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        meshes, layer_of = solver.mesh_problem(prob, mesher=mesher)
        sol = solver.solve(prob, mesher=mesher)
    assert [len(m.points) for m in meshes] == [len(m.points) for ls in sol.layer_solutions for m in ls.meshes]
    board = solver.index_board(prob, meshes, layer_of)
    with board.assembled() as (L, r):
        v, _gc, res = O.solve_system(L.tocsr(), r)
    n_vert = len(board.vindex)
    got = potentials(sol)
    scale = np.abs(v[:n_vert]).max()
    err = np.abs(got - v[:n_vert]).max() / scale
    print("pour:", n_vert, "vertices, relative deviation from the direct solve", err, "drop", np.ptp(got))
    assert res < 1e-9 and np.ptp(got) > 0.5
    assert err <= REL_TOL

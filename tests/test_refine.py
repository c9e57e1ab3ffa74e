"""``refine_meshes`` and ``solve_meshed_adaptive`` on the device: every output bit for bit against the host restatement
(tests/refine_ref.py, itself checked by tests/test_refine_host.py), a closure that outlasts a batch of sweeps, several
meshes with an empty one between them, the raw entry's refusals, the adaptive loop and its four ways to stop, and a linear
potential on a refined mesh."""
import ctypes as C
import warnings

import numpy as np
import pytest

import error_ref as R
import helpers as H
import refine_ref as RR
import sensitivity_ref as S
from padne_amd import _hip, mesh, solver
from test_refine_host import MESH_SETS, mesh_set, random_flags

pytestmark = pytest.mark.gpu

REL_TOL = 1e-8
BOARD = "problem_mixed"
# max |V_adaptive - V_uniform| over the old vertices / max |V_uniform|, after three adaptive rounds at half the first estimate
# against one all-flags round, with the host restatement's meshes and the host reference's solves (see the adaptive test)
HOST_ADAPTIVE_VS_UNIFORM = 0.08611219988513481


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        return fn(*args, **kwargs)


def on_device(ms, flags):
    return solver.refine_meshes([mesh.Mesh(p, t) for p, t in ms], flags)


def assert_same(got, want):
    """A device Refinement against the restatement's, or against another device call: the same bits."""
    if isinstance(want, solver.Refinement):
        want_meshes = [(m.points, m.triangles) for m in want.meshes]
    else:
        want_meshes = want.meshes
    assert len(got.meshes) == len(want_meshes)
    for m, (p, t), par, wpar, ends, wends in zip(got.meshes, want_meshes, got.parents, want.parents, got.midpoint_ends,
                                                 want.midpoint_ends):
        assert m.points.dtype == np.float64 and m.triangles.dtype == np.int32 and par.dtype == np.int32 and ends.dtype == np.int32
        assert m.points.shape == p.shape and np.array_equal(m.points.view(np.int64), np.asarray(p).view(np.int64))
        assert np.array_equal(m.triangles, t) and np.array_equal(par, wpar) and np.array_equal(ends, wends)


@pytest.mark.parametrize("name", MESH_SETS)
def test_bit_for_bit_against_the_restatement(ctx, name):
    ms = mesh_set(name)
    kinds = {"none": [np.zeros(len(t), dtype=bool) for _, t in ms], "all": [np.ones(len(t), dtype=bool) for _, t in ms],
             "random": random_flags(ms, 5), "random again": random_flags(ms, 6)}
    for kind, flags in kinds.items():
        want = RR.refine(ms, flags)
        got = on_device(ms, flags)
        print(name, kind, sum(len(t) for _, t in ms), "->", sum(len(m.triangles) for m in got.meshes), "faces,", got.edges, "edges,",
              got.marked_by_flags, "marked by flags,", got.marked, "after the closure,", got.sweeps, "sweeps queued")
        assert_same(got, want)
        assert got.edges == len(want.edges.lo) and got.marked_by_flags == want.marks_flagged.sum() and got.marked == want.marks.sum()
        assert_same(on_device(ms, flags), got)                      # two device calls: the same bits
    # a second round on the device's own output
    again_flags = random_flags([(m.points, m.triangles) for m in got.meshes], 7)
    assert_same(solver.refine_meshes(got.meshes, again_flags), RR.refine([(m.points, m.triangles) for m in got.meshes], again_flags))


def strip(n=40, height=10.0):
    """A zigzag strip of ``n`` faces between y = 0 and y = height whose steps along x grow: face i is (v_i, v_i+1, v_i+2), it
    shares (v_i+1, v_i+2) with face i + 1, and that edge is its longest -- sqrt(step^2 + height^2) with a growing step, against
    the two steps along one line -- so the longest edges strictly increase along the strip."""
    steps = 0.1 + 0.01 * np.arange(n + 1)
    x = np.concatenate([[0.0], np.cumsum(steps)])
    pts = np.stack([x, height * (np.arange(n + 2) % 2)], axis=1)
    tri = np.array([[i, i + 2, i + 1] if i % 2 == 0 else [i, i + 1, i + 2] for i in range(n)], dtype=np.int32)
    return pts, tri


def test_a_closure_that_outlasts_a_batch_of_sweeps(ctx):
    pts, tri = strip()
    assert (RR.signed_areas(pts, tri) > 0).all()
    E = RR.edges_of(pts, tri.astype(np.int64))
    longest = E.d[E.of_face[np.arange(len(tri)), E.longest]]
    assert (np.diff(longest) > 0).all()
    flags = [np.arange(len(tri)) == 0]
    want = RR.refine([(pts, tri)], flags)
    assert want.sweeps == len(tri) - 1 and want.marks.sum() - want.marks_flagged.sum() == len(tri) - 1
    got = on_device([(pts, tri)], flags)
    print("strip of", len(tri), "faces: the restatement needs", want.sweeps, "sweeps, the device queued", got.sweeps)
    assert_same(got, want)
    assert got.sweeps > 4 and got.marked - got.marked_by_flags == len(tri) - 1      # more than one batch between host looks


def test_several_meshes_with_an_empty_one_between_them(ctx):
    ms = mesh_set("problem_many_meshes")
    assert len(ms) == 34
    empty = (np.zeros((0, 2)), np.zeros((0, 3), dtype=np.int32))
    bare = (np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.zeros((0, 3), dtype=np.int32))      # vertices without faces
    ms = ms[:17] + [empty, bare] + ms[17:]
    flags = [np.zeros(len(t), dtype=bool) for _, t in ms]
    flags[0][:], flags[-1][:] = True, True                            # islands 0 and 33 only
    got = on_device(ms, flags)
    assert_same(got, RR.refine(ms, flags))
    for i, ((p, t), m, par, ends) in enumerate(zip(ms, got.meshes, got.parents, got.midpoint_ends)):
        if 0 < i < len(ms) - 1:
            assert np.array_equal(m.points, p) and np.array_equal(m.triangles, t), i
            assert np.array_equal(par, np.arange(len(t))) and ends.shape == (0, 2)
        else:
            assert len(m.triangles) == 4 * len(t) and len(ends) > 0
    # flags on the far side of the empty meshes only: the numbering behind them holds
    flags[0][:] = False
    assert_same(on_device(ms, flags), RR.refine(ms, flags))


def raw_create(ctx, xy, tri, voff, toff, flag, with_handle=True):
    xy, tri = _hip._f64(xy).reshape(-1, 2), _hip._i32(tri).reshape(-1, 3)
    voff, toff, flag = _hip._i64(voff), _hip._i64(toff), np.ascontiguousarray(flag, dtype=np.uint8)
    n_mesh = len(voff) - 1
    nv, nt = np.zeros(n_mesh, dtype=np.int64), np.zeros(n_mesh, dtype=np.int64)
    h = _hip._P()
    rc = ctx._lib.padne_refine_create(ctx._h, len(xy), _hip._ptr(xy, _hip._PF64), len(tri), _hip._ptr(tri, _hip._PI32), n_mesh,
                                      _hip._ptr(voff, _hip._PI64), _hip._ptr(toff, _hip._PI64),
                                      _hip._ptr(flag, C.POINTER(C.c_uint8)), _hip._ptr(nv, _hip._PI64), _hip._ptr(nt, _hip._PI64),
                                      None, C.byref(h) if with_handle else None)
    return rc, h, ctx._lib.padne_last_error().decode()


def test_the_raw_entry_refuses_what_it_cannot_do(ctx):
    """Argument errors the entry returns; nothing here reaches a kernel with an index it could follow out of bounds."""
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.5, -1.0]])
    tri = np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32)
    flag = np.array([1, 0], dtype=np.uint8)
    lib = ctx._lib

    def refused(args, match, code=_hip.E_INVALID, **kw):
        rc, h, msg = raw_create(ctx, *args, **kw)
        assert rc == code and match in msg, (rc, msg)
        assert not h.value

    refused((pts, tri, [0, 5], [0, 2], flag), "null", with_handle=False)
    refused((pts, tri, [1, 5], [0, 2], flag), "start at 0")
    refused((pts, tri, [0, 5], [1, 2], flag), "start at 0")
    refused((pts, tri, [0, 6, 5], [0, 2, 2], flag), "not monotone")
    refused((pts, tri, [0, 5, 5], [0, 3, 2], flag), "not monotone")
    refused((pts, tri, [0, 4], [0, 2], flag), "offset tables")
    refused((pts, np.array([[0, 1, 2], [1, 77, 2]]), [0, 5], [0, 2], flag), "out of range")
    refused((pts, np.array([[0, 1, 2], [1, -1, 2]]), [0, 5], [0, 2], flag), "out of range")
    refused((pts, np.array([[0, 1, 2], [1, 4, 2]]), [0, 4, 5], [0, 2, 2], flag), "out of range")      # another mesh's vertex
    refused((pts, np.array([[0, 1, 2], [1, 1, 3]]), [0, 5], [0, 2], flag), "twice")
    three = np.array([[0, 1, 2], [1, 0, 4], [0, 1, 3]])                  # three faces on the edge (0, 1)
    refused((pts, three, [0, 5], [0, 3], [0, 0, 0]), "Non-manifold", code=_hip.E_NONMANIFOLD)
    refused((pts, np.array([[0, 1, 2], [0, 1, 3]]), [0, 5], [0, 2], flag), "Non-manifold", code=_hip.E_NONMANIFOLD)
    with pytest.raises(ValueError, match="Non-manifold mesh"):
        solver.refine_meshes([mesh.Mesh(pts, three)], [np.zeros(3, dtype=bool)])
    with pytest.raises(ValueError, match="out of range"):
        solver.refine_meshes([mesh.Mesh(pts, np.array([[0, 1, 9]]))], [np.ones(1, dtype=bool)])
    assert lib.padne_refine_fetch(ctx._h, None, None, None, None, None) == _hip.E_INVALID
    assert lib.padne_refine_destroy(None) == _hip.OK
    # a good call, fetched through the raw entries; the context still works after the refusals
    rc, h, _ = raw_create(ctx, pts, tri, [0, 5], [0, 2], flag)
    assert rc == _hip.OK and h.value
    assert lib.padne_refine_fetch(None, h, None, None, None, None) == _hip.E_INVALID
    assert lib.padne_refine_destroy(h) == _hip.OK
    want = RR.refine([(pts, tri)], [flag.astype(bool)])
    assert_same(on_device([(pts, tri)], [flag.astype(bool)]), want)


# ---- the adaptive loop ------------------------------------------------------------------------------------------------

def mesh_order(layer_of, per_layer):
    out = [None] * len(layer_of)
    for li, items in enumerate(per_layer):
        for item, mi in zip(items, [mi for mi, l in enumerate(layer_of) if l == li]):
            out[mi] = item
    return out


def potentials(layer_of, sol):
    return mesh_order(layer_of, [[zf.values for zf in ls.potentials] for ls in sol.layer_solutions])


def same_solution_and_report(layer_of, a, b):
    (sol_a, rep_a), (sol_b, rep_b) = a, b
    for la, lb in zip(sol_a.layer_solutions, sol_b.layer_solutions):
        assert all(np.array_equal(u.values, v.values) for u, v in zip(la.potentials, lb.potentials))
        assert all(np.array_equal(u.values, v.values) for u, v in zip(la.power_densities, lb.power_densities))
    assert sol_a.solver_info.ground_node_current == sol_b.solver_info.ground_node_current
    assert rep_a.worst == rep_b.worst and rep_a.layers == rep_b.layers and rep_a.tolerance == rep_b.tolerance
    assert rep_a.power_error == rep_b.power_error and rep_a.estimate == rep_b.estimate
    for name in ("recovered", "ratios", "sizes"):
        for la, lb in zip(getattr(rep_a, name), getattr(rep_b, name)):
            assert len(la) == len(lb) and all(np.array_equal(u, v) for u, v in zip(la, lb)), name
    for la, lb in zip(rep_a.indicators, rep_b.indicators):
        assert all(np.array_equal(u.values, v.values) for u, v in zip(la, lb))


@pytest.fixture(scope="module")
def board(ctx):
    system = S.problem_system(BOARD)
    meshes = [mesh.Mesh(xy, tri) for xy, tri, _ in system.meshes]
    _sol, rep = quiet(solver.solve_meshed_error, system.prob, meshes, system.layer_of)
    return system, meshes, rep.estimate


def test_the_adaptive_loop(ctx, board):
    """Three rounds at half the first estimate.  The potentials at the old vertices against one all-flags round's: the two
    differ by what the discretisations differ, which the host restatement's meshes and the host reference's solves of
    the same two boards put at HOST_ADAPTIVE_VS_UNIFORM = 0.0861 of the largest potential (the terminals are point
    singularities: the estimates of the three rounds were 0.305, 0.289, 0.262 on 194, 436, 860 faces, and no xi_f came
    closer to 1 than 9e-4, so the flags do not hang on rounding).  The device's figure must be the host's to REL_TOL scale:
    each of the two potentials within REL_TOL of the largest, twice for the difference and once more for the scale."""
    system, meshes, first = board
    tolerance = first / 2
    timings = {}
    sol, rep, hist = quiet(solver.solve_meshed_adaptive, system.prob, meshes, system.layer_of, tolerance=tolerance, max_rounds=3,
                           timings=timings)
    print(BOARD, "faces", hist.faces, "vertices", hist.vertices, "estimates", hist.estimates, "flagged", hist.flagged,
          "closure edges", hist.closure_edges, "reason", hist.reason, "timings", timings)
    n = len(hist.faces)
    assert 2 <= n <= 3 and hist.reason in ("rounds", "tolerance") and (hist.reason == "rounds") == (hist.estimates[-1] > tolerance)
    assert len(hist.vertices) == len(hist.estimates) == len(hist.flagged) == len(hist.closure_edges) == n
    assert hist.estimates[0] == first and hist.faces[0] == sum(len(m.triangles) for m in meshes)
    assert all(a < b for a, b in zip(hist.faces, hist.faces[1:])) and all(a < b for a, b in zip(hist.vertices, hist.vertices[1:]))
    assert all(f > 0 for f in hist.flagged[:-1]) and all(c >= 0 for c in hist.closure_edges)
    assert hist.faces[-1] == sum(len(m.triangles) for m in hist.meshes) and rep.estimate == hist.estimates[-1]
    assert set(timings) == {"solve", "refine"}
    fresh = quiet(solver.solve_meshed_error, system.prob, hist.meshes, system.layer_of, tolerance=tolerance)
    same_solution_and_report(system.layer_of, (sol, rep), fresh)
    # against one uniform round
    uniform = solver.refine_meshes(meshes, [np.ones(len(m.triangles), dtype=bool) for m in meshes])
    sol_u = quiet(solver.solve_meshed, system.prob, uniform.meshes, system.layer_of)
    old = [len(m.points) for m in meshes]
    for m0, ma, mu in zip(meshes, hist.meshes, uniform.meshes):
        assert np.array_equal(ma.points[:len(m0.points)], m0.points) and np.array_equal(mu.points[:len(m0.points)], m0.points)
    va = np.concatenate([v[:k] for v, k in zip(potentials(system.layer_of, sol), old)])
    vu = np.concatenate([v[:k] for v, k in zip(potentials(system.layer_of, sol_u), old)])
    figure = np.abs(va - vu).max() / np.abs(vu).max()
    print(BOARD, "adaptive against uniform at the old vertices:", figure, "of the largest potential; on the host",
          HOST_ADAPTIVE_VS_UNIFORM, "; apart by", abs(figure - HOST_ADAPTIVE_VS_UNIFORM))
    assert abs(figure - HOST_ADAPTIVE_VS_UNIFORM) <= 4 * REL_TOL


def test_every_reason_to_stop(ctx, board):
    system, meshes, first = board
    n_faces = sum(len(m.triangles) for m in meshes)
    run = lambda **kw: quiet(solver.solve_meshed_adaptive, system.prob, meshes, system.layer_of, **kw)
    sol, rep, hist = run(tolerance=(1 + first) / 2)
    assert hist.reason == "tolerance" and hist.faces == [n_faces] and hist.flagged == [0] and rep.estimate == first
    assert all(a is b for a, b in zip(hist.meshes, meshes))
    _, _, hist = run(tolerance=first / 2, min_size=1e9)
    assert hist.reason == "floor" and hist.faces == [n_faces] and hist.flagged == [0]
    _, rep, hist = run(tolerance=first / 2, max_faces=n_faces + 1)
    assert hist.reason == "faces" and hist.faces == [n_faces] and hist.flagged[0] > 0 and rep.estimate == first
    assert all(a is b for a, b in zip(hist.meshes, meshes))              # the refined meshes were discarded
    _, _, hist = run(tolerance=1e-6, max_rounds=2)
    assert hist.reason == "rounds" and len(hist.faces) == 2 and hist.faces[1] > n_faces
    _, _, hist = run(tolerance=1e-6, max_rounds=1)
    assert hist.reason == "rounds" and hist.faces == [n_faces] and hist.flagged[0] > 0 and hist.closure_edges == [0]


def test_a_linear_potential_flags_nothing_on_a_refined_mesh(ctx):
    """No golden board is one uniform strip between two edge sources, so: the standalone estimate on a refined mesh with a
    linear potential.  eta_f <= 1e-12 |g| sqrt(sigma A_f), the bound of tests/test_error_host.py (measured there 2e-15)."""
    row = next(r for r in R.TABLE if r[0] == "linear_17")
    xy, tri, _x, _grad = R.table_case(row)
    tri = np.asarray(tri, dtype=np.int32)
    fine = solver.refine_meshes([mesh.Mesh(xy, tri)], random_flags([(xy, tri)], 9))
    fine = solver.refine_meshes(fine.meshes, random_flags([(fine.meshes[0].points, fine.meshes[0].triangles)], 10)).meshes[0]
    assert len(fine.triangles) > len(tri)
    x = R._linear(fine.points)
    G, eta, E, P, _top, _face = ctx.error_estimate(fine.points, fine.triangles, [0, len(fine.points)], [0, len(fine.triangles)],
                                                   [1.0], x)
    area = np.abs(RR.signed_areas(fine.points, fine.triangles))
    print("largest eta_f on the refined mesh", eta.max(), "over its scale", (eta / (R.LINEAR_GRADIENT * np.sqrt(area))).max())
    assert (eta <= 1e-12 * R.LINEAR_GRADIENT * np.sqrt(area)).all()
    assert np.abs(G - [3.0, -2.0]).max() <= 1e-12 * R.LINEAR_GRADIENT
    xi, _ = solver.refinement_ratios(eta, solver.face_sizes(fine.points, fine.triangles), float(P[0] + E[0]), len(eta), 1e-6)
    assert not (xi > 1).any()

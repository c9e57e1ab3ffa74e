"""``solve_meshed_error`` on the device: every output against the host restatement (tests/error_ref.py, itself checked by
tests/test_error_host.py) on the Solution's own potentials, the Solution against ``solve_meshed`` and
``solve_meshed_currents``, bitwise repeatability in two face orders, the standalone entry on meshes whose exact solution is
known, a hub vertex, and the plan-level entry's refusals."""
import math
import warnings

import numpy as np
import pytest

import error_ref as R
import helpers as H
import sensitivity_ref as S
from padne_amd import _hip, mesh, solver

pytestmark = pytest.mark.gpu

TOL = 1e-12
REL_TOL = 1e-8
PROBLEMS = H.problem_golden_names()
TOLERANCE = 0.05
TWO_SOLVES = 1e-12          # between the solves of one board in two face orders


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def board_of(system, name, perms=None):
    """(meshes, disconnected meshes by layer) of a golden board; ``perms``: per mesh a permutation of its faces."""
    g = H.load_golden(name)
    disc = [[] for _ in system.prob.layers]
    for q in range(int(g.get("n_disc", 0))):
        disc[int(g[f"disc_layer{q}"])].append(mesh.Mesh(g[f"disc_xy{q}"], g[f"disc_tri{q}"]))
    tris = [np.asarray(tri).reshape(-1, 3) for _, tri, _ in system.meshes]
    if perms is not None:
        tris = [tri[p] for tri, p in zip(tris, perms)]
    return [mesh.Mesh(xy, tri) for (xy, _, _), tri in zip(system.meshes, tris)], disc


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        return fn(*args, **kwargs)


def solve_error(name, tolerance=TOLERANCE, perms=None):
    system = S.problem_system(name)
    meshes, disc = board_of(system, name, perms)
    sol, rep = quiet(solver.solve_meshed_error, system.prob, meshes, system.layer_of, tolerance=tolerance,
                     disconnected_meshes_by_layer=disc)
    return system, meshes, disc, sol, rep


def mesh_order(system, per_layer):
    """Per-layer, per-mesh lists (LayerSolution order) -> a list in mesh order."""
    out = [None] * len(system.layer_of)
    for li, items in enumerate(per_layer):
        for item, mi in zip(items, [mi for mi, l in enumerate(system.layer_of) if l == li]):
            out[mi] = item
    return out


def potentials(system, sol):
    return np.concatenate(mesh_order(system, [[zf.values for zf in ls.potentials] for ls in sol.layer_solutions]))


def layers_of_meshes(system, values, n_layers):
    return np.bincount(np.asarray(system.layer_of), weights=values, minlength=n_layers)


@pytest.mark.parametrize("name", PROBLEMS)
def test_every_output_against_the_host_restatement(ctx, name):
    system, meshes, _disc, sol, rep = solve_error(name)
    n_layers = len(system.prob.layers)
    x = potentials(system, sol)
    xy, tri, face_mesh, sigma = R.flat_of(system)
    want = R.estimate_flat(xy, tri, face_mesh, sigma, x)
    toff = np.concatenate([[0], np.cumsum([len(m.triangles) for m in meshes])])
    # J* = -sigma G per vertex, relative to sigma times the largest |g_f| around the vertex
    J = np.concatenate(mesh_order(system, rep.recovered))
    sig_v = np.concatenate([np.full(len(m.points), s) for m, s in zip(meshes, sigma)])
    assert J.shape == want.G.shape
    excess = np.abs(J + sig_v[:, None] * want.G) - TOL * (sig_v * want.g_around)[:, None]
    print(name, "J*: largest error over its scale", (np.abs(J + sig_v[:, None] * want.G).max(axis=1)
                                                     / np.maximum(sig_v * want.g_around, 1e-300)).max())
    assert (excess <= 0).all()
    # eta per face, relative to sqrt(sigma A_f) times the largest |g| around the face
    eta = np.concatenate([tf.values for tf in mesh_order(system, rep.indicators)])
    scale = want.eta_scale(tri)
    print(name, "eta: largest error over its scale", (np.abs(eta - want.eta) / np.maximum(scale, 1e-300)).max())
    assert eta.shape == want.eta.shape and (np.abs(eta - want.eta) <= TOL * scale).all()
    assert (eta >= 0).all() and eta.max() > 0
    # per-layer sums: all terms are positive, the sum is its own scale
    E_want, P_want = (layers_of_meshes(system, v, n_layers) for v in (want.mesh_error, want.mesh_power))
    assert len(rep.layers) == n_layers
    for (E, P), Ew, Pw in zip(rep.layers, E_want, P_want):
        assert abs(E - Ew) <= TOL * Ew and abs(P - Pw) <= TOL * Pw
    assert abs(rep.power_error - want.power_error) <= TOL * want.power_error
    assert rep.power_error == sum(E for E, _ in rep.layers)
    assert abs(rep.estimate - want.estimate) <= TOL * want.estimate and 0 < rep.estimate < 1
    print(name, "estimate", rep.estimate, "power_error", rep.power_error)
    # the worst face of every layer
    layer_of_face = np.asarray(system.layer_of)[face_mesh]
    for li, got in enumerate(rep.worst):
        faces = np.flatnonzero(layer_of_face == li)
        assert (got is None) == (len(faces) == 0), li
        if got is None:
            continue
        value, mesh_in_layer, face, cx, cy = got
        mi = [m for m, l in enumerate(system.layer_of) if l == li][mesh_in_layer]
        g = int(toff[mi] + face)
        k = int(faces[np.argmax(want.eta[faces])])                      # the restatement's: the lowest face of the maximum
        assert value == eta[g]                                           # the worst face is a face of ``indicators``
        assert abs(value - want.eta[k]) <= TOL * scale[k], li
        # another face than the restatement's only when its eta is within rounding of the maximum
        assert g == k or want.eta[g] >= want.eta[k] - TOL * max(scale[g], scale[k]), li
        assert (cx, cy) == pytest.approx(tuple(meshes[mi].points[meshes[mi].triangles[face]].mean(axis=0)), rel=1e-14)
    # ratios and sizes of definition 6
    assert rep.tolerance == TOLERANCE
    xi_want, size_want = R.ratios_sizes(want, TOLERANCE)
    xi = np.concatenate(mesh_order(system, rep.ratios))
    size = np.concatenate(mesh_order(system, rep.sizes))
    e_bar = TOLERANCE * math.sqrt(want.total_power / want.n_faces)
    assert (np.abs(xi - xi_want) <= TOL * (scale / e_bar + xi_want)).all()
    assert np.array_equal(np.isinf(size), np.isinf(size_want))
    fin = ~np.isinf(size_want)
    # size = h / xi: the relative error of xi is that of eta, TOL scale / eta, and that of e_bar
    assert (np.abs(size[fin] - size_want[fin]) <= size_want[fin] * (TOL * scale[fin] / want.eta[fin] + TOL)).all()
    assert (xi > 1).any()


@pytest.mark.parametrize("name", PROBLEMS)
def test_the_solution_is_solve_meshed_and_the_bits_of_solve_meshed_currents(ctx, name):
    system, meshes, disc, sol, rep = solve_error(name, tolerance=None)
    assert rep.ratios is None and rep.sizes is None and rep.tolerance is None
    ref = quiet(solver.solve_meshed, system.prob, meshes, system.layer_of, disconnected_meshes_by_layer=disc)
    cur, _ = quiet(solver.solve_meshed_currents, system.prob, meshes, system.layer_of, [], disconnected_meshes_by_layer=disc)
    assert sol.problem is system.prob and sol.solver_info.residual_norm < 1e-9
    for la, lb, lc in zip(sol.layer_solutions, ref.layer_solutions, cur.layer_solutions):
        assert len(la.disconnected_meshes) == len(lb.disconnected_meshes)
        for a, b, c in zip(la.potentials, lb.potentials, lc.potentials):
            assert np.abs(a.values - b.values).max() <= REL_TOL * np.abs(b.values).max()
            assert np.array_equal(a.values, c.values)
        for a, b, c in zip(la.power_densities, lb.power_densities, lc.power_densities):
            assert np.abs(a.values - b.values).max() <= REL_TOL * np.abs(b.values).max()
            assert np.array_equal(a.values, c.values)
    assert sol.solver_info.ground_node_current == cur.solver_info.ground_node_current


def same_bits(a, b):
    assert a.worst == b.worst and a.layers == b.layers
    assert a.power_error == b.power_error and a.estimate == b.estimate
    for name in ("recovered", "ratios", "sizes"):
        for la, lb in zip(getattr(a, name), getattr(b, name)):
            assert len(la) == len(lb) and all(np.array_equal(u, v) for u, v in zip(la, lb)), name
    for la, lb in zip(a.indicators, b.indicators):
        assert all(np.array_equal(u.values, v.values) for u, v in zip(la, lb))


@pytest.mark.parametrize("name", ["problem_mixed", "problem_two_planes"])
def test_repeatable_bitwise_in_two_face_orders(ctx, name):
    """Two calls give the same bits in every output, on the board as given and on a copy whose faces were shuffled (each
    compared with itself).  Between the two boards' own solves eta is the permuted eta, on the scale of
    sqrt(sigma A_f) times the largest |g| around the face, and the per-layer (E, P), power_error and the estimate agree
    relative to themselves, all at TWO_SOLVES; every figure is printed before it is asserted.  The estimator alone is then
    compared across the two orders on EQUAL potentials (the given board's, through the standalone entry) at 1e-12."""
    system, meshes, _disc, sol, first = solve_error(name)
    _, _, _, _, second = solve_error(name)
    same_bits(first, second)
    rng = np.random.default_rng(7)
    perms = [rng.permutation(len(m.triangles)) for m in meshes]
    assert any(not np.array_equal(p, np.arange(len(p))) for p in perms)
    _, shuffled_meshes, _, sol_s, shuf_a = solve_error(name, perms=perms)
    _, _, _, _, shuf_b = solve_error(name, perms=perms)
    same_bits(shuf_a, shuf_b)
    x = potentials(system, sol)
    xy, tri, face_mesh, sigma = R.flat_of(system)
    toff = np.concatenate([[0], np.cumsum([len(m.triangles) for m in meshes])])
    perm = np.concatenate([toff[i] + p for i, p in enumerate(perms)])
    want = R.estimate_flat(xy, tri, face_mesh, sigma, x)
    scale = want.eta_scale(tri)
    # the two boards' own solves
    eta_given = np.concatenate([tf.values for tf in mesh_order(system, first.indicators)])
    eta_shuffled = np.concatenate([tf.values for tf in mesh_order(system, shuf_a.indicators)])
    eta_excess = (np.abs(eta_shuffled - eta_given[perm]) / np.maximum(scale[perm], 1e-300)).max()
    sums = [("power_error", first.power_error, shuf_a.power_error), ("estimate", first.estimate, shuf_a.estimate)]
    for li, ((E, P), (Es, Ps)) in enumerate(zip(first.layers, shuf_a.layers)):
        sums += [(f"E of layer {li}", E, Es), (f"P of layer {li}", P, Ps)]
    x_s = potentials(system, sol_s)
    print(name, "two solves: potentials differ by", np.abs(x_s - x).max() / np.abs(x).max(), "relative; eta by", eta_excess,
          "of its scale;", ", ".join(f"{what} by {abs(a - b) / a if a else 0.0:.3e}" for what, a, b in sums))
    assert eta_excess <= TWO_SOLVES
    for what, a, b in sums:
        assert abs(a - b) <= TWO_SOLVES * a, what
    # the estimator alone in the two orders, on the same potentials
    voff = system.offsets
    local = np.concatenate([np.asarray(m.triangles) for m in meshes]).astype(np.int32)
    local_s = np.concatenate([np.asarray(m.triangles) for m in shuffled_meshes]).astype(np.int32)
    G, eta, E, P, top, face = ctx.error_estimate(xy, local, voff, toff, sigma, x)
    Gs, etas, Es, Ps, tops, faces = ctx.error_estimate(xy, local_s, voff, toff, sigma, x)
    print(name, "eta across the two orders: largest difference over its scale",
          (np.abs(etas - eta[perm]) / np.maximum(scale[perm], 1e-300)).max())
    assert (np.abs(etas - eta[perm]) <= TOL * scale[perm]).all()
    assert (np.abs(Gs - G) <= TOL * want.g_around[:, None]).all()
    assert np.allclose(Es, E, rtol=TOL, atol=0) and np.allclose(Ps, P, rtol=TOL, atol=0)
    assert abs(Es.sum() - E.sum()) <= TOL * E.sum()
    assert (np.abs(tops - top) <= TOL * scale[face]).all()


# ---- the standalone entry where the exact solution is known ----------------------------------------------------------

def device_estimate(ctx, xy, tri, x, sigma=1.0):
    one, onet = np.array([0, len(xy)], dtype=np.int64), np.array([0, len(tri)], dtype=np.int64)
    return ctx.error_estimate(xy, np.asarray(tri, dtype=np.int32), one, onet, [sigma], x)


@pytest.fixture(scope="module")
def table(ctx):
    out = {}
    for row in R.TABLE:
        xy, tri, x, grad = R.table_case(row)
        want = R.estimate_flat(xy, tri, np.zeros(len(tri), dtype=np.int64), [1.0], x)
        out[row[0]] = (xy, tri, x, grad, want, device_estimate(ctx, xy, tri, x))
    return out


@pytest.mark.parametrize("name", [row[0] for row in R.TABLE])
def test_standalone_entry_is_the_restatement(table, name):
    _xy, tri, _x, _grad, want, (G, eta, E, P, top, face) = table[name]
    scale = want.eta_scale(tri)
    assert (np.abs(G - want.G) <= TOL * want.g_around[:, None]).all()
    assert (np.abs(eta - want.eta) <= TOL * scale).all()
    assert abs(E[0] - want.mesh_error[0]) <= TOL * want.mesh_error[0] + 1e-300
    assert abs(P[0] - want.mesh_power[0]) <= TOL * want.mesh_power[0]
    k = int(want.mesh_face[0])
    assert top[0] == eta[face[0]] and abs(top[0] - want.mesh_max[0]) <= TOL * scale[k]
    assert face[0] == k or want.eta[face[0]] >= want.eta[k] - TOL * max(scale[face[0]], scale[k])


@pytest.mark.parametrize("name", [row[0] for row in R.TABLE if row[1] != "linear"])
def test_standalone_estimate_is_the_true_error(table, name):
    xy, tri, _x, grad, want, (_G, _eta, E, P, _top, _face) = table[name]
    ratio = math.sqrt(E[0]) / R.true_error(xy, tri, want, grad)
    print(name, len(tri), "estimate / true error", ratio)
    assert 0.9 <= ratio <= 1.1


@pytest.mark.parametrize("family", ["annulus", "grid"])
def test_standalone_estimate_halves_with_h(table, family):
    rows = [row[0] for row in R.TABLE if row[1] == family]
    est = {}
    for n in rows:
        E, P = table[n][5][2][0], table[n][5][3][0]
        _, est[n] = solver.error_estimate_of([E], [P])
    for coarse, fine in zip(rows, rows[1:]):
        print(coarse, "->", fine, est[coarse] / est[fine])
        assert 1.8 <= est[coarse] / est[fine] <= 2.2


def test_standalone_linear_potential_has_no_error(table):
    _xy, _tri, _x, _grad, want, (G, eta, E, P, _top, _face) = table["linear_17"]
    print("largest eta_f", eta.max())
    assert (eta <= 1e-12 * R.LINEAR_GRADIENT * np.sqrt(want.sigma * want.area)).all()
    assert np.abs(G - [3.0, -2.0]).max() <= 1e-12 * R.LINEAR_GRADIENT


def test_the_module_level_wrapper(ctx, table):
    xy, tri, x, _grad, _want, (G, eta, E, P, top, face) = table["grid_17"]
    got = solver.ctx_error_estimate(ctx, xy, np.asarray(tri, dtype=np.int32), 1.0, x)
    assert np.array_equal(got[0], G) and np.array_equal(got[1], eta)
    assert got[2:] == (float(E[0]), float(P[0]), float(top[0]), int(face[0]))


def test_a_hub_of_forty_faces_and_a_mesh_of_one_face(ctx):
    n = 40
    th = np.arange(n) * (2 * np.pi / n)
    rng = np.random.default_rng(2)
    rim = np.stack([np.cos(th), np.sin(th)], axis=1) * rng.uniform(0.8, 1.2, n)[:, None]
    fan_xy = np.concatenate([[[0.05, -0.02]], rim])
    fan_tri = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], dtype=np.int32)
    fan_tri = fan_tri[rng.permutation(n)]                                 # the hub's faces in no geometric order
    one_xy = np.array([[3.0, 0.0], [4.0, 0.1], [3.4, 0.9]])
    one_tri = np.array([[0, 1, 2]], dtype=np.int32)
    xy = np.concatenate([fan_xy, one_xy])
    local = np.concatenate([fan_tri, one_tri])
    voff, toff = np.array([0, n + 1, n + 4], dtype=np.int64), np.array([0, n, n + 1], dtype=np.int64)
    sigma = np.array([1700.0, 30.0])
    x = np.exp(0.8 * xy[:, 0]) * np.cos(1.3 * xy[:, 1]) + rng.normal(0, 0.01, len(xy))
    G, eta, E, P, top, face = ctx.error_estimate(xy, local, voff, toff, sigma, x)
    tri = np.concatenate([fan_tri.astype(np.int64), one_tri + n + 1])
    face_mesh = np.concatenate([np.zeros(n, dtype=np.int64), [1]])
    want = R.estimate_flat(xy, tri, face_mesh, sigma, x)
    scale = want.eta_scale(tri)
    assert (np.abs(G - want.G) <= TOL * want.g_around[:, None]).all() and np.abs(G[0]).max() > 0
    # the hub adds its forty faces in ascending face number, as the restatement does (np.add.at in face order), and both
    # round every operation as written: the same bits.  Another order of the same sum would differ in the last bits
    assert np.array_equal(G, want.G)
    backwards = (want.area[:n, None] * want.g[:n])[::-1].cumsum(axis=0)[-1] / want.area[:n][::-1].cumsum()[-1]
    assert not np.array_equal(backwards, want.G[0])                       # (so the comparison can tell orders apart)
    assert (np.abs(eta - want.eta) <= TOL * scale).all() and (eta[:n] > 0).all()
    # a single face: every corner recovers the face's own gradient (up to the rounding of (A g) / A), so it has no error
    # and all of the power
    assert (np.abs(G[n + 1:] - want.g[n]) <= TOL * np.hypot(*want.g[n])).all()
    assert eta[n] <= TOL * scale[n] and E[1] == eta[n] ** 2
    assert abs(P[1] - want.mesh_power[1]) <= TOL * want.mesh_power[1] and top[1] == eta[n] and face[1] == n
    assert abs(E[0] - want.mesh_error[0]) <= TOL * want.mesh_error[0] and abs(P[0] - want.mesh_power[0]) <= TOL * want.mesh_power[0]
    assert face[0] == want.mesh_face[0] and top[0] == eta[face[0]]
    # a mesh without faces beside them: -1.0 and -1, and its lone vertex recovers nothing
    xy3 = np.concatenate([xy, [[9.0, 9.0]]])
    out = ctx.error_estimate(xy3, local, np.r_[voff, n + 5], np.r_[toff, n + 1], np.r_[sigma, 1.0], np.r_[x, 1.0])
    assert np.array_equal(out[0][:-1], G) and not out[0][-1].any() and np.array_equal(out[1], eta)
    assert out[4][2] == -1.0 and out[5][2] == -1 and out[2][2] == 0.0 and out[3][2] == 0.0
    with pytest.raises(ValueError, match="out of range"):
        ctx.error_estimate(xy, np.where(local == 2, 77, local), voff, toff, sigma, x)
    assert np.array_equal(ctx.error_estimate(xy, local, voff, toff, sigma, x)[1], eta)      # the context still works


# ---- the plan-level entry ---------------------------------------------------------------------------------------------

def test_plan_level_entry_refuses_what_it_cannot_do(ctx):
    system = S.problem_system("problem_mixed")
    meshes, _ = board_of(system, "problem_mixed")
    layer_of = system.layer_of
    board = solver.index_board(system.prob, meshes, layer_of)
    with board.assembled() as (L, _):
        rows, cols, vals = solver.stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], [{}])
        red, kidx, kval = solver.block_plan_inputs(L, rows, cols, vals, 1)
        members, extras = red.probe_members, red.regulator_columns
        plan = _hip.KktPlan(L.dev, L.layout.n_potential, red.elim, red.tied, red.n_free)
        n_tri, n_vert, n_mesh = len(L.tri), len(L.xy), len(meshes)
        opts = dict(rtol=solver.RTOL, abs_residual_target=solver.ABS_RESIDUAL_TARGET)
        with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):
            plan.error_estimate(1, n_tri, n_vert, n_mesh)
        p, _ = plan.solve_block_coo(1, rows, cols, vals, kidx, kval, extras, members, **opts)
        V, _ = solver._finish_block(plan, red, members, p, 1)
        first = plan.error_estimate(1, n_tri, n_vert, n_mesh)
        for bad, match in [((2, n_tri, n_vert, n_mesh), "as many columns"), ((1, n_tri + 1, n_vert, n_mesh), "n_tri, n_vert and n_mesh"),
                           ((1, n_tri, n_vert - 1, n_mesh), "n_tri, n_vert and n_mesh"),
                           ((1, n_tri, n_vert, n_mesh + 1), "n_tri, n_vert and n_mesh")]:
            with pytest.raises(ValueError, match=match):
                plan.error_estimate(*bad)
            again = plan.error_estimate(1, n_tri, n_vert, n_mesh)            # the V and the lists stay: same bits
            assert all(np.array_equal(a, b) for a, b in zip(first, again))
        assert first[0].shape == (n_vert, 2) and first[1].shape == (n_tri,) and all(a.shape == (n_mesh,) for a in first[2:])
        # the plan's arithmetic is the standalone entry's on the same potentials, and the restatement's
        xy, tri, face_mesh, sigma = R.flat_of(system)
        toff = np.concatenate([[0], np.cumsum([len(m.triangles) for m in meshes])])
        local = np.concatenate([np.asarray(m.triangles) for m in meshes]).astype(np.int32)
        alone = ctx.error_estimate(xy, local, system.offsets, toff, sigma, np.ascontiguousarray(V[:n_vert, 0]))
        assert all(np.array_equal(a, b) for a, b in zip(first, alone))
        want = R.estimate_flat(xy, tri, face_mesh, sigma, V[:n_vert, 0])
        assert (np.abs(first[1] - want.eta) <= TOL * want.eta_scale(tri)).all()
        # a solve after the finish takes the block away again
        p, _ = plan.solve_block_coo(1, rows, cols, vals, kidx, kval, extras, members, **opts)
        with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):
            plan.error_estimate(1, n_tri, n_vert, n_mesh)
        solver._finish_block(plan, red, members, p, 1)
        assert all(np.array_equal(a, b) for a, b in zip(first, plan.error_estimate(1, n_tri, n_vert, n_mesh)))
        plan.close()
        # a matrix without a mesh (an uploaded scipy matrix) has nothing to estimate on
        bare = ctx.csr_from_scipy(L.tocsr())
        try:
            plan = _hip.KktPlan(bare, L.layout.n_potential, red.elim, red.tied, red.n_free)
            p, _ = plan.solve_block_coo(1, rows, cols, vals, kidx, kval, extras, members, **opts)
            solver._finish_block(plan, red, members, p, 1)
            with pytest.raises(ValueError, match="does not carry a mesh"):
                plan.error_estimate(1, n_tri, n_vert, n_mesh)
            plan.close()
        finally:
            bare.close()


def test_timings_have_an_error_lap(ctx):
    system = S.problem_system("problem_mixed")
    meshes, disc = board_of(system, "problem_mixed")
    timings = {}
    quiet(solver.solve_meshed_error, system.prob, meshes, system.layer_of, disconnected_meshes_by_layer=disc, timings=timings)
    assert {"indexing", "assembly", "stage1", "stage2", "error", "solutions"} <= set(timings) and timings["error"] > 0

"""``solve_meshed_sensitivities`` on the device: every output against a host restatement (the oracle's M, scipy solves
with M^T, the assembly's cot weights), column 0 against ``solve_meshed`` and the vector power kernel, two identities that
tie all outputs together, finite differences of device solves, and objectives in one call against single calls."""
import warnings

import numpy as np
import pytest

import helpers as H
import sensitivity_ref as S
from padne_amd import _hip, mesh, problem, solver

pytestmark = pytest.mark.gpu

REL_TOL = 1e-8
PROBLEMS = H.problem_golden_names()


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def board_of(system, name):
    g = H.load_golden(name)
    disc = [[] for _ in system.prob.layers]
    for q in range(int(g.get("n_disc", 0))):
        disc[int(g[f"disc_layer{q}"])].append(mesh.Mesh(g[f"disc_xy{q}"], g[f"disc_tri{q}"]))
    return [mesh.Mesh(xy, tri) for xy, tri, _ in system.meshes], disc


def fixture_objectives(flat):
    """Up to five (p, n) pairs: the terminals of the first current source, voltage source, resistor, and the sense and
    output pins of the first regulator."""
    out, seen = [], set()
    for e in flat:
        kind = solver.element_kind(e)
        if kind in seen:
            continue
        seen.add(kind)
        t = e.terminals
        out.append((t[0], t[1]))
        if kind == "VoltageRegulator":
            out.append((e.s_f, e.s_t))
    return [(p, n) for p, n in out if p is not n]


def sensitivities(name, objectives=None):
    system = S.problem_system(name)
    meshes, disc = board_of(system, name)
    objectives = objectives or fixture_objectives(system.flat)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        sol, sens = solver.solve_meshed_sensitivities(system.prob, meshes, system.layer_of, objectives,
                                                      disconnected_meshes_by_layer=disc)
    return system, meshes, objectives, sol, sens


def close(got, want, tol=REL_TOL, scale=0.0):
    """|got - want| <= tol max(|want|, scale) entrywise-max (``scale``: the size of the terms want sums, when it cancels)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    scale = max(np.abs(want).max(initial=0.0), scale, 1e-300)
    return got.shape == want.shape and np.abs(got - want).max(initial=0.0) <= tol * scale


@pytest.mark.parametrize("name", PROBLEMS)
def test_every_output_against_the_host_restatement(ctx, name):
    system, meshes, objectives, sol, sens = sensitivities(name)
    assert len(sens) == len(objectives) >= 2
    M, r = system.assemble()
    x = S.solve(M, r)
    idx = system.nodes.node_to_global_index
    tri, _, _, area = S.faces(system)
    toff = np.concatenate([[0], np.cumsum([len(m.triangles) for m in meshes])])
    for j, ((p, n), s) in enumerate(zip(objectives, sens)):
        assert s.nodes[0] is p and s.nodes[1] is n
        lam = S.adjoint(M, idx[p], idx[n])
        assert abs(s.value - (x[idx[p]] - x[idx[n]])) <= REL_TOL * np.abs(x).max(), j
        sf, mag = S.face_s(system, x, lam), S.face_s_bound(system, x, lam)
        got = np.concatenate([tf.values for forms in s.densities for tf in forms])
        # densities come per layer, per mesh of the layer: put them back in mesh order
        order = [mi for li in range(len(system.prob.layers)) for mi, l in enumerate(system.layer_of) if l == li]
        want = np.concatenate([(sf / area)[toff[mi]:toff[mi + 1]] for mi in order])
        assert close(got, want, scale=(mag / area).max()), j
        want_layers = [sum(sf[toff[mi]:toff[mi + 1]].sum() for mi, l in enumerate(system.layer_of) if l == li)
                       for li in range(len(system.prob.layers))]
        assert close(s.layers, want_layers, scale=mag.sum()), j
        want_el = solver.element_sensitivities(system.rows, x, lam)
        bounds = S.element_bounds(system.rows, x, lam)
        assert list(s.elements) == [e for e, _ in system.pairs]
        for field in ("resistance", "current", "voltage", "gain"):
            keys = [(e, i) for i, (e, _) in enumerate(system.pairs) if field in want_el[i]]
            if keys:
                assert close([s.elements[e][field] for e, _ in keys], [want_el[i][field] for _, i in keys],
                             scale=bounds[field]), (j, field)


@pytest.mark.parametrize("name", PROBLEMS)
def test_column_zero_is_solve_meshed_and_its_power_the_vector_kernel(ctx, name):
    system, meshes, _objectives, sol, _sens = sensitivities(name)
    _, disc = board_of(system, name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        ref = solver.solve_meshed(system.prob, meshes, system.layer_of, disconnected_meshes_by_layer=disc)
    got = np.concatenate([zf.values for ls in sol.layer_solutions for zf in ls.potentials])
    want = np.concatenate([zf.values for ls in ref.layer_solutions for zf in ls.potentials])
    assert close(got, want)
    assert sol.problem is system.prob and sol.solver_info.residual_norm < 1e-9
    assert abs(sol.solver_info.ground_node_current - ref.solver_info.ground_node_current) <= 1e-8 * max(
        abs(ref.solver_info.ground_node_current), 1.0)
    for li, ls in enumerate(sol.layer_solutions):
        assert len(ls.disconnected_meshes) == len(disc[li])
        for zf, tf in zip(ls.potentials, ls.power_densities):
            assert np.array_equal(tf.values, solver.compute_power_density(zf, system.prob.layers[li].conductance).values)


@pytest.mark.parametrize("name", PROBLEMS)
def test_scaling_and_linearity_identities(ctx, name):
    system, _meshes, objectives, _sol, sens = sensitivities(name)
    for j, s in enumerate(sens):
        face = sum(s.layers)
        res = [e.resistance * d["resistance"] for e, d in s.elements.items() if solver.element_kind(e) == "Resistor"]
        cur = [e.current * d["current"] for e, d in s.elements.items() if solver.element_kind(e) == "CurrentSource"]
        src = [e.voltage * d["voltage"] for e, d in s.elements.items()
               if solver.element_kind(e) in ("VoltageSource", "VoltageRegulator")]
        # conductances x alpha == current sources / alpha:  sum s_f - sum R dJ/dR = -sum I dJ/dI
        # (all terms are in volts; an objective across a voltage source has them all 0 up to rounding, relative to J)
        terms = [face, *res, *cur]
        assert abs(face - sum(res) + sum(cur)) <= 1e-9 * max(sum(abs(t) for t in terms), abs(s.value)), j
        # J is linear in the sources:  sum I dJ/dI + sum U dJ/dU = J
        terms = [*cur, *src, s.value]
        assert abs(sum(cur) + sum(src) - s.value) <= 1e-9 * max(sum(abs(t) for t in terms), 1e-300), j


def device_J(g, p_num, n_num):
    """J = V(p) - V(n) of an ordinary device solve of the fixture ``g`` (its Problem rebuilt from the arrays)."""
    prob, ids, _ = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    meshes, layer_of = [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms]
    board = solver.index_board(prob, meshes, layer_of)
    with board.assembled() as (L, r):
        v, _ = solver.solve_system(L, r)
    idx = board.node_indexer.node_to_global_index
    return v[idx[ids[p_num]]] - v[idx[ids[n_num]]]


def test_finite_differences_of_device_solves(ctx):
    name = "problem_two_planes"
    g = H.load_golden(name)
    rows = g["pelements"]
    i_row = int(np.flatnonzero(rows[:, 1] == 1)[0])                  # the current source
    r_row = int(np.flatnonzero(rows[:, 1] == 0)[0])                  # a via resistor
    p_num, n_num = int(rows[i_row, 2]), int(rows[i_row, 3])
    system = S.problem_system(name, g)
    objectives = [(system.ids[p_num], system.ids[n_num])]
    meshes, _ = board_of(system, name)
    _sol, (s,) = solver.solve_meshed_sensitivities(system.prob, meshes, system.layer_of, objectives)
    # system.flat lists the elements network by network, the rows keep the fixture's order
    at = {int(row): k for k, row in enumerate(np.argsort(rows[:, 0], kind="stable"))}
    flat = system.flat
    got = {"resistor": s.elements[flat[at[r_row]]]["resistance"], "current": s.elements[flat[at[i_row]]]["current"],
           "layer": s.layers[0] / float(g["layer_sigma"][0])}

    def fd(key, arr, index):
        theta = float(g[key][index])
        h = 1e-4 * abs(theta)
        out = []
        for sign in (1, -1):
            gg = dict(g)
            gg[key] = np.array(g[key], dtype=np.float64, copy=True)
            gg[key][index] = theta + sign * h
            out.append(device_J(gg, p_num, n_num))
        return (out[0] - out[1]) / (2 * h)
    want = {"resistor": fd("pelements", rows, (r_row, 6)), "current": fd("pelements", rows, (i_row, 6)),
            "layer": fd("layer_sigma", g["layer_sigma"], 0)}
    for key in got:
        assert abs(got[key] - want[key]) <= 1e-5 * abs(want[key]), (key, got[key], want[key])


def test_objectives_together_equal_single_calls_and_repeat_bitwise(ctx):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(H.HERE), "scripts", "load_cases.py")
    spec = importlib.util.spec_from_file_location("load_cases_script", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from padne_amd.structured import StructuredMesher
    prob, loads, source = mod.board(20.0, 5.0)
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=0.2)))
    assert 35000 < sum(len(m.points) for m in meshes) < 45000
    objectives = [(load.f, load.t) for load in loads] + [(source.p, source.n)]
    assert len(objectives) == 9                            # > 4 objectives per chunk, 10 columns > 8 per column chunk
    sol, together = solver.solve_meshed_sensitivities(prob, meshes, layer_of, objectives)
    _, again = solver.solve_meshed_sensitivities(prob, meshes, layer_of, objectives)
    for a, b in zip(together, again):
        assert a.value == b.value and a.layers == b.layers
        assert all(np.array_equal(x.values, y.values) for fa, fb in zip(a.densities, b.densities) for x, y in zip(fa, fb))
        assert all(a.elements[e] == b.elements[e] for e in a.elements)
    for j, obj in enumerate(objectives):
        _, (one,) = solver.solve_meshed_sensitivities(prob, meshes, layer_of, [obj])
        s = together[j]
        assert abs(s.value - one.value) <= 1e-9 * abs(one.value), j
        assert close(s.layers, one.layers, 1e-9), j
        assert close(np.concatenate([tf.values for f in s.densities for tf in f]),
                     np.concatenate([tf.values for f in one.densities for tf in f]), 1e-9), j
        for field in ("resistance", "current", "voltage"):
            es = [e for e in s.elements if field in s.elements[e]]
            assert close([s.elements[e][field] for e in es], [one.elements[e][field] for e in es], 1e-9), (j, field)


def test_plan_level_entry_refuses_what_it_cannot_do(ctx):
    system = S.problem_system("problem_mixed")
    meshes, _ = board_of(system, "problem_mixed")
    board = solver.index_board(system.prob, meshes, system.layer_of)
    with board.assembled() as (L, _):
        terms = solver.woodbury_terms(system.rows)
        n_cols = solver.sensitivity_block_columns(1, len(terms))
        rows, cols, vals = solver.stamp_sensitivity_block(board.filtered_networks, board.node_indexer, L.shape[0], [(3, 40)],
                                                          terms)
        red, kidx, kval = solver.block_plan_inputs(L, rows, cols, vals, n_cols)
        members, extras = red.probe_members, red.regulator_columns
        plan = _hip.KktPlan(L.dev, L.layout.n_potential, red.elim, red.tied, red.n_free)
        n_tri, n_mesh = len(L.tri), len(meshes)
        W = np.zeros((1, n_cols))
        W[0, 1] = 1.0
        with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):
            plan.sensitivity_block(W, n_tri, n_mesh)
        p, _ = plan.solve_block_coo(n_cols, rows, cols, vals, kidx, kval, extras, members, rtol=solver.RTOL,
                                    abs_residual_target=solver.ABS_RESIDUAL_TARGET)
        V, _ = solver._finish_block(plan, red, members, p, n_cols)
        with pytest.raises(ValueError, match="as many columns"):
            plan.sensitivity_block(np.zeros((1, n_cols + 1)), n_tri, n_mesh)
        with pytest.raises(ValueError, match="finite"):
            plan.sensitivity_block(np.full((1, n_cols), np.nan), n_tri, n_mesh)
        power, density, totals = plan.sensitivity_block(W, n_tri, n_mesh)
        assert np.array_equal(power, L.dev.power_density(np.ascontiguousarray(V[:len(L.xy), 0]), n_tri))
        assert density.shape == (1, n_tri) and totals.shape == (1, n_mesh)
        power2, density2, totals2 = plan.sensitivity_block(W, n_tri, n_mesh)      # the V stays: a second call, same bits
        assert np.array_equal(power, power2) and np.array_equal(density, density2) and np.array_equal(totals, totals2)
        plan.close()

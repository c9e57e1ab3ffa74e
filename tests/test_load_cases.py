"""``solve_meshed_load_cases`` on the device: every case of a block against ``solve_meshed`` on its substituted Problem and
against a direct solve of that Problem's system, one case against ``solve_meshed`` bit for bit, the block's power
densities against the single-vector kernel, and the COO entry and the block power density at the plan level."""
import contextlib
import warnings

import numpy as np
import pytest

import helpers as H
from oracle import padne_oracle as O
from padne_amd import _hip, mesh, problem, solver

pytestmark = pytest.mark.gpu

REL_TOL = 1e-8
PROBLEMS = H.problem_golden_names()


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def fixture_board(name):
    """(problem, meshes, mesh_index_to_layer_index, disconnected meshes by layer, elements in stamping order)."""
    g = H.load_golden(name)
    prob, _nodes, flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    disc = [[] for _ in prob.layers]
    for q in range(int(g.get("n_disc", 0))):
        disc[int(g[f"disc_layer{q}"])].append(mesh.Mesh(g[f"disc_xy{q}"], g[f"disc_tri{q}"]))
    return prob, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms], disc, flat


def sources(flat):
    return [e for e in flat if solver.element_kind(e) in solver.CASE_FIELDS]


def block_cases(flat, k, seed):
    """k cases: the Problem itself, then each a random subset of the sources at new values; voltage sources keep their order
    (a common positive factor), so that the ground node stays where it is."""
    rng = np.random.default_rng(seed)
    src = sources(flat)
    cases = [{}]
    while len(cases) < k:
        scale = rng.uniform(0.5, 2.0)
        case = {}
        for e in src:
            if solver.element_kind(e) == "VoltageSource":
                case[e] = scale * e.voltage
            elif rng.random() < 0.6:
                case[e] = rng.uniform(-2.0, 2.0)
        cases.append(case)
    return cases


def potentials(sol):
    return np.concatenate([zf.values for ls in sol.layer_solutions for zf in ls.potentials])


def powers(sol):
    return [tf.values for ls in sol.layer_solutions for tf in ls.power_densities]


def direct_solve(prob, meshes, layer_of):
    """v of a direct solve of ``prob``'s assembled system (L downloaded, r stamped on the host)."""
    board = solver.index_board(prob, meshes, layer_of)
    with board.assembled() as (L, r):
        v, _, _ = O.solve_system(L.tocsr(), r)
    return v, len(board.vindex)


@pytest.mark.parametrize("name", ["problem_mixed", "problem_c1", "problem_many_meshes"])
def test_one_case_is_solve_meshed_on_the_substituted_problem_bit_for_bit(ctx, name):
    prob, meshes, layer_of, disc, flat = fixture_board(name)
    case = {e: 0.5 * e.voltage if solver.element_kind(e) == "VoltageSource" else -1.5 for e in sources(flat)}
    (sol,) = solver.solve_meshed_load_cases(prob, meshes, layer_of, [case], disconnected_meshes_by_layer=disc)
    sub, _ = solver.substitute_load_case(prob, solver.check_load_cases(prob, [case])[0])
    ref = solver.solve_meshed(sub, meshes, layer_of, disconnected_meshes_by_layer=disc)
    assert np.array_equal(potentials(sol), potentials(ref))
    assert all(np.array_equal(a, b) for a, b in zip(powers(sol), powers(ref)))
    assert sol.solver_info.ground_node_current == ref.solver_info.ground_node_current
    assert sol.solver_info.residual_norm == ref.solver_info.residual_norm
    assert sol.solver_info.residual_norms is None
    assert [e for n in sol.problem.networks for e in n.elements] == [e for n in sub.networks for e in n.elements]


@pytest.mark.parametrize("k", [3, 10])
@pytest.mark.parametrize("name", PROBLEMS)
def test_every_case_of_a_block_against_its_own_solve_and_the_direct_solve(ctx, name, k):
    prob, meshes, layer_of, disc, flat = fixture_board(name)
    cases = block_cases(flat, k, seed=k)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        sols = solver.solve_meshed_load_cases(prob, meshes, layer_of, cases, disconnected_meshes_by_layer=disc)
    assert len(sols) == k
    iterations = {s.solver_info.iterations for s in sols}
    assert len(iterations) == 1                                   # the block solve as a whole
    for j, (case, sol) in enumerate(zip(solver.check_load_cases(prob, cases), sols)):
        sub, _ = solver.substitute_load_case(prob, case)
        assert [e for n in sol.problem.networks for e in n.elements] == [e for n in sub.networks for e in n.elements]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", solver.SolverWarning)
            ref = solver.solve_meshed(sub, meshes, layer_of, disconnected_meshes_by_layer=disc)
        v_dir, n_vert = direct_solve(sub, meshes, layer_of)
        got = potentials(sol)
        scale = max(np.abs(v_dir[:n_vert]).max(), 1e-300)
        assert np.abs(got - potentials(ref)).max() <= REL_TOL * scale, j
        assert np.abs(got - v_dir[:n_vert]).max() <= REL_TOL * scale, j
        assert sol.solver_info.residual_norm < 1e-9, j
        assert sol.solver_info.residual_norms is None
        cur_scale = max(np.abs(v_dir[n_vert:]).max(), 1.0)
        assert abs(sol.solver_info.ground_node_current - ref.solver_info.ground_node_current) <= 1e-8 * cur_scale, j
        assert abs(sol.solver_info.ground_node_current - v_dir[-1]) <= 1e-8 * cur_scale, j
        for ls, dl in zip(sol.layer_solutions, disc):
            assert len(ls.disconnected_meshes) == len(dl) and all(a is b for a, b in zip(ls.disconnected_meshes, dl))
        # the block's power densities are those of the single-vector kernel on the case's own potentials, mesh by mesh
        for li, ls in enumerate(sol.layer_solutions):
            for zf, tf in zip(ls.potentials, ls.power_densities):
                want = solver.compute_power_density(zf, prob.layers[li].conductance).values
                assert np.array_equal(tf.values, want), (j, li)


@pytest.mark.parametrize("name", ["problem_mixed", "problem_simple_trace", "problem_c1"])
def test_a_case_with_every_source_at_zero_is_exactly_zero(ctx, name):
    prob, meshes, layer_of, _disc, flat = fixture_board(name)
    zero = {e: 0.0 for e in sources(flat)}
    sols = solver.solve_meshed_load_cases(prob, meshes, layer_of, [{}, zero, {}])
    assert not potentials(sols[1]).any()
    assert not any(p.any() for p in powers(sols[1]))
    assert sols[1].solver_info.ground_node_current == 0.0 and sols[1].solver_info.residual_norm == 0.0
    assert np.abs(potentials(sols[0]) - potentials(sols[2])).max() <= 1e-12 * np.abs(potentials(sols[0])).max()
    assert potentials(sols[0]).any()


def test_ground_current_warning_names_the_case(ctx):
    prob, meshes, layer_of, _disc, flat = fixture_board("problem_mixed")
    cur = next(e for e in flat if solver.element_kind(e) == "CurrentSource")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always", solver.SolverWarning)
        sols = solver.solve_meshed_load_cases(prob, meshes, layer_of, [{}, {cur: 2 * cur.current}])
    ground = [str(w.message) for w in caught if "Ground node current" in str(w.message)]
    for j, sol in enumerate(sols):
        named = [m for m in ground if m.startswith(f"Load case {j}:")]
        assert len(named) == (0 if np.isclose(sol.solver_info.ground_node_current, 0) else 1)


@contextlib.contextmanager
def plan_inputs(name, k, seed):
    """An assembled fixture system with its block of k load cases, closed on the way out: (L, rows, cols, vals, reduction
    pieces)."""
    prob, meshes, layer_of, _disc, flat = fixture_board(name)
    cases = solver.check_load_cases(prob, block_cases(flat, k, seed))
    board = solver.index_board(prob, meshes, layer_of)
    with board.assembled() as (L, _):
        rows, cols, vals = solver.stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], cases)
        red, kidx, kval = solver.block_plan_inputs(L, rows, cols, vals, k)
        yield L, rows, cols, vals, red, kidx, kval, red.probe_members, red.regulator_columns


@pytest.mark.parametrize("name,k", [("problem_mixed", 3), ("problem_two_planes", 10)])
def test_coo_entry_is_the_dense_entry_and_power_density_block_is_the_vector_kernel(ctx, name, k):
    with plan_inputs(name, k, seed=5) as (L, rows, cols, vals, red, kidx, kval, members, extras):
        N, n_tri, n_vert = L.shape[0], len(L.tri), len(L.xy)
        R = np.zeros((N, k))
        R[rows, cols] = vals
        plan = _hip.KktPlan(L.dev, L.layout.n_potential, red.elim, red.tied, red.n_free)
        with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):
            plan.power_density_block(k, n_tri)                                          # nothing finished yet
        opts = dict(rtol=solver.RTOL, abs_residual_target=solver.ABS_RESIDUAL_TARGET)
        p_dense, res_dense = plan.solve_block(R, kidx, kval, extras, members, **opts)
        V_dense, n_dense = solver._finish_block(plan, red, members, p_dense, k)
        pd_dense = plan.power_density_block(k, n_tri)
        p_coo, res_coo = plan.solve_block_coo(k, rows, cols, vals, kidx, kval, extras, members, power_tri=n_tri, **opts)
        with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):
            plan.power_density_block(k, n_tri)                                          # a solve came after the finish
        V_coo, n_coo = solver._finish_block(plan, red, members, p_coo, k)
        with pytest.raises(ValueError, match="as many columns"):
            plan.power_density_block(k + 1, n_tri)
        pd_coo = plan.power_density_block(k, n_tri)
        assert np.array_equal(p_dense, p_coo) and np.array_equal(V_dense, V_coo) and np.array_equal(n_dense, n_coo)
        assert res_dense.iterations == res_coo.iterations
        assert pd_coo.shape == (k, n_tri) and np.array_equal(pd_dense, pd_coo)
        for j in range(k):
            assert np.array_equal(pd_coo[j], L.dev.power_density(np.ascontiguousarray(V_coo[:n_vert, j]), n_tri)), j
        # the triples are checked before the device is touched
        with pytest.raises(ValueError, match="duplicate"):
            plan.solve_block_coo(k, np.r_[rows, rows[:1]], np.r_[cols, cols[:1]], np.r_[vals, vals[:1]], kidx, kval, extras,
                                 members, **opts)
        with pytest.raises(ValueError, match="out of range"):
            plan.solve_block_coo(k, rows, np.where(np.arange(len(cols)) == 0, k, cols), vals, kidx, kval, extras, members, **opts)
        plan.close()
        # a matrix without a mesh (an uploaded scipy matrix) has nothing to compute power densities on
        bare = ctx.csr_from_scipy(L.tocsr())
        try:
            plan = _hip.KktPlan(bare, L.layout.n_potential, red.elim, red.tied, red.n_free)
            p, _ = plan.solve_block_coo(k, rows, cols, vals, kidx, kval, extras, members, **opts)
            V_bare, _ = solver._finish_block(plan, red, members, p, k)
            assert np.abs(V_bare - V_coo).max() <= 1e-8 * np.abs(V_coo).max()
            with pytest.raises(ValueError, match="does not carry a mesh"):
                plan.power_density_block(k, n_tri)
            plan.close()
        finally:
            bare.close()

"""Host half of the load cases (no GPU): the right-hand sides of k cases as COO triples against the stamps of each
substituted Problem, their constraint values against the dense block's, and the refusals that come before the device."""
import math
import types

import numpy as np
import pytest

import helpers as H
from padne_amd import mesh, problem, solver
from padne_amd.reduction import KKTLayout, build_block_reduction

PROBLEMS = H.problem_golden_names()


def fixture_board(name):
    """(problem, meshes, mesh_index_to_layer_index, elements in stamping order) of a problem-level fixture."""
    g = H.load_golden(name)
    prob, _nodes, flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    return prob, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms], flat


def fixture_cases(prob, flat):
    """{} ; a current changed ; the highest source's voltage raised ; a regulator's voltage changed ; every source at once
    (scaled by a common positive factor, so that the ground node stays where it is)."""
    kinds = [solver.element_kind(e) for e in flat]
    cases = [{}]
    cur = [e for e, k in zip(flat, kinds) if k == "CurrentSource"]
    vs = [e for e, k in zip(flat, kinds) if k == "VoltageSource"]
    reg = [e for e, k in zip(flat, kinds) if k == "VoltageRegulator"]
    if cur:
        cases.append({cur[0]: -2.5 * cur[0].current + 0.125})
    if vs:
        top = max(vs, key=lambda e: e.voltage)                   # (the first of the highest, like the ground rule)
        cases.append({top: top.voltage + 0.75})
    if reg:
        cases.append({reg[0]: 0.8 * reg[0].voltage - 0.3})
    cases.append({e: 1.7 * getattr(e, solver.CASE_FIELDS[k]) for e, k in zip(flat, kinds) if k in solver.CASE_FIELDS})
    return cases


def stamped(prob, meshes, layer_of):
    """(stamps, r, node indexer) of ``prob`` the way solve_meshed stamps it."""
    vindex = solver.VertexIndexer.create(meshes)
    nodes = solver.NodeIndexer.create(prob, meshes, layer_of, vindex, list(prob.networks))
    stamps, r = solver.allocate_system(vindex, nodes)
    for network in prob.networks:
        solver.stamp_network_into_system(network, nodes, stamps, r)
    solver.setup_ground_node(solver.find_best_ground_node_index(prob, nodes), stamps, r)
    return stamps, r, nodes, vindex


def densify(rows, cols, vals, n, k):
    R = np.zeros((n, k))
    R[rows, cols] = vals
    return R


@pytest.mark.parametrize("name", PROBLEMS)
def test_triples_are_the_stamps_of_every_substituted_problem(name):
    prob, meshes, layer_of, flat = fixture_board(name)
    cases = solver.check_load_cases(prob, fixture_cases(prob, flat))
    assert len(cases) >= 3
    base_stamps, _, nodes, _ = stamped(prob, meshes, layer_of)
    N = base_stamps.shape[0]
    rows, cols, vals = solver.stamp_load_cases(list(prob.networks), nodes, N, cases)
    assert rows.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float64
    assert len(set(zip(rows.tolist(), cols.tolist()))) == len(rows)            # duplicates summed
    R = densify(rows, cols, vals, N, len(cases))
    for j, case in enumerate(cases):
        sub, _ = solver.substitute_load_case(prob, case)
        stamps, r, _, _ = stamped(sub, meshes, layer_of)
        assert np.array_equal(R[:, j], r), j
        for a, b in zip(stamps.arrays(), base_stamps.arrays()):                   # L does not change with the case
            assert np.array_equal(a, b), j
        assert [(c.index, c.p, c.n) for c in stamps.constraints] == [(c.index, c.p, c.n) for c in base_stamps.constraints]


@pytest.mark.parametrize("name", PROBLEMS)
def test_constraint_values_are_those_of_the_dense_block(name):
    prob, meshes, layer_of, flat = fixture_board(name)
    cases = solver.check_load_cases(prob, fixture_cases(prob, flat))
    stamps, _, nodes, vindex = stamped(prob, meshes, layer_of)
    N, k = stamps.shape[0], len(cases)
    layout = KKTLayout(size=N, n_potential=len(vindex) + nodes.internal_node_count, constraints=list(stamps.constraints))
    rows, cols, vals = solver.stamp_load_cases(list(prob.networks), nodes, N, cases)
    R = densify(rows, cols, vals, N, k)
    values = solver.load_case_constraint_values(layout, rows, cols, vals, k)
    assert sorted(values) == sorted(c.index for c in layout.constraints)
    for cst in layout.constraints:
        assert np.array_equal(values[cst.index], R[cst.index, :])
    red_a, idx_a, val_a = build_block_reduction(layout, values, [])
    red_b, idx_b, val_b = build_block_reduction(layout, {c.index: R[c.index, :] for c in layout.constraints}, [])
    assert np.array_equal(idx_a, idx_b) and np.array_equal(val_a, val_b)
    assert np.array_equal(red_a.elim, red_b.elim) and red_a.tied == red_b.tied


def test_stalled_columns_from_column_norms_is_the_dense_attribution():
    R = np.array([[1.0, 0.0, 3.0], [2.0, 1e-3, 0.0], [0.0, 0.0, 4.0]])
    res = np.array([1e-12, 5e-8, 3e-9])
    assert solver._stalled_columns(res, col_norms=np.sqrt((R * R).sum(axis=0))) == solver._stalled_columns(res, R)


def test_substituted_problem_shares_nodes_and_layers():
    prob, _meshes, _layer_of, flat = fixture_board("problem_mixed")
    cur = next(e for e in flat if solver.element_kind(e) == "CurrentSource")
    reg = next(e for e in flat if solver.element_kind(e) == "VoltageRegulator")
    sub, renamed = solver.substitute_load_case(prob, {cur: 3.0, reg: 1.25})
    assert sub.layers is prob.layers
    assert len(renamed) >= 1 and all(n in sub.networks for n in renamed.values())
    new = [e for n in sub.networks for e in n.elements]
    new_cur = next(e for e in new if solver.element_kind(e) == "CurrentSource")
    new_reg = next(e for e in new if solver.element_kind(e) == "VoltageRegulator")
    assert new_cur.current == 3.0 and new_cur.f is cur.f and new_cur.t is cur.t
    assert new_reg.voltage == 1.25 and new_reg.gain == reg.gain and new_reg.s_f is reg.s_f
    assert solver.substitute_load_case(prob, {})[0] is prob
    assert [e for n in prob.networks for e in n.elements] == flat                # the Problem itself is left alone


def _refused(prob, meshes, layer_of, cases, match, partition=None):
    # the public entry point raises before it indexes, assembles or uploads anything: this runs without a GPU
    with pytest.raises(ValueError, match=match):
        solver.solve_meshed_load_cases(prob, meshes, layer_of, cases, partition=partition)


def test_invalid_cases_are_refused_before_the_device():
    prob, meshes, layer_of, flat = fixture_board("problem_mixed")
    res = next(e for e in flat if solver.element_kind(e) == "Resistor")
    cur = next(e for e in flat if solver.element_kind(e) == "CurrentSource")
    vs = next(e for e in flat if solver.element_kind(e) == "VoltageSource")
    stranger = problem.CurrentSource(f=problem.NodeID(), t=problem.NodeID(), current=1.0)
    _refused(prob, meshes, layer_of, [{cur: 1.0}, {res: 2.0}], "Resistor cannot vary")
    _refused(prob, meshes, layer_of, [{stranger: 1.0}], "not an element of the Problem")
    _refused(prob, meshes, layer_of, [{cur: math.nan}], "finite")
    _refused(prob, meshes, layer_of, [{}, {vs: math.inf}], "finite")
    _refused(prob, meshes, layer_of, [{cur: "a lot"}], "number")
    _refused(prob, meshes, layer_of, [], "no load cases")
    _refused(prob, meshes, layer_of, {cur: 1.0}, "sequence of mappings")
    _refused(prob, meshes, layer_of, [{}, {}], "row-partitioned", partition=types.SimpleNamespace(world=2, rank=0))
    with pytest.raises(ValueError, match="no load cases"):
        solver.solve_load_cases(prob, [], mesher=object())


def test_a_case_that_moves_the_ground_node_is_refused():
    prob, meshes, layer_of, flat = fixture_board("problem_two_planes")
    vs = [e for e in flat if solver.element_kind(e) == "VoltageSource"]
    top = max(vs, key=lambda e: e.voltage)
    other = next(e for e in vs if e.n is not top.n)
    _refused(prob, meshes, layer_of, [{}, {other: top.voltage + 1.0}], "ground node")
    solver.check_load_cases(prob, [{other: top.voltage - 1e-3}])          # below the highest: the ground stays

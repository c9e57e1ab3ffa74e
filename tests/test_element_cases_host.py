"""Host half of the element cases (no GPU; scipy stands in for the device solve): every refusal that comes before the
device, the substituted Problem, the N-1 list, and the Woodbury weights against direct solves of the changed golden
matrices."""
import math
import types
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import element_cases_ref as E
import helpers as H
import sensitivity_ref as S
from padne_amd import _hip, mesh, problem, solver

REL_TOL = 1e-9                     # the weights against direct solves: 2e-11 measured, with margin for other BLAS builds
PROBLEMS = H.problem_golden_names()


def fixture_board(name):
    g = H.load_golden(name)
    prob, _ids, flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    return prob, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms], flat


def resistors(flat):
    return [e for e in flat if solver.element_kind(e) == "Resistor"]


# ---- refusals ------------------------------------------------------------------------------------------------------

def test_invalid_cases_are_refused_before_the_device(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    prob, meshes, layer_of, flat = fixture_board("problem_mixed")
    res = resistors(flat)
    vs = next(e for e in flat if solver.element_kind(e) == "VoltageSource")
    cur = next(e for e in flat if solver.element_kind(e) == "CurrentSource")
    reg = next(e for e in flat if solver.element_kind(e) == "VoltageRegulator")

    def refused(cases, match, **kw):
        with pytest.raises(ValueError, match=match):
            solver.check_element_cases(prob, cases)
        with pytest.raises(ValueError, match=match):
            solver.solve_meshed_element_cases(prob, meshes, layer_of, cases, **kw)

    refused([], "no element cases")
    refused({res[0]: 1.0}, "sequence of mappings")
    refused([[res[0], 1.0]], "not a mapping")
    refused([{}, {res[0]: 0.0}], "element case 1: the resistance of a Resistor must be > 0")
    refused([{res[0]: -2.0}], "must be > 0")
    refused([{res[0]: math.nan}], "must be > 0")
    refused([{res[0]: "big"}], "must be a number")
    refused([{problem.Resistor(a=res[0].a, b=res[0].b, resistance=3.25): 1.0}], "not an element of the Problem")
    refused([{prob.layers[0]: 2.0}], "cannot vary between element cases")            # a layer's conductance
    refused([{(reg, "gain"): 2.0}], "cannot vary between element cases")             # a regulator's gain
    refused([{cur: math.inf}], "must be finite")                                     # sources: check_load_cases' own refusals
    refused([{problem.CurrentSource(f=cur.f, t=cur.t, current=9.0): 1.0}], "not an element of the Problem")
    # check_load_cases itself is as it was
    with pytest.raises(ValueError, match="a Resistor cannot vary between load cases"):
        solver.check_load_cases(prob, [{res[0]: 1.0}])
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_meshed_element_cases(prob, meshes, layer_of, [{res[0]: 1.0}], partition=types.SimpleNamespace(world=2, rank=0))
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_element_cases(prob, [{res[0]: 1.0}], mesher=object(), partition=types.SimpleNamespace(world=2, rank=0))
    with pytest.raises(ValueError, match="no element cases"):
        solver.solve_element_cases(prob, [], mesher=object())
    with pytest.raises(ValueError, match="no objectives"):
        solver.solve_meshed_element_cases(prob, meshes, layer_of, [{res[0]: 1.0}], objectives=[])
    checked = solver.check_element_cases(prob, [{}, {res[1]: math.inf, cur: 2, reg: 1.5}, {res[0]: 7}])
    assert checked == [{}, {cur: 2.0, reg: 1.5, res[1]: math.inf}, {res[0]: 7.0}]
    assert all(type(v) is float for case in checked for v in case.values())


def test_the_ground_rule_of_load_cases_holds_for_element_cases():
    prob, _meshes, _layer_of, flat = fixture_board("problem_two_planes")
    sources = [e for e in flat if solver.element_kind(e) == "VoltageSource"]
    assert len(sources) >= 2
    top = max(sources, key=lambda e: e.voltage)
    other = next(e for e in sources if e.n is not top.n)
    with pytest.raises(ValueError, match="changes which voltage source is the highest"):
        solver.check_element_cases(prob, [{resistors(flat)[0]: 1.0}, {other: top.voltage + 1.0}])


# ---- the substituted Problem and the N-1 list ----------------------------------------------------------------------

def test_substitute_keeps_the_nodes_and_drops_open_resistors():
    prob, _meshes, _layer_of, flat = fixture_board("problem_mixed")
    res = resistors(flat)
    cur = next(e for e in flat if solver.element_kind(e) == "CurrentSource")
    case = solver.check_element_cases(prob, [{res[0]: math.inf, res[1]: 2.5, cur: -3.0}])[0]
    sub = solver.substitute_element_case(prob, case)
    assert solver.substitute_element_case(prob, {}) is prob
    assert sub.layers is prob.layers and len(sub.networks) == len(prob.networks)
    got = [e for n in sub.networks for e in n.elements]
    want = [e for e in flat if e is not res[0]]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g) is type(w) and all(a is b for a, b in zip(g.terminals, w.terminals))        # the same NodeIDs
        if w is res[1]:
            assert g.resistance == 2.5
        elif w is cur:
            assert g.current == -3.0
        else:
            assert g is w
    for new, old in zip(sub.networks, prob.networks):
        assert new.connections is old.connections
        if not any(e in case for e in old.elements):
            assert new is old


@pytest.mark.parametrize("name", ["problem_mixed", "problem_two_planes"])
def test_open_circuit_cases_are_the_resistors_in_stamping_order(name):
    prob, _meshes, _layer_of, flat = fixture_board(name)
    res = resistors(flat)
    cases = solver.open_circuit_cases(prob)
    assert len(cases) == len(res)
    assert all(list(case) == [r] and case[r] == math.inf and next(iter(case)) is r for case, r in zip(cases, res))
    some = solver.open_circuit_cases(prob, [res[2], res[0]])
    assert [next(iter(case)) for case in some] == [res[0], res[2]]
    with pytest.raises(ValueError, match="must be a Resistor"):
        solver.open_circuit_cases(prob, [next(e for e in flat if solver.element_kind(e) != "Resistor")])
    assert solver.check_element_cases(prob, cases) == cases


# ---- the weights against direct solves -----------------------------------------------------------------------------

def system_of(name):
    return S.problem_system(name) if name.startswith("problem_") else S.unknown_system(name)


def resistor_rows_of(system):
    return [i for i, row in enumerate(system.rows) if row[0] == "R"]


def plan_of(system, cases):
    """(n_src, case_source, resistor_rows, case_changes, R dense) of index-level cases, as element_case_columns gives them
    for a Problem: from the restatement's columns."""
    settings, case_source, res, R = E.columns(system, cases)
    rows = [(system.rows[i][1], system.rows[i][2], 1.0 / system.rows[i][3]) for i in res]
    changes = []
    for case in cases:
        ch = []
        for m, i in enumerate(res):
            if i in case:
                g_new = 1.0 / case[i] if math.isfinite(case[i]) else 0.0
                if g_new != rows[m][2]:
                    ch.append((m, rows[m][2], g_new))
        changes.append(ch)
    return len(settings), case_source, rows, changes, R


def solver_weights(system, cases, V=None):
    """solver.element_case_weights on the direct solve of the block: (W csr, sigma, V, R)."""
    n_src, case_source, rows, changes, R = plan_of(system, cases)
    if V is None:
        V = S.solve(system.assemble()[0], R)
    a = np.array([r[0] for r in rows], dtype=np.int64)
    b = np.array([r[1] for r in rows], dtype=np.int64)
    w_ptr, w_col, w_val, sigma = solver.element_case_weights(V[a] - V[b], n_src, case_source, changes)
    # the rows are sparse as the device takes them: the source column first with coefficient exactly 1.0, ascending columns,
    # no zeros
    for c in range(len(cases)):
        lo, hi = w_ptr[c], w_ptr[c + 1]
        assert w_col[lo] == case_source[c] and w_val[lo] == 1.0
        assert np.all(np.diff(w_col[lo:hi]) > 0) and np.all(w_val[lo:hi] != 0.0) and hi - lo <= 1 + len(changes[c])
    return sp.csr_matrix((w_val, w_col, w_ptr), shape=(len(cases), R.shape[1])), sigma, V, R


def n_potential(system):
    return sum(len(m[0]) for m in system.meshes) + system.n_internal


def assert_cases_match_direct(system, cases, sigma_floor, V=None, restamp=False):
    """Every case's x' = V w against the direct solve of its changed system (``restamp``: the changed matrices come from
    E.restamped_system, which test_restamped_matrices_are_the_assembled_ones holds to the oracle's own assembly)."""
    W, sigma, V, _R = solver_weights(system, cases, V)
    n_pot = n_potential(system)
    base = system.assemble() if restamp else None
    worst = 0.0
    for c, case in enumerate(cases):
        want = E.direct_case(system, case, base)
        got = V @ W[c].toarray().ravel()
        for part in (slice(0, n_pot), slice(n_pot, None)):
            err = np.abs(got[part] - want[part]).max() / max(np.abs(want[part]).max(), 1e-300)
            worst = max(worst, err)
            assert err <= REL_TOL, (c, case, err, sigma[c])
        assert sigma[c] >= sigma_floor, (c, sigma[c])
    return worst, sigma


def test_restamped_matrices_are_the_assembled_ones():
    for name in ("problem_mixed", "problem_two_planes"):
        system = system_of(name)
        base = system.assemble()
        r0, r1, r2 = resistor_rows_of(system)[:3]
        for case in ({r0: math.inf}, {r1: 3.5, r2: math.inf}, {r0: 0.25, r1: math.inf, r2: 1e3}):
            Ma, ra = E.changed_system(system, case)
            Mb, rb = E.restamped_system(system, case, base)
            assert np.array_equal(ra, rb)
            assert abs(Ma - Mb).max() <= 4e-16 * abs(Ma).max()


# sigma >= 0.467 (problem_c1) and >= 0.92 (problem_two_planes) were measured; what the device tests need of these boards is
# 0.1, which is what is held here
@pytest.mark.parametrize("name", ["problem_c1", "problem_two_planes", "problem_simple_trace"])
def test_every_single_open_resistor_against_the_direct_solve(name, sigma_floor=0.1):
    system = system_of(name)
    cases = [{i: math.inf} for i in resistor_rows_of(system)]
    assert len(cases) == {"problem_c1": 291, "problem_two_planes": 144, "problem_simple_trace": 2}[name]
    worst, sigma = assert_cases_match_direct(system, cases, sigma_floor, restamp=True)
    print(f"{name}: {len(cases)} single opens, worst {worst:.2e} relative, sigma >= {sigma.min():.3f}")


def corner_cases(system):
    """Every corner x0.8 / x1.25 of the first three resistors (of both, on the one fixture that has only two)."""
    res = resistor_rows_of(system)[:3]
    return [{i: system.rows[i][3] * (1.25 if (corner >> q) & 1 else 0.8) for q, i in enumerate(res)}
            for corner in range(2 ** len(res))]


@pytest.mark.parametrize("name", PROBLEMS)
def test_the_eight_corners_of_the_first_three_resistors_against_the_direct_solve(name):
    system = system_of(name)
    worst, sigma = assert_cases_match_direct(system, corner_cases(system), 0.1)
    print(f"{name}: {2 ** min(3, len(resistor_rows_of(system)))} corners, worst {worst:.2e} relative, sigma >= {sigma.min():.3f}")


def test_a_board_with_a_regulator_with_resistors_and_sources_changed_together():
    system = system_of("problem_mixed")
    M, _ = system.assemble()
    assert (M - M.T).nnz != 0                                                       # the regulator: M is unsymmetric
    r0, r1, r2 = resistor_rows_of(system)[:3]
    cur = next(i for i, row in enumerate(system.rows) if row[0] == "I")
    reg = next(i for i, row in enumerate(system.rows) if row[0] == "REG")
    R = lambda i: system.rows[i][3]  # noqa: E731
    cases = [{}, {r0: 0.5 * R(r0)}, {r1: 10 * R(r1)}, {r2: math.inf}, {r0: math.inf, cur: 2.0},
             {r0: 10 * R(r0), r1: 0.5 * R(r1), r2: 3 * R(r2)}, {cur: 2.0}, {r1: math.inf, r2: 0.5 * R(r2), reg: 1.1, cur: -1.0},
             {r0: R(r0)}]
    W, sigma, V, _ = solver_weights(system, cases)
    assert V.shape[1] == 3 + 3                                  # the settings {}, {cur}, {reg, cur} and three resistors
    assert_cases_match_direct(system, cases, 0.01, V)
    assert sigma[0] == 1.0 and sigma[6] == 1.0 and W[0].nnz == 1 and W[8].nnz == 1           # an unchanged value: no term
    Wref, sigma_ref, _, _ = E.weights(system, cases)
    assert np.abs(W.toarray() - Wref).max() <= 1e-9 * np.abs(Wref).max()
    assert np.abs(sigma - sigma_ref).max() <= 1e-9


def test_the_problem_level_columns_and_stamps_are_the_restatement():
    system = system_of("problem_mixed")
    prob, flat = system.prob, system.flat
    res = resistors(flat)
    cur = next(e for e in flat if solver.element_kind(e) == "CurrentSource")
    at = {id(e): i for i, (e, _) in enumerate(system.pairs)}
    cases = solver.check_element_cases(prob, [{res[2]: math.inf}, {}, {cur: 2.0, res[0]: 3.0}, {res[0]: 3.0, res[2]: 1.0}, {cur: 2.0}])
    index_cases = [{at[id(e)]: v for e, v in case.items()} for case in cases]
    source_cases, case_source, rows, changes = solver.element_case_columns(system.pairs, cases)
    n_src, ref_source, ref_rows, ref_changes, R = plan_of(system, index_cases)
    assert source_cases == [{}, {cur: 2.0}] and len(source_cases) == n_src
    assert case_source == ref_source == [0, 0, 1, 0, 1]
    assert rows == ref_rows and changes == ref_changes
    N = R.shape[0]
    r_, c_, v_ = solver.stamp_element_case_block(list(prob.networks), system.nodes, N, source_cases, rows)
    assert len(set(zip(r_.tolist(), c_.tolist()))) == len(r_)
    dense = np.zeros_like(R)
    dense[r_, c_] = v_
    assert np.array_equal(dense, R)
    # without a resistor the columns are the cases, one each, as stamp_load_cases takes them
    plain = solver.check_element_cases(prob, [{}, {cur: 2.0}, {}])
    assert solver.element_case_columns(system.pairs, plain) == ([{}, {cur: 2.0}, {}], [0, 1, 2], [], [[], [], []])


def test_opening_the_resistor_that_carries_the_load_is_singular():
    system = system_of("problem_mixed")
    r3 = resistor_rows_of(system)[3]
    assert system.rows[r3][3] == 50.0
    with pytest.raises(solver.SingularSystemError, match="element case 1"):
        solver_weights(system, [{}, {r3: math.inf}])
    _, sigma_ref, _, _ = E.weights(system, [{r3: math.inf}])
    assert sigma_ref[0] <= solver.ELEMENT_CASE_SINGULAR_AT
    assert solver.ELEMENT_CASE_SINGULAR_AT == 1e-8 and solver.ELEMENT_CASE_WARN_BELOW == 1e-3
    assert issubclass(solver.SingularSystemError, ValueError)


def test_an_ill_conditioned_case_warns_with_its_amplification():
    system = system_of("regulator")
    big = next(i for i in resistor_rows_of(system) if system.rows[i][3] == 1e5)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always", solver.SolverWarning)
        _W, sigma, _V, _R = solver_weights(system, [{}, {big: math.inf}])
    assert 1e-8 < sigma[1] < 1e-3 and sigma[0] == 1.0
    messages = [str(w.message) for w in caught if issubclass(w.category, solver.SolverWarning)]
    assert len(messages) == 1 and "element case 1" in messages[0] and f"{1.0 / sigma[1]:.1e}" in messages[0]


@pytest.mark.parametrize("name", ["problem_mixed", "two_layer_via", "regulator"])
def test_the_residual_bound_is_above_the_true_residual(name):
    system = system_of(name)
    res = resistor_rows_of(system)[:3]
    cases = [{}] + [{i: math.inf} for i in res[:2]] + corner_cases(system)
    n_src, case_source, rows, changes, R = plan_of(system, cases)
    M, _ = system.assemble()
    rng = np.random.default_rng(11)
    V = S.solve(M, R, refine=0)
    V = V + 1e-9 * np.abs(V).max() * rng.standard_normal(V.shape)          # columns as far off as an iterative solve leaves them
    residual_norms = np.linalg.norm(M @ V - R, axis=0)
    a = np.array([r[0] for r in rows], dtype=np.int64)
    b = np.array([r[1] for r in rows], dtype=np.int64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        w_ptr, w_col, w_val, _sigma = solver.element_case_weights(V[a] - V[b], n_src, case_source, changes)
    bounds = solver.element_case_residual_bounds(w_ptr, w_col, w_val, residual_norms)
    W = sp.csr_matrix((w_val, w_col, w_ptr), shape=(len(cases), R.shape[1]))
    for c, case in enumerate(cases):
        Mc, rc = E.changed_system(system, case)
        true = np.linalg.norm(Mc @ (V @ W[c].toarray().ravel()) - rc)
        assert residual_norms.max() > 0 and true <= bounds[c] * (1 + 1e-6) + 1e-14 * np.abs(rc).max(), (c, true, bounds[c])

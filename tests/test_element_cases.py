"""Element cases on the device: ``KktPlan.combine_block`` against the sequential numpy sum bit for bit, cases without
resistors against ``solve_meshed_load_cases`` bit for bit, and cases that change sources and resistors together against
``solve_meshed`` on their substituted Problem and a direct solve of that Problem's system."""
import contextlib
import math
import types
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H
from oracle import padne_oracle as O
from padne_amd import _hip, mesh, problem, solver

pytestmark = pytest.mark.gpu

COLUMN_TOL = 1e-8                  # what the project holds the block's columns to; a case amplifies it by 1 / sigma_c
SIGMA_FLOOR = 0.1                  # every case of these tests is at least this well conditioned: the bar never exceeds 1e-7


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


def of_kind(flat, *kinds):
    return [e for e in flat if solver.element_kind(e) in kinds]


def potentials(sol):
    return np.concatenate([zf.values for ls in sol.layer_solutions for zf in ls.potentials])


def powers(sol):
    return [tf.values for ls in sol.layer_solutions for tf in ls.power_densities]


# ---- combine_block through the C ABI ---------------------------------------------------------------------------------

@contextlib.contextmanager
def finished_blocks(name):
    """An assembled fixture system and ``finish(k)``: a fresh solve of k load cases of it finished on one plan, returning
    (plan, V (N, k)) (``finished=False``: stage 1 only, (plan, None)).  Yields (L, finish, power_of) with ``power_of(v)`` =
    compute_power_density of a column, mesh by mesh."""
    prob, meshes, layer_of, _disc, flat = fixture_board(name)
    rng = np.random.default_rng(7)
    src = of_kind(flat, "CurrentSource", "VoltageSource", "VoltageRegulator")
    board = solver.index_board(prob, meshes, layer_of)
    with board.assembled() as (L, _):
        holder = {}

        def finish(k, finished=True):
            cases = [{}]
            while len(cases) < k:
                scale = rng.uniform(0.5, 2.0)
                cases.append({e: scale * e.voltage if solver.element_kind(e) == "VoltageSource" else rng.uniform(-2.0, 2.0)
                              for e in src})
            cases = solver.check_load_cases(prob, cases)
            rows, cols, vals = solver.stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], cases)
            red, kidx, kval = solver.block_plan_inputs(L, rows, cols, vals, k)
            if "plan" not in holder:
                holder["plan"] = _hip.KktPlan(L.dev, L.layout.n_potential, red.elim, red.tied, red.n_free)
            p, _res = holder["plan"].solve_block_coo(k, rows, cols, vals, kidx, kval, red.regulator_columns, red.probe_members,
                                                     rtol=solver.RTOL, abs_residual_target=solver.ABS_RESIDUAL_TARGET,
                                                     power_tri=len(L.tri))
            if not finished:
                return holder["plan"], None
            V, _norms = solver._finish_block(holder["plan"], red, red.probe_members, p, k)
            return holder["plan"], np.array(V)

        def power_of(v):
            out = []
            for mesh_i, msh in enumerate(board.meshes):
                zf = mesh.ZeroForm(msh)
                zf.values = np.ascontiguousarray(v[board.vindex.offsets[mesh_i]:board.vindex.offsets[mesh_i] + len(msh.points)])
                out.append(solver.compute_power_density(zf, prob.layers[layer_of[mesh_i]].conductance).values)
            return np.concatenate(out)
        try:
            yield L, finish, power_of
        finally:
            if "plan" in holder:
                holder["plan"].close()


def sequential_sum(V, w_ptr, w_col, w_val):
    """V' by its definition: per row of the weights the first product starts the sum, each further one is rounded, then added."""
    out = np.zeros((V.shape[0], len(w_ptr) - 1))
    for c in range(len(w_ptr) - 1):
        lo, hi = int(w_ptr[c]), int(w_ptr[c + 1])
        if lo < hi:
            acc = w_val[lo] * V[:, w_col[lo]]
            for e in range(lo + 1, hi):
                acc = acc + w_val[e] * V[:, w_col[e]]
            out[:, c] = acc
    return out


def random_weights(rng, n_cols, n_out, dense=False):
    """CSR rows of 0 .. n_cols entries with strictly ascending columns; row 0 copies a column (one entry, 1.0), the last row
    names every column, and (from three rows on) row 1 is empty.  ``dense``: every row names every column."""
    w_ptr, w_col, w_val = [0], [], []
    for c in range(n_out):
        if dense or c == n_out - 1:
            cols = np.arange(n_cols)
        elif c == 0:
            cols = np.array([int(rng.integers(n_cols))])
        elif c == 1 and n_out >= 3:
            cols = np.array([], dtype=np.int64)
        else:
            cols = np.sort(rng.choice(n_cols, int(rng.integers(1, min(n_cols, 5) + 1)), replace=False))
        vals = rng.uniform(-2.0, 2.0, len(cols))
        if c == 0 and not dense:
            vals[:] = 1.0
        elif len(vals) and rng.random() < 0.5:
            vals[0] = 1.0                                           # a case's row: its source column at exactly 1.0
        w_col.extend(int(x) for x in cols)
        w_val.extend(float(x) for x in vals)
        w_ptr.append(len(w_col))
    return np.array(w_ptr, dtype=np.int64), np.array(w_col, dtype=np.int32), np.array(w_val, dtype=np.float64)


# n_cols = 9: 227 rows of V to a tile, so problem_simple_trace (N = 610) takes three workgroups with a short last one and
# problem_mixed (N = 131) one short one; n_cols = 1: 2048 rows to a tile.  300 dense rows of 9 are 2700 weights, more than
# are staged next to the rows: they are read from memory instead.
SHAPES = [(1, 1, False), (1, 3, False), (9, 1, False), (9, 2, False), (9, 63, False), (9, 64, False), (9, 65, False),
          (9, 130, False), (9, 300, True)]


@pytest.mark.parametrize("name,N", [("problem_mixed", 131), ("problem_simple_trace", 610)])
def test_combine_block_is_the_sequential_sum_bit_for_bit(ctx, name, N):
    rng = np.random.default_rng(5)
    with finished_blocks(name) as (L, finish, power_of):
        assert L.shape[0] == N
        n_tri = len(L.tri)
        for n_cols, n_out, dense in SHAPES:
            plan, V = finish(n_cols)
            w_ptr, w_col, w_val = random_weights(rng, n_cols, n_out, dense)
            want = sequential_sum(V, w_ptr, w_col, w_val)
            got = plan.combine_block(n_cols, w_ptr, w_col, w_val)
            assert got.shape == (N, n_out) and np.array_equal(got, want), (n_cols, n_out)
            if w_ptr[1] == 1:
                assert w_val[0] == 1.0 and np.array_equal(got[:, 0], V[:, w_col[0]])                         # one entry, 1.0: the column's bits
            # V' is the block the plan holds now: n_out columns, and the face kernels run on it
            with pytest.raises(ValueError, match="as many columns"):
                plan.power_density_block(n_cols if n_cols != n_out else n_out + 1, n_tri)
            pd = plan.power_density_block(n_out, n_tri)
            for j in sorted({0, n_out // 2, n_out - 1}):
                assert np.array_equal(pd[j], power_of(got[:, j])), (n_cols, n_out, j)
            # a second call combines V': a selection of its columns, then the same again -- the same bits both times
            pick = np.sort(rng.choice(n_out, min(n_out, 3), replace=False)).astype(np.int32)
            sel = (np.arange(len(pick) + 1, dtype=np.int64), pick, np.ones(len(pick)))
            again = plan.combine_block(n_out, *sel)
            assert np.array_equal(again, got[:, pick])
            assert plan.combine_block(len(pick), np.arange(len(pick) + 1), np.arange(len(pick)), np.ones(len(pick)),
                                      download=False) is None
            assert np.array_equal(plan.power_density_block(len(pick), n_tri), pd[pick])


def test_two_calls_give_the_same_bits(ctx):
    rng = np.random.default_rng(9)
    w = random_weights(rng, 9, 65)
    with finished_blocks("problem_simple_trace") as (_L, finish, _power_of):
        plan, V = finish(9)
        first = plan.combine_block(9, *w)
        plan2, V2 = finish(9)                                     # the same plan, a fresh finish of a block of its own
        second = plan2.combine_block(9, *w)
        assert np.array_equal(second, sequential_sum(V2, *w)) and np.array_equal(first, sequential_sum(V, *w))
        ident = (np.arange(66, dtype=np.int64), np.arange(65, dtype=np.int32), np.ones(65))
        assert np.array_equal(plan2.combine_block(65, *ident), second)
        assert np.array_equal(plan2.combine_block(65, *ident), second)


def test_combine_block_refuses_invalid_weights(ctx):
    with finished_blocks("problem_mixed") as (_L, finish, _power_of):
        plan, V = finish(3)
        good = (np.array([0, 2, 3]), np.array([0, 2, 1]), np.array([1.0, -0.5, 2.0]))

        def refused(match, ptr, col, val, n_cols=3):
            with pytest.raises(ValueError, match=match):
                plan.combine_block(n_cols, ptr, col, val)

        refused("between 1 and 4096", [0], [], [])
        refused("between 1 and 4096", np.zeros(4098, dtype=np.int64), [], [])
        refused("strictly ascending", [0, 2], [1, 1], [1.0, 1.0])
        refused("strictly ascending", [0, 2], [2, 0], [1.0, 1.0])
        refused("out of range", [0, 1], [3], [1.0])
        refused("out of range", [0, 1], [-1], [1.0])
        refused("finite", [0, 2], [0, 1], [1.0, math.nan])
        refused("finite", [0, 2], [0, 1], [math.inf, 1.0])
        refused("row pointer", [1, 2], [0, 1], [1.0, 1.0])
        refused("row pointer", [0, 2, 1, 3], [0, 1, 2], [1.0, 1.0, 1.0])
        refused("n_out \\+ 1 entries", [0, 2], [0], [1.0])
        refused("as many columns", *good, n_cols=4)
        # nothing above touched the block: it combines as if none of it had been tried
        assert np.array_equal(plan.combine_block(3, *good), sequential_sum(V, *good))
        finish(3, finished=False)
        with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):
            plan.combine_block(3, *good)                                                # a solve came after the finish


# ---- cases without resistors are load cases --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["problem_mixed", "problem_two_planes"])
def test_cases_without_resistors_have_the_bits_of_load_cases(ctx, name):
    prob, meshes, layer_of, disc, flat = fixture_board(name)
    src = of_kind(flat, "CurrentSource", "VoltageSource", "VoltageRegulator")
    case = {e: 0.5 * e.voltage if solver.element_kind(e) == "VoltageSource" else -1.5 for e in src}
    vs = of_kind(flat, "VoltageSource")[0]
    for cases in ([{}], [{}, {}], [{}, case, {}, case]):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", solver.SolverWarning)
            want = solver.solve_meshed_load_cases(prob, meshes, layer_of, cases, disconnected_meshes_by_layer=disc)
            timings = {}
            got, report = solver.solve_meshed_element_cases(prob, meshes, layer_of, cases, disconnected_meshes_by_layer=disc,
                                                            timings=timings)
            # with objectives the block is built here: the same columns, copied by combine_block
            got_obj, report_obj = solver.solve_meshed_element_cases(prob, meshes, layer_of, cases, objectives=[(vs.p, vs.n)],
                                                                    disconnected_meshes_by_layer=disc)
        assert timings["combine_calls"] == 0
        assert report.columns == len(cases) and report.drops is None and np.array_equal(report.conditioning, np.ones(len(cases)))
        assert np.array_equal(report_obj.conditioning, np.ones(len(cases)))
        for sols in (got, got_obj) if len(cases) > 1 else (got,):
            for a, b in zip(sols, want, strict=True):
                assert np.array_equal(potentials(a), potentials(b))
                assert all(np.array_equal(x, y) for x, y in zip(powers(a), powers(b), strict=True))
                assert a.solver_info.ground_node_current == b.solver_info.ground_node_current
                assert a.solver_info.residual_norm == b.solver_info.residual_norm
        for c, one in enumerate(cases):
            volts = one.get(vs, vs.voltage)
            assert abs(report_obj.drops[c, 0] - volts) <= COLUMN_TOL * max(abs(volts), 1.0)


# ---- sources and resistors together, against the direct solve ------------------------------------------------------

def direct_solve(prob, meshes, layer_of):
    """(v of a direct solve of ``prob``'s assembled system, vertices, node -> unknown)."""
    board = solver.index_board(prob, meshes, layer_of)
    with board.assembled() as (L, r):
        v, _, _ = O.solve_system(L.tocsr(), r)
    return v, len(board.vindex), board.node_indexer.node_to_global_index


def corners(res, which, scale=(0.8, 1.25)):
    return [{r: r.resistance * scale[(corner >> q) & 1] for q, r in enumerate(res[:3])} for corner in which]


def mixed_cases(name, flat):
    res = of_kind(flat, "Resistor")
    vs = of_kind(flat, "VoltageSource")
    cur = of_kind(flat, "CurrentSource")
    half = {e: 0.5 * e.voltage for e in vs}                       # a common factor: the ground node stays where it is
    load = {e: -1.5 * e.current for e in cur}
    if name == "problem_c1":
        # 16 vias open one at a time -- via 100, the worst conditioned, among them -- and four corners
        vias = list(range(0, 291, 20)) + [290]
        assert len(vias) == 16 and 100 in vias
        cases = [{res[i]: math.inf, **(half if q % 4 == 1 else {})} for q, i in enumerate(vias)]
        return cases + [{**c, **(half if q % 2 else {})} for q, c in enumerate(corners(res, (0, 3, 5, 7)))]
    if name == "problem_two_planes":
        cases = [{res[i]: math.inf, **(load if q % 2 else {})} for q, i in enumerate((0, 71, 143))]
        return cases + [{}, {**corners(res, (6,))[0], **half, **load}]
    if name == "problem_many_meshes":
        # corners only: 13 of its 292 single opens have sigma < 0.1
        return [{**c, **(load if q == 1 else {}), **(half if q == 2 else {})} for q, c in enumerate(corners(res, (0, 2, 5, 7)))]
    assert name == "problem_mixed"
    reg = of_kind(flat, "VoltageRegulator")[0]
    r0, r1, r2 = res[:3]
    return [{}, {r0: 0.5 * r0.resistance}, {r1: 10 * r1.resistance, **load}, {r2: math.inf},
            {r0: math.inf, **load}, {r0: 10 * r0.resistance, r1: 0.5 * r1.resistance, r2: 3 * r2.resistance},
            {r1: math.inf, r2: 0.5 * r2.resistance, reg: 1.1 * reg.voltage, **load}, load]


@pytest.mark.parametrize("name", ["problem_mixed", "problem_c1", "problem_two_planes", "problem_many_meshes"])
def test_every_case_against_its_own_solve_and_the_direct_solve(ctx, name):
    prob, meshes, layer_of, disc, flat = fixture_board(name)
    cases = mixed_cases(name, flat)
    res = of_kind(flat, "Resistor")
    objectives = [(res[0].a, res[0].b), (res[2].b, res[2].a)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        sols, report = solver.solve_meshed_element_cases(prob, meshes, layer_of, cases, objectives=objectives,
                                                         disconnected_meshes_by_layer=disc)
    checked = solver.check_element_cases(prob, cases)
    assert len(sols) == len(cases) and report.conditioning.shape == (len(cases),) and report.drops.shape == (len(cases), 2)
    n_settings = len({frozenset((id(e), v) for e, v in c.items() if solver.element_kind(e) != "Resistor") for c in checked})
    n_changed = len({id(e) for c in checked for e in c if solver.element_kind(e) == "Resistor"})
    assert report.columns == n_settings + n_changed
    assert len({s.solver_info.iterations for s in sols}) == 1                        # the block solve as a whole
    print(f"{name}: {len(cases)} cases from {report.columns} columns, sigma >= {report.conditioning.min():.3f}")
    for c, (case, sol) in enumerate(zip(checked, sols)):
        sigma = report.conditioning[c]
        assert sigma >= SIGMA_FLOOR, (c, sigma)
        assert sigma == 1.0 or any(solver.element_kind(e) == "Resistor" for e in case)
        bar = COLUMN_TOL / sigma
        sub = solver.substitute_element_case(prob, case)
        assert [e for n in sol.problem.networks for e in n.elements] == [e for n in sub.networks for e in n.elements]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", solver.SolverWarning)
            ref = solver.solve_meshed(sub, meshes, layer_of, disconnected_meshes_by_layer=disc)
        v_dir, n_vert, idx = direct_solve(sub, meshes, layer_of)
        got = potentials(sol)
        scale = max(np.abs(v_dir[:n_vert]).max(), 1e-300)
        err_ref, err_dir = np.abs(got - potentials(ref)).max() / scale, np.abs(got - v_dir[:n_vert]).max() / scale
        cur_scale = max(np.abs(v_dir[n_vert:]).max(), 1.0)
        err_gnd = abs(sol.solver_info.ground_node_current - v_dir[-1]) / cur_scale
        print(f"  case {c}: sigma {sigma:.3f}  vs solve_meshed {err_ref:.1e}  vs direct {err_dir:.1e}  ground {err_gnd:.1e}")
        assert err_ref <= bar and err_dir <= bar, (c, err_ref, err_dir, bar)
        assert err_gnd <= bar, (c, err_gnd, bar)
        for j, (p, n) in enumerate(objectives):
            if p in idx and n in idx:                                 # (a node that only the open resistor touched is gone)
                assert abs(report.drops[c, j] - (v_dir[idx[p]] - v_dir[idx[n]])) <= bar * scale, (c, j)
        for ls, dl in zip(sol.layer_solutions, disc):
            assert len(ls.disconnected_meshes) == len(dl) and all(a is b for a, b in zip(ls.disconnected_meshes, dl))
        # the power densities are those of the single-vector kernel on the case's own potentials, mesh by mesh
        for li, ls in enumerate(sol.layer_solutions):
            for zf, tf in zip(ls.potentials, ls.power_densities):
                assert np.array_equal(tf.values, solver.compute_power_density(zf, prob.layers[li].conductance).values), (c, li)


@pytest.mark.parametrize("rtol", [None, 1e-6])
@pytest.mark.parametrize("name", ["problem_mixed", "problem_two_planes"])
def test_residual_norm_bounds_the_residual_of_the_changed_system(ctx, monkeypatch, name, rtol):
    """The pieces of solve_meshed_element_cases one by one, to have x'_c whole: its residual against the changed system --
    the Problem's own matrix with the changed resistors' stamps replaced, the case's own source column -- is below the
    bound the Solutions report.

    The residual is formed here in long double, so the check adds no rounding of its own.  Two roundings remain that no
    code can avoid, and the comparison allows for them by their own bound, 64 u (|| |M'| sum_m |w_cm| |V_m| || + ||r||),
    u = 2^-53 (64: the entries of a row of M', those of a row of w, and the sums of the norm): the device evaluates every
    ||M V_m - R_m|| in doubles, and V' is rounded to doubles.  A converged block sits AT that floor -- measured on
    problem_mixed: bound 1.279e-11, residual of the unrounded combination 1.185e-11, of the doubles 1.329e-11; on
    problem_two_planes 9.86e-11, 7.80e-11 and 1.278e-10 -- so there the allowance (1.2e-9 and 2.2e-8) decides; with the
    block solved to 1e-6 only, the residuals (1.4e-6 and 2.5e-2) are three and six orders above it and the bound is held on
    its own."""
    if rtol is not None:
        monkeypatch.setattr(solver, "RTOL", rtol)
        monkeypatch.setattr(solver, "ABS_RESIDUAL_TARGET", 0.0)
    prob, meshes, layer_of, disc, flat = fixture_board(name)
    cases = solver.check_element_cases(prob, mixed_cases(name, flat))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        sols, report = solver.solve_meshed_element_cases(prob, meshes, layer_of, cases, disconnected_meshes_by_layer=disc)
    board = solver.index_board(prob, meshes, layer_of, None, disc)
    pairs = solver.global_elements(board.filtered_networks, board.node_indexer)
    source_cases, case_source, rows_r, changes = solver.element_case_columns(pairs, cases)
    n_src, n_cols = len(source_cases), len(source_cases) + len(rows_r)
    assert n_cols == report.columns
    with board.assembled() as (L, _):
        N = L.shape[0]
        M = L.tocsr()
        rows, cols, vals = solver.stamp_element_case_block(board.filtered_networks, board.node_indexer, N, source_cases, rows_r)
        plan, V, residual_norms, _res, _n_tri, _ = solver._solve_block_on_device(L, rows, cols, vals, n_cols, len(cases),
                                                                                solver._Laps(None))
        a, b = np.array([r[0] for r in rows_r]), np.array([r[1] for r in rows_r])
        w = solver.element_case_weights(V[a] - V[b], n_src, case_source, changes)
        Vc = plan.combine_block(n_cols, *w[:3])
    assert np.array_equal(w[3], report.conditioning)
    bounds = solver.element_case_residual_bounds(*w[:3], residual_norms)
    R = np.zeros((N, n_cols))
    R[rows, cols] = vals
    for c, sol in enumerate(sols):
        assert sol.solver_info.residual_norm == bounds[c]
        assert np.array_equal(potentials(sol), Vc[:len(board.vindex), c]) and sol.solver_info.ground_node_current == Vc[-1, c]
        ii, jj, xx = [], [], []
        for m, g, g_new in changes[c]:
            ra, rb = rows_r[m][:2]
            ii += [ra, ra, rb, rb]
            jj += [ra, rb, rb, ra]
            xx += [g - g_new, g_new - g, g - g_new, g_new - g]              # the stamp is -g d d^T
        Mc = (M + sp.coo_matrix((xx, (ii, jj)), shape=(N, N))).tocoo()
        x = Vc[:, c]
        r_c = R[:, case_source[c]]
        true = extended_residual_norm(Mc, x, r_c)
        exact = extended_residual_norm(Mc, combine_extended(V, c, *w[:3]), r_c)            # V' before it is rounded to doubles
        lo, hi = int(w[0][c]), int(w[0][c + 1])
        size = np.abs(V[:, w[1][lo:hi]]) @ np.abs(w[2][lo:hi])
        allowance = 64 * 2.0 ** -53 * (np.linalg.norm(abs(Mc).tocsr() @ size) + np.linalg.norm(r_c))
        print(f"{name} rtol {rtol} case {c}: residual {true:.3e} (of the unrounded combination {exact:.3e})  "
              f"bound {bounds[c]:.3e}  allowance {allowance:.1e}")
        assert exact <= bounds[c] + allowance and true <= bounds[c] + allowance, (c, true, exact, bounds[c], allowance)
        if rtol is not None:
            assert bounds[c] >= 100 * allowance, (c, bounds[c], allowance)              # here the bound is held on its own


def extended_residual_norm(M_coo, x, r):
    """||M x - r|| with the products and sums in long double: the rounding of the check itself is far below the residuals of
    a converged solve, which sit at the rounding floor of doubles."""
    res = -np.asarray(r, dtype=np.longdouble)
    np.add.at(res, M_coo.row, M_coo.data.astype(np.longdouble) * np.asarray(x, dtype=np.longdouble)[M_coo.col])
    return float(np.sqrt(np.sum(res * res)))


def combine_extended(V, c, w_ptr, w_col, w_val):
    lo, hi = int(w_ptr[c]), int(w_ptr[c + 1])
    return (V[:, w_col[lo:hi]].astype(np.longdouble) * w_val[lo:hi].astype(np.longdouble)).sum(axis=1)


# ---- fields=False, the singular case, the partition -----------------------------------------------------------------

def test_without_fields_only_the_report_comes_back(ctx):
    prob, meshes, layer_of, disc, flat = fixture_board("problem_two_planes")
    res = of_kind(flat, "Resistor")
    cases = solver.open_circuit_cases(prob, res[::12]) + [{}]
    objectives = [(res[0].a, res[0].b), (res[5].a, res[5].b)]
    t_with, t_without = {}, {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        sols, full = solver.solve_meshed_element_cases(prob, meshes, layer_of, cases, objectives=objectives, timings=t_with,
                                                       disconnected_meshes_by_layer=disc)
        none, lean = solver.solve_meshed_element_cases(prob, meshes, layer_of, cases, objectives=objectives, fields=False,
                                                       timings=t_without, disconnected_meshes_by_layer=disc)
    assert none is None and len(sols) == len(cases) == 13
    assert t_with["combine_calls"] == 1 and "combine" in t_with
    assert t_without["combine_calls"] == 0 and "combine" not in t_without and "power_density" not in t_without
    assert np.array_equal(full.drops, lean.drops) and np.array_equal(full.conditioning, lean.conditioning)
    assert full.columns == lean.columns == 1 + 12 and full.conditioning[-1] == 1.0
    # an open resistor carries nothing: the whole drop of case 0 is across it, no current through it
    assert full.drops.shape == (13, 2) and np.isfinite(full.drops).all()


def test_a_singular_case_is_named(ctx):
    prob, meshes, layer_of, _disc, flat = fixture_board("problem_mixed")
    r3 = of_kind(flat, "Resistor")[3]
    assert r3.resistance == 50.0
    with pytest.raises(solver.SingularSystemError, match="element case 0"):
        solver.solve_meshed_element_cases(prob, meshes, layer_of, [{r3: math.inf}, {}])
    with pytest.raises(solver.SingularSystemError, match="element case 1"):
        solver.solve_meshed_element_cases(prob, meshes, layer_of, [{}, {r3: math.inf}], fields=False)


def test_a_partition_over_several_gpus_is_refused(ctx):
    prob, meshes, layer_of, _disc, flat = fixture_board("problem_mixed")
    r0 = of_kind(flat, "Resistor")[0]
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_meshed_element_cases(prob, meshes, layer_of, [{r0: 1.0}], partition=types.SimpleNamespace(world=2, rank=0))
    sols, report = solver.solve_meshed_element_cases(prob, meshes, layer_of, [{r0: 1.0}],
                                                     partition=types.SimpleNamespace(world=1, rank=0))
    assert len(sols) == 1 and report.columns == 2

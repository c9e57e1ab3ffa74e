"""``solve_meshed_load_case_currents`` on the device: every case's report against the host restatement
(tests/currents_ref.py) on that case's own potentials, column 0 against the one-column kernels bit for bit, the envelope
against ``envelope_of`` of the per-case results, the envelope-only call, tile and chunk edges, parity with separate
solves, bitwise repeatability, and the plan-level entry's refusals."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import currents_ref as C
import helpers as H
import sensitivity_ref as S
from padne_amd import _hip, mesh, problem, solver, synthetic
from test_currents import REL_TOL, TOL, board_of, mesh_order, random_cuts
from test_load_cases import block_cases

pytestmark = pytest.mark.gpu

PROBLEMS = H.problem_golden_names()


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        return fn(*args, **kwargs)


_RUNS: dict = {}


def run(name, k, fields=True):
    """(system, meshes, disconnected meshes, cuts, checked cases, solutions, reports, envelope) of golden ``name`` with the k
    cases of ``block_cases`` and the random cuts of test_currents.py, solved once per module."""
    key = (name, k, fields)
    if key not in _RUNS:
        system = S.problem_system(name)
        meshes, disc = board_of(system, name)
        cuts = random_cuts(system)
        cases = block_cases(system.flat, k, seed=k)
        out = quiet(solver.solve_meshed_load_case_currents, system.prob, meshes, system.layer_of, cases, cuts,
                    per_case_fields=fields, disconnected_meshes_by_layer=disc)
        _RUNS[key] = (system, meshes, disc, cuts, solver.check_load_cases(system.prob, cases), *out)
    return _RUNS[key]


def potentials(system, sol):
    return np.concatenate(mesh_order(system, [[zf.values for zf in ls.potentials] for ls in sol.layer_solutions]))


def case_rows(system, case):
    """The element rows of ``system`` with the values of one load case, restated: the value sits at position 3 of a
    source's row and at position 5 of a regulator's."""
    rows = []
    for (element, row) in system.pairs:
        if element in case:
            at = 5 if row[0] == "REG" else 3
            row = tuple(case[element] if p == at else v for p, v in enumerate(row))
        rows.append(row)
    return rows


def refined_solves(M, B):
    """M X = B by one LU and two steps of iterative refinement whose residual is formed in extended precision from the
    sparse M (every row of a KKT system has entries): the forward error is near eps, not eps cond(M)."""
    M = sp.csr_matrix(M)
    lu = spla.splu(sp.csc_matrix(M))
    data = M.data.astype(np.longdouble)
    X = []
    for b in np.asarray(B, dtype=np.float64).T:
        x = np.asarray(lu.solve(b), dtype=np.longdouble)
        for _ in range(2):
            res = b.astype(np.longdouble) - np.add.reduceat(data * x[M.indices], M.indptr[:-1])
            x = x + lu.solve(np.asarray(res, dtype=np.float64))
        X.append(np.asarray(x, dtype=np.float64))
    return np.stack(X, axis=1)


def check_report(system, meshes, cuts, sol, rep, rows, xd):
    """One case's CurrentReport against the restatement on ``sol``'s own potentials, as
    test_currents.py::test_every_output_against_the_host_restatement checks it; ``xd``: the direct solve with ``rows``."""
    n_layers = len(system.prob.layers)
    x = potentials(system, sol)
    toff = np.concatenate([[0], np.cumsum([len(m.triangles) for m in meshes])])
    J_want, size = C.face_J(system, x)
    J = np.concatenate(mesh_order(system, rep.vectors))
    mag = np.concatenate([tf.values for tf in mesh_order(system, rep.magnitudes)])
    assert J.shape == J_want.shape and mag.shape == (len(J),)
    assert (np.abs(J - J_want) <= TOL * size[:, None]).all()
    mag_want = np.hypot(J_want[:, 0], J_want[:, 1])
    assert (np.abs(mag - mag_want) <= TOL * size).all()
    for li, (got, want) in enumerate(zip(rep.hotspots, C.hotspots(system, mag_want, n_layers))):
        assert (got is None) == (want is None), li
        if got is None:
            continue
        value, mesh_in_layer, face, cx, cy = got
        mi = [m for m, l in enumerate(system.layer_of) if l == li][mesh_in_layer]
        g = int(toff[mi] + face)
        assert value == mag[g]
        assert abs(value - want[0]) <= TOL * size[want[1]], li
        assert g == want[1] or mag_want[g] >= want[0] - TOL * max(size[g], size[want[1]]), li
        assert (cx, cy) == pytest.approx(tuple(meshes[mi].points[meshes[mi].triangles[face]].mean(axis=0)), rel=1e-14)
    want_layers = C.layer_power(system, x, n_layers)
    assert len(rep.layers) == n_layers
    assert all(abs(g - w) <= TOL * w for g, w in zip(rep.layers, want_layers))
    assert len(rep.cuts) == len(cuts)
    for c, got in zip(cuts, rep.cuts):
        li = next(i for i, layer in enumerate(system.prob.layers) if layer is c.layer)
        end = (c.end.x, c.end.y) if hasattr(c.end, "x") else c.end
        want, scale = C.cut_current(system, x, li, c.start, end)
        assert abs(got - want) <= TOL * scale, (c, got, want)
    want_el = C.element_flows(rows, xd)
    assert len(rep.elements) == len(rows)
    flows = list(rep.elements.values())
    for key in ("current", "power", "input_current", "input_power"):
        idx = [i for i, d in enumerate(want_el) if key in d]
        if idx:
            got = np.array([flows[i][key] for i in idx])
            ref = np.array([want_el[i][key] for i in idx])
            assert np.abs(got - ref).max() <= REL_TOL * np.abs(ref).max(), key
    assert np.abs(x - xd[:len(x)]).max() <= REL_TOL * np.abs(xd).max()
    # Tellegen per case: what the elements absorb and what the copper dissipates add up to zero
    terms = [d[k] for d in flows for k in ("power", "input_power") if k in d] + list(rep.layers)
    assert all(p >= 0 for p in rep.layers)
    assert abs(sum(terms)) <= REL_TOL * sum(abs(t) for t in terms)


def check_all_cases(system, meshes, cuts, cases, sols, reps):
    all_rows = [case_rows(system, case) for case in cases]
    M, _ = system.assemble()
    X = refined_solves(M, np.stack([system.assemble(rows=rows)[1] for rows in all_rows], axis=1))
    assert len(sols) == len(reps) == len(cases)
    for j, (sol, rep, rows) in enumerate(zip(sols, reps, all_rows)):
        check_report(system, meshes, cuts, sol, rep, rows, X[:, j])
        # the report's elements are those of the Solution's substituted Problem, in stamping order
        assert list(rep.elements) == [e for network in sol.problem.networks for e in network.elements]


def flat_report(rep):
    """The arrays and scalars of a CurrentReport that do not depend on per_case_fields."""
    return rep.hotspots, rep.layers, rep.cuts, [sorted(d.items()) for d in rep.elements.values()]


def same_arrays(a, b):
    return len(a) == len(b) and all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def envelope_arrays(env):
    return ([tf.values for forms in env.magnitudes for tf in forms], [c for cs in env.cases for c in cs])


# ---- 1. every case against the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("name", PROBLEMS)
def test_every_case_against_the_host_restatement(ctx, name, k):
    system, meshes, _disc, cuts, cases, sols, reps, _env = run(name, k)
    check_all_cases(system, meshes, cuts, cases, sols, reps)
    crossed = sum(abs(c) > 0 for c in reps[0].cuts)
    assert crossed >= len(system.prob.layers)


# ---- 2. column 0 is the one-column kernels, bit for bit ---------------------------------------------------------------

def finished_block(board, L, cases):
    """A plan on ``L`` with the block of ``cases`` solved and finished: (plan, V, the arguments of its face kernels)."""
    k = len(cases)
    rows, cols, vals = solver.stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], cases)
    red, kidx, kval = solver.block_plan_inputs(L, rows, cols, vals, k)
    plan = _hip.KktPlan(L.dev, L.layout.n_potential, red.elim, red.tied, red.n_free)
    p, _ = plan.solve_block_coo(k, rows, cols, vals, kidx, kval, red.regulator_columns, red.probe_members, rtol=solver.RTOL,
                                abs_residual_target=solver.ABS_RESIDUAL_TARGET)
    V, _ = solver._finish_block(plan, red, red.probe_members, p, k)
    return plan, V


def plan_cuts(system, cuts):
    checked = solver.check_cuts(system.prob, cuts)
    return [c[0] for c in checked], np.array([[*a, *b] for _, a, b in checked]).reshape(-1, 4)


@pytest.mark.parametrize("name", ["problem_mixed", "problem_many_meshes"])
def test_column_0_is_the_existing_kernels_bit_for_bit(ctx, name):
    """On one finished block of 3 columns, column 0 of ``current_cases`` is ``current_report`` (which reads column 0) and
    its per-mesh power is ``sensitivity_block`` with lambda = column 0 (W = e_0: 1 x_0 + 0 x_1 + 0 x_2 is x_0 exactly).  A
    one-column block of case 0's right-hand side then gives ``sensitivity_block(ones((1, 1)))``'s bits too: bitwise equality
    is asked of two kernels on the same V, never across two solves.  A finished block of 9 columns in between: there too
    ``current_report`` is row 0 of ``current_cases``."""
    system = S.problem_system(name)
    meshes, _ = board_of(system, name)
    cases = solver.check_load_cases(system.prob, block_cases(system.flat, 3, seed=3))
    cl, cxy = plan_cuts(system, random_cuts(system))
    board = solver.index_board(system.prob, meshes, system.layer_of)
    ml = np.asarray(system.layer_of, dtype=np.int32)
    with board.assembled() as (L, _):
        n_tri, n_mesh = len(L.tri), len(meshes)
        plan, _V = finished_block(board, L, cases)
        J, mag, env, env_case, mmax, mface, mpow, cut = plan.current_cases(3, n_tri, ml, cl, cxy)
        J0, mag0, mmax0, mface0, cut0 = plan.current_report(3, n_tri, ml, cl, cxy)
        _, _, totals = plan.sensitivity_block(np.array([[1.0, 0.0, 0.0]]), n_tri, n_mesh)
        assert J.shape == (3, n_tri, 2) and mag.shape == (3, n_tri) and cut.shape == (3, len(cl))
        assert mmax.shape == mface.shape == mpow.shape == (3, n_mesh)
        assert np.array_equal(J[0], J0) and np.array_equal(mag[0], mag0)
        assert np.array_equal(mmax[0], mmax0) and np.array_equal(mface[0], mface0) and np.array_equal(cut[0], cut0)
        assert np.array_equal(mpow[0], totals[0]) and (mpow[0] > 0).any()
        assert np.abs(cut0).max() > 0 and not np.array_equal(mag[1], mag[0])
        want_env, want_case = solver.envelope_of(mag)
        assert np.array_equal(env, want_env) and np.array_equal(env_case, want_case) and env_case.dtype == np.int32
        plan.close()
        # nine columns: column 0 is read with a stride beyond one chunk, and both chunk sizes meet a second, partial chunk
        nine, _ = finished_block(board, L, solver.check_load_cases(system.prob, block_cases(system.flat, 9, seed=9)))
        J9, mag9, _, _, mmax9, mface9, _, cut9 = nine.current_cases(9, n_tri, ml, cl, cxy)
        J0, mag0, mmax0, mface0, cut0 = nine.current_report(9, n_tri, ml, cl, cxy)
        assert np.array_equal(J9[0], J0) and np.array_equal(mag9[0], mag0)
        assert np.array_equal(mmax9[0], mmax0) and np.array_equal(mface9[0], mface0) and np.array_equal(cut9[0], cut0)
        assert np.abs(cut0).max() > 0 and not np.array_equal(mag9[8], mag9[0])
        nine.close()
        one, _ = finished_block(board, L, cases[:1])
        *_, mpow1, _ = one.current_cases(1, n_tri, ml, cl, cxy)
        _, _, totals1 = one.sensitivity_block(np.ones((1, 1)), n_tri, n_mesh)
        assert np.array_equal(mpow1[0], totals1[0])
        one.close()


@pytest.mark.parametrize("name", ["problem_mixed", "problem_c1", "problem_many_meshes"])
def test_one_case_is_solve_meshed_currents_bit_for_bit(ctx, name):
    system = S.problem_system(name)
    meshes, disc = board_of(system, name)
    cuts = random_cuts(system)
    (sol,), (rep,), env = quiet(solver.solve_meshed_load_case_currents, system.prob, meshes, system.layer_of, [{}], cuts,
                                disconnected_meshes_by_layer=disc)
    ref_sol, ref = quiet(solver.solve_meshed_currents, system.prob, meshes, system.layer_of, cuts,
                         disconnected_meshes_by_layer=disc)
    assert sol.problem is system.prob
    assert sol.solver_info.ground_node_current == ref_sol.solver_info.ground_node_current
    assert sol.solver_info.residual_norm == ref_sol.solver_info.residual_norm
    assert sol.solver_info.iterations == ref_sol.solver_info.iterations
    for la, lb in zip(sol.layer_solutions, ref_sol.layer_solutions):
        assert same_arrays([z.values for z in la.potentials], [z.values for z in lb.potentials])
        assert same_arrays([t.values for t in la.power_densities], [t.values for t in lb.power_densities])
        assert len(la.disconnected_meshes) == len(lb.disconnected_meshes)
    assert flat_report(rep) == flat_report(ref) and list(rep.elements) == list(ref.elements)
    for va, vb, ma, mb in zip(rep.vectors, ref.vectors, rep.magnitudes, ref.magnitudes):
        assert same_arrays(va, vb) and same_arrays([t.values for t in ma], [t.values for t in mb])
    # the envelope of one case is that case
    assert same_arrays(envelope_arrays(env)[0], [t.values for forms in rep.magnitudes for t in forms])
    assert all((c == 0).all() for c in envelope_arrays(env)[1])
    assert env.cuts == [(c, 0) for c in rep.cuts] and env.layers == [(p, 0) for p in rep.layers]


# ---- 3. the envelope ----------------------------------------------------------------------------------------------------

def check_envelope(reps, env, n_layers):
    k = len(reps)
    for li in range(n_layers):
        for mi, (tf, which) in enumerate(zip(env.magnitudes[li], env.cases[li])):
            want, want_case = solver.envelope_of(np.stack([rep.magnitudes[li][mi].values for rep in reps]))
            assert np.array_equal(tf.values, want, equal_nan=True) and np.array_equal(which, want_case)
            assert which.dtype == np.int32 and which.shape == tf.values.shape
        spots = [rep.hotspots[li] for rep in reps]
        if spots[0] is None:
            assert env.hotspots[li] is None
        else:
            _, (c,) = solver.envelope_of(np.array([[s[0]] for s in spots]))
            assert env.hotspots[li] == (spots[c][0], c, *spots[c][1:])
    values = np.array([rep.layers for rep in reps]).reshape(k, -1)
    best, case = solver.envelope_of(values)
    assert env.layers == [(float(values[c, i]), int(c)) for i, c in enumerate(case)]
    assert [abs(v) for v, _ in env.layers] == list(best)
    values = np.array([rep.cuts for rep in reps]).reshape(k, -1)
    best, case = solver.envelope_of(values)
    assert env.cuts == [(float(values[c, i]), int(c)) for i, c in enumerate(case)]
    assert [abs(v) for v, _ in env.cuts] == list(best)
    flows = [list(rep.elements.values()) for rep in reps]
    assert len(env.elements) == len(flows[0])
    for i, worst in enumerate(env.elements.values()):
        assert set(worst) == set(flows[0][i])
        for key, (value, c) in worst.items():
            column = np.array([[f[i][key]] for f in flows])
            best, (want_c,) = solver.envelope_of(column)
            assert c == want_c and value == column[c, 0] and abs(value) == best[0]


def run_with_the_island(k):
    """problem_many_meshes with its floating island (the golden's disconnected mesh: copper no connection touches) solved
    as copper like every other mesh, appended as the last mesh on its layer: nothing ties it to the ground node, so it is
    held at 0 V and carries no current in any case.  (system of the connected meshes, the island's layer, reports,
    envelope), solved once per module."""
    key = ("island", k)
    if key not in _RUNS:
        system = S.problem_system("problem_many_meshes")
        meshes, disc = board_of(system, "problem_many_meshes")
        (layer, (island,)), = [(li, ms) for li, ms in enumerate(disc) if ms]
        cases = block_cases(system.flat, k, seed=k)
        _sols, reps, env = quiet(solver.solve_meshed_load_case_currents, system.prob, meshes + [island],
                                 list(system.layer_of) + [layer], cases, random_cuts(system))
        _RUNS[key] = (system, layer, reps, env)
    return _RUNS[key]


@pytest.mark.parametrize("k", [3, 9])
def test_the_envelope_is_envelope_of_the_cases_and_the_floating_island_ties_at_zero(ctx, k):
    system, layer, reps, env = run_with_the_island(k)
    check_envelope(reps, env, len(system.prob.layers))
    assert list(env.elements) == [e for e, _ in system.pairs]
    mags, which = envelope_arrays(env)
    if k == 9:
        assert any((c != 0).any() for c in which)                         # the Problem as given is not the worst everywhere
    # the island's |J| is exactly 0 in every case: every one of its faces is a tie of all cases, which goes to case 0
    dead = [(m == 0) for m in mags]
    island = env.magnitudes[layer][-1].values
    print(f"faces at exactly 0: {sum(int(d.sum()) for d in dead)}; the island has {len(island)}, |J| up to {island.max():.3g}")
    assert sum(int(d.sum()) for d in dead) > 0
    assert len(island) > 0 and (island == 0).all() and (env.cases[layer][-1] == 0).all()
    assert all((c[d] == 0).all() for c, d in zip(which, dead))
    for rep in reps:
        per_case = [tf.values for forms in rep.magnitudes for tf in forms]
        assert all((p[d] == 0).all() for p, d in zip(per_case, dead))
        assert max(h[0] for h in rep.hotspots) > 0


def test_the_envelope_is_envelope_of_the_cases_with_a_regulator(ctx):
    system, _meshes, _disc, _cuts, _cases, _sols, reps, env = run("problem_mixed", 9)
    check_envelope(reps, env, len(system.prob.layers))
    assert list(env.elements) == [e for e, _ in system.pairs]
    assert any((c != 0).any() for c in envelope_arrays(env)[1])


def test_two_zero_cases_tie_at_case_0_everywhere(ctx):
    system = S.problem_system("problem_many_meshes")
    meshes, disc = board_of(system, "problem_many_meshes")
    zero = {e: 0.0 for e in system.flat if solver.element_kind(e) in solver.CASE_FIELDS}
    _sols, reps, env = quiet(solver.solve_meshed_load_case_currents, system.prob, meshes, system.layer_of, [zero, dict(zero)],
                             random_cuts(system), disconnected_meshes_by_layer=disc)
    mags, which = envelope_arrays(env)
    assert all((m == 0).all() for m in mags) and all((c == 0).all() for c in which)
    assert all(c == 0 for _, c in env.cuts + env.layers) and all(h[1] == 0 for h in env.hotspots if h is not None)
    assert all(c == 0 for worst in env.elements.values() for _, c in worst.values())
    check_envelope(reps, env, len(system.prob.layers))


# ---- 4. per_case_fields=False ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k", [("problem_many_meshes", 3), ("problem_mixed", 9)])
def test_envelope_only_gives_the_same_bits_without_the_fields(ctx, name, k):
    _system, _meshes, _disc, _cuts, _cases, sols, reps, env = run(name, k)
    *_, sols2, reps2, env2 = run(name, k, fields=False)
    assert all(rep.vectors is None and rep.magnitudes is None for rep in reps2)
    assert [flat_report(rep) for rep in reps2] == [flat_report(rep) for rep in reps]
    assert all(same_arrays(a, b) for a, b in zip(envelope_arrays(env), envelope_arrays(env2)))
    assert (env2.hotspots, env2.layers, env2.cuts) == (env.hotspots, env.layers, env.cuts)
    assert list(env2.elements.values()) == list(env.elements.values())
    for a, b in zip(sols, sols2):
        for la, lb in zip(a.layer_solutions, b.layer_solutions):
            assert same_arrays([z.values for z in la.potentials], [z.values for z in lb.potentials])
            assert same_arrays([t.values for t in la.power_densities], [t.values for t in lb.power_densities])


# ---- 5. tile and chunk edges ------------------------------------------------------------------------------------------------

def grid_with_faces(n_faces, y0, seed):
    """A jittered strip of exactly ``n_faces`` triangles from (0, y0): a 2-row grid of ceil(n_faces / 2) cells; for an odd
    n_faces, less the corner of its last cell that only one triangle has, with that triangle."""
    cells = (n_faces + 1) // 2
    xy, tri = synthetic.jittered_grid(cells + 1, 2, h=0.25, seed=seed, jitter=0.2, origin=(0.0, y0))
    xy, tri = np.asarray(xy), np.asarray(tri).reshape(-1, 3)
    if n_faces % 2:
        corner = next(v for v in (cells, 2 * cells + 1) if (tri == v).sum() == 1)
        tri = tri[~(tri == corner).any(axis=1)]
        tri = tri - (tri > corner)
        xy = np.delete(xy, corner, axis=0)
    assert len(tri) == n_faces and len(np.unique(tri)) == len(xy)
    return mesh.Mesh(xy, tri.astype(np.int32))


def tile_edge_board():
    """One layer with meshes of 255, 256 and 257 faces in series between a voltage source and a load, and a current source
    across the middle one: (system, meshes, cuts, the sources)."""
    lay = problem.Layer(shape=H.Geoms(3), name="L0", conductance=2000.0)
    meshes = [grid_with_faces(n, 3.0 * i, seed=10 + i) for i, n in enumerate((255, 256, 257))]
    left = [problem.Connection(layer=lay, point=H.XY(0.0, 3.0 * i)) for i in range(3)]
    right = [problem.Connection(layer=lay, point=H.XY(float(m.points[:, 0].max()), 3.0 * i + 0.25)) for i, m in enumerate(meshes)]
    g = problem.NodeID()
    vs = problem.VoltageSource(p=left[0].node_id, n=g, voltage=1.0)
    cs = problem.CurrentSource(f=right[1].node_id, t=left[1].node_id, current=0.4)
    elements = [vs, problem.Resistor(a=right[0].node_id, b=left[1].node_id, resistance=0.01),
                problem.Resistor(a=right[1].node_id, b=left[2].node_id, resistance=0.02),
                problem.Resistor(a=right[2].node_id, b=g, resistance=0.5), cs]
    prob = problem.Problem(layers=[lay], networks=[problem.Network(connections=left + right, elements=elements)])
    layer_of = [0, 0, 0]
    vindex = solver.VertexIndexer.create(meshes)
    nodes = solver.NodeIndexer.create(prob, meshes, layer_of, vindex, list(prob.networks))
    pairs = solver.global_elements(list(prob.networks), nodes)
    system = S.System(meshes=[(m.points, m.triangles, lay.conductance) for m in meshes], n_internal=nodes.internal_node_count,
                      rows=[row for _, row in pairs], ground=solver.find_best_ground_node_index(prob, nodes),
                      layer_of=layer_of, prob=prob, pairs=pairs, nodes=nodes, flat=elements)
    cuts = [solver.Cut(lay, (10.03, -1.0 + 3.0 * i), (10.11, 1.0 + 3.0 * i)) for i in range(3)]
    cuts.append(solver.Cut(lay, (-1.0, -0.5), (40.0, 7.0)))
    return system, meshes, cuts, (vs, cs)


@pytest.mark.parametrize("k", [1, 2, 8, 9, 17])
def test_tile_and_chunk_edges(ctx, k):
    system, meshes, cuts, (vs, cs) = tile_edge_board()
    assert [len(m.triangles) for m in meshes] == [255, 256, 257]
    rng = np.random.default_rng(k)
    cases = [{}] + [{vs: float(rng.uniform(0.5, 2.0)), cs: float(rng.uniform(-2.0, 2.0))} for _ in range(k - 1)]
    sols, reps, env = quiet(solver.solve_meshed_load_case_currents, system.prob, meshes, system.layer_of, cases, cuts)
    check_all_cases(system, meshes, cuts, solver.check_load_cases(system.prob, cases), sols, reps)
    assert all(abs(c) > 0 for c in reps[0].cuts[:3])
    check_envelope(reps, env, 1)


# ---- 6. against separate solves -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", PROBLEMS)
def test_every_case_against_a_separate_solve(ctx, name):
    system, meshes, disc, cuts, _cases, sols, reps, _env = run(name, 3)
    for j, (sol, rep) in enumerate(zip(sols, reps)):
        # the cuts name the layers of the Problem as given, which every substituted Problem shares
        _, ref = quiet(solver.solve_meshed_currents, sol.problem, meshes, system.layer_of, cuts, disconnected_meshes_by_layer=disc)
        mag = np.concatenate([tf.values for forms in rep.magnitudes for tf in forms])
        want = np.concatenate([tf.values for forms in ref.magnitudes for tf in forms])
        scale = want.max()
        assert scale > 0 and np.abs(mag - want).max() <= REL_TOL * scale, j
        assert list(rep.elements) == list(ref.elements)
        assert np.abs(np.array(rep.cuts) - np.array(ref.cuts)).max() <= REL_TOL * scale, j


# ---- 7. the same bits twice -------------------------------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits(ctx):
    system, meshes, disc, cuts, cases, _sols, reps, env = run("problem_mixed", 9)
    _, reps2, env2 = quiet(solver.solve_meshed_load_case_currents, system.prob, meshes, system.layer_of, cases, cuts,
                           disconnected_meshes_by_layer=disc)
    for a, b in zip(reps, reps2):
        assert flat_report(a) == flat_report(b)
        for va, vb, ma, mb in zip(a.vectors, b.vectors, a.magnitudes, b.magnitudes):
            assert same_arrays(va, vb) and same_arrays([t.values for t in ma], [t.values for t in mb])
    assert all(same_arrays(p, q) for p, q in zip(envelope_arrays(env), envelope_arrays(env2)))
    assert (env2.hotspots, env2.layers, env2.cuts) == (env.hotspots, env.layers, env.cuts)
    assert list(env2.elements.values()) == list(env.elements.values())


# ---- 8. the plan-level entry's refusals ---------------------------------------------------------------------------------------------

def test_plan_level_entry_refuses_what_it_cannot_do(ctx):
    system = S.problem_system("problem_mixed")
    meshes, _ = board_of(system, "problem_mixed")
    cases = solver.check_load_cases(system.prob, block_cases(system.flat, 2, seed=2))
    board = solver.index_board(system.prob, meshes, system.layer_of)
    with board.assembled() as (L, _):
        rows, cols, vals = solver.stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], cases)
        red, kidx, kval = solver.block_plan_inputs(L, rows, cols, vals, 2)
        plan = _hip.KktPlan(L.dev, L.layout.n_potential, red.elim, red.tied, red.n_free)
        n_tri, ml = len(L.tri), np.asarray(system.layer_of, dtype=np.int32)
        one = ([0], [[0.5, 0.5, 1.5, 1.0]])
        with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):
            plan.current_cases(2, n_tri, ml, *one)
        p, _ = plan.solve_block_coo(2, rows, cols, vals, kidx, kval, red.regulator_columns, red.probe_members, rtol=solver.RTOL,
                                    abs_residual_target=solver.ABS_RESIDUAL_TARGET)
        solver._finish_block(plan, red, red.probe_members, p, 2)
        with pytest.raises(ValueError, match="as many columns"):
            plan.current_cases(3, n_tri, ml, *one)
        with pytest.raises(ValueError, match="4096"):
            plan.current_cases(2, n_tri, ml, [0] * 4097, np.ones((4097, 4)) * [0, 0, 1, 1])
        with pytest.raises(ValueError, match="finite"):
            plan.current_cases(2, n_tri, ml, [0], [[0.0, np.inf, 1.0, 1.0]])
        with pytest.raises(ValueError, match="must differ"):
            plan.current_cases(2, n_tri, ml, [0], [[1.0, 2.0, 1.0, 2.0]])
        with pytest.raises(ValueError, match="n_tri and n_mesh"):
            plan.current_cases(2, n_tri + 1, ml, *one)
        first = plan.current_cases(2, n_tri, ml, *one)                          # the plan is still usable, and the V stays
        second = plan.current_cases(2, n_tri, ml, *one)
        assert all(np.array_equal(a, b) for a, b in zip(first, second))
        bare = plan.current_cases(2, n_tri, ml, *one, fields=False)
        assert bare[0] is None and bare[1] is None and all(np.array_equal(a, b) for a, b in zip(first[2:], bare[2:]))
        assert first[0].shape == (2, n_tri, 2) and first[4].shape == (2, len(meshes)) and first[7].shape == (2, 1)
        plan.close()

"""``solve_meshed_currents`` on the device: every output against the host restatement (tests/currents_ref.py) on the
Solution's own potentials, the Solution against ``solve_meshed``, the power balance of elements and copper, Kirchhoff's
current law through cuts on synthetic boards, bitwise repeatability, and the plan-level entry's refusals."""
import importlib.util
import os
import warnings

import numpy as np
import pytest

import currents_ref as C
import helpers as H
import sensitivity_ref as S
from padne_amd import _hip, mesh, problem, solver, synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-12
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


def random_cuts(system, seed=0, per_layer=4):
    """Seeded random segments on every layer, within its vertices' bounding box grown by 20 % (some end in copper, some
    outside it), and one diagonal across the whole box."""
    rng = np.random.default_rng(seed)
    xy = C.all_xy(system)
    offs = system.offsets
    out = []
    for li, layer in enumerate(system.prob.layers):
        pts = np.concatenate([xy[offs[mi]:offs[mi + 1]] for mi, l in enumerate(system.layer_of) if l == li])
        lo, hi = pts.min(axis=0), pts.max(axis=0)
        lo, hi = lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo)
        for _ in range(per_layer):
            a, b = rng.uniform(lo, hi), rng.uniform(lo, hi)
            out.append(solver.Cut(layer, tuple(a), H.XY(*b)))
        out.append(solver.Cut(layer, tuple(lo), tuple(hi)))
    return out


def currents(name, cuts=None):
    system = S.problem_system(name)
    meshes, disc = board_of(system, name)
    cuts = random_cuts(system) if cuts is None else cuts
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        sol, rep = solver.solve_meshed_currents(system.prob, meshes, system.layer_of, cuts, disconnected_meshes_by_layer=disc)
    return system, meshes, cuts, sol, rep


def mesh_order(system, per_layer):
    """Per-layer, per-mesh lists (LayerSolution order) -> a list in mesh order."""
    out = [None] * len(system.layer_of)
    for li, items in enumerate(per_layer):
        for item, mi in zip(items, [mi for mi, l in enumerate(system.layer_of) if l == li]):
            out[mi] = item
    return out


def potentials(system, sol):
    return np.concatenate(mesh_order(system, [[zf.values for zf in ls.potentials] for ls in sol.layer_solutions]))


@pytest.mark.parametrize("name", PROBLEMS)
def test_every_output_against_the_host_restatement(ctx, name):
    system, meshes, cuts, sol, rep = currents(name)
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
        assert value == mag[g]                                           # the hotspot is a face of ``magnitudes``
        assert abs(value - want[0]) <= TOL * size[want[1]], li
        # another face than the restatement's only when its |J| is within rounding of the maximum
        assert g == want[1] or mag_want[g] >= want[0] - TOL * max(size[g], size[want[1]]), li
        assert (cx, cy) == pytest.approx(tuple(meshes[mi].points[meshes[mi].triangles[face]].mean(axis=0)), rel=1e-14)
    want_layers = C.layer_power(system, x, n_layers)
    assert len(rep.layers) == n_layers
    assert all(abs(g - w) <= TOL * w for g, w in zip(rep.layers, want_layers))
    assert len(rep.cuts) == len(cuts)
    crossed = 0
    for c, got in zip(cuts, rep.cuts):
        li = next(i for i, layer in enumerate(system.prob.layers) if layer is c.layer)
        end = (c.end.x, c.end.y) if hasattr(c.end, "x") else c.end
        want, scale = C.cut_current(system, x, li, c.start, end)
        assert abs(got - want) <= TOL * scale, (c, got, want)
        crossed += scale > 0
    assert crossed >= n_layers
    # element flows: the restatement on a direct solve (the internal nodes and source currents are not in the Solution)
    M, r = system.assemble()
    xd = S.solve(M, r)
    want_el = C.element_flows(system.rows, xd)
    assert list(rep.elements) == [e for e, _ in system.pairs]
    for key in ("current", "power", "input_current", "input_power"):
        idx = [i for i, d in enumerate(want_el) if key in d]
        if idx:
            got = np.array([rep.elements[system.pairs[i][0]][key] for i in idx])
            ref = np.array([want_el[i][key] for i in idx])
            assert np.abs(got - ref).max() <= REL_TOL * np.abs(ref).max(), key
    assert np.abs(x - xd[:len(x)]).max() <= REL_TOL * np.abs(xd).max()


@pytest.mark.parametrize("name", PROBLEMS)
def test_the_solution_is_solve_meshed(ctx, name):
    system, meshes, _cuts, sol, _rep = currents(name, cuts=[])
    _, disc = board_of(system, name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        ref = solver.solve_meshed(system.prob, meshes, system.layer_of, disconnected_meshes_by_layer=disc)
    assert sol.problem is system.prob and sol.solver_info.residual_norm < 1e-9
    for la, lb in zip(sol.layer_solutions, ref.layer_solutions):
        assert len(la.disconnected_meshes) == len(lb.disconnected_meshes)
        for a, b in zip(la.potentials, lb.potentials):
            assert np.abs(a.values - b.values).max() <= REL_TOL * np.abs(b.values).max()
        for a, b in zip(la.power_densities, lb.power_densities):
            assert np.abs(a.values - b.values).max() <= REL_TOL * np.abs(b.values).max()


@pytest.mark.parametrize("name", PROBLEMS)
def test_power_balance(ctx, name):
    """Tellegen: what the elements absorb and what the copper dissipates add up to zero; a wrong sign anywhere breaks it."""
    _system, _meshes, _cuts, _sol, rep = currents(name, cuts=[])
    powers = [d[k] for d in rep.elements.values() for k in ("power", "input_power") if k in d]
    terms = powers + list(rep.layers)
    assert all(p >= 0 for p in rep.layers) and sum(rep.layers) > 0
    assert abs(sum(terms)) <= REL_TOL * sum(abs(t) for t in terms), (sum(powers), sum(rep.layers))


# ---- Kirchhoff's current law through cuts on synthetic boards ------------------------------------------------------

def layer(name="L0", sigma=2000.0):
    return problem.Layer(shape=H.Geoms(1), name=name, conductance=sigma)


def strip(y0=0.0, seed=1, jitter=0.2, nx=41, ny=9, h=0.25):
    """A 10 mm x 2 mm strip from (0, y0)."""
    xy, tri = synthetic.jittered_grid(nx, ny, h=h, seed=seed, jitter=jitter, origin=(0.0, y0))
    return mesh.Mesh(xy, tri)


def conn(lay, x, y):
    return problem.Connection(layer=lay, point=H.XY(x, y))


def solve(prob, meshes, layer_of, cuts):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        return solver.solve_meshed_currents(prob, meshes, layer_of, cuts)


def kcl(got, want):
    return abs(got - want) <= REL_TOL * abs(want)


def left_right_potentials(sol, li, mi, x_cut):
    """Mean potential of the vertices of mesh mi (within layer li) left of x = x_cut - 1 and right of x_cut + 1."""
    m, v = sol.layer_solutions[li].meshes[mi], sol.layer_solutions[li].potentials[mi].values
    return v[m.points[:, 0] < x_cut - 1].mean(), v[m.points[:, 0] > x_cut + 1].mean()


@pytest.mark.parametrize("jitter", [0.2, 0.0])
def test_a_strip_fed_by_a_current_source(ctx, jitter):
    lay = layer()
    cl, cr = conn(lay, 0.0, 1.0), conn(lay, 10.0, 1.0)
    src = problem.CurrentSource(f=cr.node_id, t=cl.node_id, current=1.5)      # through the copper from left to right
    prob = problem.Problem(layers=[lay], networks=[problem.Network(connections=[cl, cr], elements=[src])])
    cuts = [solver.Cut(lay, (4.03, -1.0), (4.11, 3.0)), solver.Cut(lay, (8.9, 3.1), H.XY(9.2, -2.0)),
            solver.Cut(lay, (5.0, -1.0), (5.0, 3.0)), solver.Cut(lay, (5.0, 3.0), (5.0, -1.0))]
    sol, rep = solve(prob, [strip(jitter=jitter)], [0], cuts)
    # upward cuts: left is -x, the current crosses them from left to right; downward ones the other way.  On the
    # unjittered strip the last two run through a column of vertices
    assert kcl(rep.cuts[0], 1.5) and kcl(rep.cuts[1], -1.5) and kcl(rep.cuts[2], 1.5) and kcl(rep.cuts[3], -1.5), rep.cuts
    hi, lo = left_right_potentials(sol, 0, 0, 5.0)
    assert hi > lo                                                            # from the higher potential to the lower
    assert rep.elements[src]["current"] == 1.5 and rep.elements[src]["power"] < 0
    (value, mi, face, cx, cy), = rep.hotspots
    assert mi == 0 and value == rep.magnitudes[0][0].values.max()


def test_a_strip_fed_by_a_voltage_source_into_a_resistor(ctx):
    lay = layer()
    cl, cr, g = conn(lay, 0.0, 1.0), conn(lay, 10.0, 1.0), problem.NodeID()
    vs = problem.VoltageSource(p=cl.node_id, n=g, voltage=1.0)
    load = problem.Resistor(a=cr.node_id, b=g, resistance=0.5)
    prob = problem.Problem(layers=[lay], networks=[problem.Network(connections=[cl, cr], elements=[vs, load])])
    _sol, rep = solve(prob, [strip()], [0], [solver.Cut(lay, (4.03, -1.0), (4.11, 3.0))])
    i_load = rep.elements[load]["current"]
    assert 1.0 < i_load < 2.0                                                 # 1 V over 0.5 Ohm and the strip
    assert kcl(rep.cuts[0], i_load) and kcl(rep.elements[vs]["current"], -i_load)
    assert rep.elements[vs]["power"] < 0 < rep.elements[load]["power"]


def test_two_parallel_strips_share_the_source_current(ctx):
    lay = layer()
    aL, bL, aR, bR = conn(lay, 0.0, 1.0), conn(lay, 0.0, 4.0), conn(lay, 10.0, 1.0), conn(lay, 10.0, 4.0)
    n_in, n_out = problem.NodeID(), problem.NodeID()
    src = problem.CurrentSource(f=n_out, t=n_in, current=2.0)
    ra = problem.Resistor(a=n_in, b=aL.node_id, resistance=0.01)
    rb = problem.Resistor(a=n_in, b=bL.node_id, resistance=0.03)
    ra2 = problem.Resistor(a=aR.node_id, b=n_out, resistance=0.01)
    rb2 = problem.Resistor(a=bR.node_id, b=n_out, resistance=0.02)
    net = problem.Network(connections=[aL, bL, aR, bR], elements=[src, ra, rb, ra2, rb2])
    prob = problem.Problem(layers=[lay], networks=[net])
    cuts = [solver.Cut(lay, (5.0, -1.0), (5.1, 2.5)), solver.Cut(lay, (5.0, 2.6), (5.2, 6.0)),
            solver.Cut(lay, (5.3, -1.0), (5.3, 6.0))]
    _sol, rep = solve(prob, [strip(), strip(y0=3.0, seed=2)], [0, 0], cuts)
    a, b, both = rep.cuts
    assert 0.1 < a < 1.9 and 0.1 < b < 1.9 and abs(a - b) > 0.05              # unequal paths, unequal shares
    assert kcl(a + b, 2.0) and kcl(both, 2.0)
    assert kcl(a, rep.elements[ra]["current"]) and kcl(b, rep.elements[rb]["current"])
    assert kcl(a, rep.elements[ra2]["current"]) and kcl(b, rep.elements[rb2]["current"])


def test_two_layers_with_via_resistors(ctx):
    top, bottom = layer("top"), layer("bottom", 1000.0)
    c0, c1 = conn(top, 0.0, 1.0), conn(bottom, 0.0, 1.0)
    src = problem.CurrentSource(f=c1.node_id, t=c0.node_id, current=1.2)      # into the top layer, back out of the bottom
    nets = [problem.Network(connections=[c0, c1], elements=[src])]
    vias = []
    for k, x in enumerate((8.0, 9.0, 9.6)):
        a, b = conn(top, x, 1.0), conn(bottom, x, 1.0)
        vias.append(problem.Resistor(a=a.node_id, b=b.node_id, resistance=1e-3 * (k + 1)))
        nets.append(problem.Network(connections=[a, b], elements=[vias[-1]]))
    prob = problem.Problem(layers=[top, bottom], networks=nets)
    cuts = [solver.Cut(top, (5.0, -1.0), (5.05, 3.0)), solver.Cut(bottom, (5.0, 3.0), (5.05, -1.0))]
    _sol, rep = solve(prob, [strip(), strip(seed=3)], [0, 1], cuts)
    through_vias = sum(rep.elements[v]["current"] for v in vias)
    # top: left to right across an upward cut; bottom: right to left, which is left to right across a downward cut
    assert kcl(rep.cuts[0], 1.2) and kcl(rep.cuts[1], 1.2) and kcl(through_vias, 1.2), (rep.cuts, through_vias)
    assert all(rep.elements[v]["current"] > 0 for v in vias)


# ---- repeatability, ties, the plan-level entry ----------------------------------------------------------------------

def load_case_board(side=20.0):
    path = os.path.join(os.path.dirname(H.HERE), "scripts", "load_cases.py")
    spec = importlib.util.spec_from_file_location("load_cases_script", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from padne_amd.structured import StructuredMesher
    prob, loads, source = mod.board(side, 5.0)
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=0.2)))
    return prob, meshes, layer_of


def test_repeatable_bitwise_and_a_cut_alone_is_the_same_cut(ctx):
    prob, meshes, layer_of = load_case_board()
    rng = np.random.default_rng(5)
    cuts = [solver.Cut(lay, tuple(rng.uniform(-2, 22, 2)), tuple(rng.uniform(-2, 22, 2))) for lay in prob.layers for _ in range(6)]
    cuts += [solver.Cut(lay, (-1.0, 10.3), (21.0, 10.1)) for lay in prob.layers]
    sol, rep = solve(prob, meshes, layer_of, cuts)
    _, again = solve(prob, meshes, layer_of, cuts)
    assert rep.cuts == again.cuts and rep.layers == again.layers and rep.hotspots == again.hotspots
    assert all(rep.elements[e] == again.elements[e] for e in rep.elements)
    for va, vb, ma, mb in zip(rep.vectors, again.vectors, rep.magnitudes, again.magnitudes):
        assert all(np.array_equal(a, b) for a, b in zip(va, vb))
        assert all(np.array_equal(a.values, b.values) for a, b in zip(ma, mb))
    assert any(abs(c) > 0 for c in rep.cuts[-len(prob.layers):])
    for li, (lay, ls) in enumerate(zip(prob.layers, sol.layer_solutions)):
        for mag, pd in zip(rep.magnitudes[li], ls.power_densities):
            assert np.all(np.abs(mag.values ** 2 / lay.conductance - pd.values) <= 1e-12 * pd.values + 1e-300)
    for j in (0, 7, len(cuts) - 1):
        _, one = solve(prob, meshes, layer_of, [cuts[j]])
        assert one.cuts == [rep.cuts[j]], j
    _, none = solve(prob, meshes, layer_of, [])
    assert none.cuts == [] and none.layers == rep.layers


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
        n_tri, ml = len(L.tri), np.asarray(layer_of, dtype=np.int32)
        one = ([0], [[0.5, 0.5, 1.5, 1.0]])
        with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):
            plan.current_report(1, n_tri, ml, *one)
        p, _ = plan.solve_block_coo(1, rows, cols, vals, kidx, kval, extras, members, rtol=solver.RTOL,
                                    abs_residual_target=solver.ABS_RESIDUAL_TARGET)
        solver._finish_block(plan, red, members, p, 1)
        with pytest.raises(ValueError, match="as many columns"):
            plan.current_report(2, n_tri, ml, *one)
        with pytest.raises(ValueError, match="4096"):
            plan.current_report(1, n_tri, ml, [0] * 4097, np.ones((4097, 4)) * [0, 0, 1, 1])
        with pytest.raises(ValueError, match="finite"):
            plan.current_report(1, n_tri, ml, [0], [[0.0, np.inf, 1.0, 1.0]])
        with pytest.raises(ValueError, match="must differ"):
            plan.current_report(1, n_tri, ml, [0], [[1.0, 2.0, 1.0, 2.0]])
        with pytest.raises(ValueError, match="n_tri and n_mesh"):
            plan.current_report(1, n_tri + 1, ml, *one)
        first = plan.current_report(1, n_tri, ml, *one)
        second = plan.current_report(1, n_tri, ml, *one)                        # the V stays: same bits
        assert all(np.array_equal(a, b) for a, b in zip(first, second))
        assert first[0].shape == (n_tri, 2) and first[3].shape == (len(meshes),) and first[4].shape == (1,)
        plan.close()

"""The transient electro-thermal solve on the device against the host restatement (tests/coupled_transient_ref.py, itself
checked by tests/test_coupled_transient_host.py): alpha = 0 against the one-way transient bit for bit; the new device entries
-- the scale from a transient state, the load slot written under way, the per-mesh heat, the range of the scale -- against the
restatement bit for bit; every step's temperatures and probed potentials against direct stepping; the uniform strip's scalar
recurrence through the Problem API; the balance of every step against that step's own electrical solve; the direction of the
effect; the strip without a steady state and ``stop_above``; a start from the steady electro-thermal state; repeatability,
the refusals of the device entries, and the public call under the guarded device pool.

Boards: those of tests/test_thermal.py on the films and source factors of coupled_ref.COUPLED_BOARDS / OTHER_BOARDS (rises of
tens of kelvin), c = 3e-3 as in tests/test_transient.py."""
import ctypes
import math

import numpy as np
import pytest

import coupled_ref as C
import coupled_transient_ref as CT
import thermal_ref as T
import transient_ref as R
import test_transient as TR
from padne_amd import _hip, solver
from test_coupled import alphas, in_mesh_order, sigma_of, strip_problem
from test_device_memory import three_ways
from test_load_case_currents import finished_block
from test_thermal import BAR, BOARDS, board, quiet
from test_transient import CAP, DT1, DT2, FILM, TAU, Stepping, everything

pytestmark = pytest.mark.gpu

ALL_BOARDS = dict(C.COUPLED_BOARDS, **C.OTHER_BOARDS)


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def model_of(film=FILM, ambient=25.0, initial=None, capacity=CAP, thermal=None, **kw):
    electro = solver.ElectroThermalModel(thermal=solver.ThermalModel(film=film, ambient=ambient, **(thermal or {})), **kw)
    return solver.ElectroThermalTransientModel(electrothermal=electro, areal_capacity=capacity, initial=initial)


def trace_arrays(trace):
    return [trace.increments, trace.scale_min, trace.scale_max, trace.delivered, *trace.potentials.values(),
            np.array([[it["electrical"], it["thermal"]] for it in trace.iterations])]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- 1. alpha = 0 is the one-way transient ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["single", "two_layer", "problem_many_meshes"])
def test_alpha_zero_is_the_one_way_transient_bit_for_bit(ctx, name):
    """On, off, on with another dt: every array of the TransientReport -- times, stored, loss, the heats, the fields at the
    segment ends, the envelope, the probe traces, the iterations per step -- and the Solution.  With alpha = 0 the scale is
    exactly 1, the revalued system has the assembled bits, sigma * 1 is sigma, and both calls solve the same one-column block."""
    prob, meshes, layer_of, disc, *_ = board(name)
    probes = [conn.node_id for conn in prob.networks[0].connections][:2]
    schedule = [solver.Segment(4 * DT1, 4, 0), solver.Segment(3 * DT2, 3, None), solver.Segment(3 * DT2, 3, 0)]
    kw = dict(probes=probes, keep="segments", disconnected_meshes_by_layer=disc)
    sols_w, rep_w = quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, TR.model_of(), schedule, **kw)
    sols, rep, trace = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of,
                             model_of(temperature_coefficient=0.0, conductance_temperature=-40.0), schedule, **kw)
    (arrays, scalars), (arrays_w, scalars_w) = everything(rep), everything(rep_w)
    assert scalars == scalars_w and same(arrays, arrays_w)
    for ls, ls_w in zip(sols[0].layer_solutions, sols_w[0].layer_solutions):
        for forms, forms_w in ((ls.potentials, ls_w.potentials), (ls.power_densities, ls_w.power_densities)):
            assert same([f.values for f in forms], [f.values for f in forms_w])
    on = np.array([False] + [True] * 4 + [False] * 3 + [True] * 3)
    assert (trace.scale_min[on] == 1.0).all() and (trace.scale_max[on] == 1.0).all() and np.isnan(trace.scale_min[~on]).all()
    assert (trace.increments[on] >= 0.0).all() and trace.stopped is None
    assert rep.total_heat.max() > 0.0 and (trace.delivered[~on] == 0.0).all()


# ---- 2. the new entries against the restatement ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["single", "two_in_layer", "two_layer"])
def test_the_new_entries_are_the_restatement_bit_for_bit(ctx, name):
    """From column 1 of a two-column transient state (reached by steps from a steady state): s, the face means and d, against
    coupled_ref.scale on the downloaded state, and against padne_coupled_update fed that state from the host; twice, so that
    d is taken against kept means.  Then a slot of a reserved table from a block solved on the revalued system: the load of
    the restatement on the block's own potentials, the other slots exact zeros, the per-mesh heat the bits of
    padne_thermal_report's after padne_coupled_solve_kkt and math.fsum's value to rounding; the range of the used scale.
    Last, a slot rewritten while a schedule is under way: clock and state untouched, the next right-hand side takes it."""
    ambient, t0 = 31.0, 20.0
    with Stepping(name) as dev:
        alpha, sigma = alphas(dev), sigma_of(dev)
        dev.loaded(2, seed=21)
        coupled = _hip.Coupled(dev.L.dev, dev.thermal, alpha, ambient, t0)
        try:
            dev.tr.start([None, 1])
            got, thetas = [], []
            for _ in range(2):
                dev.tr.run(DT2, 2, [0, 0])
                thetas.append(dev.tr.state()[1])
                d = coupled.update_transient(dev.tr, 1)
                got.append((d, *coupled.get_scale(dev.n_tri, means=True)))
            d_col0 = coupled.update_transient(dev.tr, 0)
            mean_col0 = coupled.get_scale(dev.n_tri, means=True)[1]
            theta_col0 = dev.tr.state()[0]
            # the slot of a reserved table
            coupled.update_transient(dev.tr, 1)
            coupled.revalue()
            s_used = coupled.get_scale(dev.n_tri, used=True)
            lo, hi = coupled.scale_range()
            plan, V = finished_block(dev.board, dev.L, dev.cases)
            try:
                rng = np.random.default_rng(22)
                nodes = rng.integers(0, dev.n_pot, 6)
                nodes[:2] = nodes[0]
                heat = (nodes, np.zeros(6, dtype=np.int32), rng.uniform(0.0, 1e-2, 6))
                dev.tr.reserve_loads(3)
                mesh_heat = coupled.transient_load(dev.tr, plan, 1, heat)
                table = dev.tr.load_vectors()
                coupled.solve_kkt(plan, heat)
                report_heat = dev.thermal.report(1, dev.n_tri, dev.n_vert, fields=False, envelope=False)[3][0]
                # under way: another load into slot 0 between two steps
                dev.tr.start([None, 1])
                dev.tr.run(DT1, 2, [1, 1])
                clock, state = dev.tr.clock(), dev.tr.state()
                again = coupled.transient_load(dev.tr, plan, 0, None)
                assert dev.tr.clock() == clock and np.array_equal(dev.tr.state(), state)
                table_after, rhs = dev.tr.load_vectors(), dev.tr.rhs(DT1, [0, None])
            finally:
                plan.close()
            coupled.reset()                                # the same state from the host, against means of 0 again
            d_host = coupled.update(thetas[0])
            s_host, mean_host = coupled.get_scale(dev.n_tri, means=True)
        finally:
            coupled.close()
    prev = np.zeros(dev.n_tri)
    for theta, (d, s, mean) in zip(thetas, got):
        s_want, mean_want = C.scale(dev.tri, dev.face_mesh, alpha, ambient, t0, theta)
        assert np.array_equal(mean, mean_want) and np.array_equal(s, s_want) and d == np.abs(mean_want - prev).max()
        prev = mean_want
    assert np.abs(thetas[1]).max() > 0.0 and got[1][0] > 0.0
    assert d_host == got[0][0] and np.array_equal(s_host, got[0][1]) and np.array_equal(mean_host, got[0][2])
    mean_want = C.face_means(dev.tri, theta_col0)
    assert np.array_equal(mean_col0, mean_want) and d_col0 == np.abs(mean_want - prev).max()
    assert np.array_equal(s_used, got[1][1]) and (lo, hi) == (s_used.min(), s_used.max()) and lo < hi
    Pf = C.face_power(dev.xy, dev.tri, dev.face_mesh, sigma, s_used, V[:dev.n_vert, 0])
    want = T.load(dev.n_pot, dev.tri, Pf, [(int(n), float(v)) for n, v in zip(heat[0], heat[2])])
    assert np.array_equal(table[1], want) and (table[[0, 2]] == 0.0).all() and np.abs(want).max() > 0.0
    assert np.array_equal(mesh_heat, report_heat) and np.array_equal(again, mesh_heat)
    for m in range(len(dev.flat)):
        exact = math.fsum(Pf[dev.toff[m]:dev.toff[m + 1]].tolist())
        assert abs(mesh_heat[m] - exact) <= 1e-12 * abs(exact)
    assert np.array_equal(table_after[0], T.load(dev.n_pot, dev.tri, Pf)) and np.array_equal(table_after[1:], table[1:])
    _A, _hM, Cv = dev.host()
    assert np.array_equal(rhs[0], R.rhs(Cv, DT1, state[0], table_after[0])) and np.array_equal(rhs[1], R.rhs(Cv, DT1, state[1]))


# ---- 3. every step against direct stepping ---------------------------------------------------------------------------------

def one_step_segments(schedule):
    return [solver.Segment(dt, 1, case) for dt, steps, case in schedule for _ in range(steps)]


@pytest.mark.parametrize("name", sorted(C.COUPLED_BOARDS))
def test_trajectory_against_the_host_reference(ctx, name):
    """test_transient.SCHEDULE (on for 12 steps, on for 12 of another dt, off for 16) on the coupled boards: every step's
    theta within BAR = 1e-8 of the run's largest |theta| of the restatement, the bar and the argument of
    test_transient.test_trajectory_against_the_host_reference -- a step's error is at most cond(S) rtol ||theta||, old errors
    decay, and the lagged scale moves the load by alpha times the error of theta, far below.  The probed potentials within
    1e-8 of the largest |V|."""
    film, factor = C.COUPLED_BOARDS[name]
    prob, meshes, layer_of, disc, *_ = board(name)
    case = C.scaled_case(prob, factor)
    model = model_of(film)
    nodes = [conn.node_id for conn in prob.networks[0].connections][:3]
    _sols, rep, trace = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, model,
                              one_step_segments(TR.SCHEDULE), cases=[case], voltage_probes=nodes, keep="segments",
                              disconnected_meshes_by_layer=disc)
    B = C.host_board(prob, meshes, layer_of, model.electrothermal, case)
    want = CT.run(B, [CAP] * len(meshes), [(dt, steps, j is not None) for dt, steps, j in TR.SCHEDULE])
    assert len(rep.temperatures) == 40 and want.states.shape[0] == 41
    top = np.abs(want.states).max()
    err = [np.abs(in_mesh_order(fields, layer_of) - 25.0 - want.states[n + 1, :B.n_vert]).max()
           for n, fields in enumerate(rep.temperatures)]
    print(name, "worst error / max|theta|", max(err) / top, "max theta", top, "increments", trace.increments[1:4])
    assert top > 10.0 and max(err) <= BAR * top
    index = solver.index_board(prob, meshes, layer_of, None, disc).node_indexer.node_to_global_index
    v_top = max(np.abs(V).max() for V in want.V if V is not None)
    for node in nodes:
        for n, V in enumerate(want.V):
            if V is None:
                assert np.isnan(trace.potentials[node][n])
            else:
                assert abs(trace.potentials[node][n] - V[index[node]]) <= 1e-8 * v_top
    on = ~np.isnan(want.increments)
    assert np.array_equal(np.isnan(trace.increments), ~on)
    assert np.abs(trace.increments[on] - want.increments[on]).max() <= BAR * top
    assert np.abs(trace.scale_min[on][1:] - want.scale_min[on][1:]).max() <= 3.93e-3 * BAR * top


# ---- 4. the strip through the Problem API ----------------------------------------------------------------------------------

LEGS = [(TAU / 4, 8, 0), (TAU / 8, 4, None), (10 * TAU, 30, 0)]


def strip_run(alpha_theta0, legs=LEGS, **kw):
    prob, meshes, layer_of = strip_problem(alpha_theta0)
    _sols, rep, trace = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, model_of(ambient=20.0),
                              one_step_segments(legs), **kw)
    return (prob, meshes, layer_of), rep, trace


def test_the_uniform_strip_follows_the_scalar_recurrence(ctx):
    """alpha theta0 = 0.3: the hotspot of every step within BAR * fixed of the recurrence; after the 30 steps of 10 tau every
    vertex within 1e-6 * 0.3 / 0.7 + BAR * fixed of solve_meshed_electrothermal at a tolerance of 1e-6 K (its own gap from
    the fixed point; the transient's remainder is 0.364^30 of the gap)."""
    (prob, meshes, layer_of), rep, trace = strip_run(0.3)
    want, _ = CT.strip_recurrence(0.3, CAP, [(dt, n, j is not None) for dt, n, j in LEGS])
    fixed = C.strip_closed_form(0.3, 1)[2]
    hot = np.array([spot[0] for spot in rep.hotspots[0]]) - 20.0
    print("worst hotspot error / fixed", np.abs(hot - want).max() / fixed, "end", hot[-1], "fixed", fixed)
    assert len(hot) == 43 and np.abs(hot - want).max() <= BAR * fixed
    electro = solver.ElectroThermalModel(thermal=solver.ThermalModel(film=FILM, ambient=20.0), tolerance=1e-6)
    _sol, steady, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, electro)
    assert coupling.converged
    end, held = rep.temperatures[-1][0][0].values, steady.temperatures[0][0].values
    assert np.abs(end - held).max() <= 1e-6 * 0.3 / 0.7 + BAR * fixed


# ---- 5. the balance of every step ------------------------------------------------------------------------------------------

EXTRAS = {"two_layer": dict(interlayer={("F.Cu", "B.Cu"): 1.5e-3}),
          "single": dict(heat_sources=[solver.HeatSource.rectangle("F.Cu", 3.0, 3.0, 5.0, 5.0, 0.01, name="U1")])}


@pytest.mark.parametrize("name", BOARDS)
def test_every_step_balances_against_its_own_electrical_solve(ctx, name):
    """(stored' - stored) / dt + loss' - total_heat' within 1e-9 of the run's largest heat (the one-way balance test's bar),
    total_heat the heat of that step's electrical solve; and total_heat within 1e-9 relative of what the sources deliver in
    that solve plus the component heat.  ``two_layer`` conducts between its layers, ``single`` carries a component."""
    film, factor = ALL_BOARDS[name]
    prob, meshes, layer_of, disc, *_ = board(name)
    schedule = [solver.Segment(4 * DT1, 4, 0), solver.Segment(3 * DT2, 3, 0), solver.Segment(3 * DT2, 3, None)]
    _sols, rep, trace = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of,
                              model_of(film, thermal=EXTRAS.get(name)), schedule, cases=[C.scaled_case(prob, factor)],
                              disconnected_meshes_by_layer=disc)
    component = 0.01 if name == "single" else 0.0
    defect = (rep.total_stored[1:] - rep.total_stored[:-1]) / np.diff(rep.times) + rep.total_loss[1:] - rep.total_heat[1:]
    top = rep.total_heat.max()
    gap = np.abs(rep.total_heat[1:8] - (trace.delivered[1:8] + component))
    print(name, "largest heat", top, "worst defect / heat", np.abs(defect).max() / top, "heat against delivered",
          (gap / trace.delivered[1:8]).max(), "heat of the first and last on step", rep.total_heat[1], rep.total_heat[7])
    assert top > 0 and (np.abs(defect) <= 1e-9 * top).all()
    assert (trace.delivered[1:8] > 0).all() and (gap <= 1e-9 * (trace.delivered[1:8] + component)).all()
    assert (rep.total_heat[8:] == 0.0).all() and (trace.delivered[8:] == 0.0).all() and rep.total_heat[0] == 0.0
    assert len(set(rep.total_heat[1:8].tolist())) == 7     # every step has its own heat
    copper = sum(layer["heat"] for layer in rep.layers)     # the layers' parts: the copper's share of the heat
    assert (copper[1:8] > 0).all() and (copper <= rep.total_heat * (1 + 1e-12)).all() and (copper[8:] == 0.0).all()


# ---- 6. the direction of the effect ----------------------------------------------------------------------------------------

def hottest(rep):
    return np.array([max(spots[n][0] for spots in rep.hotspots if spots[n] is not None) for n in range(len(rep.times))])


@pytest.mark.parametrize("name, sign", [("single", 1), ("problem_mixed", -1)])
def test_warm_copper_dissipates_more_under_a_current_and_less_under_a_voltage(ctx, name, sign):
    """``single`` is current-driven: the heat and the hotspot of every on step are at least the one-way run's and strictly
    greater at the end.  ``problem_mixed`` holds voltages: its heat ends lower."""
    film, factor = C.COUPLED_BOARDS[name]
    prob, meshes, layer_of, disc, *_ = board(name)
    schedule = [solver.Segment(6 * TAU, 6, 0)]
    kw = dict(cases=[C.scaled_case(prob, factor)], disconnected_meshes_by_layer=disc)
    _s, cold = quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, TR.model_of(film), schedule, **kw)
    _s, warm, _trace = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, model_of(film), schedule, **kw)
    print(name, "heat", cold.total_heat[-1], "->", warm.total_heat[-1], "hotspot", hottest(cold)[-1], "->", hottest(warm)[-1])
    if sign > 0:
        assert (warm.total_heat[1:] >= cold.total_heat[1:]).all() and (hottest(warm)[1:] >= hottest(cold)[1:]).all()
        assert warm.total_heat[-1] > cold.total_heat[-1] and hottest(warm)[-1] > hottest(cold)[-1]
    else:
        assert warm.total_heat[-1] < cold.total_heat[-1]


# ---- 7. no steady state ----------------------------------------------------------------------------------------------------

def test_the_strip_without_a_steady_state_runs_and_stop_above_names_the_step(ctx):
    """alpha theta0 = 1.2, where solve_meshed_electrothermal raises ThermalRunawayError: the transient runs, its hotspot
    follows the recurrence, and with stop_above = 400 the run ends at the step the recurrence names, every array with it."""
    legs = LEGS[:2] + [(10 * TAU, 3, 0)]
    on = [(dt, n, j is not None) for dt, n, j in legs]
    _board, rep, trace = strip_run(1.2, legs)
    want, _ = CT.strip_recurrence(1.2, CAP, on)
    hot = np.array([spot[0] for spot in rep.hotspots[0]]) - 20.0
    print("hotspot at the end", hot[-1] + 20.0)
    assert trace.stopped is None and len(hot) == 16 and np.abs(hot - want).max() <= BAR * want.max()
    cut, step = CT.strip_recurrence(1.2, CAP, on, stop_above=400.0)
    _board, rep, trace = strip_run(1.2, legs, stop_above=400.0, probes=[], keep="end")
    assert step is not None and len(rep.times) == step + 1 == len(cut)
    for a in trace_arrays(trace)[:4] + [rep.total_heat, rep.total_stored, rep.total_loss, rep.layers[0]["heat"]]:
        assert len(a) == step + 1
    assert len(trace.iterations) == step + 1 and len(rep.hotspots[0]) == step + 1 and len(rep.info["iterations_per_step"]) == step
    when, temperature, layer_i, mesh_i, vertex, x, y = trace.stopped
    assert when == rep.times[-1] and layer_i == 0 and mesh_i == 0
    assert temperature == rep.hotspots[0][-1][0] > 400.0 >= rep.hotspots[0][-2][0]
    assert (vertex, x, y) == rep.hotspots[0][-1][2:] and rep.snapshot_times == [rep.times[-1]]
    assert rep.temperatures[-1][0][0].values.max() == temperature


# ---- 8. a start from the steady state --------------------------------------------------------------------------------------

def test_initial_case_starts_from_the_steady_electrothermal_state_and_stays_there(ctx):
    """``single`` at a tolerance of 1e-6 K: the start's hotspot is solve_meshed_electrothermal's within BAR of the rise, and four
    steps of tau under the same case keep every vertex within the loop's own gap, tolerance * rho / (1 - rho) with rho < 0.5
    (coupled_ref measures 0.10), plus BAR of the rise."""
    film, factor = C.COUPLED_BOARDS["single"]
    prob, meshes, layer_of, disc, *_ = board("single")
    case = C.scaled_case(prob, factor)
    model = model_of(film, initial=0, tolerance=1e-6)
    _s, steady, couplings, _e = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model.electrothermal, cases=[case])
    sols, rep, trace = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, model,
                             one_step_segments([(TAU, 4, 0)]), cases=[case], keep="segments")
    want = steady[0].temperatures[0][0].values
    rise = want.max() - 25.0
    drift = max(np.abs(fields[0][0].values - want).max() for fields in rep.temperatures)
    print("rise", rise, "start hotspot", rep.hotspots[0][0][0], "steady", steady[0].hotspots[0][0], "drift", drift,
          "initial increment", trace.increments[0], "rounds' iterations", trace.iterations[0])
    assert couplings[0].converged and rise > 10.0
    assert abs(rep.hotspots[0][0][0] - steady[0].hotspots[0][0]) <= BAR * rise
    assert trace.increments[0] <= 1e-6 and trace.increments[1] == 0.0
    assert drift <= 1e-6 + BAR * rise
    # both loops stop within 1e-6 K of the fixed point, and the heat moves by alpha per kelvin
    assert abs(rep.total_heat[0] - steady[0].total_heat) <= (3.93e-3 * 1e-6 + 1e-9) * steady[0].total_heat
    assert sols[0] is not None and trace.scale_max[0] < 1.0


def test_the_initial_loop_reports_runaway_and_non_convergence_like_the_steady_call(ctx):
    """``initial=0`` on the strip at alpha theta0 = 1.2 raises ThermalRunawayError after round 4, as solve_meshed_electrothermal
    does; with ``max_rounds=1`` on a coupled board the run goes on from the unconverged state with a SolverWarning."""
    prob, meshes, layer_of = strip_problem(1.2)
    with pytest.raises(solver.ThermalRunawayError, match="F.Cu") as info:
        quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, model_of(ambient=20.0, initial=0),
              [solver.Segment(TAU, 1, 0)])
    assert "rounds 1 to 4" in str(info.value)
    film, factor = C.COUPLED_BOARDS["single"]
    prob, meshes, layer_of, *_ = board("single")
    with pytest.warns(solver.SolverWarning, match="did not converge in 1 round"):
        _s, rep, trace = solver.solve_meshed_electrothermal_transient(prob, meshes, layer_of, model_of(film, initial=0, max_rounds=1),
                                                                      [solver.Segment(TAU, 1, 0)], cases=[C.scaled_case(prob, factor)])
    assert trace.increments[0] > 1.0 and len(rep.times) == 2 and trace.iterations[0]["electrical"] > 0


# ---- 9. bits and guards ----------------------------------------------------------------------------------------------------

def driver(name="two_layer"):
    film, factor = C.COUPLED_BOARDS[name]
    prob, meshes, layer_of, disc, *_ = board(name)
    nodes = [conn.node_id for conn in prob.networks[0].connections][:2]
    schedule = [solver.Segment(3 * DT1, 3, 0), solver.Segment(2 * DT2, 2, None), solver.Segment(2 * DT2, 2, 0)]
    return solver.solve_meshed_electrothermal_transient(prob, meshes, layer_of, model_of(film), schedule,
                                                        cases=[C.scaled_case(prob, factor)], probes=nodes, voltage_probes=nodes,
                                                        keep="segments", disconnected_meshes_by_layer=disc)


def test_two_calls_give_the_same_bits(ctx):
    (_sa, rep_a, trace_a), (_sb, rep_b, trace_b) = quiet(driver), quiet(driver)
    (arrays_a, scalars_a), (arrays_b, scalars_b) = everything(rep_a), everything(rep_b)
    assert scalars_a == scalars_b and same(arrays_a, arrays_b) and same(trace_arrays(trace_a), trace_arrays(trace_b))
    assert trace_a.increments[2] > 0.0


def test_solve_electrothermal_transient_meshes_the_board_once(ctx):
    """The call that meshes: the bits of the meshed call on the mesh it was given, ``timings`` with a lap dict per step."""
    film, factor = C.COUPLED_BOARDS["single"]
    prob, meshes, layer_of, *_ = board("single")

    class OneMesh:
        def poly_to_mesh(self, polygon, seed_points):
            return meshes[0]

    schedule = [solver.Segment(3 * DT1, 3, 0), solver.Segment(2 * DT2, 2, None)]
    case = C.scaled_case(prob, factor)
    timings: dict = {}
    _s, want, trace_want = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, model_of(film), schedule,
                                 cases=[case], keep="none", timings=timings)
    sols, rep, trace = quiet(solver.solve_electrothermal_transient, prob, model_of(film), schedule, mesher=OneMesh(), cases=[case],
                             keep="none")
    assert same(everything(rep)[0], everything(want)[0]) and same(trace_arrays(trace), trace_arrays(trace_want))
    assert rep.temperatures == [] and sols[0] is not None and len(rep.times) == 6
    assert [sorted(k for k in lap if k not in ("step", "case")) for lap in timings["steps"]] == \
        [sorted(["scale", "revalue", "stage1", "stage2", "load", "thermal_step"])] * 3 + [["thermal_step"]] * 2


def test_the_public_call_under_the_guarded_pool(ctx, switches):
    three_ways(ctx, switches, lambda: driver("single"))


def test_refusals_of_the_device_entries(ctx):
    """Each returns PADNE_E_INVALID (a ValueError here) and leaves the handles usable: at the end they step to the bits of
    fresh handles."""
    lib = ctx._lib

    def stepped(dev, coupled):
        dev.tr.reserve_loads(2)
        dev.tr.start([None, None])
        coupled.reset()
        out = []
        for _ in range(2):
            d = coupled.update_transient(dev.tr, 0)
            coupled.revalue()
            plan, _V = finished_block(dev.board, dev.L, dev.cases)
            try:
                heat = coupled.transient_load(dev.tr, plan, 1, None)
            finally:
                plan.close()
            out += [d, heat, dev.tr.run(DT1, 1, [1, None])["max"], dev.tr.state()]
        return out

    with Stepping("two_layer") as dev, Stepping("single") as other:
        coupled = _hip.Coupled(dev.L.dev, dev.thermal, alphas(dev), 25.0, 20.0)
        foreign = _hip.Context(0)
        try:
            with pytest.raises(ValueError):                # before a start
                coupled.update_transient(dev.tr, 0)
            plan, _V = finished_block(dev.board, dev.L, dev.cases)
            plan_other, _V = finished_block(other.board, other.L, other.cases)
            plan_two, _V = finished_block(dev.board, dev.L, solver.check_load_cases(dev.prob, [{}, {}]))
            try:
                with pytest.raises(ValueError):            # no table yet
                    coupled.transient_load(dev.tr, plan, 0, None)
                for n_case in (0, -1, 4097):
                    with pytest.raises(ValueError):
                        dev.tr.reserve_loads(n_case)
                dev.tr.reserve_loads(2)
                other.tr.reserve_loads(1)
                dev.tr.start([None, None])
                other.tr.start([None])
                for col in (-1, 2):
                    with pytest.raises(ValueError):
                        coupled.update_transient(dev.tr, col)
                with pytest.raises(ValueError):            # a transient handle on another thermal handle
                    coupled.update_transient(other.tr, 0)
                with pytest.raises(ValueError):
                    coupled.transient_load(other.tr, plan, 0, None)
                for slot in (-1, 2):
                    with pytest.raises(ValueError):
                        coupled.transient_load(dev.tr, plan, slot, None)
                for bad in (plan_other, plan_two):         # another system's block, and a block of two columns
                    with pytest.raises(ValueError):
                        coupled.transient_load(dev.tr, bad, 0, None)
                for heat in (([dev.n_pot], [0], [1.0]), ([0], [1], [1.0]), ([0], [0], [float("inf")])):
                    with pytest.raises(ValueError):
                        coupled.transient_load(dev.tr, plan, 0, heat)
                d, lo = ctypes.c_double(), ctypes.c_double()
                out = np.zeros(dev.tr.n_mesh)
                ptr = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
                null = _hip._P()
                assert lib.padne_coupled_update_transient(ctx._h, null, dev.tr._h, 0, ctypes.byref(d)) == _hip.E_INVALID
                assert lib.padne_coupled_update_transient(ctx._h, coupled._h, null, 0, ctypes.byref(d)) == _hip.E_INVALID
                assert lib.padne_coupled_update_transient(ctx._h, coupled._h, dev.tr._h, 0, None) == _hip.E_INVALID
                assert lib.padne_coupled_update_transient(foreign._h, coupled._h, dev.tr._h, 0, ctypes.byref(d)) == _hip.E_INVALID
                assert lib.padne_coupled_transient_load(foreign._h, coupled._h, dev.tr._h, plan._h, 0, 0, None, None, None,
                                                        dev.tr.n_mesh, ptr) == _hip.E_INVALID
                assert lib.padne_coupled_transient_load(ctx._h, coupled._h, dev.tr._h, null, 0, 0, None, None, None,
                                                        dev.tr.n_mesh, ptr) == _hip.E_INVALID
                assert lib.padne_coupled_transient_load(ctx._h, coupled._h, dev.tr._h, plan._h, 0, 0, None, None, None,
                                                        dev.tr.n_mesh + 1, ptr) == _hip.E_INVALID
                assert lib.padne_coupled_transient_load(ctx._h, coupled._h, dev.tr._h, plan._h, 0, 0, None, None, None,
                                                        dev.tr.n_mesh, None) == _hip.E_INVALID
                assert lib.padne_transient_reserve_loads(foreign._h, dev.tr._h, 2) == _hip.E_INVALID
                assert lib.padne_transient_reserve_loads(ctx._h, null, 2) == _hip.E_INVALID
                assert lib.padne_coupled_scale_range(foreign._h, coupled._h, ctypes.byref(d), ctypes.byref(lo)) == _hip.E_INVALID
                assert lib.padne_coupled_scale_range(ctx._h, coupled._h, None, ctypes.byref(lo)) == _hip.E_INVALID
                assert dev.tr.clock()[0] == 0 and (dev.tr.load_vectors() == 0.0).all() and (dev.tr.state() == 0.0).all()
            finally:
                for p in (plan, plan_other, plan_two):
                    p.close()
            # a state at which the conductance model does not hold: the message of the steady path
            cold = -400.0 * FILM * T.face_area(dev.xy, dev.tri)
            dev.tr.loads(cold[None, :])
            dev.tr.start([0])
            with pytest.raises(ValueError, match="1 \\+ alpha \\(T - T0\\) is not finite and positive on face"):
                coupled.update_transient(dev.tr, 0)
            got = stepped(dev, coupled)
        finally:
            coupled.close()
            foreign.close()
        fresh = _hip.Transient(dev.thermal, dev.capacity)
        coupled = _hip.Coupled(dev.L.dev, dev.thermal, alphas(dev), 25.0, 20.0)
        kept, dev.tr = dev.tr, fresh
        try:
            want = stepped(dev, coupled)
        finally:
            dev.tr = kept
            coupled.close()
            fresh.close()
    assert same(got, want) and got[-1].max() > 0.0 and got[4] > 0.0

"""The adaptive transient on the device against the host restatement (tests/sdirk_ref.py, itself checked by
tests/test_adaptive_transient_host.py): the extrapolation and the error estimate bit for bit; stage 1 as the backward-Euler
step it is; a trial that leaves the handle alone and an accepted one that becomes the state, with the folds of its report
held to tests/fold_ref.py; the trajectory and the decisions of the step-size rule against direct stepping; the public call's
balance, times and hierarchies; the closed form of uniform heating; scenarios in lockstep; the accuracy against backward
Euler at equal cost; bitwise repeatability and the guarded pool.

Boards: those of tests/test_transient.py -- ``grid49`` for meshes of several tiles and a real hierarchy, ``two_layer`` for two
meshes and an internal node."""
import math

import numpy as np
import pytest

import fold_ref as F
import sdirk_ref as SR
import thermal_ref as T
import transient_ref as R
import test_thermal as TT
from padne_amd import _hip, solver
from test_coupled_transient import EXTRAS
from test_device_memory import three_ways
from test_thermal import BAR, quiet, random_loads
from test_transient import CAP, DT1, FILM, GRID49, TAU, Stepping, board, everything, model_of

pytestmark = pytest.mark.gpu

NEG_INF = (-np.inf, F.NO_INDEX)
GAMMA = SR.GAMMA


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def trial_arrays(tr):
    return tr.state(), tr.trial(0), tr.trial(1), tr.trial(2)


# ---- 1. the extrapolation and the estimate, bit for bit ---------------------------------------------------------------------

@pytest.mark.parametrize("name", [GRID49, "two_layer"])
@pytest.mark.parametrize("cols", [1, 3])
def test_extrapolation_and_estimate_are_the_restatement_bit_for_bit(ctx, name, cols):
    """After two ordinary steps, one trial: theta*, err and its vertex computed in numpy from the downloaded theta_n, theta_1
    and theta_{n+1} are the device's, bit for bit; internal nodes of theta* are theta_1's.  With three columns the last one
    is off since its ambient start: theta_1 = theta_n there, err exactly 0.0 at the lowest vertex."""
    initial, first, then = [None, 0, None][:cols], [0, 1, None][:cols], [1, None, None][:cols]
    with Stepping(name) as dev:
        dev.loaded(2, seed=21)
        dev.tr.start(initial)
        dev.tr.run(DT1, 2, first)
        out = dev.tr.try_step(4 * DT1, then)
        theta_n, theta_1, star, theta_new = trial_arrays(dev.tr)
    want_star = SR.extrapolate(theta_n, theta_1, dev.n_vert)
    assert np.array_equal(star, want_star) and np.array_equal(star[:, dev.n_vert:], theta_1[:, dev.n_vert:])
    assert not np.array_equal(star[0, :dev.n_vert], theta_1[0, :dev.n_vert])
    est = SR.estimate(theta_n, theta_1, star, theta_new, dev.n_vert)
    for c in range(cols):
        err, vertex = SR.error_of(est[c])
        print(name, "column", c, "err", out["err"][c], "at", out["vertex"][c])
        assert out["err"][c] == err and out["vertex"][c] == vertex
        # the same through the device's own order: tiles of 256 per mesh, then the meshes in ascending order
        best = (0.0, -1)
        for m in range(len(dev.voff) - 1):
            v0, v1 = int(dev.voff[m]), int(dev.voff[m + 1])
            top = F.mesh_top(np.abs(est[c, v0:v1]), np.arange(v0, v1), empty=NEG_INF)
            if v1 > v0 and (best[1] < 0 or top[0] > best[0]):
                best = top
        assert (out["err"][c], out["vertex"][c]) == best
    assert out["err"][0] > 0.0
    if cols == 3:
        assert np.array_equal(theta_1[2], theta_n[2]) and out["err"][2] == 0.0 and not np.signbit(out["err"][2])
        assert out["vertex"][2] == 0


# ---- 2. stage 1 is a backward-Euler step ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [GRID49, "two_layer"])
def test_stage_one_has_the_bits_of_a_backward_euler_step(ctx, name):
    """theta_1 of a trial of length dt = one step of padne_transient_run of length fl(gamma dt) from the same state on a
    second handle."""
    dt = 3 * DT1
    with Stepping(name) as dev:
        Pf, heat = random_loads(dev, 2, seed=22)
        other = _hip.Transient(dev.thermal, dev.capacity)
        try:
            for tr in (dev.tr, other):
                tr.loads(Pf, heat)
                tr.start([None, 1])
                tr.run(DT1, 2, [0, 1])
            assert np.array_equal(dev.tr.state(), other.state())
            dev.tr.try_step(dt, [1, None])
            theta_1 = dev.tr.trial(0)
            other.run(GAMMA * dt, 1, [1, None])
            want = other.state()
        finally:
            other.close()
    assert np.array_equal(theta_1, want) and np.abs(theta_1).max() > 0.0


# ---- 3. a trial changes nothing, an accepted one becomes the state ----------------------------------------------------------

def handle_snapshot(dev):
    env, env_step = dev.tr.envelope(dev.n_vert)
    return [dev.tr.state(), env, env_step, dev.tr.load_vectors()], dev.tr.clock()


@pytest.mark.parametrize("name", [GRID49, "two_layer"])
def test_a_trial_leaves_the_handle_alone_and_an_accepted_one_becomes_the_state(ctx, name):
    """State, envelope, its steps, clock and load table are bit for bit the same after a trial.  After ``accept`` the state has
    the trial's bits, the clock has advanced by one step and dt, the envelope follows the sequential rule along the states,
    and per column and mesh the report's maximum, stored heat and film loss and the stage's film loss are tests/fold_ref.py's
    on the downloaded vectors, bit for bit."""
    dt = 2 * DT1
    with Stepping(name) as dev:
        dev.loaded(2, seed=23)
        _A, hM, Cv = dev.host()
        dev.tr.start([None, 0, None])
        dev.tr.run(DT1, 1, [0, None, None])
        before, clock = handle_snapshot(dev)
        dev.tr.try_step(dt, [0, 1, None])
        after, clock_after = handle_snapshot(dev)
        # (the third entry of the clock counts the hierarchies built for S: the trial's matrix needed one)
        assert clock_after[:2] == clock[:2] and all(np.array_equal(a, b) for a, b in zip(before, after))
        _n, theta_1, _star, theta_new = trial_arrays(dev.tr)
        probes = np.array([0, dev.n_pot - 1], dtype=np.int64)
        out = dev.tr.accept(probes)
        state = dev.tr.state()
        env, env_step = dev.tr.envelope(dev.n_vert)
        step, time, _h = dev.tr.clock()
        with pytest.raises(ValueError):                    # the trial is spent
            dev.tr.accept()
    assert np.array_equal(state, theta_new) and np.array_equal(out["probes"], state[:, probes])
    assert step == clock[0] + 1 == 2 and time == clock[1] + dt
    for c in range(3):
        # the envelope before the trial is that of the start and the first step; the accepted state joins as step 2
        greater = state[c, :dev.n_vert] > before[1][c]
        assert np.array_equal(env[c], np.where(greater, state[c, :dev.n_vert], before[1][c]))
        assert np.array_equal(env_step[c], np.where(greater, 2, before[2][c]))
        for m in range(len(dev.voff) - 1):
            v0, v1 = int(dev.voff[m]), int(dev.voff[m + 1])
            assert out["stored"][c, m] == F.mesh_sum(Cv[v0:v1] * state[c, v0:v1]), (c, m)
            assert out["loss"][c, m] == F.mesh_sum(hM[v0:v1] * state[c, v0:v1]), (c, m)
            assert out["stage_loss"][c, m] == F.mesh_sum(hM[v0:v1] * theta_1[c, v0:v1]), (c, m)
            assert (out["max"][c, m], out["vertex"][c, m]) == F.mesh_top(state[c, v0:v1], np.arange(v0, v1), empty=NEG_INF)
    assert (env_step[0] == 2).any() and (out["stage_loss"][0] > 0).all() and (out["stage_loss"][2] == 0.0).all()


def test_what_ends_a_trial_and_what_the_entries_refuse(ctx):
    """``accept`` and ``trial`` are PADNE_E_INVALID (a ValueError here) without a live trial: before any, after a second
    ``accept``, and after ``run``, ``start``, ``loads`` and ``reserve_loads``; a second ``try_step`` replaces the trial.  A trial
    is refused before a start, for a dt that is not finite and positive, a case out of range and an unknown guess; ``accept``
    for a probe out of range, which leaves the trial live.  At the end the handle steps to the bits of a fresh one."""
    nan, inf = float("nan"), float("inf")
    with Stepping("two_layer") as dev:
        tr = dev.tr
        Pf, heat = random_loads(dev, 2, seed=24)
        with pytest.raises(ValueError):
            tr.try_step(DT1, [None])                       # no loads, no start
        tr.loads(Pf, heat)
        tr.n_cols = 2
        for call in (lambda: tr.try_step(DT1, [0, 1]), lambda: tr.accept(), lambda: tr.trial(0)):
            with pytest.raises(ValueError):                # loads, but no start
                call()
        tr.start([None, 0])
        for call in (lambda: tr.accept(), lambda: tr.trial(2)):
            with pytest.raises(ValueError):                # a start, but no trial
                call()
        for dt in (0.0, -DT1, nan, inf, 5e-324):
            with pytest.raises(ValueError):
                tr.try_step(dt, [0, 1])
        for call in (lambda: tr.try_step(DT1, [0, 2]), lambda: tr.try_step(DT1, [-2, 0]), lambda: tr.try_step(DT1, [0, 1], guess=3),
                     lambda: tr.try_step(DT1, [0, 1], guess=-1)):
            with pytest.raises(ValueError):
                call()
        enders = [lambda: tr.run(DT1, 1, [0, 1]), lambda: tr.start([None, 0]), lambda: (tr.loads(Pf, heat), tr.start([None, 0])),
                  lambda: (tr.reserve_loads(2), tr.loads(Pf, heat), tr.start([None, 0]))]
        for ender in enders:
            tr.try_step(DT1, [0, 1])
            tr.trial(1)
            ender()
            for call in (lambda: tr.accept(), lambda: tr.trial(0)):
                with pytest.raises(ValueError):
                    call()
        tr.start([None, 0])
        tr.try_step(DT1, [0, 1])
        for bad in ([dev.n_pot], [-1]):
            with pytest.raises(ValueError):
                tr.accept(bad)
        first = tr.trial(2)
        tr.try_step(2 * DT1, [0, 1])                       # a second trial replaces the first
        second = tr.trial(2)
        tr.accept()
        got = [tr.state(), tr.run(DT1, 2, [0, 1])["max"]]
        fresh = _hip.Transient(dev.thermal, dev.capacity)
        try:
            fresh.loads(Pf, heat)
            fresh.start([None, 0])
            fresh.try_step(2 * DT1, [0, 1])
            fresh.accept()
            want = [fresh.state(), fresh.run(DT1, 2, [0, 1])["max"]]
        finally:
            fresh.close()
    assert not np.array_equal(first, second) and np.array_equal(got[0], second)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- 4. the trajectory and the decisions ------------------------------------------------------------------------------------

def device_walk(dev, spans, tolerance, first_step=None, initial=(None,)):
    """``solver.adaptive_walk`` on the handle: (states (n_steps + 1, n_cols, n_pot), the accepted steps (dt, time, cases, the
    dict of accept), every trial's err, the walk's dict)."""
    dev.tr.start(list(initial))
    states, taken, errs = [dev.tr.state()], [], []

    def try_step(dt, cases):
        errs.append(dev.tr.try_step(dt, cases)["err"].copy())
        return errs[-1]

    def accept(dt, time, cases, errors):
        out = dev.tr.accept()
        states.append(dev.tr.state())
        taken.append((dt, time, cases, out))

    walk = solver.adaptive_walk(spans, tolerance, first_step, None, 10000, try_step, accept)
    return np.stack(states), taken, errs, walk


@pytest.mark.parametrize("fraction, first_step", [(0.03, TAU / 4), (0.01, None)])
@pytest.mark.parametrize("name", ["single", "two_layer", GRID49])
def test_trajectory_and_decisions_against_the_host_reference(ctx, name, fraction, first_step):
    """On for tau, off for tau / 2, at a tolerance of 3 % of the steady rise from a first step of tau / 4 (rejections, then
    growth) and of 1 % from the default start.  The reference rule with direct solves takes its own path; the device's
    decisions are the same, every one.  That needs the reference's estimates to keep clear of the two thresholds: none lies
    within 1e-5 relative of tolerance or tolerance / 4 (the nearest on these boards is 4e-3).  Then the restated step is
    replayed from the reference's states on the device's accepted steps: every accepted state within 1e-8 of max |theta|,
    the bar of test_trajectory_against_the_host_reference."""
    with Stepping(name) as dev:
        B = dev.loaded(1, seed=5)
        A, _hM, Cv = dev.host()
        tolerance = fraction * float(T.solve(A, B[0])[:dev.n_vert].max())
        spans = [(TAU, 0), (TAU / 2, None)]
        states, taken, errs, walk = device_walk(dev, [(d, [j]) for d, j in spans], tolerance, first_step)
    want = SR.run(A, Cv, B, spans, tolerance, first_step=first_step)
    e = np.array(want["errors"])
    nearest = min(np.abs(e / tolerance - 1).min(), np.abs(e / (tolerance / 4) - 1).min())
    print(name, "trials", len(e), "rejected", want["decisions"].count("reject"), "grown", len(want["grown"]),
          "nearest estimate to a threshold, relative", nearest)
    assert nearest > 1e-5
    assert walk["decisions"] == want["decisions"]
    assert [t[0] for t in taken] == want["step_sizes"].tolist() and [t[1] for t in taken] == want["times"][1:].tolist()
    if first_step is not None:
        assert walk["rejected"] > 0 and len(want["grown"]) > 0
    # the replay on the device's accepted steps
    stepper, theta, replay = SR.Stepper(A, Cv), np.zeros(dev.n_pot), [np.zeros(dev.n_pot)]
    for dt, _time, cases, _out in taken:
        theta = stepper.step(theta, dt, None if cases[0] is None else B[cases[0]])["theta"]
        replay.append(theta)
    replay = np.stack(replay)
    scale = np.abs(replay).max()
    err = np.abs(states[:, 0] - replay).max(axis=1)
    print(name, "worst error / max|theta|", err.max() / scale, "device err against the reference's, relative",
          max(abs(float(a[0]) - b) / tolerance for a, b in zip(errs, want["errors"])))
    assert scale > 0.0 and (err <= BAR * scale).all()
    assert taken[-1][1] == TAU + TAU / 2


def test_the_guess_of_stage_two_changes_the_result_within_the_tolerance_only(ctx):
    """The three initial guesses of stage 2 on the 49 x 49 board: theta_{n+1} within 1e-8 of max |theta| of each other; the
    iterations of each are printed."""
    with Stepping(GRID49) as dev:
        dev.loaded(1, seed=5)
        dev.tr.start([None])
        dev.tr.run(DT1, 2, [0])
        ends, its = [], []
        for guess in (0, 1, 2):
            out = dev.tr.try_step(8 * DT1, [0], guess=guess)
            ends.append(dev.tr.trial(2))
            its.append(out["stage_iterations"].tolist())
    print("stage iterations for the guesses theta_1, theta*, the line to the end of the step:", its)
    scale = np.abs(ends[0]).max()
    assert all(np.abs(e - ends[0]).max() <= BAR * scale for e in ends[1:]) and all(a[0] == its[0][0] for a in its)


# ---- 5. the public call -----------------------------------------------------------------------------------------------------

def runs_of_equal(values) -> int:
    values = np.asarray(values, dtype=np.float64)
    return int(len(values) > 0) + int((values[1:] != values[:-1]).sum())


@pytest.mark.parametrize("name, extras", [("two_layer", False), ("two_layer", True), ("single", True)])
def test_the_public_call_balances_every_step_and_lands_on_the_span_ends(ctx, name, extras):
    """On, on again, off: every accepted step obeys (stored' - stored) / dt + (1 - gamma) stage_loss + gamma loss' = total_heat
    within 1e-9 of the largest heat (the bar of the fixed-step balance test); the times are increasing, hit every span's end
    and end exactly on the sum of the durations; a hierarchy per run of equal tried steps.  ``two_layer`` with and without
    conduction between its layers and with a probe on its internal node, ``single`` with a component."""
    prob, meshes, layer_of, disc, *_ = board(name)
    kw = EXTRAS[name] if extras else {}
    probes = [prob.networks[0].elements[1].b] if name == "two_layer" else []
    spans = [solver.Span(TAU / 2, 0), solver.Span(TAU / 3, 0), solver.Span(TAU / 2, None)]
    sols, rep = quiet(solver.solve_meshed_thermal_transient_adaptive, prob, meshes, layer_of, model_of(**kw), spans,
                      tolerance=0.3, first_step=TAU / 8, probes=probes, disconnected_meshes_by_layer=disc)
    info = rep.info
    n = len(info["step_sizes"])
    assert len(sols) == 1 and len(rep.times) == n + 1 and info["error_estimates"].shape == (n, 1)
    assert info["stage_loss"].shape == (n, 1) and info["stage_iterations"].shape == (n, 2)
    assert np.array_equal(info["iterations_per_step"], info["stage_iterations"].sum(axis=1))
    assert info["tried"] == n + info["rejected"] == len(info["tried_step_sizes"]) and info["rejected"] > 0
    dts = np.diff(rep.times)
    assert (dts > 0).all() and np.allclose(dts, info["step_sizes"], rtol=1e-12, atol=0.0)
    ends = [TAU / 2, TAU / 2 + TAU / 3, (TAU / 2 + TAU / 3) + TAU / 2]
    assert all(t in rep.times for t in ends) and rep.times[-1] == ends[-1] and rep.snapshot_times == [ends[-1]]
    defect = ((rep.total_stored[1:] - rep.total_stored[:-1]) / info["step_sizes"] + (1 - GAMMA) * info["stage_loss"][:, 0]
              + GAMMA * rep.total_loss[1:] - rep.total_heat[1:])
    top = rep.total_heat.max()
    print(name, kw, "steps", n, "rejected", info["rejected"], "worst balance defect / heat", np.abs(defect).max() / top,
          "hierarchies", info["hierarchies"])
    assert top > 0 and (np.abs(defect) <= 1e-9 * top).all()
    on = rep.times[1:] <= ends[1]
    assert (rep.total_heat[1:][on] == top).all() and (rep.total_heat[1:][~on] == 0.0).all()
    assert info["hierarchies"] == runs_of_equal(info["tried_step_sizes"])
    assert (info["error_estimates"] <= 0.3).all()
    if probes:
        trace = rep.probes[probes[0]]
        assert len(trace) == n + 1 and trace[0] == 25.0 and trace.max() > 25.0
    assert set(np.unique(rep.envelope.times[0][0])) <= set(rep.times)


# ---- 6. uniform heating -----------------------------------------------------------------------------------------------------

def test_uniform_heating_follows_the_product_of_the_growth_factors(ctx):
    """``single`` with its sources at zero under a footprint over the whole board: b = q M_v, every vertex follows
    theta_inf (1 - prod_i R(-h dt_i / c)) over the accepted steps, within 1e-8 of theta_inf = P / (h area)."""
    prob, meshes, layer_of, disc, flat, *_ = board("single")
    dead = {e: 0.0 for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS}
    h, power = 2e-5, 0.75
    lid = solver.HeatSource.rectangle("F.Cu", -1, -1, 9, 9, power, name="lid")
    model = solver.TransientModel(thermal=solver.ThermalModel(film=h, ambient=20.0, heat_sources=[lid]), areal_capacity=CAP)
    xy, tri, *_ = T.flatten(flat)
    theta_inf = power / (h * math.fsum(T.face_area(xy, tri).tolist()))
    _sols, rep = quiet(solver.solve_meshed_thermal_transient_adaptive, prob, meshes, layer_of, model, [solver.Span(CAP / h, 0)],
                       cases=[dead], tolerance=1e-3 * theta_inf, keep="none", disconnected_meshes_by_layer=disc)
    left = np.cumprod([SR.growth(-h * dt / CAP) for dt in rep.info["step_sizes"]])
    want = theta_inf * (1 - np.concatenate([[1.0], left]))
    hot = np.array([spot[0] for spot in rep.hotspots[0]]) - 20.0
    print("steps", len(left), "theta_inf", theta_inf, "end", hot[-1], "worst error / theta_inf", np.abs(hot - want).max() / theta_inf)
    assert len(set(rep.info["step_sizes"].tolist())) > 3 and np.abs(hot - want).max() <= BAR * theta_inf
    assert abs(rep.total_loss[-1] - power * (1 - left[-1])) <= 1e-8 * power        # h area theta


# ---- 7. scenarios in lockstep -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [GRID49, "two_layer"])
def test_scenarios_in_lockstep_are_the_scenarios_alone_on_the_same_steps(ctx, name):
    """Three scenarios (one heats, one starts from a steady state and changes its load, one stays off) under the rule, the
    largest estimate deciding; then each alone, tried and accepted on the block's accepted steps: every state within 1e-8
    of max |theta| of the column in the block, the bar of test_scenarios_in_one_block_are_the_scenarios_alone."""
    initial = [None, 0, None]
    spans = [(TAU / 2, [0, 1, None]), (TAU / 4, [None, 1, None])]
    with Stepping(name) as dev:
        B = dev.loaded(2, seed=8)
        A, _hM, _Cv = dev.host()
        tolerance = 0.02 * float(T.solve(A, B[0])[:dev.n_vert].max())
        states, taken, errs, walk = device_walk(dev, spans, tolerance, TAU / 4, initial)
        for c in range(3):
            dev.tr.start([initial[c]])
            alone, alone_err = [dev.tr.state()[0]], []
            for dt, _time, cases, _out in taken:
                alone_err.append(dev.tr.try_step(dt, [cases[c]])["err"][0])
                dev.tr.accept()
                alone.append(dev.tr.state()[0])
            alone = np.stack(alone)
            scale = np.abs(alone).max()
            print(name, "column", c, "error / max|theta|", np.abs(states[:, c] - alone).max() / max(scale, 1e-300))
            assert np.abs(states[:, c] - alone).max() <= BAR * scale
    assert walk["rejected"] > 0 and len(taken) >= 4
    assert (states[:, 2] == 0.0).all() and not np.signbit(states[:, 2]).any() and all(e[2] == 0.0 for e in errs)


# ---- 8. accuracy against backward Euler at equal cost -----------------------------------------------------------------------

def test_the_adaptive_call_is_nearer_the_fine_answer_than_backward_euler_with_as_many_solves(ctx):
    """The 49 x 49 board, tau on and tau off at 1 % of the steady rise.  The reference is the host's SDIRK2 with 512 equal
    steps per span under the restated load of the call's own potentials (as test_solve_thermal_transient_runs_a_duty_cycle
    restates it); at the end of either span the adaptive call is nearer to it than solve_meshed_thermal_transient with as many
    solves, two per tried step."""
    prob, meshes, layer_of, disc, flat, _n_internal, pairs = board(GRID49)
    _s, steady = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(film=FILM, ambient=0.0),
                           disconnected_meshes_by_layer=disc)
    tolerance = 1e-2 * float(steady.temperatures[0][0].values.max())
    sols, rep = quiet(solver.solve_meshed_thermal_transient_adaptive, prob, meshes, layer_of, model_of(ambient=0.0),
                      [solver.Span(TAU, 0), solver.Span(TAU, None)], tolerance=tolerance, keep="segments",
                      disconnected_meshes_by_layer=disc)
    tried = rep.info["tried"]
    per_span = tried                                        # 2 * tried solves in all: tried backward-Euler steps per span
    _s, euler = quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, model_of(ambient=0.0),
                      [solver.Segment(TAU, per_span, 0), solver.Segment(TAU, per_span, None)], keep="segments",
                      disconnected_meshes_by_layer=disc)
    xy, tri, face_mesh, voff, _toff = T.flatten(flat)
    V = sols[0].layer_solutions[0].potentials[0].values
    resistor = next(e for e, row in pairs if row[0] == "R")
    nodes = solver.index_board(prob, meshes, layer_of).node_indexer.node_to_global_index
    a, b = nodes[resistor.a], nodes[resistor.b]
    half = (V[a] - V[b]) ** 2 / resistor.resistance / 2
    load = T.load(len(xy), tri, T.face_power(xy, tri, face_mesh, [prob.layers[0].conductance], V), [(a, half), (b, half)])
    checked = solver.check_thermal_model(prob, solver.ThermalModel(film=FILM))
    A, M, _hM = T.operator(flat, TT.per_mesh(checked, layer_of)[0], [FILM], 0, TT.links_of(pairs, checked))
    Cv = R.capacity(voff, [CAP], M)
    fine_on = SR.uniform(A, Cv, load, TAU, 512)[-1]
    fine_off = SR.uniform(A, Cv, None, TAU, 512, fine_on)[-1]
    field = lambda r, k: r.temperatures[k][0][0].values                                   # noqa: E731
    ours = [np.abs(field(rep, 0) - fine_on).max(), np.abs(field(rep, 1) - fine_off).max()]
    theirs = [np.abs(field(euler, 0) - fine_on).max(), np.abs(field(euler, 1) - fine_off).max()]
    print("tolerance", tolerance, "steps", len(rep.info["step_sizes"]), "tried", tried, "K off the fine answer: adaptive", ours,
          "backward Euler with", per_span, "steps per span", theirs)
    assert ours[0] < theirs[0] and ours[1] < theirs[1]


# ---- 9. two calls, the same bits; the guarded pool --------------------------------------------------------------------------

def driver(name="two_layer"):
    prob, meshes, layer_of, disc, *_ = board(name)
    nodes = [conn.node_id for conn in prob.networks[0].connections][:2]
    spans = [solver.Span(TAU / 4, (0, None)), solver.Span(TAU / 8, (None, 0))]
    return solver.solve_meshed_thermal_transient_adaptive(prob, meshes, layer_of, model_of(film=TT.FILM_REAL, **EXTRAS.get(name, {})),
                                                          spans, tolerance=0.05, first_step=TAU / 16, probes=nodes, keep="segments",
                                                          disconnected_meshes_by_layer=disc)


def all_arrays(reports):
    arrays, scalars = [], []
    for rep in reports:
        a, s = everything(rep)
        arrays += a + [rep.info[key] for key in ("step_sizes", "error_estimates", "stage_loss", "stage_iterations", "tried_step_sizes")]
        scalars.append((s, rep.info["tried"], rep.info["rejected"], rep.info["hierarchies"]))
    return arrays, scalars


@pytest.mark.parametrize("name", ["two_layer", "problem_many_meshes"])
def test_two_calls_give_the_same_bits(ctx, name):
    (arrays_a, scalars_a), (arrays_b, scalars_b) = (all_arrays(quiet(driver, name)[1]) for _ in range(2))
    assert scalars_a == scalars_b
    assert len(arrays_a) == len(arrays_b) and all(np.array_equal(a, b) for a, b in zip(arrays_a, arrays_b))
    assert len(arrays_a[0]) > 3


def test_the_public_call_under_the_guarded_pool(ctx, switches):
    three_ways(ctx, switches, lambda: driver("two_layer"))

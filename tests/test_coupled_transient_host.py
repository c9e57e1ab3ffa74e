"""Host half of the transient electro-thermal solve (no GPU): the restatement of tests/coupled_transient_ref.py against answers
that are known -- the uniform strip's scalar recurrence, the discrete balance of every step, the Picard fixed point at the end
of a long leg, the strip without a steady state, the one-way stepping at alpha = 0 -- so that the device tests compare against
something that is itself checked; and the refusals of the public call, which come before the device.

The strip: coupled_ref's 9 x 9 grid, ambient = T0 = 20, film h = 1e-3, c = 3e-3 (tau = c / h = 3 s).  It stays uniform, so the
scheme is the scalar recurrence x' = ((c / dt) x + q0 (1 + alpha x)) / (c / dt + h) with q0 = h theta0."""
import math
import types

import numpy as np
import pytest

import coupled_ref as C
import coupled_transient_ref as CT
import transient_ref as R
from padne_amd import problem as P, solver, synthetic
from test_coupled_host import small_problem, strip_board

CAP = 3e-3
TAU = CAP / C.STRIP_FILM
LEGS = [(TAU / 4, 8, True), (TAU / 8, 4, False), (10 * TAU, 30, True)]


def strip_run(alpha_theta0, schedule=LEGS, **kw):
    board = strip_board(alpha_theta0)
    return board, CT.run(board, [CAP], schedule, **kw)


def test_the_uniform_strip_follows_the_scalar_recurrence():
    """alpha theta0 = 0.3, on for 8 steps of tau / 4, off for 4 of tau / 8, on for 30 of 10 tau: every vertex of every step
    within 1e-10 of the run's largest theta of the recurrence (measured 1.7e-14): the direct solves' rounding on an 81-vertex
    system of condition < 1e4 is orders below."""
    board, out = strip_run(0.3)
    want, _ = CT.strip_recurrence(0.3, CAP, LEGS)
    assert out.states.shape == (43, board.n_pot) and len(want) == 43
    worst = np.abs(out.states - want[:, None]).max() / want.max()
    print("largest deviation from the recurrence / max theta", worst, "max theta", want.max())
    assert worst <= 1e-10
    assert np.isnan(out.increments[9:13]).all() and out.increments[1] == 0.0
    # d_n is the change of the uniform state between consecutive electrical solves
    assert abs(out.increments[2] - (want[1] - want[0])) <= 1e-10 * want.max()
    assert abs(out.increments[13] - abs(want[12] - want[7])) <= 1e-10 * want.max()
    assert (out.scale_max[1:9] <= 1.0).all() and (np.diff(out.scale_min[1:9]) < 0).all()       # the copper warms: s falls


def test_every_step_balances_against_its_own_electrical_solve():
    """(stored' - stored) / dt + loss' - heat' within 1e-12 of the largest heat (measured 4e-15), heat' the sum of the step's
    load; and that sum is the power the sources deliver within 1e-12 relative (measured 8e-15): the strip has no resistors,
    so Tellegen on the revalued system gives the copper all of it."""
    board, out = strip_run(0.3)
    stored = np.array([math.fsum((out.Cv * th[:board.n_vert]).tolist()) for th in out.states])
    loss = np.array([math.fsum((board.hM * th[:board.n_vert]).tolist()) for th in out.states])
    defect = (stored[1:] - stored[:-1]) / np.diff(out.times) + loss[1:] - out.heat[1:]
    top = out.heat.max()
    on = out.delivered > 0
    print("worst balance defect / heat", np.abs(defect).max() / top, "heat against delivered",
          np.abs(out.heat[on] / out.delivered[on] - 1).max())
    assert top > 0 and (np.abs(defect) <= 1e-12 * top).all()
    assert (np.abs(out.heat[on] - out.delivered[on]) <= 1e-12 * out.delivered[on]).all()
    assert (out.heat[9:13] == 0.0).all() and on.sum() == 38
    assert (np.diff(out.heat[1:9]) > 0).all()              # a current-driven strip dissipates more as it warms


def test_the_long_leg_ends_at_the_picard_fixed_point():
    """The error against theta0 / (1 - alpha theta0) shrinks by (c / dt + q0 alpha) / (c / dt + h) = 0.364 per step of 10 tau:
    30 steps leave 7e-14 of the gap, so the state is the fixed point within the 1e-10 relative of the restatement (measured
    5e-12 K at 109 K)."""
    board, out = strip_run(0.3)
    fixed = C.strip_closed_form(0.3, 1)[2]
    ratio = (CAP / (10 * TAU) + C.STRIP_FILM * 0.3) / (CAP / (10 * TAU) + C.STRIP_FILM)
    gap = np.abs(out.states[-1] - fixed).max()
    print("fixed point", fixed, "gap", gap, "ratio", ratio, "remaining", ratio ** 30)
    assert abs(ratio - 0.364) < 1e-3 and gap <= 1e-10 * fixed


def test_the_strip_without_a_steady_state_just_gets_hotter_and_stop_above_names_the_step():
    """alpha theta0 = 1.2: no exception, the hotspot follows the recurrence (1573 K after the first two legs and three long
    steps); with stop_above the run ends at the step the recurrence names."""
    schedule = LEGS[:2] + [(10 * TAU, 3, True)]
    board, out = strip_run(1.2, schedule)
    want, _ = CT.strip_recurrence(1.2, CAP, schedule)
    hot = out.states[:, :board.n_vert].max(axis=1)
    print("hotspot after the run", hot[-1])
    assert out.stopped is None and len(hot) == 16 and 1500.0 < hot[-1] < 1650.0
    assert np.abs(hot - want).max() <= 1e-10 * want.max()
    limit = 400.0
    want_stop, step = CT.strip_recurrence(1.2, CAP, schedule, stop_above=limit)
    _board, cut = strip_run(1.2, schedule, stop_above=limit)
    assert step is not None and 1 < step < 15 and cut.stopped == step
    assert len(cut.states) == len(cut.times) == len(cut.increments) == len(cut.delivered) == step + 1
    assert cut.states[-1].max() + 20.0 > limit >= cut.states[-2].max() + 20.0
    assert np.array_equal(cut.states, out.states[:step + 1])


def test_alpha_zero_is_the_one_way_stepping_bit_for_bit():
    xy, tri = synthetic.jittered_grid(C.STRIP_N, C.STRIP_N, h=C.STRIP_H, seed=3, jitter=0.2)
    xy, tri = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    rows = [("I", 0, 80, 0.3), ("R", 10, 70, 0.05)]
    board = C.Board([(xy, tri)], [C.STRIP_SIGMA], 0, rows, 0, [0.02], [C.STRIP_FILM], [(10, 70, 0.01)], [0.0], 25.0, 20.0)
    out = CT.run(board, [CAP], LEGS)
    _V, _P, _flows, b = CT.electrical(board, np.ones(len(tri)))
    want = R.run(board.A, out.Cv, board.hM, board.voff, [b], [(dt, n, 0 if on else None) for dt, n, on in LEGS])[0]
    assert np.array_equal(out.states, want) and out.states.max() > 0.0
    assert (out.scale_min[out.delivered > 0] == 1.0).all() and (out.scale_max[out.delivered > 0] == 1.0).all()


def test_the_initial_state_is_the_picard_loops_and_a_held_case_stays_there():
    """From the converged steady state, steps under the same case stay within the loop's own gap tolerance * rho / (1 - rho)
    (rho = alpha theta0 = 0.3) plus the restatement's 1e-10 relative."""
    board, out = strip_run(0.3, [(TAU, 6, True)], initial=True, tolerance=1e-6)
    fixed = C.strip_closed_form(0.3, 1)[2]
    assert out.picard["converged"] and np.array_equal(out.states[0], out.picard["theta"])
    assert out.increments[1] == 0.0
    assert np.abs(out.states - fixed).max() <= 1e-6 * 0.3 / 0.7 + 1e-10 * fixed


# ---- the refusals of the public call: before the device --------------------------------------------------------------------

def model_of(initial=None, capacity=CAP, **kw):
    electro = solver.ElectroThermalModel(thermal=solver.ThermalModel(film=1e-5), **kw)
    return solver.ElectroThermalTransientModel(electrothermal=electro, areal_capacity=capacity, initial=initial)


ON = [solver.Segment(1.0, 2, 0)]
NAN, INF = float("nan"), float("inf")


def test_the_checked_model():
    prob, _top = small_problem()
    checked = solver.check_electrothermal_transient_model(prob, model_of(capacity={"F.Cu": 1e-3, "B.Cu": 2e-3}))
    assert checked.capacity == [1e-3, 2e-3] and checked.initial is None
    assert checked.electrothermal.alpha == [3.93e-3, 3.93e-3] and checked.electrothermal.thermal.ambient == 25.0


@pytest.mark.parametrize("model", [
    solver.TransientModel(thermal=solver.ThermalModel(film=1e-5), areal_capacity=CAP),
    solver.ElectroThermalModel(thermal=solver.ThermalModel(film=1e-5)),
    model_of(tolerance=0.0), model_of(max_rounds=0), model_of(temperature_coefficient=NAN),
    solver.ElectroThermalTransientModel(solver.ElectroThermalModel(thermal=solver.ThermalModel(film=-1.0)), CAP),
    model_of(capacity=None), model_of(capacity=-1.0), model_of(capacity=NAN), model_of(capacity={"F.Cu": 1e-3}),
    model_of(capacity={"In1.Cu": 1e-3, "F.Cu": 1e-3, "B.Cu": 1e-3}),
    model_of(initial=(0, None)), model_of(initial=[0]), model_of(initial=3), model_of(initial=-1), model_of(initial=0.5)])
def test_an_invalid_model_is_refused(model):
    prob, _top = small_problem()
    with pytest.raises(ValueError):
        solver.solve_meshed_electrothermal_transient(prob, [], [], model, ON)
    with pytest.raises(ValueError):
        solver.solve_electrothermal_transient(prob, model, ON)


@pytest.mark.parametrize("kw", [
    dict(schedule=[]), dict(schedule=[solver.Segment(-1.0, 1, 0)]), dict(schedule=[solver.Segment(1.0, 0, 0)]),
    dict(schedule=[solver.Segment(1.0, 1, 1)]), dict(schedule=solver.Segment(1.0, 1, 0)),
    dict(schedule=[solver.Segment(1.0, 1, (0, 0))]), dict(schedule=[solver.Segment(1.0, 1, (0,))]),
    dict(cases=[{object(): 1.0}]), dict(cases=[]), dict(repeat=0),
    dict(probes=[object()]), dict(probes=[P.NodeID()]), dict(voltage_probes=[object()]), dict(voltage_probes=[P.NodeID()]),
    dict(voltage_probes="node"),
    dict(keep="all"), dict(keep=None),
    dict(stop_above=NAN), dict(stop_above=INF), dict(stop_above=25.0), dict(stop_above=10.0), dict(stop_above="hot"),
    dict(partition=types.SimpleNamespace(world=2))])
def test_invalid_arguments_are_refused(kw):
    prob, _top = small_problem()
    kw = dict(kw)
    schedule = kw.pop("schedule", ON)
    with pytest.raises(ValueError):
        solver.solve_meshed_electrothermal_transient(prob, [], [], model_of(), schedule, **kw)


def test_the_refusal_of_scenarios_says_why():
    prob, _top = small_problem()
    for model, schedule in ((model_of(initial=(0, 0)), ON), (model_of(), [solver.Segment(1.0, 1, (0, None))])):
        with pytest.raises(ValueError, match="one scenario"):
            solver.solve_meshed_electrothermal_transient(prob, [], [], model, schedule)

"""Host half of the transient thermal model (no GPU): the restatement of tests/transient_ref.py against solutions and
identities that are known, so that the device tests compare against something that is itself checked; and the refusals of
``check_transient_model``, ``check_schedule`` and the public call, which come before the device."""
import math

import numpy as np
import pytest

import thermal_ref as T
import transient_ref as R
from padne_amd import problem as P, solver, synthetic
from test_thermal_host import board

KAPPA = 2.44e-8 * 293.15 * 2.0          # the Wiedemann-Franz sheet conductance of the device boards' top layer (tests/test_thermal.py)


def grid(n, width=8.0, jitter=0.2, seed=3):
    xy, tri = synthetic.jittered_grid(n, n, h=width / (n - 1), seed=seed, jitter=jitter)
    return np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int64).reshape(-1, 3)


def one_mesh(n, film, c):
    xy, tri = grid(n)
    A, M, hM = T.operator([(xy, tri)], [KAPPA], [film], 0, [])
    voff = np.array([0, len(xy)])
    return xy, tri, A, M, hM, voff, R.capacity(voff, [c], M)


def test_uniform_heating_follows_the_closed_form():
    """P_f = q A_f and no links: theta_n = (q / h) (1 - (1 + h dt / c)^-n) at every vertex, within 1e-12 relative (measured
    3e-15 on the 17 x 17 jittered grid with h = 2e-5, c = 3e-3, dt = 10, 30 steps)."""
    q, h, c, dt = 3e-4, 2e-5, 3e-3, 10.0
    xy, tri, A, _M, hM, voff, Cv = one_mesh(17, h, c)
    B = [T.load(len(xy), tri, q * T.face_area(xy, tri))]
    states, *_ = R.run(A, Cv, hM, voff, B, [(dt, 30, 0)])
    worst = 0.0
    for n in range(31):
        want = (q / h) * (1 - (1 + h * dt / c) ** -n)
        worst = max(worst, float(np.abs(states[n] - want).max()) / (q / h))
    print("relative error", worst)
    assert worst <= 1e-12


@pytest.mark.parametrize("n", [17, 49])
@pytest.mark.parametrize("film", [1e-3, 1e-5])
def test_every_step_obeys_the_discrete_balance(n, film):
    """sum Cv (theta_{n+1} - theta_n) / dt + sum hM theta_{n+1} = sum B[j] within 1e-12 of the heat (measured <= 3e-15 over
    40 steps): K annihilates constants.  On, then off (heat 0)."""
    c = 3e-3
    xy, tri, A, _M, hM, voff, Cv = one_mesh(n, film, c)
    rng = np.random.default_rng(2)
    B = [T.load(len(xy), tri, rng.uniform(0, 1e-3, len(tri)))]
    heat = math.fsum(B[0].tolist())
    dt = c / film / 20
    schedule = [(dt, 20, 0), (dt, 20, None)]
    states, _top, _vert, stored, loss, _env, _step = R.run(A, Cv, hM, voff, B, schedule)
    worst = 0.0
    for k in range(40):
        put = heat if k < 20 else 0.0
        worst = max(worst, abs((stored[k + 1, 0] - stored[k, 0]) / dt + loss[k + 1, 0] - put) / heat)
    print("worst balance defect / heat", worst)
    assert worst <= 1e-12


def test_a_long_constant_segment_tends_to_the_steady_state():
    film, c = 1e-3, 3e-3
    xy, tri, A, _M, hM, voff, Cv = one_mesh(17, film, c)
    B = [T.load(len(xy), tri, np.random.default_rng(4).uniform(0, 1e-3, len(tri)))]
    states, *_ = R.run(A, Cv, hM, voff, B, [(5 * c / film, 40, 0)])
    steady = T.solve(A, B[0])
    assert np.abs(states[-1] - steady).max() <= 1e-10 * np.abs(steady).max()      # (1 + 5)^-40 is far below


def test_halving_dt_halves_the_error():
    """First order: against a run with 64 times as many steps, the error at the end of the segment falls by a factor in
    [1.8, 2.2] per halving."""
    film, c = 1e-3, 3e-3
    xy, tri, A, _M, hM, voff, Cv = one_mesh(17, film, c)
    B = [T.load(len(xy), tri, np.random.default_rng(4).uniform(0, 1e-3, len(tri)))]
    span = c / film

    def end(steps):
        return R.run(A, Cv, hM, voff, B, [(span / steps, steps, 0)])[0][-1]

    fine = end(8 * 64)
    errors = [float(np.abs(end(s) - fine).max()) for s in (8, 16, 32)]
    rates = [a / b for a, b in zip(errors, errors[1:])]
    print("errors", errors, "rates", rates)
    assert all(1.8 <= r <= 2.2 for r in rates), rates


def test_the_envelope_keeps_the_earliest_step_of_a_tie():
    states = np.array([[1.0, 0.0, 2.0], [1.0, 3.0, 1.0], [2.0, 3.0, 2.0], [2.0, 1.0, 2.0]])
    best, step = R.envelope(states)
    assert best.tolist() == [2.0, 3.0, 2.0] and step.tolist() == [2, 1, 0]
    env, which = solver.envelope_of(states)                # the rule of envelope_of, along time
    assert np.array_equal(env, best) and np.array_equal(which, step)


def test_the_restated_step_matrix_and_right_hand_side():
    xy, tri, A, _M, _hM, _voff, Cv = one_mesh(9, 1e-3, 3e-3)
    A2 = T.operator([(xy, tri)], [KAPPA], [1e-3], 1, [(3, len(xy), 0.1)])[0]      # an internal node: no capacity
    S = R.step_matrix(A2, Cv, 0.7)
    assert np.array_equal(S.diagonal()[:len(xy)], A2.diagonal()[:len(xy)] + Cv / 0.7) and S[len(xy), len(xy)] == A2[len(xy), len(xy)]
    D = (S - A2).tocoo()
    assert (D.row == D.col).all()
    theta, b = np.arange(len(xy) + 1.0), np.full(len(xy) + 1, 0.5)
    on, off = R.rhs(Cv, 0.7, theta, b), R.rhs(Cv, 0.7, theta)
    assert np.array_equal(on[:-1], (Cv / 0.7) * theta[:-1] + 0.5) and on[-1] == 0.5
    assert np.array_equal(off[:-1], (Cv / 0.7) * theta[:-1]) and off[-1] == 0.0


# ---- the checks that come before the device ------------------------------------------------------------------------------

def model_of(capacity=3e-3, initial=None, film=1e-5):
    return solver.TransientModel(thermal=solver.ThermalModel(film=film), areal_capacity=capacity, initial=initial)


def test_the_names_are_exported():
    for name in ("Segment", "TransientModel", "CheckedTransientModel", "TransientReport", "TransientEnvelope",
                 "check_transient_model", "check_schedule", "solve_meshed_thermal_transient", "solve_thermal_transient"):
        assert hasattr(solver, name), name


def test_the_capacity_resolves_per_layer():
    prob, top, _bottom, *_ = board()
    assert solver.check_transient_model(prob, model_of(3e-3)).capacity == [3e-3, 3e-3]
    checked = solver.check_transient_model(prob, model_of({top: 1.2e-4, "B.Cu": 3e-3}))
    assert checked.capacity == [1.2e-4, 3e-3] and checked.thermal.film == [1e-5, 1e-5]


@pytest.mark.parametrize("bad", [0.0, -3e-3, float("nan"), float("inf"), "heavy", None])
def test_a_bad_capacity_is_refused(bad):
    prob = board()[0]
    with pytest.raises(ValueError):
        solver.check_transient_model(prob, model_of(bad))
    with pytest.raises(ValueError):
        solver.check_transient_model(prob, model_of({"F.Cu": 3e-3, "B.Cu": bad}))


def test_capacity_keys_and_the_thermal_model_are_checked():
    prob = board()[0]
    with pytest.raises(ValueError, match="B.Cu"):
        solver.check_transient_model(prob, model_of({"F.Cu": 3e-3}))
    with pytest.raises(ValueError):
        solver.check_transient_model(prob, model_of({"F.Cu": 3e-3, "B.Cu": 3e-3, "In1.Cu": 3e-3}))
    with pytest.raises(ValueError):
        solver.check_transient_model(prob, model_of(film=-1.0))
    with pytest.raises(ValueError):
        solver.check_transient_model(prob, solver.ThermalModel(film=1e-5))


def test_check_schedule_flattens_repeats_and_tuples():
    S = solver.Segment
    flat, n = solver.check_schedule([S(2.0, 4, 0), S(1.0, 1, None)], 1, repeat=3)
    assert n == 1 and len(flat) == 6
    assert [(s.duration, s.steps, s.case) for s in flat] == [(2.0, 4, 0), (1.0, 1, None)] * 3
    flat, n = solver.check_schedule([S(2.0, 4, (0, 1, None)), S(1.0, 2, [None, None, 1])], 2, repeat=2)
    assert n == 3 and [s.case for s in flat] == [(0, 1, None), (None, None, 1)] * 2
    flat, n = solver.check_schedule((S(0.5, np.int64(2), 0),), 1)
    assert n == 1 and flat[0].steps == 2 and isinstance(flat[0].steps, int)


@pytest.mark.parametrize("schedule, repeat", [
    ([], 1),
    ([solver.Segment(0.0, 1, 0)], 1), ([solver.Segment(-1.0, 1, 0)], 1), ([solver.Segment(float("nan"), 1, 0)], 1),
    ([solver.Segment(float("inf"), 1, 0)], 1),
    ([solver.Segment(1.0, 0, 0)], 1), ([solver.Segment(1.0, 1.5, 0)], 1), ([solver.Segment(1.0, True, 0)], 1),
    ([solver.Segment(1.0, 1, 1)], 1), ([solver.Segment(1.0, 1, -1)], 1), ([solver.Segment(1.0, 1, 0.0)], 1),
    ([solver.Segment(1.0, 1, (0, 1))], 1),
    ([solver.Segment(1.0, 1, (0, None)), solver.Segment(1.0, 1, (0, None, 0))], 1),
    ([solver.Segment(1.0, 1, ())], 1),
    ([solver.Segment(1.0, 1, 0)], 0), ([solver.Segment(1.0, 1, 0)], -2), ([solver.Segment(1.0, 1, 0)], 1.0),
    ([solver.Segment(1.0, 50001, 0)], 2), ([solver.Segment(1.0, 100001, 0)], 1),
    ([(1.0, 1, 0)], 1), (solver.Segment(1.0, 1, 0), 1),
])
def test_a_bad_schedule_is_refused(schedule, repeat):
    with pytest.raises(ValueError):
        solver.check_schedule(schedule, 1, repeat)


def test_the_step_limit_counts_the_repeats():
    flat, _n = solver.check_schedule([solver.Segment(1.0, 50000, 0)], 1, repeat=2)
    assert sum(s.steps for s in flat) == 100000


class _World:
    world = 2


def test_the_public_call_refuses_before_the_device():
    """Everything below raises ValueError with empty mesh lists: nothing reaches the device."""
    prob, *_ = board()
    S, call = solver.Segment, solver.solve_meshed_thermal_transient
    ok = [S(1.0, 2, 0)]
    stranger = P.NodeID()
    source = prob.networks[0].elements[0]
    bad = [
        dict(model=model_of(None), schedule=ok),
        dict(model=model_of({"F.Cu": 3e-3}), schedule=ok),
        dict(model=model_of(), schedule=[]),
        dict(model=model_of(), schedule=[S(1.0, 2, 1)]),                                   # one case: index 1 is out of range
        dict(model=model_of(), schedule=ok, cases=[{source: float("nan")}]),               # what check_load_cases refuses
        dict(model=model_of(initial=2), schedule=ok),
        dict(model=model_of(initial=(0, None, 0)), schedule=[S(1.0, 2, (0, None))]),       # three against two scenarios
        dict(model=model_of(), schedule=ok, repeat=0),
        dict(model=model_of(), schedule=ok, probes=[stranger]),
        dict(model=model_of(), schedule=ok, probes=["pad"]),
        dict(model=model_of(), schedule=ok, keep="all"),
        dict(model=model_of(), schedule=ok, partition=_World()),
        dict(model=solver.ThermalModel(film=1e-5), schedule=ok),
    ]
    for kw in bad:
        model, schedule = kw.pop("model"), kw.pop("schedule")
        with pytest.raises(ValueError):
            call(prob, [], [], model, schedule, **kw)
        if "partition" not in kw:
            with pytest.raises(ValueError):
                solver.solve_thermal_transient(prob, model, schedule, mesher=object(), **kw)


def test_initial_sets_the_number_of_scenarios_when_the_schedule_has_no_tuples():
    prob, *_ = board()
    args = solver._check_transient_arguments(prob, model_of(initial=(None, 0, 0)), [solver.Segment(1.0, 2, 0)], None, 2, (), "end", None)
    _checked, cases, flat, initial, probes = args
    assert cases == [{}] and initial == (None, 0, 0) and probes == []
    assert flat == [(0.5, 2, (0, 0, 0))] * 2

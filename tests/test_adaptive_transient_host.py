"""Host half of the adaptive transient (no GPU): the restatement of tests/sdirk_ref.py against what is known of the scheme --
its order, the closed form of uniform heating, the balances of both stages and of the step, and that it beats backward Euler
at equal cost; the step-size rule of ``solver.dyadic_controller`` on synthetic error sequences and against the restated
rule; and the refusals of ``check_spans``, ``check_step_control`` and the public call, which come before the device."""
import math

import numpy as np
import pytest

import sdirk_ref as SR
import thermal_ref as T
import transient_ref as R
from padne_amd import _hip, problem as P, solver
from test_thermal_host import board
from test_transient_host import KAPPA, model_of, one_mesh


def test_the_constants():
    """gamma = 1 - 1/sqrt(2) and q = (1 - gamma) / gamma = sqrt(2) + 1 to the last bit or the one next to it, the same doubles
    in the restatement, the binding and the solver; q gamma = 1 - gamma to rounding."""
    assert SR.GAMMA == _hip.SDIRK_GAMMA == solver.SDIRK_GAMMA and SR.Q == _hip.SDIRK_Q
    assert abs(SR.GAMMA - (1 - 1 / math.sqrt(2))) <= 2.0 ** -53 and abs(SR.Q - (math.sqrt(2) + 1)) <= 2.0 ** -51
    assert abs(SR.Q * SR.GAMMA - (1 - SR.GAMMA)) <= 2.0 ** -52


# ---- 1. the scheme ---------------------------------------------------------------------------------------------------------

def random_load(xy, tri, seed=4):
    return T.load(len(xy), tri, np.random.default_rng(seed).uniform(0, 1e-3, len(tri)))


def test_halving_dt_quarters_the_error():
    """Second order: on the board and load of test_halving_dt_halves_the_error, against 512 steps, the error at the end of the
    span falls by a factor in [3.6, 4.4] per halving over 8, 16 and 32 steps."""
    film, c = 1e-3, 3e-3
    xy, tri, A, _M, _hM, _voff, Cv = one_mesh(17, film, c)
    b = random_load(xy, tri)
    span = c / film
    fine = SR.uniform(A, Cv, b, span, 512)[-1]
    errors = [float(np.abs(SR.uniform(A, Cv, b, span, s)[-1] - fine).max()) for s in (8, 16, 32)]
    rates = [a / b_ for a, b_ in zip(errors, errors[1:])]
    print("errors", errors, "rates", rates)
    assert all(3.6 <= r <= 4.4 for r in rates), rates


def test_uniform_heating_follows_the_closed_form():
    """P_f = q A_f and no links: theta_n = (q / h) (1 - R(z)^n) at every vertex with z = -h dt / c, within 1e-12 relative."""
    q, h, c, dt = 3e-4, 2e-5, 3e-3, 10.0
    xy, tri, A, _M, _hM, _voff, Cv = one_mesh(17, h, c)
    b = T.load(len(xy), tri, q * T.face_area(xy, tri))
    states = SR.uniform(A, Cv, b, 30 * dt, 30)
    grow = SR.growth(-h * dt / c)
    worst = max(float(np.abs(states[n] - (q / h) * (1 - grow ** n)).max()) / (q / h) for n in range(31))
    print("relative error", worst)
    assert 0 < grow < 1 and worst <= 1e-12


def balance_defects(A, Cv, hM, b, theta0, dt):
    """The three identities of one step from ``theta0``, each as a defect relative to the heat."""
    n_vert = len(Cv)
    heat = math.fsum(b.tolist())
    got = SR.Stepper(A, Cv).step(theta0, dt, b)
    dts = SR.GAMMA * dt
    stored = lambda th: math.fsum((Cv * th[:n_vert]).tolist())                            # noqa: E731
    loss = lambda th: math.fsum((hM * th[:n_vert]).tolist())                              # noqa: E731
    one = (stored(got["theta_1"]) - stored(theta0)) / dts + loss(got["theta_1"]) - heat
    two = (stored(got["theta"]) - stored(got["star"])) / dts + loss(got["theta"]) - heat
    step = (stored(got["theta"]) - stored(theta0)) / dt + (1 - SR.GAMMA) * loss(got["theta_1"]) + SR.GAMMA * loss(got["theta"]) - heat
    return [abs(d) / heat for d in (one, two, step)], got["theta"]


@pytest.mark.parametrize("internal", [False, True])
def test_both_stages_and_the_step_obey_their_balances(internal):
    """Stage 1, stage 2 and the step (with the weights 1 - gamma and gamma on the two film losses, since q gamma = 1 - gamma)
    each within 1e-12 of the heat, over four steps from ambient; also with an internal node that carries heat of its own, whose
    row stays A theta = b in both stages."""
    film, c = 1e-3, 3e-3
    xy, tri, A, _M, hM, voff, Cv = one_mesh(17, film, c)
    b = random_load(xy, tri, seed=2)
    if internal:
        A = T.operator([(xy, tri)], [KAPPA], [film], 1, [(3, len(xy), 0.1)])[0]
        b = np.concatenate([b, [2e-2]])
    theta, worst = np.zeros(A.shape[0]), 0.0
    for _ in range(4):
        defects, theta = balance_defects(A, Cv, hM, b, theta, c / film / 10)
        worst = max(worst, *defects)
    print("internal node" if internal else "vertices only", "worst defect / heat", worst)
    assert worst <= 1e-12
    assert not internal or theta[-1] > theta[3] > 0.0        # the heated node is hotter than the copper it hangs on


@pytest.mark.parametrize("fraction", [1e-2, 1e-3])
def test_the_adaptive_run_beats_backward_euler_with_as_many_solves(fraction):
    """one_mesh(17, 1e-5, 3e-3), 600 s on and 600 s off at a tolerance of 1 % and 0.1 % of the steady rise: at the end of
    either span the run is nearer a 4096-step SDIRK2 answer than backward Euler with as many solves as the run spent
    (two per trial, the rejected ones included)."""
    film, c = 1e-5, 3e-3
    xy, tri, A, _M, hM, voff, Cv = one_mesh(17, film, c)
    b = random_load(xy, tri)
    tolerance = fraction * float(T.solve(A, b).max())
    got = SR.run(A, Cv, [b], [(600.0, 0), (600.0, None)], tolerance)
    ends = [i for i, t in enumerate(got["times"]) if t in (600.0, 1200.0)]
    assert len(ends) == 2 and got["times"][-1] == 1200.0
    fine_on = SR.uniform(A, Cv, b, 600.0, 4096)[-1]
    fine_off = SR.uniform(A, Cv, None, 600.0, 4096, fine_on)[-1]
    per_span = len(got["decisions"])                        # two solves per trial, two spans: as many steps per span as trials
    euler = R.run(A, Cv, hM, voff, [b], [(600.0 / per_span, per_span, 0), (600.0 / per_span, per_span, None)])[0]
    ours = [float(np.abs(got["states"][ends[0]] - fine_on).max()), float(np.abs(got["states"][ends[1]] - fine_off).max())]
    theirs = [float(np.abs(euler[per_span] - fine_on).max()), float(np.abs(euler[-1] - fine_off).max())]
    print("tolerance", tolerance, "steps", len(got["taken"]), "trials", len(got["decisions"]), "K off: adaptive", ours,
          "backward Euler with", per_span, "steps per span", theirs)
    assert ours[0] < theirs[0] and ours[1] < theirs[1]


def test_a_coarse_first_step_is_rejected_and_ends_where_the_default_start_ends():
    """first_step = D / 4 on the same board: rejections, and the end state within the tolerance of the default start's."""
    film, c = 1e-5, 3e-3
    xy, tri, A, _M, _hM, _voff, Cv = one_mesh(17, film, c)
    b = random_load(xy, tri)
    tolerance = 1e-2 * float(T.solve(A, b).max())
    spans = [(600.0, 0), (600.0, None)]
    fine, coarse = SR.run(A, Cv, [b], spans, tolerance), SR.run(A, Cv, [b], spans, tolerance, first_step=150.0)
    rejected = coarse["decisions"].count("reject")
    print("default start: trials", len(fine["decisions"]), "first_step = D / 4: trials", len(coarse["decisions"]), "rejected", rejected)
    assert rejected > 0 and fine["decisions"].count("reject") == 0 and coarse["step_sizes"][0] < 150.0
    assert coarse["times"][-1] == fine["times"][-1] == 1200.0
    assert np.abs(coarse["states"][-1] - fine["states"][-1]).max() <= tolerance


# ---- 2. the step-size rule -------------------------------------------------------------------------------------------------

def drive(duration, tolerance, errors, **kw):
    """``solver.dyadic_controller`` fed ``errors`` (a callable of (dt, pos, level) or a sequence): the yielded tuples."""
    control = solver.dyadic_controller(duration, tolerance, **kw)
    seen = [next(control)]
    feed = iter(errors) if not callable(errors) else None
    while seen[-1][1] is not None:
        _verdict, dt, level, pos = seen[-1]
        seen.append(control.send(errors(dt, pos, level) if feed is None else next(feed)))
    return seen


def test_levels():
    assert solver.dyadic_levels(8.0) == (10, 30) == SR.levels(8.0)
    assert solver.dyadic_levels(8.0, first_step=2.0, min_step=1.0) == (2, 3) == SR.levels(8.0, 2.0, 1.0)
    assert solver.dyadic_levels(8.0, first_step=3.0) == (2, 30)            # the smallest k with 8 / 2^k <= 3
    assert solver.dyadic_levels(8.0, first_step=100.0, min_step=50.0) == (0, 0) == SR.levels(8.0, 100.0, 50.0)
    assert solver.dyadic_levels(8.0, first_step=3.0, min_step=3.0) == (2, 1) == SR.levels(8.0, 3.0, 3.0)


def test_small_errors_grow_the_step_only_on_an_even_position_and_land_on_the_end():
    """err = 0 throughout from level 4: 1/16, 1/16, then 1/8 (pos 2 -> 1: odd, no growth), 1/8 (pos 2 -> 1 at level 2), ..."""
    seen = drive(16.0, 1.0, lambda dt, pos, level: 0.0, first_step=1.0)
    dts = [s[1] for s in seen[:-1]]
    assert dts == [1.0, 1.0, 2.0, 4.0, 8.0] and math.fsum(dts) == 16.0
    assert [s[0] for s in seen[1:]] == ["accept"] * 5 and seen[-1][1] is None
    # growth happened only where the position in units of the step taken was even
    for (_v0, dt0, level0, pos0), (_v1, dt1, level1, pos1) in zip(seen, seen[1:-1]):
        if level1 < level0:
            assert (pos0 + 1) % 2 == 0 and level1 == level0 - 1 and pos1 == (pos0 + 1) // 2 and dt1 == 2 * dt0
        else:
            assert pos1 == pos0 + 1


def test_a_reject_halves_the_step_and_doubles_the_position():
    """An error above the tolerance whenever the step exceeds 1: from level 1 of 16 s down to level 4, pos doubling on the way
    (0 stays 0), then accepted steps of 1 that never grow because err is above tolerance / 4."""
    seen = drive(16.0, 1.0, lambda dt, pos, level: 2.0 if dt > 1.0 else 0.5, first_step=8.0)
    assert [s[0] for s in seen[1:4]] == ["reject"] * 3 and [s[2] for s in seen[:4]] == [1, 2, 3, 4]
    assert all(s[0] == "accept" for s in seen[4:]) and len(seen) == 4 + 16
    # a reject in the middle: the position doubles
    seen = drive(16.0, 1.0, [0.0, 0.0, 2.0, 0.5, 0.5] + [0.5] * 40, first_step=4.0)
    assert seen[2][:1] == ("accept",) and seen[2][2:] == (1, 1)             # two steps of 4 taken, grown to 8: pos 1 of 2
    assert seen[3] == ("reject", 4.0, 2, 2)                                  # back to 4: pos 2 of 4
    assert math.fsum(dt for (v, *_), (_v, dt, *_r) in zip(seen[1:], seen) if v != "reject") == 16.0


def test_the_deepest_level_forces_acceptance_and_warns_once():
    seen = drive(8.0, 1.0, lambda dt, pos, level: 5.0, first_step=4.0, min_step=2.0)
    assert [s[0] for s in seen[1:]] == ["reject"] + ["forced"] * 4
    taken = []
    with pytest.warns(solver.SolverWarning) as caught:
        out = solver.adaptive_walk([(8.0, "a"), (8.0, "b")], 1.0, 4.0, 2.0, 100, lambda dt, load: [5.0, 0.0],
                                   lambda dt, time, load, errors: taken.append((dt, time, load)))
    assert len([w for w in caught if issubclass(w.category, solver.SolverWarning)]) == 1
    assert out["tried"] == 10 and out["rejected"] == 2 and out["forced"] == 8
    assert [t[1] for t in taken] == [2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0, 16.0] and [t[2] for t in taken] == ["a"] * 4 + ["b"] * 4


def test_max_steps_and_a_non_finite_estimate_raise():
    nothing = lambda *a: None                                                             # noqa: E731
    with pytest.raises(RuntimeError, match="t = 3"):
        solver.adaptive_walk([(16.0, 0)], 1.0, 1.0, None, 3, lambda dt, load: [0.5], nothing)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="finite"):
            solver.adaptive_walk([(16.0, 0)], 1.0, 1.0, None, 100, lambda dt, load: [0.0, bad], nothing)


@pytest.mark.parametrize("seed", range(6))
def test_the_generator_takes_the_path_of_the_restated_rule(seed):
    """Random error sequences (a function of the step, so that both walks see the same): the decisions, the steps, the times
    and the places of growth of ``solver.adaptive_walk`` are those of ``sdirk_ref.walk``; span ends are hit exactly."""
    rng = np.random.default_rng(seed)
    table = {}

    def err_of(dt, load):
        key = (dt, load, len(table))
        return table.setdefault(key, float(rng.choice([0.0, 0.2, 0.3, 0.9, 1.5, 3.0]) * min(1.0, (dt / 0.5) ** 2)))

    spans = [(7.0, 0), (0.3, 1), (11.0, None)]
    calls = []
    want = SR.walk(spans, 1.0, lambda dt, load: (err_of(dt, load), None), first_step=2.0, min_step=0.01)
    replay = iter(want["errors"])
    out = solver.adaptive_walk(spans, 1.0, 2.0, 0.01, 100000, lambda dt, load: [next(replay)],
                               lambda dt, time, load, errors: calls.append((dt, time, load, float(errors[0]))))
    assert out["decisions"] == want["decisions"] and [c[:4] for c in calls] == [t[:4] for t in want["taken"]]
    times = [c[1] for c in calls]
    assert 7.0 in times and 7.0 + 0.3 in times and times[-1] == (7.0 + 0.3) + 11.0 and (np.diff([0.0] + times) > 0).all()
    assert out["rejected"] > 0 and len(want["grown"]) > 0


# ---- 3. the checks that come before the device ------------------------------------------------------------------------------

def test_the_names_are_exported():
    for name in ("Span", "check_spans", "check_step_control", "dyadic_levels", "dyadic_controller", "adaptive_walk",
                 "solve_meshed_thermal_transient_adaptive", "solve_thermal_transient_adaptive", "SDIRK_GAMMA"):
        assert hasattr(solver, name), name
    for name in ("try_step", "accept", "trial"):
        assert hasattr(_hip.Transient, name), name


def test_check_spans_flattens_repeats_and_tuples():
    S = solver.Span
    flat, n = solver.check_spans([S(2.0, 0), S(1.0)], 1, repeat=3)
    assert n == 1 and [(s.duration, s.case) for s in flat] == [(2.0, 0), (1.0, None)] * 3
    flat, n = solver.check_spans((S(2, (0, 1, None)), S(1.0, [None, None, 1])), 2)
    assert n == 3 and [s.case for s in flat] == [(0, 1, None), (None, None, 1)] and isinstance(flat[0].duration, float)


@pytest.mark.parametrize("schedule, repeat", [
    ([], 1), ([solver.Span(0.0, 0)], 1), ([solver.Span(-1.0, 0)], 1), ([solver.Span(float("nan"), 0)], 1),
    ([solver.Span(float("inf"), 0)], 1), ([solver.Span(1.0, 1)], 1), ([solver.Span(1.0, -1)], 1), ([solver.Span(1.0, 0.0)], 1),
    ([solver.Span(1.0, (0, 1))], 1), ([solver.Span(1.0, (0, None)), solver.Span(1.0, (0, None, 0))], 1), ([solver.Span(1.0, ())], 1),
    ([solver.Span(1.0, 0)], 0), ([solver.Span(1.0, 0)], 1.0), ([solver.Span(1.0, 0)], True),
    ([(1.0, 0)], 1), (solver.Span(1.0, 0), 1), ([solver.Segment(1.0, 1, 0)], 1), ("spans", 1), (3, 1),
])
def test_a_bad_schedule_of_spans_is_refused(schedule, repeat):
    with pytest.raises(ValueError):
        solver.check_spans(schedule, 1, repeat)


def test_check_step_control():
    assert solver.check_step_control(0.5) == (0.5, None, None, solver.MAX_TRANSIENT_STEPS)
    assert solver.check_step_control(1, 2, 2, np.int64(7)) == (1.0, 2.0, 2.0, 7)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(tolerance=0.0), dict(tolerance=-1.0), dict(tolerance=nan), dict(tolerance=inf), dict(tolerance=None),
                dict(tolerance="tight"), dict(first_step=0.0), dict(first_step=-1.0), dict(first_step=nan), dict(first_step=inf),
                dict(min_step=0.0), dict(min_step=nan), dict(min_step=inf), dict(first_step=1.0, min_step=2.0),
                dict(max_steps=0), dict(max_steps=-3), dict(max_steps=2.0), dict(max_steps=True), dict(max_steps=None)):
        with pytest.raises(ValueError):
            solver.check_step_control(**{"tolerance": 1.0, **bad})


class _World:
    world = 2


def test_the_public_call_refuses_before_the_device():
    """Everything below raises ValueError with empty mesh lists: nothing reaches the device."""
    prob, *_ = board()
    S, call = solver.Span, solver.solve_meshed_thermal_transient_adaptive
    ok = [S(1.0, 0)]
    source = prob.networks[0].elements[0]
    bad = [
        dict(model=model_of(None), schedule=ok),
        dict(model=model_of(), schedule=[]),
        dict(model=model_of(), schedule=[S(1.0, 1)]),
        dict(model=model_of(), schedule=[solver.Segment(1.0, 2, 0)]),
        dict(model=model_of(), schedule=ok, cases=[{source: float("nan")}]),
        dict(model=model_of(initial=2), schedule=ok),
        dict(model=model_of(initial=(0, None, 0)), schedule=[S(1.0, (0, None))]),
        dict(model=model_of(), schedule=ok, repeat=0),
        dict(model=model_of(), schedule=ok, probes=[P.NodeID()]),
        dict(model=model_of(), schedule=ok, keep="all"),
        dict(model=model_of(), schedule=ok, partition=_World()),
        dict(model=model_of(), schedule=ok, tolerance=0.0),
        dict(model=model_of(), schedule=ok, tolerance=float("nan")),
        dict(model=model_of(), schedule=ok, first_step=-1.0),
        dict(model=model_of(), schedule=ok, first_step=0.1, min_step=0.2),
        dict(model=model_of(), schedule=ok, max_steps=0),
        dict(model=solver.ThermalModel(film=1e-5), schedule=ok),
    ]
    for kw in bad:
        kw = dict({"tolerance": 0.1}, **kw)
        model, schedule = kw.pop("model"), kw.pop("schedule")
        with pytest.raises(ValueError):
            call(prob, [], [], model, schedule, **kw)
        if "partition" not in kw:
            with pytest.raises(ValueError):
                solver.solve_thermal_transient_adaptive(prob, model, schedule, mesher=object(), **kw)
    with pytest.raises(TypeError):                           # the tolerance has no default
        call(prob, [], [], model_of(), ok)

"""The periodic steady state on the device against the host specification (tests/periodic_ref.py, itself checked by
tests/test_periodic_host.py): the three kernel families bit for bit on random vectors; the entries that put a state into the
transient handle; the answer against a dense solve of (I - Phi) theta* = d; the physics of the periodic state; scenarios;
``interlayer``, ``heat_sources``, ``keep`` and probes; the refusals of the device entries; bitwise repeatability.

Boards: ``test_transient.BOARDS`` through its ``Stepping`` helper, and one 260 x 260 jittered grid (67 600 vertices, 265
tiles) on which the second-level fold strides past its 256 lanes.

The bit-for-bit kernel tests and the dense-answer test are the ones that can catch a wrong kernel.  Each was seen to fail
once in a scratch build of csrc/periodic.hip: with the four waves of periodic_fold_kernel joined as ((0 + 1) + 2) + 3 (a
perturbed fold order) the kernel test fails on the 260 x 260 grid and only there -- with fewer than 65 tiles wave 0 alone
holds partial sums, which is why that board is in the table; with the combination taking coefficient 1 for vector 0 and
coefficient 0 for vector 1 (a swapped coefficient) all six kernel cases and both dense-answer cases fail; with the dot's term
w[v] * V_i[v] (the Cv weight dropped) all six kernel cases fail, while the dense-answer test passes: GMRES converges in
the unweighted inner product as well, so only the bit-for-bit test holds the weight."""
import warnings

import numpy as np
import pytest

import periodic_ref as PR
import test_thermal as TT
from padne_amd import _hip, mesh, problem as P, solver, synthetic
from test_thermal import BAR, quiet, random_loads
from test_transient import GRID49, TAU, Stepping, board, model_of

pytestmark = pytest.mark.gpu

GRID260 = "grid260"
TOL = 1e-6


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def grid260_board():
    """``single`` of tests/test_thermal.py on a 260 x 260 grid: 67 600 vertices, more than 256 tiles of 256."""
    if GRID260 not in TT._BOARDS:
        top = P.Layer(shape=TT.H.Geoms(1), name="F.Cu", conductance=2086.0)
        c = [TT.conn(top, 1, 1), TT.conn(top, 7, 7)]
        net = P.Network(connections=c, elements=[P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0)])
        xy, tri = synthetic.jittered_grid(260, 260, h=8.0 / 259, seed=9, jitter=0.2)
        msh = mesh.Mesh(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3))
        prob, meshes, layer_of = P.Problem(layers=[top], networks=[net]), [msh], [0]
        vindex = solver.VertexIndexer.create(meshes)
        nodes = solver.NodeIndexer.create(prob, meshes, layer_of, vindex, list(prob.networks))
        flat = [(np.asarray(m.points, dtype=np.float64), np.asarray(m.triangles, dtype=np.int64)) for m in meshes]
        TT._BOARDS[GRID260] = (prob, meshes, layer_of, [[]], flat, nodes.internal_node_count,
                               solver.global_elements(list(prob.networks), nodes))
    return GRID260


class Krylov:
    """A ``Stepping`` with one random load case, ``n_cols`` columns started at ambient and a ``_hip.Periodic`` of
    ``max_vectors``."""

    def __init__(self, name, n_cols, max_vectors, seed=1):
        self.dev, self.n_cols, self.max_vectors, self.seed = Stepping(name), n_cols, max_vectors, seed

    def __enter__(self):
        dev = self.dev.__enter__()
        dev.tr.loads(*random_loads(dev, 1, self.seed))
        dev.tr.start([None] * self.n_cols)
        self.per = _hip.Periodic(dev.tr, self.max_vectors)
        self.Cv = dev.tr.capacity(dev.n_vert)
        return self

    def __exit__(self, *exc):
        self.per.close()
        return self.dev.__exit__(*exc)

    def random(self, rng, *lead):
        return rng.standard_normal((*lead, self.n_cols, self.dev.n_pot))


# ---- 1. the kernels, bit for bit ------------------------------------------------------------------------------------------

KERNEL_CASES = [("single", 1, 1), ("single", 8, 3), ("single", 9, 11), ("two_layer", 17, 3), ("two_in_layer", 9, 1), (GRID260, 9, 3)]


@pytest.mark.parametrize("name, n_vec, n_cols", KERNEL_CASES)
def test_the_kernels_are_the_specification_bit_for_bit(ctx, name, n_vec, n_cols):
    """Random vectors given to the entries: the Hessenberg column and v_{j+1} of a push over 1, 8, 9 and 17 basis vectors (a
    full chunk of dots, one over, two chunks and one over) in 1, 3 and 11 columns; the predicted closure with its vertex;
    the combination; the residual.  No vertex count is a multiple of 256; the 260 x 260 grid has 265 tiles."""
    if name == GRID260:
        grid260_board()
    rng = np.random.default_rng(100 + n_vec)
    with Krylov(name, n_cols, n_vec + 1) as k:
        dev, per, Cv, n_vert = k.dev, k.per, k.Cv, k.dev.n_vert
        assert n_vert % 256 != 0
        V, S, r, x = k.random(rng, n_vec), k.random(rng), k.random(rng), k.random(rng)
        for j in range(n_vec):
            per.put(j, V[j])
        per.put(per.STATE, S)
        h = per.push(n_vec - 1)
        nxt = per.vector(n_vec)
        assert np.array_equal(dev.tr.state(), S)                                # a push leaves the state alone
        coef, y = rng.standard_normal((n_cols, n_vec + 1)), rng.standard_normal((n_cols, n_vec + 1))
        per.put(per.R0, r)
        top, vert = per.predict(coef)
        per.put(per.X0, x)
        per.combine(y)
        combined = dev.tr.state()
        per.put(per.STATE, S)
        per.mark()
        per.put(per.STATE, r)
        beta, rtop, rvert = per.residual()
        r0, v0 = per.vector(per.R0), per.vector(0)
    for c in range(n_cols):
        basis = [V[j][c] for j in range(n_vec)]
        want_h, want_next = PR.push(Cv, basis, S[c])
        assert np.array_equal(h[c], want_h), c
        assert np.array_equal(nxt[c], want_next), c
        full = basis + [want_next]
        assert (top[c], vert[c]) == PR.predict(r[c], coef[c], full, n_vert), c
        assert np.array_equal(combined[c], PR.combine(x[c], y[c], full)), c
        want_r0, want_beta, want_v0, want_top = PR.residual(Cv, r[c], S[c])
        assert np.array_equal(r0[c], want_r0) and beta[c] == want_beta and np.array_equal(v0[c], want_v0), c
        assert (rtop[c], rvert[c]) == want_top, c


def test_tops_with_planted_ties_and_values_that_are_not_finite(ctx):
    """The vector is given to the entry directly.  Column 0: two equal maxima of opposite sign in different tiles, the lowest
    vertex wins; column 1: a NaN counts as +infinity and beats every number; column 2: two infinities, the lowest wins;
    column 3: all zeros, vertex 0."""
    with Krylov("single", 4, 2) as k:
        n_pot, n_vert = k.dev.n_pot, k.dev.n_vert
        r = np.random.default_rng(3).uniform(-1.0, 1.0, (4, n_pot))
        r[0, [270, 31]] = [-7.5, 7.5]
        r[1, [100, 20]] = [np.nan, 50.0]
        r[2, [280, 257, 5]] = [np.inf, -np.inf, 1e300]
        r[3] = 0.0
        k.per.put(k.per.R0, r)
        top, vert = k.per.predict(np.zeros((4, 0)))
    assert top.tolist() == [7.5, np.inf, np.inf, 0.0] and vert.tolist() == [31, 100, 257, 0]
    for c in range(4):
        assert (top[c], vert[c]) == PR.top(r[c], n_vert)


def test_a_frozen_column_stays_zero_on_the_device(ctx):
    """Column 1 is periodic at once (state = x0): beta 0, v_0 zeros, and a push from the zero state that an off-period of
    zeros ends in gives zeros, not NaN."""
    rng = np.random.default_rng(4)
    with Krylov("single", 2, 3) as k:
        S, S2, S3 = k.random(rng), k.random(rng), k.random(rng)
        S2[1], S3[1] = S[1], 0.0
        k.per.put(k.per.STATE, S)
        k.per.mark()
        k.per.put(k.per.STATE, S2)
        beta, top, _vert = k.per.residual()
        k.per.put(k.per.STATE, S3)
        h = k.per.push(0)
        v0, v1 = k.per.vector(0), k.per.vector(1)
        ptop, _ = k.per.predict(np.array([[0.5, 0.25], [0.0, 0.0]]))
    assert beta[0] > 0.0 and beta[1] == 0.0 and top[1] == 0.0
    assert not v0[1].any() and not v1[1].any() and np.isfinite(v1).all() and np.isfinite(h).all() and np.isfinite(ptop).all()
    assert h[1].tolist() == [0.0, 0.0] and h[0, 1] > 0.0 and ptop[1] == 0.0


# ---- 2. the loop -----------------------------------------------------------------------------------------------------------

def cycle_schedule(period=TAU / 30, on=0):
    """On for 40 % of the period in 6 steps, off for the rest in 8: two segments of unequal dt."""
    return [(0.4 * period / 6, 6, on), (0.6 * period / 8, 8, None)]


@pytest.mark.parametrize("name", ["two_layer", GRID49])
def test_load_combine_and_mark_put_states_into_the_handle(ctx, name):
    """_load, _combine and _mark round-trip states exactly; after either the clock is 0 and the envelope is the state with
    step 0; one off-period from v_0 through the handle is transient_ref's within the step tolerance (BAR of max |v_0|)."""
    rng = np.random.default_rng(6)
    schedule = cycle_schedule()
    with Krylov(name, 2, 4) as k:
        dev, per, n_vert = k.dev, k.per, k.dev.n_vert
        dev.tr.run(0.1, 3, [0, None])                                          # the clock runs, the envelope has moved
        S = np.abs(k.random(rng))
        per.put(per.STATE, S)
        per.mark()
        per.put(per.STATE, S + np.abs(k.random(rng)))
        per.residual()
        dev.tr.run(0.1, 2, [0, 0])
        per.load(0)
        loaded, v0 = dev.tr.state(), per.vector(0)
        clock_l, (env_l, step_l) = dev.tr.clock()[:2], dev.tr.envelope(n_vert)
        for dt, steps, _case in schedule:
            dev.tr.run(dt, steps, [None, None])
        after, clock_p = dev.tr.state(), dev.tr.clock()[:2]
        per.combine(np.zeros((2, 0)))
        back = dev.tr.state()
        clock_c, (env_c, step_c) = dev.tr.clock()[:2], dev.tr.envelope(n_vert)
        per.mark()
        marked = per.vector(per.X0)
        A, _hM, Cv = dev.host()
    assert np.array_equal(loaded, v0) and np.array_equal(back, S) and np.array_equal(marked, S)
    assert clock_l == (0, 0.0) and clock_c == (0, 0.0) and clock_p[0] == 14
    assert np.array_equal(env_l, v0[:, :n_vert]) and not step_l.any()
    assert np.array_equal(env_c, S[:, :n_vert]) and not step_c.any()
    ref = PR.Period(A, Cv, [], schedule)
    for c in range(2):
        want = ref.apply(v0[c], sources=False)
        assert np.abs(after[c] - want).max() <= BAR * np.abs(v0[c]).max(), c


# ---- 3. the answer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["single", "two_layer"])
def test_the_answer_against_the_dense_periodic_state(ctx, name):
    """The iteration of the public call through the handles, from ambient: theta(0) of the cycle within
    ||(I - Phi_vv)^-1||_inf (closure + BAR max |theta*|) of the dense theta* at the vertices (the bound of
    tests/test_periodic_host.py with the step tolerance of tests/test_transient.py as the solves' slack), the measured
    closure within the tolerance, the count of periods within one of the specification's, and the cycle bit for bit what plain
    runs give from that state."""
    schedule = cycle_schedule(TAU / 5)
    with Krylov(name, 1, 63) as k:
        dev, per, n_vert = k.dev, k.per, k.dev.n_vert
        B = dev.tr.load_vectors()
        flat = [(dt, steps, [case]) for dt, steps, case in schedule]
        found = solver.periodic_iteration(dev.tr, per, flat, TOL, 64)
        theta0 = dev.tr.state()
        per.mark()
        first = [dev.tr.run(dt, steps, cases, dev.all_unknowns()) for dt, steps, cases in flat]
        _beta, closure, _vert = per.residual()
        env = dev.tr.envelope(n_vert)
        per.put(per.STATE, theta0)
        again = [dev.tr.run(dt, steps, cases, dev.all_unknowns()) for dt, steps, cases in flat]
        env_again = dev.tr.envelope(n_vert)
        A, _hM, Cv = dev.host()
    Phi, d = PR.dense_period(A, Cv, B, schedule)
    want, _ = PR.dense_periodic_state(Phi, d)
    norm = float(np.abs(np.linalg.inv(np.eye(n_vert) - Phi[:n_vert, :n_vert])).sum(axis=1).max())
    ref = PR.gmres(PR.Period(A, Cv, B, schedule), np.zeros(dev.n_pot), TOL, 64)
    err, scale = float(np.abs(theta0[0, :n_vert] - want[:n_vert]).max()), float(np.abs(want).max())
    periods = found["applications"] + 1
    print(name, "periods", periods, "specification", ref["periods"], "closure", closure[0], "predicted", found["predicted"][-1][0],
          "error", err, "bound", norm * (closure[0] + BAR * scale))
    assert closure[0] <= TOL
    assert err <= norm * (closure[0] + BAR * scale)
    assert abs(periods - ref["periods"]) <= 1
    for a, b in zip(first, again):
        assert all(np.array_equal(a[key], b[key]) for key in ("max", "vertex", "stored", "loss", "probes"))
    assert np.array_equal(env[0], env_again[0]) and np.array_equal(env[1], env_again[1])


# ---- 4. the public call ----------------------------------------------------------------------------------------------------

def public_cycle(period=TAU / 30, case=0):
    return [solver.Segment(0.4 * period, 6, case), solver.Segment(0.6 * period, 8, None)]


def test_the_physics_of_the_periodic_state_on_the_49_grid(ctx):
    """Over the recorded cycle sum_n dt_n loss_{n+1} = sum_n dt_n heat_n and stored(T) = stored(0), both within
    tolerance * sum(Cv) -- what a closure of ``tolerance`` kelvin allows -- plus 1e-9 of the cycle's heat for the solves (the
    bar of the transient balance test).  The first cycle from ambient (``repeat=1``) has an envelope hotspot far below the
    periodic one: a rise of 0.0096 K against 0.0420 K (the board's 2 A dissipate 0.3 mW; printed by the test), so the
    assertion asks for less than half.  13 period applications, 26 hierarchies (one per change of dt)."""
    prob, meshes, layer_of, disc, *_ = board(GRID49)
    with Stepping(GRID49) as dev:
        sum_cv = float(dev.tr.capacity(dev.n_vert).sum())
    model = model_of()
    _s, rep = quiet(solver.solve_meshed_thermal_periodic, prob, meshes, layer_of, model, public_cycle(), tolerance=TOL,
                    disconnected_meshes_by_layer=disc)
    _s, once = quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, model, public_cycle(),
                     disconnected_meshes_by_layer=disc)
    cyc = rep.cycle
    dts = np.diff(cyc.times)
    lost, put = float((dts * cyc.total_loss[1:]).sum()), float((dts * cyc.total_heat[1:]).sum())
    ambient = solver.check_thermal_model(prob, model.thermal).ambient
    rise, rise_once = rep.cycle.envelope.hotspots[0][0] - ambient, once.envelope.hotspots[0][0] - ambient
    print("periods", rep.periods, "closure", rep.closure, "predicted", rep.predicted, "lost", lost, "put", put,
          "stored", cyc.total_stored[0], cyc.total_stored[-1], "hotspot rise periodic", rise, "first cycle", rise_once,
          "hierarchies", rep.info["hierarchies"])
    assert rep.converged and rep.closure <= TOL and rep.periods < 64 and len(rep.predicted) == rep.periods - 2
    assert cyc.times[0] == 0.0 and len(cyc.times) == 15 and abs(cyc.times[-1] - TAU / 30) <= 1e-12
    assert abs(lost - put) <= TOL * sum_cv + 1e-9 * put
    assert abs(cyc.total_stored[-1] - cyc.total_stored[0]) <= TOL * sum_cv + 1e-9 * put
    assert 0.0 < rise_once < 0.5 * rise
    assert rep.closure_at is not None and rep.closure_at[0] == 0


def test_three_scenarios_in_lockstep_a_frozen_one_among_them(ctx):
    """Scenarios (on/off, always off from ambient, on/off from the steady state) in lockstep against the live ones alone:
    theta(0) at the hotspot and the envelope hotspot agree within ||(I - Phi_vv)^-1||_inf 2 tolerance + BAR of the rise (each
    is within the norm times its closure of the one periodic state; the norm is at most 1 / (1 - rho) <= 1 + tau / T, 6 here).  The
    frozen scenario reports closure 0, ambient throughout and no NaN."""
    prob, meshes, layer_of, disc, *_ = board("single")
    period = TAU / 5
    S = solver.Segment
    lock = [S(0.4 * period, 6, (0, None, 0)), S(0.6 * period, 8, (None, None, None))]
    model = model_of(initial=(None, None, 0))
    _s, reps = quiet(solver.solve_meshed_thermal_periodic, prob, meshes, layer_of, model, lock, tolerance=TOL,
                     disconnected_meshes_by_layer=disc)
    assert len(reps) == 3 and all(r.converged for r in reps)
    ambient = solver.check_thermal_model(prob, model.thermal).ambient
    frozen = reps[1]
    assert frozen.closure == 0.0 and frozen.cycle.peak[0] == ambient and np.isfinite(frozen.cycle.total_stored).all()
    assert all(p == 0.0 for p in frozen.predicted)
    norm = 1.0 + TAU / period
    for c, initial in ((0, None), (2, 0)):
        _s, alone = quiet(solver.solve_meshed_thermal_periodic, prob, meshes, layer_of, model_of(initial=initial),
                          public_cycle(period), tolerance=TOL, disconnected_meshes_by_layer=disc)
        rise = alone.cycle.peak[0] - ambient
        for a, b in ((alone.cycle.hotspots[0][0][0], reps[c].cycle.hotspots[0][0][0]),
                     (alone.cycle.envelope.hotspots[0][0], reps[c].cycle.envelope.hotspots[0][0])):
            assert abs(a - b) <= norm * 2 * TOL + BAR * rise, (c, a, b)
    # the periodic state does not depend on the guess it starts from
    assert abs(reps[0].cycle.peak[0] - reps[2].cycle.peak[0]) <= norm * 2 * TOL + BAR * (reps[0].cycle.peak[0] - ambient)


def everything(rep):
    cyc = rep.cycle
    fields = [z.values for snap in cyc.temperatures for layer in snap for z in layer]
    return [cyc.times, cyc.total_stored, cyc.total_loss, cyc.total_heat, np.array([rep.closure]), np.array(rep.predicted),
            *[z.values for layer in cyc.envelope.temperatures for z in layer], *fields, *cyc.probes.values()]


@pytest.mark.parametrize("kind", ["interlayer", "heat_sources"])
def test_interlayer_heat_sources_segments_probes_and_the_same_bits_twice(ctx, kind):
    """``interlayer`` and ``heat_sources`` are honoured, one board each: the cycle balances with them (the sources' watts
    are part of the heat) and differs from the cycle without them.  ``keep="segments"`` keeps the field at the end of both
    segments, the probe's trace is the field at its vertex, and two calls give the same bits."""
    name = "two_layer" if kind == "interlayer" else "single"
    prob, meshes, layer_of, disc, *_ = board(name)
    extra = {"interlayer": {("F.Cu", "B.Cu"): 2e-3}} if kind == "interlayer" else \
        {"heat_sources": [solver.HeatSource.rectangle("F.Cu", 3, 3, 5, 5, 0.05, name="U1")]}
    probe = prob.networks[0].connections[0].node_id
    kw = dict(tolerance=TOL, probes=[probe], keep="segments", disconnected_meshes_by_layer=disc)
    _s, rep = quiet(solver.solve_meshed_thermal_periodic, prob, meshes, layer_of, model_of(**extra), public_cycle(TAU / 5), **kw)
    _s, twice = quiet(solver.solve_meshed_thermal_periodic, prob, meshes, layer_of, model_of(**extra), public_cycle(TAU / 5), **kw)
    _s, plain = quiet(solver.solve_meshed_thermal_periodic, prob, meshes, layer_of, model_of(), public_cycle(TAU / 5), **kw)
    cyc = rep.cycle
    with Stepping(name) as dev:
        sum_cv = float(dev.tr.capacity(dev.n_vert).sum())
    dts = np.diff(cyc.times)
    lost, put = float((dts * cyc.total_loss[1:]).sum()), float((dts * cyc.total_heat[1:]).sum())
    print(kind, "periods", rep.periods, "closure", rep.closure, "lost", lost, "put", put, "peak", cyc.peak[0], "without", plain.cycle.peak[0])
    assert rep.converged and abs(lost - put) <= TOL * sum_cv + 1e-9 * put
    if kind == "interlayer":                                                    # the dielectric spreads the hotspot's heat to the other layer
        assert abs(cyc.peak[0] - plain.cycle.peak[0]) > 1e-3
    else:                                                                       # 0.05 W while the case is on, and a warmer board for it
        put_plain = float((dts * plain.cycle.total_heat[1:]).sum())
        assert abs((put - put_plain) - 0.05 * 0.4 * TAU / 5) <= 1e-9 * put
        assert cyc.total_stored[0] > plain.cycle.total_stored[0] + 0.01 * 0.05 * TAU
    assert len(cyc.snapshot_times) == 2 and len(cyc.temperatures) == 2 and cyc.snapshot_times[1] == cyc.times[-1]
    assert list(cyc.probes) == [probe] and len(cyc.probes[probe]) == 15
    assert any(np.isclose(cyc.probes[probe][-1], z.values, rtol=0, atol=0).any() for layer in cyc.temperatures[1] for z in layer)
    assert all(np.array_equal(a, b) for a, b in zip(everything(rep), everything(twice)))
    assert rep.periods == twice.periods


def test_max_periods_ends_the_iteration_with_a_warning_and_the_best_cycle(ctx):
    prob, meshes, layer_of, disc, *_ = board(GRID49)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _s, rep = solver.solve_meshed_thermal_periodic(prob, meshes, layer_of, model_of(), public_cycle(), tolerance=TOL, max_periods=5,
                                                       disconnected_meshes_by_layer=disc)
    assert not rep.converged and rep.periods == 5 and len(rep.predicted) == 3 and rep.closure > TOL
    assert any(issubclass(w.category, solver.SolverWarning) and "periods" in str(w.message) for w in caught)
    assert len(rep.cycle.times) == 15 and abs(rep.closure - rep.predicted[-1]) <= BAR * (rep.cycle.peak[0] - 20.0 + 1.0)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_of_the_device_entries_leave_the_handles_usable(ctx):
    rng = np.random.default_rng(8)
    with Stepping("single") as dev:
        dev.tr.loads(*random_loads(dev, 1, 2))
        with pytest.raises(ValueError):
            _hip.Periodic(dev.tr, 4)                                            # not started
        dev.tr.start([None, None])
        for bad in (0, 4096):
            with pytest.raises(ValueError):
                _hip.Periodic(dev.tr, bad)
        per = _hip.Periodic(dev.tr, 2)
        lib = _hip.load_library()
        assert lib.padne_periodic_mark(dev.tr.ctx._h, None) == _hip.E_INVALID       # a null handle
        assert lib.padne_periodic_mark(None, per._h) == _hip.E_INVALID
        assert lib.padne_periodic_destroy(None) == _hip.OK
        S = rng.standard_normal((2, dev.n_pot))
        per.put(per.STATE, S)
        out_of_order = [per.residual, lambda: per.load(0), lambda: per.push(0), lambda: per.predict(np.zeros((2, 0))),
                        lambda: per.combine(np.zeros((2, 0))), lambda: per.vector(0), lambda: per.vector(per.R0),
                        lambda: per.put(1, S), lambda: per.put(-4, S)]
        for call in out_of_order:                                               # nothing is marked yet
            with pytest.raises(ValueError):
                call()
        assert np.array_equal(dev.tr.state(), S)
        per.mark()
        per.put(per.STATE, 2.0 * S)
        beta, _top, _vert = per.residual()
        for call in (lambda: per.load(1), lambda: per.load(-1), lambda: per.push(1), lambda: per.vector(1),
                     lambda: per.predict(np.zeros((2, 2))), lambda: per.combine(np.zeros((2, 2)))):
            with pytest.raises(ValueError):
                call()
        h = per.push(0)
        with pytest.raises(ValueError):
            per.push(1)                                                         # the basis of two is full
        with pytest.raises(ValueError):
            per.push(0)                                                         # not the newest vector
        dev.tr.start([None])                                                    # another number of columns: the handle is stale
        for call in (per.mark, per.residual, lambda: per.load(0)):
            with pytest.raises(ValueError):
                call()
        dev.tr.start([None, None])                                              # and usable again
        per.load(1)
        assert np.array_equal(dev.tr.state(), per.vector(1)) and (beta > 0.0).all() and np.isfinite(h).all()
        per.close()
        per.close()


def test_a_basis_that_does_not_fit_is_a_memory_error_not_a_fault(ctx):
    """4095 vectors of 4096 columns of the 49 x 49 board are 322 GB."""
    with Stepping(GRID49) as dev:
        dev.tr.loads(*random_loads(dev, 1, 2))
        dev.tr.start([None] * 4096)
        with pytest.raises(MemoryError):
            _hip.Periodic(dev.tr, 4095)
        small = _hip.Periodic(dev.tr, 1)                                        # the context is usable afterwards
        small.mark()
        small.close()

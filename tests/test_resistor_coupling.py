"""Resistors and vias whose resistance follows their temperature, on the device against the host restatement
(tests/resistor_coupling_ref.py, itself checked by tests/test_resistor_coupling_host.py): the resistors' scale, means, increment
and invalid-resistor report and the revalued system bit for bit; through the public calls the closed form of a via in series
with a current source, the fixed point and the round count against the restatement's loop, the balance, the direction of the
effect, load cases, repeatability and zero coefficients; the transient call against the host stepping; one public call under
the guarded pool; the refusals of the C ABI.

Boards: resistor_coupling_ref.strips_system -- two strips of 300 vertices joined by 300 resistors, 601 touched rows (two full
tiles of the row kernel and a ragged one), a parallel pair, a chain through an internal node, a resistor with both ends on one
unknown and a vertex with three resistors, one along a mesh edge -- and the goldens problem_mixed (4 resistors, an internal
node) and problem_c1 (291 resistors: a full tile of the scale kernel and a ragged one); for the public calls the boards of
coupled_ref.COUPLED_BOARDS and the series board of the restatement."""
import contextlib
import types

import numpy as np
import pytest

import coupled_ref as C
import resistor_coupling_ref as RC
import thermal_ref as T
from padne_amd import _hip, solver
from test_coupled import delivered_power, in_mesh_order, sigma_of
from test_coupled_transient import model_of as transient_model_of, one_step_segments, same, trace_arrays
from test_device_memory import leaves, three_ways
from test_film import distance_bound
from test_thermal import BAR, Device, board, quiet, sorted_csr
from test_transient import CAP, DT1, DT2, TAU, everything

pytestmark = pytest.mark.gpu

FILM = 1e-3
KERNEL_BOARDS = ["strips", "problem_mixed", "problem_c1"]
AMBIENT, T0 = 31.0, 20.0


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


@contextlib.contextmanager
def opened(ctx, name, n=300):
    """A board on the device with its thermal handle and a coupling handle: a namespace of ``L`` (the device matrix),
    ``thermal``, ``coupled``, the flattened mesh, ``sigma`` and ``face_alpha`` per mesh, and the resistors' ``a``, ``b``, ``R``.
    ``n``: the length of the strips of "strips" (tests/test_many_tiles.py takes long ones)."""
    if name == "strips":
        flat, sigma, n_vert, n_internal, rows = RC.strips_system(n)
        xy, tri, face_mesh, voff, toff = T.flatten(flat)
        n_pot = n_vert + n_internal
        L = ctx.assemble_system(n_pot, xy, np.concatenate([t for _xy, t in flat]), voff, toff, sigma, *RC.resistor_stamps(rows))
        linked = [row for row in rows if row[1] != row[2]]
        thermal = _hip.Thermal(L, n_pot, [3e-3, 2e-3], [FILM, 2 * FILM], [row[1] for row in linked], [row[2] for row in linked],
                               [0.01] * len(linked))
        stack = contextlib.ExitStack()
        stack.callback(L.close)
        stack.callback(thermal.close)
    else:
        stack = contextlib.ExitStack()
        dev = stack.enter_context(Device(name, FILM))
        L, thermal, xy, tri, face_mesh, sigma, n_pot = dev.L.dev, dev.thermal, dev.xy, dev.tri, dev.face_mesh, sigma_of(dev), dev.n_pot
        rows = [row for _e, row in dev.pairs if row[0] == "R"]
    with stack:
        face_alpha = [3.93e-3 * (1 + 0.25 * m) for m in range(len(sigma))]
        coupled = _hip.Coupled(L, thermal, face_alpha, AMBIENT, T0)
        stack.callback(coupled.close)
        yield types.SimpleNamespace(L=L, thermal=thermal, coupled=coupled, xy=xy, tri=tri, face_mesh=face_mesh, sigma=sigma,
                                    face_alpha=face_alpha, n_pot=n_pot, n_tri=len(tri), a=np.array([row[1] for row in rows]),
                                    b=np.array([row[2] for row in rows]), R=np.array([row[3] for row in rows]), n_res=len(rows))


def coefficients(d, rng):
    """(alpha, t0, theta, theta again) for the resistors of ``d``: coefficients of both signs, some exactly 0 (s_r exactly 1),
    a T0 per resistor; theta random, with resistor 3's ends at 10 and 30 K and its T0 at ambient + 20, so that 1 + alpha (T - T0)
    is exactly 1 with alpha not 0; the second theta puts the internal nodes, which no face sees, far from the first."""
    alpha = rng.uniform(-1e-3, 5e-3, d.n_res)
    alpha[::7] = 0.0
    t0 = rng.uniform(0.0, 40.0, d.n_res)
    thetas = [rng.uniform(0.0, 80.0, d.n_pot), rng.uniform(0.0, 80.0, d.n_pot)]
    k = min(3, d.n_res - 1)
    if d.a[k] != d.b[k]:
        thetas[0][d.a[k]], thetas[0][d.b[k]], t0[k], alpha[k] = 10.0, 30.0, AMBIENT + 20.0, 4e-3
    internal = np.array(sorted({int(i) for i in np.concatenate([d.a, d.b]) if i >= len(d.xy)}), dtype=np.int64)
    thetas[1][internal] = 700.0
    return alpha, t0, thetas, k


# ---- 1. the scale ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", KERNEL_BOARDS)
def test_scale_mean_increment_and_the_invalid_report_are_the_restatement_bit_for_bit(ctx, name):
    with opened(ctx, name) as d:
        rng = np.random.default_rng(31)
        alpha, t0, thetas, k = coefficients(d, rng)
        cp = d.coupled
        cp.set_resistors(d.a, d.b, d.R, alpha, t0)
        start, start_used = cp.get_resistors(d.n_res, means=True), cp.get_resistors(d.n_res, used=True)
        got = []
        for theta in thetas:
            inc = cp.update(theta)
            got.append((inc, *cp.get_resistors(d.n_res, means=True), cp.get_scale(d.n_tri, means=True)[1]))
        untouched = cp.get_resistors(d.n_res, used=True)
        cp.reset()
        after_reset = cp.get_resistors(d.n_res, means=True)
        again = cp.update(thetas[0])
        # the lowest invalid resistor is named; an invalid face comes first
        bad = alpha.copy()
        lo, hi = d.n_res // 2, d.n_res - 1
        bad[[lo, hi]] = -0.05
        cp.set_resistors(d.a, d.b, d.R, bad, np.full(d.n_res, T0))
        with pytest.raises(ValueError, match=rf"resistor {lo}\b"):
            cp.update(np.full(d.n_pot, 60.0))
        cp.set_resistors(d.a, d.b, d.R, np.full(d.n_res, 3.93e-3), np.full(d.n_res, T0))
        with pytest.raises(ValueError, match="face"):
            cp.update(np.full(d.n_pot, -1 / min(d.face_alpha) - 12.0))
    zeros = np.zeros(d.n_res)
    s0, mean0, _d = RC.resistor_scale(np.zeros(d.n_pot), d.a, d.b, alpha, AMBIENT, t0, zeros)
    assert np.array_equal(start[0], s0) and np.array_equal(start_used, s0) and (start[1] == 0.0).all()
    prev, prev_f = zeros, np.zeros(d.n_tri)
    for theta, (inc, s, mean, mean_f) in zip(thetas, got):
        s_want, mean_want, d_r = RC.resistor_scale(theta, d.a, d.b, alpha, AMBIENT, t0, prev)
        d_f = np.abs(C.face_means(d.tri, theta) - prev_f).max()
        assert np.array_equal(s, s_want) and np.array_equal(mean, mean_want)
        assert inc == max(d_f, d_r.max())
        prev, prev_f = mean_want, mean_f
    assert got[0][1][k] == 1.0 and alpha[k] != 0.0 and (got[0][1][::7] == 1.0).all()
    if len(d.xy) < d.n_pot:                                  # an internal node: the resistors' increment is the larger one
        assert got[1][0] > np.abs(C.face_means(d.tri, thetas[1]) - C.face_means(d.tri, thetas[0])).max()
    assert np.array_equal(untouched, s0)                     # the used scale moves with a revalue only
    assert np.array_equal(after_reset[0], s0) and (after_reset[1] == 0.0).all() and again == got[0][0]


# ---- 2. the revalued system ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", KERNEL_BOARDS)
def test_revalue_is_the_restatement_bit_for_bit(ctx, name):
    """Face scales in [0.5, 1.5] and the resistors' scales of a random theta at once: the values of the restatement, a symmetric
    potential block; every s_r == 1: the face-only revalue byte for byte; closed: the assembled values."""
    with opened(ctx, name) as d:
        rng = np.random.default_rng(32)
        alpha, t0, thetas, _k = coefficients(d, rng)
        s_f = rng.uniform(0.5, 1.5, d.n_tri)
        cp = d.coupled
        L0 = sorted_csr(d.L.to_scipy())

        def revalued(al):
            cp.set_resistors(d.a, d.b, d.R, al, t0)
            cp.update(thetas[0])
            cp.set_scale(s_f)
            cp.revalue()
            return sorted_csr(d.L.to_scipy()), cp.get_resistors(d.n_res, used=True) if len(al) else None

        L, used = revalued(alpha)
        L_again, _ = revalued(alpha)
        L_ones, used_ones = revalued(np.zeros(d.n_res))
        cp.set_resistors([], [], [], [], [])
        cp.update(thetas[0])
        cp.set_scale(s_f)
        cp.revalue()
        L_faces = sorted_csr(d.L.to_scipy())
        with pytest.raises(ValueError):
            cp.get_resistors(d.n_res)
        cp.set_resistors(d.a, d.b, d.R, alpha, t0)
        cp.revalue()
        cp.close()
        L_after = sorted_csr(d.L.to_scipy())
    sr, _mean, _d = RC.resistor_scale(thetas[0], d.a, d.b, alpha, AMBIENT, t0, np.zeros(d.n_res))
    faces = C.revalue(L0, d.xy, d.tri, d.face_mesh, d.sigma, s_f)
    want = RC.revalue_resistors(faces, RC.places(L0, d.a, d.b), sr, 1 / d.R)
    assert np.array_equal(used, sr) and (used_ones == 1.0).all()
    assert np.array_equal(L.indices, L0.indices) and np.array_equal(L.data, want.data) and np.array_equal(L_again.data, L.data)
    assert (want != faces).nnz > 0
    K = L[:d.n_pot, :d.n_pot]
    assert (K != K.T).nnz == 0
    assert L_ones.data.tobytes() == L_faces.data.tobytes() == faces.data.tobytes()
    assert np.array_equal(L_after.data, L0.data)
    if name == "strips":                                     # faces and resistors meet on the entries of the mesh edge 20 - 21
        assert faces[20, 21] != L0[20, 21] and L[20, 21] != faces[20, 21] and L[20, 21] == L[21, 20]


# ---- 3. through the public call --------------------------------------------------------------------------------------------

def follows(film, coefficient=RC.COPPER, **kw):
    return solver.ElectroThermalModel(thermal=solver.ThermalModel(film=film), resistor_coefficient=coefficient, **kw)


def balanced(rep, coupling):
    """total_loss and total_heat against what the sources deliver, the bar of tests/test_coupled.py."""
    delivered = delivered_power(coupling.elements)
    assert delivered > 0
    assert abs(rep.total_loss - delivered) <= 1e-9 * delivered and abs(rep.total_heat - delivered) <= 1e-9 * delivered


def test_the_series_via_meets_its_closed_form(ctx):
    """rho = alpha I^2 R0 Z = 0.3 at a tolerance of 1e-6 K: the via's heat and temperature against the closed form of
    tests/test_resistor_coupling_host.py within BAR of the value plus what the stop leaves (the last solve used the scale of the
    iterate before the last, within d / (1 - rho) of the fixed point)."""
    current = RC.series_current(0.3)
    prob, meshes, layer_of, via = RC.series_problem(current)
    model = RC.series_model(1e-6, max_rounds=40)
    _sol, rep, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model)
    _c0, _Z, rho, p, T_r = RC.series_closed_form(RC.host_board(prob, meshes, layer_of, model), current)
    state, flow = coupling.resistors[via], coupling.elements[via]
    print("rounds", coupling.rounds, "p", flow["power"], "p*", p, "T_r", state["temperature"], "T_r*", T_r, "I", flow["current"])
    assert coupling.converged and coupling.rounds > 5 and list(coupling.resistors) == [via]
    joule = current * current * RC.SERIES_R0
    assert abs(flow["power"] - p) <= BAR * p + RC.COPPER * joule * 1e-6 / (1 - rho)
    assert abs(state["temperature"] - T_r) <= BAR * T_r + 1e-6 / (1 - rho)
    assert abs(abs(flow["current"]) - current) <= 1e-8 * current
    assert state["resistance"] == RC.SERIES_R0 / state["scale"]
    assert abs(state["resistance"] - RC.SERIES_R0 * (1 + RC.COPPER * (T_r - RC.SERIES_T0))) <= RC.SERIES_R0 * RC.COPPER * (BAR * T_r + 1e-6 / (1 - rho))
    balanced(rep, coupling)
    with pytest.raises(solver.ThermalRunawayError):
        prob, meshes, layer_of, _via = RC.series_problem(RC.series_current(1.2))
        quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, RC.series_model(1e-6))


@pytest.mark.parametrize("name", sorted(C.COUPLED_BOARDS))
def test_the_fixed_point_and_the_rounds_are_the_restatements(ctx, name):
    """The device loop at 1e-6 K against the restatement iterated to 1e-12 K: theta within BAR of the rise plus d rho / (1 -
    rho) of the device's own increments; the rounds and the increments are those of the restatement stopped at 1e-6 K; the
    resistors' scales of the last solve within alpha times that distance; the case balances."""
    film, factor = C.COUPLED_BOARDS[name]
    prob, meshes, layer_of, disc, *_ = board(name)
    model, case = follows(film, tolerance=1e-6), C.scaled_case(prob, factor)
    _sols, reps, couplings, _env = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model, cases=[case],
                                         disconnected_meshes_by_layer=disc)
    rep, coupling = reps[0], couplings[0]
    B = RC.host_board(prob, meshes, layer_of, model, case)
    fine, same_stop = B.picard(1e-12), B.picard(1e-6)
    theta = in_mesh_order(rep.temperatures, layer_of) - 25.0
    rise = np.abs(fine["theta"]).max()
    err = np.abs(theta - fine["theta"][:B.board.n_vert]).max()
    print(name, "rounds", coupling.rounds, "increments", coupling.increments, "err", err, "bound", distance_bound(coupling.increments, rise))
    assert coupling.converged and fine["converged"] and coupling.rounds == len(same_stop["increments"]) > 2
    assert err <= distance_bound(coupling.increments, rise)
    for got, want in zip(coupling.increments, same_stop["increments"]):
        assert abs(got - want) <= BAR * rise
    resistors = [e for e, row in board(name)[6] if row[0] == "R"]
    assert list(coupling.resistors) == resistors
    scales = np.array([coupling.resistors[e]["scale"] for e in resistors])
    rho = coupling.increments[-1] / coupling.increments[-2]
    assert np.abs(scales - fine["resistor_scale"]).max() <= RC.COPPER * (coupling.increments[-1] / (1 - rho) + BAR * rise)
    assert (scales < 1.0).all() and all(coupling.resistors[e]["resistance"] == e.resistance / coupling.resistors[e]["scale"] for e in resistors)
    balanced(rep, coupling)


def test_a_warm_via_drops_more_under_a_current_and_dissipates_less_under_a_voltage(ctx):
    current = RC.series_current(0.3)
    prob, meshes, layer_of, via = RC.series_problem(current)
    out = {}
    for key, coefficient in (("warm", RC.COPPER), ("cold", None)):
        model = solver.ElectroThermalModel(thermal=solver.ThermalModel(film=RC.SERIES_FILM, ambient=RC.SERIES_AMBIENT),
                                           temperature_coefficient=0.0, conductance_temperature=RC.SERIES_T0,
                                           resistor_coefficient=coefficient, max_rounds=40)
        _sol, _rep, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model)
        out[key] = coupling.elements[via]
    drop = lambda flow: abs(flow["power"] / flow["current"])                                                  # noqa: E731
    print("current-driven: drop", drop(out["cold"]), "->", drop(out["warm"]), "heat", out["cold"]["power"], "->", out["warm"]["power"])
    assert drop(out["warm"]) > 1.2 * drop(out["cold"]) and out["warm"]["power"] > 1.2 * out["cold"]["power"]
    prob, meshes, layer_of, via = RC.series_problem(0.0, voltage=0.1)
    for key, coefficient in (("warm", RC.COPPER), ("cold", None)):
        model = solver.ElectroThermalModel(thermal=solver.ThermalModel(film=RC.SERIES_FILM, ambient=RC.SERIES_AMBIENT),
                                           temperature_coefficient=0.0, conductance_temperature=RC.SERIES_T0,
                                           resistor_coefficient=coefficient, max_rounds=40)
        _sol, rep, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model)
        out[key] = coupling.elements[via]
        assert coupling.converged
    print("voltage-driven: heat", out["cold"]["power"], "->", out["warm"]["power"])
    assert abs(out["cold"]["power"] - 0.1 * 0.1 / RC.SERIES_R0) <= 1e-8 * out["cold"]["power"]
    assert out["warm"]["power"] < out["cold"]["power"] / 1.2


def test_two_load_cases_one_of_them_dead(ctx):
    film, factor = C.COUPLED_BOARDS["two_layer"]
    prob, meshes, layer_of, *_ = board("two_layer")
    live = C.scaled_case(prob, factor)
    dead = {e: 0.0 for e in live}
    model = solver.ElectroThermalModel(thermal=solver.ThermalModel(film=film, ambient=40.0), resistor_coefficient=RC.COPPER)
    _s, reps, couplings, _env = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model, cases=[live, dead])
    assert couplings[0].converged and couplings[0].rounds > 1
    balanced(reps[0], couplings[0])
    s0 = 1 / (1 + RC.COPPER * ((0.0 + 40.0) - 20.0))
    assert couplings[1].rounds == 1 and couplings[1].converged and couplings[1].increments == [0.0]
    assert all(state == {"temperature": 40.0, "scale": s0, "resistance": e.resistance / s0} for e, state in couplings[1].resistors.items())
    assert len(couplings[1].resistors) == 8 and reps[1].total_heat == 0.0
    # the live case is what it is alone: the second case starts from resistors at ambient again
    _s, alone, c_alone, _e = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model, cases=[dead, live])
    assert c_alone[1].increments == couplings[0].increments and c_alone[1].resistors == couplings[0].resistors
    assert leaves(alone[1].temperatures) == leaves(reps[0].temperatures)


def steady(name, coefficient):
    film, factor = C.COUPLED_BOARDS[name]
    prob, meshes, layer_of, disc, *_ = board(name)
    return quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, follows(film, coefficient), cases=[C.scaled_case(prob, factor)],
                 disconnected_meshes_by_layer=disc)


def test_two_calls_give_the_same_bits_and_zero_coefficients_those_of_none(ctx):
    a, b = steady("two_layer", RC.COPPER), steady("two_layer", RC.COPPER)
    assert leaves(a) == leaves(b) and a[2][0].rounds > 2
    none, zero = steady("problem_mixed", None), steady("problem_mixed", 0.0)
    resistors = [e for e, row in board("problem_mixed")[6] if row[0] == "R"]
    named = steady("problem_mixed", {e: 0.0 for e in resistors})
    assert none[2][0].resistors == {} and none[2][0].rounds > 1
    for got in (zero, named):
        assert all(state["scale"] == 1.0 and state["resistance"] == e.resistance for e, state in got[2][0].resistors.items())
        assert list(got[2][0].resistors) == resistors
        got[2][0].resistors = {}
        assert leaves(got) == leaves(none)


# ---- 4. transient ----------------------------------------------------------------------------------------------------------

SCHEDULE = [(DT1, 6, 0), (DT2, 4, 0), (DT2, 4, None)]
_RUNS: dict = {}


def transient_run(name):
    """One run of SCHEDULE per board, shared by the tests: (the arguments, the report, the trace, the host stepping)."""
    if name not in _RUNS:
        film, factor = C.COUPLED_BOARDS[name]
        prob, meshes, layer_of, disc, *_ = board(name)
        case = C.scaled_case(prob, factor)
        model = transient_model_of(film, resistor_coefficient=RC.COPPER)
        _sols, rep, trace = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, model,
                                  one_step_segments(SCHEDULE), cases=[case], keep="segments", disconnected_meshes_by_layer=disc)
        B = RC.host_board(prob, meshes, layer_of, model.electrothermal, case)
        want = B.run([CAP] * len(meshes), [(dt, steps, j is not None) for dt, steps, j in SCHEDULE])
        _RUNS[name] = ((prob, meshes, layer_of), rep, trace, B, want)
    return _RUNS[name]


@pytest.mark.parametrize("name", ["two_layer", "problem_mixed"])
def test_the_trajectory_against_the_host_stepping(ctx, name):
    """Every step's theta within BAR of the run's largest |theta| of the restatement, the bar and the argument of
    tests/test_coupled_transient.py; the increments likewise; the range of the resistors' scales within alpha times that."""
    (_prob, _meshes, layer_of), rep, trace, B, want = transient_run(name)
    top = np.abs(want.states).max()
    err = [np.abs(in_mesh_order(fields, layer_of) - 25.0 - want.states[n + 1, :B.board.n_vert]).max()
           for n, fields in enumerate(rep.temperatures)]
    print(name, "worst error / max|theta|", max(err) / top, "max theta", top, "resistor scales", trace.resistor_scale_min[1:4])
    assert len(err) == 14 and top > 5.0 and max(err) <= BAR * top
    on = ~np.isnan(want.increments)
    assert np.array_equal(np.isnan(trace.increments), ~on) and np.array_equal(np.isnan(trace.resistor_scale_min), np.isnan(want.resistor_min))
    assert np.abs(trace.increments[on] - want.increments[on]).max() <= BAR * top
    live = ~np.isnan(want.resistor_min)
    assert np.abs(trace.resistor_scale_min[live] - want.resistor_min[live]).max() <= RC.COPPER * BAR * top
    assert np.abs(trace.resistor_scale_max[live] - want.resistor_max[live]).max() <= RC.COPPER * BAR * top
    assert (np.diff(trace.resistor_scale_min[1:11]) < 0).all()          # the resistors warm from step to step


@pytest.mark.parametrize("name", ["two_layer", "problem_mixed"])
def test_every_step_balances_against_its_own_electrical_solve(ctx, name):
    """(stored' - stored) / dt + loss' - total_heat' within 1e-9 of the run's largest heat, and total_heat within 1e-9 relative
    of what the sources deliver in that step's solve: the bars of tests/test_coupled_transient.py."""
    _args, rep, trace, _B, _want = transient_run(name)
    defect = (rep.total_stored[1:] - rep.total_stored[:-1]) / np.diff(rep.times) + rep.total_loss[1:] - rep.total_heat[1:]
    top = rep.total_heat.max()
    gap = np.abs(rep.total_heat[1:11] - trace.delivered[1:11])
    print(name, "largest heat", top, "worst defect / heat", np.abs(defect).max() / top, "heat against delivered", (gap / trace.delivered[1:11]).max())
    assert top > 0 and (np.abs(defect) <= 1e-9 * top).all()
    assert (trace.delivered[1:11] > 0).all() and (gap <= 1e-9 * trace.delivered[1:11]).all()
    assert (rep.total_heat[11:] == 0.0).all() and len(set(rep.total_heat[1:11].tolist())) == 10


def test_zero_coefficients_have_the_bits_of_todays_transient(ctx):
    film, factor = C.COUPLED_BOARDS["two_layer"]
    prob, meshes, layer_of, *_ = board("two_layer")
    schedule = [solver.Segment(3 * DT1, 3, 0), solver.Segment(2 * DT2, 2, None), solver.Segment(2 * DT2, 2, 0)]
    runs = [quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, transient_model_of(film, **kw), schedule,
                  cases=[C.scaled_case(prob, factor)], keep="segments") for kw in ({}, dict(resistor_coefficient=0.0))]
    (_sa, rep_a, trace_a), (_sb, rep_b, trace_b) = runs
    (arrays_a, scalars_a), (arrays_b, scalars_b) = everything(rep_a), everything(rep_b)
    assert scalars_a == scalars_b and same(arrays_a, arrays_b) and same(trace_arrays(trace_a), trace_arrays(trace_b))
    on = np.array([False] + [True] * 3 + [False] * 2 + [True] * 2)
    assert trace_a.resistor_scale_min is None and trace_a.resistor_scale_max is None and (trace_b.resistor_scale_min[on] == 1.0).all()
    assert (trace_b.resistor_scale_max[on] == 1.0).all() and np.isnan(trace_b.resistor_scale_max[~on]).all()


def test_a_long_on_leg_ends_at_the_steady_fixed_point(ctx):
    """The series via at rho = 0.3 under 30 steps of 10 tau: the lagged scale converges like the Picard loop (a factor of about
    rho / (1 + 0.1) a step), so the end is within the steady call's own gap, 1e-6 rho / (1 - rho), plus BAR of the rise."""
    current = RC.series_current(0.3)
    prob, meshes, layer_of, via = RC.series_problem(current)
    electro = RC.series_model(1e-6, max_rounds=40)
    model = solver.ElectroThermalTransientModel(electrothermal=electro, areal_capacity=CAP)
    _sols, rep, trace = quiet(solver.solve_meshed_electrothermal_transient, prob, meshes, layer_of, model,
                              one_step_segments([(10 * TAU, 30, 0)]))
    _sol, held, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, electro)
    end, want = in_mesh_order(rep.temperatures[-1], layer_of), in_mesh_order(held.temperatures, layer_of)
    rise = want.max() - RC.SERIES_AMBIENT
    print("rise", rise, "gap", np.abs(end - want).max(), "resistor scale", trace.resistor_scale_min[-1], coupling.resistors[via]["scale"])
    assert coupling.converged and rise > 50.0
    assert np.abs(end - want).max() <= 1e-6 * 0.3 / 0.7 + BAR * rise
    assert abs(trace.resistor_scale_min[-1] - coupling.resistors[via]["scale"]) <= RC.COPPER * (1e-6 / 0.7 + BAR * rise)
    assert trace.resistor_scale_min[-1] == trace.resistor_scale_max[-1]


# ---- 5. under the guarded pool ---------------------------------------------------------------------------------------------

def driver():
    film, factor = C.COUPLED_BOARDS["two_layer"]
    prob, meshes, layer_of, *_ = board("two_layer")
    schedule = [solver.Segment(2 * DT1, 2, 0), solver.Segment(DT2, 1, None), solver.Segment(DT2, 1, 0)]
    return solver.solve_meshed_electrothermal_transient(prob, meshes, layer_of,
                                                        transient_model_of(film, initial=0, resistor_coefficient=RC.COPPER), schedule,
                                                        cases=[C.scaled_case(prob, factor)], keep="segments")


def test_the_public_call_under_the_guarded_pool(ctx, switches):
    three_ways(ctx, switches, driver)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals_through_the_c_abi(ctx):
    """Each is PADNE_E_INVALID (a ValueError here) and leaves the handle with the resistors it had."""
    lib = ctx._lib
    with opened(ctx, "strips") as d:
        cp, n = d.coupled, d.n_res
        alpha, t0 = np.full(n, 3.93e-3), np.full(n, T0)
        cp.set_resistors(d.a, d.b, d.R, alpha, t0)
        cp.update(np.full(d.n_pot, 10.0))
        held = cp.get_resistors(n, means=True)

        def with_one(array, k, value):
            out = np.array(array, dtype=np.float64 if array is not d.a and array is not d.b else np.int64)
            out[k] = value
            return out

        for args in ((with_one(d.a, 2, -1), d.b, d.R, alpha, t0), (d.a, with_one(d.b, 2, d.n_pot), d.R, alpha, t0),
                     (d.a, d.b, with_one(d.R, 0, 0.0), alpha, t0), (d.a, d.b, with_one(d.R, 0, -1.0), alpha, t0),
                     (d.a, d.b, with_one(d.R, n - 1, float("inf")), alpha, t0), (d.a, d.b, with_one(d.R, 1, float("nan")), alpha, t0),
                     (d.a, d.b, d.R, with_one(alpha, 5, float("nan")), t0), (d.a, d.b, d.R, alpha, with_one(t0, 5, float("inf"))),
                     (d.a, d.b, d.R, with_one(alpha, 5, -1.0), t0),                 # 1 + alpha (ambient - T0) < 0
                     (with_one(d.a, 0, 0), with_one(d.b, 0, 250), d.R, alpha, t0),  # no stored entry (0, 250)
                     (d.a[:-1], d.b, d.R, alpha, t0)):
            with pytest.raises(ValueError):
                cp.set_resistors(*args)
        with pytest.raises(ValueError, match="no stored entry"):
            cp.set_resistors([0], [250], [0.01], [0.0], [T0])
        for count in (n - 1, n + 1, 0):
            with pytest.raises(ValueError):
                cp.get_resistors(count)
        null = _hip._P()
        assert lib.padne_coupled_set_resistors(ctx._h, null, 0, None, None, None, None, None) == _hip.E_INVALID
        assert lib.padne_coupled_set_resistors(ctx._h, cp._h, 1, None, None, None, None, None) == _hip.E_INVALID
        assert lib.padne_coupled_get_resistors(ctx._h, cp._h, 2, n, None, None) == _hip.E_INVALID
        assert lib.padne_coupled_get_resistors(ctx._h, cp._h, 0, n, None, None) == _hip.E_INVALID
        after = cp.get_resistors(n, means=True)
        assert np.array_equal(after[0], held[0]) and np.array_equal(after[1], held[1])
        cp.revalue()                                         # and the handle still works
        assert np.array_equal(cp.get_resistors(n, used=True), held[0])

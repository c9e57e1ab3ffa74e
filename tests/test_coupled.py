"""The electro-thermal coupling on the device against the host restatement (tests/coupled_ref.py, itself checked by
tests/test_coupled_host.py): the revalued system, the scale and the scaled face powers bit for bit; alpha = 0 against the
one-way path; the uniform strip's closed form through the Problem API; the fixed point against the restatement's; the balance;
the direction of the effect; load cases; repeatability and refusals.

Boards: those of tests/test_thermal.py -- one jittered 17 x 17 mesh (289 vertices: more than a wave and more than a workgroup,
a ragged last tile), two layers with a via lattice and an internal node, a 2-face mesh next to a large one, the goldens.
Films and source factors of the coupled runs: coupled_ref.COUPLED_BOARDS (rises of tens of kelvin, rho about 0.1)."""
import math
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import coupled_ref as C
import helpers as H
import thermal_ref as T
from padne_amd import _hip, mesh, problem as P, solver, synthetic
from test_load_case_currents import finished_block
from test_thermal import BAR, BOARDS, Device, board, quiet, scalars, vertex_temperatures

pytestmark = pytest.mark.gpu

FILM = 1e-3


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def sorted_csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def alphas(dev):
    """A coefficient per mesh, all different."""
    return [3.93e-3 * (1 + 0.25 * m) for m in range(len(dev.flat))]


def sigma_of(dev):
    return [dev.prob.layers[l].conductance for l in dev.layer_of]


def model_of(film=FILM, ambient=25.0, **kw):
    return solver.ElectroThermalModel(thermal=solver.ThermalModel(film=film, ambient=ambient), **kw)


# ---- 1. the revalued system ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOARDS)
def test_revalue_is_the_restatement_bit_for_bit(ctx, name):
    """Random s in [0.5, 1.5]: the values of the restatement, a symmetric stiffness block; s = 1: the assembled bits; after
    the handle is closed the system holds the assembled values again."""
    with Device(name, FILM) as dev:
        L0 = sorted_csr(dev.L.dev.to_scipy())
        coupled = _hip.Coupled(dev.L.dev, dev.thermal, alphas(dev), 25.0, 20.0)
        try:
            s = np.random.default_rng(2).uniform(0.5, 1.5, dev.n_tri)
            coupled.set_scale(s)
            coupled.revalue()
            L = sorted_csr(dev.L.dev.to_scipy())
            assert np.array_equal(coupled.get_scale(dev.n_tri, used=True), s)
            coupled.set_scale(np.ones(dev.n_tri))
            coupled.revalue()
            L1 = sorted_csr(dev.L.dev.to_scipy())
            coupled.set_scale(s)
            coupled.revalue()
        finally:
            coupled.close()
        L_after = sorted_csr(dev.L.dev.to_scipy())
    want = C.revalue(L0, dev.xy, dev.tri, dev.face_mesh, sigma_of(dev), s)
    assert H.same_structure(L, L0) and np.array_equal(L.data, want.data)
    assert (L != L0).nnz > 0
    K = L[:dev.n_vert, :dev.n_vert]
    assert (K != K.T).nnz == 0
    assert np.array_equal(L1.data, L0.data)
    assert np.array_equal(L_after.data, L0.data)


# ---- 2. the scale ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["single", "two_in_layer", "problem_many_meshes"])
def test_scale_means_and_increment_are_the_restatement_bit_for_bit(ctx, name):
    """From a theta the test uploads (random, no two entries alike): s, the face means and d = max |mean - previous mean|,
    first against the means 0 of a fresh handle, then against the first upload's; after a reset against 0 again."""
    with Device(name, FILM) as dev:
        alpha = alphas(dev)
        coupled = _hip.Coupled(dev.L.dev, dev.thermal, alpha, 31.0, 20.0)
        try:
            s_start = coupled.get_scale(dev.n_tri)
            rng = np.random.default_rng(8)
            thetas = [rng.uniform(0.0, 80.0, dev.n_pot), rng.uniform(0.0, 80.0, dev.n_pot)]
            got = []
            for theta in thetas:
                d = coupled.update(theta)
                got.append((d, *coupled.get_scale(dev.n_tri, means=True)))
            coupled.reset()
            s_reset, mean_reset = coupled.get_scale(dev.n_tri, means=True)
            d_again = coupled.update(thetas[0])
            with pytest.raises(ValueError, match="face"):                   # 1 + alpha (T - T0) <= 0 on the hottest faces
                coupled.update(np.full(dev.n_pot, -1 / min(alpha) - 12.0))
        finally:
            coupled.close()
    prev = np.zeros(dev.n_tri)
    for theta, (d, s, mean) in zip(thetas, got):
        s_want, mean_want = C.scale(dev.tri, dev.face_mesh, alpha, 31.0, 20.0, theta)
        assert np.array_equal(mean, mean_want) and np.array_equal(s, s_want)
        assert d == np.abs(mean_want - prev).max()
        prev = mean_want
    s0, _ = C.scale(dev.tri, dev.face_mesh, alpha, 31.0, 20.0, np.zeros(dev.n_pot))
    assert np.array_equal(s_start, s0) and np.array_equal(s_reset, s0) and (mean_reset == 0.0).all()
    assert d_again == got[0][0]


# ---- 3. the scaled face powers and power densities -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_layer", "two_in_layer", "problem_many_meshes"])
def test_scaled_face_powers_are_the_restatement_bit_for_bit(ctx, name):
    """On the block solved with the revalued system: the face powers the thermal handle holds after padne_coupled_solve_kkt
    and the scaled power densities, against the restatement on the block's own potentials; with s = 1 the bits of
    padne_thermal_solve_kkt's face powers and theta, and of padne_kkt_power_density_block."""
    with Device(name, FILM) as dev:
        coupled = _hip.Coupled(dev.L.dev, dev.thermal, alphas(dev), 25.0, 20.0)
        try:
            s = np.random.default_rng(5).uniform(0.5, 1.5, dev.n_tri)
            coupled.set_scale(s)
            coupled.revalue()
            plan, V = finished_block(dev.board, dev.L, dev.cases)
            try:
                theta, _ = coupled.solve_kkt(plan)
                Pf = dev.thermal.face_power(1, dev.n_tri)
                density = coupled.power_density(plan, dev.n_tri)
                theta_fed, _ = dev.thermal.solve(Pf)
            finally:
                plan.close()
            coupled.set_scale(np.ones(dev.n_tri))
            coupled.revalue()
            plan, V1 = finished_block(dev.board, dev.L, dev.cases)
            try:
                theta_1, _ = coupled.solve_kkt(plan)
                Pf_1 = dev.thermal.face_power(1, dev.n_tri)
                density_1 = coupled.power_density(plan, dev.n_tri)
                theta_plain, _ = dev.thermal.solve_kkt(plan, 1)
                Pf_plain = dev.thermal.face_power(1, dev.n_tri)
                density_plain = plan.power_density_block(1, dev.n_tri)
            finally:
                plan.close()
        finally:
            coupled.close()
    sigma = sigma_of(dev)
    assert np.array_equal(Pf[0], C.face_power(dev.xy, dev.tri, dev.face_mesh, sigma, s, V[:dev.n_vert, 0]))
    assert np.array_equal(density, C.power_density(dev.flat, sigma, s, V[:dev.n_vert, 0]))
    assert np.array_equal(theta, theta_fed)
    assert np.array_equal(Pf_1, Pf_plain) and np.array_equal(theta_1, theta_plain) and np.array_equal(density_1, density_plain[0])
    assert np.array_equal(Pf_plain[0], T.face_power(dev.xy, dev.tri, dev.face_mesh, sigma, V1[:dev.n_vert, 0]))


# ---- 4. alpha = 0 ------------------------------------------------------------------------------------------------------------

def solution_arrays(sol):
    return [a for ls in sol.layer_solutions for forms in (ls.potentials, ls.power_densities) for a in (f.values for f in forms)]


def report_arrays(rep):
    return vertex_temperatures(rep) + [tf.values for forms in rep.face_temperatures for tf in forms]


@pytest.mark.parametrize("name", ["single", "two_layer", "problem_many_meshes"])
def test_alpha_zero_is_the_one_way_path_bit_for_bit(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    kw = dict(disconnected_meshes_by_layer=disc)
    sol_w, rep_w = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(film=FILM), **kw)
    sol, rep, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of,
                               model_of(temperature_coefficient=0.0, conductance_temperature=-40.0), **kw)
    assert coupling.rounds == 1 and coupling.converged and len(coupling.increments) == 1
    assert all((tf.values == 1.0).all() for forms in coupling.conductance_scale for tf in forms)
    a, b = solution_arrays(sol), solution_arrays(sol_w)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    a, b = report_arrays(rep), report_arrays(rep_w)
    assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert scalars(rep) == scalars(rep_w)


# ---- 5. the uniform strip through the Problem API ------------------------------------------------------------------------

def strip_problem(alpha_theta0):
    layer = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=C.STRIP_SIGMA)
    xy, tri = synthetic.jittered_grid(C.STRIP_N, C.STRIP_N, h=C.STRIP_H, seed=0, jitter=0.0)
    msh = mesh.Mesh(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3))
    connections, elements = [], []
    for f, t, current in C.strip_sources(C.strip_current_density(alpha_theta0)):
        a = P.Connection(layer=layer, point=H.XY(*msh.points[f]))
        b = P.Connection(layer=layer, point=H.XY(*msh.points[t]))
        connections += [a, b]
        elements.append(P.CurrentSource(f=a.node_id, t=b.node_id, current=current))
    return P.Problem(layers=[layer], networks=[P.Network(connections=connections, elements=elements)]), [msh], [0]


def test_the_uniform_strip_follows_the_closed_form(ctx):
    """alpha theta0 = 0.3, theta0 = 76.3 K, tolerance 1e-4 K: 13 rounds (d_12 = 1.4e-4, d_13 = 4.1e-5); the increments and the
    last iterate against the closed form within BAR of the largest theta."""
    prob, meshes, layer_of = strip_problem(0.3)
    model = model_of(ambient=20.0, tolerance=1e-4)
    _sol, rep, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model)
    thetas, increments, fixed = C.strip_closed_form(0.3, 13)
    theta = vertex_temperatures(rep)[0] - 20.0
    print("rounds", coupling.rounds, "theta", theta.min(), theta.max(), "closed form", thetas[-1], "fixed point", fixed)
    assert coupling.converged and coupling.rounds == 13
    assert np.abs(np.array(coupling.increments) - np.array(increments)).max() <= BAR * fixed
    assert np.abs(theta - thetas[-1]).max() <= BAR * fixed
    assert np.abs(theta - fixed).max() <= 1e-4 * 0.3 / 0.7 + BAR * fixed


def test_the_uniform_strip_runs_away(ctx):
    prob, meshes, layer_of = strip_problem(1.2)
    with pytest.raises(solver.ThermalRunawayError, match="F.Cu") as info:
        quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model_of(ambient=20.0))
    assert "rounds 1 to 4" in str(info.value)


# ---- 6. the fixed point against the restatement ---------------------------------------------------------------------------

def in_mesh_order(by_layer, layer_of) -> np.ndarray:
    """The per-layer, per-mesh arrays of a report, concatenated in mesh order (the order of the global unknowns)."""
    by_mesh = {}
    for layer_i, forms in enumerate(by_layer):
        indices = [i for i, l in enumerate(layer_of) if l == layer_i]
        assert len(indices) == len(forms)
        by_mesh.update(zip(indices, (f.values for f in forms)))
    return np.concatenate([by_mesh[i] for i in range(len(layer_of))])


def coupled_run(name, tolerance=None, boards=C.COUPLED_BOARDS, **kw):
    film, factor = boards[name]
    prob, meshes, layer_of, disc, *_ = board(name)
    model = model_of(film) if tolerance is None else model_of(film, tolerance=tolerance)
    case = C.scaled_case(prob, factor)
    sols, reps, couplings, env = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model, cases=[case],
                                       disconnected_meshes_by_layer=disc, **kw)
    return (prob, meshes, layer_of, model, case), sols[0], reps[0], couplings[0], env


@pytest.mark.parametrize("name", sorted(C.COUPLED_BOARDS))
def test_the_fixed_point_is_the_restatements(ctx, name):
    """The device loop at a tolerance of 1e-6 K against the restatement iterated to 1e-12 K with direct solves: the vertex
    temperatures within tolerance * rho / (1 - rho) + BAR * max |theta|, rho the contraction of the restatement's own
    increments; the potentials within 1e-8 of their largest."""
    (prob, meshes, layer_of, model, case), sol, rep, coupling, _env = coupled_run(name, tolerance=1e-6)
    B = C.host_board(prob, meshes, layer_of, model, case)
    want = B.picard(1e-12)
    rho = C.contraction(want["increments"])
    theta = in_mesh_order(rep.temperatures, layer_of) - 25.0
    V = in_mesh_order([ls.potentials for ls in sol.layer_solutions], layer_of)
    gap_t = np.abs(theta - want["theta"][:B.n_vert]).max()
    gap_v = np.abs(V - want["V"][:B.n_vert]).max()
    top = np.abs(want["theta"]).max()
    print(name, "rounds", coupling.rounds, "rho", rho, "theta gap", gap_t, "allowed", 1e-6 * rho / (1 - rho) + BAR * top,
          "V gap / max|V|", gap_v / np.abs(want["V"][:B.n_vert]).max())
    assert coupling.converged and rho < 0.5
    assert gap_t <= 1e-6 * rho / (1 - rho) + BAR * top
    assert gap_v <= 1e-8 * np.abs(want["V"][:B.n_vert]).max()
    # the scale the last electrical solve used comes from the iterate before the last, within d / (1 - rho) of the fixed
    # point, and |ds| <= alpha |dT| while s <= 1 (the copper is warmer than T0)
    scale = in_mesh_order(coupling.conductance_scale, layer_of)
    assert np.abs(scale - want["scale"]).max() <= 3.93e-3 * (1e-6 / (1 - rho) + BAR * top)


# ---- 7. balance -------------------------------------------------------------------------------------------------------------

def delivered_power(elements) -> float:
    terms = []
    for element, flow in elements.items():
        if solver.element_kind(element) != "Resistor":
            terms += [-flow["power"], -flow.get("input_power", 0.0)]
    return math.fsum(terms)


@pytest.mark.parametrize("name", BOARDS)
def test_the_film_loss_is_the_power_the_sources_deliver(ctx, name):
    """At the last round, total_loss and total_heat equal the power the sources deliver within 1e-9 relative (the bar of
    test_thermal.py): the thermal load came from the last electrical solve with the same scale."""
    boards = dict(C.COUPLED_BOARDS, **C.OTHER_BOARDS)
    _args, _sol, rep, coupling, _env = coupled_run(name, boards=boards)
    delivered = delivered_power(coupling.elements)
    print(name, "rounds", coupling.rounds, "delivered", delivered, "heat", rep.total_heat, "loss", rep.total_loss)
    assert coupling.converged and coupling.rounds > 1 and delivered > 0
    assert abs(rep.total_loss - delivered) <= 1e-9 * delivered
    assert abs(rep.total_heat - delivered) <= 1e-9 * delivered


# ---- 8. the direction of the effect ------------------------------------------------------------------------------------------

def hottest(rep):
    return max(spot[0] for spot in rep.hotspots if spot is not None)


def test_warm_copper_dissipates_more_under_a_current_and_less_under_a_voltage(ctx):
    film, factor = C.COUPLED_BOARDS["single"]
    prob, meshes, layer_of, disc, *_ = board("single")
    case = C.scaled_case(prob, factor)
    _s, reps, couplings, _e = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model_of(film), cases=[case])
    _s, cold, _c, _e = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of,
                             model_of(film, temperature_coefficient=0.0), cases=[case])
    print("current-driven: hotspot", hottest(cold[0]), "->", hottest(reps[0]), "heat", cold[0].total_heat, "->", reps[0].total_heat)
    assert reps[0].total_heat > cold[0].total_heat and hottest(reps[0]) > hottest(cold[0])
    # the same board with the source's drop held instead of its current
    layer = prob.layers[0]
    c = [P.Connection(layer=layer, point=H.XY(1, 1)), P.Connection(layer=layer, point=H.XY(7, 7))]
    net = P.Network(connections=c, elements=[P.VoltageSource(p=c[0].node_id, n=c[1].node_id, voltage=0.45)])
    driven = P.Problem(layers=[layer], networks=[net])
    _s, warm, coupling = quiet(solver.solve_meshed_electrothermal, driven, meshes, layer_of, model_of(film))
    _s, cold, _c = quiet(solver.solve_meshed_electrothermal, driven, meshes, layer_of, model_of(film, temperature_coefficient=0.0))
    print("voltage-driven: hotspot", hottest(cold), "->", hottest(warm), "heat", cold.total_heat, "->", warm.total_heat,
          "rounds", coupling.rounds)
    assert coupling.converged and hottest(cold) > 35.0
    assert warm.total_heat < cold.total_heat and hottest(warm) < hottest(cold)


# ---- 9. load cases -----------------------------------------------------------------------------------------------------------

def test_two_load_cases_one_of_them_dead(ctx):
    film, factor = C.COUPLED_BOARDS["two_layer"]
    prob, meshes, layer_of, disc, *_ = board("two_layer")
    live = C.scaled_case(prob, factor)
    dead = {e: 0.0 for e in live}
    model = model_of(film, ambient=40.0)
    sols, reps, couplings, env = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model, cases=[live, dead])
    assert len(sols) == len(reps) == len(couplings) == 2
    assert couplings[0].converged and couplings[0].rounds > 1
    # the dead case: exactly ambient, one round, the scale of the copper at ambient
    assert couplings[1].rounds == 1 and couplings[1].converged and couplings[1].increments == [0.0]
    assert all((z == 40.0).all() for z in vertex_temperatures(reps[1]))
    assert reps[1].total_heat == 0.0 and reps[1].total_loss == 0.0
    s0 = 1 / (1 + 3.93e-3 * ((0.0 + 40.0) - 20.0))
    assert all((tf.values == s0).all() for forms in couplings[1].conductance_scale for tf in forms)
    # the live case is what it is alone: the second case starts from the copper at ambient again
    _s, alone, c_alone, _e = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, model, cases=[dead, live])
    assert c_alone[1].increments == couplings[0].increments
    assert all(np.array_equal(a, b) for a, b in zip(vertex_temperatures(alone[1]), vertex_temperatures(reps[0])))
    # the envelope is envelope_of on the per-case arrays
    per_case = [np.concatenate(vertex_temperatures(rep)) for rep in reps]
    best, which = solver.envelope_of(per_case)
    assert np.array_equal(np.concatenate([zf.values for forms in env.temperatures for zf in forms]), best)
    assert np.array_equal(np.concatenate([c for cs in env.cases for c in cs]), which)
    assert (which == 0).all()
    for layer_i, spot in enumerate(env.hotspots):
        assert spot[1] == 0 and spot[0] == reps[0].hotspots[layer_i][0] and spot[2:] == reps[0].hotspots[layer_i][1:]


# ---- 10. repeatability, warnings and refusals --------------------------------------------------------------------------------

def test_two_calls_give_the_same_bits(ctx):
    runs = [coupled_run("two_layer") for _ in range(2)]
    (_a, sol_a, rep_a, c_a, _e), (_b, sol_b, rep_b, c_b, _f) = runs
    assert c_a.increments == c_b.increments and c_a.rounds == c_b.rounds and scalars(rep_a) == scalars(rep_b)
    for x, y in zip(solution_arrays(sol_a) + report_arrays(rep_a), solution_arrays(sol_b) + report_arrays(rep_b)):
        assert np.array_equal(x, y)


def test_one_round_is_not_enough_on_a_coupled_board(ctx):
    film, factor = C.COUPLED_BOARDS["single"]
    prob, meshes, layer_of, *_ = board("single")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _s, _r, couplings, _e = solver.solve_meshed_electrothermal(prob, meshes, layer_of, model_of(film, max_rounds=1),
                                                                  cases=[C.scaled_case(prob, factor)])
    assert couplings[0].rounds == 1 and not couplings[0].converged
    assert any(issubclass(w.category, solver.SolverWarning) and "did not converge" in str(w.message) for w in caught)


class _World:
    world = 2


def test_refusals(ctx):
    prob, meshes, layer_of, *_ = board("single")
    with pytest.raises(ValueError):
        solver.solve_meshed_electrothermal(prob, meshes, layer_of, model_of(), partition=_World())
    with pytest.raises(ValueError):
        solver.solve_meshed_electrothermal(prob, meshes, layer_of, model_of(tolerance=0.0))
    with pytest.raises(ValueError):
        solver.solve_meshed_electrothermal(prob, meshes, layer_of, solver.ThermalModel(film=FILM))
    lib = _hip.load_library()
    with Device("two_layer", FILM) as dev, Device("single", FILM) as other:
        good = alphas(dev)
        with pytest.raises(ValueError):                    # a thermal handle of another system
            _hip.Coupled(dev.L.dev, other.thermal, good, 25.0, 20.0)
        with pytest.raises(ValueError):                    # one alpha per mesh
            _hip.Coupled(dev.L.dev, dev.thermal, good[:1], 25.0, 20.0)
        with pytest.raises(ValueError):
            _hip.Coupled(dev.L.dev, dev.thermal, [float("nan")] * len(good), 25.0, 20.0)
        with pytest.raises(ValueError, match="face 0"):    # the copper at ambient is already outside the model
            _hip.Coupled(dev.L.dev, dev.thermal, good, 25.0, 25.0 + 2 / min(good))
        # an uploaded matrix (the only kind whose columns may not ascend) carries no mesh and is not the handle's system
        A = sp.csr_matrix(dev.L.dev.to_scipy())
        upload = ctx.csr_from_scipy(A)
        try:
            with pytest.raises(ValueError):
                _hip.Coupled(upload, dev.thermal, good, 25.0, 20.0)
        finally:
            upload.close()
        coupled = _hip.Coupled(dev.L.dev, dev.thermal, good, 25.0, 20.0)
        try:
            null = _hip._P()
            d = _hip.C.c_double()
            assert lib.padne_coupled_revalue(ctx._h, null) == _hip.E_INVALID
            assert lib.padne_coupled_revalue(null, coupled._h) == _hip.E_INVALID
            assert lib.padne_coupled_update(ctx._h, coupled._h, 0, None, None) == _hip.E_INVALID
            assert lib.padne_coupled_create(ctx._h, dev.L.dev._h, null, len(good), None, 25.0, 20.0, None) == _hip.E_INVALID
            assert lib.padne_coupled_destroy(null) == _hip.OK
            with pytest.raises(ValueError):                # no thermal solve to take theta from
                coupled.update()
            with pytest.raises(ValueError):
                coupled.update(np.zeros(dev.n_pot + 1))
            with pytest.raises(ValueError):
                coupled.set_scale(np.ones(dev.n_tri - 1))
            with pytest.raises(ValueError):
                coupled.set_scale(np.zeros(dev.n_tri))
            with pytest.raises(ValueError):
                coupled.get_scale(dev.n_tri + 1)
            plan, _V = finished_block(other.board, other.L, other.cases)
            try:
                with pytest.raises(ValueError):            # a plan of another system
                    coupled.solve_kkt(plan)
                with pytest.raises(ValueError):
                    coupled.power_density(plan, dev.n_tri)
            finally:
                plan.close()
        finally:
            coupled.close()

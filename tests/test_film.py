"""Film curves on the device against the host restatement (tests/film_ref.py, itself checked by tests/test_film_host.py): the
terms and the linearised matrix bit for bit; constant curves against the float path; the uniform plate's closed form; the
fixed point and the round count against the restatement's Newton loop; film loss against heat put in; the electro-thermal
loop with curves; load cases on one electrical block solve; refusals through the C ABI.

Boards: three generated triangle strips of 255, 256 and 257 vertices in one handle (a ragged tile, a full one, one vertex
into a second tile); tests/test_thermal.py's synthetic boards and the goldens; film_ref.FILM_BOARDS for the loops (rises of
tens of kelvin, inside the curves' knots, converged on the host within 12 rounds: tests/test_film_host.py)."""
import math
import warnings

import numpy as np
import pytest

import coupled_ref as C
import film_ref as F
import thermal_ref as T
from padne_amd import _hip, solver
from test_device_memory import leaves
from test_film_host import DEVICE_TOLERANCE
from test_load_case_currents import finished_block
from test_stack import Stacked
from test_thermal import BAR, Device, board, delivered_power, quiet, sorted_csr, vertex_temperatures

pytestmark = pytest.mark.gpu

FILM = 1e-3
Curve = solver.FilmCurve


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


# ---- boards and tables ------------------------------------------------------------------------------------------------------

def strip(n, x0):
    """A triangle strip of n vertices (n - 2 faces) from x0 on, its upper row shifted so that no two faces are alike."""
    i = np.arange(n)
    xy = np.stack([x0 + 0.5 * (i // 2) + 0.2 * (i % 2), 0.7 * (i % 2) + 0.01 * np.sin(i)], axis=1)
    odd = i[:-2] % 2
    return xy, np.stack([i[:-2] + odd, i[1:-1] - odd, i[2:]], axis=1)        # every face turns the same way


class Strips:
    """Three strips of 255, 256 and 257 vertices assembled as one system with a thermal handle: no elements, no Problem."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.flat = [strip(255, 0.0), strip(256, 100.0), strip(257, 200.0)]
        self.xy, self.tri, self.face_mesh, self.voff, self.toff = T.flatten(self.flat)
        self.n_vert = self.n_pot = len(self.xy)
        self.kappa, self.film = [3e-3, 2e-3, 1e-3], [FILM, 2 * FILM, 3 * FILM]

    def __enter__(self):
        local = np.concatenate([tri for _xy, tri in self.flat])
        self.L = self.ctx.assemble_system(self.n_vert, self.xy, local, self.voff, self.toff, [1.0, 2.0, 3.0], [], [], [])
        self.thermal = _hip.Thermal(self.L, self.n_pot, self.kappa, self.film)
        return self

    def __exit__(self, *exc):
        self.thermal.close()
        self.L.close()

    def restated(self):
        return T.operator(self.flat, self.kappa, self.film, 0, [])


def tables_for(films, order=(1, 2, 64)):
    """A table per mesh whose first film is the mesh's own, of 1, 2 and 64 knots in turn (``order``)."""
    out = []
    for m, h0 in enumerate(films):
        n = order[m % len(order)]
        rise = 90.0 * (np.arange(n) / max(n - 1, 1)) ** 2
        out.append((rise, h0 * (1 + 0.02 * rise - 0.3 * np.sin(rise / 7.0) ** 2 * (rise / 90.0))))
    for rise, film in out:
        solver.check_film_curve(Curve(rise, film))
    return out


def probing_theta(tables, voff, seed):
    """Per mesh: every knot, one ulp either side of it, -0.0, values below 0 and above the last knot, then random rises from
    below 0 to beyond the last knot; a mesh of a few vertices gets the first of these."""
    rng = np.random.default_rng(seed)
    out = []
    for m, (rise, _film) in enumerate(tables):
        n = int(voff[m + 1] - voff[m])
        special = np.concatenate([[rise[-1], -0.0, np.nextafter(rise[-1], np.inf), -1.0], rise, np.nextafter(rise, -np.inf),
                                  np.nextafter(rise, np.inf), [-1e-300, 2 * rise[-1] + 1.0, 1e6, 0.0]])
        out.append(np.concatenate([special, rng.uniform(-5.0, 1.2 * rise[-1] + 5.0, n)])[:n])
    return np.concatenate(out)


def handle(ctx, name):
    if name == "strips":
        return Strips(ctx)
    if name == "two_layer_stacked":
        return Stacked("two_layer", FILM, pairs=[(0, 1, 1.5e-3)])
    return Device(name, FILM)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


# ---- 1. the terms -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["strips", "two_in_layer", "problem_many_meshes"])
def test_terms_are_the_restatement_bit_for_bit(ctx, name):
    """g, c, hM and the count above the last knot for a theta that sits on, beside and outside the knots; tables of 1, 2 and
    64 knots on different meshes; a pure function: the second call gives the same bits, the matrix is untouched."""
    with handle(ctx, name) as dev:
        order = (64, 2, 1) if name == "two_in_layer" else (1, 2, 64)
        tables = tables_for(dev.film, order)
        dev.thermal.set_film_curves(tables)
        theta = probing_theta(tables, dev.voff, seed=3)
        before = dev.thermal.matrix().to_scipy().data.copy()
        got = dev.thermal.film_terms(theta, dev.n_vert)
        again = dev.thermal.film_terms(theta, dev.n_vert)
        zero = dev.thermal.film_terms(np.zeros(dev.n_vert), dev.n_vert)
        after = dev.thermal.matrix().to_scipy().data
        M = dev.thermal.lumped(dev.n_vert)
    want = F.terms(tables, dev.voff, M, theta)
    assert sorted({len(r) for r, _ in tables}) == sorted(set(order[:len(tables)]))
    for k, what in enumerate(("g", "c", "hM")):
        assert same_bits(got[k], want[k]), what
        assert same_bits(again[k], got[k])
    assert got[3] == want[3] == again[3] and want[3] > 0
    assert np.array_equal(before, after)
    hM0 = np.repeat(np.asarray(dev.film), np.diff(dev.voff)) * M
    assert same_bits(zero[0] * M, hM0) and (zero[1] == 0.0).all() and same_bits(zero[2], hM0) and zero[3] == 0


# ---- 2. the linearised matrix ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["strips", "two_in_layer", "two_layer_stacked"])
def test_linearise_writes_only_the_diagonals(ctx, name):
    """About the theta of a solve: the matrix is the restatement's bit for bit (definition 4 on the device's own matrix of
    the create call), every off-diagonal and every internal-node row keeps its bits; about zero the create call's bits; with
    the curves removed the matrix and, through the report's film loss, hM are the create call's again."""
    with handle(ctx, name) as dev:
        A0 = sorted_csr(dev.thermal.matrix().to_scipy())
        M = dev.thermal.lumped(dev.n_vert)
        Pf = (np.random.default_rng(7).uniform(0.0, 0.06, len(dev.tri)) * T.face_area(dev.xy, dev.tri))[None, :]
        theta_plain, _ = dev.thermal.solve(Pf)
        loss_plain = dev.thermal.report(1, len(dev.tri), dev.n_vert, fields=False, envelope=False)[4]
        tables = tables_for(dev.film, (64, 2, 1))
        dev.thermal.set_film_curves(tables)
        A_set = sorted_csr(dev.thermal.matrix().to_scipy())
        dev.thermal.film_linearise(False)
        A_zero = sorted_csr(dev.thermal.matrix().to_scipy())
        theta, _ = dev.thermal.solve(Pf)
        dev.thermal.film_linearise(True)
        A_lin = sorted_csr(dev.thermal.matrix().to_scipy())
        dev.thermal.set_film_curves([])
        A_back = sorted_csr(dev.thermal.matrix().to_scipy())
        theta_back, _ = dev.thermal.solve(Pf)
        loss_back = dev.thermal.report(1, len(dev.tri), dev.n_vert, fields=False, envelope=False)[4]
        with pytest.raises(ValueError, match="no film curves"):
            dev.thermal.film_linearise(False)
    hM0 = np.repeat(np.asarray(dev.film), np.diff(dev.voff)) * M
    want = F.linearised(A0, M, hM0, tables, dev.voff, theta[0, :dev.n_vert])
    assert 10.0 < theta[0].max() < 90.0
    assert same_bits(A_set.data, A0.data) and same_bits(A_zero.data, A0.data) and same_bits(theta, theta_plain)
    assert np.array_equal(A_lin.indices, A0.indices) and same_bits(A_lin.data, want.data)
    rows = np.repeat(np.arange(A0.shape[0]), np.diff(A0.indptr))
    changed = A_lin.data.view(np.int64) != A0.data.view(np.int64)
    assert changed.sum() > 0.4 * dev.n_vert and (rows[changed] == A0.indices[changed]).all() and (rows[changed] < dev.n_vert).all()
    assert same_bits(A_back.data, A0.data) and same_bits(theta_back, theta_plain) and same_bits(loss_back, loss_plain)


# ---- 3. constant curves -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["single", "two_layer", "problem_many_meshes"])
def test_constant_curves_are_the_float_path(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    films = {layer.name: FILM * (1 + 0.5 * i) for i, layer in enumerate(prob.layers)}
    curves = {key: Curve([0.0, 50.0, 120.0], [h, h, h]) if i % 2 else Curve.constant(h) for i, (key, h) in enumerate(films.items())}
    kw = dict(disconnected_meshes_by_layer=disc)
    plain = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(film=films), **kw)
    const = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(film=curves), **kw)
    assert const[1].film is None
    a, b = leaves(plain), leaves(const)
    assert [x[:3] for x in a] == [x[:3] for x in b]
    assert all(x[3] == y[3] for x, y in zip(a, b))


# ---- 4. the uniform plate ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(F.plate_curves()))
def test_the_uniform_plate_through_the_device_solve(ctx, name):
    """P_f = p A_f uploaded to padne_thermal_solve, then the rounds by hand: theta is the root of h(theta) theta = p at every
    vertex within 1e-8 relative."""
    curve, p = F.plate_curves()[name]
    table = F.table_of(solver.check_film_curve(curve))
    root = F.plate_root(*table, p)
    prob = board("single")[0]
    no_links = {e: 0.0 for n in prob.networks for e in n.elements if solver.element_kind(e) == "Resistor"}
    increments = []
    with Device("single", float(table[1][0]), link_conductance=no_links) as dev:
        dev.thermal.set_film_curves([table])
        Pf = (p * T.face_area(dev.xy, dev.tri))[None, :]
        for k in range(12):
            dev.thermal.film_linearise(k > 0)
            theta, _ = dev.thermal.solve(Pf) if k == 0 else dev.thermal.resolve()
            increments.append(dev.thermal.film_increment()[0])
            if increments[-1] <= 1e-10 * root:
                break
        loss = dev.thermal.report(1, dev.n_tri, dev.n_vert, fields=False, envelope=False)[4]
    err = np.abs(theta[0] - root).max() / root
    print(name, "root", root, "increments", increments, "rel.err", err)
    assert increments[-1] <= 1e-10 * root
    assert err <= 1e-8
    assert abs(loss.sum() - Pf.sum()) <= 1e-9 * Pf.sum()


# ---- 5. the fixed point -----------------------------------------------------------------------------------------------------

def solve_board(name, cases=None, timings=None, **model_kw):
    spec = F.host_spec(name, **model_kw)
    disc = board(F.FILM_BOARDS[name][0])[3]
    out = quiet(solver.solve_meshed_thermal, spec.prob, spec.meshes, spec.layer_of, spec.model,
                cases=[spec.case] if cases is None else cases, disconnected_meshes_by_layer=disc, timings=timings)
    return spec, out


def distance_bound(increments, rise):
    """1e-8 * max theta + d_K rho / (1 - rho), rho = d_K / d_{K-1} of the device's own increments."""
    d, rho = increments[-1], increments[-1] / increments[-2]
    assert rho < 0.5
    return BAR * rise + d * rho / (1 - rho)


@pytest.mark.parametrize("name", sorted(F.FILM_BOARDS))
def test_the_fixed_point_is_the_restatements(ctx, name):
    """theta against the restatement's Newton loop iterated to 1e-11 K; the rounds are those of the restatement stopped at the
    same tolerance; the report's loss is sum M_v h(theta_v) theta_v of the device's own theta."""
    spec, (_sols, reps, env) = solve_board(name, film_tolerance=DEVICE_TOLERANCE)
    rep = reps[0]
    fine = F.spec_newton(spec, 1e-11)
    same = F.spec_newton(spec, DEVICE_TOLERANCE)
    theta = np.concatenate(vertex_temperatures(rep)) - spec.model.ambient
    n_vert, film = spec.B.n_vert, rep.film
    err, rise = np.abs(theta - fine["theta"][:n_vert]).max(), fine["theta"][:n_vert].max()
    print(name, "rounds", film["rounds"], "increments", film["increments"], "host", same["increments"], "err", err,
          "bound", distance_bound(film["increments"], rise))
    assert film["converged"] and film["beyond"] == 0 and film["rounds"] == len(same["increments"]) == len(film["vertices"])
    assert err <= distance_bound(film["increments"], rise)
    for d, want in zip(film["increments"], same["increments"]):
        assert abs(d - want) <= BAR * rise
    _g, _c, hM, _ = F.terms(spec.tables, spec.B.voff, spec.B.M, theta)
    assert abs(rep.total_loss - math.fsum((hM * theta).tolist())) <= 1e-12 * rep.total_loss
    assert np.array_equal(np.concatenate([zf.values for forms in env.temperatures for zf in forms]), theta + spec.model.ambient)


# ---- 6. the balance -----------------------------------------------------------------------------------------------------------

def defect(spec, report):
    return F.defect_bound(spec.tables, spec.B.voff, spec.B.M, report.film["increments"][-1])


def delivered_by_case(spec, name, cases) -> list:
    """What the sources deliver in every case: the elements' flows of the same block solve (solve_meshed_load_case_currents)."""
    disc = board(F.FILM_BOARDS[name][0])[3]
    _s, currents, _e = quiet(solver.solve_meshed_load_case_currents, spec.prob, spec.meshes, spec.layer_of, cases,
                             per_case_fields=False, disconnected_meshes_by_layer=disc)
    return [delivered_power(report) for report in currents]


@pytest.mark.parametrize("name", ["two_layer", "single_source"])
def test_the_film_loss_is_the_heat_put_in(ctx, name):
    """Three load cases, the second dead: |total_loss - delivered| <= 1e-9 delivered + the last round's linearisation defect;
    the dead case comes back as exact zeros in one round."""
    prob = board(F.FILM_BOARDS[name][0])[0]
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]
    dead = {e: 0.0 for e in sources}
    live = C.scaled_case(prob, F.FILM_BOARDS[name][1])
    half = {e: 0.5 * v for e, v in live.items()}
    kw = dict(film_tolerance=1e-9)
    if name == "single_source":                             # the component is off in the dead case
        kw["heat_sources"] = [solver.HeatSource.rectangle("F.Cu", 2.0, 2.0, 5.0, 5.0, [0.4, 0.0, 0.1])]
    spec, (_sols, reps, _env) = solve_board(name, cases=[live, dead, half], **kw)
    for j, (rep, joule) in enumerate(zip(reps, delivered_by_case(spec, name, [live, dead, half]))):
        delivered = joule + rep.source_heat
        print(name, "case", j, "delivered", delivered, "loss", rep.total_loss, "rounds", rep.film["rounds"], "last", rep.film["increments"][-1],
              "defect", defect(spec, rep))
        assert abs(rep.total_loss - delivered) <= 1e-9 * delivered + defect(spec, rep)
        assert abs(rep.total_heat - delivered) <= 1e-9 * delivered
    assert [rep.source_heat for rep in reps] == ([0.4, 0.0, 0.1] if name == "single_source" else [0.0] * 3)
    zero = reps[1]
    assert zero.film["rounds"] == 1 and zero.film["increments"] == [0.0] and zero.film["converged"]
    assert all((t == spec.model.ambient).all() for t in vertex_temperatures(zero)) and zero.total_loss == 0.0
    assert reps[0].film["rounds"] > 2 and reps[0].total_loss > 0


# ---- 7. electro-thermal -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_layer", "single_source"])
def test_alpha_zero_with_curves_is_the_thermal_solve_bit_for_bit(ctx, name):
    spec, (sols, reps, _env) = solve_board(name, film_tolerance=DEVICE_TOLERANCE)
    disc = board(F.FILM_BOARDS[name][0])[3]
    electro = solver.ElectroThermalModel(thermal=spec.model, temperature_coefficient=0.0, tolerance=DEVICE_TOLERANCE)
    _s, ereps, couplings, _e = quiet(solver.solve_meshed_electrothermal, spec.prob, spec.meshes, spec.layer_of, electro,
                                     cases=[spec.case], disconnected_meshes_by_layer=disc)
    a, b = leaves(reps[0]), leaves(ereps[0])
    assert [x[:3] for x in a] == [x[:3] for x in b]
    for x, y in zip(a, b):
        assert x[3] == y[3], x[0]
    assert couplings[0].rounds == reps[0].film["rounds"] > 2 and couplings[0].converged


@pytest.mark.parametrize("name", ["two_layer", "single_source"])
def test_the_coupled_fixed_point_balance_and_direction(ctx, name):
    """alpha of copper with curves: the fixed point of the host loop within the bound of test 5 (rho of the device's own
    increments); loss equals heat put in; and the rising film lowers the hotspot against the constant h(0) run."""
    alpha, tol = solver.COPPER_TEMPERATURE_COEFFICIENT, 1e-7
    spec = F.host_spec(name, alpha=alpha, film_tolerance=tol)
    disc = board(F.FILM_BOARDS[name][0])[3]
    electro = solver.ElectroThermalModel(thermal=spec.model, temperature_coefficient=alpha, tolerance=tol, max_rounds=40)
    run = lambda model: quiet(solver.solve_meshed_electrothermal, spec.prob, spec.meshes, spec.layer_of, model, cases=[spec.case],      # noqa: E731
                              disconnected_meshes_by_layer=disc)
    _s, reps, couplings, _e = run(electro)
    rep, coupling = reps[0], couplings[0]
    fine = F.spec_newton(spec, 1e-11, 60, coupled=True)
    theta = np.concatenate(vertex_temperatures(rep)) - spec.model.ambient
    n_vert = spec.B.n_vert
    err, rise = np.abs(theta - fine["theta"][:n_vert]).max(), fine["theta"][:n_vert].max()
    print(name, "rounds", coupling.rounds, "increments", coupling.increments, "err", err, "bound", distance_bound(coupling.increments, rise))
    assert coupling.converged and fine["converged"] and rep.film["converged"] and rep.film["rounds"] == coupling.rounds
    assert err <= distance_bound(coupling.increments, rise)
    delivered = delivered_power(coupling) + rep.source_heat      # (the elements' flows of the last electrical solve)
    print(name, "delivered", delivered, "loss", rep.total_loss, "defect", defect(spec, rep))
    assert delivered > 0 and abs(rep.total_loss - delivered) <= 1e-9 * delivered + defect(spec, rep)
    # the same board with every film held at h(0)
    flat = {spec.prob.layers[l].name: h for l, h in enumerate(spec.checked.film)}
    kw = {k: getattr(spec.model, k) for k in ("interlayer", "heat_sources")}
    constant = solver.ElectroThermalModel(thermal=solver.ThermalModel(film=flat, **kw), temperature_coefficient=alpha, tolerance=tol,
                                          max_rounds=40)
    _s, creps, _c, _e = run(constant)
    hot = lambda r: max(h[0] for h in r.hotspots if h is not None)      # noqa: E731
    print(name, "hotspot with curves", hot(rep), "with h(0)", hot(creps[0]))
    assert hot(rep) < hot(creps[0]) and creps[0].film is None


# ---- 8. load cases ------------------------------------------------------------------------------------------------------------

def test_load_cases_keep_one_block_solve_and_two_calls_give_the_same_bits(ctx, monkeypatch):
    """Three cases: one electrical block solve (the laps of the call hold one stage1 / stage2 and no round holds any), every
    case's Newton rounds in the rounds' laps, and a second call gives the same bits."""
    calls = []
    real = solver._solve_block_on_device
    monkeypatch.setattr(solver, "_solve_block_on_device", lambda *a, **k: calls.append(a[4]) or real(*a, **k))
    prob = board("two_layer")[0]
    live = C.scaled_case(prob, 0.2)
    cases = [live, {e: 0.6 * v for e, v in live.items()}, {e: 1.3 * v for e, v in live.items()}]
    timings = {}
    _spec, first = solve_board("two_layer", cases=cases, timings=timings, film_tolerance=DEVICE_TOLERANCE)
    _spec, second = solve_board("two_layer", cases=cases, film_tolerance=DEVICE_TOLERANCE)
    assert calls == [3, 3]
    assert "stage1" in timings and "stage2" in timings and "thermal_solve" in timings
    rounds = timings["rounds"]
    assert sorted({r["case"] for r in rounds}) == [0, 1, 2] and not any("stage1" in r or "revalue" in r for r in rounds)
    assert all({"linearise", "thermal_solve", "increment", "hierarchy"} <= set(r) for r in rounds)
    assert [sum(r["case"] == j for r in rounds) for j in range(3)] == [rep.film["rounds"] for rep in first[1]]
    a, b = leaves(first), leaves(second)
    assert [x[:3] for x in a] == [x[:3] for x in b] and all(x[3] == y[3] for x, y in zip(a, b))
    hot = [rep.hotspots[0][0] for rep in first[1]]
    assert hot[1] < hot[0] < hot[2]
    env = np.concatenate([zf.values for forms in first[2].temperatures for zf in forms])
    assert np.array_equal(env, np.max([np.concatenate(vertex_temperatures(rep)) for rep in first[1]], axis=0))


def test_the_round_limit_warns_and_names_the_layer(ctx):
    spec = F.host_spec("single_source", film_tolerance=1e-13, film_max_rounds=2)
    disc = board("single")[3]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _s, rep = solver.solve_meshed_thermal(spec.prob, spec.meshes, spec.layer_of, spec.model, cases=None,
                                              disconnected_meshes_by_layer=disc)
    text = [str(w.message) for w in caught if issubclass(w.category, solver.SolverWarning) and "film loop" in str(w.message)]
    assert len(text) == 1 and "2 round(s)" in text[0] and "'F.Cu'" in text[0] and f"{rep.film['increments'][-1]:.3e}" in text[0]
    assert rep.film["rounds"] == 2 and not rep.film["converged"]


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_through_the_c_abi(ctx):
    """PADNE_E_INVALID (a ValueError here) with nothing changed: the matrix, and a solve afterwards, keep their bits."""
    with Device("two_layer", FILM, cases=({}, {})) as dev:
        tables = tables_for(dev.film, (64, 2))
        Pf = (np.random.default_rng(1).uniform(0.0, 0.05, dev.n_tri) * T.face_area(dev.xy, dev.tri))[None, :]
        A0 = dev.thermal.matrix().to_scipy().data.copy()
        bad = [
            ([tables[0]], "n_mesh"),                                                                         # one table for two meshes
            ([(tables[0][0], tables[0][1] * np.nextafter(1.0, 2.0)), tables[1]], "created with"),            # not the created film
            ([tables[0], (np.array([0.0, 10.0, 20.0]), np.array([FILM, FILM, 0.2 * FILM]))], "segment 1"),   # q not monotone
            ([tables[0], (np.array([0.0, 10.0, 10.0]), np.array([FILM, FILM, FILM]))], "ascend"),
            ([tables[0], (np.array([0.0, 1.0]), np.array([FILM, np.inf]))], "finite"),
            ([tables[0], (np.arange(65.0), np.full(65, FILM))], "64"),
        ]
        for curves, match in bad:
            with pytest.raises(ValueError, match=match):
                dev.thermal.set_film_curves(curves)
            with pytest.raises(ValueError, match="no film curves"):     # nothing was installed
                dev.thermal.film_linearise(False)
        theta_plain, _ = dev.thermal.solve(Pf)
        dev.thermal.set_film_curves(tables)
        dev.thermal.film_linearise(False)
        theta, _ = dev.thermal.solve(Pf)
        dev.thermal.film_linearise(True)
        A_lin = dev.thermal.matrix().to_scipy().data.copy()
        for curves, match in bad[1:3]:                        # a refused replacement leaves the installed curves alone
            with pytest.raises(ValueError, match=match):
                dev.thermal.set_film_curves(curves)
        with pytest.raises(ValueError, match="one column at a time"):
            dev.thermal.solve(np.concatenate([Pf, Pf]))
        plan, _V = finished_block(dev.board, dev.L, dev.cases)
        try:
            with pytest.raises(ValueError, match="one column at a time"):
                dev.thermal.solve_kkt(plan, 2)
            with pytest.raises(ValueError, match="column must be one"):
                dev.thermal.solve_kkt_column(plan, 2, 2)
            with pytest.raises(ValueError, match="film curves takes no transient"):
                _hip.Transient(dev.thermal, [3e-3, 3e-3])
            with pytest.raises(ValueError, match="film curves takes no sensitivity"):
                _hip.ThermalSensitivities(dev.thermal, plan, 2, dev.kappa)
            assert np.array_equal(dev.thermal.matrix().to_scipy().data, A_lin)
            again, _ = dev.thermal.resolve()                # the held load and linearisation are still there
            by_column, _ = dev.thermal.solve_kkt_column(plan, 2, 1)
            dev.thermal.set_film_curves([])
            with pytest.raises(ValueError, match="no film curves"):
                dev.thermal.resolve()
            block, _ = dev.thermal.solve_kkt(plan, 2)
            transient = _hip.Transient(dev.thermal, [3e-3, 3e-3])       # without curves the handles are made again
            transient.close()
        finally:
            plan.close()
        back = dev.thermal.matrix().to_scipy().data
    assert same_bits(theta, theta_plain) and same_bits(back, A0) and not same_bits(A_lin, A0)
    assert np.abs(again - theta).max() > 1e-3 and np.isfinite(again).all()
    assert by_column.shape == (1, dev.n_pot) and block.shape == (2, dev.n_pot) and np.isfinite(by_column).all()

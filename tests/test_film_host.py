"""Film curves on the host ("Film curves"): what check_film_curve refuses, the helpers against their formulas,
how check_thermal_model resolves floats, curves and mixed mappings, the calls that refuse a curve before anything reaches a
device, the restatement's Newton loop (tests/film_ref.py) against the uniform plate's closed form, and the condition under
which the device tests of tests/test_film.py may trust their round limit: on every board they use, the host loop from zero
is converged to 1e-10 of the rise within 12 rounds, with no increment near the tolerance the device loop stops at; and
film_ref.increment, the increment in the kernels' order, against the plain rule (the maximum, the lowest vertex)."""
import math

import numpy as np
import pytest

import film_ref as F
import helpers as H
import thermal_ref as T
from padne_amd import problem as P, solver, synthetic

Curve = solver.FilmCurve
DEVICE_TOLERANCE = 1e-4              # the film_tolerance of the device tests that count rounds (tests/test_film.py)


# ---- check_film_curve -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curve, match", [
    (Curve([], []), "knots"),
    (Curve(np.linspace(0.0, 1.0, 65) ** 2 * 64, np.ones(65)), "knots"),
    (Curve([0.0, 1.0], [1.0]), "one film per knot"),
    (Curve([1.0, 2.0], [1.0, 1.0]), "rise of 0"),
    (Curve([0.0, 2.0, 2.0], [1.0, 1.0, 1.0]), "ascend"),
    (Curve([0.0, 3.0, 2.0], [1.0, 1.0, 1.0]), "ascend"),
    (Curve([0.0, math.inf], [1.0, 1.0]), "finite"),
    (Curve([0.0, 1.0], [1.0, math.nan]), "finite"),
    (Curve([0.0, 1.0], [1.0, 0.0]), "positive"),
    (Curve([0.0], [-1.0]), "positive"),
    (Curve([0.0, 10.0, 20.0], [1.0, 1.0, 0.2]), "segment 1"),
    ([0.0, 1.0], "FilmCurve"),
], ids=["none", "65", "lengths", "start", "equal", "descending", "inf", "nan", "zero", "negative", "falls", "type"])
def test_check_film_curve_refuses(curve, match):
    with pytest.raises(ValueError, match=match):
        solver.check_film_curve(curve)


def test_check_film_curve_accepts_and_copies():
    """The limits themselves pass: 1 and 64 knots, a fall whose q' stays positive at both ends of its segment."""
    assert solver.check_film_curve(Curve.constant(2.0)).film.tolist() == [2.0]
    many = solver.check_film_curve(Curve(np.arange(64.0), np.linspace(1.0, 2.0, 64)))
    assert len(many.rise) == 64
    with pytest.raises(ValueError, match="segment 1"):       # s = -0.04: q'(20) = 1 - 0.04 * 30 < 0
        solver.check_film_curve(Curve([0.0, 10.0, 20.0], [1.0, 1.0, 0.6]))
    gentle = Curve([0.0, 10.0, 20.0], [1.0, 1.0, 0.8])      # s = -0.02: q'(10) = 0.8, q'(20) = 1 - 0.02 * 30 = 0.4
    got = solver.check_film_curve(gentle)
    got.film[0] = 5.0
    assert gentle.film[0] == 1.0


# ---- the helpers ------------------------------------------------------------------------------------------------------------

def test_helpers_agree_with_their_formulas_at_the_knots():
    knots = 200.0 * (np.arange(33) / 32) ** 2
    nc = Curve.natural_convection(3e-4, upto=200.0)
    assert np.array_equal(nc.rise, knots)
    assert np.array_equal(nc.film[1:], 3e-4 * knots[1:] ** 0.25) and nc.film[0] == nc.film[1]     # h(0) of the law is no film
    third = Curve.natural_convection(3e-4, exponent=1 / 3, upto=50.0, knots=9)
    assert np.array_equal(third.film[1:], 3e-4 * third.rise[1:] ** (1 / 3)) and len(third.rise) == 9
    es, ta = 5.67e-14 * 0.8, 300.0
    rad = Curve.radiation(es, ta, upto=200.0)
    assert np.array_equal(rad.film, es * ((ta + knots) ** 2 + ta ** 2) * ((ta + knots) + ta))
    assert rad.film[0] == pytest.approx(4 * es * ta ** 3, rel=1e-15)
    tab = Curve.tabulate(lambda t: 1.0 + t, 8.0, knots=5)
    assert tab.rise.tolist() == [0.0, 0.5, 2.0, 4.5, 8.0] and tab.film.tolist() == [1.0, 1.5, 3.0, 5.5, 9.0]
    both = nc + rad
    assert np.array_equal(both.film, nc.film + rad.film) and np.array_equal(both.rise, knots)
    assert np.array_equal((rad + 1e-5).film, rad.film + 1e-5) and np.array_equal((1e-5 + rad).film, rad.film + 1e-5)
    with pytest.raises(ValueError, match="rises must be equal"):
        nc + third
    assert Curve.constant(3.0).is_constant() and not rad.is_constant()
    for curve in (nc, third, rad, tab, both):
        solver.check_film_curve(curve)
    assert rad(0.0) == rad.film[0] and rad(-5.0) == rad.film[0] and rad(1e4) == rad.film[-1]


# ---- check_thermal_model ----------------------------------------------------------------------------------------------------

def small_problem():
    top = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=2.0)
    bottom = P.Layer(shape=H.Geoms(1), name="B.Cu", conductance=1.0)
    c = [P.Connection(layer=top, point=H.XY(1, 1)), P.Connection(layer=bottom, point=H.XY(7, 7))]
    net = P.Network(connections=c, elements=[P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0)])
    return P.Problem(layers=[top, bottom], networks=[net]), top


def test_check_thermal_model_resolves_floats_curves_and_mixed_mappings():
    prob, top = small_problem()
    curve = F.board_curve()
    plain = solver.check_thermal_model(prob, solver.ThermalModel(film=2e-3))
    assert plain.film == [2e-3, 2e-3] and plain.film_curves is None and not plain.curved()
    assert plain.film_tolerance == solver.ElectroThermalModel.tolerance and plain.film_max_rounds == solver.ElectroThermalModel.max_rounds
    one = solver.check_thermal_model(prob, solver.ThermalModel(film=curve))
    assert one.film == [float(curve.film[0])] * 2 and one.curved()
    assert all(np.array_equal(c.film, curve.film) and np.array_equal(c.rise, curve.rise) for c in one.film_curves)
    mixed = solver.check_thermal_model(prob, solver.ThermalModel(film={top: curve, "B.Cu": 3e-3}, film_tolerance=1e-4,
                                                                 film_max_rounds=7))
    assert mixed.film == [float(curve.film[0]), 3e-3] and mixed.film_curves[1] is None and mixed.curved()
    assert mixed.film_tolerance == 1e-4 and mixed.film_max_rounds == 7
    flat = solver.check_thermal_model(prob, solver.ThermalModel(film={top: Curve.constant(4e-3), "B.Cu": 3e-3}))
    assert flat.film == [4e-3, 3e-3] and flat.film_curves[0] is not None and not flat.curved()
    assert F.tables_of(mixed, [0, 1, 0])[1][1].tolist() == [3e-3]


@pytest.mark.parametrize("kw, match", [
    (dict(film=Curve([0.0, 1.0], [1.0, 0.1])), "falls too fast on segment 0"),
    (dict(film={"F.Cu": Curve([1.0], [1.0]), "B.Cu": 1.0}), "F.Cu"),
    (dict(film={"F.Cu": F.board_curve()}), "no film coefficient"),
    (dict(film=1e-3, film_tolerance=0.0), "film_tolerance"),
    (dict(film=1e-3, film_tolerance=math.nan), "film_tolerance"),
    (dict(film=1e-3, film_max_rounds=0), "film_max_rounds"),
    (dict(film=1e-3, film_max_rounds=2.5), "film_max_rounds"),
])
def test_a_bad_film_is_refused(kw, match):
    prob, _ = small_problem()
    with pytest.raises(ValueError, match=match):
        solver.check_thermal_model(prob, solver.ThermalModel(**kw))


def test_the_modes_that_do_not_iterate_refuse_a_curve_before_the_device(monkeypatch):
    """Transient, adaptive transient, periodic, electro-thermal transient and the sensitivities: ValueError from their
    checkers that names the limit, with no context made; constant curves pass those checkers."""
    prob, top = small_problem()
    monkeypatch.setattr(solver, "get_context", lambda *a, **k: pytest.fail("a device context was asked for"))
    curved = solver.ThermalModel(film=F.board_curve())
    constant = solver.ThermalModel(film={top: Curve.constant(1e-3), "B.Cu": 1e-3})
    transient = lambda thermal: solver.TransientModel(thermal=thermal, areal_capacity=3e-3)      # noqa: E731
    with pytest.raises(ValueError, match="does not honour a film curve"):
        solver.check_transient_model(prob, transient(curved))
    solver.check_transient_model(prob, transient(constant))
    et = solver.ElectroThermalTransientModel(electrothermal=solver.ElectroThermalModel(thermal=curved), areal_capacity=3e-3)
    with pytest.raises(ValueError, match="does not honour a film curve"):
        solver.check_electrothermal_transient_model(prob, et)
    objectives = [solver.TemperatureObjective.hotspot("F.Cu")]
    monkeypatch.setattr(solver, "mesh_problem", lambda *a, **k: pytest.fail("the board was meshed"))
    schedule, spans = [solver.Segment(1.0, 10, 0)], [solver.Span(1.0, 0)]
    for call in (lambda m: solver.solve_thermal_transient(prob, transient(m), schedule, cases=[{}]),
                 lambda m: solver.solve_thermal_transient_adaptive(prob, transient(m), spans, tolerance=0.1, cases=[{}]),
                 lambda m: solver.solve_thermal_periodic(prob, transient(m), schedule, tolerance=0.1, cases=[{}]),
                 lambda m: solver.solve_thermal_sensitivities(prob, m, objectives),
                 lambda m: solver.solve_meshed_thermal_sensitivities(prob, [], [], m, objectives)):
        with pytest.raises(ValueError, match="does not honour a film curve"):
            call(curved)


# ---- the restatement --------------------------------------------------------------------------------------------------------

def plate():
    xy, tri = synthetic.jittered_grid(9, 9, h=1.0, seed=3, jitter=0.2)
    return np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int64).reshape(-1, 3)


def test_terms_at_and_around_the_knots():
    """On a knot the segment that starts there; one ulp below it the one before; below 0, -0.0 and above the last knot the
    clamped ranges: slope 0, c = 0, the first or the last film."""
    rise, film = np.array([0.0, 16.0, 64.0]), np.array([1e-3, 2e-3, 2.5e-3])
    s = F.slopes(rise, film)
    theta = np.array([0.0, -0.0, -3.0, np.nextafter(16.0, 0.0), 16.0, np.nextafter(16.0, 99.0), 64.0, np.nextafter(64.0, 99.0), 1e3])
    M = np.linspace(0.5, 1.5, len(theta))
    g, c, hM, beyond = F.terms([(rise, film)], [0, len(theta)], M, theta)
    assert beyond == 2
    assert g[0] == film[0] and c[0] == 0.0 and hM[0] == film[0] * M[0] and g[1] == film[0] and c[1] == 0.0
    assert g[2] == film[0] and c[2] == 0.0 and hM[2] == film[0] * M[2]
    assert g[3] == (film[0] + s[0] * theta[3]) + s[0] * theta[3] and g[4] == (film[1] + s[1] * 0.0) + s[1] * 16.0
    assert hM[4] == film[1] * M[4] and c[4] == ((s[1] * 16.0) * 16.0) * M[4]
    assert g[6] == film[2] and c[6] == 0.0 and g[7] == film[2] and g[8] == film[2] and hM[8] == film[2] * M[8]


@pytest.mark.parametrize("name", sorted(F.plate_curves()))
def test_host_newton_reproduces_the_uniform_plate(name):
    """b_v = sum_f (p A_f) / 3 on a jittered plate: theta is the constant root of h(theta) theta = p, to 1e-12 relative."""
    curve, p = F.plate_curves()[name]
    curve = solver.check_film_curve(curve)
    xy, tri = plate()
    table = F.table_of(curve)
    A0, M, hM0 = T.operator([(xy, tri)], [0.05], [float(curve.film[0])], 0, [])
    b = T.load(len(xy), tri, p * T.face_area(xy, tri))
    got = F.newton(A0, M, hM0, [table], [0, len(xy)], b, 1e-11 * 50)
    root = F.plate_root(*table, p)
    print(name, "root", root, "rounds", len(got["increments"]), got["increments"])
    assert got["converged"] and len(got["increments"]) <= 12 and 10.0 < root < 100.0
    assert np.abs(got["theta"] - root).max() <= 1e-12 * root
    assert abs(float(curve(root)) * root - p) <= 4e-16 * p * 4
    if name == "kink":
        assert root == 16.0
    loss = math.fsum((got["hM"] * got["theta"]).tolist())
    assert abs(loss - math.fsum(b.tolist())) <= 1e-12 * loss


@pytest.mark.parametrize("coupled", [False, True], ids=["thermal", "electrothermal"])
@pytest.mark.parametrize("name", sorted(F.FILM_BOARDS))
def test_the_boards_of_the_device_tests_converge_within_twelve_rounds(name, coupled):
    """Host Newton from zero reaches an increment below 1e-10 * max theta within 12 rounds, the rise is tens of kelvin and
    inside the curve's knots, and on the film alone (Newton: the increments square) none lies within a factor 20 of the
    tolerance at which the device tests that count rounds stop, so their count cannot hinge on rounding.  With the
    resistivity coupled in the loop is Picard's and passes every decade: there the device tests bound the distance only."""
    spec = F.host_spec(name, alpha=solver.COPPER_TEMPERATURE_COEFFICIENT if coupled else 0.0)
    first = F.spec_newton(spec, 1e300, 1, coupled=coupled)["theta"]
    got = F.spec_newton(spec, 1e-10 * first[:spec.B.n_vert].max() * 0.3, 12, coupled=coupled)
    rise = got["theta"][:spec.B.n_vert].max()
    print(name, "coupled" if coupled else "thermal", "rise", rise, "linear rise", first[:spec.B.n_vert].max(), "increments", got["increments"])
    assert got["converged"] and got["increments"][-1] < 1e-10 * rise
    assert 10.0 < rise < 100.0 and got["beyond"] == 0
    assert coupled or rise < first[:spec.B.n_vert].max() - 0.1      # the rising film cools the hotspot by more than any tolerance here
    assert coupled or all(not DEVICE_TOLERANCE / 20 <= d <= DEVICE_TOLERANCE * 20 for d in got["increments"])
    loss = math.fsum((got["hM"] * got["theta"][:spec.B.n_vert]).tolist())
    delivered = spec.B.delivered(got["flows"]) + sum(s.power for s in spec.checked.sources)
    assert abs(loss - delivered) <= 1e-9 * delivered


# ---- the increment in the kernels' order --------------------------------------------------------------------------------------

WIDE_VOFF = np.cumsum([0, 66_306, 4, 8_464, 16_770])        # tests/test_many_tiles.py's board: 260 + 1 + 34 + 66 = 361 tiles
WIDE_TILE0 = np.cumsum([0, 260, 1, 34, 66])                  # the first global tile of every mesh


def in_tile(tile: int, lane: int) -> int:
    """The vertex of lane ``lane`` of the global tile ``tile`` of WIDE_VOFF (tiles are per mesh)."""
    m = int(np.searchsorted(WIDE_TILE0, tile, side="right") - 1)
    v = int(WIDE_VOFF[m]) + (tile - int(WIDE_TILE0[m])) * 256 + lane
    assert v < WIDE_VOFF[m + 1]
    return v


def plain_increment(theta, lin):
    """The rule as DESIGN.md words it: the largest |theta - lin| and the lowest vertex that attains it."""
    moved = np.abs(theta - lin)
    return float(moved.max()), int(np.argmax(moved))


def exact_pair(n, seed):
    """(theta, lin) in 64ths, so that every |theta - lin| is exact: below 1, of both signs, with many ties."""
    rng = np.random.default_rng(seed)
    lin = rng.integers(-640, 640, n) / 64.0
    return lin + rng.choice([-1.0, 1.0], n) * (rng.integers(0, 64, n) / 64.0), lin


def test_the_increment_is_the_plain_rule_with_ties_across_tiles_and_strides():
    """Equal largest changes in tiles 3 (wave 0), 259 (A's ragged last tile: lane 3 of the second stride) and 300 (D: lane 44 of
    the second stride) go to the lowest vertex; taken away one after the other, the next one wins; a larger one wins wherever it
    sits, the board's last vertex (the ragged tile 360) included."""
    n = int(WIDE_VOFF[-1])
    theta, lin = exact_pair(n, 5)
    assert F.increment(WIDE_VOFF, theta, lin) == plain_increment(theta, lin)
    at = [in_tile(3, 77), in_tile(259, 1), in_tile(300, 200)]
    assert at[1] // 256 == 259 and WIDE_VOFF[1] - at[1] < 256 and at[2] >= WIDE_VOFF[3]
    for sign, v in zip((1.0, -1.0, 1.0), at):
        theta[v] = lin[v] + sign * 2.0
    for k, v in enumerate(at):
        assert F.increment(WIDE_VOFF, theta, lin) == (2.0, v) == plain_increment(theta, lin)
        theta[v] = lin[v]                                    # this one moves no more: the next tie holds the top
    last = n - 1
    assert last == in_tile(360, 129)
    for v in (last, in_tile(259, 0), in_tile(260, 3), in_tile(256, 255), 0):
        theta[v] = lin[v] - 3.0
        assert F.increment(WIDE_VOFF, theta, lin) == (3.0, v) == plain_increment(theta, lin)
        theta[v] = lin[v]
    theta[last], theta[int(WIDE_VOFF[1]) - 1] = lin[last] + 3.0, lin[int(WIDE_VOFF[1]) - 1] - 3.0       # both ragged tiles tie
    assert F.increment(WIDE_VOFF, theta, lin) == (3.0, int(WIDE_VOFF[1]) - 1)


def test_the_increment_of_an_all_equal_vector_and_of_small_boards():
    n = int(WIDE_VOFF[-1])
    lin = np.linspace(0.0, 40.0, n)
    assert F.increment(WIDE_VOFF, lin, lin) == (0.0, 0)                      # the complete tie over 361 tiles
    assert not math.copysign(1.0, F.increment(WIDE_VOFF, lin, lin)[0]) < 0
    assert F.increment(WIDE_VOFF, np.full(n, 4.5), np.full(n, 2.0)) == (2.5, 0)
    for voff in ([0, 255], [0, 256], [0, 257], [0, 0, 300, 300, 513], [0, 1]):      # ragged, full, one into a second tile, empty meshes
        theta, lin = exact_pair(voff[-1], voff[-1])
        assert F.increment(voff, theta, lin) == plain_increment(theta, lin), voff
        theta[-1] = lin[-1] + 1.0                            # the last lane of a ragged last tile
        assert F.increment(voff, theta, lin) == (1.0, voff[-1] - 1)
    assert F.increment([0, 0], np.zeros(0), np.zeros(0)) == (0.0, -1)


def test_the_increment_reads_the_vertices_only():
    """theta and lin run over all potential unknowns; what lies behind voff[-1] (internal nodes) is not looked at."""
    theta, lin = exact_pair(700, 9)
    theta[650] = lin[650] + 50.0
    assert F.increment([0, 300, 600], theta, lin) == plain_increment(theta[:600], lin[:600])

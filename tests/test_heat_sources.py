"""Heat sources on the device against the host restatement (tests/sources_ref.py, itself checked by
tests/test_heat_sources_host.py): the lists, the fallback flags, A_s, the load and the footprint temperatures bit for bit; the
closed form of a footprint over a whole board; the temperatures against a scipy direct solve of the restated operator and
load; the balance of film loss against delivered power plus source heat through every thermal entry point; no change
without sources; bitwise repeatability; the refusals; the pool's guarded mode.

Boards (tests/test_stack.py and tests/test_thermal.py): pair (512 and 288 faces: two 256-tiles and a ragged tail), small (a
layer of two meshes, one of them 2 faces), hole (a footprint over a hole), three (three layers, also coupled through the
dielectric), two_layer (resistor links and internal nodes) and the golden problem_c1.  Every layer with copper gets a
rectangle over all of its meshes, one over its middle and a square far smaller than a face (the fallback); the 16 x 16
boards also get the footprints of tests/test_heat_sources_host.py on their first two layers, two overlapping rectangles
among them, and one run takes 70 small shifted rectangles so that the loops over the sources cross 64."""
import gc
import math

import numpy as np
import pytest

import sources_ref as S
import test_thermal as TT
import thermal_ref as T
import transient_ref as R
from padne_amd import _hip, solver
from test_heat_sources_host import COUNTS, FOOTPRINTS
from test_stack import Stacked, board, interlayer_of
from test_thermal import BAR, FILM_REAL, FILM_STIFF, delivered_power, quiet, random_loads, restated_loads, vertex_temperatures

pytestmark = pytest.mark.gpu

HS = solver.HeatSource
BOARDS = ["pair", "small", "hole", "three", "two_layer", "problem_c1"]
SQUARE16 = ["pair", "small", "hole", "three"]                # boards whose first two layers cover the 16 x 16 square
AMBIENT = 40.0


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def rect(lo, hi):
    return np.array([(lo[0], lo[1]), (hi[0], lo[1]), (hi[0], hi[1]), (lo[0], hi[1])], dtype=np.float64)


_SOURCES: dict = {}


def sources_of(name):
    """[(label, layer index, polygon (n, 2), watts)] of a board, built once."""
    if name in _SOURCES:
        return _SOURCES[name]
    out = []
    if name == "pair70":
        out = [(f"copy{i}", i % 2, rect((1 + 0.19 * i, 2 + 0.17 * i), (2.7 + 0.19 * i, 3.3 + 0.17 * i)), 0.0) for i in range(70)]
    else:
        _prob, _meshes, layer_of, _disc, flat, *_ = board(name)
        for l in sorted(set(layer_of)):
            mine = [flat[m] for m in range(len(flat)) if layer_of[m] == l and len(flat[m][1])]
            pts = np.concatenate([xy for xy, _tri in mine])
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            d = hi - lo
            xy, tri = mine[0]
            p = 0.5 * xy[tri[0, 0]] + 0.3 * xy[tri[0, 1]] + 0.2 * xy[tri[0, 2]]      # inside face 0, off its centroid
            out += [(f"all{l}", l, rect(lo - 0.1 * d, hi + 0.1 * d), 0.0), (f"middle{l}", l, rect(lo + 0.23 * d, lo + 0.61 * d), 0.0),
                    (f"speck{l}", l, rect(p - 1e-7 * d, p + 1e-7 * d), 0.0)]
        if name in SQUARE16:
            for label, polygon in FOOTPRINTS.items():
                # (the tiny square and the disc lie in the hole of the hole board's second layer: that refusal has its own test)
                out += [(f"{label}{l}", l, np.asarray(polygon, dtype=np.float64), 0.0) for l in (0, 1)
                        if not (name == "hole" and label in ("tiny", "disc") and l == 1)]
            out += [("overlap_a", 0, rect((5.0, 5.0), (10.0, 9.0)), 0.0), ("overlap_b", 0, rect((7.5, 6.5), (12.5, 11.0)), 0.0)]
    _SOURCES[name] = [(label, l, polygon, 0.05 * (1 + i % 7)) for i, (label, l, polygon, _w) in enumerate(out)]
    return _SOURCES[name]


def board_name(name):
    return "pair" if name == "pair70" else name


_RESTATED: dict = {}


def restated_of(name):
    """The S.Restated of the board's sources, computed once and left unchanged."""
    if name not in _RESTATED:
        _prob, _meshes, layer_of, _disc, flat, *_ = board(board_name(name))
        _RESTATED[name] = S.Restated(flat, layer_of, [(l, polygon) for _label, l, polygon, _w in sources_of(name)])
    return _RESTATED[name]


def heat_sources_of(name, powers=None):
    prob = board(board_name(name))[0]
    return [HS(prob.layers[l], polygon, w if powers is None else powers[i], name=label)
            for i, (label, l, polygon, w) in enumerate(sources_of(name))]


def attach(dev, name):
    """The board's sources on the handle of ``dev``: what set_sources returns."""
    src = sources_of(name)
    return dev.thermal.set_sources(len(dev.prob.layers), dev.layer_of, [l for _a, l, _p, _w in src], [p for _a, _l, p, _w in src])


def powers_of(name, k, seed=1):
    """(k, n_source) watts; with k > 2 the last column is zero."""
    P = np.random.default_rng(seed).uniform(0.01, 0.4, (k, len(sources_of(name))))
    if k > 2:
        P[k - 1] = 0.0
    return P


def operator_of(dev, coupled):
    return dev.restated()[0] if coupled else T.operator(dev.flat, dev.kappa, dev.film, dev.n_internal, dev.links)[0]


def test_the_footprints_cover_what_the_issue_counted():
    """From the restatement itself, before any comparison with the device: a changed grid cannot turn a case into an empty
    one unnoticed."""
    ref, labels = restated_of("pair"), [label for label, *_ in sources_of("pair")]
    for label, counts in COUNTS.items():
        for l in (0, 1):
            s = labels.index(f"{label}{l}")
            assert ref.counts[s] == max(counts[l], 1) and ref.fallback[s] == (counts[l] == 0), (label, l)
    for name in BOARDS:
        ref, labels = restated_of(name), [label for label, *_ in sources_of(name)]
        specks = [s for s, label in enumerate(labels) if label.startswith("speck")]
        assert specks and ref.fallback[specks].all() and not ref.fallback[[labels.index("all0"), labels.index("middle0")]].any()
    assert (restated_of("pair70").counts > 0).all() and len(restated_of("pair70").counts) == 70
    count_of = lambda name, label: restated_of(name).counts[[a for a, *_ in sources_of(name)].index(label)]      # noqa: E731
    assert 0 < count_of("hole", "grid_lines1") < count_of("pair", "grid_lines1")                                   # over the hole


# ---- 1. lists, A_s, the load, T_s: bit for bit; theta against the direct solve ------------------------------------------------

@pytest.mark.parametrize("name,coupled", [(name, False) for name in BOARDS + ["pair70"]] + [("three", True)])
def test_lists_areas_load_and_footprint_temperatures_are_the_restatement_bit_for_bit(ctx, name, coupled):
    """The load through padne_thermal_load without and with Joule power and triples, 11 columns (a launch of 8 and a ragged
    one of 3).  film = 1e-3: theta against the direct solve of the restated operator (A' with the pairs coupled) and the
    restated load within 1e-8 of max |theta|, the bar tests/test_thermal.py holds the bare solve to."""
    ref = restated_of(name)
    with Stacked(board_name(name), FILM_STIFF, pairs=None if coupled else []) as dev:
        counts, fallback, area = attach(dev, name)
        ptr, face = dev.thermal.source_lists()
        P11 = powers_of(name, 11)
        dev.thermal.source_power(P11)
        Pf, heat = random_loads(dev, 11, seed=3)
        b_bare = dev.thermal.load(np.zeros((11, dev.n_tri)))
        b_full = dev.thermal.load(Pf, heat)
        P3 = powers_of(name, 3, seed=2)
        dev.thermal.source_power(P3)
        theta, res = dev.thermal.solve(Pf[:3], (heat[0][heat[1] < 3], heat[1][heat[1] < 3], heat[2][heat[1] < 3]))
        rises = [dev.thermal.source_report(3) for _ in range(2)]
        face_power = dev.thermal.face_power(3, dev.n_tri)
        again = attach(dev, name)                            # a second call replaces the first: the same lists
        ptr2, face2 = dev.thermal.source_lists()
        dev.thermal.set_sources(len(dev.prob.layers), dev.layer_of, [], [])      # none: the handle of before
        b_none = dev.thermal.load(Pf, heat)
    print(name, "sources", len(counts), "entries", int(counts.sum()), "fallbacks", int(fallback.sum()), "largest list", int(counts.max()))
    assert np.array_equal(counts, ref.counts) and np.array_equal(fallback.astype(bool), ref.fallback)
    assert np.array_equal(ptr, ref.ptr) and np.array_equal(face, ref.face)
    assert np.array_equal(area, ref.A)
    assert all(np.array_equal(a, b) for a, b in zip(again, (counts, fallback, area))) and np.array_equal(ptr2, ptr) and np.array_equal(face2, face)
    added = ref.load(dev.n_pot, P11)
    plain = restated_loads(dev, Pf, heat)
    assert np.array_equal(b_none, plain)
    assert np.array_equal(b_bare, added) and np.array_equal(b_full, plain + added)
    assert (b_bare[10] == 0.0).all() and (added[:, dev.n_vert:] == 0.0).all()
    for j in range(11):
        assert abs(math.fsum(b_bare[j].tolist()) - math.fsum(P11[j].tolist())) <= 1e-13 * max(math.fsum(P11[j].tolist()), 1e-300)
    assert np.array_equal(face_power, Pf[:3])                # the Joule array keeps its meaning
    A = operator_of(dev, coupled)
    b = plain[:3] + ref.load(dev.n_pot, P3)
    assert res.status == _hip.OK
    for j in range(3):
        want = T.solve(A, b[j])
        err = np.abs(theta[j] - want).max()
        print(name, "column", j, "error / max|theta|", err / np.abs(want).max(), "iterations", res.iterations)
        assert err <= BAR * np.abs(want).max()
    assert np.array_equal(rises[0], rises[1])
    assert np.array_equal(rises[0], ref.temperature(theta, 0.0))
    assert (rises[0] > 0.0).all()


@pytest.mark.parametrize("name,coupled", [(name, False) for name in BOARDS] + [("three", True)])
def test_realistic_film_meets_the_residual_bar(ctx, name, coupled):
    """film = 1e-5: ||A theta - b|| <= 1e-11 ||b|| with the restated operator and load, evaluated on the host."""
    ref = restated_of(name)
    with Stacked(name, FILM_REAL, pairs=None if coupled else []) as dev:
        attach(dev, name)
        P2 = powers_of(name, 2)
        dev.thermal.source_power(P2)
        Pf, heat = random_loads(dev, 2, seed=6)
        theta, res = dev.thermal.solve(Pf, heat)
    A = operator_of(dev, coupled)
    b = restated_loads(dev, Pf, heat) + ref.load(dev.n_pot, P2)
    for j in range(2):
        r = np.linalg.norm(A @ theta[j] - b[j]) / np.linalg.norm(b[j])
        print(name, "column", j, "residual", r, "iterations", res.iterations)
        assert r <= 1e-11


# ---- 2. the closed form -------------------------------------------------------------------------------------------------------

def test_a_footprint_over_a_whole_board_gives_the_uniform_temperature(ctx):
    """One mesh, the electrical sources at zero: b = q M_v, so theta = P / (h area) at every vertex, within 1e-8."""
    prob, meshes, layer_of, disc, flat, *_ = TT.board("single")
    dead = {e: 0.0 for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS}
    h, power = 2e-5, 0.75
    model = solver.ThermalModel(film=h, ambient=AMBIENT, heat_sources=[HS.rectangle("F.Cu", -1, -1, 9, 9, power, name="lid")])
    _sols, (rep,), _env = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, cases=[dead])
    xy, tri, *_ = T.flatten(flat)
    area = math.fsum(T.face_area(xy, tri).tolist())
    want = power / (h * area)
    (z,) = vertex_temperatures(rep)
    print("theta", want, "relative deviation", np.abs(z - AMBIENT - want).max() / want)
    assert np.abs(z - AMBIENT - want).max() <= BAR * want
    (entry,) = rep.sources
    assert entry["name"] == "lid" and entry["layer"] == 0 and entry["faces"] == len(tri) and not entry["fallback"]
    assert entry["power"] == power and abs(entry["area"] - area) <= 1e-12 * area
    assert abs(entry["temperature"] - AMBIENT - want) <= BAR * want
    assert rep.source_heat == power and rep.total_heat == power and abs(rep.total_loss - power) <= 1e-9 * power
    assert all(layer["heat"] == 0.0 for layer in rep.layers)


# ---- 3. the balance, through the Problem API ----------------------------------------------------------------------------------

_DELIVERED: dict = {}


def delivered_of(name):
    if name not in _DELIVERED:
        prob, meshes, layer_of, disc, *_ = board(name)
        _sol, currents = quiet(solver.solve_meshed_currents, prob, meshes, layer_of, disconnected_meshes_by_layer=disc)
        _DELIVERED[name] = delivered_power(currents)
    return _DELIVERED[name]


@pytest.mark.parametrize("name,coupled", [(name, False) for name in BOARDS] + [("three", True)])
def test_the_film_loss_is_the_delivered_power_plus_the_source_heat(ctx, name, coupled):
    """total_loss against delivered_power + source_heat within 1e-9 relative (the bar of tests/test_thermal.py), also with the
    layers coupled through the dielectric; the report's entries are the restatement's, and the Joule heat of the layers
    has the bits it has without sources."""
    prob, meshes, layer_of, disc, *_ = board(name)
    kw = dict(film=FILM_STIFF, ambient=AMBIENT, interlayer=interlayer_of(name) if coupled else None)
    _s, rep = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(heat_sources=heat_sources_of(name), **kw),
                    disconnected_meshes_by_layer=disc)
    _s, bare = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(**kw), disconnected_meshes_by_layer=disc)
    ref, src = restated_of(name), sources_of(name)
    want = delivered_of(name) + rep.source_heat
    print(name, "delivered", delivered_of(name), "source heat", rep.source_heat, "loss", rep.total_loss, "relative",
          abs(rep.total_loss - want) / want)
    assert rep.source_heat == math.fsum(w for *_x, w in src) and rep.source_heat > 0
    assert abs(rep.total_loss - want) <= 1e-9 * want and abs(rep.total_heat - want) <= 1e-9 * want
    assert rep.total_heat == bare.total_heat + rep.source_heat and bare.source_heat == 0.0 and bare.sources == []
    assert [layer["heat"] for layer in rep.layers] == [layer["heat"] for layer in bare.layers]
    theta = np.concatenate(vertex_temperatures(rep)) - AMBIENT
    theta = np.concatenate([theta, np.zeros(board(name)[5])])
    temps = ref.temperature(theta, AMBIENT)[0]
    scale = np.abs(theta).max()
    for i, (entry, (label, l, _polygon, w)) in enumerate(zip(rep.sources, src)):
        assert (entry["name"], entry["layer"], entry["power"]) == (label, l, w)
        assert (entry["faces"], entry["fallback"], entry["area"]) == (ref.counts[i], bool(ref.fallback[i]), ref.A[i])
        # (T - ambient gives theta back to an ulp of T, so not the device's bits: those are compared on the handle above)
        assert abs(entry["temperature"] - temps[i]) <= 1e-9 * scale and entry["temperature"] > AMBIENT
    hotter = [a.max() > b.max() for a, b in zip(vertex_temperatures(rep), vertex_temperatures(bare))]
    assert all(hotter)
    assert len(rep.interlayer) == (len(interlayer_of(name)) if coupled else 0)


def test_three_load_cases_one_of_them_dead_with_a_power_per_case(ctx):
    prob, meshes, layer_of, disc, *_ = board("pair")
    electrical = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]
    cases = [{}, {e: 1.7 * e.current for e in electrical}, {e: 0.0 for e in electrical}]
    watts = powers_of("pair", 3)
    heat_sources = heat_sources_of("pair", [tuple(watts[:, i]) for i in range(watts.shape[1])])
    heat_sources[0] = HS(heat_sources[0].layer, heat_sources[0].polygon, 0.0, name=heat_sources[0].name)      # a float serves every case
    watts[:, 0] = 0.0
    model = solver.ThermalModel(film=FILM_STIFF, ambient=AMBIENT, heat_sources=heat_sources)
    kw = dict(cases=cases, disconnected_meshes_by_layer=disc)
    _sols, currents, _env = quiet(solver.solve_meshed_load_case_currents, prob, meshes, layer_of, cases, per_case_fields=False,
                                  disconnected_meshes_by_layer=disc)
    _sols, reps, env = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, **kw)
    _sols, lean, env2 = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, per_case_fields=False, **kw)
    for j, rep in enumerate(reps):
        want = delivered_power(currents[j]) + rep.source_heat
        assert rep.source_heat == math.fsum(watts[j].tolist()) and [e["power"] for e in rep.sources] == watts[j].tolist()
        if j < 2:
            print("case", j, "relative", abs(rep.total_loss - want) / want)
            assert abs(rep.total_loss - want) <= 1e-9 * want and abs(rep.total_heat - want) <= 1e-9 * want
    assert reps[2].total_heat == 0.0 and reps[2].total_loss == 0.0
    assert all((z == AMBIENT).all() for z in vertex_temperatures(reps[2])) and all(e["temperature"] == AMBIENT for e in reps[2].sources)
    assert [e["area"] for e in reps[0].sources] == [e["area"] for e in reps[1].sources]
    for a, b in zip(lean, reps):
        assert a.temperatures is None and TT.scalars(a) == TT.scalars(b) and a.sources == b.sources and a.source_heat == b.source_heat
    assert env2.hotspots == env.hotspots
    for bad in (2, 4):                                       # one power per case, or a float
        wrong = list(heat_sources)
        wrong[3] = HS(wrong[3].layer, wrong[3].polygon, [0.1] * bad, name="short")
        with pytest.raises(ValueError, match="heat_sources.*short"):
            solver.solve_meshed_thermal(prob, meshes, layer_of, solver.ThermalModel(film=FILM_STIFF, heat_sources=wrong), **kw)


# ---- 4. electro-thermal and transient -----------------------------------------------------------------------------------------

def everything(rep):
    return (vertex_temperatures(rep) + [tf.values for forms in rep.face_temperatures for tf in forms],
            (TT.scalars(rep), [sorted(e.items()) for e in rep.interlayer], [sorted(e.items()) for e in rep.sources], rep.source_heat))


def same(rep_a, rep_b):
    (arrays_a, scalars_a), (arrays_b, scalars_b) = everything(rep_a), everything(rep_b)
    return scalars_a == scalars_b and len(arrays_a) == len(arrays_b) and all(np.array_equal(a, b) for a, b in zip(arrays_a, arrays_b))


@pytest.mark.parametrize("name", ["pair", "two_layer"])
def test_alpha_zero_is_the_one_way_path_bit_for_bit(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    thermal = solver.ThermalModel(film=FILM_STIFF, heat_sources=heat_sources_of(name))
    _s, want = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, thermal, disconnected_meshes_by_layer=disc)
    _s, rep, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of,
                              solver.ElectroThermalModel(thermal=thermal, temperature_coefficient=0.0), disconnected_meshes_by_layer=disc)
    assert coupling.rounds == 1 and same(rep, want) and len(rep.sources) == len(sources_of(name))


def test_every_round_of_the_electrothermal_loop_carries_the_same_source_heat_and_balances(ctx):
    prob, meshes, layer_of, disc, *_ = board("pair")
    thermal = solver.ThermalModel(film=FILM_STIFF, heat_sources=heat_sources_of("pair"))
    run = lambda **kw: quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of,      # noqa: E731
                             solver.ElectroThermalModel(thermal=thermal, **kw), disconnected_meshes_by_layer=disc)
    _s, last, full = run()
    assert full.converged and full.rounds > 1
    for r in sorted({1, full.rounds}):
        _s, rep, coupling = run(max_rounds=r)
        delivered = math.fsum(-flow[key] for element, flow in coupling.elements.items()
                              if solver.element_kind(element) != "Resistor" for key in ("power", "input_power") if key in flow)
        want = delivered + rep.source_heat
        print("round", r, "of", full.rounds, "delivered", delivered, "source heat", rep.source_heat, "loss", rep.total_loss)
        assert rep.source_heat == last.source_heat and [e["power"] for e in rep.sources] == [e["power"] for e in last.sources]
        assert abs(rep.total_loss - want) <= 1e-9 * want and abs(rep.total_heat - want) <= 1e-9 * want


CAP = 3e-3


def test_the_transient_load_table_and_states_against_the_restatement(ctx):
    """On the pair: the load table's columns carry the sources of their cases, bit for bit; a schedule of case / none / case
    against transient_ref.run fed with the restated table, every state within 1e-8 of the run's largest theta."""
    ref = restated_of("pair")
    tau = CAP / FILM_STIFF
    schedule = [(tau / 20, 6, 0), (0.05, 5, None), (tau / 20, 6, 1)]
    with Stacked("pair", FILM_STIFF, pairs=[]) as dev:
        attach(dev, "pair")
        capacity = [CAP * (1 + layer) for layer in dev.layer_of]
        tr = _hip.Transient(dev.thermal, capacity)
        try:
            P2 = powers_of("pair", 2)
            dev.thermal.source_power(P2)
            Pf, heat = random_loads(dev, 2, seed=5)
            tr.loads(Pf, heat)
            B = tr.load_vectors()
            tr.start([None])
            states = [tr.state()]
            for dt, steps, case in schedule:
                states.extend(tr.run(dt, steps, [case], np.arange(dev.n_pot, dtype=np.int64))["probes"])
            dev.thermal.source_power(powers_of("pair", 3))   # powers for another number of columns: no load is formed
            with pytest.raises(ValueError):
                tr.loads(Pf, heat)
        finally:
            tr.close()
    A, M, hM = T.operator(dev.flat, dev.kappa, dev.film, dev.n_internal, dev.links)
    B_want = restated_loads(dev, Pf, heat) + ref.load(dev.n_pot, P2)
    assert np.array_equal(B, B_want)
    want = R.run(A, R.capacity(dev.voff, capacity, M), hM, dev.voff, B_want, schedule)[0]
    got = np.stack(states)[:, 0]
    scale = np.abs(want).max()
    print("worst error / max|theta|", np.abs(got - want).max() / scale)
    assert scale > 0 and (np.abs(got - want).max(axis=1) <= BAR * scale).all()


def test_every_step_of_the_transient_balances_with_the_source_heat(ctx):
    prob, meshes, layer_of, disc, *_ = board("pair")
    tau = CAP / FILM_STIFF
    thermal = solver.ThermalModel(film=FILM_STIFF, ambient=AMBIENT, heat_sources=heat_sources_of("pair"))
    model = solver.TransientModel(thermal=thermal, areal_capacity=CAP)
    schedule = [solver.Segment(6 * tau / 20, 6, 0), solver.Segment(5 * 0.05, 5, None), solver.Segment(6 * tau / 20, 6, 0)]
    _sols, rep = quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, model, schedule)
    defect = (rep.total_stored[1:] - rep.total_stored[:-1]) / np.diff(rep.times) + rep.total_loss[1:] - rep.total_heat[1:]
    top = rep.total_heat.max()
    want = delivered_of("pair") + math.fsum(w for *_x, w in sources_of("pair"))
    print("heat", top, "delivered + sources", want, "worst balance defect / heat", np.abs(defect).max() / top)
    assert abs(top - want) <= 1e-9 * want
    assert (rep.total_heat[1:7] == top).all() and (rep.total_heat[7:12] == 0.0).all() and (rep.total_heat[12:] == top).all()
    assert (np.abs(defect) <= 1e-9 * top).all()             # the bar of tests/test_transient.py


# ---- 5. nothing changes without sources; two calls ----------------------------------------------------------------------------

def test_without_sources_everything_has_the_bits_of_before(ctx):
    """Steady, coupled and transient on the pair: ``heat_sources=()`` against the field left alone."""
    prob, meshes, layer_of, disc, *_ = board("pair")
    models = [solver.ThermalModel(film=FILM_STIFF, interlayer=interlayer_of("pair"), heat_sources=empty) for empty in (None, ())]
    steady = [quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, m)[1] for m in models]
    assert same(*steady) and steady[1].sources == [] and steady[1].source_heat == 0.0
    looped = [quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of, solver.ElectroThermalModel(thermal=m))[1] for m in models]
    assert same(*looped)
    schedule = [solver.Segment(0.6, 4, 0), solver.Segment(0.2, 2, None)]
    stepped = [quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, solver.TransientModel(thermal=m, areal_capacity=CAP),
                     schedule)[1] for m in models]
    for key in ("total_stored", "total_loss", "total_heat"):
        assert np.array_equal(getattr(stepped[0], key), getattr(stepped[1], key))
    for a, b in zip(stepped[0].temperatures[-1], stepped[1].temperatures[-1]):
        assert all(np.array_equal(za.values, zb.values) for za, zb in zip(a, b))


@pytest.mark.parametrize("name", ["three", "problem_c1"])
def test_two_calls_give_the_same_bits(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    model = solver.ThermalModel(film=FILM_REAL, heat_sources=heat_sources_of(name))
    runs = [quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, disconnected_meshes_by_layer=disc)[1] for _ in range(2)]
    assert same(*runs)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_of_the_device_entries(ctx):
    square = rect((4.0, 4.0), (8.0, 8.0))
    with Stacked("three", FILM_STIFF, pairs=[]) as dev:
        th, lib = dev.thermal, ctx._lib
        for n_layer, mesh_layer, layers, polygons in (
                (3, [0, 1, 3], [0], [square]), (3, [0, -1, 2], [0], [square]), (3, [0, 1], [0], [square]),      # the meshes' layers
                (3, [0, 1, 2], [3], [square]), (3, [0, 1, 2], [-1], [square]), (0, [0, 1, 2], [0], [square]),   # the source's
                (3, [0, 1, 2], [0], [square[:2]]), (3, [0, 1, 2], [0], [np.tile(square, (65, 1))]),              # 2 and 260 vertices
                (3, [0, 1, 2], [0], [square * np.nan]), (3, [0, 1, 2], [0] * 4097, [square] * 4097)):
            with pytest.raises(ValueError):
                th.set_sources(n_layer, mesh_layer, layers, polygons)
        with pytest.raises(ValueError):                      # no sources yet: nothing to give powers to, nothing to report
            th.source_power(np.zeros((1, 0)))
        for call in (th.source_lists, lambda: th.source_report(1)):
            with pytest.raises(ValueError):
                call()
        counts, fallback, area = th.set_sources(3, dev.layer_of, [0, 2], [square, square])
        ml, sl = _hip._i32(dev.layer_of), _hip._i32([0, 2])
        xy, out = _hip._f64(np.concatenate([square, square])), (np.zeros(2, np.int64), np.zeros(2, np.int32), np.zeros(2))
        P, PI32, PI64, PF64 = _hip._ptr, _hip._PI32, _hip._PI64, _hip._PF64
        for ptr in ([0, 4, 3], [1, 4, 8], [0, 2, 8]):        # a poly_ptr that does not ascend by at least 3 from 0
            pp = _hip._i64(ptr)
            assert lib.padne_thermal_set_sources(ctx._h, th._h, 3, 3, P(ml, PI32), 2, P(sl, PI32), P(pp, PI64), P(xy, PF64),
                                                 P(out[0], PI64), P(out[1], PI32), P(out[2], PF64)) == _hip.E_INVALID
        pp = _hip._i64([0, 4, 8])
        assert lib.padne_thermal_set_sources(ctx._h, th._h, 3, 3, P(ml, PI32), 2, P(sl, PI32), P(pp, PI64), None, P(out[0], PI64),
                                             P(out[1], PI32), P(out[2], PF64)) == _hip.E_INVALID       # a null pointer
        counts, fallback, area = th.set_sources(3, dev.layer_of, [0, 2], [square, square])
        assert (counts > 0).all() and not fallback.any()
        Pf = np.zeros((2, dev.n_tri))
        with pytest.raises(ValueError):                      # sources without powers form no load
            th.load(Pf)
        for bad in (np.full((2, 2), -1.0), np.full((2, 2), np.nan), np.full((2, 2), np.inf), np.zeros((2, 3))):
            with pytest.raises(ValueError):
                th.source_power(bad)
        th.source_power(np.ones((3, 2)))
        with pytest.raises(ValueError):                      # powers for three columns, a load of two: not a silent zero
            th.load(Pf)
        with pytest.raises(ValueError):
            th.solve(Pf)
        with pytest.raises(ValueError):                      # no solve yet
            th.source_report(3)
        th.source_power(np.ones((2, 2)))
        b = th.load(Pf)
        assert abs(math.fsum(b[1].tolist()) - 2.0) <= 1e-13 * 2.0
        with pytest.raises(_hip.SourceOffCopperError) as off:      # beside the board: no centroid, no owner
            th.set_sources(3, dev.layer_of, [0, 1], [square, square + 20.0])
        assert off.value.sources == [1]
        assert np.array_equal(th.load(Pf), np.zeros((2, dev.n_pot)))      # the failed call left the handle without sources
        other = _hip.Context(0)
        try:
            ph = _hip._i64([0, 4])
            rc = lib.padne_thermal_set_sources(other._h, th._h, 3, 3, P(ml, PI32), 1, P(sl, PI32), P(ph, PI64), P(xy, PF64),
                                               P(out[0], PI64), P(out[1], PI32), P(out[2], PF64))
            assert rc == _hip.E_INVALID                      # a handle of another context
        finally:
            other.close()


def test_a_source_off_the_copper_is_refused_and_the_context_still_works(ctx):
    prob, meshes, layer_of, disc, *_ = board("hole")
    good = HS.rectangle(prob.layers[0], 4.2, 5.1, 9.3, 8.4, 0.3, name="U1")
    for lost in (HS.rectangle("L0", 20, 20, 22, 22, 0.2, name="beside"), HS.rectangle("L1", 7.9, 7.9, 8.1, 8.1, 0.2, name="in the hole")):
        model = solver.ThermalModel(film=FILM_STIFF, heat_sources=[good, lost])
        with pytest.raises(ValueError, match=f"heat_sources.*{lost.name}.*{lost.layer}"):
            quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model)
    _s, rep = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(film=FILM_STIFF, heat_sources=[good]))
    want = delivered_of("hole") + 0.3
    assert abs(rep.total_loss - want) <= 1e-9 * want and rep.sources[0]["faces"] == 38


# ---- 7. the guarded pool ------------------------------------------------------------------------------------------------------

def sources_driver(ctx):
    """set_sources + load + solve + report on the three-layer board with its pairs coupled, then the public call."""
    with Stacked("three", FILM_REAL) as dev:
        counts, fallback, area = attach(dev, "three")
        lists = dev.thermal.source_lists()
        dev.thermal.source_power(powers_of("three", 2))
        Pf, heat = random_loads(dev, 2, seed=8)
        b = dev.thermal.load(Pf, heat)
        theta, res = dev.thermal.solve(Pf, heat)
        rises = dev.thermal.source_report(2)
    prob, meshes, layer_of, disc, *_ = board("three")
    model = solver.ThermalModel(film=FILM_REAL, interlayer=interlayer_of("three"), heat_sources=heat_sources_of("three"))
    _s, rep = solver.solve_meshed_thermal(prob, meshes, layer_of, model)
    return [counts, fallback, area, *lists, b, theta, rises, res.iterations, *vertex_temperatures(rep),
            [e["temperature"] for e in rep.sources], rep.total_loss]


def test_the_guarded_poisoned_pool_gives_the_same_bits_and_no_violation(ctx, switches):
    """The driver with PADNE_POOL_GUARD unset, 00 and ff (tests/test_device_memory.py's three ways): every block handed out
    poisoned with the fill byte between guard zones that are checked at its free."""
    runs, stats = [], []
    for mode in (None, "00", "ff"):
        if mode is not None:
            switches.set("PADNE_POOL_GUARD", mode)
        try:
            gc.collect()
            ctx.pool_guard(1)
            out = quiet(sources_driver, ctx)
            runs.append([np.ascontiguousarray(np.asarray(x)).tobytes() for x in out])
            del out
            gc.collect()
            stats.append(ctx.pool_guard(0))
        finally:
            switches.unset("PADNE_POOL_GUARD")
    print("guarded blocks", [s["allocations"] for s in stats])
    for mode, st in zip((None, "00", "ff"), stats):
        assert st["violations"] == 0, (mode, st, ctx._lib.padne_last_error())
    assert stats[0]["allocations"] == 0 and stats[1]["allocations"] > 0 and stats[2]["allocations"] > 0
    assert runs[1] == runs[0] and runs[2] == runs[0]

"""The host restatement of the heat sources (tests/sources_ref.py) checked on its own, on the CPU -- the weights, the load's
sum, coverage against a plain loop, the closed form of a footprint over a whole board -- and what check_thermal_model accepts
and refuses of ``heat_sources``.

Geometry: the 16 x 16 square meshed by synthetic.jittered_grid, 17 x 17 and 13 x 13 vertices (512 and 288 faces)."""
import math

import numpy as np
import pytest

import helpers as H
import sources_ref as S
import thermal_ref as T
from padne_amd import problem as P, solver
from test_stack_host import grid, three_layer_problem

HS = solver.HeatSource
MESHES, LAYER_OF = [grid(17, 1), grid(13, 2)], [0, 1]
L_SHAPE = [(3, 3), (11, 3), (11, 6), (6, 6), (6, 12), (3, 12)]
FOOTPRINTS = {"rectangle": HS.rectangle(0, 4.2, 5.1, 9.3, 8.4, 1.0).polygon, "tiny": HS.rectangle(0, 7.01, 7.01, 7.05, 7.05, 1.0).polygon,
              "l_shape": L_SHAPE, "disc": HS.disc(0, (8, 8), 2.5, 1.0, segments=40).polygon,
              "everything": HS.rectangle(0, -1, -1, 17, 17, 1.0).polygon, "grid_lines": HS.rectangle(0, 4, 4, 8, 8, 1.0).polygon,
              "half_off": HS.rectangle(0, 12.3, 2.2, 20.0, 6.1, 1.0).polygon}
COUNTS = {"rectangle": (38, 17), "tiny": (0, 0), "l_shape": (84, 51), "disc": (39, 22), "everything": (512, 288)}


def both_layers(names):
    return [(layer, FOOTPRINTS[name]) for name in names for layer in (0, 1)]


@pytest.fixture(scope="module")
def restated():
    return S.Restated(MESHES, LAYER_OF, both_layers(list(FOOTPRINTS)))


def test_the_footprints_cover_what_the_issue_counted():
    cover = S.coverage(MESHES, LAYER_OF, both_layers(list(COUNTS)))
    assert [tuple(int(n) for n in cover[2 * i:2 * i + 2].sum(axis=1)) for i in range(len(COUNTS))] == list(COUNTS.values())
    assert not cover[0::2, 512:].any() and not cover[1::2, :512].any()      # a source stays on its layer


def test_the_weights_of_every_source_sum_to_one(restated):
    w = S.weights(restated.face_area, restated.ptr, restated.face, restated.A)
    for s in range(len(restated.counts)):
        total = math.fsum(w[restated.ptr[s]:restated.ptr[s + 1]].tolist())
        assert abs(total - 1.0) <= 4 * np.finfo(np.float64).eps, (s, total)
    assert restated.fallback.tolist() == [name == "tiny" for name in FOOTPRINTS for _ in (0, 1)]
    assert (restated.counts[restated.fallback] == 1).all() and (restated.A > 0).all()


def test_the_load_sums_to_the_power(restated):
    rng = np.random.default_rng(0)
    power = rng.uniform(0.1, 3.0, (2, len(restated.counts)))
    power[1, 3] = 0.0
    b = restated.load(len(restated.xy), power)
    for j in range(2):
        want = math.fsum(power[j].tolist())
        assert abs(math.fsum(b[j].tolist()) - want) <= 1e-13 * want
    # one source at a time: the load lies on the corners of its faces only
    for s in (0, 2, 5):
        one = np.zeros(len(restated.counts))
        one[s] = 2.5
        b = restated.load(len(restated.xy), one)[0]
        mine = restated.face[restated.ptr[s]:restated.ptr[s + 1]]
        assert set(np.flatnonzero(b)) == set(restated.tri[mine].reshape(-1)) and abs(math.fsum(b.tolist()) - 2.5) <= 1e-13 * 2.5


def test_coverage_of_a_rectangle_against_a_plain_loop():
    x0, y0, x1, y1 = 4.2, 5.1, 9.3, 8.4
    xy, tri, face_mesh, _voff, _toff = T.flatten(MESHES)
    cover = S.coverage(MESHES, LAYER_OF, [(0, FOOTPRINTS["rectangle"]), (1, FOOTPRINTS["rectangle"])])
    for f, (a, b, c) in enumerate(tri.tolist()):
        cx = (xy[a][0] + xy[b][0] + xy[c][0]) / 3.0
        cy = (xy[a][1] + xy[b][1] + xy[c][1]) / 3.0
        within = x0 < cx < x1 and y0 < cy < y1
        assert bool(cover[face_mesh[f], f]) == within and not cover[1 - face_mesh[f], f]


def test_concave_self_intersecting_and_clockwise_polygons_follow_the_even_odd_rule():
    cx, cy = np.array([4.0, 8.0, 4.5, 12.0]), np.array([4.0, 8.0, 11.0, 4.0])
    assert S.inside(L_SHAPE, cx, cy).tolist() == [True, False, True, False]
    assert S.inside(L_SHAPE[::-1], cx, cy).tolist() == [True, False, True, False]
    bow = [(0, 0), (4, 4), (4, 0), (0, 4)]                  # a bow tie: its two lobes are inside, the notches are not
    assert S.inside(bow, np.array([1.0, 3.0, 2.0, 2.0]), np.array([2.0, 2.0, 0.5, 3.5])).tolist() == [True, True, False, False]


def test_a_footprint_over_the_whole_board_gives_the_uniform_solution():
    """b = q M_v for q = P / area, so theta = P / (h area) at every vertex, on any mesh, within 1e-12 relative."""
    for mesh_xy_tri in (grid(17, 1), grid(13, 2), grid(9, 4, size=8.0, ny=17)):
        meshes = [mesh_xy_tri]
        r = S.Restated(meshes, [0], [(0, FOOTPRINTS["everything"])])
        assert r.counts[0] == len(r.tri)
        h, power = 2e-5, 0.75
        A, M, _hM = T.operator(meshes, [0.0149], [h], 0, [])
        theta = T.solve(A, r.load(len(r.xy), [[power]])[0])
        want = power / (h * math.fsum(r.face_area.tolist()))
        assert np.abs(theta - want).max() <= 1e-12 * want
        assert np.abs(r.temperature(theta, 25.0)[0, 0] - (25.0 + want)) <= 1e-12 * want


def test_a_footprint_on_no_face_is_refused_by_the_restatement():
    with pytest.raises(ValueError):
        S.lists(MESHES, LAYER_OF, [(0, HS.rectangle(0, 20, 20, 22, 22, 1.0).polygon)])


# ---- check_thermal_model ---------------------------------------------------------------------------------------------------

def test_sources_are_resolved_by_layer_object_and_by_name():
    prob = three_layer_problem()
    model = solver.ThermalModel(film=1e-5, heat_sources=[HS.rectangle(prob.layers[2], 0, 0, 2, 1, 0.5, name="U1"),
                                                         HS("In1.Cu", L_SHAPE, [0.1, 0.0, 0.3])])
    first, second = solver.check_thermal_model(prob, model).sources
    assert (first.name, first.layer, first.power) == ("U1", 2, 0.5)
    assert first.polygon == ((0.0, 0.0), (2.0, 0.0), (2.0, 1.0), (0.0, 1.0))
    assert (second.name, second.layer, second.power) == ("source 1", 1, (0.1, 0.0, 0.3))
    assert second.polygon == tuple((float(x), float(y)) for x, y in L_SHAPE)


def test_no_sources_is_the_checked_model_of_today():
    prob = three_layer_problem()
    plain = solver.check_thermal_model(prob, solver.ThermalModel(film=1e-5))
    for empty in (None, (), []):
        checked = solver.check_thermal_model(prob, solver.ThermalModel(film=1e-5, heat_sources=empty))
        assert checked == plain and checked.sources == []
    assert solver.ThermalModel(film=1e-5).heat_sources is None


def twin_layers():
    layers = [P.Layer(shape=H.Geoms(1), name=name, conductance=2.0) for name in ("F.Cu", "F.Cu", "B.Cu")]
    c = [P.Connection(layer=layers[0], point=H.XY(1, 1)), P.Connection(layer=layers[2], point=H.XY(7, 7))]
    net = P.Network(connections=c, elements=[P.Resistor(a=c[0].node_id, b=c[1].node_id, resistance=0.01)])
    return P.Problem(layers=layers, networks=[net])


SQUARE = [(0, 0), (1, 0), (1, 1), (0, 1)]


@pytest.mark.parametrize("heat_sources", [
    [("F.Cu", SQUARE, 1.0)], "F.Cu", 5, {"F.Cu": 1.0}, HS("F.Cu", SQUARE, 1.0),                  # no HeatSource, no sequence
    [HS("nowhere", SQUARE, 1.0)], [HS(None, SQUARE, 1.0)],                                        # no layer
    [HS("F.Cu", [(0, 0), (1, 0)], 1.0)], [HS("F.Cu", [0, 0, 1, 0, 1, 1], 1.0)], [HS("F.Cu", [(0, 0, 0), (1, 0, 0), (1, 1, 0)], 1.0)],
    [HS("F.Cu", "polygon", 1.0)], [HS("F.Cu", [(0, 0), (1, float("nan")), (1, 1)], 1.0)],
    [HS("F.Cu", [(0, 0), (1, float("inf")), (1, 1)], 1.0)], [HS("F.Cu", [(0, 0), (1, 1), (2, 2)], 1.0)],
    [HS("F.Cu", [(0, 0), (1, 1), (0, 0), (1, 1)], 1.0)],                                          # zero signed area
    [HS.disc("F.Cu", (0, 0), 1.0, 1.0, segments=257)],                                            # more than 256 vertices
    [HS("F.Cu", SQUARE, -1.0)], [HS("F.Cu", SQUARE, float("nan"))], [HS("F.Cu", SQUARE, float("inf"))], [HS("F.Cu", SQUARE, "hot")],
    [HS("F.Cu", SQUARE, None)], [HS("F.Cu", SQUARE, [1.0, -2.0])], [HS("F.Cu", SQUARE, [1.0, "x"])], [HS("F.Cu", SQUARE, [[1.0], [2.0]])],
    [HS("F.Cu", SQUARE, 1.0)] * 4097])
def test_refusals_of_check_thermal_model(heat_sources):
    with pytest.raises(ValueError, match="heat_sources"):
        solver.check_thermal_model(three_layer_problem(), solver.ThermalModel(film=1e-5, heat_sources=heat_sources))


def test_a_layer_name_that_names_several_layers_is_refused():
    with pytest.raises(ValueError, match="heat_sources.*names 2 layers"):
        solver.check_thermal_model(twin_layers(), solver.ThermalModel(film=1e-5, heat_sources=[HS("F.Cu", SQUARE, 1.0)]))


def test_the_largest_counts_are_taken():
    prob = three_layer_problem()
    model = solver.ThermalModel(film=1e-5, heat_sources=[HS.disc("F.Cu", (0, 0), 1.0, 1.0, segments=256)] * 4096)
    assert len(solver.check_thermal_model(prob, model).sources) == 4096


def test_the_number_of_powers_is_checked_against_the_cases():
    prob = three_layer_problem()
    checked = solver.check_thermal_model(prob, solver.ThermalModel(film=1e-5, heat_sources=[HS("F.Cu", SQUARE, [1.0, 2.0]),
                                                                                           HS("B.Cu", SQUARE, 0.5)]))
    assert solver._source_powers(checked.sources, 2).tolist() == [[1.0, 0.5], [2.0, 0.5]]
    assert solver._source_powers([], 3) is None
    for k in (1, 3):
        with pytest.raises(ValueError, match="heat_sources"):
            solver._source_powers(checked.sources, k)


def test_reports_default_to_no_sources():
    rep = solver.ThermalReport(temperatures=None, face_temperatures=None, disconnected_temperatures=[], hotspots=[], layers=[],
                               elements={}, total_heat=0.0, total_loss=0.0, info={})
    assert rep.sources == [] and rep.source_heat == 0.0 and rep.interlayer == []
    checked = solver.CheckedThermalModel(film=[1e-5], kappa=[1.0], links={}, ambient=25.0, element_heat=True)
    assert checked.sources == [] and checked.interlayer == []


def test_the_helpers_polygons():
    assert HS.rectangle("F.Cu", 1, 2, 4, 3, 0.5, name="Q1") == HS("F.Cu", [(1, 2), (4, 2), (4, 3), (1, 3)], 0.5, "Q1")
    disc = HS.disc("F.Cu", (8.0, 3.0), 2.5, 1.0)
    ring = np.asarray(disc.polygon)
    assert ring.shape == (32, 2) and disc.name is None and disc.power == 1.0
    assert np.abs(np.hypot(ring[:, 0] - 8.0, ring[:, 1] - 3.0) - 2.5).max() <= 1e-14
    assert ring[0].tolist() == [10.5, 3.0] and ring[8, 1] == 5.5
    x, y = ring[:, 0], ring[:, 1]
    area = 0.5 * np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)
    assert abs(area - 0.5 * 32 * 2.5 ** 2 * math.sin(2 * math.pi / 32)) <= 1e-12      # counter-clockwise, the regular 32-gon
    assert np.asarray(HS.disc("F.Cu", (0, 0), 1.0, 1.0, segments=40).polygon).shape == (40, 2)


def test_a_partition_over_several_gpus_stays_refused():
    class World:
        world = 2
    prob = three_layer_problem()
    model = solver.ThermalModel(film=1e-5, heat_sources=[HS("F.Cu", SQUARE, 1.0)])
    with pytest.raises(ValueError, match="one GPU|several|partition"):
        solver.solve_meshed_thermal(prob, [], [], model, partition=World())

"""Host half of the thermal model (no GPU): the restatement of tests/thermal_ref.py against solutions that are known, so that
the device tests compare against something that is itself checked; and ``check_thermal_model``'s refusals and defaults,
which come before the device."""
import math

import numpy as np
import pytest

import helpers as H
import thermal_ref as T
from padne_amd import problem as P, solver, synthetic

KAPPA, FILM = 0.025, 2e-5


def grid(n, width=8.0, jitter=0.2, seed=3):
    xy, tri = synthetic.jittered_grid(n, n, h=width / (n - 1), seed=seed, jitter=jitter)
    return np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int64).reshape(-1, 3)


def test_uniform_heating_gives_q_over_h():
    """P_f = q A_f heats every vertex to theta = q / h exactly in exact arithmetic (K annihilates constants): within 1e-10
    relative here (measured <= 6e-12 for grids up to 65^2, jitter 0 and 0.2)."""
    q = 3e-4
    for jitter in (0.0, 0.2):
        xy, tri = grid(17, jitter=jitter)
        A, M, hM = T.operator([(xy, tri)], [KAPPA], [FILM], 0, [])
        theta = T.solve(A, T.load(len(xy), tri, q * T.face_area(xy, tri)))
        err = np.abs(theta - q / FILM).max() / (q / FILM)
        print("jitter", jitter, "relative error", err)
        assert err <= 1e-10
        assert abs(M.sum() - 64.0) <= 1e-12 * 64.0                     # the lumped areas tile the 8 x 8 square


def test_manufactured_solution_converges_at_second_order():
    """theta = cos(pi x / W) on the unjittered W x W grid (the |cot| weights do not converge on obtuse faces, README
    "Goal-oriented error") with P_f = (kappa pi^2 / W^2 + h) cos(pi x_c / W) A_f at the centroid: the largest vertex error
    falls by a factor in [3.9, 4.1] per halving over n = 9, 17, 33, 65 (measured 3.985, 3.996, 3.999)."""
    W = 8.0
    errors = []
    for n in (9, 17, 33, 65):
        xy, tri = grid(n, width=W, jitter=0.0)
        A, _M, _hM = T.operator([(xy, tri)], [KAPPA], [FILM], 0, [])
        xc = xy[tri].mean(axis=1)[:, 0]
        P_f = (KAPPA * math.pi ** 2 / W ** 2 + FILM) * np.cos(math.pi * xc / W) * T.face_area(xy, tri)
        theta = T.solve(A, T.load(len(xy), tri, P_f))
        errors.append(float(np.abs(theta - np.cos(math.pi * xy[:, 0] / W)).max()))
    rates = [a / b for a, b in zip(errors, errors[1:])]
    print("errors", errors, "rates", rates)
    assert all(3.9 <= r <= 4.1 for r in rates), rates


def two_mesh_case():
    """Two jittered 17 x 17 meshes, an internal node between them through two links, and heat at the node."""
    xy0, tri0 = grid(17, seed=1)
    xy1, tri1 = grid(17, seed=2)
    meshes = [(xy0, tri0), (xy1, tri1)]
    n_vert = 2 * 289
    links = [(40, n_vert, 0.02), (n_vert, 289 + 200, 0.005), (10, 289 + 10, 0.0)]
    return meshes, links, n_vert


def test_the_film_loss_balances_the_heat_load():
    """sum h M theta = sum b within 1e-12 relative (measured <= 4e-15): K and the links annihilate constants."""
    meshes, links, n_vert = two_mesh_case()
    A, _M, hM = T.operator(meshes, [KAPPA, 2 * KAPPA], [FILM, 3 * FILM], 1, links)
    xy, tri, face_mesh, _voff, _toff = T.flatten(meshes)
    rng = np.random.default_rng(5)
    V = rng.uniform(0, 1, n_vert)
    b = T.load(n_vert + 1, tri, T.face_power(xy, tri, face_mesh, [1.7, 0.9], V), heat=[(n_vert, 0.3), (40, 0.1)])
    theta = T.solve(A, b)
    loss, heat = math.fsum((hM * theta[:n_vert]).tolist()), math.fsum(b.tolist())
    print("loss", loss, "heat", heat, "relative", abs(loss - heat) / heat)
    assert abs(loss - heat) <= 1e-12 * heat
    assert (theta > 0).all()
    # the zero-conductance link stamps nothing
    assert A[10, 289 + 10] == 0.0


def test_the_face_power_is_the_quadratic_form_of_the_stiffness():
    """sum_f P_f = -V^T K_sigma V: the weights' form is what the assembled rows dissipate."""
    meshes, _links, n_vert = two_mesh_case()
    xy, tri, face_mesh, _voff, _toff = T.flatten(meshes)
    V = np.random.default_rng(7).uniform(-1, 1, n_vert)
    K = T.stiffness(meshes, [1.7, 0.9], 0, [])
    total = math.fsum(T.face_power(xy, tri, face_mesh, [1.7, 0.9], V).tolist())
    assert abs(total + V @ (K @ V)) <= 1e-12 * total


def test_the_envelope_rule_is_sequential():
    values = np.array([[1.0, 2.0, 0.0], [1.0, 3.0, 0.0], [2.0, 3.0, 0.0]])
    best, case = T.envelope(values)
    assert best.tolist() == [2.0, 3.0, 0.0] and case.tolist() == [2, 1, 0]
    env, which = solver.envelope_of(values)
    assert np.array_equal(env, best) and np.array_equal(which, case)


# ---- check_thermal_model -------------------------------------------------------------------------------------------------

def board():
    """Two layers; a source on the top layer, a sense resistor chain top -> internal node -> bottom."""
    top = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=2.0)
    bottom = P.Layer(shape=H.Geoms(1), name="B.Cu", conductance=1.0)
    c = [P.Connection(layer=top, point=H.XY(1, 1)), P.Connection(layer=top, point=H.XY(7, 7)),
         P.Connection(layer=bottom, point=H.XY(7, 7))]
    mid = P.NodeID()
    source = P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0)
    r1 = P.Resistor(a=c[1].node_id, b=mid, resistance=0.01)
    r2 = P.Resistor(a=mid, b=c[2].node_id, resistance=0.02)
    net = P.Network(connections=c, elements=[source, r1, r2])
    return P.Problem(layers=[top, bottom], networks=[net]), top, bottom, source, r1, r2


def test_wiedemann_franz_defaults():
    prob, _top, _bottom, _source, r1, r2 = board()
    checked = solver.check_thermal_model(prob, solver.ThermalModel(film=1e-5))
    assert checked.film == [1e-5, 1e-5] and checked.ambient == 25.0 and checked.element_heat
    assert checked.kappa == [2.44e-8 * 293.15 * 2.0, 2.44e-8 * 293.15 * 1.0]
    assert checked.links == {r1: 2.44e-8 * 293.15 / 0.01, r2: 2.44e-8 * 293.15 / 0.02}
    # 35 um copper: sigma = 5.96e7 S/m * 35e-6 m gives 0.0149 W/K (0.0135 W/K from k = 385 W/(m K))
    assert abs(2.44e-8 * 293.15 * 5.96e7 * 35e-6 - 0.0149) < 5e-5


def test_overrides_by_layer_name_and_element():
    prob, top, _bottom, _source, r1, r2 = board()
    model = solver.ThermalModel(film={"F.Cu": 1e-5, "B.Cu": 2e-5}, sheet_conductance={top: 0.02}, link_conductance={r1: 0.5},
                                ambient=40.0, element_heat=False)
    checked = solver.check_thermal_model(prob, model)
    assert checked.film == [1e-5, 2e-5] and checked.kappa[0] == 0.02 and checked.kappa[1] == 2.44e-8 * 293.15
    assert checked.links[r1] == 0.5 and checked.links[r2] == 2.44e-8 * 293.15 / 0.02
    assert checked.ambient == 40.0 and not checked.element_heat


@pytest.mark.parametrize("bad", [0.0, -1e-5, float("nan"), float("inf"), "warm", None])
def test_a_bad_film_is_refused(bad):
    prob = board()[0]
    with pytest.raises(ValueError):
        solver.check_thermal_model(prob, solver.ThermalModel(film=bad))
    with pytest.raises(ValueError):
        solver.check_thermal_model(prob, solver.ThermalModel(film={"F.Cu": 1e-5, "B.Cu": bad}))


def test_a_layer_without_a_film_is_refused():
    prob = board()[0]
    with pytest.raises(ValueError, match="B.Cu"):
        solver.check_thermal_model(prob, solver.ThermalModel(film={"F.Cu": 1e-5}))


@pytest.mark.parametrize("bad", [0.0, -0.01, float("nan"), float("inf")])
def test_a_bad_sheet_conductance_is_refused(bad):
    prob = board()[0]
    with pytest.raises(ValueError):
        solver.check_thermal_model(prob, solver.ThermalModel(film=1e-5, sheet_conductance={"F.Cu": bad}))


@pytest.mark.parametrize("bad", [-0.01, float("nan"), float("inf")])
def test_a_bad_link_conductance_is_refused(bad):
    prob, _top, _bottom, _source, r1, _r2 = board()
    with pytest.raises(ValueError):
        solver.check_thermal_model(prob, solver.ThermalModel(film=1e-5, link_conductance={r1: bad}))


def test_keys_that_are_not_of_the_problem_are_refused():
    prob, _top, _bottom, source, _r1, _r2 = board()
    stranger = P.Layer(shape=H.Geoms(1), name="In1.Cu", conductance=1.0)
    for model in (solver.ThermalModel(film={"F.Cu": 1e-5, "B.Cu": 1e-5, "In1.Cu": 1e-5}),
                  solver.ThermalModel(film=1e-5, sheet_conductance={stranger: 0.02}),
                  solver.ThermalModel(film=1e-5, link_conductance={P.Resistor(a=P.NodeID(), b=P.NodeID(), resistance=1.0): 0.1}),
                  solver.ThermalModel(film=1e-5, link_conductance={source: 0.1})):
        with pytest.raises(ValueError):
            solver.check_thermal_model(prob, model)


def test_a_zero_link_that_orphans_an_internal_node_is_refused():
    prob, _top, _bottom, _source, r1, r2 = board()
    # one link cut: the node still reaches the bottom layer
    solver.check_thermal_model(prob, solver.ThermalModel(film=1e-5, link_conductance={r1: 0.0}))
    with pytest.raises(ValueError, match="Resistor"):
        solver.check_thermal_model(prob, solver.ThermalModel(film=1e-5, link_conductance={r1: 0.0, r2: 0.0}))


def test_other_bad_arguments_are_refused():
    prob = board()[0]
    for model in (solver.ThermalModel(film=1e-5, ambient=float("nan")), solver.ThermalModel(film=1e-5, reference_temperature=0.0),
                  {"film": 1e-5}):
        with pytest.raises(ValueError):
            solver.check_thermal_model(prob, model)
    with pytest.raises(ValueError):
        solver.solve_meshed_thermal(prob, [], [], solver.ThermalModel(film=-1.0))


def test_heat_triples_halve_every_resistors_power():
    pairs = [(None, ("I", 0, 1, 2.0)), (None, ("R", 3, 7, 0.5)), (None, ("R", 7, 9, 0.25))]
    flows = [[{"power": -1.0}, {"power": 0.6}, {"power": 0.2}], [{"power": -2.0}, {"power": 0.0}, {"power": 0.8}]]
    node, col, val = solver.thermal_heat_triples(pairs, flows)
    assert node.tolist() == [3, 7, 7, 9, 3, 7, 7, 9] and col.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert val.tolist() == [0.3, 0.3, 0.1, 0.1, 0.0, 0.0, 0.4, 0.4]

"""Heat conduction between stacked layers on the device against the host restatement (tests/stack_ref.py, itself checked by
tests/test_stack_host.py): the link slots, G, A', the flows and the areas bit for bit; the temperatures against a scipy direct
solve of the restated A'; the balances; load cases, the electro-thermal and the transient paths with ``interlayer`` set;
bitwise repeatability; the refusals; the pool's guarded mode.

Boards (the smallest that cross the kernels' seams):
  pair      17 x 17 over 13 x 13 on the 16 x 16 square: 289 and 169 vertices, more than one 256-tile with a ragged tail
  matched   17 x 17 over itself: every query on a vertex and on edges of the target, weights exactly 0
  three     17 / 13 / 9 on three layers, pairs (0, 1) and (1, 2): the middle layer's diagonal collects from two pairs
  small     a layer with two meshes, one of 2 faces, over a full layer
  half      an upper layer half as wide as the lower
  hole      a lower layer with a hole
  neck      an upper layer narrowed to a neck, over a plane
  two_layer of tests/test_thermal.py: a via lattice and a sense resistor -- resistor links and coupling links on the same unknowns
  the goldens problem_c1, problem_many_meshes, problem_two_planes with every pair of distinct layers coupled"""
import itertools
import math

import numpy as np
import pytest

import coupled_ref as C
import helpers as H
import stack_ref as K
import test_thermal as TT
import thermal_ref as T
from padne_amd import _hip, mesh, problem as P, solver, synthetic
from test_stack_host import G, grid, with_hole
from test_thermal import BAR, FILM_REAL, FILM_STIFF, Device, delivered_power, quiet, random_loads, restated_loads, sorted_csr
from test_thermal import vertex_temperatures

pytestmark = pytest.mark.gpu

OWN = ["pair", "matched", "three", "small", "half", "hole", "neck"]
GOLDEN = ["problem_c1", "problem_many_meshes", "problem_two_planes"]
BOARDS = OWN + ["two_layer"] + GOLDEN
PER_LAYER = [name for name in BOARDS if name not in ("two_layer", "problem_many_meshes")]      # boards without internal nodes


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def as_mesh(xy, tri):
    return mesh.Mesh(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3))


def neck_mesh():
    """The 17 x 17 grid without the faces above and below a neck of width 4 in its middle."""
    xy, tri = grid(17, 1)
    c = xy[tri].mean(axis=1)
    keep = ~((c[:, 0] > 6) & (c[:, 0] < 10) & ((c[:, 1] < 6) | (c[:, 1] > 10)))
    used = np.unique(tri[keep])
    new = np.full(len(xy), -1, dtype=np.int64)
    new[used] = np.arange(len(used))
    return xy[used], new[tri[keep]]


def own_board(name):
    """(problem, meshes, layer of each mesh): a current source on the top layer, and one resistor from every further
    layer to the layer above it, so that every mesh belongs to the electrical system."""
    flat = {"pair": [grid(17, 1), grid(13, 2)], "matched": [grid(17, 3), grid(17, 3)], "three": [grid(17, 1), grid(13, 2), grid(9, 4)],
            "small": [grid(17, 1), (np.array([[20.0, 20.0], [21.0, 20.0], [21.0, 21.0], [20.0, 21.0]]), np.array([[0, 1, 2], [0, 2, 3]])),
                      grid(13, 2, size=24.0)],
            "half": [grid(9, 1, size=8.0, ny=17), grid(13, 2)], "hole": [grid(17, 1), with_hole(*grid(13, 2), 5.0, 11.0)],
            "neck": [neck_mesh(), grid(13, 2)]}[name]
    layer_of = {"three": [0, 1, 2], "small": [0, 0, 1]}.get(name, [0, 1])
    layers = [P.Layer(shape=H.Geoms(1), name=f"L{i}", conductance=2.0 - 0.5 * i) for i in range(max(layer_of) + 1)]
    at = lambda l, x, y: P.Connection(layer=layers[l], point=H.XY(x, y))      # noqa: E731
    c = [at(0, 2, 8), at(0, 6, 8) if name == "half" else at(0, 14, 8)]
    elements = [P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0)]
    for l in range(1, len(layers)):
        a, b = at(l - 1, 3, 3), at(l, 3, 3)
        c += [a, b]
        elements.append(P.Resistor(a=a.node_id, b=b.node_id, resistance=0.01))
    if name == "small":                                     # the 2-face mesh joins the circuit through a resistor of its own
        a, b = at(0, 12, 12), at(0, 20, 20)
        c += [a, b]
        elements.append(P.Resistor(a=a.node_id, b=b.node_id, resistance=0.02))
    prob = P.Problem(layers=layers, networks=[P.Network(connections=c, elements=elements)])
    return prob, [as_mesh(*m) for m in flat], layer_of


_OWN_BOARDS: dict = {}


def board(name):
    """The tuple tests/test_thermal.py's board() gives -- (problem, meshes, layer_of, disconnected meshes by layer, the flat
    (xy, tri) tuples, n_internal, element pairs) -- for the boards of this file, built once; its own for the others."""
    if name not in OWN:
        return TT.board(name)
    if name not in _OWN_BOARDS:
        prob, meshes, layer_of = own_board(name)
        vindex = solver.VertexIndexer.create(meshes)
        nodes = solver.NodeIndexer.create(prob, meshes, layer_of, vindex, list(prob.networks))
        pairs = solver.global_elements(list(prob.networks), nodes)
        flat = [(np.asarray(m.points, dtype=np.float64), np.asarray(m.triangles, dtype=np.int64)) for m in meshes]
        _OWN_BOARDS[name] = (prob, meshes, layer_of, [[] for _ in prob.layers], flat, nodes.internal_node_count, pairs)
    return _OWN_BOARDS[name]


def pairs_of(name, g=G):
    """Every pair of distinct layers that holds a connected mesh, neighbours only on the three-layer board; a different g each."""
    layers = sorted(set(board(name)[2]))
    found = [(a, b) for a, b in itertools.combinations(layers, 2) if name != "three" or b == a + 1]
    return [(a, b, g * (1 + 0.25 * i)) for i, (a, b) in enumerate(found)]


def interlayer_of(name, g=G):
    prob = board(name)[0]
    return {(prob.layers[a], prob.layers[b].name): gp for a, b, gp in pairs_of(name, g)}


def no_links(name):
    return {e: 0.0 for n in board(name)[0].networks for e in n.elements if solver.element_kind(e) == "Resistor"}


class Stacked(Device):
    """tests/test_thermal.py's Device with the handle made by padne_thermal_create_stacked."""

    def __init__(self, name, film, pairs=None, **model_kw):      # (Device's, on the boards of this file too)
        self.prob, meshes, self.layer_of, disc, self.flat, self.n_internal, self.pairs = board(name)
        self.checked = solver.check_thermal_model(self.prob, TT.model_of(film, **model_kw))
        self.kappa, self.film = TT.per_mesh(self.checked, self.layer_of)
        self.links = TT.links_of(self.pairs, self.checked)
        self.board = solver.index_board(self.prob, meshes, self.layer_of, None, disc)
        self.cases = solver.check_load_cases(self.prob, [{}])
        self.xy, self.tri, self.face_mesh, self.voff, self.toff = T.flatten(self.flat)
        self.n_vert, self.n_tri = len(self.xy), len(self.tri)
        self.n_pot = self.n_vert + self.n_internal
        self.pairs_g = pairs_of(name) if pairs is None else pairs

    def __enter__(self):
        self._stack = self.board.assembled()
        self.L, _ = self._stack.__enter__()
        self.thermal = self.make(self.pairs_g)
        return self

    def make(self, pairs, mesh_layer=None, **kw):
        return _hip.Thermal(self.L.dev, self.n_pot, self.kappa, self.film, [l[0] for l in self.links], [l[1] for l in self.links],
                            [l[2] for l in self.links], mesh_layer=self.layer_of if mesh_layer is None else mesh_layer,
                            pairs=pairs, **kw)

    def restated(self):
        return K.operator(self.flat, self.layer_of, self.kappa, self.film, self.n_internal, self.links, self.pairs_g)


# ---- 1. slots, G, A' -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOARDS)
def test_slots_coupling_and_operator_are_the_restatement_bit_for_bit(ctx, name):
    with Stacked(name, FILM_REAL) as dev:
        sizes = dev.thermal.stack_sizes()
        off, vert, owner, w, c = dev.thermal.stack_links()
        indptr, indices, data, diag = dev.thermal.stack_matrix()
        A = sorted_csr(dev.thermal.matrix().to_scipy())
        raw = dev.thermal.matrix().to_scipy()
        M = dev.thermal.lumped(dev.n_vert)
        _flow, area = dev.thermal.stack_flows(0)
        bare = dev.make([])                                  # n_pair = 0 through the new entry
        A_bare = bare.matrix().to_scipy()
        bare.close()
        plain = _hip.Thermal(dev.L.dev, dev.n_pot, dev.kappa, dev.film, [l[0] for l in dev.links], [l[1] for l in dev.links],
                             [l[2] for l in dev.links])
        A_plain = plain.matrix().to_scipy()
        plain.close()
    A_want, G_want, diag_want, M_want, _hM, (off_w, vert_w, owner_w, w_w, c_w) = dev.restated()
    assert sizes == (len(dev.pairs_g), 2 * len(dev.pairs_g), len(vert_w), G_want.nnz)
    assert np.array_equal(off, off_w) and np.array_equal(vert, vert_w) and np.array_equal(owner, owner_w)
    assert np.array_equal(w, w_w) and np.array_equal(c, c_w)
    print(name, "slots", len(vert), "without an owner", int((owner < 0).sum()), "zero conductances", int((c == 0.0).sum()),
          "entries of G", G_want.nnz, "of A", A_plain.nnz, "of A'", A.nnz)
    assert np.array_equal(indptr, G_want.indptr) and np.array_equal(indices, G_want.indices)
    assert np.array_equal(data, G_want.data) and np.array_equal(diag, diag_want)
    assert np.array_equal(M, M_want)
    assert (np.diff(raw.indices)[np.diff(np.repeat(np.arange(dev.n_pot), np.diff(raw.indptr))) == 0] > 0).all()   # columns ascend
    assert H.same_structure(A, A_want) and np.array_equal(A.data, A_want.data)
    assert (A.diagonal() > 0.0).all()
    for other in (A_bare,):
        assert np.array_equal(other.indptr, A_plain.indptr) and np.array_equal(other.indices, A_plain.indices)
        assert np.array_equal(other.data, A_plain.data)
    _f, area_want = K.flows(dev.flat, dev.layer_of, dev.pairs_g, G_want, np.zeros((0, dev.n_pot)))
    assert np.array_equal(area, area_want)
    if name == "matched":
        assert np.array_equal(np.sort(w, axis=1), np.tile([0.0, 0.0, 1.0], (len(w), 1)))
    if name in ("half", "hole", "neck", "small"):
        assert (owner < 0).any()


def test_a_layer_no_pair_names_is_left_out_of_the_search(ctx):
    """Three layers, one pair: the third layer's faces are not indexed, its vertices emit nothing, its rows are A's."""
    with Stacked("three", FILM_REAL, pairs=[(0, 1, G)]) as dev:
        off, vert, owner, w, c = dev.thermal.stack_links()
        A = sorted_csr(dev.thermal.matrix().to_scipy())
        _flow, area = dev.thermal.stack_flows(0)
    A_want, G_want, _diag, _M, _hM, (off_w, vert_w, owner_w, w_w, c_w) = dev.restated()
    assert np.array_equal(off, off_w) and np.array_equal(vert, vert_w) and np.array_equal(owner, owner_w)
    assert np.array_equal(w, w_w) and np.array_equal(c, c_w)
    assert H.same_structure(A, A_want) and np.array_equal(A.data, A_want.data)
    assert vert.max() < dev.voff[2] and (np.diff(G_want.indptr)[dev.voff[2]:] == 0).all()
    assert np.array_equal(area, K.flows(dev.flat, dev.layer_of, dev.pairs_g, G_want, np.zeros((0, dev.n_pot)))[1])


# ---- 2. theta and the flows --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOARDS)
def test_temperatures_against_the_direct_solve_and_flows_bit_for_bit(ctx, name):
    """film = 1e-3: the bar tests/test_thermal.py holds the uncoupled operator to, 1e-8 of max |theta|.  The flows are the
    restatement's on the device's own theta, bit for bit; a -> b and b -> a differ in sign."""
    with Stacked(name, FILM_STIFF) as dev:
        Pf, heat = random_loads(dev, 3, seed=5)
        theta, res = dev.thermal.solve(Pf, heat)
        flow, area = dev.thermal.stack_flows(3)
        with pytest.raises(ValueError):
            dev.thermal.stack_flows(2)                       # the solve had three columns
    A, Goff, _diag, _M, _hM, _s = dev.restated()
    b = restated_loads(dev, Pf, heat)
    assert res.status == _hip.OK
    for j in range(3):
        want = T.solve(A, b[j])
        err = np.abs(theta[j] - want).max()
        print(name, "column", j, "error / max|theta|", err / max(np.abs(want).max(), 1e-300), "iterations", res.iterations)
        assert err <= BAR * np.abs(want).max()
    assert (theta[2] == 0.0).all() and not np.signbit(theta[2]).any()
    flow_want, area_want = K.flows(dev.flat, dev.layer_of, dev.pairs_g, Goff, theta)
    assert np.array_equal(flow, flow_want) and np.array_equal(area, area_want)
    assert (flow[2] == 0.0).all() and (area > 0.0).all()
    if dev.pairs_g:                                          # (a golden with one layer has no pair)
        back, _ = K.flows(dev.flat, dev.layer_of, [(b_, a, g) for a, b_, g in dev.pairs_g], Goff, theta)
        assert (np.abs(flow + back) <= 1e-12 * np.abs(flow).max()).all()


@pytest.mark.parametrize("name", BOARDS)
def test_realistic_film_meets_the_residual_bar(ctx, name):
    """film = 1e-5 under g = 1.5e-3: ||A' theta - b|| <= 1e-11 ||b|| with the restated A', evaluated on the host."""
    with Stacked(name, FILM_REAL) as dev:
        Pf, heat = random_loads(dev, 2, seed=6)
        theta, res = dev.thermal.solve(Pf, heat)
    A = dev.restated()[0]
    b = restated_loads(dev, Pf, heat)
    for j in range(2):
        r = np.linalg.norm(A @ theta[j] - b[j]) / np.linalg.norm(b[j])
        print(name, "column", j, "residual", r, "iterations", res.iterations)
        assert r <= 1e-11


# ---- 3. through the Problem API --------------------------------------------------------------------------------------------

def strip_pair():
    """tests/test_coupled.py's uniform strip (a uniform current density, so a uniform heat per area) over a copy of its own
    mesh on a second layer that hangs on one resistor and carries no current."""
    top = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=C.STRIP_SIGMA)
    bottom = P.Layer(shape=H.Geoms(1), name="B.Cu", conductance=1.0)
    xy, tri = synthetic.jittered_grid(C.STRIP_N, C.STRIP_N, h=C.STRIP_H, seed=0, jitter=0.0)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    J = 0.05
    connections, elements = [], []
    for f, t, current in C.strip_sources(J):
        a, b = P.Connection(layer=top, point=H.XY(*xy[f])), P.Connection(layer=top, point=H.XY(*xy[t]))
        connections += [a, b]
        elements.append(P.CurrentSource(f=a.node_id, t=b.node_id, current=current))
    a, b = P.Connection(layer=top, point=H.XY(*xy[40])), P.Connection(layer=bottom, point=H.XY(*xy[40]))
    hang = P.Resistor(a=a.node_id, b=b.node_id, resistance=1.0)
    prob = P.Problem(layers=[top, bottom], networks=[P.Network(connections=connections + [a, b], elements=elements + [hang])])
    return prob, [as_mesh(xy, tri), as_mesh(xy, tri)], [0, 1], J * J / C.STRIP_SIGMA, hang


def test_the_matched_pair_follows_the_closed_form(ctx):
    """Uniform heat q per area on the top layer only: both layers are uniform, theta_1 = q / (h1 + g h2 / (g + h2)) and
    theta_2 = g theta_1 / (g + h2), within 1e-8 relative."""
    prob, meshes, layer_of, q, hang = strip_pair()
    h1, h2 = 1e-5, 3e-5
    model = solver.ThermalModel(film={"F.Cu": h1, "B.Cu": h2}, ambient=0.0, link_conductance={hang: 0.0}, element_heat=False,
                                interlayer={("F.Cu", "B.Cu"): G})
    _sol, rep = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model)
    t1 = q / (h1 + G * h2 / (G + h2))
    t2 = G * t1 / (G + h2)
    top, bottom = vertex_temperatures(rep)
    print("top", top.min(), top.max(), "closed form", t1, "bottom", bottom.min(), bottom.max(), "closed form", t2)
    assert np.abs(top - t1).max() <= 1e-8 * t1 and np.abs(bottom - t2).max() <= 1e-8 * t2
    (entry,) = rep.interlayer
    assert entry["layers"] == (0, 1) and entry["conductance"] == G
    assert abs(entry["area"] - 64.0) <= 1e-12 * 64.0
    assert abs(entry["flow"] - h2 * 64.0 * t2) <= 1e-8 * entry["flow"]


@pytest.mark.parametrize("name", BOARDS)
def test_the_film_loss_is_the_power_the_sources_deliver_and_every_layer_balances(ctx, name):
    """total_loss equals the power the sources deliver within 1e-9 relative (the bar of tests/test_coupled.py), with the
    pairs coupled; and with no heat in the elements and no thermal link through a resistor, every layer's heat is its film
    loss plus what it passes on through the dielectric, to the same bar of the board's heat."""
    prob, meshes, layer_of, disc, *_ = board(name)
    _sol, currents = quiet(solver.solve_meshed_currents, prob, meshes, layer_of, disconnected_meshes_by_layer=disc)
    delivered, copper = delivered_power(currents), math.fsum(currents.layers)
    inter = interlayer_of(name)
    _s, rep = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(film=FILM_STIFF, interlayer=inter),
                    disconnected_meshes_by_layer=disc)
    print(name, "delivered", delivered, "loss", rep.total_loss, "relative", abs(rep.total_loss - delivered) / delivered)
    assert delivered > 0
    assert abs(rep.total_loss - delivered) <= 1e-9 * delivered and abs(rep.total_heat - delivered) <= 1e-9 * delivered
    # an internal node needs its links, and the layers then exchange heat through them too: such boards end here
    assert (name in PER_LAYER) == (board(name)[5] == 0)
    if name not in PER_LAYER:
        return
    _s, bare = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of,
                     solver.ThermalModel(film=FILM_STIFF, interlayer=inter, element_heat=False, link_conductance=no_links(name)),
                     disconnected_meshes_by_layer=disc)
    assert abs(bare.total_loss - copper) <= 1e-9 * copper
    for layer in bare.layers:
        print(name, layer)
        assert abs(layer["heat"] - (layer["loss"] + layer["exchange"])) <= 1e-9 * copper
    assert abs(math.fsum(layer["exchange"] for layer in bare.layers)) <= 1e-12 * copper
    assert len(bare.interlayer) == len(inter) and all(e["area"] > 0.0 for e in bare.interlayer)
    for (a, b, g), entry in zip(pairs_of(name), bare.interlayer):
        assert entry["layers"] == (a, b) and entry["conductance"] == g


def test_the_per_layer_balance_covers_the_boards_it_is_meant_to():
    assert PER_LAYER == OWN + ["problem_c1", "problem_two_planes"]


def hottest(rep, layer):
    return rep.hotspots[layer][0]


def test_a_neck_over_a_plane_is_cooler_and_the_plane_is_warmer_than_ambient(ctx):
    prob, meshes, layer_of, disc, *_ = board("neck")
    kw = dict(film=FILM_REAL, ambient=25.0, link_conductance=no_links("neck"), element_heat=False)
    _s, alone = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(**kw))
    _s, over = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(interlayer=interlayer_of("neck"), **kw))
    print("neck alone", hottest(alone, 0), "over the plane", hottest(over, 0), "plane", hottest(alone, 1), hottest(over, 1))
    assert hottest(over, 0) < hottest(alone, 0)
    assert hottest(alone, 1) == 25.0 and hottest(over, 1) > 25.0
    assert alone.interlayer == [] and all(layer["exchange"] == 0.0 for layer in alone.layers)
    assert over.interlayer[0]["flow"] > 0.0


# ---- 4. load cases, electro-thermal, transient ------------------------------------------------------------------------------

def everything(rep):
    return (vertex_temperatures(rep) + [tf.values for forms in rep.face_temperatures for tf in forms],
            (TT.scalars(rep), [sorted(e.items()) for e in rep.interlayer]))


@pytest.mark.parametrize("name", ["three", "two_layer"])
def test_three_load_cases_one_of_them_dead(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]
    cases = [{}, {e: 1.7 * e.current for e in sources}, {e: 0.0 for e in sources}]
    model = solver.ThermalModel(film=FILM_STIFF, ambient=40.0, interlayer=interlayer_of(name))
    sols, reps, env = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, cases=cases, disconnected_meshes_by_layer=disc)
    assert all((z == 40.0).all() for z in vertex_temperatures(reps[2]))
    assert all(e["flow"] == 0.0 for e in reps[2].interlayer) and all(l["exchange"] == 0.0 for l in reps[2].layers)
    assert reps[2].total_heat == 0.0 and reps[2].total_loss == 0.0
    assert all(abs(e1["flow"]) > abs(e0["flow"]) > 0.0 for e0, e1 in zip(reps[0].interlayer, reps[1].interlayer))
    assert [e["area"] for e in reps[0].interlayer] == [e["area"] for e in reps[1].interlayer]
    best, which = solver.envelope_of([np.concatenate(vertex_temperatures(rep)) for rep in reps])
    assert np.array_equal(np.concatenate([zf.values for forms in env.temperatures for zf in forms]), best)
    assert np.array_equal(np.concatenate([c for cs in env.cases for c in cs]), which)


@pytest.mark.parametrize("name", ["pair", "two_layer"])
def test_every_alpha_zero_is_the_one_way_path_bit_for_bit(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    kw = dict(disconnected_meshes_by_layer=disc)
    thermal = solver.ThermalModel(film=FILM_STIFF, interlayer=interlayer_of(name))
    _s, want = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, thermal, **kw)
    _s, rep, coupling = quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of,
                              solver.ElectroThermalModel(thermal=thermal, temperature_coefficient=0.0), **kw)
    assert coupling.rounds == 1
    (arrays_a, scalars_a), (arrays_b, scalars_b) = everything(rep), everything(want)
    assert scalars_a == scalars_b and all(np.array_equal(a, b) for a, b in zip(arrays_a, arrays_b))
    assert len(rep.interlayer) == len(pairs_of(name))


def test_every_round_of_the_electrothermal_loop_balances(ctx):
    """Copper's alpha on the pair (the 2 A of two_layer on its 8 x 8 sheets run away at this film, with or without the
    dielectric): the loop converges in more than one round, and stopped after r = 1 .. rounds rounds (max_rounds = r) the
    report of round r balances -- film loss and heat against the power the sources deliver in that round's electrical
    solve within 1e-9 relative (the bar of tests/test_coupled.py), the layers' exchanges summing to nothing."""
    prob, meshes, layer_of, disc, *_ = board("pair")
    thermal = solver.ThermalModel(film=FILM_STIFF, interlayer=interlayer_of("pair"))
    run = lambda **kw: quiet(solver.solve_meshed_electrothermal, prob, meshes, layer_of,      # noqa: E731
                             solver.ElectroThermalModel(thermal=thermal, **kw), disconnected_meshes_by_layer=disc)
    _s, _rep, full = run()
    assert full.converged and full.rounds > 1
    losses = []
    for r in range(1, full.rounds + 1):
        _s, rep, coupling = run(max_rounds=r)
        delivered = math.fsum(-flow[key] for element, flow in coupling.elements.items()
                              if solver.element_kind(element) != "Resistor" for key in ("power", "input_power") if key in flow)
        print("round", r, "of", full.rounds, "delivered", delivered, "loss", rep.total_loss, "heat", rep.total_heat,
              "exchange", [layer["exchange"] for layer in rep.layers])
        assert coupling.rounds == r and coupling.converged == (r == full.rounds) and delivered > 0
        assert abs(rep.total_loss - delivered) <= 1e-9 * delivered and abs(rep.total_heat - delivered) <= 1e-9 * delivered
        assert abs(math.fsum(layer["exchange"] for layer in rep.layers)) <= 1e-12 * delivered
        assert rep.interlayer[0]["flow"] > 0.0
        losses.append(rep.total_loss)
    assert len(set(losses)) == len(losses)                   # the rounds differ: the loop did move


def test_the_transient_honours_the_pairs(ctx):
    """Every step balances (stored_{n+1} - stored_n) / dt + loss_{n+1} against the heat of its case within 1e-9 of the run's
    largest heat (the bar of tests/test_transient.py), and a long constant segment ends at solve_meshed_thermal's answer."""
    prob, meshes, layer_of, disc, *_ = board("pair")
    film, cap = 1e-3, 3e-3
    tau = cap / film
    thermal = solver.ThermalModel(film=film, ambient=40.0, interlayer=interlayer_of("pair"))
    model = solver.TransientModel(thermal=thermal, areal_capacity=cap)
    schedule = [solver.Segment(12 * tau / 20, 12, 0), solver.Segment(8 * 0.05, 8, None)] + \
               [solver.Segment(5 * tau, 1, 0) for _ in range(40)]
    _sols, rep = quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, model, schedule, keep="segments")
    dts = np.diff(rep.times)
    defect = (rep.total_stored[1:] - rep.total_stored[:-1]) / dts + rep.total_loss[1:] - rep.total_heat[1:]
    top = rep.total_heat.max()
    print("worst balance defect / heat", np.abs(defect).max() / top)
    assert top > 0 and (np.abs(defect) <= 1e-9 * top).all()
    _s, steady = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, thermal)
    want = np.concatenate(vertex_temperatures(steady))
    end = np.concatenate([zf.values for forms in rep.temperatures[-1] for zf in forms])
    scale = np.abs(want - 40.0).max()
    print("end of the run against the steady state, relative", np.abs(end - want).max() / scale)
    assert np.abs(end - want).max() <= 1e-6 * scale
    # without the pair the same board ends elsewhere: the transient really ran on A'
    _s, alone = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(film=film, ambient=40.0))
    assert np.abs(np.concatenate(vertex_temperatures(alone)) - want).max() > 1e-3 * scale


@pytest.mark.parametrize("name", ["three", "problem_many_meshes"])
def test_two_calls_give_the_same_bits(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    model = solver.ThermalModel(film=FILM_REAL, interlayer=interlayer_of(name))
    runs = [quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, disconnected_meshes_by_layer=disc)[1] for _ in range(2)]
    (arrays_a, scalars_a), (arrays_b, scalars_b) = everything(runs[0]), everything(runs[1])
    assert scalars_a == scalars_b
    assert len(arrays_a) == len(arrays_b) and all(np.array_equal(a, b) for a, b in zip(arrays_a, arrays_b))


# ---- 5. refusals, the guarded pool ------------------------------------------------------------------------------------------

def test_refusals_of_the_device_entries(ctx):
    with Stacked("three", FILM_STIFF) as dev:
        for mesh_layer, pairs, kw in (([0, 1, 3], [(0, 1, G)], dict(n_layer=3)), ([0, -1, 2], [(0, 1, G)], {}),
                                      ([0, 1, 2], [(1, 1, G)], {}), ([0, 1, 2], [(0, 1, G), (1, 0, G)], {}),
                                      ([0, 1, 2], [(0, 1, G), (0, 1, G)], {}), ([0, 1, 2], [(0, 1, -G)], {}),
                                      ([0, 1, 2], [(0, 1, float("nan"))], {}), ([0, 1, 2], [(0, 1, float("inf"))], {}),
                                      ([0, 1, 2], [(0, 3, G)], dict(n_layer=3)), ([0, 1], [(0, 1, G)], {})):
            with pytest.raises(ValueError):
                dev.make(pairs, mesh_layer=mesh_layer, **kw)
        with pytest.raises(ValueError):
            _hip.Thermal(dev.L.dev, dev.n_pot, dev.kappa, dev.film, [l[0] for l in dev.links], [l[1] for l in dev.links],
                         [l[2] for l in dev.links], pairs=[(0, 1, G)])                 # pairs without mesh_layer
        with pytest.raises(ValueError):                    # no solve yet
            dev.thermal.stack_flows(1)
        plain = _hip.Thermal(dev.L.dev, dev.n_pot, dev.kappa, dev.film, [l[0] for l in dev.links], [l[1] for l in dev.links],
                             [l[2] for l in dev.links])
        try:
            for call in (plain.stack_sizes, plain.stack_links, plain.stack_matrix, lambda: plain.stack_flows(0)):
                with pytest.raises((ValueError, RuntimeError)):
                    call()
        finally:
            plain.close()
        zero = dev.make([(0, 1, 0.0), (1, 2, G)])            # g = 0 is no pair: no side, no flow, no area
        try:
            assert zero.stack_sizes()[:2] == (2, 2)
            _f, area = zero.stack_flows(0)
            assert area[0] == 0.0 and area[1] > 0.0
        finally:
            zero.close()


def stacked_driver(ctx):
    """Stacked create + solve + flows on the three-layer board."""
    with Stacked("three", FILM_REAL) as dev:
        Pf, heat = random_loads(dev, 2, seed=8)
        theta, res = dev.thermal.solve(Pf, heat)
        flow, area = dev.thermal.stack_flows(2)
        A = sorted_csr(dev.thermal.matrix().to_scipy())
        links = dev.thermal.stack_links()
    return [theta, flow, area, A.indptr, A.indices, A.data, *links, res.iterations]


def test_the_guarded_poisoned_pool_gives_the_same_bits_and_no_violation(ctx, switches):
    """The driver with PADNE_POOL_GUARD unset, 00 and ff (tests/test_device_memory.py's three ways): every block handed out
    poisoned with the fill byte between guard zones that are checked at its free."""
    import gc
    runs, stats = [], []
    for mode in (None, "00", "ff"):
        if mode is not None:
            switches.set("PADNE_POOL_GUARD", mode)
        try:
            gc.collect()
            ctx.pool_guard(1)
            out = quiet(stacked_driver, ctx)
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

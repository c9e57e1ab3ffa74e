"""The thermal model on the device against the host restatement (tests/thermal_ref.py, itself checked by
tests/test_thermal_host.py): the operator, the lumped areas and the heat load bit for bit; the temperatures against a scipy
direct solve; the balance of film loss and delivered power; the device-side face powers; load cases and their envelope;
the report; bitwise repeatability.

Boards (small, but across the kernels' seams): one jittered 17 x 17 mesh (289 vertices: more than a wave and more than a
256-thread workgroup, with a ragged last tile); two such meshes on two layers joined by a via lattice, with a source and a
sense resistor through an internal node; a layer holding two meshes, one of them of 2 faces; the Problem-level goldens."""
import math
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H
import sensitivity_ref as S
import thermal_ref as T
from oracle import padne_oracle as O
from padne_amd import _hip, mesh, problem as P, solver, synthetic
from test_currents import board_of
from test_load_case_currents import finished_block

pytestmark = pytest.mark.gpu

PROBLEMS = H.problem_golden_names()
SYNTHETIC = ["single", "two_layer", "two_in_layer"]
BOARDS = SYNTHETIC + PROBLEMS
BAR = 1e-8                   # of max |theta|: the project's bar for potentials
FILM_STIFF, FILM_REAL = 1e-3, 1e-5


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        return fn(*args, **kwargs)


def grid_mesh(seed, origin=(0.0, 0.0), jitter=0.2):
    xy, tri = synthetic.jittered_grid(17, 17, h=0.5, seed=seed, jitter=jitter, origin=origin)
    return mesh.Mesh(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3))


def conn(layer, x, y):
    return P.Connection(layer=layer, point=H.XY(x, y))


def synthetic_board(name):
    """(problem, meshes, mesh_index_to_layer_index)."""
    top = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=2.0)
    if name == "single":
        c = [conn(top, 1, 1), conn(top, 7, 7), conn(top, 2, 6), conn(top, 6, 2)]
        net = P.Network(connections=c, elements=[P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0),
                                                 P.Resistor(a=c[2].node_id, b=c[3].node_id, resistance=0.05)])
        return P.Problem(layers=[top], networks=[net]), [grid_mesh(1)], [0]
    if name == "symmetric":                                # an unjittered grid: mirror images in x, in y and in the diagonal
        c = [conn(top, 1, 1), conn(top, 7, 7)]
        net = P.Network(connections=c, elements=[P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=1.0)])
        return P.Problem(layers=[top], networks=[net]), [grid_mesh(0, jitter=0.0)], [0]
    if name == "two_layer":
        bottom = P.Layer(shape=H.Geoms(1), name="B.Cu", conductance=1.0)
        c = [conn(top, 1, 1), conn(bottom, 7, 7), conn(top, 6, 2), conn(bottom, 6, 2)]
        mid = P.NodeID()
        elements = [P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0),
                    P.Resistor(a=c[2].node_id, b=mid, resistance=0.004), P.Resistor(a=mid, b=c[3].node_id, resistance=0.008)]
        for x in (2, 4, 6):                                 # the via lattice
            for y in (3, 5):
                a, b = conn(top, x, y), conn(bottom, x, y)
                c += [a, b]
                elements.append(P.Resistor(a=a.node_id, b=b.node_id, resistance=0.002))
        return P.Problem(layers=[top, bottom], networks=[P.Network(connections=c, elements=elements)]), \
            [grid_mesh(1), grid_mesh(2)], [0, 1]
    if name == "two_in_layer":
        small = mesh.Mesh(np.array([[20.0, 20.0], [21.0, 20.0], [21.0, 21.0], [20.0, 21.0]]),
                          np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))
        c = [conn(top, 1, 1), conn(top, 20, 20), conn(top, 21, 21), conn(top, 7, 7)]
        net = P.Network(connections=c, elements=[P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=1.5),
                                                 P.Resistor(a=c[2].node_id, b=c[3].node_id, resistance=0.01)])
        return P.Problem(layers=[top], networks=[net]), [grid_mesh(4), small], [0, 0]
    raise KeyError(name)


_BOARDS: dict = {}


def board(name):
    """(problem, meshes, layer_of, disconnected meshes by layer, the flat (xy, tri) tuples in mesh order, n_internal,
    element pairs on global unknowns), built once per module."""
    if name not in _BOARDS:
        if name in SYNTHETIC + ["symmetric"]:
            prob, meshes, layer_of = synthetic_board(name)
            disc = [[] for _ in prob.layers]
            vindex = solver.VertexIndexer.create(meshes)
            nodes = solver.NodeIndexer.create(prob, meshes, layer_of, vindex, list(prob.networks))
            pairs, n_internal = solver.global_elements(list(prob.networks), nodes), nodes.internal_node_count
        else:
            system = S.problem_system(name)
            meshes, disc = board_of(system, name)
            prob, layer_of, pairs, n_internal = system.prob, system.layer_of, system.pairs, system.n_internal
        flat = [(np.asarray(m.points, dtype=np.float64), np.asarray(m.triangles, dtype=np.int64)) for m in meshes]
        _BOARDS[name] = (prob, meshes, layer_of, disc, flat, n_internal, pairs)
    return _BOARDS[name]


def resistors(name):
    return [element for element, row in board(name)[6] if row[0] == "R"]


def model_of(film, **kw):
    return solver.ThermalModel(film=film, **kw)


def per_mesh(checked, layer_of):
    return [checked.kappa[l] for l in layer_of], [checked.film[l] for l in layer_of]


def links_of(pairs, checked):
    return [(row[1], row[2], checked.links[element]) for element, row in pairs if row[0] == "R"]


class Device:
    """A board assembled on the device with its thermal handle, kept open for one test."""

    def __init__(self, name, film, cases=({},), **model_kw):
        self.prob, meshes, self.layer_of, disc, self.flat, self.n_internal, self.pairs = board(name)
        self.checked = solver.check_thermal_model(self.prob, model_of(film, **model_kw))
        self.kappa, self.film = per_mesh(self.checked, self.layer_of)
        self.links = links_of(self.pairs, self.checked)
        self.board = solver.index_board(self.prob, meshes, self.layer_of, None, disc)
        self.cases = solver.check_load_cases(self.prob, list(cases))
        self.xy, self.tri, self.face_mesh, self.voff, self.toff = T.flatten(self.flat)
        self.n_vert, self.n_tri = len(self.xy), len(self.tri)
        self.n_pot = self.n_vert + self.n_internal

    def __enter__(self):
        self._stack = self.board.assembled()
        self.L, _ = self._stack.__enter__()
        self.thermal = _hip.Thermal(self.L.dev, self.n_pot, self.kappa, self.film, [l[0] for l in self.links],
                                    [l[1] for l in self.links], [l[2] for l in self.links])
        return self

    def __exit__(self, *exc):
        self.thermal.close()
        return self._stack.__exit__(*exc)

    def restated(self):
        return T.operator(self.flat, self.kappa, self.film, self.n_internal, self.links)

    def solved_block(self):
        self.plan, self.V = finished_block(self.board, self.L, self.cases)
        return self.plan, self.V


def sorted_csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def random_loads(dev, k, seed):
    """k columns of face powers and some node heat, one of the columns empty."""
    rng = np.random.default_rng(seed)
    Pf = rng.uniform(0.0, 1e-3, (k, dev.n_tri))
    nodes = rng.integers(0, dev.n_pot, 5 * k)
    cols = rng.integers(0, k, 5 * k)
    vals = rng.uniform(0.0, 1e-2, 5 * k)
    nodes[:2] = nodes[0]                                   # two triples on one unknown of one column: list order matters
    cols[:2] = cols[0]
    if k > 2:
        Pf[k - 1] = 0.0
        vals[cols == k - 1] = 0.0
    return Pf, (nodes, cols, vals)


def restated_loads(dev, Pf, heat):
    nodes, cols, vals = heat
    return np.stack([T.load(dev.n_pot, dev.tri, Pf[j], [(int(n), float(v)) for n, c, v in zip(nodes, cols, vals) if c == j])
                     for j in range(len(Pf))])


# ---- 1. A, M_v and b ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOARDS)
def test_operator_lumped_areas_and_load_are_the_restatement_bit_for_bit(ctx, name):
    """K's entries are the reference assembly's with kappa and the links (resistors of 1 / g), bit for bit; M_v and b are
    the restatement's bits; A's diagonal at a vertex is the one rounded sum (-K_ii) + h M_v."""
    # links g = 1 / R_th for thermal resistances R_th the reference assembly can be given: its 1 / R_th is g exactly
    link_g = {element: 1.0 / (37.0 + i) for i, element in enumerate(resistors(name))}
    with Device(name, FILM_REAL, link_conductance=link_g) as dev:
        A = sorted_csr(dev.thermal.matrix().to_scipy())
        M = dev.thermal.lumped(dev.n_vert)
        Pf, heat = random_loads(dev, 11, seed=3)           # 11 columns: a full launch of 8 and a ragged one of 3
        b = dev.thermal.load(Pf, heat)
    A_want, M_want, hM = dev.restated()
    assert np.array_equal(M, M_want)
    assert H.same_structure(A, A_want)
    assert np.array_equal(A.data, sorted_csr(A_want).data)
    # the reference assembly with kappa for sigma: every link a resistor whose 1 / R is the link's g exactly
    rows = [("R", a, b_, 37.0 + i) for i, (a, b_, _g) in enumerate(dev.links)]
    K, _ = O.assemble_system([(xy, tri, k) for (xy, tri), k in zip(dev.flat, dev.kappa)], dev.n_internal, rows, 0)
    K = sorted_csr(K[:dev.n_pot, :dev.n_pot])
    K.eliminate_zeros()
    assert H.same_structure(A, K)
    off_A, d_A = H.offdiag_and_diag(A)
    off_K, d_K = H.offdiag_and_diag(K)
    assert np.array_equal(sorted_csr(off_A).data, -sorted_csr(off_K).data)
    assert np.array_equal(d_A[:dev.n_vert], (-d_K[:dev.n_vert]) + hM)
    assert np.array_equal(d_A[dev.n_vert:], -d_K[dev.n_vert:])
    assert np.array_equal(b, restated_loads(dev, Pf, heat))
    assert (b[-1] == 0.0).all()


# ---- 2. theta against the direct solve -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOARDS)
def test_temperatures_against_the_direct_solve(ctx, name):
    """film = 1e-3: cond(A) is about 5e2, so rtol 1e-12 leaves the error below 1e-9; the bar is 1e-8 of max |theta|."""
    with Device(name, FILM_STIFF) as dev:
        Pf, heat = random_loads(dev, 3, seed=5)
        theta, res = dev.thermal.solve(Pf, heat)
    A, _M, _hM = dev.restated()
    b = restated_loads(dev, Pf, heat)
    assert res.status == _hip.OK
    for j in range(3):
        want = T.solve(A, b[j])
        err = np.abs(theta[j] - want).max()
        print(name, "column", j, "error / max|theta|", err / max(np.abs(want).max(), 1e-300), "iterations", res.iterations)
        assert err <= BAR * np.abs(want).max()
    assert (theta[2] == 0.0).all() and not np.signbit(theta[2]).any()        # a zero column: exact zeros


@pytest.mark.parametrize("name", BOARDS)
def test_realistic_film_meets_the_residual_bar(ctx, name):
    """film = 1e-5: cond(A) is about 5e4.  ||A theta - b|| <= 1e-11 ||b|| with the restated A, evaluated on the host; the
    error against the direct solve is printed."""
    with Device(name, FILM_REAL) as dev:
        Pf, heat = random_loads(dev, 2, seed=6)
        theta, res = dev.thermal.solve(Pf, heat)
    A, _M, _hM = dev.restated()
    b = restated_loads(dev, Pf, heat)
    for j in range(2):
        r = np.linalg.norm(A @ theta[j] - b[j]) / np.linalg.norm(b[j])
        want = T.solve(A, b[j])
        print(name, "column", j, "residual", r, "error / max|theta|", np.abs(theta[j] - want).max() / np.abs(want).max(),
              "iterations", res.iterations)
        assert r <= 1e-11


# ---- 3. uniform heating --------------------------------------------------------------------------------------------------

def test_uniform_heating_through_the_device_solve(ctx):
    """P_f = q A_f: theta = q / h at every vertex within 1e-9 relative."""
    q, film = 3e-4, 2e-5
    prob, meshes, layer_of, _disc, flat, _n_internal, _pairs = board("single")
    with Device("single", film, link_conductance={e: 0.0 for n in prob.networks for e in n.elements
                                                  if solver.element_kind(e) == "Resistor"}) as dev:
        theta, res = dev.thermal.solve((q * T.face_area(dev.xy, dev.tri))[None, :])
    err = np.abs(theta[0] - q / film).max() / (q / film)
    print("relative error", err, "iterations", res.iterations)
    assert err <= 1e-9


# ---- 4. balance on every board -------------------------------------------------------------------------------------------

def delivered_power(report) -> float:
    """What the sources deliver: minus what current sources, voltage sources and regulators absorb."""
    terms = []
    for element, flow in report.elements.items():
        if solver.element_kind(element) != "Resistor":
            terms += [-flow["power"], -flow.get("input_power", 0.0)]
    return math.fsum(terms)


@pytest.mark.parametrize("name", BOARDS)
def test_the_film_loss_is_the_power_the_sources_deliver(ctx, name):
    """total_loss equals the power the sources deliver (element_flows) within 1e-9 relative; with element_heat=False it
    equals the copper's power alone."""
    prob, meshes, layer_of, disc, *_ = board(name)
    _sol, currents = quiet(solver.solve_meshed_currents, prob, meshes, layer_of, disconnected_meshes_by_layer=disc)
    delivered, copper = delivered_power(currents), math.fsum(currents.layers)
    _s, rep = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model_of(FILM_STIFF), disconnected_meshes_by_layer=disc)
    _s, bare = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model_of(FILM_STIFF, element_heat=False),
                     disconnected_meshes_by_layer=disc)
    print(name, "delivered", delivered, "loss", rep.total_loss, "relative", abs(rep.total_loss - delivered) / delivered,
          "copper", copper, "loss without element heat", bare.total_loss, "relative", abs(bare.total_loss - copper) / copper)
    assert delivered > 0
    assert abs(rep.total_loss - delivered) <= 1e-9 * delivered
    assert abs(rep.total_heat - delivered) <= 1e-9 * delivered
    assert abs(bare.total_loss - copper) <= 1e-9 * copper
    assert all(e["heat"] == 0.0 for e in bare.elements.values())
    assert max(spot[0] for spot in rep.hotspots if spot is not None) > 25.0


# ---- 5. the face powers computed on the device --------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_layer", "two_in_layer", "problem_many_meshes"])
def test_solve_kkt_is_solve_fed_with_its_face_powers(ctx, name):
    """padne_thermal_solve_kkt gives the bits of padne_thermal_solve fed with the downloaded face powers; those are the
    restatement's on the block's own potentials, and per mesh they sum to current_cases' mesh_power within 1e-12 relative."""
    prob = board(name)[0]
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) == "CurrentSource"]
    cases = [{}] + [{e: 0.5 * (j + 1) * e.current for e in sources} for j in range(8)]       # 9 columns: chunks of 8 and 1
    with Device(name, FILM_STIFF, cases=cases) as dev:
        plan, V = dev.solved_block()
        k = len(cases)
        rng = np.random.default_rng(9)
        heat = (rng.integers(0, dev.n_pot, 12), rng.integers(0, k, 12), rng.uniform(0, 1e-3, 12))
        theta_kkt, _ = dev.thermal.solve_kkt(plan, k, heat)
        Pf = dev.thermal.face_power(k, dev.n_tri)
        theta, _ = dev.thermal.solve(Pf, heat)
        ml = np.asarray(dev.layer_of, dtype=np.int32)
        *_, mesh_power, _cuts = plan.current_cases(k, dev.n_tri, ml, [], np.zeros((0, 4)), fields=False, envelope=False)
        plan.close()
    assert np.array_equal(theta_kkt, theta)
    sigma = [prob.layers[l].conductance for l in dev.layer_of]
    assert np.array_equal(Pf, T.face_power(dev.xy, dev.tri, dev.face_mesh, sigma, V[:dev.n_vert]))
    for j in range(k):
        for m in range(len(dev.flat)):
            total = math.fsum(Pf[j, dev.toff[m]:dev.toff[m + 1]].tolist())
            assert abs(total - mesh_power[j, m]) <= 1e-12 * abs(total), (j, m)


# ---- 6. load cases and their envelope ------------------------------------------------------------------------------------

def vertex_temperatures(rep):
    return [zf.values for forms in rep.temperatures for zf in forms]


def scalars(rep):
    return rep.hotspots, rep.layers, [sorted(d.items()) for d in rep.elements.values()], rep.total_heat, rep.total_loss


@pytest.mark.parametrize("name", ["two_layer", "two_in_layer"])
def test_three_load_cases_one_of_them_dead(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]
    cases = [{}, {e: 1.7 * e.current for e in sources}, {e: 0.0 for e in sources}]
    model = model_of(FILM_STIFF, ambient=40.0)
    kw = dict(disconnected_meshes_by_layer=disc)
    sols, reps, env = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, cases=cases, **kw)
    assert len(sols) == len(reps) == 3
    for j, case in enumerate(cases):
        _s, one = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, cases=[case], **kw)[:2]
        for got, want in zip(vertex_temperatures(reps[j]), vertex_temperatures(one[0])):
            scale = max(np.abs(z - 40.0).max() for z in vertex_temperatures(one[0]))
            assert np.abs(got - want).max() <= BAR * scale
    # the dead case is exactly ambient
    assert all((z == 40.0).all() for z in vertex_temperatures(reps[2]))
    assert all((tf.values == 40.0).all() for forms in reps[2].face_temperatures for tf in forms)
    assert reps[2].total_heat == 0.0 and reps[2].total_loss == 0.0
    # the envelope is envelope_of on the per-case arrays, exactly
    per_case = [np.concatenate(vertex_temperatures(rep)) for rep in reps]
    best, which = solver.envelope_of(per_case)
    assert np.array_equal(np.concatenate([zf.values for forms in env.temperatures for zf in forms]), best)
    assert np.array_equal(np.concatenate([c for cs in env.cases for c in cs]), which)
    for layer_i, spot in enumerate(env.hotspots):
        if spot is not None:
            assert spot[1] == 1 and spot[0] == reps[1].hotspots[layer_i][0] and spot[2:] == reps[1].hotspots[layer_i][1:]
    # without the per-case fields: the same envelope, hotspots and sums
    sols2, reps2, env2 = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, cases=cases, per_case_fields=False, **kw)
    assert all(rep.temperatures is None and rep.face_temperatures is None for rep in reps2)
    assert [scalars(rep) for rep in reps2] == [scalars(rep) for rep in reps]
    assert env2.hotspots == env.hotspots
    for a, b in zip([zf.values for f in env2.temperatures for zf in f] + [c for cs in env2.cases for c in cs],
                    [zf.values for f in env.temperatures for zf in f] + [c for cs in env.cases for c in cs]):
        assert np.array_equal(a, b)


# ---- 7. the report -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["single", "two_in_layer", "problem_many_meshes"])
def test_the_report_against_the_restatement(ctx, name):
    """Face means bit for bit, the hotspot vertex with ties to the lowest, sums within 1e-12 relative, the envelope by the
    sequential rule -- all on the device's own theta.  Column 3 repeats column 0 (a tie between cases at every vertex) and
    column 2 is empty: theta = 0 exactly at every vertex, the complete tie, which must go to each mesh's first vertex."""
    with Device(name, FILM_STIFF) as dev:
        Pf, heat = random_loads(dev, 3, seed=11)
        Pf = np.concatenate([Pf, Pf[:1]])
        nodes, cols, vals = heat
        again = cols == 0
        heat = (np.concatenate([nodes, nodes[again]]), np.concatenate([cols, np.full(again.sum(), 3)]),
                np.concatenate([vals, vals[again]]))
        theta, _ = dev.thermal.solve(Pf, heat)
        mean, top, vert, heat_in, loss, env, env_case = dev.thermal.report(4, dev.n_tri, dev.n_vert)
        bare = dev.thermal.report(4, dev.n_tri, dev.n_vert, fields=False, envelope=False)
    _A, _M, hM = dev.restated()
    for j in range(4):
        mean_w, top_w, vert_w, heat_w, loss_w = T.report(dev.tri, dev.voff, dev.toff, hM, theta[j], Pf[j])
        assert np.array_equal(mean[j], mean_w)
        assert np.array_equal(top[j], top_w) and np.array_equal(vert[j], vert_w)
        assert (np.abs(heat_in[j] - heat_w) <= 1e-12 * np.abs(heat_w)).all()
        assert (np.abs(loss[j] - loss_w) <= 1e-12 * np.abs(loss_w)).all()
    assert np.array_equal(vert[2], dev.voff[:-1]) and (top[2] == 0.0).all()
    best, which = T.envelope(theta[:, :dev.n_vert])
    assert np.array_equal(env, best) and np.array_equal(env_case, which)
    assert bare[0] is None and bare[5] is None and bare[6] is None
    for a, b in zip(bare[1:5], (top, vert, heat_in, loss)):
        assert np.array_equal(a, b)


def test_hotspot_ties_go_to_the_lowest_vertex(ctx):
    """A symmetric board under a symmetric load: uniform heating of the unjittered grid, where every vertex has the same
    temperature up to rounding and mirror images may share their bits.  Whatever ties the device's theta holds, the
    hotspot is the first of its maxima; the second column is empty, the complete tie."""
    q = 3e-4
    with Device("symmetric", FILM_STIFF) as dev:
        Pf = np.stack([q * T.face_area(dev.xy, dev.tri), np.zeros(dev.n_tri)])
        theta, _ = dev.thermal.solve(Pf)
        _mean, top, vert, _heat, _loss, env, env_case = dev.thermal.report(2, dev.n_tri, dev.n_vert)
    tied = int((theta[0] == theta[0].max()).sum())
    print("vertices at the maximum of the uniformly heated symmetric board:", tied, "of", dev.n_vert)
    assert vert[0, 0] == int(np.flatnonzero(theta[0] == theta[0].max())[0]) and top[0, 0] == theta[0].max()
    assert vert[1, 0] == 0 and top[1, 0] == 0.0
    best, which = T.envelope(theta[:, :dev.n_vert])
    assert np.array_equal(env, best) and np.array_equal(env_case, which)


# ---- 8. two calls, the same bits -----------------------------------------------------------------------------------------

def everything(rep):
    return (vertex_temperatures(rep) + [tf.values for forms in rep.face_temperatures for tf in forms], scalars(rep))


@pytest.mark.parametrize("name", ["two_layer", "problem_many_meshes"])
def test_two_calls_give_the_same_bits(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    runs = [quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model_of(FILM_REAL), disconnected_meshes_by_layer=disc)[1]
            for _ in range(2)]
    (arrays_a, scalars_a), (arrays_b, scalars_b) = everything(runs[0]), everything(runs[1])
    assert scalars_a == scalars_b
    assert len(arrays_a) == len(arrays_b) and all(np.array_equal(a, b) for a, b in zip(arrays_a, arrays_b))


# ---- the entry points' refusals and the rest of the report -----------------------------------------------------------------

def test_refusals_of_the_device_entries(ctx):
    with Device("two_layer", FILM_STIFF) as dev:
        bad = dict(kappa=dev.kappa, film=dev.film)
        for key, value in (("kappa", [0.0, 1.0]), ("film", [1e-5, float("nan")]), ("film", [-1.0, 1e-5])):
            args = dict(bad, **{key: value})
            with pytest.raises(ValueError):
                _hip.Thermal(dev.L.dev, dev.n_pot, args["kappa"], args["film"])
        with pytest.raises(ValueError):
            _hip.Thermal(dev.L.dev, dev.n_pot, dev.kappa, dev.film, [0], [1], [-1.0])
        with pytest.raises(ValueError):
            _hip.Thermal(dev.L.dev, dev.n_pot, dev.kappa, dev.film, [0], [dev.n_pot], [1.0])
        with pytest.raises(ValueError):                    # the internal node has no link: its row has no diagonal
            _hip.Thermal(dev.L.dev, dev.n_pot, dev.kappa, dev.film)
        with pytest.raises(ValueError):                    # no solve yet
            dev.thermal.report(1, dev.n_tri, dev.n_vert)
        Pf = np.zeros((1, dev.n_tri))
        for heat in (([dev.n_pot], [0], [1.0]), ([0], [1], [1.0]), ([0], [0], [float("inf")])):
            with pytest.raises(ValueError):
                dev.thermal.solve(Pf, heat)
        other = finished_block(dev.board, dev.L, dev.cases + dev.cases)[0]
        try:
            with pytest.raises(ValueError):                # the finished block has two columns
                dev.thermal.solve_kkt(other, 1)
        finally:
            other.close()


def test_disconnected_meshes_report_ambient_and_elements_carry_heat(ctx):
    prob, meshes, layer_of, disc, *_ = board("two_layer")
    island = mesh.Mesh(np.array([[30.0, 0.0], [31.0, 0.0], [30.0, 1.0]]), np.array([[0, 1, 2]], dtype=np.int32))
    disc = [[island], []]
    _s, rep = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model_of(FILM_STIFF, ambient=30.0),
                    disconnected_meshes_by_layer=disc)
    assert [len(d) for d in rep.disconnected_temperatures] == [1, 0]
    assert (rep.disconnected_temperatures[0][0].values == 30.0).all()
    resistors = [e for n in prob.networks for e in n.elements if solver.element_kind(e) == "Resistor"]
    assert list(rep.elements) == resistors
    assert all(e["heat"] >= 0.0 for e in rep.elements.values()) and sum(e["heat"] for e in rep.elements.values()) > 0.0
    # heat flows through the vias from the hotter layer to the colder one: the flows are not all zero, and finite
    flows = np.array([e["flow"] for e in rep.elements.values()])
    assert np.isfinite(flows).all() and np.abs(flows).max() > 0.0
    assert rep.info["iterations"] > 0 and rep.info["rel_residual"] <= 1e-11

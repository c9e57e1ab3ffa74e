"""The kernels of thermal_sens.hip against their restatement (tests/tsens_kernel_ref.py, checked against the specification
by tests/test_tsens_kernel_ref_host.py) bit for bit, on the device's own inputs: the handles are driven directly -- block
solve of the cases, ``Thermal.solve_kkt``, ``ThermalSensitivities``, ``thermal_adjoints`` with every unknown as a probe,
``electrical_rhs`` downloaded from its device address, ``solve_block_dev`` and ``_finish_block``, then ``faces``,
``vertices``, ``pairs`` and ``sources`` -- and every output is compared with ``np.array_equal`` to the restatement
evaluated on the x, theta, lambda and mu the device itself produced.  tests/test_thermal_sensitivity.py holds the whole
call to the specification within 1e-8 of each class's largest bound; a face whose term is small against that, an objective
of a later register chunk that reads a neighbour's lambda, or a sum taken in another order than the header comment of
thermal_sens.hip promises pass there and fail here.

Boards (the smallest at which each piece can go wrong, those of tests/test_thermal_sensitivity.py):
  tiles      289 + 4 vertices, 512 + 2 faces: a full and a partial tile of both kinds and a mesh of one partial tile; five
             objectives over two cases, among them a point in the last face of the partial tile, the last vertex of the
             partial tile, and listed unknowns on both sides of the tile seam and in the small mesh
  two_layer  two load cases, an internal node with two resistors; 1, 4, 5 and 9 objectives: one, a full chunk, one over, and
             two chunks and one over of kTsensChunk = 4 (9 is also one over kThermalChunk = 8 of tsens_g_kernel), the cases
             mixed within every chunk; kinds 0 and 1, one objective on the internal node, one with an unknown listed twice
  stack      an interlayer pair and two heat sources, one of them a fallback list; 9 objectives of kinds 0, 1 and 2, the
             sources in both chunks of tsens_g_kernel

The resistors passed to ``electrical_rhs`` are the board's and six more among one of their terminals and three vertices, so
that four unknowns collect three entries or more on top of their faces' terms: two entries that start from 0.0 commute, and
the list order would not show (tests/test_tsens_kernel_ref_host.py::test_the_orders_matter).  Each test asserts that its own
list, reversed, moves bits of the restatement.

g stays in the device's scratch, so it is checked through the solve: |g_ref - A lambda_j|_2 / |g_ref|_2 with A downloaded,
against 10 times the larger of solver.RTOL and the same ratio of a forward ``Thermal.solve`` of ``random_loads`` on the same
handle (the device's residual is a recurrence, the host's is evaluated); figures in ``check_g_through_the_solve``.

That the tests bite was shown on four scratch copies of thermal_sens.hip (never committed) with the arithmetic changed and
no bound or launch touched, each built once and run once on an MI355X against this file, against
tests/test_many_tiles.py::test_temperature_sensitivities_of_nine_objectives (``wide``) and against
tests/test_thermal_sensitivity.py::test_every_output_against_the_specification (the 1e-8 comparison, 10 cases):

  the four waves of tsens_fold_kernel joined as ((0 + 1) + 2) + 3
      fails ``wide`` alone (a per-mesh sum of e_f); no mesh of this file has tiles in a third wave; the 1e-8 comparison passes
  lj[q] of tsens_rhs_kernel taken for j0 instead of j0 + q
      fails every test here with more than one objective and ``wide`` (the right-hand side of objective 1); two_layer with 1 objective passes;
      the 1e-8 comparison fails in all 10 cases
  the resistor loop of tsens_rhs_res_kernel run back to front
      fails all 6 tests here and ``wide`` (the right-hand side with the resistors, objective 0); the 1e-8 comparison passes
      in all 10 cases
  w31 and w23 exchanged in k_f
      fails all 6 tests here and ``wide`` (the thermal density) and the 1e-8 comparison in all 10 cases"""
import types

import numpy as np
import pytest
import scipy.sparse as sp

import sources_ref as SR
import stack_ref as K
import test_stack as TSK
import test_thermal as TT
import thermal_ref as T
import tsens_kernel_ref as TK
from padne_amd import _hip, solver
from test_stack_host import G
from test_thermal import FILM_STIFF, quiet, sorted_csr
from test_thermal_sensitivity import case_of

pytestmark = pytest.mark.gpu


# ---- objectives as the entry takes them: (case, kind, arg, xy, unknown, weight) ----------------------------------------------
def point(case, layer, q):
    return (case, 0, layer, tuple(q), (-1, -1, -1), (0.0, 0.0, 0.0))


def listed(case, unknowns, weights):
    pad = 3 - len(unknowns)
    return (case, 1, 0, (0.0, 0.0), tuple(unknowns) + (-1,) * pad, tuple(weights) + (0.0,) * pad)


def of_source(case, s):
    return (case, 2, s, (0.0, 0.0), (-1, -1, -1), (0.0, 0.0, 0.0))


def inside_face(xy, tri, f):
    return tuple((0.5 * xy[tri[f, 0]] + 0.3 * xy[tri[f, 1]] + 0.2 * xy[tri[f, 2]]).tolist())


def with_more(resistors, a, v0, v1, v2):
    """The board's resistors (a, b, R) and six more among the unknown ``a`` and three vertices: every one of the four collects
    three entries or more on top of its faces' terms, signs mixed."""
    a, v0, v1, v2 = int(a), int(v0), int(v1), int(v2)
    return list(resistors) + [(a, v0, 0.016), (v1, a, 0.032), (v0, v1, 0.02), (v1, v2, 0.05), (v2, v0, 0.04), (v2, a, 0.025)]


# ---- the calls ------------------------------------------------------------------------------------------------------------------
def drive(ctx, thermal, plan, L, k, kappa, layer_of, n_tri, objectives, resistors):
    """Steps 3 to 7 of the sequence on a plan whose finished block holds the k cases and a thermal handle solved for them.
    Every read-out is taken twice; the right-hand side with the resistors, with none, and with the resistors again."""
    n_obj, n_pot, N, n_mesh = len(objectives), thermal.n_potential, L.shape[0], thermal.n_mesh
    case, kind, arg, xy, unknown, weight = (list(col) for col in zip(*objectives))
    a, b, R = ([r[i] for r in resistors] for i in range(3))
    out = types.SimpleNamespace(n_obj=n_obj)
    ts = _hip.ThermalSensitivities(thermal, plan, k, kappa)
    try:
        out.unknown, out.weight, out.lam, lres = quiet(ts.thermal_adjoints, case, kind, arg, np.array(xy), np.array(unknown),
                                                       np.array(weight), layer_of, probes=np.arange(n_pot), rtol=solver.RTOL)
        assert lres.status == _hip.OK and out.lam.shape == (n_obj, n_pot)
        first = ctx.download(ts.electrical_rhs(a, b, R), (N, n_obj))
        out.rhs_none = ctx.download(ts.electrical_rhs(), (N, n_obj))
        addr = ts.electrical_rhs(a, b, R)
        out.rhs = ctx.download(addr, (N, n_obj))
        assert np.array_equal(first, out.rhs)                                       # two calls, the same bits
        none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float64))
        red, kidx, kval = solver.block_plan_inputs(L, *none, n_obj)
        probes, ares = quiet(plan.solve_block_dev, n_obj, addr, kidx, kval, red.regulator_columns, red.probe_members,
                             rtol=solver.RTOL, abs_residual_target=solver.ABS_RESIDUAL_TARGET)
        out.mu, _norms = solver._finish_block(plan, red, red.probe_members, probes, n_obj)
        out.faces = [ts.faces(n_tri, n_mesh) for _ in range(2)]
        out.film = [ts.vertices(n_mesh) for _ in range(2)]
        out.pairs = [ts.pairs() for _ in range(2)]
        out.sources = [ts.sources() for _ in range(2)]
    finally:
        ts.close()
    assert all(np.array_equal(p, q) for p, q in zip(*out.faces))                   # two calls, the same bits
    for twice in (out.film, out.pairs, out.sources):
        assert np.array_equal(*twice)
    return out


def restated_board(flat, layer_of, sigma, kappa, hM, n_pot, N, pairs=(), G_csr=None, sources=None):
    """What the restatement reads of a board: thermal_ref.flatten's arrays, the sampler's Board for the owners, and of a
    stacked handle with sources the device's own G and sources_ref's lists."""
    xy, tri, face_mesh, voff, toff = T.flatten(flat)
    return types.SimpleNamespace(xy=xy, tri=tri, face_mesh=face_mesh, voff=voff, toff=toff, sigma=list(sigma), kappa=list(kappa),
                                 hM=np.asarray(hM), n_pot=int(n_pot), N=int(N), layer_of=list(layer_of), n_mesh=len(flat),
                                 sboard=K.board_of(flat, layer_of), pairs=list(pairs), G=G_csr, sources=sources)


def restated_g(B, objective, unknown, weight):
    case, kind, arg, *_ = objective
    return TK.g_vector(B.n_pot, kind, unknown, weight, B.sources, arg)


def check(B, objectives, resistors, x, theta, out, what=""):
    """Every output of ``drive`` against the restatement on the device's x, theta (k, n_pot), lambda and mu, bit for bit.
    Returns the restated terms per objective -- (ef, kf, film terms, [pair terms per pair]) -- for further checks."""
    ed, kd, cd, mesh_e, mesh_k = out.faces[0]
    film, pairs, sources = out.film[0], out.pairs[0], out.sources[0]
    assert pairs.shape == (out.n_obj, len(B.pairs)) and sources.shape == (out.n_obj, 0 if B.sources is None else len(B.sources.A))
    terms = []
    for j, obj in enumerate(objectives):
        c, kind, arg, q, unknown, weight = obj
        at = f"{what} objective {j}"
        if kind == 0:
            want_u, want_w = TK.owner(B.sboard, arg, q)
            assert want_u[0] >= 0, at
            assert np.array_equal(out.unknown[j], want_u) and np.array_equal(out.weight[j], want_w), at
        else:
            assert np.array_equal(out.unknown[j], unknown) and np.array_equal(out.weight[j], weight), at
        lam, mu = out.lam[j], out.mu[:, j]
        args = (B.N, B.n_pot, B.xy, B.tri, B.face_mesh, B.sigma, lam, x[c])
        assert np.array_equal(out.rhs[:, j], TK.rhs(*args, resistors)), at
        assert np.array_equal(out.rhs_none[:, j], TK.rhs(*args, ())), at
        e_w, k_w, c_w, ef, kf = TK.faces(B.xy, B.tri, B.face_mesh, B.sigma, B.kappa, lam, theta[c], x[c], mu)
        assert np.array_equal(ed[j], e_w), at
        assert np.array_equal(kd[j], k_w), at
        assert np.array_equal(cd[j], c_w), at
        assert np.array_equal(mesh_e[j], TK.mesh_sums(B.toff, ef)), at
        assert np.array_equal(mesh_k[j], TK.mesh_sums(B.toff, kf)), at
        ft = TK.film_terms(B.hM, lam, theta[c])
        assert np.array_equal(film[j], TK.mesh_sums(B.voff, ft)), at
        per = []
        if B.pairs:
            want, per = TK.pair_values(B.voff, B.layer_of, B.G, B.pairs, lam, theta[c])
            assert np.array_equal(pairs[j], want), at
        if B.sources is not None:
            assert np.array_equal(sources[j], TK.sources(B.sources, lam)), at
        terms.append((ef, kf, ft, per))
    return terms


def orders_show(B, objectives, resistors, x, out):
    """The passed resistor list, reversed, moves bits of the restated right-hand side of some objective: the comparison can
    tell the order (for one column alone the roundings may happen to agree)."""
    for j, obj in enumerate(objectives):
        args = (B.N, B.n_pot, B.xy, B.tri, B.face_mesh, B.sigma, out.lam[j], x[obj[0]])
        if not np.array_equal(TK.rhs(*args, resistors), TK.rhs(*args, resistors[::-1])):
            return True
    return False


def check_g_through_the_solve(B, dev, objectives, out, watts=None):
    """g is checked through the solve that consumed it: |g_ref - A lambda_j|_2 / |g_ref|_2 on the host with the downloaded A
    (A' of a stacked handle), against 10 times the larger of solver.RTOL and the same ratio of a forward solve of
    ``random_loads`` (3 columns, the last empty) on the same handle at solver.RTOL.  Measured on an MI355X, adjoint and forward:
    1.3e-15 and 8.4e-16 at worst over the boards of this file (their systems are small enough for the coarsest level's
    inverse), 8.7e-13 and 8.3e-13 on the board of tests/test_many_tiles.py; granted 1e-11 in every case."""
    A = sorted_csr(dev.thermal.matrix().to_scipy())
    Pf, heat = TT.random_loads(dev, 3, seed=5)
    if watts is not None:
        dev.thermal.source_power(watts)
    b = dev.thermal.load(Pf, heat)
    th, res = quiet(dev.thermal.solve, Pf, heat, rtol=solver.RTOL)
    assert res.status == _hip.OK
    forward = max(np.linalg.norm(b[c] - A @ th[c]) / np.linalg.norm(b[c]) for c in range(2))
    grant = 10 * max(forward, solver.RTOL)
    worst = 0.0
    for j, obj in enumerate(objectives):
        g = restated_g(B, obj, out.unknown[j], out.weight[j])
        assert np.linalg.norm(g) > 0
        ratio = np.linalg.norm(g - A @ out.lam[j]) / np.linalg.norm(g)
        worst = max(worst, ratio)
        assert ratio <= grant, (j, ratio, grant)
    print("adjoint residual |g - A lambda| / |g|, worst:", worst, "forward:", forward, "granted:", grant)
    return worst, forward


def sigma_of(dev):
    return [float(dev.prob.layers[l].conductance) for l in dev.layer_of]


def hM_of(dev):
    return np.repeat(np.asarray(dev.film, dtype=np.float64), np.diff(dev.voff)) * dev.thermal.lumped(dev.n_vert)


def board_resistors(dev):
    return [(int(row[1]), int(row[2]), float(row[3])) for _, row in dev.pairs if row[0] == "R"]


def run_device(ctx, dev, objectives, resistors, pairs=(), G_csr=None, sources=None, watts=None):
    """The whole sequence on an entered Device; returns (B, x, theta, out)."""
    k = len(dev.cases)
    plan, V = quiet(dev.solved_block)
    try:
        x = np.ascontiguousarray(V[:dev.n_pot].T)
        theta, tres = quiet(dev.thermal.solve_kkt, plan, k, rtol=solver.RTOL)
        assert tres.status == _hip.OK
        B = restated_board(dev.flat, dev.layer_of, sigma_of(dev), dev.kappa, hM_of(dev), dev.n_pot, dev.L.shape[0], pairs, G_csr,
                           sources)
        out = drive(ctx, dev.thermal, plan, dev.L, k, dev.kappa, dev.layer_of, dev.n_tri, objectives, resistors)
    finally:
        plan.close()
    assert np.abs(x).max() > 0 and np.abs(theta).max() > 0
    check(B, objectives, resistors, x, theta, out)
    assert orders_show(B, objectives, resistors, x, out)
    check_g_through_the_solve(B, dev, objectives, out, watts)
    return B, x, theta, out


# ---- the boards -----------------------------------------------------------------------------------------------------------------
def test_tiles_a_full_and_a_partial_tile_and_a_mesh_of_one_partial_tile(ctx):
    prob = TT.board("two_in_layer")[0]
    with TT.Device("two_in_layer", FILM_STIFF, cases=({}, case_of(prob, 0.5))) as dev:
        assert np.diff(dev.voff).tolist() == [289, 4] and np.diff(dev.toff).tolist() == [512, 2]
        objectives = [point(0, 0, (3.3, 4.6)), point(1, 0, (20.6, 20.3)), point(0, 0, inside_face(dev.xy, dev.tri, 511)),
                      listed(1, [288], [1.0]), listed(0, [255, 256, 289], [0.2, 0.3, 0.5])]
        own = board_resistors(dev)
        resistors = with_more(own, own[0][0], 255, 256, 100)
        _B, _x, _theta, out = run_device(ctx, dev, objectives, resistors)
    assert np.array_equal(out.unknown[2], dev.tri[511])                 # the last live lane of the partial face tile
    assert out.unknown[1].min() >= 289                                  # the mesh of one partial tile
    assert out.pairs[0].shape == (5, 0) and out.sources[0].shape == (5, 0)


def two_layer_objectives(dev):
    points = [(1.3, 1.2), (6.6, 6.9), (4.1, 3.3), (2.2, 6.1), (7.3, 1.4)]
    objectives = [point(j % 2, j % 2, q) for j, q in enumerate(points)]
    objectives += [listed(1, [dev.n_pot - 1], [1.0]),                   # the internal node
                   listed(0, [288, 289], [0.5, 0.5]),                   # the last vertex of one mesh, the first of the next
                   listed(1, [40, 40, 300], [0.25, 0.5, 0.25]),         # an unknown listed twice: added in k order
                   point(1, 0, (5.5, 5.5))]
    return objectives


@pytest.mark.parametrize("n_obj", [1, 4, 5, 9])
def test_two_layer_register_chunks_mixed_cases_and_resistors_in_list_order(ctx, n_obj):
    prob = TT.board("two_layer")[0]
    with TT.Device("two_layer", FILM_STIFF, cases=({}, case_of(prob, 0.5))) as dev:
        objectives = two_layer_objectives(dev)[:n_obj]
        own = board_resistors(dev)
        mid = dev.n_vert
        assert dev.n_internal == 1 and sum(1 for a, b, _ in own if mid in (a, b)) == 2
        resistors = with_more(own, mid, own[2][0], own[3][0], own[4][1])      # five on it, more on three vias' vertices
        _B, x, _theta, out = run_device(ctx, dev, objectives, resistors)
    if n_obj >= 4:
        assert {o[0] for o in objectives[:4]} == {0, 1}                 # the cases are mixed within the first chunk
        assert not np.array_equal(x[0], x[1])
    # no two objectives share a lambda: a chunk that read its neighbour's would show
    assert len({out.lam[j].tobytes() for j in range(n_obj)}) == n_obj


def test_stack_a_pair_two_heat_sources_and_every_kind(ctx):
    polygons = [np.array([(6.0, 4.0), (11.0, 4.0), (11.0, 9.0), (6.0, 9.0)]),
                np.array([(4.1, 11.1), (4.2, 11.1), (4.2, 11.2), (4.1, 11.2)])]
    with TSK.Stacked("pair", FILM_STIFF, pairs=[(0, 1, G)]) as dev:
        counts, fallback, _area = dev.thermal.set_sources(2, dev.layer_of, [0, 1], polygons)
        assert list(fallback) == [0, 1] and counts[0] > 1 and counts[1] == 1
        dev.thermal.source_power(np.array([[0.03, 0.01]]))
        indptr, indices, data, _diag = dev.thermal.stack_matrix()
        G_csr = sp.csr_matrix((data, indices.astype(np.int64), indptr.astype(np.int64)), shape=(dev.n_pot, dev.n_pot))
        sources = SR.Restated(dev.flat, dev.layer_of, [(0, polygons[0]), (1, polygons[1])])
        objectives = [of_source(0, 0), of_source(0, 1), point(0, 1, (9.3, 5.2)), listed(0, [100], [1.0]), point(0, 0, (3.7, 12.2)),
                      of_source(0, 1), listed(0, [288, 289, 457], [0.3, 0.3, 0.4]), point(0, 1, (12.4, 2.6)), of_source(0, 0)]
        own = board_resistors(dev)
        resistors = with_more(own, own[0][0], 17, 300, 150)
        watts = np.array([[0.02, 0.01], [0.0, 0.03], [0.0, 0.0]])
        B, _x, _theta, out = run_device(ctx, dev, objectives, resistors, pairs=[(0, 1, G)], G_csr=G_csr, sources=sources, watts=watts)
    assert dev.n_pot == 289 + 169 and out.pairs[0].shape == (9, 1) and out.sources[0].shape == (9, 2)
    assert (out.pairs[0] != 0.0).all() and (out.sources[0] > 0.0).all()

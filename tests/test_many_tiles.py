"""Every kernel that folds in the fixed order of error.hpp (tests/fold_ref.py states it in numpy) on one board whose meshes
have many tiles, so that the strided loop of a fold takes a second and a third step, all four waves of a fold hold tiles, and
the list of a heat source wraps its slot ``tile & 255``.  Every comparison is made on the device's own solution.

The board (jittered synthetic.jittered_grid meshes, chosen for their tile counts; h = 0.125):

  mesh  layer  grid                         vertices (tiles)      faces (tiles)            what it reaches
  A     0      257 x 258                    66 306 (260, ragged)  131 584 (514, full)      strided loop taken 2-3 times, all four waves
  B     0      2 x 2                        4 (1)                 2 (1)                    one lane
  C     0      92 x 92                      8 464 (34)            16 562 (65)              first lane of wave 1
  D     1      129 x 130, spacing 2 h,      16 770 (66)           33 024 (129)             lane 0 of wave 2 (faces), wave 1 (vertices)
               over A

A source drives A against D through a lattice of vias, a second one drives C against A and returns through B: every mesh
carries current in case 0.  Three load cases, the last one dead.  One block solve, shared by the tests.

Folds added after the first ones, and what each reaches on this board:

  fold                                     test                                          strides and waves
  tsens_fold_kernel, faces (e_f, k_f)      test_temperature_sensitivities_of_nine_...    A: 514 tiles, lanes 0-1 take 3 strides, the rest
                                                                                         2, all four waves; D: 129, waves 0-2; C: 65,
                                                                                         wave 0 and lane 0 of wave 1; B: one lane
  tsens_fold_kernel, vertices (film,       the same                                      A: 260 tiles, lanes 0-3 take 2 strides, all four
  pairs)                                                                                 waves; D: 66 and C: 34, wave 0 (and 1); B: one lane
  tsens_owner_kernel                       the same                                      A's 131 584 faces in 514 strides, the owner in the
                                                                                         last; D, B and tile 300 of A
  sdirk_fold_kernel (err and its vertex)   test_one_adaptive_trial_step_of_four_...      A: the winner in tile 259 (lane 3, second stride),
                                                                                         257 (lane 1, second stride), 200 (wave 3, first)
  coupled_transient_heat_fold_kernel       test_electrothermal_transient_load_and_...    per mesh as the faces above: A 514 tiles
  coupled_transient_range_fold_kernel      the same                                      all 708 face tiles by one workgroup: 3 strides, the
                                                                                         smallest in the last tile, the largest in tile 300
  film_terms_kernel's count and            test_film_terms_and_the_count_above_the_...   the tiles of all meshes as one list, A 0-259, B 260,
  film_fold_kernel's sum of it                                                           C 261-294, D 295-360: 361 tiles, lanes 0-104 take 2
                                                                                         strides, all four waves; a count of 2 from tiles 256
                                                                                         and 360 alone (lanes 0 and 104, second stride)
  film_fold_kernel (increment, its         test_film_increment_its_vertex_the_count_...  the winner in tile 200 (wave 3, first stride), 259
  vertex, the count), hM of the pass                                                     (lane 3, second), 300 (lane 44, second), 360 (lane 104,
                                                                                         second, a ragged tile); the complete tie of 361 tiles
  coupled_resistor_scale_kernel +          test_resistor_scale_means_and_increment_...   66 006 resistors of the long strips (below): 258
  coupled_fold_kernel on its tiles                                                       tiles, lanes 0-1 take 2 strides, all four waves; the
                                                                                         winner in tile 257, 256 (second stride), 200 (wave 3)
  the lowest invalid resistor              test_the_lowest_invalid_resistor_across_...   tiles 100 and 257 of the 258; tile 257 alone
  coupled_resistor_places_kernel,          test_resistor_revalue_on_516_tiles_of_rows    132 010 incidences and 132 001 touched rows: 516
  coupled_resistor_revalue_kernel                                                        workgroups each (no fold: rows beyond a few tiles)

The resistors' tests run on resistor_coupling_ref.strips_system(66 000), two strips of 66 000 vertices joined vertex to vertex,
not on the board above, whose elements are a handful.  sample_fields_fold_kernel's three strides are held in
tests/test_temperature_sampling.py (a raster of 516 tiles).

Where the summed term is a device output, or one IEEE operation on device outputs, the per-mesh sum is compared bit for bit
with fold_ref.  Elsewhere it is compared with math.fsum of the restatement's per-item terms within fold_ref.fold_bound plus
the tolerance the entry's own test grants per item, summed over the items.  Tops and their indices are exact everywhere."""
import contextlib
import math
import types

import numpy as np
import pytest
import scipy.sparse as sp

import coupled_ref as CR
import currents_ref as C
import film_ref as FR
import fold_ref as F
import goal_ref as GR
import helpers as H
import resistor_coupling_ref as RC
import sdirk_ref as SD
import sensitivity_ref as S
import sources_ref as SR
import stack_ref as K
import test_film as TF
import test_thermal_sensitivity_kernels as KT
import thermal_ref as T
import transient_ref as R
from padne_amd import _hip, mesh, problem as P, solver, synthetic
from test_load_case_currents import finished_block, plan_cuts
from test_resistor_coupling import AMBIENT, T0, coefficients, opened
from test_stack_host import G
from test_thermal import FILM_STIFF, links_of, per_mesh, quiet, sorted_csr

pytestmark = pytest.mark.gpu

TOL = 1e-12                  # tests/test_currents.py's, tests/test_error.py's and tests/test_goal_error.py's, per item
REL_TOL = 1e-8               # tests/test_sensitivity.py's, per item
U = 2.0 ** -53
HA = 0.125
#            layer, nx, ny, h, origin, seed
GRIDS = {"A": (0, 257, 258, HA, (0.0, 0.0), 1), "B": (0, 2, 2, 1.0, (40.0, 0.0), 2), "C": (0, 92, 92, HA, (40.0, 5.0), 3),
         "D": (1, 129, 130, 2 * HA, (0.0, 0.0), 4)}
#            vertices, their tiles, faces, their tiles
COUNTS = {"A": (66_306, 260, 131_584, 514), "B": (4, 1, 2, 1), "C": (8_464, 34, 16_562, 65), "D": (16_770, 66, 33_024, 129)}
NEG_INF = (-np.inf, F.NO_INDEX)


def tiles(n) -> int:
    return -(-int(n) // 256)


def fsum(a) -> float:
    return math.fsum(np.asarray(a, dtype=np.float64).reshape(-1).tolist())


class Wide:
    """The board, its restatement's arrays and, inside the fixture, the assembled system with the finished block."""

    def __init__(self):
        self.meshes, self.layer_of = [], []
        for name, (layer, nx, ny, h, origin, seed) in GRIDS.items():
            xy, tri = synthetic.jittered_grid(nx, ny, h=h, seed=seed, jitter=0.2, origin=origin)
            m = mesh.Mesh(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3))
            got = (len(m.points), tiles(len(m.points)), len(m.triangles), tiles(len(m.triangles)))
            assert got == COUNTS[name], (name, got)
            self.meshes.append(m)
            self.layer_of.append(layer)
        assert COUNTS["A"][0] % 256 != 0 and COUNTS["A"][2] % 256 == 0 and COUNTS["A"][1] > 256 and COUNTS["A"][3] > 2 * 256
        top = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=2000.0)
        bottom = P.Layer(shape=H.Geoms(1), name="B.Cu", conductance=1000.0)
        at = lambda layer, x, y: P.Connection(layer=layer, point=H.XY(x, y))      # noqa: E731
        c = [at(top, 4, 4), at(bottom, 28, 28), at(top, 50, 15), at(top, 20, 4), at(top, 30, 20), at(top, 40, 0), at(top, 41, 1),
             at(top, 41, 6)]
        self.sources = [P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0),
                        P.CurrentSource(f=c[2].node_id, t=c[3].node_id, current=0.5)]
        elements = self.sources + [P.Resistor(a=c[4].node_id, b=c[5].node_id, resistance=0.01),       # A - B
                                   P.Resistor(a=c[6].node_id, b=c[7].node_id, resistance=0.01)]       # B - C
        for x in (6, 12, 18, 24):                            # the via lattice between A and D
            for y in (8, 16, 24):
                a, b = at(top, x, y), at(bottom, x, y)
                c += [a, b]
                elements.append(P.Resistor(a=a.node_id, b=b.node_id, resistance=0.002))
        self.prob = P.Problem(layers=[top, bottom], networks=[P.Network(connections=c, elements=elements)])
        self.cases = [{}, {self.sources[0]: 3.4, self.sources[1]: -0.3}, {e: 0.0 for e in self.sources}]
        self.board = solver.index_board(self.prob, self.meshes, self.layer_of)
        nodes = self.board.node_indexer
        self.pairs = solver.global_elements(list(self.prob.networks), nodes)
        self.n_internal = nodes.internal_node_count
        sigma = [self.prob.layers[l].conductance for l in self.layer_of]
        self.system = S.System(meshes=[(m.points, m.triangles, s) for m, s in zip(self.meshes, sigma)], n_internal=self.n_internal,
                               rows=[row for _, row in self.pairs], ground=solver.find_best_ground_node_index(self.prob, nodes),
                               layer_of=self.layer_of, prob=self.prob, pairs=self.pairs, nodes=nodes, flat=elements)
        self.flat = [(np.asarray(m.points, dtype=np.float64), np.asarray(m.triangles, dtype=np.int64)) for m in self.meshes]
        self.xy, self.tri, self.face_mesh, self.voff, self.toff = T.flatten(self.flat)
        self.sigma = np.asarray(sigma, dtype=np.float64)
        self.n_vert, self.n_tri, self.n_mesh = len(self.xy), len(self.tri), len(self.meshes)
        self.n_pot = self.n_vert + self.n_internal
        self.ml = np.asarray(self.layer_of, dtype=np.int32)
        checked = solver.check_thermal_model(self.prob, solver.ThermalModel(film=FILM_STIFF))
        self.kappa, self.film = per_mesh(checked, self.layer_of)
        self.links = links_of(self.pairs, checked)
        self.M = T.lumped(self.xy, self.tri)
        self.hM = np.repeat(np.asarray(self.film, dtype=np.float64), np.diff(self.voff)) * self.M
        self.face_area = T.face_area(self.xy, self.tri)

    def faces(self, m):
        return int(self.toff[m]), int(self.toff[m + 1])

    def verts(self, m):
        return int(self.voff[m]), int(self.voff[m + 1])

    def thermal(self, **kw):
        return _hip.Thermal(self.L.dev, self.n_pot, self.kappa, self.film, [l[0] for l in self.links], [l[1] for l in self.links],
                            [l[2] for l in self.links], **kw)

    def sum_check(self, got, terms, per_item, n_tiles, what):
        """``got`` against math.fsum of ``terms`` within fold_bound plus ``per_item`` summed; the figures are printed."""
        want, size, grant = fsum(terms), fsum(np.abs(terms)), fsum(per_item)
        bound = F.fold_bound(n_tiles, size)
        print(what, "sum", want, "error", abs(got - want), "fold bound", bound, "per-item grant", grant)
        assert abs(got - want) <= bound + grant, what


@pytest.fixture(scope="module")
def wide(ctx):
    w = Wide()
    assert 91_000 < w.n_pot < 92_000
    with w.board.assembled() as (L, _r):
        w.L = L
        w.plan, w.V = quiet(finished_block, w.board, L, solver.check_load_cases(w.prob, w.cases))
        try:
            yield w
        finally:
            w.plan.close()


def test_the_board_has_the_tile_counts_of_the_table(wide):
    for m, name in enumerate(GRIDS):
        assert (wide.voff[m + 1] - wide.voff[m], tiles(wide.voff[m + 1] - wide.voff[m]), wide.toff[m + 1] - wide.toff[m],
                tiles(wide.toff[m + 1] - wide.toff[m])) == COUNTS[name]
    assert wide.V.shape[1] == 3 and (wide.V[:, 2] == 0.0).all()                   # the dead case
    assert wide.n_internal == 0


# ---- currents and load-case currents -----------------------------------------------------------------------------------------

def cuts_of(w):
    """Down the whole height of A (a line no vertex lies on), and a line between A and the meshes B and C."""
    top = w.prob.layers[0]
    return [solver.Cut(top, (15.97, -1.0), (15.97, 34.0)), solver.Cut(top, (36.0, -1.0), (36.0, 34.0))]


def test_currents_of_three_cases(wide):
    """Per case and mesh: the hotspot is the fold of the device's own |J|, exactly; the power against math.fsum of the
    restated face powers (TOL per face, as tests/test_currents.py grants a layer's sum) and, since those are the bits
    thermal_face_power_kernel writes from the same expression (tests/test_thermal.py), bit for bit against fold_ref.  The long
    cut against math.fsum of the cut rule's terms (TOL of each, as tests/test_currents.py grants a cut); its fold runs over
    (cut, tile) pairs, at most the tiles of the layer.  The dead case: zeros, and every hotspot at its mesh's first face."""
    w = wide
    cl, cxy = plan_cuts(w.system, cuts_of(w))
    first = w.plan.current_cases(3, w.n_tri, w.ml, cl, cxy)
    second = w.plan.current_cases(3, w.n_tri, w.ml, cl, cxy)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))              # two calls, the same bits
    J, mag, env, env_case, mmax, mface, mpow, cut = first
    one = w.plan.current_report(3, w.n_tri, w.ml, cl, cxy)
    assert np.array_equal(one[2], mmax[0]) and np.array_equal(one[3], mface[0]) and np.array_equal(one[4], cut[0])
    assert (mmax[0] > 0).all() and (mpow[0] > 0).all()                            # every mesh carries current in case 0
    # the tiles the long cut crosses: more than one stride of its fold
    lo, hi = w.faces(0)
    x = w.xy[w.tri[lo:hi], 0]
    crossed = np.unique(np.flatnonzero((x.min(axis=1) < 15.97) & (x.max(axis=1) > 15.97)) // 256)
    print("tiles of A the long cut crosses:", len(crossed))
    assert len(crossed) > 256
    layer_tiles = sum(tiles(w.toff[m + 1] - w.toff[m]) for m in range(w.n_mesh) if w.layer_of[m] == 0)
    for j in range(3):
        xj = w.V[:, j]
        power = T.face_power(w.xy, w.tri, w.face_mesh, w.sigma, xj[:w.n_vert])
        for m in range(w.n_mesh):
            lo, hi = w.faces(m)
            assert (mmax[j, m], mface[j, m]) == F.mesh_top(mag[j, lo:hi], np.arange(lo, hi)), (j, m)
            w.sum_check(mpow[j, m], power[lo:hi], TOL * power[lo:hi], tiles(hi - lo), f"power, case {j}, mesh {m}")
            assert mpow[j, m] == F.mesh_sum(power[lo:hi]), (j, m)
        terms = C.cut_terms(w.system, xj, 0, cxy[0, :2], cxy[0, 2:])
        w.sum_check(cut[j, 0], terms, TOL * np.abs(terms), layer_tiles, f"long cut, case {j}")
        assert len(C.cut_terms(w.system, xj, 0, cxy[1, :2], cxy[1, 2:])) == 0 and cut[j, 1] == 0.0
    assert abs(cut[0, 0]) > 0 and len(terms) > 2 * 257
    assert np.array_equal(mface[2], w.toff[:-1]) and (mmax[2] == 0.0).all() and (mpow[2] == 0.0).all() and (cut[2] == 0.0).all()
    want_env, want_case = solver.envelope_of(mag)
    assert np.array_equal(env, want_env) and np.array_equal(env_case, want_case)
    assert (env_case == 1).any() and (env_case == 0).any()


# ---- sensitivities -----------------------------------------------------------------------------------------------------------

def test_sensitivity_totals_of_two_objectives(wide):
    """Adjoint j is column j of the block (W = e_j: the other columns enter as 0 x, exactly).  Objective 0 is the power,
    objective 1 a signed sum.  The totals against the restatement's s_f with what tests/test_sensitivity.py grants a density
    (REL_TOL of the largest, times the face's area); and against the device's own densities, whose products with the area
    are the summed s_f up to the two roundings of s_f / area * area."""
    w = wide
    _power, density, totals = w.plan.sensitivity_block(np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), w.n_tri, w.n_mesh)
    *_, area = S.faces(w.system)
    x = w.V[:, 0]
    for j in range(2):
        lam = w.V[:, j]
        sf, size = S.face_s(w.system, x, lam), S.face_s_bound(w.system, x, lam)
        grant = REL_TOL * max(np.abs(sf / area).max(), (size / area).max()) * area
        own = density[j] * w.face_area
        for m in range(w.n_mesh):
            lo, hi = w.faces(m)
            w.sum_check(totals[j, m], sf[lo:hi], grant[lo:hi], tiles(hi - lo), f"sensitivity, objective {j}, mesh {m}")
            w.sum_check(totals[j, m], own[lo:hi], 3 * U * np.abs(own[lo:hi]), tiles(hi - lo), f"the same from the densities, {j}, {m}")
    assert (totals[0] > 0).all() and (density[1] < 0).any() and (density[1] > 0).any()


# ---- error estimate and goal error ---------------------------------------------------------------------------------------------

def test_error_estimate_and_goal_error_of_one_objective(wide):
    """Field 0 is column 0 and the adjoint column 1 (W = e_1).  Per mesh against math.fsum of the restatement's terms with
    what tests/test_goal_error.py grants them: E to TOL of the squared scale of every eta_f (and the three roundings between
    eta_f^2, its root and its square), P to TOL of itself, omega and delta to TOL of the pair's scale.  omega_f and delta_f
    come home, so their sums are also held to fold_ref bit for bit.  The tops are the folds of the device's own eta and omega."""
    w = wide
    G_, eta, mesh_E, mesh_P, mesh_max, mesh_face = w.plan.error_estimate(3, w.n_tri, w.n_vert, w.n_mesh)
    _p, field0, dual, delta, omega, m_omega, m_delta, m_top, m_face = w.plan.goal_error(np.array([[0.0, 1.0, 0.0]]), w.n_tri, w.n_vert,
                                                                                     w.n_mesh)
    for a, b in zip(field0, (G_, eta, mesh_E, mesh_P, mesh_max, mesh_face)):
        assert np.array_equal(a, b)                          # goal.hip's fold of field 0 is error.hip's, bit for bit
    want = GR.goal_flat(w.xy, w.tri, w.face_mesh, w.sigma, np.stack([w.V[:w.n_vert, 0], w.V[:w.n_vert, 1]]))
    est = want.primal
    s0 = est.eta_scale(w.tri)
    pair = want.pair_scale(w.tri, 0)
    eta2 = est.eta * est.eta                                 # eta_f^2 of the restatement, up to the roundings of sqrt and square
    power = est.sigma * est.area * (est.g ** 2).sum(axis=1)
    for m in range(w.n_mesh):
        lo, hi = w.faces(m)
        n, idx = tiles(hi - lo), np.arange(lo, hi)
        w.sum_check(mesh_E[m], eta2[lo:hi], TOL * s0[lo:hi] ** 2 + 3 * U * eta2[lo:hi], n, f"E, mesh {m}")
        w.sum_check(mesh_P[m], power[lo:hi], TOL * power[lo:hi], n, f"P, mesh {m}")
        assert (mesh_max[m], mesh_face[m]) == F.mesh_top(eta[lo:hi], idx), m
        w.sum_check(m_omega[0, m], want.omega[0, lo:hi], TOL * pair[lo:hi], n, f"omega, mesh {m}")
        w.sum_check(m_delta[0, m], want.delta[0, lo:hi], TOL * pair[lo:hi], n, f"delta, mesh {m}")
        assert m_omega[0, m] == F.mesh_sum(omega[0, lo:hi]) and m_delta[0, m] == F.mesh_sum(delta[0, lo:hi]), m
        assert (m_top[0, m], m_face[0, m]) == F.mesh_top(omega[0, lo:hi], idx), m
    assert (mesh_E > 0).all() and (delta[0] < 0).any() and (delta[0] > 0).any()


# ---- the thermal report, the interlayer flows and the heat sources ------------------------------------------------------------

def footprints(w):
    """All of A (B and C lie beyond x = 40); a disc on A; a speck inside a face of A's last tile, off its centroid."""
    angle = 2 * np.pi * np.arange(64) / 64
    disc = np.stack([16.0 + 8.5 * np.cos(angle), 16.0 + 8.5 * np.sin(angle)], axis=1)
    f = w.faces(0)[0] + 513 * 256 + 100
    p = 0.5 * w.xy[w.tri[f, 0]] + 0.3 * w.xy[w.tri[f, 1]] + 0.2 * w.xy[w.tri[f, 2]]
    return [np.array([(-1.0, -1.0), (33.0, -1.0), (33.0, 33.2), (-1.0, 33.2)]), disc,
            np.array([p + (-1e-7, -1e-7), p + (1e-7, -1e-7), p + (1e-7, 1e-7), p + (-1e-7, 1e-7)])], f


def loads_of(w):
    """Four columns of face powers and node heat as tests/test_thermal.py's report test makes them: column 2 is empty,
    column 3 repeats column 0.  And the powers of the three sources, likewise."""
    rng = np.random.default_rng(11)
    Pf = rng.uniform(0.0, 1e-3, (4, w.n_tri))
    nodes, cols, vals = rng.integers(0, w.n_pot, 15), rng.integers(0, 2, 15), rng.uniform(0.0, 1e-2, 15)
    Pf[2], Pf[3] = 0.0, Pf[0]
    again = cols == 0
    heat = (np.concatenate([nodes, nodes[again]]), np.concatenate([cols, np.full(again.sum(), 3)]), np.concatenate([vals, vals[again]]))
    watts = rng.uniform(0.01, 0.4, (4, 3))
    watts[2], watts[3] = 0.0, watts[0]
    return Pf, heat, watts


@pytest.fixture(scope="module")
def heated(wide):
    """The stacked handle with its three sources, one solve of four columns and everything read from it, twice where two
    calls must agree."""
    w = wide
    polygons, speck_face = footprints(w)
    Pf, heat, watts = loads_of(w)
    th = w.thermal(mesh_layer=w.layer_of, pairs=[(0, 1, G)])
    try:
        out = dict(polygons=polygons, speck_face=speck_face, Pf=Pf, watts=watts)
        out["set"] = th.set_sources(2, w.layer_of, [0, 0, 0], polygons)
        out["lists"] = th.source_lists()
        th.source_power(watts[:1])
        out["load"] = th.load(np.zeros((1, w.n_tri)))
        th.source_power(watts)
        out["theta"], res = th.solve(Pf, heat)
        assert res.status == _hip.OK
        out["report"] = [th.report(4, w.n_tri, w.n_vert) for _ in range(2)]
        out["flows"] = [th.stack_flows(4) for _ in range(2)]
        out["rise"] = [th.source_report(4) for _ in range(2)]
        out["G"] = th.stack_matrix()
        out["M"] = th.lumped(w.n_vert)
    finally:
        th.close()
    return out


def test_thermal_report_of_four_columns(wide, heated):
    """Face means, heat input (the sum of the face powers) and film loss (the sum of hM theta, one product of device
    outputs) bit for bit; the hotspot with its vertex exactly, in the empty column each mesh's first vertex; the envelope by
    the sequential rule."""
    w, theta, Pf = wide, heated["theta"], heated["Pf"]
    mean, top, vert, heat_in, loss, env, env_case = heated["report"][0]
    assert all(np.array_equal(a, b) for a, b in zip(heated["report"][0], heated["report"][1]))      # two calls, the same bits
    assert np.array_equal(heated["M"], w.M)
    c = T.corners(w.tri)
    for j in range(4):
        assert np.array_equal(mean[j], ((theta[j][c[:, 0]] + theta[j][c[:, 1]]) + theta[j][c[:, 2]]) / 3)
        for m in range(w.n_mesh):
            (lo, hi), (v0, v1) = w.faces(m), w.verts(m)
            assert heat_in[j, m] == F.mesh_sum(Pf[j, lo:hi]), (j, m)
            terms = w.hM[v0:v1] * theta[j, v0:v1]
            assert loss[j, m] == F.mesh_sum(terms), (j, m)
            assert abs(loss[j, m] - fsum(terms)) <= F.fold_bound(tiles(v1 - v0), fsum(np.abs(terms))), (j, m)
            assert (top[j, m], vert[j, m]) == F.mesh_top(theta[j, v0:v1], np.arange(v0, v1), empty=NEG_INF), (j, m)
    assert np.array_equal(vert[2], w.voff[:-1]) and (top[2] == 0.0).all()         # the complete tie over 260 tiles
    assert (theta[2] == 0.0).all() and np.array_equal(theta[3], theta[0]) and (top[0] > 0).all()
    best, which = T.envelope(theta[:, :w.n_vert])
    assert np.array_equal(env, best) and np.array_equal(env_case, which)
    assert (env_case == 0).any() and (env_case == 1).any() and not (env_case >= 2).any()


def test_interlayer_flows(wide, heated):
    """padne_thermal_stack_flows against stack_ref.flows on the device's own G and theta, bit for bit: A's 260 vertex tiles
    take the stack fold's strided loop twice."""
    w, theta = wide, heated["theta"]
    flow, area = heated["flows"][0]
    assert np.array_equal(flow, heated["flows"][1][0]) and np.array_equal(area, heated["flows"][1][1])
    indptr, indices, data, _diag = heated["G"]
    Goff = sp.csr_matrix((data, indices.astype(np.int64), indptr.astype(np.int64)), shape=(w.n_pot, w.n_pot))
    flow_want, area_want = K.flows(w.flat, w.layer_of, [(0, 1, G)], Goff, theta)
    print("flows", flow[:, 0], "area", area)
    assert np.array_equal(flow, flow_want) and np.array_equal(area, area_want)
    assert flow[2, 0] == 0.0 and flow[0, 0] != 0.0 and area[0] > 0.9 * 32.0 * 32.0


def test_heat_sources_lists_areas_loads_and_footprint_temperatures(wide, heated):
    """The list of 131 584 faces wraps the slot ``tile & 255`` twice, the disc's fills some slots and leaves others empty, the
    speck's owner is found in the last of the 514 strides of the owner search.  Everything is sources_ref's, bit for bit."""
    w = wide
    counts, fallback, area = heated["set"]
    ptr, face = heated["lists"]
    ref = SR.Restated(w.flat, w.layer_of, [(0, polygon) for polygon in heated["polygons"]])
    print("list lengths", counts, "fallback", fallback)
    assert counts[0] == COUNTS["A"][2] and 16_384 < counts[1] < 65_536 and counts[2] == 1
    assert np.array_equal(fallback, [0, 0, 1]) and face[ptr[2]] == heated["speck_face"]
    assert np.array_equal(counts, ref.counts) and np.array_equal(fallback.astype(bool), ref.fallback)
    assert np.array_equal(ptr, ref.ptr) and np.array_equal(face, ref.face)
    assert np.array_equal(area, ref.A)
    assert [F.list_sum(w.face_area[face[ptr[s]:ptr[s + 1]]]) for s in range(3)] == list(area)
    assert np.array_equal(heated["load"], ref.load(w.n_pot, heated["watts"][:1]))
    assert abs(fsum(heated["load"]) - fsum(heated["watts"][0])) <= 1e-13 * fsum(heated["watts"][0])
    assert np.array_equal(heated["rise"][0], heated["rise"][1])
    assert np.array_equal(heated["rise"][0], ref.temperature(heated["theta"], 0.0))
    assert (heated["rise"][0][[0, 1, 3]] > 0.0).all() and (heated["rise"][0][2] == 0.0).all()


# ---- transient ------------------------------------------------------------------------------------------------------------------

def test_two_transient_steps(wide):
    """Column 0 heats from ambient, column 1 holds the steady state of case 1, column 2 stays off: the complete tie."""
    w = wide
    cap_of_mesh = [3e-3 * (1 + layer) for layer in w.layer_of]
    Cv = R.capacity(w.voff, cap_of_mesh, w.M)
    Pf, heat, _watts = loads_of(w)
    keep = heat[1] < 2
    probes = np.array([0, w.voff[1] - 1, w.n_pot - 1], dtype=np.int64)
    dt = 3e-3 / FILM_STIFF / 20
    with contextlib.ExitStack() as stack:
        th = w.thermal()
        stack.callback(th.close)
        tr = _hip.Transient(th, cap_of_mesh)
        stack.callback(tr.close)
        assert np.array_equal(tr.capacity(w.n_vert), Cv)
        tr.loads(Pf[:2], (heat[0][keep], heat[1][keep], heat[2][keep]))
        tr.start([None, 1, None])
        states, outs = [tr.state()], []
        for _ in range(2):
            outs.append(tr.run(dt, 1, [0, 1, None], probes))
            states.append(tr.state())
        env, env_step = tr.envelope(w.n_vert)
    for out, theta in zip(outs, states[1:]):
        assert np.array_equal(out["probes"][0], theta[:, probes])
        for c in range(3):
            for m in range(w.n_mesh):
                v0, v1 = w.verts(m)
                assert out["stored"][0, c, m] == F.mesh_sum(Cv[v0:v1] * theta[c, v0:v1]), (c, m)
                assert out["loss"][0, c, m] == F.mesh_sum(w.hM[v0:v1] * theta[c, v0:v1]), (c, m)
                assert (out["max"][0, c, m], out["vertex"][0, c, m]) == F.mesh_top(theta[c, v0:v1], np.arange(v0, v1), empty=NEG_INF)
            top, vert, stored, loss = R.mesh_report(w.voff, Cv, w.hM, theta[c])          # transient_ref's own statement
            assert np.array_equal(out["max"][0, c], top) and np.array_equal(out["vertex"][0, c], vert)
            for m in range(w.n_mesh):
                v0, v1 = w.verts(m)
                n = tiles(v1 - v0)
                assert abs(out["stored"][0, c, m] - stored[m]) <= F.fold_bound(n, fsum(np.abs(Cv[v0:v1] * theta[c, v0:v1])))
                assert abs(out["loss"][0, c, m] - loss[m]) <= F.fold_bound(n, fsum(np.abs(w.hM[v0:v1] * theta[c, v0:v1])))
    assert np.array_equal(outs[1]["vertex"][0, 2], w.voff[:-1]) and (outs[1]["max"][0, 2] == 0.0).all()
    assert (outs[1]["stored"][0, 0] > outs[0]["stored"][0, 0]).all()              # column 0 heats
    states = np.stack(states)
    for c in range(3):
        best, step = R.envelope(states[:, c, :w.n_vert])
        assert np.array_equal(env[c], best) and np.array_equal(env_step[c], step), c
    assert (env_step[2] == 0).all() and env_step[0].max() == 2


# ---- electro-thermal --------------------------------------------------------------------------------------------------------------

def test_scale_means_and_increment(wide):
    """The increment is the largest change of a face mean, found by one workgroup over all 708 tiles: first anywhere (a
    random theta), then with the only change in the board's last faces (the third stride, wave 3), then in tile 300 (the
    second stride, wave 0)."""
    w = wide
    alpha = [3.93e-3 * (1 + 0.25 * m) for m in range(w.n_mesh)]
    rng = np.random.default_rng(8)
    thetas = [rng.uniform(0.0, 80.0, w.n_pot)]
    bumped = (w.n_tri - 1, 300 * 256 + 7)
    for f, bump in zip(bumped, (7.5, 3.25)):
        thetas.append(thetas[-1].copy())
        thetas[-1][w.tri[f]] += bump
    assert tiles(w.n_tri) == 708                             # (this kernel's tiles run over all faces, not mesh by mesh)
    with contextlib.ExitStack() as stack:
        th = w.thermal()
        stack.callback(th.close)
        coupled = _hip.Coupled(w.L.dev, th, alpha, 31.0, 20.0)
        stack.callback(coupled.close)
        coupled.set_scale(rng.uniform(0.5, 1.5, w.n_tri))
        got = []
        for theta in thetas:
            d = coupled.update(theta)
            got.append((d, *coupled.get_scale(w.n_tri, means=True)))
    prev = np.zeros(w.n_tri)
    for theta, (d, s, mean), f in zip(thetas, got, (None,) + bumped):
        s_want, mean_want = CR.scale(w.tri, w.face_mesh, alpha, 31.0, 20.0, theta)
        assert np.array_equal(mean, mean_want) and np.array_equal(s, s_want)
        at = int(np.argmax(np.abs(mean_want - prev)))
        print("increment", d, "at face", at, "tile", at // 256)
        assert d == np.abs(mean_want - prev).max() and d > 0 and f in (None, at)
        prev = mean_want


# ---- temperature sensitivities ------------------------------------------------------------------------------------------------------

def test_temperature_sensitivities_of_nine_objectives(ctx, wide):
    """tests/test_thermal_sensitivity_kernels.py's sequence and checks on this board, with a plan of the test's own (the
    adjoint block solve replaces a plan's finished block, and the shared one keeps V for the other tests): the owners, the
    right-hand sides with resistors and without, the three densities, and every per-mesh, per-pair and per-source sum against
    tests/tsens_kernel_ref.py and fold_ref bit for bit, on the device's own x, theta, lambda and mu; and every sum against
    math.fsum of the restated terms within fold_bound.  A's 514 face tiles and 260 vertex tiles make tsens_fold_kernel stride
    twice and three times with tiles in all four waves.  The objective in the dead case gives zeros everywhere but in dT/dP_s,
    which does not depend on the case."""
    w = wide
    polygons, speck_face = footprints(w)
    p = 0.5 * w.xy[w.tri[speck_face, 0]] + 0.3 * w.xy[w.tri[speck_face, 1]] + 0.2 * w.xy[w.tri[speck_face, 2]]
    (_a0, a1), _b, (c0, c1), (d0, _d1) = (w.verts(m) for m in range(4))
    in_D, in_B, in_300 = w.faces(3)[0] + 12_345, w.faces(1)[0], 300 * 256 + 7
    objectives = [KT.point(0, 0, p), KT.point(1, 1, KT.inside_face(w.xy, w.tri, in_D)), KT.point(0, 0, KT.inside_face(w.xy, w.tri, in_B)),
                  KT.point(1, 0, KT.inside_face(w.xy, w.tri, in_300)), KT.listed(0, [a1 - 1], [1.0]),
                  KT.listed(1, [c0 + 10, c0 + 4000, c1 - 1], [0.2, 0.3, 0.5]), KT.of_source(0, 0), KT.of_source(1, 1),
                  KT.listed(2, [1000], [1.0])]
    own = [(int(row[1]), int(row[2]), float(row[3])) for _, row in w.pairs if row[0] == "R"]
    resistors = KT.with_more(own, own[0][0], 30_000, c0 + 50, d0 + 77)
    watts = np.array([[0.2, 0.1, 0.05], [0.1, 0.3, 0.02], [0.0, 0.0, 0.0]])
    with contextlib.ExitStack() as stack:
        plan, V = quiet(finished_block, w.board, w.L, solver.check_load_cases(w.prob, w.cases))
        stack.callback(plan.close)
        th = w.thermal(mesh_layer=w.layer_of, pairs=[(0, 1, G)])
        stack.callback(th.close)
        th.set_sources(2, w.layer_of, [0, 0, 0], polygons)
        th.source_power(watts)
        theta, res = quiet(th.solve_kkt, plan, 3, rtol=solver.RTOL)
        assert res.status == _hip.OK
        indptr, indices, data, _diag = th.stack_matrix()
        out = KT.drive(ctx, th, plan, w.L, 3, w.kappa, w.layer_of, w.n_tri, objectives, resistors)
        Goff = sp.csr_matrix((data, indices.astype(np.int64), indptr.astype(np.int64)), shape=(w.n_pot, w.n_pot))
        B = KT.restated_board(w.flat, w.layer_of, w.sigma, w.kappa, w.hM, w.n_pot, w.L.shape[0], [(0, 1, G)], Goff,
                              SR.Restated(w.flat, w.layer_of, [(0, polygon) for polygon in polygons]))
        dev = types.SimpleNamespace(thermal=th, n_tri=w.n_tri, n_pot=w.n_pot)
        KT.check_g_through_the_solve(B, dev, objectives, out, watts)
    x = np.ascontiguousarray(V[:w.n_pot].T)
    assert (x[2] == 0.0).all() and (theta[2] == 0.0).all()                    # the dead case
    terms = KT.check(B, objectives, resistors, x, theta, out, "wide")
    assert KT.orders_show(B, objectives, resistors, x, out)
    assert np.array_equal(out.unknown[0], w.tri[speck_face]) and np.array_equal(out.unknown[1], w.tri[in_D])
    assert np.array_equal(out.unknown[2], w.tri[in_B]) and np.array_equal(out.unknown[3], w.tri[in_300])
    _ed, _kd, _cd, mesh_e, mesh_k = out.faces[0]
    none = np.zeros(1)
    for j, (ef, kf, ft, per) in enumerate(terms):
        for m in range(w.n_mesh):
            (lo, hi), (v0, v1) = w.faces(m), w.verts(m)
            w.sum_check(mesh_e[j, m], ef[lo:hi], none, tiles(hi - lo), f"e, objective {j}, mesh {m}")
            w.sum_check(mesh_k[j, m], kf[lo:hi], none, tiles(hi - lo), f"k, objective {j}, mesh {m}")
            w.sum_check(out.film[0][j, m], ft[v0:v1], none, tiles(v1 - v0), f"film, objective {j}, mesh {m}")
        # the pair: the meshes of layer 0 folded one by one, then joined by two more additions
        pt = per[0]
        bound = sum(F.fold_bound(tiles(w.verts(m)[1] - w.verts(m)[0]), fsum(np.abs(pt[w.verts(m)[0]:w.verts(m)[1]]))) for m in range(3))
        bound += 3 * U * fsum(np.abs(pt))
        print("pair, objective", j, out.pairs[0][j, 0], "error", abs(out.pairs[0][j, 0] + fsum(pt)), "bound", bound)
        assert abs(out.pairs[0][j, 0] + fsum(pt)) <= bound and not pt[d0:].any()
        lam = out.lam[j]
        c = T.corners(w.tri)
        mean = ((lam[c[:, 0]] + lam[c[:, 1]]) + lam[c[:, 2]]) / 3
        for s in range(3):
            mine = B.sources.face[B.sources.ptr[s]:B.sources.ptr[s + 1]]
            w.sum_check(out.sources[0][j, s], (w.face_area[mine] / B.sources.A[s]) * mean[mine], none, tiles(len(mine)),
                        f"source {s}, objective {j}")
    dead = 8
    assert not out.rhs[:, dead].any() and not out.mu[:, dead].any() and out.lam[dead].any()
    assert all(not a[dead].any() for a in out.faces[0]) and not out.film[0][dead].any() and not out.pairs[0][dead].any()
    assert (out.sources[0][dead] > 0.0).all()
    live = [j for j in range(9) if j != dead]
    assert (np.abs(mesh_e[live]) > 0).all() and (out.film[0][live] < 0).all() and (out.pairs[0][live] != 0).all()


# ---- the adaptive transient ---------------------------------------------------------------------------------------------------------

def test_one_adaptive_trial_step_of_four_columns(wide):
    """One trial of 4 dt from ambient (dt and the capacities of test_two_transient_steps); the only load of columns 0, 1 and 2
    is node heat of 1e-2 W at one vertex of A each, column 3 is off.  theta* is sdirk_ref.extrapolate's; err and its vertex are
    fold_ref.mesh_top per mesh on the restated estimate, then the meshes in ascending order.  The condition under which this
    reaches what the table says: the winners lie in A's vertex tiles 259, 257 and 200 -- the second stride of lanes 3 and 1 of
    sdirk_fold_kernel, and wave 3 of the first stride -- which holds because one step after a point heat is switched on the
    estimate peaks at the heated vertex (asserted).  Column 3: err exactly 0.0 at vertex 0."""
    w = wide
    cap_of_mesh = [3e-3 * (1 + layer) for layer in w.layer_of]
    dt = 3e-3 / FILM_STIFF / 20
    hot = np.array([w.voff[1] - 1, w.voff[1] - 300, 200 * 256 + 5], dtype=np.int64)
    assert (hot // 256).tolist() == [259, 257, 200] and hot.max() < w.voff[1]
    with contextlib.ExitStack() as stack:
        th = w.thermal()
        stack.callback(th.close)
        tr = _hip.Transient(th, cap_of_mesh)
        stack.callback(tr.close)
        tr.loads(np.zeros((3, w.n_tri)), (hot, np.arange(3), np.full(3, 1e-2)))
        tr.start([None] * 4)
        first = quiet(tr.try_step, 4 * dt, [0, 1, 2, None])
        out = quiet(tr.try_step, 4 * dt, [0, 1, 2, None])
        theta_n, theta_1, star, theta_new = tr.state(), tr.trial(0), tr.trial(1), tr.trial(2)
    assert np.array_equal(first["err"], out["err"]) and np.array_equal(first["vertex"], out["vertex"])      # two calls, the same bits
    assert not theta_n.any() and np.array_equal(star, SD.extrapolate(theta_n, theta_1, w.n_vert))
    est = SD.estimate(theta_n, theta_1, star, theta_new, w.n_vert)
    for c in range(4):
        best = (0.0, -1)
        for m in range(w.n_mesh):
            v0, v1 = w.verts(m)
            top = F.mesh_top(np.abs(est[c, v0:v1]), np.arange(v0, v1), empty=NEG_INF)
            if v1 > v0 and (best[1] < 0 or top[0] > best[0]):
                best = top
        print("column", c, "err", out["err"][c], "at", out["vertex"][c], "tile", out["vertex"][c] // 256)
        assert (out["err"][c], out["vertex"][c]) == best, c
        assert (out["err"][c], out["vertex"][c]) == SD.error_of(est[c]), c
    assert (out["vertex"][:3] // 256).tolist() == [259, 257, 200] and np.array_equal(out["vertex"][:3], hot)
    assert (out["err"][:3] > 0.0).all()
    assert out["err"][3] == 0.0 and not np.signbit(out["err"][3]) and out["vertex"][3] == 0


# ---- the electro-thermal transient --------------------------------------------------------------------------------------------------

def test_electrothermal_transient_load_and_scale_range(wide):
    """tests/test_coupled_transient.py::test_the_new_entries_are_the_restatement_bit_for_bit on this board: a scale with its
    smallest value planted in the board's last face (tile 707, the third stride) and its largest in face 300 * 256 + 7 (tile
    300, the second stride), revalued; the range of the used scale is found over all 708 tiles.  Then a slot of a reserved
    table from a block solved on the revalued system: the load is the restatement's on the block's own potentials, the per-mesh
    copper heat is fold_ref's sum of the restated face powers bit for bit, math.fsum's within fold_bound, and the bits of
    padne_thermal_report's heat after padne_coupled_solve_kkt.  The assembled values are put back at the end (a scale of 1)."""
    w = wide
    alpha = [3.93e-3 * (1 + 0.25 * m) for m in range(w.n_mesh)]
    cap_of_mesh = [3e-3 * (1 + layer) for layer in w.layer_of]
    rng = np.random.default_rng(9)
    s = rng.uniform(0.5, 1.5, w.n_tri)
    s[w.n_tri - 1], s[300 * 256 + 7] = 0.25, 1.75
    nodes = rng.integers(0, w.n_pot, 6)
    nodes[:2] = nodes[0]
    heat = (nodes, np.zeros(6, dtype=np.int32), rng.uniform(0.0, 1e-2, 6))
    assert tiles(w.n_tri) == 708 and (w.n_tri - 1) // 256 == 707
    with contextlib.ExitStack() as stack:
        th = w.thermal()
        stack.callback(th.close)
        tr = _hip.Transient(th, cap_of_mesh)
        stack.callback(tr.close)
        coupled = _hip.Coupled(w.L.dev, th, alpha, 31.0, 20.0)
        stack.callback(coupled.close)

        def restore():                                       # L's assembled values back for whatever runs after this test
            coupled.set_scale(np.ones(w.n_tri))
            coupled.revalue()
        coupled.set_scale(s)
        coupled.revalue()
        stack.callback(restore)
        s_used = coupled.get_scale(w.n_tri, used=True)
        ranges = [coupled.scale_range() for _ in range(2)]
        plan, V = quiet(finished_block, w.board, w.L, solver.check_load_cases(w.prob, w.cases)[:1])
        stack.callback(plan.close)
        tr.reserve_loads(2)
        mesh_heat = coupled.transient_load(tr, plan, 1, heat)
        again = coupled.transient_load(tr, plan, 1, heat)
        table = tr.load_vectors()
        quiet(coupled.solve_kkt, plan, heat)
        report_heat = th.report(1, w.n_tri, w.n_vert, fields=False, envelope=False)[3][0]
    assert np.array_equal(s_used, s) and ranges[0] == ranges[1] == (s_used.min(), s_used.max()) == (0.25, 1.75)
    Pf = CR.face_power(w.xy, w.tri, w.face_mesh, w.sigma, s_used, V[:w.n_vert, 0])
    want = T.load(w.n_pot, w.tri, Pf, [(int(n), float(v)) for n, v in zip(heat[0], heat[2])])
    assert np.array_equal(table[1], want) and not table[0].any() and np.abs(want).max() > 0.0
    assert np.array_equal(mesh_heat, again) and np.array_equal(mesh_heat, report_heat)      # two calls, the same bits
    for m in range(w.n_mesh):
        lo, hi = w.faces(m)
        assert mesh_heat[m] == F.mesh_sum(Pf[lo:hi]), m
        w.sum_check(mesh_heat[m], Pf[lo:hi], np.zeros(1), tiles(hi - lo), f"copper heat, mesh {m}")
    assert (mesh_heat > 0.0).all()


# ---- film curves ----------------------------------------------------------------------------------------------------------------------

FILM_ORDER = (64, 1, 2, 2)                                   # knots of the tables of A, B, C and D
FILM_TILE0 = np.cumsum([0] + [COUNTS[name][1] for name in GRIDS])      # the first global tile of every mesh: A 0, B 260, C 261, D 295
#            heated vertex as (mesh, tile of the mesh, lane), watts, the global tile of film_fold_kernel it lies in
FILM_RUNS = [((0, 200, 5), 0.05, 200), ((0, 259, 1), 0.5, 259), ((3, 5, 9), 0.05, 300), ((3, 65, 129), 0.3, 360)]


def film_tile(w, v):
    """The global tile of film_terms_kernel that holds vertex v: the tiles are per mesh and numbered through."""
    m = int(np.searchsorted(w.voff, v, side="right")) - 1
    return int(FILM_TILE0[m]) + (int(v) - int(w.voff[m])) // 256


def film_tables(w):
    tables = TF.tables_for(w.film, FILM_ORDER)
    assert [len(rise) for rise, _film in tables] == list(FILM_ORDER) and FILM_TILE0[-1] == 361
    return tables


def beyond_of(w, tables, theta):
    """The vertices above the last knot of their mesh's table, tables of one knot left out."""
    return np.concatenate([np.flatnonzero(theta[v0:v1] > rise[-1]) + v0 for (rise, _film), (v0, v1) in
                           zip(tables, (w.verts(m) for m in range(w.n_mesh))) if len(rise) > 1] + [np.zeros(0, dtype=np.int64)])


def test_film_terms_and_the_count_above_the_last_knot_on_361_tiles(wide):
    """tests/test_film.py's comparison of the terms on this board: g, c, hM and the count for a theta on, beside and beyond the
    knots; for 1e6 everywhere, where every tile of a table of more than one knot counts 256 or its ragged rest; and for two
    vertices above their last knot, one in tile 256 and one at the end of tile 360 -- lanes 0 and 104 of film_fold_kernel, both
    in the second stride.  Two calls give the same bits and the matrix keeps its own."""
    w = wide
    tables = film_tables(w)
    two = np.zeros(w.n_vert)
    planted = [256 * 256 + 3, w.n_vert - 1]
    two[planted] = 100.0
    assert [film_tile(w, v) for v in planted] == [256, 360] and all(rise[-1] < 100.0 for rise, _film in tables)
    thetas = [TF.probing_theta(tables, w.voff, 3), np.full(w.n_vert, 1e6), two]
    th = w.thermal()
    try:
        th.set_film_curves(tables)
        before = th.matrix().to_scipy().data.copy()
        got = [th.film_terms(theta, w.n_vert) for theta in thetas]
        again = [th.film_terms(theta, w.n_vert) for theta in thetas]
        after = th.matrix().to_scipy().data.copy()
        M = th.lumped(w.n_vert)
    finally:
        th.close()
    assert np.array_equal(M, w.M) and TF.same_bits(before, after)
    for theta, out, twice in zip(thetas, got, again):
        want = FR.terms(tables, w.voff, M, theta)
        for k, what in enumerate(("g", "c", "hM")):
            assert TF.same_bits(out[k], want[k]), what
            assert TF.same_bits(twice[k], out[k]), what
        print("above the last knot:", out[3])
        assert out[3] == want[3] == twice[3] == len(beyond_of(w, tables, theta))
    assert got[0][3] > 0 and (np.unique([film_tile(w, v) for v in beyond_of(w, tables, thetas[0])]) >= 256).any()
    assert got[1][3] == COUNTS["A"][0] + COUNTS["C"][0] + COUNTS["D"][0] == w.n_vert - COUNTS["B"][0]
    assert got[2][3] == 2


def test_film_increment_its_vertex_the_count_and_hM_on_361_tiles(wide):
    """Two Newton rounds by hand per heated vertex, node heat at one vertex each.  After every padne_thermal_film_increment the
    triple is, exactly: the largest |theta_new - theta_lin| of the device's own downloaded thetas, the lowest vertex that attains
    it, and the number of vertices above their last knot; film_ref.increment states the first two in the kernels' order and
    agrees.  The condition under which this reaches what the table at the top says: the change peaks at the heated vertex in
    both rounds (asserted on the expected value; on the host restatement of this board the runner-up of the second round, a
    neighbour, lies 0.5 % to 5 % below), in tile 200 (wave 3 of the first stride), 259 (lane 3 of the second stride), 300 (lane
    44) and 360 (lane 104: the board's last vertex, in a ragged tile).  0.5 W and 0.3 W lift the heated vertex of tiles 259 and
    360 above the last knot, 90 K: a count that is not 0, from the second stride (asserted on the host's count).  The film loss
    of the report afterwards holds the hM the increment pass rewrote: fold_ref's sum of hM(theta) theta bit for bit.  A dead
    load is the complete tie over 361 tiles: (+0.0, vertex 0, 0).  With the curves removed the matrix has the bits it had."""
    w = wide
    tables = film_tables(w)
    none = np.zeros((1, w.n_tri))
    th = w.thermal()
    runs = []
    try:
        before = th.matrix().to_scipy().data.copy()
        th.set_film_curves(tables)
        M = th.lumped(w.n_vert)
        for (m, tile, lane), watts, _where in FILM_RUNS:
            v = w.verts(m)[0] + tile * 256 + lane
            th.film_linearise(False)
            first, res = th.solve(none, ([v], [0], [watts]))
            assert res.status == _hip.OK
            rounds = [(th.film_increment(), first[0], np.zeros(w.n_pot))]
            th.film_linearise(True)
            second, res = th.resolve()
            assert res.status == _hip.OK
            rounds.append((th.film_increment(), second[0], first[0]))
            runs.append((v, rounds, th.report(1, w.n_tri, w.n_vert, fields=False, envelope=False)[4][0]))
        linearised = th.matrix().to_scipy().data.copy()
        th.film_linearise(False)
        cold, res = th.solve(none)
        dead = th.film_increment()
        th.set_film_curves([])
        after = th.matrix().to_scipy().data.copy()
    finally:
        th.close()
    assert runs[-1][0] == w.n_vert - 1
    counted_late = 0
    for (v, rounds, loss), (_at, watts, where) in zip(runs, FILM_RUNS):
        for k, (got, new, lin) in enumerate(rounds):
            moved = np.abs(new[:w.n_vert] - lin[:w.n_vert])
            above = beyond_of(w, tables, new[:w.n_vert])
            want = (float(moved.max()), int(np.argmax(moved)), len(above))
            print("tile", where, "round", k, "device", got, "host", want, "runner-up", np.sort(moved)[-2])
            assert film_tile(w, want[1]) == where and want[1] == v and want[0] > 0.0
            assert got == want
            assert FR.increment(w.voff, new, lin) == want[:2]
            assert want[2] == FR.terms(tables, w.voff, M, new[:w.n_vert])[3]
            if watts > 0.1:
                assert want[2] > 0 and max(film_tile(w, u) for u in above) >= 256
                counted_late += 1
        theta = rounds[1][1]
        hM_want = FR.terms(tables, w.voff, M, theta[:w.n_vert])[2]
        assert not TF.same_bits(hM_want, w.hM)
        for mesh_i in range(w.n_mesh):
            v0, v1 = w.verts(mesh_i)
            terms = hM_want[v0:v1] * theta[v0:v1]
            assert loss[mesh_i] == F.mesh_sum(terms), (where, mesh_i)
            assert abs(loss[mesh_i] - fsum(terms)) <= F.fold_bound(tiles(v1 - v0), fsum(np.abs(terms))), (where, mesh_i)
    assert counted_late == 4
    assert not cold.any() and dead == (0.0, 0, 0) and not np.signbit(dead[0])
    assert TF.same_bits(after, before) and not TF.same_bits(linearised, before)


# ---- resistors that follow their temperature -----------------------------------------------------------------------------------------

N_LONG = 66_000


@pytest.fixture(scope="module")
def long_strips(ctx):
    """resistor_coupling_ref.strips_system(66 000) on the device, opened as tests/test_resistor_coupling.py opens its strips:
    66 006 resistors (258 tiles of coupled_resistor_scale_kernel), 132 001 touched rows (516 tiles of
    coupled_resistor_revalue_kernel) and 132 010 incidences (516 tiles of coupled_resistor_places_kernel)."""
    with opened(ctx, "strips", n=N_LONG) as d:
        assert d.n_res == N_LONG + 6 and tiles(d.n_res) == 258 and d.n_pot == 2 * N_LONG + 1
        incident = np.concatenate([d.a[d.a != d.b], d.b[d.a != d.b]])
        assert len(incident) == 132_010 and len(np.unique(incident)) == 132_001 and tiles(132_001) == 516
        try:
            yield d
        finally:
            d.coupled.close()                                # (the revalue test leaves a handle of its own here)


def test_resistor_scale_means_and_increment_on_258_tiles(long_strips):
    """A random theta first: scales and means are the restatement's, the increment the larger of the faces' and the resistors'.
    Then three thetas that differ from the one before at both ends of ONE resistor, in tile 257 (lane 1 of coupled_fold_kernel,
    second stride), 256 (lane 0, second stride) and 200 (wave 3): the increment is that resistor's change.  It is the
    resistors' and not the faces' because a face sees only one of the two ends, and through a third of its mean (asserted)."""
    d = long_strips
    cp = d.coupled
    alpha, t0, thetas, _k = coefficients(d, np.random.default_rng(41))
    bumped = (257 * 256 + 9, 256 * 256 + 100, 200 * 256 + 17)
    assert all(r < N_LONG for r in bumped) and [r // 256 for r in bumped] == [257, 256, 200]
    thetas = thetas[:1]
    for r, bump in zip(bumped, (7.5, 3.25, 1.125)):
        thetas.append(thetas[-1].copy())
        thetas[-1][[d.a[r], d.b[r]]] += bump
    cp.set_resistors(d.a, d.b, d.R, alpha, t0)
    cp.reset()
    got = []
    for theta in thetas:
        inc = cp.update(theta)
        got.append((inc, *cp.get_resistors(d.n_res, means=True)))
    prev, prev_f = np.zeros(d.n_res), np.zeros(d.n_tri)
    for theta, (inc, s, mean), r in zip(thetas, got, (None,) + bumped):
        s_want, mean_want, d_r = RC.resistor_scale(theta, d.a, d.b, alpha, AMBIENT, t0, prev)
        mean_f = CR.face_means(d.tri, theta)
        d_f = np.abs(mean_f - prev_f)
        print("increment", inc, "resistors", d_r.max(), "at", int(np.argmax(d_r)), "tile", int(np.argmax(d_r)) // 256, "faces", d_f.max())
        assert np.array_equal(s, s_want) and np.array_equal(mean, mean_want)
        assert inc == max(d_f.max(), d_r.max()) and inc > 0.0
        if r is not None:
            assert inc == d_r.max() and int(np.argmax(d_r)) == r and d_r.max() > d_f.max()
            assert np.count_nonzero(d_r) == 1
        prev, prev_f = mean_want, mean_f


def test_the_lowest_invalid_resistor_across_tiles(long_strips):
    """alpha = -0.05 at 60 K above ambient, as tests/test_resistor_coupling.py provokes the report (a refusal by value): of two
    in tiles 100 and 257 the one in tile 100 is named, and the one in tile 257 when it is alone."""
    d = long_strips
    cp = d.coupled
    early, late = 100 * 256 + 7, 257 * 256 + 3
    assert late < d.n_res and (early // 256, late // 256) == (100, 257)
    for planted, named in (([early, late], early), ([late], late)):
        bad = np.zeros(d.n_res)
        bad[planted] = -0.05
        cp.set_resistors(d.a, d.b, d.R, bad, np.full(d.n_res, T0))
        with pytest.raises(ValueError, match=rf"resistor {named}\b"):
            cp.update(np.full(d.n_pot, 60.0))
    cp.set_resistors(d.a, d.b, d.R, np.zeros(d.n_res), np.full(d.n_res, T0))
    assert cp.update(np.full(d.n_pot, 60.0)) >= 0.0          # and with none the same theta is taken


def test_resistor_revalue_on_516_tiles_of_rows(long_strips):
    """tests/test_resistor_coupling.py::test_revalue_is_the_restatement_bit_for_bit's sequence on the long strips: the values of
    the restatement's sequential updates on 132 001 touched rows, a symmetric potential block, zero coefficients the face-only
    bytes, and after the close the assembled bytes."""
    d = long_strips
    rng = np.random.default_rng(42)
    alpha, t0, thetas, _k = coefficients(d, rng)
    s_f = rng.uniform(0.5, 1.5, d.n_tri)
    cp = d.coupled
    L0 = sorted_csr(d.L.to_scipy())

    def revalued(al):
        cp.set_resistors(d.a, d.b, d.R, al, t0)
        cp.update(thetas[0])
        cp.set_scale(s_f)
        cp.revalue()
        return sorted_csr(d.L.to_scipy()), cp.get_resistors(d.n_res, used=True)

    L, used = revalued(alpha)
    L_again, _ = revalued(alpha)
    L_ones, used_ones = revalued(np.zeros(d.n_res))
    cp.set_resistors([], [], [], [], [])
    cp.update(thetas[0])
    cp.set_scale(s_f)
    cp.revalue()
    L_faces = sorted_csr(d.L.to_scipy())
    cp.set_resistors(d.a, d.b, d.R, alpha, t0)
    cp.revalue()
    cp.close()
    L_after = sorted_csr(d.L.to_scipy())
    d.coupled = _hip.Coupled(d.L, d.thermal, d.face_alpha, AMBIENT, T0)      # for whichever test of the fixture runs next
    sr, _mean, _d = RC.resistor_scale(thetas[0], d.a, d.b, alpha, AMBIENT, t0, np.zeros(d.n_res))
    faces = CR.revalue(L0, d.xy, d.tri, d.face_mesh, d.sigma, s_f)
    at = RC.places(L0, d.a, d.b)
    want = RC.revalue_resistors(faces, at, sr, 1 / d.R)
    assert len(at) == 132_010 and tiles(len({row for row, *_ in at})) == 516
    assert np.array_equal(used, sr) and (used_ones == 1.0).all()
    assert np.array_equal(L.indices, L0.indices) and np.array_equal(L.data, want.data) and np.array_equal(L_again.data, L.data)
    assert (want != faces).nnz > 2 * N_LONG
    K = L[:d.n_pot, :d.n_pot]
    assert (K != K.T).nnz == 0
    assert L_ones.data.tobytes() == L_faces.data.tobytes() == faces.data.tobytes()
    assert np.array_equal(L_after.data, L0.data) and not np.array_equal(L.data, L0.data)
    assert faces[20, 21] != L0[20, 21] and L[20, 21] != faces[20, 21] and L[20, 21] == L[21, 20]

"""Every per-mesh kernel on a board of 1 100 meshes (tests/many_meshes_board.py): where a mesh is found among a thousand offsets
(find_segment of csrc/face.hpp), where nearly every workgroup of a fixed-order fold holds one ragged tile of 2 to 32 live
lanes, where the tile tables have about one tile per mesh, and where the strip-numbering key carries 11 bits of mesh.  The
other axis, few meshes of many tiles, is tests/test_many_tiles.py's; its comparison rule and its tolerances are kept:

Where the summed term is a device output, or one IEEE operation on device outputs, the per-mesh sum is compared bit for bit
with fold_ref.  Elsewhere it is compared with math.fsum of the restatement's per-item terms within fold_ref.fold_bound plus
the tolerance the entry's own test grants per item, summed over the items.  Tops and their indices are exact everywhere.

Consecutive meshes lie on different layers with different conductances, and every raw entry that takes per-mesh values gets
values that differ between consecutive meshes by exactly representable factors: a face, vertex or tile attributed to the mesh
before or after changes the bits."""
import contextlib
import types
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import coupled_ref as CR
import currents_ref as C
import film_ref as FR
import fold_ref as F
import goal_ref as GR
import gridmesh_graded_ref as GG
import gridmesh_ref as GM
import many_meshes_board as B
import refine_ref as RR
import sampling_ref as SMP
import sdirk_ref as SD
import sensitivity_ref as S
import sources_ref as SR
import stack_ref as K
import temperature_sampling_ref as TR
import test_film as TF
import test_gridmesh as GMT
import test_gridmesh_graded as GGT
import test_refine as RF
import test_sampling as TS
import test_thermal_sensitivity_kernels as KT
import thermal_ref as T
import transient_ref as R
from many_meshes_board import fsum, tiles
from oracle import padne_oracle as O
from padne_amd import _hip, mesh, reduction, solver
from test_device_memory import three_ways
from test_load_case_currents import finished_block, plan_cuts, refined_solves
from test_many_tiles import NEG_INF, REL_TOL, TOL, U, Wide
from test_stack_host import G
from test_thermal import FILM_STIFF, links_of, quiet

pytestmark = pytest.mark.gpu

class Many(B.Board):
    """The board with its thermal model: kappa and film per mesh, different between consecutive meshes."""

    def __init__(self):
        super().__init__()
        checked = solver.check_thermal_model(self.prob, solver.ThermalModel(film=FILM_STIFF))
        self.kappa = [checked.kappa[l] * (1 + (m % 5) / 8) for m, l in enumerate(self.layer_of)]
        self.film = [checked.film[l] * (1 + (m % 3) / 4) for m, l in enumerate(self.layer_of)]
        self.links = links_of(self.pairs, checked)
        self.hM = np.repeat(np.asarray(self.film, dtype=np.float64), np.diff(self.voff)) * self.M
        self.stack_pairs = [(0, 3, G), (1, 3, G), (2, 3, G)]

    def thermal(self, **kw):
        return _hip.Thermal(self.L.dev, self.n_pot, self.kappa, self.film, [l[0] for l in self.links], [l[1] for l in self.links],
                            [l[2] for l in self.links], **kw)

    def solved(self):
        """solve_meshed_currents of the board, twice, made once: [(Solution, CurrentReport)] * 2."""
        if self._solved is None:
            self._solved = [quiet(solver.solve_meshed_currents, self.prob, self.meshes, self.layer_of) for _ in range(2)]
        return self._solved

    _solved = None
    sum_check = Wide.sum_check


@pytest.fixture(scope="module")
def many(ctx):
    w = Many()
    assert (w.n_mesh, w.n_vert, w.n_tri) == (B.N_MESH, B.N_VERT, B.N_TRI)
    with w.board.assembled() as (L, r):
        w.L, w.r = L, r
        w.plan, w.V = quiet(finished_block, w.board, L, solver.check_load_cases(w.prob, w.cases))
        try:
            yield w
        finally:
            w.plan.close()


# ---- 1. assembly and solve ------------------------------------------------------------------------------------------------------

def test_assembly_is_the_oracle_bit_for_bit_and_the_solve_is_the_direct_solve(many):
    """assemble (the cotangents of 18 266 faces, each with its mesh's conductance, the exact zeros of the right angles dropped)
    against the oracle's assemble_system: the same structure and the same bits.  solve_meshed_currents' potentials against
    the direct solve within REL_TOL of the largest, its power densities the oracle's on its own potentials bit for bit, and
    two calls the same bits."""
    w = many
    M, _R, X = w.direct()
    M = sp.csr_matrix(M)
    M.sort_indices()
    got = w.L.tocsr()
    assert np.array_equal(got.indptr, M.indptr) and np.array_equal(got.indices, M.indices)
    assert np.array_equal(got.data, M.data), "device assembly differs from the oracle"
    pad = w.mesh_of["pad", 0]                                 # a 2 x 2 pad: its diagonal is a dropped zero
    assert got[w.verts(pad)[0] + 1, w.verts(pad)[0] + 2] == 0.0 and got[w.verts(pad)[0], w.verts(pad)[0] + 1] != 0.0
    runs = w.solved()
    sol, _rep = runs[0]
    assert sol.solver_info.residual_norm < 1e-9
    v = np.zeros(w.n_vert)
    for li, ls in enumerate(sol.layer_solutions):
        for (m, msh, lo, hi), zf, tf in zip(w.board.layer_meshes(li), ls.potentials, ls.power_densities):
            v0, v1 = w.verts(m)
            v[v0:v1] = zf.values
            assert np.array_equal(tf.values, O.power_density(msh.points, msh.triangles, zf.values, w.sigma[m])), m
    print("potentials against the direct solve:", np.abs(v - X[:w.n_vert, 0]).max() / np.abs(X[:, 0]).max())
    assert np.abs(v - X[:w.n_vert, 0]).max() <= REL_TOL * np.abs(X[:, 0]).max()
    assert np.abs(w.V[:w.n_pot] - X[:w.n_pot]).max() <= REL_TOL * np.abs(X).max()            # the block of the fixture, too
    for la, lb in zip(runs[0][0].layer_solutions, runs[1][0].layer_solutions):
        assert all(np.array_equal(a.values, b.values) for a, b in zip(la.potentials, lb.potentials))
        assert all(np.array_equal(a.values, b.values) for a, b in zip(la.power_densities, lb.power_densities))
    pd = w.L.dev.power_density(X[:w.n_vert, 0], w.n_tri)      # and the mesh the system keeps, on the oracle's potentials
    for m in range(w.n_mesh):
        (lo, hi), (v0, v1) = w.faces(m), w.verts(m)
        assert np.array_equal(pd[lo:hi], O.power_density(w.flat[m][0], w.flat[m][1], X[v0:v1, 0], w.sigma[m])), m


# ---- 2. currents of the three cases, and cuts -----------------------------------------------------------------------------------

def cuts_of(w):
    """Along row 0 of the pads on layer 0 (it crosses every third pad of the row and the gaps between them; no vertex lies on
    it), and across the plane."""
    return [solver.Cut(w.layers[0], (-2.0, 0.12), (100.0, 0.12)), solver.Cut(w.layers[3], (50.3, -2.0), (50.3, 95.0))]


def check_currents(w, first, second, one, cl, cxy):
    assert all(np.array_equal(a, b) for a, b in zip(first, second))              # two calls, the same bits
    J, mag, env, env_case, mmax, mface, mpow, cut = first
    assert np.array_equal(one[2], mmax[0]) and np.array_equal(one[3], mface[0]) and np.array_equal(one[4], cut[0])
    assert (mmax[0] > 0).all() and (mpow[0] > 0).all()                            # every mesh carries current in case 0
    layer_tiles = [sum(tiles(w.toff[m + 1] - w.toff[m]) for m in range(w.n_mesh) if w.layer_of[m] == l) for l in range(4)]
    n_terms = {}
    for j in range(3):
        xj = w.V[:, j]
        power = T.face_power(w.xy, w.tri, w.face_mesh, w.sigma, xj[:w.n_vert])
        for m in range(w.n_mesh):
            lo, hi = w.faces(m)
            assert (mmax[j, m], mface[j, m]) == F.mesh_top(mag[j, lo:hi], np.arange(lo, hi)), (j, m)
            assert mpow[j, m] == F.mesh_sum(power[lo:hi]), (j, m)
            assert abs(mpow[j, m] - fsum(power[lo:hi])) <= F.fold_bound(tiles(hi - lo), fsum(power[lo:hi])) + TOL * fsum(power[lo:hi])
        for c in range(2):
            terms = C.cut_terms(w.system, xj, cl[c], cxy[c, :2], cxy[c, 2:])
            n_terms[j, c] = len(terms)
            w.sum_check(cut[j, c], terms, TOL * np.abs(terms), layer_tiles[cl[c]], f"cut {c}, case {j}")
    row_pads = [w.mesh_of["pad", k] for k in range(0, B.PER_ROW, 3)]
    crossed = np.unique(w.face_mesh[np.flatnonzero((w.xy[w.tri, 1].min(axis=1) < 0.12) & (w.xy[w.tri, 1].max(axis=1) > 0.12)
                                                   & (w.ml[w.face_mesh] == 0))])
    assert crossed.tolist() == row_pads and n_terms[0, 0] >= 2 * len(row_pads) and n_terms[0, 1] > 38
    assert (np.abs(cut[:2]) > 0).all()
    assert np.array_equal(mface[2], w.toff[:-1]) and (mmax[2] == 0.0).all() and (mpow[2] == 0.0).all() and (cut[2] == 0.0).all()
    want_env, want_case = solver.envelope_of(mag)
    assert np.array_equal(env, want_env) and np.array_equal(env_case, want_case)
    assert (env_case == 1).any() and (env_case == 0).any()


def run_currents(w, plan):
    cl, cxy = plan_cuts(w.system, cuts_of(w))
    first = plan.current_cases(3, w.n_tri, w.ml, cl, cxy)
    second = plan.current_cases(3, w.n_tri, w.ml, cl, cxy)
    one = plan.current_report(3, w.n_tri, w.ml, cl, cxy)
    return first, second, one, cl, cxy


def test_currents_of_three_cases_and_two_cuts(many):
    """tests/test_many_tiles.py::test_currents_of_three_cases on this board: per case and mesh the hotspot and its face exactly,
    the power bit for bit with fold_ref.mesh_sum of the restated face powers; the cut along a row of pads and the cut across
    the plane against math.fsum of currents_ref.cut_terms; the dead case zeros with every hotspot at its mesh's first face; the
    envelope solver.envelope_of's."""
    check_currents(many, *run_currents(many, many.plan))


# ---- 3. sensitivity totals, error estimate and goal error ---------------------------------------------------------------------

def test_sensitivity_totals_of_two_objectives(many):
    """tests/test_many_tiles.py's test of the same name, per mesh of this board."""
    w = many
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


def test_error_estimate_and_goal_error_of_one_objective(many):
    """tests/test_many_tiles.py's test of the same name, per mesh of this board.  The 2-face meshes have vertices whose
    recovery sums take one face (two corners) or two (the ends of the diagonal)."""
    w = many
    G_, eta, mesh_E, mesh_P, mesh_max, mesh_face = w.plan.error_estimate(3, w.n_tri, w.n_vert, w.n_mesh)
    _p, field0, dual, delta, omega, m_omega, m_delta, m_top, m_face = w.plan.goal_error(np.array([[0.0, 1.0, 0.0]]), w.n_tri, w.n_vert,
                                                                                     w.n_mesh)
    for a, b in zip(field0, (G_, eta, mesh_E, mesh_P, mesh_max, mesh_face)):
        assert np.array_equal(a, b)                          # goal.hip's fold of field 0 is error.hip's, bit for bit
    want = GR.goal_flat(w.xy, w.tri, w.face_mesh, w.sigma, np.stack([w.V[:w.n_vert, 0], w.V[:w.n_vert, 1]]))
    est = want.primal
    s0 = est.eta_scale(w.tri)
    pair = want.pair_scale(w.tri, 0)
    eta2 = est.eta * est.eta
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
    # (a 2-face pad whose two face gradients are the same bits has eta = 0 exactly: eight of them in the restatement)
    assert (mesh_E >= 0).all() and (mesh_E[np.diff(w.toff) > 2] > 0).all() and (delta[0] < 0).any() and (delta[0] > 0).any()
    faces_at = np.bincount(w.tri.reshape(-1), minlength=w.n_vert)
    v0 = w.verts(w.mesh_of["pad", 0])[0]
    assert sorted(faces_at[v0:v0 + 4].tolist()) == [1, 1, 2, 2]


# ---- 4. the thermal report, the interlayer flows and the heat sources ------------------------------------------------------------

def footprints(w):
    """A rectangle over the 5 x 5 block of pads of columns 10-14 and rows 10-14: on layer 1 it covers only that layer's pads of
    the block, scattered through the numbering.  A rectangle over all of layer 3: the plane and the 43 pads, spread over the
    whole mesh order.  A speck inside a face of the last 2-face pad of layer 1, off its centroid: the fallback, whose owner is
    found after the walk has passed about a thousand meshes.  Returns ((layer, polygon) per source, the speck's face)."""
    last = max(m for m in range(w.n_mesh) if w.layer_of[m] == 1 and w.toff[m + 1] - w.toff[m] == 2)
    f = w.faces(last)[0] + 1
    p = 0.5 * w.xy[w.tri[f, 0]] + 0.3 * w.xy[w.tri[f, 1]] + 0.2 * w.xy[w.tri[f, 2]]
    block = np.array([(29.5, 29.5), (44.0, 29.5), (44.0, 44.0), (29.5, 44.0)])
    all3 = np.array([(-2.0, -2.0), (135.0, -2.0), (135.0, 100.0), (-2.0, 100.0)])
    speck = np.array([p + (-1e-7, -1e-7), p + (1e-7, -1e-7), p + (1e-7, 1e-7), p + (-1e-7, 1e-7)])
    return [(1, block), (3, all3), (1, speck)], f, last


def loads_of(w):
    """tests/test_many_tiles.py::loads_of's pattern: four columns of face powers and node heat, column 2 empty, column 3 a
    repeat of column 0; and the powers of the three sources, likewise."""
    rng = np.random.default_rng(11)
    Pf = rng.uniform(0.0, 1e-3, (4, w.n_tri))
    nodes, cols, vals = rng.integers(0, w.n_pot, 15), rng.integers(0, 2, 15), rng.uniform(0.0, 1e-2, 15)
    Pf[2], Pf[3] = 0.0, Pf[0]
    again = cols == 0
    heat = (np.concatenate([nodes, nodes[again]]), np.concatenate([cols, np.full(again.sum(), 3)]), np.concatenate([vals, vals[again]]))
    watts = rng.uniform(0.01, 0.4, (4, 3))
    watts[2], watts[3] = 0.0, watts[0]
    return Pf, heat, watts


def heat_up(w):
    """The stacked handle with its three sources, one solve of four columns and everything read from it, twice where two
    calls must agree."""
    sources, speck_face, speck_mesh = footprints(w)
    Pf, heat, watts = loads_of(w)
    th = w.thermal(mesh_layer=w.layer_of, pairs=w.stack_pairs)
    try:
        out = dict(sources=sources, speck_face=speck_face, speck_mesh=speck_mesh, Pf=Pf, watts=watts)
        out["set"] = th.set_sources(4, w.layer_of, [layer for layer, _ in sources], [polygon for _, polygon in sources])
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
        out["links"] = th.stack_links()
        out["M"] = th.lumped(w.n_vert)
    finally:
        th.close()
    return out


@pytest.fixture(scope="module")
def heated(many):
    return heat_up(many)


def check_thermal_report(w, heated):
    theta, Pf = heated["theta"], heated["Pf"]
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
    assert np.array_equal(vert[2], w.voff[:-1]) and (top[2] == 0.0).all()         # the complete tie in every mesh
    assert (theta[2] == 0.0).all() and np.array_equal(theta[3], theta[0]) and (top[0] > 0).all()
    best, which = T.envelope(theta[:, :w.n_vert])
    assert np.array_equal(env, best) and np.array_equal(env_case, which)
    assert (env_case == 0).any() and (env_case == 1).any() and not (env_case >= 2).any()


def test_thermal_report_of_four_columns(many, heated):
    """tests/test_many_tiles.py's test of the same name on this board, with a kappa and a film of every mesh's own: face means,
    heat input and film loss (hM of the mesh's own film) bit for bit, the hotspot with its vertex exactly, in the empty column
    each mesh's first vertex; the envelope by the sequential rule."""
    check_thermal_report(many, heated)


def test_interlayer_flows(many, heated):
    """Each pad layer against layer 3.  The link slots (every pad vertex's owner among the faces of the plane and the 43 pads,
    every layer-3 vertex's owner among a thousand pads) are stack_ref.slots', bit for bit; padne_thermal_stack_flows against
    stack_ref.flows on the device's own G and theta, bit for bit: 352 meshes fold into every pair's sum, one by one."""
    w, theta = many, heated["theta"]
    flow, area = heated["flows"][0]
    assert np.array_equal(flow, heated["flows"][1][0]) and np.array_equal(area, heated["flows"][1][1])
    off, vert, owner, wt, cond = heated["links"]
    off_w, vert_w, owner_w, wt_w, cond_w = K.slots(w.flat, w.layer_of, w.stack_pairs)
    assert np.array_equal(off, off_w) and np.array_equal(vert, vert_w) and np.array_equal(owner, owner_w)
    assert np.array_equal(wt, wt_w) and np.array_equal(cond, cond_w)
    indptr, indices, data, _diag = heated["G"]
    Goff = sp.csr_matrix((data, indices.astype(np.int64), indptr.astype(np.int64)), shape=(w.n_pot, w.n_pot))
    flow_want, area_want = K.flows(w.flat, w.layer_of, w.stack_pairs, Goff, theta)
    print("flows", flow[:, 0], "area", area)
    assert np.array_equal(flow, flow_want) and np.array_equal(area, area_want)
    assert (flow[2] == 0.0).all() and (flow[0] != 0.0).all() and (area > 0.0).all()


def check_heat_sources(w, heated):
    counts, fallback, area = heated["set"]
    ptr, face = heated["lists"]
    ref = SR.Restated(w.flat, w.layer_of, heated["sources"])
    print("list lengths", counts, "fallback", fallback)
    listed = [np.unique(w.face_mesh[face[ptr[s]:ptr[s + 1]]]) for s in range(3)]
    block = sorted(w.mesh_of["pad", B.PER_ROW * j + i] for j in range(10, 15) for i in range(10, 15) if (B.PER_ROW * j + i) % 3 == 1)
    assert listed[0].tolist() == block and len(block) == 10 and np.ptp(block) > 100
    assert listed[1].tolist() == [m for m in range(w.n_mesh) if w.layer_of[m] == 3] and counts[1] == 3040 + 8 * B.N_UNDER
    assert counts[2] == 1 and np.array_equal(fallback, [0, 0, 1]) and face[ptr[2]] == heated["speck_face"]
    assert heated["speck_mesh"] > 1000
    assert np.array_equal(counts, ref.counts) and np.array_equal(fallback.astype(bool), ref.fallback)
    assert np.array_equal(ptr, ref.ptr) and np.array_equal(face, ref.face)
    assert np.array_equal(area, ref.A)
    assert [F.list_sum(w.face_area[face[ptr[s]:ptr[s + 1]]]) for s in range(3)] == list(area)
    assert np.array_equal(heated["load"], ref.load(w.n_pot, heated["watts"][:1]))
    assert abs(fsum(heated["load"]) - fsum(heated["watts"][0])) <= 1e-13 * fsum(heated["watts"][0])
    assert np.array_equal(heated["rise"][0], heated["rise"][1])
    assert np.array_equal(heated["rise"][0], ref.temperature(heated["theta"], 0.0))
    assert (heated["rise"][0][[0, 1, 3]] > 0.0).all() and (heated["rise"][0][2] == 0.0).all()


def test_heat_sources_lists_areas_loads_and_footprint_temperatures(many, heated):
    """The three footprints of ``footprints``: lists, areas, loads and footprint temperatures are sources_ref's, bit for bit."""
    check_heat_sources(many, heated)


# ---- 9. strip numbering ----------------------------------------------------------------------------------------------------------

def stamped(meshes, sigma, rows, ground, n_pot):
    """The system of element rows on global unknowns as the product stamps it (tests/helpers.py::product_system): (L, r)."""
    n_extra = sum(1 for row in rows if row[0] == "V")
    N = n_pot + n_extra + 1
    stamps, r = solver.StampList(N), np.zeros(N)
    for row in rows:
        if row[0] == "R":
            _, a, b, res = row
            g = 1 / res
            stamps.add(a, a, -g); stamps.add(a, b, g); stamps.add(b, b, -g); stamps.add(b, a, g)
        elif row[0] == "I":
            _, f, t, cur = row
            r[f] += cur
            r[t] += -cur
        else:
            _, p, n, u, iv = row
            stamps.add(iv, p, 1.0); stamps.add(iv, n, -1.0); r[iv] = u
            stamps.add(p, iv, 1.0); stamps.add(n, iv, -1.0)
            stamps.constraints.append(reduction.Constraint(index=iv, p=p, n=n, value=u))
    solver.setup_ground_node(ground, stamps, r)
    return solver.assemble_from_arrays(meshes, sigma, stamps, n_pot), r


def test_strip_numbering_on_the_device_is_the_hosts_permutation_on_a_thousand_meshes(many):
    """tests/test_gpu_parity.py::test_strip_numbering_on_the_device_is_the_hosts_permutation's pair of plans on this board, with
    voltage sources that leave 2 x 2 pads with two owners above each other (a bounding box without width: strip 0 by the rule
    both sides state), two owners side by side, three, one and none.  The device's numbering is accepted -- no refusal that
    would send solve_system to the host's -- and is the host's permutation: the reduced matrices are the same bits.
    solve_system through the device ordering agrees with the oracle's direct solve."""
    w = many
    rows, ground, pick = w.tied_rows()
    L, r = stamped(w.meshes, list(w.sigma), rows, ground, w.n_pot)
    try:
        red = reduction.build_reduction(L.layout)
        on_device = _hip.KktPlan(L.dev, w.n_pot, red.elim, red.tied, red.n_free, strip_order=True)      # (a refusal raises)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            reduction.apply_locality_ordering(red, L.xy, L.mesh_offsets)
        on_host = _hip.KktPlan(L.dev, w.n_pot, red.elim, red.tied, red.n_free, index_map=red.index_map)
        A_dev, A_host = on_device.reduced_matrix().to_scipy(), on_host.reduced_matrix().to_scipy()
        on_device.close()
        on_host.close()
        assert A_dev.shape == A_host.shape == (red.n_free, red.n_free)
        assert np.array_equal(A_dev.indptr, A_host.indptr) and np.array_equal(A_dev.indices, A_host.indices)
        assert np.array_equal(A_dev.data, A_host.data)
        v, info = quiet(solver.solve_system, L, r, reorder=True)
        Mo, ro = O.assemble_system(w.system.meshes, w.n_internal, rows, ground)
        assert np.array_equal(ro, r)
        v_ref = O.solve_system(Mo, ro)[0]
        print("strip-ordered solve against the direct solve:", np.abs(v - v_ref).max() / np.abs(v_ref).max())
        assert np.abs(v - v_ref).max() <= REL_TOL * np.abs(v_ref).max()
    finally:
        L.close()


# ---- 11. the key-field limit -------------------------------------------------------------------------------------------------------

N_CHAIN = 65_535


def chain_of_faces():
    """65 535 meshes of one face each, vertex 2 of every mesh joined to vertex 0 of the next by a resistor; 1 A through the
    whole chain, the ground at vertex 1 of the first: (meshes, sigma, rows, ground, n_pot).  (The source spans the chain so that
    the potentials are as large as the chain is long: a residual current of 1e-10 A, which the solve's stopping rule allows,
    moves a potential at the far end by the chain's 100 Ohm or so times that, whatever drives the chain.)"""
    k = np.arange(N_CHAIN, dtype=np.float64)
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    meshes = [mesh.Mesh(np.array([(2.0 * i, 0.0), (2.0 * i + 1.0, 0.0), (2.0 * i + 0.25, 1.0 + (i % 4) / 8)]), tri) for i in k]
    rows = [("R", 3 * i + 2, 3 * i + 3, 1e-3 * (1 + i % 3)) for i in range(N_CHAIN - 1)]
    rows.append(("I", 0, 3 * (N_CHAIN - 1) + 2, 1.0))
    return meshes, [2000.0 * (1 + (i % 4) / 4) for i in range(N_CHAIN)], rows, 1, 3 * N_CHAIN


def test_a_mesh_count_beyond_the_key_field_is_refused_and_ordered_on_the_host(ctx):
    """65 535 meshes do not fit the mesh field of the strip key: the plan refuses them by name, and solve_system orders the
    system on the host (the lexsort branch of reduction._strip_order) and returns the direct solve's potentials."""
    meshes, sigma, rows, ground, n_pot = chain_of_faces()
    L, r = stamped(meshes, sigma, rows, ground, n_pot)
    try:
        red = reduction.build_reduction(L.layout)
        with pytest.raises(ValueError, match="beyond the key fields"):
            _hip.KktPlan(L.dev, n_pot, red.elim, red.tied, red.n_free, strip_order=True)
        v, info = quiet(solver.solve_system, L, r, reorder=True)
        # the direct solve of the assembled matrix with two steps of refinement (tests/test_load_case_currents.py): on a chain of
        # 65 535 links a bare LU solve is itself off by several 1e-9 of the largest potential
        v_ref = refined_solves(L.tocsr(), r[:, None])[:, 0]
        print("residuals: device", info.residual_norm, "refined direct solve", np.linalg.norm(L.tocsr() @ v_ref - r))
        print("chain of faces against the direct solve:", np.abs(v - v_ref).max() / np.abs(v_ref).max())
        assert np.abs(v - v_ref).max() <= REL_TOL * np.abs(v_ref).max()
    finally:
        L.close()


# ---- 5. transient and coupled paths -------------------------------------------------------------------------------------------------

def capacities(w):
    return [3e-3 * (1 + layer) * (1 + (m % 4) / 4) for m, layer in enumerate(w.layer_of)]


def alphas(w):
    return [3.93e-3 * (1 + (m % 4) / 4) for m in range(w.n_mesh)]


def test_two_transient_steps(many):
    """tests/test_many_tiles.py's test of the same name with a capacity of every mesh's own: column 0 heats from ambient, column
    1 holds the steady state of case 1, column 2 stays off."""
    w = many
    cap_of_mesh = capacities(w)
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


def test_one_adaptive_trial_step_of_four_columns(many):
    """tests/test_many_tiles.py's test of the same name: one trial of 4 dt from ambient, node heat of 1e-2 W at one vertex per
    column -- the last vertex of the 256-vertex pad (a full tile), an inner vertex of the plane, the last vertex of the board --
    and column 3 off.  err and its vertex are fold_ref.mesh_top per mesh on the restated estimate, then the 1 100 meshes in
    ascending order; the winners are the heated vertices, in three meshes far apart in the numbering."""
    w = many
    cap_of_mesh = capacities(w)
    dt = 3e-3 / FILM_STIFF / 20
    plane = w.mesh_of["plane", 0]
    hot = np.array([w.verts(w.mesh_of["pad", 5])[1] - 1, w.verts(plane)[0] + 20 * 41 + 20, w.n_vert - 1], dtype=np.int64)
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
        print("column", c, "err", out["err"][c], "at", out["vertex"][c], "heated", hot[c] if c < 3 else None)
        assert (out["err"][c], out["vertex"][c]) == best, c
        assert (out["err"][c], out["vertex"][c]) == SD.error_of(est[c]), c
    assert np.array_equal(out["vertex"][:3], hot) and (out["err"][:3] > 0.0).all()
    assert out["err"][3] == 0.0 and not np.signbit(out["err"][3]) and out["vertex"][3] == 0


def test_scale_means_and_increment(many):
    """tests/test_many_tiles.py's test of the same name with a temperature coefficient of every mesh's own: the scales and the
    face means are coupled_ref.scale's bit for bit; the increment is the largest change of a face mean, first anywhere, then
    with the only change in the board's last face, then in a face of the 258-vertex pad."""
    w = many
    alpha = alphas(w)
    rng = np.random.default_rng(8)
    thetas = [rng.uniform(0.0, 80.0, w.n_pot)]
    bumped = (w.n_tri - 1, w.faces(w.mesh_of["pad", 600])[0] + 7)
    for f, bump in zip(bumped, (7.5, 3.25)):
        thetas.append(thetas[-1].copy())
        thetas[-1][w.tri[f]] += bump
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
        print("increment", d, "at face", at, "mesh", w.face_mesh[at])
        assert d == np.abs(mean_want - prev).max() and d > 0 and f in (None, at)
        prev = mean_want


def test_electrothermal_transient_load_and_scale_range(many):
    """tests/test_many_tiles.py's test of the same name on this board: a scale with its smallest value in the board's last face
    and its largest in a face of the plane, revalued with a temperature coefficient of every mesh's own; a slot of a reserved
    table from a block solved on the revalued system: the load is the restatement's on the block's own potentials, the per-mesh
    copper heat fold_ref's sum of the restated face powers bit for bit and the bits of padne_thermal_report's heat after
    padne_coupled_solve_kkt.  The assembled values are put back at the end (a scale of 1)."""
    w = many
    alpha, cap_of_mesh = alphas(w), capacities(w)
    rng = np.random.default_rng(9)
    s = rng.uniform(0.5, 1.5, w.n_tri)
    in_plane = w.faces(w.mesh_of["plane", 0])[0] + 1500
    s[w.n_tri - 1], s[in_plane] = 0.25, 1.75
    nodes = rng.integers(0, w.n_pot, 6)
    nodes[:2] = nodes[0]
    heat = (nodes, np.zeros(6, dtype=np.int32), rng.uniform(0.0, 1e-2, 6))
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


FILM_ORDER = (5, 64, 2, 1)                                   # knots of the table of mesh m: FILM_ORDER[m % 4]


def film_tile(w, v):
    """The global tile of film_terms_kernel that holds vertex v: the tiles are per mesh and numbered through."""
    tile0 = np.concatenate([[0], np.cumsum([tiles(n) for n in np.diff(w.voff)])])
    m = int(np.searchsorted(w.voff, v, side="right")) - 1
    return int(tile0[m]) + (int(v) - int(w.voff[m])) // 256


def beyond_of(w, tables, theta):
    """The vertices above the last knot of their mesh's table, tables of one knot left out."""
    return np.concatenate([np.flatnonzero(theta[v0:v1] > rise[-1]) + v0 for (rise, _film), (v0, v1) in
                           zip(tables, (w.verts(m) for m in range(w.n_mesh))) if len(rise) > 1] + [np.zeros(0, dtype=np.int64)])


def test_film_terms_and_the_count_above_the_last_knot_on_1107_tiles(many):
    """tests/test_many_tiles.py's film-terms test on this board, a table per mesh of 5, 64, 2 or 1 knots whose first film is the
    mesh's own: g, c, hM and the count for a theta on, beside and beyond the knots; for 1e6 everywhere; and for two vertices
    above their last knot, one in tile 256 and one in the last of the 1 107 tiles.  Two calls give the same bits and the matrix
    keeps its own."""
    w = many
    tables = TF.tables_for(w.film, FILM_ORDER)
    two = np.zeros(w.n_vert)
    m256 = next(m for m in range(w.n_mesh) if film_tile(w, w.verts(m)[0]) == 256 and len(tables[m][0]) > 1)
    last = max(m for m in range(w.n_mesh) if len(tables[m][0]) > 1)
    planted = [w.verts(m256)[0], w.verts(last)[1] - 1]
    two[planted] = 100.0
    assert film_tile(w, planted[0]) == 256 and film_tile(w, planted[1]) >= B.VERTEX_TILES - 2
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
    assert got[0][3] > 0
    assert got[1][3] == sum(w.verts(m)[1] - w.verts(m)[0] for m in range(w.n_mesh) if len(tables[m][0]) > 1)
    assert got[2][3] == 2


def test_film_increment_its_vertex_the_count_and_hM(many):
    """tests/test_many_tiles.py's film-increment test on this board: two Newton rounds by hand per heated vertex.  After every
    padne_thermal_film_increment the triple is, exactly: the largest |theta_new - theta_lin| of the device's own downloaded
    thetas, the lowest vertex that attains it, and the number of vertices above their last knot; film_ref.increment states the
    first two in the kernels' order and agrees.  The film loss of the report afterwards holds the hM the increment pass
    rewrote: fold_ref's sum of hM(theta) theta bit for bit, per mesh.  A dead load is the complete tie over 1 107 tiles."""
    w = many
    tables = TF.tables_for(w.film, FILM_ORDER)
    none = np.zeros((1, w.n_tri))
    heated_at = [(w.verts(w.mesh_of["pad", 600])[0] + 257, 0.05), (w.verts(w.mesh_of["plane", 0])[0] + 20 * 41 + 20, 0.5),
                 (w.verts(w.n_mesh - 2)[1] - 1, 0.05)]
    assert all(len(tables[int(np.searchsorted(w.voff, v, side="right")) - 1][0]) > 1 for v, _ in heated_at)      # their films are curves
    th = w.thermal()
    runs = []
    try:
        before = th.matrix().to_scipy().data.copy()
        th.set_film_curves(tables)
        M = th.lumped(w.n_vert)
        for v, watts in heated_at:
            th.film_linearise(False)
            first, res = th.solve(none, ([v], [0], [watts]))
            assert res.status == _hip.OK
            rounds = [(th.film_increment(), first[0], np.zeros(w.n_pot))]
            th.film_linearise(True)
            second, res = th.resolve()
            assert res.status == _hip.OK
            rounds.append((th.film_increment(), second[0], first[0]))
            runs.append((v, rounds, th.report(1, w.n_tri, w.n_vert, fields=False, envelope=False)[4][0]))
        th.film_linearise(False)
        cold, res = th.solve(none)
        dead = th.film_increment()
        th.set_film_curves([])
        after = th.matrix().to_scipy().data.copy()
    finally:
        th.close()
    for v, rounds, loss in runs:
        for k, (got, new, lin) in enumerate(rounds):
            moved = np.abs(new[:w.n_vert] - lin[:w.n_vert])
            above = beyond_of(w, tables, new[:w.n_vert])
            want = (float(moved.max()), int(np.argmax(moved)), len(above))
            print("heated", v, "round", k, "device", got, "host", want)
            assert want[0] > 0.0 and got == want
            assert FR.increment(w.voff, new, lin) == want[:2]
            assert want[2] == FR.terms(tables, w.voff, M, new[:w.n_vert])[3]
        theta = rounds[1][1]
        hM_want = FR.terms(tables, w.voff, M, theta[:w.n_vert])[2]
        assert not TF.same_bits(hM_want, w.hM)
        for m in range(w.n_mesh):
            v0, v1 = w.verts(m)
            terms = hM_want[v0:v1] * theta[v0:v1]
            assert loss[m] == F.mesh_sum(terms), (v, m)
            assert abs(loss[m] - fsum(terms)) <= F.fold_bound(tiles(v1 - v0), fsum(np.abs(terms))), (v, m)
    assert not cold.any() and dead == (0.0, 0, 0) and not np.signbit(dead[0])
    assert TF.same_bits(after, before)


# ---- 6. temperature sensitivities ---------------------------------------------------------------------------------------------------

def test_temperature_sensitivities_of_nine_objectives(ctx, many):
    """tests/test_many_tiles.py's test of the same name on this board, with a plan of the test's own: the owners (found among a
    thousand meshes), the right-hand sides with resistors and without, the three densities, and every per-mesh, per-pair and
    per-source sum against tests/tsens_kernel_ref.py and fold_ref bit for bit, on the device's own x, theta, lambda and mu; and
    every per-mesh sum against math.fsum of the restated terms within fold_bound.  The objective in the dead case gives zeros
    everywhere but in dT/dP_s, which does not depend on the case."""
    w = many
    sources, speck_face, _speck_mesh = footprints(w)
    plane, p5, p600, last = w.mesh_of["plane", 0], w.mesh_of["pad", 5], w.mesh_of["pad", 600], w.n_mesh - 1
    in_plane, in_first, in_last = w.faces(plane)[0] + 1500, w.faces(0)[0], w.n_tri - 1
    c0 = w.verts(plane)[0]
    objectives = [KT.point(0, 1, KT.inside_face(w.xy, w.tri, speck_face)), KT.point(1, 3, KT.inside_face(w.xy, w.tri, in_plane)),
                  KT.point(0, w.layer_of[0], KT.inside_face(w.xy, w.tri, in_first)),
                  KT.point(1, w.layer_of[last], KT.inside_face(w.xy, w.tri, in_last)), KT.listed(0, [w.verts(p5)[1] - 1], [1.0]),
                  KT.listed(1, [c0 + 10, w.verts(p600)[0] + 257, w.n_vert - 1], [0.2, 0.3, 0.5]), KT.of_source(0, 0), KT.of_source(1, 1),
                  KT.listed(2, [1000], [1.0])]
    own = [(int(row[1]), int(row[2]), float(row[3])) for _, row in w.pairs if row[0] == "R"]
    resistors = KT.with_more(own, own[0][0], 9_000, c0 + 50, w.verts(p600)[0] + 77)
    watts = np.array([[0.2, 0.1, 0.05], [0.1, 0.3, 0.02], [0.0, 0.0, 0.0]])
    with contextlib.ExitStack() as stack:
        plan, V = quiet(finished_block, w.board, w.L, solver.check_load_cases(w.prob, w.cases))
        stack.callback(plan.close)
        th = w.thermal(mesh_layer=w.layer_of, pairs=w.stack_pairs)
        stack.callback(th.close)
        th.set_sources(4, w.layer_of, [layer for layer, _ in sources], [polygon for _, polygon in sources])
        th.source_power(watts)
        theta, res = quiet(th.solve_kkt, plan, 3, rtol=solver.RTOL)
        assert res.status == _hip.OK
        indptr, indices, data, _diag = th.stack_matrix()
        out = KT.drive(ctx, th, plan, w.L, 3, w.kappa, w.layer_of, w.n_tri, objectives, resistors)
        Goff = sp.csr_matrix((data, indices.astype(np.int64), indptr.astype(np.int64)), shape=(w.n_pot, w.n_pot))
        Bd = KT.restated_board(w.flat, w.layer_of, w.sigma, w.kappa, w.hM, w.n_pot, w.L.shape[0], w.stack_pairs, Goff,
                               SR.Restated(w.flat, w.layer_of, sources))
        dev = types.SimpleNamespace(thermal=th, n_tri=w.n_tri, n_pot=w.n_pot)
        KT.check_g_through_the_solve(Bd, dev, objectives, out, watts)
    x = np.ascontiguousarray(V[:w.n_pot].T)
    assert (x[2] == 0.0).all() and (theta[2] == 0.0).all()                    # the dead case
    terms = KT.check(Bd, objectives, resistors, x, theta, out, "many")
    assert KT.orders_show(Bd, objectives, resistors, x, out)
    assert np.array_equal(out.unknown[0], w.tri[speck_face]) and np.array_equal(out.unknown[1], w.tri[in_plane])
    assert np.array_equal(out.unknown[2], w.tri[in_first]) and np.array_equal(out.unknown[3], w.tri[in_last])
    _ed, _kd, _cd, mesh_e, mesh_k = out.faces[0]
    none = np.zeros(1)
    for j, (ef, kf, ft, per) in enumerate(terms):
        for m in range(w.n_mesh):
            (lo, hi), (v0, v1) = w.faces(m), w.verts(m)
            w.sum_check(mesh_e[j, m], ef[lo:hi], none, tiles(hi - lo), f"e, objective {j}, mesh {m}")
            w.sum_check(mesh_k[j, m], kf[lo:hi], none, tiles(hi - lo), f"k, objective {j}, mesh {m}")
            w.sum_check(out.film[0][j, m], ft[v0:v1], none, tiles(v1 - v0), f"film, objective {j}, mesh {m}")
        lam = out.lam[j]
        c = T.corners(w.tri)
        mean = ((lam[c[:, 0]] + lam[c[:, 1]]) + lam[c[:, 2]]) / 3
        for s in range(3):
            mine = Bd.sources.face[Bd.sources.ptr[s]:Bd.sources.ptr[s + 1]]
            w.sum_check(out.sources[0][j, s], (w.face_area[mine] / Bd.sources.A[s]) * mean[mine], none, tiles(len(mine)),
                        f"source {s}, objective {j}")
    dead = 8
    assert not out.rhs[:, dead].any() and not out.mu[:, dead].any() and out.lam[dead].any()
    assert all(not a[dead].any() for a in out.faces[0]) and not out.film[0][dead].any() and not out.pairs[0][dead].any()
    assert (out.sources[0][dead] > 0.0).all()
    live = [j for j in range(9) if j != dead]
    # (far from an objective lambda is rounding noise of either sign: the film terms are not all negative mesh by mesh)
    assert (np.abs(mesh_e[live]) > 0).all() and (out.film[0][live] != 0).all() and (out.film[0][live].sum(axis=1) < 0).all()
    assert (out.pairs[0][live] != 0).all()


# ---- 7. sampling ----------------------------------------------------------------------------------------------------------------------

def sample_queries(b, li):
    return np.concatenate([SMP.box_points(b, li, 4000, seed=20 + li), SMP.on_edge_points(b, li, 2000, seed=30 + li)])


def test_every_centroid_is_found_in_its_face_and_its_mesh(many):
    """FieldSampler.points at every face's centroid returns that face and that mesh, for all 1 100 meshes, with the face's
    power density."""
    w = many
    sol, _rep = w.solved()[0]
    cent = (w.xy[w.tri[:, 0]] + w.xy[w.tri[:, 1]] + w.xy[w.tri[:, 2]]) / 3
    seen = 0
    with solver.FieldSampler(sol) as fs:
        for li, (lay, ls) in enumerate(zip(sol.problem.layers, sol.layer_solutions)):
            mine = [m for m in range(w.n_mesh) if w.layer_of[m] == li]
            faces = np.concatenate([np.arange(*w.faces(m)) for m in mine])
            s = fs.points(lay, cent[faces])
            assert np.array_equal(s.mesh, np.concatenate([np.full(w.faces(m)[1] - w.faces(m)[0], k) for k, m in enumerate(mine)]))
            assert np.array_equal(s.face, np.concatenate([np.arange(w.faces(m)[1] - w.faces(m)[0]) for m in mine]))
            assert np.array_equal(s.power_density, np.concatenate([tf.values for tf in ls.power_densities]))
            seen += len(mine)
    assert seen == w.n_mesh


@pytest.mark.parametrize("li", [0, 1, 2, 3])
def test_samples_are_the_restatements_through_every_index(many, li):
    """4 000 box points and 2 000 on-edge points of a layer against sampling_ref.sample, bit for bit, with inside, outside, edge
    and vertex points (500 of the layer's vertices are added for the last); the same through bins_hint 0 and 1.  The hits are
    spread over the layer's meshes: on the restatement more than 280 of the 352 pads of a pad layer, 43 of the 44 meshes of
    layer 3."""
    w = many
    sol, _rep = w.solved()[0]
    b = SMP.board_of_solution(sol)
    lay = sol.problem.layers[li]
    q = np.concatenate([sample_queries(b, li), b.xy[SMP.layer_vertices(b, li)][:500]])
    kinds = SMP.census(b, li, q)
    print(li, len(q), kinds)
    assert kinds["inside"] and kinds["outside"] and kinds["edge"] and kinds["vertex"], kinds
    face, V, J, p = SMP.sample(b, li, q)
    plain = None
    for hint in (0, 1):
        with solver.FieldSampler(sol, bins_hint=hint) as fs:
            s = fs.points(lay, q)
            st = fs.stats(lay)
        assert np.array_equal(TS.global_faces(fs, li, s), face), hint
        assert TS.same_bits(s.potential, V) and TS.same_bits(s.current_density, J) and TS.same_bits(s.power_density, p)
        assert len(np.unique(s.mesh[s.mesh >= 0])) > (40 if li == 3 else 250)
        if hint == 1:
            assert (st["bins_x"], st["bins_y"]) == (1, 1) and st["last_candidates"] == len(q) * st["faces"]
            for key in ("face", "mesh", "potential", "current_density", "power_density"):
                assert TS.same_bits(np.asarray(getattr(s, key)), np.asarray(getattr(plain, key))), key
        else:
            plain = s


def test_one_temperature_field_through_the_thermal_sampler(many):
    """One seeded field on the board's meshes through TemperatureSampler against temperature_sampling_ref.sample_fields, bit
    for bit in face, temperature and heat flux, on every layer."""
    w = many
    sol, _rep = w.solved()[0]
    b = SMP.board_of_solution(sol)
    rng = np.random.default_rng(77)
    block = rng.uniform(20.0, 95.0, size=(1, len(b.xy)))
    at, field = 0, []
    for ls in sol.layer_solutions:
        forms = []
        for msh in ls.meshes:
            zf = mesh.ZeroForm(msh)
            zf.values = block[0, at:at + len(zf.values)].copy()
            at += len(zf.values)
            forms.append(zf)
        field.append(forms)
    assert np.array_equal(TR.field_block([field]), block)
    kappa_of = {li: 0.75 + 0.5 * li for li in range(4)}
    model = solver.ThermalModel(film=1e-5, sheet_conductance={lay: kappa_of[li] for li, lay in enumerate(sol.problem.layers)})
    kappa = np.array([kappa_of[int(li)] for li in b.layer_of])
    with solver.TemperatureSampler(sol.problem, [field], model=model) as ts:
        for li, lay in enumerate(sol.problem.layers):
            q = sample_queries(b, li)[::2]
            face, T_, flux, _hot, _hf = TR.sample_fields(b, block, kappa, li, q)
            s = ts.points(lay, q, flux=True)
            assert np.array_equal(TS.global_faces(ts, li, s), face), li
            assert TS.same_bits(s.temperature, T_[:1]) and TS.same_bits(s.heat_flux, flux[:1])
            assert (face >= 0).any() and (face < 0).any()


# ---- 8. refinement --------------------------------------------------------------------------------------------------------------------

def test_refinement_behind_unflagged_meshes_and_of_every_mesh(many):
    """refine_ref bit for bit with flags on the first pad, the plane, the last pad and one 2-face pad only -- every other mesh
    comes back as it went in, and the numbering behind the unflagged meshes holds -- then with every mesh flagged."""
    w = many
    ms = [(np.asarray(m.points), np.asarray(m.triangles)) for m in w.meshes]
    two_faces = w.mesh_of["pad", 66]
    assert len(ms[two_faces][1]) == 2
    chosen = {0, w.mesh_of["plane", 0], w.n_mesh - 1, two_faces}
    flags = [np.full(len(t), m in chosen, dtype=bool) for m, (_, t) in enumerate(ms)]
    got = solver.refine_meshes(w.meshes, flags)
    RF.assert_same(got, RR.refine(ms, flags))
    for m, ((p, t), msh, par, ends) in enumerate(zip(ms, got.meshes, got.parents, got.midpoint_ends)):
        if m in chosen:
            assert len(msh.triangles) == 4 * len(t) and len(ends) > 0, m
        else:
            assert np.array_equal(msh.points, p) and np.array_equal(msh.triangles, t), m
            assert np.array_equal(par, np.arange(len(t))) and ends.shape == (0, 2)
    flags = [np.ones(len(t), dtype=bool) for _, t in ms]
    every = solver.refine_meshes(w.meshes, flags)
    RF.assert_same(every, RR.refine(ms, flags))
    RF.assert_same(solver.refine_meshes(w.meshes, flags), every)                 # two calls, the same bits
    assert sum(len(m.triangles) for m in every.meshes) == 4 * w.n_tri


# ---- 10. the mesher's batch -------------------------------------------------------------------------------------------------------------

H_MESHER = 0.25


def pad_polygons():
    """1 100 rectangles on the 3 mm pitch with sides from default_rng(3).uniform(0.3, 2.4); every third rotated about its corner
    by 0.1 (k % 7) rad; every 97th replaced by a square of 0.1 x 0.1, which yields no face."""
    rng = np.random.default_rng(3)
    polys = []
    for k in range(B.N_MESH):
        x0, y0 = B.PITCH * (k % B.PER_ROW), B.PITCH * (k // B.PER_ROW)
        a, b = rng.uniform(0.3, 2.4, 2)
        ring = GM.rect(x0, y0, x0 + a, y0 + b)
        if k % 3 == 0:
            ring = GM.rotated(ring - [x0, y0], 0.1 * (k % 7), (x0, y0))
        if k % 97 == 0:
            ring = GM.rect(x0 + 0.05, y0 + 0.05, x0 + 0.15, y0 + 0.15)
        polys.append([ring])
    return polys


@pytest.fixture(scope="module")
def pad_meshes():
    polys = pad_polygons()
    want = [GM.mesh_polygon(p, H_MESHER) for p in polys]
    return polys, want


def test_the_mesher_on_a_batch_of_1100_polygons(ctx, pad_meshes):
    """_hip.polymesh on the batch against gridmesh_ref.mesh_polygon per polygon in xy (as int64 views), tri and kind, twice as a
    batch, and for 20 of the polygons alone."""
    polys, want = pad_meshes
    n_faces = sum(len(x.tri) for x in want)
    print("faces of the batch:", n_faces)
    assert [k for k, x in enumerate(want) if len(x.tri) == 0] == list(range(0, B.N_MESH, 97)) and n_faces > 50_000
    got = _hip.polymesh(ctx, polys, H_MESHER)
    again = _hip.polymesh(ctx, polys, H_MESHER)
    assert len(got) == len(again) == B.N_MESH
    for g, a, x in zip(got, again, want):
        GMT.assert_same(g, x)
        GMT.assert_same(a, x)
    for k in list(range(0, B.N_MESH, 61)) + [97, B.N_MESH - 1]:
        (alone,) = _hip.polymesh(ctx, [polys[k]], H_MESHER)
        GMT.assert_same(alone, want[k])


def test_the_graded_mesher_on_the_batch_and_the_mesher_on_150_random_shapes(ctx, pad_meshes):
    """The same batch once through the graded entry with the first thresholds of tests/test_gridmesh_graded.py, and
    gridmesh_ref.random_shapes(1) once through the uniform entry, both against their restatements bit for bit."""
    polys, want = pad_meshes
    t = list(GGT.BATCH_THRESHOLDS[0])
    got = _hip.polymesh_graded(ctx, polys, H_MESHER, 0.25, t)
    for g, p, u in zip(got, polys, want):
        GGT.assert_same(g, GG.mesh_polygon_graded(p, H_MESHER, t, uniform=u))
    shapes = GM.random_shapes(1)
    assert len(shapes) == 150
    for g, p in zip(_hip.polymesh(ctx, shapes, H_MESHER), shapes):
        GMT.assert_same(g, GM.mesh_polygon(p, H_MESHER))


# ---- 12. the guarded allocator ----------------------------------------------------------------------------------------------------------

def test_currents_heat_sources_and_the_mesher_under_the_guarded_allocator(ctx, switches, many, pad_meshes):
    """Entries 2, 4 and 10 once under the guarded, poisoned allocator mode, through tests/test_device_memory.py's three ways: a
    block solve with the currents of the three cases and the two cuts, the stacked handle with its sources, solve and reports,
    and the batch of 1 100 polygons -- the same bits with the switch unset and under both fill bytes, and no violation."""
    w = many
    polys, _want = pad_meshes
    cases = solver.check_load_cases(w.prob, w.cases)

    def driver():
        plan, V = finished_block(w.board, w.L, cases)
        try:
            first, _second, one, _cl, _cxy = run_currents(w, plan)
        finally:
            plan.close()
        heated = heat_up(w)
        del heated["sources"]
        return [V, list(first), list(one), heated, [list(m) for m in _hip.polymesh(ctx, polys, H_MESHER)]]
    three_ways(ctx, switches, driver)

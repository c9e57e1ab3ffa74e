"""The goal-oriented error estimate on the device: the standalone entry against the host restatement (tests/goal_ref.py,
itself checked by tests/test_goal_error_host.py) and, for field 0, against ``Context.error_estimate`` bit for bit; then
``solve_meshed_goal_error`` and ``solve_meshed_goal_adaptive`` on a two-layer board with a voltmeter resistor."""
import warnings

import numpy as np
import pytest

import error_ref as R
import goal_ref as Gr
from padne_amd import mesh, problem, solver, synthetic
from padne_amd.structured import Rect, Shapes, StructuredMesher

pytestmark = pytest.mark.gpu

TOL = 1e-12                 # tests/test_error.py's: rounding relative to eta_scale, and to the product of two of them


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def quiet(fn, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        return fn(*args, **kwargs)


# ---- the standalone entry ---------------------------------------------------------------------------------------------

def grid(nx, ny, seed):
    xy, tri = synthetic.jittered_grid(nx, ny, h=0.25, seed=seed)
    return np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3)


def four_meshes(degenerate=False):
    """Meshes of 1, 256, 257 and 0 faces in one call: (xy, local tri, global tri, face_mesh, voff, toff, sigma).  The second has
    a vertex that no face uses, the third is the second's grid with one more triangle on its rim (``degenerate``: of no
    area), the fourth is a lone vertex."""
    one_xy, one_tri = np.array([[3.0, 0.0], [4.0, 0.1], [3.4, 0.9]]), np.array([[0, 1, 2]], dtype=np.int32)
    g_xy, g_tri = grid(9, 17, 5)                                       # 2 * 8 * 16 = 256 faces: exactly one tile
    assert len(g_tri) == 256
    b_xy = np.concatenate([g_xy, [[7.0, 7.0]]])                         # + a vertex used by no face
    h_xy, h_tri = grid(9, 17, 6)
    a, b = int(h_tri[0, 0]), int(h_tri[0, 1])
    apex = (h_xy[a] + h_xy[b]) / 2 if degenerate else (h_xy[a] + h_xy[b]) / 2 + [0.05, -0.21]
    c_xy = np.concatenate([h_xy, [apex]])
    c_tri = np.concatenate([h_tri, [[a, len(h_xy), b]]]).astype(np.int32)      # 257 faces: a second tile with one face
    meshes = [(one_xy, one_tri), (b_xy, g_tri), (c_xy, c_tri), (np.array([[9.0, 9.0]]), np.zeros((0, 3), dtype=np.int32))]
    voff = np.concatenate([[0], np.cumsum([len(m[0]) for m in meshes])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes])]).astype(np.int64)
    xy = np.concatenate([m[0] for m in meshes])
    local = np.concatenate([m[1] for m in meshes]).astype(np.int32)
    tri = np.concatenate([m[1].astype(np.int64) + o for m, o in zip(meshes, voff)])
    face_mesh = np.concatenate([np.full(len(m[1]), i, dtype=np.int64) for i, m in enumerate(meshes)])
    return xy, local, tri, face_mesh, voff, toff, np.array([1700.0, 30.0, 1700.0, 5.0])


def smooth_fields(xy, n_fields, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_fields):
        a, b, c = rng.uniform(0.5, 1.5, 3)
        out.append(np.exp(a * xy[:, 0] / 4) * np.cos(b * xy[:, 1]) + c * xy[:, 0] * xy[:, 1] + rng.normal(0, 0.01, len(xy)))
    return np.array(out)


@pytest.fixture(scope="module")
def standalone(ctx):
    """The four meshes with 10 fields: the device's results for 2, 4 and 10 fields, and the restatement, made once."""
    xy, local, tri, face_mesh, voff, toff, sigma = four_meshes()
    fields = smooth_fields(xy, 10)
    want = Gr.goal_flat(xy, tri, face_mesh, sigma, fields)
    got = {n: ctx.goal_error(xy, local, voff, toff, sigma, fields[:n]) for n in (2, 4, 10)}
    alone = ctx.error_estimate(xy, local, voff, toff, sigma, fields[0])
    return dict(xy=xy, local=local, tri=tri, face_mesh=face_mesh, voff=voff, toff=toff, sigma=sigma, fields=fields, want=want,
                got=got, alone=alone)


def check_against_restatement(got, want: Gr.Goal, tri, n_obj, dual_scales=None):
    """Every output of ``goal_error`` (without the power) against the restatement for its first ``n_obj`` objectives; the
    figures are printed before they are asserted.  ``dual_scales``: per objective what eta of the adjoint rounds relative to
    (default: its own eta_scale)."""
    (G, eta0, E, P, top0, face0), dual, delta, omega, m_omega, m_delta, m_top, m_face = got
    s0 = want.primal.eta_scale(tri)
    assert dual.shape == delta.shape == omega.shape == (n_obj, len(tri))
    assert (np.abs(G - want.primal.G) <= TOL * want.primal.g_around[:, None]).all()
    assert (np.abs(eta0 - want.primal.eta) <= TOL * s0).all()
    # field 0 per mesh: E relative to the sum of the faces' squared scales, P to itself, the top to the scale of its face
    n_mesh = len(want.primal.mesh_error)
    e_scale = np.bincount(want.face_mesh, weights=s0 * s0, minlength=n_mesh)
    assert (np.abs(E - want.primal.mesh_error) <= TOL * e_scale).all()
    assert (np.abs(P - want.primal.mesh_power) <= TOL * want.primal.mesh_power).all()
    for m in range(n_mesh):
        k = int(want.primal.mesh_face[m])
        if k < 0:
            assert face0[m] == -1 and top0[m] == -1.0 and E[m] == 0.0 and P[m] == 0.0
            continue
        f = int(face0[m])
        assert top0[m] == eta0[f] and abs(top0[m] - want.primal.mesh_max[m]) <= TOL * s0[k]
        assert f == k or want.primal.eta[f] >= want.primal.eta[k] - TOL * max(s0[f], s0[k])
    for j in range(n_obj):
        sj = want.duals[j].eta_scale(tri) if dual_scales is None else dual_scales[j]
        pair = s0 * sj
        tiny = 1e-300
        print("objective", j, "eta", (np.abs(dual[j] - want.eta[j]) / np.maximum(sj, tiny)).max(), "delta",
              (np.abs(delta[j] - want.delta[j]) / np.maximum(pair, tiny)).max(), "omega",
              (np.abs(omega[j] - want.omega[j]) / np.maximum(pair, tiny)).max(), "of their scales")
        assert (np.abs(dual[j] - want.eta[j]) <= TOL * sj).all()
        assert (np.abs(delta[j] - want.delta[j]) <= TOL * pair).all()
        assert (np.abs(omega[j] - want.omega[j]) <= TOL * pair).all()
        assert (np.abs(delta[j]) <= omega[j] + TOL * pair).all() and (omega[j] >= 0).all()
        # per mesh: the sums are relative to the sum of the faces' scales, the top to the scale of its face
        mesh_scale = np.bincount(want.face_mesh, weights=pair, minlength=m_omega.shape[1])
        assert (np.abs(m_omega[j] - want.mesh_omega[j]) <= TOL * mesh_scale).all()
        assert (np.abs(m_delta[j] - want.mesh_delta[j]) <= TOL * mesh_scale).all()
        for m in range(m_omega.shape[1]):
            k = int(want.mesh_face[j, m])
            if k < 0:
                assert m_face[j, m] == -1 and m_top[j, m] == -1.0 and m_omega[j, m] == 0.0 and m_delta[j, m] == 0.0
                continue
            f = int(m_face[j, m])
            assert m_top[j, m] == omega[j, f] and abs(m_top[j, m] - want.mesh_top[j, m]) <= TOL * pair[k]
            assert f == k or want.omega[j, f] >= want.omega[j, k] - TOL * max(pair[f], pair[k])


@pytest.mark.parametrize("n_fields", [2, 4, 10])
def test_standalone_entry_is_the_restatement(standalone, n_fields):
    """1, 256, 257 and 0 faces in one call, a vertex without faces, two conductances; 10 fields are two launches of 8 + 1."""
    s = standalone
    power, *rest = s["got"][n_fields]
    check_against_restatement(rest, s["want"], s["tri"], n_fields - 1)
    assert np.array_equal(power, ctx_power(s))
    # the objectives do not depend on how many ride along, chunk boundaries included
    for a, b in zip(rest[1:], s["got"][10][2:]):
        assert np.array_equal(a, b[:n_fields - 1])


def ctx_power(s):
    return solver.get_context().power_density(s["xy"], s["local"], s["voff"], s["toff"], s["sigma"], s["fields"][0])


@pytest.mark.parametrize("n_fields", [2, 4, 10])
def test_field_zero_is_the_energy_estimator_bit_for_bit(standalone, n_fields):
    got = standalone["got"][n_fields][1]
    for a, b in zip(got, standalone["alone"]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[5][3] == -1 and got[4][3] == -1.0                         # the mesh without faces
    unused = standalone["voff"][2] - 1                                    # the vertex no face uses recovers nothing
    assert not got[0][unused].any() and not got[0][-1].any()


def test_two_calls_give_the_same_bits(ctx, standalone):
    s = standalone
    again = ctx.goal_error(s["xy"], s["local"], s["voff"], s["toff"], s["sigma"], s["fields"])
    first = s["got"][10]
    assert np.array_equal(first[0], again[0])
    assert all(np.array_equal(a, b) for a, b in zip(first[1], again[1]))
    assert all(np.array_equal(a, b) for a, b in zip(first[2:], again[2:]))


def test_a_degenerate_face_gives_nan_where_the_energy_estimator_does(ctx):
    xy, local, tri, face_mesh, voff, toff, sigma = four_meshes(degenerate=True)
    fields = smooth_fields(xy, 3)
    bad = int(toff[3]) - 1                                                # the face of no area, last of the third mesh
    power, est, dual, delta, omega, m_omega, m_delta, m_top, m_face = ctx.goal_error(xy, local, voff, toff, sigma, fields)
    alone = ctx.error_estimate(xy, local, voff, toff, sigma, fields[0])
    for a, b in zip(est, alone):
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    assert np.isnan(est[1][bad]) and np.isnan(est[2][2])
    with np.errstate(all="ignore"):
        want = Gr.goal_flat(xy, tri, face_mesh, sigma, fields)
    nan0 = np.isnan(est[1])
    assert nan0.any() and not nan0[:int(toff[2])].any()                  # the other meshes are untouched
    for j in range(2):
        for got, ref in ((dual[j], want.eta[j]), (delta[j], want.delta[j]), (omega[j], want.omega[j])):
            assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(np.isnan(omega[j]), nan0)
        fine = ~nan0
        pair = want.pair_scale(tri, j)
        assert (np.abs(omega[j][fine] - want.omega[j][fine]) <= TOL * pair[fine]).all()
        assert np.isnan(m_omega[j, 2]) and np.isnan(m_delta[j, 2]) and not np.isnan(m_omega[j, :2]).any()
    again = ctx.goal_error(xy, local, voff, toff, sigma, fields)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip((dual, delta, omega, m_omega, m_top),
                                                                      (again[2], again[3], again[4], again[5], again[7])))


@pytest.mark.parametrize("nx,ny", [(5, 5), (9, 17)], ids=["one tile", "two tiles"])
def test_a_tie_on_the_top_goes_to_the_lower_face(ctx, nx, ny):
    """A mesh and its mirror image in the diagonal y = x as one mesh, the fields mirrored with it: face f and face n + f have
    the same omega, bit for bit.  (Swapping x and y swaps the two products of every cross product and the two terms of
    every sum over the components, nothing else; a mirror in x = 0 would not do, since the face gradient is a difference
    quotient towards +x.)  The top is the lower of the two faces.  32 faces put both in one tile, 256 put them in two, so
    the tie is settled once inside a tile and once in the fold."""
    xy, tri = grid(nx, ny, 9)
    n, nv = len(tri), len(xy)
    mirrored = xy[:, ::-1].copy()
    xy2 = np.concatenate([xy, mirrored])
    tri2 = np.concatenate([tri, tri + nv]).astype(np.int32)
    f = smooth_fields(xy, 2, seed=4)
    fields = np.concatenate([f, f], axis=1)
    voff, toff = np.array([0, 2 * nv], dtype=np.int64), np.array([0, 2 * n], dtype=np.int64)
    _p, est, _dual, _delta, omega, _mo, _md, m_top, m_face = ctx.goal_error(xy2, tri2, voff, toff, [2.0], fields)
    assert np.array_equal(omega[0, :n], omega[0, n:]) and np.array_equal(est[1][:n], est[1][n:])
    k = int(np.argmax(omega[0, :n]))
    assert (omega[0] == omega[0, k]).sum() == 2                            # exactly the face and its image
    assert m_face[0, 0] == k and m_top[0, 0] == omega[0, k]
    assert est[5][0] == int(np.argmax(est[1][:n]))                         # the energy estimator's own tie, likewise


def test_the_standalone_entry_refuses_what_it_cannot_do(ctx, standalone):
    s = standalone
    with pytest.raises(ValueError, match="n_fields >= 2"):
        ctx.goal_error(s["xy"], s["local"], s["voff"], s["toff"], s["sigma"], s["fields"][:1])
    with pytest.raises(ValueError, match="out of range"):
        ctx.goal_error(s["xy"], np.where(s["local"] == 2, 9999, s["local"]), s["voff"], s["toff"], s["sigma"], s["fields"][:2])
    again = ctx.goal_error(s["xy"], s["local"], s["voff"], s["toff"], s["sigma"], s["fields"][:2])      # the context still works
    assert all(np.array_equal(a, b) for a, b in zip(again[2:], s["got"][2][2:]))


# ---- the plan path: a two-layer board with a voltmeter ------------------------------------------------------------------

SIGMA = (2030.0, 1015.0)
SPOTS = dict(supply=(0.6, 1.5), via=(4.1, 1.4), load=(7.3, 1.6), probe_a=(2.3, 0.7), probe_b=(5.9, 2.4), sense=(1.8, 2.3),
             out=(6.5, 0.6))


class Board:
    """Two 8 x 3 mm layers of about 320 faces each: a 1 V source between them on the left, a 0.5 ohm via, a 0.5 A load on
    the right, and a 1 Mohm voltmeter between two probe points of the top layer.  ``regulator``: a regulator with gain 0.5
    between the layers as well, sensing on the left.  Every connection sits exactly on a vertex of the start meshes, so it
    snaps to the same vertex however the meshes are refined."""

    def __init__(self, regulator=False, size=0.4, jitter=0.1):
        layers = [problem.Layer(shape=Shapes.of(Rect(0.0, 0.0, 8.0, 3.0)), name=f"L{i}", conductance=SIGMA[i]) for i in range(2)]
        mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=size), jitter=jitter, seed=1)
        self.meshes, self.layer_of = solver.mesh_problem(problem.Problem(layers=layers, networks=[]), None, mesher)
        assert list(self.layer_of) == [0, 1]
        self.vertex = {}

        def conn(layer, spot):
            pts = self.meshes[layer].points
            v = int(np.argmin(((pts - np.asarray(SPOTS[spot])) ** 2).sum(axis=1)))
            c = problem.Connection(layer=layers[layer], point=mesh.Point(float(pts[v, 0]), float(pts[v, 1])))
            self.vertex[c.node_id] = (layer, v)
            return c
        sp, sn = conn(0, "supply"), conn(1, "supply")
        va, vb = conn(0, "via"), conn(1, "via")
        lf, lt = conn(0, "load"), conn(1, "load")
        pa, pb = conn(0, "probe_a"), conn(0, "probe_b")
        self.source = problem.VoltageSource(p=sp.node_id, n=sn.node_id, voltage=1.0)
        self.via = problem.Resistor(a=va.node_id, b=vb.node_id, resistance=0.5)
        self.load = problem.CurrentSource(f=lf.node_id, t=lt.node_id, current=0.5)
        self.meter = problem.Resistor(a=pa.node_id, b=pb.node_id, resistance=1e6)
        networks = [problem.Network(connections=[sp, sn], elements=[self.source]),
                    problem.Network(connections=[va, vb], elements=[self.via]),
                    problem.Network(connections=[lf, lt], elements=[self.load]),
                    problem.Network(connections=[pa, pb], elements=[self.meter])]
        if regulator:
            sf, st, op, on = conn(0, "sense"), conn(1, "sense"), conn(0, "out"), conn(1, "out")
            self.regulator = problem.VoltageRegulator(v_p=op.node_id, v_n=on.node_id, s_f=sf.node_id, s_t=st.node_id,
                                                      voltage=0.9, gain=0.5)
            networks.append(problem.Network(connections=[sf, st, op, on], elements=[self.regulator]))
        self.prob = problem.Problem(layers=layers, networks=networks)
        self.objectives = [(self.meter.a, self.meter.b), (self.load.f, self.load.t), (self.via.a, self.via.b)]

    def flat(self, meshes=None):
        """(xy, local tri, global tri, face_mesh, voff, toff, sigma) of the meshes, as the restatement takes them."""
        meshes = self.meshes if meshes is None else meshes
        voff = np.concatenate([[0], np.cumsum([len(m.points) for m in meshes])]).astype(np.int64)
        toff = np.concatenate([[0], np.cumsum([len(m.triangles) for m in meshes])]).astype(np.int64)
        xy = np.concatenate([m.points for m in meshes])
        local = np.concatenate([m.triangles for m in meshes]).astype(np.int32)
        tri = np.concatenate([np.asarray(m.triangles, dtype=np.int64) + o for m, o in zip(meshes, voff)])
        face_mesh = np.concatenate([np.full(len(m.triangles), i, dtype=np.int64) for i, m in enumerate(meshes)])
        return xy, local, tri, face_mesh, voff, toff, np.array(SIGMA)

    def solved_block(self, objectives):
        """(V, W) of the block solve ``solve_meshed_goal_error`` makes for ``objectives``, by the same steps: two calls give
        the same bits, so these are the V and W inside it."""
        board = solver.index_board(self.prob, self.meshes, self.layer_of)
        pairs = solver.global_elements(board.filtered_networks, board.node_indexer)
        terms = solver.woodbury_terms([row for _, row in pairs])
        idx = board.node_indexer.node_to_global_index
        rows_of = [(idx[p], idx[n]) for p, n in objectives]
        n_cols = solver.sensitivity_block_columns(len(objectives), len(terms))
        with board.assembled() as (L, _):
            rows, cols, vals = solver.stamp_sensitivity_block(board.filtered_networks, board.node_indexer, L.shape[0], rows_of, terms)
            plan, V, _norms, _res, n_tri, n_mesh = solver._solve_block_on_device(L, rows, cols, vals, n_cols, 1, solver._Laps(None))
            W = solver.adjoint_weights(V, len(objectives), terms)
            at_plan = plan.goal_error(W, n_tri, len(board.vindex), n_mesh)
            energy = plan.error_estimate(n_cols, n_tri, len(board.vindex), n_mesh)
        return np.array(V), W, terms, at_plan, energy


@pytest.fixture(scope="module")
def plain():
    return Board()


@pytest.fixture(scope="module")
def regulated():
    return Board(regulator=True)


def per_mesh(items_by_layer):
    """Per-layer, per-mesh lists of a two-layer board with one mesh each -> mesh order."""
    return [x for layer in items_by_layer for x in layer]


def goal_arrays(goals):
    """(eta, delta, omega) (k, n_tri) of a list of GoalError, faces in mesh order."""
    cat = lambda forms: np.concatenate([tf.values for tf in per_mesh(forms)])  # noqa: E731
    return (np.array([cat(g.dual_indicators) for g in goals]), np.array([cat(g.contributions) for g in goals]),
            np.array([cat(g.weights) for g in goals]))


def check_goal_call(b: Board, objectives, tolerance=None):
    """``solve_meshed_goal_error`` against the restatement on the V and W of its own block solve."""
    sol, rep, goals = quiet(solver.solve_meshed_goal_error, b.prob, b.meshes, b.layer_of, objectives, tolerance=tolerance)
    V, W, terms, at_plan, energy = quiet(b.solved_block, objectives)
    xy, _local, tri, face_mesh, voff, _toff, sigma = b.flat()
    nv = len(xy)
    x = np.concatenate([zf.values for ls in sol.layer_solutions for zf in ls.potentials])
    assert np.array_equal(x, V[:nv, 0])                                   # the block inside the call is this block
    lam = V[:nv] @ W.T
    want = Gr.goal_flat(xy, tri, face_mesh, sigma, np.concatenate([V[:nv, :1].T, lam.T]))
    # what an adjoint's eta rounds relative to: the scales of the columns it is combined from, weighted as it combines them
    col_scale = [R.estimate_flat(xy, tri, face_mesh, sigma, V[:nv, m]).eta_scale(tri) if np.abs(W[:, m]).any() else 0.0
                 for m in range(V.shape[1])]
    dual_scales = [sum(abs(W[j, m]) * col_scale[m] for m in range(V.shape[1])) for j in range(len(objectives))]
    eta, delta, omega = goal_arrays(goals)
    G = np.concatenate([-g / s for g, s in zip(per_mesh(rep.recovered), sigma)])
    eta0 = np.concatenate([tf.values for tf in per_mesh(rep.indicators)])
    E = np.array([e for e, _ in rep.layers])
    P = np.array([p for _, p in rep.layers])
    toff = np.concatenate([[0], np.cumsum([len(m.triangles) for m in b.meshes])])
    top0 = np.array([w[0] for w in rep.worst])
    face0 = np.array([toff[li] + w[2] for li, w in enumerate(rep.worst)])
    m_omega = np.array([[l[0] for l in g.layers] for g in goals])
    m_delta = np.array([[l[1] for l in g.layers] for g in goals])
    m_top = np.array([[w[0] for w in g.worst] for g in goals])
    m_face = np.array([[toff[li] + w[2] for li, w in enumerate(g.worst)] for g in goals])
    # (J* = -sigma G is divided back by sigma: one more rounding than G itself, well inside TOL)
    check_against_restatement(((G, eta0, E, P, top0, face0), eta, delta, omega, m_omega, m_delta, m_top, m_face), want, tri,
                              len(objectives), dual_scales)
    for j, (g, (p, n)) in enumerate(zip(goals, objectives)):
        assert g.nodes == (p, n) and g.tolerance == tolerance
        (lp, vp), (ln, vn) = b.vertex[p], b.vertex[n]
        assert g.value == sol.layer_solutions[lp].potentials[0].values[vp] - sol.layer_solutions[ln].potentials[0].values[vn]
        assert g.bound == sum(l[0] for l in g.layers) and g.correction == -sum(l[1] for l in g.layers)
        assert abs(g.correction) <= g.bound and g.bound > 0
        print("objective", j, "J_h", g.value, "bound", g.bound, "correction", g.correction)
        if tolerance is None:
            assert g.ratios is None
        else:
            xi = np.concatenate(per_mesh(g.ratios))
            assert np.array_equal(xi, omega[j] / (tolerance / len(tri)))
    # the plan-level entry gives the arrays the report was made from, and its field 0 is the energy estimator's on this block
    assert all(np.array_equal(a, c) for a, c in zip(at_plan[1], energy))
    assert np.array_equal(at_plan[2], eta) and np.array_equal(at_plan[3], delta) and np.array_equal(at_plan[4], omega)
    return sol, rep, goals, W, terms


def same_error_report(a, b):
    assert a.worst == b.worst and a.layers == b.layers
    assert a.power_error == b.power_error and a.estimate == b.estimate
    assert a.ratios is None and b.ratios is None and a.sizes is None and b.sizes is None and a.tolerance is None and b.tolerance is None
    for la, lb in zip(a.recovered, b.recovered):
        assert len(la) == len(lb) and all(np.array_equal(u, v) for u, v in zip(la, lb))
    for la, lb in zip(a.indicators, b.indicators):
        assert all(np.array_equal(u.values, v.values) for u, v in zip(la, lb))


def same_goals(a, b):
    assert len(a) == len(b)
    for g, h in zip(a, b):
        assert (g.value, g.bound, g.correction, g.layers, g.worst) == (h.value, h.bound, h.correction, h.layers, h.worst)
        for name in ("dual_indicators", "contributions", "weights"):
            assert all(np.array_equal(u.values, v.values) for la, lb in zip(getattr(g, name), getattr(h, name)) for u, v in zip(la, lb))


def same_solution(a, b):
    for la, lb in zip(a.layer_solutions, b.layer_solutions):
        assert all(np.array_equal(u.values, v.values) for u, v in zip(la.potentials, lb.potentials))
        assert all(np.array_equal(u.values, v.values) for u, v in zip(la.power_densities, lb.power_densities))
    assert a.solver_info.ground_node_current == b.solver_info.ground_node_current
    assert a.solver_info.residual_norm == b.solver_info.residual_norm


@pytest.mark.parametrize("k", [1, 3])
def test_goal_error_against_the_restatement_and_its_neighbours(ctx, plain, k):
    b = plain
    assert 550 <= sum(len(m.triangles) for m in b.meshes) <= 700
    objectives = b.objectives[:k]
    sol, rep, goals, W, terms = check_goal_call(b, objectives, tolerance=None if k == 1 else 1e-4)
    assert not terms and np.array_equal(W[:, 1:1 + k], np.eye(k))
    # the Solution is solve_meshed_sensitivities', bit for bit
    sens_sol, sens = quiet(solver.solve_meshed_sensitivities, b.prob, b.meshes, b.layer_of, objectives)
    same_solution(sol, sens_sol)
    assert [g.value for g in goals] == [s.value for s in sens]
    # two calls give the same bits
    sol2, rep2, goals2 = quiet(solver.solve_meshed_goal_error, b.prob, b.meshes, b.layer_of, objectives)
    same_solution(sol, sol2)
    same_error_report(rep, rep2)
    same_goals(goals, goals2)
    # the ErrorReport is solve_meshed_error's
    _sol_e, rep_e = quiet(solver.solve_meshed_error, b.prob, b.meshes, b.layer_of)
    eta_a = np.concatenate([tf.values for tf in per_mesh(rep.indicators)])
    eta_b = np.concatenate([tf.values for tf in per_mesh(rep_e.indicators)])
    print("k", k, "eta against solve_meshed_error: largest difference", np.abs(eta_a - eta_b).max(), "of", eta_b.max(),
          "; estimate", rep.estimate, rep_e.estimate)
    same_error_report(rep, rep_e)


def test_goal_error_with_a_regulator_mixes_columns(ctx, regulated):
    b = regulated
    sol, rep, goals, W, terms = check_goal_call(b, b.objectives[:2], tolerance=1e-4)
    assert len(terms) == 1 and W.shape == (2, 5)
    assert np.abs(W[:, 3:]).max() > 0                                     # Woodbury terms: an adjoint mixes columns
    sens_sol, sens = quiet(solver.solve_meshed_sensitivities, b.prob, b.meshes, b.layer_of, b.objectives[:2])
    same_solution(sol, sens_sol)
    assert [g.value for g in goals] == [s.value for s in sens]


def test_an_objective_on_one_unknown_gives_zeros(ctx, plain):
    b = plain
    twin = problem.Connection(layer=b.prob.layers[0], point=mesh.Point(*b.meshes[0].points[b.vertex[b.meter.a][1]]))
    networks = list(b.prob.networks[:3]) + [problem.Network(connections=list(b.prob.networks[3].connections) + [twin],
                                                            elements=list(b.prob.networks[3].elements))]
    prob = problem.Problem(layers=b.prob.layers, networks=networks)
    objectives = [(b.meter.a, twin.node_id), (b.meter.a, b.meter.b)]
    _sol, _rep, goals = quiet(solver.solve_meshed_goal_error, prob, b.meshes, b.layer_of, objectives, tolerance=1e-4)
    zero, other = goals
    assert zero.value == 0.0 and zero.bound == 0.0 and zero.correction == 0.0
    assert zero.layers == [(0.0, 0.0), (0.0, 0.0)]
    for forms in (zero.dual_indicators, zero.contributions, zero.weights):
        assert all(not tf.values.any() for tf in per_mesh(forms))
    assert all(not xi.any() for xi in per_mesh(zero.ratios))
    assert other.bound > 0


# ---- adaptive ---------------------------------------------------------------------------------------------------------

REASONS = {"tolerance", "floor", "rounds", "faces"}


@pytest.fixture(scope="module")
def first_bound(plain):
    _sol, _rep, goals = quiet(solver.solve_meshed_goal_error, plain.prob, plain.meshes, plain.layer_of, plain.objectives[:2])
    return max(g.bound for g in goals)


def test_goal_adaptive_loop(ctx, plain, first_bound):
    b, objectives = plain, plain.objectives[:2]
    tolerance = 0.5 * first_bound
    sol, rep, goals, history = quiet(solver.solve_meshed_goal_adaptive, b.prob, b.meshes, b.layer_of, objectives,
                                     tolerance=tolerance, max_rounds=4)
    n = len(history.faces)
    print("faces", history.faces, "bounds", history.bounds, "values", history.values, "reason", history.reason)
    assert 1 <= n <= 4 and history.reason in REASONS
    assert all(a < c for a, c in zip(history.faces, history.faces[1:]))
    assert len(history.values) == len(history.bounds) == len(history.estimates) == n
    assert all(len(v) == 2 for v in history.values) and all(len(v) == 2 for v in history.bounds)
    assert max(history.bounds[0]) == first_bound and max(history.bounds[0]) > tolerance and n >= 2
    if history.reason == "tolerance":
        assert max(history.bounds[-1]) <= tolerance
    else:
        assert max(history.bounds[-1]) > tolerance
    assert history.values[-1] == [g.value for g in goals] and history.bounds[-1] == [g.bound for g in goals]
    assert history.faces[-1] == sum(len(m.triangles) for m in history.meshes)
    # the results are the bits of solve_meshed_goal_error on history.meshes
    sol2, rep2, goals2 = quiet(solver.solve_meshed_goal_error, b.prob, history.meshes, b.layer_of, objectives, tolerance=tolerance)
    same_solution(sol, sol2)
    same_error_report(rep, rep2)
    same_goals(goals, goals2)
    assert all(np.array_equal(u, v) for g, h in zip(goals, goals2) for la, lb in zip(g.ratios, h.ratios) for u, v in zip(la, lb))


def test_goal_adaptive_budgets(ctx, plain, first_bound):
    b, objectives = plain, plain.objectives[:1]
    tolerance = 1e-3 * first_bound
    *_, history = quiet(solver.solve_meshed_goal_adaptive, b.prob, b.meshes, b.layer_of, objectives, tolerance=tolerance, max_faces=1)
    assert history.reason == "faces" and len(history.faces) == 1 and history.flagged[0] > 0 and history.meshes is not None
    assert history.faces[0] == sum(len(m.triangles) for m in b.meshes)
    *_, history = quiet(solver.solve_meshed_goal_adaptive, b.prob, b.meshes, b.layer_of, objectives, tolerance=tolerance, min_size=1e6)
    assert history.reason == "floor" and len(history.faces) == 1 and history.flagged == [0]
    *_, history = quiet(solver.solve_meshed_goal_adaptive, b.prob, b.meshes, b.layer_of, objectives, tolerance=tolerance, max_rounds=1)
    assert history.reason == "rounds" and len(history.faces) == 1 and history.flagged[0] > 0
    *_, history = quiet(solver.solve_meshed_goal_adaptive, b.prob, b.meshes, b.layer_of, objectives, tolerance=10 * first_bound)
    assert history.reason == "tolerance" and len(history.faces) == 1


@pytest.fixture(scope="module")
def regular():
    """The board on unjittered 0.5 mm squares cut into right isosceles triangles (384 faces).  Longest-edge refinement keeps
    that family (every child and every closure child is a right isosceles triangle again), so no face is ever obtuse."""
    return Board(size=0.5, jitter=0.0)


def adaptive_against_uniform(b: Board):
    """Four goal-adaptive rounds for the voltmeter's drop on ``b`` against the drop on its start meshes refined uniformly
    three times (``solve_meshed``): (distance of the start mesh's drop, distance of the last mesh's, faces of the last mesh,
    faces of the uniform meshes, the uniform meshes).  Everything is printed."""
    _sol, _rep, first = quiet(solver.solve_meshed_goal_error, b.prob, b.meshes, b.layer_of, b.objectives[:2])
    first_bound = max(g.bound for g in first)
    uniform = b.meshes
    for _ in range(3):
        uniform = solver.refine_meshes(uniform, [np.ones(len(m.triangles), dtype=bool) for m in uniform]).meshes
    ref = quiet(solver.solve_meshed, b.prob, uniform, b.layer_of)
    (la, va), (lb, vb) = b.vertex[b.meter.a], b.vertex[b.meter.b]
    for msh, (layer, v) in ((uniform[la], (la, va)), (uniform[lb], (lb, vb))):
        assert np.array_equal(msh.points[v], b.meshes[layer].points[v])    # old vertices keep their index: the probes stay put
    drop_ref = ref.layer_solutions[la].potentials[0].values[va] - ref.layer_solutions[lb].potentials[0].values[vb]
    *_, goals, history = quiet(solver.solve_meshed_goal_adaptive, b.prob, b.meshes, b.layer_of, b.objectives[:1],
                               tolerance=1e-3 * first_bound, max_rounds=4)
    assert len(history.faces) == 4 and history.reason == "rounds"
    start, final = history.values[0][0], goals[0].value
    n_uniform = sum(len(m.triangles) for m in uniform)
    print("drop: uniform x3", drop_ref, "on", n_uniform, "faces; start", start, "on", history.faces[0], "faces, off by",
          abs(start - drop_ref), "; goal-adaptive", final, "on", history.faces[-1], "faces, off by", abs(final - drop_ref),
          "; faces", history.faces, "bounds", [v[0] for v in history.bounds], "values", [v[0] for v in history.values],
          "corrections of the last round", [g.correction for g in goals])
    return abs(start - drop_ref), abs(final - drop_ref), history.faces[-1], n_uniform, uniform


def obtuse_corners(meshes) -> int:
    """Corners above 90 degrees, up to rounding."""
    count = 0
    for m in meshes:
        p = m.points[m.triangles]
        for c in range(3):
            u, v = p[:, (c + 1) % 3] - p[:, c], p[:, (c + 2) % 3] - p[:, c]
            count += int(((u * v).sum(axis=1) < -1e-9 * np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1)).sum())
    return count


def test_goal_adaptive_drop_converges_with_fewer_faces(ctx, regular):
    """The voltmeter's drop after four goal-adaptive rounds is nearer to the uniformly refined answer than the start mesh's,
    on fewer faces; no figure is asserted for how much nearer.  The board has no obtuse face and refinement makes none:
    only there is the reference's |cot| edge weight the Galerkin weight and the drop comparable across meshes (DESIGN.md,
    "Goal-oriented error", "What it does not see")."""
    off_start, off_final, faces, n_uniform, uniform = adaptive_against_uniform(regular)
    assert obtuse_corners(regular.meshes) == 0 and obtuse_corners(uniform) == 0
    assert off_final < off_start
    assert faces < n_uniform


def test_goal_adaptive_drop_on_the_jittered_board_is_measured(ctx, plain):
    """The same run on the jittered board of the other tests, where half the faces are obtuse: printed, not asserted.  The
    |cot| model's own drop differs between meshes there by more than the refinement gains (as above), so the
    last mesh may be farther from the uniform answer than the first; that limitation stays visible here."""
    off_start, off_final, faces, n_uniform, _uniform = adaptive_against_uniform(plain)
    print("jittered board:", obtuse_corners(plain.meshes), "obtuse corners at the start; off by", off_start, "->", off_final)
    assert faces < n_uniform

"""``FieldSampler`` on the device: every sample against the brute-force restatement (tests/sampling_ref.py), bit for bit and
with no point left out; against the Solution and a CurrentReport; independence of the index; rasters, lines, lifetime and
the C entries' refusals."""
import functools
import pickle
import warnings

import numpy as np
import pytest

import helpers as H
import sampling_ref as R
import sensitivity_ref as S
from padne_amd import _hip, mesh, problem, solver, synthetic

pytestmark = pytest.mark.gpu

PROBLEMS = H.problem_golden_names()
SMALL = ["unit_square", "square_with_hole", "obtuse", "star"]
WITH_HOLES = {"square_with_hole", "problem_many_meshes"}
EPS = np.finfo(np.float64).eps
KEYS = ("face", "mesh", "potential", "current_density", "power_density")


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def quiet(call, *args, **kwargs):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        return call(*args, **kwargs)


def layer(name="L0", sigma=2000.0):
    return problem.Layer(shape=H.Geoms(1), name=name, conductance=sigma)


def fed_corner_to_corner(lay, xy, current=1.5):
    lo, hi = xy.min(axis=0), xy.max(axis=0)
    a, b = problem.Connection(layer=lay, point=H.XY(*lo)), problem.Connection(layer=lay, point=H.XY(*hi))
    src = problem.CurrentSource(f=b.node_id, t=a.node_id, current=current)
    return problem.Problem(layers=[lay], networks=[problem.Network(connections=[a, b], elements=[src])])


@functools.lru_cache(maxsize=None)
def solved(name):
    """(Solution, CurrentReport or None) of a named board."""
    if name in PROBLEMS:
        system = S.problem_system(name)
        g = H.load_golden(name)
        disc = [[] for _ in system.prob.layers]
        for q in range(int(g.get("n_disc", 0))):
            disc[int(g[f"disc_layer{q}"])].append(mesh.Mesh(g[f"disc_xy{q}"], g[f"disc_tri{q}"]))
        meshes = [mesh.Mesh(xy, tri) for xy, tri, _ in system.meshes]
        return quiet(solver.solve_meshed_currents, system.prob, meshes, system.layer_of, [], disconnected_meshes_by_layer=disc)
    if name in SMALL:
        # an unknown-level fixture: its Solution is put together from the golden's own potentials and power densities
        g = H.load_golden(name)
        msh = mesh.Mesh(g["xy0"], g["tri0"])
        zf, tf = mesh.ZeroForm(msh), mesh.TwoForm(msh)
        zf.values, tf.values = np.array(g["pot0"]), np.array(g["pow0"])
        prob = problem.Problem(layers=[layer(sigma=float(g["sigma0"]))], networks=[])
        ls = solver.LayerSolution(meshes=[msh], potentials=[zf], power_densities=[tf])
        return solver.Solution(problem=prob, layer_solutions=[ls], solver_info=solver.SolverInfo(0.0, 0.0)), None
    nx, ny, seed = {"big": (240, 220, 7), "shuffled": (41, 33, 8), "grid": (23, 17, 4)}[name]
    xy, tri = synthetic.jittered_grid(nx, ny, h=0.25, seed=seed, jitter=0.2)
    if name == "shuffled":
        perm = np.random.default_rng(9).permutation(len(xy))             # new number of old vertex v: perm[v]
        xy2 = np.empty_like(xy)
        xy2[perm] = xy
        xy, tri = xy2, perm[tri].astype(np.int32)
    lay = layer()
    return quiet(solver.solve_meshed_currents, fed_corner_to_corner(lay, xy), [mesh.Mesh(xy, tri)], [0], [])


BOARDS = PROBLEMS + SMALL + ["big", "shuffled", "grid"]


def query_set(name, b, li):
    """The points of the comparison on layer li: seeded random points in the layer's box grown by 20 %, points on interior
    edges, and the vertices, edge midpoints and centroids (all of them on the small boards, a seeded share on ``big``)."""
    rng = np.random.default_rng(100 + li)
    verts, mids, cent = R.special_points(b, li)
    if name == "big":
        verts, mids, cent = (a[rng.choice(len(a), size=300, replace=False)] for a in (verts, mids, cent))
        return np.concatenate([R.box_points(b, li, 1200, seed=li + 1), R.on_edge_points(b, li, 600, seed=li + 2), verts, mids, cent])
    n_edge = 100_000 if name == "grid" else 2000                          # ``grid``: the on-edge points of the no-gaps test
    edge_seed = 11 if name == "grid" else li + 2
    on_edges = R.on_edge_points(b, li, n_edge, seed=edge_seed) if len(R.interior_edges(b, li)) else np.zeros((0, 2))
    return np.concatenate([R.box_points(b, li, 3000, seed=li + 1), on_edges, verts, mids, cent])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.isnan(a), np.isnan(b))


def global_faces(fs, li, s):
    """FieldSamples -> global face index in the sampler's flat order (-1 outside)."""
    first = fs._first_mesh[li]
    return np.where(s.mesh >= 0, fs._mto[np.clip(s.mesh + first, 0, len(fs._mto) - 1)] + s.face, -1)


@pytest.mark.parametrize("name", BOARDS)
def test_every_sample_is_the_restatements(ctx, name):
    sol, _rep = solved(name)
    b = R.board_of_solution(sol)
    with solver.FieldSampler(sol) as fs:
        for li, lay in enumerate(sol.problem.layers):
            if not len(b.faces_of(li)):
                s = fs.points(lay, [[0.0, 0.0], [1.0, 2.0]])
                assert (s.face == -1).all() and (s.mesh == -1).all() and np.isnan(s.potential).all()
                continue
            q = query_set(name, b, li)
            kinds = R.census(b, li, q)
            print(name, li, len(q), kinds)
            assert kinds["inside"] and kinds["outside"] and kinds["edge"] and kinds["vertex"], kinds
            if name in WITH_HOLES:
                assert kinds["hole"], kinds
            face, V, J, p = R.sample(b, li, q)
            s = fs.points(lay, q)
            got = global_faces(fs, li, s)
            assert np.array_equal(got, face), (np.flatnonzero(got != face)[:10], len(q))
            assert same_bits(s.potential, V) and same_bits(s.current_density, J) and same_bits(s.power_density, p)
            assert np.array_equal(s.face >= 0, face >= 0) and np.array_equal(s.mesh >= 0, face >= 0)
            assert np.isnan(s.potential[face < 0]).all() and np.isfinite(s.potential[face >= 0]).all()
            if name == "grid":                                            # no gaps on the device either
                assert (got[3000:103000] >= 0).all()
        empty = fs.points(sol.problem.layers[0], np.zeros((0, 2)))
        assert empty.face.shape == (0,) and empty.current_density.shape == (0, 2)


@pytest.mark.parametrize("name", PROBLEMS + ["big", "shuffled"])
def test_samples_are_the_solutions_and_the_reports_values(ctx, name):
    sol, rep = solved(name)
    with solver.FieldSampler(sol) as fs:
        for li, (lay, ls) in enumerate(zip(sol.problem.layers, sol.layer_solutions)):
            for mi, (msh, zf, tf) in enumerate(zip(ls.meshes, ls.potentials, ls.power_densities)):
                tri = np.asarray(msh.triangles)
                if not len(tri):
                    continue
                pts = np.asarray(msh.points)
                cent = (pts[tri[:, 0]] + pts[tri[:, 1]] + pts[tri[:, 2]]) / 3
                s = fs.points(lay, cent)
                assert (s.mesh == mi).all() and np.array_equal(s.face, np.arange(len(tri)))     # a centroid belongs to its face
                assert np.array_equal(s.power_density, tf.values)
                assert np.array_equal(s.current_density, rep.vectors[li][mi])
                # at a vertex of the owner two of the three sides are exact zeros (a factor of orient() is zero, or its two
                # products are equal), the weights are 1, 0, 0 and the sample is the corner's potential itself.  In general
                # the formula is 3 roundings per weight (two additions, a division), one per product and two additions on
                # terms of at most max |V_corner|: 6 roundings, so 8 eps max |V_corner| bounds it with room
                sv = fs.points(lay, pts)
                assert (sv.mesh == mi).all()
                corner_max = np.abs(zf.values[tri[sv.face]]).max(axis=1)
                assert (np.abs(sv.potential - zf.values) <= 8 * EPS * corner_max).all()
            every = fs.points(lay, R.box_points(R.board_of_solution(sol), li, 2000, seed=5)) if ls.meshes else None
            if every is not None:
                for k in np.flatnonzero(every.face >= 0):
                    m, f = every.mesh[k], every.face[k]
                    assert every.power_density[k] == ls.power_densities[m].values[f]
                    assert tuple(every.current_density[k]) == tuple(rep.vectors[li][m][f])


@pytest.mark.parametrize("name", BOARDS)
def test_the_index_does_not_change_an_answer(ctx, name):
    sol, _rep = solved(name)
    b = R.board_of_solution(sol)
    with solver.FieldSampler(sol) as chosen:
        stats = [chosen.stats(lay) for lay in sol.problem.layers]
    for li, st in enumerate(stats):
        assert st["faces"] == len(b.faces_of(li))
        assert st["entries"] <= 16 * st["faces"] and (st["entries"] >= st["faces"] or not st["faces"]), st
    finest = 4 * max(st["bins_x"] * st["bins_y"] for st in stats)
    layers = [li for li in range(len(stats)) if stats[li]["faces"]]
    queries = {li: np.concatenate([R.box_points(b, li, 4000, seed=20 + li), R.on_edge_points(b, li, 2000, seed=30 + li),
                                   b.xy[R.layer_vertices(b, li)][:2000]]) for li in layers}
    results = {}
    for hint in (0, 1, finest):
        # one bin: every face is a candidate of every query, so the large board sends every eighth point through it
        part = slice(None, None, 8) if (name == "big" and hint == 1) else slice(None)
        with solver.FieldSampler(sol, bins_hint=hint) as fs:
            for li in layers:
                lay, q = sol.problem.layers[li], queries[li][part]
                s, again, st = fs.points(lay, q), fs.points(lay, q), fs.stats(lay)
                assert st["last_queries"] == len(q) and (s.face >= 0).any() and (s.face < 0).any()
                if hint == 1:
                    assert (st["bins_x"], st["bins_y"]) == (1, 1) and st["last_candidates"] == len(q) * st["faces"]
                elif hint == 0:
                    results[li] = s
                    if name == "big":
                        mean = st["last_candidates"] / st["last_queries"]
                        print("big: mean candidates per query", mean, st)
                        assert st["faces"] >= 100_000 and mean < st["faces"] / 100
                else:
                    assert st["bins_x"] * st["bins_y"] > stats[li]["bins_x"] * stats[li]["bins_y"] or st["entries"] > 8 * st["faces"]
                for key in KEYS:
                    assert same_bits(getattr(s, key), getattr(again, key)), (hint, key)
                    assert same_bits(getattr(s, key), getattr(results[li], key)[part]), (li, hint, key)


@pytest.mark.parametrize("name", ["problem_many_meshes", "square_with_hole", "shuffled"])
def test_a_raster_is_its_pixel_centres(ctx, name):
    sol, _rep = solved(name)
    b = R.board_of_solution(sol)
    with solver.FieldSampler(sol) as fs:
        for li, lay in enumerate(sol.problem.layers):
            pts = b.xy[R.layer_vertices(b, li)]
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            w, h = 173, 121
            origin, pixel = lo - 0.1 * (hi - lo), (1.2 * (hi - lo)[0] / w, 1.2 * (hi - lo)[1] / h)
            img = fs.raster(lay, tuple(origin), pixel, w, h)
            centres = R.raster_points(origin[0], origin[1], pixel[0], pixel[1], w, h)
            assert img.potential.shape == (h, w) and img.current_density.shape == (h, w, 2) and img.face.shape == (h, w)
            assert np.array_equal(img.points.reshape(-1, 2), centres)
            flat = fs.points(lay, centres)
            assert (flat.face >= 0).any() and (flat.face < 0).any()
            for key in ("face", "mesh", "potential", "power_density"):
                assert same_bits(getattr(img, key).reshape(-1), getattr(flat, key)), key
            assert same_bits(img.current_density.reshape(-1, 2), flat.current_density)
            face, V, _J, _p = R.sample(b, li, centres)
            assert np.array_equal(global_faces(fs, li, flat), face) and same_bits(flat.potential, V)
            away = fs.raster(lay, tuple(hi + 1.0), 0.01, 40, 30)
            assert (away.face == -1).all() and (away.mesh == -1).all() and np.isnan(away.potential).all()
            assert np.isnan(away.current_density).all() and np.isnan(away.power_density).all()
            one = fs.raster(lay, H.XY(*(pts[0] - 0.005)), 0.01, 1, 1)        # one pixel, centred on a vertex (to rounding)
            ref = fs.points(lay, one.points.reshape(1, 2))
            assert one.face.shape == (1, 1) and same_bits(one.potential.reshape(-1), ref.potential)
            assert np.array_equal(one.face.reshape(-1), ref.face)


def test_the_profile_along_a_driven_strip(ctx):
    """The board of test_a_cut_across_a_jittered_strip_carries_the_source_current: a 10 mm x 2 mm strip driven end to end."""
    nx, ny, h = 41, 9, 0.25
    xy, tri = synthetic.jittered_grid(nx, ny, h=h, seed=1, jitter=0.2)
    lay = layer()
    left, right = xy[(ny // 2) * nx], xy[(ny // 2) * nx + nx - 1]
    cl, cr = problem.Connection(layer=lay, point=H.XY(*left)), problem.Connection(layer=lay, point=H.XY(*right))
    src = problem.CurrentSource(f=cr.node_id, t=cl.node_id, current=1.5)
    prob = problem.Problem(layers=[lay], networks=[problem.Network(connections=[cl, cr], elements=[src])])
    sol = quiet(solver.solve_meshed, prob, [mesh.Mesh(xy, tri)], [0])
    v = sol.layer_solutions[0].potentials[0].values
    with solver.FieldSampler(sol) as fs:
        prof = fs.line(lay, tuple(left), H.XY(*right), 401)
    assert np.array_equal(prof.arc_length, np.linspace(0.0, np.hypot(*(right - left)), 401))
    assert np.array_equal(prof.points[:, 0], np.linspace(left[0], right[0], 401)) and (prof.face >= 0).all()
    assert (np.diff(prof.potential) < 0).all()                            # the potential falls from left to right
    assert prof.potential[0] == v[(ny // 2) * nx] and prof.potential[-1] == v[(ny // 2) * nx + nx - 1]
    assert prof.potential[0] - prof.potential[-1] == v[(ny // 2) * nx] - v[(ny // 2) * nx + nx - 1]
    assert (prof.current_density[:, 0] > 0).all()                         # the current runs towards +x


def test_lifetime_pickles_load_cases_and_the_entries_refusals(ctx):
    system = S.problem_system("problem_mixed")
    meshes = [mesh.Mesh(xy, tri) for xy, tri, _ in system.meshes]
    prob = system.prob
    sol = quiet(solver.solve_meshed, prob, meshes, system.layer_of)
    b = R.board_of_solution(sol)
    q = [R.box_points(b, li, 500, seed=li) for li in range(len(prob.layers))]

    def answers(s):
        with solver.FieldSampler(s) as fs:
            return [fs.points(lay, q[li]) for li, lay in enumerate(s.problem.layers)]
    live = answers(sol)
    restored = answers(pickle.loads(pickle.dumps(sol)))
    for a, c in zip(live, restored):
        assert all(same_bits(getattr(a, k), getattr(c, k)) for k in KEYS) and (a.face >= 0).any()
    cases = quiet(solver.solve_meshed_load_cases, prob, meshes, system.layer_of, [{}])
    for a, c, li in zip(live, answers(cases[0]), range(len(q))):
        assert np.array_equal(a.face, c.face) and np.array_equal(a.mesh, c.mesh)
        want = R.sample(R.board_of_solution(cases[0]), li, q[li])
        assert same_bits(c.potential, want[1]) and same_bits(c.power_density, want[3])
    fs = solver.FieldSampler(sol)
    fs.close()
    with pytest.raises(ValueError, match="closed"):
        fs.points(prob.layers[0], q[0])
    with pytest.raises(ValueError, match="closed"):
        fs.raster(prob.layers[0], (0, 0), 0.1, 2, 2)
    fs.close()
    # the C entries
    lib = ctx._lib
    dev = solver.FieldSampler(sol)._dev
    n = 4
    pts = np.ascontiguousarray(q[0][:n])
    face, v, j, p = np.empty(n, np.int32), np.empty(n), np.empty((n, 2)), np.empty(n)
    F = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    args = (F(face, _hip._PI32), F(v, _hip._PF64), F(j, _hip._PF64), F(p, _hip._PF64))

    def refused(rc, match):
        assert rc == _hip.E_INVALID and match in lib.padne_last_error().decode(), (rc, lib.padne_last_error())
    refused(lib.padne_sampler_points(ctx._h, None, 0, n, F(pts, _hip._PF64), *args), "null")
    refused(lib.padne_sampler_points(ctx._h, dev._h, len(prob.layers), n, F(pts, _hip._PF64), *args), "layer out of range")
    refused(lib.padne_sampler_points(ctx._h, dev._h, -1, n, F(pts, _hip._PF64), *args), "layer out of range")
    bad = pts.copy()
    bad[2, 1] = np.inf
    refused(lib.padne_sampler_points(ctx._h, dev._h, 0, n, F(bad, _hip._PF64), *args), "finite")
    refused(lib.padne_sampler_raster(ctx._h, None, 0, 0.0, 0.0, 1.0, 1.0, 2, 2, *args), "null")
    refused(lib.padne_sampler_raster(ctx._h, dev._h, 7, 0.0, 0.0, 1.0, 1.0, 2, 2, *args), "layer out of range")
    refused(lib.padne_sampler_raster(ctx._h, dev._h, 0, 0.0, 0.0, 0.0, 1.0, 2, 2, *args), "pixel size")
    refused(lib.padne_sampler_raster(ctx._h, dev._h, 0, float("nan"), 0.0, 1.0, 1.0, 2, 2, *args), "origin")
    refused(lib.padne_sampler_raster(ctx._h, dev._h, 0, 0.0, 0.0, 1.0, 1.0, 0, 2, *args), "at least one pixel")
    refused(lib.padne_sampler_raster(ctx._h, dev._h, 0, 0.0, 0.0, 1.0, 1.0, 2 ** 14, 2 ** 13, *args), "2^26")
    counts, secs = np.zeros(6, np.int64), np.zeros(3)
    refused(lib.padne_sampler_stats(None, 0, F(counts, _hip._PI64), F(secs, _hip._PF64)), "null")
    refused(lib.padne_sampler_stats(dev._h, 9, F(counts, _hip._PI64), F(secs, _hip._PF64)), "layer out of range")
    assert lib.padne_sampler_points(ctx._h, dev._h, 0, n, F(pts, _hip._PF64), *args) == _hip.OK
    assert np.array_equal(v, live[0].potential[:n], equal_nan=True)
    assert lib.padne_sampler_destroy(None) == _hip.OK
    dev.close()
    dev.close()

"""``TemperatureSampler`` on the device: every sample of a block of fields against the brute-force restatement
(tests/temperature_sampling_ref.py) bit for bit, the electrical sampler's bits through the same kernel, rasters and their
tops, independence of the index, the steady and the transient reports end to end, the handle's lifetime, the C entries'
refusals, and a raster of 516 tiles, whose fold takes three strides."""
import functools
import types

import numpy as np
import pytest

import sampling_ref as R
import temperature_sampling_ref as TR
import test_sampling as TS
import test_thermal as TT
from padne_amd import _hip, mesh, solver

pytestmark = pytest.mark.gpu

BOARDS = ["grid", "shuffled", "square_with_hole", "problem_many_meshes"]
WITH_HOLES = {"square_with_hole", "problem_many_meshes"}
N_FIELDS = 9
same_bits = TS.same_bits


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


@functools.lru_cache(maxsize=None)
def thermal_board(name):
    """(problem, Board, the 9 fields as the reports hold them, their (9, n_vert) block, the model, kappa per mesh).  Seeded
    random fields; field 1 is constant and field 2 is field 0 again, so the first three hold both."""
    sol, _rep = TS.solved(name)
    prob = sol.problem
    b = R.board_of_solution(sol)
    rng = np.random.default_rng(77)
    block = rng.uniform(20.0, 95.0, size=(N_FIELDS, len(b.xy)))
    block[1] = 55.0
    block[2] = block[0]
    fields = []
    for row in block:
        at, fld = 0, []
        for ls in sol.layer_solutions:
            forms = []
            for msh in ls.meshes:
                zf = mesh.ZeroForm(msh)
                zf.values = row[at:at + len(zf.values)].copy()
                at += len(zf.values)
                forms.append(zf)
            fld.append(forms)
        fields.append(fld)
    assert np.array_equal(TR.field_block(fields), block)
    kappa_of = {li: 0.75 + 0.5 * li for li in range(len(prob.layers))}
    model = solver.ThermalModel(film=1e-5, sheet_conductance={lay: kappa_of[li] for li, lay in enumerate(prob.layers)})
    return prob, b, fields, block, model, np.array([kappa_of[int(li)] for li in b.layer_of])


def query_set(name, b, li):
    """As test_sampling.query_set builds them, in smaller numbers: seeded points in the layer's box grown by 20 %, points on
    interior edges, and all vertices, edge midpoints and centroids -- of a layer of more than 3000 faces a seeded share of
    400 each, as test_sampling takes of its large board, so that the brute-force restatement stays within seconds."""
    verts, mids, cent = R.special_points(b, li)
    if len(cent) > 3000:
        rng = np.random.default_rng(100 + li)
        verts, mids, cent = (a[rng.choice(len(a), size=400, replace=False)] for a in (verts, mids, cent))
    on_edges = R.on_edge_points(b, li, 600, seed=li + 2) if len(R.interior_edges(b, li)) else np.zeros((0, 2))
    return np.concatenate([R.box_points(b, li, 1500, seed=li + 1), on_edges, verts, mids, cent])


@functools.lru_cache(maxsize=None)
def reference(name, li):
    """(q, line points, the restatement at q with all 9 fields, the same along the line), computed once and left alone."""
    _prob, b, _fields, block, _model, kappa = thermal_board(name)
    q = query_set(name, b, li)
    kinds = R.census(b, li, q)
    print(name, li, len(q), kinds)
    assert kinds["inside"] and kinds["outside"] and kinds["edge"] and kinds["vertex"], kinds
    if name in WITH_HOLES:
        assert kinds["hole"], kinds
    pts = b.xy[R.layer_vertices(b, li)]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    start, end = lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo)
    line = np.stack([np.linspace(start[0], end[0], 257), np.linspace(start[1], end[1], 257)], axis=1)
    return q, (start, end, line), TR.sample_fields(b, block, kappa, li, q), TR.sample_fields(b, block, kappa, li, line)


def global_faces(ts, li, s):
    first = ts._first_mesh[li]
    return np.where(s.mesh >= 0, ts._mto[np.clip(s.mesh + first, 0, len(ts._mto) - 1)] + s.face, -1)


def layers_with_faces(prob, b):
    return [(li, lay) for li, lay in enumerate(prob.layers) if len(b.faces_of(li))]


# ---- 1. samples against the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_fields", [1, 3, 9])
@pytest.mark.parametrize("name", BOARDS)
def test_every_sample_is_the_restatements(ctx, name, n_fields):
    prob, b, fields, _block, model, _kappa = thermal_board(name)
    F = n_fields
    with solver.TemperatureSampler(prob, fields[:F], model=model) as ts:
        for li, lay in layers_with_faces(prob, b):
            q, (start, end, line), at_q, at_line = reference(name, li)
            for want, call in ((at_q, lambda **kw: ts.points(lay, q, **kw)),
                               (at_line, lambda **kw: ts.line(lay, tuple(start), tuple(end), 257, **kw))):
                face, T, flux, _hot, _hf = want
                hot, hot_field = TR.hottest_of(T[:F])
                s = call(flux=True)
                assert np.array_equal(global_faces(ts, li, s), face), np.flatnonzero(global_faces(ts, li, s) != face)[:10]
                assert s.temperature.shape == (F, len(face)) and s.heat_flux.shape == (F, len(face), 2)
                assert same_bits(s.temperature, T[:F]) and same_bits(s.heat_flux, flux[:F])
                assert same_bits(s.hottest, hot) and np.array_equal(s.hottest_field, hot_field)
                assert s.hottest_field.dtype == np.int32 and s.tops is None and s.names == list(range(F))
                assert np.isnan(s.temperature[:, face < 0]).all() and np.isfinite(s.temperature[:, face >= 0]).all()
                assert (s.hottest_field[face < 0] == -1).all() and (s.hottest_field[face >= 0] >= 0).all()
                if F >= 3:
                    assert (s.hottest_field != 2).all()                   # field 2 is field 0 again: it never takes a tie
                plain = call()
                assert plain.heat_flux is None and same_bits(plain.temperature, T[:F])
                lean = call(per_field=False)
                assert lean.temperature is None and lean.heat_flux is None
                assert np.array_equal(lean.face, s.face) and np.array_equal(lean.mesh, s.mesh)
                assert same_bits(lean.hottest, hot) and np.array_equal(lean.hottest_field, hot_field)
            assert np.array_equal(s.points, line) and s.arc_length.shape == (257,)
        empty = ts.points(prob.layers[0], np.zeros((0, 2)))
        assert empty.temperature.shape == (F, 0) and empty.hottest.shape == (0,)


# ---- 2. the electrical sampler's bits ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid", "problem_many_meshes"])
def test_a_potential_as_a_field_has_the_electrical_samplers_bits(ctx, name):
    sol, _rep = TS.solved(name)
    prob = sol.problem
    b = R.board_of_solution(sol)
    field = [ls.potentials for ls in sol.layer_solutions]
    model = solver.ThermalModel(film=1e-5, sheet_conductance={lay: float(lay.conductance) for lay in prob.layers})
    with solver.FieldSampler(sol) as fs, solver.TemperatureSampler(prob, [field], model=model) as ts:
        for li, lay in layers_with_faces(prob, b):
            q = reference(name, li)[0]
            e, t = fs.points(lay, q), ts.points(lay, q, flux=True)
            assert (e.face >= 0).any() and (e.face < 0).any()
            assert np.array_equal(e.face, t.face) and np.array_equal(e.mesh, t.mesh)
            assert same_bits(t.temperature[0], e.potential) and same_bits(t.heat_flux[0], e.current_density)
            # the handle is a field sampler's still: zero potentials, the electrical conductances
            face, v, j, p = ts._dev.points(li, q)
            assert np.array_equal(v[face >= 0], np.zeros((face >= 0).sum())) and np.isnan(v[face < 0]).all()


# ---- 3. a raster is its pixel centres --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid", "problem_many_meshes"])
def test_a_raster_is_its_pixel_centres(ctx, name):
    prob, b, fields, block, model, kappa = thermal_board(name)
    with solver.TemperatureSampler(prob, fields, model=model) as ts:
        for li, lay in layers_with_faces(prob, b):
            pts = b.xy[R.layer_vertices(b, li)]
            lo, hi = pts.min(axis=0), pts.max(axis=0)
            for w, h in ((37, 29), (300, 3)):
                origin, pixel = lo - 0.1 * (hi - lo), (1.2 * (hi - lo)[0] / w, 1.2 * (hi - lo)[1] / h)
                centres = R.raster_points(origin[0], origin[1], pixel[0], pixel[1], w, h)
                img = ts.raster(lay, tuple(origin), pixel, w, h, flux=True)
                assert img.temperature.shape == (N_FIELDS, h, w) and img.heat_flux.shape == (N_FIELDS, h, w, 2)
                assert img.hottest.shape == (h, w) and img.face.shape == (h, w) and len(img.tops) == N_FIELDS + 1
                assert np.array_equal(img.points.reshape(-1, 2), centres)
                flat = ts.points(lay, centres, flux=True)
                assert (flat.face >= 0).any() and (flat.face < 0).any()
                assert np.array_equal(img.face.reshape(-1), flat.face) and np.array_equal(img.mesh.reshape(-1), flat.mesh)
                assert same_bits(img.temperature.reshape(N_FIELDS, -1), flat.temperature)
                assert same_bits(img.heat_flux.reshape(N_FIELDS, -1, 2), flat.heat_flux)
                assert same_bits(img.hottest.reshape(-1), flat.hottest)
                assert np.array_equal(img.hottest_field.reshape(-1), flat.hottest_field)
                face, T, flux, hot, hot_field = TR.sample_fields(b, block, kappa, li, centres)
                assert np.array_equal(global_faces(ts, li, flat), face) and same_bits(flat.temperature, T)
                assert same_bits(flat.heat_flux, flux) and same_bits(flat.hottest, hot)
                want = TR.raster_tops(T, hot)
                assert None not in want and TR.tops_of(img, w) == want
                lean = ts.raster(lay, tuple(origin), pixel, w, h, per_field=False)
                assert lean.temperature is None and same_bits(lean.hottest, img.hottest) and TR.tops_of(lean, w) == want
            away = ts.raster(lay, tuple(hi + 1.0), 0.01, 40, 30)
            assert (away.face == -1).all() and (away.mesh == -1).all() and np.isnan(away.temperature).all()
            assert np.isnan(away.hottest).all() and (away.hottest_field == -1).all()
            assert away.tops == [None] * (N_FIELDS + 1)


def test_a_planted_tie_goes_to_the_lower_pixel(ctx):
    """A field of zeros is 0 at every pixel on copper -- (l_a 0 + l_b 0) + l_c 0 -- so all of them tie for its top, and the
    first of them in flat order keeps it; the raster starts beside the copper, so that pixel is not pixel 0."""
    prob, b, fields, block, model, kappa = thermal_board("grid")
    zeros = []
    for forms in fields[0]:
        zeros.append([])
        for zf in forms:
            zeros[-1].append(mesh.ZeroForm(zf.mesh))
    lo, hi = b.xy.min(axis=0), b.xy.max(axis=0)
    with solver.TemperatureSampler(prob, [fields[0], zeros, zeros], model=model) as ts:
        for w, h in ((37, 29), (300, 3)):
            origin, pixel = lo - 0.1 * (hi - lo), (1.2 * (hi - lo)[0] / w, 1.2 * (hi - lo)[1] / h)
            img = ts.raster(prob.layers[0], tuple(origin), pixel, w, h)
            on_copper = np.flatnonzero(img.face.reshape(-1) >= 0)
            assert len(on_copper) > 100 and on_copper[0] > 0
            assert (img.temperature[1].reshape(-1)[on_copper] == 0.0).all()
            tops = TR.tops_of(img, w)
            assert tops[1] == (0.0, int(on_copper[0])) and tops[2] == (0.0, int(on_copper[0]))
            assert tops == TR.raster_tops(img.temperature.reshape(3, -1), img.hottest.reshape(-1))
            # the interior vertex 195 as the centre of a single pixel: the top is that pixel
            v = b.xy[195]
            one = ts.raster(prob.layers[0], (v[0] - 0.5, v[1] - 0.5), (1.0, 1.0), 1, 1)
            assert one.face.shape == (1, 1) and one.face[0, 0] >= 0 and one.tops[0][1:3] == (0, 0)
            assert one.tops[0][0] == one.temperature[0, 0, 0] == one.hottest[0, 0]


# ---- 4. the index never changes an answer ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["grid", "square_with_hole", "problem_many_meshes"])
def test_the_index_does_not_change_an_answer(ctx, name):
    prob, b, fields, _block, model, _kappa = thermal_board(name)
    layers = layers_with_faces(prob, b)
    with solver.TemperatureSampler(prob, fields[:3], model=model) as chosen:
        stats = [chosen.stats(lay) for lay in prob.layers]
        base = {li: chosen.points(lay, reference(name, li)[0], flux=True) for li, lay in layers}
    finest = 4 * max(st["bins_x"] * st["bins_y"] for st in stats)
    for hint in (1, finest):
        with solver.TemperatureSampler(prob, fields[:3], model=model, bins_hint=hint) as ts:
            for li, lay in layers:
                q = reference(name, li)[0]
                s, st = ts.points(lay, q, flux=True), ts.stats(lay)
                assert st["last_queries"] == len(q)
                if hint == 1:
                    assert (st["bins_x"], st["bins_y"]) == (1, 1) and st["last_candidates"] == len(q) * st["faces"]
                for key in ("face", "mesh", "temperature", "heat_flux", "hottest", "hottest_field"):
                    assert same_bits(getattr(s, key), getattr(base[li], key)), (hint, li, key)


# ---- 5. and 6. end to end --------------------------------------------------------------------------------------------------

def vertex_points(forms):
    return [np.asarray(zf.mesh.points, dtype=np.float64).reshape(-1, 2) for zf in forms]


def test_end_to_end_steady_load_cases_and_their_envelope(ctx):
    prob, meshes, layer_of, disc, *_ = TT.board("two_layer")
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]
    cases = [{}, {e: 1.7 * e.current for e in sources}, {e: 0.0 for e in sources}]
    model = TT.model_of(TT.FILM_STIFF, ambient=40.0)
    _sols, reps, env = TT.quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, cases=cases,
                                disconnected_meshes_by_layer=disc)
    with solver.TemperatureSampler.of_reports(prob, reps, envelope=env, model=model) as ts, \
            solver.TemperatureSampler.of_reports(prob, reps) as cases_only:
        assert ts.names == [0, 1, 2, "envelope"] and cases_only.names == [0, 1, 2]
        for li, lay in enumerate(prob.layers):
            for mi, pts in enumerate(vertex_points(env.temperatures[li])):
                s = ts.points(lay, pts, flux=True)
                assert (s.mesh == mi).all()
                for j, rep in enumerate(reps):
                    assert np.array_equal(s.temperature[j], rep.temperatures[li][mi].values)
                assert np.array_equal(s.temperature[3], env.temperatures[li][mi].values)
                assert np.array_equal(s.hottest, env.temperatures[li][mi].values)
                c = cases_only.points(lay, pts, per_field=False)
                assert np.array_equal(c.hottest_field, env.cases[li][mi]) and c.hottest_field.dtype == np.int32
                assert np.array_equal(c.hottest, env.temperatures[li][mi].values)
                assert s.heat_flux.shape == (4, len(pts), 2) and np.isfinite(s.heat_flux).all()


def test_end_to_end_transient_snapshots_and_the_envelope(ctx):
    prob, meshes, layer_of, disc, *_ = TT.board("two_layer")
    film, cap = 1e-3, 3e-3
    model = solver.TransientModel(thermal=solver.ThermalModel(film=film, ambient=30.0), areal_capacity=cap)
    dt = cap / film / 20
    schedule = [solver.Segment(3 * dt, 3, 0), solver.Segment(2 * dt, 2, None)]
    _sols, rep = TT.quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, model, schedule, keep="segments",
                          disconnected_meshes_by_layer=disc)
    assert len(rep.snapshot_times) == 2 and len(rep.temperatures) == 2
    with solver.TemperatureSampler.of_transient(prob, rep) as ts:
        assert ts.names == list(rep.snapshot_times) + ["envelope"] and ts.n_fields == 3
        for li, lay in enumerate(prob.layers):
            for mi, pts in enumerate(vertex_points(rep.envelope.temperatures[li])):
                s = ts.points(lay, pts)
                assert (s.mesh == mi).all() and s.heat_flux is None
                for k in range(2):
                    assert np.array_equal(s.temperature[k], rep.temperatures[k][li][mi].values)
                assert np.array_equal(s.temperature[2], rep.envelope.temperatures[li][mi].values)
        with pytest.raises(ValueError, match="heat_flux needs"):
            ts.points(prob.layers[0], [[1.0, 1.0]], flux=True)


# ---- 7. replacing and removing fields ----------------------------------------------------------------------------------

def test_replacing_and_removing_fields_and_lifetime(ctx):
    prob, b, fields, block, model, kappa = thermal_board("grid")
    lay = prob.layers[0]
    q = reference("grid", 0)[0]
    ts = solver.TemperatureSampler(prob, fields[:3], model=model)
    first, again = ts.points(lay, q, flux=True), ts.points(lay, q, flux=True)
    for key in ("face", "mesh", "temperature", "heat_flux", "hottest", "hottest_field"):
        assert same_bits(getattr(first, key), getattr(again, key)), key
    dev = ts._dev
    dev.set_fields(block[3:8], kappa)                                     # another block, of another size
    face, T, flux, hot, hot_field = dev.field_points(0, q, True, True)
    want = TR.sample_fields(b, block[3:8], kappa, 0, q)
    assert np.array_equal(face, want[0]) and same_bits(T, want[1]) and same_bits(flux, want[2])
    assert same_bits(hot, want[3]) and np.array_equal(hot_field, want[4])
    dev.set_fields(block[3:8], None)                                      # without kappa: temperatures, no flux
    assert same_bits(dev.field_points(0, q, True, False)[1], want[1])
    with pytest.raises(ValueError, match="kappa"):
        dev.field_points(0, q, True, True)
    dev.set_fields(None)                                                  # n_field = 0: removed
    with pytest.raises(ValueError, match="no fields"):
        dev.field_points(0, q, False, False)
    with pytest.raises(ValueError, match="no fields"):
        dev.field_raster(0, 0.0, 0.0, 0.1, 0.1, 4, 4, False, False)
    assert np.isfinite(dev.points(0, q)[1]).any()                         # the electrical entries stay valid
    ts.close()
    with pytest.raises(ValueError, match="closed"):
        ts.points(lay, q)
    with pytest.raises(ValueError, match="closed"):
        ts.raster(lay, (0, 0), 0.1, 2, 2)
    ts.close()


# ---- 8. refusals of the C entries ------------------------------------------------------------------------------------------

def test_the_c_entries_refuse_with_nothing_written(ctx):
    prob, b, fields, block, model, kappa = thermal_board("grid")
    lib = ctx._lib
    ts = solver.TemperatureSampler(prob, fields[:3], model=model)
    dev = ts._dev
    n = 4
    pts = np.ascontiguousarray(reference("grid", 0)[0][:n])
    F = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    face, hot_field = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    T, q, hot = np.full((3, n), -7.0), np.full((3, n, 2), -7.0), np.full(n, -7.0)
    top, top_pixel = np.full(4, -7.0), np.full(4, -7, np.int64)
    outs = (F(face, _hip._PI32), F(T, _hip._PF64), F(q, _hip._PF64), F(hot, _hip._PF64), F(hot_field, _hip._PI32))
    tops = (F(top, _hip._PF64), F(top_pixel, _hip._PI64))
    xy = F(pts, _hip._PF64)

    def refused(rc, match):
        assert rc == _hip.E_INVALID and match in lib.padne_last_error().decode(), (rc, lib.padne_last_error())
        for a in (face, hot_field, T, q, hot, top, top_pixel):
            assert (a == -7).all()
    refused(lib.padne_sampler_field_points(ctx._h, None, 0, n, xy, *outs), "null")
    refused(lib.padne_sampler_field_points(ctx._h, dev._h, 1, n, xy, *outs), "layer out of range")
    refused(lib.padne_sampler_field_points(ctx._h, dev._h, -1, n, xy, *outs), "layer out of range")
    bad = pts.copy()
    bad[2, 1] = np.inf
    refused(lib.padne_sampler_field_points(ctx._h, dev._h, 0, n, F(bad, _hip._PF64), *outs), "finite")
    refused(lib.padne_sampler_field_points(ctx._h, dev._h, 0, 2 ** 26 + 1, xy, *outs), "2^26")
    refused(lib.padne_sampler_field_raster(ctx._h, None, 0, 0.0, 0.0, 1.0, 1.0, 2, 2, *outs, *tops), "null")
    refused(lib.padne_sampler_field_raster(ctx._h, dev._h, 7, 0.0, 0.0, 1.0, 1.0, 2, 2, *outs, *tops), "layer out of range")
    refused(lib.padne_sampler_field_raster(ctx._h, dev._h, 0, 0.0, 0.0, 0.0, 1.0, 2, 2, *outs, *tops), "pixel size")
    refused(lib.padne_sampler_field_raster(ctx._h, dev._h, 0, float("nan"), 0.0, 1.0, 1.0, 2, 2, *outs, *tops), "origin")
    refused(lib.padne_sampler_field_raster(ctx._h, dev._h, 0, 0.0, 0.0, 1.0, 1.0, 0, 2, *outs, *tops), "at least one pixel")
    refused(lib.padne_sampler_field_raster(ctx._h, dev._h, 0, 0.0, 0.0, 1.0, 1.0, 2 ** 14, 2 ** 13, *outs, *tops), "2^26")
    # 3 fields x 2^26 pixels is within 2^28 values; 256 fields are not (a block of 256 copies of field 0)
    refused(lib.padne_sampler_set_fields(ctx._h, None, 1, F(block, _hip._PF64), None), "null")
    refused(lib.padne_sampler_set_fields(ctx._h, dev._h, 257, F(block, _hip._PF64), None), "256")
    refused(lib.padne_sampler_set_fields(ctx._h, dev._h, -1, F(block, _hip._PF64), None), "256")
    refused(lib.padne_sampler_set_fields(ctx._h, dev._h, 2, None, None), "null")
    dev.set_fields(np.broadcast_to(block[0], (256, block.shape[1])), None)
    no_flux = (outs[0], outs[1], None, outs[3], outs[4])
    refused(lib.padne_sampler_field_raster(ctx._h, dev._h, 0, 0.0, 0.0, 1.0, 1.0, 2 ** 11, 2 ** 10, *no_flux, *tops), "2^28")
    refused(lib.padne_sampler_field_points(ctx._h, dev._h, 0, n, xy, *outs), "kappa")
    dev.set_fields(None)
    refused(lib.padne_sampler_field_points(ctx._h, dev._h, 0, n, xy, *outs), "no fields")
    refused(lib.padne_sampler_field_raster(ctx._h, dev._h, 0, 0.0, 0.0, 1.0, 1.0, 2, 2, *outs, *tops), "no fields")
    dev.set_fields(block[:3], kappa)
    assert lib.padne_sampler_field_points(ctx._h, dev._h, 0, n, xy, *outs) == _hip.OK
    want = TR.sample_fields(b, block[:3], kappa, 0, pts)
    assert np.array_equal(face, want[0]) and same_bits(T, want[1]) and same_bits(q, want[2]) and same_bits(hot, want[3])
    ts.close()


# ---- 9. a raster of several hundred tiles --------------------------------------------------------------------------------------

LARGE_W, LARGE_H = 300, 440                                  # 132 000 pixels: 516 tiles, lanes 0-3 of the fold take three strides
LARGE_PIXEL = (0.0216, 0.0087)
LARGE_FIRST_ROW, LARGE_FIRST_COL, LARGE_ROW_ON_COPPER = 46, 25, 255


def forms_like(template, value_of):
    """A field on the meshes of ``template`` (per layer, per mesh a ZeroForm) with the values ``value_of(points (n, 2))``."""
    out = []
    for forms in template:
        out.append([])
        for zf in forms:
            new = mesh.ZeroForm(zf.mesh)
            new.values = np.asarray(value_of(np.asarray(zf.mesh.points, dtype=np.float64).reshape(-1, 2)), dtype=np.float64).copy()
            out[-1].append(new)
    return out


@pytest.fixture(scope="module")
def large_raster(ctx):
    """The ``grid`` board (704 faces on [0, 5.5] x [0, 4]) under four fields -- the seeded random one, zeros, the vertices' y
    and minus that -- and a raster of 300 x 440 pixels that starts 10 % of the copper's extent outside it at the left and the
    bottom, ends outside it at the right and inside it at the top.  Pixels of 0.0216 x 0.0087 put the first row on copper at
    row 46 with its 255 pixels on copper in columns 25 .. 279: pixels 13 825 .. 14 079, all of them in tile 54 (13 824 ..
    14 079), so the first tile that has copper holds the whole lowest row of it.  Everything is sampled once."""
    prob, b, fields, _block, model, _kappa = thermal_board("grid")
    mine = [fields[0], forms_like(fields[0], lambda p: np.zeros(len(p))), forms_like(fields[0], lambda p: p[:, 1]),
            forms_like(fields[0], lambda p: -p[:, 1])]
    lo, hi = b.xy.min(axis=0), b.xy.max(axis=0)
    assert np.array_equal(lo, [0.0, 0.0]) and np.array_equal(hi, [5.5, 4.0])
    origin = lo - 0.1 * (hi - lo)
    lay = prob.layers[0]
    with solver.TemperatureSampler(prob, mine, model=model) as ts:
        img = ts.raster(lay, tuple(origin), LARGE_PIXEL, LARGE_W, LARGE_H)
        lean = ts.raster(lay, tuple(origin), LARGE_PIXEL, LARGE_W, LARGE_H, per_field=False)
        centres = R.raster_points(origin[0], origin[1], LARGE_PIXEL[0], LARGE_PIXEL[1], LARGE_W, LARGE_H)
        flat = ts.points(lay, centres)
        away = ts.raster(lay, tuple(hi + 1.0), LARGE_PIXEL, LARGE_W, LARGE_H)
        faces = global_faces(ts, 0, flat)
    return types.SimpleNamespace(b=b, block=TR.field_block(mine), img=img, lean=lean, centres=centres, flat=flat, away=away, faces=faces)


def test_a_large_raster_lies_where_its_tiles_are_meant_to(large_raster):
    """What makes the tests below reach the second and third stride of sample_fields_fold_kernel, from the image's own faces:
    516 tiles; whole leading tiles off the copper; the first pixel on copper where the fixture says, its row's copper inside one
    tile; copper in each of the tiles 512 .. 515; more than 100 000 pixels on copper."""
    face = large_raster.img.face.reshape(-1)
    assert len(face) == 132_000 and -(-len(face) // 256) == 516
    on_copper = np.flatnonzero(face >= 0)
    first = LARGE_FIRST_ROW * LARGE_W + LARGE_FIRST_COL
    assert on_copper[0] == first and first // 256 == 54 and (face[:54 * 256] < 0).all()
    row = face[LARGE_FIRST_ROW * LARGE_W:(LARGE_FIRST_ROW + 1) * LARGE_W]
    assert np.array_equal(np.flatnonzero(row >= 0), LARGE_FIRST_COL + np.arange(LARGE_ROW_ON_COPPER))
    assert (first + LARGE_ROW_ON_COPPER - 1) // 256 == 54
    assert all((face[t * 256:(t + 1) * 256] >= 0).any() for t in (512, 513, 514, 515))
    assert (face[-LARGE_W:] >= 0).any() and (face[-LARGE_W:] < 0).any()        # the top row: inside the copper, beyond it at both sides
    assert len(on_copper) > 100_000


def test_the_tops_of_a_large_raster(large_raster):
    """All five slots against np.nanmax with the lowest pixel on the device's own temperatures.  The field of zeros ties on
    every pixel on copper, across all three strides, and keeps the first one; the vertices' y peaks in the top row, in a tile
    of the third stride; minus y in the first tile that has copper; the hottest slot is the sequential rule's; without the
    per-field arrays the same tops and the same bits of ``hottest``."""
    img, lean = large_raster.img, large_raster.lean
    T, hot = img.temperature.reshape(4, -1), img.hottest.reshape(-1)
    on_copper = np.flatnonzero(img.face.reshape(-1) >= 0)
    tops = TR.tops_of(img, LARGE_W)
    print("tops", tops, "tiles", [top[1] // 256 for top in tops])
    assert len(tops) == 5 and None not in tops
    assert tops == TR.raster_tops(T, hot)
    assert (T[1][on_copper] == 0.0).all() and tops[1] == (0.0, int(on_copper[0])) and not np.signbit(tops[1][0])
    assert tops[2][1] // 256 >= 512 and tops[2][1] // LARGE_W == LARGE_H - 1
    assert tops[3][1] // 256 == on_copper[0] // 256 and tops[3][1] // LARGE_W == LARGE_FIRST_ROW
    want_hot, want_field = TR.hottest_of(T)
    assert same_bits(hot, want_hot) and np.array_equal(img.hottest_field.reshape(-1), want_field)
    assert tops[4] == TR.raster_tops(T, want_hot)[4] and tops[4][0] == max(top[0] for top in tops[:4])
    assert lean.temperature is None and same_bits(lean.hottest, img.hottest) and TR.tops_of(lean, LARGE_W) == tops
    assert np.array_equal(lean.hottest_field, img.hottest_field) and np.array_equal(lean.face, img.face)


def test_a_large_raster_is_its_pixel_centres(large_raster):
    """Every array of the image against the point query at sampling_ref.raster_points: the centres formed from idx / width on
    the device are the stated expression's up to the last pixel."""
    img, flat, centres = large_raster.img, large_raster.flat, large_raster.centres
    assert np.array_equal(img.points.reshape(-1, 2), centres)
    assert np.array_equal(img.face.reshape(-1), flat.face) and np.array_equal(img.mesh.reshape(-1), flat.mesh)
    assert same_bits(img.temperature.reshape(4, -1), flat.temperature)
    assert same_bits(img.hottest.reshape(-1), flat.hottest)
    assert np.array_equal(img.hottest_field.reshape(-1), flat.hottest_field)


def test_a_large_raster_against_the_restatement_on_a_subset(large_raster):
    """Brute force over all 704 faces at every pixel of the tiles 0, 255, 256, 511, 512 and 515 and at every 61st pixel of the
    rest (the whole image takes the restatement longer than a test may)."""
    r = large_raster
    n = LARGE_W * LARGE_H
    tile = np.arange(n) // 256
    pick = np.isin(tile, (0, 255, 256, 511, 512, 515))
    pick[np.flatnonzero(~pick)[::61]] = True
    at = np.flatnonzero(pick)
    face, T, _flux, hot, hot_field = TR.sample_fields(r.b, r.block, None, 0, r.centres[at])
    print("pixels compared", len(at), "on copper", int((face >= 0).sum()))
    assert len(at) >= 3000 and (face >= 0).sum() > 1000 and (face < 0).sum() > 300
    assert np.array_equal(r.faces[at], face) and np.array_equal(r.img.face.reshape(-1)[at] >= 0, face >= 0)
    assert same_bits(r.img.temperature.reshape(4, -1)[:, at], T)
    assert same_bits(r.img.hottest.reshape(-1)[at], hot) and np.array_equal(r.img.hottest_field.reshape(-1)[at], hot_field)


def test_a_large_raster_off_the_copper_has_no_tops(large_raster):
    away = large_raster.away
    assert away.face.shape == (LARGE_H, LARGE_W) and (away.face == -1).all() and (away.mesh == -1).all()
    assert np.isnan(away.temperature).all() and np.isnan(away.hottest).all() and (away.hottest_field == -1).all()
    assert away.tops == [None] * 5                           # every one of the 516 tile tops of every slot is the empty top

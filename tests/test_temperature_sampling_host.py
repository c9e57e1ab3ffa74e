"""The temperature sampler without a device: the restatement (tests/temperature_sampling_ref.py) against the truth of a
linear field, its ``hottest`` and ``tops`` rules, every refusal of ``TemperatureSampler`` before the device, and the
exports."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import helpers as H
import sampling_ref as R
import temperature_sampling_ref as TR
from padne_amd import _hip, build, mesh, problem, solver, synthetic

EPS = np.finfo(np.float64).eps
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_board(kappa=3.5):
    xy, tri = synthetic.jittered_grid(23, 17, h=0.25, seed=4, jitter=0.2)
    return R.board([(xy, tri, kappa, 0)], [np.zeros(len(xy))])


# ---- the restatement against truth ---------------------------------------------------------------------------------

def test_a_linear_field_and_its_flux_are_reproduced():
    """T = alpha + beta x + gamma y, sampled by the restatement, against the field evaluated in rational arithmetic.

    The temperature.  The weights are l_k = o_k / s with s = (o_a + o_b) + o_c: two sums and a quotient each, so they add up
    to 1 within 3 eps whatever the sides' own rounding is.  Then three products and two sums on terms of at most
    max |T_corner| =: Tmax: 3 + 1 + 2 = 6 roundings on a sum of terms l_k T_k that add up to at most Tmax, taken as 8 eps
    Tmax like test_sampling's vertex bound.  The corner values are themselves rounded: two products and two sums on terms
    that add up to M = |alpha| + |beta| max |x| + |gamma| max |y|, 4 eps M.  What is left is the rounding of the sides o_k:
    orient() is two differences, a product (twice) and a difference, off by at most 8 eps S^2 with S the longest edge of the
    face; because the weights still add up to 1, such an error moves the sample only along the face's own spread of T, at
    most (|beta| + |gamma|) S: 6 * 8 eps (S^2 / 2A) (|beta| + |gamma|) S, with S^2 / 2A the worst shape of the mesh.

    The flux.  interp() forms l_1, l_2 as (sum of two products of differences) / D and l_3 = 1 - l_1 - l_2, at the points
    (x_1 + 1, y_1) and (x_1, y_1 + 1).  With N_k the same expressions on absolute values (>= |l_k|), N_D the same for D
    (>= 1) and Lambda = N_1 + N_2 + (1 + N_1 + N_2) >= sum |l_k|: a numerator and D carry 4 roundings each and the quotient
    one, |dl_k| <= 9 eps N_k N_D for k = 1, 2, l_3 inherits both and adds two roundings; three products, two sums and the
    final difference add 4 eps Lambda Tmax, the corners' rounding 4 eps M Lambda.  In all eps N_D Lambda (24 Tmax + 4 M) on
    the gradient, times kappa, and one rounding of the product with kappa."""
    kappa = 3.5
    b = grid_board(kappa)
    alpha, beta, gamma = 41.0, -2.75, 1.625
    field = alpha + beta * b.xy[:, 0] + gamma * b.xy[:, 1]
    q = np.concatenate([R.box_points(b, 0, 4000, seed=3, grow=0.1), R.on_edge_points(b, 0, 500, seed=5)])
    face, T, flux, hot, hot_field = TR.sample_fields(b, field[None, :], [kappa], 0, q)
    inside = face >= 0
    assert inside.sum() > 3000 and (~inside).sum() > 100
    fa, fb, fg = Fraction(alpha), Fraction(beta), Fraction(gamma)
    want = np.array([float(fa + fb * Fraction(x) + fg * Fraction(y)) for x, y in q[inside].tolist()])
    exact_err = np.array([abs(Fraction(t) - (fa + fb * Fraction(x) + fg * Fraction(y)))
                          for t, (x, y) in zip(T[0, inside].tolist(), q[inside].tolist())], dtype=object)
    t = b.tri
    P = b.xy[t]                                                         # (n_tri, 3, 2)
    edges = np.stack([np.hypot(*(P[:, k] - P[:, (k + 1) % 3]).T) for k in range(3)], axis=1)
    S = edges.max(axis=1)
    area2 = np.abs(R.orient(P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1], P[:, 2, 0], P[:, 2, 1]))
    shape = (S * S / area2).max()
    Tmax = np.abs(field).max()
    M = abs(alpha) + abs(beta) * np.abs(b.xy[:, 0]).max() + abs(gamma) * np.abs(b.xy[:, 1]).max()
    bound = EPS * (8 * Tmax + 4 * M + 48 * shape * (abs(beta) + abs(gamma)) * S.max())
    print("temperature: worst error", float(max(exact_err)), "bound", bound, "shape", shape)
    assert max(exact_err) <= bound
    assert np.abs(T[0, inside] - want).max() <= bound + EPS * Tmax
    assert np.isnan(T[0, ~inside]).all() and np.isnan(flux[0, ~inside]).all()
    # the flux, face by face (it is the owner's face value)
    x1, y1, x2, y2, x3, y3 = P[:, 2, 0], P[:, 2, 1], P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1]
    D = np.abs((y2 - y3) * (x1 - x3) + (x3 - x2) * (y1 - y3))
    ND = (np.abs(y2 - y3) * np.abs(x1 - x3) + np.abs(x3 - x2) * np.abs(y1 - y3)) / D
    worst = 0.0
    for px, py in ((x1 + 1, y1), (x1, y1 + 1)):
        N1 = (np.abs(y2 - y3) * np.abs(px - x3) + np.abs(x3 - x2) * np.abs(py - y3)) / D
        N2 = (np.abs(y3 - y1) * np.abs(px - x3) + np.abs(x1 - x3) * np.abs(py - y3)) / D
        worst = max(worst, (ND * (N1 + N2 + (1 + N1 + N2))).max())
    flux_bound = kappa * (EPS * worst * (24 * Tmax + 4 * M) + 2 * EPS * max(abs(beta), abs(gamma)))
    err = np.abs(flux[0, inside] - np.array([-kappa * beta, -kappa * gamma])).max()
    print("flux: worst error", err, "bound", flux_bound)
    assert err <= flux_bound
    assert np.array_equal(hot[inside], T[0, inside]) and (hot_field[inside] == 0).all()


def test_at_every_vertex_the_sample_is_the_vertex_value():
    b = grid_board()
    rng = np.random.default_rng(21)
    fields = rng.uniform(20.0, 90.0, size=(3, len(b.xy)))
    face, T, _flux, _hot, _hf = TR.sample_fields(b, fields, None, 0, b.xy)
    assert (face >= 0).all() and _flux is None
    assert np.array_equal(T, fields)                                    # by bits: the weights are 1, 0, 0


# ---- hottest and tops --------------------------------------------------------------------------------------------------

def test_hottest_ties_go_to_the_lowest_field_and_outside_is_nan():
    b = grid_board()
    rng = np.random.default_rng(22)
    base = rng.uniform(20.0, 90.0, size=len(b.xy))
    other = rng.uniform(20.0, 90.0, size=len(b.xy))
    partly = other.copy()
    left = b.xy[:, 0] < b.xy[:, 0].mean()
    partly[left] = base[left]                                           # equal to field 0 on the left part of the board
    q = np.concatenate([R.box_points(b, 0, 3000, seed=6), b.xy])
    face, T, _f, hot, hot_field = TR.sample_fields(b, np.stack([base, base, partly]), None, 0, q)
    inside = face >= 0
    assert inside.any() and (~inside).any()
    assert np.array_equal(T[0], T[1], equal_nan=True)
    assert np.isnan(hot[~inside]).all() and (hot_field[~inside] == -1).all()
    assert (hot_field[inside] != 1).all()                               # the twin of field 0 never takes a tie
    equal = inside & (T[2] == T[0])
    assert equal.sum() > 100 and (hot_field[equal] == 0).all()          # ... nor does the field that is equal in part
    greater = inside & (T[2] > T[0])
    assert greater.sum() > 100 and (hot_field[greater] == 2).all() and np.array_equal(hot[greater], T[2][greater])
    assert np.array_equal(hot[inside], np.max(T[:, inside], axis=0))
    two = TR.hottest_of(np.array([[1.0, 2.0, np.nan], [1.0, 3.0, np.nan], [1.0, 3.0, np.nan]]))
    assert two[0].tolist()[:2] == [1.0, 3.0] and np.isnan(two[0][2]) and two[1].tolist() == [0, 1, -1]


def test_tops_of_a_raster():
    b = grid_board()
    rng = np.random.default_rng(23)
    fields = rng.uniform(20.0, 90.0, size=(2, len(b.xy)))
    hi = b.xy.max(axis=0)
    beside = R.raster_points(hi[0] + 1.0, hi[1] + 1.0, 0.1, 0.1, 3, 2)  # 3 x 2 pixels wholly beside the copper
    face, T, _f, hot, _hf = TR.sample_fields(b, fields, None, 0, beside)
    assert (face == -1).all() and TR.raster_tops(T, hot) == [None, None, None]
    # a planted tie: the same value at two pixels goes to the lower flat index, also where a NaN lies before it
    T = np.array([[np.nan, 3.0, 7.0, 5.0, 7.0, np.nan], [np.nan, 9.0, 1.0, 9.0, 2.0, np.nan]])
    hot, _ = TR.hottest_of(T)
    assert TR.raster_tops(T, hot) == [(7.0, 2), (9.0, 1), (9.0, 1)]
    # ... and on the board: two pixels centred on two vertices that are given the one largest value
    lo = b.xy.min(axis=0)
    pts = R.raster_points(lo[0], lo[1], 0.3, 0.3, 9, 7)
    face, T, _f, hot, _hf = TR.sample_fields(b, fields, None, 0, pts)
    tops = TR.raster_tops(T, hot)
    for (value, pixel), row in zip(tops, list(T) + [hot]):
        assert value == np.nanmax(row) and row[pixel] == value and not (row[:pixel] == value).any()


# ---- refusals ----------------------------------------------------------------------------------------------------------

class Unreachable:
    """Stands where ``_hip.Sampler`` is and cannot even be made."""

    def __init__(self, *_a, **_k):
        raise AssertionError("the device was reached")


class FieldsOnly:
    """Stands where ``_hip.Sampler`` is: it can be made and given fields, but nothing may be asked of it."""

    def __init__(self, *_a, **_k):
        pass

    def __getattr__(self, name):
        if name in ("close", "set_fields"):
            return lambda *_a, **_k: None
        raise AssertionError("the device was reached")


def small_problem():
    top = problem.Layer(shape=H.Geoms(1), name="F.Cu", conductance=2.0)
    bottom = problem.Layer(shape=H.Geoms(1), name="B.Cu", conductance=1.0)
    prob = problem.Problem(layers=[top, bottom], networks=[])
    xy, tri = synthetic.jittered_grid(5, 4, h=0.5, seed=1, jitter=0.1)
    meshes = [mesh.Mesh(xy, tri), mesh.Mesh(xy + 0.25, tri)]
    return prob, meshes


def field_on(meshes, value=30.0):
    out = []
    for k, msh in enumerate(meshes):
        zf = mesh.ZeroForm(msh)
        zf.values = np.full(len(np.asarray(msh.points)), value + k)
        out.append([zf])
    return out


def no_device(monkeypatch, stub):
    def reached(*_a, **_k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(solver, "get_context", lambda: None)
    monkeypatch.setattr(_hip, "Context", reached)
    monkeypatch.setattr(_hip, "load_library", reached)
    monkeypatch.setattr(_hip, "Sampler", stub)


def test_fields_are_refused_before_the_device(monkeypatch):
    no_device(monkeypatch, Unreachable)
    prob, meshes = small_problem()
    good = field_on(meshes)

    def refused(match, fields, **kw):
        with pytest.raises(ValueError, match=match):
            solver.TemperatureSampler(prob, fields, **kw)
    xy, tri = synthetic.jittered_grid(5, 4, h=0.5, seed=2, jitter=0.1)
    other = field_on([meshes[0], mesh.Mesh(xy, tri)])
    refused(r"field 1, layer 1, mesh 0: another mesh", [good, other])
    refused(r"field 'later', layer 1, mesh 0: another mesh", [good, other], names=["now", "later"])
    short = field_on(meshes)
    short[0][0].values = short[0][0].values[:-1]
    refused(r"field 1, layer 0, mesh 0: 19 values for 20 vertices", [good, short])
    refused(r"field 0, layer 0, mesh 0: 19 values for 20 vertices", [short])
    nan = field_on(meshes)
    nan[1][0].values[3] = np.nan
    refused(r"field 2, layer 1, mesh 0: the values are not finite", [good, good, nan])
    refused(r"field 1 is None.*per_case_fields=False", [good, None])
    refused(r"0 fields", [])
    refused(r"257 fields", [good] * 257)
    refused(r"field 1 has 1 layers", [good, good[:1]])
    refused(r"field 1, layer 0: 2 meshes", [good, [good[0] + good[0], good[1]]])
    refused(r"2 names for 1 fields", [good], names=["a", "b"])
    refused(r"not a ZeroForm", [[[np.zeros(20)], good[1]]])
    # an equal copy of the mesh is the same mesh
    copies = field_on([mesh.Mesh(np.array(m.points), np.array(m.triangles)) for m in meshes])
    monkeypatch.setattr(_hip, "Sampler", FieldsOnly)
    solver.TemperatureSampler(prob, [good, copies]).close()
    assert solver.MAX_SAMPLE_FIELDS == 256 and solver.MAX_SAMPLE_VALUES == 2 ** 28
    solver.TemperatureSampler(prob, [good] * 256).close()


def test_the_classmethods_refuse_before_the_device(monkeypatch):
    no_device(monkeypatch, Unreachable)
    prob, meshes = small_problem()

    def report(temperatures):
        return solver.ThermalReport(temperatures=temperatures, face_temperatures=None, disconnected_temperatures=[], hotspots=[],
                                    layers=[], elements={}, total_heat=0.0, total_loss=0.0, info={})
    good = report(field_on(meshes))
    with pytest.raises(ValueError, match=r"field 1 is None.*per_case_fields=False"):
        solver.TemperatureSampler.of_reports(prob, [good, report(None)])
    with pytest.raises(ValueError, match="ThermalReport"):
        solver.TemperatureSampler.of_reports(prob, [good, "x"])
    with pytest.raises(ValueError, match="ThermalEnvelope"):
        solver.TemperatureSampler.of_reports(prob, good, envelope=good)
    with pytest.raises(ValueError, match="0 fields"):
        solver.TemperatureSampler.of_reports(prob, [])
    with pytest.raises(ValueError, match="TransientReport"):
        solver.TemperatureSampler.of_transient(prob, good)
    xy, tri = synthetic.jittered_grid(5, 4, h=0.5, seed=2, jitter=0.1)
    envelope = solver.ThermalEnvelope(temperatures=field_on([meshes[0], mesh.Mesh(xy, tri)]), cases=[], hotspots=[])
    with pytest.raises(ValueError, match=r"field 'envelope', layer 1, mesh 0: another mesh"):
        solver.TemperatureSampler.of_reports(prob, [good, good], envelope=envelope)
    monkeypatch.setattr(_hip, "Sampler", FieldsOnly)
    envelope = solver.ThermalEnvelope(temperatures=field_on(meshes, 50.0), cases=[], hotspots=[])
    with solver.TemperatureSampler.of_reports(prob, [good, good], envelope=envelope) as ts:
        assert ts.names == [0, 1, "envelope"] and ts.n_fields == 3
    with solver.TemperatureSampler.of_reports(prob, good) as ts:
        assert ts.names == [0]
    tenv = solver.TransientEnvelope(temperatures=field_on(meshes, 60.0), times=[], hotspots=[])

    def transient(times, fields):
        return solver.TransientReport(times=np.zeros(1), hotspots=[], layers=[], total_stored=np.zeros(1), total_loss=np.zeros(1),
                                      total_heat=np.zeros(1), probes={}, peak=None, envelope=tenv, snapshot_times=times,
                                      temperatures=fields, face_temperatures=[], disconnected_temperatures=[], info={})
    with solver.TemperatureSampler.of_transient(prob, transient([0.5, 2.0], [field_on(meshes), field_on(meshes, 35.0)])) as ts:
        assert ts.names == [0.5, 2.0, "envelope"]
    with solver.TemperatureSampler.of_transient(prob, transient([], [])) as ts:      # no field kept: the envelope alone
        assert ts.names == ["envelope"] and ts.n_fields == 1


def test_queries_are_refused_before_the_device(monkeypatch):
    no_device(monkeypatch, FieldsOnly)
    prob, meshes = small_problem()
    top = prob.layers[0]
    stranger = problem.Layer(shape=H.Geoms(1), name=top.name, conductance=top.conductance)
    good = field_on(meshes)
    with solver.TemperatureSampler(prob, [good, good]) as ts:
        def refused(match, call, *args, **kw):
            with pytest.raises(ValueError, match=match):
                call(*args, **kw)
        # without a model there is no heat flux
        refused("heat_flux needs the sheet conductances", ts.points, top, [[0.0, 0.0]], flux=True)
        refused("heat_flux needs the sheet conductances", ts.line, top, (0, 0), (1, 1), 5, flux=True)
        refused("heat_flux needs the sheet conductances", ts.raster, top, (0, 0), 0.1, 4, 4, flux=True)
        # every refusal FieldSampler's queries make
        refused("not one of the Problem's layers", ts.points, stranger, [[0.0, 0.0]])
        refused("not one of the Problem's layers", ts.line, stranger, (0, 0), (1, 1), 5)
        refused("not one of the Problem's layers", ts.raster, stranger, (0, 0), 0.1, 4, 4)
        refused(r"shape \(n, 2\)", ts.points, top, [0.0, 1.0])
        refused(r"shape \(n, 2\)", ts.points, top, np.zeros((4, 3)))
        refused(r"\(n, 2\) array of numbers", ts.points, top, [["a", "b"]])
        refused("not finite", ts.points, top, [[0.0, np.nan]])
        refused("not finite", ts.points, top, [[np.inf, 0.0], [1.0, 1.0]])
        refused("not finite", ts.line, top, (0, 0), (np.inf, 1), 5)
        refused("at least 2 points", ts.line, top, (0, 0), (1, 1), 1)
        refused("at least 2 points", ts.line, top, (0, 0), (1, 1), 2.5)
        refused("finite and positive", ts.raster, top, (0, 0), 0.0, 4, 4)
        refused("finite and positive", ts.raster, top, (0, 0), (0.1, -0.1), 4, 4)
        refused("finite and positive", ts.raster, top, (0, 0), np.inf, 4, 4)
        refused("finite and positive", ts.raster, top, (0, 0), (np.nan, 1.0), 4, 4)
        refused("one number or", ts.raster, top, (0, 0), (1.0, 1.0, 1.0), 4, 4)
        refused("at least one pixel", ts.raster, top, (0, 0), 0.1, 0, 4)
        refused("at least one pixel", ts.raster, top, (0, 0), 0.1, 4, -1)
        refused("must be integers", ts.raster, top, (0, 0), 0.1, 4.5, 4)
        refused("not finite", ts.raster, top, (np.nan, 0), 0.1, 4, 4)
        refused("pixel centres are not finite", ts.raster, top, (1e308, 0), 1e306, 1000, 4)
        refused(f"at most {solver.MAX_RASTER_PIXELS}", ts.raster, top, (0, 0), 0.1, 2 ** 13, 2 ** 13 + 1)
        refused(f"at most {solver.MAX_SAMPLE_POINTS}", ts.line, top, (0, 0), (1, 1), solver.MAX_SAMPLE_POINTS + 1)
        many = np.broadcast_to(np.zeros((1, 2)), (solver.MAX_SAMPLE_POINTS + 1, 2))
        refused(f"at most {solver.MAX_SAMPLE_POINTS}", ts.points, top, many)
    with pytest.raises(ValueError, match="closed"):
        ts.points(top, [[0.0, 0.0]])
    with pytest.raises(ValueError, match="closed"):
        ts.raster(top, (0, 0), 0.1, 2, 2, per_field=False)
    ts.close()
    # F x n over MAX_SAMPLE_VALUES: 256 fields x (2^20 + 1) samples
    with solver.TemperatureSampler(prob, [good] * 256) as ts:
        n = solver.MAX_SAMPLE_VALUES // 256 + 1
        with pytest.raises(ValueError, match=rf"at most {solver.MAX_SAMPLE_VALUES} values.*per_field=False"):
            ts.raster(top, (0, 0), 0.1, n, 1)
        with pytest.raises(ValueError, match="per_field=False"):
            ts.line(top, (0, 0), (1, 1), n)
        with pytest.raises(ValueError, match="per_field=False"):
            ts.points(top, np.broadcast_to(np.zeros((1, 2)), (n, 2)))
        with pytest.raises(AssertionError, match="the device was reached"):      # per_field=False lifts that limit
            ts.raster(top, (0, 0), 0.1, n, 1, per_field=False)
    # a model that does not resolve is refused as check_thermal_model refuses it
    with pytest.raises(ValueError, match="film"):
        solver.TemperatureSampler(prob, [good], model=solver.ThermalModel(film=None))
    with pytest.raises(ValueError, match="ThermalModel"):
        solver.TemperatureSampler(prob, [good], model="copper")


# ---- exports -------------------------------------------------------------------------------------------------------------

def test_the_new_names_are_exported_declared_and_bound():
    for name in ("TemperatureSampler", "TemperatureSamples", "check_temperature_fields", "check_sample_line",
                 "MAX_SAMPLE_FIELDS", "MAX_SAMPLE_VALUES"):
        assert hasattr(solver, name), name
    for name in ("of_reports", "of_transient", "points", "line", "raster", "stats", "close"):
        assert callable(getattr(solver.TemperatureSampler, name)), name
    build.build(verbose=False)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "padne_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("padne_sampler_set_fields", "padne_sampler_field_points", "padne_sampler_field_raster"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _hip.SIGNATURES, f"{name} is not bound"
    for name in ("set_fields", "field_points", "field_raster"):
        assert callable(getattr(_hip.Sampler, name)), name

"""Host half of the error estimate (no GPU): the restatement of tests/error_ref.py against P1 finite elements whose true error
is known, so that the device tests compare against something that is itself checked; the host arithmetic of
``solver`` (estimate, ratios, sizes) against definitions 5 and 6; and the refusals that come before the device."""
import math
import types

import numpy as np
import pytest

import error_ref as R
import helpers as H
from padne_amd import _hip, mesh, problem, solver, synthetic

CURVED = [row for row in R.TABLE if row[1] != "linear"]


def estimate_of(row, sigma=1.0):
    xy, tri, x, grad = R.table_case(row)
    est = R.estimate_flat(xy, tri, np.zeros(len(tri), dtype=np.int64), [sigma], x)
    return xy, tri, x, grad, est


@pytest.fixture(scope="module")
def table():
    return {row[0]: estimate_of(row) for row in R.TABLE}


@pytest.mark.parametrize("name", [row[0] for row in CURVED])
def test_the_estimate_is_the_true_error_on_smooth_solutions(table, name):
    """Effectivity: sqrt(power_error) over the true error in the energy norm within [0.9, 1.1] (measured 0.981-1.000)."""
    xy, tri, _x, grad, est = table[name]
    true = R.true_error(xy, tri, est, grad)
    ratio = math.sqrt(est.power_error) / true
    print(name, len(tri), "estimate / true error", ratio, "relative error", est.estimate)
    assert 0.9 <= ratio <= 1.1, (name, ratio)
    assert est.n_faces == len(tri) and est.power_error == est.mesh_error.sum()


@pytest.mark.parametrize("family", ["annulus", "grid"])
def test_the_estimate_halves_with_h(table, family):
    """Linear elements, rate 1: between consecutive rows of a family the relative estimate falls by 1.8 - 2.2 (measured
    1.99-2.00)."""
    rows = [row[0] for row in R.TABLE if row[1] == family]
    for coarse, fine in zip(rows, rows[1:]):
        rate = table[coarse][4].estimate / table[fine][4].estimate
        print(coarse, "->", fine, rate)
        assert 1.8 <= rate <= 2.2, (coarse, fine, rate)


def test_a_linear_potential_has_no_error(table):
    """The recovered gradient of a linear field is the field's: every eta_f <= 1e-12 |g| sqrt(sigma A_f) (measured 2e-15 at
    its largest, with |g| = 3.6 and sigma = 1)."""
    _xy, _tri, _x, _grad, est = table["linear_17"]
    print("largest eta_f", est.eta.max())
    assert (est.eta <= 1e-12 * R.LINEAR_GRADIENT * np.sqrt(est.sigma * est.area)).all()
    assert np.abs(est.G - [3.0, -2.0]).max() <= 1e-12 * R.LINEAR_GRADIENT
    assert est.estimate <= 1e-12


def two_meshes(seed=3):
    """Two jittered grids of different conductance with a smooth, non-harmonic field: (xy, tri, face_mesh, sigma, x)."""
    a_xy, a_tri = synthetic.jittered_grid(9, 7, h=0.5, seed=seed)
    b_xy, b_tri = synthetic.jittered_grid(6, 6, h=0.4, seed=seed + 1, origin=(10.0, 0.0))
    xy = np.concatenate([a_xy, b_xy])
    tri = np.concatenate([np.asarray(a_tri, dtype=np.int64), np.asarray(b_tri, dtype=np.int64) + len(a_xy)])
    face_mesh = np.concatenate([np.zeros(len(a_tri), dtype=np.int64), np.ones(len(b_tri), dtype=np.int64)])
    x = np.sin(0.7 * xy[:, 0]) * np.cosh(0.3 * xy[:, 1]) + 0.1 * xy[:, 0]
    return xy, tri, face_mesh, np.array([2000.0, 500.0]), x


def test_sums_and_the_estimate_are_definition_5():
    xy, tri, face_mesh, sigma, x = two_meshes()
    est = R.estimate_flat(xy, tri, face_mesh, sigma, x)
    assert est.power_error == est.mesh_error.sum() and est.power_error > 0
    for m in range(2):
        on = face_mesh == m
        assert est.mesh_error[m] == pytest.approx((est.eta[on] ** 2).sum(), rel=1e-12)
        assert est.mesh_power[m] == pytest.approx((sigma[m] * est.area[on] * (est.g[on] ** 2).sum(axis=1)).sum(), rel=1e-12)
        assert est.mesh_face[m] == np.flatnonzero(on)[np.argmax(est.eta[on])] and est.mesh_max[m] == est.eta[on].max()
    want = math.sqrt(est.power_error / (est.mesh_power.sum() + est.power_error))
    assert est.estimate == pytest.approx(want, rel=1e-15)
    # the host arithmetic of the solver is the same
    power_error, estimate = solver.error_estimate_of(est.mesh_error, est.mesh_power)
    assert power_error == est.power_error and estimate == pytest.approx(est.estimate, rel=1e-15)
    assert solver.error_estimate_of([0.0, 0.0], [0.0, 0.0]) == (0.0, 0.0)      # no power: 0.0, not 0 / 0
    zero = R.estimate_flat(xy, tri, face_mesh, sigma, np.zeros(len(xy)))
    assert zero.estimate == 0.0 and not zero.eta.any() and not zero.G.any()


def test_ratios_and_sizes_are_definition_6():
    xy, tri, face_mesh, sigma, x = two_meshes()
    x = x.copy()
    # eta = 0 up to rounding is not enough for the xi = 0 rule: mesh 1 carries no potential at all (g = G = 0 exactly)
    x[face_mesh_vertices(tri, face_mesh, 1)] = 0.0
    est = R.estimate_flat(xy, tri, face_mesh, sigma, x)
    assert not est.eta[face_mesh == 1].any() and est.eta[face_mesh == 0].all()
    tol = 0.05
    xi, size = R.ratios_sizes(est, tol)
    e_bar = tol * math.sqrt((est.mesh_power.sum() + est.power_error) / len(tri))
    h = np.sqrt(4 * est.area / math.sqrt(3.0))
    assert np.allclose(xi, est.eta / e_bar, rtol=1e-15, atol=0)
    assert np.isinf(size[face_mesh == 1]).all() and np.allclose(size[face_mesh == 0], h[face_mesh == 0] / xi[face_mesh == 0], rtol=1e-15)
    assert (xi > 1).any() and (xi < 1).any()                              # some faces to refine, some fine enough
    # the same through the solver's host arithmetic, mesh by mesh
    for m in range(2):
        on = face_mesh == m
        local = tri[on] - tri[on].min()
        pts = xy[tri[on].min():tri[on].max() + 1]
        got_h = solver.face_sizes(pts, local)
        assert np.allclose(got_h, h[on], rtol=1e-15, atol=0)
        got_xi, got_size = solver.refinement_ratios(est.eta[on], got_h, est.total_power, est.n_faces, tol)
        assert np.allclose(got_xi, xi[on], rtol=1e-14, atol=0)
        assert np.array_equal(np.isinf(got_size), np.isinf(size[on]))
        assert np.allclose(got_size[~np.isinf(got_size)], size[on][~np.isinf(size[on])], rtol=1e-14, atol=0)
    # a board without power: xi = 0 and no size is suggested
    xi0, size0 = solver.refinement_ratios(np.zeros(4), np.ones(4), 0.0, 4, tol)
    assert not xi0.any() and np.isinf(size0).all()


def face_mesh_vertices(tri, face_mesh, m):
    return np.unique(tri[face_mesh == m])


def test_a_disconnected_mesh_is_zero_and_left_out_of_n_faces():
    xy, tri, face_mesh, sigma, x = two_meshes()
    both = R.estimate_flat(xy, tri, face_mesh, sigma, x)
    est = R.estimate_flat(xy, tri, face_mesh, sigma, x, connected=[True, False])
    off = face_mesh == 1
    assert est.n_faces == int((~off).sum()) < both.n_faces
    assert not est.eta[off].any() and not est.G[face_mesh_vertices(tri, face_mesh, 1)].any()
    assert est.mesh_error[1] == 0.0 and est.mesh_power[1] == 0.0
    assert np.array_equal(est.eta[~off], both.eta[~off]) and est.mesh_error[0] == both.mesh_error[0]
    assert est.power_error == both.mesh_error[0]
    xi, size = R.ratios_sizes(est, 0.1)
    e_bar = 0.1 * math.sqrt((est.mesh_power[0] + est.mesh_error[0]) / est.n_faces)
    assert np.allclose(xi[~off], est.eta[~off] / e_bar, rtol=1e-15, atol=0) and np.isinf(size[off]).all()


def test_permuting_the_faces_permutes_eta_and_keeps_the_sums():
    xy, tri, face_mesh, sigma, x = two_meshes()
    est = R.estimate_flat(xy, tri, face_mesh, sigma, x)
    rng = np.random.default_rng(11)
    perm = np.concatenate([rng.permutation(np.flatnonzero(face_mesh == m)) for m in range(2)])     # within each mesh
    again = R.estimate_flat(xy, tri[perm], face_mesh[perm], sigma, x)
    assert not np.array_equal(perm, np.arange(len(tri)))
    assert (np.abs(again.eta - est.eta[perm]) <= 1e-12 * est.eta_scale(tri)[perm]).all()
    assert (np.abs(again.G - est.G) <= 1e-12 * est.g_around[:, None]).all()
    for a, b in ((again.mesh_error, est.mesh_error), (again.mesh_power, est.mesh_power)):
        assert np.allclose(a, b, rtol=1e-12, atol=0)
    assert again.power_error == pytest.approx(est.power_error, rel=1e-12)
    assert again.estimate == pytest.approx(est.estimate, rel=1e-12)
    assert np.array_equal(perm[again.mesh_face], est.mesh_face)


# ---- the refusals that come before the device -----------------------------------------------------------------------

def fixture_board(name):
    g = H.load_golden(name)
    prob, _ids, _flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    return prob, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms]


@pytest.mark.parametrize("bad", [0, 0.0, 1, 1.0, -0.1, 1.5, np.nan, np.inf, -np.inf, True, False, np.True_, "0.1", b"0.1",
                                 [0.1], object()])
def test_an_invalid_tolerance_is_refused_before_the_device(monkeypatch, bad):
    def no_device(*_a, **_k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    prob, meshes, layer_of = fixture_board("problem_mixed")
    with pytest.raises(ValueError, match="tolerance"):
        solver.check_tolerance(bad)
    with pytest.raises(ValueError, match="tolerance"):
        solver.solve_meshed_error(prob, meshes, layer_of, tolerance=bad)
    with pytest.raises(ValueError, match="tolerance"):
        solver.solve_error(prob, tolerance=bad, mesher=object())


def test_valid_tolerances_and_the_partition_refusal(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    assert solver.check_tolerance(None) is None
    assert solver.check_tolerance(0.05) == 0.05 and solver.check_tolerance(np.float32(0.5)) == 0.5
    assert solver.check_tolerance(1e-300) == 1e-300 and solver.check_tolerance(1 - 2 ** -53) < 1
    prob, meshes, layer_of = fixture_board("problem_mixed")
    several = types.SimpleNamespace(world=2, rank=0)
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_meshed_error(prob, meshes, layer_of, partition=several)
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_meshed_error(prob, meshes, layer_of, tolerance=0.1, partition=several)
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_error(prob, mesher=object(), partition=several)


def test_the_report_has_the_fields_of_the_issue():
    names = [f.name for f in solver.dataclasses.fields(solver.ErrorReport)]
    assert names == ["recovered", "indicators", "worst", "layers", "power_error", "estimate", "ratios", "sizes", "tolerance"]
    rep = solver.ErrorReport([], [], [], [], 0.0, 0.0)
    assert rep.ratios is None and rep.sizes is None and rep.tolerance is None

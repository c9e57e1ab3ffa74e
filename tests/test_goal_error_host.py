"""The goal-oriented error estimate without a device: the host restatement (tests/goal_ref.py) against its own properties
and against the true a(u - u_h, z - z_h) of harmonic pairs, and the argument checks of the public entry points."""
import types

import numpy as np
import pytest

import error_ref as R
import goal_ref as Gr
import helpers as H
from padne_amd import _hip, mesh, problem, solver, synthetic


def no_device(*_a, **_k):
    raise AssertionError("the device was reached")


def random_case(seed=3, n_fields=3):
    xy, tri = synthetic.jittered_grid(9, 7, h=0.25, seed=seed)
    xy, tri = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    return xy, tri, rng.normal(size=(n_fields, len(xy)))


# ---- the restatement's own properties ---------------------------------------------------------------------------------

def test_a_field_paired_with_itself_gives_eta_squared():
    xy, tri, fields = random_case()
    goal = Gr.goal_flat(xy, tri, np.zeros(len(tri), dtype=np.int64), [3.0], [fields[0], fields[0]])
    eta2 = goal.primal.eta ** 2
    assert (eta2 > 0).all()
    tol = 4 * np.spacing(eta2)
    assert (np.abs(goal.delta[0] - eta2) <= tol).all() and (np.abs(goal.omega[0] - eta2) <= tol).all()
    assert np.array_equal(goal.eta[0], goal.primal.eta)
    assert goal.mesh_face[0, 0] == goal.primal.mesh_face[0]
    assert goal.correction[0] == -goal.mesh_delta[0].sum() and goal.bound[0] == goal.mesh_omega[0].sum()


def test_cauchy_schwarz_on_random_fields():
    for seed in range(5):
        xy, tri, fields = random_case(seed, n_fields=4)
        goal = Gr.goal_flat(xy, tri, np.zeros(len(tri), dtype=np.int64), [1.7], fields)
        assert (np.abs(goal.delta) <= goal.omega * (1 + 1e-12)).all()
        assert (goal.delta < 0).any() and (goal.delta > 0).any()           # signed
        assert (np.abs(goal.mesh_delta) <= goal.mesh_omega).all() and (np.abs(goal.correction) <= goal.bound).all()


def test_disconnected_meshes_give_zeros_and_do_not_count():
    xy, tri, fields = random_case()
    n, nv = len(tri), len(xy)
    xy2, tri2 = np.concatenate([xy, xy + [10.0, 0.0]]), np.concatenate([tri, tri + nv])
    face_mesh = np.concatenate([np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int64)])
    both = np.concatenate([fields, fields], axis=1)
    goal = Gr.goal_flat(xy2, tri2, face_mesh, [2.0, 2.0], both, connected=[True, False])
    alone = Gr.goal_flat(xy, tri, np.zeros(n, dtype=np.int64), [2.0], fields)
    assert goal.n_faces == n == alone.n_faces
    for name in ("delta", "omega"):
        assert np.array_equal(getattr(goal, name)[:, :n], getattr(alone, name)) and not getattr(goal, name)[:, n:].any()
    assert not goal.mesh_omega[:, 1].any() and not goal.mesh_delta[:, 1].any()
    assert np.array_equal(goal.bound, alone.bound) and np.array_equal(goal.correction, alone.correction)
    assert np.array_equal(Gr.goal_ratios(goal, 1e-3)[:, :n], Gr.goal_ratios(alone, 1e-3))


def test_the_ratios_formula():
    xy, tri, fields = random_case()
    goal = Gr.goal_flat(xy, tri, np.zeros(len(tri), dtype=np.int64), [1.0], fields)
    tolerance = 0.5 * goal.bound.max()
    xi = Gr.goal_ratios(goal, tolerance)
    assert xi.shape == goal.omega.shape
    assert np.allclose(xi * (tolerance / len(tri)), goal.omega, rtol=1e-15, atol=0)
    # faces at exactly their share sum to the tolerance: with a bound above it some face must be flagged
    assert (xi.max(axis=0) > 1).any()
    for j in range(2):
        assert np.array_equal(solver.goal_ratios(goal.omega[j], goal.n_faces, tolerance), xi[j])
    assert not solver.goal_ratios(goal.omega[0], 0, tolerance).any()


def test_the_sign_convention_is_the_solvers():
    assert solver.GOAL_CORRECTION_SIGN == Gr.CORRECTION_SIGN == -1.0


# ---- the yardstick ----------------------------------------------------------------------------------------------------

# sum_f delta_f over the true a(u - u_h, z - z_h), measured on the CPU with numpy 2 / scipy's SuperLU:
#   annulus (ln r with ln |p - (0.3, 0.2)|):   17x64 0.9898,  33x128 0.9986,  65x256 1.0006
#   grid (e^x cos y with e^x sin y):            17 0.9728,     33 0.9549,      65 0.9784
MEASURED = {"annulus": (0.9898, 1.0006), "grid": (0.9549, 0.9784)}


@pytest.fixture(scope="module")
def pairs():
    out = {}
    for row in R.TABLE:
        xy, tri, u_h, z_h, grad_u, grad_z = Gr.pair_case(row)
        goal = Gr.goal_flat(xy, tri, np.zeros(len(tri), dtype=np.int64), [1.0], [u_h, z_h])
        out[row[0]] = (row[1], goal, Gr.true_product(xy, tri, goal, grad_u, grad_z))
    return out


def test_sum_delta_has_the_sign_and_the_size_of_the_true_product(pairs):
    """u_h and z_h are the P1 solutions for two different harmonic functions on every row of error_ref.TABLE; the true
    a(u - u_h, z - z_h) comes from the exact gradients by the degree-2 quadrature of ``error_ref.true_error``.

    Measured ratios sum delta / true (CPU): annulus 0.9898, 0.9986, 1.0006 at 17x64, 33x128, 65x256; grid 0.9728, 0.9549,
    0.9784 at 17, 33, 65.  Asserted: the sign on every row, and the ratio inside the measured interval of its family widened
    by 10 % on each side (annulus 0.891 .. 1.101, grid 0.859 .. 1.076).

    Dropped pairs: the ``linear`` row, whose P1 solution is exact, so its true product is rounding noise (1.5e-17) without
    a sign; and for the annulus ln r with x / r^2 or with ln |p - (6, 0)|, whose errors are orthogonal to the radial error
    of ln r (true product 1e-18 against a bound of 1e-3): ln |p - (0.3, 0.2)| is paired with ln r instead."""
    for name, (family, goal, true) in pairs.items():
        total = float(goal.mesh_delta[0, 0])
        if family == "linear":
            print(name, "sum delta", total, "true", true, "bound", goal.bound[0])
            assert abs(total) <= 1e-12 and abs(true) <= 1e-12 and goal.bound[0] <= 1e-12
            continue
        ratio = total / true
        print(name, "sum delta", total, "true", true, "ratio", ratio, "|true| / bound", abs(true) / goal.bound[0])
        assert np.sign(total) == np.sign(true) != 0, name
        lo, hi = MEASURED[family]
        assert 0.9 * lo <= ratio <= 1.1 * hi, (name, ratio)
        assert abs(true) <= goal.bound[0]
        # what correction estimates: a(u - u_h, z - z_h) = -a(u - u_h, lambda - lambda_h) for lambda = -z
        assert goal.correction[0] == -total


@pytest.mark.parametrize("family", ["annulus", "grid"])
def test_the_bound_at_least_halves_when_h_halves(pairs, family):
    rows = [row[0] for row in R.TABLE if row[1] == family]
    for coarse, fine in zip(rows, rows[1:]):
        b0, b1 = pairs[coarse][1].bound[0], pairs[fine][1].bound[0]
        print(coarse, "->", fine, "bound", b0, b1, b0 / b1)
        assert b1 <= b0 / 2


# ---- argument checks --------------------------------------------------------------------------------------------------

BAD_TOLERANCES = [True, False, np.True_, "0.1", b"1", float("nan"), float("inf"), -float("inf"), 0, 0.0, -1e-3, [0.1], object()]


@pytest.mark.parametrize("bad", BAD_TOLERANCES, ids=[repr(b)[:20] for b in BAD_TOLERANCES])
def test_check_goal_tolerance_refuses(bad):
    with pytest.raises(ValueError, match="tolerance"):
        solver.check_goal_tolerance(bad)


def test_check_goal_tolerance_accepts():
    assert solver.check_goal_tolerance(None) is None
    assert solver.check_goal_tolerance(1e-3) == 1e-3 and solver.check_goal_tolerance(5) == 5.0
    assert solver.check_goal_tolerance(np.float32(0.5)) == 0.5
    assert solver.check_goal_tolerance(7.5) == 7.5             # absolute, in volts: not confined to (0, 1)


def fixture_board(name="problem_mixed"):
    g = H.load_golden(name)
    prob, _ids, flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    return prob, flat, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms]


def an_objective(flat):
    e = next(e for e in flat if len(e.terminals) >= 2 and e.terminals[0] is not e.terminals[1])
    return (e.terminals[0], e.terminals[1])


def patch_device_away(monkeypatch):
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    monkeypatch.setattr(solver, "index_board", no_device)


def test_objectives_and_tolerance_are_checked_before_the_device(monkeypatch):
    patch_device_away(monkeypatch)
    prob, flat, meshes, layer_of = fixture_board()
    good = [an_objective(flat)]
    for bad, match in [([], "no objectives"), ([good[0][0]], "not a \\(p, n\\) pair"), ([(good[0][0], good[0][0])], "p is n"),
                       ("pn", "sequence of"), ([(1, 2)], "must be NodeIDs")]:
        with pytest.raises(ValueError, match=match):
            solver.solve_meshed_goal_error(prob, meshes, layer_of, bad)
        with pytest.raises(ValueError, match=match):
            solver.solve_goal_error(prob, bad, mesher=object())
        with pytest.raises(ValueError, match=match):
            solver.solve_meshed_goal_adaptive(prob, meshes, layer_of, bad, tolerance=1e-3)
        with pytest.raises(ValueError, match=match):
            solver.solve_goal_adaptive(prob, bad, tolerance=1e-3, mesher=object())
    for bad in (0.0, -1.0, True, "1e-3", float("nan")):
        with pytest.raises(ValueError, match="tolerance"):
            solver.solve_meshed_goal_error(prob, meshes, layer_of, good, tolerance=bad)
        with pytest.raises(ValueError, match="tolerance"):
            solver.solve_goal_error(prob, good, tolerance=bad, mesher=object())
    several = types.SimpleNamespace(world=2, rank=0)
    for call in (lambda: solver.solve_meshed_goal_error(prob, meshes, layer_of, good, partition=several),
                 lambda: solver.solve_goal_error(prob, good, partition=several, mesher=object()),
                 lambda: solver.solve_meshed_goal_adaptive(prob, meshes, layer_of, good, tolerance=1e-3, partition=several),
                 lambda: solver.solve_goal_adaptive(prob, good, tolerance=1e-3, partition=several, mesher=object())):
        with pytest.raises(ValueError, match="row-partitioned"):
            call()
    # valid arguments get as far as the first device-side step
    with pytest.raises(AssertionError, match="the device was reached"):
        solver.solve_meshed_goal_error(prob, meshes, layer_of, good, tolerance=1e-3)


ADAPTIVE_BAD = [dict(tolerance=None), dict(tolerance=0), dict(tolerance=-0.1), dict(tolerance=True), dict(tolerance="0.1"),
                dict(tolerance=np.nan), dict(tolerance=np.inf), dict(max_rounds=0), dict(max_rounds=2.5), dict(max_rounds=True),
                dict(max_rounds=None), dict(max_faces=0), dict(max_faces=1.5), dict(max_faces=False), dict(min_size=-1e-9),
                dict(min_size=np.nan), dict(min_size=np.inf), dict(min_size="1"), dict(min_size=None), dict(min_size=True)]


@pytest.mark.parametrize("bad", ADAPTIVE_BAD, ids=[str(b) for b in ADAPTIVE_BAD])
def test_goal_adaptive_arguments_are_refused_before_the_first_solve(monkeypatch, bad):
    patch_device_away(monkeypatch)
    monkeypatch.setattr(solver, "solve_meshed_goal_error", no_device)
    prob, flat, meshes, layer_of = fixture_board()
    good = [an_objective(flat)]
    kwargs = dict(tolerance=1e-3)
    kwargs.update(bad)
    what = next(iter(bad))
    with pytest.raises(ValueError, match=what):
        solver.solve_meshed_goal_adaptive(prob, meshes, layer_of, good, **kwargs)
    with pytest.raises(ValueError, match=what):
        solver.solve_goal_adaptive(prob, good, mesher=object(), **kwargs)


def test_valid_goal_adaptive_arguments_and_the_history_defaults():
    assert solver.check_goal_adaptive_arguments(2.5, 8, None, 0.0) == (2.5, 8, None, 0.0)        # volts: above 1 is fine
    assert solver.check_goal_adaptive_arguments(np.float32(0.5), np.int64(1), np.int32(7), 1) == (0.5, 1, 7, 1.0)
    history = solver.GoalAdaptiveHistory()
    assert isinstance(history, solver.AdaptiveHistory)
    assert history.values == [] and history.bounds == [] and history.values is not solver.GoalAdaptiveHistory().values
    assert history.faces == [] and history.estimates == [] and history.reason == ""
    # existing uses are unchanged: the energy-norm loop's record keeps its fields
    assert [f.name for f in solver.dataclasses.fields(solver.AdaptiveHistory)] == [
        "faces", "vertices", "estimates", "flagged", "closure_edges", "reason", "meshes"]
    assert [f.name for f in solver.dataclasses.fields(solver.GoalAdaptiveHistory)][-2:] == ["values", "bounds"]

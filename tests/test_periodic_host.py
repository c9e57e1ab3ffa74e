"""Host half of the periodic steady state (no GPU): the specification of tests/periodic_ref.py against a dense solve of
(I - Phi) theta* = d built from explicit step matrices, the properties the design rests on (Phi self-adjoint in the C inner
product, a C-orthonormal basis after two Gram-Schmidt passes), the count of period applications against brute-force
repetition, frozen columns, and the refusals of ``check_periodic_control`` and the public call, which come before the
device.

Boards: the meshes of tests/test_thermal.py's small synthetic boards restated on the host -- ``single`` (one jittered
17 x 17 grid) and the two-mesh board with an internal node between the layers of tests/test_thermal_host.py -- and the
jittered 49 x 49 grid of tests/test_transient.py (kappa 0.0149, film 1e-3, c 3e-3)."""
import numpy as np
import pytest

import periodic_ref as PR
import thermal_ref as T
import transient_ref as R
from padne_amd import problem as P, solver
from test_thermal_host import board, grid, two_mesh_case
from test_transient_host import KAPPA, _World, model_of

FILM, CAP = 1e-3, 3e-3
TAU = CAP / FILM


def small_board(name):
    """(A, Cv, B, n_vert): ``single`` or ``two_layer`` with two random load cases of 1 W and 0.5 W."""
    if name == "single":
        meshes, links, n_int = [grid(17, seed=1)], [], 0
        kappa, film, cap = [KAPPA], [FILM], [CAP]
    else:
        meshes, links, _n_vert = two_mesh_case()
        n_int, kappa, film, cap = 1, [KAPPA, 2 * KAPPA], [FILM, 3 * FILM], [CAP, 2 * CAP]
    A, M, _hM = T.operator(meshes, kappa, film, n_int, links)
    _xy, tri, _face_mesh, voff, _toff = T.flatten(meshes)
    n_vert = int(voff[-1])
    Cv = R.capacity(voff, cap, M)
    rng = np.random.default_rng(11)
    B = []
    for watts in (1.0, 0.5):
        Pf = rng.uniform(0.0, 1.0, len(tri))
        heat = [(n_vert, 0.1 * watts)] if n_int else []
        B.append(T.load(n_vert + n_int, tri, watts * Pf / Pf.sum(), heat=heat))
    return A, Cv, B, n_vert


def duty(period, steps_on=6, steps_off=8, on=0):
    """On for 40 % of the period, off for the rest, with unequal dt."""
    return [(0.4 * period / steps_on, steps_on, on), (0.6 * period / steps_off, steps_off, None)]


def grid49():
    xy, tri = grid(49, seed=7)
    A, M, _hM = T.operator([(xy, tri)], [0.0149], [FILM], 0, [])
    voff = np.array([0, len(xy)])
    Pf = np.random.default_rng(5).uniform(0.0, 1.0, len(tri))
    return A, R.capacity(voff, [CAP], M), [T.load(len(xy), tri, Pf / Pf.sum())]


@pytest.mark.parametrize("name", ["single", "two_layer"])
@pytest.mark.parametrize("period", [TAU / 5, TAU / 30])
def test_the_iterate_against_the_dense_periodic_state(name, period):
    """At the vertices |theta - theta*|_inf <= ||(I - Phi_vv)^-1||_inf (closure + steps 1e-12 max |theta*|): (I - Phi)(theta -
    theta*) is minus the closure vector, whose vertex part the tolerance bounds, and Phi reads its argument at the vertices
    only, so the vertex block stands alone.  The second term is the slack of the direct step solves: cond(S) 2^-52 <= 1e-12
    relative per step, added over the steps of a period.  The norm is computed here from the dense matrices."""
    A, Cv, B, n_vert = small_board(name)
    schedule, tolerance = duty(period), 1e-6
    per = PR.Period(A, Cv, B, schedule)
    Phi, d = PR.dense_period(A, Cv, B, schedule)
    want, _ = PR.dense_periodic_state(Phi, d)
    norm = float(np.abs(np.linalg.inv(np.eye(n_vert) - Phi[:n_vert, :n_vert])).sum(axis=1).max())
    got = PR.gmres(per, np.zeros(A.shape[0]), tolerance, 64)
    closure = per.closure(got["theta"])
    err = float(np.abs(got["theta"][:n_vert] - want[:n_vert]).max())
    print(name, period, "periods", got["periods"], "closure", closure, "predicted", got["predicted"][-1], "error", err,
          "bound", norm * (closure + per.steps * 1e-12 * np.abs(want).max()), "norm", norm)
    assert closure <= tolerance and got["periods"] < 64
    assert abs(got["predicted"][-1] - closure) <= 1e-9 * np.abs(want).max()       # the prediction is the residual, to the solves' slack
    assert err <= norm * (closure + per.steps * 1e-12 * np.abs(want).max())
    # the dense fixed point is one: a period from it returns to it
    assert per.closure(want) <= per.steps * 1e-12 * np.abs(want).max() * 10


@pytest.mark.parametrize("name", ["single", "two_layer"])
def test_phi_is_self_adjoint_in_the_c_inner_product_and_the_basis_orthonormal(name):
    """C Phi_vv is symmetric to rounding (every step operator is a function of C^-1 A), and V^T C V = I within 1e-12 after
    the two Gram-Schmidt passes (twice is enough: the loss of orthogonality is a modest multiple of 2^-53)."""
    A, Cv, B, n_vert = small_board(name)
    schedule = duty(TAU / 5)
    Phi, _d = PR.dense_period(A, Cv, B, schedule)
    CPhi = Cv[:, None] * Phi[:n_vert, :n_vert]
    assert np.abs(CPhi - CPhi.T).max() <= 1e-12 * np.abs(CPhi).max()
    eig = np.linalg.eigvalsh((CPhi + CPhi.T) / 2 / np.sqrt(Cv)[:, None] / np.sqrt(Cv)[None, :])
    assert eig.min() > 0.0 and eig.max() < 1.0                                   # the spectrum lies in (0, 1)
    got = PR.gmres(PR.Period(A, Cv, B, schedule), np.zeros(A.shape[0]), 1e-9, 64)
    V = np.stack(got["V"])[:, :n_vert]
    G = (V * Cv) @ V.T
    print(name, "vectors", len(V), "worst |V^T C V - I|", np.abs(G - np.eye(len(V))).max())
    assert len(V) >= 4 and np.abs(G - np.eye(len(V))).max() <= 1e-12


def test_fewer_period_applications_than_repetition_on_the_49_grid():
    """The 49 x 49 board, a period of TAU / 30 in two segments of unequal dt (6 + 8 steps), from ambient to a closure of
    1e-6 K: GMRES in the C inner product spends 15 period applications (the first, 13 Krylov ones and the recorded one),
    brute-force repetition 369 periods.  The counts are recorded, the assertion is the strict inequality."""
    A, Cv, B = grid49()
    per = PR.Period(A, Cv, B, duty(TAU / 30))
    got = PR.gmres(per, np.zeros(A.shape[0]), 1e-6, 64)
    brute, _theta = PR.brute_force(per, np.zeros(A.shape[0]), 1e-6)
    print("gmres", got["periods"], "brute force", brute, "predicted", got["predicted"])
    assert per.closure(got["theta"]) <= 1e-6
    assert got["periods"] < brute


def test_a_frozen_column_next_to_a_loaded_one():
    """A scenario with every segment off that starts at ambient is periodic at once: beta = 0, exact zeros, no NaN, closure
    0, two period applications.  The loaded scenario next to it is untouched by it."""
    A, Cv, B, n_vert = small_board("single")
    off = PR.Period(A, Cv, B, [(dt, steps, None) for dt, steps, _case in duty(TAU / 5)])
    got = PR.gmres(off, np.zeros(A.shape[0]), 1e-6, 64)
    assert got["frozen"] and got["periods"] == 2 and got["first"] == 0.0 and got["beta"] == 0.0
    assert np.array_equal(got["theta"], np.zeros(A.shape[0])) and np.array_equal(got["V"][0], np.zeros(A.shape[0]))
    assert off.closure(got["theta"]) == 0.0
    # the kernels of a frozen column, one step on: zeros stay zeros and nothing is NaN
    h, nxt = PR.push(Cv, got["V"], off.apply(got["V"][0], sources=False))
    assert np.array_equal(h, np.zeros(2)) and np.array_equal(nxt, np.zeros(A.shape[0]))
    assert PR.predict(np.zeros(A.shape[0]), [0.0, 0.0], [got["V"][0], nxt], n_vert) == (0.0, 0)
    on = PR.gmres(PR.Period(A, Cv, B, duty(TAU / 5)), np.zeros(A.shape[0]), 1e-6, 64)
    assert not on["frozen"] and np.isfinite(on["theta"]).all()


def test_tops_count_what_is_not_finite_as_infinity_and_keep_the_lowest_vertex():
    a = np.zeros(700)
    a[[5, 300, 699]] = [-2.0, 2.0, 2.0]
    assert PR.top(a, 700) == (2.0, 5)
    a[650] = np.nan
    assert PR.top(a, 700) == (np.inf, 650)
    a[620] = -np.inf
    assert PR.top(a, 700) == (np.inf, 620)
    assert PR.top(a, 600) == (2.0, 5) and PR.top(a, 0) == (0.0, -1)


# ---- the checks that come before the device ------------------------------------------------------------------------------

def test_the_names_are_exported():
    for name in ("PeriodicReport", "check_periodic_control", "solve_meshed_thermal_periodic", "solve_thermal_periodic",
                 "periodic_iteration"):
        assert hasattr(solver, name), name


def test_check_periodic_control():
    assert solver.check_periodic_control(1e-3) == (1e-3, 64)
    assert solver.check_periodic_control(2, np.int64(3)) == (2.0, 3)
    assert solver.check_periodic_control(1e-6, 4096) == (1e-6, 4096)
    for bad in (0.0, -1e-3, float("nan"), float("inf"), None, "tight"):
        with pytest.raises(ValueError):
            solver.check_periodic_control(bad)
    for bad in (2, 0, -1, 4097, 3.0, True, None, "many"):
        with pytest.raises(ValueError):
            solver.check_periodic_control(1e-3, bad)


def test_the_public_call_refuses_before_the_device():
    """Everything the transient call refuses (tests/test_transient_host.py) and the control's own refusals raise ValueError
    with empty mesh lists: nothing reaches the device."""
    prob, *_ = board()
    S, call = solver.Segment, solver.solve_meshed_thermal_periodic
    ok = [S(1.0, 2, 0), S(2.0, 2, None)]
    stranger = P.NodeID()
    source = prob.networks[0].elements[0]
    bad = [
        dict(model=model_of(None), schedule=ok),
        dict(model=model_of({"F.Cu": 3e-3}), schedule=ok),
        dict(model=model_of(), schedule=[]),
        dict(model=model_of(), schedule=[S(1.0, 2, 1)]),
        dict(model=model_of(), schedule=[S(1.0, 0, 0)]),
        dict(model=model_of(), schedule=[solver.Span(1.0, 0)]),                           # fixed-step schedules only
        dict(model=model_of(), schedule=ok, cases=[{source: float("nan")}]),
        dict(model=model_of(initial=2), schedule=ok),
        dict(model=model_of(initial=(0, None, 0)), schedule=[S(1.0, 2, (0, None))]),
        dict(model=model_of(), schedule=ok, probes=[stranger]),
        dict(model=model_of(), schedule=ok, probes=["pad"]),
        dict(model=model_of(), schedule=ok, keep="all"),
        dict(model=model_of(), schedule=ok, partition=_World()),
        dict(model=solver.ThermalModel(film=1e-5), schedule=ok),
        dict(model=solver.ElectroThermalTransientModel(electrothermal=None, areal_capacity=3e-3), schedule=ok),   # one-way coupling only
        dict(model=model_of(), schedule=ok, tolerance=0.0),
        dict(model=model_of(), schedule=ok, tolerance=float("nan")),
        dict(model=model_of(), schedule=ok, tolerance=None),
        dict(model=model_of(), schedule=ok, max_periods=2),
        dict(model=model_of(), schedule=ok, max_periods=4097),
        dict(model=model_of(), schedule=ok, max_periods=8.0),
    ]
    for kw in bad:
        model, schedule = kw.pop("model"), kw.pop("schedule")
        kw.setdefault("tolerance", 1e-3)
        with pytest.raises(ValueError):
            call(prob, [], [], model, schedule, **kw)
        if "partition" not in kw:
            with pytest.raises(ValueError):
                solver.solve_thermal_periodic(prob, model, schedule, mesher=object(), **kw)
    with pytest.raises(TypeError):
        call(prob, [], [], model_of(), ok)                                                # the tolerance is required
    with pytest.raises(TypeError):
        call(prob, [], [], model_of(), ok, tolerance=1e-3, repeat=2)                      # a period is not repeated

"""Host half of the resistor coupling (no GPU): the restatement of tests/resistor_coupling_ref.py against answers that are
known -- a fresh assembly with every resistor at R / s, the closed form of a via in series with a current source, the balance
of every round, zero coefficients -- so that the device tests compare against something that is itself checked; and the
refusals of ``check_electrothermal_model``, which come before the device."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

import coupled_ref as C
import resistor_coupling_ref as RC
import thermal_ref as T
from padne_amd import problem as P, solver
from test_coupled_host import small_problem, thermal_board

EPS = np.finfo(np.float64).eps


# ---- 1. the revalued matrix ------------------------------------------------------------------------------------------------

def strips(s_of, sr_of):
    """The strips board assembled on the host: (L0, L revalued by the restatement, L with the faces alone revalued, the fresh
    assembly with sigma s per face and R / sr per resistor, n_vert, the resistors' rows, s, sr)."""
    meshes, sigma, n_vert, n_internal, rows = RC.strips_system()
    L0, _r = C.O.assemble_system([(xy, tri, g) for (xy, tri), g in zip(meshes, sigma)], n_internal, rows, 0)
    L0 = sp.csr_matrix(L0)
    L0.sort_indices()
    xy, tri, face_mesh, _voff, _toff = T.flatten(meshes)
    s, sr = s_of(len(tri)), sr_of(len(rows))
    a, b, R = [row[1] for row in rows], [row[2] for row in rows], np.array([row[3] for row in rows])
    faces = C.revalue(L0, xy, tri, face_mesh, sigma, s)
    L = RC.revalue_resistors(faces, RC.places(L0, a, b), sr, 1 / R)
    warm = [row[:3] + (row[3] / s_r,) for row, s_r in zip(rows, sr.tolist())]
    L_warm, _r = C.O.assemble_system([(xy, tri, g) for (xy, tri), g in zip(meshes, sigma)], n_internal, warm, 0)
    N = L0.shape[0]
    pad = lambda K: sp.block_diag([K, sp.csr_matrix((N - n_vert, N - n_vert))]).tocsr()                      # noqa: E731
    per_face = np.asarray(sigma)[face_mesh]
    fresh = pad(C.fresh_assembly(n_vert, xy, tri, per_face * s)) + (sp.csr_matrix(L_warm) - pad(C.fresh_assembly(n_vert, xy, tri, per_face)))
    return L0, L, faces, fresh.tocsr(), n_vert, rows, s, sr


def test_the_revalued_matrix_is_a_fresh_assembly_with_every_resistor_at_its_warm_resistance():
    """Per entry within 16 eps of the sum of the magnitudes stamped into it, |L0| + |fresh| (every stamp of an entry has one
    sign: faces and resistors add to the off-diagonals and take from the diagonal).  The entry with the most stamps is the
    diagonal of vertex 20: three faces (6 products) and three resistors on the restatement's side, each product, each partial
    sum and each sequential update rounded once by at most eps / 2 of a magnitude below that sum -- 6 + 6 + 1 + 3 roundings,
    8 eps -- and the fresh assembly's own sums of at most 9 terms on the other, 4.5 eps: 16 covers both."""
    rng = np.random.default_rng(21)
    L0, L, _faces, fresh, _n_vert, _rows, _s, _sr = strips(lambda n: rng.uniform(0.5, 1.5, n), lambda n: rng.uniform(0.5, 1.5, n))
    gap = np.abs((L - fresh).toarray())
    magnitude = np.abs(L0.toarray()) + np.abs(fresh.toarray())
    stored = magnitude > 0
    print("largest gap in eps of the entry's magnitudes", (gap[stored] / magnitude[stored]).max() / EPS)
    assert (gap <= 16 * EPS * magnitude).all()
    assert (L != L0).nnz > 0


def test_resistor_scales_of_one_write_nothing_and_the_block_stays_symmetric():
    rng = np.random.default_rng(22)
    L0, L, faces, _fresh, n_vert, rows, _s, sr = strips(np.ones, np.ones)
    assert np.array_equal(L.indices, L0.indices) and np.array_equal(L.data, L0.data)
    # the faces move, the resistors stay: the bits of the face-only revalue
    L0, L, faces, *_ = strips(lambda n: rng.uniform(0.5, 1.5, n), np.ones)
    assert np.array_equal(L.data, faces.data) and (faces != L0).nnz > 0
    # both move: the potential block (vertices and the internal node) is symmetric bit for bit
    L0, L, faces, _fresh, n_vert, rows, _s, sr = strips(lambda n: rng.uniform(0.5, 1.5, n), lambda n: rng.uniform(0.5, 1.5, n))
    K = L[:n_vert + 1, :n_vert + 1]
    assert (K != K.T).nnz == 0
    # rows without an incidence keep the values of the face-only revalue: vertex 7 has its joiner, so take the ground row and
    # every column outside the potential block; and the resistor with both ends on one unknown wrote nothing
    touched = sorted({row[1] for row in rows if row[1] != row[2]} | {row[2] for row in rows if row[1] != row[2]})
    assert touched == list(range(n_vert + 1))
    assert (L[n_vert + 1:] != faces[n_vert + 1:]).nnz == 0 and (L[:, n_vert + 1:] != faces[:, n_vert + 1:]).nnz == 0
    alone = RC.revalue_resistors(faces, RC.places(L0, [7], [7]), [0.5], [100.0])
    assert np.array_equal(alone.data, faces.data)
    # a row no resistor touches: the same board without the joiner of vertex 299
    at = RC.places(L0, [row[1] for row in rows[:299]], [row[2] for row in rows[:299]])
    partly = RC.revalue_resistors(faces, at, sr[:299], 1 / np.array([row[3] for row in rows[:299]]))
    assert np.array_equal(partly[299].toarray(), faces[299].toarray()) and np.array_equal(partly[599].toarray(), faces[599].toarray())
    assert (partly[298] != faces[298]).nnz > 0


def test_the_scale_expressions():
    theta = np.array([10.0, 30.0, 50.0])
    s, mean, d = RC.resistor_scale(theta, [0, 1, 2], [1, 2, 2], [4e-3, 0.0, -1e-3], 25.0, [20.0, 20.0, 30.0], [0.0, 45.0, 50.0])
    assert mean.tolist() == [20.0, 40.0, 50.0] and d.tolist() == [20.0, 5.0, 0.0]
    assert s.tolist() == [1 / (1 + 4e-3 * ((20.0 + 25.0) - 20.0)), 1.0, 1 / (1 + -1e-3 * ((50.0 + 25.0) - 30.0))]


def test_the_strips_of_300_are_the_board_they_were_and_longer_ones_keep_their_shape():
    """strips_system(n): for n = 300 (and by default) the board written out here, value for value; for another n the same
    extras at the same places relative to n, strips that do not overlap, and every stamp on a stored entry."""
    from test_film import strip
    rng = np.random.default_rng(11)
    rows = [("R", i, 300 + i, float(r)) for i, r in zip(range(300), rng.uniform(0.002, 0.02, 300))]
    rows += [("R", 5, 305, 0.004), ("R", 10, 600, 0.003), ("R", 600, 330, 0.006), ("R", 7, 7, 0.01), ("R", 20, 21, 0.005),
             ("R", 322, 20, 0.007)]
    want = ([strip(300, 0.0), strip(300, 200.0)], [2.0, 0.7], 600, 1, rows)
    for got in (RC.strips_system(), RC.strips_system(300)):
        assert got[1:] == want[1:] and len(got[0]) == 2
        for (xy, tri), (xy_want, tri_want) in zip(got[0], want[0]):
            assert xy.tobytes() == xy_want.tobytes() and xy.dtype == xy_want.dtype
            assert tri.tobytes() == tri_want.tobytes() and tri.dtype == tri_want.dtype
    n = 1000
    meshes, sigma, n_vert, n_internal, rows = RC.strips_system(n)
    assert (sigma, n_vert, n_internal, len(rows)) == ([2.0, 0.7], 2 * n, 1, n + 6)
    assert [len(xy) for xy, _tri in meshes] == [n, n] and meshes[0][0][:, 0].max() < meshes[1][0][:, 0].min()
    assert [row[1:3] for row in rows[:n]] == [(i, n + i) for i in range(n)]
    assert [row[1:] for row in rows[n:]] == [(5, n + 5, 0.004), (10, 2 * n, 0.003), (2 * n, n + 30, 0.006), (7, 7, 0.01), (20, 21, 0.005),
                                            (n + 22, 20, 0.007)]
    L0, _r = C.O.assemble_system([(xy, tri, g) for (xy, tri), g in zip(meshes, sigma)], n_internal, rows, 0)
    L0 = sp.csr_matrix(L0)
    L0.sort_indices()
    at = RC.places(L0, [row[1] for row in rows], [row[2] for row in rows])      # (asserts that every entry is stored)
    assert len(at) == 2 * (n + 5) and len({row for row, *_ in at}) == 2 * n + 1


# ---- 2. a via in series with a current source ------------------------------------------------------------------------------

def test_the_series_via_meets_its_closed_form():
    """rho = alpha I^2 R0 Z = 0.3: the loop run until d <= 1e-10 K meets p* and T_r* within 1e-10 relative (the bar of
    test_coupled_host.py for the uniform strip's closed form) plus what the stop leaves: the last solve used the scale of the
    iterate before the last, within d / (1 - rho) of the fixed point, and the last iterate is within d rho / (1 - rho)."""
    current = RC.series_current(0.3)
    prob, meshes, layer_of, _via = RC.series_problem(current)
    B = RC.host_board(prob, meshes, layer_of, RC.series_model(1e-10))
    c0, Z, rho, p, T_r = RC.series_closed_form(B, current)
    out = B.picard(1e-10)
    got_p, got_T = out["heats"][0], out["resistor_mean"][0] + RC.SERIES_AMBIENT
    print("I", current, "c0", c0, "Z", Z, "rho", rho, "p*", p, "T_r*", T_r, "rounds", len(out["increments"]), "p", got_p, "T_r", got_T)
    assert out["converged"] and abs(rho - 0.3) <= 1e-12 and c0 > 1.0 and len(out["increments"]) > 10
    joule = current * current * RC.SERIES_R0
    assert abs(got_p - p) <= 1e-10 * p + RC.COPPER * joule * 1e-10 / (1 - rho)
    assert abs(got_T - T_r) <= 1e-10 * T_r + 1e-10 * rho / (1 - rho)
    # every increment is the resistor's or the copper's: the thermal problem is linear in p, so d_k = d_1 rho^(k-1)
    d = out["increments"]
    assert all(abs(d[k] / d[k - 1] - rho) <= 1e-6 for k in range(1, 8))


def test_the_series_via_runs_away_above_one():
    current = RC.series_current(1.2)
    prob, meshes, layer_of, _via = RC.series_problem(current)
    out = RC.host_board(prob, meshes, layer_of, RC.series_model(1e-6)).picard(1e-6)
    assert out["runaway"] and not out["converged"] and len(out["increments"]) == 4
    assert solver.picard_verdict(out["increments"], 1e-6) == "runaway"


# ---- 3. balance -------------------------------------------------------------------------------------------------------------

def follows(film, **kw):
    return solver.ElectroThermalModel(thermal=solver.ThermalModel(film=film), resistor_coefficient=RC.COPPER, **kw)


@pytest.mark.parametrize("name", sorted(C.COUPLED_BOARDS))
def test_every_round_balances(name):
    """total_loss == total_heat == the power the sources deliver in every round within 1e-12 relative, the bar of
    test_coupled_host.py: the resistors' heat and the sources' power come from the flows at R / s, the resistance of the
    matrix that was solved."""
    film, factor = C.COUPLED_BOARDS[name]
    prob, meshes, layer_of = thermal_board(name)
    B = RC.host_board(prob, meshes, layer_of, follows(film), C.scaled_case(prob, factor))
    assert len(B.R) > 0
    theta, prev_r = np.zeros(B.board.n_pot), np.zeros(len(B.R))
    for k in range(3):
        s, _mean = B.board.scale_of(theta)
        sr, prev_r, _d = B.scale_of(theta, prev_r)
        _V, Pf, theta, flows = B.round(s, sr)
        heat = math.fsum(Pf.tolist() + [f["power"] for row, f in zip(B.board.rows, flows) if row[0] == "R"])
        loss, delivered = math.fsum((B.board.hM * theta[:B.board.n_vert]).tolist()), B.board.delivered(flows)
        print(name, "round", k + 1, "delivered", delivered, "heat", heat, "loss", loss, "s_r", sr.min(), sr.max())
        assert delivered > 0 and (sr < 1.0).all()
        assert abs(heat - delivered) <= 1e-12 * delivered and abs(loss - delivered) <= 1e-12 * delivered


# ---- 4. zero coefficients ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_layer", "problem_mixed"])
def test_zero_coefficients_give_the_bits_of_none(name):
    film, factor = C.COUPLED_BOARDS[name]
    prob, meshes, layer_of = thermal_board(name)
    case = C.scaled_case(prob, factor)
    thermal = solver.ThermalModel(film=film)
    want = C.host_board(prob, meshes, layer_of, solver.ElectroThermalModel(thermal=thermal), case).picard(1e-6)
    resistors = [e for n in prob.networks for e in n.elements if solver.element_kind(e) == "Resistor"]
    for coefficient in (0.0, {e: 0.0 for e in resistors}):
        B = RC.host_board(prob, meshes, layer_of, solver.ElectroThermalModel(thermal=thermal, resistor_coefficient=coefficient), case)
        got = B.picard(1e-6)
        assert got["increments"] == want["increments"] and (got["resistor_scale"] == 1.0).all()
        assert np.array_equal(got["theta"], want["theta"]) and np.array_equal(got["V"], want["V"])
        assert got["flows"] == want["flows"]


# ---- 5. check_electrothermal_model ------------------------------------------------------------------------------------------

def via_problem():
    prob, top = small_problem()
    net = prob.networks[0]
    c = list(net.connections)
    mid = P.NodeID()
    vias = [P.Resistor(a=c[0].node_id, b=mid, resistance=0.01), P.Resistor(a=mid, b=c[1].node_id, resistance=0.02),
            P.Resistor(a=c[0].node_id, b=c[1].node_id, resistance=0.03)]
    net = P.Network(connections=c, elements=list(net.elements) + vias)
    return P.Problem(layers=list(prob.layers), networks=[net]), vias


def test_the_checked_model(monkeypatch):
    monkeypatch.setattr(solver, "get_context", lambda *a, **k: pytest.fail("a device context was asked for"))
    prob, vias = via_problem()
    thermal = solver.ThermalModel(film=1e-5)
    model = lambda **kw: solver.ElectroThermalModel(thermal=thermal, **kw)                                    # noqa: E731
    checked = solver.check_electrothermal_model(prob, model())
    assert checked.resistor_alpha is None and checked.resistor_t0 == 20.0 and not checked.resistors_follow()
    # positional construction is what it was: the new fields come last
    assert solver.ElectroThermalModel(thermal, 1e-3, 30.0, 0.5, 7) == model(temperature_coefficient=1e-3, conductance_temperature=30.0,
                                                                           tolerance=0.5, max_rounds=7)
    checked = solver.check_electrothermal_model(prob, model(resistor_coefficient=3.93e-3, conductance_temperature=30.0))
    assert checked.resistor_alpha == [3.93e-3] * 3 and checked.resistor_t0 == 30.0 and checked.resistors_follow()
    checked = solver.check_electrothermal_model(prob, model(resistor_coefficient=3.93e-3, resistor_temperature=0.0))
    assert checked.resistor_t0 == 0.0 and checked.conductance_temperature == 20.0
    # a mapping names resistors by identity or equality; the others get 0
    twin = P.Resistor(a=vias[2].a, b=vias[2].b, resistance=0.03)
    checked = solver.check_electrothermal_model(prob, model(resistor_coefficient={vias[1]: 1e-3, twin: -2e-4}))
    assert checked.resistor_alpha == [0.0, 1e-3, -2e-4] and checked.resistors_follow()
    checked = solver.check_electrothermal_model(prob, model(resistor_coefficient={}))
    assert checked.resistor_alpha == [0.0] * 3 and not checked.resistors_follow()
    assert not solver.check_electrothermal_model(prob, model(resistor_coefficient=0.0)).resistors_follow()
    # the transient model wraps the steady one
    wrapped = solver.ElectroThermalTransientModel(electrothermal=model(resistor_coefficient={vias[0]: 2e-3}), areal_capacity=3e-3)
    assert solver.check_electrothermal_transient_model(prob, wrapped).electrothermal.resistor_alpha == [2e-3, 0.0, 0.0]
    stranger = P.Resistor(a=vias[0].a, b=vias[2].b, resistance=0.5)
    source = prob.networks[0].elements[0]
    for bad in (dict(resistor_coefficient=float("nan")), dict(resistor_coefficient=float("inf")), dict(resistor_coefficient="copper"),
                dict(resistor_coefficient={vias[0]: float("nan")}), dict(resistor_coefficient={stranger: 1e-3}),
                dict(resistor_coefficient={source: 1e-3}), dict(resistor_coefficient={"via": 1e-3}),
                dict(resistor_coefficient=1e-3, resistor_temperature=float("nan")),
                dict(resistor_coefficient=1e-3, resistor_temperature=float("inf")),
                dict(resistor_coefficient=3.93e-3, resistor_temperature=25.0 + 1 / 3.93e-3),        # 1 + alpha (ambient - T0) = 0
                dict(resistor_coefficient={vias[1]: -1.0}, resistor_temperature=24.0)):             # = 0 for one resistor
        with pytest.raises(ValueError):
            solver.check_electrothermal_model(prob, model(**bad))
        with pytest.raises(ValueError):
            solver.solve_meshed_electrothermal(prob, [], [], model(**bad))
        with pytest.raises(ValueError):
            solver.check_electrothermal_transient_model(prob, solver.ElectroThermalTransientModel(electrothermal=model(**bad),
                                                                                                  areal_capacity=3e-3))

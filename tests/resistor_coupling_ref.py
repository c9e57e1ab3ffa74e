"""Host restatement of the resistor coupling for the tests ("Resistor coupling"), on top of tests/coupled_ref.py
and tests/coupled_transient_ref.py: the scale of a resistor, the sequential updates of its stamps, and the Picard loop and the
semi-implicit stepping with resistors that follow their temperature, with scipy direct solves.

Resistor r has its ends at the unknowns a_r, b_r and was assembled with g_r = 1 / R_r.
 1. scale: mean_r = (theta[a_r] + theta[b_r]) / 2;  s_r = 1 / (1 + alpha_r * ((mean_r + ambient) - t0_r));  d_r = |mean_r -
    prev_r|, prev_r <- mean_r.
 2. places: for every row i a resistor with a_r != b_r touches (ascending i) and every such resistor at i (ascending r), the
    places in the values of the entry (i, the other end) and of the diagonal (i, i).
 3. revalue: behind coupled_ref.revalue, in the order of 2: t_r = (s_r - 1) * g_r; unless t_r == 0.0: val[other] = val[other] +
    t_r; val[diag] = val[diag] - t_r, each a rounded update of the stored value.
 4. a round: the electrical solve on that matrix; the element flows with R_r / s_r for R_r; the rest as coupled_ref.Board.round.
 5. Picard and stepping: as coupled_ref.Board.picard and coupled_transient_ref.run with d = max(max_f d_f, max_r d_r)."""
from __future__ import annotations

import math
import types

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import coupled_ref as C
import coupled_transient_ref as CT
import thermal_ref as T
import transient_ref as R
from padne_amd import solver


def resistor_scale(theta, a, b, alpha, ambient: float, t0, prev):
    """Definition 1: (s, mean, d) per resistor."""
    theta = np.asarray(theta, dtype=np.float64)
    mean = (theta[np.asarray(a, dtype=np.int64)] + theta[np.asarray(b, dtype=np.int64)]) / 2
    s = 1 / (1 + np.asarray(alpha, dtype=np.float64) * ((mean + ambient) - np.asarray(t0, dtype=np.float64)))
    return s, mean, np.abs(mean - np.asarray(prev, dtype=np.float64))


def places(L0, a, b) -> list:
    """Definition 2: [(row, r, place of (row, other end), place of (row, row))]; AssertionError for an entry that is not stored."""
    L0 = sp.csr_matrix(L0)
    assert L0.has_sorted_indices
    inc = []
    for r, (x, y) in enumerate(zip(a, b)):
        if int(x) != int(y):
            inc += [(int(x), r, int(y)), (int(y), r, int(x))]
    inc.sort(key=lambda e: (e[0], e[1]))

    def place(i, j):
        e0, e1 = L0.indptr[i], L0.indptr[i + 1]
        at = e0 + int(np.searchsorted(L0.indices[e0:e1], j))
        assert at < e1 and L0.indices[at] == j, f"entry ({i}, {j}) is not stored"
        return int(at)

    return [(i, r, place(i, j), place(i, i)) for i, r, j in inc]


def revalue_resistors(L, at, s, g) -> sp.csr_matrix:
    """Definition 3 on a csr matrix with sorted indices: a copy with the updates applied."""
    out = sp.csr_matrix(L).copy()
    data = out.data
    s, g = np.asarray(s, dtype=np.float64), np.asarray(g, dtype=np.float64)
    for _row, r, other, diag in at:
        t = (s[r] - 1) * g[r]
        if t == 0.0:
            continue
        data[other] = data[other] + t
        data[diag] = data[diag] - t
    return out


class ResistorBoard:
    """A coupled_ref.Board whose resistors follow their temperature: ``alpha`` per ("R", ...) row of ``board.rows`` in order,
    ``t0`` one float for all."""

    def __init__(self, board: C.Board, alpha, t0: float):
        self.board = board
        self.at_row = [i for i, row in enumerate(board.rows) if row[0] == "R"]
        self.a = np.array([board.rows[i][1] for i in self.at_row], dtype=np.int64)
        self.b = np.array([board.rows[i][2] for i in self.at_row], dtype=np.int64)
        self.R = np.array([board.rows[i][3] for i in self.at_row], dtype=np.float64)
        self.g = 1 / self.R
        self.alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
        assert self.alpha.shape == self.R.shape
        self.t0 = np.full(len(self.R), float(t0))
        self.places = places(board.L0, self.a, self.b)

    def scale_of(self, theta, prev):
        return resistor_scale(theta, self.a, self.b, self.alpha, self.board.ambient, self.t0, prev)

    def matrix(self, s, sr):
        B = self.board
        return revalue_resistors(C.revalue(B.L0, B.xy, B.tri, B.face_mesh, B.sigma, s), self.places, sr, self.g)

    def rows_used(self, sr) -> list:
        rows = list(self.board.rows)
        for i, R_r, s_r in zip(self.at_row, self.R.tolist(), np.asarray(sr, dtype=np.float64).tolist()):
            rows[i] = rows[i][:3] + (R_r / s_r,)
        return rows

    def electrical(self, s, sr, extra=None):
        """(V, P, flows, b) of the face scale ``s`` and the resistor scale ``sr``."""
        B = self.board
        V = spla.spsolve(sp.csc_matrix(self.matrix(s, sr)), B.r)
        P = C.face_power(B.xy, B.tri, B.face_mesh, B.sigma, s, V[:B.n_vert])
        flows = solver.element_flows(self.rows_used(sr), V)
        heat = []
        if B.element_heat:
            for row, flow in zip(B.rows, flows):
                if row[0] == "R":
                    heat += [(row[1], flow["power"] / 2), (row[2], flow["power"] / 2)]
        b = T.load(B.n_pot, B.tri, P, heat)
        if extra is not None:
            b = b + extra
        return V, P, flows, b

    def round(self, s, sr):
        V, P, flows, b = self.electrical(s, sr)
        return V, P, T.solve(self.board.A, b), flows

    def picard(self, tolerance: float, max_rounds: int = 200):
        """coupled_ref.Board.picard with the resistors: also ``resistor_scale`` (the used one), ``resistor_mean`` (of the last
        theta) and ``heats`` (the resistors' watts) of the last round."""
        B = self.board
        theta = np.zeros(B.n_pot)
        s, prev = B.scale_of(theta)
        sr, prev_r, _d = self.scale_of(theta, np.zeros(len(self.R)))
        increments, thetas, verdict = [], [], None
        for _ in range(max_rounds):
            used, used_r = s, sr
            V, P, theta, flows = self.round(used, used_r)
            s, mean = B.scale_of(theta)
            sr, mean_r, d_r = self.scale_of(theta, prev_r)
            increments.append(max(float(np.abs(mean - prev).max()), float(d_r.max()) if len(d_r) else 0.0))
            prev, prev_r = mean, mean_r
            thetas.append(theta)
            verdict = solver.picard_verdict(increments, tolerance)
            if verdict is not None:
                break
        return dict(V=V, P=P, theta=theta, flows=flows, scale=used, resistor_scale=used_r, resistor_mean=mean_r,
                    increments=increments, thetas=thetas, converged=verdict == "converged", runaway=verdict == "runaway",
                    heats=[f["power"] for row, f in zip(B.rows, flows) if row[0] == "R"])

    def run(self, areal_capacity, schedule, *, initial=False, tolerance=0.01, max_rounds=200):
        """coupled_transient_ref.run with the resistors, ``schedule`` = (dt, n_steps, on): a namespace over time (entry 0 the
        start) of ``states``, ``increments``, ``resistor_min`` / ``resistor_max`` (the used s_r), ``delivered`` and ``heat``."""
        B = self.board
        stepper = R.Stepper(B.A, CT.capacity(B, areal_capacity))
        nan = float("nan")
        theta, prev, prev_r = np.zeros(B.n_pot), np.zeros(len(B.tri)), np.zeros(len(self.R))
        states, increments, lo, hi, delivered, heat = [theta], [0.0], [nan], [nan], [0.0], [0.0]
        if initial:
            start = self.picard(tolerance, max_rounds)
            theta = start["theta"]
            _s, prev = B.scale_of(theta)
            _sr, prev_r, _d = self.scale_of(theta, prev_r)
            states, increments = [theta], [start["increments"][-1]]
            lo, hi = [float(start["resistor_scale"].min())], [float(start["resistor_scale"].max())]
            delivered = [B.delivered(start["flows"])]
            heat = [delivered[0]]
        for dt, n_steps, on in schedule:
            for _ in range(int(n_steps)):
                if on:
                    s, mean = B.scale_of(theta)
                    sr, mean_r, d_r = self.scale_of(theta, prev_r)
                    increments.append(max(float(np.abs(mean - prev).max()), float(d_r.max())))
                    prev, prev_r = mean, mean_r
                    _V, _P, flows, b = self.electrical(s, sr)
                    theta = stepper.step(theta, dt, b)
                    lo.append(float(sr.min()))
                    hi.append(float(sr.max()))
                    delivered.append(B.delivered(flows))
                    heat.append(math.fsum(b.tolist()))
                else:
                    theta = stepper.step(theta, dt, None)
                    increments.append(nan)
                    lo.append(nan)
                    hi.append(nan)
                    delivered.append(0.0)
                    heat.append(0.0)
                states.append(theta)
        return types.SimpleNamespace(states=np.stack(states), increments=np.array(increments), resistor_min=np.array(lo),
                                     resistor_max=np.array(hi), delivered=np.array(delivered), heat=np.array(heat))


def host_board(prob, meshes, layer_of, model, case=None) -> ResistorBoard:
    """The :class:`ResistorBoard` of a Problem on its meshes for an ElectroThermalModel and one load case."""
    checked = solver.check_electrothermal_model(prob, model)
    board = C.host_board(prob, meshes, layer_of, model, case)
    n_res = sum(1 for row in board.rows if row[0] == "R")
    alpha = [0.0] * n_res if checked.resistor_alpha is None else checked.resistor_alpha
    return ResistorBoard(board, alpha, checked.resistor_t0)


# ---- the boards of the tests ----------------------------------------------------------------------------------------------

COPPER = solver.COPPER_TEMPERATURE_COEFFICIENT


def strips_system(n: int = 300):
    """(meshes, sigma, n_vert, n_internal, element rows): two triangle strips of ``n`` vertices (tests/test_film.py's
    ``strip``), the second one beyond the end of the first, joined vertex to vertex by ``n`` resistors -- with the internal
    node 2 n + 1 touched rows; for n = 300 two full tiles of the row kernel and a ragged one -- and: a second resistor on the
    pair of vertex 5, a chain 10 - internal node - (n + 30), a resistor with both ends on vertex 7, and vertex 20 with three
    resistors, one of them along the mesh edge 20 - 21 (an entry the faces write too), one given from its higher end.
    n + 6 resistors, 2 (n + 5) incidences."""
    from test_film import strip
    n = int(n)
    assert n > 30
    meshes = [strip(n, 0.0), strip(n, max(200.0, 0.5 * n))]      # (a strip of n vertices is n / 4 + 0.2 long)
    n_vert = 2 * n
    rng = np.random.default_rng(11)
    rows = [("R", i, n + i, float(r)) for i, r in zip(range(n), rng.uniform(0.002, 0.02, n))]
    rows += [("R", 5, n + 5, 0.004), ("R", 10, n_vert, 0.003), ("R", n_vert, n + 30, 0.006), ("R", 7, 7, 0.01), ("R", 20, 21, 0.005),
             ("R", n + 22, 20, 0.007)]
    return meshes, [2.0, 0.7], n_vert, 1, rows


def resistor_stamps(rows):
    """(rows, cols, vals) of the resistors' four stamps each, g = 1 / R with one division: -g at (a, a), +g at (a, b), -g at
    (b, b), +g at (b, a)."""
    a = np.array([row[1] for row in rows], dtype=np.int64)
    b = np.array([row[2] for row in rows], dtype=np.int64)
    g = 1 / np.array([row[3] for row in rows], dtype=np.float64)
    return (np.stack([a, a, b, b], 1).reshape(-1), np.stack([a, b, b, a], 1).reshape(-1), np.stack([-g, g, -g, g], 1).reshape(-1))


SERIES_R0, SERIES_SIGMA, SERIES_FILM, SERIES_AMBIENT, SERIES_T0 = 0.05, (200.0, 100.0), 1e-3, 25.0, 20.0


def series_problem(current: float, voltage=None):
    """(problem, meshes, layer_of, the resistor): two strips of 40 vertices on two layers joined by ONE resistor between their
    vertices 20, and a current source from vertex 0 of the upper strip to vertex 39 of the lower one: all of ``current`` passes
    through the resistor whatever its value.  With ``voltage`` a voltage source across the resistor takes the current
    source's place: the resistor's drop is held instead."""
    import helpers as H
    from padne_amd import mesh, problem as P
    from test_film import strip
    layers = [P.Layer(shape=H.Geoms(1), name=name, conductance=sigma) for name, sigma in zip(("F.Cu", "B.Cu"), SERIES_SIGMA)]
    meshes = [mesh.Mesh(np.asarray(xy, dtype=np.float64), np.asarray(tri, dtype=np.int32)) for xy, tri in (strip(40, 0.0), strip(40, 0.0))]
    at = lambda layer_i, v: P.Connection(layer=layers[layer_i], point=H.XY(*meshes[layer_i].points[v]))      # noqa: E731
    c = [at(0, 0), at(1, 39), at(0, 20), at(1, 20)]
    via = P.Resistor(a=c[2].node_id, b=c[3].node_id, resistance=SERIES_R0)
    source = P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=float(current)) if voltage is None else \
        P.VoltageSource(p=c[2].node_id, n=c[3].node_id, voltage=float(voltage))
    net = P.Network(connections=c, elements=[source, via])
    return P.Problem(layers=layers, networks=[net]), meshes, [0, 1], via


def series_model(tolerance: float, **kw):
    """Copper that keeps its conductance and a via with copper's coefficient."""
    return solver.ElectroThermalModel(thermal=solver.ThermalModel(film=SERIES_FILM, ambient=SERIES_AMBIENT),
                                      temperature_coefficient=0.0, conductance_temperature=SERIES_T0, tolerance=tolerance,
                                      resistor_coefficient=COPPER, **kw)


def series_closed_form(board: "ResistorBoard", current: float):
    """(c0, Z, rho, p*, T_r*) of the series board: with the copper's heat fixed and the thermal problem linear in the
    resistor's heat p, mean_r = c0 + Z p from two linear solves, rho = alpha I^2 R0 Z, and the fixed point of p = I^2 R0 (1 +
    alpha (ambient + c0 + Z p - T0)) is p* = I^2 R0 (1 + alpha (ambient + c0 - T0)) / (1 - rho), T_r* = ambient + c0 + Z p*."""
    B = board.board
    _V, P, _flows, _b = board.electrical(np.ones(len(B.tri)), np.ones(len(board.R)))
    a, b = int(board.a[0]), int(board.b[0])
    mean = lambda theta: (theta[a] + theta[b]) / 2                                                            # noqa: E731
    c0 = mean(T.solve(B.A, T.load(B.n_pot, B.tri, P, [])))
    Z = mean(T.solve(B.A, T.load(B.n_pot, B.tri, np.zeros(len(B.tri)), [(a, 0.5), (b, 0.5)])))
    alpha, joule = float(board.alpha[0]), current * current * SERIES_R0
    rho = alpha * joule * Z
    p = joule * (1 + alpha * ((B.ambient + c0) - SERIES_T0)) / (1 - rho)
    return c0, Z, rho, p, B.ambient + c0 + Z * p


def series_current(rho: float) -> float:
    """The current at which alpha I^2 R0 Z = ``rho`` (Z does not depend on the current)."""
    prob, meshes, layer_of, _via = series_problem(1.0)
    _c0, Z, _rho, _p, _T = series_closed_form(host_board(prob, meshes, layer_of, series_model(1e-6)), 1.0)
    return math.sqrt(rho / (COPPER * SERIES_R0 * Z))

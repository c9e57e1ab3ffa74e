"""Host restatement of the film curves for the tests ("Film curves"), on top of tests/thermal_ref.py,
tests/coupled_ref.py (the host board and its electrical round), tests/stack_ref.py (the stacked operator) and
tests/sources_ref.py (the heat sources' load), in the order of operations the device states.  numpy contracts nothing, so
every term is the device's bit for bit.

A table is (rise, film): h = film[i] at the knots rise[i], rise[0] == 0, ascending; linear between the knots, held constant
below the first and above the last.  ``tables`` lists one per mesh.
 1. slopes: s_i = (film[i + 1] - film[i]) / (rise[i + 1] - rise[i]) for i < n - 1, and 0 at the last knot.
 2. segment of theta: the largest i with rise[i] <= theta, 0 when there is none; s = s_i, but s = 0 when not theta >= rise[0].
 3. terms at vertex v of mesh m with theta = theta_v:
        h = film[i] + s * (theta - rise[i]);  g = h + s * theta;  c = ((s * theta) * theta) * M_v;  hM = h * M_v
    beyond = the number of vertices with theta > rise[-1] on tables of more than one knot.
 4. diagonal of the round: D0_v + (g * M_v - hM0_v), D0 the diagonal of the operator with the constant film film[0], hM0 =
    film[0] * M_v (thermal_ref.operator's).  Every other entry is the operator's.
 5. Newton: theta_0 = 0; round k + 1 solves (definition 4 at theta_k) theta_{k+1} = b + c(theta_k) by a scipy direct solve;
    d_{k+1} = max_v |theta_{k+1} - theta_k| over the vertices; the loop ends at d <= tolerance.
 6. with the electro-thermal coupling (coupled_ref, definition 6) the same loop also revalues the electrical system with the
    scale of theta_k, takes b from its solve, and d is the larger of the film's and the coupling's increment.
 7. uniform plate: with b_v = p M_v the solution is the constant theta* with h(theta*) theta* = p, found segment by segment
    from the quadratic s theta^2 + (h_i - s t_i) theta - p = 0 in the form 2 p / (B + sqrt(B^2 + 4 s p)), B = h_i - s t_i."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import coupled_ref as C
import fold_ref
import sources_ref as Q
import stack_ref as K
import thermal_ref as T
from padne_amd import solver


def table_of(curve) -> tuple:
    """(rise, film) of a FilmCurve, or the one-knot table of a float."""
    if isinstance(curve, solver.FilmCurve):
        return np.asarray(curve.rise, dtype=np.float64), np.asarray(curve.film, dtype=np.float64)
    return np.array([0.0]), np.array([float(curve)])


def tables_of(checked, layer_of) -> list:
    """The table of every mesh for a CheckedThermalModel."""
    curves = checked.film_curves or [None] * len(checked.film)
    return [table_of(checked.film[l] if curves[l] is None else curves[l]) for l in layer_of]


def slopes(rise, film) -> np.ndarray:
    """Definition 1."""
    s = np.zeros(len(rise))
    s[:-1] = (film[1:] - film[:-1]) / (rise[1:] - rise[:-1])
    return s


def terms(tables, voff, M, theta):
    """Definitions 2 and 3 for theta (n_vert,): (g, c, hM, beyond)."""
    theta = np.asarray(theta, dtype=np.float64)
    g, c, hM, beyond = np.empty_like(theta), np.empty_like(theta), np.empty_like(theta), 0
    for m, (rise, film) in enumerate(tables):
        lo, hi = int(voff[m]), int(voff[m + 1])
        th, mv = theta[lo:hi], M[lo:hi]
        i = np.clip(np.searchsorted(rise, th, side="right") - 1, 0, len(rise) - 1)
        with np.errstate(invalid="ignore"):
            s = np.where(th >= rise[0], slopes(rise, film)[i], 0.0)
            h = film[i] + s * (th - rise[i])
            g[lo:hi] = h + s * th
            c[lo:hi] = ((s * th) * th) * mv
            hM[lo:hi] = h * mv
            if len(rise) > 1:
                beyond += int((th > rise[-1]).sum())
    return g, c, hM, beyond


def increment(voff, theta, lin) -> tuple:
    """(d, vertex) of definition 5 in the kernels' own order (fold_ref, definitions 2 and 3): every mesh's vertices in tiles of
    256 of that mesh, a lane without a vertex carrying (-inf, NO_INDEX); then one fold over the tiles of all meshes in mesh
    order.  The value is max_v |theta[v] - lin[v]| and the vertex the lowest that attains it; (0.0, -1) without vertices."""
    theta, lin = np.asarray(theta, dtype=np.float64), np.asarray(lin, dtype=np.float64)
    empty = (-np.inf, fold_ref.NO_INDEX)
    values, vertices = [np.zeros(0)], [np.zeros(0, dtype=np.int64)]
    for m in range(len(voff) - 1):
        lo, hi = int(voff[m]), int(voff[m + 1])
        v, f = fold_ref.tile_tops(np.abs(theta[lo:hi] - lin[lo:hi]), np.arange(lo, hi, dtype=np.int64), empty=empty)
        values.append(v)
        vertices.append(f)
    d, vertex = fold_ref.fold_top(np.concatenate(values), np.concatenate(vertices), empty=empty)
    return (0.0, -1) if vertex == fold_ref.NO_INDEX else (d, vertex)


def linearised(A0, M, hM0, tables, voff, theta) -> sp.csr_matrix:
    """Definition 4: the operator of the round about theta (n_vert,), with A0's pattern."""
    A = sp.csr_matrix(A0).copy()
    A.sort_indices()
    g, _c, _hM, _ = terms(tables, voff, M, theta)
    n_vert = len(M)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    at = np.flatnonzero((rows == A.indices) & (rows < n_vert))
    assert len(at) == n_vert
    A.data[at] = A.data[at] + (g * M - hM0)
    return A


def newton(A0, M, hM0, tables, voff, b, tolerance: float, max_rounds: int = 50) -> dict:
    """Definition 5 for the load b (n_pot,): theta, the increments, the vertex of each, ``converged``, ``thetas``, and hM and
    beyond at the last iterate."""
    n_vert = len(M)
    theta = np.zeros(A0.shape[0])
    increments, vertices, thetas, converged = [], [], [], False
    for _ in range(max_rounds):
        _g, c, _hM, _ = terms(tables, voff, M, theta[:n_vert])
        rhs = np.array(b, dtype=np.float64)
        rhs[:n_vert] = rhs[:n_vert] + c
        new = T.solve(linearised(A0, M, hM0, tables, voff, theta[:n_vert]), rhs)
        moved = np.abs(new[:n_vert] - theta[:n_vert])
        increments.append(float(moved.max()))
        vertices.append(int(np.argmax(moved)))
        theta = new
        thetas.append(theta)
        if increments[-1] <= tolerance:
            converged = True
            break
    _g, _c, hM, beyond = terms(tables, voff, M, theta[:n_vert])
    return dict(theta=theta, increments=increments, vertices=vertices, converged=converged, thetas=thetas, hM=hM, beyond=beyond)


def electrical_round(B: C.Board, s):
    """(V, P, flows, b) of coupled_ref.Board with the scale s: the electrical solve and the load it puts on the copper."""
    L = C.revalue(B.L0, B.xy, B.tri, B.face_mesh, B.sigma, s)
    V = spla.spsolve(sp.csc_matrix(L), B.r)
    P = C.face_power(B.xy, B.tri, B.face_mesh, B.sigma, s, V[:B.n_vert])
    flows = solver.element_flows(B.rows, V)
    heat = []
    if B.element_heat:
        for row, flow in zip(B.rows, flows):
            if row[0] == "R":
                heat += [(row[1], flow["power"] / 2), (row[2], flow["power"] / 2)]
    return V, P, flows, T.load(B.n_pot, B.tri, P, heat)


def coupled_newton(B: C.Board, tables, tolerance: float, max_rounds: int = 50, A0=None, extra=None, coupled: bool = True) -> dict:
    """Definitions 5 and 6 on a coupled_ref.Board: ``A0`` the operator in the place of B.A (the stacked one), ``extra`` a load
    added to every round's b (the heat sources').  ``coupled`` False: alpha taken as 0, one electrical solve."""
    A0 = B.A if A0 is None else A0
    theta = np.zeros(B.n_pot)
    ones = np.ones(len(B.tri))
    s, prev = B.scale_of(theta) if coupled else (ones, None)
    increments, film_increments, verdict, fixed = [], [], None, None
    for _ in range(max_rounds):
        if coupled or fixed is None:
            fixed = electrical_round(B, s)
        V, P, flows, b = fixed
        used = s
        _g, c, _hM, _ = terms(tables, B.voff, B.M, theta[:B.n_vert])
        rhs = b if extra is None else b + extra
        rhs = np.array(rhs, dtype=np.float64)
        rhs[:B.n_vert] = rhs[:B.n_vert] + c
        new = T.solve(linearised(A0, B.M, B.hM, tables, B.voff, theta[:B.n_vert]), rhs)
        d = float(np.abs(new[:B.n_vert] - theta[:B.n_vert]).max())
        film_increments.append(d)
        if coupled:
            s, mean = B.scale_of(new)
            d = max(d, float(np.abs(mean - prev).max()))
            prev = mean
        theta = new
        increments.append(d)
        verdict = solver.picard_verdict(increments, tolerance)
        if verdict is not None:
            break
    _g, _c, hM, beyond = terms(tables, B.voff, B.M, theta[:B.n_vert])
    return dict(V=V, P=P, flows=flows, theta=theta, scale=used, increments=increments, film_increments=film_increments,
                converged=verdict == "converged", hM=hM, beyond=beyond)


def stacked_operator(B: C.Board, mesh_layer, kappa, film, links, pairs) -> sp.csr_matrix:
    """A' of stack_ref for the meshes of a coupled_ref.Board."""
    return K.operator(B.meshes, mesh_layer, kappa, film, B.n_pot - B.n_vert, links, pairs)[0]


def source_load(B: C.Board, mesh_layer, sources, power) -> np.ndarray:
    """What the heat sources (layer, polygon) with ``power`` (n_source,) add to b (sources_ref, definition 5)."""
    area = T.face_area(B.xy, B.tri)
    ptr, face, _flags = Q.lists(B.meshes, mesh_layer, sources)
    return Q.load(B.n_pot, B.tri, area, ptr, face, Q.areas(area, ptr, face), np.asarray(power, dtype=np.float64))


def defect_bound(tables, voff, M, d: float) -> float:
    """d * sum_v M_v (g_max - g_min) over every mesh's table: what the linearisation of the last round, a step of d, can
    leave between the film loss and the heat put in.  g = q' ranges over both ends of every segment and the clamped film."""
    total = 0.0
    for m, (rise, film) in enumerate(tables):
        s = slopes(rise, film)
        ends = [film[-1]]
        for i in range(len(rise) - 1):
            ends += [film[i] + s[i] * (2 * rise[i] - rise[i]), film[i] + s[i] * (2 * rise[i + 1] - rise[i])]
        total += math.fsum(M[int(voff[m]):int(voff[m + 1])].tolist()) * (max(ends) - min(ends))
    return d * total


def plate_root(rise, film, p: float) -> float:
    """Definition 7: the theta >= 0 with h(theta) theta = p, p >= 0."""
    rise, film = np.asarray(rise, dtype=np.float64), np.asarray(film, dtype=np.float64)
    s = slopes(rise, film)
    for i in range(len(rise) - 1):
        if p <= film[i + 1] * rise[i + 1]:                  # q is increasing: the root lies in this segment
            big_b = film[i] - s[i] * rise[i]
            return 2 * p / (big_b + math.sqrt(big_b * big_b + 4 * s[i] * p))
    return p / film[-1]


# ---- the curves and boards of the tests ------------------------------------------------------------------------------------

def kinked_curve() -> solver.FilmCurve:
    """A rising curve with a kink at 16 K; with p = KINK_POWER the plate's root lies exactly on that knot."""
    return solver.FilmCurve([0.0, 16.0, 64.0], [1e-3, 2e-3, 2.5e-3])


KINK_POWER = 2e-3 * 16.0


def plate_curves() -> dict:
    """name -> (curve, p): the three curves of the uniform plate, with mesh units of mm and rises of tens of kelvin."""
    return {"natural_convection": (solver.FilmCurve.natural_convection(4e-4, upto=200.0), 0.05),
            "radiation": (solver.FilmCurve.radiation(5.67e-14 * 170, 298.15, upto=200.0), 0.05),
            "kink": (kinked_curve(), KINK_POWER)}


def board_curve(h0: float = 1e-3, upto: float = 400.0) -> solver.FilmCurve:
    """The rising curve of the board tests: natural convection on top of a constant part, h(0) = h0 and about 2.3 h0 at
    ``upto``; 17 knots."""
    return solver.FilmCurve.natural_convection(0.4 * h0, upto=upto, knots=17) + h0 * (1 - 0.4 * (upto / 256) ** 0.25)


# name -> (the board of tests/test_thermal.py, the factor on every source of the Problem: rises of tens of kelvin, and host
# increments that stay clear of the tolerance of the device tests (tests/test_film_host.py); what the ThermalModel gets
# beside its film)
FILM_BOARDS = {"two_layer": ("two_layer", 0.2, dict(interlayer={("F.Cu", "B.Cu"): 1.5e-3})),
               "problem_many_meshes": ("problem_many_meshes", 0.3, {}),
               "single_source": ("single", 0.3, dict(heat_sources=[solver.HeatSource.rectangle("F.Cu", 2.0, 2.0, 5.0, 5.0, 0.4)]))}


def board_model(name: str, **kw) -> solver.ThermalModel:
    """The ThermalModel of a board of FILM_BOARDS: a curve on every layer; on two_layer a curve on top and a float below."""
    film = {"F.Cu": board_curve(), "B.Cu": 1.2e-3} if name == "two_layer" else board_curve()
    return solver.ThermalModel(film=film, **dict(FILM_BOARDS[name][2], **kw))


def host_spec(name: str, alpha: float = 0.0, **model_kw):
    """What the host loop of a board of FILM_BOARDS needs: a namespace of the Problem ``prob``, ``meshes``, ``layer_of``, the
    ``model`` (ThermalModel), the load ``case``, the coupled_ref.Board ``B`` (its A and hM those of the films h(0)), the
    ``tables`` per mesh, ``A0`` (stacked with interlayer pairs) and ``extra`` (the heat sources' load, or None)."""
    import types

    import test_thermal as TT
    base, factor, _kw = FILM_BOARDS[name]
    prob, meshes, layer_of, *_ = TT.board(base)
    model = board_model(name, **model_kw)
    electro = solver.ElectroThermalModel(thermal=model, temperature_coefficient=alpha)
    case = C.scaled_case(prob, factor)
    B = C.host_board(prob, meshes, layer_of, electro, case)
    checked = solver.check_thermal_model(prob, model)
    tables = tables_of(checked, layer_of)
    A0, extra = B.A, None
    if checked.interlayer:
        links = [(row[1], row[2], checked.links[element]) for element, row in TT.board(base)[6] if row[0] == "R"]
        A0 = stacked_operator(B, layer_of, [checked.kappa[l] for l in layer_of], [checked.film[l] for l in layer_of], links,
                              checked.interlayer)
    if checked.sources:
        extra = source_load(B, layer_of, [(s.layer, np.asarray(s.polygon)) for s in checked.sources],
                            [s.power[0] if isinstance(s.power, tuple) else s.power for s in checked.sources])      # (case 0)
    return types.SimpleNamespace(prob=prob, meshes=meshes, layer_of=layer_of, model=model, case=case, B=B, tables=tables, A0=A0,
                                 extra=extra, checked=checked)


def spec_newton(spec, tolerance: float, max_rounds: int = 50, coupled: bool = False) -> dict:
    """The host loop of a :func:`host_spec`."""
    return coupled_newton(spec.B, spec.tables, tolerance, max_rounds, A0=spec.A0, extra=spec.extra, coupled=coupled)

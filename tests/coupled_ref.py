"""Host restatement of the electro-thermal coupling for the tests ("Electro-thermal"), on top of
tests/thermal_ref.py: the scale, the revalued electrical system, the scaled face powers and power densities, and the Picard
loop with scipy direct solves.

Faces are visited with the corners (g1, g2, g3) = (tri[2], tri[0], tri[1]) like the device.
 1. scale: mean_f = ((theta_1 + theta_2) + theta_3) / 3;  s_f = 1 / (1 + alpha_m * ((mean_f + ambient) - T0)).
 2. weights: w12 = cot_half(p1, p2, p3), w23 = cot_half(p2, p3, p1), w31 = cot_half(p3, p1, p2), |cot|/2 of the corner opposite
    the edge (thermal_ref.face_power's).
 3. revalue: t_f = (s_f - 1) * sigma_m.  For every vertex v and every face f incident to it, in ascending face number, with (a,
    w_a, b, w_b) = (g2, w12, g3, w31) if v is g1, (g3, w23, g1, w12) if v is g2, (g1, w31, g2, w23) if v is g3:
    c_a = t_f * w_a, c_b = t_f * w_b;  acc[v, a] += c_a;  acc[v, b] += c_b;  acc[v, v] = (acc[v, v] - c_a) - c_b, every acc
    starting at 0.0.  Then L[v, j] = L0[v, j] + acc[v, j] for every stored entry of a vertex row; a contribution to an entry
    that is not stored must be exactly 0 (an edge whose weights are all 0).  Other rows are L0's.
 4. face powers: thermal_ref.face_power with the one product sigma_m * s_f for sigma.
 5. power density: the reference's sigma |grad V|^2 of the face, then one product with s_f.
 6. Picard: theta_0 = 0 and previous means 0; round k: revalue with s^(k-1), V_k = the direct solve, P with s^(k-1), the
    resistors' heat from V_k, theta_k = the direct thermal solve, d_k = max_f |mean_k,f - mean_k-1,f|, s^(k) by 1."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import thermal_ref as T
from oracle import padne_oracle as O
from padne_amd import solver


def face_means(tri, theta) -> np.ndarray:
    c = T.corners(tri)
    theta = np.asarray(theta, dtype=np.float64)
    return ((theta[c[:, 0]] + theta[c[:, 1]]) + theta[c[:, 2]]) / 3


def scale(tri, face_mesh, alpha, ambient: float, t0: float, theta):
    """Definition 1: (s, mean) per face; ``alpha`` per mesh."""
    mean = face_means(tri, theta)
    a = np.asarray(alpha, dtype=np.float64)[face_mesh]
    return 1 / (1 + a * ((mean + ambient) - t0)), mean


def weights(xy, tri):
    """Definition 2: (w12, w23, w31) per face."""
    c = T.corners(tri)
    p1, p2, p3 = xy[c[:, 0]], xy[c[:, 1]], xy[c[:, 2]]

    def cot_half(pi, pk, po):
        vix, viy = pi[:, 0] - po[:, 0], pi[:, 1] - po[:, 1]
        vkx, vky = pk[:, 0] - po[:, 0], pk[:, 1] - po[:, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.abs((vix * vkx + viy * vky) / (vix * vky - viy * vkx)) / 2

    return cot_half(p1, p2, p3), cot_half(p2, p3, p1), cot_half(p3, p1, p2)


def corrections(xy, tri, face_mesh, sigma, s):
    """Definition 3's accumulators: (rows, cols, acc) of the off-diagonal entries, one triple per directed edge in no
    particular order, and acc_d (n_vert,) of the diagonal.  np.add.at visits its index array front to back, so with the
    contributions listed face by face every accumulator sums in ascending face number from 0.0."""
    c = T.corners(tri)
    w12, w23, w31 = weights(xy, tri)
    tf = (np.asarray(s, dtype=np.float64) - 1) * np.asarray(sigma, dtype=np.float64)[face_mesh]
    n = len(xy)
    # per face and corner position (v = g1, g2, g3): the neighbours (a, b) and their weights
    v = c                                                                   # (n_tri, 3)
    a = np.stack([c[:, 1], c[:, 2], c[:, 0]], axis=1)
    b = np.stack([c[:, 2], c[:, 0], c[:, 1]], axis=1)
    ca = tf[:, None] * np.stack([w12, w23, w31], axis=1)
    cb = tf[:, None] * np.stack([w31, w12, w23], axis=1)
    # off-diagonal: key (v, j); per face the pair (v, a) then (v, b) of every corner -- different keys, so only the face
    # order matters
    keys = np.stack([v * n + a, v * n + b], axis=2).reshape(-1)
    vals = np.stack([ca, cb], axis=2).reshape(-1)
    uniq, inverse = np.unique(keys, return_inverse=True)
    acc = np.zeros(len(uniq))
    np.add.at(acc, inverse, vals)
    # diagonal: per vertex (acc - c_a) - c_b face after face
    acc_d = np.zeros(n)
    np.subtract.at(acc_d, np.repeat(v.reshape(-1), 2), vals)
    return uniq // n, uniq % n, acc, acc_d


def revalue(L0, xy, tri, face_mesh, sigma, s) -> sp.csr_matrix:
    """Definition 3: L0 (csr, sorted indices) revalued, same pattern."""
    L0 = sp.csr_matrix(L0)
    assert L0.has_sorted_indices
    n = len(xy)
    rows, cols, acc, acc_d = corrections(xy, tri, face_mesh, sigma, s)
    add = np.zeros(L0.nnz)
    row_of = np.repeat(np.arange(L0.shape[0]), np.diff(L0.indptr))
    key0 = row_of.astype(np.int64) * L0.shape[1] + L0.indices
    key = np.concatenate([rows * L0.shape[1] + cols, np.arange(n, dtype=np.int64) * (L0.shape[1] + 1)])
    val = np.concatenate([acc, acc_d])
    at = np.searchsorted(key0, key)
    at_ok = np.minimum(at, L0.nnz - 1)
    stored = key0[at_ok] == key
    assert (val[~stored] == 0.0).all(), "a contribution that is not 0 has no stored entry"
    add[at_ok[stored]] = val[stored]
    out = L0.copy()
    vertex_rows = row_of < n
    out.data[vertex_rows] = L0.data[vertex_rows] + add[vertex_rows]
    return out


def fresh_assembly(n: int, xy, tri, conductance) -> sp.csr_matrix:
    """The stiffness with a conductance per face, reference sign, summed by scipy (another order than definition 3)."""
    c = T.corners(tri)
    w12, w23, w31 = weights(xy, tri)
    g = np.asarray(conductance, dtype=np.float64)
    i = np.concatenate([c[:, 0], c[:, 1], c[:, 1], c[:, 2], c[:, 2], c[:, 0]])
    j = np.concatenate([c[:, 1], c[:, 0], c[:, 2], c[:, 1], c[:, 0], c[:, 2]])
    w = np.concatenate([g * w12, g * w12, g * w23, g * w23, g * w31, g * w31])
    K = sp.coo_matrix((w, (i, j)), shape=(n, n)).tocsr()
    return (K - sp.diags(np.asarray(K.sum(axis=1)).reshape(-1))).tocsr()


def face_power(xy, tri, face_mesh, sigma, s, V) -> np.ndarray:
    """Definition 4."""
    per_face = np.asarray(sigma, dtype=np.float64)[face_mesh] * np.asarray(s, dtype=np.float64)
    return T.face_power(xy, tri, np.arange(len(tri)), per_face, V)


def power_density(meshes, sigma, s, V) -> np.ndarray:
    """Definition 5; ``meshes`` as (xy, local tri) tuples."""
    out, off = [], 0
    for (xy, tri, *_), sig in zip(meshes, sigma):
        out.append(O.power_density(xy, tri, V[off:off + len(xy)], float(sig)))
        off += len(xy)
    return np.concatenate(out) * np.asarray(s, dtype=np.float64)


class Board:
    """The electrical and the thermal system of a board on the host: ``meshes`` (xy, local tri) tuples, ``sigma``, ``kappa``,
    ``film`` and ``alpha`` per mesh, ``rows`` the element rows of solver.global_elements, ``links`` (a, b, g) of the thermal
    handle."""

    def __init__(self, meshes, sigma, n_internal, rows, ground, kappa, film, links, alpha, ambient, t0, element_heat=True):
        self.meshes, self.sigma, self.rows = [(m[0], m[1]) for m in meshes], list(sigma), list(rows)
        self.xy, self.tri, self.face_mesh, self.voff, self.toff = T.flatten(self.meshes)
        self.n_vert, self.n_pot = len(self.xy), len(self.xy) + int(n_internal)
        L0, self.r = O.assemble_system([(xy, tri, s) for (xy, tri), s in zip(self.meshes, sigma)], n_internal, rows, ground)
        self.L0 = sp.csr_matrix(L0)
        self.L0.sort_indices()
        self.A, self.M, self.hM = T.operator(self.meshes, kappa, film, n_internal, links)
        self.alpha, self.ambient, self.t0, self.element_heat = list(alpha), float(ambient), float(t0), element_heat

    def scale_of(self, theta):
        return scale(self.tri, self.face_mesh, self.alpha, self.ambient, self.t0, theta)

    def round(self, s):
        """One round with the scale ``s``: (V, P, theta, flows)."""
        L = revalue(self.L0, self.xy, self.tri, self.face_mesh, self.sigma, s)
        V = spla.spsolve(sp.csc_matrix(L), self.r)
        P = face_power(self.xy, self.tri, self.face_mesh, self.sigma, s, V[:self.n_vert])
        flows = solver.element_flows(self.rows, V)
        heat = []
        if self.element_heat:
            for row, flow in zip(self.rows, flows):
                if row[0] == "R":
                    heat += [(row[1], flow["power"] / 2), (row[2], flow["power"] / 2)]
        theta = T.solve(self.A, T.load(self.n_pot, self.tri, P, heat))
        return V, P, theta, flows

    def delivered(self, flows) -> float:
        terms = []
        for row, flow in zip(self.rows, flows):
            if row[0] != "R":
                terms += [-flow["power"], -flow.get("input_power", 0.0)]
        return math.fsum(terms)

    def picard(self, tolerance: float, max_rounds: int = 200):
        """Definition 6: a dict of the last round's V, P, theta, flows and scale, the increments, ``thetas`` of every round,
        ``converged`` and ``runaway`` (solver.picard_verdict's rule)."""
        theta = np.zeros(self.n_pot)
        s, prev = self.scale_of(theta)
        increments, thetas, verdict = [], [], None
        for _ in range(max_rounds):
            used = s
            V, P, theta, flows = self.round(used)
            s, mean = self.scale_of(theta)
            increments.append(float(np.abs(mean - prev).max()))
            prev = mean
            thetas.append(theta)
            verdict = solver.picard_verdict(increments, tolerance)
            if verdict is not None:
                break
        return dict(V=V, P=P, theta=theta, flows=flows, scale=used, increments=increments, thetas=thetas,
                    converged=verdict == "converged", runaway=verdict == "runaway")


def contraction(increments) -> float:
    """rho: the largest ratio of consecutive increments over the tail of the loop, where it has settled (the last five
    ratios whose increments are still above 1e-10 K, clear of the direct solves' rounding)."""
    d = [x for x in increments if x > 1e-10]
    ratios = [b / a for a, b in zip(d, d[1:])]
    return max(ratios[-5:])


# ---- the boards of the tests ----------------------------------------------------------------------------------------------

# name -> (film [W/(K mesh-unit^2)], the factor on every source of the Problem): chosen so that the one-way rise is some tens of
# kelvin and the loop contracts with rho < 0.5.  Measured with the restatement (copper's alpha, ambient 25, T0 20): single
# 43 K one-way, 48 K coupled, rho 0.10; two_layer 46 K, 50 K, rho 0.11; two_in_layer 33 K, 37 K, rho 0.11; problem_mixed
# (voltage sources among its elements) 27 K, 25 K, rho 0.08.
COUPLED_BOARDS = {"single": (1e-3, 0.3), "two_layer": (1e-3, 0.2), "two_in_layer": (1e-3, 0.12), "problem_mixed": (1e-3, 0.01)}
# the other goldens, for the balance alone: rises of 34 to 39 K
OTHER_BOARDS = {"problem_c1": (1e-3, 0.04), "problem_simple_trace": (1e-3, 0.12), "problem_two_planes": (1e-3, 0.03),
                "problem_many_meshes": (1e-3, 0.02)}


def scaled_case(prob, factor: float) -> dict:
    """The load case that multiplies every source of ``prob`` by ``factor``."""
    return {e: factor * getattr(e, solver.CASE_FIELDS[solver.element_kind(e)]) for n in prob.networks for e in n.elements
            if solver.element_kind(e) in solver.CASE_FIELDS}


def host_board(prob, meshes, layer_of, model, case=None) -> Board:
    """The :class:`Board` of a Problem on its meshes (mesh.Mesh) for an ElectroThermalModel and one load case."""
    vindex = solver.VertexIndexer.create(meshes)
    nodes = solver.NodeIndexer.create(prob, meshes, layer_of, vindex, list(prob.networks))
    pairs = solver.global_elements(list(prob.networks), nodes)
    checked = solver.check_electrothermal_model(prob, model)
    case = solver.check_load_cases(prob, [case or {}])[0]
    rows = solver._case_element_rows(pairs, [row for _, row in pairs], case)
    flat = [(np.asarray(m.points, dtype=np.float64), np.asarray(m.triangles, dtype=np.int64)) for m in meshes]
    th = checked.thermal
    return Board(flat, [prob.layers[l].conductance for l in layer_of], nodes.internal_node_count, rows,
                 solver.find_best_ground_node_index(prob, nodes), [th.kappa[l] for l in layer_of], [th.film[l] for l in layer_of],
                 [(row[1], row[2], th.links[element]) for element, row in pairs if row[0] == "R"],
                 [checked.alpha[l] for l in layer_of], th.ambient, checked.conductance_temperature, th.element_heat)


# ---- the uniform strip -----------------------------------------------------------------------------------------------------

STRIP_SIGMA, STRIP_FILM, STRIP_ALPHA, STRIP_N, STRIP_H = 2.0, 1e-3, 3.93e-3, 9, 1.0


def strip_current_density(alpha_theta0: float) -> float:
    """J with alpha theta0 = ``alpha_theta0`` for theta0 = J^2 / (sigma0 h)."""
    return math.sqrt(alpha_theta0 / STRIP_ALPHA * STRIP_SIGMA * STRIP_FILM)


def strip_sources(J: float):
    """(left vertex, right vertex, current) per grid row of the unjittered STRIP_N x STRIP_N grid: the current density J drawn
    from the left edge and fed into the right one with the consistent nodal weights h J (h J / 2 at the corners)."""
    n = STRIP_N
    return [(j * n, j * n + n - 1, J * STRIP_H * (0.5 if j in (0, n - 1) else 1.0)) for j in range(n)]


def strip_closed_form(alpha_theta0: float, rounds: int):
    """(theta_k for k = 1 .. rounds, the increments d_k, the fixed point): theta_k = theta0 (1 + alpha theta_k-1), d_k =
    theta0 (alpha theta0)^(k-1), theta0 / (1 - alpha theta0)."""
    theta0 = alpha_theta0 / STRIP_ALPHA
    thetas, prev = [], 0.0
    for _ in range(rounds):
        prev = theta0 * (1 + STRIP_ALPHA * prev)
        thetas.append(prev)
    return thetas, [theta0 * alpha_theta0 ** k for k in range(rounds)], theta0 / (1 - alpha_theta0)

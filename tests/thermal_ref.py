"""Host restatement of the thermal model for the tests ("Thermal"): the operator A, the lumped areas M_v, the
heat load b, the report and the envelope, with every sum in the order the device states, and a scipy direct solve.

Unknowns: the vertices of the meshes (numbered mesh by mesh), then ``n_internal`` internal nodes.  Faces are visited with
the corners (tri[2], tri[0], tri[1]) like the device.
 1. K: per mesh kappa_m times the reference's cotangent Laplacian (|cot|/2 weights, oracle.laplace_operator), then per
    link (a, b, g) the resistor's stamps in the reference's order, L[a,a] -= g, L[a,b] += g, L[b,b] -= g, L[b,a] += g (g = 0:
    nothing).  The reference's sign: K is negative semi-definite.
 2. A_f = |(x2 - x1)(y3 - y1) - (y2 - y1)(x3 - x1)| / 2;  M_v = sum over the faces incident to v, ascending, of A_f / 3.
 3. A = -K, and at a vertex the stored diagonal is the one rounded sum (-K_vv) + h_m M_v with h_m M_v one product.
 4. P_f = sigma ((w12 d12 d12 + w23 d23 d23) + w31 d31 d31), w_ab = |cot|/2 of the corner opposite edge (a, b) and
    d12 = V1 - V2, d23 = V2 - V3, d31 = V3 - V1 on the visiting order.
 5. b_v = sum over the faces incident to v, ascending, of P_f / 3; then the node-heat triples (node, watts) in list order.
 6. report: face mean ((theta_1 + theta_2) + theta_3) / 3; per mesh the largest theta (the lowest vertex on a tie; -inf
    and -1 without vertices), the heat sum P_f and the film loss sum (h_m M_v) theta_v (math.fsum here: the device's
    fixed-order sums agree to rounding).
 7. envelope: column 0 first, a later column replaces the value only when strictly greater."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import padne_oracle as O


def flatten(meshes):
    """(xy, global tri, face_mesh, vertex offsets, face offsets) of meshes given as (xy, tri, ...) tuples."""
    xys = [np.asarray(m[0], dtype=np.float64).reshape(-1, 2) for m in meshes]
    tris = [np.asarray(m[1], dtype=np.int64).reshape(-1, 3) for m in meshes]
    voff = np.concatenate([[0], np.cumsum([len(x) for x in xys])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(t) for t in tris])]).astype(np.int64)
    xy = np.concatenate(xys) if xys else np.zeros((0, 2))
    tri = np.concatenate([t + o for t, o in zip(tris, voff)]) if tris else np.zeros((0, 3), np.int64)
    face_mesh = np.concatenate([np.full(len(t), i, dtype=np.int64) for i, t in enumerate(tris)]) if tris else np.zeros(0, np.int64)
    return xy, tri, face_mesh, voff, toff


def corners(tri) -> np.ndarray:
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    return np.stack([tri[:, 2], tri[:, 0], tri[:, 1]], axis=1)


def face_area(xy, tri) -> np.ndarray:
    c = corners(tri)
    p1, p2, p3 = xy[c[:, 0]], xy[c[:, 1]], xy[c[:, 2]]
    return np.abs((p2[:, 0] - p1[:, 0]) * (p3[:, 1] - p1[:, 1]) - (p2[:, 1] - p1[:, 1]) * (p3[:, 0] - p1[:, 0])) / 2


def gather_thirds(n: int, tri, per_face) -> np.ndarray:
    """out[v] = sum over the faces incident to v, in ascending face number, of per_face[f] / 3: one sequential addition per
    (face, corner) in face order."""
    out = np.zeros(n)
    np.add.at(out, corners(tri).reshape(-1), np.repeat(np.asarray(per_face, dtype=np.float64) / 3, 3))
    return out


def lumped(xy, tri) -> np.ndarray:
    return gather_thirds(len(xy), tri, face_area(xy, tri))


def stiffness(meshes, kappa, n_internal: int, links) -> sp.csr_matrix:
    """Definition 1, (n_pot, n_pot), the reference's sign."""
    n_vert = sum(len(np.asarray(m[0]).reshape(-1, 2)) for m in meshes)
    n = n_vert + int(n_internal)
    rows, cols, vals, off = [], [], [], 0
    for (xy, tri, *_), k in zip(meshes, kappa):
        Lm = O.laplace_operator(xy, tri)
        rows.append(Lm.row.astype(np.int64) + off)
        cols.append(Lm.col.astype(np.int64) + off)
        vals.append(float(k) * Lm.data)
        off += Lm.shape[0]
    K = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tolil()
    for a, b, g in links:
        if g == 0.0:
            continue
        K[a, a] -= g
        K[a, b] += g
        K[b, b] -= g
        K[b, a] += g
    return K.tocsr()


def operator(meshes, kappa, film, n_internal: int, links):
    """(A csr, M_v, h_m M_v): definitions 1-3."""
    xy, tri, _face_mesh, voff, _toff = flatten(meshes)
    K = stiffness(meshes, kappa, n_internal, links)
    M = lumped(xy, tri)
    hM = np.repeat(np.asarray(film, dtype=np.float64), np.diff(voff)) * M
    A = (-K).tolil()
    d = K.diagonal()
    for v in range(len(xy)):
        A[v, v] = (-d[v]) + hM[v]
    A = A.tocsr()
    A.sort_indices()
    return A, M, hM


def face_power(xy, tri, face_mesh, sigma, V) -> np.ndarray:
    """Definition 4 for the vertex potentials ``V`` (n_vert,) or (n_vert, k): (n_tri,) or (k, n_tri)."""
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 2:
        return np.stack([face_power(xy, tri, face_mesh, sigma, V[:, j]) for j in range(V.shape[1])])
    c = corners(tri)
    p1, p2, p3 = xy[c[:, 0]], xy[c[:, 1]], xy[c[:, 2]]

    def cot_half(pi, pk, po):
        vix, viy = pi[:, 0] - po[:, 0], pi[:, 1] - po[:, 1]
        vkx, vky = pk[:, 0] - po[:, 0], pk[:, 1] - po[:, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.abs((vix * vkx + viy * vky) / (vix * vky - viy * vkx)) / 2

    w23, w31, w12 = cot_half(p2, p3, p1), cot_half(p3, p1, p2), cot_half(p1, p2, p3)
    f1, f2, f3 = V[c[:, 0]], V[c[:, 1]], V[c[:, 2]]
    d12, d23, d31 = f1 - f2, f2 - f3, f3 - f1
    s = np.asarray(sigma, dtype=np.float64)[face_mesh]
    return s * ((w12 * d12 * d12 + w23 * d23 * d23) + w31 * d31 * d31)


def load(n_pot: int, tri, P, heat=()) -> np.ndarray:
    """Definition 5 for one column: ``heat`` a sequence of (node, watts)."""
    b = np.zeros(int(n_pot))
    np.add.at(b, corners(tri).reshape(-1), np.repeat(np.asarray(P, dtype=np.float64) / 3, 3))
    for node, watts in heat:
        b[node] = b[node] + watts
    return b


def solve(A, b) -> np.ndarray:
    return spla.spsolve(sp.csc_matrix(A), b)


def report(tri, voff, toff, hM, theta, P):
    """Definition 6 for one column: (face means, per mesh: max theta, its vertex, heat, loss)."""
    c = corners(tri)
    mean = ((theta[c[:, 0]] + theta[c[:, 1]]) + theta[c[:, 2]]) / 3
    n_mesh = len(voff) - 1
    top, vert, heat, loss = np.full(n_mesh, -np.inf), np.full(n_mesh, -1, dtype=np.int64), np.zeros(n_mesh), np.zeros(n_mesh)
    for m in range(n_mesh):
        lo, hi = int(voff[m]), int(voff[m + 1])
        if hi > lo:
            k = int(np.argmax(theta[lo:hi]))                              # the first maximum: the lowest vertex
            top[m], vert[m] = theta[lo + k], lo + k
        loss[m] = math.fsum((hM[lo:hi] * theta[lo:hi]).tolist())
        heat[m] = math.fsum(np.asarray(P)[int(toff[m]):int(toff[m + 1])].tolist())
    return mean, top, vert, heat, loss


def envelope(values):
    """Definition 7 down the first axis of ``values`` (k, n): (max, the lowest case that attains it)."""
    values = np.asarray(values, dtype=np.float64)
    best, case = values[0].copy(), np.zeros(values.shape[1], dtype=np.int32)
    for j in range(1, values.shape[0]):
        greater = values[j] > best
        best[greater] = values[j][greater]
        case[greater] = j
    return best, case

"""The kernels of padne_amd/csrc/thermal_sens.hip in numpy, each expression in the kernel's own rounding order (its header
comment states them "rounded as written"; the library builds with -ffp-contract=off and numpy contracts nothing), for the
tests that hold the device to its bits on its own inputs.  Built on thermal_ref (corners, areas, cot_half's expression),
sampling_ref (the owner rule and the sides), sources_ref (the lists and the load), stack_ref (the per-vertex runs) and
fold_ref (the fixed-order sums); thermal_sens_ref is the specification these are checked against
(tests/test_tsens_kernel_ref_host.py), and shares no expression with this file.

Arrays: ``x`` and ``theta`` of one case (n_pot,), ``lam`` and ``mu`` of one objective (n_pot,) and (N,).  Corners (1, 2, 3)
of a face are thermal_ref.corners(tri): tri[:, 2], tri[:, 0], tri[:, 1], as error_corners gives them.
 1. owner: tsens_owner_kernel.  The lowest global face of the layer that contains q; the unknowns tri[f][0..2] and the
    weights o_k / ((o_a + o_b) + o_c) of sampling_ref's sides; (-1, -1, -1) and zeros for a point on no face.
 2. g_vector: tsens_g_kernel.  Kinds 0 and 1: from 0.0, plus weight[k] where unknown[k] is the row, k = 0, 1, 2 in that
    order.  Kind 2: sources_ref's load with unit power on that source, ((area_f / A_s) * 1.0) / 3 per face of the vertex's
    list front to back.
 3. rhs: tsens_rhs_kernel, then tsens_rhs_res_kernel.  Per vertex, over its faces ascending, acc = acc + (2 lbar) (s d)
    with lbar = ((l1 + l2) + l3) / 3 and d at corner 1: w12 (f1 - f2) + w31 (f1 - f3), corner 2: w12 (f2 - f1) + w23 (f2 -
    f3), corner 3: w23 (f3 - f2) + w31 (f3 - f1).  Then per resistor (a, b, R) in list order t = (2 ((l_a + l_b) / 2)) ((x_a -
    x_b) / R), out[a] = out[a] + t, out[b] = out[b] + (-1.0) t.  Rows from n_pot on are 0.
 4. faces: tsens_face_kernel.  ef = lbar P_f + s ((w12 (u1 - u2) (f1 - f2) + w23 (u2 - u3) (f2 - f3)) + w31 (u3 - u1) (f3 -
    f1)), P_f thermal_ref.face_power's expression; kf = -(kap ((w12 (l1 - l2) (t1 - t2) + w23 ...) + w31 ...)); the densities
    ef / area, kf / area and (ef + kf) / area.
 5. film_terms: tsens_vertex_kernel's term -((hM_v lam_v) theta_v).
 6. pair_vertex_terms, pair_values: tsens_pair_kernel and the join of padne_tsens_pairs.  Vertex i of a mesh of layer a: from
    0.0 over its stored partners k in G's row order with vertex_layer[k] == b, acc = acc + (-G_ik) ((l_i - l_k) (t_i - t_k));
    fold_ref.mesh_sum per mesh; the meshes of layer a ascending from 0.0; the sign.
 7. sources: sources_ref.Restated.temperature(lam, 0.0), what sources_report_field sums.
 8. mesh_sums: fold_ref.mesh_sum of the items of every mesh, tsens_fold_kernel over the tiles the kernels above leave."""
from __future__ import annotations

import numpy as np

import fold_ref as F
import sampling_ref as R
import stack_ref as K
import thermal_ref as T


def cot_half(pi, pk, po):
    """thermal_ref.face_power's (face.hpp's) |cot| / 2 of the corner ``po`` opposite the edge (pi, pk)."""
    vix, viy = pi[:, 0] - po[:, 0], pi[:, 1] - po[:, 1]
    vkx, vky = pk[:, 0] - po[:, 0], pk[:, 1] - po[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs((vix * vkx + viy * vky) / (vix * vky - viy * vkx)) / 2


def face_weights(xy, tri):
    """(corners (n_tri, 3), w12, w23, w31)."""
    c = T.corners(tri)
    p1, p2, p3 = xy[c[:, 0]], xy[c[:, 1]], xy[c[:, 2]]
    return c, cot_half(p1, p2, p3), cot_half(p2, p3, p1), cot_half(p3, p1, p2)


def owner(board: R.Board, layer: int, q):
    """Definition 1 for one point: (unknown (3,) int64, weight (3,))."""
    q = np.asarray(q, dtype=np.float64).reshape(1, 2)
    f = int(R.owners(board, layer, q)[0])
    if f < 0:
        return np.full(3, -1, dtype=np.int64), np.zeros(3)
    t = board.tri[f]
    qx, qy = q[:, 0], q[:, 1]
    oa = R.edge_side(board, t[[1]], t[[2]], qx, qy)[0]
    ob = R.edge_side(board, t[[2]], t[[0]], qx, qy)[0]
    oc = R.edge_side(board, t[[0]], t[[1]], qx, qy)[0]
    s = (oa + ob) + oc
    return np.asarray(t, dtype=np.int64), np.array([oa / s, ob / s, oc / s])


def source_g(sources, source: int, n_pot: int) -> np.ndarray:
    """sources_ref.Restated.load with unit power on ``source`` and none on the others, without its loop over every face: the
    other sources add ((area_f / A_s) * 0.0) / 3 = 0.0, which leaves a sum that started from 0.0 as it is, so what remains is
    one sequential addition of ((area_f / A_s) * 1.0) / 3 per (face of the list, corner) in ascending face order.  The host
    test holds the two to the same bits."""
    mine = sources.face[sources.ptr[source]:sources.ptr[source + 1]]
    term = ((sources.face_area[mine] / sources.A[source]) * 1.0) / 3
    g = np.zeros(int(n_pot))
    np.add.at(g, T.corners(sources.tri)[mine].reshape(-1), np.repeat(term, 3))
    return g


def g_vector(n_pot: int, kind: int, unknown=None, weight=None, sources=None, source=None) -> np.ndarray:
    """Definition 2: ``unknown`` and ``weight`` (3,) for the kinds 0 and 1 (an unknown of -1 adds nowhere); ``sources`` a
    sources_ref.Restated and ``source`` its index for kind 2."""
    if kind == 2:
        return source_g(sources, source, n_pot)
    g = np.zeros(int(n_pot))
    for u, w in zip(unknown, weight):
        if u >= 0:
            g[u] = g[u] + w
    return g


def rhs(N: int, n_pot: int, xy, tri, face_mesh, sigma, lam_j, x_c, resistors=()) -> np.ndarray:
    """Definition 3: one column (N,); ``resistors`` a sequence of (a, b, R), empty without element heat."""
    c, w12, w23, w31 = face_weights(xy, tri)
    s = np.asarray(sigma, dtype=np.float64)[face_mesh]
    l1, l2, l3 = lam_j[c[:, 0]], lam_j[c[:, 1]], lam_j[c[:, 2]]
    f1, f2, f3 = x_c[c[:, 0]], x_c[c[:, 1]], x_c[c[:, 2]]
    lbar = ((l1 + l2) + l3) / 3
    d = np.stack([w12 * (f1 - f2) + w31 * (f1 - f3), w12 * (f2 - f1) + w23 * (f2 - f3), w23 * (f3 - f2) + w31 * (f3 - f1)], axis=1)
    terms = (2 * lbar)[:, None] * (s[:, None] * d)
    out = np.zeros(int(N))
    np.add.at(out, c.reshape(-1), terms.reshape(-1))        # one sequential addition per (face, corner) in face order
    for a, b, res in resistors:
        t = (2 * ((lam_j[a] + lam_j[b]) / 2)) * ((x_c[a] - x_c[b]) / res)
        out[a] = out[a] + t
        out[b] = out[b] + (-1.0) * t
    assert not out[int(n_pot):].any()
    return out


def faces(xy, tri, face_mesh, sigma, kappa, lam_j, theta_c, x_c, mu_j):
    """Definition 4: (ef / area, kf / area, (ef + kf) / area, ef, kf), each (n_tri,)."""
    c, w12, w23, w31 = face_weights(xy, tri)
    s = np.asarray(sigma, dtype=np.float64)[face_mesh]
    kap = np.asarray(kappa, dtype=np.float64)[face_mesh]
    area = T.face_area(xy, tri)
    l1, l2, l3 = lam_j[c[:, 0]], lam_j[c[:, 1]], lam_j[c[:, 2]]
    t1, t2, t3 = theta_c[c[:, 0]], theta_c[c[:, 1]], theta_c[c[:, 2]]
    f1, f2, f3 = x_c[c[:, 0]], x_c[c[:, 1]], x_c[c[:, 2]]
    u1, u2, u3 = mu_j[c[:, 0]], mu_j[c[:, 1]], mu_j[c[:, 2]]
    lbar = ((l1 + l2) + l3) / 3
    d12, d23, d31 = f1 - f2, f2 - f3, f3 - f1
    P = s * ((w12 * d12 * d12 + w23 * d23 * d23) + w31 * d31 * d31)
    ef = lbar * P + s * ((w12 * (u1 - u2) * (f1 - f2) + w23 * (u2 - u3) * (f2 - f3)) + w31 * (u3 - u1) * (f3 - f1))
    kf = -(kap * ((w12 * (l1 - l2) * (t1 - t2) + w23 * (l2 - l3) * (t2 - t3)) + w31 * (l3 - l1) * (t3 - t1)))
    return ef / area, kf / area, (ef + kf) / area, ef, kf


def film_terms(hM, lam_j, theta_c) -> np.ndarray:
    """Definition 5: (n_vert,)."""
    n = len(hM)
    return -((hM * lam_j[:n]) * theta_c[:n])


def pair_vertex_terms(voff, mesh_layer, G, a: int, b: int, lam_j, theta_c) -> np.ndarray:
    """Definition 6, the per-vertex part for the pair of layers (a, b): (n_vert,), 0.0 at the vertices of other layers.
    ``G``: the off-diagonals of Thermal.stack_matrix() as a csr_matrix with its rows as stored."""
    n_vert = int(voff[-1])
    vertex_layer = np.repeat(np.asarray(mesh_layer, dtype=np.int64), np.diff(voff))
    rows = np.repeat(np.arange(G.shape[0]), np.diff(G.indptr))
    cols = np.asarray(G.indices, dtype=np.int64)
    keep = (rows < n_vert) & (cols < n_vert)
    keep &= (vertex_layer[np.minimum(rows, n_vert - 1)] == a) & (vertex_layer[np.minimum(cols, n_vert - 1)] == b)
    r, k, w = rows[keep], cols[keep], -G.data[keep]
    terms = w * ((lam_j[r] - lam_j[k]) * (theta_c[r] - theta_c[k]))
    starts = np.searchsorted(r, np.arange(n_vert))
    lengths = np.searchsorted(r, np.arange(n_vert), side="right") - starts
    return K._run_sums(terms, starts, lengths, init=0.0)


def mesh_sums(off, items) -> np.ndarray:
    """Definition 8: fold_ref.mesh_sum of items[off[m]:off[m + 1]] for every mesh."""
    return np.array([F.mesh_sum(items[int(off[m]):int(off[m + 1])]) for m in range(len(off) - 1)])


def pair_values(voff, mesh_layer, G, pairs, lam_j, theta_c):
    """Definition 6: (the value of every pair (n_pair,), the per-vertex terms of every pair [(n_vert,)])."""
    out, per = np.zeros(len(pairs)), []
    for p, (a, b, *_g) in enumerate(pairs):
        terms = pair_vertex_terms(voff, mesh_layer, G, a, b, lam_j, theta_c)
        folded = mesh_sums(voff, terms)
        total = 0.0
        for m in range(len(mesh_layer)):
            if mesh_layer[m] == a:
                total = total + folded[m]
        out[p] = -total
        per.append(terms)
    return out, per


def sources(restated, lam_j) -> np.ndarray:
    """Definition 7: (n_source,)."""
    return restated.temperature(lam_j, 0.0)[0]

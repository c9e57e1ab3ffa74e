"""Host restatement of the inter-layer coupling for the tests ("Stack"), on top of tests/thermal_ref.py (A, M_v)
and tests/sampling_ref.py (the owner rule by brute force, the sides), with every sum in the order the device states.

Meshes come as (xy, tri, ...) tuples in flat order with ``mesh_layer`` the layer of each; ``pairs`` is a list of (layer a,
layer b, g).
 1. sides: for every pair with g > 0, in list order, (a -> b) then (b -> a).  A side's slots are the vertices of the meshes
    of its source layer in ascending global order.
 2. slot (side s -> t, vertex v): f = the owner of xy[v] among the faces of layer t (none: -1, zeros); (o_a, o_b, o_c) the
    sides of the edges opposite tri[f][0..2]; s = (o_a + o_b) + o_c; lambda_k = o_k / s; c_k = ((0.5 g) M_v) lambda_k.
 3. links: slot q, corner k with c_k != 0 gives the directed entries (v, u, c_k) and (u, v, c_k), u = tri[f][k], numbered
    6 q + 2 k and 6 q + 2 k + 1.  G_ij = -(the sum of the entries (i, j) in ascending number); G_ii = the sum of (-G_ij) along
    row i in ascending j, from 0.0.
 4. A' = A + G on the union pattern: one rounded add where both are stored (the diagonal of a row with partners included),
    the stored one otherwise.
 5. flow(a -> b) = over the meshes of layer a in ascending order, from 0.0, the sum of the mesh's part; a mesh's part folds
    its tiles of 256 vertices as the device does (thread t takes tiles t, t + 256, ... front to back, then the workgroup
    sum); a tile is the workgroup sum of the per-vertex terms; vertex i's term is the sum over its partners j in layer b,
    ascending, of (-G_ij)(theta_i - theta_j), from 0.0.  The workgroup sum of 256 values: down each run of 64 by halving
    strides (v[:h] += v[h:2h], h = 32 .. 1), then (w0 + w1) + (w2 + w3).  area = (the same with the terms (-G_ij)) / g."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import sampling_ref as R
import thermal_ref as T
from fold_ref import mesh_sum, workgroup_sum  # noqa: F401   (definition 5's order, stated in tests/fold_ref.py)


def board_of(meshes, mesh_layer) -> R.Board:
    xy, tri, _face_mesh, voff, toff = T.flatten(meshes)
    return R.Board(xy=xy, tri=tri, toff=toff, voff=voff, sigma=np.zeros(len(meshes)),
                   layer_of=np.asarray(mesh_layer, dtype=np.int64), V=np.zeros(len(xy)))


def sides_of(pairs):
    """[(source layer, target layer, 0.5 g, pair index)] (definition 1)."""
    out = []
    for p, (a, b, g) in enumerate(pairs):
        if g != 0.0:
            out += [(a, b, 0.5 * g, p), (b, a, 0.5 * g, p)]
    return out


def slots(meshes, mesh_layer, pairs):
    """(side offsets, vertex, owner, weights (n, 3), conductances (n, 3)): definitions 1 and 2."""
    b = board_of(meshes, mesh_layer)
    M = T.lumped(b.xy, b.tri)
    off, vert, owner, weight, cond = [0], [], [], [], []
    for src, dst, half_g, _p in sides_of(pairs):
        v = R.layer_vertices(b, src)
        q = b.xy[v]
        f = R.owners(b, dst, q)
        w = np.zeros((len(v), 3))
        hit = np.flatnonzero(f >= 0)
        if len(hit):
            t = b.tri[f[hit]]
            qx, qy = q[hit, 0], q[hit, 1]
            o = [R.edge_side(b, t[:, 1], t[:, 2], qx, qy), R.edge_side(b, t[:, 2], t[:, 0], qx, qy),
                 R.edge_side(b, t[:, 0], t[:, 1], qx, qy)]
            s = (o[0] + o[1]) + o[2]
            w[hit] = np.stack([o[0] / s, o[1] / s, o[2] / s], axis=1)
        vert.append(v)
        owner.append(f)
        weight.append(w)
        cond.append(((half_g * M[v])[:, None] * w) * (f >= 0)[:, None])
        off.append(off[-1] + len(v))
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty      # noqa: E731
    return (np.asarray(off, dtype=np.int64), cat(vert, np.zeros(0, np.int64)), cat(owner, np.zeros(0, np.int64)),
            cat(weight, np.zeros((0, 3))), cat(cond, np.zeros((0, 3))))


def _run_sums(values, starts, lengths, init=None):
    """Per run (start, length) of ``values``: ((init + v_0) + v_1) + ..., or (v_0 + v_1) + ... without ``init``."""
    starts, lengths = np.asarray(starts, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    if init is None:
        out, first = values[starts].copy() if len(starts) else np.zeros(0), 1
    else:
        out, first = np.full(len(starts), float(init)), 0
    for t in range(first, int(lengths.max()) if len(lengths) else 0):
        m = lengths > t
        out[m] = out[m] + values[starts[m] + t]
    return out


def coupling(n_pot: int, tri, vertex, owner, cond):
    """(G's off-diagonals as a sorted csr_matrix with explicit entries, its diagonal): definition 3."""
    n = len(vertex)
    number = np.arange(6 * n)
    q, k, d = number // 6, (number % 6) // 2, number % 2
    c = cond[q, k]
    live = (owner[q] >= 0) & (c != 0.0)
    u = np.where(owner[q] >= 0, tri[np.maximum(owner[q], 0), k], 0)
    row, col = np.where(d == 0, vertex[q], u)[live], np.where(d == 0, u, vertex[q])[live]
    c = c[live]
    order = np.lexsort((col, row))                          # stable: equal (row, column) keep their numbers' order
    row, col, c = row[order], col[order], c[order]
    key = row * n_pot + col
    head = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
    lengths = np.diff(np.concatenate([head, [len(key)]]))
    val = -_run_sums(c, head, lengths)
    grow, gcol = row[head], col[head]
    indptr = np.searchsorted(grow, np.arange(n_pot + 1)).astype(np.int64)
    G = sp.csr_matrix((val, gcol.astype(np.int64), indptr), shape=(n_pot, n_pot))
    diag = _run_sums(-val, indptr[:-1], np.diff(indptr), init=0.0)
    return G, diag


def stacked(A, G, diag):
    """A' (definition 4), sorted, with every stored entry of A and of G kept."""
    A = sp.csr_matrix(A)
    A.sort_indices()
    n = A.shape[0]
    reached = np.flatnonzero(np.diff(G.indptr) > 0)
    a_row = np.repeat(np.arange(n), np.diff(A.indptr))
    g_row = np.concatenate([np.repeat(np.arange(n), np.diff(G.indptr)), reached])
    a_key = a_row * n + A.indices
    g_key = g_row * n + np.concatenate([G.indices, reached])
    g_val = np.concatenate([G.data, diag[reached]])
    keys = np.union1d(a_key, g_key)
    ia, ig = np.searchsorted(keys, a_key), np.searchsorted(keys, g_key)
    va, vg = np.zeros(len(keys)), np.zeros(len(keys))
    has_a, has_g = np.zeros(len(keys), bool), np.zeros(len(keys), bool)
    va[ia], has_a[ia] = A.data, True
    vg[ig], has_g[ig] = g_val, True
    data = np.where(has_a & has_g, va + vg, np.where(has_a, va, vg))
    out = sp.csr_matrix((data, (keys // n, keys % n)), shape=A.shape)
    out.sort_indices()
    assert out.nnz == len(keys)
    return out


def operator(meshes, mesh_layer, kappa, film, n_internal, links, pairs):
    """(A', G off-diagonals, G diagonal, M_v, h M_v, the slots): everything the device builds at creation."""
    A, M, hM = T.operator(meshes, kappa, film, n_internal, links)
    b = board_of(meshes, mesh_layer)
    s = slots(meshes, mesh_layer, pairs)
    G, diag = coupling(A.shape[0], b.tri, s[1], s[2], s[4])
    return stacked(A, G, diag), G, diag, M, hM, s


def full(G, diag):
    """G with its diagonal, as one csr_matrix."""
    return sp.csr_matrix(G + sp.diags(diag))


def flows(meshes, mesh_layer, pairs, G, theta):
    """(flow (k, n_pair), area (n_pair,)) for theta (k, n_pot): definition 5."""
    _xy, _tri, _fm, voff, _toff = T.flatten(meshes)
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, G.shape[0])
    vertex_layer = np.repeat(np.asarray(mesh_layer, dtype=np.int64), np.diff(voff))
    rows = np.repeat(np.arange(G.shape[0]), np.diff(G.indptr))
    flow, area = np.zeros((len(theta), len(pairs))), np.zeros(len(pairs))
    for p, (a, b, g) in enumerate(pairs):
        keep = (rows < len(vertex_layer)) & (vertex_layer[np.minimum(rows, len(vertex_layer) - 1)] == a) & \
               (vertex_layer[np.minimum(G.indices, len(vertex_layer) - 1)] == b)
        r, c, w = rows[keep], G.indices[keep], -G.data[keep]
        starts = np.searchsorted(r, np.arange(G.shape[0]))
        lengths = np.searchsorted(r, np.arange(G.shape[0]), side="right") - starts
        for col in range(len(theta) + 1):
            terms = w * (theta[col][r] - theta[col][c]) if col < len(theta) else w
            per_vertex = _run_sums(terms, starts, lengths, init=0.0)
            total = 0.0
            for m in range(len(mesh_layer)):
                if mesh_layer[m] == a:
                    total = total + mesh_sum(per_vertex[voff[m]:voff[m + 1]])
            if col < len(theta):
                flow[col, p] = total
            else:
                area[p] = total / g if g > 0.0 else 0.0
    return flow, area

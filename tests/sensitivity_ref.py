"""Host restatement of the sensitivities for the tests: the oracle's M and r, scipy solves with M and M^T, the assembly's
cot weights per face.  Works for the unknown-level fixtures (elements on global unknowns) and the problem-level ones
(networks of NodeIDs, numbered by padne_amd.solver.NodeIndexer)."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers as H
from oracle import padne_oracle as O
from padne_amd import mesh, problem, solver


@dataclass
class System:
    meshes: list                  # (xy, tri, sigma) in unknown order
    n_internal: int
    rows: list                    # element rows on global unknowns, the oracle's tuples
    ground: int
    layer_of: list = field(default_factory=list)
    prob: object = None           # problem-level fixtures only
    pairs: list = field(default_factory=list)
    nodes: object = None
    flat: list = field(default_factory=list)
    ids: dict = field(default_factory=dict)      # fixture node number -> NodeID

    def assemble(self, rows=None, extra=None):
        """(M csr, r); ``extra`` (N, N) sparse is added to M."""
        M, r = O.assemble_system(self.meshes, self.n_internal, self.rows if rows is None else rows, self.ground)
        if extra is not None:
            M = (M + extra).tocsr()
        return M, r

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum([len(m[0]) for m in self.meshes])]).astype(np.int64)


def unknown_system(name) -> System:
    g = H.load_golden(name)
    ms = H.meshes_of(g)
    return System(meshes=[(xy, tri, s) for xy, tri, s, _ in ms], n_internal=int(g["n_internal"]), rows=H.elements_of(g),
                  ground=int(g["ground"]), layer_of=[layer for *_, layer in ms])


def problem_system(name, g=None) -> System:
    g = H.load_golden(name) if g is None else g
    prob, ids, flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    meshes = [mesh.Mesh(xy, tri) for xy, tri, _ in ms]
    layer_of = [layer for _, _, layer in ms]
    vindex = solver.VertexIndexer.create(meshes)
    nodes = solver.NodeIndexer.create(prob, meshes, layer_of, vindex, list(prob.networks))
    pairs = solver.global_elements(list(prob.networks), nodes)
    sig = [prob.layers[layer].conductance for layer in layer_of]
    return System(meshes=[(xy, tri, s) for (xy, tri, _), s in zip(ms, sig)], n_internal=nodes.internal_node_count,
                  rows=[row for _, row in pairs], ground=solver.find_best_ground_node_index(prob, nodes), layer_of=layer_of,
                  prob=prob, pairs=pairs, nodes=nodes, flat=flat, ids=ids)


def solve(M, b, refine: int = 2):
    """spsolve, then ``refine`` steps of iterative refinement with the residual in extended precision (small fixtures: a
    dense long-double product), so that the forward error is near eps and not eps cond(M): finite differences of J and
    the comparisons of two ways to the same solution are then not limited by the conditioning of the fixture."""
    M = sp.csc_matrix(M)
    x = spla.spsolve(M, b)
    if refine and M.shape[0] <= 4000:
        Md = M.toarray().astype(np.longdouble)
        bd = np.asarray(b, dtype=np.longdouble)
        xd = np.asarray(x, dtype=np.longdouble)
        for _ in range(refine):
            res = bd - Md @ xd
            xd = xd + np.asarray(spla.spsolve(M, np.asarray(res, dtype=np.float64)), dtype=np.longdouble).reshape(xd.shape)
        x = np.asarray(xd, dtype=np.float64)
    return x


def adjoint(M, p, q):
    c = np.zeros(M.shape[0])
    c[p] += 1.0
    c[q] -= 1.0
    return solve(sp.csc_matrix(M.T), c)


def faces(system: System):
    """Per face in unknown order: global corners (n_tri, 3), cot weights c[t, e] of edge (tri[e], tri[e+1]), sigma, area."""
    tris, cots, sig, area = [], [], [], []
    for off, (xy, tri, s) in zip(system.offsets, system.meshes):
        tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        tris.append(tri + off)
        cots.append(O.triangle_corner_cot_half(xy, tri))
        sig.append(np.full(len(tri), s))
        a, b, c = xy[tri[:, 0]], xy[tri[:, 1]], xy[tri[:, 2]]
        area.append(np.abs((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])) / 2)
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape)  # noqa: E731
    return cat(tris, (0, 3)).astype(np.int64), cat(cots, (0, 3)), cat(sig, (0,)), cat(area, (0,))


def face_s(system: System, x, lam):
    """s_f = sigma sum_edges w_ik (lam_i - lam_k)(x_i - x_k) with the assembly's |cot|/2 weights."""
    tri, cot, sig, _ = faces(system)
    s = np.zeros(len(tri))
    for e in range(3):
        i, k = tri[:, e], tri[:, (e + 1) % 3]
        s += cot[:, e] * (lam[i] - lam[k]) * (x[i] - x[k])
    return sig * s


def face_s_bound(system: System, x, lam):
    """sigma sum_edges w_ik 2 |lam|_max |x_i - x_k|: how large the terms of s_f can be for an adjoint of this size, what
    the rounding of s_f is relative to (an objective that no face can change -- across a voltage source -- has s_f = 0 up
    to that rounding)."""
    tri, cot, sig, _ = faces(system)
    s = np.zeros(len(tri))
    lmax = np.abs(lam).max()
    for e in range(3):
        i, k = tri[:, e], tri[:, (e + 1) % 3]
        s += cot[:, e] * 2 * lmax * np.abs(x[i] - x[k])
    return sig * s


def element_bounds(rows, x, lam) -> dict:
    """Per field, the largest size the terms of element_sensitivities can have for an adjoint of this size."""
    lmax = np.abs(lam).max()
    out = {"resistance": 0.0, "current": 0.0, "voltage": 0.0, "gain": 0.0}
    for row in rows:
        if row[0] == "R":
            out["resistance"] = max(out["resistance"], 2 * lmax * abs(x[row[1]] - x[row[2]]) / row[3] ** 2)
        elif row[0] == "I":
            out["current"] = max(out["current"], 2 * lmax)
        elif row[0] == "V":
            out["voltage"] = max(out["voltage"], lmax)
        else:
            out["voltage"] = max(out["voltage"], lmax)
            out["gain"] = max(out["gain"], 2 * lmax * abs(x[row[7]]))
    return out


def face_s_gradient_form(system: System, x, lam):
    """sigma A grad(lam) . grad(x): the same as face_s on faces without an obtuse corner only."""
    tri, _, sig, area = faces(system)
    xy = np.concatenate([np.asarray(m[0], dtype=np.float64).reshape(-1, 2) for m in system.meshes])
    p = [xy[tri[:, e]] for e in range(3)]
    glx, gly = O.triangle_gradient(p[0], p[1], p[2], lam[tri[:, 0]], lam[tri[:, 1]], lam[tri[:, 2]])
    gxx, gxy = O.triangle_gradient(p[0], p[1], p[2], x[tri[:, 0]], x[tri[:, 1]], x[tri[:, 2]])
    return sig * area * (glx * gxx + gly * gxy)


def face_derivative_matrix(system: System, t: int):
    """dM/dsigma of face t alone (the face's share of the cot Laplacian, unit conductance) as an (N, N) matrix."""
    tri, _, _, _ = faces(system)
    N = sum(len(m[0]) for m in system.meshes) + system.n_internal + sum(1 for r in system.rows if r[0] in ("V", "REG")) + 1
    xy = np.concatenate([np.asarray(m[0], dtype=np.float64).reshape(-1, 2) for m in system.meshes])
    corners = tri[t]
    local = O.laplace_operator(xy[corners], np.array([[0, 1, 2]]), validate=False).tocoo()
    return sp.coo_matrix((local.data, (corners[local.row], corners[local.col])), shape=(N, N)).tocsr()

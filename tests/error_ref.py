"""Host restatement of the gradient-recovery error estimate for the tests, on flat arrays or on a sensitivity_ref.System,
and the yardstick it is itself checked against: P1 finite elements on the meshes of padne_amd.synthetic with Dirichlet data
from a known harmonic function, whose true error in the energy norm a degree-2 quadrature gives.

The definitions (faces visited with the corners (tri[2], tri[0], tri[1]) like the device):
 1. g_f: the oracle's triangle gradient; A_f = |(x2 - x1)(y3 - y1) - (y2 - y1)(x3 - x1)| / 2.
 2. G_v = (sum_f A_f g_f) / (sum_f A_f) over the faces incident to v, added in ascending global face number; 0 for a vertex
    without faces or whose areas sum to zero.
 3. eta_f^2 = sigma (A_f / 3) (|m_12|^2 + |m_23|^2 + |m_31|^2), d_c = G_(corner c) - g_f, m_ab = (d_a + d_b) / 2.
 4. per mesh E_m = sum eta_f^2, P_m = sum sigma A_f |g_f|^2, the face with the largest eta_f (the lowest on a tie).
 5. power_error = sum E_m; estimate = sqrt(power_error / (sum P_m + power_error)), 0.0 when the denominator is 0.
 6. e_bar = tolerance sqrt((sum P_m + power_error) / n_faces), xi_f = eta_f / e_bar, size h_f / xi_f with
    h_f = sqrt(4 A_f / sqrt(3)); inf where xi_f = 0.
Disconnected meshes: zeros throughout, and their faces do not count in n_faces."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle import padne_oracle as O
from padne_amd import synthetic


@dataclass
class Estimate:
    g: np.ndarray             # (n_tri, 2) face gradients
    area: np.ndarray          # (n_tri,)
    sigma: np.ndarray         # (n_tri,) the sheet conductance of each face's mesh
    G: np.ndarray             # (n_vert, 2) recovered gradients
    eta: np.ndarray           # (n_tri,)
    mesh_error: np.ndarray    # (n_mesh,) E_m
    mesh_power: np.ndarray    # (n_mesh,) P_m
    mesh_max: np.ndarray      # (n_mesh,) the largest eta_f, -1.0 for a mesh without faces
    mesh_face: np.ndarray     # (n_mesh,) its global face, -1 for a mesh without faces
    power_error: float
    estimate: float
    n_faces: int              # the faces of connected meshes
    g_around: np.ndarray      # (n_vert,) the largest |g_f| among the faces incident to each vertex (0 without faces)

    @property
    def total_power(self) -> float:
        return float(self.mesh_power.sum()) + self.power_error

    def eta_scale(self, tri) -> np.ndarray:
        """sqrt(sigma A_f) times the largest |g| around the face's corners: what the rounding of eta_f is relative to."""
        return np.sqrt(self.sigma * self.area) * self.g_around[tri].max(axis=1)


def estimate_flat(xy, tri, face_mesh, sigma, x, connected=None) -> Estimate:
    """Definitions 1-5.  ``tri`` (n_tri, 3) global corners, ``face_mesh`` (n_tri,) the mesh of each face (ascending),
    ``sigma`` (n_mesh,), ``x`` the potentials of the vertices, ``connected`` (n_mesh,) bool (default: all)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    face_mesh = np.asarray(face_mesh, dtype=np.int64)
    sigma = np.asarray(sigma, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n_vert, n_tri, n_mesh = len(xy), len(tri), len(sigma)
    live_mesh = np.ones(n_mesh, dtype=bool) if connected is None else np.asarray(connected, dtype=bool)
    live = live_mesh[face_mesh] if n_tri else np.zeros(0, dtype=bool)
    c = np.stack([tri[:, 2], tri[:, 0], tri[:, 1]], axis=1)
    p1, p2, p3 = xy[c[:, 0]], xy[c[:, 1]], xy[c[:, 2]]
    gx, gy = O.triangle_gradient(p1, p2, p3, x[c[:, 0]], x[c[:, 1]], x[c[:, 2]])
    area = np.abs((p2[:, 0] - p1[:, 0]) * (p3[:, 1] - p1[:, 1]) - (p2[:, 1] - p1[:, 1]) * (p3[:, 0] - p1[:, 0])) / 2
    g = np.where(live[:, None], np.stack([gx, gy], axis=1), 0.0)
    s_face = sigma[face_mesh] if n_tri else np.zeros(0)
    # 2: one addition per (face, corner) in face order, so every vertex adds its faces in ascending face number
    rows = c[live].reshape(-1)
    sx, sy, sa = np.zeros(n_vert), np.zeros(n_vert), np.zeros(n_vert)
    np.add.at(sx, rows, np.repeat(area[live] * g[live, 0], 3))
    np.add.at(sy, rows, np.repeat(area[live] * g[live, 1], 3))
    np.add.at(sa, rows, np.repeat(area[live], 3))
    G = np.zeros((n_vert, 2))
    some = sa > 0
    G[some, 0] = sx[some] / sa[some]
    G[some, 1] = sy[some] / sa[some]
    g_around = np.zeros(n_vert)
    np.maximum.at(g_around, rows, np.repeat(np.hypot(g[live, 0], g[live, 1]), 3))
    # 3
    d = G[c] - g[:, None, :]                                          # (n_tri, 3 corners, 2)
    m12, m23, m31 = (d[:, 0] + d[:, 1]) / 2, (d[:, 1] + d[:, 2]) / 2, (d[:, 2] + d[:, 0]) / 2
    eta2 = s_face * (area / 3) * ((m12 ** 2).sum(axis=1) + (m23 ** 2).sum(axis=1) + (m31 ** 2).sum(axis=1))
    eta2 = np.where(live, eta2, 0.0)
    eta = np.sqrt(eta2)
    # 4
    power = np.where(live, s_face * area * (g ** 2).sum(axis=1), 0.0)
    E = np.bincount(face_mesh, weights=eta2, minlength=n_mesh) if n_tri else np.zeros(n_mesh)
    P = np.bincount(face_mesh, weights=power, minlength=n_mesh) if n_tri else np.zeros(n_mesh)
    top, top_face = np.full(n_mesh, -1.0), np.full(n_mesh, -1, dtype=np.int64)
    for m in range(n_mesh):
        faces = np.flatnonzero(face_mesh == m)
        if len(faces):
            k = int(np.argmax(eta[faces]))                            # the first maximum: the lowest face
            top[m], top_face[m] = eta[faces[k]], faces[k]
    # 5
    power_error = float(E.sum())
    total = float(P.sum()) + power_error
    return Estimate(g=g, area=area, sigma=s_face, G=G, eta=eta, mesh_error=E, mesh_power=P, mesh_max=top, mesh_face=top_face,
                    power_error=power_error, estimate=math.sqrt(power_error / total) if total > 0 else 0.0,
                    n_faces=int(live.sum()), g_around=g_around)


def flat_of(system):
    """(xy, global tri, face_mesh, sigma) of a sensitivity_ref.System, meshes in unknown order."""
    xy = np.concatenate([np.asarray(m[0], dtype=np.float64).reshape(-1, 2) for m in system.meshes])
    offs = system.offsets
    tri = np.concatenate([np.asarray(m[1], dtype=np.int64).reshape(-1, 3) + off for m, off in zip(system.meshes, offs)])
    face_mesh = np.concatenate([np.full(len(np.asarray(m[1]).reshape(-1, 3)), i, dtype=np.int64)
                                for i, m in enumerate(system.meshes)])
    return xy, tri, face_mesh, np.array([m[2] for m in system.meshes], dtype=np.float64)


def estimate_system(system, x, connected=None) -> Estimate:
    xy, tri, face_mesh, sigma = flat_of(system)
    return estimate_flat(xy, tri, face_mesh, sigma, np.asarray(x)[:len(xy)], connected)


def ratios_sizes(est: Estimate, tolerance: float):
    """Definition 6: (xi_f, h_f / xi_f) of every face."""
    e_bar = tolerance * math.sqrt(est.total_power / est.n_faces)
    xi = est.eta / e_bar
    h = np.sqrt(4 * est.area / math.sqrt(3.0))
    with np.errstate(divide="ignore"):
        return xi, np.where(xi > 0, h / np.where(xi > 0, xi, 1.0), np.inf)


# ---- the yardstick: P1 finite elements against a known harmonic function ------------------------------------------------

def _log_r(p):
    return 0.5 * np.log(p[:, 0] ** 2 + p[:, 1] ** 2)


def _log_r_grad(p):
    r2 = p[:, 0] ** 2 + p[:, 1] ** 2
    return np.stack([p[:, 0] / r2, p[:, 1] / r2], axis=1)


def _exp_cos(p):
    return np.exp(p[:, 0]) * np.cos(p[:, 1])


def _exp_cos_grad(p):
    return np.stack([np.exp(p[:, 0]) * np.cos(p[:, 1]), -np.exp(p[:, 0]) * np.sin(p[:, 1])], axis=1)


def _linear(p):
    return 3 * p[:, 0] - 2 * p[:, 1] + 1


def _linear_grad(p):
    return np.tile([3.0, -2.0], (len(p), 1))


# (name, family, mesh, exact V, its gradient): rows of one family follow each other with h halved
TABLE = [
    ("annulus_17x64", "annulus", lambda: synthetic.annulus_mesh(1, 4, 17, 64), _log_r, _log_r_grad),
    ("annulus_33x128", "annulus", lambda: synthetic.annulus_mesh(1, 4, 33, 128), _log_r, _log_r_grad),
    ("annulus_65x256", "annulus", lambda: synthetic.annulus_mesh(1, 4, 65, 256), _log_r, _log_r_grad),
    ("grid_17", "grid", lambda: synthetic.jittered_grid(17, 17, h=2 / 16, seed=1), _exp_cos, _exp_cos_grad),
    ("grid_33", "grid", lambda: synthetic.jittered_grid(33, 33, h=2 / 32, seed=1), _exp_cos, _exp_cos_grad),
    ("grid_65", "grid", lambda: synthetic.jittered_grid(65, 65, h=2 / 64, seed=1), _exp_cos, _exp_cos_grad),
    ("linear_17", "linear", lambda: synthetic.jittered_grid(17, 17, h=0.125, seed=1), _linear, _linear_grad),
]
LINEAR_GRADIENT = math.hypot(3.0, 2.0)


def stiffness(xy, tri) -> sp.csr_matrix:
    """The P1 stiffness matrix (signed cotangent weights), unit conductance."""
    p = [xy[tri[:, k]] for k in range(3)]
    area2 = (p[1][:, 0] - p[0][:, 0]) * (p[2][:, 1] - p[0][:, 1]) - (p[1][:, 1] - p[0][:, 1]) * (p[2][:, 0] - p[0][:, 0])
    # grad phi_k = rot90(edge opposite k) / (2 A)
    grads = []
    for k in range(3):
        e = p[(k + 2) % 3] - p[(k + 1) % 3]
        grads.append(np.stack([-e[:, 1], e[:, 0]], axis=1) / area2[:, None])
    rows, cols, vals = [], [], []
    for a in range(3):
        for b in range(3):
            rows.append(tri[:, a])
            cols.append(tri[:, b])
            vals.append(np.abs(area2) / 2 * (grads[a] * grads[b]).sum(axis=1))
    n = len(xy)
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()


def boundary_vertices(tri) -> np.ndarray:
    """The vertices of the edges that belong to one face only."""
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    e.sort(axis=1)
    uniq, count = np.unique(e, axis=0, return_counts=True)
    return np.unique(uniq[count == 1])


def fem_solution(xy, tri, exact) -> np.ndarray:
    """The P1 Galerkin solution of Laplace's equation with ``exact`` prescribed at the boundary vertices."""
    xy, tri = np.asarray(xy, dtype=np.float64), np.asarray(tri, dtype=np.int64)
    K = stiffness(xy, tri)
    x = np.zeros(len(xy))
    bnd = boundary_vertices(tri)
    x[bnd] = exact(xy[bnd])
    free = np.setdiff1d(np.arange(len(xy)), bnd)
    x[free] = spla.spsolve(K[free][:, free].tocsc(), -(K[free][:, bnd] @ x[bnd]))
    return x


def true_error(xy, tri, est: Estimate, grad_exact) -> float:
    """sqrt(sum_f sigma int_f |grad V - g_f|^2) with the edge-midpoint rule (exact for degree 2) on the exact gradient."""
    xy, tri = np.asarray(xy, dtype=np.float64), np.asarray(tri, dtype=np.int64)
    total = np.zeros(len(tri))
    for a, b in ((0, 1), (1, 2), (2, 0)):
        mid = (xy[tri[:, a]] + xy[tri[:, b]]) / 2
        total += ((grad_exact(mid) - est.g) ** 2).sum(axis=1)
    return math.sqrt(float((est.sigma * est.area / 3 * total).sum()))


def table_case(row, sigma: float = 1.0):
    """(xy, tri, the FEM potentials, the gradient of the exact V) of a row of TABLE."""
    _name, _family, make, exact, grad = row
    xy, tri = make()
    xy, tri = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    return xy, tri, fem_solution(xy, tri, exact), grad

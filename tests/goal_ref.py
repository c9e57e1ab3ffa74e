"""Host restatement of the goal-oriented (dual-weighted) error estimate for the tests, built on tests/error_ref.py in the same
summation order, and the yardstick it is itself checked against: the true a(u - u_h, z - z_h) of two P1 solutions with
Dirichlet data from two known harmonic functions.

Field 0 is the solution, field 1 + j the adjoint of objective j.  With error_ref's definitions 1-4 applied to every field a,
d_c^a = G^a_(corner c) - g_f^a and m_12^a = (d_1^a + d_2^a) / 2 (likewise m_23, m_31):
 7. delta_jf = sigma (A_f / 3) (m_12^0 . m_12^(1+j) + m_23^0 . m_23^(1+j) + m_31^0 . m_31^(1+j)), signed;
 8. omega_jf = eta_f^0 eta_f^(1+j);
 9. per mesh the sums of omega and delta and the face with the largest omega (the lowest on a tie; a NaN never wins);
10. bound_j = sum_f omega_jf, correction_j = CORRECTION_SIGN sum_f delta_jf with CORRECTION_SIGN = -1: the estimate of
    J(exact) - J_h.  On the copper block M = -K, so the adjoint lambda = M^-T c is minus the dual solution z of K z = c, and
    J(exact) - J_h = a(u - u_h, z - z_h) = -a(u - u_h, lambda - lambda_h);
11. xi_jf = omega_jf / (tolerance / n_faces), n_faces the faces of the connected meshes.
Disconnected meshes: zeros throughout, and their faces do not count in n_faces."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import error_ref as R

CORRECTION_SIGN = -1.0


@dataclass
class Goal:
    primal: R.Estimate        # error_ref's estimate of field 0
    duals: list               # error_ref's estimate of every other field
    eta: np.ndarray           # (n_obj, n_tri) eta_f of every adjoint
    delta: np.ndarray         # (n_obj, n_tri)
    omega: np.ndarray         # (n_obj, n_tri)
    mesh_omega: np.ndarray    # (n_obj, n_mesh)
    mesh_delta: np.ndarray    # (n_obj, n_mesh)
    mesh_top: np.ndarray      # (n_obj, n_mesh) the largest omega_f, -1.0 for a mesh without faces
    mesh_face: np.ndarray     # (n_obj, n_mesh) its global face, -1 for a mesh without faces
    bound: np.ndarray         # (n_obj,)
    correction: np.ndarray    # (n_obj,)
    n_faces: int
    face_mesh: np.ndarray     # (n_tri,) as given

    def pair_scale(self, tri, j) -> np.ndarray:
        """The product of the two fields' eta_scale: what the rounding of delta_jf and omega_jf is relative to."""
        return self.primal.eta_scale(tri) * self.duals[j].eta_scale(tri)


def _midpoints(est: R.Estimate, tri):
    c = np.stack([tri[:, 2], tri[:, 0], tri[:, 1]], axis=1)
    d = est.G[c] - est.g[:, None, :]
    return (d[:, 0] + d[:, 1]) / 2, (d[:, 1] + d[:, 2]) / 2, (d[:, 2] + d[:, 0]) / 2


def goal_flat(xy, tri, face_mesh, sigma, fields, connected=None) -> Goal:
    """Definitions 7-10 for ``fields`` (n_fields, n_vert), n_fields >= 2; the other arguments are ``estimate_flat``'s."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    face_mesh = np.asarray(face_mesh, dtype=np.int64)
    fields = np.asarray(fields, dtype=np.float64)
    assert fields.ndim == 2 and fields.shape[0] >= 2
    n_tri, n_mesh, n_obj = len(tri), len(np.asarray(sigma)), fields.shape[0] - 1
    primal = R.estimate_flat(xy, tri, face_mesh, sigma, fields[0], connected)
    duals = [R.estimate_flat(xy, tri, face_mesh, sigma, f, connected) for f in fields[1:]]
    live_mesh = np.ones(n_mesh, dtype=bool) if connected is None else np.asarray(connected, dtype=bool)
    live = live_mesh[face_mesh] if n_tri else np.zeros(0, dtype=bool)
    m0 = _midpoints(primal, tri)
    eta, delta, omega = (np.zeros((n_obj, n_tri)) for _ in range(3))
    mesh_omega, mesh_delta = np.zeros((n_obj, n_mesh)), np.zeros((n_obj, n_mesh))
    top, top_face = np.full((n_obj, n_mesh), -1.0), np.full((n_obj, n_mesh), -1, dtype=np.int64)
    for j, dual in enumerate(duals):
        mj = _midpoints(dual, tri)
        dots = [(a * b).sum(axis=1) for a, b in zip(m0, mj)]
        de = primal.sigma * (primal.area / 3) * ((dots[0] + dots[1]) + dots[2])
        eta[j] = dual.eta
        delta[j] = np.where(live, de, 0.0)
        omega[j] = np.where(live, primal.eta * dual.eta, 0.0)
        if n_tri:
            mesh_omega[j] = np.bincount(face_mesh, weights=omega[j], minlength=n_mesh)
            mesh_delta[j] = np.bincount(face_mesh, weights=delta[j], minlength=n_mesh)
        for m in range(n_mesh):
            faces = np.flatnonzero(face_mesh == m)
            if len(faces) and not np.isnan(omega[j, faces]).all():
                f = faces[int(np.nanargmax(omega[j, faces]))]              # the first maximum: the lowest face
                top[j, m], top_face[j, m] = omega[j, f], f
    return Goal(primal=primal, duals=duals, eta=eta, delta=delta, omega=omega, mesh_omega=mesh_omega, mesh_delta=mesh_delta,
                mesh_top=top, mesh_face=top_face, bound=mesh_omega.sum(axis=1), correction=CORRECTION_SIGN * mesh_delta.sum(axis=1),
                n_faces=int(live.sum()), face_mesh=face_mesh)


def goal_ratios(goal: Goal, tolerance: float) -> np.ndarray:
    """Definition 11: xi_jf (n_obj, n_tri)."""
    return goal.omega / (tolerance / goal.n_faces)


# ---- the yardstick: two P1 solutions against two known harmonic functions -----------------------------------------------

def _xy_product(p):
    return p[:, 0] * p[:, 1]


def _xy_product_grad(p):
    return np.stack([p[:, 1], p[:, 0]], axis=1)


OFF_CENTRE = np.array([0.3, 0.2])


def _log_off_centre(p):
    """ln |p - c| with c inside the annulus' hole: harmonic on the annulus, and not orthogonal to ln r as every cos(m theta)
    mode about the origin is."""
    q = p - OFF_CENTRE
    return 0.5 * np.log((q ** 2).sum(axis=1))


def _log_off_centre_grad(p):
    q = p - OFF_CENTRE
    return q / (q ** 2).sum(axis=1)[:, None]


def _exp_sin(p):
    return np.exp(p[:, 0]) * np.sin(p[:, 1])


def _exp_sin_grad(p):
    return np.stack([np.exp(p[:, 0]) * np.sin(p[:, 1]), np.exp(p[:, 0]) * np.cos(p[:, 1])], axis=1)


# the second harmonic function of every family of error_ref.TABLE: (exact z, its gradient)
SECOND = {"annulus": (_log_off_centre, _log_off_centre_grad), "grid": (_exp_sin, _exp_sin_grad), "linear": (_xy_product, _xy_product_grad)}


def pair_case(row):
    """(xy, tri, u_h, z_h, grad u, grad z) of a row of error_ref.TABLE: its own function and the family's second one."""
    xy, tri, u_h, grad_u = R.table_case(row)
    exact_z, grad_z = SECOND[row[1]]
    return xy, tri, u_h, R.fem_solution(xy, tri, exact_z), grad_u, grad_z


def true_product(xy, tri, goal: Goal, grad_u, grad_z, j: int = 0) -> float:
    """a(u - u_h, z - z_h) = sum_f sigma int_f (grad u - g_f^0) . (grad z - g_f^(1+j)) with the edge-midpoint rule of
    ``error_ref.true_error`` on the exact gradients."""
    xy, tri = np.asarray(xy, dtype=np.float64), np.asarray(tri, dtype=np.int64)
    total = np.zeros(len(tri))
    for a, b in ((0, 1), (1, 2), (2, 0)):
        mid = (xy[tri[:, a]] + xy[tri[:, b]]) / 2
        total += ((grad_u(mid) - goal.primal.g) * (grad_z(mid) - goal.duals[j].g)).sum(axis=1)
    return float((goal.primal.sigma * goal.primal.area / 3 * total).sum())

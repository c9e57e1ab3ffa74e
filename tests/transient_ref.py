"""Host restatement of the transient thermal model for the tests ("Transient"), on top of tests/thermal_ref.py:
backward Euler on C dtheta/dt + A theta = b(t), every expression rounded as the device states it, the steps by a scipy
direct solve.

 1. Cv[v] = c_m(v) * M_v (one product); cdt[v] = Cv[v] / dt (one division).
 2. S = A with S_vv = A_vv + cdt[v] at a vertex (one rounded sum); every other entry is A's.
 3. rhs[v] = cdt[v] * theta_n[v] + B[j][v] at a vertex (no sum when the sources are off, j = None); B[j][v] or 0.0 at an
    internal node.
 4. theta_{n+1} = S^-1 rhs (splu, one factorisation per distinct dt).
 5. per step and mesh: the largest theta (the lowest vertex on a tie; -inf and -1 without vertices), stored = sum Cv theta
    and loss = sum (h M_v) theta (math.fsum here: the device's fixed-order sums agree to rounding).
 6. envelope along time: theta_0 first with step 0, a later step replaces the value only when strictly greater."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def capacity(voff, areal_capacity, M) -> np.ndarray:
    """Definition 1: ``areal_capacity`` per mesh, ``M`` the lumped areas."""
    return np.repeat(np.asarray(areal_capacity, dtype=np.float64), np.diff(voff)) * np.asarray(M, dtype=np.float64)


def step_matrix(A, Cv, dt: float) -> sp.csr_matrix:
    """Definition 2."""
    S = sp.csr_matrix(A).copy()
    d = S.diagonal()
    n_vert = len(Cv)
    d[:n_vert] = d[:n_vert] + Cv / dt
    S.setdiag(d)
    S.sort_indices()
    return S


def rhs(Cv, dt: float, theta, b=None) -> np.ndarray:
    """Definition 3 for one column; ``b`` None: sources off."""
    theta = np.asarray(theta, dtype=np.float64)
    n_vert = len(Cv)
    out = np.zeros(len(theta))
    out[:n_vert] = (Cv / dt) * theta[:n_vert]
    if b is not None:
        out[:n_vert] = out[:n_vert] + b[:n_vert]
        out[n_vert:] = b[n_vert:]
    return out


class Stepper:
    """Backward-Euler steps of one column, one factorisation per distinct dt."""

    def __init__(self, A, Cv):
        self.A, self.Cv, self._lu = sp.csr_matrix(A), np.asarray(Cv, dtype=np.float64), {}

    def step(self, theta, dt: float, b=None) -> np.ndarray:
        if dt not in self._lu:
            self._lu[dt] = spla.splu(sp.csc_matrix(step_matrix(self.A, self.Cv, dt)))
        return self._lu[dt].solve(rhs(self.Cv, dt, theta, b))


def mesh_report(voff, Cv, hM, theta):
    """Definition 5 for one column: per mesh (max theta, its vertex, stored, loss)."""
    n_mesh = len(voff) - 1
    top, vert, stored, loss = np.full(n_mesh, -np.inf), np.full(n_mesh, -1, dtype=np.int64), np.zeros(n_mesh), np.zeros(n_mesh)
    for m in range(n_mesh):
        lo, hi = int(voff[m]), int(voff[m + 1])
        if hi > lo:
            k = int(np.argmax(theta[lo:hi]))
            top[m], vert[m] = theta[lo + k], lo + k
        stored[m] = math.fsum((Cv[lo:hi] * theta[lo:hi]).tolist())
        loss[m] = math.fsum((hM[lo:hi] * theta[lo:hi]).tolist())
    return top, vert, stored, loss


def envelope(states):
    """Definition 6 down the first axis of ``states`` (n_steps + 1, n): (max, the first step that attains it)."""
    states = np.asarray(states, dtype=np.float64)
    best, step = states[0].copy(), np.zeros(states.shape[1], dtype=np.int32)
    for k in range(1, states.shape[0]):
        greater = states[k] > best
        best[greater] = states[k][greater]
        step[greater] = k
    return best, step


def run(A, Cv, hM, voff, B, schedule, theta0=None):
    """One column through ``schedule``, a sequence of (dt, n_steps, case or None): (states (n_steps + 1, n_pot), per step and
    mesh max / vertex / stored / loss (n_steps + 1, n_mesh) with step 0 the start, envelope (n_vert,), its steps)."""
    stepper = Stepper(A, Cv)
    n_pot, n_vert = A.shape[0], len(Cv)
    theta = np.zeros(n_pot) if theta0 is None else np.asarray(theta0, dtype=np.float64).copy()
    states = [theta]
    for dt, n_steps, case in schedule:
        for _ in range(int(n_steps)):
            theta = stepper.step(theta, dt, None if case is None else B[case])
            states.append(theta)
    states = np.stack(states)
    reports = [mesh_report(voff, Cv, hM, th) for th in states]
    top, vert, stored, loss = (np.stack([r[i] for r in reports]) for i in range(4))
    best, step = envelope(states[:, :n_vert])
    return states, top, vert, stored, loss, best, step

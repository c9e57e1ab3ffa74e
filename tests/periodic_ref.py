"""Host specification of the periodic steady state of a duty cycle ("Periodic steady state"), on top of
tests/transient_ref.py (the stepping) and tests/fold_ref.py (the fixed reduction order).

The period map of the fixed-step scheme is affine, theta(T) = Phi theta(0) + d; the periodic state solves
(I - Phi) theta* = d.  GMRES without restart in the inner product <x, y>_C = sum_v Cv[v] x[v] y[v] over the vertices:

 1. x0 given; r0 = (Phi x0 + d) - x0, one period under the schedule's cases.  If max_v |r0| <= tolerance: the answer is x0.
 2. beta = sqrt(<r0, r0>_C), v_0 = r0 / beta (zeros when beta is not positive: a frozen column).
 3. For j = 0, 1, ...: w = v_j - Phi v_j (one period with the sources off); twice: d_i = <w, v_i>_C for i <= j, then
    w = w - sum_i d_i v_i; h_ij = the sum of the two d_i; h_{j+1,j} = sqrt(<w, w>_C); v_{j+1} = w / h_{j+1,j} (zeros and
    frozen when that is not positive); y = argmin |beta e_1 - H y| by numpy; the predicted closure is
    max_v |r0 - V_{j+2} (H y)|; stop when it is <= tolerance.
 4. theta = x0 + V y.

The arithmetic of the device kernels, every expression rounded as written:
    dot      term[v] = (Cv[v] * w[v]) * v_i[v] over the vertices, summed by fold_ref.mesh_sum over the whole vertex range
    update   s = 0.0; s = s + d_i * v_i for i ascending; w = w - s        (all entries, internal nodes included)
    combine  a = base; a = a + c_i * v_i for i ascending                   (all entries)
    top      fold_ref.mesh_top of |a| over the vertices with the empty top (-inf, NO_INDEX); a value that is not finite counts
             as +inf; (0.0, -1) without vertices
Vectors carry all n_pot entries; the internal nodes ride along linearly."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

import fold_ref as F
import transient_ref as R

EMPTY_TOP = (-math.inf, F.NO_INDEX)


# ---- the kernels ----------------------------------------------------------------------------------------------------------

def dot(Cv, w, v) -> float:
    n_vert = len(Cv)
    return F.mesh_sum((Cv * w[:n_vert]) * v[:n_vert])


def root(sq: float) -> float:
    """sqrt of a squared norm: 0.0 stays, what is no number is handed on."""
    return math.sqrt(sq) if sq > 0.0 else sq


def update(w, d, V):
    s = np.zeros(len(w))
    for di, vi in zip(d, V):
        s = s + di * vi
    return w - s


def combine(base, coef, V):
    a = np.array(base, dtype=np.float64)
    for ci, vi in zip(coef, V):
        a = a + ci * vi
    return a


def top(a, n_vert: int) -> tuple:
    """(max |a| over the vertices, the lowest vertex that attains it)."""
    if n_vert == 0:
        return 0.0, -1
    with np.errstate(invalid="ignore"):
        mag = np.abs(np.asarray(a, dtype=np.float64)[:n_vert])
        mag = np.where(mag <= 1.7976931348623157e308, mag, np.inf)
    value, at = F.mesh_top(mag, np.arange(n_vert, dtype=np.int64), empty=EMPTY_TOP)
    return value, at


def scaled(w, h: float):
    return w / h if h > 0.0 else np.zeros(len(w))


def residual(Cv, state, x0):
    """padne_periodic_residual for one column: (r0, beta, v_0, (max |r0|, vertex))."""
    r0 = state - x0
    beta = root(dot(Cv, r0, r0))
    return r0, beta, scaled(r0, beta), top(r0, len(Cv))


def push(Cv, V, state):
    """padne_periodic_push for one column, V = [v_0 .. v_j]: (the Hessenberg column (j + 2,), v_{j+1})."""
    w = V[-1] - state
    h = np.zeros(len(V) + 1)
    for _ in range(2):
        d = np.array([dot(Cv, w, v) for v in V])
        w = update(w, d, V)
        h[:-1] = h[:-1] + d
    h[-1] = root(dot(Cv, w, w))
    return h, scaled(w, h[-1])


def predict(r0, coef, V, n_vert: int) -> tuple:
    return top(combine(r0, [-c for c in coef], V), n_vert)


# ---- the period map -------------------------------------------------------------------------------------------------------

class Period:
    """One period of transient_ref's stepping for one column: ``schedule`` = [(dt, steps, case or None)], B the load table."""

    def __init__(self, A, Cv, B, schedule):
        self.stepper, self.B, self.schedule = R.Stepper(A, Cv), B, list(schedule)
        self.Cv, self.n_vert, self.n_pot = np.asarray(Cv, dtype=np.float64), len(Cv), A.shape[0]
        self.steps = sum(int(s) for _dt, s, _c in self.schedule)

    def states(self, theta, sources=True):
        """The states of one period from ``theta``, (steps + 1, n_pot)."""
        out = [np.asarray(theta, dtype=np.float64)]
        for dt, steps, case in self.schedule:
            for _ in range(int(steps)):
                out.append(self.stepper.step(out[-1], dt, self.B[case] if sources and case is not None else None))
        return np.stack(out)

    def apply(self, theta, sources=True):
        """Phi theta + d, or Phi theta alone without ``sources``."""
        return self.states(theta, sources)[-1]

    def closure(self, theta) -> float:
        return top(self.apply(theta) - theta, self.n_vert)[0]


def least_squares(H, beta: float):
    """y of min |beta e_1 - H y|, H (j + 2, j + 1)."""
    e = np.zeros(H.shape[0])
    e[0] = beta
    return np.linalg.lstsq(H, e, rcond=None)[0]


def gmres(period: Period, x0, tolerance: float, max_periods: int = 64) -> dict:
    """Steps 1 to 4 for one column.  ``theta``: the iterate; ``predicted``: the predicted closure after every Krylov step;
    ``periods``: period applications spent, the first, the Krylov ones and the one that records the cycle; ``first``: the
    closure of x0; ``V``, ``H``, ``y``, ``beta``: the basis and the small problem; ``frozen``."""
    Cv, n_vert = period.Cv, period.n_vert
    x0 = np.asarray(x0, dtype=np.float64)
    r0, beta, v0, (first, _at) = residual(Cv, period.apply(x0), x0)
    out = {"first": first, "predicted": [], "beta": beta, "V": [v0], "H": np.zeros((1, 0)), "y": np.zeros(0), "frozen": not beta > 0.0}
    if first <= tolerance or out["frozen"]:
        return dict(out, theta=x0, periods=2)
    V, H = out["V"], out["H"]
    for j in range(max_periods - 2):
        h, nxt = push(Cv, V, period.apply(V[j], sources=False))
        H = np.pad(H, ((0, 1), (0, 1)))
        H[:j + 2, j] = h
        V.append(nxt)
        y = least_squares(H, beta)
        out["predicted"].append(predict(r0, H @ y, V, n_vert)[0])
        out.update(H=H, y=y)
        if not h[-1] > 0.0:
            out["frozen"] = True
        if out["predicted"][-1] <= tolerance or out["frozen"]:
            break
    return dict(out, theta=combine(x0, out["y"], V), periods=2 + len(out["predicted"]))


def brute_force(period: Period, x0, tolerance: float, max_periods: int = 100000) -> tuple:
    """Repetition from x0: (the periods run until one closes within ``tolerance``, the state that cycle starts from)."""
    theta = np.asarray(x0, dtype=np.float64)
    for n in range(1, max_periods + 1):
        nxt = period.apply(theta)
        if top(nxt - theta, period.n_vert)[0] <= tolerance:
            return n, theta
        theta = nxt
    raise RuntimeError("brute-force repetition did not close")


# ---- the dense check ------------------------------------------------------------------------------------------------------

def dense_period(A, Cv, B, schedule) -> tuple:
    """(Phi (n_pot, n_pot), d (n_pot,)) from explicit step matrices: a step is theta' = S^-1 (D theta + b), S =
    transient_ref.step_matrix, D = diag(Cv / dt) on the vertices and 0 on the internal nodes."""
    n_pot, n_vert = A.shape[0], len(Cv)
    Phi, d = np.eye(n_pot), np.zeros(n_pot)
    for dt, steps, case in schedule:
        S = R.step_matrix(A, Cv, dt).toarray()
        D = np.zeros(n_pot)
        D[:n_vert] = Cv / dt
        M = np.linalg.solve(S, np.diag(D))
        b = np.zeros(n_pot) if case is None else np.linalg.solve(S, np.asarray(B[case], dtype=np.float64))
        for _ in range(int(steps)):
            Phi, d = M @ Phi, M @ d + b
    return Phi, d


def dense_periodic_state(Phi, d):
    """theta* = (I - Phi)^-1 d, and ||(I - Phi)^-1||_inf."""
    inv = np.linalg.inv(np.eye(len(d)) - Phi)
    return inv @ d, float(np.abs(inv).sum(axis=1).max())

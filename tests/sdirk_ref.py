"""Host restatement of the adaptive transient ("Adaptive transient") for the tests, on top of
tests/transient_ref.py: Alexander's two-stage SDIRK2 from two backward-Euler solves, every expression rounded as the device
states it, the solves by a scipy direct factorisation; the dyadic step-size rule; a run over spans.

 1. gamma = 1 - 1/sqrt(2), q = (1 - gamma) / gamma = sqrt(2) + 1, each the nearest double of its decimal expansion.
 2. dts = gamma * dt (one rounded product).
 3. theta_1 = S(dts)^-1 rhs(dts, theta_n, b): transient_ref's step of length dts.
 4. theta*[v] = theta_n[v] + q * (theta_1[v] - theta_n[v]) at a vertex, theta_1 at an internal node.
 5. theta_{n+1} = S(dts)^-1 rhs(dts, theta*, b).
 6. est[v] = q * ((theta_1[v] - theta_n[v]) - (theta_{n+1}[v] - theta*[v])) at a vertex; err = max |est| with the lowest
    vertex on a tie (0.0 and -1 without vertices); an |est| that is not finite counts as +inf.
 7. the rule: per span of duration D steps of D / 2^k; start at the smallest k with D / 2^k <= first_step (default D / 1024);
    reject (k + 1, pos * 2) when err > tolerance above the deepest level (the largest k with D / 2^k >= min_step, default 30);
    otherwise accept (pos + 1), the span ends at pos = 2^k; after an accept with err <= tolerance / 4, an even pos and k > 0:
    k - 1, pos / 2.  Stated here as a plain loop, not as the product's generator."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import transient_ref as R

GAMMA = 0.29289321881345247560
Q = 2.41421356237309504880


def growth(z: float) -> float:
    """R(z) = (1 + (1 - 2 gamma) z) / (1 - gamma z)^2: what one step multiplies the distance to the steady state of a mode
    theta' = -(theta - theta_inf) / tau by, z = -dt / tau."""
    return (1 + (1 - 2 * GAMMA) * z) / (1 - GAMMA * z) ** 2


def extrapolate(theta_n, theta_1, n_vert: int) -> np.ndarray:
    """Definition 4."""
    theta_n, theta_1 = np.asarray(theta_n, dtype=np.float64), np.asarray(theta_1, dtype=np.float64)
    star = theta_1.copy()
    star[..., :n_vert] = theta_n[..., :n_vert] + Q * (theta_1[..., :n_vert] - theta_n[..., :n_vert])
    return star


def estimate(theta_n, theta_1, star, theta_new, n_vert: int) -> np.ndarray:
    """Definition 6, the vector est over the vertices."""
    cut = lambda a: np.asarray(a, dtype=np.float64)[..., :n_vert]                        # noqa: E731
    return Q * ((cut(theta_1) - cut(theta_n)) - (cut(theta_new) - cut(star)))


def error_of(est) -> tuple:
    """Definition 6: (err, its vertex) of one column's est."""
    if len(est) == 0:
        return 0.0, -1
    with np.errstate(invalid="ignore"):
        a = np.abs(np.asarray(est, dtype=np.float64))
        a = np.where(a <= np.finfo(np.float64).max, a, np.inf)
    v = int(np.argmax(a))                    # the first of the maxima
    return float(a[v]), v


class Stepper:
    """SDIRK2 steps of one column, one factorisation per distinct dts."""

    def __init__(self, A, Cv):
        self.A, self.Cv, self._lu = sp.csr_matrix(A), np.asarray(Cv, dtype=np.float64), {}
        self.n_vert = len(self.Cv)

    def stage(self, theta, dts: float, b=None) -> np.ndarray:
        if dts not in self._lu:
            self._lu[dts] = spla.splu(sp.csc_matrix(R.step_matrix(self.A, self.Cv, dts)))
        return self._lu[dts].solve(R.rhs(self.Cv, dts, theta, b))

    def step(self, theta_n, dt: float, b=None) -> dict:
        """Definitions 2 - 6: {"theta_1", "star", "theta", "est", "err", "vertex"}."""
        dts = GAMMA * dt
        theta_1 = self.stage(theta_n, dts, b)
        star = extrapolate(theta_n, theta_1, self.n_vert)
        theta = self.stage(star, dts, b)
        est = estimate(theta_n, theta_1, star, theta, self.n_vert)
        err, vertex = error_of(est)
        return {"theta_1": theta_1, "star": star, "theta": theta, "est": est, "err": err, "vertex": vertex}


def uniform(A, Cv, b, span: float, steps: int, theta0=None) -> np.ndarray:
    """The states (steps + 1, n_pot) of ``steps`` equal SDIRK2 steps over ``span`` under the load ``b`` (None: off)."""
    stepper = Stepper(A, Cv)
    theta = np.zeros(A.shape[0]) if theta0 is None else np.asarray(theta0, dtype=np.float64).copy()
    states = [theta]
    for _ in range(int(steps)):
        theta = stepper.step(theta, span / steps, b)["theta"]
        states.append(theta)
    return np.stack(states)


def levels(duration: float, first_step=None, min_step=None) -> tuple:
    """Definition 7: (the start level, the deepest level)."""
    start = 10
    if first_step is not None:
        start = next(k for k in range(0, 1000) if duration / 2.0 ** k <= first_step)
    deepest = 30
    if min_step is not None:
        fits = [k for k in range(0, 1000) if duration / 2.0 ** k >= min_step]
        deepest = fits[-1] if fits else 0
    return start, deepest


def walk(spans, tolerance: float, trial, first_step=None, min_step=None, max_steps=100000, accepted=None) -> dict:
    """Definition 7 over ``spans`` = [(duration, load)].  ``trial(dt, load)`` -> (err, a token); ``taken`` lists
    (dt, time, load, err, token) of every accepted step, ``decisions`` the verdict on every trial ("accept", "forced",
    "reject"), ``errors`` every trial's err, ``grown`` the number of the accepted step after which the step doubled.
    ``accepted(token)`` is called when a step is taken, before the next trial."""
    out = {"taken": [], "decisions": [], "errors": [], "grown": []}
    begin = 0.0
    for duration, load in spans:
        k, deepest = levels(duration, first_step, min_step)
        pos = 0
        while pos < 2 ** k:
            if len(out["decisions"]) >= max_steps:
                raise RuntimeError(f"{max_steps} steps tried, t = {begin + pos * (duration / 2.0 ** k)}")
            dt = duration / 2.0 ** k
            err, token = trial(dt, load)
            out["errors"].append(err)
            if not math.isfinite(err):
                raise RuntimeError("the error estimate is not finite")
            if err > tolerance and k < deepest:
                k, pos = k + 1, pos * 2
                out["decisions"].append("reject")
                continue
            out["decisions"].append("forced" if err > tolerance else "accept")
            pos += 1
            out["taken"].append((dt, begin + duration if pos == 2 ** k else begin + pos * dt, load, err, token))
            if accepted is not None:
                accepted(token)
            if pos < 2 ** k and err <= tolerance / 4 and pos % 2 == 0 and k > 0:
                k, pos = k - 1, pos // 2
                out["grown"].append(len(out["taken"]))
        begin = begin + duration
    return out


def run(A, Cv, B, spans, tolerance: float, first_step=None, min_step=None, theta0=None, max_steps=100000) -> dict:
    """One column through ``spans`` = [(duration, case or None)] under the rule: ``walk``'s dict with ``states``
    (n_steps + 1, n_pot), ``times`` (n_steps + 1,) and ``step_sizes``; the token of a step is ``Stepper.step``'s dict."""
    stepper = Stepper(A, Cv)
    states = [np.zeros(A.shape[0]) if theta0 is None else np.asarray(theta0, dtype=np.float64).copy()]

    def trial(dt, case):
        got = stepper.step(states[-1], dt, None if case is None else B[case])
        return got["err"], got

    out = walk(spans, tolerance, trial, first_step, min_step, max_steps, accepted=lambda got: states.append(got["theta"]))
    out["states"] = np.stack(states)
    out["times"] = np.array([0.0] + [t[1] for t in out["taken"]])
    out["step_sizes"] = np.array([t[0] for t in out["taken"]])
    return out

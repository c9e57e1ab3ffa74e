"""``solve_meshed_thermal_periodic`` on one board: what the periodic steady state of a duty cycle costs next to running the
cycle until the start-up transient has died.

The board, the film and the capacity are those of ``scripts/transient.py`` (about 1 M unknowns, tau = c / h = 300 s).  The
duty cycle is made of the first two stretches of ``profiles/r18_transient.json``, the second one off: on for 60 s in 20
steps (dt = 3 s), off for 20 s in 20 steps (dt = 1 s); a period of 80 s, two hierarchies per period.  The tolerance is
``--relative`` (1e-6) of the steady hotspot's rise.

Reported: the period applications, the predicted closures and the measured one, the wall time of the call and the device
time of its step solves; then brute-force repetition on the same handles in the same process -- ``Transient.run`` per
segment, period after period from ambient, as ``solve_meshed_thermal_transient(repeat=...)`` steps, with the closure of every
period measured on the device -- until it closes as tightly as the recorded cycle did, and the wall time of
``solve_meshed_thermal_transient`` with that ``repeat``.

``kernel_bytes`` states what the three kernel families must move at the least over the whole iteration, from the counts
alone; N unknowns, V vertices, one column, Krylov steps j = 0 .. K - 1:
  periodic_dot_kernel      per launch with m basis vectors: (m + 2) V 8 (w, Cv and the vectors); a Gram-Schmidt pass over
                           j + 1 vectors is ceil((j + 1) / 8) launches, a push two passes and one launch for the norm
  periodic_update_kernel   (j + 1 + 2) N 8 per launch (the vectors, w read and written), two launches per push
  periodic_top_kernel      (j + 2 + 1) V 8 per prediction (the vectors and r0)
With ``--kernel-stats FILE`` (the ``--stats`` table of ``rocprofv3 --kernel-trace --stats -- python scripts/periodic.py
--only periodic``, a run of its own) their total time and TB/s over those bytes are added.

    python scripts/periodic.py [--side 100] [--h 0.2] [--relative 1e-6] [--only periodic] [--kernel-stats FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time
import warnings

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from load_cases import board  # noqa: E402
from padne_amd import _hip, mesh, solver  # noqa: E402
from padne_amd.structured import StructuredMesher  # noqa: E402
from transient import CAPACITY, FILM  # noqa: E402

CYCLE = [(60.0, 20, 0), (20.0, 20, None)]


def kernel_bytes(steps: int, n_pot: int, n_vert: int) -> dict:
    dot = update = top = 0
    for j in range(steps):
        n = j + 1
        chunks = [min(8, n - first) for first in range(0, n, 8)]
        dot += 2 * sum((m + 2) * n_vert * 8 for m in chunks) + 2 * n_vert * 8
        update += 2 * (n + 2) * n_pot * 8
        top += (j + 2 + 1) * n_vert * 8
    dot += 2 * n_vert * 8                                      # beta
    return {"periodic_dot_kernel": dot, "periodic_update_kernel": update, "periodic_top_kernel": top}


def kernel_stats(path: str, bytes_: dict) -> dict:
    """Calls, total and average time of the periodic kernels from a ``--stats`` table; TB/s over ``bytes_`` where stated."""
    measured = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for name in list(bytes_) + ["periodic_fold_kernel", "periodic_fold_top_kernel", "periodic_combine_kernel",
                                        "periodic_scale_kernel", "periodic_diff_kernel"]:
                if name in row["Name"]:
                    total = float(row["TotalDurationNs"])
                    measured[name] = {"calls": int(row["Calls"]), "total_us": round(total / 1e3, 3),
                                      "average_us": round(float(row["AverageNs"]) / 1e3, 3)}
                    if name in bytes_:
                        measured[name]["TB_per_s"] = round(bytes_[name] / total / 1e3, 3)
    return measured


def brute_force(prob, meshes, layer_of, model, schedule, closure: float, limit: int = 400):
    """Repetition from ambient on the handles of the one-way transient call until a period closes within ``closure``:
    (periods, wall seconds of the stepping, the closures)."""
    checked, cases, flat, initial, probes = solver._check_transient_arguments(prob, model, schedule, None, 1, (), "none", None)
    with solver._transient_session(prob, meshes, layer_of, checked, cases, initial, probes, None, None, solver._Laps(None)) as ses:
        per = _hip.Periodic(ses.transient, 1)
        try:
            closures, t = [], time.perf_counter()
            while len(closures) < limit:
                per.mark()
                for dt, steps, seg_cases in flat:
                    ses.transient.run(dt, steps, seg_cases, rtol=solver.RTOL, max_iter=solver.MAX_ITER)
                closures.append(float(per.residual()[1][0]))
                if closures[-1] <= closure:
                    break
            return len(closures), time.perf_counter() - t, closures
        finally:
            per.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0)
    ap.add_argument("--h", type=float, default=0.2)
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--relative", type=float, default=1e-6, help="the tolerance as a fraction of the steady hotspot's rise")
    ap.add_argument("--only", choices=["periodic"], default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    thermal = solver.ThermalModel(film=FILM)
    model = solver.TransientModel(thermal=thermal, areal_capacity=CAPACITY)
    schedule = [solver.Segment(duration, steps, case) for duration, steps, case in CYCLE]
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    warnings.simplefilter("ignore", solver.SolverWarning)
    _sol, steady = solver.solve_meshed_thermal(prob, meshes, layer_of, thermal)       # warm-up; and the scale of the tolerance
    rise = max(h[0] for h in steady.hotspots if h) - thermal.ambient
    tolerance = args.relative * rise
    tm: dict = {}
    t = time.perf_counter()
    _sols, rep = solver.solve_meshed_thermal_periodic(prob, meshes, layer_of, model, schedule, tolerance=tolerance, keep="none", timings=tm)
    call_s = time.perf_counter() - t
    steps = len(rep.predicted)
    out = {
        "what": "solve_meshed_thermal_periodic on the board of scripts/transient.py under a duty cycle of on 60 s (20 steps) and "
                "off 20 s (20 steps), next to repetition from ambient on the same handles, same process, warm",
        "n_vertices": n_vert, "film_W_per_K_mm2": FILM, "capacity_J_per_K_mm2": CAPACITY, "period_s": 80.0, "tau_s": CAPACITY / FILM,
        "steady_hotspot_rise_K": rise, "tolerance_K": tolerance,
        "periodic": {"periods": rep.periods, "converged": rep.converged, "closure_K": rep.closure, "predicted_K": rep.predicted,
                     "call_s": round(call_s, 3), "iteration_host_s": round(tm.get("periodic_iteration", 0.0), 4),
                     "step_solve_seconds": rep.info["seconds"], "iterations": rep.info["iterations"],
                     "hierarchies": rep.info["hierarchies"], "envelope_hotspot_degC": max(h[0] for h in rep.cycle.envelope.hotspots if h),
                     "cycle_start_hotspot_degC": max(h[0][0] for h in rep.cycle.hotspots if h[0])},
    }
    if args.only is None:
        periods, brute_s, closures = brute_force(prob, meshes, layer_of, model, schedule, rep.closure)
        t = time.perf_counter()
        _sols, long_run = solver.solve_meshed_thermal_transient(prob, meshes, layer_of, model, schedule, repeat=periods, keep="none")
        repeat_s = time.perf_counter() - t
        out["repetition"] = {"periods": periods, "closed": closures[-1] <= rep.closure, "stepping_s": round(brute_s, 3),
                             "closure_K_first_and_last": [closures[0], closures[-1]],
                             "solve_meshed_thermal_transient_repeat_call_s": round(repeat_s, 3),
                             "end_hotspot_degC": max(h[-1][0] for h in long_run.hotspots if h[-1])}
        out["periods_ratio"] = round(periods / rep.periods, 2)
        out["wall_ratio_repeat_call_over_periodic_call"] = round(repeat_s / call_s, 2)
    bytes_ = kernel_bytes(steps, n_vert, n_vert)                # the board has no internal node
    out["kernel_bytes"] = dict(bytes_, krylov_steps=steps)
    if args.kernel_stats:
        out["kernel_stats"] = kernel_stats(args.kernel_stats, bytes_)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""``solve_meshed_thermal_transient_adaptive`` on one board: what error-controlled SDIRK2 steps cost and buy next to the
fixed-step backward-Euler call.

The board, the film and the capacity are those of ``scripts/transient.py`` (about 1 M unknowns, tau = c / h = 300 s), the
schedule its three stretches: on for 60 s, on for 20 s, off for 60 s.  Everything is measured against ONE fine run: the
adaptive call at a tolerance 100 times tighter than the tighter of the two that are reported.  The error of a run is the
largest difference to the fine run's temperatures over all vertices, at the end of each of the three stretches.

Reported: per tolerance (1 % and 0.1 % of the steady hotspot's rise) the tried and rejected steps, the hierarchies, the
wall time of the call and of its stepping part, ms per trial and its split into the two stages' iteration loops and the
setup; the fixed-step call at the grid of ``scripts/transient.py`` (20 steps per stretch) and at a grid that takes the
wall time of each adaptive call (steps in proportion to the stretches); which call is nearer per millisecond; and the
iterations of the two stages under each of the three initial guesses of stage 2 (the whole 1 % run, repeated).

``kernel_bytes`` states what the two new kernels must move at the least, from the counts alone; N unknowns, V vertices:
  sdirk_extrapolate_kernel  16 N read (theta_n, theta_1), 8 N written
  sdirk_estimate_kernel     24 V read (theta_n, theta_1, theta_{n+1}), 16 bytes written per 256 vertices
With ``--kernel-stats FILE`` (the ``--stats`` table of ``rocprofv3 --kernel-trace --stats -- python
scripts/adaptive_transient.py --only adaptive``, a run of its own) their average time and TB/s are added.

    python scripts/adaptive_transient.py [--side 100] [--h 0.2] [--only adaptive] [--kernel-stats FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from load_cases import board  # noqa: E402
from padne_amd import _hip, mesh, solver  # noqa: E402
from padne_amd.structured import StructuredMesher  # noqa: E402
from transient import CAPACITY, FILM  # noqa: E402

STRETCHES = [(60.0, 0), (20.0, 0), (60.0, None)]


def fields(rep):
    """The vertex temperatures at the end of every stretch, one flat array each."""
    return [np.concatenate([zf.values for forms in kept for zf in forms]) for kept in rep.temperatures]


def errors_against(rep, fine):
    return [float(np.abs(a - b).max()) for a, b in zip(fields(rep), fine)]


def timed(fn, *args, **kw):
    tm: dict = {}
    t = time.perf_counter()
    out = fn(*args, timings=tm, **kw)
    return out, time.perf_counter() - t, tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0)
    ap.add_argument("--h", type=float, default=0.2)
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--only", choices=["adaptive"], default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    thermal = solver.ThermalModel(film=FILM)
    model = solver.TransientModel(thermal=thermal, areal_capacity=CAPACITY)
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    warnings.simplefilter("ignore", solver.SolverWarning)
    _sol, steady = solver.solve_meshed_thermal(prob, meshes, layer_of, thermal)        # warm-up, and the scale of the tolerance
    rise = max(h[0] for h in steady.hotspots if h) - thermal.ambient
    spans = [solver.Span(d, j) for d, j in STRETCHES]
    adaptive = lambda tol, **kw: timed(solver.solve_meshed_thermal_transient_adaptive, prob, meshes, layer_of, model, spans,  # noqa: E731
                                       tolerance=tol, keep="segments", **kw)
    fixed = lambda steps: timed(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, model,                      # noqa: E731
                                [solver.Segment(d, n, j) for (d, j), n in zip(STRETCHES, steps)], keep="segments")
    if args.only == "adaptive":
        adaptive(1e-2 * rise)
        adaptive(1e-2 * rise)
        return

    adaptive(1e-2 * rise)                                                               # warm: pools, plans
    (_s, fine_rep), fine_s, _tm = adaptive(1e-5 * rise)
    fine = fields(fine_rep)
    out = {"what": "solve_meshed_thermal_transient_adaptive (SDIRK2, dyadic step control) against solve_meshed_thermal_transient "
                   "(backward Euler) on the board of scripts/transient.py: on 60 s, on 20 s, off 60 s; errors are the largest "
                   "difference in K to one fine run (SDIRK2 at 1e-5 of the steady rise) at the end of each stretch, same process, warm",
           "n_vertices": n_vert, "film_W_per_K_mm2": FILM, "capacity_J_per_K_mm2": CAPACITY, "steady_rise_K": rise,
           "fine": {"tolerance_K": 1e-5 * rise, "steps": len(fine_rep.info["step_sizes"]), "tried": fine_rep.info["tried"],
                    "call_s": round(fine_s, 3)},
           "adaptive": [], "fixed": []}
    for fraction in (1e-2, 1e-3):
        (_s, rep), call_s, tm = adaptive(fraction * rise)
        info = rep.info
        run_s = tm.get("transient_run", 0.0)
        entry = {"tolerance_K": fraction * rise, "fraction_of_steady_rise": fraction, "steps": len(info["step_sizes"]),
                 "tried": info["tried"], "rejected": info["rejected"], "hierarchies": info["hierarchies"],
                 "call_s": round(call_s, 4), "run_host_s": round(run_s, 4), "ms_per_try": round(1e3 * run_s / info["tried"], 3),
                 "accepted_loop_ms_per_step_median": round(1e3 * float(np.median(info["seconds_per_step"])), 3),
                 "accepted_setup_ms_total": round(1e3 * float(info["setup_seconds_per_step"].sum()), 3),
                 "stage_iterations_median": [float(x) for x in np.median(info["stage_iterations"], axis=0)],
                 "distinct_step_sizes": len(set(info["step_sizes"].tolist())),
                 "step_sizes_s": [float(x) for x in info["step_sizes"]],
                 "errors_K": errors_against(rep, fine)}
        # the fixed-step call that takes as long: steps in proportion to the stretches, from its own measured ms per step
        (_s, r18), r18_s, tm18 = fixed([20, 20, 20])
        ms_step = 1e3 * tm18.get("transient_run", r18_s) / 60
        total = max(3, int(round(1e3 * run_s / ms_step)))
        steps = [max(1, int(round(total * d / 140.0))) for d, _j in STRETCHES]
        (_s, same), same_s, tm_same = fixed(steps)
        entry["fixed_at_equal_time"] = {"steps": steps, "call_s": round(same_s, 4), "run_host_s": round(tm_same.get("transient_run", 0.0), 4),
                                        "errors_K": errors_against(same, fine)}
        ours, theirs = max(entry["errors_K"]), max(entry["fixed_at_equal_time"]["errors_K"])
        entry["nearer_per_ms"] = ("adaptive" if ours * run_s < theirs * tm_same.get("transient_run", same_s) else "fixed") + \
            f": worst error x stepping time {ours * run_s:.4g} K s adaptive, {theirs * tm_same.get('transient_run', same_s):.4g} K s fixed"
        out["adaptive"].append(entry)
    (_s, r18), r18_s, tm18 = fixed([20, 20, 20])
    out["fixed"].append({"steps": [20, 20, 20], "call_s": round(r18_s, 4), "run_host_s": round(tm18.get("transient_run", 0.0), 4),
                         "hierarchies": r18.info["hierarchies"], "errors_K": errors_against(r18, fine)})
    guesses = {}
    default = _hip.SDIRK_GUESS
    for guess, label in ((0, "theta_1"), (1, "theta_star"), (2, "line_to_the_end_of_the_step")):
        _hip.SDIRK_GUESS = guess
        (_s, rep), _call, _tm = adaptive(1e-2 * rise)
        guesses[label] = {"stage_1_iterations": int(rep.info["stage_iterations"][:, 0].sum()),
                          "stage_2_iterations": int(rep.info["stage_iterations"][:, 1].sum()), "steps": len(rep.info["step_sizes"])}
    _hip.SDIRK_GUESS = default
    out["stage_2_guess_iterations"] = guesses
    n_pot = n_vert                                            # the board has no internal node
    bytes_ = {"sdirk_extrapolate_kernel": 24 * n_pot, "sdirk_estimate_kernel": 24 * n_vert + 16 * (-(-n_vert // 256))}
    out["kernel_bytes"] = dict(bytes_, **{k + "_us_at_8TBs": round(1e6 * v / 8e12, 2) for k, v in bytes_.items()})
    if args.kernel_stats:
        measured = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                for name in list(bytes_) + ["sdirk_fold_kernel", "transient_rhs_kernel", "transient_report_kernel", "transient_form_kernel"]:
                    if name in row["Name"]:
                        avg = float(row["AverageNs"])
                        measured[name] = {"calls": int(row["Calls"]), "average_us": round(avg / 1e3, 3)}
                        if name in bytes_:
                            measured[name]["TB_per_s"] = round(bytes_[name] / avg / 1e3, 3)
        out["kernel_stats"] = measured
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

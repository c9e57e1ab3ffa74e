"""``solve_meshed_thermal_transient`` on one board: what a backward-Euler step costs next to the steady solve.

The board is that of ``scripts/load_cases.py`` (four ``Rect`` layers of 35 um copper meshed by ``StructuredMesher``, about
1 M unknowns by default, tied by a lattice of 1 mOhm vias), with all its loads on.  The thermal model is Wiedemann-Franz
with a film of 1e-5 W/(K mm^2) and an areal capacity of 3e-3 J/(K mm^2) (1.6 mm of FR4 under the foil): tau = c / h = 300 s.
The schedule has three segments of 20 steps each: on for 60 s (dt = 3 s), on for 20 s (dt = 1 s: a change of dt), off for
60 s (dt = 3 s again).  Per step it reports the device time of the iteration loop, the iterations and the setup time of
the hierarchy (zero on all but the first step of a dt), and next to them the iterations and the time of the one-column
steady ``solve_meshed_thermal`` of the same board from zero, in the same process.

``kernel_bytes`` states what the two per-step kernels must move at the least, from the counts alone (nothing measured),
and how long that takes at 8 TB/s; V vertices, one column:
  transient_rhs_kernel     8 V of Cv + 8 V of theta + 8 V of B read, 8 V written
  transient_report_kernel  8 V of theta + 8 V of h M_v + 8 V of Cv + 8 V of the envelope read, up to 12 V written (the envelope)
Prints one JSON object, and writes it to ``--out``.

    python scripts/transient.py [--side 100] [--h 0.2] [--out FILE]
"""
from __future__ import annotations

import argparse
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
from padne_amd import mesh, solver  # noqa: E402
from padne_amd.structured import StructuredMesher  # noqa: E402

FILM = 1e-5                     # W/(K mm^2): 10 W/(m^2 K), still air on both faces of a board
CAPACITY = 3e-3                 # J/(K mm^2): 1.6 mm of FR4 under the foil
PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    thermal = solver.ThermalModel(film=FILM)
    model = solver.TransientModel(thermal=thermal, areal_capacity=CAPACITY)
    schedule = [solver.Segment(60.0, 20, 0), solver.Segment(20.0, 20, 0), solver.Segment(60.0, 20, None)]
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    warnings.simplefilter("ignore", solver.SolverWarning)
    solver.solve_meshed_thermal(prob, meshes, layer_of, thermal)                # warm-up: library, context, pools
    tm_steady: dict = {}
    t = time.perf_counter()
    _sol, steady = solver.solve_meshed_thermal(prob, meshes, layer_of, thermal, timings=tm_steady)
    steady_s = time.perf_counter() - t
    tm: dict = {}
    t = time.perf_counter()
    _sols, rep = solver.solve_meshed_thermal_transient(prob, meshes, layer_of, model, schedule, keep="none", timings=tm)
    transient_s = time.perf_counter() - t
    its, secs, setup = (rep.info[key] for key in ("iterations_per_step", "seconds_per_step", "setup_seconds_per_step"))
    rhs_bytes, report_bytes = 32 * n_vert, 44 * n_vert
    out = {
        "what": "solve_meshed_thermal_transient, 3 segments of 20 backward-Euler steps (dt 3 s, 1 s, 3 s; on, on, off), next to "
                "the one-column steady solve_meshed_thermal of the same board from zero, same process, warm",
        "n_vertices": n_vert, "film_W_per_K_mm2": FILM, "capacity_J_per_K_mm2": CAPACITY,
        "steady": {"iterations": steady.info["iterations"], "solve_seconds": steady.info["seconds"], "call_s": round(steady_s, 3),
                   "thermal_solve_host_s": round(tm_steady.get("thermal_solve", 0.0), 4),
                   "hotspot_degC": max(h[0] for h in steady.hotspots if h)},
        "transient": {"call_s": round(transient_s, 3), "start_host_s": round(tm.get("transient_start", 0.0), 4),
                      "run_host_s": round(tm.get("transient_run", 0.0), 4), "hierarchies": rep.info["hierarchies"],
                      "iterations": rep.info["iterations"], "rel_residual": rep.info["rel_residual"],
                      "times_s": [round(float(x), 6) for x in rep.times[1:]],
                      "iterations_per_step": [int(x) for x in its], "loop_ms_per_step": [round(1e3 * float(x), 3) for x in secs],
                      "setup_ms_per_step": [round(1e3 * float(x), 3) for x in setup],
                      "median_iterations_per_step": float(np.median(its)), "median_loop_ms_per_step": round(1e3 * float(np.median(secs)), 3),
                      "peak_degC": rep.peak[0], "peak_time_s": rep.peak[1], "end_of_heating_degC": max(h[40][0] for h in rep.hotspots if h[40])},
        "step_over_steady_iterations": round(float(np.median(its)) / max(steady.info["iterations"], 1), 3),
        "kernel_bytes": {"transient_rhs_kernel": rhs_bytes, "transient_report_kernel": report_bytes,
                         "rhs_us_at_8TBs": round(1e6 * rhs_bytes / PEAK_BYTES_PER_S, 2),
                         "report_us_at_8TBs": round(1e6 * report_bytes / PEAK_BYTES_PER_S, 2)},
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

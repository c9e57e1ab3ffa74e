"""``solve_meshed_electrothermal_transient`` next to ``solve_meshed_thermal_transient`` on one board: what a step costs once
the resistivity follows the temperature, and where the time of a step goes.

The board is that of ``scripts/load_cases.py`` (four ``Rect`` layers of 35 um copper meshed by ``StructuredMesher``, about
1 M unknowns by default, tied by a lattice of 1 mOhm vias); the thermal model and the schedule are those of
``scripts/transient.py`` (a film of 1e-5 W/(K mm^2), 3e-3 J/(K mm^2), three segments of 20 steps: on for 60 s with dt = 3 s,
on for 20 s with dt = 1 s, off for 60 s with dt = 3 s); every source is multiplied by the factor of ``scripts/coupled.py``,
chosen from the one-way steady solve so that delivered power / (film x area) is ``--rise`` kelvin.  Both calls run warm in
the same process, ``--repeats`` times each, alternated; medians are reported.  ``step_ms`` splits the on steps of the last
coupled call by host laps into scale (``padne_coupled_update_transient``), revalue, the electrical plan and solve (stage 1
and stage 2), load (the element flows on the host and ``padne_coupled_transient_load``) and the thermal step; each lap ends
with a synchronous call, so it is an upper bound of the kernels' own time (``rocprofv3 --kernel-trace --stats`` on ``--only
coupled`` gives that).

``kernel_bytes`` states what the new kernels must move at the least, from the counts alone (nothing measured), and how long
that takes at 8 TB/s; V vertices, T faces, one column:
  coupled_scale_kernel on the state    12 T of corners + 8 V of theta + 8 T of previous means read, 16 T written (+ 8 per 256 faces)
  coupled_transient_heat_kernel        8 T of face powers read, 8 per 256 faces written
  coupled_transient_range_kernel       8 T of scales read, 16 per 256 faces written
  the load slot                        what padne_coupled_solve_kkt's load moves: thermal_face_power_kernel (12 T + 16 V + 8 V +
                                       8 T read, 8 T written), thermal_load_kernel (4 V + 12 T of lists + 24 T gathered, 8 V
                                       written) and one copy of 8 V into the table (16 V)
Prints one JSON object, and writes it to ``--out``.

    python scripts/coupled_transient.py [--side 100] [--h 0.2] [--rise 30] [--repeats 3] [--only coupled] [--out FILE]
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
PEAK = 8e12                     # bytes/s
LAPS = ("scale", "revalue", "stage1", "stage2", "load", "thermal_step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--rise", type=float, default=30.0, help="delivered power / (film x area) of the scaled board [K]")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["coupled"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    thermal = solver.ThermalModel(film=FILM)
    one_way_model = solver.TransientModel(thermal=thermal, areal_capacity=CAPACITY)
    model = solver.ElectroThermalTransientModel(electrothermal=solver.ElectroThermalModel(thermal=thermal), areal_capacity=CAPACITY)
    schedule = [solver.Segment(60.0, 20, 0), solver.Segment(20.0, 20, 0), solver.Segment(60.0, 20, None)]
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)
    area = len(prob.layers) * args.side ** 2
    warnings.simplefilter("ignore", solver.SolverWarning)
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]
    _sol, rep = solver.solve_meshed_thermal(prob, meshes, layer_of, thermal)        # warm-up, and the power as it stands
    factor = float(np.sqrt(args.rise * FILM * area / rep.total_heat))
    case = {e: factor * getattr(e, solver.CASE_FIELDS[solver.element_kind(e)]) for e in sources}
    calls = {
        "one_way": lambda tm=None: solver.solve_meshed_thermal_transient(prob, meshes, layer_of, one_way_model, schedule,
                                                                         cases=[case], keep="none", timings=tm),
        "coupled": lambda tm=None: solver.solve_meshed_electrothermal_transient(prob, meshes, layer_of, model, schedule,
                                                                                cases=[case], keep="none", timings=tm),
    }
    if args.only == "coupled":
        for _ in range(args.repeats):
            calls["coupled"]()
        print(json.dumps({"only": "coupled", "repeats": args.repeats, "source_factor": factor}))
        return
    _s, one_way = calls["one_way"]()
    _s, coupled, trace = calls["coupled"]()
    ms = {key: [] for key in calls}
    laps: dict = {}
    for _ in range(args.repeats):
        for key, call in calls.items():
            tm: dict = {}
            t = time.perf_counter()
            call(tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            if key == "coupled":
                laps = tm
    med = lambda xs: float(np.median(xs))  # noqa: E731
    hot = lambda r, n: max(h[n][0] for h in r.hotspots if h[n])  # noqa: E731
    on = [s for s in laps.get("steps", []) if s["case"] is not None]
    off = [s for s in laps.get("steps", []) if s["case"] is None]
    step_ms = {k: round(1e3 * med([s[k] for s in on]), 3) for k in LAPS}
    n_tiles = (n_tri + 255) // 256
    bytes_ = {"coupled_scale_kernel": 36 * n_tri + 8 * n_vert + 8 * n_tiles,
              "coupled_transient_heat_kernel": 8 * n_tri + 8 * n_tiles,
              "coupled_transient_range_kernel": 8 * n_tri + 16 * n_tiles,
              "load_slot": (28 * n_tri + 24 * n_vert) + (36 * n_tri + 12 * n_vert) + 16 * n_vert}
    out = {
        "what": "solve_meshed_electrothermal_transient vs solve_meshed_thermal_transient, one load case, 3 segments of 20 steps "
                "(dt 3 s, 1 s, 3 s; on, on, off), same board, same process, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "film_W_per_K_mm2": FILM, "capacity_J_per_K_mm2": CAPACITY,
        "source_factor": factor, "target_mean_rise_K": args.rise,
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "coupled_over_one_way": round(med(ms["coupled"]) / med(ms["one_way"]), 2),
        "phases_ms": {k: round(1e3 * v, 1) for k, v in laps.items() if isinstance(v, float)},
        "step_ms": dict(step_ms, on_step_total=round(sum(step_ms.values()), 3),
                        off_step_thermal=round(1e3 * med([s["thermal_step"] for s in off]), 3) if off else None),
        "steps_ms": [{k: round(1e3 * v, 3) if isinstance(v, float) else v for k, v in s.items()} for s in laps.get("steps", [])],
        "iterations": trace.iterations[1:],
        "hierarchies": coupled.info["hierarchies"],
        "increments_K": [None if np.isnan(x) else float(x) for x in trace.increments],
        "scale_min": [None if np.isnan(x) else float(x) for x in trace.scale_min],
        "one_way": {"heat_W": float(one_way.total_heat[40]), "end_of_heating": hot(one_way, 40)},
        "coupled": {"heat_first_step_W": float(coupled.total_heat[1]), "heat_last_on_step_W": float(coupled.total_heat[40]),
                    "delivered_last_on_step_W": float(trace.delivered[40]), "end_of_heating": hot(coupled, 40)},
        "kernel_bytes": dict(bytes_, **{f"{k}_us_at_8TBs": round(1e6 * v / PEAK, 2) for k, v in bytes_.items()}),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

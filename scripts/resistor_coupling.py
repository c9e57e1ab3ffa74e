"""``solve_meshed_electrothermal`` with and without ``resistor_coefficient`` on one board: what it costs a round to let the
vias follow their temperature.

The board, the thermal model and the scaling of the sources are those of ``scripts/coupled.py`` (four ``Rect`` layers of
35 um copper, about 1 M unknowns by default, tied by a lattice of 1 mOhm vias; Wiedemann-Franz and a film of 1e-5 W/(K mm^2);
every source times the factor that makes delivered power / (film x area) ``--rise`` kelvin in the one-way solve).  Both calls
run warm in one process and alternate, ``--repeats`` times each; medians are reported: the call, its rounds, the time per
round, and the host laps of ``revalue`` and ``update`` (the two steps that gain launches: one kernel and a copy of the
resistors' scales behind the revalue, two kernels in the scale pass), as medians over all rounds of all repeats.  Host timers
around synchronous calls: the launch, the kernels and the read-back.  Prints one JSON object, and writes it to ``--out``.

    python scripts/resistor_coupling.py [--side 100] [--h 0.2] [--rise 30] [--repeats 3] [--out FILE]
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

FILM = 1e-5                     # W/(K mm^2), as scripts/coupled.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--rise", type=float, default=30.0, help="delivered power / (film x area) of the scaled board [K]")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    thermal_model = solver.ThermalModel(film=FILM)
    models = {"none": solver.ElectroThermalModel(thermal=thermal_model),
              "copper": solver.ElectroThermalModel(thermal=thermal_model, resistor_coefficient=solver.COPPER_TEMPERATURE_COEFFICIENT)}
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    area = len(prob.layers) * args.side ** 2
    warnings.simplefilter("ignore", solver.SolverWarning)
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]
    n_res = sum(1 for n in prob.networks for e in n.elements if solver.element_kind(e) == "Resistor")

    _sol, rep = solver.solve_meshed_thermal(prob, meshes, layer_of, thermal_model)        # warm-up, and the power as it stands
    factor = float(np.sqrt(args.rise * FILM * area / rep.total_heat))
    case = {e: factor * getattr(e, solver.CASE_FIELDS[solver.element_kind(e)]) for e in sources}

    def call(key, tm=None):
        return solver.solve_meshed_electrothermal(prob, meshes, layer_of, models[key], cases=[case], timings=tm)

    results = {key: call(key) for key in models}           # warm, and what is reported of the solutions
    ms = {key: [] for key in models}
    laps = {key: {"revalue": [], "update": [], "round": []} for key in models}
    for _ in range(args.repeats):
        for key in models:
            tm: dict = {}
            t = time.perf_counter()
            call(key, tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            for r in tm["rounds"]:
                laps[key]["revalue"].append(1e3 * r["revalue"])
                laps[key]["update"].append(1e3 * r["update"])
                laps[key]["round"].append(1e3 * sum(v for k, v in r.items() if isinstance(v, float)))
    med = lambda xs: float(np.median(xs))  # noqa: E731
    hot = lambda r: max(h[0] for h in r.hotspots if h)  # noqa: E731
    out = {"what": "solve_meshed_electrothermal with resistor_coefficient None and copper's, one load case, same board, warm, alternated",
           "n_vertices": sum(len(m.points) for m in meshes), "n_triangles": sum(len(m.triangles) for m in meshes),
           "n_resistors": n_res, "film_W_per_K_mm2": FILM, "source_factor": factor, "target_mean_rise_K": args.rise,
           "repeats": args.repeats}
    for key in models:
        _s, reps, couplings, _env = results[key]
        scales = [state["scale"] for state in couplings[0].resistors.values()]
        out[key] = {"call_ms": [round(x, 1) for x in ms[key]], "call_ms_median": round(med(ms[key]), 1),
                    "rounds": couplings[0].rounds, "converged": couplings[0].converged, "increments_K": couplings[0].increments,
                    "round_ms_median": round(med(laps[key]["round"]), 3),
                    "revalue_ms_median": round(med(laps[key]["revalue"]), 3), "update_ms_median": round(med(laps[key]["update"]), 3),
                    "delivered_W": reps[0].total_heat, "hotspot": hot(reps[0]),
                    "resistor_scale_range": [min(scales), max(scales)] if scales else None}
    out["round_copper_over_none"] = round(out["copper"]["round_ms_median"] / out["none"]["round_ms_median"], 4)
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""``solve_meshed_thermal_sensitivities`` on one board: what the derivative of a temperature with respect to every face,
layer, pair, source and element costs next to the forward calls.

The board is that of ``scripts/thermal.py`` and ``scripts/stack.py`` (4 layers, about 1 M unknowns), with the dielectric
between neighbouring layers coupled and one heat source on the top layer.  Timed in one process, warm, each the median of
``--repeats`` calls: ``solve_meshed_thermal``, ``solve_meshed_sensitivities`` (one voltage drop), and the new call with 1 and
with 8 objectives (hotspots, points and the source's footprint).

The expectation the result is held against: the call costs about one ``solve_meshed_thermal`` plus n_obj thermal and n_obj
electrical adjoint columns, on hierarchies that exist.  ``adjoint_setup_seconds`` of the call's timings is what the two
adjoint solves spent on multigrid setups: anything but 0.0 is reported as a defect.  ``ratio_to_differencing`` is the call's
time over 2 x n_parameters forward calls with n_parameters the number of layers -- the coarsest question a user could ask
by differencing (the call answers it for every face at once).

``kernel_bytes`` states what each new kernel must move at the least, from the counts alone -- N unknowns, P potentials, V
vertices, T faces, k objectives, C load cases; gathers counted once per face or vertex:
  tsens_take_kernel     8 C P read, 8 C P written
  tsens_g_kernel        8 k P written (+ the vertex lists, 4 (V + 3 T), per chunk of 8 objectives with a source among them)
  tsens_rhs_kernel      per chunk of 4 objectives the lists and the mesh, 4 (V + 3 T) + 12 T + 16 V, and per objective 16 P
                        read (lambda, x) and 8 N written
  tsens_face_kernel     the mesh once, 12 T + 16 V; per objective 32 P read (lambda, theta, x, mu) and 24 T written
  tsens_vertex_kernel   8 V (hM) and per objective 16 V read, 8 bytes written per 256 vertices
  tsens_pair_kernel     G once per objective, 12 nnz(G), and 16 V read
With ``--kernel-stats FILE`` (the ``--stats`` table of ``rocprofv3 --kernel-trace --stats -- python
scripts/thermal_sensitivity.py --only sensitivities``, a run of its own) their average time and TB/s are added.

    python scripts/thermal_sensitivity.py [--side 100] [--h 0.2] [--repeats 3] [--only sensitivities] [--kernel-stats FILE] [--out FILE]
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
from padne_amd import mesh, solver  # noqa: E402
from padne_amd.structured import StructuredMesher  # noqa: E402

FILM = 1e-5                    # W / (K mm^2): 10 W/(m^2 K), still air
PAIR = 1.5e-3                  # W / (K mm^2): 0.2 mm of FR4


def timed(fn, *args, repeats=1, **kw):
    """(the last result, the median wall time, the timings of the last call)."""
    times, tm, out = [], {}, None
    for _ in range(repeats):
        tm = {}
        t = time.perf_counter()
        out = fn(*args, timings=tm, **kw)
        times.append(time.perf_counter() - t)
    return out, float(np.median(times)), tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0)
    ap.add_argument("--h", type=float, default=0.2)
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["sensitivities"], default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    layers = prob.layers
    side = args.side
    footprint = solver.HeatSource.rectangle(layers[0], 0.6 * side, 0.6 * side, 0.7 * side, 0.68 * side, 1.0, name="regulator")
    model = solver.ThermalModel(film=FILM, interlayer={(layers[i], layers[i + 1]): PAIR for i in range(len(layers) - 1)},
                                heat_sources=[footprint])
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert, n_tri = sum(len(m.points) for m in meshes), sum(len(m.triangles) for m in meshes)
    OBJ = solver.TemperatureObjective
    eight = [OBJ.hotspot(layers[0]), OBJ.of_source("regulator"), OBJ.at(layers[0], (0.31 * side, 0.47 * side)),
             OBJ.at(layers[3], (0.52 * side, 0.52 * side)), OBJ.hotspot(layers[1]), OBJ.hotspot(layers[2]), OBJ.hotspot(layers[3]),
             OBJ.at(layers[1], (0.8 * side, 0.2 * side))]
    warnings.simplefilter("ignore", solver.SolverWarning)
    sens = lambda objectives, **kw: timed(solver.solve_meshed_thermal_sensitivities, prob, meshes, layer_of, model, objectives, **kw)  # noqa: E731
    if args.only == "sensitivities":
        sens(eight)
        sens(eight)
        return

    solver.solve_meshed_thermal(prob, meshes, layer_of, model)                          # warm: pools, code objects
    _f, forward_s, forward_tm = timed(solver.solve_meshed_thermal, prob, meshes, layer_of, model, repeats=args.repeats)
    drop = [(loads[0].f, loads[0].t)]
    _e, electrical_s, _tm = timed(solver.solve_meshed_sensitivities, prob, meshes, layer_of, drop, repeats=args.repeats)
    out = {"what": "solve_meshed_thermal_sensitivities next to solve_meshed_thermal and solve_meshed_sensitivities (one drop) on the "
                   "4-layer board of scripts/stack.py with one heat source; same process, warm, medians of --repeats calls",
           "n_vertices": n_vert, "n_faces": n_tri, "layers": len(layers), "repeats": args.repeats,
           "solve_meshed_thermal_s": round(forward_s, 4), "solve_meshed_thermal_timings": {k: round(v, 4) for k, v in forward_tm.items()},
           "solve_meshed_sensitivities_s": round(electrical_s, 4), "calls": []}
    for objectives in (eight[:1], eight):
        sens(objectives)
        (_s, _r, result), call_s, tm = sens(objectives, repeats=args.repeats)
        n_obj = len(objectives)
        setup = tm.get("adjoint_setup_seconds", float("nan"))
        out["calls"].append({
            "objectives": n_obj, "call_s": round(call_s, 4), "timings": {k: round(v, 5) for k, v in tm.items()},
            "over_one_forward_call": round(call_s / forward_s, 3),
            "extra_ms_per_objective": round(1e3 * (call_s - forward_s) / n_obj, 3),
            "adjoint_setup_seconds": setup,
            "second_multigrid_setup": "none" if setup == 0.0 else f"DEFECT: the adjoint solves spent {setup:.4f} s on multigrid setups",
            "ratio_to_differencing": round(call_s / (2 * len(layers) * forward_s), 4),
            "values": [round(s.value, 4) for s in result],
            "copper_by_layer_K": [[round(layer["copper"], 5) for layer in s.layers] for s in result]})
    n_pot, N = n_vert, n_vert + 2                            # the board has no internal node: one source row, the ground row
    bytes_ = {"tsens_take_kernel": 16 * n_pot,
              "tsens_g_kernel": 8 * 8 * n_pot + 4 * (n_vert + 3 * n_tri),
              "tsens_rhs_kernel": 4 * (n_vert + 3 * n_tri) + 12 * n_tri + 16 * n_vert + 4 * (16 * n_pot + 8 * N),
              "tsens_face_kernel": 12 * n_tri + 16 * n_vert + 8 * (32 * n_pot + 24 * n_tri),
              "tsens_vertex_kernel": 8 * n_vert + 8 * 16 * n_vert}
    out["kernel_bytes"] = dict({k + " (per launch, 8 objectives in the call: g takes 8 a launch, rhs 4)": v for k, v in bytes_.items()},
                               **{k + "_us_at_8TBs": round(1e6 * v / 8e12, 2) for k, v in bytes_.items()})
    if args.kernel_stats:
        measured = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                for name in list(bytes_) + ["tsens_pair_kernel", "tsens_fold_kernel", "tsens_owner_kernel", "tsens_rhs_res_kernel",
                                            "tsens_probe_kernel", "sources_sum_kernel"]:
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

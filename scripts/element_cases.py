"""``solve_meshed_element_cases`` against the same cases as separate ``solve_meshed`` calls on the substituted Problems,
and against ``solve_meshed_load_cases`` of as many columns.

The board is ``board()`` of ``scripts/load_cases.py`` (four ``Rect`` layers meshed by ``StructuredMesher``, about 1 M
unknowns by default, 1200 via resistors, one voltage source, 8 current loads).  Two sets of cases: an N-1 over 16 vias
(each open alone: 1 + 16 columns) and the 2^3 corners of three vias at +-20 % (1 + 3 columns); the objectives are the
drops across the first two loads.  Each set runs with fields and with ``fields=False``; the yardstick is the same cases as
``solve_meshed`` calls on ``substitute_element_case`` of each, in the same run.  All calls run warm and alternate,
``--repeats`` times each; medians are reported.  ``phases_ms`` splits each element-case call by host timers (``weights``:
the small systems on the host, ``combine``: ``combine_block`` with V' home).  ``combine_bytes`` states what the kernel must
move: V [N][columns] in, V' [N][cases] out.  Prints one JSON object, and writes it to ``--out``.

    python scripts/element_cases.py [--side 100] [--h 0.2] [--repeats 3] [--only cases] [--out FILE]

``--only cases`` runs one warm-up and the N-1 call with fields alone (a target for ``rocprofv3 --kernel-trace --stats``).
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

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["cases"], default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "element_cases.json"))
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=args.h))
    meshes, layer_of = solver.mesh_problem(prob, None, mesher)
    n_vert = sum(len(m.points) for m in meshes)
    vias = [e for net in prob.networks for e in net.elements if solver.element_kind(e) == "Resistor"]
    objectives = [(load.f, load.t) for load in loads[:2]]
    sets = {
        "n1_16": solver.open_circuit_cases(prob, vias[::len(vias) // 16][:16]),
        "corners_3": [{r: r.resistance * (1.2 if (corner >> q) & 1 else 0.8) for q, r in enumerate(vias[:3])}
                      for corner in range(8)],
    }
    columns = {"n1_16": 17, "corners_3": 4}
    # load cases of as many columns: the loads scaled, every case another setting
    load_cases = {key: [{load: load.current * (1.0 + 0.01 * j) for load in loads} for j in range(k)] for key, k in columns.items()}

    def cases_call(key, fields, timings=None):
        return solver.solve_meshed_element_cases(prob, meshes, layer_of, sets[key], objectives=objectives, fields=fields,
                                                 timings=timings)

    def separate(key, _timings=None):
        return [solver.solve_meshed(solver.substitute_element_case(prob, case), meshes, layer_of)
                for case in solver.check_element_cases(prob, sets[key])]

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sols, report = cases_call("n1_16", True)                      # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "cases":
        for _ in range(args.repeats):
            cases_call("n1_16", True)
        print(json.dumps({"only": "cases", "repeats": args.repeats}))
        return
    calls = {}
    for key in sets:
        calls[f"{key}_fields"] = lambda tm, key=key: cases_call(key, True, tm)
        calls[f"{key}_report_only"] = lambda tm, key=key: cases_call(key, False, tm)
        calls[f"{key}_separate_solve_meshed"] = lambda tm, key=key: separate(key, tm)
        calls[f"{key}_load_cases_same_columns"] = lambda tm, key=key: solver.solve_meshed_load_cases(
            prob, meshes, layer_of, load_cases[key], timings=tm)
    for call in calls.values():
        call({})
    ms = {key: [] for key in calls}
    phases = {key: [] for key in calls}
    for _ in range(args.repeats):
        for key, call in calls.items():
            tm: dict = {}
            t = time.perf_counter()
            call(tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            phases[key].append(tm)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    # against the separate solves of the same run: the worst potential of any case, relative to the largest potential
    ref = separate("n1_16")
    pot = lambda s: np.concatenate([zf.values for ls in s.layer_solutions for zf in ls.potentials])  # noqa: E731
    worst = max(float(np.abs(pot(a) - pot(b)).max() / np.abs(pot(b)).max()) for a, b in zip(sols, ref))
    N = n_vert + 2 * len(loads) + 2
    combine_bytes = {key: 8 * N * (columns[key] + len(sets[key])) for key in sets}
    out = {
        "what": "solve_meshed_element_cases (N-1 over 16 vias; 8 corners of 3 vias at +-20 %) with fields and with "
                "fields=False, vs the same cases as separate solve_meshed calls and vs solve_meshed_load_cases of as many "
                "columns; same Problem, warm, alternated",
        "n_vertices": n_vert, "unknowns": N, "vias": len(vias), "columns": columns,
        "cases": {key: len(v) for key, v in sets.items()},
        "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        **{f"{key}_separate_over_fields": round(med(ms[f"{key}_separate_solve_meshed"]) / med(ms[f"{key}_fields"]), 2)
           for key in sets},
        **{f"{key}_separate_over_report_only": round(med(ms[f"{key}_separate_solve_meshed"]) / med(ms[f"{key}_report_only"]), 2)
           for key in sets},
        "phases_ms": {k: {key: round(1e3 * med([p[key] for p in v]), 2) for key in sorted(v[0]) if key != "combine_calls"}
                      for k, v in phases.items() if v[0]},
        "combine_bytes": combine_bytes,
        "combine_min_us_at_8TBps": {key: round(1e6 * b / HBM_BYTES_PER_S, 2) for key, b in combine_bytes.items()},
        "block_iterations": int(sols[0].solver_info.iterations),
        "conditioning_min": float(report.conditioning.min()),
        "n1_16_drops_V": report.drops.tolist(),
        "n1_16_worst_rel_difference_to_separate_solves": worst,
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

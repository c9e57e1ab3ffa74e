"""``solve_meshed_thermal`` next to ``solve_meshed_currents`` and ``solve_meshed`` on one board, for 1 and for 8 load cases.

The board and the k = 8 cases are those of ``scripts/load_cases.py`` (four ``Rect`` layers of 35 um copper meshed by
``StructuredMesher``, about 1 M unknowns by default, tied by a lattice of 1 mOhm vias; each load alone, then all
together).  The thermal model is Wiedemann-Franz throughout with a film of 1e-5 W/(K mm^2) (10 W/(m^2 K)).  With 8 cases the
neighbours are ``solve_meshed_load_case_currents`` (envelope only) and ``solve_meshed_load_cases``.  All calls run warm
and alternate, ``--repeats`` times each; medians are reported.  ``phases_ms`` splits the thermal calls by host timers:
indexing, assembly, stage 1 (the electrical block solve), stage 2 (V down), the power densities and element flows of the
Solutions, the thermal setup (K, the vertex lists, M_v, A), the thermal solve (face powers, load, block solve, theta down)
and the report.  The electrical solve of the same board in the same run is the yardstick of the thermal solve: the two
systems have the same size and sparsity.

``kernel_bytes`` states what each new kernel must move at the least, from the counts alone (nothing measured; an array
that several lanes gather from counts once); V vertices, T faces, k columns, nnz entries of A:
  thermal_area_kernel           12 T of corner indices + 16 V of xy read, 8 T written
  thermal_lump_kernel           4 V of list pointers + 12 T of lists + 8 T of areas read, 16 V written
  thermal_form_kernel           4 V + 12 nnz read, 8 nnz written, 8 V of h M_v
  thermal_face_power_kernel     12 T + 16 V + 8 k V of potentials read, 8 k T written
  thermal_load_kernel           per launch of q <= 8 columns: 4 V + 12 T of lists + 8 q T of powers read, 8 q V written
  thermal_report_face_kernel    12 T + 8 k V of theta + 8 k T of powers read, 8 k T written (the face means; none without fields)
  thermal_report_vertex_kernel  8 V of h M_v + 8 k V of theta read, 12 V written (the envelope)
Prints one JSON object, and writes it to ``--out``.

    python scripts/thermal.py [--side 100] [--h 0.2] [--repeats 3] [--only thermal] [--out FILE]

``--only thermal`` runs one warm-up and the thermal calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["thermal"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    cases = [{other: 0.0 for other in loads if other is not load} for load in loads[1:]] + [{}]
    k = len(cases)
    model = solver.ThermalModel(film=FILM)
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)

    calls = {
        "thermal_1": lambda tm=None: solver.solve_meshed_thermal(prob, meshes, layer_of, model, timings=tm),
        "currents_1": lambda tm=None: solver.solve_meshed_currents(prob, meshes, layer_of, timings=tm),
        "solve_meshed_1": lambda tm=None: solver.solve_meshed(prob, meshes, layer_of),
        "thermal_8": lambda tm=None: solver.solve_meshed_thermal(prob, meshes, layer_of, model, cases=cases, timings=tm),
        "thermal_8_no_fields": lambda tm=None: solver.solve_meshed_thermal(prob, meshes, layer_of, model, cases=cases,
                                                                           per_case_fields=False, timings=tm),
        "currents_8_envelope_only": lambda tm=None: solver.solve_meshed_load_case_currents(prob, meshes, layer_of, cases,
                                                                                           per_case_fields=False, timings=tm),
        "load_cases_8": lambda tm=None: solver.solve_meshed_load_cases(prob, meshes, layer_of, cases, timings=tm),
    }
    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sol1, rep1 = calls["thermal_1"]()                            # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "thermal":
        for _ in range(args.repeats):
            calls["thermal_1"]()
            calls["thermal_8"]()
        print(json.dumps({"only": "thermal", "cases": [1, k], "repeats": args.repeats}))
        return
    sols8, reps8, env8 = calls["thermal_8"]()
    for key in calls:
        calls[key]()
    ms = {key: [] for key in calls}
    phases = {key: [] for key in calls if key.startswith("thermal")}
    for _ in range(args.repeats):
        for key, call in calls.items():
            tm: dict = {}
            t = time.perf_counter()
            call(tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            if key in phases:
                phases[key].append(tm)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    keys = ("indexing", "assembly", "stage1", "stage2", "power_density", "thermal_setup", "thermal_solve", "thermal_report",
            "solutions")
    n_pot = n_vert                                               # no internal nodes on this board
    nnz = 7 * n_vert                                             # about: six neighbours and the diagonal
    out = {
        "what": "solve_meshed_thermal vs solve_meshed_currents vs solve_meshed (1 case) and vs solve_meshed_load_case_currents "
                "(envelope only) vs solve_meshed_load_cases (8 cases), same board, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "cases": k, "film_W_per_K_mm2": FILM,
        "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "thermal_over_currents_1": round(med(ms["thermal_1"]) / med(ms["currents_1"]), 2),
        "thermal_over_currents_8": round(med(ms["thermal_8_no_fields"]) / med(ms["currents_8_envelope_only"]), 2),
        "phases_ms": {key: {p: round(1e3 * med([q.get(p, 0.0) for q in v]), 1) for p in keys} for key, v in phases.items()},
        "electrical_iterations": {"1": int(sol1.solver_info.iterations), "8": int(sols8[0].solver_info.iterations)},
        "electrical_solve_seconds": {"1": float(sol1.solver_info.solve_seconds), "8": float(sols8[0].solver_info.solve_seconds)},
        "thermal_iterations": {"1": rep1.info["iterations"], "8": reps8[0].info["iterations"]},
        "thermal_solve_seconds": {"1": rep1.info["seconds"], "8": reps8[0].info["seconds"]},
        "thermal_rel_residual": {"1": rep1.info["rel_residual"], "8": reps8[0].info["rel_residual"]},
        "kernel_bytes": {
            "thermal_area_kernel": 12 * n_tri + 16 * n_vert + 8 * n_tri,
            "thermal_lump_kernel": 4 * n_vert + 20 * n_tri + 16 * n_vert,
            "thermal_form_kernel_about": 4 * n_pot + 20 * nnz + 8 * n_vert,
            "thermal_face_power_kernel": {str(c): 12 * n_tri + 16 * n_vert + 8 * c * n_vert + 8 * c * n_tri for c in (1, k)},
            "thermal_load_kernel": {str(c): 4 * n_vert + 12 * n_tri + 8 * c * n_tri + 8 * c * n_pot for c in (1, k)},
            "thermal_report_face_kernel": {str(c): 12 * n_tri + 8 * c * n_pot + 16 * c * n_tri for c in (1, k)},
            "thermal_report_vertex_kernel": {str(c): 8 * n_vert + 8 * c * n_pot + 12 * n_vert for c in (1, k)},
        },
        "total_heat_W": rep1.total_heat, "total_loss_W": rep1.total_loss,
        "hotspots_degC": [[round(h[0], 4), h[1]] if h else None for h in rep1.hotspots],
        "envelope_hotspots_degC": [[round(h[0], 4), h[1]] if h else None for h in env8.hotspots],
        "vertices_by_worst_case": np.bincount(np.concatenate([c for cs in env8.cases for c in cs]), minlength=k).tolist(),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

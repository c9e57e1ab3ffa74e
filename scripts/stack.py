"""``solve_meshed_thermal`` with and without ``ThermalModel.interlayer`` on one board, in one process.

The board is that of ``scripts/load_cases.py`` (four ``Rect`` layers of 35 um copper meshed by ``StructuredMesher``, about
1 M unknowns by default, tied by a lattice of 1 mOhm vias, all loads on).  The thermal model is Wiedemann-Franz with a film
of 1e-5 W/(K mm^2) (10 W/(m^2 K)); the coupled model adds the three pairs of neighbouring layers at 1.5e-3 W/(K mm^2)
(0.2 mm of FR4 at 0.3 W/(m K)).  Both calls run warm and alternate, ``--repeats`` times each; medians are reported, with the
host phases of both, the iterations of both thermal solves, the hotspots, and the heat through every pair.  ``create_ms``
is the ``thermal_setup`` lap of the call's host timers -- the construction of the ``_hip.Thermal`` handle with its Python
list building, ``padne_thermal_create`` in one and ``padne_thermal_create_stacked`` in the other -- not a timer around
the C entry alone.

``kernel_bytes`` states what each new kernel must move at the least, from the counts alone (nothing measured; an array
that several lanes gather from counts once, the candidate faces of a bin come on top); Q (side, vertex) slots -- every
inner layer is the source of two sides --, E = 6 Q directed entries, G stored off-diagonals of the coupling, V vertices, nnz
entries of A:
  stack_box_kernel             16 V read, 4 V written (the layer of every vertex)
  stack_locate_kernel          24 Q read (xy, M_v) + one face at the least (12 + 48), 152 Q written (slot and six entries)
  radix sort                   16 E read and written per pass
  stack_head_kernel            8 E read, 4 E written
  stack_compact_kernel         12 E + 16 per run read, 16 G written
  stack_ptr_kernel             4 V written (bisection over 4 G)
  stack_diag_kernel            4 V + 8 G read, 8 V written
  stack_merge_kernel<false>    4 V + 4 nnz + 4 V + 4 G read, 4 V written
  stack_merge_kernel<true>     12 nnz + 12 G + 8 V read, 12 (nnz + G) written at the most
  stack_flow_kernel            per report of k columns and P pairs: 8 V of row pointers + 12 G + 4 per partner (its layer) and,
                               per column, 8 V + 8 per partner of theta read; 8 (k + 1) P per tile of 256 vertices written
  stack_fold_kernel            8 (k + 1) P per tile read, 8 (k + 1) P per mesh written
Prints one JSON object, and writes it to ``--out``.

    python scripts/stack.py [--side 100] [--h 0.2] [--repeats 3] [--only stacked] [--out FILE]

``--only stacked`` runs one warm-up and the coupled calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
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
DIELECTRIC = 1.5e-3             # W/(K mm^2): 0.2 mm of FR4 at 0.3 W/(m K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["stacked"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    pairs = {(a, b): DIELECTRIC for a, b in zip(prob.layers[:-1], prob.layers[1:])}
    models = {"plain": solver.ThermalModel(film=FILM), "stacked": solver.ThermalModel(film=FILM, interlayer=pairs)}
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)

    def call(key, tm=None):
        return solver.solve_meshed_thermal(prob, meshes, layer_of, models[key], timings=tm)

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    reports = {"stacked": call("stacked")[1]}                    # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "stacked":
        for _ in range(args.repeats):
            call("stacked")
        print(json.dumps({"only": "stacked", "repeats": args.repeats}))
        return
    reports["plain"] = call("plain")[1]
    ms = {key: [] for key in models}
    phases = {key: [] for key in models}
    for _ in range(args.repeats):
        for key in models:
            tm: dict = {}
            t = time.perf_counter()
            call(key, tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            phases[key].append(tm)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    keys = ("indexing", "assembly", "stage1", "stage2", "power_density", "thermal_setup", "thermal_solve", "thermal_report",
            "solutions")
    per_layer = [sum(len(m.points) for m, l in zip(meshes, layer_of) if l == i) for i in range(len(prob.layers))]
    slots = sum(per_layer[a] + per_layer[b] for a, b in zip(range(len(per_layer) - 1), range(1, len(per_layer))))
    entries, nnz = 6 * slots, 7 * n_vert                         # about: six neighbours and the diagonal
    stored = entries                                             # at the most: every directed entry its own
    tiles = sum((len(m.points) + 255) // 256 for m in meshes)    # the report has one column here: k + 1 = 2
    out = {
        "what": "solve_meshed_thermal with and without interlayer, same board, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "film_W_per_K_mm2": FILM, "interlayer_W_per_K_mm2": DIELECTRIC,
        "pairs": len(pairs), "slots": slots, "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "phases_ms": {key: {p: round(1e3 * med([q.get(p, 0.0) for q in v]), 1) for p in keys} for key, v in phases.items()},
        "create_ms": {key: round(1e3 * med([q.get("thermal_setup", 0.0) for q in v]), 2) for key, v in phases.items()},
        "thermal_iterations": {key: rep.info["iterations"] for key, rep in reports.items()},
        "thermal_solve_seconds": {key: rep.info["seconds"] for key, rep in reports.items()},
        "thermal_rel_residual": {key: rep.info["rel_residual"] for key, rep in reports.items()},
        "kernel_bytes": {
            "stack_box_kernel": 20 * n_vert,
            "stack_locate_kernel_at_least": (24 + 60 + 152) * slots,
            "radix_sort_per_pass": 32 * entries,
            "stack_head_kernel": 12 * entries,
            "stack_compact_kernel_at_most": 12 * entries + 32 * stored,
            "stack_ptr_kernel": 4 * n_vert,
            "stack_diag_kernel_at_most": 12 * n_vert + 8 * stored,
            "stack_merge_count_at_most": 12 * n_vert + 4 * nnz + 4 * stored,
            "stack_merge_fill_at_most": 8 * n_vert + 24 * (nnz + stored),
            "stack_flow_kernel_at_most": 8 * n_vert + 16 * stored + 8 * n_vert + 8 * stored + 16 * len(pairs) * tiles,
            "stack_fold_kernel": 16 * len(pairs) * (tiles + len(meshes)),
        },
        "total_heat_W": {key: rep.total_heat for key, rep in reports.items()},
        "total_loss_W": {key: rep.total_loss for key, rep in reports.items()},
        "hotspots_degC": {key: [round(h[0], 4) if h else None for h in rep.hotspots] for key, rep in reports.items()},
        "interlayer": [{"layers": list(e["layers"]), "flow_W": e["flow"], "area_mm2": e["area"]}
                       for e in reports["stacked"].interlayer],
        "exchange_W": [layer["exchange"] for layer in reports["stacked"].layers],
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""``refine_meshes`` and ``solve_meshed_adaptive`` on one board: what one refinement round and one adaptive run cost.

The board is ``board()`` of ``scripts/load_cases.py`` (four ``Rect`` layers meshed by ``StructuredMesher``, about 1 M
unknowns by default).  One ``solve_meshed_error`` gives the flags (xi_f > 1); the refinement of those flags runs warm,
``--repeats`` times, and the median is reported with the counts of the round (edges, edges marked by the flags and after the
closure, closure sweeps queued, faces and vertices before and after).  Then one adaptive run of ``--rounds`` solves with its
history and the host time of its solves and refinements.  ``min_bytes`` states, from the array sizes, what each kernel of the
refinement must move at least; a kernel trace gives their times.  Prints one JSON object, and writes it to ``--out``.

    python scripts/refine.py [--side 100] [--h 0.2] [--repeats 5] [--rounds 2] [--only refine] [--out FILE]

``--only refine`` runs one warm-up and the refinements alone (a target for ``rocprofv3 --kernel-trace --stats``).
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

TOLERANCE = 0.05
HBM_BYTES_PER_S = 8e12


def min_bytes(n_vert: int, n_tri: int, n_edges: int, n_new: int, n_children: int, key_bytes: int) -> dict:
    """The bytes each kernel of one refinement must move at least, every array read or written once (a sweep: per sweep)."""
    corners = 3 * n_tri
    return {
        "refine_corner_kernel": 12 * n_tri + (key_bytes + 4) * corners,
        # keys and values read and written once per pass of the radix sort; one pass is the floor
        "radix_sort_pairs_per_pass": 2 * (key_bytes + 4) * corners,
        "refine_head_kernel": (key_bytes + 4) * corners + 4 * corners,
        "refine_edge_kernel": (key_bytes + 4 + 4 + 4) * corners + 4 * corners + 16 * n_vert + 16 * n_edges,
        "refine_face_kernel": 4 * corners + 8 * n_edges + n_tri + n_tri + 4 * n_edges,
        "refine_sweep_kernel": 4 * corners + n_tri + 4 * n_edges,
        "refine_count_kernel": 4 * corners + 4 * n_edges + 4 * n_tri,
        "refine_midpoint_kernel": 16 * n_vert + 12 * n_edges + 16 * (n_vert + n_new) + 8 * n_new,
        "refine_emit_kernel": 12 * n_tri + 4 * corners + n_tri + 8 * n_edges + 4 * n_tri + 16 * n_children,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="solves of the adaptive run")
    ap.add_argument("--only", choices=["refine"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=args.h))
    meshes, layer_of = solver.mesh_problem(prob, None, mesher)
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)

    warnings.simplefilter("ignore", solver.SolverWarning)
    _sol, rep = solver.solve_meshed_error(prob, meshes, layer_of, tolerance=TOLERANCE)
    flags = [None] * len(meshes)
    for layer_i in range(len(prob.layers)):
        for mi, xi in zip([mi for mi, l in enumerate(layer_of) if l == layer_i], rep.ratios[layer_i]):
            flags[mi] = xi > 1.0
    refined = solver.refine_meshes(meshes, flags)                  # warm-up: pools
    ms = []
    for _ in range(args.repeats):
        t = time.perf_counter()
        refined = solver.refine_meshes(meshes, flags)
        ms.append(1e3 * (time.perf_counter() - t))
    if args.only == "refine":
        print(json.dumps({"only": "refine", "repeats": args.repeats}))
        return
    n_children = sum(len(m.triangles) for m in refined.meshes)
    floor = min_bytes(n_vert, n_tri, refined.edges, refined.marked, n_children, 4 if n_vert * n_vert <= 2 ** 32 else 8)
    timings: dict = {}
    t = time.perf_counter()
    _sol, last, hist = solver.solve_meshed_adaptive(prob, meshes, layer_of, tolerance=TOLERANCE, max_rounds=args.rounds,
                                                    timings=timings)
    adaptive_s = time.perf_counter() - t
    out = {
        "what": "one refine_meshes of the faces with xi_f > 1, warm, and one solve_meshed_adaptive of the same Problem",
        "n_vertices": n_vert, "n_triangles": n_tri, "unknowns": n_vert + 2 * len(loads) + 2, "tolerance": TOLERANCE,
        "estimate": rep.estimate, "flagged": int(sum(int(f.sum()) for f in flags)),
        "refine_ms": [round(x, 2) for x in ms], "refine_ms_median": round(float(np.median(ms)), 2),
        "edges": refined.edges, "marked_by_flags": refined.marked_by_flags, "marked": refined.marked, "sweeps_queued": refined.sweeps,
        "vertices_after": sum(len(m.points) for m in refined.meshes), "triangles_after": n_children,
        "min_bytes": floor,
        "min_us_at_8TBps": {k: round(1e6 * b / HBM_BYTES_PER_S, 2) for k, b in floor.items()},
        "adaptive": {"rounds": args.rounds, "seconds": round(adaptive_s, 3), "solve_s": round(timings["solve"], 3),
                     "refine_s": round(timings["refine"], 3), "faces": hist.faces, "vertices": hist.vertices,
                     "estimates": hist.estimates, "flagged": hist.flagged, "closure_edges": hist.closure_edges,
                     "reason": hist.reason, "last_block_iterations": int(_sol.solver_info.iterations),
                     "last_estimate": last.estimate},
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

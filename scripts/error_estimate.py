"""``solve_meshed_error`` against ``solve_meshed_currents`` and ``solve_meshed`` on one board: what the error estimate costs on
top of the solve, with and without a tolerance.

The board is ``board()`` of ``scripts/load_cases.py`` (four ``Rect`` layers meshed by ``StructuredMesher``, about 1 M
unknowns by default, a lattice of via resistors, one voltage source, 8 current loads).  The four calls run warm and
alternate, ``--repeats`` times each; medians are reported.  ``phases_ms`` splits each estimate call by host timers: indexing,
assembly, stage 1, stage 2, power (the power densities home), error (the estimator's kernels with G and eta home; the
first call of a plan also builds the vertex -> faces lists) and the Solution and ErrorReport objects.  ``min_bytes`` states,
from the array sizes, what each of the estimator's kernels must move at least; a kernel trace gives their times.  Prints one
JSON object, and writes it to ``--out``.

    python scripts/error_estimate.py [--side 100] [--h 0.2] [--repeats 5] [--only error] [--out FILE]

``--only error`` runs one warm-up and the estimate calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
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


def min_bytes(n_vert: int, n_tri: int) -> dict:
    """The bytes each kernel of the estimator must move at least, every array read or written once."""
    pairs = 3 * n_tri
    return {
        # the (vertex, face) pairs written; a radix sort of 4-byte keys with 4-byte values reads and writes them per pass
        "error_pair_kernel": 12 * n_tri + 8 * pairs,
        "error_ptr_kernel": 4 * pairs + 4 * (n_vert + 1),
        # tri, the corners' xy and V once per vertex, (g, A) out
        "error_face_kernel": 12 * n_tri + 24 * n_vert + 24 * n_tri,
        # the row pointer, the lists, (g, A) once per face, G out
        "error_recover_kernel": 4 * (n_vert + 1) + 4 * pairs + 24 * n_tri + 16 * n_vert,
        # tri, (g, A), G once per vertex, eta out
        "error_indicator_kernel": 12 * n_tri + 24 * n_tri + 16 * n_vert + 8 * n_tri,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["error"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=args.h))
    meshes, layer_of = solver.mesh_problem(prob, None, mesher)
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)

    def error(tolerance, timings=None):
        return solver.solve_meshed_error(prob, meshes, layer_of, tolerance=tolerance, timings=timings)

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sol, rep = error(TOLERANCE)                                   # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "error":
        for _ in range(args.repeats):
            error(None)
        print(json.dumps({"only": "error", "repeats": args.repeats}))
        return
    solver.solve_meshed(prob, meshes, layer_of)
    solver.solve_meshed_currents(prob, meshes, layer_of, [])
    error(None)
    calls = {
        "solve_meshed": lambda tm: solver.solve_meshed(prob, meshes, layer_of),
        "currents": lambda tm: solver.solve_meshed_currents(prob, meshes, layer_of, [], timings=tm),
        "error": lambda tm: error(None, tm),
        "error_tolerance": lambda tm: error(TOLERANCE, tm),
    }
    ms = {key: [] for key in calls}
    phases = {key: [] for key in calls if key != "solve_meshed"}
    for _ in range(args.repeats):
        for key, call in calls.items():
            tm: dict = {}
            t = time.perf_counter()
            call(tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            if key in phases:
                phases[key].append(tm)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    xi = np.concatenate([x for layer in rep.ratios for x in layer])
    floor = min_bytes(n_vert, n_tri)
    out = {
        "what": "solve_meshed_error with and without a tolerance vs solve_meshed_currents (no cuts) and solve_meshed, "
                "same Problem, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "unknowns": n_vert + 2 * len(loads) + 2, "tolerance": TOLERANCE,
        "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "error_minus_currents_ms": round(med(ms["error"]) - med(ms["currents"]), 1),
        "error_over_solve_meshed": round(med(ms["error"]) / med(ms["solve_meshed"]), 2),
        "phases_ms": {k: {key: round(1e3 * med([p[key] for p in v]), 2) for key in sorted(v[0])} for k, v in phases.items()},
        "min_bytes": floor,
        "min_us_at_8TBps": {k: round(1e6 * b / HBM_BYTES_PER_S, 2) for k, b in floor.items()},
        "block_iterations": int(sol.solver_info.iterations),
        "residual_norm": float(sol.solver_info.residual_norm),
        "estimate": rep.estimate, "power_error_W": rep.power_error,
        "layers_E_P_W": [[float(E), float(P)] for E, P in rep.layers],
        "worst_eta": [round(w[0], 6) if w else None for w in rep.worst],
        "faces_to_refine": int((xi > 1).sum()), "largest_ratio": float(xi.max()),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

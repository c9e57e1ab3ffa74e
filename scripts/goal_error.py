"""``solve_meshed_goal_error`` against ``solve_meshed_sensitivities`` and ``solve_meshed_error`` on one board: what the
goal-oriented estimate of k voltage drops costs on top of their sensitivities' block solve and of the energy estimate.

The board is ``board()`` of ``scripts/load_cases.py`` (four ``Rect`` layers meshed by ``StructuredMesher``, about 1 M
unknowns by default, a lattice of via resistors, one voltage source, 8 current loads); the objectives are the drops
across the first k loads, k = 1 and 8.  The calls run warm and alternate, ``--repeats`` times each; medians are reported.
``phases_ms`` splits each call by host timers (``goal``: the adjoint weights, the estimator's kernels and its results
home).  ``min_bytes`` states, from the array sizes, what each pass of the estimator must move at least for each k; a kernel
trace gives their times.  Prints one JSON object, and writes it to ``--out`` (default ``profiles/goal_error.json``).

    python scripts/goal_error.py [--side 100] [--h 0.2] [--repeats 5] [--only goal] [--out FILE]

``--only goal`` runs one warm-up and the k = 8 goal calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
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
CHUNK = 8                                       # objectives per launch (kGoalChunk of csrc/goal.hip)


def min_bytes(n_vert: int, n_tri: int, n_cols: int, n_obj: int) -> dict:
    """The bytes each pass of the estimator must move at least over all its launches, every array read or written once."""
    out = {"goal_face_kernel": 0, "goal_recover_kernel": 0, "goal_indicator_kernel": 0}
    for j0 in range(0, n_obj, CHUNK):
        q = min(CHUNK, n_obj - j0)
        f = 1 + q
        planes = (16 * f + 8) * n_tri                          # g of every field and the area
        power = 8 * n_tri if j0 == 0 else 0
        eta0 = 8 * n_tri if j0 == 0 else 0
        # tri, the corners' xy once per vertex, every row of V once, g and A out, the power
        out["goal_face_kernel"] += 12 * n_tri + 16 * n_vert + 8 * n_cols * n_vert + planes + power
        # the row pointer, the lists, g and A once per face, G of every field out
        out["goal_recover_kernel"] += 4 * (n_vert + 1) + 12 * n_tri + planes + 16 * f * n_vert
        # tri, g and A, G once per vertex, eta of field 0, and eta, delta and omega of every objective out
        out["goal_indicator_kernel"] += 12 * n_tri + planes + 16 * f * n_vert + eta0 + 24 * q * n_tri
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["goal"], default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "goal_error.json"))
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=args.h))
    meshes, layer_of = solver.mesh_problem(prob, None, mesher)
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)
    objectives = {k: [(load.f, load.t) for load in loads[:k]] for k in (1, 8)}

    def goal(k, timings=None):
        return solver.solve_meshed_goal_error(prob, meshes, layer_of, objectives[k], timings=timings)

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sol, rep, goals = goal(8)                                     # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "goal":
        for _ in range(args.repeats):
            goal(8)
        print(json.dumps({"only": "goal", "repeats": args.repeats}))
        return
    calls = {"error": lambda tm: solver.solve_meshed_error(prob, meshes, layer_of, timings=tm)}
    for k in (1, 8):
        calls[f"sensitivities_k{k}"] = lambda tm, k=k: solver.solve_meshed_sensitivities(prob, meshes, layer_of, objectives[k],
                                                                                        timings=tm)
        calls[f"goal_k{k}"] = lambda tm, k=k: goal(k, tm)
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
    floors = {f"k{k}": min_bytes(n_vert, n_tri, solver.sensitivity_block_columns(k, 0), k) for k in (1, 8)}
    out = {
        "what": "solve_meshed_goal_error for 1 and 8 drops vs solve_meshed_sensitivities of the same drops and "
                "solve_meshed_error, same Problem, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "unknowns": n_vert + 2 * len(loads) + 2,
        "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        **{f"goal_minus_sensitivities_k{k}_ms": round(med(ms[f"goal_k{k}"]) - med(ms[f"sensitivities_k{k}"]), 1) for k in (1, 8)},
        "phases_ms": {k: {key: round(1e3 * med([p[key] for p in v]), 2) for key in sorted(v[0])} for k, v in phases.items()},
        "min_bytes": floors,
        "min_us_at_8TBps": {k: {name: round(1e6 * b / HBM_BYTES_PER_S, 2) for name, b in v.items()} for k, v in floors.items()},
        "block_iterations": int(sol.solver_info.iterations),
        "residual_norm": float(sol.solver_info.residual_norm),
        "estimate": rep.estimate,
        "drops_V": [g.value for g in goals], "bounds_V": [g.bound for g in goals], "corrections_V": [g.correction for g in goals],
    }
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""``solve_meshed_sensitivities`` against ``solve_meshed`` on one board: what the sensitivities of k = 1 and k = 8 voltage
drops cost on top of the solve.

The board is ``board()`` of ``scripts/load_cases.py`` (four ``Rect`` layers meshed by ``StructuredMesher``, about 1 M
unknowns by default, a lattice of via resistors, one voltage source, 8 current loads).  The objectives are the drops across
the loads: k = 1 the first load, k = 8 every load.  The three calls run warm and alternate, ``--repeats`` times each;
medians are reported.  ``phases_ms`` splits each sensitivity call by host timers: indexing (the connections snapped),
assembly (L on the device and the block's triples), stage 1 (the reduction, the triples up, the block solve), stage 2 (V
down with the residuals), sensitivity (the adjoint weights on the host and the face kernel with its results home) and the
Solution and Sensitivity objects.  Prints one JSON object, and writes it to ``--out``.

    python scripts/sensitivity.py [--side 100] [--h 0.2] [--repeats 5] [--only sens] [--out FILE]

``--only sens`` runs one warm-up and the k = 8 calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["sens"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    objectives = {1: [(loads[0].f, loads[0].t)], 8: [(load.f, load.t) for load in loads]}
    mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=args.h))
    meshes, layer_of = solver.mesh_problem(prob, None, mesher)
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)

    def sens(k, timings=None):
        return solver.solve_meshed_sensitivities(prob, meshes, layer_of, objectives[k], timings=timings)

    def plain():
        return solver.solve_meshed(prob, meshes, layer_of)

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sol8, s8 = sens(8)                                           # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "sens":
        for _ in range(args.repeats):
            sens(8)
        print(json.dumps({"only": "sens", "k": 8, "repeats": args.repeats}))
        return
    ref = plain()
    sens(1)
    worst = max(np.abs(a.values - b.values).max() / max(np.abs(b.values).max(), 1e-300)
                for la, lb in zip(sol8.layer_solutions, ref.layer_solutions) for a, b in zip(la.potentials, lb.potentials))
    ms = {"solve_meshed": [], "k1": [], "k8": []}
    phases = {"k1": [], "k8": []}
    for _ in range(args.repeats):
        t = time.perf_counter()
        plain()
        ms["solve_meshed"].append(1e3 * (time.perf_counter() - t))
        for k in (1, 8):
            tm: dict = {}
            t = time.perf_counter()
            sens(k, tm)
            ms[f"k{k}"].append(1e3 * (time.perf_counter() - t))
            phases[f"k{k}"].append(tm)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    keys = ("indexing", "assembly", "stage1", "stage2", "sensitivity", "solutions")
    out = {
        "what": "solve_meshed_sensitivities with k = 1 and k = 8 load drops vs solve_meshed, same Problem, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "unknowns": n_vert + 2 * len(loads) + 2,
        "block_columns": {"k1": 2, "k8": 9}, "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "k1_over_solve_meshed": round(med(ms["k1"]) / med(ms["solve_meshed"]), 2),
        "k8_over_solve_meshed": round(med(ms["k8"]) / med(ms["solve_meshed"]), 2),
        "phases_ms": {k: {key: round(1e3 * med([p[key] for p in v]), 1) for key in keys} for k, v in phases.items()},
        "block_iterations": int(sol8.solver_info.iterations),
        "residual_norm": float(sol8.solver_info.residual_norm),
        "max_rel_potential_difference_vs_solve_meshed": float(worst),
        "drops_V": [round(s.value, 6) for s in s8],
    }
    text = json.dumps(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""``solve_meshed_currents`` against ``solve_meshed`` on one board: what the current report costs on top of the solve, with
no cut and with 64 cuts.

The board is ``board()`` of ``scripts/load_cases.py`` (four ``Rect`` layers meshed by ``StructuredMesher``, about 1 M
unknowns by default, a lattice of via resistors, one voltage source, 8 current loads).  The 64 cuts are lines across each
layer, 16 per layer: 8 vertical and 8 horizontal ones that start and end outside the copper.  The three calls run warm and
alternate, ``--repeats`` times each; medians are reported.  ``phases_ms`` splits each current call by host timers: indexing
(the connections snapped), assembly (L on the device and the block's triples), stage 1 (the reduction, the triples up, the
block solve), stage 2 (V down with the residuals), currents (the dissipation and current kernels with their results home,
the cut/tile pairs listed) and the Solution and CurrentReport objects.  Prints one JSON object, and writes it to ``--out``.

    python scripts/currents.py [--side 100] [--h 0.2] [--repeats 5] [--only currents] [--out FILE]

``--only currents`` runs one warm-up and the 64-cut calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
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


def line_cuts(prob, side: float, per_layer: int = 16) -> list:
    """Lines across each layer: half vertical (upward), half horizontal (leftward), from 1 mm outside the board to 1 mm
    outside its other edge, at positions that avoid the mesh's vertex columns."""
    out = []
    half = per_layer // 2
    for layer in prob.layers:
        for q in range(half):
            at = side * (q + 0.5) / half + 0.0123
            out.append(solver.Cut(layer, (at, -1.0), (at, side + 1.0)))
            out.append(solver.Cut(layer, (side + 1.0, at), (-1.0, at)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["currents"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    cuts = {0: [], 64: line_cuts(prob, args.side)}
    mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=args.h))
    meshes, layer_of = solver.mesh_problem(prob, None, mesher)
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)

    def currents(k, timings=None):
        return solver.solve_meshed_currents(prob, meshes, layer_of, cuts[k], timings=timings)

    def plain():
        return solver.solve_meshed(prob, meshes, layer_of)

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sol64, rep64 = currents(64)                                  # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "currents":
        for _ in range(args.repeats):
            currents(64)
        print(json.dumps({"only": "currents", "cuts": 64, "repeats": args.repeats}))
        return
    ref = plain()
    currents(0)
    worst = max(np.abs(a.values - b.values).max() / max(np.abs(b.values).max(), 1e-300)
                for la, lb in zip(sol64.layer_solutions, ref.layer_solutions) for a, b in zip(la.potentials, lb.potentials))
    ms = {"solve_meshed": [], "cuts0": [], "cuts64": []}
    phases = {"cuts0": [], "cuts64": []}
    for _ in range(args.repeats):
        t = time.perf_counter()
        plain()
        ms["solve_meshed"].append(1e3 * (time.perf_counter() - t))
        for k in (0, 64):
            tm: dict = {}
            t = time.perf_counter()
            currents(k, tm)
            ms[f"cuts{k}"].append(1e3 * (time.perf_counter() - t))
            phases[f"cuts{k}"].append(tm)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    keys = ("indexing", "assembly", "stage1", "stage2", "currents", "solutions")
    total_load = sum(load.current for load in loads)
    powers = [d[k] for d in rep64.elements.values() for k in ("power", "input_power") if k in d]
    out = {
        "what": "solve_meshed_currents with 0 and 64 cuts vs solve_meshed, same Problem, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "unknowns": n_vert + 2 * len(loads) + 2, "cuts": 64,
        "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "cuts0_over_solve_meshed": round(med(ms["cuts0"]) / med(ms["solve_meshed"]), 2),
        "cuts64_over_solve_meshed": round(med(ms["cuts64"]) / med(ms["solve_meshed"]), 2),
        "phases_ms": {k: {key: round(1e3 * med([p[key] for p in v]), 1) for key in keys} for k, v in phases.items()},
        "block_iterations": int(sol64.solver_info.iterations),
        "residual_norm": float(sol64.solver_info.residual_norm),
        "max_rel_potential_difference_vs_solve_meshed": float(worst),
        "load_current_A": total_load,
        "layer_power_W": [round(p, 6) for p in rep64.layers],
        "power_balance_W": float(sum(powers) + sum(rep64.layers)),
        "hotspots_A_per_mm": [round(h[0], 4) if h else None for h in rep64.hotspots],
        "cuts_A_first_layer": [round(c, 6) for c in rep64.cuts[:16]],
    }
    text = json.dumps(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

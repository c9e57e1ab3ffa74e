"""``solve_meshed_load_case_currents`` on k load cases of one board: with and without the per-case fields, next to one
``solve_meshed_currents`` per case and next to ``solve_meshed_load_cases`` (potentials and power densities only).

The board and the k = 8 cases are those of ``scripts/load_cases.py`` (four ``Rect`` layers meshed by ``StructuredMesher``,
about 1 M unknowns by default; each load alone, then all together); the 64 cuts are the lines of ``scripts/currents.py``.
The four calls run warm and alternate, ``--repeats`` times each; medians are reported.  ``phases_ms`` splits the two new
calls by host timers: indexing, assembly, stage 1 (the block solve), stage 2 (V down), currents (the power densities of the
Solutions, then the face and cut kernels over all columns with their results home) and the Python objects.

``kernel_bytes`` states what the two new kernels must move, from the counts alone (nothing measured): per face the face
kernel gathers 3 corners x (16 B of xy + 8k B of V) besides 12 B of corner indices, and writes 12 B (the envelope |J| and
its case) with the envelope only, or 24k + 12 B with the per-case J and |J|; the cut kernel gathers the same per face of
every tile a cut's segment meets and writes 8k B per (cut, tile) pair.  Prints one JSON object, and writes it to ``--out``.

    python scripts/load_case_currents.py [--side 100] [--h 0.2] [--repeats 3] [--only envelope] [--out FILE]

``--only envelope`` runs one warm-up and the envelope-only calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
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

from currents import line_cuts  # noqa: E402
from load_cases import board  # noqa: E402
from padne_amd import mesh, solver  # noqa: E402
from padne_amd.structured import StructuredMesher  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["envelope"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    cases = [{other: 0.0 for other in loads if other is not load} for load in loads[1:]] + [{}]
    k = len(cases)
    cuts = line_cuts(prob, args.side)
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)
    substituted = [solver.substitute_load_case(prob, c)[0] for c in solver.check_load_cases(prob, cases)]

    def block(fields, timings=None):
        return solver.solve_meshed_load_case_currents(prob, meshes, layer_of, cases, cuts, per_case_fields=fields,
                                                      timings=timings)

    def loop():
        return [solver.solve_meshed_currents(p, meshes, layer_of, cuts) for p in substituted]

    def potentials_only():
        return solver.solve_meshed_load_cases(prob, meshes, layer_of, cases)

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sols, reps, env = block(True)                                # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "envelope":
        for _ in range(args.repeats):
            block(False)
        print(json.dumps({"only": "envelope", "cases": k, "cuts": len(cuts), "repeats": args.repeats}))
        return
    separate = loop()
    potentials_only()
    block(False)
    worst = max(np.abs(a.values - b.values).max() / max(np.abs(b.values).max(), 1e-300)
                for rep, (_, ref) in zip(reps, separate) for fa, fb in zip(rep.magnitudes, ref.magnitudes)
                for a, b in zip(fa, fb))
    ms = {"fields": [], "envelope_only": [], "currents_loop": [], "load_cases": []}
    phases = {"fields": [], "envelope_only": []}
    for _ in range(args.repeats):
        for key, fields in (("fields", True), ("envelope_only", False)):
            tm: dict = {}
            t = time.perf_counter()
            block(fields, tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            phases[key].append(tm)
        t = time.perf_counter()
        loop()
        ms["currents_loop"].append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        potentials_only()
        ms["load_cases"].append(1e3 * (time.perf_counter() - t))
    med = lambda xs: float(np.median(xs))  # noqa: E731
    keys = ("indexing", "assembly", "stage1", "stage2", "currents", "solutions")
    gathered = n_tri * (12 + 3 * (16 + 8 * k))
    out = {
        "what": "solve_meshed_load_case_currents (fields / envelope only) vs one solve_meshed_currents per case and vs "
                "solve_meshed_load_cases, same board, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "unknowns": n_vert + 2 * len(loads) + 2, "cases": k, "cuts": len(cuts),
        "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "currents_loop_over_fields": round(med(ms["currents_loop"]) / med(ms["fields"]), 2),
        "currents_loop_over_envelope_only": round(med(ms["currents_loop"]) / med(ms["envelope_only"]), 2),
        "phases_ms": {key: {p: round(1e3 * med([q[p] for q in v]), 1) for p in keys} for key, v in phases.items()},
        "kernel_bytes": {
            "face_kernel_gathered": gathered,
            "face_kernel_written_envelope_only": n_tri * 12,
            "face_kernel_written_with_fields": n_tri * (24 * k + 12),
            "cut_kernel_gathered_per_tile_of_256_faces": 256 * (12 + 3 * (16 + 8 * k)),
            "cut_kernel_written_per_pair": 8 * k,
            "home_envelope_only": n_tri * 12,
            "home_with_fields": n_tri * (24 * k + 12),
        },
        "block_iterations": int(sols[0].solver_info.iterations),
        "max_rel_magnitude_difference_vs_separate_calls": float(worst),
        "envelope_hotspots_A_per_mm": [[round(h[0], 4), h[1]] if h else None for h in env.hotspots],
        "envelope_layer_power_W": [[round(p, 6), c] for p, c in env.layers],
        "envelope_cuts_A_first_layer": [[round(v, 6), c] for v, c in env.cuts[:16]],
        "faces_by_worst_case": np.bincount(np.concatenate([c for cs in env.cases for c in cs]), minlength=k).tolist(),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""``solve_meshed_load_cases`` on k load cases of one board against k ``solve_meshed`` calls on the same Problems.

The board is a Problem on four ``Rect`` layers of ``--side`` x ``--side`` mm meshed by ``StructuredMesher`` (``--h`` mm
between vertices: about 1 M unknowns by default), the layers tied by a lattice of via resistors, one voltage source
between the top and the bottom layer and 8 current loads spread over the top layer.  The k = 8 cases are each load alone
at its own current, then all loads together (the first case is dropped so that there are 8: load 0 alone is covered by
"all").  Both forms run warm and alternate, ``--repeats`` times each.  ``block_phases_ms`` splits the block call by host
timers: indexing (the connections snapped), assembly (L on the device and the r stamps of the cases), stage 1 (the
reduction, the triples up, the block solve), stage 2 (V down with the residuals), power density (every case's, from the
V the device holds) and the Solutions.  Prints one JSON object, and writes it to ``--out``.

    python scripts/load_cases.py [--side 100] [--h 0.2] [--repeats 3] [--only block] [--out FILE]

``--only block`` runs one warm-up and the block calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from padne_amd import mesh, problem, solver  # noqa: E402
from padne_amd.structured import Rect, Shapes, StructuredMesher  # noqa: E402

N_LOADS = 8


def board(side: float, via_pitch: float):
    """(problem, loads, source): 4 layers of 35 um copper, vias on a lattice, 1 V source, 8 loads on the top layer."""
    sigma = 5.8e4 * 0.035                                        # S/mm * mm
    layers = [problem.Layer(shape=Shapes.of(Rect(0.0, 0.0, side, side)), name=f"L{i}", conductance=sigma) for i in range(4)]
    networks = []
    # vias: 1 mOhm between neighbouring layers on a lattice (off the mesh points, so that snapping has work to do)
    for i in range(3):
        for x in np.arange(via_pitch / 2, side, via_pitch):
            for y in np.arange(via_pitch / 2, side, via_pitch):
                a = problem.Connection(layer=layers[i], point=mesh.Point(float(x) + 0.013, float(y) + 0.017))
                b = problem.Connection(layer=layers[i + 1], point=mesh.Point(float(x) + 0.013, float(y) + 0.017))
                networks.append(problem.Network(connections=[a, b], elements=[problem.Resistor(a=a.node_id, b=b.node_id,
                                                                                              resistance=1e-3)]))
    p = problem.Connection(layer=layers[0], point=mesh.Point(0.05 * side, 0.05 * side))
    n = problem.Connection(layer=layers[3], point=mesh.Point(0.05 * side, 0.05 * side))
    source = problem.VoltageSource(p=p.node_id, n=n.node_id, voltage=1.0)
    networks.append(problem.Network(connections=[p, n], elements=[source]))
    loads = []
    rng = np.random.default_rng(7)
    for q in range(N_LOADS):
        x, y = rng.uniform(0.3 * side, 0.95 * side, size=2)
        f = problem.Connection(layer=layers[0], point=mesh.Point(float(x), float(y)))
        t = problem.Connection(layer=layers[3], point=mesh.Point(float(x), float(y)))
        load = problem.CurrentSource(f=f.node_id, t=t.node_id, current=0.5 + 0.25 * q)
        loads.append(load)
        networks.append(problem.Network(connections=[f, t], elements=[load]))
    return problem.Problem(layers=layers, networks=networks), loads, source


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["block"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    cases = [{other: 0.0 for other in loads if other is not load} for load in loads[1:]] + [{}]
    k = len(cases)
    mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=args.h))
    t = time.perf_counter()
    meshes, layer_of = solver.mesh_problem(prob, None, mesher)
    mesh_s = time.perf_counter() - t
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)
    substituted = [solver.substitute_load_case(prob, c)[0] for c in solver.check_load_cases(prob, cases)]

    def block(timings=None):
        return solver.solve_meshed_load_cases(prob, meshes, layer_of, cases, timings=timings)

    def loop():
        return [solver.solve_meshed(p, meshes, layer_of) for p in substituted]

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sols = block()                                               # warm-up: library, context, pools
    first_block_s = time.perf_counter() - t
    if args.only == "block":
        for _ in range(args.repeats):
            block()
        print(json.dumps({"only": "block", "k": k, "repeats": args.repeats}))
        return
    ref = loop()
    worst = max(np.abs(a.values - b.values).max() / max(np.abs(b.values).max(), 1e-300)
                for s, r in zip(sols, ref) for la, lb in zip(s.layer_solutions, r.layer_solutions)
                for a, b in zip(la.potentials, lb.potentials))
    block_ms, loop_ms, phases = [], [], []
    for _ in range(args.repeats):
        tm: dict = {}
        t = time.perf_counter()
        block(tm)
        block_ms.append(1e3 * (time.perf_counter() - t))
        phases.append(tm)
        t = time.perf_counter()
        loop()
        loop_ms.append(1e3 * (time.perf_counter() - t))
    med = lambda xs: float(np.median(xs))  # noqa: E731
    out = {
        "what": "solve_meshed_load_cases (one block) vs one solve_meshed per case, same Problems, warm",
        "k": k, "n_vertices": n_vert, "n_triangles": n_tri, "unknowns": n_vert + 2 * len(loads) + 2,
        "mesh_s": round(mesh_s, 3), "first_block_call_s": round(first_block_s, 3),
        "block_ms": [round(x, 1) for x in block_ms], "loop_ms": [round(x, 1) for x in loop_ms],
        "block_ms_median": round(med(block_ms), 1), "loop_ms_median": round(med(loop_ms), 1),
        "speedup": round(med(loop_ms) / med(block_ms), 2),
        "block_phases_ms": {key: round(1e3 * med([p[key] for p in phases]), 1)
                            for key in ("indexing", "assembly", "stage1", "stage2", "power_density", "solutions")},
        "block_iterations": int(sols[0].solver_info.iterations),
        "max_residual_norm": float(max(s.solver_info.residual_norm for s in sols)),
        "max_rel_potential_difference_vs_loop": float(worst),
    }
    text = json.dumps(out)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

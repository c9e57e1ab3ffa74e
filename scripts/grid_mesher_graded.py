"""The graded grid mesher on the four outlines of ``scripts/grid_mesher.py``: what grading costs and what it saves.

One process, warm, ``--repeats`` calls each, medians -- as ``profiles/r28_grid_mesher.json`` took them.  For the uniform call
(``padne_polymesh_create``), the graded call with the default ramp of ``Mesher.Config`` (factor 3, 0.5 to 3.0: one level) and
with factor 8: ms of the device call alone (create and destroy, nothing fetched), the vertices and faces out, the cells per
level.  ``min_bytes`` states, from the array sizes, what the stages the graded call adds must move at least, every array read
or written once; no kernel trace is taken here, so their times are known only together, as the difference of the calls.  Then
a two-layer board (an L-shaped pour with an antipad over a rectangle, ``--board-scale`` times the one of
tests/test_gridmesh.py, a current source across the L) meshed both ways at ``--maximum-size``: ms of ``mesh_problem`` and of
``solve_meshed``, the unknowns and the drop between the terminals.  Prints one JSON object, and writes it to ``--out``.

    python scripts/grid_mesher_graded.py [--side 100] [--h 0.2] [--repeats 30] [--out profiles/r29_graded_mesher.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from grid_mesher import HBM_BYTES_PER_S, outlines, sizes  # noqa: E402
from padne_amd import GridMesher, Polygon, _hip, gridmesh, mesh, problem, solver, structured  # noqa: E402


def create_alone(ctx, polygons, h, thresholds, repeats):
    """ms of every call (create + destroy), and the counts of the last: thresholds None is the uniform entry."""
    rings = [np.ascontiguousarray(r, dtype=np.float64) for poly in polygons for r in poly]
    prp = np.concatenate([[0], np.cumsum([len(p) for p in polygons])]).astype(np.int64)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    xy = np.ascontiguousarray(np.concatenate(rings))
    nv, nt = np.zeros(len(polygons), dtype=np.int64), np.zeros(len(polygons), dtype=np.int64)
    t = np.ascontiguousarray(thresholds if thresholds is not None else [0], dtype=np.int32)
    cells = np.zeros((len(polygons), len(t)), dtype=np.int64)
    head = (ctx._h, len(polygons), _hip._ptr(prp, _hip._PI64), _hip._ptr(rp, _hip._PI64), _hip._ptr(xy, _hip._PF64), h, 0.25)
    tail = (_hip._ptr(nv, _hip._PI64), _hip._ptr(nt, _hip._PI64))
    ms = []
    for _ in range(repeats + 1):                                     # (the first call warms the pools and is dropped)
        handle = C.c_void_p()
        t0 = time.perf_counter()
        if thresholds is None:
            rc = ctx._lib.padne_polymesh_create(*head, *tail, C.byref(handle))
        else:
            rc = ctx._lib.padne_polymesh_create_graded(*head, len(t), _hip._ptr(t, _hip._PI32), 0, None, *tail,
                                                       _hip._ptr(cells, _hip._PI64), C.byref(handle))
        _hip._check(rc)
        ms.append(1e3 * (time.perf_counter() - t0))
        ctx._lib.padne_polymesh_destroy(handle)
    ms = ms[1:]
    return {"thresholds": None if thresholds is None else [int(x) for x in t], "create_ms": [round(x, 3) for x in ms],
            "create_ms_median": round(float(np.median(ms)), 3), "vertices": int(nv.sum()), "faces": int(nt.sum()),
            "cells_per_level": None if thresholds is None else cells.sum(axis=0).tolist()}


def added_min_bytes(L: int, n_level: int) -> dict:
    """What the stages of the graded call must move at least beyond the uniform call's, every array read or written once:
    state and plain and ok and level one byte per lattice vertex, the two distances four."""
    out = {
        "polymesh_plain_kernel": L + L,
        "polymesh_rowdist_kernel": L + 4 * L,
        "polymesh_coldist_kernel": 4 * L + 4 * L,
        "fill_of_ok": L,
        "polymesh_level_kernel": L + L,
        "level_read_by_count_and_face": 2 * L,
    }
    for l in range(1, n_level):
        out[f"polymesh_blockmin_kernel<{l}>"] = (16 + 4 + 1) * (L // 4 ** l)
    return out


def pour_board(k: float):
    pour = Polygon([(x * k + 0.11, y * k + 0.23) for x, y in ((0, 0), (6, 0), (6, 1.7), (1.7, 1.7), (1.7, 4), (0, 4))],
                   holes=[[(k * (1.0 + 0.4 * math.cos(a)), k * (1.1 + 0.4 * math.sin(a))) for a in 2 * np.pi * np.arange(24) / 24]])
    top = problem.Layer(shape=structured.Shapes.of(pour), name="F.Cu", conductance=2.0)
    bottom = problem.Layer(shape=structured.Shapes.of(structured.Rect(0.3 * k, 0.4 * k, 5.7 * k, 1.6 * k)), name="B.Cu", conductance=1.5)

    def P(x, y):
        return mesh.Point(x * k, y * k)
    a, b = problem.Connection(layer=top, point=P(5.8, 0.9)), problem.Connection(layer=top, point=P(0.9, 3.9))
    c, d = problem.Connection(layer=top, point=P(3.0, 1.0)), problem.Connection(layer=bottom, point=P(3.0, 1.0))
    e, f = problem.Connection(layer=bottom, point=P(0.6, 0.8)), problem.Connection(layer=top, point=P(0.6, 0.8))
    nets = [problem.Network(connections=[a, b], elements=[problem.CurrentSource(f=b.node_id, t=a.node_id, current=1.0)]),
            problem.Network(connections=[c, d], elements=[problem.Resistor(a=c.node_id, b=d.node_id, resistance=0.01)]),
            problem.Network(connections=[e, f], elements=[problem.Resistor(a=e.node_id, b=f.node_id, resistance=0.02)])]
    return problem.Problem(layers=[top, bottom], networks=nets)


def board_both_ways(prob, cfg, repeats):
    out = {}
    for name, mesher in (("uniform", GridMesher(cfg)), ("graded", GridMesher(cfg, graded=True))):
        mesh_ms, solve_ms = [], []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", solver.SolverWarning)
            for _ in range(repeats + 1):
                t0 = time.perf_counter()
                meshes, layer_of = solver.mesh_problem(prob, mesher=mesher)
                t1 = time.perf_counter()
                sol = solver.solve_meshed(prob, meshes, layer_of)
                t2 = time.perf_counter()
                mesh_ms.append(1e3 * (t1 - t0))
                solve_ms.append(1e3 * (t2 - t1))
        v = np.concatenate([zf.values for ls in sol.layer_solutions for zf in ls.potentials])
        out[name] = {"thresholds": mesher.thresholds(), "vertices": [len(m.points) for m in meshes],
                     "faces": [len(m.triangles) for m in meshes],
                     "mesh_problem_ms_median": round(float(np.median(mesh_ms[1:])), 2),
                     "solve_meshed_ms": [round(x, 2) for x in solve_ms[1:]],
                     "solve_meshed_ms_median": round(float(np.median(solve_ms[1:])), 2),
                     "iterations": int(sol.solver_info.iterations), "residual_norm": float(sol.solver_info.residual_norm),
                     "drop": float(np.ptp(v))}
    out["drop_relative_difference"] = abs(out["graded"]["drop"] - out["uniform"]["drop"]) / out["uniform"]["drop"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square outlines in mm")
    ap.add_argument("--h", type=float, default=0.2, help="lattice spacing in mm")
    ap.add_argument("--antipad-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--board-scale", type=float, default=25.0)
    ap.add_argument("--maximum-size", type=float, default=0.3)
    ap.add_argument("--board-repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    polygons = outlines(args.side, args.antipad_pitch)
    ctx = solver.get_context()
    z = sizes(polygons, args.h)
    ramps = {"default_ramp": gridmesh.graded_thresholds(args.h, 3.0, 0.5, 3.0),
             "factor_8": gridmesh.graded_thresholds(args.h, 8.0, 0.5, 3.0)}
    calls = {"uniform": create_alone(ctx, polygons, args.h, None, args.repeats)}
    for name, t in ramps.items():
        calls[name] = create_alone(ctx, polygons, args.h, t, args.repeats)
        floor = added_min_bytes(z["lattice_vertices"], len(t))
        calls[name]["added_min_bytes"] = floor
        calls[name]["added_min_bytes_total"] = int(sum(floor.values()))
        calls[name]["added_min_us_at_8TBps"] = round(1e6 * sum(floor.values()) / HBM_BYTES_PER_S, 2)
        calls[name]["added_ms_median"] = round(calls[name]["create_ms_median"] - calls["uniform"]["create_ms_median"], 3)
    calls["uniform_again"] = create_alone(ctx, polygons, args.h, None, args.repeats)       # (drift over the run)
    board = board_both_ways(pour_board(args.board_scale), mesh.Mesher.Config(maximum_size=args.maximum_size), args.board_repeats)
    out = {
        "what": "padne_polymesh_create against padne_polymesh_create_graded on four board outlines, warm, the device call "
                "alone; a two-layer board meshed both ways through mesh_problem and solve_meshed; no kernel trace taken",
        "side": args.side, "h": args.h, "repeats": args.repeats, **z, "calls": calls,
        "board": {"scale": args.board_scale, "maximum_size": args.maximum_size, "repeats": args.board_repeats, **board},
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""The connectivity pre-pass on a synthetic board: what the device call costs next to the host around it and to the restatement.

The board: ``--layers`` layers (4); on each a ``--side`` mm plane (100) with antipads on a ``--antipad-pitch`` grid (5 mm: 361
of them, 16-gons), and beside it ``--pads`` undriven 1 mm pads (10 000) on a 2 mm grid.  ``--connections`` connections per
layer (2 000), as two-terminal resistor networks from layer k to layer k + 1 (cyclic): most join the planes, ``--dead`` per
layer join two pads (dead copper: the network is dropped), ``--unplaced`` per layer end in empty space; a voltage source
across the plane of layer 0 drives the board.

One process, warm, medians.  Times: ``_hip.locate_polygons`` (the rings flattened in Python, the call, the fetch), the device
locate call alone (``padne_polygons_locate`` + ``_destroy`` on arrays flattened once), ``solver.compute_connectivity`` (rings and points gathered in Python, the call, the graph),
``solver.prepare_board`` with ``GridMesher(graded=True)`` at ``--maximum-size``, and the vectorised restatement
(``tests/connectivity_ref.locate_by_layer``) on the same host; the device's result is compared with the restatement's.
``must_read_bytes`` states, from the shapes, what the locate kernel must read in each of its two passes: 32 B of box per
(query, polygon of its group) and 32 B per segment of every candidate (a polygon whose box holds the query).  No kernel
trace is taken here: the kernels' own times are not measured, only the call's.  Prints one JSON object, and writes it to ``--out``.

    python scripts/connectivity.py [--repeats 30] [--out profiles/r30_connectivity.json]
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
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import connectivity_ref as R  # noqa: E402
from grid_mesher import HBM_BYTES_PER_S, ngon  # noqa: E402
from padne_amd import GridMesher, Polygon, _hip, gridmesh, mesh, problem, solver, structured  # noqa: E402


def board(args):
    rng = np.random.default_rng(30)
    s, o, pitch = args.side, 0.037, args.antipad_pitch
    n = max(1, int(s / pitch) - 1)
    per_row = int(np.ceil(np.sqrt(args.pads)))
    layers = []
    for k in range(args.layers):
        plane = Polygon([(o, o), (s - o, o), (s - o, s - o), (o, s - o)],
                        holes=[ngon(16, 0.4, (i + 1) * pitch + o, (j + 1) * pitch + o) for j in range(n) for i in range(n)])
        pads = [structured.Rect(s + 10.0 + 2.0 * (p % per_row), 2.0 * (p // per_row), s + 11.0 + 2.0 * (p % per_row), 2.0 * (p // per_row) + 1.0)
                for p in range(args.pads)]
        layers.append(problem.Layer(shape=structured.Shapes.of(plane, *pads), name=f"L{k}", conductance=2.0))

    def on_plane():             # between the antipads: at least 1.1 mm from every antipad centre
        i, j = rng.integers(0, n, 2)
        return mesh.Point((i + 1.5) * pitch + o + rng.uniform(-1.0, 1.0), (j + 1.5) * pitch + o + rng.uniform(-1.0, 1.0)) \
            if i + 1 < n and j + 1 < n else mesh.Point(0.5 * pitch + rng.uniform(-1.0, 1.0), 0.5 * pitch + rng.uniform(-1.0, 1.0))

    def on_pad():
        p = int(rng.integers(0, args.pads))
        return mesh.Point(s + 10.5 + 2.0 * (p % per_row), 2.0 * (p // per_row) + 0.5)

    def nowhere():
        return mesh.Point(rng.uniform(-50.0, -10.0), rng.uniform(0.0, s))

    a, b = problem.Connection(layer=layers[0], point=mesh.Point(2.5, 2.5)), problem.Connection(layer=layers[0], point=mesh.Point(s - 2.5, s - 2.5))
    nets = [problem.Network(connections=[a, b], elements=[problem.VoltageSource(p=a.node_id, n=b.node_id, voltage=1.0)])]
    per_layer = args.connections // 2
    for k in range(args.layers):
        up = layers[(k + 1) % args.layers]
        for m in range(per_layer):
            if m < args.dead:
                ends = (on_pad(), on_pad())
            elif m < args.dead + args.unplaced:
                ends = (on_plane(), None)
            else:
                ends = (on_plane(), on_plane())
            c = problem.Connection(layer=layers[k], point=ends[0])
            d = problem.Connection(layer=up, point=ends[1]) if ends[1] is not None else problem.Connection(layer=up, point=nowhere())
            nets.append(problem.Network(connections=[c, d], elements=[problem.Resistor(a=c.node_id, b=d.node_id, resistance=0.01)]))
    return problem.Problem(layers=layers, networks=nets)


def flat(prob):
    polygons = [gridmesh.rings_of(g) for layer in prob.layers for g in layer.geoms]
    groups = np.array([k for k, layer in enumerate(prob.layers) for _ in layer.geoms], dtype=np.int32)
    points = np.array([(c.point.x, c.point.y) for net in prob.networks for c in net.connections], dtype=np.float64)
    point_groups = np.array([prob.layers.index(c.layer) for net in prob.networks for c in net.connections], dtype=np.int32)
    return polygons, groups, points, point_groups


def must_read(polygons, groups, points, point_groups) -> dict:
    """Bytes per pass, from the shapes: boxes of every (query, polygon of its group), segments of every candidate."""
    boxes = np.array([R.box_of(p) for p in polygons])
    n_seg = np.array([sum(len(r) for r in p) for p in polygons], dtype=np.int64)
    pairs = candidates = seg_reads = 0
    for g in np.unique(groups):
        mine, polys = np.flatnonzero(point_groups == g), np.flatnonzero(groups == g)
        x, y = points[mine, 0][:, None], points[mine, 1][:, None]
        b = boxes[polys]
        cand = (x >= b[:, 0]) & (x <= b[:, 2]) & (y >= b[:, 1]) & (y <= b[:, 3])
        pairs += cand.size
        candidates += int(cand.sum())
        seg_reads += int((cand * n_seg[polys][None, :]).sum())
    per_pass = 32 * pairs + 32 * seg_reads
    return {"query_polygon_pairs": int(pairs), "candidates": candidates, "candidate_segments": seg_reads, "bytes_per_pass": int(per_pass),
            "bytes_both_passes": int(2 * per_pass), "us_at_8TBps_both_passes": round(1e6 * 2 * per_pass / HBM_BYTES_PER_S, 2),
            "note": "the boxes of a layer (32 B per polygon) are shared by all its queries and fit in L2; HBM sees them once"}


def call_alone(ctx, polygons, groups, points, point_groups, repeats):
    """ms of ``padne_polygons_locate`` + ``_destroy`` on arrays flattened once (nothing fetched), the first call dropped."""
    import ctypes as C
    rings = [np.ascontiguousarray(r, dtype=np.float64) for poly in polygons for r in poly]
    prp = np.concatenate([[0], np.cumsum([len(p) for p in polygons])]).astype(np.int64)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    xy = np.ascontiguousarray(np.concatenate(rings))
    pg, qg = np.ascontiguousarray(groups, dtype=np.int32), np.ascontiguousarray(point_groups, dtype=np.int32)
    q = np.ascontiguousarray(points, dtype=np.float64)
    print("timing padne_polygons_locate ...", file=sys.stderr, flush=True)
    ms = []
    for _ in range(repeats + 1):
        handle, n_hit = C.c_void_p(), C.c_int64(0)
        t0 = time.perf_counter()
        rc = ctx._lib.padne_polygons_locate(ctx._h, len(polygons), _hip._ptr(prp, _hip._PI64), _hip._ptr(rp, _hip._PI64),
                                            _hip._ptr(xy, _hip._PF64), _hip._ptr(pg, _hip._PI32), len(q), _hip._ptr(q, _hip._PF64),
                                            _hip._ptr(qg, _hip._PI32), C.byref(n_hit), C.byref(handle))
        ms.append(1e3 * (time.perf_counter() - t0))
        _hip._check(rc)
        ctx._lib.padne_polygons_locate_destroy(handle)
    return [round(x, 3) for x in ms[1:]], round(float(np.median(ms[1:])), 3), int(n_hit.value)


def timed(fn, repeats, what=""):
    print(f"timing {what} ...", file=sys.stderr, flush=True)
    ms, out = [], None
    for _ in range(repeats + 1):                                     # (the first call warms the pools and is dropped)
        t0 = time.perf_counter()
        out = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return [round(x, 3) for x in ms[1:]], round(float(np.median(ms[1:])), 3), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--side", type=float, default=100.0)
    ap.add_argument("--antipad-pitch", type=float, default=5.0)
    ap.add_argument("--pads", type=int, default=10000)
    ap.add_argument("--connections", type=int, default=2000)
    ap.add_argument("--dead", type=int, default=50)
    ap.add_argument("--unplaced", type=int, default=10)
    ap.add_argument("--maximum-size", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--skip-device", action="store_true", help="the shapes, the bytes and the restatement only (no GPU needed)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob = board(args)
    polygons, groups, points, point_groups = flat(prob)
    out = {
        "what": "padne_polygons_locate on a synthetic board, warm, the device call alone; compute_connectivity and prepare_board "
                "around it; the numpy restatement on the same host; no kernel trace taken, the kernels' own times are not measured",
        "layers": args.layers, "polygons": len(polygons), "segments": int(sum(len(r) for p in polygons for r in p)),
        "connections": len(points), "networks": len(prob.networks), "repeats": args.repeats,
        "must_read_bytes": must_read(polygons, groups, points, point_groups),
    }
    ref_ms, ref_median, want = timed(lambda: R.locate_by_layer(polygons, groups, points, point_groups), args.host_repeats, "the restatement")
    out["restatement"] = {"locate_by_layer_ms": ref_ms, "locate_by_layer_ms_median": ref_median, "hits": int(len(want[1])),
                          "hits_on_the_boundary": int((want[2] == 2).sum())}
    if args.skip_device:
        out["device"] = "not measured"
    else:
        ctx = solver.get_context()
        ms, median, got = timed(lambda: _hip.locate_polygons(ctx, polygons, groups, points, point_groups), args.repeats, "locate_polygons")
        agree = all(np.array_equal(g, w) for g, w in zip(got, want))
        out["device"] = {"locate_polygons_ms": ms, "locate_polygons_ms_median": median, "equals_the_restatement": bool(agree),
                         "note": "the wrapper flattens the rings in Python before the call: host time is included"}
        ms, median, n_hit = call_alone(ctx, polygons, groups, points, point_groups, args.repeats)
        out["device"].update({"padne_polygons_locate_ms": ms, "padne_polygons_locate_ms_median": median, "hits": n_hit,
                              "call_note": "the C entry on arrays flattened once: host checks, uploads, four kernels and a scan, "
                                           "the synchronise; nothing fetched"})
        ms, median, con = timed(lambda: solver.compute_connectivity(prob), args.host_repeats, "compute_connectivity")
        kept = solver.filter_dead_networks(prob, con)
        out["compute_connectivity"] = {"ms": ms, "ms_median": median, "connected_polygons": len(con.connected), "unplaced": len(con.unplaced),
                                       "kept_networks": len(kept), "dropped_networks": len(prob.networks) - len(kept)}
        mesher = GridMesher(mesh.Mesher.Config(maximum_size=args.maximum_size), graded=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", solver.SolverWarning)
            ms, median, prepared = timed(lambda: solver.prepare_board(prob, mesher=mesher), args.host_repeats, "prepare_board")
        out["prepare_board"] = {"mesher": "GridMesher(graded=True)", "maximum_size": args.maximum_size, "ms": ms, "ms_median": median,
                                "meshes": len(prepared.meshes), "vertices": int(sum(len(m.points) for m in prepared.meshes)),
                                "faces": int(sum(len(m.triangles) for m in prepared.meshes))}
        assert agree, "the device and the restatement disagree"
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""``FieldSampler`` on one solved board: what its creation, a million points and a 4096 x 4096 raster cost.

The board is ``board()`` of ``scripts/load_cases.py`` (four ``Rect`` layers meshed by ``StructuredMesher``, about 1 M
unknowns by default).  Timed warm, ``--repeats`` alternated runs, medians: the creation of a sampler (host time, split by
the library into the upload of meshes and potentials and the index build), ``points`` with ``--points`` random points on
one layer and ``raster`` with ``--raster`` x ``--raster`` pixels over it, each with the device time of its kernel.  The
kernel's least traffic is 36 bytes out per sample (face 4, V 8, J 16, p 8), 16 bytes in per uploaded point, and the mesh it
touches (at most 12 + 24 bytes per face and vertex of the layer); ``*_of_peak`` sets that against 8 TB/s.  The baseline is
the reference viewer's way on the same host and the same points: ``scipy.spatial.cKDTree`` over the layer's vertices, built
and queried for the nearest vertex (it answers a weaker question: no containment test, no interpolation).  Prints one JSON
object, and writes it to ``--out``.

    python scripts/sampling.py [--side 100] [--h 0.2] [--repeats 5] [--only queries] [--out FILE]

``--only queries`` runs one warm-up and the query calls alone (a target for ``rocprofv3 --kernel-trace --stats``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import scipy.spatial

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from load_cases import board  # noqa: E402
from padne_amd import mesh, solver  # noqa: E402
from padne_amd.structured import StructuredMesher  # noqa: E402

PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--raster", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["queries"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    mesher = StructuredMesher(mesh.Mesher.Config(maximum_size=args.h))
    meshes, layer_of = solver.mesh_problem(prob, None, mesher)
    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    sol = solver.solve_meshed(prob, meshes, layer_of)
    solve_first_s = time.perf_counter() - t
    t = time.perf_counter()
    solver.solve_meshed(prob, meshes, layer_of)
    solve_ms = 1e3 * (time.perf_counter() - t)
    lay = prob.layers[0]
    ls = sol.layer_solutions[0]
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)
    layer_vert = sum(len(m.points) for m in ls.meshes)
    layer_tri = sum(len(m.triangles) for m in ls.meshes)
    q = np.random.default_rng(0).uniform(-0.05 * args.side, 1.05 * args.side, size=(args.points, 2))
    pixel = 1.1 * args.side / args.raster
    origin = (-0.05 * args.side, -0.05 * args.side)

    fs = solver.FieldSampler(sol)                                # warm-up: pools, first launches
    fs.points(lay, q)
    fs.raster(lay, origin, pixel, args.raster, args.raster)
    if args.only == "queries":
        for _ in range(args.repeats):
            fs.points(lay, q)
            fs.raster(lay, origin, pixel, args.raster, args.raster)
        fs.close()
        print(json.dumps({"only": "queries", "repeats": args.repeats}))
        return
    fs.close()

    ms = {k: [] for k in ("create", "create_upload", "create_index", "points", "points_kernel", "raster", "raster_kernel")}
    candidates = {}
    for _ in range(args.repeats):
        t = time.perf_counter()
        fs = solver.FieldSampler(sol)
        ms["create"].append(1e3 * (time.perf_counter() - t))
        st = fs.stats(lay)
        ms["create_upload"].append(1e3 * st["upload_seconds"])
        ms["create_index"].append(1e3 * st["build_seconds"])
        for what, call in (("points", lambda: fs.points(lay, q)),
                           ("raster", lambda: fs.raster(lay, origin, pixel, args.raster, args.raster))):
            t = time.perf_counter()
            res = call()
            ms[what].append(1e3 * (time.perf_counter() - t))
            st = fs.stats(lay)
            ms[f"{what}_kernel"].append(1e3 * st["last_kernel_seconds"])
            candidates[what] = st["last_candidates"] / st["last_queries"]
            inside = float((res.face >= 0).mean())
            candidates[f"{what}_inside_share"] = round(inside, 4)
        fs.close()

    # the reference viewer's read-out: a KD-tree over the layer's vertices, the nearest vertex of every point
    pts = np.concatenate([m.points for m in ls.meshes])
    pot = np.concatenate([zf.values for zf in ls.potentials])
    tree_ms = {"build": [], "query_points": []}
    for _ in range(max(1, min(args.repeats, 3))):
        t = time.perf_counter()
        tree = scipy.spatial.cKDTree(pts)
        tree_ms["build"].append(1e3 * (time.perf_counter() - t))
        t = time.perf_counter()
        _d, idx = tree.query(q)
        tree_ms["query_points"].append(1e3 * (time.perf_counter() - t))
    nearest = pot[idx]
    sample = solver.FieldSampler(sol)
    mine = sample.points(lay, q)
    stats = [sample.stats(layer) for layer in prob.layers]
    sample.close()
    both = mine.face >= 0
    med = lambda xs: float(np.median(xs))  # noqa: E731
    mesh_bytes = 12 * layer_tri + 24 * layer_vert
    n_pix = args.raster * args.raster
    least = {"points": 36 * args.points + 16 * args.points + mesh_bytes, "raster": 36 * n_pix + mesh_bytes}
    out = {
        "what": "FieldSampler on a solved board: creation, points and a raster of one layer, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "layer_vertices": layer_vert, "layer_triangles": layer_tri,
        "points": args.points, "raster": [args.raster, args.raster],
        "solve_meshed_first_s": round(solve_first_s, 3), "solve_meshed_ms": round(solve_ms, 1),
        **{f"{key}_ms": [round(x, 2) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 2) for key, v in ms.items()},
        "bytes_per_sample_home": 36,
        "points_least_bytes": least["points"], "raster_least_bytes": least["raster"],
        "points_kernel_of_peak": round(least["points"] / (1e-3 * med(ms["points_kernel"])) / PEAK_BYTES_PER_S, 4),
        "raster_kernel_of_peak": round(least["raster"] / (1e-3 * med(ms["raster_kernel"])) / PEAK_BYTES_PER_S, 4),
        "mean_candidates_per_query": {k: round(v, 3) if "share" not in k else v for k, v in candidates.items()},
        "index": [{k: st[k] for k in ("bins_x", "bins_y", "entries", "faces")} for st in stats],
        "kdtree_nearest_vertex_ms": {k: round(med(v), 1) for k, v in tree_ms.items()},
        "max_abs_difference_to_nearest_vertex_V": float(np.abs(mine.potential[both] - nearest[both]).max()),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

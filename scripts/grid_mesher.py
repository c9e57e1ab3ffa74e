"""The grid mesher on outlines of the size of the 1.0 M-unknown board: what one batch costs, and what it must move.

The board of ``scripts/load_cases.py`` is four layers of ``--side`` mm meshed at ``--h`` mm (100 mm at 0.2 mm: 4 x 251 001
vertices).  Here the four layers are outlines a structured mesher cannot take: an L-shaped pour, a plane with a lattice of
round antipads, a rectangle rotated by 0.3 rad and a plane with one large cut-out, all within ``--side`` and meshed in one
``padne_polymesh_create`` at the lattice spacing ``--h`` (warm, ``--repeats`` times, the median reported, fetch included and
apart).  ``min_bytes`` states, from the array sizes, what each stage must move at least, every array read or written once;
a kernel trace gives their times.  Prints one JSON object, and writes it to ``--out``.

    python scripts/grid_mesher.py [--side 100] [--h 0.2] [--repeats 5] [--only mesh] [--out FILE]

``--only mesh`` runs one warm-up and the batches alone (a target for ``rocprofv3 --kernel-trace --stats``).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from padne_amd import _hip, gridmesh, solver  # noqa: E402

HBM_BYTES_PER_S = 8e12


def ring(points):
    return np.asarray(points, dtype=np.float64)


def ngon(n, radius, cx, cy):
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([cx + radius * np.cos(a), cy + radius * np.sin(a)], axis=1)


def outlines(side: float, antipad_pitch: float):
    s, o = side, 0.037                                              # (off the lattice lines)
    ell = [ring([(o, o), (s - o, o), (s - o, 0.4 * s), (0.4 * s, 0.4 * s), (0.4 * s, s - o), (o, s - o)])]
    n = max(1, int(s / antipad_pitch) - 1)
    plane = [ring([(o, o), (s - o, o), (s - o, s - o), (o, s - o)])] + [
        ngon(16, 0.4, (i + 1) * antipad_pitch + o, (j + 1) * antipad_pitch + o) for j in range(n) for i in range(n)]
    c, q = math.cos(0.3), math.sin(0.3)
    w, hgt = 0.68 * s, 0.5 * s
    rot = [ring([(0.3 * s + c * x - q * y, 0.05 * s + q * x + c * y) for x, y in ((0, 0), (w, 0), (w, hgt), (0, hgt))])]
    cut = [ring([(o, o), (s - o, o), (s - o, s - o), (o, s - o)]), ngon(96, 0.25 * s, 0.5 * s + o, 0.5 * s)]
    return [ell, plane, rot, cut]


def sizes(polygons, h: float) -> dict:
    """Lattice vertices, rows, segments, (segment, band) pairs, and the segments a sign or cut workgroup stages (a band is
    staged once per 256 vertices of its row)."""
    n_lat = n_row = n_seg = n_band = staged = 0
    for rings in polygons:
        pts = np.concatenate(rings)
        i0, j0 = math.floor(pts[:, 0].min() / h) - 1, math.floor(pts[:, 1].min() / h) - 1
        nx, ny = math.ceil(pts[:, 0].max() / h) + 1 - i0 + 1, math.ceil(pts[:, 1].max() / h) + 1 - j0 + 1
        y0 = np.concatenate([np.roll(r[:, 1], 1) for r in rings])
        y1 = np.concatenate([r[:, 1] for r in rings])
        lo = np.floor(np.minimum(y0, y1) / h).astype(np.int64)
        hi = np.floor(np.maximum(y0, y1) / h).astype(np.int64)
        pairs = int((hi - lo + 1).sum())                            # (within a pair per segment of the exact count)
        n_lat, n_row, n_seg, n_band = n_lat + nx * ny, n_row + ny, n_seg + len(y0), n_band + pairs
        staged += pairs * ((nx + 255) // 256)
    return {"lattice_vertices": n_lat, "rows": n_row, "segments": n_seg, "band_entries": n_band, "staged_segments": staged}


def min_bytes(z: dict, n_vert: int, n_tri: int) -> dict:
    """The bytes each stage must move at least, every array read or written once."""
    L, S, B, G = z["lattice_vertices"], z["segments"], z["band_entries"], z["staged_segments"]
    return {
        "polymesh_band_kernel<count>": 36 * S + 4 * B,
        "scan_of_the_rows": 8 * z["rows"],
        "polymesh_band_kernel<fill>": 36 * S + 8 * B,
        "polymesh_sign_kernel": 36 * G + L,
        "polymesh_cut_kernel": 36 * G + L + 24 * L,
        "polymesh_snap_kernel": 24 * L + L + L + 16 * L,
        "fill_of_the_flags": 16 * L,
        "polymesh_count_kernel": L + 8 * L + 4 * 3 * n_tri,
        "scan_of_the_flags": 32 * L,
        "scan_of_the_face_counts": 16 * L,
        "polymesh_vertex_kernel": 16 * L + 4 * n_vert + 16 * n_vert + 20 * n_vert,
        "polymesh_face_kernel": L + 8 * L + 4 * 3 * n_tri + 12 * n_tri,
        "fetch": 20 * n_vert + 12 * n_tri,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="lattice spacing in mm")
    ap.add_argument("--antipad-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["mesh"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    polygons = outlines(args.side, args.antipad_pitch)
    ctx = solver.get_context()
    meshes = _hip.polymesh(ctx, polygons, args.h)                    # warm-up: pools
    ms = []
    for _ in range(args.repeats):
        t = time.perf_counter()
        meshes = _hip.polymesh(ctx, polygons, args.h)
        ms.append(1e3 * (time.perf_counter() - t))
    if args.only == "mesh":
        print(json.dumps({"only": "mesh", "repeats": args.repeats}))
        return
    # the device call alone: create and destroy, nothing fetched
    rings = [np.ascontiguousarray(r) for poly in polygons for r in poly]
    prp = np.concatenate([[0], np.cumsum([len(p) for p in polygons])]).astype(np.int64)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int64)
    xy = np.ascontiguousarray(np.concatenate(rings))
    nv, nt = np.zeros(len(polygons), dtype=np.int64), np.zeros(len(polygons), dtype=np.int64)
    create_ms = []
    for _ in range(args.repeats):
        handle = C.c_void_p()
        t = time.perf_counter()
        _hip._check(ctx._lib.padne_polymesh_create(ctx._h, len(polygons), _hip._ptr(prp, _hip._PI64), _hip._ptr(rp, _hip._PI64),
                                                   _hip._ptr(xy, _hip._PF64), args.h, 0.25, _hip._ptr(nv, _hip._PI64),
                                                   _hip._ptr(nt, _hip._PI64), C.byref(handle)))
        create_ms.append(1e3 * (time.perf_counter() - t))
        ctx._lib.padne_polymesh_destroy(handle)
    z = sizes(polygons, args.h)
    n_vert, n_tri = sum(len(m[0]) for m in meshes), sum(len(m[1]) for m in meshes)
    floor = min_bytes(z, n_vert, n_tri)
    # the host checks of GridMesher on the same batch (components, areas), for scale
    mesher = gridmesh.GridMesher(spacing=args.h, engine=lambda *_a: meshes)
    t = time.perf_counter()
    mesher.polys_to_meshes([gridmesh.Polygon(p[0], p[1:]) for p in polygons])
    checks_ms = 1e3 * (time.perf_counter() - t)
    out = {
        "what": "one padne_polymesh_create + fetch of four board outlines, warm; the create alone; GridMesher's host checks",
        "side": args.side, "h": args.h, **z, "vertices": n_vert, "faces": n_tri,
        "per_polygon": [{"vertices": len(m[0]), "faces": len(m[1]), "cut": int((m[2] == 2).sum()), "snapped": int((m[2] == 1).sum())}
                        for m in meshes],
        "report": mesher.last_report,
        "mesh_ms": [round(x, 2) for x in ms], "mesh_ms_median": round(float(np.median(ms)), 2),
        "create_ms": [round(x, 2) for x in create_ms], "create_ms_median": round(float(np.median(create_ms)), 2),
        "host_checks_ms": round(checks_ms, 2),
        "min_bytes": floor, "min_bytes_total": int(sum(floor.values())),
        "min_us_at_8TBps": {k: round(1e6 * b / HBM_BYTES_PER_S, 2) for k, b in floor.items()},
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

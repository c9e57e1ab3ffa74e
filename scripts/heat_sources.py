"""``solve_meshed_thermal`` with and without ``ThermalModel.heat_sources`` on one board, in one process.

The board is that of ``scripts/load_cases.py`` (four ``Rect`` layers of 35 um copper meshed by ``StructuredMesher``, about
1 M unknowns by default, tied by a lattice of 1 mOhm vias, all loads on) under a film of 1e-5 W/(K mm^2).  The sources are
64 footprints, 16 per layer: 12 rectangles of 3 to 8 mm and 4 squares of 0.05 mm, smaller than a face (the fallback), 0.25 W
each.  Both calls run warm and alternate, ``--repeats`` times each; medians are reported with the host phases of both.  Then,
on one handle kept open: ``Thermal.set_sources`` alone (the C entry with its Python list building, device synchronised at
its end), and ``Thermal.load`` of one column with and without the sources -- the difference is what the sources add to a
load (the upload of the face powers and the download of b are in both).

``kernel_bytes`` states what each pass must move at the least, from the counts alone (nothing measured): F faces, F_l those
of a source's layer, V vertices, S sources, E list entries, n the vertices of a polygon:
  sources_face_kernel              12 F of corners + 48 F of coordinates read at the most (gathered), 24 F written
  sources_walk_kernel<false>       per source 16 F_l of centroids read (from cache after the first source of a layer), 4 written
  sources_owner_kernel             per fallback source 12 F_l of corners + 48 F_l of coordinates at the most read, 4 written
  sources_walk_kernel<true>        as the count pass, + 4 E written
  sources_sum_kernel<false>        12 E read (face, area), 8 S written
  sources_face_lists_kernel<false> 16 F of centroids + 40 S per wave (layer, box) read, 4 F written
  sources_face_lists_kernel<true>  the same + 4 F of offsets read, 4 E written
  sources_load_kernel              per 8 columns: 8 V + 12 * 3 F (lists, two offsets per face) + 20 per (vertex, entry) read,
                                   16 V per column read and written
  sources_sum_kernel<true>         per column 24 E + the corners' theta read, 8 S written
Prints one JSON object, and writes it to ``--out``.

    python scripts/heat_sources.py [--side 100] [--h 0.2] [--repeats 3] [--only sources] [--out FILE]

``--only sources`` runs one warm-up and the calls with sources alone (a target for ``rocprofv3 --kernel-trace --stats``).
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

FILM = 1e-5                     # W/(K mm^2): 10 W/(m^2 K), still air on both faces of a board
WATTS = 0.25


def footprints(prob, side: float):
    """16 per layer on a 4 x 4 lattice of sites: 12 rectangles of 3 to 8 mm, 4 squares of 0.05 mm."""
    out = []
    for l, layer in enumerate(prob.layers):
        for i in range(16):
            cx, cy = side * (0.14 + 0.24 * (i % 4)) + 0.37 * l, side * (0.14 + 0.24 * (i // 4)) + 0.23 * l
            w, h = (0.05, 0.05) if i % 4 == l % 4 else (3.0 + (5 * i + l) % 6, 3.0 + (3 * i + 2 * l) % 6)
            out.append(solver.HeatSource.rectangle(layer, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, WATTS, name=f"U{l}.{i}"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["sources"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    sources = footprints(prob, args.side)
    models = {"plain": solver.ThermalModel(film=FILM), "sources": solver.ThermalModel(film=FILM, heat_sources=sources)}
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)

    def call(key, tm=None):
        return solver.solve_meshed_thermal(prob, meshes, layer_of, models[key], timings=tm)

    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    reports = {"sources": call("sources")[1]}                    # warm-up: library, context, pools
    first_s = time.perf_counter() - t
    if args.only == "sources":
        for _ in range(args.repeats):
            call("sources")
        print(json.dumps({"only": "sources", "repeats": args.repeats}))
        return
    reports["plain"] = call("plain")[1]
    ms = {key: [] for key in models}
    phases = {key: [] for key in models}
    for _ in range(args.repeats):
        for key in models:
            tm: dict = {}
            t = time.perf_counter()
            call(key, tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            phases[key].append(tm)
    med = lambda xs: float(np.median(xs))  # noqa: E731
    keys = ("indexing", "assembly", "stage1", "stage2", "power_density", "thermal_setup", "thermal_solve", "thermal_report",
            "solutions")

    # one handle kept open: set_sources alone, and what the sources add to a load of one column
    checked = solver.check_thermal_model(prob, models["sources"])
    indexed = solver.index_board(prob, meshes, layer_of, None, None)
    pairs = solver.global_elements(indexed.filtered_networks, indexed.node_indexer)
    resistors = [(element, row) for element, row in pairs if row[0] == "R"]
    set_ms, load_ms = [], {"plain": [], "sources": []}
    with indexed.assembled() as (L, _):
        thermal = solver._thermal_handle(L, L.layout.n_potential, checked, indexed.layer_of, len(indexed.meshes), resistors)
        try:
            face_power = np.zeros((1, n_tri))
            for _ in range(args.repeats + 1):                    # (the first of each is a warm-up)
                thermal.set_sources(len(prob.layers), indexed.layer_of, [], [])
                t = time.perf_counter()
                thermal.load(face_power)
                load_ms["plain"].append(1e3 * (time.perf_counter() - t))
                t = time.perf_counter()
                attached = solver._attach_heat_sources(thermal, prob, checked, indexed.layer_of, len(indexed.meshes))
                set_ms.append(1e3 * (time.perf_counter() - t))
                thermal.source_power(solver._source_powers(checked.sources, 1))
                t = time.perf_counter()
                b = thermal.load(face_power)
                load_ms["sources"].append(1e3 * (time.perf_counter() - t))
        finally:
            thermal.close()
    entries, n_fallback = int(attached.faces.sum()), int(attached.fallback.sum())
    per_layer = [sum(len(m.triangles) for m, l in zip(meshes, indexed.layer_of) if l == i) for i in range(len(prob.layers))]
    walked = sum(per_layer[s.layer] for s in checked.sources)
    walked_fallback = sum(per_layer[s.layer] for s, f in zip(checked.sources, attached.fallback) if f)
    n_src = len(sources)
    bytes_ = {
        "sources_face_kernel_at_most": (12 + 48 + 24) * n_tri,
        "sources_walk_count": 16 * walked + 4 * n_src,
        "sources_owner_kernel_at_most": 60 * walked_fallback + 4 * n_src,
        "sources_walk_fill": 16 * walked + 4 * entries,
        "sources_area_sum": 12 * entries + 8 * n_src,
        "sources_face_lists_count": 20 * n_tri + 40 * n_src * ((n_tri + 63) // 64),
        "sources_face_lists_fill": 24 * n_tri + 40 * n_src * ((n_tri + 63) // 64) + 4 * entries,
        "sources_load_kernel_one_column": 8 * n_vert + 36 * n_tri + 20 * 3 * entries + 16 * n_vert,
        "sources_report_one_column_at_least": 24 * entries + 8 * n_src,
    }
    set_s = 1e-3 * med(set_ms[1:])
    added_load_s = 1e-3 * (med(load_ms["sources"][1:]) - med(load_ms["plain"][1:]))
    build_bytes = sum(v for k, v in bytes_.items() if not k.startswith(("sources_load", "sources_report")))
    out = {
        "what": "solve_meshed_thermal with and without heat_sources, same board, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "film_W_per_K_mm2": FILM, "sources": n_src, "fallbacks": n_fallback,
        "list_entries": entries, "largest_list": int(attached.faces.max()), "first_call_s": round(first_s, 3),
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "phases_ms": {key: {p: round(1e3 * med([q.get(p, 0.0) for q in v]), 1) for p in keys} for key, v in phases.items()},
        "set_sources_ms": [round(x, 3) for x in set_ms[1:]], "set_sources_ms_median": round(med(set_ms[1:]), 3),
        "load_one_column_ms": {key: round(med(v[1:]), 3) for key, v in load_ms.items()},
        "load_added_ms": round(1e3 * added_load_s, 3),
        "kernel_bytes": bytes_,
        "set_sources_bytes": build_bytes,
        "set_sources_GB_per_s": round(build_bytes / set_s / 1e9, 1) if set_s > 0 else None,
        "load_added_GB_per_s": round(bytes_["sources_load_kernel_one_column"] / added_load_s / 1e9, 1) if added_load_s > 0 else None,
        "load_sum_W": float(b.sum()), "source_heat_W": reports["sources"].source_heat,
        "total_heat_W": {key: rep.total_heat for key, rep in reports.items()},
        "total_loss_W": {key: rep.total_loss for key, rep in reports.items()},
        "thermal_iterations": {key: rep.info["iterations"] for key, rep in reports.items()},
        "hotspots_degC": {key: [round(h[0], 4) if h else None for h in rep.hotspots] for key, rep in reports.items()},
        "footprints": [{k: (round(v, 4) if isinstance(v, float) else v) for k, v in e.items()} for e in reports["sources"].sources[:20]],
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

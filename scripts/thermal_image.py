"""``TemperatureSampler`` on one board: what a thermal image of all load cases costs next to the electrical sampler.

The board is that of ``scripts/thermal.py`` (4 layers, about 1 M unknowns) under ``solve_meshed_thermal`` with 8 load
cases; the sampler holds their 8 fields and the envelope, 9 in all.  Timed in one process, warm, each the median of
``--repeats`` calls on the top layer:

  creation                  ``TemperatureSampler.of_reports`` (upload of the meshes and 9 fields, the index build)
  points, 9 fields          ``--points`` (1 M) random points of the layer's box
  raster, 9 fields          ``--raster`` x ``--raster`` (2048 x 2048) pixels over the layer's box, every field
  raster, hottest alone     the same with ``per_field=False``
  nine one-field samplers   the same points through nine samplers of one field each, summed
  FieldSampler              the same points through the electrical sampler: the yardstick, the parent's code in this run

``nine_over_one_call`` is the ratio the feature was built for: nine one-field calls over one nine-field call.  The
expectation is well above 1, because the candidate tests dominate ``sample_kernel``; it is reported, not asserted.

``least_bytes`` states what each form must move at the least, from the counts alone -- n samples, F fields; the gathers of
the mesh and of the fields are not counted (they hit the caches or not, depending on the points' order):
  points                    16 n uploaded and read; 4 n (face) + 8 F n (T) + 12 n (hottest, its field) stored and brought home
  raster                    nothing uploaded; the same stores, plus 16 (F + 1) bytes per 256 pixels of tile tops
  raster, hottest alone     16 n stored and brought home, plus the tile tops
  FieldSampler              16 n uploaded and read; 36 n (face, V, J, p) stored and brought home
With ``--kernel-stats FILE`` (the ``--stats`` table of ``rocprofv3 --kernel-trace --stats -- python
scripts/thermal_image.py --only queries``, a run of its own) the kernels' average times are added.

    python scripts/thermal_image.py [--side 100] [--h 0.2] [--points 1000000] [--raster 2048] [--repeats 5] [--only queries]
                                    [--kernel-stats FILE] [--out FILE]
"""
from __future__ import annotations

import argparse
import csv
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

FILM = 1e-5                    # W / (K mm^2): 10 W/(m^2 K), still air
KERNELS = ["sample_fields_kernel<false>", "sample_fields_kernel<true>", "sample_fields_fold_kernel", "sample_kernel<false>",
           "sample_kernel<true>"]


def timed(fn, repeats):
    """(the last result, the median wall time): every call ends with its results on the host."""
    times, out = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return out, float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0)
    ap.add_argument("--h", type=float, default=0.2)
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--raster", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=["queries"], default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, loads, _source = board(args.side, args.via_pitch)
    model = solver.ThermalModel(film=FILM)
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert, n_tri = sum(len(m.points) for m in meshes), sum(len(m.triangles) for m in meshes)
    cases = [{load: (0.4 + 0.2 * ((3 * j + q) % 8)) * load.current for q, load in enumerate(loads)} for j in range(8)]
    warnings.simplefilter("ignore", solver.SolverWarning)
    sols, reports, envelope = solver.solve_meshed_thermal(prob, meshes, layer_of, model, cases=cases)
    top = prob.layers[0]
    n, side, F = args.points, args.side, len(reports) + 1
    xy = np.random.default_rng(5).uniform(0.0, side, size=(n, 2))
    w = h = args.raster
    origin, pixel = (0.0, 0.0), side / w

    make = lambda: solver.TemperatureSampler.of_reports(prob, reports, envelope=envelope, model=model)  # noqa: E731
    make().close()                                                          # warm: pools, code objects
    created = []

    def create():
        created.append(make())
        return created[-1]
    ts, creation_s = timed(create, args.repeats)
    for other in created[:-1]:
        other.close()
    fs = solver.FieldSampler(sols[0])
    queries = {"points_9_fields": lambda: ts.points(top, xy),
               "raster_9_fields": lambda: ts.raster(top, origin, pixel, w, h),
               "raster_hottest_alone": lambda: ts.raster(top, origin, pixel, w, h, per_field=False),
               "field_sampler_points": lambda: fs.points(top, xy)}
    if args.only == "queries":
        for call in queries.values():
            call()
            call()
        return
    singles = [solver.TemperatureSampler(prob, [field], model=model) for field in
               [r.temperatures for r in reports] + [envelope.temperatures]]
    queries["nine_one_field_samplers"] = lambda: [s.points(top, xy) for s in singles]
    out = {"what": "TemperatureSampler with the 8 load cases of solve_meshed_thermal and their envelope on the 4-layer board of "
                   "scripts/thermal.py, next to FieldSampler on the same points; same process, warm, medians of --repeats calls "
                   "that end with the results on the host",
           "n_vertices": n_vert, "n_faces": n_tri, "layers": len(prob.layers), "fields": F, "points": n, "raster": [h, w],
           "repeats": args.repeats, "creation_s": round(creation_s, 4), "stats_of_the_top_layer": None, "calls": {}}
    for name, call in queries.items():
        call()                                                              # warm
        _r, seconds = timed(call, args.repeats)
        out["calls"][name] = {"call_s": round(seconds, 5)}
        if name != "nine_one_field_samplers":
            st = (fs if name == "field_sampler_points" else ts).stats(top)
            out["calls"][name]["kernel_s"] = round(st["last_kernel_seconds"], 6)
            out["calls"][name]["candidates_per_query"] = round(st["last_candidates"] / max(st["last_queries"], 1), 3)
        else:
            out["calls"][name]["kernel_s"] = round(sum(s.stats(top)["last_kernel_seconds"] for s in singles), 6)
    out["stats_of_the_top_layer"] = {k: v for k, v in ts.stats(top).items() if not k.startswith("last_")}
    c = out["calls"]
    out["nine_over_one_call"] = round(c["nine_one_field_samplers"]["call_s"] / c["points_9_fields"]["call_s"], 3)
    out["nine_over_one_kernel"] = round(c["nine_one_field_samplers"]["kernel_s"] / c["points_9_fields"]["kernel_s"], 3)
    out["one_call_over_field_sampler"] = round(c["points_9_fields"]["call_s"] / c["field_sampler_points"]["call_s"], 3)
    tiles = -(-w * h // 256)
    out["least_bytes"] = {"points_9_fields": {"uploaded": 16 * n, "stored_and_home": (4 + 8 * F + 12) * n},
                          "raster_9_fields": {"uploaded": 0, "stored_and_home": (4 + 8 * F + 12) * w * h, "tile_tops": 16 * (F + 1) * tiles},
                          "raster_hottest_alone": {"uploaded": 0, "stored_and_home": 16 * w * h, "tile_tops": 16 * (F + 1) * tiles},
                          "field_sampler_points": {"uploaded": 16 * n, "stored_and_home": 36 * n},
                          "nine_one_field_samplers": {"uploaded": 9 * 16 * n, "stored_and_home": 9 * (4 + 8 + 12) * n}}
    if args.kernel_stats:
        measured = {}
        with open(args.kernel_stats) as f:
            for row in csv.DictReader(f):
                for name in KERNELS:
                    if name in row["Name"].replace(" ", ""):
                        measured[name] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 3)}
        out["kernel_stats"] = measured
    for s in singles + [ts, fs]:
        s.close()
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

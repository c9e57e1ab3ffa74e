"""``solve_meshed_thermal`` with a float film and with film curves on one board, in one process.

The board is that of ``scripts/load_cases.py`` (four ``Rect`` layers of 35 um copper meshed by ``StructuredMesher``, about
1 M unknowns by default, tied by a lattice of 1 mOhm vias).  As it stands its sources deliver about 957 W, a mean rise of
2393 K under still air, so the calls are timed on one load case that multiplies every source by a common factor, chosen from
the one-way solve so that delivered power / (film x area) is ``--rise`` kelvin (30 by default: the necks are then hundreds
of kelvin above ambient, the planes a few); the factor is stated in the output.  The float film is 1e-5 W/(K mm^2); the curve is
natural convection from a plate plus radiation of a grey surface to surroundings at the ambient temperature, tabulated to
``--upto`` kelvin, whose h(0) is that of the law (so the two calls differ: the comparison is of cost, the hotspots are
printed).  Both calls run warm and alternate, ``--repeats`` times each; medians are reported with the host phases of both,
and for the curve the rounds, the increments and the laps of every round: ``linearise`` (the pass that rewrites the
diagonals and drops the hierarchy), ``hierarchy`` (the multigrid setup inside the round's solve), ``thermal_solve`` (the
whole solve call: load plus c, setup, iteration loop, theta home), ``increment``.

``kernel_bytes`` states what each new pass must move at the least, from the counts alone (nothing measured), V vertices, N
unknowns, per round:
  film_terms_kernel (linearise)   8 V theta + 8 V M_v + 4 V diagonal places + 8 V D0 + 8 V hM0 read, 8 V diagonals + 8 V c written
  film_terms_kernel (increment)   8 V theta + 8 V linearised iterate + 8 V M_v read, 8 V hM + 20 per tile of 256 written
  film_add_kernel                 8 V c + 8 V b read, 8 V b written
  copies                          8 N the iterate kept by linearise, 8 N the load kept by the first solve
Prints one JSON object, and writes it to ``--out``.

    python scripts/film_curve.py [--side 100] [--h 0.2] [--rise 30] [--upto 600] [--repeats 3] [--out FILE]
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
AMBIENT_K = 298.15
EMISSIVITY_SIGMA = 0.9 * 5.67e-14       # W/(mm^2 K^4): a solder mask
CONVECTION = 2.6e-6             # W/(mm^2 K^1.25): h = 2.6 theta^(1/4) W/(m^2 K), a small horizontal plate in still air


def curve(upto: float) -> solver.FilmCurve:
    return solver.FilmCurve.natural_convection(CONVECTION, upto=upto) + solver.FilmCurve.radiation(EMISSIVITY_SIGMA, AMBIENT_K, upto=upto)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--rise", type=float, default=30.0, help="delivered power / (film x area) of the scaled board [K]")
    ap.add_argument("--upto", type=float, default=600.0, help="the last knot of the curve [K above ambient]")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    table = curve(args.upto)
    models = {"float": solver.ThermalModel(film=FILM, ambient=AMBIENT_K - 273.15),
              "curve": solver.ThermalModel(film=table, ambient=AMBIENT_K - 273.15)}
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)

    area = len(prob.layers) * args.side ** 2
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]
    warnings.simplefilter("ignore", solver.SolverWarning)
    t = time.perf_counter()
    _sol, unscaled = solver.solve_meshed_thermal(prob, meshes, layer_of, models["float"])       # warm-up, and the power as it stands
    first_s = time.perf_counter() - t
    factor = float(np.sqrt(args.rise * FILM * area / unscaled.total_heat))
    case = {e: factor * getattr(e, solver.CASE_FIELDS[solver.element_kind(e)]) for e in sources}

    def call(key, tm=None):
        _s, reps, _env = solver.solve_meshed_thermal(prob, meshes, layer_of, models[key], cases=[case], timings=tm)
        return _s[0], reps[0]

    reports = {"curve": call("curve")[1]}
    reports["float"] = call("float")[1]
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
    film = reports["curve"].film
    laps = ("linearise", "thermal_solve", "hierarchy", "increment")
    rounds = [{lap: round(1e3 * med([run["rounds"][r][lap] for run in phases["curve"]]), 2) for lap in laps}
              for r in range(film["rounds"])]
    for r, entry in enumerate(rounds):
        entry["iteration_loop_and_load"] = round(entry["thermal_solve"] - entry["hierarchy"], 2)
        entry["iterations"] = phases["curve"][0]["rounds"][r]["iterations"]
    n_pot = n_vert                                               # (the board has no internal nodes)
    tiles = sum((len(m.points) + 255) // 256 for m in meshes)
    bytes_ = {"film_terms_kernel_linearise": (8 + 8 + 4 + 8 + 8 + 8 + 8) * n_vert,
              "film_terms_kernel_increment": (8 + 8 + 8 + 8) * n_vert + 20 * tiles,
              "film_add_kernel": 24 * n_vert, "copies_per_round": 8 * n_pot, "copy_of_the_load_once": 8 * n_pot}
    per_round = bytes_["film_terms_kernel_linearise"] + bytes_["film_terms_kernel_increment"] + bytes_["film_add_kernel"]
    out = {
        "what": "solve_meshed_thermal with a float film and with a film curve, same board, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "film_W_per_K_mm2": FILM, "curve_knots": len(table.rise),
        "curve_h0": float(table.film[0]), "curve_h_last": float(table.film[-1]), "curve_upto_K": args.upto,
        "first_call_s": round(first_s, 3), "unscaled_delivered_W": unscaled.total_heat, "source_factor": factor,
        "target_mean_rise_K": args.rise,
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "curve_over_float": round(med(ms["curve"]) / med(ms["float"]), 2),
        "phases_ms": {key: {p: round(1e3 * med([q.get(p, 0.0) for q in v]), 1) for p in keys} for key, v in phases.items()},
        "film": {"rounds": film["rounds"], "increments_K": film["increments"], "converged": film["converged"], "beyond": film["beyond"]},
        "rounds_ms": rounds,
        "hierarchy_share_of_rounds": round(sum(r["hierarchy"] for r in rounds) / max(sum(r["linearise"] + r["thermal_solve"] + r["increment"]
                                                                                     for r in rounds), 1e-9), 3),
        "kernel_bytes": bytes_, "bytes_per_vertex_per_round": round(per_round / n_vert, 1),
        "total_heat_W": {key: rep.total_heat for key, rep in reports.items()},
        "total_loss_W": {key: rep.total_loss for key, rep in reports.items()},
        "thermal_iterations_last_solve": {key: rep.info["iterations"] for key, rep in reports.items()},
        "hotspots_degC": {key: [round(h[0], 4) if h else None for h in rep.hotspots] for key, rep in reports.items()},
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

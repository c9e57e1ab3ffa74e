"""``solve_meshed_electrothermal`` next to ``solve_meshed_thermal`` on one board, and the entries of the coupling handle
against the bytes they must move.

The board is that of ``scripts/load_cases.py`` (four ``Rect`` layers of 35 um copper meshed by ``StructuredMesher``, about
1 M unknowns by default, tied by a lattice of 1 mOhm vias), the thermal model that of ``scripts/thermal.py`` (Wiedemann-Franz,
a film of 1e-5 W/(K mm^2)).  As it stands the board's sources deliver about 957 W, a mean rise of 2393 K over its 4 x 100 x
100 mm^2 of film: meaningless for a model that is linear in the temperature.  Every source is therefore multiplied by one
factor, chosen from the one-way solve so that delivered power / (film x area) is ``--rise`` kelvin (30 by default); the
factor is stated in the output.  Both calls run warm and alternate, ``--repeats`` times each; medians are reported.
``rounds_ms`` are the host laps of every round of the last coupled call (revalue, stage 1, stage 2, the thermal solve, the
update).

``entries`` times the handle's entries on the solved board by host timers around the synchronous calls (the median of
``--entry-repeats`` calls), next to the bytes the kernels in them must move at the least and that as a share of 8 TB/s.  A
host timer sees the launch, the kernels and the read-back of a flag or a maximum: an upper bound of the kernel's own time
(``rocprofv3 --kernel-trace --stats`` on ``--only coupled`` gives that).  V vertices, T faces, N rows and nnz entries of L:
  coupled_revalue_kernel     8 nnz of L0 + 4 nnz of columns + 4 N of row pointers + 4 V + 12 T of lists + 12 T of corners +
                             16 V of xy + 8 T of scales read, 8 nnz written; the entry also copies the scale (16 T)
  coupled_scale_kernel       12 T of corners + 8 V of theta + 8 T of previous means read, 16 T written (+ 8 per 256 faces)
  coupled_post_scale_kernel  16 T read, 8 T written, behind power_density_block_kernel (12 T + 16 V + 8 V read, 8 T written)
Prints one JSON object, and writes it to ``--out``.

    python scripts/coupled.py [--side 100] [--h 0.2] [--rise 30] [--repeats 3] [--only coupled] [--out FILE]
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
from padne_amd import _hip, mesh, solver  # noqa: E402
from padne_amd.structured import StructuredMesher  # noqa: E402

FILM = 1e-5                     # W/(K mm^2): 10 W/(m^2 K), still air on both faces of a board
PEAK = 8e12                     # bytes/s


def entry_times(prob, meshes, layer_of, case, model, repeats):
    """Median seconds of the handle's entries on the board solved once with the copper at ambient."""
    checked = solver.check_electrothermal_model(prob, model)
    cases = solver.check_load_cases(prob, [case])
    b = solver.index_board(prob, meshes, layer_of)
    pairs = solver.global_elements(b.filtered_networks, b.node_indexer)
    resistors = [(e, row) for e, row in pairs if row[0] == "R"]
    th, n_mesh = checked.thermal, len(b.meshes)
    out = {}
    with b.assembled() as (L, _):
        n_tri, n_vert = len(L.tri), len(b.vindex)
        thermal = _hip.Thermal(L.dev, L.layout.n_potential, [th.kappa[layer_of[i]] for i in range(n_mesh)],
                               [th.film[layer_of[i]] for i in range(n_mesh)], [r[1] for _, r in resistors],
                               [r[2] for _, r in resistors], [th.links[e] for e, _ in resistors])
        coupled = _hip.Coupled(L.dev, thermal, [checked.alpha[layer_of[i]] for i in range(n_mesh)], th.ambient,
                               checked.conductance_temperature)
        try:
            coupled.revalue()
            rows, cols, vals = solver.stamp_load_cases(b.filtered_networks, b.node_indexer, L.shape[0], cases)
            plan, _V, _norms, _res, _t, _m = solver._solve_block_on_device(L, rows, cols, vals, 1, 1, solver._Laps(None))
            coupled.solve_kkt(plan, None, download=False)

            def timed(call):
                call()
                ts = []
                for _ in range(repeats):
                    t = time.perf_counter()
                    call()
                    ts.append(time.perf_counter() - t)
                return float(np.median(ts))

            out["update"] = timed(coupled.update)
            out["power_density"] = timed(lambda: coupled.power_density(plan, n_tri))
            solver._drop_plans(L)
            out["revalue"] = timed(coupled.revalue)
            nnz, N = L.nnz, L.shape[0]
        finally:
            solver._drop_plans(L)
            coupled.close()
            thermal.close()
    bytes_ = {"revalue": 20 * nnz + 4 * N + 20 * n_vert + 32 * n_tri + 16 * n_tri,
              "update": 36 * n_tri + 8 * n_vert + 8 * ((n_tri + 255) // 256),
              "power_density": 24 * n_tri + (20 * n_tri + 24 * n_vert)}
    return {key: {"seconds": out[key], "bytes": bytes_[key], "share_of_8TBps": round(bytes_[key] / out[key] / PEAK, 4)}
            for key in out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=float, default=100.0, help="edge of the square board in mm")
    ap.add_argument("--h", type=float, default=0.2, help="vertex spacing in mm (0.2 on 100 mm: 4 x 251 001 vertices)")
    ap.add_argument("--via-pitch", type=float, default=5.0)
    ap.add_argument("--rise", type=float, default=30.0, help="delivered power / (film x area) of the scaled board [K]")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--entry-repeats", type=int, default=20)
    ap.add_argument("--only", choices=["coupled"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    prob, _loads, _source = board(args.side, args.via_pitch)
    thermal_model = solver.ThermalModel(film=FILM)
    model = solver.ElectroThermalModel(thermal=thermal_model)
    meshes, layer_of = solver.mesh_problem(prob, None, StructuredMesher(mesh.Mesher.Config(maximum_size=args.h)))
    n_vert = sum(len(m.points) for m in meshes)
    n_tri = sum(len(m.triangles) for m in meshes)
    area = len(prob.layers) * args.side ** 2
    warnings.simplefilter("ignore", solver.SolverWarning)
    sources = [e for n in prob.networks for e in n.elements if solver.element_kind(e) in solver.CASE_FIELDS]

    t = time.perf_counter()
    _sol, rep = solver.solve_meshed_thermal(prob, meshes, layer_of, thermal_model)        # warm-up, and the power as it stands
    first_s = time.perf_counter() - t
    factor = float(np.sqrt(args.rise * FILM * area / rep.total_heat))
    case = {e: factor * getattr(e, solver.CASE_FIELDS[solver.element_kind(e)]) for e in sources}
    calls = {
        "thermal": lambda tm=None: solver.solve_meshed_thermal(prob, meshes, layer_of, thermal_model, cases=[case], timings=tm),
        "electrothermal": lambda tm=None: solver.solve_meshed_electrothermal(prob, meshes, layer_of, model, cases=[case], timings=tm),
    }
    if args.only == "coupled":
        for _ in range(args.repeats):
            calls["electrothermal"]()
        print(json.dumps({"only": "coupled", "repeats": args.repeats, "source_factor": factor}))
        return
    _s, one_way, _env = calls["thermal"]()
    _s, coupled_reps, couplings, _env = calls["electrothermal"]()
    ms = {key: [] for key in calls}
    laps: dict = {}
    for _ in range(args.repeats):
        for key, call in calls.items():
            tm: dict = {}
            t = time.perf_counter()
            call(tm)
            ms[key].append(1e3 * (time.perf_counter() - t))
            if key == "electrothermal":
                laps = tm
    med = lambda xs: float(np.median(xs))  # noqa: E731
    hot = lambda r: max(h[0] for h in r.hotspots if h)  # noqa: E731
    out = {
        "what": "solve_meshed_electrothermal vs solve_meshed_thermal, one load case, same board, warm, alternated",
        "n_vertices": n_vert, "n_triangles": n_tri, "film_W_per_K_mm2": FILM, "first_call_s": round(first_s, 3),
        "unscaled_delivered_W": rep.total_heat, "unscaled_mean_rise_K": rep.total_heat / (FILM * area),
        "source_factor": factor, "target_mean_rise_K": args.rise,
        **{f"{key}_ms": [round(x, 1) for x in v] for key, v in ms.items()},
        **{f"{key}_ms_median": round(med(v), 1) for key, v in ms.items()},
        "electrothermal_over_thermal": round(med(ms["electrothermal"]) / med(ms["thermal"]), 2),
        "rounds": couplings[0].rounds, "converged": couplings[0].converged, "increments_K": couplings[0].increments,
        "iterations": couplings[0].iterations,
        "rounds_ms": [{k: round(1e3 * v, 2) if isinstance(v, float) else v for k, v in r.items()} for r in laps.get("rounds", [])],
        "phases_ms": {k: round(1e3 * v, 1) for k, v in laps.items() if isinstance(v, float)},
        "one_way": {"delivered_W": one_way[0].total_heat, "hotspot": hot(one_way[0])},
        "coupled": {"delivered_W": coupled_reps[0].total_heat, "hotspot": hot(coupled_reps[0])},
        "entries": entry_times(prob, meshes, layer_of, case, model, args.entry_repeats),
    }
    print(json.dumps(out), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

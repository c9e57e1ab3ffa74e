"""The sha256 of every array the face-kernel entries return, for one tree: what a refactor of those entries must not move.

For each of the fixture boards ``problem_mixed``, ``problem_many_meshes`` and ``problem_two_planes`` (tests/golden), with
the random cuts and the load cases of the test suite: ``solve_meshed_currents`` with 0 cuts and with cuts,
``solve_meshed_load_case_currents`` with k = 1, 3 and 9 with and without ``per_case_fields``,
``solve_meshed_sensitivities``, ``solve_meshed_load_cases``, ``solve_meshed_error``, ``CsrMatrix.power_density``,
``Context.power_density`` and ``Context.face_gradient``.  Every numpy array in what they return is hashed over its bytes,
shape and dtype, every float with it; timings are left out.  Prints a one-line summary, and writes {entry: [hashes in
visiting order]} to ``--out``.

    python scripts/refactor_hashes.py [--tree DIR] [--out FILE]

``--tree``: the root of the tree whose ``padne_amd`` and ``tests`` are used (default: this script's own).  Run it in one
process per tree (parent, this tree, parent again) and compare the files: the parent's two runs must agree with each other
before their agreement with this tree means anything.
"""
from __future__ import annotations

import argparse
import dataclasses
import hashlib
import json
import os
import struct
import sys
import warnings

import numpy as np


def hashes(obj, out: list) -> list:
    """Appends the hash of every array and float in ``obj`` (lists, tuples, dict values, the solver's dataclasses, forms with
    ``.values``), depth first.  A Problem, its elements and a mesh hold no result and are passed over."""
    if isinstance(obj, np.ndarray):
        out.append(hashlib.sha256(np.ascontiguousarray(obj).tobytes() + repr((obj.shape, str(obj.dtype))).encode()).hexdigest())
    elif isinstance(obj, (float, np.floating)):
        out.append(hashlib.sha256(struct.pack("<d", float(obj))).hexdigest())
    elif isinstance(obj, (list, tuple)):
        for item in obj:
            hashes(item, out)
    elif isinstance(obj, dict):
        for item in obj.values():
            hashes(item, out)
    elif type(obj).__name__ == "SolverInfo":
        hashes([obj.ground_node_current, obj.residual_norm], out)            # (the rest counts iterations and seconds)
    elif dataclasses.is_dataclass(obj) and type(obj).__module__.endswith("solver"):
        for f in dataclasses.fields(obj):
            if f.name not in ("problem", "meshes", "disconnected_meshes", "nodes"):
                hashes(getattr(obj, f.name), out)
    elif isinstance(getattr(obj, "values", None), np.ndarray):
        hashes(obj.values, out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "tests")]

    import sensitivity_ref as S
    from padne_amd import solver
    from test_currents import board_of, random_cuts
    from test_load_cases import block_cases
    from test_sensitivity import fixture_objectives

    assert os.path.dirname(os.path.dirname(os.path.abspath(solver.__file__))) == tree, solver.__file__
    warnings.simplefilter("ignore", solver.SolverWarning)
    ctx = solver.get_context()
    out = {}
    for name in ("problem_mixed", "problem_many_meshes", "problem_two_planes"):
        system = S.problem_system(name)
        meshes, disc = board_of(system, name)
        board = (system.prob, meshes, system.layer_of)
        cuts = random_cuts(system)
        for label, c in (("cuts0", []), ("cuts", cuts)):
            out[f"{name}/currents/{label}"] = hashes(
                solver.solve_meshed_currents(*board, c, disconnected_meshes_by_layer=disc), [])
        for k in (1, 3, 9):
            cases = block_cases(system.flat, k, seed=k)
            for fields in (True, False):
                out[f"{name}/load_case_currents/k{k}/fields{int(fields)}"] = hashes(solver.solve_meshed_load_case_currents(
                    *board, cases, cuts, per_case_fields=fields, disconnected_meshes_by_layer=disc), [])
        out[f"{name}/sensitivities"] = hashes(solver.solve_meshed_sensitivities(
            *board, fixture_objectives(system.flat), disconnected_meshes_by_layer=disc), [])
        sols = solver.solve_meshed_load_cases(*board, block_cases(system.flat, 3, seed=3), disconnected_meshes_by_layer=disc)
        out[f"{name}/load_cases"] = hashes(sols, [])
        out[f"{name}/error"] = hashes(solver.solve_meshed_error(*board, tolerance=0.05, disconnected_meshes_by_layer=disc), [])
        # the potentials of the Problem as given, in mesh order, through the three entries that take a vector
        by_mesh = dict(zip((mi for li in range(len(system.prob.layers)) for mi, l in enumerate(system.layer_of) if l == li),
                           (zf.values for ls in sols[0].layer_solutions for zf in ls.potentials)))
        pot = np.concatenate([by_mesh[mi] for mi in range(len(meshes))])
        xy = np.concatenate([m.points for m in meshes])
        tri = np.concatenate([m.triangles for m in meshes]).astype(np.int32)
        voff = np.concatenate([[0], np.cumsum([len(m.points) for m in meshes])])
        toff = np.concatenate([[0], np.cumsum([len(m.triangles) for m in meshes])])
        sigma = [system.prob.layers[l].conductance for l in system.layer_of]
        indexed = solver.index_board(*board, None, disc)
        with indexed.assembled() as (L, _):
            out[f"{name}/csr_power_density"] = hashes(L.dev.power_density(pot, len(tri)), [])
        out[f"{name}/ctx_power_density"] = hashes(ctx.power_density(xy, tri, voff, toff, sigma, pot), [])
        out[f"{name}/ctx_face_gradient"] = hashes(ctx.face_gradient(xy, tri, voff, toff, pot), [])
    result = {"tree": tree, "arrays": sum(len(v) for v in out.values()), "hashes": out}
    print(json.dumps({"tree": tree, "arrays": result["arrays"], "entries": len(out)}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()

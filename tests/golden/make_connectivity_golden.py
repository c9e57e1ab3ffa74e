"""Generate tests/golden/connectivity_boards.json by running the REAL reference's connectivity graph.

Run in the build container only (needs the reference mounted), never on the GPU machine:

    python tests/golden/make_connectivity_golden.py

For the fixture board and the seeded random boards of tests/connectivity_ref.py the reference's own
``ConnectivityGraph.create_from_problem``, ``find_connected_layer_geom_indices`` and ``filter_dead_networks`` (loaded by
oracle/ref_loader.py) run on duck-typed objects whose geometric predicate is the restatement's
(``connectivity_ref.reference_graph``).  The file holds results only: per board the connected (layer, geom) pairs and the
indices of the kept networks.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import connectivity_ref as R  # noqa: E402
from oracle import ref_loader  # noqa: E402


def main():
    ref = ref_loader.load_reference()
    out = {"fixture": None, "random": []}
    connected, kept = R.reference_graph(ref, R.fixture_board())
    out["fixture"] = {"connected": [list(p) for p in connected], "kept": kept}
    for seed in R.RANDOM_BOARD_SEEDS:
        connected, kept = R.reference_graph(ref, R.random_board(seed))
        out["random"].append({"seed": seed, "connected": [list(p) for p in connected], "kept": kept})
    path = os.path.join(HERE, "connectivity_boards.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

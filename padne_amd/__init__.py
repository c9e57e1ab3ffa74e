"""padne_amd: MI355X-native implementation of the padne solver hot path.

``padne_amd.solver`` mirrors ``padne.solver`` (assemble + solve + post-process); the arithmetic runs in
hand-written HIP kernels for gfx950 behind the C ABI of ``include/padne_hip.h``.
"""
from . import mesh, problem  # noqa: F401
from .gridmesh import GridMesher, Polygon  # noqa: F401

__all__ = ["mesh", "problem", "solver", "synthetic", "structured", "reduction", "distributed", "gridmesh", "GridMesher", "Polygon",
           "compute_connectivity", "filter_dead_networks", "prepare_board"]
__version__ = "0.1.0"

_FROM_SOLVER = ("compute_connectivity", "filter_dead_networks", "prepare_board")


def __getattr__(name):
    # the connectivity pre-pass lives in the solver module, which is imported on first use like ``padne_amd.solver`` itself
    if name in _FROM_SOLVER:
        from . import solver
        return getattr(solver, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

"""MI355X drop-in for the hot path of ``padne/solver.py``.

Same public names, argument meaning and error behaviour as the reference
(``solver.py:24-52, 171-229, 350-615, 671-902``); the arithmetic runs in
``libpadne_hip.so``:

=====================================  ====================================================
reference (file:line)                  here
=====================================  ====================================================
HalfEdge.cotan  mesh.py:124-139        ``asm_fill_tri`` kernel (per triangle, once)
laplace_operator  solver.py:171-213    ``padne_assemble_system`` (sigma = 1, no stamps)
process_mesh_laplace_operators :563    ``padne_assemble_system`` (all meshes in one launch)
stamp_network_into_system :469-541     host emits COO stamps in element order; the device
setup_ground_node :544-560             merges them after the mesh terms, in stamp order
solve_system :767-780 (SuperLU)        reduction to SPD (reduction.py) + Jacobi-PCG kernels,
                                       multipliers recovered from device residual products
compute_connectivity :245-260          ``prepare_board`` / ``solve(..., prune=True)``: ``polygons_locate_kernel`` finds the
filter_dead_networks :618-668          polygons every connection touches, the graph over them runs on the host
produce_layer_solutions :578-615       numpy slice per mesh (contiguous blocks) + power kernel
compute_power_density :728-745         ``power_density_kernel``
(several load cases of one board)      ``solve_load_cases``: one assembly and plan, one block solve, the block's
                                       power densities from the potentials on the device
(where a voltage drop comes from)      ``solve_sensitivities``: adjoints on the load-case block, Woodbury for
                                       regulators, ``sensitivity_block_kernel`` over the faces
(where the current goes)               ``solve_currents``: the load-case block with one column, ``current_cases_face_kernel``
                                       and ``current_cases_cut_kernel`` over the faces, element flows from V's rows
(what if a via cracks open)            ``solve_element_cases``: the load-case block plus one unit-current column per changed
                                       resistor, Woodbury on the host, ``combine_block_kernel`` forms the cases' potentials
(how far the mesh is from the board)   ``solve_error``: the same block, gradient recovery through vertex -> faces lists
                                       (``error_recover_kernel``) and ``error_indicator_kernel`` over the faces
(a finer mesh where that asks)         ``refine_meshes`` / ``solve_adaptive``: longest-edge refinement with conforming
                                       closure, edges by a sort of corner keys, ``refine_emit_kernel`` over the faces
(how hot that makes the copper)        ``solve_thermal``: the load-case block, then ``thermal_face_power_kernel``, the gather
                                       ``thermal_load_kernel`` and one more block solve on the thermal sheet operator
(and how fast)                         ``solve_thermal_transient``: backward-Euler steps on S = A + C/dt from the previous state,
                                       ``transient_rhs_kernel`` and ``transient_report_kernel`` per step, one hierarchy per dt
read-out under the cursor ui.py:192    ``FieldSampler``: owner face by ``sample_kernel`` over a grid of bins per layer,
                                       V interpolated in the face, J and p of the face
thermal image (no counterpart)         ``TemperatureSampler``: the same owner, found once per query by
                                       ``sample_fields_kernel``, then every field of a block read out at it
=====================================  ====================================================

There is no CPU fallback: every entry point that computes raises
``_hip.HipUnavailableError`` when the library or the GPU is missing.
"""
from __future__ import annotations

import contextlib
import dataclasses
import logging
import math
import threading
import time
import types
import warnings
from collections.abc import Mapping
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np
import scipy.sparse as sp
import scipy.spatial

from . import _hip, mesh, problem
from .reduction import (Constraint, KKTLayout, Reduction, SingularSystemError, build_block_reduction, build_reduction,
                        floating_component_pins, infer_layout, recover_currents)

log = logging.getLogger(__name__)

DTYPE = np.float64

# tolerance of the iterative solve: ||b - A y|| <= RTOL * ||b||   
RTOL = 1e-12
MAX_ITER = 200000

_default = threading.local()        # one context per host thread: a context (stream, pools) is not shared between threads


def get_context() -> _hip.Context:
    """Device context of the calling thread (GPU 0 unless ``set_context`` was called in this thread)."""
    ctx = getattr(_default, "ctx", None)
    if ctx is None:
        ctx = _default.ctx = _hip.Context(0)
    return ctx


def set_context(ctx: Optional[_hip.Context]) -> None:
    _default.ctx = ctx


NEAREST_ON_DEVICE_FROM = 50000     # vertices of a layer from which connections are snapped on the device


def _offsets(sizes) -> np.ndarray:
    """[0, s0, s0 + s1, ...]: where each of consecutive blocks of the given sizes starts, and the total."""
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


class SolverWarning(Warning):
    """Non-fatal oddity of the problem (e.g. non-zero ground current), ``solver.py:24-30``."""


@dataclass(frozen=True)
class SolverInfo:
    ground_node_current: float   # ~0 for a well-posed problem
    residual_norm: float         # ||L v - r||_2 on the ORIGINAL (un-reduced) system
    # extras (not in the reference; default so positional construction stays compatible)
    iterations: int = 0
    rel_residual: float = 0.0
    solve_seconds: float = 0.0
    # a block r of shape (N, k): ||L v_j - r_j||_2 per column (ground_node_current is then V[-1], residual_norm the
    # Frobenius norm ||L V - R||_F); None for a single right-hand side
    residual_norms: Optional[np.ndarray] = None


@dataclass
class LayerSolution:
    meshes: list
    potentials: list
    power_densities: list = field(default_factory=list)
    disconnected_meshes: list = field(default_factory=list)


@dataclass
class Solution:
    problem: problem.Problem
    layer_solutions: list
    solver_info: SolverInfo


# --------------------------------------------------------------------------------------------
# index bookkeeping (host): VertexIndexer, NodeIndexer
# --------------------------------------------------------------------------------------------


class VertexIndexer:
    """Global numbering: one contiguous block per mesh, in mesh order (``solver.py:216-229``).

    The reference materialises a list and a dict with one entry per vertex; here the numbering
    is the offset table, and the two containers are built lazily for code that indexes them.
    """

    def __init__(self, sizes: Sequence[int] = ()):
        self.offsets = _offsets(np.asarray(list(sizes), dtype=np.int64))
        self._g2v = None
        self._v2g = None

    @classmethod
    def create(cls, meshes) -> "VertexIndexer":
        return cls([len(m.vertices) for m in meshes])

    def __len__(self) -> int:
        return int(self.offsets[-1])

    def global_index(self, mesh_idx: int, vertex_idx: int) -> int:
        return int(self.offsets[mesh_idx] + vertex_idx)

    @property
    def global_index_to_vertex_index(self) -> list:
        if self._g2v is None:
            self._g2v = [(m, v) for m in range(len(self.offsets) - 1)
                         for v in range(int(self.offsets[m + 1] - self.offsets[m]))]
        return self._g2v

    @property
    def mesh_vertex_index_to_global_index(self) -> dict:
        if self._v2g is None:
            self._v2g = {mv: g for g, mv in enumerate(self.global_index_to_vertex_index)}
        return self._v2g


@dataclass
class NodeIndexer:
    node_to_global_index: dict = field(default_factory=dict)
    extra_source_to_global_index: dict = field(default_factory=dict)
    internal_node_count: int = 0

    @classmethod
    def create(cls, prob, meshes, mesh_index_to_layer_index, vindex: VertexIndexer,
               filtered_networks) -> "NodeIndexer":
        """``solver.py:398-466``: snap connections to the nearest vertex of their layer, then number
        internal nodes and one current unknown per voltage source / regulator."""
        points = {}
        gidx = {}
        for layer_i in range(len(prob.layers)):
            blocks, ids = [], []
            for mesh_i, msh in enumerate(meshes):
                if mesh_index_to_layer_index[mesh_i] != layer_i or len(msh.vertices) == 0:
                    continue
                blocks.append(msh.points)
                ids.append(np.arange(len(msh.points), dtype=np.int64) + vindex.offsets[mesh_i])
            if not blocks:
                continue
            points[layer_i] = np.concatenate(blocks)
            gidx[layer_i] = np.concatenate(ids)
        # all connections of a layer are snapped together: small layers through a KD-tree exactly like the
        # reference (solver.py:356-396, leafsize=32, k=1); from NEAREST_ON_DEVICE_FROM vertices on, by brute force
        # on the device, where the tree build alone would cost more than the whole linear solve
        wanted = {}
        for network in filtered_networks:
            for conn in network.connections:
                wanted.setdefault(prob.layers.index(conn.layer), []).append((conn.point.x, conn.point.y))
        snapped = {}
        for layer_i, pts in wanted.items():
            q = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
            if len(points[layer_i]) >= NEAREST_ON_DEVICE_FROM:
                k, ties = get_context().nearest_vertex(points[layer_i], q, with_ties=True)
                tied = np.flatnonzero(ties > 1)
                if len(tied):
                    # several vertices at exactly the minimum distance (a connection midway between vertices of a regular
                    # grid): the reference takes whichever its KD-tree meets first (solver.py:389-392, 425).  Only then is
                    # the tree built, and only those queries go through it
                    _, kt = scipy.spatial.KDTree(points[layer_i], leafsize=32).query(q[tied], k=1)
                    k = np.array(k, dtype=np.int64)
                    k[tied] = kt
            else:
                _, k = scipy.spatial.KDTree(points[layer_i], leafsize=32).query(q, k=1)
            snapped[layer_i] = iter(np.asarray(k, dtype=np.int64))
        node_to_global = {}
        for network in filtered_networks:
            for conn in network.connections:
                layer_i = prob.layers.index(conn.layer)
                k = next(snapped[layer_i])
                g = int(gidx[layer_i][k])
                node = conn.node_id
                if node in node_to_global and node_to_global[node] != g:
                    raise ValueError("Duplicate connection vertices found, this should not happen.")
                node_to_global[node] = g
        i_at = len(vindex)
        internal = 0
        for network in filtered_networks:
            for node in network.nodes:
                if node not in node_to_global:
                    node_to_global[node] = i_at
                    i_at += 1
                    internal += 1
        extra = {}
        for network in filtered_networks:
            for elem in network.elements:
                if elem.extra_variable_count > 1:
                    raise NotImplementedError("Extra variable count > 1 not supported yet")
                for _ in range(elem.extra_variable_count):
                    extra[elem] = i_at
                    i_at += 1
        return cls(node_to_global_index=node_to_global, extra_source_to_global_index=extra,
                   internal_node_count=internal)


# --------------------------------------------------------------------------------------------
# stamps: the host only *lists* them; the device adds them up
# --------------------------------------------------------------------------------------------


class StampList:
    """Write-only stand-in for the reference's ``lil_matrix`` during stamping.

    ``L[i, j] += v`` style updates (``solver.py:475-538, 558-560``) are recorded as COO triples in
    the order they were issued; the device merge adds duplicates in that order.
    """

    def __init__(self, n: int):
        self.shape = (n, n)
        self.rows: list = []
        self.cols: list = []
        self.vals: list = []
        self.constraints: list = []          # filled by stamp_network_into_system / setup_ground_node

    def add(self, i: int, j: int, v: float) -> None:
        n = self.shape[0]
        if i < 0:
            i += n
        if j < 0:
            j += n
        self.rows.append(int(i))
        self.cols.append(int(j))
        self.vals.append(float(v))

    def arrays(self):
        return (np.asarray(self.rows, dtype=np.int64), np.asarray(self.cols, dtype=np.int64),
                np.asarray(self.vals, dtype=np.float64))


def _stamp(L, i, j, v):
    if isinstance(L, StampList):
        L.add(i, j, v)
    else:                       # any matrix with item assignment (e.g. a scipy lil_matrix)
        L[i, j] = L[i, j] + v


_ELEMENT_KINDS = ("Resistor", "CurrentSource", "VoltageSource", "VoltageRegulator")


def element_kind(element) -> Optional[str]:
    """Which of the reference's four lumped elements ``element`` is (``problem.py:98-171``), by class *name* along its
    MRO: the seam receives padne's own ``padne.problem`` objects, which are not instances of the
    classes in :mod:`padne_amd.problem`, so an ``isinstance`` test against those would reject every real problem."""
    for cls in type(element).__mro__:
        if cls.__name__ in _ELEMENT_KINDS:
            return cls.__name__
    return None


def stamp_network_into_system(network, node_indexer: NodeIndexer, L, r: np.ndarray) -> None:
    """MNA stamps of one network, same entries in the same order as ``solver.py:469-541``."""
    idx = node_indexer.node_to_global_index
    for element in network.elements:
        kind = element_kind(element)
        if kind == "Resistor":
            a, b = idx[element.a], idx[element.b]
            g = 1 / element.resistance
            _stamp(L, a, a, -g)
            _stamp(L, a, b, g)
            _stamp(L, b, b, -g)
            _stamp(L, b, a, g)
        elif kind == "CurrentSource":
            r[idx[element.f]] += element.current
            r[idx[element.t]] += -element.current
        elif kind == "VoltageSource":
            p, n = idx[element.p], idx[element.n]
            iv = node_indexer.extra_source_to_global_index[element]
            _stamp(L, iv, p, 1.0)
            _stamp(L, iv, n, -1.0)
            r[iv] = element.voltage
            _stamp(L, p, iv, 1.0)
            _stamp(L, n, iv, -1.0)
            if isinstance(L, StampList):
                L.constraints.append(Constraint(index=iv, p=p, n=n, value=float(element.voltage)))
        elif kind == "VoltageRegulator":
            vp, vn = idx[element.v_p], idx[element.v_n]
            sf, st = idx[element.s_f], idx[element.s_t]
            iv = node_indexer.extra_source_to_global_index[element]
            _stamp(L, iv, vp, 1.0)
            _stamp(L, iv, vn, -1.0)
            _stamp(L, vp, iv, 1.0)
            _stamp(L, vn, iv, -1.0)
            r[iv] += element.voltage
            _stamp(L, sf, iv, element.gain)
            _stamp(L, st, iv, -element.gain)
            if isinstance(L, StampList):
                gamma: dict = {}
                gamma[sf] = gamma.get(sf, 0.0) + element.gain
                gamma[st] = gamma.get(st, 0.0) - element.gain
                L.constraints.append(Constraint(index=iv, p=vp, n=vn, value=float(element.voltage),
                                                gamma={k: v for k, v in gamma.items() if v != 0.0}))
        else:
            raise NotImplementedError(f"Unsupported node type {element}")


def setup_ground_node(i_gnd: int, L, r: np.ndarray) -> None:
    """``solver.py:544-560``: last row/column = ground-current unknown."""
    _stamp(L, -1, i_gnd, 1.0)
    _stamp(L, i_gnd, -1, 1.0)
    r[-1] = 0
    if isinstance(L, StampList):
        L.constraints.append(Constraint(index=L.shape[0] - 1, p=int(i_gnd), n=-1, value=0.0))


def find_best_ground_node_index(prob, node_indexer: NodeIndexer) -> int:
    """``solver.py:671-686``: the ``n`` terminal of the highest-voltage source, else unknown 0."""
    best, ground = float("-inf"), 0
    for network in prob.networks:
        for element in network.elements:
            if element_kind(element) == "VoltageSource" and element.voltage > best:
                best = element.voltage
                ground = node_indexer.node_to_global_index[element.n]
    return ground


def allocate_system(vindex: VertexIndexer, node_indexer: NodeIndexer):
    """``solver.py:748-764``: N = vertices + internal nodes + extra currents + 1 (ground)."""
    N = len(vindex) + node_indexer.internal_node_count + len(node_indexer.extra_source_to_global_index) + 1
    log.info(f"System matrix size: {N}x{N} variables")
    return StampList(N), np.zeros(N, dtype=DTYPE)


# --------------------------------------------------------------------------------------------
# device-resident system matrix
# --------------------------------------------------------------------------------------------


class SystemMatrix:
    """The assembled ``L`` (reference layout and sign), resident on the GPU.

    Quacks enough like the ``lil_matrix`` the reference returns from ``assemble_system`` for the
    callers on the seam: ``shape``, ``tocsr()/tocsc()/tolil()/toarray()/todense()``, ``L[i, j]``,
    ``L @ v``.  Carries the KKT layout so that ``solve_system`` does not have to re-derive it.
    """

    def __init__(self, dev: _hip.CsrMatrix, layout: Optional[KKTLayout], xy=None, tri=None, mesh_offsets=None,
                 links=None):
        self.dev = dev
        self.layout = layout
        self.shape = dev.shape
        self._host = None
        # geometry of the mesh unknowns (optional): lets solve_system pick a cache-friendly internal ordering
        self.xy, self.tri, self.mesh_offsets = xy, tri, mesh_offsets
        # pairs of potentials coupled by lumped stamps (optional): lets solve_system find floating copper
        self.links = links
        self._plans = {}            # device plans of solve_system by the structure of the reduction (see there)

    @property
    def nnz(self) -> int:
        return self.dev.nnz

    def close(self):
        """Release the device memory of the system and of the solve plans kept with it."""
        for plan in self._plans.values():
            plan.close()
        self._plans.clear()
        self.dev.close()

    def tocsr(self):
        if self._host is None:
            self._host = self.dev.to_scipy()
        return self._host

    def tocsc(self):
        return self.tocsr().tocsc()

    def tolil(self):
        return self.tocsr().tolil()

    def tocoo(self):
        return self.tocsr().tocoo()

    def toarray(self):
        return self.tocsr().toarray()

    def todense(self):
        return self.tocsr().todense()

    def __getitem__(self, key):
        return self.tocsr()[key]

    def __matmul__(self, v):
        v = np.asarray(v, dtype=DTYPE)
        if v.ndim != 2:
            return self.dev.matvec(v)
        # a block (N, k): 8 columns per pass of the SpMM (the last pass zero-padded), each column bit-identical to L @ v_j
        if v.shape[0] != self.shape[1]:
            raise ValueError("dimension mismatch")
        out = np.empty((self.shape[0], v.shape[1]), dtype=DTYPE)
        for j in range(0, v.shape[1], 8):
            w = min(8, v.shape[1] - j)
            X = np.zeros((self.shape[1], 8), dtype=DTYPE)
            X[:, :w] = v[:, j:j + w]
            out[:, j:j + w] = self.dev.matmat8(X)[:, :w]
        return out


def _flatten_meshes(meshes, conductances):
    xy = np.concatenate([m.points for m in meshes]) if meshes else np.zeros((0, 2))
    tri = np.concatenate([m.triangles for m in meshes]) if meshes else np.zeros((0, 3), np.int32)
    mvo = _offsets([len(m.points) for m in meshes])
    mto = _offsets([len(m.triangles) for m in meshes])
    return xy, tri, mvo, mto, np.asarray(conductances, dtype=np.float64)


def laplace_operator(msh: mesh.Mesh) -> sp.coo_matrix:
    """Mesh-local cotangent Laplacian (``solver.py:171-213``), computed on the device."""
    ctx = get_context()
    n = len(msh.vertices)
    xy, tri, mvo, mto, sig = _flatten_meshes([msh], [1.0])
    empty = np.zeros(0, dtype=np.int64)
    dev = ctx.assemble_system(n, xy, tri, mvo, mto, sig, empty, empty, np.zeros(0))
    out = dev.to_scipy().tocoo()
    dev.close()
    return out


def process_mesh_laplace_operators(meshes, conductances, vindex: VertexIndexer, L) -> None:
    """``solver.py:563-575``.  With a StampList the mesh terms are not listed at all: the device
    assembles them straight from the triangles (see ``assemble_system``); this function exists for
    callers that stamp into a host matrix."""
    if isinstance(L, StampList):
        L.meshes = (list(meshes), list(conductances))
        return
    for mesh_i, (msh, conductance) in enumerate(zip(meshes, conductances)):
        L_msh = (conductance * laplace_operator(msh)).tocoo()
        off = int(vindex.offsets[mesh_i])
        for i, j, v in zip(L_msh.row, L_msh.col, L_msh.data):
            L[off + i, off + j] += v


def assemble_system(prob, meshes, mesh_index_to_layer_index, vindex: VertexIndexer, filtered_networks,
                    node_indexer: NodeIndexer):
    """``solver.py:783-812``: allocate, mesh Laplacians, network stamps, ground -> ``(L, r)``.

    ``L`` is a :class:`SystemMatrix` on the device (convertible with ``.tocsr()`` / ``.tolil()``)."""
    conductances, stamps, r, n_potential = _stamp_problem(prob, meshes, mesh_index_to_layer_index, vindex, filtered_networks,
                                                          node_indexer)
    return assemble_from_arrays(meshes, conductances, stamps, n_potential=n_potential), r


def _stamp_problem(prob, meshes, mesh_index_to_layer_index, vindex: VertexIndexer, filtered_networks, node_indexer: NodeIndexer):
    """What the Problem puts into the system besides the mesh terms: (conductance of each mesh, the network and ground stamps
    as a StampList, r, number of potential unknowns)."""
    conductances = [prob.layers[mesh_index_to_layer_index[i]].conductance for i in range(len(meshes))]
    stamps, r = allocate_system(vindex, node_indexer)
    for network in filtered_networks:
        stamp_network_into_system(network, node_indexer, stamps, r)
    setup_ground_node(find_best_ground_node_index(prob, node_indexer), stamps, r)
    return conductances, stamps, r, len(vindex) + node_indexer.internal_node_count


def assemble_from_arrays(meshes, conductances, stamps: StampList, n_potential: int) -> SystemMatrix:
    ctx = get_context()
    xy, tri, mvo, mto, sig = _flatten_meshes(meshes, conductances)
    rows, cols, vals = stamps.arrays()
    dev = ctx.assemble_system(stamps.shape[0], xy, tri, mvo, mto, sig, rows, cols, vals)
    layout = KKTLayout(size=stamps.shape[0], n_potential=n_potential, constraints=list(stamps.constraints))
    off = (rows < cols) & (cols < n_potential)
    links = np.unique(np.stack([rows[off], cols[off]], axis=1), axis=0) if off.any() else np.zeros((0, 2), np.int64)
    return SystemMatrix(dev, layout, xy=xy, tri=tri, mesh_offsets=mvo, links=links)


# --------------------------------------------------------------------------------------------
# solve
# --------------------------------------------------------------------------------------------


# The reference judges a solve by the ABSOLUTE residual of the whole system, ||L v - r||_2 < 1e-9
# (tests/test_solver.py:2083-2089).  The rows of the reduced system are rows of that system (the multiplier rows
# hold exactly by construction), so its residual is driven to a quarter of that bar whenever 1e-12 ||b|| is looser
# than that -- a voltage source across a copper plane puts kiloamperes into b.  Below RTOL_FLOOR nothing is gained:
# that is what evaluating b - A y in binary64 can resolve (the solve stops at that floor and reports what it reached).
# The rule itself is applied where ||b|| is known: on the device (padne_kkt_solve, abs_residual_target), and from the
# globally reduced norm in the row-partitioned path (distributed.solve_partitioned).
ABS_RESIDUAL_TARGET = 2.5e-10
RTOL_FLOOR = 2e-15


STALL_WARN_ABOVE = 1e-9


def _stalled(res, rtol: float) -> bool:
    return res.status != _hip.OK and not res.rel_residual <= max(rtol, STALL_WARN_ABOVE)


def _stalled_columns(residual_norms: np.ndarray, R: Optional[np.ndarray] = None, *,
                     col_norms: Optional[np.ndarray] = None) -> str:
    """Which columns of a block a stall is put down to.  The device reports the reduced solves of a block as a whole (one
    status, the largest relative residual), so this is an ATTRIBUTION, not a per-column status: the columns whose
    ||L v_j - r_j|| exceeds STALL_WARN_ABOVE ||r_j||, or, if none does, the one worst against its own right-hand side.
    Only called when the block stalled (an O(N k) pass over a dense R; ``col_norms`` = the ||r_j|| when R is not dense)."""
    if col_norms is None:
        col_norms = np.sqrt(np.einsum("ij,ij->j", R, R))
    rel = residual_norms / np.maximum(col_norms, 1e-300)
    cols = np.flatnonzero(rel > STALL_WARN_ABOVE)
    if not len(cols):
        cols = [int(np.argmax(rel))]
    return (f" (block of {len(residual_norms)} right-hand sides, reported as a whole; largest residuals against their own "
            f"right-hand side in column(s) {', '.join(str(int(j)) for j in cols[:16])})")


def _warn_if_block_stalled(res, residual_norms: np.ndarray, cols, vals, n_cols: int) -> None:
    """_warn_if_stalled for a block given by its triples: their ``cols`` and ``vals`` give the ||r_j|| that name the columns."""
    if _stalled(res, RTOL):
        col_norms = np.sqrt(np.bincount(cols, weights=vals * vals, minlength=n_cols))
        _warn_if_stalled(res, RTOL, _stalled_columns(residual_norms, col_norms=col_norms))


def _solver_info(res, ground, residual_norm, residual_norms=None) -> SolverInfo:
    """The SolverInfo of a device solve ``res`` (a SolveResult) with the figures the caller took from the solution."""
    return SolverInfo(ground_node_current=ground, residual_norm=float(residual_norm), iterations=int(res.iterations),
                      rel_residual=float(res.rel_residual), solve_seconds=float(res.seconds), residual_norms=residual_norms)


def _warn_if_stalled(res, rtol: float, where: str = "") -> None:
    """The reference's direct solve always returns *an* answer and reports its quality through
    SolverInfo.residual_norm; an iteration that stalls above the requested tolerance does the same, with a warning in
    the reference's own soft-failure style (solver.py:880-888) when the residual is worse than 1e-9 relative (matrices
    with entry ratios beyond 1e12, e.g. needle triangles).  A stall between the requested 1e-12 and 1e-9 is the
    rounding floor of evaluating b - A x for a system whose solution is large against its right-hand side (a layer
    held at hundreds of volts through a weak link: 1 of 1000 random systems of scripts/fuzz_parity.py, potentials
    still within 4e-11 of the direct solve); it is reported in SolverInfo.residual_norm and not warned about."""
    if _stalled(res, rtol):
        warnings.warn(f"iterative solve stopped at a relative residual of {res.rel_residual:.2e} "
                      f"(requested {rtol:.1e}) after {res.iterations} iterations{where}", SolverWarning)


def solve_system(L, r: np.ndarray, *, rtol: float = RTOL, reorder=None, n_potential: Optional[int] = None):
    """Solve ``L v = r`` and return ``(v, SolverInfo)`` like ``solver.py:767-780``.

    ``L`` is a :class:`SystemMatrix` from :func:`assemble_system`, or any scipy sparse matrix in the
    reference's layout (it is uploaded and its multiplier structure inferred; ``n_potential`` = number of
    potential unknowns in front of the multiplier block, if the caller knows it).  ``reorder``: None = solve in
    a band numbering when the mesh numbering is scattered (decided from the triangles), True / False = force.

    ``r`` may also be a block of shape (N, k), as ``spsolve`` accepts it: ``V`` (N, k) comes back, column j the solution
    for ``r[:, j]``, with ``ground_node_current = V[-1]``, ``residual_norm = ||L V - R||_F`` and the per-column norms in
    ``SolverInfo.residual_norms``.  The block is reduced once, its columns and the regulator columns go through one
    lockstep solve.  A C-ordered block crosses to the device as it is; any other order costs one host copy.  Shape
    (N, 1) is the single right-hand side ``r[:, 0]``: v of shape (N,).

    Copper that nothing ties to the ground node (the reference's matrix is singular there, its LU returns rounding
    noise for those potentials) is held at 0 V at one vertex; ``ground_node_current`` is, as in the reference, the net
    current injected into the grounded component (``tests/test_solver.py:1829-1833``: non-zero for an unterminated
    current loop).
    """
    r = np.asarray(r)
    if r.ndim > 2:
        raise ValueError(f"r must be a vector or an (N, k) block, not of shape {r.shape}")
    if r.ndim == 2:
        if r.shape[0] != L.shape[0]:
            raise ValueError(f"r has {r.shape[0]} rows, the system {L.shape[0]}")
        if r.shape[1] == 0:
            raise ValueError("r is a block of no right-hand sides")
        if r.shape[1] == 1:
            r = r[:, 0]
    block = r.ndim == 2
    ctx = get_context()
    r = np.ascontiguousarray(r, dtype=DTYPE)
    if isinstance(L, SystemMatrix):
        dev, layout = L.dev, L.layout
        owned = False
        Lc = None
    else:
        Lc = sp.csr_matrix(L)
        Lc.sum_duplicates()
        Lc.eliminate_zeros()
        Lc.sort_indices()
        dev, layout, owned = ctx.csr_from_scipy(Lc), None, True
        layout = infer_layout(Lc, r[:, 0] if block else r, n_potential)
    if layout is None or not layout.constraints:
        raise SingularSystemError("system has no ground constraint")
    if not block:
        # multiplier rows take their right-hand side from r (solver.py:505, 530, 560)
        for cst in layout.constraints:
            cst.value = float(r[cst.index])
    pins = _floating_pins(L, layout, Lc)
    # O(#constraints): what the reduction eliminates, ties and knows; the index map itself is made on the device.  A block
    # is reduced once: the structure is the same for every column, the known parts come per column
    if block:
        red, known_idx, known_val = build_block_reduction(layout, {cst.index: r[cst.index, :] for cst in layout.constraints},
                                                          pins)
    else:
        red: Reduction = build_reduction(layout, pins)
    plan = _plan_for(L, dev, layout, red, _wants_reorder(L, reorder), owned)
    try:
        members, extras = red.probe_members, red.regulator_columns
        if not block:
            probes, res = plan.solve(r, red.known, extras, members, rtol=rtol, max_iter=MAX_ITER,
                                     abs_residual_target=ABS_RESIDUAL_TARGET)
            _warn_if_stalled(res, rtol)
            i_reg, mult = recover_currents(red, members, probes, 1)
            v, residual_norm = plan.finish(i_reg[0], mult[0])
        else:
            k = r.shape[1]
            probes, res = plan.solve_block(r, known_idx, known_val, extras, members, rtol=rtol, max_iter=MAX_ITER,
                                           abs_residual_target=ABS_RESIDUAL_TARGET)
            v, residual_norms = _finish_block(plan, red, members, probes, k)
    finally:
        if owned:
            plan.close()
            dev.close()
    if not block:
        return v, _solver_info(res, float(v[-1]), residual_norm)
    if _stalled(res, rtol):
        _warn_if_stalled(res, rtol, _stalled_columns(residual_norms, r))
    return v, _solver_info(res, v[-1].copy(), np.sqrt(np.sum(residual_norms ** 2)), residual_norms)


def _floating_pins(L, layout: KKTLayout, Lc) -> list:
    """Unknowns that hold copper nothing ties to the ground node at 0 V (see solve_system)."""
    ground_p = layout.ground_constraint.p
    if Lc is not None:
        pins = floating_component_pins(layout.n_potential, ground_p, layout.constraints, matrix=Lc)
    elif L.links is not None and L.mesh_offsets is not None:
        pins = floating_component_pins(layout.n_potential, ground_p, layout.constraints,
                                       mesh_offsets=L.mesh_offsets, links=L.links)
    else:
        pins = []
    if pins:
        log.info(f"{len(pins)} floating component(s) held at 0 V at unknown(s) {pins[:8]}")
    return pins


def _wants_reorder(L, reorder) -> bool:
    want_reorder = False
    if isinstance(L, SystemMatrix) and L.xy is not None and reorder is not False:
        # CGAL numbers vertices in insertion order; when neighbours are far apart in the numbering the SpMV
        # gathers miss the caches, so the reduced system is solved in a band numbering by horizontal strips
        # (internal: v comes back unpermuted)
        from .reduction import ordering_is_scattered
        if reorder is True:
            want_reorder = True
        else:
            # (a property of the mesh, not of the right-hand side: looked at once per assembled system -- 4 ms of a 34 ms
            #  call at 20 M triangles otherwise)
            if getattr(L, "_scattered", None) is None:
                L._scattered = bool(ordering_is_scattered(L.tri, len(L.xy)))
            want_reorder = L._scattered
    return want_reorder


def _plan_for(L, dev, layout: KKTLayout, red: Reduction, want_reorder: bool, owned: bool) -> _hip.KktPlan:
    """The device plan of ``red`` on ``L``: the one kept with an assembled system when its structure matches, else a new one
    (kept with the system in its place)."""
    # the plan -- index map, A = -P^T L P and its multigrid hierarchy on the device -- depends on the STRUCTURE of the
    # reduction only (the values of the sources enter through c and r): kept with the assembled system, so a second
    # right-hand side on the same system finds everything in place, like a second solve with a kept factorisation
    key = (red.elim.tobytes(), tuple(red.tied), bool(want_reorder))
    plan = L._plans.get(key) if isinstance(L, SystemMatrix) else None
    if plan is None:
        try:
            if want_reorder:
                # the strip numbering is made on the device from the mesh that was assembled (padne_kkt_create, flags bit 0);
                # key fields that do not fit (65535 meshes / strips) fall back to the host's sort of the same keys -- on THAT
                # refusal only: any other invalid argument is the caller's error and is raised as it is
                try:
                    plan = _hip.KktPlan(dev, layout.n_potential, red.elim, red.tied, red.n_free, strip_order=True)
                except ValueError as exc:
                    if "the host orders this system" not in str(exc) and "beyond the key fields" not in str(exc):
                        raise
                    from .reduction import apply_locality_ordering
                    apply_locality_ordering(red, L.xy, L.mesh_offsets)
                    plan = _hip.KktPlan(dev, layout.n_potential, red.elim, red.tied, red.n_free, index_map=red.index_map)
            else:
                plan = _hip.KktPlan(dev, layout.n_potential, red.elim, red.tied, red.n_free)
        except BaseException:
            if owned:                                 # a scipy matrix uploaded for this call: it must not outlive a failed plan
                dev.close()
            raise
        if isinstance(L, SystemMatrix):
            for old in L._plans.values():             # one structure at a time: a plan holds GBs at N = 10 M
                old.close()
            L._plans.clear()
            L._plans[key] = plan
    return plan


def _finish_block(plan: _hip.KktPlan, red: Reduction, members, probes, k: int):
    """Stage 2 of a block: the multiplier currents of every column from its probe rows, then (V, ||L v_j - r_j||)."""
    i_reg, mult = recover_currents(red, members, probes, k)
    mult_idx = np.asarray(sorted(mult[0]), dtype=np.int64)
    mult_val = np.array([[m[int(i)] for i in mult_idx] for m in mult], dtype=DTYPE).reshape(k, len(mult_idx))
    return plan.finish_block(i_reg, mult_idx, mult_val)


# --------------------------------------------------------------------------------------------
# post-processing
# --------------------------------------------------------------------------------------------


def compute_triangle_gradient(vertices, values) -> mesh.Vector:
    """Gradient of the linear interpolant on one triangle (``solver.py:689-725``), on the device."""
    if len(vertices) != 3 or len(values) != 3:
        raise ValueError("Vertices and values must be of length 3 for a triangle")
    ctx = get_context()
    # the kernel visits a face as (tri[2], tri[0], tri[1]); feed (v2, v3, v1) so it sees (v1, v2, v3)
    v1, v2, v3 = vertices
    xy = np.array([[v2.p.x, v2.p.y], [v3.p.x, v3.p.y], [v1.p.x, v1.p.y]], dtype=DTYPE)
    pot = np.array([values[1], values[2], values[0]], dtype=DTYPE)
    gx, gy = ctx_face_gradient(ctx, xy, np.array([[0, 1, 2]], np.int32), pot)
    return mesh.Vector(float(gx[0]), float(gy[0]))


def ctx_face_gradient(ctx, xy, tri, pot):
    one = np.array([0, len(xy)], dtype=np.int64)
    onet = np.array([0, len(tri)], dtype=np.int64)
    return ctx.face_gradient(xy, tri, one, onet, pot)


def ctx_error_estimate(ctx, xy, tri, conductance: float, pot):
    """The gradient-recovery error estimate of ``pot`` on one mesh of sheet conductance ``conductance``
    (``Context.error_estimate``): (G, eta, sum eta^2, sum sigma A |g|^2, the largest eta, its face)."""
    one = np.array([0, len(xy)], dtype=np.int64)
    onet = np.array([0, len(tri)], dtype=np.int64)
    G, eta, E, P, top, face = ctx.error_estimate(xy, tri, one, onet, [conductance], pot)
    return G, eta, float(E[0]), float(P[0]), float(top[0]), int(face[0])


def compute_power_density(voltage: mesh.ZeroForm, conductivity: float) -> mesh.TwoForm:
    """Per-face ``sigma |grad V|^2`` (``solver.py:728-745``)."""
    ctx = get_context()
    msh = voltage.mesh
    out = mesh.TwoForm(msh)
    if len(msh.triangles):
        xy, tri, mvo, mto, sig = _flatten_meshes([msh], [conductivity])
        out.values = ctx.power_density(xy, tri, mvo, mto, sig, voltage.values)
    return out


def _layer_meshes(meshes, mesh_index_to_layer_index, tri_offsets, layer_i: int):
    """The meshes of layer ``layer_i`` in mesh order, each as (mesh index, mesh, lo, hi): its faces are lo:hi of the per-face
    arrays over all meshes (``tri_offsets`` = _offsets of the meshes' face counts)."""
    for mesh_i, msh in enumerate(meshes):
        if mesh_index_to_layer_index[mesh_i] == layer_i:
            yield mesh_i, msh, int(tri_offsets[mesh_i]), int(tri_offsets[mesh_i + 1])


def produce_layer_solutions(layers, vindex: VertexIndexer, meshes, mesh_index_to_layer_index, v: np.ndarray,
                            disconnected_meshes_by_layer, system: Optional["SystemMatrix"] = None,
                            power_all: Optional[np.ndarray] = None) -> list:
    """``solver.py:578-615``.  Each mesh's unknowns are one contiguous block of ``v``, so the scatter
    is a slice; the power densities of all meshes come from one kernel launch.  ``power_all``: the per-face power
    densities of all meshes in mesh order when the caller has them already (one case of a block of load cases)."""
    ctx = get_context()
    sig = [layers[mesh_index_to_layer_index[i]].conductance for i in range(len(meshes))]
    n_tri = sum(len(m.triangles) for m in meshes)
    if power_all is None and meshes and n_tri:
        if system is not None and system.tri is not None and len(system.tri) == n_tri:
            # the system was assembled from these meshes: they are still on the device, only the potentials travel
            power_all = system.dev.power_density(v[:len(vindex)], n_tri)
        else:
            xy, tri, mvo, mto, sg = _flatten_meshes(meshes, sig)
            power_all = ctx.power_density(xy, tri, mvo, mto, sg, v[:len(vindex)])
    toff = _offsets([len(m.triangles) for m in meshes])
    out = []
    for layer_i, _layer in enumerate(layers):
        sol = LayerSolution(meshes=[], potentials=[], power_densities=[],
                            disconnected_meshes=disconnected_meshes_by_layer[layer_i])
        for mesh_i, msh, lo, hi in _layer_meshes(meshes, mesh_index_to_layer_index, toff, layer_i):
            zf = mesh.ZeroForm(msh)
            zf.values = np.array(v[vindex.offsets[mesh_i]:vindex.offsets[mesh_i + 1]], dtype=DTYPE)
            tf = mesh.TwoForm(msh)
            if power_all is not None:
                tf.values = np.array(power_all[lo:hi], dtype=DTYPE)
            sol.meshes.append(msh)
            sol.potentials.append(zf)
            sol.power_densities.append(tf)
        out.append(sol)
    return out


# --------------------------------------------------------------------------------------------
# orchestration
# --------------------------------------------------------------------------------------------


def _solve_partitioned(prob, meshes, mesh_index_to_layer_index, vindex, filtered_networks, node_indexer, partition,
                       ctx):
    """The solve of ``solve_meshed`` with the rows dealt to several GPUs (``distributed.py``): every rank lists the
    same stamps, assembles and solves its own rows, and all ranks end up with all potentials."""
    from . import distributed
    conductances, stamps, r, n_pot = _stamp_problem(prob, meshes, mesh_index_to_layer_index, vindex, filtered_networks,
                                                    node_indexer)
    plan = distributed.build_problem_partition(meshes, conductances, list(mesh_index_to_layer_index), stamps, r, n_pot,
                                               partition.rank, partition.world)
    v_pot, res = distributed.solve_partitioned(plan, ctx, dist=partition.dist, team=partition.team, rtol=RTOL,
                                               gather=partition.gather)
    v = np.zeros(stamps.shape[0], dtype=DTYPE)
    if plan.reduction is not None:
        # sources or regulators: the whole solution vector came back -- potentials and the multiplier currents recovered
        # from the residual rows of the source-tied unknowns (distributed.solve_partitioned)
        v[:] = v_pot[:len(v)]
    else:
        v[:n_pot] = v_pot[:n_pot]
        # KCL over all potential rows: the mesh and resistor terms cancel, what is left is the ground current (row of
        # solver.py:558-560) = the net current the sources inject
        v[-1] = float(np.sum(r[:n_pot]))
    return v, _solver_info(res, float(v[-1]), res.abs_residual)


def _warn_ground_current(current: float, where: str = "") -> None:
    """The reference's soft failure for a ground current away from zero (solver.py:880-888)."""
    if not np.isclose(current, 0):
        warnings.warn(
            f"{where}Ground node current is not zero ({current} A), this may indicate an issue "
            "with the problem being solved. Check for unterminated current loops or floating connected "
            "components. This may be harmless if the current is small, but it may indicate an "
            "ill-conditioned system.", SolverWarning)


@dataclass
class IndexedBoard:
    """A meshed Problem with its unknowns numbered: what every ``solve_meshed*`` entry point starts from."""
    prob: object
    meshes: list                           # as mesh.Mesh
    layer_of: list                         # mesh_index_to_layer_index
    filtered_networks: list
    disconnected_meshes_by_layer: list
    vindex: VertexIndexer
    node_indexer: NodeIndexer
    tri_offsets: np.ndarray                # where each mesh's faces start in the per-face arrays over all meshes

    def layer_meshes(self, layer_i: int):
        """(mesh index, mesh, lo, hi) of every mesh of the layer (_layer_meshes)."""
        return _layer_meshes(self.meshes, self.layer_of, self.tri_offsets, layer_i)

    @contextlib.contextmanager
    def assembled(self):
        """``assemble_system`` of the board as a context: (L on the device, r) inside, L closed on the way out."""
        log.info("Assembling the global system")
        L, r = assemble_system(self.prob, self.meshes, self.layer_of, self.vindex, self.filtered_networks, self.node_indexer)
        try:
            yield L, r
        finally:
            L.close()


def index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks=None,
                disconnected_meshes_by_layer=None) -> IndexedBoard:
    """The :class:`IndexedBoard` of solve_meshed's arguments: their defaults filled in, the meshes as :class:`mesh.Mesh`, the
    connections snapped to vertices and the unknowns numbered."""
    meshes = [m if isinstance(m, mesh.Mesh) else mesh.Mesh.from_reference(m) for m in meshes]
    if filtered_networks is None:
        filtered_networks = list(prob.networks)
    if disconnected_meshes_by_layer is None:
        disconnected_meshes_by_layer = [[] for _ in prob.layers]
    log.info("Indexing vertices and connections")
    vindex = VertexIndexer.create(meshes)
    node_indexer = NodeIndexer.create(prob, meshes, mesh_index_to_layer_index, vindex, filtered_networks)
    return IndexedBoard(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer, vindex,
                        node_indexer, _offsets([len(m.triangles) for m in meshes]))


def _refuse_partition(partition, what: str) -> None:
    """The block features run on one GPU: ValueError for a ``partition`` over several."""
    if partition is not None and partition.world > 1:
        raise ValueError(f"{what} are solved on one GPU: the row-partitioned path (partition.world > 1) does not take them")


class _Laps:
    """The host time of consecutive steps of an entry point, written into its ``timings`` dict (None: nothing is kept)."""

    def __init__(self, timings: Optional[dict]):
        self.timings, self.since = timings, time.perf_counter()

    def lap(self, key: Optional[str] = None) -> None:
        """The time since the last lap goes under ``key`` (None: to nobody), and the next lap starts."""
        now = time.perf_counter()
        if key is not None and self.timings is not None:
            self.timings[key] = now - self.since
        self.since = now


def solve_meshed(prob, meshes, mesh_index_to_layer_index, *, filtered_networks=None,
                 disconnected_meshes_by_layer=None, partition=None) -> Solution:
    """Steps 4-11 of the reference's ``solve()`` (``solver.py:846-902``): everything after meshing.

    ``partition``: a :class:`padne_amd.distributed.Partition` -- the rows are dealt to the GPUs of the node (by layer, or
    by strips of layers when there are fewer layers than GPUs); every rank calls this with the same Problem and gets the
    same Solution."""
    board = index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer)
    if partition is not None and partition.world > 1:
        ctx = get_context()
        v, solver_info = _solve_partitioned(prob, board.meshes, mesh_index_to_layer_index, board.vindex, board.filtered_networks,
                                            board.node_indexer, partition, ctx)
        _warn_ground_current(solver_info.ground_node_current)
        layer_solutions = produce_layer_solutions(prob.layers, board.vindex, board.meshes, mesh_index_to_layer_index, v,
                                                  board.disconnected_meshes_by_layer)
        return Solution(problem=prob, layer_solutions=layer_solutions, solver_info=solver_info)
    with board.assembled() as (L, r):
        log.info("Solving the system of equations")
        v, solver_info = solve_system(L, r)
        _warn_ground_current(solver_info.ground_node_current)
        log.info("Producing the solution object")
        # the mesh is still on the device with the assembled system: the power densities need only the potentials
        layer_solutions = produce_layer_solutions(prob.layers, board.vindex, board.meshes, mesh_index_to_layer_index, v,
                                                  board.disconnected_meshes_by_layer, system=L)
    return Solution(problem=prob, layer_solutions=layer_solutions, solver_info=solver_info)


def solve(prob, mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None, partition=None, prune=False) -> Solution:
    """``padne.solver.solve`` (``solver.py:815-902``).

    CGAL meshing is out of scope.  ``mesher`` must offer ``poly_to_mesh(polygon, seed_points) -> Mesh``
    (padne's own ``mesh.Mesher`` does, and so does :class:`padne_amd.structured.StructuredMesher` for
    rectangles and annuli, and :class:`padne_amd.gridmesh.GridMesher` for polygons with holes, on the
    device).  By default every polygon of every layer is meshed and treated as connected
    (:func:`mesh_problem`).  ``prune=True`` runs the reference's chain instead -- connectivity prune,
    mesh, index, assemble, solve: :func:`prepare_board` finds on the device (one GPU) the copper a
    driven network reaches, only that is meshed, and the networks on dead copper are left out.  The
    other ``solve_*`` wrappers take the same keyword.
    """
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed(prob, meshes, mesh_index_to_layer_index, partition=partition, **pruned)


def mesh_problem(prob, mesher_config=None, mesher=None):
    """Steps 1-3 of the reference's ``solve()``: every polygon of every layer meshed, with the connections of its layer as
    seeds.  Returns (meshes, mesh_index_to_layer_index)."""
    if mesher is None:
        mesher = mesh.Mesher(mesher_config)
    meshes, mesh_index_to_layer_index = [], []
    log.info("Meshing the connected components")
    for layer_i, layer in enumerate(prob.layers):
        seeds = [mesh.Point(c.point.x, c.point.y) for net in prob.networks for c in net.connections
                 if c.layer is layer or c.layer == layer]
        geoms = list(layer.geoms)
        if hasattr(mesher, "polys_to_meshes"):          # a mesher that takes a batch: one call per layer
            meshes.extend(mesher.polys_to_meshes(geoms, seeds))
        else:
            meshes.extend(mesher.poly_to_mesh(geom, seeds) for geom in geoms)
        mesh_index_to_layer_index.extend([layer_i] * len(geoms))
    return meshes, mesh_index_to_layer_index


# --------------------------------------------------------------------------------------------
# connectivity pre-pass: which copper does a driven network reach (DESIGN.md "Connectivity pre-pass")
# --------------------------------------------------------------------------------------------

@dataclass
class BoardConnectivity:
    """What :func:`compute_connectivity` found.  ``hits[n][c]``: the ``(geom_i, kind)`` of every polygon of its layer that
    connection c of network n touches, in ascending geom_i; kind 1 inside, 2 on the boundary.  ``connected`` and ``roots``:
    sets of ``(layer_i, geom_i)``.  ``unplaced``: the ``(network_i, connection_i)`` that touch no polygon."""
    hits: list
    connected: set
    roots: set
    unplaced: list


@dataclass
class PreparedBoard:
    """What :func:`prepare_board` hands to ``solve_meshed*``.  ``skipped``: ``(layer_i, geom_i, reason)`` of the dead polygons
    that got no display mesh."""
    meshes: list
    mesh_index_to_layer_index: list
    filtered_networks: list
    disconnected_meshes_by_layer: list
    connectivity: BoardConnectivity
    skipped: list


def _device_locate(polygons, groups, points, point_groups):
    return _hip.locate_polygons(get_context(), polygons, groups, points, point_groups)


def compute_connectivity(prob, *, locate=None) -> BoardConnectivity:
    """The reference's ``compute_connectivity`` (``solver.py:84-148, 232-260``) without shapely: one locate call for the
    whole board -- all layers' polygons, all networks' connections -- and the graph on the host.

    A node per (layer, geom); per network the polygons any of its connections touches (shapely's ``intersects``: inside or
    on the boundary), all of them roots when the network has a source, all of them joined; connected is what can be
    reached from a root.  Copper is joined through networks only, never by geometric contact.  ``locate``: the engine
    ``(polygons, groups, points, point_groups) -> (hit_ptr, hit_poly, hit_kind)``, ``_hip.locate_polygons`` on the device
    by default (one GPU); the rule is stated in ``include/padne_hip.h``.  The boundary test is exact and has no tolerance:
    a point computed onto a slanted edge counts as inside or outside by parity.  The geoms are what
    ``gridmesh.rings_of`` takes: a ``structured.Rect`` or anything with ``.exterior.coords`` and ``.interiors``."""
    from . import gridmesh
    if locate is None:
        locate = _device_locate
    polygons, groups, first = [], [], [0]
    for layer_i, layer in enumerate(prob.layers):
        polygons.extend(gridmesh.rings_of(geom) for geom in layer.geoms)
        groups.extend([layer_i] * len(layer.geoms))
        first.append(len(polygons))
    points, point_groups = [], []
    for network in prob.networks:
        for conn in network.connections:
            points.append((float(conn.point.x), float(conn.point.y)))
            point_groups.append(prob.layers.index(conn.layer))
    hit_ptr, hit_poly, hit_kind = locate(polygons, np.array(groups, dtype=np.int32), np.array(points, dtype=np.float64).reshape(-1, 2),
                                         np.array(point_groups, dtype=np.int32))
    # union-find over the polygons of the batch
    parent = list(range(len(polygons)))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    hits, unplaced, root_polys, touched = [], [], set(), set()
    q = 0
    for network_i, network in enumerate(prob.networks):
        of_network, members = [], []
        for conn_i in range(len(network.connections)):
            lo, hi = int(hit_ptr[q]), int(hit_ptr[q + 1])
            base = first[point_groups[q]]
            of_network.append([(int(hit_poly[k]) - base, int(hit_kind[k])) for k in range(lo, hi)])
            members.extend(int(hit_poly[k]) for k in range(lo, hi))
            if lo == hi:
                unplaced.append((network_i, conn_i))
            q += 1
        hits.append(of_network)
        touched.update(members)
        if network.has_source:
            root_polys.update(members)
        for other in members[1:]:
            parent[find(other)] = find(members[0])
    live = {find(p) for p in root_polys}
    layer_of_poly = np.searchsorted(np.asarray(first), np.arange(len(polygons)), side="right") - 1

    def pair(p):
        return int(layer_of_poly[p]), p - first[int(layer_of_poly[p])]

    return BoardConnectivity(hits=hits, connected={pair(p) for p in touched if find(p) in live},
                             roots={pair(p) for p in root_polys}, unplaced=unplaced)


def filter_dead_networks(prob, connectivity: BoardConnectivity) -> list:
    """The reference's ``filter_dead_networks`` (``solver.py:618-668``): the networks of ``prob`` none of whose connections
    touches a polygon that is not connected.  A network with an unplaced connection stays, as in the reference."""
    kept = []
    for network, of_network in zip(prob.networks, connectivity.hits):
        dead = any((prob.layers.index(conn.layer), geom_i) not in connectivity.connected
                   for conn, of_conn in zip(network.connections, of_network) for geom_i, _kind in of_conn)
        if not dead:
            kept.append(network)
    return kept


def _display_meshes(mesher, layer_i: int, geoms, dead, skipped: list) -> list:
    """Meshes of the dead polygons ``dead`` (geom indices) of a layer, for display; those that cannot be meshed go to
    ``skipped``.  The batch first; where it raises, one polygon at a time."""
    if hasattr(mesher, "crumbs"):
        import copy
        mesher = copy.copy(mesher)
        mesher.crumbs = "drop"
    made = None
    if hasattr(mesher, "polys_to_meshes"):
        try:
            made = list(mesher.polys_to_meshes([geoms[g] for g in dead], []))
        except mesh.MeshingException:
            made = None
    out = []
    for k, g in enumerate(dead):
        try:
            m = made[k] if made is not None else mesher.poly_to_mesh(geoms[g], [])
        except mesh.MeshingException as exc:
            skipped.append((layer_i, g, str(exc)))
            continue
        if hasattr(m, "triangles") and len(m.triangles) == 0:
            skipped.append((layer_i, g, "the mesh has no face"))
            continue
        out.append(m)
    return out


def prepare_board(prob, mesher_config=None, *, mesher=None, disconnected="skip", locate=None) -> PreparedBoard:
    """Steps 1-3 of the reference's ``solve()`` with its connectivity pre-pass (``solver.py:245-330, 815-845``): only the
    polygons a driven network reaches are meshed, in (layer, geom) order, and the networks on dead copper are dropped.

    The seeds of a polygon are the connections that lie inside it (kind 1); a connection on its boundary is not a seed, as
    in the reference.  A mesher that takes a batch (``polys_to_meshes``) gets a layer's connected polygons and their seeds in
    one call, any other ``poly_to_mesh(geom, seeds of that geom)``.  A kept network with a connection on a layer that ends up
    without a mesh is a ValueError.  ``disconnected``: ``"skip"`` leaves ``disconnected_meshes_by_layer`` empty; ``"mesh"``
    meshes the dead polygons with the same mesher for display (a GridMesher with ``crumbs="drop"``) and lists those that
    yield no face or raise MeshingException in ``skipped``.  The reference meshes them by a constrained triangulation with a
    ``RELAXED`` config, which has no counterpart here.  ``locate``: see :func:`compute_connectivity`."""
    if disconnected not in ("skip", "mesh"):
        raise ValueError(f"disconnected must be 'skip' or 'mesh', got {disconnected!r}")
    if mesher is None:
        mesher = mesh.Mesher(mesher_config)
    connectivity = compute_connectivity(prob, locate=locate)
    kept = filter_dead_networks(prob, connectivity)
    meshed_layers = {layer_i for layer_i, _geom_i in connectivity.connected}
    for network in kept:
        for conn in network.connections:
            layer_i = prob.layers.index(conn.layer)
            if layer_i not in meshed_layers:
                raise ValueError(f"a connection at ({conn.point.x:g}, {conn.point.y:g}) lies on layer {layer_i} "
                                 f"({getattr(conn.layer, 'name', '')!r}), which has no connected copper: no mesh to attach it to")
    # the interior seeds of every connected polygon, and of every layer, in the order of the connections
    seeds_of = {pair: [] for pair in connectivity.connected}
    layer_seeds = [[] for _ in prob.layers]
    for network, of_network in zip(prob.networks, connectivity.hits):
        for conn, of_conn in zip(network.connections, of_network):
            layer_i = prob.layers.index(conn.layer)
            inside = [g for g, kind in of_conn if kind == 1 and (layer_i, g) in seeds_of]
            for g in inside:
                seeds_of[(layer_i, g)].append(mesh.Point(conn.point.x, conn.point.y))
            if inside:
                layer_seeds[layer_i].append(mesh.Point(conn.point.x, conn.point.y))
    meshes, mesh_index_to_layer_index, skipped = [], [], []
    disconnected_meshes_by_layer = [[] for _ in prob.layers]
    log.info("Meshing the connected components")
    for layer_i, layer in enumerate(prob.layers):
        geoms = list(layer.geoms)
        live = [g for g in range(len(geoms)) if (layer_i, g) in connectivity.connected]
        if live and hasattr(mesher, "polys_to_meshes"):          # a mesher that takes a batch: one call per layer
            meshes.extend(mesher.polys_to_meshes([geoms[g] for g in live], layer_seeds[layer_i]))
        else:
            meshes.extend(mesher.poly_to_mesh(geoms[g], seeds_of[(layer_i, g)]) for g in live)
        mesh_index_to_layer_index.extend([layer_i] * len(live))
        if disconnected == "mesh":
            dead = [g for g in range(len(geoms)) if (layer_i, g) not in connectivity.connected]
            if dead:
                disconnected_meshes_by_layer[layer_i] = _display_meshes(mesher, layer_i, geoms, dead, skipped)
    return PreparedBoard(meshes=meshes, mesh_index_to_layer_index=mesh_index_to_layer_index, filtered_networks=kept,
                         disconnected_meshes_by_layer=disconnected_meshes_by_layer, connectivity=connectivity, skipped=skipped)


def _meshed(prob, mesher_config, mesher, prune: bool) -> tuple:
    """(meshes, mesh_index_to_layer_index, keywords for ``solve_meshed*``) for the ``solve_*`` wrappers: ``mesh_problem``,
    or with ``prune`` :func:`prepare_board` and its kept networks and (empty) lists of disconnected meshes."""
    if not prune:
        meshes, mesh_index_to_layer_index = mesh_problem(prob, mesher_config, mesher)
        return meshes, mesh_index_to_layer_index, {}
    board = prepare_board(prob, mesher_config, mesher=mesher)
    return board.meshes, board.mesh_index_to_layer_index, {"filtered_networks": board.filtered_networks,
                                                           "disconnected_meshes_by_layer": board.disconnected_meshes_by_layer}


# --------------------------------------------------------------------------------------------
# load cases: one board, several settings of its sources
# --------------------------------------------------------------------------------------------

# What a load case may set, by source kind: the values that enter r and nothing else (solver.py:483-484, 490, 503).  A
# resistance, a regulator's gain or a layer's conductance enters L, which all cases of a block share.
CASE_FIELDS = {"CurrentSource": "current", "VoltageSource": "voltage", "VoltageRegulator": "voltage"}


def _ground_terminal(networks, case: dict):
    """The NodeID find_best_ground_node_index grounds, with the values of ``case`` substituted (None: no voltage source)."""
    best, node = float("-inf"), None
    for network in networks:
        for element in network.elements:
            if element_kind(element) == "VoltageSource":
                voltage = case.get(element, element.voltage)
                if voltage > best:
                    best, node = voltage, element.n
    return node


def check_load_cases(prob, cases) -> list:
    """The load cases of ``prob`` as a list of ``{element: float}``, or ValueError.

    ``cases`` is a non-empty sequence of mappings ``{element: value}``; the keys are source elements of ``prob.networks``
    (looked up like ``NodeIndexer.extra_source_to_global_index`` looks them up), the value is the ``current`` of a
    CurrentSource or the ``voltage`` of a VoltageSource / VoltageRegulator.  An element that would change L, one that is
    not in the Problem, a value that is not finite, and a case that moves the ground node (the ``n`` terminal of the
    highest-voltage source, which L stamps) are refused."""
    if isinstance(cases, (Mapping, str, bytes)):
        raise ValueError("cases must be a sequence of mappings {element: value}, one per load case")
    cases = list(cases)
    if not cases:
        raise ValueError("no load cases: give at least one mapping {element: value} ({} is the Problem as given)")
    elements = {element for network in prob.networks for element in network.elements}
    out = []
    for j, case in enumerate(cases):
        if not isinstance(case, Mapping):
            raise ValueError(f"load case {j} is not a mapping {{element: value}}")
        values = {}
        for element, value in case.items():
            kind = element_kind(element)
            if kind not in CASE_FIELDS:
                raise ValueError(f"load case {j}: a {type(element).__name__} cannot vary between load cases -- only the current "
                                 "of a CurrentSource and the voltage of a VoltageSource or VoltageRegulator leave the system "
                                 "matrix L as it is")
            if element not in elements:
                raise ValueError(f"load case {j}: the {kind} is not an element of the Problem's networks")
            try:
                x = float(value)
            except (TypeError, ValueError):
                raise ValueError(f"load case {j}: the {CASE_FIELDS[kind]} of a {kind} must be a number, not {value!r}") from None
            if not math.isfinite(x):
                raise ValueError(f"load case {j}: the {CASE_FIELDS[kind]} of a {kind} must be finite, not {value!r}")
            values[element] = x
        out.append(values)
    ground = _ground_terminal(prob.networks, {})
    for j, values in enumerate(out):
        if _ground_terminal(prob.networks, values) is not ground:
            raise ValueError(f"load case {j} changes which voltage source is the highest, and with it the ground node that L "
                             "stamps (solver.py:671-686); cases share one L")
    return out


def substitute_load_case(prob, case: dict):
    """``prob`` with the values of one checked load case: the named elements replaced (``dataclasses.replace``), the networks
    that hold them rebuilt around the same NodeIDs and connections, the layers shared.  Returns (problem, {id(old network):
    new network})."""
    if not case:
        return prob, {}
    networks, renamed = [], {}
    for network in prob.networks:
        if any(element in case for element in network.elements):
            elements = [dataclasses.replace(e, **{CASE_FIELDS[element_kind(e)]: case[e]}) if e in case else e
                        for e in network.elements]
            renamed[id(network)] = dataclasses.replace(network, elements=elements)
            networks.append(renamed[id(network)])
        else:
            networks.append(network)
    return dataclasses.replace(prob, networks=networks), renamed


def stamp_load_cases(filtered_networks, node_indexer: NodeIndexer, n_unknowns: int, cases: list):
    """The block R (n_unknowns, k) of the checked load ``cases`` as COO triples ``(rows, cols, vals)``: column j is the ``r``
    that stamp_network_into_system and setup_ground_node give for the Problem with case j substituted, entry for entry --
    the same stamps in the same order (``r[iv] = voltage`` for a voltage source, ``+=`` for regulators and current
    sources), duplicates summed as they are stamped.  Entries are listed case by case, each row where it is first stamped;
    zeros are left out."""
    idx, extra = node_indexer.node_to_global_index, node_indexer.extra_source_to_global_index
    program = []            # (row, assign, negate, element, field): the r stamps of solver.py:469-541, in stamping order
    for network in filtered_networks:
        for element in network.elements:
            kind = element_kind(element)
            if kind == "CurrentSource":
                program.append((idx[element.f], False, False, element, "current"))
                program.append((idx[element.t], False, True, element, "current"))
            elif kind == "VoltageSource":
                program.append((extra[element], True, False, element, "voltage"))
            elif kind == "VoltageRegulator":
                program.append((extra[element], False, False, element, "voltage"))
    rows, cols, vals = [], [], []
    for j, case in enumerate(cases):
        r: dict = {}
        for row, assign, negate, element, name in program:
            x = float(case[element]) if element in case else float(getattr(element, name))
            if assign:
                r[row] = x
            else:
                r[row] = r.get(row, 0.0) + (-x if negate else x)
        r[int(n_unknowns) - 1] = 0.0                  # setup_ground_node
        for row, x in r.items():
            if x != 0.0:
                rows.append(row)
                cols.append(j)
                vals.append(x)
    return np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=DTYPE)


def load_case_constraint_values(layout: KKTLayout, rows, cols, vals, k: int) -> dict:
    """``{cst.index: R[cst.index, :]}`` of the block given by its triples, what build_block_reduction takes."""
    values = {cst.index: np.zeros(int(k), dtype=DTYPE) for cst in layout.constraints}
    for row, col, val in zip(np.asarray(rows).tolist(), np.asarray(cols).tolist(), np.asarray(vals).tolist()):
        column = values.get(row)
        if column is not None:
            column[col] = val
    return values


def block_plan_inputs(L: SystemMatrix, rows, cols, vals, n_cols: int):
    """What a device plan of the block given by its triples takes, as ``build_block_reduction`` returns it: (the Reduction of
    L with its floating copper pinned, known_idx, known_val (n_cols, n_known))."""
    layout = L.layout
    if layout is None or not layout.constraints:
        raise SingularSystemError("system has no ground constraint")
    pins = _floating_pins(L, layout, None)
    return build_block_reduction(layout, load_case_constraint_values(layout, rows, cols, vals, n_cols), pins)


def _solve_block_on_device(L: SystemMatrix, rows, cols, vals, n_cols: int, power_rows: int, laps: _Laps,
                           currents: bool = False, current_cols: int = 1):
    """solve_system on the block given by its triples, up to the potentials: reduction, plan, ``solve_block_coo``,
    ``_finish_block``.  The final V stays on the device for the face kernels that follow; ``power_rows``: the rows of the
    power-density array those return, made ready while the device solves (with ``currents``, the arrays of
    ``current_report`` too, or those of ``current_cases`` for ``current_cols`` columns).  Returns (plan, V (N, n_cols), ||L v_j - r_j|| (n_cols,), SolveResult, n_tri, n_mesh); ``laps``
    receives stage1 and stage2."""
    red, known_idx, known_val = block_plan_inputs(L, rows, cols, vals, n_cols)
    plan = _plan_for(L, L.dev, L.layout, red, _wants_reorder(L, None), False)
    members = red.probe_members
    n_tri = len(L.tri) if L.tri is not None else 0
    n_mesh = len(L.mesh_offsets) - 1 if L.mesh_offsets is not None else 0
    probes, res = plan.solve_block_coo(n_cols, rows, cols, vals, known_idx, known_val, red.regulator_columns, members,
                                       rtol=RTOL, max_iter=MAX_ITER, abs_residual_target=ABS_RESIDUAL_TARGET, power_tri=n_tri,
                                       power_rows=power_rows, current_tri=n_tri if currents else 0,
                                       current_cols=current_cols)
    laps.lap("stage1")
    V, residual_norms = _finish_block(plan, red, members, probes, n_cols)
    laps.lap("stage2")
    return plan, V, residual_norms, res, n_tri, n_mesh


def _column_solution(board: IndexedBoard, prob, v: np.ndarray, residual_norm, res, power, where: str = "") -> Solution:
    """The Solution of ``prob`` from one column ``v`` of a solved block and that column's power densities ``power`` (None
    without triangles); its SolverInfo reports the block solve as a whole.  ``where`` opens the ground-current warning."""
    ground_node_current = float(v[-1])
    _warn_ground_current(ground_node_current, where)
    layer_solutions = produce_layer_solutions(board.prob.layers, board.vindex, board.meshes, board.layer_of, v,
                                              board.disconnected_meshes_by_layer, power_all=power)
    return Solution(problem=prob, layer_solutions=layer_solutions,
                    solver_info=_solver_info(res, ground_node_current, residual_norm))


def solve_meshed_load_cases(prob, meshes, mesh_index_to_layer_index, cases, *, filtered_networks=None,
                            disconnected_meshes_by_layer=None, partition=None, timings: Optional[dict] = None) -> list:
    """``solve_meshed`` for several load cases of one board: a list of Solutions, one per mapping of ``cases`` (see
    :func:`check_load_cases`; elements a case does not name keep their Problem value, and an element whose network is not
    among ``filtered_networks`` has no effect, as in the Problem itself).

    The connections are snapped, L assembled and its reduction planned once; the cases go through one block solve whose
    right-hand sides cross to the device as their non-zero entries, and the power densities of all cases are computed from
    the potentials the device holds.  Solution j carries the Problem with case j substituted, its own potentials and power
    densities, and a SolverInfo whose ``ground_node_current`` and ``residual_norm`` are its own while ``iterations``,
    ``rel_residual`` and ``solve_seconds`` are those of the block solve as a whole (``residual_norms`` is None).  One case
    is ``solve_meshed`` on its substituted Problem.  ValueError, before anything reaches the device, for invalid cases and
    for a ``partition`` over several GPUs (the row-partitioned path does not take load cases).
    ``timings`` (a dict) receives the host time of each step of a block in seconds."""
    _refuse_partition(partition, "load cases")
    cases = check_load_cases(prob, cases)
    substituted = [substitute_load_case(prob, case) for case in cases]
    if len(cases) == 1:
        sub, renamed = substituted[0]
        if filtered_networks is not None:
            filtered_networks = [renamed.get(id(network), network) for network in filtered_networks]
        return [solve_meshed(sub, meshes, mesh_index_to_layer_index, filtered_networks=filtered_networks,
                             disconnected_meshes_by_layer=disconnected_meshes_by_layer)]
    k = len(cases)
    laps = _Laps(timings)
    board = index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer)
    laps.lap("indexing")
    with board.assembled() as (L, _):
        rows, cols, vals = stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], cases)
        laps.lap("assembly")
        log.info(f"Solving {k} load cases as one block")
        plan, V, residual_norms, res, n_tri, _n_mesh = _solve_block_on_device(L, rows, cols, vals, k, k, laps)
        power = plan.power_density_block(k, n_tri) if n_tri else None
        laps.lap("power_density")
    laps.lap()
    _warn_if_block_stalled(res, residual_norms, cols, vals, k)
    log.info("Producing the solution objects")
    solutions = [_column_solution(board, sub, V[:, j], residual_norms[j], res, None if power is None else power[j],
                                  f"Load case {j}: ") for j, (sub, _) in enumerate(substituted)]
    laps.lap("solutions")
    return solutions


def solve_load_cases(prob, cases, mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None,
                     partition=None, prune=False) -> list:
    """``solve`` for several load cases of one board (see :func:`solve_meshed_load_cases`): the board is meshed once."""
    _refuse_partition(partition, "load cases")
    cases = check_load_cases(prob, cases)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_load_cases(prob, meshes, mesh_index_to_layer_index, cases, **pruned)


# --------------------------------------------------------------------------------------------
# sensitivities: where the drop between two nodes comes from (adjoint method, DESIGN.md "Sensitivities")
# --------------------------------------------------------------------------------------------

# The parameters of each lumped element that Sensitivity.elements differentiates J by
SENSITIVITY_FIELDS = {"Resistor": ("resistance",), "CurrentSource": ("current",), "VoltageSource": ("voltage",),
                      "VoltageRegulator": ("voltage", "gain")}


@dataclass
class Sensitivity:
    """Derivatives of one objective J = V(p) - V(n) of a solved Problem (see :func:`solve_meshed_sensitivities`)."""
    nodes: tuple          # (p, n) as given: two NodeIDs
    value: float          # J = V(p) - V(n) of the solution [V]
    densities: list       # per layer, per mesh of LayerSolution.meshes: TwoForm, s_f / area_f [V/mm^2]
    layers: list          # per layer: sigma_l * dJ/dsigma_l [V]  (= sum of s_f over the layer's faces)
    elements: dict        # lumped element -> {field name: dJ/d(field)}


def _is_node_id(obj) -> bool:
    """A NodeID of padne_amd.problem or of padne's own problem module (by class name, like element_kind)."""
    return any(cls.__name__ == "NodeID" for cls in type(obj).__mro__)


def check_objectives(prob, objectives, filtered_networks=None) -> list:
    """The objectives as a list of (p, n) NodeID pairs, or ValueError.

    ``objectives`` is a non-empty sequence of pairs (p, n); J = V(p) - V(n).  Both nodes must belong to the same network
    among ``filtered_networks`` (default: all networks of ``prob``) -- a terminal of one of its elements or the node of one
    of its connections -- and p is not n."""
    if isinstance(objectives, (Mapping, str, bytes)) or _is_node_id(objectives):
        raise ValueError("objectives must be a sequence of (p, n) pairs of NodeIDs")
    try:
        objectives = list(objectives)
    except TypeError:
        raise ValueError("objectives must be a sequence of (p, n) pairs of NodeIDs") from None
    if not objectives:
        raise ValueError("no objectives: give at least one (p, n) pair of NodeIDs")
    networks = list(prob.networks) if filtered_networks is None else list(filtered_networks)
    network_of = {}
    for i, network in enumerate(networks):
        for node in list(network.nodes) + [conn.node_id for conn in network.connections]:
            network_of.setdefault(node, i)
    out = []
    for j, pair in enumerate(objectives):
        if isinstance(pair, (str, bytes, Mapping)) or _is_node_id(pair):
            raise ValueError(f"objective {j} is not a (p, n) pair of NodeIDs")
        try:
            pair = tuple(pair)
        except TypeError:
            raise ValueError(f"objective {j} is not a (p, n) pair of NodeIDs") from None
        if len(pair) != 2:
            raise ValueError(f"objective {j} is not a (p, n) pair of NodeIDs: it has {len(pair)} entries")
        p, n = pair
        if not (_is_node_id(p) and _is_node_id(n)):
            raise ValueError(f"objective {j}: p and n must be NodeIDs, not {type(p).__name__} and {type(n).__name__}")
        if p is n:
            raise ValueError(f"objective {j}: p is n, so V(p) - V(n) is zero by definition")
        for name, node in (("p", p), ("n", n)):
            if node not in network_of:
                raise ValueError(f"objective {j}: {name} is not a node of the solved networks")
        if network_of[p] != network_of[n]:
            raise ValueError(f"objective {j}: p and n are nodes of different networks")
        out.append((p, n))
    return out


def global_elements(filtered_networks, node_indexer: NodeIndexer) -> list:
    """The lumped elements of the solved networks in stamping order, each as ``(element, row)`` with ``row`` the tuple of
    the reference's stamps on global unknowns: ("R", a, b, resistance), ("I", f, t, current), ("V", p, n, voltage, i_v),
    ("REG", v_p, v_n, s_f, s_t, voltage, gain, i_v)."""
    idx, extra = node_indexer.node_to_global_index, node_indexer.extra_source_to_global_index
    out = []
    for network in filtered_networks:
        for element in network.elements:
            kind = element_kind(element)
            if kind == "Resistor":
                row = ("R", idx[element.a], idx[element.b], float(element.resistance))
            elif kind == "CurrentSource":
                row = ("I", idx[element.f], idx[element.t], float(element.current))
            elif kind == "VoltageSource":
                row = ("V", idx[element.p], idx[element.n], float(element.voltage), extra[element])
            elif kind == "VoltageRegulator":
                row = ("REG", idx[element.v_p], idx[element.v_n], idx[element.s_f], idx[element.s_t], float(element.voltage),
                       float(element.gain), extra[element])
            else:
                raise NotImplementedError(f"Unsupported node type {element}")
            out.append((element, row))
    return out


def woodbury_terms(rows) -> list:
    """``(s_f, s_t, i_v, gain)`` of every regulator among the element rows (global_elements) whose gain term makes L
    unsymmetric: L^T = L + U V^T with U = [g_k e_iv,k | -g_k d_k], V = [d_k | e_iv,k], d_k = e_sf,k - e_st,k.  A regulator
    with gain 0 or with s_f and s_t on one unknown stamps nothing unsymmetric and is left out."""
    out = []
    for row in rows:
        if row[0] == "REG":
            _, _vp, _vn, sf, st, _u, gain, iv = row
            if gain != 0.0 and sf != st:
                out.append((int(sf), int(st), int(iv), float(gain)))
    return out


def sensitivity_block_columns(n_obj: int, n_terms: int) -> int:
    """Columns of the block of a sensitivity solve: r, the k objectives c_j, then per Woodbury term the unit current from s_f
    to s_t (columns 1 + k + q) and regulator q's voltage row at 1 (columns 1 + k + K + q)."""
    return 1 + int(n_obj) + 2 * int(n_terms)


def stamp_sensitivity_block(filtered_networks, node_indexer: NodeIndexer, n_unknowns: int, objective_rows, terms):
    """COO triples (rows, cols, vals) of the block of a sensitivity solve (sensitivity_block_columns): column 0 is the
    Problem's r as stamp_load_cases lists it, column 1 + j is c_j = e_p - e_n for ``objective_rows[j]`` = (p, n) as global
    unknowns (empty when both land on one unknown), then d_q and e_iv,q of the Woodbury ``terms``."""
    rows, cols, vals = stamp_load_cases(filtered_networks, node_indexer, n_unknowns, [{}])
    rows, cols, vals = rows.tolist(), cols.tolist(), vals.tolist()
    k, K = len(objective_rows), len(terms)

    def pair(col, a, b):
        if a != b:
            rows.extend((int(a), int(b)))
            cols.extend((col, col))
            vals.extend((1.0, -1.0))
    for j, (p, n) in enumerate(objective_rows):
        pair(1 + j, p, n)
    for q, (sf, st, iv, _gain) in enumerate(terms):
        pair(1 + k + q, sf, st)
        rows.append(int(iv))
        cols.append(1 + k + K + q)
        vals.append(1.0)
    return np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=DTYPE)


def adjoint_weights(V: np.ndarray, n_obj: int, terms) -> np.ndarray:
    """The weights W (n_obj, n_cols) with lambda_j = V W[j] the solution of L^T lambda_j = c_j, from the solved block V of
    stamp_sensitivity_block (only its rows s_f, s_t and i_v of the ``terms`` are read).  Without terms W selects column
    1 + j.  With them, by Woodbury, lambda = y - Z (I + V^T Z)^-1 V^T y for y = L^-1 c, Z = L^-1 U: the 2K x 2K system is
    solved here, on the host."""
    V = np.asarray(V, dtype=DTYPE)
    k, K = int(n_obj), len(terms)
    n_cols = sensitivity_block_columns(k, K)
    if V.ndim != 2 or V.shape[1] != n_cols:
        raise ValueError(f"the block must have {n_cols} columns, not {V.shape}")
    W = np.zeros((k, n_cols), dtype=DTYPE)
    W[np.arange(k), 1 + np.arange(k)] = 1.0
    if not K:
        return W
    sf = np.array([t[0] for t in terms], dtype=np.int64)
    st = np.array([t[1] for t in terms], dtype=np.int64)
    iv = np.array([t[2] for t in terms], dtype=np.int64)
    g = np.array([t[3] for t in terms], dtype=DTYPE)

    def vt(cols):                   # V^T applied to the block columns ``cols``: [d_q^T z ; z[iv_q]], (2K, len(cols))
        return np.concatenate([V[sf][:, cols] - V[st][:, cols], V[iv][:, cols]], axis=0)
    col_d = 1 + k + np.arange(K)
    col_e = 1 + k + K + np.arange(K)
    # Z = [g_q Y_e,q | -g_q Y_d,q] as block columns with coefficients
    z_cols = np.concatenate([col_e, col_d])
    z_coef = np.concatenate([g, -g])
    G = np.eye(2 * K) + vt(z_cols) * z_coef[None, :]
    A = np.linalg.solve(G, vt(1 + np.arange(k)))            # (2K, k): (I + V^T Z)^-1 V^T y_j
    # lambda_j = y_j - sum_m A[m, j] z_coef[m] Y[:, z_cols[m]]
    W[:, z_cols] -= (A * z_coef[:, None]).T
    return W


def element_sensitivities(element_rows, x: np.ndarray, lam: np.ndarray) -> list:
    """dJ/d(field) of every element row (global_elements' tuples, indices into ``x`` and ``lam``) for the solution ``x``
    and the adjoint ``lam`` (L^T lam = c), as one dict per row:

    - Resistor:         dJ/dR = -(lam_a - lam_b)(x_a - x_b) / R^2
    - CurrentSource:    dJ/dI = lam_f - lam_t
    - VoltageSource:    dJ/dU = lam_iv
    - VoltageRegulator: dJ/dU = lam_iv,  dJ/dgain = -(lam_sf - lam_st) x_iv"""
    out = []
    for row in element_rows:
        kind = row[0]
        if kind == "R":
            _, a, b, res = row
            out.append({"resistance": float(-(lam[a] - lam[b]) * (x[a] - x[b]) / (res * res))})
        elif kind == "I":
            _, f, t, _cur = row
            out.append({"current": float(lam[f] - lam[t])})
        elif kind == "V":
            out.append({"voltage": float(lam[row[4]])})
        elif kind == "REG":
            _, _vp, _vn, sf, st, _u, _gain, iv = row
            out.append({"voltage": float(lam[iv]), "gain": float(-(lam[sf] - lam[st]) * x[iv])})
        else:
            raise NotImplementedError(f"Unsupported element row {row}")
    return out


def _sensitivity_elements(pairs, V: np.ndarray, W: np.ndarray) -> list:
    """element_sensitivities of every objective, with x and lambda gathered at the elements' unknowns only."""
    local, Vu = _gather_element_rows([row for _, row in pairs], V)
    x, lam = Vu[:, 0], Vu @ W.T
    per_obj = [element_sensitivities(local, x, lam[:, j]) for j in range(W.shape[0])]
    return [{element: d[i] for i, (element, _) in enumerate(pairs)} for d in per_obj]


_ROW_UNKNOWNS = {"R": (1, 2), "I": (1, 2), "V": (1, 2, 4), "REG": (1, 2, 3, 4, 7)}     # where global_elements' rows name unknowns
_ROW_SENSITIVITY_UNKNOWNS = {"R": (1, 2), "I": (1, 2), "V": (4,), "REG": (3, 4, 7)}       # the ones element_sensitivities reads


def _gather_element_rows(rows, V: np.ndarray, positions=_ROW_SENSITIVITY_UNKNOWNS):
    """(the element rows with the unknowns at ``positions`` renumbered into the gathered rows, V's rows at those unknowns
    (n_used, n_cols)): V is read at the elements' unknowns only."""
    used = sorted({int(row[p]) for row in rows for p in positions[row[0]]})
    at = {g: i for i, g in enumerate(used)}
    local = [tuple(at[int(v)] if p in positions[row[0]] else v for p, v in enumerate(row)) for row in rows]
    Vu = V[np.asarray(used, dtype=np.int64)] if used else np.zeros((0, V.shape[1]))
    return local, Vu


def solve_meshed_sensitivities(prob, meshes, mesh_index_to_layer_index, objectives, *, filtered_networks=None,
                               disconnected_meshes_by_layer=None, partition=None,
                               timings: Optional[dict] = None):
    """``solve_meshed`` together with the sensitivities of potential differences: (Solution, [Sensitivity per objective]).

    An objective is a pair (p, n) of NodeIDs of one network among ``filtered_networks`` (:func:`check_objectives`); its
    J = V(p) - V(n).  With M x = r the reference's system (``solver.py:469-560``, M = L) and J = c^T x, c = e_p - e_n, the
    adjoint lambda solves M^T lambda = c, and for every parameter theta dJ/dtheta = lambda^T (dr/dtheta - dM/dtheta x):

    - face f of a mesh of sheet conductance sigma, whose edges (i, k) carry the assembly's cot weights w_ik (|cot|/2 of the
      opposite corner, ``HalfEdge.cotan``): s_f = sigma dJ/dsigma_f = sigma sum_edges w_ik (lambda_i - lambda_k)(x_i - x_k);
      ``densities`` holds s_f / area_f and ``layers[l]`` the sum of s_f over the layer, which is sigma_l dJ/dsigma_l;
    - ``elements``: every lumped element of the solved networks, {field: dJ/dfield} (:func:`element_sensitivities`).

    Regulators make M unsymmetric; M^T = M + U V^T (:func:`woodbury_terms`) and lambda follows by Woodbury from ordinary
    solves with M (:func:`adjoint_weights`).  All of it is one block solve of 1 + k + 2K right-hand sides on one assembly and
    plan (K: regulators with a gain term); the faces come from one kernel over the potentials the device holds.  The
    Solution is that of ``prob``, filled as ``solve_meshed_load_cases`` fills a case of a block (its SolverInfo reports the
    block solve as a whole).  ValueError, before anything reaches the device, for invalid objectives and for a
    ``partition`` over several GPUs.  ``timings`` (a dict) receives the host time of each step in seconds."""
    _refuse_partition(partition, "sensitivities")
    objectives = check_objectives(prob, objectives, filtered_networks)
    k = len(objectives)
    laps = _Laps(timings)
    board = index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer)
    pairs = global_elements(board.filtered_networks, board.node_indexer)
    terms = woodbury_terms([row for _, row in pairs])
    idx = board.node_indexer.node_to_global_index
    objective_rows = [(idx[p], idx[n]) for p, n in objectives]
    n_cols = sensitivity_block_columns(k, len(terms))
    laps.lap("indexing")
    with board.assembled() as (L, _):
        rows, cols, vals = stamp_sensitivity_block(board.filtered_networks, board.node_indexer, L.shape[0], objective_rows, terms)
        laps.lap("assembly")
        log.info(f"Solving {k} adjoint(s) and {2 * len(terms)} regulator column(s) as one block with the Problem")
        plan, V, residual_norms, res, n_tri, n_mesh = _solve_block_on_device(L, rows, cols, vals, n_cols, 1 + k, laps)
        # the adjoint weights on the host, then the face kernel on the V the device holds: the power of column 0 (n_tri,),
        # s_f / area_f (k, n_tri) and the per-mesh sums of s_f (k, n_mesh)
        W = adjoint_weights(V, k, terms)
        power = density = totals = None
        if n_tri:
            power, density, totals = plan.sensitivity_block(W, n_tri, n_mesh)
        laps.lap("sensitivity")
    laps.lap()
    log.info("Producing the solution and the sensitivities")
    _warn_if_block_stalled(res, residual_norms, cols, vals, n_cols)
    solution = _column_solution(board, prob, np.ascontiguousarray(V[:, 0]), residual_norms[0], res, power)
    elements = _sensitivity_elements(pairs, V, W)
    sens = []
    for j, ((p, n), (ip, in_)) in enumerate(zip(objectives, objective_rows)):
        densities, layer_sums = [], []
        for layer_i in range(len(prob.layers)):
            forms, total = [], 0.0
            for mesh_i, msh, lo, hi in board.layer_meshes(layer_i):
                tf = mesh.TwoForm(msh)
                if density is not None:
                    tf.values = np.array(density[j, lo:hi], dtype=DTYPE)
                    total += float(totals[j, mesh_i])
                forms.append(tf)
            densities.append(forms)
            layer_sums.append(total)
        sens.append(Sensitivity(nodes=(p, n), value=float(V[ip, 0] - V[in_, 0]), densities=densities, layers=layer_sums,
                                elements=elements[j]))
    laps.lap("solutions")
    return solution, sens


def solve_sensitivities(prob, objectives, mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None,
                        partition=None, prune=False):
    """``solve`` with the sensitivities of potential differences (see :func:`solve_meshed_sensitivities`): the board is
    meshed once.  Returns (Solution, [Sensitivity per objective])."""
    _refuse_partition(partition, "sensitivities")
    objectives = check_objectives(prob, objectives)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_sensitivities(prob, meshes, mesh_index_to_layer_index, objectives, **pruned)


# --------------------------------------------------------------------------------------------
# currents: where the current goes (DESIGN.md "Currents")
# --------------------------------------------------------------------------------------------

MAX_CUTS = 4096


@dataclass(frozen=True)
class Cut:
    """A directed straight segment on one layer of a Problem (``layer`` is matched by identity).  ``start`` and ``end`` are
    (x, y) in mm: a 2-sequence or an object with ``.x`` / ``.y``, like ``Connection.point``.  Its current is the current
    that crosses it from the left of start -> end to its right."""
    layer: object
    start: object
    end: object


@dataclass
class CurrentReport:
    """Where the current of a solved Problem goes (see :func:`solve_meshed_currents`)."""
    vectors: list         # per layer, per mesh of LayerSolution.meshes: (n_faces, 2) J = -sigma grad V [A/mm]
    magnitudes: list      # per layer, per mesh: TwoForm of |J| [A/mm]
    hotspots: list        # per layer: (max |J|, mesh index within the layer, face index, centroid x, y), None without faces
    layers: list          # per layer: the power dissipated in its copper [W]
    elements: dict        # lumped element -> {"current": A, "power": W} (+ "input_current", "input_power": regulators)
    cuts: list            # per cut, in the order given: the current crossing it [A]


def _cut_point(p, j: int, which: str) -> tuple:
    if hasattr(p, "x") and hasattr(p, "y"):
        xy = (p.x, p.y)
    elif isinstance(p, (str, bytes, Mapping)):
        raise ValueError(f"cut {j}: {which} must be (x, y) or have .x and .y")
    else:
        try:
            xy = tuple(p)
        except TypeError:
            raise ValueError(f"cut {j}: {which} must be (x, y) or have .x and .y") from None
        if len(xy) != 2:
            raise ValueError(f"cut {j}: {which} must be (x, y), not {len(xy)} numbers")
    try:
        x, y = float(xy[0]), float(xy[1])
    except (TypeError, ValueError):
        raise ValueError(f"cut {j}: {which} must be two numbers") from None
    if not (math.isfinite(x) and math.isfinite(y)):
        raise ValueError(f"cut {j}: {which} is not finite")
    return x, y


def check_cuts(prob, cuts) -> list:
    """The cuts as (layer index, (x0, y0), (x1, y1)), or ValueError: at most MAX_CUTS of them, each a :class:`Cut` (or an
    object with ``layer``, ``start``, ``end``) whose layer is one of ``prob.layers`` (by identity), with finite end points
    that differ."""
    if isinstance(cuts, (str, bytes, Mapping)) or all(hasattr(cuts, a) for a in ("layer", "start", "end")):
        raise ValueError("cuts must be a sequence of Cut")
    try:
        cuts = list(cuts)
    except TypeError:
        raise ValueError("cuts must be a sequence of Cut") from None
    if len(cuts) > MAX_CUTS:
        raise ValueError(f"{len(cuts)} cuts: at most {MAX_CUTS} in one call")
    out = []
    for j, cut in enumerate(cuts):
        if not all(hasattr(cut, a) for a in ("layer", "start", "end")):
            raise ValueError(f"cut {j} is not a Cut(layer, start, end)")
        layer_i = next((i for i, layer in enumerate(prob.layers) if layer is cut.layer), None)
        if layer_i is None:
            raise ValueError(f"cut {j}: its layer is not one of the Problem's layers")
        a, b = _cut_point(cut.start, j, "start"), _cut_point(cut.end, j, "end")
        if a == b:
            raise ValueError(f"cut {j}: start and end are the same point")
        out.append((layer_i, a, b))
    return out


def element_flows(element_rows, x: np.ndarray) -> list:
    """Current and power of every element row (global_elements' tuples, indices into ``x``), one dict per row.

    Passive sign convention: ``current`` flows through the element from its first terminal to its second, and ``power`` =
    (x_first - x_second) current is what the element absorbs.  With L = -G, row j of L x = r says that minus the current
    leaving j through the copper and the resistors, plus the stamped source terms, is r_j: every element term of row j is
    minus the current that leaves j through that element.  Hence:

    - Resistor (a, b):         row a holds -(x_a - x_b)/R, so current = (x_a - x_b) / R;
    - CurrentSource (f, t):    r_f = +current moves to the left as -current: the source takes ``current`` out of f and
      delivers it to t, so current = its ``current`` field, exactly;
    - VoltageSource (p, n):    row p holds +x_iv, so -x_iv leaves p through the source: current = -x_iv;
    - VoltageRegulator output (v_p, v_n): the same stamps, current = -x_iv;
    - VoltageRegulator input (s_f, s_t):  row s_f holds +gain x_iv: input_current = -gain x_iv, and input_power =
      (x_sf - x_st) input_current.

    The powers of all elements and the copper's dissipation add up to zero (Tellegen)."""
    out = []
    for row in element_rows:
        kind = row[0]
        if kind == "R":
            _, a, b, res = row
            cur = (x[a] - x[b]) / res
            out.append({"current": float(cur), "power": float((x[a] - x[b]) * cur)})
        elif kind == "I":
            _, f, t, cur = row
            out.append({"current": float(cur), "power": float((x[f] - x[t]) * cur)})
        elif kind == "V":
            _, p, n, _u, iv = row
            cur = -x[iv]
            out.append({"current": float(cur), "power": float((x[p] - x[n]) * cur)})
        elif kind == "REG":
            _, vp, vn, sf, st, _u, gain, iv = row
            cur, cin = -x[iv], -gain * x[iv]
            out.append({"current": float(cur), "power": float((x[vp] - x[vn]) * cur), "input_current": float(cin),
                        "input_power": float((x[sf] - x[st]) * cin)})
        else:
            raise NotImplementedError(f"Unsupported element row {row}")
    return out


def solve_meshed_currents(prob, meshes, mesh_index_to_layer_index, cuts=(), *, filtered_networks=None,
                          disconnected_meshes_by_layer=None, partition=None, timings: Optional[dict] = None):
    """``solve_meshed`` together with where the current goes: (Solution, CurrentReport).

    - ``vectors`` / ``magnitudes``: per face J = -sigma grad V [A/mm], the sheet current density, with sigma the layer's
      conductance and grad V the face gradient of the power density, so |J|^2 / sigma is the power density;
    - ``hotspots``: per layer the largest |J| (the lowest global face on a tie), its mesh within the layer, its face and the
      face's centroid;
    - ``layers``: per layer the power in its copper, sum over faces of sigma sum_edges w_ik (V_i - V_k)^2 with the
      assembly's |cot|/2 weights.  Not the gradient form A |J|^2 / sigma: the two differ on obtuse faces, and only the
      weights' form balances the elements' powers exactly;
    - ``elements``: current and power of every lumped element of the solved networks (:func:`element_flows`);
    - ``cuts``: per :class:`Cut`, the current crossing it from its left to its right.  Every face edge (P, Q), P the lower
      global vertex, whose ends lie on different sides of the cut's line (a vertex on the line counts as right) and which
      the segment crosses adds sigma |cot|/2 (V_left - V_right) from each of its faces.  A cut whose ends lie outside the
      copper and which splits a piece of copper in two gives the current between the two parts exactly (KCL on L x = r).
      A cut that ends inside copper measures a flux through the segment that is not conserved: it depends on where the
      segment ends.  Polylines and closed contours are out of scope; several cuts sum.

    One call is the load-case block path with one column and its face kernels on the V the device holds; element currents
    come from V's rows at the elements' unknowns.  Disconnected meshes carry no current and take no part.  The Solution is
    that of ``prob``, filled as ``solve_meshed_sensitivities`` fills it.  ValueError, before anything reaches the device, for
    invalid cuts (:func:`check_cuts`) and for a ``partition`` over several GPUs.  ``timings`` (a dict) receives the host
    time of each step in seconds."""
    _refuse_partition(partition, "currents")
    laps = _Laps(timings)
    (solution,), (report,), _ = _solve_block_currents(prob, meshes, mesh_index_to_layer_index, [{}], check_cuts(prob, cuts), True,
                                                      False, filtered_networks, disconnected_meshes_by_layer, laps)
    laps.lap("solutions")
    return solution, report


def solve_currents(prob, cuts=(), mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None, partition=None, prune=False):
    """``solve`` with where the current goes (see :func:`solve_meshed_currents`): the board is meshed once.  Returns
    (Solution, CurrentReport)."""
    _refuse_partition(partition, "currents")
    cuts = check_cuts(prob, cuts)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_currents(prob, meshes, mesh_index_to_layer_index,
                                 [Cut(prob.layers[i], a, b) for i, a, b in cuts], **pruned)


# --------------------------------------------------------------------------------------------
# load-case currents: the currents of every load case of one block, and their envelope (DESIGN.md "Load-case currents")
# --------------------------------------------------------------------------------------------


@dataclass
class CurrentEnvelope:
    """The worst case of every quantity of the CurrentReports of one block of load cases (see
    :func:`solve_meshed_load_case_currents`): the maximum over the cases of an absolute value, with the lowest case that
    attains it (:func:`envelope_of`)."""
    magnitudes: list      # per layer, per mesh: TwoForm of max_j |J_j| per face [A/mm]
    cases: list           # per layer, per mesh: (n_faces,) int32, the case of that maximum
    hotspots: list        # per layer: (max |J|, case, mesh index within the layer, face index, centroid x, y), None without faces
    layers: list          # per layer: (the largest power in its copper [W], case)
    elements: dict        # lumped element of the Problem -> {"current": (signed value of largest magnitude, case), "power": ...}
    cuts: list            # per cut: (signed current of largest magnitude [A], case)


def envelope_of(values) -> tuple:
    """(max_j |values[j]|, the lowest j that attains it) down the first axis of ``values`` (k, n): (n,) float64 and (n,)
    int32.  The rule is sequential over the cases: case 0 first, and a later case replaces the value only when its
    magnitude is strictly greater -- so ties go to the lowest case, and an entry that is NaN in case 0 stays NaN with case
    0.  It is the rule the device applies per face."""
    a = np.abs(np.asarray(values, dtype=DTYPE))
    if a.ndim != 2 or a.shape[0] < 1:
        raise ValueError("values must have shape (k, n) with k >= 1")
    best, case = a[0].copy(), np.zeros(a.shape[1], dtype=np.int32)
    for j in range(1, a.shape[0]):
        greater = a[j] > best
        best[greater] = a[j][greater]
        case[greater] = j
    return best, case


def _signed_envelope(values) -> list:
    """Per column of ``values`` (k, n): (the signed entry of largest magnitude, its case), by :func:`envelope_of`."""
    values = np.asarray(values, dtype=DTYPE).reshape(len(values), -1)
    _, case = envelope_of(values)
    return [(float(values[c, i]), int(c)) for i, c in enumerate(case)]


_ROW_VALUE = {"I": 3, "V": 3, "REG": 5}        # where global_elements' rows hold the value a load case may set


def _case_element_rows(pairs, rows, case: dict) -> list:
    """The element ``rows`` (those of ``pairs``, global_elements' order) with the values of one checked load case."""
    out = []
    for (element, _), row in zip(pairs, rows):
        if element in case:
            at = _ROW_VALUE[row[0]]
            row = row[:at] + (float(case[element]),) + row[at + 1:]
        out.append(row)
    return out


def _solve_block_currents(prob, meshes, mesh_index_to_layer_index, cases, cuts, fields: bool, envelope: bool,
                          filtered_networks, disconnected_meshes_by_layer, laps: _Laps):
    """The checked ``cases`` of ``prob`` as one block with the currents of every column: index, assemble, solve the block,
    ``power_density_block`` and ``current_cases`` on the V the device holds, then a Solution and a CurrentReport per case
    (``fields``: with their ``vectors`` and ``magnitudes``).  ``cuts`` as :func:`check_cuts` returns them.  Without
    ``envelope`` the per-face envelope is neither computed nor sent home.  Returns (solutions, reports, what a
    CurrentEnvelope is built from: (board, pairs, the element flows per case, env, env_case)); ``laps`` receives every step
    up to the currents."""
    substituted = [substitute_load_case(prob, case) for case in cases]
    k, n_layers = len(cases), len(prob.layers)
    board = index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer)
    pairs = global_elements(board.filtered_networks, board.node_indexer)
    laps.lap("indexing")
    with board.assembled() as (L, _):
        rows, cols, vals = stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], cases)
        laps.lap("assembly")
        log.info(f"Solving {k} load case(s) as one block, with their currents")
        plan, V, residual_norms, res, n_tri, _n_mesh = _solve_block_on_device(L, rows, cols, vals, k, k, laps, currents=fields,
                                                                              current_cols=k)
        power = J = mag = env = env_case = mesh_max = mesh_face = totals = None
        cut_values = np.zeros((k, len(cuts)))
        if n_tri:
            power = plan.power_density_block(k, n_tri)
            J, mag, env, env_case, mesh_max, mesh_face, totals, cut_values = plan.current_cases(
                k, n_tri, np.asarray(mesh_index_to_layer_index, dtype=np.int32), [c[0] for c in cuts],
                np.array([[*a, *b] for _, a, b in cuts], dtype=DTYPE).reshape(-1, 4), fields=fields, envelope=envelope)
        laps.lap("currents")
    laps.lap()
    _warn_if_block_stalled(res, residual_norms, cols, vals, k)
    log.info("Producing the solution objects and the current reports")
    solutions = [_column_solution(board, sub, np.ascontiguousarray(V[:, j]), residual_norms[j], res,
                                  None if power is None else power[j], f"Load case {j}: " if k > 1 else "")
                 for j, (sub, _) in enumerate(substituted)]
    local, Vu = _gather_element_rows([row for _, row in pairs], V, _ROW_UNKNOWNS)
    reports, flows_by_case = [], []
    for j, (case, (_, renamed)) in enumerate(zip(cases, substituted)):
        flows = element_flows(_case_element_rows(pairs, local, case), Vu[:, j])
        flows_by_case.append(flows)
        case_elements = [e for network in board.filtered_networks for e in renamed.get(id(network), network).elements]
        vectors, magnitudes, hotspots, layer_power = [], [], [], []
        for layer_i in range(n_layers):
            vecs, forms, total, best = [], [], 0.0, None
            for in_layer, (mesh_i, msh, lo, hi) in enumerate(board.layer_meshes(layer_i)):
                if n_tri:
                    total += float(totals[j, mesh_i])
                    # meshes come in global face order: a later mesh wins only with a strictly larger |J|
                    if mesh_face[j, mesh_i] >= 0 and (best is None or mesh_max[j, mesh_i] > best[0]):
                        face = int(mesh_face[j, mesh_i] - lo)
                        cx, cy = msh.points[msh.triangles[face]].mean(axis=0)
                        best = (float(mesh_max[j, mesh_i]), in_layer, face, float(cx), float(cy))
                if fields:
                    tf = mesh.TwoForm(msh)
                    if J is not None:
                        vecs.append(J[j, lo:hi])              # views of this call's own result arrays: no copies
                        tf.values = mag[j, lo:hi]
                    else:
                        vecs.append(np.zeros((len(msh.triangles), 2), dtype=DTYPE))
                    forms.append(tf)
            vectors.append(vecs)
            magnitudes.append(forms)
            hotspots.append(best)
            layer_power.append(total)
        reports.append(CurrentReport(vectors=vectors if fields else None, magnitudes=magnitudes if fields else None,
                                     hotspots=hotspots, layers=layer_power,
                                     elements={element: flows[i] for i, element in enumerate(case_elements)},
                                     cuts=[float(c) for c in cut_values[j]]))
    return solutions, reports, (board, pairs, flows_by_case, env, env_case)


def solve_meshed_load_case_currents(prob, meshes, mesh_index_to_layer_index, cases, cuts=(), *, per_case_fields=True,
                                    filtered_networks=None, disconnected_meshes_by_layer=None, partition=None,
                                    timings: Optional[dict] = None):
    """``solve_meshed_load_cases`` together with where the current goes in every case and in the worst case: ([Solution per
    case], [CurrentReport per case], CurrentEnvelope).

    Solution j is what ``solve_meshed_load_cases`` gives for case j of a block; ``reports[j]`` is the CurrentReport of
    ``solve_meshed_currents`` for that case, its ``elements`` keyed by the elements of the substituted Problem.  The
    envelope holds, for every face, layer, element and cut, the maximum over the cases of the absolute value and the
    lowest case that attains it (:func:`envelope_of`); its ``elements`` are keyed by the elements of ``prob``.  A layer's
    envelope hotspot is the hotspot of the lowest case whose hotspot is the largest, so ties go to the lowest case and then
    to the lowest global face.

    One indexing, one assembly and one block solve of k columns; the face and cut kernels then walk all columns of the V
    the device holds and reduce over the cases there.  With ``per_case_fields=False`` the device neither writes nor sends
    home any per-case J or |J|: ``vectors`` and ``magnitudes`` of every report are None and everything else has the same
    bits.  One case goes through the same path.  ValueError, before anything reaches the device, for invalid cases
    (:func:`check_load_cases`), invalid cuts (:func:`check_cuts`) and a ``partition`` over several GPUs.  ``timings`` (a
    dict) receives the host time of each step in seconds."""
    _refuse_partition(partition, "load-case currents")
    cases = check_load_cases(prob, cases)
    laps = _Laps(timings)
    solutions, reports, (board, pairs, flows_by_case, env, env_case) = _solve_block_currents(
        prob, meshes, mesh_index_to_layer_index, cases, check_cuts(prob, cuts), bool(per_case_fields), True, filtered_networks,
        disconnected_meshes_by_layer, laps)
    # the envelope: per face from the device, everything else by the same rule from the per-case scalars
    env_forms, env_cases, env_hotspots = [], [], []
    for layer_i in range(len(prob.layers)):
        forms, which = [], []
        for _mesh_i, msh, lo, hi in board.layer_meshes(layer_i):
            tf = mesh.TwoForm(msh)
            if env is not None:
                tf.values = env[lo:hi]
            forms.append(tf)
            which.append(env_case[lo:hi] if env is not None else np.zeros(len(msh.triangles), dtype=np.int32))
        env_forms.append(forms)
        env_cases.append(which)
        spots = [rep.hotspots[layer_i] for rep in reports]
        if spots[0] is None:
            env_hotspots.append(None)
        else:
            c = int(envelope_of([[spot[0]] for spot in spots])[1][0])
            env_hotspots.append((spots[c][0], c, *spots[c][1:]))
    env_elements = {}
    for i, (element, _) in enumerate(pairs):
        keys = list(flows_by_case[0][i])
        env_elements[element] = dict(zip(keys, _signed_envelope([[flows[i][key] for key in keys] for flows in flows_by_case])))
    envelope = CurrentEnvelope(magnitudes=env_forms, cases=env_cases, hotspots=env_hotspots,
                               layers=_signed_envelope([rep.layers for rep in reports]), elements=env_elements,
                               cuts=_signed_envelope([rep.cuts for rep in reports]))
    laps.lap("solutions")
    return solutions, reports, envelope


def solve_load_case_currents(prob, cases, cuts=(), mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None,
                             per_case_fields=True, partition=None, prune=False):
    """``solve`` for several load cases with their currents and the envelope (see
    :func:`solve_meshed_load_case_currents`): the board is meshed once."""
    _refuse_partition(partition, "load-case currents")
    cases = check_load_cases(prob, cases)
    cuts = check_cuts(prob, cuts)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_load_case_currents(prob, meshes, mesh_index_to_layer_index, cases,
                                           [Cut(prob.layers[i], a, b) for i, a, b in cuts], per_case_fields=per_case_fields, **pruned)


# --------------------------------------------------------------------------------------------
# thermal: the steady-state temperature of the copper from its Joule heating (DESIGN.md "Thermal")
# --------------------------------------------------------------------------------------------

LORENZ_NUMBER = 2.44e-8                 # L0 [W Ohm / K^2] of Wiedemann-Franz: kappa = L0 T sigma for a metal
MAX_HEAT_SOURCES = 4096
MAX_HEAT_SOURCE_VERTICES = 256


@dataclass
class HeatSource:
    """A component that dissipates into the copper under its footprint (DESIGN.md "Heat sources").

    - ``layer``: the layer, or its name.
    - ``polygon``: array-like (n, 2), n >= 3, in mesh units: the footprint.  Inside is decided by the even-odd rule, so a
      self-intersecting polygon is whatever that rule makes of it; footprints may overlap.
    - ``power``: the watts it dissipates, a float for every load case or a sequence with one entry per case.
    - ``name``: what the report and the error messages call it."""
    layer: object
    polygon: object
    power: object
    name: Optional[str] = None

    @classmethod
    def rectangle(cls, layer, x0, y0, x1, y1, power, name=None) -> "HeatSource":
        """The axis-parallel rectangle with the corners (x0, y0) and (x1, y1)."""
        return cls(layer, [(x0, y0), (x1, y0), (x1, y1), (x0, y1)], power, name)

    @classmethod
    def disc(cls, layer, centre, radius, power, segments=32, name=None) -> "HeatSource":
        """The regular polygon of ``segments`` vertices on the circle of ``radius`` around ``centre``, the first at angle 0."""
        angles = 2.0 * np.pi * np.arange(int(segments)) / int(segments)
        ring = np.stack([centre[0] + radius * np.cos(angles), centre[1] + radius * np.sin(angles)], axis=1)
        return cls(layer, ring, power, name)


@dataclass(frozen=True)
class CheckedHeatSource:
    """A :class:`HeatSource` resolved against a Problem (:func:`check_thermal_model`)."""
    name: str
    layer: int                 # index into Problem.layers
    polygon: tuple             # ((x, y), ...)
    power: object              # float, or a tuple of floats (one per load case)


MAX_FILM_KNOTS = 64
FILM_TOLERANCE = 0.01                   # [K] the defaults of ElectroThermalModel.tolerance and .max_rounds
FILM_MAX_ROUNDS = 20


class FilmCurve:
    """A film coefficient that depends on the temperature rise (DESIGN.md "Film curves"): ``film[i]`` [W / (K mesh-unit^2)]
    at the knots ``rise[i]`` [K above ambient], linear between the knots, held constant below the first knot and above the
    last.  A table, not a formula: it takes measured or CFD data as well as the textbook laws, and the device evaluates it
    with + - * only.  :func:`check_film_curve` states the rules; the constructor only copies."""

    def __init__(self, rise, film):
        self.rise = np.array(rise, dtype=DTYPE).reshape(-1)
        self.film = np.array(film, dtype=DTYPE).reshape(-1)

    def __repr__(self):
        return f"FilmCurve({len(self.rise)} knots, h(0)={self.film[0] if len(self.film) else None!r})"

    def __call__(self, theta):
        """h at the rises ``theta``, by the rule above (host arithmetic: np.interp, not the device's order)."""
        return np.interp(np.asarray(theta, dtype=DTYPE), self.rise, self.film)

    def is_constant(self) -> bool:
        """Every knot has the first knot's film: the curve is the float ``film[0]``."""
        return bool((self.film == self.film[0]).all())

    def __add__(self, other):
        if isinstance(other, FilmCurve):
            if self.rise.shape != other.rise.shape or not np.array_equal(self.rise, other.rise):
                raise ValueError("two film curves are added knot by knot: their rises must be equal")
            return FilmCurve(self.rise, self.film + other.film)
        if isinstance(other, (int, float, np.integer, np.floating)) and not isinstance(other, bool):
            return FilmCurve(self.rise, self.film + float(other))
        return NotImplemented

    __radd__ = __add__

    @classmethod
    def constant(cls, h) -> "FilmCurve":
        """The one-knot curve of the float ``h``."""
        return cls([0.0], [h])

    @classmethod
    def tabulate(cls, fn, upto, knots: int = 33) -> "FilmCurve":
        """``fn`` (rise -> h, vectorised) at ``knots`` knots ``upto * (i / (knots - 1))^2``: dense near 0, where a law like
        theta^(1/4) is steep."""
        knots = int(knots)
        if not 2 <= knots <= MAX_FILM_KNOTS:
            raise ValueError(f"a tabulated film curve has between 2 and {MAX_FILM_KNOTS} knots, not {knots}")
        upto = _positive_number(upto, "upto")
        rise = upto * (np.arange(knots, dtype=DTYPE) / (knots - 1)) ** 2
        return cls(rise, np.asarray(fn(rise), dtype=DTYPE))

    @classmethod
    def natural_convection(cls, coefficient, exponent=0.25, *, upto, knots: int = 33) -> "FilmCurve":
        """h = coefficient * rise^exponent, the law of natural convection from a plate.  h(0) of the law is 0, which no film
        may be: the first knot takes the value of the second, so the law holds from the second knot on."""
        coefficient = _positive_number(coefficient, "the coefficient")
        curve = cls.tabulate(lambda t: coefficient * t ** float(exponent), upto, knots)
        if curve.film[0] == 0.0:
            curve.film[0] = curve.film[1]
        return curve

    @classmethod
    def radiation(cls, emissivity_sigma, ambient_kelvin, *, upto, knots: int = 33) -> "FilmCurve":
        """h = emissivity_sigma ((Ta + rise)^2 + Ta^2) ((Ta + rise) + Ta), radiation to surroundings at ``ambient_kelvin``.
        ``emissivity_sigma`` in mesh units: 5.67e-14 W/(mm^2 K^4) for a black surface with meshes in mm."""
        es, ta = _positive_number(emissivity_sigma, "emissivity_sigma"), _positive_number(ambient_kelvin, "ambient_kelvin")
        return cls.tabulate(lambda t: es * ((ta + t) ** 2 + ta ** 2) * ((ta + t) + ta), upto, knots)


def check_film_curve(curve, what: str = "the film curve") -> FilmCurve:
    """``curve`` as a checked copy, or ValueError -- before anything reaches the device -- for: no FilmCurve; fewer than 1
    or more than 64 knots, or as many rises as films not; a value that is not finite; a film that is not positive; a
    ``rise`` that does not start at 0 or does not ascend strictly; and a loss density q(theta) = h(theta) theta that does
    not increase strictly for theta >= 0 -- on segment i with the slope s_i = (h_i+1 - h_i) / (t_i+1 - t_i) the derivative
    q' = h_i + s_i (2 theta - t_i) must be positive at both ends; the message names the segment.  A curve that falls that
    fast has more than one steady state."""
    if not isinstance(curve, FilmCurve):
        raise ValueError(f"{what} must be a FilmCurve, not {curve!r}")
    rise, film = np.array(curve.rise, dtype=DTYPE).reshape(-1), np.array(curve.film, dtype=DTYPE).reshape(-1)
    if rise.shape != film.shape:
        raise ValueError(f"{what}: {len(rise)} rises and {len(film)} films; one film per knot")
    if not 1 <= len(rise) <= MAX_FILM_KNOTS:
        raise ValueError(f"{what} has {len(rise)} knots: between 1 and {MAX_FILM_KNOTS} are taken")
    if not (np.isfinite(rise).all() and np.isfinite(film).all()):
        raise ValueError(f"{what}: every rise and every film must be finite")
    if not (film > 0.0).all():
        raise ValueError(f"{what}: every film coefficient must be positive (knot {int(np.flatnonzero(~(film > 0.0))[0])})")
    if rise[0] != 0.0:
        raise ValueError(f"{what}: the first knot must be at a rise of 0, not {rise[0]!r}")
    if not (np.diff(rise) > 0.0).all():
        raise ValueError(f"{what}: the rises must ascend strictly (knot {int(np.flatnonzero(~(np.diff(rise) > 0.0))[0]) + 1})")
    for i in range(len(rise) - 1):
        s = (film[i + 1] - film[i]) / (rise[i + 1] - rise[i])
        left, right = film[i] + s * (2 * rise[i] - rise[i]), film[i] + s * (2 * rise[i + 1] - rise[i])
        if not (math.isfinite(s) and left > 0.0 and right > 0.0):
            raise ValueError(f"{what} falls too fast on segment {i} ({rise[i]!r} K to {rise[i + 1]!r} K): the loss density "
                             "h(theta) theta must increase strictly")
    return FilmCurve(rise, film)


@dataclass
class ThermalModel:
    """What turns dissipated power into a temperature (see :func:`solve_meshed_thermal`).

    - ``film``: the film coefficient h [W / (K mesh-unit^2)] that lumps every loss from the sheet to ambient, one float for
      all layers or a mapping {layer or layer name: float} that names every layer.  Required: there is no sensible
      default.  With meshes in mm, 10 W/(m^2 K) is 1e-5.  In the place of any float a :class:`FilmCurve`: a film that
      depends on the temperature rise (DESIGN.md "Film curves"), honoured by the steady and the electro-thermal calls by
      Newton rounds and refused by the others.
    - ``film_tolerance`` [K] and ``film_max_rounds``: the Newton loop on a film curve ends when no vertex moved by more than
      the tolerance in a round, or after that many rounds with a SolverWarning.
    - ``ambient``: the ambient temperature, in the unit the temperatures are reported in.
    - ``sheet_conductance``: None, or a mapping {layer or name: kappa [W/K]}, the thermal conductance of a square of the
      sheet.  A layer that is not named gets Wiedemann-Franz, kappa = L0 T_ref layer.conductance.
    - ``link_conductance``: None, or a mapping {Resistor: g [W/K]}, the thermal conductance between the resistor's
      terminals; 0 is no link.  A resistor that is not named gets g = L0 T_ref / R.  Sources and regulators are no
      thermal path.
    - ``element_heat``: half of every resistor's dissipation is put into each of its terminals.
    - ``reference_temperature``: T_ref [K] of the Wiedemann-Franz defaults.
    - ``interlayer``: None, or a mapping {(layer or name, layer or name): g [W / (K mesh-unit^2)]}, the areal conductance
      of the dielectric between two layers (DESIGN.md "Stack").  The Problem carries no z-order, so the pairs are named
      and need not be neighbours; 0 is no pair.  0.2 mm of FR4 (0.3 W/(m K)) between two foils is 1.5e-3 with meshes in
      mm, 150 times the still-air film above.  Only the connected meshes take part: electrically disconnected copper
      stays at ambient and spreads no heat.
    - ``heat_sources``: None, or a sequence of :class:`HeatSource` (DESIGN.md "Heat sources"): components that put watts
      into the copper under their footprints, on top of the Joule heat.  A source loads the faces of the connected meshes
      of its layer whose centroid lies inside its polygon, each with the share area_f / A_s of its power (A_s the area of
      those faces together), a third of it at each corner; a footprint that covers no centroid (an 0402 on a coarse mesh)
      loads the one face that contains the mean of its vertices.  The power is per load case: a float serves every case,
      a sequence names one per case and is checked against the cases by the solve.  A source that lies on no connected
      copper is a ValueError of the solve.  At most 4096 sources of at most 256 vertices each.  Honoured by every thermal
      entry point: steady, load cases, electro-thermal (the same watts in every round, not scaled by the resistivity) and
      transient (a segment without a case has no source heat)."""
    film: object
    ambient: float = 25.0
    sheet_conductance: Optional[Mapping] = None
    link_conductance: Optional[Mapping] = None
    element_heat: bool = True
    reference_temperature: float = 293.15
    interlayer: Optional[Mapping] = None
    heat_sources: Optional[Sequence] = None
    film_tolerance: float = FILM_TOLERANCE
    film_max_rounds: int = FILM_MAX_ROUNDS


@dataclass
class CheckedThermalModel:
    """A :class:`ThermalModel` resolved against a Problem (:func:`check_thermal_model`)."""
    film: list                 # per layer: the float, or h(0) of the layer's curve
    kappa: list                # per layer
    links: dict                # Resistor of the solved networks -> g [W/K]
    ambient: float
    element_heat: bool
    interlayer: list = field(default_factory=list)      # (layer index a < b, g [W / (K mesh-unit^2)]), in the mapping's order
    sources: list = field(default_factory=list)         # CheckedHeatSource, in the model's order
    film_curves: Optional[list] = None                  # per layer: the checked FilmCurve, or None for a float; None: floats only
    film_tolerance: float = FILM_TOLERANCE
    film_max_rounds: int = FILM_MAX_ROUNDS

    def curved(self) -> bool:
        """Some layer's film depends on the temperature: the solve is a Newton loop.  Constant curves are floats."""
        return self.film_curves is not None and any(c is not None and not c.is_constant() for c in self.film_curves)


@dataclass
class ThermalReport:
    """The temperatures of one load case (see :func:`solve_meshed_thermal`)."""
    temperatures: Optional[list]        # per layer, per mesh: ZeroForm of T = theta + ambient at the vertices
    face_temperatures: Optional[list]   # per layer, per mesh: TwoForm of the mean T of each face's corners
    disconnected_temperatures: list     # per layer, per disconnected mesh: ZeroForm filled with the ambient temperature
    hotspots: list                      # per layer: (T, mesh index within the layer, vertex index, x, y), None without vertices
    layers: list                        # per layer: {"heat": the Joule heat put into its copper [W], "loss": its film loss [W],
                                        # "exchange": the net heat that leaves it through the pairs of ``interlayer`` [W]}
    elements: dict                      # Resistor -> {"heat": dissipation deposited at its terminals [W], "flow": heat a -> b through its link [W]}
    total_heat: float                   # copper and elements
    total_loss: float                   # what the films carry to ambient: equals total_heat up to the solve's tolerance
    info: dict                          # {"iterations", "rel_residual", "seconds"} of the thermal block solve
    # per pair of ThermalModel.interlayer: {"layers": (index a, index b), a < b, "conductance": g, "flow": the heat from a to
    # b through the dielectric [W], "area": the coupled area [mesh-unit^2]}
    interlayer: list = field(default_factory=list)
    # per source of ThermalModel.heat_sources: {"name", "layer": index, "power": of this case [W], "area": A_s, the area of
    # the faces it loads [mesh-unit^2], "faces": their number, "fallback": True when it covers no centroid and loads the
    # one face under its middle, "temperature": the area-weighted mean of those faces' temperatures}
    sources: list = field(default_factory=list)
    source_heat: float = 0.0            # the powers of the sources in this case; part of total_heat
    # None, or for a model with film curves how the Newton loop on the film went: {"rounds", "increments": per round the
    # largest change of a vertex temperature [K], "vertices": the global vertex of each, "converged", "beyond": the
    # vertices above the last knot of their curve, where it is held constant}.  ``info`` is then that of the last solve,
    # and every loss is sum_v M_v h(theta_v) theta_v
    film: Optional[dict] = None


@dataclass
class ThermalEnvelope:
    """The worst case over the load cases of one block (the sequential rule of :func:`envelope_of`)."""
    temperatures: list    # per layer, per mesh: ZeroForm of max_j T_j per vertex
    cases: list           # per layer, per mesh: (n_vertices,) int32, the lowest case of that maximum
    hotspots: list        # per layer: (T, case, mesh index within the layer, vertex index, x, y), None without vertices


_TERMINAL_FIELDS = {"Resistor": ("a", "b"), "CurrentSource": ("f", "t"), "VoltageSource": ("p", "n"),
                    "VoltageRegulator": ("v_p", "v_n", "s_f", "s_t")}


def _positive_number(value, what: str, allow_zero: bool = False) -> float:
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number, not {value!r}") from None
    if not math.isfinite(x) or x < 0.0 or (x == 0.0 and not allow_zero):
        raise ValueError(f"{what} must be finite and {'not negative' if allow_zero else 'positive'}, not {value!r}")
    return x


def _per_layer(prob, mapping, what: str, value_of=None) -> dict:
    """{layer index: value} of a mapping {layer or layer name: value}; ValueError for a key that is no layer of ``prob``.
    ``value_of(value, what)``: the check of a value, a positive number by default."""
    value_of = _positive_number if value_of is None else value_of
    out = {}
    for key, value in mapping.items():
        if isinstance(key, str):
            found = [i for i, layer in enumerate(prob.layers) if layer.name == key]
        else:
            found = [i for i, layer in enumerate(prob.layers) if layer is key or layer == key]
        if not found:
            raise ValueError(f"{what}: {key!r} is no layer of the Problem")
        for i in found:
            out[i] = value_of(value, f"{what} of layer {prob.layers[i].name!r}")
    return out


def check_thermal_model(prob, model, filtered_networks=None) -> CheckedThermalModel:
    """``model`` resolved against ``prob``, or ValueError -- before anything reaches the device -- for: a film that is
    missing for a layer; a film, sheet conductance or reference temperature that is not finite and positive; a link
    conductance that is negative or not finite (0 is allowed: no link); a mapping key that is no layer, or no Resistor, of
    the Problem; an ``interlayer`` key that is not a 2-tuple of layers of the Problem, that pairs a layer with itself or
    that repeats an unordered pair, or an ``interlayer`` conductance that is negative or not finite (0 is allowed: no
    pair); ``heat_sources`` that is no sequence of :class:`HeatSource` or holds more than 4096, a source whose layer is no
    layer of the Problem or names several, whose polygon is not (n >= 3, 2), not finite, of zero signed area or of more
    than 256 vertices, or whose power is negative, not finite or not a number (the length of a sequence of powers is
    checked against the load cases by the solve); an ambient temperature that is not finite; and an internal node (a terminal without a connection to
    copper) that reaches no copper through links of positive conductance -- its temperature would be undetermined.  That
    last check walks a small graph over the lumped elements only, and the error names an element at the node."""
    if not isinstance(model, ThermalModel):
        raise ValueError("model must be a ThermalModel")
    networks = list(prob.networks) if filtered_networks is None else list(filtered_networks)
    t_ref = _positive_number(model.reference_temperature, "the reference temperature")
    try:
        ambient = float(model.ambient)
    except (TypeError, ValueError):
        raise ValueError(f"the ambient temperature must be a number, not {model.ambient!r}") from None
    if not math.isfinite(ambient):
        raise ValueError(f"the ambient temperature must be finite, not {model.ambient!r}")
    n_layers = len(prob.layers)
    if model.film is None:
        raise ValueError("the film coefficient is required: a float, or a mapping {layer: float}")
    def film_of(value, what):
        return check_film_curve(value, what) if isinstance(value, FilmCurve) else _positive_number(value, what)

    if isinstance(model.film, Mapping):
        given = _per_layer(prob, model.film, "film", film_of)
        for i, layer in enumerate(prob.layers):
            if i not in given:
                raise ValueError(f"layer {layer.name!r} has no film coefficient")
        film = [given[i] for i in range(n_layers)]
    else:
        film = [film_of(model.film, "the film coefficient")] * n_layers
    film_curves = [f if isinstance(f, FilmCurve) else None for f in film]
    film = [float(f.film[0]) if isinstance(f, FilmCurve) else f for f in film]
    film_tolerance = _positive_number(model.film_tolerance, "film_tolerance")
    try:
        film_max_rounds = int(model.film_max_rounds)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"film_max_rounds must be an integer, not {model.film_max_rounds!r}") from None
    if film_max_rounds < 1 or film_max_rounds != model.film_max_rounds:
        raise ValueError(f"film_max_rounds must be an integer of at least 1, not {model.film_max_rounds!r}")
    given = {} if model.sheet_conductance is None else _per_layer(prob, model.sheet_conductance, "sheet_conductance")
    kappa = []
    for i, layer in enumerate(prob.layers):
        kappa.append(given[i] if i in given else
                     _positive_number(LORENZ_NUMBER * t_ref * float(layer.conductance),
                                      f"the Wiedemann-Franz sheet conductance of layer {layer.name!r}"))
    all_elements = [element for network in prob.networks for element in network.elements]
    overrides = {}
    if model.link_conductance is not None:
        if not isinstance(model.link_conductance, Mapping):
            raise ValueError("link_conductance must be a mapping {Resistor: W/K}")
        for key, value in model.link_conductance.items():
            if not any(element is key or element == key for element in all_elements):
                raise ValueError(f"link_conductance: {key!r} is no element of the Problem")
            if element_kind(key) != "Resistor":
                raise ValueError(f"link_conductance: a {type(key).__name__} is no thermal path, only resistors are")
            overrides[key] = _positive_number(value, "the link conductance of a Resistor", allow_zero=True)
    links = {}
    for network in networks:
        for element in network.elements:
            if element_kind(element) == "Resistor":
                links[element] = overrides[element] if element in overrides else \
                    _positive_number(LORENZ_NUMBER * t_ref / float(element.resistance), "the Wiedemann-Franz link conductance")
    # every internal node must reach copper through links of positive conductance
    on_copper = {conn.node_id for network in networks for conn in network.connections}
    neighbours: dict = {}
    at_node: dict = {}
    for network in networks:
        for element in network.elements:
            kind = element_kind(element)
            if kind is None:
                raise NotImplementedError(f"Unsupported node type {element}")
            nodes = [getattr(element, name) for name in _TERMINAL_FIELDS[kind]]
            for node in nodes:
                at_node.setdefault(node, element)
                neighbours.setdefault(node, [])
            if kind == "Resistor" and links[element] > 0.0:
                neighbours[nodes[0]].append(nodes[1])
                neighbours[nodes[1]].append(nodes[0])
    reached = {node for node in neighbours if node in on_copper}
    stack = list(reached)
    while stack:
        for other in neighbours[stack.pop()]:
            if other not in reached:
                reached.add(other)
                stack.append(other)
    for node, element in at_node.items():
        if node not in reached:
            raise ValueError(f"an internal node of {element!r} reaches no copper through a thermal link of positive conductance: "
                             "its temperature is undetermined (give a resistor at the node a link_conductance above 0)")
    return CheckedThermalModel(film=film, kappa=kappa, links=links, ambient=ambient, element_heat=bool(model.element_heat),
                               interlayer=_check_interlayer(prob, model.interlayer),
                               sources=_check_heat_sources(prob, model.heat_sources),
                               film_curves=film_curves if any(c is not None for c in film_curves) else None,
                               film_tolerance=film_tolerance, film_max_rounds=film_max_rounds)


def _refuse_film_curves(checked: CheckedThermalModel, what: str) -> None:
    """ValueError for a model whose film depends on the temperature, in a call that reads the film as a constant."""
    if checked.curved():
        raise ValueError(f"{what} does not honour a film curve that depends on the temperature: only the steady "
                         "(solve_thermal) and the electro-thermal (solve_electrothermal) calls iterate on the film; give this "
                         "call floats or constant curves")


def _check_heat_sources(prob, heat_sources) -> list:
    """``ThermalModel.heat_sources`` resolved to [CheckedHeatSource], or ValueError (see :func:`check_thermal_model`)."""
    if heat_sources is None:
        return []
    if isinstance(heat_sources, (str, bytes, Mapping, HeatSource)) or not isinstance(heat_sources, (Sequence, np.ndarray)):
        raise ValueError("heat_sources must be a sequence of HeatSource")
    if len(heat_sources) > MAX_HEAT_SOURCES:
        raise ValueError(f"heat_sources: {len(heat_sources)} sources, at most {MAX_HEAT_SOURCES} are taken")

    def watts(value, what):
        if isinstance(value, (str, bytes)) or value is None:
            raise ValueError(f"heat_sources: the power of {what} must be a number, not {value!r}")
        try:
            x = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"heat_sources: the power of {what} must be a number, not {value!r}") from None
        if not math.isfinite(x) or x < 0.0:
            raise ValueError(f"heat_sources: the power of {what} must be finite and not negative, not {value!r}")
        return x

    out = []
    for i, source in enumerate(heat_sources):
        if not isinstance(source, HeatSource):
            raise ValueError(f"heat_sources: entry {i} is no HeatSource but {source!r}")
        name = f"source {i}" if source.name is None else str(source.name)
        key = source.layer
        if isinstance(key, str):
            found = [l for l, layer in enumerate(prob.layers) if layer.name == key]
        else:
            found = [l for l, layer in enumerate(prob.layers) if layer is key] or \
                    [l for l, layer in enumerate(prob.layers) if layer == key]
        if len(found) != 1:
            raise ValueError(f"heat_sources: the layer {key!r} of {name!r} is no layer of the Problem" if not found else
                             f"heat_sources: the layer {key!r} of {name!r} names {len(found)} layers of the Problem")
        try:
            polygon = np.array(source.polygon, dtype=DTYPE)
        except (TypeError, ValueError):
            raise ValueError(f"heat_sources: the polygon of {name!r} must be array-like of shape (n, 2)") from None
        if polygon.ndim != 2 or polygon.shape[1] != 2 or polygon.shape[0] < 3:
            raise ValueError(f"heat_sources: the polygon of {name!r} must have shape (n >= 3, 2), not {polygon.shape}")
        if polygon.shape[0] > MAX_HEAT_SOURCE_VERTICES:
            raise ValueError(f"heat_sources: the polygon of {name!r} has {polygon.shape[0]} vertices, at most "
                             f"{MAX_HEAT_SOURCE_VERTICES} are taken")
        if not np.isfinite(polygon).all():
            raise ValueError(f"heat_sources: the polygon of {name!r} must be finite")
        x, y = polygon[:, 0], polygon[:, 1]
        signed = math.fsum((x * np.roll(y, -1) - np.roll(x, -1) * y).tolist())
        if not math.isfinite(signed) or signed == 0.0:
            raise ValueError(f"heat_sources: the polygon of {name!r} has no area")
        power = source.power
        if isinstance(power, (Sequence, np.ndarray)) and not isinstance(power, (str, bytes)) and np.ndim(power) > 0:
            if np.ndim(power) != 1:
                raise ValueError(f"heat_sources: the power of {name!r} must be a number or a sequence of numbers")
            power = tuple(watts(p, f"{name!r} in case {j}") for j, p in enumerate(power))
        else:
            power = watts(power, repr(name))
        out.append(CheckedHeatSource(name=name, layer=found[0], polygon=tuple((float(a), float(b)) for a, b in polygon), power=power))
    return out


def _source_powers(sources: list, n_cases: int) -> Optional[np.ndarray]:
    """The powers (n_cases, n_sources) of the checked ``sources``, or None without sources; ValueError for a source whose
    sequence of powers does not have one entry per case."""
    if not sources:
        return None
    out = np.zeros((n_cases, len(sources)), dtype=DTYPE)
    for i, source in enumerate(sources):
        if isinstance(source.power, tuple):
            if len(source.power) != n_cases:
                raise ValueError(f"heat_sources: {source.name!r} names {len(source.power)} powers, the solve has {n_cases} "
                                 "load case(s)")
            out[:, i] = source.power
        else:
            out[:, i] = source.power
    return out


def _attach_heat_sources(thermal, prob, checked: CheckedThermalModel, layer_of, n_mesh: int):
    """The checked model's heat sources given to the handle ``thermal``: None without sources, else a namespace of what
    ``Thermal.set_sources`` returns -- ``faces``, ``fallback`` and ``area`` per source.  ValueError for sources on no
    connected copper, naming them and their layers."""
    if not checked.sources:
        return None
    try:
        faces, fallback, area = thermal.set_sources(len(prob.layers), [layer_of[i] for i in range(n_mesh)],
                                                    [source.layer for source in checked.sources],
                                                    [np.asarray(source.polygon, dtype=DTYPE) for source in checked.sources])
    except _hip.SourceOffCopperError as exc:
        lost = [checked.sources[i] for i in exc.sources]
        raise ValueError("heat_sources: " + ", ".join(f"{source.name!r} on layer {prob.layers[source.layer].name!r}" for source in lost)
                         + (" lies" if len(lost) == 1 else " lie") + " on no connected copper: neither a face centroid under "
                         "the footprint nor a face under its middle") from None
    return types.SimpleNamespace(faces=faces, fallback=fallback, area=area)


def _source_entries(checked: CheckedThermalModel, attached, powers, rises, j: int) -> tuple:
    """(``ThermalReport.sources``, ``source_heat``) of case ``j``: ``attached`` as :func:`_attach_heat_sources` returns it,
    ``powers`` (k, n) and ``rises`` (k, n) the footprint temperatures above ambient; ([], 0.0) without sources."""
    if attached is None:
        return [], 0.0
    entries = [{"name": source.name, "layer": source.layer, "power": float(powers[j, i]), "area": float(attached.area[i]),
                "faces": int(attached.faces[i]), "fallback": bool(attached.fallback[i]),
                "temperature": float(checked.ambient + rises[j, i])} for i, source in enumerate(checked.sources)]
    return entries, math.fsum(powers[j].tolist())


def _check_interlayer(prob, interlayer) -> list:
    """``ThermalModel.interlayer`` resolved to [(layer index a < b, g)], or ValueError (see :func:`check_thermal_model`)."""
    if interlayer is None:
        return []
    if not isinstance(interlayer, Mapping):
        raise ValueError("interlayer must be a mapping {(layer, layer): W/(K mesh-unit^2)}")

    def index_of(key):
        if isinstance(key, str):
            found = [i for i, layer in enumerate(prob.layers) if layer.name == key]
        else:
            found = [i for i, layer in enumerate(prob.layers) if layer is key] or \
                    [i for i, layer in enumerate(prob.layers) if layer == key]
        if len(found) != 1:
            raise ValueError(f"interlayer: {key!r} is no layer of the Problem" if not found else
                             f"interlayer: {key!r} names {len(found)} layers of the Problem")
        return found[0]

    out, seen = [], set()
    for key, value in interlayer.items():
        if not isinstance(key, tuple) or len(key) != 2:
            raise ValueError(f"interlayer: a key is a pair (layer, layer), not {key!r}")
        a, b = index_of(key[0]), index_of(key[1])
        if a == b:
            raise ValueError(f"interlayer: {key!r} pairs layer {prob.layers[a].name!r} with itself")
        a, b = min(a, b), max(a, b)
        if (a, b) in seen:
            raise ValueError(f"interlayer: the layers {prob.layers[a].name!r} and {prob.layers[b].name!r} are paired twice")
        seen.add((a, b))
        out.append((a, b, _positive_number(value, f"the interlayer conductance of {key!r}", allow_zero=True)))
    return out


def _thermal_handle(L, n_potential: int, checked: CheckedThermalModel, layer_of, n_mesh: int, resistors) -> "_hip.Thermal":
    """The ``_hip.Thermal`` of the checked model on the assembled system ``L``; with ``interlayer`` pairs the stacked one."""
    stack = {}
    if checked.interlayer:
        stack = dict(mesh_layer=[layer_of[i] for i in range(n_mesh)], pairs=checked.interlayer, n_layer=len(checked.film))
    thermal = _hip.Thermal(L.dev, n_potential, [checked.kappa[layer_of[i]] for i in range(n_mesh)],
                           [checked.film[layer_of[i]] for i in range(n_mesh)],
                           [row[1] for _, row in resistors], [row[2] for _, row in resistors],
                           [checked.links[element] for element, _ in resistors], **stack)
    if checked.curved():                     # (floats and constant curves: the handle of the float path, untouched)
        try:
            thermal.set_film_curves([_film_table(checked, layer_of[i]) for i in range(n_mesh)])
        except BaseException:
            thermal.close()
            raise
    return thermal


def _film_table(checked: CheckedThermalModel, layer_i: int) -> tuple:
    """(rise, film) of a layer of a checked model with curves; a float is the table of one knot."""
    curve = checked.film_curves[layer_i]
    return ([0.0], [checked.film[layer_i]]) if curve is None else (curve.rise, curve.film)


def _stack_flows(thermal, checked: CheckedThermalModel, n_cols: int):
    """(flows (n_cols, n_pair), areas (n_pair,)) of the last solve of ``thermal`` for the model's pairs, or None without."""
    return thermal.stack_flows(n_cols) if checked.interlayer else None


def _refuse_bare_vertices(board: IndexedBoard) -> None:
    """ValueError for a vertex of a connected mesh that no face names: the thermal system has no equation for it."""
    for mesh_i, msh in enumerate(board.meshes):
        used = np.bincount(np.asarray(msh.triangles, dtype=np.int64).reshape(-1), minlength=len(msh.points))
        if len(msh.points) and (used[:len(msh.points)] == 0).any():
            raise ValueError(f"mesh {mesh_i} has a vertex without a face ({int(np.flatnonzero(used == 0)[0])}): the thermal "
                             "model has no equation for it")


def thermal_heat_triples(pairs, flows_by_case) -> tuple:
    """The node-heat triples (unknown, case, watts) that put half of every resistor's dissipation into each of its
    terminals, case by case in element order, terminal a before terminal b."""
    node, col, val = [], [], []
    for j, flows in enumerate(flows_by_case):
        for (_, row), flow in zip(pairs, flows):
            if row[0] == "R":
                half = flow["power"] / 2
                node += [row[1], row[2]]
                col += [j, j]
                val += [half, half]
    return np.asarray(node, dtype=np.int64), np.asarray(col, dtype=np.int32), np.asarray(val, dtype=DTYPE)


def _layer_hotspot(board: IndexedBoard, ambient: float, mesh_max, mesh_vert, j: int, layer_i: int, layer_meshes=None):
    """``ThermalReport.hotspots[layer_i]`` of case ``j`` from the per-mesh maxima (k, n_mesh) of ``Thermal.report``: (T, mesh
    index within the layer, vertex index, x, y), None for a layer without connected vertices.  ``layer_meshes``: the list of
    ``board.layer_meshes(layer_i)``, for a caller that asks row after row."""
    voff, best = board.vindex.offsets, None
    for in_layer, (mesh_i, msh, _lo, _hi) in enumerate(board.layer_meshes(layer_i) if layer_meshes is None else layer_meshes):
        # meshes come in global vertex order: a later mesh wins only with a strictly larger temperature
        if mesh_vert[j, mesh_i] >= 0 and (best is None or mesh_max[j, mesh_i] + ambient > best[0]):
            v = int(mesh_vert[j, mesh_i] - voff[mesh_i])
            best = (float(mesh_max[j, mesh_i] + ambient), in_layer, v, float(msh.points[v][0]), float(msh.points[v][1]))
    return best


def _cold_temperatures(board: IndexedBoard, ambient: float) -> list:
    """Per layer, per disconnected mesh: a ZeroForm filled with the ambient temperature."""
    cold = [[] for _ in board.prob.layers]
    for layer_i, out in enumerate(cold):
        for msh in board.disconnected_meshes_by_layer[layer_i]:
            msh = msh if isinstance(msh, mesh.Mesh) else mesh.Mesh.from_reference(msh)
            zf = mesh.ZeroForm(msh)
            zf.values = np.full(len(msh.vertices), ambient, dtype=DTYPE)
            out.append(zf)
    return cold


def _thermal_reports(board: IndexedBoard, checked: CheckedThermalModel, substituted, resistors, fields: bool, theta, mean,
                     mesh_max, mesh_vert, mesh_heat, mesh_loss, heat_val, infos, stack=None, sources=None) -> list:
    """The ThermalReports of k cases from what ``Thermal.report`` returns for them: ``theta`` (k, n_potential), ``mean`` (k,
    n_tri) or None without ``fields``, the per-mesh arrays (k, n_mesh), ``heat_val`` (k, n_resistors, 2) the heat put into the
    resistors' terminals or None, ``infos`` the info dict of each case.  ``substituted``: substitute_load_case of each case;
    ``resistors``: the (element, row) pairs of the board's resistors.  ``stack``: (flows (k, n_pair), areas (n_pair,)) of
    the model's ``interlayer`` pairs as ``Thermal.stack_flows`` returns them, or None without pairs.  ``sources``: (what
    :func:`_attach_heat_sources` returned, powers (k, n_source), footprint temperatures above ambient (k, n_source)) of the
    model's ``heat_sources``, or None without."""
    ambient, voff, n_layers = checked.ambient, board.vindex.offsets, len(board.prob.layers)
    reports = []
    for j, (_, renamed) in enumerate(substituted):
        case_resistors = [e for network in board.filtered_networks for e in renamed.get(id(network), network).elements
                          if element_kind(e) == "Resistor"]
        temps, faces, hotspots, layers = [], [], [], []
        for layer_i in range(n_layers):
            zfs, tfs, heat_in, loss = [], [], [], []
            best = _layer_hotspot(board, ambient, mesh_max, mesh_vert, j, layer_i)
            for in_layer, (mesh_i, msh, lo, hi) in enumerate(board.layer_meshes(layer_i)):
                heat_in.append(float(mesh_heat[j, mesh_i]))
                loss.append(float(mesh_loss[j, mesh_i]))
                if fields:
                    zf, tf = mesh.ZeroForm(msh), mesh.TwoForm(msh)
                    zf.values = theta[j, voff[mesh_i]:voff[mesh_i + 1]] + ambient
                    tf.values = mean[j, lo:hi] + ambient
                    zfs.append(zf)
                    tfs.append(tf)
            temps.append(zfs)
            faces.append(tfs)
            hotspots.append(best)
            exchange = [] if stack is None else [float(stack[0][j, p]) * (1.0 if a == layer_i else -1.0)
                                                 for p, (a, b, _) in enumerate(checked.interlayer) if layer_i in (a, b)]
            layers.append({"heat": math.fsum(heat_in), "loss": math.fsum(loss), "exchange": math.fsum(exchange)})
        interlayer = [] if stack is None else [
            {"layers": (a, b), "conductance": g, "flow": float(stack[0][j, p]), "area": float(stack[1][p])}
            for p, (a, b, g) in enumerate(checked.interlayer)]
        elements = {}
        for i, ((element, row), case_element) in enumerate(zip(resistors, case_resistors)):
            deposited = float(heat_val[j, i].sum()) if heat_val is not None else 0.0
            elements[case_element] = {"heat": deposited,
                                      "flow": float(checked.links[element] * (theta[j, row[1]] - theta[j, row[2]]))}
        total_heat = math.fsum([layer["heat"] for layer in layers] + [e["heat"] for e in elements.values()])
        entries, source_heat = ([], 0.0) if sources is None else _source_entries(checked, *sources, j)
        if sources is not None:
            total_heat = total_heat + source_heat
        reports.append(ThermalReport(
            temperatures=temps if fields else None, face_temperatures=faces if fields else None,
            disconnected_temperatures=_cold_temperatures(board, ambient), hotspots=hotspots, layers=layers,
            elements=elements, total_heat=total_heat,
            total_loss=math.fsum(layer["loss"] for layer in layers), info=infos[j], interlayer=interlayer, sources=entries,
            source_heat=source_heat))
    return reports


def _thermal_envelope(board: IndexedBoard, ambient: float, env, env_case, reports) -> ThermalEnvelope:
    """The ThermalEnvelope from the per-vertex maximum ``env`` of theta over the cases, the case ``env_case`` that attains it,
    and the cases' reports."""
    voff, n_layers, k = board.vindex.offsets, len(board.prob.layers), len(reports)
    env_temps, env_cases, env_hotspots = [], [], []
    for layer_i in range(n_layers):
        zfs, which = [], []
        for mesh_i, msh, _lo, _hi in board.layer_meshes(layer_i):
            zf = mesh.ZeroForm(msh)
            zf.values = env[voff[mesh_i]:voff[mesh_i + 1]] + ambient
            zfs.append(zf)
            which.append(env_case[voff[mesh_i]:voff[mesh_i + 1]])
        env_temps.append(zfs)
        env_cases.append(which)
        spots = [rep.hotspots[layer_i] for rep in reports]
        if spots[0] is None:
            env_hotspots.append(None)
        else:
            c = max(range(k), key=lambda j: (spots[j][0], -j))          # the lowest case of the largest temperature
            env_hotspots.append((spots[c][0], c, *spots[c][1:]))
    return ThermalEnvelope(temperatures=env_temps, cases=env_cases, hotspots=env_hotspots)


def _thermal_board(prob, meshes, mesh_index_to_layer_index, checked: CheckedThermalModel, cases, filtered_networks,
                   disconnected_meshes_by_layer, check=None) -> tuple:
    """What every thermal call does before anything reaches the device: (the indexed board, its ``global_elements`` pairs,
    ``substitute_load_case`` of every case, the heat sources' powers (k, n_source) or None, the number of vertices, k).
    ValueError for powers that are not one per case, a vertex without a face and a board without connected copper.
    ``check(board, pairs)``, if given, runs last."""
    substituted = [substitute_load_case(prob, case) for case in cases]
    k = len(cases)
    source_power = _source_powers(checked.sources, k)
    board = index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer)
    _refuse_bare_vertices(board)
    n_vert = len(board.vindex)
    if n_vert == 0 or not int(board.tri_offsets[-1]):
        raise ValueError("the thermal model needs connected copper: the board has no connected mesh with faces")
    pairs = global_elements(board.filtered_networks, board.node_indexer)
    if check is not None:
        check(board, pairs)
    return board, pairs, substituted, source_power, n_vert, k


@contextlib.contextmanager
def _thermal_block(prob, meshes, mesh_index_to_layer_index, checked: CheckedThermalModel, cases, filtered_networks,
                   disconnected_meshes_by_layer, laps: _Laps, what: str, check=None):
    """What the steady and the transient thermal paths share: the checked ``cases`` of ``prob`` solved as one electrical block
    on the load-case path, the element flows of every case, and the ``_hip.Thermal`` handle of the checked model on top of
    the assembled system.  A context: inside it the system, the plan and the handle live on the device; the value is a
    namespace of everything the two paths read.  On the way out the handle is closed and a stalled block is warned about.
    ``check``: see :func:`_thermal_board`."""
    board, pairs, substituted, source_power, n_vert, k = _thermal_board(
        prob, meshes, mesh_index_to_layer_index, checked, cases, filtered_networks, disconnected_meshes_by_layer, check)
    laps.lap("indexing")
    layer_of = board.layer_of
    with board.assembled() as (L, _):
        rows, cols, vals = stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], cases)
        laps.lap("assembly")
        log.info(f"Solving {k} load case(s) as one block, with their {what}")
        plan, V, residual_norms, res, n_tri, _n_mesh = _solve_block_on_device(L, rows, cols, vals, k, k, laps)
        power = plan.power_density_block(k, n_tri)
        local, Vu = _gather_element_rows([row for _, row in pairs], V, _ROW_UNKNOWNS)
        flows_by_case = [element_flows(_case_element_rows(pairs, local, case), Vu[:, j]) for j, case in enumerate(cases)]
        laps.lap("power_density")
        resistors = [(element, row) for element, row in pairs if row[0] == "R"]
        n_potential = L.layout.n_potential
        thermal = _thermal_handle(L, n_potential, checked, layer_of, len(board.meshes), resistors)
        try:
            sources = _attach_heat_sources(thermal, prob, checked, layer_of, len(board.meshes))
            if sources is not None:
                thermal.source_power(source_power)           # column j of every load carries the sources of case j
            laps.lap("thermal_setup")
            heat = thermal_heat_triples(pairs, flows_by_case) if checked.element_heat else None
            yield types.SimpleNamespace(board=board, substituted=substituted, pairs=pairs, resistors=resistors, plan=plan, V=V,
                                        residual_norms=residual_norms, res=res, n_tri=n_tri, n_vert=n_vert,
                                        n_potential=n_potential, power=power, thermal=thermal, heat=heat, k=k, sources=sources,
                                        source_power=source_power, L=L)
        finally:
            thermal.close()
    laps.lap()
    _warn_if_block_stalled(res, residual_norms, cols, vals, k)


def _block_solutions(blk) -> list:
    """The Solution of every case of a :func:`_thermal_block`."""
    return [_column_solution(blk.board, sub, np.ascontiguousarray(blk.V[:, j]), blk.residual_norms[j], blk.res, blk.power[j],
                             f"Load case {j}: " if blk.k > 1 else "") for j, (sub, _) in enumerate(blk.substituted)]


def _solve_block_thermal(prob, meshes, mesh_index_to_layer_index, checked: CheckedThermalModel, cases, fields: bool,
                         filtered_networks, disconnected_meshes_by_layer, laps: _Laps, check=None, inside=None):
    """The checked ``cases`` of ``prob`` as one electrical block and one thermal block on top of it, for the checked model:
    ([Solution], [ThermalReport], ThermalEnvelope).  ``fields``: with the per-case temperatures of vertices and faces.
    ``check``: see :func:`_thermal_block`.  ``inside(blk, theta, mesh_max, mesh_vert, sources)``, if given, runs after the reports
    have been read, while the block and the handle still live on the device; its value is returned as a fourth item."""
    if checked.curved():
        return _solve_block_thermal_curved(prob, meshes, mesh_index_to_layer_index, checked, cases, fields, filtered_networks,
                                           disconnected_meshes_by_layer, laps, check)
    extra = None
    with _thermal_block(prob, meshes, mesh_index_to_layer_index, checked, cases, filtered_networks,
                        disconnected_meshes_by_layer, laps, "temperatures", check) as blk:
        k, heat = blk.k, blk.heat
        theta, tres = blk.thermal.solve_kkt(blk.plan, k, heat, rtol=RTOL, max_iter=MAX_ITER)
        laps.lap("thermal_solve")
        mean, mesh_max, mesh_vert, mesh_heat, mesh_loss, env, env_case = blk.thermal.report(k, blk.n_tri, blk.n_vert, fields=fields)
        stack = _stack_flows(blk.thermal, checked, k)
        sources = None if blk.sources is None else (blk.sources, blk.source_power, blk.thermal.source_report(k))
        laps.lap("thermal_report")
        if inside is not None:
            extra = inside(blk, theta, mesh_max, mesh_vert, sources)
    if tres.status != _hip.OK and not tres.rel_residual <= max(RTOL, STALL_WARN_ABOVE):
        warnings.warn(f"The thermal solve stopped at a relative residual of {tres.rel_residual:.3e}", SolverWarning)
    board = blk.board
    solutions = _block_solutions(blk)
    info = {"iterations": int(tres.iterations), "rel_residual": float(tres.rel_residual), "seconds": float(tres.seconds)}
    heat_val = heat[2].reshape(k, len(blk.resistors), 2) if heat is not None else None
    reports = _thermal_reports(board, checked, blk.substituted, blk.resistors, fields, theta, mean, mesh_max, mesh_vert, mesh_heat,
                               mesh_loss, heat_val, [info] * k, stack, sources)
    envelope = _thermal_envelope(board, checked.ambient, env, env_case, reports)
    laps.lap("solutions")
    if inside is not None:
        return solutions, reports, envelope, extra
    return solutions, reports, envelope


def _film_layer_name(board: IndexedBoard, vertex: int) -> str:
    """The name of the layer of the global vertex ``vertex`` (-1: no vertex)."""
    if vertex < 0:
        return "?"
    mesh_i = int(np.searchsorted(np.asarray(board.vindex.offsets), vertex, side="right")) - 1
    return board.prob.layers[board.layer_of[mesh_i]].name


def _film_newton(thermal, first_solve, checked: CheckedThermalModel, where: str, board: IndexedBoard, rounds_log=None,
                 case: int = 0) -> tuple:
    """The Newton loop on the film curves of the handle ``thermal`` for one load: the film linearised about zero and
    ``first_solve()`` (today's linear solve with h(0)), then rounds of (linearise about the held theta, ``resolve``), each
    followed by ``film_increment``, until no vertex moved by more than ``checked.film_tolerance`` -- or
    ``checked.film_max_rounds`` end the loop with a SolverWarning that begins with ``where``.  (theta (1, n_potential), the
    SolveResult of the last solve, ``ThermalReport.film``).  On return hM of the handle is h(theta) M_v of the last iterate.
    ``rounds_log``: a list that receives the laps of every round."""
    increments, vertices, beyond, converged = [], [], 0, False
    theta = tres = None
    for round_i in range(1, checked.film_max_rounds + 1):
        lap = {}
        round_laps = _Laps(lap)
        thermal.film_linearise(round_i > 1)
        round_laps.lap("linearise")
        theta, tres = first_solve() if round_i == 1 else thermal.resolve(rtol=RTOL, max_iter=MAX_ITER)
        round_laps.lap("thermal_solve")
        increment, vertex, beyond = thermal.film_increment()
        round_laps.lap("increment")
        increments.append(increment)
        vertices.append(vertex)
        if rounds_log is not None:
            rounds_log.append(dict(lap, case=case, round=round_i, hierarchy=float(tres.setup_seconds),
                                   iterations=int(tres.iterations)))
        if increment <= checked.film_tolerance:
            converged = True
            break
    if not converged:
        warnings.warn(f"{where}: the film loop did not converge in {checked.film_max_rounds} round(s): the last change of a "
                      f"vertex temperature was {increments[-1]:.3e} K, on layer {_film_layer_name(board, vertices[-1])!r}, above "
                      f"the tolerance of {checked.film_tolerance:.3e} K", SolverWarning)
    return theta, tres, {"rounds": len(increments), "increments": increments, "vertices": vertices, "converged": converged,
                         "beyond": beyond}


def _solve_block_thermal_curved(prob, meshes, mesh_index_to_layer_index, checked: CheckedThermalModel, cases, fields: bool,
                                filtered_networks, disconnected_meshes_by_layer, laps: _Laps, check=None):
    """:func:`_solve_block_thermal` for a model with film curves: the electrical block and the face powers as there, then
    case by case the Newton loop of :func:`_film_newton` on the one-column thermal solve, with the one-column report, stack
    flows and source report of every case.  The envelope is :func:`envelope_of` the cases' theta."""
    rounds_log = []
    if laps.timings is not None:
        laps.timings["rounds"] = rounds_log
    per_case = []
    with _thermal_block(prob, meshes, mesh_index_to_layer_index, checked, cases, filtered_networks,
                        disconnected_meshes_by_layer, laps, "temperatures by Newton rounds on the film", check) as blk:
        k, thermal = blk.k, blk.thermal
        for j in range(k):
            where = f"Load case {j}" if k > 1 else "The thermal solve"
            heat = None
            if blk.heat is not None:
                mine = blk.heat[1] == j
                heat = (blk.heat[0][mine], np.zeros(int(mine.sum()), dtype=np.int32), blk.heat[2][mine])
            if blk.sources is not None:
                thermal.source_power(blk.source_power[j:j + 1])
            theta, tres, film = _film_newton(
                thermal, lambda: thermal.solve_kkt_column(blk.plan, k, j, heat, rtol=RTOL, max_iter=MAX_ITER), checked, where,
                blk.board, rounds_log, j)
            report = thermal.report(1, blk.n_tri, blk.n_vert, fields=fields, envelope=False)
            per_case.append((theta, tres, film, report, _stack_flows(thermal, checked, 1),
                             None if blk.sources is None else thermal.source_report(1)))
        laps.lap("thermal_solve")
    board = blk.board
    infos = []
    for j, (_theta, tres, _film, *_rest) in enumerate(per_case):
        if tres.status != _hip.OK and not tres.rel_residual <= max(RTOL, STALL_WARN_ABOVE):
            warnings.warn(f"{f'Load case {j}: ' if k > 1 else ''}The thermal solve stopped at a relative residual of "
                          f"{tres.rel_residual:.3e}", SolverWarning)
        infos.append({"iterations": int(tres.iterations), "rel_residual": float(tres.rel_residual), "seconds": float(tres.seconds)})
    solutions = _block_solutions(blk)
    theta = np.concatenate([c[0] for c in per_case])
    stacked = [None if not fields and i == 0 else np.concatenate([c[3][i] for c in per_case]) for i in range(5)]
    heat_val = blk.heat[2].reshape(k, len(blk.resistors), 2) if blk.heat is not None else None
    stack = (np.concatenate([c[4][0] for c in per_case]), per_case[0][4][1]) if checked.interlayer else None
    sources = None if blk.sources is None else (blk.sources, blk.source_power, np.concatenate([c[5] for c in per_case]))
    reports = _thermal_reports(board, checked, blk.substituted, blk.resistors, fields, theta, *stacked, heat_val, infos, stack,
                               sources)
    for report, case in zip(reports, per_case):
        report.film = case[2]
    env, env_case = envelope_of(theta[:, :blk.n_vert])
    envelope = _thermal_envelope(board, checked.ambient, env, env_case, reports)
    laps.lap("solutions")
    return solutions, reports, envelope


def solve_meshed_thermal(prob, meshes, mesh_index_to_layer_index, model: ThermalModel, *, cases=None, per_case_fields=True,
                         filtered_networks=None, disconnected_meshes_by_layer=None, partition=None,
                         timings: Optional[dict] = None):
    """``solve_meshed`` together with how hot the Joule heating makes the copper: ``(Solution, ThermalReport)``, or for a list
    of load ``cases`` (the mappings :func:`check_load_cases` accepts) ``([Solution], [ThermalReport], ThermalEnvelope)``.

    The model (DESIGN.md "Thermal") is one more sheet problem on the same meshes, for the temperature rise theta = T -
    ambient at every vertex of the connected meshes and every internal node:

        (K_kappa + diag(h M_v) + links) theta = b

    with K_kappa the cotangent stiffness with the layer's thermal sheet conductance kappa [W/K] in the place of sigma, M_v a
    third of the area of the faces around v, h the layer's film coefficient [W/(K mesh-unit^2)], a thermal conductance g
    [W/K] per resistor, and b_v a third of the Joule power [W] of the faces around v -- the weights' form sigma sum_edges
    w_ik (V_i - V_k)^2 that ``CurrentReport.layers`` sums, which balances the elements' powers exactly -- plus, with
    ``model.element_heat``, half of every resistor's dissipation at each of its terminals.  Since K and the links annihilate
    constants, ``total_loss`` (what the films carry away) equals ``total_heat`` (what the sources deliver) up to the
    solve's tolerance.  The coupling is one-way: the copper's resistivity does not follow the temperature
    (:func:`solve_meshed_electrothermal` closes that loop).

    With ``model.interlayer`` (DESIGN.md "Stack") the operator gains G, the heat conduction through the dielectric between
    the named pairs of layers: every vertex of one layer of a pair is linked to the three corners of the face of the other
    layer that contains it, with the conductance g M_v / 2 shared out by the barycentric weights, from both sides.  G
    annihilates constants, so the balance above holds; ``ThermalReport.interlayer`` gives the heat through every pair and
    the coupled area, and ``layers[i]["exchange"]`` the net heat layer i passes on.  Only connected meshes take part:
    floating copper as a pure heat spreader is out of scope.

    With ``model.heat_sources`` (DESIGN.md "Heat sources") b also carries the watts of components: source s loads the
    faces of the connected meshes of its layer whose centroid lies inside its polygon (even-odd rule), face f with the
    share area_f / A_s of the source's power in this case, a third of it at each corner; a footprint that covers no
    centroid loads the one face that contains the mean of its vertices.  The shares sum to 1, so ``total_heat`` is the
    Joule and element heat plus ``source_heat``, the sum of the powers, and ``total_loss`` still equals it.  The heat of
    ``layers[i]`` and the power densities stay the Joule heat alone.  ``ThermalReport.sources`` tells per source the power,
    the loaded area and faces, whether the fallback was taken, and the area-weighted mean temperature of the copper under
    it -- also with ``per_case_fields=False``.  A sequence of powers must have one entry per load case, and a source on
    no connected copper is refused: ValueError, the latter after the device handles have been closed.

    With a :class:`FilmCurve` for some layer's ``model.film`` (DESIGN.md "Film curves") the film follows the temperature
    rise and the solve is a Newton loop per load case: the film linearised about theta_k gives the diagonal q'(theta_k) M_v
    and the load term (q'(theta_k) theta_k - q(theta_k)) M_v, q = h(theta) theta; the first round is the linear solve with
    h(0), the loop ends when no vertex moved by more than ``model.film_tolerance`` or after ``model.film_max_rounds`` with a
    SolverWarning.  The cases keep their one electrical block solve and go through the thermal rounds one at a time.
    ``ThermalReport.film`` tells how the loop went, every ``loss`` and ``total_loss`` is sum_v M_v h(theta_v) theta_v, and
    ``total_loss`` equals ``total_heat`` up to the last round's linearisation defect.  Floats and constant curves take the
    linear path, a single solve with the bits it always gave.

    The electrical block is the load-case path; the thermal operator is then assembled from the meshes the device still
    holds, the face powers of every case are computed from the potentials it holds, and all cases go through one block
    solve with the multigrid preconditioner -- the powers never visit the host.  Disconnected meshes take no part and
    report the ambient temperature.  With ``per_case_fields=False`` no per-face temperature is computed and the reports
    carry no ``temperatures`` or ``face_temperatures``; hotspots, sums and the envelope are the same.  ValueError, before
    anything reaches the device, for an invalid model (:func:`check_thermal_model`), invalid cases, a mesh vertex without
    a face, and a ``partition`` over several GPUs.  ``timings`` (a dict) receives the host time of each step in seconds."""
    _refuse_partition(partition, "temperatures")
    checked = check_thermal_model(prob, model, filtered_networks)
    single = cases is None
    checked_cases = [{}] if single else check_load_cases(prob, cases)
    solutions, reports, envelope = _solve_block_thermal(prob, meshes, mesh_index_to_layer_index, checked, checked_cases,
                                                        bool(per_case_fields) or single, filtered_networks,
                                                        disconnected_meshes_by_layer, _Laps(timings))
    if single:
        return solutions[0], reports[0]
    return solutions, reports, envelope


def solve_thermal(prob, model: ThermalModel, mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None, cases=None,
                  per_case_fields=True, partition=None, prune=False):
    """``solve`` with the copper's temperatures (see :func:`solve_meshed_thermal`): the board is meshed once."""
    _refuse_partition(partition, "temperatures")
    check_thermal_model(prob, model)
    if cases is not None:
        cases = check_load_cases(prob, cases)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_thermal(prob, meshes, mesh_index_to_layer_index, model, cases=cases, per_case_fields=per_case_fields,
                                **pruned)


# --------------------------------------------------------------------------------------------
# temperature sensitivities: what cools a hotspot (DESIGN.md "Temperature sensitivities")
# --------------------------------------------------------------------------------------------

MAX_TEMPERATURE_OBJECTIVES = 4096


@dataclass(frozen=True)
class TemperatureObjective:
    """A temperature of one load case that :func:`solve_meshed_thermal_sensitivities` differentiates: a linear functional
    T = ambient + g^T theta of the case's temperature rise.  Made by one of the three constructors."""
    kind: str                      # "at", "source" or "hotspot"
    layer: object = None           # the layer, its name, or (checked) its index
    point: Optional[tuple] = None  # (x, y) of "at"
    source: object = None          # the name or index of a heat source, or (checked) its index
    case: int = 0

    @classmethod
    def at(cls, layer, point, case: int = 0) -> "TemperatureObjective":
        """The temperature interpolated at ``point`` = (x, y) of ``layer``: the field sampler's owner face (the containing
        face with the lowest global number) and its barycentric weights.  A point on no connected copper of the layer is a
        ValueError of the solve."""
        return cls("at", layer=layer, point=point, case=case)

    @classmethod
    def of_source(cls, source, case: int = 0) -> "TemperatureObjective":
        """The footprint temperature of one of ``model.heat_sources`` (by name or index): the number
        ``ThermalReport.sources[i]["temperature"]`` reports."""
        return cls("source", source=source, case=case)

    @classmethod
    def hotspot(cls, layer, case: int = 0) -> "TemperatureObjective":
        """The temperature at the vertex ``ThermalReport.hotspots[layer]`` names for that case, held fixed: the derivative
        is that of this vertex's temperature, valid while the argmax does not move to another vertex."""
        return cls("hotspot", layer=layer, case=case)


@dataclass
class ThermalSensitivity:
    """Derivatives of one :class:`TemperatureObjective` (see :func:`solve_meshed_thermal_sensitivities`)."""
    objective: TemperatureObjective
    case: int
    value: float          # the temperature, ambient included
    electrical: list      # per layer, per mesh of LayerSolution.meshes: TwoForm of e_f / area_f, e_f = sigma dT/dsigma_f [K]
    thermal: list         # likewise k_f / area_f, k_f = kappa dT/dkappa_f
    copper: list          # likewise (e_f + k_f) / area_f: kelvin per relative thickening of the face, per area
    layers: list          # per layer: {"electrical": sum e_f, "thermal": sum k_f, "copper": their sum, "film": h_l dT/dh_l}
    interlayer: list      # per pair of model.interlayer: {"layers": (a, b), "value": g_p dT/dg_p}
    sources: list         # per heat source: dT/dP_s [K/W] for the objective's case
    elements: dict        # lumped element -> {field: dT/dfield}; a Resistor also "link": dT/dg_link


def _resolve_layer(prob, layer, what: str) -> int:
    if isinstance(layer, str):
        found = [i for i, own in enumerate(prob.layers) if own.name == layer]
    else:
        found = [i for i, own in enumerate(prob.layers) if own is layer] or [i for i, own in enumerate(prob.layers) if own == layer]
    if len(found) != 1:
        raise ValueError(f"{what}: {layer!r} is no layer of the Problem" if not found else
                         f"{what}: {layer!r} names {len(found)} layers of the Problem")
    return found[0]


def check_temperature_objectives(prob, model, objectives, n_cases, filtered_networks=None) -> list:
    """The ``objectives`` resolved against ``prob`` and ``model`` as a list of :class:`TemperatureObjective` whose ``layer``
    and ``source`` are indices, or ValueError: ``objectives`` is a non-empty sequence of at most 4096
    :class:`TemperatureObjective`; a ``case`` is an integer in [0, n_cases); a layer is a layer of the Problem (itself or
    its name); a point is two finite numbers; a source is the name or the index of one of ``model.heat_sources``.
    ``filtered_networks`` is accepted for symmetry with the other checks: no objective depends on the networks."""
    if isinstance(objectives, (Mapping, str, bytes, TemperatureObjective)):
        raise ValueError("objectives must be a sequence of TemperatureObjective")
    try:
        objectives = list(objectives)
    except TypeError:
        raise ValueError("objectives must be a sequence of TemperatureObjective") from None
    if not objectives:
        raise ValueError("no objectives: give at least one TemperatureObjective")
    if len(objectives) > MAX_TEMPERATURE_OBJECTIVES:
        raise ValueError(f"{len(objectives)} objectives: at most {MAX_TEMPERATURE_OBJECTIVES} in one call")
    names = [source.name for source in _check_heat_sources(prob, getattr(model, "heat_sources", None))]
    out = []
    for j, obj in enumerate(objectives):
        if not isinstance(obj, TemperatureObjective):
            raise ValueError(f"objective {j} is no TemperatureObjective but {obj!r}")
        what = f"objective {j}"
        if isinstance(obj.case, bool) or not isinstance(obj.case, (int, np.integer)) or not 0 <= int(obj.case) < int(n_cases):
            raise ValueError(f"{what}: case {obj.case!r} is not one of the {int(n_cases)} load case(s)")
        case = int(obj.case)
        if obj.kind == "at":
            layer = _resolve_layer(prob, obj.layer, what)
            try:
                x, y = (float(c) for c in obj.point)
            except (TypeError, ValueError):
                raise ValueError(f"{what}: the point must be a pair (x, y) of numbers, not {obj.point!r}") from None
            if not (math.isfinite(x) and math.isfinite(y)):
                raise ValueError(f"{what}: the point {obj.point!r} is not finite")
            out.append(TemperatureObjective("at", layer=layer, point=(x, y), case=case))
        elif obj.kind == "hotspot":
            out.append(TemperatureObjective("hotspot", layer=_resolve_layer(prob, obj.layer, what), case=case))
        elif obj.kind == "source":
            key = obj.source
            if isinstance(key, str):
                found = [i for i, name in enumerate(names) if name == key]
            elif isinstance(key, (int, np.integer)) and not isinstance(key, bool):
                found = [int(key)] if 0 <= int(key) < len(names) else []
            else:
                found = []
            if len(found) != 1:
                raise ValueError(f"{what}: {key!r} is no heat source of the model" if not found else
                                 f"{what}: {key!r} names {len(found)} heat sources of the model")
            out.append(TemperatureObjective("source", source=found[0], case=case))
        else:
            raise ValueError(f"{what}: unknown kind {obj.kind!r}; use TemperatureObjective.at, .of_source or .hotspot")
    return out


def _refuse_gain_regulators(pairs) -> None:
    """ValueError for a Problem whose :func:`woodbury_terms` is not empty: the electrical adjoint would need M^T."""
    for element, row in pairs:
        if woodbury_terms([row]):
            raise ValueError(f"temperature sensitivities do not take a regulator with a gain term on distinct sense nodes "
                             f"({element!r}): its stamps make the electrical system unsymmetric, and the adjoint through both "
                             "physics is solved with the symmetric system only")


def thermal_element_sensitivities(element_rows, x, mu, lam_at, theta, element_heat: bool) -> list:
    """dT/dfield of every element row (global_elements' tuples on global unknowns) for the case's potentials ``x``, the
    electrical adjoint ``mu``, the thermal adjoint at the resistors' terminals ``lam_at`` {unknown: lambda} and the case's
    ``theta``: :func:`element_sensitivities` of (x, mu), and for a Resistor

    - "resistance": with ``element_heat``, plus -((lambda_a + lambda_b) / 2) (x_a - x_b)^2 / R^2 -- its own dissipation,
    - "link": dT/dg_link = -(lambda_a - lambda_b)(theta_a - theta_b)."""
    out = element_sensitivities(element_rows, x, mu)
    for row, d in zip(element_rows, out):
        if row[0] == "R":
            _, a, b, res = row
            la, lb = lam_at[int(a)], lam_at[int(b)]
            if element_heat:
                dx = x[a] - x[b]
                d["resistance"] = float(d["resistance"] - ((la + lb) / 2) * (dx * dx) / (res * res))
            d["link"] = float(-(la - lb) * (theta[a] - theta[b]))
    return out


def _thermal_sensitivities_inside(checked: CheckedThermalModel, cases, objs, given, laps: _Laps):
    """The pass of :func:`solve_meshed_thermal_sensitivities` that runs while the block lives on the device (the ``inside`` of
    :func:`_solve_block_thermal`): adjoints, right-hand sides, block solve, finish, the face, vertex, pair and source
    kernels, elements."""
    def inside(blk, theta, mesh_max, mesh_vert, sources):
        board, k, prob = blk.board, blk.k, blk.board.prob
        n_mesh, layer_of, voff, n_obj = len(board.meshes), board.layer_of, board.vindex.offsets, len(objs)
        case, kind, arg = [o.case for o in objs], [], []
        xy, unknown, weight = np.zeros((n_obj, 2)), np.full((n_obj, 3), -1, dtype=np.int64), np.zeros((n_obj, 3))
        spots = {}
        for j, o in enumerate(objs):
            if o.kind == "at":
                kind.append(_hip.ThermalSensitivities.KIND_POINT)
                arg.append(o.layer)
                xy[j] = o.point
            elif o.kind == "hotspot":
                spot = _layer_hotspot(board, checked.ambient, mesh_max, mesh_vert, o.case, o.layer)
                if spot is None:
                    raise ValueError(f"objective {j}: layer {prob.layers[o.layer].name!r} has no connected vertices, so no hotspot")
                spots[j] = spot
                mesh_i = list(board.layer_meshes(o.layer))[spot[1]][0]
                kind.append(_hip.ThermalSensitivities.KIND_UNKNOWNS)
                arg.append(0)
                unknown[j, 0], weight[j, 0] = voff[mesh_i] + spot[2], 1.0
            else:
                kind.append(_hip.ThermalSensitivities.KIND_SOURCE)
                arg.append(o.source)
        res_rows = [row for _, row in blk.resistors]
        terminals = sorted({int(row[p]) for row in res_rows for p in (1, 2)})
        ts = _hip.ThermalSensitivities(blk.thermal, blk.plan, k, [checked.kappa[layer_of[i]] for i in range(n_mesh)])
        try:
            try:
                unknown, weight, lam_p, lres = ts.thermal_adjoints(case, kind, arg, xy, unknown, weight,
                                                                   [layer_of[i] for i in range(n_mesh)], terminals,
                                                                   rtol=RTOL, max_iter=MAX_ITER)
            except ValueError as exc:
                if "lies on no face" not in str(exc):
                    raise
                j = int(str(exc).split("objective ")[1].split(":")[0])       # the lowest such objective, named by the device
                raise ValueError(f"objective {j} ({given[j]!r}): the point {objs[j].point} lies on no connected copper of layer "
                                 f"{prob.layers[objs[j].layer].name!r}") from None
            laps.lap("thermal_adjoints")
            heat_rows = res_rows if checked.element_heat else []
            r_dev = ts.electrical_rhs([row[1] for row in heat_rows], [row[2] for row in heat_rows], [row[3] for row in heat_rows])
            laps.lap("electrical_rhs")
            # M^T mu = c through the plan, like the adjoints of solve_meshed_sensitivities: the known values are zero
            none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=DTYPE))
            red, known_idx, known_val = block_plan_inputs(blk.L, *none, n_obj)
            members = red.probe_members
            probes, ares = blk.plan.solve_block_dev(n_obj, r_dev, known_idx, known_val, red.regulator_columns, members, rtol=RTOL,
                                                    max_iter=MAX_ITER, abs_residual_target=ABS_RESIDUAL_TARGET)
            laps.lap("adjoint_stage1")
            MU, _mu_norms = _finish_block(blk.plan, red, members, probes, n_obj)
            laps.lap("adjoint_stage2")
            e_d, k_d, c_d, mesh_e, mesh_k = ts.faces(blk.n_tri, n_mesh)
            mesh_film = ts.vertices(n_mesh)
            pair_v = ts.pairs() if checked.interlayer else None
            source_v = ts.sources() if blk.sources is not None else None
            laps.lap("sensitivity_kernels")
        finally:
            ts.close()
        for what, res in (("thermal", lres), ("electrical", ares)):
            if res.status != _hip.OK and not res.rel_residual <= max(RTOL, STALL_WARN_ABOVE):
                warnings.warn(f"The {what} adjoint solve stopped at a relative residual of {res.rel_residual:.3e}", SolverWarning)
        if laps.timings is not None:        # what the two adjoint solves spent on multigrid setups: 0.0 on hierarchies that exist
            laps.timings["adjoint_setup_seconds"] = float(lres.setup_seconds + ares.setup_seconds)
        lam_at = [dict(zip(terminals, lam_p[j].tolist())) for j in range(n_obj)]
        all_rows = [row for _, row in blk.pairs]
        out = []
        for j, o in enumerate(objs):
            c = o.case
            if o.kind == "at":
                value = float(checked.ambient + sum(weight[j, q] * theta[c, unknown[j, q]] for q in range(3)))
            elif o.kind == "hotspot":
                value = spots[j][0]
            else:
                value = float(checked.ambient + sources[2][c, o.source])
            forms = {"electrical": [], "thermal": [], "copper": []}
            layers = []
            for layer_i in range(len(prob.layers)):
                per = {name: [] for name in forms}
                tot_e, tot_k, film = [], [], []
                for mesh_i, msh, lo, hi in board.layer_meshes(layer_i):
                    for name, dens in (("electrical", e_d), ("thermal", k_d), ("copper", c_d)):
                        tf = mesh.TwoForm(msh)
                        tf.values = np.array(dens[j, lo:hi], dtype=DTYPE)
                        per[name].append(tf)
                    tot_e.append(float(mesh_e[j, mesh_i]))
                    tot_k.append(float(mesh_k[j, mesh_i]))
                    film.append(float(mesh_film[j, mesh_i]))
                for name in forms:
                    forms[name].append(per[name])
                se, sk = math.fsum(tot_e), math.fsum(tot_k)
                layers.append({"electrical": se, "thermal": sk, "copper": se + sk, "film": math.fsum(film)})
            interlayer = [] if pair_v is None else [{"layers": (a, b), "value": float(pair_v[j, p])}
                                                    for p, (a, b, _g) in enumerate(checked.interlayer)]
            rows_c = _case_element_rows(blk.pairs, all_rows, cases[c])
            per_element = thermal_element_sensitivities(rows_c, blk.V[:, c], MU[:, j], lam_at[j], theta[c], checked.element_heat)
            out.append(ThermalSensitivity(
                objective=given[j], case=c, value=value, electrical=forms["electrical"], thermal=forms["thermal"],
                copper=forms["copper"], layers=layers, interlayer=interlayer,
                sources=[] if source_v is None else [float(v) for v in source_v[j]],
                elements={element: per_element[i] for i, (element, _) in enumerate(blk.pairs)}))
        laps.lap("sensitivities")
        return out
    return inside


def solve_meshed_thermal_sensitivities(prob, meshes, mesh_index_to_layer_index, model: ThermalModel, objectives, *, cases=None,
                                       filtered_networks=None, disconnected_meshes_by_layer=None, partition=None,
                                       timings: Optional[dict] = None):
    """``solve_meshed_thermal`` together with what every parameter does to chosen temperatures: ``(Solution, ThermalReport,
    [ThermalSensitivity])``, or for a list of load ``cases`` ``([Solution], [ThermalReport], ThermalEnvelope,
    [ThermalSensitivity])``, one :class:`ThermalSensitivity` per objective in the order given.  The first items carry the
    bits ``solve_meshed_thermal`` returns for the same arguments.

    An objective (:class:`TemperatureObjective`) is a linear functional T = ambient + g^T theta of one load case: the
    temperature at a point, the footprint temperature of a heat source, or the temperature at the case's hotspot vertex of a
    layer, held fixed (valid while the argmax does not move).  With M x = r the electrical system and A theta = b(x) the
    thermal one (DESIGN.md "Temperature sensitivities"), two adjoints carry the chain through both physics:

        A lambda = g,    M^T mu = grad_x (lambda^T b(x)),    dT/dp = lambda^T (db/dp - dA/dp theta) + mu^T (dr/dp - dM/dp x)

    - ``electrical``: e_f = sigma dT/dsigma_f = lbar_f P_f + sigma sum_edges w_ik (mu_i - mu_k)(x_i - x_k) per face, as a
      density e_f / area_f: what the face's electrical conductance does through the Joule heat (lbar_f the mean of lambda at
      the face's corners, P_f its Joule power);
    - ``thermal``: k_f = kappa dT/dkappa_f = -kappa sum_edges w_ik (lambda_i - lambda_k)(theta_i - theta_k): what its thermal
      conductance does by spreading the heat;
    - ``copper``: e_f + k_f, kelvin per relative thickening of the face, since both conductances are proportional to
      thickness; ``layers[l]`` holds the three sums over the layer and ``"film"`` = h_l dT/dh_l;
    - ``interlayer``: g_p dT/dg_p of every pair; ``sources``: dT/dP_s [K/W]; ``elements``: {field: dT/dfield} with the fields
      of ``SENSITIVITY_FIELDS``, and for a Resistor also ``"link"``: dT/dg_link.

    All derivatives are partial derivatives with respect to the parameters of the *checked* model: kappa does not move with
    sigma through the Wiedemann-Franz default, and a link conductance does not move with R.  The call costs one
    ``solve_meshed_thermal`` plus one thermal and one electrical adjoint column per objective, on hierarchies the forward
    solves have built; every adjoint right-hand side is formed on the device.

    ValueError, before anything reaches the device, for what ``solve_meshed_thermal`` refuses, for invalid objectives
    (:func:`check_temperature_objectives`, more than 4096 among them), a ``partition`` over several GPUs, a model that is no
    ThermalModel (the electro-thermal and the transient models are not accepted: the resistivity feedback and the time
    stepping change the adjoint system), and a Problem with a regulator whose gain term acts on distinct sense nodes
    (:func:`woodbury_terms` not empty; the message names it).  ValueError of the solve for a point on no connected copper of
    its layer and a hotspot on a layer without connected vertices, naming the objective.  ``timings`` (a dict) receives the
    host time of each step in seconds, and ``"adjoint_setup_seconds"``: what the two adjoint solves spent building multigrid
    hierarchies, 0.0 when those of the forward solves were reused."""
    _refuse_partition(partition, "temperature sensitivities")
    if not isinstance(model, ThermalModel):
        raise ValueError("temperature sensitivities take a ThermalModel: the electro-thermal and the transient models are not "
                         f"accepted, not {type(model).__name__}")
    checked = check_thermal_model(prob, model, filtered_networks)
    _refuse_film_curves(checked, "the temperature-sensitivity solve")
    single = cases is None
    checked_cases = [{}] if single else check_load_cases(prob, cases)
    given = objectives
    if hasattr(objectives, "__iter__") and not isinstance(objectives, (Mapping, str, bytes, TemperatureObjective)):
        given = list(objectives)                     # (an iterator is read once)
    objs = check_temperature_objectives(prob, model, given, len(checked_cases), filtered_networks)
    laps = _Laps(timings)
    solutions, reports, envelope, sens = _solve_block_thermal(
        prob, meshes, mesh_index_to_layer_index, checked, checked_cases, True, filtered_networks, disconnected_meshes_by_layer, laps,
        check=lambda board, pairs: _refuse_gain_regulators(pairs),
        inside=_thermal_sensitivities_inside(checked, checked_cases, objs, given, laps))
    if single:
        return solutions[0], reports[0], sens
    return solutions, reports, envelope, sens


def solve_thermal_sensitivities(prob, model: ThermalModel, objectives, mesher_config: Optional[mesh.Mesher.Config] = None, *,
                                mesher=None, cases=None, partition=None, prune=False):
    """``solve`` with the temperatures and their sensitivities (see :func:`solve_meshed_thermal_sensitivities`): the board is
    meshed once."""
    _refuse_partition(partition, "temperature sensitivities")
    if not isinstance(model, ThermalModel):
        raise ValueError("temperature sensitivities take a ThermalModel: the electro-thermal and the transient models are not "
                         f"accepted, not {type(model).__name__}")
    _refuse_film_curves(check_thermal_model(prob, model), "the temperature-sensitivity solve")
    if cases is not None:
        cases = check_load_cases(prob, cases)
    check_temperature_objectives(prob, model, objectives, 1 if cases is None else len(cases))
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_thermal_sensitivities(prob, meshes, mesh_index_to_layer_index, model, objectives, cases=cases, **pruned)


# --------------------------------------------------------------------------------------------
# transient: the copper's temperatures under a schedule of load cases (DESIGN.md "Transient")
# --------------------------------------------------------------------------------------------

MAX_TRANSIENT_STEPS = 100000


@dataclass
class Segment:
    """A stretch of a schedule with one load and equal steps (see :func:`solve_meshed_thermal_transient`).

    - ``duration``: seconds, finite and positive.
    - ``steps``: the number (>= 1) of backward-Euler steps of ``duration / steps`` it is covered with.
    - ``case``: an index into the ``cases`` of the call, None = sources off; or a tuple with one such entry per scenario."""
    duration: float
    steps: int
    case: object = None


@dataclass
class TransientModel:
    """What turns a schedule of loads into temperatures over time (see :func:`solve_meshed_thermal_transient`).

    - ``thermal``: the :class:`ThermalModel` of the steady problem.
    - ``areal_capacity``: the heat capacity per area c [J / (K mesh-unit^2)] of the sheet, one float for all layers or a
      mapping {layer or layer name: float} that names every layer.  Required: it lumps the board under the foil as well as
      the foil, and there is no sensible default.  With meshes in mm, 35 um of copper alone are 1.2e-4 J/(K mm^2) and
      1.6 mm of FR4 about 3e-3 J/(K mm^2).
    - ``initial``: None = every scenario starts at ambient; a case index = from that case's steady state; or a tuple with
      one such entry per scenario."""
    thermal: ThermalModel
    areal_capacity: object
    initial: object = None


@dataclass
class CheckedTransientModel:
    """A :class:`TransientModel` resolved against a Problem (:func:`check_transient_model`)."""
    thermal: CheckedThermalModel
    capacity: list             # per layer
    initial: object            # None, an int, or a tuple of None / int


@dataclass
class TransientEnvelope:
    """The hottest each vertex got during one scenario (the sequential rule of :func:`envelope_of`, applied along time: the
    earliest time keeps a tie)."""
    temperatures: list    # per layer, per mesh: ZeroForm of max_n T_n per vertex
    times: list           # per layer, per mesh: (n_vertices,) the first time of that maximum [s]
    hotspots: list        # per layer: (T, time, mesh index within the layer, vertex index, x, y), None without vertices


@dataclass
class TransientReport:
    """The temperatures of one scenario over time (see :func:`solve_meshed_thermal_transient`).  Arrays over time have
    n_steps + 1 entries: entry 0 is the start, entry n the state after step n."""
    times: np.ndarray                   # [s]
    hotspots: list                      # per layer, per time: (T, mesh index within the layer, vertex index, x, y), None without vertices
    layers: list                        # per layer: {"stored": heat held above ambient [J], "loss": film loss [W], "heat": Joule heat put into its copper by the step that led here [W]}, arrays over time
    total_stored: np.ndarray            # [J]
    total_loss: np.ndarray              # [W]
    total_heat: np.ndarray              # [W]: copper and elements, of the case of the step that led here (0 at the start and with the sources off)
    probes: dict                        # node id -> T over time
    peak: Optional[tuple]               # (T, time, layer index, mesh index within the layer, vertex index, x, y): the first time of the largest hotspot
    envelope: TransientEnvelope
    snapshot_times: list                # the times of the kept fields
    temperatures: list                  # per kept time: per layer, per mesh ZeroForm of T
    face_temperatures: list             # per kept time: per layer, per mesh TwoForm of the mean T of each face's corners
    disconnected_temperatures: list     # per layer, per disconnected mesh: ZeroForm filled with the ambient temperature
    info: dict                          # {"iterations", "iterations_per_step", "seconds_per_step", "setup_seconds_per_step", "rel_residual", "hierarchies", "seconds"}


def _case_entry(value, n_cases: int, what: str):
    """None, or the int of a case index in range; ValueError otherwise."""
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError(f"{what} must be None (sources off) or the index of a load case, not {value!r}")
    if not 0 <= int(value) < n_cases:
        raise ValueError(f"{what}: {int(value)} is no load case (there are {n_cases})")
    return int(value)


def _scenario_entries(value, n_cases: int, what: str):
    """``value`` as a checked scalar entry, or as a tuple of them when it is a tuple or list."""
    if isinstance(value, (tuple, list)):
        if not value:
            raise ValueError(f"{what}: a tuple names at least one scenario")
        return tuple(_case_entry(v, n_cases, what) for v in value)
    return _case_entry(value, n_cases, what)


def check_transient_model(prob, model, filtered_networks=None) -> CheckedTransientModel:
    """``model`` resolved against ``prob``, or ValueError -- before anything reaches the device -- for everything
    :func:`check_thermal_model` refuses of ``model.thermal``; an areal capacity that is missing, not finite or not
    positive; a layer without a capacity; and a mapping key that is no layer.  ``initial`` is checked against the cases and
    the schedule by :func:`solve_meshed_thermal_transient`."""
    if not isinstance(model, TransientModel):
        raise ValueError("model must be a TransientModel")
    thermal = check_thermal_model(prob, model.thermal, filtered_networks)
    _refuse_film_curves(thermal, "a transient solve")
    if model.areal_capacity is None:
        raise ValueError("the areal heat capacity is required: a float, or a mapping {layer: float}")
    if isinstance(model.areal_capacity, Mapping):
        given = _per_layer(prob, model.areal_capacity, "areal_capacity")
        for i, layer in enumerate(prob.layers):
            if i not in given:
                raise ValueError(f"layer {layer.name!r} has no areal heat capacity")
        capacity = [given[i] for i in range(len(prob.layers))]
    else:
        capacity = [_positive_number(model.areal_capacity, "the areal heat capacity")] * len(prob.layers)
    return CheckedTransientModel(thermal=thermal, capacity=capacity, initial=model.initial)


def _check_entries(schedule, n_cases: int, repeat, kind, more=None) -> tuple:
    """What :func:`check_schedule` and :func:`check_spans` share: (the checked entries of the sequence ``schedule`` of ``kind``
    -- Segment or Span --, the number of scenarios), or ValueError.  ``more(i, entry)`` checks and returns the fields of entry
    ``i`` beyond ``duration`` and ``case``."""
    name, lower = kind.__name__, kind.__name__.lower()
    if isinstance(repeat, bool) or not isinstance(repeat, (int, np.integer)) or repeat < 1:
        raise ValueError(f"repeat must be an integer >= 1, not {repeat!r}")
    if isinstance(schedule, (Span, Segment, Mapping, str, bytes)):
        raise ValueError(f"the schedule must be a sequence of {name}s")
    try:
        schedule = list(schedule)
    except TypeError:
        raise ValueError(f"the schedule must be a sequence of {name}s") from None
    if not schedule:
        raise ValueError(f"an empty schedule: give at least one {name}")
    checked, n_scen = [], None
    for i, entry in enumerate(schedule):
        if not isinstance(entry, kind):
            raise ValueError(f"{lower} {i} is not a {name}")
        duration = _positive_number(entry.duration, f"the duration of {lower} {i}")
        fields = more(i, entry) if more is not None else {}
        case = _scenario_entries(entry.case, n_cases, f"the case of {lower} {i}")
        if isinstance(case, tuple):
            if n_scen is not None and len(case) != n_scen:
                raise ValueError(f"{lower} {i} names {len(case)} scenarios, an earlier one {n_scen}")
            n_scen = len(case)
        checked.append(kind(duration=duration, case=case, **fields))
    return checked, (1 if n_scen is None else n_scen)


def check_schedule(schedule, n_cases: int, repeat=1) -> tuple:
    """(the flattened segments, the number of scenarios) of a schedule, or ValueError.

    ``schedule`` is a non-empty sequence of :class:`Segment`; it is run ``repeat`` (>= 1) times back to back, and the
    flattened list holds ``repeat * len(schedule)`` checked Segments.  A segment's ``case`` is None, an index below
    ``n_cases``, or a tuple of those with one entry per scenario; all tuples have the same length, which is the number of
    scenarios (1 without tuples), and tuples come back as tuples.  Refused: an empty schedule, a duration that is not finite
    and positive, ``steps`` that is not an integer >= 1, a case out of range, tuples of unequal length, ``repeat < 1`` and
    more than 100 000 steps in total."""
    def steps_of(i, seg):
        if isinstance(seg.steps, bool) or not isinstance(seg.steps, (int, np.integer)) or seg.steps < 1:
            raise ValueError(f"the steps of segment {i} must be an integer >= 1, not {seg.steps!r}")
        return {"steps": int(seg.steps)}

    checked, n_scen = _check_entries(schedule, n_cases, repeat, Segment, steps_of)
    total = int(repeat) * sum(seg.steps for seg in checked)
    if total > MAX_TRANSIENT_STEPS:
        raise ValueError(f"{total} steps in total: more than {MAX_TRANSIENT_STEPS}")
    return [dataclasses.replace(seg) for _ in range(int(repeat)) for seg in checked], n_scen


def check_probes(prob, probes, filtered_networks=None) -> list:
    """The probes as a list of NodeIDs of the solved networks (connection nodes or internal nodes, as
    :func:`check_objectives` accepts them), or ValueError."""
    if isinstance(probes, (Mapping, str, bytes)) or _is_node_id(probes):
        raise ValueError("probes must be a sequence of NodeIDs")
    try:
        probes = list(probes)
    except TypeError:
        raise ValueError("probes must be a sequence of NodeIDs") from None
    networks = list(prob.networks) if filtered_networks is None else list(filtered_networks)
    known = {node for network in networks for node in list(network.nodes) + [conn.node_id for conn in network.connections]}
    for j, node in enumerate(probes):
        if not _is_node_id(node):
            raise ValueError(f"probe {j} must be a NodeID, not {type(node).__name__}")
        if node not in known:
            raise ValueError(f"probe {j} is not a node of the solved networks")
    return probes


def _check_transient_call(prob, initial, schedule, cases, repeat, probes, keep, filtered_networks, check_entries, entry_of,
                          scenarios=True, sources=(), extra=None) -> tuple:
    """The checks the three transient calls share, in the order in which they refuse: (checked cases, per flattened entry
    ``entry_of(entry, per-scenario cases)``, per-scenario initial cases, probes, the value of ``extra``).  ``check_entries``
    is :func:`check_schedule` or :func:`check_spans`; ``initial`` and every entry's case are broadcast to the scenarios.
    Without ``scenarios`` the tuple form of a case is refused, and cases and ``initial`` come back as they are; ``sources``
    are checked heat sources whose powers must be one per case.  ``extra()`` holds a call's own checks, which come after
    ``keep`` and before the probes."""
    checked_cases = [{}] if cases is None else check_load_cases(prob, cases)
    entries, n_scen = check_entries(schedule, len(checked_cases), repeat)
    tuples = any(isinstance(entry.case, tuple) for entry in entries)
    if not scenarios:
        if tuples:
            raise ValueError(f"the case of a segment: {_NO_SCENARIOS}")
        initial = _case_entry(initial, len(checked_cases), "initial")
        flat = [entry_of(entry, entry.case) for entry in entries]
    else:
        initial = _scenario_entries(initial, len(checked_cases), "initial")
        if isinstance(initial, tuple):
            if tuples and len(initial) != n_scen:
                raise ValueError(f"initial names {len(initial)} scenarios, the schedule {n_scen}")
            n_scen = len(initial)
        else:
            initial = (initial,) * n_scen
        flat = [entry_of(entry, entry.case if isinstance(entry.case, tuple) else (entry.case,) * n_scen) for entry in entries]
    _source_powers(sources, len(checked_cases))
    if keep not in ("end", "segments", "none"):
        raise ValueError(f'keep must be "end", "segments" or "none", not {keep!r}')
    own = extra() if extra is not None else None
    return checked_cases, flat, initial, check_probes(prob, probes, filtered_networks), own


def _check_transient_arguments(prob, model, schedule, cases, repeat, probes, keep, filtered_networks):
    """Every check of :func:`solve_meshed_thermal_transient`: (checked model, checked cases, per flattened segment (dt, steps,
    per-scenario cases), per-scenario initial cases, probes)."""
    checked = check_transient_model(prob, model, filtered_networks)
    checked_cases, flat, initial, probe_nodes, _ = _check_transient_call(
        prob, checked.initial, schedule, cases, repeat, probes, keep, filtered_networks, check_schedule,
        lambda seg, seg_cases: (seg.duration / seg.steps, seg.steps, seg_cases))
    return checked, checked_cases, flat, initial, probe_nodes


def _snapshot(board: IndexedBoard, ambient: float, theta: np.ndarray) -> tuple:
    """(per layer, per mesh ZeroForm of T; per layer, per mesh TwoForm of the mean T of each face's corners) of one state,
    the mean as padne_thermal_report forms it: ((theta_1 + theta_2) + theta_3) / 3 on the corners (2, 0, 1)."""
    voff, temps, faces = board.vindex.offsets, [], []
    for layer_i in range(len(board.prob.layers)):
        zfs, tfs = [], []
        for mesh_i, msh, _lo, _hi in board.layer_meshes(layer_i):
            th = theta[voff[mesh_i]:voff[mesh_i + 1]]
            tri = np.asarray(msh.triangles, dtype=np.int64).reshape(-1, 3)
            zf, tf = mesh.ZeroForm(msh), mesh.TwoForm(msh)
            zf.values = th + ambient
            tf.values = ((th[tri[:, 2]] + th[tri[:, 0]]) + th[tri[:, 1]]) / 3 + ambient
            zfs.append(zf)
            tfs.append(tf)
        temps.append(zfs)
        faces.append(tfs)
    return temps, faces


def _transient_report(board: IndexedBoard, ambient: float, times, mesh_max, mesh_vert, stored, loss, layer_heat, total_heat,
                      probes, env, env_step, snapshots, info) -> TransientReport:
    """The TransientReport of one scenario from its per-time arrays (n_steps + 1, n_mesh), the heats per time, the probe
    traces {node: theta over time}, the envelope of theta with its steps (n_vert,) and the kept states [(time, theta)]."""
    voff, n_layers, n_times = board.vindex.offsets, len(board.prob.layers), len(times)
    hotspots, layers, env_temps, env_times, env_spots, peak = [], [], [], [], [], None
    for layer_i in range(n_layers):
        in_layer = list(board.layer_meshes(layer_i))
        spots = [_layer_hotspot(board, ambient, mesh_max, mesh_vert, n, layer_i, in_layer) for n in range(n_times)]
        for n, best in enumerate(spots):
            if best is not None and (peak is None or best[0] > peak[0]):      # the first time, then the lowest layer
                peak = (best[0], float(times[n]), layer_i, *best[1:])
        hotspots.append(spots)
        ids = [mesh_i for mesh_i, *_ in in_layer]
        layers.append({"stored": np.array([math.fsum(stored[n, ids].tolist()) for n in range(n_times)]),
                       "loss": np.array([math.fsum(loss[n, ids].tolist()) for n in range(n_times)]),
                       "heat": np.asarray(layer_heat[layer_i], dtype=DTYPE)})
        zfs, whens, spot = [], [], None
        for at, (mesh_i, msh, _lo, _hi) in enumerate(in_layer):
            values, steps = env[voff[mesh_i]:voff[mesh_i + 1]], env_step[voff[mesh_i]:voff[mesh_i + 1]]
            zf = mesh.ZeroForm(msh)
            zf.values = values + ambient
            zfs.append(zf)
            whens.append(np.asarray(times)[steps])
            if len(values):
                v = int(np.argmax(values))
                if spot is None or values[v] + ambient > spot[0]:
                    spot = (float(values[v] + ambient), float(times[steps[v]]), at, v, float(msh.points[v][0]), float(msh.points[v][1]))
        env_temps.append(zfs)
        env_times.append(whens)
        env_spots.append(spot)
    fields = [_snapshot(board, ambient, theta) for _, theta in snapshots]
    return TransientReport(
        times=np.asarray(times, dtype=DTYPE), hotspots=hotspots, layers=layers,
        total_stored=np.array([math.fsum(stored[n].tolist()) for n in range(n_times)]),
        total_loss=np.array([math.fsum(loss[n].tolist()) for n in range(n_times)]), total_heat=np.asarray(total_heat, dtype=DTYPE),
        probes={node: trace + ambient for node, trace in probes.items()}, peak=peak,
        envelope=TransientEnvelope(temperatures=env_temps, times=env_times, hotspots=env_spots),
        snapshot_times=[t for t, _ in snapshots], temperatures=[f[0] for f in fields], face_temperatures=[f[1] for f in fields],
        disconnected_temperatures=_cold_temperatures(board, ambient), info=info)


def _worse(worst: float, result) -> float:
    """``worst``, or the relative residual of a solve that ended above the tolerance if that is larger."""
    return max(worst, float(result.rel_residual)) if result.status != _hip.OK else worst


def _transient_head(transient, first, probe_idx) -> dict:
    """Time 0 in the form in which ``Transient.run`` records steps: ``max``, ``vertex``, ``stored`` and ``loss`` (1, n_scen,
    n_mesh) and ``probes`` (1, n_scen, n_probe) of the state ``Transient.start`` left; ``result``: ``first``, the SolveResult
    of that start, and ``worst``: what :func:`_worse` starts from."""
    top, vert, stored, loss = transient.report()
    probes = transient.state()[:, probe_idx] if probe_idx else np.empty((top.shape[0], 0), dtype=DTYPE)
    return {"max": top[None], "vertex": vert[None], "stored": stored[None], "loss": loss[None], "probes": probes[None],
            "result": first, "worst": first.rel_residual if first.status != _hip.OK else 0.0}


def _transient_end(transient, n_vert: int, laps: _Laps) -> tuple:
    """Once the steps are taken: (the envelope of theta (n_scen, n_vert), the step of each maximum, the hierarchies built)."""
    env, env_step = transient.envelope(n_vert)
    _steps, _time, hierarchies = transient.clock()
    laps.lap("transient_run")
    return env, env_step, hierarchies


@contextlib.contextmanager
def _transient_session(prob, meshes, mesh_index_to_layer_index, checked: CheckedTransientModel, cases, initial, probe_nodes,
                       filtered_networks, disconnected_meshes_by_layer, laps: _Laps):
    """What the two one-way transient calls do before they step, as a context: the :func:`_thermal_block` of the cases, the
    Joule heat of every mesh, the ``_hip.Transient`` with the cases' loads, and the start from ``initial``.  The value is a
    namespace: ``blk``, ``transient``, ``mesh_power`` (k, n_mesh), ``probe_idx`` (the probes' unknowns) and ``head``
    (:func:`_transient_head`).  On the way out the transient handle is closed, then the block."""
    with _thermal_block(prob, meshes, mesh_index_to_layer_index, checked.thermal, cases, filtered_networks,
                        disconnected_meshes_by_layer, laps, "temperatures over time") as blk:
        board, layer_of = blk.board, blk.board.layer_of
        # the Joule heat of every mesh's copper, per case: the sum current_cases forms of the same face powers
        *_, mesh_power, _cuts = blk.plan.current_cases(blk.k, blk.n_tri, np.asarray(layer_of, dtype=np.int32), [], np.zeros((0, 4)),
                                                       fields=False, envelope=False)
        transient = _hip.Transient(blk.thermal, [checked.capacity[layer_of[i]] for i in range(len(board.meshes))])
        try:
            transient.loads_kkt(blk.plan, blk.k, blk.heat)
            first = transient.start(initial, rtol=RTOL, max_iter=MAX_ITER)
            laps.lap("transient_start")
            probe_idx = [board.node_indexer.node_to_global_index[node] for node in probe_nodes]
            yield types.SimpleNamespace(blk=blk, transient=transient, mesh_power=mesh_power, probe_idx=probe_idx,
                                        head=_transient_head(transient, first, probe_idx))
        finally:
            transient.close()


def _case_heats(blk, mesh_power, led) -> list:
    """Per scenario (the Joule heat of every layer over time, the total heat over time) of a :func:`_thermal_block` whose
    meshes dissipate ``mesh_power`` (k, n_mesh).  ``led``: per time, the case of every scenario that led there -- the
    initial case at the start (its steady state balances it), then each step's; None = no heat."""
    k, heat, layer_of = blk.k, blk.heat, blk.board.layer_of
    n_mesh, n_layers = len(blk.board.meshes), len(blk.board.prob.layers)
    case_layer_heat = [[math.fsum(float(mesh_power[j, i]) for i in range(n_mesh) if layer_of[i] == layer_i)
                        for layer_i in range(n_layers)] for j in range(k)]
    element_heat = [math.fsum(heat[2][heat[1] == j].tolist()) if heat is not None else 0.0 for j in range(k)]
    case_total = [math.fsum(case_layer_heat[j] + [element_heat[j]]) for j in range(k)]
    if blk.sources is not None:                              # the load table's column j carries the sources of case j
        case_total = [case_total[j] + math.fsum(blk.source_power[j].tolist()) for j in range(k)]
    heats = []
    for c in range(len(led[0])):
        on = [at_time[c] for at_time in led]
        heats.append(([[0.0 if j is None else case_layer_heat[j][layer_i] for j in on] for layer_i in range(n_layers)],
                      [0.0 if j is None else case_total[j] for j in on]))
    return heats


def _transient_reports(board: IndexedBoard, ambient: float, times, head: dict, records, heats, probe_nodes, end, snapshots,
                       worst: float) -> tuple:
    """([TransientReport] per scenario, the ``info`` they share) of a transient run.  ``records``: the steps in order, in
    lots as ``Transient.run`` returns them -- ``max``, ``vertex``, ``stored``, ``loss`` (steps, n_scen, n_mesh), ``probes``
    (steps, n_scen, n_probe), ``iterations``, ``seconds``, ``setup_seconds`` and ``rel_residual`` (steps,) -- after ``head``
    (:func:`_transient_head`).  ``heats``: per scenario (the layers' heats, the total heat) that led to every time;
    ``end``: :func:`_transient_end`; ``snapshots``: [(time, theta (n_scen, n_potential))].  Warns when ``worst``, the largest
    relative residual of a step that ended above the tolerance, is worth it."""
    if worst > max(RTOL, STALL_WARN_ABOVE):
        warnings.warn(f"A step of the transient thermal solve stopped at a relative residual of {worst:.3e}", SolverWarning)
    first, (env, env_step, hierarchies) = head["result"], end
    over_time = lambda key: np.concatenate([head[key]] + [lot[key] for lot in records])        # (n_steps + 1, n_scen, ...)
    per_step = lambda key: np.concatenate([lot[key] for lot in records])                       # (n_steps,)
    mesh_max, mesh_vert, stored, loss, traces = (over_time(key) for key in ("max", "vertex", "stored", "loss", "probes"))
    iterations, seconds = per_step("iterations"), per_step("seconds")
    info = {"iterations": int(first.iterations) + int(iterations.sum()), "iterations_per_step": iterations,
            "seconds_per_step": seconds, "setup_seconds_per_step": per_step("setup_seconds"),
            "rel_residual": max([float(first.rel_residual)] + per_step("rel_residual").tolist()),
            "hierarchies": int(hierarchies), "seconds": float(first.seconds) + sum(seconds.tolist())}
    reports = [_transient_report(board, ambient, times, mesh_max[:, c], mesh_vert[:, c], stored[:, c], loss[:, c], layer_heat,
                                 total_heat, {node: traces[:, c, p] for p, node in enumerate(probe_nodes)}, env[c], env_step[c],
                                 [(when, theta[c]) for when, theta in snapshots], info)
               for c, (layer_heat, total_heat) in enumerate(heats)]
    return reports, info


def solve_meshed_thermal_transient(prob, meshes, mesh_index_to_layer_index, model: TransientModel, schedule, *, cases=None,
                                   repeat=1, probes=(), keep="end", filtered_networks=None, disconnected_meshes_by_layer=None,
                                   partition=None, timings: Optional[dict] = None):
    """How hot the copper gets, and when, under a schedule of load cases: ``([Solution] per case, [TransientReport] per
    scenario)``, with one scenario ``(solutions, report)``.

    The model (DESIGN.md "Transient") adds a heat capacity to the steady problem of :func:`solve_meshed_thermal`:

        C dtheta/dt + A theta = b(t),    C = diag(c M_v)

    with c the layer's areal heat capacity ``model.areal_capacity`` and M_v the lumped area of the vertex; internal nodes
    carry no capacity and follow the copper algebraically.  Time is stepped by backward Euler: first order,
    unconditionally stable, and free of oscillation on a load step, which is why it is preferred to Crank-Nicolson here.
    One step of length dt is one solve with S = A + C/dt from the previous state.  Every step obeys the balance
    (stored_{n+1} - stored_n) / dt + loss_{n+1} = heat of the step's case, up to the solve's tolerance.

    ``cases`` are load cases as :func:`check_load_cases` accepts them (None: the one case ``{}``, the Problem as given).
    ``schedule`` is a sequence of :class:`Segment`, each naming the case that is on (None: sources off), run ``repeat``
    times back to back (a duty cycle).  Several scenarios -- the tuple form of ``Segment.case`` and of ``model.initial`` --
    share the time grid and advance in lockstep as the columns of one block.  ``probes``: node ids (connection nodes or
    internal nodes) whose temperature traces are wanted.  ``keep``: ``"end"`` keeps the field at the end, ``"segments"`` at
    the end of every segment, ``"none"`` none.  Temperatures are theta + ambient.  The coupling is one-way: the
    resistivity does not follow the temperature; :func:`solve_meshed_electrothermal_transient` is the call in which it
    does.

    On the device: one electrical block solve of the cases on the load-case path, the thermal operator and the heat load
    of every case from the potentials it holds (the powers never visit the host), then per segment the steps, each with
    the right-hand side, the block solve from the previous state, the per-mesh report and the running envelope.  The
    ``heat_sources`` of ``model.thermal`` are part of every case's load -- a segment without a case has no source heat --
    and of ``TransientReport.total_heat``, so the balance above holds with them; the
    multigrid hierarchy of S is built once per distinct dt in a row (``info["hierarchies"]``).  ValueError, before anything
    reaches the device, for what :func:`check_transient_model`, :func:`check_load_cases`, :func:`check_schedule` and
    :func:`check_probes` refuse, an ``initial`` that names a case out of range or another number of scenarios than the
    schedule, an unknown ``keep``, and a ``partition`` over several GPUs.  A SolverWarning when a step ends above the
    tolerance.  ``timings`` (a dict) receives the host time of each stage in seconds."""
    _refuse_partition(partition, "transient temperatures")
    checked, checked_cases, flat, initial, probe_nodes = _check_transient_arguments(prob, model, schedule, cases, repeat, probes,
                                                                                     keep, filtered_networks)
    laps = _Laps(timings)
    with _transient_session(prob, meshes, mesh_index_to_layer_index, checked, checked_cases, initial, probe_nodes,
                            filtered_networks, disconnected_meshes_by_layer, laps) as ses:
        transient, runs, snapshots, worst = ses.transient, [], [], ses.head["worst"]
        t, times = 0.0, [0.0]
        for at, (dt, steps, seg_cases) in enumerate(flat):
            out = transient.run(dt, steps, seg_cases, ses.probe_idx, rtol=RTOL, max_iter=MAX_ITER)
            runs.append(out)
            worst = _worse(worst, out["result"])
            for _ in range(steps):
                t = t + dt
                times.append(t)
            if keep == "segments" or (keep == "end" and at == len(flat) - 1):
                snapshots.append((t, transient.state()))
        end = _transient_end(transient, ses.blk.n_vert, laps)
    led = [initial] + [seg_cases for _dt, steps, seg_cases in flat for _ in range(steps)]
    reports, _info = _transient_reports(ses.blk.board, checked.thermal.ambient, times, ses.head, runs,
                                        _case_heats(ses.blk, ses.mesh_power, led), probe_nodes, end, snapshots, worst)
    solutions = _block_solutions(ses.blk)
    laps.lap("solutions")
    if len(reports) == 1:
        return solutions, reports[0]
    return solutions, reports


def solve_thermal_transient(prob, model: TransientModel, schedule, mesher_config: Optional[mesh.Mesher.Config] = None, *,
                            mesher=None, cases=None, repeat=1, probes=(), keep="end", partition=None, prune=False):
    """``solve`` with the copper's temperatures over a schedule (see :func:`solve_meshed_thermal_transient`): the board is
    meshed once."""
    _refuse_partition(partition, "transient temperatures")
    _check_transient_arguments(prob, model, schedule, cases, repeat, probes, keep, None)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_thermal_transient(prob, meshes, mesh_index_to_layer_index, model, schedule, cases=cases, repeat=repeat,
                                          probes=probes, keep=keep, **pruned)


# --------------------------------------------------------------------------------------------
# periodic steady state: the regime a duty cycle settles into, by GMRES on the period (DESIGN.md "Periodic steady state")
# --------------------------------------------------------------------------------------------

MIN_PERIODS, MAX_PERIODS = 3, 4096


@dataclass
class PeriodicReport:
    """The periodic steady state of one scenario under a duty cycle (see :func:`solve_meshed_thermal_periodic`)."""
    cycle: TransientReport              # one period from the periodic state: times 0 .. T; the envelope is the hottest each vertex gets in every cycle
    closure: float                      # max_v |theta(T) - theta(0)| measured on the recorded cycle [K]
    closure_at: Optional[tuple]         # (layer index, mesh index within the layer, vertex index, x, y) of that maximum, None without vertices
    predicted: list                     # the closure the Krylov iteration predicted after each of its steps [K]
    periods: int                        # period applications spent: the first, the Krylov ones and the recorded one
    converged: bool                     # closure <= tolerance
    info: dict                          # {"iterations", "seconds"} summed over all periods, "hierarchies", "rel_residual"


def check_periodic_control(tolerance, max_periods=64) -> tuple:
    """(tolerance [K], max_periods) of the periodic iteration, or ValueError: a tolerance that is not finite and positive, a
    ``max_periods`` that is not an integer from 3 to 4096 (the first period, at least one Krylov period and the recorded
    one)."""
    tolerance = _positive_number(tolerance, "the tolerance")
    if isinstance(max_periods, bool) or not isinstance(max_periods, (int, np.integer)) or not MIN_PERIODS <= max_periods <= MAX_PERIODS:
        raise ValueError(f"max_periods must be an integer from {MIN_PERIODS} to {MAX_PERIODS}, not {max_periods!r}")
    return tolerance, int(max_periods)


def _check_periodic_arguments(prob, model, schedule, cases, probes, keep, tolerance, max_periods, filtered_networks):
    """Every check of :func:`solve_meshed_thermal_periodic`: what :func:`_check_transient_arguments` returns for one period,
    and (tolerance, max_periods)."""
    checked = check_transient_model(prob, model, filtered_networks)
    checked_cases, flat, initial, probe_nodes, control = _check_transient_call(
        prob, checked.initial, schedule, cases, 1, probes, keep, filtered_networks, check_schedule,
        lambda seg, seg_cases: (seg.duration / seg.steps, seg.steps, seg_cases),
        extra=lambda: check_periodic_control(tolerance, max_periods))
    return checked, checked_cases, flat, initial, probe_nodes, control


class _PeriodicColumn:
    """The small problem of one column of the lockstep GMRES: beta, the Hessenberg matrix, the coefficients y of the iterate
    and H y of its predicted residual.  A column is frozen when beta or a subdiagonal entry is not positive: its later
    basis vectors are zeros and its coefficients stay put."""

    def __init__(self, beta: float):
        self.beta, self.H, self.y = float(beta), np.zeros((1, 0)), np.zeros(0)
        self.frozen = not self.beta > 0.0

    def push(self, h: np.ndarray) -> None:
        if self.frozen:
            return
        j = self.H.shape[1]
        self.H = np.pad(self.H, ((0, 1), (0, 1)))
        self.H[:j + 2, j] = h
        e = np.zeros(j + 2)
        e[0] = self.beta
        self.y = np.linalg.lstsq(self.H, e, rcond=None)[0]
        self.frozen = not h[-1] > 0.0

    def padded(self, values: np.ndarray, n: int) -> np.ndarray:
        out = np.zeros(n)
        out[:len(values)] = values
        return out


def periodic_iteration(transient, periodic, flat, tolerance: float, max_periods: int) -> dict:
    """Steps 1 to 3 of the periodic iteration (DESIGN.md "Periodic steady state") on a started ``_hip.Transient`` and its
    ``_hip.Periodic``; on return the state is the iterate x0 + V y with the clock at 0.  ``flat``: the period as (dt, steps,
    per-column cases).  ``first``: the closure of the start (n_cols,), ``predicted``: per Krylov step the predicted closures
    (n_cols,), ``applications``: period applications so far, ``runs``: what every ``Transient.run`` returned."""
    n_cols = transient.n_cols
    off = [None] * n_cols
    runs = []

    def period(cases_of):
        for dt, steps, seg_cases in flat:
            runs.append(transient.run(dt, steps, cases_of(seg_cases), rtol=RTOL, max_iter=MAX_ITER))

    periodic.mark()
    period(lambda seg_cases: seg_cases)
    beta, first, _vert = periodic.residual()
    columns = [_PeriodicColumn(b) for b in beta]
    predicted = []
    if not (first <= tolerance).all():
        for j in range(max_periods - 2):
            periodic.load(j)
            period(lambda _seg_cases: off)
            h = periodic.push(j)
            for c, col in enumerate(columns):
                col.push(h[c])
            top, _vert = periodic.predict(np.stack([col.padded(col.H @ col.y, j + 2) for col in columns]))
            predicted.append(top)
            if (top <= tolerance).all() or all(col.frozen for col in columns):
                break
    n = len(predicted)
    periodic.combine(np.stack([col.padded(col.y, n) for col in columns]) if n else np.zeros((n_cols, 0)))
    return {"first": first, "predicted": predicted, "applications": 1 + n, "runs": runs}


def _vertex_place(board: IndexedBoard, vertex: int) -> Optional[tuple]:
    """(layer index, mesh index within the layer, vertex index, x, y) of a global vertex, None for -1."""
    if vertex < 0:
        return None
    voff = board.vindex.offsets
    mesh_i = int(np.searchsorted(voff, vertex, side="right") - 1)
    layer_i, v = board.layer_of[mesh_i], int(vertex - voff[mesh_i])
    in_layer = [i for i, *_ in board.layer_meshes(layer_i)].index(mesh_i)
    msh = board.meshes[mesh_i]
    return layer_i, in_layer, v, float(msh.points[v][0]), float(msh.points[v][1])


def solve_meshed_thermal_periodic(prob, meshes, mesh_index_to_layer_index, model: TransientModel, schedule, *, tolerance,
                                  cases=None, max_periods=64, probes=(), keep="end", filtered_networks=None,
                                  disconnected_meshes_by_layer=None, partition=None, timings: Optional[dict] = None):
    """The regime a duty cycle settles into -- the hottest each vertex gets in every cycle, and how far it swings --
    without running the cycle until the start-up transient has died: ``([Solution] per case, PeriodicReport)``, with
    several scenarios a list of reports.

    ``schedule`` is ONE period, a sequence of :class:`Segment` as :func:`solve_meshed_thermal_transient` takes them
    (``repeat`` is 1); ``cases``, scenarios, ``probes``, ``keep`` and the model are that call's.  ``model.initial`` is only
    the guess the iteration starts from, not part of the answer.  The period map of the fixed-step scheme is affine,
    theta(T) = Phi theta(0) + d, so the periodic state solves (I - Phi) theta* = d (DESIGN.md "Periodic steady state").
    That system is solved by GMRES without restart, per scenario, all scenarios in lockstep: a product with I - Phi is one
    period of the stepping with the sources off, and the basis stays on the device, orthogonalised in the inner product
    sum_v Cv x y in which Phi is self-adjoint.  Only the modes slower than the period sit near 1 in Phi's spectrum, so the
    iteration needs about as many periods as there are such modes, where repetition needs tau / T of them.

    ``tolerance`` [K], required, bounds the closure max_v |theta(T) - theta(0)| over the vertices.  ``max_periods`` (3 to
    4096) bounds the period applications in all: the first, the Krylov ones and the recorded one; the basis holds
    ``max_periods - 1`` vectors per scenario on the device, and MemoryError says so when that does not fit.  The iterate is
    then put into the transient handle and one period is run the normal way: ``PeriodicReport.cycle`` is the
    :class:`TransientReport` of that period -- ``times`` from 0 to T, the envelope from the periodic state, ``total_heat[0]``
    the heat of the step that leads there, the cycle's last -- and ``closure`` is measured on it.  ``predicted`` holds what
    the iteration expected after each step.  A SolverWarning when ``max_periods`` ends the iteration first (the best
    iterate's cycle is still recorded), and when the measured closure exceeds the tolerance although the predicted one met
    it, which inexact step solves can do.

    Limits: fixed-step schedules only (the adaptive controller's step choice depends on the state, so its period map is
    not affine); one-way coupling only (the electro-thermal period map is nonlinear); one GPU.  The hierarchy is rebuilt at
    every change of dt within a period, as under ``repeat=`` (``info["hierarchies"]``).  ValueError, before anything
    reaches the device, for everything :func:`solve_meshed_thermal_transient` refuses and what
    :func:`check_periodic_control` refuses."""
    _refuse_partition(partition, "periodic temperatures")
    checked, checked_cases, flat, initial, probe_nodes, (tolerance, max_periods) = _check_periodic_arguments(
        prob, model, schedule, cases, probes, keep, tolerance, max_periods, filtered_networks)
    laps = _Laps(timings)
    with _transient_session(prob, meshes, mesh_index_to_layer_index, checked, checked_cases, initial, probe_nodes,
                            filtered_networks, disconnected_meshes_by_layer, laps) as ses:
        transient, first = ses.transient, ses.head["result"]
        periodic = _hip.Periodic(transient, max_periods - 1)
        try:
            found = periodic_iteration(transient, periodic, flat, tolerance, max_periods)
            laps.lap("periodic_iteration")
            # the recorded cycle: a plain run from the iterate, as solve_meshed_thermal_transient takes it from a start
            periodic.mark()
            head = _transient_head(transient, _hip.SolveResult(None, 0, 0, 0.0, 0.0, 0.0, _hip.OK), ses.probe_idx)
            runs, snapshots, worst = [], [], ses.head["worst"]
            for out in found["runs"]:
                worst = _worse(worst, out["result"])
            t, times = 0.0, [0.0]
            for at, (dt, steps, seg_cases) in enumerate(flat):
                out = transient.run(dt, steps, seg_cases, ses.probe_idx, rtol=RTOL, max_iter=MAX_ITER)
                runs.append(out)
                worst = _worse(worst, out["result"])
                for _ in range(steps):
                    t = t + dt
                    times.append(t)
                if keep == "segments" or (keep == "end" and at == len(flat) - 1):
                    snapshots.append((t, transient.state()))
            _beta, closure, closure_vertex = periodic.residual()
            end = _transient_end(transient, ses.blk.n_vert, laps)
        finally:
            periodic.close()
    board = ses.blk.board
    led = [flat[-1][2]] + [seg_cases for _dt, steps, seg_cases in flat for _ in range(steps)]
    reports, _info = _transient_reports(board, checked.thermal.ambient, times, head, runs,
                                        _case_heats(ses.blk, ses.mesh_power, led), probe_nodes, end, snapshots, worst)
    every = found["runs"] + runs
    info = {"iterations": int(first.iterations) + int(sum(int(out["iterations"].sum()) for out in every)),
            "seconds": float(first.seconds) + float(sum(float(out["seconds"].sum()) for out in every)),
            "hierarchies": int(end[2]), "rel_residual": max([float(first.rel_residual)] + [float(out["rel_residual"].max()) for out in every])}
    periods = found["applications"] + 1
    out = []
    for c, cycle in enumerate(reports):
        predicted = [float(top[c]) for top in found["predicted"]]
        expected = predicted[-1] if predicted else float(found["first"][c])
        report = PeriodicReport(cycle=cycle, closure=float(closure[c]), closure_at=_vertex_place(board, int(closure_vertex[c])),
                                predicted=predicted, periods=periods, converged=bool(closure[c] <= tolerance), info=info)
        if not report.converged:
            where = f" of scenario {c}" if len(reports) > 1 else ""
            if expected > tolerance:
                warnings.warn(f"The periodic iteration{where} spent its {max_periods} periods: the cycle closes within "
                              f"{report.closure:.3e} K, not {tolerance:.3e} K", SolverWarning)
            else:
                warnings.warn(f"The recorded cycle{where} closes within {report.closure:.3e} K although {expected:.3e} K was "
                              f"predicted: the step solves are inexact at a tolerance of {tolerance:.3e} K", SolverWarning)
        out.append(report)
    solutions = _block_solutions(ses.blk)
    laps.lap("solutions")
    if len(out) == 1:
        return solutions, out[0]
    return solutions, out


def solve_thermal_periodic(prob, model: TransientModel, schedule, mesher_config: Optional[mesh.Mesher.Config] = None, *,
                           mesher=None, tolerance, cases=None, max_periods=64, probes=(), keep="end", partition=None,
                           prune=False):
    """``solve`` with the periodic steady state of a duty cycle (see :func:`solve_meshed_thermal_periodic`): the board is
    meshed once."""
    _refuse_partition(partition, "periodic temperatures")
    _check_periodic_arguments(prob, model, schedule, cases, probes, keep, tolerance, max_periods, None)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_thermal_periodic(prob, meshes, mesh_index_to_layer_index, model, schedule, tolerance=tolerance, cases=cases,
                                         max_periods=max_periods, probes=probes, keep=keep, **pruned)


# --------------------------------------------------------------------------------------------
# adaptive transient: second-order steps whose size follows an error estimate (DESIGN.md "Adaptive transient")
# --------------------------------------------------------------------------------------------

SDIRK_GAMMA = _hip.SDIRK_GAMMA          # 1 - 1/sqrt(2)
DEFAULT_FIRST_LEVEL = 10                # the first step of a span is duration / 2^10 ...
DEFAULT_MAX_LEVEL = 30                  # ... and no step is shorter than duration / 2^30


@dataclass
class Span:
    """A stretch of a schedule with one load, covered by as many steps as the tolerance asks for (see
    :func:`solve_meshed_thermal_transient_adaptive`).

    - ``duration``: seconds, finite and positive.
    - ``case``: as in :class:`Segment`."""
    duration: float
    case: object = None


def check_spans(schedule, n_cases: int, repeat=1) -> tuple:
    """(the flattened spans, the number of scenarios) of a schedule of :class:`Span`, or ValueError: :func:`check_schedule`
    without the steps.  Refused: an empty schedule, an entry that is no Span, a duration that is not finite and positive, a
    case out of range, tuples of unequal length and ``repeat < 1``."""
    checked, n_scen = _check_entries(schedule, n_cases, repeat, Span)
    return [dataclasses.replace(span) for _ in range(int(repeat)) for span in checked], n_scen


def check_step_control(tolerance, first_step=None, min_step=None, max_steps=MAX_TRANSIENT_STEPS) -> tuple:
    """(tolerance [K], first_step, min_step [s] or None, max_steps) of the step-size control, or ValueError: a tolerance that
    is not finite and positive; a ``first_step`` or ``min_step`` that is neither None nor finite and positive;
    ``min_step > first_step``; a ``max_steps`` that is not an integer >= 1."""
    tolerance = _positive_number(tolerance, "the tolerance")
    first_step = None if first_step is None else _positive_number(first_step, "first_step")
    min_step = None if min_step is None else _positive_number(min_step, "min_step")
    if first_step is not None and min_step is not None and min_step > first_step:
        raise ValueError(f"min_step ({min_step}) must not exceed first_step ({first_step})")
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or max_steps < 1:
        raise ValueError(f"max_steps must be an integer >= 1, not {max_steps!r}")
    return tolerance, first_step, min_step, int(max_steps)


def dyadic_levels(duration: float, first_step=None, min_step=None) -> tuple:
    """(the level k a span of ``duration`` starts at, the deepest level it may reach): steps are duration / 2^k.  The start is
    the smallest k >= 0 with duration / 2^k <= first_step (None: duration / 1024), the deepest the largest k with
    duration / 2^k >= min_step (None: duration / 2^30; 0 when even the whole span is shorter)."""
    start = DEFAULT_FIRST_LEVEL
    if first_step is not None:
        start = 0
        while math.ldexp(duration, -start) > first_step:
            start += 1
    deepest = DEFAULT_MAX_LEVEL
    if min_step is not None:
        deepest = 0
        while math.ldexp(duration, -(deepest + 1)) >= min_step:
            deepest += 1
    return start, deepest


def dyadic_controller(duration: float, tolerance: float, first_step=None, min_step=None):
    """The step-size rule of one span as a generator: deterministic, and every step a dyadic fraction of the span, so that
    steps land exactly on its end.  It yields ``(verdict, dt, level, pos)``: the verdict on the trial just judged (None at
    first; "accept", "forced" or "reject"), the next step to try, dt = duration / 2^level (None once the span is covered),
    and ``pos``, the accepted steps in units of that dt -- the time reached is pos * dt after the span's begin.  ``send`` it
    the error estimate of the trial, the largest over the columns.

    - reject: err > tolerance above the deepest level: level + 1, pos * 2, again from the same state;
    - forced: err > tolerance at the deepest level (:func:`dyadic_levels`): accepted all the same;
    - accept: pos + 1; the span ends when pos = 2^level;
    - grow: after an accepted step with err <= tolerance / 4 (the estimate goes with dt^2), an even pos and level > 0:
      level - 1, pos / 2.

    An estimate that is not finite raises RuntimeError."""
    level, deepest = dyadic_levels(duration, first_step, min_step)
    pos, verdict = 0, None
    while True:
        err = yield verdict, math.ldexp(duration, -level), level, pos
        err = float(err)
        if not math.isfinite(err):
            raise RuntimeError(f"the error estimate of a step of {math.ldexp(duration, -level)} s is not finite")
        if err > tolerance and level < deepest:
            level, pos, verdict = level + 1, pos * 2, "reject"
            continue
        verdict = "forced" if err > tolerance else "accept"
        pos += 1
        if pos == 2 ** level:
            yield verdict, None, level, pos
            return
        if err <= tolerance / 4 and pos % 2 == 0 and level > 0:
            level, pos = level - 1, pos // 2


def adaptive_walk(spans, tolerance: float, first_step, min_step, max_steps: int, try_step, accept, end_of_span=None) -> dict:
    """:func:`dyadic_controller` over ``spans`` = [(duration, load)], on the host.  ``try_step(dt, load)`` returns the error
    estimates of a trial (their largest decides); ``accept(dt, time, load, errors)`` is called for every step that is taken,
    with the time it reaches: the begin of the span + pos * dt, and begin + duration at its end, where the begins add up as
    the durations do; ``end_of_span(index, time)`` after the last step of every span.  Returns {"tried", "rejected",
    "forced", "decisions": the verdict on every trial in order}.  One SolverWarning per call when steps were forced;
    RuntimeError for an estimate that is not finite and when ``max_steps`` trials do not cover the schedule (the message names
    the time reached)."""
    decisions, begin = [], 0.0
    for at, (duration, load) in enumerate(spans):
        control = dyadic_controller(duration, tolerance, first_step, min_step)
        _verdict, dt, _level, pos = next(control)
        while dt is not None:
            if len(decisions) >= max_steps:
                control.close()
                raise RuntimeError(f"{max_steps} steps tried and the schedule is not covered: t = {begin + pos * dt} s reached "
                                   f"with a step of {dt} s")
            errors = np.asarray(try_step(dt, load), dtype=DTYPE).reshape(-1)
            worst = float(errors.max()) if np.isfinite(errors).all() else float("nan")
            # (after a growth pos counts in units of the doubled step: pos * dt is the same number either way)
            verdict, dt_next, _level, pos = control.send(worst)
            decisions.append(verdict)
            if verdict != "reject":
                accept(dt, begin + (duration if dt_next is None else pos * dt_next), load, errors)
            dt = dt_next
        begin = begin + duration
        if end_of_span is not None:
            end_of_span(at, begin)
    forced = decisions.count("forced")
    if forced:
        warnings.warn(f"{forced} steps were accepted above the tolerance of {tolerance} K at the smallest step allowed",
                      SolverWarning)
    return {"tried": len(decisions), "rejected": decisions.count("reject"), "forced": forced, "decisions": decisions}


def _check_adaptive_transient_arguments(prob, model, schedule, cases, repeat, probes, keep, tolerance, first_step, min_step,
                                        max_steps, filtered_networks):
    """Every check of :func:`solve_meshed_thermal_transient_adaptive`: (checked model, checked cases, per flattened span
    (duration, per-scenario cases), per-scenario initial cases, probes, the step control)."""
    checked = check_transient_model(prob, model, filtered_networks)
    return (checked, *_check_transient_call(
        prob, checked.initial, schedule, cases, repeat, probes, keep, filtered_networks, check_spans,
        lambda span, span_cases: (span.duration, span_cases),
        extra=lambda: check_step_control(tolerance, first_step, min_step, max_steps)))


def solve_meshed_thermal_transient_adaptive(prob, meshes, mesh_index_to_layer_index, model: TransientModel, schedule, *,
                                            tolerance, cases=None, repeat=1, probes=(), keep="end", first_step=None,
                                            min_step=None, max_steps=MAX_TRANSIENT_STEPS, filtered_networks=None,
                                            disconnected_meshes_by_layer=None, partition=None, timings: Optional[dict] = None):
    """:func:`solve_meshed_thermal_transient` without a time grid to choose: second-order steps whose size follows an error
    estimate.  ``schedule`` is a sequence of :class:`Span` (a duration and the case that is on), ``tolerance`` the error in
    kelvin a single step may add at any vertex.  The return value has the shape of the fixed-step call; ``times`` is not
    uniform, and the envelope's steps count the accepted steps.

    A step (DESIGN.md "Adaptive transient") is Alexander's two-stage SDIRK2 -- second order, L-stable like backward Euler and
    so free of ringing on a load step -- from two backward-Euler solves of length gamma dt, gamma = 1 - 1/sqrt(2), on one
    matrix.  Its difference to the embedded first-order solution estimates the step's error, conservatively.  Per span of
    duration D the step is D / 2^k (:func:`dyadic_controller`): it starts at ``first_step`` (None: D / 1024), halves when the
    estimate exceeds the tolerance, doubles when it is below a quarter of it and the position allows, and never falls below
    ``min_step`` (None: D / 2^30), where steps are accepted with one SolverWarning per call.  Steps land exactly on the ends
    of the spans, and two calls take the same path.  Every accepted step obeys
    (stored_{n+1} - stored_n) / dt + (1 - gamma) stage_loss + gamma loss_{n+1} = heat of the span's case.

    ``info`` holds what the fixed-step call's does (``iterations_per_step`` the sum of a step's two solves, ``hierarchies``
    one per run of equal steps) and ``"step_sizes"`` (n_steps,), ``"error_estimates"`` (n_steps, n_scenarios) [K],
    ``"stage_loss"`` (n_steps, n_scenarios): the film loss of the first stage [W], ``"stage_iterations"`` (n_steps, 2),
    ``"tried"`` and ``"rejected"`` and ``"tried_step_sizes"`` (tried,), the rejected trials included.  ValueError, before anything reaches the device, for what the fixed-step call refuses of
    its arguments, what :func:`check_spans` and :func:`check_step_control` refuse, and a ``partition`` over several GPUs;
    RuntimeError for an estimate that is not finite and when ``max_steps`` trials do not cover the schedule."""
    _refuse_partition(partition, "transient temperatures")
    checked, checked_cases, flat, initial, probe_nodes, control = _check_adaptive_transient_arguments(
        prob, model, schedule, cases, repeat, probes, keep, tolerance, first_step, min_step, max_steps, filtered_networks)
    tolerance, first_step, min_step, max_steps = control
    laps, n_scen = _Laps(timings), len(initial)
    with _transient_session(prob, meshes, mesh_index_to_layer_index, checked, checked_cases, initial, probe_nodes,
                            filtered_networks, disconnected_meshes_by_layer, laps) as ses:
        transient = ses.transient
        steps, times, led, snapshots, last, tried_sizes, worst = [], [0.0], [initial], [], {}, [], [ses.head["worst"]]

        def try_step(dt, seg_cases):
            last["trial"] = transient.try_step(dt, seg_cases, rtol=RTOL, max_iter=MAX_ITER)
            tried_sizes.append(dt)
            worst[0] = _worse(worst[0], last["trial"]["result"])
            return last["trial"]["err"]

        def accept(dt, time, seg_cases, errors):
            out, trial = transient.accept(ses.probe_idx), last["trial"]
            # a lot of one step, as Transient.run would have recorded it: the iterations of a step are those of its two stages
            steps.append(dict({key: out[key][None] for key in ("max", "vertex", "stored", "loss", "probes")},
                              iterations=trial["stage_iterations"].sum(keepdims=True).astype(np.int32),
                              seconds=[float(trial["result"].seconds)], setup_seconds=[float(trial["stage_setup_seconds"].sum())],
                              rel_residual=[float(trial["result"].rel_residual)], dt=dt, err=errors.copy(),
                              stage_loss=out["stage_loss"], stage_iterations=trial["stage_iterations"]))
            times.append(time)
            led.append(seg_cases)

        def end_of_span(at, time):
            if keep == "segments" or (keep == "end" and at == len(flat) - 1):
                snapshots.append((time, transient.state()))

        walk = adaptive_walk(flat, tolerance, first_step, min_step, max_steps, try_step, accept, end_of_span)
        end = _transient_end(transient, ses.blk.n_vert, laps)
    reports, info = _transient_reports(ses.blk.board, checked.thermal.ambient, times, ses.head, steps,
                                       _case_heats(ses.blk, ses.mesh_power, led), probe_nodes, end, snapshots, worst[0])
    n_steps = len(steps)
    info.update({
        "step_sizes": np.array([out["dt"] for out in steps], dtype=DTYPE),
        "error_estimates": np.array([out["err"] for out in steps], dtype=DTYPE).reshape(n_steps, n_scen),
        "stage_loss": np.array([[math.fsum(out["stage_loss"][c].tolist()) for c in range(n_scen)] for out in steps],
                               dtype=DTYPE).reshape(n_steps, n_scen),
        "stage_iterations": np.array([out["stage_iterations"] for out in steps], dtype=np.int32).reshape(n_steps, 2),
        "tried": walk["tried"], "rejected": walk["rejected"], "tried_step_sizes": np.array(tried_sizes, dtype=DTYPE)})
    solutions = _block_solutions(ses.blk)
    laps.lap("solutions")
    if n_scen == 1:
        return solutions, reports[0]
    return solutions, reports


def solve_thermal_transient_adaptive(prob, model: TransientModel, schedule, mesher_config: Optional[mesh.Mesher.Config] = None, *,
                                     tolerance, mesher=None, cases=None, repeat=1, probes=(), keep="end", first_step=None,
                                     min_step=None, max_steps=MAX_TRANSIENT_STEPS, partition=None, prune=False):
    """``solve`` with the copper's temperatures over a schedule of spans (see
    :func:`solve_meshed_thermal_transient_adaptive`): the board is meshed once."""
    _refuse_partition(partition, "transient temperatures")
    _check_adaptive_transient_arguments(prob, model, schedule, cases, repeat, probes, keep, tolerance, first_step, min_step,
                                        max_steps, None)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_thermal_transient_adaptive(prob, meshes, mesh_index_to_layer_index, model, schedule, tolerance=tolerance,
                                                   cases=cases, repeat=repeat, probes=probes, keep=keep, first_step=first_step,
                                                   min_step=min_step, max_steps=max_steps, **pruned)


# --------------------------------------------------------------------------------------------
# electro-thermal: the copper's conductance follows its temperature (DESIGN.md "Electro-thermal")
# --------------------------------------------------------------------------------------------

COPPER_TEMPERATURE_COEFFICIENT = 3.93e-3        # alpha [1/K] of copper's resistivity around room temperature


class ThermalRunawayError(RuntimeError):
    """The Picard loop of :func:`solve_meshed_electrothermal` diverges: the increments grew in three consecutive rounds."""


@dataclass
class ElectroThermalModel:
    """What couples the temperatures back into the conductances (see :func:`solve_meshed_electrothermal`).

    - ``thermal``: the :class:`ThermalModel`.
    - ``temperature_coefficient``: alpha [1/K], one float for all layers or a mapping {layer or layer name: float}; a layer
      that is not named gets copper's 3.93e-3.  A face at the mean temperature T conducts
      ``layer.conductance / (1 + alpha (T - conductance_temperature))``.
    - ``conductance_temperature``: T0, the temperature at which ``Layer.conductance`` holds, in the unit of
      ``thermal.ambient``.
    - ``tolerance``: the loop stops when no face mean (and no resistor's mean) moved by more than this [K] in a round.
    - ``max_rounds``: the most rounds of the loop.
    - ``resistor_coefficient``: None = lumped resistors keep their resistance; a float = that alpha [1/K] for every
      ``Resistor`` of the solved networks (vias are copper barrels: 3.93e-3); a mapping {Resistor: alpha} names resistors by
      identity or equality, the others get 0.  A resistor at the mean temperature T of its two ends has the resistance
      ``resistance * (1 + alpha (T - resistor_temperature))``.
    - ``resistor_temperature``: T0 of the resistors, the temperature at which ``Resistor.resistance`` holds; None =
      ``conductance_temperature``."""
    thermal: ThermalModel
    temperature_coefficient: object = COPPER_TEMPERATURE_COEFFICIENT
    conductance_temperature: float = 20.0
    tolerance: float = 0.01
    max_rounds: int = 20
    resistor_coefficient: object = None
    resistor_temperature: Optional[float] = None


@dataclass
class CheckedElectroThermalModel:
    """An :class:`ElectroThermalModel` resolved against a Problem (:func:`check_electrothermal_model`)."""
    thermal: CheckedThermalModel
    alpha: list                # per layer
    conductance_temperature: float
    tolerance: float
    max_rounds: int
    resistor_alpha: Optional[list] = None      # per resistor in the order of global_elements' ("R", a, b, R) rows, or None
    resistor_t0: float = 20.0

    def resistors_follow(self) -> bool:
        """Whether a resistor's resistance moves with its temperature."""
        return self.resistor_alpha is not None and any(a != 0.0 for a in self.resistor_alpha)


@dataclass
class CouplingReport:
    """How the loop of :func:`solve_meshed_electrothermal` went for one load case."""
    rounds: int
    converged: bool
    increments: list           # d_k [K] of every round: the largest change of a face's mean temperature
    conductance_scale: list    # per layer, per mesh: TwoForm of s_f, the scale the last electrical solve used
    iterations: list           # per round: {"electrical": iterations of the electrical solve, "thermal": of the thermal one}
    elements: dict             # lumped element -> its element_flows entry in the last electrical solve (current, power, ...)
    # Resistor -> {"temperature", "scale", "resistance"} of the last electrical solve: the mean temperature of its ends, s_r
    # and resistance / s_r; empty without a resistor_coefficient
    resistors: dict = field(default_factory=dict)


def check_electrothermal_model(prob, model, filtered_networks=None) -> CheckedElectroThermalModel:
    """``model`` resolved against ``prob``, or ValueError -- before anything reaches the device -- for what
    :func:`check_thermal_model` refuses in ``model.thermal``; a temperature coefficient or conductance temperature that is
    not finite; a mapping key that is no layer of the Problem; a tolerance that is not finite and positive; ``max_rounds``
    below 1; an ambient temperature at which a layer's 1 + alpha (ambient - T0) is not positive; a resistor coefficient or
    resistor temperature that is not finite; a ``resistor_coefficient`` key that is no Resistor of the Problem; and a
    resistor whose 1 + alpha (ambient - T0) is not positive."""
    if not isinstance(model, ElectroThermalModel):
        raise ValueError("model must be an ElectroThermalModel")
    thermal = check_thermal_model(prob, model.thermal, filtered_networks)

    def finite(value, what):
        try:
            x = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{what} must be a number, not {value!r}") from None
        if not math.isfinite(x):
            raise ValueError(f"{what} must be finite, not {value!r}")
        return x

    t0 = finite(model.conductance_temperature, "the conductance temperature")
    alpha = [COPPER_TEMPERATURE_COEFFICIENT] * len(prob.layers)
    if isinstance(model.temperature_coefficient, Mapping):
        for key, value in model.temperature_coefficient.items():
            if isinstance(key, str):
                found = [i for i, layer in enumerate(prob.layers) if layer.name == key]
            else:
                found = [i for i, layer in enumerate(prob.layers) if layer is key or layer == key]
            if not found:
                raise ValueError(f"temperature_coefficient: {key!r} is no layer of the Problem")
            for i in found:
                alpha[i] = finite(value, f"the temperature coefficient of layer {prob.layers[i].name!r}")
    else:
        alpha = [finite(model.temperature_coefficient, "the temperature coefficient")] * len(prob.layers)
    tolerance = _positive_number(model.tolerance, "the tolerance")
    try:
        max_rounds = int(model.max_rounds)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"max_rounds must be an integer, not {model.max_rounds!r}") from None
    if max_rounds < 1 or max_rounds != model.max_rounds:
        raise ValueError(f"max_rounds must be an integer of at least 1, not {model.max_rounds!r}")
    for layer, a in zip(prob.layers, alpha):
        if not 1 + a * (thermal.ambient - t0) > 0.0:
            raise ValueError(f"layer {layer.name!r}: 1 + alpha (ambient - T0) = {1 + a * (thermal.ambient - t0)!r} is not "
                             "positive: the conductance model does not hold at the ambient temperature")
    resistor_t0 = t0 if model.resistor_temperature is None else finite(model.resistor_temperature, "the resistor temperature")
    resistor_alpha = None
    if model.resistor_coefficient is not None:
        networks = list(prob.networks) if filtered_networks is None else list(filtered_networks)
        resistors = [e for network in networks for e in network.elements if element_kind(e) == "Resistor"]
        if isinstance(model.resistor_coefficient, Mapping):
            every = [e for network in prob.networks for e in network.elements]
            given = []
            for key, value in model.resistor_coefficient.items():
                if element_kind(key) != "Resistor" or not any(e is key or e == key for e in every):
                    raise ValueError(f"resistor_coefficient: {key!r} is no Resistor of the Problem")
                given.append((key, finite(value, "the temperature coefficient of a Resistor")))
            resistor_alpha = [0.0] * len(resistors)
            for key, value in given:
                for i, e in enumerate(resistors):
                    if e is key or e == key:
                        resistor_alpha[i] = value
        else:
            resistor_alpha = [finite(model.resistor_coefficient, "the resistor coefficient")] * len(resistors)
        for e, a in zip(resistors, resistor_alpha):
            if not 1 + a * (thermal.ambient - resistor_t0) > 0.0:
                raise ValueError(f"{e!r}: 1 + alpha (ambient - T0) = {1 + a * (thermal.ambient - resistor_t0)!r} is not positive: "
                                 "the resistance model does not hold at the ambient temperature")
    return CheckedElectroThermalModel(thermal=thermal, alpha=alpha, conductance_temperature=t0, tolerance=tolerance,
                                      max_rounds=max_rounds, resistor_alpha=resistor_alpha, resistor_t0=resistor_t0)


def picard_verdict(increments, tolerance: float) -> Optional[str]:
    """What the increments d_1 .. d_k say after round k: "converged" when d_k <= tolerance, "runaway" when d grew in three
    consecutive rounds (d_k > d_k-1 > d_k-2 > d_k-3), else None."""
    d = list(increments)
    if d[-1] <= tolerance:
        return "converged"
    if len(d) >= 4 and d[-1] > d[-2] > d[-3] > d[-4]:
        return "runaway"
    return None


def _drop_plans(L: SystemMatrix) -> None:
    """The device plans kept with ``L`` hold A = -P^T L P of L's values: closed before those change."""
    for plan in L._plans.values():
        plan.close()
    L._plans.clear()
    L._host = None


@contextlib.contextmanager
def _coupled_handles(board: IndexedBoard, pairs, electro: CheckedElectroThermalModel, laps: _Laps, capacity=None, n_loads=0):
    """What both electro-thermal calls hold on the device, as a context: the assembled system ``L``, the ``thermal`` handle of
    ``electro.thermal`` on it, the ``coupled`` handle, the attached heat ``sources`` (None without) and, given the layers'
    ``capacity``, a ``transient`` handle with room for ``n_loads`` loads (else None); with them ``resistors`` and ``n_tri``.
    On the way out: the transient handle, the plans kept with L, the coupling, the thermal handle, L."""
    thermal_model, layer_of, n_mesh = electro.thermal, board.layer_of, len(board.meshes)
    with board.assembled() as (L, _):
        laps.lap("assembly")
        resistors = [(element, row) for element, row in pairs if row[0] == "R"]
        thermal = _thermal_handle(L, L.layout.n_potential, thermal_model, layer_of, n_mesh, resistors)
        coupled = transient = None
        try:
            coupled = _hip.Coupled(L.dev, thermal, [electro.alpha[layer_of[i]] for i in range(n_mesh)], thermal_model.ambient,
                                   electro.conductance_temperature)
            if electro.resistor_alpha is not None:
                coupled.set_resistors([row[1] for _, row in resistors], [row[2] for _, row in resistors],
                                      [row[3] for _, row in resistors], electro.resistor_alpha,
                                      [electro.resistor_t0] * len(resistors))
            sources = _attach_heat_sources(thermal, board.prob, thermal_model, layer_of, n_mesh)
            if capacity is not None:
                transient = _hip.Transient(thermal, [capacity[layer_of[i]] for i in range(n_mesh)])
                transient.reserve_loads(n_loads)
            laps.lap("thermal_setup")
            yield types.SimpleNamespace(L=L, thermal=thermal, coupled=coupled, transient=transient, sources=sources,
                                        resistors=resistors, n_tri=len(L.tri), resistor_alpha=electro.resistor_alpha)
        finally:
            if transient is not None:
                transient.close()
            if coupled is not None:
                _drop_plans(L)
                coupled.close()
            thermal.close()


def _revalued_solve(handles, board: IndexedBoard, pairs, case: dict, stamps, element_heat: bool, laps: _Laps):
    """One electrical solve of ``case`` (``stamps``: its :func:`stamp_load_cases`) on the conductances the coupling holds: the
    plans of ``handles.L`` dropped, L revalued, a fresh plan and the block solve of one column.  A namespace of ``plan``,
    ``V``, ``residual_norms``, ``res``, ``cols`` and ``vals``, the case's element rows ``case_rows`` with their ``flows``, and
    ``heat``: the resistors' node-heat triples, None without ``element_heat``."""
    rows, cols, vals = stamps
    _drop_plans(handles.L)
    handles.coupled.revalue()
    resistor_state = None
    if handles.resistor_alpha is not None:                   # (the used scale and the means it came from)
        resistor_state = handles.coupled.get_resistors(len(handles.resistors), used=True, means=True)
    laps.lap("revalue")
    plan, V, residual_norms, res, _n_tri, _n_mesh = _solve_block_on_device(handles.L, rows, cols, vals, 1, 1, laps)
    local, Vu = _gather_element_rows([row for _, row in pairs], V, _ROW_UNKNOWNS)
    case_rows = _case_element_rows(pairs, local, case)
    if resistor_state is not None:                           # the resistance this solve used: R_r / s_r, one division
        scales = iter(resistor_state[0].tolist())
        case_rows = [row[:3] + (row[3] / next(scales),) if row[0] == "R" else row for row in case_rows]
    flows = element_flows(case_rows, Vu[:, 0])
    heat = thermal_heat_triples(pairs, [flows]) if element_heat else None
    return types.SimpleNamespace(plan=plan, V=V, residual_norms=residual_norms, res=res, cols=cols, vals=vals,
                                 case_rows=case_rows, flows=flows, heat=heat, resistor_state=resistor_state)


def _picard(round_fn, electro: CheckedElectroThermalModel) -> tuple:
    """The Picard loop: ``round_fn(round)`` runs a round and returns its increment d [K].  (the increments, the verdict of
    :func:`picard_verdict` on them, None when ``electro.max_rounds`` ended the loop); with every alpha 0, of the layers and
    of the resistors, and no film curve one round converges."""
    one_round = all(a == 0.0 for a in electro.alpha) and not electro.thermal.curved() and not electro.resistors_follow()
    increments, verdict = [], None
    for round_i in range(1, electro.max_rounds + 1):
        increments.append(round_fn(round_i))
        verdict = "converged" if one_round else picard_verdict(increments, electro.tolerance)
        if verdict is not None:
            break
    return increments, verdict


def _picard_outcome(verdict, increments, where: str, board: IndexedBoard, electro: CheckedElectroThermalModel, hottest) -> bool:
    """Whether the loop of :func:`_picard` converged: :class:`ThermalRunawayError` on "runaway", a SolverWarning when the
    rounds ran out, both beginning with ``where``.  ``hottest()`` returns the largest theta of every mesh (n_mesh,) and is
    called on runaway only."""
    if verdict == "runaway":
        mesh_max = hottest()
        layer = board.prob.layers[board.layer_of[int(np.argmax(mesh_max))]].name
        raise ThermalRunawayError(
            f"{where}: thermal runaway -- the largest change of a face temperature grew in rounds {len(increments) - 3} to "
            f"{len(increments)}: {', '.join(f'{d:.6g} K' for d in increments[-4:])}; the hottest layer is "
            f"{layer!r} at {float(mesh_max.max()) + electro.thermal.ambient:.6g}.  A current-driven conductor "
            "whose heating outgrows its cooling has no steady state")
    if verdict != "converged":
        warnings.warn(f"{where}: the electro-thermal loop did not converge in {electro.max_rounds} round(s): "
                      f"the last change of a face temperature was {increments[-1]:.3e} K, above the tolerance of "
                      f"{electro.tolerance:.3e} K", SolverWarning)
    return verdict == "converged"


def _solve_electrothermal(prob, meshes, mesh_index_to_layer_index, checked: CheckedElectroThermalModel, cases, fields: bool,
                          filtered_networks, disconnected_meshes_by_layer, laps: _Laps):
    """The checked ``cases`` of ``prob``, each converged by the Picard loop on one assembly and one thermal handle:
    ([Solution], [ThermalReport], [CouplingReport], ThermalEnvelope)."""
    thermal_model, n_layers = checked.thermal, len(prob.layers)
    curved = thermal_model.curved()
    board, pairs, substituted, source_power, n_vert, k = _thermal_board(
        prob, meshes, mesh_index_to_layer_index, thermal_model, cases, filtered_networks, disconnected_meshes_by_layer)
    laps.lap("indexing")
    rounds_log = []
    if laps.timings is not None:
        laps.timings["rounds"] = rounds_log
    per_case, stack_flows, source_rises = [], [], []
    with _coupled_handles(board, pairs, checked, laps) as h:
        thermal, coupled, sources, resistors, n_tri = h.thermal, h.coupled, h.sources, h.resistors, h.n_tri
        for j, case in enumerate(cases):
            stamps = stamp_load_cases(board.filtered_networks, board.node_indexer, h.L.shape[0], [case])
            log.info(f"Load case {j}: the electro-thermal loop")
            if j > 0:
                coupled.reset()
            if sources is not None:                          # the same watts in every round: not scaled by the resistivity
                thermal.source_power(source_power[j:j + 1])
            iterations, last = [], {}
            film = {"increments": [], "vertices": [], "beyond": 0} if curved else None

            def one_round(round_i):
                lap = {}
                round_laps = _Laps(lap)
                if curved:                                   # the film about the current theta: both couplings in one loop
                    thermal.film_linearise(round_i > 1)
                    round_laps.lap("linearise")
                el = _revalued_solve(h, board, pairs, case, stamps, thermal_model.element_heat, round_laps)
                theta, tres = coupled.solve_kkt(el.plan, el.heat, rtol=RTOL, max_iter=MAX_ITER)
                round_laps.lap("thermal_solve")
                increment = coupled.update()
                round_laps.lap("update")
                if curved:
                    moved, vertex, film["beyond"] = thermal.film_increment()
                    film["increments"].append(moved)
                    film["vertices"].append(vertex)
                    increment = max(increment, moved)
                    round_laps.lap("increment")
                iterations.append({"electrical": int(el.res.iterations), "thermal": int(tres.iterations)})
                rounds_log.append(dict(lap, case=j, round=round_i))
                last.update(el=el, theta=theta, tres=tres)
                return increment

            increments, verdict = _picard(one_round, checked)
            converged = _picard_outcome(verdict, increments, f"Load case {j}", board, checked,
                                        lambda: thermal.report(1, n_tri, n_vert, fields=False, envelope=False)[1][0])
            el = last["el"]
            power = coupled.power_density(el.plan, n_tri)
            scale = coupled.get_scale(n_tri, used=True)
            report = thermal.report(1, n_tri, n_vert, fields=fields, envelope=False)
            stack_flows.append(_stack_flows(thermal, thermal_model, 1))
            if sources is not None:
                source_rises.append(thermal.source_report(1))
            if curved:
                film = {"rounds": len(increments), "increments": film["increments"], "vertices": film["vertices"],
                        "converged": converged, "beyond": film["beyond"]}
            per_case.append((el.V, el.residual_norms, el.res, el.cols, el.vals, power, scale, last["theta"], last["tres"], report,
                             el.heat, increments, iterations, converged, el.flows, film, el.resistor_state))
        laps.lap("loop")
    laps.lap()
    solutions, couplings, infos = [], [], []
    for j, (V, residual_norms, res, cols, vals, power, scale, theta, tres, report, heat, increments, iterations,
            converged, flows, _film, resistor_state) in enumerate(per_case):
        where = f"Load case {j}: " if k > 1 else ""
        _warn_if_block_stalled(res, residual_norms, cols, vals, 1)
        if tres.status != _hip.OK and not tres.rel_residual <= max(RTOL, STALL_WARN_ABOVE):
            warnings.warn(f"{where}The thermal solve stopped at a relative residual of {tres.rel_residual:.3e}", SolverWarning)
        solutions.append(_column_solution(board, substituted[j][0], np.ascontiguousarray(V[:, 0]), residual_norms[0], res, power,
                                          where))
        infos.append({"iterations": int(tres.iterations), "rel_residual": float(tres.rel_residual), "seconds": float(tres.seconds)})
        scales = []
        for layer_i in range(n_layers):
            tfs = []
            for _mesh_i, msh, lo, hi in board.layer_meshes(layer_i):
                tf = mesh.TwoForm(msh)
                tf.values = scale[lo:hi]
                tfs.append(tf)
            scales.append(tfs)
        renamed = substituted[j][1]
        case_elements = [e for network in board.filtered_networks for e in renamed.get(id(network), network).elements]
        followed = {}
        if resistor_state is not None:
            case_resistors = [e for e, (_, row) in zip(case_elements, pairs) if row[0] == "R"]
            for e, (_, row), s_r, mean_r in zip(case_resistors, resistors, resistor_state[0].tolist(), resistor_state[1].tolist()):
                followed[e] = {"temperature": mean_r + thermal_model.ambient, "scale": s_r, "resistance": row[3] / s_r}
        couplings.append(CouplingReport(rounds=len(increments), converged=converged, increments=increments,
                                        conductance_scale=scales, iterations=iterations,
                                        elements=dict(zip(case_elements, flows)), resistors=followed))
    theta = np.concatenate([c[7] for c in per_case])
    stacked = [None if not fields and i == 0 else np.concatenate([c[9][i] for c in per_case]) for i in range(5)]
    heat_val = np.stack([c[10][2].reshape(len(resistors), 2) for c in per_case]) if thermal_model.element_heat else None
    stack = (np.concatenate([f[0] for f in stack_flows]), stack_flows[0][1]) if thermal_model.interlayer else None
    heat_sources = None if sources is None else (sources, source_power, np.concatenate(source_rises))
    reports = _thermal_reports(board, thermal_model, substituted, resistors, fields, theta, *stacked, heat_val, infos, stack,
                               heat_sources)
    for report, case in zip(reports, per_case):
        report.film = case[15]
    env, env_case = envelope_of(theta[:, :n_vert])
    envelope = _thermal_envelope(board, thermal_model.ambient, env, env_case, reports)
    laps.lap("solutions")
    return solutions, reports, couplings, envelope


def solve_meshed_electrothermal(prob, meshes, mesh_index_to_layer_index, model: ElectroThermalModel, *, cases=None,
                                per_case_fields=True, filtered_networks=None, disconnected_meshes_by_layer=None, partition=None,
                                timings: Optional[dict] = None):
    """``solve_meshed_thermal`` with the loop closed: the sheet conductance of every face follows its temperature, so the
    drops, currents and temperatures are those of the warm copper.  ``(Solution, ThermalReport, CouplingReport)``, or for a
    list of load ``cases`` ``([Solution], [ThermalReport], [CouplingReport], ThermalEnvelope)``.

    Face f of a mesh of layer m conducts ``sigma_m s_f`` with ``s_f = 1 / (1 + alpha_m (Tbar_f - T0))``, ``Tbar_f`` the mean
    of its corners' temperatures as the ThermalReport's ``face_temperatures`` hold it.  The thermal side stays as it is: by
    Wiedemann-Franz kappa = L0 T sigma(T) is constant to first order.  Lumped resistors keep their resistance unless
    ``model.resistor_coefficient`` is given (DESIGN.md "Resistor coupling"): resistor r then has ``R_r / s_r`` with ``s_r = 1 /
    (1 + alpha_r (T_r - T0_r))``, ``T_r`` the mean temperature of its two ends; its stamps are revalued on the device with the
    faces, d_k also covers the resistors' means, the element flows, ``CouplingReport.elements`` and the resistors' heat use
    the resistance the solve used, ``CouplingReport.resistors`` tells it, and the thermal link of a resistor does not move with
    R.  With every coefficient 0 the results have the bits of ``resistor_coefficient=None``.  The loop is Picard, one load case at a
    time, from the copper at ambient:

        round k:  L = L0 + sum_f (s_f - 1) sigma_m K_f     the electrical system revalued on the device, same pattern
                  V_k from the electrical solve, the face powers with sigma_m s_f, theta_k from the thermal solve
                  d_k = max_f |thetabar_k,f - thetabar_k-1,f|;   s from theta_k;   stop when d_k <= model.tolerance

    With every alpha 0 the loop is one round and the results have the bits of ``solve_meshed_thermal``.  With a
    :class:`FilmCurve` in ``model.thermal.film`` (DESIGN.md "Film curves") the same loop serves both couplings: every round
    linearises the film about the current theta before the thermal solve, d_k is the larger of the face means' and the
    vertices' largest change, ``ThermalReport.film`` tells the film's share, and ``total_loss`` equals ``total_heat`` up to
    the last round's linearisation defect; with every alpha 0 the results then have the bits of ``solve_meshed_thermal``
    with the same curves (for equal tolerances).  The Solution holds
    the potentials and power densities of the last electrical solve and the ThermalReport is that of the last thermal
    solve, whose load came from that electrical solve with the same scale: ``total_loss`` equals ``total_heat`` equals the
    power the sources deliver in every round, converged or not.  Cases are converged one after another on one assembly and
    one thermal handle; the envelope is formed from their vertex temperatures by the rule of :func:`envelope_of`.  The
    ``heat_sources`` of ``model.thermal`` put the same watts into every round: they are not scaled by the resistivity.

    :class:`ThermalRunawayError` when the increments grew in three consecutive rounds (a current-driven neck may have no
    steady state); a SolverWarning and ``converged=False`` when ``model.max_rounds`` end the loop first; ValueError for an
    invalid model (:func:`check_electrothermal_model`), invalid cases and a ``partition`` over several GPUs before anything
    reaches the device, and for a face whose 1 + alpha (T - T0) is not finite and positive, found on the device.
    ``timings`` (a dict) receives the host time of each step in seconds and under "rounds" one dict of laps per round."""
    _refuse_partition(partition, "electro-thermal solves")
    checked = check_electrothermal_model(prob, model, filtered_networks)
    single = cases is None
    checked_cases = [{}] if single else check_load_cases(prob, cases)
    solutions, reports, couplings, envelope = _solve_electrothermal(
        prob, meshes, mesh_index_to_layer_index, checked, checked_cases, bool(per_case_fields) or single, filtered_networks,
        disconnected_meshes_by_layer, _Laps(timings))
    if single:
        return solutions[0], reports[0], couplings[0]
    return solutions, reports, couplings, envelope


def solve_electrothermal(prob, model: ElectroThermalModel, mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None,
                         cases=None, per_case_fields=True, partition=None, prune=False):
    """``solve`` with the copper's temperatures and the conductances that follow them (see
    :func:`solve_meshed_electrothermal`): the board is meshed once."""
    _refuse_partition(partition, "electro-thermal solves")
    check_electrothermal_model(prob, model)
    if cases is not None:
        cases = check_load_cases(prob, cases)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_electrothermal(prob, meshes, mesh_index_to_layer_index, model, cases=cases,
                                       per_case_fields=per_case_fields, **pruned)


# --------------------------------------------------------------------------------------------
# transient electro-thermal: the resistivity follows the temperature over time (DESIGN.md "Transient electro-thermal")
# --------------------------------------------------------------------------------------------

@dataclass
class ElectroThermalTransientModel:
    """What steps the electro-thermal problem through time (see :func:`solve_meshed_electrothermal_transient`).

    - ``electrothermal``: the :class:`ElectroThermalModel`; its ``tolerance`` and ``max_rounds`` govern the loop that finds
      the initial state.
    - ``areal_capacity``: as in :class:`TransientModel`.
    - ``initial``: None = the copper starts at ambient; a case index = from that case's converged electro-thermal steady
      state.  The tuple form (several scenarios) is refused."""
    electrothermal: ElectroThermalModel
    areal_capacity: object
    initial: object = None


@dataclass
class CheckedElectroThermalTransientModel:
    """An :class:`ElectroThermalTransientModel` resolved against a Problem (:func:`check_electrothermal_transient_model`)."""
    electrothermal: CheckedElectroThermalModel
    capacity: list             # per layer
    initial: object            # None or an int


@dataclass
class CouplingTrace:
    """How the coupling went, step by step (see :func:`solve_meshed_electrothermal_transient`).  Arrays over time as
    :class:`TransientReport` holds them: entry 0 is the start -- zeros and NaN from ambient, the last round of the initial
    loop otherwise -- and entry n belongs to step n."""
    increments: np.ndarray     # [K]: the largest change of a face mean since the last electrical solve (NaN in off steps)
    scale_min: np.ndarray      # the smallest and ...
    scale_max: np.ndarray      # ... the largest scale the step's electrical solve used (NaN where no electrical solve ran)
    delivered: np.ndarray      # [W]: what the sources deliver by element_flows of the step's solve (0 in off steps)
    iterations: list           # per time: {"electrical": iterations of the electrical solve, "thermal": of the thermal one}
    potentials: dict           # node id -> V over time (NaN where no electrical solve ran)
    stopped: Optional[tuple]   # None, or (time, T, layer index, mesh index within the layer, vertex index, x, y) of the stop
    # the smallest and the largest scale of a resistor in the step's electrical solve (NaN where no electrical solve ran or
    # the networks hold no resistor); None without a resistor_coefficient
    resistor_scale_min: Optional[np.ndarray] = None
    resistor_scale_max: Optional[np.ndarray] = None


_NO_SCENARIOS = ("the transient electro-thermal solve runs one scenario: several in lockstep are not built, because each "
                 "needs its own electrical matrix")


def check_electrothermal_transient_model(prob, model, filtered_networks=None) -> CheckedElectroThermalTransientModel:
    """``model`` resolved against ``prob``, or ValueError -- before anything reaches the device -- for everything
    :func:`check_electrothermal_model` refuses of ``model.electrothermal``, everything :func:`check_transient_model` refuses
    of the capacity, and an ``initial`` in the tuple form.  ``initial`` is checked against the cases by
    :func:`solve_meshed_electrothermal_transient`."""
    if not isinstance(model, ElectroThermalTransientModel):
        raise ValueError("model must be an ElectroThermalTransientModel")
    electrothermal = check_electrothermal_model(prob, model.electrothermal, filtered_networks)
    capacity = check_transient_model(prob, TransientModel(thermal=model.electrothermal.thermal, areal_capacity=model.areal_capacity),
                                     filtered_networks).capacity
    if isinstance(model.initial, (tuple, list)):
        raise ValueError(f"initial: {_NO_SCENARIOS}")
    return CheckedElectroThermalTransientModel(electrothermal=electrothermal, capacity=capacity, initial=model.initial)


def _check_electrothermal_transient_arguments(prob, model, schedule, cases, repeat, probes, voltage_probes, stop_above, keep,
                                              filtered_networks):
    """Every check of :func:`solve_meshed_electrothermal_transient`: (checked model, checked cases, per flattened segment (dt,
    steps, case), the initial case, probes, voltage probes, stop_above as a float or None)."""
    checked = check_electrothermal_transient_model(prob, model, filtered_networks)
    thermal_model = checked.electrothermal.thermal

    def checked_stop_above():
        if stop_above is None:
            return None
        try:
            stop = float(stop_above)
        except (TypeError, ValueError):
            raise ValueError(f"stop_above must be a temperature, not {stop_above!r}") from None
        if not math.isfinite(stop) or not stop > thermal_model.ambient:
            raise ValueError(f"stop_above must be finite and above the ambient temperature of {thermal_model.ambient!r}, "
                             f"not {stop!r}")
        return stop

    checked_cases, flat, initial, probe_nodes, stop = _check_transient_call(
        prob, checked.initial, schedule, cases, repeat, probes, keep, filtered_networks, check_schedule,
        lambda seg, case: (seg.duration / seg.steps, seg.steps, case), scenarios=False, sources=thermal_model.sources,
        extra=checked_stop_above)
    return checked, checked_cases, flat, initial, probe_nodes, check_probes(prob, voltage_probes, filtered_networks), stop


def _delivered_power(element_rows, flows) -> float:
    """What the sources deliver [W]: minus what the rows that are no resistor absorb in ``flows`` (:func:`element_flows`)."""
    terms = []
    for row, flow in zip(element_rows, flows):
        if row[0] != "R":
            terms += [-flow["power"], -flow.get("input_power", 0.0)]
    return math.fsum(terms)


def solve_meshed_electrothermal_transient(prob, meshes, mesh_index_to_layer_index, model: ElectroThermalTransientModel, schedule,
                                          *, cases=None, repeat=1, probes=(), voltage_probes=(), stop_above=None, keep="end",
                                          filtered_networks=None, disconnected_meshes_by_layer=None, partition=None,
                                          timings: Optional[dict] = None):
    """:func:`solve_meshed_thermal_transient` with the loop closed: the sheet conductance of every face follows its
    temperature while the copper heats and cools.  ``([Solution or None] per case, TransientReport, CouplingTrace)``.

    The scheme (DESIGN.md "Transient electro-thermal") is semi-implicit backward Euler, one scenario.  The step from t_n
    while case j is on:

        s_f = 1 / (1 + alpha_m (Tbar_f(theta_n) - T0)),   d = max_f |thetabar_f - the thetabar_f of the last electrical solve|
        L = L0 + sum_f (s_f - 1) sigma_m K_f                   the electrical system revalued on the device
        V of case j on that L, on a fresh plan                 as a round of :func:`solve_meshed_electrothermal`
        b = the face powers with sigma_m s_f, a third to each corner, the resistors' halves, the heat sources of case j
        (A + C/dt) theta_n+1 = (C/dt) theta_n + b              the step of :func:`solve_meshed_thermal_transient`

    With the sources off only the last line runs, without b.  The resistivity is that of the start of the step: the
    nonlinear term lags by one step, which is first order like backward Euler itself and, on a uniformly heated
    current-driven strip, stable exactly where a steady state exists.  Every step balances (stored_n+1 - stored_n) / dt +
    loss_n+1 against the heat of its own electrical solve, which ``TransientReport.total_heat`` and the layers' ``heat``
    now hold step by step; that heat is the power the sources deliver (``CouplingTrace.delivered``) plus the heat sources'.
    Nothing iterates within a step.  Lumped resistors keep their resistance unless ``resistor_coefficient`` of
    ``model.electrothermal`` is given: then s_r follows theta_n like s_f, the step's heat uses ``R_r / s_r``, and
    ``CouplingTrace.resistor_scale_min`` / ``resistor_scale_max`` hold the range of s_r step by step.

    ``model.initial`` None starts at ambient; a case index starts from that case's steady state, found on the same handles
    by the Picard loop of :func:`solve_meshed_electrothermal` (``tolerance``, ``max_rounds`` and :func:`picard_verdict` of
    ``model.electrothermal`` apply; :class:`ThermalRunawayError` and the warning on non-convergence as there).  The
    stepping itself never raises ThermalRunawayError: a neck without a steady state just gets hotter, and ``stop_above`` -- a
    finite temperature above ambient -- ends the run after the first step whose hotspot over all meshes is strictly
    greater: every array ends with that step and ``CouplingTrace.stopped`` names it (the fusing-time question).
    ``voltage_probes``: node ids whose potentials are wanted over time.  ``solutions[j]`` is the Solution of the last step
    that ran case j, None for a case that never ran.  ``cases``, ``schedule``, ``repeat``, ``probes`` and ``keep`` as in
    :func:`solve_meshed_thermal_transient`; ``info["iterations_per_step"]`` counts the thermal solves.

    ValueError, before anything reaches the device, for an invalid model (:func:`check_electrothermal_transient_model`),
    invalid cases, schedule or probes, the tuple forms of ``Segment.case`` and ``initial``, an unknown ``keep``, a
    ``stop_above`` that is not finite or not above ambient, and a ``partition`` over several GPUs; for a face whose
    1 + alpha (T - T0) is not finite and positive, found on the device.  A SolverWarning when a step's electrical or thermal
    solve ends above the tolerance.  ``timings`` (a dict) receives the host time of each stage and under "steps" one dict
    of laps per step: scale, revalue, stage1 and stage2 (the electrical plan and solve), load, thermal_step."""
    _refuse_partition(partition, "transient electro-thermal solves")
    checked, checked_cases, flat, initial, probe_nodes, vprobe_nodes, stop_above = _check_electrothermal_transient_arguments(
        prob, model, schedule, cases, repeat, probes, voltage_probes, stop_above, keep, filtered_networks)
    electro = checked.electrothermal
    thermal_model = electro.thermal
    laps, ambient, n_layers = _Laps(timings), thermal_model.ambient, len(prob.layers)
    board, pairs, substituted, source_power, n_vert, k = _thermal_board(
        prob, meshes, mesh_index_to_layer_index, thermal_model, checked_cases, filtered_networks, disconnected_meshes_by_layer)
    laps.lap("indexing")
    layer_of, n_mesh = board.layer_of, len(board.meshes)
    steps_log = []
    if laps.timings is not None:
        laps.timings["steps"] = steps_log
    nan = float("nan")
    last_step_of = {}                                        # case -> the last step of the schedule that runs it
    for n, case in enumerate(j for _dt, steps, j in flat for _ in range(steps)):
        if case is not None:
            last_step_of[case] = n + 1
    with _coupled_handles(board, pairs, electro, laps, checked.capacity, k) as h:
        thermal, coupled, transient, sources = h.thermal, h.coupled, h.transient, h.sources
        stamps = [stamp_load_cases(board.filtered_networks, board.node_indexer, h.L.shape[0], [case]) for case in checked_cases]
        probe_idx = [board.node_indexer.node_to_global_index[node] for node in probe_nodes]
        vprobe_idx = [board.node_indexer.node_to_global_index[node] for node in vprobe_nodes]

        def electrical(j, step_laps, want_power):
            """Parts 2 to 4 of a step for case ``j`` on the scale the coupling holds: what the step keeps of them."""
            el = _revalued_solve(h, board, pairs, checked_cases[j], stamps[j], thermal_model.element_heat, step_laps)
            if sources is not None:                          # not scaled by the resistivity
                thermal.source_power(source_power[j:j + 1])
            mesh_heat = coupled.transient_load(transient, el.plan, j, el.heat)
            step_laps.lap("load")
            _warn_if_block_stalled(el.res, el.residual_norms, el.cols, el.vals, 1)
            layer_heat = [math.fsum(float(mesh_heat[i]) for i in range(n_mesh) if layer_of[i] == layer_i)
                          for layer_i in range(n_layers)]
            total = math.fsum(layer_heat + [math.fsum(el.heat[2].tolist()) if el.heat is not None else 0.0])
            if sources is not None:
                total = total + math.fsum(source_power[j].tolist())
            followed = el.resistor_state is not None and len(el.resistor_state[0]) > 0
            return types.SimpleNamespace(
                resistor_range=(float(el.resistor_state[0].min()), float(el.resistor_state[0].max())) if followed else (nan, nan),
                case=j, V=np.ascontiguousarray(el.V[:, 0]), residual_norm=el.residual_norms[0], res=el.res,
                power=coupled.power_density(el.plan, h.n_tri) if want_power else None, layer_heat=layer_heat, total_heat=total,
                delivered=_delivered_power(el.case_rows, el.flows), scale_range=coupled.scale_range(),
                potentials=[float(el.V[i, 0]) for i in vprobe_idx])

        # the start: ambient, or the steady electro-thermal state of a case by the Picard loop on these handles
        start_increment, start_iterations, last = 0.0, {"electrical": 0, "thermal": 0}, {"start": None}
        if initial is None:
            last["first"] = transient.start([None], rtol=RTOL, max_iter=MAX_ITER)
        else:
            def one_round(_round):
                start = electrical(initial, _Laps(None), stop_above is not None or initial not in last_step_of)
                first = transient.start([initial], rtol=RTOL, max_iter=MAX_ITER)
                increment = coupled.update_transient(transient, 0)
                start_iterations["electrical"] += int(start.res.iterations)
                start_iterations["thermal"] += int(first.iterations)
                last.update(start=start, first=first)
                return increment

            increments, verdict = _picard(one_round, electro)
            _picard_outcome(verdict, increments, f"The initial state of load case {initial}", board, electro,
                            lambda: transient.report()[0][0])
            start_increment = increments[-1]
        start = last["start"]
        laps.lap("transient_start")
        head = _transient_head(transient, last["first"], probe_idx)
        runs, snapshots, stepped, last_of_case, stopped_at, worst = [], [], [], {}, None, head["worst"]
        if start is not None:
            last_of_case[initial] = start
        t, times = 0.0, [0.0]
        for at, (dt, steps, case) in enumerate(flat):
            for _ in range(steps):
                lap = {}
                step_laps = _Laps(lap)
                el, d = None, nan
                if case is not None:
                    d = coupled.update_transient(transient, 0)
                    step_laps.lap("scale")
                    el = electrical(case, step_laps, stop_above is not None or last_step_of[case] == len(times))
                    last_of_case[case] = el
                    step_laps.lap()
                out = transient.run(dt, 1, [case], probe_idx, rtol=RTOL, max_iter=MAX_ITER)
                step_laps.lap("thermal_step")
                steps_log.append(dict(lap, step=len(times), case=case))
                runs.append(out)
                stepped.append((el, d))
                worst = _worse(worst, out["result"])
                t = t + dt
                times.append(t)
                if stop_above is not None and any(out["vertex"][0, 0, i] >= 0 and out["max"][0, 0, i] + ambient > stop_above
                                                  for i in range(n_mesh)):
                    stopped_at = len(times) - 1
                    break
            if keep == "segments" or (keep == "end" and (at == len(flat) - 1 or stopped_at is not None)):
                snapshots.append((t, transient.state()))
            if stopped_at is not None:
                break
        end = _transient_end(transient, n_vert, laps)
    laps.lap()
    led = [start] + [el for el, _d in stepped]             # the electrical solve that led to every time, None without
    layer_heat = [[0.0 if el is None else el.layer_heat[layer_i] for el in led] for layer_i in range(n_layers)]
    total_heat = [0.0 if el is None else el.total_heat for el in led]
    (report,), info = _transient_reports(board, ambient, times, head, runs, [(layer_heat, total_heat)], probe_nodes, end, snapshots,
                                         worst)
    solutions = []
    for j in range(k):
        el = last_of_case.get(j)
        solutions.append(None if el is None else _column_solution(board, substituted[j][0], el.V, el.residual_norm, el.res, el.power,
                                                                  f"Load case {j}: " if k > 1 else ""))
    stopped = None
    if stopped_at is not None:
        spots = [(report.hotspots[layer_i][-1], layer_i) for layer_i in range(n_layers) if report.hotspots[layer_i][-1] is not None]
        spot, layer_i = max(spots, key=lambda entry: (entry[0][0], -entry[1]))      # the lowest layer of the largest temperature
        stopped = (float(times[-1]), spot[0], layer_i, *spot[1:])
    thermal_its = [int(head["result"].iterations)] + [int(i) for i in info["iterations_per_step"]]
    trace = CouplingTrace(
        increments=np.array([start_increment] + [d for _el, d in stepped], dtype=DTYPE),
        scale_min=np.array([nan if el is None else el.scale_range[0] for el in led], dtype=DTYPE),
        scale_max=np.array([nan if el is None else el.scale_range[1] for el in led], dtype=DTYPE),
        delivered=np.array([0.0 if el is None else el.delivered for el in led], dtype=DTYPE),
        iterations=[dict(start_iterations) if n == 0 and start is not None else
                    {"electrical": 0 if el is None else int(el.res.iterations), "thermal": thermal_its[n]}
                    for n, el in enumerate(led)],
        potentials={node: np.array([nan if el is None else el.potentials[p] for el in led], dtype=DTYPE)
                    for p, node in enumerate(vprobe_nodes)},
        stopped=stopped)
    if electro.resistor_alpha is not None:
        trace.resistor_scale_min = np.array([nan if el is None else el.resistor_range[0] for el in led], dtype=DTYPE)
        trace.resistor_scale_max = np.array([nan if el is None else el.resistor_range[1] for el in led], dtype=DTYPE)
    laps.lap("solutions")
    return solutions, report, trace


def solve_electrothermal_transient(prob, model: ElectroThermalTransientModel, schedule,
                                   mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None, cases=None, repeat=1,
                                   probes=(), voltage_probes=(), stop_above=None, keep="end", partition=None, prune=False):
    """``solve`` with the copper's temperatures over a schedule and the conductances that follow them (see
    :func:`solve_meshed_electrothermal_transient`): the board is meshed once."""
    _refuse_partition(partition, "transient electro-thermal solves")
    _check_electrothermal_transient_arguments(prob, model, schedule, cases, repeat, probes, voltage_probes, stop_above, keep, None)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_electrothermal_transient(prob, meshes, mesh_index_to_layer_index, model, schedule, cases=cases,
                                                 repeat=repeat, probes=probes, voltage_probes=voltage_probes,
                                                 stop_above=stop_above, keep=keep, **pruned)


# --------------------------------------------------------------------------------------------
# element cases: what-if cases that change resistors as well as sources (DESIGN.md "Element cases")
# --------------------------------------------------------------------------------------------

# sigma_c, the smallest singular value of a case's G = I + C D_S^T Z_S, is 1 for a case without resistors, and 1 / sigma_c
# is how much the case amplifies the error of the block's columns (held to 1e-8): at or below the first no digit is left
# (the change disconnects driven copper or leaves a node floating), below the second the case is reported.
ELEMENT_CASE_SINGULAR_AT = 1e-8
ELEMENT_CASE_WARN_BELOW = 1e-3


@dataclass
class ElementCaseReport:
    """What :func:`solve_meshed_element_cases` reports next to the Solutions."""
    conditioning: np.ndarray          # (n_cases,) sigma_c: smallest singular value of the case's G (1.0 without resistors)
    columns: int                      # columns of the one block solve behind all cases
    drops: Optional[np.ndarray]       # (n_cases, n_objectives) V(p) - V(n) per case [V]; None without objectives


def check_element_cases(prob, cases) -> list:
    """The element cases of ``prob`` as a list of ``{element: float}``, or ValueError.

    ``cases`` is a non-empty sequence of mappings ``{element: value}``.  A source key is taken exactly as
    :func:`check_load_cases` takes it (its ground rule included); a ``Resistor`` of ``prob.networks`` takes a resistance
    > 0, or ``math.inf`` for the resistor left open.  NaN, a resistance <= 0, an element that is not in the Problem and
    any other key -- a regulator's gain, a layer's conductance: they are not resistor stamps -- are refused."""
    if isinstance(cases, (Mapping, str, bytes)):
        raise ValueError("cases must be a sequence of mappings {element: value}, one per element case")
    cases = list(cases)
    if not cases:
        raise ValueError("no element cases: give at least one mapping {element: value} ({} is the Problem as given)")
    elements = {element for network in prob.networks for element in network.elements}
    source_parts, resistor_parts = [], []
    for j, case in enumerate(cases):
        if not isinstance(case, Mapping):
            raise ValueError(f"element case {j} is not a mapping {{element: value}}")
        sources, resistors = {}, {}
        for element, value in case.items():
            kind = element_kind(element)
            if kind in CASE_FIELDS:
                sources[element] = value
                continue
            if kind != "Resistor":
                raise ValueError(f"element case {j}: a {type(element).__name__} key cannot vary between element cases -- only "
                                 "the value of a source and the resistance of a Resistor can; a regulator's gain and a layer's "
                                 "conductance are not resistor stamps")
            if element not in elements:
                raise ValueError(f"element case {j}: the Resistor is not an element of the Problem's networks")
            try:
                x = float(value)
            except (TypeError, ValueError):
                raise ValueError(f"element case {j}: the resistance of a Resistor must be a number, not {value!r}") from None
            if not x > 0:
                raise ValueError(f"element case {j}: the resistance of a Resistor must be > 0 (math.inf leaves it open), "
                                 f"not {value!r}")
            resistors[element] = x
        source_parts.append(sources)
        resistor_parts.append(resistors)
    source_parts = check_load_cases(prob, source_parts)
    return [{**sources, **resistors} for sources, resistors in zip(source_parts, resistor_parts)]


def substitute_element_case(prob, case: dict):
    """``prob`` with one checked element case applied: sources and resistors replaced (``dataclasses.replace``), a resistor
    at ``math.inf`` removed from its network; the networks rebuilt around the same NodeIDs and connections, the layers
    shared.  Returns the Problem."""
    if not case:
        return prob
    networks = []
    for network in prob.networks:
        if not any(element in case for element in network.elements):
            networks.append(network)
            continue
        elements = []
        for e in network.elements:
            if e not in case:
                elements.append(e)
            elif element_kind(e) == "Resistor":
                if math.isfinite(case[e]):
                    elements.append(dataclasses.replace(e, resistance=case[e]))
            else:
                elements.append(dataclasses.replace(e, **{CASE_FIELDS[element_kind(e)]: case[e]}))
        networks.append(dataclasses.replace(network, elements=elements))
    return dataclasses.replace(prob, networks=networks)


def open_circuit_cases(prob, elements=None) -> list:
    """The N-1 list: ``[{R: math.inf}]`` for every Resistor of ``prob.networks`` in stamping order, or for those among
    ``elements`` (ValueError for one that is not a Resistor of the Problem)."""
    resistors = [e for network in prob.networks for e in network.elements if element_kind(e) == "Resistor"]
    if elements is not None:
        wanted = list(elements)
        for e in wanted:
            if element_kind(e) != "Resistor" or e not in resistors:
                raise ValueError("open_circuit_cases: every element must be a Resistor of the Problem's networks")
        resistors = [e for e in resistors if e in wanted]
    return [{e: math.inf} for e in resistors]


def element_case_columns(pairs, cases: list):
    """How the checked element ``cases`` share one block, from the solved networks' ``pairs`` (:func:`global_elements`):

    - ``source_cases``: the distinct source settings among the cases in first-appearance order (``{}`` is the Problem's),
      one block column each; when no case names a resistor, one per case as :func:`stamp_load_cases` takes them;
    - ``case_source[c]``: the column of case c's setting;
    - ``resistor_rows``: ``(a, b, g)`` on global unknowns of every resistor row that a case changes, in stamping order, one
      column ``d = e_a - e_b`` each after the source columns; a resistor with both terminals on one unknown gets none;
    - ``case_changes[c]``: ``(m, g, g')`` per changed resistor column m of case c, ascending (g' = 0: open)."""
    named = {e for case in cases for e in case if element_kind(e) == "Resistor"}
    source_cases, case_source, seen = [], [], {}
    for case in cases:
        sources = {e: v for e, v in case.items() if element_kind(e) != "Resistor"}
        key = frozenset(sources.items()) if named else len(source_cases)
        if key not in seen:
            seen[key] = len(source_cases)
            source_cases.append(sources)
        case_source.append(seen[key])
    resistor_rows, column_of = [], {}
    for i, (element, row) in enumerate(pairs):
        if row[0] == "R" and element in named and row[1] != row[2]:
            column_of[i] = len(resistor_rows)
            resistor_rows.append((int(row[1]), int(row[2]), 1.0 / row[3]))
    case_changes = []
    for case in cases:
        changes = []
        for i, m in column_of.items():
            element = pairs[i][0]
            if element in case:
                g, g_new = resistor_rows[m][2], (1.0 / case[element] if math.isfinite(case[element]) else 0.0)
                if g_new != g:
                    changes.append((m, g, g_new))
        case_changes.append(changes)
    return source_cases, case_source, resistor_rows, case_changes


def stamp_element_case_block(filtered_networks, node_indexer: NodeIndexer, n_unknowns: int, source_cases: list,
                             resistor_rows: list):
    """COO triples (rows, cols, vals) of the block [R_src | D] of element cases: the columns of :func:`stamp_load_cases` for
    ``source_cases``, then ``d = e_a - e_b`` per entry of ``resistor_rows`` (the unit-current column of
    :func:`stamp_sensitivity_block`)."""
    rows, cols, vals = stamp_load_cases(filtered_networks, node_indexer, n_unknowns, source_cases)
    rows, cols, vals = rows.tolist(), cols.tolist(), vals.tolist()
    for m, (a, b, _g) in enumerate(resistor_rows):
        rows.extend((int(a), int(b)))
        cols.extend((len(source_cases) + m, len(source_cases) + m))
        vals.extend((1.0, -1.0))
    return np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int32), np.asarray(vals, dtype=DTYPE)


def element_case_weights(DtV: np.ndarray, n_src: int, case_source: list, case_changes: list):
    """The weights of every element case on the columns of the solved block V = M^-1 [R_src | D], as CSR rows
    ``(w_ptr (n_cases + 1,), w_col, w_val)``, and ``sigma (n_cases,)``.  ``DtV`` (n_resistor_columns, n_cols) is D^T V: row m
    is V[a_m] - V[b_m], all that is read of V.

    A set S of changed resistors makes the system M + D_S C D_S^T with C = diag(g - g').  By Woodbury, with Z_S the solved
    ``d`` columns and s the case's source column, G = I + C (D_S^T Z_S), w = -G^-1 C (D_S^T V[:, s]) and
    x' = V[:, s] + Z_S w: only forward solves with M, so a regulator's unsymmetric M is no exception.  A row lists the source
    column with coefficient exactly 1.0 and then the non-zero w, columns ascending.  sigma_c is the smallest singular value
    of G: SingularSystemError naming the case at or below ELEMENT_CASE_SINGULAR_AT, a SolverWarning naming the case and
    1 / sigma_c below ELEMENT_CASE_WARN_BELOW."""
    DtV = np.asarray(DtV, dtype=DTYPE)
    w_ptr, w_col, w_val, sigma = [0], [], [], np.ones(len(case_source), dtype=DTYPE)
    for c, (s, changes) in enumerate(zip(case_source, case_changes)):
        w_col.append(int(s))
        w_val.append(1.0)
        if changes:
            S = np.array([m for m, _, _ in changes], dtype=np.int64)
            C = np.array([g - g_new for _, g, g_new in changes], dtype=DTYPE)
            G = np.eye(len(S)) + C[:, None] * DtV[S][:, int(n_src) + S]
            sigma[c] = np.linalg.svd(G, compute_uv=False).min()
            if not sigma[c] > ELEMENT_CASE_SINGULAR_AT:
                raise SingularSystemError(f"element case {c}: the changed system is singular to working precision (smallest "
                                          f"singular value of its {len(S)} x {len(S)} update {sigma[c]:.1e}): the change "
                                          "disconnects driven copper or leaves a node floating")
            if sigma[c] < ELEMENT_CASE_WARN_BELOW:
                warnings.warn(f"element case {c} is ill-conditioned: it amplifies the error of the block's columns "
                              f"{1.0 / sigma[c]:.1e} times", SolverWarning)
            w = -np.linalg.solve(G, C * DtV[S, int(s)])
            for m, x in zip(S.tolist(), w.tolist()):
                if x != 0.0:
                    w_col.append(int(n_src) + m)
                    w_val.append(x)
        w_ptr.append(len(w_col))
    return (np.asarray(w_ptr, dtype=np.int64), np.asarray(w_col, dtype=np.int32), np.asarray(w_val, dtype=DTYPE), sigma)


def _case_weight_matrix(w_ptr, w_col, w_val, n_cols: int) -> sp.csr_matrix:
    return sp.csr_matrix((w_val, w_col, w_ptr), shape=(len(w_ptr) - 1, int(n_cols)))


def element_case_residual_bounds(w_ptr, w_col, w_val, residual_norms: np.ndarray) -> np.ndarray:
    """``sum_m |w_cm| residual_norms[m]`` per case: with rho_m = M V[:, m] - R[:, m], the changed system's residual of case c
    is exactly sum_m w_cm rho_m (the defining equation of w cancels the rest), so this bounds its norm."""
    W = _case_weight_matrix(w_ptr, w_col, np.abs(w_val), len(residual_norms))
    return np.asarray(W @ np.asarray(residual_norms, dtype=DTYPE)).reshape(-1)


def solve_meshed_element_cases(prob, meshes, mesh_index_to_layer_index, cases, *, objectives=None, fields=True,
                               filtered_networks=None, disconnected_meshes_by_layer=None, partition=None,
                               timings: Optional[dict] = None):
    """``solve_meshed`` for what-if cases that change resistors as well as sources -- a via cracked open, a tolerance corner of
    a sense resistor, a second via -- from one block solve: ([Solution per case], :class:`ElementCaseReport`).

    ``cases`` as :func:`check_element_cases` takes them.  A resistor between unknowns a and b stamps -g d d^T into the system
    M, d = e_a - e_b, so a set of changed resistors is a low-rank update of M and every case follows from V = M^-1 [R_src | D]
    by Woodbury (:func:`element_case_columns`, :func:`element_case_weights`): one indexing, assembly, reduction and
    multigrid setup for all cases.  The small systems are solved on the host from the rows of V at the resistors' unknowns;
    the device then turns V into the cases' potentials (``KktPlan.combine_block``) without V crossing again, and
    ``power_density_block`` runs on the result.  V (N, columns) and the cases' potentials (N, n_cases) are on the device
    together, ``(columns + n_cases) * N * 8`` bytes; nothing is chunked.

    Solution c carries the Problem with case c substituted (:func:`substitute_element_case`), its own potentials and power
    densities, and a SolverInfo whose ``ground_node_current`` is its own (warned about as usual, opened by ``"Case c: "``)
    and whose ``residual_norm`` is a BOUND on the residual of the changed system, sum_m |w_cm| ||M V[:, m] - R[:, m]||
    (:func:`element_case_residual_bounds`); ``iterations``, ``rel_residual`` and ``solve_seconds`` are the block's.  The
    report holds each case's conditioning sigma_c (SingularSystemError at or below 1e-8, a SolverWarning below 1e-3), the
    number of block columns and, with ``objectives`` (pairs (p, n) as :func:`check_objectives` takes them), ``drops[c, j]``
    = V(p_j) - V(n_j) in case c, formed on the host from the rows of V at those nodes.

    ``fields=False`` skips the combination and the power densities: ``solutions`` is None and only the report comes back
    (the N-1 sweep over hundreds of vias).  When no case names a resistor, with ``fields`` and without ``objectives``, the
    call is ``solve_meshed_load_cases``.  ValueError, before anything reaches the device, for invalid cases or objectives
    and for a ``partition`` over several GPUs.  ``timings`` (a dict) receives the host time of each step in seconds and
    ``combine_calls``, how often ``combine_block`` ran."""
    _refuse_partition(partition, "element cases")
    cases = check_element_cases(prob, cases)
    if objectives is not None:
        objectives = check_objectives(prob, objectives, filtered_networks)
    n_cases = len(cases)
    if fields and objectives is None and not any(element_kind(e) == "Resistor" for case in cases for e in case):
        solutions = solve_meshed_load_cases(prob, meshes, mesh_index_to_layer_index, cases, filtered_networks=filtered_networks,
                                            disconnected_meshes_by_layer=disconnected_meshes_by_layer, timings=timings)
        if timings is not None:
            timings["combine_calls"] = 0
        return solutions, ElementCaseReport(conditioning=np.ones(n_cases, dtype=DTYPE), columns=n_cases, drops=None)
    laps = _Laps(timings)
    board = index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer)
    pairs = global_elements(board.filtered_networks, board.node_indexer)
    source_cases, case_source, resistor_rows, case_changes = element_case_columns(pairs, cases)
    n_src = len(source_cases)
    n_cols = n_src + len(resistor_rows)
    idx = board.node_indexer.node_to_global_index
    laps.lap("indexing")
    combine_calls = 0
    with board.assembled() as (L, _):
        rows, cols, vals = stamp_element_case_block(board.filtered_networks, board.node_indexer, L.shape[0], source_cases,
                                                    resistor_rows)
        laps.lap("assembly")
        log.info(f"Solving {n_cases} element case(s) from one block of {n_src} source and {len(resistor_rows)} resistor column(s)")
        plan, V, residual_norms, res, n_tri, _n_mesh = _solve_block_on_device(L, rows, cols, vals, n_cols, n_cases, laps)
        a = np.array([r[0] for r in resistor_rows], dtype=np.int64)
        b = np.array([r[1] for r in resistor_rows], dtype=np.int64)
        w_ptr, w_col, w_val, sigma = element_case_weights(V[a] - V[b], n_src, case_source, case_changes)
        laps.lap("weights")
        Vc = power = None
        if fields:
            Vc = plan.combine_block(n_cols, w_ptr, w_col, w_val)
            combine_calls += 1
            laps.lap("combine")
            power = plan.power_density_block(n_cases, n_tri) if n_tri else None
            laps.lap("power_density")
    laps.lap()
    if timings is not None:
        timings["combine_calls"] = combine_calls
    _warn_if_block_stalled(res, residual_norms, cols, vals, n_cols)
    drops = None
    if objectives is not None:
        p = np.array([idx[p] for p, _ in objectives], dtype=np.int64)
        n = np.array([idx[n] for _, n in objectives], dtype=np.int64)
        drops = np.asarray(_case_weight_matrix(w_ptr, w_col, w_val, n_cols) @ (V[p] - V[n]).T)
    report = ElementCaseReport(conditioning=sigma, columns=n_cols, drops=drops)
    if not fields:
        laps.lap("solutions")
        return None, report
    log.info("Producing the solution objects")
    bounds = element_case_residual_bounds(w_ptr, w_col, w_val, residual_norms)
    solutions = [_column_solution(board, substitute_element_case(prob, case), np.ascontiguousarray(Vc[:, c]), bounds[c], res,
                                  None if power is None else power[c], f"Case {c}: ") for c, case in enumerate(cases)]
    laps.lap("solutions")
    return solutions, report


def solve_element_cases(prob, cases, mesher_config: Optional[mesh.Mesher.Config] = None, *, mesher=None, objectives=None,
                        fields=True, partition=None, prune=False):
    """``solve`` for element cases (see :func:`solve_meshed_element_cases`): the board is meshed once."""
    _refuse_partition(partition, "element cases")
    cases = check_element_cases(prob, cases)
    if objectives is not None:
        objectives = check_objectives(prob, objectives)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_element_cases(prob, meshes, mesh_index_to_layer_index, cases, objectives=objectives, fields=fields,
                                      **pruned)


# --------------------------------------------------------------------------------------------
# error estimate: how far the discrete answer is from the board, per face
# --------------------------------------------------------------------------------------------


@dataclass
class ErrorReport:
    """The estimated discretisation error of a solved Problem (see :func:`solve_meshed_error`)."""
    recovered: list       # per layer, per mesh of LayerSolution.meshes: (n_vert, 2) J* = -sigma G, the recovered J [A/mm]
    indicators: list      # per layer, per mesh: TwoForm of eta_f [sqrt(W)]
    worst: list           # per layer: (max eta, mesh index within the layer, face index, centroid x, y), None without faces
    layers: list          # per layer: (sum eta_f^2, sum sigma A_f |g_f|^2) [W]
    power_error: float    # sum of eta_f^2 over all faces [W]
    estimate: float       # sqrt(power_error / (power + power_error)): the estimated relative error in the energy norm
    ratios: Optional[list] = None     # with a tolerance: per layer, per mesh (n_faces,) xi_f = eta_f / e_bar; above 1: refine
    sizes: Optional[list] = None      # with a tolerance: per layer, per mesh (n_faces,) suggested size h_f / xi_f [mm]
    tolerance: Optional[float] = None


def check_tolerance(tolerance) -> Optional[float]:
    """``tolerance`` as a float, None for None, or ValueError: a finite number strictly between 0 and 1 (a relative error
    in the energy norm); no bool and no string."""
    if tolerance is None:
        return None
    if isinstance(tolerance, (bool, np.bool_, str, bytes)):
        raise ValueError("tolerance must be a number in (0, 1)")
    try:
        value = float(tolerance)
    except (TypeError, ValueError):
        raise ValueError("tolerance must be a number in (0, 1)") from None
    if not (math.isfinite(value) and 0.0 < value < 1.0):
        raise ValueError(f"tolerance must be a finite number in (0, 1), not {tolerance!r}")
    return value


def error_estimate_of(mesh_error, mesh_power) -> tuple:
    """(power_error, estimate) from the per-mesh sums E_m and P_m of the connected meshes: power_error = sum E_m and
    estimate = sqrt(power_error / (sum P_m + power_error)), 0.0 when the denominator is 0."""
    power_error = float(np.sum(np.asarray(mesh_error, dtype=DTYPE)))
    total = float(np.sum(np.asarray(mesh_power, dtype=DTYPE))) + power_error
    return power_error, (math.sqrt(power_error / total) if total > 0.0 else 0.0)


def face_sizes(points, triangles) -> np.ndarray:
    """h_f = sqrt(4 A_f / sqrt(3)) of every face: the edge of the equilateral triangle of the face's area, with A_f as the
    device forms it (corners (tri[2], tri[0], tri[1]))."""
    p, t = np.asarray(points, dtype=DTYPE).reshape(-1, 2), np.asarray(triangles).reshape(-1, 3)
    a, b, c = p[t[:, 2]], p[t[:, 0]], p[t[:, 1]]
    area = np.abs((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])) / 2
    return np.sqrt(4 * area / math.sqrt(3.0))


def refinement_ratios(eta, h, total_power: float, n_faces: int, tolerance: float) -> tuple:
    """(xi_f, suggested size) of the faces with indicators ``eta`` and sizes ``h`` (:func:`face_sizes`): the permissible
    error per face is e_bar = tolerance sqrt(total_power / n_faces) with total_power = sum P_m + power_error and n_faces
    the faces of all connected meshes; xi_f = eta_f / e_bar and the size h_f / xi_f (linear elements: the error falls
    with h at rate 1), inf where xi_f = 0.  A board without power (e_bar = 0) has xi = 0 everywhere."""
    eta, h = np.asarray(eta, dtype=DTYPE), np.asarray(h, dtype=DTYPE)
    e_bar = tolerance * math.sqrt(total_power / n_faces) if n_faces > 0 and total_power > 0.0 else 0.0
    xi = eta / e_bar if e_bar > 0.0 else np.zeros_like(eta)
    sizes = np.full(eta.shape, np.inf, dtype=DTYPE)
    np.divide(h, xi, out=sizes, where=xi > 0)
    return xi, sizes


def _error_report(prob, board, n_tri: int, estimate_arrays, tolerance) -> ErrorReport:
    """The ErrorReport of ``KktPlan.error_estimate``'s six arrays on the indexed ``board`` (all None on a board without faces)."""
    G, eta, mesh_error, mesh_power, mesh_max, mesh_face = estimate_arrays
    power_error, estimate = error_estimate_of(mesh_error, mesh_power) if eta is not None else (0.0, 0.0)
    total_power = (float(np.sum(mesh_power)) + power_error) if eta is not None else 0.0
    voff = board.vindex.offsets
    recovered, indicators, worst, layer_sums = [], [], [], []
    ratios, sizes = ([], []) if tolerance is not None else (None, None)
    for layer_i, layer in enumerate(prob.layers):
        vecs, forms, xis, hs, E, P, best = [], [], [], [], 0.0, 0.0, None
        for mesh_i, msh, lo, hi in board.layer_meshes(layer_i):
            tf = mesh.TwoForm(msh)
            if eta is not None:
                vecs.append(-layer.conductance * G[voff[mesh_i]:voff[mesh_i + 1]])
                tf.values = eta[lo:hi]                    # views of this call's own result array: no copies
                E += float(mesh_error[mesh_i])
                P += float(mesh_power[mesh_i])
                # meshes come in global face order: a later mesh wins only with a strictly larger eta
                if mesh_face[mesh_i] >= 0 and (best is None or mesh_max[mesh_i] > best[0]):
                    face = int(mesh_face[mesh_i] - lo)
                    cx, cy = msh.points[msh.triangles[face]].mean(axis=0)
                    best = (float(mesh_max[mesh_i]), len(forms), face, float(cx), float(cy))
            else:
                vecs.append(np.zeros((len(msh.points), 2), dtype=DTYPE))
            if tolerance is not None:
                xi, size = refinement_ratios(tf.values, face_sizes(msh.points, msh.triangles), total_power, n_tri, tolerance)
                xis.append(xi)
                hs.append(size)
            forms.append(tf)
        recovered.append(vecs)
        indicators.append(forms)
        worst.append(best)
        layer_sums.append((E, P))
        if tolerance is not None:
            ratios.append(xis)
            sizes.append(hs)
    return ErrorReport(recovered=recovered, indicators=indicators, worst=worst, layers=layer_sums, power_error=power_error,
                       estimate=estimate, ratios=ratios, sizes=sizes, tolerance=tolerance)


def solve_meshed_error(prob, meshes, mesh_index_to_layer_index, *, tolerance=None, filtered_networks=None,
                       disconnected_meshes_by_layer=None, partition=None, timings: Optional[dict] = None):
    """``solve_meshed`` together with an estimate of how far its answer is from the board: (Solution, ErrorReport).

    A gradient-recovery (Zienkiewicz-Zhu) estimator on the solved potentials.  Per connected mesh with sheet conductance
    sigma, with g_f the face gradient of the power density and A_f the face's area:

    - ``recovered``: J* = -sigma G at every vertex, G_v = (sum A_f g_f) / (sum A_f) over the faces incident to v, added in
      ascending face order; 0 for a vertex without faces.  Boundary vertices get no special treatment, and nothing is
      averaged across meshes or layers;
    - ``indicators``: eta_f = sqrt(sigma (A_f / 3) (|m_12|^2 + |m_23|^2 + |m_31|^2)) with d_c = G_(corner c) - g_f and
      m_ab = (d_a + d_b) / 2: sigma times the exact integral over the face of |G_h - g_f|^2 for the piecewise-linear G_h;
      eta_f^2 is in watts;
    - ``worst``: per layer the largest eta_f (the lowest global face on a tie), its mesh within the layer, its face and the
      face's centroid;
    - ``layers``: per layer (E, P) = (sum eta_f^2, sum sigma A_f |g_f|^2).  P is the gradient form of the power, not the
      |cot|/2 weights' form of ``CurrentReport.layers``: the estimator measures the distance between two gradients;
    - ``power_error`` = sum E and ``estimate`` = sqrt(power_error / (sum P + power_error)), the estimated relative error in
      the energy norm (0.0 for a board without power);
    - with a ``tolerance`` (relative, in (0, 1)): ``ratios`` xi_f = eta_f / e_bar with the permissible error per face
      e_bar = tolerance sqrt((sum P + power_error) / n_faces) (above 1: refine here), and ``sizes`` h_f / xi_f with
      h_f = sqrt(4 A_f / sqrt(3)), the edge of the equilateral triangle of the face's area (inf where xi_f = 0).  How a
      mesher's own size measure (``Mesher.Config.maximum_size``, a circumradius bound, ...) maps onto h_f is the
      integrator's business.

    Disconnected meshes carry no current: they are not among ``LayerSolution.meshes``, have no entries here and do not
    count in n_faces.  What the estimator does not see: connections snap to single vertices, where the exact solution is
    logarithmically singular, so the faces around terminals stay flagged however fine the mesh; and the consistency error
    of the assembly's |cot| weights on obtuse faces is not a gradient jump and is not measured.

    One call is the load-case block path with one column; the estimator's kernels run on the V the device holds, through
    vertex -> faces lists built once per plan, with every sum in a fixed order: two calls give the same bits.  The Solution
    is that of ``prob``, with the bits ``solve_meshed_currents`` gives it; its power densities come from
    ``padne_kkt_power_density_block`` (there: from the sensitivity kernel, which writes the same bits).  A degenerate face
    (zero area) has no finite gradient: its three vertices recover NaN, as its power density is NaN.  ValueError, before anything reaches the device, for
    an invalid tolerance (:func:`check_tolerance`) and for a ``partition`` over several GPUs.  ``timings`` (a dict)
    receives the host time of each step in seconds; ``"error"`` is the estimator's."""
    _refuse_partition(partition, "error estimates")
    tolerance = check_tolerance(tolerance)
    laps = _Laps(timings)
    board = index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer)
    laps.lap("indexing")
    with board.assembled() as (L, _):
        rows, cols, vals = stamp_load_cases(board.filtered_networks, board.node_indexer, L.shape[0], [{}])
        laps.lap("assembly")
        log.info("Solving the Problem and estimating its error")
        plan, V, residual_norms, res, n_tri, n_mesh = _solve_block_on_device(L, rows, cols, vals, 1, 1, laps)
        power = G = eta = mesh_error = mesh_power = mesh_max = mesh_face = None
        if n_tri:
            power = plan.power_density_block(1, n_tri)[0]
            laps.lap("power")
            G, eta, mesh_error, mesh_power, mesh_max, mesh_face = plan.error_estimate(1, n_tri, len(board.vindex), n_mesh)
        laps.lap("error")
    log.info("Producing the solution and the error report")
    _warn_if_block_stalled(res, residual_norms, cols, vals, 1)
    solution = _column_solution(board, prob, np.ascontiguousarray(V[:, 0]), residual_norms[0], res, power)
    report = _error_report(prob, board, n_tri, (G, eta, mesh_error, mesh_power, mesh_max, mesh_face), tolerance)
    laps.lap("solutions")
    return solution, report


def solve_error(prob, mesher_config: Optional[mesh.Mesher.Config] = None, *, tolerance=None, mesher=None, partition=None,
                prune=False):
    """``solve`` with the error estimate of :func:`solve_meshed_error`: the board is meshed once.  Returns
    (Solution, ErrorReport)."""
    _refuse_partition(partition, "error estimates")
    tolerance = check_tolerance(tolerance)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_error(prob, meshes, mesh_index_to_layer_index, tolerance=tolerance, **pruned)


# --------------------------------------------------------------------------------------------
# refinement: act on the error estimate
# --------------------------------------------------------------------------------------------


@dataclass
class Refinement:
    """One refinement round of a list of meshes (see :func:`refine_meshes`)."""
    meshes: list             # the refined meshes, mesh.Mesh: old vertices first (same index, same coordinates), then the new
    parents: list            # per mesh (n_faces,) int32: the face of the input mesh every face came from
    midpoint_ends: list      # per mesh (n_new, 2) int32: the (lo, hi) ends of the edge every new vertex halves
    edges: int = 0           # edges of all meshes
    marked_by_flags: int = 0     # edges of the flagged faces
    marked: int = 0          # edges halved: those, and what the conforming closure added
    sweeps: int = 0          # closure sweeps the device queued


def check_refine_flags(meshes, flags) -> list:
    """``flags`` as one contiguous boolean array per mesh, or ValueError: a list of the meshes' length, each entry a boolean
    array with one entry per face."""
    try:
        flags = list(flags)
    except TypeError:
        raise ValueError("flags must have one array per mesh: a list of boolean arrays") from None
    if len(flags) != len(meshes):
        raise ValueError(f"flags must have one array per mesh: {len(flags)} arrays for {len(meshes)} meshes")
    out = []
    for i, (msh, f) in enumerate(zip(meshes, flags)):
        f = np.asarray(f)
        if f.dtype != np.bool_:
            raise ValueError(f"the flags of mesh {i} must be a boolean array, not {f.dtype}")
        if f.ndim != 1 or f.shape[0] != len(msh.triangles):
            raise ValueError(f"the flags of mesh {i} must have one entry per face: shape {f.shape} for {len(msh.triangles)} faces")
        out.append(np.ascontiguousarray(f))
    return out


def refine_meshes(meshes, flags) -> Refinement:
    """Conforming refined meshes from one flag per face: 4-triangle longest-edge refinement with conforming closure
    ("Refinement"), on the device, all meshes in one batch.

    A flagged face is cut into four through the midpoints of its edges, its longest edge first; a face that shares a
    halved edge is cut into two or three, again longest edge first, so that no vertex is left hanging on an edge -- which
    may halve further edges (the closure).  The smallest angle of a descendant is at least half that of its ancestor.
    Old vertices keep their index and coordinates (a terminal that sat on a vertex still does), new vertices follow them
    in ascending edge number, children lie in the order of their parents and keep the parents' winding.  Edges stay
    straight: a new vertex on a curved outline is not moved onto it, the copper's area is unchanged.  A mesh without
    faces passes through.  Two calls give the same bits.

    ``meshes``: mesh.Mesh objects (or the reference's); ``flags``: one boolean array per mesh, one entry per face.
    ValueError, before anything reaches the device, for a flags list of the wrong length, an array of the wrong size or
    one that is not boolean; from the device for a non-manifold mesh and a triangle index out of range."""
    meshes = [m if isinstance(m, mesh.Mesh) else mesh.Mesh.from_reference(m) for m in meshes]
    flags = check_refine_flags(meshes, flags)
    if sum(len(m.triangles) for m in meshes) == 0:
        return Refinement([mesh.Mesh(m.points.copy(), m.triangles.copy()) for m in meshes],
                          [np.zeros(0, dtype=np.int32) for _ in meshes], [np.zeros((0, 2), dtype=np.int32) for _ in meshes])
    xy, tri = _flatten_points_triangles(meshes)
    voff, toff = _offsets([len(m.points) for m in meshes]), _offsets([len(m.triangles) for m in meshes])
    xy_out, tri_out, parent, ends, nv, nt, counts = _hip.refine(get_context(), xy, tri, voff, toff,
                                                                 np.concatenate(flags).astype(np.uint8))
    v1, t1 = _offsets(nv), _offsets(nt)
    e1 = _offsets([int(n) - len(m.points) for n, m in zip(nv, meshes)])
    return Refinement(meshes=[mesh.Mesh(xy_out[v1[i]:v1[i + 1]], tri_out[t1[i]:t1[i + 1]]) for i in range(len(meshes))],
                      parents=[parent[t1[i]:t1[i + 1]] for i in range(len(meshes))],
                      midpoint_ends=[ends[e1[i]:e1[i + 1]] for i in range(len(meshes))], **counts)


def _flatten_points_triangles(meshes):
    xy = np.concatenate([m.points for m in meshes]) if meshes else np.zeros((0, 2), dtype=DTYPE)
    tri = np.concatenate([m.triangles for m in meshes]) if meshes else np.zeros((0, 3), dtype=np.int32)
    return np.ascontiguousarray(xy, dtype=DTYPE), np.ascontiguousarray(tri, dtype=np.int32)


@dataclass
class AdaptiveHistory:
    """What :func:`solve_meshed_adaptive` did, one entry per solve."""
    faces: list = field(default_factory=list)            # faces of the connected meshes solved
    vertices: list = field(default_factory=list)         # their vertices
    estimates: list = field(default_factory=list)        # ErrorReport.estimate
    flagged: list = field(default_factory=list)          # faces flagged after the solve (0 where the loop stopped before flagging)
    closure_edges: list = field(default_factory=list)    # edges the conforming closure halved beyond those of the flagged faces
    reason: str = ""                                     # "tolerance", "floor", "rounds" or "faces"
    meshes: list = field(default_factory=list)           # the meshes of the last solve


def check_adaptive_arguments(tolerance, max_rounds, max_faces, min_size) -> tuple:
    """(tolerance, max_rounds, max_faces, min_size) checked, or ValueError: a tolerance as :func:`check_tolerance` wants it
    and not None, max_rounds an integer >= 1, max_faces None or an integer >= 1, min_size a finite number >= 0."""
    tolerance = check_tolerance(tolerance)
    if tolerance is None:
        raise ValueError("tolerance must be a number in (0, 1): an adaptive solve needs one")
    for name, value, optional in (("max_rounds", max_rounds, False), ("max_faces", max_faces, True)):
        if value is None and optional:
            continue
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 1:
            raise ValueError(f"{name} must be an integer >= 1, not {value!r}")
    if isinstance(min_size, (bool, np.bool_, str, bytes)):
        raise ValueError("min_size must be a finite number >= 0")
    try:
        min_size = float(min_size)
    except (TypeError, ValueError):
        raise ValueError("min_size must be a finite number >= 0") from None
    if not (math.isfinite(min_size) and min_size >= 0.0):
        raise ValueError(f"min_size must be a finite number >= 0, not {min_size!r}")
    return tolerance, int(max_rounds), None if max_faces is None else int(max_faces), min_size


def solve_meshed_adaptive(prob, meshes, mesh_index_to_layer_index, *, tolerance, max_rounds=8, max_faces=None, min_size=0.0,
                          filtered_networks=None, disconnected_meshes_by_layer=None, partition=None,
                          timings: Optional[dict] = None):
    """Solve, estimate, flag, refine, until the estimate meets ``tolerance``: (Solution, ErrorReport, AdaptiveHistory).

    Every round calls :func:`solve_meshed_error` with ``tolerance`` and stops with ``history.reason``

    - ``"tolerance"`` when ``report.estimate <= tolerance``;
    - ``"floor"`` when no face has xi_f > 1 and h_f > ``min_size`` (h_f of :func:`face_sizes`, in mm);
    - ``"rounds"`` after ``max_rounds`` solves;
    - ``"faces"`` when the refined meshes would have more than ``max_faces`` faces: they are discarded.

    Otherwise the flagged faces are refined (:func:`refine_meshes`, all connected meshes in one batch) and the loop goes
    round again.  Disconnected meshes are never touched.  The Solution and the ErrorReport are those of the last solve,
    the bits ``solve_meshed_error`` gives on ``history.meshes``.  Terminals are point singularities whose faces stay
    flagged however fine the mesh (see :func:`solve_meshed_error`): without ``min_size`` or a budget only ``max_rounds``
    ends the loop on a board whose tolerance is out of reach.  Every solve starts from zero: nothing is interpolated from
    the round before.  New vertices are numbered behind the old ones of their mesh, which scatters the rows of
    neighbours; ``solve_system``'s own reordering is all that answers that.

    Arguments are checked once, before the first solve (:func:`check_adaptive_arguments`, and a ``partition`` over several
    GPUs is refused).  ``timings`` receives ``"solve"`` and ``"refine"``: the host time of all solves and all refinements."""
    _refuse_partition(partition, "adaptive solves")
    tolerance, max_rounds, max_faces, min_size = check_adaptive_arguments(tolerance, max_rounds, max_faces, min_size)
    meshes = [m if isinstance(m, mesh.Mesh) else mesh.Mesh.from_reference(m) for m in meshes]
    layer_of = list(mesh_index_to_layer_index)
    history = AdaptiveHistory()
    spent = {"solve": 0.0, "refine": 0.0}
    while True:
        since = time.perf_counter()
        solution, report = solve_meshed_error(prob, meshes, layer_of, tolerance=tolerance, filtered_networks=filtered_networks,
                                              disconnected_meshes_by_layer=disconnected_meshes_by_layer)
        spent["solve"] += time.perf_counter() - since
        history.faces.append(sum(len(m.triangles) for m in meshes))
        history.vertices.append(sum(len(m.points) for m in meshes))
        history.estimates.append(report.estimate)
        history.flagged.append(0)
        history.closure_edges.append(0)
        history.meshes = meshes
        log.info("Adaptive round %d: %d faces, estimate %.3e", len(history.faces), history.faces[-1], report.estimate)
        if report.estimate <= tolerance:
            history.reason = "tolerance"
            break
        flags = [None] * len(meshes)
        for layer_i in range(len(prob.layers)):
            members = [mi for mi, l in enumerate(layer_of) if l == layer_i]
            for mi, xi in zip(members, report.ratios[layer_i]):
                flags[mi] = (xi > 1.0) & (face_sizes(meshes[mi].points, meshes[mi].triangles) > min_size)
        history.flagged[-1] = int(sum(int(f.sum()) for f in flags))
        if history.flagged[-1] == 0:
            history.reason = "floor"
            break
        if len(history.faces) >= max_rounds:
            history.reason = "rounds"
            break
        since = time.perf_counter()
        refined = refine_meshes(meshes, flags)
        spent["refine"] += time.perf_counter() - since
        history.closure_edges[-1] = refined.marked - refined.marked_by_flags
        if max_faces is not None and sum(len(m.triangles) for m in refined.meshes) > max_faces:
            history.reason = "faces"
            break
        meshes = refined.meshes
    if timings is not None:
        timings.update(spent)
    return solution, report, history


def solve_adaptive(prob, mesher_config: Optional[mesh.Mesher.Config] = None, *, tolerance, mesher=None, max_rounds=8,
                   max_faces=None, min_size=0.0, partition=None, timings: Optional[dict] = None, prune=False):
    """``solve`` refined where the error estimate asks: the board is meshed once, then :func:`solve_meshed_adaptive`.
    Returns (Solution, ErrorReport, AdaptiveHistory)."""
    _refuse_partition(partition, "adaptive solves")
    check_adaptive_arguments(tolerance, max_rounds, max_faces, min_size)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_adaptive(prob, meshes, mesh_index_to_layer_index, tolerance=tolerance, max_rounds=max_rounds,
                                 max_faces=max_faces, min_size=min_size, timings=timings, **pruned)


# --------------------------------------------------------------------------------------------
# goal-oriented error: how far is a voltage drop off, and where must the mesh be finer for it (DESIGN.md "Goal-oriented error")
# --------------------------------------------------------------------------------------------

# correction = GOAL_CORRECTION_SIGN * sum_f delta_f estimates J(exact) - J_h: on the copper block M = -K, so the adjoint
# lambda = M^-T c is minus the dual solution z of K z = c, and J(e) = a(e, z - z_h) = -a(e, lambda - lambda_h)
GOAL_CORRECTION_SIGN = -1.0


@dataclass
class GoalError:
    """The estimated discretisation error of one objective J = V(p) - V(n) (see :func:`solve_meshed_goal_error`)."""
    nodes: tuple              # (p, n) as given: two NodeIDs
    value: float              # J_h = V(p) - V(n) of the solution [V]
    dual_indicators: list     # per layer, per mesh of LayerSolution.meshes: TwoForm of eta_f of the adjoint [sqrt(ohm)]
    contributions: list       # per layer, per mesh: TwoForm of delta_f, signed [V]
    weights: list             # per layer, per mesh: TwoForm of omega_f = eta_f eta_f^adjoint >= |delta_f| [V]
    layers: list              # per layer: (sum omega_f, sum delta_f) [V]
    worst: list               # per layer: (max omega, mesh index within the layer, face index, centroid x, y), None without faces
    bound: float              # sum of omega_f over all faces [V]: bounds |sum delta_f|
    correction: float         # GOAL_CORRECTION_SIGN * sum delta_f: the estimate of J(exact) - J_h [V]
    ratios: Optional[list] = None     # with a tolerance: per layer, per mesh (n_faces,) xi_f = omega_f n_faces / tolerance
    tolerance: Optional[float] = None


def check_goal_tolerance(tolerance) -> Optional[float]:
    """``tolerance`` as a float, None for None, or ValueError: a finite number greater than 0 (absolute, in volts); no bool
    and no string."""
    if tolerance is None:
        return None
    if isinstance(tolerance, (bool, np.bool_, str, bytes)):
        raise ValueError("tolerance must be a number of volts greater than 0")
    try:
        value = float(tolerance)
    except (TypeError, ValueError):
        raise ValueError("tolerance must be a number of volts greater than 0") from None
    if not (math.isfinite(value) and value > 0.0):
        raise ValueError(f"tolerance must be a finite number of volts greater than 0, not {tolerance!r}")
    return value


def goal_ratios(omega, n_faces: int, tolerance: float) -> np.ndarray:
    """xi_f = omega_f / (tolerance / n_faces): the permissible share of every face is the tolerance [V] divided evenly over
    the ``n_faces`` faces of the connected meshes.  Above 1: refine here."""
    omega = np.asarray(omega, dtype=DTYPE)
    return omega / (tolerance / n_faces) if n_faces > 0 else np.zeros_like(omega)


def solve_meshed_goal_error(prob, meshes, mesh_index_to_layer_index, objectives, *, tolerance=None, filtered_networks=None,
                            disconnected_meshes_by_layer=None, partition=None, timings: Optional[dict] = None):
    """``solve_meshed`` with an estimate of how far each voltage drop is off: (Solution, ErrorReport, [GoalError per objective]).

    An objective is a pair (p, n) of NodeIDs (:func:`check_objectives`), J = V(p) - V(n).  The estimate is dual-weighted:
    face by face, the gradient-recovery error of the solution x (field 0) against that of the adjoint lambda_j of the
    objective (field 1 + j; lambda_j = V W[j] as in :func:`solve_meshed_sensitivities`).  With the notation of
    :func:`solve_meshed_error`, for a field a: d_c^a = G^a_(corner c) - g_f^a, m_12^a = (d_1^a + d_2^a) / 2, and

    - ``dual_indicators``: eta_f of the adjoint, as ``ErrorReport.indicators`` is eta_f of the solution;
    - ``contributions``: delta_f = sigma (A_f / 3) (m_12^0 . m_12^(1+j) + m_23^0 . m_23^(1+j) + m_31^0 . m_31^(1+j)), signed:
      sigma times the exact integral over the face of the product of the two recovered-minus-raw gradient fields [V];
    - ``weights``: omega_f = eta_f^0 eta_f^(1+j), at least |delta_f| (Cauchy-Schwarz) up to rounding;
    - ``layers``: per layer (sum omega_f, sum delta_f); ``worst``: per layer the largest omega_f (the lowest global face on
      a tie), its mesh within the layer, its face and the face's centroid;
    - ``bound`` = sum omega_f and ``correction`` = -sum delta_f, the estimate of J(exact) - J_h.  The sign: on the copper
      block M = -K with K the positive stiffness matrix, so lambda = -z for the dual solution K z = c, and
      J(exact) - J_h = a(e, z - z_h) = -a(e, lambda - lambda_h); the lumped elements' part of the form is left out;
    - with a ``tolerance`` (absolute, in volts, > 0): ``ratios`` xi_f = omega_f / (tolerance / n_faces) with n_faces the
      faces of the connected meshes; above 1: refine here.

    The product is small wherever either field is smooth, so a terminal that does not matter to the drop is not flagged.
    Connections snap to one vertex.  If an objective node lands on the vertex of a source terminal, the drop itself grows
    like log(1/h) under refinement (the point-terminal model's own property): neither the drop nor the bound settles, and
    only ``min_size`` or a budget ends an adaptive run.  Objectives on probe nodes away from the sources -- the ends of a
    high-ohm "voltmeter" resistor between two connections -- converge, and those are what this is for.  An objective whose
    p and n snap to one unknown has a zero adjoint: all zeros, bound 0.  On meshes with obtuse faces the reference's |cot|
    edge weights add a consistency error to J_h that is no gradient jump and does not fall with h: the drop then does not
    settle across meshes and ``correction`` can have the wrong sign, while ``weights`` and ``bound`` still steer the
    refinement ("Goal-oriented error", with figures).

    One call is the block solve of :func:`solve_meshed_sensitivities` (1 + k + 2K columns), then one estimator over all
    fields on the V the device holds (``padne_kkt_goal_error``, objectives 8 per launch), every sum in a fixed order: two
    calls give the same bits.  The ErrorReport is ``solve_meshed_error``'s without a tolerance, computed by the same
    arithmetic on column 0 of this block.  Do not rely on its bits being those of a separate ``solve_meshed_error`` call:
    column 0 of a block of 1 + k + 2K columns agrees with a one-column solve to the solver's tolerance only, even where the
    two happen to coincide bit for bit (small boards).  The Solution is filled as ``solve_meshed_sensitivities`` fills it.  ValueError,
    before anything reaches the device, for invalid objectives, an invalid tolerance (:func:`check_goal_tolerance`) and a
    ``partition`` over several GPUs.  ``timings`` receives the host time of each step; ``"goal"`` is the estimator's."""
    _refuse_partition(partition, "goal-oriented error estimates")
    objectives = check_objectives(prob, objectives, filtered_networks)
    tolerance = check_goal_tolerance(tolerance)
    k = len(objectives)
    laps = _Laps(timings)
    board = index_board(prob, meshes, mesh_index_to_layer_index, filtered_networks, disconnected_meshes_by_layer)
    pairs = global_elements(board.filtered_networks, board.node_indexer)
    terms = woodbury_terms([row for _, row in pairs])
    idx = board.node_indexer.node_to_global_index
    objective_rows = [(idx[p], idx[n]) for p, n in objectives]
    n_cols = sensitivity_block_columns(k, len(terms))
    laps.lap("indexing")
    with board.assembled() as (L, _):
        rows, cols, vals = stamp_sensitivity_block(board.filtered_networks, board.node_indexer, L.shape[0], objective_rows, terms)
        laps.lap("assembly")
        log.info(f"Solving {k} adjoint(s) and {2 * len(terms)} regulator column(s) as one block with the Problem")
        plan, V, residual_norms, res, n_tri, n_mesh = _solve_block_on_device(L, rows, cols, vals, n_cols, 1, laps)
        W = adjoint_weights(V, k, terms)
        power = dual = delta = omega = m_omega = m_delta = m_top = m_face = None
        estimate_arrays = (None,) * 6
        if n_tri:
            power, estimate_arrays, dual, delta, omega, m_omega, m_delta, m_top, m_face = plan.goal_error(
                W, n_tri, len(board.vindex), n_mesh)
        laps.lap("goal")
    log.info("Producing the solution, the error report and the goal-oriented estimates")
    _warn_if_block_stalled(res, residual_norms, cols, vals, n_cols)
    solution = _column_solution(board, prob, np.ascontiguousarray(V[:, 0]), residual_norms[0], res, power)
    report = _error_report(prob, board, n_tri, estimate_arrays, None)
    goals = []
    for j, ((p, n), (ip, in_)) in enumerate(zip(objectives, objective_rows)):
        duals, contribs, weights, layer_sums, worst = [], [], [], [], []
        ratios = [] if tolerance is not None else None
        bound = total_delta = 0.0
        for layer_i in range(len(prob.layers)):
            fd, fc, fw, xis, s_om, s_de, best = [], [], [], [], 0.0, 0.0, None
            for mesh_i, msh, lo, hi in board.layer_meshes(layer_i):
                forms = [mesh.TwoForm(msh) for _ in range(3)]
                if omega is not None:
                    for tf, arr in zip(forms, (dual, delta, omega)):
                        tf.values = arr[j, lo:hi]                 # views of this call's own result arrays: no copies
                    s_om += float(m_omega[j, mesh_i])
                    s_de += float(m_delta[j, mesh_i])
                    # meshes come in global face order: a later mesh wins only with a strictly larger omega
                    if m_face[j, mesh_i] >= 0 and (best is None or m_top[j, mesh_i] > best[0]):
                        face = int(m_face[j, mesh_i] - lo)
                        cx, cy = msh.points[msh.triangles[face]].mean(axis=0)
                        best = (float(m_top[j, mesh_i]), len(fd), face, float(cx), float(cy))
                if tolerance is not None:
                    xis.append(goal_ratios(forms[2].values, n_tri, tolerance))
                fd.append(forms[0])
                fc.append(forms[1])
                fw.append(forms[2])
            duals.append(fd)
            contribs.append(fc)
            weights.append(fw)
            layer_sums.append((s_om, s_de))
            worst.append(best)
            bound += s_om
            total_delta += s_de
            if tolerance is not None:
                ratios.append(xis)
        goals.append(GoalError(nodes=(p, n), value=float(V[ip, 0] - V[in_, 0]), dual_indicators=duals, contributions=contribs,
                               weights=weights, layers=layer_sums, worst=worst, bound=bound,
                               correction=GOAL_CORRECTION_SIGN * total_delta, ratios=ratios, tolerance=tolerance))
    laps.lap("solutions")
    return solution, report, goals


def solve_goal_error(prob, objectives, mesher_config: Optional[mesh.Mesher.Config] = None, *, tolerance=None, mesher=None,
                     partition=None, prune=False):
    """``solve`` with the goal-oriented estimates of :func:`solve_meshed_goal_error`: the board is meshed once.  Returns
    (Solution, ErrorReport, [GoalError per objective])."""
    _refuse_partition(partition, "goal-oriented error estimates")
    objectives = check_objectives(prob, objectives)
    tolerance = check_goal_tolerance(tolerance)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_goal_error(prob, meshes, mesh_index_to_layer_index, objectives, tolerance=tolerance, **pruned)


@dataclass
class GoalAdaptiveHistory(AdaptiveHistory):
    """What :func:`solve_meshed_goal_adaptive` did: an AdaptiveHistory (``estimates`` stays the energy-norm estimate of each
    solve) with, per solve, one entry per objective."""
    values: list = field(default_factory=list)           # J_h [V]
    bounds: list = field(default_factory=list)           # GoalError.bound [V]


def check_goal_adaptive_arguments(tolerance, max_rounds, max_faces, min_size) -> tuple:
    """:func:`check_adaptive_arguments` with the goal tolerance in place of the relative one: (tolerance, max_rounds,
    max_faces, min_size) checked, or ValueError; the tolerance as :func:`check_goal_tolerance` wants it and not None."""
    tolerance = check_goal_tolerance(tolerance)
    if tolerance is None:
        raise ValueError("tolerance must be a number of volts greater than 0: an adaptive solve needs one")
    _, max_rounds, max_faces, min_size = check_adaptive_arguments(0.5, max_rounds, max_faces, min_size)
    return tolerance, max_rounds, max_faces, min_size


def solve_meshed_goal_adaptive(prob, meshes, mesh_index_to_layer_index, objectives, *, tolerance, max_rounds=8, max_faces=None,
                               min_size=0.0, filtered_networks=None, disconnected_meshes_by_layer=None, partition=None,
                               timings: Optional[dict] = None):
    """Solve, estimate, flag, refine, until every drop's bound meets ``tolerance`` [V]: (Solution, ErrorReport,
    [GoalError per objective], GoalAdaptiveHistory).

    The loop and the reasons are those of :func:`solve_meshed_adaptive`, steered by :func:`solve_meshed_goal_error`:

    - ``"tolerance"`` when max_j bound_j <= ``tolerance``;
    - ``"floor"`` when no face has max_j xi_jf > 1 and h_f > ``min_size``;
    - ``"rounds"`` after ``max_rounds`` solves;
    - ``"faces"`` when the refined meshes would have more than ``max_faces`` faces: they are discarded.

    ``history.values`` and ``history.bounds`` hold J_h and the bound of every objective for each solve;
    ``history.estimates`` stays the energy-norm estimate.  The results are those of the last solve, the bits
    ``solve_meshed_goal_error`` gives on ``history.meshes``.  See there for objectives that sit on a source terminal: their
    bound does not settle and only ``min_size`` or a budget ends the run.  Arguments are checked once, before the first
    solve (:func:`check_objectives`, :func:`check_goal_adaptive_arguments`; a ``partition`` over several GPUs is refused)."""
    _refuse_partition(partition, "adaptive solves")
    objectives = check_objectives(prob, objectives, filtered_networks)
    tolerance, max_rounds, max_faces, min_size = check_goal_adaptive_arguments(tolerance, max_rounds, max_faces, min_size)
    meshes = [m if isinstance(m, mesh.Mesh) else mesh.Mesh.from_reference(m) for m in meshes]
    layer_of = list(mesh_index_to_layer_index)
    history = GoalAdaptiveHistory()
    spent = {"solve": 0.0, "refine": 0.0}
    while True:
        since = time.perf_counter()
        solution, report, goals = solve_meshed_goal_error(prob, meshes, layer_of, objectives, tolerance=tolerance,
                                                          filtered_networks=filtered_networks,
                                                          disconnected_meshes_by_layer=disconnected_meshes_by_layer)
        spent["solve"] += time.perf_counter() - since
        history.faces.append(sum(len(m.triangles) for m in meshes))
        history.vertices.append(sum(len(m.points) for m in meshes))
        history.estimates.append(report.estimate)
        history.values.append([g.value for g in goals])
        history.bounds.append([g.bound for g in goals])
        history.flagged.append(0)
        history.closure_edges.append(0)
        history.meshes = meshes
        log.info("Goal-adaptive round %d: %d faces, largest bound %.3e V", len(history.faces), history.faces[-1],
                 max(history.bounds[-1]))
        if max(history.bounds[-1]) <= tolerance:
            history.reason = "tolerance"
            break
        flags = [None] * len(meshes)
        for layer_i in range(len(prob.layers)):
            members = [mi for mi, l in enumerate(layer_of) if l == layer_i]
            for pos, mi in enumerate(members):
                xi = np.max([g.ratios[layer_i][pos] for g in goals], axis=0)
                flags[mi] = (xi > 1.0) & (face_sizes(meshes[mi].points, meshes[mi].triangles) > min_size)
        history.flagged[-1] = int(sum(int(f.sum()) for f in flags))
        if history.flagged[-1] == 0:
            history.reason = "floor"
            break
        if len(history.faces) >= max_rounds:
            history.reason = "rounds"
            break
        since = time.perf_counter()
        refined = refine_meshes(meshes, flags)
        spent["refine"] += time.perf_counter() - since
        history.closure_edges[-1] = refined.marked - refined.marked_by_flags
        if max_faces is not None and sum(len(m.triangles) for m in refined.meshes) > max_faces:
            history.reason = "faces"
            break
        meshes = refined.meshes
    if timings is not None:
        timings.update(spent)
    return solution, report, goals, history


def solve_goal_adaptive(prob, objectives, mesher_config: Optional[mesh.Mesher.Config] = None, *, tolerance, mesher=None,
                        max_rounds=8, max_faces=None, min_size=0.0, partition=None, timings: Optional[dict] = None, prune=False):
    """``solve`` refined where the voltage drops ask: the board is meshed once, then :func:`solve_meshed_goal_adaptive`.
    Returns (Solution, ErrorReport, [GoalError per objective], GoalAdaptiveHistory)."""
    _refuse_partition(partition, "adaptive solves")
    objectives = check_objectives(prob, objectives)
    check_goal_adaptive_arguments(tolerance, max_rounds, max_faces, min_size)
    meshes, mesh_index_to_layer_index, pruned = _meshed(prob, mesher_config, mesher, prune)
    return solve_meshed_goal_adaptive(prob, meshes, mesh_index_to_layer_index, objectives, tolerance=tolerance,
                                      max_rounds=max_rounds, max_faces=max_faces, min_size=min_size, timings=timings, **pruned)


# --------------------------------------------------------------------------------------------
# sampling: the solved fields at points, along lines and on rasters
# --------------------------------------------------------------------------------------------

MAX_SAMPLE_POINTS = 2 ** 26
MAX_RASTER_PIXELS = 2 ** 26


@dataclass
class FieldSamples:
    """What a :class:`FieldSampler` returns: per sample the owner face as (``mesh`` within ``LayerSolution.meshes``, ``face``
    within that mesh), -1 / -1 outside the copper, the ``potential`` [V] interpolated in that face, and the face's
    ``current_density`` (.., 2) [A/mm] and ``power_density``; NaN outside.  ``points`` are the sampled (x, y); a line also
    carries the ``arc_length`` of each sample from its start.  A raster's arrays are shaped (height, width[, 2])."""
    points: np.ndarray
    face: np.ndarray
    mesh: np.ndarray
    potential: np.ndarray
    current_density: np.ndarray
    power_density: np.ndarray
    arc_length: Optional[np.ndarray] = None


def _layer_index(prob, layer) -> int:
    layer_i = next((i for i, own in enumerate(prob.layers) if own is layer), None)
    if layer_i is None:
        raise ValueError("the layer is not one of the Problem's layers")
    return layer_i


def check_sample_points(prob, layer, xy) -> tuple:
    """(layer index, the points as a float64 (n, 2) array), or ValueError: ``layer`` is one of ``prob.layers`` (by
    identity), ``xy`` is (n, 2) with n <= MAX_SAMPLE_POINTS and finite."""
    layer_i = _layer_index(prob, layer)
    try:
        pts = np.asarray(xy)
    except (TypeError, ValueError):
        raise ValueError("sample points must be an (n, 2) array of numbers") from None
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"sample points must have shape (n, 2), not {pts.shape}")
    if len(pts) > MAX_SAMPLE_POINTS:
        raise ValueError(f"{len(pts)} sample points: at most {MAX_SAMPLE_POINTS} in one call")
    try:
        pts = np.array(pts, dtype=DTYPE)
    except (TypeError, ValueError):
        raise ValueError("sample points must be an (n, 2) array of numbers") from None
    if not np.isfinite(pts).all():
        raise ValueError("sample points are not finite")
    return layer_i, np.ascontiguousarray(pts)


def check_raster(prob, layer, origin, pixel, width, height) -> tuple:
    """(layer index, x0, y0, dx, dy, width, height), or ValueError: ``origin`` is a finite (x, y), the lower corner of pixel
    (0, 0); ``pixel`` a finite positive size, one number or (dx, dy); ``width`` and ``height`` integers >= 1 with at most
    MAX_RASTER_PIXELS pixels, all of whose centres are finite."""
    layer_i = _layer_index(prob, layer)
    x0, y0 = _cut_point(origin, 0, "the raster's origin")
    try:
        dx, dy = (float(pixel), float(pixel)) if np.ndim(pixel) == 0 else (float(pixel[0]), float(pixel[1]))
        if np.ndim(pixel) != 0 and len(pixel) != 2:
            raise ValueError
    except (TypeError, ValueError, IndexError):
        raise ValueError("the pixel size must be one number or (dx, dy)") from None
    if not (math.isfinite(dx) and math.isfinite(dy) and dx > 0 and dy > 0):
        raise ValueError("the pixel size must be finite and positive")
    try:
        w, h = int(width), int(height)
        if w != width or h != height:
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError("width and height must be integers") from None
    if w < 1 or h < 1:
        raise ValueError("a raster has at least one pixel in each direction")
    if w * h > MAX_RASTER_PIXELS:
        raise ValueError(f"{w} x {h} pixels: at most {MAX_RASTER_PIXELS} in one call")
    if not (math.isfinite(x0 + ((w - 1) + 0.5) * dx) and math.isfinite(y0 + ((h - 1) + 0.5) * dy)):
        raise ValueError("the raster's pixel centres are not finite")
    return layer_i, x0, y0, dx, dy, w, h


def check_sample_line(prob, layer, start, end, n) -> tuple:
    """(layer index, the points (n, 2), their arc lengths (n,)) of a line of ``n`` >= 2 points from ``start`` to ``end``
    inclusive, or ValueError: the ends are finite (x, y), ``n`` an integer of at most MAX_SAMPLE_POINTS."""
    _layer_index(prob, layer)
    a, b = _cut_point(start, 0, "the line's start"), _cut_point(end, 0, "the line's end")
    try:
        count = int(n)
    except (TypeError, ValueError):
        raise ValueError("a line has an integer number of points") from None
    if count != n or count < 2:
        raise ValueError("a line has at least 2 points")
    if count > MAX_SAMPLE_POINTS:
        raise ValueError(f"{count} sample points: at most {MAX_SAMPLE_POINTS} in one call")
    xy = np.stack([np.linspace(a[0], b[0], count), np.linspace(a[1], b[1], count)], axis=1)
    layer_i, pts = check_sample_points(prob, layer, xy)
    return layer_i, pts, np.linspace(0.0, math.hypot(b[0] - a[0], b[1] - a[1]), count)


class FieldSampler:
    """Reads a :class:`Solution` out at arbitrary points: built once, it keeps the meshes, the potentials and a
    point-location index on the device and answers ``points``, ``line`` and ``raster`` until ``close`` (a context manager).

    For a point q on a layer, with the layer's faces numbered in the order of ``LayerSolution.meshes``:

    - the *owner* is the lowest face that contains q.  side(i, k) = orient(P, Q, q) for a face's edge taken from its lower
      vertex index P to its higher Q, negated where the face runs it from Q to P, so the two faces of an edge see the same
      number with opposite signs; a face contains q when its three sides are all >= 0 or all <= 0 and not all zero.  A
      point on a shared edge or vertex has exactly one owner; a point outside the outline or in a hole has none (-1, NaN);
    - ``potential`` is the linear interpolant of the owner's corner potentials with the weights side / (sum of the sides);
    - ``current_density`` and ``power_density`` are the owner's face values, the same bits as ``CurrentReport.vectors`` and
      ``LayerSolution.power_densities``.

    ``disconnected_meshes`` carry no field and take no part.  Works on any Solution whose meshes have ``points`` and
    ``triangles`` arrays (:class:`padne_amd.mesh.Mesh`).  ``bins_hint``: bins of each layer's grid, 0 = chosen."""

    def __init__(self, solution: Solution, *, bins_hint: int = 0):
        self.solution = solution
        self.problem = solution.problem
        pts, tris, pots, sig, layer_of = [], [], [], [], []
        self._first_mesh = []                          # per layer: its first mesh in the flat order
        for layer_i, (layer, ls) in enumerate(zip(self.problem.layers, solution.layer_solutions)):
            self._first_mesh.append(len(layer_of))
            for msh, zf in zip(ls.meshes, ls.potentials):
                pts.append(np.asarray(msh.points, dtype=DTYPE).reshape(-1, 2))
                tris.append(np.asarray(msh.triangles, dtype=np.int32).reshape(-1, 3))
                pots.append(np.asarray(zf.values, dtype=DTYPE).reshape(-1))
                sig.append(float(layer.conductance))
                layer_of.append(layer_i)
        mvo = _offsets([len(p) for p in pts])
        self._mto = _offsets([len(t) for t in tris])
        cat = lambda arrays, shape, dtype: (np.concatenate(arrays) if arrays else np.zeros(shape, dtype=dtype))  # noqa: E731
        self._dev = _hip.Sampler(get_context(), cat(pts, (0, 2), DTYPE), cat(tris, (0, 3), np.int32), mvo, self._mto, layer_of,
                                 sig, len(self.problem.layers), cat(pots, (0,), DTYPE), bins_hint)

    def close(self) -> None:
        if self._dev is not None:
            self._dev.close()
        self._dev = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _device(self) -> _hip.Sampler:
        if self._dev is None:
            raise ValueError("the FieldSampler is closed")
        return self._dev

    def _samples(self, layer_i: int, points, raw, shape=None, arc=None) -> FieldSamples:
        gface, v, j, p = raw
        # global face -> (mesh within the layer, face within the mesh): the meshes of a layer are adjacent in the flat order
        g = gface.astype(np.int64)
        m = np.searchsorted(self._mto, g, side="right") - 1
        inside = g >= 0
        mesh_i = np.where(inside, m - self._first_mesh[layer_i], -1)
        face = np.where(inside, g - self._mto[np.clip(m, 0, len(self._mto) - 1)], -1)
        if shape is not None:
            mesh_i, face, v, p = (a.reshape(shape) for a in (mesh_i, face, v, p))
            j = j.reshape(shape + (2,))
        return FieldSamples(points=points, face=face, mesh=mesh_i, potential=v, current_density=j, power_density=p,
                            arc_length=arc)

    def points(self, layer, xy) -> FieldSamples:
        """The fields at the points ``xy`` (n, 2) of ``layer``."""
        layer_i, pts = check_sample_points(self.problem, layer, xy)
        return self._samples(layer_i, pts, self._device().points(layer_i, pts))

    def line(self, layer, start, end, n: int) -> FieldSamples:
        """``n`` >= 2 points from ``start`` to ``end`` inclusive (``np.linspace`` per coordinate), with ``arc_length``
        ``np.linspace(0, |end - start|, n)``: the profile along a trace."""
        layer_i, pts, arc = check_sample_line(self.problem, layer, start, end, n)
        return self._samples(layer_i, pts, self._device().points(layer_i, pts), arc=arc)

    def raster(self, layer, origin, pixel, width: int, height: int) -> FieldSamples:
        """The fields at the centres of ``width`` x ``height`` pixels of size ``pixel`` (one number or (dx, dy)), pixel
        (row j, column i) centred at (origin.x + (i + 0.5) dx, origin.y + (j + 0.5) dy).  Arrays are (height, width)."""
        layer_i, x0, y0, dx, dy, w, h = check_raster(self.problem, layer, origin, pixel, width, height)
        raw = self._device().raster(layer_i, x0, y0, dx, dy, w, h)
        xs, ys = x0 + (np.arange(w) + 0.5) * dx, y0 + (np.arange(h) + 0.5) * dy
        pts = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), axis=2)
        return self._samples(layer_i, pts, raw, shape=(h, w))

    def stats(self, layer) -> dict:
        """Index and timing figures of ``layer`` (``_hip.Sampler.stats``)."""
        return self._device().stats(_layer_index(self.problem, layer))


# --------------------------------------------------------------------------------------------
# thermal images: temperature fields at points, along lines and on rasters
# --------------------------------------------------------------------------------------------

MAX_SAMPLE_FIELDS = 256
MAX_SAMPLE_VALUES = 2 ** 28


@dataclass
class TemperatureSamples:
    """What a :class:`TemperatureSampler` returns.  ``points``, ``face``, ``mesh`` and ``arc_length`` as in
    :class:`FieldSamples` (-1 / -1 outside the copper).  With F fields and n samples, or a raster of (height, width):

    - ``temperature`` (F, n) or (F, height, width): every field interpolated in the owner face, NaN outside the copper;
      None with ``per_field=False``;
    - ``heat_flux`` (F, n, 2) or (F, height, width, 2): -kappa grad T of the owner face [W per mesh unit of length]; None
      unless ``flux=True``;
    - ``hottest`` and ``hottest_field`` (int32): the maximum over the fields per sample and the field that attains it, by
      the sequential rule of :func:`envelope_of` (field 0 first, replaced on strictly greater); NaN and -1 outside;
    - ``names``: the fields' names, ``hottest_field`` indexes them;
    - ``tops``: None for points and lines; for a raster F + 1 entries, one per field and a last one for ``hottest``, each
      ``(T, row, column, x, y)`` of the hottest pixel that lies on copper -- the lowest ``row * width + column`` keeps a
      tie -- or None where no pixel does."""
    points: np.ndarray
    face: np.ndarray
    mesh: np.ndarray
    temperature: Optional[np.ndarray]
    heat_flux: Optional[np.ndarray]
    hottest: np.ndarray
    hottest_field: np.ndarray
    names: list
    arc_length: Optional[np.ndarray] = None
    tops: Optional[list] = None


def check_temperature_fields(prob, fields, names=None) -> tuple:
    """(the meshes of field 0 as (layer index, Mesh) in flat order, the values as an (F, n_vert) block, the names), or
    ValueError: ``fields`` is a sequence of 1 <= F <= MAX_SAMPLE_FIELDS fields, each per layer of ``prob`` a list of
    :class:`padne_amd.mesh.ZeroForm` -- with the layers and meshes of field 0, per mesh the same Mesh or one of equal
    ``points`` and ``triangles``, and one finite value per vertex.  ``names`` names the fields (default 0 .. F - 1)."""
    try:
        fields = list(fields)
    except TypeError:
        raise ValueError("fields must be a sequence of temperature fields") from None
    count = len(fields)
    if not 1 <= count <= MAX_SAMPLE_FIELDS:
        raise ValueError(f"{count} fields: a TemperatureSampler takes 1 to {MAX_SAMPLE_FIELDS}")
    names = list(range(count)) if names is None else list(names)
    if len(names) != count:
        raise ValueError(f"{len(names)} names for {count} fields")
    n_layers = len(prob.layers)
    flat, rows = [], []
    for f, (name, fld) in enumerate(zip(names, fields)):
        what = f"field {name!r}"
        if fld is None:
            raise ValueError(f"{what} is None: a report made with per_case_fields=False keeps no field to sample")
        try:
            layers = [list(per_layer) for per_layer in fld]
        except TypeError:
            raise ValueError(f"{what} must hold, per layer, a list of ZeroForms") from None
        if len(layers) != n_layers:
            raise ValueError(f"{what} has {len(layers)} layers, the Problem has {n_layers}")
        values, at = [], 0
        for li, per_layer in enumerate(layers):
            if f and len(per_layer) != sum(1 for lj, _ in flat if lj == li):
                raise ValueError(f"{what}, layer {li}: {len(per_layer)} meshes, field {names[0]!r} has "
                                 f"{sum(1 for lj, _ in flat if lj == li)}")
            for mi, zf in enumerate(per_layer):
                where = f"{what}, layer {li}, mesh {mi}"
                msh, vals = getattr(zf, "mesh", None), getattr(zf, "values", None)
                if msh is None or vals is None or not hasattr(msh, "points") or not hasattr(msh, "triangles"):
                    raise ValueError(f"{where}: not a ZeroForm on a mesh with points and triangles")
                if f == 0:
                    flat.append((li, msh))
                else:
                    own = flat[at][1]
                    if msh is not own and not (np.array_equal(np.asarray(msh.points), np.asarray(own.points)) and
                                               np.array_equal(np.asarray(msh.triangles), np.asarray(own.triangles))):
                        raise ValueError(f"{where}: another mesh than field {names[0]!r}'s")
                try:
                    vals = np.asarray(vals, dtype=DTYPE).reshape(-1)
                except (TypeError, ValueError):
                    raise ValueError(f"{where}: the values are not numbers") from None
                n_vert = len(np.asarray(flat[at][1].points).reshape(-1, 2))
                if len(vals) != n_vert:
                    raise ValueError(f"{where}: {len(vals)} values for {n_vert} vertices")
                if not np.isfinite(vals).all():
                    raise ValueError(f"{where}: the values are not finite")
                values.append(vals)
                at += 1
        rows.append(np.concatenate(values) if values else np.zeros(0, dtype=DTYPE))
    return flat, np.ascontiguousarray(np.stack(rows)), names


class TemperatureSampler:
    """Reads a block of temperature fields out at arbitrary points: the thermal image, the profile along a trace, the
    temperature at a sensor.  A *field* is what the thermal reports hold -- per layer, per connected mesh, a ZeroForm of T
    (``ThermalReport.temperatures``, ``ThermalEnvelope.temperatures``, ``TransientReport.temperatures[i]``,
    ``TransientEnvelope.temperatures``); ``fields`` is a sequence of them on the meshes of field 0.  Built once, it keeps the
    meshes, the fields and :class:`FieldSampler`'s point-location index on the device until ``close`` (a context manager),
    and every query locates each point once and reads all fields at it.

    The owner of a point is :class:`FieldSampler`'s.  ``temperature`` is the linear interpolant of the owner's corner values
    with the weights side / (sum of the sides), so at a vertex it is the vertex value itself; ``heat_flux`` is -kappa grad T
    of the owner, kappa the sheet conductance ``model`` (a :class:`ThermalModel`, resolved by :func:`check_thermal_model`)
    gives the owner's layer -- without a model, asking for it is a ValueError.  See :class:`TemperatureSamples`.

    Limits: disconnected meshes carry no field and take no part (a point on them is outside the copper: NaN, not ambient);
    there is no interpolation in time between kept snapshots; one GPU.  ``bins_hint`` as in :class:`FieldSampler`."""

    def __init__(self, prob, fields, *, names=None, model=None, bins_hint: int = 0):
        self.problem = prob
        flat, block, self.names = check_temperature_fields(prob, fields, names)
        checked = None
        if model is not None:
            checked = model if isinstance(model, CheckedThermalModel) else check_thermal_model(prob, model)
        self.n_fields = block.shape[0]
        pts = [np.asarray(msh.points, dtype=DTYPE).reshape(-1, 2) for _, msh in flat]
        tris = [np.asarray(msh.triangles, dtype=np.int32).reshape(-1, 3) for _, msh in flat]
        layer_of = [li for li, _ in flat]
        self._first_mesh = [sum(1 for lj in layer_of if lj < li) for li in range(len(prob.layers))]
        mvo = _offsets([len(p) for p in pts])
        self._mto = _offsets([len(t) for t in tris])
        cat = lambda arrays, shape, dtype: (np.concatenate(arrays) if arrays else np.zeros(shape, dtype=dtype))  # noqa: E731
        self._kappa = None if checked is None else np.array([checked.kappa[li] for li in layer_of], dtype=DTYPE)
        # the handle is a FieldSampler's: zero potentials, the layers' electrical conductances
        self._dev = _hip.Sampler(get_context(), cat(pts, (0, 2), DTYPE), cat(tris, (0, 3), np.int32), mvo, self._mto, layer_of,
                                 [float(prob.layers[li].conductance) for li in layer_of], len(prob.layers),
                                 np.zeros(block.shape[1], dtype=DTYPE), bins_hint)
        try:
            self._dev.set_fields(block, self._kappa)
        except Exception:
            self.close()
            raise

    @classmethod
    def of_reports(cls, prob, reports, *, envelope=None, model=None, bins_hint: int = 0):
        """Of one :class:`ThermalReport` or a list of them (the load cases of :func:`solve_meshed_thermal`), and optionally
        their :class:`ThermalEnvelope`: the cases in order named 0 .. k - 1, then the field ``"envelope"``."""
        reports = [reports] if isinstance(reports, ThermalReport) else list(reports)
        if not all(isinstance(r, ThermalReport) for r in reports):
            raise ValueError("reports must be a ThermalReport or a sequence of them")
        fields, names = [r.temperatures for r in reports], list(range(len(reports)))
        if envelope is not None:
            if not isinstance(envelope, ThermalEnvelope):
                raise ValueError("envelope must be a ThermalEnvelope")
            fields.append(envelope.temperatures)
            names.append("envelope")
        return cls(prob, fields, names=names, model=model, bins_hint=bins_hint)

    @classmethod
    def of_transient(cls, prob, report, *, model=None, bins_hint: int = 0):
        """Of a :class:`TransientReport` (also ``PeriodicReport.cycle``): the kept snapshots in order, named by their
        ``snapshot_times``, then ``report.envelope.temperatures`` as ``"envelope"`` -- alone where no field was kept."""
        if not isinstance(report, TransientReport):
            raise ValueError("report must be a TransientReport")
        fields = list(report.temperatures or []) + [report.envelope.temperatures]
        names = list(report.snapshot_times or [])[:len(fields) - 1] + ["envelope"]
        return cls(prob, fields, names=names, model=model, bins_hint=bins_hint)

    def close(self) -> None:
        if getattr(self, "_dev", None) is not None:
            self._dev.close()
        self._dev = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _device(self) -> _hip.Sampler:
        if self._dev is None:
            raise ValueError("the TemperatureSampler is closed")
        return self._dev

    def _check_outputs(self, n: int, flux: bool, per_field: bool) -> None:
        if flux and self._kappa is None:
            raise ValueError("heat_flux needs the sheet conductances: give the TemperatureSampler a model")
        if (per_field or flux) and self.n_fields * n > MAX_SAMPLE_VALUES:
            raise ValueError(f"{self.n_fields} fields x {n} samples: at most {MAX_SAMPLE_VALUES} values in one call that "
                             "returns every field (per_field=False without flux returns the hottest alone)")

    def _samples(self, layer_i: int, points, raw, shape=None, arc=None) -> TemperatureSamples:
        gface, t, q, hot, hot_field = raw[:5]
        g = gface.astype(np.int64)
        m = np.searchsorted(self._mto, g, side="right") - 1
        inside = g >= 0
        mesh_i = np.where(inside, m - self._first_mesh[layer_i], -1)
        face = np.where(inside, g - self._mto[np.clip(m, 0, len(self._mto) - 1)], -1)
        tops = None
        if shape is not None:
            mesh_i, face, hot, hot_field = (a.reshape(shape) for a in (mesh_i, face, hot, hot_field))
            t = None if t is None else t.reshape((self.n_fields,) + shape)
            q = None if q is None else q.reshape((self.n_fields,) + shape + (2,))
            tops = []
            for value, pixel in zip(raw[5], raw[6]):
                row, col = divmod(int(pixel), shape[1])
                tops.append(None if pixel < 0 else (float(value), row, col, float(points[row, col, 0]), float(points[row, col, 1])))
        return TemperatureSamples(points=points, face=face, mesh=mesh_i, temperature=t, heat_flux=q, hottest=hot,
                                  hottest_field=hot_field, names=list(self.names), arc_length=arc, tops=tops)

    def points(self, layer, xy, *, flux: bool = False, per_field: bool = True) -> TemperatureSamples:
        """The fields at the points ``xy`` (n, 2) of ``layer``."""
        layer_i, pts = check_sample_points(self.problem, layer, xy)
        self._check_outputs(len(pts), flux, per_field)
        return self._samples(layer_i, pts, self._device().field_points(layer_i, pts, per_field, flux))

    def line(self, layer, start, end, n: int, *, flux: bool = False, per_field: bool = True) -> TemperatureSamples:
        """``n`` >= 2 points from ``start`` to ``end`` inclusive with their ``arc_length``, as :meth:`FieldSampler.line`."""
        layer_i, pts, arc = check_sample_line(self.problem, layer, start, end, n)
        self._check_outputs(len(pts), flux, per_field)
        return self._samples(layer_i, pts, self._device().field_points(layer_i, pts, per_field, flux), arc=arc)

    def raster(self, layer, origin, pixel, width: int, height: int, *, flux: bool = False,
               per_field: bool = True) -> TemperatureSamples:
        """The fields at the pixel centres of :meth:`FieldSampler.raster`'s raster, arrays (F, height, width), and ``tops``."""
        layer_i, x0, y0, dx, dy, w, h = check_raster(self.problem, layer, origin, pixel, width, height)
        self._check_outputs(w * h, flux, per_field)
        raw = self._device().field_raster(layer_i, x0, y0, dx, dy, w, h, per_field, flux)
        xs, ys = x0 + (np.arange(w) + 0.5) * dx, y0 + (np.arange(h) + 0.5) * dy
        pts = np.stack(np.broadcast_arrays(xs[None, :], ys[:, None]), axis=2)
        return self._samples(layer_i, pts, raw, shape=(h, w))

    def stats(self, layer) -> dict:
        """Index and timing figures of ``layer`` (``_hip.Sampler.stats``)."""
        return self._device().stats(_layer_index(self.problem, layer))

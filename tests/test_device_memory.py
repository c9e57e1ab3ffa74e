"""What the kernels do to the memory they run in (needs an MI355X).

Every other GPU test compares values.  None knows that the pool (capi.hip: pool_alloc) rounds a request up to a power of two,
so that a write a few elements past an array lands in the block's own slack, or that a fresh block is zero pages and a recycled
one usually holds the same array of the previous, identical call, so that a word read before anything wrote it has the right
value.  Here every driver runs three times -- switch unset, PADNE_POOL_GUARD=00, PADNE_POOL_GUARD=ff -- and ``three_ways``
asserts that

  * every returned array, iteration count and residual is bit for bit the same in the three runs: a read of unwritten memory
    that is harmless under zeros differs under 0xff (NaN in both float widths, -1 in every integer width, so that a stale
    index stays inside the front guard zone);
  * no guard zone was changed (violations == 0): a write in front of a block or behind the REQUESTED size is counted when the
    block is freed;
  * the guarded runs handed out guarded blocks and the plain one none.

The first test is the mode's own self-test (padne_test_pool_guard op 2): the drivers prove nothing unless the detector detects.
The guarded mode is entered nowhere else in the suite.

Wall times on the MI355X, per test (its three runs, the host-side preparation and the comparison included; the whole module:
73 tests in 11.3 s):

    multigrid setup and cycle     d, dx (144 k unknowns) 0.58 s each; a, c, g, f and the forced paths 0.10 - 0.16 s
    assembly                      hub and ragged boards 0.42 s (the host's random choice of 700 pads), golden fixtures 0.12 -
                                  0.14 s, grids at the tile edges 0.07 - 0.08 s, nearest vertex 0.07 s
    relabel / reduce / vstack     0.15 - 0.22 s
    products                      0.07 - 0.08 s
    PCG, lockstep, dense inverse  0.08 - 0.14 s
    KKT plan                      golden fixtures and the nine-column block 0.08 - 0.09 s, the strip order 0.41 s (two Delaunay
                                  triangulations on the host)
    post-processing               problem_many_meshes 0.14 - 0.24 s, problem_mixed 0.10 - 0.12 s; refine 0.12 s, goal error of
                                  four fields 0.13 s
    order dependence              0.06 s plain, 0.13 s under 0xff
    the self-test                 0.01 s

A guarded run of a driver costs 10 - 40 ms more than the plain one (25 - 400 guarded blocks each: three fills and a wait at
the allocation, a wait for the device and two copies at the free).

Shown able to fail, in a scratch library (one change each, not committed).  Every change was chosen so that the changed code
still stays inside its own allocations -- values and flags, no index or count -- because a wild index would be a fault on
the GPU and not a red test:

    amg_setup without the f32_copy_amg launch that fills coarse_inv32 (the single-precision copy of the coarsest inverse is
        never written): 26 tests red -- every multigrid setup-and-cycle case, PCG with multigrid (not with Jacobi), every
        lockstep width, the strip order and all of problem_many_meshes' post-processing: "fill 00: out[0] differs from the
        plain run"; the dense-inverse driver (its cycle is the double-precision inverse alone), the golden fixtures and
        problem_mixed (below the dense-inverse size) stay green.  Without the guarded mode a fresh block is zero pages, and a
        cycle without its coarse correction is still a preconditioner
    assemble_system without the hipMemsetAsync of its error words d_err: 41 tests red -- every assembly driver and
        everything that assembles a board (KKT plan, post-processing, order dependence): under 0xff the untouched words
        read as "triangle refers to a vertex outside its mesh"; products, relabel, the multigrid cases on given matrices
        and refine stay green
    padne_amg_apply with its output vector allocated one element short, the cycle unchanged: 11 tests red -- the nine
        multigrid setup-and-cycle cases and both dense-inverse drivers: "pool guard: a block of 19184 bytes was written
        behind its end: first changed byte at offset 19184 of the block" (case a: 2398 doubles), under both fill bytes;
        the values stay right, since the copy back reads the element from the guard zone
"""
import dataclasses
import gc
import time
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as R
import helpers as H
import sensitivity_ref as S
from oracle import padne_oracle as O
from padne_amd import _hip, mesh, reduction, solver, synthetic

pytestmark = pytest.mark.gpu

MODES = (None, "00", "ff")
_DETECTOR = {"ok": False}


# ---- comparing everything a driver returns ---------------------------------------------------------------------------------

def leaves(obj, path="out", out=None):
    """Every array and scalar under ``obj`` as (path, dtype, shape, bytes), in a fixed order.  Wall times (names with
    "second" or "timing") and the objects of the Problem are left out."""
    out = [] if out is None else out
    if obj is None or isinstance(obj, (str, bytes, bool)):
        out.append((path, "py", (), repr(obj)))
    elif isinstance(obj, (int, float, complex, np.generic, np.ndarray)):
        a = np.asarray(obj)
        out.append((path, a.dtype.str, a.shape, np.ascontiguousarray(a).tobytes()))
    elif sp.issparse(obj):
        m = obj.tocsr()
        leaves([m.shape, m.indptr, m.indices, m.data], path + ".csr", out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            leaves(v, f"{path}[{i}]", out)
    elif isinstance(obj, dict):
        for i, (k, v) in enumerate(obj.items()):
            if isinstance(k, str) and ("second" in k or "timing" in k):
                continue
            leaves(v, f"{path}[{k if isinstance(k, (str, int)) else i}]", out)
    elif isinstance(obj, mesh.Mesh):
        leaves([obj.points, obj.triangles], path + ".mesh", out)
    elif isinstance(obj, (mesh.ZeroForm, mesh.TwoForm)):
        leaves(obj.values, path + ".values", out)
    elif type(obj).__module__ == "padne_amd.problem":
        pass
    elif dataclasses.is_dataclass(obj):
        for f in dataclasses.fields(obj):
            if "second" in f.name or "timing" in f.name:
                continue
            leaves(getattr(obj, f.name), f"{path}.{f.name}", out)
    else:
        raise TypeError(f"{path}: a {type(obj).__name__} cannot be compared")
    return out


def self_test(ctx, switches):
    """padne_test_pool_guard op 2 under both fill bytes: the block reads back as the fill byte, a write behind the requested
    size and one in front of the block are both counted, with the side and the offset; without the switch the entry refuses."""
    with pytest.raises(ValueError):
        ctx.pool_guard(2)
    assert ctx.pool_guard(1)["allocations"] == 0 and ctx.pool_guard(0)["fill"] == -1
    for fill in ("00", "ff"):
        switches.set("PADNE_POOL_GUARD", fill)
        try:
            assert ctx.pool_guard(1) == dict(allocations=0, violations=0, first=(0, None, 0), last=(None, 0), fill=int(fill, 16))
            got = ctx.pool_guard(2)
            assert got["fill"] == 1, "the block handed out did not hold the fill byte"
            assert got["allocations"] == 2 and got["violations"] == 2, got
            assert got["first"] == (1000, "back", 1000) and got["last"] == ("front", -8), got
            assert b"pool guard" in ctx._lib.padne_last_error()
            assert ctx.pool_guard(1)["violations"] == 0
        finally:
            switches.unset("PADNE_POOL_GUARD")
    _DETECTOR["ok"] = True


def three_ways(ctx, switches, fn, env=None):
    """fn() with the switch unset, under PADNE_POOL_GUARD=00 and =ff (and ``env`` in all three): the same bits, no violation."""
    if not _DETECTOR["ok"]:
        self_test(ctx, switches)
    runs, stats, times = [], [], []
    for mode in MODES:
        for k, v in (env or {}).items():
            switches.set(k, v)
        if mode is not None:
            switches.set("PADNE_POOL_GUARD", mode)
        try:
            gc.collect()
            ctx.pool_guard(1)
            t0 = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", solver.SolverWarning)
                out = fn()
            times.append(time.perf_counter() - t0)
            runs.append(leaves(out))
            del out
            gc.collect()              # what the driver left to the collector is freed, and checked, under the mode it ran in
            stats.append(ctx.pool_guard(0))
        finally:
            switches.unset("PADNE_POOL_GUARD")
            for k in (env or {}):
                switches.unset(k)
    print("wall", " ".join(f"{m or 'plain'} {t:.2f}s" for m, t in zip(MODES, times)), "| guarded blocks",
          [s["allocations"] for s in stats], "| leaves", len(runs[0]))
    for mode, st in zip(MODES, stats):
        assert st["violations"] == 0, (mode, st, ctx._lib.padne_last_error())
    assert stats[0]["allocations"] == 0 and stats[1]["allocations"] > 0 and stats[2]["allocations"] > 0, stats
    assert len(runs[0]) > 0
    for mode, run in zip(MODES[1:], runs[1:]):
        assert [r[:3] for r in run] == [r[:3] for r in runs[0]], f"fill {mode}: other arrays than the plain run"
        for (path, _, _, plain), (_, _, _, got) in zip(runs[0], run):
            assert got == plain, f"fill {mode}: {path} differs from the plain run"


def flat(meshes_spec):
    xy = np.concatenate([m[0] for m in meshes_spec])
    tri = np.concatenate([m[1] for m in meshes_spec])
    mvo = np.concatenate([[0], np.cumsum([len(m[0]) for m in meshes_spec])]).astype(np.int64)
    mto = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes_spec])]).astype(np.int64)
    return xy, tri, mvo, mto, np.array([m[2] for m in meshes_spec], dtype=float)


def stamps_of(els, N, ground=0):
    rows, cols, vals = [], [], []
    for _, a, b, res in els:
        g = 1.0 / res
        rows += [a, a, b, b]; cols += [a, b, b, a]; vals += [-g, g, -g, g]
    rows += [N - 1, ground]; cols += [ground, N - 1]; vals += [1.0, 1.0]
    return np.array(rows, np.int64), np.array(cols, np.int64), np.array(vals)


# ---- the detector ------------------------------------------------------------------------------------------------------------

def test_the_detector_detects(ctx, switches):
    self_test(ctx, switches)


def test_a_plain_solve_hands_out_no_guarded_block(ctx):
    ctx.pool_guard(1)
    A = R.layered_matrix(2, 40, 30, 4)
    d = ctx.csr_from_scipy(A)
    res = d.solve_spd(np.ones(A.shape[0]), precond="amg")
    d.close()
    assert res.levels >= 2
    assert ctx.pool_guard(0) == dict(allocations=0, violations=0, first=(0, None, 0), last=(None, 0), fill=-1)


# ---- assembly ----------------------------------------------------------------------------------------------------------------

FORCED = [None, "asm_two_pass", "asm_hash"]


def forced(force):
    return {"PADNE_FORCE": force} if force else {}


@pytest.mark.parametrize("force", FORCED)
def test_assembly_of_the_golden_fixtures(ctx, switches, force):
    systems = [H.product_system(H.load_golden(name)) for name in H.golden_names()]

    def fn():
        out = []
        for meshes, sig, stamps, r, n_pot in systems:
            L = solver.assemble_from_arrays(meshes, sig, stamps, n_pot)
            out.append(L.tocsr())
            L.close()
        return out
    three_ways(ctx, switches, fn, forced(force))


@pytest.mark.parametrize("force", FORCED)
@pytest.mark.parametrize("shape", [(128, 64), (129, 127), (257, 100)])
def test_assembly_at_tile_and_chunk_edges(ctx, switches, shape, force):
    nx, ny = shape
    xy, tri = synthetic.jittered_grid(nx, ny, seed=nx * 1000 + ny)
    n = len(xy)
    N = n + 2
    rows, cols, vals = stamps_of([("R", 3, n - 2, 0.5), ("R", n // 2, n, 2.0), ("R", n, 7, 1.0)], N)

    def fn():
        L = ctx.assemble_system(N, xy, tri.astype(np.int32), np.array([0, n], np.int64), np.array([0, len(tri)], np.int64),
                                np.array([2082.5]), rows, cols, vals)
        got = L.to_scipy()
        L.close()
        return got
    three_ways(ctx, switches, fn, forced(force))


@pytest.mark.parametrize("force", FORCED)
def test_assembly_of_the_hub_and_ragged_boards(ctx, switches, force):
    """The boards of test_long_rows_and_ragged_meshes: a hub of 700 resistors, meshes of 1200, 6 and 391 vertices."""
    rng = np.random.default_rng(3)
    parts = [synthetic.jittered_grid(40, 30, seed=1), synthetic.jittered_grid(3, 2, seed=2), synthetic.jittered_grid(17, 23, seed=3)]
    ms = [(p[0], p[1], s) for p, s in zip(parts, (2082.5, 10.0, 500.0))]
    nv = sum(len(m[0]) for m in ms)
    els = [("R", int(p), nv, 1e-3) for p in rng.choice(nv, size=700, replace=False)]
    N = nv + 2
    xy, tri, mvo, mto, sig = flat(ms)
    rows, cols, vals = stamps_of(els, N)
    x = rng.uniform(-1, 1, N)

    def fn():
        L = ctx.assemble_system(N, xy, tri, mvo, mto, sig, rows, cols, vals)
        out = [L.to_scipy(), L.matvec(x)]
        L.close()
        return out
    three_ways(ctx, switches, fn, forced(force))


def test_nearest_vertex(ctx, switches):
    rng = np.random.default_rng(17)
    pts = rng.uniform(-50, 50, (4097, 2))
    q = np.vstack([rng.uniform(-60, 60, (257, 2)), pts[rng.integers(0, len(pts), 7)]])
    three_ways(ctx, switches, lambda: [ctx.nearest_vertex(pts, q), ctx.nearest_vertex(pts[:5], q, with_ties=True)])


# ---- relabel / reduce / vstack -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("force", [None, "relabel_slots", "relabel_lanes"])
def test_relabel_reduce_and_vstack(ctx, switches, force):
    """The matrices of the parity tests: 5000 rows under injective maps (a permutation with dropped rows, a monotone column
    map), explicit zeros; 7000 rows with a row of 1300 entries under maps that only drop -- holes at both ends, scattered, a
    long run; the non-injective maps and the stack of test_relabel_and_vstack_against_scipy."""
    rng = np.random.default_rng(21)
    M = H.random_csr(5000, 5000, 9, 3).tolil()
    M[17, :40] = rng.uniform(-1, 1, 40)
    M[:60, 23] = rng.uniform(-1, 1, (60, 1))
    M = M.tocsr()
    drop = rng.choice(5000, 300, replace=False)
    rmap = rng.permutation(5000).astype(np.int32)
    rmap[drop] = -1
    rmap[rmap >= 0] = np.argsort(np.argsort(rmap[rmap >= 0])).astype(np.int32)
    n_out = int((rmap >= 0).sum())
    cmap = np.arange(5000, dtype=np.int32)
    cmap[drop[:100]] = -1
    cmap[cmap >= 0] = np.arange((cmap >= 0).sum(), dtype=np.int32)
    Mz = M.copy()
    Mz.data[::37] = 0.0
    n = 7000
    W = H.random_csr(n, n, 7, 31).tolil()
    W[33, 100:140] = rng.uniform(-1, 1, 40)
    W[70, 200:1500] = rng.uniform(-1, 1, 1300)
    W[700:703, 0:400] = rng.uniform(-1, 1, (3, 400))
    W = W.tocsr()
    W.sort_indices()
    holes = []
    for dropped in ([0], [n - 1], [0, n - 1], sorted(rng.choice(n, 200, replace=False)), [70, 701, 250, 1499], list(range(500, 600))):
        m = np.arange(n, dtype=np.int32)
        m[list(dropped)] = -1
        m[m >= 0] = np.arange(int((m >= 0).sum()), dtype=np.int32)
        holes.append((m, int((m >= 0).sum())))
    small, bottom = H.random_csr(300, 420, 9, 12), H.random_csr(77, 420, 5, 13)
    rng2 = np.random.default_rng(12)
    rmap2, cmap2 = rng2.integers(-1, 120, 300).astype(np.int32), rng2.integers(-1, 200, 420).astype(np.int32)

    def fn():
        out = []
        for src in (M, Mz):
            d = ctx.csr_from_scipy(src)
            for made in (d.reduce(rmap, n_out, -1.0), d.relabel(rmap, n_out, cmap, int((cmap >= 0).sum()), 2.5)):
                out.append(made.to_scipy())
                made.close()
            d.close()
        d = ctx.csr_from_scipy(W)
        for m, kept in holes:
            host = d.reduce(m, kept, -1.0)
            dm = ctx.to_device(m)
            dev = d.reduce(dm, kept, -1.0)
            out += [host.to_scipy(), dev.to_scipy()]
            dm.free(); host.close(); dev.close()
        d.close()
        d, b = ctx.csr_from_scipy(small), ctx.csr_from_scipy(bottom)
        made = [d.relabel(rmap2, 120, cmap2, 200, -2.0), d.vstack(b)]
        out += [m.to_scipy() for m in made]
        for m in made + [d, b]:
            m.close()
        return out
    three_ways(ctx, switches, fn, forced(force))


# ---- products ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,per_row", [((1, 1), 7), ((255, 255), 7), ((257, 100), 7), ((4097, 4097), 7), ((130, 64), 300)])
def test_products(ctx, switches, shape, per_row):
    rng = np.random.default_rng(shape[0])
    A = H.random_csr(shape[0], shape[1], per_row, seed=shape[0] + 1)
    x, X = rng.uniform(-1, 1, shape[1]), rng.uniform(-1, 1, (shape[1], 8))

    def fn():
        d = ctx.csr_from_scipy(A)
        out = [d.matvec(x), d.matmat8(X), d.residual_norm(x, np.ones(shape[0]))]
        d.close()
        return out
    three_ways(ctx, switches, fn)
    d = ctx.csr_from_scipy(A)
    assert np.array_equal(d.matvec(x), A @ x)
    d.close()


# ---- multigrid setup and solves ------------------------------------------------------------------------------------------------

AMG = {     # the cases of test_amg_vs_reference.py by their names there, and what else the run is sent through
    "a": ("a", {}), "c": ("c", {}), "g": ("g", {}), "f": ("f", {}), "d": ("d", {}), "dx": ("dx", {}),
    "a,transpose_cursors": ("a", {"PADNE_FORCE": "transpose_cursors"}), "a,spgemm_split": ("a", {"PADNE_FORCE": "spgemm_split"}),
    "b,one_stream": ("b", {"PADNE_SETUP_ONE_STREAM": "1"}),
}
_MATRICES = {}


def amg_case(name):
    from test_amg_vs_reference import CASES
    if name not in _MATRICES:
        _MATRICES[name] = CASES[name]["build"]()
    return _MATRICES[name], CASES[name]


def hierarchy(ctx, A, B):
    """Every operator and every decision of the hierarchy of A, and one cycle on the columns of B."""
    d = ctx.csr_from_scipy(A)
    try:
        out = [d.amg_apply(np.ones(A.shape[0]))]
        shapes = d.amg_shapes()
        out.append([[s[w] for w in ("A", "P", "R") if w in s] for s in shapes])
        for lvl, s in enumerate(shapes):
            out += [d.amg_level(lvl, w) for w in ("A", "P", "R") if w in s]
            if lvl + 1 < len(shapes):
                out += [d.amg_state(lvl, "AGG"), d.amg_state(lvl, "ROOT"), d.amg_state(lvl, "SCALARS")]
        out += [d.amg_apply(B[:, j]) for j in range(B.shape[1])]
    finally:
        d.close()
    return out, shapes


@pytest.mark.parametrize("name", list(AMG))
def test_multigrid_setup_and_cycle(ctx, switches, name):
    from test_amg_vs_reference import right_hand_sides
    A, case = amg_case(AMG[name][0])
    n = A.shape[0]
    B = np.ascontiguousarray(right_hand_sides(n, n // 2)[:, [0, 9, 13]])
    seen = {}

    def fn():
        out, seen["shapes"] = hierarchy(ctx, A, B)
        return out
    three_ways(ctx, switches, fn, {"PADNE_AMG_KEEP": "1", **case["env"], **AMG[name][1]})
    assert len(seen["shapes"]) >= case["min_levels"]
    if case.get("windowed") or name == "dx":
        assert n >= 65536 and int(np.diff(A.indptr).max()) <= 13            # the size the x-window plan engages at
    if case.get("long_rows"):
        assert any(s["A"][2] >= 24 * s["A"][0] for s in seen["shapes"][:-1])


def solve_fields(res):
    return [res.x, res.iterations, res.restarts, res.rel_residual, res.abs_residual, res.status, res.levels, res.operator_complexity,
            res.precond_fallbacks]


@pytest.mark.parametrize("precond,env", [("jacobi", {}), ("amg", {}), ("amg", {"PADNE_FORCE": "xhist_small"})])
def test_pcg_from_zero_and_from_a_guess(ctx, switches, precond, env):
    A, _ = amg_case("b")
    n = A.shape[0]
    b = np.random.default_rng(2).uniform(-1, 1, n)
    guess = np.random.default_rng(3).uniform(-1e-3, 1e-3, n)

    def fn():
        d = ctx.csr_from_scipy(A)
        cold = d.solve_spd(b, rtol=1e-12, precond=precond)
        warm = d.solve_spd(b, rtol=1e-12, precond=precond, x0=guess)
        d.close()
        return solve_fields(cold) + solve_fields(warm)
    three_ways(ctx, switches, fn, env)


_LAYERED = {}


def layered_block(k):
    """test_lockstep_widths_of_a_block: two layers of 60 x 60 vertices with vias, k right-hand sides."""
    if "L" not in _LAYERED:
        sysm = synthetic.layered_system(2, 60, 60, via_lattice=6)
        els = [("R", int(a), int(b), float(rr)) for a, b, rr in zip(*sysm.resistors)]
        _LAYERED["L"] = (sysm, O.assemble_system([(m[0], m[1], m[2]) for m in sysm.meshes], 0, els, sysm.ground)[0])
    sysm, Lo = _LAYERED["L"]
    src, snk = synthetic.multi_rhs_pairs(sysm, k, seed=k)
    Rk = np.zeros((Lo.shape[0], k))
    Rk[src, np.arange(k)] += 1.0 + np.arange(k)
    Rk[snk, np.arange(k)] -= 1.0 + np.arange(k)
    return Lo, Rk


def info_fields(info):
    return [info.ground_node_current, info.residual_norm, info.iterations, info.rel_residual, info.residual_norms]


@pytest.mark.parametrize("k", [1, 3, 8, 9, 17])
def test_lockstep_blocks(ctx, switches, k):
    Lo, Rk = layered_block(k)

    def fn():
        V, info = solver.solve_system(Lo, Rk)
        return [V] + info_fields(info)
    three_ways(ctx, switches, fn)


@pytest.mark.parametrize("env", [{}, {"PADNE_GJ_VECTOR": "1"}])
def test_dense_inverse(ctx, switches, env):
    """A system below PADNE_AMG_COARSE_N: the hierarchy is the dense inverse alone, on the matrix cores and by the vector kernel."""
    sysm = synthetic.layered_system(2, 36, 28, via_lattice=4)
    els = [("R", int(a), int(b), float(r)) for a, b, r in zip(*sysm.resistors)]
    Lo, ro = O.assemble_system([(m[0], m[1], m[2]) for m in sysm.meshes], 0, els, 0)
    n = sysm.n_vertices
    A = (-Lo[1:n, 1:n]).tocsr()
    b = np.random.default_rng(4).uniform(-1, 1, A.shape[0])
    assert 32 < A.shape[0] <= 2048
    levels = []

    def fn():
        d = ctx.csr_from_scipy(A)
        first = d.solve_spd(b, precond="amg", rtol=1e-12)
        second = d.solve_spd(2.0 * b, precond="amg", rtol=1e-12, x0=first.x)
        z = d.amg_apply(b)
        d.close()
        levels.append(first.levels)
        return solve_fields(first) + solve_fields(second) + [z]
    three_ways(ctx, switches, fn, env)
    assert levels == [1, 1, 1]


# ---- the KKT plan --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["voltage_source", "regulator", "two_layer_via"])
def test_solve_system_on_the_golden_fixtures(ctx, switches, name):
    meshes, sig, stamps, r, n_pot = H.product_system(H.load_golden(name))

    def fn():
        L = solver.assemble_from_arrays(meshes, sig, stamps, n_pot)
        v, info = solver.solve_system(L, r)
        L.close()
        return [v] + info_fields(info)
    three_ways(ctx, switches, fn)


@pytest.mark.parametrize("name", ["voltage_source", "regulator"])
def test_a_block_of_nine_columns_with_known_parts(ctx, switches, name):
    """Nine load cases that differ in their current injections and in the voltages of their sources (the known part of the
    potentials differs from column to column), one of them all zero."""
    meshes, sig, stamps, r, n_pot = H.product_system(H.load_golden(name))
    layout = reduction.KKTLayout(size=len(r), n_potential=n_pot, constraints=list(stamps.constraints))
    k = 9
    Rk = np.repeat(np.asarray(r, dtype=np.float64)[:, None], k, axis=1)
    sources = [c for c in layout.constraints if c.n >= 0]
    assert sources
    for j in range(1, k):
        Rk[:n_pot, j] *= 1.0 + 0.3 * j
        for c in sources:
            Rk[c.index, j] = r[c.index] * (1.0 + 0.125 * j)
    Rk[:, 3] = 0.0

    def fn():
        L = solver.assemble_from_arrays(meshes, sig, stamps, n_pot)
        V, info = solver.solve_system(L, Rk)
        L.close()
        return [V] + info_fields(info)
    three_ways(ctx, switches, fn)


def test_the_strip_order(ctx, switches):
    """test_strip_numbering_on_the_device_is_the_hosts_permutation at a third of its size: two shuffled Delaunay meshes, a
    voltage source across them, an internal node; the reduced matrix of the plan in the device's strip order and the solve."""
    from test_gpu_parity import delaunay_mesh
    m1, m2 = delaunay_mesh(3000, seed=5, hole=True), delaunay_mesh(1700, seed=6, hole=False)
    meshes = [mesh.Mesh(*m1), mesh.Mesh(m2[0] * 0.7 + 3.0, m2[1])]
    n1, n2 = len(meshes[0].points), len(meshes[1].points)
    nv = n1 + n2
    n_pot = nv + 1
    N = n_pot + 2
    stamps = solver.StampList(N)
    r = np.zeros(N)
    for a in (17, n1 + 40, n1 + 333):
        g = 1 / 0.25
        stamps.add(a, a, -g); stamps.add(a, nv, g); stamps.add(nv, nv, -g); stamps.add(nv, a, g)
    iv, p_, n_ = n_pot, 1321, n1 + 1234
    stamps.add(iv, p_, 1.0); stamps.add(iv, n_, -1.0); stamps.add(p_, iv, 1.0); stamps.add(n_, iv, -1.0)
    r[iv] = 0.5
    stamps.constraints.append(reduction.Constraint(index=iv, p=p_, n=n_, value=0.5))
    r[100] += 1.0
    r[n1 + 7] -= 1.0
    solver.setup_ground_node(3, stamps, r)

    def fn():
        L = solver.assemble_from_arrays(meshes, [2082.5, 1041.25], stamps, n_pot)
        red = reduction.build_reduction(L.layout)
        plan = _hip.KktPlan(L.dev, n_pot, red.elim, red.tied, red.n_free, strip_order=True)
        out = [plan.reduced_matrix().to_scipy()]
        plan.close()
        v, info = solver.solve_system(L, r)
        L.close()
        return out + [v] + info_fields(info)
    three_ways(ctx, switches, fn)


# ---- post-processing -------------------------------------------------------------------------------------------------------------

BOARDS = ["problem_many_meshes", "problem_mixed"]
_SYSTEMS = {}


def board(name):
    """(system, meshes, disconnected meshes by layer) of a golden board, built once (the NodeIDs are made when it is built)."""
    from test_currents import board_of
    if name not in _SYSTEMS:
        system = S.problem_system(name)
        _SYSTEMS[name] = (system, *board_of(system, name))
    return _SYSTEMS[name]


def objectives_of(system):
    from test_sensitivity import fixture_objectives
    return fixture_objectives(system.flat)[:3]


def post_currents(name):
    from test_currents import random_cuts
    system, meshes, disc = board(name)
    cuts = random_cuts(system)
    return lambda: solver.solve_meshed_currents(system.prob, meshes, system.layer_of, cuts, disconnected_meshes_by_layer=disc)


def post_load_case_currents(name):
    from test_currents import random_cuts
    from test_load_cases import block_cases
    system, meshes, disc = board(name)
    cuts, cases = random_cuts(system), block_cases(system.flat, 9, seed=9)
    return lambda: solver.solve_meshed_load_case_currents(system.prob, meshes, system.layer_of, cases, cuts, per_case_fields=True,
                                                          disconnected_meshes_by_layer=disc)


def post_sensitivities(name):
    system, meshes, disc = board(name)
    objectives = objectives_of(system)
    return lambda: solver.solve_meshed_sensitivities(system.prob, meshes, system.layer_of, objectives,
                                                     disconnected_meshes_by_layer=disc)


def post_error(name):
    system, meshes, disc = board(name)
    return lambda: solver.solve_meshed_error(system.prob, meshes, system.layer_of, tolerance=0.05, disconnected_meshes_by_layer=disc)


def post_goal_error(name):
    """Three objectives: four fields (the solution and three adjoints) through the goal kernels."""
    system, meshes, disc = board(name)
    objectives = objectives_of(system)
    assert len(objectives) == 3
    return lambda: solver.solve_meshed_goal_error(system.prob, meshes, system.layer_of, objectives, tolerance=0.05,
                                                  disconnected_meshes_by_layer=disc)


def post_sampling(name):
    system, meshes, disc = board(name)

    def fn():
        sol, _rep = solver.solve_meshed_currents(system.prob, meshes, system.layer_of, [], disconnected_meshes_by_layer=disc)
        out = []
        with solver.FieldSampler(sol) as fs:
            for li, lay in enumerate(system.prob.layers):
                pts = [np.asarray(m.points) for m, l in zip(meshes, system.layer_of) if l == li]
                if not pts:
                    continue
                pts = np.concatenate(pts)
                lo, hi = pts.min(axis=0), pts.max(axis=0)
                q = np.concatenate([np.random.default_rng(li).uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (1000, 2)), pts[:300]])
                out.append(fs.points(lay, q))
                if li == 0:
                    out.append(fs.raster(lay, tuple(lo), tuple((hi - lo) / np.array([97.0, 61.0])), 97, 61))
        return out
    return fn


def post_thermal(name):
    system, meshes, disc = board(name)
    model = solver.ThermalModel(film=1e-5)
    return lambda: solver.solve_meshed_thermal(system.prob, meshes, system.layer_of, model, disconnected_meshes_by_layer=disc)


def post_coupled(name):
    system, meshes, disc = board(name)
    model = solver.ElectroThermalModel(thermal=solver.ThermalModel(film=1e-5, ambient=25.0), max_rounds=2, tolerance=1e-9)

    def fn():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")           # two rounds do not converge to 1e-9 K: that is the driver
            return solver.solve_meshed_electrothermal(system.prob, meshes, system.layer_of, model, disconnected_meshes_by_layer=disc)
    return fn


def post_transient(name):
    """Three steps, two scenarios (sources on / off), one probe."""
    system, meshes, disc = board(name)
    model = solver.TransientModel(thermal=solver.ThermalModel(film=1e-3), areal_capacity=3e-3, initial=(None, 0))
    probes = [system.prob.networks[0].connections[0].node_id]
    schedule = [solver.Segment(0.45, 3, (0, None))]
    return lambda: solver.solve_meshed_thermal_transient(system.prob, meshes, system.layer_of, model, schedule, probes=probes,
                                                         keep="segments", disconnected_meshes_by_layer=disc)


POST = dict(currents=post_currents, load_case_currents=post_load_case_currents, sensitivities=post_sensitivities, error=post_error,
            goal_error=post_goal_error, sampling=post_sampling, thermal=post_thermal, coupled=post_coupled, transient=post_transient)


@pytest.mark.parametrize("name", BOARDS)
@pytest.mark.parametrize("what", list(POST))
def test_post_processing(ctx, switches, what, name):
    three_ways(ctx, switches, POST[what](name))


def test_one_refine_round(ctx, switches):
    """The smallest mesh set (the square of two faces) and the grid, all faces and a random 15 % of them flagged."""
    from test_refine_host import mesh_set, random_flags
    sets = [mesh_set("square"), mesh_set("grid")]

    def fn():
        out = []
        for ms in sets:
            for flags in ([np.ones(len(t), dtype=bool) for _, t in ms], random_flags(ms, 5)):
                out.append(solver.refine_meshes([mesh.Mesh(p, t) for p, t in ms], flags))
        return out
    three_ways(ctx, switches, fn)


def test_goal_error_of_four_fields_on_four_meshes(ctx, switches):
    from test_goal_error import four_meshes, smooth_fields
    xy, local, _tri, _face_mesh, voff, toff, sigma = four_meshes()
    fields = smooth_fields(xy, 4)
    three_ways(ctx, switches, lambda: [ctx.goal_error(xy, local, voff, toff, sigma, fields),
                                       ctx.error_estimate(xy, local, voff, toff, sigma, fields[0])])


# ---- order dependence ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fill", [None, "ff"])
def test_a_small_solve_after_a_large_one_is_the_solve_on_a_fresh_context(switches, fill):
    """What a long-lived process sees and no other test does: on ONE context the 144 k-unknown case d, then case a, then the
    nine-column KKT block, then case a again -- blocks and workspace of the large solves are reused by the small ones.  The two
    case-a results are the same bits, and the bits of case a on a context that has done nothing else."""
    Ad, _ = amg_case("d")
    Aa, _ = amg_case("a")
    bd = np.random.default_rng(7).uniform(-1, 1, Ad.shape[0])
    ba = np.random.default_rng(8).uniform(-1, 1, Aa.shape[0])
    meshes, sig, stamps, r, n_pot = H.product_system(H.load_golden("voltage_source"))
    Rk = np.repeat(np.asarray(r, dtype=np.float64)[:, None], 9, axis=1) * (1.0 + 0.25 * np.arange(9))

    def solve(c, A, b):
        d = c.csr_from_scipy(A)
        try:
            return leaves(solve_fields(d.solve_spd(b, precond="amg", rtol=1e-12)))
        finally:
            d.close()

    switches.set("PADNE_AMG_COARSE_N", "64")
    if fill is not None:
        switches.set("PADNE_POOL_GUARD", fill)
    shared = fresh = None
    before = solver.get_context()
    try:
        shared = _hip.Context(0)
        large = solve(shared, Ad, bd)
        first = solve(shared, Aa, ba)
        solver.set_context(shared)
        L = solver.assemble_from_arrays(meshes, sig, stamps, n_pot)
        V, info = solver.solve_system(L, Rk)
        L.close()
        solver.set_context(before)
        again = solve(shared, Aa, ba)
        stats = shared.pool_guard(0)
        fresh = _hip.Context(0)
        alone = solve(fresh, Aa, ba)
        stats_fresh = fresh.pool_guard(0)
    finally:
        solver.set_context(before)
        for c in (shared, fresh):
            if c is not None:
                c.close()
        switches.unset("PADNE_POOL_GUARD")
        switches.unset("PADNE_AMG_COARSE_N")
    assert large and info.residual_norm < 1e-9 and V.shape == Rk.shape
    assert first == again, "case a differs after the KKT block on the same context"
    assert first == alone, "case a on the shared context differs from case a on a fresh one"
    assert stats["violations"] == 0 and stats_fresh["violations"] == 0, (stats, stats_fresh)
    assert (stats["allocations"] > 0) == (fill is not None) and (stats_fresh["allocations"] > 0) == (fill is not None)

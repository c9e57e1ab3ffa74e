"""The row-partitioned solver -- halo exchange, hierarchy over all ranks, its cycle, the CG loops on it -- against host references.

W ranks are W threads of this process, each with its own context on GPU 0 and a member of one _hip.LocalTeam (as
test_gpu_parity.run_team).  The threads live as long as their team and serve callables from a queue (RankTeam), so that the
main thread can drive a host PCG whose preconditioner is a collective device call.  What the device holds is read through
the probes of include/padne_hip_probe.h (padne_test_halo_exchange, padne_test_amg_apply_dist, padne_test_amg_state with
EXPORT / HALO, padne_test_amg_tail) and put together by tests/dist_ref.py: slot (p, e) of a rank's piece is global column
off_p + exports[p][e].  Nothing is compared with another device path.

a  halo exchange   exact (data movement): after one exchange of x_q[i] = q + ((i + 131 t) mod 2^20) 2^-20 -- distinct everywhere,
                   exact in float too -- the first n_export_p slots of EVERY segment on EVERY rank are dist_ref.halo_expected bit
                   for bit, the owned part is unchanged; double and float, peer stores and PADNE_NO_P2P=1; 40 exchanges back to
                   back (the mailbox ring of four entries wraps ten times).  Plans: the layer partition of 8 x 40 x 30 on 2, 3, 4
                   ranks (3: 2 / 3 / 3 layers, unequal n_owned and n_export), the strip partition of one layer on 3 ranks, and
                   a hand-built plan of three meshes joined by ONE resistor: ranks 0 and 1 export one value, rank 2 none (m = 1).
b  hierarchy       8 x 40 x 30 under PADNE_AMG_KEEP=1, PADNE_AMG_GATHER_N=200, PADNE_AMG_COARSE_N=64.  Fine operator: the stacked
                   A_0 against the oracle's reduced matrix permuted by owned_reduced_global.  SCALARS the same bits and HALO m the
                   same on all ranks.  Per rank on the owned block: check_aggregation on AGG / ROOT, agg.max() + 1 == columns
                   of P^q, R^q == (P^q)^T, and P^q within the envelope of amg_ref.prolongator(strength(block), agg): called on
                   the BLOCK, whose omega = 1.5 / min(lambda_F(block), lambda(block)) is the device's (filtered bound of
                   the block capped by the block's plain bound).  The block is dist_ref.owned_block: A_l^q[:, :n_q] with the
                   dropped couplings lumped onto the diagonal, as block_fill of csrc/amg.hip specifies it -- with the bare
                   A_l^q[:, :n_q] the vias across a rank boundary (16 resistors on one vertex pair) shift a_ii by up to 18 %
                   and a dozen strength decisions per rank with it; the device is right by its specification.  Global: check_smoothing with the plain bound of the stacked
                   operator and, below level 0, eigsh of it; amg_ref.galerkin(A_l, blockdiag P_l) against the stacked A_{l+1}
                   (the check that sees a remote row of P in the wrong slot).  Tail: padne_test_amg_tail == the stacked gather
                   level bit for bit on every rank; its own levels through check_hierarchy of test_amg_vs_reference.py.
c  cycle           the 16 right-hand sides of test_amg_vs_reference.right_hand_sides (special row: an exported vertex of rank 1)
                   + unit vectors at the first and last owned row of every rank.  Reference: amg_ref.cycle_envelope / cycle on
                   the checked global levels, then the tail's levels, then dense_ref's inverse of the tail's coarsest operator.
                   PADNE_AMG_F64=1: every entry within the envelope.  Single precision: per vector at most F32_FACTOR (8.0, of
                   test_amg_vs_reference.py) times the plain float32 host evaluation, under PADNE_AMG_W none / fine / default,
                   each also with PADNE_AMG_EXCHANGE_ALL=1, PADNE_NO_P2P=1, PADNE_NO_SPLIT=1.
   large           2 x 300 x 240 on 2 ranks (72 k rows each: csr_build_xw_plan and build_w_operator's wide plan ask n_rows >=
                   65536 of a matrix that is no hierarchy operator -- the partitioned fine level qualifies): Galerkin and cycle.
d  CG              solve_spd_dev(max_iter=k, rtol=NEVER) on every rank, the reassembled iterate against pcg_ref with `calibrated` /
                   `check_iterate` of test_pcg_vs_reference.py (bound 100 max(d_host(k), 2^-53)): Jacobi (longdouble Jacobi;
                   k = 1, 2, 5, 12, 40); the global hierarchy (M = the device's partitioned cycle through the probe, in the
                   loop's units; default with the r32_unit calibration, and PADNE_AMG_F64=1); block-Jacobi (M = the per-rank
                   one-GPU cycles of A_block side by side); multigrid k = 1, 2, 3, 4, 5, 7, 8, 9, 17.  Every rank reports
                   iterations == k and the same status.  Stopping rule per form at rtol 1e-6 and 1e-9 through check_stop.

A rank that raises aborts its team (its peers' collectives return E_COMM), every queue wait and join has a timeout, nothing is
retried.

Measured on an MI355X (pytest -s prints these lines):
  halo            all ten plan / transport pairs: 40 exchanges exact.  layers3: n_owned 2399 / 3600 / 3600, n_export 60 / 120 / 60,
                  m 120; strips3: 399 / 400 / 400, 40 / 80 / 40, m 80; isolated: 11 / 12 / 12, 1 / 1 / 0, m 1 (the planner yields it).
  level shapes    W = 2: 9599 > 1371 > 164 > 25;  W = 3: 9599 > 1358 > 155 > 23;  W = 4: 9599 > 1366 > 157 > 22 -- two partitioned
                  levels, the gather level, a tail of two levels (asserted).  Coarse levels, W = 3: n_q 346 / 504 / 508, n_export
                  114 / 188 / 108 (m 188); gather level n_q 41 / 57 / 57, n_export 41 / 57 / 45: padded segments on every level.
  fine operator   the stacked A_0 IS the oracle's reduced matrix, bit for bit, for W = 2, 3, 4 (asserted; no envelope needed).
  envelopes       P at most 0.18, stacked A_c at most 0.61 of their envelopes (tail: 0.04 / 0.49); stability 1.1 lambda_1 / lambda_max
                  1.12 .. 1.16.  Double-precision cycle: at most 6.7e-5 of its envelope (the envelope at most 2.3e-8 of max |z|).
  f32 ratios      worst error / plain float32 error (bar F32_FACTOR = 8.0): W = 2: 2.16 / 2.16 / 2.15 for PADNE_AMG_W none / fine /
                  default; W = 3: 1.83 / 1.82 / 1.77; W = 4: 4.50 / 4.50 / 4.51.  PADNE_AMG_EXCHANGE_ALL, PADNE_NO_P2P and
                  PADNE_NO_SPLIT give the same figures to the digits printed (4.51 the worst of each).
  large           143999 > 19808 > 2025 (72 k rows per rank, gather level 9902 / 9906, m 113); A_c 0.62 of its envelope, f64 cycle
                  1.6e-6 of its envelope, f32 ratio 1.14; 5.5 s (case d of test_amg_vs_reference.py was not timed beside it); the
                  other 76 tests of this module take 7.6 s together.
  CG              device deviation | bound, the world closest to its bound:
                    jacobi      k = 1: 5.0e-17 | 1.1e-14   2: 1.8e-16 | 1.2e-14   5: 2.3e-16 | 1.1e-14   12: 3.1e-16 | 3.1e-14   40: 3.9e-16 | 3.6e-14
                    global      1: 7.2e-16 | 1.7e-06   2: 9.6e-09 | 7.6e-06   3: 2.9e-08 | 3.8e-06   4: 2.3e-08 | 1.0e-06   5: 8.8e-09 | 6.4e-07
                                7: 1.2e-09 | 2.7e-07   8: 5.7e-10 | 1.1e-07   9: 8.4e-11 | 8.2e-09   17: 8.3e-15 | 5.2e-13
                    global_f64  1: 9.7e-16 | 9.7e-14   2: 2.6e-15 | 5.4e-14   3: 8.9e-16 | 9.2e-14   4 .. 17: at most 3.2e-15 | 1.7e-13 or more
                    block       1: 1.7e-08 | 1.7e-06   2: 1.1e-08 | 9.4e-07   3: 1.1e-08 | 8.5e-07   4: 7.5e-09 | 8.0e-07   5: 7.7e-09 | 5.4e-07
                                7: 3.9e-08 | 3.2e-06   8: 2.6e-07 | 1.8e-05   9: 1.1e-06 | 7.6e-05   17: 2.5e-06 | 1.1e-04
                  stopping rule: e.g. W = 2 global 12 / 17 iterations at rtol 1e-6 / 1e-9, Jacobi 268 / 333, block 26 / 41.

Shown able to fail, in a scratch library (one perturbation each, not committed; the module's tests named were run):
  * halo_unpack_kernel reading cell k + 1 (wrapped inside the segment so that the read stays in bounds): the halo test of
    layers3 / peer stores red in exchange 0, rank 0, slot 0 (isolated, m = 1, wraps onto itself; the all-gather form has no unpack);
  * lam = std::max(...) over the ranks removed: the hierarchy test red for W = 2, 3, 4 (SCALARS differ between the ranks:
    2.016 / 2.184 / 2.006 ..);
  * one rank's share left out of team_allreduce: all four CG iterate forms red at k = 1 or 2 (6e-2 against bounds of 1e-6 .. 1e-14);
  * slot_to_global offset by one rank: applied to the copy the cycle reads (tail_slot_idx, clamped into the gathered range):
    the single-precision cycle red for every W and every PADNE_AMG_W form.  The same offset in the columns tail_pack writes
    was NOT run on the device: it makes the gathered operator unsymmetric with columns that may leave its range, and
    whether the setup's loops end on such a matrix is nothing to try out on a GPU others use.  What would see it is the
    comparison of padne_test_amg_tail with the stacked gather level (bit for bit), and tests/test_dist_ref_host.py shows on
    the host that stack() under another slot map is another matrix.
"""
import functools
import queue
import threading
import time
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import amg_ref as R
import dist_ref as DR
from test_amg_vs_reference import F32_FACTOR, check_hierarchy, norm2, reference_cycle, right_hand_sides
from test_pcg_vs_reference import NEVER, calibrated, check_iterate, check_stop, in_units
from padne_amd import _hip, distributed, synthetic

pytestmark = pytest.mark.gpu

LD = np.longdouble
WORLDS = (2, 3, 4)
WAIT = 300          # seconds the main thread waits for a rank's answer
IDLE = 900          # seconds a rank waits for its next command (the main thread may be in a host reference run)


# ---- the team: one long-lived thread per rank ---------------------------------------------------------------------------

class RankTeam:
    """`setup(rank, ctx, team) -> state` runs on every rank's thread; afterwards run(fn) has every rank (or the listed ones)
    evaluate fn(rank, state) and returns the answers in rank order.  A rank that raises aborts the team and ends the test."""

    def __init__(self, world, setup):
        self.world = world
        self.team = _hip.LocalTeam(world)
        self.cmd = [queue.Queue() for _ in range(world)]
        self.ans = [queue.Queue() for _ in range(world)]
        self.errors = []
        self.threads = [threading.Thread(target=self._main, args=(r, setup), daemon=True) for r in range(world)]
        for t in self.threads:
            t.start()
        self._collect(range(world))

    def _main(self, rank, setup):
        try:
            c = _hip.Context(0)
            state = setup(rank, c, self.team)
            self.ans[rank].put((True, None))
            while True:
                fn = self.cmd[rank].get(timeout=IDLE)
                if fn is None:
                    return
                self.ans[rank].put((True, fn(rank, state)))
        except BaseException as exc:                              # wake the peers: they wait for this rank in a collective
            self.errors.append((rank, exc))
            self.team.abort()
            self.ans[rank].put((False, exc))

    def _collect(self, ranks):
        out = []
        for r in ranks:
            try:
                ok, val = self.ans[r].get(timeout=WAIT)
            except queue.Empty:
                self.team.abort()
                raise AssertionError(f"rank {r} did not answer within {WAIT} s; errors so far: {self.errors}")
            if not ok:
                # (the peers fail with E_COMM behind it: the first error is the cause)
                raise AssertionError(f"rank {r} failed: {val!r}; all errors: {self.errors}")
            out.append(val)
        return out

    def run(self, fn, ranks=None):
        ranks = list(range(self.world)) if ranks is None else list(ranks)
        assert not self.errors, self.errors
        for r in ranks:
            self.cmd[r].put(fn)
        return self._collect(ranks)

    def close(self):
        for q in self.cmd:
            q.put(None)
        for t in self.threads:
            t.join(timeout=60)
        alive = [i for i, t in enumerate(self.threads) if t.is_alive()]
        if alive:
            self.team.abort()
        assert not alive, f"ranks {alive} did not end"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            self.close()
        else:                                                     # a failed test: end the ranks, keep the first error
            self.team.abort()
            for q in self.cmd:
                q.put(None)
            for t in self.threads:
                t.join(timeout=60)
        return False


def halo_only(plans):
    """setup of a team whose ranks only carry a halo plan (no matrix)."""
    def setup(rank, c, team):
        team.join(c, rank)
        p = plans[rank]
        c.set_halo(p.n_owned_reduced, p.m, p.export_reduced)
        return SimpleNamespace(ctx=c, plan=p)
    return setup


def solver_setup(sysm, world, block=False):
    def setup(rank, c, team):
        plan = distributed.build_layer_partition(sysm, rank, world)
        ds = distributed.DistributedSolver(c, plan, team=team, block_preconditioner=block)
        return SimpleNamespace(ctx=c, plan=plan, ds=ds)
    return setup


# the four commands the tests use
def cmd_exchange(xs, as_float):
    return lambda rank, st: st.ctx.halo_exchange_probe(xs[rank], st.plan.m, st.plan.world, as_float)


def cmd_cycle(parts):
    return lambda rank, st: st.ds.A.amg_apply_dist(parts[rank])


def cmd_solve(precond, max_iter, rtol):
    def fn(rank, st):
        res = st.ds.A.solve_spd_dev(st.ds.b, st.ds.x, max_iter=max_iter, rtol=rtol, raise_on_fail=False, precond=precond)
        res.x = st.ds.x.numpy()
        return res
    return fn


def cmd_fetch_level(level):
    """What rank q holds of partitioned level `level`: its rows of A, P and R (the gather level has no P), the probe's arrays."""
    def fn(rank, st):
        A = st.ds.A
        shapes = A.amg_shapes()
        out = SimpleNamespace(n_levels=len(shapes), A=A.amg_level(level, "A"), scalars=A.amg_state(level, "SCALARS"),
                              halo=A.amg_state(level, "HALO"), export=A.amg_state(level, "EXPORT"), P=None, R=None, agg=None, root=None)
        if "P" in shapes[level]:
            out.P, out.R = A.amg_level(level, "P"), A.amg_level(level, "R")
            try:
                out.agg, out.root = A.amg_state(level, "AGG"), A.amg_state(level, "ROOT")
            except ValueError:
                pass                                              # (not kept: no PADNE_AMG_KEEP)
        return out
    return fn


def cmd_fetch_tail(rank, st):
    """The gathered operator and the raw levels of its own hierarchy: [(A, P, scalars)], P = None on the coarsest."""
    t = st.ds.A.amg_tail()
    shapes = t.amg_shapes()
    lv = []
    for l, s in enumerate(shapes):
        lv.append((t.amg_level(l, "A"), t.amg_level(l, "P") if "P" in s else None, t.amg_state(l, "SCALARS")))
    return SimpleNamespace(A=t.to_scipy(), levels=lv)


# ---- systems ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layered(nl, nx, ny, lattice):
    return synthetic.layered_system(nl, nx, ny, via_lattice=lattice)


@functools.lru_cache(maxsize=None)
def oracle_system(nl, nx, ny, lattice):
    """(A, b) of the oracle: vertex 0 grounded and removed; unknown g of the partition is row g - 1."""
    from test_pcg_vs_reference import layered_spd
    return layered_spd(nl, nx, ny, lattice)


def same_bits(a, b):
    a, b = R.csr(a), R.csr(b)
    return a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and \
        np.array_equal(a.data.view(np.int64), b.data.view(np.int64))


# ---- a. the halo exchange -----------------------------------------------------------------------------------------------

def isolated_piece_plans():
    """Three 4 x 3 meshes, one per rank, and ONE resistor between mesh 0 and mesh 1: ranks 0 and 1 export one value each,
    rank 2 -- an isolated piece -- none, m = 1 (build_partition with the owner array written by hand)."""
    meshes = [synthetic.jittered_grid(4, 3, seed=s) + (1.0, s) for s in range(3)]
    n = 36
    coo = distributed.resistor_stamps(np.array([5]), np.array([12 + 7]), np.array([0.1]))
    owner = np.repeat(np.arange(3, dtype=np.int32), 12)
    return [distributed.build_partition(meshes, n, coo, np.zeros(n), 0, owner, r, 3) for r in range(3)]


def halo_plans(name):
    if name == "isolated":
        return isolated_piece_plans()
    if name == "strips3":
        sysm, world = layered(1, 40, 30, 0), 3
    else:
        sysm, world = layered(8, 40, 30, 5), int(name[-1])
    return [distributed.build_layer_partition(sysm, r, world) for r in range(world)]


def test_the_planner_yields_a_rank_without_exports():
    plans = isolated_piece_plans()
    assert [p.m for p in plans] == [1, 1, 1] and [len(p.export_reduced) for p in plans] == [1, 1, 0]


@pytest.mark.parametrize("p2p", ["peer_stores", "all_gather"])
@pytest.mark.parametrize("name", ["layers2", "layers3", "layers4", "strips3", "isolated"])
def test_halo_exchange_moves_the_exported_values_and_nothing_else(switches, name, p2p):
    if p2p == "all_gather":
        switches.set("PADNE_NO_P2P", "1")
    plans = halo_plans(name)
    world, m = len(plans), plans[0].m
    exports = [np.asarray(p.export_reduced, dtype=np.int64) for p in plans]
    sizes = [p.n_owned_reduced for p in plans]
    assert all(p.m == m for p in plans) and m == max(len(e) for e in exports) and max(sizes) < 2 ** 20
    if name == "layers3":
        assert len(set(sizes)) > 1 and len({len(e) for e in exports}) > 1, "2 / 3 / 3 layers: unequal ranks"
        assert min(len(e) for e in exports) < m, "a padded segment"
    if name == "strips3":
        assert all(p.partial_mesh for p in plans)
    with RankTeam(world, halo_only(plans)) as team:
        for t in range(40):
            as_float = bool(t & 1)
            xs = [q + ((np.arange(sizes[q]) + 131 * t) % 2 ** 20) * 2.0 ** -20 for q in range(world)]
            want, defined = DR.halo_expected(xs, exports, m)
            got = team.run(cmd_exchange(xs, as_float))
            for q in range(world):
                assert got[q].shape == (sizes[q] + world * m,)
                assert np.array_equal(got[q][:sizes[q]], xs[q]), f"exchange {t}: the owned part of rank {q} changed"
                area = got[q][sizes[q]:]
                bad = np.flatnonzero(defined & ~(area == want))
                assert not len(bad), (f"exchange {t} ({'float' if as_float else 'double'}), rank {q}: slots {bad[:6]} hold "
                                      f"{area[bad[:6]]}, expected {want[bad[:6]]}")
    print(f"HALO {name} {p2p}: world {world}, n_owned {sizes}, n_export {[len(e) for e in exports]}, m {m}: 40 exchanges exact")


def test_a_rank_that_raises_ends_the_team_and_the_test():
    """The harness itself: rank 1 raises instead of joining an exchange; rank 0, waiting in the collective, is woken by the
    abort (E_COMM), run() raises with the cause, and both threads have ended."""
    plans = halo_plans("layers2")
    team = RankTeam(2, halo_only(plans))
    xs = [np.zeros(p.n_owned_reduced) for p in plans]

    def fn(rank, st):
        if rank == 1:
            raise RuntimeError("rank 1 gives up")
        return st.ctx.halo_exchange_probe(xs[rank], st.plan.m, 2, False)
    t0 = time.perf_counter()
    with pytest.raises(AssertionError, match="failed"):
        team.run(fn)
    for t in team.threads:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in team.threads) and time.perf_counter() - t0 < 60
    kinds = {r: type(e) for r, e in team.errors}
    assert kinds[1] is RuntimeError and (0 not in kinds or (kinds[0] is _hip.HipError and dict(team.errors)[0].code == _hip.E_COMM))


# ---- b. the hierarchy ---------------------------------------------------------------------------------------------------

SMALL = (8, 40, 30, 5)
SMALL_ENV = {"PADNE_AMG_KEEP": "1", "PADNE_AMG_GATHER_N": "200", "PADNE_AMG_COARSE_N": "64"}
LARGE = (2, 300, 240, 6)
LARGE_ENV = {"PADNE_AMG_KEEP": "1"}


def fetch_hierarchy(team):
    """Builds the hierarchy (one collective cycle of zeros) and brings every partitioned level and the tail to the host:
    (levels[l][q], tails[q])."""
    team.run(lambda rank, st: st.ds.A.amg_apply_dist(np.zeros(st.ds.n_owned)))
    first = team.run(cmd_fetch_level(0))
    nl = first[0].n_levels
    assert all(f.n_levels == nl for f in first)
    levels = [first] + [team.run(cmd_fetch_level(l)) for l in range(1, nl)]
    return levels, team.run(cmd_fetch_tail)


def stacked_level(per_rank):
    """Global A (and P, where the level has one) of a partitioned level; the scalars must be the same bits on all ranks."""
    W = len(per_rank)
    m = int(per_rank[0].halo[0])
    assert all(int(f.halo[0]) == m for f in per_rank), f"HALO m differs: {[int(f.halo[0]) for f in per_rank]}"
    assert all(int(f.halo[1]) == len(f.export) for f in per_rank)
    s0 = per_rank[0].scalars
    assert all(np.array_equal(f.scalars.view(np.int64), s0.view(np.int64)) for f in per_rank), [f.scalars for f in per_rank]
    exports = [f.export for f in per_rank]
    A = DR.stack([f.A for f in per_rank], exports, m)
    P = DR.blockdiag_P([f.P for f in per_rank]) if per_rank[0].P is not None else None
    return SimpleNamespace(A=A, P=P, lam=float(s0[0]), jac=float(s0[1]), has_w=bool(s0[2]), f32=bool(s0[3]), m=m, exports=exports,
                           sizes=[f.A.shape[0] for f in per_rank], W=W)


def aggregation_report(l, q, f, S):
    """What the device and the rule say about the vertices of the first few aggregates they disagree on."""
    agg, root = np.asarray(f.agg, np.int64), np.asarray(f.root).astype(bool)
    ref = R.joined(S, root)
    raw = sp.csr_matrix(f.A)
    unsorted = int(sum(np.any(np.diff(raw.indices[raw.indptr[i]:raw.indptr[i + 1]]) < 0) for i in range(raw.shape[0])))
    dup = int(sum(np.any(np.diff(np.sort(raw.indices[raw.indptr[i]:raw.indptr[i + 1]])) == 0) for i in range(raw.shape[0])))
    lines = [f"AGGREGATION level {l} rank {q}: n={S.n}, {unsorted} rows of the device's piece are not sorted by column, {dup} rows "
             f"hold a column twice, {int((raw.data == 0).sum())} stored zeros"]
    order = np.lexsort((ref, agg))
    a, r = agg[order], ref[order]
    split = np.flatnonzero((a[1:] == a[:-1]) & (r[1:] != r[:-1]))
    for g in np.unique(a[split])[:3]:
        for i in np.flatnonzero(agg == g):
            k = slice(S.A.indptr[i], S.A.indptr[i + 1])
            nb = [(int(c), float(v), bool(st), int(agg[c]), int(ref[c]), bool(root[c]))
                  for c, v, st in zip(S.col[k], S.val[k], S.strong[k])]
            lines.append(f"  raw row {i}: {list(zip(raw.indices[raw.indptr[i]:raw.indptr[i + 1]].tolist(), raw.data[raw.indptr[i]:raw.indptr[i + 1]].tolist()))}")
            lines.append(f"  vertex {i}: agg {agg[i]} rule {ref[i]} root {bool(root[i])}; row (col, val, strong, agg, rule, root): {nb}")
    return "\n".join(lines)


def prolongator_report(l, q, f, S, Pt):
    """The rows of the device's P that hold an entry the reference has not, beside the reference's and the matrix row."""
    P, raw = R.csr(f.P), sp.csr_matrix(f.A)
    pos, _ = R.lookup(Pt, P)
    rows = np.unique(R.rows_of(P)[pos < 0])[:3]
    dF, keep, kappa, keep_all, unsure = R.filtered(S)
    lines = [f"PROLONGATOR level {l} rank {q}: rows {rows} of the device's P hold entries the reference has not"]
    for i in rows:
        k = slice(S.A.indptr[i], S.A.indptr[i + 1])
        lines.append(f"  raw row {i}: {list(zip(raw.indices[raw.indptr[i]:raw.indptr[i + 1]].tolist(), raw.data[raw.indptr[i]:raw.indptr[i + 1]].tolist()))}")
        lines.append(f"  row {i}: (col, val, strong, agg) {[(int(c), float(v), bool(st), int(f.agg[c])) for c, v, st in zip(S.col[k], S.val[k], S.strong[k])]}"
                     f" agg {int(f.agg[i])} dF {float(dF[i])} keep_all {bool(keep_all[i])}")
        lines.append(f"  device P row: {list(zip(P.indices[P.indptr[i]:P.indptr[i + 1]].tolist(), P.data[P.indptr[i]:P.indptr[i + 1]].tolist()))}")
        sel = Pt.row == i
        lines.append(f"  reference P row: {list(zip(Pt.col[sel].tolist(), [float(v) for v in Pt.val[sel]]))}")
    return "\n".join(lines)


def check_block(l, q, f):
    """The checks of one rank's owned block of a coarsened level; returns the worst share of P's envelope."""
    n_q = f.A.shape[0]
    assert f.P.shape[0] == n_q and f.agg is not None, f"level {l}, rank {q}: AGG / ROOT not kept"
    S = R.strength(DR.owned_block(f.A))
    try:
        R.check_aggregation(S, f.agg, f.root)
    except AssertionError:
        print(aggregation_report(l, q, f, S))
        raise
    assert int(f.agg.max()) + 1 == f.P.shape[1], (l, q, int(f.agg.max()) + 1, f.P.shape)
    assert (f.R != f.P.T).nnz == 0, f"level {l}, rank {q}: R != P^T"
    Pt, envP, _, skip = R.prolongator(S, f.agg, f.P.shape[1])
    try:
        return R.check_entries(Pt, envP, f.P, f"P_{l} of rank {q}", skip, zero_may_be_absent=True)
    except AssertionError:
        print(prolongator_report(l, q, f, S, Pt))
        raise


def check_partitioned_levels(levels, report, blocks=True):
    """Checks of section b on the partitioned levels; returns the stacked levels."""
    G = [stacked_level(f) for f in levels]
    nl = len(G)
    worst_p = worst_a = 0.0
    block_errors = []
    for l in range(nl - 1):
        g, per_rank = G[l], levels[l]
        n, m_max = g.A.shape[0], int(np.diff(g.A.indptr).max())
        if blocks:
            for q, f in enumerate(per_rank):
                try:
                    worst_p = max(worst_p, check_block(l, q, f))
                except AssertionError as exc:                     # (judged by the hierarchy test; the stacked checks go on)
                    block_errors.append(f"level {l}, rank {q}: {exc}")
        S = R.strength(g.A)
        lam_plain = R.bounds(S)[0]
        lam_max = None
        if l >= 1:
            s = 1 / np.sqrt(g.A.diagonal())
            lam_max = float(spla.eigsh(sp.diags(s) @ g.A @ sp.diags(s), k=1, which="LA", return_eigenvectors=False, tol=1e-10)[0])
        ratio = R.check_smoothing(g.lam, g.jac, lam_plain, m_max, l, lam_max)
        Act, envA = R.galerkin(g.A, g.P)
        w = R.check_entries(Act, envA, G[l + 1].A, f"stacked A_{l + 1}")
        worst_a = max(worst_a, w)
        report.append(f"  level {l}: n={n} ({g.sizes}) m={g.m} n_export={[len(e) for e in g.exports]} -> {g.P.shape[1]} aggregates; "
                      f"lambda={g.lam:.4f} (plain {float(lam_plain):.4f}) stability {'-' if ratio is None else format(ratio, '.4f')}; "
                      f"A_c {w:.2f} of the envelope; W={int(g.has_w)} f32={int(g.f32)}")
    g = G[-1]
    report.append(f"  gather level: n={g.A.shape[0]} ({g.sizes}) m={g.m} n_export={[len(e) for e in g.exports]}")
    return G, worst_p, worst_a, block_errors


def check_tail_is_the_gather_level(G, levels, tails):
    off = np.concatenate([[0], np.cumsum(G[-1].sizes)])
    for q, t in enumerate(tails):
        assert same_bits(t.A, G[-1].A), f"rank {q}: the gathered operator is not the stacked gather level"
        assert [int(f.halo[2]) for f in levels[-1]][q] == G[-1].A.shape[0] and int(levels[-1][q].halo[3]) == off[q]
        for (A, P, s), (A0, P0, s0) in zip(t.levels, tails[0].levels):
            assert same_bits(A, A0) and (P is None) == (P0 is None) and (P is None or same_bits(P, P0)) and \
                np.array_equal(s.view(np.int64), s0.view(np.int64)), f"rank {q}: its tail hierarchy differs from rank 0's"


def reference_levels(G, tail):
    """The levels of the reference cycle: partitioned levels, then the tail's, the tail's coarsest operator last."""
    lv = [dict(A=g.A, P=g.P, lam=g.lam) for g in G[:-1]]
    lv += [dict(A=A, P=P, lam=float(s[0])) for A, P, s in tail.levels[:-1]]
    return lv + [dict(A=tail.levels[-1][0])]


_HIER = {}


def small_hierarchy(switches, world):
    """The checked hierarchy of the small system on `world` ranks, its right-hand sides and reference cycle: computed once."""
    if world in _HIER:
        return _HIER[world]
    for k, v in SMALL_ENV.items():
        switches.set(k, v)
    sysm = layered(*SMALL)
    report = [f"HIERARCHY 8 x 40 x 30 on {world} ranks"]
    with RankTeam(world, solver_setup(sysm, world)) as team:
        levels, tails = fetch_hierarchy(team)
        reps = team.run(lambda rank, st: np.asarray(st.ds.owned_reduced_global))
        G, worst_p, worst_a, block_errors = check_partitioned_levels(levels, report)
        check_tail_is_the_gather_level(G, levels, tails)
        tail_report = []
        tail_levels, _ = team.run(lambda rank, st: check_hierarchy(st.ds.A.amg_tail(), dict(min_levels=2), tail_report), ranks=[0])[0]
    report += tail_report
    for k in SMALL_ENV:
        switches.unset(k)
    for (A, P, s), L in zip(tails[0].levels, tail_levels):
        assert same_bits(A, L["A"]) and (P is None or same_bits(P, L["P"]))
    shape = [g.A.shape[0] for g in G] + [A.shape[0] for A, _, _ in tails[0].levels[1:]]
    report.append(f"  shape: {' > '.join(map(str, shape))} ({len(G) - 1} partitioned levels, the gather level, a tail of "
                  f"{len(tails[0].levels)} levels); P at most {worst_p:.2f}, A_c at most {worst_a:.2f} of their envelopes")
    h = SimpleNamespace(block_errors=block_errors, G=G, tails=tails, reps=reps, report=report, shape=shape, worst_p=worst_p, worst_a=worst_a)
    # right-hand sides and the reference cycle
    n = G[0].A.shape[0]
    off = np.concatenate([[0], np.cumsum(G[0].sizes)]).astype(np.int64)
    special = int(off[1] + G[0].exports[1][0])
    B = right_hand_sides(n, special)
    units = np.zeros((n, 2 * world))
    for q in range(world):
        units[off[q], 2 * q] = units[off[q + 1] - 1, 2 * q + 1] = 1.0
    h.B, h.off = np.concatenate([B, units], axis=1), off
    h.Z, h.ENV, h.e32 = reference_cycle(reference_levels(G, tails[0]), h.B)
    _HIER[world] = h
    return h


@pytest.mark.parametrize("world", WORLDS)
def test_hierarchy_level_by_level_on_the_stacked_operators(switches, world):
    h = small_hierarchy(switches, world)
    print("\n".join(h.report))
    G = h.G
    assert not h.block_errors, "\n".join(h.block_errors)
    # the shape this setup is chosen for: two partitioned levels that coarsen, the gather level, a tail of two levels
    assert len(G) == 3 and len(h.tails[0].levels) == 2, h.shape
    assert G[-1].A.shape[0] <= 200 < G[-2].A.shape[0] and h.tails[0].levels[-1][0].shape[0] <= 64
    if world == 3:
        assert len(set(G[0].sizes)) > 1 and len({len(e) for e in G[0].exports}) > 1
    # fine operator: the oracle's reduced matrix, permuted by owned_reduced_global
    A_or, _ = oracle_system(*SMALL)
    perm = np.concatenate(h.reps) - 1
    assert np.array_equal(np.sort(perm), np.arange(A_or.shape[0]))
    want = R.csr(A_or[perm][:, perm])
    got = R.csr(G[0].A)
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), "pattern of the stacked A_0"
    bitwise = np.array_equal(got.data.view(np.int64), want.data.view(np.int64))
    rel = float(np.abs(got.data - want.data).max() / np.abs(want.data).max())
    print(f"FINE OPERATOR world {world}: stacked A_0 {'==' if bitwise else '!='} the oracle's matrix bit for bit (largest difference "
          f"{rel:.2e} of the largest entry)")
    assert bitwise


def test_nothing_is_kept_without_the_switch_on_partitioned_levels(switches):
    """Without PADNE_AMG_KEEP a partitioned level keeps neither array (the probe says so); SCALARS, EXPORT and HALO are there all
    the same; a wrong size, and EXPORT / HALO asked of a single-GPU hierarchy (the tail), are refused."""
    switches.set("PADNE_AMG_GATHER_N", "200")
    switches.set("PADNE_AMG_COARSE_N", "64")
    sysm = layered(*SMALL)

    def probe(rank, st):
        A, c = st.ds.A, st.ctx
        A.amg_apply_dist(np.zeros(st.ds.n_owned))
        lib, P = c._lib, _hip._P
        n = A.shape[0]
        buf, out, h4 = np.zeros(n, np.int32), np.zeros(4), np.zeros(4, np.int64)
        rc = dict(agg=lib.padne_test_amg_state(c._h, A._h, 0, 0, buf.ctypes.data_as(P), buf.nbytes),
                  root=lib.padne_test_amg_state(c._h, A._h, 0, 1, buf.ctypes.data_as(P), n),
                  scalars=lib.padne_test_amg_state(c._h, A._h, 0, 2, out.ctypes.data_as(P), 32),
                  halo=lib.padne_test_amg_state(c._h, A._h, 0, 4, h4.ctypes.data_as(P), 32),
                  halo_size=lib.padne_test_amg_state(c._h, A._h, 0, 4, h4.ctypes.data_as(P), 24),
                  export=lib.padne_test_amg_state(c._h, A._h, 0, 3, buf.ctypes.data_as(P), 4 * int(h4[1])),
                  export_size=lib.padne_test_amg_state(c._h, A._h, 0, 3, buf.ctypes.data_as(P), 4 * int(h4[1]) + 4),
                  unknown=lib.padne_test_amg_state(c._h, A._h, 0, 5, out.ctypes.data_as(P), 32),
                  level=lib.padne_test_amg_state(c._h, A._h, 9, 2, out.ctypes.data_as(P), 32))
        t = A.amg_tail()
        rc["tail_halo"] = lib.padne_test_amg_state(c._h, t._h, 0, 4, h4.ctypes.data_as(P), 32)
        rc["tail_agg"] = lib.padne_test_amg_state(c._h, t._h, 0, 0, buf.ctypes.data_as(P), 4 * t.shape[0])
        h = _hip._P()
        rc["tail_of_tail"] = lib.padne_test_amg_tail(t._h, _hip.C.byref(h))
        t.close()                                                 # (borrowed: closing the wrapper destroys nothing)
        A.amg_apply_dist(np.zeros(st.ds.n_owned))                 # ... the hierarchy is still whole
        return rc, np.array_equal(buf[:int(h4[1])], st.plan.export_reduced)
    with RankTeam(2, solver_setup(sysm, 2)) as team:
        for rc, export_ok in team.run(probe):
            I, OK = _hip.E_INVALID, _hip.OK
            assert rc == dict(agg=I, root=I, scalars=OK, halo=OK, halo_size=I, export=OK, export_size=I, unknown=I, level=I,
                              tail_halo=I, tail_agg=I, tail_of_tail=I), rc
            assert export_ok, "EXPORT of level 0 is the plan's export list"


# ---- c. the cycle -------------------------------------------------------------------------------------------------------

def device_cycle(team, off, B):
    """The partitioned cycle on every column of B, reassembled."""
    W = len(off) - 1
    Z = np.empty_like(B)
    for j in range(B.shape[1]):
        parts = team.run(cmd_cycle([np.ascontiguousarray(B[off[q]:off[q + 1], j]) for q in range(W)]))
        Z[:, j] = np.concatenate(parts)
    return Z


def level_flags(team, n_partitioned):
    fl = team.run(lambda rank, st: [tuple(st.ds.A.amg_state(l, "SCALARS")) for l in range(n_partitioned)])
    assert all(f == fl[0] for f in fl)
    return fl[0]


CYCLE_FORMS = [(w, extra) for w in ("none", "fine", None) for extra in (None, "PADNE_AMG_EXCHANGE_ALL", "PADNE_NO_P2P", "PADNE_NO_SPLIT")]


@pytest.mark.parametrize("world", WORLDS)
def test_double_precision_cycle_lies_in_the_envelope(switches, world):
    h = small_hierarchy(switches, world)
    for k, v in dict(SMALL_ENV, PADNE_AMG_F64="1").items():
        switches.set(k, v)
    with RankTeam(world, solver_setup(layered(*SMALL), world)) as team:
        Z64 = device_cycle(team, h.off, h.B)
        flags = level_flags(team, len(h.G) - 1)
    assert [f[0] for f in flags] == [g.lam for g in h.G[:-1]] and all(f[2:] == (0.0, 0.0) for f in flags), flags
    err = np.abs(Z64.astype(LD) - h.Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.where(h.ENV > 0, err / h.ENV, 0).max())
    print(f"CYCLE f64 world {world}: worst error {worst:.3g} of the envelope; envelope at most "
          f"{float((h.ENV.max(axis=0) / np.abs(h.Z).max(axis=0)).max()):.1e} of max |z|")
    assert (err <= h.ENV).all(), f"double-precision cycle outside its envelope: {worst:.3g} x"


@pytest.mark.parametrize("w,extra", CYCLE_FORMS)
@pytest.mark.parametrize("world", WORLDS)
def test_single_precision_cycle_against_the_plain_float32_evaluation(switches, world, w, extra):
    h = small_hierarchy(switches, world)
    assert (h.e32 > 0).all() and (h.e32 < 1e-4).all(), h.e32
    env = dict(SMALL_ENV)
    if w is not None:
        env["PADNE_AMG_W"] = w
    if extra is not None:
        env[extra] = "1"
    for k, v in env.items():
        switches.set(k, v)
    with RankTeam(world, solver_setup(layered(*SMALL), world)) as team:
        Z32 = device_cycle(team, h.off, h.B)
        flags = level_flags(team, len(h.G) - 1)
    want_w = [w is None or (w == "fine" and l == 0) for l in range(len(h.G) - 1)]
    assert [f[0] for f in flags] == [g.lam for g in h.G[:-1]], "another hierarchy than the checked one"
    assert [f[2] == 1.0 for f in flags] == want_w and all(f[3] == 1.0 for f in flags), (w, flags)
    ratio = norm2(Z32.astype(LD) - h.Z) / norm2(h.Z) / h.e32
    print(f"CYCLE f32 world {world} W={w or 'all'} {extra or '-'}: worst error / plain float32 error {float(ratio.max()):.2f} "
          f"(right-hand side {int(np.argmax(ratio))}); plain float32 error {float(h.e32.min()):.1e} .. {float(h.e32.max()):.1e}")
    assert ratio.max() <= F32_FACTOR, ratio


def test_large_case_galerkin_and_cycle_on_two_ranks(switches):
    """72 k rows per rank: the partitioned fine level takes the x-window forms.  Galerkin and cycle checks only."""
    t0 = time.perf_counter()
    world = 2
    for k, v in LARGE_ENV.items():
        switches.set(k, v)
    sysm = layered(*LARGE)
    report = ["LARGE 2 x 300 x 240 on 2 ranks"]
    with RankTeam(world, solver_setup(sysm, world)) as team:
        levels, tails = fetch_hierarchy(team)
        assert levels[0][0].A.shape[0] >= 65536
        G, _, worst_a, _ = check_partitioned_levels(levels, report, blocks=False)
        check_tail_is_the_gather_level(G, levels, tails)
        n = G[0].A.shape[0]
        off = np.concatenate([[0], np.cumsum(G[0].sizes)]).astype(np.int64)
        B = right_hand_sides(n, int(off[1] + G[0].exports[1][0]))
        units = np.zeros((n, 4))
        for q in range(world):
            units[off[q], 2 * q] = units[off[q + 1] - 1, 2 * q + 1] = 1.0
        B = np.concatenate([B, units], axis=1)
        Z, ENV, e32 = reference_cycle(reference_levels(G, tails[0]), B)
        Z32 = device_cycle(team, off, B)
        flags = level_flags(team, len(G) - 1)
    assert all(f[2:] == (1.0, 1.0) for f in flags), flags
    ratio = norm2(Z32.astype(LD) - Z) / norm2(Z) / e32
    switches.set("PADNE_AMG_F64", "1")
    with RankTeam(world, solver_setup(sysm, world)) as team:
        Z64 = device_cycle(team, off, B)
    err = np.abs(Z64.astype(LD) - Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst64 = float(np.where(ENV > 0, err / ENV, 0).max())
    shape = [g.A.shape[0] for g in G] + [A.shape[0] for A, _, _ in tails[0].levels[1:]]
    report.append(f"  shape {' > '.join(map(str, shape))}; A_c at most {worst_a:.2f} of its envelope; f64 cycle {worst64:.3g} of the "
                  f"envelope; f32 cycle {float(ratio.max()):.2f} x the plain float32 error (right-hand side {int(np.argmax(ratio))}); "
                  f"{time.perf_counter() - t0:.1f} s")
    print("\n".join(report))
    assert (err <= ENV).all(), f"double-precision cycle outside its envelope: {worst64:.3g} x"
    assert ratio.max() <= F32_FACTOR, ratio


# ---- d. CG iterates and the reported numbers ----------------------------------------------------------------------------

JACOBI_KS = (1, 2, 5, 12, 40)
MG_KS = (1, 2, 3, 4, 5, 7, 8, 9, 17)      # MG_KS of test_pcg_vs_reference.py + the edges of four iterations per look at the status
FORMS = {"jacobi": dict(precond="jacobi", env={}, block=False, ks=JACOBI_KS),
         "global": dict(precond="amg", env={}, block=False, ks=MG_KS),
         "global_f64": dict(precond="amg", env={"PADNE_AMG_F64": "1"}, block=False, ks=MG_KS),
         "block": dict(precond="amg", env={}, block=True, ks=MG_KS)}


def global_problem(team):
    """(A, b, perm) of the oracle in the team's numbering: rank order, unknown g of the partition = row g - 1 of the oracle."""
    A_or, b_or = oracle_system(*SMALL)
    reps = team.run(lambda rank, st: np.asarray(st.ds.owned_reduced_global))
    bs = team.run(lambda rank, st: st.ds.b.numpy())
    perm = np.concatenate(reps) - 1
    A = R.csr(A_or[perm][:, perm])
    b = b_or[perm]
    assert np.array_equal(np.concatenate(bs), b), "the ranks' right-hand sides are the oracle's"
    off = np.concatenate([[0], np.cumsum([len(r) for r in reps])]).astype(np.int64)
    return A, b, off


def team_solve(team, precond, max_iter, rtol):
    """One solve on every rank; the ranks' reports must agree; the reassembled iterate in .x"""
    res = team.run(cmd_solve(precond, max_iter, rtol))
    r0 = res[0]
    for r in res[1:]:
        assert (r.iterations, r.status, r.restarts, r.precond_fallbacks) == (r0.iterations, r0.status, r0.restarts, r0.precond_fallbacks)
        assert r.rel_residual == r0.rel_residual and r.abs_residual == r0.abs_residual
    return SimpleNamespace(x=np.concatenate([r.x for r in res]), iterations=r0.iterations, status=r0.status, restarts=r0.restarts,
                           precond_fallbacks=r0.precond_fallbacks, rel_residual=r0.rel_residual, abs_residual=r0.abs_residual,
                           levels=r0.levels)


def host_preconditioner(team, form, off, unit):
    """M of the reference run: None (Jacobi); the device's partitioned cycle, or the per-rank cycles of the diagonal blocks
    side by side, as black boxes in the loop's units."""
    if form == "jacobi":
        return None
    W = len(off) - 1
    split = lambda r: [np.ascontiguousarray(r[off[q]:off[q + 1]]) for q in range(W)]
    if form == "block":
        apply = lambda r: np.concatenate(team.run(lambda rank, st, p=split(r): st.ds.A_block.amg_apply(p[rank])))
    else:
        apply = lambda r: np.concatenate(team.run(cmd_cycle(split(r))))
    if form == "global_f64":
        return lambda r: apply(np.float64(r))
    s_, s_inv = in_units(unit)
    return lambda r: apply(np.float64(r) * s_inv) * s_


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("world", WORLDS)
def test_cg_iterates_of_the_partitioned_loops(switches, world, form):
    F = FORMS[form]
    for k, v in dict(SMALL_ENV, **F["env"]).items():
        switches.set(k, v)
    with RankTeam(world, solver_setup(layered(*SMALL), world, block=F["block"])) as team:
        A, b, off = global_problem(team)
        first = team_solve(team, F["precond"], 1, NEVER)             # (builds the hierarchy)
        assert first.levels == 0 if form == "jacobi" else first.levels >= 2
        if form == "block":
            f32 = team.run(lambda rank, st: bool(st.ds.A_block.amg_state(0, "SCALARS")[3]))
            assert all(f32)
        unit = np.linalg.norm(b)
        M = host_preconditioner(team, form, off, unit)
        ld, d_host = calibrated(A, b, max(F["ks"]), M=M, r32_unit=unit if form in ("global", "block") else None)
        for k in F["ks"]:
            res = team_solve(team, F["precond"], k, NEVER)
            assert res.status == _hip.E_NOTCONVERGED and res.iterations == k and res.restarts == 0 and res.precond_fallbacks == 0, \
                (k, res.status, res.iterations)
            check_iterate(f"dist{world}/{form}", k, res.x, ld, d_host)


@pytest.mark.parametrize("form", ["jacobi", "global", "block"])
@pytest.mark.parametrize("world", WORLDS)
def test_stopping_rule_and_reported_residuals_of_the_partitioned_loops(switches, world, form):
    F = FORMS[form]
    for k, v in dict(SMALL_ENV, **F["env"]).items():
        switches.set(k, v)
    with RankTeam(world, solver_setup(layered(*SMALL), world, block=F["block"])) as team:
        A, b, _ = global_problem(team)
        for rtol in (1e-6, 1e-9):
            res = team_solve(team, F["precond"], 200000, rtol)
            check_stop(A, b, res, rtol, 0.0)

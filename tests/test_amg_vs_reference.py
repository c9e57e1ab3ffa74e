"""The device's multigrid hierarchy and V-cycle (csrc/amg.hip) against the specification in tests/amg_ref.py.

Every system is set up under PADNE_AMG_KEEP=1, so that every coarsened level keeps its aggregate map and root flags
(padne_test_amg_state).  Level by level the device's arrays are then held against what the specification says a hierarchy
IS -- never against another device path, and never using a number of the device's that has not been checked first:

  1. aggregation   check_aggregation on AGG / ROOT (roots more than two strong hops apart and maximal, one root per
                   aggregate, membership by the two join passes up to renumbering); n_agg == columns of P; undecided
                   strength entries (within 1e-12 of the threshold) at most 0.1 % of a level's off-diagonals
  2. smoothing     lambda_0 == Gershgorin bound to (m + 2) u; below: lambda_l <= that bound, and 1.1 lambda_l >
                   lambda_max(D^-1/2 A_l D^-1/2) (eigsh), which is jac lambda_max < 2; jac_l == 1 / (0.55 lambda_l) to 2 ulp
  3. prolongator   pattern of the reference (exact zeros may be absent), every value within the derived envelope, row sums
                   1 - omega rowsum(A)_i / d^F_i within the row's envelope where the equation sums to zero
  4. coarse        pattern of A_{l+1} == symbolic pattern of P^T A_l P, every entry within gamma_k |P^T| |A| |P|
  5. cycle         16 right-hand sides (7 random, constant, a smooth and an oscillatory mode, unit vectors at rows 0, 63,
                   64, n - 1 and a hub / middle row, one random sparse).  PADNE_AMG_F64=1: amg_apply within the forward-error
                   envelope of the longdouble cycle on the device's (checked) A_l, P_l, lambda_l and dense_ref's inverse.
                   Single precision, under PADNE_AMG_W=none, fine and the default, and amg_apply_batch at k = 2, 4, 8
                   with units that differ by twelve orders of magnitude: per vector, the 2-norm error against the
                   longdouble cycle is at most F32_FACTOR x that of the plain float32 evaluation of the same formula on the host.

Systems (the smallest that reach each kernel family; the family's condition of aggregate() / build_prolongator() is
asserted from the level shapes):
  a  2 x 40 x 30, PADNE_AMG_COARSE_N=64   three levels (four were hoped for); small levels with nnz <= 16 n take the compact
                                          rounds and mis_tail_rounds
  b  3 x 90 x 70                          the default hierarchy
  c  8 x 40 x 30, PADNE_AMG_COARSE_N=64   a coarsened level with nnz >= 24 n, n <= 65536: nbr_max_wpr, lane-group / dense spgemm rows
  d  2 x 300 x 240 (144 k unknowns)       x-window plan; dx: the same under PADNE_NO_XWINDOW=1 -- each against the specification
  e  d + hubs of 13 .. 600 far resistors  rows over 13 entries (slot path of the prolongator).  These hubs keep their strong
                                          mesh neighbours and d^F / a_ii >= 0.4: no keep-all row, no lone vertex -- hence g
  g  a + one hub of 200 resistors of 1 mOhm   a row of 200 entries, all weak: a vertex without strong neighbours (an aggregate
                                          of its own) whose lumped diagonal collapses (keep-all row: d^F / a_ii <= 0.05)
  f  50 x 44 mesh, signed cotangents      positive off-diagonal entries (obtuse angles), PADNE_AMG_COARSE_N=64

Strength symmetry.  strong(a, d_i, d_j) multiplies a a d_i d_j from the left, which is not symmetric in its rounding, so the
device's graph can be asymmetric at an entry within ~4 u of the threshold.  Such an entry is "undecided" here (1e-12), and
no level of any case has one: the closest entry of all levels of all cases is recorded below.  Nothing to fix.

Measured on an MI355X (every run prints these lines: pytest -s).  Per system: levels n_0 > n_1 > ..; the kernel-family
conditions that held on a coarsened level; the share of undecided strength entries (and the closest entry's relative
distance to the threshold); the smallest stability ratio 1.1 lambda_l / lambda_max (the bar is > 1, not this number); the
worst single-precision error ratio over the right-hand sides and the forms (the bar is F32_FACTOR):
  a   2399 > 344 > 38           nnz <= 16 n on levels 0, 1 (compact rounds, tail rounds), a row > 13 on level 1;
                                undecided 0 (1.3e-3); stability 1.160; f32 6.05 (single cycle, the oscillatory mode), 2.80 (batched)
                                -- three levels, not four: the aggregates hold ~7 vertices, 38 <= 64 ends the hierarchy
  b   18899 > 2664 > 295        nnz <= 16 n, rows > 13 and positive off-diagonals on level 1; undecided 0 (2.9e-5);
                                stability 1.153; f32 1.39
  c   9599 > 1377 > 161 > 26    level 2: nnz = 37.9 n >= 24 n, n <= 65536 (wave-per-row neighbour maxima, long spgemm
                                rows); undecided 0 (6.4e-6); stability 1.117 (level 1), 1.141; f32 2.70
  d   143999 > 19835 > 2048     n >= 65536, rows <= 13: x-window plan; undecided 0 (1.2e-5); stability 1.121; f32 1.18
  dx  the same levels           general kernels; the same figures as d to the digits printed
  e   143999 > 19835 > 2048     max row 609 on level 0 (slot path), 1412 on level 1; undecided 0 (1.2e-5); stability 1.121;
                                f32 1.62 (single cycle, the hub's unit vector), 1.35 (batched)
  g   2399 > 347 > 42           level 0: a row of 206 entries, a keep-all row, a vertex without strong neighbours; level 1:
                                nnz = 169.5 n (long rows), keep-all rows; undecided 0 (1.5e-3); stability 1.144;
                                f32 2.08 (single cycle), 7.58 (batched, k = 4 and 8, the third random vector)
  f   2199 > 295 > 36           positive off-diagonals on every level; lambda_F > lambda on level 0 (3.715 > 3.646: omega is
                                capped by the plain bound); undecided 0 (5.1e-4); stability 1.150; f32 1.35 (single cycle), 3.20 (batched)
The errors of P are at most 0.17, those of A_c at most 0.64 of their envelopes.  The double-precision cycle uses at most
8.9e-5 of its envelope -- the envelope is dominated by the worst-case bound of the coarsest solve (8 n u |A^-1| |A| |A^-1|:
up to 1.3e-4 of max |z| with 2048 coarse unknowns, 1e-8 with 40), so that check catches a wrong stage, not a rounding;
the single-precision check is the sharper one.  The three PADNE_AMG_W forms agree within 7 % in every case.

The batched cycle of case g.  Measured apart, with the same eight right-hand sides under other units (as they are, |r|^2,
1e6 |r|^2, 1e-6 |r|^2; a power of four changes no bit): the ratios of the batched cycle scatter between 0.4 and 7.5 from one
choice of units to the next, the single cycle's stay within 0.4 .. 1.3, and cases a and f stay below 4.1.  The units only
move every rounding, so this is the spread of the cycle's rounding error itself, not a term that depends on the units:
the hub's row (200 couplings of 1000 S against a diagonal of 208000 S, and rows of 270 entries on level 1) cancels heavily
in every residual, and the batched products (spmm.hip) associate the sum of such a row differently from the long-row
forms the single cycle takes (spmv.hip).  Within the factor; the test's inputs are fixed and the kernels deterministic, so
the figure above is what every run sees.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import amg_ref as R
import dense_ref as D

pytestmark = pytest.mark.gpu

LD = np.longdouble
# The device's single-precision cycle may err by this many times the plain float32 evaluation: it associates differently
# (tile and lane sums, W = P - c D^-1 A P formed in double and rounded once before it is applied, the residual formed from
# b alone).  Worst measured ratio: 7.58 (case g, batched cycle at k = 4, third random vector; the single cycle has 2.08 there);
# 6.05 for the single cycle (case a, oscillatory mode); every other case stays below 3.3.
F32_FACTOR = 8.0


def norm2(v):
    return np.sqrt((np.asarray(v, LD) ** 2).sum(axis=0))


def hub_elements(n_vertices):
    """The hubs of test_sparse_products_with_rows_beyond_every_limit_of_the_lane_group_kernels: six vertices with 13 .. 600 far
    resistors.  Returns (elements, hub vertices)."""
    rng = np.random.default_rng(11)
    els, hubs = [], []
    for h, deg in enumerate((13, 20, 40, 80, 200, 600)):
        hub = 300 * (17 + 31 * h) + 11 * h + 7
        far = rng.choice(np.arange(1, n_vertices), size=deg, replace=False)
        els += [("R", int(hub), int(f), 0.05 + 0.01 * (k % 7)) for k, f in enumerate(far) if int(f) != hub]
        hubs.append(hub)
    return els, hubs


def lone_hub(n_vertices, hub=1234, degree=200, ohms=1e-3):
    """One vertex with `degree` far resistors so conductive that its diagonal dwarfs every entry of its row: all its
    couplings are weak (no strong neighbour), and its lumped diagonal collapses to the row sum (a keep-all row)."""
    far = np.random.default_rng(5).choice(np.setdiff1d(np.arange(1, n_vertices), [hub]), size=degree, replace=False)
    return [("R", hub, int(f), ohms) for f in far]


CASES = {
    "a": dict(build=lambda: R.layered_matrix(2, 40, 30, 4), env={"PADNE_AMG_COARSE_N": "64"}, min_levels=3, fine_share_zero=True),
    "b": dict(build=lambda: R.layered_matrix(3, 90, 70, 5), env={}, min_levels=3, fine_share_zero=True),
    "c": dict(build=lambda: R.layered_matrix(8, 40, 30, 5), env={"PADNE_AMG_COARSE_N": "64"}, min_levels=4, long_rows=True),
    "d": dict(build=lambda: R.layered_matrix(2, 300, 240, 6), env={}, min_levels=3, fine_share_zero=True, windowed=True),
    "dx": dict(build=lambda: R.layered_matrix(2, 300, 240, 6), env={"PADNE_NO_XWINDOW": "1"}, min_levels=3, fine_share_zero=True),
    "e": dict(build=lambda: R.layered_matrix(2, 300, 240, 6, hub_elements(2 * 300 * 240)[0]), env={}, min_levels=3, hubs=True),
    "g": dict(build=lambda: R.layered_matrix(2, 40, 30, 4, lone_hub(2400)), env={"PADNE_AMG_COARSE_N": "64"}, min_levels=3, lone=True),
    "f": dict(build=lambda: R.obtuse_matrix(50, 44), env={"PADNE_AMG_COARSE_N": "64"}, min_levels=3, positive=True),
}


def right_hand_sides(n, special_row):
    rng = np.random.default_rng(2024)
    i = np.arange(n)
    B = np.zeros((n, 16))
    B[:, :7] = rng.uniform(-1, 1, (n, 7))
    B[:, 7] = 1.0
    B[:, 8] = np.sin(np.pi * (i + 1) / (n + 1))
    B[:, 9] = 1.0 - 2.0 * (i & 1)
    for k, r in enumerate((0, 63, 64, n - 1, special_row)):
        B[r, 10 + k] = 1.0
    B[rng.choice(n, 5, replace=False), 15] = rng.uniform(-1, 1, 5)
    return B


def check_hierarchy(d, case, report):
    """Checks 1 - 4 on every coarsened level; returns the (checked) operators the reference cycle is built from."""
    shapes = d.amg_shapes()
    nl = len(shapes)
    assert nl >= case["min_levels"], shapes
    levels, seen = [], dict(long_rows=False, compact=False, slot=False, keep_all=False, lonely=False, positive=False)
    closest = np.inf
    for l in range(nl - 1):
        A, P, Rm = d.amg_level(l, "A"), d.amg_level(l, "P"), d.amg_level(l, "R")
        A_next = d.amg_level(l + 1, "A")
        agg, root = d.amg_state(l, "AGG"), d.amg_state(l, "ROOT")
        lam, jac, has_w, is_f32 = d.amg_state(l, "SCALARS")
        n, nnz = A.shape[0], A.nnz
        assert (n, n, nnz) == shapes[l]["A"] and (Rm != P.T).nnz == 0
        m_max = int(np.diff(A.indptr).max())
        # 1. aggregation
        S = R.strength(A)
        share = S.undecided_share()
        closest = min(closest, float(np.nanmin(np.abs(S.dist))))
        assert share <= 1e-3, f"level {l}: {share:.2%} of the off-diagonals are undecided"
        if l == 0 and case.get("fine_share_zero"):
            assert share == 0.0
        G = S.graph()
        assert (G != G.T).nnz == 0, "the strength graph of the specification is symmetric"
        skipped = R.check_aggregation(S, agg, root)
        assert int(agg.max()) + 1 == P.shape[1], f"level {l}: {int(agg.max()) + 1} aggregates, P has {P.shape[1]} columns"
        # 2. smoothing parameters
        lam_plain, lam_f = R.bounds(S)
        lam_max = None
        if l >= 1:
            s = 1 / np.sqrt(A.diagonal())
            lam_max = float(spla.eigsh(sp.diags(s) @ A @ sp.diags(s), k=1, which="LA", return_eigenvectors=False, tol=1e-10)[0])
        ratio = R.check_smoothing(lam, jac, lam_plain, m_max, l, lam_max)
        # 3. prolongator
        Pt, envP, omega, skip = R.prolongator(S, agg, P.shape[1])
        worst_p = R.check_entries(Pt, envP, P, f"P_{l}", skip, zero_may_be_absent=True)
        dF = R.filtered(S)[0]
        a_sum = R.row_sum(A, S.val)
        zero_sum = (np.abs(a_sum) <= 1e-9 * S.diag) & ~skip
        env_row = np.zeros(n, LD)
        np.add.at(env_row, Pt.row, envP)
        p_sum = R.row_sum(R.csr(P), R.csr(P).data.astype(LD))
        off_one = np.abs(p_sum - (1 - omega * a_sum / dF))[zero_sum]
        assert zero_sum.any() and (off_one <= env_row[zero_sum] + R.gamma(m_max) * 1).all(), f"level {l}: row sums of P"
        # 4. coarse operator
        Act, envA = R.galerkin(A, P)
        worst_a = R.check_entries(Act, envA, A_next, f"A_{l + 1}")
        # which kernel families this level takes (the conditions of aggregate() and build_prolongator())
        keep_all = R.filtered(S)[3]
        lonely = np.diff(G.indptr) == 0
        fam = dict(long_rows=n <= 65536 and nnz >= 24 * n, compact=nnz <= 16 * n, slot=m_max > 13, keep_all=bool(keep_all.any()),
                   lonely=bool(lonely.any()), positive=bool((S.val[S.off] > 0).any()))
        for k, v in fam.items():
            seen[k] |= v
        report.append(f"  level {l}: n={n} nnz/n={nnz / n:.1f} max row {m_max} -> {P.shape[1]} aggregates; undecided {share:.1e}"
                      f" (membership of {skipped} vertices not compared); lambda={lam:.4f} (plain {float(lam_plain):.4f}, F "
                      f"{float(lam_f):.4f}) stability {'-' if ratio is None else format(ratio, '.4f')}; P {worst_p:.2f} / A_c "
                      f"{worst_a:.2f} of the envelope; W={int(has_w)} f32={int(is_f32)}; "
                      + ",".join(k for k, v in fam.items() if v))
        levels.append(dict(A=A, P=P, lam=lam, has_w=bool(has_w), f32=bool(is_f32), ratio=ratio))
    levels.append(dict(A=d.amg_level(nl - 1, "A")))
    report.append(f"  coarsest: n={levels[-1]['A'].shape[0]}; closest strength entry {closest:.1e} from the threshold")
    # the coarsest level keeps nothing, and no level keeps what was not asked for
    with pytest.raises(Exception):
        d.amg_state(nl - 1, "AGG")
    return levels, seen


def reference_cycle(levels, B):
    """(Z, ENV, E32): the longdouble cycle on the 16 right-hand sides, the forward-error envelope of a double-precision
    evaluation, and the relative 2-norm error of the plain float32 evaluation."""
    ops = [(L["A"], L["P"], L["lam"]) for L in levels[:-1]]
    Ac = levels[-1]["A"]
    Acs = R.csr((Ac + Ac.T) * 0.5)                                           # (exactly symmetric, as dense_ref asks)
    coarse = D.refined_solver(Acs)
    inv64 = np.linalg.inv(Acs.toarray())
    Z, ENV = R.cycle_envelope(ops, coarse, Ac, B, abs_inv=np.abs(inv64) * (1 + 1e-6), coarse_delta=abs(Ac - Acs))
    Z32 = R.cycle(ops, inv64, B, dtype=np.float32)
    return Z, ENV, norm2(Z32.astype(LD) - Z) / norm2(Z)


@pytest.mark.parametrize("name", list(CASES))
def test_hierarchy_and_cycle_against_the_specification(ctx, switches, name):
    case = CASES[name]
    A = case["build"]()
    n = A.shape[0]
    switches.set("PADNE_AMG_KEEP", "1")
    for k, v in case["env"].items():
        switches.set(k, v)
    report = [f"case {name}: n={n} nnz={A.nnz}"]
    d = ctx.csr_from_scipy(A)
    try:
        d.amg_apply(np.ones(n))                                               # (builds the hierarchy)
        levels, seen = check_hierarchy(d, case, report)
        assert all(L["f32"] for L in levels[:-1]), "the default cycle runs in single precision"
        assert all(L["has_w"] for L in levels[:-1]), "by default every level goes up with W"
    finally:
        d.close()
    # the family this case is there for
    if case.get("windowed"):
        assert n >= 65536 and int(np.diff(A.indptr).max()) <= 13
    if case.get("long_rows"):
        assert seen["long_rows"], "no coarsened level with nnz >= 24 n"
    if name == "a":
        assert seen["compact"] and any(L["A"].shape[0] <= 2048 and L["A"].nnz <= 16 * L["A"].shape[0] for L in levels[1:-1])
    if case.get("hubs"):
        assert seen["slot"], seen
    if case.get("lone"):
        S0 = R.strength(A)
        assert R.filtered(S0)[3][1233] and not S0.strong[S0.row == 1233].any() and np.diff(A.indptr)[1233] > 13
    if case.get("positive"):
        assert seen["positive"]
    special = hub_elements(2 * 300 * 240)[1][-1] - 1 if case.get("hubs") else (1233 if case.get("lone") else n // 2)
    B = right_hand_sides(n, special)
    Z, ENV, e32 = reference_cycle(levels, B)
    zn = norm2(Z)
    assert (e32 > 0).all() and (e32 < 1e-4).all(), e32               # (the yardstick is a single-precision rounding error)

    def applied(env, fn):
        for k, v in env.items():
            switches.set(k, v)
        m = ctx.csr_from_scipy(A)
        try:
            out = fn(m)
            flags = [tuple(m.amg_state(l, "SCALARS")[2:]) for l in range(len(levels) - 1)]
        finally:
            m.close()
            for k in env:
                switches.unset(k)
        return out, flags

    # double-precision cycle: within the forward-error envelope, entry by entry
    Z64, flags = applied({"PADNE_AMG_F64": "1"}, lambda m: np.stack([m.amg_apply(B[:, j]) for j in range(16)], axis=1))
    assert all(f == (0.0, 0.0) for f in flags)
    err64 = np.abs(Z64.astype(LD) - Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst64 = float(np.where(ENV > 0, err64 / ENV, 0).max())
    report.append(f"  f64 cycle: worst error {worst64:.3g} of the envelope; envelope at most {float((ENV.max(axis=0) / np.abs(Z).max(axis=0)).max()):.1e} of max |z|")
    ok64 = bool((err64 <= ENV).all())
    # single-precision cycle, every up-leg form, single and batched
    ratios = {}
    for w in ("none", "fine", None):
        env = {} if w is None else {"PADNE_AMG_W": w}
        Z32, flags = applied(env, lambda m: np.stack([m.amg_apply(B[:, j]) for j in range(16)], axis=1))
        want_w = [w is None or (w == "fine" and l == 0) for l in range(len(levels) - 1)]
        assert [f[0] == 1.0 for f in flags] == want_w and all(f[1] == 1.0 for f in flags), (w, flags)
        ratios[f"W={w or 'all'}"] = norm2(Z32.astype(LD) - Z) / zn / e32
    unit2_of = lambda k: (norm2(B[:, :k]) ** 2 * (1e6 ** (np.arange(k) % 3 - 1.0))).astype(np.float64)
    for k in (2, 4, 8):
        for w in ("none", None):
            env = {} if w is None else {"PADNE_AMG_W": w}
            Zb, _ = applied(env, lambda m: m.amg_apply_batch(np.ascontiguousarray(B[:, :k].T), unit2_of(k)).T)
            ratios[f"batch{k},W={w or 'all'}"] = norm2(Zb.astype(LD) - Z[:, :k]) / zn[:k] / e32[:k]
    worst = {k: float(v.max()) for k, v in ratios.items()}
    report.append("  f32 cycle, worst error / plain float32 error (right-hand side): "
                  + ", ".join(f"{k} {v:.2f} ({int(np.argmax(ratios[k]))})" for k, v in worst.items()))
    report.append(f"  plain float32 error {float(e32.min()):.1e} .. {float(e32.max()):.1e}")
    print("\n".join(report))
    assert ok64, f"double-precision cycle outside its envelope: {worst64:.3g} x"
    assert max(worst.values()) <= F32_FACTOR, worst
    singles = [worst[f"W={w}"] for w in ("none", "fine", "all")]
    assert max(singles) <= F32_FACTOR * min(singles), f"the up-leg forms differ by more than {F32_FACTOR} x: {worst}"


def test_nothing_is_kept_without_the_switch(ctx, switches):
    """Without PADNE_AMG_KEEP the levels keep neither array (the probe says so), the scalars are there all the same; the probe
    refuses a wrong size, an unknown array, a level that does not exist and a matrix without a hierarchy."""
    from padne_amd import _hip
    A = R.layered_matrix(2, 40, 30, 4)
    d = ctx.csr_from_scipy(A)
    try:
        out = np.zeros(4)
        lib, P = ctx._lib, _hip._P
        assert lib.padne_test_amg_state(ctx._h, d._h, 0, 2, out.ctypes.data_as(P), out.nbytes) == _hip.E_INVALID      # no hierarchy yet
        d.amg_apply(np.ones(A.shape[0]))
        assert len(d.amg_shapes()) == 2
        lam, jac, _, _ = d.amg_state(0, "SCALARS")
        assert lam > 1 and abs(jac * 0.55 * lam - 1) < 1e-15
        buf = np.zeros(A.shape[0], np.int32)
        assert lib.padne_test_amg_state(ctx._h, d._h, 0, 0, buf.ctypes.data_as(P), buf.nbytes) == _hip.E_INVALID      # not kept
        assert lib.padne_test_amg_state(ctx._h, d._h, 0, 1, buf.ctypes.data_as(P), A.shape[0]) == _hip.E_INVALID
        assert lib.padne_test_amg_state(ctx._h, d._h, 0, 2, out.ctypes.data_as(P), 24) == _hip.E_INVALID             # size
        assert lib.padne_test_amg_state(ctx._h, d._h, 0, 3, out.ctypes.data_as(P), 32) == _hip.E_INVALID             # array
        assert lib.padne_test_amg_state(ctx._h, d._h, 2, 2, out.ctypes.data_as(P), 32) == _hip.E_INVALID             # level
    finally:
        d.close()
    switches.set("PADNE_AMG_KEEP", "1")
    d = ctx.csr_from_scipy(A)
    try:
        d.amg_apply(np.ones(A.shape[0]))
        agg, root = d.amg_state(0, "AGG"), d.amg_state(0, "ROOT")
        assert agg.min() == 0 and set(np.unique(root)) == {0, 1}
        buf = np.zeros(A.shape[0] + 1, np.int32)
        assert ctx._lib.padne_test_amg_state(ctx._h, d._h, 0, 0, buf.ctypes.data_as(_hip._P), buf.nbytes) == _hip.E_INVALID
    finally:
        d.close()

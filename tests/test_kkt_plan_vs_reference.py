"""Every stage of the padne_kkt plan (csrc/kkt.hip) against its contract in np.longdouble (tests/kkt_ref.py; needs an MI355X).

One KktPlan call at a time; after it the plan's device arrays are read through padne_test_kkt_state (include/padne_hip_probe.h)
and held to the reference, stage by stage (u = 2^-53; m_i, E_i and the sums over reduced rows: kkt_ref.py):

    map        IMAP / SRC_OF exact integers (a valid renumbering for a host map or the strip order, P taken from it)
    matrix     reduced_matrix(): pattern inside P^T |L| P, sorted, |A - A_ref| <= (q + 1) u sum|terms|, symmetric to twice that
    b          bit for bit without known parts (-r[src], then -= r_i over the further members, ascending); with them
               |B - b_ref| <= u sum(m_i + 2) sum(E_i); the extras bit for bit (additions in list order)
    zero       Y exactly zero where B is exactly zero
    solve      ||A_ref Y_j - B_j|| <= 4 rtol_used ||B_j|| in longdouble (rtol = 1e-10; the rule of padne_hip.h for rtol_used)
    expand     V = c + Y[imap] and Z_k = Y[n_cols + k][imap] bit for bit, from the device's own Y; spare columns zero
    probes     |probe - rho_ref| <= (m_i + 2) u E_i, |probe_k - (L Z_k)_i| <= (m_i + 1) u sum|L_ik Z_k|, from the device's V, Z
    stage 2    V_host bit for bit V + coeff Z_k (multiply, add, k ascending), mult_val at mult_idx; the norm within
               ||e_j|| + (n + 8) u norm_ref_j of the longdouble norm of the returned V; constraint rows to 4u(|c_p| + |c_n| + |y|)
               (|y|: everything added to the known parts, |Y_j[t]| + sum_k |coeff_jk Z_k|)

probe_out and V_host lie between sentinel margins; the C entries are called directly (ctx._lib) for that.

No bound is a measured number.  Measured on an MI355X (the device's worst ratio to each bound over all cases of this file):

    check          worst ratio   where the bound comes from
    matrix         0.33          (q + 1) u sum|terms| per entry of A
    symmetry       0.19          twice that
    b              0.32          u sum(m_i + 2) sum(E_i), blocks with known parts (without them: bit for bit)
    solve          0.18          4 rtol_used ||B_j||
    probes         0.39          (m_i + 2) u E_i
    extra probes   0.37          (m_i + 1) u sum|L_ik Z_k|
    norm           0.081         ||e_j|| + (n + 8) u norm_ref_j
    constraint     0.74          4u(|c_p| + |c_n| + |y|)

(the float64 numpy restatement of tests/test_kkt_ref_host.py: b 0.12, probes 0.054, norm 0.019 on its three small systems.)  The
constraint bound is a theorem without regulators (two roundings, 2u); with K of them every potential takes K more additions
and the worst case is (K + 2) 2u -- at K = 2 the device reaches 0.74 of 4u.  Every bit-for-bit check holds as it stands.

Shown able to fail, in a scratch library (one perturbation of kkt.hip each, not committed):

    kkt_gidx with the row stride min(n_cols, width) instead of the group's width (n_cols itself would write out of bounds
        for 9 and more columns): the forest at 3 and 5 columns red (C is not the scattered known part), 1, 2, 4, 8, 9, 11, 16,
        17 green -- there the two coincide
    kkt_rhs_tied starting at e0 + 1: the forest red at every width (b: 6e14 of its bound), the block without known parts red
        (not bit for bit), the large system red with and without known parts (its one tied pair)
    i < min(P, 256) in kkt_fold: the three large cases red (norm: 7 to 89 times its bound), every smaller system green
    k < n_extra - 1 in kkt_add_extras: every case with a regulator red (stage 2 is not V + coeff Z), voltage_source green
    lo < n_elim - 1 in kkt_build_imap: voltage_source red (IMAP); the forest stays green -- its last eliminated potential is
        a tied member, whose entry kkt_tie_members overwrites with its representative's number
"""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H
import kkt_ref as K
from oracle import padne_oracle as O
from padne_amd import _hip, mesh, reduction, solver, synthetic

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
RTOL = 1e-10
SENTINEL = -7.25e300
MARGIN = 64
SIGMA = 2082.5
_PI64, _PI32, _PF64 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
WORST = {}


def note(check, ratio):
    WORST[check] = max(WORST.get(check, 0.0), float(ratio))
    print(f"RATIO {check} {float(ratio):.3g}")


def held(check, diff, bound):
    ratio = K.worst_ratio(diff, bound)
    note(check, ratio)
    assert ratio <= 1.0, f"{check}: {ratio:.3g} of its bound"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def ptr(a, typ):
    return None if a is None or a.size == 0 else a.ctypes.data_as(typ)


def guarded(n):
    buf = np.full(n + 2 * MARGIN, SENTINEL)
    return buf, buf[MARGIN:MARGIN + n]


def intact(buf, n):
    return bool((buf[:MARGIN] == SENTINEL).all() and (buf[MARGIN + n:] == SENTINEL).all())


# ---- systems (built once per module) -------------------------------------------------------------------------------------

class System:
    """A KKT matrix L in the reference's layout with what the plan's callers derive from it."""

    def __init__(self, L, r, n_pot=None, with_layout=True, scale_own_r=False):
        L = sp.csr_matrix(L)
        L.sum_duplicates()
        L.sort_indices()
        self.L, self.r, self.N = L, np.asarray(r, dtype=np.float64), L.shape[0]
        self.layout = self.pins = None
        if with_layout:
            self.layout = reduction.infer_layout(L, self.r, n_pot)
            self.pins = reduction.floating_component_pins(self.layout.n_potential, self.layout.ground_constraint.p,
                                                          self.layout.constraints, matrix=L)
        self.n_pot = self.layout.n_potential if with_layout else int(n_pot)
        self._dev = None
        # (a fixture may hang copper on the ground through one large resistor: currents between random potentials would
        #  drive y to 1e6 ||b|| / ||A|| there and the float64 residual of ANY solve above 4 rtol ||b||)
        self.scale_own_r = scale_own_r

    def dev(self, ctx):
        if self._dev is None:
            self._dev = ctx.csr_from_scipy(self.L)
        return self._dev

    def block(self, k, seed, zero_cols=(), no_known=False, own_r=False):
        """k right-hand sides: six currents between random potentials (a fixture: its own, scaled), dyadic source voltages (sums of hundreds of them are exact, so
        the known parts of a long chain satisfy their constraint rows exactly); `own_r`: column 0 is the system's r."""
        rng = np.random.default_rng(seed)
        R = np.zeros((self.N, k))
        sources = [(cst.p, cst.n) for cst in self.layout.constraints if cst.n >= 0]
        for j in range(k):
            if self.scale_own_r:                           # a fixture: its own currents, scaled
                R[:self.n_pot, j] = self.r[:self.n_pot] * rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
                continue
            # balanced currents: what flows in flows out, as with real sources
            into = rng.choice(self.n_pot, min(12, self.n_pot - self.n_pot % 2), replace=False)
            if sources:                                    # (one of them between the terminals of the last source)
                rest = into[~np.isin(into, sources[-1])]
                into = np.concatenate([[sources[-1][0]], rest[:len(into) - 2], [sources[-1][1]]])
            amps = rng.uniform(0.5, 2.0, len(into) // 2)
            R[into[:len(into) // 2], j] += amps
            R[into[len(into) // 2:], j] -= amps
        for cst in self.layout.constraints:
            if cst.n >= 0 and not no_known:
                R[cst.index] = rng.integers(-256, 257, k) / 64.0
        if own_r:
            R[:, 0] = self.r
        for j in zero_cols:
            R[:, j] = 0.0
        return R

    def lists(self, R):
        """(red, known_idx, known_val, extras, probes) as solve_system makes them for the block R."""
        red, kidx, kval = reduction.build_block_reduction(self.layout, {c.index: R[c.index, :] for c in self.layout.constraints},
                                                          self.pins)
        return red, kidx, kval, red.regulator_columns, np.asarray(red.probe_members, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def golden(name):
    g = H.load_golden(name)
    return System(H.golden_L(g), g["r"], scale_own_r=True)


@functools.lru_cache(maxsize=None)
def forest(kind="plain"):
    """40 x 30 grid, voltage sources between shuffled vertices: a floating chain of 300, a chain of 40 from the ground, 270
    separate pairs, a current source and a resistor; N = 1811, 611 eliminated, 570 tied members in 271 groups (more than one
    workgroup of groups, the longest with 300 further members), 610 known parts, 882 probes.  "regs": two regulators (one
    gain row of the second is eliminated and dropped); "zero_gain": the second regulator's gain rows are both known potentials,
    its column projects to zero."""
    xy, tri = synthetic.jittered_grid(40, 30, seed=21)
    nv = len(xy)
    perm = np.random.default_rng(31).permutation(nv)
    chain_g, chain_f, pairs, spare = perm[:41], perm[41:342], perm[342:882].reshape(270, 2), perm[882:]
    ties = [(int(chain_g[i + 1]), int(chain_g[i])) for i in range(40)] + [(int(chain_f[i + 1]), int(chain_f[i])) for i in range(300)]
    ties += [(int(a), int(b)) for a, b in pairs]
    els = [("V", p, n, 0.0, nv + q) for q, (p, n) in enumerate(ties)]
    els += [("I", int(spare[0]), int(spare[1]), 1.0), ("R", int(spare[2]), int(spare[3]), 0.5)]
    iv = nv + len(ties)
    s = [int(x) for x in spare]
    if kind == "regs":
        els += [("REG", s[4], s[5], s[6], s[7], 0.5, 0.25, iv), ("REG", s[8], s[9], s[10], int(chain_g[5]), 1.0, -0.5, iv + 1)]
    elif kind == "zero_gain":
        els += [("REG", s[4], s[5], s[6], s[7], 0.5, 0.25, iv), ("REG", s[8], s[9], int(chain_g[3]), int(chain_g[7]), 1.0, -0.5, iv + 1)]
    L, r = O.assemble_system([(xy, tri, SIGMA)], 0, els, int(chain_g[0]))
    return System(L, r, nv)


def stamped(lap, n_pot, sources, ground):
    """[lap, stamps; stamps^T, 0] in the reference's layout, assembled from triples (vectorised: the large system)."""
    n_lap = lap.shape[0]
    N = n_pot + len(sources) + 1
    coo = lap.tocoo()
    rows, cols, vals = [coo.row.astype(np.int64)], [coo.col.astype(np.int64)], [coo.data]
    for q, (p, n) in enumerate(sources):
        iv = n_pot + q
        rows.append(np.array([iv, iv, p, n])); cols.append(np.array([p, n, iv, iv])); vals.append(np.array([1.0, -1.0, 1.0, -1.0]))
    rows.append(np.array([N - 1, ground])); cols.append(np.array([ground, N - 1])); vals.append(np.array([1.0, 1.0]))
    assert n_lap == n_pot
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N))


@functools.lru_cache(maxsize=None)
def large():
    """600 x 450 vertices, two sources from the ground, one tied pair in the rows of the last workgroup: N = 270004 > 262144 =
    1024 workgroups of 256, so every elementwise kernel takes a second trip of its grid-stride loop."""
    xy, tri = synthetic.jittered_grid(600, 450, seed=3)
    nv = len(xy)
    lap = (SIGMA * O.laplace_operator(xy, tri, validate=False)).tocsr()
    L = stamped(lap, nv, [(1000, 7), (200000, 1000), (nv - 3, nv - 100)], 7)
    r = np.zeros(L.shape[0])
    return System(L, r, nv)


@functools.lru_cache(maxsize=None)
def edge_base():
    xy, tri = synthetic.jittered_grid(17, 16, seed=9)
    return (SIGMA * O.laplace_operator(xy, tri).tocsr()[1:, 1:]).tocsr()          # negative definite, like its leading blocks


EDGE_KINDS = ("ground_only", "first", "last", "all_but_one", "none_free")


@functools.lru_cache(maxsize=None)
def edge(N, n_mult, kind):
    """(System without layout, elim, tied): leading block of the 17 x 16 grid operator with n_mult multiplier rows behind it."""
    n_pot = N - n_mult
    if n_mult == 0:
        L = edge_base()[:n_pot, :n_pot]
        return System(L, np.zeros(N), n_pot, with_layout=False), ([] if kind == "nothing" else list(range(n_pot))), []
    g = n_pot // 2
    sources = [(3, 10), (n_pot - 1, 20)] if n_mult == 3 else []
    L = stamped(edge_base()[:n_pot, :n_pot], n_pot, sources, g)
    tied = [(10, 3)] if n_mult == 3 else []
    elim = {"ground_only": {g}, "first": {0, g}, "last": {g, n_pot - 1}, "all_but_one": set(range(n_pot)) - {7},
            "none_free": set(range(n_pot))}[kind]
    if tied and kind in ("ground_only", "first", "last"):
        elim = elim | {10}
    else:
        tied = []
    return System(L, np.zeros(N), n_pot, with_layout=False), sorted(elim), tied


def delaunay_mesh(n_points, seed, hole):
    import scipy.spatial
    pts = np.random.default_rng(seed).uniform(0, 40, (n_points, 2))
    if hole:
        pts = pts[np.hypot(pts[:, 0] - 20, pts[:, 1] - 20) > 6.0]
    tri = scipy.spatial.Delaunay(pts).simplices.astype(np.int32)
    if hole:
        c = pts[tri].mean(axis=1)
        tri = tri[np.hypot(c[:, 0] - 20, c[:, 1] - 20) > 6.5]
    a, b, c = pts[tri[:, 0]], pts[tri[:, 1]], pts[tri[:, 2]]
    cross = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    tri[cross < 0] = tri[cross < 0][:, [0, 2, 1]]
    used = np.unique(tri)
    remap = -np.ones(len(pts), dtype=np.int64)
    remap[used] = np.arange(len(used))
    return pts[used], remap[tri].astype(np.int32)


# ---- the C entries, called directly ----------------------------------------------------------------------------------------

def extras_arrays(extras):
    p, rows, vals = [0], [], []
    for col in extras:
        rows += [int(x) for x in col]
        vals += [float(v) for v in col.values()]
        p.append(len(rows))
    return np.array(p, dtype=np.int64), np.array(rows, dtype=np.int64), np.array(vals, dtype=np.float64)


ARG_TYPES = dict(r=_PF64, kidx=_PI64, kval=_PF64, eptr=_PI64, erow=_PI64, eval=_PF64, pidx=_PI64, pout=_PF64, row=_PI64,
                 col=_PI32, val=_PF64)


def stage1(ctx, plan, entry, R, kidx, kval, extras, probes, rtol=RTOL, target=0.0, override=None):
    """(rc, probe values (n_cols + n_extra, n_probe)) of one stage-1 call; probe_out lies between sentinel margins.  `entry`:
    "single" (padne_kkt_solve), "block" or "coo".  `override`: raw arguments (arrays, None, integers, handles) that replace
    the well-formed ones -- the argument errors."""
    R = np.ascontiguousarray(R, dtype=np.float64)
    n_cols = R.shape[1]
    kidx = np.ascontiguousarray(kidx, dtype=np.int64)
    kval = np.ascontiguousarray(kval, dtype=np.float64).reshape(n_cols, len(kidx))
    eptr, erow, eval_ = extras_arrays(extras)
    probes = np.ascontiguousarray(probes, dtype=np.int64)
    n_out = (n_cols + len(extras)) * len(probes)
    buf, out = guarded(n_out)
    opts = _hip.CsrMatrix._opts(rtol, 0.0, 200000, 0, False, precond="amg", rebuild=False)
    info = _hip.SolveInfo()
    a = dict(ctx=ctx._h, plan=plan._h, n_cols=n_cols, r=R, n_known=len(kidx), kidx=kidx, kval=kval, n_extra=len(extras),
             eptr=eptr, erow=erow, eval=eval_, n_probe=len(probes), pidx=probes, pout=out, opts=C.byref(opts),
             target=float(target), info=C.byref(info))
    if entry == "coo":
        rr, cc = np.nonzero(R)
        a.update(n_entries=len(rr), row=rr.astype(np.int64), col=cc.astype(np.int32), val=np.ascontiguousarray(R[rr, cc]))
    a.update(override or {})

    def arg(name):
        x = a[name]
        if isinstance(x, np.ndarray):
            return x.ctypes.data_as(ARG_TYPES[name]) if x.size else None
        return x
    common = [arg(n) for n in ("n_known", "kidx", "kval", "n_extra", "eptr", "erow", "eval", "n_probe", "pidx", "pout", "opts",
                               "target", "info")]
    if a["eptr"] is eptr:
        common[4] = eptr.ctypes.data_as(_PI64)
    lib = ctx._lib
    if entry == "single":
        assert n_cols == 1
        rc = lib.padne_kkt_solve(arg("ctx"), arg("plan"), arg("r"), *common)
    elif entry == "block":
        rc = lib.padne_kkt_solve_block(arg("ctx"), arg("plan"), arg("n_cols"), arg("r"), *common)
    else:
        rc = lib.padne_kkt_solve_block_coo(arg("ctx"), arg("plan"), arg("n_cols"), arg("n_entries"), arg("row"), arg("col"),
                                           arg("val"), *common)
    assert intact(buf, n_out), "stage 1 wrote outside probe_out"
    return rc, out.reshape(n_cols + len(extras), len(probes)).copy()


def stage2(ctx, plan, entry, N, n_cols, coeff, midx, mval, override=None):
    """(rc, V_host (N, n_cols), norms [n_cols]) of one stage-2 call."""
    coeff = np.ascontiguousarray(coeff, dtype=np.float64).reshape(n_cols, -1)
    midx = np.ascontiguousarray(midx, dtype=np.int64)
    mval = np.ascontiguousarray(mval, dtype=np.float64).reshape(n_cols, len(midx))
    vbuf, v = guarded(N * n_cols)
    nbuf, norms = guarded(n_cols)
    a = dict(ctx=ctx._h, plan=plan._h, n_cols=n_cols, n_extra=coeff.shape[1], coeff=ptr(coeff, _PF64), n_mult=len(midx),
             midx=ptr(midx, _PI64), mval=ptr(mval, _PF64), v=v.ctypes.data_as(_PF64), norms=norms.ctypes.data_as(_PF64))
    a.update(override or {})
    lib = ctx._lib
    if entry == "single":
        rc = lib.padne_kkt_finish(a["ctx"], a["plan"], a["n_extra"], a["coeff"], a["n_mult"], a["midx"], a["mval"], a["v"], a["norms"])
    else:
        rc = lib.padne_kkt_finish_block(a["ctx"], a["plan"], a["n_cols"], a["n_extra"], a["coeff"], a["n_mult"], a["midx"],
                                        a["mval"], a["v"], a["norms"])
    assert intact(vbuf, N * n_cols) and intact(nbuf, n_cols), "stage 2 wrote outside its outputs"
    return rc, v.reshape(N, n_cols).copy(), norms.copy()


# ---- the checks ------------------------------------------------------------------------------------------------------------

def check_map(plan, S, elim, tied, exact):
    """IMAP and SRC_OF; returns the kkt_ref.Reference of the plan (P from the device's map when the numbering is the plan's own)."""
    N, n_pot = S.N, S.n_pot
    imap = plan.state("IMAP", N)
    src = plan.state("SRC_OF", plan.n_free)
    want = K.index_map(N, n_pot, elim, tied)
    if exact:
        assert np.array_equal(imap, want)
    members = np.array([m for m, _ in tied], dtype=np.int64)
    reps = np.array([r for _, r in tied], dtype=np.int64)
    gone = np.setdiff1d(np.asarray(elim, dtype=np.int64), members)
    assert (imap[n_pot:] == -1).all() and (imap[gone] == -1).all()
    own = np.setdiff1d(np.arange(n_pot), np.asarray(elim, dtype=np.int64))
    assert len(own) == plan.n_free and np.array_equal(np.sort(imap[own]), np.arange(plan.n_free))
    assert np.array_equal(imap[members], imap[reps])
    # SRC_OF[t]: the one potential that owns t (for a tied group its representative, which is not eliminated)
    assert np.array_equal(imap[src], np.arange(plan.n_free)) and np.isin(src, own).all()
    with pytest.raises(ValueError):
        plan.state("IMAP", N + 1)
    return K.Reference(S.L, n_pot, imap=imap, n_free=plan.n_free), imap.astype(np.int64), src.astype(np.int64)


def check_matrix(plan, ref):
    A = plan.reduced_matrix().to_scipy()
    nf = ref.n_free
    assert A.shape == (nf, nf)
    t, u, val, q, mass = ref.reduced_matrix()
    rows = np.repeat(np.arange(nf, dtype=np.int64), np.diff(A.indptr))
    cols = A.indices.astype(np.int64)
    if len(cols):
        inside = np.diff(cols) > 0
        assert (inside | (np.diff(rows) > 0)).all(), "indices not sorted inside a row"
    keys, ref_keys = rows * max(nf, 1) + cols, t * max(nf, 1) + u
    pos = np.searchsorted(ref_keys, keys)
    assert (pos < len(ref_keys)).all() and np.array_equal(ref_keys[pos], keys), "entry outside the pattern of P^T |L| P"
    got = np.zeros(len(ref_keys))
    got[pos] = A.data
    bound = (q + 1) * U * mass
    held("matrix", got - val, bound)
    AT = A.T.tocsr()
    AT.sort_indices()
    gotT = np.zeros(len(ref_keys))
    rowsT = np.repeat(np.arange(nf, dtype=np.int64), np.diff(AT.indptr))
    posT = np.searchsorted(ref_keys, rowsT * max(nf, 1) + AT.indices.astype(np.int64))
    assert (posT < len(ref_keys)).all()
    gotT[posT] = AT.data
    held("symmetry", got - gotT, 2 * bound)
    return t, u, val


def expected_rhs_bits(R, imap, src, n_free):
    """b without known parts, in float64 and the kernel's promised order: -r[src], then -= r_i over the further members,
    ascending."""
    b = -R[src]                                            # (n_free, k)
    rest = np.flatnonzero(imap >= 0)
    rest = rest[src[imap[rest]] != rest]                   # the further members, ascending
    tgt = imap[rest]
    order = np.argsort(tgt, kind="stable")
    rest, tgt = rest[order], tgt[order]
    first = np.flatnonzero(np.concatenate([[True], tgt[1:] != tgt[:-1]])) if len(tgt) else np.zeros(0, dtype=np.int64)
    rank = np.arange(len(tgt)) - np.repeat(first, np.diff(np.append(first, len(tgt)))) if len(tgt) else tgt
    for step in range(int(rank.max()) + 1 if len(tgt) else 0):
        sel = rank == step
        b[tgt[sel]] = b[tgt[sel]] - R[rest[sel]]
    return b


def run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, *, entry="block", red=None, seed=0, target=0.0, A=None,
        label=""):
    """One stage 1 and one stage 2 on `plan`, every stage check after each.  `red`: the multipliers are recovered as
    solve_system does and the constraint rows of the final V are checked; else stage 2 gets random coefficients and
    multipliers (its arithmetic is checked bit for bit either way).  Returns the device's B (for comparisons between entries)."""
    N, nf, n_pot = S.N, ref.n_free, S.n_pot
    R = np.ascontiguousarray(R, dtype=np.float64)
    n_cols, n_extra, n_rhs = R.shape[1], len(extras), R.shape[1] + len(extras)
    width = K.block_width(n_cols)
    kidx = np.asarray(kidx, dtype=np.int64)
    kval = np.asarray(kval, dtype=np.float64).reshape(n_cols, len(kidx))
    rc, probe = stage1(ctx, plan, entry, R, kidx, kval, extras, probes, target=target)
    assert rc == _hip.OK, ctx._lib.padne_last_error()
    B = plan.state("B", n_rhs * nf).reshape(n_rhs, nf)
    Y = plan.state("Y", n_rhs * nf).reshape(n_rhs, nf)
    Vflat = plan.state("V", N * width)
    Z = plan.state("Z", n_extra * N).reshape(n_extra, N)
    for bad in (n_rhs * nf + 1, 0 if n_rhs * nf else 1):
        with pytest.raises(ValueError):
            plan.state("B", bad)
    # -- known part
    c = ref.known(kidx, kval, n_cols)
    c64 = c.astype(np.float64)
    if len(kidx):
        Cflat = plan.state("C", N * width)
        assert same_bits(K.from_layout(Cflat, N, n_cols), c64) and not K.spare_entries(Cflat, N, n_cols).any()
    else:
        with pytest.raises(ValueError):
            plan.state("C", N * width)
    # -- right-hand side
    if nf:
        if len(kidx):
            b_ref, b_bound = ref.rhs(R, c)
            held("b", B[:n_cols].T - b_ref, b_bound)
        else:
            assert same_bits(B[:n_cols].T, expected_rhs_bits(R, imap, src, nf)), "b without known parts is not bit for bit"
        want = np.zeros((n_extra, nf))
        for k, col in enumerate(extras):
            for row, val in col.items():
                if imap[row] >= 0:
                    want[k, imap[row]] += float(val)
        assert same_bits(B[n_cols:], want), "extra right-hand sides"
    # -- zero columns, solve
    norms_b = np.sqrt((B.astype(LD) ** 2).sum(axis=1))
    live = np.flatnonzero((B != 0).any(axis=1))
    for j in np.setdiff1d(np.arange(n_rhs), live):
        assert not Y[j].any() and not np.signbit(Y[j]).any(), f"Y of the zero column {j}"
    rtol_used = RTOL
    if target > 0 and len(live) and RTOL * float(norms_b.max()) > target:
        rtol_used = max(target / float(norms_b.max()), 2e-15)
    if len(live):
        t, u, val = A
        AY = K.segment_sum(t, val[:, None] * Y[live].T.astype(LD)[u], nf)
        res = np.sqrt(((AY - B[live].T) ** 2).sum(axis=0))
        held("solve", res, 4 * rtol_used * norms_b[live])
    # -- expansion, from the device's own Y
    V1 = K.from_layout(Vflat, N, n_cols)
    free = imap >= 0
    want = c64.copy()
    want[free] = c64[free] + Y[:n_cols].T[imap[free]]
    assert same_bits(V1, want), "V != c + P Y"
    assert not K.spare_entries(Vflat, N, n_cols).any(), "spare columns of the widened group"
    wantZ = np.zeros((n_extra, N))
    wantZ[:, free] = 0.0 + Y[n_cols:][:, imap[free]]
    assert same_bits(Z, wantZ), "Z != P z"
    # -- probes, from the device's own V and Z
    if len(probes):
        rho_ref, rho_bound = ref.probes(R, V1, probes)
        held("probes", probe[:n_cols].T - rho_ref, rho_bound)
        if n_extra:
            lz_ref, lz_bound = ref.extra_probes(Z.T, probes)
            held("extra probes", probe[n_cols:].T - lz_ref, lz_bound)
    # -- stage 2
    rng = np.random.default_rng(seed + 1000)
    if red is not None:
        coeff, mult = reduction.recover_currents(red, [int(x) for x in probes], probe, n_cols)
        midx = np.asarray(sorted(mult[0]), dtype=np.int64)
        mval = np.array([[m[int(i)] for i in midx] for m in mult], dtype=np.float64).reshape(n_cols, len(midx))
    else:
        coeff = rng.uniform(-2, 2, (n_cols, n_extra))
        midx = np.arange(n_pot, N, dtype=np.int64)
        mval = rng.uniform(-3, 3, (n_cols, len(midx)))
    coeff = np.asarray(coeff, dtype=np.float64).reshape(n_cols, n_extra)
    rc, V, norms = stage2(ctx, plan, "single" if entry == "single" else "block", N, n_cols, coeff, midx, mval)
    assert rc == _hip.OK, ctx._lib.padne_last_error()
    want = V1.copy()
    for j in range(n_cols):
        for k in range(n_extra):
            want[:, j] = want[:, j] + coeff[j, k] * Z[k]
    want[midx] = mval.T
    assert same_bits(V, want), "stage 2 is not V + coeff Z, mult_val at mult_idx"
    assert same_bits(K.from_layout(plan.state("V", N * width), N, n_cols), want), "the V left on the device"
    if len(kidx) and n_cols in (1, 2, 4, 8):                # c survives stage 2 where the two layouts coincide ...
        assert same_bits(K.from_layout(plan.state("C", N * width), N, n_cols), c64)
    else:                                                  # ... and is the caller's-layout copy of V otherwise: refused
        with pytest.raises(ValueError):
            plan.state("C", N * width)
    norm_ref, norm_bound = ref.residual_norms(R, V)
    held("norm", norms - norm_ref, norm_bound)
    if red is not None:
        cons = S.layout.constraints
        p = np.array([cst.p for cst in cons], dtype=np.int64)
        n = np.array([cst.n for cst in cons], dtype=np.int64)
        idx = np.array([cst.index for cst in cons], dtype=np.int64)
        tp = imap[p]
        y = np.where((tp >= 0)[:, None], np.abs(Y[:n_cols].T[np.maximum(tp, 0)]) + np.abs(Z.T[p]) @ np.abs(coeff).T, 0.0) if nf else 0.0
        two = (n >= 0)[:, None]
        held("constraint", V[p] - np.where(two, V[n], 0.0) - R[idx], 4 * U * (np.abs(c64[p]) + np.where(two, np.abs(c64[n]), 0.0) + y))
    return B


def list_plan(ctx, S, red):
    plan = _hip.KktPlan(S.dev(ctx), S.n_pot, red.elim, red.tied, red.n_free)
    ref, imap, src = check_map(plan, S, red.elim, red.tied, exact=True)
    return plan, ref, imap, src


# ---- golden fixtures -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["voltage_source", "regulator", "glue_sources", "lumped_only", "two_layer_via"])
def test_golden_fixture_stage_by_stage(ctx, name):
    S = golden(name)
    R1 = S.r[:, None].copy()
    red, kidx, kval, extras, probes = S.lists(R1)
    plan, ref, imap, src = list_plan(ctx, S, red)
    if name == "lumped_only":
        assert red.n_free == 1
    A = check_matrix(plan, ref)
    run(ctx, plan, S, ref, imap, src, R1, kidx, kval, extras, probes, entry="single", red=red, A=A)
    R = S.block(5, seed=len(name), own_r=True)
    red5, kidx, kval, extras, probes = S.lists(R)
    assert np.array_equal(red5.elim, red.elim) and red5.tied == red.tied
    B = run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red5, A=A)
    # the tightened tolerance: an absolute target a hundred times below rtol ||b||
    run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red5, A=A,
        target=1e-12 * float(np.sqrt((B.astype(LD) ** 2).sum(axis=1)).max()))
    plan.close()


# ---- the forest: long tied lists, every width of a last group --------------------------------------------------------------

@pytest.fixture(scope="module")
def forest_plan(ctx):
    S = forest("regs")
    red = S.lists(S.block(1, 0))[0]
    assert S.N == 1813 and len(red.elim) == 613 and len(red.tied) == 572 and len({r for _, r in red.tied}) == 273
    assert max(np.bincount([r for _, r in red.tied])) == 300 and len(red.regulators) == 2
    plan, ref, imap, src = list_plan(ctx, S, red)
    A = check_matrix(plan, ref)
    yield S, plan, ref, imap, src, A
    plan.close()


def test_forest_counts_without_regulators():
    S = forest("plain")
    R = S.block(4, 0)
    red, kidx, kval, extras, probes = S.lists(R)
    assert S.N == 1811 and len(red.elim) == 611 and len(red.tied) == 570 and len({r for _, r in red.tied}) == 271
    assert max(np.bincount([r for _, r in red.tied])) == 300 and len(kidx) == 610 and len(probes) == 882 and not extras


@pytest.mark.parametrize("n_cols", [1, 2, 3, 4, 5, 8, 9, 11, 16, 17])
def test_forest_column_counts(forest_plan, ctx, n_cols):
    S, plan, ref, imap, src, A = forest_plan
    R = S.block(n_cols, seed=n_cols)
    red, kidx, kval, extras, probes = S.lists(R)
    assert len(probes) == 886 and len(extras) == 2
    run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=A, seed=n_cols)


def test_forest_dense_and_coo_entries_form_the_same_bits(forest_plan, ctx):
    S, plan, ref, imap, src, A = forest_plan
    R = S.block(11, seed=77)
    red, kidx, kval, extras, probes = S.lists(R)
    B_dense = run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=A)
    B_coo = run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=A, entry="coo")
    assert same_bits(B_dense, B_coo)


def test_forest_zero_columns_are_packed_around(forest_plan, ctx):
    S, plan, ref, imap, src, A = forest_plan
    R = S.block(11, seed=5, zero_cols=(0, 3, 10))
    red, kidx, kval, extras, probes = S.lists(R)
    B = run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=A)
    assert not B[[0, 3, 10]].any() and B[[1, 2, 4, 9]].any(axis=1).all()
    run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=A, entry="coo")


def test_forest_gain_column_that_projects_to_zero(ctx):
    S = forest("zero_gain")
    R = S.block(3, seed=9)
    red, kidx, kval, extras, probes = S.lists(R)
    plan, ref, imap, src = list_plan(ctx, S, red)
    assert len(extras) == 2 and all(imap[row] < 0 for row in extras[1])
    B = run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=check_matrix(plan, ref))
    assert B[3].any() and not B[4].any()
    plan.close()


def test_one_plan_through_shrinking_and_growing_blocks(ctx):
    """The buffers only grow while the strides follow the current block: 1 column, 11 with extras, 3 without known parts, 1
    with known parts -- on ONE plan, every stage check after each; C is refused after the third."""
    S = forest("regs")
    red = S.lists(S.block(1, 0))[0]
    plan, ref, imap, src = list_plan(ctx, S, red)
    A = check_matrix(plan, ref)
    for n_cols, no_known, seed in ((1, False, 1), (11, False, 2), (3, True, 3), (1, False, 4)):
        R = S.block(n_cols, seed=seed, no_known=no_known)
        red, kidx, kval, extras, probes = S.lists(R)
        assert (len(kidx) == 0) == no_known
        run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=A, seed=seed,
            entry="single" if seed == 4 else "block")
        if no_known:
            with pytest.raises(ValueError):
                plan.state("C", S.N * K.block_width(n_cols))
    plan.close()


# ---- hand-made lists at the edges ------------------------------------------------------------------------------------------

EDGES = [(1, 0, "nothing"), (1, 0, "none_free")]
EDGES += [(N, 1, kind) for N in (255, 256, 257) for kind in EDGE_KINDS]
EDGES += [(N, 3, kind) for N in (255, 256, 257) for kind in ("ground_only", "last")]


@pytest.mark.parametrize("N,n_mult,kind", EDGES)
def test_list_edges(ctx, N, n_mult, kind):
    S, elim, tied = edge(N, n_mult, kind)
    n_pot = N - n_mult
    n_free = n_pot - len(elim)
    plan = _hip.KktPlan(S.dev(ctx), n_pot, elim, tied, n_free)
    ref, imap, src = check_map(plan, S, elim, tied, exact=True)
    A = check_matrix(plan, ref)
    rng = np.random.default_rng(N + n_mult)
    for n_cols in (3, 1):
        R = rng.uniform(-1, 1, (N, n_cols))
        kidx = np.asarray(elim, dtype=np.int64)
        kval = rng.uniform(-2, 2, (n_cols, len(kidx)))
        rows = [0, n_pot - 1, N - 1, n_pot // 3]
        extras = [{rows[0]: 0.5, rows[2]: -0.5}, {rows[1]: 1.5, rows[3]: 0.25, rows[0]: -1.0}] if N > 1 else [{0: 0.5}]
        probes = np.unique(np.concatenate([rng.integers(0, N, 9), [0, N - 1]]))
        run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, A=A, seed=n_cols)
        if n_free == 0:
            # nothing to solve for: stage 1 leaves c, stage 2 returns it with the multipliers
            _, V, _ = stage2_after(ctx, plan, S, R, kidx, kval, extras, probes, n_cols)
            c = ref.known(kidx, kval, n_cols).astype(np.float64)
            assert same_bits(V[:n_pot], c[:n_pot]) and (V[n_pot:] == 2.5).all()
    plan.close()


def stage2_after(ctx, plan, S, R, kidx, kval, extras, probes, n_cols):
    rc, _ = stage1(ctx, plan, "block", R, kidx, kval, extras, probes)
    assert rc == _hip.OK
    midx = np.arange(S.n_pot, S.N, dtype=np.int64)
    return stage2(ctx, plan, "block", S.N, n_cols, np.zeros((n_cols, len(extras))), midx, np.full((n_cols, len(midx)), 2.5))


# ---- large: the second trip of every grid-stride loop ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def large_plan(ctx):
    S = large()
    assert S.N > 262144
    red = S.lists(S.block(1, 0))[0]
    assert red.tied == [(S.n_pot - 3, S.n_pot - 100)]
    plan, ref, imap, src = list_plan(ctx, S, red)
    A = check_matrix(plan, ref)
    yield S, plan, ref, imap, src, A
    plan.close()


@pytest.mark.parametrize("n_cols", [1, 3])
def test_large_system(large_plan, ctx, n_cols):
    S, plan, ref, imap, src, A = large_plan
    R = S.block(n_cols, seed=40 + n_cols)
    red, kidx, kval, extras, probes = S.lists(R)
    run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=A)


def test_large_system_without_known_parts(large_plan, ctx):
    S, plan, ref, imap, src, A = large_plan
    R = S.block(3, seed=50, no_known=True)
    red, kidx, kval, extras, probes = S.lists(R)
    run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=A)


# ---- one system, three constructions of the plan ---------------------------------------------------------------------------

def test_plan_from_lists_host_map_and_strip_order(ctx):
    """The device-assembled system of test_strip_numbering_on_the_device_is_the_hosts_permutation: two shuffled Delaunay meshes,
    a source across them, an internal node on three resistors, the ground."""
    m1, m2 = delaunay_mesh(9000, seed=5, hole=True), delaunay_mesh(5000, seed=6, hole=False)
    meshes = [mesh.Mesh(*m1), mesh.Mesh(m2[0] * 0.7 + 3.0, m2[1])]
    n1, n2 = len(meshes[0].points), len(meshes[1].points)
    nv = n1 + n2
    n_pot, N = nv + 1, nv + 3
    stamps = solver.StampList(N)
    r = np.zeros(N)
    for a in (17, n1 + 40, n1 + 333):
        g = 1 / 0.25
        stamps.add(a, a, -g); stamps.add(a, nv, g); stamps.add(nv, nv, -g); stamps.add(nv, a, g)
    iv, p_, n_ = n_pot, 4321, n1 + 1234
    stamps.add(iv, p_, 1.0); stamps.add(iv, n_, -1.0); stamps.add(p_, iv, 1.0); stamps.add(n_, iv, -1.0)
    stamps.constraints.append(reduction.Constraint(index=iv, p=p_, n=n_, value=0.5))
    solver.setup_ground_node(3, stamps, r)
    Ldev = solver.assemble_from_arrays(meshes, [SIGMA, SIGMA / 2], stamps, n_pot)
    S = System(Ldev.tocsr(), r, n_pot)
    S._dev = Ldev.dev
    R = S.block(3, seed=12)
    red, kidx, kval, extras, probes = S.lists(R)
    assert red.tied
    host = reduction.build_block_reduction(S.layout, {c.index: R[c.index, :] for c in S.layout.constraints}, S.pins)[0]
    reduction.apply_locality_ordering(host, Ldev.xy, Ldev.mesh_offsets)
    plans = {"lists": _hip.KktPlan(Ldev.dev, n_pot, red.elim, red.tied, red.n_free),
             "host_map": _hip.KktPlan(Ldev.dev, n_pot, red.elim, red.tied, red.n_free, index_map=host.index_map),
             "strip": _hip.KktPlan(Ldev.dev, n_pot, red.elim, red.tied, red.n_free, strip_order=True)}
    maps = {}
    for form, plan in plans.items():
        ref, imap, src = check_map(plan, S, red.elim, red.tied, exact=form == "lists")
        maps[form] = imap
        run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=check_matrix(plan, ref))
    assert np.array_equal(maps["host_map"], host.index_map) and np.array_equal(maps["strip"], maps["host_map"])
    assert not np.array_equal(maps["strip"], maps["lists"])
    for plan in plans.values():
        plan.close()
    Ldev.close()


# ---- argument errors: refused on the host, and the plan is none the worse -------------------------------------------------

def test_create_refuses_malformed_lists(ctx):
    S = golden("regulator")
    red = S.lists(S.block(1, 0))[0]
    assert red.tied
    lib, dev, n_pot, N = ctx._lib, S.dev(ctx), S.n_pot, S.N
    elim, tm, tr = red.elim.copy(), np.array([m for m, _ in red.tied], np.int64), np.array([r for _, r in red.tied], np.int64)
    wide = ctx.csr_from_scipy(sp.csr_matrix(np.ones((2, 3))))

    def create(L=dev._h, n_pot=n_pot, elim=elim, tm=tm, tr=tr, n_free=red.n_free, n_elim=None, n_tied=None, out=True):
        h = C.c_void_p()
        rc = lib.padne_kkt_create(ctx._h, L, n_pot, len(elim) if n_elim is None else n_elim, ptr(elim, _PI64),
                                  len(tm) if n_tied is None else n_tied, ptr(tm, _PI64), ptr(tr, _PI64), None, n_free, 0,
                                  C.byref(h) if out else None)
        assert (rc == _hip.OK) == bool(h.value)
        if h.value:
            lib.padne_kkt_destroy(h)
        return rc
    free = np.setdiff1d(np.arange(n_pot), elim)
    others = np.setdiff1d(elim, tm)
    bad = {
        "null": dict(out=False),
        "not square": dict(L=wide._h),
        "n_potential": dict(n_pot=N + 1),
        "list sizes": dict(elim=elim[:0], n_free=n_pot),
        "elim null": dict(elim=elim[:0], n_elim=len(elim), tm=tm[:0], tr=tr[:0]),
        "tied null": dict(tm=tm[:0], n_tied=len(tm)),
        "n_free range": dict(n_free=n_pot + 1),
        "n_free lists": dict(n_free=red.n_free - 1),
        "unsorted elim": dict(elim=elim[::-1].copy()),
        "elim outside": dict(elim=np.append(elim[:-1], n_pot)),
        "unsorted members": dict(tm=tm[::-1].copy(), tr=tr[::-1].copy()) if len(tm) > 1 else dict(tm=np.append(tm, tm), tr=np.append(tr, tr)),
        "member is its representative": dict(tr=tm.copy()),
        "member not eliminated": dict(tm=free[-1:].copy(), tr=free[:1].copy()),
        "representative eliminated": dict(tr=np.full(len(tm), others[0])),
    }
    for what, kw in bad.items():
        assert create(**kw) == _hip.E_INVALID, what
    assert create() == _hip.OK
    plan, ref, imap, src = list_plan(ctx, S, red)
    R = S.block(2, seed=1)
    red, kidx, kval, extras, probes = S.lists(R)
    run(ctx, plan, S, ref, imap, src, R, kidx, kval, extras, probes, red=red, A=check_matrix(plan, ref))
    plan.close()
    wide.close()


def test_stage_entries_refuse_malformed_arguments_and_the_plan_goes_on(ctx):
    S = golden("regulator")
    R = S.block(3, seed=2, own_r=True)
    red, kidx, kval, extras, probes = S.lists(R)
    assert extras and len(kidx) and len(probes)
    plan, ref, imap, src = list_plan(ctx, S, red)
    A = check_matrix(plan, ref)
    N, n_pot = S.N, S.n_pot
    good = (R, kidx, kval, extras, probes)
    i64 = lambda *x: np.array(x, dtype=np.int64)                                   # noqa: E731
    eptr, erow, _ = extras_arrays(extras)
    other = _hip.Context(0)
    first = np.nonzero(R)
    dup_row = np.array([first[0][0], first[0][0]], dtype=np.int64)
    dup_col = np.array([first[1][0], first[1][0]], dtype=np.int32)
    bad1 = [
        ("null opts", "block", dict(opts=None)),
        ("another context", "block", dict(ctx=other._h)),
        ("coo null", "coo", dict(row=None)),
        ("no columns", "block", dict(n_cols=0)),
        ("too many right-hand sides", "block", dict(n_cols=4096)),
        ("negative entries", "coo", dict(n_entries=-1)),
        ("coo out of range", "coo", dict(n_entries=1, row=i64(N), col=np.zeros(1, np.int32), val=np.ones(1))),
        ("coo column out of range", "coo", dict(n_entries=1, row=i64(0), col=np.full(1, 3, np.int32), val=np.ones(1))),
        ("duplicate pair", "coo", dict(n_entries=2, row=dup_row, col=dup_col, val=np.ones(2))),
        ("known null", "block", dict(kidx=None)),
        ("known negative", "block", dict(n_known=-1)),
        ("extra_ptr[0]", "block", dict(eptr=i64(*(eptr + 1)))),
        ("probes null", "block", dict(pout=None)),
        ("probes negative", "block", dict(n_probe=-1)),
        ("known index", "block", dict(kidx=i64(*kidx[:-1], n_pot))),
        ("probe index", "block", dict(pidx=i64(*probes[:-1], N))),
        ("extra_ptr order", "block", dict(eptr=i64(*eptr[:-1], -1))),
        ("extra entries null", "block", dict(erow=None)),
        ("extra row", "block", dict(erow=i64(*erow[:-1], N))),
        ("r null, block", "block", dict(r=None)),
    ]
    for what, entry, kw in bad1:
        rc, _ = stage1(ctx, plan, entry, *good, override=kw)
        assert rc == _hip.E_INVALID, what
        run(ctx, plan, S, ref, imap, src, *good, red=red, A=A)
    R1 = R[:, :1].copy()
    red1, kidx1, kval1, extras1, probes1 = S.lists(R1)
    rc, _ = stage1(ctx, plan, "single", R1, kidx1, kval1, extras1, probes1, override=dict(r=None))
    assert rc == _hip.E_INVALID
    run(ctx, plan, S, ref, imap, src, R1, kidx1, kval1, extras1, probes1, red=red1, A=A, entry="single")
    other.close()
    # stage 2
    n_cols, n_extra = 3, len(extras)
    coeff, midx, mval = np.zeros((n_cols, n_extra)), i64(N - 1), np.zeros((n_cols, 1))
    rc, _, _ = stage2(ctx, plan, "block", N, n_cols, coeff, midx, mval)
    assert rc == _hip.E_INVALID, "finish without a solve (the last block is finished)"
    fresh = _hip.KktPlan(S.dev(ctx), n_pot, red.elim, red.tied, red.n_free)
    rc, _, _ = stage2(ctx, fresh, "block", N, n_cols, coeff, midx, mval)
    assert rc == _hip.E_INVALID, "finish on a plan that never solved"
    fresh.close()
    beyond = i64(N)
    bad2 = [
        ("null v_host", dict(v=None)),
        ("null norms", dict(norms=None)),
        ("other n_cols", dict(n_cols=2)),
        ("other n_extra", dict(n_extra=n_extra + 1)),
        ("coefficients null", dict(coeff=None)),
        ("multipliers negative", dict(n_mult=-1)),
        ("multipliers null", dict(mval=None)),
        ("multiplier index", dict(midx=beyond.ctypes.data_as(_PI64))),
    ]
    for what, kw in bad2:
        rc, _ = stage1(ctx, plan, "block", *good)
        assert rc == _hip.OK
        rc, _, _ = stage2(ctx, plan, "block", N, n_cols, coeff, midx, mval, override=kw)
        assert rc == _hip.E_INVALID, what
        run(ctx, plan, S, ref, imap, src, *good, red=red, A=A)
    plan.close()


def test_accessor_refuses_what_does_not_exist(ctx):
    S = golden("voltage_source")
    red = S.lists(S.block(1, 0))[0]
    plan, ref, imap, src = list_plan(ctx, S, red)
    for which, n in (("B", ref.n_free), ("Y", ref.n_free), ("V", S.N), ("C", S.N), ("Z", 0)):
        with pytest.raises(ValueError):
            plan.state(which, n)
    assert ctx._lib.padne_test_kkt_state(plan._h, 7, None, 0) == _hip.E_INVALID
    assert ctx._lib.padne_test_kkt_state(None, 0, None, 0) == _hip.E_INVALID
    plan.close()

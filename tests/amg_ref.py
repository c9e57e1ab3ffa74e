"""The multigrid hierarchy and V-cycle of csrc/amg.hip as its header comment SPECIFIES them, evaluated in np.longdouble.

Nothing here restates how the device gets there: no priority hashes, no independent-set rounds, no launch order, no
aggregate numbering, no order of summation.  The functions say what a conforming hierarchy IS -- which entries are strong,
what a valid set of roots looks like, which aggregate a vertex must have joined given the roots, what P, P^T A P and the
cycle are as real numbers -- together with entrywise rounding envelopes derived from the standard bounds for sums and
products in double precision (gamma_k = k u / (1 - k u), u = 2^-53; Higham, Accuracy and Stability of Numerical
Algorithms, ch. 3).  A renumbering of the aggregates, another tie-break between competing roots or another order of
summation leaves every check green; a wrong neighbour, two adjacent roots, another omega or a dropped entry does not
(tests/test_amg_ref_host.py shows both on the host).

    strength    j strong for i  <=>  a_ij^2 >= theta^2 a_ii a_jj,  theta = 0.08
    filtered    d^F_i = a_ii + sum of the weak a_ij;  a row with d^F_i / a_ii <= 0.05 keeps all its entries, d^F_i = a_ii
    bounds      lambda = max_i sum_j |a_ij| / a_ii,   lambda_F = max_i (sum_kept |a_ij| + |d^F_i|) / |d^F_i|
    roots       no two within two strong hops; every vertex with a strong neighbour within two strong hops of one
    joins       two passes: a vertex without an aggregate joins that of its strongest aggregated strong neighbour
                (largest |a_ij|, ties to the smaller column); what is left, vertices without strong neighbours, is alone
    prolong     P = (I - omega D_F^-1 A_F) T,  omega = 1.5 / min(lambda_F, lambda)
    coarse      A_c = P^T A P
    cycle       x1 = c D^-1 b, r1 = b - A x1, e = cycle below on P^T r1 (coarsest: A^-1), x2 = x1 + P e,
                z = x2 + c D^-1 (b - A x2),  c = 1 / (0.55 lambda_l)
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53                  # unit roundoff of double precision
THETA = 0.08
KEEP_ALL = 0.05
OMEGA_NUM = 1.5
CHEB = 0.55                     # c = 1 / (0.5 (lambda + lambda / 10))
UNDECIDED = 1e-12               # relative distance to a threshold below which the specification does not decide


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * LD(U) / (1 - k * LD(U))


def csr(A):
    A = sp.csr_matrix(A)
    A.sort_indices()
    return A


def rows_of(A):
    return np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))


def row_sum(A, v, dtype=LD):
    """sum of the per-entry values v over every row of the pattern of A (empty rows: 0)."""
    out = np.zeros(A.shape[0], dtype)
    nz = np.diff(A.indptr) > 0
    if nz.any():
        out[nz] = np.add.reduceat(np.asarray(v, dtype), A.indptr[:-1][nz])
    return out


# ---- strength, filtering, bounds ----------------------------------------------------------------------------------

class Strength:
    """Per entry of the CSR pattern of A: strong (off-diagonal and over the threshold), dist (a_ij^2 / (theta^2 a_ii a_jj) - 1,
    nan on the diagonal), undecided (|dist| <= UNDECIDED: the device may round either way)."""

    def __init__(self, A):
        A = csr(A)
        self.A, self.n = A, A.shape[0]
        self.row, self.col, self.val = rows_of(A), A.indices, A.data.astype(LD)
        self.diag = A.diagonal().astype(LD)
        assert (self.diag > 0).all(), "a positive diagonal"
        self.off = self.row != self.col
        q = self.val * self.val / (LD(THETA) ** 2 * self.diag[self.row] * self.diag[self.col])
        self.dist = np.where(self.off, q - 1, np.nan)
        self.strong = self.off & (q >= 1)
        self.undecided = self.off & (np.abs(q - 1) <= UNDECIDED)
        self.undecided_rows = np.zeros(self.n, bool)
        self.undecided_rows[self.row[self.undecided]] = True

    def graph(self, which="spec"):
        """Boolean CSR strength graph.  "spec": as the longdouble evaluation decides; "sure": without the undecided entries;
        "may": with all of them -- whatever graph the device built lies between the last two."""
        m = {"spec": self.strong, "sure": self.strong & ~self.undecided, "may": self.strong | self.undecided}[which]
        return sp.csr_matrix((np.ones(int(m.sum()), np.int32), (self.row[m], self.col[m])), shape=(self.n, self.n))

    def undecided_share(self):
        return float(self.undecided.sum()) / max(1, int(self.off.sum()))


def strength(A):
    return Strength(A)


def filtered(S):
    """(dF, keep, kappa, keep_all, unsure): the lumped diagonal of every row (a_ii on keep-all rows), which off-diagonal entries
    A_F keeps, the cancellation factor sum |terms| / |d^F_i| of the lumped diagonal, the keep-all rows, and the rows whose
    keep-all decision lies within the rounding of d^F_i of its threshold."""
    A = S.A
    weak = S.off & ~S.strong
    lump = S.diag + row_sum(A, np.where(weak, S.val, 0))
    lump_abs = S.diag + row_sum(A, np.where(weak, np.abs(S.val), 0))
    ratio = lump / S.diag
    keep_all = ~(ratio > KEEP_ALL)
    m = np.diff(A.indptr)
    unsure = np.abs(ratio - KEEP_ALL) <= gamma(m + 2) * lump_abs / S.diag + UNDECIDED
    dF = np.where(keep_all, S.diag, lump)
    kappa = np.where(keep_all, LD(1), lump_abs / np.abs(lump))
    keep = S.off & (S.strong | keep_all[S.row])
    return dF, keep, kappa, keep_all, unsure


def bounds(S):
    """(lambda_plain, lambda_F) as the specification defines them."""
    A = S.A
    lam_plain = (row_sum(A, np.abs(S.val)) / S.diag).max()
    dF, keep, _, _, _ = filtered(S)
    lam_f = ((row_sum(A, np.where(keep, np.abs(S.val), 0)) + np.abs(dF)) / np.abs(dF)).max()
    return lam_plain, lam_f


# ---- aggregation ---------------------------------------------------------------------------------------------------

def join_pass(S, graph_mask, agg_in):
    """One join pass: every vertex with agg_in < 0 takes the aggregate of its strongest aggregated strong neighbour (largest
    |a_ij|, ties to the smaller column); the others keep theirs."""
    m = graph_mask & (agg_in[S.row] < 0) & (agg_in[S.col] >= 0)
    out = agg_in.copy()
    if m.any():
        r, c, w = S.row[m], S.col[m], np.abs(S.A.data[m])
        order = np.lexsort((c, -w, r))                      # by row, then the larger weight, then the smaller column
        r, c = r[order], c[order]
        first = np.concatenate([[True], r[1:] != r[:-1]])
        out[r[first]] = agg_in[c[first]]
    return out


def joined(S, root, which="spec"):
    """The aggregate of every vertex, labelled by the index of its root (or by its own index where the two passes leave it
    alone), that the specification determines from the roots."""
    mask = {"spec": S.strong, "sure": S.strong & ~S.undecided, "may": S.strong | S.undecided}[which]
    agg = np.where(root, np.arange(S.n), -1)
    agg = join_pass(S, mask, join_pass(S, mask, agg))
    return np.where(agg < 0, np.arange(S.n), agg)


def check_aggregation(S, agg, root):
    """Asserts that (agg, root) is an aggregation the specification allows; returns the number of vertices whose membership
    was not compared because an undecided strength entry bears on it."""
    n = S.n
    agg = np.asarray(agg).astype(np.int64)
    root = np.asarray(root).astype(bool)
    assert agg.shape == (n,) and root.shape == (n,)
    assert agg.min() >= 0, "a vertex without an aggregate"
    n_agg = int(agg.max()) + 1
    size = np.bincount(agg, minlength=n_agg)
    assert (size > 0).all(), f"{int((size == 0).sum())} empty aggregates: not a partition onto 0..n_agg-1"
    sure, may = S.graph("sure"), S.graph("may")
    # roots: more than two strong hops apart (in the graph every conforming device graph contains) ...
    ridx = np.flatnonzero(root)
    two = (sure @ sure + sure).tocsr()
    near = two[ridx][:, ridx].tocoo()
    clash = near.row != near.col
    assert not clash.any(), f"roots {ridx[near.row[clash]][:4]} and {ridx[near.col[clash]][:4]} are within two strong hops"
    # ... and maximal: every vertex within two strong hops of one, or without a strong neighbour
    two_may = (may @ may + may).tocsr()
    reached = (two_may @ root.astype(np.int32)) > 0
    lonely_sure = np.diff(sure.indptr) == 0                   # no neighbour that is certainly strong
    lonely_may = np.diff(may.indptr) == 0
    bad = ~(reached | root | lonely_sure)
    assert not bad.any(), f"vertices {np.flatnonzero(bad)[:6]} are more than two strong hops from every root"
    # one root per aggregate, or the singleton of a vertex without strong neighbours; singletons only for such vertices
    n_roots = np.bincount(agg[root], minlength=n_agg)
    assert (n_roots <= 1).all(), f"aggregates {np.flatnonzero(n_roots > 1)[:6]} hold more than one root"
    single = size[agg] == 1
    assert lonely_sure[single].all(), f"vertices {np.flatnonzero(single & ~lonely_sure)[:6]} have strong neighbours and are alone"
    rootless = n_roots[agg] == 0
    assert single[rootless].all(), f"vertices {np.flatnonzero(rootless & ~single)[:6]} lie in an aggregate without a root"
    assert single[lonely_may].all(), f"vertices {np.flatnonzero(lonely_may & ~single)[:6]} have no strong neighbour and are not alone"
    # membership: determined by the two join passes, compared exactly up to renumbering.  Not compared: rows an undecided
    # entry bears on (the row itself and, since the second pass reads the first's result, its possible neighbours).
    ref = joined(S, root)
    skip = S.undecided_rows.copy()
    if skip.any():
        skip |= (may @ skip.astype(np.int32)) > 0
    keep = ~skip
    pairs = np.unique(np.stack([agg[keep], ref[keep]]), axis=1)
    assert len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1])), _membership_report(agg, ref, keep)
    return int(skip.sum())


def _membership_report(agg, ref, keep):
    idx = np.flatnonzero(keep)
    order = np.lexsort((ref[idx], agg[idx]))
    a, r, i = agg[idx][order], ref[idx][order], idx[order]
    split = np.flatnonzero((a[1:] == a[:-1]) & (r[1:] != r[:-1]))
    if len(split):
        return f"vertices {i[split][:4]} and {i[split + 1][:4]} share a device aggregate but join different roots by the rule"
    return "two aggregates of the rule are one aggregate on the device"


def greedy_roots(S):
    """A conforming set of roots, for the host tests: greedy distance-2 independent set in index order (vertices without strong
    neighbours are their own roots).  One of many valid sets -- the device's is another."""
    G = S.graph("spec")
    two = (G @ G + G).tocsr()
    blocked = np.zeros(S.n, bool)
    root = np.zeros(S.n, bool)
    for i in range(S.n):
        if not blocked[i]:
            root[i] = True
            blocked[two.indices[two.indptr[i]:two.indptr[i + 1]]] = True
            blocked[i] = True
    return root


def renumbered(labels):
    """Labels -> 0..n_agg-1 in order of first appearance."""
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.argsort(np.argsort(first))
    return rank[inv].astype(np.int64)


# ---- sparse products in longdouble ---------------------------------------------------------------------------------

class Triplets:
    """A sparse matrix as sorted unique (row, col) pairs with longdouble values, the sum of the absolute values of the terms that
    went into every entry, and their number."""

    def __init__(self, shape, row, col, val, absval, count):
        self.shape, self.row, self.col, self.val, self.abs, self.count = shape, row, col, val, absval, count

    @classmethod
    def summed(cls, shape, row, col, val, absval=None, count=None):
        absval = np.abs(val) if absval is None else absval
        count = np.ones(len(val), np.int64) if count is None else count
        key = row.astype(np.int64) * shape[1] + col
        order = np.argsort(key, kind="stable")
        key = key[order]
        start = np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]])) if len(key) else np.zeros(0, np.int64)
        red = (lambda v: np.add.reduceat(v[order], start)) if len(key) else (lambda v: v[:0])
        k = key[start]
        return cls(shape, k // shape[1], k % shape[1], red(np.asarray(val, LD)), red(np.asarray(absval, LD)), red(count))

    @classmethod
    def of(cls, A):
        A = csr(A)
        return cls(A.shape, rows_of(A).astype(np.int64), A.indices.astype(np.int64), A.data.astype(LD),
                   np.abs(A.data.astype(LD)), np.ones(A.nnz, np.int64))

    def key(self):
        return self.row * self.shape[1] + self.col

    def indptr(self):
        return np.concatenate([[0], np.cumsum(np.bincount(self.row, minlength=self.shape[0]))])

    def transposed(self):
        return Triplets.summed((self.shape[1], self.shape[0]), self.col, self.row, self.val, self.abs, self.count)

    def matmul(self, Y):
        """self @ Y: every product formed once, summed per entry in longdouble (value, |.| sum, number of products)."""
        yp = Y.indptr()
        ln = (yp[1:] - yp[:-1])[self.col]
        rep = np.repeat(np.arange(len(self.row)), ln)
        pos = np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln) + np.repeat(yp[:-1][self.col], ln)
        return Triplets.summed((self.shape[0], Y.shape[1]), self.row[rep], Y.col[pos], self.val[rep] * Y.val[pos],
                               self.abs[rep] * Y.abs[pos], self.count[rep] * Y.count[pos])

    def to_scipy(self):
        return sp.csr_matrix((self.val.astype(np.float64), (self.row, self.col)), shape=self.shape)


def lookup(T, M):
    """Position in the triplets T of every entry of the CSR matrix M (-1: T has no such entry)."""
    M = csr(M)
    key = rows_of(M).astype(np.int64) * M.shape[1] + M.indices
    tk = T.key()
    pos = np.searchsorted(tk, key)
    pos[pos >= len(tk)] = 0
    return np.where(tk[pos] == key, pos, -1) if len(tk) else np.full(len(key), -1), key


def check_entries(T, env, M, what, skip_rows=None, zero_may_be_absent=False):
    """Asserts that the device matrix M has the pattern of the reference T (zero_may_be_absent: entries whose reference value
    is exactly zero may be missing) and that every value lies within the envelope.  Returns the largest error / envelope."""
    M = csr(M)
    assert M.shape == T.shape, f"{what}: shape {M.shape}, reference {T.shape}"
    pos, _ = lookup(T, M)
    rows = rows_of(M)
    on = np.ones(M.nnz, bool) if skip_rows is None else ~skip_rows[rows]
    ton = np.ones(len(T.row), bool) if skip_rows is None else ~skip_rows[T.row]
    extra = on & (pos < 0)
    assert not extra.any(), f"{what}: {int(extra.sum())} entries the reference has not, first at {rows[extra][:3], M.indices[extra][:3]}"
    seen = np.zeros(len(T.row), bool)
    seen[pos[pos >= 0]] = True
    missing = ton & ~seen & ((T.val != 0) if zero_may_be_absent else True)
    assert not missing.any(), f"{what}: {int(missing.sum())} entries of the reference are missing, first at {T.row[missing][:3], T.col[missing][:3]}"
    p = pos[on]
    err = np.abs(M.data[on].astype(LD) - T.val[p])
    over = err > env[p]
    assert not over.any(), (f"{what}: {int(over.sum())} values outside the envelope, worst {float((err[over] / env[p][over]).max()):.3g} x "
                            f"at {rows[on][over][:3], M.indices[on][over][:3]}")
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(env[p] > 0, err / env[p], 0)
    return float(ratio.max()) if len(ratio) else 0.0


# ---- prolongator and coarse operator -------------------------------------------------------------------------------

def prolongator(S, agg, n_agg=None, *, omega_scale=1, unlumped=None):
    """(P, envelope, omega, skip_rows).  P = (I - omega D_F^-1 A_F) T as Triplets in longdouble.

    The envelope, entry by entry: every term of an entry is 1, omega, or omega a_ij / d^F_i.  omega = 1.5 / lambda carries the
    rounding of the longest row's sum of m_max absolute values, a division by the diagonal, a maximum and the division
    (gamma_{m_max + 3}); d^F_i is a sum of at most m_i terms whose rounding, gamma_{m_i}, is amplified by the cancellation
    factor kappa_i = sum |terms| / |d^F_i| >= 1; a product, a quotient and the sum of at most m_i + 1 terms of the entry add
    gamma_{m_i + 3}.  Together: gamma_{m_max + 2 m_i + 6} kappa_i times the sum of the absolute values of the entry's terms.

    skip_rows: rows with an undecided strength entry or an undecided keep-all decision (the specification does not fix them).
    omega_scale, unlumped: mutations for the host tests (omega scaled; one weak entry, by CSR position, left in A_F instead of
    being lumped into the diagonal)."""
    A, n = S.A, S.n
    agg = np.asarray(agg).astype(np.int64)
    n_agg = int(agg.max()) + 1 if n_agg is None else int(n_agg)
    dF, keep, kappa, _, unsure = filtered(S)
    if unlumped is not None:
        i = S.row[unlumped]
        assert S.off[unlumped] and not keep[unlumped]
        dF = dF.copy()
        dF[i] -= S.val[unlumped]                              # the entry stays where it is instead of going to the diagonal
        keep = keep.copy()
        keep[unlumped] = True
    lam_plain, lam_f = bounds(S)
    omega = LD(OMEGA_NUM) / min(lam_plain, lam_f) * LD(omega_scale)
    ar = np.arange(n)
    row = np.concatenate([ar, ar, S.row[keep]])
    col = np.concatenate([agg, agg, agg[S.col[keep]]])
    val = np.concatenate([np.ones(n, LD), np.full(n, -omega), -omega * S.val[keep] / dF[S.row[keep]]])
    P = Triplets.summed((n, n_agg), row, col, val)
    m = np.diff(A.indptr)
    env = gamma(int(m.max()) + 2 * m[P.row] + 6) * kappa[P.row] * P.abs
    return P, env, omega, S.undecided_rows | unsure


def galerkin(A, P):
    """(A_c, envelope): P^T A P as Triplets in longdouble -- its rows are the symbolic pattern of the product, entries that
    cancel included -- and the entrywise envelope gamma_k |P^T| |A| |P| with k = the products of the entry (counted through
    both stages) + 2: any order of summation of any association of the triple product stays within it."""
    At, Pt = Triplets.of(A), (P if isinstance(P, Triplets) else Triplets.of(P))
    Ac = Pt.transposed().matmul(At.matmul(Pt))
    return Ac, gamma(Ac.count + 2) * Ac.abs


# ---- the cycle -----------------------------------------------------------------------------------------------------

def _product(M, dtype):
    """x -> M x in `dtype` ((n,) or (n, k)); rows summed by np.add.reduceat, no float64 anywhere."""
    M = csr(M)
    data, idx = M.data.astype(dtype), M.indices
    nz = np.diff(M.indptr) > 0
    ptr = M.indptr[:-1][nz]

    def apply(x):
        out = np.zeros((M.shape[0],) + x.shape[1:], dtype)
        if len(ptr):
            out[nz] = np.add.reduceat((data if x.ndim == 1 else data[:, None]) * x[idx], ptr, axis=0)
        return out
    return apply


class Cycle:
    """The V(1,1) cycle of the header comment on given operators.

    levels: [(A_l, P_l, lambda_l)] for every level but the coarsest; coarse: b -> A_c^-1 b (longdouble, dense_ref's refined
    solver) or a dense inverse.  dtype=np.longdouble is the reference; dtype=np.float32 is a plain single-precision
    evaluation of the same formula (operators, vectors and the coarse inverse rounded to float), the yardstick for the
    rounding of the device's single-precision cycle.  post: "full" (the specification); "skip" and "stale" are the two wrong
    cycles the host tests must tell apart (no post-sweep; post-sweep against r1 instead of b - A x2)."""

    def __init__(self, levels, coarse, dtype=LD, post="full"):
        self.dtype, self.post = dtype, post
        self.lv = []
        for A, P, lam in levels:
            A, P = csr(A), csr(P)
            c = dtype(1) / (dtype(CHEB) * dtype(lam))
            self.lv.append((_product(A, dtype), _product(P, dtype), _product(P.T, dtype),
                            c / A.diagonal().astype(dtype)))
        if callable(coarse):
            self.coarse = coarse
        else:
            # (a dense inverse: rows summed entry after entry in `dtype` -- no BLAS, whose order of summation differs between
            # machines; the float32 yardstick must be the same number everywhere)
            inv_t = np.ascontiguousarray(np.asarray(coarse).astype(dtype).T)
            self.coarse = lambda b: np.stack([np.add.reduce(inv_t * b[:, j][:, None], axis=0) for j in range(b.shape[1])], axis=1)

    def __call__(self, b, level=0):
        b = np.asarray(b).astype(self.dtype)
        if level == len(self.lv):
            flat = b.ndim == 1
            e = self.coarse(b[:, None] if flat else b)
            e = np.asarray(e).astype(self.dtype)
            return e[:, 0] if flat else e
        A, P, R, cd = self.lv[level]
        cd = cd if b.ndim == 1 else cd[:, None]
        x1 = cd * b
        r1 = b - A(x1)
        x2 = x1 + P(self(R(r1), level + 1))
        if self.post == "skip":
            return x2
        return x2 + cd * (r1 if self.post == "stale" else b - A(x2))


def cycle(levels, inv_coarse, r, dtype=LD, post="full"):
    return Cycle(levels, inv_coarse, dtype, post)(r)


def cycle_envelope(levels, coarse, coarse_A, b, abs_inv=None, coarse_delta=None):
    """(z, env) for b of shape (n,) or (n, k): the longdouble cycle and an entrywise bound of the forward error of ANY double-precision evaluation of it.

    Propagated stage by stage: a product y = M x of rows of at most m entries on an input known to err_x errs by
    |M| err_x + gamma_{m+1} |M| |x|; a sum or a scaling adds u times its result (scalings by c D^-1, two roundings for c itself:
    gamma_4).  The coarsest level multiplies by an inverse formed by Gauss-Jordan elimination without pivoting, whose
    forward error is bounded to first order by 8 n u |A^-1| |L| |U| |A^-1| (Higham, Accuracy and Stability, Thm 14.5), with
    |L| |U| replaced by |A| as for a diagonally dominant matrix; the product itself adds gamma_n |A^-1| |b|.  abs_inv: an upper
    bound of |A^-1| (by default formed from the caller's solver applied to the identity).  coarse_delta: |A_dev - A| where
    the device inverts a matrix A_dev that differs from the one `coarse` solves with (a device operator that is symmetric
    only to rounding, against its exactly symmetric part): to first order the solution moves by |A^-1| delta |A^-1| |b|."""
    ops = []
    for A, P, lam in levels:
        A, P = csr(A), csr(P)
        c = LD(1) / (LD(CHEB) * LD(lam))
        absA, absP = abs(A), abs(P)
        ops.append(dict(A=_product(A, LD), P=_product(P, LD), R=_product(P.T, LD), aA=_product(absA, LD), aP=_product(absP, LD),
                        aR=_product(absP.T, LD), cd=c / A.diagonal().astype(LD), mA=int(np.diff(A.indptr).max()),
                        mP=int(np.diff(P.indptr).max()), mR=int(np.diff(csr(P.T).indptr).max())))
    Ac = csr(coarse_A)
    aAc = _product(abs(Ac), LD)
    nc = Ac.shape[0]
    u = LD(U)

    def rec(b, eb, l):
        o = ops[l]
        cd = o["cd"] if b.ndim == 1 else o["cd"][:, None]
        x1 = cd * b
        ex1 = np.abs(cd) * eb + gamma(4) * np.abs(x1)
        r1 = b - o["A"](x1)
        er1 = eb + o["aA"](ex1) + gamma(o["mA"] + 1) * o["aA"](np.abs(x1)) + u * np.abs(r1)
        bc = o["R"](r1)
        ebc = o["aR"](er1) + gamma(o["mR"] + 1) * o["aR"](np.abs(r1))
        e, ee = solve(bc, ebc, l + 1)
        x2 = x1 + o["P"](e)
        ex2 = ex1 + o["aP"](ee) + gamma(o["mP"] + 1) * o["aP"](np.abs(e)) + u * np.abs(x2)
        r2 = b - o["A"](x2)
        er2 = eb + o["aA"](ex2) + gamma(o["mA"] + 1) * o["aA"](np.abs(x2)) + u * np.abs(r2)
        z = x2 + cd * r2
        ez = ex2 + np.abs(cd) * er2 + gamma(4) * np.abs(cd * r2) + u * np.abs(z)
        return z, ez

    inv_abs = {}

    def solve(b, eb, l):
        if l < len(ops):
            return rec(b, eb, l)
        if "M" not in inv_abs:
            inv_abs["M"] = (np.abs(np.asarray(coarse(np.eye(nc, dtype=LD)), dtype=LD)) if abs_inv is None
                            else np.asarray(abs_inv, dtype=LD))
        M = inv_abs["M"]
        e = coarse(b[:, None])[:, 0] if b.ndim == 1 else coarse(b)
        ab = M @ np.abs(b)
        ee = M @ eb + gamma(nc) * ab + 8 * nc * u * (M @ aAc(ab))
        if coarse_delta is not None and coarse_delta.nnz:
            ee = ee + M @ _product(csr(coarse_delta), LD)(ab)
        return e, ee

    b = np.asarray(b).astype(LD)
    return rec(b, np.zeros_like(b), 0) if ops else solve(b, np.zeros_like(b), 0)


def explicit_cycle_matrix(A, P, lam, Ac_inv):
    """The two-level cycle as a dense matrix (longdouble): 2cD^-1 - c^2 D^-1 A D^-1 + (I - cD^-1 A) P A_c^-1 P^T (I - cAD^-1)."""
    Ad, Pd = np.asarray(csr(A).toarray(), LD), np.asarray(csr(P).toarray(), LD)
    n = Ad.shape[0]
    c = LD(1) / (LD(CHEB) * LD(lam))
    Di = np.diag(1 / np.diag(Ad))
    I = np.eye(n, dtype=LD)
    return 2 * c * Di - c * c * Di @ Ad @ Di + (I - c * Di @ Ad) @ Pd @ Ac_inv @ Pd.T @ (I - c * Ad @ Di)


def check_smoothing(lam_dev, jac_dev, lam_plain, m_max, level, lam_max=None):
    """lambda_0 is the plain bound to (m + 2) u; below, lambda_l is at most that bound and -- stability -- 1.1 lambda_l exceeds
    the largest eigenvalue of D^-1 A (so that jac lambda_max = lambda_max / (0.55 lambda_l) < 2); jac = 1 / (0.55 lambda_l)
    to 2 ulp.  Returns the stability ratio 1.1 lambda_l / lambda_max (None on level 0 without lam_max)."""
    tol = (m_max + 2) * U
    lam_plain = float(lam_plain)
    if level == 0:
        assert abs(lam_dev - lam_plain) <= tol * lam_plain, f"lambda_0 = {lam_dev!r}, the bound is {lam_plain!r}"
    else:
        assert lam_dev <= lam_plain * (1 + tol), f"lambda_{level} = {lam_dev!r} exceeds the plain bound {lam_plain!r}"
    want = float(LD(1) / (LD(CHEB) * LD(lam_dev)))
    assert abs(jac_dev - want) <= 2 * np.spacing(want), f"jac_{level} = {jac_dev!r}, 1 / (0.55 lambda) = {want!r}"
    if lam_max is None:
        return None
    ratio = 1.1 * lam_dev / lam_max
    assert ratio > 1, f"level {level}: jac lambda_max = {2 / ratio:.4f} >= 2, the sweep is not a contraction"
    return ratio


# ---- test systems ----------------------------------------------------------------------------------------------------

def layered_matrix(n_layers, nx, ny, lattice, extra=()):
    """The SPD operator of synthetic.layered_system (vertex 0 grounded and removed), as the oracle assembles it; `extra`:
    further ("R", a, b, ohms) elements."""
    from oracle import padne_oracle as O
    from padne_amd import synthetic
    s = synthetic.layered_system(n_layers, nx, ny, via_lattice=lattice)
    els = [("R", int(a), int(b), float(r)) for a, b, r in zip(*s.resistors)]
    els += [("I", int(f), int(t), float(i)) for f, t, i in zip(*s.current_sources)]
    els += list(extra)
    Lo, _ = O.assemble_system([(m[0], m[1], m[2]) for m in s.meshes], 0, els, 0)
    n = s.n_vertices
    return csr(-Lo[1:n, 1:n])


def obtuse_matrix(nx, ny, jitter=0.3, seed=3):
    """Stiffness matrix of a jittered grid with SIGNED cotangent weights, vertex 0 removed: symmetric positive
    definite, and an edge whose two opposite angles sum to more than 180 degrees has a POSITIVE off-diagonal entry."""
    from padne_amd import synthetic
    xy, tri = synthetic.jittered_grid(nx, ny, 1.0, seed=seed, jitter=jitter)
    n = len(xy)
    rows, cols, vals = [], [], []
    for k in range(3):
        o, i, j = tri[:, k], tri[:, (k + 1) % 3], tri[:, (k + 2) % 3]
        a, b = xy[i] - xy[o], xy[j] - xy[o]
        w = 0.5 * (a * b).sum(1) / (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])
        rows += [i, j, i, j]
        cols += [j, i, i, j]
        vals += [-w, -w, w, w]
    L = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    return csr(L[1:, 1:])

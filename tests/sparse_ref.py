"""Host references of the sparse primitives under the assembly and the multigrid setup -- the exclusive scan, the slot merge
behind reduce / relabel, the transpose and the sparse product -- in numpy, int64 and np.longdouble, and the builders of the
inputs that tests/test_sparse_primitives_vs_reference.py plants at the kernels' own limits.  Checked on the CPU by
tests/test_sparse_ref_host.py against scipy and dense longdouble arithmetic; no device, no library.

  scan        offsets[n + 1] = exclusive np.cumsum in int64, the 64-bit total, whether an input is negative.
  merge       out = scale * R^T M C for index maps that may merge rows and columns and drop them (-1): for output row t and
              column c the kept source entries in ascending position of the source arrays, v = 0.0 + s a_1 + s a_2 + ...
              one after the other in float64 (s a_i rounded first: no fused multiply-add), exact zeros dropped, columns
              ascending.  That is the order the keys (column, position in the source) of reduce_fill and merge_rows fix, so
              the comparison is on bits.
  transpose   a permutation of the value bits, columns ascending: exact.
  product     the symbolic pattern of X Y, and per entry the value in longdouble, the number of products k_ij and
              (|X| |Y|)_ij.  A float64 evaluation in ANY order of the additions, with or without fused multiply-adds, of k
              products rounds each term at most k times (its product, at most k - 1 additions), so it lies within
              gamma(k) (|X||Y|)_ij of the exact value (Higham, Accuracy and Stability, ch. 3), gamma(m) = m u / (1 - m u),
              u = 2^-53; the bound used is gamma(k_ij + 1) (|X||Y|)_ij, the + 1 for the longdouble reference's own rounding
              (k 2^-64, far below one more u).  Derived, not measured.
  chain       X (Y Z) through the symbolic pattern of Y Z: a term of entry (i, j) is x y z; with k_mj products in (Y Z)_mj
              and t terms in the outer sum it is rounded at most k_mj + t <= cnt_ij + 1 times, cnt_ij = the elementary
              products of the entry; the bound is gamma(cnt_ij + 2) (|X||Y||Z|)_ij.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
INT_MAX = 2147483647

# the limits the kernels branch on (assemble.hip, amg.hip), restated for the assertions on the inputs
SCAN_SMALL = 32768            # one workgroup up to here, three kernels beyond
SCAN_CHUNK = 4096             # entries per workgroup of the three kernels
MERGE_LDS = 32                # slots of a merged row the LDS pass takes
MERGE_WAVE = 1024             # slots a wave sorts; the one-lane sort beyond
TP_WAVES = 16                 # waves of 64 rows per column the transpose lists
TP_ENTRIES = 240              # entries of a wave's 64 rows its table takes
TP_SEG = 64                   # entries of a transposed row sort_csr_rows_seg takes, in chunks of TP_CHUNK rows
TP_CHUNK = 8
TP_LIST = 2048                # entries a workgroup sorts; one thread beyond
DENSE_LDS = 150 * 1024        # bytes of the dense accumulator: n_cols * 9 + 16


def gamma(m):
    m = np.asarray(m, LD)
    return m * LD(U) / (LD(1) - m * LD(U))


def canonical(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M


# ---- scan --------------------------------------------------------------------------------------------------------------

def scan(counts):
    """(offsets int64[n + 1], total, negative)."""
    c = np.asarray(counts, np.int64)
    out = np.zeros(len(c) + 1, np.int64)
    np.cumsum(c, out=out[1:])
    return out, int(out[-1]), bool((c < 0).any())


# ---- merge -------------------------------------------------------------------------------------------------------------

def merge_slots(M, row_map, col_map):
    """The kept source entries -- both maps >= 0 -- as (source row, position in the source arrays): the slots."""
    M = canonical(M)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    keep = (np.asarray(row_map)[rows] >= 0) & (np.asarray(col_map)[M.indices] >= 0)
    return rows[keep], np.flatnonzero(keep)


def merge(M, row_map, n_rows_out, col_map, n_cols_out, scale=1.0):
    """scale * R^T M C as (indptr int32, indices int32, data float64) on bits, and per output row the slots and the largest
    number of terms of one of its columns."""
    M = canonical(M)
    row_map, col_map = np.asarray(row_map, np.int64), np.asarray(col_map, np.int64)
    src_rows, pos = merge_slots(M, row_map, col_map)
    t, c = row_map[src_rows], col_map[M.indices[pos]]
    # (the product s * a is rounded to float64 before it is added: two operations, as the kernels are compiled)
    term = np.float64(scale) * M.data[pos].astype(np.float64)
    order = np.lexsort((pos, c, t))
    t, c, term = t[order], c[order], term[order]
    slots = np.bincount(t, minlength=n_rows_out).astype(np.int64)
    if len(t) == 0:
        return np.zeros(n_rows_out + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64), slots, np.zeros(n_rows_out, np.int64)
    first = np.r_[True, (t[1:] != t[:-1]) | (c[1:] != c[:-1])]
    start = np.flatnonzero(first)
    length = np.diff(np.r_[start, len(t)])
    v = np.zeros(len(start), np.float64)
    for j in range(int(length.max())):
        on = length > j
        v[on] = v[on] + term[start[on] + j]
    gt, gc = t[start], c[start]
    terms_max = np.zeros(n_rows_out, np.int64)
    np.maximum.at(terms_max, gt, length)
    nz = v != 0.0
    indptr = np.zeros(n_rows_out + 1, np.int64)
    np.cumsum(np.bincount(gt[nz], minlength=n_rows_out), out=indptr[1:])
    return indptr.astype(np.int32), gc[nz].astype(np.int32), v[nz], slots, terms_max


def compact_rows_per_wave(n_rows, nnz):
    """compact_rows' setting for an output of that shape (assemble.hip: compact_rows_per_wave)."""
    if n_rows <= 0 or n_rows > 100000 or nnz <= 16 * n_rows:
        return 64
    return 8 if nnz <= 128 * n_rows else 1


def merging_case(targets, n_rows_out, n_cols_out, seed, fan=8, dropped_rows=(), zeros=0, cancel_rows=(), scatter=True,
                 square=False):
    """A source matrix with row and column maps whose output row t has exactly the slots `targets` plans.

    targets: {t: [terms of its 1st column, terms of its 2nd column, ...]} -- every output row and column is the image of
    `fan` source rows / columns (scattered over the source by a permutation), a column of c terms takes c distinct (source
    row, source column) pairs of the fan x fan block, so c <= fan * fan.  dropped_rows: rows of `targets` whose source rows
    hold their entries but map to -1: the output row stays empty.  zeros: that many explicit zeros among the source values.
    cancel_rows: rows of `targets` of two terms per column, a and -a: s a + s (-a) is exactly zero for every scale s.
    square: one map for rows and columns (n_rows_out == n_cols_out), as reduce takes it.
    Returns (M, row_map, col_map)."""
    rng = np.random.default_rng(seed)
    n_src_r, n_src_c = n_rows_out * fan, n_cols_out * fan
    rperm = rng.permutation(n_src_r) if scatter else np.arange(n_src_r)
    cperm = rng.permutation(n_src_c) if scatter else np.arange(n_src_c)
    if square:
        assert n_rows_out == n_cols_out
        cperm = rperm
    row_map = np.empty(n_src_r, np.int32)
    col_map = np.empty(n_src_c, np.int32)
    row_map[rperm] = np.arange(n_src_r) // fan
    col_map[cperm] = np.arange(n_src_c) // fan
    # (one map for both: a dropped row is a dropped column as well, which no planned row may count on)
    avail = np.setdiff1d(np.arange(n_cols_out), dropped_rows) if square else np.arange(n_cols_out)
    rr, cc, vv, plain = [], [], [], []
    for t, mult in targets.items():
        mult = list(mult)
        assert max(mult, default=0) <= fan * fan and len(mult) <= len(avail)
        cols_t = rng.choice(avail, len(mult), replace=False)
        for c, m in zip(cols_t, mult):
            cell = rng.choice(fan * fan, m, replace=False)
            rr.append(rperm[t * fan + cell // fan])
            cc.append(cperm[c * fan + cell % fan])
            plain.append(np.full(m, t not in cancel_rows))
            if t in cancel_rows:
                assert m == 2
                a = rng.uniform(0.5, 2.0)
                vv.append(np.array([a, -a]))
            else:
                vv.append(rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m))
    rr, cc, vv = (np.concatenate(x) if x else np.zeros(0) for x in (rr, cc, vv))
    if zeros:
        vv[rng.choice(np.flatnonzero(np.concatenate(plain)), zeros, replace=False)] = 0.0      # (not where terms must cancel)
    M = sp.csr_matrix((vv, (rr.astype(np.int64), cc.astype(np.int64))), shape=(n_src_r, n_src_c))
    M.sort_indices()
    for t in dropped_rows:
        assert t in targets
        row_map[rperm[t * fan:(t + 1) * fan]] = -1
    if square:
        col_map = row_map
    return M, row_map, col_map


def split_terms(slots, rng, lo=2, hi=40):
    """`slots` as a list of column multiplicities in lo .. hi (the last one whatever is left, at least 1)."""
    out = []
    left = slots
    while left > 0:
        m = int(min(left, rng.integers(lo, hi + 1)))
        out.append(m)
        left -= m
    return out


MERGE_LIMIT_SLOTS = [1, 2, 32, 33, 64, 1024, 1025, 1100]


def build_merge_case(name, n_rows_out=128, square=False, seed=31):
    """The inputs of the merge tests, as (M, row_map, col_map, n_rows_out, n_cols_out, plan) with plan = what the case claims:
      "limits"   rows of exactly MERGE_LIMIT_SLOTS slots at output rows 3, 10, 17, ..., a row (24 slots, and one of 40 beyond
                 the LDS pass) whose terms cancel exactly, a dropped row (row 11) between the merged rows 10 and 12, five
                 explicit zeros, small rows elsewhere; n_rows_out as asked (127, 128, 129)
      "mid"      40 rows of about 60 columns with 2 to 3 terms each: more than 16 and at most 128 entries per output row
      "wide"     24 rows of 150 columns with 2 terms each: more than 128 entries per output row"""
    rng = np.random.default_rng(seed)
    if name == "limits":
        n_cols_out = n_rows_out if square else 90
        targets = {t: split_terms(int(rng.integers(3, 20)), rng, 2, 6) for t in range(0, n_rows_out, 2)}
        plan = {"slots": {}, "cancel": [5, 14], "dropped": [11], "empty": [5, 11, 14]}
        for j, sl in enumerate(MERGE_LIMIT_SLOTS):
            targets[3 + 7 * j] = split_terms(sl, rng) if sl > 2 else [sl]
            plan["slots"][3 + 7 * j] = sl
        targets[5] = [2] * 12
        targets[14] = [2] * 20
        targets[11] = split_terms(50, rng)
        M, rm, cm = merging_case(targets, n_rows_out, n_cols_out, seed + 1, dropped_rows=(11,), zeros=5, cancel_rows=(5, 14),
                                 square=square)
        return M, rm, cm, n_rows_out, n_cols_out, plan
    if name == "mid":
        n_rows_out, n_cols_out = (100, 100) if square else (40, 100)
        targets = {t: [int(m) for m in rng.integers(2, 4, 60)] for t in range(n_rows_out)}
        M, rm, cm = merging_case(targets, n_rows_out, n_cols_out, seed + 2, square=square)
        return M, rm, cm, n_rows_out, n_cols_out, {"rpw": 8}
    assert name == "wide"
    n_rows_out, n_cols_out = (200, 200) if square else (24, 200)
    targets = {t: [2] * 150 for t in range(n_rows_out)}
    M, rm, cm = merging_case(targets, n_rows_out, n_cols_out, seed + 3, square=square)
    return M, rm, cm, n_rows_out, n_cols_out, {"rpw": 1}


# ---- transpose -----------------------------------------------------------------------------------------------------------

def transpose(M):
    """M^T as (indptr, indices, data): every value where its (column, row) belongs, the rows' columns ascending."""
    M = canonical(M)
    rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
    order = np.lexsort((rows, M.indices))
    indptr = np.zeros(M.shape[1] + 1, np.int64)
    np.cumsum(np.bincount(M.indices, minlength=M.shape[1]), out=indptr[1:])
    return indptr.astype(np.int32), rows[order].astype(np.int32), M.data[order]


def transpose_stats(M):
    """What the transpose kernels branch on: entries per wave of 64 rows, waves per column (the waves whose table does not
    take their rows count as TP_WAVES + 1 each, as the kernel books them), entries per column."""
    M = canonical(M)
    n, nc = M.shape
    rows = np.repeat(np.arange(n), np.diff(M.indptr))
    wave = rows // 64
    n_waves = (n + 63) // 64
    per_wave = np.bincount(wave, minlength=n_waves)
    pairs = np.unique(np.stack([M.indices.astype(np.int64), wave]), axis=1) if M.nnz else np.zeros((2, 0), np.int64)
    weight = np.where(per_wave[pairs[1]] > TP_ENTRIES, TP_WAVES + 1, 1)
    # (a wave beyond its table books TP_WAVES + 1 per ENTRY; one per (column, wave) is enough to know it is over the limit)
    waves_per_col = np.bincount(pairs[0], weights=weight, minlength=nc).astype(np.int64)
    col_len = np.bincount(M.indices, minlength=nc)
    return {"per_wave": per_wave, "waves_per_col": waves_per_col, "col_len": col_len,
            "sorted_cols": waves_per_col > TP_WAVES}


# ---- product -------------------------------------------------------------------------------------------------------------

class Product:
    """The symbolic product: row, col (sorted by row, then column), val and absval in longdouble, count = elementary products
    per entry, and of the rows: x_len, slots (products per row), distinct."""

    def __init__(self, shape, row, col, val, absval, count, x_len, slots):
        self.shape, self.row, self.col, self.val, self.absval, self.count = shape, row, col, val, absval, count
        self.x_len, self.slots = x_len, slots
        self.distinct = np.bincount(row, minlength=shape[0]).astype(np.int64)

    @property
    def indptr(self):
        p = np.zeros(self.shape[0] + 1, np.int64)
        np.cumsum(self.distinct, out=p[1:])
        return p

    def csr(self, what="val"):
        return sp.csr_matrix((getattr(self, what).astype(np.float64), self.col, self.indptr), shape=self.shape)


def _expand(x_indptr, x_indices, x_val, x_abs, x_cnt, Y_indptr, Y_indices, y_val, y_abs, y_cnt, shape):
    n = len(x_indptr) - 1
    xrow = np.repeat(np.arange(n), np.diff(x_indptr))
    ylen = np.diff(Y_indptr)[x_indices]
    slots = np.bincount(xrow, weights=ylen, minlength=n).astype(np.int64)
    e = np.repeat(np.arange(len(x_indices)), ylen)                     # the X entry of every product
    if len(e):
        first = np.cumsum(ylen) - ylen
        q = Y_indptr[x_indices][e] + (np.arange(len(e)) - first[e])    # its Y entry
    else:
        q = np.zeros(0, np.int64)
    r, c = xrow[e], Y_indices[q].astype(np.int64)
    v, a, k = x_val[e] * y_val[q], x_abs[e] * y_abs[q], x_cnt[e] * y_cnt[q]
    order = np.lexsort((c, r))
    r, c, v, a, k = r[order], c[order], v[order], a[order], k[order]
    if len(r) == 0:
        z = np.zeros(0, np.int64)
        return Product(shape, z, z, np.zeros(0, LD), np.zeros(0, LD), z, np.diff(x_indptr), slots)
    start = np.flatnonzero(np.r_[True, (r[1:] != r[:-1]) | (c[1:] != c[:-1])])
    return Product(shape, r[start], c[start], np.add.reduceat(v, start), np.add.reduceat(a, start),
                   np.add.reduceat(k, start), np.diff(x_indptr), slots)


def product(X, Y):
    """X Y as a Product (X, Y scipy matrices; explicit zeros count as entries)."""
    X, Y = canonical(X), canonical(Y)
    assert X.shape[1] == Y.shape[0]
    one_x, one_y = np.ones(X.nnz, np.int64), np.ones(Y.nnz, np.int64)
    return _expand(X.indptr.astype(np.int64), X.indices, X.data.astype(LD), np.abs(X.data).astype(LD), one_x,
                   Y.indptr.astype(np.int64), Y.indices, Y.data.astype(LD), np.abs(Y.data).astype(LD), one_y,
                   (X.shape[0], Y.shape[1]))


def chain(X, Y, Z):
    """X (Y Z) through the symbolic pattern of Y Z; count = elementary products x y z per entry."""
    X = canonical(X)
    YZ = product(Y, Z)
    assert X.shape[1] == YZ.shape[0]
    return _expand(X.indptr.astype(np.int64), X.indices, X.data.astype(LD), np.abs(X.data).astype(LD), np.ones(X.nnz, np.int64),
                   YZ.indptr, YZ.col, YZ.val, YZ.absval, YZ.count, (X.shape[0], YZ.shape[1])), YZ


def product_bound(P, extra=1):
    return gamma(P.count + extra) * P.absval


def check_product(P, indptr, indices, data, extra=1, drop_cancelled=False):
    """The device's CSR arrays against the Product: the pattern equal (drop_cancelled: without the entries whose terms cancel
    exactly, |X||Y| > 0 and value 0), every value within the bound.  Returns the largest share of its bound an entry used."""
    keep = np.ones(len(P.row), bool)
    if drop_cancelled:
        keep = ~((P.val == 0) & (P.absval > 0))
    ref_ptr = np.zeros(P.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(P.row[keep], minlength=P.shape[0]), out=ref_ptr[1:])
    assert np.array_equal(np.asarray(indptr, np.int64), ref_ptr), "row pointers of the product"
    assert np.array_equal(np.asarray(indices, np.int64), P.col[keep]), "columns of the product"
    err = np.abs(np.asarray(data).astype(LD) - P.val[keep])
    bound = product_bound(P, extra)[keep]
    assert (err <= bound).all(), f"value beyond its bound: worst share {float((err / np.maximum(bound, LD(1e-4000))).max())}"
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def cyclic_rows(columns, lengths):
    """Rows that walk `columns` (distinct) round and round: row r takes the next lengths[r] of them, so every row's columns are
    distinct when lengths[r] <= len(columns) and all of them appear once sum(lengths) >= len(columns)."""
    columns = np.asarray(columns)
    assert max(lengths) <= len(columns)
    out, at = [], 0
    for ln in lengths:
        out.append(columns[(at + np.arange(ln)) % len(columns)])
        at += ln
    return out


def product_case(n, n_mid, n_cols, seed, x_len, y_len, planted=(), signed=False, empty_x=(), empty_y_every=0):
    """X (n x n_mid') and Y (n_mid' x n_cols): background rows of X with x_len() entries selecting background rows of Y of
    y_len() entries, and planted rows (nx, np, nd) -- rows of X of exactly nx entries that select nx rows of Y of their own
    whose np entries cover exactly nd distinct columns (np >= nd >= ceil(np / nx)).  The planted rows replace the background
    rows at scattered places; their rows of Y are appended behind the n_mid background rows.  x_len / y_len: callables
    rng -> int.  empty_x: rows of X left empty; empty_y_every: every that-many-th background row of Y is empty."""
    rng = np.random.default_rng(seed)
    val = (lambda m: rng.uniform(0.5, 2.0, m) * (rng.choice([-1.0, 1.0], m) if signed else 1.0))
    y_rows = []
    for m in range(n_mid):
        ln = 0 if (empty_y_every and m % empty_y_every == empty_y_every - 1) else min(int(y_len(rng)), n_cols)
        y_rows.append(np.sort(rng.choice(n_cols, ln, replace=False)))
    where = {}
    if planted:
        places = (np.arange(len(planted)) * max(n // len(planted), 1) + 5) % n
        assert len(set(places.tolist())) == len(planted) and not set(places.tolist()) & set(empty_x)
        where = dict(zip(places.tolist(), planted))
    x_rows = []
    for i in range(n):
        if i in where:
            nx, npd, nd = where[i]
            assert nd <= npd <= nx * nd and nd <= n_cols and nx >= 1
            lengths = [npd // nx + (1 if r < npd % nx else 0) for r in range(nx)]
            assert max(lengths) <= nd
            cols_i = rng.choice(n_cols, nd, replace=False)
            x_rows.append(len(y_rows) + np.arange(nx))
            y_rows.extend(np.sort(r) for r in cyclic_rows(cols_i, lengths))
        elif i in empty_x:
            x_rows.append(np.zeros(0, np.int64))
        else:
            x_rows.append(np.sort(rng.choice(n_mid, min(int(x_len(rng)), n_mid), replace=False)))

    def build(rows, width):
        indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
        idx = (np.concatenate(rows) if rows and indptr[-1] else np.zeros(0)).astype(np.int32)
        return sp.csr_matrix((val(len(idx)), idx, indptr), shape=(len(rows), width))
    Y = build(y_rows, n_cols)
    X = build(x_rows, len(y_rows))
    return X, Y, where


def product_branch(P, X, n_cols):
    """The row kernel spgemm picks for a product of these shapes (amg.hip: spgemm), and its counting kernel."""
    n = P.shape[0]
    if n == 0:
        return "none", "none"
    x_avg = X.nnz / n
    count = "lanes32" if x_avg > 48.0 else ("lanes8" if x_avg > 16.0 else "thread")
    avg = float(P.slots.sum()) / n
    dense_ok = n_cols * 9 + 16 <= DENSE_LDS
    if avg > 256.0 and dense_ok:
        return count, "dense"
    if avg <= 24.0:
        return count, "lists12"
    if avg <= 256.0:
        if avg <= 110.0:
            return count, ("lanes16" if 0.0 < x_avg <= 14.0 and avg <= 48.0 else "lanes32")
        return count, "lanes64"
    return count, "rows"


def lane_pass(P, i, capp, ht, lanes):
    """Whether row i fits a pass spgemm_rows_lanes<CAPP, HT, LANES>."""
    return P.x_len[i] <= lanes and P.slots[i] <= capp and P.distinct[i] <= ht // 2


# ---- inputs of the transpose ---------------------------------------------------------------------------------------------

def random_rect(n_rows, n_cols, per_row, seed, col_lo=0, empty_rows_every=0):
    """About per_row entries per row (Poisson) on columns col_lo .. n_cols - 1, every empty_rows_every-th row empty."""
    rng = np.random.default_rng(seed)
    ln = np.minimum(rng.poisson(per_row, n_rows), n_cols - col_lo)
    if empty_rows_every:
        ln[empty_rows_every - 1::empty_rows_every] = 0
    rows = [np.sort(rng.choice(np.arange(col_lo, n_cols), k, replace=False)) for k in ln]
    return rows_to_csr(rows, n_cols, rng)


def rows_to_csr(rows, n_cols, rng):
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    idx = (np.concatenate(rows) if len(rows) and indptr[-1] else np.zeros(0)).astype(np.int32)
    return sp.csr_matrix((rng.standard_normal(len(idx)), idx, indptr), shape=(len(rows), n_cols))


TP_PLANTS = {"waves16": 48, "waves17": 49, "len64": 16, "short_sorted": 17, "len65": 24, "len2048": 32, "len2049": 40,
             "long_in_chunk": 8, "short_beside_long": 9, "full_wave": 68, "over_wave": 69}


def transpose_limits_case(seed, with_2049=True):
    """70 waves of 64 rows x 3000 columns, about 1.5 entries per row on the columns from 100 on, every 37th row empty, columns
    90 .. 99 empty, and on the columns TP_PLANTS names:
      waves16 / waves17   one entry in each of 16 / 17 waves (the list of a column takes 16)
      len64 / len65       64 / 65 entries over 32 / 33 waves: a cursor column that sort_csr_rows_seg sorts / hands on
      short_sorted        17 waves, in the chunk of len64: sorted beside it in the same chunk of eight
      len2048 / len2049   every row of waves 0 .. 31 / 32 .. 64 (+ 1): sorted by a workgroup / by one thread
      long_in_chunk       70 entries over 35 waves, with short_beside_long (17 waves) in its chunk of eight: the chunk is listed
      full_wave / over_wave   WAVES (not columns): 64 rows of exactly 240 / 241 entries."""
    rng = np.random.default_rng(seed)
    n_waves, n_cols = 70, 3000
    n_rows = n_waves * 64
    M = random_rect(n_rows, n_cols, 1.5, seed + 1, col_lo=100, empty_rows_every=37).tolil()
    P = TP_PLANTS

    def plant(col, rows):
        for r in rows:
            M[int(r), col] = rng.standard_normal()
    plant(P["waves16"], [64 * w + 3 for w in range(16)])
    plant(P["waves17"], [64 * w + 5 for w in range(20, 37)])
    plant(P["len64"], [64 * w + d for w in range(32) for d in (7, 40)])
    plant(P["short_sorted"], [64 * w + 9 for w in range(40, 57)])
    plant(P["len65"], [64 * w + d for w in range(32) for d in (11, 50)] + [64 * 32 + 1])
    plant(P["len2048"], range(0, 2048))
    if with_2049:
        plant(P["len2049"], range(2048, 2048 + 2049))
    plant(P["long_in_chunk"], [64 * w + d for w in range(35) for d in (13, 33)])
    plant(P["short_beside_long"], [64 * w + 15 for w in range(3, 20)])
    for wave, total in ((P["full_wave"], TP_ENTRIES), (P["over_wave"], TP_ENTRIES + 1)):
        ln = np.full(64, total // 64)
        ln[:total - ln.sum()] += 1
        for d, k in enumerate(rng.permutation(ln)):
            r = 64 * wave + d
            M.rows[r], M.data[r] = [], []
            for c in np.sort(rng.choice(np.arange(100, n_cols), k, replace=False)):
                M[r, int(c)] = rng.standard_normal()
    return canonical(M.tocsr())


def scattered_band_case(seed, n_rows=6000, n_cols=300):
    """A tall band matrix (three entries per row around column i n_cols / n_rows) under random permutations of its rows and
    columns: every column's ~60 entries lie in dozens of waves."""
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n_rows), 3)
    c = (i * n_cols // n_rows + np.tile([-1, 0, 1], n_rows)) % n_cols
    M = sp.csr_matrix((rng.standard_normal(len(i)), (rng.permutation(n_rows)[i], rng.permutation(n_cols)[c])), shape=(n_rows, n_cols))
    return canonical(M)


# ---- inputs of the product -----------------------------------------------------------------------------------------------

def product_route(P, X, n_cols):
    """Per row the pass of spgemm that forms it: "list" (twelve-entry lists), "first" (the branch's own lane-group kernel),
    "listed" (<256, 128, 64> over the list of the rows left), "doubled" (<1024, 512, 64>), "dense", "redo", "rows"."""
    _, branch = product_branch(P, X, n_cols)
    n = P.shape[0]
    dense_ok = n_cols * 9 + 16 <= DENSE_LDS
    fits = lambda capp, ht, lanes: (P.x_len <= lanes) & (P.slots <= capp) & (P.distinct <= ht // 2)
    last = np.where(fits(1024, 512, 64), "doubled", "dense" if dense_ok and branch != "lists12" else "redo")
    if branch in ("dense", "rows", "none"):
        return np.full(n, branch)
    if branch == "lists12":
        return np.where(P.distinct <= 12, "list", last)
    if branch == "lanes64":
        return np.where(fits(512, 256, 64), "first", last)
    first = fits(128, 32, 16) if branch == "lanes16" else fits(256, 64, 32)
    return np.where(first, "first", np.where(fits(256, 128, 64), "listed", last))


_L16 = [(16, 128, 16), (17, 100, 16), (16, 129, 16), (16, 128, 17)]
_L32 = [(32, 256, 32), (33, 66, 32), (32, 257, 32), (32, 256, 33)]
_LISTED = [(64, 256, 64), (65, 200, 60), (64, 257, 64), (64, 256, 65)]
_DOUBLED = [(64, 1024, 256), (64, 1025, 256), (64, 1024, 257)]
_L64 = [(64, 512, 128), (65, 200, 100), (64, 513, 128), (64, 512, 129)]

# name -> (arguments of product_case without seed / signed, counting kernel, row kernel, the passes that must form a row)
PRODUCT_CASES = {
    "lists12": (dict(n=600, n_mid=500, n_cols=700, x_len=lambda r: r.integers(2, 5), y_len=lambda r: r.integers(2, 5),
                     planted=[(3, 12, 12), (3, 13, 13), (7, 28, 13)] + _DOUBLED + [(65, 130, 100)], empty_x=(0, 77, 599),
                     empty_y_every=41), "thread", "lists12", {"list", "doubled", "redo"}),
    "lanes16_dense": (dict(n=500, n_mid=450, n_cols=3000, x_len=lambda r: r.integers(5, 8), y_len=lambda r: r.integers(4, 7),
                           planted=_L16 + _LISTED + _DOUBLED, empty_x=(1, 250)), "thread", "lanes16",
                      {"first", "listed", "doubled", "dense"}),
    "lanes16_redo": (dict(n=500, n_mid=450, n_cols=17065, x_len=lambda r: r.integers(5, 8), y_len=lambda r: r.integers(4, 7),
                          planted=_L16 + _LISTED + _DOUBLED), "thread", "lanes16", {"first", "listed", "doubled", "redo"}),
    "lanes32_dense": (dict(n=400, n_mid=700, n_cols=17064, x_len=lambda r: r.integers(18, 23), y_len=lambda r: r.integers(2, 5),
                           planted=_L32 + _LISTED + _DOUBLED, empty_y_every=29), "lanes8", "lanes32",
                      {"first", "listed", "doubled", "dense"}),
    "lanes32_redo": (dict(n=401, n_mid=700, n_cols=20000, x_len=lambda r: r.integers(18, 23), y_len=lambda r: r.integers(2, 5),
                          planted=_L32 + _LISTED + _DOUBLED), "lanes8", "lanes32", {"first", "listed", "doubled", "redo"}),
    "lanes64_dense": (dict(n=300, n_mid=900, n_cols=5000, x_len=lambda r: r.integers(50, 56), y_len=lambda r: r.integers(2, 5),
                           planted=_L64 + _DOUBLED), "lanes32", "lanes64", {"first", "doubled", "dense"}),
    "lanes64_redo": (dict(n=301, n_mid=900, n_cols=18000, x_len=lambda r: r.integers(50, 56), y_len=lambda r: r.integers(2, 5),
                          planted=_L64 + _DOUBLED), "lanes32", "lanes64", {"first", "doubled", "redo"}),
    "dense": (dict(n=200, n_mid=600, n_cols=2000, x_len=lambda r: r.integers(28, 33), y_len=lambda r: r.integers(8, 13),
                   empty_x=(3,)), "lanes8", "dense", {"dense"}),
    "rows": (dict(n=64, n_mid=600, n_cols=17065, x_len=lambda r: r.integers(28, 33), y_len=lambda r: r.integers(8, 13)),
             "lanes8", "rows", {"rows"}),
}


def build_product_case(name, signed, seed=11):
    kw, count, rows, passes = PRODUCT_CASES[name]
    X, Y, where = product_case(seed=seed + (1 if signed else 0), signed=signed, **kw)
    return X, Y, where, count, rows, passes


def cancellation_case(seed=5):
    """The "lists12" background with one planted exact cancellation: row 10 of X = (+1) row a + (-1) row b of Y, where rows
    a and b of Y share exactly one column, with the same value there."""
    X, Y, _ = product_case(n=200, n_mid=150, n_cols=300, seed=seed, x_len=lambda r: r.integers(2, 5),
                           y_len=lambda r: r.integers(2, 5), signed=True)
    X, Y = X.tolil(), Y.tolil()
    Y.rows[3], Y.data[3] = [7, 20, 100], [1.5, 0.75, 2.0]
    Y.rows[4], Y.data[4] = [20, 31], [0.75, -1.25]
    X.rows[10], X.data[10] = [3, 4], [1.0, -1.0]
    return canonical(X.tocsr()), canonical(Y.tocsr()), (10, 20)


# name -> (shapes of Z, of Y and of X by their row / entry lengths, row kernel of the SECOND product X (Y Z))
CHAIN_CASES = {
    "lists12": (dict(n=300, n_mid=260, n_cols=400, x_len=lambda r: r.integers(1, 4), y_len=lambda r: r.integers(1, 4)),
                350, lambda r: r.integers(2, 5), "lists12"),
    "lanes": (dict(n=300, n_mid=260, n_cols=900, x_len=lambda r: r.integers(2, 5), y_len=lambda r: r.integers(2, 5)),
              333, lambda r: r.integers(5, 9), "lanes32"),
    "dense": (dict(n=300, n_mid=260, n_cols=1500, x_len=lambda r: r.integers(4, 7), y_len=lambda r: r.integers(4, 7)),
              150, lambda r: r.integers(12, 16), "dense"),
}


def build_chain_case(name, signed, seed=21):
    kw, n_x, x_len, branch = CHAIN_CASES[name]
    Y, Z, _ = product_case(seed=seed, signed=signed, **kw)
    rng = np.random.default_rng(seed + 2)
    rows = [np.sort(rng.choice(Y.shape[0], int(x_len(rng)), replace=False)) for _ in range(n_x)]
    rows[n_x // 2] = np.zeros(0, np.int64)
    X = rows_to_csr(rows, Y.shape[0], rng)
    X.data[:] = rng.uniform(0.5, 2.0, X.nnz) * (rng.choice([-1.0, 1.0], X.nnz) if signed else 1.0)
    return X, Y, Z, branch

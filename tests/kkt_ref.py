"""The contract of the padne_kkt plan (csrc/kkt.hip) in plain numpy, in np.longdouble: what every stage of the plan has to
produce from the plan's own inputs, and beside each value what the rounding bounds of tests/test_kkt_plan_vs_reference.py need.

    P        [N x n_free] 0/1: unknown i is reduced unknown imap[i] (imap[i] < 0: none)
    c        known part of the potentials, v = c + P y
    A_ref    = -P^T L P
    b_ref    = -P^T (R - L c)
    b_extra  = P^T gamma_k
    rho_ref  = R - L V   and  L Z_k  at the probed unknowns
    norm_ref = ||L V_j - R_j||_2

Nothing of the device code or of padne_amd.reduction is restated: the index map is a cumulative count of its own, the sums are
sorted-key reductions.  Everything is vectorised over the COO form of L (the large test system has 2 M non-zeros).

Envelopes.  For a row i of L:  m_i = its number of entries,  E_i = |r_i| + sum_k |L_ik x_k|  (x the vector the row multiplies).
A product row summed in ANY order, fused or not, and subtracted from r_i is within (m_i + 2) u E_i of the exact value (m_i
products, m_i - 1 additions, one subtraction, (1 + u)^(m_i + 1) - 1 <= (m_i + 2) u for the sizes here).  For a reduced row t the
sums of (m_i + 2) and of E_i over the rows i that add into it: adding g rows costs g - 1 further additions, each at most
u times the running sum <= sum E_i, so  u * sum(m_i + 2) * sum(E_i)  bounds the whole row (it is generous by design: the
product of the sums, not the sum of the products).
"""
import numpy as np
import pytest
import scipy.sparse as sp

LD = np.longdouble
U = 2.0 ** -53
if not float(np.finfo(LD).eps) < 2e-19:
    pytest.skip("np.longdouble has no 64-bit significand here: no high-precision reference", allow_module_level=True)


# ---- the products' layout (kkt.hip, "blocks of right-hand sides") -------------------------------------------------------
# Columns in groups of 8, group g at offset 8 g N, laid out [N][w]; w = 8 for a full group, a last group of `count` columns
# is widened to 1, 2, 4 or 8 (spare columns zero).

def group_width(count):
    return 8 if count >= 5 else 4 if count >= 3 else count


def block_width(n_cols):
    return 8 * (n_cols // 8) + (group_width(n_cols % 8) if n_cols % 8 else 0)


def gidx(N, n_cols, j, i):
    """Position of entry (unknown i, column j) of a block of n_cols columns; i may be an array."""
    g = j // 8
    return g * 8 * N + np.asarray(i, dtype=np.int64) * group_width(min(8, n_cols - 8 * g)) + (j % 8)


def from_layout(flat, N, n_cols):
    """(N, n_cols) array of a block stored in the products' layout."""
    rows = np.arange(N, dtype=np.int64)
    return np.stack([flat[gidx(N, n_cols, j, rows)] for j in range(n_cols)], axis=1) if N else np.zeros((0, n_cols), flat.dtype)


def spare_entries(flat, N, n_cols):
    """The entries of the layout that belong to no column (the widened last group's spare columns)."""
    used = np.zeros(N * block_width(n_cols), dtype=bool)
    rows = np.arange(N, dtype=np.int64)
    for j in range(n_cols):
        used[gidx(N, n_cols, j, rows)] = True
    return flat[~used]


# ---- the index map ------------------------------------------------------------------------------------------------------

def index_map(N, n_potential, elim, tied):
    """int32[N]: i - #{e in elim : e < i} for the potentials that are not eliminated, members through their representative,
    -1 for everything else."""
    elim = np.asarray(elim, dtype=np.int64)
    gone = np.zeros(N, dtype=np.int64)
    gone[elim] = 1
    before = np.cumsum(gone) - gone                         # eliminated unknowns in front of i
    imap = np.arange(N, dtype=np.int64) - before
    imap[gone == 1] = -1
    imap[n_potential:] = -1
    for member, rep in tied:
        imap[member] = imap[rep]
    return imap.astype(np.int32)


def segment_sum(keys, values, n):
    """out[t] = sum of values[keys == t] (rows of a 2-D `values`), in the type of `values`, for t in [0, n)."""
    values = np.asarray(values)
    out = np.zeros((n,) + values.shape[1:], dtype=values.dtype)
    if len(keys) == 0:
        return out
    order = np.argsort(keys, kind="stable")
    ks = np.asarray(keys)[order]
    first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    out[ks[first]] = np.add.reduceat(values[order], first, axis=0)
    return out


def worst_ratio(diff, bound):
    """max of |diff| / bound as a float (0 / 0 = 0, x / 0 = inf): how much of a bound was used; <= 1 means it held."""
    diff, bound = np.abs(np.asarray(diff, dtype=LD)).reshape(-1), np.asarray(bound, dtype=LD).reshape(-1)
    if diff.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(diff == 0, 0, diff / bound)
    return float(q.max())


class Reference:
    """The contract for one plan: L (scipy CSR, N x N), the map (from the lists, or a given one) and n_free."""

    def __init__(self, L, n_potential, elim=(), tied=(), imap=None, n_free=None):
        L = sp.csr_matrix(L)
        L.sort_indices()
        self.L = L
        self.N = N = L.shape[0]
        self.n_potential = int(n_potential)
        self.imap = index_map(N, n_potential, elim, tied) if imap is None else np.asarray(imap, dtype=np.int32)
        self.n_free = int(self.imap.max(initial=-1)) + 1 if n_free is None else int(n_free)
        self.ptr = L.indptr.astype(np.int64)
        self.m = np.diff(self.ptr)                                            # m_i
        self.row = np.repeat(np.arange(N, dtype=np.int64), self.m)
        self.col = L.indices.astype(np.int64)
        self.data = L.data.astype(LD)
        self.absdata = np.abs(self.data)
        self.mapped = np.flatnonzero(self.imap >= 0)                          # the rows that add into a reduced row ...
        self.target = self.imap[self.mapped].astype(np.int64)                 # ... and which
        self.m_sum = segment_sum(self.target, (self.m[self.mapped] + 2).astype(np.float64), self.n_free)

    # -- products with L, exact to the rounding of longdouble
    def _rows(self, terms):
        out = np.zeros((self.N,) + terms.shape[1:], dtype=terms.dtype)
        full = self.m > 0
        if len(terms):
            out[full] = np.add.reduceat(terms, self.ptr[:-1][full], axis=0)
        return out

    def matmul(self, X):
        """L X for X of shape (N, k)."""
        X = np.asarray(X, dtype=LD).reshape(self.N, -1)
        return self._rows(self.data[:, None] * X[self.col])

    def absmul(self, X):
        """sum_k |L_ik X_kj|."""
        X = np.abs(np.asarray(X, dtype=LD).reshape(self.N, -1))
        return self._rows(self.absdata[:, None] * X[self.col])

    def project(self, X):
        """P^T X for X of shape (N, k)."""
        return segment_sum(self.target, np.asarray(X)[self.mapped], self.n_free)

    def expand(self, Y):
        """P Y for Y of shape (n_free, k)."""
        Y = np.asarray(Y)
        out = np.zeros((self.N, Y.shape[1]), dtype=Y.dtype)
        out[self.mapped] = Y[self.target]
        return out

    # -- the stages
    def known(self, known_idx, known_val, n_cols):
        """c (N, n_cols) from known_idx [n_known] and known_val (n_cols, n_known)."""
        c = np.zeros((self.N, n_cols), dtype=LD)
        if len(known_idx):
            c[np.asarray(known_idx, dtype=np.int64)] = np.asarray(known_val, dtype=LD).reshape(n_cols, -1).T
        return c

    def reduced_matrix(self):
        """A_ref = -P^T L P as sorted COO: (t, u, value, q = entries of L merged into (t, u), sum of their absolute values)."""
        t, u = self.imap[self.row].astype(np.int64), self.imap[self.col].astype(np.int64)
        keep = (t >= 0) & (u >= 0)
        key = t[keep] * max(self.n_free, 1) + u[keep]
        order = np.argsort(key, kind="stable")
        ks = key[order]
        first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]])) if len(ks) else np.zeros(0, dtype=np.int64)
        vals = -self.data[keep][order]
        if len(ks) == 0:
            z = np.zeros(0, dtype=np.int64)
            return z, z, np.zeros(0, LD), z, np.zeros(0, LD)
        summed = np.add.reduceat(vals, first)
        mass = np.add.reduceat(np.abs(vals), first)
        q = np.diff(np.append(first, len(ks)))
        return ks[first] // max(self.n_free, 1), ks[first] % max(self.n_free, 1), summed, q, mass

    def rhs(self, R, c=None):
        """(b_ref (n_free, k), bound (n_free, k)) with bound = u * sum(m_i + 2) * sum(E_i), E_i = |r_i| + sum_k |L_ik c_k|."""
        R = np.asarray(R, dtype=LD).reshape(self.N, -1)
        resid, E = R, np.abs(R)
        if c is not None:
            resid = R - self.matmul(c)
            E = E + self.absmul(c)
        return -self.project(resid), U * self.m_sum[:, None] * self.project(E)

    def extra_rhs(self, extras):
        """b_extra (n_free, n_extra) = P^T gamma_k for the extras given as {row: value} columns."""
        out = np.zeros((self.n_free, len(extras)), dtype=LD)
        for k, col in enumerate(extras):
            for row, val in col.items():
                if self.imap[row] >= 0:
                    out[self.imap[row], k] += LD(val)
        return out

    def probes(self, R, V, probe_idx):
        """(rho_ref, bound), both (n_probe, k): rho = R - L V at the probes, bound = (m_i + 2) u E_i."""
        p = np.asarray(probe_idx, dtype=np.int64)
        R = np.asarray(R, dtype=LD).reshape(self.N, -1)
        rho = R - self.matmul(V)
        E = np.abs(R) + self.absmul(V)
        return rho[p], (self.m[p] + 2)[:, None] * U * E[p]

    def extra_probes(self, Z, probe_idx):
        """((L Z_k) at the probes, bound = (m_i + 1) u sum_k |L_ik Z_k|), both (n_probe, n_extra); Z of shape (N, n_extra)."""
        p = np.asarray(probe_idx, dtype=np.int64)
        return self.matmul(Z)[p], (self.m[p] + 1)[:, None] * U * self.absmul(Z)[p]

    def residual_norms(self, R, V):
        """(norm_ref [k], bound [k]): ||L V_j - R_j||_2 and ||e_j||_2 + (n + 8) u norm_ref_j with e_ij = (m_i + 2) u E_ij:
        e for the rounding of every row's difference, n + 8 for the squares, their sum over n rows in any order and the
        square root."""
        R = np.asarray(R, dtype=LD).reshape(self.N, -1)
        d = self.matmul(V) - R
        e = (self.m + 2)[:, None] * U * (np.abs(R) + self.absmul(V))
        norm = np.sqrt((d * d).sum(axis=0))
        return norm, np.sqrt((e * e).sum(axis=0)) + (self.N + 8) * U * norm

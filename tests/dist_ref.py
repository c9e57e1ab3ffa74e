"""Row-partitioned operators and vectors put back together on the host (numpy / scipy only; nothing of the device's).

A rank q of W owns n_q consecutive rows of a global operator.  Its piece is a CSR matrix of shape n_q x (n_q + W m): the
first n_q columns are its own unknowns, column n_q + p m + e is the e-th value rank p exports -- exports[p][e], an index
into rank p's own unknowns -- and every rank's segment is padded to the common length m = max_p len(exports[p]).  With
off_p the first global row of rank p (rank order), slot (p, e) therefore stands for the global column off_p + exports[p][e].

    stack(pieces, exports, m)             the global square matrix the pieces are the rows of
    split(A, owner_ranges, exports, m)    its inverse: the pieces of a global matrix under given export lists
    blockdiag_P(pieces)                   per-rank prolongators n_q x c_q -> the global one (aggregates never cross ranks)
    owned_block(piece)                    the square block a rank aggregates and builds its prolongator from
    halo_expected(xs, exports, m)         what an exchange of the owned vectors xs must leave in every rank's exchange area
"""
import numpy as np
import scipy.sparse as sp


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def _checked_exports(exports, sizes, m):
    out = []
    for p, e in enumerate(exports):
        e = np.asarray(e, dtype=np.int64).reshape(-1)
        assert len(e) <= m, f"rank {p} exports {len(e)} values, the segment holds {m}"
        assert len(e) == 0 or (e.min() >= 0 and e.max() < sizes[p]), f"export list of rank {p} leaves its {sizes[p]} unknowns"
        assert len(np.unique(e)) == len(e), f"rank {p} exports an unknown twice"
        out.append(e)
    return out


def stack(pieces, exports, m):
    """Global square CSR matrix of the per-rank pieces (rank order).  Asserts that every piece has n_q + W m columns, that
    the export lists are in range, and that every slot a piece references is one its rank really exports (e < len(exports[p])).
    Entries of a row that land on the same global column are summed."""
    W = len(pieces)
    assert len(exports) == W
    pieces = [sp.csr_matrix(p) for p in pieces]
    sizes = [p.shape[0] for p in pieces]
    off = _offsets(sizes)
    exports = _checked_exports(exports, sizes, m)
    rows, cols, vals = [], [], []
    for q, A in enumerate(pieces):
        n_q = sizes[q]
        assert A.shape[1] == n_q + W * m, f"piece of rank {q}: {A.shape[1]} columns, expected {n_q} + {W} x {m}"
        A = A.tocoo()
        r, c = A.row.astype(np.int64), A.col.astype(np.int64)
        g = np.empty(len(c), dtype=np.int64)
        own = c < n_q
        g[own] = off[q] + c[own]
        s = c[~own] - n_q
        p, e = s // max(m, 1), s % max(m, 1)
        n_exp = np.array([len(x) for x in exports], dtype=np.int64)
        bad = e >= n_exp[p]
        assert not bad.any(), (f"rank {q} reads slot (rank {int(p[bad][0])}, position {int(e[bad][0])}), but that rank exports "
                               f"only {int(n_exp[p[bad][0]])} values")
        assert not (p == q).any(), f"rank {q} reads a slot of its own segment"
        flat = np.concatenate([off[k] + exports[k] for k in range(W)]) if W else np.zeros(0, np.int64)
        start = _offsets(n_exp)
        g[~own] = flat[start[p] + e]
        rows.append(off[q] + r)
        cols.append(g)
        vals.append(A.data)
    N = int(off[-1])
    G = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsr()
    G.sum_duplicates()
    G.sort_indices()
    return G


def split(A_global, owner_ranges, exports, m):
    """The pieces of a global matrix: rank q owns rows owner_ranges[q] = (a_q, b_q) (consecutive, in rank order); a column
    of another rank p must be one of exports[p] and goes to slot n_q + p m + position."""
    A = sp.csr_matrix(A_global)
    W = len(owner_ranges)
    sizes = [b - a for a, b in owner_ranges]
    off = _offsets(sizes)
    assert [a for a, _ in owner_ranges] == list(off[:-1]) and owner_ranges[-1][1] == A.shape[0] == A.shape[1]
    exports = _checked_exports(exports, sizes, m)
    pieces = []
    for q, (a, b) in enumerate(owner_ranges):
        B = A[a:b].tocoo()
        c = B.col.astype(np.int64)
        p = np.searchsorted(off, c, side="right") - 1
        loc = c - off[p]
        out = np.where(p == q, loc, -1)
        for k in range(W):
            sel = (p == k) & (k != q)
            if not sel.any():
                continue
            order = np.argsort(exports[k], kind="stable")
            pos = np.searchsorted(exports[k][order], loc[sel])
            pos = np.minimum(pos, max(len(order) - 1, 0))
            assert len(order) and (exports[k][order][pos] == loc[sel]).all(), f"rank {q} needs a value rank {k} does not export"
            out[sel] = sizes[q] + k * m + order[pos]
        P = sp.coo_matrix((B.data, (B.row, out)), shape=(b - a, sizes[q] + W * m)).tocsr()
        P.sort_indices()
        pieces.append(P)
    return pieces


def owned_block(piece):
    """The owned x owned block of a rank's piece as the setup specifies it (csrc/amg.hip, block_fill): the couplings to other
    ranks are dropped and their sum is lumped onto the diagonal -- the row sums of the block are those of the full operator,
    so the smoothed prolongator keeps its unit row sums at the exchanged vertices -- unless that would leave 30 % of the
    diagonal or less, in which case the diagonal stays as it is."""
    A = sp.csr_matrix(piece)
    n = A.shape[0]
    blk = A[:, :n].tocsr()
    dropped = np.asarray(A[:, n:].sum(axis=1)).ravel()
    d = blk.diagonal()
    lumped = (dropped != 0.0) & (d + dropped > 0.3 * d)
    blk = blk.tolil()
    blk.setdiag(np.where(lumped, d + dropped, d))
    blk = blk.tocsr()
    blk.sort_indices()
    return blk


def blockdiag_P(pieces):
    """Global prolongator of the per-rank ones (aggregates are numbered within a rank; coarse unknowns in rank order)."""
    P = sp.block_diag([sp.csr_matrix(p) for p in pieces], format="csr")
    P.sort_indices()
    return P


def halo_expected(xs, exports, m):
    """(area, defined): the exchange area [W m] every rank must hold after one exchange of the owned vectors xs[p] -- segment
    p starts with xs[p][exports[p]] -- and which of its slots are defined (the padding behind a rank's exports is not)."""
    W = len(xs)
    exports = _checked_exports(exports, [len(x) for x in xs], m)
    dtype = np.asarray(xs[0]).dtype if W else np.float64
    area = np.zeros(W * m, dtype=dtype)
    defined = np.zeros(W * m, dtype=bool)
    for p in range(W):
        k = len(exports[p])
        area[p * m:p * m + k] = np.asarray(xs[p])[exports[p]]
        defined[p * m:p * m + k] = True
    return area, defined

"""Non-canonical uploads: raw CSR arrays whose rows are permuted and name columns more than once, of matrices whose canonical
form is one definite matrix bit for bit (tests/test_noncanonical_ref_host.py holds these inputs to their conditions on the
host, tests/test_noncanonical_upload.py holds the device to them).

``padne_csr_from_host`` promises that such arrays mean the matrix their entries sum to.  A test of that promise needs inputs
whose sum does not depend on the order of the parts, or the "canonical matrix" would be a matter of rounding: every matrix
handed to ``scramble`` has its values rounded to float32 first (``round32``), and an entry is split into v/2, v/2 or v/2, v/4,
v/4 -- powers of two, so every part and every partial sum of parts (v/4, v/2, 3v/4, v) is exact in float64 in whatever order
they are added.  Nothing here goes through a scipy method that sorts or sums (``csr_matrix((data, indices, indptr))`` keeps the
arrays as they are; ``sort_indices`` is not stable and ``sum_duplicates`` adds in its own order).
"""
import ctypes as C
import functools

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import amg_ref
import helpers as H

LD = np.longdouble


def round32(A):
    """The canonical CSR of A with every value rounded to float32 (kept as float64); no value may round to zero."""
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sum_duplicates()
    A.sort_indices()
    A = sp.csr_matrix((A.data.astype(np.float32).astype(np.float64), A.indices.astype(np.int32), A.indptr.astype(np.int32)),
                      shape=A.shape)
    assert A.data.all() and A.has_canonical_format
    return A


def _not_ascending(cols, rng):
    """A permutation of the positions of ``cols`` under which they are NOT in non-decreasing order (two distinct columns at
    least are asked for)."""
    for _ in range(64):
        p = rng.permutation(len(cols))
        if (np.diff(cols[p]) < 0).any():
            return p
    return np.argsort(cols, kind="stable")[::-1]


def scramble(A, seed):
    """Raw (indptr int32, indices int32, data float64) of the canonical matrix A: every row of two or more entries permuted so
    that its columns do not ascend, entries split into two or three stored parts.  A diagonal (column == row) is split in about
    a third of the rows, one or two off-diagonals in about half; the first row with a diagonal has it split in three, a row
    whose only entry is its diagonal has it split, and the longest row has a third of its entries split."""
    A = sp.csr_matrix(A)
    assert A.has_canonical_format and A.dtype == np.float64
    rng = np.random.default_rng(seed)
    lens = np.diff(A.indptr)
    longest = int(np.argmax(lens)) if len(lens) else -1
    out_ptr, out_cols, out_vals = [0], [], []
    three_done = False
    for i in range(A.shape[0]):
        k0, k1 = A.indptr[i], A.indptr[i + 1]
        cols, vals = A.indices[k0:k1], A.data[k0:k1]
        m = k1 - k0
        parts = np.ones(m, np.int64)
        at = np.flatnonzero(cols == i)
        off = np.flatnonzero(cols != i)
        if len(at):
            if not three_done:
                parts[at[0]] = 3
                three_done = True
            elif m == 1 or rng.random() < 0.34:
                parts[at[0]] = 2 + int(rng.random() < 0.3)
        if len(off):
            if i == longest:
                pick = rng.choice(off, size=max(1, len(off) // 3), replace=False)
            elif rng.random() < 0.5:
                pick = rng.choice(off, size=min(len(off), 1 + int(rng.random() < 0.4)), replace=False)
            else:
                pick = off[:0]
            parts[pick] = 2 + (rng.random(len(pick)) < 0.3)
        c = np.repeat(cols, parts)
        v = np.repeat(vals, parts)
        first = np.cumsum(parts) - parts
        # v/2 for the first part of a split entry, v/2 (two parts) or v/4, v/4 (three) for the rest
        rank = np.arange(len(c)) - np.repeat(first, parts)
        np_of = np.repeat(parts, parts)
        v = np.where(np_of == 1, v, np.where(rank == 0, v * 0.5, np.where(np_of == 2, v * 0.5, v * 0.25)))
        if m >= 2:
            p = _not_ascending(c, rng)
        else:
            p = np.arange(len(c))
        out_cols.append(c[p])
        out_vals.append(v[p])
        out_ptr.append(out_ptr[-1] + len(c))
    indices = np.concatenate(out_cols).astype(np.int32) if out_cols else np.zeros(0, np.int32)
    data = np.concatenate(out_vals).astype(np.float64) if out_vals else np.zeros(0, np.float64)
    return np.asarray(out_ptr, np.int32), indices, data


def canonical_of(indptr, indices, data, shape, reverse=False):
    """The canonical (indptr, indices, data) of raw arrays, the parts of a column added in float64 in the order of their position
    (``reverse``: in the opposite order).  Plain numpy, no scipy method."""
    rows = np.repeat(np.arange(shape[0], dtype=np.int64), np.diff(indptr))
    pos = np.arange(len(indices), dtype=np.int64)
    order = np.lexsort((-pos if reverse else pos, indices, rows))
    r, c, v = rows[order], indices[order].astype(np.int64), data[order]
    first = np.r_[True, (r[1:] != r[:-1]) | (c[1:] != c[:-1])] if len(r) else np.zeros(0, bool)
    start = np.flatnonzero(first)
    length = np.diff(np.r_[start, len(r)])
    s = np.zeros(len(start), np.float64)
    for j in range(int(length.max()) if len(length) else 0):
        on = length > j
        s[on] = s[on] + v[start[on] + j]
    ptr = np.zeros(shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r[start], minlength=shape[0]), out=ptr[1:])
    return ptr.astype(np.int32), c[start].astype(np.int32), s


def raw_stats(A, raw):
    """What the host test asserts of a scrambled matrix, row by row: ``ascending`` (the raw columns are in non-decreasing
    order), the number of stored parts of the diagonal, the largest number of parts of an off-diagonal."""
    indptr, indices, _ = raw
    n = A.shape[0]
    rows = np.repeat(np.arange(n), np.diff(indptr))
    ascending = np.ones(n, bool)
    step = np.flatnonzero((rows[1:] == rows[:-1]) & (indices[1:] < indices[:-1]))
    ascending[rows[step]] = False
    key, count = np.unique(rows.astype(np.int64) * A.shape[1] + indices, return_counts=True)
    kr, kc = key // A.shape[1], key % A.shape[1]
    diag_parts = np.zeros(n, np.int64)
    diag_parts[kr[kr == kc]] = count[kr == kc]
    off_parts = np.zeros(n, np.int64)
    np.maximum.at(off_parts, kr[kr != kc], count[kr != kc])
    return dict(ascending=ascending, diag_parts=diag_parts, off_parts=off_parts, raw_len=np.diff(indptr), len=np.diff(A.indptr))


def upload_raw(ctx, indptr, indices, data, shape):
    """The arrays as they stand through padne_csr_from_host (Context.csr_from_scipy would sum and sort them first)."""
    from padne_amd import _hip
    indptr, indices, data = (np.ascontiguousarray(indptr, np.int32), np.ascontiguousarray(indices, np.int32),
                             np.ascontiguousarray(data, np.float64))
    assert len(indptr) == shape[0] + 1 and len(indices) == len(data) == indptr[-1]
    h = _hip._P()
    _hip._check(ctx._lib.padne_csr_from_host(ctx._h, int(shape[0]), int(shape[1]), _hip._ptr(indptr, _hip._PI32),
                                             _hip._ptr(indices, _hip._PI32), _hip._ptr(data, _hip._PF64), C.byref(h)))
    return _hip.CsrMatrix(ctx, h)


# ---- the systems (each built once) ---------------------------------------------------------------------------------------

RECT_HUB_ROW, RECT_HUB_COL = 17, 23
LARGE_HUB = 70


@functools.lru_cache(maxsize=None)
def rect_system():
    """H.random_csr(300, 420, 9, 12) with a hub row (row 17: 400 of the 420 columns) and a hub column (column 23 in 200 rows):
    rectangular, empty rows, rows of one entry."""
    rng = np.random.default_rng(120)
    M = H.random_csr(300, 420, 9, 12).tolil()
    M[RECT_HUB_ROW, 10:410] = rng.uniform(-1, 1, 400)
    M[40:240, RECT_HUB_COL] = rng.uniform(-1, 1, (200, 1))
    return round32(M.tocsr())


@functools.lru_cache(maxsize=None)
def small_spd():
    """amg_ref.layered_matrix(2, 10, 8, 4) (159 unknowns) and one unknown more that is coupled to nothing -- the row whose only
    entry is its diagonal, which no row of the board is: 160 unknowns, the dense inverse as the whole preconditioner."""
    A = amg_ref.layered_matrix(2, 10, 8, 4)
    assert A.shape == (159, 159)
    return round32(sp.block_diag([A, sp.csr_matrix([[float(np.median(A.diagonal()))]])]).tocsr())


@functools.lru_cache(maxsize=None)
def mid_spd():
    """Case a of tests/test_amg_vs_reference.py: 2399 unknowns, three levels under PADNE_AMG_COARSE_N=64."""
    A = round32(amg_ref.layered_matrix(2, 40, 30, 4))
    assert A.shape == (2399, 2399)
    return A


@functools.lru_cache(maxsize=None)
def large_system():
    """amg_ref.layered_matrix(2, 300, 240, 6) (143999 rows of at most 13 entries: the x-window plan) with a hub row (row 70:
    1300 further columns, a 64-row tile of several passes of 512 entries) and a hub column (column 70 in 600 further rows)."""
    A = amg_ref.layered_matrix(2, 300, 240, 6)
    n = A.shape[0]
    assert n == 143999
    rng = np.random.default_rng(144)
    rows = np.r_[np.full(1300, LARGE_HUB), np.arange(3000, 3600)]
    cols = np.r_[np.arange(200, 1500), np.full(600, LARGE_HUB)]
    scale = float(np.abs(A.data).mean())
    B = sp.csr_matrix((scale * rng.uniform(0.5, 2.0, 1900) * rng.choice([-1.0, 1.0], 1900), (rows, cols)), shape=A.shape)
    return round32((A + B).tocsr())


@functools.lru_cache(maxsize=None)
def kkt_system():
    """(L, r, n_potential): the whole system of the 2 x 10 x 8 board in the reference's layout (potentials, then the multiplier
    of the ground constraint), as the oracle assembles it, values rounded to float32: what solve_system takes."""
    from oracle import padne_oracle as O
    from padne_amd import synthetic
    s = synthetic.layered_system(2, 10, 8, via_lattice=4)
    els = [("R", int(a), int(b), float(r)) for a, b, r in zip(*s.resistors)]
    els += [("I", int(f), int(t), float(i)) for f, t, i in zip(*s.current_sources)]
    Lo, ro = O.assemble_system([(m[0], m[1], m[2]) for m in s.meshes], 0, els, s.ground)
    return round32(Lo), np.asarray(ro, np.float64), s.n_vertices


@functools.lru_cache(maxsize=None)
def raw_of(name):
    """(canonical A, raw arrays) of a system by name, scrambled with its own fixed seed."""
    A = SYSTEMS[name]()
    return A, scramble(A, SEEDS[name])


SYSTEMS = {"rect": rect_system, "small": small_spd, "mid": mid_spd, "large": large_system}
SEEDS = {"rect": 1, "small": 2, "mid": 3, "large": 4}
SPD = ("small", "mid")


# ---- the direct solution the device is held to ---------------------------------------------------------------------------

def direct_solution(A, B, rounds=4):
    """A^-1 B in longdouble: scipy's sparse LU, then iterative refinement with the residual formed in longdouble.  Returns
    (X longdouble, the largest last correction relative to max |X|: the reference's own error is below that)."""
    A = sp.csr_matrix(A)
    B = np.asarray(B, np.float64)
    B2 = B.reshape(len(B), -1)
    lu = spla.splu(A.tocsc())
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    aL = A.data.astype(LD)

    def residual(X):
        P = aL[:, None] * X[A.indices]
        AX = np.zeros(X.shape, LD)
        np.add.at(AX, rows, P)
        return B2.astype(LD) - AX
    X = lu.solve(B2).astype(LD)
    last = np.inf
    for _ in range(rounds):
        dx = lu.solve(residual(X).astype(np.float64))
        X = X + dx.astype(LD)
        last = float(np.abs(dx).max() / max(float(np.abs(X).max()), 1e-300))
    return X.reshape(B.shape), last


def positive_definite(A):
    """True if the dense Cholesky factorisation of the (symmetric) matrix succeeds."""
    D = sp.csr_matrix(A).toarray()
    if not np.array_equal(D, D.T):
        return False
    try:
        np.linalg.cholesky(D)
    except np.linalg.LinAlgError:
        return False
    return True


def right_hand_side(A, seed=7, k=None):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, A.shape[0] if k is None else (A.shape[0], k))

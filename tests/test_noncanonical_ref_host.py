"""The inputs of tests/test_noncanonical_upload.py are what they claim (no GPU): conditions on tests/noncanonical_ref.py, not
measurements.  A scrambled matrix must MEAN its canonical matrix exactly and in every order of summation, or the device test
would compare against a matter of rounding; and it must hold every shape of row the device can mistake."""
import numpy as np
import pytest
import scipy.sparse as sp

import noncanonical_ref as N

LD = np.longdouble
SMALL = ("rect", "small", "mid")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.fixture(scope="module", params=list(N.SYSTEMS))
def system(request):
    A, raw = N.raw_of(request.param)
    return request.param, A, raw, N.raw_stats(A, raw)


def test_the_values_are_float32_and_the_matrix_canonical(system):
    name, A, raw, st = system
    assert A.has_canonical_format and A.indptr.dtype == np.int32 and A.indices.dtype == np.int32
    assert np.array_equal(A.data, A.data.astype(np.float32).astype(np.float64)) and A.data.all()
    assert raw[0].dtype == np.int32 and raw[1].dtype == np.int32 and raw[2].dtype == np.float64
    assert raw[0][-1] == len(raw[1]) == len(raw[2]) > A.nnz and (raw[1] >= 0).all() and (raw[1] < A.shape[1]).all()


def test_the_raw_arrays_sum_to_the_matrix_exactly(system):
    """csr_matrix((data, indices, indptr)) keeps the arrays; its dense form, summed in longdouble, is A; and the parts of every
    column added in float64 forwards and backwards give A's bits."""
    name, A, raw, st = system
    indptr, indices, data = raw
    if name in SMALL:
        S = sp.csr_matrix((data, indices, indptr), shape=A.shape)
        assert S.nnz == len(data) and not S.has_canonical_format
        dense = np.zeros(A.shape, LD)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(indptr))
        np.add.at(dense, (rows, indices), data.astype(LD))
        assert np.array_equal(dense, A.toarray().astype(LD))
        assert np.array_equal(S.toarray(), A.toarray())
    for reverse in (False, True):
        ip, ix, d = N.canonical_of(indptr, indices, data, A.shape, reverse=reverse)
        assert np.array_equal(ip, A.indptr) and np.array_equal(ix, A.indices)
        assert np.array_equal(bits(d), bits(A.data)), "the sum of a column's parts depends on their order"
    # every partial sum of the parts of an entry is exact: the parts are v/2, v/2 or v/2, v/4, v/4 of a float32 value
    key = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(indptr)) * A.shape[1] + indices
    whole = A.data[np.searchsorted(np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr)) * A.shape[1] + A.indices, key)]
    ratio = data / whole
    assert np.isin(ratio, [1.0, 0.5, 0.25]).all()


def test_no_row_is_left_ascending(system):
    name, A, raw, st = system
    many = st["len"] >= 2
    assert many.any() and not st["ascending"][many].any()
    # (a row of one entry in two parts repeats its column: not strictly ascending either)
    strictly = np.ones(A.shape[0], bool)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(raw[0]))
    same = np.flatnonzero((rows[1:] == rows[:-1]) & (raw[1][1:] <= raw[1][:-1]))
    strictly[rows[same]] = False
    assert not strictly[st["raw_len"] >= 2].any()


def test_the_shares_of_split_rows(system):
    name, A, raw, st = system
    n = A.shape[0]
    assert (st["off_parts"] >= 2).sum() >= 0.25 * n, "a quarter of the rows hold a split off-diagonal"
    has_diag = st["diag_parts"] >= 1
    if name == "rect":
        # (a random rectangular matrix stores its diagonal in 7 rows of 300: the share is of those)
        assert has_diag.sum() >= 3 and (st["diag_parts"] >= 2).sum() >= 0.1 * has_diag.sum()
    else:
        assert has_diag.all() and (st["diag_parts"] >= 2).sum() >= 0.1 * n, "a tenth of the rows hold a split diagonal"
    assert (st["diag_parts"] == 3).any() and (st["off_parts"] == 3).any()
    assert (st["diag_parts"] == 2).any() and (st["off_parts"] == 2).any()


def test_the_rows_that_are_there_on_purpose():
    A, raw = N.raw_of("rect")
    st = N.raw_stats(A, raw)
    assert (st["len"] == 0).sum() >= 1 and np.array_equal(st["raw_len"] == 0, st["len"] == 0), "an empty row"
    assert st["len"][N.RECT_HUB_ROW] >= 400 and st["raw_len"][N.RECT_HUB_ROW] > 512, "the hub row, stored in over 512 parts"
    assert np.diff(A.tocsc().indptr)[N.RECT_HUB_COL] >= 200
    A, raw = N.raw_of("small")
    st = N.raw_stats(A, raw)
    assert A.shape == (160, 160) and st["len"][159] == 1 and A.indices[A.indptr[159]] == 159
    assert st["diag_parts"][159] >= 2 and st["raw_len"][159] == st["diag_parts"][159], "a row whose only entry is a split diagonal"
    assert (A[:159, :159] != N.round32(N.amg_ref.layered_matrix(2, 10, 8, 4))).nnz == 0
    A, raw = N.raw_of("large")
    st = N.raw_stats(A, raw)
    h = N.LARGE_HUB
    assert st["len"][h] > 512 and st["off_parts"][h] >= 2 and not st["ascending"][h], "a hub row of over 512 entries, permuted and split"
    k0, k1 = raw[0][h], raw[0][h + 1]
    assert len(np.unique(raw[1][k0:k1])) == st["len"][h] and k1 - k0 >= st["len"][h] + st["len"][h] // 4
    assert np.diff(A.tocsc().indptr)[h] > 512
    others = np.delete(st["len"], h)
    assert others.max() <= 14 and A.shape[0] >= 65536, "every other row as short as the x-window plan asks"


@pytest.mark.parametrize("name", N.SPD)
def test_the_rounded_systems_are_still_positive_definite_and_solved(name):
    """Rounding to float32 moves every entry by 6e-8 of itself; the operators stay symmetric positive definite (Cholesky), and
    the longdouble direct solution the device is held to has converged far below the 1e-8 it is compared at."""
    A, _ = N.raw_of(name)
    assert N.positive_definite(A)
    b = N.right_hand_side(A)
    x, last = N.direct_solution(A, b)
    assert last <= 1e-12
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    Ax = np.zeros(A.shape[0], LD)
    np.add.at(Ax, rows, A.data.astype(LD) * x[A.indices])
    # (the residual of the longdouble solution, formed in longdouble: a few units of 2^-64 |A| |x| per entry of a row)
    assert float(np.abs(b.astype(LD) - Ax).max()) <= 1e-16 * float(np.abs(A).max() * np.abs(x).max())


def test_the_kkt_system_of_the_block_solve():
    """The system of the (N, 3) block: the oracle's L of the small board in the reference's layout, values rounded to float32
    (the +-1 of the ground row are exact), still what infer_layout reads as one ground constraint."""
    L, r, n_pot = N.kkt_system()
    from padne_amd.reduction import infer_layout
    layout = infer_layout(L, r)
    assert layout.n_potential == n_pot == L.shape[0] - 1 and len(layout.constraints) == 1
    assert (L != L.T).nnz == 0
    raw = N.scramble(L, 5)
    ip, ix, d = N.canonical_of(*raw, L.shape)
    assert np.array_equal(ip, L.indptr) and np.array_equal(ix, L.indices) and np.array_equal(bits(d), bits(L.data))

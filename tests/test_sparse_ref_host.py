"""tests/sparse_ref.py on the CPU: the references against scipy, plain Python loops and dense longdouble arithmetic on small
inputs, and the input builders against the row lengths, slot counts and averages they claim -- the conditions that
tests/test_sparse_primitives_vs_reference.py asserts again before it looks at the device."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparse_ref as R

LD = np.longdouble


def test_scan_is_the_exclusive_prefix_sum_in_64_bits():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 13, 1000)
    out, total, neg = R.scan(c)
    run = 0
    for i, v in enumerate(c):
        assert out[i] == run
        run += int(v)
    assert out[-1] == run == total and not neg
    out, total, neg = R.scan(np.full(3, R.INT_MAX, np.int32))
    assert out.tolist() == [0, R.INT_MAX, 2 * R.INT_MAX, 3 * R.INT_MAX] and total == 3 * R.INT_MAX
    assert R.scan([1, -1, 2])[2] and R.scan([])[0].tolist() == [0]


def _merge_by_loops(M, row_map, n_rows_out, col_map, scale):
    """The definition, entry after entry: a dict per output row, additions in the order of the source arrays."""
    M = R.canonical(M)
    acc = [dict() for _ in range(n_rows_out)]
    for i in range(M.shape[0]):
        for k in range(M.indptr[i], M.indptr[i + 1]):
            t, c = row_map[i], col_map[M.indices[k]]
            if t < 0 or c < 0:
                continue
            acc[t][c] = acc[t].get(c, np.float64(0.0)) + np.float64(scale) * M.data[k]
    indptr, indices, data = [0], [], []
    for t in range(n_rows_out):
        for c in sorted(acc[t]):
            if acc[t][c] != 0.0:
                indices.append(c)
                data.append(acc[t][c])
        indptr.append(len(indices))
    return np.array(indptr), np.array(indices), np.array(data, np.float64)


@pytest.mark.parametrize("square", [False, True])
def test_merge_equals_the_loop_definition_on_bits_and_scipy_to_rounding(square):
    targets = {0: [3, 1, 7], 1: [2, 2], 2: [40], 4: [5] * 6, 6: [2, 2]}
    M, rm, cm = R.merging_case(targets, 7, 7 if square else 11, seed=1, dropped_rows=(1,), zeros=3, cancel_rows=(6,), square=square)
    nc = 7 if square else 11
    ip, ix, d, slots, tmax = R.merge(M, rm, 7, cm, nc, 0.37)
    ip2, ix2, d2 = _merge_by_loops(M, rm, 7, cm, 0.37)
    assert np.array_equal(ip, ip2) and np.array_equal(ix, ix2) and np.array_equal(d.view(np.int64), d2.view(np.int64))
    assert slots.tolist() == [11, 0, 40, 0, 30, 0, 4] and tmax.tolist() == [7, 0, 40, 0, 5, 0, 2]
    assert ip[2] == ip[1] and ip[7] == ip[6], "the dropped row and the cancelling row are empty"
    Rm = sp.csr_matrix((np.ones((rm >= 0).sum()), (np.flatnonzero(rm >= 0), rm[rm >= 0])), shape=(M.shape[0], 7))
    Cm = sp.csr_matrix((np.ones((cm >= 0).sum()), (np.flatnonzero(cm >= 0), cm[cm >= 0])), shape=(M.shape[1], nc))
    want = (0.37 * (Rm.T @ M @ Cm)).toarray()
    got = sp.csr_matrix((d, ix, ip), shape=(7, nc)).toarray()
    assert np.abs(got - want).max() <= 64 * 2.0 ** -52 * np.abs(want).max()
    assert (M.data == 0).sum() == 3


def test_merge_adds_in_source_order_not_in_another():
    """Three terms whose sum depends on the order: the reference takes the order of the source arrays."""
    M = sp.csr_matrix(np.array([[1.0, 2.0 ** -53, 2.0 ** -53]]))
    ip, ix, d, _, _ = R.merge(M, [0], 1, [0, 0, 0], 1)
    assert d.tolist() == [1.0]                                     # (1 + u) + u = 1, not 1 + 2u
    M = sp.csr_matrix(np.array([[2.0 ** -53, 2.0 ** -53, 1.0]]))
    assert R.merge(M, [0], 1, [0, 0, 0], 1)[2].tolist() == [1.0 + 2.0 ** -52]


@pytest.mark.parametrize("name", ["limits", "mid", "wide"])
@pytest.mark.parametrize("square", [False, True])
def test_merge_cases_hold_what_they_claim(name, square):
    for n_out in ((127, 128, 129) if name == "limits" else (128,)):
        M, rm, cm, nr, nc, plan = R.build_merge_case(name, n_out, square=square)
        ip, ix, d, slots, tmax = R.merge(M, rm, nr, cm, nc, 0.37)
        assert M.shape == (len(rm), len(cm)) and (not square or np.array_equal(rm, cm))
        if name == "limits":
            assert nr == n_out and [int(slots[t]) for t in plan["slots"]] == R.MERGE_LIMIT_SLOTS
            assert all(ip[t + 1] == ip[t] for t in plan["empty"]) and slots[5] == 24 and slots[14] == 40 and slots[11] == 0
            assert ip[11] > ip[10] and ip[13] > ip[12], "merged rows on both sides of the dropped one"
            assert tmax.max() == 40 and (M.data == 0).sum() == 5
            assert R.compact_rows_per_wave(nr, len(ix)) == 64
        else:
            assert R.compact_rows_per_wave(nr, len(ix)) == plan["rpw"] and nr <= 100000
            assert slots.min() > R.MERGE_LDS and slots.max() <= R.MERGE_WAVE


def test_transpose_is_scipys_and_moves_bits():
    M = R.random_rect(300, 170, 4.0, seed=2, empty_rows_every=7)
    ip, ix, d = R.transpose(M)
    T = sp.csr_matrix(M.T)
    T.sort_indices()
    assert np.array_equal(ip, T.indptr) and np.array_equal(ix, T.indices)
    assert np.array_equal(d.view(np.int64), T.data.view(np.int64))
    assert R.transpose(sp.csr_matrix((0, 5)))[0].tolist() == [0] * 6


def test_transpose_cases_hold_what_they_claim():
    M = R.transpose_limits_case(3)
    st, P = R.transpose_stats(M), R.TP_PLANTS
    wpc, ln = st["waves_per_col"], st["col_len"]
    assert M.shape == (70 * 64, 3000)
    assert (wpc[P["waves16"]], wpc[P["waves17"]]) == (R.TP_WAVES, R.TP_WAVES + 1)
    assert (ln[P["len64"]], ln[P["len65"]], ln[P["len2048"]], ln[P["len2049"]]) == (R.TP_SEG, R.TP_SEG + 1, R.TP_LIST, R.TP_LIST + 1)
    for k in ("len64", "len65", "len2048", "len2049", "short_sorted", "long_in_chunk", "short_beside_long"):
        assert st["sorted_cols"][P[k]], k
    assert (st["per_wave"][P["full_wave"]], st["per_wave"][P["over_wave"]]) == (R.TP_ENTRIES, R.TP_ENTRIES + 1)
    assert (st["per_wave"] > R.TP_ENTRIES).sum() == 1, "every other wave goes through its table"
    chunk = lambda c: slice(c // R.TP_CHUNK * R.TP_CHUNK, c // R.TP_CHUNK * R.TP_CHUNK + R.TP_CHUNK)
    assert ln[chunk(P["len64"])].max() == R.TP_SEG and P["short_sorted"] // R.TP_CHUNK == P["len64"] // R.TP_CHUNK
    assert (ln[chunk(P["long_in_chunk"])] > R.TP_SEG).sum() == 1 and P["short_beside_long"] // R.TP_CHUNK == P["long_in_chunk"] // R.TP_CHUNK
    assert (np.diff(M.indptr) == 0).any() and (ln == 0).any(), "empty rows and empty columns"
    # a wave beyond its table sends its columns to their cursors
    M2 = R.random_rect(128, 50, 5.0, seed=4)
    st2 = R.transpose_stats(M2)
    assert (st2["per_wave"] > R.TP_ENTRIES).all() and st2["sorted_cols"][st2["col_len"] > 0].all()
    S = R.scattered_band_case(4)
    s3 = R.transpose_stats(S)
    assert s3["per_wave"].max() <= R.TP_ENTRIES and s3["waves_per_col"].min() > R.TP_WAVES and s3["col_len"].max() <= R.TP_SEG


def _dense_ld(M):
    return np.asarray(sp.csr_matrix(M).toarray(), LD)


def test_product_is_the_dense_longdouble_product_with_its_counts():
    X, Y, where = R.product_case(n=40, n_mid=30, n_cols=50, seed=6, x_len=lambda r: r.integers(1, 6),
                                 y_len=lambda r: r.integers(1, 6), planted=[(3, 12, 5), (5, 9, 9)], signed=True, empty_x=(2,),
                                 empty_y_every=7)
    P = R.product(X, Y)
    D = _dense_ld(X) @ _dense_ld(Y)
    Dabs = np.abs(_dense_ld(X)) @ np.abs(_dense_ld(Y))
    K = (sp.csr_matrix((np.ones(X.nnz), X.indices, X.indptr), shape=X.shape) @
         sp.csr_matrix((np.ones(Y.nnz), Y.indices, Y.indptr), shape=Y.shape)).toarray()
    got = np.zeros(D.shape, LD)
    got[P.row, P.col] = P.val
    assert np.abs(got - D).max() <= 8 * 2.0 ** -63 * Dabs.max()
    assert np.array_equal(K[P.row, P.col], P.count) and (K != 0).sum() == len(P.row), "pattern = the symbolic one"
    assert np.abs(Dabs[P.row, P.col] - P.absval).max() <= 8 * 2.0 ** -63 * Dabs.max()
    assert np.array_equal(P.slots, np.asarray(K.sum(1), np.int64)) and P.slots[2] == 0
    for i, (nx, npd, nd) in where.items():
        assert (P.x_len[i], P.slots[i], P.distinct[i]) == (nx, npd, nd)
    # float64 products in two different orders of summation lie within the bound; a wrong low-order term does not
    for Z in (X @ Y, (Y.T @ X.T).T):
        Z = R.canonical(Z)
        share = R.check_product(P, Z.indptr, Z.indices, Z.data)
        assert share <= 1.0
    bad = R.canonical(X @ Y)
    k = int(np.argmax(P.count))
    bad.data[k] += 4 * float(R.gamma(P.count[k] + 1) * P.absval[k])
    with pytest.raises(AssertionError):
        R.check_product(P, bad.indptr, bad.indices, bad.data)


def test_cancellation_case_cancels_exactly_one_entry():
    X, Y, (i, j) = R.cancellation_case()
    P = R.product(X, Y)
    hit = (P.val == 0) & (P.absval > 0)
    assert hit.sum() == 1 and (P.row[hit][0], P.col[hit][0]) == (i, j) and P.count[hit][0] == 2
    assert R.product_branch(P, X, Y.shape[1])[1] == "lists12"
    Z = X @ Y                                        # scipy drops the entry as well
    Z.sort_indices()
    assert Z.nnz == len(P.row) - 1
    R.check_product(P, Z.indptr, Z.indices, Z.data, drop_cancelled=True)
    with pytest.raises(AssertionError):
        R.check_product(P, Z.indptr, Z.indices, Z.data)


def test_chain_is_the_dense_longdouble_chain_with_composed_counts():
    X, Y, Z, _ = R.build_chain_case("lists12", True)
    X, Y, Z = X[:60], Y, Z
    P, YZ = R.chain(X, Y, Z)
    D = _dense_ld(X) @ (_dense_ld(Y) @ _dense_ld(Z))
    Dabs = np.abs(_dense_ld(X)) @ (np.abs(_dense_ld(Y)) @ np.abs(_dense_ld(Z)))
    ones = lambda M: sp.csr_matrix((np.ones(M.nnz), M.indices, M.indptr), shape=M.shape)
    K = (ones(X) @ (ones(Y) @ ones(Z))).toarray()
    got = np.zeros(D.shape, LD)
    got[P.row, P.col] = P.val
    assert np.abs(got - D).max() <= 16 * 2.0 ** -63 * Dabs.max()
    assert np.array_equal(K[P.row, P.col], P.count) and (K != 0).sum() == len(P.row)
    F = R.canonical(X @ (Y @ Z))
    assert R.check_product(P, F.indptr, F.indices, F.data, extra=2) <= 1.0


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("name", sorted(R.PRODUCT_CASES))
def test_product_cases_take_the_branch_they_are_meant_for(name, signed):
    X, Y, where, count, rows, passes = R.build_product_case(name, signed)
    P = R.product(X, Y)
    assert X.shape[0] != X.shape[1] and Y.shape[0] != Y.shape[1], "rectangular"
    assert R.product_branch(P, X, Y.shape[1]) == (count, rows)
    assert set(R.product_route(P, X, Y.shape[1]).tolist()) == passes
    for i, (nx, npd, nd) in where.items():
        assert (P.x_len[i], P.slots[i], P.distinct[i]) == (nx, npd, nd), "a planted row"
    assert (X.data > 0).all() != signed and (Y.data > 0).all() != signed
    if name == "lists12":
        assert (P.x_len == 0).sum() >= 3 and (np.diff(Y.indptr) == 0).any(), "empty rows of X and of Y"


@pytest.mark.parametrize("name", sorted(R.CHAIN_CASES))
def test_chain_cases_take_the_branch_they_are_meant_for(name):
    X, Y, Z, branch = R.build_chain_case(name, True)
    P, YZ = R.chain(X, Y, Z)
    assert R.product_branch(P, X, Z.shape[1])[1] == branch


def test_lane_pass_limits_are_the_template_parameters():
    X, Y, where, *_ = R.build_product_case("lanes16_dense", False)
    P = R.product(X, Y)
    row = {v: k for k, v in where.items()}
    assert R.lane_pass(P, row[(16, 128, 16)], 128, 32, 16)
    for beyond in ((17, 100, 16), (16, 129, 16), (16, 128, 17)):
        assert not R.lane_pass(P, row[beyond], 128, 32, 16) and R.lane_pass(P, row[beyond], 256, 128, 64)

"""tests/dist_ref.py on the host: stacking the pieces of a split operator gives the operator back, a piece that reads a slot
nobody fills is refused, and the expected exchange area of a hand-written three-rank plan is what the plan says."""
import numpy as np
import pytest
import scipy.sparse as sp

import amg_ref as R
import dist_ref as DR


def layer_cut_ranges(n_layers, per_layer, world):
    """Row ranges of the layer partition of a layered matrix whose vertex 0 (the ground) was removed."""
    cuts = [(r * n_layers) // world * per_layer for r in range(world + 1)]
    cuts = [max(c - 1, 0) for c in cuts]
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def exports_of(A, ranges, rng=None):
    """Per rank, the own unknowns a row of another rank references; shuffled when a generator is given (the order of a
    segment is the exporting rank's business)."""
    A = sp.csr_matrix(A).tocoo()
    out = []
    for a, b in ranges:
        foreign_row = (A.row < a) | (A.row >= b)
        c = A.col[foreign_row & (A.col >= a) & (A.col < b)]
        e = np.unique(c) - a
        if rng is not None:
            e = rng.permutation(e)
        out.append(e)
    return out


@pytest.fixture(scope="module")
def layered():
    return R.layered_matrix(8, 40, 30, 5)


@pytest.mark.parametrize("world", [2, 3, 4])
@pytest.mark.parametrize("shuffled", [False, True])
def test_stack_of_split_is_the_matrix(layered, world, shuffled):
    A = layered
    ranges = layer_cut_ranges(8, 1200, world)
    assert ranges[-1][1] == A.shape[0]
    exports = exports_of(A, ranges, np.random.default_rng(world) if shuffled else None)
    m = max(len(e) for e in exports)
    if world == 3:
        assert len({b - a for a, b in ranges}) > 1, "2 / 3 / 3 layers: ranks of unequal size"
    pieces = DR.split(A, ranges, exports, m)
    assert [p.shape for p in pieces] == [(b - a, b - a + world * m) for a, b in ranges]
    back = DR.stack(pieces, exports, m)
    assert np.array_equal(back.indptr, A.indptr) and np.array_equal(back.indices, A.indices) and np.array_equal(back.data, A.data)
    # padding: a segment longer than every rank's exports changes the pieces' width and nothing else
    wide = DR.split(A, ranges, exports, m + 3)
    assert (DR.stack(wide, exports, m + 3) != A).nnz == 0
    # a segment order that differs between split and stack is NOT the same operator (the map is what is being tested)
    if shuffled:
        other = [np.sort(e) for e in exports]
        assert (DR.stack(pieces, other, m) != A).nnz > 0


def test_stack_refuses_what_no_rank_exports():
    # two ranks of 2 and 3 unknowns, m = 2; rank 1 exports one value only
    exports = [np.array([1, 0]), np.array([2])]
    p0 = sp.csr_matrix(([4.0, -1.0], ([0, 1], [0, 2 + 2 + 0])), shape=(2, 2 + 4))        # reads slot (1, 0): fine
    p1 = sp.csr_matrix(([4.0, -1.0], ([0, 2], [0, 3 + 0 + 1])), shape=(3, 3 + 4))        # reads slot (0, 1): fine
    G = DR.stack([p0, p1], exports, 2)
    want = np.zeros((5, 5))
    want[0, 0], want[1, 2 + 2], want[2, 2], want[4, 0] = 4.0, -1.0, 4.0, -1.0
    assert np.array_equal(G.toarray(), want)
    bad = sp.csr_matrix(([1.0], ([0], [2 + 2 + 1])), shape=(2, 6))                        # slot (1, 1): rank 1 exports one value
    with pytest.raises(AssertionError, match="exports only 1"):
        DR.stack([bad, p1], exports, 2)
    with pytest.raises(AssertionError, match="leaves its"):
        DR.stack([p0, p1], [np.array([1, 2]), np.array([2])], 2)                         # rank 0 has no unknown 2
    with pytest.raises(AssertionError, match="columns"):
        DR.stack([p0, p1], exports, 3)
    own = sp.csr_matrix(([1.0], ([0], [2 + 0 + 0])), shape=(2, 6))                         # rank 0 reads its own segment
    with pytest.raises(AssertionError, match="own segment"):
        DR.stack([own, p1], exports, 2)


def test_duplicates_of_a_row_are_summed():
    exports = [np.array([0]), np.array([0])]
    # rank 0, row 0: own column 0 twice (as COO duplicates) and the slot of rank 1
    p0 = sp.coo_matrix(([1.0, 2.0, 5.0], ([0, 0, 0], [0, 0, 1 + 1])), shape=(1, 1 + 2)).tocsr()
    p1 = sp.csr_matrix(([3.0], ([0], [0])), shape=(1, 1 + 2))
    assert np.array_equal(DR.stack([p0, p1], exports, 1).toarray(), [[3.0, 5.0], [0.0, 3.0]])


def test_owned_block_lumps_the_dropped_couplings():
    # n = 3, one exchange slot per rank of two: row 0 loses -1 of 4 (lumped: 3), row 1 nothing, row 2 loses -8 of 10 (2 <= 3: kept)
    piece = sp.csr_matrix(np.array([[4.0, -1.0, 0.0, 0.0, -1.0],
                                    [-1.0, 5.0, -2.0, 0.0, 0.0],
                                    [0.0, -2.0, 10.0, -5.0, -3.0]]))
    blk = DR.owned_block(piece)
    assert np.array_equal(blk.toarray(), [[3.0, -1.0, 0.0], [-1.0, 5.0, -2.0], [0.0, -2.0, 10.0]])
    assert np.array_equal(np.asarray(blk.sum(axis=1)).ravel()[:2], np.asarray(piece.sum(axis=1)).ravel()[:2])


def test_blockdiag_P():
    P = DR.blockdiag_P([np.array([[1.0], [0.5]]), np.array([[0.0, 2.0]])])
    assert np.array_equal(P.toarray(), [[1.0, 0, 0], [0.5, 0, 0], [0, 0.0, 2.0]])


def test_halo_expected_on_three_ranks():
    xs = [np.array([10.0, 11.0, 12.0]), np.array([20.0, 21.0]), np.array([30.0, 31.0, 32.0, 33.0])]
    exports = [np.array([2, 0]), np.array([], dtype=np.int64), np.array([1, 3, 0])]
    area, defined = DR.halo_expected(xs, exports, 3)
    assert np.array_equal(area[defined], [12.0, 10.0, 31.0, 33.0, 30.0])
    assert np.array_equal(defined, [True, True, False, False, False, False, True, True, True])
    assert np.array_equal(area[[0, 1]], [12.0, 10.0]) and np.array_equal(area[6:9], [31.0, 33.0, 30.0])
    a32, _ = DR.halo_expected([x.astype(np.float32) for x in xs], exports, 3)
    assert a32.dtype == np.float32
    with pytest.raises(AssertionError):
        DR.halo_expected(xs, [np.array([3]), exports[1], exports[2]], 3)
    with pytest.raises(AssertionError):
        DR.halo_expected(xs, exports, 2)                                                  # rank 2 exports three values

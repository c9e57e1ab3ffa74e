"""The sparse primitives under the assembly and the multigrid setup on inputs of this file's own, against tests/sparse_ref.py:
the exclusive scan in its four host forms (padne_test_scan), the slot merge behind the public reduce / relabel with maps
that merge rows, the setup's transpose and its sparse product (padne_test_csr_op).  Every case asserts on the host, from the
shapes alone, the condition of the branch or limit it is meant for before it looks at the device.

  scan        every element of out[0 .. n] equal to the int64 prefix sums, the total, the return code, the negative flag
  merge       indptr, indices and the BITS of data equal to the sequential float64 sums in source order
  transpose   indptr, indices and the BITS of data equal; again under PADNE_FORCE=transpose_cursors
  product     the pattern equal to the symbolic one, every value within gamma(k + 1) (|X||Y|)_ij (chains: gamma(cnt + 2)
              (|X||Y||Z|)_ij): the bar is 1, the largest share of its bound an entry used on an MI355X is recorded below

Largest share of its bound an entry of the product used on an MI355X (positive / signed values), per case:
  lists12        0.506 / 0.510      lanes16_dense  0.494 / 0.498      lanes16_redo   0.494 / 0.499
  lanes32_dense  0.496 / 0.496      lanes32_redo   0.497 / 0.497      lanes64_dense  0.538 / 0.515
  lanes64_redo   0.499 / 0.498      dense          0.602 / 0.621      rows           0.507 / 0.492
  chain lists12  0.571 / 0.552      chain lanes    0.628 / 0.587      chain dense    0.626 / 0.608
(0.5 is an entry of one product whose rounding is half an ulp, against gamma(2).)

Fixed with this file: spgemm kept the symbolic pattern -- none of its row kernels looks at the sums -- so an entry whose
products cancel exactly came back as a stored 0.0 (test_product_drops_an_exact_cancellation: 1814 entries against 1813).  The
product now drops such entries when it is compacted into a matrix, as the assembly and the merges do; rows that stay in their
merge slots (the Y Z of a chain) keep their symbolic pattern, which is what the chain's reference walks.

Perturbations that were planted in a scratch build (never committed) and what they turned red, everything else staying green:
  scan_apply forgets the carry of the chunks in front (carry = 0)      every scan case beyond 32768 entries (10 tests), none
                                                                        at or below
  merge_rows_lds adds the terms of a column in reverse source order    test_merge_rows_at_the_limits_of_its_three_sorts (6)
  sort_long_rows_wave starts at 34 slots instead of 33 (a row of 33    the same six (the row of exactly 33 slots)
    slots reaches the merge unsorted)
  transpose_fill_ordered counts the waves in front one entry short     test_transpose_at_its_limits (not the cursors-only run,
                                                                        which never takes the lists)
  spgemm_row_by_masks scales every term by 1 + 2^-40 (within the old   every lists12 / lanes16 / lanes32 / lanes64 product case,
    1e-12 tolerance)                                                    every chain and split case (29); dense and rows green
  not caught: transpose_fill_ordered taking a cursor for a column of exactly 16 waves (np < kTpK) without marking it for the
  sort -- the row comes out unsorted only if the waves arrive out of order, and they did not.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sparse_ref as R
from padne_amd import _hip

pytestmark = pytest.mark.gpu

PLAIN, FLAGGED, ASYNC, HALVES = 0, 1, 2, 3
FORMS = {"plain": PLAIN, "flagged": FLAGGED, "async": ASYNC, "halves": HALVES}
TRANSPOSE, MATMUL, MATMUL_CHAIN = 0, 1, 2
OK, E_INVALID, E_TOOLARGE = _hip.OK, _hip.E_INVALID, _hip.E_TOOLARGE
_PI32, _PI64, _PF64 = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double)


# ---- the probes ----------------------------------------------------------------------------------------------------------

def scan_dev(ctx, form, counts, misalign=0, in_place=False):
    """(out int32[n + 1], return code of the form, total, negative) -- total / negative -1 where the form reports none."""
    c = np.ascontiguousarray(counts, np.int32)
    out = np.full(len(c) + 1, -7, np.int32)
    info = np.zeros(3, np.int64)
    rc = ctx._lib.padne_test_scan(ctx._h, form, len(c), c.ctypes.data_as(_PI32), misalign, int(in_place),
                                  out.ctypes.data_as(_PI32), info.ctypes.data_as(_PI64))
    assert rc == OK, (rc, ctx._lib.padne_last_error())
    return out, int(info[0]), int(info[1]), int(info[2])


def to_arrays(ctx, m):
    indptr = np.empty(m.shape[0] + 1, np.int32)
    indices = np.empty(m.nnz, np.int32)
    data = np.empty(m.nnz, np.float64)
    _hip._check(ctx._lib.padne_csr_to_host(ctx._h, m._h, indptr.ctypes.data_as(_PI32), indices.ctypes.data_as(_PI32),
                                           data.ctypes.data_as(_PF64)))
    return indptr, indices, data


def csr_op(ctx, op, X, Y=None, Z=None):
    """(indptr, indices, data, shape) of X^T, X Y or X (Y Z) as the device formed it."""
    dev = [ctx.csr_from_scipy(M) if M is not None else None for M in (X, Y, Z)]
    for M, d in zip((X, Y, Z), dev):
        assert M is None or (d.nnz == M.nnz and d.shape == M.shape)
    h = _hip._P()
    _hip._check(ctx._lib.padne_test_csr_op(ctx._h, op, *[d._h if d is not None else None for d in dev], C.byref(h)))
    out = _hip.CsrMatrix(ctx, h)
    return to_arrays(ctx, out) + (out.shape,)


def same_bits(got, want, what):
    ip, ix, d = got[:3]
    assert np.array_equal(ip, want[0]), f"{what}: row pointers"
    assert np.array_equal(ix, want[1]), f"{what}: columns"
    assert np.array_equal(d.view(np.int64), np.asarray(want[2], np.float64).view(np.int64)), f"{what}: value bits"


# ---- scan ----------------------------------------------------------------------------------------------------------------

SCAN_SIZES = [0, 1, 2, 1023, 1024, 1025, 4095, 4096, 4097, 32767, 32768, 32769, 65535, 65536, 65537,
              256 * 4096 - 1, 256 * 4096, 256 * 4096 + 1]


def scan_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return {"zeros": np.zeros(n, np.int32), "ones": np.ones(n, np.int32), "random": rng.integers(0, 13, n).astype(np.int32)}


def check_scan(ctx, counts, forms=FORMS, **kw):
    want, total, neg = R.scan(counts)
    assert total < R.INT_MAX and not neg
    for name, form in forms.items():
        out, rc, tot, flag = scan_dev(ctx, form, counts, **kw)
        assert rc == OK, name
        assert np.array_equal(out.astype(np.int64), want), f"{name}: first difference at {np.flatnonzero(out != want)[:3]}"
        assert tot == (-1 if form == ASYNC else total), name
        assert flag == {PLAIN: -1, ASYNC: -1}.get(form, 0), name


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_every_form_at_every_hand_over(ctx, n):
    """One workgroup up to 32768 and three kernels beyond; chunks of 4096; one chunk per thread of scan_block_offsets up to 256
    chunks and two beyond."""
    assert (n <= R.SCAN_SMALL) == (n in SCAN_SIZES[:11]) and (-(-n // R.SCAN_CHUNK) > 256) == (n == 256 * 4096 + 1)
    for counts in scan_inputs(n, n).values():
        check_scan(ctx, counts)


@pytest.mark.parametrize("n", [4097, 32769])
def test_scan_off_the_16_byte_boundary(ctx, n):
    """The three kernels read and write 16 bytes at a time only from a 16-byte boundary; the one-workgroup kernel never."""
    counts = scan_inputs(n, 5)["random"]
    for misalign in range(4):
        check_scan(ctx, counts, misalign=misalign)


@pytest.mark.parametrize("n", [1, 1025, 32768])
def test_scan_in_place(ctx, n):
    assert n <= R.SCAN_SMALL
    check_scan(ctx, scan_inputs(n, 6)["random"], in_place=True)
    check_scan(ctx, scan_inputs(n, 6)["random"], in_place=True, misalign=1)


def test_scan_in_place_is_refused_beyond_one_workgroup(ctx):
    c = np.ones(R.SCAN_SMALL + 1, np.int32)
    out, info = np.zeros(len(c) + 1, np.int32), np.zeros(3, np.int64)
    rc = ctx._lib.padne_test_scan(ctx._h, PLAIN, len(c), c.ctypes.data_as(_PI32), 0, 1, out.ctypes.data_as(_PI32),
                                  info.ctypes.data_as(_PI64))
    assert rc == E_INVALID


@pytest.mark.parametrize("n", [1000, 40000])
def test_scan_totals_at_the_end_of_32_bits(ctx, n):
    """2147483646 is the last total that passes; 2147483647 and the saturated counts of a product too large for 32-bit offsets
    are reported with their exact 64-bit total (the split of the sparse products reads it)."""
    assert (n <= R.SCAN_SMALL) == (n == 1000)
    rng = np.random.default_rng(n)
    c = rng.integers(0, 13, n).astype(np.int32)
    at = n // 2 + 1
    c[at] = 0
    c[at] = R.INT_MAX - 1 - int(c.astype(np.int64).sum())
    assert R.scan(c)[1] == R.INT_MAX - 1
    check_scan(ctx, c)
    c[n - 1] += 1
    big = np.full(n, 2_400_000_000 // n, np.int32)
    sat = np.zeros(n, np.int32)
    sat[[0, n // 3, n - 1]] = R.INT_MAX
    for counts in (c, big, sat):
        total = R.scan(counts)[1]
        assert total >= R.INT_MAX and (counts is not big or n != 40000 or abs(total - 2.4e9) < 1e5)
        for name, form in FORMS.items():
            out, rc, tot, flag = scan_dev(ctx, form, counts)
            if form in (PLAIN, FLAGGED):
                assert rc == E_TOOLARGE and tot == total, name
            elif form == HALVES:
                assert rc == OK and tot == total and flag == 0, name     # (the halves hand the total out; their callers judge it)
            else:
                assert rc == OK and tot == -1, name


@pytest.mark.parametrize("n", [20000, 40000])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_scan_negative_input(ctx, n, where):
    """A negative count is a message of the producer.  The plain form refuses it; the flagged form and the halves report it.
    The offsets are meaningless then (common.hpp) and nothing is promised about the total: neither is asserted."""
    assert (n <= R.SCAN_SMALL) == (n == 20000)
    c = scan_inputs(n, 9)["random"]
    at = {"first": 5, "middle": (n // 2) // R.SCAN_CHUNK * R.SCAN_CHUNK + 17, "last": n - 1}[where]
    assert at // R.SCAN_CHUNK == {"first": 0, "middle": (n // 2) // R.SCAN_CHUNK, "last": (n - 1) // R.SCAN_CHUNK}[where]
    c[at] = -1
    assert R.scan(c)[2]
    assert scan_dev(ctx, PLAIN, c)[1] == E_INVALID
    out, rc, tot, flag = scan_dev(ctx, FLAGGED, c)
    assert rc == OK and flag == 1
    out, rc, tot, flag = scan_dev(ctx, HALVES, c)
    assert rc == OK and flag != 0
    assert scan_dev(ctx, ASYNC, c)[1] == OK


def test_scan_without_the_mailbox(ctx, switches):
    """PADNE_NO_MAILBOX=1: the total comes back by a copy and a synchronisation instead of the host-coherent slot."""
    switches.set("PADNE_NO_MAILBOX", "1")
    for n in (0, 1025, 32768, 32769, 65537):
        check_scan(ctx, scan_inputs(n, 3)["random"])
    c = np.zeros(40000, np.int32)
    c[[1, 39999]] = R.INT_MAX
    for form in (PLAIN, FLAGGED):
        out, rc, tot, flag = scan_dev(ctx, form, c)
        assert rc == E_TOOLARGE and tot == 2 * R.INT_MAX
    c[7] = -1
    assert scan_dev(ctx, PLAIN, c)[1] == E_INVALID and scan_dev(ctx, FLAGGED, c)[3] == 1


# ---- slot merge through reduce and relabel -----------------------------------------------------------------------------

def check_merge(ctx, name, n_out, square):
    M, rm, cm, nr, nc, plan = R.build_merge_case(name, n_out, square=square)
    scale = 0.37
    ip, ix, d, slots, tmax = R.merge(M, rm, nr, cm, nc, scale)
    # the case is what it claims
    merged = np.bincount(rm[rm >= 0], minlength=nr)
    assert merged.max() > 1, "the map merges rows: the relabel goes through the slots"
    if name == "limits":
        assert nr == n_out and [int(slots[t]) for t in plan["slots"]] == R.MERGE_LIMIT_SLOTS == [1, 2, 32, 33, 64, 1024, 1025, 1100]
        assert (R.MERGE_LDS, R.MERGE_WAVE) == (32, 1024) and slots.max() <= 1100
        assert all(ip[t + 1] == ip[t] for t in plan["empty"]) and slots[5] == 24 and slots[14] == 40 and slots[11] == 0
        assert ip[11] > ip[10] and ip[13] > ip[12] and (rm == -1).sum() == 8
        assert 2 <= tmax[52] <= 40 and tmax.max() == 40 and (M.data == 0).sum() == 5
        assert R.compact_rows_per_wave(nr, len(ix)) == 64
    else:
        assert R.compact_rows_per_wave(nr, len(ix)) == plan["rpw"] == {"mid": 8, "wide": 1}[name] and nr <= 100000
    dev = ctx.csr_from_scipy(M)
    assert dev.nnz == M.nnz, "explicit zeros are uploaded"
    out = dev.reduce(rm, nr, scale) if square else dev.relabel(rm, nr, cm, nc, scale)
    assert out.shape == (nr, nc)
    same_bits(to_arrays(ctx, out), (ip, ix, d), f"{name} {'reduce' if square else 'relabel'}")


@pytest.mark.parametrize("n_out", [127, 128, 129])
@pytest.mark.parametrize("square", [False, True], ids=["relabel", "reduce"])
def test_merge_rows_at_the_limits_of_its_three_sorts(ctx, n_out, square):
    """Merged rows of 1, 2, 32 | 33, 64, 1024 | 1025 and 1100 slots (the LDS pass, the wave sort, the one-lane sort), columns of
    up to 40 terms, rows that cancel to nothing, explicit zeros, a dropped row between merged ones."""
    check_merge(ctx, "limits", n_out, square)


@pytest.mark.parametrize("name", ["mid", "wide"])
@pytest.mark.parametrize("square", [False, True], ids=["relabel", "reduce"])
def test_merge_rows_compacted_eight_and_one_row_per_wave(ctx, name, square):
    check_merge(ctx, name, 128, square)


# ---- transpose -------------------------------------------------------------------------------------------------------------

def small_transposes():
    out = {}
    for n in (0, 1, 63, 64, 65):
        out[f"{n}x200"] = R.random_rect(n, 200, 3.0, seed=40 + n, empty_rows_every=9)
        out[f"{n}x3"] = R.random_rect(n, 3, 1.2, seed=50 + n)
    out["wide"] = R.random_rect(300, 5000, 3.0, seed=60, empty_rows_every=11)
    out["tall_dense_waves"] = R.random_rect(2048, 90, 5.0, seed=61)
    out["scattered"] = R.scattered_band_case(4)
    return out


def check_transposes(ctx, with_2049):
    cases = small_transposes()
    for n in (0, 1, 63, 64, 65):
        assert cases[f"{n}x200"].shape == (n, 200) and cases[f"{n}x3"].shape == (n, 3)
    st = R.transpose_stats(cases["tall_dense_waves"])
    assert (st["per_wave"] > R.TP_ENTRIES).all(), "every wave beyond its table"
    st = R.transpose_stats(cases["wide"])
    assert (st["col_len"] == 0).any() and st["per_wave"].max() <= R.TP_ENTRIES and not st["sorted_cols"].any()
    st = R.transpose_stats(cases["scattered"])
    assert st["waves_per_col"].min() > R.TP_WAVES and st["per_wave"].max() <= R.TP_ENTRIES
    M = R.transpose_limits_case(3, with_2049=with_2049)
    st, P = R.transpose_stats(M), R.TP_PLANTS
    wpc, ln = st["waves_per_col"], st["col_len"]
    assert (wpc[P["waves16"]], wpc[P["waves17"]]) == (16, 17) == (R.TP_WAVES, R.TP_WAVES + 1)
    assert (ln[P["len64"]], ln[P["len65"]], ln[P["len2048"]]) == (64, 65, 2048) and ln[P["len2049"]] == (2049 if with_2049 else 0)
    assert all(st["sorted_cols"][P[k]] for k in ("len64", "len65", "len2048", "short_sorted", "long_in_chunk", "short_beside_long"))
    assert (st["per_wave"][P["full_wave"]], st["per_wave"][P["over_wave"]]) == (240, 241) and (st["per_wave"] > 240).sum() == 1
    c0 = P["long_in_chunk"] // 8 * 8
    assert (ln[c0:c0 + 8] > R.TP_SEG).sum() == 1 and c0 <= P["short_beside_long"] < c0 + 8
    assert (np.diff(M.indptr) == 0).any() and (ln == 0).any()
    cases["limits"] = M
    for name, M in cases.items():
        got = csr_op(ctx, TRANSPOSE, M)
        assert got[3] == (M.shape[1], M.shape[0])
        same_bits(got, R.transpose(M), f"transpose {name}")


def test_transpose_at_its_limits(ctx):
    """16 | 17 waves per column, 240 | 241 entries per wave, transposed rows of 64 | 65 and 2048 | 2049 entries, a chunk of eight
    with one long row, empty rows and columns, 0 .. 65 rows, a scattered numbering."""
    check_transposes(ctx, with_2049=True)


def test_transpose_through_cursors_only(ctx, switches):
    """PADNE_FORCE=transpose_cursors: every wave takes the path of the waves whose rows exceed the table -- the same bits.
    (Without the row of 2049 entries: its one-thread sort is run once, above.)"""
    switches.set("PADNE_FORCE", "transpose_cursors")
    check_transposes(ctx, with_2049=False)


# ---- product ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("signed", [False, True], ids=["positive", "signed"])
@pytest.mark.parametrize("name", sorted(R.PRODUCT_CASES))
def test_product_on_every_branch(ctx, name, signed):
    """One case per counting kernel and row kernel of spgemm, with rows planted at every template limit of the lane-group
    kernels and one beyond it, so that every hand-over forms at least one row."""
    X, Y, where, count, rows, passes = R.build_product_case(name, signed)
    P = R.product(X, Y)
    assert R.product_branch(P, X, Y.shape[1]) == (count, rows)
    assert set(R.product_route(P, X, Y.shape[1]).tolist()) == passes
    for i, (nx, npd, nd) in where.items():
        assert (P.x_len[i], P.slots[i], P.distinct[i]) == (nx, npd, nd)
    assert not signed or not ((P.val == 0) & (P.absval > 0)).any(), "no cancellation by chance: the pattern is the symbolic one"
    got = csr_op(ctx, MATMUL, X, Y)
    assert got[3] == P.shape
    share = R.check_product(P, *got[:3])
    print(f"SHARE product {name} {'signed' if signed else 'positive'} {share:.3f}")


def test_product_drops_an_exact_cancellation(ctx):
    """Row 10 of X takes two rows of Y with opposite signs; they share one column with the same value: the entry (10, 20) is
    exactly zero in any arithmetic, and must be absent."""
    X, Y, (i, j) = R.cancellation_case()
    P = R.product(X, Y)
    hit = (P.val == 0) & (P.absval > 0)
    assert hit.sum() == 1 and (P.row[hit][0], P.col[hit][0]) == (i, j)
    got = csr_op(ctx, MATMUL, X, Y)
    R.check_product(P, *got[:3], drop_cancelled=True)


def test_product_of_no_rows_one_row_and_empty_rows(ctx):
    rng = np.random.default_rng(8)
    Y = R.random_rect(30, 50, 3.0, seed=70, empty_rows_every=4)
    for X in (sp.csr_matrix((0, 30)), R.rows_to_csr([np.array([2, 3, 7, 29])], 30, rng), R.rows_to_csr([np.zeros(0)], 30, rng),
              R.rows_to_csr([np.array([3, 7]), np.zeros(0), np.array([3])], 30, rng)):
        P = R.product(X, Y)
        got = csr_op(ctx, MATMUL, X, Y)
        assert got[3] == (X.shape[0], 50)
        R.check_product(P, *got[:3])
    assert np.diff(Y.indptr)[3] == 0 and np.diff(Y.indptr)[7] == 0, "empty rows of Y are selected"


@pytest.mark.parametrize("signed", [False, True], ids=["positive", "signed"])
@pytest.mark.parametrize("name", sorted(R.CHAIN_CASES))
def test_product_chain_through_the_merge_slots(ctx, name, signed):
    """X (Y Z) with Y Z read from the slots its rows were merged in, as the setup forms R (A P)."""
    X, Y, Z, branch = R.build_chain_case(name, signed)
    P, YZ = R.chain(X, Y, Z)
    assert R.product_branch(P, X, Z.shape[1])[1] == branch
    got = csr_op(ctx, MATMUL_CHAIN, X, Y, Z)
    assert got[3] == P.shape
    share = R.check_product(P, *got[:3], extra=2)
    print(f"SHARE chain {name} {'signed' if signed else 'positive'} {share:.3f}")


@pytest.mark.parametrize("n", [2, 3, 333])
def test_product_split_in_halves(ctx, switches, n):
    """PADNE_FORCE=spgemm_split:<slots>: a product of more slots than that is formed half by half (and the halves again), the
    halves stacked: same pattern, same bound."""
    X, Y, _ = R.product_case(n=n, n_mid=200, n_cols=300, seed=80 + n, x_len=lambda r: r.integers(3, 9),
                             y_len=lambda r: r.integers(3, 9), signed=True)
    P = R.product(X, Y)
    limit = max(int(P.slots.sum()) // 5, 1)
    assert P.slots.sum() > limit and n >= 2
    switches.set("PADNE_FORCE", f"spgemm_split:{limit}")
    got = csr_op(ctx, MATMUL, X, Y)
    R.check_product(P, *got[:3])
    Z = R.random_rect(300, 120, 3.0, seed=90)
    Pc, _ = R.chain(X, Y, Z)
    R.check_product(Pc, *csr_op(ctx, MATMUL_CHAIN, X, Y, Z)[:3], extra=2)

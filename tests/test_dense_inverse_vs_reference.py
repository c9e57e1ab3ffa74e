"""The coarsest-level dense inverse of csrc/amg.hip (dense_inverse) against an inverse computed independently
(tests/dense_ref.py), column by column (needs an MI355X).

How a column is read.  A system of 33 to PADNE_AMG_COARSE_N unknowns is a hierarchy of ONE level, always in double
precision, and `amg_apply` on it is one product with the inverse (padne_amg_apply hands the cycle a place for the partial sums of
r.z, so the kernel is dense_gemv_dot; dense_gemv<double> forms the same row sums in the same order).  With r = e_j every
product of a row sum is 0 but inv[i][j] * 1.0: `amg_apply(e_j)` is column j of the device's inverse BIT FOR BIT.  Every
test asserts through amg_shapes() that the hierarchy it looks at has one level.

Inputs.  (a) leading principal blocks of reduced layered operators (synthetic.layered_system + oracle.assemble_system, as
layered_spd of test_gpu_parity.py; a principal block of an SPD matrix is SPD) at the sizes around every edge of the code:
the 16 pivots of a launch of the vector form and its separate last launch (47 .. 49), the 64 pivots of a matrix-core launch
and the size up to which the vector form runs anyway (63 .. 65), the 96 x 32 wave tiles (95 .. 97, 127 .. 129, 191 .. 193),
257, 1023 .. 1025, 2047 / 2048 (the default limit) and 4096 (the largest PADNE_AMG_COARSE_N).  (b) the coarsest Galerkin
operators of the hierarchy of a 2 x 180 x 150 board with PADNE_AMG_COARSE_N = 200, 1000 and 2048, downloaded, made exactly
symmetric ((G + G^T) / 2: the triple product is symmetric only to rounding, and the reference wants a symmetric matrix)
and uploaded as systems of their own: denser and worse conditioned than (a), and what the kernels invert in production.
(c) the operator of 257 unknowns scaled D A D, D = diag(10^u), u uniform in [-3, 3]: pivots over twelve decades.
Both forms (default: 64 pivots a launch on the matrix cores; PADNE_GJ_VECTOR=1: 16 a launch, vector FMAs) at every size
up to 257, at 1025, 2048, 4096, on (b) and (c); the default form alone at 1023, 1024 and 2047.  Every (input, form) runs in
a context of its own.

Columns.  All of them up to n = 257; above, columns 0 and n - 1, 64 k - 1, 64 k, 64 k + 1 for every k, 96 k and 32 k +- 1
for the first and last three k, and 32 drawn with a fixed seed (8 at n = 4096, whose 195 edge columns cost the host's
reference 8 s as it is).

The tolerance has no constant of its own: `lapack_error(A)` -- what scipy.linalg.inv in float64 is off by on the SAME
matrix and columns, against the same reference -- times C.  All errors are the largest over the compared columns, relative
to the largest entry of the inverse.  Measured on an MI355X (device error, and its ratio to LAPACK's):

    input   n     columns  LAPACK     cores      ratio   vector     ratio
    a33     33    33       8.13e-16   6.29e-16   0.77    6.29e-16   0.77
    a47     47    47       2.71e-16   6.16e-16   2.28    6.16e-16   2.28
    a48     48    48       3.08e-16   5.84e-16   1.90    5.84e-16   1.90
    a49     49    49       2.23e-16   6.41e-16   2.88    6.41e-16   2.88
    a63     63    63       5.91e-16   4.79e-16   0.81    4.79e-16   0.81
    a64     64    64       5.50e-16   5.56e-16   1.01    5.56e-16   1.01
    a65     65    65       5.27e-16   5.37e-16   1.02    5.37e-16   1.02
    a95     95    95       8.64e-16   4.68e-16   0.54    6.00e-16   0.69
    a96     96    96       8.39e-16   5.01e-16   0.60    6.03e-16   0.72
    a97     97    97       8.77e-16   5.07e-16   0.58    6.49e-16   0.74
    a127    127   127      4.94e-16   4.48e-16   0.91    7.61e-16   1.54
    a128    128   128      5.86e-16   4.99e-16   0.85    9.81e-16   1.67
    a129    129   129      4.94e-16   5.57e-16   1.13    9.41e-16   1.90
    a191    191   191      2.44e-16   1.02e-15   4.17    1.10e-15   4.52
    a192    192   192      2.20e-16   1.11e-15   5.05    1.11e-15   5.05
    a193    193   193      2.16e-16   1.13e-15   5.21    1.13e-15   5.21
    a257    257   257      4.59e-16   1.21e-15   2.63    1.66e-15   3.60
    a1023   1023  83       2.64e-15   3.31e-15   1.26    -          -
    a1024   1024  84       2.76e-15   3.22e-15   1.17    -          -
    a1025   1025  86       2.83e-15   3.23e-15   1.14    3.61e-15   1.28
    a2047   2047  134      1.75e-15   4.50e-15   2.57    -          -
    a2048   2048  134      1.76e-15   5.00e-15   2.84    4.02e-15   2.29
    a4096   4096  205      3.52e-15   1.60e-14   4.54    2.07e-14   5.88
    g200    85    85       5.53e-15   2.27e-14   4.10    4.68e-14   8.47
    g1000   778   74       4.52e-14   6.56e-14   1.45    7.79e-14   1.72
    g2048   778   74       4.52e-14   6.56e-14   1.45    7.79e-14   1.72
    s257    257   257      4.16e-13   6.41e-16   0.00    1.92e-15   0.00

C = 64: the smallest power of two that is at least 4 x the worst ratio (8.47, g200 / vector; 4 x for the other order of
the sums of a blocked Gauss-Jordan, whose error constant grows with n where Cholesky's does not).  Not beyond 64, so no
finding; without (b) the worst is 5.88 and C would be 32.  (LAPACK's own error moves with the machine and its threads --
a1025: 1.4e-15 on one host, 2.8e-15 on another --, and up to 257 it is a unit or two of rounding: the ratios there say
how lucky LAPACK was, not how bad the device is.)  Symmetry measured at most 2.15 x LAPACK, A Z - E at most 0.055 of
n 2^-52 max|A| max|A^-1|, the two forms at most 12.2 x LAPACK apart (g200; bound 128).
g1000 and g2048 are ONE operator: the hierarchy of that board steps from above 2048 unknowns to 778.  Both stay, as
the cases that were set.  s257: LAPACK's pivoted LU is off by 4e-13 of the largest entry there and the device by 1e-15, so
that bound says little; the test therefore also takes the error back to the units of the unscaled operator, D (Z - X) D,
and holds it to C x the yardstick of a257 (measured: 2.5 and 2.9 x).

What the accuracy bound cannot see, and what does.  With ONE Newton step behind the hardware reciprocal instead of two the
errors grow 1.4 to 8.4 x (worst ratio 24, g200 / cores) -- inside C = 64 by the rule above, every assertion of the
comparison stays green.  The reciprocal is therefore tested by itself: the inverse of a DIAGONAL matrix is, entry for
entry, what that routine returns for each pivot (every other product of the elimination has a factor 0), and the hardware
reciprocal with two Newton steps is 1 / d rounded correctly but for e^2, e <= 2^-40 the error after the first step:
test_the_reciprocal_of_a_pivot_is_correctly_rounded asks for (1/2 + 2^-30) units in the last place, in exact fractions.

Shown able to fail, in a scratch copy of the tree with a perturbed library (one change each, not committed):
  * the second Newton step removed in gj_invert_block16 and gj_pivot_rows16: the reciprocal test is red in both forms
    (9.05 units in the last place; as built 0.498, the figure of a correctly rounded division), the other 93 tests green
    as said above;
  * gj64_step reading the side buffer of the other parity: every test of the default form above 64 unknowns is red
    (comparison, agreement of the forms, power-of-two scaling, same bits, reversed rows, all three solves: 49 tests); the
    vector form and n <= 64 stay green;
  * "drop the gj_block_step<false> branch" was NOT run: with a partial last block the <true> kernel reads rows
    k0 + b >= n of the scratch matrix, up to 15 rows past its end.  In its place, inside the bounds: the <false> kernel
    pads its pivot block with zeros instead of the identity.  Red: the vector form at every size that is no multiple of
    16, both forms at 33, 47, 49 and 63 (44 tests); a48, a64, a96, a128, a192, a2048, a4096 have no partial block and stay
    green, as does the default form above 64;
  * dense_from_csr storing W[cols[k]][i] (and clearing column i): GREEN, every test -- every input here is symmetric, the
    transpose of the copy is the copy.  The suite cannot see this; the library documents the inverse for symmetric
    positive definite operators only.

Wall time on the MI355X host: the whole file (95 tests) 13 s; the slowest case a4096 / cores 5.4 s, 5.2 s of it the host's
reference for 205 columns (shared with a4096 / vector, 0.16 s); every other case at most 1.1 s.

Remaining gap (out of scope here): the single-precision copy of the inverse (coarse_inv32) and the batched
single-precision apply of the lockstep loops (dense_gemm_xk) exist only from two levels on, where the inverse cannot be
isolated without a new probe; and the cycle above the coarsest level.
"""
import functools
import math
import time
from fractions import Fraction

import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import dense_ref as D
import pcg_ref as R
from oracle import padne_oracle as O
from padne_amd import _hip, synthetic

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
C = 64.0                        # device error <= C * lapack_error


# ---- inputs ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def layered_spd(nl, nx, ny, lattice):
    sysm = synthetic.layered_system(nl, nx, ny, via_lattice=lattice)
    els = [("R", int(a), int(b), float(r)) for a, b, r in zip(*sysm.resistors)]
    els += [("I", int(f), int(t), float(i)) for f, t, i in zip(*sysm.current_sources)]
    Lo, _ = O.assemble_system([(m[0], m[1], m[2]) for m in sysm.meshes], 0, els, 0)
    n = sysm.n_vertices
    A = (-Lo[1:n, 1:n]).tocsr()
    A.sort_indices()
    return A


# size -> (layers, nx, ny) of the slightly larger board whose reduced operator is cut down to it
BOARD = {33: (1, 6, 6), 47: (1, 8, 7), 48: (1, 8, 7), 49: (1, 8, 7), 63: (1, 9, 8), 64: (1, 9, 8), 65: (1, 9, 8),
         95: (1, 11, 10), 96: (1, 11, 10), 97: (1, 11, 10), 127: (2, 9, 8), 128: (2, 9, 8), 129: (2, 9, 8),
         191: (2, 11, 10), 192: (2, 11, 10), 193: (2, 11, 10), 257: (2, 13, 11), 1023: (2, 25, 22), 1024: (2, 25, 22),
         1025: (2, 25, 22), 2047: (2, 35, 31), 2048: (2, 35, 31), 4096: (2, 50, 43)}
DEFAULT_FORM_ONLY = (1023, 1024, 2047)
GALERKIN = (200, 1000, 2048)
SCALED = 257
FORMS = ("cores", "vector")


def layered_block(n):
    A = layered_spd(*BOARD[n], 4)
    assert n <= A.shape[0] <= 1.12 * n + 8
    A = A[:n, :n].tocsr()
    A.sort_indices()
    return A


def scaling(n):
    return 10.0 ** np.random.default_rng(11).uniform(-3, 3, n)


def badly_scaled(A):
    """D A D with D = diag(10^u), u uniform in [-3, 3]; entry (i, j) is a_ij * (d_i * d_j): symmetric to the bit."""
    d = scaling(A.shape[0])
    S = sp.coo_matrix(A)
    S = sp.csr_matrix((S.data * (d[S.row] * d[S.col]), (S.row, S.col)), shape=A.shape)
    S.sort_indices()
    return S


_galerkin = {}


def galerkin_operator(switches, coarse_n):
    """The coarsest operator of the hierarchy of the 2 x 180 x 150 board under PADNE_AMG_COARSE_N = coarse_n."""
    if coarse_n not in _galerkin:
        switches.set("PADNE_AMG_COARSE_N", str(coarse_n))
        A = layered_spd(2, 180, 150, 5)
        c = _hip.Context(0)
        try:
            d = c.csr_from_scipy(A)
            d.amg_apply(np.zeros(A.shape[0]))
            shapes = d.amg_shapes()
            assert len(shapes) >= 2 and 64 < shapes[-1]["A"][0] <= coarse_n, shapes
            G = d.amg_level(len(shapes) - 1, "A")
            d.close()
        finally:
            c.close()
        switches.unset("PADNE_AMG_COARSE_N")
        G = ((G + G.T) * 0.5).tocsr()
        G.sort_indices()
        _galerkin[coarse_n] = G
    return _galerkin[coarse_n]


def matrix_of(switches, case):
    kind, n = case[0], int(case[1:])
    if kind == "a":
        return layered_block(n)
    if kind == "g":
        return galerkin_operator(switches, n)
    assert kind == "s"
    return badly_scaled(layered_block(n))


CASES = [f"a{n}" for n in BOARD] + [f"g{n}" for n in GALERKIN] + [f"s{SCALED}"]
CASE_FORMS = [(case, form) for case in CASES for form in FORMS
              if not (form == "vector" and case[0] == "a" and int(case[1:]) in DEFAULT_FORM_ONLY)]
BOTH_FORMS = [case for case in CASES if (case, "vector") in CASE_FORMS]


def compared_columns(n):
    if n <= 257:
        return np.arange(n)
    k64, k96, k32 = np.arange(n // 64 + 2), np.arange(n // 96 + 1), np.arange(n // 32 + 2)
    ends = lambda k: np.concatenate([k[:3], k[-3:]])
    cols = np.concatenate([[0, n - 1], 64 * k64 - 1, 64 * k64, 64 * k64 + 1, 96 * ends(k96), 32 * ends(k32) - 1,
                           32 * ends(k32) + 1, np.random.default_rng(64).choice(n, 32 if n < 4096 else 8, replace=False)])
    return np.unique(np.clip(cols, 0, n - 1))


# ---- the reference, once per input -----------------------------------------------------------------------------------

_reference = {}


def reference_of(switches, case):
    """A, the compared columns, those columns of the reference inverse, max |A^-1| over them and LAPACK's error."""
    if case not in _reference:
        A = matrix_of(switches, case)
        cols = compared_columns(A.shape[0])
        X = D.reference_columns(A, cols)
        _reference[case] = (A, cols, X, np.abs(X).max(), D.lapack_error(A, cols, X))
    return _reference[case]


# ---- the device's columns ----------------------------------------------------------------------------------------------

def upload_as_it_stands(c, A):
    """Through the C entry itself: csr_from_scipy would sort the rows."""
    n = A.shape[0]
    indptr, indices, data = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)
    h = _hip._P()
    _hip._check(c._lib.padne_csr_from_host(c._h, n, n, _hip._ptr(indptr, _hip._PI32), _hip._ptr(indices, _hip._PI32),
                                           _hip._ptr(data, _hip._PF64), _hip.C.byref(h)))
    return _hip.CsrMatrix(c, h)


def device_columns(switches, A, cols, form, probe=None, upload=None):
    """Columns `cols` of the inverse the device forms of A, in a context of its own (and amg_apply(probe))."""
    n = A.shape[0]
    if form == "vector":
        switches.set("PADNE_GJ_VECTOR", "1")
    else:
        switches.unset("PADNE_GJ_VECTOR")
    if n > 2048:
        switches.set("PADNE_AMG_COARSE_N", "4096")
    else:
        switches.unset("PADNE_AMG_COARSE_N")
    c = _hip.Context(0)
    try:
        d = c.csr_from_scipy(A) if upload is None else upload(c, A)
        e = np.zeros(n)
        d.amg_apply(e)
        shapes = d.amg_shapes()
        assert len(shapes) == 1 and shapes[0]["A"][:2] == (n, n), f"not the dense inverse alone: {shapes}"
        Z = np.empty((n, len(cols)))
        for q, j in enumerate(cols):
            e[j] = 1.0
            Z[:, q] = d.amg_apply(e)
            e[j] = 0.0
        z = None if probe is None else d.amg_apply(probe)
        d.close()
    finally:
        c.close()
    return Z, z


_device = {}


def probe_of(n):
    return np.random.default_rng(n).uniform(-1, 1, n)


def device_of(switches, case, form):
    if (case, form) not in _device:
        A, cols = reference_of(switches, case)[:2]
        t0 = time.perf_counter()
        _device[case, form] = device_columns(switches, A, cols, form, probe_of(A.shape[0]) if A.shape[0] <= 257 else None)
        print(f"DENSEINV {case}/{form} device columns in {time.perf_counter() - t0:.2f} s")
    return _device[case, form]


# ---- against the reference ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,form", CASE_FORMS)
def test_inverse_columns_against_the_reference(switches, case, form):
    """Accuracy, symmetry, A Z = I, and (all columns at hand) amg_apply of a random vector."""
    t0 = time.perf_counter()
    A, cols, X, xmax, lap = reference_of(switches, case)
    t1 = time.perf_counter()
    n = A.shape[0]
    Z, z = device_of(switches, case, form)
    assert np.isfinite(Z).all()
    err = D.relative_error(Z, X)
    sym = float(np.abs(Z[cols] - Z[cols].T).max() / xmax)
    ident = float(np.abs(D.product(A)(Z.astype(LD)) - D.unit_columns(n, cols)).max())
    ident_scale = n * 2.0 ** -52 * np.abs(A.data).max() * float(xmax)
    print(f"DENSEINV {case}/{form} n={n} nnz={A.nnz} columns={len(cols)} lapack={lap:.3e} device={err:.3e} "
          f"ratio={err / lap:.2f} symmetry/lapack={sym / lap:.2f} identity/(n u |A| |Z|)={ident / ident_scale:.3e} "
          f"reference {t1 - t0:.2f} s, in all {time.perf_counter() - t0:.2f} s")
    assert lap > 0.0
    assert err <= C * lap
    assert sym <= C * lap
    assert ident <= C * ident_scale
    if case[0] == "s":
        # LAPACK's pivoted inverse is a poor yardstick here (4e-13, the device 1e-15): elimination without pivoting does to
        # D A D what it does to A, every entry times d_i d_j and rounded anew, so the error taken back to the units of A,
        # D (Z - X) D, is also held to the yardstick of the unscaled operator
        d, lap0 = scaling(n), reference_of(switches, f"a{n}")[4]
        back = float(np.abs(d[:, None] * (Z.astype(LD) - X) * d[cols]).max() / np.abs(d[:, None] * X * d[cols]).max())
        print(f"DENSEINV {case}/{form} in the units of the unscaled operator: {back:.3e} = {back / lap0:.2f} lapack of a{n}")
        assert back <= C * lap0
    if z is not None:
        # linearity, and the copy of the CSR rows into the dense matrix: Z r with Z assembled from the columns
        r = probe_of(n)
        Zl = Z.astype(LD)
        assert (np.abs(z - Zl @ r) <= n * 2.0 ** -52 * (np.abs(Zl) @ np.abs(r))).all()


@pytest.mark.parametrize("case", BOTH_FORMS)
def test_the_two_forms_agree(switches, case):
    """Within twice the bound; to the bit up to 64 unknowns, where both take the vector kernels; NOT to the bit above (the
    matrix cores add in another order): the switch took effect."""
    _, _, _, xmax, lap = reference_of(switches, case)
    cores, vector = device_of(switches, case, "cores")[0], device_of(switches, case, "vector")[0]
    diff = float(np.abs(cores - vector).max() / xmax)
    print(f"DENSEINV {case} forms differ by {diff:.3e} = {diff / lap:.2f} lapack")
    assert diff <= 2.0 * C * lap
    assert np.array_equal(cores, vector) == (cores.shape[0] <= 64)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [65, 129, 1025])
def test_a_power_of_two_scales_the_inverse_exactly(switches, n, form):
    """2^40 A and 2^-40 A: every operation of the elimination, the Newton-refined reciprocal included, commutes with a
    power of two while nothing under- or overflows."""
    A, cols = reference_of(switches, f"a{n}")[:2]
    Z = device_of(switches, f"a{n}", form)[0]
    for p in (40, -40):
        S = (A * 2.0 ** p).tocsr()
        assert np.array_equal(S.data, A.data * 2.0 ** p)
        Zs = device_columns(switches, S, cols, form)[0]
        assert np.array_equal(Zs, Z * 2.0 ** -p), f"2^{p} A"


@pytest.mark.parametrize("case,form", [("a129", "cores"), ("a129", "vector"), ("a1025", "cores"), ("a1025", "vector"),
                                       ("g1000", "cores")])
def test_another_context_gives_the_same_bits(switches, case, form):
    A, cols = reference_of(switches, case)[:2]
    again = device_columns(switches, A, cols, form)[0]
    assert np.array_equal(again, device_of(switches, case, form)[0])


@pytest.mark.parametrize("form", FORMS)
def test_rows_in_any_column_order_give_the_same_bits(switches, form):
    """Every row's columns reversed: padne_csr_from_host stores the canonical matrix, the inverse is the same to the bit."""
    A, cols = reference_of(switches, "a193")[:2]
    B = A.copy()
    for i in range(B.shape[0]):
        k0, k1 = B.indptr[i], B.indptr[i + 1]
        B.indices[k0:k1] = A.indices[k0:k1][::-1]
        B.data[k0:k1] = A.data[k0:k1][::-1]
    assert (np.diff(B.indptr) > 1).all() and not np.array_equal(B.indices, A.indices)
    Z = device_columns(switches, B, cols, form, upload=upload_as_it_stands)[0]
    assert np.array_equal(Z, device_of(switches, "a193", form)[0])


@pytest.mark.parametrize("form", FORMS)
def test_the_reciprocal_of_a_pivot_is_correctly_rounded(switches, form):
    """A diagonal matrix, pivots over six decades: nothing off the diagonal, and on it 1 / d_i within (1/2 + 2^-30) units
    in the last place -- the hardware reciprocal refined by two Newton steps (module docstring); judged in exact fractions."""
    n = 257
    d = 10.0 ** np.random.default_rng(3).uniform(-3, 3, n)
    Z = device_columns(switches, sp.diags(d).tocsr(), np.arange(n), form)[0]
    assert not (Z - np.diag(np.diag(Z))).any()
    worst = Fraction(0)
    for di, zi in zip(d, np.diag(Z)):
        v = 1 / Fraction(float(di))
        ulp = Fraction(2) ** (math.frexp(float(v))[1] - 53)
        worst = max(worst, abs(Fraction(float(zi)) - v) / ulp)
    print(f"DENSEINV reciprocal/{form} worst error {float(worst):.6f} units in the last place")
    assert worst <= Fraction(1, 2) + Fraction(1, 2 ** 30)


def test_at_most_32_unknowns_are_refused(ctx):
    """padne_amg_apply: "multigrid needs a square matrix with more than 32 rows" (solve_spd keeps Jacobi there)."""
    d = ctx.csr_from_scipy(layered_block(33)[:32, :32])
    with pytest.raises(ValueError, match="more than 32 rows"):
        d.amg_apply(np.ones(32))
    assert d.solve_spd(np.ones(32), precond="amg").levels == 0


def test_beyond_the_limit_there_is_a_hierarchy(switches):
    """One unknown more than PADNE_AMG_COARSE_N: levels above a smaller dense inverse, not a larger inverse."""
    switches.set("PADNE_AMG_COARSE_N", "96")
    A = layered_block(97)
    c = _hip.Context(0)
    try:
        d = c.csr_from_scipy(A)
        d.amg_apply(np.ones(97))
        shapes = d.amg_shapes()
        assert len(shapes) >= 2 and shapes[0]["A"][0] == 97 and shapes[-1]["A"][0] <= 96, shapes
        d.close()
    finally:
        c.close()


# ---- inside the CG loop: dense_gemv_dot -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 1025, 2048])
def test_first_iterate_of_the_preconditioned_solve(ctx, n):
    """x_1 of solve_spd against textbook PCG (tests/pcg_ref.py) preconditioned by the reference inverse, held to the rule
    of test_pcg_vs_reference.py: 100 * max(d_host, 2^-53), d_host the distance of the float64 run from the longdouble
    one -- the float64 run with a float64 inverse (LAPACK's Cholesky solve), as the device's run has one.  And the loop is
    over after two steps at the most."""
    A = layered_block(n)
    b = np.random.default_rng(5).uniform(-1, 1, n)
    solve = D.refined_solver(A)
    factor = sla.cho_factor(D.dense(A), lower=True)
    ld = R.pcg(A, b, 1, M=lambda r: solve(r[:, None])[:, 0])
    f64 = R.pcg(A, b, 1, dtype=np.float64, M=lambda r: sla.cho_solve(factor, r))
    d_host = R.deviation(f64.x[1], ld.x[1])
    d = ctx.csr_from_scipy(A)
    first = d.solve_spd(b, precond="amg", rtol=1e-30, max_iter=1, raise_on_fail=False)
    assert first.status == _hip.E_NOTCONVERGED and first.iterations == 1 and first.levels == 1
    assert first.restarts == 0 and first.precond_fallbacks == 0
    dev, bound = R.deviation(first.x, ld.x[1]), 100.0 * max(d_host, U)
    print(f"DENSEINV solve n={n} device={dev:.3e} d_host={d_host:.3e} bound={bound:.3e}")
    assert dev <= bound
    res = d.solve_spd(b, precond="amg", rtol=1e-12)
    print(f"DENSEINV solve n={n} iterations={res.iterations} rel_residual={res.rel_residual:.3e}")
    assert res.status == _hip.OK and res.levels == 1 and res.iterations <= 2 and res.rel_residual <= 1.1e-12
    d.close()

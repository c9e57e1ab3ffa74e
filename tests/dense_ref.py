"""Columns of the inverse of a symmetric positive definite matrix to well below double precision, in plain numpy: the
independent statement the coarsest-level inverse of csrc/amg.hip (dense_inverse) is compared with.

    X_0 = chol(A)^-1 E  in float64 (scipy),      X <- X + chol(A)^-1 (E - A X)

Nothing of the device code is restated here: no Gauss-Jordan, no blocks of 16 or 64 pivots, no elimination order at all --
a Cholesky factor of the whole matrix and iterative refinement, which contracts the error by about cond(A) 2^-53 a round.

The residual.  Formed in np.longdouble, E - A X stops at the rounding of its own sums, 2^-64 |A| |X| a row: corrections of
cond(A) 2^-64 that never fall below the 2^-58 asked for here (measured on the layered operators of the tests: 3.5e-18 ..
6e-18 at n = 257, 2e-17 at n = 2048, round after round) -- and an X kept in one longdouble leaves a residual of that size
by its own rounding.  So X is kept as an unevaluated sum of two longdoubles and the residual is formed EXACTLY, in
Python's integers (every float is an integer times a power of two; object arrays of int, the rows summed by
np.add.reduceat), and rounded once.  The corrections then fall as the theory says (4e-14, then 2e-27, at n = 2048), the
head of the pair is the inverse rounded to longdouble, and that is what is returned.
"""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

LD = np.longdouble
LONGDOUBLE_EPS = float(np.finfo(LD).eps)
if not LONGDOUBLE_EPS < 2e-19:
    pytest.skip(f"np.longdouble has no 64-bit significand here (eps = {LONGDOUBLE_EPS:.3g}): no high-precision reference",
                allow_module_level=True)

STOP = 2.0 ** -58               # a round's correction, relative to the column's largest entry, that ends the refinement
MAX_ROUNDS = 10


def dense(A):
    """float64 ndarray of a scipy sparse matrix or of anything array-like."""
    return np.asarray(A.toarray() if sp.issparse(A) else A, dtype=np.float64)


def product(A, dtype=LD):
    """X -> A X in `dtype` for X of shape (n, k).  Only the nonzero entries of A are multiplied (an exact zero adds nothing
    to a sum, so this is the dense product without its idle work); the rows are summed by np.add.reduceat."""
    S = sp.csr_matrix(A)
    S.sort_indices()
    assert S.shape[0] == S.shape[1] and (np.diff(S.indptr) > 0).all(), "square, an entry in every row (SPD: the diagonal)"
    data, idx, ptr = S.data.astype(dtype)[:, None], S.indices, S.indptr[:-1]
    return lambda X: np.add.reduceat(data * X[idx], ptr, axis=0)


def unit_columns(n, cols, dtype=LD):
    E = np.zeros((n, len(cols)), dtype)
    E[cols, np.arange(len(cols))] = 1
    return E


def as_integers(X):
    """(I, e): an object array of Python integers and an exponent with X == I * 2^e exactly, entry for entry."""
    m, ex = np.frexp(np.asarray(X, dtype=LD))
    M = np.ldexp(m, 64)                                    # the whole significand, |M| < 2^64: two halves that fit int64
    hi = np.trunc(M / 2.0 ** 32)
    lo = M - hi * 2.0 ** 32
    I = hi.astype(np.int64).astype(object) * (1 << 32) + lo.astype(np.int64).astype(object)
    ex = ex.astype(np.int64) - 64
    nz = M != 0
    e = int(ex[nz].min()) if nz.any() else 0
    return I * (2 ** np.where(nz, ex - e, 0).astype(object)), e


def exact_residual(A, B):
    """(Xh, Xl) -> B - A (Xh + Xl), every product and sum exact, the result rounded once to float64."""
    S = sp.csr_matrix(A)
    S.sort_indices()
    idx, ptr = S.indices, S.indptr[:-1]
    a_int, ea = as_integers(S.data)
    a_int = a_int[:, None]
    b_int, eb = as_integers(B)

    def residual(Xh, Xl):
        (h, eh), (l, el) = as_integers(Xh), as_integers(Xl)
        ex = min(eh, el)
        x = h * 2 ** (eh - ex) + l * 2 ** (el - ex)
        e = min(eb, ea + ex)                               # B, and A X, as integers times 2^e
        r = b_int * 2 ** (eb - e) - np.add.reduceat(a_int * x[idx], ptr, axis=0) * 2 ** (ea + ex - e)
        one = 2 ** abs(e)
        return (r / one if e <= 0 else r * one).astype(np.float64)      # (int / int: Python rounds the quotient correctly)
    return residual


def refined_solver(A):
    """B -> A^-1 B for B of shape (n, k), as np.longdouble; the Cholesky factor of A is formed once.

    The solver raises ArithmeticError when the corrections have not fallen below STOP of the column's largest entry after
    MAX_ROUNDS rounds: such a matrix is too ill-conditioned to serve as a test input.  `info`, a dict, receives the number of
    rounds and the relative size of every round's correction."""
    Ad = dense(A)
    n = Ad.shape[0]
    assert Ad.shape == (n, n) and np.array_equal(Ad, Ad.T), "a symmetric matrix"
    factor = sla.cho_factor(Ad, lower=True)              # (raises LinAlgError for a matrix that is not positive definite)

    def solve(B, info=None):
        B = np.asarray(B, dtype=LD)
        assert B.ndim == 2 and B.shape[0] == n and np.abs(B).max(axis=0).min() > 0, "columns, none of them zero"
        residual = exact_residual(A, B)
        Xh = sla.cho_solve(factor, np.float64(B)).astype(LD)
        Xl = np.zeros_like(Xh)
        history = []
        for _ in range(MAX_ROUNDS):
            d = sla.cho_solve(factor, residual(Xh, Xl))
            Xl = Xl + d
            s = Xh + Xl                                    # (the pair renormalised: |Xl| <= half a unit of Xh's last place)
            Xl = Xl - (s - Xh)
            Xh = s
            history.append(float((np.abs(d).max(axis=0) / np.abs(Xh).max(axis=0)).max()))
            if history[-1] <= STOP:
                if info is not None:
                    info.update(rounds=len(history), corrections=history)
                return Xh
        raise ArithmeticError(f"refinement with a {n} x {n} matrix has not converged after {MAX_ROUNDS} rounds "
                              f"(corrections {history}): too ill-conditioned for a test input")
    return solve


def reference_columns(A, cols=None, *, info=None):
    """Columns `cols` (all of them by default) of A^-1 as an (n, len(cols)) array of np.longdouble (refined_solver on
    columns of the identity, and its ArithmeticError)."""
    n = A.shape[0]
    cols = np.arange(n) if cols is None else np.asarray(cols, dtype=np.int64)
    return refined_solver(A)(unit_columns(n, cols), info)


def relative_error(Z, ref):
    """max |Z - ref| / max |ref| in the reference's type."""
    return float(np.abs(np.asarray(Z).astype(LD) - ref).max() / np.abs(ref).max())


def lapack_error(A, cols=None, ref=None):
    """Entry-wise error of scipy.linalg.inv(A) in plain float64 over the columns `cols`, relative to the largest entry of
    those columns of the inverse: what a well-regarded double-precision inverse of this very matrix is off by -- the
    yardstick of the tolerance the device's inverse is held to.  `ref`: reference_columns(A, cols), if already at hand."""
    Ad = dense(A)
    cols = np.arange(Ad.shape[0]) if cols is None else np.asarray(cols, dtype=np.int64)
    ref = reference_columns(A, cols) if ref is None else ref
    return relative_error(sla.inv(Ad)[:, cols], ref)

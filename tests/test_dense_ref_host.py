"""tests/dense_ref.py against what an inverse is (no GPU): A X = I and X = X^T far below double precision, and the error of
LAPACK's float64 inverse -- the yardstick of test_dense_inverse_vs_reference.py -- where theory puts it.

Scales.  A row of A X - E is a sum whose terms are as large as (|A| |X|)_ij, and the check forms it in np.longdouble: the
residual is asked to be within 2^-60 of the largest entry of |A| |X| (the reference, correctly rounded to longdouble,
leaves 2^-64 of a term per term; rows of 7 to 40 terms).  Symmetry is asked to 2^-60 of the largest entry of X.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import dense_ref as D
from oracle import padne_oracle as O
from padne_amd import synthetic

LD = np.longdouble
TIGHT = 2.0 ** -60


def hilbert_like(n=40):
    """1 / (i + j + 1) + I / 64: dense, every entry positive, and -- unlike the Hilbert matrix itself, whose condition number
    at n = 40 no float64 can hold -- conditioned like 130."""
    i = np.arange(n)
    return 1.0 / (i[:, None] + i[None, :] + 1.0) + np.eye(n) / 64.0


def layered_operator(n=200):
    """The leading n x n block of the reduced operator of a two-layer board (10 x 11 vertices a layer)."""
    sysm = synthetic.layered_system(2, 10, 11, via_lattice=4)
    els = [("R", int(a), int(b), float(r)) for a, b, r in zip(*sysm.resistors)]
    els += [("I", int(f), int(t), float(i)) for f, t, i in zip(*sysm.current_sources)]
    Lo, _ = O.assemble_system([(m[0], m[1], m[2]) for m in sysm.meshes], 0, els, 0)
    A = (-Lo[1:n + 1, 1:n + 1]).tocsr()
    A.sort_indices()
    assert A.shape == (n, n)
    return A


MATRICES = {"hilbert_like_40": hilbert_like, "layered_200": layered_operator}


@pytest.fixture(scope="module", params=list(MATRICES))
def inverse(request):
    A = MATRICES[request.param]()
    info = {}
    X = D.reference_columns(A, info=info)
    print(f"DENSEREF {request.param} corrections {info['corrections']}")
    return A, X


def test_times_the_matrix_it_is_the_identity(inverse):
    A, X = inverse
    n = A.shape[0]
    assert X.dtype == LD and X.shape == (n, n)
    residual = np.abs(D.product(A)(X) - D.unit_columns(n, np.arange(n))).max()
    scale = D.product(abs(sp.csr_matrix(A)))(np.abs(X)).max()
    print(f"DENSEREF residual {float(residual / scale):.3e} of the largest term")
    assert residual <= TIGHT * scale


def test_it_is_symmetric(inverse):
    _, X = inverse
    assert np.abs(X - X.T).max() <= TIGHT * np.abs(X).max()


def test_chosen_columns_are_those_of_the_whole(inverse):
    A, X = inverse
    cols = np.array([0, 7, A.shape[0] - 1])
    assert np.abs(D.reference_columns(A, cols) - X[:, cols]).max() <= TIGHT * np.abs(X).max()


def test_the_solver_takes_any_right_hand_side(inverse):
    A, X = inverse
    B = np.random.default_rng(4).uniform(-1, 1, (A.shape[0], 2))
    got = D.refined_solver(A)(B)
    assert np.abs(got - X @ B.astype(LD)).max() <= A.shape[0] * TIGHT * np.abs(X).max()


def test_lapack_error_is_rounding_times_conditioning(inverse):
    """Nonzero (the reference is not LAPACK's float64 inverse over again) and below cond(A) n 2^-52."""
    A, X = inverse
    n = A.shape[0]
    err = D.lapack_error(A)
    assert err == D.lapack_error(A, ref=X)
    bound = np.linalg.cond(D.dense(A)) * n * 2.0 ** -52
    print(f"DENSEREF lapack_error {err:.3e} bound {bound:.3e}")
    assert 0.0 < err <= bound


def test_a_matrix_too_ill_conditioned_is_refused():
    """The Hilbert matrix itself at n = 12 (cond 1.7e16): Cholesky breaks down or the refinement does not converge."""
    i = np.arange(12)
    H = 1.0 / (i[:, None] + i[None, :] + 1.0)
    with pytest.raises((ArithmeticError, np.linalg.LinAlgError)):
        D.reference_columns(H)

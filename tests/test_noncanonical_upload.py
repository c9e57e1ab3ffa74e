"""Matrices uploaded with unsorted rows and repeated columns are held to the matrix their entries sum to (needs an MI355X).

padne_csr_from_host takes raw CSR arrays: "the columns of a row need not ascend", and a row may name a column twice.  Every
entry of include/padne_hip.h that takes such a handle must answer as for the canonical form of that matrix, or refuse.  The
inputs are tests/noncanonical_ref.py's (held to their conditions, on the host, by tests/test_noncanonical_ref_host.py):
values rounded to float32 and split into v/2, v/2 or v/2, v/4, v/4, so that the canonical matrix is one definite matrix bit
for bit in every order of summation; every row permuted.  Every test compares with a host reference of the CANONICAL matrix,
never with another device path, and every bound is the one the entry's existing test already grants:

  shape / to_host    the canonical indptr, indices and data bit for bit, rows strictly ascending (what the header documents)
  products           padne_spmv, padne_spmv_dev, padne_spmm8_dev, padne_residual_norm against the longdouble product: the
                     per-row bound of tests/test_products_vs_reference.py, (m_i + c) u sum |a_ik x_k|, m_i the CANONICAL row
                     length (the residual norm: the 2-norm of the RESID bounds plus gamma(n + 8) of the norm for its own sum)
  reduce / relabel   drop-only, injective and merging maps under the default, PADNE_FORCE=relabel_slots and relabel_lanes,
  / vstack           against sparse_ref.merge of the canonical matrix: bit for bit, rows strictly ascending
  dense inverse      the 160-unknown system: C x LAPACK's own error, symmetry, A Z = I as test_dense_inverse_vs_reference.py
  hierarchy, cycle   case a of tests/test_amg_vs_reference.py through that file's check_hierarchy / reference_cycle, the
                     canonical matrix as A_0: its envelopes and F32_FACTOR
  solves             Jacobi, multigrid, the small system, an (N, 3) block through solve_system: REL_TOL = 1e-8 against the
                     longdouble direct solution, residual < 1e-9, status; three Jacobi iterates under the calibrated bound of
                     tests/test_pcg_vs_reference.py
  KKT plan           the voltage_source fixture, L uploaded raw, through the stage checker of test_kkt_plan_vs_reference.py
  mesh entries       padne_thermal_create*, padne_coupled_create, padne_csr_power_density answer a raw upload as they answer
                     a canonical one (no uploaded matrix carries a mesh: refusals, the context usable afterwards);
                     padne_transient_* take a thermal handle only, which no uploaded matrix can give them: not reachable
  guarded allocator  the three small systems through every family above once, under three_ways of tests/test_device_memory.py

What the parent commit did (the library as it was before padne_csr_from_host stored the canonical form; that upload kept the
raw arrays and a flag `cols_unsorted`), test by test, measured on an MI355X with this file:

  shape / to_host [rect, small, mid, large]   RED  the raw arrays came back: 3795 / 1261 / 19581 / 1201346 entries for 3352 /
                                               1046 / 16309 / 1005728, rows not ascending (documented nowhere)
  canonical upload, cancelled parts           RED  "cancelled parts": the two parts of a column were both stored
  malformed upload                            RED  only in its last line, the raw arrays again; the refusals were right
  products [rect, mid, large]                 green: a product sums a row's parts wherever they stand (every kernel form)
  reduce / relabel, drop-only and injective   RED under the default and relabel_lanes, all three systems ("row pointers"): the
                                               flag sent the matrix past the order-preserving copy, and the direct relabel
                                               of injective maps that took it instead sorts a row but never adds repeated
                                               columns -- the output named a column twice.  Green under relabel_slots
  reduce / relabel, merging                   green (the slot path sorts and adds)
  vstack [12 cases]                           RED  the stack kept the raw rows (7147 entries for 6704, 35890 for 32618) and
                                               lost the flag: see csr_vstack in the issue
  dense inverse [cores, vector]               RED  error 6.47 of max |A^-1| (bound 64 x 1.1e-15): dense_from_csr stored the last
                                               part of a repeated column, the inverse was that of another matrix
  hierarchy and cycle                         RED  level 0 of the hierarchy was the raw matrix (19581 entries); not looked at
                                               further, the level checks read A_0 as a canonical matrix
  raw preconditioner block                    RED  the same
  solves [mid amg]                            RED  converged to the right solution in 148 iterations where 40 are allowed
                                               (21 with the fixed library): the preconditioner of another matrix
  solves [small amg]                          RED  precond_fallbacks == 1: the loop gave its preconditioner up (status OK, the
                                               solution right)
  solves [mid jacobi, small jacobi]           green; Jacobi iterates 1 - 3 green (csr_dinv_kernel sums a repeated diagonal)
  block through solve_system                  not reached: the host reference's own convergence bar was set too tight in the
                                               first version of this test (2.7e-15 against 1e-15; since 1e-12, see
                                               direct_solution) -- a mistake of the test, no finding
  KKT plan                                    RED  "indices not sorted inside a row": the reduced matrix kept unsorted rows
  mesh entries                                green: refusals before and after, the same words
  guarded allocator [2]                       green: the three runs agree with each other whatever they compute
No run faulted or hung.

Deviation of the fixed library beside the bound it was held to (MI355X; every run prints these lines, pytest -s):

  products, largest share of the per-row bound (1 is the bar)
                    spmv = spmv_dev           spmm8     residual_norm (of its looser bound)
      rect          0.363                     0.475     0.001
      mid           0.381                     0.407     0.001
      large         0.473                     0.499     0.000
    (constant and unit vectors: 0.000 -- sums of a few float32 values are exact in float64)
  shape / to_host, reduce, relabel, vstack    bit for bit (no deviation to report)
  dense inverse     cores 8.55e-15 = 7.52 x LAPACK's 1.14e-15 (bound 64 x), symmetry 0.41 x, A Z - I 9.9e-3 of n u |A| |Z| (bound 64)
                    vector 8.84e-15 = 7.78 x, symmetry 0.59 x, 9.7e-3
  hierarchy         2399 > 344 > 38; P at most 0.10, A_c at most 0.53 of their envelopes; undecided strength entries 0; stability
                    1.160; f64 cycle 9.7e-5 of its envelope; f32 cycle 4.13 x, batched 3.80 x the plain float32 error (bound 8)
  solves            deviation from the longdouble solution (bound 1e-8) / residual (bound 1e-9) / iterations
      mid jacobi    2.6e-13 / 2.5e-11 / 302        mid amg      1.3e-13 / 2.2e-11 / 21 (three levels)
      small jacobi  9.9e-14 / 5.2e-12 / 68         small amg    7.3e-15 / 1.5e-13 / 1 (the dense inverse)
      Jacobi iterates 1, 2, 3: 1.4e-16, 2.0e-16, 2.7e-16 (bounds 1.4e-14, 2.5e-14, 2.5e-14)
      solve_system block: potentials at most 1.0e-14 (1e-8), multipliers 6.6e-15 (1e-9), residuals 4.5e-14 (1e-9)
  KKT plan          largest share of a stage's bound: probes 0.218, norm 0.011, solve 1.1e-5; matrix, b, constraint exact
  guarded allocator 89 and 94 compared arrays, 150 and 239 guarded blocks, no violation
The whole file: 62 tests in 8 s on the MI355X host, the slowest 3.2 s (the first use of the 144 k system: its host scramble).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import dense_ref as D
import helpers as H
import noncanonical_ref as N
import sparse_ref as R
from padne_amd import _hip, reduction, solver, synthetic
from test_amg_vs_reference import CASES as AMG_CASES, F32_FACTOR, check_hierarchy, norm2, reference_cycle, right_hand_sides
from test_dense_inverse_vs_reference import C as DENSE_C, device_columns
from test_device_memory import three_ways
from test_kkt_plan_vs_reference import System as KktSystem, check_matrix, list_plan, run as kkt_run
from test_pcg_vs_reference import calibrated, capped, check_iterate
from test_products_vs_reference import BOUND_C, PLAIN, RESID, bound_ok, exact_rows
from test_sparse_primitives_vs_reference import same_bits, to_arrays

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
REL_TOL = 1e-8
FORCES = [None, "relabel_slots", "relabel_lanes"]


def upload(ctx, name):
    A, raw = N.raw_of(name)
    return A, N.upload_raw(ctx, *raw, A.shape)


def strictly_ascending(indptr, indices):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    return not ((rows[1:] == rows[:-1]) & (indices[1:] <= indices[:-1])).any()


def held_canonical(ctx, m, A, what):
    got = to_arrays(ctx, m)
    assert m.shape == A.shape and m.nnz == A.nnz, f"{what}: {m.shape}, {m.nnz} entries against {A.shape}, {A.nnz}"
    same_bits(got, (A.indptr, A.indices, A.data), what)
    assert strictly_ascending(got[0], got[1]), what


# ---- shape / to_host -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(N.SYSTEMS))
def test_shape_and_to_host_report_the_canonical_matrix(ctx, name):
    A, d = upload(ctx, name)
    raw_nnz = int(N.raw_of(name)[1][0][-1])
    assert raw_nnz > A.nnz
    held_canonical(ctx, d, A, f"to_host of {name}")
    assert d.to_scipy().has_canonical_format
    d.close()


def test_a_canonical_upload_keeps_its_arrays_and_explicit_zeros(ctx):
    """A canonical matrix goes up as it stands, a stored 0.0 included; a raw one keeps a sum that comes to 0.0 as an entry."""
    A = N.raw_of("rect")[0].copy()
    A.data[::7] = 0.0
    d = N.upload_raw(ctx, A.indptr, A.indices, A.data, A.shape)
    assert d.nnz == A.nnz
    same_bits(to_arrays(ctx, d), (A.indptr, A.indices, A.data), "canonical upload")
    d.close()
    indptr = np.array([0, 3, 3, 5], np.int32)
    indices = np.array([2, 0, 2, 1, 1], np.int32)
    data = np.array([1.5, 2.0, -1.5, 0.25, 0.5])
    d = N.upload_raw(ctx, indptr, indices, data, (3, 3))
    same_bits(to_arrays(ctx, d), (np.array([0, 2, 2, 3]), np.array([0, 2, 1]), np.array([2.0, 0.0, 0.75])), "cancelled parts")
    assert np.array_equal(d.matvec(np.array([1.0, 2.0, 4.0])), [2.0, 0.0, 1.5])
    d.close()


def test_a_malformed_upload_is_refused_and_the_context_goes_on(ctx):
    A, raw = N.raw_of("rect")
    indptr, indices, data = raw
    bad = indices.copy()
    bad[len(bad) // 2] = A.shape[1]
    with pytest.raises(ValueError, match="column index out of range"):
        N.upload_raw(ctx, indptr, bad, data, A.shape)
    bad[len(bad) // 2] = -1
    with pytest.raises(ValueError, match="column index out of range"):
        N.upload_raw(ctx, indptr, bad, data, A.shape)
    d = N.upload_raw(ctx, indptr, indices, data, A.shape)
    held_canonical(ctx, d, A, "the upload after a refusal")
    d.close()


# ---- products --------------------------------------------------------------------------------------------------------------

def product_vectors(A, hub_col):
    rng = np.random.default_rng(A.shape[1])
    e = np.zeros(A.shape[1])
    e[hub_col] = 1.0
    X = rng.uniform(-1, 1, (A.shape[1], 8))
    X[:, 1] = 1.0
    X[:, 2] = e
    return X


def share(got, ref, lim):
    """The largest error in units of its bound (a row with bound 0 must be exact)."""
    err = np.abs(got.astype(LD) - ref)
    assert (err[lim == 0] == 0).all()
    return float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0


@pytest.mark.parametrize("name,hub_col", [("rect", N.RECT_HUB_COL), ("mid", 1200), ("large", N.LARGE_HUB)])
def test_products_against_the_longdouble_product_of_the_canonical_matrix(ctx, name, hub_col):
    A, d = upload(ctx, name)
    n, nc = A.shape
    m = np.diff(A.indptr)
    X = product_vectors(A, hub_col)
    refs = [exact_rows(A, A.data, X[:, j], LD) for j in range(8)]
    worst = {}
    for j, label in ((0, "random"), (1, "constant"), (2, "unit")):
        ref, E = refs[j]
        x = np.ascontiguousarray(X[:, j])
        y = d.matvec(x)
        xd, yd = ctx.to_device(x), ctx.empty(n)
        d.matvec_dev(xd, yd)
        y_dev = yd.numpy()
        xd.free(), yd.free()
        for entry, got in (("spmv", y), ("spmv_dev", y_dev)):
            worst[f"{entry}/{label}"] = share(got, ref, (m + BOUND_C[PLAIN]) * U * E)
            bound_ok(got, ref, E, m, BOUND_C[PLAIN], U)
        # ||b - A x||: every row within the RESID bound, the norm of n such rows within gamma(n + 8) of itself
        b = np.random.default_rng(j).uniform(-1, 1, n)
        r_ref = b.astype(LD) - ref
        lim = (m + BOUND_C[RESID]) * U * (E + np.abs(b))
        want = float(norm2(r_ref))
        slack = float(norm2(lim)) + float(R.gamma(n + 8)) * want
        got = d.residual_norm(x, b)
        worst[f"residual_norm/{label}"] = abs(got - want) / slack
        assert abs(got - want) <= slack, (label, got, want, slack)
    Y = d.matmat8(X)
    for j in range(8):
        ref, E = refs[j]
        worst["spmm8"] = max(worst.get("spmm8", 0.0), share(Y[:, j], ref, (m + BOUND_C[PLAIN]) * U * E))
        bound_ok(Y[:, j], ref, E, m, BOUND_C[PLAIN], U)
    print(f"NONCANON products {name}: share of the bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    d.close()


# ---- reduce, relabel, vstack -------------------------------------------------------------------------------------------------

def drop_only(n, seed, always=()):
    rng = np.random.default_rng(seed)
    m = np.arange(n, dtype=np.int32)
    drop = np.unique(np.r_[0, n - 1, rng.choice(n, max(2, n // 35), replace=False), np.asarray(always, np.int64)])
    m[drop] = -1
    keep = m >= 0
    m[keep] = np.arange(int(keep.sum()), dtype=np.int32)
    return m, int(keep.sum())


def injective(n, seed):
    rng = np.random.default_rng(seed)
    m = rng.permutation(n).astype(np.int32)
    m[rng.choice(n, max(2, n // 20), replace=False)] = -1
    keep = m >= 0
    m[keep] = np.argsort(np.argsort(m[keep])).astype(np.int32)
    return m, int(keep.sum())


def merging(n, seed):
    n_out = max(2, n // 3)
    return np.random.default_rng(seed).integers(-1, n_out, n).astype(np.int32), n_out


MAPS = {"drop": drop_only, "injective": injective, "merging": merging}


@functools.lru_cache(maxsize=None)
def relabel_reference(name, kind, square):
    """(row map, rows out, column map, columns out, scale, sparse_ref.merge of the CANONICAL matrix), once per case."""
    A = N.raw_of(name)[0]
    rm, nr = MAPS[kind](A.shape[0], 11)
    cm, nc = (rm, nr) if square else MAPS[kind](A.shape[1], 12)
    scale = -2.0
    return rm, nr, cm, nc, scale, R.merge(A, rm, nr, cm, nc, scale)[:3]


@pytest.mark.parametrize("force", FORCES, ids=["default", "slots", "lanes"])
@pytest.mark.parametrize("kind", list(MAPS))
@pytest.mark.parametrize("name", ["rect", "mid", "large"])
def test_reduce_and_relabel_of_a_raw_upload(ctx, switches, name, kind, force):
    A, d = upload(ctx, name)
    if force is not None:
        switches.set("PADNE_FORCE", force)
    for square in ((False, True) if A.shape[0] == A.shape[1] else (False,)):
        rm, nr, cm, nc, scale, want = relabel_reference(name, kind, square)
        if kind == "merging":
            assert np.bincount(rm[rm >= 0], minlength=nr).max() > 1
        else:
            assert np.bincount(rm[rm >= 0], minlength=nr).max() == 1 and (rm == -1).any()
        out = d.reduce(rm, nr, scale) if square else d.relabel(rm, nr, cm, nc, scale)
        assert out.shape == (nr, nc)
        got = to_arrays(ctx, out)
        same_bits(got, want, f"{name} {kind} {'reduce' if square else 'relabel'} under {force}")
        assert strictly_ascending(got[0], got[1]) and len(got[1]) > 0
        out.close()
    d.close()


@functools.lru_cache(maxsize=None)
def vstack_reference(name):
    A = N.raw_of(name)[0]
    S = sp.vstack([A, A]).tocsr()
    S.sort_indices()
    hub = {"rect": N.RECT_HUB_ROW}.get(name, 5)
    rm, nr = drop_only(S.shape[0], 21, always=[hub, A.shape[0] + hub + 1])
    cm, nc = drop_only(S.shape[1], 22)
    return S, rm, nr, cm, nc, R.merge(S, rm, nr, cm, nc, -1.0)[:3]


@pytest.mark.parametrize("force", FORCES, ids=["default", "slots", "lanes"])
@pytest.mark.parametrize("raw_on", ["top", "bottom"])
@pytest.mark.parametrize("name", ["rect", "mid"])
def test_vstack_with_a_raw_upload_then_a_drop_only_relabel(ctx, switches, name, raw_on, force):
    """The stack of a raw and a canonical upload is the stack of the canonical matrices, and so is what a map that only drops
    indices -- the order-preserving copy -- makes of it (the stack is 2n x n: relabel; a square one is reduced below)."""
    A, raw = upload(ctx, name)
    canon = ctx.csr_from_scipy(A)
    S, rm, nr, cm, nc, want = vstack_reference(name)
    if force is not None:
        switches.set("PADNE_FORCE", force)
    st = raw.vstack(canon) if raw_on == "top" else canon.vstack(raw)
    held_canonical(ctx, st, S, f"vstack, raw {raw_on}")
    out = st.relabel(rm, nr, cm, nc, -1.0)
    got = to_arrays(ctx, out)
    same_bits(got, want, f"relabel of the stack, raw {raw_on}, under {force}")
    assert strictly_ascending(got[0], got[1])
    if name == "mid":
        # a square matrix out of the stack (the first n rows of it again, by a drop-only relabel), then the reduce itself
        n = A.shape[0]
        top = np.r_[np.arange(n), np.full(n, -1)].astype(np.int32)
        sq = st.relabel(top, n, np.arange(n, dtype=np.int32), n, 1.0)
        rm2, nr2, _, _, scale, want2 = relabel_reference(name, "drop", True)
        red = sq.reduce(rm2, nr2, scale)
        same_bits(to_arrays(ctx, red), want2, f"reduce of the stack's top, raw {raw_on}, under {force}")
        red.close(), sq.close()
    out.close(), st.close(), canon.close(), raw.close()


# ---- dense inverse ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def dense_reference():
    A = N.raw_of("small")[0]
    cols = np.arange(A.shape[0])
    X = D.reference_columns(A, cols)
    return A, cols, X, np.abs(X).max(), D.lapack_error(A, cols, X)


@pytest.mark.parametrize("form", ["cores", "vector"])
def test_dense_inverse_of_a_raw_upload(switches, form):
    """Every column of the inverse the device forms of the raw upload (amg_apply(e_j), a hierarchy of one level) against the
    high-precision inverse of the canonical matrix: the bound, symmetry and A Z = I of test_inverse_columns_against_the_reference."""
    A, cols, X, xmax, lap = dense_reference()
    raw = N.raw_of("small")[1]
    n = A.shape[0]
    Z, z = device_columns(switches, A, cols, form, probe=N.right_hand_side(A, 3), upload=lambda c, M: N.upload_raw(c, *raw, M.shape))
    assert np.isfinite(Z).all() and lap > 0.0
    err = D.relative_error(Z, X)
    sym = float(np.abs(Z[cols] - Z[cols].T).max() / xmax)
    ident = float(np.abs(D.product(A)(Z.astype(LD)) - D.unit_columns(n, cols)).max())
    ident_scale = n * 2.0 ** -52 * np.abs(A.data).max() * float(xmax)
    print(f"NONCANON dense inverse/{form}: device {err:.3e}, lapack {lap:.3e}, ratio {err / lap:.2f} (bound {DENSE_C:g}); "
          f"symmetry/lapack {sym / lap:.2f}; identity {ident / ident_scale:.3e} of n u |A| |Z|")
    assert err <= DENSE_C * lap
    assert sym <= DENSE_C * lap
    assert ident <= DENSE_C * ident_scale
    Zl = Z.astype(LD)
    r = N.right_hand_side(A, 3)
    assert (np.abs(z - Zl @ r) <= n * 2.0 ** -52 * (np.abs(Zl) @ np.abs(r))).all()


# ---- hierarchy and cycle -----------------------------------------------------------------------------------------------------

def test_hierarchy_and_cycle_of_a_raw_upload(ctx, switches):
    """Case a uploaded raw under PADNE_AMG_KEEP=1: level 0 of the hierarchy IS the canonical matrix, and every level passes the
    checks of tests/test_amg_vs_reference.py (aggregation, lambda, prolongator envelope and row sums, Galerkin pattern and
    envelope); the double-precision cycle within its envelope, the single-precision one within F32_FACTOR."""
    A, raw = N.raw_of("mid")
    case = AMG_CASES["a"]
    n = A.shape[0]
    switches.set("PADNE_AMG_KEEP", "1")
    for k, v in case["env"].items():
        switches.set(k, v)
    report = [f"NONCANON hierarchy: n={n} nnz={A.nnz} uploaded as {len(raw[1])} parts"]
    d = N.upload_raw(ctx, *raw, A.shape)
    try:
        d.amg_apply(np.ones(n))
        A0 = d.amg_level(0, "A")
        same_bits((A0.indptr, A0.indices, A0.data), (A.indptr, A.indices, A.data), "level 0 of the hierarchy")
        levels, seen = check_hierarchy(d, case, report)
        assert all(L["f32"] for L in levels[:-1]) and all(L["has_w"] for L in levels[:-1])
    finally:
        d.close()
    levels[0]["A"] = A                                                       # (the canonical matrix as A_0)
    B = right_hand_sides(n, n // 2)
    Z, ENV, e32 = reference_cycle(levels, B)
    zn = norm2(Z)
    assert (e32 > 0).all() and (e32 < 1e-4).all(), e32

    def applied(env):
        for k, v in env.items():
            switches.set(k, v)
        m = N.upload_raw(ctx, *raw, A.shape)
        try:
            return np.stack([m.amg_apply(B[:, j]) for j in range(16)], axis=1)
        finally:
            m.close()
            for k in env:
                switches.unset(k)
    Z64 = applied({"PADNE_AMG_F64": "1"})
    err64 = np.abs(Z64.astype(LD) - Z)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst64 = float(np.where(ENV > 0, err64 / ENV, 0).max())
    Z32 = applied({})
    ratio = norm2(Z32.astype(LD) - Z) / zn / e32
    Zb = None
    m = N.upload_raw(ctx, *raw, A.shape)
    try:
        Zb = m.amg_apply_batch(np.ascontiguousarray(B[:, :8].T)).T
    finally:
        m.close()
    ratio_b = norm2(Zb.astype(LD) - Z[:, :8]) / zn[:8] / e32[:8]
    report.append(f"  f64 cycle: worst error {worst64:.3g} of the envelope; f32 cycle {float(ratio.max()):.2f}, batched "
                  f"{float(ratio_b.max()):.2f} x the plain float32 error (bound {F32_FACTOR:g})")
    print("\n".join(report))
    assert (err64 <= ENV).all(), f"double-precision cycle outside its envelope: {worst64:.3g} x"
    assert float(ratio.max()) <= F32_FACTOR and float(ratio_b.max()) <= F32_FACTOR


def test_a_raw_preconditioner_block(ctx, switches):
    """padne_csr_set_preconditioner_block with a raw upload as the block: the hierarchy is built on the canonical matrix."""
    A, raw = N.raw_of("mid")
    switches.set("PADNE_AMG_COARSE_N", "64")
    b = N.right_hand_side(A)
    x_ref, _ = solution("mid")
    d, blk = ctx.csr_from_scipy(A), N.upload_raw(ctx, *raw, A.shape)
    try:
        d.set_preconditioner_block(blk)
        res = d.solve_spd(b, precond="amg", rtol=1e-12)
        A0 = blk.amg_level(0, "A")
        same_bits((A0.indptr, A0.indices, A0.data), (A.indptr, A.indices, A.data), "level 0 of the block's hierarchy")
        check_solution("block", A, b, res, x_ref)
        assert res.levels >= 3 and res.iterations < 40
        d.set_preconditioner_block(None)
    finally:
        d.close(), blk.close()


# ---- solves ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def solution(name):
    A = N.raw_of(name)[0]
    return N.direct_solution(A, N.right_hand_side(A))


def check_solution(label, A, b, res, x_ref):
    dev = float(np.abs(res.x.astype(LD) - x_ref).max() / np.abs(x_ref).max())
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    Ax = np.zeros(A.shape[0], LD)
    np.add.at(Ax, rows, A.data.astype(LD) * res.x.astype(LD)[A.indices])
    rn = float(norm2(b.astype(LD) - Ax))
    print(f"NONCANON solve {label}: iterations {res.iterations} levels {res.levels} deviation {dev:.3e} (bound {REL_TOL:g}) "
          f"residual {rn:.3e} (bound 1e-9)")
    assert res.status == _hip.OK and res.precond_fallbacks == 0
    assert dev <= REL_TOL
    assert rn < 1e-9


@pytest.mark.parametrize("name,precond", [("mid", "jacobi"), ("mid", "amg"), ("small", "jacobi"), ("small", "amg")])
def test_solves_of_a_raw_upload(ctx, switches, name, precond):
    A, raw = N.raw_of(name)
    if name == "mid":
        switches.set("PADNE_AMG_COARSE_N", "64")
    b = N.right_hand_side(A)
    x_ref, last = solution(name)
    assert last <= 1e-12
    d = N.upload_raw(ctx, *raw, A.shape)
    try:
        res = d.solve_spd(b, precond=precond, rtol=1e-12)
        check_solution(f"{name}/{precond}", A, b, res, x_ref)
        assert d.residual_norm(res.x, b) < 1e-9
        if precond == "amg":
            assert res.levels == (1 if name == "small" else 3), res.levels
            assert res.iterations <= (3 if name == "small" else 40)
        else:
            assert res.levels == 0
    finally:
        d.close()


def test_jacobi_iterates_of_a_raw_upload(ctx):
    """Iterates 1, 2, 3 of the Jacobi loop against pcg_ref on the canonical matrix, under test_pcg_vs_reference's calibrated
    bound (100 x the distance of the float64 host run from the longdouble one)."""
    A, raw = N.raw_of("mid")
    b = N.right_hand_side(A)
    ld, d_host = calibrated(A, b, 3)
    d = N.upload_raw(ctx, *raw, A.shape)
    try:
        for k in (1, 2, 3):
            res = capped(d, b, k, precond="jacobi")
            assert res.iterations == k and res.levels == 0
            check_iterate("noncanonical/jacobi", k, res.x, ld, d_host)
    finally:
        d.close()


def test_a_block_through_solve_system(ctx):
    """An (N, 3) block on the whole KKT system of the small board, L uploaded raw and wrapped as solve_system takes it."""
    L, r, n_pot = N.kkt_system()
    raw = N.scramble(L, 5)
    layout = reduction.infer_layout(L, r)
    rng = np.random.default_rng(9)
    Rb = np.repeat(r[:, None], 3, axis=1)
    Rb[:n_pot, 1] *= -2.5
    Rb[:n_pot, 2] = 0.0
    into = rng.choice(n_pot, 8, replace=False)
    Rb[into[:4], 2], Rb[into[4:], 2] = 1.0, -1.0
    V_ref, last = N.direct_solution(L, Rb)
    assert last <= 1e-12
    Ls = solver.SystemMatrix(N.upload_raw(ctx, *raw, L.shape), layout)
    try:
        held_canonical(ctx, Ls.dev, L, "the uploaded KKT system")
        V, info = solver.solve_system(Ls, Rb)
    finally:
        Ls.close()
    assert V.shape == Rb.shape and info.residual_norms.shape == (3,)
    for j in range(3):
        pot = float(np.abs(V[:n_pot, j] - V_ref[:n_pot, j]).max() / np.abs(V_ref[:n_pot, j]).max())
        cur = float(np.abs(V[n_pot:, j] - V_ref[n_pot:, j]).max())
        cur_bound = max(REL_TOL * float(np.abs(V_ref[n_pot:, j]).max()), 1e-9)
        print(f"NONCANON solve_system column {j}: potentials {pot:.3e} (bound {REL_TOL:g}), multipliers {cur:.3e} (bound "
              f"{cur_bound:.1e}), residual {info.residual_norms[j]:.3e} (bound 1e-9)")
        assert pot <= REL_TOL and cur <= cur_bound
        assert info.residual_norms[j] < 1e-9
    assert info.residual_norm < 1e-9


# ---- KKT plan --------------------------------------------------------------------------------------------------------------

def test_kkt_plan_on_a_raw_upload_stage_by_stage(ctx):
    """The voltage_source fixture (values rounded to float32), L uploaded raw: the map, the reduced matrix and both stages
    through the checker of tests/test_kkt_plan_vs_reference.py, whose references are computed from the canonical L."""
    g = H.load_golden("voltage_source")
    S = KktSystem(N.round32(H.golden_L(g)), g["r"], scale_own_r=True)
    raw = N.scramble(S.L, 6)
    assert len(raw[1]) > S.L.nnz
    S._dev = N.upload_raw(ctx, *raw, S.L.shape)
    R1 = S.r[:, None].copy()
    red, kidx, kval, extras, probes = S.lists(R1)
    plan, ref, imap, src = list_plan(ctx, S, red)
    try:
        A = check_matrix(plan, ref)
        kkt_run(ctx, plan, S, ref, imap, src, R1, kidx, kval, extras, probes, entry="single", red=red, A=A)
        Rb = S.block(5, seed=3, own_r=True)
        red5, kidx, kval, extras, probes = S.lists(Rb)
        kkt_run(ctx, plan, S, ref, imap, src, Rb, kidx, kval, extras, probes, red=red5, A=A)
    finally:
        plan.close()
        S._dev.close()


# ---- entries that need the mesh of an assembled system ------------------------------------------------------------------------

def refusal(fn):
    try:
        fn()
    except ValueError as exc:
        return str(exc)
    return None


def test_mesh_entries_answer_a_raw_upload_as_a_canonical_one(ctx):
    """No uploaded matrix carries a mesh: padne_thermal_create, padne_thermal_create_stacked and padne_coupled_create refuse the
    raw upload with the words they have for the canonical one, padne_csr_power_density answers both alike, and the context
    goes on.  (padne_transient_create takes the thermal handle alone.)"""
    A, raw = N.raw_of("small")
    n = A.shape[0]
    x = N.right_hand_side(A, 4)
    want = exact_rows(A, A.data, x, LD)
    # a thermal handle of an assembled system, for padne_coupled_create to be offered with an uploaded L
    sysm = synthetic.layered_system(1, 8, 6, via_lattice=4)
    xy = np.concatenate([m[0] for m in sysm.meshes])
    tri = np.concatenate([m[1] for m in sysm.meshes])
    mvo = sysm.mesh_offsets
    mto = np.concatenate([[0], np.cumsum([len(m[1]) for m in sysm.meshes])])
    NN = sysm.n_vertices + 1
    Ld = ctx.assemble_system(NN, xy, tri, mvo, mto, [m[2] for m in sysm.meshes], [NN - 1, sysm.ground], [sysm.ground, NN - 1],
                             [1.0, 1.0])
    n_mesh = len(sysm.meshes)
    th = _hip.Thermal(Ld, NN - 1, np.full(n_mesh, 1.0), np.full(n_mesh, 0.5))
    answers = []
    for d in (ctx.csr_from_scipy(A), N.upload_raw(ctx, *raw, A.shape)):
        got = dict(
            thermal=refusal(lambda: _hip.Thermal(d, n, [1.0], [0.5])),
            stacked=refusal(lambda: _hip.Thermal(d, n, [1.0], [0.5], mesh_layer=[0])),
            coupled=refusal(lambda: _hip.Coupled(d, th, np.zeros(n_mesh), 25.0, 25.0)))
        try:
            got["power"] = d.power_density(x, 0).tobytes()
        except ValueError as exc:
            got["power"] = str(exc)
        answers.append(got)
        bound_ok(d.matvec(x), want[0], want[1], np.diff(A.indptr), BOUND_C[PLAIN], U)      # the context goes on
        d.close()
    print(f"NONCANON mesh entries: {answers[0]}")
    assert answers[0] == answers[1]
    for k in ("thermal", "stacked", "coupled"):
        assert answers[0][k], f"{k}: a matrix without a mesh was taken"
    th.close()
    Ld.close()


# ---- the guarded, poisoned allocator -------------------------------------------------------------------------------------------

def everything_once(ctx, names, multigrid):
    out = {}
    for name in names:
        A, d = upload(ctx, name)
        x = np.random.default_rng(5).uniform(-1, 1, A.shape[1])
        got = [d.to_scipy(), d.matvec(x), d.matmat8(product_vectors(A, 3)), d.residual_norm(x, np.ones(A.shape[0]))]
        for kind in MAPS:
            rm, nr, cm, nc, scale, _ = relabel_reference(name, kind, False)
            got.append(d.relabel(rm, nr, cm, nc, scale).to_scipy())
            if A.shape[0] == A.shape[1]:
                rm, nr, _, _, scale, _ = relabel_reference(name, kind, True)
                got.append(d.reduce(rm, nr, scale).to_scipy())
        canon = ctx.csr_from_scipy(A)
        st = canon.vstack(d)
        _, rm, nr, cm, nc, _ = vstack_reference(name)
        got += [st.to_scipy(), st.relabel(rm, nr, cm, nc, -1.0).to_scipy()]
        st.close(), canon.close()
        if name in N.SPD:
            b = N.right_hand_side(A)
            got.append(d.solve_spd(b, precond="jacobi", rtol=1e-10).x)
            if multigrid:
                res = d.solve_spd(b, precond="amg", rtol=1e-12)
                got += [res.x, res.iterations, res.levels, d.amg_apply(b), d.amg_shapes()]
                got += [d.amg_level(l, w) for l in range(res.levels - 1) for w in "AP"]
        out[name] = got
        d.close()
    return out


def test_the_small_systems_under_the_guarded_allocator(ctx, switches):
    """Every family above once on the rectangular and the 160-unknown system: the same bits with the switch unset, under
    PADNE_POOL_GUARD=00 and =ff, and no guard zone touched (the dense inverse as the preconditioner)."""
    three_ways(ctx, switches, lambda: everything_once(ctx, ("rect", "small"), True))


def test_the_hierarchy_of_a_raw_upload_under_the_guarded_allocator(ctx, switches):
    """Case a (three levels) the same way."""
    three_ways(ctx, switches, lambda: everything_once(ctx, ("mid",), True), env={"PADNE_AMG_COARSE_N": "64", "PADNE_AMG_KEEP": "1"})

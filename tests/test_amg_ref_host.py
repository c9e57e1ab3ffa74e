"""tests/amg_ref.py on the host: a conforming hierarchy passes every checker, every listed defect fails one.

The hierarchy is built HERE, by the plainest means the specification allows -- roots by a greedy distance-2 independent set
in index order (the device's hashed rounds pick other roots: both conform), the two join passes, P and P^T A P in
longdouble rounded once to double -- and handed to the same checkers tests/test_amg_vs_reference.py hands the device's
arrays to.  What the mutations show is that those checkers would fail for a subtly wrong kernel: one vertex in a
neighbouring aggregate, two adjacent roots, a missing root, omega off by 2 %, one weak entry not lumped, one entry of P off
by 1e-10, one entry of A_c dropped, a damping off by 1 %, a cycle without its post-sweep or with a stale residual in it.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import amg_ref as R
import dense_ref as D

LD = np.longdouble


def host_hierarchy(A, coarse_n):
    """Levels of a conforming hierarchy: dicts of A, S, root, agg, P (double), Pt / envP (reference and envelope), Ac /
    envA, lam, jac.  The last entry has only A."""
    levels = []
    A = R.csr(A)
    while A.shape[0] > coarse_n:
        S = R.strength(A)
        root = R.greedy_roots(S)
        agg = R.renumbered(R.joined(S, root))
        Pt, envP, omega, skip = R.prolongator(S, agg)
        P = Pt.to_scipy()
        Act, envA = R.galerkin(A, P)
        Ac = Act.to_scipy()
        Ac = R.csr((Ac + Ac.T) * 0.5)                                       # (exactly symmetric, as dense_ref asks)
        lam_plain, _ = R.bounds(S)
        d = 1 / np.sqrt(A.diagonal())
        lam_max = float(spla.eigsh(sp.diags(d) @ A @ sp.diags(d), k=1, which="LA", return_eigenvectors=False, tol=1e-8)[0])
        lam = float(lam_plain) if not levels else min(float(lam_plain), 1.08 * lam_max)
        levels.append(dict(A=A, S=S, root=root, agg=agg, P=P, Pt=Pt, envP=envP, skip=skip, omega=omega, Act=Act, envA=envA,
                           lam=lam, jac=float(LD(1) / (LD(R.CHEB) * LD(lam))), lam_plain=lam_plain, lam_max=lam_max))
        A = Ac
    levels.append(dict(A=A))
    return levels


@pytest.fixture(scope="module", params=["layered", "obtuse"])
def hierarchy(request):
    if request.param == "layered":
        A = R.layered_matrix(2, 40, 30, 4)
        assert A.shape[0] == 2399
    else:
        A = R.obtuse_matrix(50, 44)
        off = A - sp.diags(A.diagonal())
        assert off.data.max() > 0, "the mesh must have an edge with a positive off-diagonal entry"
    lv = host_hierarchy(A, 64)
    assert len(lv) >= 3
    return lv


def cycle_parts(lv):
    levels = [(L["A"], L["P"], L["lam"]) for L in lv[:-1]]
    return levels, D.refined_solver(lv[-1]["A"])


def test_the_conforming_hierarchy_passes_every_checker(hierarchy):
    lv = hierarchy
    for l, L in enumerate(lv[:-1]):
        assert L["S"].undecided_share() == 0.0
        assert R.check_aggregation(L["S"], L["agg"], L["root"]) == 0
        assert L["P"].shape[1] == int(L["agg"].max()) + 1 < L["A"].shape[0]
        assert R.check_entries(L["Pt"], L["envP"], L["P"], "P", L["skip"], zero_may_be_absent=True) <= 1.0
        assert R.check_entries(L["Act"], L["envA"], lv[l + 1]["A"], "A_c") <= 1.0
        ratio = R.check_smoothing(L["lam"], L["jac"], L["lam_plain"], int(np.diff(L["A"].indptr).max()), l, L["lam_max"])
        assert ratio > 1
        # unit row sums where the equation sums to zero
        P, A = L["P"], L["A"]
        zero_sum = np.abs(np.asarray(A.sum(axis=1)).ravel()) <= 1e-9 * A.diagonal()
        assert zero_sum.any()
        assert np.abs(np.asarray(P.sum(axis=1)).ravel()[zero_sum] - 1).max() <= 1e-13
    # the cycle in plain double precision lies within the forward-error envelope of the longdouble one
    levels, coarse = cycle_parts(lv)
    rng = np.random.default_rng(1)
    b = rng.uniform(-1, 1, lv[0]["A"].shape[0])
    z, env = R.cycle_envelope(levels, coarse, lv[-1]["A"], b)
    inv64 = np.float64(coarse(np.eye(lv[-1]["A"].shape[0], dtype=LD)))
    z64 = R.cycle(levels, inv64, b, dtype=np.float64)
    assert (np.abs(z64 - z) <= env).all() and np.abs(z64 - z).max() > 0
    # (the envelope is dominated by the coarsest solve, cond(A_c) u; it must stay well below the rounding of a single-precision
    # step, 6e-8, which is the smallest defect of the double-precision cycle it is there to catch)
    assert env.max() <= 1e-8 * np.abs(z).max(), "an envelope that wide checks nothing"


def test_a_vertex_in_a_neighbouring_aggregate_is_rejected(hierarchy):
    for L in hierarchy[:-1]:
        S, agg, root = L["S"], L["agg"], L["root"]
        G = S.graph()
        moved = 0
        for i in np.flatnonzero(~root):
            nb = G.indices[G.indptr[i]:G.indptr[i + 1]]
            other = nb[agg[nb] != agg[i]]
            if len(other):
                bad = agg.copy()
                bad[i] = agg[other[0]]
                with pytest.raises(AssertionError, match="join different roots|are one aggregate"):
                    R.check_aggregation(S, bad, root)
                moved += 1
                if moved == 5:
                    break
        assert moved


def test_adjacent_roots_a_missing_root_and_an_empty_aggregate_are_rejected(hierarchy):
    for L in hierarchy[:-1]:
        S, agg, root = L["S"], L["agg"], L["root"]
        G = S.graph()
        r = next(int(i) for i in np.flatnonzero(root) if G.indptr[i + 1] > G.indptr[i])
        j = int(G.indices[G.indptr[r]])
        two = root.copy()
        two[j] = True                                           # two adjacent roots, the second with an aggregate of its own
        own = agg.copy()
        own[j] = agg.max() + 1
        with pytest.raises(AssertionError, match="within two strong hops"):
            R.check_aggregation(S, own, two)
        gone = root.copy()
        gone[r] = False                                         # a root removed, its vertices left where they were
        with pytest.raises(AssertionError, match="without a root|more than two strong hops from every root"):
            R.check_aggregation(S, agg, gone)
        # ... or handed to the neighbouring roots by the join rule: the set of roots is no longer maximal
        far = R.renumbered(R.joined(S, gone))
        with pytest.raises(AssertionError, match="more than two strong hops from every root|have strong neighbours and are alone"):
            R.check_aggregation(S, far, gone)
        with pytest.raises(AssertionError, match="empty aggregates"):
            R.check_aggregation(S, agg + (agg >= 3), root)


def test_a_wrong_omega_or_an_unlumped_weak_entry_or_a_wrong_entry_of_p_is_rejected(hierarchy):
    seen_weak = False
    for L in hierarchy[:-1]:
        S, agg = L["S"], L["agg"]
        with pytest.raises(AssertionError, match="outside the envelope"):
            R.check_entries(L["Pt"], L["envP"], R.prolongator(S, agg, omega_scale=0.98)[0].to_scipy(), "P", L["skip"], True)
        # 1.4 / lambda instead of 1.5 / lambda, the issue's own example
        with pytest.raises(AssertionError, match="outside the envelope"):
            R.check_entries(L["Pt"], L["envP"], R.prolongator(S, agg, omega_scale=1.4 / 1.5)[0].to_scipy(), "P", L["skip"], True)
        _, keep, _, _, _ = R.filtered(S)
        # (a weak entry towards ANOTHER aggregate: inside the row's own aggregate lumped and unlumped give the same row of P)
        weak = np.flatnonzero(S.off & ~keep & (agg[S.row] != agg[S.col]))
        if len(weak):
            seen_weak = True
            with pytest.raises(AssertionError, match="outside the envelope|the reference has not"):
                R.check_entries(L["Pt"], L["envP"], R.prolongator(S, agg, unlumped=int(weak[len(weak) // 2]))[0].to_scipy(), "P",
                                L["skip"], True)
        P = L["P"].copy()
        k = P.nnz // 2
        P.data[k] *= 1 + 1e-10
        with pytest.raises(AssertionError, match="1 values outside the envelope"):
            R.check_entries(L["Pt"], L["envP"], P, "P", L["skip"], True)
        P = L["P"].copy()
        P.data[k] = 0.0
        P.eliminate_zeros()                                     # a dropped entry whose reference value is not zero
        with pytest.raises(AssertionError, match="1 entries of the reference are missing"):
            R.check_entries(L["Pt"], L["envP"], P, "P", L["skip"], True)
    assert seen_weak, "no level of this hierarchy has a weak entry: the lumping is not exercised"


def test_a_dropped_or_wrong_entry_of_the_coarse_operator_is_rejected(hierarchy):
    lv = hierarchy
    for l, L in enumerate(lv[:-1]):
        Ac = lv[l + 1]["A"].copy()
        k = int(np.argmin(np.abs(Ac.data)))                     # the smallest entry: invisible to a max-norm bar
        assert abs(Ac.data[k]) <= 1e-3 * np.abs(Ac.data).max() or Ac.shape[0] < 400
        small = Ac.data[k]
        Ac.data[k] = 0.0
        assert abs(Ac - lv[l + 1]["A"]).max() == abs(small)
        Ac.eliminate_zeros()
        with pytest.raises(AssertionError, match="1 entries of the reference are missing"):
            R.check_entries(L["Act"], L["envA"], Ac, "A_c")
        Ac = lv[l + 1]["A"].copy()
        Ac.data[k] *= 1 + 1e-10
        with pytest.raises(AssertionError, match="1 values outside the envelope"):
            R.check_entries(L["Act"], L["envA"], Ac, "A_c")


def test_a_damping_off_by_one_percent_or_an_unstable_bound_is_rejected(hierarchy):
    for l, L in enumerate(hierarchy[:-1]):
        m = int(np.diff(L["A"].indptr).max())
        for f in (0.99, 1.01):
            with pytest.raises(AssertionError, match="jac_"):
                R.check_smoothing(L["lam"], L["jac"] * f, L["lam_plain"], m, l, L["lam_max"])
        with pytest.raises(AssertionError, match="not a contraction"):
            R.check_smoothing(L["lam_max"] / 1.1 * 0.999, 1 / (0.55 * L["lam_max"] / 1.1 * 0.999), L["lam_plain"], m, max(l, 1),
                              L["lam_max"])
        with pytest.raises(AssertionError, match="lambda_"):
            R.check_smoothing(float(L["lam_plain"]) * 1.001, 1 / (0.55 * float(L["lam_plain"]) * 1.001), L["lam_plain"], m, l,
                              L["lam_max"])


@pytest.mark.parametrize("post", ["skip", "stale"])
def test_a_cycle_without_its_post_sweep_or_with_a_stale_residual_is_rejected(hierarchy, post):
    """Both criteria of the device test: the double-precision envelope and 8 x the error of the plain float32 evaluation."""
    lv = hierarchy
    levels, coarse = cycle_parts(lv)
    n, nc = lv[0]["A"].shape[0], lv[-1]["A"].shape[0]
    inv = coarse(np.eye(nc, dtype=LD))
    rng = np.random.default_rng(2)
    rhs = [rng.uniform(-1, 1, n), np.ones(n), np.eye(n)[n // 2]]
    for b in rhs:
        z, env = R.cycle_envelope(levels, coarse, lv[-1]["A"], b)
        wrong64 = R.cycle(levels, np.float64(inv), b, dtype=np.float64, post=post)
        assert (np.abs(wrong64 - z) > env).any()
        nrm = lambda v: float(np.sqrt((np.asarray(v, LD) ** 2).sum()))
        e32 = nrm(R.cycle(levels, inv, b, dtype=np.float32) - z) / nrm(z)
        wrong32 = nrm(R.cycle(levels, inv, b, dtype=np.float32, post=post) - z) / nrm(z)
        assert 0 < e32 < 1e-5
        assert wrong32 > 8 * e32, (post, wrong32, e32)


def test_the_longdouble_cycle_is_the_explicit_operator_and_symmetric():
    """On a 300-unknown system, two levels: the cycle applied to the identity equals
    2cD^-1 - c^2 D^-1 A D^-1 + (I - cD^-1 A) P A_c^-1 P^T (I - cAD^-1) as dense matrices, and is symmetric."""
    A = R.obtuse_matrix(43, 7)
    assert A.shape[0] == 300
    lv = host_hierarchy(A, 299)
    assert len(lv) == 2
    L = lv[0]
    inv = D.reference_columns(lv[1]["A"])
    M = R.cycle([(L["A"], L["P"], L["lam"])], inv, np.eye(300, dtype=LD))
    E = R.explicit_cycle_matrix(L["A"], L["P"], L["lam"], inv)
    scale = np.abs(E).max()
    assert np.abs(M - E).max() <= 1e-16 * scale
    assert np.abs(M - M.T).max() <= 1e-16 * scale
    assert np.linalg.eigvalsh(np.float64((M + M.T) / 2)).min() > 0
    # and the deeper hierarchy's cycle is symmetric too (every level's R is P^T, the same damping before and after)
    lv = host_hierarchy(A, 40)
    assert len(lv) >= 3
    levels, coarse = cycle_parts(lv)
    M = R.cycle(levels, coarse, np.eye(300, dtype=LD))
    assert np.abs(M - M.T).max() <= 1e-16 * np.abs(M).max()

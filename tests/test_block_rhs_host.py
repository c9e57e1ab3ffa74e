"""Host half of ``solve_system`` on a block of right-hand sides (no GPU): the block reduction, the multiplier recovery
from probe rows, and the shape checks that come before the device is touched."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers as H
from padne_amd import reduction as R
from padne_amd import solver

NAMES = H.golden_names() + H.problem_golden_names()


def layout_of(name):
    """(L, r, layout) of a fixture as ``solve_system`` infers it from the bare matrix."""
    g = H.load_golden(name)
    L = H.golden_L(g)
    L.sort_indices()
    r = np.asarray(g["r"], dtype=np.float64)
    return L, r, R.infer_layout(L, r)


def block_of(L, r, layout, k, seed):
    """k columns: r itself, then random current injections and source voltages; column 2 sets every source to 0 V."""
    rng = np.random.default_rng(seed)
    n_pot = layout.n_potential
    B = np.repeat(r[:, None], k, axis=1)
    for j in range(1, k):
        B[:n_pot, j] = r[:n_pot] * rng.uniform(-2, 2)
        for cst in layout.constraints:
            if cst.n >= 0:
                B[cst.index, j] = 0.0 if j == 2 else rng.uniform(-5, 5)
    return B


def pins_of(L, layout):
    return R.floating_component_pins(layout.n_potential, layout.ground_constraint.p, layout.constraints, matrix=L)


def structure(red):
    return (red.elim.tolist(), list(red.tied), red.n_free,
            [(list(mem), [c.index for c in cons], root) for mem, cons, root in red.groups],
            [c.index for c in red.regulators])


@pytest.mark.parametrize("name", NAMES)
def test_block_reduction_equals_the_reduction_of_every_column(name):
    L, r, layout = layout_of(name)
    B = block_of(L, r, layout, 5, seed=len(name))
    pins = pins_of(L, layout)
    red, kidx, kval = R.build_block_reduction(layout, {c.index: B[c.index, :] for c in layout.constraints}, pins)
    assert kval.shape == (5, len(kidx)) and np.all(np.diff(kidx) > 0)
    assert red.known == {}
    for j in range(5):
        for cst in layout.constraints:
            cst.value = float(B[cst.index, j])
        col = R.build_reduction(layout, pins)
        assert structure(col) == structure(red)
        # the column's known part, bit for bit, on the union of the indices; zero wherever the column knows nothing
        assert set(col.known) <= set(kidx.tolist())
        got = dict(zip(kidx.tolist(), kval[j].tolist()))
        for x, val in got.items():
            assert val == col.known.get(x, 0.0)
    if any(c.n >= 0 for c in layout.constraints):
        assert len(kidx) and not np.any(kval[2])          # sources at 0 V against a grounded terminal: nothing is known


def host_probes(L, B, red, kidx, kval, members, V):
    """What the device returns at the members, computed on the host from the direct solutions V: rho_j = r_j - L v0_j with
    v0_j the solution with zero multipliers and zero regulator currents, and L Z_k."""
    N, n_pot = L.shape[0], red.layout.n_potential
    imap = red.index_map
    rows = np.flatnonzero(imap >= 0)
    P = sp.csr_matrix((np.ones(len(rows)), (rows, imap[rows])), shape=(N, red.n_free))
    A = (-(P.T @ L @ P)).tocsc()
    Z = []
    for cst in red.regulators:
        z = spla.spsolve(A, red.project(cst.gamma))
        Z.append(P @ z)
    k = B.shape[1]
    out = np.zeros((k + len(Z), len(members)))
    for j in range(k):
        v0 = V[:, j].copy()
        v0[n_pot:] = 0.0
        for q, cst in enumerate(red.regulators):
            v0 -= V[cst.index, j] * Z[q]
        out[j] = (B[:, j] - L @ v0)[members]
    for q, z in enumerate(Z):
        out[k + q] = (L @ z)[members]
    return out


@pytest.mark.parametrize("name", [n for n in NAMES if n in ("voltage_source", "regulator", "glue_sources", "two_layer_via",
                                                            "problem_mixed", "problem_two_planes", "problem_c1")])
def test_multiplier_recovery_from_probe_rows_matches_the_direct_solve(name, monkeypatch):
    L, r, layout = layout_of(name)
    k = 4
    B = block_of(L, r, layout, k, seed=7)
    pins = pins_of(L, layout)
    red, kidx, kval = R.build_block_reduction(layout, {c.index: B[c.index, :] for c in layout.constraints}, pins)
    if pins:
        pytest.skip("floating copper: the direct solve is singular there")
    V = spla.spsolve(L.tocsc(), B)
    members = red.probe_members
    probes = host_probes(L, B, red, kidx, kval, members, V)
    calls = []
    peel = red.multipliers
    monkeypatch.setattr(red, "multipliers", lambda *a, **kw: calls.append(1) or peel(*a, **kw))
    i_reg, mult = R.recover_currents(red, members, probes, k)
    K = len(red.regulators)
    assert i_reg.shape == (k, K) and len(mult) == k
    assert len(calls) == (2 * k + K if K else k)    # per column F0 and the final peel; J once for the block
    for j in range(k):
        # (the currents of the column, or the injections where the currents vanish: rho is formed to that rounding)
        scale = max(np.abs(V[layout.n_potential:, j]).max(), np.abs(B[:layout.n_potential, j]).max(), 1e-300)
        for q, cst in enumerate(red.regulators):
            assert abs(i_reg[j, q] - V[cst.index, j]) <= 1e-9 * scale
        assert set(mult[j]) == {c.index for c in layout.constraints}
        for idx, val in mult[j].items():
            assert abs(val - V[idx, j]) <= 1e-9 * scale, (j, idx, val, V[idx, j])


def test_recovery_of_one_column_is_the_single_right_hand_side_arithmetic():
    """n_cols = 1 is what solve_system does for a vector r: the same calls in the same order, hence the same bits as the
    block's column 0 (J is formed from column 0)."""
    L, r, layout = layout_of("regulator")
    B = block_of(L, r, layout, 3, seed=3)
    red, kidx, kval = R.build_block_reduction(layout, {c.index: B[c.index, :] for c in layout.constraints}, [])
    members = red.probe_members
    V = spla.spsolve(L.tocsc(), B)
    probes = host_probes(L, B, red, kidx, kval, members, V)
    i3, m3 = R.recover_currents(red, members, probes, 3)
    single = np.concatenate([probes[:1], probes[3:]])
    i1, m1 = R.recover_currents(red, members, single, 1)
    assert np.array_equal(i1[0], i3[0]) and m1[0] == m3[0]


@pytest.mark.parametrize("shape,match", [((5, 4, 2), "vector or"), ((5, 0), "no right-hand sides"), ((4, 2), "rows")])
def test_block_shape_is_checked_before_the_device(shape, match):
    L = sp.random(5, 5, density=0.5, format="csr", random_state=0)
    with pytest.raises(ValueError, match=match):
        solver.solve_system(L, np.zeros(shape))


def test_solver_info_keeps_its_positional_fields():
    info = solver.SolverInfo(0.5, 1e-12, 3, 1e-13, 0.25)
    assert info.residual_norms is None and info.iterations == 3


def test_a_stall_of_a_block_is_attributed_to_the_columns_that_show_it():
    R = np.ones((4, 3))
    msg = solver._stalled_columns(np.array([1e-12, 5e-8, 3e-9]), R)
    assert "column(s) 1, 2)" in msg and "reported as a whole" in msg
    msg = solver._stalled_columns(np.array([1e-12, 4e-12, 2e-12]), R)      # none above the bar: the worst one
    assert "column(s) 1)" in msg

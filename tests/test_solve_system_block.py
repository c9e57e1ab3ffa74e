"""``solve_system(L, R)`` with a block R of shape (N, k), as the reference's ``spsolve`` takes it: every column against one
direct solve of the whole block, the block against its columns one by one, the lockstep grouping of its reduced solves,
and ``SystemMatrix @ V``."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import helpers as H
from oracle import padne_oracle as O
from padne_amd import solver, synthetic

pytestmark = pytest.mark.gpu

REL_TOL = 1e-8
NAMES = H.golden_names()
PROBLEMS = H.problem_golden_names()


def load_cases(r, layout, k=4, seed=0):
    """r; r with its current injections scaled; r with other source voltages (the ground row stays 0); an all-zero column."""
    rng = np.random.default_rng(seed)
    n_pot = layout.n_potential
    R = np.repeat(np.asarray(r, dtype=np.float64)[:, None], k, axis=1)
    R[:n_pot, 1] *= 2.5
    for cst in layout.constraints:
        if cst.n >= 0:
            R[cst.index, 2] = 2.5 * r[cst.index] + rng.uniform(0.1, 1.0)
    R[:, 3] = 0.0
    return R


def check_block(Lh, R, V, info, n_pot, tol=REL_TOL):
    V_ref = spla.spsolve(Lh.tocsc(), R)
    k = R.shape[1]
    assert V.shape == R.shape and V.flags.c_contiguous and V.dtype == np.float64
    assert info.residual_norms.shape == (k,) and info.ground_node_current.shape == (k,)
    assert np.array_equal(info.ground_node_current, V[-1])
    for j in range(k):
        if not R[:, j].any():
            assert not V[:, j].any()                                    # the zero column is exactly zero
            assert info.residual_norms[j] == 0.0
            continue
        scale_pot = np.abs(V_ref[:n_pot, j]).max()
        assert np.abs(V[:n_pot, j] - V_ref[:n_pot, j]).max() <= tol * scale_pot, j
        scale_cur = max(np.abs(V_ref[n_pot:, j]).max(), 1e-30)
        assert np.abs(V[n_pot:, j] - V_ref[n_pot:, j]).max() <= max(REL_TOL * scale_cur, 1e-9), j
        assert info.residual_norms[j] < 1e-9, j
    assert abs(info.residual_norm - np.sqrt(np.sum(info.residual_norms ** 2))) <= 1e-12 * max(info.residual_norm, 1e-300)
    assert np.linalg.norm(Lh @ V - R) < 1e-9
    return V_ref


def regulator_tolerance(L, r, n_pot):
    """Twice the fixture's own conditioning, as test_solve_system_vs_reference_golden holds the `regulator` fixture: how
    far one ulp in the diagonal moves its potentials (it couples two islands through 100 kOhm next to a 2 kS sheet)."""
    d = L.diagonal()
    v0 = O.solve_system(L, r)[0]
    worst = 0.0
    for seed in (0, 1):
        k = np.random.default_rng(seed).integers(-1, 2, len(d))
        v1 = O.solve_system((L + sp.diags(d * (k * 2.220446049250313e-16))).tocsr(), r)[0]
        worst = max(worst, np.abs(v1[:n_pot] - v0[:n_pot]).max() / max(np.abs(v0[:n_pot]).max(), 1e-300))
    return 2 * worst


@pytest.mark.parametrize("name", NAMES)
def test_block_of_load_cases_on_every_golden_fixture(ctx, name):
    g = H.load_golden(name)
    meshes, sig, stamps, r, n_pot = H.product_system(g)
    L = solver.assemble_from_arrays(meshes, sig, stamps, n_pot)
    R = load_cases(r, L.layout)
    V, info = solver.solve_system(L, R)
    tol = regulator_tolerance(H.golden_L(g), r, n_pot) if name == "regulator" else REL_TOL
    check_block(H.golden_L(g), R, V, info, n_pot, tol)
    L.close()


@pytest.mark.parametrize("name", PROBLEMS)
def test_block_of_load_cases_on_every_problem_fixture_as_a_bare_matrix(ctx, name):
    g = H.load_golden(name)
    Lh = H.golden_L(g)
    r = np.asarray(g["r"], dtype=np.float64)
    v1, info1 = solver.solve_system(Lh, r)                             # the single call on this matrix passes first
    assert info1.residual_norm < 1e-9
    from padne_amd.reduction import infer_layout
    layout = infer_layout(Lh.tocsr(), r)
    R = load_cases(r, layout)
    V, info = solver.solve_system(Lh, R)
    check_block(Lh, R, V, info, layout.n_potential)


def test_block_equals_its_columns_and_shares_the_plan(ctx):
    g = H.load_golden("voltage_source")
    meshes, sig, stamps, r, n_pot = H.product_system(g)
    L = solver.assemble_from_arrays(meshes, sig, stamps, n_pot)
    v_before, info_before = solver.solve_system(L, r)
    plan = next(iter(L._plans.values()))
    R = load_cases(r, L.layout)
    V, info = solver.solve_system(L, R)
    assert len(L._plans) == 1 and next(iter(L._plans.values())) is plan
    for j in range(R.shape[1]):
        v_j, info_j = solver.solve_system(L, R[:, j])
        assert np.abs(V[:, j] - v_j).max() <= 1e-9 * max(np.abs(v_j).max(), 1e-300)
    assert len(L._plans) == 1 and next(iter(L._plans.values())) is plan
    v_after, info_after = solver.solve_system(L, r)
    assert np.array_equal(v_after, v_before)
    assert info_after.residual_norm == info_before.residual_norm
    assert info_after.ground_node_current == info_before.ground_node_current
    assert info_after.residual_norms is None
    L.close()


@pytest.mark.parametrize("name", ["voltage_source", "regulator", "two_layer_via"])
def test_single_column_block_is_the_vector_call(ctx, name):
    g = H.load_golden(name)
    meshes, sig, stamps, r, n_pot = H.product_system(g)
    L = solver.assemble_from_arrays(meshes, sig, stamps, n_pot)
    v, info = solver.solve_system(L, r)
    v1, info1 = solver.solve_system(L, r[:, None])
    assert v1.shape == (len(r),)
    assert np.array_equal(v1, v)
    assert info1.residual_norm == info.residual_norm and info1.ground_node_current == info.ground_node_current
    assert info1.iterations == info.iterations and info1.residual_norms is None       # (solve_seconds is a wall time)
    L.close()


def layered(seed=3):
    """Two layers of 60 x 60 vertices with vias: above the dense-inverse size, so the reduced solves take the multigrid
    and the lockstep grouping."""
    sysm = synthetic.layered_system(2, 60, 60, via_lattice=6)
    els = [("R", int(a), int(b), float(rr)) for a, b, rr in zip(*sysm.resistors)]
    Lo, _ = O.assemble_system([(m[0], m[1], m[2]) for m in sysm.meshes], 0, els, sysm.ground)
    return sysm, Lo


@pytest.mark.parametrize("k,groups", [(2, 0), (3, 0), (4, 1), (5, 1), (8, 1), (9, 1), (17, 2)])
def test_lockstep_widths_of_a_block(ctx, k, groups):
    sysm, Lo = layered()
    N = Lo.shape[0]
    src, snk = synthetic.multi_rhs_pairs(sysm, k, seed=k)
    R = np.zeros((N, k))
    R[src, np.arange(k)] += 1.0 + np.arange(k)
    R[snk, np.arange(k)] -= 1.0 + np.arange(k)
    before = ctx.lockstep_groups()
    V, info = solver.solve_system(Lo, R)
    assert ctx.lockstep_groups() - before == groups
    check_block(Lo, R, V, info, N - 1)


def five_regulators(k):
    """The system of test_five_regulators_advance_in_lockstep_and_match_the_direct_solve, with k load cases that differ in
    the load current and the regulators' set points."""
    rng = np.random.default_rng(11)
    meshes, offs = [], [0]
    for layer, (nx, ny) in enumerate(((90, 80), (90, 80))):
        xy, tri = synthetic.jittered_grid(nx, ny, seed=20 + layer)
        meshes.append((xy, tri, 2082.5))
        offs.append(offs[-1] + len(xy))
    n_vert = offs[-1]
    vert = lambda l: int(rng.integers(offs[l], offs[l + 1]))  # noqa: E731
    els = [("R", vert(0), vert(1), float(10 ** rng.uniform(-3, -1))) for _ in range(12)]
    load = (vert(0), vert(1))
    els.append(("I", load[0], load[1], 1.5))
    used = set()

    def fresh(l):
        while True:
            v = vert(l)
            if v not in used:
                used.add(v)
                return v
    regs = []
    for q in range(5):
        vp, vn, sf, st = fresh(0), fresh(1), fresh(0), fresh(1)
        els.append(("REG", vp, vn, sf, st, 1.0 + 0.5 * q, 0.6 + 0.1 * q, n_vert + q))
        regs.append(n_vert + q)
        els.append(("R", vp, vn, 1.0 + q))
    Lo, ro = O.assemble_system(meshes, 0, els, 0)
    R = np.repeat(ro[:, None], k, axis=1)
    for j in range(1, k):
        R[load[0], j] += 0.5 * j
        R[load[1], j] -= 0.5 * j
        R[regs, j] *= 1.0 + 0.1 * j
    return Lo, R, n_vert


def test_regulator_columns_are_solved_once_per_block(ctx):
    k = 6
    Lo, R, n_pot = five_regulators(k)
    V_ref = spla.spsolve(Lo.tocsc(), R)
    before = ctx.lockstep_groups()
    V, info = solver.solve_system(Lo, R)
    # 6 load cases + 5 regulator columns = 11 reduced solves: ONE group of eight and three single ones.  Regulator columns
    # per load case would be 6 x (1 + 5): six groups
    assert ctx.lockstep_groups() - before == 1
    for j in range(k):
        assert np.abs(V[:n_pot, j] - V_ref[:n_pot, j]).max() <= REL_TOL * np.abs(V_ref[:n_pot, j]).max()
        assert np.abs(V[n_pot:, j] - V_ref[n_pot:, j]).max() <= 1e-7 * np.abs(V_ref[n_pot:, j]).max()
        assert info.residual_norms[j] < 1e-9
    assert len(set(np.round(V[n_pot:n_pot + 5].ravel(), 6))) > 5          # the load cases really differ


@pytest.mark.parametrize("name", ["voltage_source", "two_layer_via"])
def test_block_on_a_bare_lil_matrix(ctx, name):
    g = H.load_golden(name)
    Lh = H.golden_L(g)
    r = np.asarray(g["r"], dtype=np.float64)
    from padne_amd.reduction import infer_layout
    layout = infer_layout(Lh, r)
    R = load_cases(r, layout, seed=1)
    V, info = solver.solve_system(Lh.tolil(), R)
    check_block(Lh, R, V, info, layout.n_potential)
    Vf, _ = solver.solve_system(Lh.tolil(), np.asfortranarray(R))        # any memory order of the block
    assert np.array_equal(Vf, V)


@pytest.mark.parametrize("k", [1, 3, 8, 11])
def test_system_matrix_times_a_block(ctx, k):
    g = H.load_golden("two_layer_via")
    meshes, sig, stamps, r, n_pot = H.product_system(g)
    L = solver.assemble_from_arrays(meshes, sig, stamps, n_pot)
    X = np.random.default_rng(k).uniform(-1, 1, (L.shape[0], k))
    Y = L @ X
    assert Y.shape == (L.shape[0], k)
    for j in range(k):
        assert np.array_equal(Y[:, j], L @ X[:, j])
    L.close()

"""tests/kkt_ref.py held to something that is neither the device nor padne_amd.reduction (no GPU): on three small KKT systems
of the oracle's assemble_system the reference's A_ref, b_ref, b_extra and probes are carried through to a full solution --
the reduced solves by dense_ref.refined_solver, the multipliers peeled from rho_ref by hand -- and that solution has to satisfy
the ORIGINAL system L V = r to 2^-55 and every constraint row.  A reference with a wrong map, sign, known part or probe row
cannot get there.  The eliminated / tied / known lists of the three systems are written out by hand below.

Then the bounds of tests/test_kkt_plan_vs_reference.py (they are theorems about any float64 evaluation): a plain float64 numpy
restatement of b, of the probes and of the residual norms has to stay inside them -- which confirms that they were written
down correctly, and shows how much room a float64 evaluation leaves (printed with -s)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import dense_ref
import kkt_ref as K
from oracle import padne_oracle as O
from padne_amd import synthetic

LD = np.longdouble
U = 2.0 ** -53
SIGMA = 2082.5


def grid():
    xy, tri = synthetic.jittered_grid(12, 10, seed=4)
    return [(xy, tri, SIGMA)], len(xy)


@functools.lru_cache(maxsize=None)
def system(name):
    """(L, r, n_potential, elim, tied, known, constraints [(multiplier, p, n, U)], ground vertex, regulators
    [(multiplier, {row: gain})])."""
    meshes, nv = grid()
    if name == "source_to_ground":
        els = [("V", 37, 0, 1.5, nv), ("I", 5, 100, 2.0), ("R", 20, 90, 0.3)]
        L, r = O.assemble_system(meshes, 0, els, 0)
        return L, r, nv, [0, 37], [], {37: 1.5}, [(nv, 37, 0, 1.5)], 0, []
    if name == "floating_chain":
        a, b, c, d = 50, 17, 88, 64
        u1, u2, u3 = 0.75, -1.25, 0.5          # (dyadic: the known parts are exact sums)
        els = [("V", a, b, u1, nv), ("V", b, c, u2, nv + 1), ("V", c, d, u3, nv + 2), ("I", 9, 111, 1.0), ("I", 60, 2, -0.5)]
        L, r = O.assemble_system(meshes, 0, els, 3)
        # representative = the smallest member (17); v_a = v_b + u1, v_c = v_b - u2, v_d = v_c - u3
        known = {a: u1, c: -u2, d: -u2 - u3}
        return (L, r, nv, [3, a, d, c], [(a, b), (d, b), (c, b)], known,
                [(nv, a, b, u1), (nv + 1, b, c, u2), (nv + 2, c, d, u3)], 3, [])
    if name == "regulator":
        vp, vn, sf, st = 40, 71, 15, 99
        els = [("V", 110, 6, 3.3, nv), ("REG", vp, vn, sf, st, 0.75, 0.5, nv + 1), ("I", 30, 80, 1.5), ("R", 22, 101, 0.05)]
        L, r = O.assemble_system(meshes, 0, els, 6)
        return (L, r, nv, [6, vn, 110], [(vn, vp)], {110: 3.3, vn: -0.75}, [(nv, 110, 6, 3.3), (nv + 1, vp, vn, 0.75)], 6,
                [(nv + 1, {sf: 0.5, st: -0.5})])
    raise KeyError(name)


NAMES = ["source_to_ground", "floating_chain", "regulator"]


def reduced_solver(ref):
    """B -> A_ref^-1 B in longdouble: dense_ref.refined_solver on A_ref rounded to float64, refined against A_ref itself."""
    t, u, val, _, _ = ref.reduced_matrix()
    A = np.zeros((ref.n_free, ref.n_free), dtype=LD)
    A[t, u] = val
    A = (A + A.T) / 2                                      # (the two triangles are the same sums in another order)
    inner = dense_ref.refined_solver(np.float64(A))

    def solve(B):
        B = np.asarray(B, dtype=LD).reshape(ref.n_free, -1)
        Y = inner(B)
        for _ in range(4):
            res = B - A @ Y
            if not np.abs(res).max(axis=0).min() > 0:
                break
            Y = Y + inner(res)
        return Y
    return solve


def peel(constraints, ground, rho):
    """Multiplier currents {multiplier: i} from the KCL residuals rho {potential: value}: row p of a source reads +i, row n
    reads -i, the ground vertex also carries the ground row's current.  Leaves first; the ground vertex is never a leaf."""
    rho = dict(rho)
    left, out = list(constraints), {}
    while left:
        degree = {}
        for _, p, n, _ in left:
            degree[p] = degree.get(p, 0) + 1
            degree[n] = degree.get(n, 0) + 1
        for cst in left:
            idx, p, n, _ = cst
            leaf = p if degree[p] == 1 and p != ground else n if degree[n] == 1 and n != ground else None
            if leaf is None:
                continue
            sign = 1 if leaf == p else -1
            out[idx] = rho[leaf] * sign
            other = n if leaf == p else p
            rho[other] = rho[other] + sign * out[idx]
            rho[leaf] = LD(0)
            left.remove(cst)
            break
        else:
            raise AssertionError("the constraints are no forest")
    return out, rho


@functools.lru_cache(maxsize=None)
def solved(name):
    L, r, n_pot, elim, tied, known, cons, ground, regs = system(name)
    N = L.shape[0]
    ref = K.Reference(L, n_pot, sorted(elim), tied)
    kidx = np.array(sorted(known), dtype=np.int64)
    c = ref.known(kidx, np.array([[known[int(i)] for i in kidx]]), 1)
    b, _ = ref.rhs(r, c)
    solve = reduced_solver(ref)
    members = sorted({x for _, p, n, _ in cons for x in (p, n)} | {ground})
    V0 = c + ref.expand(solve(b))
    rho0, _ = ref.probes(r, V0, members)
    V = V0.copy()
    extras = [g for _, g in regs]
    if regs:
        # y = y0 + sum_k i_k z_k with A z_k = P^T gamma_k; rho(i) = rho0 - sum_k i_k (L Z_k); the regulator currents close
        # the k x k system  i = F(rho(i))  (here F is linear: peel twice)
        Z = ref.expand(solve(ref.extra_rhs(extras)))
        LZ, _ = ref.extra_probes(Z, members)
        keys = [idx for idx, _ in regs]

        def currents(i_vec):
            rho = {x: rho0[q, 0] - sum(i_vec[k] * LZ[q, k] for k in range(len(regs))) for q, x in enumerate(members)}
            for k, (_, gamma) in enumerate(regs):
                for row, g in gamma.items():
                    if row in rho:
                        rho[row] = rho[row] - LD(g) * i_vec[k]
            return peel(cons, ground, rho)
        F0 = np.array([currents(np.zeros(len(regs), LD))[0][q] for q in keys], dtype=LD)
        J = np.zeros((len(regs), len(regs)), dtype=LD)
        for k in range(len(regs)):
            e = np.zeros(len(regs), LD)
            e[k] = 1
            J[:, k] = np.array([currents(e)[0][q] for q in keys], dtype=LD) - F0
        M = np.eye(len(regs), dtype=LD) - J
        assert len(regs) == 1
        i_reg = F0 / M[0, 0]
        V = V + Z @ i_reg.reshape(-1, 1)
        mult, rest = currents(i_reg)
    else:
        mult, rest = peel(cons, ground, {x: rho0[q, 0] for q, x in enumerate(members)})
    for idx, val in mult.items():
        V[idx, 0] = val
    V[N - 1, 0] = rest[ground]                             # the ground row's current: L[ground, N - 1] = 1
    return ref, c, kidx, b, members, extras, V0, V


@pytest.mark.parametrize("name", NAMES)
def test_reference_carried_through_solves_the_original_system(name):
    L, r, n_pot, elim, tied, known, cons, ground, regs = system(name)
    assert L.shape[0] <= 400
    ref, c, kidx, b, members, extras, V0, V = solved(name)
    assert ref.n_free == n_pot - len(elim)
    res = np.abs(ref.matmul(V)[:, 0] - r.astype(LD)).max()
    norm_L = np.abs(L).sum(axis=1).max()
    bound = 2.0 ** -55 * (norm_L * np.abs(V).max() + np.abs(r).max())
    print(f"RATIO host residual {name} {float(res / bound):.3g}")
    assert res <= bound
    for idx, p, n, volt in cons:
        assert abs(V[p, 0] - V[n, 0] - LD(volt)) <= 2 * np.finfo(LD).eps * (abs(V[p, 0]) + abs(V[n, 0]) + abs(volt))
    assert V[ground, 0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_index_map_is_a_bijection_with_members_on_their_representative(name):
    L, r, n_pot, elim, tied, known, cons, ground, regs = system(name)
    imap = K.index_map(L.shape[0], n_pot, sorted(elim), tied)
    members = {m for m, _ in tied}
    assert (imap[n_pot:] == -1).all() and all(imap[e] == -1 for e in elim if e not in members)
    own = [i for i in range(n_pot) if i not in elim]
    assert imap[own].tolist() == list(range(len(own)))
    assert all(imap[m] == imap[rep] >= 0 for m, rep in tied)


@pytest.mark.parametrize("name", NAMES)
def test_float64_restatement_stays_inside_the_bounds(name):
    L, r, n_pot, elim, tied, known, cons, ground, regs = system(name)
    ref, c, kidx, b, members, extras, V0, V = solved(name)
    N = L.shape[0]
    rows = np.flatnonzero(ref.imap >= 0)
    P = sp.csr_matrix((np.ones(len(rows)), (rows, ref.imap[rows])), shape=(N, ref.n_free))
    c64 = np.float64(c[:, 0])
    b_ref, b_bound = ref.rhs(r, c)
    b64 = -(P.T @ (r - L @ c64))
    print(f"RATIO host b {name} {K.worst_ratio(b64 - b_ref[:, 0], b_bound[:, 0]):.3g}")
    assert (np.abs(b64 - b_ref[:, 0]) <= b_bound[:, 0]).all()
    V64 = np.float64(V0[:, 0])
    rho_ref, rho_bound = ref.probes(r, V64, members)
    rho64 = (r - L @ V64)[members]
    print(f"RATIO host probes {name} {K.worst_ratio(rho64 - rho_ref[:, 0], rho_bound[:, 0]):.3g}")
    assert (np.abs(rho64 - rho_ref[:, 0]) <= rho_bound[:, 0]).all()
    if extras:
        Z64 = np.float64(ref.expand(reduced_solver(ref)(ref.extra_rhs(extras))))
        lz_ref, lz_bound = ref.extra_probes(Z64, members)
        assert (np.abs((L @ Z64)[members] - lz_ref) <= lz_bound).all()
    Vf = np.float64(V[:, 0])
    norm_ref, norm_bound = ref.residual_norms(r, Vf)
    norm64 = np.linalg.norm(L @ Vf - r)
    print(f"RATIO host norm {name} {float(abs(norm64 - norm_ref[0]) / norm_bound[0]):.3g}")
    assert abs(norm64 - norm_ref[0]) <= norm_bound[0]


def test_layout_restates_the_groups_of_eight():
    assert [K.block_width(n) for n in (1, 2, 3, 4, 5, 7, 8, 9, 11, 16, 17)] == [1, 2, 4, 4, 8, 8, 8, 9, 12, 16, 17]
    N = 5
    for n_cols in (1, 3, 8, 11, 17):
        seen = np.concatenate([K.gidx(N, n_cols, j, np.arange(N)) for j in range(n_cols)])
        assert len(set(seen.tolist())) == N * n_cols and seen.max() < N * K.block_width(n_cols)
    assert K.gidx(N, 11, 9, 2) == 8 * N + 2 * 4 + 1
    flat = np.arange(N * K.block_width(11), dtype=np.float64)
    assert K.from_layout(flat, N, 11)[2, 9] == 8 * N + 2 * 4 + 1 and len(K.spare_entries(flat, N, 11)) == N


def test_reference_does_not_lean_on_the_reduction_module():
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "kkt_ref.py")).read()
    assert "import reduction" not in text and "from padne_amd" not in text and "import padne_amd" not in text

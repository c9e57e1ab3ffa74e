"""Host half of the sensitivities (no GPU; scipy stands in for the device solve): the refusals that come before the device,
the Woodbury combination of the block against a solve with M^T, and every element formula and the face formula against
central differences of the direct solve."""
import types

import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H
import sensitivity_ref as S
from padne_amd import _hip, mesh, problem, solver


def fixture_board(name):
    g = H.load_golden(name)
    prob, ids, flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    return prob, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms], flat


def _refused(prob, meshes, layer_of, objectives, match, partition=None):
    with pytest.raises(ValueError, match=match):
        solver.solve_meshed_sensitivities(prob, meshes, layer_of, objectives, partition=partition)


def test_invalid_objectives_are_refused_before_the_device(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    prob, meshes, layer_of, flat = fixture_board("problem_mixed")
    vs = next(e for e in flat if solver.element_kind(e) == "VoltageSource")
    cur = next(e for e in flat if solver.element_kind(e) == "CurrentSource")
    stranger = problem.NodeID()
    _refused(prob, meshes, layer_of, [], "no objectives")
    _refused(prob, meshes, layer_of, (vs.p, vs.n), "pair")                      # one pair, not a list of pairs
    _refused(prob, meshes, layer_of, [(vs.p, vs.n, cur.f)], "pair")
    _refused(prob, meshes, layer_of, [vs.p], "pair")
    _refused(prob, meshes, layer_of, ["pn"], "pair")
    _refused(prob, meshes, layer_of, [(vs.p, 3)], "NodeID")
    _refused(prob, meshes, layer_of, [(vs.p, vs.p)], "p is n")
    _refused(prob, meshes, layer_of, [(vs.p, stranger)], "not a node of the solved networks")
    _refused(prob, meshes, layer_of, [(vs.p, cur.f)], "different networks")
    _refused(prob, meshes, layer_of, [(vs.p, vs.n)], "row-partitioned", partition=types.SimpleNamespace(world=2, rank=0))
    # a node of a network that is not among the solved ones
    others = [n for n in prob.networks if vs not in n.elements]
    with pytest.raises(ValueError, match="not a node of the solved networks"):
        solver.solve_meshed_sensitivities(prob, meshes, layer_of, [(vs.p, vs.n)], filtered_networks=others)
    with pytest.raises(ValueError, match="no objectives"):
        solver.solve_sensitivities(prob, [], mesher=object())
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_sensitivities(prob, [(vs.p, vs.n)], mesher=object(), partition=types.SimpleNamespace(world=2, rank=0))
    assert solver.check_objectives(prob, [(vs.p, vs.n), [cur.f, cur.t]]) == [(vs.p, vs.n), (cur.f, cur.t)]


def dense_block(system, objective_rows, terms, N):
    """The block of sensitivity_block_columns, dense, by its definition."""
    k, K = len(objective_rows), len(terms)
    _, r = system.assemble()
    R = np.zeros((N, solver.sensitivity_block_columns(k, K)))
    R[:, 0] = r
    for j, (p, n) in enumerate(objective_rows):
        R[p, 1 + j] += 1.0
        R[n, 1 + j] -= 1.0
    for q, (sf, st, iv, _g) in enumerate(terms):
        R[sf, 1 + k + q] += 1.0
        R[st, 1 + k + q] -= 1.0
        R[iv, 1 + k + K + q] = 1.0
    return R


def test_problem_block_stamps_are_the_definition():
    system = S.problem_system("problem_mixed")
    M, r = system.assemble()
    N = M.shape[0]
    terms = solver.woodbury_terms(system.rows)
    assert len(terms) == 1
    objective_rows = [(3, 40), (system.rows[0][1], system.rows[0][2])]
    rows, cols, vals = solver.stamp_sensitivity_block(list(system.prob.networks), system.nodes, N, objective_rows, terms)
    R = np.zeros((N, solver.sensitivity_block_columns(2, 1)))
    R[rows, cols] = vals
    assert len(set(zip(rows.tolist(), cols.tolist()))) == len(rows)
    assert np.array_equal(R, dense_block(system, objective_rows, terms, N))
    assert np.array_equal(R[:, 0], r)


@pytest.mark.parametrize("name", ["problem_mixed", "regulator"])
def test_woodbury_combination_is_the_transposed_solve(name):
    system = S.problem_system(name) if name.startswith("problem_") else S.unknown_system(name)
    M, _ = system.assemble()
    N = M.shape[0]
    terms = solver.woodbury_terms(system.rows)
    assert terms and not (M - M.T).nnz == 0                                          # a regulator: M is unsymmetric
    n_pot = sum(len(m[0]) for m in system.meshes) + system.n_internal
    rng = np.random.default_rng(3)
    objective_rows = [tuple(int(i) for i in rng.choice(n_pot, 2, replace=False)) for _ in range(3)]
    reg = next(r for r in system.rows if r[0] == "REG")
    objective_rows.append((reg[3], reg[4]))                                           # across the regulator's sense pins
    objective_rows.append((reg[1], reg[2]))
    Y = S.solve(M, dense_block(system, objective_rows, terms, N))
    W = solver.adjoint_weights(Y, len(objective_rows), terms)
    MT = M.T.tocsr()
    cond = np.linalg.cond(M.toarray())
    norm_MT = abs(MT).sum(axis=1).max()
    for j, (p, n) in enumerate(objective_rows):
        c = np.zeros(N)
        c[p] += 1.0
        c[n] -= 1.0
        want = S.adjoint(M, p, n)
        got = Y @ W[j]
        # backward error of the combination: as small as that of the direct transposed solve (1e-12 normwise)
        assert np.abs(MT @ got - c).max() <= 1e-12 * (norm_MT * np.abs(got).max() + 1.0), j
        # forward: two backward-stable solutions agree to ~eps cond(M) only (cond(M) ~6e7 on problem_mixed, ~7e10 on
        # regulator, whose 100 kOhm resistor puts adjoint potentials of 1e5 V/A next to mV/A ones)
        tol = max(1e-12, 1e-15 * cond)
        assert np.abs(got - want).max() <= tol * max(np.abs(want).max(), 1e-300), (j, tol)
    # without the Woodbury columns the weights only select, and the symmetric solve is not the adjoint
    W0 = solver.adjoint_weights(Y[:, :1 + len(objective_rows)], len(objective_rows), [])
    assert np.array_equal(W0, np.eye(len(objective_rows), 1 + len(objective_rows), 1))


def central(f, theta, rel=1e-4):
    h = rel * abs(theta) if theta != 0.0 else rel
    return (f(theta + h) - f(theta - h)) / (2 * h)


def J_of(M, r, p, n):
    x = S.solve(M, r)
    return x[p] - x[n]


# (central differences with a relative step of 1e-4 resolve a derivative to about eps cond(M) |x| / 1e-4: the regulator
#  fixture, cond(M) ~7e10, is left to the Woodbury test above; problem_mixed carries a regulator with cond(M) ~6e7)
FD_TOL = 1e-5


@pytest.mark.parametrize("name", ["voltage_source", "star", "two_layer_via", "lumped_only", "glue_sources", "problem_mixed",
                                  "problem_simple_trace"])
def test_element_formulas_match_central_differences(name):
    system = S.problem_system(name) if name.startswith("problem_") else S.unknown_system(name)
    M, r = system.assemble()
    n_pot = sum(len(m[0]) for m in system.meshes) + system.n_internal
    p, n = n_pot - 1, 0
    x = S.solve(M, r)
    lam = S.adjoint(M, p, n)
    got = solver.element_sensitivities(system.rows, x, lam)
    fields = {"R": {"resistance": 3}, "I": {"current": 3}, "V": {"voltage": 3}, "REG": {"voltage": 5, "gain": 6}}
    scale = max(abs(v) for d in got for v in d.values())
    assert scale > 0
    for e, row in enumerate(system.rows):
        assert sorted(got[e]) == sorted(fields[row[0]])
        for name_, pos in fields[row[0]].items():
            def J(theta, e=e, pos=pos):
                rows = list(system.rows)
                rows[e] = rows[e][:pos] + (theta,) + rows[e][pos + 1:]
                Mt, rt = system.assemble(rows)
                return J_of(Mt, rt, p, n)
            fd = central(J, row[pos])
            assert abs(got[e][name_] - fd) <= FD_TOL * max(abs(fd), 1e-3 * scale), (e, row[0], name_, got[e][name_], fd)


@pytest.mark.parametrize("name", ["obtuse", "unit_square", "square_with_hole", "star", "two_layer_via", "problem_mixed"])
def test_face_formula_matches_central_differences(name):
    system = S.problem_system(name) if name.startswith("problem_") else S.unknown_system(name)
    M, r = system.assemble()
    n_vert = sum(len(m[0]) for m in system.meshes)
    p, n = 0, n_vert - 1
    x = S.solve(M, r)
    lam = S.adjoint(M, p, n)
    s = S.face_s(system, x, lam)
    tri, cot, sig, _ = S.faces(system)
    rng = np.random.default_rng(11)
    faces = sorted(set(rng.choice(len(tri), min(len(tri), 8), replace=False).tolist()) | {int(np.argmax(np.abs(s)))})
    scale = np.abs(s).max()
    assert scale > 0
    for t in faces:
        D = S.face_derivative_matrix(system, t)
        fd = central(lambda h: J_of((M + h * D).tocsr(), r, p, n), 0.0, rel=1e-3 * sig[t]) * sig[t]
        assert abs(s[t] - fd) <= FD_TOL * max(abs(fd), 1e-2 * scale), (t, s[t], fd)


def test_obtuse_faces_need_the_cot_weights_not_the_gradient_form():
    system = S.unknown_system("obtuse")
    # the fixture's own load is symmetric about the obtuse corner's bisector, which leaves x equal at the ends of the edge
    # that corner faces; a load from one of those ends breaks the symmetry
    system.rows = [("I", 1, 3, 2.0)]
    M, r = system.assemble()
    x = S.solve(M, r)
    tri = np.concatenate([np.asarray(m[1]) for m in system.meshes])
    xy = np.concatenate([np.asarray(m[0]) for m in system.meshes])
    sigma = system.meshes[0][2]
    # faces with an obtuse corner: the signed cotangent is negative there, the assembly takes its absolute value
    obtuse = sorted({t for t, c in enumerate(tri) for e in range(3)
                     if (xy[c[e]] - xy[c[(e + 2) % 3]]) @ (xy[c[(e + 1) % 3]] - xy[c[(e + 2) % 3]]) < 0})
    assert obtuse
    p, n = 1, 4
    lam = S.adjoint(M, p, n)
    s, grad = S.face_s(system, x, lam), S.face_s_gradient_form(system, x, lam)
    for t in obtuse:
        D = S.face_derivative_matrix(system, t)
        fd = central(lambda h: J_of((M + h * D).tocsr(), r, p, n), 0.0, rel=1e-4 * sigma) * sigma
        assert abs(s[t] - fd) <= 1e-6 * abs(fd), (t, s[t], fd)
        assert abs(grad[t] - fd) > 1e-2 * abs(fd), (t, grad[t], fd)              # the gradient form is wrong here
    acute = [t for t in range(len(tri)) if t not in obtuse]
    assert acute and np.allclose(s[acute], grad[acute], rtol=1e-9, atol=1e-12 * np.abs(s).max())


def test_woodbury_terms_skip_vanishing_gain():
    rows = [("REG", 1, 2, 3, 4, 1.0, 0.0, 9), ("REG", 1, 2, 5, 5, 1.0, 0.7, 10), ("REG", 1, 2, 5, 6, 1.0, -0.5, 11),
            ("R", 1, 2, 3.0)]
    assert solver.woodbury_terms(rows) == [(5, 6, 11, -0.5)]
    assert solver.sensitivity_block_columns(3, 1) == 6


def test_sparse_sanity_of_the_derivative_matrix():
    # dM/dsigma of all faces together is the mesh Laplacian at unit conductance
    system = S.unknown_system("star")
    tri, *_ = S.faces(system)
    total = sum(S.face_derivative_matrix(system, t) for t in range(len(tri)))
    xy, t_, s = system.meshes[0]
    lap = sp.csr_matrix(sp.coo_matrix(S.O.laplace_operator(xy, t_)))
    n = len(xy)
    assert np.allclose(total[:n, :n].toarray(), lap.toarray(), rtol=1e-13, atol=1e-15)

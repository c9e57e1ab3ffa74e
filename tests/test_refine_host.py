"""Host half of the refinement (no GPU): the restatement of tests/refine_ref.py against the properties the rule promises
(conforming, positively oriented, area kept, old vertices kept, marks the least fixed point, angles bounded), so that the
device tests compare against something that is itself checked; and the refusals that come before the device."""
import types

import numpy as np
import pytest

import helpers as H
import refine_ref as RR
from padne_amd import _hip, mesh, problem, solver, synthetic

SMALL_SETS = ["square", "grid", "annulus"]
MESH_SETS = SMALL_SETS + H.problem_golden_names()
FLAG_RATE = 0.15
EPS = np.finfo(np.float64).eps


def mesh_set(name):
    """[(points, triangles)] of a named set: a two-face square, a jittered grid, an annulus (a hole), a golden board's
    meshes (34 islands in one of them, islands with holes in others)."""
    if name == "square":
        return [(np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]), np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32))]
    if name == "grid":
        return [synthetic.jittered_grid(9, 7)]
    if name == "annulus":
        return [synthetic.annulus_mesh(1.0, 2.0, 5, 24)]
    return [(xy, tri) for xy, tri, _ in H.problem_meshes(H.load_golden(name))]


def random_flags(meshes, seed):
    """About 15 % of the faces of every mesh; at least one face of the set (the square has two)."""
    rng = np.random.default_rng(seed)
    flags = [rng.random(len(t)) < FLAG_RATE for _, t in meshes]
    if not any(f.any() for f in flags):
        flags[0][rng.integers(len(flags[0]))] = True
    return flags


def area_slack(points, triangles):
    """What rounding may do to a face's area formed from coordinates that are themselves rounded: every coordinate of a
    midpoint carries half an ulp of its size X, the differences and products of the cross product an ulp each of theirs, so
    the area moves by a few EPS * X * L with L the face's longest edge.  (Relative to the area itself that is EPS * X / h:
    "a few ulp" only for a mesh at the origin.)  Per face: EPS * (largest |coordinate| of the face) * (its longest edge)."""
    p, t = np.asarray(points), np.asarray(triangles)
    c = p[t]
    X = np.abs(c).max(axis=(1, 2))
    L = np.sqrt(((c - np.roll(c, 1, axis=1)) ** 2).sum(axis=2)).max(axis=1)
    return EPS * X * L


AREA_ULPS = 8      # three children's areas and the parent's, two rounded coordinates per new vertex: see area_slack


def check_round(before, flags, R):
    """Every property of one round ``R`` = refine(before, flags)."""
    E = R.edges
    xy0, tri0, voff0, toff0 = RR.flatten(before)
    # conforming: every directed edge once, every undirected edge at most twice (edges_of raises otherwise)
    xy1, tri1, voff1, toff1 = RR.flatten(R.meshes)
    E1 = RR.edges_of(xy1, tri1)
    worst = 0.0
    for (p0, t0), (p1, t1), par, ends in zip(before, R.meshes, R.parents, R.midpoint_ends):
        # old vertices unchanged, new ones the midpoints of their ends
        assert np.array_equal(p1[:len(p0)], p0)
        assert len(ends) == len(p1) - len(p0) and (ends[:, 0] < ends[:, 1]).all() and (ends < len(p0)).all()
        assert np.array_equal(p1[len(p0):], 0.5 * (p0[ends[:, 0]] + p0[ends[:, 1]]))
        if not len(t0):
            assert not len(t1)
            continue
        a1 = RR.signed_areas(p1, t1)
        assert (a1 > 0).all()                                           # every child keeps the parent's winding
        assert (np.diff(par) >= 0).all() and par[0] == 0 and par[-1] == len(t0) - 1      # children in parent order
        a0 = RR.signed_areas(p0, t0)
        summed = np.bincount(par, weights=a1, minlength=len(t0))
        slack = area_slack(p0, t0)
        worst = max(worst, float((np.abs(summed - a0) / slack).max()))
        assert (np.abs(summed - a0) <= AREA_ULPS * slack).all()
    # the boundary grows by the marked boundary edges, the vertices by the marked edges
    assert (E1.uses == 1).sum() == (E.uses == 1).sum() + (R.marks & (E.uses == 1)).sum()
    assert len(xy1) == len(xy0) + R.marks.sum() and len(E1.lo) == len(E.lo) + R.marks.sum() + (len(tri1) - len(tri0))
    # the marks: the flagged faces' edges, a fixed point, and the least one (a second sweep order gives the same)
    flag = np.concatenate(flags)
    assert R.marks[E.of_face[flag]].all() and (R.marks >= R.marks_flagged).all()
    rows = np.arange(len(tri0))
    assert not (R.marks[E.of_face].any(axis=1) & ~R.marks[E.of_face[rows, E.longest]]).any()
    assert np.array_equal(RR.close_marks_worklist(E, R.marks_flagged), R.marks)
    return worst


@pytest.fixture(scope="module")
def rounds():
    """name -> [(before, flags, Refined)] for four successive rounds at about 15 % flags."""
    out = {}
    for k, name in enumerate(MESH_SETS):
        cur, chain = mesh_set(name), []
        for r in range(4):
            flags = random_flags(cur, 100 * k + r)
            R = RR.refine(cur, flags)
            chain.append((cur, flags, R))
            cur = R.meshes
        out[name] = chain
    return out


@pytest.mark.parametrize("name", MESH_SETS)
def test_one_round_and_four_successive_rounds(rounds, name):
    for r, (before, flags, R) in enumerate(rounds[name]):
        worst = check_round(before, flags, R)
        print(name, "round", r + 1, sum(len(t) for _, t in before), "->", sum(len(t) for _, t in R.meshes), "faces,",
              int(R.marks.sum() - R.marks_flagged.sum()), "edges from the closure in", R.sweeps, "sweeps; areas off by", worst,
              "of EPS X L")
        assert any(f.any() for f in flags)


@pytest.mark.parametrize("name", MESH_SETS)
def test_the_smallest_angle_keeps_half_of_itself(rounds, name):
    """The known bound of this partition (Rosenberg and Stenger; Rivara): no angle of a descendant is below half the
    smallest angle of its ancestor.  Measured 0.90 (annulus), 0.92 (jittered grid) and 1 - 1e-12 or more on the boards."""
    first, last = rounds[name][0][0], rounds[name][-1][2].meshes
    a0 = min(RR.smallest_angle(p, t) for p, t in first if len(t))
    a1 = min(RR.smallest_angle(p, t) for p, t in last if len(t))
    print(name, "smallest angle", a0, "->", a1, "ratio", a1 / a0)
    assert a1 >= 0.5 * a0


@pytest.mark.parametrize("name", MESH_SETS)
def test_no_flags_and_all_flags(name):
    ms = mesh_set(name)
    none = RR.refine(ms, [np.zeros(len(t), dtype=bool) for _, t in ms])
    for (p0, t0), (p1, t1), par, ends in zip(ms, none.meshes, none.parents, none.midpoint_ends):
        assert np.array_equal(p0, p1) and np.array_equal(t0, t1) and np.array_equal(par, np.arange(len(t0))) and not len(ends)
    assert none.sweeps == 0 and not none.marks.any()
    every = RR.refine(ms, [np.ones(len(t), dtype=bool) for _, t in ms])
    assert every.marks.all() and every.sweeps == 0
    assert sum(len(p) for p, _ in every.meshes) == sum(len(p) for p, _ in ms) + len(every.edges.lo)
    for (_, t0), (_, t1), par in zip(ms, every.meshes, every.parents):
        assert len(t1) == 4 * len(t0) and np.array_equal(par, np.repeat(np.arange(len(t0)), 4))
    check_round(ms, [np.ones(len(t), dtype=bool) for _, t in ms], every)


def test_a_tie_goes_to_the_lower_edge_number():
    """Corners (0, 0), (2, 0), (1, 4): edges (0, 1) of d = 4 and (0, 2), (1, 2) of d = 17 each.  (0, 2) has the lower key, so
    it is the longest edge: corner 2, a = vertex 2, b = vertex 0, c = vertex 1."""
    pts = np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 4.0]])
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    E = RR.edges_of(pts, tri.astype(np.int64))
    assert list(zip(E.lo, E.hi)) == [(0, 1), (0, 2), (1, 2)] and list(E.d) == [4.0, 17.0, 17.0]
    assert E.longest[0] == 2 and E.of_face[0, 2] == 1
    R = RR.refine([(pts, tri)], [np.array([True])])
    # new vertices 3, 4, 5 halve (0, 1), (0, 2), (1, 2): m = 4, p = 3 (of bc = (0, 1)), q = 5 (of ca = (1, 2))
    assert R.meshes[0][1].tolist() == [[2, 4, 5], [5, 4, 1], [4, 0, 3], [4, 3, 1]]
    assert R.midpoint_ends[0].tolist() == [[0, 1], [0, 2], [1, 2]]
    # closure: with the face unflagged but its shortest edge halved by a neighbour, the longest must follow
    both = (np.array([[0.0, 0.0], [2.0, 0.0], [1.0, 4.0], [1.0, -0.5]]), np.array([[0, 1, 2], [1, 0, 3]], dtype=np.int32))
    R = RR.refine([both], [np.array([False, True])])
    assert R.marks.sum() - R.marks_flagged.sum() == 1 and R.sweeps == 1
    assert (R.parents[0] == 0).sum() == 3 and (R.parents[0] == 1).sum() == 4


def test_what_the_restatement_refuses():
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.5, -1.0]])
    with pytest.raises(ValueError, match="Non-manifold"):              # three faces on the edge (0, 1)
        RR.refine([(pts, np.array([[0, 1, 2], [1, 0, 4], [0, 1, 3]]))], [np.zeros(3, dtype=bool)])
    with pytest.raises(ValueError, match="Non-manifold"):              # the edge (0, 1) twice in the same direction
        RR.refine([(pts, np.array([[0, 1, 2], [0, 1, 3]]))], [np.zeros(2, dtype=bool)])
    with pytest.raises(ValueError, match="twice"):
        RR.refine([(pts, np.array([[0, 1, 1]]))], [np.zeros(1, dtype=bool)])


# ---- the refusals that come before the device -----------------------------------------------------------------------

def no_device(*_a, **_k):
    raise AssertionError("the device was reached")


def fixture_board(name):
    g = H.load_golden(name)
    prob, _ids, _flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    return prob, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms]


def test_refine_meshes_refuses_bad_flags_before_the_device(monkeypatch):
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    monkeypatch.setattr(_hip, "refine", no_device)
    _prob, meshes, _ = fixture_board("problem_mixed")
    good = [np.zeros(len(m.triangles), dtype=bool) for m in meshes]
    with pytest.raises(ValueError, match="one array per mesh"):
        solver.refine_meshes(meshes, good[:1])
    with pytest.raises(ValueError, match="one array per mesh"):
        solver.refine_meshes(meshes, good + good[:1])
    with pytest.raises(ValueError, match="one array per mesh"):
        solver.refine_meshes(meshes, None)
    with pytest.raises(ValueError, match="one entry per face"):
        solver.refine_meshes(meshes, [good[0][:-1], good[1]])
    with pytest.raises(ValueError, match="one entry per face"):
        solver.refine_meshes(meshes, [good[0], good[1].reshape(1, -1)])
    for bad in (good[0].astype(np.uint8), good[0].astype(np.int64), good[0].astype(np.float64), [0] * len(good[0])):
        with pytest.raises(ValueError, match="boolean"):
            solver.refine_meshes(meshes, [bad, good[1]])
    # meshes without faces pass through without the device
    lone = [mesh.Mesh(np.array([[0.0, 0.0], [1.0, 1.0]]), np.zeros((0, 3), dtype=np.int32)), mesh.Mesh()]
    out = solver.refine_meshes(lone, [np.zeros(0, dtype=bool)] * 2)
    assert np.array_equal(out.meshes[0].points, lone[0].points) and out.meshes[0] is not lone[0] and not len(out.meshes[1].points)
    assert [len(p) for p in out.parents] == [0, 0] and [e.shape for e in out.midpoint_ends] == [(0, 2), (0, 2)]
    assert solver.refine_meshes([], []).meshes == []


ADAPTIVE_BAD = [dict(tolerance=None), dict(tolerance=0), dict(tolerance=1.0), dict(tolerance=True), dict(tolerance="0.1"),
                dict(tolerance=np.nan), dict(max_rounds=0), dict(max_rounds=-1), dict(max_rounds=2.5), dict(max_rounds=True),
                dict(max_rounds=None), dict(max_faces=0), dict(max_faces=1.5), dict(max_faces=False), dict(min_size=-1e-9),
                dict(min_size=np.nan), dict(min_size=np.inf), dict(min_size="1"), dict(min_size=None), dict(min_size=True)]


@pytest.mark.parametrize("bad", ADAPTIVE_BAD, ids=[str(b) for b in ADAPTIVE_BAD])
def test_adaptive_arguments_are_refused_before_the_first_solve(monkeypatch, bad):
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    monkeypatch.setattr(solver, "solve_meshed_error", no_device)
    prob, meshes, layer_of = fixture_board("problem_mixed")
    kwargs = dict(tolerance=0.1)
    kwargs.update(bad)
    what = next(iter(bad))
    with pytest.raises(ValueError, match=what):
        solver.solve_meshed_adaptive(prob, meshes, layer_of, **kwargs)
    with pytest.raises(ValueError, match=what):
        solver.solve_adaptive(prob, mesher=object(), **kwargs)


def test_valid_adaptive_arguments_and_the_partition_refusal(monkeypatch):
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    monkeypatch.setattr(solver, "solve_meshed_error", no_device)
    assert solver.check_adaptive_arguments(0.05, 8, None, 0.0) == (0.05, 8, None, 0.0)
    assert solver.check_adaptive_arguments(np.float32(0.5), np.int64(1), np.int32(7), 1) == (0.5, 1, 7, 1.0)
    prob, meshes, layer_of = fixture_board("problem_mixed")
    several = types.SimpleNamespace(world=2, rank=0)
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_meshed_adaptive(prob, meshes, layer_of, tolerance=0.1, partition=several)
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_adaptive(prob, tolerance=0.1, mesher=object(), partition=several)
    with pytest.raises(TypeError):                                       # the tolerance is not optional
        solver.solve_meshed_adaptive(prob, meshes, layer_of)


def test_the_records_have_the_fields_of_the_issue():
    names = [f.name for f in solver.dataclasses.fields(solver.Refinement)]
    assert names[:3] == ["meshes", "parents", "midpoint_ends"]
    names = [f.name for f in solver.dataclasses.fields(solver.AdaptiveHistory)]
    assert names == ["faces", "vertices", "estimates", "flagged", "closure_edges", "reason", "meshes"]

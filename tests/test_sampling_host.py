"""Host half of the field sampler (no GPU): the refusals that come before the device, the restatement of the owner rule
(tests/sampling_ref.py) against exact rational arithmetic and against the other restatements on the small fixtures, and the
no-gaps property of the rule on a jittered grid."""
from fractions import Fraction

import numpy as np
import pytest

import currents_ref as C
import helpers as H
import sampling_ref as R
import sensitivity_ref as S
from oracle import padne_oracle as O
from padne_amd import _hip, problem, solver, synthetic

FIXTURES = ["unit_square", "square_with_hole", "obtuse", "star"]


class NoDevice:
    """Stands where ``_hip.Sampler`` is: it can be made, but nothing may be asked of it."""

    def __init__(self, *_a, **_k):
        pass

    def __getattr__(self, name):
        if name == "close":
            return lambda: None
        raise AssertionError("the device was reached")


def test_invalid_queries_are_refused_before_the_device(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(solver, "get_context", lambda: None)
    monkeypatch.setattr(_hip, "Context", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    monkeypatch.setattr(_hip, "Sampler", NoDevice)
    g = H.load_golden("problem_mixed")
    prob, _ids, _flat = H.build_problem(g, problem)
    sol = solver.Solution(problem=prob, layer_solutions=[solver.LayerSolution(meshes=[], potentials=[]) for _ in prob.layers],
                          solver_info=solver.SolverInfo(0.0, 0.0))
    top = prob.layers[0]
    stranger = problem.Layer(shape=H.Geoms(1), name=top.name, conductance=top.conductance)
    with solver.FieldSampler(sol) as fs:
        def refused(match, call, *args):
            with pytest.raises(ValueError, match=match):
                call(*args)
        refused("not one of the Problem's layers", fs.points, stranger, [[0.0, 0.0]])
        refused("not one of the Problem's layers", fs.line, stranger, (0, 0), (1, 1), 5)
        refused("not one of the Problem's layers", fs.raster, stranger, (0, 0), 0.1, 4, 4)
        refused(r"shape \(n, 2\)", fs.points, top, [0.0, 1.0])
        refused(r"shape \(n, 2\)", fs.points, top, np.zeros((4, 3)))
        refused(r"\(n, 2\) array of numbers", fs.points, top, [["a", "b"]])
        refused("not finite", fs.points, top, [[0.0, np.nan]])
        refused("not finite", fs.points, top, [[np.inf, 0.0], [1.0, 1.0]])
        refused("not finite", fs.line, top, (0, 0), (np.inf, 1), 5)
        refused("at least 2 points", fs.line, top, (0, 0), (1, 1), 1)
        refused("at least 2 points", fs.line, top, (0, 0), (1, 1), 2.5)
        refused("finite and positive", fs.raster, top, (0, 0), 0.0, 4, 4)
        refused("finite and positive", fs.raster, top, (0, 0), (0.1, -0.1), 4, 4)
        refused("finite and positive", fs.raster, top, (0, 0), np.inf, 4, 4)
        refused("finite and positive", fs.raster, top, (0, 0), (np.nan, 1.0), 4, 4)
        refused("one number or", fs.raster, top, (0, 0), (1.0, 1.0, 1.0), 4, 4)
        refused("at least one pixel", fs.raster, top, (0, 0), 0.1, 0, 4)
        refused("at least one pixel", fs.raster, top, (0, 0), 0.1, 4, -1)
        refused("must be integers", fs.raster, top, (0, 0), 0.1, 4.5, 4)
        refused("not finite", fs.raster, top, (np.nan, 0), 0.1, 4, 4)
        refused("pixel centres are not finite", fs.raster, top, (1e308, 0), 1e306, 1000, 4)
        refused(f"at most {solver.MAX_RASTER_PIXELS}", fs.raster, top, (0, 0), 0.1, 2 ** 13, 2 ** 13 + 1)
        refused(f"at most {solver.MAX_SAMPLE_POINTS}", fs.line, top, (0, 0), (1, 1), solver.MAX_SAMPLE_POINTS + 1)
        # (a view of one point repeated: no 1 GiB array is made for the check)
        many = np.broadcast_to(np.zeros((1, 2)), (solver.MAX_SAMPLE_POINTS + 1, 2))
        with pytest.raises(ValueError, match=f"at most {solver.MAX_SAMPLE_POINTS}"):
            fs.points(top, many)
    with pytest.raises(ValueError, match="closed"):
        fs.points(top, [[0.0, 0.0]])
    fs.close()                                                            # closing twice is harmless
    assert solver.MAX_RASTER_PIXELS == 2 ** 26 and solver.MAX_SAMPLE_POINTS == 2 ** 26
    assert solver.check_raster(prob, prob.layers[1], H.XY(1, 2), (0.5, 0.25), 8, 4) == (1, 1.0, 2.0, 0.5, 0.25, 8, 4)
    li, pts = solver.check_sample_points(prob, prob.layers[1], [(1, 2), (3, 4)])
    assert li == 1 and pts.dtype == np.float64 and pts.shape == (2, 2)
    li, pts = solver.check_sample_points(prob, top, np.zeros((0, 2)))
    assert li == 0 and pts.shape == (0, 2)


# ---- the restatement against itself --------------------------------------------------------------------------------

def fixture_board(name, potentials=None):
    g = H.load_golden(name)
    ms = H.meshes_of(g)
    pots = [g[f"pot{i}"] for i in range(len(ms))] if potentials is None else potentials
    return g, R.board([(xy, tri, s, layer) for xy, tri, s, layer in ms], pots)


def exact_owner(b, layer, q):
    """The lowest face of the layer that contains q (closed, positive area) in exact rational arithmetic."""
    qx, qy = Fraction(float(q[0])), Fraction(float(q[1]))
    for f in b.faces_of(layer):
        (ax, ay), (bx, by), (cx, cy) = [[Fraction(float(v)) for v in b.xy[k]] for k in b.tri[f]]
        o = [(x2 - x1) * (qy - y1) - (y2 - y1) * (qx - x1) for x1, y1, x2, y2 in
             ((bx, by, cx, cy), (cx, cy, ax, ay), (ax, ay, bx, by))]
        if (all(v >= 0 for v in o) or all(v <= 0 for v in o)) and any(v != 0 for v in o):
            return int(f)
    return -1


@pytest.mark.parametrize("name", FIXTURES)
def test_owner_rule_at_vertices_midpoints_and_centroids(name):
    _g, b = fixture_board(name)
    verts, mids, cent = R.special_points(b, 0)
    faces = b.faces_of(0)
    assert np.array_equal(R.owners(b, 0, cent), faces)                     # a centroid belongs to its own face
    for pts in (verts, mids, cent):
        got = R.owners(b, 0, pts)
        assert (got >= 0).all()
        # these fixtures' coordinates are short binary fractions: the rounded rule is the exact one
        assert got.tolist() == [exact_owner(b, 0, q) for q in pts]
    counts = R.containing_counts(b, 0, np.concatenate([verts, mids, cent]))
    assert (counts[:len(verts)] >= 1).all() and (counts[len(verts):len(verts) + len(mids)] >= 1).all()
    assert (counts[len(verts):len(verts) + len(mids)] <= 2).all() and (counts[-len(cent):] == 1).all()
    # the lowest containing face: every face with a lower index does not contain the point
    got = R.owners(b, 0, mids)
    for q, f in zip(mids, got):
        lower = faces[faces < f]
        assert not R.contains(*R.sides(b, lower, q[None, :])).any()
    far = b.xy.max(axis=0) + 1.0
    assert R.owners(b, 0, far[None, :]).tolist() == [-1] and R.owners(b, 1, cent).tolist() == [-1] * len(cent)


def test_the_inside_of_a_hole_is_outside():
    _g, b = fixture_board("square_with_hole")
    lo, hi = b.xy.min(axis=0), b.xy.max(axis=0)
    centre = (lo + hi) / 2
    assert exact_owner(b, 0, centre) == -1                                 # the fixture's hole is around its centre
    face, V, J, p = R.sample(b, 0, centre[None, :])
    assert face.tolist() == [-1] and np.isnan(V).all() and np.isnan(J).all() and np.isnan(p).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_a_linear_field_is_reproduced(name):
    g = H.load_golden(name)
    xy = g["xy0"]
    a, bb, c = 0.75, -1.25, 3.0
    _g, b = fixture_board(name, [a * xy[:, 0] + bb * xy[:, 1] + c])
    q = R.box_points(b, 0, 4000, seed=3, grow=0.0)
    face, V, _J, _p = R.sample(b, 0, q)
    inside = face >= 0
    assert inside.sum() > 1000
    want = a * q[:, 0] + bb * q[:, 1] + c
    # weights: two additions and a division each, then a product and two additions, on terms of size max |V|; the field
    # itself is rounded at the corners and at q (3 operations each)
    bound = 16 * np.finfo(float).eps * np.abs(b.V).max()
    assert np.abs(V[inside] - want[inside]).max() <= bound
    assert np.isnan(V[~inside]).all()


@pytest.mark.parametrize("name", FIXTURES)
def test_face_values_are_the_other_restatements(name):
    g, b = fixture_board(name)
    system = S.unknown_system(name)
    J_want, _size = C.face_J(system, np.concatenate([g["pot0"], np.zeros(len(g["v"]) - len(g["pot0"]))]))
    p_want = O.power_density(g["xy0"], g["tri0"], g["pot0"], float(g["sigma0"]))
    assert np.array_equal(p_want, g["pow0"])
    _verts, _mids, cent = R.special_points(b, 0)
    face, _V, J, p = R.sample(b, 0, cent)
    assert np.array_equal(face, np.arange(len(cent)))
    assert np.array_equal(J, J_want[face]) and np.array_equal(p, p_want[face])


# ---- no gaps ---------------------------------------------------------------------------------------------------------

def jittered_board(nx=23, ny=17, h=0.25, seed=4):
    xy, tri = synthetic.jittered_grid(nx, ny, h=h, seed=seed, jitter=0.2)
    return R.board([(xy, tri, 2000.0, 0)], [np.zeros(len(xy))])


def test_no_gaps_on_interior_edges_and_inside_the_outline():
    """Every point on an interior edge (as its convex combination rounds) and every point strictly inside the rectangle has
    an owner: rounding on an edge cannot put a point outside both of its faces."""
    b = jittered_board()
    on_edges = R.on_edge_points(b, 0, 100_000, seed=11)
    assert (R.owners(b, 0, on_edges) >= 0).all()
    lo, hi = b.xy.min(axis=0), b.xy.max(axis=0)
    inside = np.random.default_rng(12).uniform(np.nextafter(lo, hi), hi, size=(100_000, 2))
    assert ((inside > lo) & (inside < hi)).all()
    assert (R.owners(b, 0, inside) >= 0).all()
    # the on-edge points do lie on edges: the exact rule, with its rounding, gives a good share of them two faces
    counts = R.containing_counts(b, 0, on_edges[:5000])
    assert (counts >= 1).all() and (counts == 2).sum() > 100

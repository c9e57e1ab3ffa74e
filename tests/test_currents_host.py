"""Host half of the current report (no GPU; scipy stands in for the device solve): the refusals that come before the device,
the element flows and the power balance on solved fixtures, and Kirchhoff's current law through cuts of the restated cut
rule on solved strips."""
import types

import numpy as np
import pytest

import currents_ref as C
import helpers as H
import sensitivity_ref as S
from padne_amd import _hip, mesh, problem, solver, synthetic


def fixture_board(name):
    g = H.load_golden(name)
    prob, ids, flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    return prob, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms], flat


def _refused(prob, meshes, layer_of, cuts, match, partition=None):
    with pytest.raises(ValueError, match=match):
        solver.solve_meshed_currents(prob, meshes, layer_of, cuts, partition=partition)


def test_invalid_cuts_are_refused_before_the_device(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    prob, meshes, layer_of, _flat = fixture_board("problem_mixed")
    top = prob.layers[0]
    stranger = problem.Layer(shape=H.Geoms(1), name=top.name, conductance=top.conductance)
    _refused(prob, meshes, layer_of, [solver.Cut(stranger, (0, 0), (1, 1))], "not one of the Problem's layers")
    _refused(prob, meshes, layer_of, [solver.Cut(top, (0, np.nan), (1, 1))], "not finite")
    _refused(prob, meshes, layer_of, [solver.Cut(top, (0, 0), H.XY(np.inf, 1))], "not finite")
    _refused(prob, meshes, layer_of, [solver.Cut(top, (0, 0), (0.0, 0.0))], "same point")
    _refused(prob, meshes, layer_of, [solver.Cut(top, H.XY(2, 3), (2, 3))], "same point")
    _refused(prob, meshes, layer_of, [solver.Cut(top, (0, 0, 0), (1, 1))], r"\(x, y\)")
    _refused(prob, meshes, layer_of, [solver.Cut(top, "ab", (1, 1))], r"\(x, y\)")
    _refused(prob, meshes, layer_of, [(top, (0, 0), (1, 1))], "not a Cut")
    _refused(prob, meshes, layer_of, solver.Cut(top, (0, 0), (1, 1)), "sequence of Cut")
    _refused(prob, meshes, layer_of, [solver.Cut(top, (0, 0), (1, 1))] * (solver.MAX_CUTS + 1), "at most 4096")
    _refused(prob, meshes, layer_of, [], "row-partitioned", partition=types.SimpleNamespace(world=2, rank=0))
    with pytest.raises(ValueError, match="same point"):
        solver.solve_currents(prob, [solver.Cut(top, (1, 1), (1, 1))], mesher=object())
    with pytest.raises(ValueError, match="row-partitioned"):
        solver.solve_currents(prob, [], mesher=object(), partition=types.SimpleNamespace(world=2, rank=0))
    cuts = solver.check_cuts(prob, [solver.Cut(prob.layers[1], H.XY(1, 2), [3, 4])] * solver.MAX_CUTS)
    assert len(cuts) == solver.MAX_CUTS and cuts[0] == (1, (1.0, 2.0), (3.0, 4.0))


@pytest.mark.parametrize("name", H.problem_golden_names())
def test_element_flows_and_the_power_balance(name):
    system = S.problem_system(name)
    M, r = system.assemble()
    x = S.solve(M, r)
    flows = solver.element_flows(system.rows, x)
    want = C.element_flows(system.rows, x)
    assert len(flows) == len(system.rows)
    for row, got, ref in zip(system.rows, flows, want):
        assert got.keys() == ref.keys()
        for key in got:
            assert got[key] == pytest.approx(ref[key], rel=1e-15, abs=0.0), (row, key)
        if row[0] == "R":
            assert got["current"] == (x[row[1]] - x[row[2]]) / row[3]
        elif row[0] == "I":
            assert got["current"] == row[3]                                   # exactly its field
    total, size = C.element_power_sum(flows)
    copper = C.layer_power(system, x, len(system.prob.layers))
    assert (copper >= 0).all() and copper.sum() > 0
    assert abs(total + copper.sum()) <= 1e-10 * (size + copper.sum()), (total, copper.sum())


def strip_system(nx=41, ny=9, h=0.25, jitter=0.2, seed=1, current=1.5):
    """A strip [0, (nx-1) h] x [0, (ny-1) h] fed end to end: a current source from the middle vertex of the right end (f) to
    that of the left end (t) pushes ``current`` through the copper from left to right."""
    xy, tri = synthetic.jittered_grid(nx, ny, h=h, seed=seed, jitter=jitter)
    left, right = (ny // 2) * nx, (ny // 2) * nx + nx - 1
    system = S.System(meshes=[(xy, tri, 2000.0)], n_internal=0, rows=[("I", right, left, current)], ground=right,
                      layer_of=[0])
    M, r = system.assemble()
    return system, S.solve(M, r), xy


def kcl_ok(got, current, scale):
    return abs(got - current) <= 1e-10 * max(abs(current), scale)


def test_a_cut_across_a_jittered_strip_carries_the_source_current():
    system, x, xy = strip_system()
    width = xy[:, 0].max()
    _, right, left, _ = system.rows[0]
    assert x[left] > x[right]                                             # the potential falls from left to right
    for start, end in [((4.03, -1.0), (4.11, 3.0)), ((2.0, -0.5), (7.5, 2.5)), ((8.9, 3.1), (9.2, -2.0))]:
        upward = start[1] < end[1]                                        # going up, left of the cut is -x
        got, scale = C.cut_current(system, x, 0, start, end)
        assert 0 < start[0] < width and kcl_ok(got, 1.5 if upward else -1.5, scale), (start, end, got)
        back, _ = C.cut_current(system, x, 0, end, start)
        assert back == -got                                               # reversing the cut negates it, bit for bit
    # a cut that does not cross the strip from side to side: a flux, not the strip's current
    part, _ = C.cut_current(system, x, 0, (5.0, -1.0), (5.0, 1.0))
    assert 0 < part < 1.5
    # a cut on another layer, or beside the copper, crosses nothing
    assert C.cut_current(system, x, 1, (5.0, -1.0), (5.0, 3.0)) == (0.0, 0.0)
    assert C.cut_current(system, x, 0, (-1.0, -1.0), (-0.5, 3.0)) == (0.0, 0.0)


def test_a_cut_along_a_column_of_vertices_counts_them_right():
    system, x, xy = strip_system(jitter=0.0)
    col = np.flatnonzero(xy[:, 0] == 5.0)
    assert len(col) == 9                                                  # the cut's line runs through these vertices
    up, scale = C.cut_current(system, x, 0, (5.0, -1.0), (5.0, 3.0))
    down, _ = C.cut_current(system, x, 0, (5.0, 3.0), (5.0, -1.0))
    assert kcl_ok(up, 1.5, scale) and kcl_ok(down, -1.5, scale)
    # going up the column lies right of the cut, so the edges from x = 4.75 into it cross; going down it lies right again,
    # which is now +x, so the edges from it to x = 5.25 cross: two different sets of edges, the same current
    xs = lambda start, end: {round(float(v), 6) for v in  # noqa: E731
                             xy[np.unique(C.crossing_vertices(system, 0, start, end)), 0]}
    assert xs((5.0, -1.0), (5.0, 3.0)) == {4.75, 5.0} and xs((5.0, 3.0), (5.0, -1.0)) == {5.0, 5.25}

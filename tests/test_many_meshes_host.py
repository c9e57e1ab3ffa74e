"""The board of tests/many_meshes_board.py on the host: its counts, that every mesh carries current, and the locality ordering
of the reduced unknowns where more than 64 meshes have owners (the np.minimum.at branch of reduction._strip_order) and where a
mesh's owners have a bounding box without width or height."""
import warnings

import numpy as np
import pytest

import many_meshes_board as B
import thermal_ref as T
from padne_amd import reduction


@pytest.fixture(scope="module")
def board():
    return B.Board()


def test_the_board_has_the_counts_of_the_table(board):
    b = board
    assert (b.n_mesh, b.n_vert, b.n_tri) == (B.N_MESH, B.N_VERT, B.N_TRI)
    assert sum(B.tiles(n) for n in np.diff(b.toff)) == B.FACE_TILES and sum(B.tiles(n) for n in np.diff(b.voff)) == B.VERTEX_TILES
    assert set(np.diff(b.toff).tolist()) == B.FACES_PER_MESH
    sizes = {what: (int(b.voff[m + 1] - b.voff[m]), int(b.toff[m + 1] - b.toff[m])) for m, what in enumerate(b.what)}
    assert sizes["pad", 5] == (256, 254) and sizes["pad", 600] == (258, 256) and sizes["pad", 1055] == (153, 256)
    assert sizes["pad", 333] == (176, 258) and sizes["plane", 0] == (1599, 3040)
    assert (B.tiles(3040), B.tiles(1599)) == (12, 7)
    layers = np.asarray(b.layer_of)
    assert (layers[1:] != layers[:-1]).all()                 # all 1 099 consecutive pairs lie on different layers
    assert np.count_nonzero(layers == 3) == 1 + B.N_UNDER and np.count_nonzero(layers < 3) == B.N_PADS
    assert len({s for _name, s in B.LAYERS}) == 4
    assert b.n_internal == 1
    assert len(b.prob.networks[0].connections) == B.N_CONNECTIONS and len(b.prob.networks[0].elements) == B.N_ELEMENTS


def test_every_mesh_carries_current_and_the_board_is_nonsingular(board):
    b = board
    M, R, X = b.direct()
    assert M.shape[0] == b.n_pot + 1 == 15_853
    residual = np.linalg.norm(M @ X - R, axis=0)
    span = np.ptp(X[:b.n_vert, 0])
    print("residuals", residual, "potential range", span)
    assert (residual < 1e-9).all() and span > 0.1
    power = T.face_power(b.xy, b.tri, b.face_mesh, b.sigma, X[:b.n_vert, 0])
    per_mesh = np.array([B.fsum(power[lo:hi]) for lo, hi in zip(b.toff[:-1], b.toff[1:])])
    print("power per mesh from", per_mesh.min(), "to", per_mesh.max())
    assert (per_mesh > 0.0).all()
    assert (X[:, 2] == 0.0).all()                            # the dead case
    # the pads without an interior vertex have exact right angles: exact zeros among the cotangents of the assembly
    pad = b.mesh_of["pad", 0]
    assert b.grids[pad][1:3] == (2, 2)
    v0 = b.verts(pad)[0]
    assert M[v0 + 1, v0 + 2] == 0.0 and M[v0, v0 + 1] != 0.0


def test_strip_index_gives_a_degenerate_box_strip_0_without_a_warning():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert reduction.strip_index(np.array([[0.0, 0.0], [0.0, 0.25]]), [0, 0]).tolist() == [0, 0]
        assert reduction.strip_index(np.array([[0.0, 0.0], [0.25, 0.0]]), [0, 0]).tolist() == [0, 0]
        # a box of almost no width: the quotient (4e99) is clamped to 65 536, a value the guard of _strip_order sees
        tiny = reduction.strip_index(np.array([[0.0, 0.0], [1e-200, 1.0]]), [0, 0])
        assert tiny.tolist() == [0, 0x10000]
        # and an ordinary mesh keeps its strips
        x, y = np.meshgrid(np.arange(8.0), np.arange(8.0))
        pts = np.stack([x.ravel(), y.ravel()], axis=1)
        height = 3.4 * np.sqrt(49.0 / 64)
        assert np.array_equal(reduction.strip_index(pts, np.zeros(64, dtype=np.int64)), np.floor(pts[:, 1] / height).astype(np.int64))


def test_locality_ordering_on_a_thousand_meshes_with_degenerate_pads(board):
    b = board
    layout, pick = b.tied_layout()
    red = reduction.build_reduction(layout)
    want, owner, mesh_id = B.lexsort_order(red, b.xy, b.voff)
    has = owner >= 0
    owners_of = np.bincount(mesh_id[has], minlength=b.n_mesh)
    assert np.count_nonzero(owners_of) > 64                  # the np.minimum.at branch of _strip_order
    assert {name: int(owners_of[m]) for name, m in pick.items()} == dict(equal_x=2, equal_y=2, three=3, one=1, none=0, equal_x_late=2)
    ex, ey = owner[has & (mesh_id == pick["equal_x"])], owner[has & (mesh_id == pick["equal_y"])]
    assert np.ptp(b.xy[ex, 0]) == 0.0 and np.ptp(b.xy[ex, 1]) > 0.0 and np.ptp(b.xy[ey, 1]) == 0.0 and np.ptp(b.xy[ey, 0]) > 0.0
    before = np.array(red.index_map)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        reduction.apply_locality_ordering(red, b.xy, b.voff)
    after = np.asarray(red.index_map)
    free = before >= 0
    assert np.array_equal(after >= 0, free)
    new_of_old = np.full(red.n_free, -1, dtype=np.int64)
    new_of_old[before[free]] = after[free]
    assert np.array_equal(np.sort(new_of_old), np.arange(red.n_free))       # a permutation
    order = np.empty(red.n_free, dtype=np.int64)
    order[new_of_old] = np.arange(red.n_free)
    assert np.array_equal(order, want)                       # the stated rule, by a plain lexsort
    # every mesh's owners are contiguous and in mesh order, the unknown that is no vertex behind them
    assert (np.diff(mesh_id[order]) >= 0).all() and mesh_id[order][-1] == len(b.voff) and has.sum() == red.n_free - 1

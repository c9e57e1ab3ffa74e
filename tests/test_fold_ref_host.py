"""tests/fold_ref.py against a literal lane-by-lane simulation of the kernels that fold in the order of error.hpp -- 256
threads, ``__shfl_down(v, off, 64)`` where a lane whose source lies beyond lane 63 keeps its own value, the four LDS slots,
the strided loop as the kernels write it -- and against math.fsum within fold_bound; ties of the tops; tile_tops and
fold_top, the two halves of mesh_top, on their own.  No GPU."""
import math

import numpy as np
import pytest

import fold_ref as F

LENGTHS = [0, 1, 255, 256, 257, 64 * 256, 64 * 256 + 1, 256 * 256, 256 * 256 + 1, 514 * 256]
THREAD = np.arange(256)
LANE, WAVE = THREAD & 63, THREAD >> 6


# ---- the simulation: every array below has one entry per thread of a workgroup (last axis) --------------------------------

def shfl_down(v, off):
    """__shfl_down(v, off, 64) of every thread: lane + off of the same wave; its own value beyond lane 63."""
    src = np.where(LANE + off < 64, THREAD + off, THREAD)
    return v[..., src]


def sim_wave_sum(v):
    for off in (32, 16, 8, 4, 2, 1):                         # error_wave_sum: every lane adds, lane 0 holds the wave's
        v = v + shfl_down(v, off)
    return v


def sim_merge(v, f, ov, of):                                 # error_merge
    take = (ov > v) | ((ov == v) & (of < f))
    return np.where(take, ov, v), np.where(take, of, f)


def sim_wave_top(v, f):
    for off in (32, 16, 8, 4, 2, 1):                         # error_wave_top
        v, f = sim_merge(v, f, shfl_down(v, off), shfl_down(f, off))
    return v, f


def sim_sum4(v):
    """The lanes 0 of the waves write red[w]; thread 0 reads (red[0] + red[1]) + (red[2] + red[3])."""
    red = v[..., [0, 64, 128, 192]]
    return (red[..., 0] + red[..., 1]) + (red[..., 2] + red[..., 3])


def sim_top4(v, f):
    """Thread 0 holds wave 0's top and merges red[1], red[2], red[3] in that order."""
    tv, tf = v[..., 0], f[..., 0]
    for q in (1, 2, 3):
        tv, tf = sim_merge(tv, tf, v[..., 64 * q], f[..., 64 * q])
    return tv, tf


def sim_tiles(items, fill):
    """What the threads of every tile workgroup load: item blockIdx.x * 256 + threadIdx.x, ``fill`` beyond the end."""
    n = len(items)
    at = np.arange(-(-n // 256))[:, None] * 256 + THREAD[None, :]
    return np.where(at < n, np.asarray(items)[np.minimum(at, max(n - 1, 0))] if n else fill, fill)


def sim_mesh_sum(items):
    """A tile kernel (one workgroup per 256 items), then the fold kernel: one workgroup, for (i = threadIdx.x; i < n_tiles;
    i += 256) s += tile[i]."""
    tile = sim_sum4(sim_wave_sum(sim_tiles(np.asarray(items, dtype=np.float64), 0.0))) if len(items) else np.zeros(0)
    s = np.zeros(256)
    i = THREAD.copy()
    while (i < len(tile)).any():
        live = i < len(tile)
        s[live] = s[live] + tile[i[live]]
        i = i + 256
    return float(sim_sum4(sim_wave_sum(s)))


def sim_list_sum(items):
    """sources_sum_kernel: one workgroup, a tile at a time; thread (tile & 255) adds the tile's sum to its part."""
    items = np.asarray(items, dtype=np.float64)
    part = np.zeros(256)
    tile = 0
    for i0 in range(0, len(items), 256):
        at = i0 + THREAD
        v = np.where(at < len(items), items[np.minimum(at, len(items) - 1)], 0.0)
        total = sim_sum4(sim_wave_sum(v))
        part[tile & 255] = part[tile & 255] + total
        tile += 1
    return float(sim_sum4(sim_wave_sum(part)))


def sim_mesh_top(values, indices, empty):
    if len(values):
        tv, tf = sim_top4(*sim_wave_top(sim_tiles(np.asarray(values, dtype=np.float64), empty[0]),
                                        sim_tiles(np.asarray(indices, dtype=np.int64), empty[1])))
    else:
        tv, tf = np.zeros(0), np.zeros(0, np.int64)
    v, f = np.full(256, float(empty[0])), np.full(256, int(empty[1]), dtype=np.int64)
    i = THREAD.copy()
    while (i < len(tv)).any():
        live = i < len(tv)
        v[live], f[live] = sim_merge(v[live], f[live], tv[i[live]], tf[i[live]])
        i = i + 256
    v, f = sim_top4(*sim_wave_top(v, f))
    return float(v), int(f)


def terms(n, signed, seed=0):
    rng = np.random.default_rng(seed + n)
    v = rng.lognormal(0.0, 2.0, n)
    return v * rng.choice([-1.0, 1.0], n) if signed else v


# ---- sums --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("n", LENGTHS)
def test_sums_are_the_simulations_bit_for_bit(n, signed):
    v = terms(n, signed)
    assert F.mesh_sum(v) == sim_mesh_sum(v)
    assert F.list_sum(v) == sim_list_sum(v)
    assert F.list_sum(v) == F.mesh_sum(v)                    # one order, stated twice
    if n == 256:
        assert F.workgroup_sum(v) == F.mesh_sum(v) == float(sim_sum4(sim_wave_sum(v)))
    if n == 0:
        assert F.mesh_sum(v) == 0.0 and not math.copysign(1.0, F.mesh_sum(v)) < 0


def test_the_order_is_not_the_plain_one():
    """The restated order is one of many: numpy's own sum and the front-to-back sum give other bits on the same terms, so a
    bitwise comparison with fold_ref does tell the orders apart."""
    differ = 0
    for seed in range(4):
        v = terms(514 * 256, True, seed=seed)
        differ += F.mesh_sum(v) != float(np.sum(v)) or F.mesh_sum(v) != float(np.cumsum(v)[-1])
    assert differ >= 3


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("n", [1, 257, 16_770, 33_024, 66_306, 131_584, 256 * 256 + 1])
def test_sums_against_fsum_within_the_bound(n, signed):
    v = terms(n, signed, seed=3)
    exact, bound = math.fsum(v.tolist()), F.fold_bound(-(-n // 256), math.fsum(np.abs(v).tolist()))
    err = abs(F.mesh_sum(v) - exact)
    print(n, "signed" if signed else "positive", "error / bound", err / bound)
    assert err <= bound


def test_the_bound_is_the_formula():
    assert F.fold_bound(1, 1.0) == 19 * 2.0 ** -53 and F.fold_bound(256, 2.0) == 19 * 2.0 ** -52
    assert F.fold_bound(257, 1.0) == 20 * 2.0 ** -53 and F.fold_bound(514, 1.0) == 21 * 2.0 ** -53
    assert F.fold_bound(0, 1.0) == 18 * 2.0 ** -53


# ---- tops --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("empty", [F.EMPTY, (-np.inf, F.NO_INDEX)])
@pytest.mark.parametrize("n", LENGTHS)
def test_tops_are_the_simulations(n, empty):
    """Values from a set of 7, so that every tile and every stride holds ties; indices ascending from an offset, as global
    face and vertex numbers are."""
    rng = np.random.default_rng(n)
    values = rng.integers(0, 7, n).astype(np.float64)
    index = 1000 + np.arange(n, dtype=np.int64)
    got = F.mesh_top(values, index, empty=empty)
    assert got == sim_mesh_top(values, index, empty)
    if n:
        assert got == (values.max(), 1000 + int(np.argmax(values)))
        assert F.mesh_top(np.zeros(n), index, empty=empty) == (0.0, 1000)        # the complete tie
    else:
        assert got == (float(empty[0]), F.NO_INDEX)


PLACES = {"two waves of one tile": (70, 200), "two lanes of one wave": (3, 35), "two tiles of one stride": (3 * 256 + 9, 130 * 256 + 1),
          "waves 2 and 3 of the fold": (130 * 256 + 255, 200 * 256), "two strides of one thread": (5 * 256 + 17, 261 * 256 + 2),
          "the third stride": (2 * 256, 513 * 256 + 255), "a later stride in a lower wave": (100 * 256 + 4, 257 * 256 + 8)}


@pytest.mark.parametrize("where", sorted(PLACES))
def test_equal_values_in_different_waves_and_strides_go_to_the_lowest_index(where):
    n = 514 * 256
    values = np.full(n, -0.5)
    lo, hi = PLACES[where]
    values[[lo, hi]] = 2.0
    index = np.arange(n, dtype=np.int64)
    assert F.mesh_top(values, index) == (2.0, lo) == sim_mesh_top(values, index, F.EMPTY)
    values[hi] = np.nextafter(2.0, 3.0)                      # and the larger value wins wherever it sits
    assert F.mesh_top(values, index) == (values[hi], hi)
    # the rule, not the position: with the indices reversed the later item holds the lower index
    assert F.mesh_top(np.where(values > 0, 2.0, values), index[::-1].copy()) == (2.0, n - 1 - hi)


def test_workgroup_top_of_one_tile():
    values = np.full(256, -1.0)
    index = np.full(256, F.NO_INDEX, dtype=np.int64)
    assert F.workgroup_top(values, index) == F.EMPTY
    values[[65, 130]], index[[65, 130]] = 4.0, (9, 7)
    assert F.workgroup_top(values, index) == (4.0, 7)


# ---- the two halves of mesh_top, for a fold that runs over the tiles of several meshes --------------------------------------

def sim_fold_top(tv, tf, empty):
    """The fold kernel alone on a list of tile tops: the strided loop as the kernels write it, then the workgroup's top."""
    v, f = np.full(256, float(empty[0])), np.full(256, int(empty[1]), dtype=np.int64)
    i = THREAD.copy()
    while (i < len(tv)).any():
        live = i < len(tv)
        v[live], f[live] = sim_merge(v[live], f[live], tv[i[live]], tf[i[live]])
        i = i + 256
    v, f = sim_top4(*sim_wave_top(v, f))
    return float(v), int(f)


@pytest.mark.parametrize("empty", [F.EMPTY, (-np.inf, F.NO_INDEX)])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 3 * 256 + 130])
def test_tile_tops_are_the_simulations_and_the_plain_rule_per_tile(n, empty):
    rng = np.random.default_rng(n + 1)
    values = rng.integers(0, 7, n).astype(np.float64)
    index = 1000 + np.arange(n, dtype=np.int64)
    tv, tf = F.tile_tops(values, index, empty=empty)
    assert tv.shape == tf.shape == (-(-n // 256),)
    if n:
        sv, sf = sim_top4(*sim_wave_top(sim_tiles(values, empty[0]), sim_tiles(index, empty[1])))
        assert np.array_equal(tv, sv) and np.array_equal(tf, sf)
    for t in range(len(tv)):
        part = values[t * 256:(t + 1) * 256]
        assert (tv[t], tf[t]) == (part.max(), 1000 + t * 256 + int(np.argmax(part)))
    assert F.mesh_top(values, index, empty=empty) == F.fold_top(tv, tf, empty=empty)


@pytest.mark.parametrize("empty", [F.EMPTY, (-np.inf, F.NO_INDEX)])
@pytest.mark.parametrize("n_tiles", [0, 1, 64, 65, 256, 257, 361, 516, 770])
def test_fold_top_is_the_simulation_and_the_plain_rule(n_tiles, empty):
    """Tile tops as several meshes leave them: values with many ties, indices ascending with gaps (a ragged tile ends its mesh),
    and tiles that hold nothing (``empty``) in between."""
    rng = np.random.default_rng(n_tiles)
    tv = rng.integers(0, 5, n_tiles).astype(np.float64)
    tf = np.cumsum(rng.integers(1, 257, n_tiles)).astype(np.int64)
    hollow = rng.random(n_tiles) < 0.2
    tv[hollow], tf[hollow] = empty
    got = F.fold_top(tv, tf, empty=empty)
    assert got == sim_fold_top(tv, tf, empty)
    if (~hollow).any():
        top = tv[~hollow].max()
        assert got == (top, int(tf[~hollow & (tv == top)].min()))
    else:
        assert got == (float(empty[0]), F.NO_INDEX)


@pytest.mark.parametrize("where", [(3, 259), (259, 300), (104, 360), (0, 256), (255, 256), (200, 513), (256, 512)])
def test_fold_top_ties_between_strides_and_waves_go_to_the_lowest_index(where):
    lo, hi = where
    tv, tf = np.zeros(516), 256 * np.arange(516, dtype=np.int64) + 17
    tv[[lo, hi]] = 2.0
    empty = (-np.inf, F.NO_INDEX)
    assert F.fold_top(tv, tf, empty=empty) == (2.0, int(tf[lo])) == sim_fold_top(tv, tf, empty)
    tv[hi] = np.nextafter(2.0, 3.0)
    assert F.fold_top(tv, tf, empty=empty) == (tv[hi], int(tf[hi]))
    tv[hi], tf[hi] = 2.0, 5                                  # the rule, not the position: the later tile holds the lower index
    assert F.fold_top(tv, tf, empty=empty) == (2.0, 5) == sim_fold_top(tv, tf, empty)

"""The fixed reduction order of padne_amd/csrc/error.hpp in numpy, stated once for every test that holds a per-mesh, per-cut,
per-pair or per-source sum or top of the device to its bits.

Items come in tiles of 256, one workgroup each; a mesh's (cut's, list's) tiles are then folded by one more workgroup.
 1. A tile: the 256 values (dead lanes of a ragged last tile carry 0.0, or the empty top) go down each run of 64 by halving
    strides, v[:h] = v[:h] + v[h:2h] for h = 32 .. 1, and the four runs join as (w0 + w1) + (w2 + w3).
 2. The fold of n tiles: thread i starts from 0.0 (the empty top) and takes tiles i, i + 256, i + 512, ... front to back; the
    256 partial results are joined as in 1.  sources_sum_kernel states the same order differently -- every tile's sum goes
    to slot (tile & 255) -- and list_sum states it that way.
 3. A top is a (value, index) pair; of two, the larger value wins and the lower index wins a tie (error_merge).  The halving
    step merges lane i + h into lane i; the four runs merge from run 0 to run 3.  A lane without an item carries ``empty``,
    (-1.0, NO_INDEX) or (-inf, NO_INDEX) as the kernel in question does.

fold_bound is the rounding such a sum can have picked up; it is derived from the order, not measured."""
from __future__ import annotations

import math

import numpy as np

TILE = 256
NO_INDEX = 0x7fffffffffffffff            # kErrNoFace: the index of a lane that holds no item
EMPTY = (-1.0, NO_INDEX)


def _padded(items, fill, dtype):
    """``items`` as rows of 256, the last one filled up with ``fill``."""
    items = np.asarray(items, dtype=dtype).reshape(-1)
    out = np.full((-(-len(items) // TILE)) * TILE, fill, dtype=dtype)
    out[:len(items)] = items
    return out.reshape(-1, TILE)


def _workgroup_sums(rows) -> np.ndarray:
    """Definition 1 on every row of (n, 256)."""
    w = np.array(rows, dtype=np.float64).reshape(-1, 4, 64)
    for h in (32, 16, 8, 4, 2, 1):
        w[:, :, :h] = w[:, :, :h] + w[:, :, h:2 * h]
    return (w[:, 0, 0] + w[:, 1, 0]) + (w[:, 2, 0] + w[:, 3, 0])


def workgroup_sum(v) -> float:
    """256 values in the device's fixed order (definition 1)."""
    return float(_workgroup_sums(np.asarray(v, dtype=np.float64).reshape(1, TILE))[0])


def _tile_sums(items) -> np.ndarray:
    """The sum of every tile of 256 items, the ragged tail filled with 0.0."""
    return _workgroup_sums(_padded(items, 0.0, np.float64))


def _fold_sum(tiles) -> float:
    """Definition 2 on the tile sums of one mesh."""
    part = np.zeros(TILE)
    for row in _padded(tiles, 0.0, np.float64):      # (a thread without a tile in the last stride adds nothing: x + 0.0 is x,
        part = part + row                            # and a partial sum that started from 0.0 is never -0.0)
    return workgroup_sum(part)


def mesh_sum(items) -> float:
    """One mesh's items: tiles of 256, then the fold of the tiles."""
    return _fold_sum(_tile_sums(items))


def list_sum(items) -> float:
    """sources_sum_kernel's statement of the same order: one workgroup walks the list a tile at a time, and the sum of tile
    number ``tile`` is added to the partial sum of slot ``tile & 255``."""
    part = np.zeros(TILE)
    for tile, total in enumerate(_tile_sums(items)):
        part[tile & 255] = part[tile & 255] + total
    return workgroup_sum(part)


def _merge(v, f, ov, of):
    """error_merge, elementwise: (ov, of) replaces (v, f) where ov > v, or ov == v and of < f."""
    take = (ov > v) | ((ov == v) & (of < f))
    return np.where(take, ov, v), np.where(take, of, f)


def _workgroup_tops(values, indices):
    """Definition 3 on every row of (n, 256)."""
    v = np.array(values, dtype=np.float64).reshape(-1, 4, 64)
    f = np.array(indices, dtype=np.int64).reshape(-1, 4, 64)
    for h in (32, 16, 8, 4, 2, 1):
        v[:, :, :h], f[:, :, :h] = _merge(v[:, :, :h], f[:, :, :h], v[:, :, h:2 * h], f[:, :, h:2 * h])
    tv, tf = v[:, 0, 0], f[:, 0, 0]
    for q in (1, 2, 3):
        tv, tf = _merge(tv, tf, v[:, q, 0], f[:, q, 0])
    return tv, tf


def workgroup_top(values, indices):
    """(value, index) of 256 pairs."""
    tv, tf = _workgroup_tops(np.asarray(values, dtype=np.float64).reshape(1, TILE), np.asarray(indices, dtype=np.int64).reshape(1, TILE))
    return float(tv[0]), int(tf[0])


def tile_tops(values, indices, empty=EMPTY):
    """(values (n_tiles,), indices (n_tiles,)): the top of every tile of 256 pairs, the ragged tail filled with ``empty``.  For
    a kernel whose tiles are per mesh and whose fold runs over all of them (film_fold_kernel): the tops of each mesh,
    concatenated, go to :func:`fold_top`."""
    return _workgroup_tops(_padded(values, empty[0], np.float64), _padded(indices, empty[1], np.int64))


def fold_top(values, indices, empty=EMPTY):
    """Definition 2 for tops, on a list of tile tops (one mesh's, or every mesh's in tile order): (value, index); ``empty``
    for no tiles."""
    v, f = _padded(values, empty[0], np.float64), _padded(indices, empty[1], np.int64)
    pv, pf = np.full(TILE, float(empty[0])), np.full(TILE, int(empty[1]), dtype=np.int64)
    for rv, rf in zip(v, f):             # a thread without a tile in the last stride merges nothing: the fill is ``empty``
        pv, pf = _merge(pv, pf, rv, rf)
    return workgroup_top(pv, pf)


def mesh_top(values, indices, empty=EMPTY):
    """One mesh's (value, index) pairs: tiles of 256, then the fold of the tile tops.  A mesh without items gives ``empty``."""
    return fold_top(*tile_tops(values, indices, empty), empty=empty)


def fold_bound(n_tiles: int, abs_sum: float) -> float:
    """(18 + ceil(n_tiles / 256)) 2^-53 sum |term|: the additions a term can pass through -- 8 in the waves of its tile and 2
    in the join of the waves (counted generously: a wave of 64 halves 6 times), ceil(n_tiles / 256) in the strided loop,
    8 + 2 in the fold -- each with a relative error of at most 2^-53 on a partial sum no larger than sum |term|.  Terms of
    second order are left out."""
    return (18 + math.ceil(n_tiles / 256)) * 2.0 ** -53 * float(abs_sum)

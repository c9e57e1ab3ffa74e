"""Host restatement of the temperature sampler for the tests (DESIGN.md "Thermal images"): the owner by brute force over ALL
faces of the layer (tests/sampling_ref.py, no index), every field by the written formula at that one owner, the heat flux
with the face gradient's arithmetic, the sequential hottest field, and a raster's tops by ``np.nanmax`` with the lowest
index.  No fused multiply-add in numpy, so every value is the device's bit for bit."""
from __future__ import annotations

import numpy as np

import sampling_ref as R


def field_block(fields) -> np.ndarray:
    """(F, n_vert) of fields given as the reports hold them: per layer, per mesh a ZeroForm, in the flat order."""
    return np.stack([np.concatenate([np.asarray(zf.values, np.float64) for per_layer in fld for zf in per_layer]
                                    or [np.zeros(0)]) for fld in fields])


def board_of_field(prob, field) -> R.Board:
    """The Board of the meshes of one field (potentials zero, sigma the layers' electrical conductances)."""
    meshes = [(zf.mesh.points, zf.mesh.triangles, layer.conductance, li)
              for li, (layer, per_layer) in enumerate(zip(prob.layers, field)) for zf in per_layer]
    return R.board(meshes, [np.zeros(len(np.asarray(m[0]).reshape(-1, 2))) for m in meshes])


def face_flux(b: R.Board, faces, values, kappa):
    """-kappa grad T (n, 2) of the given global faces for ONE field ``values`` (n_vert,): ``sampling_ref.face_values``'
    arithmetic with the field in the place of the potential and kappa[n_mesh] in the place of sigma."""
    as_field = R.Board(xy=b.xy, tri=b.tri, toff=b.toff, voff=b.voff, sigma=np.asarray(kappa, np.float64), layer_of=b.layer_of,
                       V=np.asarray(values, np.float64))
    return R.face_values(as_field, faces)[0]


def hottest_of(T):
    """(hottest (n,), hottest_field (n,) int32) of T (F, n): field 0 first, replaced on strictly greater; a sample that is
    NaN in field 0 (no owner) is NaN and -1."""
    T = np.asarray(T, np.float64)
    hot, field = T[0].copy(), np.zeros(T.shape[1], np.int32)
    for f in range(1, T.shape[0]):
        greater = T[f] > hot
        hot[greater] = T[f][greater]
        field[greater] = f
    field[np.isnan(T[0])] = -1
    return hot, field


def sample_fields(b: R.Board, fields, kappa, layer: int, q):
    """(face (n,) global or -1, T (F, n), flux (F, n, 2) or None without kappa, hottest (n,), hottest_field (n,)); NaN and -1
    where there is no owner.  ``fields``: (F, n_vert)."""
    q = np.asarray(q, np.float64).reshape(-1, 2)
    fields = np.asarray(fields, np.float64)
    F, n = fields.shape[0], len(q)
    face = R.owners(b, layer, q)
    T = np.full((F, n), np.nan)
    flux = None if kappa is None else np.full((F, n, 2), np.nan)
    hit = np.flatnonzero(face >= 0)
    if len(hit):
        f = face[hit]
        t = b.tri[f]
        qx, qy = q[hit, 0], q[hit, 1]
        oa, ob, oc = (R.edge_side(b, t[:, 1], t[:, 2], qx, qy), R.edge_side(b, t[:, 2], t[:, 0], qx, qy),
                      R.edge_side(b, t[:, 0], t[:, 1], qx, qy))
        s = (oa + ob) + oc
        for k in range(F):
            v = fields[k]
            T[k, hit] = ((oa / s) * v[t[:, 0]] + (ob / s) * v[t[:, 1]]) + (oc / s) * v[t[:, 2]]
            if flux is not None:
                flux[k, hit] = face_flux(b, f, v, kappa)
    hot, hot_field = hottest_of(T)
    return face, T, flux, hot, hot_field


def raster_tops(T, hottest) -> list:
    """Per field of T (F, n) and then for ``hottest`` (n,): (value, flat pixel) of the largest value that is not NaN, the
    lowest pixel on a tie, or None where every pixel is NaN."""
    out = []
    for row in list(np.asarray(T, np.float64)) + [np.asarray(hottest, np.float64)]:
        if np.isnan(row).all():
            out.append(None)
            continue
        top = np.nanmax(row)
        out.append((float(top), int(np.flatnonzero(row == top)[0])))
    return out


def tops_of(samples, width: int) -> list:
    """``TemperatureSamples.tops`` as (value, flat pixel) pairs, after checking each entry's row, column and position."""
    out = []
    for entry in samples.tops:
        if entry is None:
            out.append(None)
            continue
        value, row, col, x, y = entry
        assert (x, y) == tuple(samples.points[row, col])
        out.append((value, row * width + col))
    return out

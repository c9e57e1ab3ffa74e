"""Host restatement of the current report for the tests: J = -sigma grad V per face (the oracle's gradient, corners in the
order the device visits them), |J|, the hotspot rule, the cut rule of DESIGN.md "Currents" in numpy and the element flows
from the stamps.  The cut rule uses the same orient() arithmetic as the device, so every crossing decision is the same
bit for bit; only the order of the sums differs."""
from __future__ import annotations

import numpy as np

import sensitivity_ref as S
from oracle import padne_oracle as O


def all_xy(system: S.System) -> np.ndarray:
    return np.concatenate([np.asarray(m[0], dtype=np.float64).reshape(-1, 2) for m in system.meshes])


def face_layers(system: S.System) -> np.ndarray:
    """The layer of every face, in unknown (mesh) order."""
    return np.concatenate([np.full(len(np.asarray(m[1]).reshape(-1, 3)), layer, dtype=np.int64)
                           for m, layer in zip(system.meshes, system.layer_of)] or [np.zeros(0, np.int64)])


def face_J(system: S.System, x):
    """(J (n_tri, 2) = -sigma grad x, the size of the terms each gradient sums (n_tri,)): sigma (|x_1| + |x_2| + |x_3|)
    times the longest edge over twice the area, what the rounding of grad x is relative to."""
    tri, _, sig, area = S.faces(system)
    xy = all_xy(system)
    c = [tri[:, 2], tri[:, 0], tri[:, 1]]                     # the device visits a face as (tri[2], tri[0], tri[1])
    gx, gy = O.triangle_gradient(xy[c[0]], xy[c[1]], xy[c[2]], x[c[0]], x[c[1]], x[c[2]])
    edge = np.max([np.hypot(*(xy[tri[:, e]] - xy[tri[:, (e + 1) % 3]]).T) for e in range(3)], axis=0)
    size = sig * (np.abs(x[tri]).sum(axis=1)) * edge / (2 * area)
    return np.stack([-sig * gx, -sig * gy], axis=1), size


def hotspots(system: S.System, mag, n_layers: int) -> list:
    """Per layer (max |J|, global face) over its faces, the lowest face on a tie; None for a layer without faces."""
    layers = face_layers(system)
    out = []
    for layer in range(n_layers):
        faces = np.flatnonzero(layers == layer)
        if not len(faces):
            out.append(None)
            continue
        k = int(np.argmax(mag[faces]))                        # the first maximum: the lowest face
        out.append((float(mag[faces[k]]), int(faces[k])))
    return out


def layer_power(system: S.System, x, n_layers: int) -> np.ndarray:
    """Per layer sum over its faces of sigma sum_edges w_ik (x_i - x_k)^2 (all terms >= 0: the sum is its own scale)."""
    s = S.face_s(system, x, x)
    return np.bincount(face_layers(system), weights=s, minlength=n_layers)


def orient(a, b, p):
    """(b.x - a.x)(p.y - a.y) - (b.y - a.y)(p.x - a.x), elementwise, in that order (no fused multiply-add in numpy)."""
    return (b[..., 0] - a[..., 0]) * (p[..., 1] - a[..., 1]) - (b[..., 1] - a[..., 1]) * (p[..., 0] - a[..., 0])


def cut_terms(system: S.System, x, layer: int, start, end) -> np.ndarray:
    """The nonzero terms sigma w (x_left - x_right) of the cut rule: per face of the layer, per edge (P, Q) with P the lower
    global vertex, when P and Q lie on different sides of the cut's line (orient > 0: left; on the line: right) and start
    and end on different sides of the edge's line."""
    tri, cot, sig, _ = S.faces(system)
    xy = all_xy(system)
    on = face_layers(system) == layer
    a, b = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    out = []
    for e in range(3):
        i, k = tri[:, e], tri[:, (e + 1) % 3]
        P, Q = np.minimum(i, k), np.maximum(i, k)
        lp, lq = orient(a, b, xy[P]) > 0, orient(a, b, xy[Q]) > 0
        ls, le = orient(xy[P], xy[Q], a) > 0, orient(xy[P], xy[Q], b) > 0
        cross = on & (lp != lq) & (ls != le)
        d = np.where(lp, x[P] - x[Q], x[Q] - x[P])
        out.append((sig * cot[:, e] * d)[cross])
    return np.concatenate(out)


def crossing_vertices(system: S.System, layer: int, start, end) -> np.ndarray:
    """The global vertices of the edges the cut rule counts as crossing (each edge once per face that has it)."""
    tri, _, _, _ = S.faces(system)
    xy = all_xy(system)
    on = face_layers(system) == layer
    a, b = np.asarray(start, dtype=np.float64), np.asarray(end, dtype=np.float64)
    out = []
    for e in range(3):
        i, k = tri[:, e], tri[:, (e + 1) % 3]
        P, Q = np.minimum(i, k), np.maximum(i, k)
        cross = (on & ((orient(a, b, xy[P]) > 0) != (orient(a, b, xy[Q]) > 0))
                 & ((orient(xy[P], xy[Q], a) > 0) != (orient(xy[P], xy[Q], b) > 0)))
        out.extend([P[cross], Q[cross]])
    return np.concatenate(out)


def cut_current(system: S.System, x, layer: int, start, end):
    """(the current through the cut, the sum of the absolute values of its terms)."""
    t = cut_terms(system, x, layer, start, end)
    return float(t.sum()), float(np.abs(t).sum())


def element_flows(rows, x) -> list:
    """current and power of every element row, restated from the stamps (L = -G): Resistor (x_a - x_b)/R, CurrentSource
    its field, VoltageSource and regulator output -x_iv, regulator input -gain x_iv; power (x_first - x_second) current."""
    out = []
    for row in rows:
        if row[0] == "R":
            i = (x[row[1]] - x[row[2]]) / row[3]
            out.append({"current": i, "power": (x[row[1]] - x[row[2]]) * i})
        elif row[0] == "I":
            out.append({"current": row[3], "power": (x[row[1]] - x[row[2]]) * row[3]})
        elif row[0] == "V":
            i = -x[row[4]]
            out.append({"current": i, "power": (x[row[1]] - x[row[2]]) * i})
        else:
            _, vp, vn, sf, st, _u, gain, iv = row
            i, j = -x[iv], -gain * x[iv]
            out.append({"current": i, "power": (x[vp] - x[vn]) * i, "input_current": j, "input_power": (x[sf] - x[st]) * j})
    return out


def element_power_sum(flows) -> tuple:
    """(sum of every element's absorbed power, the sum of their absolute values)."""
    p = [d[k] for d in flows for k in ("power", "input_power") if k in d]
    return float(np.sum(p)), float(np.abs(p).sum())

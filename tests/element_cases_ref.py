"""Dense numpy/scipy restatement of the element cases for the tests: the block's columns, G, w and sigma of every case by
their definitions, from direct solves, and the direct solve of a changed system.  A case is given on the element rows of a
``sensitivity_ref.System`` (global unknowns): ``{row index: new value}``, the value of a resistor row being its new
resistance (``math.inf``: open) and that of a source row its new current or voltage."""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

import sensitivity_ref as S

VALUE_AT = {"R": 3, "I": 3, "V": 3, "REG": 5}


def changed_rows(rows, case: dict) -> list:
    """The element rows with the case applied; an open resistor is left out."""
    out = []
    for i, row in enumerate(rows):
        if i in case:
            if row[0] == "R" and not math.isfinite(case[i]):
                continue
            at = VALUE_AT[row[0]]
            row = row[:at] + (float(case[i]),) + row[at + 1:]
        out.append(row)
    return out


def changed_system(system: S.System, case: dict):
    """(M', r') of the system with the case applied: same unknowns, the changed rows stamped by the oracle."""
    return system.assemble(rows=changed_rows(system.rows, case))


def restamped_system(system: S.System, case: dict, base):
    """changed_system of a case that changes resistors only, from ``base`` = (M, r) of the system as given: each changed
    resistor's stamp taken out of M and its new one put in, entry by entry, without assembling the meshes again."""
    M, r = base
    N = M.shape[0]
    rows, cols, vals = [], [], []
    for i, value in case.items():
        kind, a, b, res = system.rows[i]
        assert kind == "R"
        dg = 1.0 / res - (1.0 / value if math.isfinite(value) else 0.0)          # the stamp is -g d d^T
        rows += [a, a, b, b]
        cols += [a, b, b, a]
        vals += [dg, -dg, dg, -dg]
    return (M + sp.coo_matrix((vals, (rows, cols)), shape=(N, N))).tocsr(), r


def direct_case(system: S.System, case: dict, base=None) -> np.ndarray:
    """The direct solve of the changed system (``base``: restamped_system instead of a new assembly)."""
    M, r = changed_system(system, case) if base is None else restamped_system(system, case, base)
    return S.solve(M, r)


def columns(system: S.System, cases: list):
    """(source settings in first-appearance order, case -> its setting, changed resistor rows in stamping order that join
    two unknowns, R [N, n_src + n_res] dense)."""
    settings, case_source = [], []
    for case in cases:
        src = {i: v for i, v in case.items() if system.rows[i][0] != "R"}
        if src not in settings:
            settings.append(src)
        case_source.append(settings.index(src))
    res = sorted({i for case in cases for i in case if system.rows[i][0] == "R" and system.rows[i][1] != system.rows[i][2]})
    N = system.assemble()[0].shape[0]
    R = np.zeros((N, len(settings) + len(res)))
    for j, src in enumerate(settings):
        R[:, j] = system.assemble(rows=changed_rows(system.rows, src))[1]
    for m, i in enumerate(res):
        R[system.rows[i][1], len(settings) + m] += 1.0
        R[system.rows[i][2], len(settings) + m] -= 1.0
    return settings, case_source, res, R


def weights(system: S.System, cases: list):
    """(W dense [n_cases, n_cols], sigma [n_cases], V = M^-1 R, R): x'_c = V W[c]."""
    settings, case_source, res, R = columns(system, cases)
    M, _ = system.assemble()
    V = S.solve(M, R)
    n_src = len(settings)
    W = np.zeros((len(cases), R.shape[1]))
    sigma = np.ones(len(cases))
    for c, case in enumerate(cases):
        s = case_source[c]
        W[c, s] = 1.0
        S_cols = [m for m, i in enumerate(res) if i in case]
        if not S_cols:
            continue
        g = np.array([1.0 / system.rows[res[m]][3] for m in S_cols])
        g_new = np.array([1.0 / case[res[m]] if math.isfinite(case[res[m]]) else 0.0 for m in S_cols])
        D = R[:, [n_src + m for m in S_cols]]
        Z = V[:, [n_src + m for m in S_cols]]
        C = np.diag(g - g_new)
        G = np.eye(len(S_cols)) + C @ (D.T @ Z)
        sigma[c] = np.linalg.svd(G, compute_uv=False).min()
        W[c, [n_src + m for m in S_cols]] = -np.linalg.solve(G, C @ (D.T @ V[:, s]))
    return W, sigma, V, R

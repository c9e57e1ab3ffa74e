"""Every SpMV / SpMM kernel form and epilogue against a plain high-precision host reference (needs an MI355X).

One product at a time, on inputs chosen here, through the launchers the solver calls (padne_test_product of
include/padne_hip_probe.h runs one of them once and reports the kernel form it took).  Three kinds of check:

  * a forward error bound for every row against the exact result.  f32 forms are referred to float64 arithmetic on the
    float32 inputs (products of two floats are exact there), f64 forms to np.longdouble (64-bit significand):
        |y_i - ref_i| <= (m_i + c) * u * E_i
    m_i the row length, u = 2^-24 or 2^-53 for the type the kernel accumulates in, E_i the envelope -- sum |a_ik x_k| plus the
    magnitudes of the epilogue's other terms -- and c per epilogue (BOUND_C): any order of summing m products costs at most
    gamma_m * sum |a x| (Higham, Thm 3.1 -- the shuffle tree of the wave-per-row kernel included), every further operation of
    the epilogue one more rounding of at most u * E_i;
  * bit for bit where the code promises it: the tile kernels sum every row in CSR order and the library is built with
    -ffp-contract=off (spmv.hip:14-15), so every tile form -- gather, x windows of 72 / 128, the wide plan, the 16-per-lane form,
    the interior / boundary lists -- equals scipy's sequential CSR product followed by the epilogue restated in numpy in the
    kernel's own operation order and type; every SpMM column equals that as well (spmm.hip:11-13);
  * the dot partials: the reference dot is formed from the kernel's OWN output exactly as its epilogue forms each term, so what is
    tested is the reduction alone: |fsum(partials[:count]) - fsum(terms)| <= gamma_{n+8} * sum |terms|; every slot the launch
    does not own still holds the sentinel.

Outputs sit inside one allocation between sentinel-filled margins: a store out of range lands there and is seen.
"""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.sparse as sp

import helpers as H
from padne_amd import _hip

gpu = pytest.mark.gpu

# launchers (padne_hip_probe.h)
SPMV_MODE, SPMV_PART, DOT_X32, F32, F32_PART, F32_RESTRICT, F32_RESID_PRE, F32_EXIT, F32_EXIT_PART, F32_WUP, F32_WUP_EXIT, \
    SPMM_MODE, SPMM_F32, SPMM_F32_EXIT, SPMM_F32_WUP, SPMM_F32_WUP_EXIT = range(16)
LNAME = ["spmv_mode", "spmv_part", "spmv_dot_x32", "spmv_f32", "spmv_f32_part", "spmv_f32_restrict", "spmv_f32_resid_pre",
         "spmv_f32_exit", "spmv_f32_exit_part", "spmv_f32_wup", "spmv_f32_wup_exit", "spmm_mode", "spmm_f32", "spmm_f32_exit",
         "spmm_f32_wup", "spmm_f32_wup_exit"]
# epilogues (common.hpp)
PLAIN, DOT, RESID, ADD, JACOBI, DOT_AUX, WUP, RESTRICT, RESID_PRE = range(9)
ALL, INTERIOR, BOUNDARY = range(3)
HIER, DINV, BF32, XW, XW_WIDE, SPLIT = 1, 2, 4, 8, 16, 32
NONE, WPR, LIST, LONG, WIDE, TILE = range(6)
FNAME = ["none", "wpr", "list", "long", "wide", "tile"]
MAXP = 2048                     # kMaxPartials
MARGIN = 256                    # sentinel entries before and after every output
SENT = 0xFF                     # sentinel byte (a NaN in either precision)

# c of the bound (m_i + c) * u * E_i per epilogue: one rounding per operation behind the sum
BOUND_C = {
    PLAIN: 1,        # y = acc: the sum itself
    DOT: 1, DOT_AUX: 1,
    RESID: 2,        # b - acc: one subtraction
    ADD: 2,          # y + acc: one addition
    RESTRICT: 3,     # y2 = (s d) acc: two products on top of the sum (y itself: c = 1)
    JACOBI: 4,       # x + (s d)(b - acc): a subtraction, two products, an addition
    WUP: 4,          # x_pre + (s d) r_pre + acc, or (s d)(rhs + r_pre) + acc: two products, two additions
    RESID_PRE: 5,    # staged (s d_k) x_k: two more roundings in every product, then one subtraction
}
EXIT_EXTRA = 2       # double output times sqrt(s2): the rounding of the square root and of the product

REACHED = set()      # (launcher, mode, k, form, xw_run) of every case run


# ---- inputs ----------------------------------------------------------------------------------------------------------

def vals(rng, n, wide=False):
    """Magnitudes in [0.5, 2] with random signs (a dropped, doubled or misplaced term is far above any bound), or
    1e-6 ... 1e6 (wide): an f32 accumulator is then orders of magnitude off the f64 bound."""
    mag = 10.0 ** rng.uniform(-6, 6, n) if wide else rng.uniform(0.5, 2.0, n)
    return mag * rng.choice([-1.0, 1.0], n)


def with_values(S, seed, wide=False):
    S = sp.csr_matrix(S)
    S.sum_duplicates()
    S.sort_indices()
    S.data = vals(np.random.default_rng(seed), S.nnz, wide)
    return S


def ragged(n_rows, n_cols, per_row, seed, empty_tile=None, long_rows=(), hub=0):
    """random_csr with its values replaced, some empty rows inside tiles, optionally one all-empty 64-row tile, rows of given
    lengths at the front, and a hub row of `hub` entries."""
    A = H.random_csr(n_rows, n_cols, per_row, seed).tolil()
    rng = np.random.default_rng(seed + 100)
    for i, ln in enumerate(long_rows):
        r = (i * 67 + 3) % max(n_rows, 1)
        A.rows[r] = sorted(rng.choice(n_cols, min(ln, n_cols), replace=False).tolist())
        A.data[r] = [1.0] * len(A.rows[r])
    if hub:
        r = n_rows // 2
        A.rows[r] = sorted(rng.choice(n_cols, min(hub, n_cols), replace=False).tolist())
        A.data[r] = [1.0] * len(A.rows[r])
    A = A.tocsr()
    keep = np.ones(n_rows, bool)
    keep[rng.choice(n_rows, n_rows // 23, replace=False) if n_rows >= 23 else []] = False
    if empty_tile is not None and n_rows >= 64 * (empty_tile + 1):
        keep[64 * empty_tile:64 * (empty_tile + 1)] = False
    keep[[(i * 67 + 3) % max(n_rows, 1) for i in range(len(long_rows))] + ([n_rows // 2] if hub else [])] = True
    A = sp.diags(keep.astype(float)) @ A if n_rows else A
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    return with_values(A, seed)


def banded(n, ncols, half, seed, keep=0.5, far=0.002):
    """The band generator of test_x_window_tiles_and_gather_tiles_in_one_product: three bands (-311, 0, 297) of half-width
    `half` (3: every tile fits three runs of 72; 20: runs of 128), a few rows with far-away columns (their tiles gather)."""
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for off in (-311, 0, 297):
        for d in range(-half, half + 1):
            r = np.flatnonzero(rng.random(n) < keep)
            c = r + off + d
            ok = (c >= 0) & (c < ncols)
            rows.append(r[ok])
            cols.append(c[ok])
    fr = rng.choice(n, int(n * far), replace=False)
    rows.append(fr)
    cols.append(rng.integers(0, ncols, len(fr)))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    sel = rows % 997 != 0                                                            # some empty rows
    M = sp.csr_matrix((np.ones(sel.sum()), (rows[sel], cols[sel])), shape=(n, ncols))
    return with_values(M, seed + 1)


def w_like(n, seed):
    """A fused up-leg operator W's shape: fine rows, aggregate columns (four fine rows per aggregate, ~5 entries per row in a few
    short runs), a few far columns: the wide plan of twelve runs of 20."""
    rng = np.random.default_rng(seed)
    nc = n // 4 + 1
    r = np.repeat(np.arange(n), 5)
    base = np.arange(n) // 4
    c = np.stack([base, base + 1, base - 1, base + 40, base - 40], 1).reshape(-1)
    c = np.where(rng.random(len(c)) < 0.001, rng.integers(0, nc, len(c)), c)
    hub = np.arange(7, n, 64 * 50)                  # every 50th tile: a row of 15 scattered columns, more runs than twelve
    r = np.concatenate([r, np.repeat(hub, 15)])
    c = np.concatenate([c, rng.integers(0, nc, 15 * len(hub))])
    ok = (c >= 0) & (c < nc)
    M = sp.csr_matrix((np.ones(ok.sum()), (r[ok], c[ok])), shape=(n, nc))
    return with_values(M, seed + 1)


# ---- one product on the device ---------------------------------------------------------------------------------------

F64_IN = {SPMV_MODE, SPMV_PART, SPMM_MODE}
F64_OUT = {SPMV_MODE, SPMV_PART, DOT_X32, F32_EXIT, F32_EXIT_PART, F32_WUP_EXIT, SPMM_MODE, SPMM_F32_EXIT, SPMM_F32_WUP_EXIT}


class Guarded:
    """A device vector between two sentinel-filled margins of MARGIN entries, in one allocation."""

    def __init__(self, ctx, n, dtype, init=None):
        self.n, self.dtype = n, np.dtype(dtype)
        host = np.full((n + 2 * MARGIN) * self.dtype.itemsize, SENT, np.uint8).view(self.dtype)
        if init is not None:
            host[MARGIN:MARGIN + n] = init
        self.init = host.copy()
        self.buf = ctx.to_device(host)
        self.ptr = self.buf.ptr + MARGIN * self.dtype.itemsize

    def read(self):
        h = self.buf.numpy()
        raw, ini = h.view(np.uint8), self.init.view(np.uint8)
        b = MARGIN * self.dtype.itemsize
        assert np.array_equal(raw[:b], ini[:b]) and np.array_equal(raw[-b:], ini[-b:]), "store outside the output"
        return h[MARGIN:MARGIN + self.n]

    def untouched(self):
        return np.array_equal(self.buf.numpy().view(np.uint8), self.init.view(np.uint8))


def run(ctx, M, launcher, A, *, mode=PLAIN, k=1, part=ALL, flags=0, n_owned=0, x, y0=None, aux0=None, aux1=None, aux2=None,
        rhs=None, dot_with=None, scale=0.0, s2=None, z32=False, partials=True, done=False):
    """One launch.  Vectors are host arrays ([n] or [n][k] flattened); returns outputs, partials and the reported info."""
    lib = ctx._lib
    n = A.shape[0] * (k if launcher >= SPMM_MODE else 1)
    tin = np.float64 if launcher in F64_IN else np.float32
    keep = []

    def dev(a, dt):
        if a is None:
            return None
        d = ctx.to_device(np.ascontiguousarray(a, dtype=dt))
        keep.append(d)
        return d.ptr

    xp = dev(x, np.float32 if launcher == DOT_X32 else tin)
    y = Guarded(ctx, n, np.float64 if launcher in F64_OUT else np.float32, y0)
    y2 = Guarded(ctx, n, np.float32) if (z32 or launcher == F32_RESTRICT) else None
    done_p = dev(np.array([1 if done else 0], np.int32), np.int32)
    s2p = dev(s2, np.float64)
    ph = np.zeros(k * MAXP if launcher >= SPMM_MODE else MAXP)
    info = np.zeros(8, np.int32)
    rc = lib.padne_test_product(ctx._h, M._h, flags, n_owned, launcher, mode, k, part, xp, y.ptr, y2.ptr if y2 else None,
                                dev(aux0, tin), dev(aux1, tin), dev(aux2, tin), dev(rhs, np.float32), dev(dot_with, np.float64),
                                done_p, float(scale), s2p, ph.ctypes.data_as(C.POINTER(C.c_double)) if partials else None,
                                len(ph), info.ctypes.data_as(C.POINTER(C.c_int32)))
    _hip._check(rc)
    form, xw_state, xw_run, xw_nruns = (int(v) for v in info[:4])
    run_key = xw_run if (xw_state == 1 and form in (TILE, WIDE) and launcher < SPMM_MODE) else 0
    if not done:
        REACHED.add((LNAME[launcher], mode, k, FNAME[form], run_key))
    return dict(y=y, y2=y2, partials=ph if partials else None, form=form, xw_run=run_key, count=int(info[4]),
                n_int=int(info[5]), n_bnd=int(info[6]), off_bnd=int(info[7]))


# ---- references ------------------------------------------------------------------------------------------------------

def segsum(v, indptr):
    out = np.zeros(len(indptr) - 1, v.dtype)
    nz = indptr[1:] > indptr[:-1]
    if nz.any():
        out[nz] = np.add.reduceat(v, indptr[:-1][nz])
    return out


def exact_rows(A, a, xv, dt):
    """sum_k a_ik x_k and sum_k |a_ik x_k| in dt (float64 for float32 inputs: exact products; longdouble for doubles)."""
    p = a.astype(dt) * xv.astype(dt)[A.indices]
    return segsum(p, A.indptr), segsum(np.abs(p), A.indptr)


def bound_ok(got, ref, E, m, c, u):
    err = np.abs(got.astype(ref.dtype) - ref)
    lim = (m + c) * u * E
    bad = np.flatnonzero(~(err <= lim))
    assert bad.size == 0, (f"{bad.size} rows beyond the bound, first {bad[:5]}: got {got[bad[:3]]} ref {ref[bad[:3]]} "
                           f"err {err[bad[:3]]} bound {lim[bad[:3]]}")


def check_partials(res, terms_by_col, k, part=ALL):
    """fsum of the kernel's partials against fsum of the terms its epilogue forms (taken from its own output); every slot the
    launch does not own still holds the sentinel."""
    ph = res["partials"]
    raw = ph.view(np.uint64)
    sent = np.uint64(0xFFFFFFFFFFFFFFFF)
    for j in range(k):
        row = ph[j * MAXP:(j + 1) * MAXP]
        rr = raw[j * MAXP:(j + 1) * MAXP]
        lo, hi = 0, res["count"]
        if res["form"] == NONE:                       # nothing launched
            lo = hi = 0
        if part == INTERIOR and res["n_int"] + res["n_bnd"]:
            hi = res["off_bnd"]
        elif part == BOUNDARY and res["n_int"] + res["n_bnd"]:
            lo = res["off_bnd"]
        assert (rr[:lo] == sent).all() and (rr[hi:] == sent).all(), f"partial sums written outside [{lo}, {hi}) (column {j})"
        if terms_by_col is None or hi == lo:
            assert (rr[lo:hi] == sent).all()
            continue
        t = terms_by_col[j]
        got = math.fsum(row[lo:hi].tolist())
        ref = math.fsum(t.tolist())
        nn = len(t) + 8
        gam = nn * 2.0 ** -53 / (1 - nn * 2.0 ** -53)
        assert abs(got - ref) <= gam * float(np.abs(t).sum()), f"column {j}: partials {got!r} against {ref!r}"


def check(res, A, launcher, mode, *, k=1, x, y0=None, aux0=None, aux1=None, aux2=None, rhs=None, dot_with=None, scale=0.0,
          s2=None, z32=False, exact=None, part=ALL, rows=None):
    """Bound for every row and column; bit for bit if `exact` (tile forms, SpMM); the partials.  Vectors [n] / [n][k].
    rows: the rows a part launch computes (the others must still hold the sentinel)."""
    spmm = launcher >= SPMM_MODE
    n, nc = A.shape
    f64 = launcher in F64_IN
    x32 = launcher == DOT_X32
    T = np.float64 if (f64 or x32) else np.float32          # the type the kernel computes in
    dt = np.longdouble if (f64 or x32) else np.float64       # the reference's
    u = 2.0 ** -53 if (f64 or x32) else 2.0 ** -24
    if exact is None:
        exact = res["form"] != WPR
    col = (lambda v, j: None if v is None else np.asarray(v).reshape(-1, k)[:, j]) if spmm else (lambda v, j: v)
    a_T = A.data.astype(T)
    A_T = sp.csr_matrix((a_T, A.indices, A.indptr), shape=A.shape)
    m = np.diff(A.indptr).astype(dt)
    s = T(scale)
    d = None if aux2 is None else np.asarray(aux2, T)
    ys = res["y"].read().reshape(-1, k) if spmm else res["y"].read()
    y2s = None
    if res["y2"] is not None:
        y2s = res["y2"].read().reshape(-1, k) if spmm else res["y2"].read()
    sel = np.ones(n, bool) if rows is None else rows
    for out in (ys, y2s):
        if out is not None and not z32:
            assert (out[~sel].view(np.uint8) == SENT).all(), "rows outside the launch's tiles were written"
    terms = []
    s2v = None if s2 is None else np.atleast_1d(np.asarray(s2, np.float64))
    for j in range(k):
        xj = np.asarray(col(x, j), np.float32 if x32 else T)
        om = 1.0
        if s2v is not None:
            om = math.sqrt(s2v[j]) if s2v[j] > 0 else 1.0
        yj = ys[:, j] if spmm else ys
        y2j = None if y2s is None else (y2s[:, j] if spmm else y2s)
        b = None if aux1 is None else np.asarray(col(aux1, j), T)
        # -- the restatement in the kernel's order and type
        if mode == RESID_PRE:
            xs = xj * (s * d)
            acc = A_T @ xs
        else:
            acc = A_T @ (xj.astype(np.float64) if x32 else xj)
        term = None
        if mode in (PLAIN, DOT, DOT_AUX):
            r_out = acc
            if mode != PLAIN:
                term = (xj[:n].astype(np.float64) if x32 else np.asarray(col(dot_with, j))) * yj
        elif mode == RESID:
            r_out = b - acc
        elif mode == RESID_PRE:
            r_out = xj[:n] - acc
        elif mode == ADD:
            r_out = np.asarray(col(y0, j), yj.dtype) + acc.astype(yj.dtype)
        elif mode == RESTRICT:
            r_out = acc
            assert np.array_equal(y2j[sel], ((s * d) * acc)[sel]) if exact else True
        elif mode == JACOBI:
            r_out = xj[:n] + (s * d) * (b - acc)
        elif mode == WUP:
            r = None if rhs is None else np.asarray(col(rhs, j), np.float32)
            r_out = (s * d) * (r + b) + acc if r is not None else np.asarray(col(aux0, j), T) + (s * d) * b + acc
        exit_dot = mode in (JACOBI, WUP) and (dot_with is not None or (spmm and rhs is not None))
        got_out = yj
        if exit_dot:
            zj = y2j if z32 else None
            if z32:
                assert exact is False or np.array_equal(zj[sel], r_out[sel]), f"column {j}: z32"
                outd = zj.astype(np.float64) * om
                got_out = zj
                assert res["y"].untouched(), "the double output was written beside z32"
            else:
                outd = r_out.astype(np.float64) * om
                if exact:
                    assert np.array_equal(yj[sel], outd[sel]), f"column {j}: {np.flatnonzero(yj[sel] != outd[sel])[:5]}"
                outd = yj
            if mode == WUP and rhs is not None:
                term = (np.asarray(col(rhs, j), np.float32).astype(np.float64) * om) * outd
            else:
                term = np.asarray(col(dot_with, j)) * outd
        else:
            if exact:
                bad = np.flatnonzero(sel & (yj != r_out.astype(yj.dtype)))
                assert bad.size == 0, f"column {j}: rows {bad[:5]} differ from the restatement: {yj[bad[:3]]} {r_out[bad[:3]]}"
            if mode == JACOBI:
                term = (b * yj.astype(T)).astype(np.float64)
        terms.append(None if term is None else term[sel])
        # -- the bound against the exact result
        acc_h, S = exact_rows(A, A.data.astype(T) if not x32 else A.data,
                              (xj.astype(dt) * (s.astype(dt) * d.astype(dt)) if mode == RESID_PRE else xj), dt)
        bh = None if b is None else b.astype(dt)
        sd = None if d is None else s.astype(dt) * d.astype(dt)
        c = BOUND_C[mode]
        if mode in (PLAIN, DOT, DOT_AUX, RESTRICT):
            ref, E = acc_h, S
            if mode == RESTRICT:
                bound_ok(y2j[sel], (sd * acc_h)[sel], (np.abs(sd) * S)[sel], m[sel], c, u)
                c = 1
        elif mode == RESID:
            ref, E = bh - acc_h, np.abs(bh) + S
        elif mode == RESID_PRE:
            xr = xj[:n].astype(dt)
            ref, E = xr - acc_h, np.abs(xr) + S
        elif mode == ADD:
            y0j = np.asarray(col(y0, j), yj.dtype).astype(dt)
            ref, E = y0j + acc_h, np.abs(y0j) + S
        elif mode == JACOBI:
            xr = xj[:n].astype(dt)
            ref, E = xr + sd * (bh - acc_h), np.abs(xr) + np.abs(sd) * (np.abs(bh) + S)
        else:
            if rhs is not None:
                rh = np.asarray(col(rhs, j), np.float32).astype(dt)
                ref, E = sd * (rh + bh) + acc_h, np.abs(sd) * (np.abs(rh) + np.abs(bh)) + S
            else:
                a0 = np.asarray(col(aux0, j), T).astype(dt)
                ref, E = a0 + sd * bh + acc_h, np.abs(a0) + np.abs(sd) * np.abs(bh) + S
        if exit_dot and not z32:
            omh = np.sqrt(np.asarray(s2v[j], dt)) if (s2v is not None and s2v[j] > 0) else dt(1)
            ref, E, c = ref * omh, E * omh, c + EXIT_EXTRA
        bound_ok(got_out[sel], ref[sel], E[sel], m[sel], c, u)
    if res["partials"] is not None:
        with_dot = mode in (DOT, DOT_AUX, JACOBI) or (mode == WUP and exit_dot)
        check_partials(res, terms if with_dot else None, k, part)


# ---- the cases -------------------------------------------------------------------------------------------------------

def inputs(A, k=1, seed=0, wide=False):
    rng = np.random.default_rng(seed)
    n, nc = A.shape
    sh = (lambda ln: ln * k)
    nd = max(n, nc)
    return dict(x=vals(rng, sh(nc), wide), y0=vals(rng, sh(n)), aux0=vals(rng, sh(n)), aux1=vals(rng, sh(n)),
                rhs=vals(rng, sh(n)), dot_with=vals(rng, sh(n)), aux2=rng.uniform(0.1, 0.9, nd) * rng.choice([-1.0, 1.0], nd))


SCALE = 0.6171875 + 2.0 ** -20          # representable in float32, not a power of two
S2 = 2.25 + 2.0 ** -30                  # out_scale2: its square root is neither 1 nor the value itself


def case(ctx, A, launcher, mode, *, k=1, flags=0, part=ALL, seed=0, wide=False, z32=False, use=(), partials=None, n_owned=0,
         M=None, expect=None, s2=None, exact=None, rows=None):
    """Run one product with the inputs `use` names (x always) and check it; returns the run's record.  1/diag (aux2) is per row,
    or per column for RESID_PRE (square)."""
    v = inputs(A, k, seed, wide)
    kw = {nm: v[nm] for nm in use}
    kw["x"] = v["x"]
    if "aux2" in kw:
        kw["aux2"] = kw["aux2"][:A.shape[1] if mode == RESID_PRE else A.shape[0]]
        kw["scale"] = SCALE
    if s2 is not None:
        kw["s2"] = s2
    if launcher in (SPMV_MODE, SPMV_PART, SPMM_MODE, DOT_X32, F32_EXIT, F32_EXIT_PART, F32_WUP_EXIT, SPMM_F32_EXIT,
                    SPMM_F32_WUP_EXIT, F32, F32_PART, SPMM_F32):
        want_p = True if partials is None else partials
    else:
        want_p = False
    M = M if M is not None else ctx.csr_from_scipy(A)
    res = run(ctx, M, launcher, A, mode=mode, k=k, part=part, flags=flags, n_owned=n_owned, z32=z32, partials=want_p, **kw)
    if expect is not None:
        assert FNAME[res["form"]] == expect[0], f"{LNAME[launcher]} mode {mode}: form {FNAME[res['form']]}, not {expect[0]}"
        if len(expect) > 1:
            assert res["xw_run"] == expect[1], f"x windows of {res['xw_run']}, not {expect[1]}"
    kw.pop("scale", None)
    check(res, A, launcher, mode, k=k, z32=z32, exact=exact, part=part, scale=SCALE if "aux2" in kw else 0.0, rows=rows, **kw)
    return res


SIZES = (0, 1, 63, 64, 65, 257, 4095, 4097)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_f64_epilogues_on_the_gather_tile(ctx, n):
    """launch_spmv_mode: every epilogue the f64 cycle and the CG loop use, at the edge sizes of tiles, workgroups and slabs."""
    A = ragged(n, n, 7, 10 + n, empty_tile=1)
    M = ctx.csr_from_scipy(A)
    form = ("none",) if n == 0 else ("tile", 0)
    case(ctx, A, SPMV_MODE, PLAIN, M=M, expect=form)
    case(ctx, A, SPMV_MODE, DOT, use=("dot_with",), M=M, expect=form)
    case(ctx, A, SPMV_MODE, DOT_AUX, use=("dot_with",), M=M, expect=form)
    case(ctx, A, SPMV_MODE, RESID, use=("aux1",), M=M, expect=form)
    case(ctx, A, SPMV_MODE, ADD, use=("y0",), M=M, expect=form)
    case(ctx, A, SPMV_MODE, JACOBI, use=("aux1", "aux2"), M=M, expect=form)


@gpu
@pytest.mark.parametrize("shape", [(300, 4097), (4097, 300), (1000, 1100)])
def test_rectangular_and_long_rows(ctx, shape):
    """R-like (few rows, many columns: PLAIN, the restriction) and P-like (ADD) shapes; rows of 511..1025 entries that straddle
    a gather pass, the 16-per-lane pass and the SpMM chunk, and a hub row of several thousand."""
    n, nc = shape
    A = ragged(n, nc, 6, 7 + n, long_rows=(511, 512, 513, 1023, 1024, 1025) if nc > 1025 else (), hub=3000 if nc > 3000 else 0)
    M = ctx.csr_from_scipy(A)
    case(ctx, A, SPMV_MODE, PLAIN, M=M, expect=("tile", 0))
    case(ctx, A, SPMV_MODE, ADD, use=("y0",), M=M)
    case(ctx, A, F32, PLAIN, M=M, flags=BF32)
    case(ctx, A, F32, ADD, use=("y0",), M=M, flags=BF32)
    if n <= nc:
        case(ctx, A, F32_RESTRICT, RESTRICT, use=("aux2",), M=M, flags=BF32)
    for k in (8, 4, 2):
        case(ctx, A, SPMM_F32, PLAIN, k=k, M=M, flags=BF32, expect=("tile",))
        case(ctx, A, SPMM_F32, ADD, k=k, use=("y0",), M=M, flags=BF32)
        case(ctx, A, SPMM_MODE, PLAIN, k=k, M=M)


@gpu
@pytest.mark.parametrize("n", (63, 257, 4097))
def test_f32_cycle_epilogues_on_the_gather_tile(ctx, n):
    """launch_spmv_f32 / _restrict / _resid_pre / _exit / _wup / _wup_exit on a short-row operator (the plain tile kernel)."""
    A = ragged(n, n, 4, 20 + n, empty_tile=0)
    M = ctx.csr_from_scipy(A)
    fl = BF32 | DINV
    e = ("tile", 0)
    case(ctx, A, F32, PLAIN, M=M, flags=fl, expect=e)
    case(ctx, A, F32, RESID, use=("aux1",), M=M, flags=fl, expect=e)
    case(ctx, A, F32, ADD, use=("y0",), M=M, flags=fl, expect=e)
    case(ctx, A, F32, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e)
    case(ctx, A, F32_PART, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e)
    case(ctx, A, F32_RESTRICT, RESTRICT, use=("aux2",), M=M, flags=fl, expect=e)
    case(ctx, A, F32_RESID_PRE, RESID_PRE, use=("aux2",), M=M, flags=fl, expect=e)
    for z in (False, True):
        case(ctx, A, F32_EXIT, JACOBI, use=("aux1", "aux2", "dot_with"), s2=S2, z32=z, M=M, flags=fl, expect=e)
        case(ctx, A, F32_EXIT_PART, JACOBI, use=("aux1", "aux2", "dot_with"), s2=S2, z32=z, M=M, flags=fl, expect=e)
        case(ctx, A, F32_WUP_EXIT, WUP, use=("aux0", "aux1", "aux2", "dot_with"), s2=S2, z32=z, M=M, flags=fl, expect=e)
        case(ctx, A, F32_WUP_EXIT, WUP, use=("aux1", "aux2", "dot_with", "rhs"), s2=S2, z32=z, M=M, flags=fl, expect=e)
    case(ctx, A, F32_WUP, WUP, use=("aux0", "aux1", "aux2"), M=M, flags=fl, expect=e)
    p = np.random.default_rng(n).uniform(0.5, 2, n) * np.random.default_rng(n + 1).choice([-1, 1], n)
    res = run(ctx, M, DOT_X32, A, mode=DOT, x=p.astype(np.float32))
    assert FNAME[res["form"]] == "tile"
    check(res, A, DOT_X32, DOT, x=p.astype(np.float32))


@gpu
@pytest.mark.parametrize("k", (8, 4, 2))
@pytest.mark.parametrize("n", (65, 1000, 4097))
def test_spmm_columns_are_the_restated_single_products(ctx, k, n):
    """Every SpMM form and epilogue, each column bit for bit the sequential product plus epilogue, with a different
    out_scale2 per column (a swapped sqrt(out_scale2[j]) is seen) and per-column partial sums."""
    A = ragged(n, n, 9, 30 + n + k, long_rows=(511, 512, 513) if n > 513 else ())
    M = ctx.csr_from_scipy(A)
    fl = BF32
    s2 = 1.5 + np.arange(k) * 0.75 + 2.0 ** -29
    case(ctx, A, SPMM_MODE, PLAIN, k=k, M=M)
    case(ctx, A, SPMM_MODE, DOT, k=k, use=("dot_with",), M=M)
    case(ctx, A, SPMM_F32, RESID, k=k, use=("aux1",), M=M, flags=fl)
    case(ctx, A, SPMM_F32, JACOBI, k=k, use=("aux1", "aux2"), M=M, flags=fl)
    case(ctx, A, SPMM_F32_WUP, WUP, k=k, use=("aux0", "aux1", "aux2"), M=M, flags=fl)
    for z in (False, True):
        case(ctx, A, SPMM_F32_EXIT, JACOBI, k=k, use=("aux1", "aux2", "dot_with"), s2=s2, z32=z, M=M, flags=fl)
        case(ctx, A, SPMM_F32_WUP_EXIT, WUP, k=k, use=("aux0", "aux1", "aux2", "dot_with"), s2=s2, z32=z, M=M, flags=fl)
        case(ctx, A, SPMM_F32_WUP_EXIT, WUP, k=k, use=("aux1", "aux2", "rhs"), s2=s2, z32=z, M=M, flags=fl)


@gpu
def test_long_form(ctx):
    """The 16-per-lane gather form: f32, more than 8.5 entries per row, fewer than 500 000 rows, no plan."""
    A = ragged(5000, 5000, 12, 40, empty_tile=2, long_rows=(511, 512, 513, 1023, 1024, 1025), hub=4000)
    assert A.nnz > 8.5 * A.shape[0]
    M = ctx.csr_from_scipy(A)
    fl = BF32
    e = ("long",)
    case(ctx, A, F32, PLAIN, M=M, flags=fl, expect=e)
    case(ctx, A, F32, RESID, use=("aux1",), M=M, flags=fl, expect=e)
    case(ctx, A, F32, ADD, use=("y0",), M=M, flags=fl, expect=e)
    case(ctx, A, F32, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e)
    case(ctx, A, F32_PART, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e)
    case(ctx, A, F32_RESTRICT, RESTRICT, use=("aux2",), M=M, flags=fl, expect=e)
    # (double output, and the W product: not the long form)
    case(ctx, A, F32_EXIT, JACOBI, use=("aux1", "aux2", "dot_with"), s2=S2, M=M, flags=fl, expect=("tile", 0))
    case(ctx, A, F32_EXIT, JACOBI, use=("aux1", "aux2", "dot_with"), s2=S2, z32=True, M=M, flags=fl, expect=e)
    case(ctx, A, F32_WUP, WUP, use=("aux0", "aux1", "aux2"), M=M, flags=fl, expect=("tile", 0))
    A2 = ragged(4096, 4096, 12, 41)
    assert A2.nnz > 8.5 * A2.shape[0]
    case(ctx, A2, F32, RESID, use=("aux1",), flags=fl, expect=e)


@gpu
@pytest.mark.parametrize("shape,per_row", [((1000, 1000), 40), ((4096, 4096), 10), ((4097, 4097), 30), ((300, 2000), 40),
                                           ((2000, 300), 30), ((64, 64), 20)])
def test_wave_per_row(ctx, shape, per_row):
    """Hierarchy operators with dense rows: the wave-per-row kernel sums in a shuffle tree, so the bound alone (no bit check)."""
    n, nc = shape
    A = ragged(n, nc, per_row, 50 + n, long_rows=(1023, 1024, 1025) if nc > 1025 else ())
    M = ctx.csr_from_scipy(A)
    fl = HIER | BF32
    e = ("wpr",)
    case(ctx, A, SPMV_MODE, PLAIN, M=M, flags=fl, expect=e, exact=False)
    case(ctx, A, SPMV_MODE, ADD, use=("y0",), M=M, flags=fl, expect=e, exact=False)
    case(ctx, A, F32, PLAIN, M=M, flags=fl, expect=e, exact=False)
    case(ctx, A, F32, ADD, use=("y0",), M=M, flags=fl, expect=e, exact=False)
    if n <= nc:
        case(ctx, A, F32_RESTRICT, RESTRICT, use=("aux2",), M=M, flags=fl, expect=e, exact=False)
    if n == nc:
        case(ctx, A, SPMV_MODE, RESID, use=("aux1",), M=M, flags=fl, expect=e, exact=False)
        case(ctx, A, SPMV_MODE, DOT_AUX, use=("dot_with",), M=M, flags=fl, expect=e, exact=False)
        case(ctx, A, SPMV_MODE, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e, exact=False)
        case(ctx, A, F32, RESID, use=("aux1",), M=M, flags=fl, expect=e, exact=False)
        case(ctx, A, F32, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e, exact=False)
        case(ctx, A, F32_PART, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e, exact=False)
        case(ctx, A, F32_WUP, WUP, use=("aux0", "aux1", "aux2"), M=M, flags=fl, expect=e, exact=False)
        # the exit stage in the W form has no wave-per-row form: the tile kernel, bit for bit
        case(ctx, A, F32_WUP_EXIT, WUP, use=("aux0", "aux1", "aux2", "dot_with"), s2=S2, M=M, flags=fl, expect=("tile", 0))


@gpu
@pytest.mark.parametrize("half,run_len", [(3, 72), (20, 128)])
def test_x_window_forms(ctx, half, run_len):
    """>= 65 536 rows of three bands: tiles on runs of 72 (or 128), tiles with far columns that keep the gather path, the last
    window ending at an n_cols that is not a multiple of 4.  f64, f32, x32 and the windowed staging of RESID_PRE."""
    n = 70001 if half == 3 else 65603
    A = banded(n, n, half, 60 + half, keep=0.5 if half == 3 else 0.3)
    M = ctx.csr_from_scipy(A)
    fl = XW | BF32 | DINV
    e = ("tile", run_len)
    case(ctx, A, SPMV_MODE, DOT, use=("dot_with",), M=M, flags=fl, expect=e)
    case(ctx, A, SPMV_MODE, PLAIN, M=M, flags=fl, expect=e, seed=1, wide=True)
    case(ctx, A, SPMV_MODE, RESID, use=("aux1",), M=M, flags=fl, expect=e)
    case(ctx, A, SPMV_MODE, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e)
    case(ctx, A, F32, RESID, use=("aux1",), M=M, flags=fl, expect=e)
    case(ctx, A, F32_PART, JACOBI, use=("aux1", "aux2"), M=M, flags=fl, expect=e)
    case(ctx, A, F32_RESID_PRE, RESID_PRE, use=("aux2",), M=M, flags=fl, expect=e)
    case(ctx, A, F32_EXIT, JACOBI, use=("aux1", "aux2", "dot_with"), s2=S2, M=M, flags=fl, expect=e)
    case(ctx, A, F32_EXIT, JACOBI, use=("aux1", "aux2", "dot_with"), s2=S2, z32=True, M=M, flags=fl, expect=e)
    rng = np.random.default_rng(half)
    for wide in (False, True):
        p = vals(rng, n, wide).astype(np.float32)
        res = run(ctx, M, DOT_X32, A, mode=DOT, x=p, flags=fl)
        assert (FNAME[res["form"]], res["xw_run"]) == e
        check(res, A, DOT_X32, DOT, x=p)


@gpu
def test_wide_plan_of_the_w_product(ctx):
    """A W-shaped f32 operator the wide builder accepts: twelve runs of 20 per tile, tiles with far columns gathering."""
    A = w_like(70001, 70)
    M = ctx.csr_from_scipy(A)
    fl = BF32 | XW_WIDE
    e = ("wide", 20)
    case(ctx, A, F32_WUP, WUP, use=("aux0", "aux1", "aux2"), M=M, flags=fl, expect=e)
    for z in (False, True):
        case(ctx, A, F32_WUP_EXIT, WUP, use=("aux0", "aux1", "aux2", "dot_with"), s2=S2, z32=z, M=M, flags=fl, expect=e)
        case(ctx, A, F32_WUP_EXIT, WUP, use=("aux1", "aux2", "dot_with", "rhs"), s2=S2, z32=z, M=M, flags=fl, expect=e)
    for k in (8, 2):
        case(ctx, A, SPMM_F32_WUP_EXIT, WUP, k=k, use=("aux1", "aux2", "rhs"), s2=1.25 + np.arange(k), M=M, flags=fl)


def split_matrix(n_owned, halo, seed):
    """A row-partitioned operator: n_owned rows, columns n_owned + halo; a third of the tiles read an exchange slot (boundary)."""
    A = H.random_csr(n_owned, n_owned, 5, seed)
    A.resize((n_owned, n_owned + halo))
    rng = np.random.default_rng(seed)
    far = rng.choice(np.arange(5, n_owned, 64), n_owned // 64 // 3, replace=False)
    B = sp.csr_matrix((np.ones(len(far)), (far, n_owned + rng.integers(0, halo, len(far)))), shape=A.shape)
    return with_values(A + B, seed + 1)


def part_rows(A, n_owned, part):
    """The rows of the tiles a part launch covers: boundary tiles read a column >= n_owned, interior tiles do not."""
    row_of = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    bnd = np.zeros((A.shape[0] + 63) // 64, bool)
    bnd[row_of[A.indices >= n_owned] // 64] = True
    rows = np.repeat(bnd, 64)[:A.shape[0]]
    return rows if part == BOUNDARY else ~rows


@gpu
@pytest.mark.parametrize("n_owned", (4096, 9000, 70000))
def test_interior_and_boundary_lists(ctx, n_owned):
    """The LIST launches of a split operator: interior tiles, boundary tiles (their partial sums start at partial_off), and both
    (a product with partial sums over the whole operator).  Rows of the other part keep the sentinel, nothing is written beyond."""
    A = split_matrix(n_owned, 300, 80 + n_owned)
    M = ctx.csr_from_scipy(A)
    fl = SPLIT | BF32
    kw = dict(M=M, flags=fl, n_owned=n_owned, expect=("list",))
    r = case(ctx, A, SPMV_MODE, DOT, use=("dot_with",), **kw)
    assert r["n_bnd"] > 0 and r["n_int"] > 0 and r["off_bnd"] > 0
    case(ctx, A, SPMV_MODE, JACOBI, use=("aux1", "aux2"), **kw)
    for part in (INTERIOR, BOUNDARY):
        rows = part_rows(A, n_owned, part)
        case(ctx, A, SPMV_PART, DOT, part=part, use=("dot_with",), rows=rows, **kw)
        case(ctx, A, SPMV_PART, RESID, part=part, use=("aux1",), rows=rows, **kw)
        case(ctx, A, SPMV_PART, JACOBI, part=part, use=("aux1", "aux2"), rows=rows, **kw)
        case(ctx, A, F32_PART, RESID, part=part, use=("aux1",), rows=rows, **kw)
        case(ctx, A, F32_PART, JACOBI, part=part, use=("aux1", "aux2"), rows=rows, **kw)
        case(ctx, A, F32_EXIT_PART, JACOBI, part=part, use=("aux1", "aux2", "dot_with"), s2=S2, rows=rows, **kw)


@gpu
def test_dynamic_range_separates_the_accumulators(ctx):
    """Values over 1e-6 ... 1e6: the f64 bound holds for the f64 forms and the x32 product (a float accumulator would miss it by
    orders of magnitude), the f32 bound for the f32 forms."""
    A = with_values(H.random_csr(4097, 4097, 9, 99), 98, wide=True)
    M = ctx.csr_from_scipy(A)
    case(ctx, A, SPMV_MODE, DOT, use=("dot_with",), M=M, wide=True, expect=("tile", 0))
    case(ctx, A, F32, RESID, use=("aux1",), M=M, wide=True, flags=BF32)
    p = vals(np.random.default_rng(97), 4097, True).astype(np.float32)
    res = run(ctx, M, DOT_X32, A, mode=DOT, x=p)
    check(res, A, DOT_X32, DOT, x=p)


def test_x32_bound_rejects_a_float_accumulator():
    """Host only: the bound the x32 product is held to fails for the same product accumulated in float32 -- the test can tell
    the two precisions apart."""
    for wide in (False, True):
        A = with_values(H.random_csr(4097, 4097, 9, 99), 98, wide=wide)
        p = vals(np.random.default_rng(97), 4097, wide).astype(np.float32)
        a32 = sp.csr_matrix((A.data.astype(np.float32), A.indices, A.indptr), shape=A.shape)
        y_f32 = (a32 @ p).astype(np.float64)
        y_f64acc = (a32.astype(np.float64) @ p.astype(np.float64)).astype(np.float32).astype(np.float64)   # rounded through float
        ref, S = exact_rows(A, A.data, p, np.longdouble)
        m = np.diff(A.indptr).astype(np.longdouble)
        for bad in (y_f32, y_f64acc):
            with pytest.raises(AssertionError):
                bound_ok(bad, ref, S, m, BOUND_C[DOT], 2.0 ** -53)
        bound_ok(A @ p.astype(np.float64), ref, S, m, BOUND_C[DOT], 2.0 ** -53)


@gpu
def test_stop_word_leaves_every_output_and_partial_at_its_sentinel(ctx):
    """*done_flag = 1: every form returns before its first store -- outputs (ADD: the input y), y2, z32 and partial slots."""
    A = ragged(4097, 4097, 12, 5)
    A4 = ragged(4097, 4097, 4, 4)
    Ab = banded(70001, 70001, 3, 6)
    Aw = w_like(70001, 7)
    Ah = ragged(1000, 1000, 40, 8)
    As = split_matrix(9000, 300, 9)
    rng = np.random.default_rng(0)
    todo = [(A, 0, SPMV_MODE, DOT, 1, ALL, False), (A, 0, SPMV_MODE, ADD, 1, ALL, False), (A, BF32, F32, RESID, 1, ALL, False),
            (A, BF32, F32_RESTRICT, RESTRICT, 1, ALL, False), (A, BF32, F32_EXIT, JACOBI, 1, ALL, True),
            (A, BF32, F32_WUP_EXIT, WUP, 1, ALL, True), (A4, BF32 | DINV, F32_RESID_PRE, RESID_PRE, 1, ALL, False),
            (A, 0, DOT_X32, DOT, 1, ALL, False), (Ab, XW | BF32, F32_EXIT, JACOBI, 1, ALL, False),
            (Ab, XW, SPMV_MODE, DOT, 1, ALL, False), (Aw, BF32 | XW_WIDE, F32_WUP_EXIT, WUP, 1, ALL, True),
            (Ah, HIER | BF32, F32, JACOBI, 1, ALL, False), (Ah, HIER, SPMV_MODE, JACOBI, 1, ALL, False),
            (As, SPLIT, SPMV_PART, DOT, 1, BOUNDARY, False), (As, SPLIT, SPMV_MODE, DOT, 1, ALL, False),
            (A, 0, SPMM_MODE, DOT, 8, ALL, False), (A, BF32, SPMM_F32_EXIT, JACOBI, 4, ALL, True),
            (A, BF32, SPMM_F32_WUP_EXIT, WUP, 2, ALL, True), (A, BF32, SPMM_F32, ADD, 8, ALL, False)]
    for M_, fl, launcher, mode, k, part, z in todo:
        n, nc = M_.shape
        kk = k if launcher >= SPMM_MODE else 1
        x = vals(rng, nc * kk).astype(np.float32 if launcher == DOT_X32 else np.float64)
        kw = dict(x=x, y0=vals(rng, n * kk), aux0=vals(rng, n * kk), aux1=vals(rng, n * kk), aux2=rng.uniform(0.1, 0.9, n),
                  dot_with=vals(rng, n * kk), scale=SCALE, s2=np.full(kk, S2))
        if launcher == F32_WUP_EXIT or launcher == SPMM_F32_WUP_EXIT:
            kw["rhs"] = vals(rng, n * kk)
        res = run(ctx, ctx.csr_from_scipy(M_), launcher, M_, mode=mode, k=k, part=part, flags=fl, n_owned=n if fl & SPLIT else 0,
                  z32=z, done=True, **kw)
        assert res["y"].untouched(), f"{LNAME[launcher]} wrote y behind the stop word"
        if res["y2"] is not None:
            assert res["y2"].untouched(), f"{LNAME[launcher]} wrote y2 behind the stop word"
        assert (res["partials"].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF)).all(), LNAME[launcher]


# the launcher / epilogue pairs the solver calls (launch_spm* in amg.hip, pcg.hip, kkt.hip, capi.hip), crossed with the forms
# each takes there: (launcher, mode, k, form, x-window run)
REQUIRED = set()
for _run in (0, 72, 128):
    REQUIRED |= {("spmv_mode", DOT, 1, "tile", _run), ("spmv_mode", PLAIN, 1, "tile", _run),
                 ("spmv_dot_x32", DOT, 1, "tile", _run), ("spmv_f32_resid_pre", RESID_PRE, 1, "tile", _run),
                 ("spmv_f32", RESID, 1, "tile", _run), ("spmv_f32_part", JACOBI, 1, "tile", _run),
                 ("spmv_f32_exit", JACOBI, 1, "tile", _run)}
REQUIRED |= {("spmv_mode", m_, 1, "tile", 0) for m_ in (RESID, ADD, JACOBI, DOT_AUX)}
REQUIRED |= {("spmv_mode", m_, 1, "wpr", 0) for m_ in (PLAIN, RESID, ADD, JACOBI, DOT_AUX)}
REQUIRED |= {("spmv_mode", DOT, 1, "list", 0), ("spmv_part", DOT, 1, "list", 0)}
REQUIRED |= {("spmv_f32", m_, 1, f_, 0) for m_ in (PLAIN, RESID, ADD) for f_ in ("tile", "wpr", "long")}
REQUIRED |= {("spmv_f32_part", m_, 1, "list", 0) for m_ in (RESID, JACOBI)}
REQUIRED |= {("spmv_f32_part", JACOBI, 1, f_, 0) for f_ in ("wpr", "long")}
REQUIRED |= {("spmv_f32_restrict", RESTRICT, 1, f_, 0) for f_ in ("tile", "wpr", "long")}
REQUIRED |= {("spmv_f32_exit", JACOBI, 1, "long", 0), ("spmv_f32_exit_part", JACOBI, 1, "list", 0),
             ("spmv_f32_exit_part", JACOBI, 1, "tile", 0)}
REQUIRED |= {("spmv_f32_wup", WUP, 1, f_, r_) for f_, r_ in (("tile", 0), ("wide", 20), ("wpr", 0))}
REQUIRED |= {("spmv_f32_wup_exit", WUP, 1, f_, r_) for f_, r_ in (("tile", 0), ("wide", 20))}
for _k in (8, 4, 2):
    REQUIRED |= {("spmm_mode", PLAIN, _k, "tile", 0), ("spmm_mode", DOT, _k, "tile", 0)}
    REQUIRED |= {("spmm_f32", m_, _k, "tile", 0) for m_ in (RESID, PLAIN, ADD, JACOBI)}
    REQUIRED |= {("spmm_f32_exit", JACOBI, _k, "tile", 0), ("spmm_f32_wup", WUP, _k, "tile", 0),
                 ("spmm_f32_wup_exit", WUP, _k, "tile", 0)}


@gpu
def test_every_solver_product_form_was_reached():
    """Last: the cases above reached every (launcher, epilogue, width, form, run) the solver uses -- a path that silently stops
    being exercised fails here."""
    if not REACHED:
        pytest.skip("run with the rest of the module")
    missing = sorted(REQUIRED - REACHED)
    assert not missing, f"not reached: {missing}"

"""The one-GPU multigrid loop ends in the iteration that converges (needs an MI355X).

Since pcg_decide_kernel the books of an iteration -- count, ||r||^2, the stopping decision, the step length of the kept
directions -- are kept behind the x/r update and before the cycle; in the iteration that converges the cycle and the p update
do no work.  What a caller sees must not move: the iteration that stops, x as the sum of the kept directions up to and
including that iteration, the cap, the ring of kept directions that wraps, a start from a guess and a restart from the true
residual.  The Jacobi loop and the lockstep groups keep their kernels: their figures are those of the commit before.

Reference, systems' construction, tolerances and the comparisons themselves are those of tests/test_pcg_vs_reference.py,
imported from there: textbook PCG on the host in np.longdouble (tests/pcg_ref.py) with the device's own cycle as a black box,
the bound 100 * max(d_host(k), 2^-53) of `calibrated` / `check_iterate`, the stopping rule of `check_stop`.

Systems: synthetic.layered_system(2, 40, 40) -- 3199 unknowns, two levels, 13 workgroups in the vector kernels -- and
(2, 90, 90) -- 16199 unknowns, three levels.  The tolerances are chosen from the reference's own residuals (||r_k|| / ||b||
of the longdouble run, measured once):
    (2, 40, 40):  k = 13: 1.63e-8   14: 5.06e-9   15: 1.40e-9   16: 3.39e-10      rtol 1e-8 stops at 14, 1e-9 at 16
    (2, 90, 90):  k = 11: 1.38e-6   12: 3.95e-7   14: 2.95e-8   15: 8.40e-9       rtol 1e-8 stops at 15, 1e-6 at 12
-- every tolerance 19 % or more from the residuals on either side of it, where check_stop asks for 0.1 %.
"""
import functools

import numpy as np
import pytest

import pcg_ref as R
import test_pcg_vs_reference as T
from padne_amd import _hip

gpu = pytest.mark.gpu
LD = np.longdouble
CHECK_EVERY = 4                                            # the loop's default: iterations queued between two host looks

SYSTEMS = {"n3199": (2, 40, 40), "n16199": (2, 90, 90)}
# rtol -> the iteration the reference stops at: one between two host looks, one at a host look
STOPS = {"n3199": {1e-8: 14, 1e-9: 16}, "n16199": {1e-8: 15, 1e-6: 12}}


def system(name):
    return T.layered_spd(*SYSTEMS[name], 4)


@functools.lru_cache(maxsize=None)
def reference(name, guess):
    """(x0, ld, d_host): the longdouble run and its calibration (test_pcg_vs_reference.calibrated) for the default loop --
    single-precision cycle, search direction kept in single precision -- computed once and shared.  The preconditioner is the
    device's cycle in the loop's unit: ||b||, from a guess ||r_0||."""
    from padne_amd import solver
    A, b = system(name)
    d = solver.get_context().csr_from_scipy(A)
    T.capped(d, b, 1, precond="amg")                       # (builds the hierarchy)
    x0 = None
    unit = float(np.linalg.norm(b))
    if guess:
        cold = d.solve_spd(b, rtol=1e-10, precond="amg")
        x0 = cold.x * (1.0 + 1e-3 * np.random.default_rng(5).uniform(-1, 1, len(b)))
        unit = float(R.norm(b.astype(LD) - R.product(A, LD)(x0.astype(LD))))
    ld, d_host = T.calibrated(A, b, 24, M=T.cycle_operator(d, unit, False), x0=x0, p32=True, r32_unit=unit)
    return x0, ld, d_host


def same_bits(a, b):
    return (a.iterations == b.iterations and a.restarts == b.restarts and a.status == b.status and np.array_equal(a.x, b.x)
            and a.rel_residual == b.rel_residual and a.abs_residual == b.abs_residual)


# ---- 1. the iteration that converges, between two host looks and at one ---------------------------------------------------

@gpu
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_stops_in_the_iteration_that_converges(ctx, name):
    """iterations is the reference's count (check_stop, with the reference run deciding), x the reference's iterate of that
    count (check_iterate), the reported residuals the true ones; a second run gives the same bits."""
    A, b = system(name)
    _, ld, d_host = reference(name, False)
    d = ctx.csr_from_scipy(A)
    assert d.solve_spd(b, rtol=1e-30, max_iter=1, raise_on_fail=False, precond="amg").levels >= 2
    counts = []
    for rtol, k in STOPS[name].items():
        res = d.solve_spd(b, rtol=rtol, precond="amg")
        T.check_stop(A, b, res, rtol, 0.0, ld)
        assert res.iterations == k
        T.check_iterate(f"stop/{name}/rtol={rtol:g}", k, res.x, ld, d_host)
        assert same_bits(d.solve_spd(b, rtol=rtol, precond="amg"), res)
        counts.append(res.iterations)
    assert counts[0] % CHECK_EVERY != 0 and counts[1] % CHECK_EVERY == 0


# ---- 2. the cap ----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_cap_of_three_iterations(ctx, name):
    """max_iter = 3: three iterations, not converged (`capped` asserts the status), x the reference's third iterate."""
    A, b = system(name)
    _, ld, d_host = reference(name, False)
    d = ctx.csr_from_scipy(A)
    res = T.capped(d, b, 3, precond="amg")
    assert res.iterations == 3 and res.status == _hip.E_NOTCONVERGED
    T.check_iterate(f"cap/{name}", 3, res.x, ld, d_host)
    assert same_bits(T.capped(d, b, 3, precond="amg"), res)


# ---- 3. a ring of kept directions that wraps -------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_ring_of_eight_that_wraps_gives_the_bits_of_the_running_update(ctx, switches, name):
    """17 and 19 iterations in a ring of eight places (two wraps, the last flush a partial one) against x += alpha p in every
    iteration (PADNE_PCG_NO_XHIST=1, where the update of the converging iteration rides on the p update): the same bits."""
    A, b = system(name)
    runs = {}
    for config in ("xhist_small", "no_xhist", "default"):
        T.set_config(switches, config)
        runs[config] = ctx.csr_from_scipy(A).solve_spd(b, rtol=1e-10, precond="amg")
        for var in T.CONFIGS[config]:
            switches.unset(var)
    assert runs["no_xhist"].status == _hip.OK and runs["no_xhist"].restarts == 0 and runs["no_xhist"].iterations > 16
    assert same_bits(runs["xhist_small"], runs["no_xhist"])
    assert same_bits(runs["default"], runs["no_xhist"])


# ---- 4. from a guess, and a restart ------------------------------------------------------------------------------------------------

# from the guess the reference's ||r_k|| / ||b|| are  (2, 40, 40): 6: 2.72e-6, 7: 6.37e-7;  (2, 90, 90): 7: 2.41e-6, 8: 6.29e-7
# (7 and 8 iterations where a start from zero takes 10 and 12).  Not tighter: check_stop holds the reported residual to the
# longdouble one to 1e-6 of it, which a double-precision b - A x delivers down to about 1e-9 ||b|| on these systems
GUESS_RTOL = 1e-6


@gpu
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_start_from_a_guess(ctx, name):
    """From a solution perturbed by 1e-3: fewer iterations than from zero, the count, x and the residuals the reference's."""
    A, b = system(name)
    x0, ld, d_host = reference(name, True)
    d = ctx.csr_from_scipy(A)
    cold = d.solve_spd(b, rtol=GUESS_RTOL, precond="amg")
    res = d.solve_spd(b, rtol=GUESS_RTOL, x0=x0, precond="amg")
    T.check_stop(A, b, res, GUESS_RTOL, 0.0, ld)
    assert 0 < res.iterations < cold.iterations
    T.check_iterate(f"guess/{name}", res.iterations, res.x, ld, d_host)
    assert same_bits(d.solve_spd(b, rtol=GUESS_RTOL, x0=x0, precond="amg"), res)


@gpu
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_restart_from_the_true_residual(ctx, switches, name):
    """rtol = 1e-14 from the guess: the recurrence converges above the true residual and the loop restarts (status words
    zeroed, the first direction in place 0 again).  The stopping rule holds for the TRUE residual, which is what is reported;
    a second run and the running update of x (PADNE_PCG_NO_XHIST=1) give the same bits.

    At 1e-14 ||b|| the residual is what binary64 can evaluate, so the reported residual -- the device's b - A x in double --
    is held to the longdouble one within the rounding of that evaluation: a row's sum of m products and the subtraction err
    by at most (m + 2) 2^-53 (|A||x| + |b|) (Higham, Accuracy and Stability, 3.5: gamma_{m+1}, m + 2 for its second-order
    term), in any order of the sum; the norms of two vectors differ by at most the norm of their difference.  Measured:
    floor / ||b|| = 1.3e-13 and 3.2e-13; |reported - true| / ||b|| = 8.6e-16 and 2.5e-15."""
    A, b = system(name)
    x0, _, _ = reference(name, True)
    rtol = 1e-14
    res = ctx.csr_from_scipy(A).solve_spd(b, rtol=rtol, x0=x0, precond="amg")
    assert res.status == _hip.OK and res.restarts >= 1 and res.precond_fallbacks == 0
    nb, true = R.norm(b.astype(LD)), T.true_residual(A, b, res.x)
    m = int(np.diff(A.indptr).max())
    floor = (m + 2) * T.U * R.norm((abs(A) @ np.abs(res.x) + np.abs(b)).astype(LD))
    print(f"PCGRESTART {name} iterations={res.iterations} restarts={res.restarts} true/||b||={float(true / nb):.3e} "
          f"reported={res.rel_residual:.3e} floor/||b||={float(floor / nb):.3e} "
          f"|reported-true|/||b||={float(abs(res.abs_residual - true) / nb):.3e}")
    assert abs(res.abs_residual - true) <= floor + 1e-6 * true
    assert abs(res.rel_residual * nb - true) <= floor + 1e-6 * true
    # (padne_hip.h, as solve_one applies it behind restarts that stagnate at what binary64 can evaluate: within 10x of the
    # request, for the residual as the device evaluates it)
    assert res.rel_residual <= 10 * rtol and true <= 10 * LD(rtol) * nb + floor
    assert same_bits(ctx.csr_from_scipy(A).solve_spd(b, rtol=1e-14, x0=x0, precond="amg"), res)
    switches.set("PADNE_PCG_NO_XHIST", "1")
    assert same_bits(ctx.csr_from_scipy(A).solve_spd(b, rtol=1e-14, x0=x0, precond="amg"), res)


# ---- 5. the loops that keep their kernels ------------------------------------------------------------------------------------------

# measured with the commit before this test (rtol = 1e-9 on the 3199 unknowns): iterations, rel_residual, abs_residual
JACOBI_BEFORE = (283, float.fromhex("0x1.04219894e5029p-30"), float.fromhex("0x1.6fe19110b9579p-30"))
LOCKSTEP8_BEFORE = (112, float.fromhex("0x1.f0016dc3baad1p-32"), float.fromhex("0x1.5eba99d729a53p-28"))


@gpu
def test_jacobi_loop_and_lockstep_group_are_untouched(ctx):
    """Deterministic kernels that did not change, on inputs that are the same bits on every host (sparse assembly by sums and
    products, right-hand sides of small integers): the same figures to the bit."""
    A, b = system("n3199")
    d = ctx.csr_from_scipy(A)
    res = d.solve_spd(b, rtol=1e-9, precond="jacobi")
    print(f"PCGBEFORE jacobi {res.iterations} {float(res.rel_residual).hex()} {float(res.abs_residual).hex()}")
    assert res.status == _hip.OK and res.restarts == 0
    assert (res.iterations, res.rel_residual, res.abs_residual) == JACOBI_BEFORE
    B = T.lockstep_rhs(A.shape[0], 8)[0]
    before = ctx.lockstep_groups()
    res = d.solve_spd(B, rtol=1e-9, precond="amg")
    print(f"PCGBEFORE lockstep8 {res.iterations} {float(res.rel_residual).hex()} {float(res.abs_residual).hex()}")
    assert ctx.lockstep_groups() == before + 1 and res.status == _hip.OK and res.restarts == 0
    assert (res.iterations, res.rel_residual, res.abs_residual) == LOCKSTEP8_BEFORE

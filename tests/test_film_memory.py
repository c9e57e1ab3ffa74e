"""The film-curve entries under the pool's guarded, poisoned mode (needs an MI355X): tests/test_device_memory.py's
``three_ways`` -- switch unset, PADNE_POOL_GUARD=00, PADNE_POOL_GUARD=ff -- on one pass through every new entry.  The same
bits in the three runs (no read of memory nothing wrote), no guard zone changed (no write outside an array's requested
size), guarded blocks handed out in the guarded runs only."""
import numpy as np
import pytest

import film_ref as F
import thermal_ref as T
from test_device_memory import three_ways
from test_film import handle, probing_theta, solve_board, tables_for
from test_load_case_currents import finished_block

pytestmark = pytest.mark.gpu


def every_device_entry(ctx, name):
    """set_film_curves, film_terms, a Newton round by hand (linearise about zero, solve, increment, linearise about the held
    theta, resolve, increment), the report on the new hM, solve_kkt_column on a finished block, and the curves removed."""
    out = []
    with handle(ctx, name) as dev:
        tables = tables_for(dev.film, (64, 2, 1))
        dev.thermal.set_film_curves(tables)
        out.append(dev.thermal.film_terms(probing_theta(tables, dev.voff, seed=5), dev.n_vert))
        Pf = (np.random.default_rng(9).uniform(0.0, 0.06, len(dev.tri)) * T.face_area(dev.xy, dev.tri))[None, :]
        dev.thermal.film_linearise(False)
        out.append(dev.thermal.solve(Pf)[0])
        out.append(dev.thermal.film_increment())
        dev.thermal.film_linearise(True)
        out.append(dev.thermal.matrix().to_scipy())
        out.append(dev.thermal.resolve()[0])
        out.append(dev.thermal.film_increment())
        out.append(dev.thermal.report(1, len(dev.tri), dev.n_vert, fields=False, envelope=False))
        if name != "strips":
            plan, _V = finished_block(dev.board, dev.L, dev.cases)
            try:
                dev.thermal.film_linearise(False)
                out.append(dev.thermal.solve_kkt_column(plan, 1, 0)[0])
                out.append(dev.thermal.film_increment())
            finally:
                plan.close()
        dev.thermal.set_film_curves([])
        out.append(dev.thermal.matrix().to_scipy())
    return out


@pytest.mark.parametrize("name", ["strips", "two_in_layer", "two_layer_stacked"])
def test_the_film_entries_under_the_guarded_allocator(ctx, switches, name):
    three_ways(ctx, switches, lambda: every_device_entry(ctx, name))


def test_the_newton_loop_of_load_cases_under_the_guarded_allocator(ctx, switches):
    """solve_meshed_thermal with curves, an interlayer pair and two cases, one of them dead: everything it returns."""
    spec = F.host_spec("two_layer")
    dead = {e: 0.0 for e in spec.case}
    three_ways(ctx, switches, lambda: solve_board("two_layer", cases=[spec.case, dead], film_tolerance=1e-6)[1])

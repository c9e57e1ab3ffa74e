"""Host half of the bit-for-bit tests of thermal_sens.hip (no GPU): the restatement of its kernels (tests/tsens_kernel_ref.py)
against the validated specification (tests/thermal_sens_ref.py, checked by differentiation in
tests/test_thermal_sensitivity_host.py) on that file's three boards, every objective, element heat on and off -- so that the
device tests compare against something that is itself checked -- and the orders the restatement states, shown to matter.

The bar is 1e-13 of the magnitude bound: both sides evaluate the same sums of a few products in double precision in
different orders, which leaves a few units of 2^-53 = 1.1e-16 of the sum of the absolute terms; 1e-13 is about 500 times the
worst figure measured and five orders below the device tests' 1e-8.  Where the specification gives a bound per item (per
face, per mesh, per pair, per source) the bar is taken per item, which asks more than the bound of the class would; c and g
have no bound per row and are held to the largest magnitude.  Worst measured ratios of the difference to the bound, over
the three boards, both settings of element heat and all objectives: g 0 and source 0 (the specification states those two
in the kernel's own order), c 2.1e-16, e_f 5.7e-17, k_f 1.1e-16, the densities 1.9e-16, film 1.8e-16, pair 1.3e-16; the
face areas, which the specification takes from sensitivity_ref, 2.7e-16."""
import numpy as np
import pytest
import scipy.sparse as sp

import stack_ref as K
import thermal_ref as T
import tsens_kernel_ref as TK
from test_thermal_sensitivity_host import BOARDS, reference

BAR = 1e-13
WORST: dict = {}


def close(got, want, bound, what):
    """|got - want| <= BAR * bound, elementwise where ``bound`` is an array; the worst ratio is kept for the printout."""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / bound)
    worst = float(np.max(ratio, initial=0.0))
    WORST[what] = max(WORST.get(what, 0.0), worst)
    assert worst <= BAR, f"{what}: off by {worst:.3g} of the bound"


def inputs_of(ref, obj):
    """What tsens_thermal_adjoints is given for a checked objective: (kind, unknown (3,), weight (3,), source)."""
    if obj.kind == "at":
        unknown, weight = TK.owner(K.board_of(ref.flat, ref.layer_of), obj.layer, obj.point)
        return 0, unknown, weight, None
    if obj.kind == "hotspot":
        return 1, np.array([ref.hotspot_vertex(obj.layer, obj.case), -1, -1]), np.array([1.0, 0.0, 0.0]), None
    return 2, None, None, obj.source


def resistors_of(ref):
    return [(a, b, res) for _, a, b, res in ref.resistors] if ref.checked.element_heat else []


def compare(name, element_heat):
    ref, objs = reference(name, element_heat)
    N = ref.M.shape[0]
    G = sp.csr_matrix(ref.G) if ref.G is not None else None
    for obj in objs:
        want = ref.everything(obj)
        lam, mu, x, theta = want["lam"], want["mu"], ref.x[obj.case], ref.theta[obj.case]
        kind, unknown, weight, source = inputs_of(ref, obj)
        g = TK.g_vector(ref.n_pot, kind, unknown, weight, ref.sources, source)
        close(g, want["g"], np.abs(want["g"]).max(), "g")
        c = TK.rhs(N, ref.n_pot, ref.xy, ref.tri, ref.face_mesh, ref.sigma, lam, x, resistors_of(ref))
        close(c, want["c"], np.abs(want["c"]).max(), "c")
        e_d, k_d, c_d, ef, kf = TK.faces(ref.xy, ref.tri, ref.face_mesh, ref.sigma, ref.kappa, lam, theta, x, mu)
        area = want["area"]
        close(T.face_area(ref.xy, ref.tri), area, area, "area")
        close(ef, want["e"], want["e_bound"], "e_f")
        close(kf, want["k"], want["k_bound"], "k_f")
        close(e_d, want["e"] / area, want["e_bound"] / area, "densities")
        close(k_d, want["k"] / area, want["k_bound"] / area, "densities")
        close(c_d, (want["e"] + want["k"]) / area, (want["e_bound"] + want["k_bound"]) / area, "densities")
        film = TK.mesh_sums(ref.voff, TK.film_terms(ref.hM, lam, theta))
        close(film, want["film"], want["film_bound"], "film")
        if G is not None:
            pair, _per = TK.pair_values(ref.voff, ref.layer_of, G, ref.pairs_g, lam, theta)
            close(pair, want["pair"], want["pair_bound"], "pair")
        if ref.sources is not None:
            close(TK.sources(ref.sources, lam), want["source"], want["source_bound"], "source")


@pytest.mark.parametrize("element_heat", [True, False])
@pytest.mark.parametrize("name", BOARDS)
def test_the_restatement_against_the_specification(name, element_heat):
    compare(name, element_heat)
    print(name, "element_heat", element_heat, "worst so far, of the bound:", {k: f"{v:.2g}" for k, v in WORST.items()})


def test_every_class_was_compared():
    for name in BOARDS:
        for element_heat in (True, False):
            compare(name, element_heat)
    print("worst of all boards, of the bound:", {k: f"{v:.2g}" for k, v in WORST.items()})
    assert set(WORST) == {"g", "c", "area", "e_f", "k_f", "densities", "film", "pair", "source"}
    assert 0.0 < max(WORST.values()) <= BAR
    kinds = {obj.kind for name in BOARDS for obj in reference(name)[1]}
    assert kinds == {"at", "hotspot", "source"}


def test_the_owner_is_the_specifications():
    """The unknowns come in tri order and the weights add up to 1 to rounding; a point on no face gives -1 and zeros."""
    ref, objs = reference("stack")
    board = K.board_of(ref.flat, ref.layer_of)
    obj = [o for o in objs if o.kind == "at"][0]
    unknown, weight = TK.owner(board, obj.layer, obj.point)
    f = int(K.R.owners(board, obj.layer, np.array([obj.point]))[0])
    assert f >= 0 and np.array_equal(unknown, ref.tri[f]) and abs(weight.sum() - 1.0) <= 4 * 2.0 ** -53 and (weight > 0).all()
    unknown, weight = TK.owner(board, obj.layer, (99.0, 99.0))
    assert np.array_equal(unknown, [-1, -1, -1]) and not weight.any()


def test_the_source_objective_is_the_unit_load_of_sources_ref():
    """tsens_kernel_ref.source_g against sources_ref.Restated.load with unit power on the source, bit for bit, for both
    sources of ``stack`` (a list of many faces and the fallback list of one)."""
    ref, _objs = reference("stack")
    n = len(ref.sources.A)
    assert n == 2
    for s in range(n):
        unit = np.zeros((1, n))
        unit[0, s] = 1.0
        want = ref.sources.load(ref.n_pot, unit)[0]
        assert np.array_equal(TK.source_g(ref.sources, s, ref.n_pot), want) and want.sum() > 0.99


def test_the_orders_matter():
    """The orders the header comment of thermal_sens.hip promises are visible in the bits, so a test that asserts them can
    fail.  Resistors: two entries that meet on an unknown whose sum starts from 0.0 commute -- (0 + a) + b == (0 + b) + a in
    IEEE arithmetic -- so reversing the list of ``vias``, whose only shared unknown is its internal node with two resistors,
    cannot move a bit (asserted).  Order shows from three entries on, or from two on a vertex whose sum already holds its
    faces' terms: one further resistor from the internal node to a vertex that carries a via makes both, and reversing that
    list changes bits on the internal node or on that vertex.  Faces: a vertex's faces taken back to front change bits too."""
    ref, objs = reference("vias")
    N = ref.M.shape[0]
    obj = objs[0]
    want = ref.everything(obj)
    lam, x = want["lam"], ref.x[obj.case]
    own = resistors_of(ref)
    mid = ref.n_vert
    assert ref.n_internal == 1 and sum(1 for a, b, _ in own if mid in (a, b)) == 2
    col = lambda res: TK.rhs(N, ref.n_pot, ref.xy, ref.tri, ref.face_mesh, ref.sigma, lam, x, res)      # noqa: E731
    assert np.array_equal(col(own), col(own[::-1]))
    via = [r for r in own if mid not in r[:2]][0]
    more = own + [(mid, via[0], 0.016)]
    moved = np.flatnonzero(col(more) != col(more[::-1]))
    print("rows whose bits the resistor order moves:", moved.tolist())
    assert len(moved) and set(moved.tolist()) <= {mid, via[0]}
    # a vertex's faces back to front: the same faces numbered in reverse
    back = TK.rhs(N, ref.n_pot, ref.xy, ref.tri[::-1], ref.face_mesh[::-1], ref.sigma, lam, x, own)
    front = col(own)
    moved = int((back != front).sum())
    print("rows whose bits the face order moves:", moved, "of", ref.n_vert)
    assert moved > 0 and np.abs(back - front).max() <= 1e-13 * np.abs(front).max()

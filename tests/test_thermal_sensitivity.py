"""The temperature sensitivities on the device against the host specification (tests/thermal_sens_ref.py, validated by
differentiation in tests/test_thermal_sensitivity_host.py): every output within 1e-8 of its class's magnitude bound; the
four identities; central differences of device solves; what must be bitwise; the pool's guarded mode; the refusals.

Boards (the smallest at which each piece can go wrong):
  tiles     one layer with two meshes, 17 x 17 (289 vertices, 512 faces: a full tile of 256 and a partial one, of both) and
            one of 2 faces: the tile tables, the per-mesh folds, the vertex -> faces gather across a tile edge
  two_layer two 17 x 17 layers joined by a via lattice and two resistors through an internal node; element heat on and off
  chunks    the same board with 9 objectives -- one more than the largest chunk of the new kernels (8 columns of g; 4 in the
            gather and face kernels) -- spread over two load cases, so a chunk mixes cases and the last chunk is partial
  stack     17 x 17 over 13 x 13 with an interlayer pair and two heat sources, one of them smaller than a face
  the Problem-level goldens that have no regulator with a gain term"""
import gc
import math
import types

import numpy as np
import pytest

import helpers as H
import sensitivity_ref as S
import test_stack as TK
import test_thermal as TT
import thermal_sens_ref as TS
from padne_amd import _hip, problem as P, solver
from test_thermal import quiet
from test_thermal_sensitivity_host import IDENTITY_TOL, check_identities

pytestmark = pytest.mark.gpu

BAR = 1e-8                     # of each class's magnitude bound: tests/test_sensitivity.py's and tests/test_thermal.py's bar
OBJ = solver.TemperatureObjective
HS = solver.HeatSource
GOLDENS = [name for name in H.problem_golden_names() if not solver.woodbury_terms(S.problem_system(name).rows)]
GAINED = [name for name in H.problem_golden_names() if name not in GOLDENS]


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def case_of(prob, scale):
    """A load case that scales every current source of the Problem."""
    return {e: scale * e.current for n in prob.networks for e in n.elements if solver.element_kind(e) == "CurrentSource"}


def setup(name, element_heat=True):
    """(problem, meshes, layer_of, disconnected, ThermalModel, objectives, cases)."""
    cases = None
    if name in ("tiles", "two_layer", "chunks"):
        prob, meshes, layer_of = TT.synthetic_board({"tiles": "two_in_layer"}.get(name, "two_layer"))
        disc = [[] for _ in prob.layers]
        model = solver.ThermalModel(film=TT.FILM_STIFF, element_heat=element_heat)
        top = prob.layers[0]
        if name == "tiles":
            objectives = [OBJ.at(top, (3.3, 4.6)), OBJ.at(top, (20.6, 20.3)), OBJ.hotspot(top)]
        elif name == "two_layer":
            objectives = [OBJ.at(prob.layers[1], (5.2, 2.9)), OBJ.hotspot(top), OBJ.hotspot("B.Cu")]
        else:
            cases = [{}, case_of(prob, 0.5)]
            points = [(1.3, 1.2), (6.6, 6.9), (4.1, 3.3), (2.2, 6.1), (7.3, 1.4)]
            objectives = [OBJ.at(prob.layers[j % 2], q, case=j % 2) for j, q in enumerate(points)]
            objectives += [OBJ.hotspot(top, case=1), OBJ.hotspot(top, case=0), OBJ.hotspot("B.Cu", case=1), OBJ.at(top, (5.5, 5.5), case=1)]
    elif name == "stack":
        prob, meshes, layer_of = TK.own_board("pair")
        disc = [[] for _ in prob.layers]
        sources = [HS.rectangle(prob.layers[0], 6.0, 4.0, 11.0, 9.0, 0.03, name="regulator"),
                   HS.rectangle("L1", 4.1, 11.1, 4.2, 11.2, 0.01, name="0402")]
        model = solver.ThermalModel(film=TT.FILM_STIFF, element_heat=element_heat, heat_sources=sources,
                                    interlayer={(prob.layers[0], prob.layers[1]): TK.G})
        objectives = [OBJ.of_source("regulator"), OBJ.of_source("0402"), OBJ.at("L1", (9.3, 5.2)), OBJ.hotspot(prob.layers[0])]
    else:
        prob, meshes, layer_of, disc, *_ = TT.board(name)
        model = solver.ThermalModel(film=TT.FILM_STIFF, element_heat=element_heat)
        objectives = [OBJ.hotspot(prob.layers[l]) for l in sorted(set(layer_of))]
        m = max(range(len(meshes)), key=lambda i: len(meshes[i].triangles))
        pts = np.asarray(meshes[m].points, dtype=np.float64)[np.asarray(meshes[m].triangles)[len(meshes[m].triangles) // 2]]
        objectives.append(OBJ.at(prob.layers[layer_of[m]], tuple((0.5 * pts[0] + 0.3 * pts[1] + 0.2 * pts[2]).tolist())))
    return prob, meshes, layer_of, disc, model, objectives, cases


_RUNS: dict = {}


def solved(name, element_heat=True):
    """(the setup, what the call returned, the Reference, the checked objectives), once per board."""
    key = (name, element_heat)
    if key not in _RUNS:
        prob, meshes, layer_of, disc, model, objectives, cases = s = setup(name, element_heat)
        out = quiet(solver.solve_meshed_thermal_sensitivities, prob, meshes, layer_of, model, objectives, cases=cases,
                    disconnected_meshes_by_layer=disc)
        ref = TS.Reference(prob, meshes, layer_of, model, cases)
        checked = solver.check_temperature_objectives(prob, model, objectives, len(ref.cases))
        _RUNS[key] = (s, out, ref, checked)
    return _RUNS[key]


def in_mesh_order(ref, forms):
    """The per-layer, per-mesh TwoForms of a ThermalSensitivity as one array in global face order."""
    order = [m for layer in range(len(ref.prob.layers)) for m in range(ref.n_mesh) if ref.layer_of[m] == layer]
    parts = dict(zip(order, [tf.values for per in forms for tf in per]))
    return np.concatenate([parts[m] for m in range(ref.n_mesh)])


def near(got, want, size, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    err = np.abs(got - want).max(initial=0.0)
    print(f"{what}: {err / size if size > 0 else err:.3g} of the bound")
    assert err <= BAR * size, f"{what}: off by {err:.3e}, the bound is {size:.3e}"


def compare(ref, obj, sens, what):
    want = ref.everything(obj)
    theta_max = np.abs(ref.theta[obj.case]).max()
    assert sens.case == obj.case
    near(sens.value, want["value"], theta_max, f"{what} value")
    area = want["area"]
    near(in_mesh_order(ref, sens.electrical), want["e"] / area, (want["e_bound"] / area).max(), f"{what} electrical")
    near(in_mesh_order(ref, sens.thermal), want["k"] / area, (want["k_bound"] / area).max(), f"{what} thermal")
    near(in_mesh_order(ref, sens.copper), (want["e"] + want["k"]) / area, ((want["e_bound"] + want["k_bound"]) / area).max(),
         f"{what} copper")
    for layer in range(len(ref.prob.layers)):
        lo_hi = [(int(ref.toff[m]), int(ref.toff[m + 1])) for m in range(ref.n_mesh) if ref.layer_of[m] == layer]
        over = lambda v: math.fsum(x for lo, hi in lo_hi for x in v[lo:hi].tolist())      # noqa: E731
        meshes = [m for m in range(ref.n_mesh) if ref.layer_of[m] == layer]
        got = sens.layers[layer]
        near(got["electrical"], over(want["e"]), over(want["e_bound"]), f"{what} layer {layer} electrical")
        near(got["thermal"], over(want["k"]), over(want["k_bound"]), f"{what} layer {layer} thermal")
        near(got["copper"], over(want["e"]) + over(want["k"]), over(want["e_bound"]) + over(want["k_bound"]), f"{what} layer {layer} copper")
        near(got["film"], sum(want["film"][m] for m in meshes), sum(want["film_bound"][m] for m in meshes), f"{what} layer {layer} film")
    assert [p["layers"] for p in sens.interlayer] == [(a, b) for a, b, _ in ref.pairs_g]
    near([p["value"] for p in sens.interlayer], want["pair"], want["pair_bound"].max(initial=0.0), f"{what} pairs")
    near(sens.sources, want["source"], want["source_bound"].max(initial=0.0), f"{what} sources")
    assert list(sens.elements) == [element for element, _ in ref.pairs]
    for (element, row), got, d in zip(ref.pairs, sens.elements.values(), want["elements"]):
        fields = solver.SENSITIVITY_FIELDS[solver.element_kind(element)] + (("link",) if row[0] == "R" else ())
        assert tuple(got) == fields
        for field in fields:
            near(got[field], d[field], want["element_bound"][field], f"{what} {row[0]} {field}")


BOARDS = [("tiles", True), ("two_layer", True), ("two_layer", False), ("chunks", True), ("stack", True), ("stack", False)] + \
         [(name, True) for name in GOLDENS]


@pytest.mark.parametrize("name,element_heat", BOARDS)
def test_every_output_against_the_specification(ctx, name, element_heat):
    _setup, out, ref, checked = solved(name, element_heat)
    sens = out[-1]
    assert len(sens) == len(checked)
    for j, (obj, s) in enumerate(zip(checked, sens)):
        assert s.objective is _setup[5][j]
        compare(ref, obj, s, f"{name} objective {j}")


def test_the_boards_cross_the_seams():
    ref = solved("tiles")[2]
    assert np.diff(ref.voff).tolist() == [289, 4] and np.diff(ref.toff).tolist() == [512, 2]
    assert len(solved("chunks")[3]) == 9 and {o.case for o in solved("chunks")[3][:4]} == {0, 1}
    stack = solved("stack")[2]
    assert list(stack.sources.fallback) == [False, True] and stack.sources.counts[0] > 1 and len(stack.pairs_g) == 1
    assert solved("two_layer")[2].n_internal == 1 and GOLDENS and GAINED


@pytest.mark.parametrize("name,element_heat", [("two_layer", True), ("two_layer", False), ("stack", True), ("chunks", True)])
def test_the_identities_on_the_device(ctx, name, element_heat):
    """The scalings of every thermal conductance, every source and every electrical conductance, and the signs, on the
    device's numbers; reciprocity of the two heat sources on the stack."""
    _setup, out, ref, checked = solved(name, element_heat)
    for j, (obj, s) in enumerate(zip(checked, out[-1])):
        rows = ref.case_rows[obj.case]
        got = list(s.elements.values())
        res = [(row, d) for row, d in zip(rows, got) if row[0] == "R"]
        terms = types.SimpleNamespace(
            out=dict(k=in_mesh_order(ref, s.thermal) * ref.farea, e=in_mesh_order(ref, s.electrical) * ref.farea,
                     film=[layer["film"] for layer in s.layers], pair=[p["value"] for p in s.interlayer], source=s.sources),
            theta_obj=s.value - ref.checked.ambient,
            theta_s=float(sum(v * ref.power[obj.case, i] for i, v in enumerate(s.sources))),
            links=[g * d["link"] for (_, d), (_, _, g) in zip(res, ref.links)],
            sources_i=[row[3] * d["current"] for row, d in zip(rows, got) if row[0] == "I"],
            sources_u=[row[3] * d["voltage"] for row, d in zip(rows, got) if row[0] == "V"],
            r_terms=[row[3] * d["resistance"] for row, d in res])
        check_identities(terms, IDENTITY_TOL, f"{name} objective {j}")
    if name == "stack":
        a, b = out[-1][0], out[-1][1]
        assert abs(a.sources[1] - b.sources[0]) <= IDENTITY_TOL * (abs(a.sources[1]) + abs(b.sources[0]))


# ---- central differences of device solves ----------------------------------------------------------------------------------
def fd_board(sigma=2.0, current=2.0, film=TT.FILM_STIFF):
    """tests/test_thermal.py's single-layer board with the parameter to move, a footprint without power as the objective,
    and the sheet and link conductances given, so that nothing else moves with sigma."""
    top = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=sigma)
    c = [TT.conn(top, 1, 1), TT.conn(top, 7, 7), TT.conn(top, 2, 6), TT.conn(top, 6, 2)]
    resistor = P.Resistor(a=c[2].node_id, b=c[3].node_id, resistance=0.05)
    net = P.Network(connections=c, elements=[P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=current), resistor])
    model = solver.ThermalModel(film=film, sheet_conductance={top: 0.02}, link_conductance={resistor: 1e-3},
                                heat_sources=[HS.rectangle(top, 2.0, 2.0, 4.0, 4.0, 0.0, name="probe")])
    return P.Problem(layers=[top], networks=[net]), [TT.grid_mesh(1)], [0], model


def test_central_differences_of_device_solves(ctx):
    """A layer's sigma, a layer's film and a current source: (T(p + h) - T(p - h)) / 2h of ``solve_meshed_thermal`` with
    h = 1e-4 |p| against the adjoint derivative, within 1e-5 relative (step and tolerance of
    tests/test_sensitivity.py::test_finite_differences_of_device_solves).  Each of the three moves the objective by at least
    5 % of its rise per unit relative change on the host reference, so that no check is vacuous."""
    base = dict(sigma=2.0, current=2.0, film=TT.FILM_STIFF)
    prob, meshes, layer_of, model = fd_board(**base)
    objective = [OBJ.of_source("probe")]
    ref = TS.Reference(prob, meshes, layer_of, model)
    want = ref.everything(solver.check_temperature_objectives(prob, model, objective, 1)[0])
    theta_obj = want["value"] - ref.checked.ambient
    current_row = [d for row, d in zip(ref.rows, want["elements"]) if row[0] == "I"][0]
    elasticity = {"sigma": want["e"].sum(), "film": want["film"].sum(), "current": base["current"] * current_row["current"]}
    print("elasticities over the rise", {k: v / theta_obj for k, v in elasticity.items()})
    assert all(abs(v) >= 0.05 * theta_obj for v in elasticity.values())
    _sol, _rep, sens = quiet(solver.solve_meshed_thermal_sensitivities, prob, meshes, layer_of, model, objective)
    element = [e for e in sens[0].elements if solver.element_kind(e) == "CurrentSource"][0]
    adjoint = {"sigma": sens[0].layers[0]["electrical"] / base["sigma"], "film": sens[0].layers[0]["film"] / base["film"],
               "current": sens[0].elements[element]["current"]}

    def temperature(**moved):
        p, m, lo, mod = fd_board(**{**base, **moved})
        return quiet(solver.solve_meshed_thermal, p, m, lo, mod)[1].sources[0]["temperature"]
    for name, value in base.items():
        h = 1e-4 * abs(value)
        fd = (temperature(**{name: value + h}) - temperature(**{name: value - h})) / (2 * h)
        print(name, "central difference", fd, "adjoint", adjoint[name])
        assert abs(fd - adjoint[name]) <= 1e-5 * abs(fd), name


# ---- bits ------------------------------------------------------------------------------------------------------------------
def solution_arrays(sol):
    return [a for ls in sol.layer_solutions for a in ([zf.values for zf in ls.potentials] + [tf.values for tf in ls.power_densities])]


def same_bits(xs, ys):
    return len(xs) == len(ys) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(xs, ys))


def sensitivity_arrays(s):
    forms = [tf.values for group in (s.electrical, s.thermal, s.copper) for per in group for tf in per]
    scalars = [s.value, [sorted(d.items()) for d in s.layers], [sorted(p.items()) for p in s.interlayer], s.sources,
               [sorted(d.items()) for d in s.elements.values()]]
    return forms, scalars


@pytest.mark.parametrize("name", ["chunks", "stack"])
def test_the_first_items_are_solve_meshed_thermal_bit_for_bit_and_two_calls_agree(ctx, name):
    (prob, meshes, layer_of, disc, model, objectives, cases), out, _ref, _checked = solved(name)
    plain = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, cases=cases, disconnected_meshes_by_layer=disc)
    again = quiet(solver.solve_meshed_thermal_sensitivities, prob, meshes, layer_of, model, objectives, cases=cases,
                  disconnected_meshes_by_layer=disc)
    sols, reps = (plain[0], plain[1]) if cases is not None else ([plain[0]], [plain[1]])
    got_sols, got_reps = (out[0], out[1]) if cases is not None else ([out[0]], [out[1]])
    for a, b in zip(sols, got_sols):
        assert same_bits(solution_arrays(a), solution_arrays(b))
    for a, b in zip(reps, got_reps):
        (arrays_a, scalars_a), (arrays_b, scalars_b) = TT.everything(a), TT.everything(b)
        assert scalars_a == scalars_b and same_bits(arrays_a, arrays_b)
        assert a.interlayer == b.interlayer and a.sources == b.sources and a.source_heat == b.source_heat
    if cases is not None:
        env_a, env_b = plain[2], out[2]
        assert env_a.hotspots == env_b.hotspots
        assert same_bits([zf.values for per in env_a.temperatures for zf in per], [zf.values for per in env_b.temperatures for zf in per])
        assert same_bits([c for per in env_a.cases for c in per], [c for per in env_b.cases for c in per])
    for s, t in zip(out[-1], again[-1]):
        (forms_s, scalars_s), (forms_t, scalars_t) = sensitivity_arrays(s), sensitivity_arrays(t)
        assert scalars_s == scalars_t and same_bits(forms_s, forms_t)


def test_all_objectives_together_equal_single_objective_calls(ctx):
    """To 1e-8 of the bounds: the block solves may group the columns differently."""
    (prob, meshes, layer_of, disc, model, objectives, cases), out, ref, checked = solved("stack")
    for j in (0, 2):
        alone = quiet(solver.solve_meshed_thermal_sensitivities, prob, meshes, layer_of, model, [objectives[j]], cases=cases,
                      disconnected_meshes_by_layer=disc)[-1][0]
        want = ref.everything(checked[j])
        together = out[-1][j]
        near(in_mesh_order(ref, alone.copper), in_mesh_order(ref, together.copper),
             ((want["e_bound"] + want["k_bound"]) / want["area"]).max(), "copper")
        near(alone.sources, together.sources, want["source_bound"].max(), "sources")
        near([layer["film"] for layer in alone.layers], [layer["film"] for layer in together.layers], want["film_bound"].sum(), "film")
        near(alone.value, together.value, np.abs(ref.theta[0]).max(), "value")


def test_a_block_from_the_device_gives_the_bits_of_the_same_block_from_the_host(ctx):
    """``padne_kkt_solve_block_dev`` against ``padne_kkt_solve_block``: the same dense block of 5 columns, stage 1 and stage 2."""
    with TT.Device("two_layer", TT.FILM_STIFF) as dev:
        rows, cols, vals = solver.stamp_load_cases(dev.board.filtered_networks, dev.board.node_indexer, dev.L.shape[0], dev.cases)
        k = 5
        red, kidx, kval = solver.block_plan_inputs(dev.L, rows[:0], cols[:0], vals[:0], k)
        plan = _hip.KktPlan(dev.L.dev, dev.L.layout.n_potential, red.elim, red.tied, red.n_free)
        rng = np.random.default_rng(5)
        R = np.zeros((dev.L.shape[0], k))
        R[:dev.n_pot] = rng.standard_normal((dev.n_pot, k))
        kw = dict(rtol=solver.RTOL, abs_residual_target=solver.ABS_RESIDUAL_TARGET)
        p_host, res_host = plan.solve_block(R, kidx, kval, red.regulator_columns, red.probe_members, **kw)
        V_host, n_host = solver._finish_block(plan, red, red.probe_members, p_host, k)
        block = ctx.to_device(R)
        try:
            p_dev, res_dev = plan.solve_block_dev(k, block, kidx, kval, red.regulator_columns, red.probe_members, **kw)
            V_dev, n_dev = solver._finish_block(plan, red, red.probe_members, p_dev, k)
        finally:
            block.free()
            plan.close()
        assert np.array_equal(p_host, p_dev) and np.array_equal(V_host, V_dev) and np.array_equal(n_host, n_dev)
        assert res_host.iterations == res_dev.iterations and np.abs(V_host).max() > 0


# ---- the pool's guarded mode -------------------------------------------------------------------------------------------------
def sensitivity_driver(ctx):
    prob, meshes, layer_of, disc, model, objectives, cases = setup("stack")
    out = solver.solve_meshed_thermal_sensitivities(prob, meshes, layer_of, model, objectives, cases=cases)
    arrays = []
    for s in out[-1]:
        forms, scalars = sensitivity_arrays(s)
        arrays += forms + [np.array([s.value] + s.sources + [p["value"] for p in s.interlayer] + [d["film"] for d in s.layers])]
    return arrays


def test_the_guarded_poisoned_pool_gives_the_same_bits_and_no_violation(ctx, switches):
    """The whole call with PADNE_POOL_GUARD unset, 00 and ff (tests/test_device_memory.py's three ways): every block handed
    out poisoned with the fill byte between guard zones that are checked at its free."""
    runs, stats = [], []
    for mode in (None, "00", "ff"):
        if mode is not None:
            switches.set("PADNE_POOL_GUARD", mode)
        try:
            gc.collect()
            ctx.pool_guard(1)
            out = quiet(sensitivity_driver, ctx)
            runs.append([np.ascontiguousarray(np.asarray(x)).tobytes() for x in out])
            del out
            gc.collect()
            stats.append(ctx.pool_guard(0))
        finally:
            switches.unset("PADNE_POOL_GUARD")
    print("guarded blocks", [s["allocations"] for s in stats])
    for mode, st in zip((None, "00", "ff"), stats):
        assert st["violations"] == 0, (mode, st, ctx._lib.padne_last_error())
    assert stats[0]["allocations"] == 0 and stats[1]["allocations"] > 0 and stats[2]["allocations"] > 0
    assert runs[1] == runs[0] and runs[2] == runs[0]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_a_gain_term_regulator_is_refused_and_the_context_still_works(ctx):
    prob, meshes, layer_of, disc, *_ = TT.board(GAINED[0])
    model = solver.ThermalModel(film=TT.FILM_STIFF)
    with pytest.raises(ValueError, match="regulator with a gain term.*VoltageRegulator"):
        solver.solve_meshed_thermal_sensitivities(prob, meshes, layer_of, model, [OBJ.hotspot(prob.layers[layer_of[0]])],
                                                  disconnected_meshes_by_layer=disc)
    sol, rep = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, model, disconnected_meshes_by_layer=disc)
    assert rep.total_heat > 0


def test_objectives_off_the_copper_are_refused_by_the_solve(ctx):
    prob, meshes, layer_of, disc, model, objectives, cases = setup("tiles")
    with pytest.raises(ValueError, match=r"objective 1 .*\(12.0, 12.0\) lies on no connected copper of layer 'F.Cu'"):
        solver.solve_meshed_thermal_sensitivities(prob, meshes, layer_of, model, [objectives[0], OBJ.at("F.Cu", (12.0, 12.0)),
                                                                                 OBJ.at("F.Cu", (-3.0, 1.0))])
    out = quiet(solver.solve_meshed_thermal_sensitivities, prob, meshes, layer_of, model, objectives[:1])
    assert out[-1][0].value > model.ambient


def test_refusals_of_the_device_entries(ctx):
    """A handle of another context, a wrong column count, objectives out of range, no finished block, no thermal solve, and
    the order of the calls."""
    other = _hip.Context(0)
    try:
        with TT.Device("two_layer", TT.FILM_STIFF, cases=({}, {})) as dev:
            kappa, n_mesh, k = dev.kappa, len(dev.kappa), 2
            rows, cols, vals = solver.stamp_load_cases(dev.board.filtered_networks, dev.board.node_indexer, dev.L.shape[0], dev.cases)
            red, kidx, kval = solver.block_plan_inputs(dev.L, rows, cols, vals, k)
            fresh = _hip.KktPlan(dev.L.dev, dev.L.layout.n_potential, red.elim, red.tied, red.n_free)
            with pytest.raises(ValueError, match="follows padne_kkt_finish_block"):          # no finished block
                _hip.ThermalSensitivities(dev.thermal, fresh, k, kappa)
            fresh.close()
            plan, _V = dev.solved_block()
            with pytest.raises(ValueError, match="follows a thermal solve"):                 # no thermal solve
                _hip.ThermalSensitivities(dev.thermal, plan, k, kappa)
            quiet(dev.thermal.solve_kkt, plan, k)
            with pytest.raises(ValueError, match="as many columns"):                         # a wrong column count
                _hip.ThermalSensitivities(dev.thermal, plan, 3, kappa)
            with pytest.raises(ValueError, match="n_mesh"):
                _hip.ThermalSensitivities(dev.thermal, plan, k, kappa[:1])
            with pytest.raises(ValueError, match="finite and positive"):
                _hip.ThermalSensitivities(dev.thermal, plan, k, [-1.0] * n_mesh)
            ts = _hip.ThermalSensitivities(dev.thermal, plan, k, kappa)
            one = lambda **kw: ts.thermal_adjoints(**{**dict(case=[0], kind=[1], arg=[0], xy=[[0.0, 0.0]], unknown=[[3, -1, -1]],  # noqa: E731
                                                             weight=[[1.0, 0.0, 0.0]], mesh_layer=dev.layer_of), **kw})
            with pytest.raises(ValueError, match="padne_tsens_electrical_rhs follows"):       # the order of the calls
                ts.electrical_rhs()
            for bad, message in [(dict(case=[2]), "case out of range"), (dict(kind=[3]), "objective kind"),
                                 (dict(unknown=[[dev.n_pot, -1, -1]]), "unknown out of range"),
                                 (dict(weight=[[math.nan, 0.0, 0.0]]), "finite"), (dict(kind=[2]), "heat source out of range"),
                                 (dict(kind=[0], xy=[[math.inf, 0.0]]), "finite"), (dict(mesh_layer=dev.layer_of[:1]), "n_mesh"),
                                 (dict(probes=[dev.n_pot]), "probe out of range"),
                                 (dict(kind=[0], xy=[[99.0, 99.0]]), "objective 0: its point lies on no face")]:
                with pytest.raises(ValueError, match=message):
                    one(**bad)
            with pytest.raises(ValueError, match="between 1 and 4096 objectives"):
                ts.thermal_adjoints([], [], [], np.zeros((0, 2)), np.zeros((0, 3)), np.zeros((0, 3)), dev.layer_of)
            quiet(one)
            with pytest.raises(ValueError, match="padne_tsens_faces follows padne_tsens_electrical_rhs"):
                ts.faces(dev.n_tri, n_mesh)
            with pytest.raises(ValueError, match="resistor terminal out of range"):
                ts.electrical_rhs([dev.n_pot], [0], [1.0])
            with pytest.raises(ValueError, match="resistance must be finite and not zero"):
                ts.electrical_rhs([1], [0], [0.0])
            assert ts.electrical_rhs() != 0
            with pytest.raises(ValueError, match="as many columns as the finished block has"):      # the adjoint block is not solved yet
                ts.faces(dev.n_tri, n_mesh)
            with pytest.raises(ValueError, match="n_mesh"):
                ts.vertices(n_mesh + 1)
            assert ts.vertices(n_mesh).shape == (1, n_mesh) and ts.pairs().shape == (1, 0) and ts.sources().shape == (1, 0)
            ts.n_obj = 2
            with pytest.raises(ValueError, match="as many objectives"):
                ts.vertices(n_mesh)
            ts.n_obj = 1
            handle, ts.ctx = ts.ctx, other                                                    # a handle of another context
            try:
                with pytest.raises(ValueError, match="belongs to another context"):
                    ts.vertices(n_mesh)
            finally:
                ts.ctx = handle
            with pytest.raises(ValueError, match="null"):
                plan.solve_block_dev(1, 0, kidx, kval[:1], red.regulator_columns, red.probe_members)
            ts.close()
            plan.close()
    finally:
        other.close()

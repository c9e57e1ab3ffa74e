"""Host half of the temperature sensitivities (no GPU): the specification of tests/thermal_sens_ref.py validated by
differentiation, so that the device tests compare against something that is itself checked; the identities the derivatives
satisfy; ``check_temperature_objectives`` and the refusals that come before the device.

The differentiation is by complex step: the whole forward chain M(p) x = r(p), b(x, p), A(p) theta = b, T = g^T theta is
written once below (``chain``) with dense ``np.linalg.solve``, plain transposes and no ``abs`` or ``conj`` on anything that
depends on a parameter (the |cot| weights come from real coordinates), and dT/dp = Im T(p + i h) / h with h = 1e-30 |p| is
free of cancellation.  The reference's formulas share nothing with that chain but the geometry."""
import math
import types

import numpy as np
import pytest

import helpers as H
import stack_ref as K
import thermal_sens_ref as TS
from padne_amd import mesh, problem as P, solver, synthetic

REL_TOL = 1e-8                 # the project's bar (tests/test_sensitivity.py), scaled by each class's magnitude bound
IDENTITY_TOL = 1e-9            # of the sum of the absolute terms (test_scaling_and_linearity_identities)
OBJ = solver.TemperatureObjective
HS = solver.HeatSource


def grid_mesh(n, seed, size=6.0):
    xy, tri = synthetic.jittered_grid(n, n, h=size / (n - 1), seed=seed, jitter=0.2)
    return mesh.Mesh(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3))


def small_board(name, n=7):
    """(problem, meshes, layer of each mesh, ThermalModel keywords, objectives) on jittered n x n grids over the 6 x 6 square.
      one    one layer; a voltage source, a current source and a resistor
      vias   two layers joined by via resistors and by two resistors through an internal node; a current and a voltage source
      stack  two layers with an ``interlayer`` pair, two via resistors, a current source, and two heat sources, one of them
             smaller than a face (the fallback list of one face)"""
    top = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=2.0)
    bottom = P.Layer(shape=H.Geoms(1), name="B.Cu", conductance=1.5)
    at = lambda layer, x, y: P.Connection(layer=layer, point=H.XY(x, y))      # noqa: E731
    if name == "one":
        c = [at(top, 1, 1), at(top, 5, 5), at(top, 1, 5), at(top, 5, 1), at(top, 2, 3), at(top, 4, 3)]
        elements = [P.VoltageSource(p=c[0].node_id, n=c[1].node_id, voltage=0.02),
                    P.CurrentSource(f=c[2].node_id, t=c[3].node_id, current=2.0),
                    P.Resistor(a=c[4].node_id, b=c[5].node_id, resistance=0.05)]
        prob = P.Problem(layers=[top], networks=[P.Network(connections=c, elements=elements)])
        objectives = [OBJ.at(top, (3.3, 2.6)), OBJ.hotspot("F.Cu")]
        return prob, [grid_mesh(n, 1)], [0], dict(film=2e-3, ambient=30.0), objectives
    if name == "vias":
        c = [at(top, 1, 1), at(bottom, 5, 5), at(top, 5, 2), at(bottom, 5, 2), at(top, 1, 5), at(top, 4, 4)]
        mid = P.NodeID()
        elements = [P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0),
                    P.Resistor(a=c[2].node_id, b=mid, resistance=0.004), P.Resistor(a=mid, b=c[3].node_id, resistance=0.008),
                    P.VoltageSource(p=c[4].node_id, n=c[5].node_id, voltage=0.01)]
        for x, y in ((2, 3), (4, 3), (3, 5)):
            a, b = at(top, x, y), at(bottom, x, y)
            c += [a, b]
            elements.append(P.Resistor(a=a.node_id, b=b.node_id, resistance=0.002))
        prob = P.Problem(layers=[top, bottom], networks=[P.Network(connections=c, elements=elements)])
        objectives = [OBJ.at(bottom, (2.2, 4.1)), OBJ.hotspot(top), OBJ.hotspot(bottom)]
        return prob, [grid_mesh(n, 1), grid_mesh(n, 2)], [0, 1], dict(film={"F.Cu": 2e-3, "B.Cu": 1e-3}, ambient=25.0), objectives
    if name == "stack":
        c = [at(top, 1, 3), at(top, 5, 3), at(top, 2, 1), at(bottom, 2, 1), at(top, 4, 5), at(bottom, 4, 5)]
        elements = [P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0),
                    P.Resistor(a=c[2].node_id, b=c[3].node_id, resistance=0.01),
                    P.Resistor(a=c[4].node_id, b=c[5].node_id, resistance=0.02)]
        prob = P.Problem(layers=[top, bottom], networks=[P.Network(connections=c, elements=elements)])
        sources = [HS.rectangle(top, 1.5, 3.5, 4.5, 5.5, 0.02, name="regulator"),
                   HS.rectangle("B.Cu", 3.9, 3.9, 3.95, 3.95, 0.01, name="0402")]
        model = dict(film=2e-3, ambient=25.0, interlayer={(top, bottom): 1.5e-3}, heat_sources=sources)
        objectives = [OBJ.of_source("regulator"), OBJ.of_source(1), OBJ.at(top, (2.9, 3.2)), OBJ.hotspot(bottom)]
        return prob, [grid_mesh(n, 1), grid_mesh(n, 2)], [0, 1], model, objectives
    raise KeyError(name)


BOARDS = ["one", "vias", "stack"]
_CACHE: dict = {}


def reference(name, element_heat=True):
    """(Reference, the board's checked objectives), built once per board and element_heat."""
    key = (name, element_heat)
    if key not in _CACHE:
        prob, meshes, layer_of, model_kw, objectives = small_board(name)
        model = solver.ThermalModel(element_heat=element_heat, **model_kw)
        ref = TS.Reference(prob, meshes, layer_of, model)
        _CACHE[key] = (ref, solver.check_temperature_objectives(prob, model, objectives, 1))
    return _CACHE[key]


# ---- the forward chain, once, for complex parameters ----------------------------------------------------------------------
def base_parameters(ref):
    """The parameters of ``chain`` at the reference's values (floats; a test perturbs a copy)."""
    rows = ref.case_rows[0]
    return types.SimpleNamespace(
        sig=ref.fsig.astype(complex), kap=ref.fkap.astype(complex), film=np.asarray(ref.film, dtype=complex),
        pair=np.ones(len(ref.pairs_g), dtype=complex),
        power=(ref.power[0].astype(complex) if ref.sources is not None else np.zeros(0, dtype=complex)),
        value=np.array([row[{"R": 3, "I": 3, "V": 3, "REG": 5}[row[0]]] for row in rows], dtype=complex),
        link=np.array([g for _, _, g in ref.links], dtype=complex))


def pair_matrices(ref):
    """G with its diagonal, dense, of every pair alone: A depends on the pairs' conductances linearly."""
    out = []
    b = K.board_of(ref.flat, ref.layer_of)
    for p in range(len(ref.pairs_g)):
        alone = [(a, c, g if q == p else 0.0) for q, (a, c, g) in enumerate(ref.pairs_g)]
        s = K.slots(ref.flat, ref.layer_of, alone)
        G, diag = K.coupling(ref.n_pot, b.tri, s[1], s[2], s[4])
        out.append(K.full(G, diag).toarray())
    return out


def unit_loads(ref):
    if ref.sources is None:
        return np.zeros((0, ref.n_pot))
    return ref.sources.load(ref.n_pot, np.eye(len(ref.checked.sources)))


def chain(ref, g, p, fixed):
    """T - ambient = g^T theta for the parameters ``p`` (complex allowed); ``fixed`` = (pair_matrices, unit_loads)."""
    N, n_pot, rows = ref.M.shape[0], ref.n_pot, ref.case_rows[0]
    M, r = np.zeros((N, N), dtype=complex), np.zeros(N, dtype=complex)
    A = np.zeros((n_pot, n_pot), dtype=complex)
    for e in range(3):
        i, k = ref.ftri[:, e], ref.ftri[:, (e + 1) % 3]
        for mat, w, sign in ((M, p.sig * ref.cot[:, e], -1.0), (A, p.kap * ref.cot[:, e], 1.0)):
            np.add.at(mat, (i, i), sign * w)
            np.add.at(mat, (k, k), sign * w)
            np.add.at(mat, (i, k), -sign * w)
            np.add.at(mat, (k, i), -sign * w)
    res_i = 0
    resistors = []
    for row, val in zip(rows, p.value):
        if row[0] == "R":
            a, b = row[1], row[2]
            for mat, cond, sign in ((M, 1 / val, -1.0), (A, p.link[res_i], 1.0)):
                mat[a, a] += sign * cond
                mat[b, b] += sign * cond
                mat[a, b] -= sign * cond
                mat[b, a] -= sign * cond
            resistors.append((a, b, val))
            res_i += 1
        elif row[0] == "I":
            r[row[1]] += val
            r[row[2]] -= val
        elif row[0] == "V":
            iv = row[4]
            M[iv, row[1]] += 1
            M[iv, row[2]] -= 1
            M[row[1], iv] += 1
            M[row[2], iv] -= 1
            r[iv] = val
        else:
            raise NotImplementedError("the chain has no regulators")
    gnd = ref.system.ground
    M[N - 1, gnd] += 1
    M[gnd, N - 1] += 1
    x = np.linalg.solve(M, r)
    Pf = np.zeros(ref.n_tri, dtype=complex)
    for e in range(3):
        i, k = ref.ftri[:, e], ref.ftri[:, (e + 1) % 3]
        Pf = Pf + p.sig * ref.cot[:, e] * (x[i] - x[k]) * (x[i] - x[k])
    b = np.zeros(n_pot, dtype=complex)
    for corner in range(3):
        np.add.at(b, ref.ftri[:, corner], Pf / 3)
    if ref.checked.element_heat:
        for a, c, val in resistors:
            half = (x[a] - x[c]) * (x[a] - x[c]) / val / 2
            b[a] += half
            b[c] += half
    pair_full, loads = fixed
    for s, power in enumerate(p.power):
        b = b + power * loads[s]
    mesh_of_vertex = np.repeat(np.arange(ref.n_mesh), np.diff(ref.voff))
    A[np.arange(ref.n_vert), np.arange(ref.n_vert)] += p.film[mesh_of_vertex] * ref.Mv
    for scale, full in zip(p.pair, pair_full):
        A = A + scale * full
    theta = np.linalg.solve(A, b)
    return g @ theta


def complex_step(ref, g, fixed, perturb):
    """dT/dt at t = 0 for ``perturb(p, 1j * h)``, which moves the parameters by the (complex) relative amount given."""
    h = 1e-30
    p = base_parameters(ref)
    perturb(p, 1j * h)
    return chain(ref, g, p, fixed).imag / h


def close(got, want, bound, what, worst):
    ratio = abs(got - want) / (REL_TOL * bound) if bound > 0 else (0.0 if got == want else math.inf)
    worst[what] = max(worst.get(what, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: {got!r} against {want!r} by differentiation, bound {bound!r}, ratio {ratio:.3g}"


def scale(array_name, index):
    def perturb(p, t):
        getattr(p, array_name)[index] *= (1 + t)
    return perturb


@pytest.mark.parametrize("element_heat", [True, False])
@pytest.mark.parametrize("name", BOARDS)
def test_every_derivative_class_against_the_complex_step(name, element_heat):
    """Each derivative of the reference against Im T(p + i h) / h of the forward chain, within REL_TOL = 1e-8 of the class's
    magnitude bound (over the class, as tests/test_sensitivity.py::close takes it).  Every derivative is taken as p dT/dp, a
    relative move of the parameter.  Worst measured ratio of the difference to that tolerance, over the three boards, both
    settings of element_heat and all their objectives: face sigma 1.9e-8, face kappa 9.8e-8, face thickness 1.9e-8, film
    5.2e-7, pair 7.0e-8, source power 4.4e-8, resistance 5.7e-7, link 2.8e-8, current 2.7e-7, voltage 1.3e-6; the chain's
    own value against the reference's 5.5e-7.  Every class sits six orders below the bar: both sides are direct solves."""
    ref, objs = reference(name, element_heat)
    fixed = (pair_matrices(ref), unit_loads(ref))
    worst: dict = {}
    rows = ref.case_rows[0]
    res_index = [i for i, row in enumerate(rows) if row[0] == "R"]
    for obj in objs:
        out = ref.everything(obj)
        g = out["g"]
        theta_obj = out["value"] - ref.checked.ambient
        close(chain(ref, g, base_parameters(ref), fixed).real, theta_obj, abs(theta_obj), "value", worst)
        order = np.argsort(-np.abs(out["e"]))
        e_size, k_size = out["e_bound"].max(), out["k_bound"].max()       # the class's bound, as test_sensitivity.py::close takes it
        for f in {int(order[0]), int(order[len(order) // 2]), int(np.argmax(np.abs(out["k"]))), 3}:
            close(out["e"][f], complex_step(ref, g, fixed, scale("sig", f)), e_size, "face sigma", worst)
            close(out["k"][f], complex_step(ref, g, fixed, scale("kap", f)), k_size, "face kappa", worst)

            def thicken(p, t, f=f):
                p.sig[f] *= (1 + t)
                p.kap[f] *= (1 + t)
            close(out["e"][f] + out["k"][f], complex_step(ref, g, fixed, thicken), e_size + k_size, "face thickness", worst)
        for layer in range(len(ref.prob.layers)):
            meshes = [m for m in range(ref.n_mesh) if ref.layer_of[m] == layer]
            close(sum(out["film"][m] for m in meshes), complex_step(ref, g, fixed, scale("film", meshes)),
                  out["film_bound"].sum(), "film", worst)
        for q in range(len(ref.pairs_g)):
            close(out["pair"][q], complex_step(ref, g, fixed, scale("pair", q)), out["pair_bound"].max(), "pair", worst)
        for s in range(len(ref.checked.sources)):
            close(out["source"][s] * ref.power[0, s], complex_step(ref, g, fixed, scale("power", s)),
                  out["source_bound"][s] * ref.power[0, s], "source power", worst)
        for i, (row, d) in enumerate(zip(rows, out["elements"])):
            value = row[{"R": 3, "I": 3, "V": 3}[row[0]]]
            field = {"R": "resistance", "I": "current", "V": "voltage"}[row[0]]
            close(d[field] * value, complex_step(ref, g, fixed, scale("value", i)), out["element_bound"][field] * abs(value),
                  field, worst)
            if row[0] == "R":
                at = res_index.index(i)
                glink = ref.links[at][2]
                close(d["link"] * glink, complex_step(ref, g, fixed, scale("link", at)), out["element_bound"]["link"] * glink,
                      "link", worst)
    print(name, "element_heat", element_heat, {k: f"{v:.2g}" for k, v in worst.items()})
    assert set(worst) >= {"value", "face sigma", "face kappa", "face thickness", "film", "resistance", "link", "current"}


def test_the_boards_cover_every_class():
    """Voltage sources, internal nodes, an interlayer pair and two heat sources (one on the fallback list) all occur."""
    assert any(row[0] == "V" for row in reference("one")[0].rows) and any(row[0] == "V" for row in reference("vias")[0].rows)
    assert reference("vias")[0].n_internal == 1
    stack = reference("stack")[0]
    assert len(stack.pairs_g) == 1 and list(stack.sources.fallback) == [False, True] and stack.sources.counts[0] > 1


# ---- identities ------------------------------------------------------------------------------------------------------------
def identity_terms(ref, obj):
    """The sums the identities relate, each as (value, sum of the absolute terms)."""
    out = ref.everything(obj)
    rows = ref.case_rows[obj.case]
    theta_obj = out["value"] - ref.checked.ambient
    theta_s = float(sum(out["source"][s] * ref.power[obj.case, s] for s in range(len(out["source"]))))
    res = [(row, d) for row, d in zip(rows, out["elements"]) if row[0] == "R"]
    links = [g * d["link"] for (_, d), (_, _, g) in zip(res, ref.links)]
    sources_i = [row[3] * d["current"] for row, d in zip(rows, out["elements"]) if row[0] == "I"]
    sources_u = [row[3] * d["voltage"] for row, d in zip(rows, out["elements"]) if row[0] == "V"]
    r_terms = [row[3] * d["resistance"] for row, d in res]
    return types.SimpleNamespace(out=out, theta_obj=theta_obj, theta_s=theta_s, links=links, sources_i=sources_i,
                                 sources_u=sources_u, r_terms=r_terms)


def check_identities(t, tol, what=""):
    """The four identities on the terms of ``identity_terms`` (or on the device's numbers laid out the same way)."""
    out = t.out
    # 1. every thermal conductance scaled by s: theta -> theta / s
    terms = list(out["k"]) + list(out["film"]) + list(out["pair"]) + t.links
    size = sum(abs(v) for v in terms) + abs(t.theta_obj)
    assert abs(math.fsum(terms) + t.theta_obj) <= tol * size, f"{what} thermal scaling"
    # 2. every electrical source scaled by s: the Joule and element heat go with s^2, the component heat does not move
    terms = t.sources_i + t.sources_u
    size = sum(abs(v) for v in terms) + 2 * (abs(t.theta_obj) + abs(t.theta_s))
    assert abs(math.fsum(terms) - 2 * (t.theta_obj - t.theta_s)) <= tol * size, f"{what} source scaling"
    # 3. every electrical conductance scaled by s: T_J(s; I, U) = s F(I / s, U) with F homogeneous of degree 2
    terms = list(out["e"]) + [-v for v in t.r_terms]
    size = sum(abs(v) for v in terms) + abs(t.theta_obj) + abs(t.theta_s) + sum(abs(v) for v in t.sources_i)
    assert abs(math.fsum(terms) - ((t.theta_obj - t.theta_s) - math.fsum(t.sources_i))) <= tol * size, f"{what} conductance scaling"
    # signs: A is an M-matrix, so lambda >= 0
    assert all(v > 0 for v in out["source"]) and all(v <= 0 for v in out["film"]), f"{what} signs"


@pytest.mark.parametrize("element_heat", [True, False])
@pytest.mark.parametrize("name", BOARDS)
def test_the_identities_hold_on_the_reference(name, element_heat):
    """Scaling every thermal conductance, every source and every electrical conductance, and the signs.  All four identities
    of the issue hold on the validated reference; none had to be dropped."""
    ref, objs = reference(name, element_heat)
    for j, obj in enumerate(objs):
        check_identities(identity_terms(ref, obj), IDENTITY_TOL, f"{name} objective {j}")


def test_reciprocity_of_two_heat_sources():
    """dT_a/dP_b = dT_b/dP_a: both are g_a^T A^-1 g_b with A symmetric."""
    ref, objs = reference("stack")
    a, b = ref.everything(objs[0]), ref.everything(objs[1])
    size = abs(a["source"][1]) + abs(b["source"][0])
    assert abs(a["source"][1] - b["source"][0]) <= IDENTITY_TOL * size


def test_hotspot_resolves_to_the_reports_vertex():
    """The rule of ``ThermalReport.hotspots``: per mesh the first maximum, a later mesh of the layer only when strictly hotter
    -- on per-mesh maxima laid out as ``Thermal.report`` returns them."""
    prob, meshes, layer_of, _kw, _objs = small_board("one")
    island = mesh.Mesh(np.asarray(meshes[0].points, dtype=np.float64) + 10.0, np.asarray(meshes[0].triangles, dtype=np.int32))
    board = solver.index_board(prob, [meshes[0], island], [0, 0])           # two meshes on the one layer
    voff = board.vindex.offsets
    mesh_max = np.array([[1.5, 1.5], [1.0, 2.0]])
    mesh_vert = np.array([[voff[0] + 4, voff[1] + 9], [voff[0] + 4, voff[1] + 9]], dtype=np.int64)
    tie = solver._layer_hotspot(board, 25.0, mesh_max, mesh_vert, 0, 0)
    later = solver._layer_hotspot(board, 25.0, mesh_max, mesh_vert, 1, 0)
    assert tie[:3] == (26.5, 0, 4) and later[:3] == (27.0, 1, 9)
    assert solver._layer_hotspot(board, 25.0, mesh_max, np.full((2, 2), -1), 0, 0) is None      # no connected vertices
    ref, objs = reference("vias")
    hot = [o for o in objs if o.kind == "hotspot"][0]
    v = ref.hotspot_vertex(hot.layer, 0)
    lo, hi = int(ref.voff[hot.layer]), int(ref.voff[hot.layer + 1])
    assert lo <= v < hi and ref.theta[0][v] == ref.theta[0][lo:hi].max()


# ---- checks that come before the device ------------------------------------------------------------------------------------
def test_check_temperature_objectives():
    prob, _meshes, _layer_of, kw, objectives = small_board("stack")
    model = solver.ThermalModel(**kw)
    got = solver.check_temperature_objectives(prob, model, objectives, 2)
    assert [(o.kind, o.layer, o.source, o.case) for o in got] == [("source", None, 0, 0), ("source", None, 1, 0), ("at", 0, None, 0),
                                                                  ("hotspot", 1, None, 0)]
    assert got[2].point == (2.9, 3.2)
    assert solver.check_temperature_objectives(prob, model, [OBJ.at("B.Cu", (1, 2), case=1)], 2)[0].layer == 1
    top = prob.layers[0]
    for bad, message in [
            ([], "no objectives"), (OBJ.hotspot(top), "sequence"), ({"a": 1}, "sequence"), ("hot", "sequence"), (5, "sequence"),
            ([(top, (1, 2))], "no TemperatureObjective"), ([OBJ.hotspot(top, case=2)], "case"), ([OBJ.hotspot(top, case=-1)], "case"),
            ([OBJ.hotspot(top, case=0.5)], "case"), ([OBJ.hotspot("In1.Cu")], "no layer"), ([OBJ.at(top, (1.0, math.nan))], "finite"),
            ([OBJ.at(top, (1.0,))], "pair"), ([OBJ.at(top, "ab")], "pair"), ([OBJ.of_source("fuse")], "no heat source"),
            ([OBJ.of_source(2)], "no heat source"), ([OBJ.of_source(None)], "no heat source"),
            ([OBJ("mean", layer=top)], "unknown kind"), ([OBJ.hotspot(top)] * 4097, "at most 4096")]:
        with pytest.raises(ValueError, match=message):
            solver.check_temperature_objectives(prob, model, bad, 2)
    with pytest.raises(ValueError, match="no heat source"):
        solver.check_temperature_objectives(prob, solver.ThermalModel(film=1e-3), [OBJ.of_source(0)], 1)


def test_the_limits_are_refused_before_the_device(monkeypatch):
    """A partition over several GPUs, a regulator with a gain term on distinct sense nodes (named in the message), more than
    4096 objectives, an electro-thermal and a transient model, and an unknown source name: each a ValueError while the device
    has not been asked for anything."""
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(solver.IndexedBoard, "assembled", no_device)
    prob, meshes, layer_of, kw, objectives = small_board("one")
    model = solver.ThermalModel(**kw)
    call = lambda p=prob, m=model, o=objectives, **k: solver.solve_meshed_thermal_sensitivities(p, meshes, layer_of, m, o, **k)  # noqa: E731
    with pytest.raises(ValueError, match="one GPU"):
        call(partition=types.SimpleNamespace(world=2))
    with pytest.raises(ValueError, match="one GPU"):
        solver.solve_thermal_sensitivities(prob, model, objectives, partition=types.SimpleNamespace(world=2))
    with pytest.raises(ValueError, match="at most 4096"):
        call(o=[OBJ.hotspot(prob.layers[0])] * 4097)
    with pytest.raises(ValueError, match="electro-thermal and the transient models are not accepted"):
        call(m=solver.ElectroThermalModel(thermal=model))
    with pytest.raises(ValueError, match="electro-thermal and the transient models are not accepted"):
        call(m=solver.TransientModel(thermal=model, areal_capacity=1e-3))
    with pytest.raises(ValueError, match="no heat source"):
        call(o=[OBJ.of_source("regulator")])
    # the same board with a regulator whose gain term acts on two distinct sense nodes
    net = prob.networks[0]
    c = list(net.connections)
    reg = P.VoltageRegulator(v_p=c[0].node_id, v_n=c[1].node_id, s_f=c[4].node_id, s_t=c[5].node_id, voltage=0.02, gain=0.5)
    gained = P.Problem(layers=prob.layers, networks=[P.Network(connections=c, elements=[reg] + list(net.elements[1:]))])
    with pytest.raises(ValueError, match="regulator with a gain term.*VoltageRegulator"):
        call(p=gained, o=[OBJ.hotspot(gained.layers[0])])
    # ... and one whose gain is zero is no such term: it gets as far as the device
    plain = P.VoltageRegulator(v_p=c[0].node_id, v_n=c[1].node_id, s_f=c[4].node_id, s_t=c[5].node_id, voltage=0.02, gain=0.0)
    ungained = P.Problem(layers=prob.layers, networks=[P.Network(connections=c, elements=[plain] + list(net.elements[1:]))])
    with pytest.raises(AssertionError, match="the device was touched"):
        call(p=ungained, o=[OBJ.hotspot(ungained.layers[0])])

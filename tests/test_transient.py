"""The transient thermal model on the device against the host restatement (tests/transient_ref.py, itself checked by
tests/test_transient_host.py): the capacities, the step matrix, the load table and the right-hand side bit for bit; every
step's temperatures against direct stepping; the discrete balance of every step; the limits of long and of steady runs;
scenarios in lockstep against the same scenarios alone; the per-step report, the envelope along time and the probes; the
reuse of the hierarchy; bitwise repeatability; the refusals of the device entries; the public call.

Boards: those of tests/test_thermal.py, and one jittered 49 x 49 grid (2 401 vertices): up to 2 048 unknowns the "hierarchy"
is the dense inverse alone, so this is the smallest board on which a real hierarchy is built, reused across steps and rebuilt
on a change of dt."""
import ctypes
import warnings

import numpy as np
import pytest

import helpers as H
import thermal_ref as T
import transient_ref as R
import test_thermal as TT
from padne_amd import _hip, mesh, problem as P, solver, synthetic
from test_thermal import BAR, Device, delivered_power, quiet, random_loads, restated_loads, sorted_csr

pytestmark = pytest.mark.gpu

GRID49 = "grid49"
BOARDS = TT.BOARDS + [GRID49]
FILM, CAP = 1e-3, 3e-3
TAU = CAP / FILM
DT1, DT2 = TAU / 20, 0.05
SCHEDULE = [(DT1, 12, 0), (DT2, 12, 0), (DT2, 16, None)]      # on, on with another dt, off: 40 steps, two distinct dt


@pytest.fixture(scope="module")
def ctx():
    yield solver.get_context()


def grid49_board():
    """The board ``single`` of tests/test_thermal.py on a 49 x 49 grid over the same 8 x 8 square, in 35 um copper: 2086 S,
    so 0.0149 W/K by Wiedemann-Franz.  With the 2 S of the other synthetic boards the sheet conducts so little heat that S
    is all but diagonal, the aggregation finds nothing to merge, and the "hierarchy" would again be the dense inverse."""
    top = P.Layer(shape=H.Geoms(1), name="F.Cu", conductance=2086.0)
    c = [TT.conn(top, 1, 1), TT.conn(top, 7, 7), TT.conn(top, 2, 6), TT.conn(top, 6, 2)]
    net = P.Network(connections=c, elements=[P.CurrentSource(f=c[0].node_id, t=c[1].node_id, current=2.0),
                                             P.Resistor(a=c[2].node_id, b=c[3].node_id, resistance=0.05)])
    xy, tri = synthetic.jittered_grid(49, 49, h=8.0 / 48, seed=7, jitter=0.2)
    msh = mesh.Mesh(np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(tri, dtype=np.int32).reshape(-1, 3))
    return P.Problem(layers=[top], networks=[net]), [msh], [0]


def board(name):
    """tests/test_thermal.py's ``board``, with the 49 x 49 grid added to its table."""
    if name == GRID49 and name not in TT._BOARDS:
        prob, meshes, layer_of = grid49_board()
        vindex = solver.VertexIndexer.create(meshes)
        nodes = solver.NodeIndexer.create(prob, meshes, layer_of, vindex, list(prob.networks))
        flat = [(np.asarray(m.points, dtype=np.float64), np.asarray(m.triangles, dtype=np.int64)) for m in meshes]
        TT._BOARDS[name] = (prob, meshes, layer_of, [[] for _ in prob.layers], flat, nodes.internal_node_count,
                            solver.global_elements(list(prob.networks), nodes))
    return TT.board(name)


class Stepping(Device):
    """A board on the device with its thermal and its transient handle, kept open for one test.  The capacity differs from
    layer to layer (CAP, 2 CAP, ...) so that a mesh reading another mesh's capacity shows."""

    def __init__(self, name, film=FILM, cases=({},), **model_kw):
        board(name)
        super().__init__(name, film, cases, **model_kw)
        self.capacity = [CAP * (1 + layer) for layer in self.layer_of]

    def __enter__(self):
        super().__enter__()
        self.tr = _hip.Transient(self.thermal, self.capacity)
        return self

    def __exit__(self, *exc):
        self.tr.close()
        return super().__exit__(*exc)

    def host(self):
        """(A, hM, Cv) restated."""
        A, M, hM = self.restated()
        return A, hM, R.capacity(self.voff, self.capacity, M)

    def loaded(self, k, seed):
        """k random load cases on the handle (the last one empty when k > 2); their restated load vectors."""
        Pf, heat = random_loads(self, k, seed)
        self.tr.loads(Pf, heat)
        return restated_loads(self, Pf, heat)

    def all_unknowns(self):
        return np.arange(self.n_pot, dtype=np.int64)


def reference_states(dev, B, schedule, initial=None):
    """The states (n_steps + 1, n_pot) of one column by direct stepping; ``initial``: a case whose steady state it starts from."""
    A, hM, Cv = dev.host()
    theta0 = None if initial is None else T.solve(A, B[initial])
    return R.run(A, Cv, hM, dev.voff, B, schedule, theta0)


def device_states(dev, schedule, initial):
    """Every column through ``schedule`` = [(dt, steps, per-column cases)]: the states (n_steps + 1, n_cols, n_pot), read as
    probes of every unknown, and the list of the runs' results."""
    dev.tr.start(initial)
    states, runs = [dev.tr.state()], []
    for dt, steps, cases in schedule:
        runs.append(dev.tr.run(dt, steps, cases, dev.all_unknowns()))
        states.extend(runs[-1]["probes"])
    assert np.array_equal(states[-1], dev.tr.state())          # the probe of every unknown is the state
    return np.stack(states), runs


# ---- 1. Cv, S, B and the right-hand side ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOARDS)
def test_capacities_step_matrix_loads_and_right_hand_side_are_the_restatement_bit_for_bit(ctx, name):
    """Cv, S(dt), B and rhs have the restatement's bits.  S against A as test_thermal compares A against K: the structure,
    the off-diagonals A's, the diagonal the one rounded sum.  rhs for 11 columns -- a full launch group of 8 and a ragged 3
    -- that mix the cases and "off", on a non-zero state reached by two steps."""
    dt = 0.37
    with Stepping(name) as dev:
        Pf, heat = random_loads(dev, 3, seed=3)
        dev.tr.loads(Pf, heat)
        B, b_thermal = dev.tr.load_vectors(), dev.thermal.load(Pf, heat)
        Cv = dev.tr.capacity(dev.n_vert)
        A_dev = sorted_csr(dev.thermal.matrix().to_scipy())
        S = sorted_csr(dev.tr.matrix(dt).to_scipy())
        S2 = sorted_csr(dev.tr.matrix(2 * dt).to_scipy())
        initial = [None, 0, 1, None, 2, 0, 1, None, 0, 1, 2]
        first = [0, 1, None, 2, None, 1, 0, 0, None, None, 1]
        then = [1, None, 0, 0, 2, None, 1, None, 1, 0, None]
        dev.tr.start(initial)
        dev.tr.run(dt, 2, first)
        theta = dev.tr.state()
        rhs = dev.tr.rhs(dt, then)
        assert np.array_equal(dev.tr.state(), theta)           # rhs does not advance the state
    A, hM, Cv_want = dev.host()
    assert np.array_equal(Cv, Cv_want)
    assert np.array_equal(B, b_thermal) and np.array_equal(B, restated_loads(dev, Pf, heat))
    for got, step in ((S, dt), (S2, 2 * dt)):
        want = R.step_matrix(A, Cv_want, step)
        assert H.same_structure(got, A_dev) and H.same_structure(got, want)
        assert np.array_equal(got.data, sorted_csr(want).data)
        off_S, d_S = H.offdiag_and_diag(got)
        off_A, d_A = H.offdiag_and_diag(A_dev)
        assert np.array_equal(sorted_csr(off_S).data, sorted_csr(off_A).data)
        assert np.array_equal(d_S[:dev.n_vert], d_A[:dev.n_vert] + Cv_want / step)
        assert np.array_equal(d_S[dev.n_vert:], d_A[dev.n_vert:])
    assert np.abs(theta).max() > 0.0
    for c, j in enumerate(then):
        assert np.array_equal(rhs[c], R.rhs(Cv_want, dt, theta[c], None if j is None else B[j])), c


# ---- 2. every step against direct stepping --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", BOARDS)
def test_trajectory_against_the_host_reference(ctx, name):
    """film 1e-3, c = 3e-3 (twice that on a second layer): on for 12 steps of tau / 20, on for 12 steps of 0.05 (a change of
    dt), off for 16.  Every step's theta within 1e-8 of max |theta| over the run.  A step's error is at most cond(S) rtol
    ||theta||, old errors decay by (c / dt) / (h + c / dt) per step, so the sum stays below cond(A) rtol, about 5e-10 at this
    film: the steady test's own margin."""
    with Stepping(name) as dev:
        B = dev.loaded(1, seed=5)
        states, runs = device_states(dev, [(dt, steps, [case]) for dt, steps, case in SCHEDULE], [None])
    want = reference_states(dev, B, SCHEDULE)[0]
    scale = np.abs(want).max()
    err = np.abs(states[:, 0] - want).max(axis=1)
    print(name, "worst error / max|theta|", err.max() / scale, "at step", int(err.argmax()), "iterations per step",
          np.concatenate([r["iterations"] for r in runs]).tolist())
    assert all(r["result"].status == _hip.OK for r in runs)
    assert scale > 0.0 and (err <= BAR * scale).all()
    assert (states[0] == 0.0).all() and not np.signbit(states[0]).any()        # an ambient start: exact zeros


# ---- 3. the balance of every step, through the public call ----------------------------------------------------------------

def public_schedule():
    return [solver.Segment(12 * DT1, 12, 0), solver.Segment(12 * DT2, 12, 0), solver.Segment(16 * DT2, 16, None)]


def model_of(film=FILM, capacity=CAP, initial=None, **kw):
    return solver.TransientModel(thermal=solver.ThermalModel(film=film, **kw), areal_capacity=capacity, initial=initial)


@pytest.mark.parametrize("name", BOARDS)
def test_every_step_balances_stored_heat_film_loss_and_delivered_power(ctx, name):
    """(stored_{n+1} - stored_n) / dt + loss_{n+1} = the heat of the step's case within 1e-9 relative of the run's largest
    heat (the steady balance test's bar), 0 in the off steps; and that heat is what the sources deliver."""
    prob, meshes, layer_of, disc, *_ = board(name)
    _sol, currents = quiet(solver.solve_meshed_currents, prob, meshes, layer_of, disconnected_meshes_by_layer=disc)
    delivered = delivered_power(currents)
    sols, rep = quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, model_of(), public_schedule(),
                      disconnected_meshes_by_layer=disc)
    assert len(sols) == 1 and len(rep.times) == 41
    dts = np.diff(rep.times)
    defect = (rep.total_stored[1:] - rep.total_stored[:-1]) / dts + rep.total_loss[1:] - rep.total_heat[1:]
    top = rep.total_heat.max()
    print(name, "delivered", delivered, "heat", top, "worst balance defect / heat", np.abs(defect).max() / top)
    assert delivered > 0 and abs(top - delivered) <= 1e-9 * delivered
    assert (rep.total_heat[1:25] == top).all() and (rep.total_heat[25:] == 0.0).all() and rep.total_heat[0] == 0.0
    assert (np.abs(defect) <= 1e-9 * top).all()
    for layer in rep.layers:                                # the layers' parts add up
        assert len(layer["stored"]) == len(layer["loss"]) == len(layer["heat"]) == 41
    assert np.allclose(sum(layer["stored"] for layer in rep.layers), rep.total_stored, rtol=1e-13, atol=0.0)
    # (a hierarchy per run of equal dt: 12 * 0.05 / 12 and 16 * 0.05 / 16 may differ in their last bit)
    assert 2 <= rep.info["hierarchies"] <= 3 and rep.info["iterations"] == int(rep.info["iterations_per_step"].sum())


# ---- 4. limits ------------------------------------------------------------------------------------------------------------

def vertex_temperatures(fields):
    return np.concatenate([zf.values for forms in fields for zf in forms])


@pytest.mark.parametrize("name", ["single", "two_layer"])
def test_long_runs_reach_and_keep_the_steady_state_and_an_idle_board_stays_at_ambient(ctx, name):
    """40 steps of 5 tau under a constant load end within 1e-6 relative of solve_meshed_thermal's temperatures (the remainder
    (1 + 5)^-40 is far below); started from that steady state the same schedule stays there within 1e-8 of max |theta| at
    every step; a scenario that is off throughout from ambient is exactly ambient."""
    prob, meshes, layer_of, disc, *_ = board(name)
    ambient = 40.0
    _s, steady = quiet(solver.solve_meshed_thermal, prob, meshes, layer_of, solver.ThermalModel(film=FILM, ambient=ambient),
                       disconnected_meshes_by_layer=disc)
    want = vertex_temperatures(steady.temperatures)
    scale = np.abs(want - ambient).max()
    schedule = [solver.Segment(5 * TAU, 1, (0, 0, None)) for _ in range(40)]
    _sols, reps = quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of,
                        model_of(initial=(None, 0, None), ambient=ambient), schedule, keep="segments",
                        disconnected_meshes_by_layer=disc)
    ramp, held, idle = reps
    assert len(ramp.temperatures) == len(held.temperatures) == 40
    end = vertex_temperatures(ramp.temperatures[-1])
    print(name, "end of the ramp against the steady state, relative", np.abs(end - want).max() / scale)
    assert np.abs(end - want).max() <= 1e-6 * scale
    drift = max(np.abs(vertex_temperatures(fields) - want).max() for fields in held.temperatures)
    print(name, "largest drift from the steady state / max|theta|", drift / scale)
    assert drift <= BAR * scale
    assert all((vertex_temperatures(fields) == ambient).all() for fields in idle.temperatures)
    assert (idle.total_stored == 0.0).all() and (idle.total_loss == 0.0).all() and idle.peak[0] == ambient


# ---- 5. scenarios in lockstep ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [GRID49, "two_layer"])
def test_scenarios_in_one_block_are_the_scenarios_alone(ctx, name):
    """5 scenarios (a padded lockstep group of 8 where the operator takes the batched path), one of them off throughout:
    every column within 1e-8 of max |theta| of the same scenario run alone; then the first 3, which go one at a time.  The
    column that is off since its ambient start is exact zeros with no sign bit."""
    initial = [None, 0, None, 1, None]
    schedule = [(DT1, 5, [0, 1, None, 0, 1]), (DT2, 5, [None, 1, None, 1, 0])]
    with Stepping(name) as dev:
        dev.loaded(2, seed=8)
        alone = []
        for c in range(5):
            alone.append(device_states(dev, [(dt, n, [cases[c]]) for dt, n, cases in schedule], [initial[c]])[0][:, 0])
        for k in (5, 3):
            before = ctx.lockstep_groups()
            states, _runs = device_states(dev, [(dt, n, cases[:k]) for dt, n, cases in schedule], initial[:k])
            print(name, k, "scenarios: lockstep groups solved", ctx.lockstep_groups() - before)
            for c in range(k):
                scale = np.abs(alone[c]).max()
                err = np.abs(states[:, c] - alone[c]).max()
                print(name, k, "scenarios, column", c, "error / max|theta|", err / max(scale, 1e-300))
                assert err <= BAR * scale
            assert (states[:, 2] == 0.0).all() and not np.signbit(states[:, 2]).any()
    assert all(np.abs(alone[c]).max() > 0.0 for c in (0, 1, 3, 4))


# ---- 6. the report, the envelope and the probes ----------------------------------------------------------------------------

def check_report(dev, Cv, hM, theta, out, k):
    """Row k of a run's per-mesh arrays against the restatement on the device's own theta (n_cols, n_pot)."""
    for c in range(theta.shape[0]):
        top, vert, stored, loss = R.mesh_report(dev.voff, Cv, hM, theta[c])
        assert np.array_equal(out["max"][k, c], top) and np.array_equal(out["vertex"][k, c], vert)
        assert (np.abs(out["stored"][k, c] - stored) <= 1e-12 * np.abs(stored)).all()
        assert (np.abs(out["loss"][k, c] - loss) <= 1e-12 * np.abs(loss)).all()


@pytest.mark.parametrize("name", ["single", "two_in_layer", "problem_many_meshes"])
def test_the_report_envelope_and_probes_against_the_restatement(ctx, name):
    """On the device's own theta, step by step: per-mesh maximum and vertex exact, stored heat and film loss within 1e-12
    relative of math.fsum, the envelope and its steps exact, the probe traces the state's bits.  Column 0 heats and cools
    (its envelope peaks in the middle), column 1 starts from a steady state and keeps its load (ties between steps wherever
    the state keeps its bits), column 2 is off from ambient: the complete tie, step 0 and each mesh's first vertex."""
    with Stepping(name) as dev:
        dev.loaded(2, seed=11)
        _A, hM, Cv = dev.host()
        probes = np.array([0, dev.n_vert - 1, dev.n_pot - 1, dev.n_vert // 2], dtype=np.int64)
        dev.tr.start([None, 1, None])
        states = [dev.tr.state()]
        top0, vert0, stored0, loss0 = dev.tr.report()
        check_report(dev, Cv, hM, states[0], {"max": top0[None], "vertex": vert0[None], "stored": stored0[None], "loss": loss0[None]}, 0)
        for dt, cases in [(DT1, [0, 1, None])] * 4 + [(DT2, [None, 1, None])] * 4:
            out = dev.tr.run(dt, 1, cases, probes)
            states.append(dev.tr.state())
            check_report(dev, Cv, hM, states[-1], out, 0)
            assert np.array_equal(out["probes"][0], states[-1][:, probes])
        out = dev.tr.run(DT2, 3, [0, 1, None], dev.all_unknowns())      # several steps in one call: the rows are the steps'
        for k in range(3):
            states.append(out["probes"][k])
            check_report(dev, Cv, hM, states[-1], out, k)
        assert np.array_equal(states[-1], dev.tr.state())
        env, env_step = dev.tr.envelope(dev.n_vert)
        assert dev.tr.clock()[0] == 11
    states = np.stack(states)
    for c in range(3):
        best, step = R.envelope(states[:, c, :dev.n_vert])
        assert np.array_equal(env[c], best) and np.array_equal(env_step[c], step), c
    print(name, "vertices of the steady column whose envelope is still the start's:", int((env_step[1] == 0).sum()), "of", dev.n_vert)
    assert (env_step[2] == 0).all() and (env[2] == 0.0).all()
    assert 0 < env_step[0].max() <= 11


def test_the_envelope_of_every_column_after_every_step(ctx):
    """The envelope downloaded after every single step is the restated one of the states so far, exactly: heating, cooling
    and heating again on ``single``."""
    with Stepping("single") as dev:
        dev.loaded(2, seed=12)
        dev.tr.start([None, 0])
        states = [dev.tr.state()]
        for dt, cases in [(DT1, [0, None])] * 3 + [(DT2, [None, 1])] * 3 + [(DT1, [1, 0])] * 3:
            dev.tr.run(dt, 1, cases)
            states.append(dev.tr.state())
            env, env_step = dev.tr.envelope(dev.n_vert)
            for c in range(2):
                best, step = R.envelope(np.stack(states)[:, c, :dev.n_vert])
                assert np.array_equal(env[c], best) and np.array_equal(env_step[c], step)


def test_a_held_steady_state_keeps_the_first_step_of_every_tie(ctx):
    """A start from the steady state under its own constant load: wherever a later step reproduces a vertex's bits the
    envelope keeps the earlier step -- the restated rule on the device's own states, exactly; the ties are counted."""
    with Stepping("single") as dev:
        dev.loaded(1, seed=13)
        dev.tr.start([0])
        states = [dev.tr.state()]
        for _ in range(6):
            dev.tr.run(DT1, 1, [0])
            states.append(dev.tr.state())
        env, env_step = dev.tr.envelope(dev.n_vert)
    states = np.stack(states)[:, 0, :dev.n_vert]
    best, step = R.envelope(states)
    tied = int(((states == best[None]).sum(axis=0) > 1).sum())
    print("vertices whose maximum is attained by more than one step:", tied, "of", dev.n_vert)
    assert np.array_equal(env[0], best) and np.array_equal(env_step[0], step)


def test_a_probe_may_name_an_internal_node(ctx):
    with Stepping("two_layer") as dev:
        assert dev.n_internal == 1
        dev.loaded(1, seed=14)
        dev.tr.start([None])
        out = dev.tr.run(DT1, 3, [0], [dev.n_vert, 5])
        theta = dev.tr.state()
    assert np.array_equal(out["probes"][-1, 0], theta[0, [dev.n_vert, 5]]) and theta[0, dev.n_vert] > 0.0
    assert (np.diff(out["probes"][:, 0, 0]) > 0).all()      # the node follows the copper it is linked to


def test_hotspot_ties_go_to_the_lowest_vertex(ctx):
    """The symmetric board under uniform heating: whatever ties the device's theta holds at each step, the hotspot is the
    first of its maxima."""
    q = 3e-4
    with Stepping("symmetric") as dev:
        dev.tr.loads((q * T.face_area(dev.xy, dev.tri))[None, :])
        dev.tr.start([None])
        for k in range(4):
            out = dev.tr.run(DT1, 1, [0])
            theta = dev.tr.state()[0]
            tied = int((theta[:dev.n_vert] == theta[:dev.n_vert].max()).sum())
            print("step", k + 1, "vertices at the maximum:", tied, "of", dev.n_vert)
            assert out["vertex"][0, 0, 0] == int(np.flatnonzero(theta[:dev.n_vert] == theta[:dev.n_vert].max())[0])
            assert out["max"][0, 0, 0] == theta[:dev.n_vert].max()


# ---- 7. one hierarchy per dt ----------------------------------------------------------------------------------------------

def test_the_hierarchy_is_built_once_per_dt(ctx):
    """On the 49 x 49 board the schedule of the trajectory test builds two hierarchies, each inside the first step of its dt:
    every other step reports a setup time of zero."""
    with Stepping(GRID49) as dev:
        dev.loaded(1, seed=5)
        _states, runs = device_states(dev, [(dt, steps, [case]) for dt, steps, case in SCHEDULE], [None])
        hierarchies = dev.tr.clock()[2]
    setup = [r["setup_seconds"] for r in runs]
    print("setup seconds of the first steps", setup[0][0], setup[1][0], "levels", runs[0]["result"].levels)
    assert hierarchies == 2 and runs[0]["result"].levels >= 2
    assert setup[0][0] > 0.0 and setup[1][0] > 0.0
    assert (setup[0][1:] == 0.0).all() and (setup[1][1:] == 0.0).all() and (setup[2] == 0.0).all()


@pytest.mark.parametrize("name", [GRID49, "problem_many_meshes"])
def test_warm_started_steps_take_no_more_iterations_than_cold_ones(ctx, name):
    """The 12 steps of the constant segment: from the previous state they take no more iterations in total than the same
    systems S theta = rhs solved from zero.  The 49 x 49 board, and a board whose sheet conducts enough for the solve to
    take more than one iteration."""
    warm, cold = [], []
    with Stepping(name) as dev:
        dev.loaded(1, seed=5)
        dev.tr.start([None])
        S = dev.tr.matrix(DT1)
        for _ in range(12):
            rhs = dev.tr.rhs(DT1, [0])
            cold.append(S.solve_spd(rhs[0]).iterations)
            warm.append(int(dev.tr.run(DT1, 1, [0])["iterations"][0]))
    print(name, "iterations from the previous state", warm, "total", sum(warm), "from zero", cold, "total", sum(cold))
    assert sum(warm) <= sum(cold)


# ---- 8. two calls, the same bits ------------------------------------------------------------------------------------------

def everything(rep):
    arrays = [rep.times, rep.total_stored, rep.total_loss, rep.total_heat, rep.info["iterations_per_step"]]
    arrays += [layer[key] for layer in rep.layers for key in ("stored", "loss", "heat")]
    arrays += [zf.values for fields in rep.temperatures + rep.face_temperatures for forms in fields for zf in forms]
    arrays += [zf.values for forms in rep.envelope.temperatures for zf in forms] + [t for ts in rep.envelope.times for t in ts]
    arrays += list(rep.probes.values())
    return arrays, (rep.hotspots, rep.peak, rep.envelope.hotspots, rep.snapshot_times)


@pytest.mark.parametrize("name", ["two_layer", "problem_many_meshes"])
def test_two_calls_give_the_same_bits(ctx, name):
    prob, meshes, layer_of, disc, *_ = board(name)
    probes = [conn.node_id for conn in prob.networks[0].connections][:2]
    schedule = [solver.Segment(4 * DT1, 4, 0), solver.Segment(4 * DT2, 4, None)]
    runs = [quiet(solver.solve_meshed_thermal_transient, prob, meshes, layer_of, model_of(film=TT.FILM_REAL), schedule, probes=probes,
                  keep="segments", disconnected_meshes_by_layer=disc)[1] for _ in range(2)]
    (arrays_a, scalars_a), (arrays_b, scalars_b) = everything(runs[0]), everything(runs[1])
    assert scalars_a == scalars_b
    assert len(arrays_a) == len(arrays_b) and all(np.array_equal(a, b) for a, b in zip(arrays_a, arrays_b))


# ---- 9. the refusals of the device entries --------------------------------------------------------------------------------

def test_refusals_of_the_device_entries(ctx):
    """Each returns PADNE_E_INVALID (a ValueError here) and leaves the handle usable: at the end it runs a schedule to the
    bits of a fresh handle."""
    nan, inf = float("nan"), float("inf")
    with Stepping("two_layer") as dev:
        lib = ctx._lib
        for capacity in ([0.0, CAP], [CAP, nan], [-CAP, CAP], [CAP, inf], [CAP], [CAP, CAP, CAP]):
            with pytest.raises(ValueError):
                _hip.Transient(dev.thermal, capacity)
        tr = dev.tr
        Pf, heat = random_loads(dev, 2, seed=15)
        for call in (lambda: tr.start([None]), lambda: tr.run(DT1, 1, [None]), lambda: tr.rhs(DT1, [None])):
            with pytest.raises(ValueError):                # no loads yet, so no start either
                call()
        for bad_heat in (([dev.n_pot], [0], [1.0]), ([0], [2], [1.0]), ([0], [0], [inf])):
            with pytest.raises(ValueError):
                tr.loads(Pf, bad_heat)
        tr.loads(Pf, heat)
        tr.n_cols = 1
        for call in (lambda: tr.run(DT1, 1, [0]), lambda: tr.rhs(DT1, [0]), lambda: tr.state(), lambda: tr.envelope(dev.n_vert)):
            with pytest.raises(ValueError):                # loads, but no start
                call()
        for initial in ([2], [-2], [0, 5]):
            with pytest.raises(ValueError):
                tr.start(initial)
        tr.start([None, 0])
        for dt in (0.0, -DT1, nan, inf):
            for call in (lambda: tr.run(dt, 1, [0, 1]), lambda: tr.rhs(dt, [0, 1]), lambda: tr.matrix(dt)):
                with pytest.raises(ValueError):
                    call()
        for call in (lambda: tr.run(DT1, 1, [0, 2]), lambda: tr.run(DT1, 1, [-2, 0]), lambda: tr.rhs(DT1, [2, 0]),
                     lambda: tr.run(DT1, 0, [0, 1]), lambda: tr.run(DT1, 1, [0, 1], [dev.n_pot]), lambda: tr.run(DT1, 1, [0, 1], [-1])):
            with pytest.raises(ValueError):
                call()
        # a handle of another context, and no handle
        other = _hip.Context(0)
        out = np.zeros((2, dev.n_pot))
        cap = np.asarray(dev.capacity, dtype=np.float64)
        h = ctypes.c_void_p()
        ptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))                  # noqa: E731
        assert lib.padne_transient_create(other._h, dev.thermal._h, len(cap), ptr(cap), ctypes.byref(h)) == _hip.E_INVALID
        assert lib.padne_transient_create(ctx._h, None, len(cap), ptr(cap), ctypes.byref(h)) == _hip.E_INVALID
        assert lib.padne_transient_state(other._h, tr._h, ptr(out)) == _hip.E_INVALID
        assert lib.padne_transient_state(ctx._h, None, ptr(out)) == _hip.E_INVALID
        assert lib.padne_transient_destroy(None) == _hip.OK
        other.close()
        # the handle went through all of that unharmed
        assert np.array_equal(tr.state()[0], np.zeros(dev.n_pot)) and tr.clock()[0] == 0
        got = [tr.run(DT1, 3, [0, 1])["max"], tr.state()]
        fresh = _hip.Transient(dev.thermal, dev.capacity)
        try:
            fresh.loads(Pf, heat)
            fresh.start([None, 0])
            want = [fresh.run(DT1, 3, [0, 1])["max"], fresh.state()]
        finally:
            fresh.close()
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and np.isfinite(got[1]).all() and got[1].max() > 0.0


# ---- 10. the public call ---------------------------------------------------------------------------------------------------

def test_solve_thermal_transient_runs_a_duty_cycle(ctx):
    """``single`` under three repeats of an on / off pair, meshed by the call: the times, the peak against the envelope and
    the hotspot traces, a snapshot per segment end, each against the state direct stepping has there."""
    prob, meshes, layer_of, _disc, flat, _n_internal, pairs = board("single")

    class OneMesh:
        def poly_to_mesh(self, polygon, seed_points):
            return meshes[0]

    ambient = 30.0
    on, off = solver.Segment(6 * DT1, 6, 0), solver.Segment(4 * DT2, 4, None)
    resistor = next(e for e, row in pairs if row[0] == "R")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", solver.SolverWarning)
        sols, rep = solver.solve_thermal_transient(prob, model_of(ambient=ambient), [on, off], mesher=OneMesh(), repeat=3,
                                                   probes=[resistor.a], keep="segments")
    # the times
    dts = [DT1] * 6 + [DT2] * 4
    want_times = np.concatenate([[0.0], np.cumsum(dts * 3)])
    assert len(rep.times) == 31 and (np.diff(rep.times) > 0).all() and np.allclose(rep.times, want_times, rtol=1e-12, atol=0.0)
    # the peak, the envelope and the hotspot traces agree
    trace = [spot[0] for spot in rep.hotspots[0]]
    n_peak = int(np.argmax(trace))
    assert rep.peak[0] == max(trace) and rep.peak[1] == rep.times[n_peak] and rep.peak[2] == 0
    assert rep.peak[3:] == rep.hotspots[0][n_peak][1:]
    assert rep.envelope.hotspots[0][0] == rep.peak[0] and rep.envelope.hotspots[0][1] == rep.peak[1]
    assert rep.envelope.temperatures[0][0].values.max() == rep.peak[0]
    assert trace[0] == ambient and n_peak == 26            # the end of the third heating
    assert rep.snapshot_times == [rep.times[n] for n in (6, 10, 16, 20, 26, 30)] and len(rep.temperatures) == 6
    # the reference: the restated load of the solution's own potentials, stepped directly
    xy, tri, face_mesh, voff, _toff = T.flatten(flat)
    V = sols[0].layer_solutions[0].potentials[0].values
    nodes = solver.index_board(prob, meshes, layer_of).node_indexer.node_to_global_index
    a, b = nodes[resistor.a], nodes[resistor.b]
    half = (V[a] - V[b]) ** 2 / resistor.resistance / 2
    B = [T.load(len(xy), tri, T.face_power(xy, tri, face_mesh, [2.0], V), [(a, half), (b, half)])]
    checked = solver.check_thermal_model(prob, solver.ThermalModel(film=FILM))
    A, M, hM = T.operator(flat, TT.per_mesh(checked, layer_of)[0], [FILM], 0, TT.links_of(pairs, checked))
    states = R.run(A, R.capacity(voff, [CAP], M), hM, voff, B, [(DT1, 6, 0), (DT2, 4, None)] * 3)[0]
    scale = np.abs(states).max()
    for fields, n in zip(rep.temperatures, (6, 10, 16, 20, 26, 30)):
        err = np.abs(fields[0][0].values - ambient - states[n]).max()
        print("snapshot at step", n, "error / max|theta|", err / scale)
        assert err <= BAR * scale
    assert np.abs(rep.probes[resistor.a] - ambient - states[:, a]).max() <= BAR * scale
    assert rep.face_temperatures[0][0][0].values.shape == (len(tri),)

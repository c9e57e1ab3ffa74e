"""Host half of the load-case currents (no GPU): the envelope rule of ``envelope_of``, the refusals that come before the
device, and the new export in the header, the library and ctypes."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import helpers as H
from padne_amd import _hip, build, mesh, problem, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_envelope_of_is_the_first_argmax_of_the_magnitudes():
    rng = np.random.default_rng(0)
    for k, n in [(2, 50), (3, 257), (9, 1000), (17, 64)]:
        values = rng.normal(size=(k, n))
        # planted ties at the maximum: two cases hold the column's largest magnitude, with either sign; a column that is zero
        # in every case and one that is the same in every case
        for col in range(0, n, 5):
            a, b = rng.choice(k, size=2, replace=False)
            top = np.abs(values[:, col]).max() + 1.0
            values[a, col], values[b, col] = top * rng.choice([-1.0, 1.0]), top * rng.choice([-1.0, 1.0])
        values[:, 3] = 0.0
        values[:, 4] = -2.5
        best, case = solver.envelope_of(values)
        want = np.argmax(np.abs(values), axis=0)
        assert case.dtype == np.int32 and best.dtype == np.float64 and best.shape == case.shape == (n,)
        assert np.array_equal(case, want)
        assert np.array_equal(best, np.abs(values)[want, np.arange(n)])
        assert case[3] == 0 and best[3] == 0.0 and case[4] == 0 and best[4] == 2.5
        ties = sum(int((np.abs(values[:, c]) == best[c]).sum() > 1) for c in range(n))
        assert ties >= n // 10


def test_envelope_of_a_nan_column_and_one_case():
    values = np.array([[1.0, np.nan, -3.0], [-2.0, np.nan, 3.0], [2.0, np.nan, 1.0]])
    best, case = solver.envelope_of(values)
    assert list(case) == [1, 0, 0] and best[0] == 2.0 and np.isnan(best[1]) and best[2] == 3.0
    assert np.array_equal(case, np.argmax(np.abs(values), axis=0))
    best, case = solver.envelope_of(values[1:2])
    assert np.array_equal(best, np.abs(values[1]), equal_nan=True) and not case.any()
    best, case = solver.envelope_of(np.zeros((4, 0)))
    assert best.shape == case.shape == (0,)
    for bad in (np.zeros(3), np.zeros((0, 3)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match=r"\(k, n\)"):
            solver.envelope_of(bad)


def fixture_board(name):
    g = H.load_golden(name)
    prob, _ids, flat = H.build_problem(g, problem)
    ms = H.problem_meshes(g)
    return prob, [mesh.Mesh(xy, tri) for xy, tri, _ in ms], [layer for _, _, layer in ms], flat


def test_invalid_arguments_are_refused_before_the_device(monkeypatch):
    def no_device(*_a, **_k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(solver, "get_context", no_device)
    monkeypatch.setattr(_hip, "Context", no_device)
    monkeypatch.setattr(_hip, "load_library", no_device)
    prob, meshes, layer_of, flat = fixture_board("problem_mixed")
    top = prob.layers[0]
    source = next(e for e in flat if solver.element_kind(e) == "CurrentSource")
    resistor = next(e for e in flat if solver.element_kind(e) == "Resistor")
    good_cut, many = solver.Cut(top, (0, 0), (1, 1)), types.SimpleNamespace(world=2, rank=0)

    def refused(cases, cuts, match, **kwargs):
        with pytest.raises(ValueError, match=match):
            solver.solve_meshed_load_case_currents(prob, meshes, layer_of, cases, cuts, **kwargs)
        with pytest.raises(ValueError, match=match):
            solver.solve_load_case_currents(prob, cases, cuts, mesher=object(), **kwargs)

    refused([], [good_cut], "no load cases")
    refused({source: 1.0}, [good_cut], "sequence of mappings")
    refused([{resistor: 1.0}], [good_cut], "cannot vary")
    refused([{}, {source: np.nan}], [good_cut], "must be finite")
    refused([{}], [solver.Cut(top, (0, np.inf), (1, 1))], "not finite")
    refused([{}], [solver.Cut(top, (2, 3), H.XY(2, 3))], "same point")
    refused([{}], [good_cut] * (solver.MAX_CUTS + 1), "at most 4096")
    refused([{}], good_cut, "sequence of Cut")
    refused([{}, {source: 2.0}], [good_cut], "load-case currents are solved on one GPU", partition=many)
    refused([{}], [], "row-partitioned", partition=many, per_case_fields=False)


def test_the_new_export_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "padne_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+padne_kkt_current_cases\s*\(", text)
    build.build(verbose=False)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert hasattr(lib, "padne_kkt_current_cases")
    restype, argtypes = _hip.SIGNATURES["padne_kkt_current_cases"]
    declaration = re.search(r"padne_kkt_current_cases\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert restype is ctypes.c_int and len(argtypes) == len(declaration.split(",")) == 17
    assert callable(_hip.KktPlan.current_cases)

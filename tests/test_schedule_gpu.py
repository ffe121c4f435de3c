"""The launch schedule of the engine, pinned: for five small configurations that between them take every branch of
Engine.forward / Engine.backward and of TrainStep's eager step, the sequence of C-ABI entry points of one pass (with the
encoder-level tag each launch is filed under) and SHA-256 digests of what the pass computes equal what
tests/golden/make_step_trace.py recorded (tests/golden/step_trace.json; two runs of the generator in two processes gave the
same file).  No tolerances: the schedule has no atomics and no data-dependent launch, so a refactoring of the host side
changes neither list nor bit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu


def _generator(golden_dir):
    spec = importlib.util.spec_from_file_location("make_step_trace", os.path.join(golden_dir, "make_step_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E"])
def test_step_trace_equals_the_pinned_schedule(case, golden_dir, monkeypatch):
    from randlanet import _hip as H
    gen = _generator(golden_dir)
    with open(os.path.join(golden_dir, "step_trace.json")) as f:
        want = json.load(f)[case]
    calls = []
    monkeypatch.setattr(H, "check", gen.tracer(calls))
    got = gen.run_case(case, calls)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        if key.startswith("calls"):
            first = next((i for i, (g, w) in enumerate(zip(got[key], want[key])) if g != w), min(len(got[key]), len(want[key])))
            assert got[key] == want[key], (case, key, f"first difference at launch {first}", got[key][first:first + 3], want[key][first:first + 3])
        else:
            assert got[key] == want[key], (case, key)

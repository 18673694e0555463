"""The launches of a forward, call for call: every C-ABI call of one Engine.forward_stft -- entry point, plain int / float arguments,
stream by order of first appearance -- equals what tests/golden/forward_traces.json holds (recorded by
scripts/record_forward_traces.py on an MI355X before the forward's host code was split into a plan and a launch loop).  A change
of the host code that is meant to leave the launches alone shows here; one that is meant to change them records the fixture anew."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_forward_traces", os.path.join(ROOT, "scripts", "record_forward_traces.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

with open(recorder.FIXTURE) as _f:
    GOLD = json.load(_f)


def test_the_fixture_holds_every_case():
    assert sorted(GOLD) == sorted(recorder.CASES)


@pytest.mark.parametrize("name", list(recorder.CASES))
def test_forward_issues_the_recorded_launches(name):
    got = json.loads(json.dumps(recorder.record(name)))  # (as the fixture went through JSON)
    want = GOLD[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: call {i} is {g}, recorded {w}"
    assert len(got) == len(want), f"{name}: {len(got)} calls, recorded {len(want)}"

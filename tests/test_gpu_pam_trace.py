"""Which form every PAM window takes, pinned: fixed scenarios (tests/_pam_trace.py) on
both sides of the restricted prefetch's gate, with a window that hands a proposal back,
without the tables' bounds and without the one-workgroup windows -- medoids, accept
flags and the counters (prefetch hits, misses, restricted passes, passes over all
frames, one-workgroup windows, of them ended early, slots taken over) after every
sweep, against tests/golden/pam_window_trace.json.  That file holds what the library
computed before its window path was split into steps; the medoids and accept flags do
not depend on the form a window takes, the counters are the form."""
import json
import os

import pytest

import _pam_trace

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "pam_window_trace.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_scenarios_are_the_recorded_ones(golden):
    assert sorted(golden) == sorted(_pam_trace.SCENARIOS)


@pytest.mark.parametrize("name", sorted(_pam_trace.SCENARIOS))
def test_pam_window_trace(golden, name):
    got = _pam_trace.run(name)["sweeps"]
    want = golden[name]["sweeps"]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        print(name, "sweep", i, "counters", g["counters"])
        assert g["counters"] == w["counters"], (name, i)
        assert g["accept"] == w["accept"], (name, i)
        assert g["medoids"] == w["medoids"], (name, i)


def test_the_recorded_trace_reaches_the_branches(golden):
    """(a trace in which the branch under test never ran pins nothing)"""
    last = {name: r["sweeps"][-1]["counters"] for name, r in golden.items()}
    hits, misses, restricted, full, windows, early, ahead = last["n16384"]
    assert restricted > 0 and full > 0 and windows > 0 and ahead > 0
    assert last["n16383"][2:] == [0, 4, 0, 0, 0]       # below the gate: passes over all frames
    assert last["n16384_max_pairs_1"][5] > 0
    assert last["pairs_k400_max_pairs_1"][5] > 0
    assert last["n16384_bounds_off"][2] > 0
    assert last["n16384_one_workgroup_off"][2] > 0 and last["n16384_one_workgroup_off"][4] == 0

"""The refusals of far3d_dwconv3x3_nhwc, far3d_dwconv3x3_act_nhwc and far3d_dwsep_conv_nhwc, character for character.

tests/golden/dw_refusals.json (tools/gen_golden_dw_refusals.py) holds what the library answered, before the three entries shared their
checks, to every single faulty argument and to every pair of them -- the pair pins the order of the checks.  Per entry: the argument
names, a base call that passes, the faults (name -> overrides) and the calls as [fault index, (fault index,) message index].  Every
call ends in an argument check: nothing is launched, the made-up pointers are never read, no GPU is needed.
"""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_refusals.json")
ENTRIES = ("far3d_dwconv3x3_nhwc", "far3d_dwconv3x3_act_nhwc", "far3d_dwsep_conv_nhwc")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_refusals_of_all_three_entries(golden):
    assert set(golden["entries"]) == set(ENTRIES) and golden["status"] == -1
    for name, e in golden["entries"].items():
        calls = e["calls"]
        assert sum(len(c) == 2 for c in calls) == len(e["faults"]) >= 19 and sum(len(c) == 3 for c in calls) >= 150
        assert all(golden["messages"][c[-1]].startswith(name + ": ") for c in calls)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_are_the_recorded_ones(hip_lib, golden, entry):
    e = golden["entries"][entry]
    fn, faults = getattr(hip_lib, entry), list(e["faults"])
    wrong = []
    for *which, m in e["calls"]:
        args = dict(zip(e["args"], e["base"]))
        for i in which:
            args.update(e["faults"][faults[i]])
        status = fn(*[args[a] for a in e["args"]])
        message = hip_lib.far3d_last_error().decode()
        if (status, message) != (golden["status"], golden["messages"][m]):
            wrong.append(([faults[i] for i in which], status, message, golden["messages"][m]))
    assert not wrong, "%d calls answer differently, the first: %r" % (len(wrong), wrong[0])

"""The refusals of the normalisation family's entries, character for character.

tests/golden/norm_refusals.json (tools/gen_golden_norm_refusals.py) holds what the library answered, before the entries shared their
checks and their dispatch, to every single faulty argument and to every pair of them -- the pair pins the order of the checks.  Per
entry: the argument names, a base call that passes, the faults (name -> overrides) and the calls as [fault index, (fault index,)
message index].  Every call ends in an argument check: nothing is launched, the made-up pointers are never read, no GPU is needed.

far3d_groupnorm_nhwc's `groups * 2 <= C` rule is in the fixture in pairs only: the recorded library checked it after its first launch.
It is checked in front of that launch now, and has its own case here.
"""
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_refusals.json")
ENTRIES = ("far3d_layernorm", "far3d_layernorm_rows", "far3d_row_affine_ln", "far3d_ese_nhwc", "far3d_ese_fused_nhwc",
           "far3d_groupnorm_nhwc", "far3d_maxpool3x3s2_nhwc", "far3d_cam_embed_chain")
PAIRS_ONLY = {"far3d_groupnorm_nhwc": 1}      # faults of an entry that are recorded in pairs and never alone


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_refusals_of_all_eight_entries(golden):
    assert set(golden["entries"]) == set(ENTRIES) and golden["status"] == -1
    for name, e in golden["entries"].items():
        calls = e["calls"]
        assert sum(len(c) == 2 for c in calls) == len(e["faults"]) - PAIRS_ONLY.get(name, 0) >= 9 and sum(len(c) == 3 for c in calls) >= 30
        # far3d_layernorm_rows shares far3d_layernorm's checks and, behind its own first one, their texts
        assert all(golden["messages"][c[-1]].startswith((name + ": ", name.replace("_rows", "") + ": ")) for c in calls)
    gn = golden["entries"]["far3d_groupnorm_nhwc"]
    late = list(gn["faults"]).index("groups * 2 > C")
    assert [late] not in [c[:-1] for c in gn["calls"]] and any(late in c[:-1] for c in gn["calls"])


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


def test_groupnorm_refuses_too_many_groups_with_its_text(hip_lib):
    """C = 32 with 32 groups passes the null, size and storage checks; gn_stats_kernel needs two channels per group.  This pins the
    status and the text.  That the check stands in front of the first launch is evidenced by the source (far3d_groupnorm_nhwc in
    csrc/norm.hip), not by this test: without a GPU a launch attempted first fails and leaves the same answer."""
    status = hip_lib.far3d_groupnorm_nhwc(0x10000, 1, 0x70000, 0x80000, 0x20000, 0x50000, 2, 35, 32, 32, 1e-5, 1, 0)
    assert (status, hip_lib.far3d_last_error().decode()) == (-1, "far3d_groupnorm_nhwc: groups*2 must be <= C")

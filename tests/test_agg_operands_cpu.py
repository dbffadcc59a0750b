"""CPU: the float64 restatement and the bounds of tests/agg_operand_refs.py, the host predicate ops.aggregate_fused_supported and the
construction of the aggregation module at a shape outside the fused family.  No device."""
import pytest
import torch

from tests import agg_operand_refs as R
from tests import cases


def test_restatement_through_msda_equals_aggregation_ref():
    """operands_ref -> oracle msda_grid_sample -> sum over cameras == oracle aggregation_ref on the same float64 logits, to float64
    rounding."""
    from oracle import sampling
    ac = cases.small_aggregate_case()
    c = R.from_aggregate_case("t", ac)
    loc, w, _ = R.operands_ref(c)
    N, S, C = ac["feat"].shape
    G = ac["G"]
    shapes = torch.as_tensor([list(x) for x in ac["level_hw"]], dtype=torch.long)
    starts = torch.as_tensor(ac["level_start"], dtype=torch.long)
    got = sampling.msda_grid_sample(ac["feat"].double().reshape(N, S, G, C // G), shapes, starts, loc, w).sum(0)
    d = lambda t: t.double()
    logits = d(ac["U"])[:, None, :] + d(ac["Vc"])[None, :, :]
    want = sampling.aggregation_ref(d(ac["feat"]), d(ac["ref"]), d(ac["offsets"]), d(ac["lidar2img"]), logits, ac["level_hw"],
                                    ac["level_start"], torch.tensor(ac["pc_range"], dtype=torch.float32).double(), ac["pad_hw"], num_groups=G)
    err = (got - want).abs().max().item()
    print("restatement vs aggregation_ref, float64 logits: %.3e" % err)
    assert err < 1e-12 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("name", R.CASES)
def test_float32_evaluation_stays_inside_both_bounds(name):
    c = R.case(name)
    loc32, w32, _ = R.operands_ref(c, torch.float32)
    R.check_locations(loc32[:, :, 0, 0], c, name + " (float32 torch)")
    R.check_weights(w32, c, name + " (float32 torch)")       # the yardstick itself: holds by construction, sums included


@pytest.mark.parametrize("name", R.CASES)
def test_no_element_near_the_clamp(name):
    """No float64 z within 100 x the exclusion margin of 1e-5: the exclusion cap is never used.  The near case has points behind a
    camera, so the clamp branch itself runs."""
    c = R.case(name)
    clear = R.clamp_clearance(c)
    print("%s: clamp clearance %.1f margins" % (name, clear))
    assert clear > 100.0
    if name == "near":
        z = R.loc_bound(c)[2]
        assert int((z < 1e-5).sum()) > 0


def test_table_cases_are_the_issue_shapes():
    want = [(1, 1, 1, 1, 1, 1), (2, 2, 5, 4, 3, 5), (1, 3, 37, 8, 4, 13), (1, 5, 67, 8, 4, 16), (1, 17, 9, 2, 4, 16)]
    assert [R.case(n)["dims"] for n in R.TABLE_CASES] == want
    assert R.case("near")["dims"] == (1, 3, 96, 8, 4, 13)


def test_aggregate_fused_supported_is_the_documented_family():
    """include/far3d_hip.h, far3d_aggregate_forward: "Requires C=256, G=8, L<=4, N<=16, N*P<=256, N*P*L<=384"."""
    import os
    import re
    from far3d_amd import ops
    from tests.conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "far3d_hip.h")).read()
    m = re.search(r"Requires C=(\d+), G=(\d+), L<=(\d+), N<=(\d+),\s*\*?\s*N\*P<=(\d+), N\*P\*L<=(\d+)", hdr)
    assert m, "the header no longer states the family in this form"
    C0, G0, Lm, Nm, NPm, NLPm = (int(v) for v in m.groups())
    assert (C0, G0, Lm, Nm, NPm, NLPm) == (256, 8, 4, 16, 256, 384)
    f = ops.aggregate_fused_supported
    for C in (128, 256, 512):
        for G in (4, 8, 16):
            for L in (0, 1, 3, 4, 5):
                for N in (0, 1, 6, 7, 16, 17, 20):
                    for P in (0, 1, 5, 13, 16, 17, 24, 64):
                        want = (C == C0 and G == G0 and 1 <= L <= Lm and 1 <= N <= Nm and P >= 1 and N * P <= NPm and N * P * L <= NLPm)
                        assert f(C, G, L, N, P) == want, (C, G, L, N, P)
    assert f(256, 8, 4, 7, 13) and f(256, 8, 4, 6, 13)          # the benchmark and the reference default
    assert not f(256, 8, 4, 8, 13)                               # 8 * 13 * 4 = 416 > 384
    assert not f(128, 4, 3, 2, 5)


def test_module_builds_outside_the_family():
    from far3d_amd import plugin
    m = plugin.ATTENTION.build(dict(type="DeformableFeatureAggregationCuda", embed_dims=128, num_groups=4, num_levels=3, num_cams=2,
                                    num_pts=5))
    assert m.weights_fc.weight.shape == (4 * 3 * 5, 128) and m.learnable_fc.weight.shape == (15, 128)
    assert m.cam_embed[0].weight.shape == (64, 12) and m.output_proj.weight.shape == (128, 128)
    assert callable(m.sampling_operands)

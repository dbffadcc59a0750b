"""CPU: multi-depth 2D proposals (multi_depth_config.topk > 1) -- the test-side restatement against the reference's fixtures, and
the plugin / config surface that carries the option to the engine."""
import json
import os

import numpy as np
import pytest
import torch

from far3d_amd import config, engine, plugin, synth
from oracle import far3d_oracle
from tests import md_oracle
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")


def _roi_from_fixture(z, fi, rc, ds=8):
    """The 2D-stage outputs the multi-depth branch reads, rebuilt from a fixture: boxes / scores per camera, the selection mask, and a
    depth-probability map holding each primary's recorded probabilities at its centre cell (the only cells the branch reads)."""
    N = rc["num_cams"]
    H, W = rc["pad_hw"][0] // ds, rc["pad_hw"][1] // ds
    vi = z["f%d_valid_idx" % fi]
    S = int(vi[:, 1].max()) + 1
    valid = torch.zeros((N, S, 1), dtype=torch.bool)
    valid[vi[:, 0], vi[:, 1], 0] = True
    boxes = torch.from_numpy(z["f%d_bbox2d" % fi])
    probs = torch.from_numpy(z["f%d_cell_probs" % fi])                   # (M, D): D = the depth head's channels
    pred_depth = torch.zeros((N, probs.shape[1], H, W))
    cams = torch.from_numpy(vi[:, 0]).long()
    c2 = (boxes[:, :2] / ds).round().long()
    c2[c2 < 0] = 0
    c2[:, 0][c2[:, 0] >= W] = W - 1
    c2[:, 1][c2[:, 1] >= H] = H - 1
    pred_depth[cams, :, c2[:, 1], c2[:, 0]] = probs
    bbox_list = [boxes[cams == n] for n in range(N)]
    return dict(pred_depth=pred_depth, valid_indices=valid, bbox_list=bbox_list,
                bbox2d_scores=torch.from_numpy(z["f%d_bbox2d_scores" % fi])), S


@pytest.mark.parametrize("name", ["far3d_md2_seq", "far3d_md3_seq"])
def test_restatement_matches_the_reference_multi_depth_rows(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    rc = json.loads(bytes(z["recipe"]).decode())
    K = rc["multi_depth"]["topk"]
    assert K > 1
    cfg = far3d_oracle.default_cfg(num_cams=rc["num_cams"], multi_depth=rc["multi_depth"])
    orc = md_oracle.MultiDepthOracle({"pts_bbox_head.pc_range": torch.tensor(cfg["pc_range"])}, cfg)
    for fi in range(rc["frames"]):
        data, _ = synth.recipe_frame(rc, fi)
        roi, S = _roi_from_fixture(z, fi, rc)
        ref2d, ctx = orc._proposals(roi, torch.zeros((rc["num_cams"], S, 256)), data, tuple(rc["pad_hw"]))
        md = orc.last_md
        M, V = int(z["f%d_M" % fi]), int(z["f%d_V" % fi])
        assert md["M"] == M and md["V"] == V and 0 < V < M
        assert np.array_equal(md["valid"].numpy(), z["f%d_md_valid" % fi])
        want = z["f%d_ref2d" % fi]
        assert ref2d.shape[1] == M + (K - 1) * V == want.shape[0] == z["f%d_all_cls_scores" % fi].shape[2] - rc["num_query"] - rc["num_propagated"]
        assert np.abs(ref2d[0].numpy() - want).max() < 1e-5, "frame %d: %.3e" % (fi, np.abs(ref2d[0].numpy() - want).max())
        # extra rows: k-major copies of the valid primaries, log-odds scaled by p_k / p_0 < 1
        vrows = np.nonzero(z["f%d_md_valid" % fi])[0]
        assert md["rows"].tolist() == list(range(M)) + vrows.tolist() * (K - 1)
        lo = ctx[0, :, -1]
        assert torch.all(lo[M:].abs() <= lo[md["rows"][M:]].abs() + 1e-6)


def test_range_min_bin_is_the_references():
    # farhead.py:521-531 with the shipped values: 30 m -> bin 25
    assert md_oracle.range_min_bin(far3d_oracle.default_cfg(), 30) == 25
    dc = engine.default_cfg()["depthnet"]
    from far3d_amd import ops
    for r in (0, 1.5, 29.224, 30, 55, 109.0):
        assert ops.depth_range_min_bin(dc, r) == md_oracle.range_min_bin(far3d_oracle.default_cfg(), r)


def test_topk2_config_builds_farhead_and_reaches_engine_cfg():
    det = plugin.build_detector(config.default_model_cfg(num_query=60, num_propagated=16,
                                                         multi_depth_config=dict(topk=2, range_min=30)))
    assert det.pts_bbox_head.multi_depth_config == dict(topk=2, range_min=30)
    assert det.engine_cfg()["multi_depth"] == dict(topk=2, range_min=30)
    assert det.pts_bbox_head.engine_cfg()["multi_depth"] == dict(topk=2, range_min=30)
    assert engine.multi_depth_topk(det.engine_cfg()) == 2
    # the default stays single-depth; the reference's -1 (plain argmax) is the same computation as 1
    assert plugin.build_detector(config.default_model_cfg()).engine_cfg()["multi_depth"]["topk"] == 1
    det = plugin.build_detector(config.default_model_cfg(multi_depth_config=dict(topk=-1, range_min=30)))
    assert engine.multi_depth_topk(det.engine_cfg()) == 1


@pytest.mark.parametrize("k", [0, 9, -2])
def test_unsupported_topk_is_refused(k):
    with pytest.raises(ValueError, match="topk"):
        plugin.build_detector(config.default_model_cfg(multi_depth_config=dict(topk=k, range_min=30)))
    with pytest.raises(ValueError, match="topk"):
        engine.multi_depth_topk(dict(multi_depth=dict(topk=k)))

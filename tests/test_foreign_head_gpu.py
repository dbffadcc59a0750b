"""GPU: FarHead.forward on the reference-format dict of a FOREIGN 2D head (bbox_list, valid_indices, bbox2d_scores, pred_depth; ref
farhead.py:571-610, 711-827) -- against the oracle on the oracle's own 2D statement, against the native path on our own 2D head's
dict with the private '_far3d' entry stripped (topk 1 and 3), and the refusals.  Rig as in tests/test_plugin_modules_gpu.py: the
far3d_small_seq recipe, fp32 modules; bounds of test_modules_chain_like_the_reference_detector (logits 1e-3, assert_detections_match)."""
import json
import os

import numpy as np
import pytest
import torch

from far3d_amd import config, plugin, synth, weights
from tests.conftest import ROOT, assert_detections_match

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("bbox_list", "valid_indices", "bbox2d_scores", "pred_depth")


@pytest.fixture(scope="module")
def rig(hip_lib):
    """The recipe, a detector factory, and the oracle's statement of both frames (FPN maps, 2D dict, head outputs, detections),
    computed once."""
    from oracle import far3d_oracle
    z = np.load(os.path.join(ROOT, "tests", "golden", "far3d_small_seq.npz"))
    rc = json.loads(bytes(z["recipe"]).decode())
    kw = dict(num_cams=rc["num_cams"], num_query=rc["num_query"], num_propagated=rc["num_propagated"], memory_len=rc["memory_len"],
              topk_proposals=rc["topk_proposals"])
    sd = weights.init_state_dict(weights.detector_spec(rc["backbone"], num_query=rc["num_query"], num_propagated=rc["num_propagated"]),
                                 seed=rc["weight_seed"])

    def make(multi_depth_config=None):
        det = plugin.build_detector(config.default_model_cfg(multi_depth_config=multi_depth_config, **kw))
        det.load_state_dict(sd)
        for m in (det.img_backbone, det.img_neck, det.img_roi_head, det.pts_bbox_head):
            m.precision = "fp32"
        return det

    orc = far3d_oracle.Far3DOracle(sd, far3d_oracle.default_cfg(**kw))
    frames = []
    for fi in range(2):
        data, metas = synth.recipe_frame(rc, fi)
        prev = torch.zeros(1) if fi == 0 else torch.ones(1)
        with torch.no_grad():
            w_fpn = orc.fpn(orc.backbone(data["img"][0]))
            w_roi = orc.roi_head(w_fpn)
            w_roi.update(orc.get_bboxes(w_roi))
            w_out = orc.head_forward(w_fpn, w_roi, data, prev, tuple(rc["pad_hw"]))
            w_res = orc.decode(w_out)
        frames.append(dict(data=data, metas=metas, prev=prev, roi=w_roi, out=w_out, res=w_res, fpn=w_fpn, feats=[f[None].to(DEV) for f in w_fpn],
                           dev_data={k: v.to(DEV) for k, v in data.items() if k != "img"}))
    make.oracle = lambda: far3d_oracle.Far3DOracle(sd, far3d_oracle.default_cfg(**kw))
    return make, rc, frames


def head_call(head, fr_, roi):
    return head(fr_["metas"], roi, img_feats=fr_["feats"], prev_exists=fr_["prev"], **fr_["dev_data"])


def test_foreign_dict_of_the_oracle_matches_the_oracle(rig):
    """The oracle's own roi_head + get_bboxes dict -- the reference's keys, no '_far3d' -- as CPU tensors for frame 0 and as device
    tensors for frame 1, through the streaming memory."""
    make, rc, frames = rig
    head = make().pts_bbox_head
    for fi, f in enumerate(frames):
        roi = dict(f["roi"])
        assert "_far3d" not in roi and all(k in roi for k in KEYS)
        if fi == 1:
            roi = {k: ([b.to(DEV) for b in v] if isinstance(v, (list, tuple)) else v.to(DEV) if isinstance(v, torch.Tensor) else v)
                   for k, v in roi.items()}
        out = head_call(head, f, roi)
        assert out["dn_mask_dict"] is None
        err = (out["all_cls_scores"].cpu() - f["out"]["all_cls_scores"]).abs().max().item()
        print("[foreign head] frame %d: %d adaptive queries, logits err %.3e" % (fi, out["reference_points2d"].shape[1], err))
        assert err < 1e-3
        boxes, scores, labels = head.get_bboxes(out, f["metas"])[0]
        assert_detections_match((labels.cpu().numpy(), boxes.cpu().numpy(), scores.cpu().numpy()),
                                tuple(f["res"][k].numpy() for k in ("labels_3d", "boxes_3d", "scores_3d")), "frame %d" % fi)


@pytest.mark.parametrize("md", [None, dict(topk=3, range_min=30)], ids=["topk1", "topk3"])
def test_native_dict_without_its_private_entry_gives_the_native_result(rig, md):
    """Our own 2D head's dict on the native path, and the same dict with '_far3d' stripped on the foreign path, two frames on two
    freshly built heads: the same number of adaptive-query rows (M, or M' for topk = 3) and the same logits within 1e-3."""
    make, rc, frames = rig
    det_a, det_b = make(md), make(md)
    for fi, f in enumerate(frames):
        roi = det_a.img_roi_head(None, img_feats=f["feats"], **f["dev_data"])
        roi.update(det_a.img_roi_head.get_bboxes(roi))
        native = head_call(det_a.pts_bbox_head, f, roi)
        stripped = {k: v for k, v in roi.items() if k != "_far3d"}
        foreign = head_call(det_b.pts_bbox_head, f, stripped)
        Mn, Mf = native["reference_points2d"].shape[1], foreign["reference_points2d"].shape[1]
        err = (foreign["all_cls_scores"] - native["all_cls_scores"]).abs().max().item()
        print("[foreign head] %s frame %d: rows native %d foreign %d (boxes %d), logits diff %.3e" % (
            "topk1" if md is None else "topk3", fi, Mn, Mf, sum(b.shape[0] for b in roi["bbox_list"]), err))
        assert Mn == Mf and Mn > 0
        assert foreign["all_cls_scores"].shape == native["all_cls_scores"].shape and err < 1e-3


def test_all_cameras_empty_runs_like_the_reference_without_proposals(rig):
    """No box and no selected token in any camera (farhead.py:727 returns no proposal): the head runs on its learned and propagated
    queries alone, as a fresh oracle does on the same emptied dict."""
    make, rc, frames = rig
    f = frames[0]
    roi = {k: f["roi"][k] for k in KEYS}
    empty = dict(roi, bbox_list=[b[:0] for b in roi["bbox_list"]], bbox2d_scores=roi["bbox2d_scores"][:0],
                 valid_indices=torch.zeros_like(roi["valid_indices"]))
    with torch.no_grad():
        want = make.oracle().head_forward(f["fpn"], dict(f["roi"], **empty), f["data"], f["prev"], tuple(rc["pad_hw"]))
    head = make().pts_bbox_head
    out = head_call(head, f, empty)
    assert out["reference_points2d"].shape[1] == 0
    assert out["all_cls_scores"].shape == want["all_cls_scores"].shape == (head.num_layers, 1, rc["num_query"] + rc["num_propagated"], head.num_classes)
    assert (out["all_cls_scores"].cpu() - want["all_cls_scores"]).abs().max().item() < 1e-3
    # a selected token without a box is a disagreement, not an empty frame
    one = torch.zeros_like(roi["valid_indices"])
    one.view(one.shape[0], -1)[0, 5] = True
    with pytest.raises(ValueError, match="disagree"):
        head_call(head, f, dict(empty, valid_indices=one))


def test_refusals_name_their_cause(rig):
    make, rc, frames = rig
    head = make().pts_bbox_head
    f = frames[0]
    good = {k: f["roi"][k] for k in KEYS}
    with pytest.raises(ValueError, match="pred_depth"):                                   # a missing key
        head_call(head, f, {k: v for k, v in good.items() if k != "pred_depth"})
    with pytest.raises(ValueError, match="bbox_list, valid_indices, bbox2d_scores, pred_depth"):
        head_call(head, f, dict(enc_cls_scores=[]))
    with pytest.raises(ValueError, match=r"pred_depth must be \(\d+, 51, hd, wd\)"):      # a wrong D
        head_call(head, f, dict(good, pred_depth=good["pred_depth"][:, :-1]))
    with pytest.raises(ValueError, match=r"valid_indices must be"):                       # a wrong S
        head_call(head, f, dict(good, valid_indices=good["valid_indices"][:, :-1]))
    nums = [b.shape[0] for b in good["bbox_list"]]
    n = max(range(len(nums)), key=lambda i: nums[i])
    assert nums[n] >= 1
    off = sum(nums[:n])
    short = [b if i != n else b[:-1] for i, b in enumerate(good["bbox_list"])]
    sc = good["bbox2d_scores"]
    with pytest.raises(ValueError, match=r"boxes per camera \[.*\], selected tokens per camera \[.*\]"):
        head_call(head, f, dict(good, bbox_list=short, bbox2d_scores=torch.cat([sc[:off + nums[n] - 1], sc[off + nums[n]:]])))
    # moving a box from one camera to another keeps M: only the device-side comparison can see it
    if len(nums) > 1:
        m = (n + 1) % len(nums)
        moved = list(short)
        moved[m] = torch.cat([good["bbox_list"][m], good["bbox_list"][n][-1:]])
        with pytest.raises(ValueError, match="disagree"):
            head_call(head, f, dict(good, bbox_list=moved))
    # the head still serves the good dict afterwards
    out = head_call(head, f, good)
    assert (out["all_cls_scores"].cpu() - f["out"]["all_cls_scores"]).abs().max().item() < 1e-3

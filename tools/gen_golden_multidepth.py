"""Golden fixtures of the multi-depth 2D proposals (multi_depth_config.topk = K > 1; BUILD CONTAINER ONLY: needs the reference).

  python tools/gen_golden_multidepth.py [name ...]   # writes tests/golden/far3d_md2_seq.npz, far3d_md3_seq.npz (or the named ones)

Same pipeline as tools/gen_golden.py (its run_reference, the reference detector built by oracle/refload.py from its own files),
with cfg.pts_bbox_head.multi_depth_config = {topk: K, range_min: R}.  R is chosen from the frames' own depth maps so that every
frame has some, but not all, primaries at or beyond it (0 < V < M).  The reference's adaptive reference points are captured by
wrapping build_query2d_proposal on the instance; the test-side restatement (tests/md_oracle.py) is asserted against them and
against the logits / boxes at gen_golden.py's 2e-4 * scale bar.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from far3d_amd import synth, weights  # noqa: E402
from oracle import far3d_oracle, refload  # noqa: E402
from tests import md_oracle  # noqa: E402
from gen_golden import GOLD, SMALL, run_reference  # noqa: E402

MD2 = dict(SMALL, name="far3d_md2_seq", multi_depth=dict(topk=2))
MD3 = dict(SMALL, name="far3d_md3_seq", multi_depth=dict(topk=3), frames=2, scene_change_at=None, data_seed=7)


def _ocfg(c, md):
    return far3d_oracle.default_cfg(num_cams=c["num_cams"], num_query=c["num_query"], num_propagated=c["num_propagated"],
                                    memory_len=c["memory_len"], topk_proposals=c["topk_proposals"], multi_depth=md)


def choose_range_min(c, sd):
    """A range_min (metres) that splits every frame's primaries by their best bin (0 < V < M): the shipped 30 m if it does, else
    the middle of the bin that splits them most evenly."""
    orc = md_oracle.MultiDepthOracle(sd, _ocfg(c, dict(topk=c["multi_depth"]["topk"], range_min=0.0)))
    tops = []
    with torch.no_grad():
        for fi in range(c["frames"]):
            data, metas = synth.recipe_frame(c, fi)
            orc.simple_test(data, metas)
            tops.append(orc.last_md["topk_idx"][:, 0])
    best, score = None, -1
    for b in range(1, orc.cfg["depth_bins"]):
        s = min(min(int((t >= b).sum()), int((t < b).sum())) for t in tops)
        if s > score:
            best, score = b, s
    assert score > 0, "no depth bin splits every frame's primaries"
    oc = orc.cfg
    b30 = md_oracle.range_min_bin(oc, 30)
    if all(0 < int((t >= b30).sum()) < len(t) for t in tops):
        return 30, b30
    bin_size = 2 * (oc["depth_max"] - oc["depth_min"]) / (oc["depth_bins"] * (1 + oc["depth_bins"]))
    R = round(float(oc["depth_min"] + bin_size / 8 * ((2 * (best + 0.5) + 1) ** 2 - 1)), 3)     # mid-bin: truncates to `best`
    assert md_oracle.range_min_bin(oc, R) == best, (R, best)
    return R, best


def generate(c):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    K = c["multi_depth"]["topk"]
    spec = weights.detector_spec(c["backbone"], num_query=c["num_query"], num_propagated=c["num_propagated"])
    sd = weights.init_state_dict(spec, seed=c["weight_seed"])
    R, rbin = choose_range_min(c, sd)
    c = dict(c, multi_depth=dict(topk=K, range_min=R))
    print("[golden-md] %s: K=%d, range_min=%.3f m (bin %d)" % (c["name"], K, R, rbin))
    cfg, _ = refload.reference_model_cfg(num_cams=c["num_cams"], num_query=c["num_query"], num_propagated=c["num_propagated"],
                                         memory_len=c["memory_len"], topk_proposals=c["topk_proposals"])
    cfg["pts_bbox_head"]["multi_depth_config"] = {"topk": K, "range_min": R}
    model = refload.build_reference_detector(cfg)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    head = model.pts_bbox_head
    assert head.add_multi_depth_proposal and head.multi_depth_config["topk"] == K
    seen = {}
    inner = head.build_query2d_proposal

    def wrapped(pred_bbox_list, pred_depth, data, bn, padHW, *a, **kw):
        ref2d, ctx = inner(pred_bbox_list, pred_depth, data, bn, padHW, *a, **kw)
        # the inputs the multi-depth branch reads: each primary's depth probabilities (BN, H, W, D) at its centre cell, gathered by
        # the reference's own cell rule (farhead.py:733-747)
        ds = int(padHW[0] / pred_depth.shape[1])
        h_max, w_max = pred_depth.shape[1:3]
        probs = []
        for i, b in enumerate(pred_bbox_list):
            c2 = (b[:, :2] / ds).round().long()
            c2[c2 < 0] = 0
            c2[:, 0][c2[:, 0] >= w_max] = w_max - 1
            c2[:, 1][c2[:, 1] >= h_max] = h_max - 1
            probs.append(pred_depth[i][c2[:, 1], c2[:, 0]])
        probs = torch.cat(probs)
        valid = torch.topk(probs, K, dim=1).indices[:, 0] >= rbin
        seen.update(M=sum(len(b) for b in pred_bbox_list), ref2d=ref2d, ctx=ctx, probs=probs, valid=valid)
        return ref2d, ctx
    head.build_query2d_proposal = wrapped
    orc = md_oracle.MultiDepthOracle(sd, _ocfg(c, c["multi_depth"]))

    gold = {}
    worst = 0.0
    with torch.no_grad():
        for fi in range(c["frames"]):
            data, metas = synth.recipe_frame(c, fi)
            metas[0]["box_type_3d"] = refload.LiDARBoxes
            seen.clear()
            r = run_reference(model, copy.deepcopy(data), metas)
            o = orc.simple_test(copy.deepcopy(data), metas)
            md = orc.last_md
            M, Mx = seen["M"], seen["ref2d"].shape[1]
            assert (Mx - M) % (K - 1) == 0
            V = (Mx - M) // (K - 1)
            assert M == md["M"] and V == md["V"] and 0 < V < M, (fi, M, V, md["M"], md["V"])
            assert int(seen["valid"].sum()) == V and torch.equal(seen["valid"], md["valid"])
            pairs = [("ref2d", seen["ref2d"][0], md["ref2d"]), ("ctx", seen["ctx"][0], md["ctx"]),
                     ("depth_logit", r["roi"]["depth_logit"], o["roi"]["depth_logit"]),
                     ("bbox2d", torch.cat(r["roi"]["bbox_list"]), torch.cat(o["roi"]["bbox_list"])),
                     ("all_cls_scores", r["outs"]["all_cls_scores"], o["all_cls_scores"]),
                     ("all_bbox_preds", r["outs"]["all_bbox_preds"], o["all_bbox_preds"])]
            for name, a, b in pairs:
                assert a.shape == b.shape, (fi, name, a.shape, b.shape)
                err = (a - b).abs().max().item() if a.numel() else 0.0
                worst = max(worst, err)
                scale = max(1.0, a.abs().max().item()) if a.numel() else 1.0
                assert err < 2e-4 * scale, "frame %d %s: restatement deviates from the reference by %.3e" % (fi, name, err)
                if name == "all_cls_scores":
                    gold["f%d_oracle_logit_dev" % fi] = np.float32(err)
            from tests.conftest import assert_detections_match
            assert_detections_match(tuple(o["result"][k].numpy() for k in ("labels_3d", "boxes_3d", "scores_3d")),
                                    tuple(r["result"][k].numpy() for k in ("labels_3d", "boxes_3d", "scores_3d")), "frame %d" % fi)
            assert torch.equal(r["roi"]["valid_indices"], o["roi"]["valid_indices"])
            print("[golden-md] frame %d: M=%d primaries, V=%d valid, M'=%d, A=%d, %d boxes, worst deviation so far %.2e" %
                  (fi, M, V, Mx, r["outs"]["all_cls_scores"].shape[2], r["result"]["boxes_3d"].shape[0], worst))
            gold["f%d_all_cls_scores" % fi] = r["outs"]["all_cls_scores"].numpy()
            gold["f%d_all_bbox_preds" % fi] = r["outs"]["all_bbox_preds"].numpy()
            gold["f%d_boxes_3d" % fi] = r["result"]["boxes_3d"].numpy()
            gold["f%d_scores_3d" % fi] = r["result"]["scores_3d"].numpy()
            gold["f%d_labels_3d" % fi] = r["result"]["labels_3d"].numpy()
            gold["f%d_bbox2d" % fi] = torch.cat(r["roi"]["bbox_list"]).numpy()
            gold["f%d_bbox2d_scores" % fi] = r["roi"]["bbox2d_scores"].numpy()
            gold["f%d_valid_idx" % fi] = r["roi"]["valid_indices"].nonzero().numpy().astype(np.int32)
            gold["f%d_cell_probs" % fi] = seen["probs"].numpy()
            gold["f%d_M" % fi] = np.int32(M)
            gold["f%d_V" % fi] = np.int32(V)
            gold["f%d_md_valid" % fi] = seen["valid"].numpy()
            gold["f%d_ref2d" % fi] = seen["ref2d"][0].numpy()
    gold["recipe"] = np.frombuffer(json.dumps(c).encode(), dtype=np.uint8)
    path = os.path.join(GOLD, c["name"] + ".npz")
    np.savez_compressed(path, **gold)
    print("[golden-md] wrote %s (%d bytes; worst restatement-vs-reference deviation %.2e)" % (path, os.path.getsize(path), worst))


def main():
    only = set(sys.argv[1:])
    for c in (MD2, MD3):
        if not only or c["name"] in only:
            generate(c)


if __name__ == "__main__":
    if not refload.available():
        sys.exit("reference checkout not found: fixtures can only be regenerated in the build container")
    main()

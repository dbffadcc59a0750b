"""Golden fixtures of the VoVNet family (the depthwise and slim specs; BUILD CONTAINER ONLY: needs the reference checkout).

  python tools/gen_golden_vov.py [manifest] [maps] [seq]     # all three, or the named ones

Writes, from the reference's own modules loaded where they lie (oracle/refload.py), data only:

  tests/golden/vov_family_manifest.json  for the seven `spec_name`s of the reference registry (models/backbones/vovnet.py:89-97): the
      parameter names (in state-dict order, prefixed `img_backbone.`) and shapes of VoVNet(spec_name).state_dict() without
      num_batches_tracked.
  tests/golden/vov_family_maps.npz       for the three specs the build gained: a 2x3x64x96 input drawn from a recorded seed, weights from
      weights.init_state_dict(backbone_spec(name), seed), the reference module's four stage maps in fp32 and, per map, the relative
      deviation (max |fp32 - float64| / max |float64|) between the reference run in fp32 and the same module run in float64.  Nothing is
      written unless every deviation is below DEV_BAR = 2.5e-5 (a quarter of the tests' 1e-4 bar); a seed that fails is replaced by
      the next seed, never by another bar.  To keep the file small the two large maps are stored at every second row and column (every channel;
      first / last rows and columns included; `<spec>_s<k>_rows` / `_cols`), the two small ones in full; the map maximum the tests'
      bound refers to and the deviations are taken over the FULL maps.
  tests/golden/far3d_dw_seq.npz          gen_golden.py's far3d_small_seq recipe with backbone = V-19-slim-dw-eSE: 2 frames of one scene,
      the reference detector's own outputs in the layout of the other sequences.  The data seed is the first whose discrete decisions
      (3x3 peaks, score threshold, depth argmax at the proposals, memory top-k) all clear their bars (MARGINS); margins and bars go into the recipe.
      (oracle/far3d_oracle.py restates the plain specs only, so there is no oracle-vs-reference figure in this fixture.)
"""
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from far3d_amd import synth, weights  # noqa: E402
from oracle import refload  # noqa: E402
from gen_golden import GOLD, SMALL, run_reference  # noqa: E402

REGISTRY = ("V-19-slim-dw-eSE", "V-19-dw-eSE", "V-19-slim-eSE", "V-19-eSE", "V-39-eSE", "V-57-eSE", "V-99-eSE")
NEW = ("V-19-slim-dw-eSE", "V-19-dw-eSE", "V-19-slim-eSE")
STAGES = ("stage2", "stage3", "stage4", "stage5")
DEV_BAR = 2.5e-5
# Bars of the discrete decisions (_margins).  The 2D head's scores are products of two sigmoids (<= 1) computed from maps that two fp32
# implementations reproduce to ~1e-6 of their maximum (the fp32-vs-float64 figures of the maps fixture above): 5e-5 in score units is 50x
# that -- with ~250 cells per camera and eight neighbours each, gaps of 5e-4 between adjacent scores do not occur on any seed.  The depth
# argmax and the memory top-k read logits: 1e-3 in logit units, the bound the tests hold the fp32 engine's logits to (memory scores are
# sigmoids, slope <= 1/4: 2.5e-4 in score units).
MARGIN = 5e-5
MARGINS = dict(peak=MARGIN, threshold=MARGIN, depth_argmax=1e-3, memory_topk=2.5e-4)
DW_SEQ = dict(SMALL, name="far3d_dw_seq", backbone="V-19-slim-dw-eSE", frames=2, scene_change_at=None, weight_seed=1)


def _ref_backbone(name):
    m = refload.ref("models.backbones.vovnet").VoVNet(name, out_features=list(STAGES))
    m.eval()
    return m


def gen_manifest():
    out = {}
    for name in REGISTRY:
        sd = _ref_backbone(name).state_dict()
        rows = [["img_backbone." + k, list(v.shape)] for k, v in sd.items() if not k.endswith("num_batches_tracked")]
        spec = weights.backbone_spec(name)
        assert [r[0] for r in rows] == list(spec), "%s: key names / order differ from weights.backbone_spec" % name
        assert all(tuple(s) == tuple(spec[k]) for k, s in rows), "%s: shapes differ" % name
        out[name] = rows
        print("[golden-vov] %s: %d tensors, %.2f M parameters" % (name, len(rows), sum(int(np.prod(s)) for _, s in rows) / 1e6))
    path = os.path.join(GOLD, "vov_family_manifest.json")
    json.dump(out, open(path, "w"), indent=0, sort_keys=True)
    print("[golden-vov] wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def sample_grid(H, W):
    """Rows / columns a stage map is stored at: everything for the small maps; every second row and column plus the last ones for the
    two large maps (both borders, even and odd positions of a pixel run's tail)."""
    if H * W <= 24:
        return list(range(H)), list(range(W))
    return sorted(set(range(0, H, 2)) | {H - 1}), sorted(set(range(0, W, 2)) | {W - 1})


def gen_maps():
    gold = {}
    for name in NEW:
        spec = weights.backbone_spec(name)
        seed = 0
        while True:
            sd = weights.init_state_dict(spec, seed=seed)
            x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(1000 + seed))
            m = _ref_backbone(name)
            missing, unexpected = m.load_state_dict({k[len("img_backbone."):]: v for k, v in sd.items()}, strict=False)
            assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
            with torch.no_grad():
                y32 = m(x)
                y64 = copy.deepcopy(m).double()(x.double())
            devs = [float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(y32, y64)]
            if max(devs) < DEV_BAR:
                break
            print("[golden-vov] %s seed %d: fp32-vs-float64 deviation %.2e >= %.1e, next seed" % (name, seed, max(devs), DEV_BAR))
            seed += 1
            assert seed < 20, "no seed below the bar"
        gold[name + "_seed"] = np.int32(seed)
        gold[name + "_input_seed"] = np.int32(1000 + seed)
        for k, (a, d) in enumerate(zip(y32, devs)):
            assert a.shape[2:] == ((16, 24), (8, 12), (4, 6), (2, 3))[k], a.shape
            rows, cols = sample_grid(a.shape[2], a.shape[3])
            p = "%s_s%d" % (name, k + 2)
            gold[p] = a[:, :, rows][:, :, :, cols].contiguous().numpy()
            gold[p + "_rows"], gold[p + "_cols"] = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
            gold[p + "_max"] = np.float32(a.abs().max())
            gold[p + "_f64_dev"] = np.float32(d)
        print("[golden-vov] %s: seed %d, fp32-vs-float64 deviations %s" % (name, seed, ", ".join("%.2e" % d for d in devs)))
    path = os.path.join(GOLD, "vov_family_maps.npz")
    np.savez_compressed(path, **gold)
    print("[golden-vov] wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def _margins(r, c, topk_proposals):
    """How far the frame's discrete decisions are from a tie, from the reference's own outputs: the selection rule of
    yolox_head.py:426-438 (score = sigmoid(objectness) * sigmoid(best class), a cell is kept when it equals its 3x3 maximum and
    exceeds the threshold), the depth argmax at the proposals' cells (farhead.py:733-747) and the memory top-k (farhead.py:490-494)."""
    roi = r["roi"]
    thr = 0.1
    peak, thresh = np.inf, np.inf
    for cls, obj in zip(roi["enc_cls_scores"], roi["objectnesses"]):
        sw = obj.sigmoid() * cls.max(dim=1, keepdim=True).values.sigmoid()                    # (BN,1,h,w)
        win = F.unfold(F.pad(sw, (1, 1, 1, 1), value=-1.0), 3)                                # (BN,9,h*w), the cell itself is row 4
        own = win[:, 4]
        others = torch.cat([win[:, :4], win[:, 5:]], dim=1).max(dim=1).values
        live = torch.maximum(own, others) > thr - MARGIN                                      # cells whose peak test could decide a proposal
        if bool(live.any()):
            peak = min(peak, float((own - others).abs()[live].min()))
        is_peak = own >= others
        if bool(is_peak.any()):
            thresh = min(thresh, float((own[is_peak] - thr).abs().min()))
    dl = roi["depth_logit"]
    assert dl.dim() == 4 and dl.shape[1] == 51, dl.shape
    ds = c["pad_hw"][0] // dl.shape[2]
    depth = np.inf
    for n, b in enumerate(roi["bbox_list"]):
        if len(b):
            u = (b[:, 0] / ds).round().long().clamp(0, dl.shape[3] - 1)
            v = (b[:, 1] / ds).round().long().clamp(0, dl.shape[2] - 1)
            t2 = dl[n][:, v, u].topk(2, dim=0).values
            depth = min(depth, float((t2[0] - t2[1]).min()))
    s = r["outs"]["all_cls_scores"][-1].sigmoid().max(-1).values.flatten().sort(descending=True).values
    mem = float(s[topk_proposals - 1] - s[topk_proposals])
    return dict(peak=peak, threshold=thresh, depth_argmax=depth, memory_topk=mem)


def _build_model(c, sd):
    cfg, _ = refload.reference_model_cfg(num_cams=c["num_cams"], num_query=c["num_query"], num_propagated=c["num_propagated"],
                                         memory_len=c["memory_len"], topk_proposals=c["topk_proposals"])
    cfg["img_backbone"]["spec_name"] = c["backbone"]
    cfg["img_neck"]["in_channels"] = list(weights.VOV_SPECS[c["backbone"]]["stage_out_ch"])
    model = refload.build_reference_detector(cfg)
    canon = {weights.canonical_key(k): tuple(v.shape) for k, v in model.state_dict().items() if weights.canonical_key(k) is not None}
    spec = weights.detector_spec(c["backbone"], num_query=c["num_query"], num_propagated=c["num_propagated"])
    assert canon == {k: tuple(v) for k, v in spec.items()}, "detector schema differs from the reference"
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(weights.canonical_key(m) is None or weights.canonical_key(m) != m for m in missing), missing
    return model


def _run_seq(model, c):
    model.prev_scene_token = None           # a new sequence: the first frame resets the streaming memory
    frames, margins = [], []
    with torch.no_grad():
        for fi in range(c["frames"]):
            data, metas = synth.recipe_frame(c, fi)
            metas[0]["box_type_3d"] = refload.LiDARBoxes
            r = run_reference(model, copy.deepcopy(data), metas)
            frames.append(r)
            margins.append(_margins(r, c, c["topk_proposals"]))
    return frames, margins


def gen_seq():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    c = dict(DW_SEQ)
    spec = weights.detector_spec(c["backbone"], num_query=c["num_query"], num_propagated=c["num_propagated"])
    sd = weights.init_state_dict(spec, seed=c["weight_seed"])
    model = _build_model(c, sd)
    for seed in range(SMALL["data_seed"], SMALL["data_seed"] + 40):
        c["data_seed"] = seed
        frames, margins = _run_seq(model, c)
        worst = {k: min(m[k] for m in margins) for k in margins[0]}
        M = [int(r["roi"]["bbox2d_scores"].shape[0]) for r in frames]
        ok = all(worst[k] > MARGINS[k] for k in worst) and all(m > 0 for m in M)
        print("[golden-vov] data seed %d: M=%s margins %s -> %s" % (seed, M, {k: "%.2e" % v for k, v in worst.items()}, "ok" if ok else "next"))
        if ok:
            break
    else:
        raise SystemExit("no data seed clears the margins")
    c["margins"] = {k: float("%.4g" % v) for k, v in worst.items()}
    c["margin_bars"] = dict(MARGINS)
    gold = {}
    for fi, r in enumerate(frames):
        gold["f%d_all_cls_scores" % fi] = r["outs"]["all_cls_scores"].numpy()
        gold["f%d_all_bbox_preds" % fi] = r["outs"]["all_bbox_preds"].numpy()
        gold["f%d_boxes_3d" % fi] = r["result"]["boxes_3d"].numpy()
        gold["f%d_scores_3d" % fi] = r["result"]["scores_3d"].numpy()
        gold["f%d_labels_3d" % fi] = r["result"]["labels_3d"].numpy()
        gold["f%d_bbox2d" % fi] = torch.cat(r["roi"]["bbox_list"]).numpy()
        gold["f%d_bbox2d_scores" % fi] = r["roi"]["bbox2d_scores"].numpy()
        gold["f%d_valid_idx" % fi] = r["roi"]["valid_indices"].nonzero().numpy().astype(np.int32)
        gold["f%d_depth_argmax" % fi] = r["roi"]["pred_depth"].argmax(1).numpy().astype(np.int16)
        for l in range(4):
            gold["f%d_fpn%d_sample" % (fi, l)] = r["img_feats"][l][:, ::16, ::2, ::3].numpy()
    gold["recipe"] = np.frombuffer(json.dumps(c).encode(), dtype=np.uint8)
    path = os.path.join(GOLD, c["name"] + ".npz")
    np.savez_compressed(path, **gold)
    print("[golden-vov] wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    if not refload.available():
        sys.exit("reference checkout not found: fixtures can only be regenerated in the build container")
    only = set(sys.argv[1:])
    for key, fn in (("manifest", gen_manifest), ("maps", gen_maps), ("seq", gen_seq)):
        if not only or key in only:
            fn()

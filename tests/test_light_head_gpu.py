"""GPU: the light 2D head -- depthwise-separable YOLOX towers (use_depthwise=True, ref models/dense_heads/yolox_head.py:197-219) and the
depth branch on a coarser level (reg_depth_level p4, :300-301) -- through engine.roi_head, the detector and a captured graph.

roi_head: against a plain-torch float64 restatement built here from the same state dict, at the toy size of tests/test_vov_family_gpu.py
(2 images of 64x96: FPN maps 8x12 ... 1x2).  Bars: the ones the project holds such maps to -- fp32 within 1e-4 of each output's maximum,
bf16 within 2e-2, bf16x3 closer than bf16 on every output.  Detector: tests/golden/far3d_light_head_seq.npz (tools/gen_golden_light_head.py,
the reference's own outputs) with the bounds of test_vov_family_gpu.py::test_dw_detector_fp32_matches_reference_legacy_mode."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from far3d_amd import config, plugin, synth, weights
from tests.conftest import ROOT, assert_detections_match

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden")
R = "img_roi_head."
HW = ((8, 12), (4, 6), (2, 3), (1, 2))
CASES = [(True, 0), (True, 1), (False, 1)]          # (roi_depthwise, depth_level)


@functools.lru_cache(maxsize=None)
def _roi_case(dw):
    """(2D-head state dict, the four FPN maps (2,256,h,w) fp32) -- built once, never modified."""
    spec = {k: v for k, v in weights.detector_spec(roi_depthwise=dw).items() if k.startswith(R)}
    sd = weights.init_state_dict(spec, seed=11)
    g = torch.Generator().manual_seed(23)
    return sd, tuple(torch.randn(2, 256, h, w, generator=g) for h, w in HW)


def _conv_bn_swish(x, sd, p, groups=1, pad=0):
    """mmcv ConvModule: conv (no bias) -> BN (eval, eps 1e-3) -> Swish, in x's dtype."""
    d = lambda k: sd[p + k].to(x.dtype)
    x = F.conv2d(x, d("conv.weight"), None, 1, pad, 1, groups)
    x = F.batch_norm(x, d("bn.running_mean"), d("bn.running_var"), d("bn.weight"), d("bn.bias"), False, 0.0, 1e-3)
    return x * torch.sigmoid(x)


@functools.lru_cache(maxsize=None)
def _restatement(dw, level):
    """float64 outputs in the engine's layout: cls[l] (N,h,w,26), reg[l] (N,h,w,5: box, objectness), depth_logit (N,h,w,51)."""
    sd, maps = _roi_case(dw)
    d = lambda k: sd[R + k].double()
    cls, reg = [], []
    for l, x in enumerate(maps):
        x = x.double()
        feats = {}
        for t in ("cls", "reg"):
            f = x
            for i in range(2):
                p = R + "multi_level_%s_convs.%d.%d." % (t, l, i)
                if dw:
                    f = _conv_bn_swish(f, sd, p + "depthwise_conv.", groups=f.shape[1], pad=1)
                    f = _conv_bn_swish(f, sd, p + "pointwise_conv.")
                else:
                    f = _conv_bn_swish(f, sd, p, pad=1)
            feats[t] = f
        cls.append(F.conv2d(feats["cls"], d("multi_level_conv_cls.%d.weight" % l), d("multi_level_conv_cls.%d.bias" % l)).permute(0, 2, 3, 1))
        box = F.conv2d(feats["reg"], d("multi_level_conv_reg.%d.weight" % l), d("multi_level_conv_reg.%d.bias" % l))
        obj = F.conv2d(feats["reg"], d("multi_level_conv_obj.%d.weight" % l), d("multi_level_conv_obj.%d.bias" % l))
        reg.append(torch.cat([box, obj], 1).permute(0, 2, 3, 1))
    y = maps[level].double()
    for i in range(2):                                # DepthPredictor's head: conv3x3 + GroupNorm(32) + ReLU, twice, then the 1x1 classifier
        y = F.conv2d(y, d("depthnet.depth_head.%d.0.weight" % i), d("depthnet.depth_head.%d.0.bias" % i), 1, 1)
        y = F.relu(F.group_norm(y, 32, d("depthnet.depth_head.%d.1.weight" % i), d("depthnet.depth_head.%d.1.bias" % i), 1e-5))
    y = F.conv2d(y, d("depthnet.depth_classifier.weight"), d("depthnet.depth_classifier.bias"))
    return cls, reg, y.permute(0, 2, 3, 1)


def _engine(dw, level, precision, drop_keys=False):
    from far3d_amd import engine
    sd, _ = _roi_case(dw)
    cfg = engine.default_cfg(roi_depthwise=dw, depth_level=level)
    if drop_keys:                                     # a cfg written before the options existed
        del cfg["roi_depthwise"], cfg["depth_level"]
    return engine.Far3DEngine(sd, cfg, device=DEV, precision=precision, parts=("roi",))


def _run(eng, dw):
    _, maps = _roi_case(dw)
    out = eng.roi_head([eng.act_from_nchw(m.to(DEV)) for m in maps])
    torch.cuda.synchronize()
    return out


def _errors(got, want, tag):
    """max |got - want| / max |want| per output, in the order cls0..3, reg0..3, depth."""
    gs, ws = list(got[0]) + list(got[1]) + [got[2]], list(want[0]) + list(want[1]) + [want[2]]
    errs = []
    for g, w in zip(gs, ws):
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(w.shape), (tag, g.shape, w.shape)
        errs.append(float((g.cpu().double() - w).abs().max() / w.abs().max()))
    print("%s: errors / max %s" % (tag, ", ".join("%.2e" % e for e in errs)))
    return errs


@pytest.mark.parametrize("dw,level", CASES)
def test_roi_head_fp32_and_bf16_match_restatement(hip_lib, dw, level):
    want = _restatement(dw, level)
    assert tuple(want[2].shape) == (2,) + HW[level] + (51,)
    eng = _engine(dw, level, "fp32")
    assert all(e < 1e-4 for e in _errors(_run(eng, dw), want, "dw=%s level %d fp32" % (dw, level)))
    assert eng.depth_stride == (8, 16, 32, 64)[level]
    if dw:                                            # the pointwise convs are addressable by name (per-layer precision machinery)
        assert {"roi0.cls0.pw", "roi0.reg0.pw", "roi3.cls1.pw", "roi3.reg1.pw"} <= set(eng.convs) and "roi0.tower0" not in eng.convs
    assert all(e < 2e-2 for e in _errors(_run(_engine(dw, level, "bf16"), dw), want, "dw=%s level %d bf16" % (dw, level)))


@pytest.mark.parametrize("dw,level", CASES)
def test_roi_head_pair_closer_than_bf16(hip_lib, dw, level):
    want = _restatement(dw, level)
    e16 = _errors(_run(_engine(dw, level, "bf16"), dw), want, "dw=%s level %d bf16" % (dw, level))
    e3 = _errors(_run(_engine(dw, level, "bf16x3"), dw), want, "dw=%s level %d bf16x3" % (dw, level))
    assert all(a < b for a, b in zip(e3, e16)), (e3, e16)
    for precision in ("bf16x3_all", "bf16x3_2d1"):
        assert all(e < 2e-2 for e in _errors(_run(_engine(dw, level, precision), dw), want, "dw=%s level %d %s" % (dw, level, precision)))


@pytest.mark.parametrize("dw", [True])
def test_two_set_launch_and_two_single_launches_agree_bitwise(hip_lib, dw):
    """The engine's switch between one two-set depthwise launch and two single-set launches changes no bit."""
    for precision in ("fp32", "bf16", "bf16x3"):
        eng = _engine(dw, 1, precision)
        a = _run(eng, dw)
        eng.roi_dw_merged = not eng.roi_dw_merged
        b = _run(eng, dw)
        for x, y in zip(list(a[0]) + list(a[1]) + [a[2]], list(b[0]) + list(b[1]) + [b[2]]):
            assert torch.equal(x, y), precision


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "fp32"])
def test_default_engine_packs_and_computes_as_before(hip_lib, precision):
    """Default options: the same `roi` entries under the same names, the same path through roi_head (the two grouped launches in the
    pair-stored modes) and bit-identical outputs against an engine whose cfg does not carry the new keys."""
    new, old = _engine(False, 0, precision), _engine(False, 0, precision, drop_keys=True)
    names = set("roi%d.%s" % (l, n) for l in range(4) for n in ("tower0", "cls1", "reg1", "cls_head", "reg_head")) | {"depth.c0", "depth.c1", "depth.cls"}
    assert set(new.convs) == set(old.convs) == names
    assert all(set(a) == set(b) == {"cls", "reg", "tower0", "cls_head", "reg_head", "ctr_head"} for a, b in zip(new.roi, old.roi))
    assert not new.roi_dw and new.depth_level == 0 and new.depth_stride == 8
    calls = {}
    for tag, eng in (("new", new), ("old", old)):
        calls[tag] = []
        grouped = eng._roi_head_grouped

        def spy(raw, gt0, gt1, _g=grouped, _t=tag):
            calls[_t].append((gt0, gt1))
            return _g(raw, gt0, gt1)
        eng._roi_head_grouped = spy
    a, b = _run(new, False), _run(old, False)
    assert calls["new"] == calls["old"]
    for x, y in zip(list(a[0]) + list(a[1]) + [a[2]], list(b[0]) + list(b[1]) + [b[2]]):
        assert torch.equal(x, y)
    assert all(e < (1e-4 if precision == "fp32" else 2e-2) for e in _errors(a, _restatement(False, 0), "default %s" % precision))


# ------------------------------------------------------------------------------------------ detector level
def _light_detector(**over):
    z = np.load(os.path.join(GOLD, "far3d_light_head_seq.npz"))
    rc = json.loads(bytes(z["recipe"]).decode())
    assert rc["backbone"] == "V-19-slim-dw-eSE" and rc["use_depthwise"] is True and rc["reg_depth_level"] == "p4"
    assert all(rc["margins"][k] > rc["margin_bars"][k] for k in rc["margin_bars"])       # the generator's condition on the inputs
    det = plugin.build_detector(config.default_model_cfg(backbone=rc["backbone"], num_cams=rc["num_cams"], num_query=rc["num_query"],
                                                         num_propagated=rc["num_propagated"], memory_len=rc["memory_len"],
                                                         topk_proposals=rc["topk_proposals"], use_depthwise=True,
                                                         reg_depth_level=rc["reg_depth_level"], **over))
    spec = weights.detector_spec(rc["backbone"], num_query=rc["num_query"], num_propagated=rc["num_propagated"], roi_depthwise=True, depth_level=1)
    det.load_state_dict(weights.init_state_dict(spec, seed=rc["weight_seed"]))
    det.prepare(DEV, precision="fp32")
    assert det.engine.roi_dw and det.engine.depth_stride == 16
    return det, z, rc


def test_light_detector_fp32_matches_reference(hip_lib):
    det, z, rc = _light_detector()
    for fi in range(rc["frames"]):
        data, metas = synth.recipe_frame(rc, fi)
        res = det(return_loss=False, rescale=True, img_metas=metas, **data)[0]["pts_bbox"]
        o = det.last_outs
        want_idx = z["f%d_valid_idx" % fi]
        cnt = o["sel_cnt"].cpu().numpy()
        got = [(n, int(i)) for n in range(rc["num_cams"]) for i in o["sel_idx"][n, :cnt[n]].cpu().numpy()]
        assert got == [(int(r[0]), int(r[1])) for r in want_idx], "frame %d: proposal set differs" % fi
        assert tuple(o["depth_logit"].shape[1:3]) == (rc["pad_hw"][0] // 16, rc["pad_hw"][1] // 16)
        assert np.allclose(o["bbox2d"].cpu().numpy(), z["f%d_bbox2d" % fi], rtol=2e-3, atol=2e-3)
        for key in ("all_cls_scores", "all_bbox_preds"):
            g, want = o[key].cpu().numpy(), z["f%d_%s" % (fi, key)]
            assert g.shape == want.shape, (fi, key, g.shape, want.shape)
            err = np.abs(g - want)
            print("far3d_light_head_seq frame %d %s: max abs err %.3e" % (fi, key, err.max()))
            if key == "all_cls_scores":
                assert err.max() < 1e-3, "frame %d logits: max abs err %.3e" % (fi, err.max())
            else:                                                            # the bounds of tests/test_multidepth_gpu.py::_check_frame
                assert err[..., :3].max() < 0.076 and err[..., 3:].max() < 1e-3, "frame %d boxes" % fi
        assert_detections_match(tuple(res[k].cpu().numpy() for k in ("labels_3d", "boxes_3d", "scores_3d")),
                                tuple(z["f%d_%s" % (fi, k)] for k in ("labels_3d", "boxes_3d", "scores_3d")), "frame %d" % fi)


def test_light_detector_graph_bitwise_eager(hip_lib):
    res = {}
    for mode in ("eager", "graph"):
        det, z, rc = _light_detector(proposal_capacity=48)
        det.engine.use_graph = mode == "graph"
        out = []
        for fi in list(range(rc["frames"])) + [rc["frames"] - 1] * 2:       # frame 0 starts the scene eagerly; then capture and replays
            data, metas = synth.recipe_frame(rc, fi)
            det(return_loss=False, rescale=True, img_metas=metas, **data)
            o = det.last_outs
            out.append((int(o["num_adaptive_dev"].item()), o["all_cls_scores"].clone(), o["all_bbox_preds"].clone(),
                        {k: v.clone() for k, v in det.engine.mem.items()}))
        res[mode] = out
        if mode == "graph":
            assert det.engine._graph is not None, "the steady-state frame was not captured"
    for fi, (a, b) in enumerate(zip(res["eager"], res["graph"])):
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "frame %d: graph differs from eager" % fi
        for k in a[3]:
            assert torch.equal(a[3][k], b[3][k]), "frame %d: streaming memory '%s' differs" % (fi, k)
    M = [int(np.load(os.path.join(GOLD, "far3d_light_head_seq.npz"))["f%d_bbox2d" % fi].shape[0]) for fi in range(2)]
    assert [r[0] for r in res["eager"][:2]] == M                            # the fixed-capacity run counts the reference's proposals

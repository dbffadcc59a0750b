"""CPU: the light 2D head's host side -- the depthwise-separable tower keys (mmcv 1.6.2 DepthwiseSeparableConvModule as the reference's
YOLOXHeadCustom builds it with use_depthwise=True, models/dense_heads/yolox_head.py:197-219), the depth branch's level
(reg_depth_level p3 | p4 | p5, :300-301), the config plumbing and the options that are refused by name."""

import pytest
import torch

from far3d_amd import config, plugin, weights

R = "img_roi_head."
BN = ("weight", "bias", "running_mean", "running_var")


def _roi(**over):
    cfg = dict(type="YOLOXHeadCustom", num_classes=26, in_channels=256, strides=[8, 16, 32, 64], pred_with_depth=True,
               depthnet_config=dict(type=0, hidden_dim=256, num_depth_bins=50, depth_min=0.1, depth_max=110, stride=8),
               reg_depth_level="p3", sample_with_score=True, threshold_score=0.1, topk_proposal=None, return_context_feat=True)
    cfg.update(over)
    return cfg


def test_depthwise_schema_keys_and_shapes():
    dense = weights.detector_spec(num_query=60, num_propagated=16)
    light = weights.detector_spec(num_query=60, num_propagated=16, roi_depthwise=True, depth_level=1)
    assert weights.detector_spec(num_query=60, num_propagated=16, roi_depthwise=False, depth_level=0) == dense
    assert list(weights.detector_spec(num_query=60, num_propagated=16, depth_level=2)) == list(dense)      # the level changes no key
    want = {}
    for l in range(4):
        for t in ("cls", "reg"):
            for i in range(2):
                p = R + "multi_level_%s_convs.%d.%d." % (t, l, i)
                want[p + "depthwise_conv.conv.weight"] = (256, 1, 3, 3)
                want[p + "pointwise_conv.conv.weight"] = (256, 256, 1, 1)
                for half in ("depthwise_conv", "pointwise_conv"):
                    for k in BN:
                        want[p + half + ".bn." + k] = (256,)
    tower = {k: tuple(v) for k, v in light.items() if "_convs." in k and k.startswith(R)}
    assert tower == want
    assert not any(k.endswith("conv.bias") for k in tower)                    # no conv biases: BN follows both halves
    rest = lambda spec: {k: tuple(v) for k, v in spec.items() if not ("_convs." in k and k.startswith(R))}
    assert rest(light) == rest(dense)
    # module order of one layer: depthwise conv, its bn, pointwise conv, its bn
    p = R + "multi_level_cls_convs.0.0."
    ks = [k[len(p):] for k in light if k.startswith(p)]
    assert ks == ["depthwise_conv.conv.weight"] + ["depthwise_conv.bn." + k for k in BN] + \
                 ["pointwise_conv.conv.weight"] + ["pointwise_conv.bn." + k for k in BN]
    with pytest.raises(ValueError):
        weights.detector_spec(depth_level=4)
    with pytest.raises(ValueError):
        weights.detector_spec(fpn_levels=3, depth_level=3)


def test_strict_load_round_trip(tmp_path):
    spec = weights.detector_spec("V-19-slim-dw-eSE", num_query=60, num_propagated=16, roi_depthwise=True, depth_level=1)
    sd = weights.init_state_dict(spec, seed=4)
    assert list(sd) == list(spec) and all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    p = R + "multi_level_reg_convs.2.1.depthwise_conv."
    assert float(sd[p + "bn.running_var"].min()) >= 0.75 and float(sd[p + "conv.weight"].std()) > 0.1
    ckpt = dict(sd)
    for half in ("depthwise_conv", "pointwise_conv"):                         # a real checkpoint carries BN bookkeeping
        ckpt[R + "multi_level_cls_convs.0.0.%s.bn.num_batches_tracked" % half] = torch.tensor(3)
    path = tmp_path / "light.pth"
    torch.save(dict(meta=dict(), state_dict={"module." + k: v for k, v in ckpt.items()}), str(path))
    got = weights.load_checkpoint(str(path), strict_schema=spec)
    assert list(got) == list(spec) and all(torch.equal(got[k], sd[k]) for k in spec)
    # a depthwise checkpoint against the dense schema (and the reverse) is refused with the offending names
    dense = weights.detector_spec("V-19-slim-dw-eSE", num_query=60, num_propagated=16)
    with pytest.raises(KeyError) as e:
        weights.load_checkpoint(str(path), strict_schema=dense)
    assert "multi_level_cls_convs.0.0.conv.weight" in str(e.value)
    with pytest.raises(KeyError):
        weights.normalize_state_dict(weights.init_state_dict(dense, seed=4), strict_schema=spec)
    # the detector module holds exactly these keys
    det = plugin.build_detector(config.default_model_cfg(backbone="V-19-slim-dw-eSE", num_query=60, num_propagated=16,
                                                         use_depthwise=True, reg_depth_level="p4"))
    missing, unexpected = det.load_state_dict(got, strict=True)
    assert not missing and not unexpected
    assert {k: tuple(v.shape) for k, v in det.state_dict().items() if weights.canonical_key(k)} == {k: tuple(v) for k, v in spec.items()}
    assert torch.equal(det.state_dict()[p + "conv.weight"], sd[p + "conv.weight"])


def test_default_model_cfg_carries_the_options():
    base = config.default_model_cfg()
    assert base["img_roi_head"]["reg_depth_level"] == "p3" and base["img_roi_head"]["use_depthwise"] is False
    cfg = config.default_model_cfg(use_depthwise=True, reg_depth_level="p4")
    assert cfg["img_roi_head"]["use_depthwise"] is True and cfg["img_roi_head"]["reg_depth_level"] == "p4"
    det = plugin.build_detector(cfg)
    ec = det.engine_cfg()
    assert ec["roi_depthwise"] is True and ec["depth_level"] == 1
    assert det.img_roi_head.use_depthwise and det.img_roi_head.depth_level == 1
    ours = plugin.build_detector(base).engine_cfg()
    assert ours["roi_depthwise"] is False and ours["depth_level"] == 0
    from far3d_amd import engine
    d = engine.default_cfg()
    assert d["roi_depthwise"] is False and d["depth_level"] == 0
    assert {k: v for k, v in ec.items() if k not in ("roi_depthwise", "depth_level")} == \
           {k: v for k, v in ours.items() if k not in ("roi_depthwise", "depth_level")}


@pytest.mark.parametrize("over,name", [
    (dict(embedding_cam=True), "embedding_cam"),
    (dict(pred_depth_var=True), "pred_depth_var"),
    (dict(dcn_on_last_conv=True), "dcn_on_last_conv"),
    (dict(depthnet_config=dict(type=0, num_depth_bins=50, multi_level_pred=True)), "multi_level_pred"),
    (dict(depthnet_config=dict(type=0, num_depth_bins=50, multi_level_fusion=True)), "multi_level_fusion"),
    (dict(depthnet_config=dict(type=1, num_depth_bins=50)), "depthnet_config.type"),
    (dict(depthnet_config=dict(type=0, num_depth_bins=50, conv_layer_num=3)), "conv_layer_num"),
])
def test_unbuilt_options_raise_by_name(over, name):
    with pytest.raises(NotImplementedError) as e:
        plugin.HEADS.build(_roi(**over))
    assert name in str(e.value)


def test_switched_off_options_are_accepted():
    m = plugin.HEADS.build(_roi(embedding_cam=False, pred_depth_var=False, dcn_on_last_conv=False, use_depthwise=False,
                                depthnet_config=dict(type=0, num_depth_bins=50, multi_level_pred=False, multi_level_fusion=False,
                                                     conv_layer_num=2)))
    assert not m.use_depthwise and m.depth_level == 0


def test_depth_level_must_exist_in_strides():
    m = plugin.HEADS.build(_roi(strides=[8, 16, 32], reg_depth_level="p5"))
    assert m.depth_level == 2 and m.reg_depth_level == "p5"
    assert plugin.HEADS.build(_roi(strides=[8, 16, 32], reg_depth_level="p4", use_depthwise=True)).depth_level == 1
    # the class's own default is p4 (yolox_head.py:97)
    cfg = _roi()
    del cfg["reg_depth_level"]
    assert plugin.HEADS.build(cfg).depth_level == 1
    with pytest.raises(ValueError) as e:
        plugin.HEADS.build(_roi(strides=[8, 16], reg_depth_level="p5"))
    assert "p5" in str(e.value)
    with pytest.raises(ValueError):
        plugin.HEADS.build(_roi(reg_depth_level="p6"))

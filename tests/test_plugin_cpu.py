"""CPU: registry surface -- the reference config builds our detector unchanged; state-dict keys are the reference's."""
import json
import os

import pytest
import torch

from far3d_amd import config, plugin, weights
from tests.conftest import ROOT

# the reference's config file (projects/configs/far3d.py) as data: its `model` / `point_cloud_range` entries (tools/gen_golden_config.py)
REF_CFG = os.path.join(ROOT, "tests", "golden", "reference_config.json")


def test_default_cfg_builds_and_matches_reference_manifest():
    det = plugin.build_detector(config.default_model_cfg())
    keys = {k: list(v.shape) for k, v in det.state_dict().items() if weights.canonical_key(k)}
    man = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_manifest.json")))
    assert keys == man
    assert det.pts_bbox_head.transformer.decoder.layers[0].ffn_dim == 1024      # SURVEY finding 4 (2048 is swallowed)
    cfg = det.engine_cfg()
    assert cfg["num_cams"] == 7 and cfg["num_query"] == 644 and cfg["num_propagated"] == 256 and cfg["max_num"] == 300


def test_reference_config_file_loads_unchanged(tmp_path):
    # written back as a python config file and loaded through the same loader as the original
    p = tmp_path / "far3d.py"
    p.write_text("".join("%s = %r\n" % kv for kv in sorted(json.load(open(REF_CFG)).items())))
    cfg = config.load_config(str(p))
    assert cfg.model.type == "Far3D" and cfg.point_cloud_range[3] == 152.4
    det = plugin.build_detector(cfg.model)
    ours = plugin.build_detector(config.default_model_cfg())
    assert {k: tuple(v.shape) for k, v in det.state_dict().items()} == {k: tuple(v.shape) for k, v in ours.state_dict().items()}
    assert det.engine_cfg() == ours.engine_cfg()


def test_checkpoint_style_keys_load():
    det = plugin.build_detector(config.default_model_cfg(num_query=60, num_propagated=16))
    spec = weights.detector_spec(num_query=60, num_propagated=16)
    sd = weights.init_state_dict(spec, seed=3)
    ckpt = dict(sd)
    for i in range(1, 6):   # a real checkpoint repeats the shared branches and carries BN bookkeeping
        for k in [k for k in sd if k.startswith("pts_bbox_head.cls_branches.0.")]:
            ckpt[k.replace("cls_branches.0.", "cls_branches.%d." % i)] = sd[k]
    ckpt["img_backbone.stem.stem_1/norm.num_batches_tracked"] = torch.tensor(7)
    missing, unexpected = det.load_state_dict(ckpt, strict=True)
    assert not missing and not unexpected
    assert torch.equal(det.state_dict()["img_backbone.stem.stem_1/conv.weight"], sd["img_backbone.stem.stem_1/conv.weight"])


def test_aliases_and_train_only_names():
    for n in ("DeformableFeatureAggregationCuda", "SpatialDeformableAttention", "PerspectiveAwareAggregation"):
        assert plugin.ATTENTION.get(n) is plugin.DeformableFeatureAggregationCuda
    m = plugin.ATTENTION.build(dict(type="DeformableFeatureAggregationCuda", embed_dims=256, num_groups=8, num_levels=4, num_cams=7,
                                    dropout=0.1, num_pts=13, bias=2.0))
    assert sorted(k for k, _ in m.named_parameters()) == sorted(
        ["weights_fc.weight", "weights_fc.bias", "output_proj.weight", "output_proj.bias", "learnable_fc.weight", "learnable_fc.bias",
         "cam_embed.0.weight", "cam_embed.0.bias", "cam_embed.2.weight", "cam_embed.2.bias", "cam_embed.4.weight", "cam_embed.4.bias"])
    assert m.weights_fc.weight.shape == (416, 256) and m.learnable_fc.weight.shape == (39, 256)
    with pytest.raises(NotImplementedError):
        plugin.build_detector(config.default_model_cfg()).forward(return_loss=True)


def test_inference_without_device_is_loud():
    from far3d_amd import lib
    if lib.load().far3d_device_count() > 0:
        pytest.skip("GPU present")
    det = plugin.build_detector(config.default_model_cfg(num_query=60, num_propagated=16))
    with pytest.raises(lib.Far3dHipError):
        det.prepare("cuda:0")
    with pytest.raises(lib.Far3dHipError):
        det.simple_test([dict(pad_shape=[(64, 96, 3)], scene_token="s")], img=torch.zeros(1, 7, 3, 64, 96))

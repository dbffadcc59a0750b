"""CPU: the state-dict schema of the whole VoVNet family (the depthwise and slim specs included) against the reference's own
parameter names and shapes (tests/golden/vov_family_manifest.json, written by tools/gen_golden_vov.py), strict loading into the
registry modules, and the initialiser's determinism for the specs that existed before."""
import hashlib
import json
import os

import pytest
import torch

from far3d_amd import weights
from tests.conftest import ROOT

SPECS = ("V-19-slim-dw-eSE", "V-19-dw-eSE", "V-19-slim-eSE", "V-19-eSE", "V-39-eSE", "V-57-eSE", "V-99-eSE")


def _manifest():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "vov_family_manifest.json")))


@pytest.mark.parametrize("name", SPECS)
def test_backbone_spec_matches_reference_names_and_shapes(name):
    rows = _manifest()[name]
    spec = weights.backbone_spec(name)
    assert list(spec) == [k for k, _ in rows]                       # names, in the reference's state-dict order
    assert [tuple(v) for v in spec.values()] == [tuple(s) for _, s in rows]


def test_manifest_covers_the_reference_registry():
    assert sorted(_manifest()) == sorted(SPECS)
    assert all(n in weights.VOV_SPECS for n in SPECS)
    assert [n for n in SPECS if weights.is_dw(n)] == ["V-19-slim-dw-eSE", "V-19-dw-eSE"]


def test_reduction_only_where_widths_differ():
    """vovnet.py:200-204: a depthwise block gets a 1x1 reduction only when its input width differs from the stage width -- every
    depthwise stage but V-19-slim-dw's stage 2 (64 -> 64)."""
    for name in ("V-19-slim-dw-eSE", "V-19-dw-eSE"):
        red = sorted(int(k.split(".stage")[1][0]) for k in weights.backbone_spec(name) if "_reduction_0/conv.weight" in k)
        assert red == ([3, 4, 5] if "slim" in name else [2, 3, 4, 5]), (name, red)
    assert not any("reduction" in k or "dw_conv3x3" in k for k in weights.backbone_spec("V-19-slim-eSE"))


@pytest.mark.parametrize("cls_name", ["VoVNet", "VoVNetCP"])
@pytest.mark.parametrize("name", SPECS)
def test_registry_modules_load_strictly(name, cls_name):
    from far3d_amd import plugin
    m = plugin.BACKBONES.build(dict(type=cls_name, spec_name=name, norm_eval=True, frozen_stages=-1, input_ch=3,
                                    out_features=("stage2", "stage3", "stage4", "stage5")))
    assert isinstance(m, plugin.VoVNet) and plugin.VoVNetCP is plugin.VoVNet
    sd = weights.init_state_dict(weights.backbone_spec(name), seed=3)
    res = m.load_state_dict({k[len("img_backbone."):]: v for k, v in sd.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    got = m.state_dict()
    assert all(torch.equal(got[k[len("img_backbone."):]], v) for k, v in sd.items())


def test_detector_config_carries_the_spec_widths():
    from far3d_amd import config, plugin
    for name in ("V-19-slim-dw-eSE", "V-19-dw-eSE", "V-19-slim-eSE", "V-99-eSE"):
        cfg = config.default_model_cfg(backbone=name, num_cams=2, num_query=60, num_propagated=16, memory_len=64, topk_proposals=16)
        assert cfg["img_neck"]["in_channels"] == list(weights.VOV_SPECS[name]["stage_out_ch"])
        det = plugin.build_detector(cfg)
        spec = weights.detector_spec(name, num_query=60, num_propagated=16)
        assert {k: tuple(v.shape) for k, v in det.state_dict().items()} == {k: tuple(v) for k, v in spec.items()}
    with pytest.raises(KeyError):
        config.default_model_cfg(backbone="V-27-eSE")


def _digest(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()[:16]


# init_state_dict(detector_spec("V-99-eSE"), seed=1) as computed on the commit before the family was added: the generator draws in
# spec order, so a moved or inserted key of an existing spec would change every tensor after it
V99_SEED1 = {
    "img_backbone.stem.stem_1/conv.weight": "2e8f44dd0a741e39",
    "img_backbone.stage3.OSA3_2.layers.4.OSA3_2_4/norm.running_var": "e6e9195aa8091d66",
    "img_backbone.stage5.OSA5_3.ese.fc.bias": "5e74a51d60067641",
    "img_neck.lateral_convs.2.conv.weight": "930294d2ad651ff9",
    "pts_bbox_head.transformer.decoder.layers.5.attentions.1.learnable_fc.bias": "87ad4dae3e1f4acf",
    "img_roi_head.depthnet.depth_classifier.bias": "d4a0fe398b29c5da",
}


def test_init_state_dict_unchanged_for_existing_specs():
    spec = weights.detector_spec("V-99-eSE")
    sd = weights.init_state_dict(spec, seed=1)
    assert len(sd) == len(spec) == len(json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_manifest.json"))))
    assert list(sd)[-1] == "img_roi_head.depthnet.depth_classifier.bias"          # the last tensor drawn
    for k, want in V99_SEED1.items():
        assert _digest(sd[k]) == want, k

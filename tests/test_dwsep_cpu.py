"""CPU: the host side of the fused depthwise-separable layer -- ops.dwsep_supported (the rules of far3d_dwsep_conv_nhwc), the layers
engine.dwsep_layers names for each spec and precision, and that nothing about the default engine's configuration moved."""
import inspect

import torch

from far3d_amd import engine, ops, plugin, weights


def test_dwsep_supported_states_the_kernel_rules():
    for storage in ("bf16", "pair", ops.DT_BF16, ops.DT_BF16_PAIR, torch.bfloat16):
        for C, Cout in ((32, 32), (64, 64), (64, 32), (160, 160), (96, 224), (256, 256), (1024, 256)):
            for stride in (1, 2):
                assert ops.dwsep_supported(C, Cout, stride, storage), (C, Cout, stride, storage)
    for storage in ("bf16", "pair"):
        assert not ops.dwsep_supported(48, 64, 1, storage)          # C % 32
        assert not ops.dwsep_supported(80, 80, 1, storage)
        assert not ops.dwsep_supported(112, 112, 1, storage)
        assert not ops.dwsep_supported(64, 40, 1, storage)          # Cout % 32
        assert not ops.dwsep_supported(256, 288, 1, storage)        # Cout > 256
        assert not ops.dwsep_supported(256, 512, 1, storage)
        assert not ops.dwsep_supported(0, 64, 1, storage) and not ops.dwsep_supported(64, 0, 1, storage)
        for stride in (0, 3, 4):
            assert not ops.dwsep_supported(64, 64, stride, storage)
    for storage in ("f32", ops.DT_F32, torch.float32, ops.DT_F32_BF16X3, "fp16", None):
        assert not ops.dwsep_supported(64, 64, 1, storage), storage


def _osa(spec_name, stages=(2, 3, 4, 5)):
    s = weights.VOV_SPECS[spec_name]
    return ["s%d.b%d.c%d" % (k, b, i) for k in stages for b in range(s["block_per_stage"][k - 2]) for i in range(s["layer_per_block"])]


def test_dwsep_layers_of_the_depthwise_backbones():
    for precision in ("bf16", "bf16x3", "bf16x3_all", "bf16_fp32dec"):
        got = engine.dwsep_layers(engine.default_cfg(backbone="V-19-dw-eSE"), precision)
        assert got == ["stem2", "stem3"] + _osa("V-19-dw-eSE") and len(got) == 2 + 12, (precision, got)
    # the slim spec: stage widths 64, 80, 96, 112 -- the 80- and 112-wide layers (stages 3 and 5) keep the two launches
    got = engine.dwsep_layers(engine.default_cfg(backbone="V-19-slim-dw-eSE"), "bf16")
    assert got == ["stem2", "stem3"] + _osa("V-19-slim-dw-eSE", stages=(2, 4)), got
    spec = weights.VOV_SPECS["V-19-slim-dw-eSE"]
    assert sorted({spec["stage_conv_ch"][int(n[1]) - 2] for n in got if n.startswith("s") and n[1].isdigit()}) == [64, 96]
    # fp32 maps have no fused kernel; a dense spec has no such layer
    for name in ("V-19-dw-eSE", "V-19-slim-dw-eSE"):
        for precision in ("fp32", "bf16x3_f32act"):
            assert engine.dwsep_layers(engine.default_cfg(backbone=name), precision) == []
    for name in ("V-99-eSE", "V-19-eSE", "V-19-slim-eSE", "V-tiny-eSE"):
        for precision in ("bf16", "bf16x3", "fp32"):
            assert engine.dwsep_layers(engine.default_cfg(backbone=name), precision) == []


def test_dwsep_layers_of_the_light_head():
    """Per level the two towers' two depthwise-separable layers: four names, each one depthwise 3x3 and its pointwise 1x1 (the eight
    convolutions of the level's towers)."""
    per_level = lambda l: ["roi%d.%s%d" % (l, t, i) for t in ("cls", "reg") for i in range(2)]
    for precision in ("bf16", "bf16x3"):
        got = engine.dwsep_layers(engine.default_cfg(roi_depthwise=True, depth_level=1), precision)
        assert got == [n for l in range(4) for n in per_level(l)], got
        both = engine.dwsep_layers(engine.default_cfg(backbone="V-19-dw-eSE", roi_depthwise=True), precision)
        assert both == ["stem2", "stem3"] + _osa("V-19-dw-eSE") + got
    assert engine.dwsep_layers(engine.default_cfg(roi_depthwise=True), "fp32") == []
    assert engine.dwsep_layers(engine.default_cfg(roi_depthwise=False), "bf16") == []
    # bf16x3_2d1 assigns the towers of levels 1-3 a single bf16 product: not what the fused kernel computes, so they stay unfused
    assert engine.dwsep_layers(engine.default_cfg(roi_depthwise=True), "bf16x3_2d1") == per_level(0)
    # a cfg written before the light-head keys existed
    cfg = engine.default_cfg()
    del cfg["roi_depthwise"], cfg["depth_level"]
    assert engine.dwsep_layers(cfg, "bf16") == []


def test_default_configuration_is_unchanged():
    cfg = engine.default_cfg()
    assert "fused_dwsep" not in cfg                     # an engine attribute like roi_dw_merged, not a model option
    assert cfg["backbone"] == "V-99-eSE" and cfg["roi_depthwise"] is False and cfg["depth_level"] == 0
    assert engine.dwsep_layers(cfg, "bf16") == [] and engine.dwsep_layers(cfg, "bf16x3") == []      # the default plan has nothing to fuse
    # the flag is off unless asked for, in the engine and through Far3D.prepare
    src = inspect.getsource(engine.Far3DEngine.__init__)
    assert "self.fused_dwsep = False" in src
    p = inspect.signature(plugin.Far3D.prepare).parameters
    assert list(p)[:4] == ["self", "device", "precision", "fused_dwsep"] and p["fused_dwsep"].default is False
    assert p["device"].default == "cuda:0" and p["precision"].default == "bf16"

"""GPU: engine.fused_dwsep -- the depthwise-separable layers of the light models as one far3d_dwsep_conv_nhwc launch each.

The fused layer differs from the two launches only in the accumulation order of the pointwise sums, so it must be as close to the exact
engine as they are: for every output, dist(fused, fp32) <= 1.5 dist(unfused, fp32) + 2^-16 max|map|, dist = max |a - b|.  The yardstick is
the fp32 engine (exact fp32 MFMA) on the same weights and inputs; the unfused engine is the parent's code.
Backbone: V-19-dw-eSE on 2 x 3 x 64 x 96 (stage maps 16x24 ... 2x3).  Light head: depthwise towers on four levels 16x24 ... 2x3, N = 2.
Capture: the light detector captured into a hipGraph with the flag on returns the eager fused bits."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from far3d_amd import config, plugin, synth, weights
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BB = "V-19-dw-eSE"
HW = ((16, 24), (8, 12), (4, 6), (2, 3))
R = "img_roi_head."


@functools.lru_cache(maxsize=None)
def _bb_case():
    sd = weights.init_state_dict(weights.backbone_spec(BB), seed=7)
    return sd, torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(29))


@functools.lru_cache(maxsize=None)
def _roi_case():
    spec = {k: v for k, v in weights.detector_spec(roi_depthwise=True).items() if k.startswith(R)}
    sd = weights.init_state_dict(spec, seed=11)
    g = torch.Generator().manual_seed(23)
    return sd, tuple(torch.randn(2, 256, h, w, generator=g) for h, w in HW)


def _count_fused(eng_mod):
    """Wrap ops.dwsep_conv_nhwc to count its calls; returns (counter list, restore function)."""
    real, n = eng_mod.ops.dwsep_conv_nhwc, []

    def spy(*a, **k):
        n.append(1)
        return real(*a, **k)
    eng_mod.ops.dwsep_conv_nhwc = spy
    return n, lambda: setattr(eng_mod.ops, "dwsep_conv_nhwc", real)


def _backbone(precision, fused):
    from far3d_amd import engine
    sd, x = _bb_case()
    eng = engine.Far3DEngine(sd, engine.default_cfg(backbone=BB), device=DEV, precision=precision, parts=("backbone",))
    assert eng.fused_dwsep is False
    eng.fused_dwsep = fused
    n, restore = _count_fused(engine)
    try:
        outs = [eng.act_to_nchw(o) for o in eng.backbone(x.to(DEV))]
    finally:
        restore()
    torch.cuda.synchronize()
    layers = engine.dwsep_layers(eng.cfg, precision)
    assert len(n) == (len(layers) if fused else 0), (precision, fused, len(n), len(layers))
    has_tmp = any("dw_tmp" in k for k in eng._bufs)
    assert has_tmp == (not fused or len(layers) < 14), "the scratch map of a fused layer was allocated"
    return outs


def _roi(precision, fused):
    from far3d_amd import engine
    sd, maps = _roi_case()
    eng = engine.Far3DEngine(sd, engine.default_cfg(roi_depthwise=True, depth_level=1), device=DEV, precision=precision, parts=("roi",))
    eng.fused_dwsep = fused
    n, restore = _count_fused(engine)
    try:
        cls, reg, depth = eng.roi_head([eng.act_from_nchw(m.to(DEV)) for m in maps])
    finally:
        restore()
    torch.cuda.synchronize()
    assert len(n) == (16 if fused and precision != "fp32" else 0), (precision, fused, len(n))
    return list(cls) + list(reg) + [depth]


def _check(run, names, precision):
    exact = run("fp32", False)
    plain, fused = run(precision, False), run(precision, True)
    for name, e, p, f in zip(names, exact, plain, fused):
        assert p.shape == e.shape == f.shape and f.dtype == p.dtype
        du, df = float((p.float() - e.float()).abs().max()), float((f.float() - e.float()).abs().max())
        mx = float(e.float().abs().max())
        print("%s %s: dist(unfused, fp32) %.4e  dist(fused, fp32) %.4e  max|map| %.4e  fused differs from unfused: %s" %
              (precision, name, du, df, mx, not torch.equal(p, f)))
        assert df <= 1.5 * du + 2.0 ** -16 * mx, "%s %s: fused %.4e vs unfused %.4e from the fp32 engine (max %.3e)" % (precision, name, df, du, mx)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_backbone_fused_as_close_to_fp32_as_unfused(hip_lib, precision):
    _check(_backbone, ["stage%d" % k for k in range(2, 6)], precision)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_light_head_fused_as_close_to_fp32_as_unfused(hip_lib, precision):
    _check(_roi, ["cls%d" % l for l in range(4)] + ["reg%d" % l for l in range(4)] + ["depth_logit"], precision)


def test_flag_off_is_the_parent_path_bitwise(hip_lib):
    """Setting the flag and clearing it again leaves the two-launch path: the default engine's bits."""
    from far3d_amd import engine
    sd, maps = _roi_case()
    eng = engine.Far3DEngine(sd, engine.default_cfg(roi_depthwise=True, depth_level=1), device=DEV, precision="bf16", parts=("roi",))
    xs = [eng.act_from_nchw(m.to(DEV)) for m in maps]
    flat = lambda o: [t.clone() for t in list(o[0]) + list(o[1]) + [o[2]]]
    n, restore = _count_fused(engine)
    try:
        a = flat(eng.roi_head(xs))
        assert len(n) == 0, "the default engine issued a fused launch"
        eng.fused_dwsep = True
        eng.roi_head(xs)
        assert len(n) == 16
        eng.fused_dwsep = False
        c = flat(eng.roi_head(xs))
        assert len(n) == 16
    finally:
        restore()
    assert all(torch.equal(x, y) for x, y in zip(a, c))


def test_captured_graph_returns_the_eager_fused_bits(hip_lib):
    """The light detector (V-19-slim-dw-eSE: the 64- and 96-wide backbone layers and every tower layer fused) in bf16 through
    Far3D.prepare(fused_dwsep=True): eager frames against a captured hipGraph and its replays."""
    from far3d_amd import engine
    z = np.load(os.path.join(ROOT, "tests", "golden", "far3d_light_head_seq.npz"))
    rc = json.loads(bytes(z["recipe"]).decode())
    res = {}
    for mode in ("eager", "graph"):
        det = plugin.build_detector(config.default_model_cfg(backbone=rc["backbone"], num_cams=rc["num_cams"], num_query=rc["num_query"],
                                                             num_propagated=rc["num_propagated"], memory_len=rc["memory_len"],
                                                             topk_proposals=rc["topk_proposals"], use_depthwise=True,
                                                             reg_depth_level=rc["reg_depth_level"], proposal_capacity=48))
        spec = weights.detector_spec(rc["backbone"], num_query=rc["num_query"], num_propagated=rc["num_propagated"], roi_depthwise=True, depth_level=1)
        det.load_state_dict(weights.init_state_dict(spec, seed=rc["weight_seed"]))
        det.prepare(DEV, precision="bf16", fused_dwsep=True)
        assert det.engine.fused_dwsep is True and len(engine.dwsep_layers(det.engine.cfg, "bf16")) == 2 + 6 + 16
        det.engine.use_graph = mode == "graph"
        n, restore = _count_fused(engine)
        out = []
        try:
            for fi in list(range(rc["frames"])) + [rc["frames"] - 1] * 2:   # frame 0 starts the scene eagerly; then capture and replays
                data, metas = synth.recipe_frame(rc, fi)
                det(return_loss=False, rescale=True, img_metas=metas, **data)
                o = det.last_outs
                out.append((int(o["num_adaptive_dev"].item()), o["all_cls_scores"].clone(), o["all_bbox_preds"].clone()))
        finally:
            restore()
        assert len(n) >= 24, "the fused launches were not issued"
        assert not any("dw_tmp" in k and (k[-1] in (64, 96) or k[-1] == 256) for k in det.engine._bufs), "scratch map of a fused layer"
        if mode == "graph":
            assert det.engine._graph is not None, "the steady-state frame was not captured"
        res[mode] = out
    for fi, (a, b) in enumerate(zip(res["eager"], res["graph"])):
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "frame %d: graph differs from eager" % fi

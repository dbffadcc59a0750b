"""GPU: the depthwise and slim VoVNet specs through the engine, the registry module and the detector, against the reference's own
outputs (tests/golden/vov_family_maps.npz, far3d_dw_seq.npz; tools/gen_golden_vov.py).

Stage maps: fp32 within 1e-4 of the reference map's maximum and bf16 within 2e-2 of it -- the bars tests/test_plugin_modules_gpu.py holds
the backbone module to.  The fixture keeps the two large maps at every second row and column (plus the last ones; every channel) and the two small ones in full; the
maximum is that of the full reference map."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from far3d_amd import config, plugin, synth, weights
from tests.conftest import ROOT, assert_detections_match

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ("V-19-slim-dw-eSE", "V-19-dw-eSE", "V-19-slim-eSE")
SLIM = ("V-19-slim-dw-eSE", "V-19-slim-eSE")


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """(state dict, input, [(reference samples, rows, cols, full-map maximum)] per stage) -- loaded once, never modified."""
    z = np.load(os.path.join(GOLD, "vov_family_maps.npz"))
    sd = weights.init_state_dict(weights.backbone_spec(name), seed=int(z[name + "_seed"]))
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(int(z[name + "_input_seed"])))
    maps = []
    for k in range(2, 6):
        p = "%s_s%d" % (name, k)
        assert float(z[p + "_f64_dev"]) < 2.5e-5                      # the reference's own fp32 error: a quarter of the fp32 bar
        maps.append((torch.from_numpy(z[p]), z[p + "_rows"].tolist(), z[p + "_cols"].tolist(), float(z[p + "_max"])))
    return sd, x, maps


def _errors(got, maps, tag):
    """Per stage: max |got - reference| / max |reference| at the fixture's pixels.  got: four (N,C,H,W) fp32 maps."""
    errs = []
    for k, (g, (want, rows, cols, mx)) in enumerate(zip(got, maps)):
        s = g.cpu()[:, :, rows][:, :, :, cols]
        assert tuple(s.shape) == tuple(want.shape), (tag, k, s.shape, want.shape)
        errs.append(float((s - want).abs().max()) / mx)
    print("%s: stage errors / max %s" % (tag, ", ".join("%.2e" % e for e in errs)))
    return errs


def _engine_maps(name, precision, x=None, sd=None):
    from far3d_amd import engine
    fsd, fx, _ = _fixture(name)
    eng = engine.Far3DEngine(sd or fsd, engine.default_cfg(backbone=name), device=DEV, precision=precision, parts=("backbone",))
    outs = eng.backbone((fx if x is None else x).to(DEV))
    return eng, [eng.act_to_nchw(o) for o in outs]


@pytest.mark.parametrize("name", NEW)
def test_fp32_engine_and_module_match_reference_maps(hip_lib, name):
    sd, x, maps = _fixture(name)
    eng, got = _engine_maps(name, "fp32")
    assert [tuple(g.shape[1:]) for g in got] == [(c, h, w) for c, (h, w) in zip(weights.VOV_SPECS[name]["stage_out_ch"],
                                                                                  ((16, 24), (8, 12), (4, 6), (2, 3)))]
    assert all(e < 1e-4 for e in _errors(got, maps, "%s fp32 engine" % name))
    if weights.is_dw(name):                    # the new convs are addressable by name (per-layer precision machinery)
        assert {"stem2.pw", "stem3.pw", "s3.b0.red", "s3.b0.c1.pw", "s5.b0.c2.pw"} <= set(eng.convs)
        assert ("s2.b0.red" in eng.convs) == ("slim" not in name)
    for cls_name in ("VoVNet", "VoVNetCP"):
        bb = plugin.BACKBONES.build(dict(type=cls_name, spec_name=name, norm_eval=True, frozen_stages=-1, input_ch=3,
                                         out_features=("stage2", "stage3", "stage4", "stage5")))
        bb.load_state_dict({k[len("img_backbone."):]: v for k, v in sd.items()}, strict=True)
        bb.precision = "fp32"
        assert all(e < 1e-4 for e in _errors(bb(x.to(DEV)), maps, "%s fp32 %s module" % (name, cls_name)))


@pytest.mark.parametrize("name", NEW)
def test_bf16_engine_bounded_and_image_independent(hip_lib, name):
    sd, x, maps = _fixture(name)
    _, got = _engine_maps(name, "bf16")
    assert all(e < 2e-2 for e in _errors(got, maps, "%s bf16 engine" % name))
    # 2 images vs 1 + 1, to the same bound
    single = [_engine_maps(name, "bf16", x=x[n:n + 1])[1] for n in range(2)]
    for k, (g, (_, _, _, mx)) in enumerate(zip(got, maps)):
        for n in range(2):
            d = float((g[n] - single[n][k][0]).abs().max()) / mx
            assert d < 2e-2, "%s stage %d image %d: batch of 2 vs alone %.3e" % (name, k + 2, n, d)


def test_slim_specs_run_in_every_unpaired_mode(hip_lib):
    """The slim specs in the remaining modes without pair storage.  bf16 activations: the bf16 bar.  bf16x3_f32act (fp32 maps, split
    products): read against the bf16 engine on the same fixture, as the pair test below does -- closer on every map."""
    for name in SLIM:
        _, _, maps = _fixture(name)
        for precision in ("bf16_fp32dec", "bf16_fp32val"):
            assert all(e < 2e-2 for e in _errors(_engine_maps(name, precision)[1], maps, "%s %s" % (name, precision)))
        e16 = _errors(_engine_maps(name, "bf16")[1], maps, "%s bf16" % name)
        e3 = _errors(_engine_maps(name, "bf16x3_f32act")[1], maps, "%s bf16x3_f32act" % name)
        assert all(a < b for a, b in zip(e3, e16)), (name, e3, e16)


def test_pair_engine_closer_than_bf16(hip_lib):
    """V-19-dw-eSE in bf16x3 (pair-stored maps, split products) against the bf16 engine, both read against the reference fixture."""
    name = "V-19-dw-eSE"
    _, _, maps = _fixture(name)
    e16 = _errors(_engine_maps(name, "bf16")[1], maps, "%s bf16" % name)
    e3 = _errors(_engine_maps(name, "bf16x3")[1], maps, "%s bf16x3" % name)
    assert all(a < b for a, b in zip(e3, e16)), (e3, e16)
    for precision in ("bf16x3_all", "bf16x3_2d1"):
        assert all(e < 2e-2 for e in _errors(_engine_maps(name, precision)[1], maps, "%s %s" % (name, precision)))


@pytest.mark.parametrize("name", SLIM)
@pytest.mark.parametrize("precision", ["bf16x3", "bf16x3_all", "bf16x3_2d1"])
def test_slim_specs_refuse_pair_storage(hip_lib, name, precision):
    from far3d_amd import engine
    sd, _, _ = _fixture(name)
    with pytest.raises(ValueError) as e:
        engine.Far3DEngine(sd, engine.default_cfg(backbone=name), device=DEV, precision=precision, parts=("backbone",))
    msg = str(e.value)
    assert name in msg and "80" in msg and "fp32" in msg and "bf16_fp32dec" in msg and "bf16x3_f32act" in msg and precision in msg


# ------------------------------------------------------------------------------------------ detector level
def _dw_detector(**over):
    z = np.load(os.path.join(GOLD, "far3d_dw_seq.npz"))
    rc = json.loads(bytes(z["recipe"]).decode())
    assert rc["backbone"] == "V-19-slim-dw-eSE"
    det = plugin.build_detector(config.default_model_cfg(backbone=rc["backbone"], num_cams=rc["num_cams"], num_query=rc["num_query"],
                                                         num_propagated=rc["num_propagated"], memory_len=rc["memory_len"],
                                                         topk_proposals=rc["topk_proposals"], **over))
    spec = weights.detector_spec(rc["backbone"], num_query=rc["num_query"], num_propagated=rc["num_propagated"])
    det.load_state_dict(weights.init_state_dict(spec, seed=rc["weight_seed"]))
    det.prepare(DEV, precision="fp32")
    return det, z, rc


def test_dw_detector_fp32_matches_reference_legacy_mode(hip_lib):
    det, z, rc = _dw_detector()
    for fi in range(rc["frames"]):
        data, metas = synth.recipe_frame(rc, fi)
        res = det(return_loss=False, rescale=True, img_metas=metas, **data)[0]["pts_bbox"]
        o = det.last_outs
        want_idx = z["f%d_valid_idx" % fi]
        cnt = o["sel_cnt"].cpu().numpy()
        got = [(n, int(i)) for n in range(rc["num_cams"]) for i in o["sel_idx"][n, :cnt[n]].cpu().numpy()]
        assert got == [(int(r[0]), int(r[1])) for r in want_idx], "frame %d: proposal set differs" % fi
        assert np.allclose(o["bbox2d"].cpu().numpy(), z["f%d_bbox2d" % fi], rtol=2e-3, atol=2e-3)
        for key in ("all_cls_scores", "all_bbox_preds"):
            g, want = o[key].cpu().numpy(), z["f%d_%s" % (fi, key)]
            assert g.shape == want.shape, (fi, key, g.shape, want.shape)
            err = np.abs(g - want)
            print("far3d_dw_seq frame %d %s: max abs err %.3e" % (fi, key, err.max()))
            if key == "all_cls_scores":
                assert err.max() < 1e-3, "frame %d logits: max abs err %.3e" % (fi, err.max())
            else:                                                            # the bounds of tests/test_multidepth_gpu.py::_check_frame
                assert err[..., :3].max() < 0.076 and err[..., 3:].max() < 1e-3, "frame %d boxes" % fi
        assert_detections_match(tuple(res[k].cpu().numpy() for k in ("labels_3d", "boxes_3d", "scores_3d")),
                                tuple(z["f%d_%s" % (fi, k)] for k in ("labels_3d", "boxes_3d", "scores_3d")), "frame %d" % fi)


def test_dw_detector_graph_bitwise_eager(hip_lib):
    res = {}
    for mode in ("eager", "graph"):
        det, z, rc = _dw_detector(proposal_capacity=48)
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
    M = [int(np.load(os.path.join(GOLD, "far3d_dw_seq.npz"))["f%d_bbox2d" % fi].shape[0]) for fi in range(2)]
    assert [r[0] for r in res["eager"][:2]] == M                            # the fixed-capacity run counts the reference's proposals

"""GPU: the decoder modules run on their own -- plugin.Detr3DTransformer / Detr3DTransformerDecoder / Detr3DTemporalDecoderLayer /
MultiheadAttention forwards against tests/golden/far3d_transformer_seq.npz: the reference's own Detr3DTransformer in float64 (two
samples, 29 queries, 80 keys, 3 layers, without and with a bool attn_mask), recorded by tools/gen_golden_transformer.py.

Bar, per layer l and run: max |states - float64| <= 8 * dev64[l], where dev64[l] is what the reference itself is off by when it runs in
fp32.  Why 8: the existing tests accept 2e-5 from the fp32 attention core and LayerNorm on O(1) data, where the fp32 reference's own
rounding noise is about 2.5e-6 -- eight is the ratio the project already accepts for one operator.  The measured ratios are printed and
kept in profiles/attn_batch/README.md."""
import json
import os

import numpy as np
import pytest
import torch

from tests import transformer_cases as TC
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATIO = 8.0


@pytest.fixture(scope="module")
def rig(hip_lib):
    from far3d_amd import plugin
    z = np.load(os.path.join(ROOT, "tests", "golden", "far3d_transformer_seq.npz"))
    rc = json.loads(bytes(z["recipe"]).decode())
    model = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_config.json")))["model"]
    tr = plugin.TRANSFORMER.build(TC.transformer_cfg(model, rc))
    names = TC.seed_weights(tr, rc["weight_seed"])
    assert names == json.loads(bytes(z["names"]).decode())["state_dict"]
    case = TC.transformer_case(rc)
    for k, v in TC.input_digest(case).items():
        assert np.array_equal(z["digest_" + k], v.numpy()), "input %s is not the fixture's" % k
    mask = TC.transformer_mask(rc)
    assert np.array_equal(z["attn_mask"], mask.numpy())
    tr = tr.to(DEV)
    tr.precision = "fp32"
    dev = lambda t: t.to(DEV)
    runs = {name: tr(*TC.forward_args(case, m, dev)) for name, m in (("nomask", None), ("mask", mask))}     # computed once, shared
    return dict(z=z, rc=rc, tr=tr, case=case, mask=mask, runs=runs, dev=dev)


@pytest.mark.parametrize("run", ["nomask", "mask"])
def test_transformer_forward_within_8x_the_references_own_fp32_noise(rig, run):
    z, rc = rig["z"], rig["rc"]
    got = rig["runs"][run]
    assert got.shape == (rc["num_layers"], rc["bs"], rc["A"], rc["embed_dims"]) and got.dtype == torch.float32
    want, dev64 = torch.from_numpy(z["states_" + run]).double(), z["dev64_" + run]
    err = (got.cpu().double() - want).abs().flatten(1).max(dim=1).values.tolist()
    for l, (e, d) in enumerate(zip(err, dev64)):
        print("%s layer %d: max err %.3e, dev64 %.3e, ratio %.2f" % (run, l, e, d, e / d))
    for l, (e, d) in enumerate(zip(err, dev64)):
        assert e <= RATIO * d, "%s layer %d: %.3e above %g x dev64 = %.3e" % (run, l, e, RATIO, RATIO * d)


def test_decoder_and_single_layer_give_the_transformers_tensors(rig):
    tr, case, mask, dev = rig["tr"], rig["case"], rig["mask"], rig["dev"]
    a = TC.forward_args(case, mask, dev)
    query, query_pos, feat, spatial, lsi, mem, mpos, am, ref, pc, data, metas = a
    full = rig["runs"]["mask"]
    dec = tr.decoder(query, query_pos, feat, mem, mpos, ref, spatial, lsi, pc, data["lidar2img"], metas, am)
    assert torch.equal(dec, full)
    x = query
    for l, layer in enumerate(tr.decoder.layers):
        x = layer(x, query_pos, feat, mem, mpos, ref, spatial, lsi, pc, data["lidar2img"], metas, am)
        assert torch.equal(x, full[l]), "layer %d called directly" % l
    # a list of two masks is read like one tensor (only the self-attention reads its entry); no memory: the keys are the queries
    one = tr.decoder.layers[0](query, query_pos, feat, mem, mpos, ref, spatial, lsi, pc, data["lidar2img"], metas, [am, None])
    assert torch.equal(one, full[0])
    nomem = tr.decoder.layers[0](query, query_pos, feat, None, None, ref, spatial, lsi, pc, data["lidar2img"], metas, None)
    assert nomem.shape == query.shape and bool(torch.isfinite(nomem).all())


def test_sample_0_of_two_equals_its_own_call(rig):
    z, rc, tr, case, dev = rig["z"], rig["rc"], rig["tr"], rig["case"], rig["dev"]
    one = {k: (v[:1] if k in ("query", "query_pos", "temp_memory", "temp_pos", "reference_points", "lidar2img") else v) for k, v in case.items()}
    one["feat_flatten"] = case["feat_flatten"][:rc["num_cams"]]
    got = tr(*TC.forward_args(one, None, dev))
    assert got.shape == (rc["num_layers"], 1, rc["A"], rc["embed_dims"])
    want, dev64 = torch.from_numpy(z["states_nomask"]).double()[:, :1], z["dev64_nomask"]
    err = (got.cpu().double() - want).abs().flatten(1).max(dim=1).values.tolist()
    for l, (e, d) in enumerate(zip(err, dev64)):
        print("bs = 1 layer %d: max err %.3e, ratio %.2f; vs sample 0 of bs = 2: %.3e" %
              (l, e, e / d, (got[l, 0] - rig["runs"]["nomask"][l, 0]).abs().max().item()))
    for l, (e, d) in enumerate(zip(err, dev64)):
        assert e <= RATIO * d, "bs = 1 layer %d: %.3e above %g x dev64" % (l, e, RATIO)


@pytest.mark.parametrize("batch_first", [True, False])
def test_one_sample_without_masks_keeps_todays_calls_and_bits(rig, batch_first):
    """bs = 1, no mask: MultiheadAttention.forward is the composition of ops.linear / ops.attention_forward it was before."""
    from far3d_amd import ops, plugin
    src = rig["tr"].decoder.layers[1].attentions[0]
    m = plugin.MultiheadAttention(256, 8, batch_first=batch_first)
    m.load_state_dict(src.state_dict())
    m = m.to(DEV)
    m.precision = "fp32"
    g = torch.Generator().manual_seed(4)
    x, qpos, key, kpos = (torch.randn(1, n, 256, generator=g).to(DEV) for n in (41, 41, 64, 64))
    t = (lambda a: a) if batch_first else (lambda a: a.transpose(0, 1))
    got = m(t(x), t(key), t(key), None, query_pos=t(qpos), key_pos=t(kpos))
    E = 256
    w, b = m.attn.in_proj_weight.data, m.attn.in_proj_bias.data
    pk = lambda ww, bb: ops.PackedConv(ww, bb, dtype=torch.float32, device=torch.device(DEV))
    Q = ops.linear((x[0] + qpos[0]).contiguous(), pk(w[:E], b[:E]))
    K = ops.linear((key[0] + kpos[0]).contiguous(), pk(w[E:2 * E], b[E:2 * E]))
    V = ops.linear(key[0].contiguous(), pk(w[2 * E:], b[2 * E:]))
    att = ops.attention_forward(Q, K, V, num_heads=8)
    want = ops.linear(att, pk(m.attn.out_proj.weight.data, m.attn.out_proj.bias.data), res=x[0].contiguous())
    assert torch.equal(t(got)[0] if not batch_first else got[0], want)
    # and the masked / batched path computes the same attention (another kernel: rounding, not bits)
    zero = torch.zeros(41, 64, dtype=torch.bool, device=DEV)
    masked = m(t(x), t(key), t(key), None, query_pos=t(qpos), key_pos=t(kpos), attn_mask=zero)
    assert masked.shape == got.shape and (masked - got).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())


def test_multihead_attention_masks_against_torch_float64(rig):
    """Both batch_first values, bool 3-D mask plus key padding, against torch.nn.MultiheadAttention in float64 under mmcv's wrapper
    semantics (positions on q / k only, identity + out); the bar of tests/test_plugin_modules_gpu.py's module test."""
    from far3d_amd import plugin
    src = rig["tr"].decoder.layers[2].attentions[0]
    g = torch.Generator().manual_seed(6)
    bs, Aq, Nk = 2, 29, 80
    x, qpos, key, kpos = (torch.randn(bs, n, 256, generator=g) for n in (Aq, Aq, Nk, Nk))
    am = torch.rand(bs * 8, Aq, Nk, generator=g) < 0.3
    kp = torch.rand(bs, Nk, generator=g) < 0.2
    ref = torch.nn.MultiheadAttention(256, 8, 0.0, batch_first=True).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in src.attn.state_dict().items()})
    with torch.no_grad():
        want = x.double() + ref.train()((x + qpos).double(), (key + kpos).double(), key.double(), attn_mask=am, key_padding_mask=kp)[0]
    for batch_first in (True, False):
        m = plugin.MultiheadAttention(256, 8, batch_first=batch_first)
        m.load_state_dict(src.state_dict())
        m = m.to(DEV)
        m.precision = "fp32"
        t = (lambda a: a.to(DEV)) if batch_first else (lambda a: a.to(DEV).transpose(0, 1))
        got = m(t(x), t(key), t(key), None, query_pos=t(qpos), key_pos=t(kpos), attn_mask=am.to(DEV), key_padding_mask=kp.to(DEV))
        got = got if batch_first else got.transpose(0, 1)
        err = (got.cpu().double() - want).abs().max().item()
        print("MultiheadAttention batch_first=%s masks: max err %.3e" % (batch_first, err))
        assert got.shape == want.shape and err < 2e-5 * max(1.0, want.abs().max().item())


def test_bf16_precision_is_finite_and_shaped(rig):
    tr, case, mask, dev, rc = rig["tr"], rig["case"], rig["mask"], rig["dev"], rig["rc"]
    tr.precision = "bf16"
    try:
        got = tr(*TC.forward_args(case, mask, dev))
    finally:
        tr.precision = "fp32"
    assert got.shape == (rc["num_layers"], rc["bs"], rc["A"], rc["embed_dims"]) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    d = (got - rig["runs"]["mask"]).abs().flatten(1)
    print("bf16 vs fp32 per layer: max %s mean %s" % (["%.3e" % v for v in d.max(dim=1).values.tolist()], ["%.3e" % v for v in d.mean(dim=1).tolist()]))
    again = tr(*TC.forward_args(case, mask, dev))         # back in fp32: the packed weights follow the precision attribute
    assert torch.equal(again, rig["runs"]["mask"])

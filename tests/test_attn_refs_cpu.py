"""CPU: tests/attn_refs.py (the float64 yardstick of the batched attention kernel) against torch.nn.MultiheadAttention in float64.
The module's in/out projections are set to the identity with zero biases, which isolates the core: scores, masks, softmax, PV."""
import pytest
import torch

from tests import attn_refs as R

B, AQ, NK, H, E = 3, 7, 11, 4, 32


def _mha():
    m = torch.nn.MultiheadAttention(E, H, dropout=0.0, batch_first=True).double()
    with torch.no_grad():
        m.in_proj_weight.copy_(torch.eye(E, dtype=torch.float64).repeat(3, 1))
        m.in_proj_bias.zero_()
        m.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
        m.out_proj.bias.zero_()
    return m.train()     # dropout is 0; training mode keeps torch on its plain (non-fused) path


def _qkv(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, AQ, E, generator=g, dtype=torch.float64) * 2, torch.randn(B, NK, E, generator=g, dtype=torch.float64),
            torch.randn(B, NK, E, generator=g, dtype=torch.float64), g)


def _masks(kind, g):
    am = kp = None
    if kind in ("bool2d", "both", "full_row"):
        am = torch.rand(AQ, NK, generator=g) < 0.3
        am[:, 0] = False
    if kind == "bool3d":
        am = torch.rand(B * H, AQ, NK, generator=g) < 0.3
        am[:, :, 0] = False
    if kind == "float":
        am = (torch.rand(AQ, NK, generator=g, dtype=torch.float64) * 8 - 4).masked_fill(torch.rand(AQ, NK, generator=g) < 0.2, float("-inf"))
        am[:, 0] = 0.5
    if kind in ("padding", "both"):
        kp = torch.zeros(B, NK, dtype=torch.bool)
        kp[0, 8:] = True
        kp[2, 3] = True
    if kind == "full_row":
        am[4, :] = True
    return am, kp


@pytest.mark.parametrize("kind", ["none", "bool2d", "bool3d", "float", "padding", "both", "full_row"])
def test_restatement_equals_torch_mha_float64(kind):
    q, k, v, g = _qkv(11)
    am, kp = _masks(kind, g)
    with torch.no_grad():
        want = _mha()(q, k, v, attn_mask=am, key_padding_mask=kp)[0]
    got = R.attention_ref(q, k, v, H, attn_mask=am, key_padding_mask=kp)
    assert got.shape == want.shape == (B, AQ, E) and got.dtype == torch.float64
    if kind == "full_row":
        assert bool(torch.isnan(want[:, 4]).all()) and bool(torch.isnan(got[:, 4]).all())       # NaN in both, the whole row
        keep = [i for i in range(AQ) if i != 4]
        got, want = got[:, keep], want[:, keep]
    assert bool(torch.isfinite(want).all()) and bool(torch.isfinite(got).all())
    err = (got - want).abs().max().item()
    print("%s: max |restatement - torch| = %.3e" % (kind, err))
    assert err <= 1e-12


def test_float_inputs_are_promoted_and_uint8_masks_exclude():
    q, k, v, g = _qkv(12)
    am = torch.rand(AQ, NK, generator=g) < 0.3
    am[:, 0] = False
    a = R.attention_ref(q.float(), k.float(), v.float(), H, attn_mask=am.to(torch.uint8))
    b = R.attention_ref(q.float().double(), k.float().double(), v.float().double(), H, attn_mask=am)
    assert a.dtype == torch.float64 and torch.equal(a, b)

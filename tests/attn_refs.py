"""Float64 restatement of the masked multi-head attention core that far3d_attention_batched computes: per sample b and head h
out[b] = softmax(q[b] k[b]^T / sqrt(d) + M[b,h] + P[b]) v[b] -- scores, masks, softmax, PV, nothing else.  Checked against
torch.nn.MultiheadAttention in float64 by tests/test_attn_refs_cpu.py; the yardstick of tests/test_attn_batch_gpu.py.

attn_mask: (Aq, Nk) or (B * H, Aq, Nk); bool / uint8 -> nonzero excludes the key (-inf), a float mask is added.
key_padding_mask: (B, Nk) bool / uint8, nonzero excludes the key for every query of the sample.
A query without a key left is NaN in its whole row (softmax of all -inf = 0 / 0), as in torch."""
import torch


def additive_mask(attn_mask, key_padding_mask, B, H, Aq, Nk):
    """The two masks as one float64 (B, H, Aq, Nk) term added to the scores."""
    add = torch.zeros(B, H, Aq, Nk, dtype=torch.float64)
    if attn_mask is not None:
        m = attn_mask
        if m.dtype in (torch.bool, torch.uint8):
            m = torch.zeros(m.shape, dtype=torch.float64).masked_fill(m != 0, float("-inf"))
        m = m.double()
        add = add + (m.view(1, 1, Aq, Nk) if m.dim() == 2 else m.view(B, H, Aq, Nk))
    if key_padding_mask is not None:
        p = torch.zeros(B, Nk, dtype=torch.float64).masked_fill(key_padding_mask != 0, float("-inf"))
        add = add + p.view(B, 1, 1, Nk)
    return add


def attention_ref(q, k, v, num_heads, attn_mask=None, key_padding_mask=None):
    """q (B, Aq, E), k / v (B, Nk, E), any float dtype -> (B, Aq, E) float64."""
    q, k, v = q.double(), k.double(), v.double()
    B, Aq, E = q.shape
    Nk = k.shape[1]
    d = E // num_heads
    qh = (q * d ** -0.5).view(B, Aq, num_heads, d).transpose(1, 2)
    kh = k.view(B, Nk, num_heads, d).transpose(1, 2)
    vh = v.view(B, Nk, num_heads, d).transpose(1, 2)
    s = qh @ kh.transpose(2, 3) + additive_mask(attn_mask, key_padding_mask, B, num_heads, Aq, Nk)
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    p = e / e.sum(dim=-1, keepdim=True)          # a row of all -inf: 0 / 0 = NaN
    return (p @ vh).transpose(1, 2).reshape(B, Aq, E)

"""GPU: far3d_attention_batched (csrc/attn_batch.hip) through ops.attention_batched against the float64 restatement tests/attn_refs.py
on the FULL tensor.  Bars are the ones tests/test_attn_norm_gpu.py holds the same arithmetic to on the same data (randn, q * 2):
fp32 2e-5 max (5e-5 with the forced rescale), bf16 1e-2 max and 1e-3 mean -- masks only remove terms, so none is wider.
Shapes (B, Aq, Nk): one tile; a tail query block with two key tiles; two query blocks with two tiles plus a tail; 300 x 333 once.
A row the reference makes NaN (no key left) must be NaN in every element, and no other element may be."""
import ctypes

import pytest
import torch

from tests import attn_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, E = 8, 256
SHAPES = [(1, 37, 50), (3, 29, 80), (2, 70, 130)]
CASES = ["none", "bool2d", "bool3d", "f32", "padding_last_tile", "both", "first64", "last_partial", "full_row"]
_cache = {}


def _data(B, Aq, Nk, seed=None):
    g = torch.Generator().manual_seed(1000 * B + 10 * Aq + Nk if seed is None else seed)
    q, k, v = (torch.randn(B, n, E, generator=g) for n in (Aq, Nk, Nk))
    return q * 2.0, k, v, g      # q * 2: a softmax peaky enough to exercise the running-max rescale


def _masks(case, B, Aq, Nk, g):
    am = kp = None
    if case in ("bool2d", "both", "first64", "last_partial", "full_row"):
        am = torch.rand(Aq, Nk, generator=g) < 0.3
    if case == "bool3d":
        am = torch.rand(B * H, Aq, Nk, generator=g) < 0.3
    if case == "f32":
        am = (torch.rand(Aq, Nk, generator=g) * 8 - 4).masked_fill(torch.rand(Aq, Nk, generator=g) < 0.2, float("-inf"))
    if case == "padding_last_tile":     # the whole last 64-key tile; with a single tile (Nk <= 64) its second 32-key half instead
        kp = torch.zeros(B, Nk, dtype=torch.bool)
        kp[:, (64 * ((Nk - 1) // 64) if Nk > 64 else 32):] = True
    if case == "both":
        kp = torch.rand(B, Nk, generator=g) < 0.25
        kp[:, 1] = False
    r = Aq // 2 + 1
    if case == "first64":               # the row's first tile is excluded entirely: its state must survive an all -inf FIRST tile
        am[r, :64] = True
        am[r, 64:] = False
    if case == "last_partial":          # the only key left lies in the last (partial) tile
        am[r, :] = True
        am[r, Nk - 1] = False
    if case == "full_row":
        am[r, :] = True
    return am, kp


def _inputs(shape, case):
    key = (shape, case)
    if key not in _cache:
        B, Aq, Nk = shape
        q, k, v, g = _data(B, Aq, Nk)
        am, kp = _masks(case, B, Aq, Nk, g)
        want = {dt: R.attention_ref(q.to(dt), k.to(dt), v.to(dt), H, am, kp) for dt in (torch.float32, torch.bfloat16)}
        _cache[key] = (q, k, v, am, kp, want)
    return _cache[key]


def _d(t):
    return None if t is None else t.to(DEV)


def _compare(got, want, dt, what, f32_bar=2e-5):
    got = got.float().cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "%s: NaN pattern differs from the reference's (%d vs %d elements)" % (
        what, int(torch.isnan(got).sum()), int(nan.sum()))
    assert bool((nan.all(dim=-1) == nan.any(dim=-1)).all())        # a NaN row is NaN in every element
    d = (got.double() - want)[~nan].abs()
    print("%s %s: max %.3e mean %.3e (%d NaN rows)" % (what, dt, d.max().item(), d.mean().item(), int(nan.all(dim=-1).sum())))
    if dt == torch.float32:
        assert d.max().item() < f32_bar
    else:      # P is rounded to bf16 before the PV product (2^-9 relative per element, averaged by the sum)
        assert d.max().item() < 1e-2 and d.mean().item() < 1e-3


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_float64(hip_lib, shape, case, dt):
    from far3d_amd import ops
    q, k, v, am, kp, want = _inputs(shape, case)
    got = ops.attention_batched(q.to(dt).to(DEV), k.to(dt).to(DEV), v.to(dt).to(DEV), H, attn_mask=_d(am), key_padding_mask=_d(kp))
    assert got.shape == q.shape and got.dtype == torch.float32
    if case == "full_row":
        assert bool(torch.isnan(want[dt][:, shape[1] // 2 + 1]).all())
    _compare(got, want[dt], dt, "%s %s" % (shape, case))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_300x333_masks_and_padding(hip_lib, dt):
    """Five query blocks, five key tiles and a tail of 13 keys; a per-(sample, head) bool mask plus key padding, then an f32 mask."""
    from far3d_amd import ops
    B, Aq, Nk = 2, 300, 333
    q, k, v, g = _data(B, Aq, Nk)
    am = torch.rand(B * H, Aq, Nk, generator=g) < 0.3
    kp = torch.rand(B, Nk, generator=g) < 0.25
    fm = (torch.rand(Aq, Nk, generator=g) * 8 - 4).masked_fill(torch.rand(Aq, Nk, generator=g) < 0.2, float("-inf"))
    qd, kd, vd = (t.to(dt).to(DEV) for t in (q, k, v))
    for what, a, p in (("bool3d + padding", am, kp), ("f32 + padding", fm, kp)):
        want = R.attention_ref(q.to(dt), k.to(dt), v.to(dt), H, a, p)
        _compare(ops.attention_batched(qd, kd, vd, H, attn_mask=_d(a), key_padding_mask=_d(p)), want, dt, "300x333 " + what)


@pytest.mark.parametrize("masked", [False, True])
def test_rescale_branch_forced_with_masked_spikes(hip_lib, masked):
    """The spike of test_attention_rescale_branch_forced (one key per query dominates and sits in a late tile, so the running max jumps);
    with `masked`, the spike key is excluded for every second row, whose maximum then must NOT jump."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(7)
    B, Aq, Nk = 2, 96, 400
    q, k, v = torch.randn(B, Aq, E, generator=g), torch.randn(B, Nk, E, generator=g), torch.randn(B, Nk, E, generator=g)
    am = torch.zeros(Aq, Nk, dtype=torch.bool)
    for i in range(Aq):
        k[:, 100 + 3 * i] += 3.0 * q[:, i]      # spike in tiles 1..6
        am[i, 100 + 3 * i] = masked and i % 2 == 1
    want = R.attention_ref(q, k, v, H, am)
    got = ops.attention_batched(q.to(DEV), k.to(DEV), v.to(DEV), H, attn_mask=am.to(DEV) if masked else None)
    _compare(got, want, torch.float32, "spike masked=%s" % masked, f32_bar=5e-5)


def test_strided_views_of_one_qkv_buffer(hip_lib):
    """q / k / v produced by one GEMM into a (B, rows, 768) buffer are consumed in place; the output lands in a view too."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(2, 200, 768, generator=g)
    buf[..., :256] *= 2.0
    am = torch.rand(150, 200, generator=g) < 0.3
    want = R.attention_ref(buf[:, :150, :256], buf[:, :, 256:512], buf[:, :, 512:], H, am)
    d = buf.to(DEV)
    obuf = torch.full((2, 160, 512), 7.0, device=DEV)
    got = ops.attention_batched(d[:, :150, :256], d[:, :, 256:512], d[:, :, 512:], H, attn_mask=am.to(DEV), out=obuf[:, :150, 256:])
    assert got.data_ptr() == obuf[:, :150, 256:].data_ptr()
    _compare(got, want, torch.float32, "strided views")
    assert bool((obuf[:, :, :256] == 7.0).all()) and bool((obuf[:, 150:] == 7.0).all())     # nothing outside the view is written


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["bool", "f32"])
def test_bits_of_a_sample_do_not_depend_on_the_batch(hip_lib, kind, dt):
    from far3d_amd import ops
    B, Aq, Nk = 3, 70, 130
    q, k, v, g = _data(B, Aq, Nk, seed=99)
    am = torch.rand(B * H, Aq, Nk, generator=g) < 0.3
    if kind == "f32":
        am = (torch.rand(B * H, Aq, Nk, generator=g) * 8 - 4).masked_fill(am, float("-inf"))
    kp = torch.rand(B, Nk, generator=g) < 0.2
    qd, kd, vd, amd, kpd = (t.to(DEV) for t in (q.to(dt), k.to(dt), v.to(dt), am, kp))
    full = ops.attention_batched(qd, kd, vd, H, attn_mask=amd, key_padding_mask=kpd)
    assert bool(torch.isfinite(full).all())
    for b in range(B):
        one = ops.attention_batched(qd[b:b + 1], kd[b:b + 1], vd[b:b + 1], H, attn_mask=amd[b * H:(b + 1) * H], key_padding_mask=kpd[b:b + 1])
        assert torch.equal(one[0], full[b]), "sample %d differs between its B = 1 call and the B = 3 call" % b


def test_bad_arguments_raise_and_launch_nothing(hip_lib):
    from far3d_amd import lib, ops
    B, Aq, Nk = 1, 37, 50
    q, k, v, _ = _data(B, Aq, Nk)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    out = torch.full((B, Aq, E), 7.0, device=DEV)
    with pytest.raises(lib.Far3dHipError, match="head_dim"):
        ops.attention_batched(qd, kd, vd, 4, out=out)                      # head_dim 64
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    mask = torch.zeros(Aq, Nk, dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(kind, ldm, mptr=None, B_=B, Aq_=Aq, Nk_=Nk, qp=None):
        return hip_lib.far3d_attention_batched(p(qd) if qp is None else qp, p(kd), p(vd), 0, p(out), 0, B_, Aq_, Nk_, H, 32, E, E, E, E, Aq * E, Nk * E, Nk * E,
                                               Aq * E, 32 ** -0.5, mptr or p(mask), kind, ldm, 0, None, st)
    for what, rc in (("ldm < Nk", raw(1, Nk - 1)), ("mask_kind 3", raw(3, Nk)), ("B < 1", raw(0, Nk, B_=0)), ("Aq < 1", raw(0, Nk, Aq_=0)),
                     ("Nk < 1", raw(0, Nk, Nk_=0)), ("null q", raw(0, Nk, qp=ctypes.c_void_p(0)))):
        assert rc == -1, what
        assert hip_lib.far3d_last_error(), what
        with pytest.raises(lib.Far3dHipError):
            lib.check(rc, what)
    assert raw(1, Nk) == 0 and raw(0, 0) == 0       # the same calls with good arguments run
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())
    out.fill_(7.0)
    for rc in (raw(1, Nk - 1), raw(3, Nk)):
        assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                  # a refused call launches nothing
    with pytest.raises(ValueError, match=r"\(37, 50\)"):
        ops.attention_batched(qd, kd, vd, H, attn_mask=torch.zeros(Aq, Nk + 1, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match=r"key_padding_mask must be \(1, 50\)"):
        ops.attention_batched(qd, kd, vd, H, key_padding_mask=torch.zeros(B, Nk + 1, dtype=torch.bool, device=DEV))
    with pytest.raises(TypeError):
        ops.attention_batched(qd, kd.bfloat16(), vd, H)

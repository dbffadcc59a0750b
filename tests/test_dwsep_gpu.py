"""GPU: far3d_dwsep_conv_nhwc (csrc/dwsep.hip), y = act2(W_pw . round_storage(act1(dw3x3(x; w9) + b1)) + b2) in one launch, on bf16 and
pair-stored maps.

1. The depthwise half, bitwise: with W_pw the identity (no b2, no act2) the output is far3d_dwconv3x3_act_nhwc's.  Multiplying by 1 and
   0 is exact, and in pair storage hi + lo is exact.  (One value of pair storage has two encodings when |lo| is exactly half an ulp of hi
   and hi's last bit is odd; the fused kernel re-splits the exact sum hi + lo, so there it writes the even-hi encoding of the same fp32
   value.  The pair comparison is therefore: the fp32 values are equal, and the stored bits are the split of that value.)
2. The pointwise half on exact integers: centre-tap depthwise weights, x in [-4, 4], the asymmetric W_pw[o][c] = ((3o + 5c) % 5) - 2 and
   an integer b2 -- every fp32 sum is exact, so the output is the integer result rounded once to storage and equals ops.conv2d_nhwc's,
   bit for bit.  A transposed or permuted MFMA lane map cannot pass.
3. Random data against float64.  The intermediate a comes from ops.dwconv3x3_act_nhwc (test 1 proves it is the MFMA operand); the
   reference is the float64 1x1 on a + b2 + act2.  Bound per element, S = sum_c |a_c||w_c| + |b2|:
     bf16  2 K 2^-24 S  (at most K additions of relative error <= 2^-23 on partial sums <= S; products of bf16 operands are exact in fp32)
     pair  tests/test_pair_gpu.py::_bound(K, a, w)[0], the project's bound for split products
     + 2^-8 |y| (bf16 output) or 2^-16 |y| (pair output); Swish as act2: 1.1 x the bound + chain_bound, as tests/test_dwconv_act_gpu.py.
4. Channel-slice views (ldx > C, ldy > Cout) leave every byte outside the slice alone; a batch of two is 1 + 1 bit for bit.
5. Refusals raise Far3dHipError and write nothing."""
import functools

import pytest
import torch

from tests.head_refs import chain_bound
from tests.test_dwconv_gpu import _load, _round_storage, _store, _weights
from tests.test_pair_gpu import _bound as _pair_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (N, H, W, C, Cout, stride)
SHAPES = [(1, 1, 1, 32, 32, 1), (1, 2, 3, 64, 64, 2), (2, 5, 7, 64, 32, 1), (1, 3, 9, 160, 160, 1), (1, 9, 12, 96, 224, 2),
          (1, 4, 17, 256, 256, 1), (1, 8, 33, 128, 128, 1)]
DTS = ("bf16", "pair")
ACTS = (None, "relu", "swish")
CASES = [(s, dt) for s in SHAPES for dt in DTS]
IDS = ["%s-%s" % ("x".join(map(str, s)), dt) for s, dt in CASES]


def _pc(w, b, dt):
    """The 1x1 PackedConv the engine would hold for this storage: bf16 weights, or split fp32 weights for pair-stored maps."""
    from far3d_amd import ops
    if dt == "bf16":
        return ops.PackedConv(w, b, dtype=torch.bfloat16, device=DEV)
    return ops.PackedConv(w, b, dtype=torch.float32, device=DEV, compute="bf16x3")


@functools.lru_cache(maxsize=None)
def _case(shape, dt, seed=0):
    """x, depthwise weights (C,1,3,3), b1 (C,), pointwise weights (Cout,C) and b2 (Cout,), x and the pointwise weights rounded to what
    the storage holds -- built once per (shape, dt), never modified."""
    N, H, W, C, Cout, stride = shape
    g = torch.Generator().manual_seed(seed + 17 * C + 3 * Cout + H)
    x = _round_storage(torch.randn(N, H, W, C, generator=g), dt)
    w = _weights(C, g)
    b1 = (torch.randn(C, generator=g) * 0.5).float()
    wp = _round_storage(torch.randn(Cout, C, generator=g) * (2.0 / C) ** 0.5, dt)
    b2 = (torch.randn(Cout, generator=g) * 0.5).float()
    return x, w, b1, wp, b2


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_depthwise_half_is_dwconv3x3_act_bitwise(hip_lib, shape, dt):
    from far3d_amd import ops
    N, H, W, C, _, stride = shape
    x, w, b1, _, _ = _case(shape, dt)
    xs, w9, b1d = _store(x, dt), ops.pack_dw3x3(w, DEV), b1.to(DEV)
    eye = _pc(torch.eye(C), None, dt)
    pair = dt == "pair"
    for act in ACTS:
        for bias in (None, b1d):
            want = ops.dwconv3x3_act_nhwc(xs, w9, stride, bias=bias, act=act, pair=pair)
            got = ops.dwsep_conv_nhwc(xs, w9, eye, stride, bias1=bias, act1=act, pair=pair)
            torch.cuda.synchronize()
            tag = "%s %s act1 %s bias %s" % (shape, dt, act, bias is not None)
            assert got.shape == want.shape and got.dtype == want.dtype, tag
            if pair:
                assert torch.equal(ops.pair_to_float(got), ops.pair_to_float(want)), tag
                assert torch.equal(_bits(got.cpu()), _bits(ops.pair_from_float(ops.pair_to_float(want.cpu())))), tag
                print("%s: %d of %d stored words are the other encoding" % (tag, int((_bits(got) != _bits(want)).sum()), got.numel()))
            else:
                assert torch.equal(_bits(got), _bits(want)), tag


@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
def test_pointwise_half_exact_integers(hip_lib, shape, dt):
    from far3d_amd import ops
    N, H, W, C, Cout, stride = shape
    g = torch.Generator().manual_seed(5 + C + Cout)
    x = torch.randint(-4, 5, (N, H, W, C), generator=g).float()
    centre = torch.zeros(C, 1, 3, 3)
    centre[:, 0, 1, 1] = 1.0
    o, c = torch.arange(Cout)[:, None], torch.arange(C)[None, :]
    wp = (((3 * o + 5 * c) % 5) - 2).float()
    b2 = torch.randint(-9, 10, (Cout,), generator=g).float()
    pc = _pc(wp, b2, dt)
    pair = dt == "pair"
    got = ops.dwsep_conv_nhwc(_store(x, dt), ops.pack_dw3x3(centre, DEV), pc, stride, pair=pair)
    xsub = x[:, ::stride, ::stride].contiguous()                       # the pixels the centre tap of a stride-s window picks
    conv = ops.conv2d_nhwc(_store(xsub, dt), pc)
    torch.cuda.synchronize()
    want = xsub.double() @ wp.double().t() + b2.double()              # integers below 2^24: exact in fp32 in any order
    assert float(want.abs().max()) < 2 ** 24
    assert tuple(got.shape) == (N, (H - 1) // stride + 1, (W - 1) // stride + 1, Cout * (2 if pair else 1))
    assert torch.equal(_bits(got.cpu()), _bits(_store(want.float(), dt).cpu())), "integer result rounded once to storage"
    assert torch.equal(_bits(got), _bits(conv)), "ops.conv2d_nhwc on the same integers"


CFGS = [(None, False, "relu"), ("swish", True, "swish"), ("relu", True, None)]      # (act1, b1, act2): backbone, towers, a third mix


@pytest.mark.parametrize("shape,dt", CASES, ids=IDS)
@pytest.mark.parametrize("cfg", CFGS, ids=["none-relu", "swish-b1-swish", "relu-b1-none"])
def test_matches_float64_on_its_own_intermediate(hip_lib, shape, dt, cfg):
    from far3d_amd import ops
    N, H, W, C, Cout, stride = shape
    act1, use_b1, act2 = cfg
    x, w, b1, wp, b2 = _case(shape, dt)
    xs, w9 = _store(x, dt), ops.pack_dw3x3(w, DEV)
    b1d = b1.to(DEV) if use_b1 else None
    pair = dt == "pair"
    a = _load(ops.dwconv3x3_act_nhwc(xs, w9, stride, bias=b1d, act=act1, pair=pair), dt)        # the MFMA operand (test 1)
    got = _load(ops.dwsep_conv_nhwc(xs, w9, _pc(wp, b2, dt), stride, bias1=b1d, act1=act1, act2=act2, pair=pair), dt)
    pre = a.double() @ wp.double().t() + b2.double()
    S = a.double().abs() @ wp.double().abs().t() + b2.double().abs()
    K = C
    bound = 2 * K * 2.0 ** -24 * S if dt == "bf16" else torch.full_like(S, _pair_bound(K, a, wp)[0])
    if act2 == "relu":
        y = pre.clamp(min=0)
    elif act2 == "swish":
        y = pre * torch.sigmoid(pre)
        p32 = pre.float()
        bound = 1.1 * bound + chain_bound(float(((p32 * torch.sigmoid(p32)).double() - y).abs().max()), y)
    else:
        y = pre
    bound = bound + (2.0 ** -8 if dt == "bf16" else 2.0 ** -16) * y.abs()
    assert tuple(got.shape) == tuple(y.shape)
    err = (got.double() - y).abs()
    worst = float((err / bound.clamp(min=1e-300)).max())
    print("dwsep %s %s %s: max err %.3e, worst err / bound %.3f" % (shape, dt, cfg, float(err.max()), worst))
    assert bool((err <= bound).all()), "%d elements over the bound (worst %.3f x)" % (int((err > bound).sum()), worst)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("stride", [1, 2])
def test_channel_slices_keep_their_neighbours_and_batch_is_one_plus_one(hip_lib, dt, stride):
    from far3d_amd import ops
    shape = (2, 6, 9, 64, 96, stride)
    N, H, W, C, Cout, _ = shape
    x, w, b1, wp, b2 = _case(shape, dt, seed=3)
    cs = 2 if dt == "pair" else 1
    pair = dt == "pair"
    xs, w9, b1d, pc = _store(x, dt), ops.pack_dw3x3(w, DEV), b1.to(DEV), _pc(wp, b2, dt)
    call = lambda xin, out=None: ops.dwsep_conv_nhwc(xin, w9, pc, stride, bias1=b1d, act1="swish", act2="swish", out=out, pair=pair)
    dense = call(xs)
    Ho, Wo = dense.shape[1], dense.shape[2]
    xin = torch.zeros((N, H, W, (32 + C + 32) * cs), dtype=xs.dtype, device=DEV)
    xin[..., 32 * cs:(32 + C) * cs] = xs
    xin[..., :32 * cs] = 7.0          # neighbours that must not be read as part of the window
    xin[..., (32 + C) * cs:] = -5.0
    out = torch.full((N, Ho, Wo, (64 + Cout + 32) * cs), 3.0, dtype=xs.dtype, device=DEV)
    before = out.clone()
    dst = out[..., 64 * cs:(64 + Cout) * cs]
    r = call(xin[..., 32 * cs:(32 + C) * cs], dst)
    torch.cuda.synchronize()
    assert r.data_ptr() == dst.data_ptr()
    assert torch.equal(_bits(dst), _bits(dense))
    assert torch.equal(out[..., :64 * cs], before[..., :64 * cs]) and torch.equal(out[..., (64 + Cout) * cs:], before[..., (64 + Cout) * cs:])
    for n in range(N):
        one = call(xs[n:n + 1].contiguous())
        assert torch.equal(_bits(one[0]), _bits(dense[n])), "image %d" % n
    # input and output as disjoint channel slices of ONE buffer (an OSA concat buffer) are no overlap
    if stride == 1:
        cat = torch.zeros((N, H, W, (C + Cout) * cs), dtype=xs.dtype, device=DEV)
        cat[..., :C * cs] = xs
        call(cat[..., :C * cs], cat[..., C * cs:])
        torch.cuda.synchronize()
        assert torch.equal(_bits(cat[..., C * cs:]), _bits(dense)) and torch.equal(_bits(cat[..., :C * cs]), _bits(xs))


def test_refusals_raise_and_write_nothing(hip_lib):
    from far3d_amd import ops
    from far3d_amd.lib import Far3dHipError
    bf, nan = torch.bfloat16, float("nan")

    def refuse(x, C, Cout, stride, out, dt="bf16", what="", pc=None):
        w9 = torch.ones((9, C), device=DEV)
        pc = pc or _pc(torch.ones(Cout, C), torch.ones(Cout), dt)
        with pytest.raises(Far3dHipError):
            ops.dwsep_conv_nhwc(x, w9, pc, stride, out=out, pair=dt == "pair")
        torch.cuda.synchronize()
        assert bool(torch.isnan(out.float()).all()), "%s: the refused call wrote to its output" % what

    z = lambda *s, dtype=bf: torch.zeros(s, dtype=dtype, device=DEV)
    f = lambda *s, dtype=bf: torch.full(s, nan, dtype=dtype, device=DEV)
    refuse(z(1, 4, 4, 48), 48, 64, 1, f(1, 4, 4, 64), what="C = 48")
    refuse(z(1, 4, 4, 96), 48, 64, 1, f(1, 4, 4, 128), dt="pair", what="C = 48 (pair)")
    refuse(z(1, 4, 4, 64), 64, 288, 1, f(1, 4, 4, 288), what="Cout = 288")
    refuse(z(1, 4, 4, 64), 64, 40, 1, f(1, 4, 4, 40), what="Cout = 40")
    refuse(z(1, 6, 6, 64), 64, 64, 3, f(1, 2, 2, 64), what="stride 3")
    # f32 storage: fp32 maps with fp32 weights, and with split weights (the bf16x3_f32act mode's operands)
    refuse(z(1, 4, 4, 64, dtype=torch.float32), 64, 64, 1, f(1, 4, 4, 64, dtype=torch.float32), what="f32 storage",
           pc=ops.PackedConv(torch.ones(64, 64), None, dtype=torch.float32, device=DEV))
    refuse(z(1, 4, 4, 64, dtype=torch.float32), 64, 64, 1, f(1, 4, 4, 64, dtype=torch.float32), what="f32 storage, split weights",
           pc=_pc(torch.ones(64, 64), None, "pair"))
    # misaligned pointers: a channel slice that starts 4 channels (8 bytes) in, on the input and on the output side
    wide = z(1, 4, 4, 72)
    refuse(wide[..., 4:68], 64, 64, 1, f(1, 4, 4, 64), what="misaligned input")
    owide = f(1, 4, 4, 72)
    refuse(z(1, 4, 4, 64), 64, 64, 1, owide[..., 4:68], what="misaligned output")
    assert bool(torch.isnan(owide.float()).all())
    # overlap: in place, and channel slices of one buffer that share channels
    buf = f(1, 4, 4, 64)
    refuse(buf, 64, 64, 1, buf, what="in place")
    buf = f(1, 4, 4, 96)
    refuse(buf[..., :64], 64, 64, 1, buf[..., 32:], what="overlapping channel slices")
    assert bool(torch.isnan(buf.float()).all())

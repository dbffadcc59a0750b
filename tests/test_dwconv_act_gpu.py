"""GPU: far3d_dwconv3x3_act_nhwc (depthwise 3x3 + folded-BN bias + activation, one or two weight sets per window; csrc/dwconv.hip)
against F.conv2d(groups=C) + bias + activation in float64 on the CPU.

Inputs are rounded to the storage type first, as tests/test_dwconv_gpu.py does.  Bounds per element, with S = sum |x w| over the nine taps:
  pre-activation   16 * 2^-24 * (S + |b|)       that file's bound with the bias as a tenth term
  ReLU             the same                      (|relu(a) - relu(b)| <= |a - b|)
  Swish            1.1 x the pre-activation bound (|d swish / dx| <= 1.1) + what tests/test_glue_gpu.py grants a chain through expf:
                   4 x (the float32 restatement's own distance from float64 on the same inputs) + 2 ulp of the largest output
  output storage   + 2^-8 |y| for bf16, + 2^-16 |y| for pair
Bitwise: reps = 1 / no bias / no activation is far3d_dwconv3x3_nhwc; each half of a two-set call is the single-set call with that set;
a batch of two is 1 + 1; channel-slice views leave every byte outside the slice alone."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.head_refs import chain_bound
from tests.test_dwconv_gpu import _load, _round_storage, _store, _weights

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (1,3,9,8,1): a run of 8 plus a tail of one at the smallest channel count; (1,4,17,256,1): two full runs plus a tail at the tower width
SHAPES = [(1, 1, 1, 64, 1), (1, 2, 3, 96, 2), (2, 5, 7, 64, 1), (1, 3, 9, 8, 1), (1, 9, 12, 80, 2), (1, 4, 17, 256, 1)]
DTS = ("f32", "bf16", "pair")
ACTS = (None, "relu", "swish")
CASES = [(s, dt, reps, act, bias) for s in SHAPES for dt in DTS if dt != "pair" or s[3] % 32 == 0
         for reps in (1, 2) for act in ACTS for bias in (False, True)]


def _id(c):
    s, dt, reps, act, bias = c
    return "%s-%s-r%d-%s-%s" % ("x".join(map(str, s)), dt, reps, act or "none", "bias" if bias else "nobias")


@functools.lru_cache(maxsize=None)
def _case(shape, dt, seed=0):
    """x (rounded to the storage type), two weight sets (C,1,3,3) and two biases (C,) -- built once per (shape, dt), never modified."""
    N, H, W, C, stride = shape
    g = torch.Generator().manual_seed(seed + 17 * C + H)
    x = _round_storage(torch.randn(N, H, W, C, generator=g), dt)
    ws = (_weights(C, g), _weights(C, g).flip(2))
    bs = ((torch.randn(C, generator=g) * 0.5).float(), (torch.randn(C, generator=g) * 0.5 + 0.25).float())
    return x, ws, bs


def _reference(x, ws, bs, stride, act, reps, bias):
    """float64 result (N,Ho,Wo,reps*C), the pre-activation bound's magnitude S + |b|, and the float32 restatement's yardstick."""
    xd = x.double().permute(0, 3, 1, 2)
    ys, mags = [], []
    for r in range(reps):
        wd = ws[r].double()
        C = wd.shape[0]
        y = F.conv2d(xd, wd, bs[r].double() if bias else None, stride, 1, 1, C)
        S = F.conv2d(xd.abs(), wd.abs(), bs[r].double().abs() if bias else None, stride, 1, 1, C)
        ys.append(y.permute(0, 2, 3, 1))
        mags.append(S.permute(0, 2, 3, 1))
    pre, mag = torch.cat(ys, -1), torch.cat(mags, -1)
    yard = 0.0
    if act == "relu":
        y = pre.clamp(min=0)
    elif act == "swish":
        y = pre * torch.sigmoid(pre)
        p32 = pre.float()
        yard = float(((p32 * torch.sigmoid(p32)).double() - y).abs().max())
    else:
        y = pre
    return y, mag, yard


def _bound(y, mag, yard, act, dt):
    b = 16 * 2.0 ** -24 * mag
    if act == "swish":
        b = 1.1 * b + chain_bound(yard, y)
    if dt == "bf16":
        b = b + 2.0 ** -8 * y.abs()
    if dt == "pair":
        b = b + 2.0 ** -16 * y.abs()
    return b


def _call(x, ws, bs, stride, act, reps, bias, dt, out=None, xs=None):
    from far3d_amd import ops
    w, b = ops.pack_dw3x3_sets(list(ws[:reps]), list(bs[:reps]) if bias else None, DEV)
    return ops.dwconv3x3_act_nhwc(_store(x, dt) if xs is None else xs, w, stride, bias=b, act=act, out=out, pair=dt == "pair")


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_dwconv_act_matches_float64(hip_lib, case):
    shape, dt, reps, act, bias = case
    x, ws, bs = _case(shape, dt)
    stride = shape[4]
    got = _call(x, ws, bs, stride, act, reps, bias, dt)
    torch.cuda.synchronize()
    cs = 2 if dt == "pair" else 1
    C = shape[3]
    assert got.shape[-1] == reps * C * cs
    y, mag, yard = _reference(x, ws, bs, stride, act, reps, bias)
    # pair storage keeps every set's C logical channels as C*2 stored ones, set after set (C % 32 == 0)
    g = torch.cat([_load(got[..., r * C * cs:(r + 1) * C * cs].contiguous(), dt) for r in range(reps)], -1)
    assert tuple(g.shape) == tuple(y.shape), (g.shape, y.shape)
    err = (g.double() - y).abs()
    bound = _bound(y, mag, yard, act, dt)
    worst = float((err / bound.clamp(min=1e-300)).max())
    print("%s: max err %.3e, worst err / bound %.3f" % (_id(case), float(err.max()), worst))
    assert bool((err <= bound).all()), "%s: %d elements over the bound (worst %.3f x)" % (_id(case), int((err > bound).sum()), worst)


PLAIN = [(s, dt) for s in SHAPES for dt in DTS if dt != "pair" or s[3] % 32 == 0]


@pytest.mark.parametrize("shape,dt", PLAIN, ids=["%s-%s" % ("x".join(map(str, s)), d) for s, d in PLAIN])
def test_plain_call_is_dwconv3x3_nhwc_bitwise(hip_lib, shape, dt):
    from far3d_amd import ops
    x, ws, bs = _case(shape, dt)
    xs = _store(x, dt)
    for r in range(2):
        want = ops.dwconv3x3_nhwc(xs, ops.pack_dw3x3(ws[r], DEV), shape[4], pair=dt == "pair")
        got = ops.dwconv3x3_act_nhwc(xs, ops.pack_dw3x3(ws[r], DEV), shape[4], pair=dt == "pair")       # a (9,C) tensor is one set
        assert torch.equal(got, want), "set %d" % r


@pytest.mark.parametrize("shape,dt", PLAIN, ids=["%s-%s" % ("x".join(map(str, s)), d) for s, d in PLAIN])
@pytest.mark.parametrize("act", ACTS)
def test_two_sets_are_two_single_sets_bitwise(hip_lib, shape, dt, act):
    x, ws, bs = _case(shape, dt)
    xs = _store(x, dt)
    for bias in (False, True):
        both = _call(x, ws, bs, shape[4], act, 2, bias, dt, xs=xs)
        half = both.shape[-1] // 2
        for r in range(2):
            one = _call(x, ws[r:], bs[r:], shape[4], act, 1, bias, dt, xs=xs)
            assert torch.equal(both[..., r * half:(r + 1) * half], one), "set %d bias %s" % (r, bias)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("reps", [1, 2])
def test_batch_of_two_is_one_plus_one_bitwise(hip_lib, dt, stride, reps):
    x, ws, bs = _case((2, 5, 11, 96, stride), dt, seed=5)
    xs = _store(x, dt)
    full = _call(x, ws, bs, stride, "swish", reps, True, dt, xs=xs)
    for n in range(2):
        one = _call(x, ws, bs, stride, "swish", reps, True, dt, xs=xs[n:n + 1].contiguous())
        assert torch.equal(one[0], full[n]), "image %d" % n


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("reps", [1, 2])
def test_channel_slices_keep_their_neighbours(hip_lib, dt, reps):
    """Input read from, and output written into, channel slices of wider buffers: the result is the dense call's, bit for bit, and every
    byte outside the output slice stays."""
    N, H, W, C, stride = 2, 6, 9, 64, 1
    x, ws, bs = _case((N, H, W, C, stride), dt, seed=3)
    cs = 2 if dt == "pair" else 1
    xs = _store(x, dt)
    xin = torch.zeros((N, H, W, (32 + C + 16) * cs), dtype=xs.dtype, device=DEV)
    xin[..., 32 * cs:(32 + C) * cs] = xs
    xin[..., :32 * cs] = 7.0          # neighbours that must not be read as part of the window
    xin[..., (32 + C) * cs:] = -5.0
    Co = reps * C
    out = torch.full((N, H, W, (64 + Co + 32) * cs), 3.0, dtype=xs.dtype, device=DEV)
    before = out.clone()
    dst = out[..., 64 * cs:(64 + Co) * cs]
    r = _call(x, ws, bs, stride, "swish", reps, True, dt, out=dst, xs=xin[..., 32 * cs:(32 + C) * cs])
    dense = _call(x, ws, bs, stride, "swish", reps, True, dt, xs=xs)
    torch.cuda.synchronize()
    assert r.data_ptr() == dst.data_ptr()
    assert torch.equal(dst, dense)
    assert torch.equal(out[..., :64 * cs], before[..., :64 * cs]) and torch.equal(out[..., (64 + Co) * cs:], before[..., (64 + Co) * cs:])


def test_bad_arguments_launch_nothing(hip_lib):
    from far3d_amd import ops
    from far3d_amd.lib import Far3dHipError
    nan = float("nan")
    bf = torch.bfloat16

    def refuse(x, C, out, reps=1, act=None, pair=False, what=""):
        w = torch.ones((reps, 9, C), device=DEV)
        b = torch.ones((reps, C), device=DEV)
        with pytest.raises(Far3dHipError):
            ops.dwconv3x3_act_nhwc(x, w, 1, bias=b, act=act, out=out, pair=pair)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out.float()).all()), "%s: the refused call wrote to its output" % what

    # misaligned rows: a bf16 channel slice that starts 4 channels (8 bytes) in, on the input and on the output side
    wide = torch.zeros((1, 4, 4, 24), dtype=bf, device=DEV)
    refuse(wide[..., 4:20], 16, torch.full((1, 4, 4, 16), nan, dtype=bf, device=DEV), what="misaligned input")
    owide = torch.full((1, 4, 4, 40), nan, dtype=bf, device=DEV)
    refuse(torch.zeros((1, 4, 4, 16), dtype=bf, device=DEV), 16, owide[..., 4:36], reps=2, what="misaligned output")
    assert bool(torch.isnan(owide.float()).all())
    # a pixel stride that is no multiple of 16 bytes (fp32 rows of 18 floats)
    wide = torch.zeros((1, 4, 4, 18), device=DEV)
    refuse(wide[..., :16], 16, torch.full((1, 4, 4, 16), nan, device=DEV), what="misaligned pixel stride")
    # a misaligned bias: one float into its buffer
    x = torch.zeros((1, 4, 4, 16), device=DEV)
    out = torch.full((1, 4, 4, 16), nan, device=DEV)
    with pytest.raises(Far3dHipError):
        ops.dwconv3x3_act_nhwc(x, torch.ones((1, 9, 16), device=DEV), 1, bias=torch.ones(20, device=DEV)[1:17].view(1, 16), out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    # three weight sets, an unknown activation
    refuse(torch.zeros((1, 4, 4, 16), device=DEV), 16, torch.full((1, 4, 4, 48), nan, device=DEV), reps=3, what="reps=3")
    refuse(torch.zeros((1, 4, 4, 16), device=DEV), 16, torch.full((1, 4, 4, 16), nan, device=DEV), act=3, what="act=3")
    # pair storage with C % 32
    refuse(torch.zeros((1, 4, 4, 96), dtype=bf, device=DEV), 48, torch.full((1, 4, 4, 96), nan, dtype=bf, device=DEV), pair=True,
           what="pair C % 32")

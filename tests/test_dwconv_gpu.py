"""GPU: far3d_dwconv3x3_nhwc (depthwise 3x3, pad 1, stride 1 | 2; csrc/dwconv.hip) against F.conv2d(groups=C) in float64 on the CPU.

The inputs are rounded to the storage type under test first (bf16, or the 16 significant bits of pair storage), so that only the
kernel's accumulation and its output rounding count.  Bound per element, with S = sum |x w| over the nine taps in float64:
16 * 2^-24 * S (nine products and eight additions in any order, fused or not: gamma_9 < 16 u), plus 2^-8 |y| for a bf16 output and
2^-16 |y| for a pair output.  Every tap and every channel has its own weight, so a transposed or mirrored window fails."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 5, 7, 64, 1), (1, 9, 12, 80, 2), (2, 8, 8, 112, 1), (1, 7, 5, 224, 2), (1, 2, 3, 96, 2), (1, 1, 1, 64, 1)]
CASES = [(s, dt) for s in SHAPES for dt in ("f32", "bf16", "pair") if dt != "pair" or s[3] % 32 == 0]


def _round_storage(x, dt):
    """fp32 values as the storage type holds them (exactly representable there)."""
    from far3d_amd import ops
    if dt == "f32":
        return x
    if dt == "bf16":
        return x.to(torch.bfloat16).float()
    return ops.pair_to_float(ops.pair_from_float(x))


def _store(x, dt):
    """NHWC fp32 values (already rounded) -> the stored tensor on the device."""
    from far3d_amd import ops
    if dt == "f32":
        return x.to(DEV)
    if dt == "bf16":
        return x.to(torch.bfloat16).to(DEV)
    return ops.pair_from_float(x).to(DEV)


def _load(y, dt):
    from far3d_amd import ops
    y = y.cpu()
    return ops.pair_to_float(y) if dt == "pair" else y.float()


def _weights(C, g):
    """(C,1,3,3): a different value per tap and per channel, signs mixed, nothing symmetric."""
    base = torch.tensor([[0.9, -0.35, 0.2], [-0.6, 1.1, 0.45], [0.15, -0.8, 0.55]])
    return (base[None, None] * (1.0 + 0.5 * torch.rand(C, 1, 3, 3, generator=g)) + 0.05 * torch.randn(C, 1, 3, 3, generator=g)).float()


def _reference(x, w, stride):
    """float64 result (N,Ho,Wo,C) and S = sum |x w| per element."""
    xd, wd = x.double().permute(0, 3, 1, 2), w.double()
    y = F.conv2d(xd, wd, None, stride, 1, 1, w.shape[0])
    S = F.conv2d(xd.abs(), wd.abs(), None, stride, 1, 1, w.shape[0])
    return y.permute(0, 2, 3, 1), S.permute(0, 2, 3, 1)


def _bound(y, S, dt):
    b = 16 * 2.0 ** -24 * S
    if dt == "bf16":
        b = b + 2.0 ** -8 * y.abs()
    if dt == "pair":
        b = b + 2.0 ** -16 * y.abs()
    return b


def _case(shape, dt, seed=0):
    N, H, W, C, stride = shape
    g = torch.Generator().manual_seed(seed + 17 * C + H)
    x = _round_storage(torch.randn(N, H, W, C, generator=g), dt)
    w = _weights(C, g)
    return x, w


def _check(got, x, w, stride, dt, tag):
    y, S = _reference(x, w, stride)
    assert tuple(got.shape) == tuple(y.shape), (tag, got.shape, y.shape)
    err = (got.double() - y).abs()
    bound = _bound(y, S, dt)
    worst = float((err / bound.clamp(min=1e-300)).max())
    print("%s: max err %.3e, worst err / bound %.3f" % (tag, float(err.max()), worst))
    assert bool((err <= bound).all()), "%s: %d elements over the bound (worst %.3f x)" % (tag, int((err > bound).sum()), worst)


@pytest.mark.parametrize("shape,dt", CASES, ids=["%s-%s" % ("x".join(map(str, s)), d) for s, d in CASES])
def test_dwconv_matches_float64(hip_lib, shape, dt):
    from far3d_amd import ops
    x, w = _case(shape, dt)
    stride = shape[4]
    got = ops.dwconv3x3_nhwc(_store(x, dt), ops.pack_dw3x3(w, DEV), stride, pair=dt == "pair")
    torch.cuda.synchronize()
    _check(_load(got, dt), x, w, stride, dt, "dwconv %s %s" % (shape, dt))


@pytest.mark.parametrize("dt", ["f32", "bf16", "pair"])
def test_dwconv_channel_slices_of_wider_buffers(hip_lib, dt):
    """Input read from, and output written into, channel slices of wider buffers; every byte outside the output slice stays."""
    from far3d_amd import ops
    N, H, W, C, stride = 2, 6, 9, 64, 1
    x, w = _case((N, H, W, C, stride), dt, seed=3)
    cs = 2 if dt == "pair" else 1
    xs = _store(x, dt)
    xin = torch.zeros((N, H, W, (32 + C + 16) * cs), dtype=xs.dtype, device=DEV)
    xin[..., 32 * cs:(32 + C) * cs] = xs
    xin[..., :32 * cs] = 7.0          # neighbours that must not be read as part of the window
    xin[..., (32 + C) * cs:] = -5.0
    out = torch.full((N, H, W, (64 + C + 32) * cs), 3.0, dtype=xs.dtype, device=DEV)
    before = out.clone()
    dst = out[..., 64 * cs:(64 + C) * cs]
    r = ops.dwconv3x3_nhwc(xin[..., 32 * cs:(32 + C) * cs], ops.pack_dw3x3(w, DEV), stride, out=dst, pair=dt == "pair")
    torch.cuda.synchronize()
    assert r.data_ptr() == dst.data_ptr()
    _check(_load(dst.contiguous(), dt), x, w, stride, dt, "slices %s" % dt)
    assert torch.equal(out[..., :64 * cs], before[..., :64 * cs]) and torch.equal(out[..., (64 + C) * cs:], before[..., (64 + C) * cs:])


@pytest.mark.parametrize("dt", ["f32", "bf16", "pair"])
@pytest.mark.parametrize("stride", [1, 2])
def test_dwconv_batch_independent(hip_lib, dt, stride):
    """Image n computed alone equals image n computed in a batch of 3, bit for bit."""
    from far3d_amd import ops
    x, w = _case((3, 7, 10, 96, stride), dt, seed=5)
    w9 = ops.pack_dw3x3(w, DEV)
    xs = _store(x, dt)
    full = ops.dwconv3x3_nhwc(xs, w9, stride, pair=dt == "pair")
    for n in range(3):
        one = ops.dwconv3x3_nhwc(xs[n:n + 1].contiguous(), w9, stride, pair=dt == "pair")
        assert torch.equal(one[0], full[n]), "image %d (%s, stride %d)" % (n, dt, stride)


def test_dwconv_bad_arguments_launch_nothing(hip_lib):
    from far3d_amd import ops
    from far3d_amd.lib import Far3dHipError
    nan = float("nan")

    def refuse(x, C, stride, out, pair=False, what=""):
        w9 = torch.ones((9, C), device=DEV)
        with pytest.raises(Far3dHipError):
            ops.dwconv3x3_nhwc(x, w9, stride, out=out, pair=pair)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out.float()).all()), "%s: the refused call wrote to its output" % what

    bf = torch.bfloat16
    # C % 8
    refuse(torch.zeros((1, 4, 4, 12), device=DEV), 12, 1, torch.full((1, 4, 4, 12), nan, device=DEV), what="C % 8")
    refuse(torch.zeros((1, 4, 4, 4), dtype=bf, device=DEV), 4, 1, torch.full((1, 4, 4, 4), nan, dtype=bf, device=DEV), what="C % 8 (bf16)")
    # a stride other than 1 or 2
    for s in (0, 3):
        refuse(torch.zeros((1, 6, 6, 16), device=DEV), 16, s, torch.full((1, 2, 2, 16), nan, device=DEV), what="stride %d" % s)
    # misaligned rows: a bf16 channel slice that starts 4 channels (8 bytes) in, on the input and on the output side
    wide = torch.zeros((1, 4, 4, 24), dtype=bf, device=DEV)
    refuse(wide[..., 4:20], 16, 1, torch.full((1, 4, 4, 16), nan, dtype=bf, device=DEV), what="misaligned input")
    owide = torch.full((1, 4, 4, 24), nan, dtype=bf, device=DEV)
    refuse(torch.zeros((1, 4, 4, 16), dtype=bf, device=DEV), 16, 1, owide[..., 4:20], what="misaligned output")
    assert bool(torch.isnan(owide.float()).all())
    # a pixel stride that is no multiple of 16 bytes (fp32 rows of 18 floats)
    wide = torch.zeros((1, 4, 4, 18), device=DEV)
    refuse(wide[..., :16], 16, 1, torch.full((1, 4, 4, 16), nan, device=DEV), what="misaligned pixel stride")
    # pair storage with C % 32
    refuse(torch.zeros((1, 4, 4, 96), dtype=bf, device=DEV), 48, 1, torch.full((1, 4, 4, 96), nan, dtype=bf, device=DEV), pair=True,
           what="pair C % 32")
    # Ho / Wo that do not match
    refuse(torch.zeros((1, 5, 7, 16), device=DEV), 16, 1, torch.full((1, 5, 6, 16), nan, device=DEV), what="Wo")
    refuse(torch.zeros((1, 5, 7, 16), device=DEV), 16, 2, torch.full((1, 2, 4, 16), nan, device=DEV), what="Ho")

"""GPU: far3d_attention_streams (csrc/attn.hip, ops.attention_streams) -- the engine's attention kernel for B samples in one launch.
The contract is bitwise: out[b] is far3d_attention_forward on sample b's operands and hole_count[b], whatever B is.  An independent
statement too: every sample against the float64 restatement tests/attn_refs.py at the bars tests/test_attn_norm_gpu.py holds
far3d_attention_forward to on the same kind of data (randn, q * 2): fp32 2e-5 max, bf16 1e-2 max and 1e-3 mean.
heads = 2 (E = 64), B = 3 independent samples.  Shapes (Aq, Nk): one partial query block with one partial key tile; two query blocks
with three 64-key tiles over the four key parts of a workgroup (one part has no tile); q / k / v as column blocks of one
(B, 300, 2 * 3 * 64) buffer with q the first 150 rows (row and batch strides)."""
import ctypes

import pytest
import torch

from tests import attn_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, E, B = 2, 64, 3
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["f32", "bf16"]
_cache = {}


def _data(Aq, Nk):
    if (Aq, Nk) not in _cache:
        g = torch.Generator().manual_seed(10 * Aq + Nk)
        q, k, v = (torch.randn(B, n, E, generator=g) for n in (Aq, Nk, Nk))
        _cache[(Aq, Nk)] = (q * 2.0, k, v)      # q * 2: a softmax peaky enough to exercise the running-max rescale
    return _cache[(Aq, Nk)]


def _equal_per_sample(ops, q, k, v, odt, hole=None):
    """The B = 3 launch, each sample's one-sample launch and each sample's batch-of-one launch: the same bits.  -> the B = 3 result."""
    full = ops.attention_streams(q, k, v, H, out_dtype=odt, hole=hole)
    assert full.shape == q.shape and full.dtype == odt and bool(torch.isfinite(full.float()).all())
    for b in range(B):
        hb = None if hole is None else (hole[0][b:b + 1], hole[1], hole[2])
        one = ops.attention_forward(q[b], k[b], v[b], H, out_dtype=odt, hole=hb)
        assert torch.equal(full[b], one), "sample %d of the B = %d launch differs from far3d_attention_forward" % (b, B)
        single = ops.attention_streams(q[b:b + 1], k[b:b + 1], v[b:b + 1], H, out_dtype=odt, hole=hb)
        assert torch.equal(single[0], one), "sample %d as a batch of one differs from far3d_attention_forward" % b
    return full


@pytest.mark.parametrize("odt", DTYPES, ids=["out_" + i for i in IDS])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(37, 50), (70, 130)], ids=lambda s: "x".join(map(str, s)))
def test_bitwise_against_the_one_sample_entry(hip_lib, shape, dt, odt):
    from far3d_amd import ops
    q, k, v = (t.to(dt).to(DEV) for t in _data(*shape))
    _equal_per_sample(ops, q, k, v, odt)


@pytest.mark.parametrize("odt", DTYPES, ids=["out_" + i for i in IDS])
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_bitwise_on_column_blocks_of_one_qkv_buffer(hip_lib, dt, odt):
    """q / k / v of the SECOND of two [q | k | v] column blocks of a (B, 300, 2 * 3 * 64) buffer, q its first 150 rows: row stride 384,
    batch stride 300 * 384, nothing copied."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(5)
    buf = torch.randn(B, 300, 2 * 3 * E, generator=g)
    buf[..., 3 * E:4 * E] *= 2.0
    d = buf.to(dt).to(DEV)
    q, k, v = d[:, :150, 3 * E:4 * E], d[:, :, 4 * E:5 * E], d[:, :, 5 * E:]
    assert not q.is_contiguous() and q.stride(0) == 300 * 6 * E
    full = _equal_per_sample(ops, q, k, v, odt)
    obuf = torch.full((B, 160, 2 * E), 7.0, device=DEV, dtype=odt)
    got = ops.attention_streams(q, k, v, H, out=obuf[:, :150, E:])
    assert torch.equal(got, full)
    assert bool((obuf[:, :, :E] == 7.0).all()) and bool((obuf[:, 150:] == 7.0).all())     # nothing outside the view is written


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_hole_counts_per_sample(hip_lib, dt):
    """Nk = 50, hole [20, 40), counts (0, 7, 20): sample 0 masks the whole hole, sample 1 keys [27, 40), sample 2 none."""
    from far3d_amd import ops
    q, k, v = (t.to(dt).to(DEV) for t in _data(37, 50))
    counts = torch.tensor([0, 7, 20], dtype=torch.int32, device=DEV)
    full = _equal_per_sample(ops, q, k, v, torch.float32, hole=(counts, 20, 40))
    free = ops.attention_streams(q, k, v, H)
    assert not torch.equal(full[0], free[0]), "sample 0 masks 20 keys: a kernel that ignores hole_count[b] gives the hole-free result"
    assert not torch.equal(full[1], free[1])
    assert torch.equal(full[2], free[2])            # count 20 = the whole hole is real: nothing is masked
    # a kernel that reads hole_count[0] for every sample
    assert not torch.equal(full[1], ops.attention_forward(q[1], k[1], v[1], H, hole=(counts[0:1], 20, 40)))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", [(37, 50), (70, 130)], ids=lambda s: "x".join(map(str, s)))
def test_against_float64(hip_lib, shape, dt):
    from far3d_amd import ops
    q, k, v = (t.to(dt) for t in _data(*shape))
    Nk = shape[1]
    counts = torch.tensor([0, 7, 20], dtype=torch.int32)
    for hole in (None, (counts.to(DEV), 20, 40)):
        kp = None
        if hole is not None:
            kp = torch.zeros(B, Nk, dtype=torch.bool)
            for b in range(B):
                kp[b, 20 + int(counts[b]):40] = True
        want = R.attention_ref(q, k, v, H, None, kp)
        got = ops.attention_streams(q.to(DEV), k.to(DEV), v.to(DEV), H, hole=hole).cpu()
        for b in range(B):
            d = (got[b].double() - want[b]).abs()
            print("%s %s hole=%s sample %d: max %.3e mean %.3e" % (shape, dt, hole is not None, b, d.max().item(), d.mean().item()))
            if dt == torch.float32:
                assert d.max().item() < 2e-5
            else:      # P is rounded to bf16 before the PV product (2^-9 relative per element, averaged by the sum)
                assert d.max().item() < 1e-2 and d.mean().item() < 1e-3


def test_bad_arguments_raise_and_launch_nothing(hip_lib):
    from far3d_amd import lib, ops
    Aq, Nk = 37, 50
    qd, kd, vd = (t.to(DEV) for t in _data(Aq, Nk))
    out = torch.full((B, Aq, E), 7.0, device=DEV)
    cnt = torch.zeros(B, dtype=torch.int32, device=DEV)
    with pytest.raises(lib.Far3dHipError, match="head_dim"):
        ops.attention_streams(qd, kd, vd, 1, out=out)                                     # head_dim 64
    with pytest.raises(lib.Far3dHipError, match="hole"):
        ops.attention_streams(qd, kd, vd, H, out=out, hole=(cnt, 20, Nk + 1))             # a hole outside [0, Nk]
    with pytest.raises(lib.Far3dHipError, match="hole"):
        ops.attention_streams(qd, kd, vd, H, out=out, hole=(cnt, -1, 40))
    big = torch.zeros(B * (Aq * E + 2), device=DEV)
    mis = big.as_strided((B, Aq, E), (Aq * E + 2, E, 1))                                   # batch stride 8 bytes off a 16-byte multiple
    with pytest.raises(lib.Far3dHipError, match="aligned"):
        ops.attention_streams(mis, kd, vd, H, out=out)
    with pytest.raises(lib.Far3dHipError, match="aligned"):
        ops.attention_streams(qd, kd, vd, H, out=torch.zeros(B * (Aq * E + 2), device=DEV).as_strided((B, Aq, E), (Aq * E + 2, E, 1)))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)

    def raw(qp=None, kp=None, vp=None, op=None, B_=B):
        qp, kp, vp, op = (p(t) if a is None else a for a, t in ((qp, qd), (kp, kd), (vp, vd), (op, out)))
        return hip_lib.far3d_attention_streams(qp, kp, vp, 0, op, 0, B_, Aq, Nk, H, 32, E, E, E, E,
                                               Aq * E, Nk * E, Nk * E, Aq * E, 32 ** -0.5, None, 0, 0, st)
    for what, rc in (("null q", raw(qp=null)), ("null k", raw(kp=null)), ("null v", raw(vp=null)), ("null out", raw(op=null)),
                     ("B < 1", raw(B_=0))):
        assert rc == -1, what
        assert hip_lib.far3d_last_error(), what
        with pytest.raises(lib.Far3dHipError):
            lib.check(rc, what)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                  # a refused call launches nothing
    assert raw() == 0                                # the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())
    assert torch.equal(out, ops.attention_streams(qd, kd, vd, H))
    with pytest.raises(ValueError, match="one count per sample"):
        ops.attention_streams(qd, kd, vd, H, hole=(cnt[:1], 20, 40))
    with pytest.raises(TypeError):
        ops.attention_streams(qd, kd.bfloat16(), vd, H)

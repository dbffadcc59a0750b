"""GPU: far3d_decode_topk_mem_streams (csrc/post.hip, ops.decode_topk_mem_streams) -- the decode and memory top-k launch for B scene
streams at once.  The contract is bitwise: stream b's boxes / scores / labels / keep / mem_idx are those of far3d_decode_topk_mem on
stream b's operands, whatever B is.  One shape per instantiation of the fused launch (A * ncls <= 4096, <= 16384, <= 40960) and one
outside it (the per-stream fallback), with streams whose ranking is decided by the tie rule."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NCLS, CODE, K, MEM_K = 26, 10, 300, 16
RANGE = [-60.0, -60.0, -5.0, 60.0, 60.0, 5.0]
SHAPES = [100, 400, 700, 1600]          # A: 2600 / 10400 / 18200 logits (the three instantiations), 41600 (per-stream fallback)


def _streams(A, seed):
    """Three streams' operands, (3, A, .) on the host.  Stream 0: logits quantised to 7 values, far fewer than K = 300, so ties decide
    nearly every rank.  Stream 1: all logits and memory scores equal.  Stream 2: continuous logits, every box centre outside RANGE."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randn(3, A, NCLS, generator=g)
    cls[0] = torch.round(cls[0] * 1.5) / 1.5
    cls[0].clamp_(-2.0, 2.0)
    cls[1] = 0.25
    box = torch.randn(3, A, CODE, generator=g)
    box[:, :, :3] *= 20.0
    box[:, :, 2].clamp_(-4.0, 4.0)
    box[2, :, 0] = 100.0 + box[2, :, 0].abs()
    mem = torch.rand(3, A, generator=g)
    mem[0] = torch.round(mem[0] * 4) / 4
    mem[1] = 0.5
    return cls, box, mem


def _one(ops, cls, box, mem):
    res, idx = ops.decode_topk(cls, box, K, RANGE, mem_scores=mem, mem_K=MEM_K)
    return dict(res, mem_idx=idx)


def _check(got, idx, want, b, what):
    for k in ("boxes_3d", "scores_3d", "labels_3d", "keep"):
        assert torch.equal(got[k][b], want[k]), "%s: stream %d: %s differs from the one-stream entry" % (what, b, k)
    assert torch.equal(idx[b], want["mem_idx"]), "%s: stream %d: mem_idx differs from the one-stream entry" % (what, b)


@pytest.mark.parametrize("A", SHAPES)
def test_streams_are_bitwise_the_one_stream_entry(hip_lib, A):
    from far3d_amd import ops
    cls, box, mem = (t.to(DEV) for t in _streams(A, 11 + A))
    want = [_one(ops, cls[b].contiguous(), box[b].contiguous(), mem[b].contiguous()) for b in range(3)]
    assert len(torch.unique(cls[0])) < 10 < K                       # K larger than the number of distinct values
    assert int(want[2]["keep"].sum()) == 0 and int(want[0]["keep"].sum()) > 0
    # all-equal logits: the tie rule alone ranks them -- lower flat index (query-major, then class) first
    flat = torch.arange(K, device=DEV)
    assert torch.equal(want[1]["labels_3d"], flat % NCLS) and torch.equal(want[1]["mem_idx"], torch.arange(MEM_K, device=DEV))
    got, idx = ops.decode_topk_mem_streams(cls, box, K, RANGE, mem, MEM_K)
    assert tuple(got["boxes_3d"].shape) == (3, K, CODE - 1) and tuple(idx.shape) == (3, MEM_K)
    for b in range(3):
        _check(got, idx, want[b], b, "B = 3")
    # B = 1, and independence of B: stream 0 alone has the result it has among three
    got1, idx1 = ops.decode_topk_mem_streams(cls[:1], box[:1], K, RANGE, mem[:1], MEM_K)
    _check(got1, idx1, want[0], 0, "B = 1")
    for k in got:
        assert torch.equal(got1[k][0], got[k][0])
    assert torch.equal(idx1[0], idx[0])
    # streams that are views into larger buffers (a batch stride above the stream's extent), in another order
    pad = lambda t: torch.cat([t, torch.zeros_like(t[:, :5])], dim=1)[:, :A]
    order = [2, 0, 1]
    cv, bv, mv = pad(cls[order]), pad(box[order]), pad(mem[order])
    assert cv.stride(0) == (A + 5) * NCLS and not cv.is_contiguous()
    got, idx = ops.decode_topk_mem_streams(cv, bv, K, RANGE, mv, MEM_K)
    for i, b in enumerate(order):
        _check(got, idx, want[b], i, "strided, order %s" % order)


def test_bad_arguments_name_the_argument_and_launch_nothing(hip_lib):
    from far3d_amd import lib, ops
    A, B = 100, 3
    cls, box, mem = (t.to(DEV) for t in _streams(A, 5))
    boxes = torch.full((B, K, CODE - 1), 7.0, device=DEV)
    scores = torch.full((B, K), 7.0, device=DEV)
    labels = torch.full((B, K), 7, dtype=torch.int64, device=DEV)
    keep = torch.full((B, K), 7, dtype=torch.uint8, device=DEV)
    idx = torch.full((B, MEM_K), 7, dtype=torch.int64, device=DEV)
    rng = (ctypes.c_float * 6)(*RANGE)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    good = dict(cls_last=p(cls), box_last=p(box), B=B, A=A, num_classes=NCLS, code_size=CODE, K=K,
                post_center_range=ctypes.cast(rng, ctypes.c_void_p), boxes=p(boxes), scores=p(scores), labels=p(labels), keep=p(keep),
                workspace=null, workspace_bytes=0, mem_scores=p(mem), mem_n=A, mem_K=MEM_K, mem_idx_out=p(idx))
    strides = [A * NCLS, A * CODE, K * (CODE - 1), K, K, K, A, MEM_K]

    def raw(strides_=strides, **over):
        a = dict(good, **over)
        bs = (ctypes.c_long * 8)(*strides_)
        return hip_lib.far3d_decode_topk_mem_streams(*[a[k] for k in good], ctypes.cast(bs, ctypes.c_void_p), st)

    def stride(i, v):
        s = list(strides)
        s[i] = v
        return s

    cases = [(name, dict([(name, null)]), name) for name in ("cls_last", "box_last", "post_center_range", "boxes", "scores", "labels",
                                                             "keep", "mem_scores", "mem_idx_out")]
    cases += [("B < 1", dict(B=0), "B=0"), ("K > 1024", dict(K=1025), "K=1025"), ("K > A * ncls", dict(A=1, K=27), "K=27"),
              ("code_size < 8", dict(code_size=7), "code_size=7"), ("mem_K > mem_n", dict(mem_K=A + 1), "mem_K=%d" % (A + 1)),
              ("mem_n > 40960", dict(mem_n=40961), "mem_n=40961"),
              ("no workspace beyond 40960 logits", dict(A=1600), "workspace")]
    for what, over, names in cases:
        rc = raw(**over)
        assert rc == -1, what
        msg = hip_lib.far3d_last_error().decode()
        assert "far3d_decode_topk_mem_streams" in msg and names in msg, (what, msg)
        with pytest.raises(lib.Far3dHipError):
            lib.check(rc, what)
    for i, name in enumerate(("cls_last", "box_last", "boxes", "scores", "labels", "keep", "mem_scores", "mem_idx_out")):
        for bad in (strides[i] - 1, -strides[i]):                    # streams that would share addresses, or run backwards
            assert raw(strides_=stride(i, bad)) == -1, name
            msg = hip_lib.far3d_last_error().decode()
            assert "batch_strides[%d] (%s)" % (i, name) in msg, msg
    assert hip_lib.far3d_decode_topk_mem_streams(*[good[k] for k in good], null, st) == -1
    assert "batch_strides" in hip_lib.far3d_last_error().decode()
    torch.cuda.synchronize()
    for t in (boxes, scores, labels, keep, idx):                     # a refused call launches nothing, for any stream
        assert bool((t == 7).all())
    assert raw() == 0                                                # the same call with good arguments runs
    torch.cuda.synchronize()
    want, widx = ops.decode_topk_mem_streams(cls, box, K, RANGE, mem, MEM_K)
    assert torch.equal(boxes, want["boxes_3d"]) and torch.equal(scores, want["scores_3d"]) and torch.equal(labels, want["labels_3d"])
    assert torch.equal(keep.bool(), want["keep"]) and torch.equal(idx, widx)
    assert raw(B=1, strides_=[0] * 8) == 0                           # one stream: the strides are not read
    with pytest.raises(ValueError, match="contiguous streams"):
        ops.decode_topk_mem_streams(cls.transpose(1, 2), box, K, RANGE, mem, MEM_K)
    with pytest.raises(ValueError, match="disagree"):
        ops.decode_topk_mem_streams(cls, box[:2], K, RANGE, mem, MEM_K)

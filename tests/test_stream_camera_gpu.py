"""GPU: StreamBatch's shared camera pass and shared head launches (far3d_amd/streams.py camera_batch / head_batch;
Far3DEngine.camera_stage_streams, _head_finish_streams) on the toy golden engine of tests/test_stream_batch_gpu.py (2 cameras,
64x96, proposal_topk=12).  The contract is the runner's: every stream's results are, bit for bit, those of the plain engine on that
stream's frames -- fp32, bf16 and bf16x3, for any number of streams and any chunking of the camera pass."""
import pytest
import torch

from far3d_amd import ops
from tests.test_stream_batch_gpu import B, PRECISIONS, SCHEDULE, _engine, _frame, _plain_sequence, _same, _snapshot

pytestmark = pytest.mark.gpu
PER_CAMERA = ("depth_logit", "ref2d", "ctx", "box2d", "score2d", "sel_idx", "sel_cnt")


def _clone_stage(st):
    snap = {k: st[k].clone() for k in PER_CAMERA}
    snap["tokens"] = st["tokens"].clone()
    snap.update({"raw%d" % i: r.clone() for i, r in enumerate(st["raw"])})
    return snap


def _joint_stage(sb, eng, frames, pad_hw):
    """Stage every stream's frame in the runner's joint buffers and run its camera passes -> a cloned snapshot per stream."""
    with ops.use_tile_tables(eng.bf16_tile_table()):
        dds = []
        for b, (data, _) in enumerate(frames):
            with sb._stream(b):
                dds.append(eng._stage_inputs(data))
        sts = sb._camera_streams(dds, pad_hw)
    return sts, [_clone_stage(st) for st in sts]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_camera_stage_streams_is_bitwise_the_camera_stage_per_stream(hip_lib, precision):
    from far3d_amd.streams import StreamBatch
    eng, rc = _engine(precision)
    frames = [_frame(rc, s, 0, 0) for s in range(B)]
    pad_hw = tuple(frames[0][1][0]["pad_shape"][0][:2])
    want = []
    for data, _ in frames:
        want.append(_clone_stage(eng._camera_part(eng._stage_inputs(data), pad_hw)))
    assert not torch.equal(want[0]["tokens"], want[1]["tokens"])
    assert sum(not torch.equal(want[a]["sel_idx"], want[b]["sel_idx"]) for a, b in ((0, 1), (0, 2), (1, 2))) >= 1
    # the planner's extent is the engine's: the largest per-image map of the pass just run is the span the passes are planned from
    N, H, W = frames[0][0]["img"].shape[-4], frames[0][0]["img"].shape[-2], frames[0][0]["img"].shape[-1]
    stage_maps = ("cat", "xt", "stage", "red", "dw_tmp", "lat", "fpn")          # the camera stage's NHWC buffers (backbone, fpn)
    maps = [t for k, t in eng._bufs.items() if k[0] == eng._par and k[1] in stage_maps and t.dim() == 4 and t.shape[0] == N and
            tuple(t.shape[1:3]) != (1, 1)]
    assert len(maps) > 10
    assert max(t.numel() * t.element_size() // N for t in maps) == eng.camera_image_span(H, W)
    sb = StreamBatch(eng, streams=B)
    sts, got = _joint_stage(sb, eng, frames, pad_hw)
    assert sb.camera_chunks == [B]
    for b in range(B):
        assert set(got[b]) == set(want[b])
        for k in want[b]:
            assert torch.equal(got[b][k], want[b][k]), "stream %d: %s differs from the one-stream camera stage" % (b, k)
        assert tuple(sts[b]["hw"]) == tuple(sts[0]["hw"]) and sts[b]["overflow"] is None and sts[b]["m_dev"] is None
    # the token maps landed in the one (B, N, S, 256) allocation: camera b * N + n is slice [b, n]
    step = sts[0]["tokens"].numel() * sts[0]["tokens"].element_size()
    assert all(sts[b]["tokens"].data_ptr() == sb._tokens.data_ptr() + b * step for b in range(B))
    # chunked: at most 2 streams per pass -> 2 + 1, the same bits
    sb2 = StreamBatch(eng, streams=B, max_camera_streams=2)
    _, got2 = _joint_stage(sb2, eng, frames, pad_hw)
    assert sb2.camera_chunks == [2, 1]
    for b in range(B):
        for k in want[b]:
            assert torch.equal(got2[b][k], want[b][k]), "chunked pass, stream %d: %s differs" % (b, k)


def _run(sb, frames, calls):
    n = sb.streams
    snaps = []
    for call in range(calls):
        outs = sb.forward_frames([frames[s][call][0] for s in range(n)], [frames[s][call][1] for s in range(n)])
        snaps.append([_snapshot(outs[s], sb.memory(s)) for s in range(n)])
    return snaps


@pytest.mark.parametrize("precision", PRECISIONS)
def test_runner_with_both_switches_is_the_runner_without_and_the_plain_engine(hip_lib, precision):
    """The six-call schedule with a scene change in stream 1: both switches on (one pass, and chunked 2 + 1) against both off and
    against the plain engine, outputs and memories."""
    from far3d_amd.streams import StreamBatch
    eng, rc = _engine(precision)
    frames = [[_frame(rc, s, *SCHEDULE[s][call]) for call in range(6)] for s in range(B)]
    want = [_plain_sequence(eng, frames[s]) for s in range(B)]
    off = _run(StreamBatch(eng, streams=B, camera_batch=False, head_batch=False), frames, 6)
    on = _run(StreamBatch(eng, streams=B, camera_batch=True, head_batch=True), frames, 6)
    for call in range(6):
        for s in range(B):
            _same(off[call][s], want[s][call], "switches off, call %d stream %d" % (call, s))
            _same(on[call][s], want[s][call], "switches on, call %d stream %d" % (call, s))
    # one switch at a time, and the chunked camera pass: three calls, across stream 1's scene change
    sub = [f[2:5] for f in frames]
    ref = [[w[call] for call in range(2, 5)] for w in want]
    for kw in (dict(camera_batch=True, head_batch=False), dict(camera_batch=False, head_batch=True),
               dict(camera_batch=True, head_batch=True, max_camera_streams=2)):
        sb = StreamBatch(eng, streams=B, **kw)
        for s in range(B):                 # bring every stream's memory to where call 2 finds it
            for k, v in sb.memory(s).items():
                v.copy_(want[s][1]["memory." + k])
            sb._state[s]["prev_scene"], sb._state[s]["mem_valid"] = frames[s][1][1][0]["scene_token"], True
        got = _run(sb, sub, 3)
        for call in range(3):
            for s in range(B):
                _same(got[call][s], ref[s][call], "%s, call %d stream %d" % (kw, call + 2, s))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_stream_with_both_switches_is_the_plain_engine(hip_lib, precision):
    from far3d_amd.streams import StreamBatch
    eng, rc = _engine(precision)
    frames = [[_frame(rc, 0, call, 0) for call in range(3)]]
    want = _plain_sequence(eng, frames[0])
    got = _run(StreamBatch(eng, streams=1, camera_batch=True, head_batch=True), frames, 3)
    for call in range(3):
        _same(got[call][0], want[call], "call %d" % call)


def test_three_streams_issue_the_conv_launches_of_one_camera_stage(hip_lib, monkeypatch):
    """Counted: the convolution launches (ops.conv2d_nhwc outside ops.linear, and the grouped entry) inside camera_stage.  One
    forward_frames call of three streams issues what ONE plain camera stage issues; with camera_batch off, three times that."""
    from far3d_amd.streams import StreamBatch
    eng, rc = _engine("bf16x3")
    count = dict(conv=0, stage=0, in_stage=0, in_linear=0)
    conv, grouped, linear, stage = ops.conv2d_nhwc, ops.conv2d_nhwc_grouped, ops.linear, eng.camera_stage

    def counted(fn, n):
        def wrapped(*a, **kw):
            if count["in_stage"] and not count["in_linear"]:
                count["conv"] += n(a)
            return fn(*a, **kw)
        return wrapped

    def nested(fn, key, tick=None):
        def wrapped(*a, **kw):
            count[key] += 1
            if tick:
                count[tick] += 1
            try:
                return fn(*a, **kw)
            finally:
                count[key] -= 1
        return wrapped

    monkeypatch.setattr(ops, "conv2d_nhwc", counted(conv, lambda a: 1))
    monkeypatch.setattr(ops, "conv2d_nhwc_grouped", counted(grouped, lambda a: 1))
    monkeypatch.setattr(ops, "linear", nested(linear, "in_linear"))
    monkeypatch.setattr(eng, "camera_stage", nested(stage, "in_stage", "stage"))
    frames = [_frame(rc, s, 0, 0) for s in range(B)]
    eng.forward_frame(*frames[0])
    one = count["conv"]
    assert count["stage"] == 1 and one > 50
    count.update(conv=0, stage=0)
    StreamBatch(eng, streams=B).forward_frames([f[0] for f in frames], [f[1] for f in frames])
    assert (count["stage"], count["conv"]) == (1, one)
    count.update(conv=0, stage=0)
    StreamBatch(eng, streams=B, camera_batch=False).forward_frames([f[0] for f in frames], [f[1] for f in frames])
    assert (count["stage"], count["conv"]) == (B, B * one)


def test_refusals_hold_with_the_new_keywords(hip_lib):
    from far3d_amd.streams import StreamBatch
    for kw in (dict(camera_batch=True, head_batch=True), dict(camera_batch=False, head_batch=False),
               dict(camera_batch=True, head_batch=True, max_camera_streams=1)):
        with pytest.raises(ValueError, match="proposal_capacity"):
            StreamBatch(_engine("bf16", proposal_topk=None, proposal_capacity=128)[0], streams=2, **kw)
        with pytest.raises(ValueError, match="proposal_topk"):
            StreamBatch(_engine("bf16", proposal_topk=None)[0], streams=2, **kw)
        with pytest.raises(ValueError, match="multi_depth"):
            StreamBatch(_engine("bf16", multi_depth=dict(topk=2, range_min=30))[0], streams=2, **kw)
        eng, rc = _engine("bf16")
        for opt in ("fused_rows", "use_graph", "pipeline"):
            setattr(eng, opt, True)
            with pytest.raises(ValueError, match=opt):
                StreamBatch(eng, streams=2, **kw)
            setattr(eng, opt, False)
        sb = StreamBatch(eng, streams=2, **kw)
        eng.use_graph = True                 # set after the constructor looked
        frames = [_frame(rc, s, 0, 0) for s in range(2)]
        with pytest.raises(ValueError, match="use_graph"):
            sb.forward_frames([f[0] for f in frames], [f[1] for f in frames])
        eng.use_graph = False
        with pytest.raises(ValueError, match="one frame per stream"):
            sb.forward_frames([frames[0][0]], [frames[0][1]])
        assert len(sb.forward_frames([f[0] for f in frames], [f[1] for f in frames])) == 2
    with pytest.raises(ValueError, match="max_camera_streams"):
        StreamBatch(_engine("bf16")[0], streams=2, max_camera_streams=0)

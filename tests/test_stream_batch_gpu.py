"""GPU: several scene streams on one engine (far3d_amd/streams.py StreamBatch, Far3DEngine.decoder_streams) on the toy golden engine
(tests/golden/far3d_small_seq.npz: 2 cameras, 64x96, 60 queries, 16 propagated, 64 memory slots; proposal_topk=12: A = 100 rows,
148 keys).  The contract is bitwise: every stream's results are those of a plain engine with the same weights fed that stream's
frames, whatever the number of streams -- fp32, bf16 (unfused decoder layers) and bf16x3."""
import pytest
import torch

from far3d_amd import synth

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "bf16", "bf16x3"]
B = 3
_ENGINES = {}


def _engine(precision, **over):
    """One engine per (precision, cfg) for the whole module: the plain engine the streams are compared with and the engine the
    StreamBatch drives are the SAME object (one set of weights; the runner keeps its own memories and buffer sets)."""
    from tests.test_engine_gpu import _golden_engine
    over.setdefault("proposal_topk", 12)
    key = (precision,) + tuple(sorted((k, str(v)) for k, v in over.items()))
    if key not in _ENGINES:
        eng, _, rc = _golden_engine(precision, **over)
        _ENGINES[key] = (eng, rc)
    eng, rc = _ENGINES[key]
    eng.reset_memory()
    eng.fused_rows, eng.use_graph, eng.pipeline = False, False, False
    return eng, rc


def _frame(rc, stream, fi, scene):
    """Frame `fi` of scene `scene` of stream `stream` (synth.recipe_frame): its own images and calibration (data seed) and its own
    scene tokens."""
    r = dict(rc, data_seed=rc["data_seed"] + 1000 * stream, scene_change_at=0 if scene else None)
    data, metas = synth.recipe_frame(r, fi)
    metas[0]["scene_token"] = "stream-%d-%s" % (stream, metas[0]["scene_token"])
    return data, metas


def _decoder_operands(eng, rc, stream):
    """Two frames of the stream through the plain engine (live memory keys), then the decoder's operands of the second, cloned."""
    eng.reset_memory()
    for fi in (0, 1):
        data, metas = _frame(rc, stream, fi, 0)
        eng.forward_frame(data, metas)
    cfg = eng.cfg
    pad_hw = tuple(metas[0]["pad_shape"][0][:2])
    A = cfg["num_query"] + eng.static_adaptive_rows(cfg["num_cams"]) + cfg["num_propagated"]
    TQ, QP, RF, X2 = (eng._bufs[(0, k)] for k in ("tq", "qp", "rf", "x2op"))
    st = eng._camera_part(eng._stage_inputs(data), pad_hw)
    assert X2[A:].float().abs().sum().item() > 0, "no live memory keys"
    ops_ = dict(X2=X2.clone(), x0=TQ[:A].clone(), qpos=QP[:A].clone(), tokens=st["tokens"].clone(), ref=RF[:A].clone(),
                lidar2img=eng._ins[0]["lidar2img"][0].clone())
    return ops_, st["hw"], st["starts"], pad_hw, A


@pytest.mark.parametrize("precision", PRECISIONS)
def test_decoder_streams_is_bitwise_the_decoder_per_stream(hip_lib, precision):
    eng, rc = _engine(precision)
    sets = []
    for s in range(B):
        o, hw, starts, pad_hw, A = _decoder_operands(eng, rc, s)
        sets.append(o)
    assert A == 100 and sets[0]["X2"].shape[0] == 148
    assert not torch.equal(sets[0]["X2"], sets[1]["X2"]) and not torch.equal(sets[1]["tokens"], sets[2]["tokens"])
    one = lambda o: (o["X2"].clone(), o["x0"], o["qpos"], o["tokens"], o["ref"], hw, starts, o["lidar2img"], pad_hw, A)
    col = lambda ss, n: [o[n] for o in ss]
    many = lambda ss: ([o["X2"].clone() for o in ss], col(ss, "x0"), col(ss, "qpos"), col(ss, "tokens"), col(ss, "ref"), hw, starts,
                       col(ss, "lidar2img"), pad_hw, A)
    want = []
    for o in sets:
        want.append(eng.decoder(*one(o)).clone())
        assert want[-1].shape == (eng.cfg["num_layers"], A, eng.cfg["embed_dims"]) and bool(torch.isfinite(want[-1]).all())
    assert not torch.equal(want[0], want[1])
    got = eng.decoder_streams(*many(sets))
    assert tuple(got.shape) == (B,) + tuple(want[0].shape)
    for b in range(B):
        for li in range(got.shape[1]):
            assert torch.equal(got[b, li], want[b][li]), "stream %d, layer %d differs from the one-stream decoder" % (b, li)
    # whatever B is: the first two streams alone, and the last as a batch of one
    got2 = eng.decoder_streams(*many(sets[:2])).clone()
    got1 = eng.decoder_streams(*many(sets[2:]))
    assert torch.equal(got2[0], want[0]) and torch.equal(got2[1], want[1]) and torch.equal(got1[0], want[2])


KEYS = ("all_cls_scores", "all_bbox_preds", "memory_topk")
RESULT = ("boxes_3d", "scores_3d", "labels_3d", "keep")


def _snapshot(outs, mem):
    """What the runner is compared on, cloned: logits, boxes, the decoded result, the memory's top-k and every tensor of the memory."""
    snap = {k: outs[k].clone() for k in KEYS}
    snap.update({"result." + k: outs["result"][k].clone() for k in RESULT})
    snap.update({"memory." + k: v.clone() for k, v in mem.items()})
    snap["keys"] = set(outs)
    return snap


def _same(got, want, what):
    assert got["keys"] == want["keys"], "%s: output keys differ from forward_frame's" % what
    for k in want:
        if k != "keys":
            assert torch.equal(got[k], want[k]), "%s: %s differs" % (what, k)


def _plain_sequence(eng, frames, reset_before=()):
    """The plain engine over one stream's frames (reset_memory() before the calls listed) -> a snapshot per call."""
    eng.reset_memory()
    snaps = []
    for call, (data, metas) in enumerate(frames):
        if call in reset_before:
            eng.reset_memory()
        snaps.append(_snapshot(eng.forward_frame(data, metas), eng.mem))
    return snaps


# per stream and call: (frame index inside the scene, scene).  Stream 1 starts a new scene at call 3, where streams 0 and 2 continue.
SCHEDULE = [[(c, 0) for c in range(6)],
            [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)],
            [(c, 0) for c in range(6)]]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_runner_is_bitwise_the_plain_engine_per_stream(hip_lib, precision):
    """Six calls of StreamBatch(engine, streams=3) against the plain engine (the same weights: the same engine, run before, one stream
    after the other) on every stream's own frame sequence."""
    from far3d_amd.streams import StreamBatch
    eng, rc = _engine(precision)
    frames = [[_frame(rc, s, *SCHEDULE[s][call]) for call in range(6)] for s in range(B)]
    want = [_plain_sequence(eng, frames[s]) for s in range(B)]
    assert not torch.equal(want[0][5]["all_cls_scores"], want[2][5]["all_cls_scores"])
    assert not torch.equal(want[1][3]["memory.emb"], want[0][3]["memory.emb"])     # stream 1 restarted at call 3
    sb = StreamBatch(eng, streams=B)
    for call in range(6):
        outs = sb.forward_frames([frames[s][call][0] for s in range(B)], [frames[s][call][1] for s in range(B)])
        assert len(outs) == B
        step = outs[0]["feat_flatten"].numel() * outs[0]["feat_flatten"].element_size()
        for s in range(B):
            _same(_snapshot(outs[s], sb.memory(s)), want[s][call], "call %d stream %d" % (call, s))
            # the value maps are not copied: stream s's camera stage wrote slice s of the ONE allocation the decoder pass reads
            assert outs[s]["feat_flatten"].data_ptr() == outs[0]["feat_flatten"].data_ptr() + s * step


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_stream_is_the_plain_engine(hip_lib, precision):
    from far3d_amd.streams import StreamBatch
    eng, rc = _engine(precision)
    frames = [_frame(rc, 0, call, 0) for call in range(3)]
    want = _plain_sequence(eng, frames)
    sb = StreamBatch(eng, streams=1)
    for call, (data, metas) in enumerate(frames):
        _same(_snapshot(sb.forward_frames([data], [metas])[0], sb.memory(0)), want[call], "call %d" % call)


def test_reset_memory_of_one_stream(hip_lib):
    """reset_memory(1) before call 2: stream 1's frame is the first of a scene again, streams 0 and 2 go on."""
    from far3d_amd.streams import StreamBatch
    eng, rc = _engine("fp32")
    frames = [[_frame(rc, s, call, 0) for call in range(3)] for s in range(B)]
    want = [_plain_sequence(eng, frames[s], reset_before=(2,) if s == 1 else ()) for s in range(B)]
    cont = _plain_sequence(eng, frames[1])
    assert not torch.equal(cont[2]["all_cls_scores"], want[1][2]["all_cls_scores"]), "the reset must change stream 1's third frame"
    sb = StreamBatch(eng, streams=B)
    for call in range(3):
        if call == 2:
            sb.reset_memory(1)
        outs = sb.forward_frames([frames[s][call][0] for s in range(B)], [frames[s][call][1] for s in range(B)])
        for s in range(B):
            _same(_snapshot(outs[s], sb.memory(s)), want[s][call], "call %d stream %d" % (call, s))


def test_refusals_name_the_option(hip_lib):
    from far3d_amd.streams import StreamBatch
    with pytest.raises(ValueError, match="proposal_capacity"):
        StreamBatch(_engine("bf16", proposal_topk=None, proposal_capacity=128)[0], streams=2)
    with pytest.raises(ValueError, match="proposal_topk"):
        StreamBatch(_engine("bf16", proposal_topk=None)[0], streams=2)
    with pytest.raises(ValueError, match="multi_depth"):
        StreamBatch(_engine("bf16", multi_depth=dict(topk=2, range_min=30))[0], streams=2)
    eng, rc = _engine("bf16")
    for opt in ("fused_rows", "use_graph", "pipeline"):
        setattr(eng, opt, True)
        with pytest.raises(ValueError, match=opt):
            StreamBatch(eng, streams=2)
        setattr(eng, opt, False)
    sb = StreamBatch(eng, streams=2)
    eng.use_graph = True                 # set after the constructor looked
    frames = [_frame(rc, s, 0, 0) for s in range(2)]
    with pytest.raises(ValueError, match="use_graph"):
        sb.forward_frames([f[0] for f in frames], [f[1] for f in frames])
    eng.use_graph = False
    with pytest.raises(ValueError, match="one frame per stream"):
        sb.forward_frames([frames[0][0]], [frames[0][1]])
    assert len(sb.forward_frames([f[0] for f in frames], [f[1] for f in frames])) == 2

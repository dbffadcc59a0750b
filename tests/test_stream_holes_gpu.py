"""GPU: StreamBatch(hole_rows=True) -- several scene streams in the proposal modes that leave a hole of unused query rows: the
fixed-capacity threshold mode (proposal_topk=None, proposal_capacity=R; the reference's shipped rule at a static row count) and
multi_depth topk > 1 in either static mode -- and Far3DEngine.decoder_streams(holes=...).  On the toy golden engine
(tests/golden/far3d_small_seq.npz: 2 cameras, 60 queries, 16 propagated, 64 memory slots, 26-29 proposals per frame).

The contract is bitwise: every stream's outputs and streaming memory are those of the plain engine in the same mode on that stream's
frames, hole rows included -- fp32, bf16 and bf16x3, with the shared camera pass and head launches on and off.  Stream 0 on the golden's
own frames is also held to the reference's outputs at tests/test_capacity_gpu.py's bars."""
import numpy as np
import pytest
import torch

from far3d_amd import synth
from tests.conftest import assert_detections_match
from tests.test_capacity_gpu import _valid_rows

pytestmark = pytest.mark.gpu
PRECISIONS = ["fp32", "bf16", "bf16x3"]
B = 3
MD = dict(topk=2, range_min=30)
CONFIGS = {"capacity": dict(proposal_topk=None, proposal_capacity=48),
           "capacity_md": dict(proposal_topk=None, proposal_capacity=48, multi_depth=MD),
           "topk_md": dict(proposal_topk=12, multi_depth=MD)}
_ENGINES = {}


def _engine(precision, **over):
    """One engine per (precision, cfg) for the whole module; the plain engine and the one StreamBatch drives are the same object."""
    from tests.test_engine_gpu import _golden_engine
    key = (precision,) + tuple(sorted((k, str(v)) for k, v in over.items()))
    if key not in _ENGINES:
        _ENGINES[key] = _golden_engine(precision, **over)
    eng, z, rc = _ENGINES[key]
    eng.reset_memory()
    eng.fused_rows, eng.use_graph, eng.pipeline = False, False, False
    return eng, z, rc


def _frame(rc, stream, fi, scene):
    """Frame `fi` of scene `scene` of stream `stream`: its own data seed and scene tokens; stream 0 has the golden's own frames."""
    r = dict(rc, data_seed=rc["data_seed"] + 1000 * stream, scene_change_at=0 if scene else None)
    data, metas = synth.recipe_frame(r, fi)
    metas[0]["scene_token"] = "stream-%d-%s" % (stream, metas[0]["scene_token"])
    return data, metas


# ------------------------------------------------------------------------------------------------ 1. the decoder pass
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
    ops_ = dict(X2=X2.clone(), x0=TQ[:A].clone(), qpos=QP[:A].clone(), tokens=st["tokens"].clone(), ref=RF[:A].clone(),
                lidar2img=eng._ins[0]["lidar2img"][0].clone())
    return ops_, st["hw"], st["starts"], pad_hw, A


@pytest.mark.parametrize("precision", PRECISIONS)
def test_decoder_streams_with_holes_is_bitwise_the_decoder_per_stream(hip_lib, precision):
    eng, _, rc = _engine(precision, **CONFIGS["capacity"])
    sets = []
    for s in range(B):
        o, hw, starts, pad_hw, A = _decoder_operands(eng, rc, s)
        sets.append(o)
    nq, cap = eng.cfg["num_query"], 48
    assert A == nq + cap + eng.cfg["num_propagated"]
    # a different count per stream: most of the rows empty, about the golden's own count, no hole at all
    holes = [(torch.tensor([c], dtype=torch.int32, device="cuda:0"), nq, nq + cap) for c in (7, 26, cap)]
    one = lambda o, h: eng.decoder(o["X2"].clone(), o["x0"], o["qpos"], o["tokens"], o["ref"], hw, starts, o["lidar2img"], pad_hw, A, hole=h)
    col = lambda ss, n: [o[n] for o in ss]
    many = lambda ss, hh: eng.decoder_streams([o["X2"].clone() for o in ss], col(ss, "x0"), col(ss, "qpos"), col(ss, "tokens"), col(ss, "ref"),
                                              hw, starts, col(ss, "lidar2img"), pad_hw, A, holes=hh)
    want = [one(o, h).clone() for o, h in zip(sets, holes)]
    assert all(bool(torch.isfinite(w).all()) for w in want)
    assert not torch.equal(want[0], one(sets[0], holes[1])), "the count must matter"
    got = many(sets, holes)
    assert tuple(got.shape) == (B, eng.cfg["num_layers"], A, eng.cfg["embed_dims"])
    for b in range(B):
        assert torch.equal(got[b], want[b]), "stream %d differs from the one-stream decoder with its hole" % b
    # whatever B is
    got2 = many(sets[:2], holes[:2]).clone()
    got1 = many(sets[2:], holes[2:])
    assert torch.equal(got2[0], want[0]) and torch.equal(got2[1], want[1]) and torch.equal(got1[0], want[2])
    with pytest.raises(ValueError, match="same start and end"):
        many(sets, [holes[0], holes[1], (holes[2][0], nq + 1, nq + cap)])
    with pytest.raises(ValueError, match="all of them None or none"):
        many(sets, [holes[0], None, holes[2]])


# ------------------------------------------------------------------------------------------------ 2. the runner
KEYS = ("all_cls_scores", "all_bbox_preds", "outs_dec", "memory_topk", "num_adaptive_dev", "bbox2d", "bbox2d_scores", "sel_cnt", "sel_idx",
        "proposal_overflow")
RESULT = ("boxes_3d", "scores_3d", "labels_3d", "keep")


def _snapshot(outs, mem):
    snap = {k: outs[k].clone() for k in KEYS}
    # a camera's selection list is written up to its count; what lies behind is never read (threshold mode: uninitialised memory)
    cap = snap["sel_idx"].shape[1]
    snap["sel_idx"][torch.arange(cap, device=snap["sel_idx"].device)[None, :] >= snap["sel_cnt"][:, None]] = -1
    snap["num_adaptive"] = torch.tensor(outs["num_adaptive"])
    if "md_records" in outs:
        # one record per primary proposal: proposal_gather_md writes the first sum(sel_cnt) of them and proposal_extra_rows reads no
        # more (threshold mode: the records behind them are uninitialised memory; top-K mode: every record is written)
        snap.update({"md_records.%d" % i: t.clone() for i, t in enumerate(outs["md_records"])})
        for i in range(len(outs["md_records"])):
            snap["md_records.%d" % i][int(snap["sel_cnt"].sum().item()):] = -1
    snap.update({"result." + k: outs["result"][k].clone() for k in RESULT})
    snap.update({"memory." + k: v.clone() for k, v in mem.items()})
    snap["keys"] = set(outs)
    return snap


def _same(got, want, what):
    assert got["keys"] == want["keys"], "%s: output keys differ from forward_frame's" % what
    assert set(got) == set(want)
    for k in want:
        if k != "keys":
            assert torch.equal(got[k], want[k]), "%s: %s differs" % (what, k)


def _plain_sequence(eng, frames, reset_before=()):
    eng.reset_memory()
    snaps = []
    for call, (data, metas) in enumerate(frames):
        if call in reset_before:
            eng.reset_memory()
        snaps.append(_snapshot(eng.forward_frame(data, metas), eng.mem))
    return snaps


# per stream and call: (frame index inside the scene, scene).  First frame, two steady frames, stream 1 changes scene at call 3, and
# stream 2's memory is reset before call 4.
SCHEDULE = [[(c, 0) for c in range(5)],
            [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)],
            [(c, 0) for c in range(5)]]
CALLS, RESET = 5, (4, 2)      # reset_memory(2) before call 4


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("precision", PRECISIONS)
def test_runner_with_hole_rows_is_bitwise_the_plain_engine_per_stream(hip_lib, precision, config):
    from far3d_amd.streams import StreamBatch
    eng, _, rc = _engine(precision, **CONFIGS[config])
    frames = [[_frame(rc, s, *SCHEDULE[s][call]) for call in range(CALLS)] for s in range(B)]
    want = [_plain_sequence(eng, frames[s], reset_before=(RESET[0],) if s == RESET[1] else ()) for s in range(B)]
    # what keeps the comparison from passing vacuously
    counts = [[int(want[s][c]["num_adaptive_dev"].item()) for s in range(B)] for c in range(CALLS)]
    rows = int(want[0][0]["num_adaptive"])
    print("%s %s: %d adaptive rows, counts per call %s" % (precision, config, rows, counts))
    assert all(n < rows for c in counts for n in c), "every stream needs a hole"
    assert any(len(set(c)) > 1 for c in counts), "two streams must differ in their count in some call"
    if "multi_depth" in CONFIGS[config]:
        prim = [[int(want[s][c]["sel_cnt"].sum().item()) if CONFIGS[config]["proposal_topk"] is None else want[s][c]["bbox2d"].shape[0]
                 for s in range(B)] for c in range(CALLS)]
        print("primaries per call %s" % prim)
        assert any(n > p for cn, cp in zip(counts, prim) for n, p in zip(cn, cp)), "some stream must have multi-depth extra rows"
        assert "md_records.0" in want[0][0]
    assert not torch.equal(want[1][3]["memory.emb"], want[0][3]["memory.emb"])
    for kw in (dict(camera_batch=True, head_batch=True), dict(camera_batch=False, head_batch=False)):
        sb = StreamBatch(eng, streams=B, hole_rows=True, **kw)
        for call in range(CALLS):
            if call == RESET[0]:
                sb.reset_memory(RESET[1])
            outs = sb.forward_frames([frames[s][call][0] for s in range(B)], [frames[s][call][1] for s in range(B)])
            for s in range(B):
                _same(_snapshot(outs[s], sb.memory(s)), want[s][call], "%s call %d stream %d" % (kw, call, s))
            sb.check_proposal_overflow()


# ------------------------------------------------------------------------------------------------ 3. the reference's own outputs
def test_stream_0_reproduces_the_reference_in_the_mode_the_goldens_were_made_in(hip_lib):
    """The goldens were generated in threshold mode.  Stream 0 runs the recipe's own frames (streams 1 and 2 their seeded ones) at
    capacity 48: the reference's proposals, logits, boxes and detections on the rows that hold queries, at test_capacity_gpu's bars."""
    from far3d_amd.streams import StreamBatch
    eng, z, rc = _engine("fp32", **CONFIGS["capacity"])
    nq, cap = rc["num_query"], 48
    sb = StreamBatch(eng, streams=B, hole_rows=True)
    for fi in range(rc["frames"]):
        fr = [synth.recipe_frame(rc, fi)] + [_frame(rc, s, fi, 0) for s in (1, 2)]
        o = sb.forward_frames([f[0] for f in fr], [f[1] for f in fr])[0]
        sb.check_proposal_overflow()
        M = int(o["num_adaptive_dev"].item())
        want_idx = z["f%d_valid_idx" % fi]
        assert o["num_adaptive"] == cap and M == len(want_idx), (fi, M, len(want_idx))
        cnt = o["sel_cnt"].cpu().numpy()
        got = [(n, int(i)) for n in range(rc["num_cams"]) for i in o["sel_idx"][n, :cnt[n]].cpu().numpy()]
        assert got == [(int(a[0]), int(a[1])) for a in want_idx]
        cls, box, r = o["all_cls_scores"], o["all_bbox_preds"], o["result"]
        g_cls = _valid_rows(cls, 2, nq, M, cap).cpu().numpy()
        g_box = _valid_rows(box, 2, nq, M, cap).cpu().numpy()
        w_cls, w_box = z["f%d_all_cls_scores" % fi], z["f%d_all_bbox_preds" % fi]
        assert g_cls.shape == w_cls.shape, (g_cls.shape, w_cls.shape)
        print("frame %d: logits %.3e (bar 1e-3), centres %.3e (bar 0.076), rest %.3e (bar 1e-3)" %
              (fi, np.abs(g_cls - w_cls).max(), np.abs(g_box - w_box)[..., :3].max(), np.abs(g_box - w_box)[..., 3:].max()))
        assert np.abs(g_cls - w_cls).max() < 1e-3, "frame %d logits: %.3e" % (fi, np.abs(g_cls - w_cls).max())
        assert np.abs(g_box - w_box)[..., :3].max() < 0.076 and np.abs(g_box - w_box)[..., 3:].max() < 1e-3
        hole = cls[:, 0, nq + M:nq + cap]
        assert hole.numel() > 0 and bool(torch.isinf(hole).all())
        keep = r["keep"].cpu().numpy()
        assert_detections_match(tuple(r[k].cpu().numpy()[keep] for k in ("labels_3d", "boxes_3d", "scores_3d")),
                                tuple(z["f%d_%s" % (fi, k)] for k in ("labels_3d", "boxes_3d", "scores_3d")), "frame %d" % fi)


# ------------------------------------------------------------------------------------------------ 4. overflow
def test_check_proposal_overflow_names_the_streams(hip_lib):
    """27 rows: the golden's frame 0 holds 29 proposals, its frame 1 at most 27."""
    from far3d_amd import lib
    from far3d_amd.streams import StreamBatch
    eng, z, rc = _engine("fp32", proposal_topk=None, proposal_capacity=27)
    assert len(z["f1_valid_idx"]) <= 27 < len(z["f0_valid_idx"])
    sb = StreamBatch(eng, streams=B, hole_rows=True)
    sb.check_proposal_overflow()                                   # nothing has run: nothing to report
    f0, f1 = synth.recipe_frame(rc, 0), synth.recipe_frame(rc, 1)
    for fr, over in (([f1, f0, f1], [1]), ([f1, f1, f1], []), ([f0, f1, f0], [0, 2])):
        outs = sb.forward_frames([f[0] for f in fr], [f[1] for f in fr])
        assert [b for b in range(B) if int(outs[b]["proposal_overflow"].item()) != 0] == over
        if over:
            with pytest.raises(lib.Far3dHipError, match=r"streams \[%s\]" % ", ".join(str(b) for b in over)):
                sb.check_proposal_overflow()
        else:
            sb.check_proposal_overflow()


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_with_and_without_the_keyword(hip_lib):
    from far3d_amd.streams import StreamBatch
    with pytest.raises(ValueError, match="proposal_topk=None without proposal_capacity"):
        StreamBatch(_engine("bf16", proposal_topk=None)[0], streams=2, hole_rows=True)
    eng = _engine("bf16", **CONFIGS["capacity_md"])[0]
    for opt in ("fused_rows", "use_graph", "pipeline"):
        setattr(eng, opt, True)
        with pytest.raises(ValueError, match=opt):
            StreamBatch(eng, streams=2, hole_rows=True)
        setattr(eng, opt, False)
    for name, val in (("agg_variant", 7), ("agg_split_extra", 8)):
        keep = getattr(eng, name)
        setattr(eng, name, val)
        with pytest.raises(ValueError, match=name):
            StreamBatch(eng, streams=2, hole_rows=True)
        setattr(eng, name, keep)
    StreamBatch(eng, streams=2, hole_rows=True)
    # without the keyword: refused as before
    with pytest.raises(ValueError, match="proposal_capacity"):
        StreamBatch(_engine("bf16", **CONFIGS["capacity"])[0], streams=2)
    with pytest.raises(ValueError, match="multi_depth"):
        StreamBatch(_engine("bf16", **CONFIGS["topk_md"])[0], streams=2)
    with pytest.raises(ValueError, match="proposal_capacity"):
        StreamBatch(eng, streams=2)

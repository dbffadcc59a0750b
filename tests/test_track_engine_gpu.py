"""GPU: track ids through the engine (cfg track) on the small golden sequence of tests/test_engine_gpu.py (2 cameras, 64x96, 60
queries, 16 propagated = 16 top-k, 64 memory slots, ego motion, a scene change at frame 2): switching tracking on moves no bit of
what the untracked engine returns, the ids are those of the CPU restatement (tests/track_refs.py) fed with the run's own ranking
and score plane, and every execution mode hands out the same ids."""
import numpy as np
import pytest
import torch

from far3d_amd import synth
from tests import track_refs as tr

pytestmark = pytest.mark.gpu
SEQ = [0, 1, 2, 3, 3, 3]            # frames of the golden recipe: scene 0 (0, 1), scene 1 (2, 3), then steady frames (graph replay)
_CACHE = {}


def engine_track_options(cfg, track):
    from far3d_amd import engine
    return engine.track_options(dict(cfg, track=track))


def _engine(track, **over):
    """One engine per configuration for the module (building one packs a VoV-99), handed out with its memory and ids forgotten."""
    from tests.test_engine_gpu import _golden_engine
    over.setdefault("proposal_topk", 12)
    key = (track is not None,) + tuple(sorted((k, str(v)) for k, v in over.items()))
    if key not in _CACHE:
        eng, _, rc = _golden_engine("fp32", track=track, **over)
        _CACHE[key] = (eng, rc)
    eng, rc = _CACHE[key]
    eng.use_graph, eng.pipeline, eng._graph = False, False, None
    if eng.track is not None:
        eng.track = engine_track_options(eng.cfg, track)      # the threshold is read at every call: one engine serves every value
        eng.reset_tracks()
    else:
        eng.reset_memory()
    return eng, rc


def _tensors(outs):
    flat = {k: v for k, v in outs.items() if isinstance(v, torch.Tensor)}
    flat.update({"result." + k: v for k, v in outs["result"].items()})
    return flat


def _run(eng, rc, seq=SEQ):
    """The sequence through forward_frame -> per frame (scene token, cloned tensors of the outputs, cloned memory)."""
    frames = []
    for fi in seq:
        data, metas = synth.recipe_frame(rc, fi)
        o = eng.forward_frame(data, metas)
        eng.wait_outputs()
        frames.append((metas[0]["scene_token"], {k: v.clone() for k, v in _tensors(o).items()}, {k: v.clone() for k, v in eng.mem.items()},
                       o["num_adaptive"]))
    return frames


def _same_outputs(want, got, fi):
    """Every tensor of the untracked frame's outputs, bit for bit (sel_idx: a camera's entries up to its count -- the rest of the
    selection buffer is never written)."""
    for k, v in want.items():
        g = got[k]
        if k == "sel_idx":
            cnt = want["sel_cnt"].tolist()
            assert all(torch.equal(g[n, :c], v[n, :c]) for n, c in enumerate(cnt)), "frame %d: sel_idx changes when tracking is switched on" % fi
        else:
            assert torch.equal(g, v), "frame %d: %s changes when tracking is switched on" % (fi, k)


def _restate(frames, cfg, birth_thr):
    """The restatement over a run's frames: asserts query_idx / track_ids / mem['track'] / the ids' life cycle; returns the ids per frame."""
    st, scene, per_frame, ever = tr.TrackState(cfg["memory_len"]), None, [], set()
    P, nq, ncls = cfg["num_propagated"], cfg["num_query"], cfg["num_classes"]
    for fi, (token, o, mem, M) in enumerate(frames):
        if token != scene:
            st.scene_reset()
            scene, alive = token, set()
        cls_last = o["all_cls_scores"][-1, 0].cpu().numpy()
        q, lab = tr.decode_query_rows(cls_last, o["result.scores_3d"].numel())
        assert o["result.query_idx"].cpu().numpy().tolist() == q.tolist(), "frame %d: query_idx" % fi
        assert o["result.labels_3d"].cpu().numpy().tolist() == lab.tolist()
        before = st.next_id
        ids, det = tr.track_frame(st, o["memory_topk"].cpu().numpy(), o["memory_scores"].cpu().numpy(), nq + M, P, birth_thr, q)
        assert o["result.track_ids"].cpu().numpy().tolist() == det.tolist(), "frame %d: track_ids" % fi
        assert o["result.track_ids"].dtype == torch.int64 and o["result.query_idx"].dtype == torch.int32
        assert mem["track"][0].cpu().numpy().tolist() == st.mem_track.tolist(), "frame %d: mem['track']" % fi
        live = set(ids[ids > 0].tolist())
        born = {i for i in live if i >= before}
        assert not (born & ever), "frame %d: an id was handed out twice" % fi
        assert live - born <= alive, "frame %d: an id that is not of this scene survived" % fi
        ever |= born
        alive |= born
        per_frame.append((ids, born))
    return per_frame


@pytest.mark.parametrize("birth_thr", [0.0, "median"])
def test_tracking_moves_no_bit_and_matches_the_restatement(hip_lib, birth_thr):
    plain, rc = _engine(None)
    assert "track" not in plain.mem and plain.track is None
    want = _run(plain, rc)
    for _, o, mem, _ in want:
        assert not any(k in o for k in ("result.track_ids", "result.query_idx", "memory_scores"))
    if birth_thr == "median":
        # a threshold that splits the ranked rows of this sequence: the median of frame 0's ranked max-class probabilities, taken from
        # the UNTRACKED run's logits (an input of the test, no tolerance)
        o0 = want[0][1]
        birth_thr = float(torch.sigmoid(o0["all_cls_scores"][-1, 0].max(-1).values)[o0["memory_topk"]].median().item())
        assert 0.0 < birth_thr < 1.0
    eng, rc = _engine(dict(birth_thr=birth_thr))
    got = _run(eng, rc)
    for fi, (w, g) in enumerate(zip(want, got)):
        assert set(g[1]) == set(w[1]) | {"result.track_ids", "result.query_idx", "memory_scores"}
        _same_outputs(w[1], g[1], fi)
        assert set(g[2]) == set(w[2]) | {"track"}
        for k, v in w[2].items():
            assert torch.equal(g[2][k], v), "frame %d: memory '%s' changes when tracking is switched on" % (fi, k)
    per_frame = _restate(got, eng.cfg, birth_thr)
    ids0, born0 = per_frame[0]
    ids1, born1 = per_frame[1]
    assert born0 and set(ids1[ids1 > 0].tolist()) & born0, "no id of frame 0 survived into frame 1 of the same scene"
    ids2, born2 = per_frame[2]
    assert set(ids2[ids2 > 0].tolist()) == born2 and min(born2) > max(born0 | born1), "an id crossed the scene change"
    if birth_thr > 0.0:
        assert any((ids == 0).any() for ids, _ in per_frame), "the threshold kept no ranked row without an identity"
    else:
        assert all((ids > 0).all() for ids, _ in per_frame)


def _ids(frames):
    return [(o["result.track_ids"], o["result.query_idx"], mem["track"]) for _, o, mem, _ in frames]


def test_graph_replay_hands_out_the_same_ids(hip_lib):
    eng, rc = _engine(dict(birth_thr=0.0))
    want = _ids(_run(eng, rc))
    counter = int(eng._track_next.item())
    assert counter > 1
    eng.reset_tracks()
    eng.use_graph = True
    got = _ids(_run(eng, rc))
    assert eng._graph is not None
    for fi, (w, g) in enumerate(zip(want, got)):
        for a, b in zip(w, g):
            assert torch.equal(a, b), "frame %d: graph replay differs from eager" % fi
    assert int(eng._track_next.item()) == counter
    eng.use_graph, eng._graph = False, None


def test_fixed_capacity_hole_mode(hip_lib):
    """proposal_capacity=48 (the smallest configuration of tests/test_capacity_gpu.py on this sequence): the propagated rows start behind
    the static 48 adaptive rows, the rows of the hole sit at -inf and are never born."""
    plain, rc = _engine(None, proposal_topk=None, proposal_capacity=48)
    want = _run(plain, rc)
    eng, rc = _engine(dict(birth_thr=0.0), proposal_topk=None, proposal_capacity=48)
    got = _run(eng, rc)
    eng.check_proposal_overflow()
    for fi, (w, g) in enumerate(zip(want, got)):
        assert g[3] == 48
        _same_outputs(w[1], g[1], fi)
        for k, v in w[2].items():
            assert torch.equal(g[2][k], v), "frame %d: memory '%s' changes when tracking is switched on" % (fi, k)
        sc = g[1]["memory_scores"]
        M = int(g[1]["num_adaptive_dev"].item())
        assert M < 48 and bool(torch.isinf(sc[eng.cfg["num_query"] + M:eng.cfg["num_query"] + 48]).all())
    _restate(got, eng.cfg, 0.0)
    eng.reset_tracks()
    eng.use_graph = True
    again = _run(eng, rc)
    for fi, (w, g) in enumerate(zip(_ids(got), _ids(again))):
        for a, b in zip(w, g):
            assert torch.equal(a, b), "frame %d: graph replay differs from eager" % fi
    eng.use_graph, eng._graph = False, None


def test_stream_batch_hands_out_the_ids_of_two_plain_engines(hip_lib):
    from far3d_amd.streams import StreamBatch
    from tests.test_stream_batch_gpu import _frame
    eng, rc = _engine(dict(birth_thr=0.0))
    eng.fused_rows = False
    schedule = [[(c, 0) for c in range(4)], [(0, 0), (1, 0), (0, 1), (1, 1)]]        # stream 1 changes its scene at call 2
    frames = [[_frame(rc, s, *schedule[s][call]) for call in range(4)] for s in range(2)]
    want = []
    for s in range(2):
        eng.reset_tracks()
        rows = []
        for data, metas in frames[s]:
            o = eng.forward_frame(data, metas)
            rows.append((o["result"]["track_ids"].clone(), o["result"]["query_idx"].clone(), eng.mem["track"].clone(),
                         o["result"]["scores_3d"].clone(), eng._track_next.clone()))
        want.append(rows)
    assert not torch.equal(want[0][3][1], want[1][3][1])
    for kw in (dict(), dict(head_batch=False)):
        sb = StreamBatch(eng, streams=2, **kw)
        for call in range(4):
            outs = sb.forward_frames([frames[s][call][0] for s in range(2)], [frames[s][call][1] for s in range(2)])
            for s in range(2):
                w, r = want[s][call], outs[s]["result"]
                assert torch.equal(r["track_ids"], w[0]) and torch.equal(r["query_idx"], w[1]) and torch.equal(r["scores_3d"], w[3]), (call, s)
                assert torch.equal(sb.memory(s)["track"], w[2]) and torch.equal(sb._track[1][s:s + 1], w[4]), (call, s)
        sb.reset_tracks(1)
        assert sb._track[1].view(-1).tolist()[1] == 1 and sb._track[1].view(-1).tolist()[0] > 1
    eng.fused_rows = True


def test_tracking_off_leaves_no_trace(hip_lib):
    from far3d_amd.streams import StreamBatch
    eng, rc = _engine(None)
    data, metas = synth.recipe_frame(rc, 0)
    o = eng.forward_frame(data, metas)
    assert "track" not in eng.mem and not hasattr(eng, "_track_next")
    assert set(o["result"]) == {"boxes_3d", "scores_3d", "labels_3d", "keep"} and "memory_scores" not in o
    with pytest.raises(ValueError, match="tracking is off"):
        eng.reset_tracks()
    eng.fused_rows = False
    sb = StreamBatch(eng, streams=2)
    assert sb._track is None and all("track" not in sb.memory(b) for b in range(2))
    eng.fused_rows = True


def test_detector_reports_the_kept_boxes_ids(hip_lib):
    """The registry-level surface: Far3D.prepare(track=True) -> pts_bbox['track_ids_3d'] (kept rows), FarHead.get_bboxes' fourth entry."""
    from far3d_amd import config, plugin, weights
    _, rc = _engine(None)
    spec = weights.detector_spec(rc["backbone"], num_query=rc["num_query"], num_propagated=rc["num_propagated"])
    det = plugin.build_detector(config.default_model_cfg(num_cams=rc["num_cams"], num_query=rc["num_query"], num_propagated=rc["num_propagated"],
                                                         memory_len=rc["memory_len"], topk_proposals=rc["topk_proposals"], proposal_capacity=48))
    det.load_state_dict(weights.init_state_dict(spec, seed=rc["weight_seed"]))
    det.prepare("cuda:0", precision="fp32")
    data, metas = synth.recipe_frame(rc, 0)
    assert "track_ids_3d" not in det(return_loss=False, rescale=True, img_metas=metas, **data)[0]["pts_bbox"]
    det.prepare("cuda:0", precision="fp32", track=True)
    assert det.engine.track == dict(birth_thr=0.0)
    seen = []
    for fi in (0, 1):
        data, metas = synth.recipe_frame(rc, fi)
        res = det(return_loss=False, rescale=True, img_metas=metas, **data)[0]["pts_bbox"]
        r = det.last_outs["result"]
        assert torch.equal(res["track_ids_3d"], r["track_ids"][r["keep"]]) and res["track_ids_3d"].shape == res["scores_3d"].shape
        boxes = det.pts_bbox_head.get_bboxes(dict(_far3d_result=r), metas)[0]
        assert len(boxes) == 4 and torch.equal(boxes[3], res["track_ids_3d"])
        plain = {k: v for k, v in r.items() if k not in ("track_ids", "query_idx")}
        assert len(det.pts_bbox_head.get_bboxes(dict(_far3d_result=plain), metas)[0]) == 3
        seen.append(set(r["track_ids"].tolist()) - {0})
    assert seen[0] and seen[0] & seen[1]

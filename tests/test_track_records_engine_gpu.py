"""GPU: track records through the engine (cfg track records=True) on the toy sequence of tests/test_track_engine_gpu.py (2 cameras,
64x96, 60 queries, 16 propagated = 16 top-k, 64 memory slots, ego motion, a scene change at frame 2): the eager engine against the CPU
restatement (tests/track_record_refs.py) driven from the run's own ranking, score plane, query rows, keep flags, boxes and pre-updated
memory -- integers exactly, the velocity within VEL_RTOL; graph replay, the pipelined engine and StreamBatch against the eager engine
bit for bit; and no trace of the records where the option is absent."""
import numpy as np
import pytest
import torch

from far3d_amd import synth
from tests import test_track_engine_gpu as tte
from tests import track_record_refs as rr

pytestmark = pytest.mark.gpu
SEQ = [0, 1, 2, 3, 3]               # 5 frames: scene 0 (0, 1), scene 1 (2, 3, 3)
REC = ("track_age", "track_primary", "track_velocity")
TRACK = dict(birth_thr=0.0, records=True)
_CACHE = {}


def _engine():
    """The records engine of the module (tests/test_track_engine_gpu.py caches its engines by 'tracking on': they must stay without
    records), handed out eager, with its memory and ids forgotten."""
    from tests.test_engine_gpu import _golden_engine
    if "eng" not in _CACHE:
        eng, _, rc = _golden_engine("fp32", track=TRACK, proposal_topk=12)
        _CACHE["eng"] = (eng, rc)
    eng, rc = _CACHE["eng"]
    eng.use_graph, eng.pipeline, eng._graph, eng.fused_rows = False, False, None, True
    eng.reset_tracks()
    return eng, rc


def _run(eng, rc, seq=SEQ, spy=False):
    """The sequence through forward_frame -> per frame dict(token, o: cloned output tensors, mem: cloned memory, M[, m: the pre-updated
    memory the head read])."""
    seen = []
    if spy:
        inner = eng._head_prepare
        def prepare(*a, **k):
            hs = inner(*a, **k)
            seen.append(hs.m)
            return hs
        eng._head_prepare = prepare
    frames = []
    try:
        for fi in seq:
            data, metas = synth.recipe_frame(rc, fi)
            o = eng.forward_frame(data, metas)
            eng.wait_outputs()
            fr = dict(token=metas[0]["scene_token"], o={k: v.clone() for k, v in tte._tensors(o).items()},
                      mem={k: v.clone() for k, v in eng.mem.items()}, M=o["num_adaptive"])
            if spy:
                fr["m"] = {k: seen[-1][k].clone() for k in ("ref", "ts")}
            frames.append(fr)
    finally:
        if spy:
            del eng._head_prepare
    return frames


def _eager():
    """The eager records run, computed once for the module and left unchanged."""
    if "eager" not in _CACHE:
        eng, rc = _engine()
        _CACHE["eager"] = _run(eng, rc, spy=True)
    return _CACHE["eager"]


def _same_records(want, got, what):
    for fi, (w, g) in enumerate(zip(want, got)):
        for k in ("result." + r for r in REC + ("track_ids", "query_idx", "boxes_3d", "scores_3d", "labels_3d", "keep")):
            assert torch.equal(w["o"][k], g["o"][k]), "frame %d: %s: %s differs from eager" % (fi, what, k)
        for k in ("track", "track_hits", "ref", "ts"):
            assert torch.equal(w["mem"][k], g["mem"][k]), "frame %d: %s: mem['%s'] differs from eager" % (fi, what, k)


def test_eager_engine_matches_the_restatement(hip_lib):
    eng, rc = _engine()
    frames = _eager()
    cfg = eng.cfg
    P, nq, L = cfg["num_propagated"], cfg["num_query"], cfg["memory_len"]
    assert tuple(eng.mem["track_hits"].shape) == (1, L) and eng.mem["track_hits"].dtype == torch.int32
    st, scene, ages, moving = rr.RecordState(L), None, [], []
    for fi, fr in enumerate(frames):
        o = fr["o"]
        if fr["token"] != scene:
            st.scene_reset()
            scene = fr["token"]
        A = nq + fr["M"] + P
        boxes = o["result.boxes_3d"].cpu().numpy()
        ids, det, rec = rr.track_records_frame(st, o["memory_topk"].cpu().numpy(), o["memory_scores"].cpu().numpy(), A, A - P, P, 0.0,
                                               o["result.query_idx"].cpu().numpy(), o["result.keep"].cpu().numpy(), boxes,
                                               fr["m"]["ref"][0].cpu().numpy(), fr["m"]["ts"][0, :, 0].cpu().numpy())
        K = boxes.shape[0]
        age, prim, vel = (o["result." + k] for k in REC)
        assert age.dtype == torch.int32 and prim.dtype == torch.bool and vel.dtype == torch.float32
        assert tuple(age.shape) == (K,) and tuple(prim.shape) == (K,) and tuple(vel.shape) == (K, 3)
        assert o["result.track_ids"].cpu().numpy().tolist() == det.tolist(), "frame %d: track_ids" % fi
        assert fr["mem"]["track"][0].cpu().numpy().tolist() == st.mem_track.tolist(), "frame %d: mem['track']" % fi
        assert fr["mem"]["track_hits"][0].cpu().numpy().tolist() == st.mem_hits.tolist(), "frame %d: mem['track_hits']" % fi
        assert st.invariant()
        assert age.cpu().numpy().tolist() == rec["age"].tolist(), "frame %d: track_age" % fi
        assert prim.cpu().numpy().tolist() == rec["primary"].tolist(), "frame %d: track_primary" % fi
        v = vel.cpu().numpy()
        nz = rec["velocity64"] != 0
        print("frame %d: %d boxes with a velocity, max rel err %.3e (bound %.3e)" %
              (fi, int(nz.any(axis=1).sum()), (np.abs(v - rec["velocity64"])[nz] / np.abs(rec["velocity64"][nz])).max() if nz.any() else 0.0, rr.VEL_RTOL))
        assert rr.velocity_within_bound(v, rec["velocity64"]), "frame %d: track_velocity" % fi
        pid = o["result.track_ids"][prim]
        assert pid.unique().numel() == pid.numel() and bool((pid != 0).all()), "frame %d: two primaries of one id" % fi
        assert bool(o["result.keep"][prim].all())
        ages.append(rec["age"])
        moving.append(int(nz.any(axis=1).sum()))
    assert ages[0].max() == 0 and ages[1].max() == 1 and ages[2].max() == 0 and ages[3].max() == 1 and ages[4].max() == 2
    assert moving[0] == 0 and moving[2] == 0 and moving[1] > 0 and moving[3] > 0      # a scene's first frame inherits nothing
    dup = [fr["o"]["result.track_ids"] for fr in frames]
    assert any(t[t != 0].unique().numel() < int((t != 0).sum()) for t in dup), "no frame of the sequence has two boxes of one id"


def test_graph_replay_equals_eager_bit_for_bit(hip_lib):
    want = _eager()
    eng, rc = _engine()
    eng.use_graph = True
    got = _run(eng, rc)
    assert eng._graph is not None
    _same_records(want, got, "graph replay")
    eng.use_graph, eng._graph = False, None


def test_pipelined_engine_equals_eager(hip_lib):
    """Tracking -- ids and records -- through the frame pipeline (pipeline + use_graph): extra steady frames so that every buffer set
    captures and replays."""
    eng, rc = _engine()
    seq = SEQ + [3] * 4
    want = _run(eng, rc, seq)
    eng.reset_tracks()
    eng.use_graph = eng.pipeline = True
    try:
        got = _run(eng, rc, seq)
        assert sorted(eng._pipe["g_head"]) == list(range(eng.pipeline_sets))
        torch.cuda.synchronize()
    finally:
        eng.use_graph = eng.pipeline = False
    _same_records(want, got, "pipeline")
    assert int(want[-1]["o"]["result.track_age"].max().item()) >= 2


def test_stream_batch_equals_two_plain_engines(hip_lib):
    from far3d_amd.streams import StreamBatch
    from tests.test_stream_batch_gpu import _frame
    eng, rc = _engine()
    eng.fused_rows = False
    schedule = [[(c, 0) for c in range(4)], [(0, 0), (1, 0), (0, 1), (1, 1)]]        # stream 1 changes its scene at call 2
    frames = [[_frame(rc, s, *schedule[s][call]) for call in range(4)] for s in range(2)]
    keys = REC + ("track_ids", "scores_3d")
    want = []
    for s in range(2):
        eng.reset_tracks()
        rows = []
        for data, metas in frames[s]:
            r = eng.forward_frame(data, metas)["result"]
            rows.append(({k: r[k].clone() for k in keys}, eng.mem["track"].clone(), eng.mem["track_hits"].clone()))
        want.append(rows)
    assert int(want[0][3][0]["track_age"].max().item()) >= 1 and int(want[1][2][0]["track_age"].max().item()) == 0
    assert bool(want[0][1][0]["track_velocity"].any())
    try:
        for kw in (dict(), dict(head_batch=False)):
            sb = StreamBatch(eng, streams=2, **kw)
            assert len(sb._track) == 3 and tuple(sb._track[2].shape) == (2, eng.cfg["memory_len"])
            for call in range(4):
                outs = sb.forward_frames([frames[s][call][0] for s in range(2)], [frames[s][call][1] for s in range(2)])
                for s in range(2):
                    w, r = want[s][call], outs[s]["result"]
                    for k in keys:
                        assert torch.equal(r[k], w[0][k]), (kw, call, s, k)
                    assert torch.equal(sb.memory(s)["track"], w[1]) and torch.equal(sb.memory(s)["track_hits"], w[2]), (kw, call, s)
                    assert sb.memory(s)["track_hits"].data_ptr() == sb._track[2][s].data_ptr()
    finally:
        eng.fused_rows = True


def test_records_absent_leaves_no_trace(hip_lib):
    """track=dict(birth_thr=0.0) without `records`: none of the three keys, no mem['track_hits'], and boxes, scores, labels and ids are
    those of the records-on run bit for bit."""
    want = _eager()
    plain, rc = tte._engine(dict(birth_thr=0.0))
    assert plain.track == dict(birth_thr=0.0) and "track_hits" not in plain.mem
    got = _run(plain, rc)
    for fi, (w, g) in enumerate(zip(want, got)):
        assert not any("result." + k in g["o"] for k in REC) and "track_hits" not in g["mem"]
        assert set(w["o"]) == set(g["o"]) | {"result." + k for k in REC} and set(w["mem"]) == set(g["mem"]) | {"track_hits"}
        for k in ("result.boxes_3d", "result.scores_3d", "result.labels_3d", "result.track_ids", "result.query_idx", "result.keep",
                  "all_cls_scores", "all_bbox_preds"):
            assert torch.equal(w["o"][k], g["o"][k]), "frame %d: %s changes when the records are switched on" % (fi, k)
        for k in g["mem"]:
            assert torch.equal(w["mem"][k], g["mem"][k]), "frame %d: memory '%s' changes when the records are switched on" % (fi, k)


def test_detector_reports_the_kept_boxes_records(hip_lib):
    """The registry-level surface: Far3D.prepare(track=dict(records=True)) -> pts_bbox['track_age_3d' / 'track_primary_3d' /
    'track_velocity_3d'] (kept rows), FarHead.get_bboxes' entries behind the ids; the four-entry shape without `records`."""
    from far3d_amd import config, plugin, weights
    _, rc = _engine()
    spec = weights.detector_spec(rc["backbone"], num_query=rc["num_query"], num_propagated=rc["num_propagated"])
    det = plugin.build_detector(config.default_model_cfg(num_cams=rc["num_cams"], num_query=rc["num_query"], num_propagated=rc["num_propagated"],
                                                         memory_len=rc["memory_len"], topk_proposals=rc["topk_proposals"], proposal_capacity=48))
    det.load_state_dict(weights.init_state_dict(spec, seed=rc["weight_seed"]))
    det.prepare("cuda:0", precision="fp32", track=dict(records=True))
    assert det.engine.track == dict(birth_thr=0.0, records=True)
    for fi in (0, 1):
        data, metas = synth.recipe_frame(rc, fi)
        res = det(return_loss=False, rescale=True, img_metas=metas, **data)[0]["pts_bbox"]
        r = det.last_outs["result"]
        boxes = det.pts_bbox_head.get_bboxes(dict(_far3d_result=r), metas)[0]
        assert len(boxes) == 7 and torch.equal(boxes[3], res["track_ids_3d"])
        for n, k in enumerate(REC):
            assert torch.equal(res[k + "_3d"], r[k][r["keep"]]) and torch.equal(boxes[4 + n], res[k + "_3d"])
            assert res[k + "_3d"].shape[0] == res["scores_3d"].shape[0]
        ids_only = {k: v for k, v in r.items() if k not in REC}
        assert len(det.pts_bbox_head.get_bboxes(dict(_far3d_result=ids_only), metas)[0]) == 4
    assert res["track_age_3d"].dtype == torch.int32 and res["track_primary_3d"].dtype == torch.bool and res["track_velocity_3d"].shape[1] == 3

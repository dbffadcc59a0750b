"""GPU: duplicate suppression through the engine (cfg dedup) on the toy sequence of tests/test_track_engine_gpu.py.  The engines are
that module's and tests/test_track_records_engine_gpu.py's own (building one packs a VoV-99): the option is read at every frame, so one
engine serves off and on -- which is also the strongest form of 'off leaves no trace'.  Dedup on against off bit for bit, dup_keep /
dup_of against a stand-alone ops.box_dedup and against the float64 contract (tests/dedup_refs.py) at a centre radius that suppresses a
share of the boxes; eager, graph replay, the frame pipeline and StreamBatch against each other; the track records' primary; the plugin."""
import numpy as np
import pytest
import torch

from far3d_amd import synth
from tests import dedup_refs as dr
from tests import test_track_engine_gpu as tte
from tests import test_track_records_engine_gpu as trg
from tests import track_record_refs as rr

pytestmark = pytest.mark.gpu
DUP = ("dup_keep", "dup_of")
_CACHE = {}


def _set(eng, dedup):
    """Switch the option on an engine whose graphs are forgotten (they hold or lack the launch)."""
    from far3d_amd import engine
    eng.dedup = engine.dedup_options(dict(eng.cfg, dedup=dedup))
    eng.use_graph, eng.pipeline, eng._graph = False, False, None
    for p in list(eng._pipe.slots):
        eng._pipe.drop(p)
    return eng


def _plain(dedup):
    eng, rc = tte._engine(None)
    return _set(eng, dedup), rc


def _records(dedup):
    eng, rc = trg._engine()
    return _set(eng, dedup), rc


def _off():
    """The plain engine's run without the option, computed once and left unchanged."""
    if "off" not in _CACHE:
        eng, rc = _plain(None)
        _CACHE["off"] = tte._run(eng, rc)
    return _CACHE["off"]


def _frame_inputs(o):
    return tuple(o["result." + k].cpu().numpy() for k in ("boxes_3d", "scores_3d", "labels_3d", "keep"))


def _search(frames, d2, accept):
    """The smallest radius between two neighbouring squared distances of d2 (ascending) that keeps every pair distance of every frame
    clear of it by MARGIN and whose float64 results (one per frame, class-blind) `accept` takes."""
    for lo, hi in zip(d2[:-1], d2[1:]):
        if lo <= 0 or hi < lo * (1.0 + 4.0 * dr.MARGIN):
            continue
        thr = float(np.sqrt(np.sqrt(lo * hi)))
        res = [dr.dedup(*f, mode="centre", thr=thr, class_aware=False) for f in frames]
        if all(dr.margin_ok(r["overlaps"], r["judged"], "centre", thr) for r in res) and accept(res):
            return thr
    raise AssertionError("no radius between two pair distances does what the test needs")


def _radius():
    """A centre-mode radius for the off run's boxes: between two neighbouring pair distances of frame 0, the smallest that suppresses
    a tenth of frame 0's candidates."""
    if "radius" not in _CACHE:
        frames = [_frame_inputs(o) for _, o, _, _ in _off()]
        b, s, l, k = frames[0]
        J = dr.judged_pairs(b, s, l, k, class_aware=False)
        d2 = np.unique(dr.overlaps64(b, J, "centre")[J])
        cand = int(dr.candidates(s, k).sum())
        assert len(d2) > 10 and cand > 10
        _CACHE["radius"] = _search(frames, d2, lambda res: (res[0]["dup_of"] >= 0).sum() >= 0.1 * cand)
    return _CACHE["radius"]


def _centre():
    return dict(mode="centre", thr=_radius(), class_aware=False)


def _same(want, got, what):
    for fi, (w, g) in enumerate(zip(want, got)):
        for k in [k for k in w[1] if k.startswith("result.")] + ["all_cls_scores", "all_bbox_preds", "memory_topk"]:
            assert torch.equal(w[1][k], g[1][k]), "frame %d: %s: %s differs" % (fi, what, k)
        for k in ("ref", "ts"):
            assert torch.equal(w[2][k], g[2][k]), "frame %d: %s: mem['%s'] differs" % (fi, what, k)


def test_on_against_off_and_a_stand_alone_launch(hip_lib):
    from far3d_amd import ops
    off = _off()[:3]
    assert not any("result." + k in o for _, o, _, _ in off for k in DUP)
    try:
        for dedup in (dict(), dict(mode="centre", thr=2.0, score_thr=0.2)):
            eng, rc = _plain(dedup)
            on = tte._run(eng, rc, tte.SEQ[:3])
            for fi, ((_, w, wm, wM), (_, g, gm, gM)) in enumerate(zip(off, on)):
                assert set(g) == set(w) | {"result." + k for k in DUP} and set(gm) == set(wm) and gM == wM
                tte._same_outputs(w, g, fi)
                for k in wm:
                    assert torch.equal(wm[k], gm[k]), "frame %d: memory '%s' changes when dedup is switched on" % (fi, k)
                dk, of = ops.box_dedup(*(g["result." + k][None] for k in ("boxes_3d", "scores_3d", "labels_3d", "keep")), **eng.dedup)
                assert g["result.dup_keep"].dtype == torch.bool and g["result.dup_of"].dtype == torch.int32
                assert tuple(g["result.dup_keep"].shape) == tuple(g["result.keep"].shape) == tuple(g["result.dup_of"].shape)
                assert torch.equal(g["result.dup_keep"], dk[0]) and torch.equal(g["result.dup_of"], of[0]), "frame %d: not the stand-alone launch" % fi
                assert bool((g["result.dup_keep"] <= g["result.keep"]).all())
    finally:
        _plain(None)


def test_a_radius_that_suppresses_matches_the_float64_contract(hip_lib):
    thr = _radius()
    eng, rc = _plain(_centre())
    try:
        on = tte._run(eng, rc, tte.SEQ[:3])
    finally:
        _plain(None)
    for fi, ((_, w, _, _), (_, g, _, _)) in enumerate(zip(_off(), on)):
        ref = dr.dedup(*_frame_inputs(w), mode="centre", thr=thr, class_aware=False)
        assert dr.margin_ok(ref["overlaps"], ref["judged"], "centre", thr)
        assert g["result.dup_keep"].cpu().numpy().tolist() == ref["dup_keep"].tolist(), "frame %d: dup_keep" % fi
        assert g["result.dup_of"].cpu().numpy().tolist() == ref["dup_of"].tolist(), "frame %d: dup_of" % fi
        print("frame %d: radius %.4f m, %d of %d candidates suppressed" % (fi, thr, int((ref["dup_of"] >= 0).sum()), int(ref["dup_keep"].sum() + (ref["dup_of"] >= 0).sum())))
        if fi == 0:
            assert (ref["dup_of"] >= 0).any() and ref["dup_keep"].any()


def test_eager_graph_replay_and_pipeline_agree(hip_lib):
    eng, rc = _plain(_centre())
    seq = tte.SEQ + [3] * 4
    try:
        want = tte._run(eng, rc, seq)
        assert any(bool((o["result.dup_of"] >= 0).any()) for _, o, _, _ in want)
        _set(eng, _centre()).use_graph = True
        got = tte._run(eng, rc, seq)
        assert eng._graph is not None
        _same(want, got, "graph replay")
        _set(eng, _centre())
        eng.use_graph = eng.pipeline = True
        got = tte._run(eng, rc, seq)
        assert sorted(eng._pipe["g_head"]) == list(range(eng.pipeline_sets))
        torch.cuda.synchronize()
        _same(want, got, "pipeline")
    finally:
        _plain(None)


def test_track_records_take_the_survivors(hip_lib):
    """ids, age and velocity keep the bits of the dedup-off run; track_primary is the restatement's, fed dup_keep as keep."""
    eng, rc = _records(None)
    off = trg._run(eng, rc)
    # a radius of its own: between two neighbouring distances of frame 1's primaries, the smallest that suppresses a primary of the off run
    prim = [f["o"]["result.track_primary"].cpu().numpy() for f in off]
    c = off[1]["o"]["result.boxes_3d"].cpu().numpy()[prim[1]][:, :2].astype(np.float64)
    d2 = np.unique(((c[:, None, :] - c[None, :, :]) ** 2).sum(-1)[np.triu_indices(len(c), 1)])
    thr = _search([_frame_inputs(f["o"]) for f in off], d2, lambda res: any((~r["dup_keep"] & p).any() for r, p in zip(res, prim)))
    eng, rc = _records(dict(mode="centre", thr=thr, class_aware=False))
    try:
        on = trg._run(eng, rc)
    finally:
        _records(None)
    cfg = eng.cfg
    P, L = cfg["num_propagated"], cfg["memory_len"]
    moved = 0
    for fi, (w, g) in enumerate(zip(off, on)):
        assert set(g["o"]) == set(w["o"]) | {"result." + k for k in DUP}
        for k in w["o"]:
            if k not in ("result.track_primary", "sel_idx"):
                assert torch.equal(w["o"][k], g["o"][k]), "frame %d: %s changes when dedup is switched on" % (fi, k)
        for k in w["mem"]:
            assert torch.equal(w["mem"][k], g["mem"][k]), "frame %d: memory '%s' changes when dedup is switched on" % (fi, k)
        o = g["o"]
        A = cfg["num_query"] + g["M"] + P
        rec = rr.records_frame(np.zeros(L, dtype=np.int32), o["memory_topk"].cpu().numpy(), g["mem"]["track"][0, :o["memory_topk"].numel()].cpu().numpy(),
                               A, A - P, P, o["result.query_idx"].cpu().numpy(), o["result.track_ids"].cpu().numpy(),
                               o["result.dup_keep"].cpu().numpy(), o["result.boxes_3d"].cpu().numpy(), np.zeros((L, 3), dtype=np.float32), np.zeros(L))
        prim = o["result.track_primary"]
        assert prim.cpu().numpy().tolist() == rec["primary"].tolist(), "frame %d: track_primary" % fi
        assert bool(o["result.dup_keep"][prim].all()), "frame %d: a primary is not a survivor" % fi
        pid = o["result.track_ids"][prim]
        assert pid.unique().numel() == pid.numel() and bool((pid != 0).all())
        moved += int((prim != w["o"]["result.track_primary"]).sum().item())
    print("primaries that moved or left with dedup on: %d" % moved)
    assert moved > 0, "the radius suppresses no primary of the dedup-off run: the test shows nothing"


def test_stream_batch_equals_two_plain_engines(hip_lib):
    from far3d_amd.streams import StreamBatch
    from tests.test_stream_batch_gpu import _frame
    eng, rc = _records(_centre())
    eng.fused_rows = False
    schedule = [[(c, 0) for c in range(3)], [(0, 0), (0, 1), (1, 1)]]        # stream 1 changes its scene at call 1
    frames = [[_frame(rc, s, *schedule[s][call]) for call in range(3)] for s in range(2)]
    keys = DUP + ("track_primary", "track_ids", "scores_3d", "keep")
    try:
        want = []
        for s in range(2):
            eng.reset_tracks()
            rows = []
            for data, metas in frames[s]:
                r = eng.forward_frame(data, metas)["result"]
                rows.append({k: r[k].clone() for k in keys})
            want.append(rows)
        assert any(bool((w["dup_of"] >= 0).any()) for rows in want for w in rows)
        for kw in (dict(), dict(head_batch=False)):
            sb = StreamBatch(eng, streams=2, **kw)
            for call in range(3):
                outs = sb.forward_frames([frames[s][call][0] for s in range(2)], [frames[s][call][1] for s in range(2)])
                for s in range(2):
                    for k in keys:
                        assert torch.equal(outs[s]["result"][k], want[s][call][k]), (kw, call, s, k)
    finally:
        eng.fused_rows = True
        _records(None)


def test_detector_returns_the_survivors(hip_lib):
    """Far3D.prepare(dedup=...) -> simple_test and FarHead.get_bboxes return exactly the dup_keep rows; without the option the keep rows."""
    from far3d_amd import config, ops, plugin, weights
    _, rc = _plain(None)
    spec = weights.detector_spec(rc["backbone"], num_query=rc["num_query"], num_propagated=rc["num_propagated"])
    det = plugin.build_detector(config.default_model_cfg(num_cams=rc["num_cams"], num_query=rc["num_query"], num_propagated=rc["num_propagated"],
                                                         memory_len=rc["memory_len"], topk_proposals=rc["topk_proposals"], proposal_capacity=48))
    det.load_state_dict(weights.init_state_dict(spec, seed=rc["weight_seed"]))
    det.prepare("cuda:0", precision="fp32", track=dict(records=True), dedup=dict(mode="centre", thr=3.0, class_aware=False))
    assert det.engine.dedup == dict(mode="centre", thr=3.0, class_aware=False, score_thr=0.0) and det.engine_cfg()["dedup"]["thr"] == 3.0
    dropped = 0
    for fi in (0, 1):
        data, metas = synth.recipe_frame(rc, fi)
        res = det(return_loss=False, rescale=True, img_metas=metas, **data)[0]["pts_bbox"]
        r = det.last_outs["result"]
        dk = r["dup_keep"]
        assert bool((dk <= r["keep"]).all())
        alone = ops.box_dedup(*(r[k][None] for k in ("boxes_3d", "scores_3d", "labels_3d", "keep")), **det.engine.dedup)      # an engine BUILT with the option
        assert torch.equal(dk, alone[0][0]) and torch.equal(r["dup_of"], alone[1][0])
        dropped += int((r["keep"] & ~dk).sum().item())
        boxes = det.pts_bbox_head.get_bboxes(dict(_far3d_result=r), metas)[0]
        for n, k in enumerate(("boxes_3d", "scores_3d", "labels_3d", "track_ids", "track_age", "track_primary", "track_velocity")):
            assert torch.equal(res[k if k.endswith("_3d") else k + "_3d"], r[k][dk]) and torch.equal(boxes[n], r[k][dk]), k
        off = {k: v for k, v in r.items() if k not in DUP}
        assert torch.equal(det.pts_bbox_head.get_bboxes(dict(_far3d_result=off), metas)[0][1], r["scores_3d"][r["keep"]])
    assert dropped > 0, "a 3 m radius drops no kept box of the toy model: the test shows nothing"

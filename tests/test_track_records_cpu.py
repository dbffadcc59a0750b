"""CPU: the track-record contract (tests/track_record_refs.py) on designed sequences at A=10, K=4, L=8 (propagated rows = the last P
query rows = memory slots 0..P-1), the `records` option, the result columns, and the ABI entry -- nothing here needs a device."""
import os
import re

import numpy as np
import pytest

from tests import track_record_refs as rr
from tests.conftest import ROOT

A, K, L = 10, 4, 8
HALF = np.full(A, 0.5, dtype=np.float32)


def _frame(st, idx, P, query=None, keep=None, boxes=None, m_ref=None, m_ts=None, score=HALF, thr=0.0):
    query = list(idx) if query is None else query
    n = len(query)
    keep = [True] * n if keep is None else keep
    boxes = np.zeros((n, 7), dtype=np.float32) if boxes is None else boxes
    m_ref = np.zeros((L, 3), dtype=np.float32) if m_ref is None else m_ref
    m_ts = np.full(L, 0.1) if m_ts is None else m_ts
    out = rr.track_records_frame(st, idx, score, A, A - P, P, thr, query, keep, boxes, m_ref, m_ts)
    assert st.invariant(), "hits > 0 must hold exactly where an id sits"
    return out


def test_a_track_ranked_four_frames_ages_0_1_2_3():
    P = 4
    st = rr.RecordState(L)
    ids, det, rec = _frame(st, [2, 7, 0, 5], P)
    assert rec["age"].tolist() == [0, 0, 0, 0] and st.mem_hits.tolist() == [1, 1, 1, 1, 0, 0, 0, 0]
    track = int(ids[0])                                  # row 2's id sits in slot 0 = row 6 of the next frame
    ages = [0]
    for idx in ([6, 1, 3, 4], [6, 0, 1, 2], [6, 9, 2, 3]):       # re-selected at rank 0 every frame: slot 0 again
        ids, det, rec = _frame(st, idx, P)
        assert int(ids[0]) == track
        ages.append(int(rec["age"][0]))
    assert ages == [0, 1, 2, 3] and int(st.mem_hits[0]) == 4
    # the last frame's row 9 = slot 3: the id born one frame earlier at rank 3, now in its second frame
    assert rec["age"].tolist()[1] == 1 and st.mem_hits.tolist()[:4] == [4, 2, 1, 1]
    assert st.mem_hits.tolist()[4:] == [3, 1, 1, 1]      # the old plane shifted by K, like the ids


def test_a_track_pushed_past_slot_p_ends():
    P = 2
    st = rr.RecordState(L)
    ids0, _, _ = _frame(st, [0, 1, 2, 3], P)             # ids 1..4 in slots 0..3; only slots 0, 1 are propagated (rows 8, 9)
    ids1, _, rec = _frame(st, [8, 4, 5, 6], P)
    assert ids1.tolist()[0] == ids0.tolist()[0] and rec["age"].tolist() == [1, 0, 0, 0]
    ids2, _, rec = _frame(st, [9, 8, 0, 1], P)           # slots 0, 1 now hold frame 1's ranks 0, 1
    assert ids2.tolist()[:2] == [ids1.tolist()[1], ids1.tolist()[0]] and rec["age"].tolist() == [1, 2, 0, 0]
    live = set(ids1.tolist()) | set(ids2.tolist())
    assert not {int(ids0[2]), int(ids0[3])} & live       # the ids of slots 2, 3 were never propagated: they ended at age 0
    assert st.mem_hits.tolist() == [2, 3, 1, 1, 2, 1, 1, 1]      # their counters ride on in the queue, as the ids do, and are never read


def test_scene_reset_clears_hits_with_ids():
    P = 4
    st = rr.RecordState(L)
    _frame(st, [0, 1, 2, 3], P)
    _frame(st, [6, 7, 8, 9], P)
    assert st.mem_hits.tolist()[:4] == [2, 2, 2, 2]
    st.scene_reset()
    assert not st.mem_hits.any() and not st.mem_track.any() and st.invariant()
    ids, _, rec = _frame(st, [6, 7, 8, 9], P)            # propagated rows of an empty memory: births, age 0, no velocity
    assert rec["age"].tolist() == [0] * 4 and ids.min() > 4 and not rec["velocity"].any()
    st.reset_tracks()
    assert not st.mem_hits.any() and st.next_id == 1


def test_unborn_rows_duplicates_primary_and_velocity():
    P = 4
    st = rr.RecordState(L)
    sc = HALF.copy()
    sc[1] = 0.1                                          # below the threshold: ranked, but no identity
    ids, det, rec = _frame(st, [0, 1, 2, 3], P, query=[0, 0, 1, 2, 5], keep=[False, True, True, True, True], score=sc, thr=0.3)
    assert ids.tolist() == [1, 0, 2, 3] and det.tolist() == [1, 1, 0, 2, 0]
    assert rec["age"].tolist() == [0, 0, -1, 0, -1]
    assert rec["primary"].tolist() == [False, True, False, True, False]      # the better box of id 1 is not kept: the second is primary
    assert st.mem_hits.tolist() == [1, 0, 1, 1, 0, 0, 0, 0]
    # next frame: row 6 = slot 0 (id 1) moved by (3.0, -1.5, 0.25) m/s over 0.1 s; row 8 = slot 2 whose m_ts is 0; row 7 = slot 1, no id
    m_ref = np.zeros((L, 3), dtype=np.float32)
    m_ref[0] = [10.0, 20.0, 1.0]
    m_ts = np.array([0.1, 0.1, 0.0, np.nan, 0.1, 0.1, 0.1, 0.1])
    boxes = np.zeros((5, 7), dtype=np.float32)
    boxes[0, :3] = boxes[1, :3] = [10.3, 19.85, 1.025]
    boxes[2, :3] = boxes[3, :3] = boxes[4, :3] = [1.0, 2.0, 3.0]
    ids, det, rec = _frame(st, [6, 8, 7, 9], P, query=[6, 6, 8, 7, 9], boxes=boxes, m_ref=m_ref, m_ts=m_ts)
    assert ids.tolist() == [1, 2, 4, 3] and rec["age"].tolist() == [1, 1, 1, 0, 1]
    assert rec["primary"].tolist() == [True, False, True, True, True]
    assert np.allclose(rec["velocity64"][0], [3.0, -1.5, 0.25], rtol=1e-5) and rr.velocity_within_bound(rec["velocity"], rec["velocity64"])
    assert np.array_equal(rec["velocity"][0], rec["velocity"][1])
    assert not rec["velocity"][2:].any() and not np.signbit(rec["velocity"][2:]).any()      # m_ts 0, a birth, m_ts NaN: exactly +0.0


def test_track_options_accepts_records_and_returns_exactly_what_was_given():
    from far3d_amd import engine
    opt = engine.track_options
    assert opt(engine.default_cfg(track=dict(birth_thr=0.25, records=True))) == dict(birth_thr=0.25, records=True)
    assert opt(engine.default_cfg(track=dict(records=True))) == dict(birth_thr=0.0, records=True)
    assert opt(engine.default_cfg(track=dict(birth_thr=0.5, records=False))) == dict(birth_thr=0.5, records=False)
    assert opt(engine.default_cfg(track=dict(birth_thr=0.25))) == dict(birth_thr=0.25)        # no defaulted key
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="records"):
            opt(engine.default_cfg(track=dict(records=bad)))
    with pytest.raises(ValueError, match="unknown option"):
        opt(engine.default_cfg(track=dict(record=True)))


def _outputs():
    import torch
    outs = [dict(boxes_3d=torch.rand(4, 7), scores_3d=torch.tensor([0.9, 0.8, 0.7, 0.6]), labels_3d=torch.tensor([0, 1, 2, 0])),
            dict(pts_bbox=dict(boxes_3d=torch.rand(3, 7), scores_3d=torch.tensor([0.5, 0.4, 0.3]), labels_3d=torch.tensor([1, 1, 2])))]
    infos = [dict(scene_id="a", lidar_timestamp_ns=1), dict(scene_id="a", lidar_timestamp_ns=2)]
    ids = [torch.tensor([7, 7, 0, 9]), [7, 3, 3]]
    recs = [dict(age=torch.tensor([2, 2, -1, 0], dtype=torch.int32), primary=torch.tensor([True, False, False, True]),
                 velocity=torch.tensor([[1.0, 2.0, 3.0]] * 2 + [[0.0] * 3] * 2)),
            dict(age=[3, 0, 0], primary=[True, True, False], velocity=np.array([[4.0, 5.0, 6.0], [0, 0, 0], [0, 0, 0]], dtype=np.float32))]
    return outs, infos, ids, recs


def test_format_results_writes_the_record_columns_only_when_given():
    from far3d_amd.data_pipeline import results
    outs, infos, ids, recs = _outputs()
    cols = ("track_age", "track_primary", "vx_m", "vy_m", "vz_m")
    assert not set(cols) & set(results.format_results(outs, infos, track_ids=ids).columns)
    df = results.format_results(outs, infos, track_ids=ids, track_records=recs)
    assert set(cols) <= set(df.columns) and len(df) == 7
    assert df["track_age"].dtype == np.int32 and df["track_primary"].dtype == bool and df["vx_m"].dtype == np.float32
    rows = {round(float(r.score), 1): r for r in df.itertuples()}
    assert (rows[0.9].track_id, rows[0.9].track_age, rows[0.9].track_primary, rows[0.9].vx_m, rows[0.9].vz_m) == (7, 2, True, 1.0, 3.0)
    assert (rows[0.7].track_id, rows[0.7].track_age, rows[0.7].track_primary) == (0, -1, False)
    assert (rows[0.5].track_age, rows[0.5].vy_m) == (3, 5.0)
    with pytest.raises(AssertionError, match="age"):
        results.format_results(outs, infos, track_ids=ids, track_records=[dict(recs[0], age=[1, 2]), recs[1]])
    with pytest.raises(AssertionError):
        results.format_results(outs, infos, track_records=recs[:1])
    with pytest.raises(ValueError, match="primary_only"):
        results.format_results(outs, infos, track_ids=ids, primary_only=True)


def test_primary_only_leaves_one_row_per_log_timestamp_and_id():
    from far3d_amd.data_pipeline import results
    outs, infos, ids, recs = _outputs()
    full = results.format_results(outs, infos, track_ids=ids, track_records=recs).reset_index()
    assert full.duplicated(["log_id", "timestamp_ns", "track_id"]).any()
    df = results.format_results(outs, infos, track_ids=ids, track_records=recs, primary_only=True).reset_index()
    assert not df.duplicated(["log_id", "timestamp_ns", "track_id"]).any()
    assert bool(df["track_primary"].all()) and (df["track_id"] != 0).all()
    assert sorted(zip(df["timestamp_ns"].tolist(), df["track_id"].tolist())) == [(1, 7), (1, 9), (2, 3), (2, 7)]
    assert sorted(round(float(s), 1) for s in df["score"]) == [0.4, 0.5, 0.6, 0.9]


def test_abi_entry_is_declared_and_has_a_signature():
    from far3d_amd import lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "far3d_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+far3d_track_records\s*\(([^)]*)\)", src)
    assert m, "include/far3d_hip.h does not declare far3d_track_records"
    restype, argtypes = lib.SIGNATURES["far3d_track_records"]
    assert len(argtypes) == len(m.group(1).split(",")) == 22
    assert "far3d_track_records" in open(os.path.join(ROOT, "far3d_amd", "csrc", "track.hip")).read()

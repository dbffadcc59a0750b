"""CPU: the track-id contract (tests/track_refs.py) on hand-made three-frame chains at A=10, K=4, L=8, P=4 (propagated rows 6..9 =
memory slots 0..3), the configuration refusal, and the host-side surfaces that need no device."""
import numpy as np
import pytest

from tests import track_refs as tr

A, K, L, P = 10, 4, 8, 4
ROW0 = A - P
HALF = np.full(A, 0.5, dtype=np.float32)


def test_reselected_row_keeps_its_id_and_a_new_row_gets_a_fresh_one():
    st = tr.TrackState(L)
    ids, _ = tr.track_frame(st, [2, 7, 0, 5], HALF, ROW0, P)          # row 7 is a propagated row, but its slot holds no identity yet
    assert ids.tolist() == [1, 2, 3, 4] and st.mem_track.tolist() == [1, 2, 3, 4, 0, 0, 0, 0] and st.next_id == 5
    ids, det = tr.track_frame(st, [8, 1, 6, 3], HALF, ROW0, P, query_idx=[8, 8, 3, 4])
    assert ids.tolist() == [3, 5, 1, 6]                                 # row 8 = slot 2 (id 3), row 6 = slot 0 (id 1); rows 1, 3 are born
    assert st.mem_track.tolist() == [3, 5, 1, 6, 1, 2, 3, 4] and st.next_id == 7      # the id moved to its new slot, the queue shifted
    assert det.tolist() == [3, 3, 6, 0]                                 # two boxes of one query share its id; row 4 is not in the top-k
    ids, _ = tr.track_frame(st, [9, 7, 6, 2], HALF, ROW0, P)
    assert ids.tolist() == [6, 5, 3, 7] and st.mem_track.tolist() == [6, 5, 3, 7, 3, 5, 1, 6] and st.next_id == 8


def test_row_below_birth_thr_is_born_a_frame_later():
    st = tr.TrackState(L)
    sc = HALF.copy()
    sc[1] = 0.1
    ids, det = tr.track_frame(st, [0, 1, 2, 3], sc, ROW0, P, birth_thr=0.3, query_idx=[1, 2])
    assert ids.tolist() == [1, 0, 2, 3] and st.next_id == 4 and det.tolist() == [0, 2]       # the births count past the unborn row
    sc = HALF.copy()
    sc[7] = 0.9
    ids, _ = tr.track_frame(st, [7, 6, 4, 5], sc, ROW0, P, birth_thr=0.3)
    assert ids.tolist() == [4, 1, 5, 6] and st.next_id == 7            # row 7 = slot 1, id-less so far, now above the threshold
    ids, _ = tr.track_frame(st, [6, 7, 8, 9], sc, ROW0, P, birth_thr=0.3)
    assert ids.tolist() == [4, 1, 5, 6] and st.next_id == 7            # all four propagated: nothing is born


def test_threshold_is_inclusive_and_holes_are_never_born():
    st = tr.TrackState(L)
    sc = np.array([0.25, -np.inf, np.nan, 0.2499999] + [0.5] * 6, dtype=np.float32)
    ids, _ = tr.track_frame(st, [0, 1, 2, 3], sc, ROW0, P, birth_thr=0.25)
    assert ids.tolist() == [1, 0, 0, 0] and st.next_id == 2
    ids, _ = tr.track_frame(tr.TrackState(L), [0, 1, 2, 3], sc, ROW0, P, birth_thr=0.0)
    assert ids.tolist() == [1, 0, 0, 2]                                 # birth_thr 0: every finite ranked row


def test_scene_reset_clears_the_ids_and_the_counter_continues():
    st = tr.TrackState(L)
    tr.track_frame(st, [0, 1, 2, 3], HALF, ROW0, P)
    st.scene_reset()
    assert st.mem_track.tolist() == [0] * L and st.next_id == 5
    ids, _ = tr.track_frame(st, [6, 7, 8, 9], HALF, ROW0, P)
    assert ids.tolist() == [5, 6, 7, 8]                                 # propagated rows of an empty memory: all new, none reused
    ids, _ = tr.track_frame(st, [6, 7, 8, 9], HALF, ROW0, P)
    assert ids.tolist() == [5, 6, 7, 8]
    st.reset_tracks()
    assert st.next_id == 1 and not st.mem_track.any()


def test_fewer_propagated_slots_than_ranked_rows_lets_ids_die():
    p, row0 = 2, A - 2
    st = tr.TrackState(L)
    ids, _ = tr.track_frame(st, [0, 1, 2, 3], HALF, row0, p)
    assert ids.tolist() == [1, 2, 3, 4]
    seen = []
    for idx in ([8, 4, 5, 6], [9, 8, 0, 1], [8, 9, 2, 3]):              # rows 8, 9 = slots 0, 1: ids 3 and 4 sat in slots 2, 3
        ids, _ = tr.track_frame(st, idx, HALF, row0, p)
        seen += ids.tolist()
    assert seen[:4] == [1, 5, 6, 7] and 3 not in seen and 4 not in seen and 2 not in seen
    assert sorted(set(seen)) == [1, 5, 6, 7, 8, 9, 10, 11]


def test_more_propagated_slots_than_ranked_rows_is_refused():
    with pytest.raises(ValueError, match="num_propagated=6 > topk_proposals=4"):
        tr.track_frame(tr.TrackState(L), [0, 1, 2, 3], HALF, A - 6, 6)
    from far3d_amd import engine
    cfg = engine.default_cfg(num_propagated=32, topk_proposals=16)
    assert engine.track_options(cfg) is None                            # off: any configuration
    with pytest.raises(ValueError, match="num_propagated=32 > topk_proposals=16"):
        engine.track_options(dict(cfg, track=dict(birth_thr=0.0)))
    with pytest.raises(ValueError, match="birth_thr"):
        engine.track_options(engine.default_cfg(track=dict(birth_thr=1.5)))
    with pytest.raises(ValueError, match="unknown option"):
        engine.track_options(engine.default_cfg(track=dict(threshold=0.5)))
    assert engine.track_options(engine.default_cfg(track=dict(birth_thr=0.25))) == dict(birth_thr=0.25)
    assert engine.track_options(engine.default_cfg(track=True)) == dict(birth_thr=0.0)
    assert engine.default_cfg()["track"] is None


def test_decode_query_rows_breaks_ties_by_flat_index():
    cls = np.zeros((5, 3), dtype=np.float32)
    cls[3, 1] = 1.0
    q, lab = tr.decode_query_rows(cls, 5)
    assert q.tolist() == [3, 0, 0, 0, 1] and lab.tolist() == [1, 0, 1, 2, 0]


def test_format_results_writes_track_id_only_when_given():
    import torch
    from far3d_amd.data_pipeline import results
    outs = [dict(boxes_3d=torch.rand(3, 7), scores_3d=torch.tensor([0.9, 0.5, 0.7]), labels_3d=torch.tensor([0, 1, 2])),
            dict(pts_bbox=dict(boxes_3d=torch.rand(2, 7), scores_3d=torch.tensor([0.8, 0.6]), labels_3d=torch.tensor([1, 1])))]
    infos = [dict(scene_id="a", lidar_timestamp_ns=1), dict(scene_id="a", lidar_timestamp_ns=2)]
    assert "track_id" not in results.format_results(outs, infos).columns
    df = results.format_results(outs, infos, track_ids=[torch.tensor([7, 0, 9]), [3, 4]])
    assert df["track_id"].dtype == np.int64
    assert sorted(zip([round(float(s), 3) for s in df["score"]], df["track_id"].tolist())) ==[(0.5, 0), (0.6, 4), (0.7, 9), (0.8, 3), (0.9, 7)]

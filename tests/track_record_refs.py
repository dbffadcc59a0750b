"""Track records, restated on the CPU in plain Python and numpy: the contract of far3d_track_records (include/far3d_hip.h).  The ids
are those of tests/track_refs.py, which this file imports and leaves alone.  The GPU tests compare the kernel with this file: the
integers exactly, the velocity against `velocity64` within VEL_RTOL."""
import math

import numpy as np

from tests import track_refs as tr

# |v - v64| <= VEL_RTOL * |v64| per component, v64 the float64 evaluation of the same fp32 inputs: the kernel rounds m_ts to fp32, then
# one correctly rounded fp32 subtraction and one division -- three relative errors of at most 2^-24 each, (1 + 2^-24)^3 - 1 < 4 * 2^-24
VEL_RTOL = 4.0 * 2.0 ** -24


class RecordState(tr.TrackState):
    """TrackState plus mem_hits (L,) int32: the number of frames the id in that queue slot has been ranked (> 0 exactly where
    mem_track != 0)."""

    def __init__(self, L, next_id=1):
        super().__init__(L, next_id)
        self.mem_hits = np.zeros(int(L), dtype=np.int32)

    def scene_reset(self):
        super().scene_reset()
        self.mem_hits[:] = 0

    def reset_tracks(self):
        super().reset_tracks()
        self.mem_hits[:] = 0

    def invariant(self):
        return bool(((self.mem_hits > 0) == (self.mem_track != 0)).all())


def records_frame(mem_hits, idx, ranked_ids, num_rows, row_start, num_propagated, query_idx, track_ids, keep, boxes, m_ref, m_ts):
    """One frame of far3d_track_records.  mem_hits (L,) int32 BEFORE the frame; idx (K,) the ranked rows and ranked_ids (K,) their ids
    after track_update (its mem_track[:K]); the boxes' query_idx / track_ids / keep (Kdec,) and boxes (Kdec, >= 3) f32; m_ref (L, 3) f32
    and m_ts (L,) f64 of the pre-updated memory.  Returns dict(mem_hits (L,) int32, age (Kdec,) int32, primary (Kdec,) bool,
    velocity (Kdec, 3) f32, velocity64 (Kdec, 3) f64: the same expression in float64 on the same inputs)."""
    old = np.asarray(mem_hits, dtype=np.int32).reshape(-1)
    idx = [int(r) for r in np.asarray(idx).reshape(-1)]
    ranked_ids = [int(i) for i in np.asarray(ranked_ids).reshape(-1)]
    K, L, P, A = len(idx), len(old), int(num_propagated), int(num_rows)
    assert len(ranked_ids) == K and P <= K <= L
    boxes = np.asarray(boxes, dtype=np.float32)
    m_ref = np.asarray(m_ref, dtype=np.float32).reshape(L, 3)
    m_ts = np.asarray(m_ts, dtype=np.float64).reshape(L)
    inherited = lambda r: row_start <= r < row_start + P and old[r - row_start] > 0
    hits, rank_of = [], {}
    for t, (r, tid) in enumerate(zip(idx, ranked_ids)):
        hits.append(int(old[r - row_start]) + 1 if inherited(r) else (1 if tid != 0 else 0))
        if 0 <= r < A:                                      # a row outside the plane matches no box (track_update step 4)
            rank_of[r] = t
    new = np.concatenate([np.asarray(hits, dtype=np.int32), old])[:L]
    query_idx = [int(q) for q in np.asarray(query_idx).reshape(-1)]
    track_ids = [int(i) for i in np.asarray(track_ids).reshape(-1)]
    keep = [bool(k) for k in np.asarray(keep).reshape(-1)]
    n = len(query_idx)
    age = np.full(n, -1, dtype=np.int32)
    primary = np.zeros(n, dtype=bool)
    vel = np.zeros((n, 3), dtype=np.float32)
    vel64 = np.zeros((n, 3), dtype=np.float64)
    seen = set()
    for j, (q, tid, kp) in enumerate(zip(query_idx, track_ids, keep)):
        rank = rank_of.get(q) if q >= 0 else None
        if tid != 0 and rank is not None:
            age[j] = hits[rank] - 1
        if tid != 0 and kp and tid not in seen:
            primary[j] = True
            seen.add(tid)
        if rank is not None and inherited(q):
            ts = float(m_ts[q - row_start])
            if ts > 0.0 and math.isfinite(ts):
                with np.errstate(all="ignore"):
                    vel[j] = (boxes[j, :3] - m_ref[q - row_start]) / np.float32(ts)          # fp32: one subtraction, one division
                    vel64[j] = (boxes[j, :3].astype(np.float64) - m_ref[q - row_start].astype(np.float64)) / ts
    return dict(mem_hits=new, age=age, primary=primary, velocity=vel, velocity64=vel64)


def track_records_frame(state, idx, score, num_rows, row_start, num_propagated, birth_thr, query_idx, keep, boxes, m_ref, m_ts):
    """The ids (tests/track_refs.track_frame) and then the records of one frame on a RecordState, updated in place.  Returns
    (ids of the ranked rows (K,), track_ids (Kdec,), the dict of records_frame)."""
    ids, track_ids = tr.track_frame(state, idx, score, row_start, num_propagated, birth_thr, query_idx)
    rec = records_frame(state.mem_hits, idx, ids, num_rows, row_start, num_propagated, query_idx, track_ids, keep, boxes, m_ref, m_ts)
    state.mem_hits = rec["mem_hits"]
    return ids, track_ids, rec


def velocity_within_bound(v, v64):
    """The velocity bound, elementwise: |v - v64| <= VEL_RTOL * |v64| (so an exact +0.0 is required wherever v64 is 0)."""
    v, v64 = np.asarray(v, dtype=np.float64), np.asarray(v64, dtype=np.float64)
    return bool((np.abs(v - v64) <= VEL_RTOL * np.abs(v64)).all())

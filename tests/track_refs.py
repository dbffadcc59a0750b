"""Track ids, restated on the CPU in plain Python and numpy: the contract of far3d_track_update (include/far3d_hip.h) and of
the query rows of far3d_decode_topk_tracked.  The GPU tests compare the kernels with this file exactly (they are integers)."""
import math

import numpy as np


class TrackState:
    """One scene stream's state: mem_track (L,) int64, one id per memory slot (0 = no identity), and the counter of the next id."""

    def __init__(self, L, next_id=1):
        self.mem_track = np.zeros(int(L), dtype=np.int64)
        self.next_id = int(next_id)

    def scene_reset(self):
        """What a scene change, reset_memory() or a fresh stream does: the ids go with the memory, the counter stays."""
        self.mem_track[:] = 0

    def reset_tracks(self):
        self.mem_track[:] = 0
        self.next_id = 1


def check_config(num_propagated, topk_proposals):
    if num_propagated > topk_proposals:
        raise ValueError("track: num_propagated=%d > topk_proposals=%d: a memory slot that was carried over would be propagated a second time "
                         "with the same id" % (num_propagated, topk_proposals))


def track_frame(state, idx, score, row_start, num_propagated, birth_thr=0.0, query_idx=None):
    """One frame.  idx (K,) the ranked query rows, score (A,) the score plane (probabilities; -inf in a hole), row_start the first
    propagated row, birth_thr a probability.  Updates state in place; returns (ids of the ranked rows (K,), track_ids (Kdec,) | None)."""
    idx = [int(r) for r in np.asarray(idx).reshape(-1)]
    score = np.asarray(score, dtype=np.float32).reshape(-1)
    K, L, P = len(idx), len(state.mem_track), int(num_propagated)
    check_config(P, K)
    assert K <= L
    old = state.mem_track.copy()
    thr = float(birth_thr)                                   # compared in float64, like the kernel
    ids, births = [], 0
    for r in idx:                                            # rank order
        tid = int(old[r - row_start]) if row_start <= r < row_start + P else 0          # step 1
        if tid == 0:                                                                    # step 2
            s = float(score[r])
            if math.isfinite(s) and s >= thr:
                tid = state.next_id + births
                births += 1
        ids.append(tid)
    state.next_id += births
    state.mem_track = np.concatenate([np.asarray(ids, dtype=np.int64), old])[:L]      # step 3
    track_ids = None
    if query_idx is not None:                                                         # step 4
        of_row = dict(zip(idx, ids))
        track_ids = np.asarray([of_row.get(int(q), 0) for q in np.asarray(query_idx).reshape(-1)], dtype=np.int64)
    return np.asarray(ids, dtype=np.int64), track_ids


def decode_query_rows(cls_last, K):
    """The decode's ranking on the CPU: a stable descending sort of the flat logits (ties: lower flat index first) -> the first K
    (flat index // num_classes, flat index % num_classes)."""
    cls_last = np.asarray(cls_last, dtype=np.float32)
    flat = cls_last.reshape(-1)
    order = np.argsort(-flat.astype(np.float64), kind="stable")[:K]
    return (order // cls_last.shape[1]).astype(np.int32), (order % cls_last.shape[1]).astype(np.int64)

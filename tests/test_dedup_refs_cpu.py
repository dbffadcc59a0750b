"""CPU: the duplicate-suppression contract (tests/dedup_refs.py) against itself -- the float64 overlap on cases with a known answer,
the greedy rule on hand-made chains, the input generator's promises, and the numpy fp32 restatement of the kernel's arithmetic
against the float64 overlaps on the generated inputs."""
import math

import numpy as np
import pytest

from tests import dedup_refs as dr



def box(x, y, d3, d4, yaw, code=7):
    b = np.zeros(code, dtype=np.float32)
    b[[0, 1, 3, 4, 5, 6]] = [x, y, d3, d4, 1.5, yaw]
    return b


# ------------------------------------------------------------------------------------------------ the float64 overlap
def test_analytic_overlaps():
    a = box(30.0, -70.0, 4.0, 1.0, 0.3)
    assert abs(dr.iou_bev64(a, a) - 1.0) < 1e-12
    assert abs(dr.iou_bev64(box(0, 0, 4, 1, 0.0), box(0, 0, 4, 1, math.pi / 2)) - 1.0 / 7.0) < 1e-7      # pi / 2 is rounded to fp32
    assert abs(dr.iou_bev64(box(5, 5, 1, 1, 0.0), box(5, 5, 1, 1, math.pi / 4)) - math.sqrt(2.0) / 2.0) < 1e-7
    assert dr.iou_bev64(box(0, 0, 2, 2, 0.0), box(2, 0, 2, 2, 0.0)) == 0.0                                # they share an edge
    assert dr.iou_bev64(box(0, 0, 2, 2, 0.0), box(2, 2, 2, 2, 0.0)) == 0.0                                # they share a corner
    assert dr.iou_bev64(box(0, 0, 2, 2, 0.3), box(9, 1, 2, 2, 1.0)) == 0.0                                # disjoint
    assert abs(dr.iou_bev64(box(0, 0, 2, 2, 0.0), box(1, 0, 2, 2, 0.0)) - 1.0 / 3.0) < 1e-12             # half of each
    assert abs(dr.iou_bev64(box(0, 0, 6, 2, 0.0), box(1, 0.5, 2, 1, 0.0)) - 2.0 / 12.0) < 1e-12          # one inside the other
    # d3 runs along the heading: turned by 90 degrees, a 4 x 1 box covers x in [-0.5, 0.5], y in [-2, 2]
    assert abs(dr.iou_bev64(box(0, 0, 4, 1, math.pi / 2), box(0, 1.5, 1, 1, 0.0)) - 1.0 / 4.0) < 1e-7


def test_overlap_is_symmetric_and_moves_with_the_pair():
    rng = np.random.default_rng(0)
    seen = 0
    for _ in range(60):
        a = box(*rng.uniform(-2, 2, size=2), *rng.uniform(0.5, 5.0, size=2), rng.uniform(-3, 3))
        b = box(*rng.uniform(-2, 2, size=2), *rng.uniform(0.5, 5.0, size=2), rng.uniform(-3, 3))
        o = dr.iou_bev64(a, b)
        assert abs(o - dr.iou_bev64(b, a)) < 1e-12
        # a common rigid motion, applied in float64 and kept in float64 rows (the reference reads what it is given)
        th, tx, ty = rng.uniform(-3, 3), *rng.uniform(-100, 100, size=2)
        def moved(r):
            m = r.astype(np.float64)
            x, y = float(r[0]), float(r[1])
            m[0], m[1], m[6] = math.cos(th) * x - math.sin(th) * y + tx, math.sin(th) * x + math.cos(th) * y + ty, float(r[6]) + th
            return m
        assert abs(o - dr.iou_bev64(moved(a), moved(b))) < 1e-9
        seen += 0.05 < o < 0.95
    assert seen > 10


# ------------------------------------------------------------------------------------------------ the greedy rule
def _chain(code=7):
    """Seven boxes.  0, 1, 2 in a row, 0.6 m apart, 2.4 x 1 m: neighbours hit (IoU 0.6, 0.6 m), 0 and 2 do not (1/3, 1.2 m).  3 on top
    of 0 but not kept; 4 on top of 0 with another label; 5 a NaN centre and 6 a zero extent, both on top of 0."""
    boxes = np.stack([box(10.0, 5.0, 2.4, 1.0, 0.0, code), box(10.6, 5.0, 2.4, 1.0, 0.0, code), box(11.2, 5.0, 2.4, 1.0, 0.0, code),
                      box(10.0, 5.0, 2.4, 1.0, 0.0, code), box(10.0, 5.0, 2.4, 1.0, 0.0, code), box(np.nan, 5.0, 2.4, 1.0, 0.0, code),
                      box(10.0, 5.0, 0.0, 1.0, 0.0, code)])
    scores = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3], dtype=np.float32)
    labels = np.array([1, 1, 1, 1, 2, 1, 1], dtype=np.int64)
    keep = np.array([1, 1, 1, 0, 1, 1, 1], dtype=bool)
    return boxes, scores, labels, keep


@pytest.mark.parametrize("mode, thr", [("iou_bev", 0.5), ("centre", 1.0)])
def test_greedy_rule_on_a_hand_made_chain(mode, thr):
    boxes, scores, labels, keep = _chain()
    r = dr.dedup(boxes, scores, labels, keep, mode, thr, class_aware=True)
    # 0 kills 1, so 2 (hit only by 1) lives; 3 is no candidate; 4 has another label; 5 and 6 cannot be judged and stay
    assert r["dup_keep"].tolist() == [True, False, True, False, True, True, True]
    assert r["dup_of"].tolist() == [-1, 0, -1, -1, -1, -1, -1]
    assert dr.saved_by_a_dead_suppressor(r).tolist() == [2]
    r = dr.dedup(boxes, scores, labels, keep, mode, thr, class_aware=False)
    assert r["dup_keep"].tolist() == [True, False, True, False, False, True, True] and r["dup_of"].tolist() == [-1, 0, -1, -1, 0, -1, -1]
    # the would-be suppressor 0 below score_thr: 1 lives and kills 2; 4 is below it too
    r = dr.dedup(boxes, np.array([0.2, 0.8, 0.7, 0.6, 0.1, 0.4, 0.3], dtype=np.float32), labels, keep, mode, thr, score_thr=0.25)
    assert r["dup_keep"].tolist() == [False, True, False, False, False, True, True] and r["dup_of"].tolist() == [-1, -1, 1, -1, -1, -1, -1]
    # 3 kept: hit by 0 like 1; a NaN score is no candidate
    r = dr.dedup(boxes, np.array([0.9, np.nan, 0.7, 0.6, 0.5, 0.4, 0.3], dtype=np.float32), labels, np.ones(7, dtype=bool), mode, thr)
    assert r["dup_keep"].tolist() == [True, False, True, False, True, True, True] and r["dup_of"].tolist() == [-1, -1, -1, 0, -1, -1, -1]


def _would_be_suppressors(code=7):
    """Seven boxes on four places 20 m apart.  Place A: 0 is not kept, 1 lies on it and nothing else hits 1.  Place B: 2 is kept but
    below the score threshold of the case (0.25), 3 lies on it.  Place C: 4 has a NaN heading, 5 lies on it.  Place D: 6 alone.
    With 0, 2 and 4 in force each would suppress the box on top of it; none of them is, so 1, 3 and 5 live."""
    boxes = np.stack([box(0.0, 0.0, 4.0, 2.0, 0.3, code), box(0.1, 0.0, 4.0, 2.0, 0.3, code), box(20.0, 0.0, 4.0, 2.0, 0.3, code),
                      box(20.1, 0.0, 4.0, 2.0, 0.3, code), box(40.0, 0.0, 4.0, 2.0, np.nan, code), box(40.0, 0.0, 4.0, 2.0, 0.3, code),
                      box(60.0, 0.0, 4.0, 2.0, 0.3, code)])
    scores = np.array([0.9, 0.8, 0.2, 0.7, 0.6, 0.5, 0.4], dtype=np.float32)
    labels = np.ones(7, dtype=np.int64)
    keep = np.array([0, 1, 1, 1, 1, 1, 1], dtype=bool)
    return boxes, scores, labels, keep


@pytest.mark.parametrize("mode, thr", [("iou_bev", 0.5), ("centre", 1.0)])
def test_a_box_that_is_no_candidate_suppresses_nobody(mode, thr):
    boxes, scores, labels, keep = _would_be_suppressors()
    r = dr.dedup(boxes, scores, labels, keep, mode, thr, score_thr=0.25)
    assert r["dup_keep"].tolist() == [False, True, False, True, True, True, True] and (r["dup_of"] == -1).all()
    # the same boxes with 0 kept and 2 above the threshold: 1 and 3 die, each of the box under it
    r = dr.dedup(boxes, scores, labels, np.ones(7, dtype=bool), mode, thr, score_thr=0.1)
    assert r["dup_keep"].tolist() == [True, False, True, False, True, True, True] and r["dup_of"].tolist() == [-1, 0, -1, 2, -1, -1, -1]


def test_dup_of_is_the_smallest_surviving_hitter():
    boxes = np.stack([box(0.0, 0, 2.4, 1, 0), box(1.2, 0, 2.4, 1, 0), box(0.6, 0, 2.4, 1, 0)])      # 0 and 1 apart, 2 between them
    r = dr.dedup(boxes, np.float32([0.9, 0.8, 0.7]), np.zeros(3, dtype=np.int64), np.ones(3, dtype=bool))
    assert r["dup_keep"].tolist() == [True, True, False] and r["dup_of"].tolist() == [-1, -1, 0]


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("K, seed", dr.INPUTS)
def test_generated_inputs_keep_their_margin_and_are_not_vacuous(K, seed):
    c = dr.generated(K, seed)
    assert c["boxes"].shape == (K, 7 + seed % 3) and c["boxes"].dtype == np.float32 and len(c["scores"]) == K
    assert (np.diff(c["scores"]) <= 0).all()
    ok = dr.judgeable(c["boxes"])
    assert (np.abs(c["boxes"][ok, :2]) <= 155.0).all() and (c["boxes"][ok, 3:5] >= 0.29).all() and (c["boxes"][ok, 3:5] <= 15.01).all()
    assert (~ok).any() and (~c["keep"]).any()
    cand = dr.candidates(c["scores"], c["keep"])
    for mode, thr in (("iou_bev", dr.IOU_THR), ("centre", dr.CENTRE_THR)):
        for ca in (True, False):
            r = dr.dedup(c["boxes"], c["scores"], c["labels"], c["keep"], mode, thr, ca)
            assert dr.margin_ok(r["overlaps"], r["judged"], mode, thr)
            sup, saved = int((cand & ~r["dup_keep"]).sum()), dr.saved_by_a_dead_suppressor(r)
            print("K=%d %s class_aware=%s: %d candidates, %d suppressed, %d saved by a dead suppressor" % (K, mode, ca, cand.sum(), sup, len(saved)))
            assert sup >= 0.3 * cand.sum() and r["dup_keep"].sum() >= 0.2 * cand.sum() and len(saved) >= 1
            assert (r["dup_keep"] <= cand).all() and ((r["dup_of"] >= 0) == (cand & ~r["dup_keep"])).all()


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in fp32
def test_fp32_restatement_stays_within_a_quarter_of_the_margin():
    """The largest error seen goes into profiles/dedup/README.md."""
    worst = {}
    for K, seed in dr.INPUTS:
        c = dr.generated(K, seed)
        for mode, thr in (("iou_bev", dr.IOU_THR), ("centre", dr.CENTRE_THR)):
            r = dr.dedup(c["boxes"], c["scores"], c["labels"], c["keep"], mode, thr, class_aware=False)
            got = dr.overlaps_f32(c["boxes"], r["judged"], mode)
            assert got.dtype == np.float32 and not got[~r["judged"]].any()
            worst[mode] = max(worst.get(mode, 0.0), dr.overlap_error(got, r["overlaps"], mode, thr))
            assert (dr.hits(got.astype(np.float64), r["judged"], mode, thr) == r["hits"]).all()
    print("fp32 restatement, largest error: iou_bev %.3e (absolute), centre %.3e (relative d^2); bound %.3e" %
          (worst["iou_bev"], worst["centre"], dr.MARGIN / 4))
    assert worst["iou_bev"] < dr.MARGIN / 4 and worst["centre"] < dr.MARGIN / 4


def test_fp32_restatement_on_the_degenerate_pairs():
    """Identical boxes, shared edges, a shared corner, one box inside the other, the crossed pair and the turned square: the pieces of
    boundary two rectangles share are counted once."""
    pairs = [(box(30, -70, 4, 1, 0.3), box(30, -70, 4, 1, 0.3)), (box(-149, 149, 15, 0.3, -2.0), box(-149, 149, 15, 0.3, -2.0)),
             (box(0, 0, 2, 2, 0), box(2, 0, 2, 2, 0)), (box(0, 0, 2, 2, 0), box(0, -2, 2, 2, 0)), (box(0, 0, 2, 2, 0), box(2, 2, 2, 2, 0)),
             (box(0, 0, 2, 2, 0), box(1, 0, 2, 2, 0)), (box(0, 0, 6, 2, 0), box(1, 0.5, 2, 1, 0)), (box(1, 0.5, 2, 1, 0), box(0, 0, 6, 2, 0)),
             (box(0, 0, 6, 2, 0), box(2, 0, 2, 2, 0)), (box(0, 0, 4, 1, 0), box(0, 0, 4, 1, math.pi / 2)),
             (box(5, 5, 1, 1, 0), box(5, 5, 1, 1, math.pi / 4)), (box(0, 0, 2, 2, math.pi / 2), box(0, 2, 2, 2, 0))]
    for a, b in pairs:
        boxes = np.stack([a, b])
        J = np.array([[False, False], [True, False]])
        want = dr.overlaps64(boxes, J, "iou_bev")[1, 0]
        got = dr.overlaps_f32(boxes, J, "iou_bev")[1, 0]
        assert abs(float(got) - want) < 1e-6, (a, b, got, want)

"""Duplicate suppression, restated on the CPU: the contract of far3d_box_dedup (include/far3d_hip.h) in float64, the kernel's own
fp32 arithmetic in numpy, and the generator of the tests' inputs.

The rule.  Inputs in the decode's order: boxes (Kdec, >= 7) f32 rows (x, y, z, d3, d4, h, yaw, ...), scores (Kdec) f32, labels (Kdec)
int64, keep (Kdec).  A box is a CANDIDATE iff keep != 0, its score is finite and (double)score >= score_thr.  Its FOOTPRINT is the
rectangle centred at (x, y) that extends d3 along (cos yaw, sin yaw) and d4 along (-sin yaw, cos yaw).  A candidate with a non-finite
x, y, d3, d4, yaw or with d3 <= 0 or d4 <= 0 is UNJUDGEABLE: it neither suppresses nor is suppressed.  A JUDGED pair is (j, i), j < i,
both judgeable candidates, with equal labels if class_aware.  Its overlap o: 'iou_bev' the IoU of the footprints, a hit iff o > thr;
'centre' the squared distance of the centres, a hit iff o < thr * thr.  Greedy in index order: box i is suppressed iff a surviving
j < i hits it.  dup_keep: 1 exactly for candidates that are not suppressed; dup_of: the smallest surviving j that hit i, else -1.

The contract is exact mathematics on the fp32 inputs; `dedup` evaluates it in float64, the intersection of two footprints as the
intersection of two convex polygons (Sutherland-Hodgman) and its area by the shoelace sum.  A kernel in fp32 can only agree on inputs
whose judged pairs keep a distance from the threshold: `clustered_boxes` produces such inputs (MARGIN, a condition on INPUTS), and
`overlaps_f32` -- the kernel's arithmetic, line by line, in numpy float32 -- must stay within MARGIN / 4 of the float64 overlaps on
them, so that no rounding of that size can flip a decision."""
import math

import numpy as np

MODES = ("iou_bev", "centre")
MARGIN = 1e-3          # |o - thr| >= MARGIN (IoU);  |o - thr^2| >= MARGIN * thr^2 (centre, o in m^2)


# ------------------------------------------------------------------------------------------------ float64: the contract
def corners64(box):
    """The footprint's corners, counter-clockwise, float64 (4, 2)."""
    x, y, d3, d4, yaw = (float(box[k]) for k in (0, 1, 3, 4, 6))
    c, s = math.cos(yaw), math.sin(yaw)
    ux, uy, vx, vy = 0.5 * d3 * c, 0.5 * d3 * s, -0.5 * d4 * s, 0.5 * d4 * c
    return np.array([[x + ux + vx, y + uy + vy], [x - ux + vx, y - uy + vy], [x - ux - vx, y - uy - vy], [x + ux - vx, y + uy - vy]])


def _clip(poly, a, b):
    """poly (list of points) against the half-plane left of a -> b (closed)."""
    out = []
    ex, ey = b[0] - a[0], b[1] - a[1]
    side = [ex * (p[1] - a[1]) - ey * (p[0] - a[0]) for p in poly]
    for k, p in enumerate(poly):
        q, sp, sq = poly[(k + 1) % len(poly)], side[k], side[(k + 1) % len(poly)]
        if sp >= 0:
            out.append(p)
        if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
            t = sp / (sp - sq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def _area(poly):
    return 0.5 * sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[k][1] * poly[(k + 1) % len(poly)][0] for k in range(len(poly)))


def iou_bev64(box_j, box_i):
    """IoU of the two footprints in float64; the polygons are moved to box_j's centre first (a translation: exact mathematics)."""
    pj, pi = corners64(box_j), corners64(box_i)
    org = np.array([float(box_j[0]), float(box_j[1])])
    poly = [tuple(p) for p in (pi - org)]
    q = pj - org
    for k in range(4):
        poly = _clip(poly, q[k], q[(k + 1) % 4])
        if len(poly) < 3:
            return 0.0
    inter = max(_area(poly), 0.0)
    aj, ai = float(box_j[3]) * float(box_j[4]), float(box_i[3]) * float(box_i[4])
    return inter / (aj + ai - inter)


def candidates(scores, keep, score_thr=0.0):
    sc = np.asarray(scores, dtype=np.float32).astype(np.float64)
    return (np.asarray(keep) != 0) & np.isfinite(sc) & (np.where(np.isfinite(sc), sc, -1.0) >= float(score_thr))


def judgeable(boxes):
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.isfinite(b[:, [0, 1, 3, 4, 6]]).all(axis=1) & (b[:, 3] > 0) & (b[:, 4] > 0)


def judged_pairs(boxes, scores, labels, keep, class_aware=True, score_thr=0.0):
    """(Kdec, Kdec) bool: [i][j] is a judged pair (j < i)."""
    act = candidates(scores, keep, score_thr) & judgeable(boxes)
    lab = np.asarray(labels, dtype=np.int64)
    J = act[:, None] & act[None, :] & np.tri(len(act), k=-1, dtype=bool)
    if class_aware:
        J &= lab[:, None] == lab[None, :]
    return J


def pair_overlaps64(boxes, ii, jj, mode):
    """The float64 overlap of the pairs (jj[n], ii[n]).  IoU: two footprints whose centres are further apart than the sum of their
    circumradii are disjoint, their IoU is exactly 0 -- those pairs are not clipped."""
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    d2 = (b[ii, 0] - b[jj, 0]) ** 2 + (b[ii, 1] - b[jj, 1]) ** 2
    if mode == "centre":
        return d2
    rad = 0.5 * np.hypot(b[:, 3], b[:, 4])
    o = np.zeros(len(ii), dtype=np.float64)
    for n in np.nonzero(np.sqrt(d2) <= rad[ii] + rad[jj])[0]:
        o[n] = iou_bev64(b[jj[n]], b[ii[n]])
    return o


def overlaps64(boxes, judged, mode):
    """(Kdec, Kdec) float64: the overlap of every judged pair, 0 elsewhere."""
    O = np.zeros(judged.shape, dtype=np.float64)
    ii, jj = np.nonzero(judged)
    if len(ii):
        O[ii, jj] = pair_overlaps64(boxes, ii, jj, mode)
    return O


def clear_of(o, mode, thr):
    """No overlap of o within MARGIN of the threshold."""
    return bool((np.abs(o - thr) >= MARGIN).all()) if mode == "iou_bev" else bool((np.abs(o - thr * thr) >= MARGIN * thr * thr).all())


def hits(O, judged, mode, thr):
    return judged & ((O > thr) if mode == "iou_bev" else (O < float(thr) * float(thr)))


def greedy(H, cand):
    """H (Kdec, Kdec) bool hits [i][j], cand (Kdec) -> (dup_keep bool, dup_of int32)."""
    n = len(cand)
    alive, of = np.array(cand, dtype=bool), np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if alive[i]:
            js = np.nonzero(H[i, :i] & alive[:i])[0]
            if len(js):
                alive[i], of[i] = False, js[0]
    return alive, of


def dedup(boxes, scores, labels, keep, mode="iou_bev", thr=0.5, class_aware=True, score_thr=0.0):
    """The contract in float64 -> dict(dup_keep, dup_of, overlaps (Kdec, Kdec) f64, judged, hits)."""
    assert mode in MODES
    J = judged_pairs(boxes, scores, labels, keep, class_aware, score_thr)
    O = overlaps64(boxes, J, mode)
    H = hits(O, J, mode, thr)
    dk, of = greedy(H, candidates(scores, keep, score_thr))
    return dict(dup_keep=dk, dup_of=of, overlaps=O, judged=J, hits=H)


def saved_by_a_dead_suppressor(res):
    """Indices of the boxes that live only because a box that hits them was itself suppressed."""
    dead = ~res["dup_keep"]
    return np.nonzero(res["dup_keep"] & (res["hits"] & dead[None, :]).any(axis=1))[0]


def margin_ok(O, judged, mode, thr):
    """No judged pair within MARGIN of the threshold."""
    return clear_of(O[judged], mode, thr)


def overlap_error(got, O, mode, thr):
    """The largest error of fp32 overlaps `got` against the float64 O, in the margin's unit: absolute in IoU, relative to the pair's
    own d^2 in centre mode (a 0 must be a 0).  Below MARGIN / 4 no decision of an input with the margin property can flip: IoU is
    plain; centre, o >= thr^2 (1 + MARGIN) gives got >= o (1 - MARGIN / 4) > thr^2, and o <= thr^2 (1 - MARGIN) gives got < thr^2."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - O)
    if not err.size:
        return 0.0
    if mode == "iou_bev":
        return float(err.max())
    if (err[O == 0] != 0).any():
        return float("inf")
    return float((err[O > 0] / O[O > 0]).max()) if (O > 0).any() else 0.0


# ------------------------------------------------------------------------------------------------ fp32: the kernel's arithmetic
_f = np.float32


def _clip_closed(g0, g1, same, t0, t1, ok):
    out, on = (g0 < 0) & (g1 < 0), (g0 == 0) & (g1 == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = g0 / (g0 - g1)
    ok = np.where(out, False, np.where(on, ok & same, ok))
    enter, leave = ~out & ~on & (g0 < 0), ~out & ~on & ~(g0 < 0) & (g1 < 0)
    return np.where(enter, np.maximum(t0, t), t0), np.where(leave, np.minimum(t1, t), t1), ok


def _clip_open(f0, f1, t0, t1, ok):
    out = (f0 <= 0) & (f1 <= 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = f0 / (f0 - f1)
    enter, leave = ~out & (f0 <= 0), ~out & ~(f0 <= 0) & (f1 <= 0)
    return np.where(enter, np.maximum(t0, t), t0), np.where(leave, np.minimum(t1, t), t1), ok & ~out


def _piece(x0, y0, x1, y1, t0, t1, ok, ox, oy):
    ex, ey = x1 - x0, y1 - y0
    sx, sy, fx, fy = x0 + t0 * ex - ox, y0 + t0 * ey - oy, x0 + t1 * ex - ox, y0 + t1 * ey - oy
    return np.where(ok & (t1 > t0), sx * fy - sy * fx, _f(0))


def iou_local_f32(a, b, lx, ly, cr, sr, hx, hy):
    """csrc/dedup.hip dd_iou_local on arrays of pairs, float32 throughout: Q = [-a, a] x [-b, b], P centred (lx, ly), half extents
    hx, hy, turned by (cr, sr).  The boundary of P n Q = P's edges inside the closed Q + Q's edges inside the open P; area by Green."""
    ux, uy, vx, vy = hx * cr, hx * sr, -hy * sr, hy * cr
    px = [lx + ux + vx, lx - ux + vx, lx - ux - vx, lx + ux - vx]
    py = [ly + uy + vy, ly - uy + vy, ly - uy - vy, ly + uy - vy]
    qx, qy = [a, a, -a, -a], [-b, b, b, -b]
    areaQ, areaP = _f(4) * a * b, _f(4) * hx * hy
    small = areaP < areaQ
    ox, oy = np.where(small, lx, _f(0)), np.where(small, ly, _f(0))
    acc = np.zeros_like(a)
    one, zero = np.ones_like(a), np.zeros_like(a)
    for k in range(4):
        x0, y0, x1, y1 = px[k], py[k], px[(k + 1) & 3], py[(k + 1) & 3]
        t0, t1, ok = zero, one, np.ones(a.shape, dtype=bool)
        t0, t1, ok = _clip_closed(a - x0, a - x1, y1 > y0, t0, t1, ok)
        t0, t1, ok = _clip_closed(b - y0, b - y1, x1 < x0, t0, t1, ok)
        t0, t1, ok = _clip_closed(x0 + a, x1 + a, y1 < y0, t0, t1, ok)
        t0, t1, ok = _clip_closed(y0 + b, y1 + b, x1 > x0, t0, t1, ok)
        acc = acc + _piece(x0, y0, x1, y1, t0, t1, ok, ox, oy)
    f = [[None] * 4 for _ in range(4)]
    for k in range(4):
        ex, ey = px[(k + 1) & 3] - px[k], py[(k + 1) & 3] - py[k]
        for m in range(4):
            f[k][m] = ex * (qy[m] - py[k]) - ey * (qx[m] - px[k])
    for m in range(4):
        t0, t1, ok = zero, one, np.ones(a.shape, dtype=bool)
        for k in range(4):
            t0, t1, ok = _clip_open(f[k][m], f[k][(m + 1) & 3], t0, t1, ok)
        acc = acc + _piece(qx[m], qy[m], qx[(m + 1) & 3], qy[(m + 1) & 3], t0, t1, ok, ox, oy)
    inter = np.minimum(np.maximum(_f(0.5) * acc, _f(0)), np.minimum(areaP, areaQ))
    return inter / (areaP + areaQ - inter)


def overlaps_f32(boxes, judged, mode):
    """(Kdec, Kdec) float32: what the kernel computes for every judged pair (its overlap_out), 0 elsewhere."""
    b = np.asarray(boxes, dtype=np.float32)
    O = np.zeros(judged.shape, dtype=np.float32)
    ii, jj = np.nonzero(judged)
    if len(ii) == 0:
        return O
    with np.errstate(invalid="ignore"):      # an unjudgeable box is in no pair
        hx, hy, cs, sn = _f(0.5) * b[:, 3], _f(0.5) * b[:, 4], np.cos(b[:, 6]), np.sin(b[:, 6])
    assert hx.dtype == np.float32 and cs.dtype == np.float32
    rad = np.sqrt(hx * hx + hy * hy)
    dx, dy = b[ii, 0] - b[jj, 0], b[ii, 1] - b[jj, 1]
    d2 = dx * dx + dy * dy
    if mode == "centre":
        O[ii, jj] = d2
        return O
    rs = rad[ii] + rad[jj]
    near = d2 <= rs * rs
    ii, jj, dx, dy = ii[near], jj[near], dx[near], dy[near]
    cj, sj, ci, si = cs[jj], sn[jj], cs[ii], sn[ii]
    o = iou_local_f32(hx[jj], hy[jj], cj * dx + sj * dy, cj * dy - sj * dx, ci * cj + si * sj, si * cj - ci * sj, hx[ii], hy[ii])
    assert o.dtype == np.float32
    O[ii, jj] = o
    return O


# ------------------------------------------------------------------------------------------------ inputs
IOU_THR, CENTRE_THR = 0.5, 1.0      # the thresholds the generated inputs keep their margin from


def clustered_boxes(rng, Kdec, code=7, iou_thr=IOU_THR, centre_thr=CENTRE_THR, num_labels=4, tries=200):
    """Kdec boxes as a decode could leave them: AV2-like extents 0.3 - 15 m, centres within +-150 m, objects in clusters of 1 - 5 with
    jitter in centre, size and heading, the members of a cluster mostly of one label; descending scores; a few boxes not kept, a few
    unjudgeable (NaN, zero extent).  Every box is drawn again until none of its pairs with the boxes in front of it -- judgeable
    candidates, whatever their labels -- lies within MARGIN of iou_thr in IoU or of centre_thr^2 in squared centre distance: the
    inputs serve both modes, class-aware or not.  No box is left out.  Returns dict(boxes f32, scores f32, labels i64, keep bool)."""
    owner = []
    while len(owner) < Kdec:
        owner += [len(owner)] * int(rng.integers(1, 6))
    owner = np.asarray(owner[:Kdec])[rng.permutation(Kdec)]
    base = {}
    for o in np.unique(owner):
        ext = np.exp(rng.uniform(math.log(0.3), math.log(15.0), size=2))
        base[int(o)] = dict(c=rng.uniform(-150.0, 150.0, size=2), d=ext, yaw=rng.uniform(-math.pi, math.pi), lab=int(rng.integers(0, num_labels)),
                            chain=rng.random() < 0.3, n=0)
        if base[int(o)]["chain"]:      # a row of boxes 2.4 thr long, 0.6 thr apart along the heading: neighbours hit each other in both
            base[int(o)]["d"] = np.array([2.4 * centre_thr, rng.uniform(0.5, 2.0)])      # modes (IoU 0.6), the next but one does not (1/3)
    scores = np.sort(rng.uniform(0.05, 0.95, size=Kdec).astype(np.float32))[::-1].copy()
    keep = rng.random(Kdec) < 0.9
    labels = np.asarray([base[int(o)]["lab"] if rng.random() < 0.8 else int(rng.integers(0, num_labels)) for o in owner], dtype=np.int64)
    boxes = np.zeros((Kdec, code), dtype=np.float32)
    bad = rng.random(Kdec) < 0.03
    act = np.zeros(Kdec, dtype=bool)
    for i in range(Kdec):
        g = base[int(owner[i])]
        for _ in range(tries):
            row = np.zeros(code)
            row[2] = rng.uniform(-2.0, 2.0)
            row[5] = rng.uniform(0.5, 4.0)
            if g["chain"]:
                step = 0.6 * centre_thr * g["n"]
                row[0:2] = g["c"] + step * np.array([math.cos(g["yaw"]), math.sin(g["yaw"])]) + rng.normal(0.0, 0.02, size=2)
                row[3:5] = g["d"] * np.exp(rng.normal(0.0, 0.01, size=2))
                row[6] = g["yaw"] + rng.normal(0.0, 0.01)
            else:
                s = float(min(g["d"].min(), 2.0 * centre_thr))
                row[0:2] = g["c"] + rng.normal(0.0, 0.14, size=2) * s
                row[3:5] = np.clip(g["d"] * np.exp(rng.normal(0.0, 0.08, size=2)), 0.3, 15.0)
                row[6] = g["yaw"] + rng.normal(0.0, 0.05) + (math.pi / 2 if rng.random() < 0.05 else 0.0)
            row[6] = (row[6] + math.pi) % (2.0 * math.pi) - math.pi
            if code > 7:
                row[7:] = rng.normal(0.0, 3.0, size=code - 7)
            boxes[i] = row.astype(np.float32)
            if bad[i]:
                boxes[i, [0, 3, 4, 6][int(rng.integers(0, 4))]] = [np.nan, 0.0, -1.0, np.inf][int(rng.integers(0, 4))]
            act[i] = keep[i] and bool(judgeable(boxes[i:i + 1])[0])
            if not act[i]:
                break
            jj = np.nonzero(act[:i])[0]
            ii = np.full(len(jj), i)
            if clear_of(pair_overlaps64(boxes[:i + 1], ii, jj, "iou_bev"), "iou_bev", iou_thr) and \
                    clear_of(pair_overlaps64(boxes[:i + 1], ii, jj, "centre"), "centre", centre_thr):
                break
        else:
            raise RuntimeError("clustered_boxes: box %d found no place clear of the thresholds in %d tries" % (i, tries))
        g["n"] += 1
    return dict(boxes=boxes, scores=scores, labels=labels, keep=keep)


# the inputs of the tests, (Kdec, seed): 65 and 129 put a box first in a second and a third mask word, 300 is the engine's max_num,
# 1024 the kernel's limit; three streams of 40.  The seeds are chosen so that every one is non-vacuous in both modes, class-aware or not
# (tests/test_dedup_refs_cpu.py asserts it)
INPUTS = ((65, 65), (129, 129), (300, 300), (1024, 1024), (40, 1), (40, 3), (40, 17))
_GENERATED = {}


def generated(K, seed):
    """clustered_boxes(default_rng(seed), K) with 7 + seed % 3 floats per box, made once per process; do not write to it."""
    if (K, seed) not in _GENERATED:
        _GENERATED[K, seed] = clustered_boxes(np.random.default_rng(seed), K, code=7 + seed % 3)
    return _GENERATED[K, seed]

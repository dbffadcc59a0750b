"""GPU: far3d_track_records against its CPU restatement (tests/track_record_refs.py) at the smallest shapes where it can go wrong --
the integers (mem_hits, age, primary) exactly, the velocity within VEL_RTOL of the float64 evaluation of the same fp32 inputs (the
bound is derived in track_record_refs, not measured) -- and every refusal of the entry by name, in front of any launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import track_record_refs as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _stream_case(rng, A, K, L, P, Kdec, code=7, out_of_plane=(), old=None):
    """One stream's inputs as track_update would leave them, random: a consistent old state (hits > 0 exactly where an id sits), K
    distinct ranked rows (the ranks in out_of_plane get rows outside [0, A)), half of the id-less ranks born; boxes of ranked and of
    unranked queries with duplicates, random keep flags; m_ts with zeros, negatives, NaN and inf among the seconds.  old: the (id queue,
    hits plane) the frame starts from, in place of random ones."""
    row0 = A - P
    if old is None:
        old_track = np.where(rng.random(L) < 0.6, rng.integers(1, 10 ** 6, size=L), 0).astype(np.int64)
        old_hits = np.where(old_track != 0, rng.integers(1, 50, size=L), 0).astype(np.int32)
    else:
        old_track, old_hits = np.asarray(old[0], dtype=np.int64), np.asarray(old[1], dtype=np.int32)
    idx = rng.permutation(A)[:K].astype(np.int64)
    for n, t in enumerate(out_of_plane):
        idx[t] = (A + 5 + n) if n % 2 == 0 else -(n + 1)
    ids = np.zeros(K, dtype=np.int64)
    for t, r in enumerate(idx):
        if row0 <= r < row0 + P and old_track[r - row0] != 0:
            ids[t] = old_track[r - row0]
        elif 0 <= r < A and rng.random() < 0.5:
            ids[t] = 10 ** 6 + int(rng.integers(0, 10 ** 6)) * 1024 + t
    track = np.concatenate([ids, old_track])[:L]
    query = np.where(rng.random(Kdec) < 0.8, idx[rng.integers(0, K, size=Kdec)], rng.integers(0, A, size=Kdec))
    query = np.clip(query, 0, A - 1).astype(np.int32)
    of_row = {int(r): int(i) for r, i in zip(idx, ids) if 0 <= r < A}
    tids = np.asarray([of_row.get(int(q), 0) for q in query], dtype=np.int64)
    keep = rng.random(Kdec) < 0.7
    boxes = rng.uniform(-50.0, 50.0, size=(Kdec, code)).astype(np.float32)
    m_ref = rng.uniform(-50.0, 50.0, size=(L, 3)).astype(np.float32)
    m_ts = rng.uniform(0.05, 0.6, size=L)
    special = rng.permutation(L)[:max(4, L // 8)]
    m_ts[special] = rng.choice([0.0, -0.1, np.nan, np.inf], size=len(special))
    return dict(A=A, K=K, L=L, P=P, row0=row0, idx=idx, track=track, hits=old_hits, query=query, tids=tids, keep=keep, boxes=boxes,
                m_ref=m_ref, m_ts=m_ts)


def _want(c):
    return rr.records_frame(c["hits"], c["idx"], c["track"][:c["K"]], c["A"], c["row0"], c["P"], c["query"], c["tids"], c["keep"], c["boxes"],
                            c["m_ref"], c["m_ts"])


def _gpu(cases, pad=0):
    """ops.track_records on B streams (pad > 0: every operand a view into a buffer `pad` elements wider per stream, filled with a
    sentinel that must survive).  Returns (mem_hits, age, primary, velocity) as numpy, leading B."""
    from far3d_amd import ops
    def dev(key, dtype):
        a = torch.tensor(np.stack([c[key] for c in cases]), dtype=dtype)
        if not pad:
            return a.to(DEV), None
        flat = a.reshape(a.shape[0], -1)
        wide = torch.full((flat.shape[0], flat.shape[1] + pad), 1, dtype=dtype)
        wide[:, :flat.shape[1]] = flat
        wide = wide.to(DEV)
        return wide[:, :flat.shape[1]].view(a.shape), wide
    ops_in = {k: dev(k, dt) for k, dt in (("idx", torch.int64), ("track", torch.int64), ("hits", torch.int32), ("query", torch.int32),
                                          ("tids", torch.int64), ("keep", torch.bool), ("boxes", torch.float32), ("m_ref", torch.float32),
                                          ("m_ts", torch.float64))}
    t = {k: v[0] for k, v in ops_in.items()}
    c = cases[0]
    age, prim, vel = ops.track_records(t["idx"], t["track"], t["hits"], t["query"], t["tids"], t["keep"], t["boxes"], t["m_ref"], t["m_ts"],
                                       c["A"], c["row0"], c["P"])
    torch.cuda.synchronize()
    assert age.dtype == torch.int32 and prim.dtype == torch.bool and vel.dtype == torch.float32
    for k, (view, wide) in ops_in.items():
        if wide is not None:
            n = view[0].numel()
            assert bool((wide[:, n:] == 1).all()), "%s: the padding between the streams was written" % k
        if k != "hits":
            same = torch.tensor(np.stack([c[k] for c in cases]), dtype=view.dtype).numpy().tobytes()      # bytes: m_ts holds NaNs
            assert view.cpu().contiguous().numpy().tobytes() == same, "%s: an input was written" % k
    return t["hits"].cpu().numpy(), age.cpu().numpy(), prim.cpu().numpy(), vel.cpu().numpy()


def _check(cases, got, tag=""):
    hits, age, prim, vel = got
    for b, c in enumerate(cases):
        w = _want(c)
        assert hits[b].tolist() == w["mem_hits"].tolist(), "%s stream %d: mem_hits" % (tag, b)
        assert age[b].tolist() == w["age"].tolist(), "%s stream %d: track_age" % (tag, b)
        assert prim[b].tolist() == w["primary"].tolist(), "%s stream %d: track_primary" % (tag, b)
        err = np.abs(vel[b].astype(np.float64) - w["velocity64"])
        rel = err[w["velocity64"] != 0] / np.abs(w["velocity64"][w["velocity64"] != 0])
        print("%s stream %d: velocity max rel err %.3e (bound %.3e), %d moving boxes" %
              (tag, b, rel.max() if rel.size else 0.0, rr.VEL_RTOL, int((w["velocity64"] != 0).any(axis=1).sum())))
        assert rr.velocity_within_bound(vel[b], w["velocity64"]), "%s stream %d: track_velocity" % (tag, b)
        still = ~(w["velocity64"] != 0).any(axis=1)
        assert not vel[b][still].any() and not np.signbit(vel[b][still]).any(), "%s stream %d: a box without velocity is not +0.0" % (tag, b)
        ids = c["tids"][prim[b]]
        assert len(set(ids.tolist())) == len(ids) and (ids != 0).all(), "%s stream %d: two primaries of one id" % (tag, b)
        assert ((hits[b] > 0) == (c["track"] != 0)).all(), "%s stream %d: hits > 0 must hold exactly where an id sits" % (tag, b)
    return got


# ------------------------------------------------------------------------------------------ shape A: designed
def _designed(ts2):
    """K=5, Kdec=7, L=12, P=3, A=9 (row0 = 6): tails of the 4-wide row scan, a partial wave.  Slot 0 holds id 11 (3 hits), slot 1
    none, slot 2 id 13 (1 hit) whose m_ts is ts2."""
    idx = np.array([6, 2, 40, 7, 8], dtype=np.int64)                   # inherited, a birth, outside the plane, unborn, inherited
    ids = np.array([11, 100, 0, 0, 13], dtype=np.int64)
    old_track = np.array([11, 0, 13, 5, 0, 6, 7, 0, 0, 0, 0, 0], dtype=np.int64)
    old_hits = np.array([3, 0, 1, 2, 0, 1, 4, 0, 0, 0, 0, 0], dtype=np.int32)
    query = np.array([6, 6, 2, 8, 8, 4, 7], dtype=np.int32)            # two boxes of row 6 and of row 8; row 4 unranked; row 7 has no id
    tids = np.array([11, 11, 100, 13, 13, 0, 0], dtype=np.int64)
    keep = np.array([1, 1, 1, 0, 1, 1, 1], dtype=bool)                 # the better box of id 13 is not kept
    boxes = np.zeros((7, 7), dtype=np.float32)
    boxes[:, :3] = [[10.3, 19.85, 1.025]] * 2 + [[1.0, 2.0, 3.0]] * 5
    boxes[:, 3:] = 9.0
    m_ref = np.zeros((12, 3), dtype=np.float32)
    m_ref[0] = [10.0, 20.0, 1.0]                                       # (3.0, -1.5, 0.25) m/s over 0.1 s
    m_ref[2] = [0.5, 0.5, 0.5]
    m_ts = np.full(12, 0.1)
    m_ts[2] = ts2
    return dict(A=9, K=5, L=12, P=3, row0=6, idx=idx, track=np.concatenate([ids, old_track])[:12], hits=old_hits, query=query, tids=tids,
                keep=keep, boxes=boxes, m_ref=m_ref, m_ts=m_ts)


@pytest.mark.parametrize("ts2", [0.25, 0.0, float("nan"), float("inf"), -0.1])
def test_designed_small_shape(ts2):
    c = _designed(ts2)
    hits, age, prim, vel = _check([c], _gpu([c]), "designed")
    assert hits[0].tolist() == [4, 1, 0, 0, 2, 3, 0, 1, 2, 0, 1, 4]
    assert age[0].tolist() == [3, 3, 0, 1, 1, -1, -1]
    assert prim[0].tolist() == [True, False, True, False, True, False, False]
    v64 = (np.float32([10.3, 19.85, 1.025]).astype(np.float64) - [10.0, 20.0, 1.0]) / 0.1
    assert np.allclose(v64, [3.0, -1.5, 0.25], rtol=1e-5)
    assert np.array_equal(vel[0, 0], vel[0, 1]) and (np.abs(vel[0, 0] - v64) <= rr.VEL_RTOL * np.abs(v64)).all()
    if ts2 == 0.25:
        assert (np.abs(vel[0, 3] - np.array([2.0, 6.0, 10.0])) <= rr.VEL_RTOL * np.array([2.0, 6.0, 10.0])).all()
        assert np.array_equal(vel[0, 3], vel[0, 4])
    else:
        assert not vel[0, 2:].any()


# ------------------------------------------------------------------------------------------ shape B: the limits
def test_limits_k1024_l4096_two_frames():
    """K = Kdec = 1024, L = 4096, A = 2000, P = 1024: all 16 waves, every LDS array full; the second frame starts from the plane the
    first one wrote."""
    rng = np.random.default_rng(21)
    c = _stream_case(rng, 2000, 1024, 4096, 1024, 1024, code=7, out_of_plane=(3, 500, 1023))
    hits, age, prim, vel = _check([c], _gpu([c]), "limits frame 0")
    assert (age[0] > 0).sum() > 100 and prim[0].sum() > 100 and vel[0].any(axis=1).sum() > 100
    c2 = _stream_case(rng, 2000, 1024, 4096, 1024, 1024, code=10, old=(c["track"], hits[0]))      # frame 1 on frame 0's result
    hits2, age2, _, _ = _check([c2], _gpu([c2]), "limits frame 1")
    assert age2[0].max() >= 2 and hits2[0][1024:].tolist() == hits[0][:3072].tolist()


# ------------------------------------------------------------------------------------------ streams
def test_three_streams_with_padded_strides_equal_their_own_launches():
    rng = np.random.default_rng(4)
    cases = [_stream_case(rng, 90, 20, 64, 16, 30, code=9, out_of_plane=(b,)) for b in range(3)]
    alone = [_gpu([c]) for c in cases]
    for pad in (0, 5):
        got = _check(cases, _gpu(cases, pad=pad), "B=3 pad=%d" % pad)
        for b in range(3):
            for g, a in zip(got, alone[b]):
                assert g[b].tobytes() == a[0].tobytes(), "stream %d differs from its own one-stream launch" % b


def test_no_decoded_boxes_still_shifts_the_counters():
    rng = np.random.default_rng(9)
    c = _stream_case(rng, 40, 8, 32, 8, 0)
    hits, age, prim, vel = _check([c], _gpu([c]), "Kdec=0")
    assert age.shape == (1, 0) and vel.shape == (1, 0, 3)


# ------------------------------------------------------------------------------------------ refusals
NAMES = ("topk_idx", "mem_track", "query_idx", "track_ids", "keep", "boxes", "m_ref", "m_ts", "mem_hits", "track_age", "track_primary",
         "track_velocity")


def _raw(B=1, A=9, K=5, L=12, Kdec=7, row0=6, P=3, box_stride=7, null=None, strides=None, no_strides=False):
    """The C entry on zeroed operands of the designed shape; returns (status, message, the operands)."""
    from far3d_amd import lib as _lib
    lib = _lib.require_device()
    n = max(B, 1)
    dts = (torch.int64, torch.int64, torch.int32, torch.int64, torch.uint8, torch.float32, torch.float32, torch.float64, torch.int32,
           torch.int32, torch.uint8, torch.float32)
    ext = (5, 12, 7, 7, 7, 49, 36, 12, 12, 7, 7, 21)
    ts = [torch.full((n, e), 5, dtype=dt, device=DEV) for dt, e in zip(dts, ext)]
    st = (ctypes.c_long * 12)(*(list(ext) if strides is None else strides))
    args = [None if name == null else ctypes.c_void_p(t.data_ptr()) for name, t in zip(NAMES, ts)]
    status = lib.far3d_track_records(*args, B, A, K, L, Kdec, row0, P, box_stride, None if no_strides else ctypes.cast(st, ctypes.c_void_p),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = lib.far3d_last_error().decode() if status != 0 else ""
    torch.cuda.synchronize()
    assert status == 0 or all(bool((t == 5).all()) for t in ts), "a refused call wrote to its operands: it launched"
    return status, msg


@pytest.mark.parametrize("name", NAMES + ("batch_strides",))
def test_null_pointers_are_refused_by_name(name):
    status, msg = _raw(null=name, no_strides=name == "batch_strides")
    assert status != 0 and "far3d_track_records" in msg and name in msg and "null pointer" in msg, msg


@pytest.mark.parametrize("kw, match", [
    (dict(B=0), "B=0"), (dict(K=0), "bad sizes"), (dict(K=1025, A=2000, L=4096), "bad sizes"), (dict(L=4097), "bad sizes"),
    (dict(K=13), "bad sizes"), (dict(A=4), "bad sizes"), (dict(Kdec=1025), "bad sizes"), (dict(Kdec=-1), "bad sizes"),
    (dict(row0=7), "propagated rows"), (dict(row0=-1), "propagated rows"), (dict(P=6, row0=3), "P=6 propagated slots > K=5"),
    (dict(box_stride=2), "box_stride=2"), (dict(box_stride=0), "box_stride=0")])
def test_bad_sizes_are_refused(kw, match):
    status, msg = _raw(**kw)
    assert status != 0 and "far3d_track_records" in msg and match in msg, msg


@pytest.mark.parametrize("i", range(12))
def test_a_stream_stride_below_one_streams_extent_is_refused_by_name(i):
    ext = [5, 12, 7, 7, 7, 49, 36, 12, 12, 7, 7, 21]
    assert _raw(B=2, strides=ext)[0] == 0
    ext[i] -= 1
    status, msg = _raw(B=2, strides=ext)
    assert status != 0 and "batch_strides[%d] (%s)" % (i, NAMES[i]) in msg and "below one stream's" in msg, msg
    assert _raw(B=1, strides=ext)[0] == 0                   # one stream: the strides are not read


def test_the_wrapper_refuses_wrong_tensors():
    from far3d_amd import ops
    c = _designed(0.1)
    t = dict(idx=torch.tensor(c["idx"][None], device=DEV), track=torch.tensor(c["track"][None], device=DEV),
             hits=torch.tensor(c["hits"][None], device=DEV), query=torch.tensor(c["query"][None], device=DEV),
             tids=torch.tensor(c["tids"][None], device=DEV), keep=torch.tensor(c["keep"][None], device=DEV),
             boxes=torch.tensor(c["boxes"][None], device=DEV), m_ref=torch.tensor(c["m_ref"][None], device=DEV),
             m_ts=torch.tensor(c["m_ts"][None], device=DEV))
    call = lambda **over: ops.track_records(*[dict(t, **over)[k] for k in ("idx", "track", "hits", "query", "tids", "keep", "boxes", "m_ref", "m_ts")],
                                            over.get("A", 9), over.get("row0", 6), over.get("P", 3))
    with pytest.raises(ValueError, match="mem_hits"):
        call(hits=t["hits"].long())
    with pytest.raises(ValueError, match="m_ts"):
        call(m_ts=t["m_ts"].float())
    with pytest.raises(ValueError, match="keep"):
        call(keep=t["keep"].int())
    with pytest.raises(ValueError, match="boxes"):
        call(boxes=t["boxes"][:, :, :2].contiguous())
    with pytest.raises(ValueError, match="m_ref"):
        call(m_ref=t["m_ref"][:, :5])
    with pytest.raises(ValueError, match="num_propagated=6"):
        call(P=6, row0=3)
    assert t["hits"].cpu().numpy().tolist() == c["hits"][None].tolist()
    age, prim, vel = call(keep=t["keep"].to(torch.uint8))      # uint8 flags are taken like bool ones
    assert prim[0].tolist() == [True, False, True, False, True, False, False]

"""GPU: far3d_box_dedup against the float64 contract (tests/dedup_refs.py) at the smallest shapes where it can go wrong: dup_keep and
dup_of EXACTLY, the kernel's own overlaps (overlap_out) within MARGIN / 4 of the float64 ones -- on inputs whose judged pairs keep
MARGIN from the threshold, so that an error of that size flips no decision -- and every refusal of the entry by name, in front of any
launch."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import dedup_refs as dr
from tests.test_dedup_refs_cpu import _chain, _would_be_suppressors, box

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THR = dict(iou_bev=dr.IOU_THR, centre=dr.CENTRE_THR)
KEYS = (("boxes", torch.float32), ("scores", torch.float32), ("labels", torch.int64), ("keep", torch.bool))


def _gpu(cases, mode, class_aware=True, score_thr=0.0, thr=None, pad=0):
    """ops.box_dedup on B streams (pad > 0: every input a view into a buffer `pad` elements wider per stream, filled with a sentinel
    that must survive); no input may be written.  Returns (dup_keep, dup_of, overlaps) as numpy, leading B."""
    from far3d_amd import ops
    views, wides = {}, {}
    for k, dt in KEYS:
        a = torch.tensor(np.stack([c[k] for c in cases]), dtype=dt)
        if pad:
            flat = a.reshape(a.shape[0], -1)
            wide = torch.full((flat.shape[0], flat.shape[1] + pad), 1, dtype=dt)
            wide[:, :flat.shape[1]] = flat
            wides[k] = wide.to(DEV)
            views[k] = wides[k][:, :flat.shape[1]].view(a.shape)
        else:
            views[k] = a.to(DEV)
    dk, of, ov = ops.box_dedup(views["boxes"], views["scores"], views["labels"], views["keep"], mode=mode, thr=THR[mode] if thr is None else thr,
                               class_aware=class_aware, score_thr=score_thr, return_overlaps=True)
    torch.cuda.synchronize()
    K = views["scores"].shape[1]
    assert dk.dtype == torch.bool and of.dtype == torch.int32 and ov.dtype == torch.float32
    assert tuple(dk.shape) == tuple(of.shape) == (len(cases), K) and tuple(ov.shape) == (len(cases), K, K)
    for k, dt in KEYS:
        if pad:
            n = views[k][0].numel()
            assert bool((wides[k][:, n:] == 1).all()), "%s: the padding between the streams was written" % k
        same = torch.tensor(np.stack([c[k] for c in cases]), dtype=dt).numpy().tobytes()      # bytes: the boxes hold NaNs
        assert views[k].cpu().contiguous().numpy().tobytes() == same, "%s: an input was written" % k
    dk2, of2 = ops.box_dedup(views["boxes"], views["scores"], views["labels"], views["keep"].to(torch.uint8), mode=mode,
                             thr=THR[mode] if thr is None else thr, class_aware=class_aware, score_thr=score_thr)
    assert torch.equal(dk, dk2) and torch.equal(of, of2), "the launch without overlap_out (uint8 keep flags) decides differently"
    return dk.cpu().numpy(), of.cpu().numpy(), ov.cpu().numpy()


def _check(cases, got, mode, class_aware=True, score_thr=0.0, thr=None, tag=""):
    thr = THR[mode] if thr is None else thr
    worst = 0.0
    for b, c in enumerate(cases):
        w = dr.dedup(c["boxes"], c["scores"], c["labels"], c["keep"], mode, thr, class_aware, score_thr)
        assert dr.margin_ok(w["overlaps"], w["judged"], mode, thr), "%s stream %d: the input has a pair within MARGIN of the threshold" % (tag, b)
        err = dr.overlap_error(got[2][b], w["overlaps"], mode, thr)
        worst = max(worst, err)
        print("%s stream %d %s class_aware=%s: overlap_out max err %.3e (bound %.3e), %d judged pairs, %d of %d candidates suppressed" %
              (tag, b, mode, class_aware, err, dr.MARGIN / 4, int(w["judged"].sum()), int((w["dup_of"] >= 0).sum()),
               int(dr.candidates(c["scores"], c["keep"], score_thr).sum())))
        assert not got[2][b][~w["judged"]].any(), "%s stream %d: overlap_out is not 0 outside the judged pairs" % (tag, b)
        assert err < dr.MARGIN / 4, "%s stream %d: overlap_out" % (tag, b)
        assert got[0][b].tolist() == w["dup_keep"].tolist(), "%s stream %d: dup_keep" % (tag, b)
        assert got[1][b].tolist() == w["dup_of"].tolist(), "%s stream %d: dup_of" % (tag, b)
    return worst


# ------------------------------------------------------------------------------------------ designed, Kdec = 7
@pytest.mark.parametrize("mode", dr.MODES)
@pytest.mark.parametrize("class_aware", [True, False])
def test_designed_chain(mode, class_aware):
    """tests/test_dedup_refs_cpu.py's chain: 0 kills 1, so 2 lives; a would-be suppressor that is not kept; another label; a NaN box
    and a zero-extent box on top of box 0."""
    boxes, scores, labels, keep = _chain(code=9)
    c = dict(boxes=boxes, scores=scores, labels=labels, keep=keep)
    dk, of, ov = _gpu([c], mode, class_aware)
    _check([c], (dk, of, ov), mode, class_aware, tag="chain")
    assert dk[0].tolist() == [True, False, True, False, class_aware, True, True]
    assert of[0].tolist() == [-1, 0, -1, -1, -1 if class_aware else 0, -1, -1]
    if mode == "iou_bev":
        assert abs(ov[0, 1, 0] - 0.6) < 2e-6 and abs(ov[0, 2, 0] - 1.0 / 3.0) < 2e-6 and abs(ov[0, 2, 1] - 0.6) < 2e-6      # 10.6 is rounded to fp32
    else:
        assert abs(ov[0, 1, 0] - 0.36) < 2e-6 and abs(ov[0, 2, 0] - 1.44) < 2e-6
    # box 0 below score_thr: 1 lives and kills 2
    sc = dict(c, scores=np.array([0.2, 0.8, 0.7, 0.6, 0.1, 0.4, 0.3], dtype=np.float32))
    got = _gpu([sc], mode, class_aware, score_thr=0.25)
    _check([sc], got, mode, class_aware, score_thr=0.25, tag="chain score_thr")
    assert got[0][0].tolist() == [False, True, False, False, False, True, True] and got[1][0].tolist() == [-1, -1, 1, -1, -1, -1, -1]


@pytest.mark.parametrize("mode", dr.MODES)
def test_designed_would_be_suppressors(mode):
    """Kdec = 7: a box that is not kept, one below score_thr and one with a NaN heading, each with a later box on top of it that
    nothing else hits -- the later boxes live; with the first two in force they die."""
    boxes, scores, labels, keep = _would_be_suppressors(code=8)
    c = dict(boxes=boxes, scores=scores, labels=labels, keep=keep)
    got = _gpu([c], mode, score_thr=0.25)
    _check([c], got, mode, score_thr=0.25, tag="would-be suppressors")
    assert got[0][0].tolist() == [False, True, False, True, True, True, True] and (got[1][0] == -1).all()
    c = dict(c, keep=np.ones(7, dtype=bool))
    got = _gpu([c], mode, score_thr=0.1)
    _check([c], got, mode, score_thr=0.1, tag="suppressors in force")
    assert got[0][0].tolist() == [True, False, True, False, True, True, True] and got[1][0].tolist() == [-1, 0, -1, 2, -1, -1, -1]


def test_designed_analytic_overlaps():
    """Kdec = 7 pairs with a known IoU, read through overlap_out: identical boxes 1, two 4 x 1 rectangles crossed on one centre 1/7,
    a unit square against itself turned by 45 degrees sqrt(2)/2, boxes that share an edge 0, disjoint boxes 0."""
    rows = [box(100.0, -120.0, 4.0, 1.0, 0.7), box(100.0, -120.0, 4.0, 1.0, 0.7),            # 1 on 0: identical
            box(-50.0, 60.0, 4.0, 1.0, 0.0), box(-50.0, 60.0, 4.0, 1.0, math.pi / 2),         # 3 on 2: crossed
            box(5.0, 5.0, 1.0, 1.0, 0.0), box(5.0, 5.0, 1.0, 1.0, math.pi / 4),               # 5 on 4: the turned square
            box(6.0, 5.0, 1.0, 1.0, 0.0)]                                                     # 6 shares an edge with 4
    c = dict(boxes=np.stack(rows), scores=np.linspace(0.9, 0.3, 7).astype(np.float32), labels=np.zeros(7, dtype=np.int64), keep=np.ones(7, dtype=bool))
    for thr, keep in ((0.5, [True, False, True, True, True, False, True]), (0.1, [True, False, True, False, True, False, True])):
        dk, of, ov = _gpu([c], "iou_bev", thr=thr)
        _check([c], (dk, of, ov), "iou_bev", thr=thr, tag="analytic thr=%g" % thr)
        assert dk[0].tolist() == keep
    assert abs(ov[0, 1, 0] - 1.0) < 1e-6 and abs(ov[0, 3, 2] - 1.0 / 7.0) < 1e-6 and abs(ov[0, 5, 4] - math.sqrt(2.0) / 2.0) < 1e-6
    assert ov[0, 6, 4] == 0.0 and ov[0, 2, 0] == 0.0 and ov[0, 6, 0] == 0.0
    assert of[0].tolist() == [-1, 0, -1, 2, -1, 4, -1]


# ------------------------------------------------------------------------------------------ generated inputs
@pytest.mark.parametrize("K, seed", [ks for ks in dr.INPUTS if ks[0] != 40])
def test_generated_inputs(K, seed):
    """65 and 129: the first box of a second and a third mask word; 300: the engine's max_num; 1024: every LDS array full."""
    c = dr.generated(K, seed)
    worst = {}
    for mode in dr.MODES:
        for ca in (True, False):
            worst[mode] = max(worst.get(mode, 0.0), _check([c], _gpu([c], mode, ca), mode, ca, tag="K=%d" % K))
    print("K=%d: overlap_out, largest error: iou_bev %.3e (absolute), centre %.3e (relative d^2)" % (K, worst["iou_bev"], worst["centre"]))


# ------------------------------------------------------------------------------------------ streams
def test_three_streams_with_padded_strides_equal_their_own_launches():
    cases = [dr.generated(K, seed) for K, seed in dr.INPUTS if K == 40]
    cases = [dict(c, boxes=np.ascontiguousarray(c["boxes"][:, :7])) for c in cases]      # one box width for the batch
    assert len(cases) == 3
    for mode in dr.MODES:
        alone = [_gpu([c], mode) for c in cases]
        for pad in (0, 5):
            got = _gpu(cases, mode, pad=pad)
            _check(cases, got, mode, tag="B=3 pad=%d" % pad)
            for b in range(3):
                for g, a in zip(got, alone[b]):
                    assert g[b].tobytes() == a[0].tobytes(), "stream %d differs from its own one-stream launch" % b


def test_padded_output_strides_through_the_c_entry():
    """The wrapper allocates contiguous outputs; here dup_keep, dup_of and overlap_out of B = 3 streams are views into buffers 5
    elements wider per stream, filled with a sentinel that must survive, and hold the wrapper's results."""
    from far3d_amd import lib as _lib, ops
    lib = _lib.require_device()
    cases = [dr.generated(K, seed) for K, seed in dr.INPUTS if K == 40]
    ins = [torch.tensor(np.stack([np.ascontiguousarray(c[k][:, :7]) if k == "boxes" else c[k] for c in cases]), dtype=dt).to(DEV) for k, dt in KEYS]
    for mode in dr.MODES:
        dk, of, ov = ops.box_dedup(*ins, mode=mode, thr=THR[mode], return_overlaps=True)
        ext = (40, 40, 1600)
        outs = [torch.full((3, e + 5), 7, dtype=dt, device=DEV) for e, dt in zip(ext, (torch.uint8, torch.int32, torch.float32))]
        st = (ctypes.c_long * 7)(280, 40, 40, 40, 45, 45, 1605)
        status = lib.far3d_box_dedup(*[ctypes.c_void_p(t.data_ptr()) for t in [ins[0], ins[1], ins[2], ins[3].to(torch.uint8)] + outs], 3, 40, 7,
                                     dr.MODES.index(mode), 1, THR[mode], 0.0, ctypes.cast(st, ctypes.c_void_p),
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert status == 0, lib.far3d_last_error().decode()
        for o, e, want in zip(outs, ext, (dk.to(torch.uint8), of, ov.reshape(3, 1600))):
            assert bool((o[:, e:] == 7).all()), "the padding between the streams' outputs was written"
            assert torch.equal(o[:, :e], want)


def test_no_decoded_boxes():
    from far3d_amd import ops
    for B in (1, 2):
        dk, of, ov = ops.box_dedup(torch.zeros((B, 0, 7), device=DEV), torch.zeros((B, 0), device=DEV), torch.zeros((B, 0), dtype=torch.int64, device=DEV),
                                   torch.zeros((B, 0), dtype=torch.bool, device=DEV), return_overlaps=True)
        torch.cuda.synchronize()
        assert tuple(dk.shape) == (B, 0) and tuple(of.shape) == (B, 0) and tuple(ov.shape) == (B, 0, 0)


# ------------------------------------------------------------------------------------------ refusals
NAMES = ("boxes", "scores", "labels", "keep", "dup_keep", "dup_of", "overlap_out")
EXT = (49, 7, 7, 7, 7, 7, 49)


def _raw(B=1, Kdec=7, box_stride=7, mode=0, class_aware=1, thr=0.5, score_thr=0.0, null=None, strides=None, no_strides=False, no_overlap=False):
    """The C entry on operands of the designed shape filled with 5s; returns (status, message)."""
    from far3d_amd import lib as _lib
    lib = _lib.require_device()
    n = max(B, 1)
    dts = (torch.float32, torch.float32, torch.int64, torch.uint8, torch.uint8, torch.int32, torch.float32)
    ts = [torch.full((n, e), 5, dtype=dt, device=DEV) for dt, e in zip(dts, EXT)]
    st = (ctypes.c_long * 7)(*(list(EXT) if strides is None else strides))
    args = [None if name == null or (no_overlap and name == "overlap_out") else ctypes.c_void_p(t.data_ptr()) for name, t in zip(NAMES, ts)]
    status = lib.far3d_box_dedup(*args, B, Kdec, box_stride, mode, class_aware, thr, score_thr,
                                 None if no_strides else ctypes.cast(st, ctypes.c_void_p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = lib.far3d_last_error().decode() if status != 0 else ""
    torch.cuda.synchronize()
    assert status == 0 or all(bool((t == 5).all()) for t in ts), "a refused call wrote to its operands: it launched"
    return status, msg


@pytest.mark.parametrize("name", NAMES[:6] + ("batch_strides",))
def test_null_pointers_are_refused_by_name(name):
    status, msg = _raw(null=name, no_strides=name == "batch_strides")
    assert status != 0 and "far3d_box_dedup" in msg and name in msg and "null pointer" in msg, msg


def test_a_null_overlap_out_is_legal():
    assert _raw(no_overlap=True)[0] == 0


@pytest.mark.parametrize("kw, match", [
    (dict(B=0), "B=0"), (dict(B=-1), "B=-1"), (dict(Kdec=1025), "Kdec=1025"), (dict(Kdec=-1), "Kdec=-1"), (dict(box_stride=6), "box_stride=6"),
    (dict(box_stride=0), "box_stride=0"), (dict(mode=2), "mode=2"), (dict(mode=-1), "mode=-1"), (dict(thr=float("nan")), "thr is a NaN"),
    (dict(thr=1.0), "thr=1 outside [0, 1)"), (dict(thr=-0.25), "thr=-0.25 outside [0, 1)"), (dict(mode=1, thr=0.0), "thr=0 is not a finite distance"),
    (dict(mode=1, thr=-1.0), "thr=-1 is not a finite distance"), (dict(mode=1, thr=float("inf")), "thr=inf is not a finite distance"),
    (dict(mode=1, thr=float("nan")), "thr is a NaN"), (dict(score_thr=1.5), "score_thr=1.5"), (dict(score_thr=-0.5), "score_thr=-0.5"),
    (dict(score_thr=float("nan")), "score_thr=nan")])
def test_bad_arguments_are_refused(kw, match):
    status, msg = _raw(**kw)
    assert status != 0 and "far3d_box_dedup" in msg and match in msg, msg


def test_legal_edges_of_the_arguments():
    assert _raw(thr=0.0)[0] == 0 and _raw(mode=1, thr=1e-3)[0] == 0 and _raw(score_thr=1.0)[0] == 0 and _raw(box_stride=7, class_aware=0)[0] == 0


@pytest.mark.parametrize("i", range(7))
def test_a_stream_stride_below_one_streams_extent_is_refused_by_name(i):
    ext = list(EXT)
    assert _raw(B=2, strides=ext)[0] == 0
    ext[i] -= 1
    status, msg = _raw(B=2, strides=ext)
    assert status != 0 and "batch_strides[%d] (%s)" % (i, NAMES[i]) in msg and "below one stream's" in msg, msg
    assert _raw(B=1, strides=ext)[0] == 0                   # one stream: the strides are not read
    if i == 6:
        assert _raw(B=2, strides=ext, no_overlap=True)[0] == 0      # nor is the last one without overlap_out


def test_the_wrapper_refuses_wrong_tensors():
    from far3d_amd import ops
    boxes, scores, labels, keep = _chain()
    t = dict(boxes=torch.tensor(boxes[None], device=DEV), scores=torch.tensor(scores[None], device=DEV),
             labels=torch.tensor(labels[None], device=DEV), keep=torch.tensor(keep[None], device=DEV))
    call = lambda kw={}, **over: ops.box_dedup(*[dict(t, **over)[k] for k in ("boxes", "scores", "labels", "keep")], **kw)
    with pytest.raises(ValueError, match="boxes"):
        call(boxes=t["boxes"][:, :, :6].contiguous())
    with pytest.raises(ValueError, match="boxes"):
        call(boxes=t["boxes"].double())
    with pytest.raises(ValueError, match="boxes"):
        call(boxes=t["boxes"][:, :5])
    with pytest.raises(ValueError, match="scores"):
        call(scores=t["scores"].double())
    with pytest.raises(ValueError, match="scores"):
        call(scores=t["scores"].cpu())
    with pytest.raises(ValueError, match="labels"):
        call(labels=t["labels"].int())
    with pytest.raises(ValueError, match="keep"):
        call(keep=t["keep"].int())
    with pytest.raises(ValueError, match="keep"):
        call(keep=t["keep"][0])
    with pytest.raises(ValueError, match="mode"):
        call(dict(mode="iou3d"))
    with pytest.raises(ValueError, match="thr=1.0"):
        call(dict(thr=1.0))
    with pytest.raises(ValueError, match="thr=0.0"):
        call(dict(mode="centre", thr=0.0))
    with pytest.raises(ValueError, match="score_thr"):
        call(dict(score_thr=2.0))
    with pytest.raises(ValueError, match="Kdec=1025"):
        ops.box_dedup(torch.zeros((1, 1025, 7), device=DEV), torch.zeros((1, 1025), device=DEV), torch.zeros((1, 1025), dtype=torch.int64, device=DEV),
                      torch.zeros((1, 1025), dtype=torch.bool, device=DEV))
    dk, of = call()
    assert dk[0].tolist() == [True, False, True, False, True, True, True] and of[0].tolist() == [-1, 0, -1, -1, -1, -1, -1]

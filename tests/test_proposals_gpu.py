"""GPU: the 2D-proposal kernels (csrc/frontend.hip: far3d_proposal_select -- score map, 3x3 peak test, threshold and top-K mode --
and far3d_proposal_gather) against the float64 restatements of tests/head_refs.py, on the seeded cases of head_refs.PROP_CASES.

Exclusion rule.  Peak or not, above the threshold or not, inside the top K or not, and the rounded depth-map cell are discontinuous: a
decision whose float64 margin is below the fp32 error bound of the quantity it is taken on (head_refs.SCORE_MARGIN relative for scores,
head_refs.CELL_MARGIN for the cell) is skipped together with what depends on it; an exact tie (margin 0) has one right answer and is
not skipped.  At most 1 % of the decisions of a kind may be skipped per case (tests/test_head_refs_cpu.py asserts that the reference's
own count stays inside that for every case).  The depth bin is an arg-max over logits that are *inputs* here: both sides compare the
same float32 values, so it has no margin and is never skipped.
Tolerances as in tests/test_glue_gpu.py; every test prints its figures (pytest -s)."""
import pytest
import torch

from tests import head_refs as hr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = hr.U32
CASE_IDS = ["-".join(str(x) for x in c) for c in hr.PROP_CASES]


def report(tag, **kw):
    print("[prop] %s: %s" % (tag, "  ".join("%s=%.3e" % (k, v) if isinstance(v, float) else "%s=%s" % (k, v) for k, v in kw.items())))


def dev_maps(case):
    return [c.to(DEV).contiguous() for c in case["cls"]], [r.to(DEV).contiguous() for r in case["reg"]]


def select(case, cap, thr=0.1, topk=False):
    from far3d_amd import ops
    cls_d, reg_d = dev_maps(case)
    wgt, idx, cnt = ops.proposal_select(cls_d, reg_d, case["strides"], cap, thr=thr, topk=topk)
    return wgt, idx, cnt, reg_d


def reference_maps(case):
    cls, reg = hr.widen(case["cls"]), hr.widen(case["reg"])
    raw, peak = hr.proposal_weights(cls, reg)
    pm = hr.peak_margin(cls, reg)
    return raw, peak, (pm > 0) & (pm < hr.SCORE_MARGIN)


def at_most_one_percent(skipped, total, tag):
    assert skipped <= 0.01 * total, "%s: %d of %d decisions inside the fp32 margin (more than 1 %%)" % (tag, skipped, total)


@pytest.mark.parametrize("case_args", hr.PROP_CASES, ids=CASE_IDS)
def test_score_and_peak_map_against_float64(hip_lib, case_args):
    """Every cell of the weight map: the score where the reference says "peak", exactly 0.0 where it says "not a peak" -- level and
    camera borders included (the `border` case puts every camera's largest scores on the rim of level 1)."""
    case = hr.proposal_case(*case_args)
    wgt = select(case, case["S"])[0].cpu()
    raw, peak, undecided = reference_maps(case)
    tag = "peak map " + "-".join(str(x) for x in case_args)
    at_most_one_percent(int(undecided.sum()), undecided.numel(), tag)
    is_peak = peak > 0
    ok = ~undecided
    assert torch.equal((wgt > 0)[ok], is_peak[ok]), "%s: %d cells differ in the peak decision" % (tag, int(((wgt > 0) != is_peak)[ok].sum()))
    assert bool((wgt[ok & ~is_peak] == 0.0).all()), tag
    raw32, _ = hr.proposal_weights(case["cls"], case["reg"])
    y = hr.yard(raw32, raw)
    b = hr.chain_bound(y, raw)
    sel = ok & is_peak
    err = (wgt.double() - raw)[sel].abs().max().item()
    assert err <= b, "%s: score error %.3e above the bound %.3e" % (tag, err, b)
    # a window never looks into the neighbouring level or camera: the ties / border cases have their peaks on the rims
    report(tag, peaks=int(is_peak.sum()), skipped=int(undecided.sum()), yard=y, bound=b, err=err)


@pytest.mark.parametrize("thr", [0.1, 0.3])
@pytest.mark.parametrize("case_args", hr.PROP_CASES, ids=CASE_IDS)
def test_threshold_mode_against_float64(hip_lib, case_args, thr):
    """sel_cnt / sel_idx = the reference's `weight > thr` set in ascending index order; with a capacity below the count the first
    `cap` in index order are kept."""
    case = hr.proposal_case(*case_args)
    N, S = case["N"], case["S"]
    _, idx, cnt, _ = select(case, S, thr=thr)
    idx, cnt = idx.cpu(), cnt.cpu()
    raw, peak, undecided = reference_maps(case)
    near_thr = (peak > 0) & ((peak - thr).abs() / thr < hr.SCORE_MARGIN)
    undecided = undecided | near_thr
    tag = "threshold %.1f " % thr + "-".join(str(x) for x in case_args)
    at_most_one_percent(int(undecided.sum()), undecided.numel(), tag)
    cap_small = 5
    _, idx5, cnt5, _ = select(case, cap_small, thr=thr)
    idx5, cnt5 = idx5.cpu(), cnt5.cpu()
    for n in range(N):
        want = torch.nonzero(peak[n] > thr)[:, 0]
        got = idx[n, :cnt[n]].long()
        assert bool((got[1:] > got[:-1]).all()), "%s camera %d: not in ascending index order" % (tag, n)
        gm, wm = torch.zeros(S, dtype=torch.bool), torch.zeros(S, dtype=torch.bool)
        gm[got], wm[want] = True, True
        assert not ((gm != wm) & ~undecided[n]).any(), "%s camera %d: the selected set differs in decided cells" % (tag, n)
        if not undecided[n].any():
            assert int(cnt[n]) == want.numel() and torch.equal(got, want), (tag, n)
            assert int(cnt5[n]) == min(cap_small, want.numel()) and torch.equal(idx5[n, :cnt5[n]].long(), want[:cap_small]), (tag, n)
    if case["variant"] == "empty":
        assert int(cnt[0]) == 0 and int(cnt5[0]) == 0, tag + ": camera 0 has nothing above the threshold"
    report(tag, counts=cnt.tolist(), skipped=int(undecided.sum()))


@pytest.mark.parametrize("K", [7, 92])
@pytest.mark.parametrize("case_args", hr.PROP_CASES, ids=CASE_IDS)
def test_topk_mode_against_the_float64_peak_map(hip_lib, case_args, K):
    """The K best cells per camera against a stable sort of the *float64* peak map (ties towards the lower index, output ascending).
    A cell is undecided if its peak decision is, or if its weight is within the margin of the K-th weight without being equal to it."""
    case = hr.proposal_case(*case_args)
    N, S = case["N"], case["S"]
    _, idx, cnt, _ = select(case, K, topk=True)
    idx, cnt = idx.cpu(), cnt.cpu()
    raw, peak, undecided = reference_maps(case)
    tag = "top-%d " % K + "-".join(str(x) for x in case_args)
    skipped = 0
    for n in range(N):
        order = torch.sort(-peak[n], stable=True).indices[:K]
        kth = peak[n][order[-1]]
        near = (peak[n] != kth) & ((peak[n] - kth).abs() < hr.SCORE_MARGIN * kth)
        und = undecided[n] | near
        skipped += int(und.sum())
        got = idx[n].long()
        assert int(cnt[n]) == K and bool((got[1:] > got[:-1]).all()), (tag, n)
        gm, wm = torch.zeros(S, dtype=torch.bool), torch.zeros(S, dtype=torch.bool)
        gm[got], wm[order] = True, True
        assert not ((gm != wm) & ~und).any(), "%s camera %d: the selected set differs in decided cells" % (tag, n)
        if not und.any():
            assert torch.equal(got, torch.sort(order).values), (tag, n)
    at_most_one_percent(skipped, N * S, tag)
    report(tag, skipped=skipped)


GATHER_CASES = [c for c in hr.PROP_CASES if c[3] in ("plain", "wide", "empty")]


@pytest.mark.parametrize("form", ["legacy", "rows_total", "rows_short"])
@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case_args", GATHER_CASES, ids=["-".join(str(x) for x in c) for c in GATHER_CASES])
def test_gather_against_float64(hip_lib, case_args, feat_dtype, form):
    """far3d_proposal_gather on the device's own threshold selection: box decode, depth cell and bin, unprojection, context row,
    log-odds -- in the legacy form (N * cap rows, the first M written) and the fixed-capacity form (rows_total rows: the rest zero,
    the count and the overflow flag on the device; rows_short: fewer rows than proposals, the surplus dropped and flagged)."""
    from far3d_amd import ops
    case = hr.proposal_case(*case_args, with_feat=True, feat_dtype=feat_dtype)
    N, S, C = case["N"], case["S"], case["feat"].shape[2]
    cap = min(S, 2048)
    wgt_d, idx_d, cnt_d, reg_d = select(case, cap, thr=0.1)
    wgt, idx, cnt = wgt_d.cpu(), idx_d.cpu(), cnt_d.cpu()
    assert int(cnt.max()) < cap
    sel = [idx[n, :cnt[n]].long() for n in range(N)]
    M = int(cnt.sum())
    tag = "gather %s %s %s" % ("-".join(str(x) for x in case_args), str(feat_dtype).split(".")[1], form)
    rows_total = dict(legacy=0, rows_total=M + 37, rows_short=max(M - 3, 1))[form]
    m_out = torch.full((1,), -1, dtype=torch.int32, device=DEV) if rows_total else None
    ovf = torch.full((1,), -1, dtype=torch.int32, device=DEV) if rows_total else None
    nrows = rows_total or N * cap
    out = (torch.full((nrows, 3), 7.0, device=DEV), torch.full((nrows, C + 1), 7.0, device=DEV), torch.full((nrows, 4), 7.0, device=DEV),
           torch.full((nrows,), 7.0, device=DEV))
    ops.proposal_gather(reg_d, case["strides"], idx_d, cnt_d, wgt_d, case["depth_logit"].to(DEV), case["ds"], hr.DEPTH_CFG,
                        case["img2lidar"].to(DEV), case["feat"].to(DEV), case["pc_range"], 0.1, out=out, rows_total=rows_total,
                        m_out=m_out, overflow_out=ovf)
    ref2d, ctx, box2d, score = [t.cpu() for t in out]
    Mv = M if not rows_total else min(M, rows_total)
    if rows_total:
        assert int(m_out.item()) == Mv and int(ovf.item()) == (1 if M > rows_total else 0), tag
        for t in (ref2d, ctx, box2d, score):
            assert not t[Mv:].any(), tag + ": rows past the count must be zero"
    else:
        assert bool((ref2d[M:] == 7.0).all()) and bool((ctx[M:] == 7.0).all()), tag + ": rows past the count are not written"
    args64 = (hr.widen(case["reg"]), case["strides"], sel, wgt.double(), case["depth_logit"].double(), case["ds"], hr.DEPTH_CFG,
              case["img2lidar"].double(), case["feat"].double(), case["pc_range"], 0.1)
    want = hr.proposal_rows(*args64)
    f32 = hr.proposal_rows(case["reg"], case["strides"], sel, wgt, case["depth_logit"], case["ds"], hr.DEPTH_CFG, case["img2lidar"],
                           case["feat"].float(), case["pc_range"], 0.1)
    assert want["cam"].numel() == M
    want, f32 = {k: v[:Mv] for k, v in want.items()}, {k: v[:Mv] for k, v in f32.items()}
    ref2d, ctx, box2d, score = ref2d[:Mv], ctx[:Mv], box2d[:Mv], score[:Mv]
    # copies
    flat = torch.cat([n * S + s for n, s in enumerate(sel)])[:Mv]
    assert torch.equal(score, wgt.reshape(-1)[flat]), tag + " score"
    assert torch.equal(ctx[:, :C], case["feat"].reshape(N * S, C)[flat].float()), tag + " context channels"
    # log-odds: chain through logf
    yl = hr.yard(f32["ctx"][:, C], want["ctx"][:, C])
    bl = hr.chain_bound(yl, want["ctx"][:, C])
    el = (ctx[:, C].double() - want["ctx"][:, C]).abs().max().item()
    assert el <= bl, "%s: log-odds error %.3e above %.3e" % (tag, el, bl)
    # box centre: derived from the chain; width / height: relative, yardstick
    cb = hr.centre_bound(want)
    ec = (box2d[:, :2].double() - want["box2d"][:, :2]).abs()
    assert bool((ec <= cb).all()), "%s: box centre error %.3e above its chain bound" % (tag, ec.max().item())
    rel = lambda a, ref: ((a.double() - ref).abs() / ref).max().item()
    yw = rel(f32["box2d"][:, 2:], want["box2d"][:, 2:])
    bw = 4 * yw + 2 * hr.ULP32
    ew = rel(box2d[:, 2:], want["box2d"][:, 2:])
    assert ew <= bw, "%s: relative width / height error %.3e above %.3e" % (tag, ew, bw)
    # depth cell (a rounding decision) -> bin -> reference point
    und = hr.cell_undecided(want, case["ds"])
    at_most_one_percent(int(und.sum()), max(Mv, 1), tag + " depth cell")
    rb = hr.ref2d_bound(want, case, cb)
    er = (ref2d.double() - want["ref2d"]).abs()
    bad = (er > rb).any(dim=-1) & ~und
    assert not bad.any(), "%s: %d reference points off (a wrong cell, a wrong depth bin or the unprojection), worst %.3e against %.3e" % (
        tag, int(bad.sum()), er[bad].max().item(), rb[bad].max().item())
    outside = int(((want["cell_pos"].round() < 0) | (want["cell_pos"].round() > torch.tensor([case["wd"] - 1, case["hd"] - 1]))).any(dim=-1).sum())
    if case["variant"] == "wide":
        assert outside > 0 and want["box2d"][:, 2:].max().item() > 1e3, tag + ": the case must hold clamped centres and 1e3-px boxes"
    report(tag, M=M, logodds_yard=yl, logodds_bound=bl, logodds_err=el, centre_err=ec.max().item(), centre_bound=cb.max().item(),
           wh_yard=yw, wh_bound=bw, wh_err=ew, ref2d_err=er[~und].max().item() if (~und).any() else 0.0, ref2d_bound=rb.max().item(),
           cells_skipped=int(und.sum()), clamped=outside)

"""GPU: the kernels of the foreign-2D-head path (csrc/foreign.hip): far3d_mask_compact against torch.nonzero and against the native
selection, far3d_proposal_from_boxes bit for bit against far3d_proposal_gather / far3d_proposal_gather_md on their own boxes, and
against the float64 restatement of tests/foreign_refs.py on arbitrary boxes with a probability map.

The bitwise comparison holds as it stands (no rounding-order exception): after the box, both kernels evaluate the same fp32
expressions in the same order.  Bounds of the float64 comparison: head_refs.ref2d_bound with a ZERO centre bound (the boxes are
inputs), head_refs.chain_bound for the log-odds column; cell, bins and token columns exact, no exclusions
(tests/test_foreign_refs_cpu.py shows that the seeded inputs leave none of these decisions to rounding).  pytest -s prints the figures."""
import pytest
import torch

from tests import foreign_refs as fr
from tests import head_refs as hr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def check_compaction(mask, cap):
    from far3d_amd import ops
    N, S = mask.shape
    ovf = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    idx, cnt = ops.mask_compact(mask.to(DEV), cap, overflow_out=ovf)
    idx, cnt = idx.cpu(), cnt.cpu()
    over = False
    for n in range(N):
        want = torch.nonzero(mask[n])[:, 0]
        over |= want.numel() > cap
        assert int(cnt[n]) == min(want.numel(), cap), (n, int(cnt[n]), want.numel())
        assert torch.equal(idx[n, :cnt[n]].long(), want[:cap]), "camera %d: not the first %d selected indices in ascending order" % (n, cap)
    assert int(ovf.item()) == (1 if over else 0)
    return cnt


def test_compaction_case_a_random_none_all(hip_lib):
    hw = [(7, 11), (4, 6), (2, 3), (1, 2)]
    S = sum(h * w for h, w in hw)
    assert S == 109
    g = torch.Generator().manual_seed(1)
    mask = torch.zeros(3, S, dtype=torch.bool)
    mask[0] = torch.rand(S, generator=g) < 0.2
    mask[2] = True
    cnt = check_compaction(mask, S)
    assert 0 < int(cnt[0]) < S and int(cnt[1]) == 0 and int(cnt[2]) == S


@pytest.mark.parametrize("cap", [5000, 8])
def test_compaction_case_b_chunk_borders_and_capacity(hip_lib, cap):
    S = 5000
    g = torch.Generator().manual_seed(2)
    mask = torch.rand(2, S, generator=g) < 0.03
    mask[:, [0, 63, 64, 65, 255, 256, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 4999]] = True
    cnt = check_compaction(mask, cap)
    if cap == 8:
        assert cnt.tolist() == [8, 8]


def test_compaction_takes_uint8_and_unaligned_rows(hip_lib):
    """One byte per token, any non-zero value selects; rows that start on every residue of the 16-byte grid (S odd, 17 cameras)."""
    g = torch.Generator().manual_seed(3)
    m8 = (torch.rand(17, 37, generator=g) < 0.4).to(torch.uint8) * torch.randint(1, 256, (17, 37), generator=g).to(torch.uint8)
    check_compaction(m8 != 0, 37)
    from far3d_amd import ops
    idx, cnt = ops.mask_compact(m8.to(DEV), 37)
    idx2, cnt2 = ops.mask_compact((m8 != 0).to(DEV), 37)
    assert torch.equal(cnt, cnt2) and all(torch.equal(idx[n, :cnt[n]], idx2[n, :cnt[n]]) for n in range(17))


def native(case, K):
    """The native pair on a proposal case: threshold selection, then far3d_proposal_gather (K = 1) or far3d_proposal_gather_md."""
    from far3d_amd import ops
    cls_d, reg_d = [c.to(DEV).contiguous() for c in case["cls"]], [r.to(DEV).contiguous() for r in case["reg"]]
    N, S, C = case["N"], case["S"], case["feat"].shape[2]
    wgt, idx, cnt = ops.proposal_select(cls_d, reg_d, case["strides"], S, thr=0.1)
    dev = dict(depth=case["depth_logit"].to(DEV), i2l=case["img2lidar"].to(DEV), feat=case["feat"].to(DEV))
    rows = N * S
    if K == 1:
        out = ops.proposal_gather(reg_d, case["strides"], idx, cnt, wgt, dev["depth"], case["ds"], hr.DEPTH_CFG, dev["i2l"], dev["feat"],
                                  case["pc_range"], 0.1)
        rec = None
    else:
        out = (torch.empty((rows, 3), device=DEV), torch.empty((rows, C + 1), device=DEV), torch.empty((rows, 4), device=DEV),
               torch.empty((rows,), device=DEV))
        rec = (torch.empty((rows,), dtype=torch.int32, device=DEV), torch.empty((rows, 2 * K), dtype=torch.int32, device=DEV))
        ops.proposal_gather_md(reg_d, case["strides"], idx, cnt, wgt, dev["depth"], case["ds"], hr.DEPTH_CFG, dev["i2l"], dev["feat"],
                               case["pc_range"], K, fr.BOX_RANGE_MIN_BIN, rec, out)
    return wgt, idx, cnt, out, rec, dev


def test_compaction_gives_back_the_native_selection(hip_lib):
    from far3d_amd import ops
    case = hr.proposal_case("small3", 26, 5, "plain", with_feat=True)
    wgt, idx, cnt, _, _, _ = native(case, 1)
    N, S = case["N"], case["S"]
    c = cnt.cpu().tolist()
    mask = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    for n in range(N):
        mask[n, idx[n, :c[n]].long()] = True
    idx2, cnt2 = ops.mask_compact(mask, S)
    assert sum(c) > 20 and torch.equal(cnt2, cnt)
    assert all(torch.equal(idx2[n, :c[n]], idx[n, :c[n]]) for n in range(N))


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("geom", ["small3", "odd2"])
def test_from_boxes_equals_the_native_gather_bit_for_bit(hip_lib, geom, feat_dtype, K):
    """Fed with the box2d, score, sel_idx and sel_cnt far3d_proposal_gather(_md) wrote and with its logits as the depth map, ref2d and
    ctx (and for K = 3 the records) are the native ones, bit for bit."""
    from far3d_amd import ops
    case = hr.proposal_case(geom, 26, 5, "plain", with_feat=True, feat_dtype=feat_dtype)
    wgt, idx, cnt, out, rec, dev = native(case, K)
    M = int(cnt.sum().item())
    assert M > 20
    boxes, scores = out[2][:M].contiguous(), out[3][:M].contiguous()
    rec2 = None
    if K > 1:
        rec2 = (torch.full((M,), -7, dtype=torch.int32, device=DEV), torch.full((M, 2 * K), -7, dtype=torch.int32, device=DEV))
    mis = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ref2d, ctx = ops.proposal_from_boxes(boxes, cnt, scores, idx, cnt, dev["depth"], case["ds"], hr.DEPTH_CFG, dev["i2l"], dev["feat"],
                                         case["pc_range"], depth_is_prob=False, depth_layout="nhwc", score_thr=0.1, topk=K,
                                         range_min_bin=fr.BOX_RANGE_MIN_BIN, records=rec2, mismatch_out=mis)
    assert int(mis.item()) == 0
    bits = lambda t: t.view(torch.int32)
    assert torch.equal(bits(ref2d), bits(out[0][:M])), "ref2d: %d values differ" % int((bits(ref2d) != bits(out[0][:M])).sum())
    assert torch.equal(bits(ctx), bits(out[1][:M])), "ctx: %d values differ" % int((bits(ctx) != bits(out[1][:M])).sum())
    if K > 1:
        assert torch.equal(rec2[0], rec[0][:M]) and torch.equal(rec2[1], rec[1][:M]), "multi-depth records differ"
        assert 0 < int(rec2[0].sum()) < M, "valid and invalid primaries"


@pytest.fixture(scope="module")
def box_refs():
    """The float64 reference and the fp32 yardstick of the seeded boxes case, computed once (K = 1 and K = BOX_TOPK)."""
    case = fr.boxes_case()
    return case, {K: (fr.case_rows(case, torch.float64, K), fr.case_rows(case, torch.float32, K)) for K in (1, fr.BOX_TOPK)}


def run_from_boxes(case, feat, K, layout, box_cnt=None):
    from far3d_amd import ops
    N, S, C = case["N"], case["S"], feat.shape[2]
    nums = [b.shape[0] for b in case["boxes"]]
    M = sum(nums)
    box2d, score = torch.zeros((K * M, 4), device=DEV), torch.zeros((K * M,), device=DEV)
    box2d[:M], score[:M] = torch.cat(case["boxes"]).to(DEV), case["scores"].to(DEV)
    cnt_d = torch.tensor(nums if box_cnt is None else box_cnt, dtype=torch.int32, device=DEV)
    sel_idx, sel_cnt = ops.mask_compact(case["mask"].to(DEV), max(nums))
    depth = case["depth"] if layout == "nhwc" else case["depth"].permute(0, 3, 1, 2)
    out = (torch.full((K * M, 3), 7.0, device=DEV), torch.full((K * M, C + 1), 7.0, device=DEV), box2d, score)
    rec = (torch.zeros((M,), dtype=torch.int32, device=DEV), torch.zeros((M, 2 * K), dtype=torch.int32, device=DEV)) if K > 1 else None
    flags = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    i2l = case["img2lidar"].to(DEV)
    ops.proposal_from_boxes(box2d, cnt_d, score, sel_idx, sel_cnt, depth.contiguous().to(DEV), case["ds"], hr.DEPTH_CFG, i2l, feat.to(DEV),
                            case["pc_range"], depth_is_prob=True, depth_layout=layout, topk=K, range_min_bin=fr.BOX_RANGE_MIN_BIN,
                            records=rec, out=out, mismatch_out=flags[1:2], rows=M)
    Mq = M
    if K > 1:
        ops.proposal_extra_rows(cnt_d, 0, M, K, rec, i2l, hr.DEPTH_CFG, case["pc_range"], out, fill_hole=False, m_out=flags[0:1])
        Mq = int(flags[0].item())
    return out[0].cpu(), out[1].cpu(), rec, Mq, int(flags[1].item())


@pytest.mark.parametrize("K", [1, fr.BOX_TOPK])
@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_from_boxes_against_float64(hip_lib, box_refs, feat_dtype, K):
    """Arbitrary boxes (random, exact half cells of both parities, a negative centre, centres beyond the right and bottom edges, an
    empty camera between two others) and a probability map: cell and bins exact, reference points within their chain bound, log-odds
    within the chain bound, token columns equal; for K = 3 through far3d_proposal_extra_rows, in the reference's row order."""
    case, refs = box_refs
    want, f32 = refs[K]
    feat = case["feat"].to(feat_dtype)
    M, Mw, C = want["cell"].shape[0], want["cam"].numel(), feat.shape[2]
    ref2d, ctx, rec, Mq, mis = run_from_boxes(case, feat, K, "nhwc")
    assert mis == 0 and Mq == Mw, (mis, Mq, Mw)
    tag = "from_boxes K=%d %s" % (K, str(feat_dtype).split(".")[1])
    # decisions: exact.  The cell is visible through the bins only if the map differs from cell to cell (it does: seeded noise).
    if K > 1:
        info = rec[1].cpu()
        assert torch.equal(info[:, 0].long(), want["cam"][:M]), tag + " record camera"
        assert torch.equal(info[:, 1:1 + K].long(), want["topk_idx"]), tag + ": depth bins (or the cell they were read at) differ"
        assert torch.equal(rec[0].cpu().bool(), want["valid"]), tag + " valid flags"
        ratio = info[:, K + 1:].contiguous().view(torch.float32)
        yr = hr.yard(f32["ratio"][:, 1:], want["ratio"][:, 1:])
        er = (ratio.double() - want["ratio"][:, 1:]).abs().max().item()
        assert er <= hr.chain_bound(yr, want["ratio"][:, 1:]), "%s: ratio error %.3e" % (tag, er)
    # token columns: copies
    tok = feat.float()[want["cam"], want["token"][want["src"]]]
    assert torch.equal(ctx[:Mw, :C], tok), tag + " token columns"
    # log-odds column
    yl = hr.yard(f32["ctx"][:, C], want["ctx"][:, C])
    bl = hr.chain_bound(yl, want["ctx"][:, C])
    el = (ctx[:Mw, C].double() - want["ctx"][:, C]).abs().max().item()
    assert el <= bl, "%s: log-odds error %.3e above %.3e" % (tag, el, bl)
    # reference points: a wrong cell or bin is far outside the bound (neighbouring bins are >= 0.08 m apart)
    rb = hr.ref2d_bound(want, case, torch.zeros(Mw, 2, dtype=torch.float64))
    er = (ref2d[:Mw].double() - want["ref2d"]).abs()
    bad = (er > rb).any(dim=-1)
    assert not bad.any(), "%s: %d reference points off (rows %s), worst %.3e against %.3e" % (
        tag, int(bad.sum()), torch.nonzero(bad).flatten().tolist()[:8], er[bad].max().item(), rb[bad].max().item())
    # (K = 1 carries no record: cell and bin are pinned through the reference point alone)
    assert bool((ref2d[Mw:] == 7.0).all()) and bool((ctx[Mw:] == 7.0).all()), tag + ": rows past the count are not written"
    print("[foreign] %s: M=%d M'=%d logodds yard=%.3e bound=%.3e err=%.3e ref2d err=%.3e bound=%.3e" % (
        tag, M, Mw, yl, bl, el, er.max().item(), rb.max().item()))
    # the reference's own (N,D,hd,wd) layout reads the same values
    ref2d_c, ctx_c, rec_c, _, _ = run_from_boxes(case, feat, K, "nchw")
    assert torch.equal(ref2d_c[:Mw], ref2d[:Mw]) and torch.equal(ctx_c[:Mw], ctx[:Mw]), tag + " nchw depth layout"
    if K > 1:
        assert torch.equal(rec_c[1], rec[1]) and torch.equal(rec_c[0], rec[0])


def test_from_boxes_flags_a_count_mismatch(hip_lib, box_refs):
    """box_cnt != sel_cnt for a camera sets the flag; rows are written for the smaller of the two and never past the buffers."""
    case, _ = box_refs
    nums = [b.shape[0] for b in case["boxes"]]
    for cnt in ([nums[0] - 1, 0, nums[2]], [nums[0], 1, nums[2]], [nums[0], 0, nums[2] + 5]):
        *_, mis = run_from_boxes(case, case["feat"], 1, "nhwc", box_cnt=cnt)
        assert mis == 1, cnt
    *_, mis = run_from_boxes(case, case["feat"], 1, "nhwc")
    assert mis == 0


@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_from_boxes_with_a_channel_count_that_is_no_multiple_of_8(hip_lib, box_refs, feat_dtype):
    """C = 20: the token rows are not 16-byte aligned and are read element by element; everything else as with C = 256."""
    case, refs = box_refs
    want = refs[1][0]
    M = want["cam"].numel()
    feat = fr.boxes_case(feat_dtype=feat_dtype, C=20)["feat"]
    ref2d, ctx, _, _, mis = run_from_boxes(case, feat, 1, "nhwc")
    ref2d_w, ctx_w, _, _, _ = run_from_boxes(case, case["feat"], 1, "nhwc")
    assert mis == 0 and ctx.shape[1] == 21
    assert torch.equal(ctx[:M, :20], feat.float()[want["cam"], want["token"]])
    assert torch.equal(ctx[:M, 20], ctx_w[:M, 256]) and torch.equal(ref2d[:M], ref2d_w[:M])

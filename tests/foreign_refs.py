"""Plain-torch restatement of the reference's build_query2d_proposal (farhead.py:711-827) for GIVEN boxes, token mask, scores and
depth map -- the inputs a foreign 2D head hands to FarHead -- for multi_depth_config.topk = 1 and K > 1, and the seeded inputs the
CPU and GPU tests of the foreign path share.

TEST INFRASTRUCTURE ONLY: no device code, nothing derived from far3d_amd/csrc/foreign.hip.  Like tests/head_refs.py every function
computes in the dtype of its floating inputs: widened inputs give the float64 reference, float32 inputs the fp32 yardstick."""
import torch

from tests import head_refs as hr


def foreign_rows(boxes, mask, scores, depth, ds, depth_cfg, img2lidar, feat, pc_range, topk=1, range_min_bin=0, depth_is_prob=True,
                 score_thr=0.1):
    """boxes: N tensors (M_i,4) cx,cy,w,h in pixels; mask (N,S) bool with M_i selected tokens in camera i (the j-th box pairs with the
    j-th selected token, farhead.py:578-579); scores (M,); depth (N,hd,wd,nd) probabilities (or logits: depth_is_prob=False, the
    softmax is taken here, :573); img2lidar (N,4,4); feat (N,S,C).
    Returns None when there is no box (:727), else a dict in the reference's row order (the M primaries camera-major, then for
    k = 1 .. K-1 the valid primaries, :760-771): ref2d (M',3), ctx (M',C+1), box2d (M',4), bin (M',), cam (M',), src (M',) the
    primary of every row, and per primary: cell (M,2) (u,v), cell_pos (M,2) centre / ds, chain (M,2) |c| + wh/2, topk_idx (M,K),
    ratio (M,K) p_k / p_0, valid (M,) bool."""
    dt = depth.dtype
    N, hd, wd, nd = depth.shape
    nums = [int(b.shape[0]) for b in boxes]
    if sum(nums) == 0:
        return None
    K = max(int(topk), 1)
    lo, span = hr._span(pc_range, dt)
    prob = depth if depth_is_prob else depth.softmax(dim=-1)
    cam = torch.cat([torch.full((m,), n, dtype=torch.long) for n, m in enumerate(nums)])
    box = torch.cat([b.to(dt) for b in boxes])                                        # (M,4)
    tok = torch.cat([torch.nonzero(mask[n].reshape(-1))[:, 0] for n in range(N)])     # ascending per camera = boolean-mask indexing
    assert tok.numel() == box.shape[0], "the mask must select one token per box"
    pos = box[:, :2] / ds
    cell = pos.round().long()                                                          # half to even, :736
    cell[cell < 0] = 0                                                                 # :737-739
    cell[:, 0] = torch.where(cell[:, 0] >= wd, torch.full_like(cell[:, 0], wd - 1), cell[:, 0])
    cell[:, 1] = torch.where(cell[:, 1] >= hd, torch.full_like(cell[:, 1], hd - 1), cell[:, 1])
    at = lambda m: m[cam, cell[:, 1], cell[:, 0]]                                      # (M,nd)
    order = torch.sort(-at(depth), dim=1, stable=True).indices[:, :K]                  # best first, lower bin first on ties
    pk = torch.gather(at(prob), 1, order)
    ratio = pk / pk[:, 0:1]                                                            # :778
    valid = order[:, 0] >= range_min_bin if K > 1 else torch.ones_like(cam, dtype=torch.bool)
    vrows = torch.nonzero(valid)[:, 0]
    src = torch.cat([torch.arange(cam.numel())] + [vrows] * (K - 1))
    bins = torch.cat([order[:, 0]] + [order[vrows, k] for k in range(1, K)])
    dsc = torch.cat([ratio[:, 0]] + [ratio[vrows, k] for k in range(1, K)])
    sc = scores.reshape(-1).to(dt).clamp(min=1e-6)
    thr = torch.tensor(score_thr, dtype=dt)
    lodds = torch.log(sc / (1 - sc)) - torch.log(thr / (1 - thr))                      # :774-775
    ctx = torch.cat([feat.to(dt)[cam, tok][src], (lodds[src] * dsc)[:, None]], dim=-1) # :781-784
    d = depth_cfg["depth_min"] + hr.depth_bin_size(depth_cfg, dt) / 8 * (torch.square(bins.to(dt) / 0.5 + 1) - 1)      # :521-527
    dm = torch.maximum(d, torch.full_like(d, 1e-5))
    c = box[src, :2]
    coords = torch.stack([c[:, 0] * dm, c[:, 1] * dm, d, torch.ones_like(d)], dim=-1)  # :792-794
    c3 = (img2lidar.to(dt)[cam[src]] @ coords[:, :, None])[:, :3, 0]                   # :808
    return dict(ref2d=(c3 - lo) / span, ctx=ctx, box2d=box[src], bin=bins, cam=cam[src], src=src, cell=cell, cell_pos=pos,
                chain=box[:, :2].abs() + box[:, 2:] / 2, topk_idx=order, ratio=ratio, valid=valid, token=tok)


# ------------------------------------------------------------------------------------------------ seeded inputs
BOX_SEED = 0
BOX_GEOM = "small3"
BOX_TOPK = 3
BOX_RANGE_MIN_BIN = 12


def boxes_case(seed=BOX_SEED, feat_dtype=torch.float32, C=256):
    """Arbitrary boxes on geometry small3 (3 cameras, depth map 16 x 24 at stride 8, S = 510 tokens); camera 1 has NO box between two
    that have some.  Camera 0: 23 random boxes, then centres at exact half cells stride * (k + 0.5) for even and odd k (round half to
    even: down for even k, up for odd), a negative centre and centres beyond the right and the bottom edge.  Camera 2: 17 random
    boxes.  The depth map holds probabilities (softmax of seeded logits).  -> dict; `deliberate` marks the half-cell rows."""
    from far3d_amd import synth
    N, hw = hr.PROP_GEOMS[BOX_GEOM]
    hd, wd = hw[0]
    ds, S = 8, sum(h * w for h, w in hw)
    g = torch.Generator().manual_seed(5000 + seed)
    W, H = wd * ds, hd * ds

    def rand_boxes(m):
        c = torch.rand(m, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
        return torch.cat([c, 4 + torch.rand(m, 2, generator=g) * 90], dim=-1)

    half = torch.tensor([[ds * (2 + 0.5), ds * (3 + 0.5), 20.0, 30.0],        # even k on x, odd k on y
                         [ds * (5 + 0.5), ds * (4 + 0.5), 12.0, 9.0],         # odd k on x, even k on y
                         [ds * (0 + 0.5), ds * (1 + 0.5), 7.0, 7.0],
                         [ds * (wd - 1 + 0.5), ds * (hd - 1 + 0.5), 40.0, 40.0]])      # rounds up past the map -> clamped
    out = torch.tensor([[-13.25, 40.5, 30.0, 20.0], [W + 57.0, 17.75, 25.0, 25.0], [33.1, H + 91.0, 10.0, 50.0],
                        [-0.3, -250.0, 5.0, 5.0], [W + 3.0, H + 3.0, 8.0, 8.0]])
    cam0 = torch.cat([rand_boxes(23), half, out])
    boxes = [cam0, torch.zeros(0, 4), rand_boxes(17)]
    deliberate = torch.zeros(sum(b.shape[0] for b in boxes), dtype=torch.bool)
    deliberate[23:23 + half.shape[0]] = True
    mask = torch.zeros(N, S, dtype=torch.bool)
    for n, b in enumerate(boxes):
        mask[n, torch.randperm(S, generator=g)[:b.shape[0]]] = True
    M = int(mask.sum())
    scores = 0.1 + 0.89 * torch.rand(M, generator=g)
    depth = (torch.randn(N, hd, wd, hr.DEPTH_CFG["num_depth_bins"] + 1, generator=g) * 1.5).softmax(dim=-1)
    return dict(N=N, hw=hw, S=S, ds=ds, hd=hd, wd=wd, boxes=boxes, mask=mask, scores=scores, depth=depth, deliberate=deliberate,
                img2lidar=torch.linalg.inv(synth.ring_cameras(N, (hd * ds, wd * ds), dtype=torch.float64)[2]).float().contiguous(),
                feat=torch.randn(N, S, C, generator=g).to(feat_dtype), pc_range=[-152.4, -152.4, -5.0, 152.4, 152.4, 5.0])


def case_rows(case, dtype, topk=1):
    """foreign_rows on a boxes_case in `dtype` (float64: the reference on the widened float32 inputs)."""
    w = (lambda t: t.to(dtype))
    return foreign_rows([w(b) for b in case["boxes"]], case["mask"], w(case["scores"]), w(case["depth"]), case["ds"], hr.DEPTH_CFG,
                        w(case["img2lidar"]), w(case["feat"].float()), case["pc_range"], topk=topk,
                        range_min_bin=BOX_RANGE_MIN_BIN if topk > 1 else 0, depth_is_prob=True)

"""Plain-torch restatements of the FarHead bookkeeping kernels (csrc/glue.hip, csrc/frontend.hip), one function per operation.

TEST INFRASTRUCTURE ONLY: no device code.  Every function computes in the dtype of its floating inputs, so the same function gives
the float64 reference value (inputs widened with .double(): the values stay the float32 ones the kernel sees) and the float32
yardstick (how far the reference's own fp32 arithmetic is from float64).  Citations are file:line under projects/mmdet3d_plugin/
of the reference; where oracle/far3d_oracle.py has the expression it is called.

dim_t: the reference builds it in float32 and lets type promotion widen `pos / dim_t` (positional_encoding.py:16-17,30-32); so does
the kernel (a float tensor argument).  `dim_t(n)` returns those float32 values; `sincos_code` widens them to the dtype of `pos`.
The oracle's pos2posemb builds dim_t in float64 when pos is float64; `dim_t_gap` measures what that changes.
"""
import math

import torch
import torch.nn.functional as F

from oracle import far3d_oracle as fo

U32 = 2.0 ** -24          # unit roundoff of float32 (half an ulp, relative)
ULP32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ codes
def dim_t(n, temperature=10000):
    d = torch.arange(n, dtype=torch.float32)
    return temperature ** (2 * torch.div(d, 2, rounding_mode="floor") / n)


def sincos_code(pos, dt):
    """One coordinate -> interleaved sin / cos over the len(dt) slots (positional_encoding.py:13-36): slot i holds
    sin(2 pi pos / dt[i]) for even i, cos for odd i; dt[2j] == dt[2j+1]."""
    p = (pos * (2 * math.pi))[..., None] / dt.to(pos.dtype)
    return torch.stack((p[..., 0::2].sin(), p[..., 1::2].cos()), dim=-1).flatten(-2)


def posemb3d(pos, dt):
    """(R,3) -> (R, 3*len(dt)), ordered y, x, z (positional_encoding.py:24)."""
    return torch.cat([sincos_code(pos[..., 1], dt), sincos_code(pos[..., 0], dt), sincos_code(pos[..., 2], dt)], dim=-1)


def time_code(ts, dt):
    """pos2posemb1d on the float64 memory timestamps (L,) -> (L, 256) float64; the caller casts to float32 (farhead.py:303)."""
    return sincos_code(ts.double(), dt)


def motion_input(velo, ts, pose):
    """(L,15) float32: cat(velo, ts, pose[:3,:].flatten()).float() -- the reference's cast (farhead.py:297) is part of the definition."""
    L = velo.shape[0]
    return torch.cat([velo.double(), ts.double().reshape(L, 1), pose.double().reshape(L, 4, 4)[:, :3, :].reshape(L, 12)], dim=-1).float()


def motion_code(velo, ts, pose, dtype=torch.float64):
    """nerf_positional_encoding of the float32 motion vector (positional_encoding.py:38-80): for f in 1,2,4,..,32:
    [sin(v f) (15), cos(v f) (15)] -> (L,180).  dtype: arithmetic after the reference's float32 cast."""
    return fo.nerf_encoding(motion_input(velo, ts, pose).to(dtype))


# ------------------------------------------------------------------------------------------------ memory
def _span(pc_range, dtype):
    pc = torch.as_tensor(pc_range, dtype=torch.float32)
    return pc[:3].to(dtype), (pc[3:6] - pc[:3]).to(dtype)       # the span is taken in float32 as the kernel's host code does


def pre_update(state, ego_inv, timestamp, pseudo_ref, x, P, pc_range, fresh=False):
    """farhead.py:453-477 + :287.  state: emb (L,E) ref (L,3) ts (L,) f64 pose (L,4,4) velo (L,2); ego_inv (4,4); timestamp python
    float / f64 scalar; x = prev_exists (0. or 1.).  fresh: the reference's first frame (memory is None -> zeros, no warp).
    Returns (m dict, temp_ref (L,3))."""
    dt = state["ref"].dtype
    lo, span = _span(pc_range, dt)
    if fresh:
        m = {k: torch.zeros_like(v) for k, v in state.items()}
    else:
        m = dict(ts=(state["ts"].double() + float(timestamp)) * float(x),
                 pose=(ego_inv.to(dt)[None] @ state["pose"]) * x,
                 ref=fo.Far3DOracle._transform_ref(state["ref"][None], ego_inv.to(dt)[None])[0] * x,
                 emb=state["emb"] * x, velo=state["velo"] * x)
    if P > 0:
        pseudo = pseudo_ref.to(dt)[:P] * span + lo
        m["ref"] = torch.cat([m["ref"][:P] + (1 - x) * pseudo, m["ref"][P:]])
        m["pose"] = torch.cat([m["pose"][:P] + (1 - x) * torch.eye(4, dtype=dt), m["pose"][P:]])
    return m, (m["ref"] - lo) / span


def post_update(m, topk_idx, dec_last, box_last, ego_pose, timestamp, L):
    """farhead.py:479-508 (+ the truncation to L of :467-471): the selected queries go in front, everything is warped by ego_pose."""
    dt = m["ref"].dtype
    K = topk_idx.numel()
    g = lambda t: t[topk_idx]
    pose = torch.cat([torch.eye(4, dtype=dt).expand(K, 4, 4), m["pose"]])[:L]
    ref = torch.cat([g(box_last)[:, :3].to(dt), m["ref"]])[:L]
    return dict(emb=torch.cat([g(dec_last).to(dt), m["emb"]])[:L],
                ts=torch.cat([torch.zeros(K, dtype=torch.float64), m["ts"].double()])[:L] - float(timestamp),
                pose=ego_pose.to(dt)[None] @ pose,
                ref=fo.Far3DOracle._transform_ref(ref[None], ego_pose.to(dt)[None])[0],
                velo=torch.cat([g(box_last)[:, -2:].to(dt), m["velo"]])[:L])


def exact_product(a, b):
    """True where a * b is exact in any IEEE format: a factor is 0 or +-1."""
    return (a == 0) | (b == 0) | (a.abs() == 1) | (b.abs() == 1)


def matmul_bound(A, B, n_ops):
    """Forward error bound of fl32(A @ B) against the exact product of the same operands: 2 * n_ops * 2^-24 * |A| @ |B| (n_ops = the
    roundings on the longest path of the kernel's expression; the 2 covers the compiler's freedom to contract into FMAs or not).
    An output whose terms are all exact products with at most one of them non-zero is exact (x * 0, x * 1 and x + 0 do not round):
    the bound is 0 there -- this keeps the constant row (0,0,0,1) of a pose exact, as it is on any IEEE machine."""
    A, B = A.double(), B.double()
    terms = A[..., :, :, None].abs() * B[..., None, :, :].abs()                      # (..., i, k, j)
    exact = exact_product(A[..., :, :, None], B[..., None, :, :]).all(dim=-2) & ((terms != 0).sum(dim=-2) <= 1)
    return torch.where(exact, torch.zeros((), dtype=torch.float64), 2 * n_ops * U32 * terms.sum(dim=-2))


def homog(ref):
    return torch.cat([ref, torch.ones_like(ref[..., :1])], dim=-1)


def prepare_bounds(st64, ego_inv, pseudo, x, P, lo, span):
    """fp32 error bounds of far3d_memory_prepare's warps against float64, from the kernel's expressions:
    pose: v = sum_k e_ik p_kj (product, 4 accumulating adds), v *= x, v += (1 - x) I  -> 6 roundings on the longest path (the add to the
    zero accumulator does not round); ref: 3 products + 3 adds, * x, + pseudo term -> 6; the pseudo term itself (rows < P, x = 0):
    p * span + lo -> 2 roundings on |p span| + |lo| (the product with 1 - x = 1 and the add to 0 are exact)."""
    L = st64["ref"].shape[0]
    bp = matmul_bound(ego_inv[None], st64["pose"], 6) * x
    br = 2 * 6 * U32 * (ego_inv.double().abs()[:3] @ homog(st64["ref"]).abs().T).T * x
    if P > 0:
        rows = torch.zeros(L, 1, dtype=torch.float64)
        rows[:P] = 1.0
        pb = torch.zeros(L, 3, dtype=torch.float64)
        pb[:P] = 2 * 2 * U32 * ((pseudo.double()[:P] * span).abs() + lo.abs())
        br = br + (1 - x) * rows * pb
    return bp, br


def post_bounds(m64, push_ref64, K, L, ego):
    """far3d_memory_post_update: pose = sum_k e_ik p_kj -> product + 4 adds = 5 roundings (0 for the pushed identity rows: exact
    products, see matmul_bound); ref = e_i0 r0 + e_i1 r1 + e_i2 r2 + e_i3 -> product + 3 adds = 4."""
    pose = torch.cat([torch.eye(4, dtype=torch.float64).expand(K, 4, 4), m64["pose"]])[:L]
    ref = torch.cat([push_ref64, m64["ref"]])[:L]
    return matmul_bound(ego[None], pose, 5), 2 * 4 * U32 * (ego.double().abs()[:3] @ homog(ref).abs().T).T


# ------------------------------------------------------------------------------------------------ rows
def row_affine_ln(x, gamma, beta, add=None, do_ln=True, eps=1e-5):
    """misc.py:153-190 as the engine applies it: gamma * LN_noaffine(x) + beta (+ add); gamma / beta / add (rows,C) or one row."""
    v = F.layer_norm(x, (x.shape[-1],), None, None, eps) if do_ln else x
    out = gamma.reshape(-1, x.shape[-1]) * v + beta.reshape(-1, x.shape[-1])
    return out + add.reshape(-1, x.shape[-1]) if add is not None else out


def finalize(reg, ref, cls_last, pc_range):
    """farhead.py:649-664, :490.  reg (layers,A,code), ref (A,3), cls_last (A,ncls) -> boxes (layers,A,code), scores (A,)."""
    lo, span = _span(pc_range, reg.dtype)
    xyz = (reg[..., :3] + fo.inverse_sigmoid(ref)[None]).sigmoid() * span + lo
    return torch.cat([xyz, reg[..., 3:]], dim=-1), cls_last.max(dim=-1).values.sigmoid()


# ------------------------------------------------------------------------------------------------ 2D proposals
def proposal_weights(cls, reg):
    """yolox_head.py:426-438.  cls[l] (N,h,w,ncls), reg[l] (N,h,w,>=5) with the objectness in channel 4.
    -> raw (N,S) = sigmoid(obj) * sigmoid(max cls), peak (N,S) = raw where raw equals its 3x3 maximum (inside its own level) else 0."""
    raws, peaks = [], []
    for c, r in zip(cls, reg):
        n = c.shape[0]
        sw = r[..., 4].sigmoid() * c.max(dim=-1).values.sigmoid()                   # (N,h,w)
        nms = F.max_pool2d(sw[:, None], (3, 3), stride=1, padding=1)[:, 0]
        raws.append(sw.reshape(n, -1))
        peaks.append((sw * (sw == nms).to(sw.dtype)).reshape(n, -1))
    return torch.cat(raws, dim=1), torch.cat(peaks, dim=1)


def neighbour_max(raw_level):
    """(N,h,w) -> the largest of the (up to 8) neighbours of every cell, -inf where there is none."""
    n, h, w = raw_level.shape
    p = F.pad(raw_level, (1, 1, 1, 1), value=float("-inf"))
    out = torch.full_like(raw_level, float("-inf"))
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                out = torch.maximum(out, p[:, dy:dy + h, dx:dx + w])
    return out


def peak_margin(cls, reg):
    """Relative float64 margin of every cell's peak decision: |raw - largest neighbour| / raw, (N,S)."""
    out = []
    for c, r in zip(cls, reg):
        sw = r[..., 4].double().sigmoid() * c.double().max(dim=-1).values.sigmoid()
        out.append(((sw - neighbour_max(sw)).abs() / sw).reshape(sw.shape[0], -1))
    return torch.cat(out, dim=1)


def depth_bin_size(depth_cfg, dtype):
    one = torch.ones((), dtype=dtype)
    return 2 * (one * depth_cfg["depth_max"] - one * depth_cfg["depth_min"]) / (one * depth_cfg["num_depth_bins"] * (1 + one * depth_cfg["num_depth_bins"]))


def proposal_rows(reg, strides, sel, weights, depth_logit, ds, depth_cfg, img2lidar, feat, pc_range, score_thr=0.1):
    """yolox_head.py:491-501 (box decode, xyxy -> cxcywh), farhead.py:736-747 (depth cell: round half to even, clamped), :521-527 (LID
    un-binning), :571-610 (unprojection), :810-827 (context row with the log-odds).  sel: per camera a 1-D long tensor of flat cell
    indices (ascending); weights (N,S) the peak weights the scores are read from; feat (N,S,C); img2lidar (N,4,4).
    Returns a dict: ref2d (M,3), ctx (M,C+1), box2d (M,4) cx,cy,w,h, score (M,), and the decisions it took: cell (M,2) long (u,v),
    cell_pos (M,2) centre / ds before rounding, bin (M,) long, cam (M,), chain (M,2) |cx|+w/2, |cy|+h/2, xy_mag (M,2) |p st| + prior."""
    dt = reg[0].dtype
    lo, span = _span(pc_range, dt)
    hw = [(r.shape[1], r.shape[2]) for r in reg]
    start = [0]
    for h, w in hw:
        start.append(start[-1] + h * w)
    N, hd, wd, nd = depth_logit.shape
    rows = dict(ref2d=[], ctx=[], box2d=[], score=[], cell=[], cell_pos=[], bin=[], cam=[], chain=[], xy_mag=[])
    bin_size = depth_bin_size(depth_cfg, dt)
    thr = torch.tensor(score_thr, dtype=dt)
    for n in range(N):
        s = sel[n].long()
        if s.numel() == 0:
            continue
        lvl = torch.zeros_like(s)
        for l in range(1, len(hw)):
            lvl = torch.where(s >= start[l], torch.full_like(s, l), lvl)
        st_, W_ = torch.tensor(strides, dtype=dt)[lvl], torch.tensor([w for _, w in hw])[lvl]
        r = s - torch.tensor(start[:-1])[lvl]
        y, x = torch.div(r, W_, rounding_mode="floor"), r % W_
        pred = torch.cat([rl[n].reshape(-1, rl.shape[-1]) for rl in reg])[s]
        xy =pred[:, :2] * st_[:, None] + torch.stack([x, y], dim=-1).to(dt) * st_[:, None]
        wh = pred[:, 2:4].exp() * st_[:, None]
        tl, br = xy - wh / 2, xy + wh / 2
        c, wh2 = (tl + br) / 2, br - tl
        pos = c / ds
        cell = pos.round().long()
        cell[:, 0].clamp_(0, wd - 1)
        cell[:, 1].clamp_(0, hd - 1)
        b = depth_logit[n][cell[:, 1], cell[:, 0]].argmax(dim=-1)                   # first maximum
        d = depth_cfg["depth_min"] + bin_size / 8 * (torch.square(b.to(dt) / 0.5 + 1) - 1)
        dm = torch.maximum(d, torch.full_like(d, 1e-5))
        coords = torch.stack([c[:, 0] * dm, c[:, 1] * dm, d, torch.ones_like(d)], dim=-1)
        c3 = (img2lidar[n].to(dt) @ coords.T).T[:, :3]
        sc = weights[n][s].to(dt)
        scc = sc.clamp(min=1e-6)
        lodds = torch.log(scc / (1 - scc)) - torch.log(thr / (1 - thr))
        rows["ref2d"].append((c3 - lo) / span)
        rows["ctx"].append(torch.cat([feat[n][s].to(dt), lodds[:, None]], dim=-1))
        rows["box2d"].append(torch.cat([c, wh2], dim=-1))
        rows["score"].append(sc)
        rows["cell"].append(cell)
        rows["cell_pos"].append(pos)
        rows["bin"].append(b)
        rows["cam"].append(torch.full_like(s, n))
        rows["chain"].append(xy.abs() + wh / 2)
        rows["xy_mag"].append((pred[:, :2] * st_[:, None]).abs() + torch.stack([x, y], dim=-1).to(dt) * st_[:, None])
    if not rows["cam"]:
        return None
    return {k: torch.cat(v) for k, v in rows.items()}


# ------------------------------------------------------------------------------------------------ bounds shared by the CPU and GPU tests
SCORE_MARGIN = 32 * ULP32       # relative; sigmoid(obj) * sigmoid(max cls) in fp32: two expf (<= 3 ulp each, amplified by at most 1 in
                                # 1 / (1 + e)), two adds, two divisions, one product -> < 10 ulp per side; both sides of a comparison err
CELL_MARGIN = lambda chain, ds: 4 * ULP32 * chain / ds     # the xyxy -> cxcywh chain: ~4 roundings of one ulp on |c| + w/2


def cell_undecided(rows, ds):
    """(M,) bool: the float64 centre / ds is closer to a half-integer than the fp32 error bound of the chain that produced it."""
    pos = rows["cell_pos"].double()
    dist = ((pos - torch.floor(pos)) - 0.5).abs()
    return (dist < CELL_MARGIN(rows["chain"].double(), ds)).any(dim=-1)


def centre_bound(rows):
    """fp32 error bound of box2d cx / cy from the chain (not from the final value): xy = p * st + prior (2 roundings on |p st| +
    |prior|), wh = expf(.) * st (expf <= 3 ulp + 1 product: 7 * 2^-24 relative), tl / br = xy -+ wh / 2 (1 rounding each on
    |xy| + wh/2), c = (tl + br) / 2 (1 rounding on |c|); times 2 for contraction freedom."""
    chain = rows["chain"].double()
    wh = rows["box2d"][:, 2:].double()
    return 2 * U32 * (2 * rows["xy_mag"].double() + 3.5 * wh + chain + rows["box2d"][:, :2].double().abs())


def ref2d_bound(rows, case, cbound):
    """fp32 error bound of the normalised reference points, from the kernel's chain (U = 2^-24 per rounding, times 2 at the end):
    d = dmin + (bin_size / 8) (q^2 - 1): bin_size 2 roundings, product 1, sum 1, the float32 value of dmin 1 -> 5 U d (q, q^2 - 1 and
    the division by 8 are exact); px = cx dm: the centre's own bound (cbound, already doubled) * dm + |cx| 5 U dm + U |px|;
    w_k = m_k0 px + m_k1 py + m_k2 d + m_k3: the propagated terms + 4 U sum |terms|; c3 = (w - lo) / span: / span + 3 U (|w| + |lo|) / span."""
    lo, span = _span(case["pc_range"], torch.float64)
    c = rows["box2d"][:, :2].double()
    b = rows["bin"].double()
    d = DEPTH_CFG["depth_min"] + depth_bin_size(DEPTH_CFG, torch.float64) / 8 * ((b / 0.5 + 1) ** 2 - 1)
    dm = d.clamp(min=1e-5)
    p = c * dm[:, None]
    e_p = cbound / 2 * dm[:, None] + c.abs() * 5 * U32 * dm[:, None] + U32 * p.abs()
    m = case["img2lidar"].double().abs()[rows["cam"]]                                   # (M,4,4)
    v = torch.cat([p.abs(), d[:, None], torch.ones_like(d)[:, None]], dim=-1)           # (M,4)
    e_v = torch.cat([e_p, (5 * U32 * d)[:, None], torch.zeros_like(d)[:, None]], dim=-1)
    w_mag = (m[:, :3, :] * v[:, None, :]).sum(-1)
    e_w = (m[:, :3, :] * e_v[:, None, :]).sum(-1) + 4 * U32 * w_mag
    return 2 * (e_w / span + 3 * U32 * (w_mag + lo.abs()) / span)


def yard(fn32, fn64):
    """max |f32 restatement - f64 restatement| per output tensor."""
    return (fn32.double() - fn64).abs().max().item()


def chain_bound(yardstick, ref64):
    """Chains through expf / logf / sinf / cosf / sqrtf: 4 x the yardstick + 2 ulp of the output's largest magnitude (the device's
    transcendental functions and summation order differ from the CPU's by a few ulp; 4 x leaves room for that and stays ~100 x below
    what a wrong frequency, a swapped sin / cos or a missing clamp produces)."""
    mag = ref64.abs().max().item() if ref64.numel() else 0.0
    ulp = 2.0 ** (math.floor(math.log2(mag)) - 23) if mag > 0 else 0.0
    return 4 * yardstick + 2 * ulp


def dim_t_gap(pos):
    """max |code with the reference's float32 dim_t - code with the oracle's float64 dim_t| for float64 positions."""
    out = 0.0
    for n in (128, 256):
        out = max(out, (sincos_code(pos.double(), dim_t(n)) - fo.pos2posemb(pos.double(), n)).abs().max().item())
    return out


# ------------------------------------------------------------------------------------------------ seeded inputs (CPU and GPU tests share them)
MEM_SIZES = [(1024, 256, 256), (48, 256, 16), (37, 100, 0), (5, 256, 5)]
MEM_MODES = ["fresh", "steady", "scene"]
MEM_SCALES = ["synthetic", "dataset", "epoch", "city"]


def drive(scale, frames, seed=0):
    """-> (poses (frames,4,4) f64 ego -> global, timestamps list of python floats).  synthetic: synth.ego_pose_at, t = 0,1,2..;
    dataset: the same drive, t = 20000 + k (the streaming path's dataset index); epoch: t = 1.7e9 + steps of 0.1 / 0.5 s (not
    representable in fp32); city: epoch timestamps and city_SE3_ego-like poses -- translations of a few thousand metres, 1..15 m and up
    to 10 degrees of yaw per frame -- so that ego_inv @ pose cancels large terms."""
    from far3d_amd import synth
    g = torch.Generator().manual_seed(1000 + seed)
    if scale == "synthetic":
        ts = [float(k) for k in range(frames)]
    elif scale == "dataset":
        ts = [20000.0 + k for k in range(frames)]
    else:
        ts, t = [], 1.7e9 + 0.37
        for k in range(frames):
            ts.append(t)
            t += 0.1 if k % 2 == 0 else 0.5
    if scale != "city":
        return torch.stack([synth.ego_pose_at(k) for k in range(frames)]), ts
    poses, yaw, pos = [], 0.7, torch.tensor([2311.53, -4127.81, 14.2], dtype=torch.float64)
    for k in range(frames):
        E = torch.eye(4, dtype=torch.float64)
        E[0, 0], E[0, 1], E[1, 0], E[1, 1] = math.cos(yaw), -math.sin(yaw), math.sin(yaw), math.cos(yaw)
        E[:3, 3] = pos
        poses.append(E)
        step = 1.0 + 14.0 * torch.rand((), generator=g, dtype=torch.float64).item()
        yaw += math.radians(10.0) * (2 * torch.rand((), generator=g, dtype=torch.float64).item() - 1)
        pos = pos + torch.tensor([step * math.cos(yaw), step * math.sin(yaw), 0.05 * step], dtype=torch.float64)
    return torch.stack(poses), ts


def rigid_inverse(pose):
    """Closed-form inverse of a rigid 4x4 in float64 (data_pipeline/streaming.py does the same before its float32 cast)."""
    inv = torch.eye(4, dtype=torch.float64)
    inv[:3, :3] = pose[:3, :3].T
    inv[:3, 3] = -pose[:3, :3].T @ pose[:3, 3]
    return inv


def memory_case(L, E, P, mode, scale, seed=0):
    """One far3d_memory_prepare call at frame 3 of drive(scale).  The live state is what far3d_memory_post_update leaves: slot s was
    pushed at frame j(s) in {0,1,2}: pose = ego_pose_j, ref = ego_pose_j applied to a point within the range, ts = -t_j, a velocity and
    an embedding.  All tensors are CPU; float tensors hold float32 values (ts float64)."""
    g = torch.Generator().manual_seed(seed * 7919 + L * 31 + E + P)
    poses, ts = drive(scale, 4, seed)
    k = 3
    if mode == "fresh":
        state = dict(emb=torch.zeros(L, E), ref=torch.zeros(L, 3), ts=torch.zeros(L, dtype=torch.float64), pose=torch.zeros(L, 4, 4), velo=torch.zeros(L, 2))
    else:
        j = torch.randint(0, k, (L,), generator=g)
        local = (torch.rand(L, 3, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([300.0, 300.0, 10.0], dtype=torch.float64)
        ref = (poses[j] @ homog(local)[..., None])[:, :3, 0]
        state = dict(emb=torch.randn(L, E, generator=g), ref=ref.float(), ts=-torch.tensor(ts, dtype=torch.float64)[j], pose=poses[j].float(),
                     velo=torch.randn(L, 2, generator=g) * 8)
    return dict(state=state, ego_pose=poses[k].float(), ego_inv=rigid_inverse(poses[k]).float(), timestamp=ts[k],
                pseudo_ref=torch.rand(P, 3, generator=g) if P else None, x=1.0 if mode == "steady" else 0.0, fresh=mode == "fresh",
                L=L, E=E, P=P, pc_range=[-152.4, -152.4, -5.0, 152.4, 152.4, 5.0])


def widen(t):
    """float32 tensors (and dicts / lists of them) -> float64 with the same values; everything else unchanged."""
    if isinstance(t, dict):
        return {k: widen(v) for k, v in t.items()}
    if isinstance(t, (list, tuple)):
        return [widen(v) for v in t]
    if isinstance(t, torch.Tensor) and t.dtype in (torch.float32, torch.bfloat16):
        return t.double()
    return t


PROP_GEOMS = dict(small3=(3, [(16, 24), (8, 12), (4, 6), (2, 3)]), odd2=(2, [(17, 23), (9, 12), (5, 6)]),
                  bench7=(7, [(80, 120), (40, 60), (20, 30), (10, 15)]))
DEPTH_CFG = dict(depth_min=0.1, depth_max=110.0, num_depth_bins=50)
PROP_CASES = [("small3", 26, 5, "plain"), ("small3", 1, 6, "border"), ("small3", 26, 6, "ties"), ("small3", 26, 5, "wide"),
              ("small3", 1, 5, "empty"), ("odd2", 26, 5, "plain"), ("odd2", 1, 6, "wide"), ("odd2", 26, 5, "ties"), ("bench7", 26, 5, "plain")]


def proposal_case(geom, ncls, nreg, variant="plain", seed=0, with_feat=False, feat_dtype=torch.float32, C=256):
    """Random 2D-head maps as tests/test_frontend_gpu.py makes them.  variant: border = every camera's largest scores sit on the first /
    last row and column of level 1 (and so next to the end of level 0 / the start of level 2 in the flat index); ties = camera 1 has
    logits quantised to 0.5 (exact ties inside 3x3 windows); wide = boxes of the order of 1e3 px and centres up to ~100 px off their
    cell (some outside the depth map); empty = camera 0 has no cell above any threshold."""
    from far3d_amd import synth
    N, hw = PROP_GEOMS[geom]
    strides = (8, 16, 32, 64)[:len(hw)]
    g = torch.Generator().manual_seed(97 * seed + 11 * ncls + nreg + len(variant) + N)
    cls = [torch.randn(N, h, w, ncls, generator=g) * 2 - 1 for h, w in hw]
    reg = [torch.randn(N, h, w, nreg, generator=g) for h, w in hw]
    if variant == "ties":
        for c, r in zip(cls, reg):
            c[1] = torch.round(c[1] * 2) / 2
            r[1, ..., 4] = torch.round(r[1, ..., 4] * 2) / 2
    if variant == "border":
        c, r = cls[1], reg[1]
        edge = torch.zeros(c.shape[1], c.shape[2], dtype=torch.bool)
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
        c[:, edge] = c[:, edge] + 9.0
        r[:, edge, 4] = r[:, edge, 4].abs() + 6.0
    if variant == "wide":
        for r, s in zip(reg, strides):
            r[..., 2:4] = r[..., 2:4] * 0.5 + math.log(1000.0 / s)
            r[..., 0:2] = r[..., 0:2] * (100.0 / s)
    if variant == "empty":
        for r in reg:
            r[0, ..., 4] = -10.0
    hd, wd = hw[0]
    case = dict(N=N, hw=hw, strides=strides, cls=cls, reg=reg, ncls=ncls, nreg=nreg, ds=8, hd=hd, wd=wd, variant=variant,
                depth_logit=torch.randn(N, hd, wd, DEPTH_CFG["num_depth_bins"] + 1, generator=g),
                img2lidar=torch.linalg.inv(synth.ring_cameras(N, (hd * 8, wd * 8), dtype=torch.float64)[2]).float().contiguous(),
                pc_range=[-152.4, -152.4, -5.0, 152.4, 152.4, 5.0], S=sum(h * w for h, w in hw))
    if with_feat:
        case["feat"] = torch.randn(N, case["S"], C, generator=g).to(feat_dtype)
    return case


def decision_census(case, thrs=(0.1, 0.3), topks=(7, 92)):
    """The float64 reference's own count of decisions that sit inside the fp32 margin, for one proposal case: peak cells, threshold
    cells (per thr), cells next to the K-th weight (per K), depth-map cells of the rows selected at thr[0].  -> dict name -> (inside, total);
    exact_ties -> (0, number of cells that tie exactly with their largest neighbour).  Exact ties (margin 0) have one
    right answer on any IEEE machine (the same operands give the same score) and are not counted."""
    cls, reg = widen(case["cls"]), widen(case["reg"])
    raw, peak = proposal_weights(cls, reg)
    pm = peak_margin(cls, reg)
    out = dict(peak=(int(((pm > 0) & (pm < SCORE_MARGIN)).sum()), pm.numel()))
    for thr in thrs:
        tm = (peak - thr).abs() / thr
        out["thr%.1f" % thr] = (int(((peak > 0) & (tm < SCORE_MARGIN)).sum()), peak.numel())
    for K in topks:
        near = 0
        for n in range(case["N"]):
            kth = torch.sort(peak[n], descending=True).values[K - 1]
            near += int(((peak[n] != kth) & ((peak[n] - kth).abs() < SCORE_MARGIN * kth)).sum())
        out["top%d" % K] = (near, peak.numel())
    out["exact_ties"] = (0, int((pm == 0).sum()))
    sel = [torch.nonzero(peak[n] > thrs[0])[:, 0] for n in range(case["N"])]
    rows = proposal_rows(reg, case["strides"], sel, peak, case["depth_logit"].double(), case["ds"], DEPTH_CFG, case["img2lidar"].double(),
                         torch.zeros(case["N"], case["S"], 1, dtype=torch.float64), case["pc_range"])
    out["cell"] = (int(cell_undecided(rows, case["ds"]).sum()), rows["cam"].numel()) if rows is not None else (0, 0)
    return out

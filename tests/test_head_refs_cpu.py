"""CPU: the float64 restatements of tests/head_refs.py are themselves checked, without a GPU --
 (a) against the oracle method each one restates, in float64 (a Far3DOracle(dtype=torch.float64) of a small spec);
 (b) against hand-computed values for the layout questions two restatements copied from one source could share;
 (c) the exclusion rule of tests/test_proposals_gpu.py: the share of decisions the float64 reference itself puts inside the fp32
     margin, per case;
 (d) every numeric bound of the GPU tests bites: the reference perturbed the way a plausible kernel slip would (a timestamp rounded
     to fp32, ego_inv on the right, a swapped sin / cos ...) FAILS the same bound against the unperturbed reference."""
import math

import pytest
import torch
import torch.nn.functional as F

from far3d_amd import weights
from oracle import far3d_oracle as fo
from tests import head_refs as hr

PC = [-152.4, -152.4, -5.0, 152.4, 152.4, 5.0]
H = "pts_bbox_head."
L_, P_, E_ = 48, 16, 256


@pytest.fixture(scope="module")
def orc():
    spec = weights.detector_spec("V-tiny-eSE", num_query=20, num_propagated=P_)
    sd = weights.init_state_dict(spec, seed=2)
    cfg = fo.default_cfg(backbone=fo.VOV_TINY, num_cams=3, num_query=20, num_propagated=P_, memory_len=L_, topk_proposals=16)
    return fo.Far3DOracle(sd, cfg, dtype=torch.float64)


def batched(st):
    L = st["emb"].shape[0]
    return dict(emb=st["emb"][None].clone(), ref=st["ref"][None].clone(), ts=st["ts"].reshape(1, L, 1).clone(), pose=st["pose"][None].clone(),
                velo=st["velo"][None].clone())


def close(a, b, tol=1e-12):
    scale = max(1.0, b.abs().max().item())
    return a.shape == b.shape and (a - b).abs().max().item() <= tol * scale


def exceeds(got, want, bound):
    """True if the comparison of the GPU tests would fail."""
    return bool(((got.double() - want.double()).abs() > bound).any())


# ------------------------------------------------------------------------------------------------ (a) restatement against the oracle
@pytest.mark.parametrize("mode", hr.MEM_MODES)
def test_pre_update_is_the_oracles(orc, mode):
    mc = hr.memory_case(L_, E_, P_, mode, "city")
    st = hr.widen(mc["state"])
    pseudo = orc.P(H + "pseudo_reference_points.weight")
    orc.mem = None if mode == "fresh" else batched(st)
    data = dict(timestamp=torch.tensor([mc["timestamp"]], dtype=torch.float64), ego_pose_inv=mc["ego_inv"].double()[None])
    orc._pre_update_memory(data, torch.tensor([mc["x"]], dtype=torch.float64))
    m, tref = hr.pre_update(st, mc["ego_inv"].double(), mc["timestamp"], pseudo, mc["x"], P_, PC, fresh=mc["fresh"])
    for k in m:
        assert close(m[k].reshape(orc.mem[k].shape[1:]), orc.mem[k][0]), (mode, k)
    # the operands _temporal_alignment builds from the memory: the reference points it appends, and the motion code through the MLN.
    # The memory is rounded to float32 values first (what the device holds): the reference's .float() of the motion vector is then exact
    # and the float64 oracle, which has no such cast, computes the same thing.
    m = {k: v.float().double() for k, v in m.items()}
    orc.mem = batched(m)
    lo, span = hr._span(PC, torch.float64)
    g = torch.Generator().manual_seed(1)
    A = 7
    qp, tg, rf = (torch.randn(1, A, n, generator=g, dtype=torch.float64) for n in (256, 256, 3))
    tgt, qpos, ref, temp_mem, temp_pos, _ = orc._temporal_alignment(qp, tg, rf)
    assert close(ref[0, A:], ((m["ref"] - lo) / span)[:P_])
    code = hr.motion_code(m["velo"], m["ts"], m["pose"])
    assert torch.equal(hr.motion_input(m["velo"], m["ts"], m["pose"]).double(), torch.cat([m["velo"], m["ts"][:, None], m["pose"][:, :3].reshape(L_, 12)], -1))
    mine = orc._mln(F.layer_norm(m["emb"][None], (256,)), code[None], H + "ego_pose_memory")
    assert close(torch.cat([tgt[:, A:], temp_mem], dim=1), mine, 1e-10), mode
    orc.mem = None


def test_post_update_is_the_oracles_push(orc):
    """head_forward's post-update lines (oracle/far3d_oracle.py, farhead.py:479-508) on the same tensors."""
    mc = hr.memory_case(L_, E_, P_, "steady", "city")
    m = hr.widen(mc["state"])
    g = torch.Generator().manual_seed(3)
    A, code, K = 30, 10, 16
    dec, box = torch.randn(A, E_, generator=g, dtype=torch.float64), torch.randn(A, code, generator=g, dtype=torch.float64)
    idx = torch.randint(0, A, (K,), generator=g)
    mb = batched(m)
    gt = lambda t: t[None][:, idx]
    want = dict(emb=torch.cat([gt(dec), mb["emb"]], 1), ts=torch.cat([torch.zeros(1, K, 1, dtype=torch.float64), mb["ts"]], 1) - mc["timestamp"],
                pose=mc["ego_pose"].double()[None, None] @ torch.cat([torch.eye(4, dtype=torch.float64).expand(1, K, 4, 4), mb["pose"]], 1),
                ref=fo.Far3DOracle._transform_ref(torch.cat([gt(box)[..., :3], mb["ref"]], 1), mc["ego_pose"].double()[None]),
                velo=torch.cat([gt(box)[..., -2:], mb["velo"]], 1))
    got = hr.post_update(m, idx, dec, box, mc["ego_pose"].double(), mc["timestamp"], L_)
    for k in got:
        assert close(got[k].reshape(L_, -1), want[k][0, :L_].reshape(L_, -1)), k


def test_codes_are_the_oracles_up_to_dim_t():
    """With dim_t widened to float64 *before* the power (the oracle's variant) the restatement is the oracle's pos2posemb to rounding; with
    the reference's float32 dim_t it differs by the figure dim_t_gap reports (printed; quoted in the pull request)."""
    g = torch.Generator().manual_seed(0)
    pos = torch.rand(300, 3, generator=g, dtype=torch.float64) * 2 - 0.5
    ts = torch.rand(300, generator=g, dtype=torch.float64) * 6
    for n, p in ((128, pos[:, 0]), (256, ts)):
        d64 = 10000 ** (2 * torch.div(torch.arange(n, dtype=torch.float64), 2, rounding_mode="floor") / n)
        assert close(hr.sincos_code(p, d64), fo.pos2posemb(p, n), 1e-14)
    d128 = 10000 ** (2 * torch.div(torch.arange(128, dtype=torch.float64), 2, rounding_mode="floor") / 128)
    assert close(hr.posemb3d(pos, d128), fo.pos2posemb3d(pos), 1e-14)
    gap_pos, gap_ts = hr.dim_t_gap(pos.reshape(-1)), hr.dim_t_gap(ts)
    print("[refs] float32 dim_t against the oracle's float64 dim_t: %.3e on positions in [-0.5, 1.5], %.3e on timestamps in [0, 6]" % (gap_pos, gap_ts))
    assert 0 < gap_pos < 1e-6 and 0 < gap_ts < 5e-6        # 2^-24 relative on dim_t times the argument (<= 3 pi, <= 12 pi)
    assert torch.equal(hr.dim_t(256)[0::2], hr.dim_t(256)[1::2]) and hr.dim_t(128)[0].item() == 1.0


def oracle_roi(case):
    f = lambda t: t.double().permute(0, 3, 1, 2)
    return dict(enc_cls_scores=[f(c) for c in case["cls"]], enc_bbox_preds=[f(r)[:, :4] for r in case["reg"]],
                objectnesses=[f(r)[:, 4:5] for r in case["reg"]])


@pytest.mark.parametrize("variant", ["plain", "ties", "wide"])
def test_proposal_restatements_are_the_oracles(orc, variant):
    case = hr.proposal_case("small3", 26, 5, variant, with_feat=True)
    roi = oracle_roi(case)
    out = orc.get_bboxes(roi)
    raw, peak = hr.proposal_weights(hr.widen(case["cls"]), hr.widen(case["reg"]))
    assert torch.equal(out["raw_weight"][..., 0], raw) and torch.equal(out["peak_weight"][..., 0], peak)
    sel = [torch.nonzero(peak[n] > 0.1)[:, 0] for n in range(case["N"])]
    assert torch.equal(out["valid_indices"][..., 0], peak > 0.1)
    i2l = torch.linalg.inv(case["img2lidar"].double())            # any invertible lidar2img: the oracle inverts it back
    rows = hr.proposal_rows(hr.widen(case["reg"]), case["strides"], sel, peak, case["depth_logit"].double(), case["ds"], hr.DEPTH_CFG,
                            torch.linalg.inv(i2l), case["feat"].double(), PC)
    assert close(rows["box2d"], torch.cat(out["bbox_list"]))
    roi.update(out)
    roi["pred_depth"] = case["depth_logit"].double().permute(0, 3, 1, 2).softmax(dim=1)
    c3, ctx = orc._proposals(roi, case["feat"].double(), dict(lidar2img=i2l[None]), (case["hd"] * 8, case["wd"] * 8))
    # the oracle un-bins the depth in torch's default dtype whatever its own (`idx / 0.5` on an int64 tensor is float32), so its float64
    # mode carries one float32 rounding of d (6e-8 relative) into the point; the un-binning itself is pinned by hand below
    assert close(c3[0], rows["ref2d"], 2e-7) and close(ctx[0], rows["ctx"])


def test_finalize_and_row_affine_are_the_oracles_expressions(orc):
    g = torch.Generator().manual_seed(5)
    reg, ref, cls = torch.randn(2, 9, 10, generator=g, dtype=torch.float64), torch.rand(9, 3, generator=g, dtype=torch.float64), torch.randn(9, 26, generator=g, dtype=torch.float64)
    ref[0] = torch.tensor([0.0, 1.0, 1.5])
    pc = orc.P(H + "pc_range")
    box, score = hr.finalize(reg, ref, cls, PC)
    xyz = (reg[..., 0:3] + fo.inverse_sigmoid(ref)[None]).sigmoid() * (pc[3:6] - pc[0:3]) + pc[0:3]         # head_forward's line
    assert close(box, torch.cat([xyz, reg[..., 3:]], dim=-1)) and close(score, cls.sigmoid().topk(1, dim=-1).values[..., 0])
    x, c = torch.randn(1, 9, 256, generator=g, dtype=torch.float64), torch.randn(1, 9, 180, generator=g, dtype=torch.float64)
    name = H + "ego_pose_pe"
    h = F.relu(orc._lin(c, name + ".reduce.0"))
    gamma, beta = orc._lin(h, name + ".gamma")[0], orc._lin(h, name + ".beta")[0]
    assert close(hr.row_affine_ln(x[0], gamma, beta), orc._mln(F.layer_norm(x, (256,)), c, name)[0])


# ------------------------------------------------------------------------------------------------ (b) hand-computed layout cases
def test_one_memory_slot_by_hand():
    """Distinct values in every field of one slot: which box channels become the velocity, where each frequency and each of sin / cos sits
    in the 180 / 256 / 384 columns, and that posemb3d is ordered y, x, z."""
    box = torch.arange(10, dtype=torch.float64)[None] + 100.0        # code_size 10: channels 100 .. 109
    m = dict(emb=torch.zeros(0, 4, dtype=torch.float64), ref=torch.zeros(0, 3, dtype=torch.float64), ts=torch.zeros(0, dtype=torch.float64),
             pose=torch.zeros(0, 4, 4, dtype=torch.float64), velo=torch.zeros(0, 2, dtype=torch.float64))
    ego = torch.eye(4, dtype=torch.float64)
    ego[:3, 3] = torch.tensor([1.0, 2.0, 3.0])
    st = hr.post_update(m, torch.tensor([0]), torch.ones(1, 4, dtype=torch.float64), box, ego, 5.5, 1)
    assert st["velo"].tolist() == [[108.0, 109.0]] and st["ref"].tolist() == [[101.0, 103.0, 105.0]] and st["ts"].tolist() == [-5.5]
    assert torch.equal(st["pose"][0], ego)
    # next frame: ego_inv translates by (-2, -2, -2) and turns a quarter about z (x -> y, y -> -x)
    inv = torch.tensor([[0.0, -1.0, 0.0, -2.0], [1.0, 0.0, 0.0, -2.0], [0.0, 0.0, 1.0, -2.0], [0.0, 0.0, 0.0, 1.0]], dtype=torch.float64)
    mm, tref = hr.pre_update(st, inv, 6.0, None, 1.0, 0, PC)
    assert mm["ref"].tolist() == [[-105.0, 99.0, 103.0]] and mm["ts"].tolist() == [0.5] and mm["velo"].tolist() == [[108.0, 109.0]]
    assert mm["pose"][0].tolist() == [[0.0, -1.0, 0.0, -4.0], [1.0, 0.0, 0.0, -1.0], [0.0, 0.0, 1.0, 1.0], [0.0, 0.0, 0.0, 1.0]]
    lo = float(torch.tensor(152.4, dtype=torch.float32))            # the range is a float32 tensor in the reference
    assert abs(tref[0, 0].item() - (-105.0 + lo) / (2 * lo)) < 1e-15 and abs(tref[0, 2].item() - (103.0 + 5.0) / 10.0) < 1e-15
    # motion code: v = [velo (2), ts, pose row 0, row 1, row 2]; column f * 30 + d = sin(v_d 2^f), f * 30 + 15 + d = cos(v_d 2^f)
    velo, ts, pose = torch.tensor([[0.25, -0.5]]), torch.tensor([0.75], dtype=torch.float64), torch.arange(16, dtype=torch.float32).reshape(1, 4, 4) / 8 + 1
    code = hr.motion_code(velo, ts, pose)[0]
    v = [0.25, -0.5, 0.75] + [1 + k / 8 for k in range(12)]
    for f in range(6):
        for d in range(15):
            assert abs(code[f * 30 + d].item() - math.sin(v[d] * 2 ** f)) < 1e-15 and abs(code[f * 30 + 15 + d].item() - math.cos(v[d] * 2 ** f)) < 1e-15
    # time code: column 2 j = sin(2 pi t / 10000^(2 j / 256)), 2 j + 1 = cos(the same)
    tc = hr.time_code(ts, hr.dim_t(256))[0]
    for j in (0, 1, 64, 127):
        a = 2 * math.pi * 0.75 / float(hr.dim_t(256)[2 * j])
        assert abs(tc[2 * j].item() - math.sin(a)) < 1e-15 and abs(tc[2 * j + 1].item() - math.cos(a)) < 1e-15
        assert abs(float(hr.dim_t(256)[2 * j]) - 10000 ** (2 * j / 256)) < 1e-6 * 10000 ** (2 * j / 256)
    # posemb3d: columns [0,128) from y, [128,256) from x, [256,384) from z
    pe = hr.posemb3d(torch.tensor([[0.1, 0.2, 0.3]], dtype=torch.float64), hr.dim_t(128))[0]
    for blk, p in ((0, 0.2), (1, 0.1), (2, 0.3)):
        for j in (0, 5, 63):
            a = 2 * math.pi * p / float(hr.dim_t(128)[2 * j])
            assert abs(pe[blk * 128 + 2 * j].item() - math.sin(a)) < 1e-15 and abs(pe[blk * 128 + 2 * j + 1].item() - math.cos(a)) < 1e-15


def one_level(h, w, obj, cls_logit, nreg=5):
    reg = torch.zeros(1, h, w, nreg, dtype=torch.float64)
    reg[0, ..., 4] = torch.as_tensor(obj, dtype=torch.float64)
    return [torch.as_tensor(cls_logit, dtype=torch.float64).reshape(1, h, w, 1)], [reg]


def test_exact_tie_in_a_window_gives_two_peaks():
    obj = [[0.0, 0.0, 0.0, -1.0], [0.0, 2.0, 2.0, -1.0], [0.0, 0.0, 0.0, 1.0]]
    cls, reg = one_level(3, 4, obj, torch.ones(3, 4))
    raw, peak = hr.proposal_weights(cls, reg)
    s = 1 / (1 + math.exp(-2.0)) / (1 + math.exp(-1.0))
    want = torch.zeros(12, dtype=torch.float64)
    want[5] = want[6] = s                                  # both tied cells are peaks; (2,3) is beaten by its neighbour (1,2)
    assert (peak[0] - want).abs().max().item() < 1e-15 and int((peak[0] > 0).sum()) == 2
    assert hr.peak_margin(cls, reg)[0, 5].item() == 0.0    # an exact tie: margin 0, never skipped


def test_clamped_centre_and_half_cell_by_hand():
    """stride 8, depth stride 8, a (4,6) level and depth map.  Cell (y=1,x=2) with dx = 0.5: cx = 0.5 * 8 + 16 = 20 -> 20 / 8 = 2.5 ->
    round half to even = 2; cell (1,3): cx = 28 -> 3.5 -> 4; cell (0,0) with dx = dy = -5: centre (-40,-40) -> cell (-5,-5) -> clamped
    to (0,0); cell (3,5) with dx = +5: cx = 80 -> 10 -> clamped to 5.  The depth logits make bin = 1 + 6 v + u the arg-max of cell (v,u)."""
    reg = torch.zeros(1, 4, 6, 5, dtype=torch.float64)
    reg[0, 1, 2, 0] = reg[0, 1, 3, 0] = 0.5
    reg[0, 0, 0, :2] = -5.0
    reg[0, 3, 5, 0] = 5.0
    dl = torch.zeros(1, 4, 6, 51, dtype=torch.float64)
    for v in range(4):
        for u in range(6):
            dl[0, v, u, 1 + 6 * v + u] = 1.0
    sel = [torch.tensor([0, 6 + 2, 6 + 3, 18 + 5])]
    rows = hr.proposal_rows([reg], (8,), sel, torch.full((1, 24), 0.5, dtype=torch.float64), dl, 8, hr.DEPTH_CFG, torch.eye(4, dtype=torch.float64)[None],
                            torch.zeros(1, 24, 2, dtype=torch.float64), PC)
    assert rows["box2d"].tolist() == [[-40.0, -40.0, 8.0, 8.0], [20.0, 8.0, 8.0, 8.0], [28.0, 8.0, 8.0, 8.0], [80.0, 24.0, 8.0, 8.0]]
    assert rows["cell"].tolist() == [[0, 0], [2, 1], [4, 1], [5, 3]] and rows["bin"].tolist() == [1, 1 + 6 + 2, 1 + 6 + 4, 1 + 18 + 5]
    # LID un-binning and unprojection with img2lidar = I: d = 0.1 + bs / 8 ((2 b + 1)^2 - 1), point = (cx d, cy d, d)
    bs = 2 * (110.0 - 0.1) / (50 * 51)
    d = 0.1 + bs / 8 * ((2 * 9 + 1) ** 2 - 1)
    lo = float(torch.tensor(152.4, dtype=torch.float32))
    assert abs(rows["ref2d"][1, 0].item() - (20.0 * d + lo) / (2 * lo)) < 1e-12 and abs(rows["ref2d"][1, 2].item() - (d + 5.0) / 10.0) < 1e-12
    assert abs(rows["ctx"][0, 2].item() - (0.0 - math.log(0.1 / 0.9))) < 1e-12      # score 0.5: log-odds 0, minus the threshold's
    assert hr.cell_undecided(rows, 8).tolist() == [False, True, True, False]        # the two half cells sit inside the margin by rule...
    # ... but they are constructed (exact in fp32 as well): the GPU tests' random cases never produce one (census below)


# ------------------------------------------------------------------------------------------------ (c) the exclusion rule
@pytest.mark.parametrize("case_args", hr.PROP_CASES, ids=["-".join(str(x) for x in c) for c in hr.PROP_CASES])
def test_reference_keeps_the_skipped_share_below_one_percent(case_args):
    census = hr.decision_census(hr.proposal_case(*case_args))
    print("[refs] decisions inside the fp32 margin, %s: %s" % ("-".join(str(x) for x in case_args), census))
    for kind, (inside, total) in census.items():
        assert inside <= 0.01 * total, (case_args, kind, inside, total)
    if case_args[3] == "ties":
        assert census["exact_ties"][1] > 0, "the quantised camera must hold exact ties inside 3x3 windows"


# ------------------------------------------------------------------------------------------------ (d) every bound bites
def test_memory_bounds_reject_plausible_slips():
    mc = hr.memory_case(L_, E_, P_, "steady", "city")
    st, inv, T = hr.widen(mc["state"]), mc["ego_inv"].double(), mc["timestamp"]
    lo, span = hr._span(PC, torch.float64)
    m, tref = hr.pre_update(st, inv, T, mc["pseudo_ref"], 1.0, P_, PC)
    bp, br = hr.prepare_bounds(st, mc["ego_inv"], mc["pseudo_ref"], 1.0, P_, lo, span)
    # the fp32 restatement passes its own bound (the bound is not vacuous the other way round)
    m32, _ = hr.pre_update(mc["state"], mc["ego_inv"], T, mc["pseudo_ref"], 1.0, P_, PC)
    assert not exceeds(m32["pose"], m["pose"], bp) and not exceeds(m32["ref"], m["ref"], br)
    # ego_inv applied on the right
    assert exceeds(st["pose"] @ inv, m["pose"], bp)
    # the translation forgotten / the inverse not taken
    assert exceeds((inv[:3, :3] @ st["ref"].T).T, m["ref"], br) and exceeds((mc["ego_pose"].double() @ hr.homog(st["ref"]).T).T[:, :3], m["ref"], br)
    # timestamp path in fp32 at the epoch scale: m_ts is compared for equality
    ts32 = (st["ts"].float() + torch.tensor(T).float()).double()
    assert not torch.equal(ts32, m["ts"]) and (ts32 - m["ts"]).abs().max().item() > 0.05     # 1.7e9 has an fp32 ulp of 128 s
    t64 = hr.time_code(m["ts"], hr.dim_t(256))
    assert exceeds(hr.time_code(ts32, hr.dim_t(256)), t64, hr.chain_bound(hr.yard(t64.float(), t64), t64))
    # temp_ref normalised by the upper corner instead of the span
    assert exceeds((m["ref"] - lo) / torch.tensor(PC[3:], dtype=torch.float64), tref, 2 * 3 * hr.U32 * (m["ref"].abs() + lo.abs()) / span + br / span)
    # the push: velocity from channels code-3, code-2; ego_pose on the right; bit-equality / the warp bound notice
    g = torch.Generator().manual_seed(9)
    dec, box = torch.randn(30, E_, generator=g), torch.randn(30, 10, generator=g)
    idx = torch.randint(0, 30, (16,), generator=g)
    ego = mc["ego_pose"].double()
    want = hr.post_update(m, idx, dec.double(), box.double(), ego, T, L_)
    slip = torch.cat([box[idx][:, 7:9].double(), m["velo"]])[:L_]
    assert not torch.equal(slip, want["velo"])
    pb, rb = hr.post_bounds(m, box.double()[idx][:, :3], 16, L_, mc["ego_pose"])
    kept = torch.cat([torch.eye(4, dtype=torch.float64).expand(16, 4, 4), m["pose"]])[:L_]
    assert exceeds(kept @ ego, want["pose"], pb)
    got32 = hr.post_update(hr.pre_update(mc["state"], mc["ego_inv"], T, mc["pseudo_ref"], 1.0, P_, PC)[0], idx, dec, box, mc["ego_pose"], T, L_)
    assert (got32["pose"].double() - want["pose"]).abs().max().item() < 1e-2      # (error inherited from the fp32 prepare; the GPU sequence test accumulates it)


def test_code_bounds_reject_plausible_slips():
    mc = hr.memory_case(L_, E_, P_, "steady", "city")
    m, _ = hr.pre_update(mc["state"], mc["ego_inv"], mc["timestamp"], mc["pseudo_ref"], 1.0, P_, PC)
    n64 = hr.motion_code(m["velo"], m["ts"], m["pose"])
    bn = hr.chain_bound(hr.yard(hr.motion_code(m["velo"], m["ts"], m["pose"], torch.float32), n64), n64)
    v = hr.motion_input(m["velo"], m["ts"], m["pose"]).double()
    swapped = torch.cat([t for f in range(6) for t in (torch.cos(v * 2 ** f), torch.sin(v * 2 ** f))], dim=-1)
    next_freq = torch.cat([t for f in range(6) for t in (torch.sin(v * 2 ** (f + 1)), torch.cos(v * 2 ** (f + 1)))], dim=-1)
    interleaved = torch.stack([t for f in range(6) for t in (torch.sin(v * 2 ** f), torch.cos(v * 2 ** f))], dim=-1).flatten(-2)
    pose_cols = hr.motion_code(m["velo"], m["ts"], m["pose"].transpose(-1, -2))
    for slip in (swapped, next_freq, interleaved, pose_cols):
        assert exceeds(slip, n64, bn)
    dt = hr.dim_t(256)
    t64 = hr.time_code(m["ts"], dt)
    bt = hr.chain_bound(hr.yard(t64.float(), t64), t64)
    p = (m["ts"].double() * 2 * math.pi)[:, None] / dt.double()
    assert exceeds(torch.stack((p[:, 0::2].cos(), p[:, 1::2].sin()), dim=-1).flatten(-2), t64, bt)            # sin / cos swapped
    assert exceeds(torch.cat((p[:, 0::2].sin(), p[:, 1::2].cos()), dim=-1), t64, bt)                              # not interleaved
    assert exceeds(hr.time_code(m["ts"], hr.dim_t(128).repeat_interleave(2)), t64, bt)                             # the 128-slot table
    g = torch.Generator().manual_seed(2)
    pos = torch.rand(37, 3, generator=g) * 2 - 0.5
    d128 = hr.dim_t(128)
    w = hr.posemb3d(pos.double(), d128)
    bpe = hr.chain_bound(hr.yard(hr.posemb3d(pos, d128), w), w)
    xyz = torch.cat([hr.sincos_code(pos.double()[:, k], d128) for k in range(3)], dim=-1)
    assert exceeds(xyz, w, bpe)                                                                                    # x, y, z order
    assert exceeds(hr.posemb3d(pos.double(), hr.dim_t(128, temperature=1000)), w, bpe)
    assert exceeds(hr.posemb3d(pos.double() / (2 * math.pi), d128), w, bpe)                                         # the 2 pi forgotten


def test_row_and_finalize_bounds_reject_plausible_slips():
    g = torch.Generator().manual_seed(8)
    x, ga, be, ad = (torch.randn(64, 256, generator=g) for _ in range(4))
    x = x * 1.7 + 0.3
    w = hr.row_affine_ln(x.double(), ga.double(), be.double(), ad.double())
    b = hr.chain_bound(hr.yard(hr.row_affine_ln(x, ga, be, ad), w), w)
    xd = x.double()
    unbiased = (xd - xd.mean(-1, keepdim=True)) / torch.sqrt(xd.var(-1, unbiased=True, keepdim=True) + 1e-5)      # variance over C - 1
    assert exceeds(ga.double() * unbiased + be.double() + ad.double(), w, b)
    assert exceeds(hr.row_affine_ln(xd, ga.double(), be.double(), ad.double(), eps=1e-3), w, b)
    assert exceeds(hr.row_affine_ln(xd, be.double(), ga.double(), ad.double()), w, b)                              # gamma / beta swapped
    off = 1e3 + torch.randn(64, 256, generator=g)
    wo = hr.row_affine_ln(off.double(), ga.double(), be.double())
    bo = hr.chain_bound(hr.yard(hr.row_affine_ln(off, ga, be), wo), wo)
    mean, sq = off.mean(-1, keepdim=True), (off * off).mean(-1, keepdim=True)                                      # one pass in fp32
    onepass = ga * ((off - mean) / torch.sqrt((sq - mean * mean).clamp(min=0) + 1e-5)) + be
    assert exceeds(onepass, wo, bo)
    wa = hr.row_affine_ln(xd, ga.double(), be.double(), ad.double(), do_ln=False)
    ba = 2 * 3 * hr.U32 * ((ga.double() * xd).abs() + be.double().abs() + ad.double().abs())
    assert not exceeds(hr.row_affine_ln(x, ga, be, ad, do_ln=False), wa, ba) and exceeds(hr.row_affine_ln(xd, ga.double(), be.double(), None, do_ln=False), wa, ba)
    # finalize: eps = 1e-6 in the inverse sigmoid shows at reference points on / beyond the clamp; the class maximum over all classes
    reg, ref, cls = torch.randn(2, 300, 10, generator=g) * 2, torch.rand(300, 3, generator=g), torch.randn(300, 26, generator=g) * 3
    ref[:3] = torch.tensor([[0.0, 1.0, 5e-6], [1.0, 0.0, 1.0 - 2e-6], [-0.3, 1.2, 9.9e-6]])
    cls[8, 25] = 20.0
    wb, ws = hr.finalize(reg.double(), ref.double(), cls.double(), PC)
    fb, fs = hr.finalize(reg, ref, cls, PC)
    bb, bs = hr.chain_bound(hr.yard(fb[..., :3], wb[..., :3]), wb[..., :3]), hr.chain_bound(hr.yard(fs, ws), ws)
    lo, span = hr._span(PC, torch.float64)
    r64 = ref.double()
    assert exceeds((reg.double()[..., :3] + fo.inverse_sigmoid(r64, eps=1e-6)[None]).sigmoid() * span + lo, wb[..., :3], bb)
    unclamped = torch.log(r64.clamp(min=1e-5) / (1 - r64).clamp(min=1e-5))
    assert exceeds((reg.double()[..., :3] + unclamped[None]).sigmoid() * span + lo, wb[..., :3], bb)
    assert exceeds(cls.double()[:, :25].max(-1).values.sigmoid(), ws, bs) and exceeds(cls.double().sigmoid().mean(-1), ws, bs)


def test_proposal_bounds_reject_plausible_slips():
    case = hr.proposal_case("small3", 26, 5, "wide", with_feat=True)
    cls, reg = hr.widen(case["cls"]), hr.widen(case["reg"])
    raw, peak = hr.proposal_weights(cls, reg)
    raw32, _ = hr.proposal_weights(case["cls"], case["reg"])
    b = hr.chain_bound(hr.yard(raw32, raw), raw)
    slip = torch.cat([(r[..., 4].sigmoid() * c[..., :25].max(-1).values.sigmoid()).reshape(3, -1) for c, r in zip(cls, reg)], dim=1)
    assert exceeds(slip, raw, b)                                                                  # the last class left out of the maximum
    # a 3x3 window that wraps a row (and runs into the next level): the peak decisions differ in decided cells
    flat = F.pad(raw, (1, 1), value=float("-inf"))
    wrapped = raw.clone()
    start = 0
    for h, w in case["hw"]:
        for s in range(start, start + h * w):
            nb = [flat[:, 1 + s + dy * w + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 0 <= s + dy * w + dx < raw.shape[1]]
            wrapped[:, s] = torch.where(raw[:, s] >= torch.stack(nb).max(0).values, raw[:, s], torch.zeros((), dtype=torch.float64))
        start += h * w
    pm = hr.peak_margin(cls, reg)
    decided = ~((pm > 0) & (pm < hr.SCORE_MARGIN))
    assert ((wrapped > 0) != (peak > 0))[decided].any()
    # gather
    sel = [torch.nonzero(peak[n] > 0.1)[:, 0] for n in range(case["N"])]
    args = lambda regs, i2l=case["img2lidar"].double(), ds=case["ds"], cfg=hr.DEPTH_CFG, thr=0.1: hr.proposal_rows(
        regs, case["strides"], sel, peak, case["depth_logit"].double(), ds, cfg, i2l, case["feat"].double(), PC, thr)
    want = args(reg)
    f32 = hr.proposal_rows(case["reg"], case["strides"], sel, peak.float(), case["depth_logit"], case["ds"], hr.DEPTH_CFG, case["img2lidar"],
                           case["feat"], PC)
    cb = hr.centre_bound(want)
    rbound = hr.ref2d_bound(want, case, cb)
    und = hr.cell_undecided(want, case["ds"])
    assert not exceeds(f32["box2d"][:, :2], want["box2d"][:, :2], cb)                            # the fp32 restatement passes ...
    assert not exceeds(f32["ref2d"][~und], want["ref2d"][~und], rbound[~und])
    assert want["box2d"][:, 2:].max().item() > 1e3
    half = [r.clone() for r in reg]
    for r, s in zip(half, case["strides"]):
        r[..., 0:2] += 0.5                                                                        # prior at the cell centre: + stride / 2
    assert exceeds(args(half)["box2d"][:, :2], want["box2d"][:, :2], cb)
    assert exceeds(args(reg, ds=4)["ref2d"][~und], want["ref2d"][~und], rbound[~und])            # the depth map read at the wrong stride
    assert exceeds(args(reg, i2l=case["img2lidar"].double().transpose(1, 2))["ref2d"][~und], want["ref2d"][~und], rbound[~und])
    assert exceeds(args(reg, cfg=dict(hr.DEPTH_CFG, num_depth_bins=51))["ref2d"][~und], want["ref2d"][~und], rbound[~und])
    yl = hr.yard(f32["ctx"][:, -1], want["ctx"][:, -1])
    assert exceeds(args(reg, thr=0.5)["ctx"][:, -1], want["ctx"][:, -1], hr.chain_bound(yl, want["ctx"][:, -1]))     # the threshold's log-odds dropped
    rel = lambda a: ((a.double() - want["box2d"][:, 2:]).abs() / want["box2d"][:, 2:]).max().item()
    bw = 4 * rel(f32["box2d"][:, 2:]) + 2 * hr.ULP32
    lvl = [r.clone() for r in reg]
    lvl[1][..., 2:4] += math.log(2.0)                                                              # level 1 decoded with level 2's stride
    assert rel(args(lvl)["box2d"][:, 2:]) > bw
    # round half to even against floor(x + 0.5) on the constructed half cell (test_clamped_centre_and_half_cell_by_hand): cell 2 against 3
    r1 = torch.zeros(1, 4, 6, 5, dtype=torch.float64)
    r1[0, 1, 2, 0] = 0.5
    dl = torch.zeros(1, 4, 6, 51, dtype=torch.float64)
    for u in range(6):
        dl[0, 1, u, 1 + 5 * u] = 1.0
    c1 = dict(img2lidar=torch.eye(4)[None], pc_range=PC)
    one = lambda dlog: hr.proposal_rows([r1], (8,), [torch.tensor([8])], torch.full((1, 24), 0.5, dtype=torch.float64), dlog, 8, hr.DEPTH_CFG,
                                        torch.eye(4, dtype=torch.float64)[None], torch.zeros(1, 24, 2, dtype=torch.float64), PC)
    even = one(dl)
    assert even["cell"].tolist() == [[2, 1]] and math.floor(2.5 + 0.5) == 3
    up = one(torch.roll(dl, shifts=-1, dims=2))                                                    # what reading cell 3 would give
    assert up["bin"].item() == 16 and even["bin"].item() == 11
    assert exceeds(up["ref2d"], even["ref2d"], hr.ref2d_bound(even, c1, hr.centre_bound(even)))

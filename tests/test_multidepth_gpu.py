"""GPU: multi-depth 2D proposals (multi_depth topk = K > 1; ref farhead.py:754-805).

Kernel level: far3d_proposal_gather_md + far3d_proposal_extra_rows against far3d_proposal_gather (primary rows bit for bit) and a
host restatement of the extra rows.  Engine level: the reference's own K = 2 / K = 3 sequences (tests/golden/far3d_md*_seq.npz) in
the legacy and fixed-capacity threshold modes, graph / pipeline replay against eager, a full-size top-K frame, and the camera-sharded
runner's refusal."""
import json
import os

import numpy as np
import pytest
import torch

from far3d_amd import synth, weights
from tests.conftest import ROOT, assert_detections_match
from tests.test_capacity_gpu import _valid_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(ROOT, "tests", "golden")
DEPTH = dict(num_depth_bins=50, depth_min=0.1, depth_max=110.0, stride=8)
PC = [-152.4, -152.4, -5.0, 152.4, 152.4, 5.0]


def _inputs(N, hw_img, nd, C, feat_dtype, seed, sel_cap, topk):
    """Random 2D-head maps, depth logits, value maps and cameras; the selection by far3d_proposal_select (top-K or threshold)."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(seed)
    H, W = hw_img
    strides = (8, 16, 32, 64)
    hw = [(-(-H // s), -(-W // s)) for s in strides]
    S = sum(h * w for h, w in hw)
    cls = [torch.randn((N, h, w, 26), generator=g).to(DEV) for h, w in hw]
    reg = [(torch.randn((N, h, w, 5), generator=g) * 0.5).to(DEV) for h, w in hw]
    wgt, sel_idx, sel_cnt = ops.proposal_select(cls, reg, strides, sel_cap, thr=0.1, topk=topk)
    hd, wd = hw[0]
    dl = (torch.randn((N, hd, wd, nd), generator=g) * 2).to(DEV)
    feat = torch.randn((N, S, C), generator=g).to(DEV).to(feat_dtype)
    data, _ = synth.make_frame(N, hw_img, seed=seed, frame_index=0)
    i2l = data["lidar2img"][0].inverse().float().contiguous().to(DEV)
    return dict(reg=reg, strides=strides, wgt=wgt, sel_idx=sel_idx, sel_cnt=sel_cnt, dl=dl, feat=feat, i2l=i2l, C=C)


def _bufs(rows, C, fill=float("nan")):
    return (torch.full((rows, 3), fill, device=DEV), torch.full((rows, C + 1), fill, device=DEV), torch.full((rows, 4), fill, device=DEV),
            torch.full((rows,), fill, device=DEV))


def _restate_extras(x, prim, M, K, rmb):
    """Host restatement: per primary row, the top-K bins of its cell by logit (stable: lower bin first on ties), p = softmax in fp32,
    ratios p_k / p_0, valid = bin_0 >= rmb; the extra rows in k-major order."""
    ref2d, ctx, box2d, score = [t[:M].cpu() for t in prim]
    cnt = x["sel_cnt"].cpu().tolist()
    cams = torch.cat([torch.full((c,), n, dtype=torch.long) for n, c in enumerate(cnt)])[:M]
    dl = x["dl"].cpu()
    hd, wd = dl.shape[1:3]
    ds = float(DEPTH["stride"])
    u = torch.round(box2d[:, 0] / ds).long().clamp(0, wd - 1)
    v = torch.round(box2d[:, 1] / ds).long().clamp(0, hd - 1)
    lg = dl[cams, v, u]                                                   # (M, nd)
    order = torch.sort(lg, dim=1, descending=True, stable=True).indices[:, :K]
    p = torch.softmax(lg, dim=1)
    pk = torch.gather(p, 1, order)
    ratio = pk / pk[:, :1]
    valid = order[:, 0] >= rmb
    vr = torch.nonzero(valid).flatten()
    rows = torch.cat([vr] * (K - 1)).long()
    kk = torch.cat([torch.full((len(vr),), k) for k in range(1, K)]).long()
    bins = order[rows, kk].float()
    bin_size = torch.tensor(2.0 * (DEPTH["depth_max"] - DEPTH["depth_min"]) / (DEPTH["num_depth_bins"] * (1.0 + DEPTH["num_depth_bins"])))
    q = bins / 0.5 + 1
    d = DEPTH["depth_min"] + bin_size / 8 * (q * q - 1)
    dm = d.clamp(min=1e-5)
    pts = torch.stack([box2d[rows, 0] * dm, box2d[rows, 1] * dm, d, torch.ones_like(d)], 1)
    w = torch.einsum("rij,rj->ri", x["i2l"].cpu()[cams[rows]], pts)[:, :3]
    lo, hi = torch.tensor(PC[:3]), torch.tensor(PC[3:])
    ref = (w - lo) / (hi - lo)
    ctxe = ctx[rows].clone()
    ctxe[:, -1] = ctx[rows, -1] * ratio[rows, kk]
    return dict(valid=valid, V=len(vr), ref2d=ref, ctx=ctxe, box2d=box2d[rows], score=score[rows], order=order)


def _run_md(x, K, rmb, rows_total, primary_rows=0, sel_cap=0):
    from far3d_amd import ops
    N, cap = x["sel_idx"].shape
    P = primary_rows or N * cap
    out = _bufs(rows_total, x["C"])
    rec = (torch.zeros((P,), dtype=torch.int32, device=DEV), torch.zeros((P, 2 * K), dtype=torch.int32, device=DEV))
    m, ovf = torch.full((1,), -1, dtype=torch.int32, device=DEV), torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ops.proposal_gather_md(x["reg"], x["strides"], x["sel_idx"], x["sel_cnt"], x["wgt"], x["dl"], DEPTH["stride"], DEPTH, x["i2l"],
                           x["feat"], PC, K, rmb, rec, out, primary_rows=primary_rows)
    ops.proposal_extra_rows(x["sel_cnt"], sel_cap, P, K, rec, x["i2l"], DEPTH, PC, out, fill_hole=True, m_out=m, overflow_out=ovf)
    torch.cuda.synchronize()
    return out, rec, int(m.item()), int(ovf.item())


def _check(x, K, rmb, out, m, ovf, rows_total, want_valid=None):
    from far3d_amd import ops
    N, cap = x["sel_idx"].shape
    M = int(x["sel_cnt"].sum().item())
    ref = _bufs(N * cap, x["C"])
    ops.proposal_gather(x["reg"], x["strides"], x["sel_idx"], x["sel_cnt"], x["wgt"], x["dl"], DEPTH["stride"], DEPTH, x["i2l"], x["feat"],
                        PC, out=ref)
    for a, b in zip(out, ref):                                              # primaries: bit for bit the single-depth kernel's rows
        assert torch.equal(a[:M], b[:M])
    r = _restate_extras(x, ref, M, K, rmb)
    V = r["V"]
    if want_valid == "none":
        assert V == 0
    elif want_valid == "all":
        assert V == M
    elif want_valid == "some":
        assert 0 < V < M
    Mx = M + (K - 1) * V
    assert m == min(Mx, rows_total) and ovf == (1 if Mx > rows_total else 0)
    n = m - M                                                               # extras kept, in reference order
    e = slice(M, m)
    assert torch.equal(out[2][e].cpu(), r["box2d"][:n]) and torch.equal(out[3][e].cpu(), r["score"][:n])
    assert torch.equal(out[1][e, :-1].cpu(), r["ctx"][:n, :-1])
    assert torch.allclose(out[1][e, -1].cpu(), r["ctx"][:n, -1], rtol=1e-5, atol=1e-6)
    assert torch.allclose(out[0][e].cpu(), r["ref2d"][:n], rtol=1e-5, atol=1e-5), (out[0][e].cpu() - r["ref2d"][:n]).abs().max()
    for t in out:                                                           # the hole is exactly zero
        assert bool((t[m:rows_total] == 0).all())
    return M, V


@pytest.mark.parametrize("K,feat_dtype", [(2, torch.float32), (3, torch.bfloat16)])
def test_md_kernels_threshold_mode_none_some_all_valid(hip_lib, K, feat_dtype):
    x = _inputs(3, (64, 96), 51, 64, feat_dtype, seed=11 + K, sel_cap=128, topk=False)
    N, cap = x["sel_idx"].shape
    for rmb, want in ((51, "none"), (25, "some"), (0, "all")):
        rows = K * N * cap
        out, rec, m, ovf = _run_md(x, K, rmb, rows)
        _check(x, K, rmb, out, m, ovf, rows, want)


@pytest.mark.parametrize("K", [2, 3])
def test_md_kernels_fixed_capacity_and_overflow(hip_lib, K):
    x = _inputs(2, (64, 96), 51, 32, torch.float32, seed=5, sel_cap=16, topk=True)   # top-K selection: M = 32 static primaries
    M = int(x["sel_cnt"].sum().item())
    out, rec, m, ovf = _run_md(x, K, 25, M + (K - 1) * M, primary_rows=M)
    M_, V = _check(x, K, 25, out, m, ovf, M + (K - 1) * M, "some")
    # capacity below M': the flag is set, the extras are cut in reference order (k-major, primary order), nothing else moves
    small = M + V // 2 + 1
    out, rec, m, ovf = _run_md(x, K, 25, small, primary_rows=M)
    assert m == small and ovf == 1
    _check(x, K, 25, out, m, ovf, small)


def test_md_kernels_full_size(hip_lib):
    """7 cameras x 92 top-K primaries on the benchmark geometry: 640x960 images, an 80x120x51 depth map, C = 256, K = 2."""
    x = _inputs(7, (640, 960), 51, 256, torch.float32, seed=3, sel_cap=92, topk=True)
    M = 7 * 92
    out, rec, m, ovf = _run_md(x, 2, 25, 2 * M, primary_rows=M)
    _check(x, 2, 25, out, m, ovf, 2 * M, "some")


# ------------------------------------------------------------------------------------------ engine level
def test_extra_row_is_a_primary_of_the_swapped_depth_map(hip_lib):
    """The extra rows' reference points come from the code the primaries' come from: with the best and the second-best bin of every
    cell exchanged, plain proposal_gather makes each primary's point from the bin the K = 2 extra row of the same primary used -- the
    same bits, with the same box and context features.  One camera, one 4 x 4 level, 3 proposals, 8 depth bins, C = 8."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(5)
    N, cap, nd, C, K = 1, 3, 8, 8, 2
    depth = dict(num_depth_bins=nd, depth_min=0.1, depth_max=60.0, stride=8)
    cls = [torch.randn((N, 4, 4, 26), generator=g).to(DEV)]
    reg = [(torch.randn((N, 4, 4, 5), generator=g) * 0.5).to(DEV)]
    wgt, sel_idx, sel_cnt = ops.proposal_select(cls, reg, (8,), cap, thr=0.1, topk=True)
    dl = torch.randn((N, 4, 4, nd), generator=g) * 2
    top2 = torch.topk(dl, 2, dim=-1)
    assert bool((top2.values[..., 0] > top2.values[..., 1]).all())          # no ties: best and second-best are defined
    swapped = dl.scatter(-1, top2.indices, top2.values.flip(-1))
    assert torch.equal(torch.topk(swapped, 2, dim=-1).indices, top2.indices.flip(-1))
    feat = torch.randn((N, 16, C), generator=g).to(DEV)
    data, _ = synth.make_frame(N, (32, 32), seed=5, frame_index=0)
    i2l = data["lidar2img"][0].inverse().float().contiguous().to(DEV)
    x = dict(reg=reg, strides=(8,), wgt=wgt, sel_idx=sel_idx, sel_cnt=sel_cnt, dl=dl.to(DEV), feat=feat, i2l=i2l, C=C)
    out, rec = _bufs(K * cap, C), (torch.zeros((cap,), dtype=torch.int32, device=DEV), torch.zeros((cap, 2 * K), dtype=torch.int32, device=DEV))
    m = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    ops.proposal_gather_md(reg, (8,), sel_idx, sel_cnt, wgt, x["dl"], 8, depth, i2l, feat, PC, K, 0, rec, out)
    ops.proposal_extra_rows(sel_cnt, 0, cap, K, rec, i2l, depth, PC, out, m_out=m)
    prim = ops.proposal_gather(reg, (8,), sel_idx, sel_cnt, wgt, swapped.to(DEV), 8, depth, i2l, feat, PC)
    torch.cuda.synchronize()
    assert int(sel_cnt.item()) == cap and int(m.item()) == K * cap and bool((rec[0] == 1).all())    # every primary valid: extra row cap + r
    assert torch.equal(out[0][cap:], prim[0][:cap]) and not torch.equal(out[0][:cap], prim[0][:cap])    # ref2d, bit for bit
    assert torch.equal(out[2][cap:], prim[2][:cap]) and torch.equal(out[1][cap:, :C], prim[1][:cap, :C])


def _md_engine(name, precision="fp32", **over):
    from far3d_amd import engine
    z = np.load(os.path.join(GOLD, name + ".npz"))
    rc = json.loads(bytes(z["recipe"]).decode())
    spec = weights.detector_spec(rc["backbone"], num_query=rc["num_query"], num_propagated=rc["num_propagated"])
    sd = weights.init_state_dict(spec, seed=rc["weight_seed"])
    cfg = engine.default_cfg(backbone=rc["backbone"], num_cams=rc["num_cams"], num_query=rc["num_query"], num_propagated=rc["num_propagated"],
                             memory_len=rc["memory_len"], topk_proposals=rc["topk_proposals"], multi_depth=dict(rc["multi_depth"]), **over)
    return engine.Far3DEngine(sd, cfg, device=DEV, precision=precision), z, rc


def _check_frame(o, z, rc, fi, cls, box, Mx):
    K = rc["multi_depth"]["topk"]
    M, V = int(z["f%d_M" % fi]), int(z["f%d_V" % fi])
    assert Mx == M + (K - 1) * V, "frame %d: M' %d, reference %d" % (fi, Mx, M + (K - 1) * V)
    want_idx = z["f%d_valid_idx" % fi]
    cnt = o["sel_cnt"].cpu().numpy()
    got = [(n, int(i)) for n in range(rc["num_cams"]) for i in o["sel_idx"][n, :cnt[n]].cpu().numpy()]
    assert got == [(int(r[0]), int(r[1])) for r in want_idx], "frame %d: proposal set differs" % fi
    assert o["bbox2d"].shape[0] >= M and np.allclose(o["bbox2d"][:M].cpu().numpy(), z["f%d_bbox2d" % fi], rtol=2e-3, atol=2e-3)
    nq = rc["num_query"]
    ref = o["reference_points"][nq:nq + Mx].cpu().numpy()
    assert np.abs(ref - z["f%d_ref2d" % fi]).max() < 1e-4, "frame %d reference points: %.3e" % (fi, np.abs(ref - z["f%d_ref2d" % fi]).max())
    for key, g in (("all_cls_scores", cls), ("all_bbox_preds", box)):
        want = z["f%d_%s" % (fi, key)]
        assert g.shape == want.shape, (fi, key, g.shape, want.shape)
        err = np.abs(g - want)
        print("%s frame %d %s: max abs err %.3e" % (rc["name"], fi, key, err.max()))
        if key == "all_cls_scores":
            assert err.max() < 1e-3, "frame %d logits: max abs err %.3e" % (fi, err.max())
        else:
            assert err[..., :3].max() < 0.076 and err[..., 3:].max() < 1e-3, "frame %d boxes" % fi


@pytest.mark.parametrize("name", ["far3d_md2_seq", "far3d_md3_seq"])
def test_engine_fp32_multi_depth_matches_reference_legacy_mode(hip_lib, name):
    eng, z, rc = _md_engine(name)
    for fi in range(rc["frames"]):
        data, metas = synth.recipe_frame(rc, fi)
        o = eng.forward_frame(data, metas)
        Mx = o["num_adaptive"]
        _check_frame(o, z, rc, fi, o["all_cls_scores"].cpu().numpy(), o["all_bbox_preds"].cpu().numpy(), Mx)
        assert o["bbox2d"].shape[0] == int(z["f%d_M" % fi])                 # the 2D outputs keep the primaries only
        r = o["result"]
        keep = r["keep"].cpu().numpy()
        assert_detections_match(tuple(r[k].cpu().numpy()[keep] for k in ("labels_3d", "boxes_3d", "scores_3d")),
                                tuple(z["f%d_%s" % (fi, k)] for k in ("labels_3d", "boxes_3d", "scores_3d")), "frame %d" % fi)


@pytest.mark.parametrize("name", ["far3d_md2_seq", "far3d_md3_seq"])
def test_engine_fp32_multi_depth_matches_reference_fixed_capacity(hip_lib, name):
    cap = 48
    eng, z, rc = _md_engine(name, proposal_capacity=cap)
    K = rc["multi_depth"]["topk"]
    rows = cap * K
    assert eng.static_adaptive_rows() == rows
    nq = rc["num_query"]
    for fi in range(rc["frames"]):
        data, metas = synth.recipe_frame(rc, fi)
        o = eng.forward_frame(data, metas)
        eng.check_proposal_overflow()
        Mx = int(o["num_adaptive_dev"].item())
        assert o["num_adaptive"] == rows
        cls, box = o["all_cls_scores"], o["all_bbox_preds"]
        _check_frame(o, z, rc, fi, _valid_rows(cls, 2, nq, Mx, rows).cpu().numpy(), _valid_rows(box, 2, nq, Mx, rows).cpu().numpy(), Mx)
        hole = cls[:, 0, nq + Mx:nq + rows]
        assert hole.numel() > 0 and bool(torch.isinf(hole).all())
        r = o["result"]
        keep = r["keep"].cpu().numpy()
        assert_detections_match(tuple(r[k].cpu().numpy()[keep] for k in ("labels_3d", "boxes_3d", "scores_3d")),
                                tuple(z["f%d_%s" % (fi, k)] for k in ("labels_3d", "boxes_3d", "scores_3d")), "frame %d" % fi)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_engine_multi_depth_graph_and_pipeline_bitwise_eager(hip_lib, precision):
    res = {}
    for mode in ("eager", "graph", "pipeline"):
        eng, z, rc = _md_engine("far3d_md2_seq", precision, proposal_capacity=48)
        eng.use_graph = mode != "eager"
        eng.pipeline = mode == "pipeline"
        out = []
        for fi in list(range(rc["frames"])) + [rc["frames"] - 1] * 5:      # + steady frames: every pipeline buffer set captures and replays
            data, metas = synth.recipe_frame(rc, fi)
            o = eng.forward_frame(data, metas)
            eng.wait_outputs()
            eng.check_proposal_overflow()
            out.append((int(o["num_adaptive_dev"].item()), o["all_cls_scores"].clone(), o["all_bbox_preds"].clone(),
                        o["reference_points"].clone(), {k: v.clone() for k, v in eng.mem.items()}))
        res[mode] = out
    for mode in ("graph", "pipeline"):
        for fi, (a, b) in enumerate(zip(res["eager"], res[mode])):
            assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]), \
                "frame %d: %s differs from eager" % (fi, mode)
            for k in a[4]:
                assert torch.equal(a[4][k], b[4][k]), "frame %d (%s): streaming memory '%s' differs" % (fi, mode, k)


def test_engine_multi_depth_full_size_topk_graph(hip_lib):
    """One 7 x 640 x 960 scene, proposal_topk = 92 (644 primaries), K = 2, graph mode: M' = 644 + V with V recomputed from the
    engine's own depth logits and selections; A = 644 + 1288 + 256 = 2188 queries x 26 classes runs the decode's workspace path."""
    from far3d_amd import engine, ops
    spec = weights.detector_spec("V-99-eSE")
    sd = weights.init_state_dict(spec, seed=1)
    eng = engine.Far3DEngine(sd, engine.default_cfg(proposal_topk=92, multi_depth=dict(topk=2, range_min=30)), device=DEV, precision="bf16")
    eng.use_graph = True
    nq, P = 644, 7 * 92
    assert eng.static_adaptive_rows() == 2 * P
    rmb = ops.depth_range_min_bin(eng.cfg["depthnet"], 30)
    for fi in range(3):                                                     # frame 0 eager (scene start), then capture + replays
        data, metas = synth.make_frame(7, (640, 960), seed=4, frame_index=fi)
        o = eng.forward_frame(data, metas)
        torch.cuda.synchronize()
        cls = o["all_cls_scores"]
        assert cls.shape[2] == nq + 2 * P + 256 == 2188
        assert o["all_cls_scores"].shape[2] * 26 > 40960 and ops.decode_ws_bytes(cls.shape[2] * 26, 300) > 0
        # V from the engine's own depth logits at the primaries' cells (first maximum, like the kernels)
        box = o["bbox2d"].cpu()
        assert box.shape[0] == P
        dl = o["depth_logit"].cpu()
        hd, wd = dl.shape[1:3]
        cams = torch.arange(7).repeat_interleave(92)
        u = torch.round(box[:, 0] / 8).long().clamp(0, wd - 1)
        v = torch.round(box[:, 1] / 8).long().clamp(0, hd - 1)
        V = int((torch.argmax(dl[cams, v, u], dim=1) >= rmb).sum())
        Mx = int(o["num_adaptive_dev"].item())
        assert Mx == P + V and 0 < V, (Mx, V)
        live = torch.cat([cls[:, 0, :nq + Mx], cls[:, 0, nq + 2 * P:]], dim=1)
        assert bool(torch.isfinite(live).all())
        hole = cls[:, 0, nq + Mx:nq + 2 * P]
        assert hole.numel() == 0 or bool(torch.isinf(hole).all())
        assert bool(torch.isfinite(o["result"]["scores_3d"]).all())


def test_sharded_frame_refuses_multi_depth(hip_lib):
    from far3d_amd import dist
    eng, z, rc = _md_engine("far3d_md2_seq", proposal_topk=16)
    with pytest.raises(ValueError, match="topk=2"):
        dist.ShardedFrame(eng)

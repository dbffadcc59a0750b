"""Times of the foreign-2D-head path at the benchmark geometry (7 cameras x 640 x 960: token maps 80x120 ... 10x15 x 256 channels,
92 proposals per camera = 644 adaptive queries), beside the native pair, in one job.

  python tools/probe/foreign_head_times.py [--out profiles/foreign_head/times.txt] [--rounds 7]

Recorded, not asserted:
  kernels  far3d_proposal_select (top-92 mode) + far3d_proposal_gather  against  far3d_mask_compact + far3d_proposal_from_boxes on
           the mask / boxes / scores the native pair produced (hipGraph replay, alternating repetitions), each kernel alone too, and
           the multi-depth forms (topk = 3) with far3d_proposal_extra_rows.
  module   plugin.FarHead.forward (bf16 modules) on the native dict and on the same dict in the reference's format (device tensors),
           host clock around the call (it ends in the read of M), alternating repetitions.

The driver starts one child process per step, each under its own time limit, and stops at the first step that does not end cleanly."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "probe"))
from vov_family_times import graph_us  # noqa: E402

N, C, K_PROP = 7, 256, 92
HW = ((80, 120), (40, 60), (20, 30), (10, 15))
STRIDES = (8, 16, 32, 64)
DEPTH = dict(depth_min=0.1, depth_max=110.0, num_depth_bins=50)
PC = [-152.4, -152.4, -5.0, 152.4, 152.4, 5.0]
STEP_LIMIT = 240
REPS = 5
DEV = "cuda:0"


def _maps(seed=1, ncls=26, nreg=5):
    import torch
    from far3d_amd import synth
    g = torch.Generator().manual_seed(seed)
    cls = [(torch.randn(N, h, w, ncls, generator=g) * 2 - 1).to(DEV) for h, w in HW]
    reg = [torch.randn(N, h, w, nreg, generator=g).to(DEV) for h, w in HW]
    depth = torch.randn(N, HW[0][0], HW[0][1], DEPTH["num_depth_bins"] + 1, generator=g).to(DEV)
    S = sum(h * w for h, w in HW)
    feat = torch.randn(N, S, C, generator=g).to(torch.bfloat16).to(DEV)
    i2l = torch.linalg.inv(synth.ring_cameras(N, (640, 960), dtype=torch.float64)[2]).float().contiguous().to(DEV)
    return cls, reg, depth, feat, i2l, S


def step_kernels(rounds):
    import torch
    from far3d_amd import ops
    cls, reg, depth, feat, i2l, S = _maps()
    wgt, idx, cnt = ops.proposal_select(cls, reg, STRIDES, K_PROP, topk=True)
    rows = N * K_PROP
    out = ops.proposal_gather(reg, STRIDES, idx, cnt, wgt, depth, 8, DEPTH, i2l, feat, PC, 0.1)
    mask = torch.zeros(N, S, dtype=torch.bool, device=DEV)
    for n in range(N):
        mask[n, idx[n].long()] = True
    boxes, scores = out[2].clone(), out[3].clone()
    prob_nchw = depth.softmax(dim=-1).permute(0, 3, 1, 2).contiguous()
    idx2, cnt2 = ops.mask_compact(mask, K_PROP)
    o2 = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    ops.proposal_from_boxes(boxes, cnt, scores, idx2, cnt2, depth, 8, DEPTH, i2l, feat, PC, depth_is_prob=False, out=o2)
    torch.cuda.synchronize()
    same = bool(torch.equal(idx2, idx)) and bool(torch.equal(o2[0], out[0])) and bool(torch.equal(o2[1], out[1]))
    print(json.dumps(dict(kind="check", same_rows_as_native=same, proposals=int(cnt.sum().item()), S=S)), flush=True)

    def native():
        w, i, c = ops.proposal_select(cls, reg, STRIDES, K_PROP, topk=True)
        ops.proposal_gather(reg, STRIDES, i, c, w, depth, 8, DEPTH, i2l, feat, PC, 0.1, out=out)

    def foreign():
        i, c = ops.mask_compact(mask, K_PROP)
        ops.proposal_from_boxes(boxes, cnt, scores, i, c, prob_nchw, 8, DEPTH, i2l, feat, PC, depth_is_prob=True, depth_layout="nchw", out=o2)

    singles = [("far3d_proposal_select (top-92)", lambda: ops.proposal_select(cls, reg, STRIDES, K_PROP, topk=True)),
               ("far3d_proposal_gather", lambda: ops.proposal_gather(reg, STRIDES, idx, cnt, wgt, depth, 8, DEPTH, i2l, feat, PC, 0.1, out=out)),
               ("far3d_mask_compact", lambda: ops.mask_compact(mask, K_PROP)),
               ("far3d_proposal_from_boxes (probabilities, N,D,h,w)", lambda: ops.proposal_from_boxes(
                   boxes, cnt, scores, idx2, cnt2, prob_nchw, 8, DEPTH, i2l, feat, PC, depth_is_prob=True, depth_layout="nchw", out=o2)),
               ("far3d_proposal_from_boxes (logits, N,h,w,D)", lambda: ops.proposal_from_boxes(
                   boxes, cnt, scores, idx2, cnt2, depth, 8, DEPTH, i2l, feat, PC, depth_is_prob=False, out=o2))]
    for name, fn in singles:
        med, mn = graph_us(fn, 10, rounds)
        print(json.dumps(dict(kind="single", name=name, us=med, us_min=mn)), flush=True)
    for rep in range(REPS):
        a, _ = graph_us(native, 10, rounds)
        b, _ = graph_us(foreign, 10, rounds)
        print(json.dumps(dict(kind="pair", rep=rep, native_us=a, foreign_us=b)), flush=True)
    # multi-depth, topk = 3
    K = 3
    big = lambda: (torch.empty((K * rows, 3), device=DEV), torch.empty((K * rows, C + 1), device=DEV), torch.zeros((K * rows, 4), device=DEV),
                   torch.zeros((K * rows,), device=DEV))
    rec = lambda: (torch.zeros((rows,), dtype=torch.int32, device=DEV), torch.empty((rows, 2 * K), dtype=torch.int32, device=DEV))
    pa, ra, pb, rb = big(), rec(), big(), rec()
    pb[2][:rows], pb[3][:rows] = boxes, scores
    m_dev = torch.zeros((1,), dtype=torch.int32, device=DEV)
    rmb = ops.depth_range_min_bin(DEPTH, 30)

    def native_md():
        w, i, c = ops.proposal_select(cls, reg, STRIDES, K_PROP, topk=True)
        ops.proposal_gather_md(reg, STRIDES, i, c, w, depth, 8, DEPTH, i2l, feat, PC, K, rmb, ra, pa)
        ops.proposal_extra_rows(c, 0, rows, K, ra, i2l, DEPTH, PC, pa, fill_hole=False, m_out=m_dev)

    def foreign_md():
        i, c = ops.mask_compact(mask, K_PROP)
        ops.proposal_from_boxes(pb[2], cnt, pb[3], i, c, prob_nchw, 8, DEPTH, i2l, feat, PC, depth_is_prob=True, depth_layout="nchw",
                                topk=K, range_min_bin=rmb, records=rb, out=pb, rows=rows)
        ops.proposal_extra_rows(cnt, 0, rows, K, rb, i2l, DEPTH, PC, pb, fill_hole=False, m_out=m_dev)

    for rep in range(REPS):
        a, _ = graph_us(native_md, 10, rounds)
        b, _ = graph_us(foreign_md, 10, rounds)
        print(json.dumps(dict(kind="pair_md", rep=rep, native_us=a, foreign_us=b)), flush=True)


def step_module(rounds):
    import torch
    from far3d_amd import config, ops, plugin, synth
    det = plugin.build_detector(config.default_model_cfg())
    det.init_weights(seed=1)
    head = det.pts_bbox_head
    cls, reg, depth, _, _, S = _maps(ncls=head.num_classes)
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn(1, N, C, h, w, generator=g).to(DEV) for h, w in HW]
    data, metas = synth.make_frame(N, (640, 960), seed=5, frame_index=0)
    dd = {k: v.to(DEV) for k, v in data.items() if k != "img"}
    wgt, idx, cnt = ops.proposal_select(cls, reg, STRIDES, K_PROP, topk=True)
    eye = torch.eye(4, device=DEV)[None].repeat(N, 1, 1).contiguous()
    _, _, box2d, score = ops.proposal_gather(reg, STRIDES, idx, cnt, wgt, depth, 8, DEPTH, eye, torch.zeros((N, S, C), device=DEV), PC, 0.1)
    native = dict(_far3d=dict(cls=cls, reg=reg, depth_logit=depth, depth_stride=8, sel_idx=idx, sel_cnt=cnt, peak_weight=wgt))
    mask = torch.zeros(N, S, 1, dtype=torch.bool, device=DEV)
    for n in range(N):
        mask[n, idx[n].long(), 0] = True
    foreign = dict(bbox_list=[box2d[n * K_PROP:(n + 1) * K_PROP] for n in range(N)], bbox2d_scores=score[:N * K_PROP, None], valid_indices=mask,
                   pred_depth=depth.softmax(dim=-1).permute(0, 3, 1, 2).contiguous())
    prev = torch.ones(1)

    def call(roi):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = head(metas, roi, img_feats=feats, prev_exists=prev, **dd)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    for roi in (native, foreign, native, foreign):            # warm up both paths
        call(roi)
    head.reset_memory()
    _, a = call(native)
    head.reset_memory()
    _, b = call(foreign)
    diff = (a["all_cls_scores"].float() - b["all_cls_scores"].float()).abs().max().item()
    print(json.dumps(dict(kind="module_check", rows=int(a["reference_points2d"].shape[1]), rows_foreign=int(b["reference_points2d"].shape[1]),
                          logits_diff=diff)), flush=True)
    for rep in range(REPS):
        ta = sorted(call(native)[0] for _ in range(rounds))
        tb = sorted(call(foreign)[0] for _ in range(rounds))
        print(json.dumps(dict(kind="module", rep=rep, native_ms=ta[len(ta) // 2], foreign_ms=tb[len(tb) // 2])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foreign_head", "times.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step", default=None, help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        return step_kernels(a.rounds) if a.step == "kernels" else step_module(a.rounds)
    rows = []
    for step in ("kernels", "module"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--rounds", str(a.rounds)], capture_output=True,
                               text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            sys.exit("step %s did not finish within %d s; stopping" % (step, STEP_LIMIT))
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("step %s ended with status %d; stopping" % (step, r.returncode))
        rows += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        print("step %s done" % step, flush=True)
    write(rows, a.out)


def write(rows, path):
    L = ["Foreign-2D-head path at %d x 640 x 960 (token maps %s x %d channels, %d proposals per camera), median of the rounds" %
         (N, ", ".join("%dx%d" % hw for hw in HW), C, K_PROP), ""]
    for r in rows:
        if r["kind"] == "check":
            L.append("from_boxes on the native pair's boxes, logits and selection: rows bit-equal to the native rows: %s (%d proposals, S = %d)" %
                     (r["same_rows_as_native"], r["proposals"], r["S"]))
    L += ["", "single calls, hipGraph replay (us, median (min))"]
    for r in rows:
        if r["kind"] == "single":
            L.append("  %-52s %8.1f (%7.1f)" % (r["name"], r["us"], r["us_min"]))
    for kind, title in (("pair", "select + gather  against  mask_compact + from_boxes"),
                        ("pair_md", "topk = 3: select + gather_md + extra_rows  against  mask_compact + from_boxes + extra_rows")):
        mine = [r for r in rows if r["kind"] == kind]
        if not mine:
            continue
        L += ["", "%s, %d alternating repetitions (us per pair)" % (title, len(mine)), "  %3s %10s %10s" % ("rep", "native", "foreign")]
        L += ["  %3d %10.1f %10.1f" % (r["rep"], r["native_us"], r["foreign_us"]) for r in mine]
        a, b = [r["native_us"] for r in mine], [r["foreign_us"] for r in mine]
        L.append("  mean native %.1f, mean foreign %.1f; run-to-run spread %.1f" % (sum(a) / len(a), sum(b) / len(b), max(max(a) - min(a), max(b) - min(b))))
    for r in rows:
        if r["kind"] == "module_check":
            L += ["", "FarHead.forward, bf16 modules: %d adaptive-query rows native, %d foreign, largest logit difference %.3e" %
                  (r["rows"], r["rows_foreign"], r["logits_diff"])]
    mine = [r for r in rows if r["kind"] == "module"]
    if mine:
        L += ["FarHead.forward, host clock around the call, %d alternating repetitions (ms, median)" % len(mine), "  %3s %10s %10s" % ("rep", "native", "foreign")]
        L += ["  %3d %10.3f %10.3f" % (r["rep"], r["native_ms"], r["foreign_ms"]) for r in mine]
        a, b = [r["native_ms"] for r in mine], [r["foreign_ms"] for r in mine]
        L.append("  mean native %.3f, mean foreign %.3f; run-to-run spread %.3f" % (sum(a) / len(a), sum(b) / len(b), max(max(a) - min(a), max(b) - min(b))))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()

"""Times of the fused depthwise-separable layer (far3d_dwsep_conv_nhwc) against the two launches it replaces (far3d_dwconv3x3[_act]_nhwc
into a scratch map + far3d_conv2d_nhwc), at the benchmark geometry 7 x 640 x 960, hipGraph replay.

  python tools/probe/dwsep_times.py [--out profiles/dwsep/times.txt] [--rounds 5]

Recorded, not asserted:
  layer    per layer shape and storage (bf16, pair), fused and two-launch alternating in ONE process, five repetitions each, so that the
           run-to-run spread of either side is known: microseconds and algorithmic bytes per second (fused: input + output + weights;
           two launches: the same plus the scratch map written and read back).  Shapes: the four tower levels (256 -> 256, bias + Swish
           on both halves) and the six V-19-dw-eSE layer shapes (stem2, stem3 at stride 2, the layers of stages 2-5; ReLU after the 1x1).
  roi      engine.roi_head with depthwise towers (depth on p3), fused_dwsep off and on, bf16 and bf16x3.
  backbone engine.backbone of V-19-dw-eSE, fused_dwsep off and on, bf16 and bf16x3.

The driver starts one child process per step, each under its own time limit, and stops at the first step that does not end cleanly."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "probe"))
from vov_family_times import graph_us  # noqa: E402

N = 7
STEP_LIMIT = 300      # seconds per child
REPS = 5
# (name, H, W, C, Cout, stride, act1, bias1, act2)
TOWERS = [("tower p%d" % (3 + i), h, w, 256, 256, 1, "swish", True, "swish") for i, (h, w) in enumerate(((80, 120), (40, 60), (20, 30), (10, 15)))]
VOV = [("stem2", 320, 480, 64, 64, 1, None, False, "relu"), ("stem3", 320, 480, 64, 64, 2, None, False, "relu"),
       ("stage2", 160, 240, 128, 128, 1, None, False, "relu"), ("stage3", 80, 120, 160, 160, 1, None, False, "relu"),
       ("stage4", 40, 60, 192, 192, 1, None, False, "relu"), ("stage5", 20, 30, 224, 224, 1, None, False, "relu")]


def step_layers(dt, rounds):
    import torch
    from far3d_amd import ops
    pair = dt == "pair"
    dev = "cuda:0"
    for name, H, W, C, Cout, stride, act1, bias1, act2 in TOWERS + VOV:
        g = torch.Generator().manual_seed(1)
        x = torch.randn(N, H, W, C, generator=g).to(dev)
        xs = ops.pair_from_float(x) if pair else x.to(torch.bfloat16)
        del x
        w9 = (torch.randn(9, C, generator=g) / 3).to(dev)
        b1 = (torch.randn(C, generator=g) / 4).to(dev) if bias1 else None
        wp, b2 = torch.randn(Cout, C, generator=g) * (2.0 / C) ** 0.5, torch.randn(Cout, generator=g) / 4
        pc = (ops.PackedConv(wp, b2, dtype=torch.float32, device=dev, compute="bf16x3") if pair else
              ops.PackedConv(wp, b2, dtype=torch.bfloat16, device=dev))
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        cs = 2 if pair else 1
        tmp = torch.empty((N, Ho, Wo, C * cs), dtype=xs.dtype, device=dev)
        out = torch.empty((N, Ho, Wo, Cout * cs), dtype=xs.dtype, device=dev)
        nb = lambda *ts: sum(t.numel() * t.element_size() for t in ts if t is not None)
        wbytes = Cout * C * (4 if pair else 2) + 4 * Cout
        fused_bytes = nb(xs, out, w9, b1) + wbytes
        split_bytes = fused_bytes + 2 * nb(tmp)

        def fused():
            ops.dwsep_conv_nhwc(xs, w9, pc, stride, bias1=b1, act1=act1, act2=act2, out=out, pair=pair)

        def split():
            if act1 is None and b1 is None:           # the engine's _layer3
                ops.dwconv3x3_nhwc(xs, w9, stride, out=tmp, pair=pair)
            else:                                     # the engine's _light_towers
                ops.dwconv3x3_act_nhwc(xs, w9, stride, bias=b1, act=act1, out=tmp, pair=pair)
            ops.conv2d_nhwc(tmp, pc, out=out, act=act2)
        iters = 10 if N * Ho * Wo <= 7 * 160 * 240 else 4
        for rep in range(REPS):                       # alternating: fused, two launches, fused, ...
            f, _ = graph_us(fused, iters, rounds)
            s, _ = graph_us(split, iters, rounds)
            print(json.dumps(dict(kind="layer", dt=dt, name=name, shape=[N, H, W, C, Cout, stride], rep=rep, fused_us=f, split_us=s,
                                  fused_bytes=fused_bytes, split_bytes=split_bytes)), flush=True)
        del xs, tmp, out
        torch.cuda.empty_cache()


def step_roi(precision, rounds):
    import torch
    from far3d_amd import engine, weights
    spec = {k: v for k, v in weights.detector_spec(roi_depthwise=True).items() if k.startswith("img_roi_head.")}
    eng = engine.Far3DEngine(weights.init_state_dict(spec, seed=1), engine.default_cfg(roi_depthwise=True, depth_level=0), device="cuda:0",
                             precision=precision, parts=("roi",))
    g = torch.Generator().manual_seed(3)
    raw = [eng.act_from_nchw(torch.randn(N, 256, h, w, generator=g).to("cuda:0")) for _, h, w, *_ in TOWERS]
    for rep in range(REPS):
        row = dict(kind="total", what="light roi_head (depthwise towers, depth on p3)", precision=precision, rep=rep)
        for key, flag in (("fused_ms", True), ("split_ms", False)):
            eng.fused_dwsep = flag
            row[key] = graph_us(lambda: eng.roi_head(raw), 2, rounds)[0] / 1e3
        print(json.dumps(row), flush=True)


def step_backbone(precision, rounds):
    import torch
    from far3d_amd import engine, weights
    name = "V-19-dw-eSE"
    eng = engine.Far3DEngine(weights.init_state_dict(weights.backbone_spec(name), seed=1), engine.default_cfg(backbone=name), device="cuda:0",
                             precision=precision, parts=("backbone",))
    img = torch.randn(N, 3, 640, 960, generator=torch.Generator().manual_seed(0)).to("cuda:0")
    for rep in range(REPS):
        row = dict(kind="total", what="%s backbone" % name, precision=precision, rep=rep)
        for key, flag in (("fused_ms", True), ("split_ms", False)):
            eng.fused_dwsep = flag
            row[key] = graph_us(lambda: eng.backbone(img), 1, rounds)[0] / 1e3
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwsep", "times.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", default=None, help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        kind, _, arg = a.step.partition(":")
        return {"layers": step_layers, "roi": step_roi, "backbone": step_backbone}[kind](arg, a.rounds)
    rows = []
    for step in ("layers:bf16", "layers:pair", "roi:bf16", "roi:bf16x3", "backbone:bf16", "backbone:bf16x3"):
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


def _stats(v):
    return sum(v) / len(v), max(v) - min(v)


def write(rows, path):
    L = ["Fused depthwise-separable layer against its two launches at %d x 640 x 960, hipGraph replay, %d alternating repetitions" % (N, REPS),
         "(each the median of the rounds); mean us, [spread = max - min over the repetitions], algorithmic TB/s", "",
         "%-5s %-10s %-24s %18s %18s %7s %12s %12s" % ("dtype", "layer", "N,H,W,C,Cout,stride", "fused us [spread]", "2-launch us [spr]", "ratio",
                                                      "fused TB/s", "2-launch TB/s")]
    keys = []
    for r in rows:
        if r["kind"] == "layer" and (r["dt"], r["name"]) not in keys:
            keys.append((r["dt"], r["name"]))
    for dt, name in keys:
        mine = [r for r in rows if r["kind"] == "layer" and r["dt"] == dt and r["name"] == name]
        (f, fs), (s, ss) = _stats([r["fused_us"] for r in mine]), _stats([r["split_us"] for r in mine])
        L.append("%-5s %-10s %-24s %10.1f [%5.1f] %10.1f [%5.1f] %7.2f %12.2f %12.2f" %
                 (dt, name, ",".join(map(str, mine[0]["shape"])), f, fs, s, ss, f / s, mine[0]["fused_bytes"] / f / 1e6, mine[0]["split_bytes"] / s / 1e6))
    L += ["", "engine totals, fused_dwsep on / off (ms)", "%-7s %-50s %18s %18s %7s" % ("mode", "what", "fused ms [spread]", "2-launch ms [spr]", "ratio")]
    keys = []
    for r in rows:
        if r["kind"] == "total" and (r["precision"], r["what"]) not in keys:
            keys.append((r["precision"], r["what"]))
    for prec, what in keys:
        mine = [r for r in rows if r["kind"] == "total" and r["precision"] == prec and r["what"] == what]
        (f, fs), (s, ss) = _stats([r["fused_ms"] for r in mine]), _stats([r["split_ms"] for r in mine])
        L.append("%-7s %-50s %9.3f [%6.3f] %9.3f [%6.3f] %7.2f" % (prec, what, f, fs, s, ss, f / s))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()

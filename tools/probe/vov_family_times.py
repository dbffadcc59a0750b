"""Backbone times of the VoVNet family at the benchmark geometry (7 x 640 x 960, hipGraph replay), per spec and precision, and the
depthwise kernel alone on the layers of the two depthwise specs: microseconds per layer and achieved bytes/s against its algorithmic
bytes (input + output + weights) at 8 TB/s.  Recorded, not asserted: nobody had timed these backbones.

  python tools/probe/vov_family_times.py [--out profiles/vov_family/backbone_times.txt] [--rounds 5]

The driver starts one child process per step (a spec's precisions; the depthwise layers), each under its own time limit, and stops at
the first step that does not end cleanly -- the steps are chained like `a && b && c`.  Every child prints JSON lines; the driver
formats them and writes the file."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SPECS = ("V-19-slim-dw-eSE", "V-19-dw-eSE", "V-19-slim-eSE", "V-19-eSE", "V-99-eSE")
N, H, W = 7, 640, 960
HBM = 8e12
STEP_LIMIT = 240      # seconds per child


def dw_layers(spec):
    """(name, H, W, C, stride, count) of the depthwise launches of one frame's image (per camera map sizes at 640 x 960)."""
    from far3d_amd import weights
    s = weights.VOV_SPECS[spec]
    out = [("stem2", H // 2, W // 2, s["stem"][1], 1, 1), ("stem3", H // 2, W // 2, s["stem"][2], 2, 1)]
    h, w = H // 4, W // 4
    for si, c in enumerate(s["stage_conv_ch"]):
        out.append(("stage%d" % (si + 2), h, w, c, 1, s["layer_per_block"] * s["block_per_stage"][si]))
        h, w = h // 2, w // 2
    return out


def graph_us(fn, iters, rounds):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / (3 * iters))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def step_backbone(spec, rounds):
    import torch
    from far3d_amd import engine, weights
    sd = weights.init_state_dict(weights.backbone_spec(spec), seed=1)
    img = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(0)).to("cuda:0")
    for prec in ("bf16", "bf16x3", "fp32"):
        try:
            eng = engine.Far3DEngine(sd, engine.default_cfg(backbone=spec), device="cuda:0", precision=prec, parts=("backbone",))
        except ValueError:       # the engine's own refusal (a slim spec in a pair-stored mode): reported as "refused"
            continue
        med, mn = graph_us(lambda: eng.backbone(img, keep_stage2=False), 2, rounds)
        print(json.dumps(dict(kind="backbone", spec=spec, precision=prec, ms=med / 1e3, ms_min=mn / 1e3)), flush=True)
        del eng
        torch.cuda.empty_cache()


def step_dw(rounds):
    import torch
    from far3d_amd import ops, weights
    for spec in SPECS:
        if not weights.is_dw(spec):
            continue
        for name, h, w, c, stride, count in dw_layers(spec):
            for dt in ("bf16", "pair", "f32"):
                if dt == "pair" and c % 32:
                    continue
                x = torch.randn(N, h, w, c, generator=torch.Generator().manual_seed(1)).to("cuda:0")
                xs = ops.pair_from_float(x) if dt == "pair" else x.to(torch.bfloat16 if dt == "bf16" else torch.float32)
                w9 = (torch.randn(9, c, generator=torch.Generator().manual_seed(2)) / 3).to("cuda:0")
                out = ops.dwconv3x3_nhwc(xs, w9, stride, pair=dt == "pair")
                med, mn = graph_us(lambda: ops.dwconv3x3_nhwc(xs, w9, stride, out=out, pair=dt == "pair"), 10, rounds)
                nbytes = xs.numel() * xs.element_size() + out.numel() * out.element_size() + w9.numel() * 4
                print(json.dumps(dict(kind="dw", spec=spec, layer=name, shape=[N, h, w, c], stride=stride, count=count, dt=dt, us=med,
                                      us_min=mn, bytes=nbytes, out_bytes=out.numel() * out.element_size(), tbps=nbytes / (med * 1e-6) / 1e12)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vov_family", "backbone_times.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", default=None, help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        kind, _, spec = a.step.partition(":")
        return step_dw(a.rounds) if kind == "dw" else step_backbone(spec, a.rounds)
    rows = []
    for step in ["backbone:" + s for s in SPECS] + ["dw"]:
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
    bb = {(r["spec"], r["precision"]): r for r in rows if r["kind"] == "backbone"}
    dw = [r for r in rows if r["kind"] == "dw"]
    L = ["VoVNet family, backbone alone, %d x %d x %d, hipGraph replay, median (min) of the rounds; keep_stage2=False as in the detector's frames" % (N, H, W),
         "", "%-18s %14s %14s %14s" % ("spec", "bf16 ms", "bf16x3 ms", "fp32 ms")]
    for s in SPECS:
        cell = lambda p: "%6.2f (%5.2f)" % (bb[(s, p)]["ms"], bb[(s, p)]["ms_min"]) if (s, p) in bb else "%14s" % "refused"
        L.append("%-18s %14s %14s %14s" % (s, cell("bf16"), cell("bf16x3"), cell("fp32")))
    L += ["", "far3d_dwconv3x3_nhwc alone (algorithmic bytes = input + output + weights; share of the %.0f TB/s HBM peak)" % (HBM / 1e12),
          "%-18s %-7s %-18s %2s %5s %9s %9s %8s %7s" % ("spec", "layer", "N x H x W x C", "s", "dtype", "us", "MB", "TB/s", "of peak")]
    for r in dw:
        L.append("%-18s %-7s %-18s %2d %5s %9.1f %9.1f %8.2f %6.0f%%" % (r["spec"], r["layer"], "x".join(map(str, r["shape"])), r["stride"], r["dt"],
                                                                         r["us"], r["bytes"] / 1e6, r["tbps"], 100 * r["tbps"] * 1e12 / HBM))
    L += ["", "share of the depthwise backbone's time spent in the depthwise launches (sum over the frame's launches of the stand-alone time; each",
          "writes its scratch map once and the pointwise GEMM reads it once -- the round trip a fused depthwise->pointwise kernel would remove)"]
    for s in SPECS:
        for p, dt in (("bf16", "bf16"), ("bf16x3", "pair"), ("fp32", "f32")):
            mine = [r for r in dw if r["spec"] == s and r["dt"] == dt]
            if mine and (s, p) in bb:
                tot = sum(r["us"] * r["count"] for r in mine) / 1e3
                scratch = sum(2 * r["out_bytes"] * r["count"] for r in mine) / 1e6
                L.append("%-18s %-7s depthwise launches %5.2f ms of %5.2f ms = %4.1f %%; scratch maps written + read %6.0f MB per frame" %
                         (s, p, tot, bb[(s, p)]["ms"], 100 * tot / bb[(s, p)]["ms"], scratch))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()

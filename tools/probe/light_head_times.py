"""Times of the light 2D head at the benchmark geometry (7 x 640 x 960: FPN maps 80x120 ... 10x15 x 256 channels, hipGraph replay).

  python tools/probe/light_head_times.py [--out profiles/light_head/times.txt] [--rounds 5]

Three things, recorded and not asserted:
  kernel   far3d_dwconv3x3_act_nhwc (bias + Swish, one and two weight sets) beside far3d_dwconv3x3_nhwc on the (7,80,120,256) map, bf16 and
           pair storage, in one process: microseconds and achieved bytes/s against the algorithmic bytes (input + output + weights).
  merge    ONE two-set launch against TWO single-set launches on that map, five alternating repetitions, so that the run-to-run spread of
           either side is known.  The engine's roi_dw_merged default follows this: the two-set launch stays only if it is faster by more
           than that spread.
  roi      engine.roi_head in bf16 and bf16x3 for dense towers + depth on p3, depthwise towers + depth on p3, depthwise towers + depth on p4.

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

N, C = 7, 256
HW = ((80, 120), (40, 60), (20, 30), (10, 15))
STEP_LIMIT = 240      # seconds per child
REPS = 5


def _map(dt, hw=HW[0]):
    import torch
    from far3d_amd import ops
    x = torch.randn(N, hw[0], hw[1], C, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    return ops.pair_from_float(x) if dt == "pair" else x.to(torch.bfloat16)


def _sets():
    import torch
    g = torch.Generator().manual_seed(2)
    w = (torch.randn(2, 9, C, generator=g) / 3).to("cuda:0")
    b = (torch.randn(2, C, generator=g) / 4).to("cuda:0")
    return w, b


def step_kernel(rounds):
    import torch
    from far3d_amd import ops
    w, b = _sets()
    for dt in ("bf16", "pair"):
        xs, pair = _map(dt), dt == "pair"
        nb = lambda *ts: sum(t.numel() * t.element_size() for t in ts)
        out1 = torch.empty_like(xs)
        out2 = torch.empty(xs.shape[:3] + (2 * xs.shape[3],), dtype=xs.dtype, device=xs.device)
        w0, w1, b0, b1 = w[:1].contiguous(), w[1:].contiguous(), b[:1].contiguous(), b[1:].contiguous()
        rows = [("dwconv3x3_nhwc", lambda: ops.dwconv3x3_nhwc(xs, w[0], 1, out=out1, pair=pair), nb(xs, out1, w[0])),
                ("act reps=1 bias swish", lambda: ops.dwconv3x3_act_nhwc(xs, w0, 1, bias=b0, act="swish", out=out1, pair=pair), nb(xs, out1, w0, b0)),
                ("act reps=2 bias swish", lambda: ops.dwconv3x3_act_nhwc(xs, w, 1, bias=b, act="swish", out=out2, pair=pair), nb(xs, out2, w, b))]
        for name, fn, nbytes in rows:
            med, mn = graph_us(fn, 10, rounds)
            print(json.dumps(dict(kind="kernel", dt=dt, name=name, us=med, us_min=mn, bytes=nbytes, tbps=nbytes / (med * 1e-6) / 1e12)), flush=True)
        o_a, o_b = torch.empty_like(xs), torch.empty_like(xs)

        def two():
            ops.dwconv3x3_act_nhwc(xs, w0, 1, bias=b0, act="swish", out=o_a, pair=pair)
            ops.dwconv3x3_act_nhwc(xs, w1, 1, bias=b1, act="swish", out=o_b, pair=pair)
        for rep in range(REPS):                       # alternating: merged, split, merged, split, ...
            m, _ = graph_us(rows[2][1], 10, rounds)
            s, _ = graph_us(two, 10, rounds)
            print(json.dumps(dict(kind="merge", dt=dt, rep=rep, merged_us=m, split_us=s)), flush=True)


def step_roi(precision, rounds):
    import torch
    from far3d_amd import engine, weights
    for name, dw, level in (("dense towers, depth on p3", False, 0), ("depthwise towers, depth on p3", True, 0),
                            ("depthwise towers, depth on p4", True, 1)):
        spec = {k: v for k, v in weights.detector_spec(roi_depthwise=dw).items() if k.startswith("img_roi_head.")}
        eng = engine.Far3DEngine(weights.init_state_dict(spec, seed=1), engine.default_cfg(roi_depthwise=dw, depth_level=level), device="cuda:0",
                                 precision=precision, parts=("roi",))
        g = torch.Generator().manual_seed(3)
        raw = [eng.act_from_nchw(torch.randn(N, C, h, w, generator=g).to("cuda:0")) for h, w in HW]
        variants = [(None, name)] if not dw else [(True, name + ", one two-set launch"), (False, name + ", two single-set launches")]
        for merged, label in variants:
            if merged is not None:
                eng.roi_dw_merged = merged
            med, mn = graph_us(lambda: eng.roi_head(raw), 2, rounds)
            print(json.dumps(dict(kind="roi", precision=precision, name=label, ms=med / 1e3, ms_min=mn / 1e3)), flush=True)
        del eng, raw
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_head", "times.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", default=None, help="internal: run one step in this process")
    a = ap.parse_args()
    if a.step:
        kind, _, arg = a.step.partition(":")
        return step_kernel(a.rounds) if kind == "kernel" else step_roi(arg, a.rounds)
    rows = []
    for step in ("kernel", "roi:bf16", "roi:bf16x3"):
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
    L = ["Light 2D head at %d x 640 x 960 (FPN maps %s x %d channels), hipGraph replay, median (min) of the rounds" %
         (N, ", ".join("%dx%d" % hw for hw in HW), C), "",
         "depthwise kernels on the (%d,%d,%d,%d) map (algorithmic bytes = input + output + weights + bias)" % ((N,) + HW[0] + (C,)),
         "%-5s %-24s %9s %9s %8s" % ("dtype", "call", "us", "MB", "TB/s")]
    for r in rows:
        if r["kind"] == "kernel":
            L.append("%-5s %-24s %9.1f %9.1f %8.2f" % (r["dt"], r["name"], r["us"], r["bytes"] / 1e6, r["tbps"]))
    L += ["", "one two-set launch against two single-set launches, %d alternating repetitions (us)" % REPS,
          "%-5s %3s %10s %10s" % ("dtype", "rep", "two-set", "2 x single")]
    for dt in ("bf16", "pair"):
        mine = [r for r in rows if r["kind"] == "merge" and r["dt"] == dt]
        if not mine:
            continue
        for r in mine:
            L.append("%-5s %3d %10.1f %10.1f" % (dt, r["rep"], r["merged_us"], r["split_us"]))
        m, s = [r["merged_us"] for r in mine], [r["split_us"] for r in mine]
        spread = max(max(m) - min(m), max(s) - min(s))
        gain = sum(s) / len(s) - sum(m) / len(m)
        L.append("%-5s mean two-set %.1f, mean 2 x single %.1f: gain %.1f us against a run-to-run spread of %.1f us -> %s" %
                 (dt, sum(m) / len(m), sum(s) / len(s), gain, spread, "two-set launch is faster" if gain > spread else "not faster by more than the spread"))
    L += ["", "engine.roi_head", "%-7s %-58s %16s" % ("mode", "head", "ms")]
    for r in rows:
        if r["kind"] == "roi":
            L.append("%-7s %-58s %7.3f (%6.3f)" % (r["precision"], r["name"], r["ms"], r["ms_min"]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()

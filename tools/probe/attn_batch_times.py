"""Times of the batched, masked attention kernel (far3d_attention_batched) next to the one-sample kernel (far3d_attention_forward) at
the decoder's size: Aq = 1544 queries x Nk = 2312 keys x 8 heads of 32, fp32 and bf16, hipGraph replay.

  python tools/probe/attn_batch_times.py [--out profiles/attn_batch/times.txt] [--rounds 5]

Recorded, not asserted.  Per dtype, REPS repetitions in ONE process with the arms alternating inside a repetition, so that the spread
of every figure is known: microseconds per arm, the median of `rounds` timed windows.  A window is as many replays of one hipGraph as
fill `--window` seconds of device time (the count comes from a first timed run of 10 replays), between two device events; a graph
holds 8 repetitions of its arm, so the host's replay call is not what is timed.  Arms: the old kernel once (`old_B1`); the new kernel
at B = 1 without a mask; B = 2 and B = 4 in one launch against that many launches of the old kernel; at B = 2 a bool (Aq, Nk) mask
(p = 0.3), a bool (B * heads, Aq, Nk) mask and an f32 additive mask.  Operands are random (randn, q * 2) and every output is
preallocated.  Before timing, each arm's result is compared with the old kernel's / the float64 restatement on one head block."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

REPS = 3
PER_GRAPH = 8


def graph_us(fn, rounds, window_s):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(PER_GRAPH):
            fn()

    def window(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3

    window(3)
    replays = max(3, int(window_s / (window(10) / 10)) + 1)
    ts = sorted(window(replays) * 1e6 / (replays * PER_GRAPH) for _ in range(rounds))
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.1, help="seconds of device time per timed window")
    args = ap.parse_args()
    import torch
    from far3d_amd import lib, ops
    from tests import attn_refs
    lib.require_device()
    dev = "cuda:0"
    Aq, Nk, H, E, BMAX = 1544, 2312, 8, 256, 4
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    emit(dict(kind="geometry", Aq=Aq, Nk=Nk, heads=H, head_dim=E // H, device=torch.cuda.get_device_name(0)))
    g = torch.Generator().manual_seed(0)
    q32, k32, v32 = (torch.randn(BMAX, n, E, generator=g) for n in (Aq, Nk, Nk))
    q32 = q32 * 2.0
    m2 = (torch.rand(Aq, Nk, generator=g) < 0.3).to(dev)
    m3 = (torch.rand(2 * H, Aq, Nk, generator=g) < 0.3).to(dev)
    mf = (torch.rand(Aq, Nk, generator=g) * 8 - 4).masked_fill(torch.rand(Aq, Nk, generator=g) < 0.2, float("-inf")).to(dev)
    for dt in (torch.float32, torch.bfloat16):
        q, k, v = (t.to(dt).to(dev) for t in (q32, k32, v32))
        out = torch.empty(BMAX, Aq, E, device=dev)
        old = lambda B: [ops.attention_forward(q[b], k[b], v[b], num_heads=H, out=out[b]) for b in range(B)]
        new = lambda B, **kw: ops.attention_batched(q[:B], k[:B], v[:B], H, out=out[:B], **kw)
        arms = [("old_B1", lambda: old(1)), ("new_B1", lambda: new(1)), ("old_x2", lambda: old(2)), ("new_B2", lambda: new(2)),
                ("old_x4", lambda: old(4)), ("new_B4", lambda: new(4)), ("new_B2_bool2d", lambda: new(2, attn_mask=m2)),
                ("new_B2_bool3d", lambda: new(2, attn_mask=m3)), ("new_B2_f32mask", lambda: new(2, attn_mask=mf))]
        # agreement first: new vs old without a mask (full tensor), masked arms vs float64 on the first 64 queries of sample 0
        old(2)
        ref = out[:2].clone()
        d_nomask = (new(2) - ref).abs().max().item()
        errs = {}
        for name, m in (("bool2d", m2), ("bool3d", m3), ("f32mask", mf)):
            got = new(2, attn_mask=m)[:1, :64].cpu().double()
            mm = m.cpu()
            mm = mm[:64] if mm.dim() == 2 else mm[:H, :64]
            want = attn_refs.attention_ref(q[:1, :64].cpu(), k[:1].cpu(), v[:1].cpu(), H, mm)
            errs[name] = (got - want).abs().max().item()
        emit(dict(kind="agreement", dtype=str(dt), new_vs_old_max=d_nomask, masked_vs_float64_max=errs))
        for rep in range(REPS):
            row = dict(kind="times_us", dtype=str(dt), rep=rep)
            for name, fn in arms:
                row[name] = round(graph_us(fn, args.rounds, args.window), 2)
            emit(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

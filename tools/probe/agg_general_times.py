"""Times of the general aggregation path (far3d_agg_operands -> far3d_msda_forward -> far3d_camera_sum, ops.aggregate_general) next to
the fused launch (far3d_aggregate_forward) at the benchmark geometry: 7 cameras, 640 x 960, A = 1544, P = 13, G = 8, L = 4, on f32 and
bf16 value maps, hipGraph replay.

  python tools/probe/agg_general_times.py [--out profiles/agg_general/times.txt] [--rounds 5]

Recorded, not asserted.  Per value dtype, five repetitions in ONE process, the launches alternating inside a repetition (operands, MSDA,
camera sum, the three together, fused), so that the run-to-run spread of every figure is known: microseconds per launch, the median of
`rounds` timed windows, and the operand bytes written.  A window is as many replays of one hipGraph as fill `--window` seconds of
device time (0.25 s; the count comes from a first timed run of 10 replays), between two device events.  A graph holds LAUNCHES[key]
launches, 8 to 64, so that one replay is 0.16 - 1.5 ms of device work and the host's replay call is not what is timed.
Before timing, the two paths are compared on the same inputs (max |general - fused|).  The fused launch is timed with its camera tables
precomputed (far3d_agg_tables is per frame, not per layer) and without a workgroup order, as ops.aggregate_forward runs it for a
stand-alone call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

REPS = 5
LAUNCHES = dict(operands=8, msda=16, camera_sum=64, general=8, fused=32)     # per graph; every launch allocates its outputs


def graph_us(fn, iters, rounds, window_s):
    """Microseconds per call of fn: `iters` calls captured in one hipGraph, `rounds` windows of enough replays to last window_s each.
    -> (median, replays per window)."""
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()

    def window(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3      # seconds

    window(3)
    replays = max(3, int(window_s / (window(10) / 10)) + 1)
    ts = sorted(window(replays) * 1e6 / (replays * iters) for _ in range(rounds))
    return ts[len(ts) // 2], replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timed window")
    args = ap.parse_args()
    import torch
    from far3d_amd import lib, ops
    from tests import cases
    lib.require_device()
    dev = "cuda:0"
    c = cases.config2_aggregate_case(seed=0)
    N, S, C = c["feat"].shape
    A, P, G, L = c["ref"].shape[0], c["offsets"].shape[1], c["G"], len(c["level_hw"])
    d = lambda t: t.to(dev).contiguous()
    ref, offs, l2i, U, Vc = d(c["ref"]), d(c["offsets"]).reshape(A, -1), d(c["lidar2img"]), d(c["U"]), d(c["Vc"])
    shapes = torch.tensor([list(x) for x in c["level_hw"]], dtype=torch.int64, device=dev)
    starts = torch.tensor(c["level_start"], dtype=torch.int64, device=dev)
    tables = ops.agg_tables(Vc)
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    emit(dict(kind="geometry", cams=N, image=list(c["pad_hw"]), S=S, C=C, A=A, P=P, G=G, L=L,
              operand_bytes=4 * N * A * L * P * G * 3, per_camera_output_bytes=4 * N * A * C))
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        feat = d(c["feat"].to(dt))
        value = feat.view(N, S, G, C // G)
        st = {}

        def operands():
            st["loc"], st["w"] = ops.agg_operands(ref, offs, l2i, U, Vc, L, G, c["pc_range"], c["pad_hw"])

        def msda():
            st["per_cam"] = ops.msda_forward(value, shapes, starts, st["loc"], st["w"], im2col_step=N)

        def cam_sum():
            st["out"] = ops.camera_sum(st["per_cam"], N)

        def general():
            operands(), msda(), cam_sum()

        def fused():
            st["fused"] = ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, c["level_hw"], c["level_start"], c["pc_range"], c["pad_hw"],
                                                num_groups=G, tables=tables)

        general(), fused()
        torch.cuda.synchronize()
        emit(dict(kind="agreement", values=name, max_abs_general_minus_fused=(st["out"][0] - st["fused"]).abs().max().item(),
                  max_abs_fused=st["fused"].abs().max().item()))
        for rep in range(REPS):
            row = dict(kind="times_us", values=name, rep=rep, replays={})
            for key, fn in (("operands", operands), ("msda", msda), ("camera_sum", cam_sum), ("general", general), ("fused", fused)):
                general()                       # the inputs of the timed launch are eager tensors, not a finished graph's pool
                torch.cuda.synchronize()
                us, row["replays"][key] = graph_us(fn, LAUNCHES[key], args.rounds, args.window)
                row[key] = round(us, 2)
            emit(row)
        del feat, value, st
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

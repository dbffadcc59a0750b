"""Times of the batched fused aggregation (far3d_aggregate_batched, ops.aggregate_batched) next to its two yardsticks -- B one-sample
far3d_aggregate_forward launches, and the general path the module ran for a batch before (ops.aggregate_general: far3d_agg_operands ->
far3d_msda_forward -> far3d_camera_sum) -- at the benchmark geometry: 7 cameras, 640 x 960, A = 1544, P = 13, G = 8, L = 4, on f32
and bf16 value maps, B = 1, 2, 4 samples, hipGraph replay.

  python tools/probe/agg_batched_times.py [--out profiles/agg_batched/times.txt] [--rounds 5]

Recorded, not asserted.  The windows are tools/probe/agg_general_times.py's: per (value dtype, B), five repetitions in ONE process, the
three launches alternating inside a repetition, so that the run-to-run spread of every figure is known; microseconds per call, the
median of `rounds` timed windows; a window is as many replays of one hipGraph as fill `--window` seconds of device time, between two
device events; a graph holds LAUNCHES[key] calls.  Every sample has its own maps, queries and (rolled) cameras.  The camera tables are
precomputed for all three (far3d_agg_tables is per frame, not per layer), and no workgroup order is used, as for a stand-alone call.
Before timing, the batched launch is compared with the B one-sample launches (bitwise) and with the general path (max abs)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from agg_general_times import graph_us      # noqa: E402  (the same windows)

REPS = 5
BATCHES = (1, 2, 4)
LAUNCHES = dict(batched=16, singles=16, general=4)     # calls per graph; every call allocates its outputs


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
    cs = [cases.config2_aggregate_case(seed=b) for b in range(max(BATCHES))]
    for b, c in enumerate(cs):
        c["lidar2img"] = torch.roll(c["lidar2img"], b, 0)
    c0 = cs[0]
    N, S, C = c0["feat"].shape
    A, P, G, L = c0["ref"].shape[0], c0["offsets"].shape[1], c0["G"], len(c0["level_hw"])
    geom = (c0["level_hw"], c0["level_start"], c0["pc_range"], c0["pad_hw"])
    shapes = torch.tensor([list(x) for x in c0["level_hw"]], dtype=torch.int64, device=dev)      # device tensors: no copy inside a capture
    starts = torch.tensor(c0["level_start"], dtype=torch.int64, device=dev)
    st = lambda k, B: torch.stack([c[k] for c in cs[:B]]).to(dev).contiguous()
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    emit(dict(kind="geometry", cams=N, image=list(c0["pad_hw"]), S=S, C=C, A=A, P=P, G=G, L=L, batches=list(BATCHES),
              general_operand_bytes_per_sample=4 * N * A * L * P * G * 3))
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        feat_all = torch.stack([c["feat"].to(dt) for c in cs]).to(dev).contiguous()
        for B in BATCHES:
            feat = feat_all[:B]
            ref, offs, l2i, U, Vc = st("ref", B), st("offsets", B).reshape(B, A, -1), st("lidar2img", B), st("U", B), st("Vc", B)
            tables = ops.agg_tables(Vc)
            res = {}

            def batched():
                res["batched"] = ops.aggregate_batched(feat, ref, offs, l2i, U, Vc, *geom, num_groups=G, tables=tables)

            def singles():
                res["singles"] = [ops.aggregate_forward(feat[b], ref[b], offs[b], l2i[b], U[b], Vc[b], *geom, num_groups=G,
                                                        tables=tables[b]) for b in range(B)]

            def general():
                res["general"] = ops.aggregate_general(feat.view(B * N, S, C), ref, offs, l2i, U, Vc, shapes, starts,
                                                       c0["pc_range"], c0["pad_hw"], G)

            batched(), singles(), general()
            torch.cuda.synchronize()
            emit(dict(kind="agreement", values=name, B=B,
                      batched_equals_singles_bitwise=all(torch.equal(res["batched"][b], res["singles"][b]) for b in range(B)),
                      max_abs_general_minus_batched=(res["general"] - res["batched"]).abs().max().item(),
                      max_abs_batched=res["batched"].abs().max().item()))
            for rep in range(REPS):
                row = dict(kind="times_us", values=name, B=B, rep=rep, replays={})
                for key, fn in (("batched", batched), ("singles", singles), ("general", general)):
                    torch.cuda.synchronize()
                    us, row["replays"][key] = graph_us(fn, LAUNCHES[key], args.rounds, args.window)
                    row[key] = round(us, 2)
                emit(row)
            del res, feat, ref, offs, l2i, U, Vc, tables
            torch.cuda.empty_cache()
        del feat_all
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

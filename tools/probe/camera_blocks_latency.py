"""The reference's timing protocol (a device sync before and after every frame) at the benchmark geometry (7 x 640 x 960, V-99-eSE,
hipGraph replay) in a proposal mode bench.py's own --latency-groups block does not cover: the plain engine against
latency.CameraGroupFrame with the fixed-capacity threshold rule and / or multi-depth proposals, ALTERNATING on the same device in one
process.  Recorded, not asserted (profiles/camera_blocks/README.md).

  python tools/probe/camera_blocks_latency.py [--capacity 1024 | --topk 92] [--multi-depth K] [--groups 2] [--rounds 4] [--frames 25]
  python tools/probe/camera_blocks_latency.py --only groups --rounds 1 --frames 20      # a short run to put under a kernel trace

Prints one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16x3")
    ap.add_argument("--capacity", type=int, default=1024, help="fixed-capacity threshold mode: rows of the adaptive queries")
    ap.add_argument("--topk", type=int, default=None, help="static top-K mode instead (needs --multi-depth > 1 to take the merged path)")
    ap.add_argument("--multi-depth", type=int, default=1)
    ap.add_argument("--groups", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--only", default="both", choices=["both", "plain", "groups"])
    args = ap.parse_args()
    import torch
    from far3d_amd import engine, synth, weights
    from far3d_amd.latency import CameraGroupFrame
    dev = "cuda:0"
    over = dict(proposal_topk=args.topk) if args.topk else dict(proposal_topk=None, proposal_capacity=args.capacity)
    if args.multi_depth > 1:
        over["multi_depth"] = dict(topk=args.multi_depth, range_min=30)
    cfg = engine.default_cfg(**over)
    sd = weights.init_state_dict(weights.detector_spec(cfg["backbone"]), seed=0)
    frames = [synth.make_frame(7, (640, 960), seed=0, frame_index=fi, device=dev, ego_motion=True) for fi in range(4)]
    runners = {}
    for name in ("plain", "groups"):
        if args.only not in ("both", name):
            continue
        eng = engine.Far3DEngine(sd, cfg, device=dev, precision=args.precision)      # an engine each: own buffers, memory queue, graphs
        eng.pipeline, eng.tile_table, eng.use_graph = False, "tuning_mi355x.json", True
        runners[name] = (eng, eng if name == "plain" else CameraGroupFrame(eng, groups=args.groups))
    step = 0
    for name, (eng, run) in runners.items():                                         # scene start, captures, two replays
        for fi in range(4):
            out = run.forward_frame(*frames[fi])
        torch.cuda.synchronize()
        flag = out.get("proposal_overflow")
        runners[name] += (dict(adaptive_queries=int(out["num_adaptive_dev"].item()) if out.get("num_adaptive_dev") is not None else out["num_adaptive"],
                               overflow=int(flag.item()) if flag is not None else 0),)
    ms = {name: [] for name in runners}
    for _ in range(args.rounds):
        for name, (eng, run, _) in runners.items():
            for _ in range(args.frames):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run.forward_frame(*frames[step % len(frames)])
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
                step += 1
    res = dict(precision=args.precision, mode=over, groups=args.groups, rounds=args.rounds,
               frames_per_round=args.frames, protocol="sync before and after every frame; runners alternate round by round")
    for name, v in ms.items():
        per_round = [sum(v[i:i + args.frames]) / args.frames for i in range(0, len(v), args.frames)]
        s = sorted(v)
        res[name] = dict(mean_ms=sum(v) / len(v), p50_ms=s[len(s) // 2], min_ms=s[0], round_means_ms=[round(x, 4) for x in per_round],
                         last_warm_frame=runners[name][2])
    print(json.dumps(res))


if __name__ == "__main__":
    main()

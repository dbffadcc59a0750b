"""Whole-frame times of far3d_amd/streams.py StreamBatch at the benchmark geometry (7 cameras of 640 x 960, V-99, 92 proposals per
camera: A = 1544 queries), B = 1, 2, 4 scene streams, bf16 and bf16x3: one forward_frames call with the shared camera pass and the
shared head launches (camera_batch, head_batch) against the same call with both off -- the per-stream camera stage and head around the
one decoder pass, which is what the runner was before it had the switches.

  python tools/probe/stream_frame_times.py [--out profiles/stream_batch/frame_times.txt] [--rounds 5] [--reps 5]
  python tools/probe/stream_frame_times.py --root <another checkout, built> --out ...     # e.g. the parent commit: its StreamBatch as it is

Recorded, not asserted -- except the bits: before timing, per (dtype, B), two calls of every variant on the same frames from a reset
memory must agree bitwise with the switches-off runner (outputs and memories), or the probe stops.  The windows are those of
tools/probe/stream_batch_times.py (agg_general_times.graph_us): per (dtype, B) `reps` repetitions in ONE process, the variants
alternating inside a repetition; a figure is the median of `rounds` timed windows in microseconds per call (one call = one frame of
every stream); a window is as many replays of one hipGraph as fill `--window` seconds of device time, between two device events; a
graph holds ONE forward_frames call in its steady state (same scene, frames resident on the device).  Replaying a graph leaves the
host's launch cost out: the figures are device time.  Weights: the benchmark's random initialisation; stream b's frames are
synth.make_frame(seed=b)."""
import argparse
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPS = 5
BATCHES = (1, 2, 4)
K_PROP = 92
KEYS = ("all_cls_scores", "all_bbox_preds", "memory_topk", "outs_dec", "feat_flatten", "bbox2d", "sel_idx")
RESULT = ("boxes_3d", "scores_3d", "labels_3d", "keep")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)), help="the checkout whose far3d_amd is timed (built)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timed window")
    ap.add_argument("--precisions", default="bf16,bf16x3")
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from agg_general_times import graph_us      # the same windows (the import puts this tree in front: --root goes in front of it)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from far3d_amd import engine, lib, streams, synth, weights
    lib.require_device()
    dev = "cuda:0"
    switches = "camera_batch" in inspect.signature(streams.StreamBatch.__init__).parameters
    variants = dict(on=dict(camera_batch=True, head_batch=True), off=dict(camera_batch=False, head_batch=False)) if switches else dict(asis={})
    batches = [int(b) for b in args.batches.split(",")]
    cfg = engine.default_cfg(proposal_topk=K_PROP)
    sd = weights.init_state_dict(weights.detector_spec(cfg["backbone"]), seed=0)
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    emit(dict(kind="geometry", root=os.path.abspath(args.root) == os.path.dirname(os.path.dirname(HERE)) and "this tree" or "other checkout",
              cams=7, image=[640, 960], proposal_topk=K_PROP, batches=batches, variants=sorted(variants), rounds=args.rounds, reps=args.reps))
    # per stream three consecutive frames of one scene (ego motion on), resident on the device
    frames = [[synth.make_frame(7, (640, 960), seed=b, frame_index=fi, device=dev, ego_motion=True) for fi in range(3)] for b in range(max(batches))]
    for b, fs in enumerate(frames):
        for _, metas in fs:
            metas[0]["scene_token"] = "stream-%d" % b
    for name in args.precisions.split(","):
        eng = engine.Far3DEngine(sd, cfg, device=dev, precision=name)
        eng.fused_rows, eng.use_graph, eng.pipeline = False, False, False
        for B in batches:
            call = lambda sb, fi: sb.forward_frames([frames[b][fi][0] for b in range(B)], [frames[b][fi][1] for b in range(B)])
            runners = {v: streams.StreamBatch(eng, streams=B, **kw) for v, kw in variants.items()}
            # ---- the bits: two frames from a reset memory, every variant against the switches-off runner
            snaps = {}
            for v, sb in runners.items():
                sb.reset_memory()
                snap = []
                for fi in (0, 1):
                    outs = call(sb, fi)
                    for b in range(B):
                        snap += [outs[b][k].clone() for k in KEYS] + [outs[b]["result"][k].clone() for k in RESULT]
                        snap += [t.clone() for t in outs[b]["fpn"]] + [sb.memory(b)[k].clone() for k in sorted(sb.memory(b))]
                snaps[v] = snap
            torch.cuda.synchronize()
            base = snaps["off" if switches else "asis"]
            agree = {v: len(s) == len(base) and all(torch.equal(x, y) for x, y in zip(s, base)) for v, s in snaps.items()}
            finite = all(bool(torch.isfinite(t.float()).all()) for t in base if t.is_floating_point())
            chunks = getattr(runners.get("on"), "camera_chunks", None)
            emit(dict(kind="agreement", dtype=name, B=B, bitwise_equal_to_switches_off=agree, outputs_finite=finite, camera_chunks=chunks,
                      tensors_compared=len(base)))
            del snaps, base
            if not all(agree.values()):
                raise SystemExit("stream_frame_times: the variants disagree bitwise at %s, B = %d: %s" % (name, B, agree))
            # ---- the times: frame 2 of the scene, replayed (the memory keeps evolving; the launches do not depend on its values)
            for rep in range(args.reps):
                row = dict(kind="times_us", dtype=name, B=B, rep=rep, replays={})
                for v, sb in runners.items():
                    torch.cuda.synchronize()
                    us, row["replays"][v] = graph_us(lambda: call(sb, 2), 1, args.rounds, args.window)
                    row[v] = round(us, 2)
                emit(row)
            del runners
            torch.cuda.empty_cache()
        del eng
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Whole-frame times of the engine at the benchmark geometry (7 cameras of 640 x 960, V-99, 92 proposals per camera: A = 1544
queries, 256 propagated = 256 top-k, 1024 memory slots) with track ids on (cfg track=dict(birth_thr=0.0): the tracked decode and one
far3d_track_update launch per frame) against off, bf16 and bf16x3.

  python tools/probe/track_times.py [--out profiles/track_ids/times.txt] [--rounds 5] [--reps 5]
  python tools/probe/track_times.py --root <another checkout, built> --out ...     # e.g. the parent commit: it has no tracking, `off` only

Recorded, not asserted -- except the bits: before timing, three frames from a reset memory must give the same logits, boxes, decoded
result and memory with tracking on as with it off, or the probe stops.  The windows are those of tools/probe/stream_frame_times.py
(agg_general_times.graph_us): `reps` repetitions in ONE process, the variants alternating inside a repetition; a figure is the median of
`rounds` timed windows in microseconds per frame; a window is as many replays of one hipGraph as fill `--window` seconds of device
time, between two device events and closed by a device synchronisation; a graph holds ONE forward_frame call in its steady state (same
scene, the frame resident on the device).  Replaying a graph leaves the host's launch cost out: the figures are device time.  The
summary row gives, per variant, the median over the repetitions and their spread (min, max).  Weights: the benchmark's random
initialisation; frames: synth.make_frame(seed=0)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPS = 5
K_PROP = 92
KEYS = ("all_cls_scores", "all_bbox_preds", "memory_topk", "outs_dec")
RESULT = ("boxes_3d", "scores_3d", "labels_3d", "keep")
MEM = ("emb", "ref", "ts", "pose", "velo")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)), help="the checkout whose far3d_amd is timed (built)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timed window")
    ap.add_argument("--precisions", default="bf16,bf16x3")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from agg_general_times import graph_us      # the same windows (the import puts this tree in front: --root goes in front of it)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from far3d_amd import engine, lib, synth, weights
    lib.require_device()
    dev = "cuda:0"
    tracking = "track" in engine.default_cfg()
    variants = dict(off=None, on=dict(birth_thr=0.0)) if tracking else dict(off=None)
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    this = os.path.abspath(args.root) == os.path.dirname(os.path.dirname(HERE))
    emit(dict(kind="geometry", root="this tree" if this else "other checkout", cams=7, image=[640, 960], proposal_topk=K_PROP,
              variants=sorted(variants), rounds=args.rounds, reps=args.reps))
    frames = [synth.make_frame(7, (640, 960), seed=0, frame_index=fi, device=dev, ego_motion=True) for fi in range(4)]
    for name in args.precisions.split(","):
        engines = {}
        for v, tr in variants.items():
            cfg = engine.default_cfg(proposal_topk=K_PROP, **(dict(track=tr) if tracking else {}))
            sd = weights.init_state_dict(weights.detector_spec(cfg["backbone"]), seed=0)
            engines[v] = engine.Far3DEngine(sd, cfg, device=dev, precision=name)
            engines[v].use_graph = engines[v].pipeline = False
        # ---- the bits: three frames from a reset memory
        snaps = {}
        for v, eng in engines.items():
            eng.reset_memory()
            snap = []
            for fi in range(3):
                o = eng.forward_frame(*frames[fi])
                snap += [o[k].clone() for k in KEYS] + [o["result"][k].clone() for k in RESULT] + [eng.mem[k].clone() for k in MEM]
            snaps[v] = snap
            if v == "on":
                ids = o["result"]["track_ids"]
                emit(dict(kind="ids", dtype=name, frame=2, boxes=int(ids.numel()), with_id=int((ids > 0).sum().item()),
                          next_id=int(eng._track_next.item())))
        torch.cuda.synchronize()
        agree = {v: all(torch.equal(x, y) for x, y in zip(s, snaps["off"])) for v, s in snaps.items()}
        emit(dict(kind="agreement", dtype=name, bitwise_equal_to_off=agree, tensors_compared=len(snaps["off"])))
        del snaps
        if not all(agree.values()):
            raise SystemExit("track_times: tracking on changes the untracked outputs at %s: %s" % (name, agree))
        # ---- the times: frame 3 of the scene, replayed (the memory keeps evolving; the launches do not depend on its values)
        per = {v: [] for v in engines}
        for rep in range(args.reps):
            row = dict(kind="times_us", dtype=name, rep=rep, replays={})
            for v, eng in engines.items():
                torch.cuda.synchronize()
                us, row["replays"][v] = graph_us(lambda: eng.forward_frame(*frames[3]), 1, args.rounds, args.window)
                row[v] = round(us, 2)
                per[v].append(us)
            emit(row)
        summ = dict(kind="summary_us", dtype=name)
        for v, ts in per.items():
            ts = sorted(ts)
            summ[v] = dict(median=round(ts[len(ts) // 2], 2), min=round(ts[0], 2), max=round(ts[-1], 2))
        if "on" in per:
            summ["on_minus_off"] = round(summ["on"]["median"] - summ["off"]["median"], 2)
        emit(summ)
        del engines
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

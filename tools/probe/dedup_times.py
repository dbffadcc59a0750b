"""What duplicate suppression costs (cfg dedup: one far3d_box_dedup launch per frame behind the decode).

  python tools/probe/dedup_times.py [--out profiles/dedup/times.txt] [--rounds 5] [--reps 3]

Two parts, one process, recorded, not asserted -- except the bits (below).
  1. The isolated launch at the engine's Kdec = 300 boxes for B = 1, 2, 4 streams, in both modes, on two scenes: `spread` (a grid of
     small boxes 17 m apart: every pair is rejected by the distance of its centres) and `clustered` (tests/dedup_refs.clustered_boxes:
     clusters of 1 - 5, about a third of the candidates suppressed): 20 launches captured in one hipGraph, microseconds per launch.
     far3d_track_records at the benchmark geometry (tools/probe/track_records_times.py) is timed beside it, alternating, as the
     yardstick: the neighbouring single-workgroup launch of the frame.
  2. Whole-frame times of the engine at the benchmark geometry (7 cameras of 640 x 960, V-99, 92 proposals per camera) with dedup
     off, with the default IoU rule and with a 2 m centre rule: one forward_frame call in its steady state, captured in one hipGraph.
     Before timing, three frames from a reset memory must give the same logits, boxes, decoded result and memory in all variants, or
     the probe stops.
The windows are those of tools/probe/track_times.py (agg_general_times.graph_us): `reps` repetitions with the variants alternating
inside a repetition; a figure is the median of `rounds` timed windows; a window is as many replays as fill `--window` seconds of device
time, between two device events and closed by a device synchronisation.  Replaying a graph leaves the host's launch cost out: the
figures are device time.  The summary rows give, per variant, the median over the repetitions and their spread (min, max)."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
K_PROP = 92
KDEC = 300
KEYS = ("all_cls_scores", "all_bbox_preds", "memory_topk", "outs_dec")
RESULT = ("boxes_3d", "scores_3d", "labels_3d", "keep")
MEM = ("emb", "ref", "ts", "pose", "velo")


def scenes(torch, np, B, dev):
    """-> {scene: dict(boxes (B, 300, 7), scores, labels, keep) on the device}."""
    from tests import dedup_refs as dr
    g = np.arange(KDEC)
    spread = np.zeros((KDEC, 7), dtype=np.float32)
    spread[:, 0], spread[:, 1] = (g % 18 - 8.5) * 17.0, (g // 18 - 8.0) * 17.0
    spread[:, 3:6], spread[:, 6] = [4.5, 1.9, 1.6], np.linspace(-3.0, 3.0, KDEC)
    flat = dict(boxes=spread, scores=np.linspace(0.9, 0.1, KDEC).astype(np.float32), labels=(g % 4).astype(np.int64), keep=np.ones(KDEC, dtype=bool))
    out = {}
    for name, cases in (("spread", [flat] * B), ("clustered", [dr.clustered_boxes(np.random.default_rng(300 + b), KDEC) for b in range(B)])):
        out[name] = {k: torch.tensor(np.stack([c[k] for c in cases])).to(dev) for k in ("boxes", "scores", "labels", "keep")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timed window")
    ap.add_argument("--precisions", default="bf16")
    ap.add_argument("--skip-frames", action="store_true", help="part 1 only")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from agg_general_times import graph_us
    from track_records_times import GEOM, launch_operands, summary
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import numpy as np
    import torch
    from far3d_amd import engine, lib, ops, synth, weights
    lib.require_device()
    dev = "cuda:0"
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    emit(dict(kind="geometry", Kdec=KDEC, yardstick=GEOM, cams=7, image=[640, 960], proposal_topk=K_PROP, rounds=args.rounds, reps=args.reps))
    # ---- 1. the isolated launch
    row0 = GEOM["A"] - GEOM["P"]
    for B in (1, 2, 4):
        t = launch_operands(torch, B, dev)
        ids = ops.track_update(t["idx"], t["score"], t["track"], t["next"], row0, GEOM["P"], 0.0, query_idx=t["query"])
        fns = dict(track_records=lambda: ops.track_records(t["idx"], t["track"], t["hits"], t["query"], ids, t["keep"], t["boxes"], t["m_ref"],
                                                           t["m_ts"], GEOM["A"], row0, GEOM["P"]))
        for scene, s in scenes(torch, np, B, dev).items():
            for mode, thr in (("iou_bev", 0.5), ("centre", 1.0)):
                dk, of = ops.box_dedup(s["boxes"], s["scores"], s["labels"], s["keep"], mode=mode, thr=thr)
                emit(dict(kind="scene", B=B, scene=scene, mode=mode, candidates=int(s["keep"].sum().item()), suppressed=int((of >= 0).sum().item())))
                fns["%s_%s" % (scene, mode)] = (lambda s=s, mode=mode, thr=thr: ops.box_dedup(s["boxes"], s["scores"], s["labels"], s["keep"], mode=mode, thr=thr))
        per = {v: [] for v in fns}
        for rep in range(args.reps):
            for v, fn in fns.items():
                torch.cuda.synchronize()
                us, _ = graph_us(fn, 20, args.rounds, args.window)
                per[v].append(us)
        emit(dict(kind="launch_us", B=B, launches_per_graph=20, **summary(per)))
    # ---- 2. the frame
    if not args.skip_frames:
        variants = dict(off=None, iou_bev=dict(), centre=dict(mode="centre", thr=2.0))
        frames = [synth.make_frame(7, (640, 960), seed=0, frame_index=fi, device=dev, ego_motion=True) for fi in range(4)]
        for name in args.precisions.split(","):
            engines = {}
            for v, dd in variants.items():
                cfg = engine.default_cfg(proposal_topk=K_PROP, dedup=dd)
                sd = weights.init_state_dict(weights.detector_spec(cfg["backbone"]), seed=0)
                engines[v] = engine.Far3DEngine(sd, cfg, device=dev, precision=name)
                engines[v].use_graph = engines[v].pipeline = False
            snaps = {}
            for v, eng in engines.items():
                eng.reset_memory()
                snap = []
                for fi in range(3):
                    o = eng.forward_frame(*frames[fi])
                    snap += [o[k].clone() for k in KEYS] + [o["result"][k].clone() for k in RESULT] + [eng.mem[k].clone() for k in MEM]
                snaps[v] = snap
                r = o["result"]
                if v == "off":
                    assert "dup_keep" not in r
                else:
                    emit(dict(kind="dedup", dtype=name, variant=v, frame=2, boxes=int(r["keep"].numel()), kept=int(r["keep"].sum().item()),
                              survivors=int(r["dup_keep"].sum().item()), suppressed=int((r["dup_of"] >= 0).sum().item())))
            torch.cuda.synchronize()
            agree = {v: all(torch.equal(x, y) for x, y in zip(s, snaps["off"])) for v, s in snaps.items()}
            emit(dict(kind="agreement", dtype=name, bitwise_equal_to_off=agree, tensors_compared=len(snaps["off"])))
            del snaps
            if not all(agree.values()):
                raise SystemExit("dedup_times: a variant changes the outputs of another at %s: %s" % (name, agree))
            per = {v: [] for v in engines}
            for rep in range(args.reps):
                row = dict(kind="times_us", dtype=name, rep=rep)
                for v, eng in engines.items():
                    torch.cuda.synchronize()
                    us, _ = graph_us(lambda: eng.forward_frame(*frames[3]), 1, args.rounds, args.window)
                    row[v] = round(us, 2)
                    per[v].append(us)
                emit(row)
            summ = dict(kind="summary_us", dtype=name, **summary(per))
            summ["iou_bev_minus_off"] = round(summ["iou_bev"]["median"] - summ["off"]["median"], 2)
            summ["centre_minus_off"] = round(summ["centre"]["median"] - summ["off"]["median"], 2)
            emit(summ)
            del engines
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

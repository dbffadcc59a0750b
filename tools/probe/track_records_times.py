"""What the track records cost (cfg track=dict(records=True): one far3d_track_records launch per frame behind far3d_track_update).

  python tools/probe/track_records_times.py [--out profiles/track_records/times.txt] [--rounds 5] [--reps 5]

Two parts, one process, recorded, not asserted -- except the bits (below).
  1. The isolated launch at the benchmark geometry (K = 256 ranked rows, L = 1024 memory slots, Kdec = 300 boxes, A = 1544 query rows,
     P = 256) for B = 1, 2, 4 streams: 20 launches captured in one hipGraph, microseconds per launch.  far3d_track_update on the same
     operands is timed beside it, alternating, as the yardstick.
  2. Whole-frame times of the engine at the benchmark geometry (7 cameras of 640 x 960, V-99, 92 proposals per camera) with tracking
     off, with track ids only, and with ids + records: one forward_frame call in its steady state, captured in one hipGraph.  Before
     timing, three frames from a reset memory must give the same logits, boxes, decoded result and memory in all three variants, and the
     same ids with and without the records, or the probe stops.
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
KEYS = ("all_cls_scores", "all_bbox_preds", "memory_topk", "outs_dec")
RESULT = ("boxes_3d", "scores_3d", "labels_3d", "keep")
MEM = ("emb", "ref", "ts", "pose", "velo")
GEOM = dict(A=1544, K=256, L=1024, Kdec=300, P=256)


def summary(per):
    out = {}
    for v, ts in per.items():
        ts = sorted(ts)
        out[v] = dict(median=round(ts[len(ts) // 2], 2), min=round(ts[0], 2), max=round(ts[-1], 2))
    return out


def launch_operands(torch, B, dev):
    """B streams of random operands as a frame in flight has them: half of the slots hold an id, ranked rows distinct, boxes of ranked
    queries."""
    g = torch.Generator().manual_seed(B)
    A, K, L, Kdec = GEOM["A"], GEOM["K"], GEOM["L"], GEOM["Kdec"]
    idx = torch.stack([torch.randperm(A, generator=g)[:K] for _ in range(B)])
    track = torch.where(torch.rand((B, L), generator=g) < 0.5, torch.randint(1, 10 ** 6, (B, L), generator=g), torch.zeros((B, L), dtype=torch.int64))
    query = torch.gather(idx, 1, torch.randint(0, K, (B, Kdec), generator=g)).int()
    t = dict(idx=idx, score=torch.rand((B, A), generator=g), track=track, next=torch.full((B, 1), 10 ** 7), hits=(track != 0).int(), query=query,
             keep=torch.rand((B, Kdec), generator=g) < 0.5, boxes=torch.randn((B, Kdec, 7), generator=g),
             m_ref=torch.randn((B, L, 3), generator=g), m_ts=torch.full((B, L), 0.1, dtype=torch.float64))
    return {k: v.to(dev) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timed window")
    ap.add_argument("--precisions", default="bf16")
    ap.add_argument("--skip-frames", action="store_true", help="part 1 only")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    from agg_general_times import graph_us
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    from far3d_amd import engine, lib, ops, synth, weights
    lib.require_device()
    dev = "cuda:0"
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    emit(dict(kind="geometry", launch=GEOM, cams=7, image=[640, 960], proposal_topk=K_PROP, rounds=args.rounds, reps=args.reps))
    # ---- 1. the isolated launch
    row0 = GEOM["A"] - GEOM["P"]
    for B in (1, 2, 4):
        t = launch_operands(torch, B, dev)
        ids = ops.track_update(t["idx"], t["score"], t["track"], t["next"], row0, GEOM["P"], 0.0, query_idx=t["query"])
        fns = dict(track_update=lambda: ops.track_update(t["idx"], t["score"], t["track"], t["next"], row0, GEOM["P"], 0.0, query_idx=t["query"]),
                   track_records=lambda: ops.track_records(t["idx"], t["track"], t["hits"], t["query"], ids, t["keep"], t["boxes"], t["m_ref"],
                                                           t["m_ts"], GEOM["A"], row0, GEOM["P"]))
        per = {v: [] for v in fns}
        for rep in range(args.reps):
            for v, fn in fns.items():
                torch.cuda.synchronize()
                us, _ = graph_us(fn, 20, args.rounds, args.window)
                per[v].append(us)
        emit(dict(kind="launch_us", B=B, launches_per_graph=20, **summary(per)))
    # ---- 2. the frame
    if not args.skip_frames:
        variants = dict(off=None, ids=dict(birth_thr=0.0), records=dict(birth_thr=0.0, records=True))
        frames = [synth.make_frame(7, (640, 960), seed=0, frame_index=fi, device=dev, ego_motion=True) for fi in range(4)]
        for name in args.precisions.split(","):
            engines = {}
            for v, tr in variants.items():
                cfg = engine.default_cfg(proposal_topk=K_PROP, track=tr)
                sd = weights.init_state_dict(weights.detector_spec(cfg["backbone"]), seed=0)
                engines[v] = engine.Far3DEngine(sd, cfg, device=dev, precision=name)
                engines[v].use_graph = engines[v].pipeline = False
            snaps, idsnap = {}, {}
            for v, eng in engines.items():
                eng.reset_memory()
                snap, idsnap[v] = [], []
                for fi in range(3):
                    o = eng.forward_frame(*frames[fi])
                    snap += [o[k].clone() for k in KEYS] + [o["result"][k].clone() for k in RESULT] + [eng.mem[k].clone() for k in MEM]
                    if v != "off":
                        idsnap[v] += [o["result"]["track_ids"].clone(), eng.mem["track"].clone()]
                snaps[v] = snap
                if v == "records":
                    r = o["result"]
                    emit(dict(kind="records", dtype=name, frame=2, boxes=int(r["track_ids"].numel()), with_id=int((r["track_ids"] > 0).sum().item()),
                              primaries=int(r["track_primary"].sum().item()), max_age=int(r["track_age"].max().item()),
                              with_velocity=int(r["track_velocity"].ne(0).any(-1).sum().item())))
            torch.cuda.synchronize()
            agree = {v: all(torch.equal(x, y) for x, y in zip(s, snaps["off"])) for v, s in snaps.items()}
            agree["ids_of_records_equal_ids"] = all(torch.equal(x, y) for x, y in zip(idsnap["ids"], idsnap["records"]))
            emit(dict(kind="agreement", dtype=name, bitwise_equal_to_off=agree, tensors_compared=len(snaps["off"])))
            del snaps
            if not all(agree.values()):
                raise SystemExit("track_records_times: a variant changes the outputs of another at %s: %s" % (name, agree))
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
            summ["records_minus_ids"] = round(summ["records"]["median"] - summ["ids"]["median"], 2)
            summ["ids_minus_off"] = round(summ["ids"]["median"] - summ["off"]["median"], 2)
            emit(summ)
            del engines
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Times of the hole support of the batched aggregation and of StreamBatch(hole_rows=True), at the benchmark geometry (7 cameras of
640 x 960: S = 12750 tokens; A = 1544 queries = 644 learned + 644 adaptive rows + 256 propagated), B = 1, 2, 4:

  (a) the aggregation launch WITHOUT a hole: far3d_aggregate_batched_holes(hole_count = NULL) and far3d_aggregate_batched of this tree
      against far3d_aggregate_batched of another build of the library (--parent-lib: the parent commit's libfar3d_hip.so), which is
      timed TWICE per repetition so that the other build's own spread stands next to the difference;
  (b) the launch with a half-empty hole: rows [644, 1288), every sample's count 322;
  (c) a whole forward_frames call of StreamBatch(hole_rows=True) in the fixed-capacity threshold mode (proposal_topk=None,
      proposal_capacity=644) against B forward_frame calls of the plain engine in that mode (fused_rows off, as StreamBatch requires).

  python tools/probe/stream_holes_times.py [--out profiles/stream_holes/times.txt] [--parent-lib PATH] [--parts ab,c] [--rounds 5]

Recorded, not asserted -- except the bits: before timing, the launches without a hole must agree bitwise with each other (and with the
other build), the half-empty launch must hold zero rows in the hole and the same bits elsewhere, and every stream of forward_frames
must agree bitwise with the plain engine, or the probe stops.  The windows are tools/probe/stream_batch_times.py's
(agg_general_times.graph_us): per (dtype, B) five repetitions in ONE process, the calls alternating inside a repetition; microseconds
per call, the median of `rounds` timed windows; a window is as many replays of one hipGraph as fill `--window` seconds of device time;
a graph holds 16 aggregation launches or one frame of every stream."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from agg_general_times import graph_us      # noqa: E402  (the same windows)

REPS = 5
BATCHES = (1, 2, 4)
NQ, ROWS = 644, 644                  # learned queries; adaptive rows = the capacity: the hole is [NQ, NQ + ROWS)
KEYS = ("all_cls_scores", "all_bbox_preds", "memory_topk", "outs_dec", "bbox2d", "sel_idx", "sel_cnt", "num_adaptive_dev", "proposal_overflow")
RESULT = ("boxes_3d", "scores_3d", "labels_3d", "keep")


def aggregation(args, emit):
    import torch
    from far3d_amd import lib, ops
    from tests import cases
    dev = "cuda:0"
    mine = lib.load()
    other = None
    if args.parent_lib:
        other = ctypes.CDLL(os.path.abspath(args.parent_lib))
        other.far3d_aggregate_batched.restype, other.far3d_aggregate_batched.argtypes = lib.SIGNATURES["far3d_aggregate_batched"]
    cs = [cases.config2_aggregate_case(seed=b) for b in range(max(BATCHES))]
    for b, c in enumerate(cs):
        c["lidar2img"] = torch.roll(c["lidar2img"], b, 0)
    c0 = cs[0]
    N, S, C = c0["feat"].shape
    A, P, G, L = c0["ref"].shape[0], c0["offsets"].shape[1], c0["G"], len(c0["level_hw"])
    assert A >= NQ + ROWS
    emit(dict(kind="geometry", part="aggregation", cams=N, S=S, C=C, A=A, P=P, L=L, hole=[NQ, NQ + ROWS], half_empty_count=ROWS // 2,
              other_build=bool(other), launches_per_graph=16))
    hw_keep, hw_p = ops._host_i32([list(x) for x in c0["level_hw"]])
    st_keep, st_p = ops._host_i32(list(c0["level_start"]))
    pc_keep, pc_p = ops._host_f32(list(c0["pc_range"]))
    stack = lambda k, dt=None: torch.stack([c[k] if dt is None else c[k].to(dt) for c in cs]).to(dev).contiguous()
    for name, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        feat, ref, offs, l2i, U, Vc = stack("feat", dt), stack("ref"), stack("offsets"), stack("lidar2img"), stack("U"), stack("Vc")
        for B in BATCHES:
            tabs = ops.agg_tables(Vc[:B])
            out = {k: torch.empty((B, A, C), dtype=dt, device=dev) for k in ("other_1", "other_2", "batched", "holes_null", "holes_half")}
            half = torch.full((B,), ROWS // 2, dtype=torch.int32, device=dev)
            p = ops._ptr

            def call(fn, o, *hole):
                rc = fn(p(feat), ops._dt(feat), p(ref), p(offs), p(l2i), p(U), p(Vc), p(tabs), p(o), ops._dt(o), B, A, N, S, C, G, P, L, hw_p, st_p,
                        pc_p, float(c0["pad_hw"][0]), float(c0["pad_hw"][1]), 0, 0, *hole, ops._stream(feat))
                if rc != 0:
                    raise SystemExit("stream_holes_times: the library refused the call: %s" % mine.far3d_last_error().decode())

            calls = [("batched", lambda: call(mine.far3d_aggregate_batched, out["batched"])),
                     ("holes_null", lambda: call(mine.far3d_aggregate_batched_holes, out["holes_null"], None, 0, 0)),
                     ("holes_half", lambda: call(mine.far3d_aggregate_batched_holes, out["holes_half"], p(half), NQ, NQ + ROWS))]
            if other:
                calls = [("other_1", lambda: call(other.far3d_aggregate_batched, out["other_1"]))] + calls + \
                        [("other_2", lambda: call(other.far3d_aggregate_batched, out["other_2"]))]
            for _, fn in calls:
                fn()
            torch.cuda.synchronize()
            hole = torch.zeros(A, dtype=torch.bool, device=dev)
            hole[NQ + ROWS // 2:NQ + ROWS] = True
            agree = dict(holes_null_equals_batched=bool(torch.equal(out["holes_null"], out["batched"])),
                         other_build_equals_batched=bool(torch.equal(out["other_1"], out["batched"])) if other else None,
                         hole_rows_zero=bool((out["holes_half"][:, hole] == 0).all()),
                         other_rows_equal=bool(torch.equal(out["holes_half"][:, ~hole], out["batched"][:, ~hole])),
                         finite=bool(torch.isfinite(out["batched"].float()).all()))
            emit(dict(kind="agreement", part="aggregation", dtype=name, B=B, **agree))
            if not all(v for v in agree.values() if v is not None):
                raise SystemExit("stream_holes_times: the launches disagree at %s, B = %d: %s" % (name, B, agree))
            for rep in range(REPS):
                row = dict(kind="times_us", part="aggregation", dtype=name, B=B, rep=rep, replays={})
                for key, fn in calls:
                    torch.cuda.synchronize()
                    us, row["replays"][key] = graph_us(fn, 16, args.rounds, args.window)
                    row[key] = round(us, 3)
                emit(row)
            del out, tabs
        del feat, ref, offs, l2i, U, Vc
        torch.cuda.empty_cache()


def frames(args, emit):
    import torch
    from far3d_amd import engine, streams, synth, weights
    dev = "cuda:0"
    cfg = engine.default_cfg(proposal_topk=None, proposal_capacity=ROWS)
    sd = weights.init_state_dict(weights.detector_spec(cfg["backbone"]), seed=0)
    emit(dict(kind="geometry", part="frame", cams=7, image=[640, 960], proposal_topk=None, proposal_capacity=ROWS, batches=list(BATCHES)))
    fr = [[synth.make_frame(7, (640, 960), seed=b, frame_index=fi, device=dev, ego_motion=True) for fi in range(3)] for b in range(max(BATCHES))]
    for b, fs in enumerate(fr):
        for _, metas in fs:
            metas[0]["scene_token"] = "stream-%d" % b
    snap = lambda o, mem: [o[k].clone() for k in KEYS] + [o["result"][k].clone() for k in RESULT] + [mem[k].clone() for k in sorted(mem)]
    for name in args.precisions.split(","):
        eng = engine.Far3DEngine(sd, cfg, device=dev, precision=name)
        eng.fused_rows, eng.use_graph, eng.pipeline = False, False, False
        for B in BATCHES:
            sb = streams.StreamBatch(eng, streams=B, hole_rows=True)
            # ---- the bits: three frames from a reset memory, every stream against the plain engine
            want = []
            for b in range(B):
                eng.reset_memory()
                want.append([snap(eng.forward_frame(*fr[b][fi]), eng.mem) for fi in range(3)])
            got = [[] for _ in range(B)]
            for fi in range(3):
                outs = sb.forward_frames([fr[b][fi][0] for b in range(B)], [fr[b][fi][1] for b in range(B)])
                for b in range(B):
                    got[b].append(snap(outs[b], sb.memory(b)))
            counts = [int(outs[b]["num_adaptive_dev"].item()) for b in range(B)]
            flags = [int(outs[b]["proposal_overflow"].item()) for b in range(B)]
            agree = all(torch.equal(x, y) for b in range(B) for fi in range(3) for x, y in zip(got[b][fi], want[b][fi]))
            emit(dict(kind="agreement", part="frame", dtype=name, B=B, bitwise_equal_to_plain_engine=agree, rows_with_a_query=counts,
                      overflow_flags=flags, camera_chunks=sb.camera_chunks))
            del want, got
            if not agree:
                raise SystemExit("stream_holes_times: StreamBatch(hole_rows=True) differs from the plain engine at %s, B = %d" % (name, B))

            # the plain engine has ONE memory: its B calls carry one scene token, so that each is a steady frame like the streams' own
            same_scene = [(fr[b][2][0], [dict(fr[b][2][1][0], scene_token="plain")] + list(fr[b][2][1][1:])) for b in range(B)]

            def plain():
                for b in range(B):
                    eng.forward_frame(*same_scene[b])

            def batch():
                sb.forward_frames([fr[b][2][0] for b in range(B)], [fr[b][2][1] for b in range(B)])

            eng.reset_memory()
            plain()                                        # the scene's first frames: the timed calls are steady ones
            for rep in range(args.reps):
                row = dict(kind="times_us", part="frame", dtype=name, B=B, rep=rep, replays={})
                for key, fn in (("forward_frames", batch), ("B_forward_frame", plain)):
                    torch.cuda.synchronize()
                    us, row["replays"][key] = graph_us(fn, 1, args.rounds, args.window)
                    row[key] = round(us, 2)
                emit(row)
            del sb
            torch.cuda.empty_cache()
        del eng
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libfar3d_hip.so of another build (the parent commit's) for part (a)")
    ap.add_argument("--parts", default="ab,c")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=REPS)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timed window")
    ap.add_argument("--precisions", default="bf16", help="part (c): the engine precisions, comma separated")
    args = ap.parse_args()
    from far3d_amd import lib
    lib.require_device()
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    parts = args.parts.split(",")
    if "ab" in parts:
        aggregation(args, emit)
    if "c" in parts:
        frames(args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Digests of whole frames through the decoder and the heads, for comparing two checkouts bit for bit (a refactor of the host code that
issues the decoder's launches: Far3DEngine.decoder / decoder_streams / _head_finish / _head_finish_streams).

  python tools/probe/decoder_body_digest.py --out full.txt --summary profiles/decoder_body/digest_this_tree.txt
  python tools/probe/decoder_body_digest.py --root <another checkout, built> --out ... --summary ...     # e.g. the parent commit
  python tools/probe/decoder_body_digest.py --trace      # the short run a kernel trace is taken of: bf16 unfused, top-K, one frame

Only the API that both sides have: Far3DEngine.forward_frame, StreamBatch.forward_frames and the toy golden engine of
tests/test_engine_gpu.py (2 cameras, 64 x 96, 60 queries, 16 propagated, 64 memory slots).  Per configuration FRAMES calls (three frames
of one scene, then a scene change; stream 1 of a batch changes one call earlier), and per call and stream one line

  <sha256 of the raw bytes>  <configuration> <stream> <call> <tensor>

for all_cls_scores, all_bbox_preds, outs_dec, memory_topk, every tensor of `result` and every tensor of the streaming memory.
Configurations.  Plain engine: fp32, bf16 with fused_rows off and on, bf16x3 (fused_rows off), each in the proposal modes top-K
(proposal_topk=12) and tests/test_stream_holes_gpu.py's fixed-capacity threshold, threshold + multi-depth and top-K + multi-depth; bf16
top-K once more with use_graph on (row chains off and on).  StreamBatch, B = 2, on the unfused precisions in the same modes (hole_rows
where the mode leaves a hole), with camera_batch / head_batch both on and both off.  Two runs agree when their files are identical.
--summary FILE writes the short form that is kept in the repository: per configuration one line `<sha256 of its lines above>
<configuration> <number of lines>`, and a last line for the whole output."""
import argparse
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
MD = dict(topk=2, range_min=30)
MODES = {"topk": dict(proposal_topk=12),
         "capacity": dict(proposal_topk=None, proposal_capacity=48),
         "capacity_md": dict(proposal_topk=None, proposal_capacity=48, multi_depth=MD),
         "topk_md": dict(proposal_topk=12, multi_depth=MD)}
# per stream and call: (frame index inside the scene, scene)
FRAMES = [[(0, 0), (1, 0), (2, 0), (0, 1)],
          [(0, 0), (1, 0), (0, 1), (1, 1)]]
PLAIN = [("fp32", False), ("bf16", False), ("bf16", True), ("bf16x3", False)]        # (precision, fused_rows)
RESULT = ("boxes_3d", "scores_3d", "labels_3d", "keep")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None, help="write one digest per configuration, and one of the whole output, to this file")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(HERE)), help="the checkout whose far3d_amd runs (built)")
    ap.add_argument("--trace", action="store_true", help="bf16 unfused, top-K: the plain engine and StreamBatch B = 2, one frame each")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from far3d_amd import lib, synth
    from far3d_amd.streams import StreamBatch
    from tests.test_engine_gpu import _golden_engine
    lib.require_device()
    lines, engines = [], {}
    calls = 1 if args.trace else len(FRAMES[0])

    def engine(precision, mode):
        if (precision, mode) not in engines:
            engines[precision, mode] = _golden_engine(precision, **MODES[mode])
        eng, _, rc = engines[precision, mode]
        eng.reset_memory()
        eng.fused_rows, eng.use_graph, eng.pipeline, eng._graph = False, False, False, None
        return eng, rc

    def frame(rc, stream, call):
        fi, scene = FRAMES[stream][call]
        data, metas = synth.recipe_frame(dict(rc, data_seed=rc["data_seed"] + 1000 * stream, scene_change_at=0 if scene else None), fi)
        metas[0]["scene_token"] = "stream-%d-%s" % (stream, metas[0]["scene_token"])
        return data, metas

    def digest(config, stream, call, outs, mem):
        tensors = [(k, outs[k]) for k in ("all_cls_scores", "all_bbox_preds", "outs_dec", "memory_topk")]
        tensors += [("result." + k, outs["result"][k]) for k in RESULT] + [("memory." + k, mem[k]) for k in sorted(mem)]
        for name, t in tensors:
            raw = t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()
            lines.append("%s  %s %d %d %s" % (hashlib.sha256(raw).hexdigest(), config, stream, call, name))
            print(lines[-1], flush=True)

    def plain(precision, mode, fused, graph=False):
        eng, rc = engine(precision, mode)
        eng.fused_rows, eng.use_graph = fused, graph
        config = "plain/%s/%s/%s%s" % (precision, mode, "chains" if fused else "unfused", "/graph" if graph else "")
        for call in range(calls):
            outs = eng.forward_frame(*frame(rc, 0, call))
            eng.wait_outputs()
            digest(config, 0, call, outs, eng.mem)

    def batch(precision, mode, on):
        eng, rc = engine(precision, mode)
        sb = StreamBatch(eng, streams=2, camera_batch=on, head_batch=on, hole_rows=mode != "topk")
        config = "streams2/%s/%s/%s" % (precision, mode, "batched" if on else "per-stream")
        for call in range(calls):
            frames = [frame(rc, s, call) for s in range(2)]
            outs = sb.forward_frames([f[0] for f in frames], [f[1] for f in frames])
            for s in range(2):
                digest(config, s, call, outs[s], sb.memory(s))

    if args.trace:
        plain("bf16", "topk", False)
        batch("bf16", "topk", True)
    else:
        for mode in MODES:
            for precision, fused in PLAIN:
                plain(precision, mode, fused)
        for fused in (False, True):
            plain("bf16", "topk", fused, graph=True)
        for mode in MODES:
            for precision, fused in PLAIN:
                if not fused:
                    for on in (True, False):
                        batch(precision, mode, on)
    torch.cuda.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if args.summary:
        groups = {}
        for ln in lines:
            groups.setdefault(ln.split()[1], []).append(ln)
        groups["ALL"] = lines
        sha = lambda ls: hashlib.sha256(("\n".join(ls) + "\n").encode()).hexdigest()
        with open(args.summary, "w") as f:
            f.write("".join("%s  %s %d\n" % (sha(ls), config, len(ls)) for config, ls in groups.items()))


if __name__ == "__main__":
    main()

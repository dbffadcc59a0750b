"""Times of the two batched pieces behind far3d_amd/streams.py StreamBatch next to the one-stream code they replace, at the benchmark
geometry (A = 1544 queries, 2312 keys, 8 heads, 7 cameras of 640 x 960: S = 12750 tokens), B = 1, 2, 4 streams, bf16 and fp32:

  (a) attention: ONE far3d_attention_streams launch  against  B far3d_attention_forward launches (q / k / v read in place from a
      (B, 2312, 6 * 3 * 256) QKV buffer, layer 0's column block);
  (b) decoder:   Far3DEngine.decoder_streams         against  B Far3DEngine.decoder calls in their unfused form (fused_rows off);
      bf16 also lists B decoder calls with the row chains (fused_rows on: the default bf16 engine's decoder, other bits).

  python tools/probe/stream_batch_times.py [--out profiles/stream_batch/times.txt] [--rounds 5]

Recorded, not asserted.  The windows are tools/probe/agg_general_times.py's: per (dtype, B) five repetitions in ONE process, the calls
alternating inside a repetition, so that the run-to-run spread of every figure is known; microseconds per call (one call = all B
streams), the median of `rounds` timed windows; a window is as many replays of one hipGraph as fill `--window` seconds of device
time, between two device events; a graph holds LAUNCHES[key] calls.  The decoder's weights are a random initialisation of the
benchmark's head (only the head is built); every stream has its own value maps, reference points, rolled cameras and random query /
memory rows.  Before timing, the batched results are compared with the one-stream results (bitwise)."""
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
LAUNCHES = dict(attn_streams=16, attn_singles=16, dec_streams=2, dec_singles=2, dec_chains=2)     # calls per graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25, help="seconds of device time per timed window")
    args = ap.parse_args()
    import torch
    from far3d_amd import engine, lib, ops, weights
    from tests import cases
    lib.require_device()
    dev = "cuda:0"
    cs = [cases.config2_aggregate_case(seed=b) for b in range(max(BATCHES))]
    for b, c in enumerate(cs):
        c["lidar2img"] = torch.roll(c["lidar2img"], b, 0)
    c0 = cs[0]
    N, S, C = c0["feat"].shape
    A = c0["ref"].shape[0]
    cfg = engine.default_cfg(proposal_topk=(A - 644 - 256) // N)
    E, H, nL, Lm = cfg["embed_dims"], cfg["num_heads"], cfg["num_layers"], cfg["memory_len"]
    Kt = A - cfg["num_propagated"] + Lm
    sd = weights.init_state_dict(weights.detector_spec(cfg["backbone"], num_query=cfg["num_query"], num_propagated=cfg["num_propagated"]), seed=1)
    lines = []

    def emit(row):
        s = json.dumps(row)
        print(s, flush=True)
        lines.append(s)

    emit(dict(kind="geometry", cams=N, image=list(c0["pad_hw"]), S=S, C=C, A=A, keys=Kt, heads=H, layers=nL, batches=list(BATCHES)))
    g = torch.Generator().manual_seed(3)
    for name in ("bf16", "fp32"):
        eng = engine.Far3DEngine(sd, cfg, device=dev, precision=name, parts=("head",))
        at, vt = eng.prec["dec"], eng.prec["value"]
        Bm = max(BATCHES)
        qkv_all = torch.randn(Bm, Kt, nL * 3 * E, generator=g).to(at).to(dev)
        qkv_all[..., :E] *= 2.0
        x2_all = torch.randn(Bm, Kt, 2 * E, generator=g).to(at).to(dev)
        x0_all, qp_all = (torch.randn(Bm, A, E, generator=g).to(dev) for _ in range(2))
        tok_all = torch.stack([c["feat"].to(vt) for c in cs]).to(dev).contiguous()
        ref_all = torch.stack([c["ref"] for c in cs]).to(dev).contiguous()
        l2i_all = torch.stack([c["lidar2img"] for c in cs]).to(dev).contiguous()
        geom = (c0["level_hw"], c0["level_start"])
        for B in BATCHES:
            qkv = qkv_all[:B]
            q, k, v = qkv[:, :A, :E], qkv[:, :, E:2 * E], qkv[:, :, 2 * E:3 * E]
            att_b = torch.empty((B, A, E), dtype=at, device=dev)
            att_s = torch.empty((B, A, E), dtype=at, device=dev)
            lst = lambda t: [t[b] for b in range(B)]
            res = {}

            def attn_streams():
                ops.attention_streams(q, k, v, H, out=att_b)

            def attn_singles():
                for b in range(B):
                    ops.attention_forward(q[b], k[b], v[b], H, out=att_s[b])

            def dec_args(b=None):
                x2 = x2_all[:B].clone()         # the one-stream decoder overwrites the query rows of its operand
                if b is None:
                    return (lst(x2), lst(x0_all), lst(qp_all), lst(tok_all), lst(ref_all), *geom, lst(l2i_all), c0["pad_hw"], A)
                return (x2[b], x0_all[b], qp_all[b], tok_all[b], ref_all[b], *geom, l2i_all[b], c0["pad_hw"], A)

            x2_run = x2_all[:B].clone()

            def dec_streams():
                res["dec_streams"] = eng.decoder_streams(lst(x2_run), lst(x0_all), lst(qp_all), lst(tok_all), lst(ref_all), *geom, lst(l2i_all),
                                                         c0["pad_hw"], A)

            def dec_singles():
                for b in range(B):
                    res["dec_singles"] = eng.decoder(x2_run[b], x0_all[b], qp_all[b], tok_all[b], ref_all[b], *geom, l2i_all[b], c0["pad_hw"], A)

            eng.fused_rows = False
            attn_streams(), attn_singles()
            got = eng.decoder_streams(*dec_args()).clone()
            want = [eng.decoder(*dec_args(b)).clone() for b in range(B)]
            torch.cuda.synchronize()
            emit(dict(kind="agreement", dtype=name, B=B, attention_streams_equals_singles_bitwise=bool(torch.equal(att_b, att_s)),
                      decoder_streams_equals_singles_bitwise=all(torch.equal(got[b], want[b]) for b in range(B)),
                      decoder_outputs_finite=bool(torch.isfinite(got).all()), max_abs_decoder_output=got.abs().max().item()))
            del got, want
            calls = [("attn_streams", attn_streams, False), ("attn_singles", attn_singles, False), ("dec_streams", dec_streams, False),
                     ("dec_singles", dec_singles, False)]
            if name == "bf16":
                calls.append(("dec_chains", dec_singles, True))
            for rep in range(REPS):
                row = dict(kind="times_us", dtype=name, B=B, rep=rep, replays={})
                for key, fn, chains in calls:
                    eng.fused_rows = chains
                    x2_run.copy_(x2_all[:B])
                    torch.cuda.synchronize()
                    us, row["replays"][key] = graph_us(fn, LAUNCHES[key], args.rounds, args.window)
                    row[key] = round(us, 2)
                emit(row)
            eng.fused_rows = False
            del res, att_b, att_s, x2_run
            torch.cuda.empty_cache()
        del eng, qkv_all, x2_all, x0_all, qp_all, tok_all, ref_all, l2i_all
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

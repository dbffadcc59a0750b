"""Sweep the workgroup tile of far3d_conv2d_nhwc for every distinct conv shape of the VoV-99 640x960x7 frame (bf16) and
write the winners to gpurun_out/tuning_mi355x.json (key "Cout,Cin,k,stride,Npix"; copied to far3d_amd/data/).  Device time
via hipGraph replay.  MODE=bf16x3: the split-precision mode (fp32 tensors, tiles 1-5) -> tuning_mi355x_bf16x3.json.
GROUPS=1: the layer groups of the FPN outputs / 2D head as grouped launches (tiles 500-559) -> tuning_mi355x_groups.json."""
import json, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from far3d_amd import ops, weights

def shapes():
    spec = weights.VOV_SPECS["V-99-eSE"]
    N, H, W = int(os.environ.get("NCAM", "7")), 640, 960      # NCAM=1/2/4: the per-rank shapes of camera-sharded runs
    out = []   # (name, N, H, W, Cin, Cout, k, stride)
    h, w = H // 2, W // 2
    out.append(("stem1", N, h, w, 32, 64, 1, 1)); out.append(("stem2", N, h, w, 64, 64, 3, 1)); out.append(("stem3", N, h, w, 64, 128, 3, 2))
    h, w = h // 2, w // 2
    in_ch = 128
    for si in range(4):
        sc, oc = spec["stage_conv_ch"][si], spec["stage_out_ch"][si]
        if si > 0:
            h, w = -(-h // 2), -(-w // 2)
        for b in range(2 if spec["block_per_stage"][si] > 1 else 1):
            out.append(("s%d.b%d.c0" % (si + 2, b), N, h, w, in_ch, sc, 3, 1))
            out.append(("s%d.b%d.c1" % (si + 2, b), N, h, w, sc, sc, 3, 1))
            out.append(("s%d.b%d.cat" % (si + 2, b), N, h, w, in_ch + 5 * sc, oc, 1, 1))
            in_ch = oc
    hw = [(80, 120), (40, 60), (20, 30), (10, 15)]
    for i, cin in zip((2, 1, 0), (1024, 768, 512)):
        out.append(("fpn.lat%d" % i, N, hw[i][0], hw[i][1], cin, 256, 1, 1))
    for l in range(4):
        out.append(("c256.l%d" % l, N, hw[l][0], hw[l][1], 256, 256, 3, 1))
        out.append(("c512.l%d" % l, N, hw[l][0], hw[l][1], 256, 512, 3, 1))
        out.append(("head26.l%d" % l, N, hw[l][0], hw[l][1], 256, 26, 1, 1))
        out.append(("head5.l%d" % l, N, hw[l][0], hw[l][1], 256, 5, 1, 1))
    out.append(("fpn.out3", N, 20, 30, 256, 256, 3, 2)); out.append(("depth.cls", N, 80, 120, 256, 51, 1, 1))
    # decoder linears (A = 1544 queries, 768 memory rows, 644 adaptive proposals)
    for nm, M, ci, co in () if N != 7 else (("dec.qk", 1544, 256, 512), ("dec.v", 1544, 256, 256), ("dec.memk", 768, 256, 256), ("dec.wfc", 1544, 256, 416),
                          ("dec.lfc", 1544, 256, 39), ("dec.ffn1", 1544, 256, 1024), ("dec.ffn2", 1544, 1024, 256), ("dec.m644", 644, 256, 256),
                          ("dec.m300", 300, 256, 256), ("dec.ce", 7, 256, 256)):
        out.append((nm, 1, 1, M, ci, co, 1, 1))
    return out

def timeit(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / (3 * iters)

def timeit_concurrent(make_fn, nstreams=3, iters=8):
    """Time per launch when `nstreams` independent copies of the launch sequence run side by side on high-priority streams -- the
    regime of the frame pipeline (engine.cam_streams), where a tile is judged by the CU-time it occupies, not by its own latency."""
    import time
    fns = [make_fn(j) for j in range(nstreams)]
    graphs = []
    for fn in fns:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        graphs.append(g)
    streams = [torch.cuda.Stream("cuda:0", priority=-1) for _ in range(nstreams)]

    def go():
        for g, st in zip(graphs, streams):
            with torch.cuda.stream(st):
                g.replay()
    go(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(4):
        go()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (4 * nstreams * iters)


def main():
    dev = "cuda:0"
    conc = int(os.environ.get("CONCURRENT", "0"))      # CONCURRENT=3: sweep under the frame pipeline's concurrency -> tuning_mi355x_tput.json
    table, seen = {}, set()
    only = os.environ.get("ONLY_K")
    x3 = os.environ.get("MODE") == "bf16x3"
    pair = os.environ.get("MODE") == "pair"      # pair-stored activations (the bf16x3 engine mode): tiles 150+ -> tuning_mi355x_pair.json
    tdt = torch.float32 if x3 else torch.bfloat16
    for name, N, H, W, Cin, Cout, k, stride in shapes():
        if only and int(only) != k:
            continue
        if os.environ.get("ONLY_NAME") and not name.startswith(os.environ["ONLY_NAME"]):
            continue
        key = "%d,%d,%d,%d,%d" % (Cout, Cin, k, stride, N * H * W)
        if key in seen:
            continue
        seen.add(key)
        if pair and (name.startswith("dec.") or Cin % 32):
            continue
        x = torch.randn(N, H, W, Cin, device=dev).to(tdt)
        if pair:
            x = ops.pair_from_float(x.float())
        pc = ops.PackedConv(torch.randn(Cout, Cin, k, k) * 0.05, torch.randn(Cout), stride=stride, pad=k // 2, dtype=torch.float32 if pair else tdt,
                            device=dev, compute="bf16x3" if (x3 or pair) else None)
        Ho, Wo = pc.out_hw(H, W)
        y = torch.empty(N, Ho, Wo, Cout * 2 if (pair and Cout % 32 == 0) else Cout, device=dev, dtype=tdt if not (pair and Cout % 32) else torch.float32)
        fl = 2.0 * N * Ho * Wo * Cout * Cin * k * k
        res = {}
        tiles = ((0, 1, 2, 3, 4, 18, 43, 46, 48) if not (k == 3 and stride == 1) else (0,)) + ((70, 71, 72, 73, 74, 75, 76, 77, 78, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 110, 111, 114, 116, 117, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 140, 141, 142, 143, 144, 145) if (k == 1 and stride == 1) else ()) + ((50, 52, 60, 61, 63, 64, 65, 90, 92, 93, 96, 100, 101, 102, 103, 130, 131, 132, 133, 134, 135, 136, 137, 138, 139) if (k == 3 and stride == 1) else ())
        if k == 3 and stride == 2 and not (x3 or pair):
            tiles = tiles + (30, 31, 32, 33, 34, 35)
        if x3:
            tiles = (0, 1, 2, 3, 4, 5)
        if pair:
            tiles = (0, 150, 152, 154, 155, 157, 160, 161, 162, 163, 164, 165, 166, 167, 168, 169, 190, 198, 191, 192, 193, 197) + \
                    ((400, 401, 403, 404, 405, 406, 410, 411, 412, 413, 416, 417, 418, 419, 450, 451, 452, 453, 454, 455, 456, 457, 459) if Cout % 32 == 0 and not os.environ.get("NO_WS") else ()) \
                if (k == 3 and stride == 1) else \
                    ((0, 170, 171, 172, 173, 174, 175, 176, 177, 178, 179, 180, 181, 185, 186, 187, 188) + ((460, 461, 462, 463, 464, 465, 466, 467, 468, 469, 470, 471, 473, 474, 475, 476) if Cout % 32 == 0 and not os.environ.get("NO_WS") else ()) if (k == 1 and stride == 1) else
                     (0, 1, 2, 3, 4, 5, 330, 331) if (k == 3 and stride == 2) else (0, 1, 2, 3, 4, 5))
        if k == 3 and stride == 1 and os.environ.get("EXTRA_TILES"):
            tiles = tiles + tuple(int(v) for v in os.environ["EXTRA_TILES"].split(","))
        # SUMS=1: time the 1x1 layers WITH the channel sums of the eSE fusion in their epilogue (GEMM tiles only, Ho*Wo >= 512)
        sums = torch.zeros(N, Cout, dtype=torch.int64, device=dev) if (os.environ.get("SUMS") and k == 1 and Ho * Wo >= 512 and Cout % 8 == 0) else None
        if sums is not None:
            tiles = tuple(tl for tl in tiles if ops.tile_takes_sums(tl, pair))
        ys = [torch.empty_like(y) for _ in range(conc)] if conc else None
        for tile in tiles:
            try:
                if conc:
                    t = timeit_concurrent(lambda j: (lambda: ops.conv2d_nhwc(x, pc, out=ys[j], act="relu", tile=tile, sums=sums)), conc)
                else:
                    t = timeit(lambda: ops.conv2d_nhwc(x, pc, out=y, act="relu", tile=tile, sums=sums))
            except Exception:      # a tile that refuses the channel sums (no LDS left, map smaller than the tile)
                if sums is None:
                    raise
                continue
            res[tile] = t
        tiles = tuple(tl for tl in tiles if tl in res)
        if 0 not in res:
            res[0] = float("nan")
        best = min((t, tl) for tl, t in res.items() if tl != 0)
        table[key] = best[1]
        if ops.is_ws_tile(best[1]):
            # the persistent wave-specialised kernel covers plain layers only: the entry carries the fastest general tile beside it, and the
            # ws tile is taken only where it wins by more than the run-to-run noise (3 %)
            other = min((t, tl) for tl, t in res.items() if tl != 0 and not ops.is_ws_tile(tl))
            table[key] = [best[1], other[1]] if best[0] < 0.97 * other[0] else other[1]
        print("%-10s %-24s auto %7.1f us | " % (name, key, res[0] * 1e6) + " ".join("t%d %4.0f" % (tl, res[tl] * 1e6) for tl in tiles if tl) +
              " | best t%d %6.1f us %6.1f TF/s" % (best[1], best[0] * 1e6, fl / best[0] / 1e12), flush=True)
    name = "tuning_mi355x_pair" if pair else ("tuning_mi355x_bf16x3" if x3 else "tuning_mi355x")
    if conc:
        name += "_tput"
    if os.environ.get("NCAM", "7") != "7":
        name += "_n" + os.environ["NCAM"]
    json.dump(table, open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", name + ".json"), "w"), indent=0, sort_keys=True)

GROUP_CANDIDATES = (500, 505, 552, 556, 559)


def group_shapes(N):
    """The layer groups engine.fpn / engine.roi_head launch as one grouped call: name -> [(H, W, Cout, act, y2)] at Cin 256."""
    hw = [(80, 120), (40, 60), (20, 30), (10, 15)]
    return {"fpn.out": [(h, w, 256, None, True) for h, w in hw[:3]],
            "roi.tower0": [(h, w, 512, "swish", False) for h, w in hw] + [(80, 120, 256, None, False)],
            "roi.cls1reg1": [(h, w, 256, "swish", False) for h, w in hw] * 2 + [(80, 120, 256, None, False)]}


def groups_main():
    """GROUPS=1: time each layer group as its per-layer launches (the tiles the tables ship) and as one grouped launch per candidate tile
    -> $OUT_DIR/tuning_mi355x_groups.json (default: the working directory; copy it to far3d_amd/data/), key "<group>,<level-0 pixels>".  A group gets an entry only where its best grouped launch
    beats the per-layer launches by more than 3 % (the tables' rule for a persistent tile)."""
    dev = "cuda:0"
    N = int(os.environ.get("NCAM", "7"))
    table = {}
    for gname, shp in group_shapes(N).items():
        probs = []
        for (H, W, cout, act, mln) in shp:
            x = ops.pair_from_float(torch.randn(N, H, W, 256, device=dev))
            pc = ops.PackedConv(torch.randn(cout, 256, 3, 3) * 0.05, torch.randn(cout), stride=1, pad=1, dtype=torch.float32, device=dev, compute="bf16x3")
            d = dict(x=x, pc=pc, out=torch.empty(N, H, W, 2 * cout, dtype=torch.bfloat16, device=dev), act=act)
            if mln:
                d.update(y2=torch.empty(N, H, W, cout, device=dev), y2_scale=torch.rand(N, cout, device=dev), y2_shift=torch.rand(N, cout, device=dev))
            probs.append(d)
        fl = sum(2.0 * p["x"].shape[0] * p["x"].shape[1] * p["x"].shape[2] * p["pc"].Cout * 256 * 9 for p in probs)
        t_single = timeit(lambda: [ops.conv2d_nhwc(p["x"], p["pc"], out=p["out"], act=p["act"], y2=p.get("y2"), y2_scale=p.get("y2_scale"),
                                                   y2_shift=p.get("y2_shift")) for p in probs])
        res = {tl: timeit(lambda: ops.conv2d_nhwc_grouped(probs, tl)) for tl in GROUP_CANDIDATES}
        best = min((t, tl) for tl, t in res.items())
        npix = N * shp[0][0] * shp[0][1]
        if best[0] < 0.97 * t_single:
            table["%s,%d" % (gname, npix)] = best[1]
        print("%-13s %2d layers %6.1f GFLOP | per-layer %7.1f us %5.0f TF/s | " % (gname, len(probs), fl / 1e9, t_single * 1e6, fl / t_single / 1e12) +
              " ".join("g%d %6.1f" % (tl, t * 1e6) for tl, t in sorted(res.items())) +
              " | best g%d %6.1f us %5.0f TF/s (%+.1f %%)" % (best[1], best[0] * 1e6, fl / best[0] / 1e12, 100 * (best[0] / t_single - 1)), flush=True)
    name = "tuning_mi355x_groups" + ("" if N == 7 else "_n%d" % N)
    out_dir = os.environ.get("OUT_DIR", ".")
    os.makedirs(out_dir, exist_ok=True)
    json.dump(table, open(os.path.join(out_dir, name + ".json"), "w"), indent=0, sort_keys=True)


if __name__ == "__main__":
    groups_main() if os.environ.get("GROUPS") else main()

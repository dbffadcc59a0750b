"""On / off timings of the parts of the persistent 3x3 kernel (csrc/conv_ws.hpp) on the layers they were built for.

  python tools/probe/ws_conv_parts.py            # the shipped library: every layer / tile once per round (compare two trees by alternating)
  python tools/probe/ws_conv_parts.py parts      # the profiling build: each layer / tile with the deferral and the cost deal switched
                                                 # off in turn (far3d_conv_ws_set_ablate bits 16 / 32: results stay right), alternating
Device time per launch by hipGraph replay (10 launches per graph, 3 replays), ROUNDS rounds; prints every round, not a mean."""
import ctypes, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from far3d_amd import lib as flib
PARTS = len(sys.argv) > 1 and sys.argv[1] == "parts"
if PARTS:
    flib.LIB_PATH = os.path.join(os.path.dirname(flib.LIB_PATH), "libfar3d_hip_prof.so")
from far3d_amd import ops

# (name, N, H, W, Cin, Cout, tiles)
LAYERS = [("s3.c1", 7, 80, 120, 160, 160, (452, 459, 405)), ("s3.b0.c0", 7, 80, 120, 256, 160, (452, 453)),
          ("stem2", 7, 320, 480, 64, 64, (452, 454)), ("s2.c1", 7, 160, 240, 128, 128, (454, 452, 450))]
MASKS = ((0, "all on"), (16, "no deferral"), (32, "static deal"), (48, "neither")) if PARTS else ((0, "shipped"),)
ROUNDS = 3
dev = "cuda:0"
lib = flib.load()
abl = lib.far3d_conv_ws_set_ablate if PARTS else None


def graph_of(fn, iters=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay(); torch.cuda.synchronize()
    return g, iters


def time_graph(g, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(3):
        g.replay()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (3 * iters)


for name, N, H, W, Cin, Cout, tiles in LAYERS:
    x = ops.pair_from_float(torch.randn(N, H, W, Cin, device=dev))
    pc = ops.PackedConv(torch.randn(Cout, Cin, 3, 3) * 0.05, torch.randn(Cout), stride=1, pad=1, dtype=torch.float32, device=dev, compute="bf16x3")
    y = torch.empty(N, H, W, 2 * Cout, device=dev, dtype=torch.bfloat16)
    for tile in tiles:
        graphs = []
        for mask, label in MASKS:
            if abl:
                abl(ctypes.c_int(mask))          # read at launch: captured with the graph's kernel arguments
            graphs.append((label,) + graph_of(lambda: ops.conv2d_nhwc(x, pc, out=y, act="relu", tile=tile)))
        if abl:
            abl(ctypes.c_int(0))
        for r in range(ROUNDS):
            print("%-9s t%d round %d: " % (name, tile, r + 1) + "  ".join("%s %6.1f us" % (label, time_graph(g, it)) for label, g, it in graphs), flush=True)

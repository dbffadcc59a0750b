"""Times of ops.dwconv3x3_nhwc (far3d_dwconv3x3_nhwc) with TWO builds of the library in one process: the one of another commit
(--parent-lib, built from a checkout of that commit) and this tree's, at the six V-19-dw-eSE layer shapes of dwsep_times.py, N = 7,
hipGraph replay (vov_family_times.graph_us).

  python tools/probe/dwconv_plain_times.py --parent-lib /path/to/other/libfar3d_hip.so [--out profiles/dw_core/times.txt] [--rounds 5]

bf16 and pair storage at all six shapes, f32 storage at stem3 and stage3.  Five repetitions per side, alternating parent, this tree,
parent, ...; per shape the mean and the spread (max - min over the repetitions) of either side, and whether this tree's mean exceeds the
parent's by more than the larger of the two spreads.  Both libraries are called through the same wrapper: far3d_amd.lib's handle is
exchanged between the repetitions.  The driver starts one child process per storage, each under its own time limit, and stops at the
first that does not end cleanly."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "probe"))
from vov_family_times import graph_us  # noqa: E402
from dwsep_times import N, VOV  # noqa: E402

STEP_LIMIT = 240      # seconds per child
REPS = 5
F32_SHAPES = ("stem3", "stage3")


def step(dt, parent_lib, rounds):
    import torch
    from far3d_amd import lib, ops
    mine = lib.load()
    parent = ctypes.CDLL(parent_lib)
    for name, (res, args) in lib.SIGNATURES.items():
        if hasattr(parent, name):
            getattr(parent, name).restype, getattr(parent, name).argtypes = res, args
    dev = "cuda:0"
    for name, H, W, C, _, stride, *_ in VOV:
        if dt == "f32" and name not in F32_SHAPES:
            continue
        g = torch.Generator().manual_seed(1)
        x = torch.randn(N, H, W, C, generator=g).to(dev)
        xs = ops.pair_from_float(x) if dt == "pair" else x.to(torch.bfloat16) if dt == "bf16" else x
        w9 = (torch.randn(9, C, generator=g) / 3).to(dev)
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        outs = {}
        for side in ("parent", "new"):
            outs[side] = torch.empty((N, Ho, Wo, xs.shape[3]), dtype=xs.dtype, device=dev)

        def run(side):
            ops.dwconv3x3_nhwc(xs, w9, stride, out=outs[side], pair=dt == "pair")
        iters = 10 if N * Ho * Wo <= 7 * 160 * 240 else 4
        for rep in range(REPS):
            row = dict(dt=dt, name=name, shape=[N, H, W, C, stride], rep=rep)
            for side, handle in (("parent", parent), ("new", mine)):
                lib._lib = handle
                row[side + "_us"] = graph_us(lambda: run(side), iters, rounds)[0]
            lib._lib = mine
            print(json.dumps(row), flush=True)
        print(json.dumps(dict(dt=dt, name=name, same_bits=bool(torch.equal(outs["parent"], outs["new"])))), flush=True)
        del x, xs, outs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dw_core", "times.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", default=None, help="internal: run one storage in this process")
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.parent_lib, a.rounds)
    rows = []
    for dt in ("bf16", "pair", "f32"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", dt, "--parent-lib", a.parent_lib, "--rounds", str(a.rounds)],
                               capture_output=True, text=True, timeout=STEP_LIMIT)
        except subprocess.TimeoutExpired:
            sys.exit("step %s did not finish within %d s; stopping" % (dt, STEP_LIMIT))
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("step %s ended with status %d; stopping" % (dt, r.returncode))
        rows += [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
        print("step %s done" % dt, flush=True)
    write(rows, a.out)


def write(rows, path):
    L = ["ops.dwconv3x3_nhwc, the other commit's library (parent) against this tree's (new) in one process, N = %d, hipGraph replay," % N,
         "%d alternating repetitions (each the median of the rounds); mean us [spread = max - min over the repetitions];" % REPS,
         "bar: new mean - parent mean <= the larger spread", "",
         "%-5s %-7s %-20s %18s %18s %9s %6s %9s" % ("dtype", "layer", "N,H,W,C,stride", "parent us [spread]", "new us [spread]", "new - par", "bar", "same bits")]
    keys = []
    for r in rows:
        if "rep" in r and (r["dt"], r["name"]) not in keys:
            keys.append((r["dt"], r["name"]))
    for dt, name in keys:
        mine = [r for r in rows if "rep" in r and r["dt"] == dt and r["name"] == name]
        same = [r["same_bits"] for r in rows if "same_bits" in r and r["dt"] == dt and r["name"] == name]
        p, n = [r["parent_us"] for r in mine], [r["new_us"] for r in mine]
        pm, ps, nm, ns = sum(p) / len(p), max(p) - min(p), sum(n) / len(n), max(n) - min(n)
        L.append("%-5s %-7s %-20s %10.2f [%5.2f] %10.2f [%5.2f] %+9.2f %6s %9s" %
                 (dt, name, ",".join(map(str, mine[0]["shape"])), pm, ps, nm, ns, nm - pm, "met" if nm - pm <= max(ps, ns) else "MISSED", same))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()

"""Fixture for tests/test_dw_refusals_cpu.py: what the three depthwise entries answer to faulty arguments.

  python tools/gen_golden_dw_refusals.py [path/to/libfar3d_hip.so]     # rewrites tests/golden/dw_refusals.json

Calls far3d_dwconv3x3_nhwc, far3d_dwconv3x3_act_nhwc and far3d_dwsep_conv_nhwc of the given library (default: this tree's; to pin a
refactor, the library built from the commit before it) with every single fault of FAULTS and every pair of them that does not set the
same argument twice.  The pointers are made-up integers: every call must end in an argument check (FAR3D_ERR_ARG) -- the tool refuses to
record anything else -- so nothing is launched and no GPU is needed.  A pair of faults pins the ORDER of the checks: the message is the
one of the check that comes first.  The fixture holds, per entry, the argument names in the order of the C signature, the base values,
the faults that apply to it (name -> overrides) and the calls as [fault index, (fault index,) message index]; the distinct messages
once; the one status.  Fixtures hold data only.
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from far3d_amd import lib as far3d_lib  # noqa: E402

F32, BF16, X3, PAIR = 0, 1, 2, 3
ERR_ARG = -1

# argument names in the order of the C signatures
ARGS = {
    "far3d_dwconv3x3_nhwc": "x dt w y N H W C ldx xs Ho Wo ldy ys stride stream".split(),
    "far3d_dwconv3x3_act_nhwc": "x dt w bias y N H W C ldx xs Ho Wo ldy ys stride reps act stream".split(),
    "far3d_dwsep_conv_nhwc": "x dt w b1 act1 w_pw w_dt b2 act2 y N H W C ldx xs Ho Wo Cout ldy ys stride stream".split(),
}
# a call that passes every check: two 5x6 bf16 images of 32 channels, stride 1, dense rows (the fused entry: 64 output channels)
BASE = dict(x=0x10000, w=0x20000, y=0x30000, bias=0x40000, b1=0x40000, b2=0x50000, w_pw=0x60000, dt=BF16, w_dt=BF16, N=2, H=5, W=6, C=32,
            ldx=32, xs=960, Ho=5, Wo=6, ldy=32, ys=960, stride=1, reps=1, act=1, act1=1, act2=2, Cout=64, stream=0)
FUSED_BASE = dict(ldy=64, ys=1920)

# name -> overrides; a fault applies to the entries that have all its arguments
FAULTS = {
    "null x": dict(x=0), "null w": dict(w=0), "null y": dict(y=0), "null w_pw": dict(w_pw=0),
    "unknown dtype": dict(dt=7),
    "stride 3": dict(stride=3),
    "N = 0": dict(N=0),
    "C = 12": dict(C=12),
    "pair storage, C = 48": dict(dt=PAIR, w_dt=X3, C=48),
    "wrong Ho": dict(Ho=4), "wrong Wo": dict(Wo=5),
    "ldx below the channels": dict(ldx=24), "ldy below the channels": dict(ldy=24),
    "x image stride below one image": dict(xs=952), "y image stride below one image": dict(ys=952),
    "ldx off 16 bytes": dict(ldx=36), "ldy off 16 bytes": dict(ldy=68),
    "x off 16 bytes": dict(x=0x10008), "y off 16 bytes": dict(y=0x30008), "w off 16 bytes": dict(w=0x20008),
    "bias off 16 bytes": dict(bias=0x40008), "b1 off 16 bytes": dict(b1=0x40008), "b2 off 16 bytes": dict(b2=0x50008),
    "w_pw off 16 bytes": dict(w_pw=0x60008),
    "reps 0": dict(reps=0), "reps 3": dict(reps=3),
    "act -1": dict(act=-1), "act 3": dict(act=3), "act1 -1": dict(act1=-1), "act2 3": dict(act2=3),
    "storage and weight mismatch": dict(w_dt=X3),
    "Cout = 288": dict(Cout=288), "Cout = 48": dict(Cout=48),
    "x and y overlap": dict(y=0x10040),
    # the other element sizes and channel counts of the stride and alignment messages
    "f32 storage, ldx off 16 bytes": dict(dt=F32, ldx=34),
    "pair storage, ldx below the stored channels": dict(dt=PAIR, w_dt=X3, ldx=32),
    "two weight sets, ldy below them": dict(reps=2, ldy=32),
}


def entry_faults(names):
    """The faults that apply to an entry with these arguments, reduced to them.  w_dt belongs to the fused entry only (elsewhere the
    pair faults are their other overrides), and so does the overlap rule."""
    return {k: {a: v for a, v in f.items() if a in names} for k, f in FAULTS.items()
            if all(a in names or (a == "w_dt" and len(f) > 1) for a in f) and (k != "x and y overlap" or "Cout" in names)}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else far3d_lib.LIB_PATH
    lib = ctypes.CDLL(path)
    lib.far3d_last_error.restype = ctypes.c_char_p
    messages, entries = [], {}
    for entry, names in ARGS.items():
        base = dict(BASE, **(FUSED_BASE if entry == "far3d_dwsep_conv_nhwc" else {}))
        mine = entry_faults(names)
        keys = list(mine)
        fn = getattr(lib, entry)
        fn.restype, fn.argtypes = far3d_lib.SIGNATURES[entry]
        calls = []
        combos = [(k,) for k in keys] + [c for c in itertools.combinations(keys, 2) if not set(mine[c[0]]) & set(mine[c[1]])]
        for combo in combos:
            args = dict(base)
            for k in combo:
                args.update(mine[k])
            status = fn(*[args[a] for a in names])
            if status != ERR_ARG:
                raise SystemExit("%s with %s returned %d: not an argument refusal" % (entry, combo, status))
            msg = lib.far3d_last_error().decode()
            if msg not in messages:
                messages.append(msg)
            calls.append([keys.index(k) for k in combo] + [messages.index(msg)])
        entries[entry] = dict(args=names, base=[base[a] for a in names], faults=mine, calls=calls)
    out = os.path.join(ROOT, "tests", "golden", "dw_refusals.json")
    with open(out, "w") as f:          # compact, but with line breaks a diff can show
        f.write('{"status": %d,\n "messages": [\n  %s],\n "entries": {\n' % (ERR_ARG, ",\n  ".join(json.dumps(m) for m in messages)))
        blocks = []
        for entry, e in entries.items():
            rows = [json.dumps(e["calls"][i:i + 24], separators=(",", ":"))[1:-1] for i in range(0, len(e["calls"]), 24)]
            blocks.append('  %s: {"args": %s,\n   "base": %s,\n   "faults": {\n    %s},\n   "calls": [\n    %s]}' % (
                json.dumps(entry), json.dumps(e["args"]), json.dumps(e["base"]),
                ",\n    ".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in e["faults"].items()), ",\n    ".join(rows)))
        f.write(",\n".join(blocks) + "}}\n")
    n = sum(len(e["calls"]) for e in entries.values())
    print("wrote", out, "(%d calls, %d distinct messages)" % (n, len(messages)))


if __name__ == "__main__":
    main()

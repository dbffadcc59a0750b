"""Fixture for tests/test_norm_refusals_cpu.py: what the entries of the normalisation family answer to faulty arguments.

  python tools/gen_golden_norm_refusals.py [path/to/libfar3d_hip.so]     # rewrites tests/golden/norm_refusals.json

Calls far3d_layernorm, far3d_layernorm_rows, far3d_row_affine_ln, far3d_ese_nhwc, far3d_ese_fused_nhwc, far3d_groupnorm_nhwc,
far3d_maxpool3x3s2_nhwc and far3d_cam_embed_chain of the given library (default: this tree's; to pin a refactor, the library built from
the commit before it) with every single fault of the entry and every pair of them that does not set the same argument twice.  The
pointers are made-up integers: every call must end in an argument check (FAR3D_ERR_ARG) -- the tool refuses to record anything else --
so nothing is launched and no GPU is needed.  A pair of faults pins the ORDER of the checks: the message is the one of the check that
comes first.  A fault listed in PAIRS_ONLY is recorded in pairs and never alone: before its check moved in front of the first launch,
far3d_groupnorm_nhwc answered `groups * 2 > C` alone with FAR3D_ERR_ARG only after it had launched a kernel.  The fixture has the
layout of tests/golden/dw_refusals.json: per entry the argument names in the order of the C signature, the base values, the faults
(name -> overrides) and the calls as [fault index, (fault index,) message index]; the distinct messages once; the one status.
Fixtures hold data only.
"""
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from far3d_amd import lib as far3d_lib  # noqa: E402

F32, BF16, PAIR = 0, 1, 3
ERR_ARG = -1

_LN_ARGS = "x gamma beta y rows C ldx ldy eps act add lda y2 ldy2 y2_dt yb ldyb yb_dt".split()
_LN_BASE = dict(x=0x10000, gamma=0x20000, beta=0x30000, y=0x40000, rows=5, C=256, ldx=256, ldy=256, eps=1e-5, act=0, add=0x50000, lda=256,
                y2=0x60000, ldy2=256, y2_dt=F32, yb=0x70000, ldyb=256, yb_dt=BF16, out_rows=0x80000, stream=0)
_LN_FAULTS = {
    "null x": dict(x=0), "null y": dict(y=0),
    "rows = -1": dict(rows=-1), "C = 0": dict(C=0), "C = 258": dict(C=258), "C = 1028": dict(C=1028),
    "ldx off 4": dict(ldx=258), "ldy off 4": dict(ldy=258), "lda off 4": dict(lda=258), "ldy2 off 4": dict(ldy2=258),
    "ldyb off 4": dict(ldyb=258), "y2 without add": dict(add=0),
}
_NHWC = dict(x=0x10000, y=0x20000, identity=0x30000, pooled=0x40000, scratch=0x50000, gate=0x60000, fcw=0x70000, fcb=0x80000,
             gamma=0x70000, beta=0x80000, dt=BF16, N=2, stream=0)

# entry -> (argument names in the order of the C signature, a call that passes every check, name -> overrides)
ENTRIES = {
    "far3d_layernorm": (_LN_ARGS + ["stream"], _LN_BASE, _LN_FAULTS),
    "far3d_layernorm_rows": (_LN_ARGS + ["out_rows", "stream"], _LN_BASE,
                             dict(_LN_FAULTS, **{"null out_rows": dict(out_rows=0), "neither y2 nor yb": dict(y2=0, yb=0)})),
    "far3d_row_affine_ln": ("x gamma beta add y rows C ldx ldg lda ldy eps do_ln stream".split(),
                            dict(x=0x10000, gamma=0x20000, beta=0x30000, add=0x40000, y=0x50000, rows=5, C=256, ldx=256, ldg=256, lda=256,
                                 ldy=256, eps=1e-5, do_ln=1, stream=0),
                            {"null x": dict(x=0), "null gamma": dict(gamma=0), "null beta": dict(beta=0), "null y": dict(y=0),
                             "C = 128": dict(C=128), "ldx off 4": dict(ldx=258), "ldg off 4": dict(ldg=258), "lda off 4": dict(lda=258),
                             "ldy off 4": dict(ldy=258)}),
    # two 5x6 bf16 maps of 64 channels, dense rows, an identity, no fixed-point sums
    "far3d_ese_nhwc": ("x dt fcw fcb identity y scratch N HW C ldx xs ldi is ldy ys chan_sums stream".split(),
                       dict(_NHWC, HW=30, C=64, ldx=64, xs=1920, ldi=64, ldy=64, ys=1920, chan_sums=0, **{"is": 1920}),
                       {"null x": dict(x=0), "null fcw": dict(fcw=0), "null fcb": dict(fcb=0), "null y": dict(y=0), "null scratch": dict(scratch=0),
                        "unknown storage": dict(dt=7), "fixed-point sums, f32 storage": dict(dt=F32, chan_sums=0x90000),
                        "N = 0": dict(N=0), "HW = 0": dict(HW=0), "C = 0": dict(C=0), "C = 66": dict(C=66), "C = 1028": dict(C=1028),
                        "pair storage, C = 48": dict(dt=PAIR, C=48),
                        "ldx off 4": dict(ldx=66), "ldy off 4": dict(ldy=66), "ldi off 4": dict(ldi=66)}),
    # the same maps with the fixed-point sums, the full-resolution output and the 2x3 pooled one
    "far3d_ese_fused_nhwc": ("x dt fcw fcb identity y pooled gate N H W C ldx xs ldi is ldy ys Hp Wp ldp ps chan_sums stream".split(),
                             dict(_NHWC, H=5, W=6, C=64, ldx=64, xs=1920, ldi=64, ldy=64, ys=1920, Hp=2, Wp=3, ldp=64, ps=384,
                                  chan_sums=0x90000, **{"is": 1920}),
                             {"null x": dict(x=0), "null fcw": dict(fcw=0), "null fcb": dict(fcb=0), "null gate": dict(gate=0),
                              "null chan_sums": dict(chan_sums=0), "y and pooled both null": dict(y=0, pooled=0),
                              "f32 storage": dict(dt=F32), "unknown storage": dict(dt=7),
                              "N = 0": dict(N=0), "C = 0": dict(C=0), "C = 68": dict(C=68), "C = 1032": dict(C=1032),
                              "pair storage, C = 80": dict(dt=PAIR, C=80),
                              "x off 16 bytes": dict(x=0x10008), "identity off 16 bytes": dict(identity=0x30008), "y off 16 bytes": dict(y=0x20008),
                              "pooled off 16 bytes": dict(pooled=0x40008), "gate off 16 bytes": dict(gate=0x60008),
                              "ldx off 8": dict(ldx=68), "xs off 8": dict(xs=1924), "ldi off 8": dict(ldi=68), "is off 8": {"is": 1924},
                              "ldy off 8": dict(ldy=68), "ys off 8": dict(ys=1924), "ldp off 8": dict(ldp=68), "ps off 8": dict(ps=388),
                              "wrong Hp": dict(Hp=3), "wrong Wp": dict(Wp=2)}),
    # two 5x7 bf16 maps of 256 channels, 32 groups
    "far3d_groupnorm_nhwc": ("x dt gamma beta y scratch N HW C groups eps relu stream".split(),
                             dict(_NHWC, HW=35, C=256, groups=32, eps=1e-5, relu=1),
                             {"null x": dict(x=0), "null gamma": dict(gamma=0), "null beta": dict(beta=0), "null y": dict(y=0),
                              "null scratch": dict(scratch=0), "N = 0": dict(N=0), "HW = 0": dict(HW=0), "C = 258": dict(C=258),
                              "C = 1056": dict(C=1056), "groups = 0": dict(groups=0), "groups = 48": dict(groups=48),
                              "unknown storage": dict(dt=7), "pair storage, C = 48": dict(dt=PAIR, C=48, groups=12),
                              "groups * 2 > C": dict(C=32, groups=32)}),
    # two 8x9 bf16 maps of 64 channels -> 4x4
    "far3d_maxpool3x3s2_nhwc": ("x dt y N H W C Ho Wo ldy ys stream".split(),
                                dict(_NHWC, H=8, W=9, C=64, Ho=4, Wo=4, ldy=64, ys=1024),
                                {"null x": dict(x=0), "null y": dict(y=0), "unknown storage": dict(dt=7),
                                 "pair storage, C = 48": dict(dt=PAIR, C=48, ldy=96), "pair storage, ldy below the stored channels": dict(dt=PAIR),
                                 "N = 0": dict(N=0), "H = 0": dict(H=0), "C = 66": dict(C=66), "ldy below the channels": dict(ldy=32),
                                 "ldy off 4": dict(ldy=66), "wrong Ho": dict(Ho=3), "wrong Wo": dict(Wo=5)}),
    "far3d_cam_embed_chain": ("l2i w0t b0 w2t b2 ln_g ln_b w3t b3 out N L J Hd eps ld_l2i stream".split(),
                              dict(l2i=0x10000, w0t=0x20000, b0=0x30000, w2t=0x40000, b2=0x50000, ln_g=0x60000, ln_b=0x70000, w3t=0x80000,
                                   b3=0x90000, out=0xa0000, N=5, L=3, J=416, Hd=128, eps=1e-5, ld_l2i=16, stream=0),
                              dict({"null " + p: {p: 0} for p in "l2i w0t b0 w2t b2 ln_g ln_b w3t b3 out".split()},
                                   **{"N = 0": dict(N=0), "L = 0": dict(L=0), "J = 0": dict(J=0), "Hd = 0": dict(Hd=0), "Hd = 257": dict(Hd=257),
                                      "ld_l2i = 11": dict(ld_l2i=11)})),
}
PAIRS_ONLY = {"far3d_groupnorm_nhwc": ("groups * 2 > C",)}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else far3d_lib.LIB_PATH
    lib = ctypes.CDLL(path)
    lib.far3d_last_error.restype = ctypes.c_char_p
    messages, entries = [], {}
    for entry, (names, base, faults) in ENTRIES.items():
        keys = list(faults)
        fn = getattr(lib, entry)
        fn.restype, fn.argtypes = far3d_lib.SIGNATURES[entry]
        calls = []
        combos = [(k,) for k in keys if k not in PAIRS_ONLY.get(entry, ())]
        combos += [c for c in itertools.combinations(keys, 2) if not set(faults[c[0]]) & set(faults[c[1]])]
        for combo in combos:
            args = dict(base)
            for k in combo:
                args.update(faults[k])
            status = fn(*[args[a] for a in names])
            if status != ERR_ARG:
                raise SystemExit("%s with %s returned %d: not an argument refusal" % (entry, combo, status))
            msg = lib.far3d_last_error().decode()
            if msg not in messages:
                messages.append(msg)
            calls.append([keys.index(k) for k in combo] + [messages.index(msg)])
        entries[entry] = dict(args=names, base=[base[a] for a in names], faults=faults, calls=calls)
    out = os.path.join(ROOT, "tests", "golden", "norm_refusals.json")
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

"""What the tile selection of far3d_amd.ops hands out, as one JSON-able record (no GPU needed).  tests/golden/tile_selection.json is this
record taken at the commit whose selection is the reference (copy this file into that checkout: it uses only what ops had then);
tests/test_tile_selection_cpu.py replays it on the current tree.
  python tests/tile_selection.py [out.json]
"""
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from far3d_amd import ops, weights  # noqa: E402

DATA = os.path.join(ROOT, "far3d_amd", "data")
SEVENTHS = (7, 1, 2, 3, 4, 5, 6)          # the entry's own pixel count, then the camera-sharded ones


def tuned(table):
    """key -> per pixel count of SEVENTHS: [ws_ok False, ws_ok True] of _tuned_tile."""
    out = {}
    for key in sorted(json.load(open(os.path.join(DATA, table)))):
        co, ci, k, st, npix = (int(v) for v in key.split(","))
        out[key] = [[ops._tuned_tile(co, ci, k, st, npix * f // 7, table, ws_ok=ws) for ws in (False, True)] for f in SEVENTHS]
    return out


def pair(bf16_table):
    """key -> per pixel count: [terms 3 / ws_ok False, 3 / True, 1 / False, 1 / True] of _pair_tile under the pair table of bf16_table."""
    out = {}
    with ops.use_tile_tables(bf16_table):
        for key in sorted(json.load(open(os.path.join(DATA, ops.tile_tables()[1])))):
            co, ci, k, st, npix = (int(v) for v in key.split(","))
            pcs = [types.SimpleNamespace(Cout=co, Cin=ci, KH=k, KW=k, stride=st, pad=k // 2, terms=t) for t in (3, 1)]
            out[key] = [[ops._pair_tile(pc, ci, npix * f // 7, 0, ws) for pc in pcs for ws in (False, True)] for f in SEVENTHS]
    return out


def groups():
    out = {}
    for key in sorted(json.load(open(os.path.join(DATA, ops.GROUP_TILE_TABLE)))):
        g, npix = key.rsplit(",", 1)
        out[key] = [ops.group_tile(g, int(npix)), ops.group_tile(g, int(npix) // 2)]
    return out


def concat_layers():
    """(stage, first block, cameras, pair) of the OSA concat layers tests/test_host_cpu.py walks."""
    spec = weights.VOV_SPECS["V-99-eSE"]
    hw = [(160, 240), (80, 120), (40, 60), (20, 30)]
    in_ch = spec["stem"][2]
    for si in range(4):
        sc, oc = spec["stage_conv_ch"][si], spec["stage_out_ch"][si]
        for first in (True, False):
            cin = (in_ch if first else oc) + 5 * sc
            for pr in (False, True):
                pc = ops.PackedConv(torch.zeros(oc, cin, 1, 1), torch.zeros(oc), dtype=torch.float32 if pr else torch.bfloat16, device="cpu",
                                    compute="bf16x3" if pr else None)
                for ncam in (7, 4, 2, 1):
                    yield "%d,%d,%d,%d" % (si, first, ncam, pr), torch.empty(ncam, hw[si][0], hw[si][1], cin * (2 if pr else 1), dtype=torch.bfloat16), pc
            if spec["block_per_stage"][si] == 1:
                break
        in_ch = oc


def record():
    return {"tuned": {t: tuned(t) for t in ("tuning_mi355x.json", "tuning_mi355x_tput.json", "tuning_mi355x_bf16x3.json")},
            "pair": {t: pair(t) for t in ("tuning_mi355x.json", "tuning_mi355x_tput.json")},
            "groups": groups(),
            "fuse_sums": {k: bool(ops.conv_can_fuse_sums(x, pc)) for k, x, pc in concat_layers()}}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "tile_selection.json")
    json.dump(record(), open(out, "w"), separators=(",", ":"), sort_keys=True)

"""CPU: the tile selection of far3d_amd.ops reproduces tests/golden/tile_selection.json entry for entry.  The fixture was recorded by
tests/tile_selection.py at the commit BEFORE the selection moved into ops._conv_plan: every key of the shipped tables, at its
own and at the camera-sharded pixel counts, with and without ws_ok, split products and hi planes only; the grouped table; and
conv_can_fuse_sums on the OSA concat layers of the benchmarked frame (bf16 and pair-stored)."""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_selection_matches_the_recorded_one(hip_lib):
    from tests import tile_selection as gen
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "tile_selection.json")))
    got = json.loads(json.dumps(gen.record()))
    assert sorted(got) == sorted(want)
    for part in want:
        assert sorted(got[part]) == sorted(want[part]), part
        for name, entries in want[part].items():
            assert got[part][name] == entries, (part, name)


def test_conv_tile_reports_what_conv2d_nhwc_launches(hip_lib):
    """ops.conv_tile with the call's optional arguments = the tile of ops._conv_plan, i.e. of conv2d_nhwc: on a [ws, general] entry the
    persistent tile for a plain call, the general one for a call with a residual or an fp32 output."""
    import torch
    from far3d_amd import ops
    table = json.load(open(os.path.join(ROOT, "far3d_amd", "data", "tuning_mi355x_pair.json")))
    key, (ws, gen) = next((k, v) for k, v in sorted(table.items()) if isinstance(v, list) and k.split(",")[2] == "3")
    cout, cin, k, stride, npix = (int(v) for v in key.split(","))
    pc = ops.PackedConv(torch.zeros(cout, cin, 3, 3), None, stride=1, pad=1, dtype=torch.float32, device="cpu", compute="bf16x3")
    x = torch.empty(1, npix // 32, 32, 2 * cin, dtype=torch.bfloat16)
    assert ops.conv_tile(x, pc) == ws and ops.is_ws_tile(ws) and not ops.is_ws_tile(gen)
    assert ops.conv_tile(x, pc, res=torch.empty(1, npix // 32, 32, 2 * cout, dtype=torch.bfloat16)) == gen
    assert ops.conv_tile(x, pc, out_dtype=torch.float32) == gen and ops.conv_tile(x, pc, sums=True) == gen

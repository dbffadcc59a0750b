"""CPU: ops.tiles_as_for -- inside it a convolution on the images of several scene streams plans its launch as ONE stream's images
would (Far3DEngine.camera_stage_streams): the tile-table lookups, and the library's own heuristic where the tables have no entry.
Planning reads shapes, strides and addresses only, so host tensors do."""
import pytest
import torch

from far3d_amd import ops


def _pc(cout, cin, k, dtype, stride=1, compute=None):
    return ops.PackedConv(torch.zeros(cout, cin, k, k), None, stride=stride, pad=k // 2, dtype=dtype, compute=compute)


def test_auto_tile_is_the_register_staged_kernels_heuristic():
    # csrc/igemm_kernels.hpp igemm_auto_tile: Cout <= 64: 2 from 128 * 512 pixels, else 3; else 1 from 512 tiles of 128 x 128, 4 from 512
    # tiles of 128 x 64, else 3
    assert ops._auto_tile(128 * 512, 64) == 2 and ops._auto_tile(128 * 512 - 1, 64) == 3
    assert ops._auto_tile(128 * 511 + 1, 128) == 1 and ops._auto_tile(128 * 511, 128) == 4
    assert ops._auto_tile(64 * 511 + 1, 128) == 4 and ops._auto_tile(64 * 511, 128) == 3
    assert ops._auto_tile(128 * 255 + 1, 256) == 1 and ops._auto_tile(100, 1024) == 3


def test_table_lookups_see_one_streams_pixels():
    # tuning_mi355x.json, layer (192, 192, 3x3): tile 102 at 2400 pixels (one 40 x 60 image), 100 at 16800 (seven)
    pc = _pc(192, 192, 3, torch.bfloat16)
    one, seven = torch.empty(1, 40, 60, 192, dtype=torch.bfloat16), torch.empty(7, 40, 60, 192, dtype=torch.bfloat16)
    t1, t7 = ops.conv_tile(one, pc), ops.conv_tile(seven, pc)
    assert t1 != t7 and t1 and t7
    with ops.tiles_as_for(1, 7):
        assert ops.conv_tile(seven, pc) == t1
        assert ops.conv_tile(one, pc) == t1                      # another image count: not touched
        assert ops.plan_images(7) == 1 and ops.plan_images(1) == 1 and ops.plan_images(14) == 14
        with ops.tiles_as_for(7, 14):                            # nests, and restores
            assert ops.plan_images(14) == 7 and ops.plan_images(7) == 7
        assert ops.plan_images(7) == 1
    assert ops.conv_tile(seven, pc) == t7 and ops.plan_images(7) == 7
    # the grouped launches: the group's pixel count scales the same way (an entry holds only near its own count)
    import json
    import os
    groups = json.load(open(os.path.join(os.path.dirname(ops.__file__), "data", ops.GROUP_TILE_TABLE)))
    name, npx = next(iter(groups)).rsplit(",", 1)
    want = ops.group_tile(name, int(npx))
    assert want and not ops.group_tile(name, 4 * int(npx))
    with ops.tiles_as_for(7, 28):
        assert ops.group_tile(name, 4 * int(npx)) == want


def test_the_librarys_heuristic_is_pinned_to_one_streams_answer():
    # fp32 maps and weights have no table: tile 0 = igemm_auto_tile(pixels, Cout).  7 images of 40 x 60: 16800 pixels -> 3; 28: 67200 -> 1
    pc = _pc(128, 64, 3, torch.float32)
    x7, x28 = torch.empty(7, 40, 60, 64), torch.empty(28, 40, 60, 64)
    assert ops.conv_tile(x7, pc) == 0 and ops.conv_tile(x28, pc) == 0
    assert ops._auto_tile(7 * 2400, 128) == 3 and ops._auto_tile(28 * 2400, 128) == 1
    with ops.tiles_as_for(7, 28):
        assert ops.conv_tile(x28, pc) == 3                       # explicit: the same kernel, one stream's tile
        assert ops.conv_tile(x7, pc) == 0
    # an explicit tile of the caller's is never replaced
    with ops.tiles_as_for(7, 28):
        assert ops._conv_plan(x28, pc, torch.float32, tile=4)[2] == 4
    # pair-stored 3x3 / 1x1 stride-1 layers without a table entry keep the library's fixed defaults (tile 0 -> 160 / 179)
    pp = _pc(96, 96, 3, torch.float32, compute="bf16x3")
    xp = torch.empty(28, 40, 60, 192, dtype=torch.bfloat16)
    assert ops.conv_tile(xp, pp) == 0
    with ops.tiles_as_for(7, 28):
        assert ops.conv_tile(xp, pp) == 0
    # ... and a strided one gets the heuristic's answer for one stream
    ps = _pc(96, 96, 3, torch.float32, stride=2, compute="bf16x3")
    with ops.tiles_as_for(7, 28):
        assert ops.conv_tile(xp, ps) == ops._auto_tile(7 * 20 * 30, 96)


def test_a_choice_that_cannot_be_pinned_is_refused_by_name():
    # fp32 rows x split weights, 1x1: tiles 479 / 480 by the pixel count, and only where the library's alignment checks pass
    pc = _pc(1024, 96, 1, torch.float32, compute="bf16x3")
    small, big = torch.empty(4, 64, 64, 96), torch.empty(16, 64, 64, 96)      # 128 x 8 tiles = 1024 per 4 images; 4096 per 16
    assert ops.conv_tile(big, pc) == 0
    with ops.tiles_as_for(4, 16):
        with pytest.raises(ValueError, match="96 -> 1024"):
            ops.conv_tile(big, pc)
        assert ops.conv_tile(small, pc) == 0
    with ops.tiles_as_for(8, 16):                                # 2048 and 4096 tiles: the same answer, left to the library
        assert ops.conv_tile(big, pc) == 0
    with pytest.raises(ValueError, match="whole number"):
        with ops.tiles_as_for(3, 7):
            pass

"""GPU: the persistent 3x3 kernel's skipped padded channel slices, deferred epilogue and cost-dealt items (csrc/conv_ws.hpp).

None of the three changes a product or the order of the products of an output element, so every output here must be bit-identical
(torch.equal) to the same layer on the general pair tile 163 -- the yardstick tests/test_pair_gpu.py pins the persistent tiles to.
Outputs are channel / row slices of wider buffers pre-filled with a sentinel: the columns beyond Cout and the rows beyond the image
must stay untouched, also by the epilogue that is emitted late, inside the next item's steps.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.0
REF_TILE = 163


@functools.lru_cache(maxsize=None)
def _layer(cin, cout, bias, seed=0):
    from far3d_amd import ops
    g = torch.Generator().manual_seed(1000 * cin + cout + seed)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    b = torch.randn(cout, generator=g) if bias else None
    return ops.PackedConv(w, b, stride=1, pad=1, dtype=torch.float32, device=DEV, compute="bf16x3")


@functools.lru_cache(maxsize=None)
def _input(N, H, W, cin):
    from far3d_amd import ops
    g = torch.Generator().manual_seed(N * 7 + H * 5 + W * 3 + cin)
    return ops.pair_from_float(torch.randn(N, H, W, cin, generator=g)).to(DEV)


def _out_buffer(N, H, W, cout):
    """(whole buffer, the output view): 2 extra rows per image and 64 + 96 extra stored channels around the output, all SENTINEL."""
    buf = torch.full((N, H + 2, W, 2 * cout + 160), SENTINEL, dtype=torch.bfloat16, device=DEV)
    return buf, buf[:, :H, :, 64:64 + 2 * cout]


def _conv(tile, N, H, W, cin, cout, act, bias):
    from far3d_amd import ops
    buf, out = _out_buffer(N, H, W, cout)
    ops.conv2d_nhwc(_input(N, H, W, cin), _layer(cin, cout, bias), out=out, act=act, tile=tile)
    return buf


@functools.lru_cache(maxsize=None)
def _reference(N, H, W, cin, cout, act, bias):
    buf = _conv(REF_TILE, N, H, W, cin, cout, act, bias)
    H_, c0, c1 = H, 64, 64 + 2 * cout
    assert (buf[:, H_:] == SENTINEL).all() and (buf[..., :c0] == SENTINEL).all() and (buf[..., c1:] == SENTINEL).all()
    assert not (buf[:, :H_, :, c0:c1] == SENTINEL).all()
    return buf


def _check(tile, N, H, W, cin, cout, act, bias):
    want = _reference(N, H, W, cin, cout, act, bias)
    got = _conv(tile, N, H, W, cin, cout, act, bias)
    # the sentinel columns and rows are part of the comparison: one torch.equal over the whole buffer
    assert torch.equal(got, want), "tile %d differs from tile %d on N=%d H=%d W=%d Cin=%d Cout=%d act=%s bias=%s" % (
        tile, REF_TILE, N, H, W, cin, cout, act, bias)


# BM = 64 tiles of each consumer layout (452: 2 x 4 waves of 32 ch x 2 rows, 454: 1 x 8 of 64 ch x 1 row, 459: 2 x 4 of 32 ch x 1 row)
# and the BM = 128 tile 405 (2 x 4 of 64 ch x 1 row: with Cout = 160 its second channel tile has one valid slice of four)
SLICE_TILES = (452, 454, 459, 405)


@pytest.mark.parametrize("tile", SLICE_TILES)
def test_padded_channel_slices(hip_lib, tile):
    for cout in (32, 96, 160, 224):
        for act in ("relu", "swish", None):
            for bias in (True, False):
                _check(tile, 2, 11, 37, 64, cout, act, bias)


@pytest.mark.parametrize("tile", SLICE_TILES)
def test_several_items_per_workgroup_with_mixed_costs(hip_lib, tile):
    """Cout = 160 on N = 4, H = 61, W = 150: ragged in both directions; with 8-row tiles 4 x 8 x 5 pixel tiles x 3 channel tiles = 480 items
    on 256 workgroups -- full and light items in one workgroup, every epilogue but the last deferred.  N = 1, H = 8, W = 32: at most three
    items in the launch, nothing is deferred."""
    _check(tile, 4, 61, 150, 64, 160, "swish", True)
    _check(tile, 1, 8, 32, 64, 160, "relu", True)


@pytest.mark.parametrize("tile", (452, 454, 450))
def test_one_chunk_items_have_fewer_groups_than_slices(hip_lib, tile):
    """Cin = 32 on a tile with one hand-over per kernel row: an item is three hand-over groups, its pending epilogue four slices."""
    _check(tile, 4, 61, 150, 32, 160, "swish", True)
    _check(tile, 4, 61, 150, 32, 160, None, False)


@pytest.mark.parametrize("tile", (552, 559))
def test_grouped_launch_pending_item_keeps_its_problem(hip_lib, tile):
    """Two problems of different size, Cout and activation in one launch, more items than workgroups: some workgroups finish an item of
    the first (large) problem and emit its epilogue inside an item of the second, whose pointers, strides, Cout and activation differ.
    Both write the fp32 y2 output, and both have items that are not the last of their workgroup: deferred y2 stores, and pending items
    that carry each problem's own activation, Cout and pointers.  Bit for bit the per-problem launches on tile 163."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(tile)
    # 8-row tile 552: 4 x 5 x 5 x 3 = 300 items, then 4 x 7 x 10 x 1 = 280, on 256 workgroups: workgroups 0-43 walk A, A, B, workgroups
    # 44-67 A, B, B -- pending items of either problem, emitted inside an item of the second; 4-row tile 559: 600 + 560 items
    shapes = ((4, 40, 150, 160, "swish", True), (4, 56, 300, 64, None, True))
    probs, want = [], []
    for (N, H, W, cout, act, mln) in shapes:
        pc = _layer(64, cout, True, seed=tile)
        x = _input(N, H, W, 64)
        d = dict(x=x, pc=pc, act=act)
        ref = dict(x=x, pc=pc, act=act)
        for dd in (d, ref):
            dd["buf"], dd["out"] = _out_buffer(N, H, W, cout)
        if mln:
            scale, shift = torch.randn(N, cout, generator=g).to(DEV) + 1.0, torch.randn(N, cout, generator=g).to(DEV)
            for dd in (d, ref):
                dd["y2buf"] = torch.full((N, H * W + 5, cout + 8), 9.0, device=DEV)
                dd["y2"] = dd["y2buf"][:, 3:3 + H * W, :cout].view(N, H, W, cout)
                dd["y2_scale"], dd["y2_shift"] = scale, shift
        probs.append(d)
        want.append(ref)
    for r in want:
        kw = {k: r[k] for k in ("y2", "y2_scale", "y2_shift") if k in r}
        ops.conv2d_nhwc(r["x"], r["pc"], out=r["out"], act=r["act"], tile=REF_TILE, **kw)
    ops.conv2d_nhwc_grouped([{k: v for k, v in p.items() if k not in ("buf", "y2buf")} for p in probs], tile)
    for i, (p, r) in enumerate(zip(probs, want)):
        assert not (r["out"] == SENTINEL).all()
        assert torch.equal(p["buf"], r["buf"]), "tile %d, problem %d: grouped output differs from the single launch" % (tile, i)
        if "y2buf" in p:
            assert not (r["y2"] == 9.0).all()
            assert torch.equal(p["y2buf"], r["y2buf"]), "tile %d, problem %d: grouped y2 differs from the single launch" % (tile, i)

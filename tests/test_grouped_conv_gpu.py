"""GPU: grouped launches of the persistent 3x3 kernel (ops.conv2d_nhwc_grouped, far3d_conv2d_nhwc_grouped, tiles 500-559).

Several independent 3x3 convolutions of one Cin walk ONE item list of the persistent wave-specialised kernel.  Every output must be
bit-identical (torch.equal) to the same problem launched on its own with the tiles the engine ships for it: the split-product 3x3
kernels all add the same products in the same order (chunk-major, tap, k-half; lo*hi', hi*lo', hi*hi'), so grouping changes no
element's accumulation chain -- including the camera-aware MLN second output y2 of the FPN outputs.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUP_TILES = (500, 505, 552, 556, 559)


def _layer(g, cin, cout):
    from far3d_amd import ops
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.05
    b = torch.randn(cout, generator=g)
    return ops.PackedConv(w, b, stride=1, pad=1, dtype=torch.float32, device=DEV, compute="bf16x3")


def _pair_map(g, N, H, W, C, pad_c=0):
    """A pair-stored (N,H,W,2C) map, as a channel slice [pad_c, pad_c + C) of a wider buffer when pad_c > 0."""
    from far3d_amd import ops
    x = torch.randn(N, H, W, C, generator=g)
    buf = torch.full((N, H, W, 2 * (C + 2 * pad_c)), 3.0, dtype=torch.bfloat16, device=DEV)
    buf[..., 2 * pad_c:2 * pad_c + 2 * C] = ops.pair_from_float(x).to(DEV)
    return buf[..., 2 * pad_c:2 * pad_c + 2 * C]


def _mln(g, N, H, W, C):
    y2buf = torch.full((N, H * W + 5, C), 9.0, device=DEV)        # a token slice of a wider buffer, as in engine.fpn
    y2 = y2buf[:, 3:3 + H * W].view(N, H, W, C)
    return y2buf, y2, torch.randn(N, C, generator=g).to(DEV) + 1.0, torch.randn(N, C, generator=g).to(DEV)


def _case(g, shapes, cin, mln=False, out_slices=False):
    """shapes: (N, H, W, Cout, act) per problem.  Returns the problem dicts (outputs unset) and per-problem extra state."""
    probs = []
    for i, (N, H, W, cout, act) in enumerate(shapes):
        p = dict(x=_pair_map(g, N, H, W, cin, pad_c=32 * (i % 2)), pc=_layer(g, cin, cout), act=act)
        if mln:
            p["y2buf"], p["y2"], p["y2_scale"], p["y2_shift"] = _mln(g, N, H, W, cout)
        p["pad"] = 32 if out_slices and i % 2 else 0
        probs.append(p)
    return probs


def _outs(probs):
    """Fresh output buffers (7.0 everywhere, the output as a channel slice where pad > 0) and fresh y2 buffers."""
    bufs = []
    for p in probs:
        N, H, W, _ = p["x"].shape
        C, pad = p["pc"].Cout, p["pad"]
        buf = torch.full((N, H, W, 2 * (C + 2 * pad)), 7.0, dtype=torch.bfloat16, device=DEV)
        y2buf = p["y2buf"].clone().fill_(9.0) if "y2buf" in p else None
        bufs.append((buf, buf[..., 2 * pad:2 * pad + 2 * C], y2buf))
    return bufs


def _y2_view(p, y2buf):
    N, H, W, _ = p["x"].shape
    return y2buf[:, 3:3 + H * W].view(N, H, W, p["pc"].Cout)


def _run_single(probs, bufs):
    """Each problem on its own, with the tile the engine ships for it (table lookup: persistent where the call allows it, else general)."""
    from far3d_amd import ops
    for p, (_, out, y2buf) in zip(probs, bufs):
        kw = {}
        if y2buf is not None:
            kw = dict(y2=_y2_view(p, y2buf), y2_scale=p["y2_scale"], y2_shift=p["y2_shift"])
        ops.conv2d_nhwc(p["x"], p["pc"], out=out, act=p["act"], **kw)


def _run_grouped(probs, bufs, tile):
    from far3d_amd import ops
    arg = []
    for p, (_, out, y2buf) in zip(probs, bufs):
        d = dict(x=p["x"], pc=p["pc"], out=out, act=p["act"])
        if y2buf is not None:
            d.update(y2=_y2_view(p, y2buf), y2_scale=p["y2_scale"], y2_shift=p["y2_shift"])
        arg.append(d)
    return ops.conv2d_nhwc_grouped(arg, tile)


def _check_equal(probs, want, got, tile):
    for i, (p, (wb, _, wy), (gb, _, gy)) in enumerate(zip(probs, want, got)):
        assert torch.equal(wb, gb), "tile %d, problem %d %s: grouped output differs from the single launch" % (tile, i, tuple(p["x"].shape))
        if wy is not None:
            assert torch.equal(wy, gy), "tile %d, problem %d: grouped y2 differs from the single launch" % (tile, i)
            assert (gy[:, :3] == 9.0).all() and (gy[:, 3 + p["x"].shape[1] * p["x"].shape[2]:] == 9.0).all()


@pytest.mark.parametrize("tile", GROUP_TILES)
def test_grouped_conv3x3_equals_single_launches(hip_lib, tile):
    """Ragged H / W (W % 32, H % TH), channel-slice views in and out, mixed Cout (incl. one channel tile past the packed rows), mixed
    activations, several images, more items than one round of workgroups: every output bit for bit the single launch's."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(tile)
    shapes = [(7, 80, 120, 512, "swish"), (7, 40, 60, 512, "swish"), (7, 20, 30, 512, "swish"), (7, 10, 15, 512, "swish"),
              (7, 80, 120, 256, None)]
    probs = _case(g, shapes, 256)
    want, got = _outs(probs), _outs(probs)
    _run_single(probs, want)
    _run_grouped(probs, got, tile)
    _check_equal(probs, want, got, tile)
    # ragged small problems, mixed Cout and activations, channel slices on both sides, Cin of one chunk
    g = torch.Generator().manual_seed(1000 + tile)
    shapes = [(2, 13, 45, 224, "relu"), (1, 9, 70, 64, None), (3, 20, 30, 96, "swish"), (1, 1, 1, 32, "relu")]
    for cin in (32, 160):
        probs = _case(g, shapes, cin, out_slices=True)
        want, got = _outs(probs), _outs(probs)
        for p, (_, out, _) in zip(probs, want):
            ops.conv2d_nhwc(p["x"], p["pc"], out=out, act=p["act"], tile=163)
        _run_grouped(probs, got, tile)
        _check_equal(probs, want, got, tile)
        for p, (buf, _, _) in zip(probs, got):
            pad, C = 2 * p["pad"], 2 * p["pc"].Cout
            assert (buf[..., :pad] == 7.0).all() and (buf[..., pad + C:] == 7.0).all()


@pytest.mark.parametrize("tile", (552, 559))
def test_grouped_conv3x3_mln_second_output(hip_lib, tile):
    """The FPN outputs' group: no activation, the fp32 second output y2 = scale[n][m] * v + shift[n][m] into token slices -- bit for
    bit the general kernel's y2 (the persistent single-layer kernel has no y2 epilogue)."""
    g = torch.Generator().manual_seed(77 + tile)
    probs = _case(g, [(7, 80, 120, 256, None), (7, 40, 60, 256, None), (7, 20, 30, 256, None)], 256, mln=True)
    want, got = _outs(probs), _outs(probs)
    _run_single(probs, want)
    _run_grouped(probs, got, tile)
    _check_equal(probs, want, got, tile)
    # y2 on for some problems and off for others in one launch
    g = torch.Generator().manual_seed(78 + tile)
    probs = _case(g, [(2, 13, 45, 96, "relu"), (3, 9, 33, 64, None)], 64, mln=True)
    del probs[1]["y2buf"]
    want, got = _outs(probs), _outs(probs)
    _run_single(probs, want)
    _run_grouped(probs, got, tile)
    _check_equal(probs, want, got, tile)


def test_grouped_conv3x3_single_problem(hip_lib):
    """G = 1: a group of one is the single launch."""
    g = torch.Generator().manual_seed(5)
    probs = _case(g, [(7, 40, 60, 512, "swish")], 256)
    want, got = _outs(probs), _outs(probs)
    _run_single(probs, want)
    _run_grouped(probs, got, 559)
    _check_equal(probs, want, got, 559)


def test_grouped_conv3x3_refusals_are_errors(hip_lib):
    """Mixed Cin, more than GROUP_MAX problems, an unsupported layer or epilogue, an unknown tile: errors, nothing is launched."""
    from far3d_amd import lib, ops
    g = torch.Generator().manual_seed(9)
    a = dict(x=_pair_map(g, 1, 8, 8, 64), pc=_layer(g, 64, 64))
    b = dict(x=_pair_map(g, 1, 8, 8, 96), pc=_layer(g, 96, 64))
    sentinel = torch.full((1, 8, 8, 128), 5.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(Exception):
        ops.conv2d_nhwc_grouped([dict(a, out=sentinel), b], 552)                   # mixed Cin
    with pytest.raises(Exception):
        ops.conv2d_nhwc_grouped([a] * (ops.GROUP_MAX + 1), 552)                    # too many problems
    with pytest.raises(Exception):
        ops.conv2d_nhwc_grouped([a], 452)                                          # not a grouped tile
    with pytest.raises(Exception):
        ops.conv2d_nhwc_grouped([a], 501)                                          # no such grouped tile
    s2 = ops.PackedConv(torch.randn(64, 64, 3, 3), None, stride=2, pad=1, dtype=torch.float32, device=DEV, compute="bf16x3")
    with pytest.raises(Exception):
        ops.conv2d_nhwc_grouped([a, dict(x=a["x"], pc=s2)], 552)                   # stride 2
    hi = _layer(g, 64, 64)
    hi.terms = 1
    with pytest.raises(Exception):
        ops.conv2d_nhwc_grouped([dict(x=a["x"], pc=hi)], 552)                      # one-product layer
    with pytest.raises(Exception):
        ops.conv2d_nhwc_grouped([dict(a, out=torch.empty(1, 8, 8, 64, device=DEV))], 552)      # fp32 output
    torch.cuda.synchronize()
    assert (sentinel == 5.0).all()
    # the C entry itself refuses mixed Cin and an oversized group (the wrapper checks first; the library never relies on it)
    arr = (ops._ConvProblem * 2)()
    for i, p in enumerate((a, b)):
        c = arr[i]
        c.x, c.w, c.y = p["x"].data_ptr(), p["pc"].w.data_ptr(), sentinel.data_ptr()
        c.N, c.H, c.W, c.Cin, c.Cout, c.ldx, c.ldy = 1, 8, 8, p["pc"].Cin, 64, p["x"].stride(2), 128
        c.x_img_stride, c.y_img_stride = p["x"].stride(0), 8 * 8 * 128
    import ctypes
    assert hip_lib.far3d_conv2d_nhwc_grouped(ctypes.cast(arr, ctypes.c_void_p), 2, 552, None) != 0
    assert b"Cin" in lib.load().far3d_last_error()
    assert hip_lib.far3d_conv2d_nhwc_grouped(ctypes.cast(arr, ctypes.c_void_p), ops.GROUP_MAX + 1, 552, None) != 0
    torch.cuda.synchronize()
    assert (sentinel == 5.0).all()


def test_engine_grouped_head_is_bitwise_the_per_layer_head(hip_lib):
    """engine.fpn / roi_head with the grouped launches against the same engine with grouping switched off: every output map equal."""
    from far3d_amd import engine, ops, synth, weights
    kw = dict(num_cams=2, num_query=60, num_propagated=16, memory_len=64, topk_proposals=16)
    spec = weights.detector_spec("V-99-eSE", num_query=60, num_propagated=16)
    sd = weights.init_state_dict(spec, seed=1)
    eng = engine.Far3DEngine(sd, engine.default_cfg(**kw), device=DEV, precision="bf16x3")
    data, metas = synth.make_frame(2, (128, 192), seed=5, frame_index=0)
    res = {}
    for grouped in (False, True):
        saved = dict(ops._TUNING)
        try:
            ops._TUNING[ops.GROUP_TILE_TABLE] = {"fpn.out": [(2 * 16 * 24, 552)], "roi.tower0": [(2 * 16 * 24, 552)],
                                                "roi.cls1reg1": [(2 * 16 * 24, 559)]} if grouped else {}
            eng.reset_memory()
            with torch.no_grad():
                out = eng.forward_frame(data, metas)
            torch.cuda.synchronize()
            res[grouped] = {k: v.clone() for k, v in out.items() if isinstance(v, torch.Tensor)}
            res[grouped].update({"%s.%d" % (k, i): t.clone() for k, v in out.items() if isinstance(v, (list, tuple))
                                 for i, t in enumerate(v) if isinstance(t, torch.Tensor)})      # the FPN maps
        finally:
            ops._TUNING.clear()
            ops._TUNING.update(saved)
    assert res[False].keys() == res[True].keys() and res[False]
    for k in res[False]:
        a, b = res[False][k], res[True][k]
        if k == "sel_idx" and "sel_cnt" in res[False]:      # a capacity buffer: only the first sel_cnt[n] entries of row n are defined
            cnt = res[False]["sel_cnt"]
            assert torch.equal(cnt, res[True]["sel_cnt"])
            a = torch.cat([a[n, :int(c)] for n, c in enumerate(cnt.flatten().tolist())])
            b = torch.cat([b[n, :int(c)] for n, c in enumerate(cnt.flatten().tolist())])
        assert torch.equal(a, b), k

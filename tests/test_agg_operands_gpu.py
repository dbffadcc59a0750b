"""GPU: far3d_agg_operands / far3d_camera_sum (csrc/agg_operands.hip), ops.aggregate_general and the aggregation module outside the
fused family.  References and bounds: tests/agg_operand_refs.py (float64 restatement of the reference's text; locations bounded per
element by the counted roundings, weights by chain_bound against the float32 restatement's own error).

Figures of one MI355X run (the tests print them): locations at most 0.11 of their bound, key points 0.36, weights 0.17 of chain_bound
(9.4e-9 .. 9.1e-8 absolute), row sums off from 1 by at most 3.4e-7 (row bounds 2.4e-7 .. 7.8e-6); aggregate_general against the oracle
3.9e-7 .. 1.3e-6 on fp32 and bf16 values, the fused kernel beside it 4.2e-7 .. 1.3e-6 (bar 2e-5); the module at 128 / 4 / 3 / 2 / 5 with
two samples 2.2e-7 (bar 2e-4)."""
import copy
import ctypes

import pytest
import torch

from tests import agg_operand_refs as R
from tests import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(t):
    return t.to(DEV).contiguous()


def _run(c, expand=True, ld_extra=None, key_points=False, sample=None):
    """ops.agg_operands on a named case.  ld_extra: None = dense operands; k = U and the offsets as column blocks of one row-strided
    buffer of J + 1 + 3P + k columns (the gaps hold NaN).  sample: only that sample of the batch, as a batch of one."""
    from far3d_amd import ops
    B, N, A, G, L, P = c["dims"]
    sl = slice(None) if sample is None else slice(sample, sample + 1)
    ref, l2i, Vc = _dev(c["ref"][sl]), _dev(c["lidar2img"][sl]), _dev(c["Vc"][sl])
    U, offs = c["U"][sl], c["offsets"][sl].reshape(-1, A, 3 * P)
    if ld_extra is None:
        U, offs = _dev(U), _dev(offs)
    else:
        J = U.shape[-1]
        buf = torch.full((U.shape[0], A, J + 1 + 3 * P + ld_extra), float("nan"))
        buf[:, :, :J], buf[:, :, J + 1:J + 1 + 3 * P] = U, offs
        buf = buf.to(DEV)
        U, offs = buf[:, :, :J], buf[:, :, J + 1:J + 1 + 3 * P]
    return ops.agg_operands(ref, offs, l2i, U, Vc, L, G, c["pc_range"], c["pad_hw"], expand=expand, key_points=key_points)


def test_lds_above_64k_in_ascending_size(hip_lib):
    """The kernel's dynamic LDS depends on the shape, and above 64 KiB the runtime must be told the kernel's limit, once per device.
    Four shapes above 64 KiB in ascending size (67072, 132608, 133120, 134144 bytes) in one process: each later call needs more than
    any call before it.  This is the first test of the file so that, in file order, its first call is also the process's first above
    64 KiB; then the smallest of them once more."""
    for name in R.LDS_ASCENDING + R.LDS_ASCENDING[:1]:
        c = R.case(name)
        loc, w = _run(c)
        R.check_locations(loc.cpu()[:, :, 0, 0], c, name)
        R.check_weights(w.cpu(), c, name)


@pytest.mark.parametrize("name", R.CASES)
def test_operands_against_float64(hip_lib, name):
    c = R.case(name)
    B, N, A, G, L, P = c["dims"]
    if name == "near":
        assert int((R.loc_bound(c)[2] < 1e-5).sum()) > 0, "the clamp branch must run"
    loc, w, kp = _run(c, key_points=True)
    assert loc.shape == (B * N, A, G, L, P, 2) and w.shape == (B * N, A, G, L * P) and kp.shape == (B, A, P, 3)
    loc_c, w_c = loc.cpu(), w.cpu()
    assert torch.equal(loc_c, loc_c[:, :, :1, :1].expand_as(loc_c)), "every (group, level) repeats the same P points"
    R.check_locations(loc_c[:, :, 0, 0], c, name)
    R.check_weights(w_c, c, name)
    R.check_key_points(kp.cpu(), c, name)
    J = L * P * G
    for extra in ((4 - (J + 1 + 3 * P) % 4) % 4, (4 - (J + 1 + 3 * P) % 4) % 4 + 1):     # row stride a multiple of 4 floats, and not
        loc_s, w_s = _run(c, ld_extra=extra)
        assert torch.equal(loc_s, loc) and torch.equal(w_s, w), "row-strided U / offsets (ld = J + %d) change the result" % (1 + 3 * P + extra)


@pytest.mark.parametrize("name", ["general", "groups3"])
def test_batch_equals_single_calls_bitwise(hip_lib, name):
    c = R.case(name)
    B, N = c["dims"][:2]
    loc, w, kp = _run(c, key_points=True)
    for b in range(B):
        l1, w1, k1 = _run(c, key_points=True, sample=b)
        assert torch.equal(l1, loc[b * N:(b + 1) * N]) and torch.equal(w1, w[b * N:(b + 1) * N]) and torch.equal(k1, kp[b:b + 1])


@pytest.mark.parametrize("name", ["general", "family", "groups3", "unstaged"])
def test_compact_locations_and_rerun_bitwise(hip_lib, name):
    c = R.case(name)
    B, N, A, G, L, P = c["dims"]
    loc, w = _run(c)
    loc_c, w_c = _run(c, expand=False)
    assert loc_c.shape == (B * N, A, P, 2)
    assert torch.equal(loc_c, loc[:, :, 0, 0]) and torch.equal(w_c, w)
    loc2, w2 = _run(c)
    assert torch.equal(loc2, loc) and torch.equal(w2, w)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_aggregate_general_matches_oracle(hip_lib, dtype):
    """The bar tests/test_sampling_gpu.py holds the fused kernel to on this case; the fused kernel beside it on the same inputs.  bf16
    values: the oracle runs on the same bf16-rounded maps, as there."""
    from far3d_amd import ops
    for seed in range(3):
        c = cases.small_aggregate_case(seed)
        want = cases.oracle_aggregate(c, dtype)
        got = ops.aggregate_general(_dev(c["feat"].to(dtype)), _dev(c["ref"]), _dev(c["offsets"]), _dev(c["lidar2img"]), _dev(c["U"]),
                                    _dev(c["Vc"]), c["level_hw"], c["level_start"], c["pc_range"], c["pad_hw"], c["G"])
        assert got.shape == (1,) + tuple(want.shape)
        err = (got[0].cpu() - want).abs().max().item()
        fused = (cases.hip_aggregate(c, DEV, dtype).float().cpu() - want).abs().max().item()
        print("seed %d %s: aggregate_general %.3e, fused %.3e" % (seed, dtype, err, fused))
        assert err < 2e-5 and fused < 2e-5


def test_aggregate_general_batched_equals_per_sample(hip_lib):
    """Two samples in one call (different maps, cameras and queries) == the two one-sample calls, bit for bit."""
    from far3d_amd import ops
    cs = [cases.small_aggregate_case(seed) for seed in (3, 4)]
    cs[1]["lidar2img"] = torch.roll(cs[1]["lidar2img"], 1, 0)
    one = [ops.aggregate_general(_dev(c["feat"]), _dev(c["ref"]), _dev(c["offsets"]), _dev(c["lidar2img"]), _dev(c["U"]), _dev(c["Vc"]),
                                 c["level_hw"], c["level_start"], c["pc_range"], c["pad_hw"], c["G"]) for c in cs]
    st = lambda k: _dev(torch.stack([c[k] for c in cs]))
    c = cs[0]
    both = ops.aggregate_general(_dev(torch.cat([x["feat"] for x in cs])), st("ref"), st("offsets"), st("lidar2img"), st("U"), st("Vc"),
                                 c["level_hw"], c["level_start"], c["pc_range"], c["pad_hw"], c["G"])
    assert both.shape == (2, 37, 256)
    assert torch.equal(both[0:1], one[0]) and torch.equal(both[1:2], one[1])


@pytest.mark.parametrize("shape", [(2, 3, 5, 12), (1, 17, 3, 7), (2, 7, 37, 256), (3, 1, 4, 8)])
def test_camera_sum(hip_lib, shape):
    from far3d_amd import ops
    B, N, A, C = shape
    x = torch.randn(B * N, A, C, generator=torch.Generator().manual_seed(B + 10 * N))
    got = ops.camera_sum(_dev(x), N).cpu()
    xs = x.view(B, N, A, C)
    loop = xs[:, 0].clone()
    for n in range(1, N):
        loop = loop + xs[:, n]
    assert got.shape == (B, A, C) and torch.equal(got, loop)
    want, mag = xs.double().sum(1), xs.double().abs().sum(1)
    assert bool(((got.double() - want).abs() <= N * 2.0 ** -24 * mag).all())


# ------------------------------------------------------------------------------------------------ the module
def _module(embed_dims, num_groups, num_levels, num_cams, num_pts, seed):
    from far3d_amd import plugin
    m = plugin.ATTENTION.build(dict(type="DeformableFeatureAggregationCuda", embed_dims=embed_dims, num_groups=num_groups,
                                    num_levels=num_levels, num_cams=num_cams, dropout=0.1, num_pts=num_pts, bias=2.0))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.05 if p.dim() > 1 else 0.1))
        m.learnable_fc.weight.mul_(10.0)
    m.precision = "fp32"
    return m, g


def _module_inputs(g, bs, A, C, N, L, pad_hw=(64, 96)):
    from far3d_amd import synth
    hw = synth.level_shapes(pad_hw)[:L]
    starts, S = synth.level_starts(hw)
    _, _, l2i = synth.ring_cameras(N, pad_hw)
    return dict(x=torch.randn(bs, A, C, generator=g), qpos=torch.randn(bs, A, C, generator=g), feat=torch.randn(bs * N, S, C, generator=g),
                ref=torch.rand(bs, A, 3, generator=g), shapes=torch.tensor([list(h) for h in hw]), starts=torch.tensor(starts),
                pc=torch.tensor(list(synth.PC_RANGE)), l2i=torch.stack([torch.roll(l2i, b, 0) for b in range(bs)]).contiguous(),
                metas=[dict(pad_shape=[pad_hw + (3,)] * N)], pad_hw=pad_hw)


def _call(fn, i):
    return fn(i["x"].to(DEV), i["qpos"].to(DEV), i["feat"].to(DEV), i["ref"].to(DEV), i["shapes"].to(DEV), i["starts"].to(DEV),
              i["pc"].to(DEV), i["l2i"].to(DEV), i["metas"])


def _reference_forward(m, i):
    """The reference module's forward (detr3d_transformer.py:522-569), float64, on a copy of the module's own parameters."""
    from oracle import sampling
    r = copy.deepcopy(m).double()
    x, qpos, feat, ref, l2i = (i[k].double() for k in ("x", "qpos", "feat", "ref", "l2i"))
    bs, A = ref.shape[:2]
    G, N = r.num_groups, l2i.shape[1]
    pc = i["pc"].double()
    ref_m = ref * (pc[3:6] - pc[0:3]) + pc[0:3]
    key_points = ref_m.unsqueeze(-2) + r.learnable_fc(x).reshape(bs, A, -1, 3)
    cam = r.cam_embed(l2i[..., :3, :].flatten(-2))
    feat_pos = (x + qpos).unsqueeze(2) + cam.unsqueeze(1)
    w = r.weights_fc(feat_pos).reshape(bs, A, -1, G).softmax(dim=-2)
    w = w.reshape(bs, A, N, -1, G).permute(0, 2, 1, 4, 3).contiguous().flatten(end_dim=1)
    p2d = sampling.project_points(key_points, l2i, i["pad_hw"]).flatten(end_dim=1)
    p2d = p2d[:, :, None, None, :, :].repeat(1, 1, G, r.num_levels, 1, 1)
    bn, S, C = feat.shape
    out = sampling.msda_grid_sample(feat.reshape(bn, S, G, -1), i["shapes"], i["starts"], p2d, w)
    out = out.reshape(bs, N, A, -1).sum(1)
    return r.output_proj(out) + x


def test_module_outside_the_family_batched(hip_lib):
    """embed_dims 128, 4 groups, 3 levels, 2 cameras, 5 points, two samples, fp32: against the float64 restatement of the reference
    forward, at the bar tests/test_plugin_gpu.py holds its module test to (2e-4)."""
    m, g = _module(128, 4, 3, 2, 5, seed=21)
    i = _module_inputs(g, bs=2, A=23, C=128, N=2, L=3)
    with torch.no_grad():
        want = _reference_forward(m, i)
    m = m.to(DEV)
    got = _call(m, i)
    assert got.shape == (2, 23, 128)
    err = (got.cpu().double() - want).abs().max().item()
    print("module 128/4/3/2/5, bs 2: max abs err %.3e" % err)
    assert err < 2e-4
    so = _call(m.sampling_operands, i)
    assert so["sampling_locations"].shape == (4, 23, 4, 3, 5, 2) and so["attention_weights"].shape == (4, 23, 4, 15)
    assert so["key_points"].shape == (2, 23, 5, 3)


def test_sampling_operands_equal_ops_agg_operands(hip_lib):
    from far3d_amd import ops
    m, g = _module(128, 4, 3, 2, 5, seed=22)
    i = _module_inputs(g, bs=2, A=9, C=128, N=2, L=3)
    m = m.to(DEV)
    so = _call(m.sampling_operands, i)
    P = m._pack(torch.device(DEV))
    x, xq = i["x"].to(DEV).reshape(18, 128), (i["x"] .to(DEV) + i["qpos"].to(DEV)).reshape(18, 128)
    l2i = i["l2i"].to(DEV)
    ce = ops.linear(ops.linear(l2i[:, :, :3, :].reshape(4, 12).contiguous(), P["ce0"], act="relu"), P["ce2"], act="relu")
    ce = ops.layernorm(ce, *P["ce_ln"])
    Vc, U, offs = ops.linear(ce, P["wfc_full"]), ops.linear(xq.contiguous(), P["wfc"]), ops.linear(x.contiguous(), P["lfc"])
    loc, w, kp = ops.agg_operands(i["ref"].to(DEV), offs.view(2, 9, 15), l2i, U.view(2, 9, 60), Vc.view(2, 2, 60), 3, 4,
                                  i["pc"].tolist(), i["pad_hw"], key_points=True)
    assert torch.equal(so["sampling_locations"], loc) and torch.equal(so["attention_weights"], w) and torch.equal(so["key_points"], kp)


def test_module_family_shape_keeps_the_fused_calls(hip_lib):
    """bs = 1 at the family shape: bit-equal to the sequence of ops the module has always run, the fused kernel called directly."""
    from far3d_amd import ops
    m, g = _module(256, 8, 4, 3, 13, seed=23)
    i = _module_inputs(g, bs=1, A=50, C=256, N=3, L=4)
    m = m.to(DEV)
    got = _call(m, i)
    P = m._pack(torch.device(DEV))
    x = i["x"].to(DEV)[0].float().contiguous()
    xq = (i["x"].to(DEV)[0] + i["qpos"].to(DEV)[0]).float().contiguous()
    l2i = i["l2i"].to(DEV)[0].float().contiguous()
    ce = ops.linear(ops.linear(l2i[:, :3, :].flatten(1).contiguous(), P["ce0"], act="relu"), P["ce2"], act="relu")
    ce = ops.layernorm(ce, *P["ce_ln"])
    Vc, U, offs = ops.linear(ce, P["wfc_full"]), ops.linear(xq, P["wfc"]), ops.linear(x, P["lfc"])
    hw = [tuple(int(v) for v in r) for r in i["shapes"].tolist()]
    agg = ops.aggregate_forward(i["feat"].to(DEV).contiguous(), i["ref"].to(DEV)[0].float().contiguous(), offs, l2i, U, Vc, hw,
                                [int(v) for v in i["starts"].tolist()], [float(v) for v in i["pc"].tolist()], (64, 96), num_groups=8)
    want = ops.linear(agg, P["oproj"], res=x)[None]
    assert got.shape == (1, 50, 256) and torch.equal(got, want)
    # and the general path agrees with it at the fused kernel's own tolerance, through the output projection
    gen = m._forward_general(i["x"].to(DEV), i["qpos"].to(DEV), i["feat"].to(DEV), i["ref"].to(DEV), i["shapes"].to(DEV),
                             i["starts"].to(DEV), i["pc"].to(DEV), i["l2i"].to(DEV), i["metas"])
    assert (gen - got).abs().max().item() < 2e-4


# ------------------------------------------------------------------------------------------------ refusals
REFUSED = [dict(N=33), dict(L=9), dict(P=65), dict(G=65), dict(N=32, L=8, P=64), dict(N=0), dict(G=0), dict(ldU=-1)]


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: "-".join("%s%s" % kv for kv in d.items()))
def test_refused_sizes_launch_nothing(hip_lib, bad):
    """Sizes outside what the kernel is built for: FAR3D_ERR_ARG with the sizes in the message, the output buffers keep every byte, and
    the next good call works."""
    from far3d_amd import lib, ops
    s = dict(B=1, A=2, N=2, G=2, P=3, L=2, ldU=0)
    s.update(bad)
    J = s["L"] * s["P"] * s["G"]
    if s["ldU"] < 0:
        s["ldU"] = J - 1                      # a row stride shorter than the row
    n_in = max(1, s["B"] * s["A"] * max(J, 3 * s["P"]), s["B"] * max(s["N"], 1) * max(J, 16))
    src = torch.zeros(n_in, device=DEV)
    n_out = max(1, s["B"] * max(s["N"], 1) * s["A"] * 2 * J)
    loc, w = torch.full((n_out,), 7.0, device=DEV), torch.full((n_out,), 7.0, device=DEV)
    pc = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = hip_lib.far3d_agg_operands(p(src), p(src), p(src), p(src), p(src), p(loc), p(w), None, s["B"], s["A"], s["N"], s["G"], s["P"],
                                    s["L"], ctypes.cast(pc, ctypes.c_void_p), 64.0, 96.0, s["ldU"], 0, 1, None)
    msg = hip_lib.far3d_last_error().decode()
    assert st == -1, (st, msg)
    key = [k for k in bad if k != "ldU"] or ["ldU"]
    assert all(("%s=%d" % (k, s[k])) in msg for k in key), msg
    torch.cuda.synchronize()
    assert bool((loc == 7.0).all()) and bool((w == 7.0).all())
    with pytest.raises(lib.Far3dHipError):
        ops.agg_operands(torch.zeros(2, 3, device=DEV), torch.zeros(2, 65 * 3, device=DEV), torch.zeros(2, 4, 4, device=DEV),
                         torch.zeros(2, 65 * 4, device=DEV), torch.zeros(2, 65 * 4, device=DEV), 2, 2, [-1, -1, -1, 1, 1, 1], (64, 96))
    c = R.case("general")
    loc_ok, w_ok = _run(c)
    R.check_locations(loc_ok.cpu()[:, :, 0, 0], c, "after a refusal")
    R.check_weights(w_ok.cpu(), c, "after a refusal")

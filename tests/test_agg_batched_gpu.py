"""GPU: far3d_aggregate_batched (ops.aggregate_batched) -- the fused aggregation for a batch of samples in one launch -- and the
aggregation module's bs > 1 dispatch at the fused family.

The contract under test is bitwise: out[b] of the batched launch == far3d_aggregate_forward on sample b's operands, whatever B is.  So
the bars here are torch.equal, except where the issue asks for an independent statement: each sample against the CPU oracle at 2e-5 (the
bar tests/test_agg_operands_gpu.py holds the fused kernel and the general path to on the same case) and the module against the float64
restatement of the reference forward at 2e-4 (that file's bar).  The tests print the measured errors.

Figures of one MI355X run: the batched launch against the oracle 3.0e-7 .. 1.2e-6 on f32 and on bf16-rounded maps (bar 2e-5); the module at
256 / 8 / 4 / 3 / 13 with two samples 2.7e-7 against the float64 restatement (bar 2e-4).

Inputs: cases.aggregate_case(num_cams, (64, 96), A, P, seed) -- S = 128 tokens, 4 levels -- one seed per sample, camera matrices
rolled per sample."""
import ctypes
import functools

import pytest
import torch

from tests import cases
from tests.test_agg_operands_gpu import _call, _module, _module_inputs, _reference_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B3 = 3

# (N, P, A): what it hits
SHAPES = [(3, 13, 37),     # kernel 8, the P = 13 specialisation; 40 slots, 3 idle
          (3, 4, 5),       # kernel 8 generic; fewer queries than XCD slots
          (8, 8, 37),      # kernel 8 at its camera limit; N*P*L = 256
          (9, 8, 37),      # kernel 7, by N > 8
          (3, 17, 37)]     # kernel 7, by P > 16
OPERANDS = ("feat", "ref", "offsets", "lidar2img", "U", "Vc")


@functools.lru_cache(maxsize=None)
def _samples(N, P, A):
    """B3 samples of one shape (host tensors, never modified): a list of cases, and the stacked operands."""
    cs = [cases.aggregate_case(N, (64, 96), A, P=P, seed=11 * N + P + b, offset_std=4.0) for b in range(B3)]
    for b, c in enumerate(cs):
        c["lidar2img"] = torch.roll(c["lidar2img"], b, 0)
    return cs, {k: torch.stack([c[k] for c in cs]) for k in OPERANDS}


def _dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def _geom(c):
    return c["level_hw"], c["level_start"], c["pc_range"], c["pad_hw"]


def _batched(cs, st, sl=slice(None), feat_dtype=torch.float32, **kw):
    from far3d_amd import ops
    return ops.aggregate_batched(_dev(st["feat"][sl], feat_dtype), _dev(st["ref"][sl]), _dev(st["offsets"][sl]), _dev(st["lidar2img"][sl]),
                                 _dev(st["U"][sl]), _dev(st["Vc"][sl]), *_geom(cs[0]), num_groups=cs[0]["G"], **kw)


def _single(c, feat_dtype=torch.float32, **kw):
    from far3d_amd import ops
    return ops.aggregate_forward(_dev(c["feat"], feat_dtype), _dev(c["ref"]), _dev(c["offsets"]), _dev(c["lidar2img"]), _dev(c["U"]),
                                 _dev(c["Vc"]), *_geom(c), num_groups=c["G"], **kw)


# ------------------------------------------------------------------------------------------------ 1. bitwise against the one-sample launch
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["out_f32", "out_bf16"])
@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16], ids=["maps_f32", "maps_bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-P%d-A%d" % s)
def test_batched_equals_one_sample_launches_bitwise(hip_lib, shape, feat_dtype, out_dtype):
    cs, st = _samples(*shape)
    N, P, A = shape
    got = _batched(cs, st, feat_dtype=feat_dtype, out_dtype=out_dtype)
    assert got.shape == (B3, A, 256) and got.dtype == out_dtype
    one = [_single(c, feat_dtype, out_dtype=out_dtype) for c in cs]
    for b in range(B3):
        assert one[b].abs().max().item() > 0
        assert torch.equal(got[b], one[b]), "sample %d differs from its one-sample launch" % b
    # a batch of one is the one-sample call, for every sample: the result does not depend on B
    for b in range(B3):
        assert torch.equal(_batched(cs, st, slice(b, b + 1), feat_dtype, out_dtype=out_dtype)[0], one[b])
    assert torch.equal(_batched(cs, st, feat_dtype=feat_dtype, out_dtype=out_dtype), got)      # and the same from run to run


# ------------------------------------------------------------------------------------------------ 2. against the CPU oracle
@pytest.mark.parametrize("feat_dtype", [torch.float32, torch.bfloat16], ids=["maps_f32", "maps_bf16"])
def test_batched_against_the_oracle(hip_lib, feat_dtype):
    """bf16 maps: the oracle runs on the same bf16-rounded maps."""
    cs, st = _samples(3, 13, 37)
    got = _batched(cs, st, feat_dtype=feat_dtype).cpu()
    for b, c in enumerate(cs):
        err = (got[b] - cases.oracle_aggregate(c, feat_dtype)).abs().max().item()
        print("sample %d, %s maps: batched launch vs oracle %.3e (bar 2e-5)" % (b, feat_dtype, err))
        assert err < 2e-5


# ------------------------------------------------------------------------------------------------ 3. samples do not touch each other
@pytest.mark.parametrize("shape", [(3, 13, 37), (9, 8, 37)], ids=lambda s: "N%d-P%d-A%d" % s)
def test_a_nan_sample_leaves_its_neighbours_alone(hip_lib, shape):
    cs, st = _samples(*shape)
    clean = _batched(cs, st)
    bad = {k: v.clone() for k, v in st.items()}
    for k in ("feat", "U", "offsets", "ref"):
        bad[k][1] = float("nan")
    got = _batched(cs, bad)
    for b in (0, 2):
        assert torch.equal(got[b], clean[b]) and bool(torch.isfinite(got[b]).all())


# ------------------------------------------------------------------------------------------------ 4. row-strided operands
def _strided(st, A, P, k):
    """U and the offsets as column blocks of ONE (B*A, J + 1 + 3P + k) buffer whose gaps hold NaN."""
    J = st["U"].shape[-1]
    buf = torch.full((B3 * A, J + 1 + 3 * P + k), float("nan"))
    buf[:, :J], buf[:, J + 1:J + 1 + 3 * P] = st["U"].reshape(B3 * A, J), st["offsets"].reshape(B3 * A, 3 * P)
    buf = buf.to(DEV).view(B3, A, -1)
    return buf[:, :, :J], buf[:, :, J + 1:J + 1 + 3 * P]


@pytest.mark.parametrize("shape", [(3, 13, 37), (9, 8, 37)], ids=lambda s: "N%d-P%d-A%d" % s)
def test_row_strided_operands(hip_lib, shape):
    from far3d_amd import lib, ops
    cs, st = _samples(*shape)
    N, P, A = shape
    J = st["U"].shape[-1]
    k = 4 + (-(J + 1 + 3 * P)) % 4                 # a trailing gap too, and a row stride that is a multiple of 4 floats
    feat, ref, l2i, Vc = (_dev(st[n]) for n in ("feat", "ref", "lidar2img", "Vc"))
    U, offs = _strided(st, A, P, k)
    assert U.stride(1) % 4 == 0 and not U.is_contiguous()
    assert torch.equal(ops.aggregate_batched(feat, ref, offs, l2i, U, Vc, *_geom(cs[0]), num_groups=8), _batched(cs, st))
    # a row stride that is no multiple of 4 floats: refused, as in the one-sample entry
    U, offs = _strided(st, A, P, k + 1)
    with pytest.raises(lib.Far3dHipError, match="ldU=%d" % U.stride(1)):
        ops.aggregate_batched(feat, ref, offs, l2i, U, Vc, *_geom(cs[0]), num_groups=8)
    with pytest.raises(lib.Far3dHipError, match="ldU=%d" % U.stride(1)):
        ops.aggregate_forward(feat[0], ref[0], offs[0], l2i[0], U[0], Vc[0], *_geom(cs[0]), num_groups=8)


# ------------------------------------------------------------------------------------------------ 5. nothing is written outside `out`
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["out_f32", "out_bf16"])
@pytest.mark.parametrize("shape", [(3, 13, 37), (9, 8, 37)], ids=lambda s: "N%d-P%d-A%d" % s)
def test_nothing_is_written_outside_out(hip_lib, shape, out_dtype):
    cs, st = _samples(*shape)
    A, guard = shape[2], 64
    big = torch.full((guard + B3 * A + guard, 256), 7.0, dtype=out_dtype, device=DEV)
    out = big[guard:guard + B3 * A].view(B3, A, 256)
    got = _batched(cs, st, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((big[:guard] == 7.0).all()) and bool((big[guard + B3 * A:] == 7.0).all())
    assert torch.equal(out, _batched(cs, st, out_dtype=out_dtype))


# ------------------------------------------------------------------------------------------------ 6. refusals launch nothing
GOOD = dict(B=2, A=5, N=3, S=128, C=256, G=8, P=4, L=4, Vc=True)
REFUSED = [(dict(C=128), "C=128"), (dict(G=4), "G=4"), (dict(N=17), "N=17"), (dict(L=5), "L=5"), (dict(N=8, P=13), "N*P*L=416"),
           (dict(B=-1), "B=-1"), (dict(N=9, Vc=False), "N=9")]


def _raw_call(hip_lib, s, src, tables, out):
    hw = (ctypes.c_int32 * 16)(8, 12, 4, 6, 2, 3, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1)
    starts = (ctypes.c_int32 * 8)(0, 96, 120, 126, 127, 127, 127, 127)
    pc = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return hip_lib.far3d_aggregate_batched(p(src), 0, p(src), p(src), p(src), p(src), p(src) if s["Vc"] else None, p(tables), p(out), 0,
                                           s["B"], s["A"], s["N"], s["S"], s["C"], s["G"], s["P"], s["L"], vp(hw), vp(starts), vp(pc),
                                           64.0, 96.0, 0, 0, None)


@pytest.mark.parametrize("bad,named", REFUSED, ids=[n for _, n in REFUSED])
def test_refused_sizes_launch_nothing(hip_lib, bad, named):
    """FAR3D_ERR_ARG with the offending size in the message, every output byte kept, and the next good call works."""
    s = dict(GOOD)
    s.update(bad)
    src = torch.zeros(1 << 20, device=DEV)                      # more floats than any operand of these sizes
    tables = torch.ones(1 << 16, device=DEV)
    out = torch.full((1 << 16,), 7.0, device=DEV)
    st = _raw_call(hip_lib, s, src, tables, out)
    msg = hip_lib.far3d_last_error().decode()
    assert st == -1, (st, msg)
    assert "far3d_aggregate_batched" in msg and named in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    cs, stk = _samples(3, 4, 5)
    assert torch.equal(_batched(cs, stk)[1], _single(cs[1]))


@pytest.mark.parametrize("empty", [dict(B=0), dict(A=0)], ids=["B0", "A0"])
def test_empty_batch_is_ok_and_launches_nothing(hip_lib, empty):
    s = dict(GOOD)
    s.update(empty)
    src, tables = torch.zeros(1 << 20, device=DEV), torch.ones(1 << 16, device=DEV)
    out = torch.full((1 << 16,), 7.0, device=DEV)
    assert _raw_call(hip_lib, s, src, tables, out) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 7. the module
def _counted(monkeypatch):
    from far3d_amd import ops
    calls, real = [], ops.aggregate_general

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(ops, "aggregate_general", counting)
    return calls


def test_module_family_shape_two_samples(hip_lib, monkeypatch):
    """256 / 8 / 4 levels / 3 cameras / 13 points, bs = 2, A = 50, fp32: the module == the op sequence called directly (the batched
    linears, ops.aggregate_batched, the output projection), within 2e-4 of the float64 restatement of the reference forward, and the
    general path is not taken.  (No bit equality between bs = 2 and bs = 1 is asked of the module: the linears may pick different tiles
    for different row counts.)"""
    from far3d_amd import ops
    m, g = _module(256, 8, 4, 3, 13, seed=31)
    i = _module_inputs(g, bs=2, A=50, C=256, N=3, L=4)
    with torch.no_grad():
        want64 = _reference_forward(m, i)
    m = m.to(DEV)
    calls = _counted(monkeypatch)
    got = _call(m, i)
    assert got.shape == (2, 50, 256) and not calls
    P = m._pack(torch.device(DEV))
    xd, qd, l2i = i["x"].to(DEV), i["qpos"].to(DEV), i["l2i"].to(DEV).float().contiguous()
    x, xq = xd.float().reshape(100, 256).contiguous(), (xd + qd).float().reshape(100, 256).contiguous()
    ce = ops.linear(ops.linear(l2i[:, :, :3, :].reshape(6, 12).contiguous(), P["ce0"], act="relu"), P["ce2"], act="relu")
    ce = ops.layernorm(ce, *P["ce_ln"])
    Vc, U, offs = ops.linear(ce, P["wfc_full"]), ops.linear(xq, P["wfc"]), ops.linear(x, P["lfc"])
    hw = [tuple(int(v) for v in r) for r in i["shapes"].tolist()]
    agg = ops.aggregate_batched(i["feat"].to(DEV).contiguous(), i["ref"].to(DEV).float().contiguous(), offs.view(2, 50, -1), l2i,
                                U.view(2, 50, -1), Vc.view(2, 3, -1), hw, [int(v) for v in i["starts"].tolist()],
                                [float(v) for v in i["pc"].tolist()], (64, 96), num_groups=8)
    want = ops.linear(agg.view(100, 256), P["oproj"], res=x).view(2, 50, 256)
    assert torch.equal(got, want)
    err = (got.cpu().double() - want64).abs().max().item()
    print("module 256/8/4/3/13, bs 2: max abs err vs float64 reference %.3e (bar 2e-4)" % err)
    assert err < 2e-4


def test_module_outside_the_family_keeps_the_general_path(hip_lib, monkeypatch):
    m, g = _module(128, 4, 3, 2, 5, seed=32)
    i = _module_inputs(g, bs=2, A=23, C=128, N=2, L=3)
    m = m.to(DEV)
    calls = _counted(monkeypatch)
    assert _call(m, i).shape == (2, 23, 128) and len(calls) == 1

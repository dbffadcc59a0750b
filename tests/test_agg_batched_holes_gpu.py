"""GPU: far3d_aggregate_batched_holes (ops.aggregate_batched(..., hole=)) -- the batched fused aggregation with a hole of unused query
rows per sample.

The contract is bitwise, so every bar is torch.equal: a hole row of out[b] is an exact zero row and none of its operands is read; every
other row has the bits of the call without a hole; out[b] as a whole is far3d_aggregate_forward on sample b with the perm of
far3d_agg_order for that sample's count.  Three samples whose counts give a whole hole, a part of one and none.

Inputs and helpers: tests/test_agg_batched_gpu.py's (cases.aggregate_case, one seed per sample)."""
import ctypes

import pytest
import torch

from tests.test_agg_batched_gpu import B3, DEV, _batched, _dev, _geom, _samples, _single

pytestmark = pytest.mark.gpu

# (N, P, A), hole [start, end), counts per sample: what it hits
CASES = [((3, 13, 37), (10, 30), (0, 7, 20)),     # kernel 8, the P = 13 specialisation
         ((3, 4, 5), (1, 4), (0, 1, 3)),          # kernel 8 generic; fewer queries than XCD slots
         ((9, 8, 37), (10, 30), (0, 7, 20))]      # kernel 7
IDS = ["N%d-P%d-A%d" % c[0] for c in CASES]
DTYPES = [torch.float32, torch.bfloat16]
maps = pytest.mark.parametrize("feat_dtype", DTYPES, ids=["maps_f32", "maps_bf16"])
outs = pytest.mark.parametrize("out_dtype", DTYPES, ids=["out_f32", "out_bf16"])
shapes = pytest.mark.parametrize("case", CASES, ids=IDS)


def _counts(cnt):
    return torch.tensor(list(cnt), dtype=torch.int32, device=DEV)


def _hole_mask(A, span, cnt):
    """(B, A) bool: True where sample b's row holds no query."""
    m = torch.zeros((len(cnt), A), dtype=torch.bool)
    for b, c in enumerate(cnt):
        m[b, span[0] + c:span[1]] = True
    return m.to(DEV)


@outs
@maps
@shapes
def test_hole_rows_are_zero_and_the_others_keep_their_bits(hip_lib, case, feat_dtype, out_dtype):
    shape, span, cnt = case
    cs, st = _samples(*shape)
    plain = _batched(cs, st, feat_dtype=feat_dtype, out_dtype=out_dtype)
    got = _batched(cs, st, feat_dtype=feat_dtype, out_dtype=out_dtype, hole=(_counts(cnt), *span))
    assert got.shape == plain.shape and got.dtype == out_dtype
    hole = _hole_mask(shape[2], span, cnt)
    assert int(hole[0].sum()) == span[1] - span[0] and int(hole[2].sum()) == 0 and 0 < int(hole[1].sum()) < span[1] - span[0]
    assert bool((got[hole] == 0).all()) and plain[hole].float().abs().sum().item() > 0      # the rows would not be zero by themselves
    assert torch.equal(got[~hole], plain[~hole])


@outs
@maps
@shapes
def test_each_sample_is_the_one_sample_launch_with_the_orders_perm(hip_lib, case, feat_dtype, out_dtype):
    from far3d_amd import ops
    shape, span, cnt = case
    cs, st = _samples(*shape)
    counts = _counts(cnt)
    got = _batched(cs, st, feat_dtype=feat_dtype, out_dtype=out_dtype, hole=(counts, *span))
    for b, c in enumerate(cs):
        perm = ops.aggregation_order(_dev(c["ref"]), _dev(c["lidar2img"]), c["pc_range"], c["pad_hw"], hole=(counts[b:b + 1], *span))
        assert int((perm < 0).sum()) == span[1] - span[0] - cnt[b]
        one = _single(c, feat_dtype, out_dtype=out_dtype, perm=perm)
        assert torch.equal(got[b], one), "sample %d differs from its one-sample launch" % b
        # a batch of one, with that sample's count alone: the result depends neither on B nor on the other samples' counts
        alone = _batched(cs, st, slice(b, b + 1), feat_dtype, out_dtype=out_dtype, hole=(counts[b:b + 1].clone(), *span))
        assert torch.equal(alone[0], one)
    assert torch.equal(_batched(cs, st, feat_dtype=feat_dtype, out_dtype=out_dtype, hole=(counts, *span)), got)   # the same from run to run


@shapes
def test_nan_in_the_hole_rows_changes_nothing(hip_lib, case):
    shape, span, cnt = case
    cs, st = _samples(*shape)
    hole = _hole_mask(shape[2], span, cnt).cpu()
    clean = _batched(cs, st, hole=(_counts(cnt), *span))
    bad = {k: v.clone() for k, v in st.items()}
    for k in ("ref", "offsets", "U"):
        bad[k][hole] = float("nan")
    got = _batched(cs, bad, hole=(_counts(cnt), *span))
    assert bool(torch.isfinite(got).all()) and torch.equal(got, clean)
    assert bool((got[hole.to(DEV)] == 0).all())


def test_a_count_out_of_range_is_clamped(hip_lib):
    """Counts below 0 and above end - start behave as 0 and end - start (the proposal kernels never write one)."""
    shape, span, _ = CASES[0]
    cs, st = _samples(*shape)
    got = _batched(cs, st, hole=(_counts((-5, 7, 1000)), *span))
    assert torch.equal(got, _batched(cs, st, hole=(_counts((0, 7, span[1] - span[0])), *span)))


@outs
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_without_a_hole_it_is_todays_call_and_nothing_is_written_outside_out(hip_lib, case, out_dtype):
    shape, span, cnt = case
    cs, st = _samples(*shape)
    A, guard = shape[2], 64
    assert torch.equal(_batched(cs, st, out_dtype=out_dtype, hole=None), _batched(cs, st, out_dtype=out_dtype))
    big = torch.full((guard + B3 * A + guard, 256), 7.0, dtype=out_dtype, device=DEV)
    out = big[guard:guard + B3 * A].view(B3, A, 256)
    got = _batched(cs, st, out=out, hole=(_counts(cnt), *span))
    assert got.data_ptr() == out.data_ptr()
    assert bool((big[:guard] == 7.0).all()) and bool((big[guard + B3 * A:] == 7.0).all())
    assert torch.equal(out, _batched(cs, st, out_dtype=out_dtype, hole=(_counts(cnt), *span)))


def _raw_holes(hip_lib, B, A, counts, start, end, src, tables, out):
    """far3d_aggregate_batched_holes at N = 3, P = 4 (kernel 8) on zero operands, the hole passed as given; NULL count: `counts` None."""
    hw = (ctypes.c_int32 * 16)(8, 12, 4, 6, 2, 3, 1, 2, 1, 1, 1, 1, 1, 1, 1, 1)
    starts = (ctypes.c_int32 * 8)(0, 96, 120, 126, 127, 127, 127, 127)
    pc = (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return hip_lib.far3d_aggregate_batched_holes(p(src), 0, p(src), p(src), p(src), p(src), p(src), p(tables), p(out), 0, B, A, 3, 128, 256, 8, 4,
                                                 4, vp(hw), vp(starts), vp(pc), 64.0, 96.0, 0, 0, p(counts) if counts is not None else None,
                                                 start, end, None)


@pytest.mark.parametrize("start,end", [(1, 6), (-1, 4), (4, 1)], ids=["end_above_A", "negative_start", "start_above_end"])
def test_a_bad_hole_is_refused_and_launches_nothing(hip_lib, start, end):
    src, tables = torch.zeros(1 << 20, device=DEV), torch.ones(1 << 16, device=DEV)
    out = torch.full((1 << 16,), 7.0, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    rc = _raw_holes(hip_lib, 2, 5, counts, start, end, src, tables, out)
    msg = hip_lib.far3d_last_error().decode()
    assert rc == -1, (rc, msg)
    assert "far3d_aggregate_batched_holes" in msg and "hole" in msg, msg
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # without a count the same numbers mean nothing: the call is far3d_aggregate_batched's
    assert _raw_holes(hip_lib, 2, 5, None, start, end, src, tables, out) == 0
    torch.cuda.synchronize()
    assert bool((out[:2 * 5 * 256] != 7.0).all()) and bool((out[2 * 5 * 256:] == 7.0).all())


def test_counts_of_the_wrong_length_are_refused_and_launch_nothing(hip_lib):
    shape, span, cnt = CASES[1]
    cs, st = _samples(*shape)
    out = torch.full((B3, shape[2], 256), 7.0, device=DEV)
    for bad in (_counts(cnt[:2]), _counts(cnt).long(), _counts(cnt).cpu()):
        with pytest.raises(ValueError, match="one count per sample"):
            _batched(cs, st, out=out, hole=(bad, *span))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert torch.equal(_batched(cs, st, out=out, hole=(_counts(cnt), *span))[2], _single(cs[2]))

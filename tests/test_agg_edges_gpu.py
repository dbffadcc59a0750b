"""GPU: the aggregation kernels and far3d_msda_forward against the float64 reference on the designed inputs of tests/agg_edge_cases.py:
exact token centres and band edges, the two sides of the patch / per-corner decision, queries that every camera sees (list flushes, the
sorted mode's third-camera arm, sibling workgroups), kernel 8's shape limits, points at and behind the z clamp beside visible ones, and
logits whose spread makes softmax factors underflow -- in a geometry where every position is exact in float32 and in one where it is an
ulp off.  tests/test_agg_edges_cpu.py shows that the cases are what they claim.

Forms, fp32 and bf16 maps each (bf16: the reference runs on the bf16-rounded maps), every shape a form accepts: far3d_aggregate_forward
variants 0, 3, 7, 11, 12; variant 8 with the order of far3d_agg_order; the sorted mode (bit-identical to that call); variant 9 with a
sibling slot for every row (unsplit rows bit-identical to variant 8, tickets back at zero, an all_cameras row marked); far3d_aggregate_batched
with the case and its row-reversed twin as two samples (bit-identical to the one-sample launches); the general path agg_operands ->
msda_forward -> camera_sum; far3d_msda_forward on its own edge locations.

Bar: max |got - float64| < 2e-5 over the FULL tensors, nothing excluded -- the bar tests/test_sampling_gpu.py holds this arithmetic to on
small cases with outputs of size about 1 (here at most 1.6).  The float32 restatements of the reference are 1e-7 .. 1.2e-6 from float64 on
these inputs (asserted < 2e-6 in the CPU test), so the bar leaves a factor of 10 .. 100 for reassociation, the v_rcp projection and the exp2
softmax, while a wrong corner, token, weight row or a dropped item moves an element by 1e-2 or more.  In the dyadic geometry the rows
designed to be zero must be exactly zero.

Worst errors of one MI355X run (the tests print one figure per case, form and dtype; all cases, fp32 and bf16 maps): variant 0 1.3e-6,
variant 3 1.1e-6, variants 7 and 11 1.1e-6, variant 12 1.4e-6, variant 8 in far3d_agg_order's order and the sorted mode 1.3e-6, variant 9
1.4e-6 (19 of 25 rows split), the batched launch 1.3e-6, aggregate_general 1.1e-6, far3d_msda_forward 1.0e-6; 0 where one camera and one
point make the arithmetic exact.  No form came closer to the bar than a factor of 14, and no kernel had to change."""
import functools

import pytest
import torch

from tests import agg_edge_cases as ec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR = 2e-5
CASES = [(g, s) for g in ec.GEOMETRIES for s in ec.SHAPES]
K8_CASES = [(g, s) for g, s in CASES if ec.kernel8_shape(s)]
DTYPES = [torch.float32, torch.bfloat16]
VARIANT_CASES = [(g, s, v) for g, s in CASES for v in (0, 3, 7, 11, 12) if v != 12 or ec.kernel8_shape(s)]      # 12 is kernel 8 only


def _cid(g, s):
    return "%s-N%d-P%d-L%d" % ((g,) + tuple(s))


def _dt(d):
    return "maps_f32" if d == torch.float32 else "maps_bf16"


@functools.lru_cache(maxsize=None)
def _operands(geom, shape, dtype):
    """The case's operands on the device (never modified): feat, ref, offsets (A, 3P), lidar2img, U, Vc, and the geometry arguments."""
    c = ec.case(geom, shape)
    d = lambda t: t.to(DEV).contiguous()
    A = c["ref"].shape[0]
    return (d(c["feat"].to(dtype)), d(c["ref"]), d(c["offsets"].reshape(A, -1)), d(c["lidar2img"]), d(c["U"]), d(c["Vc"])), \
        (c["level_hw"], c["level_start"], c["pc_range"], c["pad_hw"])


def _check(got, geom, shape, dtype, form, reversed_rows=False):
    want = ec.reference(geom, shape, dtype == torch.bfloat16)
    want = want.flip(0) if reversed_rows else want
    got = got.detach().double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    err = (got - want).abs().max().item()
    print("%s %s %s: max |got - float64| %.3e (bar %.0e, max |out| %.2f)" % (_cid(geom, shape), form, _dt(dtype), err, BAR, want.abs().max().item()))
    assert err < BAR, (form, err)
    if geom == "dyadic":      # the positions are exact: a point on the edge of a map contributes exactly nothing
        zero = want.abs().amax(1) == 0
        assert int(zero.sum()) >= 1 and got[zero].abs().max().item() == 0.0
    return err


# ------------------------------------------------------------------------------------------------ the kernel variants
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("geom,shape,variant", VARIANT_CASES, ids=["%s-v%d" % (_cid(g, s), v) for g, s, v in VARIANT_CASES])
def test_variants_against_float64(hip_lib, geom, shape, variant, dtype):
    """Variant 0 is kernel 8 on its shapes and kernel 7 beyond them; 12 is kernel 8 with the greedy dealing."""
    from far3d_amd import ops
    (feat, ref, offs, l2i, U, Vc), geo = _operands(geom, shape, dtype)
    got = ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, *geo, num_groups=ec.G, variant=variant)
    _check(got, geom, shape, dtype, "variant %d" % variant)
    again = ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, *geo, num_groups=ec.G, variant=variant)
    assert torch.equal(again, got)


# ------------------------------------------------------------------------------------------------ far3d_agg_order: variant 8 and the sorted mode
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("geom,shape", K8_CASES, ids=[_cid(g, s) for g, s in K8_CASES])
def test_ordered_and_sorted_mode(hip_lib, geom, shape, dtype):
    """Variant 8 in the order of far3d_agg_order; the sorted mode (operands stored through inv, qbase) is the same call bit for bit.  The
    all_cameras rows have more cameras than the hint's two: their other cameras take the arm that forms the weights inside the item loop."""
    from far3d_amd import ops
    from far3d_amd.lib import Far3dHipError
    (feat, ref, offs, l2i, U, Vc), geo = _operands(geom, shape, dtype)
    hw, starts, pc, pad = geo
    A = ref.shape[0]
    tab = ops.agg_tables(Vc)
    perm = ops.aggregation_order(ref, l2i, pc, pad)
    assert sorted(perm.cpu().tolist()) == list(range(A))
    base = ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, *geo, num_groups=ec.G, perm=perm, variant=8, tables=tab)
    _check(base, geom, shape, dtype, "variant 8 + order")
    perm, (inv, qbase) = ops.aggregation_order(ref, l2i, pc, pad, sorted_operands=True)
    pm, iv = perm.cpu().long(), inv.cpu().long()
    assert torch.equal(pm[iv], torch.arange(A)), "perm[inv[a]] names row a"
    Us, Os = torch.full_like(U, float("nan")), torch.full_like(offs, float("nan"))
    Us[inv.long()], Os[inv.long()] = U, offs
    run = lambda: ops.aggregate_forward(feat, ref, Os, l2i, Us, Vc, *geo, num_groups=ec.G, perm=perm, tables=tab, qbase=qbase)
    assert ops.aggregate_sorted_applies(*shape) == ec.sorted_mode_shape(shape)
    if not ec.sorted_mode_shape(shape):       # L * P * 2 > 104 float4 per hinted camera row: the library refuses the call
        with pytest.raises(Far3dHipError, match="sorted mode"):
            run()
        return
    unsorted = ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, *geo, num_groups=ec.G, perm=perm, variant=8, tables=tab)
    got = run()
    _check(got, geom, shape, dtype, "sorted mode")
    assert torch.equal(got, unsorted), "sorted mode differs from the unsorted variant-8 call"
    assert torch.equal(run(), got)
    c = ec.case(geom, shape)
    if shape[0] >= 3 and "all_cameras" in c["family"]:
        hint = int(qbase.cpu().view(torch.int32)[:, 3][iv][ec.rows_of(c, "all_cameras")[0]])
        assert (hint & 0xff) != ((hint >> 8) & 0xff), "two hinted cameras: the row's other cameras form their weights in the item loop"


def test_sorted_gate_at_l4_p14(hip_lib):
    """N = 2, P = 14, L = 4 (L * P = 56 > 52) is kernel 8's shape but not the sorted mode's: the library refuses a forced qbase, and
    ops.aggregate_sorted_applies -- the gate the engine asks -- says no for the same shape, so the engine never forces it."""
    from far3d_amd import ops
    from far3d_amd.lib import Far3dHipError
    shape = (2, 14, 4)
    (feat, ref, offs, l2i, U, Vc), geo = _operands("dyadic", shape, torch.float32)
    perm, (inv, qbase) = ops.aggregation_order(ref, l2i, geo[2], geo[3], sorted_operands=True)
    with pytest.raises(Far3dHipError, match="sorted mode"):
        ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, *geo, num_groups=ec.G, perm=perm, qbase=qbase)
    assert ops.aggregate_kernel8_applies(*shape) and not ops.aggregate_sorted_applies(*shape)
    _check(ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, *geo, num_groups=ec.G, perm=perm), "dyadic", shape, torch.float32, "variant 0 unsorted")


# ------------------------------------------------------------------------------------------------ variant 9: sibling workgroups
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("geom,shape", K8_CASES, ids=[_cid(g, s) for g, s in K8_CASES])
def test_sibling_workgroups(hip_lib, geom, shape, dtype):
    from far3d_amd import ops
    (feat, ref, offs, l2i, U, Vc), geo = _operands(geom, shape, dtype)
    hw, starts, pc, pad = geo
    c = ec.case(geom, shape)
    A = ref.shape[0]
    tab = ops.agg_tables(Vc)
    base = ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, *geo, num_groups=ec.G, perm=ops.aggregation_order(ref, l2i, pc, pad), variant=8, tables=tab)
    sp = ops.AggSplit(A, A, DEV)
    perm = ops.aggregation_order(ref, l2i, pc, pad, split=sp)
    pm = perm.cpu().numpy()
    main, sib = pm[:A], pm[A:]
    assert sorted((main & 0x1fffffff).tolist()) == list(range(A))
    marked = sorted((main[(main & (1 << 29)) != 0] & 0x1fffffff).tolist())
    used = sib[sib != 0x7fffffff]
    assert sorted((used & 0x1fffffff).tolist()) == marked, "every marked query has exactly one sibling entry"
    if shape[0] >= 2 and "all_cameras" in c["family"]:
        assert set(ec.rows_of(c, "all_cameras")) <= set(marked), "a query every camera sees is a heavy one"
    if shape[0] == 1:
        assert marked == []
    run = lambda: ops.aggregate_forward(feat, ref, offs, l2i, U, Vc, *geo, num_groups=ec.G, perm=perm, tables=tab, split=sp)
    got = run()
    _check(got, geom, shape, dtype, "variant 9 (%d of %d rows split)" % (len(marked), A))
    unsplit = torch.ones(A, dtype=torch.bool)
    unsplit[marked] = False
    assert torch.equal(got[unsplit.to(DEV)], base[unsplit.to(DEV)]), "rows without a sibling take variant 8's path bit for bit"
    assert int(sp.tickets.abs().sum()) == 0
    assert torch.equal(run(), got) and int(sp.tickets.abs().sum()) == 0


# ------------------------------------------------------------------------------------------------ far3d_aggregate_batched
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("geom,shape", CASES, ids=[_cid(g, s) for g, s in CASES])
def test_batched_two_samples(hip_lib, geom, shape, dtype):
    """Sample 0 is the case, sample 1 the case with its rows reversed (same maps and cameras)."""
    from far3d_amd import ops
    (feat, ref, offs, l2i, U, Vc), geo = _operands(geom, shape, dtype)
    two = lambda t: torch.stack([t, t])
    rev = lambda t: torch.stack([t, t.flip(0)])
    got = ops.aggregate_batched(torch.cat([feat, feat]), rev(ref), rev(offs), two(l2i), rev(U), two(Vc), *geo, num_groups=ec.G)
    _check(got[0], geom, shape, dtype, "batched sample 0")
    _check(got[1], geom, shape, dtype, "batched sample 1 (rows reversed)", reversed_rows=True)
    one = [ops.aggregate_forward(feat, r, o, l2i, u, Vc, *geo, num_groups=ec.G) for r, o, u in ((ref, offs, U), (ref.flip(0), offs.flip(0), U.flip(0)))]
    for b in range(2):
        assert torch.equal(got[b], one[b]), "sample %d differs from its one-sample launch" % b


# ------------------------------------------------------------------------------------------------ the general path
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("geom", list(ec.GEOMETRIES))
@pytest.mark.parametrize("shape", [(9, 13, 3), (16, 6, 4), (7, 13, 4)], ids=lambda s: "N%d-P%d-L%d" % s)
def test_general_path(hip_lib, geom, shape, dtype):
    """far3d_agg_operands -> far3d_msda_forward -> far3d_camera_sum on the two shapes beyond kernel 8 and on the model's."""
    from far3d_amd import ops
    (feat, ref, offs, l2i, U, Vc), geo = _operands(geom, shape, dtype)
    got = ops.aggregate_general(feat, ref, offs, l2i, U, Vc, *geo, ec.G)
    assert got.shape[0] == 1
    _check(got[0], geom, shape, dtype, "aggregate_general")


# ------------------------------------------------------------------------------------------------ far3d_msda_forward
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: "values_f32" if d == torch.float32 else "values_bf16")
@pytest.mark.parametrize("name", list(ec.MSDA))
def test_msda_on_edge_locations(hip_lib, name, dtype):
    from far3d_amd import ops
    c = ec.msda_case(name)
    want = ec.msda_reference(name, dtype == torch.bfloat16)
    got = ops.msda_forward(c["value"].to(dtype).to(DEV), c["shapes"].to(DEV), c["lsi"].to(DEV), c["loc"].to(DEV), c["w"].to(DEV)).double().cpu()
    assert got.shape == want.shape
    err = (got - want).abs().max().item()
    print("msda %s %s: max |got - float64| %.3e (bar %.0e, max |out| %.2f)" % (name, dtype, err, BAR, want.abs().max().item()))
    assert err < BAR

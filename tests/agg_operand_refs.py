"""Float64 restatement and error bounds for far3d_agg_operands (csrc/agg_operands.hip), shared by tests/test_agg_operands_cpu.py and
tests/test_agg_operands_gpu.py.

operands_ref is the reference module's own text with a batch dimension: oracle.sampling.project_points for the locations
(detr3d_transformer.py:547-552) and the two weight lines of oracle.sampling.aggregation_ref (:540-542).  Inputs are float32 values (the
pc_range list is rounded to float32 first, as the kernel receives it), evaluated in `dtype`.

Locations, per element.  u = 2^-24.  Every key-point component k goes through 4 float32 roundings -- hi - lo, ref * (hi - lo), + lo,
+ offset -- of quantities no larger than mag_k = |ref| |hi - lo| + |lo| + |offset| (mag_3 = 1 for the homogeneous one, which is exact).
Row r of the projection adds the rounding of its 3 products and of its 3 additions; with S_r = sum_k |M[r,k]| mag_k the products'
roundings sum to at most 1 u S_r and every partial sum is at most S_r, so |dx| <= (4 + 1 + 3) u S_x and |dz| <= 8 u S_z.  The division by
zc and the division by the padded size round once each, relative to |x / zc| <= S_x / zc.  To first order

    |d loc| <= c u (S_x / zc + |x| S_z / zc^2) / pad,      c = 4 + 1 + 3 + 1 + 1 = 10 roundings

(a fused multiply-add only removes roundings from the count).  The first-order form holds while |dz| << zc; an element whose float64 z
lies within c u S_z of the clamp value 1e-5 may take the other side of fmaxf and is left out (LOC_EXCLUDE_CAP: at most 1 in 1000), and the
CPU test asserts that on every input used here no element lies within 100 x that margin, so nothing is left out in practice and the
second-order term stays below 1 % of the z term.

Weights: tests.head_refs.chain_bound (a chain through expf) with the float32 torch restatement's own distance from float64 on the same
inputs as the yardstick.  The sum of a (b, a, g) row of N L P weights is held to the same rule with its own yardstick: chain_bound of the
float32 restatement's largest |row sum - 1| (the sums taken in float64) around the value 1, i.e. 4 x that distance + 2 ulp of 1."""
import functools

import torch

from far3d_amd import synth
from oracle import sampling
from tests import cases
from tests.head_refs import chain_bound

LOC_ROUNDINGS = 10
LOC_EXCLUDE_CAP = 1e-3
U24 = 2.0 ** -24


def operands_ref(c, dtype=torch.float64):
    """c: an operand case (operand_case / from_aggregate_case).  -> (loc (B*N,A,G,L,P,2), weights (B*N,A,G,L*P), key_points (B,A,P,3))."""
    B, N, A, G, L, P = c["dims"]
    ref, offs, l2i, U, Vc = (c[k].to(dtype) for k in ("ref", "offsets", "lidar2img", "U", "Vc"))
    pc = torch.tensor(c["pc_range"], dtype=torch.float32).to(dtype)
    ref_m = ref * (pc[3:6] - pc[0:3]) + pc[0:3]
    key_points = ref_m[:, :, None, :] + offs
    p2d = sampling.project_points(key_points, l2i, c["pad_hw"]).flatten(end_dim=1)             # (B*N,A,P,2)
    loc = p2d[:, :, None, None, :, :].repeat(1, 1, G, L, 1, 1)
    logits = U[:, :, None, :] + Vc[:, None, :, :]                                               # (B,A,N,J)
    w = logits.reshape(B, A, -1, G).softmax(dim=-2)
    w = w.reshape(B, A, N, -1, G).permute(0, 2, 1, 4, 3).contiguous().flatten(end_dim=1)        # (B*N,A,G,L*P)
    return loc, w, key_points


def loc_bound(c):
    """-> (bound (B*N,A,P,2) float64 per compact location element, margin (B*N,A,P) = c u S_z, z (B*N,A,P) float64)."""
    B, N, A, G, L, P = c["dims"]
    ref, offs, M = c["ref"].double(), c["offsets"].double(), c["lidar2img"].double()
    pc = torch.tensor(c["pc_range"], dtype=torch.float32).double()
    kp = (ref * (pc[3:6] - pc[0:3]) + pc[0:3])[:, :, None, :] + offs                                              # (B,A,P,3)
    mag = (ref.abs() * (pc[3:6] - pc[0:3]).abs() + pc[0:3].abs())[:, :, None, :] + offs.abs()
    kp1 = torch.cat([kp, torch.ones_like(kp[..., :1])], -1)
    mag1 = torch.cat([mag, torch.ones_like(mag[..., :1])], -1)
    xyz = torch.einsum("bnrk,bapk->bnapr", M[:, :, :3, :], kp1)                                                    # (B,N,A,P,3)
    S = torch.einsum("bnrk,bapk->bnapr", M[:, :, :3, :].abs(), mag1)
    zc = xyz[..., 2].clamp(min=1e-5)
    pad = torch.tensor([c["pad_hw"][1], c["pad_hw"][0]], dtype=torch.float64)
    b = LOC_ROUNDINGS * U24 * (S[..., :2] / zc[..., None] + xyz[..., :2].abs() * S[..., 2:3] / zc[..., None] ** 2) / pad
    return b.flatten(end_dim=1), (LOC_ROUNDINGS * U24 * S[..., 2]).flatten(end_dim=1), xyz[..., 2].flatten(end_dim=1)


def check_locations(got, c, what):
    """got: compact locations (B*N,A,P,2), any float dtype, on the CPU.  Asserts the per-element bound outside the excluded elements and
    the cap on those; returns (fraction excluded, largest error / bound)."""
    loc64 = reference(c["name"])[0][:, :, 0, 0]
    bound, margin, z = loc_bound(c)
    keep = (z - 1e-5).abs() > margin
    frac = 1.0 - keep.double().mean().item()
    assert frac <= LOC_EXCLUDE_CAP, "%s: %.2e of the elements lie at the clamp" % (what, frac)
    ratio = ((got.double() - loc64).abs() / bound)[keep]
    worst = ratio.max().item() if ratio.numel() else 0.0
    print("%s: locations: worst error / bound %.3f, %.2e excluded" % (what, worst, frac))
    assert worst <= 1.0, "%s: location error is %.3f x the bound" % (what, worst)
    return frac, worst


def check_key_points(got, c, what):
    """got (B,A,P,3) on the CPU: 4 roundings of quantities no larger than mag (module docstring)."""
    ref, offs = c["ref"].double(), c["offsets"].double()
    pc = torch.tensor(c["pc_range"], dtype=torch.float32).double()
    mag = (ref.abs() * (pc[3:6] - pc[0:3]).abs() + pc[0:3].abs())[:, :, None, :] + offs.abs()
    ratio = ((got.double() - reference(c["name"])[2]).abs() / (4 * U24 * mag)).max().item()
    print("%s: key points: worst error / bound %.3f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def _row_sums(w, c):
    B, N, A, G, L, P = c["dims"]
    return w.double().reshape(B, N, A, G, L * P).sum(dim=(1, 4))


def weight_bounds(c):
    """-> (element bound, row-sum bound), both chain_bound with the float32 torch restatement's own error as the yardstick."""
    w64 = reference(c["name"])[1]
    w32 = operands_ref(c, torch.float32)[1]
    one = torch.ones(1, dtype=torch.float64)
    return (chain_bound((w32.double() - w64).abs().max().item(), w64),
            chain_bound((_row_sums(w32, c) - 1.0).abs().max().item(), one))


def check_weights(got, c, what):
    """got: weights (B*N,A,G,L*P) on the CPU.  The element bound, and every (b, a, g) row of N*L*P weights sums to 1 within the row bound."""
    w64 = reference(c["name"])[1]
    bound, row_bound = weight_bounds(c)
    err = (got.double() - w64).abs().max().item()
    off = (_row_sums(got, c) - 1.0).abs().max().item()
    print("%s: weights: max error %.3e (bound %.3e), row sums off by %.3e (bound %.3e)" % (what, err, bound, off, row_bound))
    assert err <= bound and off <= row_bound, (what, err, bound, off, row_bound)


# ------------------------------------------------------------------------------------------------ seeded inputs
def operand_case(name, B, N, A, G, L, P, seed, pad_hw=(64, 96), offset_std=4.0):
    """Batched operands of far3d_agg_operands.  Sample b sees the ring cameras rotated by b places, so the samples of a batch differ."""
    g = torch.Generator().manual_seed(seed)
    _, _, l2i = synth.ring_cameras(N, pad_hw)
    J = L * P * G
    return dict(name=name, dims=(B, N, A, G, L, P),
                ref=torch.rand(B, A, 3, generator=g), offsets=torch.randn(B, A, P, 3, generator=g) * offset_std,
                lidar2img=torch.stack([torch.roll(l2i, b, 0) for b in range(B)]).contiguous(),
                U=torch.randn(B, A, J, generator=g), Vc=torch.randn(B, N, J, generator=g),
                level_hw=synth.level_shapes(pad_hw, strides=[8 << i for i in range(L)]), pc_range=list(synth.PC_RANGE), pad_hw=tuple(pad_hw))


def from_aggregate_case(name, c):
    """tests.cases aggregate case (one sample) -> operand case with B = 1; the value maps stay in c["feat"]."""
    N, A, P, G, L = c["lidar2img"].shape[0], c["ref"].shape[0], c["offsets"].shape[1], c["G"], len(c["level_hw"])
    return dict(name=name, dims=(1, N, A, G, L, P), ref=c["ref"][None], offsets=c["offsets"][None], lidar2img=c["lidar2img"][None],
                U=c["U"][None], Vc=c["Vc"][None], level_hw=c["level_hw"], pc_range=c["pc_range"], pad_hw=c["pad_hw"])


def near_small_case(seed):
    """cases.near_aggregate_case(A=96) -- queries a few metres from the cameras, metre-scale offsets, points behind the cameras -- at 3
    cameras of a 64x96 image."""
    A = 96
    c = cases.aggregate_case(num_cams=3, pad_hw=(64, 96), A=A, seed=seed, offset_std=1.5)
    g = torch.Generator().manual_seed(seed + 77)
    c["ref"] = 0.5 + (torch.rand(A, 3, generator=g) - 0.5) * torch.tensor([0.08, 0.08, 0.4])
    return c


# name -> builder.  The seeds are the first ones for which no float64 z lies within 100 x the exclusion margin of the clamp value
# (tests/test_agg_operands_cpu.py asserts it), so the exclusion rule is never what makes a comparison pass.
SEEDS = {"smallest": 0, "general": 0, "family": 0, "row320": 0, "row1088": 0, "groups3": 0, "unstaged": 0, "near": 963, "lds66k": 0, "unstaged1": 0, "staged16k": 0}
_BUILDERS = {
    "smallest": lambda s: operand_case("smallest", 1, 1, 1, 1, 1, 1, s),
    "general": lambda s: operand_case("general", 2, 2, 5, 4, 3, 5, s),
    "family": lambda s: from_aggregate_case("family", cases.small_aggregate_case(seed=s)),
    "row320": lambda s: operand_case("row320", 1, 5, 67, 8, 4, 16, s),                  # softmax row 320 > 256 threads
    "row1088": lambda s: operand_case("row1088", 1, 17, 9, 2, 4, 16, s),                # row 1088 > 1024, N beyond the fused family
    "groups3": lambda s: operand_case("groups3", 2, 3, 7, 3, 2, 7, s),                  # G no power of two (LDS-only reduction), J % 4 != 0
    "unstaged": lambda s: operand_case("unstaged", 1, 2, 2, 64, 8, 64, s),               # J = 32768 > 16384: no LDS transpose
    # with "unstaged", the shapes whose dynamic LDS exceeds 64 KiB, in ascending size (LDS_ASCENDING): 67072, 132608, 133120, 134144 bytes
    "lds66k": lambda s: operand_case("lds66k", 1, 1, 1, 16, 8, 64, s),                  # J = 8192, transposed
    "unstaged1": lambda s: operand_case("unstaged1", 1, 1, 2, 64, 8, 64, s),            # J = 32768, one camera
    "staged16k": lambda s: operand_case("staged16k", 1, 4, 1, 32, 8, 64, s),            # J = 16384: the largest transposed run
    "near": lambda s: from_aggregate_case("near", near_small_case(s)),
}
TABLE_CASES = ["smallest", "general", "family", "row320", "row1088"]      # the issue's table, in its order
LDS_ASCENDING = ["lds66k", "unstaged1", "unstaged", "staged16k"]
CASES = TABLE_CASES + ["groups3", "near"] + LDS_ASCENDING


@functools.lru_cache(maxsize=None)
def case(name):
    """The seeded inputs of a named case: built once, never modified."""
    return _BUILDERS[name](SEEDS[name])


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 (loc, weights, key_points) of a named case: computed once, shared, never modified."""
    return operands_ref(case(name))


def clamp_clearance(c):
    """min over the elements of |z - 1e-5| / (exclusion margin): the CPU test wants > 100."""
    _, margin, z = loc_bound(c)
    return ((z - 1e-5).abs() / margin).min().item()

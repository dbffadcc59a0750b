"""Designed inputs and the float64 reference for the edge tests of the aggregation kernels (far3d_aggregate_forward in all its forms,
far3d_aggregate_batched, the general path through far3d_agg_operands / far3d_msda_forward / far3d_camera_sum) and of far3d_msda_forward,
shared by tests/test_agg_edges_cpu.py and tests/test_agg_edges_gpu.py.

Geometry.  Camera n is the pinhole matrix [[8, 0, cx_n, 0], [0, 8, cy_n, 0], [0, 0, 1, 0], [0, 0, 0, 1]]; a key point (X, Y, Z) projects to
the pixel (8 X / Z + cx_n, 8 Y / Z + cy_n).  All designed key points have Z = 1, so on level 0 (stride 8) of a padded image of width pad_w

    px = (8 X + cx_n) / pad_w * W0 - 0.5 = X + cx_n / 8 - 0.5        (W0 = pad_w / 8; likewise py = Y + cy_n / 8 - 0.5)

and on level l the same with 2^-l (X + cx_n / 8) in front.  Camera 0 has cx = cy = 0: a family below states the level-0 position
(px, py) of its points in camera 0 and the key point is (px + 0.5, py + 0.5, 1).  Cameras n >= 1 are shifted by whole eighths of a token,
cx_n / 8 = -(2 + (n - 1) / 8) tokens and cy_n / 8 in {-0.5, -0.25, 0, 0.25, 0.5}: every camera is a different one, a set placed 3 .. 6
tokens from the left border is inside EVERY camera (`all_cameras`), a set within one token of the left border is inside camera 0 alone
(`one_camera`, the left band, the left corners), and the sets at the right border land at interior positions of the other cameras.

Two geometries carry the same families.  "dyadic": the padded image (64, 128), levels 8x16, 4x8, 2x4, 1x2 -- every number in the chain
(ref * span + lo, + offset, the matrix product, / pad, * W - 0.5) is a small dyadic rational, exact in float32 and float64 alike, so the
designed positions ARE the positions on both sides of a comparison: a point on a token centre has a corner weight of exactly 0 and a tent
of exactly 1, px == -1 and px == W contribute exactly nothing.  "ulp": the padded image (64, 96), levels 8x12, 4x6, 2x3, 1x2 -- 1 / 96 is
not a float32, the x positions come out within an ulp of the designed ones (2.9999998 for 3) on one side or the other of every edge; the
y positions stay exact.  Bilinear sampling with zero padding is continuous in the position and max(z, 1e-5) is continuous in z, so the
float64 reference is well defined on every element of both: nothing is excluded from a comparison.

pc_range is [-8, -8, -3, 24, 24, 5] (spans 32, 32, 8).  A row's reference point is r = (ref_m - lo) / span with ref_m = (the centre of the row's
points rounded to 1 / 8, 1): multiples of 1 / 256 in x and y and 0.5 in z, never 0, so ref * span + lo is exercised and exact; the offsets
are key point - ref_m.  (`behind` has r_z = 0.375, ref_m_z = 0, so that the z offsets -3, 0 and float32(1e-5) arrive unrounded.)

Families, one or a few rows each, all stacked as the rows of ONE case per (geometry, shape):

  centre               all points on one token centre (3, 2)
  lattice (2)          integer px with half-integer py; the transpose
  left_band, top_band  px (py) cycles through -0.75, -1, -0.5, -0.25, 0, 0.25, 0.5, the other coordinate inside
  right_band, bottom_band   px (py) cycles through W - 0.25, W, W - 1.5 .. W - 0.5 in steps of 0.25
  corner (4)           both coordinates in the bands, one row per corner of the map
  patch_8x8, wide_9x8  the points span exactly 8 x 8 tokens (the patch path); the same with one point one token further right (per-corner)
  patch_16x4, wide_16x5     16 x 4 tokens (12 x 4 in the "ulp" geometry, whose level 0 is 12 wide: the same power-of-two patch width 16); one
                       point one token further down
  column (2)           one token column over the full height; one token row over the full width
  coincident           all points at (5.375, 2.625)
  behind               patch_8x8 with its last four points replaced by (0, 0, -3), (0, 0, 0), (0, 0, float32(1e-5)) and (5, 5, -1)
  one_camera           px in -0.75 .. 1: inside camera 0 only
  all_cameras (2)      the wide_9x8 and the patch_8x8 set, placed where every camera sees all of it
  logits_pm30          patch_8x8; +30 on every 7th and -30 on every 11th (from 3) column of the row's U
  dominant_invisible   patch_8x8 with point 2 far outside every map and +8 on all its logits: the row is small, not zero
  edge_zero            every point on the left edge px_l = -1 of the coarsest level l, where that edge is furthest out (the finer levels and
                       the other cameras have it beyond the edge): the row is zero.  With one camera also the right, top and bottom
                       edge W_l, -1, H_l, one row each ("dyadic": exactly 0; "ulp": an x edge may be an ulp inside, |row| < 1e-6)

The point lists are 16 long and a shape takes the first P of them (the points that define a span come first); the families that need
several points are left out at P < 6.  Camera 0's Vc is raised by 1 (N >= 2): the camera whose positions are designed carries e times the weight
of another one, so that a row only camera 0 sees is not small at 16 cameras.  Camera N - 1's Vc is lowered by 60 on every other float4 of its row (N >= 2): the camera factor
exp(V[n] - max_n V) of the factored softmax is e^-60 there, and its product with a query factor of e^-60 (logits_pm30) underflows.

Shapes (N, P, L): (7, 13, 4) the model's; (8, 12, 4) N P L = 384 with a generic P and cameras 4..7 all present; (6, 16, 4) P at kernel
8's limit; (1, 1, 1); (3, 13, 2); (9, 13, 3) and (16, 6, 4) beyond kernel 8.

Reference: oracle.sampling.aggregation_ref in float64 on the float32 input values (the logits U + Vc are added in float64; for bf16 maps
the maps are rounded to bf16 first), cached per case and never modified.  MSDA: oracle.sampling.msda_grid_sample in float64 on locations
that run through every pair of 0, 1, -0.5 / W, -1 / W, (W + 0.5) / W, the token centres (k + 0.5) / W and the token borders k / W, and the same
in y."""
import functools

import torch

from far3d_amd import synth
from oracle import sampling

GEOMETRIES = {"dyadic": (64, 128), "ulp": (64, 96)}
SHAPES = [(7, 13, 4), (8, 12, 4), (6, 16, 4), (1, 1, 1), (3, 13, 2), (9, 13, 3), (16, 6, 4)]
PC_RANGE = [-8.0, -8.0, -3.0, 24.0, 24.0, 5.0]
G, C = 8, 256
NPTS = 16                    # length of a family's point list; a shape takes the first P
MULTI_POINT_MIN_P = 6        # the span / behind / logit families need their defining points
ZERO_FAMILY, SMALL_FAMILY = "edge_zero", "dominant_invisible"
FAR = 99.5                   # px of dominant_invisible's outlier


def kernel8_shape(shape):
    N, P, L = shape
    return N <= 8 and P <= 16


def sorted_mode_shape(shape):
    N, P, L = shape
    return kernel8_shape(shape) and L * P * 2 <= 104


def camera_shift(n):
    """(cx_n / 8, cy_n / 8): the shift of camera n's level-0 positions against camera 0's, in tokens."""
    return (0.0, 0.0) if n == 0 else (-(2.0 + (n - 1) * 0.125), ((3 * n) % 5 - 2) * 0.25)


def _cyc(vals, step=1):
    return [vals[(i * step) % len(vals)] for i in range(NPTS)]


def _span_sets(W, H):
    xs8 = [0.5, 6.5, 1, 2, 3, 4, 5, 6, 1.5, 2.5, 3.5, 4.5, 5.5, 2.25, 4.75, 3.25]
    ys8 = [0.5, 6.5, 6, 5, 4, 3, 2, 1, 1.5, 2.5, 3.5, 4.5, 5.5, 3.75, 1.25, 5.25]
    xs9 = list(xs8)
    xs9[1] = 7.5
    Wp = min(16, W)
    xs16 = [0.5, Wp - 1.5] + [1.0 + (i % (Wp - 3)) for i in range(11)] + [Wp - 4.0, Wp - 3.0, Wp - 2.5]
    ys4 = [0.5, 2.5] + [1.0 + 0.125 * i for i in range(11)] + [1.5, 2.25, 0.75]
    ys5 = list(ys4)
    ys5[1] = 3.5
    return xs8, ys8, xs9, xs16, ys4, ys5


def zero_edges(hw):
    """Camera-0 level-0 positions (left, right, top, bottom) that lie exactly on the edge -1 / W_l / H_l of the level where that edge is
    furthest out (the coarsest one) and beyond the edge on every other level: a point there contributes nothing on any level."""
    H0, W0 = hw[0]
    sx, sy = [w / W0 for _, w in hw], [h / H0 for h, _ in hw]          # level-l tokens per level-0 token: px_l = (px_0 + 0.5) s_l - 0.5
    return (min(-0.5 / s for s in sx) - 0.5, max((w + 0.5) / s for (_, w), s in zip(hw, sx)) - 0.5,
            min(-0.5 / s for s in sy) - 0.5, max((h + 0.5) / s for (h, _), s in zip(hw, sy)) - 0.5)


def family_rows(hw, N, P):
    """-> list of (family, px list, py list, special) for the levels hw: NPTS designed camera-0 level-0 positions per row; special is
    None, "behind", "pm30" or "dominant".  The band cycles start inside the band (at P = 1 the first point is the row)."""
    H, W = hw[0]
    LB = [-0.75, -1.0, -0.5, -0.25, 0.0, 0.25, 0.5]
    RB = [W - 0.25, float(W), W - 1.5, W - 1.25, W - 1.0, W - 0.75, W - 0.5]
    BB = [H - 0.25, float(H), H - 1.5, H - 1.25, H - 1.0, H - 0.75, H - 0.5]
    inx = [1.25 + (i * 3) % (W - 3) for i in range(NPTS)]
    iny = [1.25 + (i * 2) % (H - 3) for i in range(NPTS)]
    rows = [("centre", [3.0] * NPTS, [2.0] * NPTS, None),
            ("lattice", [float(i % W) for i in range(NPTS)], [(i * 3) % (H - 1) + 0.5 for i in range(NPTS)], None),
            ("lattice", [(i * 3) % (W - 1) + 0.5 for i in range(NPTS)], [float(i % H) for i in range(NPTS)], None),
            ("left_band", _cyc(LB), iny, None), ("top_band", inx, _cyc(LB), None),
            ("right_band", _cyc(RB), iny, None), ("bottom_band", inx, _cyc(BB), None)]
    for xb, yb in ((LB, LB), (RB, LB), (LB, BB), (RB, BB)):
        rows.append(("corner", _cyc(xb), _cyc(yb, 3), None))
    rows.append(("coincident", [5.375] * NPTS, [2.625] * NPTS, None))
    rows.append(("one_camera", _cyc([-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75, 1.0]), [0.25 + (i * 0.5) % (H - 1) for i in range(NPTS)], None))
    zl, zr, zt, zb = zero_edges(hw)
    edge_y = _cyc([-1.0, 0.0, 0.5, 1.75, 3.0, H - 1.0, float(H), 4.25])
    rows.append((ZERO_FAMILY, [zl] * NPTS, edge_y, None))
    if N == 1:
        rows.append((ZERO_FAMILY, [zr] * NPTS, edge_y, None))
        rows.append((ZERO_FAMILY, inx, [zt] * NPTS, None))
        rows.append((ZERO_FAMILY, inx, [zb] * NPTS, None))
    if P >= MULTI_POINT_MIN_P:
        xs8, ys8, xs9, xs16, ys4, ys5 = _span_sets(W, H)
        ox = 6.0 if W >= 16 else 3.0       # where every camera (shifts down to -3.75 tokens) still sees a 9-token-wide set
        rows += [("patch_8x8", xs8, ys8, None), ("wide_9x8", xs9, ys8, None), ("patch_16x4", xs16, ys4, None), ("wide_16x5", xs16, ys5, None),
                 ("column", [5.0] * NPTS, [0.0, H - 1.0] + [(0.5 + 0.5 * i) % (H - 1) for i in range(NPTS - 2)], None),
                 ("column", [0.0, W - 1.0] + [(0.75 + 0.75 * i) % (W - 1) for i in range(NPTS - 2)], [3.0] * NPTS, None),
                 ("behind", xs8, ys8, "behind"),
                 ("all_cameras", [x + ox for x in xs9], ys8, None), ("all_cameras", [x + ox for x in xs8], ys8, None),
                 ("logits_pm30", xs8, ys8, "pm30"),
                 (SMALL_FAMILY, xs8[:2] + [FAR] + xs8[3:], ys8, "dominant")]
    return rows


BEHIND_POINTS = [(0.0, 0.0, -3.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1e-5), (5.0, 5.0, -1.0)]      # the last four key points of `behind`


@functools.lru_cache(maxsize=None)
def case(geom, shape):
    """The designed inputs of one (geometry, shape): the keys of tests.cases.aggregate_case, plus `family` (the family of every row),
    `design` ((A, P, 2) the designed camera-0 level-0 positions, NaN where a point is given as a key point), `key_points`, `shape` and
    `geom`.  Built once, never modified."""
    N, P, L = shape
    pad_hw = GEOMETRIES[geom]
    hw = synth.level_shapes(pad_hw)[:L]
    starts, S = synth.level_starts(hw)
    H0, W0 = hw[0]
    rows = family_rows(hw, N, P)
    A, J = len(rows), L * P * G
    g = torch.Generator().manual_seed(1000 * N + 10 * P + L + (0 if geom == "dyadic" else 500000))
    feat = torch.randn(N, S, C, generator=g)
    U = torch.randn(A, J, generator=g)
    Vc = torch.randn(N, J, generator=g)
    if N >= 2:
        Vc[0] += 1.0         # the designed positions are camera 0's: e times the weight of another camera
        Vc[N - 1, (torch.arange(J) // 4) % 2 == 1] -= 60.0
    l2i = torch.zeros(N, 4, 4)
    for n in range(N):
        sx, sy = camera_shift(n)
        l2i[n] = torch.tensor([[8.0, 0.0, 8.0 * sx, 0.0], [0.0, 8.0, 8.0 * sy, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    lo, span = torch.tensor(PC_RANGE[:3]), torch.tensor(PC_RANGE[3:]) - torch.tensor(PC_RANGE[:3])
    kp = torch.zeros(A, P, 3)
    design = torch.zeros(A, P, 2)
    ref_m = torch.zeros(A, 3)
    for a, (fam, xs, ys, special) in enumerate(rows):
        design[a, :, 0], design[a, :, 1] = torch.tensor(xs[:P]), torch.tensor(ys[:P])
        kp[a, :, 0], kp[a, :, 1], kp[a, :, 2] = design[a, :, 0] + 0.5, design[a, :, 1] + 0.5, 1.0
        near = design[a, :, 0] < FAR
        if special == "behind":
            kp[a, P - 4:] = torch.tensor(BEHIND_POINTS)
            design[a, P - 4:] = float("nan")
            near[P - 4:] = False
        if special == "pm30":
            b = torch.zeros(J)
            b[::7] = 30.0
            b[3::11] = -30.0
            U[a] += b
        if special == "dominant":
            U[a].view(L, P, G)[:, 2, :] += 8.0
        ref_m[a, :2] = torch.round(kp[a, near, :2].mean(0) * 8.0) / 8.0
        ref_m[a, 2] = 0.0 if special == "behind" else 1.0
    ref = (ref_m - lo) / span
    offsets = kp - ref_m[:, None, :]
    assert torch.equal(ref * span + lo, ref_m) and torch.equal(ref_m[:, None, :] + offsets, kp), "the key points are exact in float32"
    assert float(ref.min()) > 0.0 and float(ref.max()) < 1.0 and A <= 32
    return dict(feat=feat, ref=ref, offsets=offsets, lidar2img=l2i, U=U, Vc=Vc, level_hw=hw, level_start=starts, pc_range=list(PC_RANGE),
                pad_hw=tuple(pad_hw), G=G, family=[r[0] for r in rows], design=design, key_points=kp, shape=shape, geom=geom)


def rows_of(c, family):
    return [a for a, f in enumerate(c["family"]) if f == family]


def sub_case(c, rows=None, cams=None, levels=None):
    """The case restricted to some rows, cameras and (leading) levels: for the CPU test's per-row path statistics."""
    rows = list(range(len(c["family"]))) if rows is None else rows
    N, P, L = c["shape"]
    cams = list(range(N)) if cams is None else cams
    levels = L if levels is None else levels
    hw = c["level_hw"][:levels]
    starts, S = synth.level_starts(hw)
    d = dict(c)
    d.update(feat=c["feat"][cams][:, :S], ref=c["ref"][rows], offsets=c["offsets"][rows], lidar2img=c["lidar2img"][cams],
             U=c["U"][rows].view(len(rows), L, P * G)[:, :levels].reshape(len(rows), -1),
             Vc=c["Vc"][cams].view(len(cams), L, P * G)[:, :levels].reshape(len(cams), -1),
             level_hw=hw, level_start=starts, family=[c["family"][a] for a in rows], shape=(len(cams), P, levels))
    return d


def run_ref(fn, c, dtype, bf16_maps=False):
    """fn = sampling.aggregation_ref / aggregation_tent on the case's values in `dtype` (the logits are added in `dtype`)."""
    feat = c["feat"].to(torch.bfloat16).float() if bf16_maps else c["feat"]
    logits = c["U"].to(dtype)[:, None, :] + c["Vc"].to(dtype)[None, :, :]
    return fn(feat.to(dtype), c["ref"].to(dtype), c["offsets"].to(dtype), c["lidar2img"].to(dtype), logits, c["level_hw"], c["level_start"],
              c["pc_range"], c["pad_hw"], num_groups=c["G"])


@functools.lru_cache(maxsize=None)
def reference(geom, shape, bf16_maps=False):
    """float64 (A, 256) of a case: computed once, shared, never modified."""
    return run_ref(sampling.aggregation_ref, case(geom, shape), torch.float64, bf16_maps)


def reversed_case(c):
    """The same case with its rows in reverse order (the second sample of the batched test)."""
    d = dict(c)
    d.update(ref=c["ref"].flip(0), offsets=c["offsets"].flip(0), U=c["U"].flip(0), family=c["family"][::-1])
    return d


# ------------------------------------------------------------------------------------------------ far3d_msda_forward
MSDA = {"levels": dict(H=8, Dh=32, hw=((8, 16), (4, 8), (2, 4), (1, 2)), Q=13, P=4),        # the dyadic geometry's levels
        "small": dict(H=2, Dh=4, hw=((6, 9), (3, 5), (2, 2)), Q=20, P=5)}                    # odd sizes: an ulp from the edges


def edge_coordinates(W):
    return [0.0, 1.0, -0.5 / W, -1.0 / W, (W + 0.5) / W] + [(k + 0.5) / W for k in range(W)] + [k / W for k in range(W)]


@functools.lru_cache(maxsize=None)
def msda_case(name):
    """Locations that run through every (x, y) pair of edge_coordinates on level 0 (and cycle through them on the others)."""
    m = MSDA[name]
    H, Dh, hw, Q, P, bs = m["H"], m["Dh"], m["hw"], m["Q"], m["P"], 2
    L = len(hw)
    starts, S = synth.level_starts(hw)
    g = torch.Generator().manual_seed(41 + H)
    s = torch.arange(bs * Q * H * P).view(bs, Q, H, P)
    loc = torch.zeros(bs, Q, H, L, P, 2)
    for l, (Hl, Wl) in enumerate(hw):
        xs, ys = torch.tensor(edge_coordinates(Wl), dtype=torch.float64), torch.tensor(edge_coordinates(Hl), dtype=torch.float64)
        loc[:, :, :, l, :, 0] = xs[s % len(xs)].float()
        loc[:, :, :, l, :, 1] = ys[(s // len(xs)) % len(ys)].float()
    assert bs * Q * H * P >= len(edge_coordinates(hw[0][0])) * len(edge_coordinates(hw[0][1])), "every pair occurs on level 0"
    return dict(value=torch.randn(bs, S, H, Dh, generator=g), shapes=torch.tensor([list(x) for x in hw], dtype=torch.long),
                lsi=torch.tensor(starts, dtype=torch.long), loc=loc, w=torch.rand(bs, Q, H, L, P, generator=g))


@functools.lru_cache(maxsize=None)
def msda_reference(name, bf16_values=False):
    c = msda_case(name)
    v = c["value"].to(torch.bfloat16).float() if bf16_values else c["value"]
    return sampling.msda_grid_sample(v.double(), c["shapes"], c["lsi"], c["loc"].double(), c["w"].double())

"""CPU: the designed cases of tests/agg_edge_cases.py are what they claim, and their float64 reference agrees with two independent
statements of the operation.  No GPU.

  * path per family: oracle.sampling.aggregation_tent mirrors the kernels' patch rule (spanx <= 64 and spany <= 64 >> lw); its `stats` on
    level 0 of camera 0 say which path a row's item takes there, and how many list rows a whole query makes;
  * exact positions: in the dyadic geometry project_points gives the same bits in float32 and float64 on every point inside a map's
    band, and camera 0's level-0 positions are the designed ones -- integers, -1 and W where the family says so;
  * no near-clamp element: a point with z <= 1e-5 either has the key point X = Y = 0 -- then x = cx z and y = cy z are single exact
    products and the position cx z / max(z, 1e-5) does not feel a rounding of z -- or projects at least one image width outside;
  * rows are not degenerate: max |row| >= 0.05 in float64, except the rows designed to be zero (exactly 0 in the dyadic geometry, below
    1e-6 an ulp from the edge) and dominant_invisible (not zero);
  * the yardstick: aggregation_ref in float32 and aggregation_tent against the float64 result on every case, msda_loops against the
    float64 msda_grid_sample on the small MSDA case -- each below 2e-6.  tests/test_agg_edges_gpu.py holds the kernels to 2e-5.

Distances of one run (printed by the tests): aggregation_ref in float32 1.2e-7 .. 1.2e-6 and aggregation_tent 1.2e-7 .. 1.1e-6 from float64 on
outputs up to 1.5 (3.3 at one camera, one point); msda_loops 1.0e-6 on outputs up to 3.3.  The largest belong to the "ulp" geometry and to
logits_pm30, whose float32 logits of size 30 carry an ulp of 1.9e-6.  An all_cameras query lists 399 .. 657 rows at N >= 7."""
import pytest
import torch

from oracle import sampling
from tests import agg_edge_cases as ec

CASES = [(g, s) for g in ec.GEOMETRIES for s in ec.SHAPES]
CASE_IDS = ["%s-N%d-P%d-L%d" % ((g,) + s) for g, s in CASES]
PATCH_FAMILIES = ("patch_8x8", "patch_16x4", "centre", "coincident", "left_band", "right_band", "top_band", "bottom_band", "corner", "column",
                  "one_camera", "logits_pm30")
WIDE_FAMILIES = ("wide_9x8", "wide_16x5", "behind")


def _stats(c, rows=None, cams=None, levels=None):
    return ec.run_ref(sampling.aggregation_tent, ec.sub_case(c, rows, cams, levels), torch.float32)[1]


@pytest.mark.parametrize("geom,shape", CASES, ids=CASE_IDS)
def test_every_family_takes_the_path_it_names(geom, shape):
    c = ec.case(geom, shape)
    N, P, L = shape
    assert len(c["family"]) <= 32
    for a, fam in enumerate(c["family"]):
        s = _stats(c, [a], [0], 1)
        if fam in PATCH_FAMILIES:
            assert s["patch"] == 1 and s["wide"] == 0, (fam, a, s)
        if fam in WIDE_FAMILIES:
            assert s["wide"] == 1 and s["rows"] > 0, (fam, a, s)
        if fam == ec.ZERO_FAMILY:
            assert s["wide"] == 0 and s["rows"] == 0, (fam, a, s)
        if fam == "all_cameras":
            whole = _stats(c, [a])
            print("%s %s row %d: all_cameras lists %d rows (camera 0, level 0: %s)" % (geom, shape, a, whole["rows"], s))
            # every camera sees every point of the set on every level
            assert whole["patch"] + whole["wide"] == N * L
            if N >= 7:
                assert whole["rows"] > 256, (a, whole)
    if P >= ec.MULTI_POINT_MIN_P:
        for fam in PATCH_FAMILIES + WIDE_FAMILIES + ("all_cameras", ec.SMALL_FAMILY):
            assert ec.rows_of(c, fam), fam
    # the two all_cameras rows are one patch and one per-corner set on camera 0's level 0
    ac = ec.rows_of(c, "all_cameras")
    if ac:
        assert _stats(c, ac[:1], [0], 1)["wide"] == 1 and _stats(c, ac[1:], [0], 1)["patch"] == 1


def _level0(c, dtype):
    """Level-0 pixel positions (N, A, P, 2) of the case's key points, evaluated in dtype along the reference's text."""
    pc = torch.tensor(c["pc_range"], dtype=dtype)
    kp = (c["ref"].to(dtype) * (pc[3:] - pc[:3]) + pc[:3])[:, None, :] + c["offsets"].to(dtype)
    p2d = sampling.project_points(kp[None], c["lidar2img"].to(dtype)[None], c["pad_hw"])[0]
    H0, W0 = c["level_hw"][0]
    return torch.stack([p2d[..., 0] * W0 - 0.5, p2d[..., 1] * H0 - 0.5], -1), kp


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "N%d-P%d-L%d" % s)
def test_dyadic_positions_are_exact(shape):
    c = ec.case("dyadic", shape)
    N, P, L = shape
    H0, W0 = c["level_hw"][0]
    p32, kp32 = _level0(c, torch.float32)
    p64, kp64 = _level0(c, torch.float64)
    assert torch.equal(kp32.double(), kp64) and torch.equal(kp32, c["key_points"])
    band = (p64[..., 0] >= -1) & (p64[..., 0] <= W0) & (p64[..., 1] >= -1) & (p64[..., 1] <= H0) & (kp64[None, :, :, 2] > 1e-5)
    assert int(band.sum()) > 0 and torch.equal(p32.double()[band], p64[band]), "float32 and float64 positions differ inside the band"
    # camera 0 sees the designed positions; camera n the same shifted by camera_shift(n)
    design = c["design"].double()
    given = ~torch.isnan(design[..., 0])
    for n in range(N):
        sx, sy = ec.camera_shift(n)
        assert torch.equal(p64[n][given], (design + torch.tensor([sx, sy], dtype=torch.float64))[given]), n
    # ... and the same on the coarser levels: 2^-l (px + 0.5) - 0.5 with the level's size
    p2d = sampling.project_points(kp32[None], c["lidar2img"][None], c["pad_hw"])[0]
    for l, (Hl, Wl) in enumerate(c["level_hw"]):
        assert torch.equal((p2d[0, ..., 0] * Wl - 0.5)[given].double(), ((design[..., 0] + 0.5) / 2 ** l - 0.5)[given])
    fam = lambda f: design[ec.rows_of(c, f)]
    is_int = lambda t: bool((t == t.round()).all())
    is_half = lambda t: bool(((t - 0.5) == (t - 0.5).round()).all())
    assert is_int(fam("centre"))
    la, lb = fam("lattice")
    assert is_int(la[:, 0]) and is_half(la[:, 1]) and is_half(lb[:, 0]) and is_int(lb[:, 1])
    # a band row: starts inside the band (one column of corners inside the map), holds the edge itself and the last token centre
    edges = {"left_band": (0, -0.75, -1.0, 0.0), "top_band": (1, -0.75, -1.0, 0.0), "right_band": (0, W0 - 0.25, float(W0), W0 - 1.0),
             "bottom_band": (1, H0 - 0.25, float(H0), H0 - 1.0)}
    for f, (axis, first, edge, last) in edges.items():
        v = fam(f)[0, :, axis].tolist()
        assert v[0] == first
        if P >= 7:
            assert edge in v and last in v, (f, v)
    for row in fam("corner"):
        assert bool(((row[:, 0] <= 0.5) | (row[:, 0] >= W0 - 1.5)).all() and ((row[:, 1] <= 0.5) | (row[:, 1] >= H0 - 1.5)).all())
    # edge_zero: exactly on an edge of the coarsest level, beyond it on the finer ones
    Hc, Wc = c["level_hw"][-1]
    zc = (fam(ec.ZERO_FAMILY) + 0.5) / 2 ** (L - 1) - 0.5
    assert bool(((zc[..., 0] == -1) | (zc[..., 0] == Wc) | (zc[..., 1] == -1) | (zc[..., 1] == Hc)).all(-1).all())
    assert len(zc) == (4 if N == 1 else 1)
    assert bool((fam("one_camera")[..., 0] > -1).all()) and bool((fam("one_camera")[..., 0] - 2 <= -1).all())
    if P >= ec.MULTI_POINT_MIN_P:
        span = lambda t, size: int(min(t.max().floor() + 1, size - 1) - max(t.min().floor(), 0)) + 1
        for f, sx, sy in (("patch_8x8", 8, 8), ("wide_9x8", 9, 8), ("patch_16x4", 16, 4), ("wide_16x5", 16, 5)):
            pts = fam(f)[0]
            assert (span(pts[:, 0], W0), span(pts[:, 1], H0)) == (sx, sy), f
        ca, cb = fam("column")
        assert (span(ca[:, 0], W0), span(ca[:, 1], H0)) == (2, H0) and is_int(ca[:, 0]) and (span(cb[:, 0], W0), span(cb[:, 1], H0)) == (W0, 2)
        for row in fam("all_cameras"):        # inside every camera on level 0
            for n in range(N):
                sx, sy = ec.camera_shift(n)
                assert bool((row[:, 0] + sx > -1).all() and (row[:, 0] + sx < W0).all() and (row[:, 1] + sy > -1).all() and (row[:, 1] + sy < H0).all())


@pytest.mark.parametrize("geom,shape", CASES, ids=CASE_IDS)
def test_no_element_hangs_on_the_z_clamp(geom, shape):
    c = ec.case(geom, shape)
    pc = torch.tensor(c["pc_range"], dtype=torch.float64)
    kp = (c["ref"].double() * (pc[3:] - pc[:3]) + pc[:3])[:, None, :] + c["offsets"].double()             # (A,P,3)
    kp1 = torch.cat([kp, torch.ones_like(kp[..., :1])], -1)
    xyz = torch.einsum("nrk,apk->napr", c["lidar2img"].double()[:, :3, :], kp1)
    uv = sampling.project_points(kp[None], c["lidar2img"].double()[None], c["pad_hw"])[0]                 # (N,A,P,2) in [0,1] inside
    clamped = xyz[..., 2] <= 1e-5
    on_axis = ((kp[..., 0] == 0) & (kp[..., 1] == 0))[None].expand_as(clamped)
    outside = ((uv < -1) | (uv > 2)).any(-1)
    assert bool((~clamped | on_axis | outside).all())
    if "behind" in c["family"]:
        assert int(clamped.sum()) == 4 * shape[0] and int((clamped & on_axis).sum()) == 3 * shape[0]
        # the on-axis points of camera 0 land on (0, 0): inside the corner token with weight 0.25
        a = ec.rows_of(c, "behind")[0]
        assert torch.equal(uv[0, a, -4:-1], torch.zeros(3, 2, dtype=torch.float64))
    else:
        assert int(clamped.sum()) == 0


@pytest.mark.parametrize("geom,shape", CASES, ids=CASE_IDS)
def test_rows_are_not_degenerate(geom, shape):
    c = ec.case(geom, shape)
    for bf16 in (False, True):
        r = ec.reference(geom, shape, bf16)
        assert r.dtype == torch.float64 and r.shape == (len(c["family"]), 256)
        rowmax = r.abs().amax(1)
        for a, fam in enumerate(c["family"]):
            if fam == ec.ZERO_FAMILY:
                assert rowmax[a].item() == 0.0 if geom == "dyadic" else rowmax[a].item() < 1e-6, (a, rowmax[a].item())
            elif fam == ec.SMALL_FAMILY:
                assert 0.0 < rowmax[a].item() < 0.05, (a, rowmax[a].item())
            else:
                assert rowmax[a].item() >= 0.05, (fam, a, rowmax[a].item())
    if shape[0] >= 2 and "logits_pm30" in c["family"]:
        # the factored softmax's camera factor is e^-60 on half of the last camera's row, and the product with the query factor underflows
        a = ec.rows_of(c, "logits_pm30")[0]
        V, U = c["Vc"], c["U"][a]
        cam = torch.exp(V[-1] - V.max(0).values)
        qry = torch.exp(U + V.max(0).values - (U + V.max(0).values).max())
        assert float(cam.min()) < 1e-25 and float((cam * qry).min()) == 0.0


@pytest.mark.parametrize("geom,shape", CASES, ids=CASE_IDS)
def test_reference_agrees_with_the_float32_restatements(geom, shape):
    c = ec.case(geom, shape)
    r64 = ec.reference(geom, shape)
    d_ref = (ec.run_ref(sampling.aggregation_ref, c, torch.float32).double() - r64).abs().max().item()
    d_tent = (ec.run_ref(sampling.aggregation_tent, c, torch.float32)[0].double() - r64).abs().max().item()
    print("%s %s: aggregation_ref f32 - f64 %.3e, aggregation_tent f32 - f64 %.3e, max |out| %.2f" % (geom, shape, d_ref, d_tent, r64.abs().max().item()))
    assert d_ref < 2e-6 and d_tent < 2e-6


def test_msda_reference_agrees_with_the_scalar_restatement():
    c = ec.msda_case("small")
    r64 = ec.msda_reference("small")
    loops = torch.from_numpy(sampling.msda_loops(c["value"].numpy(), c["shapes"].tolist(), c["lsi"].tolist(), c["loc"].numpy(), c["w"].numpy()))
    d = (loops.double() - r64).abs().max().item()
    print("msda small: msda_loops f32 - msda_grid_sample f64 %.3e, max |out| %.2f" % (d, r64.abs().max().item()))
    assert d < 2e-6
    for name in ec.MSDA:
        m = ec.msda_case(name)
        Hl, Wl = ec.MSDA[name]["hw"][0]
        x, y = m["loc"][:, :, :, 0, :, 0].flatten().double(), m["loc"][:, :, :, 0, :, 1].flatten().double()
        pairs = {(round(float(a) * Wl * 2), round(float(b) * Hl * 2)) for a, b in zip(x, y)}       # half-token units
        nx, ny = len(set(round(v * Wl * 2) for v in ec.edge_coordinates(Wl))), len(set(round(v * Hl * 2) for v in ec.edge_coordinates(Hl)))
        assert len(pairs) == nx * ny, "every pair of edge coordinates occurs on level 0"
        assert ec.msda_reference(name).abs().max().item() > 0.5

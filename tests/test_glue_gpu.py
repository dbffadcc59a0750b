"""GPU: the FarHead bookkeeping kernels one by one (csrc/glue.hip: far3d_memory_prepare, far3d_memory_post_update, far3d_posemb3d,
far3d_head_finalize; csrc/frontend.hip: far3d_row_affine_ln) against the float64 restatements of tests/head_refs.py.

Tolerances (none is tuned against the kernels):
 * copies / selections: bit-equal; float64 outputs (timestamps): equal (one IEEE add / subtract);
 * fp32 dot products (pose / reference-point warps, the affine): 2 * n_ops * 2^-24 * sum |a_k| |b_k| on the float64 magnitudes,
   n_ops counted from the kernel's expression (head_refs.matmul_bound);
 * chains through expf / logf / sinf / cosf / sqrtf: at most 4 x (the float32 restatement's own distance from float64, on the same
   inputs) + 2 ulp of the output's largest magnitude (head_refs.chain_bound).
tests/test_head_refs_cpu.py shows that each of these bounds rejects the slips it is there for.  Every test prints its figures
(pytest -s shows them)."""
import math

import pytest
import torch

from tests import head_refs as hr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = hr.U32
PC = [-152.4, -152.4, -5.0, 152.4, 152.4, 5.0]


def report(tag, **kw):
    print("[glue] %s: %s" % (tag, "  ".join("%s=%.3e" % (k, v) for k, v in kw.items())))


def to_dev_mem(st):
    """head_refs layout (L,..) CPU -> the engine's (1,L,..) device layout."""
    L = st["emb"].shape[0]
    return dict(emb=st["emb"].float().reshape(1, L, -1).to(DEV).contiguous(), ref=st["ref"].float().reshape(1, L, 3).to(DEV).contiguous(),
                ts=st["ts"].double().reshape(1, L, 1).to(DEV).contiguous(), pose=st["pose"].float().reshape(1, L, 4, 4).to(DEV).contiguous(),
                velo=st["velo"].float().reshape(1, L, 2).to(DEV).contiguous())


def from_dev_mem(d):
    L = d["emb"].shape[1]
    return dict(emb=d["emb"].cpu()[0], ref=d["ref"].cpu()[0], ts=d["ts"].cpu().reshape(L), pose=d["pose"].cpu()[0], velo=d["velo"].cpu()[0])


def within(got, want, bound, tag):
    """|got - want| <= bound elementwise (bound 0 = exact); returns (largest error, largest bound) for the report."""
    err = (got.double() - want.double()).abs()
    bad = ~(err <= bound)                      # NaN-proof
    assert not bad.any(), "%s: %d elements off, worst error %.3e against its bound %.3e" % (
        tag, int(bad.sum()), err[bad].max().item(), (bound.expand_as(err)[bad][err[bad].argmax()].item() if torch.is_tensor(bound) else bound))
    return err.max().item(), (bound.max().item() if torch.is_tensor(bound) else bound)


@pytest.mark.parametrize("scale", hr.MEM_SCALES)
@pytest.mark.parametrize("mode", hr.MEM_MODES)
@pytest.mark.parametrize("L,E,P", hr.MEM_SIZES)
def test_memory_prepare_against_float64(hip_lib, L, E, P, mode, scale):
    """One far3d_memory_prepare call: every output against head_refs.pre_update / motion_code / time_code."""
    from far3d_amd import ops
    mc = hr.memory_case(L, E, P, mode, scale)
    st, x = mc["state"], mc["x"]
    dt256 = hr.dim_t(256)
    pseudo_d = mc["pseudo_ref"].to(DEV) if P else None
    m_d, tref_d, nerf_d, tpos_d = ops.memory_prepare(to_dev_mem(st), mc["ego_inv"].to(DEV), torch.tensor([mc["timestamp"]], dtype=torch.float64, device=DEV),
                                                     pseudo_d, dt256.to(DEV), x, mc["fresh"], PC, P)
    got = from_dev_mem(m_d)
    tref, nerf, tpos = tref_d.cpu(), nerf_d.cpu(), tpos_d.cpu()
    st64 = hr.widen(st)
    want, want_tref = hr.pre_update(st64, mc["ego_inv"].double(), mc["timestamp"], mc["pseudo_ref"], x, P, PC, fresh=mc["fresh"])
    lo, span = hr._span(PC, torch.float64)
    tag = "prepare L=%d E=%d P=%d %s %s" % (L, E, P, mode, scale)
    # copies and the float64 timestamp
    assert torch.equal(got["emb"], st["emb"] * x) and torch.equal(got["velo"], st["velo"] * x), tag
    assert got["ts"].dtype == torch.float64 and torch.equal(got["ts"], want["ts"]), tag
    # warps
    bp, br = hr.prepare_bounds(st64, mc["ego_inv"], mc["pseudo_ref"], x, P, lo, span)
    ep = within(got["pose"], want["pose"], bp, tag + " m_pose")
    er = within(got["ref"], want["ref"], br, tag + " m_ref")
    if x == 0.0:      # rows >= P receive neither the pseudo reference points nor the identity
        assert not got["ref"][P:].any() and not got["pose"][P:].any(), tag
        assert torch.equal(got["pose"][:P], torch.eye(4).expand(P, 4, 4)), tag
    # temp_ref: (v - lo) / span on the kernel's own m_ref: subtract, divide (+1) -> 3 roundings; and against float64 end to end
    own = (got["ref"].double() - lo) / span
    bt = 2 * 3 * U * (got["ref"].double().abs() + lo.abs()) / span
    et = within(tref, own, bt, tag + " temp_ref (own m_ref)")
    within(tref, want_tref, bt + br / span, tag + " temp_ref")
    # codes, against the float64 code of the kernel's own (just verified) outputs
    n64 = hr.motion_code(got["velo"], got["ts"], got["pose"], torch.float64)
    yn = hr.yard(hr.motion_code(got["velo"], got["ts"], got["pose"], torch.float32), n64)
    bn = hr.chain_bound(yn, n64)
    en = within(nerf, n64, bn, tag + " nerf")
    t64 = hr.time_code(got["ts"], dt256)
    yt = hr.yard(t64.float(), t64)
    btp = hr.chain_bound(yt, t64)
    etp = within(tpos, t64, btp, tag + " tpos")
    report(tag, pose_err=ep[0], pose_bound=ep[1], ref_err=er[0], ref_bound=er[1], tref_err=et[0], tref_bound=et[1],
           nerf_yard=yn, nerf_bound=bn, nerf_err=en[0], tpos_yard=yt, tpos_bound=btp, tpos_err=etp[0])


def push_inputs(A, E, code, K, seed):
    g = torch.Generator().manual_seed(seed)
    box = torch.randn(A, code, generator=g)
    box[:, :3] = (torch.rand(A, 3, generator=g) - 0.5) * torch.tensor([300.0, 300.0, 10.0])
    box[:, -2:] = torch.randn(A, 2, generator=g) * 8
    idx = torch.randint(0, A, (K,), generator=g)
    if K >= 4:
        idx[1] = idx[0]                    # a repeated index, unsorted
        idx[2], idx[3] = A - 1, 0
    return torch.randn(A, E, generator=g), box, idx


@pytest.mark.parametrize("code", [8, 10])
@pytest.mark.parametrize("L,E,K", [(1024, 256, 0), (1024, 256, 1), (1024, 256, 256), (1024, 256, 1024), (37, 100, 5), (5, 256, 5)])
def test_memory_post_update_against_float64(hip_lib, L, E, K, code):
    """The push: K repeated / unsorted indices in front, the kept rows shifted by K, the last K dropped, everything warped by the
    (city-frame) ego pose; the state buffers held NaN before, so every element is written."""
    from far3d_amd import ops
    mc = hr.memory_case(L, E, 0, "steady", "city", seed=K + code)
    m = mc["state"]
    A = 1544 if L > 100 else 41
    dec, box, idx = push_inputs(A, E, code, K, seed=5 * K + code)
    state_d = {k: torch.full_like(v, float("nan")) for k, v in to_dev_mem(m).items()}
    ops.memory_post_update(to_dev_mem(m), idx.to(DEV), dec.to(DEV), box.to(DEV), mc["ego_pose"].to(DEV),
                           torch.tensor([mc["timestamp"]], dtype=torch.float64, device=DEV), state_d)
    got = from_dev_mem(state_d)
    m64 = hr.widen(m)
    want = hr.post_update(m64, idx, dec.double(), box.double(), mc["ego_pose"].double(), mc["timestamp"], L)
    tag = "post L=%d E=%d K=%d code=%d" % (L, E, K, code)
    assert torch.equal(got["emb"], torch.cat([dec[idx], m["emb"]])[:L]), tag
    assert torch.equal(got["velo"], torch.cat([box[idx][:, code - 2:], m["velo"]])[:L]), tag
    assert got["ts"].dtype == torch.float64 and torch.equal(got["ts"], want["ts"]), tag
    assert torch.equal(got["ts"][:K], torch.full((K,), -mc["timestamp"], dtype=torch.float64)), tag
    assert torch.equal(got["pose"][:K], mc["ego_pose"].expand(K, 4, 4)), tag + ": a pushed row's pose is ego_pose itself"
    bp, br = hr.post_bounds(m64, box.double()[idx][:, :3], K, L, mc["ego_pose"])
    ep = within(got["pose"], want["pose"], bp, tag + " pose")
    er = within(got["ref"], want["ref"], br, tag + " ref")
    report(tag, pose_err=ep[0], pose_bound=ep[1], ref_err=er[0], ref_bound=er[1])


@pytest.mark.parametrize("way", ["engine", "reference"])
def test_memory_sequence_against_float64(hip_lib, way):
    """Eight frames of prepare -> push on the device and in float64 side by side (L = 3 K: the queue is full from the third frame
    on), epoch timestamps and city-frame poses, one scene change at frame 4 -- the engine's way (zeroed state + fresh) or the reference's
    (prev_exists = 0 on the live state).  The whole state is compared after every frame.  The bound of an entry is accumulated over
    the warps it has lived through: e' = |M| e + bound(this warp), entry by entry, so a young entry is not judged by an old one's
    allowance; the report lists error / bound by age."""
    from far3d_amd import ops
    K, L, E, P, A, code, frames, change = 16, 48, 256, 16, 97, 10, 8, 4
    poses, ts = hr.drive("city", frames, seed=3)
    g = torch.Generator().manual_seed(12)
    pseudo = torch.rand(P, 3, generator=g)
    lo, span = hr._span(PC, torch.float64)
    dt256 = hr.dim_t(256).to(DEV)
    zero = dict(emb=torch.zeros(L, E), ref=torch.zeros(L, 3), ts=torch.zeros(L, dtype=torch.float64), pose=torch.zeros(L, 4, 4), velo=torch.zeros(L, 2))
    dev = to_dev_mem(zero)
    ref = hr.widen(zero)
    e_pose, e_ref = torch.zeros(L, 4, 4, dtype=torch.float64), torch.zeros(L, 3, dtype=torch.float64)
    age = torch.zeros(L, dtype=torch.long)
    worst = {}
    for f in range(frames):
        ego, ego_inv = poses[f].float(), hr.rigid_inverse(poses[f]).float()
        T = torch.tensor([ts[f]], dtype=torch.float64, device=DEV)
        first = f == 0 or (f == change and way == "engine")
        x = 0.0 if (first or f == change) else 1.0
        if first:
            for v in dev.values():
                v.zero_()
            ref = hr.widen(zero)
        m_d, _, _, _ = ops.memory_prepare(dev, ego_inv.to(DEV), T, pseudo.to(DEV), dt256, x, first, PC, P)
        bp, br = hr.prepare_bounds(ref, ego_inv, pseudo, x, P, lo, span)
        m64, _ = hr.pre_update(ref, ego_inv.double(), ts[f], pseudo, x, P, PC, fresh=first)
        em_pose = x * (ego_inv.double().abs()[None] @ e_pose) + bp
        em_ref = x * (ego_inv.double().abs()[:3, :3] @ e_ref.T).T + br
        got = from_dev_mem(m_d)
        tag = "sequence (%s) frame %d prepare" % (way, f)
        assert torch.equal(got["ts"], m64["ts"]) and torch.equal(got["emb"].double(), m64["emb"]) and torch.equal(got["velo"].double(), m64["velo"]), tag
        within(got["pose"], m64["pose"], em_pose, tag + " m_pose")
        within(got["ref"], m64["ref"], em_ref, tag + " m_ref")
        dec, box, idx = push_inputs(A, E, code, K, seed=100 + f)
        ops.memory_post_update(m_d, idx.to(DEV), dec.to(DEV), box.to(DEV), ego.to(DEV), T, dev)
        bp, br = hr.post_bounds(m64, box.double()[idx][:, :3], K, L, ego)
        ref = hr.post_update(m64, idx, dec.double(), box.double(), ego.double(), ts[f], L)
        e_pose = ego.double().abs()[None] @ torch.cat([torch.zeros(K, 4, 4, dtype=torch.float64), em_pose])[:L] + bp
        e_ref = (ego.double().abs()[:3, :3] @ torch.cat([torch.zeros(K, 3, dtype=torch.float64), em_ref])[:L].T).T + br
        age = torch.cat([torch.zeros(K, dtype=torch.long), (age + 1) * (0 if x == 0.0 else 1)])[:L]
        got = from_dev_mem(dev)
        tag = "sequence (%s) frame %d state" % (way, f)
        assert torch.equal(got["ts"], ref["ts"]) and torch.equal(got["emb"].double(), ref["emb"]) and torch.equal(got["velo"].double(), ref["velo"]), tag
        within(got["pose"], ref["pose"], e_pose, tag + " pose")
        within(got["ref"], ref["ref"], e_ref, tag + " ref")
        for a in age.unique().tolist():
            rows = age == a
            err = max((got["pose"].double() - ref["pose"])[rows].abs().max().item(), (got["ref"].double() - ref["ref"])[rows].abs().max().item())
            bnd = max(e_pose[rows].max().item(), e_ref[rows].max().item())
            w = worst.setdefault(a, [0.0, 0.0])
            w[0], w[1] = max(w[0], err), max(w[1], bnd)
    assert max(worst) == 2, "L = 3 K: an entry lives through at most three pushes"
    for a, (err, bnd) in sorted(worst.items()):
        report("sequence (%s) entries pushed %d frames ago" % (way, a), err=err, bound=bnd)


@pytest.mark.parametrize("R", [1, 37, 2836])
def test_posemb3d_against_float64(hip_lib, R):
    from far3d_amd import ops
    g = torch.Generator().manual_seed(R)
    pos = torch.rand(R, 3, generator=g) * 2 - 0.5            # reference points do leave [0, 1]
    pos[0] = torch.tensor([0.0, 1.0, 0.25])
    if R > 2:
        pos[1], pos[2] = torch.tensor([1.0, 0.0, 1.0]), torch.zeros(3)
    dt = hr.dim_t(128)
    got = ops.posemb3d(pos.to(DEV), dt.to(DEV)).cpu()
    want = hr.posemb3d(pos.double(), dt)
    y = hr.yard(hr.posemb3d(pos, dt), want)
    b = hr.chain_bound(y, want)
    e = within(got, want, b, "posemb3d R=%d" % R)
    report("posemb3d R=%d" % R, yard=y, bound=b, err=e[0])


@pytest.mark.parametrize("do_ln", [True, False])
@pytest.mark.parametrize("add", [None, "rows", "one"])
@pytest.mark.parametrize("gb", ["rows", "one"])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1544])
def test_row_affine_ln_against_float64(hip_lib, rows, gb, add, do_ln):
    """x, out (and the per-row gamma / beta) are row-strided views of wider buffers; the other columns of out's buffer stay untouched.
    do_ln off: pure affine, derived bound (g x + b + a: product + 2 adds = 3 roundings); on: the LayerNorm chain, yardstick rule."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(rows * 13 + (gb == "one") * 5 + (add is not None) * 3 + do_ln)
    C = 256
    xw = torch.randn(rows, C + 64, generator=g) * 1.7 + 0.3
    gbw = torch.randn(rows if gb == "rows" else 1, 2 * C, generator=g)
    aw = None if add is None else torch.randn(rows if add == "rows" else 1, C, generator=g)
    xd, gbd = xw.to(DEV), gbw.to(DEV)
    x_v, g_v, b_v = xd[:, 32:32 + C], gbd[:, :C], gbd[:, C:]
    if gb == "one":
        g_v, b_v = g_v[0].contiguous(), b_v[0].contiguous()       # 1-D single row
    ad = None if aw is None else aw.to(DEV)
    outw = torch.full((rows, C + 8), 7.0, device=DEV)
    ops.row_affine_ln(x_v, g_v, b_v, add=ad, do_ln=do_ln, out=outw[:, 4:4 + C])
    ow = outw.cpu()
    assert bool((ow[:, :4] == 7.0).all()) and bool((ow[:, 4 + C:] == 7.0).all()), "columns outside the view were written"
    got = ow[:, 4:4 + C]
    x, ga, be = xw[:, 32:32 + C], gbw[:, :C], gbw[:, C:]
    want = hr.row_affine_ln(x.double(), ga.double(), be.double(), None if aw is None else aw.double(), do_ln)
    tag = "row_affine_ln rows=%d gamma=%s add=%s ln=%d" % (rows, gb, add, do_ln)
    if do_ln:
        y = hr.yard(hr.row_affine_ln(x, ga, be, aw, True), want)
        b = hr.chain_bound(y, want)
        e = within(got, want, b, tag)
        report(tag, yard=y, bound=b, err=e[0])
    else:
        b = 2 * 3 * U * ((ga.double() * x.double()).abs() + be.double().abs() + (aw.double().abs() if aw is not None else 0.0))
        e = within(got, want, b, tag)
        report(tag, err=e[0], bound=e[1])


def test_row_affine_ln_constant_and_offset_rows(hip_lib):
    """A constant row has variance 0: the normalised row is exactly 0 (the tree sum of 256 equal values and the division by 256 are
    exact), so out = beta.  Rows of 1e3 + unit noise: the variance must come from the centred values (two passes); a one-pass
    E[x^2] - E[x]^2 in fp32 loses all of it (1e6 against 1)."""
    from far3d_amd import ops
    g = torch.Generator().manual_seed(4)
    C, R = 256, 64
    ga, be = torch.randn(R, C, generator=g), torch.randn(R, C, generator=g)
    const = torch.full((R, C), 0.37) * torch.arange(1, R + 1)[:, None]
    got = ops.row_affine_ln(const.to(DEV), ga.to(DEV), be.to(DEV)).cpu()
    assert torch.equal(got, be), "constant rows: out must be beta exactly"
    off = 1e3 + torch.randn(R, C, generator=g)
    got = ops.row_affine_ln(off.to(DEV), ga.to(DEV), be.to(DEV)).cpu()
    want = hr.row_affine_ln(off.double(), ga.double(), be.double())
    y = hr.yard(hr.row_affine_ln(off, ga, be), want)
    b = hr.chain_bound(y, want)
    e = within(got, want, b, "row_affine_ln offset rows")
    report("row_affine_ln 1e3 + noise", yard=y, bound=b, err=e[0])


@pytest.mark.parametrize("ncls", [1, 10, 26])
@pytest.mark.parametrize("code", [8, 10])
@pytest.mark.parametrize("A", [1, 300, 2188])
@pytest.mark.parametrize("layers", [1, 6])
def test_head_finalize_arithmetic_against_float64(hip_lib, layers, A, code, ncls):
    from far3d_amd import ops
    g = torch.Generator().manual_seed(layers * 1000 + A + code + ncls)
    ref = torch.rand(A, 3, generator=g)
    reg = torch.randn(layers, A, code, generator=g) * 2
    cls = torch.randn(layers, 1, A, ncls, generator=g) * 3
    special = torch.tensor([[0.0, 1.0, 5e-6], [1.0, 0.0, 1.0 - 2e-6], [-0.3, 1.2, 9.9e-6], [1e-5, 0.5, 2.0]])
    ref[:min(A, 4)] = special[:min(A, 4)]
    reg[0, 0, :3] = torch.tensor([30.0, -30.0, 30.0])                 # saturated sigmoid
    if A > 8:
        reg[-1, 5, :3], reg[-1, 6, :3] = torch.tensor([-30.0, 30.0, -30.0]), torch.tensor([30.0, 30.0, 30.0])
        ref[6] = torch.tensor([1.0, 0.0, 0.5])
        cls[-1, 0, 7, 0], cls[-1, 0, 8, ncls - 1] = 20.0, 20.0           # the row maximum in the first / the last class
    cls_d = cls.to(DEV)
    box_d, score_d = ops.head_finalize(reg.reshape(-1, code).to(DEV), ref.to(DEV), cls_d, PC, layers, ncls)
    box, score = box_d.cpu().reshape(layers, A, code), score_d.cpu()
    assert torch.equal(cls_d.cpu(), cls), "without a hole the logits are read only"
    assert torch.equal(box[..., 3:], reg[..., 3:]), "channels 3.. are copies"
    wb, ws = hr.finalize(reg.double(), ref.double(), cls[-1, 0].double(), PC)
    fb, fs = hr.finalize(reg, ref, cls[-1, 0], PC)
    tag = "finalize layers=%d A=%d code=%d ncls=%d" % (layers, A, code, ncls)
    yb, ys = hr.yard(fb[..., :3], wb[..., :3]), hr.yard(fs, ws)
    bb, bs = hr.chain_bound(yb, wb[..., :3]), hr.chain_bound(ys, ws)
    eb = within(box[..., :3], wb[..., :3], bb, tag + " xyz")
    es = within(score, ws, bs, tag + " score")
    if A > 8:
        assert abs(score[7].item() - 1 / (1 + math.exp(-20.0))) < 1e-6 and abs(score[8].item() - 1 / (1 + math.exp(-20.0))) < 1e-6, tag
    report(tag, xyz_yard=yb, xyz_bound=bb, xyz_err=eb[0], score_yard=ys, score_bound=bs, score_err=es[0])


def test_wrappers_refuse_what_the_kernels_cannot_take(hip_lib):
    """The kernels index dense (L, ..) buffers and 256 dense channels: the wrappers refuse everything else with ValueError before any
    launch."""
    from far3d_amd import ops
    mc = hr.memory_case(48, 256, 16, "steady", "synthetic")
    st = to_dev_mem(mc["state"])
    T = torch.tensor([1.0], dtype=torch.float64, device=DEV)
    dt256, ego, pseudo = hr.dim_t(256).to(DEV), mc["ego_inv"].to(DEV), mc["pseudo_ref"].to(DEV)
    wide = torch.zeros(1, 48, 512, device=DEV)
    with pytest.raises(ValueError):
        ops.memory_prepare(dict(st, emb=wide[:, :, :256]), ego, T, pseudo, dt256, 1.0, False, PC, 16)          # non-contiguous state
    with pytest.raises(ValueError):
        ops.memory_prepare(dict(st, velo=torch.zeros(1, 47, 2, device=DEV)), ego, T, pseudo, dt256, 1.0, False, PC, 16)
    with pytest.raises(ValueError):
        ops.memory_prepare(st, ego, T, pseudo, dt256, 1.0, False, PC, 49)                                        # P > L
    with pytest.raises(ValueError):
        ops.memory_prepare(st, ego, T, pseudo[:8], dt256, 1.0, False, PC, 16)                                    # fewer pseudo points than P
    m, _, _, _ = ops.memory_prepare(st, ego, T, pseudo, dt256, 1.0, False, PC, 16)
    dec, box, idx = push_inputs(60, 256, 10, 49, seed=1)
    with pytest.raises(ValueError):
        ops.memory_post_update(m, idx.to(DEV), dec.to(DEV), box.to(DEV), ego, T, st)                             # K = 49 > L = 48
    with pytest.raises(ValueError):
        ops.memory_post_update(m, idx[:16].to(DEV), dec.to(DEV), box.to(DEV), ego, T, m)                         # in place
    with pytest.raises(ValueError):
        ops.memory_post_update(m, idx[:16].to(DEV), dec[:, :128].contiguous().to(DEV), box.to(DEV), ego, T, st)  # E mismatch
    with pytest.raises(ValueError):
        ops.memory_post_update(dict(m, pose=m["pose"].transpose(2, 3)), idx[:16].to(DEV), dec.to(DEV), box.to(DEV), ego, T, st)
    x = torch.randn(8, 512, device=DEV)
    gm, bt = torch.ones(256, device=DEV), torch.zeros(256, device=DEV)
    with pytest.raises(ValueError):
        ops.row_affine_ln(x[:, ::2], gm, bt)                                                                     # channel stride 2
    with pytest.raises(ValueError):
        ops.row_affine_ln(x[:, :256], torch.ones(3, 256, device=DEV), torch.zeros(3, 256, device=DEV))           # 3 gamma rows for 8 rows
    with pytest.raises(ValueError):
        ops.row_affine_ln(x[:, :256], gm, bt, out=torch.empty(7, 256, device=DEV))
    from far3d_amd import lib
    with pytest.raises(lib.Far3dHipError):
        ops.row_affine_ln(x[:, :128], gm[:128], bt[:128])                                                        # C != 256: refused by the ABI

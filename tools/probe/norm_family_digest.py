"""The normalisation family with TWO builds of the library in one process: the one of another commit (--parent-lib, built from a
checkout of that commit) and this tree's, on the same inputs, compared bit for bit (torch.equal).

  python tools/probe/norm_family_digest.py --parent-lib /path/to/other/libfar3d_hip.so [--out profiles/norm_core/digest.txt]
  python tools/probe/norm_family_digest.py --parent-lib ... --time [--out profiles/norm_core/times.txt] [--rounds 5]

Entries: far3d_layernorm / far3d_layernorm_rows, far3d_row_affine_ln, far3d_ese_nhwc, far3d_ese_fused_nhwc, far3d_groupnorm_nhwc,
far3d_maxpool3x3s2_nhwc, far3d_cam_embed_chain and the four row chains.  The inputs are small; each shape is there for one place a kernel
can go wrong (a row count that is no multiple of the four rows of a workgroup, C past one float4 per lane, channel slices, the
fixed-point channel sums, a pooled edge that needs the ceil-mode window).  Both libraries are called through the same wrappers:
far3d_amd.lib's handle is exchanged between the two runs of a case.  Outputs that a case writes into a wider buffer start from a fill,
so what lies outside the slice is compared too.  The file written holds one line per case, not the tensors.

--time: hipGraph replay (vov_family_times.graph_us) of the frame's own shapes, the two libraries alternating, five repetitions per side;
per shape the mean and the spread (max - min) of either side, and whether this tree's mean exceeds the parent's by more than the larger
spread.  It is for kernels whose machine code differs from the other commit's; with identical code there is nothing to time."""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools", "probe"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"
FILL = 7.0
REPS = 5


def _rand(*shape, seed=0, scale=1.0):
    import torch
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _store(x, dt):
    import torch
    from far3d_amd import ops
    return ops.pair_from_float(x) if dt == "pair" else x.to(torch.bfloat16) if dt == "bf16" else x


def _logical(xs, dt):
    from far3d_amd import ops
    return ops.pair_to_float(xs) if dt == "pair" else xs.float()


def _fixed_sums(xs, dt):
    """far3d_conv2d_nhwc's chan_sums of a stored map, filled by hand: round(sum over H*W * 2^18), int64 [N][C]."""
    import torch
    v = _logical(xs, dt).double().sum(dim=(1, 2))
    return torch.round(v * (1 << 18)).to(torch.int64).contiguous()


def layernorm_cases():
    import torch
    from far3d_amd import ops
    for rows in (1, 5, 1544):
        for C in (12, 256, 260, 1024):
            x, g, b, add = _rand(rows, C, seed=rows + C), 1 + 0.1 * _rand(C, seed=1), 0.1 * _rand(C, seed=2), _rand(rows, C, seed=3)
            wide = _rand(rows, 3 * C, seed=rows + C + 1)
            perm = torch.randperm(rows, generator=torch.Generator().manual_seed(rows)).to(torch.int32).to(DEV)
            tag = "layernorm rows=%d C=%d " % (rows, C)
            buf = lambda dtype, cols=C: torch.full((rows, cols), FILL, dtype=dtype, device=DEV)
            yield tag + "no gamma/beta", lambda: [ops.layernorm(x, None, None)]
            yield tag + "relu", lambda: [ops.layernorm(x, g, b, act="relu")]
            yield tag + "y2 f32", lambda: list(ops.layernorm(x, g, b, add=add))
            yield tag + "y2 bf16", lambda: list(ops.layernorm(x, g, b, add=add, add_dtype=torch.bfloat16))
            yield tag + "yb", lambda: list(ops.layernorm(x, g, b, bf16_copy=True))

            def strided():
                out, xw = buf(torch.float32, 2 * C), buf(torch.bfloat16, 2 * C)
                ops.layernorm(wide[:, C:2 * C], g, b, out=out[:, C:], add=wide[:, 2 * C:], y2=xw[:, :C], yb=xw[:, C:])
                return [out, xw]
            yield tag + "row-strided views", strided

            def permuted():
                y2, yb = buf(torch.float32), buf(torch.bfloat16)
                return [ops.layernorm(x, g, b, add=add, y2=y2, yb=yb, out_rows=perm)[0], y2, yb]
            yield tag + "out_rows permutation", permuted


def row_affine_cases():
    from far3d_amd import ops
    C = 256
    for rows in (1, 5):
        x = _rand(rows, C, seed=10 + rows)
        per = [_rand(rows, C, seed=20 + i) for i in range(3)]
        one = [_rand(C, seed=30 + i) for i in range(3)]
        for name, (g, b, a) in (("per-row", per), ("single-row", one)):
            for do_ln in (0, 1):
                yield "row_affine_ln rows=%d %s gamma/beta/add do_ln=%d" % (rows, name, do_ln), \
                    (lambda g=g, b=b, a=a, do_ln=do_ln: [ops.row_affine_ln(x, g, b, add=a, do_ln=bool(do_ln))])
                yield "row_affine_ln rows=%d %s gamma/beta, no add, do_ln=%d" % (rows, name, do_ln), \
                    (lambda g=g, b=b, do_ln=do_ln: [ops.row_affine_ln(x, g, b, do_ln=bool(do_ln))])


def ese_cases():
    import torch
    from far3d_amd import ops
    N, H, W = 2, 13, 17
    for dt in ("f32", "bf16", "pair"):
        for C in (64, 768):
            xs = _store(_rand(N, H, W, C, seed=C), dt)
            fcw, fcb = _rand(C, C, seed=C + 1, scale=C ** -0.5), _rand(C, seed=C + 2, scale=0.1)
            cs = xs.shape[3]
            wide = _store(_rand(N, H, W, 2 * C, seed=C + 3), dt)      # pair: [hi | lo] blocks of 32, so a 64-multiple slice is a map
            tag = "ese_nhwc %s 2x13x17 C=%d " % (dt, C)
            yield tag + "no identity", lambda: [ops.ese_nhwc(xs, fcw, fcb, pair=dt == "pair")]

            def sliced():
                out = torch.full((N, H, W, 2 * cs), FILL, dtype=xs.dtype, device=DEV)
                ops.ese_nhwc(xs, fcw, fcb, identity=wide[..., cs:], out=out[..., :cs], pair=dt == "pair")
                return [out]
            yield tag + "identity as a channel slice", sliced
            if dt != "f32":
                def fixed():
                    sums = _fixed_sums(xs, dt)
                    return [ops.ese_nhwc(xs, fcw, fcb, identity=wide[..., cs:], pair=dt == "pair", sums=sums), sums]
                yield tag + "hand-filled fixed-point sums", fixed


def ese_fused_cases():
    import torch
    from far3d_amd import ops
    N, H, W = 2, 13, 17
    Hp, Wp = ops.maxpool_out_hw(H, W)
    for dt in ("bf16", "pair"):
        for C in (256, 768):
            xs, idn = _store(_rand(N, H, W, C, seed=C), dt), _store(_rand(N, H, W, C, seed=C + 5), dt)
            fcw, fcb = _rand(C, C, seed=C + 1, scale=C ** -0.5), _rand(C, seed=C + 2, scale=0.1)
            for what in ("y", "pooled", "y and pooled"):
                for with_idn in (False, True):
                    def run(what=what, with_idn=with_idn):
                        sums = _fixed_sums(xs, dt)
                        gate = torch.full((N * C,), FILL, device=DEV)
                        out = torch.full_like(xs, FILL) if "y" in what.split() else None
                        pooled = torch.full((N, Hp, Wp, xs.shape[3]), FILL, dtype=xs.dtype, device=DEV) if "pooled" in what else None
                        ops.ese_fused_nhwc(xs, fcw, fcb, sums, gate, identity=idn if with_idn else None, out=out, pooled=pooled, pair=dt == "pair")
                        return [t for t in (out, pooled, gate, sums) if t is not None]
                    yield "ese_fused_nhwc %s 2x13x17 C=%d %s%s" % (dt, C, what, ", identity" if with_idn else ""), run


def groupnorm_cases():
    from far3d_amd import ops
    for dt, C in (("f32", 256), ("bf16", 256), ("pair", 256), ("f32", 64), ("bf16", 64)):
        xs = _store(_rand(2, 5, 7, C, seed=C), dt)
        g, b = 1 + 0.1 * _rand(C, seed=1), 0.1 * _rand(C, seed=2)
        yield "groupnorm_nhwc %s 2x5x7x%d, 32 groups" % (dt, C), (lambda xs=xs, g=g, b=b, dt=dt: [ops.groupnorm_nhwc(xs, g, b, 32, pair=dt == "pair")])


def maxpool_cases():
    import torch
    from far3d_amd import ops
    for H, W in ((8, 9), (17, 23)):
        Ho, Wo = ops.maxpool_out_hw(H, W)
        for dt in ("f32", "bf16", "pair"):
            xs = _store(_rand(2, H, W, 64, seed=H), dt)
            cs = xs.shape[3]
            yield "maxpool3x3s2_nhwc %s 2x%dx%dx64" % (dt, H, W), (lambda xs=xs, dt=dt: [ops.maxpool3x3s2_nhwc(xs, pair=dt == "pair")])

            def sliced(xs=xs, dt=dt, cs=cs, Ho=Ho, Wo=Wo):
                out = torch.full((2, Ho, Wo, 3 * cs), FILL, dtype=xs.dtype, device=DEV)
                ops.maxpool3x3s2_nhwc(xs, out=out[..., cs:2 * cs], pair=dt == "pair")
                return [out]
            yield "maxpool3x3s2_nhwc %s 2x%dx%dx64 into a channel slice" % (dt, H, W), sliced


def cam_embed_cases():
    from far3d_amd import ops
    N, L, J, Hd = 5, 3, 416, 128
    p = dict(w0t=_rand(L, 12, Hd, seed=1, scale=0.3), b0=_rand(L, Hd, seed=2, scale=0.1), w2t=_rand(L, Hd, 256, seed=3, scale=Hd ** -0.5),
             b2=_rand(L, 256, seed=4, scale=0.1), ln_g=1 + 0.1 * _rand(L, 256, seed=5), ln_b=0.1 * _rand(L, 256, seed=6),
             w3t=_rand(L, 256, J, seed=7, scale=1 / 16), b3=_rand(L, J, seed=8, scale=0.1))
    l2i = _rand(N, 4, 4, seed=9)
    yield "cam_embed_chain N=5 L=3 J=416 Hd=128 ld=16", lambda: [ops.cam_embed_chain(l2i, p)]
    yield "cam_embed_chain N=5 L=3 J=416 Hd=128 ld=12", lambda: [ops.cam_embed_chain(l2i[:, :3, :].reshape(N, 12).contiguous(), p)]


def rowchain_cases():
    """The four row chains with the inputs of tests/test_rowchain_gpu.py."""
    import torch
    from far3d_amd import ops
    import test_rowchain_gpu as T
    E = T.E
    ly, nxt = T._layer(5), T._layer(6)
    cls, lns, reg, rb = T._branches(21)
    for M in (1, 16, 37):
        att, x, qpos = T._inputs(M, M, wide=M == 37)

        def attn_out(att=att, x=x, qpos=qpos, M=M):
            x1, ul = torch.full((M, E), FILL, device=DEV), torch.full((M, 512), FILL, device=DEV)
            ops.rowchain_attn_out(att, x, qpos, ly["rc"], x1, ul)
            return [x1, ul]
        yield "rowchain_attn_out M=%d" % M, attn_out

        def ffn(att=att, x=x, qpos=qpos, M=M):
            out, qkv = torch.full((M, E), FILL, device=DEV), torch.full((M, 3 * E), FILL, dtype=torch.bfloat16, device=DEV)
            xop = torch.full((M, 2 * E), FILL, dtype=torch.bfloat16, device=DEV)
            ops.rowchain_ffn(att, x, qpos, ly["rc"], out, nxt=nxt["rc"], qkv=qkv, xop=xop)
            return [out, qkv, xop]
        yield "rowchain_ffn M=%d" % M, ffn

        def qkv_alone(x=x, qpos=qpos, M=M):
            return [ops.rowchain_qkv(x, qpos, nxt["rc"], torch.full((M, 3 * E), FILL, dtype=torch.bfloat16, device=DEV))]
        yield "rowchain_qkv M=%d" % M, qkv_alone

        def branches(att=att, M=M):
            co, ro = torch.full((M, rb.n_cls), FILL, device=DEV), torch.full((M, rb.n_reg), FILL, device=DEV)
            ops.rowchain_branches(att, rb, co, ro)
            return [co, ro]
        yield "rowchain_branches M=%d" % M, branches


FAMILY = (layernorm_cases, row_affine_cases, ese_cases, ese_fused_cases, groupnorm_cases, maxpool_cases, cam_embed_cases, rowchain_cases)


def timed_cases():
    """The frame's own shapes (seven 640x960 cameras, V-99, 1544 decoder rows) of the kernels that have a shape of their own."""
    import torch
    from far3d_amd import ops
    rows, C = 1544, 256
    x, g, b, add = _rand(rows, C), 1 + 0.1 * _rand(C, seed=1), 0.1 * _rand(C, seed=2), _rand(rows, C, seed=3)
    y, xw = torch.empty(rows, C, device=DEV), torch.empty(rows, 2 * C, dtype=torch.bfloat16, device=DEV)
    yield "layernorm 1544x256, y2 + yb", lambda: ops.layernorm(x, g, b, out=y, add=add, y2=xw[:, :C], yb=xw[:, C:])
    gr, br = _rand(rows, C, seed=4), _rand(rows, C, seed=5)
    yield "row_affine_ln 1544x256", lambda: ops.row_affine_ln(x, gr, br, out=y)
    xs = _rand(7, 80, 120, 256).to(torch.bfloat16)
    go, scratch = torch.empty_like(xs), torch.empty(ops.ese_scratch_floats(7, 256), device=DEV)
    yield "groupnorm_nhwc bf16 7x80x120x256", lambda: ops.groupnorm_nhwc(xs, g, b, 32, out=go, scratch=scratch)
    xe = _rand(7, 40, 60, 768).to(torch.bfloat16)
    fcw, fcb = _rand(768, 768, scale=768 ** -0.5), _rand(768, scale=0.1)
    eo, es = torch.empty_like(xe), torch.empty(ops.ese_scratch_floats(7, 768), device=DEV)
    yield "ese_nhwc bf16 7x40x60x768", lambda: ops.ese_nhwc(xe, fcw, fcb, out=eo, scratch=es)
    Ho, Wo = ops.maxpool_out_hw(160, 240)
    xm = _rand(7, 160, 240, 256).to(torch.bfloat16)
    mo = torch.empty(7, Ho, Wo, 256, dtype=torch.bfloat16, device=DEV)
    yield "maxpool3x3s2_nhwc bf16 7x160x240x256", lambda: ops.maxpool3x3s2_nhwc(xm, out=mo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    from far3d_amd import lib
    mine = lib.load()
    parent = ctypes.CDLL(a.parent_lib)
    for name, (res, args) in lib.SIGNATURES.items():
        if hasattr(parent, name):
            getattr(parent, name).restype, getattr(parent, name).argtypes = res, args
    sides = (("parent", parent), ("new", mine))
    L = []
    try:
        if a.time:
            from vov_family_times import graph_us
            L += ["the other commit's library (parent) against this tree's (new) in one process, hipGraph replay, %d alternating repetitions;" % REPS,
                  "mean us [spread = max - min]; bar: new mean - parent mean <= the larger spread", ""]
            for name, fn in timed_cases():
                us = {"parent": [], "new": []}
                for _ in range(REPS):
                    for side, handle in sides:
                        lib._lib = handle
                        us[side].append(graph_us(fn, 10, a.rounds)[0])
                p, n = us["parent"], us["new"]
                pm, ps, nm, ns = sum(p) / REPS, max(p) - min(p), sum(n) / REPS, max(n) - min(n)
                L.append("%-40s parent %9.2f [%5.2f]  new %9.2f [%5.2f]  new - parent %+7.2f  %s" %
                         (name, pm, ps, nm, ns, nm - pm, "met" if nm - pm <= max(ps, ns) else "MISSED"))
                print(L[-1], flush=True)
        else:
            differ = 0
            for family in FAMILY:
                n = same = 0
                for name, fn in family():
                    outs = {}
                    for side, handle in sides:
                        lib._lib = handle
                        outs[side] = [t.clone() for t in fn()]
                        torch.cuda.synchronize()
                    ok = len(outs["parent"]) == len(outs["new"]) and all(torch.equal(p, q) for p, q in zip(outs["parent"], outs["new"]))
                    finite = all(torch.isfinite(t.float()).all().item() for t in outs["new"])
                    n, same = n + 1, same + ok
                    L.append("%-5s %s%s" % ("same" if ok else "DIFFER", name, "" if finite else "  (non-finite values)"))
                    print(L[-1], flush=True)
                differ += n - same
                L.append("-- %s: %d of %d cases equal bit for bit" % (family.__name__, same, n))
                print(L[-1], flush=True)
            L.append("== %d cases differ" % differ)
            print(L[-1])
    finally:
        lib._lib = mine
    out = a.out or os.path.join(ROOT, "profiles", "norm_core", "times.txt" if a.time else "digest.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(L) + "\n")
    return 1 if (not a.time and differ) else 0


if __name__ == "__main__":
    sys.exit(main())

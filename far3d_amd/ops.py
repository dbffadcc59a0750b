"""Tensor-level wrappers over the C-ABI: checks + allocation + raw pointers, nothing else.

Every function launches on torch's *current* HIP stream of the tensors' device (so torch.cuda
events / graphs see the kernels) and never synchronises.
"""
import contextlib
import ctypes
import functools
import json
import os
import threading

import numpy as np
import torch

from . import lib as _lib

DT_F32, DT_BF16 = 0, 1
DT_F32_BF16X3 = 2       # FAR3D_DT_F32_BF16X3: conv weight code "fp32 data, two-term bf16 split products"
DT_BF16_PAIR = 3        # FAR3D_DT_BF16_PAIR: activations stored split, [32 hi | 32 lo] bf16 per 32-channel block


# ---- pair storage (include/far3d_hip.h FAR3D_DT_BF16_PAIR): a map of C logical channels (C % 32 == 0) is a bf16 tensor with 2C
# channels; every 32-channel block is 32 hi = bf16(x) then 32 lo = bf16(x - hi), so hi + lo carries 16 significant bits.
def pair_from_float(t):
    """(..., C) f32 -> (..., 2C) bf16 pair storage."""
    C = t.shape[-1]
    if C % 32:
        raise ValueError("pair storage needs C %% 32 == 0 (got %d)" % C)
    b = t.float().reshape(t.shape[:-1] + (C // 32, 32))
    hi = b.to(torch.bfloat16)
    lo = (b - hi.float()).to(torch.bfloat16)
    return torch.cat([hi, lo], dim=-1).reshape(t.shape[:-1] + (2 * C,)).contiguous()


def pair_to_float(t):
    """(..., 2C) bf16 pair storage -> (..., C) f32 (exact: hi + lo)."""
    C2 = t.shape[-1]
    b = t.reshape(t.shape[:-1] + (C2 // 64, 2, 32)).float()
    return (b[..., 0, :] + b[..., 1, :]).reshape(t.shape[:-1] + (C2 // 2,))


def _dt(t):
    if t.dtype == torch.float32:
        return DT_F32
    if t.dtype == torch.bfloat16:
        return DT_BF16
    raise TypeError("far3d_amd: unsupported dtype %s (float32 / bfloat16 only)" % t.dtype)


def _chk(t, name, dtype=None, ndim=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.Far3dHipError("%s must live on a HIP device (got %s); there is no CPU path" % (name, t.device))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if dtype is not None and t.dtype != dtype:
        raise TypeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s must have %d dims (got %s)" % (name, ndim, tuple(t.shape)))
    return t


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _host_i32(vals):
    a = np.ascontiguousarray(np.asarray(vals, dtype=np.int32))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _host_f32(vals):
    a = np.ascontiguousarray(np.asarray(vals, dtype=np.float32))
    return a, a.ctypes.data_as(ctypes.c_void_p)


def _hole(hole):
    """hole: None or (count int32 device tensor (1,), start, end): the query rows [start + count, end) hold no query (fixed-capacity
    proposal mode, far3d_hip.h far3d_proposal_gather).  -> (pointer | None, start, end) C arguments."""
    if hole is None:
        return None, 0, 0
    cnt, start, end = hole
    _chk(cnt, "hole count", torch.int32)
    return _ptr(cnt), int(start), int(end)


def msda_forward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step=64):
    """mmcv `ms_deform_attn_forward` contract (reference call site detr3d_transformer.py:561-563).

    value (bs,S,H,Dh) f32|bf16; spatial_shapes (L,2) i64; level_start_index (L,) i64;
    sampling_locations (bs,Q,H,L,P,2) f32; attention_weights (bs,Q,H,L,P) or (bs,Q,H,L*P) f32.
    Returns (bs,Q,H*Dh) f32.
    """
    lib = _lib.require_device()
    _chk(value, "value", ndim=4)
    _chk(spatial_shapes, "value_spatial_shapes", torch.int64, 2)
    _chk(level_start_index, "value_level_start_index", torch.int64, 1)
    _chk(sampling_locations, "sampling_locations", torch.float32, 6)
    _chk(attention_weights, "attention_weights", torch.float32)
    bs, S, H, Dh = value.shape
    _, Q, H2, L, P, two = sampling_locations.shape
    if H2 != H or two != 2 or sampling_locations.shape[0] != bs:
        raise ValueError("sampling_locations shape %s inconsistent with value %s" %
                         (tuple(sampling_locations.shape), tuple(value.shape)))
    if attention_weights.numel() != bs * Q * H * L * P:
        raise ValueError("attention_weights shape %s != (bs,Q,H,L*P)" % (tuple(attention_weights.shape),))
    if spatial_shapes.shape[0] != L or level_start_index.shape[0] != L:
        raise ValueError("spatial_shapes/level_start_index must have L=%d rows" % L)
    step = min(bs, im2col_step)
    if step > 0 and bs % step != 0:  # mmcv asserts the same
        raise RuntimeError("batch(%d) must divide im2col_step(%d)" % (bs, step))
    out = torch.empty((bs, Q, H * Dh), dtype=torch.float32, device=value.device)
    _lib.check(lib.far3d_msda_forward(_ptr(value), _dt(value), _ptr(spatial_shapes), _ptr(level_start_index),
                                      _ptr(sampling_locations), _ptr(attention_weights), _ptr(out),
                                      bs, S, H, Dh, L, Q, P, _stream(value)), "far3d_msda_forward")
    return out


def agg_tables(Vc, out=None):
    """Softmax factors of the camera part of the aggregation logits (far3d_agg_tables): Vc (layers, N, J) or (N, J) f32 ->
    (layers, 2 + N, J) / (2 + N, J) f32 = [max over cameras | sum of exp | exp(Vc - max)].  Per frame, for all layers at once."""
    lib = _lib.require_device()
    _chk(Vc, "Vc", torch.float32)
    v3 = Vc if Vc.dim() == 3 else Vc[None]
    Ls, N, J = v3.shape
    tab = out if out is not None else torch.empty((Ls, 2 + N, J), dtype=torch.float32, device=Vc.device)
    _lib.check(lib.far3d_agg_tables(_ptr(v3), _ptr(tab), Ls, N, J, _stream(Vc)), "far3d_agg_tables")
    return tab if Vc.dim() == 3 else tab[0]


class AggSplit:
    """Workspace of far3d_aggregate_forward variant 9 (sibling workgroups for heavy queries): partial sums [rows][2][256] f32, arrival
    tickets [rows] int32 (zero at rest) and the number of sibling slots far3d_agg_order may hand out."""

    def __init__(self, rows, extra=384, device="cuda:0"):
        self.rows, self.extra = int(rows), int(extra)
        self.partials = torch.empty((self.rows, 2, 256), dtype=torch.float32, device=device)
        self.tickets = torch.zeros((self.rows,), dtype=torch.int32, device=device)


class AggLists:
    """Workspace of far3d_aggregate_forward variant 13 (the two-kernel split, A/B only): FAR3D_AGG_LISTS_FLOATS(A) floats of row lists +
    softmax denominators, 2 * 8 * ceil(A / 8) int32 of per-wave entry counts."""

    def __init__(self, A, device):
        slots = -(-A // 8) * 8
        self.rows = A
        self.buf = torch.zeros((slots * (2 * 1024 * 9 + 8),), dtype=torch.float32, device=device)
        self.counts = torch.zeros((slots * 2,), dtype=torch.int32, device=device)


def _agg_host_operands(who, Vc, tables, kernel8, tab_shape, tab_name, level_hw, level_start, pc_range):
    """What aggregate_forward and aggregate_batched hand the library besides tensors: the tables (agg_tables(Vc) when kernel 8 will
    run and the caller passed none; checked against tab_shape) and the host arrays level_hw / level_start / pc_range.
    Returns (tables, keep-alive, level_hw pointer, level_start pointer, pc_range pointer)."""
    if tables is None and kernel8:
        tables = agg_tables(Vc)
    if tables is not None:
        _chk(tables, "tables", torch.float32, len(tab_shape))
        if tuple(tables.shape) != tab_shape:
            raise ValueError("%s: tables must be %s = %s, got %s" % (who, tab_name, tab_shape, tuple(tables.shape)))
    hw_keep, hw_p = _host_i32([list(x) for x in level_hw])
    st_keep, st_p = _host_i32(list(level_start))
    pc_keep, pc_p = _host_f32(list(pc_range))
    return tables, (hw_keep, st_keep, pc_keep), hw_p, st_p, pc_p


def aggregate_forward(feat, ref, offsets, lidar2img, U, Vc, level_hw, level_start, pc_range, pad_hw,
                      num_groups=8, out=None, perm=None, out_dtype=torch.float32, variant=0, tables=None, split=None, qbase=None, lists=None):
    """Fused perspective-aware aggregation for ONE sample (B=1).

    feat (N,S,256) f32|bf16 token-major value maps; ref (A,3) f32 normalised reference points;
    offsets (A,P,3) f32 = learnable_fc(x); lidar2img (N,4,4) f32; U (A,L*P*G) f32 query part of the
    attention logits; Vc (N,L*P*G) f32 camera part (incl. bias); level_hw [(H,W)]*L; level_start [L];
    pc_range 6 floats; pad_hw (H,W) of the padded image.  Returns (A,256) f32 = sum over cameras of
    MSDA(feat_n, project_n(ref+offsets), softmax_{n,l,p}(U+Vc)).  U / offsets may be row-strided views (unit inner stride)
    only through .contiguous() -- the kernel reads dense rows.  variant: see include/far3d_hip.h (0 = default).
    tables: agg_tables(Vc) (2+N, L*P*G) -- the per-frame softmax factors the default kernel reads instead of Vc; computed here
    (one more launch) when the default kernel runs and the caller did not pass them.
    qbase: aggregation_order(..., sorted_operands=True)'s (A, 4) table -- SORTED mode of the default kernel: U and offsets hold the
    query of perm entry e at row e (their producers stored through the order's `inv`), ref is not read; same bits as the unsorted call.
    """
    lib = _lib.require_device()
    _chk(feat, "feat", ndim=3)
    _chk(ref, "ref", torch.float32, 2)
    _chk(lidar2img, "lidar2img", torch.float32, 3)
    _chk(Vc, "Vc", torch.float32, 2)
    N, S, C = feat.shape
    A = ref.shape[0]
    L = len(level_hw)
    G = num_groups
    if offsets.dim() == 3:
        offsets = offsets.reshape(A, -1)
    for t, n in ((U, "U"), (offsets, "offsets")):     # row-strided views are fine (column blocks of a merged-GEMM output)
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and (A == 0 or t.stride(1) == 1)):
            raise ValueError("aggregate_forward: %s must be a 2-D f32 device tensor with unit inner stride" % n)
    P = offsets.shape[1] // 3
    if U.shape != (A, L * P * G) or Vc.shape != (N, L * P * G) or lidar2img.shape != (N, 4, 4):
        raise ValueError("aggregate_forward: inconsistent shapes U%s Vc%s l2i%s (A=%d N=%d L=%d P=%d G=%d)" %
                         (tuple(U.shape), tuple(Vc.shape), tuple(lidar2img.shape), A, N, L, P, G))
    if out is None:
        out = torch.empty((A, C), dtype=out_dtype, device=feat.device)
    nperm = None
    if perm is not None:
        _chk(perm, "perm", torch.int32, 1)
        nperm = perm.numel() - (split.extra if split is not None else 0)        # main entries (the sibling entries follow them)
        if nperm > A or nperm < 0:
            raise ValueError("aggregate_forward: perm has more entries than there are rows")
    if split is not None:
        if perm is None or split.rows < A or variant not in (0, 9):
            raise ValueError("aggregate_forward: split needs the perm of aggregation_order(split=...), a workspace of >= A rows and variant 0 / 9")
        variant = 9
    if qbase is not None:
        _chk(qbase, "qbase", torch.float32, 2)
        if perm is None or split is not None or variant not in (0, 8, 13) or tuple(qbase.shape) != (nperm, 4) or nperm != A:
            raise ValueError("aggregate_forward: qbase (sorted mode) needs the full perm of aggregation_order(sorted_operands=True), "
                             "variant 0 / 8 / 13, no split and shape (A, 4)")
        variant = 13 if variant == 13 else 8
    if variant == 13:
        if qbase is None or lists is None or lists.rows < A:
            raise ValueError("aggregate_forward: variant 13 (two-kernel split) needs the sorted mode's qbase and an AggLists workspace of >= A rows")
    k8 = variant in (0, 8, 9, 12, 13) and A > 0 and aggregate_kernel8_applies(N, P, L, S, C, feat.element_size())
    tables, _keep, hw_p, st_p, pc_p = _agg_host_operands("aggregate_forward", Vc, tables, k8, (2 + N, L * P * G), "(2+N, L*P*G)",
                                                         level_hw, level_start, pc_range)
    _lib.check(lib.far3d_aggregate_forward(_ptr(feat), _dt(feat), _ptr(ref), _ptr(offsets), _ptr(lidar2img),
                                           _ptr(U), _ptr(Vc), _ptr(tables) if tables is not None else None,
                                           _ptr(perm) if perm is not None else None, _ptr(out), _dt(out),
                                           A if perm is None else nperm, N, S, C, G, P, L, hw_p, st_p, pc_p,
                                           float(pad_hw[0]), float(pad_hw[1]), U.stride(0) if A > 0 else 0,
                                           offsets.stride(0) if A > 0 else 0, int(variant),
                                           _ptr(split.partials) if split is not None else (_ptr(lists.buf) if lists is not None else None),
                                           _ptr(split.tickets) if split is not None else (_ptr(lists.counts) if lists is not None else None),
                                           split.extra if split is not None else 0, _ptr(qbase) if qbase is not None else None,
                                           _stream(feat)),
               "far3d_aggregate_forward")
    return out


# The shape family of far3d_aggregate_forward (include/far3d_hip.h: "Requires C=256, G=8, L<=4, N<=16, N*P<=256, N*P*L<=384").
AGG_FUSED_C, AGG_FUSED_G, AGG_FUSED_MAX_L, AGG_FUSED_MAX_N, AGG_FUSED_MAX_NP, AGG_FUSED_MAX_NLP = 256, 8, 4, 16, 256, 384


def aggregate_fused_supported(C, G, L, N, P):
    """Does far3d_aggregate_forward (aggregate_forward) take embed width C, G groups, L levels, N cameras and P points?  A host
    predicate: no device, no library.  The rules are the library's size checks, one for one."""
    C, G, L, N, P = int(C), int(G), int(L), int(N), int(P)
    return (C == AGG_FUSED_C and G == AGG_FUSED_G and 1 <= L <= AGG_FUSED_MAX_L and 1 <= N <= AGG_FUSED_MAX_N and P >= 1 and
            N * P <= AGG_FUSED_MAX_NP and N * P * L <= AGG_FUSED_MAX_NLP)


# Kernel 8 (the default kernel: factored softmax over agg_tables) and its sorted mode (csrc/sampling.hip: agg_kernel8_applies, AGG8_WCAM).
AGG_K8_MAX_N, AGG_K8_MAX_P, AGG_SORTED_MAX_LP = 8, 16, 52


def aggregate_kernel8_applies(N, P, L, S=None, C=256, esz=None):
    """Does variant 0 of far3d_aggregate_forward / far3d_aggregate_batched run kernel 8 (and read the tables of agg_tables) for N
    cameras, P points and L levels?  Otherwise it runs kernel 7, which reads Vc.  With the S tokens per camera and the element size
    esz (bytes) of the value maps the rule includes that one sample's maps stay below 4 GiB (kernel 8 forms 32-bit byte offsets).
    A host predicate: no device, no library.  The rule is the library's (agg_kernel8_applies, with the tables present), one for one."""
    N, P, L = int(N), int(P), int(L)
    ok = N <= AGG_K8_MAX_N and P <= AGG_K8_MAX_P and L <= AGG_FUSED_MAX_L
    if S is not None and esz is not None:
        ok = ok and N * int(S) * int(C) * int(esz) < (1 << 32)
    return ok


def aggregate_sorted_applies(N, P, L, S=None, C=256, esz=None):
    """Does far3d_aggregate_forward take the sorted mode's operands (qbase)?  Kernel 8's rule and L * P <= 52: a camera row of the
    query's weights has to fit the kernel's LDS slot.  A host predicate like aggregate_kernel8_applies; the library's rule, one for one."""
    return aggregate_kernel8_applies(N, P, L, S, C, esz) and int(L) * int(P) <= AGG_SORTED_MAX_LP


def _batch_rows(t, B, A, name, who):
    """(B,A,K) f32 device tensor -> its rows b*A + a as ONE (B*A,K) view with unit inner stride and any row stride, so that a column
    block of a merged-GEMM output stays a view; a tensor whose rows do not lie at one stride is copied."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and tuple(t.shape[:2]) == (B, A)):
        raise ValueError("%s: %s must be a (B,A,.) f32 device tensor" % (who, name))
    K = t.shape[2]
    if B * A == 0:
        return t.new_empty((0, K))
    if t.stride(2) != 1 or (B > 1 and t.stride(0) != A * t.stride(1)):
        t = t.contiguous()
    return t.as_strided((B * A, K), (t.stride(1), 1))      # keeps the view's storage offset


def _agg_batched(ref, offsets, lidar2img, U, Vc, who):
    """The operands of aggregate_forward with or without a batch dimension -> (B, A, N, ref (B,A,3), offsets (B*A,3P) row-strided,
    lidar2img (B,N,4,4), U (B*A,J) row-strided, Vc (B,N,J))."""
    _chk(ref, "ref", torch.float32)
    if ref.dim() == 2:
        ref, offsets, lidar2img, U, Vc = ref[None], offsets[None], lidar2img[None], U[None], Vc[None]
    if ref.dim() != 3 or ref.shape[2] != 3:
        raise ValueError("%s: ref must be (A,3) or (B,A,3), got %s" % (who, tuple(ref.shape)))
    B, A = ref.shape[:2]
    _chk(lidar2img, "lidar2img", torch.float32, 4)
    _chk(Vc, "Vc", torch.float32, 3)
    N = lidar2img.shape[1]
    if tuple(lidar2img.shape) != (B, N, 4, 4) or tuple(Vc.shape[:2]) != (B, N):
        raise ValueError("%s: inconsistent shapes ref%s l2i%s Vc%s" % (who, tuple(ref.shape), tuple(lidar2img.shape), tuple(Vc.shape)))
    if offsets.dim() == 4:
        offsets = offsets.reshape(B, A, -1)
    return B, A, N, ref, _batch_rows(offsets, B, A, "offsets", who), lidar2img, _batch_rows(U, B, A, "U", who), Vc


def aggregate_batched(feat, ref, offsets, lidar2img, U, Vc, level_hw, level_start, pc_range, pad_hw,
                      num_groups=8, out=None, out_dtype=torch.float32, tables=None, hole=None):
    """aggregate_forward for a batch of samples in ONE launch (far3d_aggregate_batched): the fused kernel with the sample as a second
    grid index.  feat (B*N,S,256) or (B,N,S,256) f32|bf16; ref (B,A,3); offsets (B,A,P,3) or (B,A,P*3); lidar2img (B,N,4,4);
    U (B,A,L*P*G); Vc (B,N,L*P*G) -- the batched operands agg_operands takes (or one sample's, without B); U / offsets may be
    row-strided views (column blocks of a merged-GEMM output; U's stride a multiple of 4 floats).  tables: agg_tables(Vc)
    (B, 2+N, L*P*G), computed here (one more launch) when kernel 8 applies and the caller did not pass them.  Returns (B,A,256) of
    out_dtype; out[b] has the bits of aggregate_forward on sample b, whatever B is.  The shape family is aggregate_fused_supported's.
    hole: None or (counts int32 device tensor (B,), start, end), the tuple attention_streams takes: sample b's rows
    [start + counts[b], end) hold no query (far3d_aggregate_batched_holes): zero rows, their operands are not read, and out[b] has the
    bits of aggregate_forward with perm = aggregation_order(hole=(counts[b:b + 1], start, end))."""
    lib = _lib.require_device()
    B, A, N, ref, offs, l2i, U2, Vc = _agg_batched(ref, offsets, lidar2img, U, Vc, "aggregate_batched")
    if hole is not None:
        cnt = hole[0]
        if not (isinstance(cnt, torch.Tensor) and cnt.is_cuda and cnt.dtype == torch.int32 and cnt.numel() == B and cnt.is_contiguous()):
            raise ValueError("aggregate_batched: the hole needs one count per sample (%d) as an int32 device tensor, got %s" %
                             (B, "%s %s" % (cnt.dtype, tuple(cnt.shape)) if isinstance(cnt, torch.Tensor) else type(cnt).__name__))
    _chk(feat, "feat")
    if feat.dim() == 4:
        feat = feat.reshape(-1, *feat.shape[2:])
    if feat.dim() != 3 or feat.shape[0] != B * N:
        raise ValueError("aggregate_batched: feat %s does not hold B*N = %d*%d maps (S, C)" % (tuple(feat.shape), B, N))
    _, S, C = feat.shape
    L, G = len(level_hw), int(num_groups)
    P = offs.shape[1] // 3
    J = L * P * G
    if offs.shape[1] != P * 3 or U2.shape[1] != J or Vc.shape[2] != J:
        raise ValueError("aggregate_batched: inconsistent shapes offsets%s U%s Vc%s (L=%d P=%d G=%d)" %
                         (tuple(offs.shape), tuple(U2.shape), tuple(Vc.shape), L, P, G))
    if out is None:
        out = torch.empty((B, A, C), dtype=out_dtype, device=feat.device)
    else:
        _chk(out, "out", ndim=3)
        if tuple(out.shape) != (B, A, C):
            raise ValueError("aggregate_batched: out must be (B,A,C) = %s, got %s" % ((B, A, C), tuple(out.shape)))
    k8 = B * A > 0 and aggregate_kernel8_applies(N, P, L, S, C, feat.element_size())
    tables, _keep, hw_p, st_p, pc_p = _agg_host_operands("aggregate_batched", Vc, tables, k8, (B, 2 + N, J), "(B, 2+N, L*P*G)",
                                                         level_hw, level_start, pc_range)
    args = (_ptr(feat), _dt(feat), _ptr(ref), _ptr(offs), _ptr(l2i), _ptr(U2), _ptr(Vc), _ptr(tables) if tables is not None else None,
            _ptr(out), _dt(out), B, A, N, S, C, G, P, L, hw_p, st_p, pc_p, float(pad_hw[0]), float(pad_hw[1]),
            U2.stride(0) if B * A > 0 else 0, offs.stride(0) if B * A > 0 else 0)
    if hole is None:
        _lib.check(lib.far3d_aggregate_batched(*args, _stream(feat)), "far3d_aggregate_batched")
    else:
        _lib.check(lib.far3d_aggregate_batched_holes(*args, *_hole(hole), _stream(feat)), "far3d_aggregate_batched_holes")
    return out


def agg_operands(ref, offsets, lidar2img, U, Vc, num_levels, num_groups, pc_range, pad_hw, expand=True, key_points=False):
    """The two MSDA operands of the aggregation in the reference's layout (far3d_agg_operands; reference detr3d_transformer.py:535-555).

    ref (B,A,3) f32 normalised reference points; offsets (B,A,P,3) or (B,A,P*3) f32; lidar2img (B,N,4,4) f32; U (B,A,L*P*G) f32;
    Vc (B,N,L*P*G) f32 -- or the one-sample tensors of aggregate_forward (no B).  U / offsets may be row-strided views.
    Returns (loc, weights): loc (B*N,A,G,L,P,2) f32 -- expand=False: the compact (B*N,A,P,2) -- and weights (B*N,A,G,L*P) f32, what
    msda_forward takes with bs = B*N.  key_points=True: also the key points in metres (B,A,P,3), as a third result."""
    lib = _lib.require_device()
    B, A, N, ref, offs, l2i, U2, Vc = _agg_batched(ref, offsets, lidar2img, U, Vc, "agg_operands")
    L, G = int(num_levels), int(num_groups)
    P = offs.shape[1] // 3
    J = L * P * G
    if offs.shape[1] != P * 3 or U2.shape[1] != J or Vc.shape[2] != J:
        raise ValueError("agg_operands: inconsistent shapes offsets%s U%s Vc%s (L=%d P=%d G=%d)" %
                         (tuple(offs.shape), tuple(U2.shape), tuple(Vc.shape), L, P, G))
    dev = ref.device
    loc = torch.empty((B * N, A, G, L, P, 2) if expand else (B * N, A, P, 2), dtype=torch.float32, device=dev)
    w = torch.empty((B * N, A, G, L * P), dtype=torch.float32, device=dev)
    kp = torch.empty((B, A, P, 3), dtype=torch.float32, device=dev) if key_points else None
    pc_keep, pc_p = _host_f32(list(pc_range))
    _lib.check(lib.far3d_agg_operands(_ptr(ref), _ptr(offs), _ptr(l2i), _ptr(U2), _ptr(Vc), _ptr(loc), _ptr(w),
                                      _ptr(kp) if kp is not None else None, B, A, N, G, P, L, pc_p, float(pad_hw[0]), float(pad_hw[1]),
                                      U2.stride(0), offs.stride(0), 1 if expand else 0,
                                      _stream(ref)), "far3d_agg_operands")
    return (loc, w, kp) if key_points else (loc, w)


def camera_sum(x, num_cams):
    """x (B*N, A, C) f32 -> (B, A, C) f32, the cameras of a sample added in ascending order (far3d_camera_sum)."""
    lib = _lib.require_device()
    _chk(x, "x", torch.float32, 3)
    N = int(num_cams)
    BN, A, C = x.shape
    if N < 1 or BN % N:
        raise ValueError("camera_sum: %d maps are not a multiple of %d cameras" % (BN, N))
    out = torch.empty((BN // N, A, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.far3d_camera_sum(_ptr(x), _ptr(out), BN // N, N, A, C, _stream(x)), "far3d_camera_sum")
    return out


def _level_tensor(v, device):
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=torch.int64).contiguous()
    return torch.tensor([list(r) if isinstance(r, (tuple, list)) else int(r) for r in v], dtype=torch.int64, device=device)


def aggregate_general(feat, ref, offsets, lidar2img, U, Vc, level_hw, level_start, pc_range, pad_hw, num_groups):
    """The aggregation for any shape and batch, as the reference runs it: agg_operands -> msda_forward on feat.view(B*N, S, G, C/G) ->
    camera_sum.  feat (B*N,S,C) f32|bf16 with (C/G) % 4 == 0; the other operands as agg_operands takes them (batched or one sample);
    level_hw [(H,W)]*L and level_start [L], as lists or as the (L,2) / (L,) integer tensors of the reference.  Returns (B,A,C) f32.
    Three launches and the operands through memory: the path for what aggregate_fused_supported refuses, and the independent statement
    the fused kernel is tested against -- aggregate_forward stays the path of the family."""
    _chk(feat, "feat", ndim=3)
    BN, S, C = feat.shape
    G = int(num_groups)
    if G < 1 or C % G or (C // G) % 4:
        raise ValueError("aggregate_general: C=%d must split into G=%d groups of a multiple of 4 channels" % (C, G))
    shapes, starts = _level_tensor(level_hw, feat.device), _level_tensor(level_start, feat.device)
    loc, w = agg_operands(ref, offsets, lidar2img, U, Vc, shapes.shape[0], G, pc_range, pad_hw)
    if loc.shape[0] != BN:
        raise ValueError("aggregate_general: feat holds %d maps, the operands describe %d (B*N)" % (BN, loc.shape[0]))
    per_cam = msda_forward(feat.view(BN, S, G, C // G), shapes, starts, loc, w, im2col_step=max(BN, 1))
    return camera_sum(per_cam, lidar2img.shape[-3])


# --------------------------------------------------------------------------------------------------
# implicit-GEMM convolution / linear
# --------------------------------------------------------------------------------------------------
ACT = {None: 0, "none": 0, "relu": 1, "swish": 2}
_TUNING = {}


# Tile tables conv2d_nhwc / linear consult when the caller passes tile = 0.  The two names below are the PROCESS DEFAULTS (what a
# stand-alone op or a plugin module gets); an engine selects its own tables for the duration of its entry points with
# use_tile_tables(), which is thread-local and restores the previous selection on exit -- an engine that ran earlier, or one driven
# from another thread, never changes what somebody else's launches look up (the tables used to be re-assigned module globals).
BF16_TILE_TABLE = "tuning_mi355x.json"
PAIR_TILE_TABLE = "tuning_mi355x_pair.json"   # pair-stored activations (the bf16x3 engine mode)
_PAIR_TABLE_OF = {"tuning_mi355x.json": "tuning_mi355x_pair.json", "tuning_mi355x_tput.json": "tuning_mi355x_pair_tput.json"}
_TABLE_SEL = threading.local()


def pair_table_for(bf16_table):
    """The pair-storage tile table that goes with a bf16 one: the shipped pairs by name, `<stem>_pair.json` beside a custom table when
    that file exists, else the default pair table -- never the bf16 table itself."""
    if bf16_table in _PAIR_TABLE_OF:
        return _PAIR_TABLE_OF[bf16_table]
    import os
    cand = bf16_table[:-5] + "_pair.json" if bf16_table.endswith(".json") else bf16_table + "_pair"
    if os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", cand)):
        return cand
    return "tuning_mi355x_pair.json"


def tile_tables():
    """(bf16 table, pair table) in force for this thread."""
    return getattr(_TABLE_SEL, "cur", None) or (BF16_TILE_TABLE, PAIR_TILE_TABLE)


@contextlib.contextmanager
def use_tile_tables(bf16_table, pair_table=None):
    """Select the tile tables for the launches issued (or captured into a graph) inside the block, for this thread only."""
    prev = getattr(_TABLE_SEL, "cur", None)
    _TABLE_SEL.cur = (bf16_table, pair_table or pair_table_for(bf16_table))
    try:
        yield
    finally:
        _TABLE_SEL.cur = prev


@contextlib.contextmanager
def tiles_as_for(images, of):
    """Inside the block (this thread only), a convolution on `of` images chooses its tile as the same layer on `images` images would:
    the table lookups of _conv_plan and group_tile see images / of of the pixels, and where they leave the choice to the library's
    heuristic (tile 0) and that heuristic reads the pixel count, the launch gets the heuristic's answer for `images` images as an
    explicit tile -- or is refused by name where no explicit tile reproduces it (_pin_auto_tile).  For a pass over the images of several
    scene streams at once (Far3DEngine.camera_stage_streams): a tile fixes the order in which a pixel's products are added, so every
    image keeps the bits of its own stream's pass.  Calls on any other image count (linear(): one image) are not touched."""
    images, of = int(images), int(of)
    if images < 1 or of % images:
        raise ValueError("tiles_as_for: %d images is not a whole number of blocks of %d" % (of, images))
    prev = getattr(_TABLE_SEL, "as_for", None)
    _TABLE_SEL.as_for = (images, of)
    try:
        yield
    finally:
        _TABLE_SEL.as_for = prev


def plan_images(N):
    """The image count whose tile choice a launch on N images takes (tiles_as_for; N itself outside one)."""
    sel = getattr(_TABLE_SEL, "as_for", None)
    return sel[0] if sel is not None and sel[1] == N else N


def _auto_tile(npix, Cout):
    """igemm_auto_tile (csrc/igemm_kernels.hpp): the register-staged kernel's tile for tile = 0."""
    if Cout <= 64:
        return 2 if npix >= 128 * 512 else 3
    if -(-npix // 128) * -(-Cout // 128) >= 512:
        return 1
    return 4 if -(-npix // 64) * -(-Cout // 128) >= 512 else 3


def _pin_auto_tile(x, pc, pair_in, n, Ho, Wo):
    """tile = 0 on x's N images, to be chosen as for n < N of them: what far3d_conv2d_nhwc's own choice (csrc/igemm.hip,
    igemm_pair.hip) reads the pixel count for, answered for n images.  Pair-stored 3x3 / stride 1 / pad 1 and 1x1 / stride 1 layers
    have fixed defaults (160 / 179) and stay 0.  The register-staged kernel's heuristic (igemm_auto_tile) becomes an explicit id 1-5,
    which takes the same kernel.  fp32 rows x split weights on a 1x1 layer may take tiles 479 / 480 by the pixel count, and whether
    they do depends on alignment the library checks: left at 0 where neither heuristic changes its answer, refused otherwise."""
    N = x.shape[0]
    one, all_ = n * Ho * Wo, N * Ho * Wo
    g1 = (pc.KH, pc.KW, pc.stride, pc.pad) == (1, 1, 1, 0)
    g3 = (pc.KH, pc.KW, pc.stride, pc.pad) == (3, 3, 1, 1)
    if pair_in and (g1 or g3):
        return 0
    if not pair_in and x.dtype == torch.float32 and pc.w_code == DT_F32_BF16X3 and g1:
        big = lambda px: -(-px // 128) * -(-pc.Cout // 128) >= 2048
        if big(one) != big(all_) or _auto_tile(one, pc.Cout) != _auto_tile(all_, pc.Cout):
            raise ValueError("tiles_as_for: the 1x1 layer %d -> %d on fp32 rows with split weights has no tile-table entry, and the library's "
                             "choice for %d images differs from its choice for %d; run it per %d images" % (pc.Cin, pc.Cout, N, n, n))
        return 0
    return _auto_tile(one, pc.Cout)


GROUP_MAX = 16                  # FAR3D_WS_GROUP_MAX in include/far3d_hip.h
GROUP_TILE_TABLE = "tuning_mi355x_groups.json"

# far3d_conv_tile_caps (include/far3d_hip.h, FAR3D_TILE_*): what a tile id is.  The table itself is csrc/conv_tiles.hpp.
TILE_ANY, TILE_1X1, TILE_3X3, TILE_3X3S2 = 0, 1, 2, 3                  # caps & 3: the layer geometry the tile takes
TILE_HI_ONLY, TILE_PERSISTENT, TILE_HAS_GROUP, TILE_GROUPED, TILE_SUMS, TILE_LDS_DMA = 32, 64, 128, 256, 512, 1024
_STORAGES = ((DT_BF16, DT_BF16), (DT_BF16_PAIR, DT_F32_BF16X3), (DT_F32, DT_F32_BF16X3), (DT_F32, DT_F32), (DT_F32, DT_BF16))


@functools.lru_cache(maxsize=None)
def tile_caps(tile, x_dt=None, w_dt=None):
    """The FAR3D_TILE_* mask of a tile id for activations x_dt and weights w_dt, -1 = no such tile for that storage; without a storage,
    for the first storage that has the tile (an id above 5 belongs to one).  (caps >> 2) & 7 is the storage, caps >> 16 the pixels per
    tile.  Asks the library, which is loaded at the first query (no device needed)."""
    if x_dt is None:
        return next((c for c in (tile_caps(tile, *st) for st in _STORAGES) if c >= 0), -1)
    return _lib.load().far3d_conv_tile_caps(int(tile), x_dt, w_dt)


def is_ws_tile(tile):
    """A persistent wave-specialised tile (csrc/conv_ws.hpp; bias + activation + store only), grouped ids included."""
    return tile_caps(tile) >= 0 and bool(tile_caps(tile) & TILE_PERSISTENT)


def is_group_tile(tile):
    """An id of conv2d_nhwc_grouped."""
    return tile_caps(tile) >= 0 and bool(tile_caps(tile) & TILE_GROUPED)


def tile_takes_sums(tile, pair):
    """Can the tile add the channel sums of its output (conv2d_nhwc(sums=...)) on a bf16 (pair: pair-stored) map?"""
    c = tile_caps(tile, DT_BF16_PAIR, DT_F32_BF16X3) if pair else tile_caps(tile, DT_BF16, DT_BF16)
    return c >= 0 and bool(c & TILE_SUMS)


def _table(name, groups=False):
    """far3d_amd/data/<name>, read once (a missing file is an empty table): {key without its pixel count: [(pixel count, entry)]}; the
    key is the layer's (Cout, Cin, k, stride), or the group's name (groups)."""
    tab = _TUNING.get(name)
    if tab is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", name)
        tab = _TUNING[name] = {}
        for key, tile in (json.load(open(path)) if os.path.exists(path) else {}).items():
            k, npx = key.rsplit(",", 1)
            tab.setdefault(k if groups else tuple(int(v) for v in k.split(",")), []).append(
                (int(npx), tuple(int(t) for t in tile) if isinstance(tile, (list, tuple)) else int(tile)))
    return tab


def _tuned_tile(Cout, Cin, k, stride, npix, table=None, ws_ok=False):
    """Workgroup tile measured fastest on MI355X for this conv shape (tools/tune_conv.py); 0 = kernel heuristic.
    Shapes that were not swept (e.g. fewer cameras per rank in camera-sharded mode) borrow the entry of the same layer
    geometry with the closest pixel count.  table: tuning_mi355x.json (bf16) or tuning_mi355x_bf16x3.json (split mode).
    An entry may be a pair [ws tile, other tile]: the wave-specialised kernel where the call allows it (ws_ok: no residual, second
    output or channel sums, same storage in and out), else the fastest of the general kernels -- an explicit choice per call, the
    library itself never substitutes a kernel."""
    cands = _table(table or tile_tables()[0]).get((Cout, Cin, k, stride))
    if not cands:
        return 0
    npx, tile = min(cands, key=lambda c: abs(c[0] - npix))
    if isinstance(tile, tuple):
        # a persistent tile was measured at ITS pixel count (its grid is one workgroup per CU walking npix / tile items): a borrowed entry
        # (camera-sharded ranks see 1/2 .. 1/7 of the pixels) keeps the general tile
        return tile[0] if (ws_ok and 4 * abs(npx - npix) <= npx) else tile[1]
    return tile


class PackedConv:
    """Weights of one conv / linear layer in the kernel's layout (built once at model-prepare time).

    w (rows=ceil(Cout/128)*128, taps*cin_pad) in the compute dtype (bf16 -> bf16 MFMA, fp32 -> exact fp32
    MFMA), tap-major K; bias (rows,) f32 or None.  compute="bf16x3" (fp32 weights and activations only): products as a
    two-term bf16 split on the bf16 MFMA with fp32 accumulation (FAR3D_DT_F32_BF16X3).
    """

    def __init__(self, weight, bias=None, stride=1, pad=0, dtype=torch.bfloat16, device=None, compute=None):
        if compute not in (None, "bf16x3") or (compute == "bf16x3" and dtype != torch.float32):
            raise ValueError("PackedConv: compute=%r needs dtype=float32 (got %s)" % (compute, dtype))
        if weight.dim() == 2:
            weight = weight[:, :, None, None]
        Cout, Cin, KH, KW = weight.shape
        device = device if device is not None else weight.device
        cin_pad = (Cin + 31) // 32 * 32
        rows = (Cout + 255) // 256 * 256 + 256   # zero rows so that ANY channel tile (<= 256 rows) may over-read
        w = torch.zeros(rows, KH * KW, cin_pad, dtype=torch.float32, device=weight.device)
        w[:Cout, :, :Cin] = weight.detach().float().permute(0, 2, 3, 1).reshape(Cout, KH * KW, Cin)
        if compute == "bf16x3":    # pre-split rows: per 32-channel block [32 hi | 32 lo] bf16 (include/far3d_hip.h)
            blk = w.reshape(rows, KH * KW * cin_pad // 32, 32)
            hi = blk.to(torch.bfloat16)
            lo = (blk - hi.float()).to(torch.bfloat16)
            self.w = torch.cat([hi, lo], dim=2).reshape(rows, 2 * KH * KW * cin_pad).to(device).contiguous()
        else:
            self.w = w.reshape(rows, KH * KW * cin_pad).to(dtype).to(device).contiguous()
        self.bias = None
        if bias is not None:
            b = torch.zeros(rows, dtype=torch.float32, device=weight.device)
            b[:Cout] = bias.detach().float()
            self.bias = b.to(device)
        self.Cout, self.Cin, self.KH, self.KW, self.stride, self.pad = Cout, Cin, KH, KW, stride, pad
        self.w_code = DT_F32_BF16X3 if compute == "bf16x3" else _dt(self.w)
        # pair-stored inputs only: 3 = split products (default); 1 = hi halves only, i.e. a single-bf16 layer inside a pair-stored
        # network (the per-layer precision assignment measured by tools/precision_sweep.py)
        self.terms = 3

    def out_hw(self, H, W):
        return ((H + 2 * self.pad - self.KH) // self.stride + 1, (W + 2 * self.pad - self.KW) // self.stride + 1)


def _nhwc_view(t, name):
    """(N,H,W,C) view with unit channel stride and dense rows: returns (ld, img_stride)."""
    if t.dim() != 4 or t.stride(3) != 1 or t.stride(1) != t.shape[2] * t.stride(2):
        raise ValueError("%s must be an NHWC view with unit channel stride and dense rows, got shape %s stride %s" %
                         (name, tuple(t.shape), t.stride()))
    if not t.is_cuda:
        raise _lib.Far3dHipError("%s must live on a HIP device; there is no CPU path" % name)
    return t.stride(2), t.stride(0)


SUMS_MAX_PARTS = 32     # FAR3D_SUMS_MAX_PARTS in include/far3d_hip.h


def ese_scratch_floats(N, C):
    """FAR3D_SUMS_SCRATCH_FLOATS(N, C): workspace of ese_nhwc / groupnorm_nhwc (never needs zeroing)."""
    return N * C * (2 * SUMS_MAX_PARTS + 1)


def _is_pair_input(x, pc):
    return pc.w_code == DT_F32_BF16X3 and x.dtype == torch.bfloat16


def _pair_tile(pc, Cin, npix, tile, ws_ok=False):
    """Tile id for a pair-stored input: the measured split-product tile (far3d_amd/data/tuning_mi355x_pair.json, ids 150+, 0 = the
    library default), mapped to a hi-planes-only kernel when the layer is assigned a single bf16 product (pc.terms == 1): tile + 100
    where that is the hi-only form of the tile (conv_tiles.hpp), else the default hi-only tile of the layer's kernel size."""
    fast = pc.stride == 1 and ((pc.KH == 3 and pc.pad == 1) or (pc.KH == 1 and pc.pad == 0))
    if tile == 0:
        tile = _tuned_tile(pc.Cout, Cin, pc.KH, pc.stride, npix, tile_tables()[1], ws_ok=ws_ok and pc.terms != 1)
    if pc.terms == 1 and fast and (tile == 0 or 150 <= tile < 200):
        c, hi = tile_caps(tile, DT_BF16_PAIR, DT_F32_BF16X3), tile_caps(tile + 100, DT_BF16_PAIR, DT_F32_BF16X3)
        tile = tile + 100 if c >= 0 and hi >= 0 and hi & TILE_HI_ONLY and (hi & 3) == (c & 3) else (260 if pc.KH == 3 else 279)
    return tile


def _conv_plan(x, pc, out_dtype, res=None, y2=None, sums=None, tile=0, out=None):
    """What conv2d_nhwc launches for this call: (pair_in, ws_ok, tile).  out_dtype: the dtype of the call's output; out: the output view
    when there is one (a fresh output is dense and aligned); sums: anything but None = the call asks for channel sums.
    ws_ok -- what the persistent wave-specialised kernels cover (anything else takes the table's general tile) -- exists only here."""
    N, H, W, Cx = x.shape
    pair_in = _is_pair_input(x, pc)
    Cin = Cx // 2 if pair_in else Cx
    Ho, Wo = pc.out_hw(H, W)
    dense = (out is None or (out.stride(2) % 8 == 0 and out.stride(0) % 8 == 0 and out.data_ptr() % 16 == 0)) and \
        x.stride(2) % 8 == 0 and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0
    ws_ok = (res is None and y2 is None and pc.stride == 1 and
             ((pc.KH == 3 and pc.KW == 3 and pc.pad == 1 and sums is None) or
              (pc.KH == 1 and pc.KW == 1 and pc.pad == 0 and pair_in and (sums is None or (Ho * Wo >= 256 and Cin >= 192)))) and
             Cin % 32 == 0 and pc.Cout % 32 == 0 and out_dtype == torch.bfloat16 and dense)
    Nt = plan_images(N)          # tiles_as_for: the image count whose choice this launch takes
    auto = tile == 0
    if pair_in:
        tile = _pair_tile(pc, Cin, Nt * H * W, tile, ws_ok)
    elif tile == 0 and x.dtype == torch.bfloat16:
        tile = _tuned_tile(pc.Cout, Cin, pc.KH, pc.stride, Nt * H * W, ws_ok=ws_ok)
    elif tile == 0 and pc.w_code == DT_F32_BF16X3:
        tile = _tuned_tile(pc.Cout, Cin, pc.KH, pc.stride, Nt * H * W, "tuning_mi355x_bf16x3.json")
    if auto and tile == 0 and Nt != N:
        tile = _pin_auto_tile(x, pc, pair_in, Nt, Ho, Wo)
    return pair_in, ws_ok, tile


def conv_tile(x, pc, out_dtype=None, res=None, y2=None, sums=None, out=None):
    """The tile conv2d_nhwc(x, pc, tile=0, ...) with the same optional arguments will use (0 = kernel heuristic)."""
    return _conv_plan(x, pc, out.dtype if out is not None else out_dtype or x.dtype, res, y2, sums, 0, out)[2]


def conv2d_nhwc(x, pc, out=None, act=None, out_dtype=None, res=None, y2=None, y2_scale=None, y2_shift=None, tile=0, sums=None):
    """x: (N,H,W,Cin) NHWC view (f32|bf16).  pc: PackedConv.  out: optional (N,Ho,Wo,Cout) NHWC view to write
    into (e.g. a channel slice of an OSA concat buffer).  Returns out.
    Pair storage: with split weights (compute="bf16x3") a bf16 `x` is a pair-stored map (N,H,W,2*Cin) (pair_from_float); a bf16
    `out` / `res` is then pair-stored too ((..., 2*Cout)), an f32 `out` / `y2` is plain.
    sums: optional zeroed int64 (N, Cout) device tensor -- the layer's epilogue adds the fixed-point channel sums of its stored output
    (far3d_hip.h, chan_sums; see conv_can_fuse_sums); ese_nhwc(sums=...) consumes them."""
    lib = _lib.require_device()
    N, H, W, Cx = x.shape
    pair_in = _is_pair_input(x, pc)
    Cin = Cx // 2 if pair_in else Cx
    if Cin != pc.Cin or (pair_in and Cx % 64):
        raise ValueError("conv2d_nhwc: input has %d channels, layer expects %d" % (Cin, pc.Cin))
    ldx, xs = _nhwc_view(x, "x")
    Ho, Wo = pc.out_hw(H, W)
    if out is None:
        odt = out_dtype or x.dtype
        out = torch.empty((N, Ho, Wo, pc.Cout * (2 if pair_in and odt == torch.bfloat16 else 1)), dtype=odt, device=x.device)
    pair_out = pair_in and out.dtype == torch.bfloat16
    cso = 2 if pair_out else 1
    if tuple(out.shape) != (N, Ho, Wo, pc.Cout * cso):
        raise ValueError("conv2d_nhwc: out shape %s != %s" % (tuple(out.shape), (N, Ho, Wo, pc.Cout * cso)))
    ldy, ys = _nhwc_view(out, "out")
    rp, rdt, ldr, rs, Hr, Wr = None, 0, 0, 0, Ho, Wo
    if res is not None:
        ldr, rs = _nhwc_view(res, "res")
        pair_res = pair_in and res.dtype == torch.bfloat16
        if res.shape[0] != N or res.shape[3] != pc.Cout * (2 if pair_res else 1):
            raise ValueError("conv2d_nhwc: residual shape %s incompatible" % (tuple(res.shape),))
        rp, rdt, Hr, Wr = _ptr(res), DT_BF16_PAIR if pair_res else _dt(res), res.shape[1], res.shape[2]
    y2p, y2dt, ldy2, y2s, sp, hp = None, 0, 0, 0, None, None
    if y2 is not None:
        ldy2, y2s = _nhwc_view(y2, "y2")
        _chk(y2_scale, "y2_scale", torch.float32)
        _chk(y2_shift, "y2_shift", torch.float32)
        if y2_scale.numel() != N * pc.Cout or y2_shift.numel() != N * pc.Cout or tuple(y2.shape) != (N, Ho, Wo, pc.Cout):
            raise ValueError("conv2d_nhwc: y2/scale/shift shapes inconsistent")
        y2p, y2dt, sp, hp = _ptr(y2), _dt(y2), _ptr(y2_scale), _ptr(y2_shift)
    tile = _conv_plan(x, pc, out.dtype, res, y2, sums, tile, out)[2]
    _lib.check(lib.far3d_conv2d_nhwc(
        _ptr(x), DT_BF16_PAIR if pair_in else _dt(x), _ptr(pc.w), pc.w_code, _ptr(pc.bias) if pc.bias is not None else None, _ptr(out),
        DT_BF16_PAIR if pair_out else _dt(out),
        N, H, W, Cin, ldx, xs, Ho, Wo, pc.Cout, ldy, ys, pc.KH, pc.KW, pc.stride, pc.pad, ACT[act],
        rp, rdt, ldr, rs, Hr, Wr, y2p, y2dt, ldy2, y2s, sp, hp, _sums_ptr(sums, N, pc.Cout), tile,
        _stream(x)), "far3d_conv2d_nhwc")
    return out


class _ConvProblem(ctypes.Structure):
    """far3d_conv_problem (include/far3d_hip.h)."""
    _fields_ = [("x", ctypes.c_void_p), ("w", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("y", ctypes.c_void_p),
                ("y2", ctypes.c_void_p), ("y2_scale", ctypes.c_void_p), ("y2_shift", ctypes.c_void_p),
                ("x_img_stride", ctypes.c_long), ("y_img_stride", ctypes.c_long), ("y2_img_stride", ctypes.c_long),
                ("N", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("Cin", ctypes.c_int), ("Cout", ctypes.c_int),
                ("ldx", ctypes.c_int), ("ldy", ctypes.c_int), ("ldy2", ctypes.c_int), ("act", ctypes.c_int)]


def conv_groupable(x, pc):
    """True if (x, pc) can be one problem of conv2d_nhwc_grouped: a 3x3 / stride 1 / pad 1 layer with split products (pc.terms 3) on a
    pair-stored map whose channels are a multiple of 32, 16-byte aligned rows."""
    if not (_is_pair_input(x, pc) and pc.terms == 3 and pc.KH == 3 and pc.KW == 3 and pc.stride == 1 and pc.pad == 1):
        return False
    if pc.Cin % 32 or pc.Cout % 32 or x.shape[-1] != 2 * pc.Cin or x.dim() != 4 or x.stride(3) != 1:
        return False
    return x.data_ptr() % 16 == 0 and x.stride(2) % 8 == 0 and x.stride(0) % 8 == 0


def group_tile(name, npix, table=None):
    """The grouped tile measured for the named layer group (far3d_amd/data/tuning_mi355x_groups.json, key "<group>,<level-0 pixels>";
    tools/tune_conv.py GROUPS=1), or 0 = the group is launched layer by layer.  Like a persistent single-layer tile, an entry holds only
    near the pixel count it was measured at: the group replaces the per-layer launches only where it was measured to win."""
    cands = _table(table or GROUP_TILE_TABLE, groups=True).get(name)
    if not cands:
        return 0
    sel = getattr(_TABLE_SEL, "as_for", None)
    if sel is not None:          # tiles_as_for: npix counts the pixels of sel[1] images; the group is chosen as for sel[0] of them
        npix = npix * sel[0] // sel[1]
    npx, tile = min(cands, key=lambda c: abs(c[0] - npix))
    return tile if 4 * abs(npx - npix) <= npx else 0


def conv2d_nhwc_grouped(problems, tile):
    """Up to GROUP_MAX independent 3x3 convolutions of one Cin as ONE launch of the persistent kernel (far3d_conv2d_nhwc_grouped).
    problems: list of dicts with x (pair-stored NHWC view), pc (PackedConv, split products), optional out (pair-stored view), act, and
    optional y2 / y2_scale / y2_shift (the fp32 second output of conv2d_nhwc).  Every output is bit-identical to conv2d_nhwc of the same
    problem.  Returns the list of outputs.  Anything the launch does not cover is an error, never a per-layer fallback."""
    lib = _lib.require_device()
    if not 1 <= len(problems) <= GROUP_MAX:
        raise ValueError("conv2d_nhwc_grouped: %d problems (1..%d)" % (len(problems), GROUP_MAX))
    if not is_group_tile(tile):
        raise ValueError("conv2d_nhwc_grouped: tile %r is not a grouped tile" % (tile,))
    arr = (_ConvProblem * len(problems))()
    outs = []
    for i, pr in enumerate(problems):
        x, pc = pr["x"], pr["pc"]
        if not conv_groupable(x, pc):
            raise ValueError("conv2d_nhwc_grouped: problem %d is not a 3x3 / s1 / p1 split-product layer on an aligned pair-stored map" % i)
        N, H, W, _ = x.shape
        ldx, xs = _nhwc_view(x, "x")
        out = pr.get("out")
        if out is None:
            out = torch.empty((N, H, W, 2 * pc.Cout), dtype=torch.bfloat16, device=x.device)
        if out.dtype != torch.bfloat16 or tuple(out.shape) != (N, H, W, 2 * pc.Cout):
            raise ValueError("conv2d_nhwc_grouped: problem %d: out must be a pair-stored %s map" % (i, (N, H, W, 2 * pc.Cout)))
        ldy, ys = _nhwc_view(out, "out")
        c = arr[i]
        c.x, c.w, c.y = x.data_ptr(), pc.w.data_ptr(), out.data_ptr()
        c.bias = pc.bias.data_ptr() if pc.bias is not None else None
        c.x_img_stride, c.y_img_stride = xs, ys
        c.N, c.H, c.W, c.Cin, c.Cout, c.ldx, c.ldy, c.act = N, H, W, pc.Cin, pc.Cout, ldx, ldy, ACT[pr.get("act")]
        y2 = pr.get("y2")
        if y2 is not None:
            sc, sh = pr["y2_scale"], pr["y2_shift"]
            if y2.dtype != torch.float32:
                raise TypeError("conv2d_nhwc_grouped: problem %d: y2 must be float32 (got %s)" % (i, y2.dtype))
            _chk(sc, "y2_scale", torch.float32)
            _chk(sh, "y2_shift", torch.float32)
            if sc.numel() != N * pc.Cout or sh.numel() != N * pc.Cout or tuple(y2.shape) != (N, H, W, pc.Cout):
                raise ValueError("conv2d_nhwc_grouped: problem %d: y2/scale/shift shapes inconsistent" % i)
            c.ldy2, c.y2_img_stride = _nhwc_view(y2, "y2")
            c.y2, c.y2_scale, c.y2_shift = y2.data_ptr(), sc.data_ptr(), sh.data_ptr()
        outs.append(out)
    _lib.check(lib.far3d_conv2d_nhwc_grouped(ctypes.cast(arr, ctypes.c_void_p), len(problems), tile, _stream(problems[0]["x"])),
               "far3d_conv2d_nhwc_grouped")
    return outs


# linear(): tile for fp32 rows x fp32 weights (exact fp32 MFMA on the pipelined GEMM kernel, far3d_hip.h tiles 482-494); 0 = the
# register-staged kernel of rounds 1-5.  482 = 64 x 64, 2 stages: the fastest of 482-486 on every decoder shape; 487-494 split K between
# wave groups INSIDE the workgroup (a 32 x 32 tile over K = 1 024 is a 16 us serial MFMA chain however idle the chip is): 493 (32 x 64, 2
# groups) wins the K <= 512 shapes of up to 768 columns, 489 (32 x 64, 4 groups) the K = 1 024 one, 482 stays for >= 1 024 columns where
# the tiles already fill the chip (tools/probe/f32x_gemm_ab.py, profiles/r6/f32x_gemm_ab.txt).
F32X_LINEAR_TILE = 482


def f32x_linear_tile(cout, K):
    """The exact-fp32 tile of linear() for a (cout, K) weight.  A function of the WEIGHT's shape only, never of the number of rows: the
    tile fixes the order in which a row's products are added, and the query-sharded decoder (row subsets) reproduces the replicated one
    bit for bit."""
    if not F32X_LINEAR_TILE:
        return 0
    if K >= 1024:
        return 489
    return F32X_LINEAR_TILE if cout >= 1024 else 493
SUMS_FRAC_BITS = 18      # FAR3D_SUMS_FRAC_BITS in include/far3d_hip.h
_GEMM_TILE_PIXELS = 512  # no GEMM tile holds more pixels


def _sums_ptr(sums, N, C):
    if sums is None:
        return None
    if sums.dtype != torch.int64 or sums.numel() < N * C or not sums.is_contiguous():
        raise ValueError("channel sums: contiguous int64 tensor of at least N*C = %d elements" % (N * C))
    return _ptr(sums)


def conv_can_fuse_sums(x, pc, out_dtype=torch.bfloat16):
    """True if conv2d_nhwc(x, pc, sums=...) is possible: a 1x1 / stride-1 layer whose measured tile is one of the pipelined GEMM
    kernels, bf16 or pair output, and a map of at least one pixel tile (otherwise the eSE op pools the map itself)."""
    N, H, W, Cx = x.shape
    if pc.KH != 1 or pc.KW != 1 or pc.stride != 1 or pc.pad != 0 or out_dtype != torch.bfloat16 or x.dtype != torch.bfloat16:
        return False
    if H * W < _GEMM_TILE_PIXELS or pc.Cout % 8:
        return False
    pair_in = _is_pair_input(x, pc)
    if (Cx // 2 if pair_in else Cx) % 32:
        return False
    tile = _conv_plan(x, pc, out_dtype, sums=True)[2]
    return tile_takes_sums(tile, pair_in) or (pair_in and tile == 0)


def linear(x, pc, act=None, res=None, out=None, out_dtype=torch.float32, tile=0):
    """y = act(x @ W^T + b) (+ res).  x (M,K) with unit inner stride (row stride free); returns (M,Cout)."""
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("linear: x must be (M,K) with unit inner stride")
    M = x.shape[0]
    xv = x.as_strided((1, 1, M, x.shape[1]), (M * x.stride(0), M * x.stride(0), x.stride(0), 1))
    if out is None:
        out = torch.empty((M, pc.Cout), dtype=out_dtype, device=x.device)
    ov = out.as_strided((1, 1, M, pc.Cout), (M * out.stride(0), M * out.stride(0), out.stride(0), 1))
    rv = None
    if res is not None:
        rv = res.as_strided((1, 1, M, pc.Cout), (M * res.stride(0), M * res.stride(0), res.stride(0), 1))
    conv2d_nhwc(xv, pc, out=ov, act=act, res=rv, tile=tile or _linear_own_tile(x, pc))
    return out


def _linear_own_tile(x, pc):
    """The tile linear() chooses itself for x (M,K), before the tile table is asked (0: it leaves the choice to conv2d_nhwc)."""
    M, K = x.shape
    if x.dtype == torch.bfloat16 and pc.w.dtype == torch.bfloat16 and K % 32 == 0 and _tuned_tile(pc.Cout, K, 1, 1, M) == 0:
        return 80     # untuned small GEMM: 64x64 pipelined tile (the winner on every decoder-sized shape of the table)
    if F32X_LINEAR_TILE and x.dtype == torch.float32 and pc.w.dtype == torch.float32 and pc.w_code == DT_F32 and \
            K % 32 == 0 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and M * x.stride(0) * 4 < 2 ** 31 - 1:
        # exact fp32 on the LDS-DMA pipelined kernel (round 6): the GEMMs of the fp32 / in-tolerance engines' decoder and FarHead.  The
        # choice must NOT depend on the number of rows: the query-sharded decoder launches row subsets and has to reproduce the replicated
        # decoder bit for bit (a row's bits depend on the kernel, not on which rows share its launch)
        return f32x_linear_tile(pc.Cout, K)
    return 0


def linear_tile(x, pc, out_dtype=torch.float32, res=None, out=None):
    """The tile linear(x, pc, ...) with the same optional arguments runs on (0 = kernel heuristic): linear's own choice, then the tile
    table's.  For callers that must give other rows the bits of THIS launch (linear_streams)."""
    M = x.shape[0]
    tile = _linear_own_tile(x, pc)
    v4 = lambda t: None if t is None else t.as_strided((1, 1, M, t.shape[1]), (M * t.stride(0), M * t.stride(0), t.stride(0), 1))
    return _conv_plan(v4(x), pc, out.dtype if out is not None else out_dtype, v4(res), None, None, tile, v4(out))[2]


def linear_streams(x, pc, act=None, res=None, out=None, out_dtype=torch.float32):
    """linear() for B row blocks in ONE launch (the image-stride form of far3d_conv2d_nhwc, one image per block): x (B,M,K), res / out
    (B,M,Cout), each with unit inner stride and any row and block stride, so the blocks may be views of larger per-stream buffers.
    The tile is linear's choice for ONE block's M rows (linear_tile), never for B*M: a tile table keyed on the row count cannot pick
    another K order, and out[b] has the bits of linear(x[b], ...)."""
    if x.dim() != 3 or x.stride(2) != 1:
        raise ValueError("linear_streams: x must be (B,M,K) with unit inner stride")
    B, M, K = x.shape
    if out is None:
        out = torch.empty((B, M, pc.Cout), dtype=out_dtype, device=x.device)
    for t, n in ((out, "out"), (res, "res")):
        if t is not None and (t.dim() != 3 or tuple(t.shape) != (B, M, pc.Cout) or t.stride(2) != 1):
            raise ValueError("linear_streams: %s must be (%d,%d,%d) with unit inner stride" % (n, B, M, pc.Cout))
    if ((B - 1) * x.stride(0) + M * x.stride(1)) * x.element_size() >= 2 ** 31 - 1:     # linear()'s own limit, for the whole launch
        raise ValueError("linear_streams: the %d blocks of x span 2 GiB or more; split the launch" % B)
    tile = linear_tile(x[0], pc, res=None if res is None else res[0], out=out[0])
    if tile == 0:
        raise ValueError("linear_streams: linear() leaves this shape (K=%d, Cout=%d, %s) to the kernel's heuristic, which may depend on "
                         "the row count" % (K, pc.Cout, x.dtype))
    v4 = lambda t: t.as_strided((B, 1, M, t.shape[2]), (t.stride(0), M * t.stride(1), t.stride(1), 1), t.storage_offset())
    conv2d_nhwc(v4(x), pc, out=v4(out), act=act, res=None if res is None else v4(res), tile=tile)
    return out


# --------------------------------------------------------------------------------------------------
# row-resident decoder chains (csrc/rowchain.hip)
# --------------------------------------------------------------------------------------------------
ROWCHAIN_E, ROWCHAIN_FF, ROWCHAIN_WL_TILES = 256, 1024, 29


def pack_rowchain(pc, cols=None):
    """A PackedConv's (rows, K) bf16 weight in the MFMA fragment order the row chains stream (include/far3d_hip.h):
    [ceil(cols / 16)][K / 32][64][8], element j of lane l of (tile t, step s) = W[16 t + (l & 15)][32 s + 8 (l >> 4) + j].
    Returns (packed weight, f32 bias covering the padded columns)."""
    w = pc.w
    if w.dtype != torch.bfloat16 or pc.KH * pc.KW != 1 or pc.w_code != DT_BF16:
        raise ValueError("pack_rowchain: plain bf16 linear weights only")
    K = w.shape[1]
    if K % 256 != 0:
        raise ValueError("pack_rowchain: K=%d must be a multiple of 256" % K)
    cols = pc.Cout if cols is None else cols
    nt = -(-cols // 16)
    if nt * 16 > w.shape[0]:
        raise ValueError("pack_rowchain: %d columns exceed the packed weight's %d rows" % (nt * 16, w.shape[0]))
    frag = w[:nt * 16].reshape(nt, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()      # [t][s][l >> 4][l & 15][j]
    bias = pc.bias[:nt * 16].contiguous() if pc.bias is not None else torch.zeros(nt * 16, dtype=torch.float32, device=w.device)
    return frag.reshape(nt, K // 32, 64, 8), bias


class RowChainLayer:
    """The packed operands of one decoder layer's two row chains.  ly: the engine's layer dict (PackedConvs out / wl / oproj /
    ffn1 / ffn2 / qkv and the three (gamma, beta) pairs)."""

    def __init__(self, ly):
        self.out, self.b_out = pack_rowchain(ly["out"])
        self.wl, self.b_wl = pack_rowchain(ly["wl"])
        self.n_wl = ly["wl"].Cout
        self.oproj, self.b_oproj = pack_rowchain(ly["oproj"])
        self.ffn1, self.b_ffn1 = pack_rowchain(ly["ffn1"])
        self.ffn2, self.b_ffn2 = pack_rowchain(ly["ffn2"])
        self.qkv, self.b_qkv = pack_rowchain(ly["qkv"])
        self.norms = [(g.contiguous(), b.contiguous()) for g, b in ly["norms"]]

    @staticmethod
    def supported(ly, E, dtype):
        """The chains are built for the benchmark's decoder geometry (E = 256, FFN 1024, 449..464 aggregation outputs, bf16)."""
        return (dtype == torch.bfloat16 and E == ROWCHAIN_E and ly["ffn1"].Cout == ROWCHAIN_FF and ly["ffn2"].Cin == ROWCHAIN_FF and
                16 * (ROWCHAIN_WL_TILES - 1) < ly["wl"].Cout <= 16 * ROWCHAIN_WL_TILES and ly["wl"].Cin == 2 * E and
                ly["qkv"].Cin == 2 * E and ly["qkv"].Cout == 3 * E and all(ly[k].w.dtype == torch.bfloat16 and ly[k].w_code == DT_BF16
                                                                           for k in ("out", "wl", "oproj", "ffn1", "ffn2", "qkv")))


class RowChainBranches:
    """Packed operands of far3d_rowchain_branches.  cls / reg: the three PackedConvs of each branch; cls_ln: two (gamma, beta)."""

    def __init__(self, cls, cls_ln, reg):
        (self.c0, self.b_c0), (self.c1, self.b_c1) = (pack_rowchain(pc) for pc in cls[:2])
        (self.r0, self.b_r0), (self.r1, self.b_r1) = (pack_rowchain(pc) for pc in reg[:2])
        (self.c2, self.b_c2), (self.r2, self.b_r2) = pack_rowchain(cls[2], cols=32), pack_rowchain(reg[2], cols=32)   # two tiles each
        self.cls_ln = [(g.contiguous(), b.contiguous()) for g, b in cls_ln]
        self.n_cls, self.n_reg = cls[2].Cout, reg[2].Cout

    @staticmethod
    def supported(cls, reg, E, dtype):
        pcs = list(cls) + list(reg)
        return (dtype == torch.bfloat16 and E == ROWCHAIN_E and all(pc.w.dtype == torch.bfloat16 and pc.w_code == DT_BF16 and pc.Cin == E for pc in pcs) and
                all(pc.Cout == E for pc in (cls[0], cls[1], reg[0], reg[1])) and 1 <= cls[2].Cout <= 32 and 1 <= reg[2].Cout <= 32)


def _rows(t, name, dtype, cols):
    if t.dim() != 2 or t.stride(1) != 1 or t.dtype != dtype or t.shape[1] < cols or not t.is_cuda:
        raise ValueError("%s must be a (M, >=%d) %s device tensor with unit inner stride" % (name, cols, dtype))
    return t


def rowchain_attn_out(att, x, qpos, rc, x1, ul, eps=1e-5, ul_rows=None):
    """x1 = LN0(att @ W_out^T + b + x); ul[:, :n_wl] = [x1 + qpos | x1] @ W_wl^T + b  -- one launch (far3d_rowchain_attn_out).
    att (M,E) bf16; x, qpos (M,E) f32; x1 (M,E) f32 out; ul (M, >= n_wl) f32 out.  rc: RowChainLayer.
    ul_rows (M) int32: row i of ul is stored at row ul_rows[i] (aggregation_order's inv: the aggregation kernel's launch order)."""
    lib = _lib.require_device()
    E = ROWCHAIN_E
    M = att.shape[0]
    _rows(att, "att", torch.bfloat16, E); _rows(x, "x", torch.float32, E); _rows(qpos, "qpos", torch.float32, E)
    _rows(x1, "x1", torch.float32, E); _rows(ul, "ul", torch.float32, rc.n_wl)
    for t in (x, qpos, x1, ul):
        if t.shape[0] != M:
            raise ValueError("rowchain_attn_out: row counts differ")
    g0, be0 = rc.norms[0]
    if ul_rows is not None:
        _chk(ul_rows, "ul_rows", torch.int32, 1)
        if ul_rows.numel() != M:
            raise ValueError("rowchain_attn_out: ul_rows needs one entry per row")
    _lib.check(lib.far3d_rowchain_attn_out(_ptr(att), att.stride(0), _ptr(x), x.stride(0), _ptr(qpos), qpos.stride(0),
                                           _ptr(rc.out), _ptr(rc.b_out), _ptr(g0), _ptr(be0), _ptr(rc.wl), _ptr(rc.b_wl), rc.n_wl,
                                           _ptr(x1), x1.stride(0), _ptr(ul), ul.stride(0), _ptr(ul_rows) if ul_rows is not None else None,
                                           M, float(eps), _stream(att)),
               "far3d_rowchain_attn_out")
    return x1, ul


def rowchain_ffn(agg, x1, qpos, rc, out, nxt=None, qkv=None, xop=None, eps=1e-5):
    """x2 = LN1(agg @ W_o^T + b + x1); out = LN2(relu(x2 @ W_1^T + b) @ W_2^T + b + x2); with nxt (the NEXT layer's
    RowChainLayer): qkv = [out + qpos | out] @ W_qkv^T + b (bf16, (M, 3E)) -- one launch (far3d_rowchain_ffn).
    xop: optional (M, 2E) bf16 out, [out + qpos | out]."""
    lib = _lib.require_device()
    E = ROWCHAIN_E
    M = agg.shape[0]
    _rows(agg, "agg", torch.bfloat16, E); _rows(x1, "x1", torch.float32, E); _rows(qpos, "qpos", torch.float32, E)
    _rows(out, "out", torch.float32, E)
    if (nxt is None) != (qkv is None):
        raise ValueError("rowchain_ffn: nxt and qkv go together")
    if qkv is not None:
        _rows(qkv, "qkv", torch.bfloat16, 3 * E)
    if xop is not None:
        _rows(xop, "xop", torch.bfloat16, 2 * E)
    for t in (x1, qpos, out, qkv, xop):
        if t is not None and t.shape[0] != M:
            raise ValueError("rowchain_ffn: row counts differ")
    (g1, be1), (g2, be2) = rc.norms[1], rc.norms[2]
    _lib.check(lib.far3d_rowchain_ffn(_ptr(agg), agg.stride(0), _ptr(x1), x1.stride(0), _ptr(qpos), qpos.stride(0),
                                      _ptr(rc.oproj), _ptr(rc.b_oproj), _ptr(g1), _ptr(be1), _ptr(rc.ffn1), _ptr(rc.b_ffn1),
                                      _ptr(rc.ffn2), _ptr(rc.b_ffn2), _ptr(g2), _ptr(be2),
                                      _ptr(nxt.qkv) if nxt is not None else None, _ptr(nxt.b_qkv) if nxt is not None else None,
                                      _ptr(out), out.stride(0), _ptr(qkv) if qkv is not None else None,
                                      qkv.stride(0) if qkv is not None else 0, _ptr(xop) if xop is not None else None,
                                      xop.stride(0) if xop is not None else 0, M, float(eps), _stream(agg)), "far3d_rowchain_ffn")
    return out


def rowchain_qkv(x, qpos, rc, qkv):
    """qkv (M,3E) bf16 = [x + qpos | x] @ W_qkv^T + b of layer `rc` (RowChainLayer) -- bit-identical to what rowchain_ffn(..., nxt=rc)
    writes for the same rows (far3d_rowchain_qkv)."""
    lib = _lib.require_device()
    E = ROWCHAIN_E
    M = x.shape[0]
    _rows(x, "x", torch.float32, E); _rows(qpos, "qpos", torch.float32, E); _rows(qkv, "qkv", torch.bfloat16, 3 * E)
    if qpos.shape[0] != M or qkv.shape[0] != M:
        raise ValueError("rowchain_qkv: row counts differ")
    _lib.check(lib.far3d_rowchain_qkv(_ptr(x), x.stride(0), _ptr(qpos), qpos.stride(0), _ptr(rc.qkv), _ptr(rc.b_qkv), _ptr(qkv), qkv.stride(0),
                                      M, _stream(x)), "far3d_rowchain_qkv")
    return qkv


def rowchain_branches(h, rb, cls_out, reg_out, eps=1e-5):
    """cls_out (M, n_cls), reg_out (M, n_reg) f32 = the classification / regression branches of h (M,E) bf16 in one launch
    (far3d_rowchain_branches).  rb: RowChainBranches."""
    lib = _lib.require_device()
    M = h.shape[0]
    _rows(h, "h", torch.bfloat16, ROWCHAIN_E); _rows(cls_out, "cls_out", torch.float32, rb.n_cls); _rows(reg_out, "reg_out", torch.float32, rb.n_reg)
    if cls_out.shape[0] != M or reg_out.shape[0] != M:
        raise ValueError("rowchain_branches: row counts differ")
    (g0, be0), (g1, be1) = rb.cls_ln
    _lib.check(lib.far3d_rowchain_branches(_ptr(h), h.stride(0), _ptr(rb.c0), _ptr(rb.b_c0), _ptr(g0), _ptr(be0), _ptr(rb.c1), _ptr(rb.b_c1),
                                           _ptr(g1), _ptr(be1), _ptr(rb.c2), _ptr(rb.b_c2), rb.n_cls, _ptr(rb.r0), _ptr(rb.b_r0),
                                           _ptr(rb.r1), _ptr(rb.b_r1), _ptr(rb.r2), _ptr(rb.b_r2), rb.n_reg, _ptr(cls_out), cls_out.stride(0),
                                           _ptr(reg_out), reg_out.stride(0), M, float(eps), _stream(h)), "far3d_rowchain_branches")
    return cls_out, reg_out


# --------------------------------------------------------------------------------------------------
# attention / normalisation / pooling
# --------------------------------------------------------------------------------------------------
def attention_f32_variant(variant=-1):
    """A/B switch of the fp32 attention instantiation (include/far3d_hip.h); returns the previous value, -1 only reads."""
    return _lib.load().far3d_attention_f32_variant(int(variant))


def attention_forward(q, k, v, num_heads=8, out=None, out_dtype=torch.float32, hole=None):
    """softmax(q k^T / sqrt(d)) v per head.  q (Aq,E), k/v (Nk,E) f32|bf16 with unit inner stride; out (Aq,E) f32.
    hole: keys [start + count, end) are masked (see _hole)."""
    lib = _lib.require_device()
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if t.dim() != 2 or t.stride(1) != 1 or not t.is_cuda:
            raise ValueError("attention_forward: %s must be a 2-D device tensor with unit inner stride" % n)
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError("attention_forward: q/k/v dtypes differ")
    Aq, E = q.shape
    Nk = k.shape[0]
    hd = E // num_heads
    if out is None:
        out = torch.empty((Aq, E), dtype=out_dtype, device=q.device)
    _lib.check(lib.far3d_attention_forward(_ptr(q), _ptr(k), _ptr(v), _dt(q), _ptr(out), _dt(out), Aq, Nk, num_heads, hd,
                                           q.stride(0), k.stride(0), v.stride(0), out.stride(0),
                                           float(hd) ** -0.5, *_hole(hole), _stream(q)), "far3d_attention_forward")
    return out


def _batched_qkv(fn, q, k, v, num_heads):
    """Operand checks of the batched attention entries `fn`: q (B,Aq,E), k/v (B,Nk,E) device tensors of one dtype with unit inner stride,
    E a multiple of num_heads.  Returns (B, Aq, Nk, E, head_dim)."""
    for t, n in ((q, "q"), (k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.stride(2) != 1 or not t.is_cuda:
            raise ValueError("%s: %s must be a 3-D device tensor (B, rows, E) with unit inner stride" % (fn, n))
    if not (q.dtype == k.dtype == v.dtype):
        raise TypeError("%s: q/k/v dtypes differ" % fn)
    B, Aq, E = q.shape
    Nk = k.shape[1]
    if k.shape != (B, Nk, E) or v.shape != (B, Nk, E):
        raise ValueError("%s: k/v must be (%d, Nk, %d), got %s / %s" % (fn, B, E, tuple(k.shape), tuple(v.shape)))
    if E % num_heads:
        raise ValueError("%s: embed dim %d is not a multiple of num_heads %d" % (fn, E, num_heads))
    return B, Aq, Nk, E, E // num_heads


def _batched_out(fn, out, q, out_dtype):
    """`out` of the batched attention entries `fn`: q's shape, unit inner stride, on the device; allocated in out_dtype when None.  Its
    own step because attention_batched validates its masks first, and the order decides which error a call with two faults raises."""
    B, Aq, E = q.shape
    if out is None:
        out = torch.empty((B, Aq, E), dtype=out_dtype, device=q.device)
    elif tuple(out.shape) != (B, Aq, E) or out.stride(2) != 1 or not out.is_cuda:
        raise ValueError("%s: out must be a (%d, %d, %d) device tensor with unit inner stride" % (fn, B, Aq, E))
    return out


def attention_streams(q, k, v, num_heads=8, out=None, out_dtype=torch.float32, hole=None):
    """attention_forward for B samples in ONE launch (far3d_attention_streams): out[b] has the bits of attention_forward on sample b.
    q (B,Aq,E), k/v (B,Nk,E) f32|bf16 with unit inner stride (views of one (B,rows,layers*3*E) buffer are read in place); out (B,Aq,E).
    hole: None or (counts int32 device tensor (B,), start, end): sample b masks the keys [start + counts[b], end).
    attention_f32_variant does not apply: a batch always takes the default fp32 kernel."""
    lib = _lib.require_device()
    B, Aq, Nk, E, hd = _batched_qkv("attention_streams", q, k, v, num_heads)
    out = _batched_out("attention_streams", out, q, out_dtype)
    if hole is not None and hole[0].numel() != B:
        raise ValueError("attention_streams: the hole needs one count per sample (%d), got %d" % (B, hole[0].numel()))
    _lib.check(lib.far3d_attention_streams(_ptr(q), _ptr(k), _ptr(v), _dt(q), _ptr(out), _dt(out), B, Aq, Nk, num_heads, hd,
                                           q.stride(1), k.stride(1), v.stride(1), out.stride(1),
                                           q.stride(0), k.stride(0), v.stride(0), out.stride(0), float(hd) ** -0.5,
                                           *_hole(hole), _stream(q)), "far3d_attention_streams")
    return out


def attention_batched(q, k, v, num_heads=8, attn_mask=None, key_padding_mask=None, out=None, out_dtype=torch.float32):
    """Per sample and head softmax(q k^T / sqrt(d) + attn_mask + key padding) v in one launch (far3d_attention_batched).
    q (B,Aq,E), k/v (B,Nk,E) f32|bf16 with unit inner stride (views of one (B,rows,3E) buffer are read in place); out (B,Aq,E).
    attn_mask (Aq,Nk) or (B*num_heads,Aq,Nk): torch.bool / uint8 -> nonzero EXCLUDES the key; a float mask is added to the scores (may
    hold -inf; a dtype other than float32 is cast on the host).  key_padding_mask (B,Nk) bool / uint8: nonzero excludes the key.
    A query without any key left gets NaN in its whole row, as torch does."""
    lib = _lib.require_device()
    B, Aq, Nk, E, hd = _batched_qkv("attention_batched", q, k, v, num_heads)
    kind, mptr, ldm, mbs = 0, None, 0, 0
    if attn_mask is not None:
        if not isinstance(attn_mask, torch.Tensor) or not attn_mask.is_cuda:
            raise ValueError("attention_batched: attn_mask must be a device tensor")
        if attn_mask.dim() == 2:
            want = (Aq, Nk)
        elif attn_mask.dim() == 3:
            want = (B * num_heads, Aq, Nk)
        else:
            want = None
        if want is None or tuple(attn_mask.shape) != want:
            raise ValueError("attention_batched: attn_mask must be (%d, %d) or (%d, %d, %d), got %s" %
                             (Aq, Nk, B * num_heads, Aq, Nk, tuple(attn_mask.shape)))
        if attn_mask.dtype in (torch.bool, torch.uint8):
            kind = 1
            attn_mask = attn_mask.view(torch.uint8) if attn_mask.dtype == torch.bool else attn_mask
        elif attn_mask.is_floating_point():
            kind = 2
            attn_mask = attn_mask.float()
        else:
            raise TypeError("attention_batched: attn_mask dtype %s (bool, uint8 or a float type)" % attn_mask.dtype)
        if attn_mask.stride(-1) != 1 or (attn_mask.dim() == 3 and attn_mask.stride(0) < 0):
            attn_mask = attn_mask.contiguous()
        mptr, ldm = _ptr(attn_mask), attn_mask.stride(-2)
        mbs = attn_mask.stride(0) if attn_mask.dim() == 3 else 0
    pptr = None
    if key_padding_mask is not None:
        if not isinstance(key_padding_mask, torch.Tensor) or not key_padding_mask.is_cuda:
            raise ValueError("attention_batched: key_padding_mask must be a device tensor")
        if tuple(key_padding_mask.shape) != (B, Nk):
            raise ValueError("attention_batched: key_padding_mask must be (%d, %d), got %s" % (B, Nk, tuple(key_padding_mask.shape)))
        if key_padding_mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError("attention_batched: key_padding_mask dtype %s (bool or uint8)" % key_padding_mask.dtype)
        key_padding_mask = key_padding_mask.contiguous()
        key_padding_mask = key_padding_mask.view(torch.uint8) if key_padding_mask.dtype == torch.bool else key_padding_mask
        pptr = _ptr(key_padding_mask)
    out = _batched_out("attention_batched", out, q, out_dtype)
    _lib.check(lib.far3d_attention_batched(_ptr(q), _ptr(k), _ptr(v), _dt(q), _ptr(out), _dt(out), B, Aq, Nk, num_heads, hd,
                                           q.stride(1), k.stride(1), v.stride(1), out.stride(1),
                                           q.stride(0), k.stride(0), v.stride(0), out.stride(0), float(hd) ** -0.5,
                                           mptr, kind, ldm, mbs, pptr, _stream(q)), "far3d_attention_batched")
    return out


def layernorm(x, gamma, beta, eps=1e-5, act=None, add=None, out=None, add_dtype=torch.float32, bf16_copy=False, y2=None, yb=None,
              out_rows=None):
    """Returns LN(x); with `add`: (LN(x), LN(x)+add [add_dtype]); with bf16_copy also a bf16 copy of LN(x) (last).
    out_rows (rows) int32: row i of y2 / yb is stored at row out_rows[i] (far3d_layernorm_rows; LN(x) itself stays in place).
    y2 / yb: optional preallocated (rows,C) outputs (f32|bf16, unit inner stride, any row stride) for LN(x)+add and the
    copy of LN(x) -- e.g. the two halves of one (rows,2C) [x+pos | x] merged-GEMM operand; they are returned in place of
    freshly allocated ones."""
    lib = _lib.require_device()
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32:
        raise ValueError("layernorm: x must be (rows,C) f32 with unit inner stride")
    rows, C = x.shape
    y = out if out is not None else torch.empty((rows, C), dtype=torch.float32, device=x.device)
    if y2 is None and add is not None:
        y2 = torch.empty((rows, C), dtype=add_dtype, device=x.device)
    if yb is None and bf16_copy:
        yb = torch.empty((rows, C), dtype=torch.bfloat16, device=x.device)
    if y2 is not None and add is None:
        raise ValueError("layernorm: y2 needs add")
    for t in (y, y2, yb):
        if t is not None and (t.stride(1) != 1 or tuple(t.shape) != (rows, C)):
            raise ValueError("layernorm: outputs must be (rows,C) with unit inner stride")
    args = (_ptr(x), _ptr(gamma) if gamma is not None else None,
            _ptr(beta) if beta is not None else None, _ptr(y), rows, C, x.stride(0), y.stride(0),
            float(eps), 1 if act == "relu" else 0,
            _ptr(add) if add is not None else None, add.stride(0) if add is not None else 0,
            _ptr(y2) if y2 is not None else None, y2.stride(0) if y2 is not None else 0,
            _dt(y2) if y2 is not None else 0, _ptr(yb) if yb is not None else None,
            yb.stride(0) if yb is not None else 0, _dt(yb) if yb is not None else 0)
    if out_rows is not None:
        _chk(out_rows, "out_rows", torch.int32, 1)
        if out_rows.numel() != rows:
            raise ValueError("layernorm: out_rows needs one entry per row")
        _lib.check(lib.far3d_layernorm_rows(*args, _ptr(out_rows), _stream(x)), "far3d_layernorm_rows")
    else:
        _lib.check(lib.far3d_layernorm(*args, _stream(x)), "far3d_layernorm")
    res = (y,) + ((y2,) if y2 is not None else ()) + ((yb,) if yb is not None else ())
    return res if len(res) > 1 else y


def _norm_operands(who, x, pair, *views):
    """What the NHWC normalisation wrappers do alike.  x: (N,H,W,C) (pair: a pair-stored bf16 map of 2C stored channels, checked under the
    wrapper's name `who`).  views: (tensor | None, name) pairs.  Returns N, H, W, the logical C, the storage code and, per view, what
    the library takes: (pointer, pixel stride, image stride), (None, 0, 0) for an absent one."""
    N, H, W, C = x.shape
    if pair:
        if x.dtype != torch.bfloat16 or C % 64:
            raise ValueError("%s: pair storage is bf16 with a multiple of 64 stored channels" % who)
        C //= 2
    args = tuple((None, 0, 0) if t is None else (_ptr(t),) + _nhwc_view(t, name) for t, name in views)
    return (N, H, W, C, DT_BF16_PAIR if pair else _dt(x)) + args


def _norm_scratch(who, scratch, N, C, device):
    """The ese_scratch_floats(N, C) f32 workspace of ese_nhwc / groupnorm_nhwc: allocated when None, refused when too small."""
    if scratch is None:
        scratch = torch.empty(ese_scratch_floats(N, C), dtype=torch.float32, device=device)
    if scratch.numel() < ese_scratch_floats(N, C):
        raise ValueError("%s: scratch needs %d floats" % (who, ese_scratch_floats(N, C)))
    return scratch


def ese_nhwc(x, fcw, fcb, identity=None, out=None, scratch=None, pair=False, sums=None):
    """x * hsigmoid(fc(mean_hw x)) (+ identity) on NHWC views (any channel slice / pixel stride).  scratch: optional
    ese_scratch_floats(N, C) f32 workspace (never needs zeroing; the pooling is deterministic).  pair: x / identity / out are
    pair-stored bf16 maps (2C stored channels).  sums: the int64 channel sums conv2d_nhwc(..., sums=) accumulated while it produced
    x -- the pooling pass is skipped and the sums come back zeroed."""
    lib = _lib.require_device()
    if out is None:
        out = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device)
    N, H, W, C, dt, (xp, ldx, xs), (yp, ldy, ys), (ip, ldi, isd) = _norm_operands("ese_nhwc", x, pair, (x, "x"), (out, "out"), (identity, "identity"))
    scratch = _norm_scratch("ese_nhwc", scratch, N, C, x.device)
    _lib.check(lib.far3d_ese_nhwc(xp, dt, _ptr(fcw), _ptr(fcb), ip, yp, _ptr(scratch), N, H * W, C,
                                  ldx, xs, ldi, isd, ldy, ys, _sums_ptr(sums, N, C), _stream(x)), "far3d_ese_nhwc")
    return out


def ese_fused_ok(x, pair=False):
    """Whether ese_fused_nhwc takes this map: bf16 / pair storage, 8-channel (16-byte) pieces everywhere."""
    C = x.shape[-1] // (2 if pair else 1)
    return x.dtype == torch.bfloat16 and C % (32 if pair else 8) == 0 and C <= 1024 and x.stride(2) % 8 == 0 and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0


def maxpool_out_hw(H, W):
    """MaxPool2d(3, 2, ceil_mode=True) output size (ref models/backbones/vovnet.py:249-250)."""
    Ho, Wo = -(-(H - 3) // 2) + 1, -(-(W - 3) // 2) + 1
    if (Ho - 1) * 2 >= H:
        Ho -= 1
    if (Wo - 1) * 2 >= W:
        Wo -= 1
    return Ho, Wo


def ese_fused_nhwc(x, fcw, fcb, sums, gate, identity=None, out=None, pooled=None, pair=False):
    """eSE with the stage-end pooling fused into the apply pass (far3d_ese_fused_nhwc): gates from the fixed-point channel sums `sums` of
    the concat convolution, y = x * gate (+ identity) into `out` (None: not written) and, optionally, MaxPool2d(3, 2, ceil_mode=True)(y) into
    `pooled` (an NHWC view, e.g. the input slice of the next stage's concat buffer).  gate: >= N*C floats of workspace."""
    lib = _lib.require_device()
    if out is None and pooled is None:
        raise ValueError("ese_fused_nhwc: nothing to write (out and pooled are both None)")
    N, H, W, C, dt, (xp, ldx, xs), (yp, ldy, ys), (ip, ldi, isd), (pp, ldp, ps) = _norm_operands(
        "ese_fused_nhwc", x, pair, (x, "x"), (out, "out"), (identity, "identity"), (pooled, "pooled"))
    Hp, Wp = (pooled.shape[1], pooled.shape[2]) if pooled is not None else (0, 0)
    if gate.numel() < N * C or gate.dtype != torch.float32:
        raise ValueError("ese_fused_nhwc: gate needs N*C floats")
    _lib.check(lib.far3d_ese_fused_nhwc(xp, dt, _ptr(fcw), _ptr(fcb), ip, yp, pp, _ptr(gate), N, H, W, C,
                                        ldx, xs, ldi, isd, ldy, ys, Hp, Wp, ldp, ps, _sums_ptr(sums, N, C), _stream(x)), "far3d_ese_fused_nhwc")
    return out if out is not None else pooled


def groupnorm_nhwc(x, gamma, beta, groups=32, eps=1e-5, relu=True, out=None, scratch=None, pair=False):
    lib = _lib.require_device()
    _chk(x, "x", ndim=4)
    N, H, W, C, dt = _norm_operands("groupnorm_nhwc", x, pair)
    if out is None:
        out = torch.empty_like(x)
    scratch = _norm_scratch("groupnorm_nhwc", scratch, N, C, x.device)
    _lib.check(lib.far3d_groupnorm_nhwc(_ptr(x), dt, _ptr(gamma), _ptr(beta), _ptr(out), _ptr(scratch), N, H * W, C,
                                        groups, float(eps), 1 if relu else 0, _stream(x)), "far3d_groupnorm_nhwc")
    return out


def maxpool3x3s2_nhwc(x, out=None, pair=False):
    lib = _lib.require_device()
    _chk(x, "x", ndim=4)
    Ho, Wo = maxpool_out_hw(x.shape[1], x.shape[2])
    if out is None:
        out = torch.empty((x.shape[0], Ho, Wo, x.shape[3]), dtype=x.dtype, device=x.device)
    N, H, W, C, dt, (yp, ldy, ys) = _norm_operands("maxpool3x3s2_nhwc", x, pair, (out, "out"))
    _lib.check(lib.far3d_maxpool3x3s2_nhwc(_ptr(x), dt, yp, N, H, W, C, Ho, Wo, ldy, ys, _stream(x)), "far3d_maxpool3x3s2_nhwc")
    return out


def pack_dw3x3(weight, device=None):
    """Depthwise 3x3 weights (C,1,3,3) -> the kernel's [9][C] f32 layout, w9c[ky*3 + kx][c] = weight[c][0][ky][kx]."""
    C = weight.shape[0]
    if tuple(weight.shape) != (C, 1, 3, 3):
        raise ValueError("pack_dw3x3: expected a (C,1,3,3) depthwise weight, got %s" % (tuple(weight.shape),))
    w = weight.detach().float().reshape(C, 9).t().contiguous()
    return w.to(device) if device is not None else w


DW_ACTS = {None: 0, "none": 0, "relu": 1, "swish": 2}


def _dw_act(act):
    """None | "relu" | "swish" (or the library's code 0 / 1 / 2) -> the library's code."""
    return DW_ACTS[act] if (act is None or isinstance(act, str)) else int(act)


def _dw_operands(who, x, pair, w, w_name, w_ndim, w_text, bias, b_name, stride, out, out_text="", sets=1, Cout=None):
    """What the three depthwise wrappers do alike.  x: NHWC view (pair: bf16 with 2C stored channels).  w: f32 whose last two dimensions
    are (9, C) (`w_text`: its message, taking the shape and C); bias: None or f32 of w's leading dimensions + (C,).  out: None (allocated
    for 3x3 / pad 1 / `stride`) or an NHWC view of x's storage with Cout (None: sets * C) logical channels (`out_text` ends its message).
    Returns the storage code, C, out and the library's arguments of the two maps: (ldx, x_img_stride), (Ho, Wo, ldy, y_img_stride)."""
    N, H, W, Cs = x.shape
    cs = 2 if pair else 1
    C = Cs // cs
    if pair and x.dtype != torch.bfloat16:
        raise TypeError("%s: pair storage is bf16" % who)
    _chk(w, w_name, torch.float32, w_ndim)
    if tuple(w.shape[-2:]) != (9, C):
        raise ValueError(("%s: " + w_text) % (who, tuple(w.shape), C))
    if bias is not None:
        _chk(bias, b_name, torch.float32, w.dim() - 1)
        if tuple(bias.shape) != tuple(w.shape[:-2]) + (C,):
            raise ValueError("%s: %s %s != %s" % (who, b_name, tuple(bias.shape), tuple(w.shape[:-2]) + (C,)))
    xv = _nhwc_view(x, "x")
    Cy = (sets * C if Cout is None else Cout) * cs
    if out is None:
        s = int(stride)
        if s < 1:
            raise ValueError("%s: stride %r" % (who, stride))
        out = torch.empty((N, (H - 1) // s + 1, (W - 1) // s + 1, Cy), dtype=x.dtype, device=x.device)
    if out.dtype != x.dtype or out.shape[0] != N or out.shape[3] != Cy:
        raise ValueError("%s: out %s %s does not match x %s %s%s" % (who, tuple(out.shape), out.dtype, tuple(x.shape), x.dtype, out_text))
    return (DT_BF16_PAIR if pair else _dt(x)), C, out, xv, (out.shape[1], out.shape[2]) + _nhwc_view(out, "out")


def dwconv3x3_nhwc(x, w9c, stride, out=None, pair=False):
    """Depthwise 3x3 / pad 1 / stride 1|2 convolution without bias or activation (nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False)) on
    an NHWC view x (f32 | bf16; pair: a pair-stored bf16 map of 2C stored channels).  w9c: (9, C) f32 (pack_dw3x3).  out: optional NHWC view
    of x's storage (a channel slice of a wider buffer is fine).  Sizes, strides and alignment are checked by the library
    (Far3dHipError, nothing launched)."""
    lib = _lib.require_device()
    dt, C, out, (ldx, xs), (Ho, Wo, ldy, ys) = _dw_operands("dwconv3x3_nhwc", x, pair, w9c, "w9c", 2, "weights %s != (9, %d)", None, None,
                                                            stride, out)
    _lib.check(lib.far3d_dwconv3x3_nhwc(_ptr(x), dt, _ptr(w9c), _ptr(out), x.shape[0], x.shape[1], x.shape[2], C, ldx, xs, Ho, Wo, ldy, ys,
                                        int(stride), _stream(x)), "far3d_dwconv3x3_nhwc")
    return out


def pack_dw3x3_sets(weights, biases=None, device=None):
    """One or two depthwise layers of the same width -> far3d_dwconv3x3_act_nhwc's operands: (reps, 9, C) f32 weights (pack_dw3x3 per
    set) and the (reps, C) f32 biases (None: no bias).  weights: a list of (C,1,3,3) tensors; biases: a list of (C,) tensors."""
    w = torch.stack([pack_dw3x3(wi) for wi in weights]).contiguous()
    b = None if biases is None else torch.stack([bi.detach().float() for bi in biases]).contiguous()
    if b is not None and tuple(b.shape) != (w.shape[0], w.shape[2]):
        raise ValueError("pack_dw3x3_sets: biases %s do not match weights %s" % (tuple(b.shape), tuple(w.shape)))
    if device is not None:
        w, b = w.to(device), (None if b is None else b.to(device))
    return w, b


def dwconv3x3_act_nhwc(x, w, stride, bias=None, act=None, out=None, pair=False):
    """dwconv3x3_nhwc with a bias, an activation and one or two weight sets per window: out[..., r*C + c] = act(dw(x[..., c]; w[r]) + bias[r][c]).
    w: (reps, 9, C) f32 (a (9, C) tensor is one set), reps 1 or 2; bias: (reps, C) f32 or None; act: None | "relu" | "swish" (or the
    library's code 0 / 1 / 2).  out: optional NHWC view of x's storage with reps*C logical channels.  With reps = 1, no bias and no
    activation the result is dwconv3x3_nhwc's, bit for bit.  Sizes, strides, alignment, reps and act are checked by the library
    (Far3dHipError, nothing launched)."""
    lib = _lib.require_device()
    if w.dim() == 2:
        w = w[None]
    if bias is not None and bias.dim() == 1:
        bias = bias[None]
    reps = w.shape[0] if w.dim() == 3 else 1
    dt, C, out, (ldx, xs), (Ho, Wo, ldy, ys) = _dw_operands("dwconv3x3_act_nhwc", x, pair, w, "w", 3, "weights %s != (reps, 9, %d)", bias, "bias",
                                                            stride, out, " with %d weight sets" % reps, sets=reps)
    _lib.check(lib.far3d_dwconv3x3_act_nhwc(_ptr(x), dt, _ptr(w), _ptr(bias) if bias is not None else None, _ptr(out), x.shape[0], x.shape[1],
                                            x.shape[2], C, ldx, xs, Ho, Wo, ldy, ys, int(stride), int(reps), _dw_act(act), _stream(x)),
               "far3d_dwconv3x3_act_nhwc")
    return out


DWSEP_MAX_COUT = 256


def dwsep_supported(C, Cout, stride, storage):
    """Does far3d_dwsep_conv_nhwc (dwsep_conv_nhwc) take a depthwise-separable layer of C -> Cout channels at this stride on maps of
    this storage?  storage: "bf16" | "pair" | "f32" (or the DT_* code / torch dtype of the maps).  A host predicate: no device, no
    library.  The rules are the library's: bf16 or pair storage, C and Cout multiples of 32, Cout <= 256, stride 1 or 2."""
    storage = {DT_BF16: "bf16", DT_BF16_PAIR: "pair", DT_F32: "f32", torch.bfloat16: "bf16", torch.float32: "f32"}.get(storage, storage)
    if storage not in ("bf16", "pair"):
        return False
    C, Cout = int(C), int(Cout)
    return C > 0 and Cout > 0 and C % 32 == 0 and Cout % 32 == 0 and Cout <= DWSEP_MAX_COUT and stride in (1, 2)


def dwsep_conv_nhwc(x, w9, pc, stride, bias1=None, act1=None, act2=None, out=None, pair=False):
    """A depthwise-separable layer in one launch: act2(pc(act1(dw3x3(x; w9) + bias1))), the result of dwconv3x3_act_nhwc followed by
    conv2d_nhwc(., pc, act=act2) without the map between them (the depthwise half bit for bit, the pointwise sums in another order).
    x: NHWC view, bf16 (pair: a pair-stored map of 2C stored channels).  w9: (9, C) f32 (pack_dw3x3; a (1, 9, C) set of
    pack_dw3x3_sets is taken too).  pc: the 1x1 PackedConv the two-launch path uses (bf16 weights for bf16 maps, split weights for
    pair-stored ones).  bias1: (C,) f32 or None.  act1 / act2: None | "relu" | "swish".  out: optional NHWC view of x's storage with
    pc.Cout logical channels.  What dwsep_supported refuses, a misaligned view or an overlap of x and out is an error of the library
    (Far3dHipError, nothing launched) -- there is no two-launch fallback in here."""
    lib = _lib.require_device()
    if w9.dim() == 3 and w9.shape[0] == 1:
        w9 = w9[0]
    if bias1 is not None and bias1.dim() == 2 and bias1.shape[0] == 1:
        bias1 = bias1[0]
    dt, C, out, (ldx, xs), (Ho, Wo, ldy, ys) = _dw_operands("dwsep_conv_nhwc", x, pair, w9, "w9", 2, "depthwise weights %s != (9, %d)", bias1,
                                                            "bias1", stride, out, " and %d output channels" % pc.Cout, Cout=pc.Cout)
    if (pc.KH, pc.KW, pc.stride, pc.pad) != (1, 1, 1, 0) or pc.Cin != C or pc.terms != 3:
        raise ValueError("dwsep_conv_nhwc: pc must be a 1x1 / stride 1 / pad 0 layer of %d input channels with full products" % C)
    _lib.check(lib.far3d_dwsep_conv_nhwc(_ptr(x), dt, _ptr(w9), _ptr(bias1) if bias1 is not None else None, _dw_act(act1), _ptr(pc.w),
                                         pc.w_code, _ptr(pc.bias) if pc.bias is not None else None, _dw_act(act2), _ptr(out), x.shape[0],
                                         x.shape[1], x.shape[2], C, ldx, xs, Ho, Wo, pc.Cout, ldy, ys, int(stride), _stream(x)),
               "far3d_dwsep_conv_nhwc")
    return out


# --------------------------------------------------------------------------------------------------
# front-end glue: stem im2col, 2D proposals, MLN apply
# --------------------------------------------------------------------------------------------------
def stem_im2col(img, out_dtype=torch.bfloat16, out=None, pair=False):
    """(N,3,H,W) f32 NCHW -> (N,Ho,Wo,32) NHWC im2col of the stride-2 3x3 stem conv (pair: (N,Ho,Wo,64) bf16 pair storage)."""
    lib = _lib.require_device()
    _chk(img, "img", torch.float32, 4)
    N, C, H, W = img.shape
    if C != 3:
        raise ValueError("stem_im2col expects 3 input channels")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, 64 if pair else 32), dtype=torch.bfloat16 if pair else out_dtype, device=img.device)
    _lib.check(lib.far3d_stem_im2col(_ptr(img), _ptr(out), DT_BF16_PAIR if pair else _dt(out), N, H, W, _stream(img)), "far3d_stem_im2col")
    return out


def stem_conv(img, pc, act="relu", out=None):
    """VoVNet's first stem convolution (3 -> 64, 3x3, stride 2, pad 1) straight from the (N,3,H,W) f32 NCHW image: bf16 NHWC output,
    bit-identical to conv2d_nhwc(stem_im2col(img), pc).  pc: the layer packed as a 1x1 conv over the 32-channel im2col rows (bf16)."""
    lib = _lib.require_device()
    _chk(img, "img", torch.float32, 4)
    N, C, H, W = img.shape
    if C != 3 or pc.Cout != 64 or pc.Cin != 32 or pc.KH != 1 or pc.w.dtype != torch.bfloat16:
        raise ValueError("stem_conv: 3-channel image and the 64 x 32 bf16 packing of the stem layer")
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if out is None:
        out = torch.empty((N, Ho, Wo, 64), dtype=torch.bfloat16, device=img.device)
    ldy, ys = _nhwc_view(out, "out")
    _lib.check(lib.far3d_stem_conv(_ptr(img), _ptr(pc.w), _ptr(pc.bias) if pc.bias is not None else None, _ptr(out), N, H, W, ldy, ys,
                                   {None: 0, "relu": 1}[act], _stream(img)), "far3d_stem_conv")
    return out


def _ptr_array(tensors):
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr


def proposal_select(cls_maps, reg_maps, strides, cap, thr=0.1, topk=False):
    """cls_maps[l] (N,h,w,ncls) f32, reg_maps[l] (N,h,w,>=5) f32 (dx,dy,logw,logh,obj).  Returns
    (weights (N,S) f32, sel_idx (N,cap) i32, sel_cnt (N) i32) -- all on device, no sync."""
    lib = _lib.require_device()
    L = len(cls_maps)
    for t in list(cls_maps) + list(reg_maps):
        _chk(t, "cls/reg map", torch.float32, 4)
    N = cls_maps[0].shape[0]
    hw = [(int(c.shape[1]), int(c.shape[2])) for c in cls_maps]
    S = sum(h * w for h, w in hw)
    dev = cls_maps[0].device
    sw = torch.empty((N, S), dtype=torch.float32, device=dev)
    wgt = torch.empty((N, S), dtype=torch.float32, device=dev)
    sel_idx = torch.empty((N, cap), dtype=torch.int32, device=dev)     # entries >= sel_cnt[n] are never read
    sel_cnt = torch.empty((N,), dtype=torch.int32, device=dev)
    hk, hp = _host_i32([list(x) for x in hw])
    sk, sp = _host_i32(list(strides))
    ca, ra = _ptr_array(cls_maps), _ptr_array(reg_maps)
    _lib.check(lib.far3d_proposal_select(ca, ra, cls_maps[0].shape[3], reg_maps[0].shape[3], N, L, hp, sp, _ptr(sw), _ptr(wgt),
                                         _ptr(sel_idx), _ptr(sel_cnt), cap, float(thr), 1 if topk else 0, _stream(wgt)),
               "far3d_proposal_select")
    return wgt, sel_idx, sel_cnt


def _opt_ptr(t):
    return _ptr(t) if t is not None else None


def _chk_i32_scalars(*ts):
    for t in (t for t in ts if t is not None):
        _chk(t, "m_out / overflow_out", torch.int32)


class _PropOperands:
    """The common part of proposal_gather / proposal_gather_md / proposal_extra_rows / proposal_from_boxes: the tensor checks (depth map,
    img2lidar, tokens, records = (flags, info)) and the C arguments every entry takes in the same form: the level table (reg-map
    pointers, nreg, L, sizes, strides), the depth-config triple and pc_range.  The host arrays live as long as the object."""

    def __init__(self, depth_cfg, pc_range, img2lidar, depth=None, depth_name="depth_logit", feat=None, reg_maps=None, strides=None, records=None):
        if depth is not None:
            _chk(depth, depth_name, torch.float32, 4)
        _chk(img2lidar, "img2lidar", torch.float32, 3)
        if feat is not None:
            _chk(feat, "feat", ndim=3)
        if records is not None:
            _chk(records[0], "md_flags", torch.int32, 1)
            _chk(records[1], "md_info", torch.int32, 2)
        if reg_maps is not None:
            self._hw, hp = _host_i32([[int(c.shape[1]), int(c.shape[2])] for c in reg_maps])
            self._st, sp = _host_i32(list(strides))
            self._ra = _ptr_array(reg_maps)
            self.levels = (self._ra, reg_maps[0].shape[3], len(reg_maps), hp, sp)     # reg, nreg, L, level_hw, strides
        self._pc, self.pc_range = _host_f32(list(pc_range))
        self.depth_cfg = (float(depth_cfg["depth_min"]), float(depth_cfg["depth_max"]), int(depth_cfg["num_depth_bins"]))


def _proposal_gather(fn, name, p, N, cap, sel_idx, sel_cnt, weights, depth_logit, depth_stride, img2lidar, feat, score_thr, out, tail):
    """The call far3d_proposal_gather and far3d_proposal_gather_md share up to the four outputs; tail: the entry's own arguments."""
    reg, nreg, L, hp, sp = p.levels
    _, hd, wd, nd = depth_logit.shape
    _lib.check(fn(reg, nreg, N, L, hp, sp, _ptr(sel_idx), _ptr(sel_cnt), cap, _ptr(weights), _ptr(depth_logit), hd, wd, nd,
                  int(depth_stride), *p.depth_cfg, _ptr(img2lidar), _ptr(feat), _dt(feat), feat.shape[2], p.pc_range, float(score_thr),
                  *[_ptr(t) for t in out], *tail, _stream(feat)), name)
    return tuple(out)


def proposal_gather(reg_maps, strides, sel_idx, sel_cnt, weights, depth_logit, depth_stride, depth_cfg, img2lidar,
                    feat, pc_range, score_thr=0.1, out=None, rows_total=0, m_out=None, overflow_out=None):
    """Returns ref2d (N*cap,3), ctx (N*cap,C+1), box2d (N*cap,4), score (N*cap); rows >= sum(sel_cnt) are NOT written
    (callers slice [:M]).  out: optional (ref2d, ctx, box2d, score) buffers to write into.
    rows_total > 0: fixed-capacity mode -- the buffers have rows_total rows, rows past M = sum(sel_cnt) are zero-filled, m_out /
    overflow_out (int32 device tensors of one element) receive min(M, rows_total) and the dropped-proposal flag."""
    lib = _lib.require_device()
    N, cap = sel_idx.shape
    p = _PropOperands(depth_cfg, pc_range, img2lidar, depth=depth_logit, feat=feat, reg_maps=reg_maps, strides=strides)
    C = feat.shape[2]
    dev = feat.device
    M = N * cap if not rows_total else int(rows_total)
    if out is not None:
        ref2d, ctx, box2d, score = out
    else:
        ref2d = torch.empty((M, 3), dtype=torch.float32, device=dev)
        ctx = torch.empty((M, C + 1), dtype=torch.float32, device=dev)
        box2d = torch.empty((M, 4), dtype=torch.float32, device=dev)
        score = torch.empty((M,), dtype=torch.float32, device=dev)
    if ref2d.stride(0) != 3 or ctx.stride(0) != C + 1:
        raise ValueError("proposal_gather: ref2d / ctx must be dense rows")
    if rows_total and min(ref2d.shape[0], ctx.shape[0], box2d.shape[0], score.shape[0]) < rows_total:
        raise ValueError("proposal_gather: the output buffers need rows_total=%d rows" % rows_total)
    _chk_i32_scalars(m_out, overflow_out)
    return _proposal_gather(lib.far3d_proposal_gather, "far3d_proposal_gather", p, N, cap, sel_idx, sel_cnt, weights, depth_logit,
                            depth_stride, img2lidar, feat, score_thr, (ref2d, ctx, box2d, score),
                            (int(rows_total), _opt_ptr(m_out), _opt_ptr(overflow_out)))


def depth_range_min_bin(depth_cfg, range_min):
    """The depth bin of `range_min` metres, as the reference computes it (farhead.py:521-531 with inverse=True, called at :758): the
    inverse LID map on a one-element tensor in torch's default dtype, truncated to int64."""
    dmin, dmax, nb = float(depth_cfg["depth_min"]), float(depth_cfg["depth_max"]), int(depth_cfg["num_depth_bins"])
    bin_size = 2 * (dmax - dmin) / (nb * (1 + nb))
    t = torch.tensor([range_min])
    return int((-0.5 + 0.5 * torch.sqrt(1 + 8 * (t - dmin) / bin_size)).type(torch.int64).item())


def proposal_gather_md(reg_maps, strides, sel_idx, sel_cnt, weights, depth_logit, depth_stride, depth_cfg, img2lidar, feat, pc_range,
                       topk, range_min_bin, records, out, primary_rows=0, score_thr=0.1):
    """Multi-depth proposals, part 1 (per camera block): the primary rows of proposal_gather, bit for bit, into out = (ref2d, ctx,
    box2d, score) (rows [0, N*cap), or [0, primary_rows) in fixed-capacity mode), and a record per primary into records = (flags
    (rows,) int32, info (rows, 2*topk) int32) for proposal_extra_rows.  2 <= topk <= 8."""
    lib = _lib.require_device()
    N, cap = sel_idx.shape
    ref2d, ctx, box2d, score = out
    flags, info = records
    p = _PropOperands(depth_cfg, pc_range, img2lidar, depth=depth_logit, feat=feat, reg_maps=reg_maps, strides=strides, records=records)
    rows = int(primary_rows) if primary_rows else N * cap
    if ref2d.stride(0) != 3 or ctx.stride(0) != feat.shape[2] + 1:
        raise ValueError("proposal_gather_md: ref2d / ctx must be dense rows")
    if min(ref2d.shape[0], ctx.shape[0], box2d.shape[0], score.shape[0], flags.shape[0], info.shape[0]) < rows or info.shape[1] != 2 * topk:
        raise ValueError("proposal_gather_md: the output buffers and records need %d rows (info: %d columns)" % (rows, 2 * topk))
    return _proposal_gather(lib.far3d_proposal_gather_md, "far3d_proposal_gather_md", p, N, cap, sel_idx, sel_cnt, weights, depth_logit,
                            depth_stride, img2lidar, feat, score_thr, (ref2d, ctx, box2d, score),
                            (int(primary_rows), int(topk), int(range_min_bin), _ptr(flags), _ptr(info)))


def proposal_extra_rows(sel_cnt, sel_cap, primary_rows, topk, records, img2lidar, depth_cfg, pc_range, out, fill_hole=True,
                        m_out=None, overflow_out=None):
    """Multi-depth proposals, part 2 (all cameras): the extra rows after the Mp = min(sum sel_cnt, primary_rows) primaries of
    out = (ref2d, ctx, box2d, score) (rows_total = their row count), in the reference's k-major order; fill_hole zeroes rows
    [M', rows_total).  m_out / overflow_out: int32 device scalars for M' and the dropped-row flag (sel_cap > 0 also flags a camera
    that filled its selection).  One launch, no sync."""
    lib = _lib.require_device()
    _chk(sel_cnt, "sel_cnt", torch.int32, 1)
    p = _PropOperands(depth_cfg, pc_range, img2lidar, records=records)
    flags, info = records
    ref2d, ctx, box2d, score = out
    rows_total = ref2d.shape[0]
    C = ctx.shape[1] - 1
    if ref2d.stride(0) != 3 or ctx.stride(0) != C + 1 or min(ctx.shape[0], box2d.shape[0], score.shape[0]) < rows_total:
        raise ValueError("proposal_extra_rows: ref2d / ctx / box2d / score must be dense rows, as many as ref2d's")
    if min(flags.shape[0], info.shape[0]) < primary_rows or info.shape[1] != 2 * topk or img2lidar.shape[0] < sel_cnt.shape[0]:
        raise ValueError("proposal_extra_rows: records need %d rows and %d columns, img2lidar one matrix per camera" % (primary_rows, 2 * topk))
    _chk_i32_scalars(m_out, overflow_out)
    _lib.check(lib.far3d_proposal_extra_rows(_ptr(sel_cnt), sel_cnt.shape[0], int(sel_cap), int(primary_rows), int(topk), _ptr(flags),
                                             _ptr(info), _ptr(img2lidar), *p.depth_cfg, p.pc_range, C, _ptr(ref2d), _ptr(ctx), _ptr(box2d),
                                             _ptr(score), int(rows_total), 1 if fill_hole else 0, _opt_ptr(m_out), _opt_ptr(overflow_out),
                                             _stream(ctx)),
               "far3d_proposal_extra_rows")
    return ref2d, ctx, box2d, score


def mask_compact(valid, cap, overflow_out=None):
    """Ordered compaction of a token mask (far3d_hip.h far3d_mask_compact).  valid (N,S) bool | uint8 on the device, non-zero =
    selected.  Returns (sel_idx (N,cap) i32: the first min(count, cap) selected indices per camera, ascending; sel_cnt (N) i32);
    overflow_out: optional int32 device scalar, 1 when a camera holds more than cap.  No sync."""
    lib = _lib.require_device()
    _chk(valid, "valid", ndim=2)
    if valid.dtype not in (torch.bool, torch.uint8):
        raise TypeError("valid must be torch.bool or torch.uint8 (got %s)" % valid.dtype)
    N, S = valid.shape
    cap = int(cap)
    if N < 1 or S < 1 or cap < 1:
        raise ValueError("mask_compact: need N >= 1, S >= 1 and cap >= 1 (got N=%d S=%d cap=%d)" % (N, S, cap))
    if overflow_out is not None:
        _chk(overflow_out, "overflow_out", torch.int32)
    sel_idx = torch.empty((N, cap), dtype=torch.int32, device=valid.device)     # entries >= sel_cnt[n] are never read
    sel_cnt = torch.empty((N,), dtype=torch.int32, device=valid.device)
    _lib.check(lib.far3d_mask_compact(_ptr(valid), N, S, _ptr(sel_idx), _ptr(sel_cnt), cap,
                                      _ptr(overflow_out) if overflow_out is not None else None, _stream(valid)), "far3d_mask_compact")
    return sel_idx, sel_cnt


def proposal_from_boxes(boxes, box_cnt, scores, sel_idx, sel_cnt, depth, depth_stride, depth_cfg, img2lidar, feat, pc_range,
                        depth_is_prob=True, depth_layout="nhwc", score_thr=0.1, topk=1, range_min_bin=0, records=None, out=None,
                        mismatch_out=None, rows=None):
    """Adaptive-query rows from given boxes (far3d_hip.h far3d_proposal_from_boxes).  boxes (rows,4) f32 cxcywh camera-major with
    box_cnt (N) i32 per camera, scores (rows,) f32; sel_idx (N,cap) / sel_cnt (N) from mask_compact; depth f32 (N,hd,wd,nd)
    ("nhwc") or (N,nd,hd,wd) ("nchw"), logits or probabilities; feat (N,S,C) f32 | bf16.  Returns (ref2d (rows,3), ctx (rows,C+1))
    -- `out` gives the buffers -- of which the rows of the given boxes are written.  topk > 1: records = (flags (rows,) i32, info
    (rows,2*topk) i32) receive the multi-depth records; run proposal_extra_rows next with (ref2d, ctx, boxes, scores) as its `out`.
    rows: the rows that may hold primaries (default: all of boxes'; fewer when the buffers also hold room for the extra rows).
    mismatch_out: optional int32 device scalar, 1 when box_cnt != sel_cnt for a camera.  No sync."""
    lib = _lib.require_device()
    _chk(boxes, "boxes", torch.float32, 2)
    _chk(scores, "scores", torch.float32, 1)
    _chk(box_cnt, "box_cnt", torch.int32, 1)
    _chk(sel_idx, "sel_idx", torch.int32, 2)
    _chk(sel_cnt, "sel_cnt", torch.int32, 1)
    p = _PropOperands(depth_cfg, pc_range, img2lidar, depth=depth, depth_name="depth", feat=feat)
    if depth_layout not in ("nhwc", "nchw"):
        raise ValueError("proposal_from_boxes: depth_layout %r (nhwc or nchw)" % (depth_layout,))
    N, cap = sel_idx.shape
    S, C = int(feat.shape[1]), int(feat.shape[2])
    rows = int(boxes.shape[0]) if rows is None else int(rows)
    if depth_layout == "nhwc":
        _, hd, wd, nd = depth.shape
    else:
        _, nd, hd, wd = depth.shape
    if boxes.shape[1] != 4 or rows < 1 or boxes.shape[0] < rows or scores.shape[0] < rows:
        raise ValueError("proposal_from_boxes: boxes must be (>= rows >= 1, 4) and scores hold a value per row")
    if not (box_cnt.shape[0] == sel_cnt.shape[0] == feat.shape[0] == depth.shape[0] == N) or img2lidar.shape[0] < N:
        raise ValueError("proposal_from_boxes: box_cnt, sel_cnt, feat, depth and img2lidar need an entry per camera (%d)" % N)
    dev = feat.device
    if out is not None:
        ref2d, ctx = out[0], out[1]
    else:
        ref2d = torch.empty((rows, 3), dtype=torch.float32, device=dev)
        ctx = torch.empty((rows, C + 1), dtype=torch.float32, device=dev)
    _chk(ref2d, "ref2d", torch.float32, 2)
    _chk(ctx, "ctx", torch.float32, 2)
    if ref2d.shape[1] != 3 or ctx.shape[1] != C + 1 or min(ref2d.shape[0], ctx.shape[0]) < rows:
        raise ValueError("proposal_from_boxes: ref2d (>= %d, 3) and ctx (>= %d, %d) must be dense rows" % (rows, rows, C + 1))
    topk = int(topk)
    flags = info = None
    if topk > 1:
        if records is None:
            raise ValueError("proposal_from_boxes: topk > 1 needs records = (flags, info)")
        flags, info = records
        _chk(flags, "md_flags", torch.int32, 1)
        _chk(info, "md_info", torch.int32, 2)
        if min(flags.shape[0], info.shape[0]) < rows or info.shape[1] != 2 * topk:
            raise ValueError("proposal_from_boxes: the records need %d rows (info: %d columns)" % (rows, 2 * topk))
    if mismatch_out is not None:
        _chk(mismatch_out, "mismatch_out", torch.int32)
    _lib.check(lib.far3d_proposal_from_boxes(_ptr(boxes), _ptr(box_cnt), _ptr(scores), rows, _ptr(sel_idx), _ptr(sel_cnt), cap, N, S,
                                             _ptr(depth), 0 if depth_layout == "nhwc" else 1, 1 if depth_is_prob else 0, hd, wd, nd,
                                             int(depth_stride), *p.depth_cfg, _ptr(img2lidar), _ptr(feat), _dt(feat), C, p.pc_range,
                                             float(score_thr), _ptr(ref2d), _ptr(ctx), topk, int(range_min_bin), _opt_ptr(flags),
                                             _opt_ptr(info), _opt_ptr(mismatch_out), _stream(feat)),
               "far3d_proposal_from_boxes")
    return ref2d, ctx


def proposal_merge_blocks(blocks, out, sel_cnt_out, primary_rows, records_out=None, m_out=None, overflow_out=None):
    """The proposals of camera blocks -> the frame's layout (far3d_hip.h far3d_proposal_merge_blocks).  blocks: dicts in ascending
    camera order with rows = (ref2d, ctx, box2d, score) of the block's own buffers, sel_cnt (cams,) int32, first_cam, and optionally
    records = (flags, info) (multi-depth; all blocks or none), count (int32 device scalar, or a static int; absent: min(sum sel_cnt,
    the buffers' rows)) and overflow (int32 device scalar).  out = the frame's (ref2d, ctx, box2d, score) (rows_total = their rows):
    rows [0, Mp) receive the blocks' primaries back to back, Mp = min(sum counts, primary_rows).  records_out = the frame's (flags,
    info): multi-depth, rows past Mp are left for proposal_extra_rows; None: single depth, rows [Mp, rows_total) are zero-filled.
    sel_cnt_out (N,) int32; m_out / overflow_out: int32 device scalars for Mp and the OR of the flags | overflow.  One launch, no sync."""
    lib = _lib.require_device()
    nb = len(blocks)
    ref2d, ctx, box2d, score = out
    rows_total = ref2d.shape[0]
    C = ctx.shape[1] - 1
    _chk(sel_cnt_out, "sel_cnt_out", torch.int32, 1)
    if ref2d.stride(0) != 3 or ctx.stride(0) != C + 1 or min(ctx.shape[0], box2d.shape[0], score.shape[0]) < rows_total:
        raise ValueError("proposal_merge_blocks: ref2d / ctx / box2d / score must be dense rows, as many as ref2d's")
    if not (box2d.is_contiguous() and score.is_contiguous()) or box2d.dim() != 2 or box2d.shape[1] != 4 or score.dim() != 1:
        raise ValueError("proposal_merge_blocks: the frame's box2d (rows, 4) and score (rows,) must be contiguous")
    md = records_out is not None
    if any(("records" in b and b["records"] is not None) != md for b in blocks):
        raise ValueError("proposal_merge_blocks: multi-depth records come from every block and go to records_out, or from none")
    topk = 0
    if md:
        _chk(records_out[0], "md_flags", torch.int32, 1)
        _chk(records_out[1], "md_info", torch.int32, 2)
        topk = records_out[1].shape[1] // 2
        if min(records_out[0].shape[0], records_out[1].shape[0]) < primary_rows:
            raise ValueError("proposal_merge_blocks: records_out needs primary_rows=%d rows" % primary_rows)
    for t in (m_out, overflow_out):
        if t is not None:
            _chk(t, "m_out / overflow_out", torch.int32)
    rows_b, cams_b, cnt_host, cnt_dev, ovf = [], [], [], [], []
    for b in blocks:
        r, c, x, s = b["rows"]
        n = min(r.shape[0], c.shape[0], x.shape[0], s.shape[0])
        _chk(b["sel_cnt"], "block sel_cnt", torch.int32, 1)
        if r.stride(0) != 3 or c.stride(0) != C + 1 or c.shape[1] != C + 1 or not (x.is_contiguous() and s.is_contiguous()):
            raise ValueError("proposal_merge_blocks: a block's ref2d / ctx / box2d / score must be dense rows of the frame's widths")
        if md:
            f, i = b["records"]
            _chk(f, "block md_flags", torch.int32, 1)
            _chk(i, "block md_info", torch.int32, 2)
            if i.shape[1] != 2 * topk:
                raise ValueError("proposal_merge_blocks: a block's md_info has %d columns, the frame's %d" % (i.shape[1], 2 * topk))
            n = min(n, f.shape[0], i.shape[0])
        cnt = b.get("count")
        if isinstance(cnt, torch.Tensor):
            _chk(cnt, "block count", torch.int32)
        if b.get("overflow") is not None:
            _chk(b["overflow"], "block overflow", torch.int32)
        rows_b.append(n)
        cams_b.append(b["sel_cnt"].shape[0])
        cnt_dev.append(cnt.data_ptr() if isinstance(cnt, torch.Tensor) else None)
        cnt_host.append(-1 if cnt is None or isinstance(cnt, torch.Tensor) else int(cnt))
        ovf.append(b["overflow"].data_ptr() if b.get("overflow") is not None else None)
    pa = lambda vals: (ctypes.c_void_p * nb)(*vals)
    arr = [_ptr_array([b["rows"][k] for b in blocks]) for k in range(4)]
    rec = [_ptr_array([b["records"][k] for b in blocks]) if md else None for k in range(2)]
    hk, hp = _host_i32(cnt_host)
    fk, fp = _host_i32([int(b["first_cam"]) for b in blocks])
    ck, cp = _host_i32(cams_b)
    rk, rp = _host_i32(rows_b)
    _lib.check(lib.far3d_proposal_merge_blocks(nb, arr[0], arr[1], arr[2], arr[3], rec[0], rec[1], _ptr_array([b["sel_cnt"] for b in blocks]),
                                               pa(cnt_dev), hp, pa(ovf), fp, cp, rp, sel_cnt_out.shape[0], C, topk, int(primary_rows),
                                               int(rows_total), _ptr(ref2d), _ptr(ctx), _ptr(box2d), _ptr(score),
                                               _ptr(records_out[0]) if md else None, _ptr(records_out[1]) if md else None,
                                               _ptr(sel_cnt_out), _ptr(m_out) if m_out is not None else None,
                                               _ptr(overflow_out) if overflow_out is not None else None, _stream(ctx)),
               "far3d_proposal_merge_blocks")
    return ref2d, ctx, box2d, score


MD_BLOCK_SECTIONS = ("header", "sel_cnt", "img2lidar", "ref2d", "ctx", "box2d", "score", "md_flags", "md_info")


def md_block_layout(per, rows, E, K):
    """Word layout of the record one rank contributes to a multi-depth camera-sharded exchange (far3d_hip.h
    far3d_proposal_pack_block): `per` camera slots, `rows` = the block rows of `per` cameras, context width E, multi_depth topk K.
    -> dict(per, rows, E, K, <section>: first word ..., words: total); every section starts on a 16-byte boundary and the total is
    a multiple of 4 words, so records stacked as (world, words) stay aligned.  Host arithmetic only; the same on every rank."""
    per, rows, E, K = int(per), int(rows), int(E), int(K)
    if per < 1 or rows < 1 or E < 1 or not 2 <= K <= 8:
        raise ValueError("md_block_layout: per, rows, E >= 1 and 2 <= K <= 8 (got %s)" % ((per, rows, E, K),))
    sizes = (4, per, per * 16, rows * 3, rows * (E + 1), rows * 4, rows, rows, rows * 2 * K)
    lay = dict(per=per, rows=rows, E=E, K=K)
    o = 0
    for name, n in zip(MD_BLOCK_SECTIONS, sizes):
        lay[name] = o
        o = (o + n + 3) // 4 * 4
    lay["words"] = o
    return lay


def proposal_pack_block(st, record, layout, count=None, overflow=None):
    """Pack a multi-depth camera block into its record (far3d_hip.h far3d_proposal_pack_block).  st: the result of
    camera_stage(..., block_rows=...) for the block (ref2d, ctx, box2d, score2d, sel_cnt, md.records, md.img2lidar), or None for the
    empty block of a rank without cameras.  record: (words,) or (1, words) float32, layout = md_block_layout(...).  count: the static
    number of valid rows (top-K mode: cameras * K) or None (fixed-capacity mode: min(sum sel_cnt, the block's rows), a larger sum
    raises the record's overflow flag); overflow: optional int32 device scalar OR-ed into that flag.  One launch, no sync."""
    lib = _lib.require_device()
    _chk(record, "record", torch.float32)
    L = layout
    if record.numel() != L["words"]:
        raise ValueError("proposal_pack_block: the record has %d words, the layout %d" % (record.numel(), L["words"]))
    if overflow is not None:
        _chk(overflow, "overflow", torch.int32)
    ovf = _ptr(overflow) if overflow is not None else None
    if st is None:
        if count not in (None, 0):
            raise ValueError("proposal_pack_block: the empty block has no rows (count=%s)" % (count,))
        args = [0, L["per"], 0, L["rows"], L["E"], L["K"]] + [None] * 8 + [-1 if count is None else 0, ovf]
    else:
        flags, info = st["md"]["records"]
        i2l = st["md"]["img2lidar"]
        ref2d, ctx, box2d, score, sel_cnt = st["ref2d"], st["ctx"], st["box2d"], st["score2d"], st["sel_cnt"]
        for t, name, dt in ((ref2d, "ref2d", torch.float32), (ctx, "ctx", torch.float32), (box2d, "box2d", torch.float32),
                            (score, "score2d", torch.float32), (i2l, "img2lidar", torch.float32), (sel_cnt, "sel_cnt", torch.int32),
                            (flags, "md_flags", torch.int32), (info, "md_info", torch.int32)):
            _chk(t, name, dt)
        cams = sel_cnt.numel()
        if ref2d.shape[1:] != (3,) or ctx.shape[1:] != (L["E"] + 1,) or box2d.shape[1:] != (4,) or score.dim() != 1 or flags.dim() != 1 or \
                info.shape[1:] != (2 * L["K"],) or i2l.numel() != cams * 16:
            raise ValueError("proposal_pack_block: the block's arrays do not have the layout's widths (E=%d, K=%d)" % (L["E"], L["K"]))
        n = min(t.shape[0] for t in (ref2d, ctx, box2d, score, flags, info))
        if not 1 <= cams <= L["per"] or not 1 <= n <= L["rows"]:
            raise ValueError("proposal_pack_block: %d cameras / %d rows do not fit the layout's %d / %d" % (cams, n, L["per"], L["rows"]))
        if count is not None and not 0 <= int(count) <= n:
            raise ValueError("proposal_pack_block: count=%s outside the block's %d rows" % (count, n))
        args = [cams, L["per"], n, L["rows"], L["E"], L["K"], _ptr(sel_cnt), _ptr(i2l), _ptr(ref2d), _ptr(ctx), _ptr(box2d), _ptr(score),
                _ptr(flags), _ptr(info), -1 if count is None else int(count), ovf]
    _lib.check(lib.far3d_proposal_pack_block(*args, _ptr(record), L["words"], _stream(record)), "far3d_proposal_pack_block")
    return record


def md_block_views(record, layout, ncams, first_cam, sel_cap):
    """One rank's record (words,) float32 (e.g. a row of the gathered (world, words) buffer) -> the block dict
    Far3DEngine.merge_camera_blocks takes, made of VIEWS into the record: nothing is copied, so the views built once stay valid for
    every later frame that lands in the same buffer.  ncams / first_cam: the rank's cameras (static, from dist.camera_shards);
    sel_cap: the per-camera selection capacity of the fixed-capacity mode (0 in the top-K mode), as camera_stage's md.sel_cap.
    m_dev and overflow are the header's count and flag."""
    L = layout
    if record.dim() != 1 or record.dtype != torch.float32 or record.numel() != L["words"] or not record.is_contiguous():
        raise ValueError("md_block_views: the record must be a contiguous (%d,) float32 tensor" % L["words"])
    if not 1 <= ncams <= L["per"]:
        raise ValueError("md_block_views: %d cameras in a record of %d slots" % (ncams, L["per"]))
    rows, E, K = L["rows"], L["E"], L["K"]
    irec = record.view(torch.int32)
    f = lambda name, n, w: record[L[name]:L[name] + n * w].view(n, w)
    return dict(ref2d=f("ref2d", rows, 3), ctx=f("ctx", rows, E + 1), box2d=f("box2d", rows, 4), score2d=record[L["score"]:L["score"] + rows],
                sel_cnt=irec[L["sel_cnt"]:L["sel_cnt"] + ncams], cams=(int(first_cam), int(first_cam) + int(ncams)),
                m_dev=irec[L["header"] + 1:L["header"] + 2], overflow=irec[L["header"] + 2:L["header"] + 3],
                md=dict(records=(irec[L["md_flags"]:L["md_flags"] + rows], irec[L["md_info"]:L["md_info"] + rows * 2 * K].view(rows, 2 * K)),
                        img2lidar=record[L["img2lidar"]:L["img2lidar"] + ncams * 16].view(ncams, 4, 4), sel_cap=int(sel_cap)))


def compact_rows(src, counts, dst, m_out, overflow_out):
    """src (nblocks, rows_per_block, D) f32 with counts[b] valid rows in block b -> dst (dst_rows, D): the valid rows in block order,
    the rest zero; m_out = min(sum counts, dst_rows); overflow_out |= (sum counts > dst_rows).  One launch, no sync."""
    lib = _lib.require_device()
    _chk(src, "src", torch.float32, 3)
    _chk(counts, "counts", torch.int32, 1)
    _chk(dst, "dst", torch.float32, 2)
    _chk(m_out, "m_out", torch.int32)
    _chk(overflow_out, "overflow_out", torch.int32)
    nb, rpb, D = src.shape
    if counts.numel() != nb or dst.shape[1] != D:
        raise ValueError("compact_rows: inconsistent shapes")
    _lib.check(lib.far3d_compact_rows(_ptr(src), _ptr(counts), nb, rpb, D, _ptr(dst), dst.shape[0], _ptr(m_out), _ptr(overflow_out),
                                      _stream(src)), "far3d_compact_rows")
    return dst


def row_affine_ln(x, gamma, beta, add=None, do_ln=True, eps=1e-5, out=None):
    """out[r] = gamma[r] * LN(x[r]) + beta[r] (+ add[r]); gamma/beta/add may be a single row (broadcast).  C = 256.
    x / out / gamma / beta / add may be row-strided views (unit stride along the channels, row strides multiples of 4)."""
    lib = _lib.require_device()
    if x.dim() != 2:
        raise ValueError("row_affine_ln: x must be (rows, C) (got %s)" % (tuple(x.shape),))
    rows, C = x.shape
    bc = lambda t: 0 if (t.dim() == 1 or t.shape[0] == 1) else t.stride(0)
    if out is None:
        out = torch.empty((rows, C), dtype=torch.float32, device=x.device)
    if tuple(out.shape) != (rows, C):
        raise ValueError("row_affine_ln: out must be (%d, %d) (got %s)" % (rows, C, tuple(out.shape)))
    for t, name in ((x, "x"), (gamma, "gamma"), (beta, "beta"), (add, "add"), (out, "out")):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float32:
            raise TypeError("row_affine_ln: %s must be a float32 tensor on the HIP device" % name)
        if t.dim() not in (1, 2) or t.shape[-1] != C or t.stride(-1) != 1 or (t.dim() == 2 and t.shape[0] not in (1, rows)):
            raise ValueError("row_affine_ln: %s must be (%d, %d) or one row of %d, unit stride along the channels (got %s, strides %s)"
                             % (name, rows, C, C, tuple(t.shape), t.stride()))
    if bc(gamma) != bc(beta):
        raise ValueError("row_affine_ln: gamma and beta must broadcast alike")
    _lib.check(lib.far3d_row_affine_ln(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(add) if add is not None else None, _ptr(out),
                                       rows, C, x.stride(0), bc(gamma), bc(add) if add is not None else 0, out.stride(0),
                                       float(eps), 1 if do_ln else 0, _stream(x)), "far3d_row_affine_ln")
    return out


def camera_sorted_order(ref, lidar2img, pc_range, pad_hw, spatial=True):
    """Query order for aggregate_forward's `perm`: queries sorted by the camera whose image centre their reference point
    projects closest to, then (spatial=True) by image tile (8 x 8 coarse cells, row-major) inside that camera, so that
    consecutive workgroups of one XCD touch neighbouring pixels.  Pure scheduling hint -- results do not depend on it."""
    pc = pc_range if isinstance(pc_range, torch.Tensor) else torch.as_tensor(pc_range, dtype=torch.float32, device=ref.device)
    pts = ref * (pc[3:6] - pc[0:3]) + pc[0:3]
    p = torch.einsum("nij,aj->nai", lidar2img[:, :3, :3], pts) + lidar2img[:, :3, 3][:, None, :]       # (N,A,3)
    z = p[..., 2]
    u = p[..., 0] / z.clamp(min=1e-5) / pad_hw[1] - 0.5
    v = p[..., 1] / z.clamp(min=1e-5) / pad_hw[0] - 0.5
    cost = torch.where(z > 1e-5, u * u + v * v, torch.full_like(z, 1e9))
    cam = cost.argmin(dim=0)
    key = cam
    if spatial:
        uu = torch.gather(u, 0, cam[None])[0]
        vv = torch.gather(v, 0, cam[None])[0]
        ub = ((uu + 0.5).clamp(0, 0.999) * 8).long()
        vb = ((vv + 0.5).clamp(0, 0.999) * 8).long()
        key = (cam * 8 + vb) * 8 + ub
    return torch.sort(key, stable=True).indices.to(torch.int32).contiguous()


# --------------------------------------------------------------------------------------------------
# fused FarHead bookkeeping (glue.hip)
# --------------------------------------------------------------------------------------------------
def posemb3d(pos, dim_t128):
    lib = _lib.require_device()
    _chk(pos, "pos", torch.float32, 2)
    out = torch.empty((pos.shape[0], 384), dtype=torch.float32, device=pos.device)
    _lib.check(lib.far3d_posemb3d(_ptr(pos), _ptr(dim_t128), _ptr(out), pos.shape[0], _stream(pos)), "far3d_posemb3d")
    return out


_MEM_KEYS = (("emb", torch.float32, 3), ("ref", torch.float32, 3), ("ts", torch.float64, 3), ("pose", torch.float32, 4), ("velo", torch.float32, 3))


def _chk_memory(d, name, L=None, E=None):
    """A memory dict emb (1,L,E) ref (1,L,3) ts (1,L,1) f64 pose (1,L,4,4) velo (1,L,2): the kernels index dense buffers."""
    for k, dt, nd in _MEM_KEYS:
        _chk(d[k], "%s[%r]" % (name, k), dt, nd)
    L = d["emb"].shape[1] if L is None else L
    E = d["emb"].shape[2] if E is None else E
    want = dict(emb=(1, L, E), ref=(1, L, 3), ts=(1, L, 1), pose=(1, L, 4, 4), velo=(1, L, 2))
    for k, shp in want.items():
        if tuple(d[k].shape) != shp:
            raise ValueError("%s[%r] must be %s (got %s)" % (name, k, shp, tuple(d[k].shape)))
    return L, E


def memory_prepare(state, ego_pose_inv, timestamp, pseudo_ref, dim_t256, prev_exists, fresh, pc_range, num_propagated,
                   temp_ref_out=None):
    """state: dict emb (1,L,E) ref (1,L,3) ts (1,L,1) f64 pose (1,L,4,4) velo (1,L,2).  Returns (m dict, temp_ref, nerf, tpos)."""
    lib = _lib.require_device()
    L, E = _chk_memory(state, "memory_prepare: state")
    P = int(num_propagated)
    _chk(ego_pose_inv, "ego_pose_inv", torch.float32)
    _chk(timestamp, "timestamp", torch.float64)
    _chk(dim_t256, "dim_t256", torch.float32)
    if ego_pose_inv.numel() != 16 or timestamp.numel() != 1 or dim_t256.numel() != 256:
        raise ValueError("memory_prepare: ego_pose_inv must hold 16 values, timestamp one, dim_t256 256")
    if not 0 <= P <= L:
        raise ValueError("memory_prepare: num_propagated=%d outside [0, L=%d]" % (P, L))
    if P > 0:
        if pseudo_ref is None:
            raise ValueError("memory_prepare: num_propagated > 0 needs pseudo_ref")
        _chk(pseudo_ref, "pseudo_ref", torch.float32, 2)
        if pseudo_ref.shape[0] < P or pseudo_ref.shape[1] != 3:
            raise ValueError("memory_prepare: pseudo_ref must be (>= %d, 3) (got %s)" % (P, tuple(pseudo_ref.shape)))
    dev = state["emb"].device
    m = {k: torch.empty_like(state[k]) for k, _, _ in _MEM_KEYS}      # the kernel's five planes (an engine's memory may carry more keys)
    temp_ref = temp_ref_out if temp_ref_out is not None else torch.empty((L, 3), dtype=torch.float32, device=dev)
    if tuple(temp_ref.shape) != (L, 3) or not temp_ref.is_contiguous():
        raise ValueError("memory_prepare: temp_ref_out must be a contiguous (L,3) tensor")
    nerf = torch.empty((L, 180), dtype=torch.float32, device=dev)
    tpos = torch.empty((L, 256), dtype=torch.float32, device=dev)
    pk, pp = _host_f32(list(pc_range))
    _lib.check(lib.far3d_memory_prepare(_ptr(state["emb"]), _ptr(state["ref"]), _ptr(state["ts"]), _ptr(state["pose"]), _ptr(state["velo"]),
                                        _ptr(ego_pose_inv), _ptr(timestamp), _ptr(pseudo_ref) if P > 0 else None,
                                        _ptr(dim_t256), float(prev_exists), 1 if fresh else 0, pp, L, E, P,
                                        _ptr(m["emb"]), _ptr(m["ref"]), _ptr(m["ts"]), _ptr(m["pose"]), _ptr(m["velo"]),
                                        _ptr(temp_ref), _ptr(nerf), _ptr(tpos), _stream(temp_ref)), "far3d_memory_prepare")
    return m, temp_ref, nerf, tpos


def head_finalize(reg, ref, cls_all, pc_range, layers, num_classes, hole=None, out=None):
    """reg (layers*A, code) -> box (layers*A, code) with metres in [:3]; score (A,) = max-class sigmoid of the last layer.
    cls_all: the contiguous (layers, ..., A, num_classes) logits.  hole: rows without a query get score -inf and -inf logits in
    every layer, written into cls_all in place (see _hole).  out: optional contiguous f32 (box, score) to write into."""
    lib = _lib.require_device()
    A, code = ref.shape[0], reg.shape[1]
    _chk(cls_all, "cls_all", torch.float32)
    if cls_all.numel() != layers * A * num_classes:
        raise ValueError("head_finalize: cls_all must hold layers * A * num_classes logits")
    if out is not None:
        box, score = out
        _chk(box, "out box", torch.float32)
        _chk(score, "out score", torch.float32)
        if tuple(box.shape) != tuple(reg.shape) or tuple(score.shape) != (A,):
            raise ValueError("head_finalize: out must be (box %s, score (%d,))" % (tuple(reg.shape), A))
    else:
        box = torch.empty_like(reg)
        score = torch.empty((A,), dtype=torch.float32, device=reg.device)
    pk, pp = _host_f32(list(pc_range))
    _lib.check(lib.far3d_head_finalize(_ptr(reg), _ptr(ref), _ptr(cls_all), _ptr(box), _ptr(score), layers, A, code, num_classes, pp,
                                       *_hole(hole), _stream(reg)), "far3d_head_finalize")
    return box, score


def memory_post_update(m, topk_idx, dec_last, box_last, ego_pose, timestamp, state):
    """state <- [the K = len(topk_idx) selected queries (dec_last / box_last rows), then the first L - K slots of m], warped by ego_pose
    (K <= L; K = 0 only warps).  m and state are distinct memory dicts of the same shapes; every element of state is written."""
    lib = _lib.require_device()
    L, E = _chk_memory(state, "memory_post_update: state")
    _chk_memory(m, "memory_post_update: m", L, E)
    _chk(topk_idx, "topk_idx", torch.int64, 1)
    _chk(dec_last, "dec_last", torch.float32, 2)
    _chk(box_last, "box_last", torch.float32, 2)
    _chk(ego_pose, "ego_pose", torch.float32)
    _chk(timestamp, "timestamp", torch.float64)
    K = topk_idx.numel()
    if K > L:
        raise ValueError("memory_post_update: %d selected queries do not fit the %d memory slots" % (K, L))
    if dec_last.shape[1] != E or dec_last.shape[0] != box_last.shape[0] or box_last.shape[1] < 5:
        raise ValueError("memory_post_update: dec_last must be (A, %d) and box_last (A, code >= 5) (got %s, %s)"
                         % (E, tuple(dec_last.shape), tuple(box_last.shape)))
    if ego_pose.numel() != 16 or timestamp.numel() != 1:
        raise ValueError("memory_post_update: ego_pose must hold 16 values, timestamp one")
    if any(m[k].data_ptr() == state[k].data_ptr() for k, _, _ in _MEM_KEYS):
        raise ValueError("memory_post_update: m and state must be different buffers (slots are shifted, not updated in place)")
    _lib.check(lib.far3d_memory_post_update(_ptr(m["emb"]), _ptr(m["ref"]), _ptr(m["ts"]), _ptr(m["pose"]), _ptr(m["velo"]), _ptr(topk_idx),
                                            _ptr(dec_last), _ptr(box_last), _ptr(ego_pose), _ptr(timestamp), L, E, K,
                                            box_last.shape[1], _ptr(state["emb"]), _ptr(state["ref"]), _ptr(state["ts"]),
                                            _ptr(state["pose"]), _ptr(state["velo"]), _stream(dec_last)), "far3d_memory_post_update")


def add_cast(a, b, sum_dtype, a_dtype=None, out_sum=None, out_a=None):
    """Returns (a+b as sum_dtype, a as a_dtype or None) in one pass; a,b (rows,C) f32 contiguous.  out_sum / out_a: optional
    (rows,C) destinations with unit inner stride and any row stride (e.g. halves of one (rows,2C) operand buffer)."""
    lib = _lib.require_device()
    _chk(a, "a", torch.float32, 2)
    _chk(b, "b", torch.float32, 2)
    rows, C = a.shape
    osum = out_sum if out_sum is not None else torch.empty(a.shape, dtype=sum_dtype, device=a.device)
    oa = out_a if out_a is not None else (torch.empty(a.shape, dtype=a_dtype, device=a.device) if a_dtype is not None else None)
    for t in (osum, oa):
        if t is not None and (tuple(t.shape) != (rows, C) or t.stride(1) != 1):
            raise ValueError("add_cast: outputs must be (rows,C) with unit inner stride")
    _lib.check(lib.far3d_add_cast(_ptr(a), _ptr(b), _ptr(osum), _dt(osum), _ptr(oa) if oa is not None else None,
                                  _dt(oa) if oa is not None else 0, rows, C, osum.stride(0), oa.stride(0) if oa is not None else 0,
                                  _stream(a)), "far3d_add_cast")
    return osum, oa


def aggregation_order(ref, lidar2img, pc_range, pad_hw, out=None, hole=None, rows=None, Vc=None, tables_out=None, split=None,
                      sorted_operands=None):
    """Query order for aggregate_forward's `perm` (camera, then 8x8 image cell), one single-workgroup launch.  Groups the
    same way as camera_sorted_order(spatial=True); the order inside a cell is arbitrary (scheduling only).  hole: rows without a
    query are entered as ~a so that aggregate_forward writes zero rows for them (see _hole).  rows=(a0, a1): order only the rows
    [a0, a1) of ref; the entries are absolute row indices (pass the full-size buffers and this perm to aggregate_forward).
    Vc (layers, N, J): the same launch also computes agg_tables(Vc) (into tables_out when given); returns (perm, tables) then.
    sorted_operands: True, or a preallocated (inv (A) int32, qbase (A, 4) f32) pair -- the same launch also writes the operands of
    aggregate_forward's sorted mode (include/far3d_hip.h); they are appended to the return value as (inv, qbase)."""
    lib = _lib.require_device()
    _chk(ref, "ref", torch.float32, 2)
    a0, a1 = (0, ref.shape[0]) if rows is None else rows
    A = a1 - a0
    extra = split.extra if split is not None else 0        # AggSplit: A main entries + `extra` sibling entries (aggregate_forward variant 9)
    perm = out if out is not None else torch.empty((A + extra,), dtype=torch.int32, device=ref.device)
    if perm.numel() != A + extra:
        raise ValueError("aggregation_order: perm needs %d entries (A = %d + %d sibling slots), got %d" % (A + extra, A, extra, perm.numel()))
    pk, pp = _host_f32(list(pc_range))
    tab, layers, J = None, 0, 0
    if Vc is not None:
        _chk(Vc, "Vc", torch.float32, 3)
        layers, Nv, J = Vc.shape
        if Nv != lidar2img.shape[0]:
            raise ValueError("aggregation_order: Vc has %d cameras, lidar2img %d" % (Nv, lidar2img.shape[0]))
        tab = tables_out if tables_out is not None else torch.empty((layers, 2 + Nv, J), dtype=torch.float32, device=ref.device)
    inv = qbase = None
    if sorted_operands is not None and sorted_operands is not False:
        if split is not None:
            raise ValueError("aggregation_order: sorted operands and sibling workgroups (split) do not combine")
        if sorted_operands is True:
            inv = torch.empty((A,), dtype=torch.int32, device=ref.device)
            qbase = torch.empty((A, 4), dtype=torch.float32, device=ref.device)
        else:
            inv, qbase = sorted_operands
        _chk(inv, "inv", torch.int32, 1)
        _chk(qbase, "qbase", torch.float32, 2)
        if inv.numel() != A or tuple(qbase.shape) != (A, 4):
            raise ValueError("aggregation_order: inv needs A = %d entries and qbase the shape (A, 4)" % A)
    _lib.check(lib.far3d_agg_order(_ptr(ref), _ptr(lidar2img), _ptr(perm), A, lidar2img.shape[0], pp, float(pad_hw[0]), float(pad_hw[1]),
                                   *_hole(hole), int(a0), _ptr(Vc) if Vc is not None else None, _ptr(tab) if tab is not None else None,
                                   layers, J, int(extra), _ptr(inv) if inv is not None else None, _ptr(qbase) if qbase is not None else None,
                                   _stream(ref)), "far3d_agg_order")
    res = (perm,) + ((tab,) if Vc is not None else ()) + (((inv, qbase),) if inv is not None else ())
    return res if len(res) > 1 else perm


def topk(vals, K, with_values=False):
    """Descending top-K indices (int64) of a 1-D f32 device tensor (n <= 40960, K <= 1024), ties -> lower index."""
    lib = _lib.require_device()
    _chk(vals, "vals", torch.float32, 1)
    idx = torch.empty((K,), dtype=torch.int64, device=vals.device)
    out = torch.empty((K,), dtype=torch.float32, device=vals.device) if with_values else None
    _lib.check(lib.far3d_topk(_ptr(vals), vals.numel(), int(K), _ptr(idx), _ptr(out) if out is not None else None, _stream(vals)),
               "far3d_topk")
    return (idx, out) if with_values else idx


DECODE_CHUNK = 40960     # logits one workgroup ranks (csrc/post.hip)


def decode_ws_bytes(n, K):
    """FAR3D_DECODE_WS_BYTES: workspace far3d_decode_topk needs for n = A * num_classes logits (0: single-launch path)."""
    return 0 if n <= DECODE_CHUNK else -(-n // DECODE_CHUNK) * K * 8


def _decode_outputs(dev, n, code, K, workspace, B=None):
    """The decode's outputs for n = A * ncls logits per stream (each with a leading B for B streams) and its workspace, allocated here when
    the chunked decode needs one and none, or too small a one, is given: (dict, workspace | None, workspace bytes per stream)."""
    lead = () if B is None else (B,)
    res = dict(boxes_3d=torch.empty(lead + (K, code - 1), dtype=torch.float32, device=dev),
               scores_3d=torch.empty(lead + (K,), dtype=torch.float32, device=dev),
               labels_3d=torch.empty(lead + (K,), dtype=torch.int64, device=dev),
               keep=torch.empty(lead + (K,), dtype=torch.bool, device=dev))
    need = decode_ws_bytes(n, K)
    total = need * (1 if B is None else B)
    if need and (workspace is None or workspace.numel() * workspace.element_size() < total):
        workspace = torch.empty((total,), dtype=torch.uint8, device=dev)
    return res, (workspace if need else None), need


def decode_topk(cls_last, box_last, K, post_center_range, workspace=None, mem_scores=None, mem_K=None):
    """NMS-free decode of the last layer: returns dict(boxes_3d (K,code-1), scores_3d (K), labels_3d (K) i64, keep (K) bool).
    workspace: optional uint8 device buffer of decode_ws_bytes(A * ncls, K) bytes (allocated here when needed and not given).
    mem_scores (n) f32 + mem_K: the same launch also ranks them (far3d_decode_topk_mem: topk(mem_scores, mem_K) in a second workgroup);
    returns (dict, idx (mem_K) int64) then."""
    lib = _lib.require_device()
    _chk(cls_last, "cls_last", torch.float32, 2)
    _chk(box_last, "box_last", torch.float32, 2)
    A, ncls = cls_last.shape
    code = box_last.shape[1]
    dev = cls_last.device
    res, workspace, need = _decode_outputs(dev, A * ncls, code, int(K), workspace)
    rk, rp = _host_f32(list(post_center_range))
    args = (_ptr(cls_last), _ptr(box_last), A, ncls, code, int(K), rp, _ptr(res["boxes_3d"]), _ptr(res["scores_3d"]), _ptr(res["labels_3d"]),
            _ptr(res["keep"]), _opt_ptr(workspace), need)
    if mem_scores is not None:
        _chk(mem_scores, "mem_scores", torch.float32, 1)
        idx = torch.empty((int(mem_K),), dtype=torch.int64, device=dev)
        _lib.check(lib.far3d_decode_topk_mem(*args, _ptr(mem_scores), mem_scores.numel(), int(mem_K), _ptr(idx), _stream(cls_last)),
                   "far3d_decode_topk_mem")
        return res, idx
    _lib.check(lib.far3d_decode_topk(*args, _stream(cls_last)), "far3d_decode_topk")
    return res


def _decode_streams(who, cls_last, box_last, K, post_center_range, mem_scores, mem_K, workspace, tracked):
    """The checks, outputs and call of decode_topk_mem_streams (tracked False) and decode_topk_tracked (True: + query_idx)."""
    lib = _lib.require_device()
    for t, name in ((cls_last, "cls_last"), (box_last, "box_last")):
        if t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda or not t[0].is_contiguous():
            raise ValueError("%s: %s must be a (B, A, C) float32 device tensor with contiguous streams" % (who, name))
    if mem_scores.dim() != 2 or mem_scores.dtype != torch.float32 or not mem_scores.is_cuda or mem_scores.stride(1) != 1:
        raise ValueError("%s: mem_scores must be a (B, n) float32 device tensor with unit inner stride" % who)
    B, A, ncls = cls_last.shape
    code = box_last.shape[2]
    if box_last.shape[:2] != (B, A) or mem_scores.shape[0] != B:
        raise ValueError("%s: cls_last %s, box_last %s and mem_scores %s disagree on (B, A)" %
                         (who, tuple(cls_last.shape), tuple(box_last.shape), tuple(mem_scores.shape)))
    K, mem_K, dev = int(K), int(mem_K), cls_last.device
    res, workspace, need = _decode_outputs(dev, A * ncls, code, K, workspace, B)
    outs = [res[k] for k in ("boxes_3d", "scores_3d", "labels_3d", "keep")]
    idx = torch.empty((B, mem_K), dtype=torch.int64, device=dev)
    rk, rp = _host_f32(list(post_center_range))
    strides = (ctypes.c_long * 8)(cls_last.stride(0), box_last.stride(0), *[t.stride(0) for t in outs], mem_scores.stride(0), idx.stride(0))
    args = (_ptr(cls_last), _ptr(box_last), B, A, ncls, code, K, rp, *[_ptr(t) for t in outs], _opt_ptr(workspace), need, _ptr(mem_scores),
            mem_scores.shape[1], mem_K, _ptr(idx), ctypes.cast(strides, ctypes.c_void_p))
    if tracked:
        q = res["query_idx"] = torch.empty((B, K), dtype=torch.int32, device=dev)
        _lib.check(lib.far3d_decode_topk_tracked(*args, _ptr(q), q.stride(0), _stream(cls_last)), "far3d_decode_topk_tracked")
    else:
        _lib.check(lib.far3d_decode_topk_mem_streams(*args, _stream(cls_last)), "far3d_decode_topk_mem_streams")
    return res, idx


def decode_topk_mem_streams(cls_last, box_last, K, post_center_range, mem_scores, mem_K, workspace=None):
    """decode_topk(..., mem_scores, mem_K) for B scene streams in ONE launch of 2 * B workgroups (far3d_decode_topk_mem_streams):
    cls_last (B, A, ncls), box_last (B, A, code), mem_scores (B, n) f32, each stream's block contiguous, any stride between the blocks (so
    they may be views into larger buffers).  Returns (dict(boxes_3d (B, K, code-1), scores_3d (B, K), labels_3d (B, K) i64, keep (B, K)
    bool), idx (B, mem_K) i64); [b] of each has the bits of the one-stream call on stream b's operands, whatever B is.  Shapes outside
    the fused launch (A * ncls > 40960 or n > 4096) run the one-stream entry per stream; workspace: optional uint8 device buffer of
    B * decode_ws_bytes(A * ncls, K) bytes for that case (allocated here when needed and not given)."""
    return _decode_streams("decode_topk_mem_streams", cls_last, box_last, K, post_center_range, mem_scores, mem_K, workspace, False)


def decode_topk_tracked(cls_last, box_last, K, post_center_range, mem_scores, mem_K, workspace=None):
    """decode_topk_mem_streams whose dict also holds query_idx (B, K) int32: the query row every decoded box came from (its flat index
    in cls_last // ncls; far3d_decode_topk_tracked).  Same arguments; every other output has the bits of decode_topk_mem_streams."""
    return _decode_streams("decode_topk_tracked", cls_last, box_last, K, post_center_range, mem_scores, mem_K, workspace, True)


TRACK_MAX_K, TRACK_MAX_L, TRACK_MAX_DEC = 1024, 4096, 1024     # csrc/track.hip


def track_update(topk_idx, score, mem_track, next_id, row_start, num_propagated, birth_thr=0.0, query_idx=None):
    """Track ids of one frame for B scene streams in ONE launch (far3d_track_update; the contract is in include/far3d_hip.h and,
    executable, in tests/track_refs.py).  topk_idx (B, K) int64 the memory update's ranked rows, score (B, A) f32 head_finalize's score
    plane (probabilities; -inf in a hole), mem_track (B, L) int64 and next_id (B, 1) int64 the streams' state, UPDATED IN PLACE;
    row_start: the first propagated query row (num_query + adaptive rows); birth_thr: a probability.  Each stream's block contiguous,
    any stride between the blocks.  query_idx (B, Kdec) int32 (decode_topk_tracked) -> returns track_ids (B, Kdec) int64; None -> None."""
    lib = _lib.require_device()
    for t, name, dt in ((topk_idx, "topk_idx", torch.int64), (score, "score", torch.float32), (mem_track, "mem_track", torch.int64),
                        (next_id, "next_id", torch.int64)) + (((query_idx, "query_idx", torch.int32),) if query_idx is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != dt or not t.is_cuda or t.stride(1) != 1:
            raise ValueError("track_update: %s must be a (B, n) %s device tensor with unit inner stride" % (name, dt))
    B, K = topk_idx.shape
    A, L = score.shape[1], mem_track.shape[1]
    if score.shape[0] != B or mem_track.shape[0] != B or tuple(next_id.shape) != (B, 1) or (query_idx is not None and query_idx.shape[0] != B):
        raise ValueError("track_update: topk_idx %s, score %s, mem_track %s, next_id %s%s disagree on B (next_id is (B, 1))" %
                         (tuple(topk_idx.shape), tuple(score.shape), tuple(mem_track.shape), tuple(next_id.shape),
                          ", query_idx %s" % (tuple(query_idx.shape),) if query_idx is not None else ""))
    P = int(num_propagated)
    if P > K:
        raise ValueError("track_update: num_propagated=%d > the %d ranked rows (topk_proposals): a memory slot that was carried over would "
                         "be propagated a second time with the same id" % (P, K))
    thr = float(birth_thr)
    if not 0.0 <= thr <= 1.0:
        raise ValueError("track_update: birth_thr=%r is a probability in [0, 1]" % (birth_thr,))
    Kdec = 0 if query_idx is None else query_idx.shape[1]
    ids = torch.empty((B, Kdec), dtype=torch.int64, device=score.device) if query_idx is not None else None
    strides = (ctypes.c_long * 6)(topk_idx.stride(0), score.stride(0), query_idx.stride(0) if Kdec else 0, mem_track.stride(0),
                                  next_id.stride(0), ids.stride(0) if Kdec else 0)
    _lib.check(lib.far3d_track_update(_ptr(topk_idx), _ptr(score), _ptr(query_idx) if Kdec else None, _ptr(mem_track), _ptr(next_id),
                                      _ptr(ids) if Kdec else None, B, A, K, L, Kdec, int(row_start), P, thr,
                                      ctypes.cast(strides, ctypes.c_void_p), _stream(score)), "far3d_track_update")
    return ids


def track_records(topk_idx, mem_track, mem_hits, query_idx, track_ids, keep, boxes, m_ref, m_ts, num_rows, row_start, num_propagated):
    """Track records of one frame for B scene streams in ONE launch behind track_update (far3d_track_records; the contract is in
    include/far3d_hip.h and, executable, in tests/track_record_refs.py).  topk_idx (B, K) int64 and mem_track (B, L) int64 as
    track_update took / left them, mem_hits (B, L) int32 the streams' counter plane, UPDATED IN PLACE; query_idx (B, Kdec) int32,
    track_ids (B, Kdec) int64, keep (B, Kdec) bool or uint8 and boxes (B, Kdec, >= 3) f32 of the decode; m_ref (B, L, 3) f32 and
    m_ts (B, L) f64 of this frame's memory_prepare; num_rows: the A query rows, row_start: the first propagated one.  Each stream's
    block contiguous, any stride between the blocks.  Returns (track_age (B, Kdec) int32, track_primary (B, Kdec) bool,
    track_velocity (B, Kdec, 3) f32)."""
    lib = _lib.require_device()
    for t, name, dts in ((topk_idx, "topk_idx", (torch.int64,)), (mem_track, "mem_track", (torch.int64,)), (mem_hits, "mem_hits", (torch.int32,)),
                         (query_idx, "query_idx", (torch.int32,)), (track_ids, "track_ids", (torch.int64,)),
                         (keep, "keep", (torch.bool, torch.uint8)), (m_ts, "m_ts", (torch.float64,))):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in dts or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError("track_records: %s must be a (B, n) %s device tensor with unit inner stride" % (name, " or ".join(map(str, dts))))
    for t, name in ((boxes, "boxes"), (m_ref, "m_ref")):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != torch.float32 or not t.is_cuda or (t.numel() > 0 and t.stride(2) != 1):
            raise ValueError("track_records: %s must be a (B, n, c) torch.float32 device tensor with unit inner stride" % name)
    B, K = topk_idx.shape
    L, Kdec = mem_track.shape[1], query_idx.shape[1]
    if any(t.shape[0] != B for t in (mem_track, mem_hits, query_idx, track_ids, keep, boxes, m_ref, m_ts)):
        raise ValueError("track_records: the operands disagree on B=%d (the leading dimension of topk_idx)" % B)
    if tuple(mem_hits.shape) != (B, L) or tuple(m_ts.shape) != (B, L) or tuple(m_ref.shape) != (B, L, 3) or m_ref.stride(1) != 3:
        raise ValueError("track_records: mem_hits %s and m_ts %s must be (B, L=%d) like mem_track, m_ref %s (B, L, 3) with contiguous streams" %
                         (tuple(mem_hits.shape), tuple(m_ts.shape), L, tuple(m_ref.shape)))
    if tuple(track_ids.shape) != (B, Kdec) or tuple(keep.shape) != (B, Kdec) or boxes.shape[1] != Kdec or boxes.shape[2] < 3:
        raise ValueError("track_records: track_ids %s and keep %s must be (B, Kdec=%d) like query_idx, boxes %s (B, Kdec, >= 3)" %
                         (tuple(track_ids.shape), tuple(keep.shape), Kdec, tuple(boxes.shape)))
    P = int(num_propagated)
    if P > K:
        raise ValueError("track_records: num_propagated=%d > the %d ranked rows (topk_proposals): a memory slot that was carried over would "
                         "be propagated a second time with the same id" % (P, K))
    dev = mem_hits.device
    age = torch.empty((B, Kdec), dtype=torch.int32, device=dev)
    primary = torch.empty((B, Kdec), dtype=torch.bool, device=dev)
    velocity = torch.empty((B, Kdec, 3), dtype=torch.float32, device=dev)
    ptr = lambda t: _ptr(t) if Kdec else None
    strides = (ctypes.c_long * 12)(topk_idx.stride(0), mem_track.stride(0), query_idx.stride(0), track_ids.stride(0), keep.stride(0),
                                   boxes.stride(0), m_ref.stride(0), m_ts.stride(0), mem_hits.stride(0), age.stride(0), primary.stride(0),
                                   velocity.stride(0))
    _lib.check(lib.far3d_track_records(_ptr(topk_idx), _ptr(mem_track), ptr(query_idx), ptr(track_ids), ptr(keep), ptr(boxes), _ptr(m_ref),
                                       _ptr(m_ts), _ptr(mem_hits), ptr(age), ptr(primary), ptr(velocity), B, int(num_rows), K, L, Kdec,
                                       int(row_start), P, boxes.stride(1) if Kdec else boxes.shape[2], ctypes.cast(strides, ctypes.c_void_p), _stream(mem_hits)),
               "far3d_track_records")
    return age, primary, velocity


DEDUP_MAX_DEC = 1024                          # csrc/dedup.hip
DEDUP_MODES = ("iou_bev", "centre")           # far3d_box_dedup's mode 0 / 1


def box_dedup(boxes, scores, labels, keep, mode="iou_bev", thr=0.5, class_aware=True, score_thr=0.0, return_overlaps=False):
    """Duplicate suppression of the decoded boxes of B scene streams in ONE launch (far3d_box_dedup; the contract is in
    include/far3d_hip.h and, executable, in tests/dedup_refs.py).  boxes (B, Kdec, >= 7) f32, scores (B, Kdec) f32, labels (B, Kdec)
    int64, keep (B, Kdec) bool or uint8: the decode's outputs in its order; none is written.  Each stream's block contiguous, any
    stride between the blocks.  mode 'iou_bev' (thr an IoU in [0, 1)) or 'centre' (thr a distance in metres > 0).  Returns (dup_keep
    (B, Kdec) bool, dup_of (B, Kdec) int32[, overlaps (B, Kdec, Kdec) f32 with return_overlaps: the kernel's own overlap of every
    judged pair, for inspection])."""
    lib = _lib.require_device()
    for t, name, dts in ((scores, "scores", (torch.float32,)), (labels, "labels", (torch.int64,)), (keep, "keep", (torch.bool, torch.uint8))):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in dts or not t.is_cuda or (t.shape[1] > 1 and t.stride(1) != 1):
            raise ValueError("box_dedup: %s must be a (B, Kdec) %s device tensor with unit inner stride" % (name, " or ".join(map(str, dts))))
    if (not isinstance(boxes, torch.Tensor) or boxes.dim() != 3 or boxes.dtype != torch.float32 or not boxes.is_cuda or boxes.shape[2] < 7
            or (boxes.numel() > 0 and boxes.stride(2) != 1)):
        raise ValueError("box_dedup: boxes must be a (B, Kdec, >= 7) torch.float32 device tensor with unit inner stride")
    B, Kdec = scores.shape
    if B < 1 or any(tuple(t.shape[:2]) != (B, Kdec) for t in (boxes, labels, keep)):
        raise ValueError("box_dedup: boxes %s, labels %s and keep %s must be (B=%d, Kdec=%d) like scores" %
                         (tuple(boxes.shape), tuple(labels.shape), tuple(keep.shape), B, Kdec))
    if Kdec > DEDUP_MAX_DEC:
        raise ValueError("box_dedup: Kdec=%d boxes beyond far3d_box_dedup's %d" % (Kdec, DEDUP_MAX_DEC))
    if mode not in DEDUP_MODES:
        raise ValueError("box_dedup: mode=%r is none of %s" % (mode, ", ".join(DEDUP_MODES)))
    thr, score_thr = float(thr), float(score_thr)
    if mode == "iou_bev" and not 0.0 <= thr < 1.0:
        raise ValueError("box_dedup: thr=%r is an IoU in [0, 1) (mode iou_bev)" % (thr,))
    if mode == "centre" and not 0.0 < thr < float("inf"):
        raise ValueError("box_dedup: thr=%r is a finite distance > 0 in metres (mode centre)" % (thr,))
    if not 0.0 <= score_thr <= 1.0:
        raise ValueError("box_dedup: score_thr=%r is a probability in [0, 1]" % (score_thr,))
    dev = scores.device
    dup_keep = torch.empty((B, Kdec), dtype=torch.bool, device=dev)
    dup_of = torch.empty((B, Kdec), dtype=torch.int32, device=dev)
    over = torch.empty((B, Kdec, Kdec), dtype=torch.float32, device=dev) if return_overlaps else None
    ptr = lambda t: _ptr(t) if Kdec and t is not None else None
    strides = (ctypes.c_long * 7)(boxes.stride(0), scores.stride(0), labels.stride(0), keep.stride(0), dup_keep.stride(0), dup_of.stride(0),
                                  over.stride(0) if over is not None else 0)
    _lib.check(lib.far3d_box_dedup(ptr(boxes), ptr(scores), ptr(labels), ptr(keep), ptr(dup_keep), ptr(dup_of), ptr(over), B, Kdec,
                                   boxes.stride(1) if Kdec else boxes.shape[2], DEDUP_MODES.index(mode), 1 if class_aware else 0, thr,
                                   score_thr, ctypes.cast(strides, ctypes.c_void_p), _stream(scores)), "far3d_box_dedup")
    return (dup_keep, dup_of, over) if return_overlaps else (dup_keep, dup_of)


def camera_prep(lidar2img, intrinsics=None, extrinsics=None):
    """lidar2img / intrinsics / extrinsics (N,4,4) f32 -> (img2lidar (N,4,4) = inverse(lidar2img), c14 (N,14) | None)."""
    lib = _lib.require_device()
    _chk(lidar2img, "lidar2img", torch.float32, 3)
    N, dev = lidar2img.shape[0], lidar2img.device
    i2l = torch.empty((N, 4, 4), dtype=torch.float32, device=dev)
    c14 = None
    if intrinsics is not None:
        _chk(intrinsics, "intrinsics", torch.float32, 3)
        _chk(extrinsics, "extrinsics", torch.float32, 3)
        c14 = torch.empty((N, 14), dtype=torch.float32, device=dev)
    _lib.check(lib.far3d_camera_prep(_ptr(lidar2img), _ptr(intrinsics) if c14 is not None else None,
                                     _ptr(extrinsics) if c14 is not None else None, _ptr(i2l),
                                     _ptr(c14) if c14 is not None else None, N, _stream(lidar2img)), "far3d_camera_prep")
    return i2l, c14


def nan_to_num_(x, bf16_copy=False):
    """In-place torch.nan_to_num on a contiguous f32 tensor; optionally also returns a bf16 copy of the result."""
    lib = _lib.require_device()
    _chk(x, "x", torch.float32)
    xb = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if bf16_copy else None
    _lib.check(lib.far3d_nan_to_num(_ptr(x), _ptr(xb) if xb is not None else None, x.numel(), _stream(x)), "far3d_nan_to_num")
    return xb


def cam_embed_chain(l2i, packed, eps=1e-5):
    """Camera term of the aggregation logits for all decoder layers in one launch.  l2i: lidar2img (N,4,4) f32 (read in
    place) or its (N,12) top-three-rows flattening; packed: dict of stacked, transposed fp32 weights (see
    pack_cam_embed_chain).  Returns (L,N,J) f32."""
    lib = _lib.require_device()
    N = l2i.shape[0]
    l2i = _chk(l2i.reshape(N, -1), "l2i", torch.float32, 2)
    L, E, J = packed["w3t"].shape
    Hd = packed["w0t"].shape[2]
    if E != 256 or l2i.shape[1] not in (12, 16) or tuple(packed["w2t"].shape) != (L, Hd, 256) or Hd > 256:
        raise ValueError("cam_embed_chain: expects 12 -> Hd (<=256) -> 256 -> J weights, got %s" % {k: tuple(v.shape) for k, v in packed.items()})
    out = torch.empty((L, N, J), dtype=torch.float32, device=l2i.device)
    _lib.check(lib.far3d_cam_embed_chain(_ptr(l2i), _ptr(packed["w0t"]), _ptr(packed["b0"]), _ptr(packed["w2t"]),
                                         _ptr(packed["b2"]), _ptr(packed["ln_g"]), _ptr(packed["ln_b"]), _ptr(packed["w3t"]),
                                         _ptr(packed["b3"]), _ptr(out), N, L, J, Hd, eps, l2i.shape[1], _stream(l2i)), "far3d_cam_embed_chain")
    return out


def pack_cam_embed_chain(layers, device):
    """layers: list of (W0 (Hd,12), b0, W2 (256,Hd), b2, ln_g, ln_b, W3 (J,256), b3) per decoder layer (state-dict tensors)."""
    f = lambda ts: torch.stack([t.detach().float() for t in ts]).contiguous().to(device)
    return dict(w0t=f([l[0].t() for l in layers]), b0=f([l[1] for l in layers]), w2t=f([l[2].t() for l in layers]),
                b2=f([l[3] for l in layers]), ln_g=f([l[4] for l in layers]), ln_b=f([l[5] for l in layers]),
                w3t=f([l[6].t() for l in layers]), b3=f([l[7] for l in layers]))

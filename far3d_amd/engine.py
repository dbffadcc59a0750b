"""Far3DEngine: one 7-camera frame through the HIP kernels, batch 1, inference only.

Host-side orchestration only: every heavy step is a C-ABI kernel from libfar3d_hip.so (far3d_amd.ops).  torch is used
for device memory, the stream, and a handful of O(1k)-element index/glue ops (sin/cos position codes, top-k, 4x4 pose
products) that SURVEY.md marks negligible; there is NO CPU path -- constructing the engine without a HIP device raises.

Data layout (HBM): all feature maps are NHWC (channels-last) in the activation dtype (bf16 in 'bf16' mode, fp32 in
'fp32' parity mode); an OSA block's input and its five 3x3 outputs live in ONE (N,H,W,Cin+5*Cs) buffer and every conv
writes its channel slice in place, so torch.cat never runs; FPN outputs are written twice by the same conv epilogue:
raw (for the 2D head) and camera-modulated, token-major (N, S, 256), which IS `feat_flatten` of the reference.
"""
import contextlib
import fnmatch
import functools
import math
import os
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import lib as _lib
from . import ops, weights
from .frame_pipeline import FramePipeline
from .synth import level_starts

PRECISIONS = {
    # act: activations/weights of the backbone / FPN / 2D-head convs; value: the token-major value maps the decoder samples;
    # dec: decoder + FarHead GEMM operands (weights, attention q/k/v, GEMM inputs); the query stream, softmaxes, LayerNorms,
    # projections and every accumulation are fp32 in all modes.
    "bf16": dict(act=torch.bfloat16, value=torch.bfloat16, dec=torch.bfloat16),
    "fp32": dict(act=torch.float32, value=torch.float32, dec=torch.float32),          # parity mode (exact-fp32 MFMA)
    # mixed assignments measured by tests/test_engine_full_gpu.py::test_bf16_error_budget_is_measured_and_bounded
    "bf16_fp32dec": dict(act=torch.bfloat16, value=torch.bfloat16, dec=torch.float32),
    "bf16_fp32val": dict(act=torch.bfloat16, value=torch.float32, dec=torch.float32),
    # fp32 data everywhere; conv products (backbone / FPN / 2D head: 95 % of the FLOPs) as a two-term bf16 split on the bf16 MFMA
    # with fp32 accumulation (far3d_hip.h FAR3D_DT_F32_BF16X3), decoder + FarHead GEMMs on the exact fp32 MFMA: the cheapest
    # assignment that keeps single-frame logits within the north-star 1e-3
    # Activations of the conv stages are PAIR-STORED (ops.pair_from_float: [32 hi | 32 lo] bf16 per 32-channel block, fp32's byte
    # size, 16 significant bits) so that the split products run on the LDS-DMA pipelined kernels (csrc/igemm_pair.hip).
    "bf16x3": dict(act=torch.bfloat16, pair=True, value=torch.float32, dec=torch.float32, mma="bf16x3", dec_mma=None),
    "bf16x3_all": dict(act=torch.bfloat16, pair=True, value=torch.float32, dec=torch.float32, mma="bf16x3", dec_mma="bf16x3"),
    # bf16x3 with the layers that reach the logits ONLY through discrete decisions (2D-head levels 1-3 on the benchmark frames, the
    # depth head's argmax) as single bf16 products: tools/precision_sweep.py (profiles/r3/precision_sweep.log) finds that on frame 0
    # these 18 layers change no logit at all while every layer of the continuous path costs 1e-3..2e-2 and flips proposals.  NOT
    # the default: the zero is a property of that frame (a flipped argmax / peak replaces a whole query), and it saves only 5 %
    # of the conv MFMA work.  Kept as a measured, opt-in assignment.
    "bf16x3_2d1": dict(act=torch.bfloat16, pair=True, value=torch.float32, dec=torch.float32, mma="bf16x3", dec_mma=None,
                       single_bf16=("roi[123].*", "depth.*")),
    # the same arithmetic on plain fp32 activations (split while staging, register-staged kernel): round 2's form, kept for A/B
    "bf16x3_f32act": dict(act=torch.float32, value=torch.float32, dec=torch.float32, mma="bf16x3", dec_mma=None),
}


def default_cfg(**over):
    cfg = dict(
        backbone="V-99-eSE", embed_dims=256, num_classes=26, strides=(8, 16, 32, 64),
        num_cams=7, num_query=644, num_propagated=256, memory_len=1024, topk_proposals=256,
        num_layers=6, num_heads=8, num_groups=8, num_levels=4, num_pts=13, ffn_dim=1024,
        pc_range=[-152.4, -152.4, -5.0, 152.4, 152.4, 5.0], code_size=8, max_num=300,
        depthnet=dict(num_depth_bins=50, depth_min=0.1, depth_max=110.0, stride=8), score_thr=0.1,
        proposal_topk=None,      # None = reference rule (score > thr, data-dependent M); K = static K best per camera
        proposal_cap=512,        # per-camera capacity of the selection in threshold mode
        # Threshold mode with STATIC shapes ("cap + count"): the adaptive queries occupy `proposal_capacity`
        # rows of which the first M (counted on the device) are real; the rest is a masked hole (attention keys, memory top-k,
        # decode, aggregation).  Graph-capturable, pipelinable, shardable -- no host sync; `check_proposal_overflow()` reports, after
        # the fact, a frame whose proposals did not fit.  None = legacy threshold mode (host sync on M, buffers grow).
        proposal_capacity=None,
        # multi-depth 2D proposals (ref farhead.py:754-805): topk = K > 1 adds, for every primary whose best depth bin is at or beyond
        # range_min (metres), K-1 adaptive queries at its next-best bins (K-major after all primaries).  topk 1 (or the reference's -1,
        # plain argmax: the same numbers) keeps the single-depth path.
        multi_depth=dict(topk=1, range_min=30),
        # extra rows reserved for them in the static proposal modes (None = (K-1) x the primary rows: never overflows); a smaller
        # value drops extras past it in reference order, reported by check_proposal_overflow().  The legacy threshold mode sizes
        # them from its selection capacity and ignores this.
        multi_depth_capacity=None,
        # the light 2D head (ref yolox_head.py:197-219, :300-301).  roi_depthwise: the towers are depthwise-separable (use_depthwise=True:
        # depthwise 3x3 + BN + Swish, pointwise 1x1 + BN + Swish per layer).  depth_level: the FPN level the depth branch reads
        # (reg_depth_level p3 / p4 / p5 = 0 / 1 / 2); the proposals take the depth map's stride from strides[depth_level]
        roi_depthwise=False, depth_level=0,
        # track ids (INTEGRATION.md "Track ids"): None = off; dict(birth_thr=p) adds `query_idx` / `track_ids` to the result -- the identity
        # of a detection across the frames of its scene, carried through the streaming memory (far3d_track_update).  birth_thr: the
        # max-class probability from which a ranked query without an identity is given a new one (0.0: every ranked query).
        # records=True (INTEGRATION.md "Track records") adds `track_age` / `track_primary` / `track_velocity` (far3d_track_records)
        track=None,
        # duplicate suppression (INTEGRATION.md "Duplicate suppression"): None = off; dict(mode="iou_bev" | "centre", thr, class_aware,
        # score_thr) adds `dup_keep` / `dup_of` to the result -- a greedy pass over the decoded boxes' rotated BEV footprints
        # (far3d_box_dedup); with track records=True `track_primary` is then the first SURVIVING box of its id
        dedup=None,
    )
    cfg.update(over)
    return cfg


def multi_depth_topk(cfg):
    """K of cfg['multi_depth'] (1: single-depth proposals).  The reference's topk -1 (plain argmax) is the same computation as 1."""
    md = cfg.get("multi_depth") or {}
    k = md.get("topk", 1)
    k = 1 if k is None or int(k) == -1 else int(k)
    if not 1 <= k <= 8:
        raise ValueError("multi_depth topk=%s: supported values are 1 ... 8 (or -1, the same as 1)" % md.get("topk"))
    return k


def track_options(cfg):
    """cfg['track'] checked: None (tracking off) or dict(birth_thr=<probability>[, records=<bool>]: `records` is in the result only where
    the caller gave it).  Tracking needs num_propagated <= topk_proposals: a memory
    slot beyond the frame's top-k is one that was carried over, and propagating it again would put its id on two queries.  A pure
    function of cfg: no device, no library."""
    tr = cfg.get("track")
    if tr is None or tr is False:
        return None
    tr = {} if tr is True else dict(tr)
    unknown = sorted(set(tr) - {"birth_thr", "records"})
    if unknown:
        raise ValueError("track: unknown option(s) %s (known: birth_thr, records)" % ", ".join(unknown))
    if "records" in tr and not isinstance(tr["records"], bool):
        raise ValueError("track records=%r: a bool" % (tr["records"],))
    thr = float(tr.get("birth_thr", 0.0))
    if not 0.0 <= thr <= 1.0:
        raise ValueError("track birth_thr=%r: a probability in [0, 1]" % (tr.get("birth_thr"),))
    if cfg["num_propagated"] > cfg["topk_proposals"]:
        raise ValueError("track: num_propagated=%d > topk_proposals=%d: a memory slot that was carried over would be propagated a second time "
                         "with the same id; tracking needs num_propagated <= topk_proposals" % (cfg["num_propagated"], cfg["topk_proposals"]))
    if cfg["topk_proposals"] > ops.TRACK_MAX_K or cfg["memory_len"] > ops.TRACK_MAX_L or cfg["max_num"] > ops.TRACK_MAX_DEC:
        raise ValueError("track: topk_proposals=%d / memory_len=%d / max_num=%d beyond far3d_track_update's %d / %d / %d" %
                         (cfg["topk_proposals"], cfg["memory_len"], cfg["max_num"], ops.TRACK_MAX_K, ops.TRACK_MAX_L, ops.TRACK_MAX_DEC))
    return dict(birth_thr=thr, **({"records": tr["records"]} if "records" in tr else {}))


DEDUP_DEFAULTS = dict(mode="iou_bev", thr=0.5, class_aware=True, score_thr=0.0)


def dedup_options(cfg):
    """cfg['dedup'] checked: None (duplicate suppression off) or the dict(mode, thr, class_aware, score_thr) of ops.box_dedup with the
    defaults filled in (True: all defaults).  mode 'iou_bev': thr an IoU in [0, 1); mode 'centre': thr a distance in metres, finite and
    > 0.  A pure function of cfg: no device, no library."""
    dd = cfg.get("dedup")
    if dd is None or dd is False:
        return None
    dd = {} if dd is True else dict(dd)
    unknown = sorted(set(dd) - set(DEDUP_DEFAULTS))
    if unknown:
        raise ValueError("dedup: unknown option(s) %s (known: %s)" % (", ".join(unknown), ", ".join(DEDUP_DEFAULTS)))
    dd = dict(DEDUP_DEFAULTS, **dd)
    if dd["mode"] not in ops.DEDUP_MODES:
        raise ValueError("dedup mode=%r: one of %s" % (dd["mode"], ", ".join(ops.DEDUP_MODES)))
    for k in ("thr", "score_thr"):
        if isinstance(dd[k], bool) or not isinstance(dd[k], (int, float)):
            raise ValueError("dedup %s=%r: a number" % (k, dd[k]))
        dd[k] = float(dd[k])
    if dd["mode"] == "iou_bev" and not 0.0 <= dd["thr"] < 1.0:
        raise ValueError("dedup thr=%r: an IoU in [0, 1) (mode iou_bev)" % (dd["thr"],))
    if dd["mode"] == "centre" and not 0.0 < dd["thr"] < float("inf"):
        raise ValueError("dedup thr=%r: a finite distance > 0 in metres (mode centre)" % (dd["thr"],))
    if not isinstance(dd["class_aware"], bool):
        raise ValueError("dedup class_aware=%r: a bool" % (dd["class_aware"],))
    if not 0.0 <= dd["score_thr"] <= 1.0:
        raise ValueError("dedup score_thr=%r: a probability in [0, 1]" % (dd["score_thr"],))
    if cfg["max_num"] > ops.DEDUP_MAX_DEC:
        raise ValueError("dedup: max_num=%d decoded boxes beyond far3d_box_dedup's %d" % (cfg["max_num"], ops.DEDUP_MAX_DEC))
    return dd


def dwsep_layers(cfg, precision):
    """Names of the depthwise-separable layers an engine of this cfg and precision runs as ONE far3d_dwsep_conv_nhwc launch when its
    `fused_dwsep` is set -- every such layer ops.dwsep_supported accepts; the others keep the two-launch form.  Backbone layers of a
    depthwise spec: 'stem2', 'stem3', 's<stage>.b<block>.c<layer>'; light-head tower layers (cfg roi_depthwise): 'roi<level>.cls<i>' /
    'roi<level>.reg<i>' (each name is one layer = a depthwise 3x3 and its pointwise 1x1; the pointwise PackedConv is convs[name + '.pw']).
    A pure function of its arguments: no device, no library."""
    prec = PRECISIONS[precision] if isinstance(precision, str) else precision
    storage = "pair" if prec.get("pair") else ("bf16" if prec["act"] == torch.bfloat16 else "f32")
    # a pointwise layer assigned a single bf16 product inside a pair-stored network (single_bf16) is not what the fused kernel computes
    single = lambda name: storage == "pair" and any(fnmatch.fnmatchcase(name + ".pw", pat) for pat in prec.get("single_bf16", ()))
    ok = lambda name, C, Cout, stride: ops.dwsep_supported(C, Cout, stride, storage) and not single(name)
    names = []
    spec = weights.VOV_SPECS[cfg["backbone"]]
    if spec.get("dw"):
        st = spec["stem"]
        names += [n for n, C, Cout, s in (("stem2", st[0], st[1], 1), ("stem3", st[1], st[2], 2)) if ok(n, C, Cout, s)]
        for si in range(4):
            sc = spec["stage_conv_ch"][si]
            for bi in range(spec["block_per_stage"][si]):
                names += ["s%d.b%d.c%d" % (si + 2, bi, i) for i in range(spec["layer_per_block"]) if ok("s%d.b%d.c%d" % (si + 2, bi, i), sc, sc, 1)]
    if cfg.get("roi_depthwise"):
        E = cfg["embed_dims"]
        for l in range(len(cfg["strides"])):
            names += ["roi%d.%s%d" % (l, t, i) for t in ("cls", "reg") for i in range(2) if ok("roi%d.%s%d" % (l, t, i), E, E, 1)]
    return names


def pos2posemb(pos, num_pos_feats, temperature=10000):
    dim_t = torch.arange(num_pos_feats, dtype=torch.float32, device=pos.device)
    dim_t = temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / num_pos_feats)
    p = (pos * (2 * math.pi))[..., None] / dim_t
    return torch.stack((p[..., 0::2].sin(), p[..., 1::2].cos()), dim=-1).flatten(-2)


def pos2posemb3d(pos):   # reference order (y, x, z): models/utils/positional_encoding.py:13-25
    return torch.cat([pos2posemb(pos[..., 1], 128), pos2posemb(pos[..., 0], 128), pos2posemb(pos[..., 2], 128)], dim=-1)


def nerf_encoding(t, n=6):   # positional_encoding.py:38-80
    out = []
    for k in range(n):
        f = float(2.0 ** k)
        out += [torch.sin(t * f), torch.cos(t * f)]
    return torch.cat(out, dim=-1)


def inverse_sigmoid(x, eps=1e-5):
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


class _Lin:
    """A Linear layer packed for far3d_conv2d_nhwc."""

    def __init__(self, sd, name, dtype, device, bias=True, rows=None, compute=None):
        w = sd[name + ".weight"]
        b = sd[name + ".bias"] if bias else None
        if rows is not None:
            w = w[rows]
            b = b[rows] if b is not None else None
        self.pc = ops.PackedConv(w, b, dtype=dtype, device=device, compute=compute)

    def __call__(self, x, act=None, res=None, out=None, out_dtype=torch.float32):
        return ops.linear(x, self.pc, act=act, res=res, out=out, out_dtype=out_dtype)


# the (rows, C) view the row-local kernels take of a (rows, C) operand (itself) or of B streams' (B, A, C) blocks
_rows = lambda t: t if t.dim() == 2 else t.view(-1, t.shape[-1])


def _with_tile_tables(fn):
    """Entry points that issue (or capture) convolutions run under the engine's own tile tables: ops.use_tile_tables is thread-local and
    restores the previous selection on exit, so engines with different settings -- and stand-alone ops -- can share a process."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        with ops.use_tile_tables(self.bf16_tile_table()):
            return fn(self, *args, **kwargs)
    return wrapped


class Far3DEngine:
    def __init__(self, state_dict, cfg=None, device="cuda:0", precision="bf16", parts=("backbone", "neck", "roi", "head")):
        _lib.require_device()
        self.parts = tuple(parts)
        self.cfg = cfg or default_cfg()
        self.dev = torch.device(device)
        self.prec = dict(PRECISIONS[precision]) if isinstance(precision, str) else dict(precision)
        self.precision = precision if isinstance(precision, str) else "custom"
        self.pair = bool(self.prec.get("pair"))     # conv-stage activations in pair storage
        self.cs = 2 if self.pair else 1             # stored elements per logical channel of those maps
        self.sd = {}
        for k, v in state_dict.items():
            ck = weights.canonical_key(k)
            if ck is not None:
                self.sd[ck] = v.detach().float()
        self.spec = weights.VOV_SPECS[self.cfg["backbone"]]
        if self.pair:
            # pair storage keeps [32 hi | 32 lo] per 32-channel block: a map whose width is no multiple of 32 has no such layout
            odd = [c for c in tuple(self.spec["stem"]) + tuple(self.spec["stage_conv_ch"]) + tuple(self.spec["stage_out_ch"]) if c % 32]
            if odd:
                raise ValueError("backbone %s has a channel width of %d, which is not a multiple of 32: the pair-stored precision %r cannot "
                                 "hold it; the modes that run this spec are %s" %
                                 (self.cfg["backbone"], odd[0], self.precision, ", ".join(k for k, v in PRECISIONS.items() if not v.get("pair"))))
        self.convs = {}           # name -> PackedConv of every conv layer of the per-camera stages
        self._bufs = {}
        self.token_slices = {}      # buffer-set key -> callable (N, S, dtype) -> that set's token buffer (_token_buffer; streams.StreamBatch)
        self.image_slices = {}      # buffer-set key -> callable (shape) -> that set's staged image buffer (_stage_inputs; streams.StreamBatch)
        self._ins = {}              # static input buffers per buffer-set parity (graph replay reads them)
        self._graph = None
        self._graph_outs = None
        self.use_graph = False      # set True to capture the steady-state frame into one hipGraph (needs static shapes: top-K or
                                    # fixed-capacity threshold proposals, static_adaptive_rows() is not None)
        # pipeline (with use_graph): consecutive frames of a stream are software-pipelined -- the per-camera stages of frame
        # i+1 (which do not depend on the streaming memory) run on their own HIP stream while the head of frame i is still in
        # flight (frame_pipeline.FramePipeline: streams, events, staleness of the graphs, the steady frame).  pipeline_sets
        # complete buffer sets (frame index modulo) and two graphs per set (camera stages, head: _capture_frame); the
        # head graphs are ordered on one stream, so the memory updates stay sequential and the results are bit-identical to
        # the unpipelined engine.  Throughput only: the latency of a single frame does not change.  In this mode the outputs of
        # forward_frame are ready on `output_stream()`; a caller that reads them on its own stream calls `wait_outputs()` first
        # (ordering the caller's stream after every head automatically would serialise the next frame's camera stages again).
        self.pipeline = False
        self.cam_priority = -1      # HIP stream priority of the camera-stage streams in pipeline mode (-1 = high: the head's latency-bound
                                    # launches must not hold back the throughput-critical camera stages; 0 = default, A/B in bench.py)
        self._overflow = None       # fixed-capacity threshold mode: device flag of the latest frame (check_proposal_overflow)
        self._ready = None          # event of the latest pipelined head (None: outputs are on the caller's stream)
        self.tile_table = None      # bf16 conv tile table: None = by mode -- "tuning_mi355x_tput.json" (tiles picked under the pipeline's
                                    # 3-stream concurrency, where a tile is judged by the CU-time it occupies) when frames are pipelined,
                                    # "tuning_mi355x.json" (tiles picked for the latency of a launch alone) otherwise
        self.cam_streams = 3        # pipeline mode: streams the camera stages of consecutive frames alternate between (< pipeline_sets)
        self.pipeline_sets = 4      # pipeline mode: buffer sets = frames in flight (4: the camera stages of THREE frames run
                                    # concurrently on three streams under the head of a fourth; 2: round 3's camera || head overlap only).
                                    # Measured (profiles/r4/pipeline_ab.txt, bf16): 2 sets 164.5, 3 sets 193.1, 4 sets / 2 streams 195.8,
                                    # 4 sets / 3 streams 200.5 samples/s -- with the camera streams at high priority; at equal priority the
                                    # head's small launches interleave with the camera stages and the gain is lost (167.0 at 3 sets)
        self._par = 0               # buffer set currently in use (always 0 without pipelining)
        self._fidx = 0
        self._pipe = FramePipeline(self)      # the pipeline's streams and per-buffer-set graphs (falsy until used)
        self.agg_variant = 0        # far3d_aggregate_forward kernel variant (0 = default; tools/ use 3 for A/B timing)
        self.agg_sorted = True      # the aggregation kernel's SORTED mode (round 6): far3d_agg_order also emits the launch slot of every
                                    # row and the reference points in launch order; the producers of the per-layer logits / offsets store in launch
                                    # order, so that no load of the kernel waits for perm[e] (replicated decoder, kernel 8, no split)
        self.agg_split_extra = 0    # > 0: far3d_aggregate_forward variant 9 -- that many sibling workgroups for the queries two cameras see
                                    # (far3d_agg_order marks them; ops.AggSplit holds the partial sums / tickets, one per buffer set)
        self.fused_rows = True      # bf16 decoder: the row-local parts of a decoder layer and the cls / reg branches run as row-resident
                                    # chains (far3d_rowchain_attn_out / _ffn / _branches: 4 launches per layer instead of 11).  Default since
                                    # round 5 (the full GPU suite ran on it); False selects the unfused kernels (A/B: bench.py --no-fused-rows).
                                    # Ignored where the chains do not apply (other decoder dtypes / geometries)
        self.mem = None
        self.prev_scene = None
        self.md_k = multi_depth_topk(self.cfg)
        self.track = track_options(self.cfg)      # None, or dict(birth_thr): mem["track"] / _track_next exist, the result carries track ids
        self.dedup = dedup_options(self.cfg)      # None, or ops.box_dedup's options: the result carries dup_keep / dup_of
        self.roi_dw = bool(self.cfg.get("roi_depthwise", False))
        self.depth_level = int(self.cfg.get("depth_level", 0) or 0)
        if not 0 <= self.depth_level < len(self.cfg["strides"]):
            raise ValueError("depth_level %d is outside the %d levels of strides %s" % (self.depth_level, len(self.cfg["strides"]), self.cfg["strides"]))
        self.depth_stride = self.cfg["strides"][self.depth_level]     # the reference derives it from the map's size (farhead.py:722)
        self.roi_dw_merged = False  # light towers: True = both towers' first depthwise layers as ONE two-set launch (one read of the level map).
                                    # Measured slower than two single-set launches (profiles/light_head/README.md: 142 vs 123 us in bf16, 155
                                    # vs 147 us pair-stored on the 7x80x120x256 map -- two weight sets cost the kernel its second wave per
                                    # SIMD), so the default issues two launches; bit-identical either way
        self.fused_dwsep = False    # True: every depthwise-separable layer far3d_dwsep_conv_nhwc takes (dwsep_layers) is ONE launch -- the depthwise
                                    # result goes to the pointwise MFMA in registers, no scratch map; the others keep the two launches.  Opt-in:
                                    # the pointwise sums accumulate in another order, so outputs differ in the last bits (profiles/dwsep/README.md)
        self._dwsep = frozenset(dwsep_layers(self.cfg, self.prec))
        self.md_min_bin = (ops.depth_range_min_bin(self.cfg["depthnet"], (self.cfg.get("multi_depth") or {}).get("range_min", -1))
                           if self.md_k > 1 else None)
        self._prepare()

    # ------------------------------------------------------------------------------------------ weights
    def _conv_bn(self, prefix, conv="/conv", norm="/norm", eps=1e-5, stride=1, pad=1):
        sd = self.sd
        n = prefix + norm + "."
        w, b = weights.fold_bn(sd[prefix + conv + ".weight"], sd[n + "weight"], sd[n + "bias"], sd[n + "running_mean"],
                               sd[n + "running_var"], eps)
        return w, b, stride, pad

    def _pack(self, w, b, stride=1, pad=0, name=None):
        """name: key in self.convs (the per-layer precision assignment addresses conv layers by it: 'stem2', 's3.b1.c4', 's4.b0.cat',
        'fpn.lat1', 'fpn.out0', 'roi2.tower0', 'roi0.cls1', 'roi0.cls_head', 'depth.c0', ...)."""
        wdt = torch.float32 if self.prec.get("mma") == "bf16x3" else self.prec["act"]
        pc = ops.PackedConv(w, b, stride=stride, pad=pad, dtype=wdt, device=self.dev, compute=self.prec.get("mma"))
        if name is not None:
            self.convs[name] = pc
            if self.pair and any(fnmatch.fnmatchcase(name, pat) for pat in self.prec.get("single_bf16", ())):
                pc.terms = 1            # hi halves only: one bf16 product (tools/precision_sweep.py measures what that costs)
        return pc

    def _prepare(self):
        if "backbone" in self.parts:
            self._prepare_backbone()
        if "neck" in self.parts:
            self._prepare_neck()
        if "roi" in self.parts or ("neck" in self.parts and "head" in self.parts):
            self._prepare_roi()
        if "head" in self.parts:
            self._prepare_head()
        torch.cuda.synchronize(self.dev)

    def _prepare_backbone(self):
        sd, dev = self.sd, self.dev
        f32 = lambda t: t.to(dev).float().contiguous()
        # ---- backbone (a2)
        bb = {}
        w, b, _, _ = self._conv_bn("img_backbone.stem.stem_1")
        bb["stem1"] = self._pack(F.pad(w.permute(0, 2, 3, 1).reshape(w.shape[0], 27), (0, 5)), b, name="stem1")   # 1x1 over the 32-ch im2col
        dw = bool(self.spec.get("dw"))

        def layer3(prefix, name, stride=1):
            """A 3x3 layer: conv + BN + ReLU as one PackedConv, or -- depthwise specs (vovnet.py:100-121) -- the [9][C] depthwise weights
            plus the pointwise 1x1 with `pw_norm` folded in (named '<name>.pw'; nothing nonlinear sits between the two)."""
            if not dw:
                return self._pack(*self._conv_bn(prefix, stride=stride), name=name)
            return dict(dw=ops.pack_dw3x3(sd[prefix + "/dw_conv3x3.weight"], dev), stride=stride, name=name,
                        pw=self._pack(*self._conv_bn(prefix, conv="/pw_conv1x1", norm="/pw_norm", pad=0), name=name + ".pw"))

        bb["stem2"] = layer3("img_backbone.stem.stem_2", "stem2")
        bb["stem3"] = layer3("img_backbone.stem.stem_3", "stem3", stride=2)
        stages = []
        in_ch = self.spec["stem"][2]
        for si in range(4):
            k = si + 2
            sc = self.spec["stage_conv_ch"][si]
            blocks = []
            for bi in range(self.spec["block_per_stage"][si]):
                name = "OSA%d_%d" % (k, bi + 1)
                p = "img_backbone.stage%d.%s" % (k, name)
                convs = [layer3("%s.layers.%d.%s_%d" % (p, i, name, i), "s%d.b%d.c%d" % (k, bi, i))
                         for i in range(self.spec["layer_per_block"])]
                cw, cb, _, _ = self._conv_bn("%s.concat.%s_concat" % (p, name), pad=0)
                blk = dict(convs=convs, concat=self._pack(cw, cb, name="s%d.b%d.cat" % (k, bi)), fcw=f32(sd[p + ".ese.fc.weight"].flatten(1)),
                           fcb=f32(sd[p + ".ese.fc.bias"]))
                if dw and in_ch != sc:      # 1x1 + BN + ReLU in front of layer 0 only; the concat keeps the unreduced input (vovnet.py:200-204,220-230)
                    blk["red"] = self._pack(*self._conv_bn("%s.conv_reduction.%s_reduction_0" % (p, name), pad=0), name="s%d.b%d.red" % (k, bi))
                blocks.append(blk)
                in_ch = self.spec["stage_out_ch"][si]
            stages.append(blocks)
        bb["stages"] = stages
        self.bb = bb

    def _prepare_neck(self):
        sd, cfg, dev = self.sd, self.cfg, self.dev
        # ---- FPN (a3)
        nl = len(self.spec["stage_out_ch"]) - 1
        self.fpn_lat = [self._pack(sd["img_neck.lateral_convs.%d.conv.weight" % i], sd["img_neck.lateral_convs.%d.conv.bias" % i], name="fpn.lat%d" % i)
                        for i in range(nl)]
        self.fpn_out = [self._pack(sd["img_neck.fpn_convs.%d.conv.weight" % i], sd["img_neck.fpn_convs.%d.conv.bias" % i],
                                   stride=2 if i == nl else 1, pad=1, name="fpn.out%d" % i) for i in range(nl + 1)]

    def _prepare_roi(self):
        sd, cfg, dev = self.sd, self.cfg, self.dev
        f32 = lambda t: t.to(dev).float().contiguous()
        # ---- 2D head + depth (a4)
        r = "img_roi_head."
        self.roi = []
        for l in range(len(cfg["strides"])):
            lv = {}
            if self.roi_dw:
                # depthwise-separable towers: per layer the folded depthwise (9,C) weights + bias (ops.dwconv3x3_act_nhwc, Swish) and the
                # pointwise 1x1 with its BN folded ('roi<l>.<tower><i>.pw', Swish in the GEMM's epilogue)
                for t in ("cls", "reg"):
                    lv[t] = []
                    for i in range(2):
                        p = r + "multi_level_%s_convs.%d.%d" % (t, l, i)
                        w, b, _, _ = self._conv_bn(p, conv=".depthwise_conv.conv", norm=".depthwise_conv.bn", eps=1e-3)
                        pw = self._pack(*self._conv_bn(p, conv=".pointwise_conv.conv", norm=".pointwise_conv.bn", eps=1e-3, pad=0),
                                        name="roi%d.%s%d.pw" % (l, t, i))
                        lv[t].append(dict(dw=ops.pack_dw3x3_sets([w], [b], dev), w=w, b=b, pw=pw, name="roi%d.%s%d" % (l, t, i)))
                # both towers' first depthwise layers read the same map: packed as one two-set operand (cls channels first) for roi_dw_merged
                lv["dw0"] = ops.pack_dw3x3_sets([lv["cls"][0]["w"], lv["reg"][0]["w"]], [lv["cls"][0]["b"], lv["reg"][0]["b"]], dev)
            else:
                for t in ("cls", "reg"):
                    lv[t] = [self._pack(*self._conv_bn(r + "multi_level_%s_convs.%d.%d" % (t, l, i), conv=".conv", norm=".bn", eps=1e-3),
                                        name="roi%d.%s1" % (l, t) if i == 1 else None) for i in range(2)]
                # the two towers' first convs read the same map: one 256 -> 512 conv (cls channels first), half the launches and
                # twice the workgroups on the small levels
                wc, bc, _, _ = self._conv_bn(r + "multi_level_cls_convs.%d.0" % l, conv=".conv", norm=".bn", eps=1e-3)
                wr, br, _, _ = self._conv_bn(r + "multi_level_reg_convs.%d.0" % l, conv=".conv", norm=".bn", eps=1e-3)
                lv["tower0"] = self._pack(torch.cat([wc, wr]), torch.cat([bc, br]), 1, 1, name="roi%d.tower0" % l)
            lv["cls_head"] = self._pack(sd[r + "multi_level_conv_cls.%d.weight" % l], sd[r + "multi_level_conv_cls.%d.bias" % l], name="roi%d.cls_head" % l)
            lv["reg_head"] = self._pack(torch.cat([sd[r + "multi_level_conv_reg.%d.weight" % l], sd[r + "multi_level_conv_obj.%d.weight" % l]]),
                                        torch.cat([sd[r + "multi_level_conv_reg.%d.bias" % l], sd[r + "multi_level_conv_obj.%d.bias" % l]]),
                                        name="roi%d.reg_head" % l)
            if r + "multi_level_conv_centers2d.%d.weight" % l in sd:     # only the stand-alone module forward returns it (loss input)
                lv["ctr_head"] = self._pack(sd[r + "multi_level_conv_centers2d.%d.weight" % l], sd[r + "multi_level_conv_centers2d.%d.bias" % l])
            self.roi.append(lv)
        self.depth = dict(
            convs=[self._pack(sd[r + "depthnet.depth_head.%d.0.weight" % i], sd[r + "depthnet.depth_head.%d.0.bias" % i], pad=1, name="depth.c%d" % i)
                   for i in range(2)],
            gn=[(f32(sd[r + "depthnet.depth_head.%d.1.weight" % i]), f32(sd[r + "depthnet.depth_head.%d.1.bias" % i])) for i in range(2)],
            cls=self._pack(sd[r + "depthnet.depth_classifier.weight"], sd[r + "depthnet.depth_classifier.bias"], name="depth.cls"))

    def _prepare_head(self):
        sd, cfg, dev = self.sd, self.cfg, self.dev
        f32 = lambda t: t.to(dev).float().contiguous()
        # ---- FarHead (a6, a10)
        h = "pts_bbox_head."
        dw = self.prec["dec"]
        E = cfg["embed_dims"]
        pk = lambda w, b=None: ops.PackedConv(w, b, dtype=dw, device=dev, compute=self.prec.get("dec_mma"))
        L = lambda name, **kw: _Lin(sd, h + name, dw, dev, compute=self.prec.get("dec_mma"), **kw)
        W = lambda name: sd[h + name + ".weight"]
        B = lambda name: sd[h + name + ".bias"]
        self.pc_range = f32(sd[h + "pc_range"])
        self.sa = dict(reduce=L("spatial_alignment.reduce.0"), gamma=L("spatial_alignment.gamma"), beta=L("spatial_alignment.beta"))
        self.qe = (L("query_embedding.0"), L("query_embedding.2"))
        self.ce = (L("context_embed.0"), L("context_embed.2"))
        self.te = L("time_embedding.0")
        self.te_ln = (f32(sd[h + "time_embedding.1.weight"]), f32(sd[h + "time_embedding.1.bias"]))
        # MLN(180) of temporal_alignment (farhead.py:292-300): the two modules read the same code, so their `reduce` layers
        # run as ONE GEMM (Cout 2E) and each module's gamma|beta as one GEMM over its half of the hidden rows
        names = ("ego_pose_pe", "ego_pose_memory")
        self.mln_reduce = pk(torch.cat([W(n + ".reduce.0") for n in names]), torch.cat([B(n + ".reduce.0") for n in names]))
        self.mln_gb = {n: pk(torch.cat([W(n + ".gamma"), W(n + ".beta")]), torch.cat([B(n + ".gamma"), B(n + ".beta")])) for n in names}
        self.cls_b = (L("cls_branches.0.0"), L("cls_branches.0.3"), L("cls_branches.0.6"))
        self.cls_ln = [(f32(sd[h + "cls_branches.0.%d.weight" % j]), f32(sd[h + "cls_branches.0.%d.bias" % j])) for j in (1, 4)]
        self.reg_b = (L("reg_branches.0.0"), L("reg_branches.0.2"), L("reg_branches.0.4"))
        cls_pcs, reg_pcs = tuple(l.pc for l in self.cls_b), tuple(l.pc for l in self.reg_b)
        self.branch_rc = ops.RowChainBranches(cls_pcs, self.cls_ln, reg_pcs) if ops.RowChainBranches.supported(cls_pcs, reg_pcs, E, dw) else None
        self.ref_fixed = f32(sd[h + "reference_points.weight"])
        self.pseudo_ref = f32(sd[h + "pseudo_reference_points.weight"]) if cfg["num_propagated"] > 0 else None
        # ---- decoder layers (a7, a8).  Merged GEMMs over the [x+pos | x] operand (K = 2E, block weights):
        #   qkv:  [q | k | v] = [x+pos | x] @ [[Wq;Wk] 0; 0 Wv]^T          (mmcv MHA: pos on q/k only, detr3d_transformer.py:378-396)
        #   wl:   [weights_fc(x+pos) | learnable_fc(x)]                     (detr3d_transformer.py:525,538; weights_fc bias is in Vc)
        #   memkv (all layers at once): the memory rows' k / v of every layer, written under the layers' q/k/v column blocks
        z = lambda r, c: torch.zeros(r, c)
        self.layers = []
        memkv_w, memkv_b = [], []
        nJ = cfg["num_groups"] * cfg["num_levels"] * cfg["num_pts"]
        nO = cfg["num_pts"] * 3
        for i in range(cfg["num_layers"]):
            lp = h + "transformer.decoder.layers.%d." % i
            a, c = lp + "attentions.0.attn.", lp + "attentions.1."
            ipw, ipb = sd[a + "in_proj_weight"], sd[a + "in_proj_bias"]
            wq, wk, wv = ipw[:E], ipw[E:2 * E], ipw[2 * E:]
            qkv_w = torch.cat([torch.cat([wq, z(E, E)], 1), torch.cat([wk, z(E, E)], 1), torch.cat([z(E, E), wv], 1)])
            memkv_w.append(torch.cat([z(E, 2 * E), torch.cat([wk, z(E, E)], 1), torch.cat([z(E, E), wv], 1)]))
            memkv_b.append(torch.cat([torch.zeros(E), ipb[E:]]))
            wl_w = torch.cat([torch.cat([sd[c + "weights_fc.weight"], z(nJ, E)], 1), torch.cat([z(nO, E), sd[c + "learnable_fc.weight"]], 1)])
            wl_b = torch.cat([torch.zeros(nJ), sd[c + "learnable_fc.bias"]])
            ly = dict(
                qkv=pk(qkv_w, ipb), out=pk(sd[a + "out_proj.weight"], sd[a + "out_proj.bias"]), wl=pk(wl_w, wl_b),
                oproj=pk(sd[c + "output_proj.weight"], sd[c + "output_proj.bias"]),
                ffn1=pk(sd[lp + "ffns.0.layers.0.0.weight"], sd[lp + "ffns.0.layers.0.0.bias"]),
                ffn2=pk(sd[lp + "ffns.0.layers.1.weight"], sd[lp + "ffns.0.layers.1.bias"]),
                norms=[(f32(sd[lp + "norms.%d.weight" % j]), f32(sd[lp + "norms.%d.bias" % j])) for j in range(3)])
            # packed operands of the row-resident chains (csrc/rowchain.hip; used when fused_rows is set)
            ly["rc"] = ops.RowChainLayer(ly) if ops.RowChainLayer.supported(ly, E, dw) else None
            self.layers.append(ly)
        self.memkv = pk(torch.cat(memkv_w), torch.cat(memkv_b))
        cl = []
        for i in range(cfg["num_layers"]):
            c = h + "transformer.decoder.layers.%d.attentions.1." % i
            cl.append((sd[c + "cam_embed.0.weight"], sd[c + "cam_embed.0.bias"], sd[c + "cam_embed.2.weight"], sd[c + "cam_embed.2.bias"],
                       sd[c + "cam_embed.4.weight"], sd[c + "cam_embed.4.bias"], sd[c + "weights_fc.weight"], sd[c + "weights_fc.bias"]))
        self.cam_chain = ops.pack_cam_embed_chain(cl, dev)
        # ---- frame-invariant pieces of temporal_alignment (farhead.py:284-303): the current frame's ego motion is the
        # identity, so its MLN(180) codes are constants, and the learned queries never change.
        mk_dim_t = lambda n: (10000 ** (2 * torch.div(torch.arange(n, dtype=torch.float32, device=dev), 2, rounding_mode="floor") / n)).contiguous()
        self.dim_t128, self.dim_t256 = mk_dim_t(128), mk_dim_t(256)
        eye = torch.eye(4, device=dev)[:3, :].flatten()
        rec = nerf_encoding(torch.cat([torch.zeros(3, device=dev), eye])[None])              # (1,180)
        hh = ops.linear(rec, self.mln_reduce, act="relu")                                    # (1,2E): [pe | memory] hidden
        self.rec_gb = {n: ops.linear(hh[:, j * E:(j + 1) * E], self.mln_gb[n]) for j, n in enumerate(names)}   # (1,2E) gamma|beta
        self.time0 = ops.layernorm(self.te(pos2posemb(torch.zeros(1, device=dev), 256)), *self.te_ln)   # (1,256)
        qp = self._query_pos(self.ref_fixed)
        g, b = self._gb(self.rec_gb["ego_pose_pe"])
        self.qpos_fixed = ops.row_affine_ln(qp, g, b, add=self.time0)
        g, b = self._gb(self.rec_gb["ego_pose_memory"])
        self.tgt_fixed = ops.row_affine_ln(torch.zeros_like(qp), g, b)
        self._mem_alloc()

    def _gb(self, gb):
        E = self.cfg["embed_dims"]
        return gb[:, :E], gb[:, E:]

    def _query_pos(self, ref):
        return self.qe[1](self.qe[0](ops.posemb3d(ref, self.dim_t128), act="relu"))

    def static_adaptive_rows(self, ncam=None):
        """Rows the adaptive queries occupy when that number is static (top-K mode: ncam * K; fixed-capacity threshold mode:
        proposal_capacity; each + the multi-depth extra rows), else None (legacy threshold mode: data-dependent, needs a host sync)."""
        K = self.cfg["proposal_topk"]
        if K is not None:
            P = (self.cfg["num_cams"] if ncam is None else ncam) * K
        else:
            P = self.cfg.get("proposal_capacity")
        return None if P is None else P + self.md_extra_rows(P)

    def md_extra_rows(self, primary_rows):
        """Rows reserved for the multi-depth extra queries after `primary_rows` primary rows (0 when topk = 1)."""
        if self.md_k <= 1:
            return 0
        X = self.cfg.get("multi_depth_capacity")
        return (self.md_k - 1) * primary_rows if X is None else int(X)

    def bf16_tile_table(self):
        """The tile table the bf16 convolutions of this engine's launches consult (see tile_table)."""
        if self.tile_table is not None:
            return self.tile_table
        return "tuning_mi355x_tput.json" if (self.pipeline and self.use_graph) else "tuning_mi355x.json"

    def check_proposal_overflow(self):
        """Fixed-capacity threshold mode: raise if the latest frame had more proposals than rows (or a camera filled its selection
        capacity).  Synchronises; call it when the outputs are read, not between pipelined frames."""
        f = getattr(self, "_overflow", None)
        if f is not None and int(f.item()) != 0:
            raise _lib.Far3dHipError("proposal capacity exceeded: more than proposal_capacity=%s proposals in the frame, or a camera reached "
                                     "proposal_cap=%s; raise them (the reference keeps every peak above the threshold)" %
                                     (self.cfg.get("proposal_capacity"), self.cfg["proposal_cap"]))

    def act_from_nchw(self, x):
        """(N,C,H,W) float map -> the engine's NHWC activation storage (bf16 / f32 / pair-stored bf16)."""
        y = x.permute(0, 2, 3, 1).contiguous()
        return ops.pair_from_float(y) if self.pair else y.to(self.prec["act"])

    def act_to_nchw(self, y):
        """An NHWC activation map of this engine (or an f32 head output) -> (N,C,H,W) f32."""
        y = ops.pair_to_float(y) if (self.pair and y.dtype == torch.bfloat16) else y.float()
        return y.permute(0, 3, 1, 2).contiguous()

    def _buf(self, key, shape, dtype):
        key = (self._par,) + tuple(key)
        b = self._bufs.get(key)
        if b is None or tuple(b.shape) != tuple(shape) or b.dtype != dtype:
            b = torch.empty(shape, dtype=dtype, device=self.dev)
            self._bufs[key] = b
        return b

    def _token_buffer(self, N, S, dtype):
        """The frame's token-major value maps (N, S, 256).  A buffer set with an entry in token_slices (a scene stream of
        streams.StreamBatch) takes what that callable hands out -- slice b of the batch's ONE (B, N, S, 256) allocation, so that
        decoder_streams reads every stream's maps without a copy; every other set owns its buffer."""
        owner = self.token_slices.get(self._par)
        return owner(N, S, dtype) if owner is not None else self._buf(("tokens",), (N, S, 256), dtype)

    # ------------------------------------------------------------------------------------------ a2: backbone
    def _layer3(self, src, layer, out=None):
        """One 3x3 layer of the backbone on the NHWC view `src` (+ BN + ReLU) into `out` (None: a fresh map).  A plain spec's layer is one
        convolution; a depthwise spec's (a dict, _prepare_backbone) is far3d_dwconv3x3_nhwc into a scratch map of the layer's width and
        the pointwise 1x1 GEMM from there, whose epilogue applies the folded BN and the ReLU."""
        if not isinstance(layer, dict):
            return ops.conv2d_nhwc(src, layer, out=out, act="relu")
        N, H, W, Cs = src.shape
        s = layer["stride"]
        if self.fused_dwsep and layer["name"] in self._dwsep:     # one launch, no scratch map (nothing nonlinear between the halves)
            return ops.dwsep_conv_nhwc(src, layer["dw"], layer["pw"], s, act2="relu", out=out, pair=self.pair)
        shape = (N, (H - 1) // s + 1, (W - 1) // s + 1, Cs)
        # one scratch map per shape and buffer set: the launches of a stream are ordered, and a captured graph keeps its address
        tmp = ops.dwconv3x3_nhwc(src, layer["dw"], s, out=self._buf(("dw_tmp",) + shape, shape, self.prec["act"]), pair=self.pair)
        return ops.conv2d_nhwc(tmp, layer["pw"], out=out, act="relu")

    def backbone_geometry(self, H, W):
        """The backbone's maps for an H x W image, per image: dict(stem=(h, w, stored channels) of the stem1 / stem2 outputs, stages=[dict(
        h, w, cat / cat_next / out = stored channels of the stage's first concat buffer, of its later blocks' (0: one block) and of its
        block outputs)]).  backbone() takes its buffer shapes from here, and camera_image_span() its bound: one source for both."""
        spec, cs = self.spec, self.cs
        Lb = spec["layer_per_block"]
        h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1                  # stem1: 3x3 / stride 2 / pad 1
        geo = dict(stem=(h, w, max(spec["stem"][:2]) * cs), stages=[])
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1                  # stem3: 3x3 / stride 2 / pad 1
        in_ch = spec["stem"][2]
        for si, nblk in enumerate(spec["block_per_stage"]):
            sc, oc = spec["stage_conv_ch"][si], spec["stage_out_ch"][si]
            if si > 0:                                             # MaxPool2d(3, 2, ceil_mode=True)
                hp, wp = h, w
                h, w = -(-(hp - 3) // 2) + 1, -(-(wp - 3) // 2) + 1
                if (h - 1) * 2 >= hp:
                    h -= 1
                if (w - 1) * 2 >= wp:
                    w -= 1
            geo["stages"].append(dict(h=h, w=w, cat=(in_ch + Lb * sc) * cs, cat_next=(oc + Lb * sc) * cs if nblk > 1 else 0,
                                      out=oc * cs))
            in_ch = oc
        return geo

    def camera_image_span(self, H, W):
        """Bytes of the largest map ONE H x W image has anywhere in camera_stage: the image, the stem's im2col rows and outputs, the
        backbone's concat buffers and block outputs (backbone_geometry), and the 2D head's widest map (both towers of a level, at the
        first FPN level; everything behind the backbone is smaller than the backbone's own maps at that level).  The kernels bound the
        span of ALL images of a launch (streams.stream_chunks)."""
        es = 4 if self.prec["act"] == torch.float32 else 2
        geo = self.backbone_geometry(H, W)
        sh, sw, sch = geo["stem"]
        spans = [3 * H * W * 4, sh * sw * 32 * self.cs * es, sh * sw * sch * es]
        spans += [g["h"] * g["w"] * max(g["cat"], g["cat_next"], g["out"]) * es for g in geo["stages"]]
        if len(geo["stages"]) > 1:
            g = geo["stages"][1]
            spans.append(g["h"] * g["w"] * 512 * self.cs * 4)
        return max(spans)

    @_with_tile_tables
    def backbone(self, img, keep_stage2=True):
        """img (N,3,H,W) f32 NCHW on device -> [stage2..stage5] dense NHWC maps (pair mode: 2C stored bf16 channels each).
        keep_stage2=False (the detector's own frames): nothing but the stage-3 pooling reads the stage-2 map, so its last eSE writes
        the pooled map only and the first entry of the result is None (the stand-alone VoVNet module returns all four maps)."""
        act, spec, cs, pair = self.prec["act"], self.spec, self.cs, self.pair
        N = img.shape[0]
        Lb = spec["layer_per_block"]
        # eSE workspace (per-workgroup partial channel sums + gates): stream-ordered, so one buffer serves every block
        scratch = self._buf(("ese_scratch",), (ops.ese_scratch_floats(N, max(spec["stage_out_ch"])),), torch.float32)
        # fixed-point channel sums the concat convolutions accumulate in their epilogue (the eSE pooling without a second pass over the
        # map); zero at rest: every eSE call consumes and re-zeroes them, and an eager call re-zeroes them in case a frame was aborted
        # (plain bf16 AND pair-stored maps.  Round 3 switched the pair mode back to its fp32 pooling pass after its full-size streaming
        # check lost one query; the cause was a near-tie of the rig's 3x3 peak test, not the pooling -- tests/test_engine_full_gpu.py --
        # and the pair mode takes the sums again).  One tensor per BUFFER SET (camera stages of two frames run
        # concurrently in pipeline mode) and per image count (any batch of images may be passed); created zeroed, and never
        # replaced once a graph has captured its address.
        esums = None
        if act == torch.bfloat16:
            ek = (self._par, "esums", N)
            esums = self._bufs.get(ek)
            if esums is None:
                esums = self._bufs[ek] = torch.zeros((N, max(spec["stage_out_ch"])), dtype=torch.int64, device=self.dev)
        if esums is not None and not torch.cuda.is_current_stream_capturing():
            esums.zero_()
        # eSE with the stage-end pooling fused into its apply pass (far3d_ese_fused_nhwc): the gates' workspace
        egate = self._buf(("ese_gate", N), (N * max(spec["stage_out_ch"]),), torch.float32) if esums is not None else None
        if act == torch.bfloat16 and not pair:
            x = ops.stem_conv(img, self.bb["stem1"], act="relu")      # im2col folded into the convolution (bit-identical, csrc/stem.hip)
        else:
            x = ops.stem_im2col(img, act, pair=pair)
            x = ops.conv2d_nhwc(x, self.bb["stem1"], act="relu")
        x = self._layer3(x, self.bb["stem2"])
        geo = self.backbone_geometry(img.shape[2], img.shape[3])
        assert tuple(x.shape[1:]) == (geo["stem"][0], geo["stem"][1], spec["stem"][1] * cs), (tuple(x.shape), geo["stem"])
        in_ch = spec["stem"][2]
        outs = []
        stage_in = None   # dense input of the stage (stem3 output is written straight into the first concat buffer)
        pooled_by_ese = False      # the previous stage's last eSE launch already wrote this stage's pooled input
        next_cat = None            # ... into this tensor (the next stage's first concat buffer)
        for si, blocks in enumerate(self.bb["stages"]):
            sc, oc = spec["stage_conv_ch"][si], spec["stage_out_ch"][si]
            g = geo["stages"][si]
            H, W = g["h"], g["w"]
            # this stage's first concat buffer: the SAME tensor the previous stage's last eSE pass pooled into (fetched once there and
            # handed over: a second _buf lookup with a drifted shape would silently allocate another buffer)
            want_shape = (N, H, W, g["cat"])
            if next_cat is not None:
                assert tuple(next_cat.shape) == want_shape, (tuple(next_cat.shape), want_shape)
                cat, next_cat = next_cat, None
            else:
                cat = self._buf(("cat", si, 0), want_shape, act)
            if si == 0:
                self._layer3(x, self.bb["stem3"], out=cat[..., :in_ch * cs])
            elif not pooled_by_ese:
                assert stage_in is not None, "the previous stage's map was skipped (keep_stage2=False) but its eSE pass did not pool it"
                ops.maxpool3x3s2_nhwc(stage_in, out=cat[..., :in_ch * cs], pair=pair)
            pooled_by_ese = False
            cur_in = in_ch
            for bi, blk in enumerate(blocks):
                last = bi == len(blocks) - 1
                src = cat[..., :cur_in * cs]
                if "red" in blk:       # depthwise block whose input width differs from the stage width: layer 0 reads the reduced map
                    src = ops.conv2d_nhwc(src, blk["red"], out=self._buf(("red", si), (N, H, W, sc * cs), act), act="relu")
                for i, pc in enumerate(blk["convs"]):
                    dst = cat[..., (cur_in + i * sc) * cs: (cur_in + (i + 1) * sc) * cs]
                    self._layer3(src, pc, out=dst)
                    src = dst
                fuse = esums is not None and ops.conv_can_fuse_sums(cat, blk["concat"])
                xt = ops.conv2d_nhwc(cat, blk["concat"], out=self._buf(("xt", si), (N, H, W, g["out"]), act), act="relu",
                                     sums=esums if fuse else None)
                idn = cat[..., :cur_in * cs] if bi > 0 else None
                will_fuse = fuse and ops.ese_fused_ok(xt, pair) and (idn is None or ops.ese_fused_ok(idn, pair))
                pooled = None
                if will_fuse and last and si + 1 < len(self.bb["stages"]):   # the next stage's input slice: MaxPool2d(3, 2, ceil) of this output
                    Hn, Wn = ops.maxpool_out_hw(H, W)
                    gn = geo["stages"][si + 1]
                    assert (Hn, Wn) == (gn["h"], gn["w"]), ((Hn, Wn), gn)
                    next_cat = self._buf(("cat", si + 1, 0), (N, Hn, Wn, gn["cat"]), act)
                    pooled = next_cat[..., :oc * cs]
                skip_out = pooled is not None and si == 0 and not keep_stage2     # nothing but the pooling reads the stage-2 map
                if last:
                    out = None if skip_out else self._buf(("stage", si), (N, H, W, oc * cs), act)
                    nxt = None
                else:
                    nxt = self._buf(("cat", si, 1 + (bi % 2)), (N, H, W, g["cat_next"]), act)
                    out = nxt[..., :oc * cs]
                if will_fuse and (out is None or ops.ese_fused_ok(out, pair)):
                    ops.ese_fused_nhwc(xt, blk["fcw"], blk["fcb"], esums, egate, identity=idn, out=out, pooled=pooled, pair=pair)
                    pooled_by_ese = pooled is not None
                else:
                    if out is None:
                        out = self._buf(("stage", si), (N, H, W, oc * cs), act)
                    ops.ese_nhwc(xt, blk["fcw"], blk["fcb"], identity=idn, out=out, scratch=scratch, pair=pair, sums=esums if fuse else None)
                if not last:
                    cat, cur_in = nxt, oc
            stage_in = out
            outs.append(stage_in)
            in_ch = oc
        return outs

    # ------------------------------------------------------------------------------------------ a3 + MLN: FPN
    @_with_tile_tables
    def fpn(self, feats, mln_scale, mln_shift):
        """Returns (raw levels [NHWC act; pair mode: 512 stored channels], feat_flatten (N,S,256) value dtype, level_hw, level_start)."""
        act, val = self.prec["act"], self.prec["value"]
        ins = feats[1:]
        N = ins[0].shape[0]
        n = len(ins)
        hw = [(f.shape[1], f.shape[2]) for f in ins]
        hw.append(self.fpn_out[n].out_hw(*hw[-1]))
        starts, S = level_starts(hw)
        tokens = self._token_buffer(N, S, val)
        lat = [None] * n
        for i in range(n - 1, -1, -1):   # top-down: laterals[i-1] += nearest_upsample(laterals[i])
            lat[i] = ops.conv2d_nhwc(ins[i], self.fpn_lat[i], out=self._buf(("lat", i), (N, hw[i][0], hw[i][1], 256 * self.cs), act),
                                     res=lat[i + 1] if i + 1 < n else None)
        raw = [None] * (n + 1)
        y2s = [tokens[:, starts[i]: starts[i] + hw[i][0] * hw[i][1]].view(N, hw[i][0], hw[i][1], 256) for i in range(n + 1)]
        outs = [self._buf(("fpn", i), (N, hw[i][0], hw[i][1], 256 * self.cs), act) for i in range(n + 1)]
        # the stride-1 outputs are independent of one another: one grouped launch where it was measured to win (ops.group_tile)
        gt = ops.group_tile("fpn.out", N * hw[0][0] * hw[0][1]) if self.pair else 0
        if gt and all(ops.conv_groupable(lat[i], self.fpn_out[i]) for i in range(n)):
            raw[:n] = ops.conv2d_nhwc_grouped([dict(x=lat[i], pc=self.fpn_out[i], out=outs[i], y2=y2s[i], y2_scale=mln_scale, y2_shift=mln_shift)
                                               for i in range(n)], gt)
        else:
            for i in range(n):
                raw[i] = ops.conv2d_nhwc(lat[i], self.fpn_out[i], out=outs[i], y2=y2s[i], y2_scale=mln_scale, y2_shift=mln_shift)
        raw[n] = ops.conv2d_nhwc(raw[n - 1], self.fpn_out[n], out=outs[n], y2=y2s[n], y2_scale=mln_scale, y2_shift=mln_shift)
        return raw, tokens, hw, starts

    # ------------------------------------------------------------------------------------------ a4: 2D head + depth
    @_with_tile_tables
    def roi_head(self, raw, centers2d=None):
        """YOLOX towers + depth head on the raw FPN maps.  centers2d: optional list that receives the (N,h,w,2) centre-offset maps
        (a loss input the inference path never reads; the stand-alone YOLOXHeadCustom.forward returns them like the reference)."""
        d = raw[0]
        npix = d.shape[0] * d.shape[1] * d.shape[2]
        gt0 = ops.group_tile("roi.tower0", npix) if self.pair else 0
        gt1 = ops.group_tile("roi.cls1reg1", npix) if self.pair else 0
        light = self.roi_dw or self.depth_level != 0      # the grouped launches cover the dense towers with the depth branch on p3 only
        if gt0 and gt1 and centers2d is None and not light and self._roi_groupable(raw):
            return self._roi_head_grouped(raw, gt0, gt1)
        cls, reg = [], []
        for l, x in enumerate(raw):
            lv = self.roi[l]
            if self.roi_dw:
                cf, rf = self._light_towers(x, lv)
            else:
                t0 = ops.conv2d_nhwc(x, lv["tower0"], act="swish")                 # (N,h,w,512): cls | reg
                half = t0.shape[-1] // 2
                cf = ops.conv2d_nhwc(t0[..., :half], lv["cls"][1], act="swish")
                rf = ops.conv2d_nhwc(t0[..., half:], lv["reg"][1], act="swish")
            cls.append(ops.conv2d_nhwc(cf, lv["cls_head"], out_dtype=torch.float32))
            reg.append(ops.conv2d_nhwc(rf, lv["reg_head"], out_dtype=torch.float32))
            if centers2d is not None:
                centers2d.append(ops.conv2d_nhwc(rf, lv["ctr_head"], out_dtype=torch.float32))
        d = raw[self.depth_level]
        gscr = self._buf(("gn_scratch",), (ops.ese_scratch_floats(d.shape[0], d.shape[-1] // self.cs),), torch.float32)
        for i in range(2):
            d = ops.conv2d_nhwc(d, self.depth["convs"][i])
            d = ops.groupnorm_nhwc(d, *self.depth["gn"][i], groups=32, relu=True, scratch=gscr, pair=self.pair)
        return cls, reg, ops.conv2d_nhwc(d, self.depth["cls"], out_dtype=torch.float32)

    def _light_towers(self, x, lv):
        """The depthwise-separable cls and reg towers of one level (yolox_head.py:197-219) on the NHWC map x -> (cls feature, reg feature).
        Per tower and layer: far3d_dwconv3x3_act_nhwc (folded BN bias + Swish), then the pointwise 1x1 + BN + Swish -- or, with fused_dwsep,
        both as one far3d_dwsep_conv_nhwc launch for the layers it takes.  Layer 0 of both towers reads x: with roi_dw_merged the depthwise
        halves of the unfused ones are one two-set launch (cls channels first), otherwise single-set launches."""
        fused = lambda ly: self.fused_dwsep and ly["name"] in self._dwsep
        sep = lambda f, ly: ops.dwsep_conv_nhwc(f, ly["dw"][0], ly["pw"], 1, bias1=ly["dw"][1], act1="swish", act2="swish", pair=self.pair)
        if self.roi_dw_merged and not (fused(lv["cls"][0]) or fused(lv["reg"][0])):
            t0 = ops.dwconv3x3_act_nhwc(x, lv["dw0"][0], 1, bias=lv["dw0"][1], act="swish", pair=self.pair)      # (N,h,w,2C): cls | reg
            half = t0.shape[-1] // 2
            t0 = (t0[..., :half], t0[..., half:])
        else:
            t0 = tuple(None if fused(lv[t][0]) else
                       ops.dwconv3x3_act_nhwc(x, lv[t][0]["dw"][0], 1, bias=lv[t][0]["dw"][1], act="swish", pair=self.pair) for t in ("cls", "reg"))
        out = []
        for t, h in zip(("cls", "reg"), t0):
            f = sep(x, lv[t][0]) if h is None else ops.conv2d_nhwc(h, lv[t][0]["pw"], act="swish")
            if fused(lv[t][1]):
                out.append(sep(f, lv[t][1]))
                continue
            f = ops.dwconv3x3_act_nhwc(f, lv[t][1]["dw"][0], 1, bias=lv[t][1]["dw"][1], act="swish", pair=self.pair)
            out.append(ops.conv2d_nhwc(f, lv[t][1]["pw"], act="swish"))
        return out

    def _roi_groupable(self, raw):
        if 2 * len(raw) + 1 > ops.GROUP_MAX:
            return False
        lv0 = [(x, self.roi[l]["tower0"]) for l, x in enumerate(raw)]
        c1 = [lv["cls"][1] for lv in self.roi] + [lv["reg"][1] for lv in self.roi] + list(self.depth["convs"])
        return (all(ops.conv_groupable(x, pc) for x, pc in lv0) and ops.conv_groupable(raw[0], self.depth["convs"][0]) and
                all(pc.terms == 3 and pc.KH == 3 and pc.stride == 1 and pc.pad == 1 and pc.Cin == 256 and pc.Cout % 32 == 0 for pc in c1) and
                all(pc.Cout == 512 for _, pc in lv0))

    def _roi_head_grouped(self, raw, gt0, gt1):
        """roi_head as two grouped launches of the persistent 3x3 kernel -- {tower0 of every level, depth.c0}, then {cls1 and reg1 of every
        level, depth.c1} -- with the depth head's GroupNorm between them and the 1x1 heads after: the same layers on the same inputs, every
        output bit-identical to the per-layer launches (ops.conv2d_nhwc_grouped)."""
        L = len(raw)
        outs = ops.conv2d_nhwc_grouped([dict(x=x, pc=self.roi[l]["tower0"], act="swish") for l, x in enumerate(raw)] +
                                       [dict(x=raw[0], pc=self.depth["convs"][0])], gt0)
        t0s, d = outs[:L], outs[L]
        gscr = self._buf(("gn_scratch",), (ops.ese_scratch_floats(d.shape[0], d.shape[-1] // self.cs),), torch.float32)
        d = ops.groupnorm_nhwc(d, *self.depth["gn"][0], groups=32, relu=True, scratch=gscr, pair=self.pair)
        half = [t.shape[-1] // 2 for t in t0s]
        outs = ops.conv2d_nhwc_grouped([dict(x=t[..., :h], pc=self.roi[l]["cls"][1], act="swish") for l, (t, h) in enumerate(zip(t0s, half))] +
                                       [dict(x=t[..., h:], pc=self.roi[l]["reg"][1], act="swish") for l, (t, h) in enumerate(zip(t0s, half))] +
                                       [dict(x=d, pc=self.depth["convs"][1])], gt1)
        d = ops.groupnorm_nhwc(outs[2 * L], *self.depth["gn"][1], groups=32, relu=True, scratch=gscr, pair=self.pair)
        cls = [ops.conv2d_nhwc(outs[l], self.roi[l]["cls_head"], out_dtype=torch.float32) for l in range(L)]
        reg = [ops.conv2d_nhwc(outs[L + l], self.roi[l]["reg_head"], out_dtype=torch.float32) for l in range(L)]
        return cls, reg, ops.conv2d_nhwc(d, self.depth["cls"], out_dtype=torch.float32)

    # ------------------------------------------------------------------------------------------ memory (a6/a11)
    def _mem_alloc(self):
        """Persistent streaming-memory buffers, allocated ONCE: a captured hipGraph reads / writes them in place, so a scene
        change must never replace them (reset_memory zeroes them in place).  The reference grows the queue to 1280 and
        truncates to memory_len at the next frame (farhead.py:467-471,501-505); truncating right after the update is the same."""
        cfg, dev = self.cfg, self.dev
        Lm, E = cfg["memory_len"], cfg["embed_dims"]
        self.mem = dict(emb=torch.zeros(1, Lm, E, device=dev), ref=torch.zeros(1, Lm, 3, device=dev),
                        ts=torch.zeros(1, Lm, 1, device=dev, dtype=torch.float64), pose=torch.zeros(1, Lm, 4, 4, device=dev),
                        velo=torch.zeros(1, Lm, 2, device=dev))
        if self.track is not None:
            # one id per memory slot (0: none), zeroed with the memory; the counter of the next id lives beside it: a scene change
            # does not reset it, so an id is never used twice (reset_tracks)
            self.mem["track"] = torch.zeros(1, Lm, dtype=torch.int64, device=dev)
            self._track_next = torch.ones(1, 1, dtype=torch.int64, device=dev)
            if self.track.get("records"):
                # frames the id of each slot has been ranked (> 0 exactly where track != 0): shifted and zeroed with the ids
                self.mem["track_hits"] = torch.zeros(1, Lm, dtype=torch.int32, device=dev)
        self._mem_valid = False

    def reset_memory(self):
        """Forget the streaming memory (detectors/far3d.py:252-257): the next frame is treated as the first of a scene."""
        self._mem_valid = False
        self.prev_scene = None

    def reset_tracks(self):
        """Start the track ids at 1 again and forget the streaming memory (ids of the old numbering must not survive in it).  A scene
        change alone never resets the counter."""
        if self.track is None:
            raise ValueError("reset_tracks: tracking is off (cfg track=None)")
        self._track_next.fill_(1)
        self.reset_memory()

    # ------------------------------------------------------------------------------------------ a7/a8: decoder
    def _row_chains(self, packed):
        """Do the row-resident chains (csrc/rowchain.hip) run in place of the unfused kernels?  fused_rows is set, the decoder dtype is
        bf16 and every operand set of `packed` (the layers' RowChainLayer, the heads' RowChainBranches) could be built."""
        return self.fused_rows and self.prec["dec"] == torch.bfloat16 and all(p is not None for p in packed)

    def _agg_sorted_gate(self, A, split, tokens):
        """Does the decoder store the aggregation's operands in launch order (the default kernel's sorted mode)?  Only where the
        library takes them (ops.aggregate_sorted_applies): any other configuration runs unsorted on the kernel variant 0 picks.
        tokens: the (N, S, C) value maps."""
        cfg = self.cfg
        N, S, C = tokens.shape
        return bool(self.agg_sorted and split is None and self.agg_variant in (0, 8) and A > 0 and
                    ops.aggregate_sorted_applies(N, cfg["num_pts"], cfg["num_levels"], S, C, tokens.element_size()))

    def _decoder_buffers(self, buf, lead, Kt, A, N, **operands):
        """The persistent buffers of one decoder pass, with `operands`, as one object: lead () for one stream (_decoder_setup), (B,)
        for B streams (decoder_streams); buf(name, shape, dtype) hands a buffer out under the caller's keys (the layer outputs' key
        is not of that scheme: they come in with the operands).  Kt: A + memory keys."""
        cfg, rows = self.cfg, lead + (A,)
        E, nL, at = cfg["embed_dims"], len(self.layers), self.prec["dec"]
        nJ, nO = cfg["num_groups"] * cfg["num_levels"] * cfg["num_pts"], cfg["num_pts"] * 3
        return SimpleNamespace(
            nJ=nJ, nO=nO, QKV=buf("qkv", lead + (Kt, nL * 3 * E), at),  # per layer a [q | k | v] column block
            XW=buf("xw", rows + (2 * E,), at),                           # [x1+pos | x1] operand of the logit / offset GEMM
            UL=buf("ul", rows + (-(-(nJ + nO) // 64) * 64,), torch.float32),     # [U (nJ) | key-point offsets (nO)] per query
            x1=buf("x1", rows + (E,), torch.float32), x2=buf("x2", rows + (E,), torch.float32),
            x2b=buf("x2b", rows + (E,), at) if at == torch.bfloat16 else None,      # the bf16 copy the bf16 FFN reads
            agg_out=buf("agg_out", rows + (E,), at), att_out=buf("att_out", rows + (E,), at),
            tab=buf("agg_tab", (nL,) + lead + (2 + N, nJ), torch.float32), **operands)

    def _decoder_prologue(self, X2, lidar2img, QKV, A):
        """One stream's query-independent launches: the memory rows' K / V of all layers (one GEMM, X2[A:] -> QKV[A:]), the camera
        term of the aggregation logits of all layers (one launch) -> (layers, N, nJ), bias included."""
        if X2.shape[0] > A:
            ops.linear(X2[A:], self.memkv, out=QKV[A:], out_dtype=self.prec["dec"])
        return ops.cam_embed_chain(lidar2img, self.cam_chain)

    def _in_projection(self, li, X2, QKV, A):
        """Layer li's q / k / v of one stream's query rows: X2[:A] ([x+pos | x]) -> the layer's column block of QKV[:A]."""
        E3 = 3 * self.cfg["embed_dims"]
        ops.linear(X2[:A], self.layers[li]["qkv"], out=QKV[:A, li * E3:(li + 1) * E3], out_dtype=self.prec["dec"])

    def _layer_after_attention(self, linear, ly, att, x, qpos, x1, xw, ul, out_rows=None):
        """The unfused layer from the attention core to the aggregation, ONE copy for _decoder_layer (linear = ops.linear, (rows, .)
        views) and decoder_streams (ops.linear_streams, (B, A, .) blocks): out-projection + residual x, LN0 -> x1 and
        [x1 + pos | x1] -> xw (at the rows out_rows in the sorted mode), the logit / offset GEMM xw -> ul."""
        E = x1.shape[-1]
        y = linear(att, ly["out"], res=x)
        ops.layernorm(_rows(y), *ly["norms"][0], out=_rows(x1), add=_rows(qpos), y2=_rows(xw)[:, :E], yb=_rows(xw)[:, E:], out_rows=out_rows)
        linear(xw, ly["wl"], out=ul)

    def _layer_after_aggregation(self, linear, ly, agg, x1, qpos, x2, x2b, dst, nxt):
        """The unfused layer behind the aggregation, as _layer_after_attention: output projection + residual x1, LN1 -> x2 (x2b: its
        bf16 copy, None in the fp32 decoder), FFN x + W2 relu(W1 x), hidden 1024 (SURVEY.md finding 4), LN2 -> dst and, with nxt, the
        next in-projection's operand [dst + pos | dst] -> nxt."""
        E = x1.shape[-1]
        y = linear(agg, ly["oproj"], res=x1)
        ops.layernorm(_rows(y), *ly["norms"][1], out=_rows(x2), yb=None if x2b is None else _rows(x2b))
        hdn = linear(x2 if x2b is None else x2b, ly["ffn1"], act="relu", out_dtype=self.prec["dec"])
        y = linear(hdn, ly["ffn2"], res=x2)
        feed = {} if nxt is None else dict(add=_rows(qpos), y2=_rows(nxt)[:, :E], yb=_rows(nxt)[:, E:])
        ops.layernorm(_rows(y), *ly["norms"][2], out=_rows(dst), **feed)

    def _decoder_setup(self, X2, x0, qpos, tokens, ref, hw, starts, lidar2img, pad_hw, A, hole, rows=None):
        """The decoder's per-frame working set (buffers, static operands, the aggregation's order and tables) as one object, and the
        query-independent launches.  rows None: the replicated run over all A queries; rows (a0, a1): a rank's share of the
        query-sharded run, which orders only its own rows and runs neither the sorted mode nor sibling workgroups."""
        cfg = self.cfg
        ws = self._decoder_buffers(lambda name, shape, dt: self._buf((name,), shape, dt), (), X2.shape[0], A, lidar2img.shape[0],
                                   X2=X2, x0=x0, qpos=qpos, tokens=tokens, ref=ref, hw=hw, starts=starts, lidar2img=lidar2img, pad_hw=pad_hw,
                                   hole=hole, chains=self._row_chains(ly["rc"] for ly in self.layers), perm=None, inv=None, qbase=None, split=None,
                                   outs=self._buf(("outs_dec",), (len(self.layers), A, cfg["embed_dims"]), torch.float32))
        ws.vc_all = self._decoder_prologue(X2, lidar2img, ws.QKV, A)
        if rows is not None:
            # a rank's share: the order of its own rows (absolute row indices; nothing to order for a rank without rows) and the tables
            if rows[1] > rows[0]:
                ws.perm = ops.aggregation_order(ref, lidar2img, cfg["pc_range"], pad_hw, out=self._buf(("perm_qs",), (rows[1] - rows[0],), torch.int32),
                                                hole=hole, rows=rows)
            ws.tabs = ops.agg_tables(ws.vc_all, out=ws.tab)
            return ws
        # per-frame preparations of the aggregation in ONE launch: reference points are fixed across the layers -> one camera-sorted
        # workgroup order (scheduling only); the camera factors of the factored softmax for all layers (include/far3d_hip.h)
        sp = None
        if self.agg_split_extra > 0 and self.agg_variant in (0, 9):
            sk = (self._par, "agg_split", A, int(self.agg_split_extra))
            sp = self._bufs.get(sk)
            if sp is None:
                sp = self._bufs[sk] = ops.AggSplit(A, self.agg_split_extra, self.dev)
        self.last_agg_split = ws.split = sp
        srt = None
        if self._agg_sorted_gate(A, sp, tokens):
            srt = (self._buf(("agg_inv",), (A,), torch.int32), self._buf(("agg_qbase",), (A, 4), torch.float32))
            ws.inv, ws.qbase = srt
        res = ops.aggregation_order(ref, lidar2img, cfg["pc_range"], pad_hw, out=self._buf(("perm",), (A + (sp.extra if sp else 0),), torch.int32),
                                    hole=hole, Vc=ws.vc_all, tables_out=ws.tab, split=sp, sorted_operands=srt)
        ws.perm, ws.tabs = res[0], res[1]
        return ws

    def _decoder_layer(self, ws, li, a0, a1, dst, feed_next):
        """The row-local part of layer `li` for the query rows [a0, a1) against the keys / values of ALL rows (ws.QKV holds the
        layer's q / k / v): attention, out-projection, aggregation, FFN, the three LayerNorms; the post-LN2 rows go to dst
        ((a1 - a0, E) f32).  Every kernel here works row by row and gives a row the same bits whatever rows the launch covers, which
        is what makes ONE body valid for the whole range (the replicated run) and for any rank's share of it.
        Two forms.  Unfused (_layer_after_attention, _layer_after_aggregation -- the halves decoder_streams runs too): 10 launches
        (11 with the in-projection the caller issues).  Row chains (ws.chains, csrc/rowchain.hip): the attention core,
        far3d_rowchain_attn_out (out-projection + residual + LN0 + the aggregation's logit / offset linears), the aggregation kernel,
        far3d_rowchain_ffn (output projection + residual + LN1 + FFN + LN2) -- 4 launches; same operands and arithmetic as the
        unfused form (bf16 operands, fp32 accumulation and LayerNorms), a different K order inside the GEMMs.
        feed_next (the replicated run): the last launch also writes the next layer's operand for these rows -- unfused [x + pos | x]
        into ws.X2, with the chains the NEXT layer's q / k / v into ws.QKV (nothing after the last layer).  Without it (a rank's
        share, dst = its send buffer) nothing but dst is written: the next operand is built from the exchanged rows."""
        cfg, ly = self.cfg, self.layers[li]
        E, nJ, nO = cfg["embed_dims"], ws.nJ, ws.nO
        c0, r = li * 3 * E, slice(a0, a1)
        x = (ws.x0 if li == 0 else ws.outs[li - 1])[r]
        qpos, x1, att = ws.qpos[r], ws.x1[r], ws.att_out[r]
        # self-attention: q = x+pos, k = cat[x,mem]+cat[pos,mempos], v = cat[x,mem] (detr3d_transformer.py:378-396)
        ops.attention_forward(ws.QKV[r, c0:c0 + E], ws.QKV[:, c0 + E:c0 + 2 * E], ws.QKV[:, c0 + 2 * E:c0 + 3 * E],
                              num_heads=cfg["num_heads"], out=att, hole=ws.hole)
        # (sorted mode, ws.inv: the rows of the logits / offsets go to the aggregation kernel's launch slots -- the chain stores them
        # there, the unfused form stores the GEMM-operand rows [x1 + pos | x1] there so that the GEMM writes in launch order)
        if ws.chains:
            ops.rowchain_attn_out(att, x, qpos, ly["rc"], x1, ws.UL[r], ul_rows=ws.inv)
        else:
            self._layer_after_attention(ops.linear, ly, att, x, qpos, x1, ws.XW[r], ws.UL[r, :nJ + nO], out_rows=ws.inv)
        # cross-attention: fused perspective-aware aggregation (detr3d_transformer.py:522-569) of the rows ws.perm lists, on the
        # full-size buffers
        U, off = ws.UL[:, :nJ], ws.UL[:, nJ:nJ + nO]
        ops.aggregate_forward(ws.tokens, ws.ref, off, ws.lidar2img, U, ws.vc_all[li], ws.hw, ws.starts, cfg["pc_range"], ws.pad_hw,
                              num_groups=cfg["num_groups"], perm=ws.perm, out=ws.agg_out, variant=self.agg_variant, tables=ws.tabs[li],
                              split=ws.split, qbase=ws.qbase)
        self.last_agg = (ws.tokens, ws.ref, off, ws.lidar2img, U, ws.vc_all[li], ws.hw, ws.starts, ws.pad_hw, ws.perm, ws.tabs[li], ws.qbase)
        agg = ws.agg_out[r]
        if ws.chains:
            feed = feed_next and li + 1 < len(self.layers)
            ops.rowchain_ffn(agg, x1, qpos, ly["rc"], dst, nxt=self.layers[li + 1]["rc"] if feed else None,
                             qkv=ws.QKV[r, c0 + 3 * E:c0 + 6 * E] if feed else None)
        else:
            self._layer_after_aggregation(ops.linear, ly, agg, x1, qpos, ws.x2[r], None if ws.x2b is None else ws.x2b[r], dst,
                                          ws.X2[r] if feed_next else None)

    def decoder(self, X2, x0, qpos, tokens, ref, hw, starts, lidar2img, pad_hw, A, hole=None, qshard=None):
        """X2 (A+Km, 2E) `dec` dtype: rows [:A] = [tgt+pos | tgt] of the queries, rows [A:] = [mem+mempos | mem] of the memory
        keys; x0 (A,E) f32 = tgt; qpos (A,E) f32.  Returns the stacked post-LN outputs (layers, A, E) f32.
        qshard: query-sharded execution over several ranks (far3d_amd.dist.QueryShard), see decoder_query_sharded."""
        if qshard is not None:
            return self.decoder_query_sharded(X2, x0, qpos, tokens, ref, hw, starts, lidar2img, pad_hw, A, hole, qshard)
        ws = self._decoder_setup(X2, x0, qpos, tokens, ref, hw, starts, lidar2img, pad_hw, A, hole)
        for li in range(len(self.layers)):
            # the in-projection is a GEMM launch of its own for layer 0 only with the row chains (the FFN chain of layer li - 1 wrote
            # this layer's q / k / v), for every layer without them
            if li == 0 or not ws.chains:
                self._in_projection(li, X2, ws.QKV, A)
            self._decoder_layer(ws, li, 0, A, ws.outs[li], True)
        return ws.outs

    def decoder_query_sharded(self, X2, x0, qpos, tokens, ref, hw, starts, lidar2img, pad_hw, A, hole, qs):
        """The decoder with its QUERIES sharded over the ranks of a camera-sharded frame (SURVEY.md 8(e) "alternatives"): every rank
        holds all value maps (they were gathered for the replicated head anyway) and runs rows [a0, a1) of the A queries through
        each layer -- attention queries, out-projection, aggregation, FFN, the three LayerNorms -- against the K / V of ALL rows; one
        small all-gather per layer (A x E fp32 = 1.5 MB at the benchmark size) hands every rank the full layer output, from which
        the next layer's keys / values are recomputed locally (one GEMM over all rows: cheaper than gathering K and V).
        Row-wise kernels give every row the same bits whatever subset of rows a launch covers, so the result is BIT-IDENTICAL to
        the replicated decoder (tests/test_dist_gpu.py, tests/test_decoder_gpu.py): both run _decoder_layer, here on a share of
        the rows.  Per layer the sharded part is ~11 of 12 launches; what stays replicated is
        the qkv GEMM, the memory K/V GEMM, the camera term and the cls / reg heads."""
        E, at = self.cfg["embed_dims"], self.prec["dec"]
        per = qs.rows_per_rank(A)
        a0, a1 = min(qs.rank * per, A), min((qs.rank + 1) * per, A)
        nr = a1 - a0
        ws = self._decoder_setup(X2, x0, qpos, tokens, ref, hw, starts, lidar2img, pad_hw, A, hole, rows=(a0, a1))
        gsrc = self._buf(("qs_src",), (per, E), torch.float32)           # this rank's rows of a layer output (zero padded)
        gdst = self._buf(("qs_dst",), (qs.world * per, E), torch.float32)
        if nr < per:
            gsrc[nr:].zero_()
        for li, ly in enumerate(self.layers):
            c0 = li * 3 * E
            # the in-projection over ALL rows (every rank needs every K / V).  With the row chains, layers > 0 take it as
            # far3d_rowchain_qkv on the exchanged rows: bit-identical to the tail of the FFN chain that writes it in the replicated run
            if ws.chains and li > 0:
                ops.rowchain_qkv(ws.outs[li - 1], qpos, ly["rc"], ws.QKV[:A, c0:c0 + 3 * E])
            else:
                self._in_projection(li, X2, ws.QKV, A)
            if nr > 0:
                self._decoder_layer(ws, li, a0, a1, gsrc[:nr], False)
            qs.gather(gsrc, gdst)                                       # the layer's ONE exchange (never captured into a graph)
            ws.outs[li].copy_(gdst[:A])    # rank r owns rows [r * per, (r + 1) * per): the blocks are already in row order, padding last
            # next layer's operand [x + pos | x] for ALL rows (what the fused LayerNorm epilogue writes in the replicated decoder;
            # the row chains build it inside far3d_rowchain_qkv)
            if not ws.chains:
                ops.add_cast(ws.outs[li], qpos, at, out_sum=X2[:A, :E], out_a=X2[:A, E:])
        return ws.outs

    def decoder_streams(self, X2, x0, qpos, tokens, ref, hw, starts, lidar2img, pad_hw, A, holes=None):
        """`decoder` for B scene streams in ONE pass: X2, x0, qpos, tokens, ref, lidar2img are lists of B per-stream operands as
        `decoder` takes them (same shapes in every stream); hw, starts, pad_hw, A are shared.  Returns (B, layers, A, E) f32 whose
        [b] is, bit for bit, decoder(..., hole=holes[b]) on stream b's operands in its unfused form (fused_rows off), hole rows
        included -- in every decoder dtype and whatever B is.
        holes: None, or a list of B per-stream (count int32 device scalar, start, end) tuples (_head_prepare's hs.hole: the
        fixed-capacity threshold mode and the multi-depth extra rows), all None or none, start / end the same in every stream.  The
        B counts are gathered into ONE (B,) buffer of the pass -- B small device copies, no sync -- which every layer's
        far3d_attention_streams and far3d_aggregate_batched_holes launch reads.
        Per layer ONE far3d_attention_streams launch, ONE far3d_aggregate_batched launch, and the halves of _decoder_layer's unfused
        form (_layer_after_attention, _layer_after_aggregation) once over all B * A rows of _decoder_buffers' (B, A, .) set.  Their
        GEMMs go through ops.linear_streams, which takes its tile from ONE stream's row count, so a tile table keyed on rows cannot
        choose another K order; every other kernel gives a row the same bits whatever rows the launch covers (_decoder_layer).  Per
        stream stay _decoder_prologue and layer 0's in-projection (they read the caller's X2[b]) and small copies of x0 / qpos / ref /
        lidar2img.  The value maps are read in place when tokens[b] are the slices of one (B, N, S, 256) allocation (_token_buffer)."""
        cfg = self.cfg
        B, E, nL, at = len(X2), cfg["embed_dims"], len(self.layers), self.prec["dec"]
        Kt, N = X2[0].shape[0], lidar2img[0].shape[0]
        if any(tuple(x.shape) != (Kt, 2 * E) for x in X2) or any(tuple(t.shape) != tuple(tokens[0].shape) for t in tokens) or \
                not (len(x0) == len(qpos) == len(tokens) == len(ref) == len(lidar2img) == B):
            raise ValueError("decoder_streams: every stream needs operands of the same shapes (one X2, x0, qpos, tokens, ref, lidar2img each)")
        buf = lambda name, shape, dt: self._buf(("ds_" + name, B), shape, dt)
        hole = None
        if holes is not None and any(h is not None for h in holes):
            if len(holes) != B or any(h is None for h in holes):
                raise ValueError("decoder_streams: holes is one (count, start, end) per stream (%d), all of them None or none" % B)
            if any((int(h[1]), int(h[2])) != (int(holes[0][1]), int(holes[0][2])) for h in holes):
                raise ValueError("decoder_streams: every stream's hole must have the same start and end, got %s" %
                                 [(int(h[1]), int(h[2])) for h in holes])
            cnt = buf("hole_cnt", (B,), torch.int32)
            for b, h in enumerate(holes):
                cnt[b:b + 1].copy_(h[0].view(-1)[:1])
            hole = (cnt, int(holes[0][1]), int(holes[0][2]))
        ws = self._decoder_buffers(buf, (B,), Kt, A, N, outs=buf("outs", (nL, B, A, E), torch.float32))
        nJ, nO, QKV, UL, outs = ws.nJ, ws.nO, ws.QKV, ws.UL, ws.outs
        XN = buf("xn", (B, A, 2 * E), at)                          # [x+pos | x] operand of the next layer's in-projection
        X0, QP = buf("x0", (B, A, E), torch.float32), buf("qpos", (B, A, E), torch.float32)
        REF, L2I = buf("ref", (B, A, 3), torch.float32), buf("l2i", (B, N, 4, 4), torch.float32)
        VC = buf("vc", (nL, B, N, nJ), torch.float32)              # camera term of the aggregation logits, bias included
        t0 = tokens[0]
        if all(t.is_contiguous() and t.dtype == t0.dtype and t.data_ptr() == t0.data_ptr() + b * t0.numel() * t0.element_size()
               for b, t in enumerate(tokens)):
            tok = t0.as_strided((B,) + tuple(t0.shape), (t0.numel(),) + tuple(t0.stride()))   # slices of one allocation: read in place
        else:
            tok = torch.stack(list(tokens))
        for b in range(B):
            X0[b].copy_(x0[b]); QP[b].copy_(qpos[b]); REF[b].copy_(ref[b]); L2I[b].copy_(lidar2img[b])
            VC[:, b].copy_(self._decoder_prologue(X2[b], lidar2img[b], QKV[b], A))
            self._in_projection(0, X2[b], QKV[b], A)
        # the same table pass as far3d_agg_order's (agg_tables_body): the bits of the one-stream decoder's tables, where its kernel reads them
        tabs = ops.aggregate_kernel8_applies(N, cfg["num_pts"], cfg["num_levels"], tok.shape[2], tok.shape[3], tok.element_size())
        if tabs:
            ops.agg_tables(VC.view(nL * B, N, nJ), out=ws.tab.view(nL * B, 2 + N, nJ))
        for li, ly in enumerate(self.layers):
            c0 = li * 3 * E
            if li > 0:
                ops.linear_streams(XN, ly["qkv"], out=QKV[:, :A, c0:c0 + 3 * E])
            ops.attention_streams(QKV[:, :A, c0:c0 + E], QKV[:, :, c0 + E:c0 + 2 * E], QKV[:, :, c0 + 2 * E:c0 + 3 * E],
                                  num_heads=cfg["num_heads"], out=ws.att_out, hole=hole)
            self._layer_after_attention(ops.linear_streams, ly, ws.att_out, X0 if li == 0 else outs[li - 1], QP, ws.x1, ws.XW, UL[:, :, :nJ + nO])
            ops.aggregate_batched(tok, REF, UL[:, :, nJ:nJ + nO], L2I, UL[:, :, :nJ], VC[li], hw, starts, cfg["pc_range"], pad_hw,
                                  num_groups=cfg["num_groups"], out=ws.agg_out, tables=ws.tab[li] if tabs else None, hole=hole)
            self._layer_after_aggregation(ops.linear_streams, ly, ws.agg_out, ws.x1, QP, ws.x2, ws.x2b, outs[li], XN if li + 1 < nL else None)
        return outs.permute(1, 0, 2, 3)

    # ------------------------------------------------------------------------------------------ one frame
    @_with_tile_tables
    def camera_stage(self, img, dd, cam_ids, pad_hw, block_rows=None):
        """Everything that is independent per camera: backbone, FPN (+MLN), 2D head, depth, proposal
        selection and adaptive-query construction.  img (n,3,H,W) on device for the contiguous camera block `cam_ids`."""
        st, heads = self._camera_maps(img, dd, cam_ids, pad_hw)
        st.update(self.proposals(*heads, st["tokens"], block_rows))
        return st

    @_with_tile_tables
    def _camera_maps(self, img, dd, cam_ids, pad_hw):
        """camera_stage up to the proposals: backbone, FPN (+MLN), 2D head and depth for the camera block -> (st without the proposal
        part, (cls, reg, depth_logit, img2lidar): what `proposals` takes in front of the tokens).  camera_stage_streams runs this once
        over the images of several scene streams and, where a stream's proposals carry a count of their own, `proposals` per stream."""
        cfg = self.cfg
        n = img.shape[0]
        cam_ids = list(cam_ids)
        lo, hi = cam_ids[0], cam_ids[-1] + 1
        assert cam_ids == list(range(lo, hi)) and hi - lo == n, "camera_stage works on a contiguous block of cameras"
        E = cfg["embed_dims"]
        lidar2img = dd["lidar2img"][0, lo:hi]
        # img2lidar = inverse(lidar2img) (farhead.py:798) and the 14-float MLN code (farhead.py:553-556): one launch
        img2lidar, c14 = ops.camera_prep(lidar2img, dd["intrinsics"][0, lo:hi], dd["extrinsics"][0, lo:hi])
        per = ops.plan_images(n)
        if per == n:
            hh = self.sa["reduce"](c14, act="relu")
            mln_scale, mln_shift = self.sa["gamma"](hh), self.sa["beta"](hh)           # (n, E) each
        else:
            # the cameras of several scene streams (camera_stage_streams): these small GEMMs choose their kernel by the row count, so
            # they stay per stream -- each on an aligned copy of its rows, like the one-stream pass's own c14
            mln_scale, mln_shift = (torch.empty((n, E), dtype=torch.float32, device=self.dev) for _ in range(2))
            for r in range(0, n, per):
                hh = self.sa["reduce"](c14[r:r + per].clone(), act="relu")
                self.sa["gamma"](hh, out=mln_scale[r:r + per])
                self.sa["beta"](hh, out=mln_shift[r:r + per])
        feats = self.backbone(img, keep_stage2=False)
        raw, tokens, hw, starts = self.fpn(feats, mln_scale, mln_shift)
        st = dict(tokens=tokens, hw=hw, starts=starts, raw=raw, lidar2img=lidar2img, cams=(lo, hi))
        cls, reg, depth_logit = self.roi_head(raw)
        return st, (cls, reg, depth_logit, img2lidar)

    def camera_stage_streams(self, dds, pad_hw, key, img, stream_keys=None):
        """camera_stage ONCE on the images of len(dds) scene streams (streams.StreamBatch): dds the streams' staged inputs
        (_stage_inputs), each of N cameras; img (len(dds) * N, 3, H, W) their images, stream-major -- the buffer the streams staged
        into (image_slices); key: the buffer set of this pass, whose token buffer (token_slices) spans the streams' slices of the
        batch's one allocation.  lidar2img / intrinsics / extrinsics are the
        streams' concatenated, so camera b * N + n is camera n of stream b everywhere; proposal selection and gather work per camera,
        and in the static top-K mode stream b's rows are [b * N * K, (b + 1) * N * K) of the joint ref2d / ctx / box2d / score2d.
        Every launch chooses its tile as ONE stream's N images would (ops.tiles_as_for), so each image has the bits of its own
        stream's camera_stage.  Returns one `st` dict per stream, views into the joint results.
        stream_keys (the streams' own buffer sets, one per stream): the modes whose proposals carry a count per frame -- the
        fixed-capacity threshold mode and multi-depth topk > 1 in either static mode.  The joint pass then ends behind the 2D head
        (_camera_maps) and `proposals` runs per stream, on that stream's slices of the head's maps, inside its own buffer set: each
        stream gets its own count, overflow flag and multi-depth records, and its reference points land in its own query buffer, as
        in the whole-frame path.  Without stream_keys those modes are refused."""
        cfg = self.cfg
        nb, N, K = len(dds), dds[0]["img"].shape[0], cfg["proposal_topk"]
        per_stream = K is None or self.md_k > 1
        if per_stream and (stream_keys is None or (K is None and cfg.get("proposal_capacity") is None)):
            raise ValueError("camera_stage_streams: the static top-K proposal mode with single-depth proposals only")
        if per_stream and len(stream_keys) != nb:
            raise ValueError("camera_stage_streams: stream_keys names one buffer set per stream (%d), got %d" % (nb, len(stream_keys)))
        if tuple(img.shape) != (nb * N,) + tuple(dds[0]["img"].shape[1:]):
            raise ValueError("camera_stage_streams: img %s is not the %d streams' %d images each" % (tuple(img.shape), nb, N))
        joint = {k: torch.cat([dd[k] for dd in dds], dim=1) for k in ("lidar2img", "intrinsics", "extrinsics")}
        rows = lambda t, b, per: t[b * per:(b + 1) * per]
        res = []
        if per_stream:
            with self.buffers(key), ops.tiles_as_for(N, nb * N):
                st, (cls, reg, depth_logit, img2lidar) = self._camera_maps(img, joint, range(nb * N), pad_hw)
            for b in range(nb):
                sb = dict(tokens=rows(st["tokens"], b, N), raw=[rows(r, b, N) for r in st["raw"]], hw=st["hw"], starts=st["starts"],
                          lidar2img=rows(st["lidar2img"], b, N), cams=(0, N))
                with self.buffers(stream_keys[b]):
                    sb.update(self.proposals([rows(c, b, N) for c in cls], [rows(r, b, N) for r in reg], rows(depth_logit, b, N),
                                             rows(img2lidar, b, N), sb["tokens"]))
                res.append(sb)
            return res
        with self.buffers(key), ops.tiles_as_for(N, nb * N):
            st = self.camera_stage(img, joint, range(nb * N), pad_hw, block_rows=nb * N * K)
        for b in range(nb):
            res.append(dict(tokens=rows(st["tokens"], b, N), raw=[rows(r, b, N) for r in st["raw"]], hw=st["hw"], starts=st["starts"],
                            lidar2img=rows(st["lidar2img"], b, N), cams=(0, N), depth_logit=rows(st["depth_logit"], b, N),
                            peak_weight=rows(st["peak_weight"], b, N), sel_idx=rows(st["sel_idx"], b, N), sel_cnt=rows(st["sel_cnt"], b, N),
                            m_dev=st["m_dev"], overflow=st["overflow"],
                            **{k: rows(st[k], b, N * K) for k in ("ref2d", "ctx", "box2d", "score2d")}))
        return res

    def proposals(self, cls, reg, depth_logit, img2lidar, tokens, block_rows=None):
        """a5 + the adaptive-query part of a6: peak selection and 3D proposal construction for n cameras.
        block_rows (None: the cameras are the frame, or a top-K shard whose rows are static): the cameras are a BLOCK of the frame and
        the result goes into buffers of block_rows rows (camera_block_rows(n)).  Single depth, fixed-capacity threshold mode: the block's
        proposals compacted and zero-padded, with its own count and flag (a rank's record block of the camera-sharded runner).  Multi-depth
        (either static mode): the block's primaries and per-primary records only -- no extra rows, no count, no flag;
        merge_camera_blocks packs the blocks and runs the extras."""
        cfg = self.cfg
        n = tokens.shape[0]
        E = cfg["embed_dims"]
        K = cfg["proposal_topk"]
        capT = cfg.get("proposal_capacity") if K is None else None
        cap = K if K is not None else min(cfg["proposal_cap"], tokens.shape[1])
        while True:
            wgt, sel_idx, sel_cnt = ops.proposal_select(cls, reg, cfg["strides"], cap, thr=cfg["score_thr"], topk=K is not None)
            if K is not None or capT is not None or cap >= tokens.shape[1]:
                break
            # legacy threshold mode keeps EVERY peak above score_thr (yolox_head.py:429-438): a camera that fills the
            # capacity may have lost peaks, so grow and redo (this mode syncs on M anyway)
            if int(sel_cnt.max().item()) < cap:
                break
            cap = min(2 * cap, tokens.shape[1])
        whole = n == cfg["num_cams"] and "head" in self.parts and block_rows is None
        prim = n * cap if capT is None else (capT if block_rows is None else block_rows)
        Kmd = self.md_k
        block = block_rows is not None
        if block and capT is None and (K is None or block_rows != prim):
            raise ValueError("block_rows: a camera block has min(proposal_capacity, its share) rows in the fixed-capacity threshold mode "
                             "and cameras * proposal_topk = %s rows in the top-K mode (got %d)" % (prim if K is not None else None, block_rows))
        # multi-depth: [primaries | extras | hole]; legacy threshold mode sizes the extras from the selection capacity (never overflows).
        # A camera block (block_rows) builds its primaries and records only: merge_camera_blocks packs the blocks and runs the extras
        extra = 0 if (Kmd <= 1 or block) else (self.md_extra_rows(prim) if (K is not None or capT is not None) else (Kmd - 1) * prim)
        rows = prim + extra
        if (K is not None or capT is not None) and whole:
            # every camera is local and the row count is static: the reference points land directly in the adaptive-query rows
            # of the head's query-major buffer (head_stage then has nothing to copy)
            nq = cfg["num_query"]
            ref_out = self._buf(("rf",), (nq + rows + cfg["memory_len"], 3), torch.float32)[nq:nq + rows]
        else:
            ref_out = self._buf(("ref2d",), (rows, 3), torch.float32)
        out = (ref_out, self._buf(("ctx",), (rows, E + 1), torch.float32),
               self._buf(("box2d",), (rows, 4), torch.float32), self._buf(("score2d",), (rows,), torch.float32))
        m_dev = ovf = None
        if (capT is not None or Kmd > 1) and not (block and Kmd > 1):      # a multi-depth block has no count or flag of its own
            m_dev = self._buf(("m_dev",), (1,), torch.int32)
            if capT is not None or K is not None:
                ovf = self._buf(("ovf",), (1,), torch.int32)
                self._overflow = ovf
        if Kmd > 1:
            # part 1 of the multi-depth proposals: the primary rows + a record per primary; the extra rows are written by
            # proposal_extra_rows at the start of the cross-camera part (_head_part), once every camera's primaries exist
            rec = (self._buf(("md_flags",), (prim,), torch.int32), self._buf(("md_info",), (prim, 2 * Kmd), torch.int32))
            i2l = self._buf(("md_i2l",), tuple(img2lidar.shape), torch.float32)
            i2l.copy_(img2lidar)
            ops.proposal_gather_md(reg, cfg["strides"], sel_idx, sel_cnt, wgt, depth_logit, self.depth_stride, cfg["depthnet"],
                                   img2lidar, tokens, cfg["pc_range"], Kmd, self.md_min_bin, rec, out,
                                   primary_rows=prim if capT is not None else 0, score_thr=0.1)
            md = dict(records=rec, img2lidar=i2l, primary_rows=prim, sel_cap=cap if capT is not None else 0, rows=rows)
            return dict(ref2d=out[0], ctx=out[1], box2d=out[2], score2d=out[3], sel_idx=sel_idx, sel_cnt=sel_cnt, depth_logit=depth_logit,
                        peak_weight=wgt, m_dev=m_dev, overflow=ovf, md=md)
        # the log-odds threshold is the reference's hard-coded 0.1 (farhead.py:577), not cfg score_thr
        ref2d, ctx, box2d, score2d = ops.proposal_gather(reg, cfg["strides"], sel_idx, sel_cnt, wgt, depth_logit,
                                                         self.depth_stride, cfg["depthnet"], img2lidar, tokens,
                                                         cfg["pc_range"], score_thr=0.1, out=out, rows_total=rows if capT is not None else 0,
                                                         m_out=m_dev, overflow_out=ovf)
        return dict(ref2d=ref2d, ctx=ctx, box2d=box2d, score2d=score2d, sel_idx=sel_idx, sel_cnt=sel_cnt, depth_logit=depth_logit, peak_weight=wgt,
                    m_dev=m_dev, overflow=ovf)

    @_with_tile_tables
    def head_stage(self, tokens, ref2d, ctx, M, dd, img_metas, hw, starts, pad_hw, m_dev=None, qshard=None):
        """The cross-camera part: streaming memory, query construction, 6-layer decoder, heads, decode (a6-a12).
        M: adaptive-query ROWS.  m_dev (int32 device scalar; fixed-capacity threshold mode): only the first m_dev of them are
        queries, rows [nq + m_dev, nq + M) are the masked hole (their inputs are zero-filled by proposal_gather).
        Three steps: _head_prepare (memory, query construction: the decoder's operands), the decoder, _head_finish (heads, decode,
        memory update).  streams.StreamBatch runs the first and the last per scene stream around ONE decoder_streams pass."""
        hs = self._head_prepare(tokens, ref2d, ctx, M, dd, img_metas, m_dev)
        outs_dec = self.decoder(hs.X2, hs.x0, hs.qpos, tokens, hs.ref, hw, starts, hs.lidar2img, pad_hw, hs.A, hole=hs.hole, qshard=qshard)
        return self._head_finish(hs, outs_dec)

    def _head_prepare(self, tokens, ref2d, ctx, M, dd, img_metas, m_dev=None):
        """The part of head_stage in front of the decoder (a6): scene change, memory pre-update, temporal codes, the query-major
        state buffers -> the decoder's operands and what _head_finish needs, as one object."""
        cfg = self.cfg
        E, at = cfg["embed_dims"], self.prec["dec"]
        lidar2img = dd["lidar2img"][0]
        # ---- scene change / memory (detectors/far3d.py:252-257): the persistent buffers are zeroed IN PLACE
        fresh = img_metas[0]["scene_token"] != self.prev_scene or not self._mem_valid
        if fresh:
            self.prev_scene = img_metas[0]["scene_token"]
            for v in self.mem.values():
                v.zero_()
            self._mem_valid = True
        P_, Lm, nq = cfg["num_propagated"], cfg["memory_len"], cfg["num_query"]
        A, Kt = nq + M + P_, nq + M + Lm
        # query-major state buffers: rows [0,nq) learned queries (constant), [nq,nq+M) adaptive queries, then the Lm memory
        # slots, whose first P_ are the propagated queries and whose rest are the extra self-attention keys
        # (farhead.py:305-311) -- so tgt = TQ[:A], memory = TQ[A:], with no concatenation copies
        TQ, QP, RF = self._query_buffers(M)
        # ---- a6: memory pre-update + temporal codes (one kernel)
        m, _, mem_code, tpos = ops.memory_prepare(self.mem, dd["ego_pose_inv"], dd["timestamp"], self.pseudo_ref, self.dim_t256,
                                                  0.0 if fresh else 1.0, fresh, cfg["pc_range"], P_, temp_ref_out=RF[nq + M:])
        if M > 0 and ref2d.data_ptr() != RF[nq:nq + M].data_ptr():     # already in place in the single-rank static-M path
            RF[nq:nq + M].copy_(ref2d[:M])
        # position codes of the adaptive queries and the memory slots in one pass (rows [nq, Kt))
        qp_raw = self._query_pos(RF[nq:])
        hh = ops.linear(mem_code, self.mln_reduce, act="relu", out_dtype=at)                  # (Lm, 2E): [pe | memory] hidden
        gb_pe = ops.linear(hh[:, :E], self.mln_gb["ego_pose_pe"])                            # (Lm, 2E) gamma | beta
        gb_mem = ops.linear(hh[:, E:], self.mln_gb["ego_pose_memory"])
        t_emb = ops.layernorm(self.te(tpos), *self.te_ln)
        if M > 0:
            g, b = self._gb(self.rec_gb["ego_pose_pe"])
            ops.row_affine_ln(qp_raw[:M], g, b, add=self.time0, out=QP[nq:nq + M])
            g, b = self._gb(self.rec_gb["ego_pose_memory"])
            ops.row_affine_ln(self.ce[1](self.ce[0](ctx[:M], act="relu")), g, b, out=TQ[nq:nq + M])
        g, b = self._gb(gb_pe)
        ops.row_affine_ln(qp_raw[M:], g, b, add=t_emb, out=QP[nq + M:])
        g, b = self._gb(gb_mem)
        ops.row_affine_ln(m["emb"][0], g, b, out=TQ[nq + M:])
        X2 = self._buf(("x2op",), (Kt, 2 * E), at)
        ops.add_cast(TQ, QP, at, out_sum=X2[:, :E], out_a=X2[:, E:])
        hole = (m_dev, nq, nq + M) if m_dev is not None else None
        return SimpleNamespace(X2=X2, x0=TQ[:A], qpos=QP[:A], ref=RF[:A], tokens=tokens, lidar2img=lidar2img, A=A, M=M, m=m, m_dev=m_dev,
                               hole=hole, dd=dd)

    def _head_operand(self, outs_dec):
        """nan_to_num of the decoder's contiguous f32 outputs, in place -> the heads' (rows, E) operand (bf16 decoder: the bf16 copy)."""
        flat = outs_dec.view(-1, outs_dec.shape[-1])
        flatb = ops.nan_to_num_(flat, bf16_copy=self.prec["dec"] == torch.bfloat16)
        return flat if flatb is None else flatb

    def _head_branches(self, linear, hin, cls_out=None):
        """The unfused cls branch (linear, LN + relu, linear, LN + relu, linear) and reg branch (three linears), ONE copy for _head_finish
        (ops.linear, hin (rows, E)) and _head_finish_streams (ops.linear_streams, hin (B, rows, E)) -> (logits, in cls_out if given; box codes)."""
        at, fast = self.prec["dec"], self.prec["dec"] == torch.bfloat16
        def ln_relu(t, ln):
            r = ops.layernorm(_rows(t), *ln, act="relu", bf16_copy=fast)
            return (r[1] if fast else r).view(t.shape)
        h = ln_relu(linear(hin, self.cls_b[0].pc), self.cls_ln[0])
        h = ln_relu(linear(h, self.cls_b[1].pc), self.cls_ln[1])
        cls = linear(h, self.cls_b[2].pc, out=cls_out)
        rr = linear(hin, self.reg_b[0].pc, act="relu", out_dtype=at)
        return cls, linear(linear(rr, self.reg_b[1].pc, act="relu", out_dtype=at), self.reg_b[2].pc)

    @staticmethod
    def _head_result(hs, all_cls, all_box, outs_dec, idx, result, scores=None):
        """One stream's `outs` of the head (hs: its _head_prepare result).  scores (tracking on): the score plane memory_topk ranked and
        the births were judged on, as `memory_scores`."""
        outs = dict(all_cls_scores=all_cls, all_bbox_preds=all_box, outs_dec=outs_dec, num_adaptive=hs.M, num_adaptive_dev=hs.m_dev,
                    feat_flatten=hs.tokens, reference_points=hs.ref, memory_topk=idx, result=result)
        if scores is not None:
            outs["memory_scores"] = scores
        return outs

    def _head_finish(self, hs, outs_dec):
        """The part of head_stage behind the decoder: the shared cls / reg heads over all layers (_head_branches, or the row chain),
        finalize, decode, the memory's post-update.  hs: _head_prepare's result; outs_dec (layers, A, E) f32, contiguous."""
        cfg, A, nl = self.cfg, hs.A, self.cfg["num_layers"]
        hin = self._head_operand(outs_dec)          # ---- a10: shared heads over all layers at once (farhead.py:646-664)
        if self._row_chains([self.branch_rc]):      # both branches in one row-resident launch (csrc/rowchain.hip)
            cls_flat = self._buf(("cls_flat",), (nl * A, cfg["num_classes"]), torch.float32)
            rr = self._buf(("reg_flat",), (nl * A, cfg["code_size"]), torch.float32)
            ops.rowchain_branches(hin, self.branch_rc, cls_flat, rr)
        else:
            cls_flat, rr = self._head_branches(ops.linear, hin)
        all_cls = cls_flat.view(nl, 1, A, cfg["num_classes"])
        box_flat, sc = ops.head_finalize(rr, hs.ref, all_cls, cfg["pc_range"], nl, cfg["num_classes"], hole=hs.hole)
        all_box = box_flat.view(nl, 1, A, cfg["code_size"])
        # ---- a11: memory post-update (farhead.py:479-508): top-k by max-class score, push, truncate, ego warp -- in place
        # (the top-k rides in the decode's launch as a second workgroup: far3d_decode_topk_mem -- both rank the last layer's outputs)
        if self.track is None:
            result, idx = self.decode(all_cls, all_box, mem_scores=sc, mem_K=cfg["topk_proposals"])
            if self.dedup is not None:
                result = dict(result)
                self._box_dedup(result, lambda v: v[None], lambda v: v[0])
        else:           # the same decode + the boxes' query rows, then the ids: the one-stream case of the streams path
            results, idx = self.decode_streams(all_cls[-1], all_box[-1], sc[None], cfg["topk_proposals"], tracked=True)
            self._box_dedup(results)
            self._track_update(results, idx, sc[None], [hs], self.mem["track"], self._track_next, self.mem.get("track_hits"))
            result, idx = {k: v[0] for k, v in results.items()}, idx[0]
        ops.memory_post_update(hs.m, idx, outs_dec[-1], all_box[-1][0], hs.dd["ego_pose"], hs.dd["timestamp"], self.mem)
        return self._head_result(hs, all_cls, all_box, outs_dec, idx, result, sc if self.track is not None else None)

    def _box_dedup(self, results, to_streams=lambda v: v, from_streams=lambda v: v):
        """Duplicate suppression on (cfg dedup): ONE far3d_box_dedup launch behind the decode for the B streams of results (leading B
        after to_streams); results gains dup_keep and dup_of.  It reads the decode's outputs and writes none of them.  Off: nothing."""
        if self.dedup is not None:
            dk, of = ops.box_dedup(*(to_streams(results[k]) for k in ("boxes_3d", "scores_3d", "labels_3d", "keep")), **self.dedup)
            results["dup_keep"], results["dup_of"] = from_streams(dk), from_streams(of)

    def _track_update(self, results, idx, scores, hss, mem_track, next_id, mem_hits=None):
        """One far3d_track_update launch for the B streams of results / idx / scores (leading B; hss: their _head_prepare results): the
        streams' mem_track (B, L) and next_id (B, 1) are updated in place, results gains track_ids (B, Kdec).  The propagated rows are
        the last num_propagated of the A.  mem_hits (track records=True): the streams' (B, L) counter plane, updated in place by ONE
        far3d_track_records launch behind the ids; results gains track_age, track_primary (B, Kdec) and track_velocity (B, Kdec, 3).
        It reads the pre-updated memory hs.m, so it runs before memory_post_update -- which writes the state, never hs.m."""
        P, A = self.cfg["num_propagated"], hss[0].A
        results["track_ids"] = ops.track_update(idx, scores, mem_track, next_id, A - P, P, self.track["birth_thr"],
                                                query_idx=results["query_idx"])
        if mem_hits is not None:
            B, L = mem_hits.shape
            if B == 1:
                m_ref, m_ts = hss[0].m["ref"], hss[0].m["ts"].view(1, L)
            else:       # every stream's memory_prepare wrote buffers of its own: one gathering copy each
                m_ref = torch.cat([hs.m["ref"] for hs in hss], out=self._buf(("trk_ref", B), (B, L, 3), torch.float32))
                m_ts = torch.cat([hs.m["ts"] for hs in hss], out=self._buf(("trk_ts", B), (B, L, 1), torch.float64)).view(B, L)
            results["track_age"], results["track_primary"], results["track_velocity"] = ops.track_records(
                idx, mem_track, mem_hits, results["query_idx"], results["track_ids"], results.get("dup_keep", results["keep"]),
                results["boxes_3d"], m_ref, m_ts, A, A - P, P)      # dedup on: the primary is the first SURVIVING box of its id

    def _head_finish_streams(self, hss, outs_dec, enter, track=None):
        """_head_finish for B scene streams (streams.StreamBatch): hss the B _head_prepare results, outs_dec decoder_streams' result
        (B, layers, A, E), enter(b) a context manager that makes the engine stream b (its buffer set and streaming memory).  Returns the
        B result dicts of _head_finish, bit for bit.  The row-local work runs once over all streams' rows on (B, layers * A, .)
        buffers: ONE gathering copy of the decoder's (layers, B, A, E) rows into stream-major order, nan_to_num, _head_finish's own
        unfused cls / reg branches (_head_branches; StreamBatch refuses fused_rows) through ops.linear_streams (the tile of ONE stream's
        layers * A rows); the decode and the memory update's top-k of all streams are ONE far3d_decode_topk_mem_streams launch.  Per
        stream stay head_finalize and memory_post_update.  track (tracking on): the streams' (mem_track (B, L), next_id (B, 1)[,
        mem_hits (B, L)]), updated by ONE far3d_track_update launch [and ONE far3d_track_records launch]."""
        cfg = self.cfg
        E, nl, ncls, code = cfg["embed_dims"], cfg["num_layers"], cfg["num_classes"], cfg["code_size"]
        B, A = len(hss), hss[0].A
        buf = lambda name, shape, dt: self._buf(("hs_" + name, B), shape, dt)
        OD = buf("outs_dec", (B, nl, A, E), torch.float32).copy_(outs_dec)
        CLS, rr = self._head_branches(ops.linear_streams, self._head_operand(OD).view(B, nl * A, E), cls_out=buf("cls", (B, nl * A, ncls), torch.float32))
        BOX, SC = buf("box", (B, nl * A, code), torch.float32), buf("score", (B, A), torch.float32)
        for b, hs in enumerate(hss):
            ops.head_finalize(rr[b], hs.ref, CLS[b], cfg["pc_range"], nl, ncls, hole=hs.hole, out=(BOX[b], SC[b]))
        results, idx = self.decode_streams(CLS.view(B, nl, A, ncls)[:, -1], BOX.view(B, nl, A, code)[:, -1], SC, cfg["topk_proposals"],
                                           tracked=self.track is not None)
        self._box_dedup(results)
        if self.track is not None:
            self._track_update(results, idx, SC, hss, *track)
        res = []
        for b, hs in enumerate(hss):
            all_cls, all_box = CLS[b].view(nl, 1, A, ncls), BOX[b].view(nl, 1, A, code)
            with enter(b):
                ops.memory_post_update(hs.m, idx[b], OD[b, -1], all_box[-1][0], hs.dd["ego_pose"], hs.dd["timestamp"], self.mem)
            res.append(self._head_result(hs, all_cls, all_box, OD[b], idx[b], {k: v[b] for k, v in results.items()},
                                         SC[b] if self.track is not None else None))
        return res

    def decode_streams(self, cls_last, box_last, mem_scores, mem_K, tracked=False):
        """`decode` of B scene streams in one launch: cls_last (B, A, num_classes) / box_last (B, A, code_size) the last layer's logits
        and boxes, mem_scores (B, A) -- views with contiguous streams.  -> (dict of (B, .) results, idx (B, mem_K)).  tracked: the
        dict also holds query_idx (B, K), the query row of every box (ops.decode_topk_tracked)."""
        B, A, ncls = cls_last.shape
        K, ws, rng = self._decode_args(A * ncls, B)
        fn = ops.decode_topk_tracked if tracked else ops.decode_topk_mem_streams
        return fn(cls_last, box_last, K, rng, mem_scores, mem_K, workspace=ws)

    def _stage_inputs(self, data):
        """Copy the frame's inputs into static device buffers (so that a captured graph can be replayed on them)."""
        dev = self.dev
        img = data["img"]
        if img.dim() == 5:
            assert img.shape[0] == 1, "batch 1 per engine (one scene stream per GPU)"
            img = img[0]
        keys = ("lidar2img", "intrinsics", "extrinsics", "ego_pose", "ego_pose_inv", "timestamp")
        cur = self._ins.get(self._par)
        if cur is None or tuple(cur["img"].shape) != tuple(img.shape):
            # (re)allocation: graphs captured on the old buffers of THIS parity are stale.  The single-graph mode drops its graph
            # here; the pipeline's per-parity graphs are dropped by FramePipeline.slot BEFORE it decides to replay (this dict is no
            # longer the one they were captured on), and its streams are never dropped, so a scene start can always wait for heads in flight.
            # a buffer set with an entry in image_slices (a scene stream of streams.StreamBatch) stages its images in the slice that callable
            # hands out -- its part of ONE (B * N, 3, H, W) buffer, which camera_stage_streams reads without a copy
            owner = self.image_slices.get(self._par)
            cur = dict(img=owner(tuple(img.shape)) if owner is not None else torch.empty(tuple(img.shape), dtype=torch.float32, device=dev))
            for k in keys:
                cur[k] = torch.empty(tuple(data[k].shape), dtype=torch.float64 if k == "timestamp" else torch.float32, device=dev)
            self._ins[self._par] = cur
            self._graph = None
        cur["img"].copy_(img, non_blocking=True)
        for k in keys:
            cur[k].copy_(data[k], non_blocking=True)
        return cur

    def _frame_body(self, dd, img_metas, pad_hw):
        return self._head_part(self._camera_part(dd, pad_hw), dd, img_metas, pad_hw)

    def _camera_part(self, dd, pad_hw):
        img = dd["img"]
        return self.camera_stage(img, dd, range(img.shape[0]), pad_hw)

    def _head_rows(self, st, N):
        """The step of _head_part in front of head_stage, for a frame of N cameras whose camera stage gave `st`: the multi-depth extra
        rows, then -> (M: adaptive-query rows, Mb: rows of the 2D boxes, m_dev: the device count of the rows that hold a query,
        None where the shapes are exact).  streams.StreamBatch calls it per stream (static modes: no sync)."""
        M = self.static_adaptive_rows(N)
        md = st.get("md")
        m_dev = st["m_dev"]
        if md is not None:
            # part 2 of the multi-depth proposals (every camera's primaries exist): the extra rows, M' on the device, the hole
            self.proposal_extra_rows(st, M is not None)
        if M is None:
            if md is None:
                M = int(st["sel_cnt"].sum().item())      # legacy threshold mode: the reference's data-dependent M, one host sync
                Mb = M
            else:
                M, Mb = (int(v) for v in torch.stack([m_dev[0], st["sel_cnt"].sum(dtype=torch.int32)]).tolist())   # M' and M: one sync
            m_dev = None                                 # exact shapes, no hole
        else:
            Mb = M if md is None else md["primary_rows"]
        return M, Mb, m_dev

    @staticmethod
    def _head_outputs(outs, st, Mb):
        """The camera stage's part of a frame's outputs (st; Mb: _head_rows') into the head's `outs`."""
        outs.update(fpn=st["raw"], depth_logit=st["depth_logit"], bbox2d=st["box2d"][:Mb], bbox2d_scores=st["score2d"][:Mb],
                    sel_idx=st["sel_idx"], sel_cnt=st["sel_cnt"], proposal_overflow=st["overflow"])
        if st.get("md") is not None:
            outs["md_records"] = st["md"]["records"]
        return outs

    def _head_part(self, st, dd, img_metas, pad_hw):
        M, Mb, m_dev = self._head_rows(st, dd["img"].shape[0])
        outs = self.head_stage(st["tokens"], st["ref2d"], st["ctx"], M, dd, img_metas, st["hw"], st["starts"], pad_hw, m_dev=m_dev)
        return self._head_outputs(outs, st, Mb)

    @contextlib.contextmanager
    def buffers(self, key):
        """Run what is inside with the engine's persistent buffers taken from the set `key` (any hashable): camera blocks of one frame
        that must keep their results side by side, e.g. camera_stage(..., block_rows=...) per block before merge_camera_blocks."""
        keep = self._par
        self._par = key
        try:
            yield
        finally:
            self._par = keep

    def camera_block_rows(self, ncam):
        """Rows of the proposal buffers of a block of `ncam` cameras (camera_stage's block_rows) in the two static proposal modes."""
        K, capT = self.cfg["proposal_topk"], self.cfg.get("proposal_capacity")
        if K is not None:
            return ncam * K
        if capT is None:
            raise ValueError("camera blocks need a static proposal mode (proposal_topk or proposal_capacity): the legacy threshold mode syncs on M")
        return min(capT, ncam * self.cfg["proposal_cap"])

    def merge_camera_blocks(self, blocks):
        """blocks: the results of camera_stage(..., block_rows=self.camera_block_rows(n)) for contiguous camera blocks that together are the
        frame, in ascending camera order, each run inside its own `buffers` set.  Packs their proposals into the frame's layout
        (proposal_merge_blocks: primaries camera-major, records with the frame's camera indices, one count, one flag), straight into
        the adaptive-query rows of the head's buffer, then runs proposal_extra_rows when multi_depth topk > 1.  Two launches (one for
        a single depth) + a small copy per block (img2lidar), no sync.  -> the proposal part of a whole-frame camera_stage result
        (ref2d, ctx, box2d, score2d, sel_cnt, m_dev, overflow, md, md_records, rows) for head_stage."""
        cfg = self.cfg
        N, E, nq, Kmd = cfg["num_cams"], cfg["embed_dims"], cfg["num_query"], self.md_k
        K = cfg["proposal_topk"]
        capT = cfg.get("proposal_capacity") if K is None else None
        if K is None and capT is None:
            raise ValueError("merge_camera_blocks needs a static proposal mode (proposal_topk or proposal_capacity)")
        P = N * K if K is not None else capT
        if [b["cams"][0] for b in blocks] + [N] != [0] + [b["cams"][1] for b in blocks]:
            raise ValueError("merge_camera_blocks: the blocks must be the frame's cameras in ascending order, got %s" % [b["cams"] for b in blocks])
        rows = P + self.md_extra_rows(P)
        out = (self._buf(("rf",), (nq + rows + cfg["memory_len"], 3), torch.float32)[nq:nq + rows], self._buf(("ctx",), (rows, E + 1), torch.float32),
               self._buf(("box2d",), (rows, 4), torch.float32), self._buf(("score2d",), (rows,), torch.float32))
        sel_cnt = self._buf(("sel_cnt",), (N,), torch.int32)
        m_dev = ovf = None
        if capT is not None or Kmd > 1:
            m_dev, ovf = self._buf(("m_dev",), (1,), torch.int32), self._buf(("ovf",), (1,), torch.int32)
            self._overflow = ovf
        rec = md = None
        if Kmd > 1:
            rec = (self._buf(("md_flags",), (P,), torch.int32), self._buf(("md_info",), (P, 2 * Kmd), torch.int32))
            i2l = self._buf(("md_i2l",), (N, 4, 4), torch.float32)
            for b in blocks:
                i2l[b["cams"][0]:b["cams"][1]].copy_(b["md"]["img2lidar"])
            md = dict(records=rec, img2lidar=i2l, primary_rows=P, sel_cap=blocks[0]["md"]["sel_cap"], rows=rows)
        parts = [dict(rows=(b["ref2d"], b["ctx"], b["box2d"], b["score2d"]), sel_cnt=b["sel_cnt"], first_cam=b["cams"][0],
                      records=b["md"]["records"] if Kmd > 1 else None, overflow=b["overflow"],
                      count=(b["cams"][1] - b["cams"][0]) * K if K is not None else b["m_dev"]) for b in blocks]
        ops.proposal_merge_blocks(parts, out, sel_cnt, P, records_out=rec, m_out=m_dev, overflow_out=ovf)
        st = dict(ref2d=out[0], ctx=out[1], box2d=out[2], score2d=out[3], sel_cnt=sel_cnt, m_dev=m_dev, overflow=ovf, md=md, rows=rows,
                  md_records=rec)
        if md is not None:
            self.proposal_extra_rows(st, True)
        return st

    def proposal_extra_rows(self, st, fill_hole=True):
        """The multi-depth extra rows of a frame whose primaries proposals() built (st: its result): one launch, no sync."""
        md = st["md"]
        ops.proposal_extra_rows(st["sel_cnt"], md["sel_cap"], md["primary_rows"], self.md_k, md["records"], md["img2lidar"],
                                self.cfg["depthnet"], self.cfg["pc_range"], (st["ref2d"], st["ctx"], st["box2d"], st["score2d"]),
                                fill_hole=fill_hole, m_out=st["m_dev"], overflow_out=st["overflow"])

    def _capture_frame(self, dd, img_metas, pad_hw):
        """FramePipeline's capture: the camera stages and the head of the current buffer set as two hipGraphs."""
        gc, gh = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(gc):
            st = self._camera_part(dd, pad_hw)
        with torch.cuda.graph(gh):
            outs = self._head_part(st, dd, img_metas, pad_hw)
        return gc, gh, outs, None

    def output_stream(self):
        """The stream the latest forward_frame's outputs are produced on."""
        return self._pipe.output_stream() if self.pipeline else torch.cuda.current_stream(self.dev)

    def wait_outputs(self):
        """Order the caller's current stream after the latest frame's outputs (a no-op outside pipeline mode)."""
        if self._ready is not None:
            torch.cuda.current_stream(self.dev).wait_event(self._ready)

    def _query_buffers(self, M):
        """The head's query-major state buffers tq / qp (Kt, E) and rf (Kt, 3) for M adaptive-query rows, Kt = num_query + M +
        memory_len.  The constant learned-query rows are written when the buffers are (re)allocated (a new buffer set, or M changed
        in the legacy threshold mode), not per frame."""
        cfg = self.cfg
        E, nq = cfg["embed_dims"], cfg["num_query"]
        Kt = nq + M + cfg["memory_len"]
        old = self._bufs.get((self._par, "tq"))
        TQ = self._buf(("tq",), (Kt, E), torch.float32)
        QP = self._buf(("qp",), (Kt, E), torch.float32)
        RF = self._buf(("rf",), (Kt, 3), torch.float32)
        if TQ is not old:
            TQ[:nq].copy_(self.tgt_fixed); QP[:nq].copy_(self.qpos_fixed); RF[:nq].copy_(self.ref_fixed)
        return TQ, QP, RF

    def _alloc_query_buffers(self, ncam):
        """Before a capture: make the query buffers and their constant rows exist, so that the captured head neither allocates them
        nor rewrites the constants on every replay."""
        self._query_buffers(self.static_adaptive_rows(ncam))

    @torch.no_grad()
    @_with_tile_tables
    def forward_frame(self, data, img_metas):
        """data: the reference's per-frame dict (img (1,N,3,H,W), lidar2img, intrinsics, extrinsics, ego_pose(_inv),
        timestamp); tensors may live on the host (they are uploaded) or already on the device.  With `use_graph` the
        steady-state frame (same scene, static proposal mode) is captured once into a hipGraph and replayed; the first
        frame of every scene runs eagerly (it resets the streaming memory in place, so the captured graph stays valid).
        Outputs live in engine-owned buffers that the next frame overwrites: clone what must outlive it."""
        pad_hw = tuple(img_metas[0]["pad_shape"][0][:2])
        steady = img_metas[0]["scene_token"] == self.prev_scene and self._mem_valid
        if self.pipeline and self.use_graph and self.static_adaptive_rows() is not None:
            self._par = self._fidx % max(2, int(self.pipeline_sets))
            self._fidx += 1
            if steady:
                return self._pipe.frame(self._capture_frame, data, img_metas, pad_hw)
            self._pipe.drain()               # scene start: runs eagerly on the caller's stream, after everything in flight
            outs = self._frame_body(self._stage_inputs(data), img_metas, pad_hw)
            self._overflow = outs.get("proposal_overflow")
            return outs
        dd = self._stage_inputs(data)
        if self.use_graph and steady and self.static_adaptive_rows() is not None:
            if self._graph is None:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._graph_outs = self._frame_body(dd, img_metas, pad_hw)
                self._graph = g
            self._graph.replay()
            self._overflow = self._graph_outs.get("proposal_overflow")
            return self._graph_outs
        outs = self._frame_body(dd, img_metas, pad_hw)
        self._overflow = outs.get("proposal_overflow")
        return outs

    # ------------------------------------------------------------------------------------------ a12: NMS-free decode
    def _decode_args(self, n, B=None):
        """K, the workspace and the centre range of the decode of n = A * num_classes logits, for one stream (B None) or B streams."""
        K = min(self.cfg["max_num"], n)
        need = ops.decode_ws_bytes(n, K)      # > 0 beyond 40960 logits (many adaptive queries): chunked two-launch decode
        key, size = (("decode_ws",), need) if B is None else (("decode_ws_streams", B), B * need)
        return K, (self._buf(key, (size,), torch.uint8) if need else None), self.cfg.get("post_center_range", self.cfg["pc_range"])

    def decode(self, all_cls, all_box, mem_scores=None, mem_K=None):   # core/bbox/coders/nms_free_coder.py:39-112; farhead.py:1224-1245
        K, ws, rng = self._decode_args(all_cls[-1][0].numel())
        return ops.decode_topk(all_cls[-1][0], all_box[-1][0], K, rng, workspace=ws, mem_scores=mem_scores, mem_K=mem_K)

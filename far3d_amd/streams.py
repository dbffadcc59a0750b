"""StreamBatch: several scene streams on ONE engine -- one set of weights, one decoder pass per call for all of them.

Far3DEngine.forward_frame runs one scene stream (its `B == 1` assertion stays).  StreamBatch(engine, streams=B) takes one frame per
stream and call: the camera stage and the head's bookkeeping (memory prepare, position codes, MLN rows, cls / reg branches, finalize,
decode, memory update) run per stream on the engine's own code, each stream in its own buffer set and with its own streaming memory;
the six decoder layers run once for all streams (Far3DEngine.decoder_streams: per layer one far3d_attention_streams launch, one
far3d_aggregate_batched launch, every row-local launch over all B * A rows).  Every stream's outputs are, bit for bit, those of a
plain engine with the same weights fed that stream's frames -- whatever B is, and for B = 1 too.

Scope: eager execution on one GPU in the static top-K proposal mode (cfg proposal_topk = K) with single-depth proposals and the
unfused decoder layers.  That mode has no hole of unused query rows, which far3d_aggregate_batched cannot skip.  Everything else is
refused with a ValueError that names the option."""
import contextlib
import functools

import torch

from . import ops


def _refusal(engine):
    """The first engine option StreamBatch does not run with, as the text of a ValueError; None when there is none."""
    cfg = engine.cfg
    if "head" not in engine.parts or "backbone" not in engine.parts:
        return "parts=%s: StreamBatch runs whole frames (backbone, neck, roi, head)" % (engine.parts,)
    if cfg["proposal_topk"] is None:
        if cfg.get("proposal_capacity") is not None:
            return ("proposal_capacity=%s: the fixed-capacity threshold mode leaves a hole of unused query rows, which the batched "
                    "aggregation cannot skip; use proposal_topk=K" % cfg["proposal_capacity"])
        return "proposal_topk=None (the reference's threshold mode): its query count depends on the frame; use proposal_topk=K"
    if engine.md_k > 1:
        return "multi_depth topk=%d: the extra rows leave a hole of unused query rows; use topk=1" % engine.md_k
    if engine.use_graph:
        return "use_graph: StreamBatch runs eagerly"
    if engine.pipeline:
        return "pipeline: StreamBatch runs eagerly, frame by frame"
    if engine._row_chains(ly["rc"] for ly in engine.layers):
        return "fused_rows: the batched decoder pass is the unfused layer body; set engine.fused_rows = False"
    if engine.agg_variant != 0:
        return "agg_variant=%s: the batched aggregation is the default kernel" % engine.agg_variant
    if engine.agg_split_extra:
        return "agg_split_extra=%s: the batched aggregation has no sibling workgroups" % engine.agg_split_extra
    return None


class StreamBatch:
    def __init__(self, engine, streams):
        if int(streams) < 1:
            raise ValueError("streams=%s: at least one scene stream" % (streams,))
        why = _refusal(engine)
        if why is not None:
            raise ValueError("StreamBatch: " + why)
        self.engine, self.streams = engine, int(streams)
        # per stream: the streaming memory (allocated once, zeroed in place on that stream's scene change) and the scene it is in
        self._state = [dict(mem={k: torch.zeros_like(v) for k, v in engine.mem.items()}, prev_scene=None, mem_valid=False)
                       for _ in range(self.streams)]
        self._tokens = None         # (B, N, S, 256): stream b's camera stage writes slice b, the decoder pass reads all of it
        for b in range(self.streams):
            engine.token_slices[self._key(b)] = functools.partial(self._token_slice, b)

    def _key(self, b):
        return ("stream", id(self), b)

    def _token_slice(self, b, N, S, dtype):
        t = self._tokens
        if t is None or tuple(t.shape) != (self.streams, N, S, 256) or t.dtype != dtype:
            t = self._tokens = torch.empty((self.streams, N, S, 256), dtype=dtype, device=self.engine.dev)
        return t[b]

    @contextlib.contextmanager
    def _stream(self, b):
        """The engine as stream b sees it: its buffer set, its streaming memory, its scene."""
        e, s = self.engine, self._state[b]
        keep = (e.mem, e.prev_scene, e._mem_valid)
        e.mem, e.prev_scene, e._mem_valid = s["mem"], s["prev_scene"], s["mem_valid"]
        try:
            with e.buffers(self._key(b)):
                yield
        finally:
            s["prev_scene"], s["mem_valid"] = e.prev_scene, e._mem_valid
            e.mem, e.prev_scene, e._mem_valid = keep

    def reset_memory(self, b=None):
        """Forget the streaming memory of stream b (None: of every stream): its next frame is the first of a scene."""
        for i in (range(self.streams) if b is None else [int(b)]):
            self._state[i]["prev_scene"], self._state[i]["mem_valid"] = None, False

    def memory(self, b):
        """Stream b's streaming memory (the dict of Far3DEngine.mem)."""
        return self._state[b]["mem"]

    @torch.no_grad()
    def forward_frames(self, datas, img_metas_list):
        """One frame per stream: datas[b] / img_metas_list[b] as Far3DEngine.forward_frame takes them (same image size and camera count
        in every stream).  Returns a list of B output dicts with forward_frame's keys.  Outputs live in buffers of the stream's own
        set that its next frame overwrites: clone what must outlive it."""
        e, B = self.engine, self.streams
        if len(datas) != B or len(img_metas_list) != B:
            raise ValueError("forward_frames: one frame per stream (%d), got %d / %d" % (B, len(datas), len(img_metas_list)))
        why = _refusal(e)          # the options are attributes: they may have been set since the constructor looked
        if why is not None:
            raise ValueError("StreamBatch: " + why)
        pad_hw = tuple(img_metas_list[0][0]["pad_shape"][0][:2])
        if any(tuple(m[0]["pad_shape"][0][:2]) != pad_hw for m in img_metas_list):
            raise ValueError("forward_frames: every stream's frame must have the same padded size")
        cfg = e.cfg
        with ops.use_tile_tables(e.bf16_tile_table()):
            sts, hss = [], []
            for b in range(B):
                with self._stream(b):
                    dd = e._stage_inputs(datas[b])
                    st = e._camera_part(dd, pad_hw)
                    M = e.static_adaptive_rows(dd["img"].shape[0])
                    hss.append(e._head_prepare(st["tokens"], st["ref2d"], st["ctx"], M, dd, img_metas_list[b], st["m_dev"]))
                    sts.append(st)
            pick = lambda name: [getattr(hs, name) for hs in hss]
            outs_dec = e.decoder_streams(pick("X2"), pick("x0"), pick("qpos"), pick("tokens"), pick("ref"), sts[0]["hw"], sts[0]["starts"],
                                         pick("lidar2img"), pad_hw, hss[0].A)
            res = []
            for b, (st, hs) in enumerate(zip(sts, hss)):
                with self._stream(b):
                    # the heads read a stream's layers as ONE (layers * A, E) block: the stream's rows of the pass, gathered
                    od = e._buf(("outs_dec",), (len(e.layers), hs.A, cfg["embed_dims"]), torch.float32)
                    od.copy_(outs_dec[b])
                    outs = e._head_finish(hs, od)
                    outs.update(fpn=st["raw"], depth_logit=st["depth_logit"], bbox2d=st["box2d"][:hs.M], bbox2d_scores=st["score2d"][:hs.M],
                                sel_idx=st["sel_idx"], sel_cnt=st["sel_cnt"], proposal_overflow=st["overflow"])
                    res.append(outs)
        return res

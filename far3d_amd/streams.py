"""StreamBatch: several scene streams on ONE engine -- one set of weights, one pass per call for all of them.

Far3DEngine.forward_frame runs one scene stream (its `B == 1` assertion stays).  StreamBatch(engine, streams=B) takes one frame per
stream and call.  Per stream stay the parts that carry a stream's own state: staging its inputs, the streaming memory (memory prepare,
scene change, memory update), the query construction and head_finalize, each stream in its own buffer set.  Shared by all streams:
  * the six decoder layers (Far3DEngine.decoder_streams: per layer one far3d_attention_streams launch, one far3d_aggregate_batched
    launch, every row-local launch over all B * A rows) -- always;
  * camera_batch: the camera stage (backbone, FPN, 2D head, proposals) as ONE pass over the B * N images of the B frames
    (Far3DEngine.camera_stage_streams), in chunks of streams where the kernels' 32-bit extents bound a launch (stream_chunks);
  * head_batch: the cls / reg branches over every stream's layers * A rows as one launch sequence, and the decode and memory top-k of
    all streams as ONE far3d_decode_topk_mem_streams launch (Far3DEngine._head_finish_streams).
With both switches off a call is the per-stream camera stage and head around the one decoder pass.  Every stream's outputs are, bit
for bit, those of a plain engine with the same weights fed that stream's frames -- whatever B is, for B = 1 too, with any switches.

Scope: eager execution on one GPU with the unfused decoder layers.  By default the static top-K proposal mode (cfg proposal_topk = K)
with single-depth proposals: the mode without a hole of unused query rows, which far3d_aggregate_batched cannot skip.
StreamBatch(..., hole_rows=True) also runs the modes that leave one -- the fixed-capacity threshold mode (proposal_topk=None,
proposal_capacity=R: the reference's shipped proposal rule at a static row count) and multi_depth topk > 1 in either static mode.
There every stream carries its own count of rows that hold a query, on the device: `proposals` runs per stream behind the joint
backbone / FPN / 2D-head pass, the decoder pass hands the B counts to far3d_attention_streams and far3d_aggregate_batched_holes, and
head_finalize masks each stream's hole.  No host sync in any mode; check_proposal_overflow() is the one that reads the flags.
Track ids (engine cfg track): the streams' id queues and counters are rows of one tensor each, so head_batch updates all of them in ONE
far3d_track_update launch; every stream's ids are those of a plain engine fed its frames.  Track records (track records=True): the
streams' hit counters are the rows of a third tensor, updated by ONE far3d_track_records launch behind the ids.
Duplicate suppression (engine cfg dedup): head_batch makes ONE far3d_box_dedup launch behind the joint decode, a workgroup per stream.
Everything else is refused with a ValueError that names the option."""
import contextlib
import functools

import torch

from . import lib as _lib
from . import ops

# What the convolution entries bound for ONE launch (csrc/igemm.hip, far3d_conv2d_nhwc; csrc/conv_ws.hip, the grouped entry): the span
# of all images of an input map in bytes -- ((N - 1) * image stride + H * W * pixel stride) * element size < 0x7fffffff -- and the
# pixel count, N * H * W < 2^31 - 4096.  A map of at least one byte per pixel meets the second whenever it meets the first.
SPAN_LIMIT_BYTES = 0x7fffffff


def stream_chunks(streams, images, image_span, limit=SPAN_LIMIT_BYTES, max_streams=None):
    """Sizes of the camera passes for `streams` scene streams of `images` cameras each: a list of stream counts, in stream order, that
    sums to `streams`.  image_span: bytes of the largest map one image has in the pass (Far3DEngine.camera_image_span); a pass of n
    streams keeps n * images * image_span below `limit`, the bound of the kernels' 32-bit extents, so the library never has to refuse
    a launch for the chunking to be found.  max_streams caps the streams per pass.  A pass is never empty: where even one stream is
    over the limit the passes are single streams, which then fail or run exactly as the per-stream camera stage does."""
    streams, images, image_span = int(streams), int(images), int(image_span)
    if streams < 1 or images < 1 or image_span < 1:
        raise ValueError("stream_chunks: streams=%d images=%d image_span=%d must all be positive" % (streams, images, image_span))
    if max_streams is not None and int(max_streams) < 1:
        raise ValueError("stream_chunks: max_streams=%s: a pass holds at least one stream" % (max_streams,))
    per = max(1, (int(limit) - 1) // (images * image_span))          # the largest n with n * images * image_span < limit
    if max_streams is not None:
        per = min(per, int(max_streams))
    per = min(per, streams)
    return [per] * (streams // per) + ([streams % per] if streams % per else [])


def _refusal(engine, hole_rows=False):
    """The first engine option StreamBatch does not run with, as the text of a ValueError; None when there is none.
    hole_rows: the runner takes the modes with a hole of unused query rows (StreamBatch's keyword)."""
    cfg = engine.cfg
    if "head" not in engine.parts or "backbone" not in engine.parts:
        return "parts=%s: StreamBatch runs whole frames (backbone, neck, roi, head)" % (engine.parts,)
    if cfg["proposal_topk"] is None:
        if cfg.get("proposal_capacity") is not None:
            if not hole_rows:
                return ("proposal_capacity=%s: the fixed-capacity threshold mode leaves a hole of unused query rows, which the batched "
                        "aggregation cannot skip; use proposal_topk=K" % cfg["proposal_capacity"])
        elif hole_rows:
            return ("proposal_topk=None without proposal_capacity (the reference's threshold mode): its query count depends on the frame; "
                    "use proposal_capacity=R or proposal_topk=K")
        else:
            return "proposal_topk=None (the reference's threshold mode): its query count depends on the frame; use proposal_topk=K"
    if engine.md_k > 1 and not hole_rows:
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
    def __init__(self, engine, streams, camera_batch=True, head_batch=True, max_camera_streams=None, hole_rows=False):
        """camera_batch / head_batch: the shared camera pass and the shared head launches (module docstring); both off is the
        per-stream path around the one decoder pass.  max_camera_streams caps the streams of one camera pass (stream_chunks).
        hole_rows: also run the modes that leave a hole of unused query rows (module docstring); off, they are refused."""
        if int(streams) < 1:
            raise ValueError("streams=%s: at least one scene stream" % (streams,))
        if max_camera_streams is not None and int(max_camera_streams) < 1:
            raise ValueError("max_camera_streams=%s: a camera pass holds at least one stream" % (max_camera_streams,))
        self.hole_rows = bool(hole_rows)
        why = _refusal(engine, self.hole_rows)
        if why is not None:
            raise ValueError("StreamBatch: " + why)
        self.engine, self.streams = engine, int(streams)
        self._overflow = [None] * int(streams)      # per stream: the latest frame's overflow flag (device int32; None: the mode has none)
        self.camera_batch, self.head_batch, self.max_camera_streams = bool(camera_batch), bool(head_batch), max_camera_streams
        self.camera_chunks = None   # the stream counts of the latest call's camera passes (camera_batch)
        # per stream: the streaming memory (allocated once, zeroed in place on that stream's scene change) and the scene it is in
        self._state = [dict(mem={k: torch.zeros_like(v) for k, v in engine.mem.items()}, prev_scene=None, mem_valid=False)
                       for _ in range(self.streams)]
        # track ids (engine cfg track): the streams' id queues are the rows of ONE (B, L) tensor and their counters of ONE (B, 1), so that
        # a single far3d_track_update launch reaches all of them; stream b's mem["track"] is its row, zeroed with the rest of its memory
        self._track = None
        if engine.track is not None:
            self._track = (torch.zeros((self.streams, engine.cfg["memory_len"]), dtype=torch.int64, device=engine.dev),
                           torch.ones((self.streams, 1), dtype=torch.int64, device=engine.dev))
            if "track_hits" in engine.mem:      # track records: one more plane beside the ids, a row per stream
                self._track += (torch.zeros((self.streams, engine.cfg["memory_len"]), dtype=torch.int32, device=engine.dev),)
            for b, st in enumerate(self._state):
                st["mem"]["track"] = self._track[0][b:b + 1]
                if len(self._track) > 2:
                    st["mem"]["track_hits"] = self._track[2][b:b + 1]
        self._tokens = None         # (B, N, S, 256): stream b's camera stage writes slice b, the decoder pass reads all of it
        self._images = None         # (B * N, 3, H, W): stream b stages its images in rows [b * N, (b + 1) * N) (camera_batch)
        for b in range(self.streams):
            engine._ins.pop(self._key(b), None)      # staged inputs of an earlier runner whose id() this one has: slices of ITS buffer
            engine.token_slices[self._key(b)] = functools.partial(self._token_slice, b)
            if self.camera_batch:
                engine.image_slices[self._key(b)] = functools.partial(self._image_slice, b)
            else:
                engine.image_slices.pop(self._key(b), None)

    def _key(self, b):
        return ("stream", id(self), b)

    def _token_slice(self, b, N, S, dtype):
        t = self._tokens
        if t is None or tuple(t.shape) != (self.streams, N, S, 256) or t.dtype != dtype:
            t = self._tokens = torch.empty((self.streams, N, S, 256), dtype=dtype, device=self.engine.dev)
        return t[b]

    def _pass_tokens(self, b0, b1, n, S, dtype):
        """The token buffer of the camera pass over streams [b0, b1): their slices of the one allocation, as (images, S, 256)."""
        N = n // (b1 - b0)
        self._token_slice(b0, N, S, dtype)
        return self._tokens[b0:b1].view(n, S, 256)

    def _image_slice(self, b, shape):
        N, t = shape[0], self._images
        if t is None or tuple(t.shape) != (self.streams * N,) + tuple(shape[1:]):
            t = self._images = torch.empty((self.streams * N,) + tuple(shape[1:]), dtype=torch.float32, device=self.engine.dev)
        return t[b * N:(b + 1) * N]

    @contextlib.contextmanager
    def _stream(self, b):
        """The engine as stream b sees it: its buffer set, its streaming memory, its scene."""
        e, s = self.engine, self._state[b]
        keep = (e.mem, e.prev_scene, e._mem_valid)
        e.mem, e.prev_scene, e._mem_valid = s["mem"], s["prev_scene"], s["mem_valid"]
        if self._track is not None:
            keep_next, e._track_next = e._track_next, self._track[1][b:b + 1]
        try:
            with e.buffers(self._key(b)):
                yield
        finally:
            s["prev_scene"], s["mem_valid"] = e.prev_scene, e._mem_valid
            e.mem, e.prev_scene, e._mem_valid = keep
            if self._track is not None:
                e._track_next = keep_next

    def reset_memory(self, b=None):
        """Forget the streaming memory of stream b (None: of every stream): its next frame is the first of a scene."""
        for i in (range(self.streams) if b is None else [int(b)]):
            self._state[i]["prev_scene"], self._state[i]["mem_valid"] = None, False

    def reset_tracks(self, b=None):
        """Far3DEngine.reset_tracks for stream b (None: every stream): its ids start at 1 again and its memory is forgotten."""
        if self._track is None:
            raise ValueError("reset_tracks: tracking is off (engine cfg track=None)")
        for i in (range(self.streams) if b is None else [int(b)]):
            self._track[1][i].fill_(1)
        self.reset_memory(b)

    def memory(self, b):
        """Stream b's streaming memory (the dict of Far3DEngine.mem)."""
        return self._state[b]["mem"]

    def check_proposal_overflow(self):
        """Far3DEngine.check_proposal_overflow for the latest forward_frames call: raise, naming the streams, if a stream's frame had
        more proposals than rows (or a camera filled its selection capacity).  One sync for all streams; the per-stream flags stay in
        the outputs (proposal_overflow)."""
        flags = [(b, f) for b, f in enumerate(self._overflow) if f is not None]
        if not flags:
            return
        over = [b for (b, _), v in zip(flags, torch.stack([f.view(-1)[0] for _, f in flags]).tolist()) if v != 0]
        if over:
            cfg = self.engine.cfg
            raise _lib.Far3dHipError("proposal capacity exceeded in streams %s: more than proposal_capacity=%s proposals (multi_depth_capacity=%s "
                                     "extra rows) in the frame, or a camera reached proposal_cap=%s; raise them" %
                                     (over, cfg.get("proposal_capacity"), cfg.get("multi_depth_capacity"), cfg["proposal_cap"]))

    def _camera_streams(self, dds, pad_hw):
        """The camera stage of all streams in as few passes as the kernels' extents allow -> the B per-stream `st` dicts."""
        e, B = self.engine, self.streams
        img = dds[0]["img"]
        N = img.shape[0]
        if any(tuple(dd["img"].shape) != tuple(img.shape) for dd in dds):
            raise ValueError("forward_frames: every stream's frame must have the same cameras and image size")
        if self._images is None or any(dd["img"].data_ptr() != self._images[b * N].data_ptr() for b, dd in enumerate(dds)):
            raise RuntimeError("StreamBatch: a stream's staged images are not its slice of the joint image buffer")
        self.camera_chunks = stream_chunks(B, N, e.camera_image_span(img.shape[2], img.shape[3]), max_streams=self.max_camera_streams)
        sts, b0 = [], 0
        for nb in self.camera_chunks:
            b1 = b0 + nb
            key = ("streams_cam", id(self), b0, b1)
            e.token_slices[key] = functools.partial(self._pass_tokens, b0, b1)
            sts += e.camera_stage_streams(dds[b0:b1], pad_hw, key, self._images[b0 * N:b1 * N],
                                          stream_keys=[self._key(b) for b in range(b0, b1)] if self.hole_rows else None)
            b0 = b1
        return sts

    @torch.no_grad()
    def forward_frames(self, datas, img_metas_list):
        """One frame per stream: datas[b] / img_metas_list[b] as Far3DEngine.forward_frame takes them (same image size and camera count
        in every stream).  Returns a list of B output dicts with forward_frame's keys.  Outputs live in buffers of the stream's own
        set, or of the batch, that the next call overwrites: clone what must outlive it."""
        e, B = self.engine, self.streams
        if len(datas) != B or len(img_metas_list) != B:
            raise ValueError("forward_frames: one frame per stream (%d), got %d / %d" % (B, len(datas), len(img_metas_list)))
        why = _refusal(e, self.hole_rows)          # the options are attributes: they may have been set since the constructor looked
        if why is not None:
            raise ValueError("StreamBatch: " + why)
        pad_hw = tuple(img_metas_list[0][0]["pad_shape"][0][:2])
        if any(tuple(m[0]["pad_shape"][0][:2]) != pad_hw for m in img_metas_list):
            raise ValueError("forward_frames: every stream's frame must have the same padded size")
        cfg = e.cfg
        with ops.use_tile_tables(e.bf16_tile_table()):
            sts, hss, dds, rows = [], [], [], []
            if self.camera_batch:
                for b in range(B):
                    with self._stream(b):
                        dds.append(e._stage_inputs(datas[b]))
                sts = self._camera_streams(dds, pad_hw)
            for b in range(B):
                with self._stream(b):
                    if not self.camera_batch:
                        dds.append(e._stage_inputs(datas[b]))
                        sts.append(e._camera_part(dds[b], pad_hw))
                    dd, st = dds[b], sts[b]
                    M, Mb, m_dev = e._head_rows(st, dd["img"].shape[0])      # static modes (_refusal): no sync
                    rows.append(Mb)
                    hss.append(e._head_prepare(st["tokens"], st["ref2d"], st["ctx"], M, dd, img_metas_list[b], m_dev))
            pick = lambda name: [getattr(hs, name) for hs in hss]
            outs_dec = e.decoder_streams(pick("X2"), pick("x0"), pick("qpos"), pick("tokens"), pick("ref"), sts[0]["hw"], sts[0]["starts"],
                                         pick("lidar2img"), pad_hw, hss[0].A, holes=pick("hole"))
            if self.head_batch:
                res = e._head_finish_streams(hss, outs_dec, self._stream, track=self._track)
            else:
                res = []
                for b, hs in enumerate(hss):
                    with self._stream(b):
                        # the heads read a stream's layers as ONE (layers * A, E) block: the stream's rows of the pass, gathered
                        od = e._buf(("outs_dec",), (len(e.layers), hs.A, cfg["embed_dims"]), torch.float32)
                        od.copy_(outs_dec[b])
                        res.append(e._head_finish(hs, od))
            for st, Mb, outs in zip(sts, rows, res):
                e._head_outputs(outs, st, Mb)
            self._overflow = [st["overflow"] for st in sts]
        return res

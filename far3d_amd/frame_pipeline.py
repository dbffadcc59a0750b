"""The two-stream software pipeline of consecutive frames, ONE implementation for the runners that replay a frame as a camera half
and a head half: Far3DEngine.pipeline (one GPU) and dist.ShardedFrame (camera-sharded ranks).  ShardedFrame's unpipelined graph mode
keeps its graphs in the same slots, under the same staleness rule, without the streams.

Stream s_cam (one of `s_cams`, round-robin): [wait until the head that last used this buffer set is done] -> input staging -> camera
replayable -> the owner's "after camera" hook (the sharded runner's exchange).  Stream s_head: [wait for s_cam, and for the hook's work
handles] -> head replayable.  The heads are ordered on one stream, so the streaming-memory updates stay sequential and the results are
bit-identical to the unpipelined run.  The buffer set of a frame is the engine's current one (`engine._par`, set by the caller).
What is captured, and how, stays with the owner, who hands in capture(dd, img_metas, pad_hw) -> (camera replayable | None, head
replayable, outputs, anything to keep alive and hand to the hook), called with the device quiet, on the staged inputs `dd`.
"""
import weakref

import torch


class FramePipeline:
    def __init__(self, engine):
        self.eng = weakref.proxy(engine)      # no cycle: whoever owns a pipeline owns, or is, the engine, whose last reference frees its buffers
        self.slots = {}         # buffer set -> dict(ins, cam, head, outs, keep, cam_done, head_done); absent = never captured / dropped
        self.streams = None     # dict(s_cams, s_head, n_issued) from the first pipelined frame on; NEVER dropped: drain() needs them

    # `runner._pipe` reads as it always did: falsy until the first pipelined frame, then _pipe["s_cams"] / _pipe["s_head"]; and the
    # read accessor _pipe["g_cam"] / _pipe["g_head"] -> {buffer set that holds captured graphs: its camera / head replayable}
    def __bool__(self):
        return self.streams is not None

    def __getitem__(self, key):
        return {p: s[key[2:]] for p, s in self.slots.items()} if key in ("g_cam", "g_head") else self.streams[key]

    # ------------------------------------------------------------------------------------------ the one staleness rule
    def drop(self, p):
        """Forget buffer set p's graphs, after waiting for any replay of them in flight: the owner re-allocated buffers they read."""
        if p in self.slots:
            torch.cuda.synchronize(self.eng.dev)
            del self.slots[p]

    def slot(self, capture, data, img_metas, pad_hw):
        """-> (the current buffer set's slot, was it captured just now).  It is captured, with the device quiet before and after, if it
        never was, or was dropped, or its graphs bake the addresses of staged inputs that are gone: the engine has re-allocated them
        since (another resolution or camera count came by), or this frame's shape will make it do so.  All of that is the same
        on every rank (frame sequence, input shapes, buffer-set index): the sharded capture holds an eager collective."""
        eng = self.eng
        p, img = eng._par, data["img"]
        slot, shape = self.slots.get(p), tuple(img.shape[1:] if img.dim() == 5 else img.shape)
        if slot is not None and slot["ins"] is eng._ins.get(p) and tuple(slot["ins"]["img"].shape) == shape:
            return slot, False
        torch.cuda.synchronize(eng.dev)
        self.slots.pop(p, None)
        dd = eng._stage_inputs(data)
        if (p, "tq") not in eng._bufs:      # the query-major buffers and their constant rows exist before the capture
            eng._alloc_query_buffers(dd["img"].shape[0])
        cam, head, outs, keep = capture(dd, img_metas, pad_hw)
        self.slots[p] = dict(ins=dd, cam=cam, head=head, outs=outs, keep=keep, cam_done=torch.cuda.Event(), head_done=torch.cuda.Event())
        torch.cuda.synchronize(eng.dev)
        return self.slots[p], True

    # ------------------------------------------------------------------------------------------ frames
    def frame(self, capture, data, img_metas, pad_hw, after_camera=None):
        """One steady-state frame, pipelined.  after_camera(buffer set, the slot's `keep`) -> work handles the head stream waits for.
        Outputs are ready on output_stream() (engine.wait_outputs())."""
        eng = self.eng
        if self.streams is None:
            # the camera stages are the throughput-critical half: their streams get the higher priority so that the head of the
            # previous frame (latency-bound, few CUs) does not delay their workgroups (engine.cam_priority, A/B in bench.py)
            # pipeline_sets >= 3: two camera-stage streams.  A frame's per-camera stages are ~215 dependent launches, many of them one
            # or two rounds of workgroups (stages 4-5, FPN, 2D head); the stages of the NEXT frame on a second stream fill their tails:
            # two camera graphs take 4.66 ms per frame side by side against 5.62 ms back to back (profiles/r4/cam_overlap.txt)
            ncs = max(1, min(int(eng.pipeline_sets) - 1, int(eng.cam_streams)))
            self.streams = dict(s_cams=[torch.cuda.Stream(eng.dev, priority=eng.cam_priority) for _ in range(ncs)],
                                s_head=torch.cuda.Stream(eng.dev), n_issued=0)
        S = self.streams
        here = torch.cuda.Event()
        here.record(torch.cuda.current_stream(eng.dev))     # the caller's stream up to this call: inputs, eager scene starts
        slot, first = self.slot(capture, data, img_metas, pad_hw)    # stale graphs go BEFORE the decision to replay
        s_cam = S["s_cams"][S["n_issued"] % len(S["s_cams"])]      # consecutive frames alternate between the camera streams
        S["n_issued"] += 1
        s_cam.wait_event(here)
        for v in data.values():                             # the caller may free its input tensors right after this call
            if isinstance(v, torch.Tensor) and v.is_cuda:
                v.record_stream(s_cam)
        with torch.cuda.stream(s_cam):
            if not first:
                s_cam.wait_event(slot["head_done"])         # the head that last read this set (inputs, exchange buffers); none after a capture
            eng._stage_inputs(data)
            if slot["cam"] is not None:                     # an idle rank has no camera graph
                slot["cam"].replay()
            works = after_camera(eng._par, slot["keep"]) if after_camera is not None else ()
            slot["cam_done"].record(s_cam)
        with torch.cuda.stream(S["s_head"]):
            S["s_head"].wait_event(here)
            S["s_head"].wait_event(slot["cam_done"])
            for w in works:
                w.wait()                                    # stream-ordered on the RCCL backend: s_head waits, the host does not
            slot["head"].replay()
            slot["head_done"].record(S["s_head"])
        eng._ready = slot["head_done"]
        # the overflow flag this frame writes lives in ITS buffer set: bind it per frame (the replayed graph never runs the Python
        # line that recorded it at capture time)
        eng._overflow = slot["outs"].get("proposal_overflow")
        return slot["outs"]

    def drain(self):
        """Order the caller's stream after everything in flight: a scene start runs on it, eagerly, and its outputs are that stream's."""
        if self.streams is not None:
            cur = torch.cuda.current_stream(self.eng.dev)
            for sc in self.streams["s_cams"]:
                cur.wait_stream(sc)
            cur.wait_stream(self.streams["s_head"])
        self.eng._ready = None

    def output_stream(self):
        """The stream the latest frame's outputs are produced on."""
        pipelined = self.streams is not None and self.eng._ready is not None
        return self.streams["s_head"] if pipelined else torch.cuda.current_stream(self.eng.dev)

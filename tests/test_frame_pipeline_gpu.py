"""GPU: the paths of far3d_amd.frame_pipeline.FramePipeline that Far3DEngine.pipeline and dist.ShardedFrame share and that the
sequences of the other suites never reach: an input shape that changes while frames are pipelined (every buffer set's graphs are
stale and are captured again), on the engine and on the sharded runner (where the exchange buffers change with it), and a scene
start that arrives while every buffer set is in flight on two camera streams.  At the golden toy size (2 cameras, 64 x 96), against
the eager engine, bit for bit.  These pin behaviour the pipeline already had before it became one implementation."""
import os
import queue
import socket

import pytest
import torch

from far3d_amd import synth
from tests.test_engine_gpu import _golden_engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(64, 96), (96, 128), (64, 96)]     # the golden size, one with other FPN level shapes on every level, and back


def _resize_sequence(per_size):
    """`per_size` frames of ONE scene at each of SIZES in turn (frame 0 is the scene start), timestamps and ego poses running on."""
    return [synth.make_frame(2, hw, seed=5, frame_index=k * per_size + i, ego_motion=True)
            for k, hw in enumerate(SIZES) for i in range(per_size)]


def _state(o, eng):
    return [o["all_cls_scores"].clone(), o["all_bbox_preds"].clone()] + [eng.mem[k].clone() for k in sorted(eng.mem)]


def _heads(graphs, sets):
    """The head replayable of every buffer set in `graphs` ({buffer set: replayable}), which must be all `sets` of them."""
    assert sorted(graphs) == list(range(sets))
    return [graphs[p] for p in range(sets)]


def _run_resizes(eng, runner, per_size, head_graphs=None):
    """The resize sequence through `runner` (waiting for every frame's outputs) -> per-frame states; checks on the way that each
    size captured every buffer set anew (head_graphs() -> the runner's {buffer set: head replayable})."""
    out, heads = [], []
    for fi, (data, metas) in enumerate(_resize_sequence(per_size)):
        o = runner.forward_frame(data, metas)
        runner.wait_outputs()
        out.append(_state(o, eng))
        if head_graphs is not None and (fi + 1) % per_size == 0:
            now = _heads(head_graphs(), eng.pipeline_sets)
            assert all(a is not b for a, b in zip(now, heads)), "size %s: a buffer set kept the graphs of the size before" % (SIZES[fi // per_size],)
            heads = now
    return out


def test_input_shape_change_inside_the_pipeline_is_bitwise_eager(hip_lib):
    res = {}
    for mode in ("eager", "pipeline"):
        eng, _, _ = _golden_engine("fp32", proposal_topk=12)
        eng.use_graph = eng.pipeline = mode == "pipeline"
        res[mode] = _run_resizes(eng, eng, eng.pipeline_sets + 2, (lambda: eng._pipe["g_head"]) if eng.pipeline else None)
    for fi, (a, b) in enumerate(zip(res["eager"], res["pipeline"])):
        assert torch.isfinite(a[0]).all()
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "frame %d: the pipeline differs from eager" % fi


def _sharded_worker(port, q):
    import torch.distributed as dist
    from far3d_amd import dist as fdist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 8) // 2)))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        ref, _, _ = _golden_engine("fp32", proposal_topk=12)
        eng, _, _ = _golden_engine("fp32", proposal_topk=12)
        runner = fdist.ShardedFrame(eng, use_graph=True, pipeline=True)
        assert runner.pipeline
        want = _run_resizes(ref, ref, eng.pipeline_sets + 2)
        got = _run_resizes(eng, runner, eng.pipeline_sets + 2, lambda: runner._g_head)
        q.put([fi for fi, (a, b) in enumerate(zip(want, got)) if not all(torch.equal(x, y) for x, y in zip(a, b))])
    finally:
        dist.destroy_process_group()


def test_input_shape_change_inside_the_sharded_pipeline_is_bitwise_eager(hip_lib):
    """World 1 over gloo: the staged inputs AND the exchange buffers of every buffer set are re-allocated at each size change."""
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_sharded_worker, args=(port, q))
    p.start()
    try:
        for _ in range(60):
            try:
                differing = q.get(timeout=5)
                break
            except queue.Empty:      # a child that died is reported now, not when the time runs out
                assert p.is_alive(), "the child ended without a result (exit code %s)" % p.exitcode
    finally:
        p.join(timeout=30)
        if p.is_alive():
            p.terminate()
    assert differing == [], "frames whose logits, boxes or streaming memory differ from the eager engine: %s" % differing


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_scene_start_drains_three_buffer_sets_in_flight(hip_lib, precision):
    """test_engine_gpu.py::test_pipelined_frames_in_flight_end_in_the_same_state with three buffer sets on two camera streams: scene
    A x (sets + 2) so that every set has captured and one has replayed, then scene B x 2 with no wait anywhere -- the eager scene
    start must wait for both camera streams and the head stream."""
    fin = {}
    for mode in ("eager", "pipeline"):
        eng, z, rc = _golden_engine(precision, proposal_topk=12)
        eng.use_graph = eng.pipeline = mode == "pipeline"
        eng.pipeline_sets = 3
        frames = [synth.recipe_frame(rc, fi, device=DEV) for fi in range(rc["frames"])]
        for fi in [0] + [1] * (eng.pipeline_sets + 1) + [2, 3]:
            o = eng.forward_frame(*frames[fi])
        torch.cuda.synchronize()
        if mode == "pipeline":
            assert len(eng._pipe["s_cams"]) == 2 and len(_heads(eng._pipe["g_head"], 3)) == 3
        fin[mode] = _state(o, eng) + [o["result"][k].clone() for k in sorted(o["result"])]
    assert all(torch.equal(a, b) for a, b in zip(fin["eager"], fin["pipeline"]))

"""GPU: multi-depth proposals on the camera-sharded runner (dist.ShardedFrame(multi_depth=True)) end to end.  As in
tests/test_dist_gpu.py the ranks share cuda:0 over gloo (collectives staged through the host); each packs its camera block into ONE
record (far3d_proposal_pack_block), the records are gathered, and every rank's head merges them (merge_camera_blocks) and must
reproduce the single-rank engine on the multi-depth golden sequence: same proposals, same records, same M', logits and boxes within the
bound of tests/test_dist_gpu.py / tests/test_camera_blocks_gpu.py, every rank bit-identical to rank 0.  At most 3 ranks + this process
hold the GPU."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NAME = "far3d_md2_seq"


def _frame_ids(rc, frames):
    """Golden frames (through the scene change), then the last one repeated: steady frames for the graphs and the pipeline's buffer sets."""
    return [min(fi, rc["frames"] - 1) for fi in range(frames)]


def _record(o, P):
    """What the comparison needs of one frame's outputs, on the host."""
    sel = o["sel_cnt"].cpu().numpy()
    Mp = min(int(sel.sum()), P)
    return dict(cls=o["all_cls_scores"].cpu().numpy(), box=o["all_bbox_preds"].cpu().numpy(), sel_cnt=sel, m=int(o["num_adaptive_dev"].item()),
                rows=int(o["num_adaptive"]), flags=o["md_records"][0][:Mp].cpu().numpy(), info=o["md_records"][1][:Mp].cpu().numpy(),
                box2d=o["bbox2d"][:Mp].cpu().numpy(), score2d=o["bbox2d_scores"][:Mp].cpu().numpy(), overflow=int(o["proposal_overflow"].item()))


def _primary_rows(rc, mode):
    return mode["proposal_capacity"] if "proposal_capacity" in mode else rc["num_cams"] * mode["proposal_topk"]


def _worker(rank, world, port, q, mode, use_graph, pipeline, frames, decoders):
    import torch.distributed as dist
    from far3d_amd import synth
    from far3d_amd import dist as fdist
    from tests.test_multidepth_gpu import _md_engine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    # every rank builds an engine on the host: without a cap each spawns a thread per core and the builds slow each other down
    torch.set_num_threads(max(1, min(16, (os.cpu_count() or 8) // (2 * world))))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng, z, rc = _md_engine(NAME, **mode)
        P = _primary_rows(rc, mode)
        try:
            fdist.ShardedFrame(eng)
            refused = False
        except ValueError as e:
            refused = ("topk=%d" % eng.md_k) in str(e) and "multi_depth=True" in str(e)
        res = {}
        for dec in decoders:
            eng.reset_memory()
            runner = fdist.ShardedFrame(eng, use_graph=use_graph, pipeline=pipeline, decoder=dec, multi_depth=True)
            assert runner.md and len(runner.cams) == (1 if rank < rc["num_cams"] else 0)
            outs = []
            for fi in _frame_ids(rc, frames):
                data, metas = synth.recipe_frame(rc, fi)
                o = runner.forward_frame(data, metas)
                runner.wait_outputs()
                torch.cuda.synchronize()
                eng.check_proposal_overflow()
                outs.append((_record(o, P), o["outs_dec"].clone(), {k: v.clone() for k, v in eng.mem.items()}))
            if pipeline:
                assert sorted(runner._g_head) == list(range(eng.pipeline_sets))
            res[dec] = outs
        same = True
        if len(decoders) == 2:                                      # the query-sharded decoder against the replicated one, bit for bit
            assert runner.qshard is not None and runner.qshard.world == world
            for a, b in zip(res[decoders[0]], res[decoders[1]]):
                same = same and all(np.array_equal(a[0][k], b[0][k]) for k in ("cls", "sel_cnt", "flags", "info")) and a[0]["m"] == b[0]["m"]
                same = same and torch.equal(a[1], b[1]) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
        q.put((rank, refused, bool(same), [o[0] for o in res[decoders[-1]]]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _valid(t, nq, m, rows):
    """Drop the hole rows [nq + m, nq + rows) of the query axis (tests/test_capacity_gpu.py _valid_rows, on the host)."""
    return np.concatenate([t[:, :, :nq + m], t[:, :, nq + rows:]], axis=2)


CASES = [
    (2, dict(proposal_topk=16), True, True, 9, ("replicated",)),
    (3, dict(proposal_capacity=48), False, False, 3, ("replicated",)),                    # rank 2 is idle: it packs the empty block
    (2, dict(proposal_capacity=48), True, False, 5, ("replicated", "query_sharded")),
]


@pytest.mark.parametrize("world,mode,use_graph,pipeline,frames,decoders", CASES,
                         ids=["w2-topk-graph-pipeline", "w3-capacity-eager-idle-rank", "w2-capacity-graph-query-sharded"])
def test_sharded_multi_depth_ranks_match_single_rank(hip_lib, world, mode, use_graph, pipeline, frames, decoders):
    import torch.multiprocessing as mp
    from far3d_amd import synth
    from tests.test_multidepth_gpu import _md_engine
    eng, z, rc = _md_engine(NAME, **mode)
    P, nq = _primary_rows(rc, mode), rc["num_query"]
    want = []
    for fi in _frame_ids(rc, frames):
        data, metas = synth.recipe_frame(rc, fi)
        o = eng.forward_frame(data, metas)
        torch.cuda.synchronize()
        eng.check_proposal_overflow()
        want.append(_record(o, P))
    del eng
    torch.cuda.empty_cache()
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, mode, use_graph, pipeline, frames, decoders)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = {r[0]: r for r in (q.get(timeout=150 * world) for _ in procs)}
    finally:
        for p in procs:
            p.join(timeout=20)
            if p.is_alive():
                p.terminate()
    assert sorted(res) == list(range(world))
    for r in range(world):
        assert res[r][1], "rank %d: ShardedFrame(engine) without multi_depth=True must still refuse topk > 1, naming the keyword" % r
        assert res[r][2], "rank %d: query-sharded decoder differs from the replicated decoder" % r
        for fi in range(frames):
            g, w = res[r][3][fi], want[fi]
            what = "rank %d frame %d" % (r, fi)
            assert np.array_equal(g["sel_cnt"], w["sel_cnt"]) and g["m"] == w["m"] and g["rows"] == w["rows"] and g["overflow"] == 0, what
            assert g["m"] > int(w["sel_cnt"].sum()) > 0, what + ": the fixture must produce extra rows"
            for k in ("flags", "info"):
                assert np.array_equal(g[k], w[k]), "%s: %s" % (what, k)
            for k in ("box2d", "score2d"):                          # the primaries' 2D boxes (the bound test_multidepth_gpu.py puts on them)
                assert g[k].shape == w[k].shape and np.allclose(g[k], w[k], rtol=2e-3, atol=2e-3), "%s: %s" % (what, k)
            for k in ("cls", "box"):
                a, b = _valid(g[k], nq, g["m"], g["rows"]), _valid(w[k], nq, w["m"], w["rows"])
                assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all(), what
                tol = 1e-3 * max(1.0, np.abs(b).max() / 10.0)
                err = np.abs(a - b).max()
                print("%s %s: max abs difference %.3e (bound %.3e)" % (what, k, err, tol))
                assert err < tol, "%s %s: %.3e" % (what, k, err)
    # the replicated head is deterministic: every rank holds the same results, bit for bit
    for fi in range(frames):
        for r in range(1, world):
            assert np.array_equal(res[0][3][fi]["cls"], res[r][3][fi]["cls"])
            assert np.array_equal(_valid(res[0][3][fi]["box"], nq, want[fi]["m"], want[fi]["rows"]),
                                  _valid(res[r][3][fi]["box"], nq, want[fi]["m"], want[fi]["rows"]))

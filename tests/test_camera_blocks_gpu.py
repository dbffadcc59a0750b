"""GPU: proposals from camera blocks above the kernel -- Far3DEngine.merge_camera_blocks and latency.CameraGroupFrame in the
fixed-capacity threshold mode and with multi-depth proposals, against the plain engine on the golden toy sequences (two cameras, one per
block), through their scene change.  The bound on logits and boxes is that of tests/test_latency_gpu.py: the same kernels on the same
per-camera data, but a layer whose tile-table entry depends on the pixel count may take another tile for one camera than for two."""
import numpy as np
import pytest
import torch

from far3d_amd import synth
from tests.test_capacity_gpu import _valid_rows
from tests.test_multidepth_gpu import _md_engine

pytestmark = pytest.mark.gpu


def _close(a, b, key, nq, what, precision="fp32"):
    """Logits / boxes of two runs with equal M' on the device: the rows of the hole (-inf logits by construction) are left out."""
    Ma, Mb = a["num_adaptive_dev"], b["num_adaptive_dev"]
    assert a["num_adaptive"] == b["num_adaptive"]
    w, g = a[key], b[key]
    if Ma is not None:
        assert int(Ma.item()) == int(Mb.item()), "%s: M' %d, plain engine %d" % (what, int(Mb.item()), int(Ma.item()))
        w, g = (_valid_rows(t, 2, nq, int(Ma.item()), a["num_adaptive"]) for t in (w, g))
    w, g = w.cpu().numpy(), g.cpu().numpy()
    assert g.shape == w.shape and np.isfinite(g).all() and np.isfinite(w).all(), what
    tol = (1e-3 if precision in ("fp32", "bf16x3") else 8e-2) * max(1.0, np.abs(w).max() / 10.0)
    err = np.abs(g - w).max()
    print("%s %s: max abs difference %.3e (bound %.3e)" % (what, key, err, tol))
    assert err < tol, "%s %s: %.3e" % (what, key, err)


def _same_records(a, b, sel_cnt, P, what):
    Mp = min(int(sel_cnt.sum().item()), P)
    assert Mp > 0
    for x, y in zip(a, b):
        assert torch.equal(x[:Mp], y[:Mp]), what


@pytest.mark.parametrize("mode", [dict(proposal_capacity=48), dict(proposal_topk=16)], ids=["capacity", "topk"])
def test_engine_camera_blocks_then_merge_equal_forward_frame(hip_lib, mode):
    """camera_stage per block (block_rows) + merge_camera_blocks + head_stage against forward_frame, multi_depth topk = 2."""
    ref, z, rc = _md_engine("far3d_md2_seq", **mode)
    eng, _, _ = _md_engine("far3d_md2_seq", **mode)
    N, nq = rc["num_cams"], rc["num_query"]
    P = 48 if "proposal_capacity" in mode else N * 16
    with torch.no_grad():
        for fi in range(3):                                         # frame 2 starts a new scene
            data, metas = synth.recipe_frame(rc, fi)
            a = ref.forward_frame(data, metas)
            pad_hw = tuple(metas[0]["pad_shape"][0][:2])
            dd = eng._stage_inputs(data)
            sts = []
            for c in range(N):
                with eng.buffers(("block", c)):
                    sts.append(eng.camera_stage(dd["img"][c:c + 1], dd, range(c, c + 1), pad_hw, block_rows=eng.camera_block_rows(1)))
                assert sts[-1]["ctx"].shape[0] == eng.camera_block_rows(1) and sts[-1]["cams"] == (c, c + 1)
            st = eng.merge_camera_blocks(sts)
            assert st["rows"] == eng.static_adaptive_rows() == 2 * P
            b = eng.head_stage(torch.cat([s["tokens"] for s in sts]), st["ref2d"], st["ctx"], st["rows"], dd, metas, sts[0]["hw"],
                               sts[0]["starts"], pad_hw, m_dev=st["m_dev"])
            torch.cuda.synchronize()
            ref.check_proposal_overflow()
            eng.check_proposal_overflow()
            assert torch.equal(a["sel_cnt"], st["sel_cnt"])
            assert int(a["num_adaptive_dev"].item()) == int(b["num_adaptive_dev"].item()) > int(st["sel_cnt"].sum().item())   # extras exist
            _same_records(a["md_records"], st["md_records"], st["sel_cnt"], P, "frame %d" % fi)
            for key in ("all_cls_scores", "all_bbox_preds"):
                _close(a, b, key, nq, "frame %d" % fi)


def test_engine_camera_blocks_need_a_static_mode_and_their_own_row_count(hip_lib):
    eng, z, rc = _md_engine("far3d_md2_seq")                        # legacy threshold mode
    with pytest.raises(ValueError, match="static proposal mode"):
        eng.camera_block_rows(1)
    with pytest.raises(ValueError, match="static proposal mode"):
        eng.merge_camera_blocks([])
    eng, z, rc = _md_engine("far3d_md2_seq", proposal_topk=16)      # top-K: a block of one camera has 16 rows, nothing else
    assert eng.camera_block_rows(1) == 16
    data, metas = synth.recipe_frame(rc, 0)
    with torch.no_grad():
        dd = eng._stage_inputs(data)
        with eng.buffers(("block", 0)), pytest.raises(ValueError, match="block_rows"):
            eng.camera_stage(dd["img"][:1], dd, range(1), tuple(metas[0]["pad_shape"][0][:2]), block_rows=17)


CASES = [
    ("far3d_md2_seq", dict(proposal_topk=16), "fp32", False),
    ("far3d_md2_seq", dict(proposal_topk=16), "fp32", True),
    ("far3d_md3_seq", dict(proposal_topk=16), "fp32", False),
    ("far3d_md3_seq", dict(proposal_topk=16), "fp32", True),
    ("far3d_md2_seq", dict(proposal_capacity=48), "fp32", False),
    ("far3d_md2_seq", dict(proposal_capacity=48), "fp32", True),
    ("far3d_md3_seq", dict(proposal_capacity=48), "fp32", False),
    ("far3d_md3_seq", dict(proposal_capacity=48), "fp32", True),
    ("far3d_small_seq", dict(proposal_capacity=48), "fp32", False),
    ("far3d_small_seq", dict(proposal_capacity=48), "fp32", True),
    ("far3d_md2_seq", dict(proposal_topk=16), "bf16x3", True),
]


def _engines(name, precision, mode):
    if name == "far3d_small_seq":                                   # single depth
        from tests.test_engine_gpu import _golden_engine
        over = dict(mode, proposal_topk=None) if "proposal_capacity" in mode else mode
        return _golden_engine(precision, name, **over), _golden_engine(precision, name, **over)[0]
    return _md_engine(name, precision, **mode), _md_engine(name, precision, **mode)[0]


@pytest.mark.parametrize("name,mode,precision,use_graph", CASES,
                         ids=["%s-%s-%s-%s" % (n[6:-4], list(m)[0][9:], p, "graph" if g else "eager") for n, m, p, g in CASES])
def test_camera_groups_with_merged_proposals_reproduce_the_plain_engine(hip_lib, name, mode, precision, use_graph):
    from far3d_amd.latency import CameraGroupFrame
    (ref, z, rc), eng = _engines(name, precision, mode)
    run = CameraGroupFrame(eng, groups=2, use_graph=use_graph)
    assert run.merge and run.blocks == [(0, 1), (1, 2)]
    nq = rc["num_query"]
    frames = list(range(rc["frames"])) + [rc["frames"] - 1] * 3     # through the scene change (md2, small), then steady replays
    for fi in frames:
        data, metas = synth.recipe_frame(rc, fi)
        a, b = ref.forward_frame(data, metas), run.forward_frame(data, metas)
        torch.cuda.synchronize()
        ref.check_proposal_overflow()
        run.check_proposal_overflow()
        assert torch.equal(a["sel_cnt"], b["sel_cnt"])
        if eng.md_k > 1:
            P = 48 if "proposal_capacity" in mode else 32
            _same_records(a["md_records"], b["md_records"], b["sel_cnt"], P, "frame %d" % fi)
        for key in ("all_cls_scores", "all_bbox_preds"):
            _close(a, b, key, nq, "frame %d" % fi, precision)
        for k in ref.mem:
            d = (ref.mem[k].float() - eng.mem[k].float()).abs().max().item()
            assert d < 1e-3, (fi, k, d)
    if use_graph:
        assert run._g_head is not None and sorted(run._g_cam) == [0, 1]


@pytest.mark.parametrize("use_graph", [False, True])
def test_camera_groups_report_the_overflow_the_plain_engine_reports(hip_lib, use_graph):
    """proposal_capacity = 16 with 26-29 proposals per frame: both drop the same rows, and both say so."""
    from far3d_amd import lib
    from far3d_amd.latency import CameraGroupFrame
    (ref, z, rc), eng = _engines("far3d_md2_seq", "fp32", dict(proposal_capacity=16))
    run = CameraGroupFrame(eng, groups=2, use_graph=use_graph)
    for fi in (0, 1, 1):
        data, metas = synth.recipe_frame(rc, fi)
        a, b = ref.forward_frame(data, metas), run.forward_frame(data, metas)
        torch.cuda.synchronize()
        assert int(a["sel_cnt"].sum().item()) > 16
        with pytest.raises(lib.Far3dHipError, match="proposal capacity exceeded"):
            ref.check_proposal_overflow()
        with pytest.raises(lib.Far3dHipError, match="proposal capacity exceeded"):
            run.check_proposal_overflow()
        assert int(a["num_adaptive_dev"].item()) == int(b["num_adaptive_dev"].item())
        _same_records(a["md_records"], b["md_records"], b["sel_cnt"], 16, "frame %d" % fi)


def test_camera_groups_still_refuse_the_legacy_threshold_mode(hip_lib):
    from far3d_amd.latency import CameraGroupFrame
    eng, z, rc = _md_engine("far3d_md2_seq")
    with pytest.raises(ValueError, match="static proposal mode"):
        CameraGroupFrame(eng, groups=2)

"""GPU: far3d_proposal_merge_blocks (csrc/md_blocks.hip) -- the proposals of camera blocks packed into the frame's layout.

Reference: ONE proposal_gather_md + proposal_extra_rows (single depth: proposal_gather) over all three cameras.  Merged: the same
kernels per camera block on the sliced per-camera maps, into the block's own buffers, then the merge, then proposal_extra_rows.
Everything the reference wrote must come out bit for bit: the four row arrays over [0, M'), a zero hole, the records, the selection
counts, M' and the overflow flag.  3 cameras of 128 tokens (64 x 96 image) are the smallest frame with three ways to split it."""
import functools

import pytest
import torch

from tests.test_multidepth_gpu import DEPTH, DEV, PC, _bufs, _inputs

pytestmark = pytest.mark.gpu
N, HW, ND = 3, (64, 96), 51
SPLITS = [(2, 1), (1, 2), (1, 1, 1)]
# K -> (context width - 1, value-map dtype): 65-word rows (dword moves unless the row offset is a multiple of 4), bf16 value maps,
# 64-word rows (every run 16-byte aligned)
SHAPES = {2: (64, torch.float32), 3: (64, torch.bfloat16), 8: (63, torch.float32)}
# selections: 6 best per camera; score > 0.1 with 16 slots per camera (these maps fill them: the frame is flagged) and with a slot per
# token (every camera keeps its own number); 4 slots for the cases that are about the flag
SEL = {"topk": dict(sel_cap=6, topk=True), "thr": dict(sel_cap=16, topk=False), "thr_wide": dict(sel_cap=128, topk=False),
       "thr_full": dict(sel_cap=4, topk=False)}


def _blocks(split):
    lo, out = 0, []
    for n in split:
        out.append((lo, lo + n))
        lo += n
    return out


@functools.lru_cache(maxsize=None)
def _case(sel, K, empty_cam=None):
    """Inputs of a case (shared, never modified).  empty_cam: that camera's class logits are -20, so the threshold keeps none of it."""
    from far3d_amd import ops
    C, dt = SHAPES[K]
    seed = 11 + K
    x = _inputs(N, HW, ND, C, dt, seed=seed, sel_cap=SEL[sel]["sel_cap"], topk=SEL[sel]["topk"])
    if empty_cam is not None:
        g = torch.Generator().manual_seed(seed)                     # _inputs draws the class maps first
        cls = [torch.randn((N, r.shape[1], r.shape[2], 26), generator=g).to(DEV) for r in x["reg"]]
        for c in cls:
            c[empty_cam] = -20.0
        x["wgt"], x["sel_idx"], x["sel_cnt"] = ops.proposal_select(cls, x["reg"], x["strides"], SEL[sel]["sel_cap"], thr=0.1, topk=SEL[sel]["topk"])
    x["cnt"] = x["sel_cnt"].cpu().tolist()
    return x


def _slice(x, lo, hi):
    return dict(reg=[r[lo:hi] for r in x["reg"]], sel_idx=x["sel_idx"][lo:hi], sel_cnt=x["sel_cnt"][lo:hi], wgt=x["wgt"][lo:hi],
                dl=x["dl"][lo:hi], feat=x["feat"][lo:hi], i2l=x["i2l"][lo:hi])


def _scalars():
    return torch.full((1,), -1, dtype=torch.int32, device=DEV), torch.full((1,), -1, dtype=torch.int32, device=DEV)


def _records(P, K):
    return torch.zeros((P,), dtype=torch.int32, device=DEV), torch.zeros((P, 2 * K), dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def _reference_md(sel, K, empty_cam, rmb, P, rows_total):
    """All cameras at once; computed once per (inputs, sizes) and shared by the splits."""
    from far3d_amd import ops
    x = _case(sel, K, empty_cam)
    cap = x["sel_idx"].shape[1]
    out, rec = _bufs(rows_total, x["C"]), _records(P, K)
    m, ovf = _scalars()
    ops.proposal_gather_md(x["reg"], x["strides"], x["sel_idx"], x["sel_cnt"], x["wgt"], x["dl"], DEPTH["stride"], DEPTH, x["i2l"], x["feat"],
                           PC, K, rmb, rec, out, primary_rows=P)
    ops.proposal_extra_rows(x["sel_cnt"], 0 if SEL[sel]["topk"] else cap, P, K, rec, x["i2l"], DEPTH, PC, out, fill_hole=True, m_out=m,
                            overflow_out=ovf)
    torch.cuda.synchronize()
    return out, rec, int(m.item()), int(ovf.item())


def _merged_md(sel, K, empty_cam, rmb, P, rows_total, split):
    from far3d_amd import ops
    x = _case(sel, K, empty_cam)
    cap = x["sel_idx"].shape[1]
    topk = SEL[sel]["topk"]
    parts = []
    for lo, hi in _blocks(split):
        b = _slice(x, lo, hi)
        rows_b = min(P, (hi - lo) * cap)                            # what Far3DEngine.block_rows gives a block
        ob, rb = _bufs(rows_b, x["C"]), _records(rows_b, K)
        ops.proposal_gather_md(b["reg"], x["strides"], b["sel_idx"], b["sel_cnt"], b["wgt"], b["dl"], DEPTH["stride"], DEPTH, b["i2l"],
                               b["feat"], PC, K, rmb, rb, ob, primary_rows=rows_b)
        # top-K: the static count; threshold: none (the kernel takes min(sum sel_cnt, rows_b), what gather_md kept)
        parts.append(dict(rows=ob, records=rb, sel_cnt=b["sel_cnt"], first_cam=lo, count=(hi - lo) * cap if topk else None))
    out, rec = _bufs(rows_total, x["C"]), _records(P, K)
    sel_cnt = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    m, ovf = _scalars()
    ops.proposal_merge_blocks(parts, out, sel_cnt, P, records_out=rec, m_out=m, overflow_out=ovf)
    torch.cuda.synchronize()
    M = sum(x["cnt"])
    Mp = min(M, P)
    assert int(m.item()) == Mp and int(ovf.item()) == (1 if M > P else 0)       # the merge's own count and flag
    assert sel_cnt.cpu().tolist() == x["cnt"]
    for t in out:                                                   # rows past the primaries are not the merge's: still the NaN fill
        assert bool(torch.isnan(t[Mp:]).all())
    ops.proposal_extra_rows(sel_cnt, 0 if topk else cap, P, K, rec, x["i2l"], DEPTH, PC, out, fill_hole=True, m_out=m, overflow_out=ovf)
    torch.cuda.synchronize()
    return out, rec, int(m.item()), int(ovf.item())


def _same(got, want, rows_total, what):
    (o, rec, m, ovf), (ro, rrec, rm, rovf) = got, want
    assert (m, ovf) == (rm, rovf), "%s: M' %d / flag %d, all cameras at once %d / %d" % (what, m, ovf, rm, rovf)
    for a, b in zip(o, ro):
        assert torch.equal(a[:m], b[:m]), what
        assert bool((a[m:rows_total] == 0).all()), what
    if rec is not None:
        assert torch.equal(rec[0], rrec[0]) and torch.equal(rec[1], rrec[1]), what


def _sweep_md(sel, K, split, empty_cam=None):
    """range_min_bin none / some / all valid x primary_rows ample / M / M - 1 x rows_total full / cutting the extras inside a k."""
    x = _case(sel, K, empty_cam)
    cap = x["sel_idx"].shape[1]
    M = sum(x["cnt"])
    seen = []
    for rmb, want in ((ND, "none"), (25, "some"), (0, "all")):
        for P in (N * cap, M, M - 1):
            Mp = min(M, P)
            full = K * P
            ref = _reference_md(sel, K, empty_cam, rmb, P, full)
            V = (ref[2] - Mp) // (K - 1)
            assert {"none": V == 0, "some": 0 < V < Mp, "all": V == Mp}[want], (want, V, Mp)
            cut = Mp + (K - 2) * V + V // 2 + 1                    # the last k loses the second half of its rows
            for rows_total in {full, max(cut, P)}:
                what = "%s K=%d split=%s rmb=%d P=%d rows=%d" % (sel, K, split, rmb, P, rows_total)
                ref = _reference_md(sel, K, empty_cam, rmb, P, rows_total)
                _same(_merged_md(sel, K, empty_cam, rmb, P, rows_total, split), ref, rows_total, what)
                seen.append((want, P, rows_total, ref[2], ref[3]))
    return M, seen


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("K", [2, 3, 8])
@pytest.mark.parametrize("sel", ["topk", "thr", "thr_wide"])
def test_merge_blocks_multi_depth_equals_all_cameras_at_once(hip_lib, sel, K, split):
    M, seen = _sweep_md(sel, K, split)
    cnt = _case(sel, K, None)["cnt"]
    print(sel, K, split, "M", M, cnt, seen)
    if sel == "topk":
        assert cnt == [6] * N
    elif sel == "thr":
        assert cnt == [16] * N                                      # every camera at its selection capacity: always flagged
    else:
        assert len(set(cnt)) > 1 and max(cnt) < 128                 # the cameras differ, none is full
    assert any(ovf == 1 for *_, ovf in seen)                        # M - 1 primary rows and the cut drop rows
    assert sel == "thr" or any(ovf == 0 for *_, ovf in seen)        # ample rows do not
    assert any(m < rows for _, _, rows, m, _ in seen)                                   # and some case has a hole


@pytest.mark.parametrize("split,empty_cam", [((2, 1), 2), ((1, 2), 0), ((1, 1, 1), 1)])
def test_merge_blocks_with_a_block_without_proposals(hip_lib, split, empty_cam):
    x = _case("thr", 2, empty_cam)
    assert x["cnt"][empty_cam] == 0 and sum(x["cnt"]) > 0
    _sweep_md("thr", 2, split, empty_cam)


@pytest.mark.parametrize("split", SPLITS)
def test_merge_blocks_camera_at_its_selection_capacity_sets_the_flag(hip_lib, split):
    x = _case("thr_full", 3, None)
    cap = x["sel_idx"].shape[1]
    assert max(x["cnt"]) == cap                                     # a camera filled sel_cap: peaks may be lost, the frame is flagged
    P = N * cap
    ref = _reference_md("thr_full", 3, None, 25, P, 3 * P)
    assert ref[3] == 1 and ref[2] < 3 * P
    _same(_merged_md("thr_full", 3, None, 25, P, 3 * P, split), ref, 3 * P, "thr_full %s" % (split,))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("sel", ["thr_wide", "thr_full"])
def test_merge_blocks_single_depth_equals_proposal_gather(hip_lib, sel, split):
    """Records NULL: the merge also writes the hole and is the whole job; the blocks' counts and flags are proposal_gather's own."""
    from far3d_amd import ops
    x = _case(sel, 2, None)
    cap = x["sel_idx"].shape[1]
    M = sum(x["cnt"])
    for rows_total in (N * cap, M, M - 1):
        ref, (rm, rovf) = _bufs(rows_total, x["C"]), _scalars()
        ops.proposal_gather(x["reg"], x["strides"], x["sel_idx"], x["sel_cnt"], x["wgt"], x["dl"], DEPTH["stride"], DEPTH, x["i2l"], x["feat"],
                            PC, out=ref, rows_total=rows_total, m_out=rm, overflow_out=rovf)
        parts = []
        for lo, hi in _blocks(split):
            b = _slice(x, lo, hi)
            rows_b = min(rows_total, (hi - lo) * cap)
            ob, (mb, fb) = _bufs(rows_b, x["C"]), _scalars()
            ops.proposal_gather(b["reg"], x["strides"], b["sel_idx"], b["sel_cnt"], b["wgt"], b["dl"], DEPTH["stride"], DEPTH, b["i2l"],
                                b["feat"], PC, out=ob, rows_total=rows_b, m_out=mb, overflow_out=fb)
            parts.append(dict(rows=ob, sel_cnt=b["sel_cnt"], first_cam=lo, count=mb, overflow=fb))
        out, (m, ovf) = _bufs(rows_total, x["C"]), _scalars()
        sel_cnt = torch.full((N,), -1, dtype=torch.int32, device=DEV)
        ops.proposal_merge_blocks(parts, out, sel_cnt, rows_total, m_out=m, overflow_out=ovf)
        torch.cuda.synchronize()
        want_flag = 1 if (M > rows_total or max(x["cnt"]) >= cap) else 0
        assert int(rm.item()) == min(M, rows_total) and int(rovf.item()) == want_flag
        assert sel_cnt.cpu().tolist() == x["cnt"]
        _same((out, None, int(m.item()), int(ovf.item())), (ref, None, int(rm.item()), int(rovf.item())), rows_total,
              "%s split=%s rows=%d" % (sel, split, rows_total))


def test_merge_blocks_single_depth_top_k_static_counts(hip_lib):
    """Top-K: the blocks' counts are static host numbers, there is no flag and no hole."""
    from far3d_amd import ops
    x = _case("topk", 2, None)
    cap = x["sel_idx"].shape[1]
    P = N * cap
    ref = _bufs(P, x["C"])
    ops.proposal_gather(x["reg"], x["strides"], x["sel_idx"], x["sel_cnt"], x["wgt"], x["dl"], DEPTH["stride"], DEPTH, x["i2l"], x["feat"], PC,
                        out=ref)
    parts = []
    for lo, hi in _blocks((1, 2)):
        b = _slice(x, lo, hi)
        ob = _bufs((hi - lo) * cap, x["C"])
        ops.proposal_gather(b["reg"], x["strides"], b["sel_idx"], b["sel_cnt"], b["wgt"], b["dl"], DEPTH["stride"], DEPTH, b["i2l"], b["feat"],
                            PC, out=ob)
        parts.append(dict(rows=ob, sel_cnt=b["sel_cnt"], first_cam=lo, count=(hi - lo) * cap))
    out, (m, ovf) = _bufs(P, x["C"]), _scalars()
    sel_cnt = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    ops.proposal_merge_blocks(parts, out, sel_cnt, P, m_out=m, overflow_out=ovf)
    torch.cuda.synchronize()
    assert int(m.item()) == P and int(ovf.item()) == 0 and sel_cnt.cpu().tolist() == [cap] * N
    for a, b in zip(out, ref):
        assert torch.equal(a, b)


def _offset_bufs(rows, C, off, K=None):
    """The four row arrays (and records) as views that start `off` words into their allocation: rows that begin 4 * off bytes past a
    16-byte boundary."""
    view = lambda w, dt, fill: torch.full((rows * w + 4,), fill, dtype=dt, device=DEV)[off:off + rows * w]
    out = (view(3, torch.float32, float("nan")).view(rows, 3), view(C + 1, torch.float32, float("nan")).view(rows, C + 1),
           view(4, torch.float32, float("nan")).view(rows, 4), view(1, torch.float32, float("nan")))
    rec = (view(1, torch.int32, 0), view(2 * K, torch.int32, 0).view(rows, 2 * K)) if K else None
    return out, rec


@pytest.mark.parametrize("off", [1, 2, 3])
def test_merge_blocks_rows_that_start_off_a_16_byte_boundary(hip_lib, off):
    """Source and destination `off` words past a 16-byte boundary: the copy peels 4 - off words, then moves 16 bytes per lane (block 0
    of every array; the later blocks land wherever their row offset puts them)."""
    from far3d_amd import ops
    sel, K, rmb = "thr_wide", 2, 25
    x = _case(sel, K, None)
    cap = x["sel_idx"].shape[1]
    P = N * cap
    ref = _reference_md(sel, K, None, rmb, P, K * P)
    parts = []
    for lo, hi in _blocks((1, 2)):
        b = _slice(x, lo, hi)
        ob, rb = _offset_bufs((hi - lo) * cap, x["C"], off, K)
        assert all(t.data_ptr() % 16 == 4 * off and t.is_contiguous() for t in ob + rb)
        ops.proposal_gather_md(b["reg"], x["strides"], b["sel_idx"], b["sel_cnt"], b["wgt"], b["dl"], DEPTH["stride"], DEPTH, b["i2l"],
                               b["feat"], PC, K, rmb, rb, ob, primary_rows=(hi - lo) * cap)
        parts.append(dict(rows=ob, records=rb, sel_cnt=b["sel_cnt"], first_cam=lo))
    out, _ = _offset_bufs(K * P, x["C"], off)
    _, rec = _offset_bufs(P, x["C"], off, K)
    assert x["cnt"][0] * (x["C"] + 1) > 8                           # block 0's context run has a 16-byte body behind the peeled words
    sel_cnt = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    m, ovf = _scalars()
    ops.proposal_merge_blocks(parts, out, sel_cnt, P, records_out=rec, m_out=m, overflow_out=ovf)
    ops.proposal_extra_rows(sel_cnt, cap, P, K, rec, x["i2l"], DEPTH, PC, out, fill_hole=True, m_out=m, overflow_out=ovf)
    torch.cuda.synchronize()
    _same((out, rec, int(m.item()), int(ovf.item())), ref, K * P, "offset %d" % off)
    # single depth: the merge's own zero-fill starts off the boundary too
    ref1, (rm, rovf) = _bufs(P, x["C"]), _scalars()
    ops.proposal_gather(x["reg"], x["strides"], x["sel_idx"], x["sel_cnt"], x["wgt"], x["dl"], DEPTH["stride"], DEPTH, x["i2l"], x["feat"], PC,
                        out=ref1, rows_total=P, m_out=rm, overflow_out=rovf)
    out1, _ = _offset_bufs(P, x["C"], off)
    ops.proposal_merge_blocks([dict(rows=p["rows"], sel_cnt=p["sel_cnt"], first_cam=p["first_cam"]) for p in parts], out1, sel_cnt, P,
                              m_out=m, overflow_out=ovf)
    torch.cuda.synchronize()
    _same((out1, None, int(m.item()), int(ovf.item())), (ref1, None, int(rm.item()), int(rovf.item())), P, "offset %d, single depth" % off)


def test_merge_blocks_refuses_blocks_that_are_not_the_frame(hip_lib):
    from far3d_amd import lib, ops
    x = _case("topk", 2, None)
    cap = x["sel_idx"].shape[1]
    ob = _bufs(cap, x["C"])
    part = dict(rows=ob, sel_cnt=x["sel_cnt"][:1], first_cam=1, count=cap)          # starts at camera 1
    out = _bufs(N * cap, x["C"])
    with pytest.raises(lib.Far3dHipError, match="ascending"):
        ops.proposal_merge_blocks([part], out, torch.zeros((N,), dtype=torch.int32, device=DEV), N * cap)
    part["first_cam"] = 0                                                           # one camera of three
    with pytest.raises(lib.Far3dHipError, match="cameras"):
        ops.proposal_merge_blocks([part], out, torch.zeros((N,), dtype=torch.int32, device=DEV), N * cap)

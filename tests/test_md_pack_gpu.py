"""GPU: far3d_proposal_pack_block and the record path above it (ops.proposal_pack_block, ops.md_block_views ->
Far3DEngine.merge_camera_blocks) -- what a rank of dist.ShardedFrame(multi_depth=True) sends and what every rank's head reads.
(a) the kernel on random words against a numpy construction, word for word; (b) simulated ranks on the multi-depth golden sequence:
the merge from gathered records must equal the merge from the blocks themselves bit for bit; (c) the overflow flag travels."""
import numpy as np
import pytest
import torch

from far3d_amd import synth
from tests.test_multidepth_gpu import _md_engine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7fc00001          # a NaN: survives no copy and no zero-fill
E = 256                        # 257-word context rows: odd word offsets inside the section


def _words(rng, shape):
    """Random 32-bit patterns (negative ints, denormals, infinities and NaNs among them), a few exact NaNs forced in."""
    a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = a.reshape(-1)
    flat[::7] = np.uint32(0xffc00000) | (flat[::7] & np.uint32(0x3fffff))
    flat[3::11] |= np.uint32(0x80000000)
    return a


def _f32(a):
    return torch.from_numpy(a.view(np.int32).copy()).to(DEV).view(torch.float32)


def _i32(a):
    return torch.from_numpy(a.view(np.int32).copy()).to(DEV)


def _block(rng, cams, n, K, sel):
    """A block as camera_stage leaves it (names and shapes), filled with random words; sel: its sel_cnt."""
    raw = dict(ref2d=_words(rng, (n, 3)), ctx=_words(rng, (n, E + 1)), box2d=_words(rng, (n, 4)), score=_words(rng, (n,)),
               md_flags=_words(rng, (n,)), md_info=_words(rng, (n, 2 * K)), img2lidar=_words(rng, (cams, 4, 4)),
               sel_cnt=np.asarray(sel, dtype=np.int32).view(np.uint32))
    st = dict(ref2d=_f32(raw["ref2d"]), ctx=_f32(raw["ctx"]), box2d=_f32(raw["box2d"]), score2d=_f32(raw["score"]), sel_cnt=_i32(raw["sel_cnt"]),
              md=dict(records=(_i32(raw["md_flags"]), _i32(raw["md_info"])), img2lidar=_f32(raw["img2lidar"])))
    return raw, st


def _expected(lay, raw, cams, c, flag):
    rec = np.zeros(lay["words"], dtype=np.uint32)
    rec[:4] = (cams, c, flag, 0)
    rec[lay["sel_cnt"]:lay["sel_cnt"] + cams] = raw["sel_cnt"]
    rec[lay["img2lidar"]:lay["img2lidar"] + cams * 16] = raw["img2lidar"].reshape(-1)
    for name in ("ref2d", "ctx", "box2d", "score", "md_flags", "md_info"):
        v = raw[name][:c].reshape(-1)
        rec[lay[name]:lay[name] + v.size] = v
    return rec


def _sentinel_record(words, lead=1):
    return torch.full((lead, words), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("rows", [5, 16])
@pytest.mark.parametrize("cams", [1, 2])
def test_pack_block_equals_a_numpy_construction_word_for_word(hip_lib, K, rows, cams):
    from far3d_amd import ops
    per = 2
    n = rows if cams == per else (rows + 1) // 2                    # a rank with fewer cameras than slots has a smaller block
    lay = ops.md_block_layout(per, rows, E, K)
    rng = np.random.default_rng(1000 * K + 10 * rows + cams)
    split = lambda tot: [tot] if cams == 1 else [tot // 2, tot - tot // 2]
    # (count argument, sel_cnt, rows that must arrive, flag from the count rule)
    counts = [(None, split(n - 1), n - 1, 0), (None, split(n), n, 0), (None, split(n + 3), n, 1), (None, split(0), 0, 0),
              (n - 1, split(2 * n), n - 1, 0), (n, split(1), n, 0), (0, split(n), 0, 0)]
    for count, sel, c, cflag in counts:
        for flag_in in (None, 0, 1, -5):
            raw, st = _block(rng, cams, n, K, sel)
            rec = _sentinel_record(lay["words"])
            ovf = None if flag_in is None else torch.tensor([flag_in], dtype=torch.int32, device=DEV)
            assert ops.proposal_pack_block(st, rec, lay, count=count, overflow=ovf) is rec
            got = rec.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1)
            flag = 1 if (cflag or flag_in not in (None, 0)) else 0
            want = _expected(lay, raw, cams, c, flag)
            what = "K=%d rows=%d cams=%d count=%s sel=%s flag_in=%s" % (K, rows, cams, count, sel, flag_in)
            assert not (got == np.uint32(SENTINEL)).any(), what + ": a word of the record was left unwritten"
            assert tuple(got[:4]) == (cams, c, flag, 0), what + ": header %s" % (got[:4],)
            bad = np.nonzero(got != want)[0]
            assert bad.size == 0, what + ": %d words differ, first at %d" % (bad.size, bad[0])
    with pytest.raises(ValueError, match="count"):                  # a static count cannot exceed the block's rows
        ops.proposal_pack_block(st, rec, lay, count=n + 1)


@pytest.mark.parametrize("count", [None, 0])
def test_pack_block_of_an_idle_rank_is_all_zeros(hip_lib, count):
    from far3d_amd import ops
    lay = ops.md_block_layout(2, 16, E, 3)
    rec = _sentinel_record(lay["words"])
    ops.proposal_pack_block(None, rec, lay, count=count)
    assert int(rec.view(torch.int32).abs().max().item()) == 0
    with pytest.raises(ValueError, match="empty block"):
        ops.proposal_pack_block(None, rec, lay, count=3)
    with pytest.raises(ValueError, match="words"):
        ops.proposal_pack_block(None, rec[:, :-4].contiguous(), lay)


def _blocks_of(eng, dd, pad_hw, N):
    sts = []
    for c in range(N):
        with eng.buffers(("block", c)):
            sts.append(eng.camera_stage(dd["img"][c:c + 1], dd, range(c, c + 1), pad_hw, block_rows=eng.camera_block_rows(1)))
    return sts


def _snapshot(st):
    keep = {k: st[k].clone() for k in ("ref2d", "ctx", "box2d", "score2d", "sel_cnt", "m_dev", "overflow")}
    keep["md_records"] = tuple(t.clone() for t in st["md_records"])
    return keep


def _through_records(eng, sts, world):
    """The blocks as `world` ranks would exchange them (one camera per rank, the ranks past the cameras idle): packed into a
    sentinel-filled (world, words) tensor, then merged from views into it."""
    from far3d_amd import ops
    K = eng.cfg["proposal_topk"]
    capT = eng.cfg.get("proposal_capacity") if K is None else None
    lay = ops.md_block_layout(1, eng.camera_block_rows(1), eng.cfg["embed_dims"], eng.md_k)
    buf = _sentinel_record(lay["words"], world)
    for r in range(world):
        st = sts[r] if r < len(sts) else None
        ops.proposal_pack_block(st, buf[r:r + 1], lay, count=(K if st is not None else 0) if K is not None else None)
    assert not bool((buf.view(torch.int32) == SENTINEL).any())
    assert all(int(buf[r].view(torch.int32).abs().max().item()) == 0 for r in range(len(sts), world))
    sel_cap = sts[0]["md"]["sel_cap"]
    assert sel_cap == (min(eng.cfg["proposal_cap"], sts[0]["tokens"].shape[1]) if capT is not None else 0)
    blocks = [ops.md_block_views(buf[r], lay, 1, r, sel_cap) for r in range(len(sts))]
    return eng.merge_camera_blocks(blocks), buf, lay


@pytest.mark.parametrize("mode", [dict(proposal_topk=16), dict(proposal_capacity=48)], ids=["topk", "capacity"])
def test_merge_from_gathered_records_equals_merge_from_the_blocks(hip_lib, mode):
    eng, z, rc = _md_engine("far3d_md2_seq", **mode)
    N = rc["num_cams"]
    P = 48 if "proposal_capacity" in mode else N * 16
    with torch.no_grad():
        for fi in range(3):                                         # frame 2 starts a new scene
            data, metas = synth.recipe_frame(rc, fi)
            pad_hw = tuple(metas[0]["pad_shape"][0][:2])
            dd = eng._stage_inputs(data)
            sts = _blocks_of(eng, dd, pad_hw, N)
            want = _snapshot(eng.merge_camera_blocks(sts))
            m, Mp = int(want["m_dev"].item()), min(int(want["sel_cnt"].sum().item()), P)
            assert m > int(want["sel_cnt"].sum().item()) > 0, "frame %d: the fixture must produce extra rows" % fi
            for world in (2, 3):
                got, _, _ = _through_records(eng, sts, world)
                what = "frame %d world %d" % (fi, world)
                for k in ("sel_cnt", "m_dev", "overflow"):
                    assert torch.equal(got[k], want[k]), "%s: %s" % (what, k)
                for k in ("ref2d", "ctx", "box2d", "score2d"):
                    assert torch.equal(got[k][:m].view(torch.int32), want[k][:m].view(torch.int32)), "%s: %s" % (what, k)
                for a, b in zip(got["md_records"], want["md_records"]):
                    assert torch.equal(a[:Mp], b[:Mp]), what + ": records"
                eng.check_proposal_overflow()


def test_overflow_flag_travels_through_the_record(hip_lib):
    """proposal_capacity = 8 with 13+ proposals per camera.  The header of an overflowing block says so, and the frame's flag after the
    merge from records is the one the merge from the blocks gives.  (With multi-depth records far3d_proposal_extra_rows writes the
    frame's final flag from the frame's sel_cnt, which the records carry; a flag handed to the pack reaches the header: test above.)"""
    from far3d_amd import lib
    # a camera with more proposals than its block has rows: the pack's own count rule raises the flag in the header
    eng, z, rc = _md_engine("far3d_md2_seq", proposal_capacity=8)
    N = rc["num_cams"]
    with torch.no_grad():
        data, metas = synth.recipe_frame(rc, 0)
        dd = eng._stage_inputs(data)
        sts = _blocks_of(eng, dd, tuple(metas[0]["pad_shape"][0][:2]), N)
        rows = eng.camera_block_rows(1)
        sel = torch.cat([s["sel_cnt"] for s in sts]).cpu().numpy()
        assert rows == 8 and sel.max() > rows
        want = _snapshot(eng.merge_camera_blocks(sts))
        got, buf, lay = _through_records(eng, sts, 3)
        head = buf.view(torch.int32)[:, :4].cpu().numpy()
        assert [tuple(h) for h in head] == [(1, min(int(s), rows), int(s > rows), 0) for s in sel] + [(0, 0, 0, 0)]
        assert int(got["overflow"].item()) == 1 == int(want["overflow"].item()) and torch.equal(got["m_dev"], want["m_dev"])
        with pytest.raises(lib.Far3dHipError, match="proposal capacity exceeded"):
            eng.check_proposal_overflow()

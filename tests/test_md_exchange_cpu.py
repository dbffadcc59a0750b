"""CPU: the host arithmetic of the multi-depth camera-sharded exchange -- the word layout of a rank's record (ops.md_block_layout,
the layout far3d_proposal_pack_block writes and ops.md_block_views reads) and the rank -> camera-block mapping that
dist.ShardedFrame(multi_depth=True) derives from dist.camera_shards."""
import itertools

import pytest

SECTIONS = ("header", "sel_cnt", "img2lidar", "ref2d", "ctx", "box2d", "score", "md_flags", "md_info")


def _sizes(per, rows, E, K):
    return dict(header=4, sel_cnt=per, img2lidar=per * 16, ref2d=rows * 3, ctx=rows * (E + 1), box2d=rows * 4, score=rows, md_flags=rows,
                md_info=rows * 2 * K)


@pytest.mark.parametrize("K,E,rows,per", list(itertools.product((2, 3, 8), (256, 8), (1, 5, 16), (1, 2))))
def test_record_sections_are_aligned_disjoint_and_ordered(K, E, rows, per):
    from far3d_amd import ops
    assert ops.MD_BLOCK_SECTIONS == SECTIONS
    lay = ops.md_block_layout(per, rows, E, K)
    assert (lay["per"], lay["rows"], lay["E"], lay["K"]) == (per, rows, E, K)
    size = _sizes(per, rows, E, K)
    assert lay["header"] == 0
    end = 0
    for name in SECTIONS:
        assert lay[name] % 4 == 0, "%s starts at word %d: not a 16-byte boundary" % (name, lay[name])
        assert end <= lay[name] < end + 4, "%s overlaps its predecessor or leaves more than an alignment gap" % name
        end = lay[name] + size[name]
    assert end <= lay["words"] < end + 4 and lay["words"] % 4 == 0      # records stacked as (world, words) stay aligned
    # a function of the four static sizes only: every rank computes the same record, whatever cameras it owns
    assert ops.md_block_layout(per, rows, E, K) == lay


def test_record_layout_refuses_what_the_kernel_refuses():
    from far3d_amd import ops
    for bad in ((0, 4, 256, 2), (1, 0, 256, 2), (1, 4, 0, 2), (1, 4, 256, 1), (1, 4, 256, 9)):
        with pytest.raises(ValueError, match="md_block_layout"):
            ops.md_block_layout(*bad)


@pytest.mark.parametrize("cams,world", [(2, 2), (2, 3), (7, 8), (7, 4)])
def test_rank_blocks_ascend_and_cover_the_cameras(cams, world):
    """What ShardedFrame._head_md turns into merge_camera_blocks' blocks: rank r's cameras are one contiguous run, the runs of the
    non-idle ranks ascend and tile [0, N), and an idle rank (only padding slots) contributes no block."""
    from far3d_amd.dist import camera_shards
    per, shards = camera_shards(cams, world)
    assert per == -(-cams // world) and len(shards) == world and all(len(s) == per for s in shards)
    blocks, idle = [], 0
    for slots in shards:
        own = [c for c in slots if c >= 0]
        assert slots == own + [-1] * (per - len(own))               # padding slots come last
        if own:
            assert own == list(range(own[0], own[0] + len(own)))
            blocks.append((own[0], own[0] + len(own)))
        else:
            idle += 1
    assert [b[0] for b in blocks] + [cams] == [0] + [b[1] for b in blocks]
    assert len(blocks) + idle == world
    assert idle == {(2, 2): 0, (2, 3): 1, (7, 8): 1, (7, 4): 0}[(cams, world)]

"""CPU: the tile registry (far3d_amd/csrc/conv_tiles.hpp through far3d_conv_tile_caps) names exactly the tiles the dispatchers had when
the table was introduced, family by family and storage by storage.  The id sets are literals on purpose: a tile that appears, vanishes
or changes family shows up here before any GPU run.  The GPU suites launch the same ids (TILES_3X3, TILES_1X1, TILES_WS, TILES_WS_GEMM of
test_pair_gpu.py, the parametrisations of test_igemm_gpu.py, GROUP_TILES of test_grouped_conv_gpu.py)."""
import pytest

from far3d_amd import ops

BF16, PAIR, F32_SPLIT, F32 = (ops.DT_BF16, ops.DT_BF16), (ops.DT_BF16_PAIR, ops.DT_F32_BF16X3), (ops.DT_F32, ops.DT_F32_BF16X3), (ops.DT_F32, ops.DT_F32)
F32_BF16 = (ops.DT_F32, ops.DT_BF16)
ANY, K1, K3, K3S2 = ops.TILE_ANY, ops.TILE_1X1, ops.TILE_3X3, ops.TILE_3X3S2

IGEMM = {1, 2, 3, 4, 5}                                                             # register-staged, every storage
DMA = {1, 2, 3, 4, 18, 43, 46, 48}
GEMM_BF16 = {*range(70, 90), *range(110, 118), *range(120, 130), *range(140, 146)}
CONV3_BF16 = {*range(50, 56), *range(57, 68), *range(90, 98), *range(100, 107), *range(130, 140)}
CONV3S2_BF16 = {*range(30, 36)}
WS_CONV3_BF16 = {420, 421, 422, 423}
GEMM_PAIR = {*range(170, 182), *range(185, 189)}
GEMM_PAIR_HI = {279, 280}
CONV3_PAIR = {150, *range(152, 156), 157, *range(159, 170), *range(190, 194), 197, 198}
CONV3_PAIR_HI = {252, 260, 265}
CONV3S2_PAIR = {330, 331}
WS_CONV3_PAIR = {*range(400, 420), 440, 444, 445, *range(450, 460)}
WS_GEMM = {*range(460, 472), *range(473, 477)}
GROUPED = {500, 505, 552, 556, 559}
GEMM_F32_SPLIT = {479, 480, 481}
GEMM_F32 = {*range(482, 495)}

# storage -> {geometry: ids}
EXPECTED = {
    BF16: {ANY: DMA | {5}, K1: GEMM_BF16, K3: CONV3_BF16 | WS_CONV3_BF16, K3S2: CONV3S2_BF16},
    PAIR: {ANY: IGEMM, K1: GEMM_PAIR | GEMM_PAIR_HI | WS_GEMM, K3: CONV3_PAIR | CONV3_PAIR_HI | WS_CONV3_PAIR | GROUPED, K3S2: CONV3S2_PAIR},
    F32_SPLIT: {ANY: IGEMM, K1: GEMM_F32_SPLIT},
    F32: {ANY: IGEMM, K1: GEMM_F32},
    F32_BF16: {ANY: IGEMM},
}
# the tiles far3d_conv2d_nhwc took channel sums on when the table was introduced: the pipelined GEMM tiles that leave LDS for the sums'
# scratch (114 / 115 fill the 160 KB with their ring) and the persistent GEMM; never a K-group tile (487-494) or any fp32-row tile
SUMS_BF16 = GEMM_BF16 - {114, 115}
SUMS_PAIR = GEMM_PAIR | GEMM_PAIR_HI | WS_GEMM
ALL_IDS = range(0, 700)


@pytest.mark.parametrize("store", list(EXPECTED), ids=["bf16", "pair", "f32_split", "f32", "f32_bf16"])
def test_registry_is_exactly_the_expected_ids(store, hip_lib):
    got = {}
    for t in ALL_IDS:
        c = hip_lib.far3d_conv_tile_caps(t, *store)
        if c >= 0:
            assert (c >> 2) & 7 == list(EXPECTED).index(store), (t, c)               # the storage it was asked about
            assert c >> 16 > 0 and (c >> 16) % 32 == 0, (t, c)                      # pixels per tile
            got.setdefault(c & 3, set()).add(t)
    assert got == EXPECTED[store]
    assert hip_lib.far3d_conv_tile_caps(0, *store) == -1 and hip_lib.far3d_conv_tile_caps(-1, *store) == -1
    assert hip_lib.far3d_conv_tile_caps(1000, *store) == -1


def test_wrong_storage_and_bad_dtypes_have_no_tiles(hip_lib):
    for t, store in ((70, PAIR), (170, BF16), (479, F32), (482, F32_SPLIT), (400, BF16), (420, PAIR), (460, BF16), (500, BF16), (18, F32), (330, BF16)):
        assert hip_lib.far3d_conv_tile_caps(t, *store) == -1, (t, store)
    for x_dt, w_dt in ((ops.DT_BF16, ops.DT_F32), (ops.DT_BF16_PAIR, ops.DT_BF16), (ops.DT_BF16_PAIR, ops.DT_F32), (7, 0), (0, 7), (ops.DT_F32_BF16X3, 0)):
        assert all(hip_lib.far3d_conv_tile_caps(t, x_dt, w_dt) == -1 for t in (1, 70, 179, 400)), (x_dt, w_dt)


def test_flags(hip_lib):
    caps = {t: ops.tile_caps(t) for t in ALL_IDS if t > 5 and ops.tile_caps(t) >= 0}
    flagged = lambda bit: {t for t, c in caps.items() if c & bit}      # noqa: E731
    assert flagged(ops.TILE_HI_ONLY) == GEMM_PAIR_HI | CONV3_PAIR_HI
    assert flagged(ops.TILE_PERSISTENT) == WS_CONV3_BF16 | WS_CONV3_PAIR | WS_GEMM | GROUPED == {t for t in ALL_IDS if ops.is_ws_tile(t)}
    assert flagged(ops.TILE_GROUPED) == GROUPED == {t for t in ALL_IDS if ops.is_group_tile(t)}
    assert flagged(ops.TILE_HAS_GROUP) == {t - 100 for t in GROUPED}
    for t in GROUPED:                   # a grouped id is the workgroup of id - 100: same geometry, storage, pixels
        drop = ops.TILE_GROUPED | ops.TILE_HAS_GROUP
        assert caps[t] & ~drop == caps[t - 100] & ~drop and ops.tile_caps(t, *PAIR) == caps[t], t
    assert flagged(ops.TILE_LDS_DMA) == set(caps)                      # everything but the register-staged ids 1-5 ...
    assert all(ops.tile_caps(t, *BF16) & ops.TILE_LDS_DMA for t in (1, 2, 3, 4)) and not ops.tile_caps(5, *BF16) & ops.TILE_LDS_DMA
    assert not any(ops.tile_caps(t, *s) & ops.TILE_LDS_DMA for t in IGEMM for s in (PAIR, F32_SPLIT, F32, F32_BF16))
    # pixels per tile: channels x PIXELS of the GEMM rows, 32 x rows of the 3x3 rows
    assert [caps[t] >> 16 for t in (70, 72, 80, 114, 185, 187, 460, 470, 491)] == [128, 256, 64, 512, 160, 96, 128, 256, 32]
    assert [caps[t] >> 16 for t in (50, 131, 169, 331, 400, 405, 456, 505)] == [128, 512, 224, 64, 256, 128, 224, 128]


def test_channel_sums_are_possible_exactly_where_they_were(hip_lib):
    assert {t for t in ALL_IDS if ops.tile_takes_sums(t, False)} == SUMS_BF16
    assert {t for t in ALL_IDS if ops.tile_takes_sums(t, True)} == SUMS_PAIR
    for t in (114, 115, *range(487, 495)):
        assert ops.tile_caps(t) >= 0 and not ops.tile_caps(t) & ops.TILE_SUMS, t
    assert not any(ops.tile_caps(t) & ops.TILE_SUMS for t in GEMM_F32_SPLIT | GEMM_F32)

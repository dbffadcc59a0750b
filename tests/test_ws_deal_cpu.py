"""CPU: how a single-problem launch of the persistent 3x3 kernel deals its items to its workgroups (far3d_ws_deal, the host entry of
the inline function the kernel evaluates -- csrc/conv_ws.hpp ws_deal_*).

A launch has F full items and L light ones (the items of a partly empty last channel tile, whose padded 32-channel slices the consumers
skip).  The mapping (workgroup, k) -> item must be a permutation of the items, and the heaviest workgroup must cost no more than one
light item above what greedy longest-first dealing gives.

Cost ratio assumed here: light : full = 1 : 2 (0.5), the ratio the mapping itself is built for (FAR3D_WS_DEAL_LIGHT / FAR3D_WS_DEAL_FULL).
Longest-first with these costs: every full item, then every light item, each to the workgroup that is lightest at that moment.
"""
import heapq

import pytest

FULL, LIGHT = 2, 1
GRIDS = (1, 7, 256, 512)
PAIRS = ((560, 280), (0, 5), (5, 0), (255, 1), (1, 700))


def _greedy_max(F, L, G):
    heap = [0] * G
    for cost in [FULL] * F + [LIGHT] * L:
        heapq.heappush(heap, heapq.heappop(heap) + cost)
    return max(heap)


def _deal(lib, F, L, G):
    per_wg = []
    for wg in range(G):
        items, k = [], 0
        while True:
            it = lib.far3d_ws_deal(F, L, G, wg, k)
            if it < 0:
                break
            items.append(it)
            k += 1
            assert k <= F + L, "workgroup %d of %d never ends" % (wg, G)
        assert lib.far3d_ws_deal(F, L, G, wg, k + 1) == -1 and lib.far3d_ws_deal(F, L, G, wg, -1) == -1
        per_wg.append(items)
    return per_wg


@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("F,L", PAIRS)
def test_deal_is_a_permutation_within_one_light_item_of_greedy(hip_lib, F, L, G):
    per_wg = _deal(hip_lib, F, L, G)
    flat = [it for items in per_wg for it in items]
    assert sorted(flat) == list(range(F + L)), "not a permutation of the %d items" % (F + L)
    for items in per_wg:                          # full items go first in every workgroup
        kinds = [it >= F for it in items]
        assert kinds == sorted(kinds)
    heaviest = max(sum(LIGHT if it >= F else FULL for it in items) for items in per_wg)
    assert heaviest <= _greedy_max(F, L, G) + LIGHT, (F, L, G, heaviest, _greedy_max(F, L, G))
    # full items round-robin: workgroup b holds the fulls b, b + G, ...
    for b, items in enumerate(per_wg):
        assert [it for it in items if it < F] == list(range(b, F, G))


def test_deal_without_light_items_is_the_static_round_robin(hip_lib):
    for G in GRIDS:
        for wg in (0, G // 2, G - 1):
            for k in range(4):
                it = wg + k * G
                assert hip_lib.far3d_ws_deal(1000, 0, G, wg, k) == (it if it < 1000 else -1)


def test_deal_refuses_bad_arguments(hip_lib):
    for args in ((-1, 0, 4, 0, 0), (1, -1, 4, 0, 0), (4, 4, 0, 0, 0), (4, 4, 4, 4, 0), (4, 4, 4, -1, 0)):
        assert hip_lib.far3d_ws_deal(*args) == -1

"""CPU: the two host predicates of the aggregation's kernel choice (ops.aggregate_kernel8_applies, ops.aggregate_sorted_applies) on both
sides of every boundary of the library's rule (csrc/sampling.hip: agg_kernel8_applies, the qbase check), and the engine's sorted gate."""
from types import SimpleNamespace

import pytest

from far3d_amd import ops

GIB4 = 1 << 32


@pytest.mark.parametrize("N,P,L,want", [
    (8, 16, 4, True), (9, 16, 4, False),          # cameras
    (8, 16, 1, True), (8, 17, 1, False),          # points
    (2, 1, 4, True), (2, 1, 5, False),            # levels
    (1, 1, 1, True), (7, 13, 4, True),            # the smallest shape and the model's
    (16, 6, 4, False),
])
def test_kernel8_rule_boundaries(N, P, L, want):
    assert ops.aggregate_kernel8_applies(N, P, L) is want
    assert ops.aggregate_kernel8_applies(N, P, L, 16, 256, 4) is want       # small maps change nothing


@pytest.mark.parametrize("esz", [2, 4])
def test_kernel8_rule_needs_the_maps_of_a_sample_below_4_gib(esz):
    """N * S * C * esz < 2^32, with integers only: the largest S that passes and the one above, for bf16 and fp32 rows."""
    N, C = 8, 256
    s_max = (GIB4 - 1) // (N * C * esz)
    assert N * s_max * C * esz < GIB4 <= N * (s_max + 1) * C * esz
    assert ops.aggregate_kernel8_applies(N, 13, 4, s_max, C, esz)
    assert not ops.aggregate_kernel8_applies(N, 13, 4, s_max + 1, C, esz)
    assert ops.aggregate_sorted_applies(N, 13, 4, s_max, C, esz)
    assert not ops.aggregate_sorted_applies(N, 13, 4, s_max + 1, C, esz)
    # without S or without the element size the byte rule is not part of the answer
    assert ops.aggregate_kernel8_applies(N, 13, 4, s_max + 1) and ops.aggregate_kernel8_applies(N, 13, 4, esz=esz)
    # the same S passes with 2-byte rows where it fails with 4-byte rows
    s4 = (GIB4 - 1) // (N * C * 4) + 1
    assert ops.aggregate_kernel8_applies(N, 13, 4, s4, C, 2) and not ops.aggregate_kernel8_applies(N, 13, 4, s4, C, 4)


@pytest.mark.parametrize("N,P,L,want", [
    (7, 13, 4, True),                             # L * P = 52
    (2, 14, 4, False), (7, 14, 4, False),         # 56
    (8, 16, 3, True), (8, 16, 4, False),          # 48 / 64
    (1, 53, 1, False), (2, 4, 13, False),         # 53 / 52 products outside kernel 8's family (P > 16, L > 4)
    (7, 26, 2, False),                            # L * P = 52 but P > 16: kernel 7's shape
    (9, 13, 4, False),                            # N > 8
])
def test_sorted_rule_is_kernel8s_and_lp_at_most_52(N, P, L, want):
    assert ops.aggregate_sorted_applies(N, P, L) is want
    assert ops.aggregate_sorted_applies(N, P, L) == (ops.aggregate_kernel8_applies(N, P, L) and L * P <= 52)


def _gate(N, P, L, A=10, split=None, agg_sorted=True, variant=0, S=100, esz=2):
    from far3d_amd.engine import Far3DEngine
    eng = SimpleNamespace(cfg={"num_pts": P, "num_levels": L}, agg_sorted=agg_sorted, agg_variant=variant)
    tokens = SimpleNamespace(shape=(N, S, 256), element_size=lambda: esz)
    return Far3DEngine._agg_sorted_gate(eng, A, split, tokens)


def test_engine_sorted_gate_is_the_predicate():
    """P = 26, L = 2, N = 7 passed the engine's earlier expression (N <= 8 and P * L <= 52), stored the operands in launch order and was
    then refused by the library; the gate is the library's rule now, and such a configuration runs unsorted."""
    N, P, L = 7, 26, 2
    assert N <= 8 and P * L <= 52                 # the earlier expression
    assert _gate(N, P, L) is False
    for N, P, L in [(7, 13, 4), (2, 14, 4), (8, 16, 3), (8, 16, 4), (9, 13, 4), (7, 26, 2), (1, 1, 1)]:
        assert _gate(N, P, L) is ops.aggregate_sorted_applies(N, P, L)
    assert _gate(7, 13, 4, S=GIB4 // (7 * 256 * 2) + 1) is False            # maps of 4 GiB: kernel 7, unsorted
    # what the gate asked before besides the shape stays: the flag, no sibling split, variant 0 / 8, rows to order
    assert _gate(7, 13, 4) is True and _gate(7, 13, 4, variant=8) is True
    assert _gate(7, 13, 4, agg_sorted=False) is False and _gate(7, 13, 4, split=object()) is False
    assert _gate(7, 13, 4, variant=7) is False and _gate(7, 13, 4, A=0) is False

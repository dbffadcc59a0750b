"""GPU: the decoder at engine level on the toy golden sequence (tests/golden/far3d_small_seq.npz: 2 cameras, 64x96, 60 queries, 16
propagated, 64 memory slots) -- a rank's rows of the query-sharded decoder against the same rows of the replicated one, in ONE process
(tests/test_dist_gpu.py runs the 2-process identity), and the aggregation's sorted mode against the unsorted one."""
import pytest
import torch

from far3d_amd import dist as fdist
from far3d_amd import synth

pytestmark = pytest.mark.gpu

_ENGINES = {}


def _engine(precision, **over):
    """One engine per (precision, proposal mode) for the whole module: the tests set every flag they depend on and reset the memory."""
    from tests.test_engine_gpu import _golden_engine
    key = (precision,) + tuple(sorted(over.items()))
    if key not in _ENGINES:
        eng, _, rc = _golden_engine(precision, **over)
        _ENGINES[key] = (eng, rc)
    eng, rc = _ENGINES[key]
    eng.reset_memory()
    eng.fused_rows, eng.agg_sorted = True, True
    return eng, rc


class _OneRank(fdist.QueryShard):
    """Rank `rank` of `world` without a process group: the exchange checks this rank's rows against the replicated decoder's and hands
    back the replicated layer output in place of the other ranks' rows (their equality is what the same check proves for those ranks)."""

    def __init__(self, rank, world, want, A):
        self.rank, self.world, self.want, self.A = rank, world, want, A
        self.layers = 0

    def gather(self, src, dst):
        per, A = self.rows_per_rank(self.A), self.A
        a0, a1 = min(self.rank * per, A), min((self.rank + 1) * per, A)
        nr = a1 - a0
        assert src.shape[0] == per and dst.shape[0] == self.world * per
        assert torch.equal(src[:nr], self.want[self.layers][a0:a1]), "layer %d: rows %d:%d of rank %d / %d differ from the replicated decoder's" % (
            self.layers, a0, a1, self.rank, self.world)
        assert not src[nr:].any(), "layer %d: the padding rows of the send buffer are not zero" % self.layers
        dst[:A].copy_(self.want[self.layers])
        self.layers += 1


# (world, rank) per proposal mode.  top-K 6: A = 60 + 2 * 6 + 16 = 88 rows, 136 keys.  Capacity 128: A = 204, the hole starts at row
# 60 + m_dev (frame 1 has 26 proposals in bf16: row 86): ranks (2, 0) = 0:104 and (5, 1) = 44:88 straddle it.  The test derives the
# rows from rows_per_rank and asserts the properties the cases are there for.
CASES = {"topk": ((2, 0), (2, 1), (5, 1), (5, 4), (23, 21), (23, 22)), "capacity": ((2, 0), (2, 1), (5, 1), (5, 4))}
MODES = {"topk": dict(proposal_topk=6), "capacity": dict(proposal_topk=None, proposal_capacity=128)}


@pytest.mark.parametrize("precision,fused,mode", [("fp32", False, "topk"), ("bf16", True, "topk"), ("bf16", False, "topk"),
                                                  ("bf16", True, "capacity"), ("bf16", False, "capacity")],
                         ids=["fp32", "bf16-chains", "bf16-unfused", "bf16-chains-capacity", "bf16-unfused-capacity"])
def test_a_ranks_rows_of_the_sharded_decoder_are_bitwise_the_replicated_rows(hip_lib, precision, fused, mode):
    """Frame 1 of the golden sequence (live memory keys): decoder(..., qshard=rank r of w) must hand the exchange exactly rows
    [a0, a1) of every layer of the replicated decoder, zero padding behind them, six exchanges, and return the replicated result --
    for a full share, a share whose first row is no multiple of the row chains' 16-row groups, a short last share, an empty
    share and (capacity mode) a share that straddles the first row of the hole."""
    eng, rc = _engine(precision, **MODES[mode])
    eng.fused_rows = fused
    chains = fused and precision == "bf16"
    assert not chains or all(ly["rc"] is not None for ly in eng.layers)
    for fi in (0, 1):
        data, metas = synth.recipe_frame(rc, fi)
        if fi == 1:
            assert metas[0]["scene_token"] == eng.prev_scene, "frame 1 must continue frame 0's scene"
        eng.forward_frame(data, metas)
    cfg = eng.cfg
    pad_hw = tuple(metas[0]["pad_shape"][0][:2])
    dd = eng._stage_inputs(data)
    st = eng._camera_part(dd, pad_hw)
    nq, P_ = cfg["num_query"], cfg["num_propagated"]
    M = eng.static_adaptive_rows(cfg["num_cams"])
    A = nq + M + P_
    TQ, QP, RF, X2 = (eng._bufs[(0, k)] for k in ("tq", "qp", "rf", "x2op"))
    assert X2.shape[0] == nq + M + cfg["memory_len"] and X2[A:].float().abs().sum().item() > 0, "no live memory keys"
    hole = hole_row = None
    if mode == "capacity":
        m_dev = int(st["m_dev"].item())
        print("capacity %d: %d proposals" % (M, m_dev))
        assert 0 < m_dev < M
        hole, hole_row = (st["m_dev"], nq, nq + M), nq + m_dev
    else:
        assert (A, X2.shape[0]) == (88, 136)
    args = (X2, TQ[:A], QP[:A], st["tokens"], RF[:A], st["hw"], st["starts"], dd["lidar2img"][0], pad_hw, A)
    keep = X2.clone()                      # the replicated decoder overwrites the query rows of its operand
    want = eng.decoder(*args, hole=hole).clone()
    assert want.shape == (cfg["num_layers"], A, cfg["embed_dims"]) and torch.isfinite(want).all()
    seen = set()
    for world, rank in CASES[mode]:
        stub = _OneRank(rank, world, want, A)
        per = stub.rows_per_rank(A)
        a0, a1 = min(rank * per, A), min((rank + 1) * per, A)
        seen |= {"full"} if a1 - a0 == per else set()
        seen |= {"odd start"} if a0 % 16 and a1 > a0 else set()
        seen |= {"short"} if 0 < a1 - a0 < per else set()
        seen |= {"empty"} if a1 == a0 else set()
        seen |= {"hole"} if hole_row is not None and a0 < hole_row < a1 else set()
        X2.copy_(keep)
        got = eng.decoder(*args, hole=hole, qshard=stub)
        assert stub.layers == 6, "rank %d / %d: %d exchanges" % (rank, world, stub.layers)
        assert torch.equal(got, want), "rank %d / %d: the sharded decoder's result differs" % (rank, world)
    assert seen >= ({"full", "odd start", "short", "empty"} if mode == "topk" else {"full", "short", "hole"}), seen


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sorted_aggregation_mode_is_bitwise_the_unsorted_engine(hip_lib, precision):
    """agg_sorted only changes where the aggregation's operands are stored and read (tests/test_sampling_gpu.py asserts the
    operator's identity): logits, boxes and decoder states of golden frames 0 and 1 are the same bits either way -- fp32 (unfused
    loop, LN0 stores through the row map) and bf16 with the row chains (the attention-output chain does)."""
    eng, rc = _engine(precision, proposal_topk=6)
    res = {}
    for srt in (True, False):
        eng.reset_memory()
        eng.agg_sorted = srt
        out = []
        for fi in (0, 1):
            o = eng.forward_frame(*synth.recipe_frame(rc, fi))
            out.append({k: o[k].clone() for k in ("all_cls_scores", "all_bbox_preds", "outs_dec")})
        assert (eng.last_agg[-1] is not None) == srt, "the sorted mode did not follow the flag"
        res[srt] = out
    for fi, (a, b) in enumerate(zip(res[True], res[False])):
        for k in a:
            assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), "frame %d: %s differs between sorted and unsorted" % (fi, k)

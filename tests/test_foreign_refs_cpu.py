"""CPU: tests/foreign_refs.py (the float64 restatement of build_query2d_proposal for given boxes) agrees with tests/head_refs.py where
both state the same thing, and the seeded inputs of tests/test_foreign_props_gpu.py leave no decision to rounding.

Margins.  The depth bins are ranked on values that are INPUTS (both sides compare the same float32 numbers), which is why
tests/test_proposals_gpu.py gives that decision no margin and never skips it: the bar here is a strictly positive gap between ranks
k and k + 1 for every proposal, zero exclusions.  The depth cell is round(centre / stride): a centre must stay head_refs.CELL_MARGIN
away from a cell border unless it was put on one deliberately (exact half cells, where half-to-even decides on both sides)."""
import pytest
import torch

from tests import foreign_refs as fr
from tests import head_refs as hr


@pytest.mark.parametrize("geom,variant", [("small3", "plain"), ("odd2", "wide"), ("small3", "empty")])
def test_restatement_agrees_with_head_refs_on_its_own_boxes(geom, variant):
    """Fed with the boxes, scores and selection hr.proposal_rows itself produces, foreign_rows returns proposal_rows' rows."""
    case = hr.proposal_case(geom, 26, 5, variant, with_feat=True)
    _, peak = hr.proposal_weights(hr.widen(case["cls"]), hr.widen(case["reg"]))
    sel = [torch.nonzero(peak[n] > 0.1)[:, 0] for n in range(case["N"])]
    want = hr.proposal_rows(hr.widen(case["reg"]), case["strides"], sel, peak, case["depth_logit"].double(), case["ds"], hr.DEPTH_CFG,
                            case["img2lidar"].double(), case["feat"].double(), case["pc_range"])
    M = want["cam"].numel()
    assert M > 20
    off = [0]
    for s in sel:
        off.append(off[-1] + s.numel())
    mask = torch.zeros(case["N"], case["S"], dtype=torch.bool)
    for n, s in enumerate(sel):
        mask[n, s] = True
    got = fr.foreign_rows([want["box2d"][off[n]:off[n + 1]] for n in range(case["N"])], mask, want["score"], case["depth_logit"].double(),
                          case["ds"], hr.DEPTH_CFG, case["img2lidar"].double(), case["feat"].double(), case["pc_range"], topk=1,
                          depth_is_prob=False)
    assert torch.equal(got["cell"], want["cell"]) and torch.equal(got["bin"], want["bin"]) and torch.equal(got["cam"], want["cam"])
    assert torch.equal(got["ctx"][:, :-1], want["ctx"][:, :-1])
    # the same float64 expressions in another association: a few ulp of float64 at most
    for k in ("ref2d", "ctx", "box2d"):
        err = (got[k] - want[k]).abs().max().item()
        assert err <= 1e-12 * max(1.0, want[k].abs().max().item()), (k, err)
    if variant == "empty":
        assert sel[0].numel() == 0, "camera 0 of the empty variant selects nothing: a camera without boxes in front of two with some"


def test_multi_depth_rows_follow_the_reference_order():
    """K = 3: the primaries first, then per k the valid primaries in row order; log-odds scaled by p_k / p_0; reference points of bin k."""
    case = fr.boxes_case()
    one, three = fr.case_rows(case, torch.float64, 1), fr.case_rows(case, torch.float64, fr.BOX_TOPK)
    M, V = one["cam"].numel(), int(three["valid"].sum())
    assert 0 < V < M, "the case must hold valid and invalid primaries (V=%d of %d)" % (V, M)
    assert three["cam"].numel() == M + 2 * V
    assert torch.equal(three["ref2d"][:M], one["ref2d"]) and torch.equal(three["ctx"][:M], one["ctx"])
    vrows = torch.nonzero(three["valid"])[:, 0]
    for k in (1, 2):
        blk = slice(M + (k - 1) * V, M + k * V)
        assert torch.equal(three["src"][blk], vrows) and torch.equal(three["bin"][blk], three["topk_idx"][vrows, k])
        assert torch.equal(three["ctx"][blk, -1], one["ctx"][vrows, -1] * three["ratio"][vrows, k])
        assert torch.equal(three["ctx"][blk, :-1], one["ctx"][vrows, :-1])
    assert bool((three["ratio"][:, 1:] < 1).all()) and bool((three["ratio"][:, 2] <= three["ratio"][:, 1]).all())


def test_gpu_inputs_leave_no_decision_to_rounding():
    """The conditions tests/test_foreign_props_gpu.py relies on, on the float64 reference alone.  A seed that fails them is changed,
    not the bar."""
    case = fr.boxes_case()
    rows = fr.case_rows(case, torch.float64, fr.BOX_TOPK)
    M = rows["cell"].shape[0]
    assert M == sum(b.shape[0] for b in case["boxes"]) == 49 and case["boxes"][1].shape[0] == 0
    # depth bins: ranks k and k + 1 apart for k < K (and rank K apart from rank K + 1), every proposal
    p = case["depth"].double()[rows["cam"][:M], rows["cell"][:, 1], rows["cell"][:, 0]]
    top = torch.sort(p, dim=1, descending=True).values[:, :fr.BOX_TOPK + 1]
    gap = (top[:, :-1] - top[:, 1:])
    print("[foreign] smallest gap between consecutive depth ranks: %.3e (relative %.3e)" % (gap.min().item(), (gap / top[:, :-1]).min().item()))
    assert bool((gap > 0).all()), "%d proposals hold tied depth bins among their best %d" % (int((gap <= 0).any(1).sum()), fr.BOX_TOPK + 1)
    # depth cell
    pos = rows["cell_pos"]
    dist = ((pos - torch.floor(pos)) - 0.5).abs()
    near = (dist < hr.CELL_MARGIN(rows["chain"], case["ds"])).any(dim=-1)
    assert torch.equal(near, case["deliberate"]), "centres inside the cell margin: rows %s, deliberate rows %s" % (
        torch.nonzero(near).flatten().tolist(), torch.nonzero(case["deliberate"]).flatten().tolist())
    assert bool((dist[case["deliberate"]] == 0).all()), "the deliberate centres sit exactly on half cells"
    # half to even, both parities, on both axes
    d = rows["cell"][case["deliberate"]]
    assert d.tolist() == [[2, 4], [6, 4], [0, 2], [case["wd"] - 1, case["hd"] - 1]]
    # the case holds what it promises: clamped centres on every side
    r = pos.round()
    assert bool((r[:, 0] < 0).any()) and bool((r[:, 1] < 0).any()) and bool((r[:, 0] > case["wd"] - 1).any()) and bool((r[:, 1] > case["hd"] - 1).any())

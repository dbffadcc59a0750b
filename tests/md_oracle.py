"""Test-side restatement of the reference's multi-depth 2D proposals (farhead.py:754-805, multi_depth_config.topk = K > 1).

oracle/far3d_oracle.py restates the topk = 1 path only and is not edited; MultiDepthOracle overrides its `_proposals` with the
K > 1 branch.  tools/gen_golden_multidepth.py pins it to the reference; tests/test_multidepth_cpu.py checks it against the fixtures.
"""
import torch

from oracle import far3d_oracle


def range_min_bin(cfg, range_min):
    """farhead.py:521-531 (inverse=True) as called at :758: fp32 torch on a one-element tensor, truncated to int64."""
    bin_size = 2 * (cfg["depth_max"] - cfg["depth_min"]) / (cfg["depth_bins"] * (1 + cfg["depth_bins"]))
    t = torch.tensor([range_min])
    return int((-0.5 + 0.5 * torch.sqrt(1 + 8 * (t - cfg["depth_min"]) / bin_size)).type(torch.int64).item())


def adopt_near_ties(device_bins, rel=1e-6):
    """forced_depth hook for MultiDepthOracle: where the device ranked the depth bins of a primary differently, adopt its order if
    the probabilities it swapped are within `rel` of each other (a near-tie decided by rounding), else keep the oracle's (and let
    the comparison fail).  device_bins: (M, K) int tensor in primary order."""
    def hook(probs, idx):
        dev = device_bins.to(idx.device).long()
        if dev.shape != idx.shape:
            return idx
        out = idx.clone()
        for m in torch.nonzero((dev != idx).any(1)).flatten().tolist():
            a, b = probs[m, idx[m]], probs[m, dev[m]]
            if torch.all((a - b).abs() <= rel * a.abs().clamp(min=1e-30)):
                out[m] = dev[m]
        return out
    return hook


class MultiDepthOracle(far3d_oracle.Far3DOracle):
    """cfg['multi_depth'] = dict(topk=K, range_min=R).  K <= 1 (or -1) is the parent's path.  `last_md` holds the latest frame's
    M, V, valid mask, per-row depth bins and log-odds ratios.  forced_depth (K > 1): callable(probs (M, D), idx (M, K)) -> idx."""

    def _proposals(self, outs_roi, feat_flatten, data, pad_hw, forced_depth=None):
        md = self.cfg.get("multi_depth") or {}
        K = int(md.get("topk", 1))
        if K <= 1:
            return super()._proposals(outs_roi, feat_flatten, data, pad_hw, forced_depth)
        h = "pts_bbox_head."
        pc = self.P(h + "pc_range")
        pred_depth = outs_roi["pred_depth"]                                   # (BN, D, H, W) softmax
        valid2d = outs_roi["valid_indices"]
        C = feat_flatten.shape[-1]
        ctx = feat_flatten[valid2d.repeat(1, 1, C)].reshape(-1, C)
        bbox_list, scores = outs_roi["bbox_list"], outs_roi["bbox2d_scores"]
        nums = [len(b) for b in bbox_list]
        if sum(nums) == 0:
            return None, None
        boxes = torch.cat(bbox_list, dim=0).to(self.dtype)
        ds = int(pad_hw[0] / pred_depth.shape[2])
        hmax, wmax = pred_depth.shape[2:]
        probs = []
        for i, b in enumerate(bbox_list):
            if nums[i] == 0:
                continue
            dm = pred_depth[i].permute(1, 2, 0).flatten(0, 1)                 # (HW, D)
            c2 = (b[:, :2] / ds).round().long()
            c2[c2 < 0] = 0
            c2[:, 0][c2[:, 0] >= wmax] = wmax - 1
            c2[:, 1][c2[:, 1] >= hmax] = hmax - 1
            flat = c2[:, 1] * (pad_hw[1] / ds) + c2[:, 0]
            probs.append(torch.gather(dm, 0, flat.long().unsqueeze(1).repeat(1, dm.shape[1])))
        probs = torch.cat(probs, dim=0)                                       # (M, D)
        vals, idx = torch.topk(probs, K, dim=1)
        if forced_depth is not None:                                          # test rigs: near-ties resolved the device's way
            idx = forced_depth(probs, idx)
            vals = torch.gather(probs, 1, idx)
        M = probs.shape[0]
        valid = idx[:, 0] >= range_min_bin(self.cfg, md.get("range_min", -1))
        vrows = torch.nonzero(valid).flatten()
        rows = torch.cat([torch.arange(M)] + [vrows] * (K - 1))               # k-major: all primaries, then k = 1 .. K-1
        bins = torch.cat([idx[:, 0]] + [idx[vrows, k] for k in range(1, K)])
        ratio = vals / vals[:, 0:1]
        dscore = torch.cat([ratio[:, 0]] + [ratio[vrows, k] for k in range(1, K)])
        thr = torch.tensor([0.1], dtype=self.dtype)
        scores = scores.clamp(min=1e-6)                                       # as the parent (static top-K fillers only)
        log_odds = (torch.log(scores / (1 - scores)) - torch.log(thr / (1 - thr)))[:, 0]
        ctx = torch.cat([ctx[rows], (log_odds[rows] * dscore)[:, None]], dim=-1)
        d = self._bin_to_depth(bins[:, None])
        coords = torch.cat([boxes[rows, :2], d], dim=1)
        coords = torch.cat([coords, torch.ones_like(coords[..., :1])], dim=-1)
        coords[..., :2] = coords[..., :2] * torch.maximum(coords[..., 2:3], torch.ones_like(coords[..., 2:3]) * 1e-5)
        i2l = data["lidar2img"].inverse().view(-1, 1, 4, 4)
        i2l = torch.cat([i2l[k].repeat(n, 1, 1) for k, n in enumerate(nums)], dim=0)[rows]
        c3 = torch.matmul(i2l, coords.unsqueeze(-1)).squeeze(-1)[..., :3]
        c3 = (c3 - pc[0:3]) / (pc[3:6] - pc[0:3])
        self.last_md = dict(M=M, V=int(valid.sum()), valid=valid, bins=bins, rows=rows, dscore=dscore, topk_idx=idx, ref2d=c3, ctx=ctx)
        return c3.unsqueeze(0), ctx.unsqueeze(0)

"""Seeded weights and inputs of the transformer-level fixture (tests/golden/far3d_transformer_seq.npz), shared by its generator
(tools/gen_golden_transformer.py) and tests/test_transformer_level_gpu.py.  Everything here is torch on the CPU."""
import torch

from far3d_amd import synth

RECIPE = dict(name="far3d_transformer_seq", weight_seed=31, input_seed=5, mask_seed=9, num_layers=3, bs=2, A=29, M=51, num_cams=2,
              level_hw=[[4, 6], [2, 3], [1, 2], [1, 1]], pad_hw=[64, 96], embed_dims=256, mask_p=0.3, first64_row=11)
INPUT_KEYS = ("query", "query_pos", "feat_flatten", "temp_memory", "temp_pos", "reference_points", "lidar2img", "pc_range")


def transformer_cfg(model_cfg, recipe=RECIPE):
    """The `transformer` dict of a Far3D model config (the reference's, or tests/golden/reference_config.json) at the fixture's sizes."""
    import copy
    cfg = copy.deepcopy(model_cfg["pts_bbox_head"]["transformer"])
    cfg["decoder"]["num_layers"] = recipe["num_layers"]
    for a in cfg["decoder"]["transformerlayers"]["attn_cfgs"]:
        if a["type"] == "DeformableFeatureAggregationCuda":
            a["num_cams"] = recipe["num_cams"]
    return cfg


def seed_weights(module, seed):
    """Fill every parameter of a transformer (reference or plugin: same state-dict names) from one generator, in name order: matrices
    N(0, 0.05^2) (the sampling offsets' ten times that: metres), LayerNorm gains 1 + N(0, 0.1^2), other vectors N(0, 0.1^2)."""
    g = torch.Generator().manual_seed(seed)
    sd = module.state_dict()
    with torch.no_grad():
        for name in sorted(sd):
            p = sd[name]
            r = torch.randn(p.shape, generator=g)
            if p.dim() > 1:
                r = r * (0.5 if name.endswith("learnable_fc.weight") else 0.05)
            elif name.endswith("weight"):     # the only 1-D weights are LayerNorm gains (norms.*, cam_embed.4)
                r = 1.0 + 0.1 * r
            else:
                r = 0.1 * r
            p.copy_(r.to(p.dtype))
    return sorted(sd)


def transformer_case(recipe=RECIPE):
    """-> dict of f32 CPU inputs in the reference's layout, plus spatial_flatten / level_start_index / img_metas."""
    g = torch.Generator().manual_seed(recipe["input_seed"])
    bs, A, M, N, C = recipe["bs"], recipe["A"], recipe["M"], recipe["num_cams"], recipe["embed_dims"]
    hw = [tuple(x) for x in recipe["level_hw"]]
    pad_hw = tuple(recipe["pad_hw"])
    starts, S = synth.level_starts(hw)
    _, _, l2i = synth.ring_cameras(N, pad_hw)      # the ring of the other fixtures; sample b sees it rotated by b cameras
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(query=rn(bs, A, C), query_pos=rn(bs, A, C), feat_flatten=rn(bs * N, S, C), temp_memory=rn(bs, M, C), temp_pos=rn(bs, M, C),
                reference_points=torch.rand(bs, A, 3, generator=g),
                lidar2img=torch.stack([torch.roll(l2i, b, 0) for b in range(bs)]).contiguous(),
                pc_range=torch.tensor(list(synth.PC_RANGE)), spatial_flatten=torch.tensor([list(x) for x in hw]),
                level_start_index=torch.tensor(starts), img_metas=[dict(pad_shape=[pad_hw + (3,)] * N)])


def transformer_mask(recipe=RECIPE):
    """(A, A + M) bool, True = excluded, p = mask_p; row first64_row has its first 64 keys excluded and the rest allowed; every other row
    keeps its own query as a key, so no row is fully masked."""
    g = torch.Generator().manual_seed(recipe["mask_seed"])
    A, Nk = recipe["A"], recipe["A"] + recipe["M"]
    m = torch.rand(A, Nk, generator=g) < recipe["mask_p"]
    m[torch.arange(A), torch.arange(A)] = False
    r = recipe["first64_row"]
    m[r, :64] = True
    m[r, 64:] = False
    assert not bool(m.all(dim=1).any())
    return m


def input_digest(case):
    """Per input: its float64 sum and 16 evenly spaced values -- what the fixture stores and the test asserts."""
    out = {}
    for k in INPUT_KEYS:
        flat = case[k].double().flatten()
        idx = torch.linspace(0, flat.numel() - 1, 16).long()
        out[k] = torch.cat([flat.sum()[None], flat[idx]])
    return out


def forward_args(case, attn_mask, to=lambda t: t):
    """Positional arguments of Detr3DTransformer.forward (models/utils/detr3d_transformer.py:58-70)."""
    t = lambda k: to(case[k])
    return (t("query"), t("query_pos"), t("feat_flatten"), t("spatial_flatten"), t("level_start_index"), t("temp_memory"), t("temp_pos"),
            None if attn_mask is None else to(attn_mask), t("reference_points"), t("pc_range"), dict(lidar2img=t("lidar2img")),
            case["img_metas"])

"""Golden fixture of the transformer level (BUILD CONTAINER ONLY: needs the reference checkout).

  python tools/gen_golden_transformer.py

Writes tests/golden/far3d_transformer_seq.npz: the reference's OWN Detr3DTransformer (models/utils/detr3d_transformer.py, executed where
it lies through oracle/refload.py), built from the reference config with num_layers = 3 and 2 cameras, run on the seeded weights and
inputs of tests/transformer_cases.py: two samples, 29 queries, 51 memory rows (80 keys), levels (4,6),(2,3),(1,2),(1,1) of a 64 x 96
pad.  Two runs -- attn_masks=None, and the bool mask of transformer_cases.transformer_mask (p = 0.3, one row with its first 64 keys
excluded, no fully masked row).  Stored per run: the float64 run of the same modules rounded to f32 (`states_*`), and per layer
dev64 = max |reference in fp32 - reference in fp64| (`dev64_*`), the reference's own rounding noise that the test's bar is a multiple
of.  Also: the recipe, each input's float64 sum and 16 samples, the reference's forward parameter names of the three classes and its
state-dict keys.  Data only."""
import copy
import inspect
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refload  # noqa: E402
from tests import transformer_cases as TC  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "far3d_transformer_seq.npz")
MAX_BYTES = 650 * 1000


def main():
    rc = dict(TC.RECIPE)
    mod = refload.ref("models.utils.detr3d_transformer")
    model_cfg, _ = refload.reference_model_cfg(num_cams=rc["num_cams"])
    cfg = TC.transformer_cfg(model_cfg, rc)
    cfg["decoder"]["transformerlayers"] = refload.ConfigDict(cfg["decoder"]["transformerlayers"])
    tr = refload.TRANSFORMER.build(cfg).eval()
    keys = TC.seed_weights(tr, rc["weight_seed"])
    tr64 = copy.deepcopy(tr).double()
    case = TC.transformer_case(rc)
    dbl = lambda t: t.double() if t.is_floating_point() else t
    out = dict(recipe=np.frombuffer(json.dumps(rc).encode(), dtype=np.uint8))
    for k, v in TC.input_digest(case).items():
        out["digest_" + k] = v.numpy()
    names = dict(state_dict=keys)
    for cls in ("Detr3DTransformer", "Detr3DTransformerDecoder", "Detr3DTemporalDecoderLayer"):
        names[cls] = [p for p in inspect.signature(getattr(mod, cls).forward).parameters if p != "self"]
    out["names"] = np.frombuffer(json.dumps(names).encode(), dtype=np.uint8)
    mask = TC.transformer_mask(rc)
    out["attn_mask"] = mask.numpy()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for run, m in (("nomask", None), ("mask", mask)):
            s32 = tr(*TC.forward_args(case, m))
            s64 = tr64(*TC.forward_args(case, m, dbl))
            assert s32.shape == (rc["num_layers"], rc["bs"], rc["A"], rc["embed_dims"]) and bool(torch.isfinite(s64).all())
            dev = (s32.double() - s64).abs().flatten(1).max(dim=1).values
            out["states_" + run] = s64.float().numpy()
            out["dev64_" + run] = dev.numpy()
            print("%s: |states| max %.3f, dev64 per layer %s" % (run, s64.abs().max().item(), ["%.3e" % d for d in dev.tolist()]))
        # the statement of the issue this fixture answers: sample 0 of the two-sample run equals the one-sample run
        one = {k: (v[:1] if k in ("query", "query_pos", "temp_memory", "temp_pos", "reference_points", "lidar2img") else v) for k, v in case.items()}
        one["feat_flatten"] = case["feat_flatten"][:rc["num_cams"]]
        d = (tr(*TC.forward_args(one, None))[:, 0] - tr(*TC.forward_args(case, None))[:, 0]).abs().max().item()
        print("reference fp32: sample 0 of bs = 2 vs bs = 1: %.2e" % d)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print("wrote %s (%d bytes)" % (OUT, size))
    assert size < MAX_BYTES


if __name__ == "__main__":
    main()

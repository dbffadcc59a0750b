"""CPU: the transformer-level surface exists -- the three decoder classes have forwards with the reference's parameter names (the lists
tests/golden/far3d_transformer_seq.npz recorded from the reference), the C ABI declares and exports far3d_attention_batched, and
MultiheadAttention's shape checks answer before any device is asked for."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import transformer_cases as TC
from tests.conftest import ROOT


def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "far3d_transformer_seq.npz"))


def _transformer():
    from far3d_amd import plugin
    model = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_config.json")))["model"]
    return plugin.TRANSFORMER.build(TC.transformer_cfg(model))


def test_forwards_carry_the_reference_parameter_names():
    from far3d_amd import plugin
    names = json.loads(bytes(_fixture()["names"]).decode())
    for cls in ("Detr3DTransformer", "Detr3DTransformerDecoder", "Detr3DTemporalDecoderLayer"):
        c = getattr(plugin, cls)
        assert "forward" in vars(c), "%s has no forward of its own" % cls
        got = [p for p in inspect.signature(c.forward).parameters if p != "self"]
        assert got == names[cls], "%s.forward%s, the reference has %s" % (cls, got, names[cls])


def test_fixture_recipe_inputs_and_state_dict_names():
    z = _fixture()
    assert json.loads(bytes(z["recipe"]).decode()) == TC.RECIPE
    case = TC.transformer_case()
    for k, v in TC.input_digest(case).items():
        assert np.array_equal(z["digest_" + k], v.numpy()), k
    mask = TC.transformer_mask()
    assert np.array_equal(z["attn_mask"], mask.numpy())
    assert bool(mask[TC.RECIPE["first64_row"], :64].all()) and not bool(mask.all(dim=1).any())
    tr = _transformer()
    assert sorted(tr.state_dict()) == json.loads(bytes(z["names"]).decode())["state_dict"]
    assert len(tr.decoder.layers) == 3 and z["states_mask"].shape == (3, 2, 29, 256) and z["dev64_nomask"].shape == (3,)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "far3d_transformer_seq.npz")) < 650 * 1000


def test_header_declares_and_library_exports_the_batched_attention(hip_lib):
    from far3d_amd import lib, ops
    src = open(os.path.join(ROOT, "include", "far3d_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+far3d_attention_batched\s*\(", src)
    assert hasattr(hip_lib, "far3d_attention_batched") and "far3d_attention_batched" in lib.SIGNATURES
    assert callable(ops.attention_batched)
    # argument checks of the C entry answer without a device: nothing is launched for a refused call
    rc = hip_lib.far3d_attention_batched(None, None, None, 0, None, 0, 1, 1, 1, 8, 32, 256, 256, 256, 256, 256, 256, 256, 256, 0.1,
                                         None, 0, 0, 0, None, None)
    assert rc == -1 and b"null pointer" in hip_lib.far3d_last_error()


def test_multihead_attention_shape_errors_need_no_device():
    from far3d_amd import plugin
    m = plugin.MultiheadAttention(256, 8, batch_first=True)
    q, k = torch.zeros(2, 5, 256), torch.zeros(2, 9, 256)
    with pytest.raises(ValueError, match=r"attn_mask must be \(5, 9\) or \(16, 5, 9\)"):
        m(q, k, k, attn_mask=torch.zeros(5, 8, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"attn_mask must be \(5, 9\) or \(16, 5, 9\)"):
        m(q, k, k, attn_mask=torch.zeros(2, 5, 9, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"key_padding_mask must be \(2, 9\)"):
        m(q, k, k, key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="one batch size"):
        m(q, k[:1], k[:1])
    m2 = plugin.MultiheadAttention(256, 8, batch_first=False)
    with pytest.raises(ValueError, match=r"attn_mask must be \(5, 9\) or \(16, 5, 9\)"):
        m2(q.transpose(0, 1), k.transpose(0, 1), k.transpose(0, 1), attn_mask=torch.zeros(9, 5, dtype=torch.bool))


def test_layer_refuses_a_wrong_number_of_masks_without_a_device():
    tr = _transformer()
    layer = tr.decoder.layers[0]
    z = torch.zeros(1, 4, 256)
    with pytest.raises(ValueError, match="3 attn_masks for 2 attention modules"):
        layer(z, z, None, None, None, None, None, None, None, None, None, attn_masks=[None, None, None])

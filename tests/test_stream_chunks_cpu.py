"""CPU: streams.stream_chunks -- how many scene streams one camera pass of StreamBatch holds -- and the per-image extent it bounds
(Far3DEngine.camera_image_span, from the same geometry backbone() allocates its buffers with)."""
import inspect

import pytest
import torch

from far3d_amd import weights
from far3d_amd.engine import Far3DEngine
from far3d_amd.streams import SPAN_LIMIT_BYTES, stream_chunks


def _covers(chunks, B):
    assert sum(chunks) == B and all(isinstance(c, int) and c >= 1 for c in chunks), chunks


def test_everything_fits_in_one_pass():
    assert stream_chunks(4, 7, 1000) == [4]
    assert stream_chunks(1, 2, 1) == [1]


def test_exactly_at_the_limit_and_one_over():
    # the kernels refuse a span of `limit` bytes and take limit - 1: 2 streams x 2 images x 10 bytes = 40
    assert stream_chunks(2, 2, 10, limit=41) == [2]
    assert stream_chunks(2, 2, 10, limit=40) == [1, 1]
    assert stream_chunks(5, 2, 10, limit=41) == [2, 2, 1]
    assert stream_chunks(5, 2, 10, limit=61) == [3, 2]


def test_a_stream_that_does_not_fit_runs_alone():
    # never an empty pass: one stream over the limit is a pass of its own, and fails or runs as the per-stream camera stage does
    assert stream_chunks(3, 7, SPAN_LIMIT_BYTES) == [1, 1, 1]
    assert stream_chunks(1, 7, 10 * SPAN_LIMIT_BYTES) == [1]


def test_the_cap_keyword():
    assert stream_chunks(3, 2, 100, max_streams=2) == [2, 1]
    assert stream_chunks(3, 2, 100, max_streams=1) == [1, 1, 1]
    assert stream_chunks(3, 2, 100, max_streams=8) == [3]
    assert stream_chunks(5, 2, 10, limit=61, max_streams=2) == [2, 2, 1]       # the cap never lifts the kernels' bound
    assert stream_chunks(5, 2, 10, limit=41, max_streams=3) == [2, 2, 1]
    with pytest.raises(ValueError, match="max_streams"):
        stream_chunks(3, 2, 100, max_streams=0)


@pytest.mark.parametrize("B", [1, 2, 3, 7, 16])
@pytest.mark.parametrize("span", [1, 1 << 20, 118 << 20, 1 << 31])
@pytest.mark.parametrize("cap", [None, 1, 3])
def test_chunks_cover_the_streams_in_order(B, span, cap):
    chunks = stream_chunks(B, 7, span, max_streams=cap)
    _covers(chunks, B)
    per = chunks[0]
    assert chunks == [per] * (B // per) + ([B % per] if B % per else [])       # full passes first, stream order kept
    if per > 1:
        assert per * 7 * span < SPAN_LIMIT_BYTES
    if cap is not None:
        assert per <= cap
    elif per < B:
        assert (per + 1) * 7 * span >= SPAN_LIMIT_BYTES                        # a pass is as large as the bound allows


def test_bad_sizes():
    for bad in (dict(streams=0), dict(images=0), dict(image_span=0)):
        with pytest.raises(ValueError, match="positive"):
            stream_chunks(**dict(dict(streams=2, images=2, image_span=8), **bad))


def _bare_engine(spec, pair, act):
    """An engine with the attributes the geometry reads and nothing else (no device, no weights)."""
    e = Far3DEngine.__new__(Far3DEngine)
    e.spec, e.pair, e.cs, e.prec = weights.VOV_SPECS[spec], pair, 2 if pair else 1, dict(act=act)
    return e


def test_span_is_the_geometry_the_backbone_allocates_from():
    """The benchmark geometry (7 cameras, 640 x 960, V-99, pair-stored maps): the stage-2 concat buffer of 160 x 240 x (128 + 5 * 128)
    channel pairs of bf16 is the largest map of an image, ~118 MB; two streams fit one pass, three do not."""
    e = _bare_engine("V-99-eSE", True, torch.bfloat16)
    geo = e.backbone_geometry(640, 960)
    assert geo["stem"] == (320, 480, 128)
    assert [(g["h"], g["w"]) for g in geo["stages"]] == [(160, 240), (80, 120), (40, 60), (20, 30)]
    assert geo["stages"][0] == dict(h=160, w=240, cat=1536, cat_next=0, out=512)
    assert geo["stages"][1]["cat"] == (256 + 5 * 160) * 2 and geo["stages"][1]["cat_next"] == (512 + 5 * 160) * 2
    span = e.camera_image_span(640, 960)
    assert span == 160 * 240 * 1536 * 2 == 117964800
    assert stream_chunks(2, 7, span) == [2] and stream_chunks(3, 7, span) == [2, 1] and stream_chunks(4, 7, span) == [2, 2]
    # fp32 maps of the same network: 768 channels of 4 bytes, the same span; plain bf16: half of it
    assert _bare_engine("V-99-eSE", False, torch.float32).camera_image_span(640, 960) == span
    assert _bare_engine("V-99-eSE", False, torch.bfloat16).camera_image_span(640, 960) == span // 2
    assert stream_chunks(4, 7, span // 2) == [4] and stream_chunks(6, 7, span // 2) == [5, 1]
    # odd sizes: the ceil-mode pooling of the stages
    assert [(g["h"], g["w"]) for g in e.backbone_geometry(70, 100)["stages"]] == [(18, 25), (9, 12), (4, 6), (2, 3)]
    # one source: backbone() takes its buffer shapes from the same method (it asserts the stem's and the pooled shapes against it),
    # and StreamBatch plans its passes from camera_image_span
    from far3d_amd import streams
    assert "backbone_geometry" in inspect.getsource(Far3DEngine.backbone)
    assert "backbone_geometry" in inspect.getsource(Far3DEngine.camera_image_span)
    assert "camera_image_span" in inspect.getsource(streams.StreamBatch._camera_streams)

"""CPU: engine.dedup_options -- the defaults filled in, None stays None, every refusal by the option's name."""
import pytest

from far3d_amd import engine


def _cfg(**over):
    return engine.default_cfg(**over)


def test_off_by_default_and_none_stays_none():
    assert _cfg()["dedup"] is None
    assert engine.dedup_options(_cfg()) is None
    assert engine.dedup_options(_cfg(dedup=None)) is None and engine.dedup_options(_cfg(dedup=False)) is None
    cfg = _cfg()
    del cfg["dedup"]                    # a cfg written before the option existed
    assert engine.dedup_options(cfg) is None


def test_defaults_are_filled_in():
    want = dict(mode="iou_bev", thr=0.5, class_aware=True, score_thr=0.0)
    assert engine.dedup_options(_cfg(dedup={})) == want and engine.dedup_options(_cfg(dedup=True)) == want
    assert engine.dedup_options(_cfg(dedup=dict(mode="centre", thr=2))) == dict(want, mode="centre", thr=2.0)
    got = engine.dedup_options(_cfg(dedup=dict(thr=0.3, class_aware=False, score_thr=0.2)))
    assert got == dict(mode="iou_bev", thr=0.3, class_aware=False, score_thr=0.2)
    assert isinstance(got["thr"], float)
    given = dict(thr=0.1)
    engine.dedup_options(_cfg(dedup=given))
    assert given == dict(thr=0.1)       # the caller's dict is left alone
    assert engine.dedup_options(_cfg(dedup=dict(thr=0.0)))["thr"] == 0.0
    assert engine.dedup_options(_cfg(dedup={}, max_num=1024))["mode"] == "iou_bev"


@pytest.mark.parametrize("dedup, over, match", [
    (dict(iou=0.5), {}, "unknown option.*iou"),
    (dict(thr=0.5, radius=1.0, klass=True), {}, "unknown option.*klass, radius"),
    (dict(mode="iou3d"), {}, "mode='iou3d'"),
    (dict(mode=0), {}, "mode=0"),
    (dict(thr=1.0), {}, r"thr=1\.0.*IoU"),
    (dict(thr=-0.1), {}, r"thr=-0\.1.*IoU"),
    (dict(thr=float("nan")), {}, "thr=nan"),
    (dict(mode="centre", thr=0.0), {}, r"thr=0\.0.*metres"),
    (dict(mode="centre", thr=float("inf")), {}, "thr=inf.*metres"),
    (dict(mode="centre", thr=float("nan")), {}, "thr=nan.*metres"),
    (dict(thr="0.5"), {}, "thr='0.5'"),
    (dict(class_aware=1), {}, "class_aware=1"),
    (dict(class_aware=None), {}, "class_aware=None"),
    (dict(score_thr=1.5), {}, r"score_thr=1\.5"),
    (dict(score_thr=-0.01), {}, r"score_thr=-0\.01"),
    (dict(score_thr=float("nan")), {}, "score_thr=nan"),
    ({}, dict(max_num=1025), "max_num=1025"),
])
def test_refusals_name_the_option(dedup, over, match):
    with pytest.raises(ValueError, match=match):
        engine.dedup_options(_cfg(dedup=dedup, **over))


def test_the_option_does_not_touch_the_others():
    assert engine.dedup_options(_cfg(track=dict(records=True))) is None
    assert engine.dedup_options(_cfg(dedup={}, track=dict(records=True)))["mode"] == "iou_bev"
    assert engine.track_options(_cfg(dedup={})) is None
    assert engine.track_options(_cfg(dedup={}, track=dict(records=True))) == dict(birth_thr=0.0, records=True)
    assert {k: v for k, v in _cfg(dedup={}).items() if k != "dedup"} == {k: v for k, v in _cfg().items() if k != "dedup"}


def test_the_detector_hands_the_option_to_the_engine_cfg():
    from far3d_amd import config, plugin
    model = config.default_model_cfg(num_query=60, num_propagated=16)
    assert plugin.build_detector(model).engine_cfg()["dedup"] is None
    want = dict(mode="iou_bev", thr=0.5, class_aware=True, score_thr=0.0)
    assert engine.dedup_options(plugin.build_detector(dict(model, dedup={})).engine_cfg()) == want      # an empty dict: on, all defaults
    assert engine.dedup_options(plugin.build_detector(dict(model, dedup=True)).engine_cfg()) == want
    assert engine.dedup_options(plugin.build_detector(dict(model, dedup=False)).engine_cfg()) is None
    det = plugin.build_detector(dict(model, dedup=dict(mode="centre", thr=1.5)))
    assert engine.dedup_options(det.engine_cfg()) == dict(want, mode="centre", thr=1.5)
    with pytest.raises(ValueError, match="unknown option.*radius"):
        engine.dedup_options(plugin.build_detector(dict(model, dedup=dict(radius=1.5))).engine_cfg())

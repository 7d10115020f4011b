"""train.DynamicLossScale and TrainConfig.loss_scale: argument rules and host-side state, no GPU."""
import math

import pytest


def test_defaults_and_host_state():
    from transception_amd.train import DynamicLossScale, SegLoss
    s = DynamicLossScale()
    assert (s.growth_factor, s.backoff_factor, s.growth_interval, s.min_scale, s.max_scale) == (2.0, 0.5, 2000, 1.0, 2.0 ** 24)
    assert s.state_dict() == {"scale": 65536.0, "growth_tracker": 0, "skipped": 0}          # no device state yet: nothing to read back
    s.load_state_dict({"scale": 512.0, "growth_tracker": 7, "skipped": 3})
    assert s.state_dict() == {"scale": 512.0, "growth_tracker": 7, "skipped": 3} and s.value() == 512.0 and s.skipped() == 3
    assert SegLoss(9, loss_scale=s).loss_scale is s
    assert SegLoss(9, loss_scale=4096).loss_scale == 4096.0 and SegLoss(9).loss_scale == 1.0
    w = s._words(8.0, 2, 5)                                                                  # the layout of include/transception_hip.h
    import torch
    assert w.tolist()[:2] == [8.0, 0.125] and w.view(torch.int32).tolist()[2:] == [2, 5]


@pytest.mark.parametrize("kw", [
    dict(growth_factor=0.5), dict(growth_factor=0.999),
    dict(backoff_factor=1.0), dict(backoff_factor=1.5), dict(backoff_factor=0.0), dict(backoff_factor=-0.5),
    dict(growth_interval=0), dict(growth_interval=-3), dict(growth_interval=2.5),
    dict(init_scale=0.5), dict(init_scale=2.0 ** 25), dict(init_scale=4.0, min_scale=8.0), dict(init_scale=64.0, max_scale=32.0),
    dict(min_scale=0.0, init_scale=0.0),
    dict(init_scale=math.inf, max_scale=math.inf), dict(init_scale=math.nan), dict(growth_factor=math.inf), dict(growth_factor=math.nan),
    dict(backoff_factor=math.nan), dict(min_scale=math.nan), dict(max_scale=math.inf), dict(max_scale=math.nan), dict(min_scale=-math.inf),
])
def test_bad_arguments_are_rejected(kw):
    from transception_amd.train import DynamicLossScale
    with pytest.raises(ValueError):
        DynamicLossScale(**kw)


def test_load_state_dict_rejects_a_bad_scale():
    from transception_amd.train import DynamicLossScale
    for bad in (0.0, -2.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            DynamicLossScale().load_state_dict({"scale": bad})


def test_train_config_loss_scale():
    from transception_amd.train import DynamicLossScale
    from transception_amd.trainer import TrainConfig, make_loss_scale
    assert TrainConfig(root_path="a", list_dir="b").loss_scale is None
    assert TrainConfig(root_path="a", list_dir="b", loss_scale="dynamic").loss_scale == "dynamic"
    assert TrainConfig(root_path="a", list_dir="b", loss_scale=4096.0).loss_scale == 4096.0
    assert make_loss_scale(None) == 1.0 and make_loss_scale(4096) == 4096.0
    assert isinstance(make_loss_scale("dynamic"), DynamicLossScale)
    for bad in ("auto", "Dynamic", 0.0, -1.0, math.inf, math.nan, True, [4096.0]):
        with pytest.raises(ValueError):
            TrainConfig(root_path="a", list_dir="b", loss_scale=bad)

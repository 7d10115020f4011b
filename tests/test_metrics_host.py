"""Host side of the device metrics (transception_amd.evaluate): the fp64 interpolation between the two order statistics the GPU returns,
the scratch-size helpers, and the refusal to run without a GPU.  No GPU needed."""
import numpy as np
import pytest
import torch


def test_interpolation_matches_numpy_percentile():
    """hd95_from_order_stats(n, d2 at floor(0.95 (n-1)), d2 at the next position) against numpy.percentile(sqrt(values), 95)."""
    from transception_amd.evaluate import hd95_from_order_stats
    g = np.random.default_rng(0)
    sets = [np.array([7]), np.array([3, 50]), np.array([50, 3]), np.full(37, 12), np.zeros(5, np.int64), np.arange(21), np.arange(101) ** 2]
    for n in (3, 4, 19, 20, 21, 22, 40, 41, 100, 1000, 4097):
        sets.append(g.integers(0, 3 * 511 ** 2, n))
        sets.append(g.integers(0, 6, n))
    for v in sets:
        s = np.sort(v)
        n = len(s)
        lo = int(np.floor(0.95 * (n - 1)))
        got = hd95_from_order_stats(n, int(s[lo]), int(s[min(lo + 1, n - 1)]))
        assert abs(got - np.percentile(np.sqrt(v.astype(np.float64)), 95)) <= 1e-12, (n, got)
    assert hd95_from_order_stats(1, 9, 9) == 3.0 and hd95_from_order_stats(37, 0, 0) == 0.0


def test_scratch_sizes():
    from transception_amd.evaluate import metrics_hist_bins, metrics_scratch_bytes
    assert metrics_hist_bins((148, 512, 512)) == 147 ** 2 + 2 * 511 ** 2 + 1 == 543852
    assert metrics_hist_bins((1, 5, 7)) == metrics_hist_bins((5, 7)) == 16 + 36 + 1
    assert metrics_hist_bins((1, 1, 1)) == 1
    n = 148 * 512 * 512
    # two uint8 surface maps, two int32 distance maps, nine uint32 histograms, int64 [2][9][3]
    assert metrics_scratch_bytes((148, 512, 512), 9) == 2 * n + 8 * n + 4 * 9 * 543852 + 8 * 54 == 407552224
    assert metrics_scratch_bytes((3, 4), 2) == 2 * 12 + 8 * 12 + 4 * 2 * 14 + 8 * 12
    with pytest.raises(ValueError):
        metrics_hist_bins((2, 3, 4, 5))


def test_device_metrics_have_no_cpu_fallback():
    from transception_amd.evaluate import evaluate_volume, hd95_device, inference, metrics_device
    lab = torch.zeros((2, 8, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics_device(lab, lab, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hd95_device(lab, lab)
    model = torch.nn.Conv2d(1, 9, 1)                                   # any module on the CPU: refused before it is called
    image, label = np.zeros((2, 32, 32), np.float32), np.zeros((2, 32, 32), np.uint8)
    for hd in (False, True):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            evaluate_volume(model, image, label, 9, (32, 32), with_hd95=hd, device_metrics=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference(model, [(image, label, "case")], 9, 32, device_metrics=True)


def test_train_config_carries_the_switch():
    from transception_amd.trainer import TrainConfig
    assert TrainConfig.__dataclass_fields__["device_metrics"].default is False

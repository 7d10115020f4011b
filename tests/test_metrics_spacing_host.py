"""Voxel spacing on the host metric path (transception_amd.evaluate.calculate_metric_percase, TrainConfig.voxelspacing): HD95 in physical
units against the brute-force definition (oracle.eval_hd95 with `spacing`).  No GPU."""
import numpy as np
import pytest

SPACINGS_3D = [(2.5, 0.75, 0.75), (5.0, 0.7, 0.8), (0.5, 1.0, 3.0)]


def _blob(shape, centre, radii, g, rough=0.3):
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    r2 = sum(((x - c) / r) ** 2 for x, c, r in zip(grids, centre, radii))
    return r2 + g.uniform(-rough, rough, shape) < 1.0


def _pairs():
    g = np.random.default_rng(99)
    return [(_blob((6, 14, 12), (2.5, 6, 5), (2, 4, 4), g), _blob((6, 14, 12), (3, 7, 6), (2.5, 5, 3), g)),
            (_blob((4, 10, 16), (0, 2, 3), (2, 4, 5), g), _blob((4, 10, 16), (3, 8, 12), (2, 3, 6), g))]


@pytest.mark.parametrize("spacing", SPACINGS_3D)
def test_calculate_metric_percase_with_spacing_follows_the_definition(spacing):
    """Dice is 2|P&G| / (|P|+|G|) whatever the spacing; HD95 within 1e-9 * max(1, want) of the brute-force definition: both sides take the
    percentile of square roots of sums of three fp64 squares below 1e4, which differ by a few ulps."""
    from oracle.transception_oracle import eval_hd95
    from transception_amd.evaluate import calculate_metric_percase
    for a, b in _pairs():
        assert a.any() and b.any()
        dice, hd = calculate_metric_percase(a, b, voxelspacing=spacing)
        want = eval_hd95(a, b, spacing=spacing)
        assert dice == 2.0 * (a & b).sum() / (a.sum() + b.sum())
        assert abs(hd - want) <= 1e-9 * max(1.0, want)
        assert hd != calculate_metric_percase(a, b)[1]                       # the spacing is really used
        assert calculate_metric_percase(a, b, voxelspacing=(1.0, 1.0, 1.0)) == calculate_metric_percase(a, b)


def test_two_d_and_scalar_spacing():
    from oracle.transception_oracle import eval_hd95
    from transception_amd.evaluate import calculate_metric_percase
    g = np.random.default_rng(3)
    a, b = _blob((18, 22), (8, 10), (5, 7), g), _blob((18, 22), (10, 12), (6, 5), g)
    want = eval_hd95(a, b, spacing=(0.5, 1.25))
    assert abs(calculate_metric_percase(a, b, voxelspacing=(0.5, 1.25))[1] - want) <= 1e-9 * max(1.0, want)
    twice = calculate_metric_percase(a, b, voxelspacing=2.0)[1]
    assert abs(twice - 2.0 * calculate_metric_percase(a, b)[1]) <= 1e-12 * twice


def test_empty_set_conventions_do_not_depend_on_spacing():
    from transception_amd.evaluate import calculate_metric_percase
    a = np.zeros((3, 6, 6), bool)
    b = a.copy()
    b[1, 2, 2] = True
    s = (2.5, 0.75, 0.75)
    assert calculate_metric_percase(b, a, voxelspacing=s) == (1.0, 0.0)          # only the prediction is non-empty
    assert calculate_metric_percase(a, b, voxelspacing=s) == (0.0, 0.0)
    assert calculate_metric_percase(a, a, voxelspacing=s) == (0.0, 0.0)


def test_train_config_has_no_spacing_by_default():
    from transception_amd.trainer import TrainConfig
    assert TrainConfig(root_path="", list_dir="").voxelspacing is None
    assert TrainConfig(root_path="", list_dir="", voxelspacing=(3.0, 0.8, 0.8)).voxelspacing == (3.0, 0.8, 0.8)

"""HD95 in physical units on the MI355X: `voxelspacing` through csrc/metrics.hip's fp64 kernels (tc_metric_edt_f64, tc_metric_select_f64) and
transception_amd.evaluate -- against the brute-force definition (oracle.eval_hd95 with `spacing`), scipy.ndimage and the host path.

The HD95 bound used throughout, |got - want| <= 1e-9 * max(1, want), is derived: a percentile is a continuous function of the pooled values,
every squared distance is a sum of three non-negative fp64 products, so the two sides differ by a few ulps of values below 1e4 (~1e-15
relative); the bound leaves several orders of magnitude over that and is far below the gap between two distinct answers that matter."""
import math

import numpy as np
import pytest
import torch

from metrics_util import DEV, dev as _dev, label_volume as _label_volume, mask_pairs

pytestmark = pytest.mark.gpu

MASK_PAIRS = mask_pairs(4711, (2, 4, 5), (1, 4, 3))
SPACINGS_3D = [(2.5, 0.75, 0.75), (5.0, 0.7, 0.8), (0.5, 1.0, 3.0)]
SPACING_2D = (0.5, 1.25)


def _close(got, want):
    return abs(got - want) <= 1e-9 * max(1.0, want)


@pytest.mark.parametrize("name,a,b", MASK_PAIRS, ids=[p[0] for p in MASK_PAIRS])
def test_hd95_device_with_spacing_follows_the_definition(name, a, b):
    """hd95_device(a, b, voxelspacing=s) against oracle.eval_hd95(a, b, spacing=s) within the module's bound, symmetric in its arguments,
    and 0.0 of a mask against itself."""
    from oracle.transception_oracle import eval_hd95
    from transception_amd.evaluate import hd95_device
    assert a.any() and b.any()
    for s in (SPACINGS_3D if a.ndim == 3 else [SPACING_2D]):
        want = eval_hd95(a, b, spacing=s)
        got = hd95_device(_dev(a), _dev(b), voxelspacing=s)
        back = hd95_device(_dev(b.astype(np.uint8)), _dev(a.astype(np.uint8)), voxelspacing=s)
        print(f"{name} {s}: device {got!r} back {back!r} oracle {want!r}")
        assert want > 0 and _close(got, want) and _close(back, want)
        assert got == back                                                             # one pooled multiset either way
        assert hd95_device(_dev(a), _dev(a), voxelspacing=s) == 0.0 and hd95_device(_dev(b), _dev(b), voxelspacing=s) == 0.0


def test_weighted_distance_maps_against_scipy():
    """edt_squared(surf, k, voxelspacing=s) against scipy's distance_transform_edt(sampling=s) ** 2 on a 24 x 96 x 80 volume with 9 labels,
    within 1e-12 relative element by element; +inf everywhere for an absent class; the int32 map without spacing is what it was."""
    from scipy.ndimage import distance_transform_edt
    from transception_amd.evaluate import edt_squared, surfaces_counts
    g = np.random.default_rng(17)
    shape = (24, 96, 80)
    pred = _label_volume(shape, g, 8, skip=(5,))
    gt = _label_volume(shape, g, 8, skip=(3,))
    pred[0, :, :40] = 2                                                # a class that lies on the array border
    gt[:, 90:, :] = 6
    sp, sg, _ = surfaces_counts(_dev(pred), _dev(gt), 9)
    worst = 0.0
    for surf, absent in ((sp, 5), (sg, 3)):
        want_surf = surf.cpu().numpy()
        for k in range(1, 9):
            for s in (SPACINGS_3D[0], SPACINGS_3D[2]):
                d2 = edt_squared(surf, k, voxelspacing=s).cpu().numpy()
                assert d2.dtype == np.float64 and d2.shape == shape
                if k == absent:
                    assert not (want_surf == k).any() and np.isposinf(d2).all()
                    continue
                assert (want_surf == k).any()
                want = distance_transform_edt(want_surf != k, sampling=s) ** 2
                err = np.abs(d2 - want)
                worst = max(worst, float((err / np.maximum(want, 1e-300)).max()))
                assert (err <= 1e-12 * want).all(), (k, s)
            d2i = edt_squared(surf, k).cpu().numpy()
            assert d2i.dtype == np.int32
            if k != absent:
                np.testing.assert_array_equal(d2i, np.rint(distance_transform_edt(want_surf != k) ** 2).astype(np.int64))
                unit = edt_squared(surf, k, voxelspacing=1.0).cpu().numpy()
                np.testing.assert_array_equal(unit, d2i.astype(np.float64))     # sums of squared integers are exact in fp64
    print(f"largest relative difference from scipy: {worst:.3e}")
    assert bool((sp[0] == 2).any())
    sl = edt_squared(sp[0], 2, voxelspacing=SPACING_2D).cpu().numpy()      # [H,W]: true 2-D, no z pass
    want = distance_transform_edt(sp[0].cpu().numpy() != 2, sampling=SPACING_2D) ** 2
    assert (np.abs(sl - want) <= 1e-12 * want).all()


def _compare_with_host(pred, gt, spacing, classes=9):
    from transception_amd.evaluate import calculate_metric_percase, metrics_device
    got = metrics_device(_dev(pred), _dev(gt), classes, voxelspacing=spacing)
    want = [calculate_metric_percase(pred == k, gt == k, voxelspacing=spacing) for k in range(1, classes)]
    assert len(got) == classes - 1
    for k, ((d, h), (wd, wh)) in enumerate(zip(got, want), start=1):
        print(f"class {k}: device ({d!r}, {h!r}) host ({wd!r}, {wh!r})")
    for k, ((d, h), (wd, wh)) in enumerate(zip(got, want), start=1):
        assert abs(d - wd) <= 1e-12 and _close(h, wh), k
    return got, want


def test_metrics_device_with_spacing_vs_the_host_path_on_long_lines():
    """40 x 256 x 224 at spacing (3.0, 0.8, 0.8): lines longer than a wave and than one LDS tile's width; class 4 absent from the prediction,
    6 from the ground truth, 8 from both.  Dice within 1e-12, HD95 within the module's bound of the host `calculate_metric_percase` with the
    same spacing; the empty-set conventions (utils.py:53-60) exact."""
    shape = (40, 256, 224)
    gt = _label_volume(shape, np.random.default_rng(41), 8, skip=(6, 8))
    pred = np.roll(_label_volume(shape, np.random.default_rng(41), 8, skip=(4, 8)), (1, 3, -2), (0, 1, 2))     # the same organs, displaced
    assert not (pred == 4).any() and (gt == 4).any() and (pred == 6).any() and not (gt == 6).any()
    got, want = _compare_with_host(pred, gt, (3.0, 0.8, 0.8))
    assert got[3] == (0.0, 0.0) and got[5] == (1.0, 0.0) and got[7] == (0.0, 0.0)
    assert all(0 < wd < 1 and wh > 0 for wd, wh in (want[i] for i in (0, 1, 2, 4, 6)))


def test_a_line_longer_than_1024_takes_the_narrowest_tile():
    """2 x 1100 x 64: the y pass stages 1100-voxel lines, 8 to a tile."""
    shape = (2, 1100, 64)
    g = np.random.default_rng(43)
    gt = _label_volume(shape, g, 3)
    pred = np.roll(gt, (0, 37, 3), (0, 1, 2))
    pred[:, :40] = 0                                                   # (what the roll wrapped round)
    pred[1, 1090:, :5] = 3                                             # a far outlier: long scans along y
    assert all((pred == k).any() and (gt == k).any() for k in (1, 2, 3))
    _, want = _compare_with_host(pred, gt, (3.0, 0.8, 0.8), classes=4)
    assert all(wh > 0 for _, wh in want)


def test_unit_spacing_and_scaling():
    """voxelspacing (1, 1, 1) is the integer path's result within 1e-12, and (2, 2, 2) twice it within 1e-12 relative."""
    from transception_amd.evaluate import hd95_device, metrics_device
    g = np.random.default_rng(19)
    shape = (10, 48, 40)
    pred, gt = _dev(_label_volume(shape, g, 5)), _dev(_label_volume(shape, g, 5))
    base = metrics_device(pred, gt, 6)
    unit = metrics_device(pred, gt, 6, voxelspacing=(1.0, 1.0, 1.0))
    twice = metrics_device(pred, gt, 6, voxelspacing=(2.0, 2.0, 2.0))
    scalar = metrics_device(pred, gt, 6, voxelspacing=2.0)
    assert sum(h > 0 for _, h in base) >= 4
    for (d0, h0), (d1, h1), (d2, h2) in zip(base, unit, twice):
        assert d0 == d1 == d2 and abs(h1 - h0) <= 1e-12 and abs(h2 - 2.0 * h0) <= 1e-12 * max(2.0 * h0, 1.0)
    assert scalar == twice
    a, b = (pred == 2), (gt == 2)
    assert abs(hd95_device(a, b, voxelspacing=(1.0, 1.0, 1.0)) - hd95_device(a, b)) <= 1e-12


def test_determinism_and_inputs_untouched():
    """Two runs give bit-identical (n, d2_lo, d2_hi) and float64 maps; the label volumes are not modified; the record of a class that was
    not selected is left alone and the selected one is overwritten (the header's rule)."""
    from transception_amd._lib import TC_METRIC_SELECT_WORK_BYTES, lib
    from transception_amd.evaluate import edt_squared, metrics_order_stats, metrics_scratch_bytes, surfaces_counts
    g = np.random.default_rng(23)
    shape = (10, 48, 40)
    s = (2.5, 0.75, 0.75)
    pred_h, gt_h = _label_volume(shape, g, 5), _label_volume(shape, g, 5)
    pred, gt = _dev(pred_h), _dev(gt_h)
    r1 = metrics_order_stats(pred, gt, 6, voxelspacing=s).cpu()
    r2 = metrics_order_stats(pred, gt, 6, voxelspacing=s).cpu()
    assert torch.equal(r1, r2) and int(r1[1, 1:, 0].min()) > 0
    np.testing.assert_array_equal(pred.cpu().numpy(), pred_h)
    np.testing.assert_array_equal(gt.cpu().numpy(), gt_h)
    assert torch.equal(r1[1, :, 0], metrics_order_stats(pred, gt, 6).cpu()[1, :, 0])        # the pooled counts do not depend on spacing
    d2 = r1[1, 1:, 1:].contiguous().view(torch.float64)
    assert bool((d2[:, 0] <= d2[:, 1]).all()) and bool((d2 > 0).all()) and bool(torch.isfinite(d2).all())
    sp, sg, _ = surfaces_counts(pred, gt, 6)
    dp, dg = edt_squared(sp, 2, voxelspacing=s), edt_squared(sg, 2, voxelspacing=s)
    assert torch.equal(edt_squared(sp, 2, torch.full_like(dp, -5.0), voxelspacing=s), dp)   # OVERWRITTEN, and the same bits again
    # the order statistics against a sort of the pooled values (this check may sort; the library does not)
    pool = torch.cat((dg[sp == 2], dp[sg == 2])).sort().values
    n = pool.numel()
    lo = int(math.floor(0.95 * (n - 1)))
    assert n == int(r1[1, 2, 0]) and float(pool[lo]) == float(d2[1, 0]) and float(pool[min(lo + 1, n - 1)]) == float(d2[1, 1])
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    work = torch.full((TC_METRIC_SELECT_WORK_BYTES,), 0xAB, dtype=torch.uint8, device=DEV)  # dirty work is fine: the entry zeroes it
    out = torch.full((6, 3), -9, dtype=torch.int64, device=DEV)
    L.tc_metric_select_f64(sp.data_ptr(), sg.data_ptr(), dp.data_ptr(), dg.data_ptr(), 2, 6, *shape, work.data_ptr(), out.data_ptr(), stream)
    assert torch.equal(out[2].cpu(), r1[1, 2]) and bool((out[[0, 1, 3, 4, 5]] == -9).all())
    n_vox = shape[0] * shape[1] * shape[2]
    assert metrics_scratch_bytes(shape, 6, voxelspacing=s) == 2 * n_vox + 16 * n_vox + TC_METRIC_SELECT_WORK_BYTES + 8 * 2 * 6 * 3
    assert metrics_scratch_bytes(shape, 6) == metrics_scratch_bytes(shape, 6, None)


def test_bad_spacing_and_arguments_raise_without_launching():
    from transception_amd._lib import TC_METRIC_SELECT_WORK_BYTES, TcError, lib
    from transception_amd.evaluate import edt_squared, hd95_device, metrics_device
    shape = (2, 8, 8)
    u8 = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    u8[1, 3, 3] = 1
    for bad in [(1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, -0.5, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0), 0.0,
                -1.0, float("nan")]:
        for call in (lambda: metrics_device(u8, u8, 2, voxelspacing=bad), lambda: hd95_device(u8, u8, voxelspacing=bad),
                     lambda: edt_squared(u8, 1, voxelspacing=bad)):
            with pytest.raises(ValueError, match="voxelspacing"):
                call()
    with pytest.raises(ValueError, match="voxelspacing"):
        hd95_device(u8[0], u8[0], voxelspacing=(1.0, 1.0, 1.0))                       # three components for [H,W]
    cpu = torch.zeros(shape, dtype=torch.uint8)
    for call in (lambda: metrics_device(cpu, cpu, 2, voxelspacing=(1.0, 1.0, 1.0)), lambda: hd95_device(cpu, cpu, voxelspacing=(1.0, 1.0, 1.0)),
                 lambda: edt_squared(cpu, 1, voxelspacing=(1.0, 1.0, 1.0))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    zero = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    f64 = torch.zeros(shape, dtype=torch.float64, device=DEV)
    work = torch.zeros(TC_METRIC_SELECT_WORK_BYTES, dtype=torch.uint8, device=DEV)
    out = torch.zeros((16, 3), dtype=torch.int64, device=DEV)
    p, q, w, o = zero.data_ptr(), f64.data_ptr(), work.data_ptr(), out.data_ptr()
    nan, inf = float("nan"), float("inf")
    bad = [
        lambda: L.tc_metric_edt_f64(None, 1, q, 2, 8, 8, 1, 1.0, 1.0, 1.0, stream),
        lambda: L.tc_metric_edt_f64(p, 1, None, 2, 8, 8, 1, 1.0, 1.0, 1.0, stream),
        lambda: L.tc_metric_edt_f64(p, 0, q, 2, 8, 8, 1, 1.0, 1.0, 1.0, stream),
        lambda: L.tc_metric_edt_f64(p, 16, q, 2, 8, 8, 1, 1.0, 1.0, 1.0, stream),
        lambda: L.tc_metric_edt_f64(p, 1, q, 2, 4096, 8, 1, 1.0, 1.0, 1.0, stream),             # a line longer than 2048
        lambda: L.tc_metric_edt_f64(p, 1, q, 0, 8, 8, 1, 1.0, 1.0, 1.0, stream),
        lambda: L.tc_metric_edt_f64(p, 1, q, 2048, 1024, 1024, 1, 1.0, 1.0, 1.0, stream),       # D*H*W >= 2^31
        lambda: L.tc_metric_edt_f64(p, 1, q, 2, 8, 8, 1, 0.0, 1.0, 1.0, stream),
        lambda: L.tc_metric_edt_f64(p, 1, q, 2, 8, 8, 1, 1.0, -1.0, 1.0, stream),
        lambda: L.tc_metric_edt_f64(p, 1, q, 2, 8, 8, 1, 1.0, 1.0, nan, stream),
        lambda: L.tc_metric_edt_f64(p, 1, q, 2, 8, 8, 1, 1.0, inf, 1.0, stream),
        lambda: L.tc_metric_select_f64(None, p, q, q, 1, 9, 2, 8, 8, w, o, stream),
        lambda: L.tc_metric_select_f64(p, p, q, None, 1, 9, 2, 8, 8, w, o, stream),
        lambda: L.tc_metric_select_f64(p, p, q, q, 1, 9, 2, 8, 8, None, o, stream),
        lambda: L.tc_metric_select_f64(p, p, q, q, 1, 9, 2, 8, 8, w, None, stream),
        lambda: L.tc_metric_select_f64(p, p, q, q, 0, 9, 2, 8, 8, w, o, stream),
        lambda: L.tc_metric_select_f64(p, p, q, q, 9, 9, 2, 8, 8, w, o, stream),                # class outside its range
        lambda: L.tc_metric_select_f64(p, p, q, q, 1, 17, 2, 8, 8, w, o, stream),
        lambda: L.tc_metric_select_f64(p, p, q, q, 1, 9, 2, 8, 4096, w, o, stream),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(TcError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    torch.cuda.synchronize()                                                           # the CUDA error state is clean
    assert float(f64.abs().sum()) == 0.0 and int(out.abs().sum()) == 0 and int(work.sum()) == 0     # nothing ran


def _model():
    from transception_amd import MSTransception
    from transception_amd.seeded_init import seeded_state_dict
    m = MSTransception(num_classes=9)
    m.load_state_dict(seeded_state_dict(), strict=True)
    return m.to(DEV).eval()


def test_spacing_through_the_public_path():
    """evaluate_volume / inference with voxelspacing: device_metrics=True against the host metric of the same prediction (same model, same
    device forward and zooms on both sides), Dice within 1e-12 and HD95 within the module's bound; Dice-only results do not see the spacing."""
    from transception_amd.evaluate import evaluate_volume, inference
    g = np.random.default_rng(5)
    m = _model()
    s = (2.5, 0.75, 0.75)
    vols = []
    for c in range(2):
        D = 4 + c
        image = g.random((D, 96, 80)).astype(np.float32)
        label = g.integers(0, 9, (D, 96, 80)).astype(np.uint8)
        vols.append((image, label, f"case{c}"))
    image, label, _ = vols[0]
    host = evaluate_volume(m, image, label, 9, (64, 64), batch=2, with_hd95=True, device_metrics=False, voxelspacing=s)
    dev = evaluate_volume(m, image, label, 9, (64, 64), batch=2, with_hd95=True, device_metrics=True, voxelspacing=s)
    plain = evaluate_volume(m, image, label, 9, (64, 64), batch=2, with_hd95=True, device_metrics=True)
    print("host", host, "\ndevice", dev, "\nunit spacing", plain)
    assert len(dev) == len(host) == 8
    assert sum(0 < wd < 1 and wh > 0 for wd, wh in host) >= 4          # real surfaces on both sides, not the empty-set conventions
    for (d, h), (wd, wh) in zip(dev, host):
        assert abs(d - wd) <= 1e-12 and _close(h, wh)
    assert any(h != ph for (_, h), (_, ph) in zip(dev, plain))         # millimetres, not voxels
    for device_metrics in (False, True):
        assert evaluate_volume(m, image, label, 9, (64, 64), batch=2, device_metrics=device_metrics, voxelspacing=s) == \
            evaluate_volume(m, image, label, 9, (64, 64), batch=2, device_metrics=device_metrics)
    a = inference(m, vols, 9, 64, batch=2, voxelspacing=s)
    b = inference(m, vols, 9, 64, batch=2, device_metrics=True, voxelspacing=s)
    assert abs(a[0] - b[0]) <= 1e-12 and _close(b[1], a[1])

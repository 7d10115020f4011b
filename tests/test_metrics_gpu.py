"""Dice and HD95 on the MI355X (csrc/metrics.hip, transception_amd.evaluate.metrics_device): `calculate_metric_percase` of the reference
(utils.py:50-60) in exact integer arithmetic -- surface maps, separable squared Euclidean distance transform, histogram of squared
distances, two order statistics -- against the brute-force definition (oracle.eval_hd95), scipy.ndimage and the host path."""
import numpy as np
import pytest
import torch

from metrics_util import DEV, dev as _dev, label_volume as _label_volume, mask_pairs

pytestmark = pytest.mark.gpu

MASK_PAIRS = mask_pairs(2024, (1, 3, 6), (2, 5, 3))


@pytest.mark.parametrize("name,a,b", MASK_PAIRS, ids=[p[0] for p in MASK_PAIRS])
def test_hd95_device_follows_the_definition(name, a, b):
    """|hd95_device - oracle.eval_hd95| <= 1e-9.  The bound is derived: both sides interpolate in fp64 between the square roots of the same two
    integers (values < 1e3, ulp ~1e-13), and two different answers are at least sqrt(n+1) - sqrt(n) > 5e-4 apart for n < 1e6."""
    from oracle.transception_oracle import eval_hd95
    from transception_amd.evaluate import hd95_device
    assert a.any() and b.any()
    want = eval_hd95(a, b)
    got = hd95_device(_dev(a), _dev(b))
    back = hd95_device(_dev(b.astype(np.uint8)), _dev(a.astype(np.uint8)))
    print(f"{name}: device {got!r} oracle {want!r}")
    assert abs(got - want) <= 1e-9 and abs(back - want) <= 1e-9
    assert hd95_device(_dev(a), _dev(a)) == 0.0 and hd95_device(_dev(b), _dev(b)) == 0.0


def test_hd95_device_rejects_what_the_host_rejects():
    from transception_amd.evaluate import hd95_device
    a = np.zeros((3, 6, 6), bool)
    b = a.copy()
    b[1, 2, 2] = True
    for x, y in ((a, b), (b, a), (a, a)):
        with pytest.raises(RuntimeError, match="non-empty"):
            hd95_device(_dev(x), _dev(y))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hd95_device(torch.from_numpy(b), torch.from_numpy(b))


def test_intermediate_results_are_exact():
    """Surface maps, squared distance maps and counts against scipy.ndimage / numpy on a 24 x 96 x 80 volume with 9 labels: no tolerance."""
    from scipy.ndimage import binary_erosion, distance_transform_edt
    from transception_amd._lib import TC_METRIC_NO_SOURCE
    from transception_amd.evaluate import edt_squared, surfaces_counts
    g = np.random.default_rng(7)
    shape = (24, 96, 80)
    pred = _label_volume(shape, g, 8, skip=(5,))
    gt = _label_volume(shape, g, 8, skip=(3,))
    pred[0, :, :40] = 2                                                # a class that lies on the array border
    gt[:, 90:, :] = 6
    sp, sg, counts = surfaces_counts(_dev(pred), _dev(gt), 9)
    for lab, surf in ((pred, sp), (gt, sg)):
        want = np.zeros(shape, np.uint8)
        for k in range(1, 9):
            m = lab == k
            want += (k * (m ^ binary_erosion(m))).astype(np.uint8)    # connectivity 1, border_value 0
        np.testing.assert_array_equal(surf.cpu().numpy(), want)
        for k in range(1, 9):
            d2 = edt_squared(surf, k).cpu().numpy()
            assert d2.dtype == np.int32
            if (want == k).any():
                np.testing.assert_array_equal(d2, np.rint(distance_transform_edt(want != k) ** 2).astype(np.int64))
            else:
                assert k in (3, 5)
                np.testing.assert_array_equal(d2, np.full(shape, TC_METRIC_NO_SOURCE, np.int32))
    want_counts = np.array([[((pred == k) & (gt == k)).sum(), (pred == k).sum(), (gt == k).sum()] for k in range(9)], np.int64)
    np.testing.assert_array_equal(counts.cpu().numpy(), want_counts)


def test_metrics_device_vs_the_host_path_on_long_lines():
    """40 x 256 x 224: lines longer than a wave and than one LDS tile's width; class 4 absent from the prediction, 6 from the ground truth, 8 from both.
    Dice within 1e-12, HD95 within 1e-9 of the host `calculate_metric_percase`; the empty-set conventions (utils.py:53-60) exact."""
    from transception_amd.evaluate import calculate_metric_percase, metrics_device
    shape = (40, 256, 224)
    gt = _label_volume(shape, np.random.default_rng(31), 8, skip=(6, 8))
    pred = np.roll(_label_volume(shape, np.random.default_rng(31), 8, skip=(4, 8)), (1, 3, -2), (0, 1, 2))     # the same organs, displaced
    assert not (pred == 4).any() and (gt == 4).any() and (pred == 6).any() and not (gt == 6).any()
    got = metrics_device(_dev(pred), _dev(gt), 9)
    want = [calculate_metric_percase(pred == k, gt == k) for k in range(1, 9)]
    assert len(got) == 8
    for k, ((d, h), (wd, wh)) in enumerate(zip(got, want), start=1):
        print(f"class {k}: device ({d!r}, {h!r}) host ({wd!r}, {wh!r})")
    for k, ((d, h), (wd, wh)) in enumerate(zip(got, want), start=1):
        assert abs(d - wd) <= 1e-12 and abs(h - wh) <= 1e-9, k
    assert got[3] == (0.0, 0.0) and got[5] == (1.0, 0.0) and got[7] == (0.0, 0.0)
    assert all(0 < wd < 1 and wh > 0 for wd, wh in (want[i] for i in (0, 1, 2, 4, 6)))


def _model():
    from transception_amd import MSTransception
    from transception_amd.seeded_init import seeded_state_dict
    m = MSTransception(num_classes=9)
    m.load_state_dict(seeded_state_dict(), strict=True)
    return m.to(DEV).eval()


def test_device_metrics_through_the_public_path():
    """evaluate_volume / inference with device_metrics=True against the host metric of the same prediction (same model, same device
    forward and zooms on both sides): Dice within 1e-12, HD95 within 1e-9; a 96 x 80 volume at network size 64 x 64, so both zooms run."""
    from transception_amd.evaluate import evaluate_volume, inference
    g = np.random.default_rng(5)
    m = _model()
    vols = []
    for c in range(2):
        D = 4 + c
        image = g.random((D, 96, 80)).astype(np.float32)
        label = g.integers(0, 9, (D, 96, 80)).astype(np.uint8)
        vols.append((image, label, f"case{c}"))
    image, label, _ = vols[0]
    host = evaluate_volume(m, image, label, 9, (64, 64), batch=2, with_hd95=True, device_metrics=False)
    dev = evaluate_volume(m, image, label, 9, (64, 64), batch=2, with_hd95=True, device_metrics=True)
    print("host", host, "\ndevice", dev)
    assert len(dev) == len(host) == 8
    assert sum(0 < wd < 1 and wh > 0 for wd, wh in host) >= 4          # real surfaces on both sides, not the empty-set conventions
    for (d, h), (wd, wh) in zip(dev, host):
        assert abs(d - wd) <= 1e-12 and abs(h - wh) <= 1e-9
    dice_host = evaluate_volume(m, image, label, 9, (64, 64), batch=2)
    dice_dev = evaluate_volume(m, image, label, 9, (64, 64), batch=2, device_metrics=True)
    assert len(dice_dev) == 8 and max(abs(a - b) for a, b in zip(dice_dev, dice_host)) <= 1e-12
    a = inference(m, vols, 9, 64, batch=2)
    b = inference(m, vols, 9, 64, batch=2, device_metrics=True)
    assert abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-9


def test_determinism_and_buffer_rules():
    """Two runs give bit-identical (n, d2_lo, d2_hi); counts and histograms are ACCUMULATED (the header's rule): non-zero buffers passed in
    come back with the new values added; surface maps, distance maps and the order statistics are overwritten."""
    from transception_amd._lib import lib
    from transception_amd.evaluate import edt_squared, metrics_hist_bins, metrics_order_stats, surfaces_counts
    g = np.random.default_rng(13)
    shape = (10, 48, 40)
    pred, gt = _dev(_label_volume(shape, g, 5)), _dev(_label_volume(shape, g, 5))
    r1 = metrics_order_stats(pred, gt, 6).cpu()
    r2 = metrics_order_stats(pred, gt, 6).cpu()
    assert torch.equal(r1, r2) and int(r1[1, 1:, 0].min()) > 0
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    sp, sg, counts = surfaces_counts(pred, gt, 6)
    sp2, sg2 = torch.full_like(sp, 77), torch.full_like(sg, 77)
    counts2 = torch.full_like(counts, 1000)
    L.tc_metric_surfaces(pred.data_ptr(), gt.data_ptr(), sp2.data_ptr(), sg2.data_ptr(), counts2.data_ptr(), *shape, 6, 1, stream)
    assert torch.equal(sp2, sp) and torch.equal(sg2, sg) and torch.equal(counts2, counts + 1000)
    nbins = metrics_hist_bins(shape)
    dp, dg = edt_squared(sp, 2), edt_squared(sg, 2)
    assert torch.equal(edt_squared(sp, 2, torch.full_like(dp, -5)), dp)
    h0 = torch.zeros((6, nbins), dtype=torch.int32, device=DEV)
    h1 = torch.full((6, nbins), 3, dtype=torch.int32, device=DEV)
    for h in (h0, h1):
        L.tc_metric_hist(sp.data_ptr(), sg.data_ptr(), dp.data_ptr(), dg.data_ptr(), 2, h.data_ptr(), nbins, 6, *shape, stream)
    assert torch.equal(h1, h0 + 3) and int(h0[2].sum()) == int(r1[1, 2, 0]) and int(h0[:2].sum()) == 0 and int(h0[3:].sum()) == 0
    out = torch.full((6, 3), -9, dtype=torch.int64, device=DEV)
    L.tc_metric_select(h0.data_ptr(), nbins, 6, out.data_ptr(), stream)
    assert torch.equal(out[2].cpu(), r1[1, 2]) and int(out[[0, 1, 3, 4, 5]].abs().sum()) == 0


def test_bad_arguments_raise_without_launching():
    from transception_amd._lib import TcError, lib
    from transception_amd.evaluate import metrics_hist_bins
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    shape = (2, 8, 8)
    u8 = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    i32 = torch.zeros(shape, dtype=torch.int32, device=DEV)
    cnt = torch.zeros((16, 3), dtype=torch.int64, device=DEV)
    nbins = metrics_hist_bins(shape)
    hist = torch.zeros((16, nbins), dtype=torch.int32, device=DEV)
    p, q, c, h = u8.data_ptr(), i32.data_ptr(), cnt.data_ptr(), hist.data_ptr()
    bad = [
        lambda: L.tc_metric_surfaces(None, p, p, p, c, 2, 8, 8, 9, 1, stream),
        lambda: L.tc_metric_surfaces(p, p, p, p, None, 2, 8, 8, 9, 1, stream),
        lambda: L.tc_metric_surfaces(p, p, p, p, c, 2, 8, 8, 17, 1, stream),                 # ncls > 16
        lambda: L.tc_metric_surfaces(p, p, p, p, c, 2048, 1024, 1024, 9, 1, stream),          # D*H*W >= 2^31
        lambda: L.tc_metric_surfaces(p, p, p, p, c, 2, 4096, 8, 9, 1, stream),                # a line longer than 2048
        lambda: L.tc_metric_surfaces(p, p, p, p, c, 0, 8, 8, 9, 1, stream),
        lambda: L.tc_metric_edt(None, 1, q, 2, 8, 8, 1, stream),
        lambda: L.tc_metric_edt(p, 0, q, 2, 8, 8, 1, stream),
        lambda: L.tc_metric_edt(p, 16, q, 2, 8, 8, 1, stream),
        lambda: L.tc_metric_edt(p, 1, q, 2048, 1024, 1024, 1, stream),
        lambda: L.tc_metric_hist(p, p, q, q, 1, h, nbins - 1, 9, 2, 8, 8, stream),            # histogram too small for the array
        lambda: L.tc_metric_hist(p, p, q, q, 9, h, nbins, 9, 2, 8, 8, stream),                # class outside the histogram
        lambda: L.tc_metric_hist(p, p, q, None, 1, h, nbins, 9, 2, 8, 8, stream),
        lambda: L.tc_metric_select(h, nbins, 17, c, stream),
        lambda: L.tc_metric_select(None, nbins, 9, c, stream),
        lambda: L.tc_metric_select(h, 0, 9, c, stream),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(TcError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    assert L.tc_metric_hist_bins(2, 8, 8) == nbins == 1 + 49 + 49 + 1 and L.tc_metric_hist_bins(2048, 1024, 1024) == 0
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0 and int(hist.abs().sum()) == 0 and int(i32.abs().sum()) == 0      # nothing ran

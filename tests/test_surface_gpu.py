"""The directed surface statistics on the MI355X (csrc/surface.hip; include/transception_surface.h): tc_surface_stats / tc_surface_stats_f64
on the C ABI against the brute force of tests/surface_ref.py -- exactly where every distance is a multiple of 0.5, within the rounding of
the square roots and of the summation elsewhere --, the edges of the entry (absent classes, the other classes' slots, garbage in `work`,
any base address, guard bytes, run-to-run identity), its refusals, `surface_metrics_device` against `surface_metrics_host`, and the public
path: `evaluate_volume_report`, `inference_report` and the trainer's `surface_metrics`."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import surface_ref as R
from metrics_util import DEV, dev, ellipsoid, label_volume

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transception_amd import _lib  # noqa: E402
from transception_amd._lib import lib  # noqa: E402

pytestmark = pytest.mark.gpu

SPACING = (2.0, 0.5, 1.5)
POISON = 0x5A5A5A5A5A5A5A5A
WORK_WORDS = _lib.TC_SURFACE_WORK_BYTES // 8
INTEGER_KEYS = ("dice", "jaccard", "precision", "recall", "defined")
EPS = 2.0 ** -52


def shape3(shape):
    return (1,) * (3 - len(shape)) + tuple(shape)


def spacing_of(ndim, spaced):
    return SPACING[3 - ndim:] if spaced else None


def maps(pred, gt, k, ncls, spacing):
    """(surf_pred, surf_gt, d2_pred, d2_gt) of class k on the device, from the kernels of csrc/metrics.hip: what the entry is given in use."""
    from transception_amd.evaluate import edt_squared, surfaces_counts
    sp, sg, _ = surfaces_counts(dev(pred.astype(np.uint8)), dev(gt.astype(np.uint8)), ncls)
    return sp, sg, edt_squared(sp, k, voxelspacing=spacing), edt_squared(sg, k, voxelspacing=spacing)


def stats(sp, sg, dp, dg, k, ncls, tol2, out=None, work=None):
    """One call of the entry that belongs to the distance maps' dtype; `work` full of 0xFF unless given.  Returns `out` ([ncls,2,4] int64)."""
    entry = lib().tc_surface_stats_f64 if dp.dtype == torch.float64 else lib().tc_surface_stats
    if out is None:
        out = torch.full((ncls, 2, 4), POISON, dtype=torch.int64, device=DEV)
    if work is None:
        work = torch.full((WORK_WORDS,), -1, dtype=torch.int64, device=DEV)
    entry(sp.data_ptr(), sg.data_ptr(), dp.data_ptr(), dg.data_ptr(), k, ncls, *shape3(sp.shape), float(tol2), work.data_ptr(), out.data_ptr(),
          torch.cuda.current_stream().cuda_stream)
    return out


def decode(out, k, spaced):
    """((n, sum, within, max), (n, sum, within, max)) of class k as Python numbers."""
    rec = out[k].cpu()
    as_double = rec.view(torch.float64)
    return tuple((int(rec[i, 0]), float(as_double[i, 1]), int(rec[i, 2]), float(as_double[i, 3]) if spaced else int(rec[i, 3])) for i in range(2))


# ---------------------------------------------------------------------------------------------------------------- 1. exact
def slabs(shape, a, b, c, d):
    pred, gt = np.zeros(shape, bool), np.zeros(shape, bool)
    pred[..., a:b] = True
    gt[..., c:d] = True
    return pred, gt


SLABS = [((5, 12, 20), (3, 9, 6, 15)), ((12, 20), (2, 7, 11, 18)), ((3, 420, 420), (2, 6, 4, 7))]      # (12, 20): the 2-D form of (1, 12, 20)


@pytest.mark.parametrize("spaced", [False, True], ids=["int32", "fp64"])
@pytest.mark.parametrize("shape,cut", SLABS, ids=lambda v: "x".join(map(str, v)))
def test_slabs_exactly(shape, cut, spaced):
    """Full-width slabs along the last axis: every surface distance is a multiple of 0.5 (asserted of the reference), so the sums are exact
    in any order and all eight slots equal the reference.  3 x 420 x 420 has more voxels than the 2048 x 256 threads of the capped grid."""
    pred, gt = slabs(shape, *cut)
    spacing = spacing_of(len(shape), spaced)
    d2 = R.all_d2(pred, gt, spacing)
    assert len(d2) and (np.sqrt(d2) * 2 % 1 == 0).all()
    tol2 = float(np.unique(R.directed_d2(R.surface(pred), R.surface(gt), spacing))[-2])      # the largest member but one: the test is <=, and exact
    want = R.records(pred, gt, spacing, tol2)
    assert int(np.prod(shape)) > 2048 * 256 or shape != (3, 420, 420)
    got = decode(stats(*maps(pred, gt, 1, 2, spacing), 1, 2, tol2), 1, spaced)
    print(shape, spaced, got)
    assert got == want and 0 < want[0][2] < want[0][0]


# ---------------------------------------------------------------------------------------------------------------- 2. general shapes
def rough_pair(shape, seed):
    g = np.random.default_rng(seed)
    c = [(n - 1) / 2 for n in shape]
    a = ellipsoid(shape, [v + g.uniform(-1, 1) for v in c], [max(1.2, n / 3.2) for n in shape], g, 0.35)
    b = ellipsoid(shape, [v + g.uniform(-1.5, 1.5) for v in c], [max(1.2, n / 3.6) for n in shape], g, 0.35)
    return a.astype(np.uint8), b.astype(np.uint8)


def organ_pair(shape=(9, 40, 48), seed=5):
    """Two label volumes of one seed with organs 1..4 of 6 classes: organ 2 is missing from the prediction, organ 3 from the label, class 5
    from both; the prediction is shifted by two and three voxels along the last two axes."""
    pred = label_volume(shape, np.random.default_rng(seed), 4, skip=(2,))
    gt = label_volume(shape, np.random.default_rng(seed), 4, skip=(3,))
    return np.roll(pred, (2, 3), axis=(-2, -1)), gt


def safe_tolerance(d2):
    """The first tau of a fixed list whose square no reference squared distance comes within 1e-9 relative of, and that splits them."""
    for tau in (1.7, 2.3, 2.9, 3.3, 1.3, 4.1):
        if (np.abs(d2 - tau * tau) > 1e-9 * tau * tau).all() and d2.min() <= tau * tau < d2.max():
            return tau
    raise AssertionError("no tolerance of the list keeps clear of the reference's squared distances")


GENERAL = [("rough-3d", rough_pair((9, 40, 48), 3), 2), ("rough-2d", rough_pair((37, 53), 4), 2), ("organs", organ_pair(), 6)]


@pytest.fixture(scope="module")
def general_reference():
    """Per (case, spaced, class): (tau, the reference's two records).  Computed once."""
    ref = {}
    for name, (pred, gt), ncls in GENERAL:
        for spaced in (False, True):
            spacing = spacing_of(pred.ndim, spaced)
            for k in range(1, ncls):
                if (pred == k).any() and (gt == k).any():
                    tau = safe_tolerance(R.all_d2(pred == k, gt == k, spacing))
                    ref[name, spaced, k] = tau, R.records(pred == k, gt == k, spacing, tau * tau)
    return ref


@pytest.mark.parametrize("spaced", [False, True], ids=["int32", "fp64"])
@pytest.mark.parametrize("name,pair,ncls", GENERAL, ids=[c[0] for c in GENERAL])
def test_general_shapes(name, pair, ncls, spaced, general_reference):
    """int32: n, within and max equal, |sum - fsum| <= (n + 1) 2^-52 fsum.  fp64: n equal, max within 1e-12 relative (the bound the fp64 maps
    are held to), sum within that plus the summation term, within equal at a tolerance that keeps clear of every reference distance."""
    pred, gt = pair
    spacing = spacing_of(pred.ndim, spaced)
    seen = 0
    for k in range(1, ncls):
        if (name, spaced, k) not in general_reference:
            continue
        tau, want = general_reference[name, spaced, k]
        got = decode(stats(*maps(pred, gt, k, ncls, spacing), k, ncls, tau * tau), k, spaced)
        for g, w in zip(got, want):
            print(name, spaced, k, g, w)
            assert g[0] == w[0] > 0 and g[2] == w[2]
            if spaced:
                assert abs(g[3] - w[3]) <= 1e-12 * w[3] and abs(g[1] - w[1]) <= 1e-12 * w[1] + R.sum_bound(w[0], w[1])
            else:
                assert g[3] == w[3] and abs(g[1] - w[1]) <= R.sum_bound(w[0], w[1])
        seen += 1
    assert seen == (2 if name == "organs" else 1)


def test_grid_stride_wrap_on_random_maps():
    """The entry reads whatever maps it is given: random bytes and random perfect squares over 3 x 1500 x 2048 voxels, more 16-byte pieces
    than the capped grid has threads, so every thread takes a second piece; the surface maps start 5 and 16 bytes into their allocations.
    The sums are sums of integers: exact."""
    g = np.random.default_rng(9)
    shape, n = (3, 1500, 2048), 3 * 1500 * 2048
    assert n // 16 > 2048 * 256
    surf = [np.where(g.random(n) < 0.02, g.integers(1, 4, n), 0).astype(np.uint8) for _ in range(2)]
    root = [g.integers(0, 1000, n).astype(np.int32) for _ in range(2)]
    d2 = [np.where(g.random(n) < 0.01, _lib.TC_METRIC_NO_SOURCE + 7, r * r).astype(np.int32) for r in root]
    raw = [torch.zeros(n + 32, dtype=torch.uint8, device=DEV) for _ in range(2)]
    sp, sg = raw[0][5:5 + n].view(shape), raw[1][16:16 + n].view(shape)
    sp.copy_(dev(surf[0]).view(shape)); sg.copy_(dev(surf[1]).view(shape))
    assert sp.data_ptr() % 16 == 5 and sg.data_ptr() % 16 == 0
    tol2 = 300.0 ** 2
    got = decode(stats(sp, sg, dev(d2[0]).view(shape), dev(d2[1]).view(shape), 2, 4, tol2), 2, False)
    for i, (s, d) in enumerate(((surf[0], d2[1]), (surf[1], d2[0]))):
        v = d[(s == 2) & (d < _lib.TC_METRIC_NO_SOURCE)].astype(np.int64)
        assert got[i] == (len(v), float(np.sqrt(v).astype(np.int64).sum()), int((v <= tol2).sum()), int(v.max())) and len(v) > 10000


# ---------------------------------------------------------------------------------------------------------------- 3. edges
def test_absent_classes_other_slots_tolerances_and_repeatability():
    pred, gt = organ_pair()
    ncls = 6
    for spaced in (False, True):
        spacing = spacing_of(3, spaced)
        out = torch.full((ncls, 2, 4), POISON, dtype=torch.int64, device=DEV)
        for k in (2, 3, 5):                                                   # absent from the prediction, from the label, from both
            m = maps(pred, gt, k, ncls, spacing)
            before = out.clone()
            stats(*m, k, ncls, 4.0, out=out)
            assert decode(out, k, spaced) == ((0, 0.0, 0, 0),) * 2 and not out[k].any()
            others = [c for c in range(ncls) if c != k]
            assert torch.equal(out[others], before[others])                   # the other classes' slots are not touched
        m = maps(pred, gt, 1, ncls, spacing)
        keep = [t.clone() for t in m]
        first = stats(*m, 1, ncls, 4.0, out=out.clone())
        garbage = torch.randint(-2 ** 62, 2 ** 62, (WORK_WORDS,), dtype=torch.int64, device=DEV)
        again = stats(*m, 1, ncls, 4.0, out=out.clone(), work=garbage)
        assert torch.equal(first, again) and all(torch.equal(a, b) for a, b in zip(m, keep))      # to the bit, and the inputs are unchanged
        (n0, s0, w0, m0), (n1, s1, w1, m1) = decode(first, 1, spaced)
        assert n0 > w0 > 0 and n1 > w1 > 0
        d2_at = [m[3][m[0] == 1], m[2][m[1] == 1]]                            # the members of either direction, as the maps hold them
        zero = decode(stats(*m, 1, ncls, 0.0), 1, spaced)
        assert [r[2] for r in zero] == [int((d == 0).sum()) for d in d2_at]
        above = decode(stats(*m, 1, ncls, float(max(m0, m1)) * 1.5 + 1.0), 1, spaced)
        assert [r[2] for r in above] == [n0, n1] == [d.numel() for d in d2_at]
        assert all(a[:2] == b[:2] == c[:2] and a[3] == b[3] == c[3] for a, b, c in zip(zero, above, ((n0, s0, w0, m0), (n1, s1, w1, m1))))
        assert [m0, m1] == [d.max().item() for d in d2_at]


@pytest.mark.parametrize("spaced", [False, True], ids=["int32", "fp64"])
def test_any_base_address_and_guards(spaced):
    """uint8 maps 1 and 3 bytes into their allocations, distance maps one element in, `out` and `work` between guard words: the aligned
    call's result, and not a guard byte touched."""
    pred, gt = rough_pair((9, 40, 47), 6)                                     # 16920 voxels: a head, 16-byte pieces and a tail on both maps
    spacing, n, shape = spacing_of(3, spaced), pred.size, pred.shape
    m = maps(pred, gt, 1, 2, spacing)
    want = stats(*m, 1, 2, 6.25)
    moved = []
    for t, off in zip(m, (1, 3, 1, 1)):
        raw = torch.zeros(n + 64, dtype=t.dtype, device=DEV)
        view = raw[off:off + n].view(shape)
        view.copy_(t)
        assert view.data_ptr() == raw.data_ptr() + off * t.element_size()
        moved.append(view)
    assert moved[0].data_ptr() % 16 != moved[1].data_ptr() % 16
    G = 64
    out = torch.full((G + 2 * 8 + G,), POISON, dtype=torch.int64, device=DEV)
    work = torch.full((G + WORK_WORDS + G,), -1, dtype=torch.int64, device=DEV)
    got = stats(*moved, 1, 2, 6.25, out=out[G:G + 16].view(2, 2, 4), work=work[G:G + WORK_WORDS])
    # which thread takes which voxel follows the maps' alignment, so the sums are the same roots added in another order; the rest is exact
    for g, w in zip(decode(got, 1, spaced), decode(want, 1, spaced)):
        assert g[0] == w[0] > 0 and g[2:] == w[2:] and abs(g[1] - w[1]) <= R.sum_bound(w[0], w[1])
    assert torch.equal(stats(*moved, 1, 2, 6.25)[1], got[1])                  # and at one alignment a run repeats to the bit
    assert (out[:G] == POISON).all() and (out[G + 16:] == POISON).all() and (out[G:G + 8] == POISON).all()      # class 0's slots as well
    assert (work[:G] == -1).all() and (work[G + WORK_WORDS:] == -1).all()
    assert all(torch.equal(a, b) for a, b in zip(moved, m))


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_output_as_it_was():
    pred, gt = rough_pair((5, 12, 20), 2)
    for spaced in (False, True):
        m = maps(pred, gt, 1, 2, spacing_of(3, spaced))
        entry = lib().tc_surface_stats_f64 if spaced else lib().tc_surface_stats
        out = torch.full((16, 2, 4), POISON, dtype=torch.int64, device=DEV)
        work = torch.full((WORK_WORDS,), -1, dtype=torch.int64, device=DEV)
        good = [t.data_ptr() for t in m] + [1, 2, 5, 12, 20, 4.0, work.data_ptr(), out.data_ptr()]
        bad = [(i, None) for i in (0, 1, 2, 3, 10, 11)]
        bad += [(4, 0), (4, 2), (4, -1), (5, 17), (5, 0), (6, 2049), (7, 0), (8, 2049), (9, -1.0), (9, float("nan")), (9, float("inf"))]
        for pos, value in bad:
            args = list(good)
            args[pos] = value
            with pytest.raises(_lib.TcError, match="status -1"):
                entry(*args, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (out == POISON).all() and (work == -1).all()
        entry(*good, torch.cuda.current_stream().cuda_stream)                 # and the call they were made from is a good one
        assert not (out[1] == POISON).any() and (out[0] == POISON).all() and (out[2:] == POISON).all()


# ---------------------------------------------------------------------------------------------------------------- 5. Python
def assert_reports_agree(got, want, spaced, nvox):
    """Two per-class reports of one prediction, one from the device and one from scipy.  What is formed from integers is equal -- with unit
    spacing that includes nsd and hd.  A sum of at most `nvox` square roots is within (nvox + 1) 2^-52 relative of its exact value on either
    side, a division adds an ulp; with a spacing the squared distances themselves agree within 1e-12 relative.  hd95 is held to the bound of
    the existing device-metric tests (1e-9)."""
    assert len(got) == len(want)
    rel = 2 * (nvox + 3) * EPS + (1e-12 if spaced else 0.0)
    for k, (g, w) in enumerate(zip(got, want), 1):
        assert list(g) == list(w)
        for key in INTEGER_KEYS:
            assert g[key] == w[key] and type(g[key]) is type(w[key]), (k, key)
        for key in ("asd_pred", "asd_gt", "assd"):
            assert abs(g[key] - w[key]) <= rel * w[key], (k, key, g[key], w[key])
        if spaced:
            assert abs(g["hd"] - w["hd"]) <= 1e-12 * w["hd"], k
        else:
            assert g["hd"] == w["hd"], k
        assert g["nsd"] == w["nsd"], k
        assert abs(g["hd95"] - w["hd95"]) <= 1e-9 * max(1.0, w["hd95"]), k


@pytest.mark.parametrize("spaced", [False, True], ids=["unit", "spaced"])
@pytest.mark.parametrize("ndim", [3, 2])
def test_surface_metrics_device_against_host(ndim, spaced):
    from transception_amd.evaluate import SurfaceMetrics, calculate_metric_percase, metrics_device, surface_metrics_device, surface_metrics_host
    pred, gt = organ_pair() if ndim == 3 else organ_pair((37, 53), 8)
    ncls, spacing = 6, spacing_of(ndim, spaced)
    present = [k for k in range(1, ncls) if (pred == k).any() and (gt == k).any()]
    assert not (pred == 2).any() and (gt == 2).any() and (pred == 3).any() and not (gt == 3).any() and present == [1, 4]
    # one tolerance per class; with a spacing each keeps clear of the reference's squared distances, so that the counts are equal
    taus = [safe_tolerance(R.all_d2(pred == k, gt == k, spacing)) if spaced and k in present else 1.0 + 0.5 * k for k in range(1, ncls)]
    surface = SurfaceMetrics(tuple(taus))
    got = surface_metrics_device(dev(pred), dev(gt), ncls, spacing, surface)
    want = surface_metrics_host(pred, gt, ncls, spacing, surface)
    print(got)
    assert_reports_agree(got, want, spaced, pred.size)
    assert [d["defined"] for d in got] == [True, False, False, True, False]
    assert got[2]["dice"] == got[2]["nsd"] == 1.0 and got[2]["hd"] == 0.0 and got[1]["recall"] == 0.0        # only the prediction / only the label
    # dice and hd95 are metrics_device's, which the refactored loop has not changed
    plain = metrics_device(dev(pred), dev(gt), ncls, spacing)
    assert [(d["dice"], d["hd95"]) for d in got] == plain
    for (d, h), k in zip(plain, range(1, ncls)):
        wd, wh = calculate_metric_percase(pred == k, gt == k, spacing)
        assert abs(d - wd) <= 1e-12 and abs(h - wh) <= 1e-9 * max(1.0, wh), k
    # a scalar tolerance is that tolerance for every class
    if not spaced:
        assert surface_metrics_device(dev(pred), dev(gt), ncls, None, SurfaceMetrics(2.0)) == \
            surface_metrics_device(dev(pred), dev(gt), ncls, None, SurfaceMetrics((2.0,) * 5))
        with pytest.raises(ValueError, match="nsd_tolerance"):
            surface_metrics_device(dev(pred), dev(gt), ncls, None, SurfaceMetrics((2.0,) * 4))


def test_the_launches_of_metrics_device_are_kept(monkeypatch):
    """`surface_metrics_device` makes `metrics_device`'s calls of the library plus one tc_surface_stats per class, and `metrics_device` none."""
    from transception_amd import evaluate as E
    pred, gt = organ_pair()
    L, seen = lib(), []
    for name in ("tc_metric_surfaces", "tc_metric_edt", "tc_metric_hist", "tc_metric_select", "tc_surface_stats"):
        monkeypatch.setattr(L, name, (lambda real, name: lambda *a: (seen.append(name), real(*a))[1])(getattr(L, name), name))
    E.metrics_device(dev(pred), dev(gt), 6)
    plain = list(seen)
    assert plain.count("tc_metric_edt") == 10 and plain.count("tc_metric_hist") == 5 and "tc_surface_stats" not in plain
    del seen[:]
    E.surface_metrics_device(dev(pred), dev(gt), 6)
    assert [s for s in seen if s != "tc_surface_stats"] == plain and seen.count("tc_surface_stats") == 5


# ---------------------------------------------------------------------------------------------------------------- 6. the public path
def real_network(dtype):
    from transception_amd import MSTransception
    from transception_amd.seeded_init import seeded_state_dict
    net = MSTransception(num_classes=9)
    net.load_state_dict(seeded_state_dict(), strict=True)
    net.to(DEV)
    net.set_compute_dtype(dtype)
    return net


def blocky_volume(seed, d=3, n=96):
    g = np.random.default_rng(seed)
    lab = np.kron(g.integers(0, 9, (d, n // 8, n // 8)), np.ones((8, 8), np.int64)).astype(np.uint8)
    return (lab / 8).astype(np.float32), np.roll(lab, 1, axis=2)


def test_reports_of_the_public_path():
    """A seeded network at patch 64 x 64 on 96 x 96 volumes: `evaluate_volume_report` on the device and on the host agree, its dice and hd95 are
    `evaluate_volume`'s, and `inference_report`'s overall pair is `inference`'s."""
    from transception_amd.evaluate import SURFACE_KEYS, SurfaceMetrics, evaluate_volume, evaluate_volume_report, inference, inference_report
    net = real_network(torch.float32).train()
    vols = [blocky_volume(21) + ("a",), tuple(v[:2] for v in blocky_volume(22)) + ("b",)]
    surface = SurfaceMetrics((1.0, 1.5, 2.0, 2.5, 3.0, 1.0, 2.0, 3.0))
    image, gt, _ = vols[0]
    on = evaluate_volume_report(net, image, gt, 9, (64, 64), batch=2, device_metrics=True, surface=surface)
    off = evaluate_volume_report(net, image, gt, 9, (64, 64), batch=2, surface=surface)
    assert net.training and len(on) == 8
    assert_reports_agree(on, off, False, gt.size)
    for dm, rep in ((True, on), (False, off)):
        assert [(d["dice"], d["hd95"]) for d in rep] == evaluate_volume(net, image, gt, 9, (64, 64), batch=2, with_hd95=True, device_metrics=dm)
    for dm in (True, False):
        lines = []
        rep = inference_report(net, vols, 9, 64, batch=2, log=lines.append, device_metrics=dm, surface=surface)
        assert (rep["overall"]["dice"], rep["overall"]["hd95"]) == inference(net, vols, 9, 64, batch=2, device_metrics=dm)
        assert [c["name"] for c in rep["cases"]] == ["a", "b"] and all(len(c["classes"]) == 8 for c in rep["cases"])
        assert tuple(rep["mean"]) == tuple(rep["overall"]) == SURFACE_KEYS and all(len(v) == 8 for v in rep["mean"].values())
        assert rep["n_defined"] == [sum(c["classes"][k]["defined"] for c in rep["cases"]) for k in range(8)]
        for key in SURFACE_KEYS:
            per_class = [(rep["cases"][0]["classes"][k][key] + rep["cases"][1]["classes"][k][key]) / 2 for k in range(8)]
            assert rep["mean"][key] == per_class and abs(rep["overall"][key] - sum(per_class) / 8) <= 1e-12 * max(1.0, abs(sum(per_class) / 8))
        assert any("mean_assd" in line for line in lines) and any("mean_dice" in line for line in lines)
        if dm:
            assert rep["cases"][0]["classes"] == on


def test_trainer_fills_hist_surface(tmp_path):
    from transception_amd import data as D
    from transception_amd import trainer as T
    from transception_amd.evaluate import SURFACE_KEYS, SurfaceMetrics
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=1, slices_per_case=4, size=64, seed=2)
    g = np.random.default_rng(0)
    vol = (g.random((3, 96, 96)).astype(np.float32), (g.random((3, 96, 96)) * 3).astype(np.uint8), "case0")
    hists = {}
    for name, option in (("with", dict(surface_metrics=SurfaceMetrics((1.0,) * 8))), ("without", dict())):
        net = real_network(torch.bfloat16)
        net.train()
        cfg = T.TrainConfig(root_path=base, list_dir=lists, max_epochs=1, batch_size=2, img_size=64, seed=5, model_name="tiny",
                            device_metrics=True, **option)
        hists[name] = T.trainer_synapse(cfg, net, str(tmp_path / ("snap_" + name)), volumes=lambda: [vol], log=lambda s: None)
    hist = hists["with"]
    assert "surface" not in hists["without"] and set(hist) == set(hists["without"]) | {"surface"}
    assert len(hist["surface"]) == len(hist["dice"]) == 1 and tuple(hist["surface"][0]) == SURFACE_KEYS
    s = hist["surface"][0]
    assert s["dice"] == hist["dice"][0] and s["hd95"] == hist["hd95"][0] and all(math.isfinite(v) for v in s.values())
    assert 0.0 <= s["nsd"] <= 1.0 and s["hd"] >= s["hd95"] >= 0.0

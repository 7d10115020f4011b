"""The surface metrics without a GPU: the binding derived from include/transception_surface.h, `surface_metrics_host` against the brute
force of tests/surface_ref.py, the three-way per-case rule, the validation of `SurfaceMetrics` / `surface=` / `TrainConfig.surface_metrics`,
and the signatures that must stay what they were."""
import ctypes
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest

import surface_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "transception_surface.h")
ENTRIES = {"tc_surface_abi_version": 0, "tc_surface_stats": 13, "tc_surface_stats_f64": 13}
SPACING = (2.0, 0.5, 1.5)
KEYS = ("dice", "jaccard", "precision", "recall", "hd95", "hd", "asd_pred", "asd_gt", "assd", "nsd")


@pytest.fixture(scope="module")
def built():
    from transception_amd.build import build
    return build(verbose=False)


# ---------------------------------------------------------------------------------------------------------------- the binding
def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = {}
    for m in re.finditer(r"\b(?:int|long long)\s+(tc_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        fns[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return fns


def test_binding_is_the_header(built):
    from transception_amd import _header, _lib
    from transception_amd.build import SOURCES
    fns = header_functions()
    assert fns == ENTRIES
    dll = ctypes.CDLL(built)
    for name in fns:
        assert hasattr(dll, name), f"{name} declared in the header but not exported by {built}"
    assert {n: len(f.argtypes) for n, f in _lib.SURFACE.functions.items()} == ENTRIES
    assert {n for n, f in _lib.SURFACE.functions.items() if f.query} == {"tc_surface_abi_version"}
    for name in ("tc_surface_stats", "tc_surface_stats_f64"):
        at = _lib.SURFACE.functions[name].argtypes
        assert at[:4] == [ctypes.c_void_p] * 4 and at[4:9] == [ctypes.c_int] * 5 and at[9] is ctypes.c_double and at[10:] == [ctypes.c_void_p] * 3
    assert not _lib.SURFACE.structs
    assert _lib.SURFACE.constants == {"TC_SURFACE_ABI_VERSION": 1, "TC_SURFACE_WORK_BYTES": 131072}
    assert _lib.TC_SURFACE_WORK_BYTES == 2048 * 8 * 8 and _lib.SURFACE_ABI_VERSION == 1 == dll.tc_surface_abi_version()
    assert _header.load(HEADER).functions.keys() == fns.keys()               # self-contained: the parser refuses an #include
    # the names are this header's alone, and the main header is what it was
    others = [_lib.SIGNATURES] + [_lib.SIDE[s.attr].functions for s in _header.SIDE_HEADERS if s.attr != "SURFACE"]
    assert len(others) == len(_header.SIDE_HEADERS)
    for other in others:
        assert not set(ENTRIES) & set(other) and not any(n.startswith("tc_surface_") for n in other)
    assert _lib.ABI_VERSION == 15 and len(_lib.SIGNATURES) == 137
    assert "surface.hip" in SOURCES
    attrs = [s.attr for s in _header.SIDE_HEADERS]
    assert attrs[-1] == "LOSS" and attrs.count("SURFACE") == 1
    side = _header.SIDE_HEADERS[attrs.index("SURFACE")]
    assert (side.file, side.version, side.entry) == ("transception_surface.h", "TC_SURFACE_ABI_VERSION", "tc_surface_abi_version")
    L = _lib.lib()
    assert L.tc_surface_abi_version is L.cdll.tc_surface_abi_version         # the query is exposed raw, the status entries checked
    for name in ("tc_surface_stats", "tc_surface_stats_f64"):
        assert getattr(L, name).__name__ == name and getattr(L, name) is not getattr(L.cdll, name)


def test_entries_refuse_bad_arguments_before_any_launch(built):
    """Argument checks come before any launch, so they run without a GPU: the addresses below are never dereferenced."""
    from transception_amd import _lib
    L = _lib.lib()
    A, B, C, D, WK, OUT = (0x10000 * i for i in range(1, 7))
    good = [A, B, C, D, 1, 9, 4, 8, 8, 1.0, WK, OUT]
    bad = [(i, None) for i in (0, 1, 2, 3, 10, 11)]                          # a null pointer
    bad += [(4, 0), (4, 9), (4, -1), (5, 17), (5, 0), (6, 0), (6, 2049), (7, 2049), (8, -3), (8, 2049),
            (9, -1.0), (9, -1e-300), (9, float("nan")), (9, float("inf")), (9, -float("inf"))]
    for name in ("tc_surface_stats", "tc_surface_stats_f64"):
        for pos, value in bad:
            args = list(good)
            args[pos] = value
            with pytest.raises(_lib.TcError, match=name + " failed with status -1"):
                getattr(L, name)(*args, None)
        with pytest.raises(_lib.TcError, match="status -1"):                 # 2^31 voxels, each extent legal
            getattr(L, name)(A, B, C, D, 1, 9, 2048, 1024, 1024, 1.0, WK, OUT, None)


# ---------------------------------------------------------------------------------------------------------------- against the brute force
def mask_pairs():
    g = np.random.default_rng(11)
    pairs = []
    a = np.zeros((6, 11, 12), bool); b = np.zeros_like(a)
    a[1:5, 2:9, 2:10] = True; b[2:4, 4:7, 4:8] = True
    pairs.append(("nested", a, b))
    a = np.zeros((5, 9, 10), bool); b = np.zeros_like(a)
    a[:2, :3, :4] = True; b[3:, 6:, 7:] = True
    pairs.append(("disjoint", a, b))
    a = g.random((5, 8, 9)) < 0.4
    pairs.append(("identical", a, a.copy()))
    a = np.zeros((4, 7, 8), bool); a[2, 3, 5] = True
    b = np.zeros_like(a); b[0:3, 1:5, 0:4] = True
    pairs.append(("single-voxel", a, b))
    a = np.zeros((5, 8, 9), bool); b = np.zeros_like(a)
    a[0:3, 0:5, 4:9] = True; b[2:5, 3:8, 0:6] = True
    pairs.append(("border", a, b))
    a = np.zeros((13, 17), bool); b = np.zeros_like(a)
    a[2:9, 3:12] = True; b[5:13, 0:8] = True; b[7, 3] = False
    pairs.append(("2-d", a, b))
    return pairs


PAIRS = mask_pairs()


@pytest.mark.parametrize("spaced", [False, True], ids=["unit", "spaced"])
@pytest.mark.parametrize("name,a,b", PAIRS, ids=[p[0] for p in PAIRS])
def test_host_against_the_brute_force(name, a, b, spaced):
    from transception_amd.evaluate import SurfaceMetrics, calculate_metric_percase, surface_metrics_host, surface_stats_host
    spacing = SPACING[3 - a.ndim:] if spaced else None
    tau = 1.5
    want = R.records(a, b, spacing, tau * tau)
    got = surface_stats_host(a, b, spacing, tau * tau)
    for w, g in zip(want, got):
        assert g[0] == w[0] and g[2] == w[2]                                 # the counts
        if spaced:
            assert abs(g[3] - w[3]) <= 1e-12 * w[3] and abs(g[1] - w[1]) <= 1e-12 * w[1] + R.sum_bound(w[0], w[1])
        else:
            assert type(g[3]) is int and g[3] == w[3] and g[1] == w[1]       # exact integers, the same fsum of the same roots
    m = surface_metrics_host(a.astype(np.uint8), b.astype(np.uint8), 2, spacing, SurfaceMetrics(tau))
    assert len(m) == 1 and tuple(m[0]) == KEYS + ("defined",) and m[0]["defined"] is True
    ref = R.metrics(want)
    # medpy's assd restated: the mean of the two directed means
    assert ref["assd"] == (want[0][1] / want[0][0] + want[1][1] / want[1][0]) / 2
    for key, v in ref.items():
        assert m[0][key] == pytest.approx(v, rel=1e-12 if spaced else 0, abs=0), key
    assert (m[0]["dice"], m[0]["hd95"]) == calculate_metric_percase(a, b, spacing)
    inter, p, g = int((a & b).sum()), int(a.sum()), int(b.sum())
    assert (m[0]["jaccard"], m[0]["precision"], m[0]["recall"]) == (inter / (p + g - inter), inter / p, inter / g)
    assert m[0]["hd"] >= m[0]["hd95"] and m[0]["hd"] >= max(m[0]["asd_pred"], m[0]["asd_gt"]) and 0.0 <= m[0]["nsd"] <= 1.0
    if name == "identical":
        assert (m[0]["hd"], m[0]["assd"], m[0]["nsd"], m[0]["dice"]) == (0.0, 0.0, 1.0, 1.0)


def test_assd_is_not_the_pooled_mean():
    from transception_amd.evaluate import surface_metrics_host
    _, a, b = PAIRS[3]                                                        # one voxel against a block: very different surface sizes
    (n0, s0, _, _), (n1, s1, _, _) = R.records(a, b)
    m = surface_metrics_host(a.astype(np.uint8), b.astype(np.uint8), 2)[0]
    assert m["assd"] == (s0 / n0 + s1 / n1) / 2 and abs(m["assd"] - (s0 + s1) / (n0 + n1)) > 0.1


def test_tolerance_is_tested_on_squared_distances():
    """Two parallel plates three voxels apart: every distance is exactly 3, so tau = 3 counts everything and the next double below nothing."""
    from transception_amd.evaluate import SurfaceMetrics, surface_metrics_host
    a = np.zeros((1, 6, 8), np.uint8); b = np.zeros_like(a)
    a[0, :, 1] = 1; b[0, :, 4] = 1
    assert surface_metrics_host(a, b, 2, None, SurfaceMetrics(3.0))[0]["nsd"] == 1.0
    assert surface_metrics_host(a, b, 2, None, SurfaceMetrics(math.nextafter(3.0, 0.0)))[0]["nsd"] == 0.0
    assert surface_metrics_host(a, a, 2, None, SurfaceMetrics(0.0))[0]["nsd"] == 1.0
    per_class = surface_metrics_host(np.where(a, 2, 0).astype(np.uint8), np.where(b, 2, 0).astype(np.uint8), 3, None, SurfaceMetrics((9.0, 2.5)))
    assert per_class[1]["nsd"] == 0.0 and per_class[1]["hd"] == 3.0 and not per_class[0]["defined"]


# ---------------------------------------------------------------------------------------------------------------- degenerate cases
def test_the_three_way_rule():
    from transception_amd.evaluate import surface_metrics_host
    pred = np.zeros((3, 6, 6), np.uint8); gt = np.zeros_like(pred)
    pred[1, 1:4, 1:4] = 1; gt[1, 2:5, 2:5] = 1                                # class 1: both
    pred[0, 0, 0] = 2                                                         # class 2: only the prediction
    gt[2, 5, 5] = 3                                                           # class 3: only the label; class 4: neither
    both, only_pred, only_gt, neither = surface_metrics_host(pred, gt, 5)
    assert both["defined"] is True and 0 < both["dice"] < 1 and both["hd"] > 0
    assert only_pred == dict({k: 1.0 for k in ("dice", "jaccard", "precision", "recall", "nsd")},
                             **{k: 0.0 for k in ("hd95", "hd", "asd_pred", "asd_gt", "assd")}, defined=False)
    zero = dict({k: 0.0 for k in KEYS}, defined=False)
    assert only_gt == zero and neither == zero
    assert [tuple(d) for d in (both, only_pred, only_gt, neither)] == [KEYS + ("defined",)] * 4


def test_surface_metrics_validation():
    from transception_amd.evaluate import VALID_OPTION, SurfaceMetrics
    assert SurfaceMetrics().nsd_tolerance == 1.0 and SurfaceMetrics(2).nsd_tolerance == 2.0
    assert SurfaceMetrics([1, 2.5]).nsd_tolerance == (1.0, 2.5) and SurfaceMetrics(np.array([0.0, 3.0])).tolerances(3) == (0.0, 3.0)
    assert SurfaceMetrics(1.5).tolerances(9) == (1.5,) * 8 and SurfaceMetrics((1.0, 2.0)) == SurfaceMetrics([1, 2])
    with pytest.raises(dataclasses.FrozenInstanceError):
        SurfaceMetrics().nsd_tolerance = 2.0
    for bad in (-1.0, float("nan"), float("inf"), True, None, "1.0", (), (1.0, -0.5), (1.0, float("nan")), (1.0, True), (1.0, "2")):
        with pytest.raises(ValueError, match="nsd_tolerance"):
            SurfaceMetrics(bad)
    with pytest.raises(ValueError, match="nsd_tolerance"):
        SurfaceMetrics((1.0,) * 7).tolerances(9)
    assert VALID_OPTION["surface"](None) and VALID_OPTION["surface"](SurfaceMetrics()) and not VALID_OPTION["surface"](1.0)


def test_bad_options_are_refused_before_anything_runs():
    """The model here is None: a ValueError must come before it or the device is touched."""
    from transception_amd.evaluate import SurfaceMetrics, evaluate_volume_report, inference_report, surface_metrics_device, surface_metrics_host
    img, lab = np.zeros((1, 96, 96), np.float32), np.zeros((1, 96, 96), np.uint8)
    for bad in (SurfaceMetrics((1.0,) * 7), SurfaceMetrics((1.0,) * 9)):       # the wrong length for nine classes
        with pytest.raises(ValueError, match="nsd_tolerance"):
            evaluate_volume_report(None, img, lab, patch_size=(64, 64), surface=bad)
        with pytest.raises(ValueError, match="nsd_tolerance"):
            inference_report(None, [(img, lab, "case")], surface=bad)
        with pytest.raises(ValueError, match="nsd_tolerance"):
            surface_metrics_host(lab, lab, 9, None, bad)
        with pytest.raises(ValueError, match="nsd_tolerance"):
            surface_metrics_device(None, None, 9, None, bad)
    for bad in (None, 1.0, (1.0,) * 8):
        with pytest.raises(ValueError, match="surface"):
            evaluate_volume_report(None, img, lab, patch_size=(64, 64), surface=bad)
        with pytest.raises(ValueError, match="surface"):
            inference_report(None, [(img, lab, "case")], surface=bad)
    with pytest.raises(ValueError, match="resample"):
        evaluate_volume_report(None, img, lab, patch_size=(64, 64), resample="bilinear")
    with pytest.raises(ValueError, match="inference_report"):
        inference_report(None, [])


# ---------------------------------------------------------------------------------------------------------------- signatures
def test_train_config_surface_metrics():
    from transception_amd.evaluate import SurfaceMetrics
    from transception_amd.trainer import KEYWORD_OPTIONS, TrainConfig
    assert TrainConfig("root", "lists").surface_metrics is None and TrainConfig.surface_metrics is None
    sm = SurfaceMetrics((1.0,) * 8)
    cfg = TrainConfig("root", "lists", surface_metrics=sm)
    assert cfg.surface_metrics is sm and "surface_metrics=SurfaceMetrics(" in repr(cfg) and repr(cfg).endswith("resample='labels')")
    assert TrainConfig("root", "lists", num_classes=4, surface_metrics=SurfaceMetrics(2.0)).surface_metrics.tolerances(4) == (2.0,) * 3
    for bad in (1.0, (1.0,) * 8, True, "on", SurfaceMetrics((1.0,) * 7)):
        with pytest.raises(ValueError, match="surface_metrics|nsd_tolerance"):
            TrainConfig("root", "lists", surface_metrics=bad)
    with pytest.raises(ValueError, match="nsd_tolerance"):
        TrainConfig("root", "lists", num_classes=4, surface_metrics=sm)
    params = inspect.signature(TrainConfig).parameters
    assert params["surface_metrics"].kind is inspect.Parameter.KEYWORD_ONLY and params["surface_metrics"].default is None
    assert list(params)[-1] == "resample" and KEYWORD_OPTIONS[0][0] == "surface_metrics" and KEYWORD_OPTIONS[-1][0] == "resample"
    names = [f.name for f in dataclasses.fields(TrainConfig)]
    assert names[-4:] == ["no_decay", "ema_decay", "ema_warmup", "ema_eval"] and "surface_metrics" not in names
    positional = [p.default for p in params.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD][2:]
    assert TrainConfig("root", "lists", *positional).surface_metrics is None
    with pytest.raises(TypeError):
        TrainConfig("root", "lists", *positional, sm)                         # not reachable by position


def test_evaluate_signatures():
    from transception_amd import evaluate as E
    kw = inspect.Parameter.KEYWORD_ONLY
    ev, inf = inspect.signature(E.evaluate_volume).parameters, inspect.signature(E.inference).parameters
    assert list(ev) == ["model", "image", "label", "classes", "patch_size", "batch", "with_hd95", "host_zoom", "device_metrics", "voxelspacing",
                        "postprocess", "tta", "resample"]
    assert list(inf) == ["model", "volumes", "classes", "img_size", "batch", "log", "device_metrics", "voxelspacing", "postprocess", "tta", "resample"]
    for params in (ev, inf):
        assert [n for n, p in params.items() if p.kind is kw] == ["resample"]
    rep, irep = inspect.signature(E.evaluate_volume_report).parameters, inspect.signature(E.inference_report).parameters
    assert list(rep) == [n for n in ev if n != "with_hd95"] + ["surface"] and list(irep) == list(inf) + ["surface"]
    for params in (rep, irep):
        assert [n for n, p in params.items() if p.kind is kw] == ["resample", "surface"] and params["surface"].default == E.SurfaceMetrics()
    for fn in (E.surface_metrics_device, E.surface_metrics_host):
        assert list(inspect.signature(fn).parameters) == ["pred", "label", "classes", "voxelspacing", "surface"]
    for fn, names in ((E.metrics_order_stats, ["pred", "label", "classes", "voxelspacing"]), (E.metrics_device, ["pred", "label", "classes", "voxelspacing"]),
                      (E.hd95_device, ["result", "reference", "voxelspacing"])):
        assert list(inspect.signature(fn).parameters) == names
    assert E.SURFACE_KEYS == KEYS

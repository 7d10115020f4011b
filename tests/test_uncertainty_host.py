"""Uncertainty maps and calibration without a GPU: the binding derived from include/transception_uncertainty.h, every refusal of the two
entries before any launch, the validation of `Calibration` / `TrainConfig.calibration`, `calibration_from_stats` on hand-made slots,
`calibration_host` against a brute-force loop, and the number facts the GPU equalities rest on."""
import ctypes
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import uncertainty_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "transception_uncertainty.h")
ENTRIES = {"tc_uncert_abi_version": 0, "tc_calib_work_bytes": 2, "tc_calib_out_slots": 2, "tc_uncert_maps": 14, "tc_calib_stats": 15}
QUERIES = {"tc_uncert_abi_version", "tc_calib_work_bytes", "tc_calib_out_slots"}


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
    V, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert header_functions() == ENTRIES
    dll = ctypes.CDLL(built)
    for name in ENTRIES:
        assert hasattr(dll, name), f"{name} declared in the header but not exported by {built}"
    fns = _lib.UNCERT.functions
    assert {n: len(f.argtypes) for n, f in fns.items()} == ENTRIES and {n for n, f in fns.items() if f.query} == QUERIES
    assert fns["tc_uncert_maps"].argtypes == [V, I, I, F, V, V, V, V, V, I, I, I, I, V]
    assert fns["tc_calib_stats"].argtypes == [V, I, I, F, V, I, I, I, I, I, I, I, V, V, V]
    assert fns["tc_calib_work_bytes"].restype is ctypes.c_longlong and fns["tc_calib_out_slots"].restype is I
    assert not _lib.UNCERT.structs
    assert _lib.UNCERT.constants == {"TC_UNCERT_ABI_VERSION": 1, "TC_UNCERT_LOGITS": 0, "TC_UNCERT_PROB_SUMS": 1, "TC_CALIB_FOREGROUND": 1,
                                     "TC_CALIB_MAX_BINS": 32}
    assert _lib.UNCERT_ABI_VERSION == 1 == dll.tc_uncert_abi_version()
    assert _header.load(HEADER).functions.keys() == ENTRIES.keys()           # self-contained: the parser refuses an #include
    # the names are this header's alone, the main header is what it was, and LOSS is still the last side header
    others = [_lib.SIGNATURES] + [_lib.SIDE[s.attr].functions for s in _header.SIDE_HEADERS if s.attr != "UNCERT"]
    assert len(others) == len(_header.SIDE_HEADERS)
    for other in others:
        assert not set(ENTRIES) & set(other) and not any(n.startswith(("tc_uncert_", "tc_calib_")) for n in other)
    assert _lib.ABI_VERSION == 15 and len(_lib.SIGNATURES) == 137
    assert "uncertainty.hip" in SOURCES
    attrs = [s.attr for s in _header.SIDE_HEADERS]
    assert attrs[-1] == "LOSS" and attrs.count("UNCERT") == 1
    side = _header.SIDE_HEADERS[attrs.index("UNCERT")]
    assert (side.file, side.version, side.entry) == ("transception_uncertainty.h", "TC_UNCERT_ABI_VERSION", "tc_uncert_abi_version")
    L = _lib.lib()
    for name in QUERIES:
        assert getattr(L, name) is getattr(L.cdll, name)                      # a query is exposed raw, the status entries checked
    for name in ("tc_uncert_maps", "tc_calib_stats"):
        assert getattr(L, name).__name__ == name and getattr(L, name) is not getattr(L.cdll, name)


def test_sizes(built):
    from transception_amd import _lib
    L = _lib.lib()
    for bins, ncls in ((1, 1), (15, 9), (32, 16), (10, 2)):
        slots = 3 * bins + 4 + 3 * ncls
        assert L.tc_calib_out_slots(bins, ncls) == slots
        assert L.tc_calib_work_bytes(bins, ncls) > 0 and L.tc_calib_work_bytes(bins, ncls) % (8 * slots) == 0
    for bins, ncls in ((0, 9), (33, 9), (15, 0), (15, 17), (-1, -1)):
        assert L.tc_calib_out_slots(bins, ncls) == 0 and L.tc_calib_work_bytes(bins, ncls) == 0


def test_entries_refuse_bad_arguments_before_any_launch(built):
    """Argument checks come before any launch, so they run without a GPU: the addresses below are never dereferenced."""
    from transception_amd import _lib
    L = _lib.lib()
    S, VES, E, C, M, P, LAB, WK, OUT = (0x10000 * i for i in range(1, 10))
    F32, BF16, F16, LOGITS, SUMS = _lib.TC_F32, _lib.TC_BF16, _lib.TC_F16, _lib.TC_UNCERT_LOGITS, _lib.TC_UNCERT_PROB_SUMS

    def refused(name, args):
        with pytest.raises(_lib.TcError, match=name + " failed with status -1"):
            getattr(L, name)(*args, None)

    # scores, dtype, kind, inv_views, ves, entropy, confidence, mi, pred, N, ncls, H, W
    good = [S, F32, LOGITS, 1.0, VES, E, C, M, P, 2, 9, 8, 8]
    bad = [(0, None),                                                        # scores NULL
           (4, None), (7, None),                                             # mutual_info without view_entropy_sum, and the reverse
           (5, S), (6, S), (7, S), (8, S),                                   # an output aliasing the scores
           (2, 2), (2, -1), (1, 3), (1, -1),                                 # kind, dtype unknown
           (3, 0.0), (3, -0.25), (3, 1.5), (3, float("nan")), (3, float("inf")),
           (10, 0), (10, 17), (10, -1), (9, 0), (9, -2), (11, 0), (12, 0), (12, -5)]
    for pos, value in bad:
        args = list(good)
        args[pos] = value
        refused("tc_uncert_maps", args)
    refused("tc_uncert_maps", [S, F32, LOGITS, 1.0, None, None, None, None, None, 2, 9, 8, 8])       # every output NULL
    for dt in (BF16, F16):
        refused("tc_uncert_maps", [S, dt, SUMS, 0.25, VES, E, C, M, P, 2, 9, 8, 8])                  # PROB_SUMS with a 16-bit dtype
    refused("tc_uncert_maps", [S, F32, LOGITS, 1.0, VES, E, C, M, P, 16, 16, 4096, 2048])            # 2^31 elements, each extent legal
    refused("tc_uncert_maps", [S, F32, LOGITS, 1.0, VES, E, C, M, P, 32768, 16, 4096, 1])

    # scores, dtype, kind, inv_views, labels, ignore_index, flags, bins, N, ncls, H, W, work, out
    good = [S, F32, SUMS, 0.25, LAB, -1, 0, 15, 2, 9, 8, 8, WK, OUT]
    bad = [(0, None), (4, None), (12, None), (13, None),
           (2, 2), (1, 3), (1, BF16), (1, F16),                              # (PROB_SUMS with a 16-bit dtype)
           (3, 0.0), (3, -1.0), (3, 1.0001), (3, float("nan")),
           (7, 0), (7, 33), (7, -1), (6, 2), (6, 3), (6, -1), (6, 256),      # bins; unknown flag bits
           (9, 0), (9, 17), (8, 0), (10, 0), (11, -1)]
    for pos, value in bad:
        args = list(good)
        args[pos] = value
        refused("tc_calib_stats", args)
    refused("tc_calib_stats", [S, F32, LOGITS, 1.0, LAB, 255, 1, 15, 16, 16, 4096, 2048, WK, OUT])


# ---------------------------------------------------------------------------------------------------------------- validation
def test_calibration_validation():
    from transception_amd.evaluate import VALID_OPTION, Calibration
    c = Calibration()
    assert (c.bins, c.foreground_only, c.ignore_index) == (15, False, None)
    assert Calibration(np.int64(10), np.bool_(True), np.uint8(255)) == Calibration(10, True, 255)
    assert type(Calibration(np.int64(10)).bins) is int
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.bins = 10
    for bad in (0, 33, -1, True, 15.0, "15", None):
        with pytest.raises(ValueError, match="bins"):
            Calibration(bins=bad)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError, match="foreground_only"):
            Calibration(foreground_only=bad)
    for bad in (-1, 256, True, 1.0, "255"):
        with pytest.raises(ValueError, match="ignore_index"):
            Calibration(ignore_index=bad)
    assert VALID_OPTION["calibration"](None) and VALID_OPTION["calibration"](c) and not VALID_OPTION["calibration"](15)


def test_train_config_calibration():
    from transception_amd.evaluate import Calibration
    from transception_amd.trainer import KEYWORD_OPTIONS, TrainConfig
    assert TrainConfig("root", "lists").calibration is None and TrainConfig.calibration is None
    c = Calibration(bins=10)
    cfg = TrainConfig("root", "lists", calibration=c)
    assert cfg.calibration is c and "calibration=Calibration(bins=10" in repr(cfg) and repr(cfg).endswith("resample='labels')")
    for bad in (10, True, "on", (15,), {"bins": 15}):
        with pytest.raises(ValueError, match="calibration"):
            TrainConfig("root", "lists", calibration=bad)
    params = inspect.signature(TrainConfig).parameters
    assert params["calibration"].kind is inspect.Parameter.KEYWORD_ONLY and params["calibration"].default is None
    assert [o[0] for o in KEYWORD_OPTIONS][:2] == ["surface_metrics", "calibration"] and list(params)[-1] == "resample"
    assert "calibration" not in [f.name for f in dataclasses.fields(TrainConfig)]
    positional = [p.default for p in params.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD][2:]
    with pytest.raises(TypeError):
        TrainConfig("root", "lists", *positional, c)                          # not reachable by position


def test_bad_options_are_refused_before_anything_runs():
    """The model here is None: a ValueError must come before it or the device is touched."""
    from transception_amd import evaluate as E
    img, lab = np.zeros((1, 96, 96), np.float32), np.zeros((1, 96, 96), np.uint8)
    for bad in (None, 15, (15, False, None)):
        with pytest.raises(ValueError, match="calibration"):
            E.evaluate_volume_calibration(None, img, lab, patch_size=(64, 64), calibration=bad)
        with pytest.raises(ValueError, match="calibration"):
            E.inference_calibration(None, [(img, lab, "case")], calibration=bad)
    with pytest.raises(ValueError, match="tta"):
        E.evaluate_volume_calibration(None, img, lab, patch_size=(64, 64), tta=4)
    with pytest.raises(ValueError, match="square"):
        E.evaluate_volume_calibration(None, img, lab, patch_size=(64, 96), tta=E.TTA.dihedral())
    with pytest.raises(ValueError, match="inference_calibration"):
        E.inference_calibration(None, [])
    with pytest.raises(ValueError, match="kind"):
        E.uncertainty_maps(torch.zeros(1, 2, 2, 2), kind="probs")
    with pytest.raises(RuntimeError, match="MI355X"):
        E.uncertainty_maps(torch.zeros(1, 2, 2, 2))
    with pytest.raises(ValueError, match="views"):
        E.uncertainty_maps(torch.zeros(1, 2, 2, 2), views=0)
    sig = inspect.signature(E.predict_uncertainty).parameters
    assert list(sig) == ["model", "slices", "batch", "tta", "out_size"] and sig["out_size"].kind is inspect.Parameter.KEYWORD_ONLY
    assert E.Uncertainty._fields == ("pred", "entropy", "confidence", "mutual_information")
    # the prediction entries are what they were
    for fn in (E.predict_slices, E.predict_probs):
        assert list(inspect.signature(fn).parameters) == ["model", "slices", "batch", "tta", "out_size"]
    assert list(inspect.signature(E._predict).parameters)[:6] == ["model", "slices", "batch", "views", "out_size", "labels"]
    assert inspect.signature(E._predict).parameters["ves"].default is None


# ---------------------------------------------------------------------------------------------------------------- decoding
def raw_slots(table, totals, per_class):
    """int64 slots as the kernel leaves them, from (count, confidence sum, correct) rows, (n, nll, brier, correct) and per-class rows."""
    out = []
    for c, s, k in table:
        out += [c, int(round(s * 2 ** 32)), k]
    n, nll, brier, ok = totals
    out += [n, int(np.float64(nll).view(np.int64)), int(np.float64(brier).view(np.int64)), ok]
    for c, s, k in per_class:
        out += [c, int(round(s * 2 ** 32)), k]
    return np.array(out, dtype=np.int64)


def test_calibration_from_stats_on_hand_made_slots():
    from transception_amd.evaluate import calibration_from_stats, decode_calibration_stats
    # 4 bins, 2 classes; bin 1 is empty
    table = [(4, 4 * 0.125, 1), (0, 0.0, 0), (8, 8 * 0.625, 4), (4, 4 * 0.875, 4)]
    raw = raw_slots(table, (16, 8.0, 4.0, 9), [(10, 10 * 0.5, 6), (6, 6 * 0.25, 3)])
    d = calibration_from_stats(raw, 4, 2)
    gaps = [abs(1 / 4 - 0.125), abs(4 / 8 - 0.625), abs(4 / 4 - 0.875)]
    assert d["n"] == 16 and d["nll"] == 0.5 and d["brier"] == 0.25 and d["accuracy"] == 9 / 16
    assert d["ece"] == (4 * gaps[0] + 8 * gaps[1] + 4 * gaps[2]) / 16 and d["mce"] == max(gaps)
    assert d["bins"] == [{"count": 4, "confidence": 0.125, "accuracy": 0.25}, {"count": 0, "confidence": 0.0, "accuracy": 0.0},
                         {"count": 8, "confidence": 0.625, "accuracy": 0.5}, {"count": 4, "confidence": 0.875, "accuracy": 1.0}]
    assert d["classes"] == [{"count": 10, "entropy": 0.5, "accuracy": 0.6}, {"count": 6, "entropy": 0.25, "accuracy": 0.5}]
    # decoded slots add: twice the same statistics is the same calibration, from a tensor as from an array
    dec = decode_calibration_stats(raw, 4)
    assert dec.dtype == np.float64 and dec[0] == 4 and dec[1] == 0.5 and dec[13] == 8.0 and dec[14] == 4.0 and dec[17] == 5.0
    assert torch.equal(decode_calibration_stats(torch.from_numpy(raw), 4), torch.from_numpy(dec))
    twice = calibration_from_stats(dec + dec, 4, 2)
    assert twice["n"] == 32 and all(twice[k] == d[k] for k in ("ece", "mce", "nll", "brier", "accuracy"))
    # n = 0: all zeros, no NaN
    zero = calibration_from_stats(np.zeros(3 * 4 + 4 + 3 * 2, np.int64), 4, 2)
    assert zero["n"] == 0 and all(zero[k] == 0.0 for k in ("ece", "mce", "nll", "brier", "accuracy"))
    assert all(r == {"count": 0, "confidence": 0.0, "accuracy": 0.0} for r in zero["bins"])
    assert all(r == {"count": 0, "entropy": 0.0, "accuracy": 0.0} for r in zero["classes"])
    # perfectly calibrated: the accuracy of every bin is its mean confidence
    perfect = raw_slots([(8, 8 * 0.25, 2), (4, 4 * 0.5, 2), (4, 4 * 0.75, 3), (0, 0.0, 0)], (16, 1.0, 1.0, 7), [(16, 0.0, 7), (0, 0.0, 0)])
    p = calibration_from_stats(perfect, 4, 2)
    assert p["ece"] == 0.0 and p["mce"] == 0.0 and p["accuracy"] == 7 / 16
    for bad in (raw[:-1], raw.astype(np.int32), np.zeros((2, 11))):
        with pytest.raises(ValueError):
            calibration_from_stats(bad, 4, 2)


# ---------------------------------------------------------------------------------------------------------------- the host counterpart
def brute_force(probs, labels, bins, ignore_index, foreground):
    N, C, H, W = probs.shape
    table = [[0, 0.0, 0] for _ in range(bins)]
    per_class = [[0, 0.0, 0] for _ in range(C)]
    n = ok = 0
    nll, brier = [], []
    for i in range(N):
        for r in range(H):
            for q in range(W):
                p, y = [float(v) for v in probs[i, :, r, q]], int(labels[i, r, q])
                pred = max(range(C), key=lambda k: (p[k], -k))
                if y >= C or y == ignore_index or (foreground and y == 0 and pred == 0):
                    continue
                conf = p[pred]
                b = min(bins - 1, int(np.float32(conf) * np.float32(bins)))
                h = -sum(v * math.log(v) for v in p if v > 0) / math.log(C) if C > 1 else 0.0
                h = min(1.0, max(0.0, h))
                for row, s in ((table[b], math.floor(conf * 2 ** 32) / 2 ** 32), (per_class[pred], h)):
                    row[0] += 1; row[1] += s; row[2] += int(pred == y)
                n += 1; ok += int(pred == y)
                nll.append(-math.log(max(p[y], R.FLT_MIN)))
                brier.append(sum((v - (k == y)) ** 2 for k, v in enumerate(p)))
    return table, (n, math.fsum(nll), math.fsum(brier), ok), per_class


@pytest.mark.parametrize("bins,ignore_index,foreground", [(15, None, False), (10, 7, False), (16, 7, True), (1, None, True)])
def test_calibration_host_against_a_brute_force_loop(bins, ignore_index, foreground):
    from transception_amd.evaluate import Calibration, calibration_from_stats, calibration_host, calibration_stats_host
    shape = (2, 5, 6, 7)
    probs = (R.seeded_prob_sums(shape, 3, seed=5).double() / 3).to(torch.float32).numpy()
    probs[0, :, 0, 0] = (1.0, 0.0, 0.0, 0.0, 0.0)                             # a zero probability, confidence 1: the last bin
    probs[0, :, 0, 1] = (0.0, 0.5, 0.5, 0.0, 0.0)                             # a tie: the lower class
    labels = R.seeded_labels(shape, seed=5, extra=(7, 5)).numpy()
    labels[0, 0, :2] = (3, 2)
    cal = Calibration(bins, foreground, ignore_index)
    table, totals, per_class = brute_force(probs, labels, bins, ignore_index, foreground)
    got = calibration_stats_host(probs, labels, cal)
    want = np.array([v for row in table for v in row] + list(totals) + [v for row in per_class for v in row])
    assert got.shape == want.shape and got.dtype == np.float64
    counts = np.ones(len(want), bool)
    counts[1:3 * bins:3] = counts[3 * bins + 5::3] = False
    counts[3 * bins + 1:3 * bins + 3] = False
    assert np.array_equal(got[counts], want[counts]) and totals[0] > 0
    assert np.allclose(got[~counts], want[~counts], rtol=1e-13, atol=1e-13)
    d = calibration_host(probs, labels, cal)
    assert set(d) == {"ece", "mce", "nll", "brier", "accuracy", "n", "bins", "classes", "stats"} and np.array_equal(d["stats"], got)
    ref = calibration_from_stats(want, bins, 5)
    for key in ("ece", "mce", "nll", "brier", "accuracy"):
        assert d[key] == pytest.approx(ref[key], rel=1e-12, abs=1e-15), key
    assert d["n"] == totals[0] and 0.0 <= d["ece"] <= d["mce"] <= 1.0
    # everything ignored: all zeros
    none = calibration_host(probs, np.full_like(labels, 7), Calibration(bins, foreground, 7))
    assert none["n"] == 0 and not none["stats"].any() and none["ece"] == 0.0


# ---------------------------------------------------------------------------------------------------------------- number facts
def test_number_facts_the_gpu_equalities_rest_on():
    # logits 0 and -200: the other classes vanish exactly, so s = 1, p = 1, H = log 1 - 0 = 0
    assert np.exp(np.float32(-200.0)) == 0.0 and np.log(np.float32(1.0)) == 0.0
    for dt in (torch.bfloat16, torch.float16):
        assert float(torch.tensor(-200.0).to(dt)) == -200.0 and float(torch.tensor(1.0).to(dt)) == 1.0
    # multiples of 1/64 summing to 4: stored exactly in fp32, p = t * 0.25 exact, conf * 2^32 an exact integer, squares and their sums exact
    for shape in R.SHAPES:
        t, planted = R.dyadic_prob_sums(shape, seed=3)
        x = t.numpy()
        assert np.array_equal(x.astype(np.float64) * 64, np.round(x.astype(np.float64) * 64))
        p = x * np.float32(0.25)
        assert np.array_equal(p.astype(np.float64), x.astype(np.float64) / 4)
        if planted == 0:
            assert np.array_equal(x.sum(axis=1, dtype=np.float64), np.full(x.sum(axis=1).shape, 4.0))
        d2 = (p.astype(np.float64) - 1.0) ** 2
        assert np.array_equal(d2.astype(np.float32).astype(np.float64), d2)
        conf = p.max(axis=1)
        assert conf.min() >= 2.0 ** -8 and np.array_equal(np.floor(conf.astype(np.float64) * 2 ** 32), conf.astype(np.float64) * 2 ** 32)
        if planted:
            em = R.emulate_prob_sums(t, 4, R.seeded_labels(shape, seed=3), 16)
            assert (em["table"][:, 0] > 0).all()                              # every bin, bin 0 included
            edges = np.isin(em["conf"].astype(np.float64) * 16, np.arange(1, 16))
            assert edges.sum() >= 15                                          # a confidence exactly on every inner edge
    assert float(np.float32(1.0 / 3)) != 1.0 / 3 and np.float32(1.0 / 4) == 0.25
    # an edge belongs to the bin above it: conf = b / 16 exactly goes to bin b
    for b in range(1, 16):
        assert int(np.float32(b / 16) * np.float32(16)) == b


@pytest.mark.parametrize("name", list(R.TORCH_DTYPES))
def test_float32_entropy_stays_under_the_bound_on_the_seeded_inputs(name):
    """The header's fp32 expression of h, emulated in NumPy float32 on the inputs of the GPU test, against the float64 model: a formula whose
    rounding alone broke the bound would show here, without a GPU."""
    worst = 0.0
    for i, shape in enumerate(R.SHAPES):
        logits = R.seeded_logits(shape, R.TORCH_DTYPES[name], seed=10 + i, scale=1.0 + i % 3)
        h = R.emulate_entropy_logits(logits)
        worst = max(worst, float(np.abs(h.astype(np.float64) - R.model(logits, "logits")["h"].numpy()).max()))
    assert worst <= R.ENTROPY_BOUND <= R.ENTROPY_CAP, worst


def test_safe_vector_is_safe_and_few_pixels_are_replaced():
    for i, shape in enumerate(R.SHAPES):
        C = shape[1]
        conf = float(R.model(R.safe_vector(C).view(1, C, 1, 1), "logits")["conf"])
        for bins in (10, 15, 16):
            pos = conf * bins
            assert C == 1 or abs(pos - round(pos)) > 0.01, (C, bins)
        for name, dt in R.TORCH_DTYPES.items():
            safe, share = R.make_safe(R.seeded_logits(shape, dt, seed=10 + i, scale=1.0 + i % 3))
            assert share <= 0.01 and R.make_safe(safe)[1] == 0.0, (shape, name, share)

"""The prediction loop of evaluate.py (predict_slices, predict_probs, evaluate_volume) as a contract: which C-ABI entries every call makes
per batch and in which order, the bits it returns, and the memory it holds at its peak.

The bits and the peaks are recorded in tests/golden/predict_paths.json from the code as it stood before the loop was consolidated: the
SHA-256 of each returned tensor's bytes, `float.hex` of every metric `evaluate_volume` returns and, for two label calls with views, the peak
of `torch.cuda.max_memory_allocated()` above the allocation before the call.  `compute()` below is what wrote the file and what the tests
run again; the comparison is equality (for the peaks: not larger).  Everything in it is elementwise torch work plus kernels that write each
element from one thread, and integer atomics in the metrics, so nothing is order-dependent: the file was written twice and compared.

3 slices of 32 x 48 with batch 2 -- two batches, the second short; not square, so only flip views are legal -- and out_size (40, 56)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from transception_amd import _lib  # noqa: E402
from transception_amd._lib import lib  # noqa: E402

DEV = "cuda:0"
N, H, W, BATCH = 3, 32, 48, 2
OTHER = (40, 56)
VIEW, ACC, ARGMAX, RESAMPLE = "tc_tta_view", "tc_tta_accumulate", "tc_argmax_counts", "tc_resample_scores"
#        name                        function          views     out_size  entries per batch
ROWS = [("slices",                   "predict_slices", None,     None,     [ARGMAX]),
        ("slices_other",             "predict_slices", None,     OTHER,    [RESAMPLE]),
        ("slices_views03",           "predict_slices", (0, 3),   None,     [VIEW, ACC] * 2),
        ("slices_view2",             "predict_slices", (2,),     None,     [VIEW, ACC]),
        ("slices_views03_other",     "predict_slices", (0, 3),   OTHER,    [VIEW, ACC] * 2 + [RESAMPLE]),
        ("probs",                    "predict_probs",  None,     None,     [VIEW, ACC]),
        ("probs_views03",            "predict_probs",  (0, 3),   None,     [VIEW, ACC] * 2),
        ("probs_views03_other",      "predict_probs",  (0, 3),   OTHER,    [VIEW, ACC] * 2 + [RESAMPLE])]
PEAK_ROWS = ("slices_views03", "slices_views03_other")
OPTION_SETS = ("default", "hd95", "host_zoom", "device_hd95", "device_post", "host_zoom_post", "scores", "scores_flips_device_hd95",
               "spacing_hd95", "spacing_device_hd95")                                 # of evaluate_volume: `option_sets` below
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_paths.json")


class _Stub(torch.nn.Module):
    """The stub of tests/test_tta_gpu.py -- logits that depend on the intensity and on the absolute position, so that the views disagree --
    which records only the mode it ran in: no clones, so that the peak of the allocator is the loop's and the forward's alone."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self.modes = []

    def forward(self, x):
        _, _, h, w = x.shape
        k = torch.round((x[:, 0] * 0.5 + 0.5) * 8).long().clamp(0, 8)
        hot = torch.nn.functional.one_hot(k, 9).permute(0, 3, 1, 2).float()
        c = torch.arange(9, device=x.device, dtype=torch.float32).view(1, 9, 1, 1)
        r = torch.arange(h, device=x.device, dtype=torch.float32).view(1, 1, h, 1)
        q = torch.arange(w, device=x.device, dtype=torch.float32).view(1, 1, 1, w)
        self.modes.append(self.training)
        return (6.0 * hot + 2.5 * torch.sin(0.9 * c + 0.21 * r) + 2.5 * torch.cos(1.3 * c - 0.17 * q)).contiguous()


def stub_slices():
    g = torch.Generator().manual_seed(3)
    return (torch.randint(0, 9, (N, H, W), generator=g).float() / 8).to(DEV)


def call(row, model, slices, out_size="row"):
    from transception_amd import evaluate as E
    _, fn, views, size, _ = row
    return getattr(E, fn)(model, slices, batch=BATCH, tta=None if views is None else E.TTA(views), out_size=size if out_size == "row" else out_size)


def sha(t: torch.Tensor) -> str:
    t = t.detach().cpu().contiguous()
    return f"{str(t.dtype).replace('torch.', '')}{list(t.shape)}:" + hashlib.sha256(t.numpy().tobytes()).hexdigest()


def volume():
    """A blocky 6 x 64 x 64 image of levels k / 8 and labels derived from it, shifted by a pixel (`volume` of tests/test_resample_gpu.py)."""
    g = np.random.default_rng(33)
    lab = np.kron(g.integers(0, 9, (6, 8, 8)), np.ones((8, 8), np.int64)).astype(np.uint8)
    return (lab / 8).astype(np.float32), np.roll(lab, 1, axis=2)


def option_sets():
    from transception_amd.evaluate import TTA, PostProcess
    post, spacing = PostProcess("min_voxels", 3), (2.0, 0.5, 0.75)
    return {"default": dict(),
            "hd95": dict(with_hd95=True),
            "host_zoom": dict(host_zoom=True),
            "device_hd95": dict(device_metrics=True, with_hd95=True),
            "device_post": dict(device_metrics=True, postprocess=post),
            "host_zoom_post": dict(host_zoom=True, postprocess=post),
            "scores": dict(resample="scores"),
            "scores_flips_device_hd95": dict(resample="scores", tta=TTA.flips(), device_metrics=True, with_hd95=True),
            "spacing_hd95": dict(voxelspacing=spacing, with_hd95=True),
            "spacing_device_hd95": dict(voxelspacing=spacing, with_hd95=True, device_metrics=True)}


def compute() -> dict:
    """Everything the golden file holds, from the package as it is."""
    from transception_amd.evaluate import evaluate_volume
    slices, m = stub_slices(), _Stub().to(DEV).eval()
    out = {"predict": {}, "evaluate": {}, "peak_bytes": {}}
    for row in ROWS:
        out["predict"][row[0]] = sha(call(row, m, slices))
    for row in ROWS:
        if row[0] in PEAK_ROWS:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            res = call(row, m, slices)
            torch.cuda.synchronize()
            out["peak_bytes"][row[0]] = torch.cuda.max_memory_allocated() - before
            del res
    image, gt = volume()
    for name, kw in option_sets().items():
        got = evaluate_volume(m, image, gt, 9, (48, 48), batch=4, **kw)
        out["evaluate"][name] = [[float(v).hex() for v in case] if isinstance(case, tuple) else float(case).hex() for case in got]
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def computed():
    return compute()


# ---------------------------------------------------------------------------------------------------------------- 1. launch sequence
@pytest.fixture
def entries(monkeypatch):
    """[names of the non-query entries called], recorded on the loaded library object."""
    L, seen = lib(), []
    for header in (_lib.ABI, _lib.POST, _lib.EMA, _lib.TTA, _lib.RESAMPLE):
        for name, f in header.functions.items():
            if f.query:
                continue

            def recorded(*a, _name=name, _real=getattr(L, name)):
                seen.append(_name)
                return _real(*a)

            monkeypatch.setattr(L, name, recorded)
    return seen


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_entries_per_batch(row, entries):
    slices = stub_slices()
    for training in (True, False):
        m = _Stub().to(DEV).train(training)
        del entries[:]
        call(row, m, slices)
        assert entries == row[4] * 2                                                  # two batches
        nviews = len(row[2]) if row[2] else 1
        assert m.modes == [False] * (2 * nviews) and m.training is training            # eval inside, restored after
    # out_size equal to the slices' size: the row without out_size
    plain = next(r for r in ROWS if r[1:4] == (row[1], row[2], None))
    del entries[:]
    call(row, m, slices, out_size=(H, W))
    assert entries == plain[4] * 2


# ---------------------------------------------------------------------------------------------------------------- 2. the same bits
def test_the_golden_file_is_complete(golden):
    assert sorted(golden["predict"]) == sorted(r[0] for r in ROWS)                     # none of the eight calls may be left out
    assert sorted(golden["peak_bytes"]) == sorted(PEAK_ROWS)
    assert sorted(golden["evaluate"]) == sorted(OPTION_SETS) == sorted(option_sets())


@pytest.mark.parametrize("name", [r[0] for r in ROWS])
def test_predictions_are_the_recorded_bits(name, golden, computed):
    assert computed["predict"][name] == golden["predict"][name]


@pytest.mark.parametrize("name", OPTION_SETS)
def test_evaluate_volume_returns_the_recorded_floats(name, golden, computed):
    assert computed["evaluate"][name] == golden["evaluate"][name]


# ---------------------------------------------------------------------------------------------------------------- 3. no new buffers
@pytest.mark.parametrize("name", PEAK_ROWS)
def test_peak_memory_is_not_larger(name, golden, computed):
    print(f"peak bytes of {name}: {computed['peak_bytes'][name]} (recorded {golden['peak_bytes'][name]})")
    assert computed["peak_bytes"][name] <= golden["peak_bytes"][name]

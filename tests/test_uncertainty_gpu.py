"""Uncertainty maps and calibration statistics on the device (csrc/uncertainty.hip: tc_uncert_maps, tc_calib_stats; evaluate.uncertainty_maps,
predict_uncertainty, calibration_stats, evaluate_volume_calibration, inference_calibration, TrainConfig.calibration) against the float64
model and the float32 emulation of tests/uncertainty_ref.py.

Equalities: logits 0 at one class and -200 elsewhere make every quantity 0 or 1 exactly; probability sums that are multiples of 1/64
make every sum the kernel forms exact; and for ANY probability sums the bin table and every count follow from one fp32 multiply and one
truncation, which NumPy float32 repeats to the bit.  Bounds, on seeded normals stored in the tested dtype: confidence within the project's
2e-6 of the float64 model; the label within twice that of the model's maximum; the entropy bound (uncertainty_ref.ENTROPY_BOUND) for the
entropy, the mutual information and, per pixel, the per-class entropy sums; n (entropy bound x log C + 2e-6 C) for the NLL and Brier sums.

MEASURED on the MI355X (printed by test_logits_bounds and test_prob_sums_any_input; 82 tests, 6.4 s): worst |conf - model| 3.39e-7 (bound
2e-6); worst |h - model| 2.522e-7 (sums of three views, 3 x 16 x 33 x 33; 1.84e-7 on logits), hence ENTROPY_BOUND = 4 x 2.522e-7 = 1.009e-6,
under the cap of 2e-5; worst |mi - model| 2.48e-7; per counted pixel, worst |sum nll - model| 1.63e-7 and worst |sum brier - model| 2.96e-8
against n (ENTROPY_BOUND x log C + 2e-6 C) = 2.0e-5 n at nine classes; replaced (unsafe) pixels: at most 0.9 % (bf16, where stored ties are common).  Through
predict_uncertainty with the position-dependent stub (float64 model of the float64 sums, the device on its fp32 accumulator): worst |h - model|
1.31e-7 and worst |mi - model| 1.47e-7 (flips, 5 x 7), 1.19e-7 for the mutual information at out_size: all under ENTROPY_BOUND as it is.
With the real network at 64 x 64: |nll - host| 9.1e-8, |brier - host| 4.0e-10 per pixel, every count and confidence sum equal."""
import math

import numpy as np
import pytest
import torch

import uncertainty_ref as R
from tta_ref import unview

pytestmark = pytest.mark.gpu

from transception_amd import _lib  # noqa: E402
from transception_amd._lib import lib  # noqa: E402

DEV = "cuda:0"
EXTRA = [(1, 16, 8, 24), (1, 5, 2, 6)]       # 16 classes on the 16-byte pieces of every dtype; a plane of 12: pieces in fp32, single pixels in 16 bit
SHAPES = R.SHAPES + EXTRA
TC = {"fp32": _lib.TC_F32, "bf16": _lib.TC_BF16, "fp16": _lib.TC_F16}
LOGITS, SUMS = _lib.TC_UNCERT_LOGITS, _lib.TC_UNCERT_PROB_SUMS
GUARD = 64
FIXED = 2.0 ** -32                            # what the truncation of a fixed-point term can lose


def sid(shape):
    return "x".join(map(str, shape))


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def guarded(numel, dtype, fill, off=0):
    """(flat, view): `numel` elements of a buffer filled with `fill`, GUARD + off elements in: guards on both sides, base misaligned by `off`."""
    flat = torch.full((numel + 2 * GUARD + 1,), fill, dtype=dtype, device=DEV)
    return flat, flat[GUARD + off:GUARD + off + numel]


def guards_intact(flat, numel, fill, off=0):
    return bool((flat[:GUARD + off] == fill).all()) and bool((flat[GUARD + off + numel:] == fill).all())


def placed(t, off=0):
    """`t` on the device, contiguous, its base `off` elements past an allocation's (aligned) start."""
    flat = torch.empty(t.numel() + off + 8, dtype=t.dtype, device=DEV)
    view = flat[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() == flat.data_ptr() + off * t.element_size()
    return view


def run_maps(scores, kind, views=1, ves=None, want="ecmp", off=0):
    """tc_uncert_maps on host tensors; the outputs named in `want` (e c m p) inside sentinel guards.  Returns {letter: cpu tensor}."""
    N, C, H, W = scores.shape
    sc = placed(scores, off)
    vs = None if ves is None else placed(ves, off)
    out = {}
    for letter in want:
        dtype, fill = (torch.uint8, 201) if letter == "p" else (torch.float32, -7.25)
        out[letter] = guarded(N * H * W, dtype, fill, off) + (fill,)
    ptr = lambda letter: out[letter][1].data_ptr() if letter in out else None
    lib().tc_uncert_maps(sc.data_ptr(), TC[{torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[scores.dtype]], kind,
                         float(np.float32(1.0 / views)), None if vs is None else vs.data_ptr(), ptr("e"), ptr("c"), ptr("m"), ptr("p"), N, C, H, W, stream())
    torch.cuda.synchronize()
    for letter, (flat, _, fill) in out.items():
        assert guards_intact(flat, N * H * W, fill, off), f"output {letter} written outside its map"
    return {letter: view.view(N, H, W).cpu() for letter, (_, view, _) in out.items()}


def run_calib(scores, kind, labels, bins, views=1, ignore_index=-1, flags=0, off=0):
    """tc_calib_stats on host tensors: the raw int64 slots (NumPy).  `work` is filled with garbage, `out` sits inside sentinel guards."""
    N, C, H, W = scores.shape
    sc, lab = placed(scores, off), placed(labels, off)
    L = lib()
    slots, wbytes = L.tc_calib_out_slots(bins, C), L.tc_calib_work_bytes(bins, C)
    assert slots == 3 * bins + 4 + 3 * C and wbytes > 0
    work = torch.full((wbytes // 8,), 0x7f7f5a5a7f7f5a5a, dtype=torch.int64, device=DEV)
    flat, out = guarded(slots, torch.int64, -99)
    L.tc_calib_stats(sc.data_ptr(), TC[{torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}[scores.dtype]], kind,
                     float(np.float32(1.0 / views)), lab.data_ptr(), ignore_index, flags, bins, N, C, H, W, work.data_ptr(), out.data_ptr(), stream())
    torch.cuda.synchronize()
    assert guards_intact(flat, slots, -99)
    return out.cpu().numpy()


def split(raw, bins, C):
    """(table [bins,3] int64, n, nll, brier, correct, per_class [C,3] int64) of raw slots."""
    t = raw[3 * bins:3 * bins + 4]
    return (raw[:3 * bins].reshape(bins, 3), int(t[0]), float(t[1:2].view(np.float64)[0]), float(t[2:3].view(np.float64)[0]), int(t[3]),
            raw[3 * bins + 4:].reshape(C, 3))


# ---------------------------------------------------------------------------------------------------------------- 1. equalities
@pytest.mark.parametrize("name", list(TC))
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_one_hot_logits_are_exact(shape, name):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(7)
    hot = torch.randint(0, C, (N, H, W), generator=g)
    logits = torch.full(shape, -200.0).scatter_(1, hot.unsqueeze(1), 0.0).to(R.TORCH_DTYPES[name])
    for off in (0, 1):
        m = run_maps(logits, LOGITS, want="ecp", off=off)
        assert bool((m["c"] == 1.0).all()) and bool((m["e"] == 0.0).all()) and torch.equal(m["p"].long(), hot)
    labels = hot.to(torch.uint8)
    labels[0, 0, 0] = (int(hot[0, 0, 0]) + 1) % max(C, 2)                     # one wrong pixel (one class: label 1 >= C, not counted)
    raw = run_calib(logits, LOGITS, labels, 15)
    table, n, nll, brier, ok, per_class = split(raw, 15, C)
    wrong = 1 if C > 1 else 0
    assert n == N * H * W - (C == 1) and ok == n - wrong
    assert table[:14].sum() == 0 and list(table[14]) == [n, n << 32, ok]
    keep = labels.long() < C
    assert list(per_class[:, 0]) == np.bincount(hot[keep].numpy(), minlength=C).tolist() and per_class[:, 1].sum() == 0 and per_class[:, 2].sum() == ok
    # the wrong pixel: p_y = expf(-200) / 1 = 0 exactly, so nll = logf(1) - (-200) and brier = 1 + 1
    assert (nll, brier) == ((200.0, 2.0) if wrong else (0.0, 0.0))
    # equal logits: the lower class, the uniform distribution's entropy
    m = run_maps(torch.full(shape, 0.5).to(R.TORCH_DTYPES[name]), LOGITS, want="ecp")
    assert bool((m["p"] == 0).all()) and float((m["c"].double() - 1.0 / C).abs().max()) <= R.PER_VIEW
    assert bool((m["e"] == (1.0 if C > 1 else 0.0)).all())


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_dyadic_prob_sums_every_slot_is_the_emulation(shape):
    """Sums of four views' probabilities in multiples of 1/64, 16 bins: some confidences sit exactly on an edge, and in the shapes with room
    every bin is filled.  Every slot of the bin table, n, the correct count, the per-class counts and the Brier sum equal the float32 emulation."""
    N, C, H, W = shape
    t, planted = R.dyadic_prob_sums(shape, seed=3)
    labels = R.seeded_labels(shape, seed=3)
    em = R.emulate_prob_sums(t, 4, labels, 16)
    for off in (0, 1):
        raw = run_calib(t, SUMS, labels, 16, views=4, off=off)
        table, n, nll, brier, ok, per_class = split(raw, 16, C)
        assert np.array_equal(table, em["table"]) and (n, ok) == (em["n"], em["correct"]) and n == N * H * W
        assert np.array_equal(per_class[:, [0, 2]], em["per_class"]) and brier == em["brier"]
    if planted:
        assert (table[:, 0] > 0).all()
    m = run_maps(t, SUMS, views=4, want="cp")
    assert np.array_equal(m["c"].numpy(), em["conf"]) and np.array_equal(m["p"].numpy(), em["pred"].astype(np.uint8))


@pytest.mark.parametrize("bins", [10, 15])
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_prob_sums_any_input(shape, bins):
    """Seeded normals through a float64 softmax, three views summed and rounded to fp32 once, inv_views = (float)(1 / 3): the whole bin
    table and all counts equal the float32 emulation -- with an ignored value, labels >= C and the foreground rule --; the maps and the
    float sums are within the bounds of the float64 model (p = t / 3)."""
    N, C, H, W = shape
    t = R.seeded_prob_sums(shape, 3, seed=20 + bins)
    labels = R.seeded_labels(shape, seed=20, extra=(200, C))
    m64 = R.model(t, "prob_sums", 3, labels)
    ves = (torch.rand((N, H, W), generator=torch.Generator().manual_seed(4)) * 3).float()
    got = run_maps(t, SUMS, views=3, ves=ves, off=1)
    em = R.emulate_prob_sums(t, 3, labels, bins)
    assert np.array_equal(got["c"].numpy(), em["conf"]) and np.array_equal(got["p"].numpy(), em["pred"].astype(np.uint8))
    dev_h = float((got["e"].double() - m64["h"]).abs().max())
    mi = (m64["h"] - ves.double() * float(np.float32(1.0 / 3))).clamp(min=0.0)
    dev_mi = float((got["m"].double() - mi).abs().max())
    print(f"prob_sums {sid(shape)}: max |h - model| {dev_h:.3e}, max |mi - model| {dev_mi:.3e}")
    assert dev_h <= R.ENTROPY_BOUND and dev_mi <= R.ENTROPY_BOUND and bool((got["m"] >= 0).all())
    for ignore_index, flags in ((-1, 0), (200, 0), (200, 1), (300, 1)):
        ii = ignore_index if 0 <= ignore_index <= 255 else None
        em = R.emulate_prob_sums(t, 3, labels, bins, ii, bool(flags))
        raw = run_calib(t, SUMS, labels, bins, views=3, ignore_index=ignore_index, flags=flags)
        table, n, nll, brier, ok, per_class = split(raw, bins, C)
        assert np.array_equal(table, em["table"]) and (n, ok) == (em["n"], em["correct"])
        assert np.array_equal(per_class[:, [0, 2]], em["per_class"])
        want = R.stats_model(m64, labels, bins, C, ii, bool(flags), conf=torch.from_numpy(em["conf"].astype(np.float64)),
                             pred=torch.from_numpy(em["pred"]))
        assert n == want[3 * bins] and abs(nll - want[3 * bins + 1]) <= R.sums_bound(n, C) and abs(brier - want[3 * bins + 2]) <= R.sums_bound(n, C)
        hsum = per_class[:, 1].astype(np.float64) * FIXED
        assert (np.abs(hsum - want[3 * bins + 5::3]) <= per_class[:, 0] * (R.ENTROPY_BOUND + FIXED)).all()
        if n:
            print(f"  ignore {ignore_index} flags {flags}: n {n}, |nll - model| / n {abs(nll - want[3 * bins + 1]) / n:.3e}, "
                  f"|brier - model| / n {abs(brier - want[3 * bins + 2]) / n:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 2. bounds on the logits
@pytest.mark.parametrize("name", list(TC))
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_logits_bounds(shape, name):
    """Seeded normals x 1, 2 or 3 stored in the tested dtype, against the float64 model of the stored values.

    MEASURED on the MI355X over these shapes and dtypes: worst |conf - model| 3.39e-7 (4 x 9 x 96 x 96, fp16), worst |h - model| 1.84e-7 (the
    same case; 2.522e-7 in test_prob_sums_any_input, which sets ENTROPY_BOUND = 1.009e-6), worst |mi - model| 1.84e-7; per counted pixel, worst
    |sum nll - model| 9.5e-8 and |sum brier - model| 2.7e-8 (both 1 x 5 x 2 x 6) against bounds of 2.0e-5 (C = 9) to 3.5e-5 (C = 16)."""
    N, C, H, W = shape
    i = SHAPES.index(shape)
    logits = R.seeded_logits(shape, R.TORCH_DTYPES[name], seed=10 + i, scale=1.0 + i % 3)
    m64 = R.model(logits, "logits")
    ves = (torch.rand((N, H, W), generator=torch.Generator().manual_seed(5)) * 4).float()
    got = run_maps(logits, LOGITS, views=4, ves=ves)
    dev_c = float((got["c"].double() - m64["conf"]).abs().max())
    dev_h = float((got["e"].double() - m64["h"]).abs().max())
    mi = (m64["h"] - ves.double() * 0.25).clamp(min=0.0)
    dev_mi = float((got["m"].double() - mi).abs().max())
    at_pred = m64["p"].gather(1, got["p"].long().unsqueeze(1))[:, 0]
    print(f"logits {sid(shape)} {name}: max |conf - model| {dev_c:.3e}, max |h - model| {dev_h:.3e}, max |mi - model| {dev_mi:.3e}")
    assert dev_c <= R.PER_VIEW and bool((at_pred >= m64["conf"] - 2 * R.PER_VIEW).all())
    assert dev_h <= R.ENTROPY_BOUND and dev_mi <= R.ENTROPY_BOUND and bool((got["m"] >= 0).all())
    assert bool((got["e"] >= 0).all()) and bool((got["e"] <= 1).all())
    # the statistics, on safe pixels: counts are equalities, sums are bounded
    safe, share = R.make_safe(logits)
    assert share <= 0.01
    labels = R.seeded_labels(shape, seed=10 + i, extra=(200, C))
    m64 = R.model(safe, "logits", 1, labels)
    for bins, ignore_index, flags in ((10, -1, 0), (15, 200, 0), (16, 200, 1)):
        want = R.stats_model(m64, labels, bins, C, ignore_index if ignore_index >= 0 else None, bool(flags))
        for off in (0, 1):
            raw = run_calib(safe, LOGITS, labels, bins, ignore_index=ignore_index, flags=flags, off=off)
            table, n, nll, brier, ok, per_class = split(raw, bins, C)
            assert np.array_equal(table[:, 0], want[0:3 * bins:3]) and np.array_equal(table[:, 2], want[2:3 * bins:3])
            assert (n, ok) == (want[3 * bins], want[3 * bins + 3])
            assert np.array_equal(per_class[:, 0], want[3 * bins + 4::3]) and np.array_equal(per_class[:, 2], want[3 * bins + 6::3])
            assert (np.abs(table[:, 1] * FIXED - want[1:3 * bins:3]) <= table[:, 0] * (R.PER_VIEW + FIXED)).all()
            assert (np.abs(per_class[:, 1] * FIXED - want[3 * bins + 5::3]) <= per_class[:, 0] * (R.ENTROPY_BOUND + FIXED)).all()
            assert abs(nll - want[3 * bins + 1]) <= R.sums_bound(n, C) and abs(brier - want[3 * bins + 2]) <= R.sums_bound(n, C)
        if n:
            print(f"  bins {bins}: n {n}, |nll - model| / n {abs(nll - want[3 * bins + 1]) / n:.3e}, |brier - model| / n "
                  f"{abs(brier - want[3 * bins + 2]) / n:.3e}, bound / n {R.sums_bound(1, C):.3e}")


# ---------------------------------------------------------------------------------------------------------------- 3. hygiene
@pytest.mark.parametrize("shape", [SHAPES[4], SHAPES[5], EXTRA[0]], ids=sid)
def test_null_outputs_all_ignored_and_run_to_run(shape):
    N, C, H, W = shape
    logits = R.seeded_logits(shape, torch.bfloat16, seed=31, scale=2.0)
    ves = torch.rand((N, H, W), generator=torch.Generator().manual_seed(6)).float() * 2
    full = run_maps(logits, LOGITS, views=2, ves=ves)
    for want in ("e", "c", "p", "m", "cp"):                                   # an output that is not given is NULL: the others are what they were
        part = run_maps(logits, LOGITS, views=2, ves=ves if "m" in want else None, want=want, off=1)
        assert all(torch.equal(part[k], full[k]) for k in want)
    again = run_maps(logits, LOGITS, views=2, ves=ves)
    assert all(torch.equal(again[k], full[k]) for k in full)
    labels = R.seeded_labels(shape, seed=31, extra=(255,))
    for kind, scores, views in ((LOGITS, logits, 1), (SUMS, R.seeded_prob_sums(shape, 3, seed=32), 3)):
        a, b = (run_calib(scores, kind, labels, 15, views=views, ignore_index=255, flags=1) for _ in range(2))
        assert np.array_equal(a, b) and a[45] > 0                             # bit-identical, the fp64 sums included
        none = run_calib(scores, kind, torch.full_like(labels, 255), 15, views=views, ignore_index=255)
        assert not none.any()
        beyond = run_calib(scores, kind, torch.full_like(labels, C), 15, views=views)       # labels >= ncls are never counted
        assert not beyond.any()


# ---------------------------------------------------------------------------------------------------------------- 4. the public path
def reference_maps(stub, views, batch, n_slices):
    """float64 (sums [N,C,H,W], view-entropy sum [N,H,W]) from the logits the stub itself returned, batch by batch and view by view."""
    nb = math.ceil(n_slices / batch)
    assert len(stub.outputs) == len(views) * nb
    sums, ves = [], []
    for b in range(nb):
        outs = stub.outputs[b * len(views):(b + 1) * len(views)]
        ms = [R.model(o, "logits") for o in outs]
        sums.append(sum(unview(m["p"], v).contiguous() for m, v in zip(ms, views)))
        ves.append(sum(unview(m["h"], v).contiguous() for m, v in zip(ms, views)))
    return torch.cat(sums), torch.cat(ves)


class _Pointwise(torch.nn.Module):
    """Logits that are a function of the pixel's value alone: every view agrees."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        c = torch.arange(9, device=x.device, dtype=torch.float32).view(1, 9, 1, 1)
        return (2.0 * torch.sin(3.0 * x + 0.7 * c) + 0.5 * x * c).contiguous()


@pytest.mark.parametrize("h,w,tta_name", [(5, 7, None), (5, 7, "flips"), (8, 8, "dihedral")], ids=["plain", "flips-5x7", "dihedral-8x8"])
def test_predict_uncertainty_through_a_stub(h, w, tta_name):
    from test_tta_gpu import _Stub, stub_slices
    from transception_amd._lib import _Lib
    from transception_amd.evaluate import TTA, Uncertainty, predict_probs, predict_slices, predict_uncertainty
    tta = None if tta_name is None else getattr(TTA, tta_name)()
    views = (0,) if tta is None else tta.views
    V, batch = len(views), 2
    slices = stub_slices(5, h, w)
    m = _Stub().to(DEV).train()
    before = _Lib.calls
    u = predict_uncertainty(m, slices, batch=batch, tta=tta)
    calls = _Lib.calls - before
    assert isinstance(u, Uncertainty) and m.training and m.modes == [False] * (V * 3)
    # the calls of predict_probs (a view and an accumulation per view and batch), one entropy launch per view with several, one final launch a batch
    assert calls == 2 * V * 3 + (V * 3 if V > 1 else 0) + 3
    sums, ves = reference_maps(m, views, batch, 5)
    ref = R.model(sums, "prob_sums", V)
    assert u.pred.dtype == torch.uint8 and all(t.shape == (5, h, w) for t in u if t is not None)
    bound_p = V * R.PER_VIEW / V + 2.0 ** -24
    assert float((u.confidence.cpu().double() - ref["conf"]).abs().max()) <= bound_p
    # the float64 model reads the float64 sums, the device its own fp32 accumulator: the entropy bound holds for the whole path
    dev_h = float((u.entropy.cpu().double() - ref["h"]).abs().max())
    print(f"predict_uncertainty {h}x{w} {tta_name}: max |h - model| {dev_h:.3e} (bound {R.ENTROPY_BOUND:.3e})")
    assert dev_h <= R.ENTROPY_BOUND
    at_pred = ref["p"].gather(1, u.pred.cpu().long().unsqueeze(1))[:, 0]
    assert bool((at_pred >= ref["conf"] - 2 * bound_p).all())
    if V == 1:
        assert u.mutual_information is None
    else:
        mi = (ref["h"] - ves / V).clamp(min=0.0)
        assert bool((u.mutual_information >= 0).all())
        dev_mi = float((u.mutual_information.cpu().double() - mi).abs().max())
        print(f"predict_uncertainty {h}x{w} {tta_name}: max |mi - model| {dev_mi:.3e}")
        assert dev_mi <= R.ENTROPY_BOUND
        assert float(u.mutual_information.max()) > 1e-3                       # the stub's views do disagree
    # pred is predict_slices' wherever the float64 sums tell the two best classes apart
    m2 = _Stub().to(DEV).eval()
    labels = predict_slices(m2, slices, batch=batch, tta=tta)
    clear = ref["gap"] > 2 * V * R.PER_VIEW
    assert bool(clear.any()) and torch.equal(u.pred.cpu()[clear], labels.cpu()[clear])
    # predict_probs is what it was: the same number of library calls as before this feature
    before = _Lib.calls
    predict_probs(_Stub().to(DEV), slices, batch=batch, tta=tta)
    assert _Lib.calls - before == 2 * V * 3


def test_predict_uncertainty_pointwise_views_agree_and_out_size():
    from transception_amd.evaluate import TTA, predict_probs, predict_uncertainty, resample_scores, uncertainty_maps
    g = torch.Generator().manual_seed(9)
    slices = torch.rand((3, 8, 8), generator=g).to(DEV)
    net = _Pointwise().to(DEV)
    one = predict_uncertainty(net, slices, batch=2)
    for tta in (TTA.flips(), TTA.dihedral()):
        u = predict_uncertainty(net, slices, batch=2, tta=tta)
        assert float(u.mutual_information.max()) <= 2 * R.ENTROPY_BOUND and bool((u.mutual_information >= 0).all())
        assert float((u.entropy - one.entropy).abs().max()) <= R.ENTROPY_BOUND
        assert float((u.confidence - one.confidence).abs().max()) <= 2 * R.PER_VIEW
    # out_size: the maps of the resampled accumulator and of the resampled view-entropy sum, the same final call
    from test_tta_gpu import _Stub
    tta = TTA.dihedral()
    stub = _Stub().to(DEV)
    u = predict_uncertainty(stub, slices, batch=2, tta=tta, out_size=(16, 16))
    assert all(t.shape == (3, 16, 16) for t in u)
    sums, ves = reference_maps(stub, tta.views, 2, 3)
    big = predict_probs(_Stub().to(DEV), slices, batch=2, tta=tta, out_size=(16, 16)) * 8      # the resampled accumulator (x / 8 * 8 is exact)
    ves_big = resample_scores(ves.float().unsqueeze(1).to(DEV), (16, 16), scores=True, pred=False)[0][:, 0]
    want = uncertainty_maps(big, kind="prob_sums", views=8, pred=True, view_entropy_sum=ves_big)
    assert torch.equal(u.pred, want.pred) and torch.equal(u.confidence, want.confidence)
    assert float((u.entropy - want.entropy).abs().max()) <= R.ENTROPY_BOUND
    dev_mi = float((u.mutual_information - want.mutual_information).abs().max())   # the device's view-entropy sum against the model's, resampled
    print(f"predict_uncertainty out_size: max |mi - mi from the model's view entropies| {dev_mi:.3e}")
    assert dev_mi <= R.ENTROPY_BOUND
    ref = R.model(big, "prob_sums", 8)
    assert float((u.entropy.cpu().double() - ref["h"]).abs().max()) <= R.ENTROPY_BOUND and bool((u.mutual_information >= 0).all())


def real_network(dtype):
    from transception_amd import MSTransception
    from transception_amd.seeded_init import seeded_state_dict
    net = MSTransception(num_classes=9)
    net.load_state_dict(seeded_state_dict(), strict=True)
    net.to(DEV)
    net.set_compute_dtype(dtype)
    return net


class _Recorded(torch.nn.Module):
    """The network with a tape: `replay()` makes the next passes return the logits of the recorded ones, in order, so that two entries see the
    same fp32 logits whether or not two forward passes of the network repeat to the bit."""

    def __init__(self, net):
        super().__init__()
        self.net, self.tape, self.pos = net, [], None

    def replay(self):
        self.pos = 0

    def forward(self, x):
        if self.pos is None:
            self.tape.append(self.net(x).detach().clone())
            return self.tape[-1].clone()
        self.pos += 1
        return self.tape[self.pos - 1].clone()


def small_volume(seed, d=3, n=64):
    g = np.random.default_rng(seed)
    lab = np.kron(g.integers(0, 9, (d, n // 8, n // 8)), np.ones((8, 8), np.int64)).astype(np.uint8)
    return (lab / 8).astype(np.float32), np.roll(lab, 1, axis=2)


@pytest.mark.parametrize("tta_name", [None, "flips"])
def test_volume_calibration_of_a_real_network(tta_name):
    """The seeded network at 64 x 64: the device's bin table and counts EQUAL `calibration_host` fed with `predict_probs` copied to the host --
    the same fp32 probabilities (x * 0.25 is x / 4) --; ECE, NLL and Brier are within the bounds; the pool of two volumes is the sum of their slots."""
    from transception_amd.evaluate import (TTA, Calibration, calibration_from_stats, calibration_host, evaluate_volume_calibration,
                                           inference_calibration, predict_probs)
    tta = None if tta_name is None else getattr(TTA, tta_name)()
    live = real_network(torch.float32).train()
    net = _Recorded(live).train()
    cal = Calibration(bins=10, foreground_only=True)
    vols = [small_volume(41) + ("a",), small_volume(42) + ("b",)]
    image, gt, _ = vols[0]
    got = evaluate_volume_calibration(net, image, gt, 9, (64, 64), batch=2, tta=tta, calibration=cal)
    assert net.training and got["n"] > 0 and got["stats"].dtype == np.float64
    net.replay()
    probs = predict_probs(net, torch.from_numpy(image).to(DEV), batch=2, tta=tta).cpu().numpy()
    assert net.pos == len(net.tape) == 2 * (1 if tta is None else 4)
    net = live
    host = calibration_host(probs, gt, cal)
    bins = cal.bins
    counts = np.ones(len(host["stats"]), bool)
    counts[3 * bins + 1:3 * bins + 3] = counts[3 * bins + 5::3] = False
    assert np.array_equal(got["stats"][counts], host["stats"][counts])      # the bin table, confidence sums included, and every count
    n = got["n"]
    assert np.abs(got["stats"][3 * bins + 5::3] - host["stats"][3 * bins + 5::3]).max() <= n * (R.ENTROPY_BOUND + FIXED)
    assert got["ece"] == host["ece"] and got["mce"] == host["mce"] and got["accuracy"] == host["accuracy"]
    print(f"volume calibration {tta_name}: n {n}, ece {got['ece']:.4f}, |nll - host| {abs(got['nll'] - host['nll']):.3e}, "
          f"|brier - host| {abs(got['brier'] - host['brier']):.3e}")
    assert abs(got["nll"] - host["nll"]) <= R.sums_bound(1, 9) and abs(got["brier"] - host["brier"]) <= R.sums_bound(1, 9)
    # a resized volume: labels by the order-0 rule, scores at the network size
    big = evaluate_volume_calibration(net, np.kron(image, np.ones((2, 2), np.float32)), np.kron(gt, np.ones((2, 2), np.uint8)), 9, (64, 64), batch=2,
                                      calibration=Calibration(bins=10))
    assert big["n"] == 3 * 64 * 64
    lines = []
    pool = inference_calibration(net, vols, 9, 64, batch=2, log=lines.append, tta=tta, calibration=cal)
    assert [c["name"] for c in pool["cases"]] == ["a", "b"] and pool["cases"][0]["n"] == got["n"]
    total = pool["cases"][0]["stats"] + pool["cases"][1]["stats"]
    want = calibration_from_stats(total, bins, 9)
    assert np.array_equal(pool["overall"]["stats"], total) and {k: v for k, v in pool["overall"].items() if k != "stats"} == want
    assert len(lines) == 3 and "case a calibration ece" in lines[0] and lines[2].startswith("Calibration over 2 cases: ece")


def test_trainer_fills_hist_calibration(tmp_path, monkeypatch):
    from transception_amd import data as D
    from transception_amd import trainer as T
    from transception_amd._lib import _Lib
    from transception_amd.evaluate import Calibration
    L, seen, calls = lib(), [], {}
    for name in ("tc_uncert_maps", "tc_calib_stats"):
        monkeypatch.setattr(L, name, (lambda real, name: lambda *a: (seen.append(name), real(*a))[1])(getattr(L, name), name))

    def counting(real, key):                                                  # the library calls made inside one entry of the evaluation
        def run(*a, **kw):
            before = _Lib.calls
            out = real(*a, **kw)
            calls.setdefault(key, []).append(_Lib.calls - before)
            return out
        return run

    monkeypatch.setattr(T, "inference", counting(T.inference, "inference"))
    monkeypatch.setattr(T, "inference_calibration", counting(T.inference_calibration, "calibration"))
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=1, slices_per_case=4, size=64, seed=2)
    g = np.random.default_rng(0)
    vol = (g.random((3, 96, 96)).astype(np.float32), (g.random((3, 96, 96)) * 3).astype(np.uint8), "case0")
    hists, launches, totals, evals = {}, {}, {}, {}
    for name, option in (("without", dict()), ("with", dict(calibration=Calibration(bins=10)))):
        net = real_network(torch.bfloat16)
        net.train()
        cfg = T.TrainConfig(root_path=base, list_dir=lists, max_epochs=1, batch_size=2, img_size=64, seed=5, model_name="tiny",
                            device_metrics=True, **option)
        del seen[:]
        calls.clear()
        before = _Lib.calls
        hists[name] = T.trainer_synapse(cfg, net, str(tmp_path / ("snap_" + name)), volumes=lambda: [vol], log=lambda s: None)
        launches[name], totals[name], evals[name] = list(seen), _Lib.calls - before, dict(calls)
    hist = hists["with"]
    assert "calibration" not in hists["without"] and set(hist) == set(hists["without"]) | {"calibration"} and launches["without"] == []
    assert launches["with"] and set(launches["with"]) == {"tc_calib_stats"}
    # the library calls of an evaluation are what they were: the same inside `inference`, and the whole run differs by the calibration pass alone
    assert evals["without"] == {"inference": evals["with"]["inference"]} and len(evals["with"]["inference"]) == 1 and evals["with"]["inference"][0] > 0
    assert len(evals["with"]["calibration"]) == 1 and totals["with"] == totals["without"] + evals["with"]["calibration"][0]
    assert len(hist["calibration"]) == len(hist["dice"]) == 1
    c = hist["calibration"][0]
    assert c["n"] == 3 * 64 * 64 and len(c["bins"]) == 10 and len(c["classes"]) == 9 and sum(b["count"] for b in c["bins"]) == c["n"]
    assert 0.0 <= c["ece"] <= c["mce"] <= 1.0 and c["nll"] > 0 and 0.0 < c["brier"] <= 2.0 and all(math.isfinite(c[k]) for k in ("ece", "nll", "brier"))

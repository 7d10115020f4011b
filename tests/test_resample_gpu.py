"""Class scores resampled to another size and their argmax on the device (csrc/resample.hip: tc_resample_scores; evaluate.resample_scores,
predict_slices / predict_probs with `out_size`, evaluate_volume / inference / TrainConfig with `resample`) against the float64 reference of
tests/resample_ref.py, which tests/test_resample_host.py holds to torch.nn.functional.interpolate.

Exact: on inputs that are multiples of 1/8 in [-8, 8] and ratios whose weights are multiples of 1/32 every product and sum of the definition
is an fp32 number, so the scores EQUAL the reference and the labels its argmax, ties included.

Bounded: on seeded normals |scores - ref| <= 16 x 2^-24 x max|v| at every element.  The value is two levels of lerps of values <= max|v|:
each level is a multiply-add pair with at most two roundings per output of that level (contracted or not), three lerps, so at most eight
roundings of half an ulp of a value <= max|v| (8 x 2^-24 max|v|); the weights 1 - l carry one rounding of their own and l the one of its
division, which doubles it.  Labels are held at EVERY pixel to ref[label] >= max ref - 2 x that bound: a label the float64 scores cannot
tell from their maximum within the error of two values.

Measured on the MI355X: worst |scores - ref| on the normals 1.62 x 2^-24 max|v| (bound 16), 0 at the identity shapes; worst |mean - ref| of
predict_probs with `out_size` 2.7e-7 (bound 3.0e-6)."""
import math

import numpy as np
import pytest
import torch

from resample_ref import labels as ref_labels, resample
from tta_ref import sum_probs

pytestmark = pytest.mark.gpu

from transception_amd import _lib  # noqa: E402
from transception_amd._lib import lib  # noqa: E402

DEV = "cuda:0"
#          N  C   h    w     H    W
SHAPES = [(2, 9, 7, 7, 16, 16),           # the workload's ratio 7/16, below a tile
          (1, 2, 3, 130, 6, 260),         # rows wider than a 128-column tile
          (3, 16, 33, 33, 132, 132),      # one past a tile edge; 16 classes; element-wise staging (33 is no multiple of a piece)
          (2, 9, 64, 64, 128, 256),       # different ratios per axis
          (1, 9, 5, 7, 7, 5),             # one axis grows, one shrinks
          (2, 9, 9, 5, 13, 300),
          (1, 1, 12, 12, 5, 7),           # shrink, one class
          (1, 9, 32, 32, 32, 32),         # identity
          (1, 9, 224, 224, 512, 512),     # the workload
          (1, 9, 12, 160, 12, 160),       # identity whose footprint (10 x 136 words a class) is staged in two chunks of classes
          (1, 3, 40, 1200, 3, 5)]         # strong shrink: the footprint of a tile exceeds the staging budget, taps are read unstaged
EXACT = [s for s in SHAPES if s[2:] in ((7, 7, 16, 16), (3, 130, 6, 260), (33, 33, 132, 132), (64, 64, 128, 256), (32, 32, 32, 32),
                                         (224, 224, 512, 512), (12, 160, 12, 160))]
DTYPES = [(torch.float32, _lib.TC_F32), (torch.bfloat16, _lib.TC_BF16), (torch.float16, _lib.TC_F16)]
ULPS = 16.0
GUARD = 1024                               # elements of sentinel in front of and behind every output
S_SENT, P_SENT = -1234.5, 255


def ids(vals):
    return ["x".join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else str(v[0]).replace("torch.", "") for v in vals]


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def launch(src, tc, size, want_scores=True, want_pred=True):
    """The entry on `src` (device, contiguous) with the outputs inside sentinel-filled buffers; checks the guard regions and returns
    (scores or None, pred or None)."""
    N, C, h, w = src.shape
    H, W = size
    sbuf = torch.full((N * C * H * W + 2 * GUARD,), S_SENT, dtype=torch.float32, device=DEV)
    pbuf = torch.full((N * H * W + 2 * GUARD,), P_SENT, dtype=torch.uint8, device=DEV)
    scores, pred = sbuf[GUARD:-GUARD].view(N, C, H, W), pbuf[GUARD:-GUARD].view(N, H, W)
    lib().tc_resample_scores(src.data_ptr(), tc, scores.data_ptr() if want_scores else None, pred.data_ptr() if want_pred else None,
                             N, C, h, w, H, W, stream())
    for buf, sent in ((sbuf, S_SENT), (pbuf, P_SENT)):
        assert bool((buf[:GUARD] == sent).all()) and bool((buf[-GUARD:] == sent).all())
    if not want_scores:
        assert bool((sbuf == S_SENT).all())
    if not want_pred:
        assert bool((pbuf == P_SENT).all())
    return (scores if want_scores else None), (pred if want_pred else None)


_CASES = {}


def case(shape, dt, kind):
    """(host input in dt, float64 reference): built once per case and never changed."""
    key = (shape, dt, kind)
    if key not in _CASES:
        N, C, h, w, H, W = shape
        g = torch.Generator().manual_seed(100 + SHAPES.index(shape))
        if kind == "normal":
            v = torch.randn((N, C, h, w), generator=g)
        else:
            v = torch.randint(-64, 65, (N, C, h, w), generator=g).float() / 8
            v[..., : max(h // 2, 1), : max(w // 3, 1)] = 0.625                     # a region constant over position AND class: label 0
            if C > 1:
                v[:, C - 1] = v[:, 0]                                                # two equal classes everywhere: the lower one wins
            if C > 2:
                v[:, 1, h // 2:] = 8.0
                v[:, 2, h // 2:] = 8.0                                                # two equal classes at the top of the range: label 1
        v = v.to(dt)
        _CASES[key] = (v, resample(v, (H, W)))
    return _CASES[key]


def bound(v):
    return ULPS * 2.0 ** -24 * float(v.float().abs().max())


def label_criterion(pred, ref, tol):
    chosen = ref.gather(1, pred.cpu().long().unsqueeze(1))[:, 0]
    slack = float((ref.max(dim=1).values - chosen).max())
    assert slack <= 2 * tol, slack


# ---------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("dt,tc", DTYPES, ids=ids(DTYPES))
@pytest.mark.parametrize("shape", EXACT, ids=ids(EXACT))
def test_exact_on_eighths(shape, dt, tc):
    v, ref = case(shape, dt, "eighths")
    assert torch.equal(v.float().double(), (v.float() * 8).round().double() / 8) and float(v.float().abs().max()) <= 8
    scores, pred = launch(v.to(DEV).contiguous(), tc, shape[4:])
    assert torch.equal(scores.cpu().double(), ref)
    want = ref_labels(ref)
    assert torch.equal(pred.cpu(), want)
    if shape[1] > 1:
        assert not bool((want == shape[1] - 1).any())                                 # the copy of class 0 never wins
        assert bool((want == 0).any())


# ---------------------------------------------------------------------------------------------------------------- 2. bounded
@pytest.mark.parametrize("dt,tc", DTYPES, ids=ids(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_normals_within_the_bound(shape, dt, tc):
    v, ref = case(shape, dt, "normal")
    scores, pred = launch(v.to(DEV).contiguous(), tc, shape[4:])
    err = float((scores.cpu().double() - ref).abs().max())
    print(f"resample {shape} {dt}: max |scores - ref| = {err / (2.0 ** -24 * float(v.float().abs().max())):.2f} x 2^-24 max|v| (bound {ULPS:g})")
    assert err <= bound(v)
    label_criterion(pred, ref, bound(v))


# ---------------------------------------------------------------------------------------------------------------- 3. identity
@pytest.mark.parametrize("dt,tc", DTYPES, ids=ids(DTYPES))
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2:4] == s[4:]], ids=ids([s for s in SHAPES if s[2:4] == s[4:]]))
def test_identity_is_the_input(shape, dt, tc):
    from transception_amd.evaluate import argmax_counts
    v, _ = case(shape, dt, "normal")
    vd = v.to(DEV).contiguous()
    scores, pred = launch(vd, tc, shape[4:])
    assert torch.equal(scores.view(torch.int32), vd.float().view(torch.int32))      # bit for bit
    assert torch.equal(pred, argmax_counts(vd.float())[0])


# ---------------------------------------------------------------------------------------------------------------- 4. independent, in bounds
@pytest.mark.parametrize("dt,tc", DTYPES, ids=ids(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_outputs_are_independent_and_any_base_will_do(shape, dt, tc):
    v, _ = case(shape, dt, "normal")
    vd = v.to(DEV).contiguous()
    scores, pred = launch(vd, tc, shape[4:])
    only_p = launch(vd, tc, shape[4:], want_scores=False)[1]
    only_s = launch(vd, tc, shape[4:], want_pred=False)[0]
    assert torch.equal(only_p, pred) and torch.equal(only_s.view(torch.int32), scores.view(torch.int32))
    assert torch.equal(vd.cpu().view(torch.int16 if dt != torch.float32 else torch.int32), v.view(torch.int16 if dt != torch.float32 else torch.int32))
    # the same input one element further on: no 16-byte aligned row
    buf = torch.zeros(v.numel() + 9, dtype=dt, device=DEV)
    off = buf[1:1 + v.numel()].view(v.shape)
    off.copy_(vd)
    assert off.data_ptr() % 16 != 0
    s2, p2 = launch(off, tc, shape[4:])
    assert torch.equal(p2, pred) and torch.equal(s2.view(torch.int32), scores.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 5. run to run
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[8]], ids=ids([SHAPES[2], SHAPES[8]]))
def test_run_to_run_identity(shape):
    v, _ = case(shape, torch.bfloat16, "normal")
    vd = v.to(DEV).contiguous()
    a, b = launch(vd, _lib.TC_BF16, shape[4:]), launch(vd, _lib.TC_BF16, shape[4:])
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert bool(torch.isfinite(a[0]).all())


# ---------------------------------------------------------------------------------------------------------------- 6. through the API
PER_VIEW = 2e-6                             # tc_tta_accumulate's bound per view (tests/test_tta_gpu.py)


class _Stub(torch.nn.Module):
    """Logits that depend on the intensity and on the absolute position (the stub of tests/test_tta_gpu.py); records inputs and outputs."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self.inputs, self.outputs, self.modes = [], [], []

    def forward(self, x):
        _, _, h, w = x.shape
        k = torch.round((x[:, 0] * 0.5 + 0.5) * 8).long().clamp(0, 8)
        hot = torch.nn.functional.one_hot(k, 9).permute(0, 3, 1, 2).float()
        c = torch.arange(9, device=x.device, dtype=torch.float32).view(1, 9, 1, 1)
        r = torch.arange(h, device=x.device, dtype=torch.float32).view(1, 1, h, 1)
        q = torch.arange(w, device=x.device, dtype=torch.float32).view(1, 1, 1, w)
        out = (6.0 * hot + 2.5 * torch.sin(0.9 * c + 0.21 * r) + 2.5 * torch.cos(1.3 * c - 0.17 * q)).contiguous()
        self.inputs.append(x.detach().clone())
        self.outputs.append(out.detach().clone())
        self.modes.append(self.training)
        return out


class _Recorder(torch.nn.Module):
    def __init__(self, model):
        super().__init__()
        self.model = model
        self.inputs, self.outputs = [], []

    def forward(self, x):
        out = self.model(x)
        self.inputs.append(x.detach().clone())
        self.outputs.append(out.detach().clone())
        return out


def recorded_scores(outputs, nviews, size):
    """(float64 reference at `size`, its error bound) from the logits a recording model returned: per batch the logits themselves (nviews
    None: no TTA) or the float64 sum of the softmax of its views (flip views un-flipped by tests/tta_ref.py), resampled by the reference."""
    if nviews is None:
        full = torch.cat([resample(o, size) for o in outputs])
        return full, ULPS * 2.0 ** -24 * max(float(o.float().abs().max()) for o in outputs)
    assert len(outputs) % nviews == 0
    sums = [sum_probs(list(range(nviews)), outputs[b:b + nviews]) for b in range(0, len(outputs), nviews)]
    # the accumulator is within PER_VIEW x views of the sums, a convex combination of it is too; then the resampling of values <= views
    return torch.cat([resample(s, size) for s in sums]), PER_VIEW * nviews + ULPS * 2.0 ** -24 * nviews


def stub_slices(n, h, w, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 9, (n, h, w), generator=g).float() / 8).to(DEV)


@pytest.mark.parametrize("h,w,size", [(64, 64, (128, 128)), (32, 64, (75, 100))], ids=["64-128", "32x64-75x100"])
@pytest.mark.parametrize("flips", [False, True], ids=["plain", "flips"])
def test_predict_with_out_size_through_a_stub(h, w, size, flips):
    from transception_amd.evaluate import TTA, predict_probs, predict_slices
    slices, batch = stub_slices(5, h, w), 2
    tta, nv = (TTA.flips(), 4) if flips else (None, None)
    m = _Stub().to(DEV).train()
    got = predict_slices(m, slices, batch=batch, tta=tta, out_size=size)
    assert m.training and m.modes == [False] * ((nv or 1) * 3)
    assert got.shape == (5,) + size and got.dtype == torch.uint8
    for b in range(3):                                                                # what the model was given is what it is given without out_size
        want = ((slices[2 * b:2 * b + 2].float() - 0.5) / 0.5)
        assert torch.equal(m.inputs[b * (nv or 1)][:, 0], want)
    ref, tol = recorded_scores(m.outputs, nv, size)
    label_criterion(got, ref, tol)
    assert len(torch.unique(got)) > 3
    # out_size equal to the slices' size, or None: the calls without it, to the bit
    m2 = _Stub().to(DEV).eval()
    assert torch.equal(predict_slices(m2, slices, batch=batch, tta=tta, out_size=(h, w)), predict_slices(m2, slices, batch=batch, tta=tta))
    assert torch.equal(predict_slices(m2, slices, batch=batch, tta=tta, out_size=None), predict_slices(m2, slices, batch=batch, tta=tta))
    # the probabilities: the sums of the views resampled, over their number (without tta: the softmax of the one pass)
    m3 = _Stub().to(DEV).eval()
    probs = predict_probs(m3, slices, batch=batch, tta=tta, out_size=size)
    assert probs.shape == (5, 9) + size and probs.dtype == torch.float32
    pref, ptol = recorded_scores(m3.outputs, nv or 1, size)
    err = float((probs.cpu().double() - pref / (nv or 1)).abs().max())
    print(f"predict_probs {h}x{w} -> {size} views {nv}: max |mean - ref| = {err:.3e} (bound {ptol / (nv or 1) + 2.0 ** -24:.3e})")
    assert err <= ptol / (nv or 1) + 2.0 ** -24
    assert torch.equal(predict_probs(m3, slices, batch=batch, tta=tta, out_size=(h, w)), predict_probs(m3, slices, batch=batch, tta=tta))


def count_entry(monkeypatch):
    """[number of tc_resample_scores calls], counted on the loaded library object"""
    L, n = lib(), [0]
    real = L.tc_resample_scores

    def counted(*a):
        n[0] += 1
        return real(*a)

    monkeypatch.setattr(L, "tc_resample_scores", counted)
    return n


def finish(pred, gt, classes, kw):
    """evaluate_volume's steps after the prediction at the label's size (uint8, on the device), from the existing pieces."""
    from transception_amd.evaluate import calculate_metric_percase, dice_from_counts, metrics_device, postprocess_device, surfaces_counts
    pred = pred.clone()
    if kw.get("postprocess") is not None:
        pred = postprocess_device(pred, classes, kw["postprocess"])
    if kw.get("device_metrics"):
        label_t = torch.from_numpy(np.ascontiguousarray(gt)).to(DEV)
        if kw.get("with_hd95"):
            return metrics_device(pred, label_t, classes, kw.get("voxelspacing"))
        return dice_from_counts(surfaces_counts(pred, label_t, classes)[2].cpu().numpy())
    p = pred.cpu().numpy()
    if kw.get("with_hd95"):
        return [calculate_metric_percase(p == k, gt == k, kw.get("voxelspacing")) for k in range(1, classes)]
    counts = np.zeros((classes, 3))
    for k in range(classes):
        counts[k] = (np.logical_and(p == k, gt == k).sum(), (p == k).sum(), (gt == k).sum())
    return dice_from_counts(counts)


def volume(seed=21, d=3, n=128):
    """A blocky image of levels k / 8 (blocks of 8 pixels survive the zoom to half the size) and labels derived from it, shifted by a pixel."""
    g = np.random.default_rng(seed)
    coarse = g.integers(0, 9, (d, n // 8, n // 8))
    lab = np.kron(coarse, np.ones((8, 8), np.int64)).astype(np.uint8)
    return (lab / 8).astype(np.float32), np.roll(lab, 1, axis=2)


def real_network(dtype):
    from transception_amd import MSTransception
    from transception_amd.seeded_init import seeded_state_dict
    net = MSTransception(num_classes=9)
    net.load_state_dict(seeded_state_dict(), strict=True)
    net.to(DEV)
    net.set_compute_dtype(dtype)
    return net


@pytest.mark.parametrize("which", ["stub", "network"])
def test_evaluate_volume_and_inference_with_scores(which, monkeypatch):
    """resample="scores" on a 3 x 128 x 128 volume at network size 64: the labels at 128 x 128 are held to the reference applied to the
    logits the model returned, and every variant of evaluate_volume / inference equals the existing pieces applied to those labels."""
    from transception_amd.evaluate import (TTA, PostProcess, evaluate_volume, inference, predict_slices, zoom_labels, zoom_volume_to_network)
    image, gt = volume()
    m = (_Stub().to(DEV) if which == "stub" else _Recorder(real_network(torch.float32))).train()
    calls = count_entry(monkeypatch)
    sl = zoom_volume_to_network(torch.from_numpy(image).to(DEV), (64, 64))
    post = PostProcess("min_voxels", 5)
    kws = (dict(), dict(with_hd95=True), dict(device_metrics=True), dict(device_metrics=True, with_hd95=True),
           dict(with_hd95=True, postprocess=post), dict(device_metrics=True, with_hd95=True, postprocess=post, voxelspacing=(2.5, 0.8, 0.8)))
    for tta, nv in ((None, None), (TTA.flips(), 4)):
        del m.outputs[:], m.inputs[:]
        calls[0] = 0
        pred = predict_slices(m, sl, batch=2, tta=tta, out_size=(128, 128))
        assert m.training and len(m.outputs) == 2 * (nv or 1) and calls[0] == 2
        ref, tol = recorded_scores([o if o.dtype in (torch.float32, torch.bfloat16, torch.float16) else o.float() for o in m.outputs], nv, (128, 128))
        label_criterion(pred, ref, tol)
        blocky = zoom_labels(predict_slices(m, sl, batch=2, tta=tta), (128, 128))
        assert pred.shape == blocky.shape
        if which == "stub":
            assert not torch.equal(pred, blocky)                                      # the two ways differ along the boundaries
        for kw in (kws if which == "stub" else kws[-2:]):                             # the network: both metric paths, with a PostProcess
            calls[0] = 0
            got = evaluate_volume(m, image, gt, 9, (64, 64), batch=2, tta=tta, resample="scores", **kw)
            assert calls[0] == 2 and m.training, kw
            assert got == finish(pred, gt, 9, kw), kw
            # "labels", and no argument at all: today's calls, to the bit, and not one call of the new entry
            calls[0] = 0
            today = finish(blocky, gt, 9, kw)
            assert evaluate_volume(m, image, gt, 9, (64, 64), batch=2, tta=tta, resample="labels", **kw) == today, kw
            assert evaluate_volume(m, image, gt, 9, (64, 64), batch=2, tta=tta, **kw) == today, kw
            assert calls[0] == 0
        for dm in (False, True):
            calls[0] = 0
            vols = [(image, gt, "a"), (image[:2], gt[:2], "b")]
            got = inference(m, vols, 9, 64, batch=2, device_metrics=dm, tta=tta, resample="scores")
            assert calls[0] == 3
            a, b = (np.array(finish(p, g, 9, dict(with_hd95=True, device_metrics=dm))) for p, g in ((pred, gt), (pred[:2], gt[:2])))
            mean = (a + b) / 2
            assert got == (float(mean.mean(axis=0)[0]), float(mean.mean(axis=0)[1]))
            if which == "stub":
                assert inference(m, vols, 9, 64, batch=2, device_metrics=dm, tta=tta, resample="labels") == \
                    inference(m, vols, 9, 64, batch=2, device_metrics=dm, tta=tta)
    # without a resize both values run the same calls
    small, small_gt = image[:, :64, :64], gt[:, :64, :64]
    calls[0] = 0
    assert evaluate_volume(m, small, small_gt, 9, (64, 64), batch=2, with_hd95=True, resample="scores") == \
        evaluate_volume(m, small, small_gt, 9, (64, 64), batch=2, with_hd95=True)
    assert calls[0] == 0
    with pytest.raises(ValueError, match="host_zoom"):
        evaluate_volume(m, image, gt, 9, (64, 64), host_zoom=True, resample="scores")


def test_logits_keep_their_dtype():
    """A model that returns bfloat16 logits: they reach the entry as they are (the reference widens the same 16-bit values)."""
    from transception_amd.evaluate import predict_slices

    class Half(_Stub):
        def forward(self, x):
            out = super().forward(x).to(torch.bfloat16)
            self.outputs[-1] = out.detach().clone()
            return out

    m = Half().to(DEV).eval()
    pred = predict_slices(m, stub_slices(3, 32, 32), batch=2, out_size=(80, 72))
    assert all(o.dtype == torch.bfloat16 for o in m.outputs)
    ref, tol = recorded_scores(m.outputs, None, (80, 72))
    label_criterion(pred, ref, tol)


# ---------------------------------------------------------------------------------------------------------------- 7. the trainer
def test_trainer_hands_resample_to_inference(tmp_path, monkeypatch):
    """TrainConfig.resample reaches the evaluation after the last epoch: `inference` is called with it, and a 96 x 96 volume at network size
    64 goes through the new entry once (one batch of three slices)."""
    from transception_amd import trainer as T
    from transception_amd import data as D
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=1, slices_per_case=4, size=64, seed=2)
    net = real_network(torch.bfloat16)
    net.train()
    cfg = T.TrainConfig(root_path=base, list_dir=lists, max_epochs=1, batch_size=2, img_size=64, seed=5, model_name="tiny", resample="scores")
    seen = []
    real = T.inference

    def spy(model, vols, *a, **kw):
        seen.append(kw.get("resample"))
        return real(model, vols, *a, **kw)

    monkeypatch.setattr(T, "inference", spy)
    calls = count_entry(monkeypatch)
    g = np.random.default_rng(0)
    vol = (g.random((3, 96, 96)).astype(np.float32), (g.random((3, 96, 96)) * 3).astype(np.uint8), "case0")
    hist = T.trainer_synapse(cfg, net, str(tmp_path / "snap"), volumes=lambda: [vol], log=lambda s: None)
    assert seen == ["scores"] and calls[0] == 1
    assert net.training and len(hist["dice"]) == 1 and 0.0 <= hist["dice"][0] <= 1.0 and math.isfinite(hist["hd95"][0])
    # the default configuration asks for "labels"
    assert T.TrainConfig(root_path=base, list_dir=lists).resample == "labels"

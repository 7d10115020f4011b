"""Test-time augmentation on the device (csrc/tta.hip: tc_tta_view, tc_tta_accumulate; evaluate.TTA, predict_slices, predict_probs,
evaluate_volume, inference) against the float64 reference of tests/tta_ref.py.

The view kernel and the geometry of the accumulation are equalities: with logits 0 at one class and -200 elsewhere every probability is
0 or 1 exactly (tests/test_tta_host.py checks the number facts), so the accumulator after any sequence of views holds integer counts.
On seeded normals the bound is 2e-6 per view at every element: p <= 1; at most 16 exponentials of 1-2 ulp, one division, and one running
add of a value <= 8 make <= 24 x 2^-24 = 1.4e-6 per view (a float32 emulation on the CPU stays below 1e-6 for all eight views together,
tests/test_tta_host.py).  Labels are held at EVERY pixel to ref[label] >= max ref - 2 x that bound: a label the float64 sums cannot
tell from their maximum within the accumulated error.  The mean of predict_probs is the accumulator over the number of views: the bound
over the number of views, plus half an ulp of a value <= 1 for the division.

Measured on the MI355X: worst |acc - ref| on the normals 7.4e-7 over eight views (bound 1.6e-5) and 3.8e-7 over four (bound 8e-6); worst
|mean - ref| of predict_probs 3.4e-7 with the stub, 3.7e-8 with the real network (bound 2.06e-6)."""
import math

import numpy as np
import pytest
import torch

from tta_ref import sum_probs, unview, view

pytestmark = pytest.mark.gpu

from transception_amd import _lib  # noqa: E402
from transception_amd._lib import lib  # noqa: E402

DEV = "cuda:0"
SHAPES = [(2, 9, 5, 7),           # odd, non-square, below a tile
          (1, 2, 3, 130),         # wider than 64, not a multiple of it
          (3, 16, 33, 33),        # square, one past a 32-tile edge, 16 classes (the transposed tile takes more than 64 KiB of LDS)
          (2, 9, 64, 64),         # network-like: 4 columns a thread
          (1, 1, 4, 4)]
DTYPES = [(torch.float32, _lib.TC_F32), (torch.bfloat16, _lib.TC_BF16), (torch.float16, _lib.TC_F16)]
PER_VIEW = 2e-6
SENTINEL = -1234.5


def ids(vals):
    return ["x".join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else str(v[0]).replace("torch.", "") for v in vals]


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def views_of(H, W):
    return list(range(8 if H == W else 4))


def view_shape(N, C, H, W, v):
    return (N, C, W, H) if v & 4 else (N, C, H, W)


def accumulate(lg, tc, acc, pred, shape, v, first):
    N, C, H, W = shape
    assert lg.is_contiguous() and lg.shape == view_shape(N, C, H, W, v)
    lib().tc_tta_accumulate(lg.data_ptr(), tc, None if acc is None else acc.data_ptr(), None if pred is None else pred.data_ptr(), N, C, H, W,
                            v, int(first), stream())


def label_criterion(pred, ref, nviews):
    """ref: float64 sums [N,C,H,W]; at every pixel the chosen class is within 2 x the bound of the largest sum."""
    chosen = ref.gather(1, pred.cpu().long().unsqueeze(1))[:, 0]
    slack = ref.max(dim=1).values - chosen
    assert float(slack.max()) <= 2 * PER_VIEW * nviews, float(slack.max())


# ---------------------------------------------------------------------------------------------------------------- 1. the view kernel
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_view_kernel_equals_torch(shape):
    N, _, H, W = shape
    x = torch.rand((N, H, W), generator=torch.Generator().manual_seed(1), dtype=torch.float32)
    xd = x.to(DEV)
    want = (x - 0.5) / 0.5
    for v in views_of(H, W):
        dst = torch.full((N, W, H) if v & 4 else (N, H, W), float("nan"), dtype=torch.float32, device=DEV)
        lib().tc_tta_view(xd.data_ptr(), dst.data_ptr(), N, H, W, v, 0.5, 0.5, stream())
        assert torch.equal(dst.cpu(), view(want, v).contiguous()), v
        assert torch.equal(dst, view((xd - 0.5) / 0.5, v).contiguous()), v            # and the device's own expression
    assert torch.equal(xd.cpu(), x)


# ---------------------------------------------------------------------------------------------------------------- 2. geometry, exact
def one_hot_logits(shape, v, seed, dt):
    """(codes of the view [N,h,w], logits in dt on the device: 0 at class code(n,y,x), -200 elsewhere)."""
    N, C, H, W = shape
    code = torch.randint(0, C, view_shape(N, 1, H, W, v)[:1] + view_shape(N, 1, H, W, v)[2:], generator=torch.Generator().manual_seed(seed))
    lg = torch.full(view_shape(N, C, H, W, v), -200.0)
    lg.scatter_(1, code.unsqueeze(1), 0.0)
    return code, lg.to(dt).to(DEV).contiguous()


@pytest.mark.parametrize("dt,tc", DTYPES, ids=ids(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_geometry_is_exact(shape, dt, tc):
    N, C, H, W = shape
    order = views_of(H, W)
    order = order[3:] + order[:3]                                                    # not the natural order: 3, (4 .. 7,) 0, 1, 2
    counts = torch.zeros(shape, dtype=torch.float64)
    acc = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)           # first = 1 overwrites, never reads
    for j, v in enumerate(order):
        code, lg = one_hot_logits(shape, v, 100 + v, dt)
        counts = counts + unview(torch.nn.functional.one_hot(code, C).permute(0, 3, 1, 2).double(), v)
        if j == len(order) - 1:
            # the last view as labels: the accumulator keeps the counts of the views before it
            before = acc.clone()
            pred = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
            accumulate(lg, tc, acc, pred, shape, v, first=0)
            assert torch.equal(acc, before)
            assert torch.equal(pred.cpu().long(), counts.argmax(dim=1)), v            # integer counts: first maximum, as torch.argmax
        accumulate(lg, tc, acc, None, shape, v, first=(j == 0))
        assert torch.equal(acc.cpu().double(), counts), (j, v)
    assert float(counts.sum()) == len(order) * N * H * W
    # first = 1 with labels: a sentinel-filled accumulator is neither read nor written, and NULL will do
    v = order[0]
    code, lg = one_hot_logits(shape, v, 100 + v, dt)
    want = unview(code, v)
    sent = torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)
    for a in (sent, None):
        pred = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
        accumulate(lg, tc, a, pred, shape, v, first=1)
        assert torch.equal(pred.cpu().long(), want)
    assert bool((sent == SENTINEL).all())


@pytest.mark.parametrize("shape", [(1, 2, 2080, 2080), (1, 2, 1029, 1029)], ids=["2080", "1029"])
def test_geometry_beyond_one_pass(shape):
    """Maps larger than one trip of the kernels' loops: 2080^2 is 4225 tiles (the transposed kernels' grid holds 4096) and 1,081,600 groups of 4
    columns, 1029^2 is 1,058,841 single columns (the flip kernels' grid holds 2048 x 256 threads).  Exact, as above."""
    N, C, H, W = shape
    x = torch.rand((N, H, W), generator=torch.Generator().manual_seed(2)).to(DEV)
    want = (x - 0.5) / 0.5
    counts = torch.zeros(shape, dtype=torch.float32)
    acc = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    pred = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
    order = (3, 7, 0, 4)
    for j, v in enumerate(order):
        dst = torch.full((N, W, H) if v & 4 else (N, H, W), float("nan"), dtype=torch.float32, device=DEV)
        lib().tc_tta_view(x.data_ptr(), dst.data_ptr(), N, H, W, v, 0.5, 0.5, stream())
        assert torch.equal(dst, view(want, v).contiguous()), v
        code, lg = one_hot_logits(shape, v, 200 + v, torch.bfloat16)
        counts += unview(torch.nn.functional.one_hot(code, C).permute(0, 3, 1, 2).float(), v)
        if j >= 2:                                                                   # labels from a flip view and from a transposed one
            accumulate(lg, _lib.TC_BF16, acc, pred, shape, v, first=0)
            assert torch.equal(pred.cpu().long(), counts.argmax(dim=1)), v
        accumulate(lg, _lib.TC_BF16, acc, None, shape, v, first=(j == 0))
        assert torch.equal(acc.cpu(), counts), (j, v)


# ---------------------------------------------------------------------------------------------------------------- 3. numerics
_NORMALS = {}


def normal_logits(shape, dt, scale):
    """Per view: randn x scale rounded to dt, on the host (built once per case and never changed)."""
    key = (shape, dt, scale)
    if key not in _NORMALS:
        N, C, H, W = shape
        g = torch.Generator().manual_seed(1000 + 7 * SHAPES.index(shape) + int(scale))
        _NORMALS[key] = [(torch.randn(view_shape(N, C, H, W, v), generator=g) * scale).to(dt) for v in views_of(H, W)]
    return _NORMALS[key]


@pytest.mark.parametrize("dt,tc", DTYPES, ids=ids(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=ids(SHAPES))
def test_numerics_within_the_bound(shape, dt, tc):
    N, C, H, W = shape
    views = views_of(H, W)
    for scale in (1.0, 4.0, 12.0):
        host = normal_logits(shape, dt, scale)
        ref = sum_probs(views, host)                                                  # float64, of the same rounded values
        acc = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
        pred = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
        for j, v in enumerate(views):
            lg = host[j].to(DEV).contiguous()
            if j == len(views) - 1:
                accumulate(lg, tc, acc if j else None, pred, shape, v, first=(j == 0))
            accumulate(lg, tc, acc, None, shape, v, first=(j == 0))
        err = float((acc.cpu().double() - ref).abs().max())
        print(f"tta numerics {shape} {dt} x{scale:g}: max |acc - ref| = {err:.3e} over {len(views)} views (bound {PER_VIEW * len(views):.1e})")
        assert err <= PER_VIEW * len(views), (scale, err)
        label_criterion(pred, ref, len(views))


# ---------------------------------------------------------------------------------------------------------------- 4. ties
@pytest.mark.parametrize("dt,tc", DTYPES, ids=ids(DTYPES))
def test_ties_go_to_the_lower_class(dt, tc):
    shape = N, C, H, W = (2, 9, 5, 7)
    lg = torch.randn(shape, generator=torch.Generator().manual_seed(5)).to(dt).float()
    lg[:, 2] = lg[:, 5] = lg.max(dim=1).values + 1.0                                   # equal logits, above the rest: exactly equal p
    lg = lg.to(dt)
    assert torch.equal(lg[:, 2], lg[:, 5])
    for v in range(4):
        pred = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
        accumulate(lg.to(DEV).contiguous(), tc, None, pred, shape, v, first=1)
        assert bool((pred == 2).all()), v
    # two views, two classes with equal sums: class 5 wins all of view 0, class 2 all of view 3 (p exactly 1 each)
    a, b = torch.full(shape, -200.0), torch.full(shape, -200.0)
    a[:, 5], b[:, 2] = 0.0, 0.0
    acc = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    pred = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
    accumulate(a.to(dt).to(DEV).contiguous(), tc, acc, None, shape, 0, first=1)
    accumulate(b.to(dt).to(DEV).contiguous(), tc, acc, pred, shape, 3, first=0)
    assert bool((pred == 2).all())
    assert bool((acc[:, 5] == 1).all()) and float(acc.sum()) == N * H * W              # the label launch did not add view 3


# ---------------------------------------------------------------------------------------------------------------- 5. run to run
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=ids([SHAPES[2], SHAPES[3]]))
def test_run_to_run_identity(shape):
    N, C, H, W = shape
    views = views_of(H, W)
    logits = [lg.to(DEV).contiguous() for lg in normal_logits(shape, torch.bfloat16, 4.0)]
    runs = []
    for _ in range(2):
        acc = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
        pred = torch.full((N, H, W), 255, dtype=torch.uint8, device=DEV)
        for j, v in enumerate(views):
            if j == len(views) - 1:
                accumulate(logits[j], _lib.TC_BF16, acc, pred, shape, v, first=0)
            accumulate(logits[j], _lib.TC_BF16, acc, None, shape, v, first=(j == 0))
        runs.append((acc, pred))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert bool(torch.isfinite(runs[0][0]).all())


# ---------------------------------------------------------------------------------------------------------------- 6. through the API
class _Stub(torch.nn.Module):
    """Logits that depend on the intensity AND on the absolute position, so the views disagree: 6 x the one-hot of the intensity binned into
    9 levels (`_Binned` of test_postprocess_gpu.py) plus a term that varies with class, row and column.  Records what it was given and what it
    returned."""

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


class _Binned(torch.nn.Module):
    """An image of k / 8 is predicted as label k: feeds given labels to evaluate_volume."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        k = torch.round((x[:, 0] * 0.5 + 0.5) * 8).long().clamp(0, 8)
        return torch.nn.functional.one_hot(k, 9).permute(0, 3, 1, 2).float().contiguous()


def recorded_reference(stub, slices, views, batch):
    """float64 sums [N,C,H,W] from the logits the stub itself returned, batch by batch and view by view; also checks that each input was
    the torch view of the normalised batch."""
    N = slices.shape[0]
    nb = math.ceil(N / batch)
    assert len(stub.outputs) == len(views) * nb
    parts = []
    for b in range(nb):
        want = (slices[b * batch:(b + 1) * batch].float() - 0.5) / 0.5
        outs = stub.outputs[b * len(views):(b + 1) * len(views)]
        for j, v in enumerate(views):
            assert torch.equal(stub.inputs[b * len(views) + j][:, 0], view(want, v).contiguous()), (b, v)
        parts.append(sum_probs(list(views), outs))
    return torch.cat(parts)


def stub_slices(n, h, w, seed=3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 9, (n, h, w), generator=g).float() / 8).to(DEV)


@pytest.mark.parametrize("h,w,views", [(64, 64, tuple(range(8))), (48, 64, (0, 1, 2, 3)), (64, 64, (6, 3)), (32, 32, (5,))],
                         ids=["dihedral", "flips-nonsquare", "two-views", "one-view"])
def test_predict_through_a_stub(h, w, views):
    from transception_amd.evaluate import TTA, predict_probs, predict_slices
    slices, batch = stub_slices(5, h, w), 2
    m = _Stub().to(DEV).train()
    probs = predict_probs(m, slices, batch=batch, tta=TTA(views))
    assert m.training and m.modes == [False] * (len(views) * 3)                    # eval inside, restored; views x ceil(5 / 2) calls
    ref = recorded_reference(m, slices, views, batch)
    assert probs.shape == (5, 9, h, w) and probs.dtype == torch.float32
    err = float((probs.cpu().double() - ref / len(views)).abs().max())
    print(f"predict_probs {h}x{w} views {views}: max |mean - ref| = {err:.3e}")
    assert err <= PER_VIEW + 2.0 ** -24
    m2 = _Stub().to(DEV).eval()
    labels = predict_slices(m2, slices, batch=batch, tta=TTA(views))
    assert not m2.training and len(m2.outputs) == len(views) * 3
    assert labels.shape == (5, h, w) and labels.dtype == torch.uint8
    label_criterion(labels, recorded_reference(m2, slices, views, batch), len(views))


def test_predict_probs_without_tta_is_view_zero():
    from transception_amd.evaluate import predict_probs
    slices = stub_slices(3, 32, 64)
    m = _Stub().to(DEV).eval()
    probs = predict_probs(m, slices, batch=2)
    assert len(m.outputs) == 2
    ref = torch.softmax(torch.cat(m.outputs).cpu().double(), dim=1)
    assert float((probs.cpu().double() - ref).abs().max()) <= PER_VIEW


def test_evaluate_volume_and_inference_with_tta():
    """The stub's margins are wide (asserted on the float64 sums), so the labels must EQUAL the reference's, and evaluate_volume / inference
    with `tta` must equal the same functions fed those labels through `_Binned`."""
    from transception_amd._lib import _Lib
    from transception_amd.evaluate import TTA, PostProcess, evaluate_volume, inference, predict_slices
    tta, batch = TTA.dihedral(), 4
    g = np.random.default_rng(21)
    image = (g.integers(0, 9, (6, 64, 64)) / 8).astype(np.float32)
    gt = g.integers(0, 9, (6, 64, 64)).astype(np.uint8)
    m = _Stub().to(DEV).train()
    labels = predict_slices(m, torch.from_numpy(image).to(DEV), batch=batch, tta=tta)
    ref = recorded_reference(m, torch.from_numpy(image).to(DEV), tta.views, batch)
    top = ref.topk(2, dim=1).values
    assert float((top[:, 0] - top[:, 1]).min()) > 4 * PER_VIEW * 8                   # about the test's input: no pixel near a tie
    ref_labels = ref.argmax(dim=1)
    assert torch.equal(labels.cpu().long(), ref_labels)
    fed = (ref_labels.numpy() / 8).astype(np.float32)
    assert not np.array_equal(ref_labels.numpy(), np.round(image * 8))               # the position terms changed labels: the views matter
    binned = _Binned().to(DEV)
    post = PostProcess("min_voxels", 3)
    for kw in (dict(), dict(with_hd95=True), dict(host_zoom=True), dict(device_metrics=True, with_hd95=True),
               dict(device_metrics=True, postprocess=post), dict(host_zoom=True, postprocess=post)):
        calls = len(m.outputs)
        got = evaluate_volume(m, image, gt, 9, (64, 64), batch=batch, tta=tta, **kw)
        assert len(m.outputs) - calls == 8 * 2 and m.training, kw                    # views x ceil(6 / 4); training mode restored
        assert got == evaluate_volume(binned, fed, gt, 9, (64, 64), batch=batch, **kw), kw
    for dm in (False, True):
        got = inference(m, [(image, gt, "a"), (image[:3], gt[:3], "b")], 9, 64, batch=batch, device_metrics=dm, tta=tta)
        assert got == inference(binned, [(fed, gt, "a"), (fed[:3], gt[:3], "b")], 9, 64, batch=batch, device_metrics=dm), dm
    # tta=None is the call without the argument, to the bit
    plain = evaluate_volume(m, image, gt, 9, (64, 64), batch=batch, with_hd95=True)
    assert evaluate_volume(m, image, gt, 9, (64, 64), batch=batch, with_hd95=True, tta=None) == plain
    assert torch.equal(predict_slices(m, torch.from_numpy(image).to(DEV), batch=batch, tta=None),
                       predict_slices(m, torch.from_numpy(image).to(DEV), batch=batch))
    assert plain != evaluate_volume(m, image, gt, 9, (64, 64), batch=batch, with_hd95=True, tta=tta)
    # a transposed view on a 48 x 64 patch: refused before the model or the library is called
    m3 = _Stub().to(DEV).train()
    before = _Lib.calls
    with pytest.raises(ValueError, match="square"):
        evaluate_volume(m3, image[:, :48], gt[:, :48], 9, (48, 64), batch=batch, tta=tta)
    with pytest.raises(ValueError, match="square"):
        predict_slices(m3, torch.from_numpy(image[:, :48]).to(DEV), batch=batch, tta=tta)
    with pytest.raises(ValueError, match="square"):
        evaluate_volume(m3, image, gt, 9, (32, 64), batch=batch, tta=TTA((0, 4)))
    assert _Lib.calls == before and not m3.outputs and m3.training


# ---------------------------------------------------------------------------------------------------------------- 7. the real network
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


def test_real_network_four_views():
    """MSTransception(num_classes=9) at 64 x 64, B = 2, fp32, seeded weights: only the plumbing is under test, so the reference is the torch
    composition (float64 softmax, flip back, sum) over the logits the same model returned for the torch views of the input."""
    from transception_amd import MSTransception
    from transception_amd.evaluate import TTA, predict_probs, predict_slices
    from transception_amd.seeded_init import seeded_state_dict
    net = MSTransception(num_classes=9)
    net.load_state_dict(seeded_state_dict(), strict=True)
    net.to(DEV)
    net.set_compute_dtype(torch.float32)
    slices = torch.rand((2, 64, 64), generator=torch.Generator().manual_seed(9)).to(DEV)
    tta = TTA.flips()
    rec = _Recorder(net).train()
    probs = predict_probs(rec, slices, batch=2, tta=tta)
    assert rec.training and net.training and len(rec.outputs) == 4
    assert all(o.dtype == torch.float32 and o.shape == (2, 9, 64, 64) for o in rec.outputs)
    ref = recorded_reference(rec, slices, tta.views, 2)
    err = float((probs.cpu().double() - ref / 4).abs().max())
    print(f"real network, four views: max |mean - ref| = {err:.3e}")
    assert err <= PER_VIEW + 2.0 ** -24
    assert float((probs.sum(dim=1) - 1).abs().max()) <= 1e-5
    assert not torch.equal(rec.outputs[0], unview(rec.outputs[3], 3).contiguous())   # the network is not flip-equivariant: the views differ
    rec2 = _Recorder(net).eval()
    labels = predict_slices(rec2, slices, batch=2, tta=tta)
    label_criterion(labels, recorded_reference(rec2, slices, tta.views, 2), 4)


# ---------------------------------------------------------------------------------------------------------------- 8. the trainer
def test_trainer_hands_tta_to_inference(tmp_path, monkeypatch):
    """TrainConfig.tta reaches the evaluation after the last epoch: `inference` is called with it, four forward passes per batch of
    slices run in eval mode, and the model is back in training mode with a finite score in the history."""
    from transception_amd import MSTransception, trainer as T
    from transception_amd import data as D
    from transception_amd.evaluate import TTA
    from transception_amd.seeded_init import seeded_state_dict
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=1, slices_per_case=4, size=64, seed=2)
    net = MSTransception(num_classes=9)
    net.load_state_dict(seeded_state_dict(), strict=True)
    net.to(DEV)
    net.set_compute_dtype(torch.bfloat16)
    net.train()
    tta = TTA.flips()
    cfg = T.TrainConfig(root_path=base, list_dir=lists, max_epochs=1, batch_size=2, img_size=64, seed=5, model_name="tiny", tta=tta)
    seen, evals = [], []
    real = T.inference

    def spy(model, vols, *a, **kw):
        seen.append(kw.get("tta"))
        hook = model.register_forward_hook(lambda m, i, o: evals.append((m.training, tuple(i[0].shape))))
        try:
            return real(model, vols, *a, **kw)
        finally:
            hook.remove()

    monkeypatch.setattr(T, "inference", spy)
    g = np.random.default_rng(0)
    vol = (g.random((3, 64, 64)).astype(np.float32), (g.random((3, 64, 64)) * 3).astype(np.uint8), "case0")
    hist = T.trainer_synapse(cfg, net, str(tmp_path / "snap"), volumes=lambda: [vol], log=lambda s: None)
    assert seen == [tta] and seen[0] is tta
    assert evals == [(False, (3, 1, 64, 64))] * 4                                    # one batch of three slices, four views
    assert net.training and len(hist["dice"]) == 1 and 0.0 <= hist["dice"][0] <= 1.0 and math.isfinite(hist["hd95"][0])

"""The class-weighted loss with ignore_index, the parts that need no GPU: argument validation in SegLoss and TrainConfig, the host
branch of loss_from_sums (CPU sums, as the gloo tests use it) against the fp64 torch expression, the zero-denominator rule and the
three new C-ABI symbols."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

NCLS = 9


def _good_weights():
    return [0.5, 1.0, 2.0, 0.0, 4.0, 0.25, 1.5, 3.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------- 1. validation
@pytest.mark.parametrize("kw", [
    dict(ce_weight=[1.0] * 8),                                     # wrong length
    dict(ce_weight=[1.0] * 10),
    dict(dice_weight=[1.0] * 8),
    dict(ce_weight=[1.0] * 8 + [-0.5]),                            # negative
    dict(dice_weight=[1.0] * 8 + [-0.5]),
    dict(ce_weight=[1.0] * 8 + [float("nan")]),                    # not finite
    dict(ce_weight=[1.0] * 8 + [float("inf")]),
    dict(dice_weight=[1.0] * 8 + [float("nan")]),
    dict(ce_weight=[0.0] * 9),                                     # all zero
    dict(ce_weight=[1.0] * 8 + [True]),                            # bools
    dict(dice_weight=[False] + [1.0] * 8),
    dict(ce_weight=[1.0] * 8 + ["1"]),
    dict(ce_weight=3.0),                                           # not a sequence
    dict(ignore_index=0), dict(ignore_index=8), dict(ignore_index=4),      # inside the class range
    dict(ignore_index=True), dict(ignore_index=255.0), dict(ignore_index="255"),
    dict(ignore_index=2 ** 31), dict(ignore_index=-2 ** 31),       # does not fit the kernels' 32-bit compare / is their "off" value
])
def test_seg_loss_rejects_bad_arguments(kw):
    from transception_amd.train import SegLoss
    with pytest.raises(ValueError):
        SegLoss(NCLS, **kw)


def test_seg_loss_accepts_good_arguments_and_routes():
    from transception_amd.train import IGNORE_NONE, SegLoss
    plain = SegLoss(NCLS)
    assert not plain.weighted and plain._route("cpu") is None                      # nothing set: today's calls
    assert SegLoss(NCLS, dice_weight=[0.0] * 9).weighted                           # an all-zero Dice weight is allowed
    for ii in (255, -100, 9, -1):
        assert SegLoss(NCLS, ignore_index=ii).ignore_index == ii
    lf = SegLoss(NCLS, ce_weight=_good_weights(), ignore_index=255)
    w, ii = lf._route("cpu")
    assert ii == 255 and w.dtype == torch.float32 and w.tolist() == _good_weights() + [1.0] * 9      # CE weights, then Dice weights
    assert lf.weights("cpu") is w                                                  # one tensor per device, never replaced
    lf = SegLoss(NCLS, dice_weight=tuple(_good_weights()))
    w, ii = lf._route("cpu")
    assert ii == IGNORE_NONE == -2 ** 31 and w.tolist() == [1.0] * 9 + _good_weights()
    with pytest.raises(ValueError):
        SegLoss(17, ignore_index=255)                                              # the kernels take at most 16 classes
    assert not SegLoss(17).weighted


@pytest.mark.parametrize("kw", [
    dict(class_weights=(1.0,) * 8), dict(class_weights=(1.0,) * 8 + (-1.0,)), dict(class_weights=(1.0,) * 8 + (float("nan"),)),
    dict(class_weights=(0.0,) * 9), dict(class_weights=(1.0,) * 8 + (True,)), dict(class_weights=2.0),
    dict(ignore_index=3), dict(ignore_index=True), dict(ignore_index=1.5),
    dict(num_classes=4, class_weights=(1.0,) * 9), dict(num_classes=4, ignore_index=3),
])
def test_train_config_rejects_bad_arguments(kw):
    from transception_amd.trainer import TrainConfig
    with pytest.raises(ValueError):
        TrainConfig(root_path="x", list_dir="y", **kw)


def test_train_config_accepts_good_arguments():
    from transception_amd.trainer import TrainConfig
    cfg = TrainConfig(root_path="x", list_dir="y")
    assert cfg.class_weights is None and cfg.ignore_index is None
    cfg = TrainConfig(root_path="x", list_dir="y", class_weights=tuple(_good_weights()), ignore_index=255)
    assert cfg.class_weights == tuple(_good_weights()) and cfg.ignore_index == 255
    TrainConfig(root_path="x", list_dir="y", num_classes=4, class_weights=(1, 2, 0, 1), ignore_index=4)


# ---------------------------------------------------------------------------------------------------------------- 2. loss_from_sums on the host
def _cpu_sums(logits, labels, w_ce, ii):
    """The sums vector as the weighted forward leaves it, built on the CPU in double: sums[0] = sum_i w[y_i] nll_i and the unweighted
    I_k, Y_k, Z_k, all over the pixels whose label is not ii."""
    ncls = logits.shape[1]
    p = torch.softmax(logits, 1)
    valid = labels != ii
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    oh = F.one_hot(safe, ncls).permute(0, 3, 1, 2).double() * valid[:, None]
    nll = -torch.log(p.gather(1, safe[:, None])[:, 0])
    s = torch.zeros(1 + 3 * ncls, dtype=torch.float64)
    s[0] = (w_ce[safe] * nll * valid).sum()
    s[1::3] = (p * oh).sum((0, 2, 3))
    s[2::3] = oh.sum((0, 2, 3))
    s[3::3] = (p * p * valid[:, None]).sum((0, 2, 3))
    return s


def _reference(logits, labels, w_ce, w_dice, ii):
    """fp64 torch: F.cross_entropy(weight, ignore_index) and the Dice of tests/test_ops_gpu.py::test_seg_loss_and_sgd with a valid-pixel
    mask on both p and the one-hot and dice_weight inside the class sum."""
    ncls = logits.shape[1]
    ce = F.cross_entropy(logits, labels, weight=w_ce, ignore_index=ii)
    p = torch.softmax(logits, 1)
    valid = (labels != ii)[:, None].double()
    oh = F.one_hot(torch.where(labels != ii, labels, torch.zeros_like(labels)), ncls).permute(0, 3, 1, 2).double() * valid
    p = p * valid
    inter, ys, zs = (p * oh).sum((0, 2, 3)), oh.sum((0, 2, 3)), (p * p).sum((0, 2, 3))
    dice = (w_dice * (1 - (2 * inter + 1e-5) / (zs + ys + 1e-5))).sum() / ncls
    return 0.4 * ce + 0.6 * dice, ce, dice


def test_host_loss_from_sums_with_weights_matches_fp64_torch():
    from transception_amd.train import loss_from_sums
    g = torch.Generator().manual_seed(3)
    B, H, ii = 2, 16, 255
    logits = torch.randn(B, NCLS, H, H, generator=g, dtype=torch.float64) * 2.0
    labels = torch.randint(0, NCLS, (B, H, H), generator=g)
    labels[torch.rand(B, H, H, generator=g) < 0.25] = ii                          # about a quarter of the pixels ignored
    assert 0.15 < float((labels == ii).double().mean()) < 0.35
    w_ce = torch.tensor(_good_weights(), dtype=torch.float64)
    w_dice = torch.tensor(_good_weights()[::-1], dtype=torch.float64)
    sums = _cpu_sums(logits, labels, w_ce, ii)
    want = _reference(logits, labels, w_ce, w_dice, ii)
    assert all(bool(torch.isfinite(t)) for t in want)
    got = loss_from_sums(sums, float("nan"), 0.4, 0.6, torch.cat([w_ce, w_dice]))  # n_pix is not used on the weighted path
    for a, b, name in zip(got, want, ("loss", "ce", "dice")):
        assert abs(float(a) - float(b)) < 1e-12, (name, float(a), float(b))
    # fp32 sums and fp32 weights (what the gloo tests would hold): same values to fp32 rounding of the inputs
    got32 = loss_from_sums(sums.float(), 0.0, 0.4, 0.6, torch.cat([w_ce, w_dice]).float())
    assert got32[0].dtype == torch.float64 and abs(float(got32[0]) - float(want[0])) < 1e-6
    # all-ones weights and nothing ignored: the plain expression
    labels2 = torch.randint(0, NCLS, (B, H, H), generator=g)
    ones = torch.ones(NCLS, dtype=torch.float64)
    s2 = _cpu_sums(logits, labels2, ones, ii)
    a = loss_from_sums(s2, float(B * H * H), 0.4, 0.6)
    b = loss_from_sums(s2, 0.0, 0.4, 0.6, torch.ones(2 * NCLS, dtype=torch.float64))
    assert all(abs(float(x) - float(y)) < 1e-12 for x, y in zip(a, b))


def test_zero_denominator_gives_zero_ce_and_a_finite_loss():
    from transception_amd.train import loss_from_sums
    g = torch.Generator().manual_seed(4)
    logits = torch.randn(1, NCLS, 8, 8, generator=g, dtype=torch.float64)
    w = torch.tensor(_good_weights(), dtype=torch.float64)                         # class 3 has weight 0
    every_ignored = torch.full((1, 8, 8), 255)
    only_zero_weight = torch.full((1, 8, 8), 3)
    for labels in (every_ignored, only_zero_weight):
        sums = _cpu_sums(logits, labels, w, 255)
        loss, ce, dice = loss_from_sums(sums, 64.0, 0.4, 0.6, torch.cat([w, w]))
        assert float(ce) == 0.0 and bool(torch.isfinite(loss)) and bool(torch.isfinite(dice))
        assert abs(float(loss) - 0.6 * float(dice)) < 1e-15
    # (torch itself gives NaN here: the stated difference)
    assert bool(torch.isnan(F.cross_entropy(logits, every_ignored, weight=w, ignore_index=255)))


# ---------------------------------------------------------------------------------------------------------------- 3. the library
def test_library_exports_the_weighted_loss_entries():
    from transception_amd import _lib
    from transception_amd.build import build
    dll = ctypes.CDLL(build(verbose=False))
    for name, nargs in (("tc_seg_loss_fwd_w", 12), ("tc_seg_loss_value_w", 7), ("tc_seg_loss_bwd_w", 18)):
        assert hasattr(dll, name), name
        assert len(_lib.SIGNATURES[name]) == nargs
    assert dll.tc_abi_version() == _lib.ABI_VERSION
    # argument checks come before any launch, so they run without a GPU: a class index as ignore_index, and more than 16 classes
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    lab = (ctypes.c_longlong * 4)()
    p, lp = ctypes.addressof(buf), ctypes.addressof(lab)
    for ncls, ii in ((9, 0), (9, 8), (17, 255)):
        with pytest.raises(_lib.TcError, match="status -1"):
            L.tc_seg_loss_fwd_w(p, 0, lp, None, ii, p, p, 1, ncls, 4, 0, None)
        with pytest.raises(_lib.TcError, match="status -1"):
            L.tc_seg_loss_bwd_w(p, None, 0, lp, None, ii, p, p, 0, 1, ncls, 4, 0.4, 0.6, 1.0, None, 0, None)
    with pytest.raises(_lib.TcError, match="status -1"):
        L.tc_seg_loss_value_w(p, None, 17, 0.4, 0.6, p, None)

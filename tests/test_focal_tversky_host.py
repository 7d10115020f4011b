"""Focal cross-entropy and Tversky overlap, the parts that need no GPU: the float64 reference of tests/focal_tversky_ref.py against the
class-weighted reference and against the closed-form gradient of include/transception_loss.h, the validation in SegLoss and TrainConfig,
the host branch of loss_from_sums, the side header's binding and the refusals of the three entries (status -1 before any launch)."""
import ctypes
import inspect

import pytest
import torch

from focal_tversky_ref import closed_form, reference

NCLS = 9
II = 255
SETTINGS = [(g, o, a, b) for g in (0.0, 0.5, 2.0) for o, a, b in (("dice", 0.5, 0.5), ("tversky", 0.5, 0.5), ("tversky", 0.3, 0.7),
                                                                     ("tversky", 1.0, 0.0), ("tversky", 0.9, 0.6))]


def _case(seed, B=2, HW=45, ncls=NCLS, frac=0.2):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, ncls, HW, generator=g, dtype=torch.float64) * 2.0
    labels = torch.randint(0, ncls, (B, HW), generator=g)
    labels[torch.rand(B, HW, generator=g) < frac] = II
    w_ce = 0.25 + 3.75 * torch.rand(ncls, generator=g, dtype=torch.float64)
    w_dice = 0.25 + 3.75 * torch.rand(ncls, generator=g, dtype=torch.float64)
    w_ce[3] = 0.0
    return logits, labels, w_ce, w_dice


# ---------------------------------------------------------------------------------------------------------------- 1. the reference itself
def test_reference_at_gamma_0_and_dice_is_the_class_weighted_reference():
    from test_weighted_loss_gpu import reference as weighted_reference
    logits, labels, w_ce, w_dice = _case(1)
    for wc, wd, ii in ((w_ce, w_dice, II), (None, None, None), (w_ce, None, II)):
        lab = labels if ii is not None else labels.clamp(max=NCLS - 1)
        want = weighted_reference(logits, lab, wc, wd, ii)
        got = reference(logits, lab, wc, wd, ii)
        for a, b in zip((got.loss, got.ce, got.overlap), want[:3]):
            assert abs(a - b) < 1e-13, (a, b)
        assert float((got.grad - want[3]).abs().max()) < 1e-15
        assert torch.equal(got.grad, got.grad_ce + got.grad_overlap)


@pytest.mark.parametrize("gamma,overlap,alpha,beta", SETTINGS)
def test_closed_form_gradient_is_autograd(gamma, overlap, alpha, beta):
    """The gradient as the header states it (m_i, ca_k, cb_k; cb not multiplied by p under Tversky) against float64 autograd, to 1e-12:
    with weights and ignored pixels, and without either."""
    logits, labels, w_ce, w_dice = _case(2)
    for wc, wd, ii in ((w_ce, w_dice, II), (None, None, None)):
        lab = labels if ii is not None else labels.clamp(max=NCLS - 1)
        want = reference(logits, lab, wc, wd, ii, gamma, overlap, alpha, beta)
        got = closed_form(logits, lab, wc, wd, ii, gamma, overlap, alpha, beta)
        err = float((got - want.grad).abs().max())
        assert err < 1e-12, err
        if ii is not None:
            assert bool((got.permute(0, 2, 1)[lab == ii] == 0).all())


def test_tversky_half_half_is_the_linear_dice_not_the_reference_dice():
    logits, labels, _, _ = _case(3)
    tv = reference(logits, labels, None, None, II, 0.0, "tversky", 0.5, 0.5)
    I, Y, P = tv.sums[1::3], tv.sums[2::3], tv.sums[3::3]
    linear = (1.0 - (2.0 * I + 2e-5) / (P + Y + 2e-5)).sum() / NCLS
    assert abs(tv.overlap - float(linear)) < 1e-13
    assert abs(tv.overlap - reference(logits, labels, None, None, II).overlap) > 1e-3


# ---------------------------------------------------------------------------------------------------------------- 2. validation
@pytest.mark.parametrize("kw", [
    dict(focal_gamma=-0.5), dict(focal_gamma=float("nan")), dict(focal_gamma=float("inf")), dict(focal_gamma=True), dict(focal_gamma="2"),
    dict(focal_gamma=None),
    dict(overlap="Dice"), dict(overlap="focal"), dict(overlap=1), dict(overlap=None),
    dict(overlap="tversky", tversky_alpha=-0.1), dict(overlap="tversky", tversky_beta=-0.1),
    dict(overlap="tversky", tversky_alpha=float("nan")), dict(overlap="tversky", tversky_beta=float("inf")),
    dict(overlap="tversky", tversky_alpha=0.0, tversky_beta=0.0), dict(overlap="tversky", tversky_alpha=True),
    dict(overlap="tversky", tversky_beta="0.5"),
    dict(tversky_alpha=0.3), dict(tversky_beta=0.7), dict(overlap="dice", tversky_alpha=0.3, tversky_beta=0.7),     # a typo must not train on Dice
])
def test_bad_values_raise_in_seg_loss_and_train_config(kw):
    from transception_amd.train import SegLoss
    from transception_amd.trainer import TrainConfig
    with pytest.raises(ValueError):
        SegLoss(NCLS, **kw)
    with pytest.raises(ValueError):
        TrainConfig("root", "lists", **kw)


def test_defaults_and_routes():
    from transception_amd.train import IGNORE_NONE, SegLoss
    lf = SegLoss(NCLS)
    assert (lf.focal_gamma, lf.overlap, lf.tversky_alpha, lf.tversky_beta) == (0.0, "dice", 0.5, 0.5)
    assert not lf.focal_tversky and lf._route("cpu") is None                                          # today's calls
    assert SegLoss(NCLS, focal_gamma=0.0, overlap="dice", tversky_alpha=0.5, tversky_beta=0.5)._route("cpu") is None
    assert SegLoss(NCLS, focal_gamma=0)._route("cpu") is None
    assert len(SegLoss(NCLS, ignore_index=II)._route("cpu")) == 2                                     # the class-weighted entries, as today
    w, ii, *rest = SegLoss(NCLS, focal_gamma=2)._route("cpu")
    assert ii == IGNORE_NONE and w.tolist() == [1.0] * (2 * NCLS) and rest == [2.0, "dice", 0.5, 0.5]
    lf = SegLoss(NCLS, overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7, ignore_index=II, ce_weight=[2.0] * NCLS)
    w, ii, *rest = lf._route("cpu")
    assert ii == II and w.tolist() == [2.0] * NCLS + [1.0] * NCLS and rest == [0.0, "tversky", 0.3, 0.7] and lf.weights("cpu") is w
    assert SegLoss(NCLS, overlap="tversky", tversky_alpha=1, tversky_beta=0).focal_tversky            # one of the two may be 0
    import numpy as np
    lf = SegLoss(NCLS, focal_gamma=np.float32(2.0), overlap="tversky", tversky_alpha=np.float64(0.25), tversky_beta=1)     # any real number
    assert lf._route("cpu")[2:] == (2.0, "tversky", 0.25, 1.0) and all(type(v) is float for v in (lf.focal_gamma, lf.tversky_alpha, lf.tversky_beta))
    with pytest.raises(ValueError):
        SegLoss(17, focal_gamma=2.0)                                                                  # the kernels take at most 16 classes
    assert SegLoss(17)._route("cpu") is None


def test_train_config_options_are_keyword_only_and_the_fields_are_what_they_were():
    import dataclasses
    from transception_amd.trainer import TrainConfig
    cfg = TrainConfig("root", "lists")
    assert (cfg.focal_gamma, cfg.overlap, cfg.tversky_alpha, cfg.tversky_beta) == (0.0, "dice", 0.5, 0.5)
    assert (TrainConfig.focal_gamma, TrainConfig.overlap, TrainConfig.tversky_alpha, TrainConfig.tversky_beta) == (0.0, "dice", 0.5, 0.5)
    cfg = TrainConfig("root", "lists", focal_gamma=2.0, overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7, resample="scores")
    assert (cfg.focal_gamma, cfg.overlap, cfg.tversky_alpha, cfg.tversky_beta, cfg.resample) == (2.0, "tversky", 0.3, 0.7, "scores")
    params = inspect.signature(TrainConfig).parameters
    for name in ("focal_gamma", "overlap", "tversky_alpha", "tversky_beta"):
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY
    # the options are no fields: == does not see them (stated beside KEYWORD_OPTIONS), repr does
    assert cfg == TrainConfig("root", "lists") and repr(cfg) != repr(TrainConfig("root", "lists"))
    assert repr(cfg).endswith("focal_gamma=2.0, overlap='tversky', tversky_alpha=0.3, tversky_beta=0.7, resample='scores')")
    names = [f.name for f in dataclasses.fields(TrainConfig)]
    assert names[-4:] == ["no_decay", "ema_decay", "ema_warmup", "ema_eval"] and not {"focal_gamma", "overlap"} & set(names)
    # positionally as before: every positional parameter filled in order, none of the new options among them
    positional = [p for p in params.values() if p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD]
    assert [p.name for p in positional[:4]] == ["root_path", "list_dir", "num_classes", "max_epochs"]
    full = TrainConfig("root", "lists", *[p.default for p in positional[2:]])
    assert full == TrainConfig("root", "lists") and full.overlap == "dice"
    with pytest.raises(TypeError):
        TrainConfig("root", "lists", *[p.default for p in positional[2:]], 2.0)


# ---------------------------------------------------------------------------------------------------------------- 3. loss_from_sums on the host
@pytest.mark.parametrize("gamma,overlap,alpha,beta", SETTINGS)
def test_host_loss_from_sums_matches_the_reference(gamma, overlap, alpha, beta):
    from transception_amd.train import loss_from_sums
    logits, labels, w_ce, w_dice = _case(4)
    want = reference(logits, labels, w_ce, w_dice, II, gamma, overlap, alpha, beta)
    got = loss_from_sums(want.sums, float("nan"), 0.4, 0.6, torch.cat([w_ce, w_dice]), overlap=overlap, tversky_alpha=alpha, tversky_beta=beta)
    for a, b in zip(got, (want.loss, want.ce, want.overlap)):
        assert a.dtype == torch.float64 and abs(float(a) - b) < 1e-12, (float(a), b)
    # no weights: the denominator is the number of counted pixels
    lab = labels.clamp(max=NCLS - 1)
    want = reference(logits, lab, None, None, None, gamma, overlap, alpha, beta)
    got = loss_from_sums(want.sums, float(lab.numel()), 0.4, 0.6, overlap=overlap, tversky_alpha=alpha, tversky_beta=beta)
    for a, b in zip(got, (want.loss, want.ce, want.overlap)):
        assert abs(float(a) - b) < 1e-12, (float(a), b)
    with pytest.raises(ValueError):
        loss_from_sums(want.sums, 1.0, 0.4, 0.6, overlap="linear")


def test_host_loss_from_sums_with_every_pixel_ignored():
    from transception_amd.train import loss_from_sums
    logits, labels, w_ce, w_dice = _case(5)
    want = reference(logits, torch.full_like(labels, II), w_ce, w_dice, II, 2.0, "tversky", 0.3, 0.7)
    got = loss_from_sums(want.sums, 0.0, 0.4, 0.6, torch.cat([w_ce, w_dice]), overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7)
    assert float(got[1]) == 0.0 == want.ce and abs(float(got[2])) < 1e-15 and abs(want.overlap) < 1e-15      # T_k = eps / eps = 1


# ---------------------------------------------------------------------------------------------------------------- 4. the library
ENTRIES = {"tc_loss_abi_version": 0, "tc_seg_loss_fwd_ft": 14, "tc_seg_loss_value_ft": 10, "tc_seg_loss_bwd_ft": 22}


def test_binding_of_the_side_header():
    from transception_amd import _header, _lib
    assert _header.SIDE_HEADERS[-1].attr == "LOSS" and _header.SIDE_HEADERS[-1].file == "transception_loss.h"
    assert _lib.LOSS.constants == {"TC_LOSS_ABI_VERSION": 1, "TC_OVERLAP_DICE": 0, "TC_OVERLAP_TVERSKY": 1}
    assert {n: len(f.argtypes) for n, f in _lib.LOSS.functions.items()} == ENTRIES
    assert {n for n, f in _lib.LOSS.functions.items() if f.query} == {"tc_loss_abi_version"}
    assert _lib.LOSS_ABI_VERSION == 1 and not set(ENTRIES) & set(_lib.SIGNATURES)                # nothing of it in the main header
    at = _lib.LOSS.functions["tc_seg_loss_bwd_ft"].argtypes
    assert at[12:16] == [ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int] and at[16:19] == [ctypes.c_float] * 3


def test_library_exports_and_refusals():
    """Argument checks come before any launch, so they run without a GPU (host pointers are never dereferenced by a refused call)."""
    from transception_amd import _lib
    from transception_amd.build import build
    dll = ctypes.CDLL(build(verbose=False))
    for name in ENTRIES:
        assert hasattr(dll, name), name
    assert dll.tc_loss_abi_version() == _lib.LOSS_ABI_VERSION == 1
    L = _lib.lib()
    assert L.tc_loss_abi_version is L.cdll.tc_loss_abi_version and L.tc_seg_loss_fwd_ft is not L.cdll.tc_seg_loss_fwd_ft
    buf = (ctypes.c_float * 64)()
    lab = (ctypes.c_longlong * 4)()
    p, lp = ctypes.addressof(buf), ctypes.addressof(lab)
    nan, inf = float("nan"), float("inf")
    DICE, TV, OFF = _lib.TC_OVERLAP_DICE, _lib.TC_OVERLAP_TVERSKY, _lib.TC_IGNORE_NONE

    def fwd(gamma=2.0, overlap=TV, ii=OFF, ncls=9, ld=0, prob=p):
        L.tc_seg_loss_fwd_ft(p, ld, lp, None, ii, gamma, overlap, prob, p, 1, ncls, 4, 0, None)

    def value(overlap=TV, alpha=0.3, beta=0.7, ncls=9):
        L.tc_seg_loss_value_ft(p, None, ncls, 0.4, 0.6, overlap, alpha, beta, p, None)

    def bwd(gamma=2.0, overlap=TV, alpha=0.3, beta=0.7, ii=OFF, ncls=9):
        L.tc_seg_loss_bwd_ft(p, None, 0, lp, None, ii, p, p, 0, 1, ncls, 4, 0.4, 0.6, gamma, overlap, alpha, beta, 1.0, None, 0, None)

    bad = [lambda: fwd(gamma=-0.5), lambda: fwd(gamma=nan), lambda: fwd(gamma=inf), lambda: fwd(overlap=2), lambda: fwd(overlap=-1),
           lambda: fwd(ii=0), lambda: fwd(ii=8), lambda: fwd(ncls=17), lambda: fwd(prob=None), lambda: fwd(ld=8),
           lambda: value(overlap=2), lambda: value(alpha=-0.1), lambda: value(beta=-0.1), lambda: value(alpha=nan), lambda: value(beta=inf),
           lambda: value(alpha=0.0, beta=0.0), lambda: value(ncls=17),
           lambda: bwd(gamma=-0.5), lambda: bwd(gamma=nan), lambda: bwd(gamma=inf), lambda: bwd(overlap=2), lambda: bwd(alpha=-0.1),
           lambda: bwd(beta=-0.1), lambda: bwd(alpha=nan), lambda: bwd(alpha=inf), lambda: bwd(beta=nan), lambda: bwd(alpha=0.0, beta=0.0),
           lambda: bwd(ii=0), lambda: bwd(ii=8), lambda: bwd(ncls=17)]
    for call in bad:
        with pytest.raises(_lib.TcError, match="status -1"):
            call()

"""Top-k (hard-pixel) cross-entropy, the parts that need no GPU: the side header's binding and placement, the library's exports, version
and refusals (status -1 before any launch), the validation, defaults and routes of SegLoss and TrainConfig, the host branch of
loss_from_sums, and the float64 reference of tests/topk_ref.py against torch.topk over CrossEntropyLoss(reduction="none")."""
import ctypes
import inspect
import math

import pytest
import torch

from topk_ref import reference, reference_ranks, select, topk_k

NCLS = 9
II = 255
ENTRIES = {"tc_topk_abi_version": 0, "tc_topk_work_bytes": 0, "tc_seg_loss_fwd_topk": 15, "tc_topk_select": 7, "tc_seg_loss_value_topk": 10,
           "tc_seg_loss_bwd_topk": 25}


def _case(seed, B=2, HW=45, ncls=NCLS, frac=0.2):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, ncls, HW, generator=g, dtype=torch.float64) * 2.0
    labels = torch.randint(0, ncls, (B, HW), generator=g)
    labels[torch.rand(B, HW, generator=g) < frac] = II
    w_ce = 0.25 + 3.75 * torch.rand(ncls, generator=g, dtype=torch.float64)
    w_dice = 0.25 + 3.75 * torch.rand(ncls, generator=g, dtype=torch.float64)
    return logits, labels, w_ce, w_dice


# ---------------------------------------------------------------------------------------------------------------- 1. the header and the library
def test_binding_and_placement_of_the_side_header():
    from transception_amd import _header, _lib
    attrs = [s.attr for s in _header.SIDE_HEADERS]
    assert "TOPK" in attrs and attrs[-1] == "LOSS" and attrs.index("TOPK") < len(attrs) - 1
    side = _header.SIDE_HEADERS[attrs.index("TOPK")]
    assert (side.file, side.version, side.entry) == ("transception_topk.h", "TC_TOPK_ABI_VERSION", "tc_topk_abi_version")
    assert _lib.TOPK.constants == {"TC_TOPK_ABI_VERSION": 1} and _lib.TOPK.structs == {}              # plain arrays only
    assert {n: len(f.argtypes) for n, f in _lib.TOPK.functions.items()} == ENTRIES
    assert {n for n, f in _lib.TOPK.functions.items() if f.query} == {"tc_topk_abi_version", "tc_topk_work_bytes"}
    assert _lib.TOPK.functions["tc_topk_work_bytes"].restype is ctypes.c_longlong
    assert _lib.TOPK_ABI_VERSION == 1
    assert not set(ENTRIES) & set(_lib.SIGNATURES) and not set(ENTRIES) & set(_lib.LOSS.functions)     # nothing of it in the main or LOSS headers
    at = _lib.TOPK.functions["tc_seg_loss_bwd_topk"].argtypes
    assert at[:20] == _lib.LOSS.functions["tc_seg_loss_bwd_ft"].argtypes[:20]                          # the _ft arguments, then the three new ones
    assert at[20:] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    af = _lib.TOPK.functions["tc_seg_loss_fwd_topk"].argtypes
    assert af[:9] == _lib.LOSS.functions["tc_seg_loss_fwd_ft"].argtypes[:9] and af[9] is ctypes.c_void_p
    assert _lib.TOPK.functions["tc_seg_loss_value_topk"].argtypes == _lib.LOSS.functions["tc_seg_loss_value_ft"].argtypes
    assert _lib.TOPK.functions["tc_topk_select"].argtypes == [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double,
                                                              ctypes.c_void_p, ctypes.c_void_p]


def test_library_exports_version_and_refusals():
    """Argument checks come before any launch, so they run without a GPU (host pointers are never dereferenced by a refused call)."""
    from transception_amd import _lib
    from transception_amd.build import SOURCES, build
    assert "topk.hip" in SOURCES
    dll = ctypes.CDLL(build(verbose=False))
    for name in ENTRIES:
        assert hasattr(dll, name), name
    assert dll.tc_topk_abi_version() == _lib.TOPK_ABI_VERSION == 1
    L = _lib.lib()
    assert L.tc_topk_work_bytes is L.cdll.tc_topk_work_bytes and L.tc_topk_select is not L.cdll.tc_topk_select
    wb = L.tc_topk_work_bytes()
    assert 4 * 4 * 256 < wb <= 1 << 16 and wb % 8 == 0                                                 # four 256-bin histograms and the fp64 slots
    buf = (ctypes.c_double * 64)()
    lab = (ctypes.c_longlong * 4)()
    p, lp = ctypes.addressof(buf), ctypes.addressof(lab)
    nan, inf = float("nan"), float("inf")
    TV, OFF = _lib.TC_OVERLAP_TVERSKY, _lib.TC_IGNORE_NONE

    def fwd(gamma=2.0, overlap=TV, ii=OFF, ncls=9, ld=0, prob=p, values=p):
        L.tc_seg_loss_fwd_topk(p, ld, lp, None, ii, gamma, overlap, prob, p, values, 1, ncls, 4, 0, None)

    def sel(values=p, n=4, state=p, sums=p, inv_world=1.0, work=p):
        L.tc_topk_select(values, n, state, sums, inv_world, work, None)

    def value(overlap=TV, alpha=0.3, beta=0.7, ncls=9):
        L.tc_seg_loss_value_topk(p, None, ncls, 0.4, 0.6, overlap, alpha, beta, p, None)

    def bwd(gamma=2.0, overlap=TV, alpha=0.3, beta=0.7, ii=OFF, ncls=9, values=p, state=p, inv_world=1.0):
        L.tc_seg_loss_bwd_topk(p, None, 0, lp, None, ii, p, p, 0, 1, ncls, 4, 0.4, 0.6, gamma, overlap, alpha, beta, 1.0, None, values, state,
                               inv_world, 0, None)

    bad = [lambda: fwd(gamma=-0.5), lambda: fwd(gamma=nan), lambda: fwd(gamma=inf), lambda: fwd(overlap=2), lambda: fwd(ii=0), lambda: fwd(ii=8),
           lambda: fwd(ncls=17), lambda: fwd(prob=None), lambda: fwd(ld=8), lambda: fwd(values=None),
           lambda: sel(values=None), lambda: sel(n=0), lambda: sel(n=-1), lambda: sel(n=2 ** 31 - 1), lambda: sel(state=None), lambda: sel(sums=None),
           lambda: sel(work=None), lambda: sel(work=p + 4), lambda: sel(state=p + 4), lambda: sel(inv_world=0.0), lambda: sel(inv_world=-0.5),
           lambda: sel(inv_world=2.0), lambda: sel(inv_world=nan), lambda: sel(inv_world=inf),
           lambda: value(overlap=2), lambda: value(alpha=-0.1), lambda: value(alpha=nan), lambda: value(alpha=0.0, beta=0.0), lambda: value(ncls=17),
           lambda: bwd(gamma=-0.5), lambda: bwd(gamma=nan), lambda: bwd(overlap=2), lambda: bwd(alpha=-0.1), lambda: bwd(beta=inf),
           lambda: bwd(alpha=0.0, beta=0.0), lambda: bwd(ii=0), lambda: bwd(ii=8), lambda: bwd(ncls=17), lambda: bwd(values=None),
           lambda: bwd(state=None), lambda: bwd(state=p + 4), lambda: bwd(inv_world=0.0), lambda: bwd(inv_world=1.5), lambda: bwd(inv_world=nan)]
    for call in bad:
        with pytest.raises(_lib.TcError, match="status -1"):
            call()


# ---------------------------------------------------------------------------------------------------------------- 2. validation, defaults, routes
@pytest.mark.parametrize("frac", [0, 0.0, -0.1, 1.0000001, 2, float("nan"), float("inf"), True, False, "0.1", [0.1]])
def test_bad_fractions_raise_in_seg_loss_and_train_config(frac):
    from transception_amd.train import SegLoss
    from transception_amd.trainer import TrainConfig
    with pytest.raises(ValueError):
        SegLoss(NCLS, ce_topk=frac)
    with pytest.raises(ValueError):
        TrainConfig("root", "lists", ce_topk=frac)
    with pytest.raises(ValueError):
        SegLoss(NCLS, ce_topk=0.5).set_topk(frac)


def test_defaults_and_routes():
    import numpy as np
    from transception_amd.train import IGNORE_NONE, SegLoss
    lf = SegLoss(NCLS)
    assert lf.ce_topk is None and lf._route("cpu") is None and lf._topk_state == {}                   # today's calls, nothing allocated
    assert len(SegLoss(NCLS, ignore_index=II)._route("cpu")) == 2 and len(SegLoss(NCLS, focal_gamma=2)._route("cpu")) == 6
    assert SegLoss(NCLS, ce_topk=None, focal_gamma=0.0)._route("cpu") is None
    with pytest.raises(ValueError):
        lf.topk_state("cpu")
    with pytest.raises(ValueError):
        lf.set_topk(0.5)                                                                              # off stays off: the route is fixed at construction
    lf = SegLoss(NCLS, ce_topk=0.25)
    route = lf._route("cpu")
    w, ii, *rest, state = route
    assert len(route) == 7 and ii == IGNORE_NONE and w.tolist() == [1.0] * (2 * NCLS) and rest == [0.0, "dice", 0.5, 0.5]
    assert state is lf.topk_state("cpu") and state.dtype == torch.float64 and state.tolist() == [0.25] + [0.0] * 7
    lf.set_topk(np.float32(0.5))                                                                      # any real number; in place
    assert lf.topk_state("cpu") is state and state.tolist() == [0.5] + [0.0] * 7 and type(lf.ce_topk) is float
    with pytest.raises(ValueError):
        lf.set_topk(None)
    assert lf.topk_stats("cpu") == {"n": 0, "k": 0, "n_gt": 0, "n_eq": 0, "threshold": 0.0, "tie_share": 0.0}
    lf = SegLoss(NCLS, ce_topk=1, focal_gamma=2.0, overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7, ignore_index=II, ce_weight=[2.0] * NCLS)
    w, ii, *rest, state = lf._route("cpu")
    assert ii == II and w.tolist() == [2.0] * NCLS + [1.0] * NCLS and rest == [2.0, "tversky", 0.3, 0.7] and float(state[0]) == 1.0
    with pytest.raises(ValueError):
        SegLoss(17, ce_topk=0.1)                                                                      # the kernels take at most 16 classes
    assert SegLoss(16, ce_topk=0.1).ce_topk == 0.1 and SegLoss(17)._route("cpu") is None


def test_train_config_option_is_keyword_only_and_sits_after_calibration():
    import dataclasses
    from transception_amd.trainer import KEYWORD_OPTIONS, TrainConfig
    names = [n for n, _, _ in KEYWORD_OPTIONS]
    assert names[:4] == ["surface_metrics", "calibration", "ce_topk", "focal_gamma"] and names[-1] == "resample"
    cfg = TrainConfig("root", "lists")
    assert cfg.ce_topk is None and TrainConfig.ce_topk is None
    cfg = TrainConfig("root", "lists", ce_topk=0.1)
    assert cfg.ce_topk == 0.1 and inspect.signature(TrainConfig).parameters["ce_topk"].kind is inspect.Parameter.KEYWORD_ONLY
    assert "ce_topk=0.1, focal_gamma=0.0" in repr(cfg) and repr(cfg).endswith("tversky_beta=0.5, resample='labels')")
    assert "ce_topk" not in [f.name for f in dataclasses.fields(TrainConfig)] and cfg == TrainConfig("root", "lists")
    with pytest.raises(ValueError):
        TrainConfig("root", "lists", num_classes=17, ce_topk=0.1)
    assert TrainConfig("root", "lists", num_classes=17).ce_topk is None


# ---------------------------------------------------------------------------------------------------------------- 3. k and the reference
@pytest.mark.parametrize("frac", [1e-9, 0.1, 1.0 / 3.0, 1.0])
def test_k_formula(frac):
    """k = max(1, min(n, ceil(frac n))), the product once in float64."""
    for n in (1, 2, 3, 9, 10, 11, 30, 242, 512, 270000, 2 ** 24 + 1):
        k = topk_k(frac, n)
        assert k == max(1, min(n, math.ceil(frac * n))) and 1 <= k <= n
        if frac == 1.0:
            assert k == n
        if frac == 1e-9:
            assert k == 1
    assert topk_k(0.1, 30) == 3 and topk_k(0.1, 31) == 4 and topk_k(1.0 / 3.0, 9) == 3 and topk_k(1.0 / 3.0, 10) == 4 and topk_k(frac, 0) == 0
    v = torch.arange(1, 31, dtype=torch.float64)
    s = select(v, frac)
    assert s.n == 30 and s.k == topk_k(frac, 30) and s.t == 31.0 - s.k and s.n_gt == s.k - 1 and s.n_eq == 1 and s.f == 1.0
    assert s.S == sum(range(32 - s.k, 31)) and s.ce == (s.S + s.t) / s.k


def test_select_shares_ties():
    v = torch.tensor([5.0, 3.0, 3.0, 3.0, 3.0, 1.0, 0.0, 0.0], dtype=torch.float64)
    s = select(v, 3 / 8)                                                                              # k = 3: one above, two of the four threes
    assert (s.n, s.k, s.n_gt, s.n_eq, s.t, s.S, s.f) == (8, 3, 1, 4, 3.0, 5.0, 0.5) and s.ce == 11.0 / 3.0
    s = select(v, 1.0)
    assert (s.k, s.n_gt, s.n_eq, s.t, s.f) == (8, 6, 2, 0.0, 1.0) and s.ce == 18.0 / 8.0 and s.gap == math.inf


@pytest.mark.parametrize("frac", [0.1, 0.25, 0.5, 1.0])
def test_reference_is_torch_topk_over_unreduced_cross_entropy(frac):
    """Tie-free float64 inputs: the CE is torch.topk's mean over CrossEntropyLoss(reduction="none") -- class weights and ignore_index included
    (torch multiplies the unreduced terms by the weights, and gives an ignored pixel 0, which is dropped here) -- and so is its gradient."""
    logits, labels, w_ce, w_dice = _case(11)
    for wc, ii in ((None, None), (w_ce, II)):
        lab = labels if ii is not None else labels.clamp(max=NCLS - 1)
        want = reference(logits, lab, frac, wc, w_dice, ii)
        assert want.sel[0].gap > 1e-9
        x = logits.clone().requires_grad_()
        per = torch.nn.CrossEntropyLoss(weight=wc, ignore_index=-100 if ii is None else ii, reduction="none")(x, lab)
        counted = per[lab != II] if ii is not None else per.reshape(-1)
        k = topk_k(frac, counted.numel())
        ce = torch.topk(counted, k).values.mean()
        assert want.sel[0].k == k and abs(float(ce.detach()) - want.ce) < 1e-13
        g, = torch.autograd.grad(0.4 * ce, x)
        assert float((g - want.grad_ce[0]).abs().max()) < 1e-14
        assert torch.equal(want.grad[0], want.grad_ce[0] + want.grad_overlap[0])
        if ii is not None:
            assert bool((want.values[0][lab == II] == -1.0).all()) and bool((want.grad[0].permute(0, 2, 1)[lab == II] == 0).all())


def test_reference_at_frac_1_without_weights_is_the_plain_cross_entropy_and_with_weights_is_not():
    from focal_tversky_ref import reference as ft_reference
    logits, labels, w_ce, w_dice = _case(12)
    for gamma, overlap, a, b in ((0.0, "dice", 0.5, 0.5), (2.0, "tversky", 0.3, 0.7)):
        plain = ft_reference(logits, labels, None, w_dice, II, gamma, overlap, a, b)
        full = reference(logits, labels, 1.0, None, w_dice, II, gamma, overlap, a, b)
        assert abs(full.ce - plain.ce) < 1e-13 and abs(full.overlap - plain.overlap) < 1e-15
        assert float((full.grad[0] - plain.grad).abs().max()) < 1e-14
        tenth = reference(logits, labels, 0.1, None, w_dice, II, gamma, overlap, a, b)
        assert tenth.ce > plain.ce + 1e-3 and tenth.overlap == full.overlap                            # the overlap term is untouched
    weighted = reference(logits, labels, 1.0, w_ce, w_dice, II)
    torch_mean = ft_reference(logits, labels, w_ce, w_dice, II)
    counted = labels != II
    assert abs(weighted.ce - torch_mean.ce * float(w_ce[labels[counted]].sum()) / int(counted.sum())) < 1e-12    # the divisor is k, not sum w
    assert abs(weighted.ce - torch_mean.ce) > 1e-3


def test_reference_over_ranks_is_the_mean_of_the_ranks_top_k_means():
    logits, labels, w_ce, w_dice = _case(13, B=4)
    labels[2:, :30] = II                                                                              # the second rank counts fewer pixels
    halves = [logits[:2], logits[2:]], [labels[:2], labels[2:]]
    both = reference_ranks(*halves, 0.25, w_ce, w_dice, II)
    singles = [reference(x, y, 0.25, w_ce, w_dice, II) for x, y in zip(*halves)]
    assert both.sel[0].k != both.sel[1].k and [s.k for s in both.sel] == [r.sel[0].k for r in singles]
    assert abs(both.ce - 0.5 * (singles[0].ce + singles[1].ce)) < 1e-14
    for r in range(2):
        assert float((both.grad_ce[r] - 0.5 * singles[r].grad_ce[0]).abs().max()) < 1e-15
    whole = reference(logits, labels, 0.25, w_ce, w_dice, II)
    assert abs(both.overlap - whole.overlap) < 1e-14 and abs(both.ce - whole.ce) > 1e-6               # the overlap term is global, the selection is not


# ---------------------------------------------------------------------------------------------------------------- 4. loss_from_sums on the host
@pytest.mark.parametrize("overlap,alpha,beta", [("dice", 0.5, 0.5), ("tversky", 0.3, 0.7)])
def test_host_loss_from_sums_takes_the_cross_entropy_from_the_first_sum(overlap, alpha, beta):
    from focal_tversky_ref import reference as ft_reference
    from transception_amd.train import loss_from_sums
    logits, labels, w_ce, w_dice = _case(14)
    want = reference(logits, labels, 0.25, w_ce, w_dice, II, 2.0, overlap, alpha, beta)
    sums = ft_reference(logits, labels, w_ce, w_dice, II, 2.0, overlap, alpha, beta).sums.clone()
    sums[0] = want.ce                                                                                 # what tc_topk_select leaves there
    kw = dict(overlap=overlap, tversky_alpha=alpha, tversky_beta=beta, topk=True)
    got = loss_from_sums(sums, float("nan"), 0.4, 0.6, torch.cat([w_ce, w_dice]), **kw)
    for a, b in zip(got, (want.loss, want.ce, want.overlap)):
        assert a.dtype == torch.float64 and abs(float(a) - b) < 1e-12, (float(a), b)
    want = reference(logits, labels, 0.25, None, None, II, 2.0, overlap, alpha, beta)
    sums = ft_reference(logits, labels, None, None, II, 2.0, overlap, alpha, beta).sums.clone()
    sums[0] = want.ce
    got = loss_from_sums(sums, float("nan"), 0.4, 0.6, **kw)
    for a, b in zip(got, (want.loss, want.ce, want.overlap)):
        assert abs(float(a) - b) < 1e-12, (float(a), b)
    # off, the expression is the one it was: the first sum is divided by the weighted count
    off = loss_from_sums(sums, float("nan"), 0.4, 0.6, torch.ones(2 * NCLS, dtype=torch.float64), overlap=overlap, tversky_alpha=alpha, tversky_beta=beta)
    assert abs(float(off[1]) - want.ce / float(sums[2::3].sum())) < 1e-15

"""Focal cross-entropy and Tversky overlap on the MI355X: the tc_seg_loss_*_ft entries (include/transception_loss.h), SegLoss(focal_gamma,
overlap, tversky_alpha, tversky_beta), the captured step and the trainer against the float64 autograd reference of
tests/focal_tversky_ref.py, which tests/test_focal_tversky_host.py holds to the class-weighted reference and to the closed-form gradient.

Bounds.  The three scalars: the project's 2e-6 absolute (fp32 results of O(1) losses).  The gradient: 1e-8 + 1e-4 (|CE part| + |overlap part|)
per element -- the project's 1e-8 + 1e-4 |ref| applied to the two terms before they cancel, since each is formed in fp32 on its own.
Shapes: B = 2, HW = 37 x 29 = 1073 (no multiple of 256, 64 or 4; five workgroups) and one case at B HW = 3 x 700."""
import math
import re

import pytest
import torch

from focal_tversky_ref import reference

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
II = 255
OFF = -2 ** 31                                  # TC_IGNORE_NONE
DICE, TVERSKY = 0, 1                            # TC_OVERLAP_*
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
B, HW = 2, 37 * 29
OVERLAPS = {"dice": ("dice", 0.5, 0.5), "tversky_half": ("tversky", 0.5, 0.5), "tversky_fn": ("tversky", 0.3, 0.7), "tversky_fp": ("tversky", 1.0, 0.0)}


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _weights(ncls, g, zero_at=None):
    """[0.25, 4] with exactly one class at weight 0."""
    w = 0.25 + 3.75 * torch.rand(ncls, generator=g, dtype=torch.float64)
    w[int(torch.randint(0, ncls, (1,), generator=g)) if zero_at is None else zero_at] = 0.0
    return w


def _labels(shape, ncls, g, frac):
    lab = torch.randint(0, ncls, shape, generator=g)
    n = lab.numel()
    lab.view(-1)[torch.randperm(n, generator=g)[:int(frac * n)]] = II
    return lab


def _wdev(w_ce, w_dice, ncls):
    if w_ce is None and w_dice is None:
        return None
    ones = torch.ones(ncls, dtype=torch.float64)
    return torch.cat([ones if w_ce is None else w_ce, ones if w_dice is None else w_dice]).float().to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_nchw(vals, lab, wdev, ii, gamma, overlap, alpha, beta, gscale=1.0, gscale_dev=None, w=(0.4, 0.6)):
    """The _ft entries on fp32 NCHW values [B, C, HW] (ld = 0): (out3 on the host, sums, prob, dlogits [B, C, HW])."""
    from transception_amd._lib import lib
    L, st = lib(), _stream()
    nb, C, hw = vals.shape
    code = TVERSKY if overlap == "tversky" else DICE
    prob = torch.empty(nb, C, hw, device=DEV)
    sums = torch.zeros(1 + 3 * C, device=DEV)
    out3 = torch.empty(3, device=DEV)
    d = torch.full((nb, C, hw), 7.0, device=DEV)                                   # a sentinel: every element must be written
    L.tc_seg_loss_fwd_ft(vals.data_ptr(), 0, lab.data_ptr(), _ptr(wdev), ii, gamma, code, prob.data_ptr(), sums.data_ptr(), nb, C, hw, 0, st)
    L.tc_seg_loss_value_ft(sums.data_ptr(), _ptr(wdev), C, w[0], w[1], code, alpha, beta, out3.data_ptr(), st)
    L.tc_seg_loss_bwd_ft(prob.data_ptr(), None, 0, lab.data_ptr(), _ptr(wdev), ii, sums.data_ptr(), d.data_ptr(), 0, nb, C, hw, w[0], w[1],
                         gamma, code, alpha, beta, gscale, _ptr(gscale_dev), 0, st)
    torch.cuda.synchronize()
    return out3.cpu(), sums, prob, d


def check_scalars(got, want, what):
    errs = [abs(float(a) - b) for a, b in zip(got, (want.loss, want.ce, want.overlap))]
    print(f"{what}: |loss, ce, overlap - fp64| = {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}")
    assert max(errs) < 2e-6, (what, [float(a) for a in got], (want.loss, want.ce, want.overlap))


def check_grad(got, want, what):
    got = got.detach().double().cpu()
    assert got.shape == want.grad.shape, (what, got.shape, want.grad.shape)
    err = (got - want.grad).abs()
    tol = 1e-8 + 1e-4 * (want.grad_ce.abs() + want.grad_overlap.abs())
    worst = (err / tol).max().item()
    print(f"{what}: max |dlogits - fp64| = {err.max().item():.3e} (ref max {want.grad.abs().max().item():.3e}), worst err / tol = {worst:.3f}")
    assert bool((err <= tol).all()), f"{what}: max err {err.max().item():.3e}, worst err / tol {worst:.3f}"
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. the entries against fp64
_INPUTS = {}


def _inputs(ncls, shape=(B, HW)):
    """One set of logits, labels (with and without ignored pixels) and weights per class count, shared by every setting."""
    key = (ncls, shape)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(7 * ncls + shape[0])
        vals = torch.randn(shape[0], ncls, shape[1], generator=g) * 2.0
        full = torch.randint(0, ncls, shape, generator=g)
        part = full.clone()
        part.view(-1)[torch.randperm(part.numel(), generator=g)[:part.numel() // 5]] = II        # about 20 % ignored
        _INPUTS[key] = (vals, vals.to(DEV), full, part, _weights(ncls, g), _weights(ncls, g))
    return _INPUTS[key]


@pytest.mark.parametrize("ov", list(OVERLAPS))
@pytest.mark.parametrize("gamma", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("ncls", [2, 9, 16])
def test_entries_match_fp64(ncls, gamma, ov):
    """NCHW fp32, with and without class weights (one CE weight zero), with and without ignore_index = 255 on 20 % of the pixels."""
    overlap, alpha, beta = OVERLAPS[ov]
    vals, vdev, full, part, w_ce, w_dice = _inputs(ncls)
    worst = 0.0
    for weighted in (False, True):
        for ignoring in (False, True):
            wc, wd = (w_ce, w_dice) if weighted else (None, None)
            lab_c, ii = (part, II) if ignoring else (full, None)
            want = reference(vals, lab_c, wc, wd, ii, gamma, overlap, alpha, beta)
            out3, sums, prob, d = run_nchw(vdev, lab_c.to(DEV), _wdev(wc, wd, ncls), OFF if ii is None else ii, gamma, overlap, alpha, beta)
            what = f"ncls {ncls} gamma {gamma} {ov} weights {weighted} ignore {ignoring}"
            check_scalars(out3, want, what)
            worst = max(worst, check_grad(d, want, what))
            assert not bool((d == 7.0).any())
            if ignoring:
                ign = lab_c == II
                assert bool(ign.any()) and bool((d.cpu().permute(0, 2, 1)[ign] == 0).all())
    print(f"ncls {ncls} gamma {gamma} {ov}: worst err / tol over the four cases = {worst:.3f}")


def test_entries_match_fp64_across_a_workgroup_stride():
    """B HW = 3 x 700 = 2100 pixels: nine workgroups, an image boundary inside one."""
    vals, vdev, full, part, w_ce, w_dice = _inputs(9, (3, 700))
    want = reference(vals, part, w_ce, w_dice, II, 2.0, "tversky", 0.3, 0.7)
    out3, sums, prob, d = run_nchw(vdev, part.to(DEV), _wdev(w_ce, w_dice, 9), II, 2.0, "tversky", 0.3, 0.7)
    check_scalars(out3, want, "3 x 700")
    check_grad(d, want, "3 x 700")
    assert bool((d.cpu().permute(0, 2, 1)[part == II] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 2. saturation
@pytest.mark.parametrize("ov", ["dice", "tversky_fn"])
@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_saturated_probabilities(gamma, ov):
    """Nine classes, one logit of every pixel at +a and the others at -a.  a = 40 with the label on the hot class: p_t is 1 to the last bit
    in fp32 and q = 8 e^-80 is tiny but not 0.  a = 60 with the label on the hot class: the other classes' exponentials underflow, q = 0
    exactly, and the CE gradient must be exactly 0 (no 0^(gamma - 1)).  The label on a cold class, 1 % of the pixels each: a = 40 gives
    p_t = e^-80 / (1 + ...) = 1.8e-35, a = 60 gives p_t = 0 in fp32 and 7.7e-53 in fp64 -- both below the 1e-38 clamp -- with q = 1.  A quarter
    of the pixels keep ordinary logits.  The wrong pixels are few so that the loss stays O(1), which the 2e-6 absolute bound presupposes:
    a CE of 40 has an fp32 spacing of 3.8e-6."""
    overlap, alpha, beta = OVERLAPS[ov]
    ncls = 9
    g = torch.Generator().manual_seed(61)
    n = B * HW
    hot = torch.randint(0, ncls, (n,), generator=g)
    kind = torch.rand(n, generator=g)
    a = torch.where(kind < 0.5, 40.0, 60.0)
    vals = -a[:, None].expand(n, ncls).clone()
    vals[torch.arange(n), hot] = a
    ordinary = kind > 0.75
    vals[ordinary] = torch.randn(int(ordinary.sum()), ncls, generator=g) * 2.0
    lab = hot.clone()
    wrong = (torch.rand(n, generator=g) < 0.02) & ~ordinary
    lab[wrong] = (hot[wrong] + 1 + torch.randint(0, ncls - 1, (int(wrong.sum()),), generator=g)) % ncls
    lab[torch.rand(n, generator=g) < 0.1] = II
    vals = vals.view(B, HW, ncls).permute(0, 2, 1).contiguous()
    lab = lab.view(B, HW)
    zero_q = ((a == 60.0) & ~ordinary & ~wrong).view(B, HW) & (lab != II)
    clamped = ((a == 60.0) & wrong).view(B, HW) & (lab != II)
    assert int(zero_q.sum()) > 100 and int(clamped.sum()) >= 2 and int((wrong.view(B, HW) & (lab != II)).sum()) >= 8
    w_ce, w_dice = _weights(ncls, g), _weights(ncls, g)
    want = reference(vals, lab, w_ce, w_dice, II, gamma, overlap, alpha, beta)
    out3, sums, prob, d = run_nchw(vals.to(DEV), lab.to(DEV), _wdev(w_ce, w_dice, ncls), II, gamma, overlap, alpha, beta)
    check_scalars(out3, want, f"saturated gamma {gamma} {ov}")
    assert bool(torch.isfinite(d).all()) and not bool((d == 7.0).any())
    # the premises, on the probabilities the kernel wrote
    p = prob.cpu().permute(0, 2, 1)                                                # [B, HW, C]
    onehot = torch.nn.functional.one_hot(lab.clamp(max=ncls - 1), ncls).bool()
    pt = (p * onehot).sum(-1)
    assert bool((pt[zero_q] == 1.0).all()) and bool(((p * ~onehot).sum(-1)[zero_q] == 0.0).all())
    assert bool((pt[clamped] < 1e-38).all())
    # the CE term alone (w_dice = 0): exactly zero where q = 0, finite everywhere, not zero everywhere
    _, _, _, dce = run_nchw(vals.to(DEV), lab.to(DEV), _wdev(w_ce, w_dice, ncls), II, gamma, overlap, alpha, beta, w=(0.4, 0.0))
    dce = dce.cpu().permute(0, 2, 1)
    assert bool(torch.isfinite(dce).all()) and bool((dce[zero_q] == 0.0).all()) and bool((dce[lab == II] == 0.0).all())
    assert float(dce.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- 3. structure cases
@pytest.mark.parametrize("ov", ["dice", "tversky_fn"])
@pytest.mark.parametrize("case", ["all_ignored", "class_absent", "only_zero_weight"])
def test_structure_cases(case, ov):
    """Every pixel ignored: loss, CE and the overlap term are 0 (the overlap term to fp32 rounding of eps / eps), every gradient exactly 0,
    nothing NaN.  One class absent from the labels: Y_k = 0, and under Tversky its T_k = eps / (alpha P_k + eps) is held against the
    reference.  Only zero-weight classes present: CE 0 with a zero CE gradient, the overlap term and its gradient as the reference's."""
    overlap, alpha, beta = OVERLAPS[ov]
    ncls, gamma = 9, 2.0
    g = torch.Generator().manual_seed(31)
    vals = torch.randn(B, ncls, HW, generator=g) * 2.0
    w_ce, w_dice = _weights(ncls, g, zero_at=2), _weights(ncls, g, zero_at=7)
    if case == "all_ignored":
        lab_c = torch.full((B, HW), II)
    elif case == "class_absent":
        lab_c = _labels((B, HW), ncls, g, 0.1)
        lab_c[lab_c == 4] = 5
    else:
        lab_c = torch.full((B, HW), 2)
        lab_c.view(-1)[torch.randperm(B * HW, generator=g)[:200]] = II
    want = reference(vals, lab_c, w_ce, w_dice, II, gamma, overlap, alpha, beta)
    out3, sums, prob, d = run_nchw(vals.to(DEV), lab_c.to(DEV), _wdev(w_ce, w_dice, ncls), II, gamma, overlap, alpha, beta)
    assert bool(torch.isfinite(out3).all()) and bool(torch.isfinite(d).all()) and not bool((d == 7.0).any())
    check_scalars(out3, want, f"{case} {ov}")
    check_grad(d, want, f"{case} {ov}")
    assert bool((d.cpu().permute(0, 2, 1)[lab_c == II] == 0).all())
    if case == "all_ignored":
        assert float(out3[1]) == 0.0 and abs(float(out3[0])) < 1e-6 and abs(float(out3[2])) < 1e-6 and bool((d == 0).all())
    elif case == "class_absent":
        s = sums.double().cpu()
        assert float(s[2 + 3 * 4]) == 0.0 and float(s[1 + 3 * 4]) == 0.0
        if overlap == "tversky":
            t4 = 1e-5 / (alpha * float(s[3 + 3 * 4]) + 1e-5)
            ref4 = 1e-5 / (alpha * float(want.sums[3 + 3 * 4]) + 1e-5)
            assert abs(t4 - ref4) < 1e-5 * ref4, (t4, ref4)
    else:
        assert float(out3[1]) == 0.0 and want.ce == 0.0 and float(want.grad_ce.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 4. token-major
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("ncls", [9, 16])
def test_token_major_entries(ncls, padded, dtype):
    """Token-major logits [B HW, ld], ld = 16 (16-byte padded rows) or ncls, with the probability map and without it, and once more from a base
    pointer misaligned by one element, which must take the element path.  The rule of the class-weighted test: the NCHW fp32 run of the
    same entries on the SAME stored values is held against fp64; dlogits in the storage type equals that run rounded to the storage type
    bit for bit; sums within 1e-5 relative; pad columns zero on the 16-byte path and untouched on the element path; map and recompute runs
    bit-equal."""
    from transception_amd._lib import lib
    L, st = lib(), _stream()
    ld = 16 if padded else ncls
    code = CODE[dtype]
    g = torch.Generator().manual_seed(100 * ncls + 10 * padded + code)
    w_ce, w_dice = _weights(ncls, g), _weights(ncls, g)
    lab_c = _labels((B, HW), ncls, g, 0.2)
    lab, wdev = lab_c.to(DEV), _wdev(w_ce, w_dice, ncls)
    flat = (torch.randn(B * HW * ld + 1, generator=g) * 2.0).to(DEV).to(dtype)
    for misaligned in (False, True):
        buf = flat[1:] if misaligned else flat[:-1]
        tok = buf.view(B * HW, ld)
        assert tok.data_ptr() % 16 == (flat.element_size() if misaligned else 0)
        nchw = tok[:, :ncls].float().view(B, HW, ncls).permute(0, 2, 1).contiguous()         # the stored values, widened
        vec = dtype != torch.float32 and ld % 8 == 0 and not misaligned
        pad8 = (ncls + 7) // 8 * 8 if vec else ncls
        for gamma, (overlap, alpha, beta) in ((2.0, OVERLAPS["tversky_fn"]), (0.5, OVERLAPS["dice"])):
            ov = TVERSKY if overlap == "tversky" else DICE
            what = f"ncls {ncls} ld {ld} {dtype} misaligned {misaligned} gamma {gamma} {overlap}"
            want = reference(nchw, lab_c, w_ce, w_dice, II, gamma, overlap, alpha, beta)
            out3, sa, pa, da = run_nchw(nchw, lab, wdev, II, gamma, overlap, alpha, beta, gscale=128.0)
            check_scalars(out3, want, what)
            check_grad(da / 128.0, want, what)                                     # (a power of two: the scale is exact)
            want_tok = da.permute(0, 2, 1).reshape(B * HW, ncls).to(dtype)
            runs = []
            for with_prob in (True, False):
                pb = torch.empty(B, ncls, HW, device=DEV) if with_prob else None
                sb = torch.zeros(1 + 3 * ncls, device=DEV)
                dflat = torch.full((B * HW * ld + 1,), 3.0, device=DEV, dtype=dtype)
                db = (dflat[1:] if misaligned else dflat[:-1]).view(B * HW, ld)
                L.tc_seg_loss_fwd_ft(tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, gamma, ov, _ptr(pb), sb.data_ptr(), B, ncls, HW, code, st)
                L.tc_seg_loss_bwd_ft(_ptr(pb), None if with_prob else tok.data_ptr(), ld if not with_prob else 0, lab.data_ptr(), wdev.data_ptr(), II,
                                     sa.data_ptr(), db.data_ptr(), ld, B, ncls, HW, 0.4, 0.6, gamma, ov, alpha, beta, 128.0, None, code, st)
                torch.cuda.synchronize()
                if with_prob:
                    assert torch.equal(pa, pb), what
                assert float(((sa - sb).abs() / (sa.abs() + 1e-6)).max()) < 1e-5, what
                assert torch.equal(db[:, :ncls], want_tok), (what, with_prob, float((db[:, :ncls].float() - want_tok.float()).abs().max()))
                assert bool((db[:, ncls:pad8] == 0.0).all()) and bool((db[:, pad8:] == 3.0).all()), (what, with_prob)
                assert bool((db[(lab == II).view(-1)][:, :ncls] == 0).all())
                runs.append(db)
            assert torch.equal(runs[0], runs[1]), what


# ---------------------------------------------------------------------------------------------------------------- 5. determinism
def test_dlogits_is_bit_identical_from_run_to_run():
    """The captured step's form (bf16 rows of pitch 16, no probability map): two forwards agree to 1e-5 relative in the atomically folded
    sums; two backwards from the same sums agree bit for bit."""
    from transception_amd._lib import lib
    L, st = lib(), _stream()
    ncls, ld = 9, 16
    g = torch.Generator().manual_seed(71)
    tok = (torch.randn(B * HW, ld, generator=g) * 2.0).to(DEV).to(torch.bfloat16)
    lab = _labels((B, HW), ncls, g, 0.2).to(DEV)
    wdev = _wdev(_weights(ncls, g), _weights(ncls, g), ncls)
    sums, outs = [], []
    for _ in range(2):
        s = torch.zeros(1 + 3 * ncls, device=DEV)
        L.tc_seg_loss_fwd_ft(tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, 2.0, TVERSKY, None, s.data_ptr(), B, ncls, HW, 1, st)
        sums.append(s)
    for _ in range(2):
        d = torch.full((B * HW, ld), 3.0, device=DEV, dtype=torch.bfloat16)
        L.tc_seg_loss_bwd_ft(None, tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, sums[0].data_ptr(), d.data_ptr(), ld, B, ncls, HW, 0.4, 0.6,
                             2.0, TVERSKY, 0.3, 0.7, 1024.0, None, 1, st)
        outs.append(d)
    torch.cuda.synchronize()
    assert float(((sums[0] - sums[1]).abs() / (sums[0].abs() + 1e-6)).max()) < 1e-5
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)) and float(outs[0].float().abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- 6. routing
FT_ENTRIES = ("tc_seg_loss_fwd_ft", "tc_seg_loss_value_ft", "tc_seg_loss_bwd_ft")


def _count_ft(monkeypatch):
    """{entry: calls}, counted through wrappers on the loaded library object's attributes"""
    from transception_amd._lib import lib
    L, n = lib(), {name: 0 for name in FT_ENTRIES}
    for name in FT_ENTRIES:
        def counted(*a, _real=getattr(L, name), _name=name):
            n[_name] += 1
            return _real(*a)
        monkeypatch.setattr(L, name, counted)
    return n


def test_seg_loss_routes(monkeypatch):
    """SegLoss() and SegLoss(focal_gamma=0.0, overlap="dice") never reach the new entries and give bit-equal dlogits; focal_gamma=2 goes
    through them, differs from the plain loss by more than 1e-3 and matches the reference.  The bit-equality is asked at 11 x 11 as well
    as at 37 x 29: two evaluations are two forwards, whose sums are folded with one atomic add per workgroup in arrival order, so from five
    workgroups they -- and the gradient formed from them -- may differ in the last bits between ANY two runs of the same loss (measured:
    they do); B HW = 242 is one workgroup, one addend per element, and there the comparison is an equality.  At 37 x 29 the two are held
    to 1e-5 of the largest gradient, the bound the sums themselves are held to."""
    from transception_amd.train import SegLoss
    ncls, H, W = 9, 37, 29
    g = torch.Generator().manual_seed(81)
    logits = torch.randn(B, ncls, H, W, generator=g) * 2.0
    lab = torch.randint(0, ncls, (B, H, W), generator=g)
    calls = _count_ft(monkeypatch)

    def run(lf, logits=logits, lab=lab):
        x = logits.to(DEV).requires_grad_()
        out = lf(x, lab.to(DEV))
        out[0].backward()
        return [float(t.detach()) for t in out], x.grad

    small = (logits[:, :, :11, :11].contiguous(), lab[:, :11, :11].contiguous())
    d1, d2 = run(SegLoss(ncls), *small)[1], run(SegLoss(ncls, focal_gamma=0.0, overlap="dice"), *small)[1]
    assert torch.equal(d1, d2) and float(d1.abs().max()) > 0.0
    plain, dplain = run(SegLoss(ncls))
    same, dsame = run(SegLoss(ncls, focal_gamma=0.0, overlap="dice"))
    assert calls == {name: 0 for name in FT_ENTRIES}
    assert abs(plain[0] - same[0]) < 2e-6 and float((dplain - dsame).abs().max()) <= 1e-5 * float(dplain.abs().max())
    assert SegLoss(ncls)._route(DEV) is None and SegLoss(ncls, focal_gamma=0.0, overlap="dice")._route(DEV) is None
    focal, dfocal = run(SegLoss(ncls, focal_gamma=2.0))
    assert calls == {"tc_seg_loss_fwd_ft": 1, "tc_seg_loss_value_ft": 0, "tc_seg_loss_bwd_ft": 1}      # Dice: the value entry of the weighted loss
    assert abs(focal[0] - plain[0]) > 1e-3 and abs(focal[2] - plain[2]) < 2e-6            # the Dice term is the same
    want = reference(logits.view(B, ncls, H * W), lab.view(B, H * W), gamma=2.0)
    check_scalars(focal, want, "SegLoss(focal_gamma=2)")
    check_grad(dfocal.view(B, ncls, H * W), want, "SegLoss(focal_gamma=2)")
    tv, dtv = run(SegLoss(ncls, overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7, ignore_index=II))
    want = reference(logits.view(B, ncls, H * W), lab.view(B, H * W), None, None, II, 0.0, "tversky", 0.3, 0.7)
    check_scalars(tv, want, "SegLoss(overlap=tversky)")
    check_grad(dtv.view(B, ncls, H * W), want, "SegLoss(overlap=tversky)")
    assert calls == {"tc_seg_loss_fwd_ft": 2, "tc_seg_loss_value_ft": 1, "tc_seg_loss_bwd_ft": 2}


# ---------------------------------------------------------------------------------------------------------------- 7. the gradient scale
def test_gradient_scale_from_device_memory():
    """fp32 NCHW: a gscale_dev word of 512 with gscale = 0.5 scales dlogits by 256 exactly.  Both backwards read the sums and the
    probabilities of ONE forward: a second forward's atomically folded sums may differ in the last bits."""
    from transception_amd._lib import lib
    L, st = lib(), _stream()
    ncls = 9
    vals, vdev, full, part, w_ce, w_dice = _inputs(ncls)
    lab, wdev = part.to(DEV), _wdev(w_ce, w_dice, ncls)
    word = torch.tensor([512.0], device=DEV)
    _, sums, prob, base = run_nchw(vdev, lab, wdev, II, 2.0, "tversky", 0.3, 0.7)
    out = []
    for gscale, dev in ((1.0, None), (0.5, word)):
        d = torch.full((B, ncls, HW), 7.0, device=DEV)
        L.tc_seg_loss_bwd_ft(prob.data_ptr(), None, 0, lab.data_ptr(), wdev.data_ptr(), II, sums.data_ptr(), d.data_ptr(), 0, B, ncls, HW, 0.4, 0.6,
                             2.0, TVERSKY, 0.3, 0.7, gscale, _ptr(dev), 0, st)
        out.append(d)
    torch.cuda.synchronize()
    assert torch.equal(out[0], base) and torch.equal(out[1], out[0] * 256.0) and float(base.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- 8. the step
def _step_inputs():
    from test_weighted_loss_gpu import BATCH, SIZE
    from transception_amd.seeded_init import seeded_input, seeded_labels
    x = torch.from_numpy(seeded_input(BATCH, size=SIZE)).to(DEV)
    lab = torch.from_numpy(seeded_labels(BATCH, size=SIZE))
    lab[:, :20, :] = II                                                            # an unlabelled margin: 31 % of the pixels
    return x, lab.to(DEV)


CW = (0.5, 1.0, 2.0, 0.0, 4.0, 0.25, 1.5, 3.0, 1.0)
FT = dict(focal_gamma=2.0, overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7)


def test_captured_step_follows_the_eager_step(monkeypatch):
    """fp32 model, 64 x 64, B = 2, class weights and ignore_index with focal_gamma = 2 and Tversky(0.3, 0.7): three replayed steps follow
    three eager train_steps from the same state within the class-weighted test's 5e-4 on the loss, through the new entries (token-major,
    no probability map); the first loss differs from the default loss's by more than 1e-3."""
    from test_weighted_loss_gpu import _fresh
    from transception_amd.train import FusedSGD, GraphedStep, SegLoss, train_step
    x, lab = _step_inputs()
    me, mg, md = _fresh(), _fresh(), _fresh()
    oe, og, od = FusedSGD(me, lr=0.05), FusedSGD(mg, lr=0.05), FusedSGD(md, lr=0.05)
    le, lg = (SegLoss(9, ce_weight=CW, dice_weight=CW, ignore_index=II, **FT) for _ in range(2))
    default = train_step(md, SegLoss(9, ce_weight=CW, dice_weight=CW, ignore_index=II), od, x, lab)[0].item()
    first = train_step(me, le, oe, x, lab)[0].item()
    assert math.isfinite(first) and abs(first - default) > 1e-3, (first, default)
    train_step(me, le, oe, x, lab)                                                 # as many steps as the capture's warm-up takes
    calls = _count_ft(monkeypatch)
    step = GraphedStep(mg, lg, og, x, lab, None, warmup=2)
    assert calls == {name: 3 for name in FT_ENTRIES}                               # two warm-up steps and the capture
    for i in range(3):
        a = [t.item() for t in train_step(me, le, oe, x, lab)]
        b = [t.item() for t in step()]
        print(f"step {i}: eager {a}, replayed {b}")
        assert all(math.isfinite(v) for v in b)
        assert abs(a[0] - b[0]) < 5e-4, (a, b)
    assert bool(torch.isfinite(mg.flat_parameters()).all())


def test_captured_step_under_a_dynamic_loss_scale():
    """float16 storage, DynamicLossScale(4096), the same options.  Three models from the same state take one eager step each (the
    optimiser state exists, "first step" is not what gets captured): an eager twin and the captured one with the options, and one with the
    default overlap and exponent.  Then one more step: the replayed one follows the eager twin's within the 5e-4 of the fp32 comparison on
    the loss (both read the same float16 logits; the two models differ by the order of the weight-gradient atomics of one step, a float16
    unit in the last place of some weights) and differs from the default run's by more than 1e-3; nothing is skipped and the scale stays
    4096.  The loss of a step does not see that step's gradient, so the update is compared too: the replayed step's parameter change
    against the eager twin's, relative l2 difference below 0.05 -- float16 gradients carry 2^-11 per element, which the backward sweep
    and the atomics' order compound to the order of 1e-2, while a gradient scale handed over wrongly (taken twice, or not at all:
    a factor of 4096) moves the ratio to 1 or beyond.  Measured on the MI355X: the three scalars within 1.1e-5, relative l2 difference 1.7e-3."""
    from test_loss_scale_gpu import _fresh
    from transception_amd.train import DynamicLossScale, FusedSGD, GraphedStep, SegLoss, train_step
    x, lab = _step_inputs()
    base = dict(ce_weight=CW, dice_weight=CW, ignore_index=II)
    runs = {}
    for name, kw in (("eager", FT), ("graphed", FT), ("default", {})):
        m = _fresh(torch.float16)
        scaler = DynamicLossScale(init_scale=4096.0)
        lf, opt = SegLoss(9, loss_scale=scaler, **base, **kw), FusedSGD(m, lr=0.05)
        first = [t.item() for t in train_step(m, lf, opt, x, lab)]
        assert all(math.isfinite(v) for v in first) and not opt.last_step_skipped(), (name, first)
        runs[name] = (m, lf, opt, scaler)
    m, lf, opt, _ = runs["graphed"]
    step = GraphedStep(m, lf, opt, x, lab, None, warmup=0)
    before = {k: runs[k][0].flat_parameters().clone() for k in ("eager", "graphed")}
    b = [t.item() for t in step()]
    a = [t.item() for t in train_step(*runs["eager"][:3], x, lab)]
    d = [t.item() for t in train_step(*runs["default"][:3], x, lab)]
    print(f"second step: eager {a}, replayed {b}, default loss {d}")
    assert all(math.isfinite(v) for v in a + b + d)
    assert all(abs(u - v) < 5e-4 for u, v in zip(a, b)), (a, b)
    assert abs(b[0] - d[0]) > 1e-3 and abs(b[1] - d[1]) > 1e-3, (b, d)
    for k in ("eager", "graphed", "default"):
        assert not runs[k][2].last_step_skipped() and runs[k][3].state_dict() == {"scale": 4096.0, "growth_tracker": 2, "skipped": 0}, k
    de = (runs["eager"][0].flat_parameters() - before["eager"]).double()
    dg = (runs["graphed"][0].flat_parameters() - before["graphed"]).double()
    rel = float((dg - de).norm() / de.norm())
    print(f"parameter change of the second step: |eager| {float(de.norm()):.4e}, |replayed| {float(dg.norm()):.4e}, relative l2 difference {rel:.3e}")
    assert float(de.norm()) > 0.0 and bool(torch.isfinite(dg).all()) and rel < 0.05, rel


# ---------------------------------------------------------------------------------------------------------------- 9. the trainer
def test_trainer_hands_the_options_to_the_loss(tmp_path, monkeypatch):
    """trainer_synapse for one epoch with the options set through TrainConfig: the second and third scalar of the first log line are the
    focal CE and the Tversky term of the first batch, as a direct SegLoss evaluation on an identical model gives them."""
    from test_weighted_loss_gpu import _fresh
    from transception_amd import data as D
    from transception_amd import trainer as T
    from transception_amd.train import SegLoss
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=1, slices_per_case=4, size=64, seed=2)
    cfg = T.TrainConfig(root_path=base, list_dir=lists, max_epochs=1, batch_size=2, img_size=64, seed=5, model_name="tiny", class_weights=CW,
                        ignore_index=II, **FT)
    batches = []
    real = T.train_step

    def spy(model, loss_fn, opt, x, y, group=None):
        batches.append((x.clone(), y.clone()))
        assert (loss_fn.focal_gamma, loss_fn.overlap, loss_fn.tversky_alpha, loss_fn.tversky_beta) == (2.0, "tversky", 0.3, 0.7)
        return real(model, loss_fn, opt, x, y, group)

    monkeypatch.setattr(T, "train_step", spy)
    lines = []
    hist = T.trainer_synapse(cfg, _fresh(), str(tmp_path / "snap"), log=lines.append)
    assert hist["iterations"] == 2 and all(math.isfinite(v) for v in hist["loss"])
    first = next(l for l in lines if l.startswith("iteration 1 "))
    logged = [float(v) for v in re.search(r"loss : (\S+), loss_ce: (\S+), loss_dice: (\S+)", first).groups()]
    x, y = batches[0]
    with torch.no_grad():
        got = SegLoss(9, ce_weight=CW, dice_weight=CW, ignore_index=II, **FT)(_fresh()(x), y)
    got = [float(t) for t in got]
    print(f"logged {logged}, direct {got}")
    assert all(abs(a - b) < 2e-6 for a, b in zip(logged, got)), (logged, got)
    assert abs(got[0] - (0.4 * got[1] + 0.6 * got[2])) < 2e-6

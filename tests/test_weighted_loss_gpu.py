"""The class-weighted loss with ignore_index on the MI355X: SegLoss(ce_weight, dice_weight, ignore_index) and the tc_seg_loss_*_w entries
against a CPU fp64 autograd reference written here --

  CE   = F.cross_entropy(logits64, labels, weight=w, ignore_index=ii)
  Dice = the expression of tests/test_ops_gpu.py::test_seg_loss_and_sgd with a valid-pixel mask on both p and the one-hot and
         dice_weight inside the class sum

-- on NCHW and token-major logits, fp32 / bf16 / fp16 storage, with and without the probability map, with the dynamic loss scale, and
inside the captured step.  Bounds against fp64 are those of test_seg_loss_and_sgd: 2e-6 absolute on the three scalars, 1e-8 + 1e-4 |ref|
on the gradients.  Random cases ignore at most half of the pixels and draw weights from [0.25, 4] with exactly one class at weight 0."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
II = 255
OFF = -2 ** 31                                  # TC_IGNORE_NONE
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _weights(ncls, g, zero_at=None):
    """[0.25, 4] with exactly one class at weight 0."""
    w = 0.25 + 3.75 * torch.rand(ncls, generator=g, dtype=torch.float64)
    w[int(torch.randint(0, ncls, (1,), generator=g)) if zero_at is None else zero_at] = 0.0
    return w


def _labels(shape, ncls, g, frac):
    """Random labels with a fraction `frac` <= 0.5 of the pixels set to the ignored value."""
    assert frac <= 0.5
    lab = torch.randint(0, ncls, shape, generator=g)
    n = lab.numel()
    idx = torch.randperm(n, generator=g)[:int(frac * n)]
    lab.view(-1)[idx] = II
    return lab


def reference(logits, labels, w_ce, w_dice, ii):
    """fp64 autograd on the CPU.  logits [B, C, HW] (any float type, widened), labels [B, HW]; w_ce / w_dice fp64 or None; ii or None.
    Returns (loss, ce, dice, dlogits [B, C, HW]) for loss = 0.4 CE + 0.6 Dice."""
    x = logits.detach().double().cpu().clone().requires_grad_()
    labels = labels.cpu()
    ncls = x.shape[1]
    ce = F.cross_entropy(x, labels, weight=w_ce, ignore_index=-100 if ii is None else ii)
    valid = torch.ones_like(labels, dtype=torch.bool) if ii is None else labels != ii
    p = torch.softmax(x, 1) * valid[:, None]
    oh = F.one_hot(torch.where(valid, labels, torch.zeros_like(labels)), ncls).permute(0, 2, 1).double() * valid[:, None]
    inter, ys, zs = (p * oh).sum((0, 2)), oh.sum((0, 2)), (p * p).sum((0, 2))
    wd = torch.ones(ncls, dtype=torch.float64) if w_dice is None else w_dice
    dice = (wd * (1 - (2 * inter + 1e-5) / (zs + ys + 1e-5))).sum() / ncls
    loss = 0.4 * ce + 0.6 * dice
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all()), "the reference itself is not finite for this seed"
    return loss.item(), ce.item(), dice.item(), x.grad


def check_scalars(got, want, what):
    errs = [abs(float(a.detach()) - b) for a, b in zip(got, want)]
    print(f"{what}: |loss, ce, dice - fp64| = {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}")
    assert max(errs) < 2e-6, (what, [float(a.detach()) for a in got], want)


def check_grad(got, want, what):
    got, want = got.detach().double().cpu(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    tol = 1e-8 + 1e-4 * want.abs()
    print(f"{what}: max |dlogits - fp64| = {err.max().item():.3e} (ref max {want.abs().max().item():.3e}), worst err / tol = {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all()), f"{what}: max err {err.max().item():.3e}, worst err / tol {(err / tol).max().item():.3f}"


def _wdev(w_ce, w_dice, ncls):
    ones = torch.ones(ncls, dtype=torch.float64)
    return torch.cat([ones if w_ce is None else w_ce, ones if w_dice is None else w_dice]).float().to(DEV)


def run_nchw(vals, lab, wdev, ii, gscale=1.0):
    """The _w entries on fp32 NCHW values [B, C, HW] (ld = 0): (loss3, sums, prob, dlogits [B, C, HW])."""
    from transception_amd._lib import lib
    L, st = lib(), _stream()
    B, C, HW = vals.shape
    prob = torch.empty(B, C, HW, device=DEV)
    sums = torch.zeros(1 + 3 * C, device=DEV)
    out3 = torch.empty(3, device=DEV)
    d = torch.full((B, C, HW), 7.0, device=DEV)                                    # a sentinel: every element must be written
    wp = None if wdev is None else wdev.data_ptr()
    L.tc_seg_loss_fwd_w(vals.data_ptr(), 0, lab.data_ptr(), wp, ii, prob.data_ptr(), sums.data_ptr(), B, C, HW, 0, st)
    L.tc_seg_loss_value_w(sums.data_ptr(), wp, C, 0.4, 0.6, out3.data_ptr(), st)
    L.tc_seg_loss_bwd_w(prob.data_ptr(), None, 0, lab.data_ptr(), wp, ii, sums.data_ptr(), d.data_ptr(), 0, B, C, HW, 0.4, 0.6, gscale, None, 0, st)
    torch.cuda.synchronize()
    return out3.cpu(), sums, prob, d


# ---------------------------------------------------------------------------------------------------------------- 1. through SegLoss, NCHW fp32
@pytest.mark.parametrize("setting", ["ce_weight", "dice_weight", "ignore_index", "all"])
def test_seg_loss_module_matches_fp64_reference(setting):
    """SegLoss on NCHW fp32 logits, B = 2, 9 classes, 32 x 32: loss, CE, Dice and dlogits against the fp64 reference."""
    from transception_amd.train import SegLoss
    B, ncls, H = 2, 9, 32
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(B, ncls, H, H, generator=g) * 2.0
    w_ce = _weights(ncls, g) if setting in ("ce_weight", "all") else None
    w_dice = _weights(ncls, g) if setting in ("dice_weight", "all") else None
    ii = II if setting in ("ignore_index", "all") else None
    lab = _labels((B, H, H), ncls, g, 0.4 if ii is not None else 0.0)
    want = reference(logits.view(B, ncls, H * H), lab.view(B, H * H), w_ce, w_dice, ii)
    lf = SegLoss(ncls, ce_weight=None if w_ce is None else w_ce.tolist(), dice_weight=None if w_dice is None else w_dice.tolist(),
                 ignore_index=ii)
    ld = logits.to(DEV).requires_grad_()
    got = lf(ld, lab.to(DEV))
    check_scalars(got, want[:3], setting)
    got[0].backward()
    check_grad(ld.grad.view(B, ncls, H * H), want[3], setting)
    if ii is not None:
        ign = (lab == II).view(B, 1, H, H).expand(B, ncls, H, H)
        assert bool((ld.grad.cpu()[ign] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 2. the raw entries, token-major
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("ncls", [2, 9, 16])
def test_token_major_entries(ncls, padded, dtype):
    """tc_seg_loss_fwd_w / _bwd_w on token-major logits [B*HW, ld], B = 3, HW = 70 (a tail inside a wave and inside a 256-thread block),
    ld = 16 (16-byte padded rows; 16 classes fill two pieces) or ncls + 3 (element by element), with the probability map and without it
    (the backward then recomputes the softmax).  The fp32 result -- the same entries on the NCHW fp32 copy of the SAME stored values --
    is held against the fp64 reference; dlogits in the storage type must equal that fp32 result rounded to the storage type bit for bit,
    the probabilities must be equal bit for bit, pad columns come back zero on the 16-byte path (up to the multiple of 8 classes its pieces
    cover) and untouched otherwise, and ignored pixels get exact zeros."""
    from transception_amd._lib import lib
    L, st = lib(), _stream()
    B, HW = 3, 70
    ld = 16 if padded else ncls + 3
    code = CODE[dtype]
    g = torch.Generator().manual_seed(100 * ncls + 10 * padded + code)
    buf = (torch.randn(B * HW, ld, generator=g) * 2.0).to(DEV).to(dtype)
    tok = buf[:, :ncls]
    w_ce, w_dice = _weights(ncls, g), _weights(ncls, g)
    lab_c = _labels((B, HW), ncls, g, 0.3)
    lab, wdev = lab_c.to(DEV), _wdev(w_ce, w_dice, ncls)
    nchw = tok.float().view(B, HW, ncls).permute(0, 2, 1).contiguous()             # the stored values, widened
    want = reference(nchw, lab_c, w_ce, w_dice, II)
    out3, sa, pa, da = run_nchw(nchw, lab, wdev, II, gscale=128.0)
    what = f"ncls {ncls} ld {ld} {dtype}"
    check_scalars(out3, want[:3], what)
    check_grad(da / 128.0, want[3], what)                                          # (a power of two: the scale is exact)
    want_tok = da.permute(0, 2, 1).reshape(B * HW, ncls).to(dtype)
    ign = (lab == II).view(-1)
    assert bool(ign.any()) and bool((want_tok[ign] == 0).all())
    # the 16-byte path writes whole pieces up to the next multiple of 8 classes: those pad columns are zeros; columns beyond them (2 classes in
    # rows of pitch 16: 8 .. 15) and every pad column of the element-by-element path are not touched
    pad8 = (ncls + 7) // 8 * 8 if (dtype != torch.float32 and ld % 8 == 0) else ncls
    # with the probability map
    pb, sb = torch.empty(B, ncls, HW, device=DEV), torch.zeros(1 + 3 * ncls, device=DEV)
    L.tc_seg_loss_fwd_w(tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, pb.data_ptr(), sb.data_ptr(), B, ncls, HW, code, st)
    db = torch.full((B * HW, ld), 3.0, device=DEV, dtype=dtype)
    L.tc_seg_loss_bwd_w(pb.data_ptr(), None, 0, lab.data_ptr(), wdev.data_ptr(), II, sa.data_ptr(), db.data_ptr(), ld, B, ncls, HW, 0.4, 0.6,
                        128.0, None, code, st)
    # without it: sums only, the softmax recomputed from the logits
    sc = torch.zeros(1 + 3 * ncls, device=DEV)
    L.tc_seg_loss_fwd_w(tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, None, sc.data_ptr(), B, ncls, HW, code, st)
    dc = torch.full((B * HW, ld), 3.0, device=DEV, dtype=dtype)
    L.tc_seg_loss_bwd_w(None, tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, sa.data_ptr(), dc.data_ptr(), ld, B, ncls, HW, 0.4, 0.6,
                        128.0, None, code, st)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb)                                                     # ignored pixels write their probabilities too
    for s in (sb, sc):
        assert float(((sa - s).abs() / (sa.abs() + 1e-6)).max()) < 1e-5
    for d, mode in ((db, "prob"), (dc, "recompute")):
        assert torch.equal(d[:, :ncls], want_tok), (what, mode, float((d[:, :ncls].float() - want_tok.float()).abs().max()))
        assert bool((d[:, ncls:pad8] == 0.0).all()) and bool((d[:, pad8:] == 3.0).all()), (what, mode)


# ---------------------------------------------------------------------------------------------------------------- 3. structure cases
def _structure_labels(case, B, HW, ncls, g):
    if case == "image_ignored":
        lab = _labels((B, HW), ncls, g, 0.1)
        lab[1] = II
    elif case == "class_absent":
        lab = _labels((B, HW), ncls, g, 0.1)
        lab[lab == 4] = 5
    else:
        lab = torch.full((B, HW), II)
    return lab


@pytest.mark.parametrize("case", ["image_ignored", "class_absent", "all_ignored"])
def test_structure_cases(case):
    """B = 3, HW = 70, 9 classes: one whole image ignored; one class absent from the labels (Y_k = 0); every pixel ignored (loss 0, CE 0,
    a finite Dice, every gradient exactly 0 -- torch's CE is NaN there).  fp32 NCHW against the fp64 reference, and the captured step's
    form (bf16 rows padded to 16, no probability map) for the zeros: dlogits, filled with a sentinel first, is exactly 0 at every
    ignored pixel."""
    from transception_amd._lib import lib
    L, st = lib(), _stream()
    B, HW, ncls = 3, 70, 9
    g = torch.Generator().manual_seed(31)
    vals = torch.randn(B, ncls, HW, generator=g) * 2.0
    w_ce, w_dice = _weights(ncls, g, zero_at=2), _weights(ncls, g, zero_at=7)
    lab_c = _structure_labels(case, B, HW, ncls, g)
    assert (case != "class_absent") or not bool((lab_c == 4).any())
    lab, wdev = lab_c.to(DEV), _wdev(w_ce, w_dice, ncls)
    out3, sums, prob, d = run_nchw(vals.to(DEV), lab, wdev, II)
    ign = (lab_c == II)
    assert bool(ign.any())
    if case == "all_ignored":
        assert float(out3[0]) == 0.0 and float(out3[1]) == 0.0 and math.isfinite(float(out3[2]))
        assert bool((d == 0).all())
    else:
        want = reference(vals, lab_c, w_ce, w_dice, II)
        check_scalars(out3, want[:3], case)
        check_grad(d, want[3], case)
        if case == "class_absent":
            assert float(sums[2 + 3 * 4]) == 0.0
    assert bool((d.cpu().permute(0, 2, 1)[ign] == 0).all()) and not bool((d == 7.0).any())
    # bf16 token rows of pitch 16, softmax recomputed, a dynamic-scale sized gscale: zeros stay zeros, the rest is finite
    tok = torch.zeros(B * HW, 16, device=DEV, dtype=torch.bfloat16)
    tok[:, :ncls] = vals.permute(0, 2, 1).reshape(B * HW, ncls).to(DEV)
    s2 = torch.zeros(1 + 3 * ncls, device=DEV)
    d2 = torch.full((B * HW, 16), 7.0, device=DEV, dtype=torch.bfloat16)
    L.tc_seg_loss_fwd_w(tok.data_ptr(), 16, lab.data_ptr(), wdev.data_ptr(), II, None, s2.data_ptr(), B, ncls, HW, 1, st)
    L.tc_seg_loss_bwd_w(None, tok.data_ptr(), 16, lab.data_ptr(), wdev.data_ptr(), II, s2.data_ptr(), d2.data_ptr(), 16, B, ncls, HW, 0.4, 0.6,
                        65536.0, None, 1, st)
    torch.cuda.synchronize()
    assert bool((d2[ign.view(-1).to(DEV)] == 0).all()) and bool((d2[:, ncls:] == 0).all()) and bool(torch.isfinite(d2.float()).all())
    if case != "all_ignored":
        assert float(d2[~ign.view(-1).to(DEV)][:, :ncls].float().abs().max()) > 0.0
    else:
        assert bool((d2 == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 4. neutral settings
@pytest.mark.parametrize("null_weights", [False, True])
def test_neutral_settings_are_the_plain_kernels(null_weights):
    """All-ones weights (as a tensor and as the NULL pointer) and no ignore_index through the _w entries: dlogits and prob bit-equal to
    the plain entries', the atomically accumulated sums within the 1e-5 relative the token-major test allows.  NCHW fp32, and token-major
    bf16 at ld = 16 with and without the probability map.  B = 3, 24 x 24: seven workgroups."""
    from transception_amd._lib import lib
    L, st = lib(), _stream()
    B, ncls, HW, ld = 3, 9, 576, 16
    g = torch.Generator().manual_seed(41)
    wp = None if null_weights else torch.ones(2 * ncls, device=DEV)
    wptr = None if wp is None else wp.data_ptr()
    npix = float(B * HW)
    lab = torch.randint(0, ncls, (B, HW), generator=g).to(DEV)
    # NCHW fp32
    x = (torch.randn(B, ncls, HW, generator=g) * 2.0).to(DEV)
    pa, pb = torch.empty(B, ncls, HW, device=DEV), torch.empty(B, ncls, HW, device=DEV)
    sa, sb = torch.zeros(1 + 3 * ncls, device=DEV), torch.zeros(1 + 3 * ncls, device=DEV)
    da, db = torch.empty(B, ncls, HW, device=DEV), torch.empty(B, ncls, HW, device=DEV)
    oa, ob = torch.empty(3, device=DEV), torch.empty(3, device=DEV)
    L.tc_seg_loss_fwd(x.data_ptr(), lab.data_ptr(), pa.data_ptr(), sa.data_ptr(), B, ncls, HW, 0, st)
    L.tc_seg_loss_fwd_w(x.data_ptr(), 0, lab.data_ptr(), wptr, OFF, pb.data_ptr(), sb.data_ptr(), B, ncls, HW, 0, st)
    L.tc_seg_loss_value(sa.data_ptr(), ncls, npix, 0.4, 0.6, oa.data_ptr(), st)
    L.tc_seg_loss_value_w(sa.data_ptr(), wptr, ncls, 0.4, 0.6, ob.data_ptr(), st)
    L.tc_seg_loss_bwd(pa.data_ptr(), lab.data_ptr(), sa.data_ptr(), da.data_ptr(), B, ncls, HW, 0.4, 0.6, npix, 128.0, None, 0, st)
    L.tc_seg_loss_bwd_w(pa.data_ptr(), None, 0, lab.data_ptr(), wptr, OFF, sa.data_ptr(), db.data_ptr(), 0, B, ncls, HW, 0.4, 0.6, 128.0, None, 0, st)
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(da, db)
    assert float(((sa - sb).abs() / (sa.abs() + 1e-6)).max()) < 1e-5
    assert torch.equal(oa, ob)                                                     # same sums in, same double arithmetic
    # token-major bf16, rows padded to 16
    tok = (torch.randn(B * HW, ld, generator=g) * 2.0).to(DEV).to(torch.bfloat16)
    for with_prob in (True, False):
        qa, qb = torch.zeros(B, ncls, HW, device=DEV), torch.zeros(B, ncls, HW, device=DEV)
        ta, tb = torch.zeros(1 + 3 * ncls, device=DEV), torch.zeros(1 + 3 * ncls, device=DEV)
        ea, eb = (torch.full((B * HW, ld), 3.0, device=DEV, dtype=torch.bfloat16) for _ in range(2))
        L.tc_seg_loss_fwd_tok(tok.data_ptr(), ld, lab.data_ptr(), qa.data_ptr() if with_prob else None, ta.data_ptr(), B, ncls, HW, 1, st)
        L.tc_seg_loss_fwd_w(tok.data_ptr(), ld, lab.data_ptr(), wptr, OFF, qb.data_ptr() if with_prob else None, tb.data_ptr(), B, ncls, HW, 1, st)
        pr = qa.data_ptr() if with_prob else None
        lg = None if with_prob else tok.data_ptr()
        L.tc_seg_loss_bwd_tok(pr, lg, ld, lab.data_ptr(), ta.data_ptr(), ea.data_ptr(), ld, B, ncls, HW, 0.4, 0.6, npix, 128.0, None, 1, st)
        L.tc_seg_loss_bwd_w(pr, lg, ld, lab.data_ptr(), wptr, OFF, ta.data_ptr(), eb.data_ptr(), ld, B, ncls, HW, 0.4, 0.6, 128.0, None, 1, st)
        torch.cuda.synchronize()
        assert torch.equal(qa, qb) and torch.equal(ea.view(torch.int16), eb.view(torch.int16)), with_prob
        assert float(((ta - tb).abs() / (ta.abs() + 1e-6)).max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------- 5. the loss scale
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("padded", [True, False])
def test_weighted_gradient_scaled_from_device_memory(padded, dtype):
    """tc_seg_loss_bwd_w, B = 1, HW = 70, weights and ignored pixels: gscale = 1 with gscale_dev -> 512 (word 0 of a loss-scale state) is
    bit-equal to gscale = 512 with a null pointer, on 16-byte-padded and on unpadded token rows."""
    from transception_amd._lib import lib
    from transception_amd.train import DynamicLossScale
    L, HW, ncls = lib(), 70, 9
    ld = 16 if padded else ncls
    g = torch.Generator().manual_seed(50 + padded)
    logits = torch.randn(HW, ld, generator=g).to(device=DEV, dtype=dtype)
    labels = _labels((1, HW), ncls, g, 0.3).to(DEV)
    wdev = _wdev(_weights(ncls, g), _weights(ncls, g), ncls)
    sums = torch.zeros(1 + 3 * ncls, dtype=torch.float32, device=DEV)
    tc = CODE[dtype]
    L.tc_seg_loss_fwd_w(logits.data_ptr(), ld, labels.data_ptr(), wdev.data_ptr(), II, None, sums.data_ptr(), 1, ncls, HW, tc, _stream())
    state = DynamicLossScale(init_scale=512.0).state(DEV)
    out = []
    for gscale, dev in ((1.0, state.data_ptr()), (512.0, None)):
        d = torch.zeros(HW, ld, dtype=dtype, device=DEV)
        L.tc_seg_loss_bwd_w(None, logits.data_ptr(), ld, labels.data_ptr(), wdev.data_ptr(), II, sums.data_ptr(), d.data_ptr(), ld, 1, ncls, HW,
                            0.4, 0.6, gscale, dev, tc, _stream())
        out.append(d)
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int16), out[1].view(torch.int16))
    assert bool(torch.isfinite(out[0].float()).all()) and float(out[0][:, :ncls].float().abs().max()) > 0.5       # scaled: 512 * O(1e-2)
    assert bool((out[0][(labels == II).view(-1)] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 6. the captured step
SIZE, BATCH = 64, 2
_SD = None


def _fresh():
    from transception_amd import MSTransception
    from transception_amd.seeded_init import seeded_state_dict
    global _SD
    if _SD is None:
        _SD = seeded_state_dict()
    m = MSTransception(num_classes=9)
    m.load_state_dict(_SD, strict=True)
    m.to(DEV)
    m.set_compute_dtype(torch.float32)
    return m.train()


@pytest.mark.parametrize("split", [False, True])
def test_captured_step_with_class_weights_and_ignore_index(split):
    """fp32 model, 64 x 64, B = 2 (the size of the graphed-against-eager trainer comparison of tests/test_trainer_gpu.py), class weights
    and ignore_index set: three replayed steps follow three eager train_steps from the same state within that comparison's 5e-4 on the
    loss, as one graph and in the split (multi-GPU) form.  Then, with the learning rate at 0 so that replays repeat, the loss's weight
    tensor is filled IN PLACE with new values: the next replay's loss changes -- the graph holds the tensor's address, not its values."""
    from transception_amd.seeded_init import seeded_input, seeded_labels
    from transception_amd.train import FusedSGD, GraphedStep, SegLoss, train_step
    x = torch.from_numpy(seeded_input(BATCH, size=SIZE)).to(DEV)
    lab = torch.from_numpy(seeded_labels(BATCH, size=SIZE))
    lab[:, :20, :] = II                                                            # an unlabelled margin: 31 % of the pixels
    lab = lab.to(DEV)
    cw = (0.5, 1.0, 2.0, 0.0, 4.0, 0.25, 1.5, 3.0, 1.0)
    me, mg = _fresh(), _fresh()
    oe, og = FusedSGD(me, lr=0.05), FusedSGD(mg, lr=0.05)
    le, lg = (SegLoss(9, ce_weight=cw, dice_weight=cw, ignore_index=II) for _ in range(2))
    for _ in range(2):                                                             # as many steps as the capture's warm-up takes
        train_step(me, le, oe, x, lab)
    step = GraphedStep(mg, lg, og, x, lab, None, warmup=2, force_split=split)
    for i in range(3):
        a = [t.item() for t in train_step(me, le, oe, x, lab)]
        b = [t.item() for t in step()]
        print(f"step {i}: eager {a}, replayed {b}")
        assert all(math.isfinite(v) for v in b)
        assert abs(a[0] - b[0]) < 5e-4, (a, b)
    assert bool(torch.isfinite(mg.flat_parameters()).all())
    og.set_lr(0.0)
    step()                                                                         # (the momentum buffer moves, the weights no longer do)
    l1 = step()[0].item()
    l2 = step()[0].item()
    assert abs(l1 - l2) < 2e-5, (l1, l2)
    w = lg.weights(DEV)
    ptr = w.data_ptr()
    w.copy_(torch.tensor([3.0, 0.25, 0.5, 2.0, 0.25, 4.0, 1.0, 0.5, 2.0] * 2, device=DEV))
    assert lg.weights(DEV).data_ptr() == ptr
    l3 = step()[0].item()
    print(f"replays at lr 0: {l1} {l2}, after new weights in place: {l3}")
    assert math.isfinite(l3) and abs(l3 - l2) > 1e-3, (l2, l3)

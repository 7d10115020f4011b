"""Dynamic loss scaling for float16 storage (train.DynamicLossScale): the device-resident scale, the scaled SGD entry, the loss
backward reading the scale from device memory, and the whole of it in eager steps, in captured steps and in the trainer."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZE, BATCH = 64, 2


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


_SD = None


def _fresh(dtype=torch.float16):
    from transception_amd import MSTransception
    from transception_amd.seeded_init import seeded_state_dict
    global _SD
    if _SD is None:
        _SD = seeded_state_dict()
    m = MSTransception(num_classes=9)
    m.load_state_dict(_SD, strict=True)
    m.to(DEV)
    m.set_compute_dtype(dtype)
    return m.train()


def _batch():
    from transception_amd.seeded_init import seeded_input, seeded_labels
    return torch.from_numpy(seeded_input(BATCH, size=SIZE)).to(DEV), torch.from_numpy(seeded_labels(BATCH, size=SIZE)).to(DEV)


def _words(state):
    w = state.cpu()
    return [float(w[0]), float(w[1]), int(w.view(torch.int32)[2]), int(w.view(torch.int32)[3])]


# ---------------------------------------------------------------------------------------------------------------- 1. the update rule
def _rule(scale, tracker, skipped, ss, growth=2.0, backoff=0.5, interval=3, lo=2.0, hi=32.0):
    """torch.amp.GradScaler.update's rule with the two clamps, as the header states it."""
    if not math.isfinite(ss):
        return max(scale * backoff, lo), 0, skipped + 1
    tracker += 1
    if tracker == interval:
        return min(scale * growth, hi), 0, skipped
    return scale, tracker, skipped


def test_update_rule_matches_the_model_exactly():
    """interval 3, init 8, min 2, max 32: after every launch the four words equal the host model of the rule (every scale is a power of
    two, so scale and 1 / scale are exact).  The sequence grows to the upper clamp and stays there, grows directly after a backoff,
    backs off through inf and NaN down to the lower clamp and stays there, loses a half-built run of clean steps to an overflow, and
    grows again."""
    from transception_amd._lib import lib
    from transception_amd.train import DynamicLossScale
    F, I, N = 1.5, math.inf, math.nan
    seq = [F] * 3 + [0.0] * 3 + [F] * 3 + [F] * 3 + [I] + [3.0e38] * 3 + [N, I, I, N, I, N] + [F, F, I] + [F] * 3 + [F, N] + [F] * 6
    s = DynamicLossScale(init_scale=8.0, growth_interval=3, min_scale=2.0, max_scale=32.0)
    st = s.state(DEV)
    ss = torch.zeros(1, dtype=torch.float32, device=DEV)
    want, seen = (8.0, 0, 0), []
    assert _words(st) == [8.0, 0.125, 0, 0]
    for v in seq:
        ss.fill_(v)
        lib().tc_loss_scale_update(st.data_ptr(), ss.data_ptr(), 2.0, 0.5, 3, 2.0, 32.0, _stream())
        want = _rule(*want, v)
        seen.append(want[0])
        assert _words(st) == [want[0], 1.0 / want[0], want[1], want[2]], (len(seen), v, _words(st), want)
    # the sequence did what the docstring says (a property of the model, so of the test's own inputs)
    assert seen[8] == seen[11] == 32.0 and seen[12] == 16.0 and seen[15] == 32.0 and min(seen) == 2.0 and seen.count(2.0) >= 3
    assert want[2] == sum(not math.isfinite(v) for v in seq) == s.skipped() and s.value() == want[0]
    # the same through the class, and the argument rules of the entry
    s.update(ss.fill_(I))
    assert _words(st)[0] == max(want[0] * 0.5, 2.0) and _words(st)[3] == want[2] + 1
    from transception_amd._lib import TcError
    for bad in [(0.5, 0.5, 3, 2.0, 32.0), (2.0, 1.0, 3, 2.0, 32.0), (2.0, 0.0, 3, 2.0, 32.0), (2.0, 0.5, 0, 2.0, 32.0), (2.0, 0.5, 3, 0.0, 32.0),
                (2.0, 0.5, 3, 64.0, 32.0), (2.0, 0.5, 3, 2.0, I), (N, 0.5, 3, 2.0, 32.0)]:
        with pytest.raises(TcError, match="status -1"):
            lib().tc_loss_scale_update(st.data_ptr(), ss.data_ptr(), *bad, _stream())


# ---------------------------------------------------------------------------------------------------------------- 2. the scaled SGD entry
N_ARENA = 200
SEGS = [(0, 96), (104, 37)]            # a multiple of 8 elements (the 16-byte path) and an odd length (the scalar path)


@pytest.mark.parametrize("clip", [5.0, math.inf])
@pytest.mark.parametrize("lp_dtype", [None, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("first", [1, 0])
def test_scaled_sgd_is_the_static_one_at_a_power_of_two(first, lp_dtype, clip):
    """scale 1024: parameters, momentum and the 16-bit working copy after tc_sgd_step_multi_scaled are bit-equal to tc_sgd_step_multi with
    gscale = 1 / 1024 and clip_norm * 1024 (both products are exact).  The gradient's true norm is about 14, so clip = 5 is active.  A
    non-finite squared norm leaves all three buffers as they were; without clip_sumsq the entry refuses."""
    from transception_amd._lib import TC_BF16, TC_F16, TcError, lib
    from transception_amd.train import DynamicLossScale
    L = lib()
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(N_ARENA, generator=g).to(DEV)
    grad = (torch.randn(N_ARENA, generator=g) * 1024.0).to(DEV)
    buf0 = torch.randn(N_ARENA, generator=g).to(DEV)
    segs = torch.tensor([v for s in SEGS for v in s], dtype=torch.int64, device=DEV)
    ss = torch.zeros(1, dtype=torch.float32, device=DEV)
    L.tc_grad_sumsq(grad.data_ptr(), N_ARENA, ss.data_ptr(), _stream())
    assert clip == math.inf or math.sqrt(float(ss)) / 1024.0 > clip                     # the clip is active
    state = DynamicLossScale(init_scale=1024.0).state(DEV)
    tc = {None: 0, torch.bfloat16: TC_BF16, torch.float16: TC_F16}[lp_dtype]

    def run(scaled, sumsq=ss):
        p, buf = p0.clone(), buf0.clone()
        lp = p0.to(lp_dtype) if lp_dtype is not None else None
        lpp = lp.data_ptr() if lp is not None else None
        head = (p.data_ptr(), grad.data_ptr(), buf.data_ptr(), segs.data_ptr(), len(SEGS), max(n for _, n in SEGS), 0.05, None, 0.9, 1e-4)
        if scaled:
            L.tc_sgd_step_multi_scaled(*head, 1.0, first, sumsq.data_ptr() if sumsq is not None else None, clip, lpp, tc, state.data_ptr(),
                                       _stream())
        else:
            L.tc_sgd_step_multi(*head, 1.0 / 1024.0, first, sumsq.data_ptr(), clip * 1024.0, lpp, tc, _stream())
        torch.cuda.synchronize()
        return p, buf, lp

    a, b = run(True), run(False)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16),
                                                        y.view(torch.int32 if y.dtype == torch.float32 else torch.int16))
    live = torch.zeros(N_ARENA, dtype=torch.bool, device=DEV)
    for off, n in SEGS:
        live[off:off + n] = True
    assert bool((a[0] != p0)[live].all()) and torch.equal(a[0][~live], p0[~live]) and torch.equal(a[1][~live], buf0[~live])
    if lp_dtype is not None:
        assert torch.equal(a[2][live], a[0][live].to(lp_dtype)) and torch.equal(a[2][~live], p0.to(lp_dtype)[~live])
    for bad in (math.inf, math.nan):                                                      # the skip: nothing is touched
        p, buf, lp = run(True, torch.full((1,), bad, dtype=torch.float32, device=DEV))
        assert torch.equal(p, p0) and torch.equal(buf, buf0) and (lp is None or torch.equal(lp, p0.to(lp_dtype)))
    with pytest.raises(TcError, match="status -1"):
        run(True, None)


# ---------------------------------------------------------------------------------------------------------------- 3. the loss gradient
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("ncls", [9, 2])
def test_loss_gradient_scaled_from_device_memory(ncls, padded, dtype):
    """tc_seg_loss_bwd_tok, B = 1, HW = 70: gscale = 1 with gscale_dev -> 512 (word 0 of a loss-scale state) is bit-equal to
    gscale = 512 with a null pointer, on 16-byte-padded and on unpadded token rows."""
    from transception_amd._lib import TC_BF16, TC_F16, lib
    from transception_amd.train import DynamicLossScale
    L, HW = lib(), 70
    ld = (ncls + 7) // 8 * 8 if padded else ncls
    g = torch.Generator().manual_seed(ncls + 17 * padded)
    logits = torch.randn(HW, ld, generator=g).to(device=DEV, dtype=dtype)
    labels = torch.randint(0, ncls, (HW,), generator=g).to(DEV)
    sums = torch.zeros(1 + 3 * ncls, dtype=torch.float32, device=DEV)
    tc = TC_BF16 if dtype == torch.bfloat16 else TC_F16
    L.tc_seg_loss_fwd_tok(logits.data_ptr(), ld, labels.data_ptr(), None, sums.data_ptr(), 1, ncls, HW, tc, _stream())
    state = DynamicLossScale(init_scale=512.0).state(DEV)
    out = []
    for gscale, dev in ((1.0, state.data_ptr()), (512.0, None)):
        d = torch.zeros(HW, ld, dtype=dtype, device=DEV)
        L.tc_seg_loss_bwd_tok(None, logits.data_ptr(), ld, labels.data_ptr(), sums.data_ptr(), d.data_ptr(), ld, 1, ncls, HW, 0.4, 0.6, float(HW),
                              gscale, dev, tc, _stream())
        out.append(d)
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int16), out[1].view(torch.int16))
    assert bool(torch.isfinite(out[0].float()).all()) and float(out[0][:, :ncls].float().abs().max()) > 0.5       # scaled: 512 * O(1e-2)


# ---------------------------------------------------------------------------------------------------------------- 4. eager model steps
def test_eager_steps_skip_back_off_and_grow():
    """fp16 model, 64 x 64, B = 2, scale 2^40 with growth_interval 2: w_ce / n_pix = 0.4 / 8192 = 5e-5 times 1e12 is far above 65504, so
    the loss gradient itself overflows and the first step is skipped by arithmetic.  On every step: skipped <=> scale halved <=>
    parameters, momentum and working copy bit-equal to before.  Overall: a step is taken, two taken steps in a row double the scale,
    everything stays finite and the device's skip count is the number seen."""
    from transception_amd.train import DynamicLossScale, FusedSGD, SegLoss, train_step
    m = _fresh()
    x, y = _batch()
    scaler = DynamicLossScale(init_scale=2.0 ** 40, max_scale=2.0 ** 40, growth_interval=2)
    loss_fn, opt = SegLoss(9, loss_scale=scaler), FusedSGD(m, lr=0.05)
    m(x)                                                   # creates the arenas and the 16-bit working copy the first step is compared with
    opt.buf = torch.zeros_like(m.flat_parameters())
    prev = (m.flat_parameters().clone(), opt.buf.clone(), m._flat_lp.clone())
    scale, nskip, taken_run, doubled, history = scaler.value(), 0, 0, False, []
    for it in range(48):
        loss, _, _ = train_step(m, loss_fn, opt, x, y)
        sd = scaler.state_dict()
        now = (m.flat_parameters(), opt.buf, m._flat_lp)
        same = [torch.equal(a, b) for a, b in zip(now, prev)]
        skipped, halved = sd["skipped"] == nskip + 1, sd["scale"] == scale / 2
        history.append((scale, skipped))
        assert sd["skipped"] in (nskip, nskip + 1)
        assert skipped == halved == all(same) == any(same) == opt.last_step_skipped(), (it, history, sd, same)
        assert math.isfinite(float(loss.detach()))         # the reported loss is unscaled
        if it == 0:
            assert skipped
        if not skipped:
            taken_run += 1
            if taken_run % 2 == 0:                         # two taken steps in a row: the tracker reached the interval
                assert sd["scale"] == min(scale * 2, 2.0 ** 40) and sd["growth_tracker"] == 0, (it, history, sd)
                doubled = True
            else:
                assert sd["scale"] == scale and sd["growth_tracker"] == 1, (it, history, sd)
        else:
            taken_run = 0
        nskip, scale = sd["skipped"], sd["scale"]
        prev = tuple(t.clone() for t in now)
        if doubled and it >= 8:
            break
    print(f"eager dynamic steps (scale before the step, skipped): {history}")
    assert nskip < len(history) and doubled, history
    assert all(bool(torch.isfinite(t.float()).all()) for t in prev)
    assert scaler.skipped() == nskip == sum(s for _, s in history) == opt.skipped_steps


# ---------------------------------------------------------------------------------------------------------------- 5. static and dynamic agree
def test_dynamic_step_agrees_with_the_static_path():
    """One step from the same seeded fp16 model three times: static 4096 twice, then a DynamicLossScale that holds 4096.  When the two
    static runs are bit-equal so must the dynamic one be; otherwise it lies within 4 x their largest element-wise difference (the
    weight-gradient atomics make a step order-dependent; that spread is the parent path's own).
    Measured on the MI355X: the two static runs are not bit-equal; their spread is 2.8e-07 in the parameters, 5.6e-06 in the momentum
    and 1.2e-04 (one float16 step) in the working copy, and the dynamic run's distance from them was the same three figures."""
    from transception_amd.train import DynamicLossScale, FusedSGD, SegLoss, train_step
    x, y = _batch()
    out = []
    for ls in (4096.0, 4096.0, DynamicLossScale(init_scale=4096.0, growth_interval=10 ** 6)):
        m = _fresh()
        opt = FusedSGD(m, lr=0.05)
        train_step(m, SegLoss(9, loss_scale=ls), opt, x, y)
        torch.cuda.synchronize()
        assert not opt.last_step_skipped()
        out.append((m.flat_parameters().clone(), opt.buf.clone(), m._flat_lp.float()))
    for k, name in enumerate(("parameters", "momentum", "working copy")):
        a, b, d = out[0][k], out[1][k], out[2][k]
        spread = float((a - b).abs().max())
        dyn = max(float((d - a).abs().max()), float((d - b).abs().max()))
        print(f"{name}: static-static spread {spread:.3e}, dynamic-static {dyn:.3e}, bit-equal statics: {torch.equal(a, b)}")
        if torch.equal(a, b):
            assert torch.equal(d, a), (name, dyn)
        else:
            assert dyn <= 4.0 * spread, (name, dyn, spread)


# ---------------------------------------------------------------------------------------------------------------- 6. the captured step
@pytest.mark.parametrize("split", [False, True])
def test_captured_step_carries_the_scale(split):
    """A GraphedStep with DynamicLossScale(4096, growth_interval 3): six replays move the device state as the rule says for six clean
    steps; a scale of 2^40 loaded IN PLACE (same data_ptr) makes the next replay overflow: parameters bit-equal, scale halved."""
    from transception_amd.train import DynamicLossScale, FusedSGD, GraphedStep, SegLoss, train_step
    m = _fresh()
    x, y = _batch()
    scaler = DynamicLossScale(init_scale=4096.0, growth_interval=3)
    loss_fn, opt = SegLoss(9, loss_scale=scaler), FusedSGD(m, lr=0.05)
    train_step(m, loss_fn, opt, x, y)                      # the optimiser state exists and "first step" is not what gets captured
    step = GraphedStep(m, loss_fn, opt, x, y, None, warmup=0, force_split=split)
    sd = scaler.state_dict()
    assert sd == {"scale": 4096.0, "growth_tracker": 1, "skipped": 0}, sd          # capturing runs nothing
    want = (sd["scale"], sd["growth_tracker"], sd["skipped"])
    for _ in range(6):
        loss = step()[0]
        want = _rule(*want, 1.0, interval=3, lo=1.0, hi=2.0 ** 24)
    assert math.isfinite(float(loss))
    sd = scaler.state_dict()
    assert (sd["scale"], sd["growth_tracker"], sd["skipped"]) == want == (16384.0, 1, 0), (sd, want)
    ptr = scaler.state(DEV).data_ptr()
    scaler.load_state_dict({"scale": 2.0 ** 40, "growth_tracker": sd["growth_tracker"], "skipped": 0})
    assert scaler.state(DEV).data_ptr() == ptr
    before = (m.flat_parameters().clone(), opt.buf.clone(), m._flat_lp.clone())
    step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((m.flat_parameters(), opt.buf, m._flat_lp), before))
    assert scaler.state_dict() == {"scale": 2.0 ** 39, "growth_tracker": 0, "skipped": 1} and opt.last_step_skipped()
    assert scaler.state(DEV).data_ptr() == ptr
    scaler.load_state_dict({"scale": 4096.0})              # and back: the same graph takes a step again
    step()
    assert not torch.equal(m.flat_parameters(), before[0]) and bool(torch.isfinite(m.flat_parameters()).all())
    assert scaler.state_dict() == {"scale": 4096.0, "growth_tracker": 1, "skipped": 0}


# ---------------------------------------------------------------------------------------------------------------- 7. the trainer
def test_trainer_with_a_dynamic_loss_scale(tmp_path):
    """The test_trainer_gpu.py recipe with an fp16 model: loss_scale="dynamic" trains (finite losses, parameters finite and moved) and
    records the scale at every log line; loss_scale=None keeps the history's keys as they were."""
    from transception_amd import data as D
    from transception_amd.trainer import TrainConfig, trainer_synapse
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=2, slices_per_case=6, size=128, seed=11)
    hists = {}
    for ls in ("dynamic", None):
        m = _fresh()
        m._ensure_flat(torch.device(DEV))
        init = m.flat_parameters().clone()
        cfg = TrainConfig(root_path=base, list_dir=lists, max_epochs=3, batch_size=4, base_lr=0.05, img_size=64, seed=5, model_name="tiny",
                          loss_scale=ls)
        lines = []
        hists[ls] = hist = trainer_synapse(cfg, m, str(tmp_path / f"snap_{ls}"), log=lines.append)
        assert hist["iterations"] == 9 and len(hist["loss"]) == 9
        if ls == "dynamic":
            assert all(math.isfinite(v) for v in hist["loss"]), hist["loss"]
            assert len(hist["loss_scale"]) == 9 and all(1.0 <= v <= 2.0 ** 24 and math.log2(v) % 1 == 0 for v in hist["loss_scale"])
            p = m.flat_parameters()
            assert bool(torch.isfinite(p).all()) and not torch.equal(p, init)
            nskip = sum("update SKIPPED" in l for l in lines)
            assert all("dynamic loss scale now" in l for l in lines if "update SKIPPED" in l)
            assert hist["loss_scale"][-1] == 65536.0 / 2 ** nskip, (hist["loss_scale"], nskip)       # nine steps: no growth yet
            print(f"trainer, dynamic: loss scale per log line {hist['loss_scale']}, {nskip} skipped")
    assert "loss_scale" not in hists[None] and set(hists["dynamic"]) == set(hists[None]) | {"loss_scale"}

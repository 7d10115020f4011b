"""Weight averaging on the flat arenas (csrc/ema.hip: tc_ema_advance, tc_ema_update_multi, tc_swap_f32; train.WeightEMA): the state
words against the float64 schedule of tests/ema_ref.py to the bit, the update kernel against the float64 closed form -- exactly on grid
inputs, within the derived bound (that module's docstring: |e' - ref| <= 4 u omd |w - e| + 2 u |ref|, u = 2^-24) on seeded normals --,
the copy of the first update, the skip, the in-place exchange, and the optimiser hook in eager steps, in captured steps, under the skip,
in swapped(), through state_dict() and in the trainer.

Measured on the MI355X, worst error / bound: 0.499 for tc_ema_update_multi at decay 0.999 on the seeded normals, 0.500 over the
optimiser's eager and replayed steps (the bound is the first-order count doubled, so 0.5 is the count itself); the state words matched
to the bit."""
import math
import os

import pytest
import torch

from ema_ref import ema_ref, state_words

pytestmark = pytest.mark.gpu

from transception_amd._lib import lib  # noqa: E402

DEV = "cuda:0"
N_ARENA = 700000
SEGS = [(0, 96),                  # 16-byte path, one pass
        (104, 37),                # odd length: element path
        (144, 524296),            # 16-byte path, more than one pass of its blocks x 256 threads x 4 elements
        (524448, 70001)]          # element path, more than one pass
SENT_P, SENT_E = 1234.5, -77.25
SIZE, BATCH = 64, 2


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32 if a.element_size() == 4 else torch.int16),
                                                                     b.view(torch.int32 if b.element_size() == 4 else torch.int16))


def words(n, d, omd, r=0):
    """An EMA state from its four words (n and r are int32)."""
    w = torch.zeros(4, dtype=torch.float32)
    w[1], w[2] = d, omd
    w.view(torch.int32)[0], w.view(torch.int32)[3] = n, r
    return w


def read_words(state):
    w = state.detach().cpu()
    return int(w.view(torch.int32)[0]), float(w[1]), float(w[2]), int(w.view(torch.int32)[3])


def live_mask():
    live = torch.zeros(N_ARENA, dtype=torch.bool)
    for off, ln in SEGS:
        live[off:off + ln] = True
    return live


_ARENA = {}


def arena(kind):
    """(weights, shadow, live mask) on the host, a sentinel outside the segments; built once per kind, never changed.
    "grid": multiples of 2^-8 in [-4, 4]; "normal": seeded normals."""
    if kind not in _ARENA:
        g = torch.Generator().manual_seed(11)
        live = live_mask()
        if kind == "grid":
            p = torch.randint(-1024, 1025, (N_ARENA,), generator=g).float() / 256.0
            e = torch.randint(-1024, 1025, (N_ARENA,), generator=g).float() / 256.0
        else:
            p, e = torch.randn(N_ARENA, generator=g), torch.randn(N_ARENA, generator=g)
        p[~live], e[~live] = SENT_P, SENT_E
        _ARENA[kind] = (p, e, live)
    return _ARENA[kind]


def run_update(p0, e0, state, ss=None):
    """tc_ema_update_multi on device copies; returns (shadow, weights) on the host."""
    p, e = p0.to(DEV), e0.to(DEV)
    sd = torch.tensor([x for s in SEGS for x in s], dtype=torch.int64, device=DEV)
    st = state.to(DEV)
    lib().tc_ema_update_multi(ptr(e), ptr(p), ptr(sd), len(SEGS), max(n for _, n in SEGS), ptr(st), ptr(ss), stream())
    torch.cuda.synchronize()
    assert same_bits(st, state)                                              # the update kernel only reads the state
    return e.cpu(), p.cpu()


def check_untouched(e, p, p0, e0, live):
    assert same_bits(p, p0), "the weights were written"
    assert same_bits(e[~live], e0[~live]), "a sentinel outside the segments was written"


# ---------------------------------------------------------------------------------------------------------------- 1. tc_ema_advance
@pytest.mark.parametrize("decay", [0.999, 0.9])
@pytest.mark.parametrize("warmup", [True, False], ids=["warmup", "plain"])
def test_advance_words_match_the_schedule_to_the_bit(warmup, decay):
    """From counts 0, 1, 8 and 99 999, with no sum and with a finite one: all four words are the reference's, bit for bit.  With an inf or
    a NaN sum all four words -- a non-zero reserved word among them -- stay as they were."""
    for n0 in (0, 1, 8, 99999):
        start = words(*state_words(n0, decay, warmup)) if n0 else torch.zeros(4)
        want = words(*state_words(n0 + 1, decay, warmup))
        for s in (None, 3.0e38):
            st = start.to(DEV)
            ss = None if s is None else torch.full((1,), s, dtype=torch.float32, device=DEV)
            lib().tc_ema_advance(ptr(st), ptr(ss), decay, int(warmup), stream())
            torch.cuda.synchronize()
            assert same_bits(st, want), (n0, s, read_words(st), read_words(want))
        odd = start.clone()
        odd.view(torch.int32)[3] = 7
        for bad in (math.inf, math.nan):                                     # (a sum of squares is never negative)
            st = odd.to(DEV)
            ss = torch.full((1,), bad, dtype=torch.float32, device=DEV)
            lib().tc_ema_advance(ptr(st), ptr(ss), decay, int(warmup), stream())
            torch.cuda.synchronize()
            assert same_bits(st, odd), (n0, bad, read_words(st))


# ---------------------------------------------------------------------------------------------------------------- 2. tc_ema_update_multi
def test_update_is_exact_on_grid_inputs():
    """w and e multiples of 2^-8 in [-4, 4], decay 1 - 2^-6: w - e is a multiple of 2^-8 below 2^4, its product by 2^-6 a multiple of
    2^-14, and the sum a multiple of 2^-14 below 2^3 -- 17 bits: every intermediate is exact in float32 with or without fusion, so the
    result equals the float64 closed form."""
    p0, e0, live = arena("grid")
    e, p = run_update(p0, e0, words(5, 1.0 - 2.0 ** -6, 2.0 ** -6))
    ref, _ = ema_ref(e0[live], p0[live], 2.0 ** -6)
    assert torch.equal(e[live].double(), ref)
    assert bool((e[live] != e0[live]).any())
    check_untouched(e, p, p0, e0, live)


def test_update_meets_the_derived_bound_on_normals():
    p0, e0, live = arena("normal")
    n, d, omd, _ = state_words(100000, 0.999, True)
    e, p = run_update(p0, e0, words(n, d, omd))
    ref, bound = ema_ref(e0[live], p0[live], omd)
    err = (e[live].double() - ref).abs()
    print(f"tc_ema_update_multi, decay 0.999 on normals: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), float((err / bound).max())
    assert bool((e[live] != e0[live]).any())
    check_untouched(e, p, p0, e0, live)


def test_first_update_copies_the_value_itself():
    """omd == 1.0f: the shadow is bit-equal to the weights, also where e + (w - e) != w in float32 (e = 1e8, w = 1; e = -3e7, w = 0.1)."""
    p0, e0, live = arena("normal")
    p0, e0 = p0.clone(), e0.clone()
    for off, ln in SEGS:                                                     # a few such elements in every segment, on both element paths
        e0[off:off + ln:5], p0[off:off + ln:5] = 1.0e8, 1.0
        e0[off + 1:off + ln:7], p0[off + 1:off + ln:7] = -3.0e7, 0.1
    assert bool(((e0 + (p0 - e0)) != p0)[live].any())
    e, p = run_update(p0, e0, words(*state_words(1, 0.999, True)))
    assert same_bits(e[live], p0[live])
    check_untouched(e, p, p0, e0, live)


@pytest.mark.parametrize("bad", [math.inf, math.nan], ids=["inf", "nan"])
def test_update_skips_on_a_non_finite_norm(bad):
    p0, e0, live = arena("normal")
    n, d, omd, _ = state_words(50, 0.9, False)
    ss = torch.full((1,), bad, dtype=torch.float32, device=DEV)
    e, p = run_update(p0, e0, words(n, d, omd), ss)
    assert same_bits(e, e0) and same_bits(p, p0)
    e, p = run_update(p0, e0, words(1, 0.0, 1.0), ss)                        # a copying update is skipped too
    assert same_bits(e, e0) and same_bits(p, p0)
    fine = torch.full((1,), 5.0, dtype=torch.float32, device=DEV)
    e, p = run_update(p0, e0, words(n, d, omd), fine)                        # and a finite sum is not
    assert not same_bits(e, e0)
    check_untouched(e, p, p0, e0, live)


# ---------------------------------------------------------------------------------------------------------------- 3. tc_swap_f32
@pytest.mark.parametrize("n", [4, 1028, 700000])
def test_swap_exchanges_bit_patterns(n):
    """Random 32-bit patterns (NaN payloads, infinities and subnormals among them) plus -0.0 and two NaNs with payloads: exchanged bit for
    bit, four guard words behind each buffer untouched, and a second call restores both."""
    g = torch.Generator().manual_seed(n)
    a0 = torch.randint(-2 ** 31, 2 ** 31, (n + 4,), generator=g, dtype=torch.int64).to(torch.int32)
    b0 = torch.randint(-2 ** 31, 2 ** 31, (n + 4,), generator=g, dtype=torch.int64).to(torch.int32)
    a0[0], a0[1], b0[2] = -2 ** 31, 0x7FC01234, -0x3FFEDC                    # -0.0, a quiet NaN with a payload, a negative NaN with one
    a, b = a0.view(torch.float32).to(DEV), b0.view(torch.float32).to(DEV)
    lib().tc_swap_f32(ptr(a), ptr(b), n, stream())
    torch.cuda.synchronize()
    ai, bi = a.cpu().view(torch.int32), b.cpu().view(torch.int32)
    assert torch.equal(ai[:n], b0[:n]) and torch.equal(bi[:n], a0[:n])
    assert torch.equal(ai[n:], a0[n:]) and torch.equal(bi[n:], b0[n:])
    lib().tc_swap_f32(ptr(a), ptr(b), n, stream())
    torch.cuda.synchronize()
    assert torch.equal(a.cpu().view(torch.int32), a0) and torch.equal(b.cpu().view(torch.int32), b0)


# ---------------------------------------------------------------------------------------------------------------- the model
_SD = None


def _fresh(dtype):
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


def _optimizer(kind, M):
    from transception_amd.train import FusedAdamW, FusedSGD
    return FusedSGD(M, lr=0.05) if kind == "sgd" else FusedAdamW(M, lr=1e-3, no_decay="norm_bias")


def _ema_live(ema, n):
    live = torch.zeros(n, dtype=torch.bool, device=DEV)
    for off, ln in ema.segments():
        live[off:off + ln] = True
    return live


def check_step(ema, shadow_before, n, what):
    """The shadow after the n-th update against the closed form from the shadow before it and the weights as they stand; the state words
    to the bit; everything outside the EMA's segments still equal to the weights there (they never move)."""
    flat = ema.model.flat_parameters()
    want = state_words(n, ema.decay, ema.warmup)
    assert read_words(ema._state) == want, (what, read_words(ema._state), want)
    live = _ema_live(ema, flat.numel())
    ref, bound = ema_ref(shadow_before[live], flat[live], want[2])
    err = (ema.shadow[live].double() - ref).abs()
    ratio = float((err / (bound + 1e-300)).max())                            # (a copying update: error 0 against a bound of 0)
    print(f"{what}, update {n}: worst error / bound {ratio:.3f}")
    assert bool((err <= bound).all()), (what, n, ratio)
    assert torch.equal(ema.shadow[~live], flat[~live]) and torch.equal(ema.shadow[~live], shadow_before[~live])


# ---------------------------------------------------------------------------------------------------------------- 4. the optimiser hook
@pytest.mark.parametrize("kind,dtype", [("sgd", torch.float32), ("adamw", torch.bfloat16)], ids=["sgd-fp32", "adamw-bf16"])
def test_optimizer_steps_average_the_weights(kind, dtype):
    """Three eager steps, then four replays of a GraphedStep: after each the shadow follows the closed form and updates() is the number of
    steps.  AdamW runs with the overflow guard on (the launches receive the squared norm), SGD without (they receive none).  Then one inf
    in the gradient arena under the guard: the update is skipped and weights, shadow and state word stay bit-identical.  The segment table
    is one decay class: fewer segments than no_decay="norm_bias" hands the Adam kernel."""
    from transception_amd.train import GraphedStep, SegLoss, WeightEMA, train_step
    M = _fresh(dtype)
    x, y = _batch()
    opt, loss_fn = _optimizer(kind, M), SegLoss(9)
    ema = opt.ema = WeightEMA(M, decay=0.9, warmup=True)
    if kind == "adamw":
        opt.guard_overflow = True
    M._ensure_flat(torch.device(DEV))
    shadow = M.flat_parameters().clone()                                     # what the shadow starts as: a clone of the arena
    n = 0
    for _ in range(3):
        train_step(M, loss_fn, opt, x, y)
        torch.cuda.synchronize()
        n += 1
        assert ema.updates() == n
        check_step(ema, shadow, n, f"{kind} eager")
        shadow = ema.shadow.clone()
    ptrs = (ema.shadow.data_ptr(), ema._state.data_ptr(), ema._segs_dev.data_ptr())
    step = GraphedStep(M, loss_fn, opt, x, y, None, warmup=0)
    assert ema.updates() == n                                                # capturing runs nothing
    for _ in range(4):
        loss = step()[0]
        torch.cuda.synchronize()
        n += 1
        assert math.isfinite(float(loss)) and ema.updates() == n
        check_step(ema, shadow, n, f"{kind} replay")
        shadow = ema.shadow.clone()
    assert n == 7 and ptrs == (ema.shadow.data_ptr(), ema._state.data_ptr(), ema._segs_dev.data_ptr())
    assert not torch.equal(ema.shadow, M.flat_parameters())
    nseg = len(ema.segments())
    print(f"{kind}: EMA segments {nseg}, optimiser segments {len(opt._segs())}")
    assert nseg == len(opt._segs()) if kind == "sgd" else nseg < len(opt._segs())       # SGD's own table is one decay class too
    # the skip
    opt.guard_overflow = True
    live = _ema_live(ema, shadow.numel())
    M.flat_gradients()[int(live.nonzero()[0])] = math.inf
    before = (M.flat_parameters().clone(), ema.shadow.clone(), ema._state.clone())
    opt.step()
    torch.cuda.synchronize()
    assert opt.last_step_skipped()
    assert same_bits(M.flat_parameters(), before[0]) and same_bits(ema.shadow, before[1]) and same_bits(ema._state, before[2])
    assert ema.updates() == 7


def test_no_ema_no_launch():
    """ema is None: the step launches what it always did (two C-ABI entries fewer than with the average attached)."""
    from transception_amd import _lib
    from transception_amd.train import SegLoss, WeightEMA, train_step
    M = _fresh(torch.float32)
    x, y = _batch()
    opt, loss_fn = _optimizer("sgd", M), SegLoss(9)
    train_step(M, loss_fn, opt, x, y)
    c0 = _lib._Lib.calls
    opt.step()
    plain = _lib._Lib.calls - c0
    opt.ema = WeightEMA(M)
    c0 = _lib._Lib.calls
    opt.step()
    torch.cuda.synchronize()
    assert _lib._Lib.calls - c0 == plain + 2 and opt.ema.updates() == 1
    with pytest.raises(ValueError, match="another model"):
        opt.ema = WeightEMA(torch.nn.Linear(2, 2))
        opt.step()


# ---------------------------------------------------------------------------------------------------------------- 5. swapped()
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_swapped_evaluates_the_averaged_weights(dtype):
    """Inside swapped() the eval-mode logits are bit-equal to those of a second model that loaded model_state_dict() strictly; afterwards
    the arena, the shadow and the 16-bit copy are bit-identical to what they were and the captured step still runs.  Nested entry and an
    opt.step() inside raise."""
    from transception_amd.train import GraphedStep, SegLoss, WeightEMA, train_step
    M = _fresh(dtype)
    x, y = _batch()
    opt, loss_fn = _optimizer("adamw", M), SegLoss(9)
    ema = opt.ema = WeightEMA(M, decay=0.5, warmup=False)
    train_step(M, loss_fn, opt, x, y)
    train_step(M, loss_fn, opt, x, y)
    step = GraphedStep(M, loss_fn, opt, x, y, None, warmup=0)
    step()
    torch.cuda.synchronize()
    assert ema.updates() == 3 and not torch.equal(ema.shadow, M.flat_parameters())
    lp = lambda: M._flat_lp.clone() if dtype != torch.float32 else None
    before = (M.flat_parameters().clone(), ema.shadow.clone(), lp())
    ptrs = (M.flat_parameters().data_ptr(), ema.shadow.data_ptr())
    sd = ema.model_state_dict()
    assert list(sd) == list(M.state_dict())
    other = _fresh(dtype)
    other.load_state_dict(sd, strict=True)
    other.eval()
    M.eval()
    with torch.no_grad():
        plain = M(x)
        with ema.swapped() as inner:
            assert inner is M and same_bits(M.flat_parameters(), before[1]) and same_bits(ema.shadow, before[0])
            if dtype != torch.float32:
                assert torch.equal(M._flat_lp, before[1].to(dtype))
            averaged = M(x)
            with pytest.raises(RuntimeError, match="already active"):
                with ema.swapped():
                    pass
            with pytest.raises(RuntimeError, match="swapped"):
                opt.step()
            assert same_bits(M.flat_parameters(), before[1])                 # neither attempt moved anything
        want = other(x)
    torch.cuda.synchronize()
    assert same_bits(averaged, want) and not torch.equal(averaged, plain)
    M.train()
    assert same_bits(M.flat_parameters(), before[0]) and same_bits(ema.shadow, before[1])
    assert dtype == torch.float32 or same_bits(M._flat_lp, before[2])
    assert ptrs == (M.flat_parameters().data_ptr(), ema.shadow.data_ptr()) and ema.updates() == 3
    loss = step()[0]
    torch.cuda.synchronize()
    assert math.isfinite(float(loss)) and ema.updates() == 4
    for k, v in M.named_parameters():                                        # the parameter entries are clones of the averaged values
        off, shape = M._index[k]
        assert sd[k].data_ptr() != v.data_ptr() and torch.equal(sd[k].reshape(-1), before[1][off:off + v.numel()])


# ---------------------------------------------------------------------------------------------------------------- 6. state_dict
def test_state_dict_round_trip_in_place():
    from transception_amd.train import SegLoss, WeightEMA, train_step
    M = _fresh(torch.float32)
    x, y = _batch()
    opt, loss_fn = _optimizer("sgd", M), SegLoss(9)
    ema = opt.ema = WeightEMA(M, decay=0.9, warmup=True)
    for _ in range(2):
        train_step(M, loss_fn, opt, x, y)
    sd = ema.state_dict()
    assert set(sd) == {"n", "decay", "warmup", "shadow"} and (sd["n"], sd["decay"], sd["warmup"]) == (2, 0.9, True)
    assert sd["shadow"].data_ptr() != ema.shadow.data_ptr() and torch.equal(sd["shadow"], ema.shadow)
    for _ in range(2):
        train_step(M, loss_fn, opt, x, y)
    torch.cuda.synchronize()
    assert ema.updates() == 4 and not torch.equal(sd["shadow"], ema.shadow)
    ptrs = (ema.shadow.data_ptr(), ema._state.data_ptr())
    ema.load_state_dict(sd)
    assert ptrs == (ema.shadow.data_ptr(), ema._state.data_ptr())
    assert ema.updates() == 2 and torch.equal(ema.shadow, sd["shadow"])
    train_step(M, loss_fn, opt, x, y)                                        # the next update is the third: d = min(0.9, 4 / 13)
    torch.cuda.synchronize()
    check_step(ema, sd["shadow"], 3, "after load_state_dict")
    for bad in (dict(sd, decay=0.5), dict(sd, warmup=False), dict(sd, n=-1), dict(sd, decay=1.0)):
        with pytest.raises(ValueError):
            ema.load_state_dict(bad)
    assert ema.updates() == 3 and (ema.decay, ema.warmup) == (0.9, True)


# ---------------------------------------------------------------------------------------------------------------- 7. the trainer
@pytest.mark.parametrize("dtype,loss_scale", [(torch.bfloat16, None), (torch.float16, "dynamic")], ids=["bf16", "fp16-dynamic"])
@pytest.mark.parametrize("graphed", [True, False], ids=["graphed", "eager"])
def test_trainer_with_ema(tmp_path, graphed, dtype, loss_scale):
    """The tiny synthetic set and configuration of the AdamW trainer test, a checkpoint after every epoch and an evaluation on the
    averaged weights: one averaged checkpoint beside every plain one, each loading strictly and differing from it, the device's count
    equal to the iterations, and the model left holding the trained weights.
    bf16 storage skips no update, so the count is the iterations.  Under that test's own storage, fp16 with the dynamic loss scale, an
    overflowing update is skipped on the device and must not be averaged in: the count is the iterations minus the skips every log line
    saw, which is the optimiser's own device count; an averaged checkpoint written after fewer than two counted updates is a copy."""
    import numpy as np
    from transception_amd import data as D
    from transception_amd.trainer import TrainConfig, trainer_synapse
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=2, slices_per_case=6, size=128, seed=11)
    M = _fresh(dtype)
    cfg = TrainConfig(root_path=base, list_dir=lists, max_epochs=3, batch_size=4, img_size=64, seed=5, model_name="tiny", graphed=graphed,
                      optimizer="adamw", base_lr=1e-3, no_decay="norm_bias", loss_scale=loss_scale, eval_interval=1, ema_decay=0.9)
    g = np.random.default_rng(0)
    vol = (g.random((2, 64, 64)).astype(np.float32), (g.random((2, 64, 64)) * 3).astype(np.uint8), "case0")
    lines = []
    hist = trainer_synapse(cfg, M, str(tmp_path / "snap"), volumes=lambda: [vol], log=lines.append)
    snap = str(tmp_path / "snap")
    nskip = sum("update SKIPPED" in l for l in lines)
    print(f"trainer with EMA, graphed={graphed}, {dtype}: {hist['ema_updates']} updates averaged, {nskip} skipped")
    assert hist["iterations"] == 9 and all(math.isfinite(v) for v in hist["loss"])
    assert hist["ema_updates"] == hist["iterations"] - nskip == hist["optimizer_step"] and nskip < 8
    assert nskip == 0 or loss_scale == "dynamic"
    assert hist["checkpoints"] == [os.path.join(snap, f"tiny_epoch_{e}.pth") for e in range(3)]
    assert hist["ema_checkpoints"] == [os.path.join(snap, f"tiny_ema_epoch_{e}.pth") for e in range(3)]
    assert sorted(os.listdir(snap)) == sorted(os.path.basename(p) for p in hist["checkpoints"] + hist["ema_checkpoints"])
    assert len(hist["dice"]) == 3 and all(0.0 <= d <= 1.0 for d in hist["dice"])
    params = set(M._index)
    fresh = _fresh(dtype)
    for epoch, (plain_path, ema_path) in enumerate(zip(hist["checkpoints"], hist["ema_checkpoints"])):
        plain, avg = torch.load(plain_path), torch.load(ema_path)
        fresh.load_state_dict(avg, strict=True)
        assert list(plain) == list(avg)
        if 3 * (epoch + 1) - nskip >= 2:                                     # at least two counted updates by then, wherever the skips fell
            assert any(not torch.equal(plain[k], avg[k]) for k in params)
        assert all(torch.equal(plain[k], avg[k]) for k in plain if k not in params)       # buffers are the live ones
    last = torch.load(hist["checkpoints"][-1])
    now = M.state_dict()
    assert all(torch.equal(last[k], now[k]) for k in params)                # swapped back after the last evaluation


def test_trainer_without_ema_is_unchanged(tmp_path):
    """ema_decay=None: no averaged checkpoint, no key in the history, no WeightEMA on the way."""
    from transception_amd import data as D
    from transception_amd.trainer import TrainConfig, trainer_synapse
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=1, slices_per_case=4, size=64, seed=2)
    M = _fresh(torch.bfloat16)
    cfg = TrainConfig(root_path=base, list_dir=lists, max_epochs=2, batch_size=2, img_size=64, seed=5, model_name="tiny", optimizer="adamw",
                      base_lr=1e-3)
    hist = trainer_synapse(cfg, M, str(tmp_path / "snap"), log=lambda s: None)
    assert "ema_checkpoints" not in hist and "ema_updates" not in hist and hist["iterations"] == 4
    assert os.listdir(str(tmp_path / "snap")) == ["tiny_epoch_1.pth"]

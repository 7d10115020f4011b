"""Fused Adam / AdamW on the flat arenas (csrc/train.hip: tc_adam_advance, tc_adam_step_multi; train.FusedAdamW): the kernels against the
float64 closed form of tests/adam_ref.py within bounds derived by counting the kernel's roundings (that module's docstring: with
u = 2^-24,  m' within 20 u Am,  v' within 38 u Av,  w' within 4 u |w| + 54 u (lr / bc1) Am / den; every K is the counted number doubled),
the step count on the device, the skip, and the optimiser in eager steps, in captured steps, under the dynamic loss scale and in the trainer.

The reference takes the bias terms from the Adam state READ BACK from the device and the clip coefficient from the squared norm read back
(tc_adam_advance and tc_grad_sumsq have tests of their own), so the update kernel is judged on its own.
Measured on the MI355X, worst error / bound over all cases: m 0.15, v 0.15, weights 0.31; tc_adam_advance's bias words matched to the bit."""
import math

import numpy as np
import pytest
import torch

from adam_ref import adam_ref, betas32, bias_terms, bounds, f32

pytestmark = pytest.mark.gpu

from transception_amd._lib import TC_BF16, TC_F16, TcError, lib  # noqa: E402

DEV = "cuda:0"
N_ARENA = 700000
SEGS = [(0, 96),                  # 16-byte path, one pass
        (104, 37),                # odd length: element path
        (144, 524296),            # 16-byte path, more than one pass of its 256 blocks x 256 threads x 4 elements
        (524448, 70001)]          # element path, more than one pass of 256 x 256
SENT_P, SENT_G, SENT_M, SENT_V = 1234.5, -3.0, -77.25, 55.5
HYPERS = [(1e-3, (0.9, 0.999), 1e-8, 1e-2),      # torch.optim.AdamW's defaults
          (1e-2, (0.5, 0.9), 1e-3, 0.1)]         # every term large enough that misplacing it cannot hide
LP = {None: 0, torch.bfloat16: TC_BF16, torch.float16: TC_F16}
CLIP = 400.0                      # the arena's gradient norm is about 1.2e3 (asserted): active
SIZE, BATCH = 64, 2


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def ptr(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def ibits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(ibits(a), ibits(b))


_ARENA = {}


def arena():
    """(parameters, gradient, m, v, live mask) on the host: seeded normals inside the segments (v = z^2 + 1e-3), a sentinel everywhere
    else.  Built once, never changed."""
    if not _ARENA:
        g = torch.Generator().manual_seed(7)
        live = torch.zeros(N_ARENA, dtype=torch.bool)
        for off, ln in SEGS:
            live[off:off + ln] = True
        p, gr, m = torch.randn(N_ARENA, generator=g), torch.randn(N_ARENA, generator=g), torch.randn(N_ARENA, generator=g)
        v = torch.randn(N_ARENA, generator=g) ** 2 + 1e-3
        p[~live], gr[~live], m[~live], v[~live] = SENT_P, SENT_G, SENT_M, SENT_V
        _ARENA["a"] = (p, gr, m, v, live)
    return _ARENA["a"]


def adam_words(state):
    w = state.detach().cpu()
    return [int(w.view(torch.int32)[0]), float(w[1]), float(w[2]), int(w.view(torch.int32)[3])]


def state_at(t, betas=(0.9, 0.999)):
    """An Adam state that has counted t updates (the bias words as tc_adam_advance would have left them)."""
    w = torch.zeros(4, dtype=torch.float32)
    w.view(torch.int32)[0] = t
    if t:
        w[1], w[2] = bias_terms(*betas, t)
    return w.to(DEV)


def device_sumsq(gd):
    ss = torch.zeros(1, dtype=torch.float32, device=DEV)
    lib().tc_grad_sumsq(ptr(gd), gd.numel(), ptr(ss), stream())
    torch.cuda.synchronize()
    return ss


def coef_of(ss, clip):
    """clip_grad_norm_'s coefficient from the squared norm of the gradients as stored."""
    return min(clip / (math.sqrt(float(ss)) + 1e-6), 1.0)


def run_adam(hyper, t0, decoupled, lp_dtype, lr_on_device=True, gscale=1.0, ss=None, clip=math.inf, wd_seg=None, scale_state=None):
    """tc_adam_advance (from a state that counted t0 updates) + tc_adam_step_multi on device copies of the arena.  The host's lr is 999
    when the real one sits in lr_dev.  Returns (p, g, m, v, lp, state) on the device."""
    lr, betas, eps, wd = hyper
    p0, g0, m0, v0, _ = arena()
    p, gd, m, v = p0.to(DEV), g0.to(DEV), m0.to(DEV), v0.to(DEV)
    lp = p0.to(lp_dtype).to(DEV) if lp_dtype is not None else None
    sd = torch.tensor([x for s in SEGS for x in s], dtype=torch.int64, device=DEV)
    wdd = torch.tensor(wd_seg, dtype=torch.float32, device=DEV) if wd_seg is not None else None
    lr_dev = torch.full((1,), lr, dtype=torch.float32, device=DEV) if lr_on_device else None
    st = state_at(t0, betas)
    lib().tc_adam_advance(ptr(st), ptr(ss), betas[0], betas[1], stream())
    lib().tc_adam_step_multi(ptr(p), ptr(gd), ptr(m), ptr(v), ptr(sd), ptr(wdd), len(SEGS), max(n for _, n in SEGS), 999.0 if lr_on_device else lr,
                             ptr(lr_dev), betas[0], betas[1], eps, wd, int(decoupled), gscale, ptr(ss), clip, ptr(lp), LP[lp_dtype], ptr(scale_state),
                             ptr(st), stream())
    torch.cuda.synchronize()
    return p, gd, m, v, lp, st


def check_update(new, old, live, hyper, bc, decoupled, c=1.0, wd=None, what=""):
    """The three derived bounds on the live elements of (p, m, v) tensors -- host or device, all of one kind; prints the worst
    error / bound ratios before it asserts.  wd: a float64 tensor per live element, or None for the hyper set's."""
    lr, betas, eps, wd0 = hyper
    (pn, mn, vn), (w, g, m, v) = new, old
    wd = f32(wd0) if wd is None else wd
    w_ref, m_ref, v_ref, Am, Av, den = adam_ref(w[live], g[live], m[live], v[live], f32(lr), *betas32(*betas), f32(eps), wd, bc[0], bc[1], decoupled, c)
    bm, bv, bw = bounds(w[live], f32(lr), bc[0], Am, Av, den)
    em, ev, ew = (mn[live].double() - m_ref).abs(), (vn[live].double() - v_ref).abs(), (pn[live].double() - w_ref).abs()
    tiny = 1e-300                                                            # (padding words: error 0 against a bound of 0)
    rm, rv, rw = float((em / (bm + tiny)).max()), float((ev / (bv + tiny)).max()), float((ew / (bw + tiny)).max())
    print(f"{what}: worst error / bound: m {rm:.3f}, v {rv:.3f}, weights {rw:.3f}")
    assert bool((em <= bm).all()), (what, "m", rm)
    assert bool((ev <= bv).all()), (what, "v", rv)
    assert bool((ew <= bw).all()), (what, "weights", rw)


def check_arena(out, hyper, t0, decoupled, lp_dtype, c=1.0, wd=None, what=""):
    """check_update on the arena's live elements with the bias terms of the state read back, plus the exact checks: t advanced by one,
    sentinels and the gradient bit-unchanged, lp bit-equal to the rounding of the returned p."""
    p0, g0, m0, v0, live = arena()
    p, gd, m, v, lp, st = out
    words = adam_words(st)
    assert words[0] == t0 + 1 and words[3] == 0, words
    check_update((p.cpu(), m.cpu(), v.cpu()), (p0, g0, m0, v0), live, hyper, (words[1], words[2]), decoupled, c, wd, what)
    dead = ~live
    assert same_bits(p.cpu()[dead], p0[dead]) and same_bits(m.cpu()[dead], m0[dead]) and same_bits(v.cpu()[dead], v0[dead]) and same_bits(gd, g0)
    assert bool((p.cpu()[live] != p0[live]).any()) and bool((v.cpu()[live] > 0).all())
    if lp_dtype is not None:
        assert torch.equal(lp.cpu()[live], p.cpu()[live].to(lp_dtype)) and same_bits(lp.cpu()[dead], p0.to(lp_dtype)[dead])


# ---------------------------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("lp_dtype", [None, torch.bfloat16, torch.float16], ids=["lp=None", "lp=bf16", "lp=f16"])
@pytest.mark.parametrize("lr_on_device", [True, False], ids=["lr_dev", "lr_arg"])
@pytest.mark.parametrize("hyper", HYPERS, ids=["defaults", "large-terms"])
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("t0", [0, 1000], ids=["t=0->1", "t=1000->1001"])
def test_adam_step_multi(t0, decoupled, hyper, lr_on_device, lp_dtype):
    """Four segments (both element paths, one pass and several) of a 700 k arena, from random m and v = z^2 + 1e-3, against adam_ref within
    the derived bounds; sentinels outside the segments and the gradient bit-unchanged, lp the rounding of the returned p."""
    out = run_adam(hyper, t0, decoupled, lp_dtype, lr_on_device)
    check_arena(out, hyper, t0, decoupled, lp_dtype, what=f"adam {hyper} t0={t0} decoupled={decoupled} lr_dev={lr_on_device}")


# ---------------------------------------------------------------------------------------------------------------- 2. per-segment decay
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_adam_step_multi_per_segment_decay(decoupled):
    """wd_dev = (0, 0.1, 0, 0.1) over the four segments (the scalar wd argument is 7: it must not be used): each segment meets the bounds
    with its own decay."""
    hyper = HYPERS[1]
    decays = (0.0, 0.1, 0.0, 0.1)
    out = run_adam((hyper[0], hyper[1], hyper[2], 7.0), 3, decoupled, torch.bfloat16, wd_seg=decays)
    per = torch.zeros(N_ARENA, dtype=torch.float64)
    for (off, n), d in zip(SEGS, decays):
        per[off:off + n] = f32(d)
    live = arena()[4]
    check_arena(out, hyper, 3, decoupled, torch.bfloat16, wd=per[live], what=f"adam wd_dev decoupled={decoupled}")
    # and the decay does act where it is 0.1: with decoupled decay the weights of segment 1 differ from a run without any
    if decoupled:
        none = run_adam((hyper[0], hyper[1], hyper[2], 0.0), 3, True, None)
        a, b = out[0].cpu(), none[0].cpu()
        assert torch.equal(a[:96], b[:96]) and bool((a[104:141] != b[104:141]).any())


# ---------------------------------------------------------------------------------------------------------------- 3. the skip
@pytest.mark.parametrize("lp_dtype", [None, torch.bfloat16, torch.float16], ids=["lp=None", "lp=bf16", "lp=f16"])
@pytest.mark.parametrize("bad", [math.inf, math.nan], ids=["inf", "nan"])
def test_adam_skips_on_a_non_finite_norm(bad, lp_dtype):
    """*clip_sumsq inf / NaN: p, m, v, lp and all four state words are bit-identical after tc_adam_advance + tc_adam_step_multi, with and
    without a clip threshold; a finite sum advances t by one."""
    p0, g0, m0, v0, _ = arena()
    ss = torch.full((1,), bad, dtype=torch.float32, device=DEV)
    for clip in (CLIP, math.inf):
        p, gd, m, v, lp, st = run_adam(HYPERS[1], 1000, True, lp_dtype, ss=ss, clip=clip)
        assert same_bits(p, p0) and same_bits(m, m0) and same_bits(v, v0) and same_bits(gd, g0) and (lp is None or same_bits(lp, p0.to(lp_dtype)))
        assert same_bits(st, state_at(1000, HYPERS[1][1]))
    fine = torch.full((1,), 5.0, dtype=torch.float32, device=DEV)
    p, _, _, _, _, st = run_adam(HYPERS[1], 1000, True, lp_dtype, ss=fine, clip=math.inf)
    assert adam_words(st)[0] == 1001 and not same_bits(p, p0)


# ---------------------------------------------------------------------------------------------------------------- 4. clip and scale
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
@pytest.mark.parametrize("gscale", [1.0, 1.0 / 128], ids=["gscale=1", "gscale=1/128"])
def test_adam_active_clip(gscale, decoupled):
    """clip_norm below the arena's norm (asserted): the bounds hold with the coefficient taken from the squared norm read back."""
    g0 = arena()[1]
    ss = device_sumsq(g0.to(DEV))
    coef = coef_of(ss, CLIP)
    assert coef < 1.0 and math.sqrt(float(ss)) > 1.0e3, float(ss)
    out = run_adam(HYPERS[1], 5, decoupled, torch.float16, gscale=gscale, ss=ss, clip=CLIP)
    check_arena(out, HYPERS[1], 5, decoupled, torch.float16, c=f32(gscale) * coef, what=f"adam clip gscale={gscale} decoupled={decoupled}")
    none = run_adam(HYPERS[1], 5, decoupled, torch.float16, gscale=gscale, ss=ss, clip=math.inf)
    assert not same_bits(out[2], none[2])                                    # the clip did act


@pytest.mark.parametrize("clip", [CLIP / 1024.0, math.inf], ids=["clip", "noclip"])
@pytest.mark.parametrize("lp_dtype", [None, torch.bfloat16], ids=["lp=None", "lp=bf16"])
def test_adam_with_a_loss_scale_state_is_the_static_call_at_a_power_of_two(lp_dtype, clip):
    """scale_state holding 1024: bit-equal to the call without it at gscale / 1024 and clip_norm * 1024 (both products are exact), as
    tc_sgd_step_multi_scaled is to tc_sgd_step_multi.  The arena's norm is 1.2e3, so CLIP / 1024 on the true norm is active."""
    from transception_amd.train import DynamicLossScale
    g0 = arena()[1]
    ss = device_sumsq(g0.to(DEV))
    state = DynamicLossScale(init_scale=1024.0).state(DEV)
    a = run_adam(HYPERS[1], 5, True, lp_dtype, gscale=1.0, ss=ss, clip=clip, scale_state=state)
    b = run_adam(HYPERS[1], 5, True, lp_dtype, gscale=1.0 / 1024.0, ss=ss, clip=clip * 1024.0)
    for x, y in zip(a, b):
        assert (x is None and y is None) or same_bits(x, y)
    assert not same_bits(a[0], arena()[0])


# ---------------------------------------------------------------------------------------------------------------- 5. tc_adam_advance
def test_adam_advance_counts_and_corrects():
    """1200 launches from t = 0 with betas (0.9, 0.999), the state copied aside on the device after each: word 0 is the count, words 1
    and 2 are within one float32 ulp of float32(1 - beta1^t) and float32(sqrt(1 - beta2^t)) formed in numpy float64, word 3 is 0.  Every
    97th launch sees an inf or a NaN sum and must leave all four words alone; every other one alternates a finite sum and no sum."""
    n = 1200
    st = torch.zeros(4, dtype=torch.float32, device=DEV)
    hist = torch.zeros(n, 4, dtype=torch.float32, device=DEV)
    ss = torch.zeros(1, dtype=torch.float32, device=DEV)
    sums = [(math.inf if (i // 97) % 2 else math.nan) if i % 97 == 96 else (None if i % 2 else 3.0e38) for i in range(n)]
    for i, s in enumerate(sums):
        if s is not None:
            ss.fill_(s)
        lib().tc_adam_advance(ptr(st), None if s is None else ptr(ss), 0.9, 0.999, stream())
        hist[i].copy_(st)
    h = hist.cpu()
    hi = h.view(torch.int32)
    t, worst = 0, 0.0
    for i, s in enumerate(sums):
        if s is None or math.isfinite(s):
            t += 1
        elif i:
            assert same_bits(h[i], h[i - 1]), i
        want1, want2 = np.float32(1.0 - np.float64(0.9) ** t), np.float32(np.sqrt(1.0 - np.float64(0.999) ** t))
        assert int(hi[i, 0]) == t and int(hi[i, 3]) == 0, (i, t, hi[i].tolist())
        e1, e2 = abs(float(h[i, 1]) - float(want1)) / float(np.spacing(want1)), abs(float(h[i, 2]) - float(want2)) / float(np.spacing(want2))
        worst = max(worst, e1, e2)
        assert e1 <= 1.0 and e2 <= 1.0, (i, t, float(h[i, 1]), float(want1), float(h[i, 2]), float(want2))
    assert t == n - sum(s is not None and not math.isfinite(s) for s in sums) == n - 12
    print(f"tc_adam_advance over {t} counted steps: worst bias-term error {worst:.2f} ulp")


# ---------------------------------------------------------------------------------------------------------------- 6. argument rules
def test_adam_argument_rules():
    p = torch.zeros(64, dtype=torch.float32, device=DEV)
    g, m, v = torch.ones_like(p), torch.zeros_like(p), torch.zeros_like(p)
    lp = torch.zeros(64, dtype=torch.bfloat16, device=DEV)
    sd = torch.tensor([0, 64], dtype=torch.int64, device=DEV)
    ss = torch.ones(1, dtype=torch.float32, device=DEV)
    st, scale = state_at(1), torch.tensor([2.0, 0.5, 0.0, 0.0], dtype=torch.float32, device=DEV)

    def call(nseg=1, betas=(0.9, 0.999), eps=1e-8, lp_=None, lp_dtype=0, sumsq=None, scale_state=None, state=st):
        lib().tc_adam_step_multi(ptr(p), ptr(g), ptr(m), ptr(v), ptr(sd), None, nseg, 64, 1e-3, None, betas[0], betas[1], eps, 0.0, 1, 1.0, ptr(sumsq),
                                 math.inf, ptr(lp_), lp_dtype, ptr(scale_state), ptr(state), stream())

    bad = [dict(betas=(1.0, 0.999)), dict(betas=(-0.1, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(0.9, -1e-3)), dict(betas=(math.nan, 0.9)),
           dict(eps=0.0), dict(eps=-1e-8), dict(nseg=0), dict(nseg=-3), dict(lp_=lp, lp_dtype=7), dict(state=None), dict(scale_state=scale)]
    for kw in bad:
        with pytest.raises(TcError, match="status -1"):
            call(**kw)
    for betas in ((1.0, 0.9), (0.9, 1.5), (-0.5, 0.9)):
        with pytest.raises(TcError, match="status -1"):
            lib().tc_adam_advance(ptr(st), None, betas[0], betas[1], stream())
    with pytest.raises(TcError, match="status -1"):
        lib().tc_adam_advance(None, None, 0.9, 0.999, stream())
    torch.cuda.synchronize()
    assert float(p.abs().max()) == 0.0 and same_bits(st, state_at(1))          # nothing ran
    call(lp_=lp, lp_dtype=TC_BF16, sumsq=ss, scale_state=scale)                # and the good call does
    torch.cuda.synchronize()
    assert float(p.abs().min()) > 0.0 and torch.equal(lp, p.to(torch.bfloat16))


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


def _arena_masks(opt, n):
    """(live mask, per-element decay in float64) of the optimiser's segment table, on the device."""
    live, wd = torch.zeros(n, dtype=torch.bool, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV)
    for off, ln, d in opt._segs3():
        live[off:off + ln] = True
        wd[off:off + ln] = f32(d)
    return live, wd


# ---------------------------------------------------------------------------------------------------------------- 7. eager steps vs torch
def test_eager_model_steps_match_torch_adamw():
    """Three eager fp32 train_steps of the seeded model (64 x 64, B = 2) with FusedAdamW(no_decay="norm_bias").  After each, the gradients
    the model exposes go to the host and float64 torch.optim.AdamW -- two parameter groups by the same predicate, its state set to the
    moments before the step -- acts on a float64 copy of the parameters before the step.  Every tensor with a gradient agrees within the
    weight bound of the kernel test evaluated on that tensor; every tensor without one is bit-identical to its initial value.
    torch works from the double betas where the kernel holds float(beta), float(1 - beta) and float32 bias words: at most 0.2 u, 0.8 u and
    0.5 u + 0.5 u relative, inside the factor of two that the bound's K carries."""
    from transception_amd.train import FusedAdamW, SegLoss, train_step
    M = _fresh(torch.float32)
    x, y = _batch()
    lr, betas, eps, wd = HYPERS[0]
    opt = FusedAdamW(M, lr=lr, betas=betas, eps=eps, weight_decay=wd, no_decay="norm_bias")
    M._ensure_flat(torch.device(DEV))
    init = M.flat_parameters().clone()
    index = {n: M._index[n] for n, _ in M.named_parameters()}
    n_el = init.numel()
    graded = None
    for t in range(1, 4):
        w_in = M.flat_parameters().cpu()
        m_in = opt.m.cpu() if opt.m is not None else torch.zeros(n_el)
        v_in = opt.v.cpu() if opt.v is not None else torch.zeros(n_el)
        train_step(M, SegLoss(9), opt, x, y)
        torch.cuda.synchronize()
        assert opt.device_step() == t
        grads = {n: p.grad.detach().cpu() for n, p in M.named_parameters() if p.grad is not None}
        graded = set(grads) if graded is None else graded
        assert set(grads) == graded and 0 < len(graded) < len(index)
        # float64 torch.optim.AdamW on views of flat float64 copies: the step writes the reference in place
        w64, m64, v64, g64 = w_in.double(), m_in.double(), v_in.double(), torch.zeros(n_el, dtype=torch.float64)
        groups = {True: [], False: []}
        params = {}
        for n in sorted(graded):
            off, shape = index[n]
            k = math.prod(shape)
            q = torch.nn.Parameter(w64[off:off + k].view(shape))
            g64[off:off + k] = grads[n].double().reshape(-1)
            q.grad = g64[off:off + k].view(shape)
            groups[len(shape) <= 1].append(q)
            params[n] = q
        ref = torch.optim.AdamW([{"params": groups[False], "weight_decay": f32(wd)}, {"params": groups[True], "weight_decay": 0.0}],
                                lr=f32(lr), betas=betas, eps=f32(eps))
        for n, q in params.items():
            off, shape = index[n]
            k = math.prod(shape)
            ref.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": m64[off:off + k].view(shape), "exp_avg_sq": v64[off:off + k].view(shape)}
        ref.step()
        # the bound, per element on the device, then judged tensor by tensor
        live, wd_el = _arena_masks(opt, n_el)
        bc = bias_terms(*betas, t)
        _, _, _, Am, Av, den = adam_ref(w_in.to(DEV), g64.to(DEV), m_in.to(DEV), v_in.to(DEV), f32(lr), *betas32(*betas), f32(eps), wd_el, bc[0], bc[1], True)
        bw = bounds(w_in.to(DEV), f32(lr), bc[0], Am, Av, den)[2]
        ratio = ((M.flat_parameters().double() - w64.to(DEV)).abs() / (bw + 1e-300)).cpu()     # (error 0 against a bound of 0 is 0)
        worst, worst_name = 0.0, None
        for n in sorted(graded):
            off, shape = index[n]
            r = float(ratio[off:off + math.prod(shape)].max())
            if r > worst:
                worst, worst_name = r, n
        print(f"step {t}: {len(graded)} tensors with a gradient, worst error / bound {worst:.3f} ({worst_name})")
        assert worst <= 1.0, (t, worst_name, worst)
        now = M.flat_parameters()
        for n in index:
            if n not in graded:                                              # decoupled decay must not reach the grad-less tensors
                off, shape = index[n]
                assert torch.equal(now[off:off + math.prod(shape)], init[off:off + math.prod(shape)]), n
    assert len(index) - len(graded) == 332


# ---------------------------------------------------------------------------------------------------------------- 8. the captured step
@pytest.mark.parametrize("split", [False, True], ids=["one-graph", "split"])
def test_captured_step_reads_the_step_count_from_the_device(split):
    """bf16: one eager step, then GraphedStep(warmup=0) and three replays.  Each replay's new p, m, v are checked against adam_ref from the
    snapshot before it and the gradient arena after it, with t = 2, 3, 4 -- a t baked at capture would be off by 19 % in lr / bc1 between
    t = 4 and 5, far outside the bounds.  The working copy is the rounding of the parameters, the state word reads 4, and the graph has
    one kernel node more than FusedSGD's for the same configuration (tc_adam_advance)."""
    from transception_amd.train import FusedAdamW, FusedSGD, GraphedStep, SegLoss, train_step
    x, y = _batch()
    lr, betas, eps, wd = HYPERS[0]
    hyper = HYPERS[0]
    M = _fresh(torch.bfloat16)
    opt = FusedAdamW(M, lr=lr, betas=betas, eps=eps, weight_decay=wd, no_decay="norm_bias")
    loss_fn = SegLoss(9)
    train_step(M, loss_fn, opt, x, y)
    step = GraphedStep(M, loss_fn, opt, x, y, None, warmup=0, force_split=split)
    assert opt.device_step() == 1                                            # capturing runs nothing
    live, wd_el = _arena_masks(opt, M.flat_parameters().numel())
    ptrs = (opt.m.data_ptr(), opt.v.data_ptr(), opt._adam_state.data_ptr())
    for t in (2, 3, 4):
        before = (M.flat_parameters().clone(), opt.m.clone(), opt.v.clone())
        loss = step()[0]
        torch.cuda.synchronize()
        assert math.isfinite(float(loss))
        words = adam_words(opt._adam_state)
        assert words[0] == t and words[3] == 0, words
        check_update((M.flat_parameters(), opt.m, opt.v), (before[0], M.flat_gradients(), before[1], before[2]), live, hyper,
                     (words[1], words[2]), True, 1.0, wd_el[live], f"captured split={split} t={t}")
        assert torch.equal(M._flat_lp[live], M.flat_parameters()[live].to(torch.bfloat16))
        assert torch.equal(M.flat_parameters()[~live], before[0][~live])
    assert opt.device_step() == 4 and ptrs == (opt.m.data_ptr(), opt.v.data_ptr(), opt._adam_state.data_ptr()) and not opt.last_step_skipped()
    nodes = step.kernel_nodes()
    del step
    S = _fresh(torch.bfloat16)
    sgd = FusedSGD(S, lr=0.05)
    train_step(S, loss_fn, sgd, x, y)
    want = GraphedStep(S, loss_fn, sgd, x, y, None, warmup=0, force_split=split).kernel_nodes()
    print(f"kernel nodes, split={split}: AdamW {nodes}, SGD {want}")
    assert nodes is not None and want is not None and nodes == want + 1


# ---------------------------------------------------------------------------------------------------------------- 9. the dynamic loss scale
@pytest.mark.parametrize("split", [False, True], ids=["one-graph", "split"])
def test_captured_adamw_step_under_the_dynamic_loss_scale(split):
    """fp16 with DynamicLossScale(4096): a scale of 2^40 loaded IN PLACE makes the next replay overflow by arithmetic (an inf in a sum): p, m, v,
    the working copy and t stay bit-equal, the scale halves and last_step_skipped() reports it; with 4096 loaded back the same graph
    takes a step and t advances."""
    from transception_amd.train import DynamicLossScale, FusedAdamW, GraphedStep, SegLoss, train_step
    M = _fresh(torch.float16)
    x, y = _batch()
    scaler = DynamicLossScale(init_scale=4096.0, growth_interval=1000)
    loss_fn, opt = SegLoss(9, loss_scale=scaler), FusedAdamW(M, lr=1e-3, no_decay="norm_bias")
    train_step(M, loss_fn, opt, x, y)
    step = GraphedStep(M, loss_fn, opt, x, y, None, warmup=0, force_split=split)
    step()
    torch.cuda.synchronize()
    assert opt.device_step() == 2 and not opt.last_step_skipped() and scaler.state_dict() == {"scale": 4096.0, "growth_tracker": 2, "skipped": 0}
    sptr = scaler.state(DEV).data_ptr()
    scaler.load_state_dict({"scale": 2.0 ** 40, "growth_tracker": 2, "skipped": 0})
    assert scaler.state(DEV).data_ptr() == sptr
    before = (M.flat_parameters().clone(), opt.m.clone(), opt.v.clone(), M._flat_lp.clone(), opt._adam_state.clone())
    step()
    torch.cuda.synchronize()
    assert all(same_bits(a, b) for a, b in zip((M.flat_parameters(), opt.m, opt.v, M._flat_lp, opt._adam_state), before))
    assert scaler.state_dict() == {"scale": 2.0 ** 39, "growth_tracker": 0, "skipped": 1} and opt.last_step_skipped() and opt.device_step() == 2
    scaler.load_state_dict({"scale": 4096.0})
    step()
    torch.cuda.synchronize()
    assert opt.device_step() == 3 and not opt.last_step_skipped()
    assert not torch.equal(M.flat_parameters(), before[0]) and bool(torch.isfinite(M.flat_parameters()).all()) and bool(torch.isfinite(opt.v).all())
    assert scaler.state_dict() == {"scale": 4096.0, "growth_tracker": 1, "skipped": 0}


# ---------------------------------------------------------------------------------------------------------------- 10. state_dict
def test_state_dict_round_trip_in_place():
    """Two fp32 models from the same seed train two steps and then two more on two other batches: two runs of the same path, whose
    element-wise difference is the path's own spread (the weight-gradient atomics make a step order-dependent).  The first model's
    optimiser state was saved after step two; its weights and that state are then loaded back IN PLACE (same data_ptrs) and the two
    batches replayed.  Bit-equal runs demand a bit-equal replay; otherwise the replay lies within 4 x the spread of either run, the rule
    of test_dynamic_step_agrees_with_the_static_path."""
    from transception_amd.train import FusedAdamW, SegLoss, train_step
    x, y = _batch()
    batches = [(x, y), (x, y), (x.flip(-1).contiguous(), y.flip(-1).contiguous()), (x.flip(-2).contiguous(), y.flip(-2).contiguous())]
    loss_fn = SegLoss(9)
    runs, saved = [], None
    for k in range(2):
        M = _fresh(torch.float32)
        opt = FusedAdamW(M, lr=1e-3, no_decay="norm_bias")
        for i, (bx, by) in enumerate(batches):
            if i == 2 and k == 0:
                saved = (opt.state_dict(), M.flat_parameters().clone())
            train_step(M, loss_fn, opt, bx, by)
        torch.cuda.synchronize()
        runs.append((M.flat_parameters().clone(), opt.m.clone(), opt.v.clone()))
        if k == 0:
            first = (M, opt)
    M, opt = first
    sd, w2 = saved
    assert sd["step"] == 2 and set(sd) == {"step", "exp_avg", "exp_avg_sq"} and sd["exp_avg"].data_ptr() != opt.m.data_ptr()
    assert opt.device_step() == 4 and not torch.equal(sd["exp_avg"], opt.m)
    ptrs = (opt.m.data_ptr(), opt.v.data_ptr(), opt._adam_state.data_ptr(), M.flat_parameters().data_ptr())
    opt.load_state_dict(sd)
    M.flat_parameters().copy_(w2)
    M.invalidate_working_copy()
    assert ptrs == (opt.m.data_ptr(), opt.v.data_ptr(), opt._adam_state.data_ptr(), M.flat_parameters().data_ptr())
    assert opt.device_step() == 2 and torch.equal(opt.m, sd["exp_avg"]) and torch.equal(opt.v, sd["exp_avg_sq"])
    for bx, by in batches[2:]:
        train_step(M, loss_fn, opt, bx, by)
    torch.cuda.synchronize()
    assert opt.device_step() == 4
    again = (M.flat_parameters(), opt.m, opt.v)
    for k, name in enumerate(("parameters", "exp_avg", "exp_avg_sq")):
        a, b, d = runs[0][k], runs[1][k], again[k]
        spread = float((a - b).abs().max())
        dist = max(float((d - a).abs().max()), float((d - b).abs().max()))
        print(f"{name}: run-run spread {spread:.3e}, replay-run {dist:.3e}, bit-equal runs: {torch.equal(a, b)}")
        if torch.equal(a, b):
            assert torch.equal(d, a), (name, dist)
        else:
            assert dist <= 4.0 * spread, (name, dist, spread)


# ---------------------------------------------------------------------------------------------------------------- 11. the trainer
@pytest.mark.parametrize("graphed", [True, False], ids=["graphed", "eager"])
def test_trainer_with_adamw(tmp_path, graphed):
    """The tiny synthetic set of the trainer tests, fp16 storage, optimizer="adamw" with base_lr 1e-3, no decay on norms and biases and
    the dynamic loss scale: finite losses, weights finite and moved, and the device's step count is the iterations minus the skipped
    updates (every iteration logs, so every skip is seen)."""
    from transception_amd import data as D
    from transception_amd.trainer import TrainConfig, trainer_synapse
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=2, slices_per_case=6, size=128, seed=11)
    M = _fresh(torch.float16)
    M._ensure_flat(torch.device(DEV))
    init = M.flat_parameters().clone()
    cfg = TrainConfig(root_path=base, list_dir=lists, max_epochs=3, batch_size=4, img_size=64, seed=5, model_name="tiny", graphed=graphed,
                      optimizer="adamw", base_lr=1e-3, no_decay="norm_bias", loss_scale="dynamic")
    lines = []
    hist = trainer_synapse(cfg, M, str(tmp_path / "snap"), log=lines.append)
    assert hist["iterations"] == 9 and len(hist["loss"]) == 9 and all(math.isfinite(v) for v in hist["loss"]), hist["loss"]
    p = M.flat_parameters()
    assert bool(torch.isfinite(p).all()) and not torch.equal(p, init)
    nskip = sum("update SKIPPED" in l for l in lines)
    print(f"trainer adamw graphed={graphed}: losses {hist['loss']}, {nskip} skipped, loss scale {hist['loss_scale']}")
    assert hist["optimizer_step"] == 9 - nskip and nskip < 9
    assert hist["loss_scale"][-1] == 65536.0 / 2 ** nskip

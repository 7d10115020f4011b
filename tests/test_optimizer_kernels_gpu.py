"""The optimizer kernels of csrc/train.hip -- tc_sgd_step_multi, tc_sgd_step, tc_grad_sumsq, tc_fill_f32 -- each against a float64
reference (tests/layout_ref.py: torch.optim.SGD after clip_grad_norm_, and its closed form), with bounds that are derived, not measured.

u = 2^-24 is float32's unit roundoff.  With A = |g gscale coef| + |wd w| + |mom m| taken from the reference:

  momentum   |b - b_ref|   <= 16 u A
  weights    |w' - w'_ref| <= 4 u |w| + 16 u lr A

The kernel rounds at most four times per result (g * (gscale coef) + wd w and mom m + d are one fused multiply-add each, or two
operations; w - lr b likewise), gscale * coef carries the correctly rounded sqrtf, the + 1e-6, the division and the product (4 u), and the
hyper-parameters reach the kernel as float32 (the reference takes the same float32 values).  That is below 8 u A; 16 leaves a factor of
two.  The clip coefficient of the reference comes from the squared norm READ BACK from the device, so the update kernel is judged on its
own; the reduction has its own test:

  tc_grad_sumsq   |s - s_ref| <= 1100 u s_ref

All terms are positive, so the relative error is at most u times the additions on the longest path: the per-thread chain (n / 4 float4
per 256 x blocks threads, four additions each: 36 for the largest n here) + 9 for the wave and block fold + one atomic per block, at most
1024 blocks."""
import math

import pytest
import torch

from layout_ref import clip_coef, sgd_ref, sgd_torch_ref

pytestmark = pytest.mark.gpu

from transception_amd._lib import TC_BF16, TC_F16, TcError, lib  # noqa: E402

DEV = "cuda:0"
U = 2.0 ** -24
N_ARENA = 700000
SEGS = [(0, 96),                  # 16-byte path, one pass
        (104, 37),                # odd length: element path
        (144, 524296),            # 16-byte path, more than one pass of its 256 blocks x 256 threads x 4 elements
        (524448, 70001)]          # element path, more than one pass of 256 x 256
SMALL = SEGS[:2]
SENT_P, SENT_G, SENT_M = 1234.5, -3.0, -77.25
HYPERS = [(0.05, 0.9, 1e-4),      # the workload's
          (0.05, 0.5, 1e-2)]      # every term large enough that misplacing it cannot hide
LP = {None: 0, torch.bfloat16: TC_BF16, torch.float16: TC_F16}
CLIP = 400.0                      # the arena's gradient norm is about 1.2e3 (asserted): active


def f32(v):
    """The float32 value the kernel receives for a host float."""
    return float(torch.tensor(v, dtype=torch.float32))


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def ptr(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def ibits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(ibits(a), ibits(b))


def _live(n, segs):
    live = torch.zeros(n, dtype=torch.bool)
    for off, ln in segs:
        live[off:off + ln] = True
    return live


_ARENA = {}


def arena(n=N_ARENA, segs=SEGS, seed=7):
    """(parameters, gradient, momentum, live mask) on the host: seeded normals inside the segments, a sentinel everywhere else.  Built once."""
    key = (n, tuple(segs), seed)
    if key not in _ARENA:
        g = torch.Generator().manual_seed(seed)
        live = _live(n, segs)
        p, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
        p[~live], gr[~live], m[~live] = SENT_P, SENT_G, SENT_M
        _ARENA[key] = (p, gr, m, live)
    return _ARENA[key]


def device_sumsq(gd):
    ss = torch.zeros(1, dtype=torch.float32, device=DEV)
    lib().tc_grad_sumsq(ptr(gd), gd.numel(), ptr(ss), stream())
    torch.cuda.synchronize()
    return ss


def check_update(p_new, b_new, w, g, m, live, lr, mom, wd, gscale, first, coef, what=""):
    """The two derived bounds of the module docstring on the live elements; prints the worst ratio before it asserts."""
    w_ref, b_ref, A = sgd_ref(w[live], g[live], m[live], f32(lr), f32(mom), f32(wd), gscale, first, coef)
    eb = (b_new.cpu()[live].double() - b_ref).abs()
    ew = (p_new.cpu()[live].double() - w_ref).abs()
    bound_b = 16 * U * A
    bound_w = 4 * U * w[live].double().abs() + 16 * U * f32(lr) * A
    rb, rw = float((eb / bound_b).max()), float((ew / bound_w).max())
    print(f"{what}: worst error / bound: momentum {rb:.3f}, weights {rw:.3f}")
    assert bool((eb <= bound_b).all()), (what, "momentum", rb)
    assert bool((ew <= bound_w).all()), (what, "weights", rw)


# ---------------------------------------------------------------------------------------------------------------- tc_sgd_step_multi
def run_multi(p0, g0, m0, segs, lr, mom, wd, gscale, first, ss, clip, lp_dtype, lr_on_device=True):
    p, gd, buf = p0.to(DEV), g0.to(DEV), m0.to(DEV)
    lp = p0.to(lp_dtype).to(DEV) if lp_dtype is not None else None
    sd = torch.tensor([v for s in segs for v in s], dtype=torch.int64, device=DEV)
    lr_dev = torch.full((1,), lr, dtype=torch.float32, device=DEV) if lr_on_device else None
    lib().tc_sgd_step_multi(ptr(p), ptr(gd), ptr(buf), ptr(sd), len(segs), max(n for _, n in segs), 999.0 if lr_on_device else lr, ptr(lr_dev),
                            mom, wd, gscale, int(first), ptr(ss), clip, ptr(lp), LP[lp_dtype], stream())
    torch.cuda.synchronize()
    return p, gd, buf, lp


def check_multi(out, p0, g0, m0, live, lp_dtype, hyper, gscale, first, coef, what):
    p, gd, buf, lp = out
    check_update(p, buf, p0, g0, m0, live, *hyper, gscale, first, coef, what)
    # everything outside the segments, in every buffer, bit for bit
    dead = ~live
    assert same_bits(p.cpu()[dead], p0[dead]) and same_bits(buf.cpu()[dead], m0[dead]) and same_bits(gd, g0)
    assert bool((p.cpu()[live] != p0[live]).any())
    if lp_dtype is not None:
        assert torch.equal(lp.cpu()[live], p.cpu()[live].to(lp_dtype)) and same_bits(lp.cpu()[dead], p0.to(lp_dtype)[dead])


@pytest.mark.parametrize("lp_dtype", [None, torch.bfloat16, torch.float16], ids=["lp=None", "lp=bf16", "lp=f16"])
@pytest.mark.parametrize("gscale", [1.0, 1.0 / 128], ids=["gscale=1", "gscale=1/128"])
@pytest.mark.parametrize("clip", [math.inf, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("first", [1, 0], ids=["first", "later"])
@pytest.mark.parametrize("hyper", HYPERS, ids=["workload", "large-terms"])
def test_sgd_step_multi(hyper, first, clip, gscale, lp_dtype):
    """Four segments (both paths, one pass and several) of a 700 k arena against the float64 reference within the derived bounds; the
    host's lr is 999 and the real one sits in lr_dev; whatever lies outside the segments is bit-unchanged in all four buffers."""
    p0, g0, m0, live = arena()
    ss = device_sumsq(g0.to(DEV))
    coef = clip_coef(float(ss), clip)
    assert (coef < 1.0) == (clip != math.inf), (float(ss), clip)           # the clip is active exactly when asked for
    out = run_multi(p0, g0, m0, SEGS, *hyper, gscale, first, ss, clip, lp_dtype)
    check_multi(out, p0, g0, m0, live, lp_dtype, hyper, gscale, first, coef, f"multi {hyper} first={first} clip={clip} gscale={gscale}")


@pytest.mark.parametrize("first", [1, 0], ids=["first", "later"])
def test_sgd_step_multi_host_lr_and_no_clip_pointer(first):
    """lr_dev = None: the host's lr is the one used.  clip_sumsq = None: no coefficient at all, whatever clip_norm says."""
    p0, g0, m0, live = arena()
    hyper = HYPERS[1]
    out = run_multi(p0, g0, m0, SEGS, *hyper, 0.25, first, None, CLIP, torch.bfloat16, lr_on_device=False)
    check_multi(out, p0, g0, m0, live, torch.bfloat16, hyper, 0.25, first, 1.0, f"multi host lr first={first}")


@pytest.mark.parametrize("lp_dtype", [None, torch.bfloat16, torch.float16], ids=["lp=None", "lp=bf16", "lp=f16"])
@pytest.mark.parametrize("bad", [math.inf, math.nan], ids=["inf", "nan"])
def test_sgd_step_multi_skips_on_a_non_finite_norm(bad, lp_dtype):
    p0, g0, m0, _ = arena()
    ss = torch.full((1,), bad, dtype=torch.float32, device=DEV)
    for clip in (CLIP, math.inf):
        p, gd, buf, lp = run_multi(p0, g0, m0, SEGS, *HYPERS[1], 1.0, 0, ss, clip, lp_dtype)
        assert same_bits(p, p0) and same_bits(buf, m0) and same_bits(gd, g0) and (lp is None or same_bits(lp, p0.to(lp_dtype)))


# ---------------------------------------------------------------------------------------------------------------- tc_sgd_step
@pytest.mark.parametrize("first", [1, 0], ids=["first", "later"])
@pytest.mark.parametrize("n", [5, 1200000])
def test_sgd_step_single_segment(n, first):
    """n = 5 and n = 1 200 000 (more than one pass of 4096 blocks x 256 threads), gscale = 1/4, same reference and bounds; the eight
    elements after the segment keep their sentinel.  n = 5 takes its lr from the host, the large one from lr_dev (host: 999)."""
    lr, mom, wd = HYPERS[1]
    g = torch.Generator().manual_seed(n + first)
    p0, g0, m0 = torch.randn(n + 8, generator=g), torch.randn(n + 8, generator=g), torch.randn(n + 8, generator=g)
    p0[n:], g0[n:], m0[n:] = SENT_P, SENT_G, SENT_M
    p, gd, buf = p0.to(DEV), g0.to(DEV), m0.to(DEV)
    lr_dev = torch.full((1,), lr, dtype=torch.float32, device=DEV) if n > 5 else None
    lib().tc_sgd_step(ptr(p), ptr(gd), ptr(buf), n, 999.0 if n > 5 else lr, ptr(lr_dev), mom, wd, 0.25, first, stream())
    torch.cuda.synchronize()
    live = _live(n + 8, [(0, n)])
    check_update(p, buf, p0, g0, m0, live, lr, mom, wd, 0.25, first, 1.0, f"single n={n} first={first}")
    assert same_bits(p.cpu()[n:], p0[n:]) and same_bits(buf.cpu()[n:], m0[n:]) and same_bits(gd, g0)


# ---------------------------------------------------------------------------------------------------------------- tc_grad_sumsq
@pytest.mark.parametrize("n", [4, 200, 2097156])
def test_grad_sumsq(n):
    """Against the float64 sum of squares within 1100 u relative (module docstring); n = 2 097 156 floats is more than one pass of the
    reduction's blocks.  A second call adds to the same word; the eight elements behind the buffer are not read (an inf sits there)."""
    g = torch.randn(n + 8, generator=torch.Generator().manual_seed(n))
    g[n:] = math.inf
    gd = g.to(DEV)
    want = float((g[:n].double() ** 2).sum())
    ss = torch.zeros(1, dtype=torch.float32, device=DEV)
    lib().tc_grad_sumsq(ptr(gd), n, ptr(ss), stream())
    torch.cuda.synchronize()
    one = float(ss)
    print(f"sumsq n={n}: relative error {abs(one - want) / want:.3e} (bound {1100 * U:.3e})")
    assert abs(one - want) <= 1100 * U * want
    lib().tc_grad_sumsq(ptr(gd), n, ptr(ss), stream())
    torch.cuda.synchronize()
    assert abs(float(ss) - 2 * want) <= 1100 * U * 2 * want               # (the same count of additions bounds either call's path)


def test_grad_sumsq_refusals_and_overflow():
    gd = torch.ones(64, dtype=torch.float32, device=DEV)
    ss = torch.zeros(1, dtype=torch.float32, device=DEV)
    with pytest.raises(TcError, match="status -1"):
        lib().tc_grad_sumsq(ptr(gd), 6, ptr(ss), stream())                  # n % 4 != 0
    with pytest.raises(TcError, match="status -1"):
        lib().tc_grad_sumsq(ptr(gd, 1), 8, ptr(ss), stream())               # not 16-byte aligned
    torch.cuda.synchronize()
    assert float(ss) == 0.0
    gd[37] = math.inf
    lib().tc_grad_sumsq(ptr(gd), 64, ptr(ss), stream())
    torch.cuda.synchronize()
    assert not math.isfinite(float(ss))


# ---------------------------------------------------------------------------------------------------------------- tc_fill_f32
@pytest.mark.parametrize("n", [1, 600001])
def test_fill_f32(n):
    """Exact, with eight sentinels on both sides; 600 001 is more than one pass of 2048 blocks x 256 threads."""
    buf = torch.full((n + 16,), SENT_P, dtype=torch.float32, device=DEV)
    for v in (2.5, -0.0):
        lib().tc_fill_f32(ptr(buf, 8), n, v, stream())
        torch.cuda.synchronize()
        want = torch.full((n + 16,), SENT_P, dtype=torch.float32)
        want[8:8 + n] = v
        assert same_bits(buf, want)


# ---------------------------------------------------------------------------------------------------------------- three steps
@pytest.mark.parametrize("lp_dtype", [None, torch.float16], ids=["lp=None", "lp=f16"])
def test_three_step_trajectory(lp_dtype):
    """Three steps on the two small segments, momentum carried by the kernel and `first` on step one only, against three steps of float64
    torch.optim.SGD with clip_grad_norm_.  The gradients lie on a grid (multiples of 1/8, |v| <= 4), so their squared norm is exact in
    float32 whatever the order of the additions and clip_grad_norm_ sees the very norm the device computed (asserted).  Each step's bound
    is applied to that step's own inputs: the reference restarts from the device's previous output, so errors do not compound."""
    n, (lr, mom, wd), clip = 200, HYPERS[1], 5.0
    p0, _, m0, live = arena(n, SMALL, seed=11)
    p, buf = p0.to(DEV), m0.to(DEV)
    lp = p0.to(lp_dtype).to(DEV) if lp_dtype is not None else None
    sd = torch.tensor([v for s in SMALL for v in s], dtype=torch.int64, device=DEV)
    lr_dev = torch.full((1,), lr, dtype=torch.float32, device=DEV)
    gen = torch.Generator().manual_seed(5)
    for step in range(3):
        g = (torch.randn(n, generator=gen) * 16).round().clamp(-32, 32) / 8
        g[~live] = 0.0                                                      # parameters without a gradient hold zeros in the arena
        gd = g.to(DEV)
        w_in, m_in = p.cpu(), buf.cpu()
        ss = device_sumsq(gd)
        assert float(ss) == float((g.double() ** 2).sum()) and math.sqrt(float(ss)) > clip
        lib().tc_sgd_step_multi(ptr(p), ptr(gd), ptr(buf), ptr(sd), len(SMALL), max(k for _, k in SMALL), 999.0, ptr(lr_dev), mom, wd, 1.0,
                                int(step == 0), ptr(ss), clip, ptr(lp), LP[lp_dtype], stream())
        torch.cuda.synchronize()
        w_ref, b_ref = sgd_torch_ref(w_in[live], g[live], m_in[live], f32(lr), f32(mom), f32(wd), 1.0, step == 0, clip)
        _, _, A = sgd_ref(w_in[live], g[live], m_in[live], f32(lr), f32(mom), f32(wd), 1.0, step == 0, clip_coef(float(ss), clip))
        eb, ew = (buf.cpu()[live].double() - b_ref).abs(), (p.cpu()[live].double() - w_ref).abs()
        bound_b, bound_w = 16 * U * A, 4 * U * w_in[live].double().abs() + 16 * U * f32(lr) * A
        print(f"step {step}: worst error / bound: momentum {float((eb / bound_b).max()):.3f}, weights {float((ew / bound_w).max()):.3f}")
        assert bool((eb <= bound_b).all()) and bool((ew <= bound_w).all()), step
        assert same_bits(p.cpu()[~live], p0[~live]) and same_bits(buf.cpu()[~live], m0[~live])
        if lp is not None:
            assert torch.equal(lp.cpu()[live], p.cpu()[live].to(lp_dtype)) and same_bits(lp.cpu()[~live], p0.to(lp_dtype)[~live])
        if step == 0:                                                       # `first`: the momentum it was handed is replaced, not blended
            assert bool((buf.cpu()[live] != m_in[live]).all())

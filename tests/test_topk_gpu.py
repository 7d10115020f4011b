"""Top-k (hard-pixel) cross-entropy on the MI355X: tc_topk_select alone against NumPy on the bit patterns, the tc_seg_loss_*_topk entries
(include/transception_topk.h) against the float64 reference of tests/topk_ref.py, SegLoss(ce_topk), the captured step and the trainer.

Bounds.  The select: n, k, n_gt, n_eq and the bits of t are equalities; S within (n + 1) 2^-52 relative of math.fsum (any order of adding n
non-negative doubles stays within (n - 1) 2^-53); f equal to (k - n_gt) / n_eq in double; sums[0] within one fp32 rounding (2^-23 relative) of
the double expression.  Forward values: 1e-6 max(1, v) against float64 on the stored-precision logits.  The three scalars: 2e-6 max(1, |ref|).
The gradient: 1e-8 + 1e-4 (|CE part| + |overlap part|) per element.  The loss cases assert their own precondition: the reference's k-th and
(k + 1)-th largest values differ by at least 1e-4 relative (about 1000 fp32 roundings), so the fp32 and the float64 selections coincide; the
seeds below are pinned so that it holds in every case."""
import math
import re

import numpy as np
import pytest
import torch

from topk_ref import pixel_values, reference, reference_ranks, topk_k

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
II = 255
OFF = -2 ** 31                                  # TC_IGNORE_NONE
DICE, TVERSKY = 0, 1
CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
SHAPES = [(2, 9, 16, 16), (2, 9, 11, 11), (1, 2, 5, 7)]
SEED = {(2, 9, 16, 16): 7, (2, 9, 11, 11): 7, (1, 2, 5, 7): 1}          # pinned: see the module docstring and _case
FRACS = [0.1, 0.25, 0.5, 1.0]
COMBOS = [(wt, ig, gm) for wt in (False, True) for ig in (False, True) for gm in (0.0, 2.0)]
TOPK_ENTRIES = ("tc_seg_loss_fwd_topk", "tc_topk_select", "tc_seg_loss_value_topk", "tc_seg_loss_bwd_topk")


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _lib():
    from transception_amd._lib import lib
    return lib()


# ---------------------------------------------------------------------------------------------------------------- 1. the select alone
GUARD = 33                                      # floats before and after the map: the map's base is misaligned by 4 bytes


class Sel:
    """One tc_topk_select call with guard regions around values, state and work, the work buffer pre-filled with 0xFF bytes."""

    def __init__(self, values: np.ndarray):
        n = values.size
        self.n = n
        buf = np.full(n + 2 * GUARD, 3.0e38, dtype=np.float32)                     # a guard that is read would be counted, at the very top
        buf[GUARD:GUARD + n] = values
        self.vbuf = torch.from_numpy(buf).to(DEV)
        self.values = self.vbuf[GUARD:GUARD + n]
        assert self.values.data_ptr() % 8 == 4
        self.sbuf = torch.full((8 + 16,), -7.0, dtype=torch.float64, device=DEV)
        self.state = self.sbuf[8:16]
        self.wb = _lib().tc_topk_work_bytes()
        self.wbuf = torch.full((self.wb + 128,), 0xA5, dtype=torch.uint8, device=DEV)
        self.work = self.wbuf[64:64 + self.wb]
        self.sums = torch.full((28,), 5.0, device=DEV)

    def run(self, frac, inv_world=1.0):
        self.work.fill_(0xFF)
        self.state[0:1].fill_(frac)
        _lib().tc_topk_select(self.values.data_ptr(), self.n, self.state.data_ptr(), self.sums.data_ptr(), inv_world, self.work.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert bool((self.sbuf[:8] == -7.0).all()) and bool((self.sbuf[16:] == -7.0).all())
        assert bool((self.wbuf[:64] == 0xA5).all()) and bool((self.wbuf[64 + self.wb:] == 0xA5).all())
        assert bool((self.sums[1:] == 5.0).all())                                 # only sums[0] is the select's
        assert bool((self.vbuf[:GUARD] == 3.0e38).all()) and bool((self.vbuf[GUARD + self.n:] == 3.0e38).all())
        return self.state.cpu().numpy().copy(), self.sums[:1].cpu().numpy().copy()


def expected_select(values: np.ndarray, frac: float, inv_world: float = 1.0):
    """(n, k, n_gt, n_eq, bits of t, S, f, CE inv_world) from NumPy on the uint32 view; every entry with the sign bit set is not counted."""
    u = values.view(np.uint32)
    counted = u < 0x80000000
    c, cv = u[counted], values[counted].astype(np.float64)
    n = int(c.size)
    if n == 0:
        return 0, 0, 0, 0, 0, 0.0, 0.0, 0.0
    k = max(1, min(n, math.ceil(frac * n)))
    tb = int(np.sort(c)[n - k])
    above = c > tb
    n_gt, n_eq = int(above.sum()), int((c == tb).sum())
    top = cv[above]
    S = math.fsum(top.tolist()) if bool(np.isfinite(top).all()) else float(top.sum())
    t = float(np.array([tb], dtype=np.uint32).view(np.float32)[0])
    with np.errstate(all="ignore"):
        ce = float((np.float64(S) + np.float64(k - n_gt) * np.float64(t)) / np.float64(k) * np.float64(inv_world))
    return n, k, n_gt, n_eq, tb, S, (k - n_gt) / n_eq, ce


def _same(a: float, b: float) -> bool:
    return (math.isnan(a) and math.isnan(b)) or a == b


def check_select(values, frac, state, s0, what, inv_world=1.0):
    n, k, n_gt, n_eq, tb, S, f, ce = expected_select(values, frac, inv_world)
    assert state[0] == frac, what                                                 # the caller's word is read, not written
    assert (state[1], state[2], state[3], state[4]) == (n, k, n_gt, n_eq), (what, state.tolist(), (n, k, n_gt, n_eq))
    got_t = np.array([state[5]], dtype=np.float64).astype(np.float32)
    assert float(got_t[0]) == state[5] or math.isnan(state[5]), what              # a float widened exactly
    if n:
        assert int(got_t.view(np.uint32)[0]) == tb or (math.isnan(state[5]) and tb > 0x7f800000), (what, hex(int(got_t.view(np.uint32)[0])), hex(tb))
    if math.isfinite(S):
        assert abs(state[6] - S) <= (n + 1) * 2.0 ** -52 * abs(S), (what, state[6], S)
    else:
        assert _same(state[6], S), (what, state[6], S)
    assert state[7] == f, (what, state[7], f)
    got = float(s0[0])
    with np.errstate(all="ignore"):
        want32 = float(np.float32(ce))
    if math.isfinite(ce) and math.isfinite(want32):
        assert abs(got - ce) <= max(2.0 ** -23 * abs(ce), 2.0 ** -149), (what, got, ce)
    else:
        assert _same(got, want32), (what, got, ce)


def _content(kind: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(1000 + n)
    if kind == "normal":
        return np.abs(rng.standard_normal(n)).astype(np.float32)
    if kind == "equal":
        return np.full(n, 0.7231, dtype=np.float32)
    if kind == "zeros":
        return np.zeros(n, dtype=np.float32)
    if kind == "low8":                                                             # values that differ in the lowest 8 bits only
        return (np.uint32(0x3fc00000) + rng.integers(0, 256, n).astype(np.uint32)).view(np.float32)
    if kind == "exponent":                                                         # values that differ in the exponent only
        return (rng.integers(1, 255, n).astype(np.uint32) << np.uint32(23)).view(np.float32)
    if kind == "denormal":
        return rng.integers(0, 1 << 23, n).astype(np.uint32).view(np.float32)
    v = np.abs(rng.standard_normal(n)).astype(np.float32)
    if kind == "inf_nan":                                                          # +inf and a NaN (sign bit clear) present
        v[rng.integers(0, n)] = np.inf
        v[rng.integers(0, n)] = np.array([0x7fc00001], dtype=np.uint32).view(np.float32)[0]
        if n > 2:
            v[rng.integers(0, n)] = np.inf
    elif kind == "ignored_20":
        v[rng.random(n) < 0.2] = -1.0
    else:
        assert kind == "all_ignored"
        v[:] = -1.0
    return v


CONTENTS = ["normal", "equal", "zeros", "low8", "exponent", "denormal", "inf_nan", "ignored_20", "all_ignored"]
SIZES = [1, 63, 64, 65, 257, 1000, 3 * 300 * 300]


@pytest.mark.parametrize("kind", CONTENTS)
def test_select_matches_numpy_on_the_bit_patterns(kind):
    """Every size (one, around a wave, more than a workgroup, 270 000: more than 1024 workgroups of 256, so the grid strides) and every
    fraction: tiny (k = 1), 0.1, 0.5, 1.0 (k = n).  Scratch pre-filled with 0xFF, guards around all three buffers, the map at a base
    misaligned by 4 bytes; a second run of the last fraction is the same bit for bit."""
    for n in SIZES:
        values = _content(kind, n)
        sel = Sel(values)
        for frac in (1e-9, 0.1, 0.5, 1.0):
            state, s0 = sel.run(frac)
            check_select(values, frac, state, s0, f"{kind} n {n} frac {frac}")
            if kind == "all_ignored":
                assert not np.isnan(state).any() and float(s0[0]) == 0.0 and not state[1:].any()
        again, s1 = sel.run(1.0)
        assert state.tobytes() == again.tobytes() and s0.tobytes() == s1.tobytes(), (kind, n)


def test_select_follows_the_fraction_in_device_memory_and_scales_by_inv_world():
    values = _content("normal", 1000)
    sel = Sel(values)
    a, sa = sel.run(0.1)
    b, sb = sel.run(0.5)                                                           # no argument of the call changed: only the device word
    assert (a[2], b[2]) == (100.0, 500.0) and a[5] > b[5] and float(sa[0]) > float(sb[0])
    c, sc = sel.run(0.5, inv_world=0.5)
    assert c.tobytes() == b.tobytes()                                              # the state is the rank's own
    check_select(values, 0.5, c, sc, "inv_world 0.5", inv_world=0.5)
    for bad, k in ((0.0, 1.0), (-3.0, 1.0), (float("nan"), 1.0), (7.0, 1000.0), (float("inf"), 1000.0)):      # never out of range
        sel.work.fill_(0xFF)
        sel.state[0:1].fill_(bad)
        _lib().tc_topk_select(sel.values.data_ptr(), sel.n, sel.state.data_ptr(), sel.sums.data_ptr(), 1.0, sel.work.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert float(sel.state[2]) == k and float(sel.state[1]) == 1000.0, (bad, sel.state.tolist())


# ---------------------------------------------------------------------------------------------------------------- inputs shared by 2 and 3
_CASES = {}


def _case(shape, seed=None):
    """Per shape, built once and left unchanged: logits [B, C, HW] (scaled normals), labels without and with 20 % ignored pixels, CE and
    overlap weights in [0.25, 4]."""
    key = (shape, seed)
    if key not in _CASES:
        B, C, H, W = shape
        g = torch.Generator().manual_seed(SEED[shape] if seed is None else seed)
        vals = torch.randn(B, C, H * W, generator=g) * 2.0
        full = torch.randint(0, C, (B, H * W), generator=g)
        part = full.clone()
        part.view(-1)[torch.randperm(part.numel(), generator=g)[:part.numel() // 5]] = II
        w_ce = 0.25 + 3.75 * torch.rand(C, generator=g, dtype=torch.float64)
        w_dice = 0.25 + 3.75 * torch.rand(C, generator=g, dtype=torch.float64)
        _CASES[key] = (vals, full, part, w_ce, w_dice)
    return _CASES[key]


def _combo(shape, weighted, ignoring, seed=None):
    vals, full, part, w_ce, w_dice = _case(shape, seed)
    return vals, (part if ignoring else full), (w_ce if weighted else None), (w_dice if weighted else None), (II if ignoring else None)


def _wdev(w_ce, w_dice, ncls):
    if w_ce is None:
        return None
    return torch.cat([w_ce, w_dice]).float().to(DEV)


def _overlap_of(gamma):
    """The loss cases pair gamma = 2 with Tversky(0.3, 0.7) and gamma = 0 with Dice."""
    return ("tversky", 0.3, 0.7) if gamma else ("dice", 0.5, 0.5)


def fwd_nchw(vals, lab, wdev, ii, gamma, code, topk=True):
    """fp32 NCHW forward: (prob, sums, values or None)."""
    L, st = _lib(), _stream()
    B, C, HW = vals.shape
    prob = torch.empty(B, C, HW, device=DEV)
    sums = torch.zeros(1 + 3 * C, device=DEV)
    if not topk:
        L.tc_seg_loss_fwd_ft(vals.data_ptr(), 0, lab.data_ptr(), _ptr(wdev), ii, gamma, code, prob.data_ptr(), sums.data_ptr(), B, C, HW, 0, st)
        return prob, sums, None
    values = torch.full((B * HW,), 9.0, device=DEV)
    L.tc_seg_loss_fwd_topk(vals.data_ptr(), 0, lab.data_ptr(), _ptr(wdev), ii, gamma, code, prob.data_ptr(), sums.data_ptr(), values.data_ptr(),
                           B, C, HW, 0, st)
    return prob, sums, values


def check_values(values, want, lab_c, ii, what):
    got = values.double().cpu().view(want.shape)
    tol = 1e-6 * torch.clamp(want, min=1.0)
    err = (got - want).abs()
    print(f"{what}: max |v - fp64| / tol = {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all()), (what, float((err / tol).max()))
    if ii is not None:
        assert bool((got[lab_c == ii] == -1.0).all()) and bool((got[lab_c != ii] >= 0.0).all()), what
    else:
        assert bool((got >= 0.0).all()), what


# ---------------------------------------------------------------------------------------------------------------- 2. forward values
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_values_sums_and_probabilities(shape):
    """fp32 NCHW with the probability map, bf16 and fp16 token-major rows of pitch 9, 16 and 24 without it;
    with and without class weights, ignore_index and gamma = 2.  The value map against float64 on the stored-precision logits, -1 exactly
    at ignored pixels; sums[0] left alone; sums[1..] as tc_seg_loss_fwd_ft leaves them (1e-5 relative: atomically folded); the
    probability map bit-equal to the _ft forward's."""
    L, st = _lib(), _stream()
    B, C, H, W = shape
    HW = H * W
    for weighted, ignoring, gamma in COMBOS:
        vals, lab_c, w_ce, w_dice, ii = _combo(shape, weighted, ignoring)
        lab, wdev, iik = lab_c.to(DEV), _wdev(w_ce, w_dice, C), OFF if ii is None else ii
        code = TVERSKY if gamma else DICE
        what = f"{shape} weights {weighted} ignore {ignoring} gamma {gamma}"
        want = pixel_values(vals, lab_c, w_ce, ii, gamma)
        vdev = vals.to(DEV)
        pa, sa, _ = fwd_nchw(vdev, lab, wdev, iik, gamma, code, topk=False)
        pb, sb, values = fwd_nchw(vdev, lab, wdev, iik, gamma, code)
        torch.cuda.synchronize()
        check_values(values, want, lab_c, ii, what + " fp32 NCHW")
        assert torch.equal(pa, pb) and float(sb[0]) == 0.0, what
        assert float(((sa[1:] - sb[1:]).abs() / (sa[1:].abs() + 1e-6)).max()) < 1e-5, what
        for dtype in (torch.bfloat16, torch.float16):
            stored = vals.to(dtype)
            want16 = pixel_values(stored, lab_c, w_ce, ii, gamma)
            for ld in (9, 16, 24):
                tok = torch.zeros(B * HW, ld, dtype=dtype, device=DEV)
                tok[:, :C] = stored.permute(0, 2, 1).reshape(B * HW, C).to(DEV)
                s_ft, s_tk = torch.zeros(1 + 3 * C, device=DEV), torch.zeros(1 + 3 * C, device=DEV)
                v16 = torch.full((B * HW,), 9.0, device=DEV)
                L.tc_seg_loss_fwd_ft(tok.data_ptr(), ld, lab.data_ptr(), _ptr(wdev), iik, gamma, code, None, s_ft.data_ptr(), B, C, HW, CODE[dtype], st)
                L.tc_seg_loss_fwd_topk(tok.data_ptr(), ld, lab.data_ptr(), _ptr(wdev), iik, gamma, code, None, s_tk.data_ptr(), v16.data_ptr(),
                                       B, C, HW, CODE[dtype], st)
                torch.cuda.synchronize()
                check_values(v16, want16, lab_c, ii, f"{what} {dtype} ld {ld}")
                assert float(s_tk[0]) == 0.0 and float(((s_ft[1:] - s_tk[1:]).abs() / (s_ft[1:].abs() + 1e-6)).max()) < 1e-5, (what, dtype, ld)


# ---------------------------------------------------------------------------------------------------------------- 3. loss and gradient
def check_scalars(got, want, what):
    refs = (want.loss, want.ce, want.overlap)
    errs = [abs(float(a) - b) / max(1.0, abs(b)) for a, b in zip(got, refs)]
    print(f"{what}: |loss, ce, overlap - fp64| / max(1, |ref|) = {errs[0]:.3e} {errs[1]:.3e} {errs[2]:.3e}")
    assert max(errs) < 2e-6, (what, [float(a) for a in got], refs)


def check_grad(got, want, what, rank=0):
    got = got.detach().double().cpu()
    ref, rce, rov = want.grad[rank], want.grad_ce[rank], want.grad_overlap[rank]
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    tol = 1e-8 + 1e-4 * (rce.abs() + rov.abs())
    worst = (err / tol).max().item()
    print(f"{what}: max |dlogits - fp64| = {err.max().item():.3e} (ref max {ref.abs().max().item():.3e}), worst err / tol = {worst:.3f}")
    assert bool((err <= tol).all()), f"{what}: max err {err.max().item():.3e}, worst err / tol {worst:.3f}"


class Run:
    """The four entries on fp32 NCHW values [B, C, HW]: the forward once, then select + value + backward per fraction."""

    def __init__(self, vals, lab, wdev, ii, gamma, overlap, alpha, beta, w=(0.4, 0.6)):
        self.vals, self.lab, self.wdev, self.ii, self.gamma, self.w = vals, lab, wdev, ii, gamma, w
        self.code, self.alpha, self.beta = (TVERSKY if overlap == "tversky" else DICE), alpha, beta
        self.prob, self.sums, self.values = fwd_nchw(vals, lab, wdev, ii, gamma, self.code)
        self.state = torch.zeros(8, dtype=torch.float64, device=DEV)
        self.work = torch.full((_lib().tc_topk_work_bytes() // 8,), -1, dtype=torch.int64, device=DEV)

    def select(self, frac, inv_world=1.0):
        self.state[0:1].fill_(frac)
        _lib().tc_topk_select(self.values.data_ptr(), self.values.numel(), self.state.data_ptr(), self.sums.data_ptr(), inv_world,
                              self.work.data_ptr(), _stream())

    def value(self, sums=None):
        out3 = torch.empty(3, device=DEV)
        C = self.vals.shape[1]
        _lib().tc_seg_loss_value_topk((self.sums if sums is None else sums).data_ptr(), _ptr(self.wdev), C, self.w[0], self.w[1], self.code,
                                      self.alpha, self.beta, out3.data_ptr(), _stream())
        return out3

    def bwd(self, sums=None, inv_world=1.0, gscale=1.0):
        B, C, HW = self.vals.shape
        d = torch.full((B, C, HW), 7.0, device=DEV)                                # a sentinel: every element must be written
        _lib().tc_seg_loss_bwd_topk(self.prob.data_ptr(), None, 0, self.lab.data_ptr(), _ptr(self.wdev), self.ii,
                                    (self.sums if sums is None else sums).data_ptr(), d.data_ptr(), 0, B, C, HW, self.w[0], self.w[1], self.gamma,
                                    self.code, self.alpha, self.beta, gscale, None, self.values.data_ptr(), self.state.data_ptr(), inv_world, 0, _stream())
        return d


@pytest.mark.parametrize("shape", SHAPES)
def test_loss_and_gradient_match_fp64(shape):
    """fp32 NCHW, every combination of class weights, ignore_index and (gamma = 2, Tversky) / (gamma = 0, Dice), every fraction."""
    B, C, H, W = shape
    for weighted, ignoring, gamma in COMBOS:
        vals, lab_c, w_ce, w_dice, ii = _combo(shape, weighted, ignoring)
        overlap, alpha, beta = _overlap_of(gamma)
        run = Run(vals.to(DEV), lab_c.to(DEV), _wdev(w_ce, w_dice, C), OFF if ii is None else ii, gamma, overlap, alpha, beta)
        plain = None
        for frac in FRACS:
            what = f"{shape} weights {weighted} ignore {ignoring} gamma {gamma} frac {frac}"
            want = reference(vals, lab_c, frac, w_ce, w_dice, ii, gamma, overlap, alpha, beta)
            print(f"{what}: k {want.sel[0].k} of {want.sel[0].n}, relative gap below the threshold {want.sel[0].gap:.3e}")
            assert want.sel[0].gap >= 1e-4, (what, want.sel[0].gap)                # the precondition, on the test's own inputs
            run.select(frac)
            out3, d = run.value(), run.bwd()
            torch.cuda.synchronize()
            st = run.state.cpu().tolist()
            assert (st[1], st[2], st[3], st[4]) == (want.sel[0].n, want.sel[0].k, want.sel[0].n_gt, want.sel[0].n_eq), (what, st)
            check_scalars(out3.cpu(), want, what)
            check_grad(d, want, what)
            assert not bool((d == 7.0).any())
            if ignoring:
                assert bool((d.cpu().permute(0, 2, 1)[lab_c == II] == 0).all())
            if not weighted:
                if plain is None:                                                  # the CE of the _ft entries on the same input
                    L, s = _lib(), _stream()
                    _, sums_ft, _ = fwd_nchw(run.vals, run.lab, None, run.ii, gamma, run.code, topk=False)
                    o = torch.empty(3, device=DEV)
                    L.tc_seg_loss_value_ft(sums_ft.data_ptr(), None, C, 0.4, 0.6, run.code, alpha, beta, o.data_ptr(), s)
                    plain = float(o[1])
                if frac == 0.1:
                    assert float(out3[1]) - plain > 1e-3, (what, float(out3[1]), plain)
                if frac == 1.0:
                    assert abs(float(out3[1]) - plain) < 2e-6, (what, float(out3[1]), plain)


@pytest.mark.parametrize("dtype,ld", [(torch.bfloat16, 16), (torch.bfloat16, 9), (torch.float16, 24), (torch.float16, 9), (torch.float32, 9)])
def test_token_major_backward_is_the_nchw_run_rounded_to_the_storage_type(dtype, ld):
    """2 x 9 x 11 x 11, class weights, ignore_index, gamma = 2, Tversky, frac = 0.25.  Token-major rows [B HW, ld] without a probability
    map: the value map is bit-equal to that of the fp32 NCHW run on the SAME stored values (same operations in the same order), and so,
    from the same sums and state, dlogits in the storage type equals the NCHW run's (held against float64) rounded to the storage type bit
    for bit.  Pad columns are zeros on the 16-byte path and untouched on the element path."""
    L, st = _lib(), _stream()
    shape = SHAPES[1]
    B, C, H, W = shape
    HW = H * W
    vals, lab_c, w_ce, w_dice, ii = _combo(shape, True, True)
    stored = vals.to(dtype)
    lab, wdev = lab_c.to(DEV), _wdev(w_ce, w_dice, C)
    want = reference(stored, lab_c, 0.25, w_ce, w_dice, ii, 2.0, "tversky", 0.3, 0.7)
    assert want.sel[0].gap >= 1e-4
    run = Run(stored.float().to(DEV), lab, wdev, II, 2.0, "tversky", 0.3, 0.7)
    run.select(0.25)
    out3, da = run.value(), run.bwd(gscale=128.0)
    check_scalars(out3.cpu(), want, f"{dtype} ld {ld}")
    check_grad(da / 128.0, want, f"{dtype} ld {ld}")                                # (a power of two: the scale is exact)
    tok = torch.zeros(B * HW, ld, dtype=dtype, device=DEV)
    tok[:, :C] = stored.permute(0, 2, 1).reshape(B * HW, C).to(DEV)
    sums = torch.zeros(1 + 3 * C, device=DEV)
    v = torch.full((B * HW,), 9.0, device=DEV)
    L.tc_seg_loss_fwd_topk(tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, 2.0, TVERSKY, None, sums.data_ptr(), v.data_ptr(), B, C, HW, CODE[dtype], st)
    d = torch.full((B * HW, ld), 3.0, dtype=dtype, device=DEV)
    L.tc_seg_loss_bwd_topk(None, tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, run.sums.data_ptr(), d.data_ptr(), ld, B, C, HW, 0.4, 0.6,
                           2.0, TVERSKY, 0.3, 0.7, 128.0, None, v.data_ptr(), run.state.data_ptr(), 1.0, CODE[dtype], st)
    torch.cuda.synchronize()
    assert torch.equal(v, run.values)
    want_tok = da.permute(0, 2, 1).reshape(B * HW, C).to(dtype)
    assert torch.equal(d[:, :C], want_tok), float((d[:, :C].float() - want_tok.float()).abs().max())
    vec = dtype != torch.float32 and ld % 8 == 0
    pad8 = (C + 7) // 8 * 8 if vec else C
    assert bool((d[:, C:pad8] == 0.0).all()) and bool((d[:, pad8:] == 3.0).all())
    assert bool((d[(lab == II).view(-1)][:, :C] == 0).all())
    d2 = torch.full((B * HW, ld), 3.0, dtype=dtype, device=DEV)
    L.tc_seg_loss_bwd_topk(None, tok.data_ptr(), ld, lab.data_ptr(), wdev.data_ptr(), II, run.sums.data_ptr(), d2.data_ptr(), ld, B, C, HW, 0.4, 0.6,
                           2.0, TVERSKY, 0.3, 0.7, 128.0, None, v.data_ptr(), run.state.data_ptr(), 1.0, CODE[dtype], st)
    torch.cuda.synchronize()
    assert torch.equal(d.view(torch.int16 if dtype != torch.float32 else torch.int32), d2.view(torch.int16 if dtype != torch.float32 else torch.int32))


# ---------------------------------------------------------------------------------------------------------------- 4. ties
def test_ties_share_the_places_left_at_the_threshold():
    """320 pixels of nine classes built from the row (a, 0, ..., 0) with label 0, whose value log(1 + 8 e^-a) falls with a: seven distinct
    rows above, eight IDENTICAL rows (bit-identical values) spread over both workgroups, 305 distinct rows below.  frac = 1/32 gives k = 10:
    n_gt = 7, n_eq = 8, three places left, f = 3/8.  With frac = 3/64, k = 15 takes all eight (f = 1): a tied pixel's CE gradient under
    k = 10 is (3/8) (15/10) of that, within a few fp32 roundings, and the eight are bit-equal."""
    n, C = 320, 9
    a = torch.empty(n, dtype=torch.float64)
    tied = torch.tensor([3, 60, 64, 127, 200, 255, 256, 319])
    rest = torch.tensor([i for i in range(n) if i not in set(tied.tolist())])
    g = torch.Generator().manual_seed(5)
    rest = rest[torch.randperm(rest.numel(), generator=g)]
    a[tied] = 0.0
    a[rest[:7]] = -3.0 + 0.25 * torch.arange(7, dtype=torch.float64)
    a[rest[7:]] = 0.5 + 0.01 * torch.arange(305, dtype=torch.float64)
    vals = torch.zeros(1, C, n)
    vals[0, 0] = a.float()
    lab_c = torch.zeros(1, n, dtype=torch.int64)
    want = reference(vals, lab_c, 1.0 / 32.0)
    assert (want.sel[0].k, want.sel[0].n_gt, want.sel[0].n_eq, want.sel[0].f) == (10, 7, 8, 0.375)
    run = Run(vals.to(DEV), lab_c.to(DEV), None, OFF, 0.0, "dice", 0.5, 0.5)
    run.select(1.0 / 32.0)
    out3, d = run.value(), run.bwd()
    torch.cuda.synchronize()
    st = run.state.cpu().tolist()
    assert st[1:5] == [320.0, 10.0, 7.0, 8.0] and st[7] == 0.375, st
    assert len(set(run.values.cpu()[tied].view(torch.int32).tolist())) == 1 and float(run.values[3]) == st[5]
    check_scalars(out3.cpu(), want, "ties")
    check_grad(d, want, "ties")
    ce10 = Run(vals.to(DEV), lab_c.to(DEV), None, OFF, 0.0, "dice", 0.5, 0.5, w=(0.4, 0.0))          # the CE term alone
    ce10.select(1.0 / 32.0)
    d10 = ce10.bwd().clone()
    ce10.select(3.0 / 64.0)
    d15 = ce10.bwd()
    torch.cuda.synchronize()
    assert ce10.state.cpu().tolist()[2:5] == [15.0, 7.0, 8.0] and float(ce10.state[7]) == 1.0
    t10, t15 = d10[0][:, tied].cpu().double(), d15[0][:, tied].cpu().double()
    assert float(t15.abs().min()) > 0.0
    assert float(((t10 - t15 * 0.375 * 1.5).abs() / t15.abs()).max()) < 4 * 2.0 ** -23
    assert all(torch.equal(d10[0][:, tied[0]].view(torch.int32), d10[0][:, i].view(torch.int32)) for i in tied.tolist())
    assert bool((d10[0][:, rest[7:]] == 0).all()) and bool((d10[0][:, rest[:7]] != 0).all())       # below: no CE gradient; above: all of it


# ---------------------------------------------------------------------------------------------------------------- 5. degenerate batches
def test_every_pixel_ignored_and_a_single_counted_pixel():
    shape = SHAPES[1]
    B, C, H, W = shape
    vals, full, part, w_ce, w_dice = _case(shape)
    lab_c = torch.full_like(full, II)
    run = Run(vals.to(DEV), lab_c.to(DEV), _wdev(w_ce, w_dice, C), II, 2.0, "tversky", 0.3, 0.7)
    run.select(0.25)
    out3, d = run.value(), run.bwd()
    torch.cuda.synchronize()
    assert bool((run.values == -1.0).all()) and run.state.cpu().tolist() == [0.25] + [0.0] * 7
    assert float(out3[1]) == 0.0 and bool(torch.isfinite(out3).all()) and bool((d == 0.0).all())
    lab_c[1, 57] = 4
    want = reference(vals, lab_c, 0.25, w_ce, w_dice, II, 2.0, "tversky", 0.3, 0.7)
    run = Run(vals.to(DEV), lab_c.to(DEV), _wdev(w_ce, w_dice, C), II, 2.0, "tversky", 0.3, 0.7)
    run.select(0.25)
    out3, d = run.value(), run.bwd()
    torch.cuda.synchronize()
    st = run.state.cpu().tolist()
    assert st[1:5] == [1.0, 1.0, 0.0, 1.0] and st[7] == 1.0 and st[6] == 0.0 and st[5] == float(run.values[H * W + 57])
    check_scalars(out3.cpu(), want, "one counted pixel")
    check_grad(d, want, "one counted pixel")
    assert bool((d.cpu().permute(0, 2, 1)[lab_c == II] == 0).all()) and float(d[1, :, 57].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- 6. two ranks
def test_two_ranks_emulated_on_one_gpu():
    """Two half-batches through the entries with inv_world = 0.5, their sums added as the all-reduce would: the CE is the mean of the two
    ranks' top-k means, each rank ranking its own pixels (the second half carries the ignored pixels, so k differs), the overlap term and
    its gradient are those of the whole batch."""
    shape = (4, 9, 11, 11)
    B, C, H, W = shape
    g = torch.Generator().manual_seed(2)
    vals = torch.randn(B, C, H * W, generator=g) * 2.0
    lab_c = torch.randint(0, C, (B, H * W), generator=g)
    lab_c[2:].view(-1)[torch.randperm(2 * H * W, generator=g)[:90]] = II
    w_ce = 0.25 + 3.75 * torch.rand(C, generator=g, dtype=torch.float64)
    w_dice = 0.25 + 3.75 * torch.rand(C, generator=g, dtype=torch.float64)
    want = reference_ranks([vals[:2], vals[2:]], [lab_c[:2], lab_c[2:]], 0.25, w_ce, w_dice, II, 2.0, "tversky", 0.3, 0.7)
    assert want.sel[0].k != want.sel[1].k and min(s.gap for s in want.sel) >= 1e-4
    wdev = _wdev(w_ce, w_dice, C)
    runs = [Run(vals[r:r + 2].contiguous().to(DEV), lab_c[r:r + 2].contiguous().to(DEV), wdev, II, 2.0, "tversky", 0.3, 0.7) for r in (0, 2)]
    for run in runs:
        run.select(0.25, inv_world=0.5)
    total = runs[0].sums + runs[1].sums
    out3 = runs[0].value(total)
    ds = [run.bwd(total, inv_world=0.5) for run in runs]
    torch.cuda.synchronize()
    assert [float(run.state[2]) for run in runs] == [float(s.k) for s in want.sel]
    check_scalars(out3.cpu(), want, "two ranks")
    for r in range(2):
        check_grad(ds[r], want, f"two ranks, rank {r}", rank=r)


# ---------------------------------------------------------------------------------------------------------------- 7. the Python entries
def _count(monkeypatch):
    L, n = _lib(), {name: 0 for name in TOPK_ENTRIES}
    for name in TOPK_ENTRIES:
        def counted(*a, _real=getattr(L, name), _name=name):
            n[_name] += 1
            return _real(*a)
        monkeypatch.setattr(L, name, counted)
    return n


def _eval(lf, logits, lab):
    x = logits.to(DEV).requires_grad_()
    out = lf(x, lab.to(DEV))
    out[0].backward()
    return [float(t.detach()) for t in out], x.grad


def test_seg_loss_eager_set_topk_and_stats(monkeypatch):
    from transception_amd.train import SegLoss
    shape = SHAPES[0]
    B, C, H, W = shape
    vals, lab_c, w_ce, w_dice, ii = _combo(shape, True, True)
    logits, lab = vals.view(B, C, H, W), lab_c.view(B, H, W)
    calls = _count(monkeypatch)
    _eval(SegLoss(C, ce_weight=w_ce, dice_weight=w_dice, ignore_index=II), logits, lab)
    assert calls == {name: 0 for name in TOPK_ENTRIES}                             # ce_topk=None: none of the new entries
    lf = SegLoss(C, ce_weight=w_ce, dice_weight=w_dice, ignore_index=II, focal_gamma=2.0, overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7,
                 ce_topk=0.25)
    state = lf.topk_state(DEV)
    got, d = _eval(lf, logits, lab)
    assert calls == {name: 1 for name in TOPK_ENTRIES}
    want = reference(vals, lab_c, 0.25, w_ce, w_dice, II, 2.0, "tversky", 0.3, 0.7)
    assert want.sel[0].gap >= 1e-4
    check_scalars(got, want, "SegLoss(ce_topk=0.25)")
    check_grad(d.view(B, C, H * W), want, "SegLoss(ce_topk=0.25)")
    stats = lf.topk_stats(DEV)
    s = want.sel[0]
    assert (stats["n"], stats["k"], stats["n_gt"], stats["n_eq"], stats["tie_share"]) == (s.n, s.k, s.n_gt, s.n_eq, s.f)
    assert abs(stats["threshold"] - s.t) <= 1e-6 * max(1.0, s.t) and set(stats) == {"n", "k", "n_gt", "n_eq", "threshold", "tie_share"}
    lf.set_topk(0.5)
    assert lf.topk_state(DEV) is state and float(state[0]) == 0.5
    got, d = _eval(lf, logits, lab)
    want = reference(vals, lab_c, 0.5, w_ce, w_dice, II, 2.0, "tversky", 0.3, 0.7)
    assert want.sel[0].gap >= 1e-4 and lf.topk_stats(DEV)["k"] == want.sel[0].k == topk_k(0.5, s.n)
    check_scalars(got, want, "set_topk(0.5)")
    check_grad(d.view(B, C, H * W), want, "set_topk(0.5)")
    # a static loss scale multiplies the gradient that leaves the loss, not the loss: a power of two, so exactly
    scaled = SegLoss(C, ce_weight=w_ce, dice_weight=w_dice, ignore_index=II, focal_gamma=2.0, overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7,
                     ce_topk=0.5, loss_scale=128.0)
    got128, d128 = _eval(scaled, logits[:, :, :8, :], lab[:, :8, :])               # 256 pixels: one workgroup, one addend per sum
    got1, d1 = _eval(lf, logits[:, :, :8, :], lab[:, :8, :])
    assert got128 == got1 and torch.equal(d128, d1 * 128.0) and float(d1.abs().max()) > 0.0


CW = (0.5, 1.0, 2.0, 0.0, 4.0, 0.25, 1.5, 3.0, 1.0)


def _step_inputs():
    from test_weighted_loss_gpu import BATCH, SIZE
    from transception_amd.seeded_init import seeded_input, seeded_labels
    x = torch.from_numpy(seeded_input(BATCH, size=SIZE)).to(DEV)
    lab = torch.from_numpy(seeded_labels(BATCH, size=SIZE))
    lab[:, :20, :] = II                                                            # an unlabelled margin: 31 % of the pixels
    return x, lab.to(DEV)


def test_captured_step_follows_the_eager_step_and_the_fraction(monkeypatch):
    """fp32 model, 64 x 64, B = 2, ce_topk = 0.25 with class weights and ignore_index: three replayed steps follow three eager train_steps
    from the same state within the 5e-4 of the other captured-step tests; set_topk(0.5) then changes the next replay's k, with no new
    capture (no entry is called again)."""
    from test_weighted_loss_gpu import _fresh
    from transception_amd.train import FusedSGD, GraphedStep, SegLoss, train_step
    x, lab = _step_inputs()
    n = int((lab != II).sum())
    me, mg, md = _fresh(), _fresh(), _fresh()
    oe, og, od = FusedSGD(me, lr=0.05), FusedSGD(mg, lr=0.05), FusedSGD(md, lr=0.05)
    le, lg = (SegLoss(9, ce_weight=CW, dice_weight=CW, ignore_index=II, ce_topk=0.25) for _ in range(2))
    default = [t.item() for t in train_step(md, SegLoss(9, ce_weight=CW, dice_weight=CW, ignore_index=II), od, x, lab)]
    first = [t.item() for t in train_step(me, le, oe, x, lab)]
    assert all(math.isfinite(v) for v in first) and abs(first[1] - default[1]) > 1e-3 and abs(first[2] - default[2]) < 2e-6, (first, default)
    train_step(me, le, oe, x, lab)                                                 # as many steps as the capture's warm-up takes
    calls = _count(monkeypatch)
    step = GraphedStep(mg, lg, og, x, lab, None, warmup=2)
    assert calls == {name: 3 for name in TOPK_ENTRIES}                             # two warm-up steps and the capture
    for i in range(3):
        a = [t.item() for t in train_step(me, le, oe, x, lab)]
        b = [t.item() for t in step()]
        print(f"step {i}: eager {a}, replayed {b}")
        assert all(math.isfinite(v) for v in b)
        assert abs(a[0] - b[0]) < 5e-4, (a, b)
    assert lg.topk_stats(DEV)["n"] == n and lg.topk_stats(DEV)["k"] == topk_k(0.25, n)
    before = dict(calls)
    lg.set_topk(0.5)
    c = [t.item() for t in step()]
    assert calls == before and lg.topk_stats(DEV)["k"] == topk_k(0.5, n)
    assert all(math.isfinite(v) for v in c) and c[1] < b[1] - 1e-3, (b, c)         # the mean of more, smaller terms
    assert bool(torch.isfinite(mg.flat_parameters()).all())


def test_bf16_step_with_dynamic_loss_scale_adamw_and_ema():
    """bf16 storage, DynamicLossScale, FusedAdamW with a WeightEMA, ce_topk = 0.1 with gamma = 2 and Tversky: one eager step and one
    replayed step -- nothing skipped, every scalar finite, the average moved."""
    from test_loss_scale_gpu import _fresh
    from transception_amd.train import DynamicLossScale, FusedAdamW, GraphedStep, SegLoss, WeightEMA, train_step
    x, lab = _step_inputs()
    m = _fresh(torch.bfloat16)
    scaler = DynamicLossScale(init_scale=1024.0)
    lf = SegLoss(9, loss_scale=scaler, ce_weight=CW, dice_weight=CW, ignore_index=II, focal_gamma=2.0, overlap="tversky", tversky_alpha=0.3,
                 tversky_beta=0.7, ce_topk=0.1)
    opt = FusedAdamW(m, lr=1e-3)
    ema = opt.ema = WeightEMA(m, decay=0.9)
    a = [t.item() for t in train_step(m, lf, opt, x, lab)]
    assert all(math.isfinite(v) for v in a) and not opt.last_step_skipped(), a
    step = GraphedStep(m, lf, opt, x, lab, None, warmup=0)
    b = [t.item() for t in step()]
    print(f"eager {a}, replayed {b}")
    assert all(math.isfinite(v) for v in b) and not opt.last_step_skipped() and scaler.skipped() == 0
    n = int((lab != II).sum())
    assert lf.topk_stats(DEV)["k"] == topk_k(0.1, n) and ema.updates() == 2 and bool(torch.isfinite(m.flat_parameters()).all())


def test_trainer_logs_the_top_k_cross_entropy(tmp_path, monkeypatch):
    """trainer_synapse for one tiny epoch with TrainConfig(ce_topk=0.1): the loss it builds carries the fraction, and loss_ce of the first
    log line is the top-k CE of the first batch, as a direct SegLoss evaluation on an identical model gives it."""
    from test_weighted_loss_gpu import _fresh
    from transception_amd import data as D
    from transception_amd import trainer as T
    from transception_amd.train import SegLoss
    base, lists = str(tmp_path / "train_npz"), str(tmp_path / "lists")
    D.write_synthetic_synapse(base, lists, n_cases=1, slices_per_case=4, size=64, seed=2)
    cfg = T.TrainConfig(root_path=base, list_dir=lists, max_epochs=1, batch_size=2, img_size=64, seed=5, model_name="tiny", class_weights=CW,
                        ignore_index=II, ce_topk=0.1)
    batches = []
    real = T.train_step

    def spy(model, loss_fn, opt, x, y, group=None):
        batches.append((x.clone(), y.clone()))
        assert loss_fn.ce_topk == 0.1
        return real(model, loss_fn, opt, x, y, group)

    monkeypatch.setattr(T, "train_step", spy)
    lines = []
    hist = T.trainer_synapse(cfg, _fresh(), str(tmp_path / "snap"), log=lines.append)
    assert hist["iterations"] == 2 and all(math.isfinite(v) for v in hist["loss"])
    first = next(l for l in lines if l.startswith("iteration 1 "))
    logged = [float(v) for v in re.search(r"loss : (\S+), loss_ce: (\S+), loss_dice: (\S+)", first).groups()]
    x, y = batches[0]
    with torch.no_grad():
        got = [float(t) for t in SegLoss(9, ce_weight=CW, dice_weight=CW, ignore_index=II, ce_topk=0.1)(_fresh()(x), y)]
        off = [float(t) for t in SegLoss(9, ce_weight=CW, dice_weight=CW, ignore_index=II)(_fresh()(x), y)]
    print(f"logged {logged}, direct {got}, without top-k {off}")
    assert all(abs(a - b) < 2e-6 * max(1.0, abs(b)) for a, b in zip(logged, got)), (logged, got)
    assert abs(got[1] - off[1]) > 1e-3 and abs(got[2] - off[2]) < 2e-6

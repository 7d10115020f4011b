"""The Scale_reduce tail in one launch each way (tc_sr_ln_fwd / tc_sr_ln_bwd, include/transception_bridge.h) against the launches it replaces,
run on the same inputs in the same test through the C ABI:

  forward   tc_ew_multi (de-interleaves + row-block copy into a [B * Nk, 64] matrix), then tc_layernorm_fwd
  backward  tc_layernorm_bwd_defer (+ tc_layernorm_fold), then tc_ew_multi with the inverse / accumulate flags

Every comparison of an activation or an activation gradient is of bit patterns: the new kernels run the per-row arithmetic of the old ones on
the same values, only the addresses differ.  Output and gradient buffers are larger than needed and pre-filled with a sentinel, and the whole
buffer is compared.  The gradient that is already in the row-block source (the accumulate flag) holds multiples of 1/8.

dgamma / dbeta: the new backward keeps tc_layernorm_bwd_defer's rows in the same workgroups, so the parked per-workgroup partials are compared
bit for bit -- that is the deterministic statement.  tc_layernorm_fold adds ceil(nblk / 128) partial sums per column with atomics: up to two
addends the folded dgamma / dbeta are order-independent and compared bit for bit too; with more (the 5292-row case: three) two runs of the
SAME path may differ in the last place, so there both paths are held against a float64 reference from the same 16-bit inputs: the new path's
error may not exceed the old path's by more than one fp32 unit in the last place of the largest entry (both errors are printed)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from transception_amd._lib import (ACT_NONE, EW_COPY, EW_DEINTERLEAVE, TC_BF16, TC_F16, TC_F32, TcError, TcEwSeg, TcLnFold, TcSrSrc, lib)  # noqa: E402
from transception_amd.seeded_init import seeded_tensor  # noqa: E402

DEV = "cuda:0"
TC = {torch.bfloat16: TC_BF16, torch.float16: TC_F16}
SENT = -96.0
CD = 64
LDY, LDS = 72, 80                  # row strides of y / dy and of the row-block source: not the row width

#        B  P    mults      row-block rows  order of the sources inside an image (d = de-interleaved in turn, c = the row block)
CASES = [(1, 1,   (1, 2, 5), 1,  "dddc"),          # Nk = 9: less than one workgroup's rows
         (3, 1,   (1, 2, 5), 3,  "dddc"),          # Nk = 11, 33 rows: three workgroups of 16, the last one short
         (1, 4,   (1, 2, 5), 4,  "dddc"),
         (3, 4,   (1, 2, 5), 3,  "cddd"),          # the row block first
         (3, 49,  (1, 2, 5), 3,  "dddc"),          # Nk = 395, 1185 rows
         (1, 49,  (1, 2, 5), 49, "ddcd"),          # the row block in the middle
         (3, 4,   (1,),      3,  "dc"),
         (1, 49,  (2,),      49, "dc"),
         (3, 4,   (2,),      4,  "dc"),
         (3, 49,  (5,),      3,  "dc"),
         (1, 1,   (5,),      3,  "cd"),
         (3, 196, (1, 2, 5), 196, "dddc")]         # 5292 rows: the forward's four-rows-per-lane-group launch (>= 4096 rows), three fold addends


def _name(dtype):
    return str(dtype).split(".")[-1]


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def vals(tag, shape, dtype, scale=3.0):
    return torch.from_numpy(seeded_tensor("sr_ln/" + tag, shape, scale)).to(dtype).to(DEV)


def grid(tag, shape, dtype):
    t = torch.from_numpy(seeded_tensor("sr_ln/grid/" + tag, shape, 2.0))
    return ((t * 8).round().clamp(-32, 32) / 8 + 0.0).to(dtype).to(DEV)


def sent(shape, dtype):
    return torch.full(shape, SENT, dtype=dtype, device=DEV)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))


def ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


class Setup:
    """Inputs of one case and the source lists of both paths."""

    def __init__(self, case, dtype):
        B, P, mults, crow, order = case
        self.B, self.P, self.dtype, self.dt = B, P, dtype, TC[dtype]
        tag = f"{case}{_name(dtype)}"
        self.items, off, mi = [], 0, iter(mults)            # ("d", tensor, mult, off) | ("c", tensor, rows, off)
        for k, kind in enumerate(order):
            if kind == "d":
                m = next(mi)
                self.items.append(("d", vals(f"{tag}x{k}", (B * P, CD * m), dtype), m, off))
                off += m * P
            else:
                # row block: `crow` rows per image, one spare row between the images, three rows in front, row stride LDS
                self.c_sb, self.c_off = (crow + 1) * LDS, 3 * LDS
                self.items.append(("c", vals(f"{tag}c{k}", (3 + B * (crow + 1) + 2, LDS), dtype), crow, off))
                off += crow
        self.Nk, self.rows = off, B * off
        self.gamma, self.beta = vals(tag + "g", (CD,), dtype, 1.0) + 1.0, vals(tag + "b", (CD,), dtype, 0.5)
        self.dy = vals(tag + "dy", (self.rows + 2, LDY), dtype, 1.0)

    def ew_segs(self, red, grads=None):
        """The old path's layout moves into (grads None) or out of the [rows, 64] matrix `red`."""
        segs = []
        for i, (kind, t, n, off) in enumerate(self.items):
            if kind == "d":
                segs.append(TcEwSeg(EW_DEINTERLEAVE, 0 if grads is None else 1, ptr(t if grads is None else grads[i]), ptr(red, off * CD),
                                    0, self.Nk * CD, 0, CD, self.B, self.P, CD, n, 0, 0))
            elif grads is None:
                segs.append(TcEwSeg(EW_COPY, 0, ptr(t, self.c_off), ptr(red, off * CD), self.c_sb, self.Nk * CD, LDS, CD, self.B, n, CD, 0, 0, 0))
            else:
                segs.append(TcEwSeg(EW_COPY, 1, ptr(red, off * CD), ptr(grads[i], self.c_off), self.Nk * CD, self.c_sb, CD, LDS, self.B, n, CD,
                                    0, 0, 0))
        return (TcEwSeg * len(segs))(*segs), len(segs)

    def sources(self, grads=None):
        arr = (TcSrSrc * len(self.items))()
        for i, (kind, t, n, off) in enumerate(self.items):
            g = None if grads is None else grads[i]
            if kind == "d":
                arr[i] = TcSrSrc(ptr(t), ptr(g) if g is not None else None, 0, n, self.P, 0, 0, off, 0)
            else:
                arr[i] = TcSrSrc(ptr(t, self.c_off), ptr(g, self.c_off) if g is not None else None, self.c_sb, 0, 0, LDS, n, off, 1)
        return arr, len(self.items)

    def grad_buffers(self, tag):
        """Gradient buffers of the sources: sentinel-filled and two elements long for the de-interleaved ones (written once), multiples of
        1/8 everywhere for the row block (accumulated into)."""
        out = []
        for k, (kind, t, n, off) in enumerate(self.items):
            out.append(sent((t.numel() + 16,), self.dtype) if kind == "d" else grid(f"{tag}{k}", tuple(t.shape), self.dtype))
        return out


def run_old_fwd(S):
    L, s = lib(), stream()
    red = sent((S.rows, CD), S.dtype)
    y, mean, rstd = sent((S.rows + 3, LDY), S.dtype), sent((S.rows + 5,), torch.float32), sent((S.rows + 5,), torch.float32)
    segs, n = S.ew_segs(red)
    L.tc_ew_multi(segs, n, S.dt, s)
    L.tc_layernorm_fwd(ptr(red), CD, ptr(S.gamma), ptr(S.beta), ptr(y), LDY, ptr(mean), ptr(rstd), S.rows, CD, 1e-5, ACT_NONE, 1, 0, S.dt, s)
    return red, y, mean, rstd


def run_new_fwd(S):
    y, mean, rstd = sent((S.rows + 3, LDY), S.dtype), sent((S.rows + 5,), torch.float32), sent((S.rows + 5,), torch.float32)
    srcs, n = S.sources()
    lib().tc_sr_ln_fwd(srcs, n, S.B, S.Nk, ptr(S.gamma), ptr(S.beta), ptr(y), LDY, ptr(mean), ptr(rstd), 1e-5, S.dt, stream())
    return y, mean, rstd


def fold(part, nblk):
    dg, db = torch.zeros(CD, dtype=torch.float32, device=DEV), torch.zeros(CD, dtype=torch.float32, device=DEV)
    site = (TcLnFold * 1)(TcLnFold(ptr(part), ptr(dg), ptr(db), 0, nblk, CD, 1))
    lib().tc_layernorm_fold(site, 1, stream())
    return dg, db


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_name)
@pytest.mark.parametrize("case", CASES, ids=str)
def test_sr_ln_matches_the_launches_it_replaces(case, dtype):
    L, s = lib(), stream()
    S = Setup(case, dtype)
    assert L.tc_sr_ln_supported(S.rows, CD, S.dt) == 1
    red, y0, mean0, rstd0 = run_old_fwd(S)
    y1, mean1, rstd1 = run_new_fwd(S)
    torch.cuda.synchronize()
    assert same_bits(y1, y0) and same_bits(mean1, mean0) and same_bits(rstd1, rstd0)
    assert bool((y0[:S.rows, :CD] != SENT).any()) and bool((y0[S.rows:] == SENT).all()) and bool((y0[:, CD:] == SENT).all())

    # backward: both from the old forward's statistics (equal to the new one's, checked above)
    nblk = int(L.tc_layernorm_bwd_nblk(S.rows, CD))
    assert nblk > 0
    nf = nblk * 2 * CD
    part0, part1 = sent((nf + 8,), torch.float32), sent((nf + 8,), torch.float32)
    g0, g1 = S.grad_buffers(f"{case}g"), S.grad_buffers(f"{case}g")
    dred = sent((S.rows, CD), dtype)
    dg_unused, db_unused = torch.zeros(CD, dtype=torch.float32, device=DEV), torch.zeros(CD, dtype=torch.float32, device=DEV)
    L.tc_layernorm_bwd_defer(ptr(S.dy), LDY, ptr(red), CD, ptr(S.gamma), ptr(S.beta), ptr(mean0), ptr(rstd0), ptr(dred), CD, None, 0,
                             ptr(dg_unused), ptr(db_unused), S.rows, CD, ACT_NONE, 1, 0, ptr(part0), nf, S.dt, s)
    segs, n = S.ew_segs(dred, g0)
    L.tc_ew_multi(segs, n, S.dt, s)
    srcs, n = S.sources(g1)
    L.tc_sr_ln_bwd(srcs, n, S.B, S.Nk, ptr(S.dy), LDY, ptr(S.gamma), ptr(mean0), ptr(rstd0), ptr(part1), nf, S.dt, s)
    dg0, db0 = fold(part0, nblk)
    dg1, db1 = fold(part1, nblk)
    torch.cuda.synchronize()
    for a, b_, (kind, t, _, _) in zip(g1, g0, S.items):
        assert same_bits(a, b_), kind
        if kind == "d":
            assert bool((b_[:t.numel()] != SENT).all()) and bool((b_[t.numel():] == SENT).all())     # every element written once, nothing past the end
    assert same_bits(part1, part0) and bool((part0[nf:] == SENT).all())
    if (nblk + 127) // 128 <= 2:
        assert same_bits(dg1, dg0) and same_bits(db1, db0)
    else:
        xh = (red.double() - mean0[:S.rows].double()[:, None]) * rstd0[:S.rows].double()[:, None]
        d64 = S.dy[:S.rows, :CD].double()
        for name, new, old, ref in (("dgamma", dg1, dg0, (d64 * xh).sum(0)), ("dbeta", db1, db0, d64.sum(0))):
            e_new, e_old = float((new.double() - ref).abs().max()), float((old.double() - ref).abs().max())
            ulp = float(torch.finfo(torch.float32).eps) * float(2.0 ** torch.floor(torch.log2(ref.abs().max())))
            print(f"{name}: |new - fp64| = {e_new:.3e}, |old - fp64| = {e_old:.3e}, one fp32 ulp of the largest entry = {ulp:.3e}")
            assert e_new <= e_old + ulp


def test_unsupported_arguments_are_refused():
    L, s = lib(), stream()
    assert L.tc_sr_ln_supported(100, 32, TC_BF16) == 0 and L.tc_sr_ln_supported(100, 128, TC_F16) == 0        # C != 64
    assert L.tc_sr_ln_supported(100, CD, TC_F32) == 0                                                           # fp32 storage
    assert L.tc_sr_ln_supported(1 << 17, CD, TC_BF16) == 0 and L.tc_sr_ln_supported(0, CD, TC_BF16) == 0
    assert L.tc_sr_ln_supported(7056, CD, TC_BF16) == 1 and L.tc_sr_ln_supported(7056, CD, TC_F16) == 1
    S = Setup((1, 4, (1, 2, 5), 3, "dddc"), torch.bfloat16)
    y, mean, rstd = sent((S.rows, LDY), S.dtype), sent((S.rows,), torch.float32), sent((S.rows,), torch.float32)
    part = sent((int(L.tc_layernorm_bwd_nblk(S.rows, CD)) * 2 * CD,), torch.float32)
    grads = S.grad_buffers("refuse")

    def fwd(srcs, n, dt=S.dt, Nk=S.Nk, yp=ptr(y), ldy=LDY):
        L.tc_sr_ln_fwd(srcs, n, S.B, Nk, ptr(S.gamma), ptr(S.beta), yp, ldy, ptr(mean), ptr(rstd), 1e-5, dt, s)

    def bwd(srcs, n, dt=S.dt, nf=part.numel(), dyp=ptr(S.dy)):
        L.tc_sr_ln_bwd(srcs, n, S.B, S.Nk, dyp, LDY, ptr(S.gamma), ptr(mean), ptr(rstd), ptr(part), nf, dt, s)

    srcs, n = S.sources()
    gsrcs, _ = S.sources(grads)
    fwd(srcs, n)                                                   # the operands as they are: taken
    bwd(gsrcs, n)
    torch.cuda.synchronize()
    before = (y.clone(), [g.clone() for g in grads])
    refusals = [lambda: fwd(srcs, n, dt=TC_F32), lambda: bwd(gsrcs, n, dt=TC_F32),          # fp32
                lambda: fwd(srcs, n, yp=ptr(y) + 2), lambda: fwd(srcs, n, ldy=LDY + 4),      # output rows off the 16-byte grid
                lambda: bwd(gsrcs, n, dyp=ptr(S.dy) + 2),
                lambda: fwd(srcs, n, Nk=S.Nk + 1), lambda: fwd(srcs, n - 1),                 # the sources do not tile [0, Nk)
                lambda: bwd(srcs, n),                                                        # no gradient destinations
                lambda: bwd(gsrcs, n, nf=part.numel() - 1),                                  # partial buffer too small
                lambda: fwd(srcs, 0), lambda: fwd(None, n)]
    for k in range(n):                                             # one misaligned source pointer at a time; overlapping rows
        for field, delta in (("src", 2), ("off", 1)):
            bad, _ = S.sources()
            setattr(bad[k], field, getattr(bad[k], field) + delta)
            refusals.append(lambda bad=bad: fwd(bad, n))
    bad, _ = S.sources()
    bad[n - 1].ld = LDS + 4                                        # row-block stride off the 16-byte grid
    refusals.append(lambda: fwd(bad, n))
    for r in refusals:
        with pytest.raises(TcError, match="status -1"):
            r()
    torch.cuda.synchronize()
    assert same_bits(y, before[0]) and all(same_bits(a, b_) for a, b_ in zip(grads, before[1]))          # a refused call launches nothing


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_name)
def test_engine_sr_ln_against_sr_gather_and_layernorm(dtype):
    """Graph.sr_ln against Graph.sr_gather + Graph.layernorm on a stage-major token buffer as the model lays it out: outputs, the gradients
    of the three convolution outputs, the token buffer's region gradient and the LayerNorm's parameter gradients, bit for bit; one launch
    fewer each way."""
    from transception_amd import _lib
    from transception_amd.engine import Graph, P, Var
    B, Pn, ntok3, pre = 2, 4, 3, 5                                 # `pre` token rows of other stages in front of the stage-4 rows
    mults = (1, 2, 5)
    Nk = sum(mults) * Pn + ntok3
    roffs = [0, Pn, 3 * Pn, 8 * Pn]
    res = {}
    for fused in (False, True):
        G = Graph(dtype, torch.device(DEV), training=True, record=True)
        n = Var(vals("eng_n", (pre + B * ntok3, CD), dtype))
        xs = [Var(vals(f"eng_x{k}", (B * Pn, CD * m), dtype)) for k, m in enumerate(mults)]
        gp = P(vals("eng_g", (CD,), dtype, 1.0) + 1.0, torch.zeros(CD, dtype=torch.float32, device=DEV), 0)
        bp = P(vals("eng_b", (CD,), dtype, 0.5), torch.zeros(CD, dtype=torch.float32, device=DEV), 0)
        calls0 = _lib._Lib.calls
        if fused:
            parts, copy = [(xs[k], roffs[k], Pn, mults[k]) for k in range(3)], (n, pre * CD, ntok3 * CD, roffs[3], ntok3)
            assert G.sr_ln_supported(parts, copy, B, Nk, gp, bp)
            rn = G.sr_ln(parts, copy, B, Nk, gp, bp)
        else:
            red = G.new(B * Nk, CD)
            G.sr_gather([(xs[k], roffs[k] * CD, Nk * CD, B, Pn, CD, mults[k]) for k in range(3)],
                        (n, pre * CD, ntok3 * CD, roffs[3] * CD, Nk * CD, B, ntok3, CD), red)
            rn = G.layernorm(red, gp, bp)
        nfwd = _lib._Lib.calls - calls0
        rn.root.grad_t, rn.root.whole_written = vals("eng_dy", (B * Nk, CD), dtype, 1.0), True
        G._region_grad(n.root, 0, n.data.numel())                  # a gradient that is already there: multiples of 1/8
        n.root.grad_t.copy_(grid("eng_gn", tuple(n.data.shape), dtype))
        calls0 = _lib._Lib.calls
        G.backward()
        torch.cuda.synchronize()
        res[fused] = (rn.data.clone(), [G.grad_of(x).clone() for x in xs], n.root.grad_t.clone(), gp.grad.clone(), bp.grad.clone(),
                      nfwd, _lib._Lib.calls - calls0)
    old, new = res[False], res[True]
    assert same_bits(new[0], old[0]) and all(same_bits(a, b_) for a, b_ in zip(new[1], old[1])) and same_bits(new[2], old[2])
    assert same_bits(new[3], old[3]) and same_bits(new[4], old[4])
    assert (old[5], new[5]) == (2, 1) and old[6] - new[6] == 1     # forward: 2 -> 1; backward: the fold stays, one launch fewer

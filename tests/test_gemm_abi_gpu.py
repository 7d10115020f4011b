"""csrc/gemm.hip through the C ABI, one hand-filled TcGemm at a time, against the float64 reference of tests/gemm_ref.py.

Every comparison but the sigmoid's is exact.  Operands are small integers (gemm_ref's docstring; tests/test_gemm_ref_host.py holds every
case to it), so every product, every fp32 partial sum in any order, every split-K atomic and every workspace fold is exact, a 16-bit C is
the exact value rounded once, and the WHOLE output buffer -- oversize, pre-filled with the sentinel -96 where the op stores and with grid
values where it accumulates -- is compared by bit pattern with what the reference says it must hold (the sign of a zero apart, which the
header does not define: alpha = -2 times an exact 0 is -0 in one epilogue and +0 after `+ bias` in another).  Operand buffers are NaN
everywhere outside the logical matrices (ld padding, rows in front and behind, batch gaps, bgap gaps), so one element read from outside
turns a result into NaN; they are checked to come back unchanged.

The XCD tile grids need M up to 23 tiles of 64 rows; every other case keeps M, N <= 520 and K <= 8256.  DESIGN.md section 2 lists which
test reaches which branch of gemm_plan / tc_gemm_pair / tc_gemm_multi."""
import ctypes as C

import pytest
import torch

import gemm_ref as gr
from gemm_ref import CNT_BYTES, PART_BYTES, Problem

pytestmark = pytest.mark.gpu

from transception_amd._lib import (ACT_GELU, ACT_NONE, ACT_SCALE, ACT_SIGMOID, FFN_EP, FFN_LN_A, FFN_LN_B, TC_BF16, TC_F16, TC_F32, TcError,  # noqa: E402
                                   TcGemm, lib)

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = [torch.bfloat16, torch.float16]
TC = {torch.float32: TC_F32, torch.bfloat16: TC_BF16, torch.float16: TC_F16}


def _name(dtype):
    return str(dtype).split(".")[-1]


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def bits(t):
    t = (t.detach().cpu() + 0.0).contiguous()                                   # -0.0 -> +0.0, nothing else changes
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def raw(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def upload(p):
    return {k: v.to(DEV) for k, v in p.bufs.items()}


def ptr(d, p, name):
    return d[name].data_ptr() + p.off[name] * d[name].element_size() if name in d else None


def desc(p, d, ws=None, ws_bytes=0, **over):
    g = TcGemm()
    for k, v in p.fields.items():
        setattr(g, k, v)
    g.A, g.B, g.C, g.bias, g.R = ptr(d, p, "A"), ptr(d, p, "B"), ptr(d, p, "C"), ptr(d, p, "bias"), ptr(d, p, "R")
    g.rowsum, g.bn_part, g.bn_shift = ptr(d, p, "rowsum"), ptr(d, p, "bn_part"), ptr(d, p, "bn_shift")
    g.dtype = TC[p.dtype]
    g.ws, g.ws_bytes = ws, ws_bytes
    for k, v in over.items():
        setattr(g, k, v)
    return g


def check(p, d, what=""):
    """Every output buffer holds, element for element, what the reference says; every input buffer is as it was."""
    for name, want in p.expect.items():
        got = d[name].cpu()
        assert got.dtype == want.dtype and got.shape == want.shape
        bg, bw = bits(got), bits(want)
        if not torch.equal(bg, bw):
            bad = (bg != bw).nonzero().view(-1)
            i = int(bad[0])
            inside = bool((p.idx[name] == i).any()) if name in p.idx else None
            pytest.fail(f"{p.tag} {_name(p.dtype)} {what}{name}: {bad.numel()} of {got.numel()} elements differ, first at {i} "
                        f"({'inside' if inside else 'OUTSIDE'} the logical matrix): got {float(got[i])}, want {float(want[i])}")
    for name in ("A", "B", "R", "bias", "bn_shift"):
        if name in d:
            assert torch.equal(raw(d[name]), raw(p.bufs[name])), f"{p.tag}: {name} was written"


def run(kw, dtype, **ws):
    p = Problem(dtype=dtype, **kw)
    d = upload(p)
    g = desc(p, d, **ws)
    lib().tc_gemm(C.byref(g), stream())
    torch.cuda.synchronize()
    check(p, d)
    return p, d


class Workspace:
    """CNT_BYTES of arrival counters + `slots` partial-tile slots, zeroed, and a tail of 0xA5 bytes behind them that is not part of it."""
    TAIL = 4096

    def __init__(self, slots, shift=0):
        self.n, self.shift = CNT_BYTES + slots * PART_BYTES, shift
        self.buf = torch.zeros(shift + self.n + self.TAIL, dtype=torch.uint8, device=DEV)
        self.buf[shift + self.n:] = 0xA5
        self.args = dict(ws=self.buf.data_ptr() + shift, ws_bytes=self.n)

    def after(self, used):
        b = self.buf.cpu()
        assert bool((b[self.shift:self.shift + CNT_BYTES] == 0).all()), "arrival counters are not left zero"
        assert bool((b[self.shift + self.n:] == 0xA5).all()), "bytes behind the workspace were written"
        assert bool((b[self.shift + CNT_BYTES:self.shift + self.n] != 0).any()) == used, f"fix-up through the workspace: expected used = {used}"


# ---------------------------------------------------------------------------------------------------------------- 1. layouts x tails
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("layout", gr.LAYOUTS, ids=lambda l: f"tA{l[0]}tB{l[1]}")
def test_layouts_and_tails(layout, dtype):
    """Every (M, K), (N, K) and (M, N) pair of M, N in {1, 63, 64, 65, 200} and K in {1 ... 320}: 1 to 5 slabs (every has1 / has2 exit of
    the double-buffered loop), DB false (K <= 128) and true, FAST with a partial last slab (136) and the general loop (130, 100, 7, and
    M or N not a multiple of 8 where strips run along them), alpha 1, 0.5 and -2."""
    for kw in gr.layout_cases(*layout):
        run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 2. alignment
ALIGN = gr.align_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kw", ALIGN, ids=[k["tag"] for k in ALIGN])
def test_alignment(kw, dtype):
    """A, B, C, R moved by one element or given an odd ld, one at a time (vecA / vecB / vecC false in turn), N % 8 != 0 on an aligned C
    (vec8C false, vecC true), and an fp32 C from 16-bit operands."""
    run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 3. epilogue terms
EPI = gr.epilogue_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kw", EPI, ids=[k["tag"] for k in EPI])
def test_epilogue_terms(kw, dtype):
    """bias, R, both, TC_ACT_SCALE, accumulate into a 16-bit and an fp32 C, one bias per level-1 batch; results on 16-bit ties."""
    run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 4. batches
BATCH = gr.batch_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kw", BATCH, ids=[k["tag"] for k in BATCH])
def test_batches(kw, dtype):
    """nb1 = 2, nb2 = 3 with eight distinct non-contiguous strides; atomic = 1 with sC = 0: six (three) batches add into one fp32 C."""
    run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 5. caller split-K
SPLITK = gr.splitk_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kw", SPLITK, ids=[k["tag"] for k in SPLITK])
def test_splitk_atomics(kw, dtype):
    """splitk 2, 3, 128 without a workspace: fp32 atomics into C, the bias (and R) from the first split only, a short or absent last split."""
    run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 6. workspace fix-up
FIX = gr.fixup_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("how", ["exact", "one-slot-short", "misaligned"])
@pytest.mark.parametrize("case", FIX, ids=[k["tag"] for k, _ in FIX])
def test_fixup_own_split(case, how, dtype):
    """splitk = 1 with a workspace: the engine splits K itself (4 ways on one tile, 2 ways on 3 x 2 tiles), the last arrival folds the
    partials and runs the plain-store epilogue once.  One slot short or 8 bytes off 16-byte alignment: no split, same result."""
    kw, slots = case
    w = Workspace(slots - (how == "one-slot-short"), shift=8 if how == "misaligned" else 0)
    run(kw, dtype, **w.args)
    w.after(used=(how == "exact"))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("how", ["exact", "one-slot-short", "misaligned"])
def test_fixup_group_fold_129(how, dtype):
    """splitk = 129 (> 128): nine groups of up to 16 splits fold through the workspace and only the group leaders add into C atomically;
    the ninth group has one member (gm == 1) and skips the workspace.  Without a usable workspace: 129 atomic splits, same result."""
    (kw, slots), = gr.fixup129_cases(dtype)
    w = Workspace(slots - (how == "one-slot-short"), shift=8 if how == "misaligned" else 0)
    run(kw, dtype, **w.args)
    w.after(used=(how == "exact"))


# ---------------------------------------------------------------------------------------------------------------- 7. XCD renumbering, fdiv
XCD = gr.xcd_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kw", XCD, ids=[k["tag"] for k in XCD])
def test_xcd_tile_grids(kw, dtype):
    """5 x 13, 3 x 23 and 8 x 8 workgroups (65, 69, 64 tiles: T % 8 = 1, 5, 0) and 8 x 8 x (3 batches x 2 splits): every tile is computed
    once and lands in its own place."""
    run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 8. rowsum
ROWSUM = gr.rowsum_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kw", ROWSUM, ids=[k["tag"] for k in ROWSUM])
def test_rowsum(kw, dtype):
    """rowsum[m] += sum_k op(A)[m, k] from the first N tile only, over splits and level-2 batches, per level-1 batch with sRow1."""
    run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 9. bgap
BGAP = gr.bgap_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kw", BGAP, ids=[k["tag"] for k in BGAP])
def test_bgap_blocks(kw, dtype):
    run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 10. bn_part
BN = gr.bn_cases()


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("kw", BN, ids=[k["tag"] for k in BN])
def test_bn_part(kw, dtype):
    """[shift | per-tile sums | per-tile squares] of the rounded C, with an integer shift and with a NULL one."""
    run(kw, dtype)


# ---------------------------------------------------------------------------------------------------------------- 11. tc_gemm_pair
def _pair(pa, pb):
    da, db = upload(pa), upload(pb)
    ga, gb = desc(pa, da), desc(pb, db)
    lib().tc_gemm_pair(C.byref(ga), C.byref(gb), stream())
    torch.cuda.synchronize()
    check(pa, da, "pair a: ")
    check(pb, db, "pair b: ")
    sa, sb = upload(pa), upload(pb)
    lib().tc_gemm(C.byref(desc(pa, sa)), stream())
    lib().tc_gemm(C.byref(desc(pb, sb)), stream())
    torch.cuda.synchronize()
    for d, s, p in ((da, sa, pa), (db, sb, pb)):
        for name in p.expect:
            assert torch.equal(bits(d[name]), bits(s[name])), (p.tag, name)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("form", ["merged", "merged-xcd", "a-transposed"])
def test_gemm_pair(form, dtype):
    """dX (4 x 3 tiles) and dW with rowsum (3 x 2 tiles x 2 splits) in one grid (16-bit: gxA != gxB, xcd |= 2 on the dW problem), and
    the same with 9 x 8 dX tiles (XCD-aware numbering on both), and the fallbacks to two launches: fp32 storage, a transposed `a`."""
    a = dict(gr.PAIR["a"], tA=1) if form == "a-transposed" else gr.PAIR["a_big" if form == "merged-xcd" else "a"]
    _pair(Problem(dtype=dtype, **a), Problem(dtype=dtype, **gr.PAIR["b"]))


# ---------------------------------------------------------------------------------------------------------------- 12. tc_gemm_multi
def _multi(probs, with_ws=True):
    ds = [upload(p) for p in probs]
    wss = {}
    for i, p in enumerate(probs):                           # a problem the engine splits on its own gets its OWN workspace slice
        f = p.fields
        if with_ws and f["splitk"] == 1 and f["K"] >= 512:
            tiles = ((f["M"] + 63) // 64) * ((f["N"] + 63) // 64)
            wss[i] = Workspace(tiles * min(512 // tiles, f["K"] // 256, 16))
    mk = lambda bufs: (TcGemm * len(probs))(*[desc(p, d, **(wss[i].args if i in wss else {})) for i, (p, d) in enumerate(zip(probs, bufs))])
    lib().tc_gemm_multi(mk(ds), len(probs), stream())
    torch.cuda.synchronize()
    for p, d in zip(probs, ds):
        check(p, d, "multi: ")
    for w in wss.values():
        w.after(used=True)
    ss = [upload(p) for p in probs]
    arr = mk(ss)
    for i in range(len(probs)):
        lib().tc_gemm(C.byref(arr[i]), stream())
    torch.cuda.synchronize()
    for p, d, s in zip(probs, ds, ss):
        for name in p.expect:
            assert torch.equal(bits(d[name]), bits(s[name])), (p.tag, name)
    return len(wss)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_gemm_multi_merged(dtype):
    """Twelve problems of the three kinds with distinct K, M, N and values in one grid (16-bit; fp32: one launch each): the sort by K
    chunk reorders them across the kinds, two of them split K through their own workspace slices."""
    assert _multi([Problem(dtype=dtype, **kw) for kw in gr.multi_cases(12)]) == 2


@pytest.mark.parametrize("dtype", HALF, ids=_name)
@pytest.mark.parametrize("form", ["n13", "tt-member", "mixed-types"])
def test_gemm_multi_fallbacks(form, dtype):
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    if form == "n13":
        probs = [Problem(dtype=dtype, **kw) for kw in gr.multi_cases(13)]
    elif form == "tt-member":
        probs = [Problem(dtype=dtype, **(dict(kw, tA=1, tB=1) if i == 4 else kw)) for i, kw in enumerate(gr.multi_cases(12))]
    else:
        probs = [Problem(dtype=other if i == 3 else dtype, **kw) for i, kw in enumerate(gr.multi_cases(12))]
    _multi(probs)


# ---------------------------------------------------------------------------------------------------------------- 13. sigmoid
SIG = gr.sigmoid_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kw", SIG, ids=[k["tag"] for k in SIG])
def test_sigmoid(kw, dtype):
    """The one inexact epilogue, against float64 sigmoid of the exact pre-activation: fp32 storage within 2e-5 + 2e-5 |ref| (test_linear's
    bound for this activation), 16-bit storage within half a storage spacing of the reference (x 1.001) plus 2e-5.  Everything outside the
    logical C keeps the sentinel.  Measured worst errors: fp32 storage 6.0e-8 (0.001 of the bound), bf16 1.94e-3 (0.98 of it), fp16
    2.44e-4 (0.92 of it) -- the 16-bit figures are the storage rounding itself."""
    p = Problem(dtype=dtype, **kw)
    d = upload(p)
    lib().tc_gemm(C.byref(desc(p, d)), stream())
    torch.cuda.synchronize()
    got = d["C"].cpu()
    ref = p.ref
    err = (got[p.idx["C"]].double() - ref).abs()
    if p.cdtype == torch.float32:
        bound = 2e-5 + 2e-5 * ref.abs()
    else:
        mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
        spacing = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))) - mant)
        bound = 0.5 * spacing * 1.001 + 2e-5
    print(f"[gemm sigmoid] {p.tag} {_name(dtype)} C {_name(p.cdtype)}: worst |err| {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound).max()))
    outside = torch.ones(got.numel(), dtype=torch.bool)
    outside[p.idx["C"].reshape(-1)] = False
    assert torch.equal(raw(got[outside]), raw(p.bufs["C"][outside]))


# ---------------------------------------------------------------------------------------------------------------- 14. refusals
@pytest.mark.parametrize("dtype", HALF, ids=_name)
def test_refusals(dtype):
    """One call per clause of gemm_args_ok and per bn_part clause of gemm_plan: TC_ERR_ARG, nothing written.  Each refused descriptor
    differs from a valid one in the named members only and its buffers carry enough slack for the call it describes (fp32 elements in
    place of 16-bit ones, a second batch, a wider ldc); the valid descriptors run afterwards on the same buffers."""
    L, s = lib(), stream()
    p = Problem(dtype=dtype, tag="refuse", M=64, N=72, K=64, tB=1, bias=True, R=True, bn="shift", slack=40000)
    d = upload(p)
    aux = torch.zeros(1 << 16, dtype=torch.float32, device=DEV)            # stands in for the MixFFN hook arrays a clause needs non-null
    ax = aux.data_ptr()
    ffn = dict(ffn_gamma=ax, ffn_beta=ax, ffn_stat=ax, ffn_part=ax, ffn_part2=ax, ffn_d=ax, ffn_nchunk=1, ffn_chunk_n=64)
    nobn = dict(bn_part=None, bn_shift=None)
    f32 = TC_F32
    bad = {
        "A null": dict(nobn, A=None), "B null": dict(nobn, B=None), "C null": dict(nobn, C=None),
        "M = 0": dict(nobn, M=0), "N = 0": dict(nobn, N=0), "K = 0": dict(nobn, K=0), "M < 0": dict(nobn, M=-64),
        "nb1 = 0": dict(nobn, nb1=0), "nb2 = 0": dict(nobn, nb2=0), "splitk = 0": dict(nobn, splitk=0),
        "splitk without accumulate": dict(nobn, splitk=2, c_f32=1),
        "splitk into a 16-bit C": dict(nobn, splitk=2, accumulate=1),
        "splitk with an activation": dict(nobn, splitk=2, accumulate=1, c_f32=1, act=ACT_SIGMOID),
        "splitk with SCALE": dict(nobn, splitk=2, accumulate=1, c_f32=1, act=ACT_SCALE),
        "atomic without accumulate": dict(nobn, atomic=1, c_f32=1),
        "atomic into a 16-bit C": dict(nobn, atomic=1, accumulate=1),
        "act = GELU": dict(nobn, act=ACT_GELU), "act = 7": dict(nobn, act=7), "act = -1": dict(nobn, act=-1),
        "SCALE with an FFN hook": dict(nobn, act=ACT_SCALE, ffn_mode=FFN_LN_A, **ffn),
        "bgap_every < 0": dict(nobn, transB=0, bgap_every=-64), "bgap with transB": dict(nobn, bgap_every=64, bgap=8),
        "bgap_every % 64": dict(nobn, transB=0, bgap_every=32, bgap=8), "bgap % 8": dict(nobn, transB=0, bgap_every=64, bgap=4),
        "ffn_mode = -1": dict(nobn, ffn_mode=-1, **ffn), "ffn_mode = 4": dict(nobn, ffn_mode=4, **ffn),
        "FFN without gamma": dict(nobn, ffn_mode=FFN_LN_A, **dict(ffn, ffn_gamma=None)),
        "FFN without beta": dict(nobn, ffn_mode=FFN_LN_A, **dict(ffn, ffn_beta=None)),
        "FFN without stat": dict(nobn, ffn_mode=FFN_LN_A, **dict(ffn, ffn_stat=None)),
        "FFN with bgap": dict(nobn, transA=1, transB=0, c_f32=1, ffn_mode=FFN_LN_B, bgap_every=64, bgap=8, **ffn),
        "LN_A without part": dict(nobn, ffn_mode=FFN_LN_A, **dict(ffn, ffn_part=None)),
        "LN_A nchunk = 0": dict(nobn, ffn_mode=FFN_LN_A, **dict(ffn, ffn_nchunk=0)),
        "LN_A chunk_n = 0": dict(nobn, ffn_mode=FFN_LN_A, **dict(ffn, ffn_chunk_n=0)),
        "EP without d": dict(nobn, transB=0, bias=None, R=None, ffn_mode=FFN_EP, **dict(ffn, ffn_d=None)),
        "EP without part2": dict(nobn, transB=0, bias=None, R=None, ffn_mode=FFN_EP, **dict(ffn, ffn_part2=None)),
        "ffn_sRow1 < 0": dict(nobn, ffn_mode=FFN_LN_A, ffn_sRow1=-1, **ffn),
        "ffn_sPar1 > 2^31": dict(nobn, ffn_mode=FFN_LN_A, ffn_sPar1=1 << 31, **ffn),
        # gemm_plan's bn_part clauses
        "bn_part: fp32 storage": dict(dtype=f32), "bn_part: fp32 C": dict(c_f32=1), "bn_part: accumulate": dict(accumulate=1),
        "bn_part: batches": dict(nb1=2, sA1=8000, sB1=8000, sC1=8000, sR1=8000), "bn_part: batches (nb2)": dict(nb2=2, sA2=8000, sB2=8000, sC2=8000, sR2=8000),
        "bn_part: odd ldc": dict(ldc=p.fields["ldc"] + 1), "bn_part: ldc % 8": dict(ldc=p.fields["ldc"] + 4),
        "bn_part: N % 8": dict(N=68), "bn_part: C off by one element": dict(C=ptr(d, p, "C") + 2),
        "bn_part: C off by 8 bytes": dict(C=ptr(d, p, "C") + 8),
        "bn_part: an FFN hook": dict(transA=1, transB=0, ffn_mode=FFN_LN_B, **ffn),
        "bn_part: sigmoid": dict(act=ACT_SIGMOID), "bn_part: SCALE": dict(act=ACT_SCALE),
    }
    for what, over in bad.items():
        g = desc(p, d, **over)
        with pytest.raises(TcError, match="status -1"):
            L.tc_gemm(C.byref(g), s)
            pytest.fail(what + " was accepted")
    plain, withbn = desc(p, d, **nobn), desc(p, d)
    for what, call in {"pair: bn_part on a": lambda: L.tc_gemm_pair(C.byref(withbn), C.byref(plain), s),
                       "pair: bn_part on b": lambda: L.tc_gemm_pair(C.byref(plain), C.byref(withbn), s),
                       "pair: a refused": lambda: L.tc_gemm_pair(C.byref(desc(p, d, **dict(nobn, M=0))), C.byref(plain), s),
                       "multi: bn_part": lambda: L.tc_gemm_multi((TcGemm * 2)(plain, withbn), 2, s),
                       "multi: second refused": lambda: L.tc_gemm_multi((TcGemm * 2)(plain, desc(p, d, **dict(nobn, K=0))), 2, s),
                       "multi: n = 0": lambda: L.tc_gemm_multi((TcGemm * 1)(plain), 0, s),
                       "multi: null list": lambda: L.tc_gemm_multi(None, 1, s)}.items():
        with pytest.raises(TcError, match="status -1"):
            call()
            pytest.fail(what + " was accepted")
    torch.cuda.synchronize()
    for name in ("C", "bn_part"):
        assert torch.equal(raw(d[name]), raw(p.bufs[name])), name + " was written by a refused call"
    L.tc_gemm(C.byref(withbn), s)                                          # the descriptor the refusals were derived from is valid
    torch.cuda.synchronize()
    check(p, d)
    d["C"].copy_(p.bufs["C"])
    L.tc_gemm(C.byref(plain), s)
    torch.cuda.synchronize()
    assert torch.equal(bits(d["C"]), bits(p.expect["C"]))

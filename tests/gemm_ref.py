"""Host reference of tc_gemm / tc_gemm_pair / tc_gemm_multi (include/transception_hip.h), the exact input families of
tests/test_gemm_abi_gpu.py and the buffers those tests hand to the C ABI.  Nothing here needs a GPU; tests/test_gemm_ref_host.py checks it.

gemm_ref evaluates the logical product in float64 from the header's definition.  A Problem lays the same logical matrices out the way one
TcGemm describes them: every operand buffer is larger than its matrix (ld > columns, rows in front and behind, gaps between the batches and
between the bgap blocks) and NaN everywhere outside it, every output buffer is oversize and pre-filled -- with the sentinel where the op
stores, with grid values where it accumulates -- and `expect` holds the whole buffer as the call must leave it.

Exactness.  Operands are seeded integers in [-2, 2], bias / R / the old C integers in [-8, 8], alpha is 1, 0.5 or -2.  With K <= 8256 every
product and every partial sum is an integer (or half of one) below 2^24 in magnitude, so fp32 holds it exactly in ANY order of summation:
MFMA accumulation order, split-K atomics and the workspace fold cannot change a bit.  A 16-bit C is that exact value rounded once to nearest
even.  `exact` is the guard: the float64 result must survive the cast to fp32 unchanged."""
import torch

from transception_amd._lib import ACT_NONE, ACT_SCALE, ACT_SIGMOID
from transception_amd.seeded_init import seeded_tensor

SENT = -96.0                       # exact in every storage type; no result of the families below is a whole buffer of it
CNT_BYTES, PART_BYTES = 16384, 64 * 64 * 4          # gemm_plan's workspace layout: arrival counters, then one slot per tile and split
MS = NS = (1, 63, 64, 65, 200)
KS = (1, 7, 8, 64, 72, 100, 128, 130, 136, 192, 256, 320)
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))


def gemm_ref(opA, opB, alpha=1.0, bias=None, R=None, act=ACT_NONE, c_old=None, shared_c=False, rowsum_old=None, shared_rowsum=False):
    """opA [nb1, nb2, M, K]; opB [nb1, nb2, K, N] or the list of its bgap blocks along K; bias [nb1 or 1, N]; R, c_old [nb1, nb2, M, N]
    (c_old [1, 1, M, N] when the batches share one C: `shared_c`, the atomic form); rowsum_old [nb1 or 1, M].
    Returns (C, rowsum) in float64: C = act(alpha * AB + bias + R), or alpha * (AB + bias + R) for TC_ACT_SCALE, plus c_old when given;
    rowsum[b1, m] = rowsum_old + sum over b2 and k of opA (over b1 too when the level-1 batches share one vector: sRow1 = 0)."""
    A = opA.double()
    B = (torch.cat([b.double() for b in opB], dim=2) if isinstance(opB, (list, tuple)) else opB.double())
    AB = torch.matmul(A, B)
    b = bias.double()[:, None, None, :] if bias is not None else None
    if act == ACT_SCALE:
        pre = AB
        if b is not None:
            pre = pre + b
        if R is not None:
            pre = pre + R.double()
        pre = alpha * pre
    else:
        pre = alpha * AB
        if b is not None:
            pre = pre + b
        if R is not None:
            pre = pre + R.double()
        if act == ACT_SIGMOID:
            pre = torch.sigmoid(pre)
    if shared_c:
        pre = pre.sum(dim=(0, 1), keepdim=True)
    C = pre + c_old.double() if c_old is not None else pre
    rowsum = None
    if rowsum_old is not None:
        rs = A.sum(dim=3).sum(dim=1)
        if shared_rowsum:
            rs = rs.sum(dim=0, keepdim=True)
        rowsum = rowsum_old.double() + rs
    return C, rowsum


def exact(ref64):
    """The float64 result is an fp32 value: no fp32 partial sum of the exact families was rounded either."""
    return bool(torch.equal(ref64.float().double(), ref64))


def ints(tag, shape, lim):
    """Seeded integers in [-lim, lim] (float64, no -0.0)."""
    t = torch.from_numpy(seeded_tensor("gemm/" + tag, tuple(shape), 0.6 * lim)).double()
    return t.round().clamp(-lim, lim) + 0.0


def _up8(v):
    return (v + 7) // 8 * 8


class Layout:
    """Where op(X)[b1, b2, i, j] of one matrix operand lies in its flat buffer: off + b1 s1 + b2 s2 + row ld + col (+ the bgap term)."""

    def __init__(self, n1, n2, stored_t, nb1, nb2, k, misalign=False, odd=False, shared=False, bgap_every=0, bgap=0, slack=0):
        rows, cols = (n2, n1) if stored_t else (n1, n2)
        self.n1, self.n2, self.stored_t, self.nb1, self.nb2 = n1, n2, stored_t, nb1, nb2
        self.ld = _up8(cols) + 8 + (1 if odd else 0)
        nblocks = (rows + bgap_every - 1) // bgap_every if bgap_every else 1
        mat = rows * self.ld + (nblocks - 1) * bgap
        self.s2 = 0 if shared else _up8(mat) + 8 * k
        self.s1 = 0 if shared else nb2 * self.s2 + 8 * (k + 8)
        self.off = _up8(2 * self.ld) + (1 if misalign else 0)
        self.bgap_every, self.bgap = bgap_every, bgap
        span = mat if shared else (nb1 - 1) * self.s1 + (nb2 - 1) * self.s2 + mat
        self.total = self.off + span + _up8(2 * self.ld) + 8 + slack

    def index(self):
        i = torch.arange(self.n1).view(1, 1, -1, 1)
        j = torch.arange(self.n2).view(1, 1, 1, -1)
        row, col = (j, i) if self.stored_t else (i, j)
        b1 = torch.arange(self.nb1).view(-1, 1, 1, 1)
        b2 = torch.arange(self.nb2).view(1, -1, 1, 1)
        idx = self.off + b1 * self.s1 + b2 * self.s2 + row * self.ld + col
        if self.bgap_every:
            idx = idx + (row // self.bgap_every) * self.bgap
        idx = idx.expand(self.nb1, self.nb2, self.n1, self.n2)
        assert int(idx.min()) >= 0 and int(idx.max()) < self.total
        return idx


class Problem:
    """One TcGemm on host tensors.  bufs: name -> flat CPU tensor as the call receives it; off: name -> element offset of the pointer
    into it; fields: every scalar member of the struct; expect: name -> the whole output buffer afterwards (C, and rowsum / bn_part when
    asked for); ref: the float64 logical C; idx: name -> positions of the logical elements.  `misalign` / `odd` name the matrices (of "A",
    "B", "C", "R") whose pointer is moved by one element / whose ld is odd."""

    def __init__(self, tag, dtype, M, N, K, tA=0, tB=0, nb1=1, nb2=1, alpha=1.0, bias=False, R=False, act=ACT_NONE, accumulate=0, splitk=1,
                 c_f32=0, atomic=0, rowsum=False, bias_per_batch=False, rowsum_per_batch=False, bgap_every=0, bgap=0, misalign=(), odd=(),
                 shared_c=False, lim=2, bn=None, slack=0, positive=False):
        self.tag, self.dtype = tag, dtype
        if c_f32 == "auto":
            c_f32 = 0 if dtype == torch.float32 else 1
        cdtype = torch.float32 if (c_f32 or dtype == torch.float32) else dtype
        self.cdtype = cdtype
        lay = {"A": Layout(M, K, bool(tA), nb1, nb2, 2, "A" in misalign, "A" in odd, slack=slack),
               "B": Layout(K, N, bool(tB), nb1, nb2, 3, "B" in misalign, "B" in odd, bgap_every=bgap_every, bgap=bgap, slack=slack),
               "C": Layout(M, N, False, nb1, nb2, 5, "C" in misalign, "C" in odd, shared=shared_c, slack=slack)}
        if R:
            lay["R"] = Layout(M, N, False, nb1, nb2, 7, "R" in misalign, "R" in odd, slack=slack)
        self.lay = lay
        self.idx = {k: v.index() for k, v in lay.items()}
        opA, opB = ints(tag + "/A", (nb1, nb2, M, K), lim), ints(tag + "/B", (nb1, nb2, K, N), lim)
        if positive:                                           # sums far from zero: results around 256, where bf16 spacing is 2
            opA, opB = opA.abs(), opB.abs()
        self.opA, self.opB = opA, opB
        self.bufs, self.off, self.expect = {}, {}, {}

        def operand(name, logical):
            buf = torch.full((lay[name].total,), float("nan"), dtype=torch.float64)
            buf[self.idx[name]] = logical
            self.bufs[name], self.off[name] = buf.to(dtype), lay[name].off

        operand("A", opA)
        operand("B", opB)
        Rl = None
        if R:
            Rl = ints(tag + "/R", (nb1, nb2, M, N), 8)
            operand("R", Rl)
        bl, sBias1 = None, 0
        if bias:
            nbb = nb1 if bias_per_batch else 1
            sBias1 = N + 11 if bias_per_batch else 0
            bl = ints(tag + "/bias", (nbb, N), 8)
            buf = torch.full((8 + nb1 * (N + 11) + 8,), float("nan"), dtype=torch.float64)
            buf[(8 + torch.arange(nbb).view(-1, 1) * sBias1 + torch.arange(N).view(1, -1))] = bl
            self.bufs["bias"], self.off["bias"] = buf.to(dtype), 8
        # the output: sentinel where the op stores, grid values where it accumulates (the whole buffer, padding included)
        if accumulate:
            c0 = ints(tag + "/C0", (lay["C"].total,), 8)
        else:
            c0 = torch.full((lay["C"].total,), SENT, dtype=torch.float64)
        c_old = c0[self.idx["C"][:1, :1] if shared_c else self.idx["C"]] if accumulate else None
        rs0, rs_old, sRow1 = None, None, 0
        if rowsum:
            nbr = nb1 if rowsum_per_batch else 1
            sRow1 = M + 5 if rowsum_per_batch else 0
            rs0 = ints(tag + "/rs0", (8 + nb1 * (M + 5) + 8,), 8)
            self.idx["rowsum"] = 8 + torch.arange(nbr).view(-1, 1) * sRow1 + torch.arange(M).view(1, -1)
            rs_old = rs0[self.idx["rowsum"]]
        self.ref, rs = gemm_ref(opA, opB, alpha, bl, Rl, act, c_old, shared_c, rs_old, shared_rowsum=not rowsum_per_batch)
        self.bufs["C"], self.off["C"] = c0.to(cdtype), lay["C"].off
        want = c0.clone()
        want[self.idx["C"][:1, :1] if shared_c else self.idx["C"]] = self.ref
        self.expect["C"] = want.float().to(cdtype)
        if rowsum:
            self.bufs["rowsum"], self.off["rowsum"] = rs0.float(), 8
            w = rs0.clone()
            w[self.idx["rowsum"]] = rs
            self.expect["rowsum"], self.ref_rowsum = w.float(), rs
        if bn:
            # [shift | per 64-row tile: sum of (c - shift) | per tile: sum of (c - shift)^2], from the ROUNDED C
            T = (M + 63) // 64
            shift = ints(tag + "/shift", (N,), 8) if bn == "shift" else torch.zeros(N, dtype=torch.float64)
            if bn == "shift":
                self.bufs["bn_shift"], self.off["bn_shift"] = torch.cat([torch.full((4,), float("nan")), shift.float()]), 4
            c = self.ref.float().to(cdtype).double()[0, 0] - shift
            part = torch.full((N * (1 + 2 * T) + 24,), SENT, dtype=torch.float64)
            self.bufs["bn_part"], self.off["bn_part"] = part.float(), 0
            part[:N] = shift
            for t in range(T):
                part[N + t * N:N + (t + 1) * N] = c[64 * t:64 * t + 64].sum(0)
                part[N + (T + t) * N:N + (T + t + 1) * N] = (c[64 * t:64 * t + 64] ** 2).sum(0)
            self.ref_bn = part
            self.expect["bn_part"] = part.float()
        f = dict(M=M, N=N, K=K, lda=lay["A"].ld, ldb=lay["B"].ld, ldc=lay["C"].ld, ldr=lay["R"].ld if R else 0, transA=tA, transB=tB,
                 nb1=nb1, nb2=nb2, sA1=lay["A"].s1, sA2=lay["A"].s2, sB1=lay["B"].s1, sB2=lay["B"].s2, sC1=lay["C"].s1, sC2=lay["C"].s2,
                 sR1=lay["R"].s1 if R else 0, sR2=lay["R"].s2 if R else 0, alpha=float(alpha), accumulate=accumulate, act=act, splitk=splitk,
                 c_f32=c_f32, atomic=atomic, sBias1=sBias1, sRow1=sRow1, bgap_every=bgap_every, bgap=bgap)
        self.fields = f

    def exact(self):
        ok = exact(self.ref) and (not hasattr(self, "ref_rowsum") or exact(self.ref_rowsum)) and (not hasattr(self, "ref_bn") or exact(self.ref_bn))
        # inputs are storage-type values: the casts above changed nothing
        for name in ("A", "B", "R", "bias"):
            if name in self.bufs:
                b = self.bufs[name]
                ok = ok and bool(torch.equal(b[~b.isnan()].double(), b[~b.isnan()].double().round())) and float(b[~b.isnan()].abs().max()) <= 8
        return ok


# ------------------------------------------------------------------------------------------------------------------ the case tables
# Each entry is the keyword set of one Problem (dtype apart).  The GPU file runs them, the host file checks every one of them for exactness.
def layout_cases(tA, tB):
    """All (K, M) pairs of the issue's lists for one operand layout, N stepping so that every (K, N) and (M, N) pair occurs as well."""
    out = []
    for ki, K in enumerate(KS):
        for mi, M in enumerate(MS):
            N = NS[(mi + ki + 2 * tA + tB) % 5]
            out.append(dict(tag=f"lay{tA}{tB}/{M}x{N}x{K}", M=M, N=N, K=K, tA=tA, tB=tB, alpha=(1.0, 0.5, -2.0)[(ki + mi) % 3]))
    return out


def align_cases():
    out = []
    for tA, tB in LAYOUTS:
        for name in ("A", "B", "C", "R"):
            for how in ("misalign", "odd"):
                # N = 72, K = 136: a multiple of 8 everywhere, so only the named matrix takes its kernel off the 16-byte paths
                out.append(dict(tag=f"al{tA}{tB}/{how}{name}", M=65, N=72, K=136, tA=tA, tB=tB, bias=True, R=True, **{how: (name,)}))
    out.append(dict(tag="al/n68", M=65, N=68, K=136, tB=1, bias=True, R=True))              # aligned C, N % 8 != 0: vec8C false, vecC true
    out.append(dict(tag="al/n67", M=65, N=67, K=136, tB=1, bias=True, R=True))              # the scalar tail of a vecC row
    for tA, tB in LAYOUTS:                                                                      # fp32 C from 16-bit operands
        out.append(dict(tag=f"al{tA}{tB}/cf32", M=65, N=70, K=136, tA=tA, tB=tB, bias=True, R=True, c_f32=1))
        out.append(dict(tag=f"al{tA}{tB}/cf32oddC", M=65, N=72, K=136, tA=tA, tB=tB, bias=True, R=True, c_f32=1, odd=("C",)))
    return out


def epilogue_cases():
    base = dict(M=70, N=72, K=72, tB=1)
    out = [dict(tag="ep/bias", bias=True, alpha=0.5, **base), dict(tag="ep/R", R=True, alpha=-2.0, **base),
           dict(tag="ep/biasR", bias=True, R=True, alpha=0.5, **base),
           dict(tag="ep/scale", bias=True, R=True, alpha=0.5, act=ACT_SCALE, **base),
           dict(tag="ep/scale-n70", bias=True, R=True, alpha=-2.0, act=ACT_SCALE, M=70, N=70, K=72, tB=1),
           dict(tag="ep/acc", bias=True, R=True, alpha=0.5, accumulate=1, **base),
           dict(tag="ep/acc-n70", bias=True, R=True, alpha=-2.0, accumulate=1, M=70, N=70, K=72, tB=1),
           dict(tag="ep/acc-cf32", bias=True, R=True, alpha=0.5, accumulate=1, c_f32=1, **base),
           dict(tag="ep/scale-cf32", bias=True, R=True, alpha=-2.0, act=ACT_SCALE, c_f32=1, **base),
           dict(tag="ep/sbias1", bias=True, bias_per_batch=True, nb1=3, **base),
           dict(tag="ep/sbias1-cf32", bias=True, bias_per_batch=True, nb1=3, c_f32=1, **base)]
    # all-positive operands: results near 0.8 K, i.e. odd integers above 256 and half-integers above 128 -- ties of the 16-bit rounding
    for tA, tB in LAYOUTS:
        out.append(dict(tag=f"ep/ties{tA}{tB}", M=70, N=72 - 2 * tA, K=320, tA=tA, tB=tB, positive=True, alpha=(1.0, 0.5)[tB]))
    return out


def batch_cases():
    return [dict(tag="bt/2x3", M=65, N=72, K=72, tB=1, nb1=2, nb2=3, bias=True, R=True),
            dict(tag="bt/2x3-nn", M=65, N=70, K=100, nb1=2, nb2=3, bias=True, R=True, alpha=0.5),
            dict(tag="bt/2x3-dw", M=65, N=72, K=72, tA=1, nb1=2, nb2=3, c_f32=1, accumulate=1, R=True),
            dict(tag="bt/shared", M=65, N=72, K=72, tA=1, nb1=2, nb2=3, c_f32="auto", accumulate=1, atomic=1, shared_c=True, bias=True, R=True),
            dict(tag="bt/shared-rows", M=65, N=70, K=64, tB=1, nb1=3, nb2=1, c_f32="auto", accumulate=1, atomic=1, shared_c=True, bias=True)]


def splitk_cases():
    out = []
    for sk in (2, 3, 128):
        for tA, tB, K in ((1, 0, 200), (0, 1, 200), (1, 0, 8256 if sk == 128 else 520)):
            out.append(dict(tag=f"sk{sk}/{tA}{tB}/{K}", M=70, N=72, K=K, tA=tA, tB=tB, splitk=sk, accumulate=1, c_f32="auto", bias=True, alpha=0.5))
    out.append(dict(tag="sk3/R", M=70, N=67, K=200, tA=1, splitk=3, accumulate=1, c_f32="auto", bias=True, R=True))
    return out


def fixup_cases():
    """(kwargs, tiles * splits the engine's plan needs as workspace slots)"""
    a = [(dict(tag="fx/1tile", M=64, N=64, K=1024, tB=1, bias=True, R=True, alpha=0.5, act=ACT_SCALE), 1 * 4),
         (dict(tag="fx/3x2", M=130, N=128, K=512, tB=1, bias=True, R=True, alpha=0.5, act=ACT_SCALE), 6 * 2),
         (dict(tag="fx/3x2-nn", M=130, N=126, K=512, bias=True, R=True, alpha=-2.0), 6 * 2)]
    return a


def fixup129_cases(dtype):
    K = 2064 if dtype == torch.float32 else 8256
    return [(dict(tag=f"fx129/{K}", M=70, N=64, K=K, tA=1, splitk=129, accumulate=1, c_f32="auto", bias=True, rowsum=True), 2 * 129)]


def xcd_cases():
    # grid.x x grid.y workgroups of 64 x 64; K = 8: every tile its own values (random operands), nothing but the tile index differs
    return [dict(tag="xcd/5x13", M=13 * 64 - 3, N=5 * 64 - 7, K=8, tB=1, bias=True),
            dict(tag="xcd/3x23", M=23 * 64 - 60, N=3 * 64 - 8, K=8, R=True),
            dict(tag="xcd/8x8", M=512, N=512, K=8, tB=1),
            dict(tag="xcd/8x8-dw", M=505, N=512, K=8, tA=1, c_f32=1),
            dict(tag="xcd/z3split", M=8 * 64 - 1, N=8 * 64, K=136, tA=1, nb1=3, splitk=2, accumulate=1, c_f32="auto", bias=True, bias_per_batch=True)]


def rowsum_cases():
    out = []
    for tA in (1, 0):
        for M in (63, 130):
            for sk in (1, 3):
                out.append(dict(tag=f"rs/{tA}/{M}/sk{sk}", M=M, N=72, K=200, tA=tA, tB=0, splitk=sk, accumulate=1, c_f32="auto", rowsum=True, bias=True))
            out.append(dict(tag=f"rs/{tA}/{M}/srow1", M=M, N=130, K=136, tA=tA, tB=0, nb1=2, accumulate=1, c_f32="auto", rowsum=True, rowsum_per_batch=True))
            out.append(dict(tag=f"rs/{tA}/{M}/shared", M=M, N=72, K=72, tA=tA, tB=0, nb1=2, nb2=2, accumulate=1, c_f32="auto", rowsum=True))
    return out


def bgap_cases():
    out = []
    for gap in (8, 72):
        for N in (64, 60):                                     # N = 60: the general loop (N % 8 != 0 with B stored [K, N])
            for tA in (0, 1):
                out.append(dict(tag=f"bg/{gap}/{N}/{tA}", M=65, N=N, K=192, tA=tA, tB=0, bgap_every=64, bgap=gap, bias=True))
    out.append(dict(tag="bg/8/short", M=65, N=64, K=168, tB=0, bgap_every=64, bgap=8))          # the last block is not full
    return out


def bn_cases():
    return [dict(tag=f"bn/{M}/{N}/{bn}", M=M, N=N, K=64, tB=1, lim=1, bn=bn) for M in (64, 100, 200) for N in (8, 72) for bn in ("shift", "null")]


PAIR = dict(a=dict(tag="pair/dx", M=200, N=136, K=72), b=dict(tag="pair/dw", M=130, N=72, K=200, tA=1, c_f32=1, accumulate=1, splitk=2, rowsum=True),
            # 9 x 8 tiles: the dX problem of a pair takes the XCD-aware numbering as well
            a_big=dict(tag="pair/dx-big", M=520, N=512, K=72, R=True, alpha=0.5))


def multi_cases(n=12):
    """n problems of the three kinds a Linear produces, every one with its own M, N, K and values; K is neither sorted nor sorted by kind, so
    the engine's stable sort by K chunk reorders them across the kinds."""
    ks = (1024, 512, 192, 320, 136, 64, 72, 256, 200, 128, 448, 100, 384)
    out = []
    for i in range(n):
        kind, K = i % 3, ks[i]
        M, N = 40 + 23 * i, 8 * (3 + (5 * i) % 11)
        if i in (8, 9):                                        # >= 64 tiles: XCD-aware numbering inside the merged grid (forward: tc_xcd_tile;
            M, N = 520 - 8 * (i - 8), 512                      # weight gradient: the split-major deal only)
        if kind == 0:
            kw = dict(tB=1, bias=True, R=(i % 2 == 0), alpha=0.5)
        elif kind == 1:
            kw = dict(R=True, alpha=-2.0)
        else:
            kw = dict(tA=1, c_f32=1, accumulate=1, splitk=1 + i % 4, rowsum=True, bias=(i % 2 == 1))
        out.append(dict(tag=f"multi{n}/{i}", M=M, N=N, K=K, **kw))
    return out


def sigmoid_cases():
    return [dict(tag="sig/lds", M=70, N=72, K=72, tB=1, bias=True, R=True, alpha=0.5, act=ACT_SIGMOID),
            dict(tag="sig/rows", M=70, N=70, K=100, tB=0, bias=True, alpha=0.5, act=ACT_SIGMOID),
            dict(tag="sig/cf32", M=70, N=72, K=72, tA=1, bias=True, alpha=0.5, act=ACT_SIGMOID, c_f32=1)]


def all_exact_cases(dtype):
    """Every keyword set whose result the GPU file compares exactly, for the host guard."""
    out = []
    for tA, tB in LAYOUTS:
        out += layout_cases(tA, tB)
    out += align_cases() + epilogue_cases() + batch_cases() + splitk_cases() + xcd_cases() + rowsum_cases() + bgap_cases()
    out += [kw for kw, _ in fixup_cases()] + [kw for kw, _ in fixup129_cases(dtype)]
    out += list(PAIR.values()) + multi_cases(12) + multi_cases(13)
    if dtype != torch.float32:
        out += bn_cases()
    return out

"""Host reference of the LayerNorm family of csrc/norm.hip (include/transception_hip.h: tc_layernorm_fwd, tc_layernorm_ps_fwd, tc_layernorm_bwd,
tc_layernorm_ps_bwd, tc_layernorm_bwd_params, tc_layernorm_bwd_defer, tc_layernorm_fold), in float64 on CPU tensors, with the operands, the error
bounds and the case table of tests/test_layernorm_abi_gpu.py.  tests/test_ln_ref_host.py holds the reference to torch.nn.functional.layer_norm
and its autograd, shows that the bounds hold for honest fp32 arithmetic in several orders, and that they catch a list of mistakes.

Layout: an operand of the reference is [groups, rows, C] (stacked row blocks), its parameters [groups, C] -- in device memory the parameters of
block g stand g * pstride elements behind those of block 0.  A pixel-shuffled LayerNorm reads x as the un-shuffled [B H W, p p C] matrix: output
row (b, h p + p1, w p + p2) is the C-wide chunk p1 p + p2 of row (b, h, w) (`ps_rows`, ln_row_off of the kernels).

Exactness rule (as tests/dw_ref.py): maps and gradients are multiples of 1/2 with |v| <= 2, gamma and beta multiples of 1/4 with |v| <= 2.  What
follows from it exactly is asserted bit for bit: the row mean for power-of-two C, dbeta without activation (a column sum of grid values, exact
in any order while rows * max|dy| / quantum + |initial| / quantum < 2^24), tc_layernorm_fold on grid-valued partials.  rstd, y, dx and dgamma go
through rsqrtf and order-dependent roundings: each has an elementwise bound derived below (`fwd_bounds`, `bwd_bounds`), never a tuned tolerance.

Figures in the bounds that are ASSUMED, not derived: RSQRT_ULP (the HIP math documentation is not part of the toolchain's files; the hardware
reciprocal square root is specified to 1 ulp, 2 ulp are allowed here) and PHI_ERR_16 (taken from tests/test_ops_gpu.py::
test_gelu_16bit_polynomial_against_erf, which asserts it for every storage value of [-8, 8])."""
import math
import zlib

import torch

from dw_ref import NAN, SENT, Map, Params, halves, in_map, is_f32_value, out_map  # noqa: F401  (one set of buffer idioms for the ABI suites)

ACT_NONE, ACT_GELU = 0, 4
U = 2.0 ** -24                      # unit roundoff of fp32
RSQRT_ULP = 2.0                     # ASSUMED accuracy of rsqrtf in units of the last place (1 ulp <= 2 U relative)
# |Phi~(z) - Phi(z)| of the fp32 kernels (gelu_cdf_pdf, csrc/tc_common.h): Abramowitz-Stegun 7.1.26 has |erf error| <= 1.5e-7, Phi = (1 + erf) / 2
# halves it; the arithmetic on top -- Horner in t <= 1 with sum|a_i| = 4.48 (gamma_10 * 4.48 <= 45 U), the reciprocal (<= 3 U relative), the
# exponential (argument error gamma_5 z^2 with z^2 e^{-z^2} <= 1/e, the hardware exp2 taken as 1 ulp like rsqrtf: <= 5 U absolute), three products
# and the final subtraction -- stays under (45 + 3 + 5 + 3) / 2 + 1 < 32 U after the factor 0.5; 48 U are allowed.
PHI_ERR_32 = 0.75e-7 + 48 * U
# the 16-bit kernels: the forward polynomial's absolute error in Phi as test_gelu_16bit_polynomial_against_erf asserts it (1.05e-5 |x| on x Phi(x));
# their backward keeps the A-S form with the hardware reciprocal (error as PHI_ERR_32), which the same figure covers
PHI_ERR_16 = 1.05e-5
PDF_ERR = 4 * U                     # |pdf~ - pdf|: 0.3989 * (5 U from the exponential) + one rounding of a value <= 0.4
GELU_D1, GELU_D2 = 1.13, 0.8        # max |gelu'| = 1.129, max |gelu''| = 2 pdf(0) = 0.798
MANT_EMIN = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}


def gam(n):
    """gamma_n = n U / (1 - n U): the relative error of a product of n factors (1 + delta), |delta| <= U (Higham, Lemma 3.1)."""
    assert n * U < 0.01
    return n * U / (1.0 - n * U)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------------------------------------------------------- the reference
def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def _g3(t):
    """[rows, C] -> [1, rows, C]; parameters [C] -> [1, C]."""
    return t.double() if t.dim() == 3 else t.double()[None]


def _p3(p):
    return (p.double() if p.dim() == 2 else p.double()[None])[:, None, :]          # [groups, 1, C]


def ps_rows(B, H, W, p):
    """(source row, chunk) of every output row of the pixel-shuffled map, ln_row_off written out: output row (b, oh, ow) of the [B, H p, W p] map
    reads chunk (oh % p) p + ow % p of source row (b H + oh / p) W + ow / p."""
    r = torch.arange(B * H * p * W * p)
    ow, t = r % (W * p), r // (W * p)
    oh, b = t % (H * p), t // (H * p)
    return (b * H + oh // p) * W + ow // p, (oh % p) * p + ow % p


def ps_gather(x2, B, H, W, p, C, swap=False):
    """x2 [B H W, p p C] -> [B Hp Wp, C] (swap: the chunk index with p1 and p2 exchanged -- a mutation of the host tests)."""
    src, ch = ps_rows(B, H, W, p)
    if swap:
        ch = (ch % p) * p + ch // p
    return x2.reshape(B * H * W, p * p, C)[src, ch]


def ps_scatter(v, B, H, W, p, C):
    """The inverse of ps_gather: [B Hp Wp, C] -> [B H W, p p C]."""
    src, ch = ps_rows(B, H, W, p)
    out = torch.zeros(B * H * W, p * p, C, dtype=v.dtype)
    out[src, ch] = v
    return out.reshape(B * H * W, p * p * C)


def fwd(x, gamma, beta, eps, act=ACT_NONE):
    """(y, mean, rstd): biased variance, eps inside the square root (nn.LayerNorm), optionally the exact-erf GELU behind it.
    x [rows, C] with gamma / beta [C], or [groups, rows, C] with [groups, C]."""
    x3 = _g3(x)
    mean = x3.mean(-1, keepdim=True)
    d = x3 - mean
    rstd = ((d * d).mean(-1, keepdim=True) + eps).rsqrt()
    y = d * rstd * _p3(gamma) + _p3(beta)
    if act == ACT_GELU:
        y = gelu(y)
    sh = x.shape
    return y.reshape(sh), mean.reshape(sh[:-1]), rstd.reshape(sh[:-1])


def bwd(dy, x, gamma, beta, eps, act=ACT_NONE, dres=None, ps=None):
    """(dx, dgamma, dbeta), written out from the formulas:  xh = (x - mean) rstd,  dz = dy gelu'(xh gamma + beta) (or dy),  dbeta = sum_rows dz,
    dgamma = sum_rows dz xh,  a = dz gamma,  dx = rstd (a - mean_C(a) - xh mean_C(a xh)) (+ dres).
    Groups: x, dy, dres [groups, rows, C] with gamma / beta [groups, C].  ps = (B, H, W, p): x (and dx) are the un-shuffled [B H W, p p C] matrix,
    dy is indexed by output pixel."""
    if ps is not None:
        C = dy.shape[-1]
        dx, dg, db = bwd(dy, ps_gather(x.double(), *ps, C), gamma, beta, eps, act)
        return ps_scatter(dx, *ps, C), dg, db
    x3, dy3, g = _g3(x), _g3(dy), _p3(gamma)
    mean = x3.mean(-1, keepdim=True)
    d = x3 - mean
    rstd = ((d * d).mean(-1, keepdim=True) + eps).rsqrt()
    xh = d * rstd
    dz = dy3 * gelu_grad(xh * g + _p3(beta)) if act == ACT_GELU else dy3
    dbeta, dgamma = dz.sum(1), (dz * xh).sum(1)
    a = dz * g
    dx = rstd * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + _g3(dres)
    pshape = gamma.shape
    return dx.reshape(x.shape), dgamma.reshape(pshape), dbeta.reshape(pshape)


def fold(part, nblk, C, groups):
    """tc_layernorm_fold's sums of one site: part [groups][nblk][dgamma C | dbeta C] -> (dgamma, dbeta) [groups, C], float64."""
    s = part.double().reshape(groups, nblk, 2, C).sum(1)
    return s[:, 0], s[:, 1]


# ---------------------------------------------------------------------------------------------------------------- dispatcher geometry, restated
def lane_group(C):
    """(GS, NV) of TC_LN_DISPATCH."""
    q = C // 4
    for lim, cls in ((16, (16, 1)), (32, (32, 1)), (64, (64, 1)), (128, (64, 2)), (256, (64, 4)), (320, (64, 5))):
        if q <= lim:
            return cls
    return 64, 8


def bwd_nblk(rows, C, with_params=True, deferred=False):
    """ln_bwd_nblk: workgroups of a backward launch (tc_layernorm_bwd_nblk is the deferred, with-parameters value)."""
    q = C // 4
    GS = 16 if q <= 16 else (32 if q <= 32 else 64)
    ilp = q <= 64 and rows >= 8192
    rpg = max(1, min(4, rows // ((256 // GS) * 1024))) if with_params else 1
    if ilp and rpg < 2:
        rpg = 2
    cap = (4096 if deferred else 1024) if with_params else 8192
    return max(1, min(cap, -(-rows // ((256 // GS) * rpg))))


def v8_rows_in_flight(rows, C, nblk):
    """The host's rpt rule of ln_bwd_v8_kernel: rows the grid takes per iteration with one row per 8-channel lane group."""
    rpi = nblk * (2048 // C)
    return 4 if rows >= 4 * rpi else (2 if rows >= 2 * rpi else 1)


def scratch_floats(C, groups, nblk):
    """What a launch with a usable workspace needs: 4096 counter words + one parked partial row per workgroup."""
    return 4096 + groups * nblk * 2 * C


# ---------------------------------------------------------------------------------------------------------------- error bounds
def ulp_of(w, dtype):
    """Spacing of the 16-bit storage type at |w| (subnormals included)."""
    mant, emin = MANT_EMIN[dtype]
    return torch.exp2(torch.floor(torch.log2(w.abs().clamp_min(2.0 ** emin))) - mant)


def excess(got, want64, bound, dtype):
    """|got - want64| - (bound + half a storage spacing for 16-bit storage): <= 0 where the check holds, +inf where got is not finite."""
    tol = bound if dtype == torch.float32 else bound + 0.5 * ulp_of(want64, dtype)
    e = (got.double() - want64).abs() - tol
    return torch.where(torch.isfinite(got.double()), e, torch.full_like(e, float("inf")))


def fwd_bounds(x, gamma, beta, eps, act=ACT_NONE, half=False, sums_exact=True):
    """Elementwise bounds (mean, rstd, y) on |computed - exact| for the forward computed in fp32 from fp32 values, whatever the order of the sums and
    whichever products are fused with an add; y before the rounding to a 16-bit storage type (`excess` adds that).  Notation: every fp32 operation
    returns the exact result times (1 + delta), |delta| <= U; a product of n such factors is 1 + theta_n, |theta_n| <= gamma_n = gam(n)."""
    x3, g, b = _g3(x), _p3(gamma), _p3(beta)
    C = x3.shape[-1]
    mu = x3.mean(-1, keepdim=True)
    d = x3 - mu
    v = (d * d).mean(-1, keepdim=True) + eps
    r = v.rsqrt()
    # mean = fl(fl(sum x) fl(1 / C)).  A sum of C terms in any order has C - 1 additions on the path of each term: error <= gamma_{C-1} sum|x|; the
    # rounded 1 / C and the product add two factors: <= gamma_{C+1} sum|x| / C.  Where every partial sum is exactly representable (sums_exact: grid
    # values, sum|x| / quantum < 2^24, `premise`) only those two factors remain: <= gamma_2 |mean|; for a power-of-two C both are exact as well and
    # the mean has no error at all (the tests assert it bit for bit).
    Emu = gam(C + 1) * x3.abs().mean(-1, keepdim=True)
    if sums_exact:
        Emu = torch.zeros_like(mu) if C & (C - 1) == 0 else gam(2) * mu.abs()
    # d^ = fl(x - mean^) = (x - mean^)(1 + delta):  |d^ - d| <= Emu + U |x - mean^| <= Emu (1 + U) + U |d|
    Ed = Emu * (1 + U) + U * d.abs()
    # sum_j d^_j^2: one rounding per square (none when fused), C - 1 additions: sum d^_j^2 (1 + theta_C).  Times fl(1 / C), rounded (or fused), plus
    # eps, rounded: three more factors, and since every term is >= 0,  v^ = (sum d^_j^2 / C + eps)(1 + theta_{C+3}).
    # |d^_j^2 - d_j^2| = |e_j| |2 d_j + e_j| <= Ed_j (2 |d_j| + Ed_j)
    Evar = (Ed * (2 * d.abs() + Ed)).mean(-1, keepdim=True)
    Ev = Evar * (1 + gam(C + 3)) + gam(C + 3) * v
    rho = Ev / v                                                               # relative error of the argument of rsqrtf
    assert float(rho.max()) < 0.5
    # rstd^ = rsqrtf(v^) = v^^{-1/2} (1 + RSQRT_ULP ulp), 1 ulp <= 2 U relative;  v^^{-1/2} = r (1 + e)^{-1/2} with |e| <= rho, largest at e = -rho
    Er = r * ((1 - rho) ** -0.5 * (1 + 2 * U * RSQRT_ULP) - 1)
    # t^ = fl(fl(d^ rstd^) gamma) = d^ rstd^ gamma (1 + theta_2) (fewer factors when fused);  y^ = fl(t^ + beta) = (t^ + beta)(1 + delta)
    t = d * r * g
    Et = g.abs() * ((d.abs() + Ed) * (r + Er) * (1 + gam(2)) - d.abs() * r)
    Ey = Et * (1 + U) + U * (t.abs() + b.abs())
    y = t + b
    if act == ACT_GELU:
        # out^ = fl(y^ Phi~(y^)):  |gelu(y^) - gelu(y)| <= max|gelu'| Ey;  |y^| |Phi~ - Phi| <= (|y| + Ey) PHI_ERR;  one rounding of the product
        phi = PHI_ERR_16 if half else PHI_ERR_32
        Eg = GELU_D1 * Ey + (y.abs() + Ey) * phi
        Ey = Eg + U * (gelu(y).abs() + Eg)
    sh = x.shape
    return Emu.reshape(sh[:-1]), Er.reshape(sh[:-1]), Ey.reshape(sh)


def bwd_bounds(dy, x, gamma, beta, eps, act=ACT_NONE, dres=None, half=False, dg0=None, db0=None, ps=None):
    """Elementwise bounds (dx, dgamma, dbeta) on |computed - exact| for the backward computed in fp32 from the saved statistics mean^ = fl(mean),
    rstd^ = fl(rstd) (the float64 statistics rounded once: |mean^ - mean| <= U |mean|, |rstd^ - rstd| <= U rstd), any order, any fusion; dx before
    the rounding to 16-bit storage.  dg0 / db0: the values dgamma / dbeta are added to ([groups, C]; they enter the sums as one more term)."""
    if ps is not None:
        C = dy.shape[-1]
        Edx, Edg, Edb = bwd_bounds(dy, ps_gather(x.double(), *ps, C), gamma, beta, eps, act, None, half, dg0, db0)
        return ps_scatter(Edx, *ps, C), Edg, Edb
    x3, dy3, g, b = _g3(x), _g3(dy), _p3(gamma), _p3(beta)
    n, C = x3.shape[1], x3.shape[2]
    mu = x3.mean(-1, keepdim=True)
    d = x3 - mu
    r = ((d * d).mean(-1, keepdim=True) + eps).rsqrt()
    xh = d * r
    Emu, Er = U * mu.abs(), U * r
    # xh^ = fl(fl(x - mean^) rstd^):  d^ as in fwd_bounds, then one more factor
    Ed = Emu * (1 + U) + U * d.abs()
    Exh = (d.abs() + Ed) * (r + Er) * (1 + U) - d.abs() * r
    if act == ACT_GELU:
        # z^ = fl(fl(xh^ gamma) + beta): the error of xh^ carried through, two roundings on each term;  gelu'(z^): |gelu''| <= GELU_D2 carries Ez,
        # Phi~ and z^ pdf~ have their own errors, the product and the sum round (|gelu'| <= 1.13, |z pdf| <= 0.25: 2 U covers both)
        z = xh * g + b
        Ez = g.abs() * Exh + gam(2) * (g.abs() * (xh.abs() + Exh) + b.abs())
        gp = gelu_grad(z)
        Egp = GELU_D2 * Ez + (PHI_ERR_16 if half else PHI_ERR_32) + (z.abs() + Ez) * PDF_ERR + 2 * U
        dz = dy3 * gp
        Edz = dy3.abs() * (Egp * (1 + U) + U * gp.abs())                       # dz^ = fl(dy gelu'^)
    else:
        dz, Edz = dy3, torch.zeros_like(dy3)
    # dbeta = d0 + sum_rows dz^: n + 1 terms, n additions on the path of each (atomics, folds and partial sums are only another order)
    d0b = torch.zeros(x3.shape[0], C, dtype=torch.float64) if db0 is None else db0.double().reshape(-1, C).abs()
    d0g = torch.zeros(x3.shape[0], C, dtype=torch.float64) if dg0 is None else dg0.double().reshape(-1, C).abs()
    Edb = gam(n) * (d0b + (dz.abs() + Edz).sum(1)) + Edz.sum(1)
    # dgamma = d0 + sum_rows fl(dz^ xh^) (the product unrounded when fused into the accumulation)
    pr = dz * xh
    Epr = (dz.abs() + Edz) * (xh.abs() + Exh) * (1 + U) - pr.abs()
    Edg = gam(n) * (d0g + (pr.abs() + Epr).sum(1)) + Epr.sum(1)
    # a^ = fl(dz^ gamma);  s1^ = fl(fl(sum_C a^) fl(1 / C)),  s2^ = fl(fl(sum_C fl(a^ xh^)) fl(1 / C)): C - 1 additions, 1 / C, the product
    a = dz * g
    Ea = g.abs() * Edz * (1 + U) + U * a.abs()
    s1 = a.mean(-1, keepdim=True)
    Es1 = (gam(C + 1) * (a.abs() + Ea) + Ea).mean(-1, keepdim=True)
    q = a * xh
    Eq = (a.abs() + Ea) * (xh.abs() + Exh) * (1 + U) - q.abs()
    s2 = q.mean(-1, keepdim=True)
    Es2 = (gam(C + 1) * (q.abs() + Eq) + Eq).mean(-1, keepdim=True)
    # w^ = fl(fl(a^ - s1^) - fl(xh^ s2^)): the three terms' own errors, then at most three roundings on any of them
    w = a - s1 - xh * s2
    xs = (xh.abs() + Exh) * (s2.abs() + Es2)
    Ew = Ea + Es1 + (xs - (xh * s2).abs()) + gam(3) * (a.abs() + Ea + s1.abs() + Es1 + xs)
    # dx^ = fl(fl(rstd^ w^) + dres) (one rounding when fused, or without dres)
    Erw = (r + Er) * (w.abs() + Ew) * (1 + U) - r * w.abs()
    Edx = Erw * (1 + U) + U * ((r * w).abs() + (0.0 if dres is None else _g3(dres).abs()))
    return Edx.reshape(x.shape), Edg.reshape(gamma.shape), Edb.reshape(gamma.shape)


# ---------------------------------------------------------------------------------------------------------------- inputs and buffers
def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def quarters2(tag, shape, dtype=torch.float32):
    """Seeded multiples of 1/4 with |v| <= 2: exact in bf16 (a sign, 2 integer and 2 fraction bits) and fp16."""
    return (torch.randint(-8, 9, shape, generator=_gen("q2/" + tag)).float() / 4).to(dtype)


def max_offset(dtype):
    """The offset of the `offset rows` case: fp32 512; 16-bit the largest at which offset + grid is still stored with step 1/2 (the binade below
    2^(mantissa bits): bf16 [64, 128), fp16 [512, 1024))."""
    if dtype == torch.float32:
        return 512.0
    return 2.0 ** MANT_EMIN[dtype][0] - 2.5


class Case:
    """One LayerNorm problem with every operand of both directions, laid out for the C ABI.  Row strides: ldx = C + pad, ldy = C + 2 pad, lddy = C + 3 pad,
    lddx = C + 4 pad, ldres = C + 5 pad (pad 8: every row piece keeps the 16-byte alignment of the 8-wide kernels; `ldx`, `lead` override);
    x and dy stand `lead` elements behind the start of their buffers."""

    def __init__(self, tag, rows, C, groups=1, pgap=8, eps=1e-5, act=ACT_NONE, kind="grid", ldx=None, lead=8, ps=None, pad=8, dtypes=None):
        self.tag, self.rows, self.C, self.groups, self.act, self.kind, self.ps, self.lead = tag, rows, C, groups, act, kind, ps, lead
        self.eps = f32(eps)                                                   # the entry takes a float
        self.pstride = C + pgap if groups > 1 else 0
        self.ld = dict(x=ldx or C + pad, y=C + 2 * pad, dy=C + 3 * pad, dx=C + 4 * pad, res=C + 5 * pad)
        if ps is not None:
            B, H, W, p = ps
            assert rows == B * H * p * W * p and groups == 1
            self.src_rows, self.src_cols = B * H * W, p * p * C
            self.ld["x"], self.ld["dx"] = self.src_cols + pad, self.src_cols + 2 * pad       # both wider than p p C
        self.dtypes = dtypes
        self._built = {}

    def on(self, dtype):
        """The operands in one storage type (built once)."""
        if dtype not in self._built:
            self._built[dtype] = Operands(self, dtype)
        return self._built[dtype]


class Operands:
    def __init__(self, c, dtype):
        self.c, self.dtype, self.tag = c, dtype, f"{c.tag}/{str(dtype).split('.')[-1]}"
        G, R, C = c.groups, c.rows, c.C
        tot = G * R
        if c.ps is None:
            self.x = in_map(c.tag + "/x", tot, C, c.ld["x"], dtype, c.lead)
            if c.kind == "offset":
                self.x.logical().copy_((self.x.logical().double() + max_offset(dtype)).to(dtype))
            elif c.kind == "const":
                self.x.logical().copy_(self.x.logical()[:, :1].expand(tot, C))
        else:
            self.x = in_map(c.tag + "/x", c.src_rows, c.src_cols, c.ld["x"], dtype, c.lead)
        self.dy = in_map(c.tag + "/dy", tot, C, c.ld["dy"], dtype, c.lead)
        self.res = in_map(c.tag + "/res", tot, C, c.ld["res"], dtype, 0)
        n = max(c.pstride, C)
        self.gamma = Params(c.tag + "/gamma", C, G, n, dtype, quarters2, NAN)
        self.beta = Params(c.tag + "/beta", C, G, n, dtype, quarters2, NAN)
        self._ref = {}

    # operands as the reference takes them
    def x3(self):
        c = self.c
        if c.ps is not None:
            return ps_gather(self.x.logical().double(), *c.ps, c.C)[None]
        return self.x.logical().double().reshape(c.groups, c.rows, c.C)

    def dy3(self):
        return self.dy.logical().double().reshape(self.c.groups, self.c.rows, self.c.C)

    def res3(self):
        return self.res.logical().double().reshape(self.c.groups, self.c.rows, self.c.C)

    def g2(self):
        return self.gamma.blocks().double()

    def b2(self):
        return self.beta.blocks().double()

    # output buffers before the call
    def y0(self):
        return out_map(self.tag + "/y0", self.c.groups * self.c.rows, self.c.C, self.c.ld["y"], self.dtype, False, 0)

    def dx0(self, ld=None):
        c = self.c
        if c.ps is not None:
            return out_map(self.tag + "/dx0", c.src_rows, c.src_cols, c.ld["dx"], self.dtype, False, 0)
        return out_map(self.tag + "/dx0", c.groups * c.rows, c.C, ld or c.ld["dx"], self.dtype, False, 0)

    def dg0(self):
        return Params(self.tag + "/dg0", self.c.C, self.c.groups, max(self.c.pstride, self.c.C), torch.float32, halves, SENT)

    def db0(self):
        return Params(self.tag + "/db0", self.c.C, self.c.groups, max(self.c.pstride, self.c.C), torch.float32, halves, SENT)

    # float64 references and bounds (computed once per case and storage type, shared by the forward and the backward tests)
    def _cached(self, key, fn):
        if key not in self._ref:
            self._ref[key] = fn()
        return self._ref[key]

    def half(self):
        return self.dtype != torch.float32

    def ref_fwd(self):
        """(y, mean, rstd) with the group axis folded into the rows, as the buffers hold them."""
        def make():
            y, m, r = fwd(self.x3(), self.g2(), self.b2(), self.c.eps, self.c.act)
            return y.reshape(-1, self.c.C), m.reshape(-1), r.reshape(-1)
        return self._cached("fwd", make)

    def bound_fwd(self):
        def make():
            em, er, ey = fwd_bounds(self.x3(), self.g2(), self.b2(), self.c.eps, self.c.act, self.half(), self.sums_exact())
            return ey.reshape(-1, self.c.C), em.reshape(-1), er.reshape(-1)
        return self._cached("fwdb", make)

    def stats32(self):
        """The statistics a backward call is given: the float64 ones rounded once to fp32."""
        _, m, r = self.ref_fwd()
        return m.float(), r.float()

    def _xsrc(self):
        return self.x.logical().double() if self.c.ps is not None else self.x3()

    def ref_bwd(self, res=False):
        return self._cached(("bwd", res), lambda: bwd(self.dy3() if self.c.ps is None else self.dy3()[0], self._xsrc(), self.g2() if self.c.ps is None
                                                      else self.g2()[0], self.b2() if self.c.ps is None else self.b2()[0], self.c.eps, self.c.act,
                                                      self.res3() if res else None, self.c.ps))

    def bound_bwd(self, res=False, dg0=None, db0=None):
        ps = self.c.ps
        return self._cached(("bwdb", res, dg0 is not None), lambda: bwd_bounds(
            self.dy3() if ps is None else self.dy3()[0], self._xsrc(), self.g2() if ps is None else self.g2()[0],
            self.b2() if ps is None else self.b2()[0], self.c.eps, self.c.act, self.res3() if res else None, self.half(),
            None if dg0 is None else dg0.blocks(), None if db0 is None else db0.blocks(), ps))

    # premises
    def sums_exact(self):
        """Every partial sum of a row of x is exactly representable: multiples of 1/2 (after the offset too) with sum|x| / (1/2) < 2^24."""
        x = self.x3()
        return bool(((x * 2) % 1 == 0).all()) and float(x.abs().sum(-1).max()) * 2 < 2.0 ** 24

    def dbeta_exact(self):
        """dbeta without activation is a column sum of grid values on a grid-valued start: rows * max|dy| / quantum + |start| / quantum < 2^24."""
        dy = self.dy3()
        return self.c.act == ACT_NONE and bool(((dy * 2) % 1 == 0).all()) and (float(dy.abs().sum(1).max()) + 2.0) * 2 < 2.0 ** 24

    def premise(self):
        """The grids, the exact sums, and that mean (power-of-two C) and dbeta (no activation) are fp32 values."""
        c = self.c
        dy, g, b = self.dy3(), self.g2(), self.b2()
        assert bool(((dy * 2) % 1 == 0).all()) and float(dy.abs().max()) <= 2.0, self.tag
        for t in (g, b):
            assert bool(((t * 4) % 1 == 0).all()) and float(t.abs().max()) <= 2.0, self.tag
        for m in (self.x, self.dy, self.res, self.gamma, self.beta):           # the storage type holds the values: nothing was rounded away
            assert torch.equal(m.flat.double().nan_to_num(7.0).to(self.dtype).double(), m.flat.double().nan_to_num(7.0)), self.tag
        x = self.x3()
        lim = max_offset(self.dtype) + 2.0 if c.kind == "offset" else 2.0
        assert bool(((x * 2) % 1 == 0).all()) and float(x.abs().max()) <= lim and self.sums_exact(), self.tag
        if c.kind == "offset":
            assert float(x.min()) >= max_offset(self.dtype) - 2.0
        if c.kind == "const":
            assert float((x - x[..., :1]).abs().max()) == 0.0
        _, mean, _ = self.ref_fwd()
        if c.C & (c.C - 1) == 0:
            assert is_f32_value(mean), self.tag
        if c.act == ACT_NONE:
            assert self.dbeta_exact(), self.tag
            db = self.ref_bwd()[2].reshape(c.groups, c.C) + self.db0().blocks().double()
            assert is_f32_value(db), self.tag
        return True


# ---------------------------------------------------------------------------------------------------------------- the cases of test_layernorm_abi_gpu.py
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ALL, HALF = (F32, BF16, F16), (BF16, F16)
WIDTHS = (64, 128, 256, 320, 1024, 1280, 2048)        # one C per (GS, NV) class of TC_LN_DISPATCH
PARTIAL = (4, 36, 160)                                # partially filled lane groups of the first three classes
ROWS = 37                                             # ragged against every rows-per-block value (256 / GS = 16, 8, 4)
V8_CS = (64, 128, 256, 512)
BIG = 65541                                           # >= 65536: the forward's 8-wide kernel; 5 rows into the next group of four


def _cases():
    t = {}

    def add(c):
        assert c.tag not in t
        t[c.tag] = c
    for C in WIDTHS + PARTIAL:
        add(Case(f"w{C}", ROWS, C))
    add(Case("eps025", ROWS, 64, eps=0.25))           # an eps that 16-bit rounding cannot hide: omitted or misplaced, it moves y by percents
    add(Case("offset", ROWS, 64, kind="offset"))      # x = offset + grid: E[x^2] - mean^2 cancels
    add(Case("const", ROWS, 64, kind="const"))        # variance 0: y = beta, rstd = eps^-1/2
    add(Case("inflight4", 4099, 64))                  # rows >= 4096: four rows per lane group in flight (NV = 1)
    add(Case("inflight2", 4099, 320))                 # two rows (NV = 2)
    add(Case("ilp", 8197, 64, dtypes=(F32,)))         # the backward's row pairing from 8192 rows
    add(Case("ilpldx4", 8197, 64, ldx=68, dtypes=HALF))   # ... in 16-bit storage, where aligned rows of 64 are the 8-wide kernel's
    add(Case("g3p8", ROWS, 64, groups=3, pgap=8))     # pstride = C + 8: the 8-wide kernels' alignment holds
    add(Case("g3p4", ROWS, 64, groups=3, pgap=4))     # pstride = C + 4: it does not
    add(Case("g2w1280", ROWS, 1280, groups=2))        # the wide split with groups
    add(Case("g2w2048", ROWS, 2048, groups=2))
    add(Case("g2c36", ROWS, 36, groups=2))
    add(Case("w512", ROWS, 512))                      # the widest row of the 8-wide kernels
    add(Case("gelu64", ROWS, 64, act=ACT_GELU, groups=2))
    add(Case("gelu1280", ROWS, 1280, act=ACT_GELU, groups=2))
    add(Case("gelu36", ROWS, 36, act=ACT_GELU, groups=2))
    add(Case("ldx4", ROWS, 64, ldx=68, dtypes=HALF))  # ldx = C + 4: 16-bit rows off the 16-byte grid -> the 4-wide kernels
    for p in (2, 4):
        for C in (64, 96):
            add(Case(f"ps{p}c{C}", 2 * 3 * p * 5 * p, C, ps=(2, 3, 5, p)))
    # the forward's 8-wide kernel (16-bit, rows >= 65536): C = 64 in both types, the wider rows in one type each
    add(Case("big64", BIG, 64, dtypes=HALF))
    add(Case("big128", BIG, 128, dtypes=(BF16,)))
    add(Case("big256", BIG, 256, dtypes=(F16,)))
    add(Case("big512", BIG, 512, dtypes=(BF16,)))
    add(Case("big64m1", 65535, 64, dtypes=HALF))      # one row short of the threshold: the 4-wide kernel on the same problem
    add(Case("big64ldx4", BIG, 64, ldx=68, dtypes=HALF))   # misaligned rows: the 4-wide kernel again
    add(Case("big64g2", 65537, 64, groups=2, dtypes=(BF16,)))    # groups on the 8-wide forward (with the interleaved statistics)
    # the backward's 8-wide kernel with 2 and 4 rows in flight (1: the 37-row cases), at the smallest row counts that get there
    for i, C in enumerate(V8_CS):
        for rpt in (2, 4):
            add(Case(f"v8c{C}r{rpt}", v8_rows(C, rpt), C, dtypes=(HALF[(i + rpt // 4) % 2],)))
    return t


def v8_rows(C, rpt):
    """The smallest 2^k + 5 rows at which a tc_layernorm_bwd launch with parameter gradients keeps rpt rows in flight per lane group."""
    for k in range(8, 21):
        rows = 2 ** k + 5
        if v8_rows_in_flight(rows, C, bwd_nblk(rows, C, True, False)) == rpt:
            return rows
    raise AssertionError((C, rpt))


CASES = _cases()
SMALL = [k for k, c in CASES.items() if c.rows * c.groups <= 5000]


def case_dtypes(c):
    return c.dtypes or ALL


def all_operands(names=None):
    for k in (names or CASES):
        for dt in case_dtypes(CASES[k]):
            yield CASES[k].on(dt)

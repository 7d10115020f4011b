"""tests/ln_ref.py proves itself on the host: the float64 LayerNorm model agrees with torch.nn.functional.layer_norm (+ gelu) and its autograd in
float64; the derived error bounds hold for honest fp32 arithmetic in three summation orders, with and without fused multiply-add, at every case
of the table tests/test_layernorm_abi_gpu.py runs; each of a list of plausible kernel mistakes, applied to the same fp32 emulation, breaks a
bound or an exactness assertion on a named case (so the bounds cannot hide it); and the premises of every case hold (grids, exact sums, the
references that are compared bit for bit are fp32 values) -- a premise that fails shows up here, not on the device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ln_ref as R

f32, f64 = np.float32, np.float64
ORDERS = ("seq", "lane", "rev")
VARIANTS = [(o, fma) for o in ORDERS for fma in (False, True)]
LARGE = [k for k in R.CASES if k not in R.SMALL]


# ---------------------------------------------------------------------------------------------------------------- the model against torch
def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def torch_ln(x, g, b, eps, act):
    y = F.layer_norm(x, x.shape[-1:], g, b, eps)
    return F.gelu(y) if act == R.ACT_GELU else y


@pytest.mark.parametrize("act", [R.ACT_NONE, R.ACT_GELU])
@pytest.mark.parametrize("groups,rows,C", [(1, 37, 64), (3, 11, 36), (2, 5, 1280)])
def test_model_against_torch_float64(groups, rows, C, act):
    """ln_ref.fwd / ln_ref.bwd (groups, dres, both activations) == F.layer_norm (+ F.gelu) and its autograd in float64, to 1e-12 relative."""
    gen = torch.Generator().manual_seed(groups * 1000 + C + act)
    x = torch.randn(groups, rows, C, generator=gen, dtype=torch.float64) * 3 + 1
    dy, res = torch.randn(groups, rows, C, generator=gen, dtype=torch.float64), torch.randn(groups, rows, C, generator=gen, dtype=torch.float64)
    g, b = torch.randn(groups, C, generator=gen, dtype=torch.float64), torch.randn(groups, C, generator=gen, dtype=torch.float64)
    eps = 1e-5
    y, mean, rstd = R.fwd(x, g, b, eps, act)
    dx, dg, db = R.bwd(dy, x, g, b, eps, act, res)
    for i in range(groups):
        xi, gi, bi = x[i].clone().requires_grad_(), g[i].clone().requires_grad_(), b[i].clone().requires_grad_()
        yi = torch_ln(xi, gi, bi, eps, act)
        yi.backward(dy[i])
        assert rel(y[i], yi.detach()) < 1e-12
        assert rel(mean[i], x[i].mean(-1)) < 1e-12 and rel(rstd[i], (x[i].var(-1, unbiased=False) + eps).rsqrt()) < 1e-12
        assert rel(dx[i], xi.grad + res[i]) < 1e-12 and rel(dg[i], gi.grad) < 1e-12 and rel(db[i], bi.grad) < 1e-12
    # one group through the 2-D form
    y2, _, _ = R.fwd(x[0], g[0], b[0], eps, act)
    assert torch.equal(y2, y[0])


@pytest.mark.parametrize("p,C", [(2, 8), (4, 12)])
def test_pixel_shuffle_map_against_rearrange(p, C):
    """ps_gather / ps_scatter / bwd(ps=...) against the explicit rearrange 'b h w (p1 p2 c) -> b (h p1) (w p2) c' and autograd through it."""
    B, H, W = 2, 3, 5
    gen = torch.Generator().manual_seed(p)
    x2 = torch.randn(B * H * W, p * p * C, generator=gen, dtype=torch.float64)
    g, b = torch.randn(C, generator=gen, dtype=torch.float64), torch.randn(C, generator=gen, dtype=torch.float64)
    dy = torch.randn(B * H * p * W * p, C, generator=gen, dtype=torch.float64)
    shuffle = lambda t: t.reshape(B, H, W, p, p, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H * p * W * p, C)  # noqa: E731
    assert torch.equal(R.ps_gather(x2, B, H, W, p, C), shuffle(x2))
    assert torch.equal(R.ps_scatter(shuffle(x2), B, H, W, p, C), x2)
    assert not torch.equal(R.ps_gather(x2, B, H, W, p, C, swap=True), shuffle(x2))
    xi, gi, bi = x2.clone().requires_grad_(), g.clone().requires_grad_(), b.clone().requires_grad_()
    yi = torch_ln(shuffle(xi), gi, bi, 1e-5, R.ACT_NONE)
    yi.backward(dy)
    y, _, _ = R.fwd(R.ps_gather(x2, B, H, W, p, C), g, b, 1e-5)
    dx, dg, db = R.bwd(dy, x2, g, b, 1e-5, ps=(B, H, W, p))
    assert rel(y, yi.detach()) < 1e-12 and rel(dx, xi.grad) < 1e-12 and rel(dg, gi.grad) < 1e-12 and rel(db, bi.grad) < 1e-12


def test_fold_model_and_geometry():
    """ln_ref.fold is the plain sum over the parked rows; the restated dispatcher geometry on hand-checked values."""
    part = torch.arange(2 * 3 * 2 * 4, dtype=torch.float64).reshape(2, 3, 2, 4)
    dg, db = R.fold(part.reshape(-1), 3, 4, 2)
    assert torch.equal(dg, part[:, :, 0].sum(1)) and torch.equal(db, part[:, :, 1].sum(1))
    assert [R.lane_group(C) for C in R.WIDTHS] == [(16, 1), (32, 1), (64, 1), (64, 2), (64, 4), (64, 5), (64, 8)]
    assert [R.lane_group(C) for C in R.PARTIAL] == [(16, 1), (16, 1), (64, 1)]
    assert R.bwd_nblk(37, 64) == 3 and R.bwd_nblk(37, 512) == 10 and R.bwd_nblk(8197, 64) == 257        # (the row pairing halves the count)
    assert R.bwd_nblk(65541, 64) == 1024 and R.bwd_nblk(65541, 64, deferred=True) == 1025 and R.bwd_nblk(10 ** 6, 64, False) == 8192
    assert R.v8_rows_in_flight(65541, 64, 1024) == 2 and R.v8_rows_in_flight(37, 64, 3) == 1 and R.v8_rows_in_flight(16389, 512, 1024) == 4


# ---------------------------------------------------------------------------------------------------------------- fp32 arithmetic, emulated
def rsum(a, b, axis, order, fma):
    """sum of a * b (b None: of a) along `axis` in fp32.  Products are exact in float64 (24 + 24 bits); fma: they enter the running sum unrounded
    (the sum itself rounded once from float64 -- a fused multiply-add up to a double rounding of relative 2^-53).
    seq / rev: one running sum from either end; lane: four consecutive terms in turn, then a pairwise tree (a lane's pieces, then the shuffles)."""
    t = np.moveaxis(a, axis, 0).astype(f64)
    fused = fma and b is not None
    if b is not None:
        t = t * np.moveaxis(np.broadcast_to(b, a.shape), axis, 0).astype(f64)
    if not fused:
        t = t.astype(f32)
    n = t.shape[0]
    if order in ("seq", "rev"):
        if order == "rev":
            t = t[::-1]
        if not fused:
            return np.add.accumulate(t, axis=0, dtype=f32)[-1]
        acc = t[0].astype(f32)
        for i in range(1, n):
            acc = (acc.astype(f64) + t[i]).astype(f32)
        return acc
    pad = (-n) % 4
    if pad:
        t = np.concatenate([t, np.zeros((pad,) + t.shape[1:], t.dtype)])
    t = t.reshape((t.shape[0] // 4, 4) + t.shape[1:])
    acc = t[:, 0].astype(f32)
    for k in range(1, 4):
        acc = (acc.astype(f64) + t[:, k].astype(f64)).astype(f32)
    while acc.shape[0] > 1:
        if acc.shape[0] & 1:
            acc = np.concatenate([acc, np.zeros((1,) + acc.shape[1:], f32)])
        acc = acc[0::2] + acc[1::2]
    return acc[0]


def muladd(a, b, c, fma):
    """fl(a b + c), or fl(fl(a b) + c)."""
    if fma:
        return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    return a * b + c


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(f64))


def emu_fwd(x, g, b, eps, act, order, fma, mut=None):
    """The forward in fp32: x [G, R, C], g / b [G, 1, C] float32 arrays -> (y, mean, rstd).  mut: one of the mistakes of MUTATIONS."""
    C = x.shape[-1]
    invC, eps = f32(1) / f32(C), f32(eps)
    if mut == "gamma0":
        g, b = g[:1], b[:1]
    mu = (rsum(x, None, -1, order, fma) * invC)[..., None]
    d = x - mu
    if mut == "onepass":
        var = rsum(x, x, -1, order, fma)[..., None] * invC - mu * mu
    else:
        var = rsum(d, d, -1, order, fma)[..., None] * (f32(1) / f32(C - 1) if mut == "cminus1" else invC)
    if mut == "noeps":
        rs = (1.0 / np.sqrt(var.astype(f64))).astype(f32)
    elif mut == "epsout":
        rs = (1.0 / (np.sqrt(var.astype(f64)) + eps)).astype(f32)
    else:
        rs = (1.0 / np.sqrt((var + eps).astype(f64))).astype(f32)            # a correctly rounded rsqrtf
    y = muladd(d * rs, g, b, fma)
    if act == R.ACT_GELU:
        y64 = _t(y)
        y = (y64 * 0.5 * (1.0 + torch.erf(y64 / 2.0 ** 0.5))).numpy().astype(f32)
    return y, mu[..., 0], rs[..., 0]


def emu_bwd(dy, x, g, b, mean, rstd, act, res, dg0, db0, order, fma, mut=None):
    """The backward in fp32 from the saved statistics -> (dx, dgamma, dbeta) (dgamma / dbeta added to dg0 / db0 [G, C])."""
    C = x.shape[-1]
    invC = f32(1) / f32(C)
    if mut == "gamma0":
        g, b = g[:1], b[:1]
    mu, rs = mean[..., None], rstd[..., None]
    xh = (x - mu) * rs
    if act == R.ACT_GELU:
        z = _t(muladd(xh, g, np.broadcast_to(b, xh.shape), fma))
        dz = dy * R.gelu_grad(z).numpy().astype(f32)
    else:
        dz = dy
    pz, px = dz, xh
    if mut == "droprow":
        pz, px = dz[:, :-1], xh[:, :-1]
    elif mut == "doublerow":
        pz, px = np.concatenate([dz, dz[:, -1:]], 1), np.concatenate([xh, xh[:, -1:]], 1)
    dbeta = db0 + rsum(pz, None, 1, order, fma)
    dgamma = dg0 + rsum(pz, px, 1, order, fma)
    a = dz * g
    s1 = (rsum(a, None, -1, order, fma) * invC)[..., None]
    s2 = (rsum(a, xh, -1, order, fma) * invC)[..., None]
    w = muladd(-xh, np.broadcast_to(s2, xh.shape), a - s1, fma)
    zero = np.zeros_like(w)
    r = zero if res is None or mut == "nodres" else (res + res if mut == "dres2" else res)
    dx = muladd(np.broadcast_to(rs, w.shape), w, r, fma)
    if mut == "lastdx":
        dx = dx.copy()
        dx[-1, -1] = f32(R.SENT)                                              # the output buffer's sentinel stays
    return dx, dgamma, dbeta


def arrays(o, res=False):
    c = o.c
    n = lambda t: t.float().numpy()  # noqa: E731
    m, r = o.stats32()
    G = c.groups
    return dict(x=n(o.x3()), dy=n(o.dy3()), g=n(o.g2())[:, None], b=n(o.b2())[:, None], res=n(o.res3()) if res else None,
                mean=m.numpy().reshape(G, -1), rstd=r.numpy().reshape(G, -1), dg0=n(o.dg0().blocks()), db0=n(o.db0().blocks()))


def stored(a, dtype):
    """An fp32 result as the kernel leaves it in the storage type."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def worst(got, want, bound, dtype):
    return float(R.excess(got, want, bound, dtype).max())


def check_fwd(o, order, fma, mut=None):
    """Largest excess over the bounds (and the exactness assertion of the mean) of the emulated forward of operands o: <= 0 when all hold."""
    c, A = o.c, arrays(o)
    x = A["x"]
    if mut == "swap":
        x = R.ps_gather(o.x.logical().double(), *c.ps, c.C, swap=True)[None].float().numpy()
    y, mean, rstd = emu_fwd(x, A["g"], A["b"], c.eps, c.act, order, fma, mut)
    wy, wm, wr = o.ref_fwd()
    by, bm, br = o.bound_fwd()
    e = max(worst(stored(y.reshape(-1, c.C), o.dtype), wy, by, o.dtype), worst(stored(mean.reshape(-1), torch.float32), wm, bm, torch.float32),
            worst(stored(rstd.reshape(-1), torch.float32), wr, br, torch.float32))
    if c.C & (c.C - 1) == 0 and not torch.equal(stored(mean.reshape(-1), torch.float32).double(), wm):
        e = float("inf")                                                       # the mean of a power-of-two row is exact
    return e


def check_bwd(o, order, fma, mut=None, res=False):
    c, A = o.c, arrays(o, res)
    x = A["x"]
    if mut == "swap":
        x = R.ps_gather(o.x.logical().double(), *c.ps, c.C, swap=True)[None].float().numpy()
    dx, dg, db = emu_bwd(A["dy"], x, A["g"], A["b"], A["mean"], A["rstd"], c.act, A["res"], A["dg0"], A["db0"], order, fma, mut)
    dg0, db0 = o.dg0(), o.db0()
    wdx, wdg, wdb = o.ref_bwd(res)
    bdx, bdg, bdb = o.bound_bwd(res, dg0, db0)
    wdg, wdb = wdg.reshape(c.groups, c.C) + dg0.blocks().double(), wdb.reshape(c.groups, c.C) + db0.blocks().double()
    dxs = stored(dx[0] if c.ps is not None else dx, o.dtype)
    if c.ps is not None:
        dxs = R.ps_scatter(dxs, *c.ps, c.C)
    e = max(worst(dxs.reshape(wdx.shape), wdx, bdx, o.dtype), worst(stored(dg, torch.float32), wdg, bdg.reshape(c.groups, c.C), torch.float32),
            worst(stored(db, torch.float32), wdb, bdb.reshape(c.groups, c.C), torch.float32))
    if c.act == R.ACT_NONE and not torch.equal(stored(db, torch.float32).double(), wdb):
        e = float("inf")                                                       # dbeta without activation is exact
    return e


# ---------------------------------------------------------------------------------------------------------------- premises, bounds, mutations
@pytest.mark.parametrize("name", list(R.CASES))
def test_premises_of_every_case(name):
    """Grids, exactly representable sums, 2^24 exactness of dbeta, `the reference is an fp32 value` where exactness is claimed -- for every case and
    storage type of the device table; the workspace arithmetic of the cases that use one."""
    c = R.CASES[name]
    for dt in R.case_dtypes(c):
        assert c.on(dt).premise()
    for k in c.ld.values():
        assert k % 4 == 0
    nb = R.bwd_nblk(c.rows, c.C)
    assert R.scratch_floats(c.C, c.groups, nb) <= 4096 + c.groups * 1024 * 2 * c.C      # tc_layernorm_bwd_scratch_floats covers every launch
    c._built.clear()


@pytest.mark.parametrize("name", R.SMALL)
def test_bounds_hold_for_honest_fp32(name):
    """Sequential, lane-wise pairwise and reversed sums, each with and without fused multiply-add, forward and backward (with and without dres): every
    output of every variant stays inside the bounds, in every storage type of the case."""
    c = R.CASES[name]
    for dt in R.case_dtypes(c):
        o = c.on(dt)
        for order, fma in VARIANTS:
            assert check_fwd(o, order, fma) <= 0, (o.tag, "fwd", order, fma)
            assert check_bwd(o, order, fma) <= 0, (o.tag, "bwd", order, fma)
            if c.ps is None:
                assert check_bwd(o, order, fma, res=True) <= 0, (o.tag, "bwd + dres", order, fma)
    c._built.clear()


@pytest.mark.parametrize("name", LARGE)
def test_bounds_hold_for_honest_fp32_large_rows(name):
    """The many-row cases (the device runs the forward of the big* cases and the backward of big64 and the v8* cases): the two variants furthest apart -- sequential unfused and
    lane-wise fused -- in the first storage type of the case."""
    c = R.CASES[name]
    o = c.on(R.case_dtypes(c)[0])
    for order, fma in (("seq", False), ("lane", True)):
        assert check_fwd(o, order, fma) <= 0, (o.tag, "fwd", order, fma)
        if name == "big64" or not name.startswith("big"):
            assert check_bwd(o, order, fma) <= 0, (o.tag, "bwd", order, fma)
    c._built.clear()


# mistake -> (the case that catches it, direction, with dres)
MUTATIONS = {
    "onepass": ("offset", "fwd", False),          # variance by E[x^2] - mean^2
    "cminus1": ("w64", "fwd", False),             # variance divided by C - 1
    "noeps": ("eps025", "fwd", False),            # eps omitted
    "epsout": ("eps025", "fwd", False),           # eps added outside the square root
    "droprow": ("w64", "bwd", False),             # one row dropped from dgamma / dbeta
    "doublerow": ("w64", "bwd", False),           # one row counted twice
    "lastdx": ("w64", "bwd", False),              # the last row's dx left unwritten
    "gamma0": ("g3p8", "fwd", False),             # gamma of group 0 used for group 1
    "swap": ("ps2c64", "fwd", False),             # chunk index p2 p + p1
    "nodres": ("w64", "bwd", True),               # dres not added
    "dres2": ("w64", "bwd", True),                # dres added twice
}


@pytest.mark.parametrize("dtype", R.ALL, ids=lambda d: str(d).split(".")[-1])
@pytest.mark.parametrize("mut", list(MUTATIONS))
def test_bounds_catch_the_mistake(mut, dtype):
    """Each mistake, applied to the emulation, violates a bound or an exactness assertion on its named case in every storage type and every variant
    -- while the unmutated emulation of the same case passes (test_bounds_hold_for_honest_fp32)."""
    name, direction, res = MUTATIONS[mut]
    o = R.CASES[name].on(dtype)
    for order, fma in VARIANTS:
        e = check_fwd(o, order, fma, mut) if direction == "fwd" else check_bwd(o, order, fma, mut, res)
        assert e > 0, (mut, name, order, fma)
        ok = check_fwd(o, order, fma) if direction == "fwd" else check_bwd(o, order, fma, None, res)
        assert ok <= 0


def test_mistakes_in_the_other_direction_too():
    """The mistakes that live in both directions are caught in the backward as well: the group's gamma and the chunk index."""
    for mut, name in (("gamma0", "g3p8"), ("swap", "ps2c64"), ("gamma0", "gelu36")):
        for dt in R.ALL:
            assert check_bwd(R.CASES[name].on(dt), "lane", True, mut) > 0, (mut, name, dt)


def test_constant_rows():
    """Variance 0: y = beta, rstd = eps^-1/2, and the bounds stay finite and small."""
    o = R.CASES["const"].on(torch.float32)
    y, _, rstd = o.ref_fwd()
    assert torch.equal(y, o.b2().expand(37, 64)) and float((rstd - o.c.eps ** -0.5).abs().max()) < 1e-9
    by, bm, br = o.bound_fwd()
    assert float(by.max()) < 1e-4 and float(bm.max()) < 1e-6 and float((br / rstd).max()) < 1e-5


def test_storage_spacing():
    for dt, w, s in ((torch.bfloat16, 1.0, 2.0 ** -7), (torch.bfloat16, 1.99, 2.0 ** -7), (torch.float16, 3.0, 2.0 ** -9), (torch.float16, 0.0, 2.0 ** -24)):
        assert float(R.ulp_of(torch.tensor([w], dtype=torch.float64), dt)) == s
    assert R.max_offset(torch.bfloat16) == 125.5 and R.max_offset(torch.float16) == 1021.5

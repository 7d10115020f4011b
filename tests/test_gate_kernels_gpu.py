"""The gate, pooling and aggregate kernels -- all of csrc/cbam.hip and the arithmetic half of csrc/elementwise.hip -- one C-ABI entry point
at a time on raw pointers, in float32, bfloat16 and float16, against the float64 host references of tests/gate_ref.py.

Exactness rule.  Inputs lie on a coarse grid: multiples of 1/2 with |v| <= 2; gates, att and the stored sigmoid in {0, 1/4, 1/2, 3/4, 1};
scalars are powers of two (alpha = 0.25, gamma = 0.5); pooled lengths are powers of two in the exact cases.  Every fp32 product and every
partial sum inside a kernel is then exact whatever the summation order, and the only rounding is the round-to-nearest-even store: the
assertion is got == want64.to(dtype), element for element, after the test has asserted its own premise (want64 is a float32 value; for each
reduction sum|term| / quantum < 2^24).  fp32 side outputs (att2, dw, db, dgamma) and idx are compared exactly too; dw, db and dgamma are +=
targets and start from a chosen grid value.

Four things cannot be made exact and are held to the float64 reference by derived bounds:
  * a mean over a length that is not a power of two: |got - want| <= 3 * 2^-24 |want| (one rounding each for 1/N, the product and one
    more operation), plus half a storage spacing at want (x 1.001) in 16-bit storage.  Where a backward kernel adds terms, the inputs of these
    cases are non-negative, so that each rounding is relative to a partial sum no larger than the result;
  * tc_sa_conv_fwd's sigmoid of an exact pre-activation: 2e-6 + 1e-5 |want| (test_ops_gpu.test_cbam_pieces), plus half a spacing;
  * tc_cam_att_fwd's softmax of exact energies: 2e-5 + 2e-5 |want| (test_ops_gpu.test_cam_module_and_gelu); |x| <= 1/2 keeps the energy
    differences below 10;
  * tc_gelu_bwd: 5e-6 |dy| (the same test), plus half a spacing, on every finite storage value of [-8, 8].

Every leading dimension is larger than the column count and differs between operands; output buffers have spare rows and columns and are
pre-filled with a sentinel (or, where the op accumulates, with grid values); the WHOLE buffer is compared."""
import zlib

import pytest
import torch

import gate_ref as R

pytestmark = pytest.mark.gpu

from transception_amd._lib import TC_BF16, TC_F16, TC_F32, TcError, lib  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TC = {torch.float32: TC_F32, torch.bfloat16: TC_BF16, torch.float16: TC_F16}
SENT = -96.0                       # exact in every storage type, never a result of the grids below
ALPHA, GAMMA = 0.25, 0.5
SHAPES = [(2, 1, 4), (2, 8, 24), (1, 64, 72), (2, 8, 128), (3, 64, 4)]      # (B, N, C): every channel edge, every power-of-two token edge
MEANS = [(2, 37, 24), (1, 37, 72)]                                         # N = 37: the bounded means
ACC = pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
EACH_DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])


# ---------------------------------------------------------------------------------------------------------------- inputs
def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def halves(tag, shape, dtype, lim=4):
    """Seeded multiples of 1/2 with |v| <= lim / 2 (no -0.0)."""
    return (torch.randint(-lim, lim + 1, shape, generator=_gen("h/" + tag)).float() / 2).to(dtype)


def nonneg(tag, shape, dtype, lim=4):
    return (torch.randint(0, lim + 1, shape, generator=_gen("n/" + tag)).float() / 2).to(dtype)


def quarters(tag, shape, dtype):
    """Seeded values of {0, 1/4, 1/2, 3/4, 1}."""
    return (torch.randint(0, 5, shape, generator=_gen("q/" + tag)).float() / 4).to(dtype)


def vals(tag, shape, dtype):
    """Arbitrary finite values of the storage type, with -0.0 and +-the largest finite value among them."""
    t = (torch.randn(shape, generator=_gen("v/" + tag)) * 3).to(dtype)
    f = t.view(-1)
    for i, v in enumerate((-0.0, torch.finfo(dtype).max, -torch.finfo(dtype).max)[:f.numel()]):
        f[(i * 7) % f.numel()] = v
    return t


def sent(shape, dtype):
    return torch.full(shape, SENT, dtype=dtype)


def outbuf(tag, rows, cols, dtype, acc=0, spare=2, fn=halves):
    """The output buffer before the call: the sentinel, or grid values where the op adds to what is there."""
    return fn(tag, (rows + spare, cols), dtype) if acc else sent((rows + spare, cols), dtype)


def f32buf(n, first):
    """An fp32 += target of n elements starting from grid values, with two sentinel elements behind it."""
    t = sent((n + 2,), torch.float32)
    t[:n] = first
    return t


def dev(t):
    return t.to(DEV)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


def sync():
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- comparisons
def premise(sum_abs, quantum):
    """Every partial sum of the reduction is a multiple of `quantum` below 2^24 quanta, so fp32 adds it exactly in any order."""
    assert float(torch.as_tensor(sum_abs).max()) / quantum < 2.0 ** 24, "the test's own inputs must keep the reduction exact"


def exact(got, want64, what=""):
    """got == the float64 reference cast to got's type; the reference itself must be a float32 value (nothing rounds before the store)."""
    assert torch.equal(want64.float().double(), want64), "the test's own inputs must make the fp32 result exact: " + what
    g, want = got.detach().cpu(), want64.to(got.dtype)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not torch.equal(g, want):
        bad = (g != want).nonzero()
        i = tuple(bad[0].tolist())
        pytest.fail(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at {i}: got {float(g[i])}, want {float(want[i])}")


def same_bits(got, want, what=""):
    g = got.detach().cpu().contiguous()
    assert g.dtype == want.dtype and g.shape == want.shape, what
    iv = torch.int32 if g.dtype == torch.float32 else torch.int16
    assert torch.equal(g.view(iv), want.contiguous().view(iv)), what


def spacing(v, dtype):
    """Storage spacing at v (subnormals included), as in test_ops_gpu.test_gelu_16bit_polynomial_against_erf."""
    mant, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** emin))) - mant)


def half_spacing(want64, dtype):
    return 0.0 if dtype == torch.float32 else 0.5 * spacing(want64, dtype) * 1.001


def within(got, want64, tol, what):
    g = got.detach().cpu().double()
    assert g.shape == want64.shape, (what, g.shape, want64.shape)
    err = (g - want64).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    ratio = torch.where(err > 0, err / tol, torch.zeros_like(err))              # inf where an error meets a zero bound
    k = int(ratio.argmax())
    print(f"\n[gate] {what} {str(got.dtype).split('.')[-1]}: largest error / bound {float(ratio.view(-1)[k]):.3f} (error {float(err.view(-1)[k]):.3e}, "
          f"bound {float(tol.reshape(-1)[k]):.3e}, want {float(want64.reshape(-1)[k]):.6g}); largest error {float(err.max()):.3e}")
    assert bool((err <= tol).all()), (what, float(err.view(-1)[k]), float(tol.reshape(-1)[k]), float(want64.reshape(-1)[k]))


def mean_close(got, want64, what):
    """The bounded mean: 3 * 2^-24 |want| for the fp32 arithmetic, plus half a storage spacing in 16-bit."""
    within(got, want64, 3 * 2.0 ** -24 * want64.abs() + half_spacing(want64, got.dtype), what)


def check(got, want64, is_exact, what):
    exact(got, want64, what) if is_exact else mean_close(got, want64, what)


def pow2(n):
    return n & (n - 1) == 0


# ---------------------------------------------------------------------------------------------------------------- fma3 / add / pointwise
@EACH_DTYPE
@ACC
@pytest.mark.parametrize("shape", SHAPES + MEANS, ids=str)
def test_fma3_and_add(shape, acc, dtype):
    """tc_fma3_fwd, tc_fma3_bwd (db written and accumulated) and tc_add, four different row strides."""
    B, N, C = shape
    rows, tc, L, tag = B * N, TC[dtype], lib(), f"fma{shape}"
    a, b, c = halves(tag + "a", (rows, C + 4), dtype), halves(tag + "b", (rows, C + 8), dtype), halves(tag + "c", (rows, C + 12), dtype)
    o0 = outbuf(tag + "o", rows, C + 16, dtype)
    ad, bd, cd, od = dev(a), dev(b), dev(c), dev(o0)
    L.tc_fma3_fwd(ptr(ad), C + 4, ptr(bd), C + 8, ptr(cd), C + 12, ptr(od), C + 16, rows, C, ALPHA, tc, stream())
    sync()
    exact(od, R.fma3_fwd_ref(a[:, :C], b[:, :C], c[:, :C], ALPHA, o0), "fma3 out")
    y0 = outbuf(tag + "y", rows, C + 16, dtype)
    yd = dev(y0)
    L.tc_add(ptr(ad), C + 4, ptr(cd), C + 12, ptr(yd), C + 16, rows, C, tc, stream())
    sync()
    exact(yd, R.add_ref(a[:, :C], c[:, :C], y0), "add")
    d = halves(tag + "d", (rows, C + 16), dtype)
    da0, db0, dc0 = outbuf(tag + "da", rows, C + 4, dtype), outbuf(tag + "db", rows, C + 8, dtype, acc, 1), outbuf(tag + "dc", rows, C + 12, dtype, 0, 3)
    dd, dad, dbd, dcd = dev(d), dev(da0), dev(db0), dev(dc0)
    L.tc_fma3_bwd(ptr(dd), C + 16, ptr(bd), C + 8, ptr(cd), C + 12, ptr(dad), C + 4, ptr(dbd), C + 8, acc, ptr(dcd), C + 12, rows, C, ALPHA, tc, stream())
    sync()
    wa, wb, wc = R.fma3_bwd_ref(d[:, :C], b[:, :C], c[:, :C], ALPHA, da0, db0, dc0, bool(acc))
    exact(dad, wa, "da")
    exact(dbd, wb, "db")
    exact(dcd, wc, "dc")
    same_bits(bd, b, "b is only read")


@EACH_DTYPE
@pytest.mark.parametrize("n", [1, 5, 1037])
def test_sigmoid_bwd_and_relu(n, dtype):
    """tc_sigmoid_bwd on a stored sigmoid in quarters; tc_relu_fwd on inputs with +-0.0 and tc_relu_bwd with y == 0 among its rows (values
    compared); the three elements behind the n keep the sentinel."""
    tc, L, tag = TC[dtype], lib(), f"pw{n}"
    dy, s = halves(tag + "dy", (n,), dtype), quarters(tag + "s", (n,), dtype)
    z0 = sent((n + 3,), dtype)
    dyd, sd, zd = dev(dy), dev(s), dev(z0)
    L.tc_sigmoid_bwd(ptr(dyd), ptr(sd), ptr(zd), n, tc, stream())
    sync()
    exact(zd, R.sigmoid_bwd_ref(dy, s, z0), "sigmoid'")
    x = halves(tag + "x", (n,), dtype)
    x[0] = -0.0
    if n > 4:
        x[3], x[4] = 0.0, -0.5
    xd, yd = dev(x), dev(z0)
    L.tc_relu_fwd(ptr(xd), ptr(yd), n, tc, stream())
    sync()
    want = R.relu_fwd_ref(x, z0)
    exact(yd, want, "relu")
    assert bool((yd.cpu()[:n] >= 0).all()) and (n < 5 or float(yd[3]) == 0.0)
    y = want[:n].to(dtype)                                                  # zeros where x <= 0
    assert bool((y == 0).any()) or n == 1
    dzd = dev(z0)
    y_d = dev(y)
    L.tc_relu_bwd(ptr(dyd), ptr(y_d), ptr(dzd), n, tc, stream())
    sync()
    exact(dzd, R.relu_bwd_ref(dy, y, z0), "relu'")
    ym = y.clone()
    ym[0] = -0.0                                                            # y == -0.0 passes nothing either
    dzd = dev(z0)
    ym_d = dev(ym)
    L.tc_relu_bwd(ptr(dyd), ptr(ym_d), ptr(dzd), n, tc, stream())
    sync()
    exact(dzd, R.relu_bwd_ref(dy, ym, z0), "relu' at -0.0")


# ---------------------------------------------------------------------------------------------------------------- SE_Block
@EACH_DTYPE
@ACC
@pytest.mark.parametrize("shape", SHAPES + MEANS, ids=str)
def test_chan_pool(shape, acc, dtype):
    """tc_chan_pool_fwd and tc_chan_pool_bwd: exact at N in {1, 8, 64}, the bounded mean at N = 37 (non-negative gradients there)."""
    B, N, C = shape
    rows, tc, L, tag, ex = B * N, TC[dtype], lib(), f"cp{shape}", pow2(N)
    fn = halves if ex else nonneg
    x, p0 = halves(tag + "x", (rows, C + 4), dtype), outbuf(tag + "p", B, C, dtype)
    premise(x[:, :C].double().abs().view(B, N, C).sum(1), 0.5)
    xd, pd = dev(x), dev(p0)
    L.tc_chan_pool_fwd(ptr(xd), C + 4, ptr(pd), B, N, C, tc, stream())
    sync()
    check(pd, R.chan_pool_fwd_ref(x[:, :C], B, N, p0), ex, "chan_pool mean")
    dp, dx0 = fn(tag + "dp", (B, C), dtype), outbuf(tag + "dx", rows, C + 8, dtype, acc, fn=fn)
    dpd, dxd = dev(dp), dev(dx0)
    L.tc_chan_pool_bwd(ptr(dpd), ptr(dxd), C + 8, B, N, C, acc, tc, stream())
    sync()
    check(dxd, R.chan_pool_bwd_ref(dp, B, N, dx0, bool(acc)), ex, "chan_pool dx")


@EACH_DTYPE
@ACC
@pytest.mark.parametrize("shape", SHAPES + MEANS, ids=str)
def test_chan_gate(shape, acc, dtype):
    """tc_chan_gate_fwd and tc_chan_gate_bwd (dx written / accumulated, dgate summed over the image's rows): exact at every N."""
    B, N, C = shape
    rows, tc, L, tag = B * N, TC[dtype], lib(), f"cg{shape}"
    x, g, y0 = halves(tag + "x", (rows, C + 4), dtype), quarters(tag + "g", (B, C), dtype), outbuf(tag + "y", rows, C + 8, dtype)
    xd, gd, yd = dev(x), dev(g), dev(y0)
    L.tc_chan_gate_fwd(ptr(xd), C + 4, ptr(gd), ptr(yd), C + 8, B, N, C, tc, stream())
    sync()
    exact(yd, R.chan_gate_fwd_ref(x[:, :C], g, B, N, y0), "gated")
    dy, dx0, dg0 = halves(tag + "dy", (rows, C + 12), dtype), outbuf(tag + "dx", rows, C + 8, dtype, acc), outbuf(tag + "dg", B, C, dtype, 0, 1)
    premise((dy[:, :C].double() * x[:, :C].double()).abs().view(B, N, C).sum(1), 0.25)
    dyd, dxd, dgd = dev(dy), dev(dx0), dev(dg0)
    L.tc_chan_gate_bwd(ptr(dyd), C + 12, ptr(xd), C + 4, ptr(gd), ptr(dxd), C + 8, acc, ptr(dgd), B, N, C, tc, stream())
    sync()
    wx, wg = R.chan_gate_bwd_ref(dy[:, :C], x[:, :C], g, B, N, dx0, dg0, bool(acc))
    exact(dxd, wx, "dx")
    exact(dgd, wg, "dgate")


# ---------------------------------------------------------------------------------------------------------------- CoordAtt
COORD = [(2, 4, 8, 8), (1, 8, 2, 24), (2, 5, 9, 8)]                        # (B, H, W, C): H != W; 5 x 9 is the bounded mean


@EACH_DTYPE
@pytest.mark.parametrize("case", COORD, ids=str)
def test_coord_pool(case, dtype):
    """tc_coord_pool_fwd / _bwd on non-square maps: rows (b, h) average over W and scale back by 1 / W, rows (b, w) by 1 / H.  5 x 9 is
    held to the bounded mean, its backward with non-negative gradients into an empty buffer; the exact maps also accumulate."""
    B, H, W, C = case
    rows, tc, L, tag, ex = B * H * W, TC[dtype], lib(), f"cop{case}", pow2(H) and pow2(W)
    fn = halves if ex else nonneg
    x, p0 = halves(tag + "x", (rows, C), dtype), outbuf(tag + "p", B * (H + W), C, dtype)
    xd, pd = dev(x), dev(p0)
    L.tc_coord_pool_fwd(ptr(xd), ptr(pd), B, H, W, C, tc, stream())
    sync()
    check(pd, R.coord_pool_fwd_ref(x, B, H, W, p0), ex, "coord_pool means")
    for acc in ((0, 1) if ex else (0,)):                                    # the bounded case adds two rounded terms already
        dp, dx0 = fn(tag + "dp", (B * (H + W), C), dtype), outbuf(tag + "dx", rows, C, dtype, acc)
        dpd, dxd = dev(dp), dev(dx0)
        L.tc_coord_pool_bwd(ptr(dpd), ptr(dxd), B, H, W, C, acc, tc, stream())
        sync()
        check(dxd, R.coord_pool_bwd_ref(dp, B, H, W, dx0, bool(acc)), ex, "coord_pool dx")


@EACH_DTYPE
@ACC
@pytest.mark.parametrize("case", COORD, ids=str)
def test_coord_gate(case, acc, dtype):
    """tc_coord_gate_fwd / _bwd: products and sums only, so exact on every map, 5 x 9 included."""
    B, H, W, C = case
    rows, tc, L, tag = B * H * W, TC[dtype], lib(), f"cog{case}"
    x, att, y0 = halves(tag + "x", (rows, C), dtype), quarters(tag + "a", (B * (H + W), C), dtype), outbuf(tag + "y", rows, C, dtype)
    xd, ad, yd = dev(x), dev(att), dev(y0)
    L.tc_coord_gate_fwd(ptr(xd), ptr(ad), ptr(yd), B, H, W, C, tc, stream())
    sync()
    exact(yd, R.coord_gate_fwd_ref(x, att, B, H, W, y0), "gated")
    dy, dx0, da0 = halves(tag + "dy", (rows, C), dtype), outbuf(tag + "dx", rows, C, dtype, acc), outbuf(tag + "da", B * (H + W), C, dtype, 0, 3)
    premise((dy.double() * x.double()).abs().view(B, H * W, C).sum(1), 1.0 / 16)
    dyd, dxd, dad = dev(dy), dev(dx0), dev(da0)
    L.tc_coord_gate_bwd(ptr(dyd), ptr(xd), ptr(ad), ptr(dxd), acc, ptr(dad), B, H, W, C, tc, stream())
    sync()
    wx, wa = R.coord_gate_bwd_ref(dy, x, att, B, H, W, dx0, da0, bool(acc))
    exact(dxd, wx, "dx")
    exact(dad, wa, "datt")


# ---------------------------------------------------------------------------------------------------------------- pure moves
@EACH_DTYPE
@pytest.mark.parametrize("inverse", [0, 1], ids=["expand", "inverse"])
@pytest.mark.parametrize("case", [(2, 3, 5, 4, 8), (1, 2, 2, 2, 4)], ids=str)
def test_pixel_shuffle(case, inverse, dtype):
    B, H, W, p, c = case
    n = B * H * W * p * p * c
    x, o0 = vals(f"ps{case}{inverse}", (n,), dtype), sent((n + 8,), dtype)
    xd, od = dev(x), dev(o0)
    lib().tc_pixel_shuffle(ptr(xd), ptr(od), B, H, W, p, c, inverse, TC[dtype], stream())
    sync()
    same_bits(od, R.pixel_shuffle_ref(x, o0, B, H, W, p, c, bool(inverse)), "pixel shuffle")


@EACH_DTYPE
@pytest.mark.parametrize("case", [(3, 50, 9), (2, 33, 65)], ids=str)
def test_transpose(case, dtype):
    nb, Rr, Cc = case
    n = nb * Rr * Cc
    x, o0 = vals(f"tr{case}", (n,), dtype), sent((n + 8,), dtype)
    xd, od = dev(x), dev(o0)
    lib().tc_transpose(ptr(xd), ptr(od), nb, Rr, Cc, TC[dtype], stream())
    sync()
    same_bits(od, R.transpose_ref(x, o0, nb, Rr, Cc), "transpose")


# ---------------------------------------------------------------------------------------------------------------- CBAM: token pooling
def _chan_pool2_run(x, B, N, C, ldx, dtype, is_exact, what):
    """tc_chan_pool2_fwd on x[:, :C]; checks pooled (max rows always exact) and idx against the reference; returns the device's idx."""
    p0, i0 = sent((2 * B + 1, C), dtype), torch.full((B + 1, C), -7, dtype=torch.int32)
    premise(x[:, :C].double().abs().view(B, N, C).sum(1), 0.5)
    xd, pd, idd = dev(x), dev(p0), dev(i0)
    lib().tc_chan_pool2_fwd(ptr(xd), ldx, ptr(pd), ptr(idd), B, N, C, TC[dtype], stream())
    sync()
    wp, wi = R.chan_pool2_fwd_ref(x[:, :C], B, N, p0, i0)
    exact(pd[:B], wp[:B], what + " max")
    check(pd, wp, is_exact, what + " max | mean")
    assert torch.equal(idd.cpu(), wi), what + " idx"
    return idd, wi


def _chan_pool2_bwd(idd, wi, B, N, C, dtype, acc, is_exact, tag):
    fn = halves if is_exact else nonneg
    dp, dx0 = fn(tag + "dp", (2 * B, C), dtype), outbuf(tag + "dx", B * N, C + 8, dtype, acc, fn=fn)
    dpd, dxd = dev(dp), dev(dx0)
    lib().tc_chan_pool2_bwd(ptr(dpd), ptr(idd), ptr(dxd), C + 8, B, N, C, acc, TC[dtype], stream())
    sync()
    check(dxd, R.chan_pool2_bwd_ref(dp, wi, B, N, dx0, bool(acc)), is_exact, "chan_pool2 dx")


@EACH_DTYPE
@pytest.mark.parametrize("shape", SHAPES + MEANS, ids=str)
def test_chan_pool2(shape, dtype):
    """tc_chan_pool2_fwd / _bwd on grid inputs (where maxima tie as a matter of course): value, first index, mean, and the gradient
    routed to idx, written and accumulated.  N = 37: the mean half and the backward (non-negative, written) are the bounded mean."""
    B, N, C = shape
    ex = pow2(N)
    x = halves(f"c2{shape}", (B * N, C + 4), dtype)
    idd, wi = _chan_pool2_run(x, B, N, C, C + 4, dtype, ex, "chan_pool2")
    for acc in ((0, 1) if ex else (0,)):
        _chan_pool2_bwd(idd, wi, B, N, C, dtype, acc, ex, f"c2b{shape}{acc}")


@EACH_DTYPE
@pytest.mark.parametrize("N", [64, 8])
def test_chan_pool2_planted_ties(N, dtype):
    """The first maximal row: the maximum 2.0 planted above values <= 1.5 at the first and last row, the last alone, rows r and r + 1 (two row
    lanes), r and r + 16 (one lane), a later lane holding the earlier row, an all-equal column, and a column whose maximum is zero with -0.0
    before +0.0 (values compared, the index is the first zero)."""
    B, C = 2, 8
    x = halves(f"c2t{N}", (B * N, C + 4), dtype, lim=3)
    x3 = x.view(B, N, C + 4)
    far = (5, 21) if N > 21 else (1, 5)
    back = (17, 2) if N > 17 else (6, 2)
    x3[:, 0, 0] = x3[:, N - 1, 0] = 2.0
    x3[:, N - 1, 1] = 2.0
    x3[:, 5, 2] = x3[:, 6, 2] = 2.0
    x3[:, far[0], 3] = x3[:, far[1], 3] = 2.0
    x3[:, :, 4] = 1.0
    x3[:, :, 5] = -x3[:, :, 5].abs() - 0.5
    x3[:, 3, 5], x3[:, 7, 5] = -0.0, 0.0
    x3[:, back[0], 6] = x3[:, back[1], 6] = 2.0
    x3[:, :, 7] = -x3[:, :, 7].abs() - 0.5
    x3[:, 4, 7], x3[:, 2, 7] = -0.0, 0.0                                     # +0.0 first this time
    idd, wi = _chan_pool2_run(x, B, N, C, C + 4, dtype, True, "planted ties")
    assert wi[:B].tolist() == [[0, N - 1, 5, far[0], 0, 3, 2, 2]] * B
    for acc in (0, 1):
        _chan_pool2_bwd(idd, wi, B, N, C, dtype, acc, True, f"c2tb{N}{acc}")


# ---------------------------------------------------------------------------------------------------------------- CBAM: channel statistics
def _pix_stats_run(x, rows, C, ldx, dtype, what):
    ex = pow2(C)
    s0, i0 = sent((rows + 2, 2), dtype), torch.full((rows + 3,), -7, dtype=torch.int32)
    premise(x[:, :C].double().abs().sum(1), 0.5)
    xd, sd, idd = dev(x), dev(s0), dev(i0)
    lib().tc_pix_stats_fwd(ptr(xd), ldx, ptr(sd), ptr(idd), rows, C, TC[dtype], stream())
    sync()
    ws, wi = R.pix_stats_fwd_ref(x[:, :C], s0, i0)
    exact(sd[:, 0], ws[:, 0], what + " max")
    check(sd, ws, ex, what + " max | mean")
    assert torch.equal(idd.cpu(), wi), what + " idx"
    return idd, wi


def _pix_stats_bwd(idd, wi, rows, C, dtype, acc, tag):
    ex = pow2(C)
    fn = halves if ex else nonneg
    ds, dx0 = fn(tag + "ds", (rows, 2), dtype), outbuf(tag + "dx", rows, C + 8, dtype, acc, fn=fn)
    dsd, dxd = dev(ds), dev(dx0)
    lib().tc_pix_stats_bwd(ptr(dsd), ptr(idd), ptr(dxd), C + 8, rows, C, acc, TC[dtype], stream())
    sync()
    check(dxd, R.pix_stats_bwd_ref(ds, wi, C, dx0, bool(acc)), ex, "pix_stats dx")


@EACH_DTYPE
@pytest.mark.parametrize("shape", SHAPES + MEANS, ids=str)
def test_pix_stats(shape, dtype):
    """tc_pix_stats_fwd / _bwd: the pooled length is C here, so C in {4, 128} is exact and C in {24, 72} the bounded mean (its backward
    non-negative and written only).  Rows B N in {2, 16, 37, 64, 74, 192}: fewer than, exactly and more than one block of 16 row lanes."""
    B, N, C = shape
    rows = B * N
    x = halves(f"px{shape}", (rows, C + 4), dtype)
    idd, wi = _pix_stats_run(x, rows, C, C + 4, dtype, "pix_stats")
    for acc in ((0, 1) if pow2(C) else (0,)):
        _pix_stats_bwd(idd, wi, rows, C, dtype, acc, f"pxb{shape}{acc}")


@EACH_DTYPE
@pytest.mark.parametrize("C", [128, 8])
def test_pix_stats_planted_ties(C, dtype):
    """The first maximal channel: the maximum planted at the first and last channel, the last alone, two channels of one quad, of two quads
    (two lanes), of one lane's two passes (c and c + 64), an earlier channel in a later lane, an all-equal row, and rows whose maximum is zero
    with both signs present.  20 rows: the last four belong to a second block."""
    rows = 20
    x = halves(f"pxt{C}", (rows, C + 4), dtype, lim=3)
    two_pass = (5, 69) if C > 69 else (1, 6)
    later = (70, 9) if C > 70 else (6, 1)
    x[0, 0] = x[0, C - 1] = 2.0
    x[1, C - 1] = 2.0
    x[2, 5] = x[2, 6] = 2.0
    x[3, 2] = x[3, 7] = 2.0
    x[4, two_pass[0]] = x[4, two_pass[1]] = 2.0
    x[5, later[0]] = x[5, later[1]] = 2.0
    x[6, :C] = 0.5
    x[7, :C] = -x[7, :C].abs() - 0.5
    x[7, 3], x[7, 6] = -0.0, 0.0
    x[8, :C] = -x[8, :C].abs() - 0.5
    x[8, 7], x[8, 1] = -0.0, 0.0
    x[17, 4] = x[17, C - 1] = 2.0                                            # and in the second block
    idd, wi = _pix_stats_run(x, rows, C, C + 4, dtype, "planted ties")
    assert wi[:9].tolist() == [0, C - 1, 5, 2, two_pass[0], later[1], 0, 3, 1] and int(wi[17]) == 4
    for acc in (0, 1):
        _pix_stats_bwd(idd, wi, rows, C, dtype, acc, f"pxtb{C}{acc}")


# ---------------------------------------------------------------------------------------------------------------- CBAM: spatial attention
SA = [(2, 5, 9), (1, 3, 3)]                                                # the 3 x 3 map is smaller than the 7 x 7 window


@EACH_DTYPE
@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("case", SA, ids=str)
def test_sa_conv_fwd(case, k, dtype):
    """tc_sa_conv_fwd: weights in eighths, statistics in halves and a bias of 1/4 make the pre-activation exact; the sigmoid is held to
    2e-6 + 1e-5 |want| (+ half a storage spacing)."""
    B, H, W = case
    n, tag = B * H * W, f"saf{case}{k}"
    st = halves(tag + "st", (n, 2), dtype)
    w, bias = (halves(tag + "w", (2 * k * k,), dtype, lim=2) / 4).to(dtype), torch.tensor([0.25], dtype=dtype)
    pre = R.sa_conv_pre_ref(st, w, bias, B, H, W, k)
    assert torch.equal(pre.float().double(), pre)
    premise(0.25 + 2 * k * k * float(w.double().abs().max()) * float(st.double().abs().max()), 1.0 / 16)
    g0 = sent((n + 3,), dtype)
    sd, wd, bd, gd = dev(st), dev(w), dev(bias), dev(g0)
    lib().tc_sa_conv_fwd(ptr(sd), ptr(wd), ptr(bd), ptr(gd), B, H, W, k, TC[dtype], stream())
    sync()
    want = R.sa_conv_fwd_ref(st, w, bias, B, H, W, k, g0)
    within(gd, want, 2e-6 + 1e-5 * want.abs() + half_spacing(want, dtype), f"sa_conv sigmoid {case} k={k}")
    assert bool((gd.cpu()[n:] == SENT).all())


@EACH_DTYPE
@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("case", SA, ids=str)
def test_sa_conv_bwd(case, k, dtype):
    """tc_sa_conv_bwd from a stored gate in quarters: dz = dg g (1 - g) is a multiple of 1/32, the transposed convolution into dst and the
    fp32 += of dw and db (from the grid values 1.5 and -0.5) are exact."""
    B, H, W = case
    n, tag = B * H * W, f"sab{case}{k}"
    dg, g, st, w = halves(tag + "dg", (n,), dtype), quarters(tag + "g", (n,), dtype), halves(tag + "st", (n, 2), dtype), halves(tag + "w", (2 * k * k,), dtype)
    d0, dw0, db0 = sent((n + 1, 2), dtype), f32buf(2 * k * k, 1.5), f32buf(1, -0.5)
    premise(n * 2.0 * 0.25 * 2.0, 1.0 / 64)                                 # dw: n terms |dz| <= 1/2 times |st| <= 2; dst: 2 k k <= n terms below that
    premise(2 * k * k * 2.0 * 0.5, 1.0 / 64)
    dgd, gd, sd, wd, dd, dwd, dbd = dev(dg), dev(g), dev(st), dev(w), dev(d0), dev(dw0), dev(db0)
    lib().tc_sa_conv_bwd(ptr(dgd), ptr(gd), ptr(sd), ptr(wd), ptr(dd), ptr(dwd), ptr(dbd), B, H, W, k, TC[dtype], stream())
    sync()
    wdst, wdw, wdb = R.sa_conv_bwd_ref(dg, g, st, w, B, H, W, k, d0[:n], dw0[:2 * k * k], db0[:1])
    exact(dd[:n], wdst, "dst")
    exact(dwd[:2 * k * k], wdw, "dw")
    exact(dbd[:1], wdb, "db")
    assert float(dd[n, 0]) == SENT and bool((dwd.cpu()[2 * k * k:] == SENT).all()) and bool((dbd.cpu()[1:] == SENT).all())


@EACH_DTYPE
@ACC
@pytest.mark.parametrize("shape", SHAPES + MEANS, ids=str)
def test_pix_gate(shape, acc, dtype):
    """tc_pix_gate_fwd / _bwd: per-token gate in quarters; dg sums dy x over the channels (16 lanes per row, two passes at C = 128)."""
    B, N, C = shape
    rows, tc, L, tag = B * N, TC[dtype], lib(), f"pg{shape}"
    x, g, y0 = halves(tag + "x", (rows, C + 4), dtype), quarters(tag + "g", (rows,), dtype), outbuf(tag + "y", rows, C + 8, dtype)
    xd, gd, yd = dev(x), dev(g), dev(y0)
    L.tc_pix_gate_fwd(ptr(xd), C + 4, ptr(gd), ptr(yd), C + 8, rows, C, tc, stream())
    sync()
    exact(yd, R.pix_gate_fwd_ref(x[:, :C], g, y0), "gated")
    dy, dx0, dg0 = halves(tag + "dy", (rows, C + 12), dtype), outbuf(tag + "dx", rows, C + 8, dtype, acc), sent((rows + 3,), dtype)
    premise((dy[:, :C].double() * x[:, :C].double()).abs().sum(1), 0.25)
    dyd, dxd, dgd = dev(dy), dev(dx0), dev(dg0)
    L.tc_pix_gate_bwd(ptr(dyd), C + 12, ptr(xd), C + 4, ptr(gd), ptr(dxd), C + 8, acc, ptr(dgd), rows, C, tc, stream())
    sync()
    wx, wg = R.pix_gate_bwd_ref(dy[:, :C], x[:, :C], g, dx0, dg0, bool(acc))
    exact(dxd, wx, "dx")
    exact(dgd, wg, "dg")


# ---------------------------------------------------------------------------------------------------------------- CAM_Module
CAM = [(2, 1, 4), (2, 8, 24), (1, 64, 72), (2, 8, 128), (1, 37, 4)]


@EACH_DTYPE
@pytest.mark.parametrize("shape", CAM, ids=str)
def test_cam_att_fwd(shape, dtype):
    """tc_cam_att_fwd: x in {-1/2, 0, 1/2} ({-1/4, 0, 1/4} at N = 64) makes the 4 x 4 energies exact and keeps each row's spread below 10; softmax(max - E) is held to 2e-5 + 2e-5 |want|.
    att is fp32 in every storage type; the five floats behind it keep the sentinel."""
    B, N, C = shape
    x = halves(f"ca{shape}", (B * N, 4 * C + 4), dtype, lim=1)
    if N > 37:
        x = (x / 2).to(dtype)                                               # {-1/4, 0, 1/4}: 64 tokens of 1/2 would spread the energies past 10
    E = R.cam_energy_ref(x[:, :4 * C], B, N)
    assert torch.equal(E.float().double(), E) and float((E.max(dim=-1)[0] - E.min(dim=-1)[0]).max()) < 10.0
    premise(N * 0.25, 1.0 / 16)
    a0 = sent((B * C * 16 + 5,), torch.float32)
    xd, ad = dev(x), dev(a0)
    lib().tc_cam_att_fwd(ptr(xd), 4 * C + 4, ptr(ad), B, N, C, TC[dtype], stream())
    sync()
    want = R.cam_att_fwd_ref(x[:, :4 * C], B, N, a0)
    within(ad, want, 2e-5 + 2e-5 * want.abs(), f"cam att {shape} ({str(dtype).split('.')[-1]} storage)")
    assert bool((ad.cpu()[B * C * 16:] == SENT).all())


def _cam_inputs(tag, B, N, C, dtype, lim=4):
    x, dy = halves(tag + "x", (B * N, 4 * C + 4), dtype, lim), halves(tag + "dy", (B * N, 4 * C + 12), dtype, lim)
    return x, dy, quarters(tag + "att", (B * C * 16,), torch.float32), torch.tensor([GAMMA], dtype=torch.float32)


@EACH_DTYPE
@pytest.mark.parametrize("shape", CAM, ids=str)
def test_cam_apply_fwd(shape, dtype):
    """tc_cam_apply_fwd from an att the test chose (quarters, not a softmax: each of the 16 weights is its own value)."""
    B, N, C = shape
    x, _, att, gamma = _cam_inputs(f"cf{shape}", B, N, C, dtype)
    y0 = outbuf("cfy", B * N, 4 * C + 8, dtype)
    xd, ad, gd, yd = dev(x), dev(att), dev(gamma), dev(y0)
    lib().tc_cam_apply_fwd(ptr(xd), 4 * C + 4, ptr(ad), ptr(gd), ptr(yd), 4 * C + 8, B, N, C, TC[dtype], stream())
    sync()
    exact(yd, R.cam_apply_fwd_ref(x[:, :4 * C], att, GAMMA, B, N, y0), "cam y")


def _cam_bwd_premise(x, dy, G, B, N, att_q=0.25):
    """With x and dy in halves and att a multiple of att_q <= 1: dA sums gamma dy x (quantum 1/8); dE = -A (dA - rowsum(A dA)) is a multiple
    of att_q^2 / 8 and at most 5 max|dA|; dx adds G x (half that quantum) with G the reference's own att2; dgamma sums dy (A x) (att_q / 4)."""
    x4, d4 = R._paths(x, B, N).abs(), R._paths(dy, B, N).abs()
    dA = GAMMA * float((d4.amax(2) * x4.amax(2)).sum(1).max())               # bounds the sum of |terms| of every dA[p][q]
    premise(dA, 1.0 / 8)
    premise(5 * dA, att_q * att_q / 8)
    premise(float(G.abs().max()), att_q * att_q / 8)
    premise(float(d4.max()) * (1 + 4 * GAMMA) + 4 * float(G.abs().max()) * float(x4.max()), att_q * att_q / 16)
    premise(1.0 + float((d4.sum(2) * x4.sum(2)).sum()), att_q / 4)                # |A x| <= sum_q |x_q|


@EACH_DTYPE
@ACC
@pytest.mark.parametrize("shape", CAM, ids=str)
def test_cam_bwd(shape, acc, dtype):
    """tc_cam_bwd from a chosen att: att2 (fp32, = dE + dE^T), dgamma (fp32, += from 0.75) and dx (written / accumulated), all exact."""
    B, N, C = shape
    x, dy, att, gamma = _cam_inputs(f"cb{shape}", B, N, C, dtype)
    a20, dgm0, dx0 = sent((B * C * 16 + 4,), torch.float32), f32buf(1, 0.75), outbuf("cbdx", B * N, 4 * C + 8, dtype, acc)
    xd, dyd, ad, gd, a2d, dgd, dxd = dev(x), dev(dy), dev(att), dev(gamma), dev(a20), dev(dgm0), dev(dx0)
    lib().tc_cam_bwd(ptr(xd), 4 * C + 4, ptr(dyd), 4 * C + 12, ptr(ad), ptr(gd), ptr(a2d), ptr(dgd), ptr(dxd), 4 * C + 8, acc, B, N, C, TC[dtype], stream())
    sync()
    w2, wg, wx = R.cam_bwd_ref(x[:, :4 * C], dy[:, :4 * C], att, GAMMA, B, N, a20, dgm0[:1], dx0, bool(acc))
    _cam_bwd_premise(x[:, :4 * C], dy[:, :4 * C], w2[:B * C * 16], B, N)
    exact(a2d, w2, "att2")
    exact(dgd[:1], wg, "dgamma")
    exact(dxd, wx, "dx")
    assert bool((dgd.cpu()[1:] == SENT).all())


@EACH_DTYPE
@ACC
@pytest.mark.parametrize("shape", SHAPES + MEANS, ids=str)
def test_gamma_res(shape, acc, dtype):
    """tc_gamma_res_fwd / _bwd with gamma = 1/2 on the device: y, da, dx (written / accumulated) and the fp32 dgamma += from -1.25."""
    B, N, C = shape
    rows, tc, L, tag = B * N, TC[dtype], lib(), f"gr{shape}"
    a, x, y0 = halves(tag + "a", (rows, C + 4), dtype), halves(tag + "x", (rows, C + 8), dtype), outbuf(tag + "y", rows, C + 12, dtype)
    gamma = torch.tensor([GAMMA], dtype=torch.float32)
    ad, xd, gd, yd = dev(a), dev(x), dev(gamma), dev(y0)
    L.tc_gamma_res_fwd(ptr(ad), C + 4, ptr(xd), C + 8, ptr(gd), ptr(yd), C + 12, rows, C, tc, stream())
    sync()
    exact(yd, R.gamma_res_fwd_ref(a[:, :C], x[:, :C], GAMMA, y0), "y")
    dy = halves(tag + "dy", (rows, C + 12), dtype)
    da0, dx0, dgm0 = outbuf(tag + "da", rows, C + 16, dtype), outbuf(tag + "dx", rows, C + 8, dtype, acc, 1), f32buf(1, -1.25)
    premise(1.25 + float((dy[:, :C].double() * a[:, :C].double()).abs().sum()), 0.25)
    dyd, dad, dxd, dgd = dev(dy), dev(da0), dev(dx0), dev(dgm0)
    L.tc_gamma_res_bwd(ptr(dyd), C + 12, ptr(ad), C + 4, ptr(gd), ptr(dad), C + 16, ptr(dxd), C + 8, acc, ptr(dgd), rows, C, tc, stream())
    sync()
    wa, wx, wg = R.gamma_res_bwd_ref(dy[:, :C], a[:, :C], GAMMA, da0, dx0, dgm0[:1], bool(acc))
    exact(dad, wa, "da")
    exact(dxd, wx, "dx")
    exact(dgd[:1], wg, "dgamma")
    assert float(dgd[1]) == SENT


@EACH_DTYPE
def test_gelu_bwd(dtype):
    """tc_gelu_bwd on every finite storage value of [-8, 8] (float32: every bfloat16 and every float16 value, which it holds exactly)
    against dy (Phi(x) + x phi(x)) in float64: 5e-6 |dy| (+ half a storage spacing)."""
    pat = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    xs = [pat.view(t).float() for t in ((torch.bfloat16, torch.float16) if dtype == torch.float32 else (dtype,))]
    x = torch.cat(xs)
    x = x[torch.isfinite(x) & (x.abs() <= 8.0)].to(dtype)
    n = x.numel()
    dy, z0 = halves("gelu.dy", (n,), dtype), sent((n + 3,), dtype)
    xd, dyd, zd = dev(x), dev(dy), dev(z0)
    lib().tc_gelu_bwd(ptr(dyd), ptr(xd), ptr(zd), n, TC[dtype], stream())
    sync()
    want = R.gelu_bwd_ref(dy, x, z0)
    tol = torch.zeros(n + 3, dtype=torch.float64)
    tol[:n] = 5e-6 * dy.double().abs()
    within(zd, want, tol + half_spacing(want, dtype), "gelu gradient")


# ---------------------------------------------------------------------------------------------------------------- beyond one grid pass
# One case per grid-stride kernel, in bfloat16, with just more work than the capped grid covers in one pass (the caps are on the launch
# lines of csrc/elementwise.hip and csrc/cbam.hip): 8192 blocks x 256 quads (g1 / gq) or elements (the three flat kernels and gelu'), 4096
# blocks x 16 rows, 4096 / 256 blocks x 256 tokens (sa_conv), 1024 blocks x 256 quads (gamma_res_bwd).  Values in {-1, -1/2, 0, 1/2, 1}.
WD = torch.bfloat16
QUADS = 8192 * 256


def wgrid(tag, shape):
    return halves("w/" + tag, shape, WD, lim=2)


def _w_fma3():
    rows, C = 8200, 1024
    assert rows * C // 4 > QUADS
    a, b, c, d = (wgrid("fma" + k, (rows, C)) for k in "abcd")
    o0 = sent((rows + 1, C), WD)
    ad, bd, cd, dd, od = dev(a), dev(b), dev(c), dev(d), dev(o0)
    L = lib()
    L.tc_fma3_fwd(ptr(ad), C, ptr(bd), C, ptr(cd), C, ptr(od), C, rows, C, ALPHA, TC[WD], stream())
    sync()
    exact(od, R.fma3_fwd_ref(a, b, c, ALPHA, o0), "fma3 out")
    L.tc_add(ptr(ad), C, ptr(bd), C, ptr(od), C, rows, C, TC[WD], stream())
    sync()
    exact(od, R.add_ref(a, b, o0), "add")
    dad, dbd, dcd = dev(o0), dev(a), dev(o0)
    L.tc_fma3_bwd(ptr(dd), C, ptr(bd), C, ptr(cd), C, ptr(dad), C, ptr(dbd), C, 1, ptr(dcd), C, rows, C, ALPHA, TC[WD], stream())
    sync()
    wa, wb, wc = R.fma3_bwd_ref(d, b, c, ALPHA, o0, a, o0, True)
    exact(dad, wa, "da")
    exact(dbd, wb, "db")
    exact(dcd, wc, "dc")


def _w_flat():
    n = QUADS + 1029
    dy, s, x = wgrid("fl.dy", (n,)), quarters("fl.s", (n,), WD), wgrid("fl.x", (n,))
    z0 = sent((n + 3,), WD)
    dyd, sd, xd, zd = dev(dy), dev(s), dev(x), dev(z0)
    L = lib()
    L.tc_sigmoid_bwd(ptr(dyd), ptr(sd), ptr(zd), n, TC[WD], stream())
    sync()
    exact(zd, R.sigmoid_bwd_ref(dy, s, z0), "sigmoid'")
    L.tc_relu_fwd(ptr(xd), ptr(zd), n, TC[WD], stream())
    sync()
    y = R.relu_fwd_ref(x, z0)
    exact(zd, y, "relu")
    yd, dzd = dev(y[:n].to(WD)), dev(z0)
    L.tc_relu_bwd(ptr(dyd), ptr(yd), ptr(dzd), n, TC[WD], stream())
    sync()
    exact(dzd, R.relu_bwd_ref(dy, y[:n], z0), "relu'")
    L.tc_gelu_bwd(ptr(dyd), ptr(xd), ptr(dzd), n, TC[WD], stream())
    sync()
    want = R.gelu_bwd_ref(dy, x, z0)
    tol = torch.zeros(n + 3, dtype=torch.float64)
    tol[:n] = 5e-6 * dy.double().abs()
    within(dzd, want, tol + half_spacing(want, WD), "gelu gradient beyond one pass")


def _w_chan():
    B, N, C = 1025, 8, 1024
    assert B * N * C // 4 > QUADS
    x, dp, g = wgrid("ch.x", (B * N, C)), wgrid("ch.dp", (2 * B, C)), quarters("ch.g", (B, C), WD)
    o0 = sent((B * N + 1, C), WD)
    xd, dpd, gd, od = dev(x), dev(dp), dev(g), dev(o0)
    L = lib()
    L.tc_chan_pool_bwd(ptr(dpd), ptr(od), C, B, N, C, 0, TC[WD], stream())
    sync()
    exact(od, R.chan_pool_bwd_ref(dp, B, N, o0), "chan_pool dx")
    L.tc_chan_gate_fwd(ptr(xd), C, ptr(gd), ptr(od), C, B, N, C, TC[WD], stream())
    sync()
    exact(od, R.chan_gate_fwd_ref(x, g, B, N, o0), "chan gate")
    idx = torch.randint(0, N, (B, C), generator=_gen("ch.idx")).to(torch.int32)
    acc0 = torch.cat([x, wgrid("ch.t", (1, C))])
    ad = dev(acc0)
    idx_d = dev(idx)
    L.tc_chan_pool2_bwd(ptr(dpd), ptr(idx_d), ptr(ad), C, B, N, C, 1, TC[WD], stream())
    sync()
    exact(ad, R.chan_pool2_bwd_ref(dp, idx, B, N, acc0, True), "chan_pool2 dx")


def _w_coord():
    B, H, W, C = 2050, 2, 2, 1024
    assert B * (H + W) * C // 4 > QUADS and B * H * W * C // 4 > QUADS
    rows = B * H * W
    x, dy, att, dp = wgrid("co.x", (rows, C)), wgrid("co.dy", (rows, C)), quarters("co.a", (B * (H + W), C), WD), wgrid("co.dp", (B * (H + W), C))
    o0 = sent((rows + 1, C), WD)
    xd, dyd, ad, dpd, od = dev(x), dev(dy), dev(att), dev(dp), dev(o0)
    L = lib()
    L.tc_coord_pool_fwd(ptr(xd), ptr(od), B, H, W, C, TC[WD], stream())
    sync()
    exact(od, R.coord_pool_fwd_ref(x, B, H, W, o0), "coord means")
    L.tc_coord_pool_bwd(ptr(dpd), ptr(od), B, H, W, C, 0, TC[WD], stream())
    sync()
    exact(od, R.coord_pool_bwd_ref(dp, B, H, W, o0), "coord_pool dx")
    L.tc_coord_gate_fwd(ptr(xd), ptr(ad), ptr(od), B, H, W, C, TC[WD], stream())
    sync()
    exact(od, R.coord_gate_fwd_ref(x, att, B, H, W, o0), "coord gate")
    dad = dev(o0)
    L.tc_coord_gate_bwd(ptr(dyd), ptr(xd), ptr(ad), ptr(od), 0, ptr(dad), B, H, W, C, TC[WD], stream())
    sync()
    wx, wa = R.coord_gate_bwd_ref(dy, x, att, B, H, W, o0, o0)
    exact(od, wx, "coord gate dx")
    exact(dad, wa, "datt")


def _w_pixel_shuffle():
    B, H, W, p, c = 2, 64, 65, 4, 64
    n = B * H * W * p * p * c
    assert n // 4 > QUADS
    x, o0 = vals("w.ps", (n,), WD), sent((n + 8,), WD)
    xd, od = dev(x), dev(o0)
    for inverse in (0, 1):
        lib().tc_pixel_shuffle(ptr(xd), ptr(od), B, H, W, p, c, inverse, TC[WD], stream())
        sync()
        same_bits(od, R.pixel_shuffle_ref(x, o0, B, H, W, p, c, bool(inverse)), f"pixel shuffle inverse={inverse}")


def _w_rows():
    """pix_stats_fwd / pix_gate_bwd: 65 552 rows at C = 8 (4096 blocks x 16 rows is 65 536); pix_stats_bwd and pix_gate_fwd on 8200 x 1024."""
    rows, C = 4096 * 16 + 16, 8
    x, dy, g = wgrid("rw.x", (rows, C)), wgrid("rw.dy", (rows, C)), quarters("rw.g", (rows,), WD)
    idd, wi = _pix_stats_run(x, rows, C, C, WD, "pix_stats beyond one pass")
    dx0, dg0 = sent((rows + 1, C), WD), sent((rows + 3,), WD)
    xd, dyd, gd, dxd, dgd = dev(x), dev(dy), dev(g), dev(dx0), dev(dg0)
    lib().tc_pix_gate_bwd(ptr(dyd), C, ptr(xd), C, ptr(gd), ptr(dxd), C, 0, ptr(dgd), rows, C, TC[WD], stream())
    sync()
    wx, wg = R.pix_gate_bwd_ref(dy, x, g, dx0, dg0)
    exact(dxd, wx, "pix_gate dx")
    exact(dgd, wg, "pix_gate dg")
    rows, C = 8200, 1024
    x, ds, g = wgrid("rw.x2", (rows, C)), wgrid("rw.ds", (rows, 2)), quarters("rw.g2", (rows,), WD)
    idx = torch.randint(0, C, (rows,), generator=_gen("rw.idx")).to(torch.int32)
    o0 = sent((rows + 1, C), WD)
    xd, od = dev(x), dev(o0)
    g_d = dev(g)
    lib().tc_pix_gate_fwd(ptr(xd), C, ptr(g_d), ptr(od), C, rows, C, TC[WD], stream())
    sync()
    exact(od, R.pix_gate_fwd_ref(x, g, o0), "pix_gate y")
    ds_d, idx_d = dev(ds), dev(idx)
    lib().tc_pix_stats_bwd(ptr(ds_d), ptr(idx_d), ptr(od), C, rows, C, 0, TC[WD], stream())
    sync()
    exact(od, R.pix_stats_bwd_ref(ds, idx, C, o0), "pix_stats dx")


def _w_sa_conv():
    """forward: 1 x 1025 x 1024 tokens (the cap is 4096 x 256 = 1 048 576); backward: 1 x 260 x 256 (256 x 256 = 65 536)."""
    k = 3
    B, H, W = 1, 1025, 1024
    n = B * H * W
    st, w, bias = wgrid("sa.st", (n, 2)), (wgrid("sa.w", (2 * k * k,)) / 4).to(WD), torch.tensor([0.25], dtype=WD)
    g0 = sent((n + 3,), WD)
    gd = dev(g0)
    st_d, w_d, bias_d = dev(st), dev(w), dev(bias)
    lib().tc_sa_conv_fwd(ptr(st_d), ptr(w_d), ptr(bias_d), ptr(gd), B, H, W, k, TC[WD], stream())
    sync()
    want = R.sa_conv_fwd_ref(st, w, bias, B, H, W, k, g0)
    within(gd, want, 2e-6 + 1e-5 * want.abs() + half_spacing(want, WD), "sa_conv sigmoid beyond one pass")
    B, H, W = 1, 260, 256
    n = B * H * W
    dg, g, st, w = wgrid("sb.dg", (n,)), quarters("sb.g", (n,), WD), wgrid("sb.st", (n, 2)), wgrid("sb.w", (2 * k * k,))
    premise(n * 0.25 * 1.0, 1.0 / 64)
    d0, dw0, db0 = sent((n + 1, 2), WD), f32buf(2 * k * k, 1.5), f32buf(1, -0.5)
    dd, dwd, dbd = dev(d0), dev(dw0), dev(db0)
    dg_d, g_d, st_d, w_d = dev(dg), dev(g), dev(st), dev(w)
    lib().tc_sa_conv_bwd(ptr(dg_d), ptr(g_d), ptr(st_d), ptr(w_d), ptr(dd), ptr(dwd), ptr(dbd), B, H, W, k, TC[WD], stream())
    sync()
    wdst, wdw, wdb = R.sa_conv_bwd_ref(dg, g, st, w, B, H, W, k, d0[:n], dw0[:2 * k * k], db0[:1])
    exact(dd[:n], wdst, "dst")
    exact(dwd[:2 * k * k], wdw, "dw")
    exact(dbd[:1], wdb, "db")
    assert float(dd[n, 0]) == SENT


def _w_gamma_res():
    """forward on 8200 x 1024; backward on 1032 x 1024 = 264 192 quads (the cap is 1024 x 256 = 262 144)."""
    gamma = dev(torch.tensor([GAMMA], dtype=torch.float32))
    rows, C = 8200, 1024
    a, x, o0 = wgrid("g.a", (rows, C)), wgrid("g.x", (rows, C)), sent((rows + 1, C), WD)
    od = dev(o0)
    a_d, x_d = dev(a), dev(x)
    lib().tc_gamma_res_fwd(ptr(a_d), C, ptr(x_d), C, ptr(gamma), ptr(od), C, rows, C, TC[WD], stream())
    sync()
    exact(od, R.gamma_res_fwd_ref(a, x, GAMMA, o0), "y")
    rows = 1032
    assert rows * C // 4 > 1024 * 256
    dy, a = wgrid("g.dy", (rows, C)), wgrid("g.a2", (rows, C))
    premise(1.25 + float((dy.double() * a.double()).abs().sum()), 0.25)
    da0, dx0, dgm0 = sent((rows + 1, C), WD), wgrid("g.dx", (rows + 1, C)), f32buf(1, -1.25)
    dad, dxd, dgd = dev(da0), dev(dx0), dev(dgm0)
    dy_d, a_d = dev(dy), dev(a)
    lib().tc_gamma_res_bwd(ptr(dy_d), C, ptr(a_d), C, ptr(gamma), ptr(dad), C, ptr(dxd), C, 1, ptr(dgd), rows, C, TC[WD], stream())
    sync()
    wa, wx, wg = R.gamma_res_bwd_ref(dy, a, GAMMA, da0, dx0, dgm0[:1], True)
    exact(dad, wa, "da")
    exact(dxd, wx, "dx")
    exact(dgd[:1], wg, "dgamma")


def _w_cam():
    """cam_apply (both modes): 1 x 32 800 rows x 4 x 256 channels = 2 099 200 quads.  dy is sparse (one value in 64 is non-zero) and att
    in {0, 1/2, 1}, so that the dgamma sum over 33 M products keeps the premise."""
    B, N, C = 1, 32800, 256
    assert B * N * C // 4 > QUADS
    x = wgrid("cam.x", (N, 4 * C))
    dy = (wgrid("cam.dy", (N, 4 * C)) * (torch.randint(0, 64, (N, 4 * C), generator=_gen("cam.m")) == 0)).to(WD)
    att = (torch.randint(0, 3, (B * C * 16,), generator=_gen("cam.att")).float() / 2)
    gamma = dev(torch.tensor([GAMMA], dtype=torch.float32))
    o0 = sent((N + 1, 4 * C), WD)
    xd, dyd, ad, od = dev(x), dev(dy), dev(att), dev(o0)
    lib().tc_cam_apply_fwd(ptr(xd), 4 * C, ptr(ad), ptr(gamma), ptr(od), 4 * C, B, N, C, TC[WD], stream())
    sync()
    exact(od, R.cam_apply_fwd_ref(x, att, GAMMA, B, N, o0), "cam y")
    a20, dgm0 = sent((B * C * 16 + 4,), torch.float32), f32buf(1, 0.75)
    a2d, dgd, dxd = dev(a20), dev(dgm0), dev(o0)
    lib().tc_cam_bwd(ptr(xd), 4 * C, ptr(dyd), 4 * C, ptr(ad), ptr(gamma), ptr(a2d), ptr(dgd), ptr(dxd), 4 * C, 0, B, N, C, TC[WD], stream())
    sync()
    w2, wg, wx = R.cam_bwd_ref(x, dy, att, GAMMA, B, N, a20, dgm0[:1], o0)
    _cam_bwd_premise(x, dy, w2[:B * C * 16], B, N, att_q=0.5)
    exact(a2d, w2, "att2")
    exact(dgd[:1], wg, "dgamma")
    exact(dxd, wx, "dx")


WRAPS = {"fma3_add": _w_fma3, "sigmoid_relu_gelu": _w_flat, "chan_pool_gate_pool2": _w_chan, "coord": _w_coord, "pixel_shuffle": _w_pixel_shuffle,
         "pix_stats_pix_gate": _w_rows, "sa_conv": _w_sa_conv, "gamma_res": _w_gamma_res, "cam": _w_cam}


@pytest.mark.parametrize("which", sorted(WRAPS))
def test_beyond_one_grid_pass(which):
    WRAPS[which]()


# ---------------------------------------------------------------------------------------------------------------- refusals
# name -> (index of a size argument, its refused value, index of a pointer argument, the argument list of a valid call).  Pointers are
# written as ("p", k): region k of one sentinel-filled buffer.  B = 1, N = 2 (H = 2, W = 1), C = 8, contiguous rows.
P = [("p", k) for k in range(12)]
REFUSALS = {
    "tc_fma3_fwd": (9, 6, 0, [P[0], 8, P[1], 8, P[2], 8, P[3], 8, 2, 8, ALPHA]),
    "tc_fma3_bwd": (9, 10, 6, [P[0], 8, P[1], 8, P[2], 8, P[3], 8, P[4], 8, 0, P[5], 8, 2, 8, ALPHA]),
    "tc_add": (5, 10, 4, [P[0], 8, P[1], 8, P[2], 8, 2, 8]),
    "tc_sigmoid_bwd": (3, 0, 1, [P[0], P[1], P[2], 16]),
    "tc_relu_fwd": (2, 0, 0, [P[0], P[1], 16]),
    "tc_relu_bwd": (3, 0, 2, [P[0], P[1], P[2], 16]),
    "tc_chan_pool_fwd": (5, 6, 2, [P[0], 8, P[1], 1, 2, 8]),
    "tc_chan_pool_bwd": (2, 10, 0, [P[0], P[1], 8, 1, 2, 8, 0]),
    "tc_chan_gate_fwd": (1, 10, 2, [P[0], 8, P[1], P[2], 8, 1, 2, 8]),
    "tc_chan_gate_bwd": (1, 10, 8, [P[0], 8, P[1], 8, P[2], P[3], 8, 0, P[4], 1, 2, 8]),
    "tc_coord_pool_fwd": (5, 6, 1, [P[0], P[1], 1, 2, 1, 8]),
    "tc_coord_pool_bwd": (5, 6, 0, [P[0], P[1], 1, 2, 1, 8, 0]),
    "tc_coord_gate_fwd": (6, 6, 1, [P[0], P[1], P[2], 1, 2, 1, 8]),
    "tc_coord_gate_bwd": (9, 6, 5, [P[0], P[1], P[2], P[3], 0, P[4], 1, 2, 1, 8]),
    "tc_pixel_shuffle": (6, 6, 0, [P[0], P[1], 1, 1, 1, 2, 4, 0]),
    "tc_transpose": (2, 0, 1, [P[0], P[1], 1, 2, 8]),
    "tc_chan_pool2_fwd": (1, 10, 3, [P[0], 8, P[1], P[2], 1, 2, 8]),
    "tc_chan_pool2_bwd": (6, 6, 1, [P[0], P[1], P[2], 8, 1, 2, 8, 0]),
    "tc_pix_stats_fwd": (5, 6, 2, [P[0], 8, P[1], P[2], 2, 8]),
    "tc_pix_stats_bwd": (3, 10, 1, [P[0], P[1], P[2], 8, 2, 8, 0]),
    "tc_sa_conv_fwd": (7, 5, 2, [P[0], P[1], P[2], P[3], 1, 2, 1, 3]),
    "tc_sa_conv_bwd": (10, 5, 5, [P[0], P[1], P[2], P[3], P[4], P[5], P[6], 1, 2, 1, 3]),
    "tc_pix_gate_fwd": (4, 10, 2, [P[0], 8, P[1], P[2], 8, 2, 8]),
    "tc_pix_gate_bwd": (10, 6, 8, [P[0], 8, P[1], 8, P[2], P[3], 8, 0, P[4], 2, 8]),
    "tc_cam_att_fwd": (5, 6, 2, [P[0], 32, P[1], 1, 2, 8]),
    "tc_cam_apply_fwd": (5, 34, 3, [P[0], 32, P[1], P[2], P[3], 32, 1, 2, 8]),
    "tc_cam_bwd": (3, 34, 6, [P[0], 32, P[1], 32, P[2], P[3], P[4], P[5], P[6], 32, 0, 1, 2, 8]),
    "tc_gamma_res_fwd": (1, 10, 4, [P[0], 8, P[1], 8, P[2], P[3], 8, 2, 8]),
    "tc_gamma_res_bwd": (6, 10, 10, [P[0], 8, P[1], 8, P[2], P[3], 8, P[4], 8, 0, P[5], 2, 8]),
    "tc_gelu_bwd": (3, 0, 1, [P[0], P[1], P[2], 16]),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_argument_refusals(name):
    """A column count or leading dimension that is not a multiple of 4 (k = 5 for sa_conv; a count of 0 for the entries that take no such
    argument), and a null pointer: each returns TC_ERR_ARG before any launch, and nothing the pointers reach has changed."""
    size_at, size_bad, ptr_at, args = REFUSALS[name]
    buf = dev(sent((12 * 512,), torch.float32))
    good = [ptr(buf, 512 * a[1]) if isinstance(a, tuple) else a for a in args]
    assert isinstance(args[ptr_at], tuple) and not isinstance(args[size_at], tuple)
    fn = getattr(lib(), name)
    for at, value in ((size_at, size_bad), (ptr_at, None)):
        bad = list(good)
        bad[at] = value
        for tc in (TC_F32, TC_BF16, TC_F16):
            with pytest.raises(TcError, match="status -1"):
                fn(*bad, tc, stream())
    sync()
    assert bool((buf == SENT).all())

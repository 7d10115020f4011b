"""The layout moves of csrc/elementwise.hip, one entry point at a time, against the host references of tests/layout_ref.py.

Every comparison in this file is exact.  A forward move carries bits: its inputs are arbitrary finite values of the storage type (with -0.0
and the type's largest finite value among them) and the bit patterns are compared.  An accumulating move (a backward into a gradient that
exists, tc_col2im3s2's up to four taps, accumulate = 1) gets inputs on a grid -- multiples of 1/8 with |v| <= 4 -- for the incoming
gradient and for the gradient already there: a sum of up to five such terms is a multiple of 1/8 below 32, which float32, bfloat16 (8
significant bits) and float16 all hold exactly, so the result equals the float64 reference cast to the type.  Output buffers are larger than
the op needs and pre-filled with a sentinel; the whole buffer is compared, so rows and columns the op must leave alone are checked too."""
import pytest
import torch

from layout_ref import col2im3s2_ref, im2col3s2_ref, stem_im2col_ref, tokens_to_nchw, window_rows_ref

pytestmark = pytest.mark.gpu

from transception_amd._lib import EW_COPY, EW_DEINTERLEAVE, EW_MULTI_MAX, EW_PATCHIFY, TC_BF16, TC_F16, TC_F32, TcError, TcEwSeg, lib  # noqa: E402
from transception_amd.seeded_init import seeded_tensor  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TC = {torch.float32: TC_F32, torch.bfloat16: TC_BF16, torch.float16: TC_F16}
SENT = -96.0                       # exact in every storage type, outside the grid's sums (|sum of five| <= 20)


def _name(dtype):
    return str(dtype).split(".")[-1]


def vals(tag, shape, dtype):
    """Arbitrary finite seeded values rounded to the storage type, with -0.0 and +-the largest finite value planted at the front."""
    t = torch.from_numpy(seeded_tensor("layout/" + tag, shape, 3.0)).to(dtype)
    f = t.view(-1)
    for i, v in enumerate((-0.0, torch.finfo(dtype).max, -torch.finfo(dtype).max)[:f.numel()]):
        f[(i * 7) % f.numel()] = v
    return t


def grid(tag, shape, dtype):
    """Seeded multiples of 1/8 in [-4, 4] (no -0.0)."""
    t = torch.from_numpy(seeded_tensor("layout/grid/" + tag, shape, 2.0))
    return ((t * 8).round().clamp(-32, 32) / 8 + 0.0).to(dtype)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return torch.equal(bits(got), bits(want))


def same_vals(got, want64):
    """got == the float64 reference cast to got's type (exact sums: the cast rounds nothing)."""
    want = want64.to(got.dtype)
    assert torch.equal(want.double(), want64), "the test's own inputs must make the sum exact"
    return got.shape == want.shape and torch.equal(got.detach().cpu(), want)


def sent(shape, dtype):
    return torch.full(shape, SENT, dtype=dtype)


def graph(dtype):
    from transception_amd.engine import Graph
    return Graph(dtype, torch.device(DEV), training=True, record=True)


def var(t, requires_grad=True):
    from transception_amd.engine import Var
    return Var(t.to(DEV).contiguous(), requires_grad=requires_grad)


def set_grad(v, g):
    """Hand the root of v a gradient, as the consumer's backward would have."""
    v.root.grad_t = g.to(DEV).contiguous()
    v.root.whole_written = True


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


# ---------------------------------------------------------------------------------------------------------------- window_rows
WIN_CASES = [(2, 6, 9, 3, 14, 4, 8),       # non-square, ntw > ws*ws, off > 0
             (1, 4, 4, 4, 16, 0, 8),       # one window
             (2, 4, 6, 2, 5, 1, 16),
             (1, 3, 5, 1, 2, 1, 8)]        # ws == 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("acc", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("case", WIN_CASES, ids=str)
def test_window_rows_partition(case, acc, dtype):
    """dir 0 (windows <- map) through Graph.window_rows, and its backward (map gradient <- window gradient) written or accumulated."""
    B, H, W, ws, ntw, off, Cc = case
    nwin, tag = B * (H // ws) * (W // ws), f"wp{case}"
    G = graph(dtype)
    m, win0 = vals(tag + "m", (B * H * W, Cc), dtype), sent((nwin * ntw + 3, Cc), dtype)
    mv, wv = var(m), var(win0)
    G.window_rows(mv, wv, B, H, W, ws, ntw, off, to_map=False)
    assert same_bits(wv.data, window_rows_ref(m, win0, B, H, W, ws, ntw, off, to_map=False))
    gw, g0 = grid(tag + "gw", tuple(win0.shape), dtype), grid(tag + "g0", tuple(m.shape), dtype)
    set_grad(wv, gw)
    if acc:
        set_grad(mv, g0)
    G.backward()
    torch.cuda.synchronize()
    want = window_rows_ref(gw, g0 if acc else torch.zeros_like(g0), B, H, W, ws, ntw, off, to_map=True, accumulate=True)
    assert same_vals(G.grad_of(mv), want)
    assert same_bits(wv.root.grad_t, gw)                                   # the incoming gradient is only read


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", WIN_CASES, ids=str)
def test_window_rows_reverse(case, dtype):
    """dir 1 (map <- windows) and its backward: the window-matrix gradient starts as zeros and only rows off : off + ws*ws receive."""
    B, H, W, ws, ntw, off, Cc = case
    nwin, tag = B * (H // ws) * (W // ws), f"wr{case}"
    G = graph(dtype)
    win, map0 = vals(tag + "w", (nwin * ntw, Cc), dtype), sent((B * H * W + 2, Cc), dtype)
    wv, mv = var(win), var(map0)
    G.window_rows(wv, mv, B, H, W, ws, ntw, off, to_map=True)
    assert same_bits(mv.data, window_rows_ref(win, map0, B, H, W, ws, ntw, off, to_map=True))
    gm = grid(tag + "gm", tuple(map0.shape), dtype)
    set_grad(mv, gm)
    G.backward()
    torch.cuda.synchronize()
    want = window_rows_ref(gm, torch.zeros_like(win), B, H, W, ws, ntw, off, to_map=False, accumulate=True)
    assert same_vals(G.grad_of(wv), want)
    live = torch.zeros(nwin, ntw, dtype=torch.bool)
    live[:, off:off + ws * ws] = True
    assert bool((G.grad_of(wv).cpu().view(nwin, ntw, Cc)[~live] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_window_rows_two_scales_share_a_gradient(dtype):
    """Two reverse steps read rows 0:4 and 5:9 of the same 9-row windows: after both backwards each set of rows holds its own gradient and
    row 4, which no launch covers, is zero (the "four scales' launches together cover it" contract of Graph.window_rows)."""
    B, H, W, ws, ntw, Cc = 2, 4, 6, 2, 9, 16
    nwin = B * (H // ws) * (W // ws)
    G = graph(dtype)
    wv = var(vals("w2", (nwin * ntw, Cc), dtype))
    maps, grads = [], []
    for k, off in enumerate((0, 5)):
        mv = var(sent((B * H * W, Cc), dtype))
        G.window_rows(wv, mv, B, H, W, ws, ntw, off, to_map=True)
        maps.append(mv)
        grads.append(grid(f"w2g{k}", (B * H * W, Cc), dtype))
        set_grad(mv, grads[-1])
    G.backward()
    torch.cuda.synchronize()
    want = torch.zeros(nwin * ntw, Cc, dtype=torch.float64)
    for g, off in zip(grads, (0, 5)):
        want = window_rows_ref(g, want, B, H, W, ws, ntw, off, to_map=False, accumulate=True)
    got = G.grad_of(wv)
    assert same_vals(got, want)
    assert bool((got.cpu().view(nwin, ntw, Cc)[:, 4] == 0).all()) and bool((got.cpu().view(nwin, ntw, Cc)[:, :4] != 0).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_window_rows_column_slices(dtype):
    """ld > C on both sides: src and dst are column slices 3 : 3 + C of buffers 5 columns wider; the columns beside the slice, the window
    rows outside off : off + ws*ws and the rows past the end keep the sentinel, in both directions and in the backward."""
    B, H, W, ws, ntw, off, Cc = WIN_CASES[0]
    nwin, wide = B * (H // ws) * (W // ws), Cc + 5
    G = graph(dtype)
    m, win0 = vals("wsm", (B * H * W, wide), dtype), sent((nwin * ntw + 3, wide), dtype)
    mv, wv = var(m), var(win0)
    G.window_rows(mv.colslice(3, 3 + Cc), wv.colslice(3, 3 + Cc), B, H, W, ws, ntw, off, to_map=False)
    want = win0.clone()
    want[:, 3:3 + Cc] = window_rows_ref(m[:, 3:3 + Cc], win0[:, 3:3 + Cc], B, H, W, ws, ntw, off, to_map=False)
    assert same_bits(wv.data, want)
    gw = grid("wsg", tuple(win0.shape), dtype)
    set_grad(wv, gw)
    G.backward()
    torch.cuda.synchronize()
    wantg = torch.zeros(B * H * W, wide, dtype=torch.float64)              # a sliced writer's root gradient starts as zeros
    wantg[:, 3:3 + Cc] = window_rows_ref(gw[:, 3:3 + Cc], wantg[:, 3:3 + Cc], B, H, W, ws, ntw, off, to_map=True, accumulate=True)
    assert same_vals(mv.root.grad_t, wantg)
    # the reverse direction on slices (forward: its backward takes whole window matrices only)
    G2 = graph(dtype)
    src, map0 = var(want), var(sent((B * H * W + 2, wide), dtype))
    G2.window_rows(src.colslice(3, 3 + Cc), map0.colslice(3, 3 + Cc), B, H, W, ws, ntw, off, to_map=True)
    wantm = sent((B * H * W + 2, wide), dtype)
    wantm[:B * H * W, 3:3 + Cc] = m[:, 3:3 + Cc]
    assert same_bits(map0.data, wantm)


# ---------------------------------------------------------------------------------------------------------------- im2col3s2 / col2im3s2
I2C_CASES = [(2, 3, 5, 7),                 # odd sizes; 9 Cin = 27 in rows of 32: pad columns are written as zeros
             (1, 2, 6, 4), (2, 1, 1, 1), (1, 3, 2, 9), (2, 8, 8, 8)]


def _out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("acc", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("case", I2C_CASES, ids=str)
def test_im2col3s2_tokens_and_backward(case, acc, dtype):
    """Token-major source through Graph.im2col3s2: the patch matrix with its zero pad columns, then tc_col2im3s2 as its backward into an
    empty gradient (write) and into one already present (accumulate).  The pad columns of the incoming gradient hold the sentinel: they
    must not be read."""
    B, Cin, H, W = case
    Ho, Wo = _out_hw(H, W)
    ldc, tag = (9 * Cin + 7) // 8 * 8, f"i2c{case}"
    G = graph(dtype)
    x = vals(tag + "x", (B * H * W, Cin), dtype)
    xv = var(x)
    cols = G.im2col3s2(xv, B, Cin, H, W)
    want = torch.zeros(B * Ho * Wo, ldc, dtype=dtype)
    want[:, :9 * Cin] = im2col3s2_ref(tokens_to_nchw(x, B, H, W))
    assert tuple(cols.root.data.shape) == tuple(want.shape) and same_bits(cols.root.data, want)
    d = sent(tuple(want.shape), dtype)
    d[:, :9 * Cin] = grid(tag + "d", (B * Ho * Wo, 9 * Cin), dtype)
    g0 = grid(tag + "g0", tuple(x.shape), dtype)
    set_grad(cols, d)
    if acc:
        set_grad(xv, g0)
    G.backward()
    torch.cuda.synchronize()
    want64 = col2im3s2_ref(d[:, :9 * Cin], B, Cin, H, W) + (g0.double() if acc else 0.0)
    assert same_vals(G.grad_of(xv), want64)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("one", [False, True], ids=["src_ch=Cin", "src_ch=1"])
@pytest.mark.parametrize("case", I2C_CASES, ids=str)
def test_im2col3s2_image_source(case, one, dtype):
    """NCHW image source: its own Cin channels, or one channel feeding all of them."""
    B, Cin, H, W = case
    Ho, Wo = _out_hw(H, W)
    img = vals(f"i2i{case}{one}", (B, 1 if one else Cin, H, W), dtype)
    cols = graph(dtype).im2col3s2(img.to(DEV), B, Cin, H, W, src_ch=1 if one else Cin)
    want = torch.zeros(B * Ho * Wo, (9 * Cin + 7) // 8 * 8, dtype=dtype)
    want[:, :9 * Cin] = im2col3s2_ref(img, Cin)
    assert same_bits(cols.root.data, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", I2C_CASES[:2], ids=str)
def test_im2col3s2_strides_and_guards(case, dtype):
    """The two entries with row strides of the caller's choice: the source map is a column slice (ldx = Cin + 3), the patch rows are
    9 Cin + 5 wide (all written: zeros beyond 9 Cin) and the rows past the last one keep the sentinel; col2im3s2 writes a column slice of a
    wider gradient (lddx = Cin + 3) whose other columns and extra rows keep it."""
    B, Cin, H, W = case
    Ho, Wo = _out_hw(H, W)
    L, tc, tag = lib(), TC[dtype], f"i2g{case}"
    rows, ldc, ldx = B * Ho * Wo, 9 * Cin + 5, Cin + 3
    xw = vals(tag + "x", (B * H * W, ldx), dtype)
    xd, cd = xw.to(DEV), sent((rows + 2, ldc), dtype).to(DEV)
    L.tc_im2col3s2(ptr(xd, 2), ldx, 0, 0, ptr(cd), ldc, B, Cin, H, W, tc, stream())
    want = sent((rows + 2, ldc), dtype)
    want[:rows] = 0
    want[:rows, :9 * Cin] = im2col3s2_ref(tokens_to_nchw(xw[:, 2:2 + Cin], B, H, W))
    torch.cuda.synchronize()
    assert same_bits(cd, want)
    for acc in (0, 1):
        d = sent((rows, ldc), dtype)
        d[:, :9 * Cin] = grid(tag + "d", (rows, 9 * Cin), dtype)
        g0 = grid(tag + "g0", (B * H * W + 1, ldx), dtype) if acc else sent((B * H * W + 1, ldx), dtype)
        dd, gd = d.to(DEV), g0.to(DEV)
        L.tc_col2im3s2(ptr(dd), ldc, ptr(gd, 2), ldx, B, Cin, H, W, acc, tc, stream())
        torch.cuda.synchronize()
        want64 = g0.double()
        want64[:B * H * W, 2:2 + Cin] = col2im3s2_ref(d[:, :9 * Cin], B, Cin, H, W) + (g0[:B * H * W, 2:2 + Cin].double() if acc else 0.0)
        assert same_vals(gd, want64)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", I2C_CASES, ids=str)
def test_im2col3s2_adjoint(case, dtype):
    """<im2col(x), d> == <x, col2im(d)> in float64 on the host, from the DEVICE's two outputs on grid inputs: products are multiples of
    1/64 below 64 and there are fewer than 2^20 of them, so both sums are exact and the identity holds with ==."""
    B, Cin, H, W = case
    Ho, Wo = _out_hw(H, W)
    G = graph(dtype)
    x, d = grid(f"adj{case}x", (B * H * W, Cin), dtype), grid(f"adj{case}d", (B * Ho * Wo, (9 * Cin + 7) // 8 * 8), dtype)
    xv = var(x)
    cols = G.im2col3s2(xv, B, Cin, H, W)
    set_grad(cols, d)
    G.backward()
    torch.cuda.synchronize()
    lhs = (cols.data.cpu().double() * d[:, :9 * Cin].double()).sum()
    rhs = (x.double() * G.grad_of(xv).cpu().double()).sum()
    assert float(lhs) == float(rhs)


# ---------------------------------------------------------------------------------------------------------------- stem_im2col
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", [(2, 3, 9, 6), (1, 1, 5, 13), (1, 3, 4, 4), (1, 1, 1, 1)], ids=str)
def test_stem_im2col(case, dtype):
    """7 x 7 stride-4 pad-3 patches through Graph.stem_im2col (148 columns, the last one zero), and the entry itself with rows of 152:
    columns 147 .. 151 zero, the rows past the end untouched."""
    B, in_ch, H, W = case
    img = vals(f"stem{case}", (B, in_ch, H, W), dtype)
    imd = img.to(DEV)
    want = stem_im2col_ref(img)
    out = graph(dtype).stem_im2col(imd, B, in_ch, H, W)
    assert same_bits(out.data, want) and bool((out.data[:, 147] == 0).all())
    rows = want.shape[0]
    buf = sent((rows + 2, 152), dtype).to(DEV)
    lib().tc_stem_im2col(ptr(imd), ptr(buf), 152, B, in_ch, H, W, TC[dtype], stream())
    torch.cuda.synchronize()
    want2 = sent((rows + 2, 152), dtype)
    want2[:rows] = 0
    want2[:rows, :148] = want
    assert same_bits(buf, want2)


# ---------------------------------------------------------------------------------------------------------------- copy3d / TC_EW_COPY
# (nb, rows, cols, lds, ldd, sbs, sbd, source offset in elements).  The first row takes the 16-byte path in every type; each of the
# next six breaks one of its conditions (cols, either row stride -- 12 is still a multiple of float32's 4 --, either batch stride, the
# source pointer), the last is a single piece.
COPY_TABLE = [(2, 5, 8, 16, 16, 96, 104, 0),
              (2, 5, 7, 16, 16, 96, 104, 0),
              (2, 5, 8, 12, 16, 96, 104, 0),
              (2, 5, 8, 16, 12, 96, 104, 0),
              (2, 5, 8, 16, 16, 101, 104, 0),
              (2, 5, 8, 16, 16, 96, 101, 0),
              (2, 5, 8, 16, 16, 96, 104, 1),
              (1, 1, 8, 8, 8, 0, 0, 0)]
# more elements than one pass of the grid (8192 blocks x 256 threads): element path, then 16-byte path at just over 2 097 152 pieces
# (cols = one piece: 8 elements of a 16-bit type, 4 of float32 -- filled in per type)
COPY_BIG = [(4, 100000, 7, 7, 7, 700000, 700000, 0), (1, 2097160, None, None, None, 0, 0, 0)]


def _copy_ref(src, dst, row, acc):
    nb, rows, cols, lds, ldd, sbs, sbd, soff = row
    out = dst.clone()
    s = torch.as_strided(src, (nb, rows, cols), (sbs, lds, 1), soff)
    d = torch.as_strided(out, (nb, rows, cols), (sbd, ldd, 1), 0)
    if acc:
        tot = s.double() + d.double()
        assert torch.equal(tot.to(dst.dtype).double(), tot)
        d.copy_(tot.to(dst.dtype))
    else:
        d.copy_(s)
    return out


def _copy_seg(sd, dd, row, acc):
    nb, rows, cols, lds, ldd, sbs, sbd, soff = row
    return TcEwSeg(EW_COPY, acc, ptr(sd, soff), ptr(dd), sbs, sbd, lds, ldd, nb, rows, cols, 0, 0, 0)


def _copy_run(entry, sd, dd, row, acc, dtype):
    nb, rows, cols, lds, ldd, sbs, sbd, soff = row
    if entry == "copy3d":
        lib().tc_copy3d(ptr(sd, soff), sbs, lds, ptr(dd), sbd, ldd, nb, rows, cols, acc, TC[dtype], stream())
    else:
        lib().tc_ew_multi((TcEwSeg * 1)(_copy_seg(sd, dd, row, acc)), 1, TC[dtype], stream())
    torch.cuda.synchronize()


def _copy_extent(row):
    nb, rows, cols, lds, ldd, sbs, sbd, soff = row
    return soff + (nb - 1) * sbs + (rows - 1) * lds + cols, (nb - 1) * sbd + (rows - 1) * ldd + cols


def _copy_inputs(tag, row, acc, dtype):
    ns, nd = _copy_extent(row)
    ns, nd = (ns + 8 + 7) // 8 * 8, (nd + 8 + 7) // 8 * 8                  # slack after the last element read / written
    make = grid if acc else vals
    return make(tag + "s", (ns,), dtype), (grid(tag + "d", (nd,), dtype) if acc else sent((nd,), dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("entry", ["copy3d", "ew_multi"])
@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("row", COPY_TABLE, ids=str)
def test_copy3d_table(row, acc, entry, dtype):
    """Every row through tc_copy3d and through a one-segment tc_ew_multi, writing (bits) and accumulating (exact sums); the whole
    destination buffer is compared, so everything between and after the rows keeps what it held."""
    src, dst = _copy_inputs(f"cp{row}{acc}", row, acc, dtype)
    sd, dd = src.to(DEV), dst.to(DEV)
    _copy_run(entry, sd, dd, row, acc, dtype)
    assert same_bits(dd, _copy_ref(src, dst, row, acc)) and same_bits(sd, src)


def _big_row(k, dtype):
    row = COPY_BIG[k]
    if row[2] is None:
        v = 16 // torch.empty(0, dtype=dtype).element_size()
        row = (row[0], row[1], v, v, v) + row[5:]
    return row


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("entry", ["copy3d", "ew_multi"])
@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("k", [0, 1], ids=["elements", "pieces"])
def test_copy3d_beyond_one_grid_pass(k, acc, entry, dtype):
    """4 x 100 000 x 7 elements on the element path and 2 097 160 16-byte pieces on the wide path: both exceed the 2 097 152 threads of
    the capped grid, so the grid-stride loop's second pass carries the tail."""
    row = _big_row(k, dtype)
    src, dst = _copy_inputs(f"cpbig{k}{acc}", row, acc, dtype)
    sd, dd = src.to(DEV), dst.to(DEV)
    _copy_run(entry, sd, dd, row, acc, dtype)
    assert same_bits(dd, _copy_ref(src, dst, row, acc))


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_ew_multi_segments_of_very_different_size(dtype):
    """Four segments in one launch -- a 40-element copy, a k = 2 patchify, a de-interleave and the 2.8 M-element copy, which sizes the
    grid -- each bit-equal to the same move launched alone, and the two copies bit-equal to the host reference."""
    L, tc = lib(), TC[dtype]
    tiny, big = COPY_TABLE[0], _big_row(0, dtype)
    B, H, W, Cc, k = 2, 4, 6, 8, 2                                          # patchify: map [B, H, W, C] -> cols [B (H/k) (W/k), k k C]
    Bd, P, Cd, mult = 2, 5, 6, 3                                            # de-interleave: in [B, P, C mult] -> out [B, mult P, C]
    pm, di = vals("ewm.map", (B * H * W * Cc,), dtype), vals("ewm.in", (Bd * P * Cd * mult,), dtype)
    ts, td = _copy_inputs("ewm.t", tiny, 0, dtype)
    bs, bd = _copy_inputs("ewm.b", big, 0, dtype)
    out = []
    for fused in (True, False):
        pmd, did, tsd, bsd = pm.to(DEV), di.to(DEV), ts.to(DEV), bs.to(DEV)
        pc, do = sent((pm.numel() + 8,), dtype).to(DEV), sent((di.numel() + 8,), dtype).to(DEV)
        tdd, bdd = td.to(DEV), bd.to(DEV)
        if fused:
            segs = (TcEwSeg * 4)(_copy_seg(tsd, tdd, tiny, 0),
                                 TcEwSeg(EW_PATCHIFY, 0, ptr(pmd), ptr(pc), H * W * Cc, 0, Cc, 0, B, H, W, Cc, k, 0),
                                 TcEwSeg(EW_DEINTERLEAVE, 0, ptr(did), ptr(do), 0, mult * P * Cd, 0, Cd, Bd, P, Cd, mult, 0, 0),
                                 _copy_seg(bsd, bdd, big, 0))
            L.tc_ew_multi(segs, 4, tc, stream())
        else:
            _copy_run("copy3d", tsd, tdd, tiny, 0, dtype)
            L.tc_patchify(ptr(pmd), H * W * Cc, Cc, ptr(pc), B, H, W, Cc, k, 0, tc, stream())
            L.tc_sr_deinterleave(ptr(did), ptr(do), mult * P * Cd, Cd, Bd, P, Cd, mult, 0, tc, stream())
            _copy_run("copy3d", bsd, bdd, big, 0, dtype)
        torch.cuda.synchronize()
        out.append((tdd, pc, do, bdd))
    for a, b, what in zip(out[0], out[1], ("tiny copy", "patchify", "de-interleave", "large copy")):
        assert same_bits(a, b), what
    assert same_bits(out[0][0], _copy_ref(ts, td, tiny, 0)) and same_bits(out[0][3], _copy_ref(bs, bd, big, 0))
    # the two moves that have no reference of their own in this file, restated with torch on the host
    wantp = pm.view(B, H // k, k, W // k, k, Cc).permute(0, 1, 3, 5, 2, 4).reshape(-1)            # row (b, oy, ox), column (c, ky, kx)
    wantd = di.view(Bd, P, Cd, mult).permute(0, 3, 1, 2).reshape(-1)                                # out[b, g P + pos, c] = in[b, pos, c mult + g]
    assert same_bits(out[0][1][:pm.numel()], wantp.contiguous()) and same_bits(out[0][2][:di.numel()], wantd.contiguous())
    assert bool((out[0][1][pm.numel():] == SENT).all()) and bool((out[0][2][di.numel():] == SENT).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_copy_rows_offsets_through_the_engine(dtype):
    """Graph.copy_rows with a batch stride and an offset on both sides, forward and backward: the engine's pointer arithmetic."""
    nb, rows, cols = 2, 4, 8
    s_shape, d_shape = (nb * 6, 16), (nb * 7, 24)
    s_off, s_sb, d_off, d_sb = 16, 6 * 16, 2 * 24 + 8, 7 * 24
    G = graph(dtype)
    src, dst0 = vals("cr.s", s_shape, dtype), sent(d_shape, dtype)
    sv, dv = var(src), var(dst0)
    G.copy_rows(sv, s_off, s_sb, dv, d_off, d_sb, nb, rows, cols)
    fwd = (nb, rows, cols, 16, 24, s_sb, d_sb, s_off)
    want = _copy_ref(src.view(-1), dst0.view(-1)[d_off:], fwd, 0)
    assert same_bits(dv.data.view(-1)[d_off:], want) and same_bits(dv.data.view(-1)[:d_off], dst0.view(-1)[:d_off])
    gd = grid("cr.g", d_shape, dtype)
    set_grad(dv, gd)
    G.backward()
    torch.cuda.synchronize()
    bwd = (nb, rows, cols, 24, 16, d_sb, s_sb, d_off)
    wantg = torch.zeros(src.numel(), dtype=dtype)
    wantg[s_off:] = _copy_ref(gd.view(-1), wantg[s_off:], bwd, 1)
    assert same_bits(sv.root.grad_t.view(-1), wantg)


# ---------------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", [(3, 50, 9), (1, 33, 65), (2, 32, 32), (1, 1, 40)], ids=str)
def test_transpose(case, dtype):
    """[nb, R, C] -> [nb, C, R] through Graph.transpose; its backward transposes the gradient back, so feeding the output in as the
    gradient returns the input bit for bit."""
    nb, R, Cc = case
    G = graph(dtype)
    x = vals(f"tr{case}", (nb * R, Cc), dtype)
    xv = var(x)
    out = G.transpose(xv, nb)
    assert same_bits(out.data, x.view(nb, R, Cc).transpose(1, 2).reshape(nb * Cc, R))
    set_grad(out, out.data.clone().cpu())
    G.backward()
    torch.cuda.synchronize()
    assert same_bits(G.grad_of(xv), x)
    G2 = graph(dtype)                                                       # and a gradient of its own
    xv2 = var(x)
    out2 = G2.transpose(xv2, nb)
    gy = vals(f"trg{case}", (nb * Cc, R), dtype)
    set_grad(out2, gy)
    G2.backward()
    torch.cuda.synchronize()
    assert same_bits(G2.grad_of(xv2), gy.view(nb, Cc, R).transpose(1, 2).reshape(nb * R, Cc))


# ---------------------------------------------------------------------------------------------------------------- cast
def _f32(patterns):
    """float32 values from their bit patterns."""
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v for v in patterns], dtype=torch.int32).view(torch.float32)


def _special_f32():
    ties_bf16 = _f32([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF])   # half-way: to even, down and up
    ties_f16 = _f32([0x3F801000, 0x3F803000, 0xBF801000, 0xBF803000, 0x3F801001, 0x3F800FFF, 0x3F803001, 0x3F802FFF])
    misc = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), 65504.0, 65519.996, 65520.0, -65520.0, 1.0e5, -1.0e5, 3.0e38, -3.0e38,
                         torch.finfo(torch.float32).max, -torch.finfo(torch.float32).max], dtype=torch.float32)
    # float16 subnormals: 2^-24 is the smallest; 2^-25 is the tie with zero, 3 * 2^-25 the tie between 2^-24 and 2^-23
    sub = torch.tensor([2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20), 3 * 2.0 ** -25, -3 * 2.0 ** -25, 1.0e-6, -1.0e-6, 6.0e-5,
                        2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12), 1.0e-9, -1.0e-9, 2.0 ** -126], dtype=torch.float32)
    return torch.cat([ties_bf16, ties_f16, misc, sub])


def _cast(src, dst_dtype, n=None):
    n = src.numel() if n is None else n
    sd = src.to(DEV)
    dd = sent((src.numel() + 3,), dst_dtype).to(DEV)
    lib().tc_cast(ptr(sd), ptr(dd), n, TC[src.dtype], TC[dst_dtype], stream())
    torch.cuda.synchronize()
    got = dd.cpu()
    assert bool((got[n:] == SENT).all())                                    # nothing past n
    return got[:n]


def _eq_but_nan(got, want):
    nan = torch.isnan(want.float())
    return torch.equal(torch.isnan(got.float()), nan) and torch.equal(bits(got)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("dst", [torch.bfloat16, torch.float16], ids=_name)
def test_cast_from_float32(dst, capsys):
    """tc_cast float32 -> 16-bit is torch's round-to-nearest-even cast bit for bit: 2 097 159 values (one grid pass is 2 097 152) of
    seeded normals at three scales with the special values at both ends -- exact ties both ways, +-0, +-inf, overflow to inf, values that
    land on float16 subnormals -- and the first 5 alone (the tail).  NaN stays NaN (payload not compared).  float32 SUBNORMAL inputs to
    bfloat16 are printed, not asserted: whether the hardware pair conversion keeps or flushes them is a mode this suite does not pin."""
    n = 2097159
    sp = _special_f32()
    body = torch.from_numpy(seeded_tensor("layout/cast", (n,), 1.0))
    body[n // 3:2 * n // 3] *= 300.0                                        # beyond float16's range in places
    body[2 * n // 3:] *= 1.0e-5                                             # float16 subnormals
    body[:sp.numel()] = sp
    body[-sp.numel():] = sp.flip(0)
    body[100] = float("nan")
    body[-100] = -float("nan")
    assert not bool(((body != 0) & (body.abs() < 2.0 ** -126)).any())       # no float32 subnormals in the asserted set
    assert _eq_but_nan(_cast(body, dst), body.to(dst))
    assert _eq_but_nan(_cast(body, dst, 5), body[:5].to(dst))
    if dst == torch.bfloat16:
        den = _f32([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00400000, 0x80400000, 0x807FFFFF])
        got = _cast(den, dst)
        with capsys.disabled():
            print(f"\n[tc_cast] float32 subnormals {[hex(v & 0xffffffff) for v in bits(den).tolist()]} -> bfloat16 "
                  f"{[hex(v & 0xffff) for v in bits(got).tolist()]} (torch: {[hex(v & 0xffff) for v in bits(den.to(dst)).tolist()]})")


@pytest.mark.parametrize("src", [torch.bfloat16, torch.float16], ids=_name)
def test_cast_to_float32(src):
    """Every one of the 65 536 bit patterns of the 16-bit type, 33 times over (2 162 688 > one grid pass), and the first 5: exact."""
    pat = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(src)
    x = pat.repeat(33)
    assert _eq_but_nan(_cast(x, torch.float32), x.float())
    five = vals("cast5", (5,), src)
    assert same_bits(_cast(five, torch.float32), five.float())


def test_cast_refuses_other_pairs():
    buf = torch.zeros(64, dtype=torch.float32, device=DEV)
    for a, b in ((TC_BF16, TC_F16), (TC_F16, TC_BF16), (TC_F32, TC_F32), (TC_BF16, TC_BF16)):
        with pytest.raises(TcError, match="status -1"):
            lib().tc_cast(ptr(buf), ptr(buf), 8, a, b, stream())


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_argument_refusals():
    """One call per guard the entry points state; each returns TC_ERR_ARG before anything is launched."""
    L, s = lib(), stream()
    buf = torch.zeros(8192, dtype=torch.float32, device=DEV)
    a, b = ptr(buf), ptr(buf, 4096)
    ok_copy = TcEwSeg(EW_COPY, 0, a, b, 0, 0, 8, 8, 1, 1, 8, 0, 0, 0)
    bad = {
        "window_rows: H % ws != 0": lambda: L.tc_window_rows(a, 8, b, 8, 1, 5, 4, 2, 4, 0, 8, 0, 0, TC_F32, s),
        "window_rows: C % 8 != 0": lambda: L.tc_window_rows(a, 12, b, 12, 1, 4, 4, 2, 4, 0, 12, 0, 0, TC_F32, s),
        "window_rows: off + ws*ws > ntw": lambda: L.tc_window_rows(a, 8, b, 8, 1, 4, 4, 2, 5, 2, 8, 0, 0, TC_F32, s),
        "im2col3s2: ldc < 9 Cin": lambda: L.tc_im2col3s2(a, 3, 0, 0, b, 26, 1, 3, 4, 4, TC_F32, s),
        "col2im3s2: lddx < Cin": lambda: L.tc_col2im3s2(a, 32, b, 2, 1, 3, 4, 4, 0, TC_F32, s),
        "stem_im2col: in_ch == 2": lambda: L.tc_stem_im2col(a, b, 148, 1, 2, 4, 4, TC_F32, s),
        "stem_im2col: ldc < 147": lambda: L.tc_stem_im2col(a, b, 146, 1, 3, 4, 4, TC_F32, s),
        "ew_multi: nseg = 0": lambda: L.tc_ew_multi((TcEwSeg * 1)(ok_copy), 0, TC_F32, s),
        "ew_multi: nseg > TC_EW_MULTI_MAX": lambda: L.tc_ew_multi((TcEwSeg * (EW_MULTI_MAX + 1))(*[ok_copy] * (EW_MULTI_MAX + 1)), EW_MULTI_MAX + 1, TC_F32, s),
        "ew_multi: patchify with n1 % n4 != 0": lambda: L.tc_ew_multi((TcEwSeg * 1)(TcEwSeg(EW_PATCHIFY, 0, a, b, 5 * 4 * 8, 0, 8, 0, 1, 5, 4, 8, 2, 0)), 1, TC_F32, s),
    }
    for what, call in bad.items():
        with pytest.raises(TcError, match="status -1"):
            call()
            pytest.fail(what + " was accepted")
    L.tc_ew_multi((TcEwSeg * 1)(ok_copy), 1, TC_F32, s)                      # the segment the refusals reuse is itself a valid one
    torch.cuda.synchronize()
    assert bool((buf == 0).all())

"""tests/dw_ref.py without a GPU.

a. The shift-and-add reference against torch.nn.functional.conv2d (groups = C) and its autograd in float64, on continuous random inputs: every
   k in {3, 5, 7} and stride in {1, 2}, with and without bias and "+ x", on non-square maps including H or W = 1 and H, W < k, and the
   groups / wstride semantics against one conv2d per set.  Both evaluate the same sums, so agreement is to float64 round-off (1e-12 relative to
   the tensor's largest magnitude, the tolerance of tests/test_gate_ref_host.py).
b. chunk_stats and fold against their definitions written as loops.
c. Every case of tests/test_dwconv_abi_gpu.py keeps its own exactness premise (grids, sum|term| / quantum < 2^24, references that are float32
   values), takes the dispatcher branch its list is named after (pick_cg against tc_ffn_chunk, the walker counts against tc_dwconv_bwd_plan) and
   stays below a million elements per operand -- so a bad input list fails here and not on the GPU."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import dw_ref as R

MAPS = [(2, 5, 8), (1, 1, 6), (2, 7, 1), (1, 2, 3), (1, 4, 2), (1, 1, 1), (2, 6, 9)]       # (B, H, W): non-square, H or W = 1, H, W < k
CH = 6


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _same(got, want, what=""):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max()) if got.numel() else 0.0
    assert err <= 1e-12 * max(1.0, float(want.abs().max())), (what, err)


def _torch_conv(x, w, bias, k, stride, add):
    """NHWC in, NHWC out: conv2d with groups = C, padding (k - 1) / 2."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w[:, None], bias, stride=stride, padding=(k - 1) // 2, groups=x.shape[-1]).permute(0, 2, 3, 1)
    return y + x if add else y


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("k", R.KS)
def test_reference_against_conv2d_and_autograd(k, stride):
    for mi, (B, H, W) in enumerate(MAPS):
        for with_bias in (False, True):
            for add in ((False, True) if stride == 1 else (False,)):
                seed = 1000 * k + 100 * stride + 10 * mi
                x, w, b = _rand((B, H, W, CH), seed), _rand((CH, k, k), seed + 1), _rand((CH,), seed + 2)
                xr, wr, br = x.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
                y = _torch_conv(xr, wr, br if with_bias else None, k, stride, add)
                dy = _rand(tuple(y.shape), seed + 3)
                y.backward(dy)
                what = f"k{k} s{stride} {B}x{H}x{W} bias{with_bias} add{add}"
                assert tuple(y.shape[1:3]) == R.out_hw(H, W, k, stride), what
                _same(R.fwd(x, w, b if with_bias else None, k, stride, add), y.detach(), "fwd " + what)
                _same(R.bwd_input(dy, w, H, W, k, stride, add), xr.grad, "bwd_input " + what)
                dw, db = R.bwd_weight(dy, x, k, stride)
                _same(dw[0], wr.grad, "dw " + what)
                if with_bias:
                    _same(db[0], br.grad, "db " + what)
                else:
                    _same(db[0], dy.sum(dim=(0, 1, 2)), "db " + what)


@pytest.mark.parametrize("k", R.KS)
def test_groups_are_stacked_sets_with_their_own_parameters(k):
    G, B, H, W = 3, 2, 4, 5
    x, w, b = _rand((G * B, H, W, CH), k), _rand((G, CH, k, k), k + 1), _rand((G, CH), k + 2)
    dy = _rand((G * B, H, W, CH), k + 3)
    y, dx = R.fwd(x, w, b, k, 1, True, G), R.bwd_input(dy, w, H, W, k, 1, True, G)
    dw, db = R.bwd_weight(dy, x, k, 1, G)
    for g in range(G):
        s = slice(g * B, (g + 1) * B)
        _same(y[s], R.fwd(x[s], w[g], b[g], k, 1, True), f"y of set {g}")
        _same(dx[s], R.bwd_input(dy[s], w[g], H, W, k, 1, True), f"dx of set {g}")
        dwg, dbg = R.bwd_weight(dy[s], x[s], k, 1)
        _same(dw[g], dwg[0], f"dw of set {g}")
        _same(db[g], dbg[0], f"db of set {g}")
    # Params: the blocks of group g stand g * wstride behind group 0's, the fill between them
    p = R.Params("host/p", 5, 3, 9, torch.float32, R.halves, R.SENT)
    assert p.flat.numel() == 2 * 9 + 5 + 2 and bool((p.flat[5:9] == R.SENT).all()) and bool((p.flat[23:] == R.SENT).all())
    want = p.expect_add(torch.ones(3, 5, dtype=torch.float64))
    assert torch.equal(want[9:14], p.flat[9:14].double() + 1) and bool((want[14:18] == R.SENT).all())


def test_chunk_stats_and_fold_are_their_definitions():
    y = _rand((2, 3, 4, 12), 7)
    st = R.chunk_stats(y, 4)
    assert tuple(st.shape) == (2, 3, 4, 3, 2)
    for c in range(3):
        v = y[..., 4 * c:4 * c + 4]
        _same(st[..., c, 0], v.sum(-1), "sum")
        _same(st[..., c, 1], v.var(-1, unbiased=False) * 4, "squared deviations")
    G, chunks, gx, nt, ch, Cc = 2, 2, 5, 10, 4, 6
    part = _rand((G * chunks, gx, nt, ch), 8)
    got = R.fold(part, Cc, 9, ch, chunks, gx, nt, G)
    assert tuple(got.shape) == (G, nt, Cc)
    for g in range(G):
        for t in range(nt):
            for c in range(Cc):
                want = sum(float(part[g * chunks + c // ch, m, t, c % ch]) for m in range(gx))
                assert abs(float(got[g, t, c]) - want) <= 1e-12


def test_buffers_are_poisoned_outside_the_operand():
    m = R.in_map("host/in", 6, 8, 12, torch.bfloat16, lead=4)
    assert m.flat.numel() == 4 + 7 * 12 and not bool(m.logical().isnan().any())
    assert int(m.flat.isnan().sum()) == m.flat.numel() - 6 * 8
    o = R.out_map("host/out", 6, 8, 12, torch.float16, acc=True, lead=4)
    assert int((o.flat == R.SENT).sum()) == o.flat.numel() - 6 * 8
    want = o.expect(torch.ones(6, 8, dtype=torch.float64), accumulate=True)
    assert torch.equal(o.logical(want), o.logical().double() + 1) and int((want == R.SENT).sum()) == o.flat.numel() - 6 * 8


# ---------------------------------------------------------------------------------------------------------------- the GPU file's cases
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
EACH_DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])


@pytest.fixture(scope="module")
def L():
    from transception_amd.build import build
    from transception_amd import _lib
    build(verbose=False)
    return _lib.lib()


def _tc(dtype):
    from transception_amd._lib import TC_BF16, TC_F16, TC_F32
    return {torch.float32: TC_F32, torch.bfloat16: TC_BF16, torch.float16: TC_F16}[dtype]


@EACH_DTYPE
def test_every_gpu_case_keeps_its_exactness_premise(dtype):
    n = 0
    for p in R.all_probs(dtype):
        assert p.premise(), p.tag
        assert max(p.x.flat.numel(), p.dy.flat.numel()) <= 1.0e6, p.tag       # "about a million elements per operand"
        for bias in (False, True):
            for add in ((False, True) if p.stride == 1 else (False,)):
                assert R.is_f32_value(p.ref_fwd(bias, add)), p.tag
        assert R.is_f32_value(p.ref_bwd_input(p.stride == 1)) and all(R.is_f32_value(t) for t in p.ref_bwd_weight()), p.tag
        assert R.is_f32_value(p.dx0(True).expect(p.ref_bwd_input(False), True)), p.tag
        assert R.is_f32_value(p.dw0().expect_add(p.ref_bwd_weight()[0].reshape(p.groups, -1))), p.tag
        n += 1
    assert n >= 100


@EACH_DTYPE
def test_case_lists_reach_the_branches_they_are_named_after(L, dtype):
    from transception_amd._lib import TcDwFold
    vec, tc = R.vec_of(dtype), _tc(dtype)
    for cg in R.CGS:
        Cc = R.c_for_cg(cg, vec)
        assert R.pick_cg(Cc, vec) == cg and int(L.tc_ffn_chunk(Cc, tc)) == cg * vec
    for Cc, cg, chunks, partial in R.chunk_cs(vec):
        assert int(L.tc_ffn_chunk(Cc, tc)) == cg * vec == R.tile_geom(1, 1, 1, Cc, vec)[1]
        assert R.tile_geom(1, 1, 1, Cc, vec)[2] == chunks and (Cc % (cg * vec) != 0) == partial and Cc % vec == 0
    for Cc, _ in R.ffn_cases(vec):
        ch = int(L.tc_ffn_chunk(Cc, tc))
        assert Cc % ch == 0 and ch & (ch - 1) == 0
    for name, (B, H, W, Cc, k, G) in R.walker_cases(vec).items():
        site = TcDwFold()
        nf = int(L.tc_dwconv_bwd_plan(B, H, W, Cc, k, G, tc, C.byref(site)))
        cg, ch, chunks, _, ntiles = R.tile_geom(B, H, W, Cc, vec)
        assert (site.ch, site.chunks, site.nt, site.gx) == (ch, chunks, k * k + 1, R.walkers(B, H, W, Cc, G, vec)), name
        assert nf == chunks * G * site.gx * site.nt * ch
        assert R.walker_premise(name, site.gx, ntiles), (name, site.gx, ntiles)
    for k in R.KS:                                                            # the strip maps: two W-segments that do not divide W; one segment
        (B, H, W, G), (B2, H2, W2, G2) = R.STRIP_MAPS[k][0], R.STRIP_MAPS[k][2]
        n = R.strip_nseg(B, H, W, 16, k, G)
        assert n == 2 and W % n != 0 and R.strip_nseg(B2, H2, W2, 16, k, G2) == 1
        assert R.strip_nseg(*R.STRIP_MAPS[k][1][:3], 16, k, 2) >= 2
    if dtype != torch.float32:                                                # dw_tile_ok is false for the reason the case names, and only that one
        for why, s in R.STRIP_WHY.items():
            p = R.strip_prob(dtype, why, 3, R.STRIP_MAPS[3][0])
            odd = [p.C % 8 != 0, p.ld["x"] % 8 != 0 or p.ld["dy"] % 8 != 0, bool(p.lead)]
            assert sum(odd) == 1 or why == "C=68", why
            assert all(v % 4 == 0 for v in p.ld.values()) and all(v % 4 == 0 for v in p.lead.values())       # 8-byte accesses stay aligned

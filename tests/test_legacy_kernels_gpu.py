"""The gather kernels of the legacy Transception encoder (csrc/legacy.hip) through engine.Graph on the MI355X:
tc_im2col_dil / tc_col2im_dil against F.unfold / F.conv2d and their autograd, tc_nearest_concat_fwd / _bwd against F.interpolate + cat
and theirs.  Gathers must be exact; the adjoints sum in fp32 and round once to the storage type."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _graph(dtype):
    from transception_amd.engine import Graph
    return Graph(dtype, torch.device(DEV), training=True, record=True)


def _var(t):
    from transception_amd.engine import Var
    return Var(t.to(DEV).contiguous())


def _backward(G, out, g):
    r = out.root
    r.grad_t = g.to(DEV).contiguous().view(r.rows, r.cols)
    r.whole_written = True
    G.backward()
    torch.cuda.synchronize()


def _adjoint_tol(dtype):
    return dict(atol=1e-5, rtol=1e-5) if dtype == torch.float32 else dict(atol=1e-2, rtol=1e-2 if dtype == torch.bfloat16 else 2e-3)


# (Cin, H, k, stride, pad, dilation): the dilated 3x3 of dil_conv = 1 (56 -> 26, 28 -> 12, 14 -> 5), the 3x3 of dil_conv = 0, the 1x1 branch
GEOMS = [(64, 56, 3, 2, 0, 2), (128, 28, 3, 2, 0, 2), (320, 14, 3, 2, 0, 2), (64, 56, 3, 2, 1, 1), (128, 28, 1, 2, 0, 1), (320, 14, 1, 2, 0, 1)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geo", GEOMS)
def test_im2col_dil_against_unfold(geo, dtype):
    Cin, H, k, s, p, d = geo
    B = 2
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, Cin, H, H, generator=g).to(dtype)
    G = _graph(dtype)
    xv = _var(x.permute(0, 2, 3, 1).reshape(B * H * H, Cin))
    cols = G.im2col_dil(xv, B, H, H, k, s, p, d)
    Ho = (H + 2 * p - d * (k - 1) - 1) // s + 1
    assert Ho in (26, 12, 5, 28, 14, 7)
    xr = x.float().requires_grad_(True)
    u = F.unfold(xr, k, dilation=d, padding=p, stride=s)                  # [B, Cin*k*k, L], channel-major
    want = u.view(B, Cin, k * k, Ho * Ho).permute(0, 3, 2, 1).reshape(B * Ho * Ho, k * k * Cin)
    assert torch.equal(cols.data.cpu().float(), want.detach())           # a gather: bit for bit
    gy = torch.randn(B * Ho * Ho, k * k * Cin, generator=g).to(dtype)
    _backward(G, cols, gy)
    (want * gy.float()).sum().backward()
    got = G.grad_of(xv).cpu().float().view(B, H, H, Cin).permute(0, 3, 1, 2)
    torch.testing.assert_close(got, xr.grad, **_adjoint_tol(dtype))


@pytest.mark.parametrize("geo", GEOMS[:4])
def test_im2col_dil_product_is_conv2d(geo):
    """The tap-major columns times the permuted [Cout, k*k*Cin] weight (engine.Graph.permuted_weight) equal F.conv2d, gradients included."""
    from transception_amd.engine import P
    Cin, H, k, s, p, d = geo
    B, Cout = 2, 32
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, Cin, H, H, generator=g)
    w = (torch.randn(Cout, Cin, k, k, generator=g) * 0.05)
    G = _graph(torch.float32)
    xv = _var(x.permute(0, 2, 3, 1).reshape(B * H * H, Cin))
    wd, wg = w.to(DEV).contiguous(), torch.zeros(Cout, Cin * k * k, device=DEV)
    Wp = G.permuted_weight(P(wd.view(Cout, Cin * k * k), wg), Cout, Cin, k * k)
    y = G.linear(G.im2col_dil(xv, B, H, H, k, s, p, d), Wp)
    Ho = (H + 2 * p - d * (k - 1) - 1) // s + 1
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    ref = F.conv2d(xr, wr, None, s, p, d)
    torch.testing.assert_close(y.data.cpu().view(B, Ho, Ho, Cout).permute(0, 3, 1, 2), ref.detach(), atol=1e-4, rtol=1e-4)
    gy = torch.randn(B, Cout, Ho, Ho, generator=g)
    _backward(G, y, gy.permute(0, 2, 3, 1).reshape(B * Ho * Ho, Cout))
    (ref * gy).sum().backward()
    torch.testing.assert_close(G.grad_of(xv).cpu().view(B, H, H, Cin).permute(0, 3, 1, 2), xr.grad, atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(wg.cpu().view(Cout, Cin, k, k), wr.grad, atol=1e-3, rtol=1e-4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("branch_major", [True, False])
@pytest.mark.parametrize("grids", [(26, 28, 128), (12, 14, 320), (5, 7, 512), (28, 28, 128)])
def test_nearest_concat_against_interpolate(grids, branch_major, dtype):
    g1, g2, C = grids
    B, n1, n2 = 2, grids[0] ** 2, grids[1] ** 2
    g = torch.Generator().manual_seed(7)
    a = torch.randn(B, n1, C, generator=g).to(dtype)
    b = torch.randn(B, n2, C, generator=g).to(dtype)
    seq = torch.cat([a.reshape(B * n1, C), b.reshape(B * n2, C)]) if branch_major else torch.cat([a, b], 1).reshape(B * (n1 + n2), C)
    G = _graph(dtype)
    sv = _var(seq)
    y = G.nearest_concat(sv, B, g1, g1, g2, g2, branch_major=branch_major)
    ar, br = a.float().requires_grad_(True), b.float().requires_grad_(True)
    m1 = F.interpolate(ar.reshape(B, g1, g1, C).permute(0, 3, 1, 2), [g2, g2])
    m2 = br.reshape(B, g2, g2, C).permute(0, 3, 1, 2)
    want = torch.cat((m1, m2), 1).permute(0, 2, 3, 1).reshape(B * n2, 2 * C)
    assert torch.equal(y.data.cpu().float(), want.detach())
    gy = torch.randn(B * n2, 2 * C, generator=g).to(dtype)
    _backward(G, y, gy)
    (want * gy.float()).sum().backward()
    gs = G.grad_of(sv).cpu().float()
    if branch_major:
        ga, gb = gs[:B * n1].view(B, n1, C), gs[B * n1:].view(B, n2, C)
    else:
        gs = gs.view(B, n1 + n2, C)
        ga, gb = gs[:, :n1], gs[:, n1:]
    torch.testing.assert_close(ga, ar.grad, **_adjoint_tol(dtype))
    assert torch.equal(gb, br.grad)                                      # a copy

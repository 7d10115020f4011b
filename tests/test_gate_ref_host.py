"""The references of tests/gate_ref.py against torch autograd in float64, on continuous random inputs: the formulas that the GPU tests
trust are themselves checked where there is no GPU.  The references and torch evaluate the same expressions, so agreement is to float64
round-off (1e-12 relative to the tensor's largest magnitude).  The first-maximum rule is checked on planted ties against torch's max(dim)
index and the gradient routing of adaptive_max_pool2d."""
import pytest
import torch
import torch.nn.functional as F

import gate_ref as R


def _rand(shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def _same(got, want, what=""):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((got - want).abs().max())
    assert err <= 1e-12 * max(1.0, float(want.abs().max())), (what, err)


def _leaf(t):
    return t.clone().requires_grad_()


def _z(*shape):
    return torch.zeros(*shape, dtype=torch.float64)


ROWS, C = 15, 8


def test_fma3_add_and_the_pointwise_gradients():
    a, b, c, d, g0 = (_rand((ROWS, C), s) for s in range(5))
    ar, br, cr = _leaf(a), _leaf(b), _leaf(c)
    out = 0.3 * ar + br * cr
    out.backward(d)
    _same(R.fma3_fwd_ref(a, b, c, 0.3, _z(ROWS, C)), out.detach(), "fma3")
    da, db, dc = R.fma3_bwd_ref(d, b, c, 0.3, _z(ROWS, C), g0, _z(ROWS, C), db_accumulate=True)
    _same(da, ar.grad, "da")
    _same(db, g0 + br.grad, "db accumulated")
    _same(dc, cr.grad, "dc")
    _same(R.fma3_bwd_ref(d, b, c, 0.3, g0, g0, g0)[1], br.grad, "db written")
    _same(R.add_ref(a, b, _z(ROWS, C)), a + b, "add")
    zr = _leaf(a)
    s = torch.sigmoid(zr)
    s.backward(d)
    _same(R.sigmoid_bwd_ref(d, s.detach(), _z(ROWS, C)), zr.grad, "sigmoid'")
    xr = _leaf(a)
    y = torch.relu(xr)
    y.backward(d)
    _same(R.relu_fwd_ref(a, _z(ROWS, C)), y.detach(), "relu")
    _same(R.relu_bwd_ref(d, y.detach(), _z(ROWS, C)), xr.grad, "relu'")
    xr = _leaf(a * 2)
    F.gelu(xr).backward(d)
    _same(R.gelu_bwd_ref(d, a * 2, _z(ROWS, C)), xr.grad, "gelu'")


def test_outputs_keep_what_the_op_does_not_own():
    """The padded-buffer convention: rows past the end and columns past C keep their values; flat outputs keep their tail."""
    a, b = _rand((ROWS, C), 1), _rand((ROWS, C), 2)
    y0 = _rand((ROWS + 2, C + 4), 3)
    y = R.add_ref(a, b, y0)
    assert torch.equal(y[:ROWS, :C], a + b) and torch.equal(y[ROWS:], y0[ROWS:]) and torch.equal(y[:, C:], y0[:, C:])
    f0 = _rand((ROWS * C + 5,), 4)
    f = R.relu_fwd_ref(a, f0)
    assert torch.equal(f[ROWS * C:], f0[ROWS * C:]) and torch.equal(f[:ROWS * C], a.clamp_min(0).reshape(-1))


def test_gamma_residual():
    a, x, d, g0 = (_rand((ROWS, C), s) for s in range(10, 14))
    gamma = torch.tensor([0.45], dtype=torch.float64)
    ar, xr, gr = _leaf(a), _leaf(x), _leaf(gamma)
    y = gr * ar + xr
    y.backward(d)
    _same(R.gamma_res_fwd_ref(a, x, gamma, _z(ROWS, C)), y.detach(), "y")
    da, dx, dgm = R.gamma_res_bwd_ref(d, a, gamma, _z(ROWS, C), g0, torch.tensor([1.5], dtype=torch.float64), dx_accumulate=True)
    _same(da, ar.grad, "da")
    _same(dx, g0 + xr.grad, "dx")
    _same(dgm, 1.5 + gr.grad, "dgamma")


@pytest.mark.parametrize("B,N", [(2, 7), (3, 1), (1, 16)])
def test_se_block_pool_and_gate(B, N):
    x, d, g0 = (_rand((B * N, C), s) for s in range(20, 23))
    gp, gate = _rand((B, C), 23), _rand((B, C), 24)
    xr = _leaf(x)
    pooled = F.adaptive_avg_pool2d(xr.view(B, N, 1, C).permute(0, 3, 1, 2), 1).view(B, C)
    pooled.backward(gp)
    _same(R.chan_pool_fwd_ref(x, B, N, _z(B, C)), pooled.detach(), "pooled")
    _same(R.chan_pool_bwd_ref(gp, B, N, g0, accumulate=True), g0 + xr.grad, "dx of the pooling")
    xr, ar = _leaf(x), _leaf(gate)
    y = (xr.view(B, N, C) * ar.view(B, 1, C)).reshape(B * N, C)
    y.backward(d)
    _same(R.chan_gate_fwd_ref(x, gate, B, N, _z(B * N, C)), y.detach(), "gated")
    dx, dgate = R.chan_gate_bwd_ref(d, x, gate, B, N, g0, _z(B, C), dx_accumulate=True)
    _same(dx, g0 + xr.grad, "dx of the gate")
    _same(dgate, ar.grad, "dgate")


@pytest.mark.parametrize("B,H,W", [(2, 4, 8), (1, 8, 2), (2, 5, 9), (1, 1, 3)])
def test_coord_pool_and_gate_on_non_square_maps(B, H, W):
    rows = B * H * W
    x, d, g0 = (_rand((rows, C), s) for s in range(30, 33))
    gp, att = _rand((B * (H + W), C), 33), _rand((B * (H + W), C), 34)
    xr = _leaf(x)
    x4 = xr.view(B, H, W, C)
    pooled = torch.cat([x4.mean(dim=2).reshape(B * H, C), x4.mean(dim=1).reshape(B * W, C)], 0)
    pooled.backward(gp)
    _same(R.coord_pool_fwd_ref(x, B, H, W, _z(B * (H + W), C)), pooled.detach(), "pooled")
    _same(R.coord_pool_bwd_ref(gp, B, H, W, g0, accumulate=True), g0 + xr.grad, "dx of the pooling")
    xr, ar = _leaf(x), _leaf(att)
    ah, aw = ar[:B * H].view(B, H, 1, C), ar[B * H:].view(B, 1, W, C)
    y = (xr.view(B, H, W, C) * aw * ah).reshape(rows, C)
    y.backward(d)
    _same(R.coord_gate_fwd_ref(x, att, B, H, W, _z(rows, C)), y.detach(), "gated")
    dx, datt = R.coord_gate_bwd_ref(d, x, att, B, H, W, g0, _z(B * (H + W), C), dx_accumulate=True)
    _same(dx, g0 + xr.grad, "dx of the gate")
    _same(datt, ar.grad, "datt")


@pytest.mark.parametrize("B,H,W,p,c", [(2, 3, 5, 4, 8), (1, 2, 2, 2, 4)])
def test_pixel_shuffle_and_transpose(B, H, W, p, c):
    n = B * H * W * p * p * c
    x = _rand((n,), 40)
    # the kernel's channel order is (p1 p + p2) c + cc (torch's pixel_shuffle has cc p p + p1 p + p2): restated with explicit loops
    fine = torch.zeros(B, H * p, W * p, c, dtype=torch.float64)
    coarse = x.view(B, H, W, p * p * c)
    for p1 in range(p):
        for p2 in range(p):
            fine[:, p1::p, p2::p, :] = coarse[..., (p1 * p + p2) * c:(p1 * p + p2 + 1) * c]
    out0 = _rand((n + 3,), 41)
    got = R.pixel_shuffle_ref(x, out0, B, H, W, p, c)
    assert torch.equal(got[:n], fine.reshape(-1)) and torch.equal(got[n:], out0[n:])
    assert torch.equal(R.pixel_shuffle_ref(got[:n], out0, B, H, W, p, c, inverse=True)[:n], x)
    nb, Rr, Cc = 3, 5, 7
    s = _rand((nb * Rr * Cc,), 42)
    t = R.transpose_ref(s, _z(nb * Rr * Cc + 2), nb, Rr, Cc)
    assert torch.equal(t[:-2].view(nb, Cc, Rr), s.view(nb, Rr, Cc).transpose(1, 2)) and bool((t[-2:] == 0).all())


@pytest.mark.parametrize("B,H,W", [(2, 5, 9), (1, 3, 3)])
@pytest.mark.parametrize("k", [3, 7])
def test_cbam_pieces(B, H, W, k):
    N, rows = H * W, B * H * W
    x, d, g0 = (_rand((rows, C), s) for s in range(50, 53))
    gp = _rand((2 * B, C), 53)
    xr = _leaf(x)
    x4 = xr.view(B, H, W, C).permute(0, 3, 1, 2)
    mx, av = F.adaptive_max_pool2d(x4, 1).view(B, C), F.adaptive_avg_pool2d(x4, 1).view(B, C)
    (torch.cat([mx, av], 0) * gp).sum().backward()
    pooled, idx = R.chan_pool2_fwd_ref(x, B, N, _z(2 * B, C), torch.zeros(B, C, dtype=torch.int32))
    _same(pooled, torch.cat([mx, av], 0).detach(), "max | mean pooling")
    assert torch.equal(idx.long(), x.view(B, N, C).max(dim=1)[1])
    _same(R.chan_pool2_bwd_ref(gp, idx, B, N, g0, accumulate=True), g0 + xr.grad, "pooling gradient")
    # statistics -> convolution -> sigmoid -> gate
    w, b = _rand((1, 2, k, k), 54, 0.3), _rand((1,), 55, 0.1)
    xr, wr, br = _leaf(x), _leaf(w), _leaf(b)
    x4 = xr.view(B, H, W, C).permute(0, 3, 1, 2)
    st = torch.cat([x4.max(dim=1, keepdim=True)[0], x4.mean(dim=1, keepdim=True)], 1)
    st.retain_grad()
    pre = F.conv2d(st, wr, br, padding=k // 2)
    sa = torch.sigmoid(pre)
    sa.retain_grad()
    y = (x4 * sa).permute(0, 2, 3, 1).reshape(rows, C)
    y.backward(d)
    st_ref, ix = R.pix_stats_fwd_ref(x, _z(rows, 2), torch.zeros(rows, dtype=torch.int32))
    st_tok = st.detach().permute(0, 2, 3, 1).reshape(rows, 2)
    _same(st_ref, st_tok, "channel max | mean")
    assert torch.equal(ix.long(), x.max(dim=1)[1])
    _same(R.sa_conv_pre_ref(st_tok, w, b, B, H, W, k), pre.detach().reshape(-1), "pre-activation")
    g = R.sa_conv_fwd_ref(st_tok, w, b, B, H, W, k, _z(rows))
    _same(g, sa.detach().reshape(-1), "spatial attention")
    _same(R.pix_gate_fwd_ref(x, g, _z(rows, C)), y.detach(), "gated map")
    dxg, dg = R.pix_gate_bwd_ref(d, x, g, _z(rows, C), _z(rows))
    _same(dg, sa.grad.reshape(-1), "dg")
    dst, dw, db = R.sa_conv_bwd_ref(dg, g, st_tok, w, B, H, W, k, _z(rows, 2), _rand((2 * k * k,), 56), torch.tensor([0.25], dtype=torch.float64))
    _same(dst, st.grad.permute(0, 2, 3, 1).reshape(rows, 2), "dst")
    _same(dw, _rand((2 * k * k,), 56) + wr.grad.reshape(-1), "dw accumulated")
    _same(db, 0.25 + br.grad, "db accumulated")
    _same(R.pix_stats_bwd_ref(dst, ix, C, dxg, accumulate=True), xr.grad, "dx through gate, statistics and convolution")


@pytest.mark.parametrize("B,N,Cc", [(2, 37, 8), (1, 5, 4), (3, 1, 4)])
def test_cam_module(B, N, Cc):
    """softmax(max - E), y, dx and dgamma against autograd; the backward takes the forward's att, as the ABI does."""
    rows = B * N
    x, d, g0 = _rand((rows, 4 * Cc), 60, 0.5), _rand((rows, 4 * Cc), 61), _rand((rows, 4 * Cc), 62)
    gamma = torch.tensor([0.45], dtype=torch.float64)
    xr, gr = _leaf(x), _leaf(gamma)
    x5 = xr.view(B, N, 4, Cc).permute(0, 3, 2, 1)                           # [B, C, 4, N]
    energy = x5 @ x5.transpose(-1, -2)
    att = torch.softmax(energy.max(-1, keepdim=True)[0] - energy, -1)
    y = (gr * (att @ x5) + x5).permute(0, 3, 2, 1).reshape(rows, 4 * Cc)
    y.backward(d)
    _same(R.cam_energy_ref(x, B, N), energy.detach(), "energy")
    a = R.cam_att_fwd_ref(x, B, N, _z(B * Cc * 16 + 3))
    assert bool((a[-3:] == 0).all())
    _same(a[:-3].view(B, Cc, 4, 4), att.detach(), "att")
    _same(R.cam_apply_fwd_ref(x, a, gamma, B, N, _z(rows, 4 * Cc)), y.detach(), "y")
    att2, dgm, dx = R.cam_bwd_ref(x, d, a, gamma, B, N, _z(B * Cc * 16), torch.tensor([2.0], dtype=torch.float64), g0, dx_accumulate=True)
    _same(dx, g0 + xr.grad, "dx")
    _same(dgm, 2.0 + gr.grad, "dgamma")
    G = att2.view(B, Cc, 4, 4)
    assert torch.equal(G, G.transpose(-1, -2))                               # dE + dE^T


def test_first_maximum_on_planted_ties():
    """Ties: the value and the first index, as torch's max(dim), and the gradient goes to that one position, as adaptive_max_pool2d's."""
    B, N, Cc = 2, 20, 8
    x = (_rand((B * N, Cc), 70) * 2).round() / 2
    x = x.clamp(-1.5, 1.5)
    x3 = x.view(B, N, Cc)
    x3[:, 0, 0] = x3[:, N - 1, 0] = 2.0                                      # first and last
    x3[:, N - 1, 1] = 2.0                                                    # last only
    x3[:, 5, 2] = x3[:, 6, 2] = 2.0
    x3[:, 17, 3] = x3[:, 2, 3] = 2.0
    x3[:, :, 4] = 1.0                                                        # all equal
    x3[:, :, 5] = -x3[:, :, 5].abs() - 0.5
    x3[:, 3, 5], x3[:, 9, 5] = -0.0, 0.0                                     # the maximum is zero, both signs present
    pooled, idx = R.chan_pool2_fwd_ref(x, B, N, _z(2 * B, Cc), torch.full((B, Cc), -7, dtype=torch.int32))
    assert idx[:, :6].tolist() == [[0, N - 1, 5, 2, 0, 3]] * B
    xr = _leaf(x)
    mx = F.adaptive_max_pool2d(xr.view(B, N, 1, Cc).permute(0, 3, 1, 2), 1).view(B, Cc)
    gp = _rand((2 * B, Cc), 71)
    gp[B:] = 0                                                               # the max half alone
    (mx * gp[:B]).sum().backward()
    assert torch.equal(pooled[:B], mx.detach())
    assert torch.equal(idx.long(), x3.max(dim=1)[1])
    _same(R.chan_pool2_bwd_ref(gp, idx, B, N, _z(B * N, Cc)), xr.grad, "routing")
    dx = R.chan_pool2_bwd_ref(gp, idx, B, N, _z(B * N, Cc)).view(B, N, Cc)
    assert bool(((dx != 0).sum(dim=1) <= 1).all()) and torch.equal(dx.sum(dim=1), gp[:B])
    # per token over the channels
    rows = 6
    t = ((_rand((rows, 16), 72) * 2).round() / 2).clamp(-1.5, 1.5)
    t[0, 0] = t[0, 15] = 2.0
    t[1, 15] = 2.0
    t[2, 5] = t[2, 6] = 2.0
    t[3, 9] = t[3, 14] = 2.0
    t[4] = 0.5
    t[5] = -t[5].abs() - 0.5
    t[5, 7], t[5, 2] = 0.0, -0.0
    st, ix = R.pix_stats_fwd_ref(t, _z(rows, 2), torch.zeros(rows, dtype=torch.int32))
    assert ix.tolist() == [0, 15, 5, 9, 0, 2]
    tv, ti = t.max(dim=1)
    assert torch.equal(st[:, 0], tv) and torch.equal(ix.long(), ti)
    dst = _rand((rows, 2), 73)
    dst[:, 1] = 0
    dxt = R.pix_stats_bwd_ref(dst, ix, 16, _z(rows, 16))
    assert bool(((dxt != 0).sum(dim=1) <= 1).all()) and torch.equal(dxt[torch.arange(rows), ix.long()], dst[:, 0])

"""Host references of the gate, pooling and aggregate kernels: all of csrc/cbam.hip and the arithmetic half of csrc/elementwise.hip, one
function per C-ABI entry point, in float64 on CPU tensors.  Each is written as the definition in include/transception_hip.h (tensor
expressions over the [B, N, C] / [B, H, W, C] views), not as the kernel's loop; tests/test_gate_ref_host.py checks them against torch autograd.

Conventions.  A token map is a [rows, C] tensor (a column slice of a wider buffer is fine: the references only index it).  An entry point
that writes through a row stride takes the WHOLE output buffer as it is before the call ([rows + spare, ld]) and returns the whole buffer
expected afterwards, in float64: the op owns rows 0 : rows and columns 0 : C, everything else stays, `accumulate` adds to what was there.
fp32 side outputs (dw, db, dgamma, att2) and index arrays follow the same rule.  The two pure moves (pixel shuffle, transpose) keep the
storage type, so that a caller may compare bits.  Maxima return the value and the FIRST maximal index (numpy.argmax's documented rule)."""
import math

import numpy as np
import torch


def _place(out0: torch.Tensor, val: torch.Tensor, accumulate=False) -> torch.Tensor:
    """out0 (any float type) as float64 with val written to, or added into, its leading rows and columns."""
    out = out0.double().clone()
    r, c = val.shape
    out[:r, :c] = out[:r, :c] + val if accumulate else val
    return out


def _place_flat(out0: torch.Tensor, val: torch.Tensor) -> torch.Tensor:
    out = out0.double().clone().view(-1)
    out[:val.numel()] = val.reshape(-1)
    return out.view(out0.shape)


# ---------------------------------------------------------------------------------------------------------------- elementwise
def fma3_fwd_ref(a, b, c, alpha, out0):
    """tc_fma3_fwd: out = alpha a + b c."""
    return _place(out0, alpha * a.double() + b.double() * c.double())


def fma3_bwd_ref(dout, b, c, alpha, da0, db0, dc0, db_accumulate=False):
    """tc_fma3_bwd: da = alpha dout; db (+)= dout c; dc = dout b."""
    d = dout.double()
    return _place(da0, alpha * d), _place(db0, d * c.double(), db_accumulate), _place(dc0, d * b.double())


def add_ref(a, b, y0):
    """tc_add: y = a + b."""
    return _place(y0, a.double() + b.double())


def sigmoid_bwd_ref(dy, s, dz0):
    """tc_sigmoid_bwd: dz = dy s (1 - s) on the first dy.numel() elements."""
    s = s.double()
    return _place_flat(dz0, dy.double() * s * (1.0 - s))


def relu_fwd_ref(x, y0):
    """tc_relu_fwd: y = max(x, 0)."""
    return _place_flat(y0, x.double().clamp_min(0.0))


def relu_bwd_ref(dy, y, dz0):
    """tc_relu_bwd: dz = dy where y > 0, else 0."""
    return _place_flat(dz0, torch.where(y.double() > 0, dy.double(), torch.zeros((), dtype=torch.float64)))


def gelu_bwd_ref(dy, x, dz0):
    """tc_gelu_bwd: dz = dy GELU'(x), GELU'(x) = Phi(x) + x phi(x) (erf form)."""
    x = x.double()
    grad = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return _place_flat(dz0, dy.double() * grad)


def gamma_res_fwd_ref(a, x, gamma, y0):
    """tc_gamma_res_fwd: y = gamma a + x."""
    return _place(y0, float(gamma) * a.double() + x.double())


def gamma_res_bwd_ref(dy, a, gamma, da0, dx0, dgamma0, dx_accumulate=False):
    """tc_gamma_res_bwd: da = gamma dy; dx (+)= dy; dgamma += sum dy a.  Returns (da, dx, dgamma)."""
    d = dy.double()
    return _place(da0, float(gamma) * d), _place(dx0, d, dx_accumulate), dgamma0.double() + (d * a.double()).sum()


# ---------------------------------------------------------------------------------------------------------------- SE_Block
def chan_pool_fwd_ref(x, B, N, pooled0):
    """tc_chan_pool_fwd: pooled[b, c] = mean over the image's N rows."""
    return _place(pooled0, x.double().reshape(B, N, -1).mean(dim=1))


def chan_pool_bwd_ref(dpooled, B, N, dx0, accumulate=False):
    """tc_chan_pool_bwd: dx[b, n, c] (+)= dpooled[b, c] / N."""
    g = dpooled.double()[:B] / N
    return _place(dx0, g[:, None, :].expand(B, N, g.shape[1]).reshape(B * N, -1), accumulate)


def chan_gate_fwd_ref(x, gate, B, N, y0):
    """tc_chan_gate_fwd: y[b, n, c] = x[b, n, c] gate[b, c]."""
    C = x.shape[1]
    return _place(y0, (x.double().reshape(B, N, C) * gate.double()[:B, None, :]).reshape(B * N, C))


def chan_gate_bwd_ref(dy, x, gate, B, N, dx0, dgate0, dx_accumulate=False):
    """tc_chan_gate_bwd: dx (+)= dy gate; dgate[b, c] = sum_n dy x.  Returns (dx, dgate)."""
    C = x.shape[1]
    d = dy.double().reshape(B, N, C)
    dx = (d * gate.double()[:B, None, :]).reshape(B * N, C)
    return _place(dx0, dx, dx_accumulate), _place(dgate0, (d * x.double().reshape(B, N, C)).sum(dim=1))


# ---------------------------------------------------------------------------------------------------------------- CoordAtt
def _coord_rows(ph, pw, B, H, W):
    """[B, H, C] and [B, W, C] -> the pooled / att row order: B*H rows (b, h), then B*W rows (b, w)."""
    C = ph.shape[-1]
    return torch.cat([ph.reshape(B * H, C), pw.reshape(B * W, C)], 0)


def _coord_split(t, B, H, W):
    C = t.shape[1]
    t = t.double()
    return t[:B * H].reshape(B, H, 1, C), t[B * H:B * (H + W)].reshape(B, 1, W, C)


def coord_pool_fwd_ref(x, B, H, W, pooled0):
    """tc_coord_pool_fwd: rows (b, h) = mean over w, then rows (b, w) = mean over h."""
    x4 = x.double().reshape(B, H, W, -1)
    return _place(pooled0, _coord_rows(x4.mean(dim=2), x4.mean(dim=1), B, H, W))


def coord_pool_bwd_ref(dpooled, B, H, W, dx0, accumulate=False):
    """tc_coord_pool_bwd: dx[b, h, w] (+)= dpooled[(b, h)] / W + dpooled[(b, w)] / H."""
    gh, gw = _coord_split(dpooled, B, H, W)
    return _place(dx0, (gh / W + gw / H).reshape(B * H * W, -1), accumulate)


def coord_gate_fwd_ref(x, att, B, H, W, y0):
    """tc_coord_gate_fwd: y[b, h, w] = x[b, h, w] a_w[b, w] a_h[b, h]."""
    ah, aw = _coord_split(att, B, H, W)
    return _place(y0, (x.double().reshape(B, H, W, -1) * aw * ah).reshape(B * H * W, -1))


def coord_gate_bwd_ref(dy, x, att, B, H, W, dx0, datt0, dx_accumulate=False):
    """tc_coord_gate_bwd: dx (+)= dy a_w a_h; datt[(b, h)] = sum_w dy x a_w; datt[(b, w)] = sum_h dy x a_h.  Returns (dx, datt)."""
    ah, aw = _coord_split(att, B, H, W)
    d = dy.double().reshape(B, H, W, -1)
    dx = (d * aw * ah).reshape(B * H * W, -1)
    dxv = d * x.double().reshape(B, H, W, -1)
    datt = _coord_rows((dxv * aw).sum(dim=2), (dxv * ah).sum(dim=1), B, H, W)
    return _place(dx0, dx, dx_accumulate), _place(datt0, datt)


# ---------------------------------------------------------------------------------------------------------------- pure moves
def pixel_shuffle_ref(inp, out0, B, H, W, p, c, inverse=False):
    """tc_pixel_shuffle: coarse pixel (b, h, w), channel (p1 p + p2) c + cc  <->  fine pixel (b, h p + p1, w p + p2), channel cc.
    Flat buffers in the storage type; the elements past the map stay."""
    n = B * H * W * p * p * c
    out = out0.clone().view(-1)
    src = inp.reshape(-1)[:n]
    if not inverse:
        out[:n] = src.view(B, H, W, p, p, c).permute(0, 1, 3, 2, 4, 5).reshape(-1)
    else:
        out[:n] = src.view(B, H, p, W, p, c).permute(0, 1, 3, 2, 4, 5).reshape(-1)
    return out.view(out0.shape)


def transpose_ref(src, dst0, nb, R, C):
    """tc_transpose: dst[b, c, r] = src[b, r, c] (storage type, flat buffers)."""
    n = nb * R * C
    out = dst0.clone().view(-1)
    out[:n] = src.reshape(-1)[:n].view(nb, R, C).transpose(1, 2).reshape(-1)
    return out.view(dst0.shape)


# ---------------------------------------------------------------------------------------------------------------- CBAMBlock
def _first_max(t: torch.Tensor, axis: int):
    """(max, first maximal index) along axis: numpy.argmax returns the first occurrence."""
    a = t.double().numpy()
    i = np.argmax(a, axis=axis)
    return torch.from_numpy(np.take_along_axis(a, np.expand_dims(i, axis), axis).squeeze(axis)), torch.from_numpy(i.astype(np.int32))


def chan_pool2_fwd_ref(x, B, N, pooled0, idx0):
    """tc_chan_pool2_fwd: pooled rows 0..B-1 = max over the image's N rows, idx[b, c] = the first maximal row; rows B..2B-1 = mean.
    Returns (pooled, idx)."""
    x3 = x.double().reshape(B, N, -1)
    mx, ix = _first_max(x3, 1)
    idx = idx0.clone()
    idx[:B, :ix.shape[1]] = ix
    return _place(pooled0, torch.cat([mx, x3.mean(dim=1)], 0)), idx


def chan_pool2_bwd_ref(dpooled, idx, B, N, dx0, accumulate=False):
    """tc_chan_pool2_bwd: dx[b, n, c] (+)= (n == idx[b, c] ? dpooled[b, c] : 0) + dpooled[B + b, c] / N."""
    g = dpooled.double()
    C = g.shape[1]
    hit = torch.arange(N).view(1, N, 1) == idx[:B, :C].long().view(B, 1, C)
    dx = hit.double() * g[:B, None, :] + g[B:2 * B, None, :] / N
    return _place(dx0, dx.reshape(B * N, C), accumulate)


def pix_stats_fwd_ref(x, st0, idx0):
    """tc_pix_stats_fwd: st[row] = (max over the channels, mean over them), idx[row] = the first maximal channel.  Returns (st, idx)."""
    mx, ix = _first_max(x, 1)
    idx = idx0.clone()
    idx[:ix.shape[0]] = ix
    return _place(st0, torch.stack([mx, x.double().mean(dim=1)], 1)), idx


def pix_stats_bwd_ref(dst, idx, C, dx0, accumulate=False):
    """tc_pix_stats_bwd: dx[r, c] (+)= dst[r, 1] / C + (c == idx[r] ? dst[r, 0] : 0)."""
    g = dst.double()
    rows = g.shape[0]
    hit = torch.arange(C).view(1, C) == idx[:rows].long().view(rows, 1)
    return _place(dx0, hit.double() * g[:, :1] + g[:, 1:2] / C, accumulate)


def _shifted(t, dy, dx):
    """t [B, H, W, ...] -> s with s[b, y, x] = t[b, y + dy, x + dx], zero outside the map."""
    B, H, W = t.shape[:3]
    out = torch.zeros_like(t)
    ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[:, ys:ye, xs:xe] = t[:, ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def sa_conv_pre_ref(st, w, bias, B, H, W, k):
    """The pre-activation of tc_sa_conv_fwd: bias + sum_{ch, ky, kx} w[ch][ky][kx] st[b, y + ky - P, x + kx - P, ch], zero padding.  [B*H*W]."""
    s4, wv, P = st.double().reshape(B, H, W, 2), w.double().reshape(2, k, k), k // 2
    z = torch.full((B, H, W), float(bias.double().reshape(-1)[0]), dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            sh = _shifted(s4, ky - P, kx - P)
            z = z + wv[0, ky, kx] * sh[..., 0] + wv[1, ky, kx] * sh[..., 1]
    return z.reshape(-1)


def sa_conv_fwd_ref(st, w, bias, B, H, W, k, g0):
    """tc_sa_conv_fwd: g = sigmoid(Conv2d(2 -> 1, k x k, padding k / 2)(st)) over the [B, H, W] token grid."""
    return _place_flat(g0, torch.sigmoid(sa_conv_pre_ref(st, w, bias, B, H, W, k)))


def sa_conv_bwd_ref(dg, g, st, w, B, H, W, k, dst0, dw0, db0):
    """tc_sa_conv_bwd from the stored gate g: dz = dg g (1 - g); dst[b, y, x, ch] = sum_taps w[ch][ky][kx] dz[b, y - ky + P, x - kx + P];
    dw[ch][ky][kx] += sum_p dz[p] st[p + tap]; db += sum dz.  Returns (dst, dw, db)."""
    n, P = B * H * W, k // 2
    gd = g.double().reshape(-1)[:n]
    dz = (dg.double().reshape(-1)[:n] * gd * (1.0 - gd)).reshape(B, H, W)
    s4, wv = st.double().reshape(-1)[:2 * n].reshape(B, H, W, 2), w.double().reshape(2, k, k)
    dst = torch.zeros(B, H, W, 2, dtype=torch.float64)
    dw = torch.zeros(2, k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            back = _shifted(dz, P - ky, P - kx)
            dst[..., 0] += wv[0, ky, kx] * back
            dst[..., 1] += wv[1, ky, kx] * back
            dw[:, ky, kx] = (dz[..., None] * _shifted(s4, ky - P, kx - P)).sum(dim=(0, 1, 2))
    return _place_flat(dst0, dst), dw0.double() + dw.reshape(dw0.shape), db0.double() + dz.sum()


def pix_gate_fwd_ref(x, g, y0):
    """tc_pix_gate_fwd: y[r, c] = x[r, c] g[r]."""
    return _place(y0, x.double() * g.double().reshape(-1)[:x.shape[0], None])


def pix_gate_bwd_ref(dy, x, g, dx0, dg0, dx_accumulate=False):
    """tc_pix_gate_bwd: dx (+)= dy g[r]; dg[r] = sum_c dy x.  Returns (dx, dg)."""
    d = dy.double()
    return _place(dx0, d * g.double().reshape(-1)[:d.shape[0], None], dx_accumulate), _place_flat(dg0, (d * x.double()).sum(dim=1))


# ---------------------------------------------------------------------------------------------------------------- CAM_Module
def _paths(x, B, N):
    """[B*N, 4C] (column p C + c) -> [B, N, 4, C] float64."""
    return x.double().reshape(B, N, 4, -1)


def cam_energy_ref(x, B, N):
    """E[b, c, p, q] = sum_n x[n, p] x[n, q]."""
    x4 = _paths(x, B, N)
    return torch.stack([torch.stack([(x4[:, :, p] * x4[:, :, q]).sum(dim=1) for q in range(4)], -1) for p in range(4)], -2)


def cam_att_fwd_ref(x, B, N, att0):
    """tc_cam_att_fwd: att[b, c, p, :] = softmax_q(max_q E[p, :] - E[p, q]), fp32 [B][C][16]."""
    E = cam_energy_ref(x, B, N)
    return _place_flat(att0, torch.softmax(E.max(dim=-1, keepdim=True)[0] - E, dim=-1))


def cam_apply_fwd_ref(x, att, gamma, B, N, y0):
    """tc_cam_apply_fwd from a given att: y[n, p] = gamma sum_q A[p][q] x[n, q] + x[n, p]."""
    x4 = _paths(x, B, N)
    C = x4.shape[-1]
    A = att.double().reshape(-1)[:B * C * 16].reshape(B, 1, C, 4, 4)
    y = torch.stack([float(gamma) * sum(A[..., p, q] * x4[:, :, q] for q in range(4)) + x4[:, :, p] for p in range(4)], 2)
    return _place(y0, y.reshape(B * N, 4 * C))


def cam_bwd_ref(x, dy, att, gamma, B, N, att2_0, dgamma0, dx0, dx_accumulate=False):
    """tc_cam_bwd from a given att A: dA[p][q] = gamma sum_n dy[n, p] x[n, q]; dEn = A (.) (dA - rowsum(A (.) dA)); dE = -dEn;
    G = dE + dE^T (att2); dx[n, p] (+)= dy[n, p] + gamma sum_q A[q][p] dy[n, q] + sum_q G[p][q] x[n, q]; dgamma += sum dy (.) (A x).
    Returns (att2, dgamma, dx)."""
    x4, d4, gm = _paths(x, B, N), _paths(dy, B, N), float(gamma)
    C = x4.shape[-1]
    A = att.double().reshape(-1)[:B * C * 16].reshape(B, C, 4, 4)
    dA = gm * torch.stack([torch.stack([(d4[:, :, p] * x4[:, :, q]).sum(dim=1) for q in range(4)], -1) for p in range(4)], -2)
    dE = -A * (dA - (A * dA).sum(dim=-1, keepdim=True))
    G = dE + dE.transpose(-1, -2)
    Ab, Gb = A[:, None], G[:, None]
    dx = torch.stack([d4[:, :, p] + gm * sum(Ab[..., q, p] * d4[:, :, q] for q in range(4)) + sum(Gb[..., p, q] * x4[:, :, q] for q in range(4))
                      for p in range(4)], 2)
    ax = torch.stack([sum(Ab[..., p, q] * x4[:, :, q] for q in range(4)) for p in range(4)], 2)
    return _place_flat(att2_0, G), dgamma0.double() + (d4 * ax).sum(), _place(dx0, dx.reshape(B * N, 4 * C), dx_accumulate)

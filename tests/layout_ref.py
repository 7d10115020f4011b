"""Host references of the layout moves in csrc/elementwise.hip and of the SGD update in csrc/train.hip, written with torch library calls
only (tests/test_layout_ref_host.py checks each of them against a nested-loop restatement of the formula in include/transception_hip.h).

Every layout reference moves values without arithmetic (or, for the adjoints, sums them in float64), so a caller may compare bit patterns
of the forward moves and exact values of the accumulating ones.  Token-major maps are [B*H*W, C] matrices."""
import math

import torch
import torch.nn.functional as F


def tokens_to_nchw(x: torch.Tensor, B: int, H: int, W: int) -> torch.Tensor:
    return x.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def nchw_to_tokens(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _unfold(x: torch.Tensor, k: int, stride: int, pad: int) -> torch.Tensor:
    """[B, C, H, W] -> [B*Ho*Wo, C*k*k], column c*k*k + ky*k + kx; evaluated in float64 (a superset of every storage type) and cast back."""
    B = x.shape[0]
    u = F.unfold(x.double(), k, stride=stride, padding=pad)                  # [B, C*k*k, L]
    return u.transpose(1, 2).reshape(B * u.shape[2], u.shape[1]).to(x.dtype)


def im2col3s2_ref(x_nchw: torch.Tensor, Cin: int = None) -> torch.Tensor:
    """tc_im2col3s2: [B*Ho*Wo, 9*Cin] with column c*9 + ky*3 + kx = x(b, 2 oy + ky - 1, 2 ox + kx - 1, c), zero outside the map.  An image
    with one channel feeds all Cin channels (src_ch == 1)."""
    B, Cs, H, W = x_nchw.shape
    if Cin is not None and Cs == 1 and Cin != 1:
        x_nchw = x_nchw.expand(B, Cin, H, W)
    return _unfold(x_nchw, 3, 2, 1)


def col2im3s2_ref(d: torch.Tensor, B: int, C: int, H: int, W: int) -> torch.Tensor:
    """tc_col2im3s2 (the adjoint of im2col3s2_ref): d [B*Ho*Wo, 9*C] -> the float64 token-major gradient [B*H*W, C]."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = F.fold(d.double().reshape(B, Ho * Wo, 9 * C).transpose(1, 2), (H, W), 3, stride=2, padding=1)
    return nchw_to_tokens(y)


def stem_im2col_ref(img: torch.Tensor) -> torch.Tensor:
    """tc_stem_im2col: NCHW image with 3 channels, or 1 channel repeated three times -> [B*Ho*Wo, 148], column ci*49 + ky*7 + kx of the
    7 x 7 stride-4 pad-3 patches; column 147 is zero."""
    B, Cs, H, W = img.shape
    img3 = img.expand(B, 3, H, W) if Cs == 1 else img
    u = _unfold(img3, 7, 4, 3)
    return torch.cat([u, torch.zeros(u.shape[0], 1, dtype=u.dtype)], dim=1)


def window_partition_ref(src: torch.Tensor, B: int, H: int, W: int, ws: int) -> torch.Tensor:
    """Token map [B*H*W, C] -> [B*(H/ws)*(W/ws), ws*ws, C]: pixel (b, wy ws + iy, wx ws + ix) is token iy ws + ix of window (b, wy, wx)."""
    C = src.shape[1]
    return src.reshape(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B * (H // ws) * (W // ws), ws * ws, C)


def window_reverse_ref(win: torch.Tensor, B: int, H: int, W: int, ws: int) -> torch.Tensor:
    """The inverse permutation: [B*(H/ws)*(W/ws), ws*ws, C] -> token map [B*H*W, C]."""
    C = win.shape[2]
    return win.reshape(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B * H * W, C)


def window_rows_ref(src: torch.Tensor, dst: torch.Tensor, B: int, H: int, W: int, ws: int, ntw: int, off: int, to_map: bool,
                    accumulate: bool = False) -> torch.Tensor:
    """tc_window_rows on host copies: dir 0 places the map's pixels at rows off : off + ws*ws of each window's ntw rows of dst (every other
    row of dst stays), dir 1 gathers those rows into the map.  accumulate adds in float64 and returns float64."""
    nwin = B * (H // ws) * (W // ws)
    out = (dst.double() if accumulate else dst).clone().contiguous()
    if not to_map:
        part = window_partition_ref(src[:B * H * W], B, H, W, ws)
        v = out[:nwin * ntw].view(nwin, ntw, -1)
        v[:, off:off + ws * ws] = v[:, off:off + ws * ws] + part.double() if accumulate else part
    else:
        part = window_reverse_ref(src[:nwin * ntw].reshape(nwin, ntw, -1)[:, off:off + ws * ws], B, H, W, ws)
        out[:B * H * W] = out[:B * H * W] + part.double() if accumulate else part
    return out


def clip_coef(sumsq: float, clip: float) -> float:
    """clip_grad_norm_'s coefficient min(clip / (norm + 1e-6), 1), from the squared norm of the gradients AS STORED (tc_grad_sumsq): the
    kernels clip the stored gradients and apply gscale to the result, so a caller that scales folds 1 / gscale into clip."""
    return min(clip / (math.sqrt(sumsq) + 1e-6), 1.0)


def sgd_ref(w, g, m, lr, mom, wd, gscale=1.0, first=False, coef=1.0):
    """The update of tc_sgd_step / tc_sgd_step_multi in float64: d = g gscale coef + wd w; b = d (first) or mom m + d; w' = w - lr b.
    Returns (w', b, A) with A = |g gscale coef| + |wd w| + |mom m|, the magnitude the derived error bounds are stated in."""
    w, g, m = w.double(), g.double(), m.double()
    t = g * (gscale * coef)
    d = t + wd * w
    b = d if first else mom * m + d
    A = t.abs() + (wd * w).abs() + (0.0 if first else (mom * m).abs())
    return w - lr * b, b, A


def sgd_torch_ref(w, g, m, lr, mom, wd, gscale=1.0, first=False, clip=math.inf):
    """The same step by float64 torch.optim.SGD: torch.nn.utils.clip_grad_norm_(clip) on the stored gradient g, the result times gscale,
    then the optimizer's step.  Returns (w', b)."""
    p = torch.nn.Parameter(w.double().clone())
    p.grad = g.double().clone()
    opt = torch.optim.SGD([p], lr=lr, momentum=mom, weight_decay=wd)
    if not first:
        opt.state[p]["momentum_buffer"] = m.double().clone()
    if clip != math.inf:
        torch.nn.utils.clip_grad_norm_([p], clip)
    p.grad.mul_(gscale)
    opt.step()
    return p.detach(), opt.state[p]["momentum_buffer"].clone()

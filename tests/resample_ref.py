"""The definition of include/transception_resample.h in float64: bilinear, align_corners=False, no antialiasing, with rational coordinates.

For output coordinate o of `out` positions over `n` source positions:
    num = max((2o + 1) n - out, 0),  t0 = num // (2 out),  t1 = min(t0 + 1, n - 1),  l = float32(num mod 2 out) / float32(2 out)
-- the weight is the fp32 quotient the kernel forms, everything after it is float64:
    value = (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11).
Two forms: `taps` / `resample_index` spell it out index by index, `resample` is the same thing vectorised in torch.
"""
import numpy as np
import torch


def tap(o: int, n: int, out: int):
    """(t0, t1, l) of output coordinate o: the index form."""
    num = max((2 * o + 1) * n - out, 0)
    t0 = num // (2 * out)
    return t0, min(t0 + 1, n - 1), float(np.float32(num % (2 * out)) / np.float32(2 * out))


def taps(n: int, out: int):
    """(t0, t1, l) for every output coordinate: int64 [out], int64 [out], float64 [out] (each l a float32 value)."""
    o = torch.arange(out, dtype=torch.int64)
    num = ((2 * o + 1) * n - out).clamp_(min=0)
    t0 = num // (2 * out)
    lam = (num % (2 * out)).to(torch.float32) / torch.tensor(2 * out, dtype=torch.float32)
    return t0, (t0 + 1).clamp_(max=n - 1), lam.double()


def resample(src: torch.Tensor, size) -> torch.Tensor:
    """float64 [N,C,H,W] from `src` [N,C,h,w] (any float dtype, widened exactly): the vectorised form."""
    H, W = size
    v = src.detach().cpu().double()
    y0, y1, ly = taps(v.shape[-2], H)
    x0, x1, lx = taps(v.shape[-1], W)
    ly = ly[:, None]
    top = (1 - lx) * v[..., y0, :][..., x0] + lx * v[..., y0, :][..., x1]
    bot = (1 - lx) * v[..., y1, :][..., x0] + lx * v[..., y1, :][..., x1]
    return (1 - ly) * top + ly * bot


def resample_index(src: torch.Tensor, size) -> torch.Tensor:
    """The same, one output element at a time (small inputs only)."""
    H, W = size
    v = src.detach().cpu().double().numpy()
    N, C, h, w = v.shape
    out = np.empty((N, C, H, W), np.float64)
    for o in range(H):
        y0, y1, ly = tap(o, h, H)
        for p in range(W):
            x0, x1, lx = tap(p, w, W)
            out[:, :, o, p] = (1 - ly) * ((1 - lx) * v[:, :, y0, x0] + lx * v[:, :, y0, x1]) + ly * ((1 - lx) * v[:, :, y1, x0] + lx * v[:, :, y1, x1])
    return torch.from_numpy(out)


def labels(scores: torch.Tensor) -> torch.Tensor:
    """uint8 [N,H,W]: the first maximum over the classes."""
    return scores.argmax(dim=1).to(torch.uint8)

"""The references of tests/layout_ref.py against plain nested-loop restatements of the formulas in include/transception_hip.h, on tiny
shapes: the library-call formulations that the GPU tests trust are themselves checked where there is no GPU.  Everything here is exact."""
import math

import pytest
import torch

from layout_ref import (clip_coef, col2im3s2_ref, im2col3s2_ref, nchw_to_tokens, sgd_ref, sgd_torch_ref, stem_im2col_ref, tokens_to_nchw,
                        window_partition_ref, window_reverse_ref, window_rows_ref)


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _im2col_loops(x, k, stride, pad, Cout_ch, ld):
    """x [B, Cs, H, W]: column c*k*k + ky*k + kx = x(b, stride oy + ky - pad, stride ox + kx - pad, c), zero outside the map and up to ld;
    a one-channel source feeds every one of the Cout_ch channels."""
    B, Cs, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    out = torch.zeros(B * Ho * Wo, ld, dtype=x.dtype)
    for b in range(B):
        for oy in range(Ho):
            for ox in range(Wo):
                for c in range(Cout_ch):
                    for ky in range(k):
                        for kx in range(k):
                            iy, ix = stride * oy + ky - pad, stride * ox + kx - pad
                            if 0 <= iy < H and 0 <= ix < W:
                                out[(b * Ho + oy) * Wo + ox, c * k * k + ky * k + kx] = x[b, 0 if Cs == 1 else c, iy, ix]
    return out


@pytest.mark.parametrize("B,Cs,Cin,H,W", [(2, 3, 3, 5, 7), (1, 2, 2, 6, 4), (2, 1, 1, 1, 1), (2, 1, 3, 4, 3)])
def test_im2col3s2_ref(B, Cs, Cin, H, W):
    x = _rand((B, Cs, H, W), 1)
    assert torch.equal(im2col3s2_ref(x, Cin), _im2col_loops(x, 3, 2, 1, Cin, 9 * Cin))
    t = nchw_to_tokens(x)                                                    # the token-major source is the same map
    assert torch.equal(tokens_to_nchw(t, B, H, W), x)


@pytest.mark.parametrize("B,C,H,W", [(2, 3, 5, 7), (1, 2, 6, 4), (2, 1, 1, 1)])
def test_col2im3s2_ref(B, C, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = torch.randint(-32, 33, (B * Ho * Wo, 9 * C), generator=torch.Generator().manual_seed(2)).double() / 8      # grid values: sums exact
    want = torch.zeros(B * H * W, C, dtype=torch.float64)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                for c in range(C):
                    for ky in range(3):
                        for kx in range(3):
                            sy, sx = y + 1 - ky, x + 1 - kx
                            if sy >= 0 and sx >= 0 and sy % 2 == 0 and sx % 2 == 0 and sy // 2 < Ho and sx // 2 < Wo:
                                want[(b * H + y) * W + x, c] += d[(b * Ho + sy // 2) * Wo + sx // 2, c * 9 + ky * 3 + kx]
    got = col2im3s2_ref(d, B, C, H, W)
    assert torch.equal(got, want)
    # and it is the adjoint of im2col3s2_ref: <im2col(x), d> == <x, col2im(d)> exactly on grid values
    xt = torch.randint(-32, 33, (B * H * W, C), generator=torch.Generator().manual_seed(3)).double() / 8
    assert float((im2col3s2_ref(tokens_to_nchw(xt, B, H, W)) * d).sum()) == float((xt * got).sum())


@pytest.mark.parametrize("B,Cs,H,W", [(2, 3, 9, 6), (1, 1, 5, 13), (1, 1, 1, 1)])
def test_stem_im2col_ref(B, Cs, H, W):
    img = _rand((B, Cs, H, W), 4)
    got = stem_im2col_ref(img)
    assert got.shape[1] == 148 and torch.equal(got, _im2col_loops(img, 7, 4, 3, 3, 148)) and bool((got[:, 147] == 0).all())


@pytest.mark.parametrize("B,H,W,ws,ntw,off,C", [(2, 6, 9, 3, 14, 4, 2), (1, 4, 4, 4, 16, 0, 1), (1, 3, 5, 1, 2, 1, 3)])
def test_window_rows_ref(B, H, W, ws, ntw, off, C):
    nwin = B * (H // ws) * (W // ws)
    m = _rand((B * H * W, C), 5)
    win0 = _rand((nwin * ntw + 2, C), 6)
    want, want_acc = win0.clone(), win0.clone()
    for b in range(B):
        for y in range(H):
            for x in range(W):
                r = ((b * (H // ws) + y // ws) * (W // ws) + x // ws) * ntw + off + (y % ws) * ws + x % ws
                want[r] = m[(b * H + y) * W + x]
                want_acc[r] += m[(b * H + y) * W + x]
    got = window_rows_ref(m, win0, B, H, W, ws, ntw, off, to_map=False)
    assert torch.equal(got, want)
    # the reverse reads the same rows back, whatever the other rows hold; the two permutations are inverses
    map0 = _rand((B * H * W + 1, C), 7)
    back = window_rows_ref(got, map0, B, H, W, ws, ntw, off, to_map=True)
    assert torch.equal(back[:-1], m) and torch.equal(back[-1], map0[-1])
    assert torch.equal(window_reverse_ref(window_partition_ref(m, B, H, W, ws), B, H, W, ws), m)
    acc = window_rows_ref(got, map0, B, H, W, ws, ntw, off, to_map=True, accumulate=True)
    assert torch.equal(acc[:-1], map0[:-1] + m) and torch.equal(acc[-1], map0[-1])
    acc = window_rows_ref(m, win0, B, H, W, ws, ntw, off, to_map=False, accumulate=True)
    assert torch.equal(acc, want_acc)


@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("clip", [math.inf, 0.5])
@pytest.mark.parametrize("gscale", [1.0, 1.0 / 128])
def test_sgd_refs_agree(first, clip, gscale):
    """The closed form, float64 torch.optim.SGD after clip_grad_norm_, and an element loop of the header's formula."""
    n, lr, mom, wd = 37, 0.05, 0.5, 1e-2
    w, g, m = _rand((n,), 8), _rand((n,), 9) * 3, _rand((n,), 10)
    ss = float((g * g).sum())
    coef = clip_coef(ss, clip)
    assert (coef < 1.0) == (clip != math.inf)
    w1, b1, A = sgd_ref(w, g, m, lr, mom, wd, gscale, first, coef)
    w2, b2 = sgd_torch_ref(w, g, m, lr, mom, wd, gscale, first, clip)
    for i in range(n):
        d = float(g[i]) * (gscale * coef) + wd * float(w[i])
        b = d if first else mom * float(m[i]) + d
        assert float(b1[i]) == b and float(w1[i]) == float(w[i]) - lr * b
        assert float(A[i]) == abs(float(g[i]) * (gscale * coef)) + abs(wd * float(w[i])) + (0.0 if first else abs(mom * float(m[i])))
    # torch applies the factors in another order (g coef, then gscale, then + wd w): a few float64 roundings apart
    assert float((b1 - b2).abs().max()) <= 8 * 2.0 ** -53 * float(A.max()) and float((w1 - w2).abs().max()) <= 8 * 2.0 ** -53 * float((w.abs() + lr * A).max())

"""Host reference of the Adam / AdamW update in csrc/train.hip (tc_adam_step_multi), in float64 numpy, and the error bounds the GPU tests
hold the kernel to (tests/test_adam_host.py pins the closed form to torch.optim.AdamW and torch.optim.Adam).

The bounds, derived by counting the kernel's roundings to first order (u = 2^-24, float32's unit roundoff; each count is then doubled).
G = |g c| + |wd w| (coupled decay; |g c| alone when decoupled) is the sum of the absolute terms of gh, so |gh| <= G.

  gh = g c + wd w          c = gscale x 1 / scale x min(clip x scale / (sqrt(ss) + 1e-6), 1) carries at most 6 roundings (two products by
                           the loss-scale words, the correctly rounded sqrtf, the sum, the division, the last product; fminf is exact),
                           g c one more, wd w one, the sum one (fewer where the compiler fuses):      |gh - gh_ref| <= 8 u G
  m' = b1 m + omb1 gh      the two products and the sum add one rounding to the gh term and two to the m term:
                           <= 2 u |b1 m| + 10 u omb1 G <= 10 u Am,   Am = |b1 m| + omb1 G.            K = 10, doubled: 20
  v' = b2 v + (omb2 gh) gh   gh enters twice (16), two products and the sum (3); the v term takes 2:
                           <= 19 u Av,   Av = b2 v + omb2 G^2.                                        K = 19, doubled: 38
  w' = w dk - step q       dk = 1 - lr wd (2 roundings, of magnitude <= 1), w dk (1) and the final subtraction (1): 4 u |w|, which the
                           bound states as it is.  The step term step m' / den, step = lr / bc1, den = sqrt(v') / bc2 + eps:
                           the division lr / bc1, m' / den, the product and the share of the final subtraction: 4; inherited from m':
                           10 u Am; den's own sqrtf, division and sum: 3; inherited from v' through the square root: half its relative
                           error, 9.5 u Av / v'.  When decoupled every term of v' is non-negative and Av = v'_ref, so the factor is 1.
                           With coupled decay Av / v' exceeds 1 only where g c and wd w cancel (|gh| << G); the sharper product form
                           of the same term, 8 u omb2 G |gh| / v', stays of order 10 u for the arenas of the tests (v >= 1e-3), which
                           the doubling covers.  All relative to |step q| <= step Am / den:  4 + 10 + 3 + 9.5 = 26.5.  K = 27, doubled: 54

      |m' - m'_ref| <= 20 u Am        |v' - v'_ref| <= 38 u Av        |w' - w'_ref| <= 4 u |w| + 54 u (lr / bc1) Am / den_ref

The hyper-parameters reach the kernel as float32 (lr, eps, wd) or are rounded once from double on the host side of the launch (float(beta),
float(1 - beta)); the reference takes those same values, and the bias terms as the float32 words of the Adam state, so none of them
contributes to the bounds."""
import numpy as np

U = 2.0 ** -24
K_M, K_V, K_W = 20.0, 38.0, 54.0


def f32(v) -> float:
    """The float32 value a kernel receives for a host float, as a Python float."""
    return float(np.float32(v))


def betas32(beta1: float, beta2: float):
    """(float(beta1), float(1 - beta1), float(beta2), float(1 - beta2)): each rounded once from double, as the C entry does."""
    return f32(beta1), f32(1.0 - beta1), f32(beta2), f32(1.0 - beta2)


def bias_terms(beta1: float, beta2: float, t: int):
    """Words 1 and 2 of the Adam state after t updates: float32(1 - beta1^t), float32(sqrt(1 - beta2^t)), formed in float64."""
    return f32(1.0 - np.float64(beta1) ** t), f32(np.sqrt(1.0 - np.float64(beta2) ** t))


def _f64(a):
    return a.double() if hasattr(a, "double") else np.asarray(a, dtype=np.float64)


def adam_ref(w, g, m, v, lr, b1, omb1, b2, omb2, eps, wd, bc1, bc2, decoupled=True, c=1.0):
    """The update in float64 from float32 arrays: numpy arrays, or torch tensors on any device (the result is of the same kind).  lr, eps,
    wd, b1 = float(beta1), omb1 = float(1 - beta1), b2, omb2 are the float32 VALUES the kernel uses; bc1 = 1 - beta1^t and
    bc2 = sqrt(1 - beta2^t) the bias terms; wd a scalar or a float64 array per element; c = gscale x clip coefficient (x 1 / loss scale).
    Returns (w', m', v', Am, Av, den): the magnitudes Am = |b1 m| + omb1 G and Av = b2 v + omb2 G^2 with G = |g c| + |wd w| (coupled) and
    the reference denominator den = sqrt(v') / bc2 + eps, in which the module docstring states the bounds."""
    w, g, m, v = _f64(w), _f64(g), _f64(m), _f64(v)
    t = g * c
    if decoupled:
        w1, gh, G = w * (1.0 - lr * wd), t, abs(t)
    else:
        w1, gh, G = w, t + wd * w, abs(t) + abs(wd * w)
    m1 = b1 * m + omb1 * gh
    v1 = b2 * v + omb2 * gh * gh
    den = v1 ** 0.5 / bc2 + eps
    w2 = w1 - (lr / bc1) * m1 / den
    return w2, m1, v1, abs(b1 * m) + omb1 * G, b2 * v + omb2 * G * G, den


def bounds(w, lr, bc1, Am, Av, den):
    """(bound on m', bound on v', bound on w') of the module docstring."""
    return K_M * U * Am, K_V * U * Av, 4.0 * U * abs(_f64(w)) + K_W * U * (lr / bc1) * Am / den

"""Host reference of the weight averaging in csrc/ema.hip (tc_ema_advance, tc_ema_update_multi; include/transception_ema.h): the decay
schedule in float64, the float64 closed form of the update from float32 arrays, and the error bound the GPU tests hold the kernel to
(tests/test_ema_host.py pins the closed form to torch.optim.swa_utils.AveragedModel).

The schedule.  At the n-th counted update (n = 1, 2, ...) the decay is, in float64,
    d = 0 for n = 1 (the first update copies);  min(decay, (1 + n) / (10 + n)) with warmup;  decay without.
The state words are n, float32(d), float32(1 - d), 0: each float rounded once from the double, so the reference matches them to the bit.

The update.  With omd = the float32 word 2:  e' = w exactly where omd == 1;  elsewhere e' = e + omd (w - e).

The bound, derived by counting the kernel's roundings to first order (u = 2^-24, float32's unit roundoff; the count is then doubled, as
in tests/adam_ref.py).  omd reaches the kernel and the reference as the same float32 value and contributes nothing.
    t  = fl(w - e)        one rounding:                                        t  = (w - e)(1 + d1)
    q  = fl(omd t)        one rounding -- none when the compiler fuses it into the sum (-ffp-contract=fast):
                                                                               q  = omd (w - e)(1 + d1)(1 + d2)
    e' = fl(e + q)        one rounding of the result:                          e' = (e + q)(1 + d3)
  so  e' - ref = omd (w - e)(d1 + d2) + ref d3  to first order, and
      |e' - ref| <= 2 u omd |w - e| + u |ref|.
  Doubled:  |e' - ref| <= 4 u omd |w - e| + 2 u |ref|  (+ 2^-148: two steps of the subnormal grid, for a product or a sum that lands
  below 2^-126, where a rounding is absolute, not relative).
The fused form has one rounding fewer and lies inside the same bound.  Where omd == 1 the bound is 0."""
import numpy as np

U = 2.0 ** -24
K_DIFF, K_RESULT = 4.0, 2.0
TINY = 2.0 ** -148


def f32(v) -> float:
    """The float32 value nearest a host float, as a Python float."""
    return float(np.float32(v))


def decay_at(n: int, decay: float, warmup: bool) -> float:
    """The decay the n-th counted update applies (n >= 1), in float64."""
    if n < 1:
        raise ValueError(f"updates are counted from 1, got {n}")
    if n == 1:
        return 0.0
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def state_words(n: int, decay: float, warmup: bool):
    """(n, d, 1 - d, 0) as tc_ema_advance leaves them after the n-th counted update: the two floats as float32 values."""
    d = decay_at(n, decay, warmup)
    return n, f32(d), f32(1.0 - d), 0


def _f64(a):
    return a.double() if hasattr(a, "double") else np.asarray(a, dtype=np.float64)


def ema_ref(e, w, omd: float):
    """The update in float64 from float32 arrays: numpy arrays, or torch tensors on any device (the result is of the same kind).  omd is
    the float32 VALUE of state word 2.  Returns (e', bound): the closed form and the module docstring's bound on |kernel - e'|."""
    e, w = _f64(e), _f64(w)
    if omd == 1.0:
        return (w.clone(), w.new_zeros(w.shape)) if hasattr(w, "clone") else (w.copy(), np.zeros_like(w))
    diff = w - e
    ref = e + omd * diff
    return ref, K_DIFF * U * omd * abs(diff) + K_RESULT * U * abs(ref) + TINY

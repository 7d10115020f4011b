"""Training-step harness: the reference's trainer.py semantics on the MI355X engine.

  loss = 0.4 * CrossEntropy + 0.6 * Dice(softmax=True)           trainer.py:141-143, utils.py:11-47
  SGD(momentum 0.9, weight_decay 1e-4), per-iteration cosine LR   trainer.py:125-127, 151-153
  (FusedAdamW: torch.optim.AdamW / Adam in its place, with the step count of the bias corrections on the device)
  batch-dim sharding: one process per GPU, gradients all-reduced over RCCL (the reference uses
  nn.DataParallel, trainer.py:110-111); the Dice sums are all-reduced so the loss equals the
  single-process global-batch loss.

Loss and optimiser are HIP kernels too (tc_seg_loss_*, tc_sgd_step); torch provides memory, streams and
torch.distributed only.
"""
from __future__ import annotations

import contextlib
import math
import numbers
import os
from typing import Optional, Union

import torch
import torch.distributed as dist

from ._lib import TC_IGNORE_NONE, TC_OVERLAP_DICE, TC_OVERLAP_TVERSKY, lib
from .engine import TC_DTYPE


def _dt(t: torch.Tensor) -> int:
    return TC_DTYPE[t.dtype]


COMM_AT_WORLD_1 = os.environ.get("TC_COMM_WORLD1", "0") == "1"


def comm_on(group=None) -> bool:
    """True when the step's collectives are to be issued: a process group of more than one rank -- or of exactly ONE rank when
    COMM_AT_WORLD_1 is set (TC_COMM_WORLD1=1; bench.py --gpus 1 --force-split and tests/test_rccl_gpu.py): a 1-rank RCCL all-reduce
    still goes through communicator creation, the collective stream, the async work handles and the no-collective-in-capture rule
    of the split step, so the structure the driver's 8-GPU run uses is executed on one GPU first."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size(group) > 1 or COMM_AT_WORLD_1


def seg_sums_allreduce(sums: torch.Tensor, n_pix: float, group=None):
    """C2 of SURVEY.md section 8(e): the [1 + 3*classes] vector (sum CE, then intersect/y_sum/z_sum per class) is summed over
    ranks so that every rank forms the loss of the GLOBAL batch (Dice is not linear in the batch, utils.py:24-32)."""
    world = 1
    if comm_on(group):
        world = dist.get_world_size(group)
        dist.all_reduce(sums, group=group)
    return sums, n_pix * world, world


OVERLAPS = {"dice": TC_OVERLAP_DICE, "tversky": TC_OVERLAP_TVERSKY}     # SegLoss(overlap=...) -> the constant of include/transception_loss.h


def loss_from_sums(sums: torch.Tensor, n_pix: float, w_ce: float, w_dice: float, weights: Optional[torch.Tensor] = None, *,
                   overlap: str = "dice", tversky_alpha: float = 0.5, tversky_beta: float = 0.5, topk: bool = False):
    """0.4*CE + 0.6*Dice from the (global) sums: trainer.py:141-143, utils.py:34-47 (smooth 1e-5, mean over classes).
    Device sums: one tc_seg_loss_value launch.  Host sums (the gloo tests): the same expression in torch, double.

    weights (the class-weighted / ignoring loss, SegLoss._route): [2 * classes] floats, CE weights then Dice weights, on the device
    of `sums`.  sums[0] is then sum_i w[y_i] nll_i and the CE denominator is sum_k w_ce[k] Y_k, taken from the sums themselves
    (n_pix is not used); a zero denominator gives CE = 0, not NaN.  Dice = sum_k w_dice[k] (1 - ...) / classes (utils.py:42-46).

    overlap="tversky" (sums of the tc_seg_loss_fwd_ft forward under TC_OVERLAP_TVERSKY: the third per-class sum is P_k = sum p): the
    second term is sum_k w_dice[k] (1 - (I_k + 1e-5) / ((1 - a - b) I_k + a P_k + b Y_k + 1e-5)) / classes with a, b = tversky_alpha,
    tversky_beta, and the CE denominator is sum_k w_ce[k] Y_k whether weights are given or not.  A focal gamma needs nothing here:
    sums[0] carries the factor already.

    topk (sums of the tc_seg_loss_fwd_topk forward after tc_topk_select, include/transception_topk.h): sums[0] IS the cross-entropy, the
    mean over the ranks of each rank's top-k mean; nothing divides it."""
    ncls = (sums.numel() - 1) // 3
    if overlap not in OVERLAPS:
        raise ValueError(f"overlap must be one of {tuple(OVERLAPS)}, got {overlap!r}")
    if sums.is_cuda:
        out3 = torch.empty(3, dtype=torch.float32, device=sums.device)
        stream = torch.cuda.current_stream(sums.device).cuda_stream
        if topk:
            lib().tc_seg_loss_value_topk(sums.data_ptr(), None if weights is None else weights.data_ptr(), ncls, float(w_ce), float(w_dice),
                                         OVERLAPS[overlap], float(tversky_alpha), float(tversky_beta), out3.data_ptr(), stream)
        elif overlap != "dice":
            lib().tc_seg_loss_value_ft(sums.data_ptr(), None if weights is None else weights.data_ptr(), ncls, float(w_ce), float(w_dice),
                                       OVERLAPS[overlap], float(tversky_alpha), float(tversky_beta), out3.data_ptr(), stream)
        elif weights is None:
            lib().tc_seg_loss_value(sums.data_ptr(), ncls, float(n_pix), float(w_ce), float(w_dice), out3.data_ptr(), stream)
        else:
            lib().tc_seg_loss_value_w(sums.data_ptr(), weights.data_ptr(), ncls, float(w_ce), float(w_dice), out3.data_ptr(), stream)
        return out3[0], out3[1], out3[2]
    s = sums.double()
    inter, ysum, zsum = s[1::3], s[2::3], s[3::3]
    if overlap == "dice":
        per_class = 1.0 - (2.0 * inter + 1e-5) / (zsum + ysum + 1e-5)
    else:
        a, b = float(tversky_alpha), float(tversky_beta)
        per_class = 1.0 - (inter + 1e-5) / ((1.0 - a - b) * inter + a * zsum + b * ysum + 1e-5)
        if weights is None:
            weights = torch.ones(2 * ncls, dtype=torch.float64)
    if topk:
        ce = s[0]
        dice = per_class.mean() if weights is None else (weights.double()[ncls:] * per_class).sum() / ncls
    elif weights is None:
        ce = s[0] / n_pix
        dice = per_class.mean()
    else:
        w = weights.double()
        den = (w[:ncls] * ysum).sum()
        ce = s[0] / den if float(den) > 0.0 else torch.zeros((), dtype=torch.float64)
        dice = (w[ncls:] * per_class).sum() / ncls
    return w_ce * ce + w_dice * dice, ce, dice


IGNORE_NONE = TC_IGNORE_NONE     # "no ignore_index" for the tc_seg_loss_*_w entries


def check_class_weights(name: str, w, ncls: int, need_positive: bool) -> Optional[tuple]:
    """A per-class weight vector as a tuple of floats (None stays None): `ncls` finite numbers >= 0, not bools; with
    need_positive at least one of them > 0.  Anything else is a ValueError."""
    if w is None:
        return None
    if isinstance(w, torch.Tensor):
        w = w.detach().cpu().tolist()
    try:
        vals = list(w)
    except TypeError:
        raise ValueError(f"{name} must be a sequence of {ncls} numbers, got {w!r}") from None
    if len(vals) != ncls:
        raise ValueError(f"{name} must have {ncls} entries (one per class), got {len(vals)}")
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must hold finite numbers >= 0, got {v!r}")
    if need_positive and not any(v > 0 for v in vals):
        raise ValueError(f"{name} must not be all zero")
    return tuple(float(v) for v in vals)


def check_ignore_index(ii, ncls: int) -> Optional[int]:
    """None, or an int outside [0, ncls) that a 32-bit label compare can hold (the kernels' "off" value excluded)."""
    if ii is None:
        return None
    if isinstance(ii, bool) or not isinstance(ii, int):
        raise ValueError(f"ignore_index must be an int or None, got {ii!r}")
    if 0 <= ii < ncls:
        raise ValueError(f"ignore_index {ii} is a class index: it must lie outside [0, {ncls})")
    if not IGNORE_NONE < ii < 2 ** 31:
        raise ValueError(f"ignore_index {ii} does not fit the kernels' 32-bit label compare")
    return ii


def check_focal_tversky(gamma, overlap, alpha, beta) -> tuple:
    """(focal_gamma, overlap, tversky_alpha, tversky_beta) as (float, str, float, float).  gamma: a finite number >= 0; overlap: "dice" or
    "tversky"; alpha, beta: finite numbers >= 0, not both 0 -- and, under overlap="dice", left at their default 0.5, so that a Tversky
    setting without overlap="tversky" does not train on Dice unnoticed.  A number is any numbers.Real but a bool (numpy scalars from a sweep
    included).  Anything else is a ValueError."""
    for name, v in (("focal_gamma", gamma), ("tversky_alpha", alpha), ("tversky_beta", beta)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    if not isinstance(overlap, str) or overlap not in OVERLAPS:
        raise ValueError(f"overlap must be one of {tuple(OVERLAPS)}, got {overlap!r}")
    if overlap == "dice" and (alpha != 0.5 or beta != 0.5):
        raise ValueError(f'tversky_alpha / tversky_beta are read under overlap="tversky" only, got {alpha!r}, {beta!r} with overlap="dice"')
    if alpha + beta == 0:
        raise ValueError("tversky_alpha + tversky_beta must be > 0")
    return float(gamma), overlap, float(alpha), float(beta)


def check_ce_topk(frac, ncls: int) -> Optional[float]:
    """SegLoss(ce_topk=...): None (off) stays None; else a number in (0, 1], not a bool, as a float.  Anything else is a ValueError, and so
    is top-k above the 16 classes the loss kernels take."""
    if frac is None:
        return None
    if isinstance(frac, bool) or not isinstance(frac, numbers.Real) or not math.isfinite(frac) or not 0.0 < frac <= 1.0:
        raise ValueError(f"ce_topk must be None or a number in (0, 1], got {frac!r}")
    if ncls > 16:
        raise ValueError(f"the top-k loss kernels take at most 16 classes, got {ncls}")
    return float(frac)


class DynamicLossScale:
    """A loss scale for float16 storage that lives in device memory and tunes itself from inside the (captured) step.

    The rule is torch.amp.GradScaler.update's, with two clamps added: a step whose squared gradient norm is not finite is skipped
    (FusedSGD) and multiplies the scale by `backoff_factor`, never below `min_scale`; `growth_interval` clean steps in a row multiply
    it by `growth_factor`, never above `max_scale`.  Unlike GradScaler nothing is read back on the host: the state is four 32-bit
    words on the device (include/transception_hip.h: scale, 1 / scale, growth tracker, skipped count), the loss backward multiplies by
    word 0, tc_sgd_step_multi_scaled divides by it through word 1, and tc_loss_scale_update -- one single-thread launch after the
    update -- applies the rule.  A GraphedStep therefore carries the scale, the skip and the adjustment in its replayed graph.

    Several GPUs: the squared norm is taken AFTER the gradient all-reduce, so every rank sees the same value -- inf or NaN included
    when only one rank overflowed, since a sum with a non-finite term is not finite.  Every rank makes the same decision from the
    same number and keeps the same scale: no collective of its own is needed.

    Pass it as SegLoss(loss_scale=DynamicLossScale()); train_step / GraphedStep hand it to the optimiser.  The device state is created
    on the first device it meets.  value(), skipped() and state_dict() read it back: each is a host sync, for log lines and
    checkpoints, not for the step."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                 min_scale: float = 1.0, max_scale: float = 2.0 ** 24):
        vals = dict(init_scale=init_scale, growth_factor=growth_factor, backoff_factor=backoff_factor, min_scale=min_scale, max_scale=max_scale)
        for k, v in vals.items():
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{k} must be a finite number, got {v!r}")
        if isinstance(growth_interval, bool) or not isinstance(growth_interval, int) or not 1 <= growth_interval < 2 ** 31:
            raise ValueError(f"growth_interval must be an integer >= 1, got {growth_interval!r}")
        if not growth_factor >= 1.0:
            raise ValueError(f"growth_factor must be >= 1, got {growth_factor!r}")
        if not 0.0 < backoff_factor < 1.0:
            raise ValueError(f"backoff_factor must lie in (0, 1), got {backoff_factor!r}")
        if not 0.0 < min_scale <= init_scale <= max_scale:
            raise ValueError(f"need 0 < min_scale <= init_scale <= max_scale, got {min_scale!r}, {init_scale!r}, {max_scale!r}")
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), growth_interval
        self.min_scale, self.max_scale = float(min_scale), float(max_scale)
        self._host = (float(init_scale), 0, 0)           # (scale, tracker, skipped) until the device state exists
        self._state: Optional[torch.Tensor] = None       # fp32[4]; words 2 and 3 are int32

    def _words(self, scale: float, tracker: int, skipped: int) -> torch.Tensor:
        w = torch.zeros(4, dtype=torch.float32)
        w[0], w[1] = scale, 1.0 / scale
        w.view(torch.int32)[2], w.view(torch.int32)[3] = tracker, skipped
        return w

    def state(self, device) -> torch.Tensor:
        """The four-word device state (created on first use).  Its address is baked into captured launches: it is never replaced."""
        if self._state is None:
            self._state = self._words(*self._host).to(device)
        elif (d := torch.device(device)).type != self._state.device.type or d.index not in (None, self._state.device.index):
            raise RuntimeError(f"this DynamicLossScale lives on {self._state.device}, not {device}: use one per device")
        return self._state

    def update(self, sumsq: torch.Tensor):
        """The rule's step from the squared gradient norm of the step just taken (FusedSGD.step calls it): one launch, no sync."""
        st = self.state(sumsq.device)
        lib().tc_loss_scale_update(st.data_ptr(), sumsq.data_ptr(), self.growth_factor, self.backoff_factor, self.growth_interval,
                                   self.min_scale, self.max_scale, torch.cuda.current_stream(sumsq.device).cuda_stream)

    def state_dict(self) -> dict:
        """{"scale", "growth_tracker", "skipped"}.  Reads the device state back once it exists: a host sync."""
        if self._state is not None:
            w = self._state.cpu()
            self._host = (float(w[0]), int(w.view(torch.int32)[2]), int(w.view(torch.int32)[3]))
        return {"scale": self._host[0], "growth_tracker": self._host[1], "skipped": self._host[2]}

    def load_state_dict(self, sd: dict):
        """Writes an existing device state IN PLACE: a captured step has its address in its launches and sees the new value on the
        next replay (a fresh tensor would leave the graph reading the old one)."""
        scale, tracker, skipped = float(sd["scale"]), int(sd.get("growth_tracker", 0)), int(sd.get("skipped", 0))
        if not (math.isfinite(scale) and scale > 0.0) or tracker < 0 or skipped < 0:
            raise ValueError(f"bad loss-scale state {sd!r}")
        self._host = (scale, tracker, skipped)
        if self._state is not None:
            self._state.copy_(self._words(*self._host))

    def value(self) -> float:
        """The current scale.  A host sync."""
        return self.state_dict()["scale"]

    def skipped(self) -> int:
        """Updates skipped so far, counted on the device by every step (not only those a log line looked at).  A host sync."""
        return self.state_dict()["skipped"]


def _wire_loss_scale(loss_fn, opt, device) -> None:
    """The optimiser takes out the scale the loss puts in: a static one as grad_scale, a DynamicLossScale through its device state."""
    ls = getattr(loss_fn, "loss_scale", 1.0)
    if isinstance(ls, DynamicLossScale):
        ls.state(device)                                  # exists before anything is captured
        opt.loss_scaler, opt.grad_scale = ls, 1.0
    else:
        opt.loss_scaler, opt.grad_scale = None, 1.0 / ls


def _overlap_of(route) -> dict:
    """loss_from_sums' overlap keywords for a SegLoss._route: none for the plain and the class-weighted loss."""
    if route is None or len(route) == 2:
        return {}
    kw = {"overlap": route[3], "tversky_alpha": route[4], "tversky_beta": route[5]}
    if len(route) == 7:                        # top-k: sums[0] is the cross-entropy itself
        kw["topk"] = True
    return kw


def _inv_world(group) -> float:
    """1 / (number of ranks whose sums are added): the share of a rank's top-k mean in the global cross-entropy."""
    return 1.0 / dist.get_world_size(group) if comm_on(group) else 1.0


def _topk_buffers(n_pix: int, device):
    """(value map, select scratch) of the top-k cross-entropy: 4 bytes per pixel and tc_topk_work_bytes()."""
    return (torch.empty(n_pix, dtype=torch.float32, device=device),
            torch.empty((lib().tc_topk_work_bytes() + 7) // 8, dtype=torch.int64, device=device))


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, ncls, w_ce, w_dice, group, loss_scale=1.0, route=None):
        """route: None (the plain loss), or SegLoss._route's (weights tensor or None, ignore_index as the kernels take it) -- the
        class-weighted / ignoring entries, NCHW through ld = 0 -- or its six-element form, for the tc_seg_loss_*_ft entries, or its
        seven-element form (the state tensor last) for the tc_seg_loss_*_topk entries and tc_topk_select."""
        L = lib()
        logits = logits.contiguous()
        B, C, H, W = logits.shape
        assert C == ncls and labels.shape == (B, H, W) and labels.dtype == torch.int64
        stream = torch.cuda.current_stream(logits.device).cuda_stream
        prob = torch.empty((B, C, H, W), dtype=torch.float32, device=logits.device)
        sums = torch.zeros(1 + 3 * ncls, dtype=torch.float32, device=logits.device)
        labels = labels.contiguous()
        if route is None:
            L.tc_seg_loss_fwd(logits.data_ptr(), labels.data_ptr(), prob.data_ptr(), sums.data_ptr(), B, ncls, H * W, _dt(logits), stream)
        elif len(route) == 2:
            L.tc_seg_loss_fwd_w(logits.data_ptr(), 0, labels.data_ptr(), route[0].data_ptr(), route[1], prob.data_ptr(), sums.data_ptr(),
                                B, ncls, H * W, _dt(logits), stream)
        elif len(route) == 6:                  # focal CE / Tversky overlap: (weights, ignore_index, gamma, overlap, alpha, beta)
            L.tc_seg_loss_fwd_ft(logits.data_ptr(), 0, labels.data_ptr(), route[0].data_ptr(), route[1], route[2], OVERLAPS[route[3]],
                                 prob.data_ptr(), sums.data_ptr(), B, ncls, H * W, _dt(logits), stream)
        else:                                  # top-k CE: the value map, then this rank's select BEFORE the sums travel
            values, work = _topk_buffers(B * H * W, logits.device)
            L.tc_seg_loss_fwd_topk(logits.data_ptr(), 0, labels.data_ptr(), route[0].data_ptr(), route[1], route[2], OVERLAPS[route[3]],
                                   prob.data_ptr(), sums.data_ptr(), values.data_ptr(), B, ncls, H * W, _dt(logits), stream)
            L.tc_topk_select(values.data_ptr(), B * H * W, route[6].data_ptr(), sums.data_ptr(), _inv_world(group), work.data_ptr(), stream)
            ctx.topk = (values, route[6].clone(), _inv_world(group))      # the state as this forward left it: a later forward overwrites it
        sums, n_pix, world = seg_sums_allreduce(sums, float(B * H * W), group)
        loss, ce, dice = loss_from_sums(sums, n_pix, w_ce, w_dice, None if route is None else route[0], **_overlap_of(route))
        ctx.save_for_backward(prob, labels, sums)
        ctx.meta = (ncls, w_ce, w_dice, n_pix, world, logits.dtype, loss_scale if isinstance(loss_scale, DynamicLossScale) else float(loss_scale))
        ctx.route = route
        return loss.float(), ce.float(), dice.float()

    @staticmethod
    def backward(ctx, gloss, gce, gdice):
        prob, labels, sums = ctx.saved_tensors
        ncls, w_ce, w_dice, n_pix, world, dtype, loss_scale = ctx.meta
        B, C, H, W = prob.shape
        L = lib()
        stream = torch.cuda.current_stream(prob.device).cuda_stream
        d = torch.empty((B, C, H, W), dtype=dtype, device=prob.device)
        # gradients of the *global* loss w.r.t. local logits; the later gradient all-reduce SUMS ranks, so the usual
        # DDP mean is folded in by the caller (gscale).  gloss is 1 for a plain loss.backward().
        gl = gloss.detach().float().contiguous()             # upstream d(loss) stays on the device: no host sync
        if isinstance(loss_scale, DynamicLossScale):         # ... times the device scale: a one-element product, still no host sync
            gl = (gl * loss_scale.state(prob.device)[0]).reshape(1)
            loss_scale = 1.0
        if ctx.route is None:
            L.tc_seg_loss_bwd(prob.data_ptr(), labels.data_ptr(), sums.data_ptr(), d.data_ptr(), B, ncls, H * W, float(w_ce), float(w_dice),
                              float(n_pix), loss_scale, gl.data_ptr(), _dt(d), stream)
        elif len(ctx.route) == 2:
            L.tc_seg_loss_bwd_w(prob.data_ptr(), None, 0, labels.data_ptr(), ctx.route[0].data_ptr(), ctx.route[1], sums.data_ptr(),
                                d.data_ptr(), 0, B, ncls, H * W, float(w_ce), float(w_dice), loss_scale, gl.data_ptr(), _dt(d), stream)
        elif len(ctx.route) == 6:
            w, ii, gamma, overlap, alpha, beta = ctx.route
            L.tc_seg_loss_bwd_ft(prob.data_ptr(), None, 0, labels.data_ptr(), w.data_ptr(), ii, sums.data_ptr(), d.data_ptr(), 0, B, ncls, H * W,
                                 float(w_ce), float(w_dice), gamma, OVERLAPS[overlap], alpha, beta, loss_scale, gl.data_ptr(), _dt(d), stream)
        else:
            w, ii, gamma, overlap, alpha, beta, _ = ctx.route
            values, state, inv_world = ctx.topk
            L.tc_seg_loss_bwd_topk(prob.data_ptr(), None, 0, labels.data_ptr(), w.data_ptr(), ii, sums.data_ptr(), d.data_ptr(), 0, B, ncls, H * W,
                                   float(w_ce), float(w_dice), gamma, OVERLAPS[overlap], alpha, beta, loss_scale, gl.data_ptr(),
                                   values.data_ptr(), state.data_ptr(), inv_world, _dt(d), stream)
        return d, None, None, None, None, None, None, None


class SegLoss(torch.nn.Module):
    """0.4*CE + 0.6*Dice over the (global) batch; returns (loss, ce, dice).

    ce_weight / dice_weight / ignore_index (all None: the plain loss, through the same calls as ever):
      CE   = torch.nn.CrossEntropyLoss(weight=ce_weight, ignore_index=ignore_index), mean reduction (trainer.py:141):
             sum_i w[y_i] nll_i / sum_i w[y_i] over the pixels whose label is not ignore_index -- but 0 with a zero gradient, not NaN,
             when that denominator is 0 (every pixel ignored, or only zero-weight classes present): a NaN there would read as an
             overflow to the loss-scale guard and skip the update silently;
      Dice = the reference's DiceLoss.forward(weight=dice_weight, softmax=True) (utils.py:34-47):
             sum_k dice_weight[k] (1 - (2 I_k + 1e-5) / (Z_k + Y_k + 1e-5)) / n_classes, an ignored pixel entering none of I, Y, Z.
    The gradient at an ignored pixel is exactly zero in every class.  The weights live in one small device tensor per device
    (weights(device): CE weights, then Dice weights), created on first use and never replaced: captured launches hold its address, so
    new values are written IN PLACE (weights(device).copy_(...)) and are seen by the next replay.  The CE denominator is taken from the fp32 per-class pixel counts of the
    sums vector, which are exact while the global number of counted pixels is below 2^24.

    focal_gamma / overlap / tversky_alpha / tversky_beta (0.0, "dice", 0.5, 0.5: the loss above, through the same calls as ever;
    include/transception_loss.h has the definition and the gradient):
      CE      = sum_i w[y_i] q_i^gamma nll_i / sum_i w[y_i] with q_i = 1 - p_t, the focal modulation of every pixel's term (the denominator
                is not modulated);
      overlap = "tversky": sum_k dice_weight[k] (1 - (I_k + 1e-5) / (I_k + alpha FP_k + beta FN_k + 1e-5)) / n_classes, with FP_k = sum p_k
                off class k and FN_k = sum (1 - p_k) on it.  alpha = beta = 0.5 is the LINEAR Dice 2 I / (P + Y), not the reference's squared
                one, which overlap="dice" stays.
    The returned triple is then (loss, focal CE, overlap term).  These four are scalars, not device memory: a captured step (GraphedStep)
    keeps the values it was captured with, and changing them needs a new GraphedStep.

    ce_topk (None: off -- no launch, no allocation, the calls above; include/transception_topk.h has the definition and the gradient): a
    fraction in (0, 1].  The CE is then the mean of the k = max(1, min(n, ceil(ce_topk n))) LARGEST per-pixel terms w[y_i] q_i^gamma nll_i
    of the n counted pixels -- nnU-Net's TopK loss, online hard-example mining -- chosen on the device by an exact select; it combines with
    every argument above.  Two things to know: the divisor is k whatever the class weights (ce_topk=1 with ce_weight is the mean of the
    weighted terms, not torch's weighted mean), and pixels tied at the threshold share the places left there equally, so the gradient is a
    function of the values (torch.topk picks among ties arbitrarily).  Across ranks each rank selects among its own pixels and the CE is
    the mean of the ranks' top-k means.  The returned triple is (loss, top-k CE, overlap term).  The fraction lives in device memory
    (topk_state(device)[0]): set_topk writes it in place and the next call -- a replay of a captured step included -- follows it."""

    def __init__(self, n_classes: int = 9, w_ce: float = 0.4, w_dice: float = 0.6, group=None,
                 loss_scale: Union[float, DynamicLossScale] = 1.0, ce_weight=None, dice_weight=None, ignore_index: Optional[int] = None,
                 focal_gamma: float = 0.0, overlap: str = "dice", tversky_alpha: float = 0.5, tversky_beta: float = 0.5,
                 ce_topk: Optional[float] = None):
        """loss_scale: the gradient that leaves this loss is multiplied by it (the reported loss is not) -- loss scaling for float16
        storage; FusedSGD.step divides it out again (train_step wires the two together).  A float is a static scale; a
        DynamicLossScale is read from device memory by the backward kernel and adjusts itself after every update.
        ce_weight: n_classes finite numbers >= 0, not all zero; dice_weight: n_classes finite numbers >= 0; ignore_index: an int
        outside [0, n_classes), e.g. 255 or -100.  Bad values raise ValueError."""
        super().__init__()
        self.n_classes, self.w_ce, self.w_dice, self.group = n_classes, w_ce, w_dice, group
        self.loss_scale = loss_scale if isinstance(loss_scale, DynamicLossScale) else float(loss_scale)
        self.ce_weight = check_class_weights("ce_weight", ce_weight, n_classes, need_positive=True)
        self.dice_weight = check_class_weights("dice_weight", dice_weight, n_classes, need_positive=False)
        self.ignore_index = check_ignore_index(ignore_index, n_classes)
        self.focal_gamma, self.overlap, self.tversky_alpha, self.tversky_beta = check_focal_tversky(focal_gamma, overlap, tversky_alpha, tversky_beta)
        if self.weighted and n_classes > 16:
            raise ValueError(f"the class-weighted loss kernels take at most 16 classes, got {n_classes}")
        if self.focal_tversky and n_classes > 16:
            raise ValueError(f"the focal / Tversky loss kernels take at most 16 classes, got {n_classes}")
        self.ce_topk = check_ce_topk(ce_topk, n_classes)
        self._weights = {}                               # device -> fp32 [2 * n_classes]
        self._topk_state = {}                            # device -> fp64 [8]: the fraction, then what tc_topk_select leaves

    @property
    def weighted(self) -> bool:
        """True when the class-weighted / ignoring kernels are used (any of the three arguments set)."""
        return self.ce_weight is not None or self.dice_weight is not None or self.ignore_index is not None

    @property
    def focal_tversky(self) -> bool:
        """True when the focal / Tversky kernels are used (a focal_gamma above 0 or overlap="tversky")."""
        return self.focal_gamma != 0.0 or self.overlap != "dice"

    def _host_weights(self) -> torch.Tensor:
        ones = (1.0,) * self.n_classes
        return torch.tensor((self.ce_weight or ones) + (self.dice_weight or ones), dtype=torch.float32)

    def weights(self, device) -> torch.Tensor:
        """The [2 * n_classes] weight tensor of `device` (CE weights, then Dice weights; ones where none were given)."""
        d = self._device(device)
        if d not in self._weights:
            self._weights[d] = self._host_weights().to(d)
        return self._weights[d]

    def _device(self, device) -> torch.device:
        d = torch.device(device)
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        return d

    def topk_state(self, device) -> torch.Tensor:
        """The [8] float64 state of the top-k select on `device`: [0] the fraction (read on the device), [1..7] n, k, n_gt, n_eq, t, S, f as
        the last select left them.  Created on first use and never replaced: captured launches hold its address."""
        if self.ce_topk is None:
            raise ValueError("this SegLoss was built with ce_topk=None")
        d = self._device(device)
        if d not in self._topk_state:
            self._topk_state[d] = torch.tensor([self.ce_topk] + [0.0] * 7, dtype=torch.float64).to(d)
        return self._topk_state[d]

    def set_topk(self, frac: float) -> None:
        """A new fraction, written IN PLACE into every device's state: the next call or replay selects with it (no new capture)."""
        if self.ce_topk is None:
            raise ValueError("this SegLoss was built with ce_topk=None: top-k cannot be switched on afterwards")
        if frac is None:
            raise ValueError("ce_topk cannot be switched off afterwards")
        self.ce_topk = check_ce_topk(frac, self.n_classes)
        for st in self._topk_state.values():
            st[0:1].fill_(self.ce_topk)

    def topk_stats(self, device) -> dict:
        """What the last select on `device` found: {n, k, n_gt, n_eq, threshold, tie_share} (reads the state back: a host sync)."""
        st = self.topk_state(device).cpu().tolist()
        return {"n": int(st[1]), "k": int(st[2]), "n_gt": int(st[3]), "n_eq": int(st[4]), "threshold": st[5], "tie_share": st[7]}

    def _route(self, device):
        """None for the plain loss; else (weights tensor, ignore_index or the kernels' "off" value) for the tc_seg_loss_*_w entries; with
        a focal_gamma above 0 or overlap="tversky" that pair followed by (focal_gamma, overlap, tversky_alpha, tversky_beta), for the
        tc_seg_loss_*_ft entries; with ce_topk set those six followed by the state tensor, for the tc_seg_loss_*_topk entries."""
        if not self.weighted and not self.focal_tversky and self.ce_topk is None:
            return None
        if self.ce_topk is not None:
            return (self.weights(device), IGNORE_NONE if self.ignore_index is None else self.ignore_index, self.focal_gamma, self.overlap,
                    self.tversky_alpha, self.tversky_beta, self.topk_state(device))
        pair = self.weights(device), IGNORE_NONE if self.ignore_index is None else self.ignore_index
        if not self.focal_tversky:
            return pair
        return (*pair, self.focal_gamma, self.overlap, self.tversky_alpha, self.tversky_beta)

    def forward(self, logits: torch.Tensor, labels: torch.Tensor):
        route = self._route(logits.device)
        if route is None:
            return _SegLossFn.apply(logits, labels.long(), self.n_classes, self.w_ce, self.w_dice, self.group, self.loss_scale)
        return _SegLossFn.apply(logits, labels.long(), self.n_classes, self.w_ce, self.w_dice, self.group, self.loss_scale, route)


def cosine_lr(base_lr: float, step: int, t_max: int) -> float:
    """CosineAnnealingLR(eta_min=0) after `step` scheduler.step() calls (trainer.py:126-127,151-153)."""
    return 0.5 * base_lr * (1.0 + math.cos(math.pi * step / t_max))


def build_segments(views):
    """The update kernels' segment table from the sorted (offset, numel, decay) views of the parameters that receive a gradient: every view
    is padded to a multiple of 8 elements (the arena's own padding, model._ensure_flat) and adjacent views of the same decay are merged.
    Returns [(offset, length, decay)].  Pure host code."""
    segs = []
    for off, n, wd in views:
        n8 = (n + 7) // 8 * 8
        if segs and segs[-1][0] + segs[-1][1] == off and segs[-1][2] == wd:
            segs[-1][1] += n8
        else:
            segs.append([off, n8, wd])
    return [(o, n, wd) for o, n, wd in segs]


def check_no_decay(no_decay):
    """None, a predicate (name, shape) -> bool, or "norm_bias" (every tensor with ndim <= 1: LayerNorm / BatchNorm affine parameters
    and all biases).  Returns the predicate or None; anything else is a ValueError."""
    if no_decay is None or callable(no_decay):
        return no_decay
    if no_decay == "norm_bias":
        return lambda name, shape: len(shape) <= 1
    raise ValueError(f'no_decay must be None, "norm_bias" or a predicate (name, shape) -> bool, got {no_decay!r}')


def check_ema_decay(decay) -> float:
    """An EMA decay as a float: a finite number in [0, 1), not a bool.  Anything else is a ValueError."""
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not math.isfinite(decay) or not 0.0 <= decay < 1.0:
        raise ValueError(f"the EMA decay must be a finite number in [0, 1), got {decay!r}")
    return float(decay)


class WeightEMA:
    """An exponential moving average of the weights, kept in a shadow of the model's flat fp32 arena and updated from inside the
    (captured) step: attach it to a fused optimiser (`opt.ema = WeightEMA(model)`) and every opt.step() launches tc_ema_advance and
    tc_ema_update_multi right after its own update kernel, on the same stream, under the same squared gradient norm -- a step the
    device skips (float16 overflow) is not averaged in and not counted.

    The rule is torch.optim.swa_utils.AveragedModel's with get_ema_multi_avg_fn(decay): the first update copies the weights, every later
    one is e.lerp_(w, 1 - d).  warmup: d = min(decay, (1 + n) / (10 + n)) at the n-th update, so that early averages are not dominated by
    the initial weights.  The count n and the decay derived from it live in four 32-bit words on the device (include/transception_ema.h),
    because a captured kernel's scalar arguments are frozen at capture.

    The shadow is a clone of the whole arena, created on first use: parameters that never receive a gradient hold their true value in it
    for good, and memory grows by 4 bytes per weight.  Neither the shadow nor the state word is ever replaced (captured launches hold
    their addresses).  The segment table is the optimiser's set of views under ONE decay class: adjacent views always merge, whatever
    no_decay splits the optimiser's own table into.  BatchNorm running statistics are buffers, not weights: they are not averaged and
    are taken live (AveragedModel(use_buffers=False)).  Several GPUs: every rank averages identical weights, so no collective is needed."""

    def __init__(self, model, decay: float = 0.999, warmup: bool = True):
        self.model, self.decay, self.warmup = model, check_ema_decay(decay), bool(warmup)
        self.shadow: Optional[torch.Tensor] = None       # fp32, the arena's size
        self._state: Optional[torch.Tensor] = None       # fp32[4]; words 0 and 3 are int32
        self._segs_dev: Optional[torch.Tensor] = None
        self._launched = False                           # an update was launched (perhaps captured) with this decay and warmup
        self._swapped = False

    def _ensure_state(self):
        """The shadow arena and the four-word state.  Their addresses are baked into captured launches: never replaced."""
        M = self.model
        if M._flat is None:
            M._ensure_flat(next(M.parameters()).device)
        if self.shadow is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the EMA's shadow arena must exist before a step is captured: run one eager step first")
            self.shadow = M._flat.clone()
            self._state = torch.zeros(4, dtype=torch.float32, device=M._flat.device)
        elif self.shadow.shape != M._flat.shape or self.shadow.device != M._flat.device:
            raise RuntimeError("the model's parameter arena was rebuilt after this WeightEMA was created: make a new one")

    def segments(self):
        """[(offset, length)] over the views of the parameters that receive a gradient, as ONE decay class (build_segments)."""
        flat = self.model._flat
        views = sorted((off, math.prod(shape), 0.0) for off, shape in self.model._used_views.values())
        return [(off, min(n, flat.numel() - off)) for off, n, _ in build_segments(views)]

    def update(self, sumsq: Optional[int], stream: int):
        """The two launches of one step (the fused optimisers call it right after their update kernel).  sumsq: the device address of
        the squared gradient norm that update used, or None."""
        self.check_not_swapped()
        self._ensure_state()
        if self._segs_dev is None:
            segs = self.segments()
            self._segs_dev = torch.tensor([v for s in segs for v in s], dtype=torch.int64, device=self.shadow.device)
            self._nseg, self._maxlen = len(segs), max(n for _, n in segs)
        L = lib()
        L.tc_ema_advance(self._state.data_ptr(), sumsq, self.decay, int(self.warmup), stream)
        L.tc_ema_update_multi(self.shadow.data_ptr(), self.model._flat.data_ptr(), self._segs_dev.data_ptr(), self._nseg, self._maxlen,
                              self._state.data_ptr(), sumsq, stream)
        self._launched = True

    def updates(self) -> int:
        """Updates averaged so far, as counted on the device (skipped ones are not).  A host sync."""
        return 0 if self._state is None else int(self._state.view(torch.int32)[0].item())

    def check_not_swapped(self):
        if self._swapped:
            raise RuntimeError("the averaged weights are swapped into the model (WeightEMA.swapped()): no optimiser step in there")

    def _swap(self):
        M = self.model
        lib().tc_swap_f32(M._flat.data_ptr(), self.shadow.data_ptr(), M._flat.numel(), torch.cuda.current_stream(M._flat.device).cuda_stream)
        M.invalidate_working_copy()                      # the 16-bit copy follows, in place

    @contextlib.contextmanager
    def swapped(self):
        """Inside the context the model holds the averaged weights and the shadow holds the trained ones: the contents of the two
        arenas are exchanged IN PLACE (tc_swap_f32) and the 16-bit working copy is recast, on entry and again on exit.  Addresses never
        change, so a captured step keeps working afterwards.  Entering twice raises, and so does an opt.step() inside."""
        if self._swapped:
            raise RuntimeError("WeightEMA.swapped() is already active")
        self._ensure_state()
        self._swap()
        self._swapped = True
        try:
            yield self.model
        finally:
            self._swap()
            self._swapped = False

    def model_state_dict(self) -> dict:
        """model.state_dict() with every parameter entry replaced by a clone of its averaged value; buffers (the BatchNorm statistics
        among them) are the live ones.  Loads with strict=True wherever model.state_dict() does."""
        self._ensure_state()
        M = self.model
        src = M._flat if self._swapped else self.shadow
        sd = M.state_dict()
        for name, (off, shape) in M._index.items():
            if name in sd:
                sd[name] = src[off:off + math.prod(shape)].view(shape).clone()
        return sd

    def state_dict(self) -> dict:
        """{"n", "decay", "warmup", "shadow"}: the device's count (a host sync), the two settings and a clone of the shadow arena."""
        self.check_not_swapped()
        self._ensure_state()
        return {"n": self.updates(), "decay": self.decay, "warmup": self.warmup, "shadow": self.shadow.clone()}

    def load_state_dict(self, sd: dict):
        """Writes the count and the shadow IN PLACE (same data_ptrs): a captured step keeps working and sees them on its next replay.
        Words 1 and 2 need no restoring: tc_ema_advance rewrites them from the count before any use.  decay and warmup are arguments
        of the launches, frozen in a captured step: once an update has been launched, other values than the current ones are refused."""
        n, decay, warmup = int(sd["n"]), check_ema_decay(sd["decay"]), bool(sd["warmup"])
        if n < 0:
            raise ValueError(f"bad EMA update count {sd['n']!r}")
        if self._launched and (decay, warmup) != (self.decay, self.warmup):
            raise ValueError(f"updates were launched with decay {self.decay!r}, warmup {self.warmup!r}: cannot load {decay!r}, {warmup!r}")
        self.check_not_swapped()
        self._ensure_state()
        self.decay, self.warmup = decay, warmup
        self.shadow.copy_(sd["shadow"])
        self._state.view(torch.int32)[0:1].copy_(torch.tensor([n], dtype=torch.int32))


class _FusedOptimizer:
    """What the fused optimisers share: the segment table over the parameters that receive a gradient (the 332 grad-less tensors of
    the reference are left untouched, as torch.optim skips `p.grad is None`), the device learning rate, the squared-norm launches of
    clipping and of the overflow guard, the choice of the 16-bit working copy the update refreshes, the skip read-back, and the weight
    average that follows the update (`ema`)."""

    def __init__(self, model, lr: float, weight_decay: float, clip_norm: Optional[float]):
        self.model, self.lr, self.wd = model, lr, weight_decay
        self.clip_norm = clip_norm                       # nn.utils.clip_grad_norm_(max_norm, 2) before the update (trainer.py:147-148)
        self.steps = 0
        self._segments = None
        self._segs_dev: Optional[torch.Tensor] = None
        self._wd_dev: Optional[torch.Tensor] = None      # per-segment decay (FusedAdamW(no_decay=...)); None: one decay for all
        self.lr_dev: Optional[torch.Tensor] = None       # device scalar read by the kernel (hipGraph-friendly schedule)
        self._sumsq: Optional[torch.Tensor] = None       # squared gradient norm (clip_norm)
        self.grad_scale = 1.0                            # gradients in the arena are this many times too small (1 / loss scale)
        self.guard_overflow: Optional[bool] = None       # skip the update when the gradient norm is not finite; None: on for float16 storage
        self.loss_scaler: Optional[DynamicLossScale] = None   # gradients carry its device scale instead (the guard is then always on)
        self.ema: Optional[WeightEMA] = None             # averages the weights after every update, under the update's own skip; None: no launch
        self.skipped_steps = 0                           # updates found skipped by last_step_skipped() (read back at the caller's log cadence)

    def last_step_skipped(self) -> bool:
        """True when the last update was skipped because the gradient norm was not finite (float16 overflow under a loss scale:
        the update kernel returns without touching the weights).  Reads one float back (a host sync): call it where the loop already
        reads its loss scalars; a run whose every step overflows would otherwise look like a plateau."""
        if self._sumsq is None:
            return False
        skipped = not math.isfinite(float(self._sumsq.item()))
        self.skipped_steps += int(skipped)
        return skipped

    def set_lr(self, lr: float):
        self.lr = lr
        if self.lr_dev is not None:
            self.lr_dev.fill_(lr)

    def _decay_of(self, name: str, shape) -> float:
        return self.wd

    def _segs3(self):
        if self._segments is None:
            M = self.model
            names = {}
            for name, pid in getattr(M, "_pid", {}).items():
                names.setdefault(pid, name)
            views = sorted((off, math.prod(shape), self._decay_of(names.get(pid, ""), shape)) for pid, (off, shape) in M._used_views.items())
            self._segments = build_segments(views)
        return self._segments

    def _segs(self):
        return [(o, n) for o, n, _ in self._segs3()]

    def zero_grad(self):
        if self.model._gflat is not None:
            self.model._gflat.zero_()

    def _tables(self, flat):
        """The device learning rate and the device segment table, created on first use and never replaced."""
        if self.lr_dev is None:
            self.lr_dev = torch.full((1,), float(self.lr), dtype=torch.float32, device=flat.device)
        if self._segs_dev is None:
            segs = [(off, min(n, flat.numel() - off)) for off, n in self._segs()]
            self._segs_dev = torch.tensor([v for s in segs for v in s], dtype=torch.int64, device=flat.device)
            self._nseg, self._maxlen = len(segs), max(n for _, n in segs)

    def _norm_launches(self, L, g, stream):
        """tc_fill_f32 + tc_grad_sumsq when clipping or guarding; returns the device address of the squared norm, or None."""
        M = self.model
        guard = self.loss_scaler is not None or (self.guard_overflow if self.guard_overflow is not None else M.compute_dtype == torch.float16)
        if not (self.clip_norm or guard):
            return None
        # clip_grad_norm_(max_norm, 2): one reduction kernel for the squared norm (grad-less parameters hold zeros, so the arena's
        # norm is the model's), the coefficient min(1, max_norm / (norm + 1e-6)) is applied inside the update kernel
        if self._sumsq is None:
            self._sumsq = torch.zeros(1, dtype=torch.float32, device=g.device)
        L.tc_fill_f32(self._sumsq.data_ptr(), 1, 0.0, stream)
        L.tc_grad_sumsq(g.data_ptr(), g.numel(), self._sumsq.data_ptr(), stream)
        return self._sumsq.data_ptr()

    def _ema_check(self):
        """Before anything is launched: an attached WeightEMA is this model's and does not have its weights swapped in."""
        if self.ema is not None:
            if self.ema.model is not self.model:
                raise ValueError("the attached WeightEMA averages another model")
            self.ema.check_not_swapped()

    def _working_copy(self):
        """The 16-bit working copy of the weights that the update kernel refreshes (the forward then skips its cast pass over the arena)."""
        M = self.model
        return M._flat_lp if (M.compute_dtype != torch.float32 and M._flat_lp is not None and M._flat_lp.dtype == M.compute_dtype) else None


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD(momentum, weight_decay) semantics as one kernel over the model's flat arenas.

    Parameters that never receive a gradient (332 tensors in the reference) are left untouched, exactly as
    torch.optim.SGD skips `p.grad is None`: the update runs over the used segments only."""

    def __init__(self, model, lr: float = 0.05, momentum: float = 0.9, weight_decay: float = 1e-4, clip_norm: Optional[float] = None):
        super().__init__(model, lr, weight_decay, clip_norm)
        self.momentum = momentum
        self.buf: Optional[torch.Tensor] = None

    def step(self, grad_scale: Optional[float] = None):
        grad_scale = self.grad_scale if grad_scale is None else grad_scale
        self._ema_check()
        M = self.model
        flat, g = M._flat, M._gflat
        if self.buf is None:
            self.buf = torch.zeros_like(flat)
        self._tables(flat)
        L = lib()
        stream = torch.cuda.current_stream(flat.device).cuda_stream
        scaler = self.loss_scaler
        sumsq = self._norm_launches(L, g, stream)
        lp = self._working_copy()
        # `first` is baked into a captured kernel's arguments, and a skipped first step is harmless all the same: the momentum buffer
        # starts as zeros, so the later form mom * 0 + d equals the first-step form d
        args = (flat.data_ptr(), g.data_ptr(), self.buf.data_ptr(), self._segs_dev.data_ptr(), self._nseg, self._maxlen,
                float(self.lr), self.lr_dev.data_ptr(), float(self.momentum), float(self.wd), float(grad_scale),
                int(self.steps == 0), sumsq, float((self.clip_norm or math.inf) / grad_scale),
                lp.data_ptr() if lp is not None else None, M._tc_dtype() if lp is not None else 0)
        if scaler is None:
            L.tc_sgd_step_multi(*args, stream)
        else:
            # the arena's gradients carry the device scale (grad_scale is 1 here): the kernel divides it out and clips the true norm,
            # then the scale takes its own step from the same squared norm
            L.tc_sgd_step_multi_scaled(*args, scaler.state(flat.device).data_ptr(), stream)
            scaler.update(self._sumsq)
        if self.ema is not None:
            self.ema.update(sumsq, stream)               # the same squared norm: a skipped update is not averaged in
        M._lp_fresh = lp is not None
        self.steps += 1


class FusedAdamW(_FusedOptimizer):
    """torch.optim.AdamW (decoupled=True) or torch.optim.Adam (decoupled=False: the decay enters the gradient) as one kernel over the
    model's flat arenas, under everything FusedSGD runs under: the captured step, gradient clipping, the 16-bit working copy, the
    overflow guard and a DynamicLossScale.

    The step number t of the bias corrections lives on the device (an Adam state, include/transception_hip.h: t, 1 - beta1^t,
    sqrt(1 - beta2^t)): a captured kernel's scalar arguments are frozen at capture, so tc_adam_advance -- one single-thread launch
    before the update -- counts the step and rewrites the two terms, and leaves all of it alone when the update is about to be skipped.
    `steps` counts calls of step(); the device word counts applied updates (state_dict()["step"]).

    no_decay: a predicate (name, shape) -> bool, or "norm_bias" for every tensor with ndim <= 1 (LayerNorm / BatchNorm affine parameters
    and all biases): those tensors take no weight decay.  Segments are then not merged across a change of decay class and the kernel
    reads one decay per segment from device memory."""

    def __init__(self, model, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, decoupled: bool = True,
                 clip_norm: Optional[float] = None, no_decay=None):
        super().__init__(model, lr, weight_decay, clip_norm)
        b1, b2 = (float(b) for b in betas)
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {betas!r}")
        if not (isinstance(eps, (int, float)) and eps > 0.0):
            raise ValueError(f"eps must be > 0, got {eps!r}")
        if not (isinstance(weight_decay, (int, float)) and weight_decay >= 0.0):
            raise ValueError(f"weight_decay must be >= 0, got {weight_decay!r}")
        self.betas, self.eps, self.decoupled = (b1, b2), float(eps), bool(decoupled)
        self._no_decay = check_no_decay(no_decay)
        self.m: Optional[torch.Tensor] = None            # exp_avg
        self.v: Optional[torch.Tensor] = None            # exp_avg_sq
        self._adam_state: Optional[torch.Tensor] = None  # fp32[4]; words 0 and 3 are int32

    def _decay_of(self, name: str, shape) -> float:
        return 0.0 if self._no_decay is not None and self._no_decay(name, tuple(shape)) else float(self.wd)

    def _ensure_state(self):
        """Both moment arenas and the four-word Adam state.  Their addresses are baked into captured launches: never replaced."""
        M = self.model
        if M._flat is None:
            M._ensure_flat(next(M.parameters()).device)
        if self.m is None:
            self.m, self.v = torch.zeros_like(M._flat), torch.zeros_like(M._flat)
            self._adam_state = torch.zeros(4, dtype=torch.float32, device=M._flat.device)

    def device_step(self) -> int:
        """Updates applied so far, as counted on the device (skipped ones are not).  A host sync."""
        return 0 if self._adam_state is None else int(self._adam_state.view(torch.int32)[0].item())

    def step(self, grad_scale: Optional[float] = None):
        grad_scale = self.grad_scale if grad_scale is None else grad_scale
        self._ema_check()
        M = self.model
        flat, g = M._flat, M._gflat
        self._ensure_state()
        self._tables(flat)
        if self._no_decay is not None and self._wd_dev is None:
            self._wd_dev = torch.tensor([wd for _, _, wd in self._segs3()], dtype=torch.float32, device=flat.device)
        L = lib()
        stream = torch.cuda.current_stream(flat.device).cuda_stream
        scaler = self.loss_scaler
        sumsq = self._norm_launches(L, g, stream)
        lp = self._working_copy()
        st = self._adam_state.data_ptr()
        L.tc_adam_advance(st, sumsq, self.betas[0], self.betas[1], stream)
        L.tc_adam_step_multi(flat.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self._segs_dev.data_ptr(),
                             self._wd_dev.data_ptr() if self._wd_dev is not None else None, self._nseg, self._maxlen, float(self.lr),
                             self.lr_dev.data_ptr(), self.betas[0], self.betas[1], self.eps, float(self.wd), int(self.decoupled),
                             float(grad_scale), sumsq, float((self.clip_norm or math.inf) / grad_scale),
                             lp.data_ptr() if lp is not None else None, M._tc_dtype() if lp is not None else 0,
                             scaler.state(flat.device).data_ptr() if scaler is not None else None, st, stream)
        if scaler is not None:
            scaler.update(self._sumsq)               # the scale takes its own step from the same squared norm
        if self.ema is not None:
            self.ema.update(sumsq, stream)               # the same squared norm: a skipped update is not averaged in
        M._lp_fresh = lp is not None
        self.steps += 1

    def state_dict(self) -> dict:
        """{"step", "exp_avg", "exp_avg_sq"}: the device's count of applied updates (a host sync) and clones of the two moment arenas."""
        self._ensure_state()
        return {"step": self.device_step(), "exp_avg": self.m.clone(), "exp_avg_sq": self.v.clone()}

    def load_state_dict(self, sd: dict):
        """Writes the step word and both arenas IN PLACE (same data_ptrs): a captured step keeps working and sees them on its next
        replay.  The two bias words need no restoring: tc_adam_advance rewrites them from the step word before any use."""
        step = int(sd["step"])
        if step < 0:
            raise ValueError(f"bad optimiser step {sd['step']!r}")
        self._ensure_state()
        self.m.copy_(sd["exp_avg"])
        self.v.copy_(sd["exp_avg_sq"])
        self._adam_state.view(torch.int32)[0:1].copy_(torch.tensor([step], dtype=torch.int32))


def gradient_buckets(model, max_gap: int = 1 << 18):
    """Contiguous ranges of the flat gradient arena that hold live gradients, merged across gaps of < max_gap elements: the
    332 grad-less tensors (9.2 M of 47.3 M elements, SURVEY 8e: `conv1_1_s*`, decoder_3's unused blocks, ...) are not worth
    sending, but neither are dozens of tiny collectives.  Falls back to the whole arena before the first forward."""
    views = getattr(model, "_used_views", None)
    n = model._gflat.numel()
    if not views:
        return [(0, n)]
    rng = sorted((off, off + math.prod(shape)) for off, shape in views.values())
    out = [list(rng[0])]
    for a, b in rng[1:]:
        if a - out[-1][1] < max_gap:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return [(a, min(b, n)) for a, b in out]


def split_buckets(buckets, cut: int):
    """(early, late): the buckets below / at-or-above arena offset `cut`, a bucket that straddles it cut in two."""
    early, late = [], []
    for a, b in buckets:
        if b <= cut:
            early.append((a, b))
        elif a >= cut:
            late.append((a, b))
        else:
            early.append((a, cut))
            late.append((cut, b))
    return early, late


def clip_buckets(buckets, ranges):
    """The parts of `buckets` inside the arena `ranges` (both lists of half-open element ranges)."""
    out = []
    for lo, hi in ranges:
        for a, b in buckets:
            a2, b2 = max(a, lo), min(b, hi)
            if a2 < b2:
                out.append((a2, b2))
    return sorted(out)


SPAN_GAP_MAX = int(os.environ.get("TC_DDP_SPAN_GAP_MAX", str(2 << 20)))     # elements: a gap of dead (grad-less, zero) words up to this size is sent along rather than starting a new collective.  8 MB of zeros cost a one-link ring about what a collective's own latency does (2 (N-1) hops x 6 us at N = 8 = 84 us x 153 GB/s / 1.75); the 8 M elements of round 5 put 32 MB of zeros on the wire to save one


def comm_schedule(model):
    """ONE collective per stop of the split backward sweep (the nine bucket collectives of round 4 cost ~75 us each
    even on a 1-rank communicator and 2 (N-1) ring hops each on N ranks).  For every piece of model.gradient_pieces(), in order:
      * its live buckets are merged across gaps that hold only grad-less words (zeros in every rank's arena: sending them is harmless)
        up to SPAN_GAP_MAX elements -- never across words that belong to a LATER piece (they are not final yet and would be reduced twice);
      * the largest merged run is the piece's collective ("span"); smaller stragglers of at most COALESCE_MAX elements in all are
        deferred to the last piece;
      * the last piece (nothing left to hide it under) travels packed through a staging buffer ("pack"), stragglers included.
    Returns [(stop, [("span", a, b) | ("pack", [(a, b), ...]), ...]), ...]; every live word appears in exactly one entry."""
    live = gradient_buckets(model)
    pieces = model.gradient_pieces()

    def dead_only(x, y):
        return not any(a < y and x < b for a, b in live)

    sched, deferred = [], []
    for pi, (stop, ranges) in enumerate(pieces):
        bs = clip_buckets(live, ranges)
        runs = []
        for a, b in bs:
            if runs and (a == runs[-1][1] or (a - runs[-1][1] <= SPAN_GAP_MAX and dead_only(runs[-1][1], a))):
                runs[-1][1] = b
            else:
                runs.append([a, b])
        runs = [(a, b) for a, b in runs]
        if pi == len(pieces) - 1:
            allr = sorted(runs + deferred)
            if not allr:                                   #  nothing live in the last piece and nothing deferred: no collective, not an empty pack
                sched.append((stop, []))
            elif len(allr) == 1:
                sched.append((stop, [("span",) + allr[0]]))
            elif sum(b - a for a, b in allr) <= COALESCE_MAX:
                sched.append((stop, [("pack", allr)]))
            else:
                sched.append((stop, [("span", a, b) for a, b in allr]))
            continue
        if not runs:
            sched.append((stop, []))
            continue
        big = max(runs, key=lambda r: r[1] - r[0])
        small = [r for r in runs if r != big]
        if sum(b - a for a, b in small) <= COALESCE_MAX // 2:
            deferred += small
            sched.append((stop, [("span",) + big]))
        else:
            sched.append((stop, [("span", a, b) for a, b in runs]))
    return sched


def allreduce_scheduled(model, entries, group=None, async_op: bool = False):
    """Issues the collectives of one stop of comm_schedule(); returns the work handles (async_op) -- _PackedWork for a packed entry."""
    works = []
    if not comm_on(group):
        return works
    for e in entries:
        if e[0] == "span":
            w = dist.all_reduce(model._gflat[e[1]:e[2]], group=group, async_op=async_op)
            if async_op:
                works.append(w)
        else:
            w = _PackedWork(model._gflat, e[1], group, async_op)
            if async_op:
                works.append(w)
    return works


XGMI_LINK_GBS, XGMI_LINKS, RING_HOP_US = 153.0, 7, 6.0     # MI355X: 7 point-to-point links per GPU; per-hop latency of a ring step (assumed)


def comm_plan(model, n_ranks: int):
    """What a data-parallel step of `n_ranks` GPUs sends, without sending it: the pieces of the split backward sweep
    (model.gradient_pieces), the all-reduce buckets inside each (fp32 elements of the flat gradient arena, the grad-less tensors left
    out), and the time a ring all-reduce of each would take over xGMI -- a ring moves 2 (N-1)/N of the bytes through every GPU and is
    bound by ONE link per direction (153 GB/s) unless RCCL runs one ring per link (7), so both bounds are given, plus 2 (N-1) hops of
    latency per collective.  Lets the first multi-GPU run be read against an expectation."""
    out, tot, live = [], 0, 0
    f = 2.0 * (n_ranks - 1) / max(n_ranks, 1)
    lb = gradient_buckets(model)
    for stop, entries in comm_schedule(model):
        spans = [(e[1], e[2]) for e in entries if e[0] == "span"] + [r for e in entries if e[0] == "pack" for r in e[1]]
        nbytes = 4 * sum(b - a for a, b in spans)
        nlive = 4 * sum(max(0, min(b, y) - max(a, x)) for a, b in spans for x, y in lb)
        tot += nbytes
        live += nlive
        ncoll = len(entries)
        lat = 2 * (n_ranks - 1) * RING_HOP_US * 1e-3 * ncoll
        out.append({"sent_when_backward_reaches": stop or "end of backward (exposed)", "collectives": ncoll,
                    "how": [e[0] for e in entries],
                    "buckets_elements": [[int(a), int(b)] for a, b in spans], "megabytes": nbytes / 1e6, "live_megabytes": nlive / 1e6,
                    "ring_ms_one_link": f * nbytes / (XGMI_LINK_GBS * 1e9) * 1e3 + lat,
                    "ring_ms_seven_links": f * nbytes / (XGMI_LINK_GBS * XGMI_LINKS * 1e9) * 1e3 + lat})
    return {"ranks": n_ranks, "pieces": out, "gradient_megabytes_per_step": tot / 1e6, "live_gradient_megabytes_per_step": live / 1e6,
            "collectives_per_step": sum(p["collectives"] for p in out) + 1, "loss_sums_bytes": 28 * 4,
            "total_ring_ms_one_link": sum(p["ring_ms_one_link"] for p in out), "total_ring_ms_seven_links": sum(p["ring_ms_seven_links"] for p in out),
            "exposed_ring_ms_one_link": out[-1]["ring_ms_one_link"], "exposed_ring_ms_seven_links": out[-1]["ring_ms_seven_links"],
            "model": "ring all-reduce: 2 (N-1)/N x bytes per GPU over 153 GB/s per xGMI link (one ring) or 7 links (one ring per link), + 2 (N-1) "
                     "hops x 6 us per collective; every piece but the last travels under the rest of the backward sweep"}


class _PackedWork:
    """Several small, non-adjacent buckets sent as ONE collective: packed into a staging buffer, all-reduced, unpacked on wait()."""

    def __init__(self, grads, buckets, group, async_op):
        self.grads, self.buckets = grads, buckets
        self.flat = torch.cat([grads[a:b] for a, b in buckets])
        self.work = dist.all_reduce(self.flat, group=group, async_op=async_op)
        if not async_op:
            self._unpack()

    def _unpack(self):
        at = 0
        for a, b in self.buckets:
            self.grads[a:b].copy_(self.flat[at:at + b - a])
            at += b - a

    def wait(self):
        if self.work is not None:
            self.work.wait()
        self._unpack()


COALESCE_MAX = int(os.environ.get("TC_DDP_COALESCE_MAX", str(4 << 20)))     # elements: pieces up to this size travel as one collective


def allreduce_gradients(model, group=None, part: Optional[str] = None, async_op: bool = False, ranges=None, coalesce: bool = False):
    """C1: all-reduce(sum) of the live parts of the flat gradient arena over RCCL/xGMI (gloo in CPU tests): a handful of
    large buckets, every rank the same ones (the used set is a property of the architecture).  part="late" / "early" sends only
    the buckets at or above / below model.late_gradient_offset() (bridge + decoders / encoder); async_op returns the work
    handles instead of waiting, so the late part can travel under the encoder's backward.
    coalesce: a piece of several small non-adjacent buckets (the LAST piece of the split sweep: three ranges, 2.7 MB, nothing left to
    hide it under) goes as one collective through a packed staging buffer -- every collective costs 2 (N-1) ring hops of latency."""
    works = []
    if comm_on(group):
        buckets = gradient_buckets(model)
        if part is not None:
            early, late = split_buckets(buckets, model.late_gradient_offset())
            buckets = late if part == "late" else early
        if ranges is not None:                           # one piece of a split backward sweep (model.gradient_pieces)
            buckets = clip_buckets(buckets, ranges)
        if coalesce and len(buckets) > 1 and sum(b - a for a, b in buckets) <= COALESCE_MAX:
            w = _PackedWork(model._gflat, buckets, group, async_op)
            return [w] if async_op else []
        for a, b in buckets:
            w = dist.all_reduce(model._gflat[a:b], group=group, async_op=async_op)
            if async_op:
                works.append(w)
    return works


def train_step(model, loss_fn: SegLoss, opt: _FusedOptimizer, images: torch.Tensor, labels: torch.Tensor, group=None):
    """One step with trainer.py semantics; returns (loss, ce, dice) tensors (no host sync)."""
    opt.zero_grad()
    _wire_loss_scale(loss_fn, opt, images.device)
    logits = model(images)
    loss, ce, dice = loss_fn(logits, labels)
    loss.backward()
    allreduce_gradients(model, group)
    opt.step()
    return loss, ce, dice


# Only the capturing thread is held to the capture rules: the RCCL watchdog thread polls events and the input pipeline's reader
# thread page-locks staging buffers while a step is being captured.
_CAPTURE_MODE = "thread_local"


def graph_kernel_nodes(g) -> Optional[int]:
    """Kernel nodes of a captured hipGraph (hipGraphGetNodes / hipGraphNodeGetType on the raw handle; the graph must have been
    created with keep_graph=True).  None when the runtime does not expose it."""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
        raw = C.c_void_p(g.raw_cuda_graph())
        n = C.c_size_t(0)
        if hip.hipGraphGetNodes(raw, None, C.byref(n)) != 0:
            return None
        arr = (C.c_void_p * max(n.value, 1))()
        if hip.hipGraphGetNodes(raw, arr, C.byref(n)) != 0:
            return None
        k, t = 0, C.c_int(-1)
        for i in range(n.value):
            if hip.hipGraphNodeGetType(C.c_void_p(arr[i]), C.byref(t)) == 0 and t.value == 0:       # hipGraphNodeTypeKernel
                k += 1
        return k
    except Exception:
        return None


def _new_graph():
    try:
        return torch.cuda.CUDAGraph(keep_graph=True)             # keeps the hipGraph_t so that its nodes can be counted
    except TypeError:
        return torch.cuda.CUDAGraph()


def _instantiate(g):
    if hasattr(g, "instantiate"):
        try:
            g.instantiate()
        except Exception:
            pass


class GraphedStep:
    """A whole training step captured into hipGraphs and replayed: ~1800 kernel launches per step become graph launches,
    removing the host from the loop.  Inputs are copied into static buffers; the learning rate is a device scalar
    (FusedSGD.set_lr).  The loss's scalars -- w_ce, w_dice, focal_gamma, overlap, tversky_alpha, tversky_beta -- are kernel arguments
    and keep the values of the capture: changing them needs a new GraphedStep (the class weights live in device memory and do not, and
    neither does the top-k fraction: SegLoss.set_topk).

    world == 1: ONE graph = zero_grad + forward + loss + backward + SGD (through torch.autograd).
    world  > 1: no collective is ever captured.  Three graphs with the two RCCL all-reduces between them, driven through
    the engine directly (no autograd):  A = zero_grad + forward + per-pixel softmax / CE / Dice partial sums;
    all-reduce(28 floats);  B1 = loss gradient + backward of decoders and bridge;  async all-reduce of their gradient buckets
    (72 % of the live bytes) on the collective stream while B2 = the encoder's backward runs;  all-reduce of the encoder
    buckets;  C = fused SGD."""

    def __init__(self, model, loss_fn: SegLoss, opt: FusedSGD, images: torch.Tensor, labels: torch.Tensor, group=None, warmup: int = 3,
                 force_split: bool = False, pre=None):
        """pre(x, y): launches (on the current stream) that FILL the step's static inputs, captured at the head of the step's first graph
        -- the device input pipeline's augmentation / resize kernels reading one raw batch slot (data.DeviceLoader.iter_raw): a
        loader-fed loop is then graph launch after graph launch, with no eager launch in between."""
        self.model, self.loss_fn, self.opt, self.group = model, loss_fn, opt, group
        self._pre = pre
        self._topk = None                                # top-k CE: (value map, select scratch), allocated by the first _fwd
        self.x, self.y = images.clone(), labels.clone().long().contiguous()
        self._dtype = model.compute_dtype                # the captured launches hold pointers into this storage type's working copy
        _wire_loss_scale(loss_fn, opt, images.device)
        if getattr(loss_fn, "ce_topk", None) is not None:
            loss_fn.topk_state(images.device)            # exists before anything is captured
        self.distributed = comm_on(group)
        self.split = self.distributed or force_split
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                if self.split:
                    self._fwd(); self._reduce_sums(); self._bwd(); self._bwd_rest(); allreduce_gradients(model, group); opt.step()
                else:
                    self._whole_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.g_main = _new_graph()
        if not self.split:
            with torch.cuda.graph(self.g_main, capture_error_mode=_CAPTURE_MODE):
                self._whole_step()
            self.g_bwd = self.g_bwd_rest = self.g_opt = None
        else:
            with torch.cuda.graph(self.g_main, capture_error_mode=_CAPTURE_MODE):
                self._fwd()
            self._reduce_sums()
            self.g_bwd = _new_graph()
            with torch.cuda.graph(self.g_bwd, capture_error_mode=_CAPTURE_MODE):
                self._bwd()
            # the encoder's sweep in legs (stage 4, stage 3, the rest): each leg's gradients travel while the next leg runs
            self._pieces = model.gradient_pieces()
            self.g_bwd_legs = []
            for until, _ in self._pieces[1:]:
                g = _new_graph()
                with torch.cuda.graph(g, capture_error_mode=_CAPTURE_MODE):
                    self._bwd_leg(until)
                self.g_bwd_legs.append(g)
            self.g_bwd_rest = self.g_bwd_legs[-1]
            self._sched = comm_schedule(model)
            assert [st for st, _ in self._sched] == [st for st, _ in self._pieces]
            allreduce_gradients(model, group)
            self.g_opt = _new_graph()
            with torch.cuda.graph(self.g_opt, capture_error_mode=_CAPTURE_MODE):
                opt.step()
        for g in [self.g_main, self.g_bwd, self.g_opt] + (self.g_bwd_legs if self.split else []):
            if g is not None:
                _instantiate(g)

    def kernel_nodes(self) -> Optional[int]:
        """Kernel launches of one replayed step = kernel nodes of its captured graph(s)."""
        ks = [graph_kernel_nodes(g) for g in [self.g_main, self.g_bwd, self.g_opt] + (self.g_bwd_legs if self.split else []) if g is not None]
        return None if any(k is None for k in ks) else sum(ks)

    def _whole_step(self):
        """One process, no exchange: the same engine-driven pieces back to back in one graph (the loss kernels read the token-major
        logits of the classifier directly; train_step's nn.Module boundary would add the NCHW transpose and fp32 copies both ways)."""
        self._fwd()
        self._npix = self._npix_local
        self._bwd()
        self._bwd_rest()
        self.opt.step()

    # ---- the three pieces of the split step (engine driven directly; no torch.autograd in between)
    def _fwd(self):
        M, L = self.model, lib()
        M._ensure_flat(self.x.device)
        if self._pre is not None:
            self._pre(self.x, self.y)
        self.opt.zero_grad()
        logits, G, out_var = M._run(self.x, record=True, token_logits=True)     # [B*H*W, classes], storage type: no transpose, no fp32 copy
        self._G, self._out_var = G, out_var
        B, H, W = self.x.shape[0], self.x.shape[2], self.x.shape[3]
        C = logits.shape[1]
        assert logits.shape[0] == B * H * W and logits.stride(1) == 1
        stream = torch.cuda.current_stream(logits.device).cuda_stream
        self._logits, self._shape = logits, (B, C, H, W)           # (no probability map: the backward recomputes the softmax)
        self._sums = torch.zeros(1 + 3 * C, dtype=torch.float32, device=logits.device)
        route = self.loss_fn._route(logits.device)                 # (weights, ignore_index): the class-weighted / ignoring entries
        if route is None:
            L.tc_seg_loss_fwd_tok(logits.data_ptr(), logits.stride(0), self.y.data_ptr(), None, self._sums.data_ptr(), B, C, H * W,
                                  _dt(logits), stream)
        elif len(route) == 2:
            L.tc_seg_loss_fwd_w(logits.data_ptr(), logits.stride(0), self.y.data_ptr(), route[0].data_ptr(), route[1], None,
                                self._sums.data_ptr(), B, C, H * W, _dt(logits), stream)
        elif len(route) == 6:                  # focal CE / Tversky overlap: the scalars are baked into the captured launches
            L.tc_seg_loss_fwd_ft(logits.data_ptr(), logits.stride(0), self.y.data_ptr(), route[0].data_ptr(), route[1], route[2],
                                 OVERLAPS[route[3]], None, self._sums.data_ptr(), B, C, H * W, _dt(logits), stream)
        else:                                  # top-k CE: value map and scratch held for the life of the step; this rank's select runs here,
            if self._topk is None:             # BEFORE the sums travel, and leaves its share of the global CE in sums[0]
                self._topk = _topk_buffers(B * H * W, logits.device)
            L.tc_seg_loss_fwd_topk(logits.data_ptr(), logits.stride(0), self.y.data_ptr(), route[0].data_ptr(), route[1], route[2],
                                   OVERLAPS[route[3]], None, self._sums.data_ptr(), self._topk[0].data_ptr(), B, C, H * W, _dt(logits), stream)
            L.tc_topk_select(self._topk[0].data_ptr(), B * H * W, route[6].data_ptr(), self._sums.data_ptr(), _inv_world(self.group),
                             self._topk[1].data_ptr(), stream)
        self._npix_local = float(B * H * W)

    def _reduce_sums(self):
        self._sums, self._npix, _ = seg_sums_allreduce(self._sums, self._npix_local, self.group)

    def _bwd(self):
        M, L = self.model, lib()
        B, C, H, W = self._shape
        lf, lg = self.loss_fn, self._logits
        route = lf._route(lg.device)
        self.out = tuple(t.float() for t in loss_from_sums(self._sums, self._npix, lf.w_ce, lf.w_dice, None if route is None else route[0],
                                                           **_overlap_of(route)))
        stream = torch.cuda.current_stream(lg.device).cuda_stream
        # the gradient of the token-major logits, in the logits' own layout (their rows are padded to 16 bytes when the fused LayerNorm +
        # classifier produced them: Graph.ln_cls)
        d = torch.empty((B * H * W, lg.stride(0)), dtype=self.model.compute_dtype, device=lg.device)[:, :C]
        # a DynamicLossScale is read from its device state (word 0) by the kernel: the scale of every replay is the one the last left
        dyn = isinstance(lf.loss_scale, DynamicLossScale)
        gscale, gscale_dev = (1.0, lf.loss_scale.state(lg.device).data_ptr()) if dyn else (float(lf.loss_scale), None)
        if route is None:
            L.tc_seg_loss_bwd_tok(None, lg.data_ptr(), lg.stride(0), self.y.data_ptr(), self._sums.data_ptr(), d.data_ptr(), d.stride(0), B, C,
                                  H * W, float(lf.w_ce), float(lf.w_dice), float(self._npix), gscale, gscale_dev, _dt(d), stream)
        elif len(route) == 2:                  # the CE denominator comes from the (all-reduced) sums: no pixel count is passed
            L.tc_seg_loss_bwd_w(None, lg.data_ptr(), lg.stride(0), self.y.data_ptr(), route[0].data_ptr(), route[1], self._sums.data_ptr(),
                                d.data_ptr(), d.stride(0), B, C, H * W, float(lf.w_ce), float(lf.w_dice), gscale, gscale_dev, _dt(d), stream)
        elif len(route) == 6:
            w, ii, gamma, overlap, alpha, beta = route
            L.tc_seg_loss_bwd_ft(None, lg.data_ptr(), lg.stride(0), self.y.data_ptr(), w.data_ptr(), ii, self._sums.data_ptr(), d.data_ptr(),
                                 d.stride(0), B, C, H * W, float(lf.w_ce), float(lf.w_dice), gamma, OVERLAPS[overlap], alpha, beta, gscale,
                                 gscale_dev, _dt(d), stream)
        else:
            w, ii, gamma, overlap, alpha, beta, state = route
            L.tc_seg_loss_bwd_topk(None, lg.data_ptr(), lg.stride(0), self.y.data_ptr(), w.data_ptr(), ii, self._sums.data_ptr(), d.data_ptr(),
                                   d.stride(0), B, C, H * W, float(lf.w_ce), float(lf.w_dice), gamma, OVERLAPS[overlap], alpha, beta, gscale,
                                   gscale_dev, self._topk[0].data_ptr(), state.data_ptr(), _inv_world(self.group), _dt(d), stream)
        M._backward(self._G, self._out_var, d, until="encoder_done")     # loss gradient, decoders, bridge

    def _bwd_leg(self, until: Optional[str]):
        self.model._backward_continue(self._G, until)                   # one leg of the encoder's sweep (None: to the end)
        if until is None:
            self._G = self._out_var = None

    def _bwd_rest(self):
        self._bwd_leg(None)                                             # the whole encoder in one go

    def __call__(self, images: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None, comm: bool = True):
        """comm=False replays the same graphs without the collectives between them (bench.py: the time the all-reduces add to a
        step is the difference; the ranks' parameters diverge, so it is a timing aid only)."""
        if self.model.compute_dtype != self._dtype:
            raise RuntimeError("the model's compute dtype changed after this step was captured: capture a new GraphedStep")
        if images is not None and images.data_ptr() != self.x.data_ptr():     # a loader may write straight into self.x / self.y
            self.x.copy_(images, non_blocking=True)
            self.y.copy_(labels, non_blocking=True)
        self.g_main.replay()
        if self.split:
            works = []
            if comm:
                self._reduce_sums()                  # C2: in place on the static 28-float buffer
            self.g_bwd.replay()
            if comm:                                 # C1, bridge + decoders: ONE collective (comm_schedule); the collective stream waits for g_bwd only
                works = allreduce_scheduled(self.model, self._sched[0][1], self.group, async_op=True)
            for g, (until, entries) in zip(self.g_bwd_legs, self._sched[1:]):
                g.replay()                           # stages 4 + 3, rest of the encoder: each leg's collective leaves under the next leg
                if comm:                             # (the last piece has nothing to hide under: everything left goes packed as ONE collective)
                    works += allreduce_scheduled(self.model, entries, self.group, async_op=True)
            for w in works:
                w.wait()                                     # the compute stream waits for the collectives, the host does not
            self.g_opt.replay()
        return self.out

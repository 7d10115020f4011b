"""`trainer_synapse` of the reference (trainer.py:49-237) on the MI355X path: the same schedule, loss, optimiser, checkpoint
cadence and evaluation calls, with the device input pipeline in place of `Synapse_dataset` + `DataLoader` and the captured
training step in place of the per-iteration Python loop body.

What is kept from the reference loop:
  * global batch = batch_size * n_gpu (trainer.py:86) -- here batch_size per rank, one process per GPU;
  * loss 0.4 CE + 0.6 Dice (trainer.py:141-143) -- with focal_gamma / overlap="tversky" set, 0.4 focal CE + 0.6 Tversky, and the log line's
    loss_ce / loss_dice are then those two terms --, SGD(momentum 0.9, weight_decay 1e-4) (:125) -- or, by TrainConfig.optimizer, AdamW / Adam
    (train.FusedAdamW) under the same schedule, clipping, loss scale and skip logging; base_lr is used as given, and its default 0.05 is SGD's value;
  * CosineAnnealingLR(T_max = max_epochs * len(loader)) stepped every iteration (:126-127,151-153), or the polynomial decay
    base_lr (1 - iter/max_iter)^0.9 when use_scheduler is off (:154-157); optional clip_grad_norm_(5) (:147-148);
  * the learning-rate scaling quirk of the launcher (train_MSTransception.py:123-124) as `scaled_base_lr`;
  * checkpoints `<model_name>_epoch_<n>.pth` = `state_dict()` at the reference's epochs (:180-214), each followed by `inference`
    when evaluation volumes are given, and always after the last epoch.
Not kept: TensorBoard writers and the matplotlib/CSV result plots (:216-237).
"""
from __future__ import annotations

import contextlib
import logging
import inspect
import math
import os
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Union

import torch
import torch.distributed as dist

from .data import DeviceLoader, SynapseSlices
from .evaluate import (RESAMPLE_MODES, SURFACE_KEYS, TTA, VALID_OPTION, Calibration, PostProcess, SurfaceMetrics, calibration_from_stats,
                       calibration_line, inference, inference_calibration, inference_report)
from .train import (DynamicLossScale, FusedAdamW, FusedSGD, GraphedStep, SegLoss, WeightEMA, check_ce_topk, check_class_weights, check_ema_decay,
                    check_focal_tversky, check_ignore_index, cosine_lr, train_step)

OPTIMIZERS = ("sgd", "adamw", "adam")


@dataclass
class TrainConfig:
    root_path: str
    list_dir: str
    num_classes: int = 9
    max_epochs: int = 400
    batch_size: int = 24               # per GPU (train_MSTransception.py:35-36)
    base_lr: float = 0.05              # SGD's value (train_MSTransception.py); it is used as given under every optimizer, never rescaled
                                       # for one -- AdamW / Adam want something near 1e-3
    img_size: int = 224
    seed: int = 1234
    eval_interval: int = 20
    model_name: str = "transCeption"
    grad_clipping: bool = False
    use_scheduler: bool = True
    augment: bool = True
    graphed: bool = True               # replay the captured step (hipGraph); False launches every kernel from Python
    device_metrics: bool = False       # Dice / HD95 of the evaluation on the GPU (evaluate.metrics_device) instead of scipy on the host
    voxelspacing: Optional[tuple] = None   # (z, y, x) voxel size for the HD95 of the evaluation, on either metric path; None: in voxels
    postprocess: Optional[PostProcess] = None   # connected-component post-processing of the evaluation's predictions (evaluate.PostProcess); None: none
    # test-time augmentation of the evaluation (evaluate.TTA: flip / transpose views whose class probabilities are averaged); None: one pass.
    # Keyword-only, so the positional order of the fields around it is what it was
    tta: Optional[TTA] = field(default=None, kw_only=True)
    log_every: int = 1                 # iterations between log lines (each one reads three scalars back from the GPU)
    loss_scale: Union[None, float, str] = None   # float16 storage: None = no scale (1), a number = static scale, "dynamic" = a default
                                       # train.DynamicLossScale (device-resident, adjusts itself inside the captured step)
    class_weights: Optional[tuple] = None  # num_classes weights >= 0, not all zero, used as BOTH the CrossEntropyLoss weight and the Dice weight
    ignore_index: Optional[int] = None     # a label value outside [0, num_classes) (e.g. 255) whose pixels count in neither loss term
    optimizer: str = "sgd"             # "sgd": the reference's SGD(momentum 0.9); "adamw" / "adam": train.FusedAdamW, decoupled / coupled decay
    weight_decay: Optional[float] = None   # None: 1e-4 for sgd (trainer.py:125), 1e-2 for adamw / adam (torch's AdamW default)
    betas: tuple = (0.9, 0.999)        # adamw / adam
    adam_eps: float = 1e-8             # adamw / adam
    no_decay: Optional[str] = None     # adamw / adam: "norm_bias" = no decay on tensors with ndim <= 1 (norm affine parameters and biases)
    ema_decay: Optional[float] = None  # a number in [0, 1): keep an exponential moving average of the weights (train.WeightEMA) inside the step
    ema_warmup: bool = True            # the n-th update uses min(ema_decay, (1 + n) / (10 + n))
    ema_eval: bool = True              # evaluate the averaged weights (BatchNorm statistics stay the live ones) instead of the last iterate

    def __post_init__(self):
        if self.optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {OPTIMIZERS}, got {self.optimizer!r}")
        wd = self.weight_decay
        if wd is not None and (isinstance(wd, bool) or not isinstance(wd, (int, float)) or not math.isfinite(wd) or wd < 0):
            raise ValueError(f"weight_decay must be None or a finite number >= 0, got {wd!r}")
        try:
            b1, b2 = self.betas
            ok = all(isinstance(b, (int, float)) and not isinstance(b, bool) and 0.0 <= b < 1.0 for b in (b1, b2))
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"betas must be two numbers in [0, 1), got {self.betas!r}")
        e = self.adam_eps
        if isinstance(e, bool) or not isinstance(e, (int, float)) or not math.isfinite(e) or e <= 0:
            raise ValueError(f"adam_eps must be a finite number > 0, got {e!r}")
        if self.no_decay not in (None, "norm_bias"):
            raise ValueError(f'no_decay must be None or "norm_bias", got {self.no_decay!r}')
        if self.no_decay is not None and self.optimizer == "sgd":
            raise ValueError("no_decay needs optimizer=\"adamw\" or \"adam\": the SGD kernel takes one decay for all segments")
        if not VALID_OPTION["postprocess"](self.postprocess):
            raise ValueError(f"postprocess must be None or an evaluate.PostProcess, got {self.postprocess!r}")
        if not VALID_OPTION["tta"](self.tta):
            raise ValueError(f"tta must be None or an evaluate.TTA, got {self.tta!r}")
        if not VALID_OPTION["resample"](self.resample):
            raise ValueError(f"resample must be one of {RESAMPLE_MODES}, got {self.resample!r}")
        if not VALID_OPTION["surface"](self.surface_metrics):
            raise ValueError(f"surface_metrics must be None or an evaluate.SurfaceMetrics, got {self.surface_metrics!r}")
        if self.surface_metrics is not None:
            self.surface_metrics.tolerances(self.num_classes)         # one tolerance, or one per class 1..num_classes-1
        if not VALID_OPTION["calibration"](self.calibration):
            raise ValueError(f"calibration must be None or an evaluate.Calibration, got {self.calibration!r}")
        check_focal_tversky(self.focal_gamma, self.overlap, self.tversky_alpha, self.tversky_beta)
        check_ce_topk(self.ce_topk, self.num_classes)
        make_loss_scale(self.loss_scale)
        check_class_weights("class_weights", self.class_weights, self.num_classes, need_positive=True)
        check_ignore_index(self.ignore_index, self.num_classes)
        if self.ema_decay is not None:
            check_ema_decay(self.ema_decay)


# Options that are keyword-only, validated in `__post_init__` and kept as plain attributes beside the dataclass fields: the field list -- the
# positional order and eq of the configuration, which ends with the ema_* fields -- is what it was.  (name, type, default), in the
# order of the signature, which ends with `resample`.  What follows from that: `==` compares the fields only, so two configurations that differ
# in these options alone compare equal, and `dataclasses.replace` / `asdict` do not carry them (a replaced copy has the defaults: pass them
# again).  `repr` does show them, after the fields.
#   surface_metrics: an evaluate.SurfaceMetrics -- the evaluation after a checkpoint then runs `inference_report` and `hist["surface"]` collects
#     its overall ASD / ASSD / HD / surface Dice beside `hist["dice"]` and `hist["hd95"]`; None: `inference`, as before;
#   calibration: an evaluate.Calibration -- the evaluation after a checkpoint then also runs `inference_calibration` on the rank's share of the
#     volumes (one more prediction pass per volume), the decoded statistics are all-reduced as one float64 vector and `hist["calibration"]`
#     collects the pool's ECE / MCE / NLL / Brier / accuracy with its reliability table; None: no key, no pass, no launch;
#   ce_topk: None, or a fraction in (0, 1] -- the cross-entropy is then the mean of that fraction's largest per-pixel terms only (train.SegLoss,
#     include/transception_topk.h) and the log line's loss_ce is that top-k CE; None: no launch, no allocation, the calls made today;
#   focal_gamma, overlap, tversky_alpha, tversky_beta: the loss (train.SegLoss has the definition) -- the focal exponent of the
#     cross-entropy, "dice" or "tversky" for the overlap term, and the Tversky weights of false positives and false negatives;
#   resample: what the evaluation resamples to the label's size (evaluate.evaluate_volume: "labels", the reference's order-0 zoom of the
#     argmax, or "scores", bilinear class scores and then the argmax).
KEYWORD_OPTIONS = (("surface_metrics", Optional[SurfaceMetrics], None), ("calibration", Optional[Calibration], None),
                   ("ce_topk", Optional[float], None), ("focal_gamma", float, 0.0), ("overlap", str, "dice"), ("tversky_alpha", float, 0.5), ("tversky_beta", float, 0.5),
                   ("resample", str, "labels"))


def _keyword_only_options(cls):
    """`TrainConfig(..., focal_gamma=2.0, overlap="tversky", resample="scores")`: KEYWORD_OPTIONS on the dataclass's `__init__`."""
    init = cls.__init__
    defaults = {name: default for name, _, default in KEYWORD_OPTIONS}

    def __init__(self, *args, **kwargs):
        for name, default in defaults.items():
            setattr(self, name, kwargs.pop(name, default))
        init(self, *args, **kwargs)

    sig = inspect.signature(init)
    extra = [inspect.Parameter(name, inspect.Parameter.KEYWORD_ONLY, default=default, annotation=t) for name, t, default in KEYWORD_OPTIONS]
    __init__.__signature__ = sig.replace(parameters=[*sig.parameters.values(), *extra])
    __init__.__qualname__ = init.__qualname__
    cls.__init__ = __init__
    fields_repr = cls.__repr__

    def __repr__(self):
        return fields_repr(self)[:-1] + "".join(f", {name}={getattr(self, name)!r}" for name in defaults) + ")"

    cls.__repr__ = __repr__
    for name, default in defaults.items():
        setattr(cls, name, default)               # the defaults, readable on the class as a field's would be
    return cls


TrainConfig = _keyword_only_options(TrainConfig)


def make_loss_scale(spec) -> Union[float, DynamicLossScale]:
    """TrainConfig.loss_scale -> what SegLoss takes.  Anything but None, a positive finite number or "dynamic" is a ValueError."""
    if spec is None:
        return 1.0
    if spec == "dynamic":
        return DynamicLossScale()
    if isinstance(spec, (int, float)) and not isinstance(spec, bool) and math.isfinite(spec) and spec > 0:
        return float(spec)
    raise ValueError(f'loss_scale must be None, a positive finite number or "dynamic", got {spec!r}')


def make_optimizer(cfg: TrainConfig, model):
    """The optimiser TrainConfig asks for.  "sgd" is the reference's, built with the arguments it always had."""
    clip = 5.0 if cfg.grad_clipping else None
    if cfg.optimizer == "sgd":
        return FusedSGD(model, lr=cfg.base_lr, momentum=0.9, weight_decay=1e-4 if cfg.weight_decay is None else cfg.weight_decay, clip_norm=clip)
    return FusedAdamW(model, lr=cfg.base_lr, betas=tuple(cfg.betas), eps=cfg.adam_eps, weight_decay=1e-2 if cfg.weight_decay is None else cfg.weight_decay,
                      decoupled=cfg.optimizer == "adamw", clip_norm=clip, no_decay=cfg.no_decay)


def scaled_base_lr(base_lr: float, batch_size: int) -> float:
    """train_MSTransception.py:123-124: the learning rate is rescaled only when batch_size != 24 and batch_size % 5 == 0."""
    return base_lr * batch_size / 24 if batch_size != 24 and batch_size % 5 == 0 else base_lr


def checkpoint_epochs(max_epoch: int, eval_interval: int) -> List[int]:
    """Epochs after which the reference saves + evaluates (trainer.py:180-214)."""
    out = []
    for e in range(max_epoch):
        early = e >= int(max_epoch / 2) and e < int(max_epoch - 100) and (e + 1) % 20 == 0
        late = e >= int(max_epoch - 100) and (e + 1) % eval_interval == 0
        if early or late or e >= max_epoch - 1:
            out.append(e)
    return out


def trainer_synapse(cfg: TrainConfig, model, snapshot_path: str, volumes: Optional[Callable[[], list]] = None, group=None,
                    log: Optional[Callable[[str], None]] = None) -> dict:
    """Trains `model` (a transception_amd.MSTransception on the GPU) and returns the history.  `volumes` is a callable that
    yields the evaluation volumes as (image, label, case) triples (the `.npy.h5` reader needs h5py, see data.SynapseSlices).
    Under optimizer="adamw" / "adam" the history also holds "optimizer_step", the updates the device counted as applied.
    With ema_decay set it holds "ema_checkpoints" (`<model_name>_ema_epoch_<n>.pth`, the averaged weights, written beside every plain
    checkpoint) and "ema_updates", the updates the device averaged in; the evaluation then runs on the averaged weights (ema_eval)."""
    log = log or logging.info
    distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1
    rank = dist.get_rank(group) if distributed else 0
    world = dist.get_world_size(group) if distributed else 1
    dev = next(model.parameters()).device
    os.makedirs(snapshot_path, exist_ok=True)
    ds = SynapseSlices(cfg.root_path, cfg.list_dir, split="train")
    loader = DeviceLoader(ds, cfg.batch_size, img_size=cfg.img_size, device=dev, seed=cfg.seed, rank=rank, world=world,
                          augment=cfg.augment, epochs=cfg.max_epochs)
    per_epoch = len(loader) // cfg.max_epochs            # >= 1 for a non-empty set: data.rank_batches completes the last global batch
    max_iterations = cfg.max_epochs * per_epoch
    log("The length of train set is: {}".format(len(ds)))
    log("{} iterations per epoch. {} max iterations ".format(per_epoch, max_iterations))
    model.train()
    loss_scale = make_loss_scale(cfg.loss_scale)
    scaler = loss_scale if isinstance(loss_scale, DynamicLossScale) else None
    loss_fn = SegLoss(cfg.num_classes, group=group, loss_scale=loss_scale, ce_weight=cfg.class_weights, dice_weight=cfg.class_weights,
                      ignore_index=cfg.ignore_index, focal_gamma=cfg.focal_gamma, overlap=cfg.overlap, tversky_alpha=cfg.tversky_alpha,
                      tversky_beta=cfg.tversky_beta, **({} if cfg.ce_topk is None else {"ce_topk": cfg.ce_topk}))
    opt = make_optimizer(cfg, model)
    ema = None
    if cfg.ema_decay is not None:
        ema = opt.ema = WeightEMA(model, decay=cfg.ema_decay, warmup=cfg.ema_warmup)

    def lr_at(it: int) -> float:
        """Learning rate of step `it` (0-based).  Cosine: scheduler.step() follows every optimizer.step() (trainer.py:151-153).
        Polynomial: the reference computes lr_ from iter_num BEFORE incrementing it and assigns it for the NEXT step (:154-159),
        so steps 0 and 1 both run at base_lr and step k at base_lr (1 - (k-1)/max)^0.9."""
        if cfg.use_scheduler:
            return cosine_lr(cfg.base_lr, it, max_iterations)
        return cfg.base_lr * (1.0 - max(it - 1, 0) / max_iterations) ** 0.9

    if distributed:
        # identical replicas before the first step (the reference's DataParallel re-broadcasts rank 0's weights every forward,
        # trainer.py:110-111): parameters and BatchNorm statistics come from rank 0
        model._ensure_flat(dev)
        dist.broadcast(model.flat_parameters(), src=0, group=group)
        model.invalidate_working_copy()
        for buf in model.buffers():
            dist.broadcast(buf, src=0, group=group)

    saves = set(checkpoint_epochs(cfg.max_epochs, cfg.eval_interval))
    hist = {"loss": [], "lr": [], "dice": [], "hd95": [], "checkpoints": []}
    if ema is not None:
        hist["ema_checkpoints"] = []
    if scaler is not None:
        hist["loss_scale"] = []                                   # the scale after the step of each log line
    if cfg.surface_metrics is not None:
        hist["surface"] = []                                      # per evaluation: inference_report's `overall`, {key: mean over cases and classes}
    if cfg.calibration is not None:
        hist["calibration"] = []                                  # per evaluation: the pool's calibration_from_stats dict
    step = None
    iter_num = 0
    for x, y in loader:
        opt.set_lr(lr_at(iter_num))
        if iter_num == 0 or not cfg.graphed:
            # the first iteration runs eagerly: it creates the optimiser state and workspaces the captured step then refers to
            # (capturing at step 0 would bake "first step" into the SGD kernel's arguments), and it counts as iteration 1
            loss, ce, dice = train_step(model, loss_fn, opt, x, y, group)
        else:
            if step is None:
                step = GraphedStep(model, loss_fn, opt, x, y, group, warmup=0)
                loader.out = (step.x, step.y)                     # later batches land in the step's static inputs: no copy per step
            loss, ce, dice = step(x, y)
        iter_num += 1
        if iter_num % cfg.log_every == 0:
            lv, cv, dv = float(loss.detach()), float(ce.detach()), float(dice.detach())
            hist["loss"].append(lv)
            hist["lr"].append(lr_at(iter_num))
            log('iteration %d : lr: %f, loss : %f, loss_ce: %f, loss_dice: %f' % (iter_num, lr_at(iter_num), lv, cv, dv))
            if scaler is not None:                                # read with the loss scalars above: no sync point of its own
                ls = scaler.state_dict()
                hist["loss_scale"].append(ls["scale"])
                if opt.last_step_skipped():                       # the scale has halved already; the count is the device's, every step in it
                    log('iteration %d : update SKIPPED, gradient norm not finite (%d skipped so far; dynamic loss scale now %g)'
                        % (iter_num, ls["skipped"], ls["scale"]))
            elif opt.last_step_skipped():                         # float16: a non-finite gradient norm skips the update (no weights were touched)
                log('iteration %d : update SKIPPED, gradient norm not finite (%d skipped so far; lower the loss scale if this persists)'
                    % (iter_num, opt.skipped_steps))
        if iter_num % per_epoch == 0:
            epoch_num = iter_num // per_epoch - 1
            if epoch_num in saves:
                if rank == 0:
                    path = os.path.join(snapshot_path, f'{cfg.model_name}_epoch_{epoch_num}.pth')
                    torch.save(model.state_dict(), path)
                    hist["checkpoints"].append(path)
                    log("save model to {}".format(path))
                    if ema is not None:
                        path = os.path.join(snapshot_path, f'{cfg.model_name}_ema_epoch_{epoch_num}.pth')
                        torch.save(ema.model_state_dict(), path)
                        hist["ema_checkpoints"].append(path)
                        log("save averaged model to {}".format(path))
                if volumes is not None:
                    # Every rank evaluates its share of the volumes with the replica the checkpoint holds (rank 0's BatchNorm statistics
                    # are broadcast first; the weights are identical already) and the per-case sums are all-reduced: no rank sits in a
                    # collective while another spends minutes in host-side HD95 (a process-group timeout would abort the job).
                    vols = list(volumes())
                    if distributed:
                        for buf in model.buffers():
                            dist.broadcast(buf, src=0, group=group)
                        vols = vols[rank::world]
                    res = torch.zeros(3 + (len(SURFACE_KEYS) if cfg.surface_metrics is not None else 0), dtype=torch.float64, device=dev)
                    if cfg.calibration is not None:               # the decoded slots: counts and sums, additive over the ranks
                        calib = torch.zeros(3 * cfg.calibration.bins + 4 + 3 * cfg.num_classes, dtype=torch.float64, device=dev)
                    if vols:
                        if rank == 0:
                            log(f"Running Inference after epoch {epoch_num}")
                        # the averaged weights are swapped into the arenas for the evaluation and out again (every rank holds the same average)
                        with ema.swapped() if ema is not None and cfg.ema_eval else contextlib.nullcontext():
                            options = dict(log=log, device_metrics=cfg.device_metrics, voxelspacing=cfg.voxelspacing, postprocess=cfg.postprocess,
                                           tta=cfg.tta, resample=cfg.resample)
                            if cfg.surface_metrics is None:
                                mean_dice, mean_hd95 = inference(model, vols, cfg.num_classes, cfg.img_size, **options)
                            else:
                                overall = inference_report(model, vols, cfg.num_classes, cfg.img_size, surface=cfg.surface_metrics, **options)["overall"]
                                mean_dice, mean_hd95 = overall["dice"], overall["hd95"]
                                res[3:] = torch.tensor([overall[key] * len(vols) for key in SURFACE_KEYS], dtype=torch.float64)
                            if cfg.calibration is not None:
                                pool = inference_calibration(model, vols, cfg.num_classes, cfg.img_size, log=log, tta=cfg.tta,
                                                             calibration=cfg.calibration)["overall"]
                                calib.copy_(torch.from_numpy(pool["stats"]))
                        res[0], res[1], res[2] = mean_dice * len(vols), mean_hd95 * len(vols), len(vols)
                        model.train()
                    if distributed:
                        dist.all_reduce(res, group=group)
                    hist["dice"].append(float(res[0] / res[2].clamp(min=1)))
                    hist["hd95"].append(float(res[1] / res[2].clamp(min=1)))
                    if cfg.surface_metrics is not None:           # all-reduced like the two means above
                        hist["surface"].append(dict(zip(SURFACE_KEYS, (res[3:] / res[2].clamp(min=1)).tolist())))
                    if cfg.calibration is not None:
                        if distributed:
                            dist.all_reduce(calib, group=group)
                        hist["calibration"].append(calibration_from_stats(calib.cpu().numpy(), cfg.calibration.bins, cfg.num_classes))
                        if distributed and rank == 0:             # the lines above are each rank's own share; this one is the pool of all ranks
                            log('Calibration over all ranks: ' + calibration_line(hist["calibration"][-1]))
    hist["iterations"] = iter_num
    if isinstance(opt, FusedAdamW):
        hist["optimizer_step"] = opt.device_step()                # updates applied, as the device counted them: iterations minus skipped
    if ema is not None:
        hist["ema_updates"] = ema.updates()                       # likewise: a skipped update is not averaged in
    return hist

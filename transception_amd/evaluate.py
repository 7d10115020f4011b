"""Evaluation of the TransCeption path on MI355X: the device side of the reference's
`test_single_volume` (utils.py:63-110) and `inference` (test.py:60-86).

The reference runs one slice at a time (batch 1, host sync per slice, `utils.py:67-88`).  Here the slices of a volume are
normalised and pushed through the eval-mode forward in batches, `argmax(softmax(logits))` and the per-class voxel counts of
the Dice score are one HIP kernel (`tc_argmax_counts`), and only the uint8 label map returns to the host.

The order-3 zoom of a slice to the network size and the order-0 zoom of the prediction back (`utils.py:69-70,83-84`) run on the
device too (`host_zoom=True` keeps scipy per slice, as the reference does).

The metric (`calculate_metric_percase`, `utils.py:50-60`) has two forms.  The default is the host one: HD95 is
`medpy.metric.binary.hd95` (`utils.py:55`; medpy is not installable here) restated from its published algorithm on scipy.ndimage --
surface voxels = mask minus its erosion (connectivity 1), distances by the Euclidean distance transform of the other mask's
surface, 95th percentile of both directions pooled.  Parity with medpy itself is unpinned; tests pin it to a brute-force
evaluation of that definition.  With `device_metrics=True` the prediction never leaves the GPU: `metrics_device` computes the
Dice counts and the same HD95 (connectivity 1) with the kernels of csrc/metrics.hip -- surface maps, a separable squared Euclidean
distance transform, the two order statistics of the squared distances met on the other surface -- and one small copy of
(counts, n, d2_lo, d2_hi) per volume returns to the host, which takes the square roots.  Without `voxelspacing` (unit spacing)
that is exact integer work: int32 maps and a histogram indexed by the squared distance.  With `voxelspacing` (medpy's argument:
one positive float per array axis, or a scalar for all) the maps are float64 and the order statistics come from a radix select
over the doubles' bit patterns; the sums of squares differ from scipy's by rounding only.  Both metric paths take it, through
`calculate_metric_percase`, `evaluate_volume`, `inference` and `TrainConfig.voxelspacing`.

Connected-component post-processing (`PostProcess`; the reference has no such step) removes stray islands from the prediction before
either metric: per class keep the largest component, or every component of at least N voxels.  `postprocess_device` runs it on the GPU
(csrc/postprocess.hip: a lock-free union-find, integer atomics only), `postprocess_host` is the same definition on scipy.ndimage.label;
include/transception_post.h states the definition.  `postprocess=None`, the default everywhere, changes nothing.

Test-time augmentation (`TTA`; the reference scores one forward pass per slice, but trains on every flipped and 90-degree-rotated
orientation, dataset_synapse.py:39-46) averages the class probabilities over flip / transpose views of the input before the argmax.  Per
view `tc_tta_view` makes the normalised view, the network runs, and `tc_tta_accumulate` reads the logits once and folds their softmax
into one fp32 accumulator at the un-transformed position -- or, for the last view, writes the label (csrc/tta.hip;
include/transception_tta.h states the definition).  `tta=None`, the default everywhere, changes nothing.

Evaluation at label resolution (`resample="scores"`; the reference carries it as a commented-out line, utils.py:81): instead of zooming the
argmax with order 0, the class scores -- the logits, or with `TTA` the summed probabilities -- are resampled bilinearly to the label's size and
the argmax is taken there.  `tc_resample_scores` reads the small score maps once, interpolates in registers and writes only the uint8 label
(csrc/resample.hip; include/transception_resample.h states the definition).  `resample="labels"`, the default everywhere, changes nothing.

Surface metrics (`SurfaceMetrics`; the reference reports Dice and HD95 only): ASD in both directions, ASSD, the surface Dice at a tolerance
and the full Hausdorff distance, with Jaccard, precision and recall from the counts.  `surface_metrics_device` runs `metrics_device`'s
per-class loop and, on the same two distance maps of every class, tc_surface_stats: the directed count, sum of distances, count within
the tolerance and largest squared distance (csrc/surface.hip; include/transception_surface.h states the definitions).
`surface_metrics_host` is the same from scipy; `evaluate_volume_report` and `inference_report` are `evaluate_volume` and `inference` with
these per-class dicts.  `evaluate_volume`, `inference` and the functions above them are what they were.

Uncertainty and calibration (`predict_uncertainty`, `Calibration`; the reference reduces its scores to an argmax): a second use of the fp32
probability accumulator of the views.  `tc_uncert_maps` reads class scores once -- a view's logits, or the summed probabilities -- and writes
the normalised predictive entropy, the maximum-probability confidence, the label and, from the sum of the views' own entropies, the mutual
information between the views.  `tc_calib_stats` reads scores and labels once and leaves the reliability table, the NLL and Brier sums and
the per-predicted-class entropy sums as 8-byte slots, from which `calibration_from_stats` forms ECE, MCE, NLL, Brier and accuracy
(csrc/uncertainty.hip; include/transception_uncertainty.h states the definitions).  Calibration is measured where the scores live, at the
network size, against labels brought there by `zoom_labels`; `calibration_host` is the same from NumPy in float64.  `evaluate_volume_calibration`
and `inference_calibration` are entries of their own: nothing above runs them, and `TrainConfig.calibration=None`, the default, changes nothing.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple, Union

import math

import numpy as np
import torch

from ._lib import (TC_CALIB_FOREGROUND, TC_CALIB_MAX_BINS, TC_CC_LARGEST, TC_CC_MIN_VOXELS, TC_F32, TC_METRIC_SELECT_WORK_BYTES,
                   TC_RESAMPLE_MAX_EXTENT, TC_SURFACE_WORK_BYTES, TC_TTA_FLIP_H, TC_TTA_FLIP_W, TC_TTA_TRANSPOSE, TC_UNCERT_LOGITS,
                   TC_UNCERT_PROB_SUMS, lib)
from .engine import TC_DTYPE

NO_CPU = "transception_amd.evaluate runs on MI355X only (no CPU fallback)"


def argmax_counts(logits: torch.Tensor, labels: Optional[torch.Tensor] = None,
                  counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """pred[b,h,w] = argmax_k logits[b,k,h,w] (uint8).  With `labels` (int64 [B,H,W]) the per-class counts
    (|pred==k & gt==k|, |pred==k|, |gt==k|) are ADDED to `counts` (float32 [ncls,3], created zeroed when None)."""
    if not logits.is_cuda:
        raise RuntimeError(NO_CPU)
    B, C, H, W = logits.shape
    lg = logits.contiguous().float()
    pred = torch.empty((B, H, W), dtype=torch.uint8, device=lg.device)
    lab = None
    if labels is not None:
        lab = labels.contiguous().long()
        if counts is None:
            counts = torch.zeros((C, 3), dtype=torch.float32, device=lg.device)
    stream = torch.cuda.current_stream(lg.device).cuda_stream
    lib().tc_argmax_counts(lg.data_ptr(), lab.data_ptr() if lab is not None else None, pred.data_ptr(),
                           counts.data_ptr() if counts is not None else None, B, C, H * W, TC_F32, stream)
    return pred, counts


def _percase(inter, p, g, hd95_fn: Callable[[], float]) -> Tuple[float, float]:
    """The reference's rule for one class of one volume (utils.py:50-60) from |P&G|, |P| and |G|: (Dice, hd95_fn()) when both are non-empty
    -- the distance is computed only then --, (1, 0) when only the prediction is non-empty, else (0, 0)."""
    if p > 0 and g > 0:
        return float(2.0 * inter / (p + g)), hd95_fn()
    if p > 0:
        return 1.0, 0.0
    return 0.0, 0.0


def dice_from_counts(counts: np.ndarray) -> List[float]:
    """Per-class Dice with calculate_metric_percase's conventions (utils.py:50-60) for classes 1..C-1:
    2|P&G|/(|P|+|G|) when both are non-empty, 1 when only the prediction is non-empty, else 0."""
    return [_percase(inter, p, g, lambda: 0.0)[0] for inter, p, g in np.asarray(counts, dtype=np.float64)[1:]]


def surface_distances(result: np.ndarray, reference: np.ndarray, voxelspacing=None, connectivity: int = 1) -> np.ndarray:
    """Distances from every surface voxel of `result` to the nearest surface voxel of `reference` (medpy __surface_distances)."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    if not result.any() or not reference.any():
        raise RuntimeError("surface distances need non-empty masks")
    footprint = generate_binary_structure(result.ndim, connectivity)
    result_border = result ^ binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ binary_erosion(reference, structure=footprint, iterations=1)
    dt = distance_transform_edt(~reference_border, sampling=voxelspacing)
    return dt[result_border]


def hd95(result: np.ndarray, reference: np.ndarray, voxelspacing=None, connectivity: int = 1) -> float:
    """95th percentile of the symmetric surface distances (medpy.metric.binary.hd95, called at utils.py:55)."""
    a = surface_distances(result, reference, voxelspacing, connectivity)
    b = surface_distances(reference, result, voxelspacing, connectivity)
    return float(np.percentile(np.hstack((a, b)), 95))


def calculate_metric_percase(pred: np.ndarray, gt: np.ndarray, voxelspacing=None) -> Tuple[float, float]:
    """(dice, hd95) of one class of one volume with the reference's conventions (utils.py:50-60); `voxelspacing` as `hd95` takes it."""
    pred, gt = pred > 0, gt > 0
    return _percase(np.logical_and(pred, gt).sum(), int(pred.sum()), int(gt.sum()), lambda: hd95(pred, gt, voxelspacing))


def _shape3(shape) -> Tuple[int, int, int]:
    """[D,H,W], or [H,W] as one slice."""
    if len(shape) not in (2, 3):
        raise ValueError(f"label volumes are [D,H,W] or [H,W], got {tuple(shape)}")
    return (1,) * (3 - len(shape)) + tuple(int(v) for v in shape)


def metrics_hist_bins(shape) -> int:
    """Bins of one class's histogram of squared distances: the largest squared distance inside the array, plus one."""
    D, H, W = _shape3(shape)
    return (D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2 + 1


def _spacing3(voxelspacing, ndim: int) -> Tuple[float, float, float]:
    """(sz, sy, sx) from medpy's `voxelspacing`: `ndim` floats in array axis order or one scalar for every axis, each finite and > 0
    (sz = 1 for [H,W]: unused)."""
    sp = np.asarray(voxelspacing, dtype=np.float64)
    if sp.ndim == 0:
        sp = np.full(ndim, float(sp))
    if sp.shape != (ndim,):
        raise ValueError(f"voxelspacing needs {ndim} components (one per array axis) or a scalar, got {voxelspacing!r}")
    if not (np.isfinite(sp).all() and (sp > 0).all()):
        raise ValueError(f"voxelspacing components must be finite and > 0, got {voxelspacing!r}")
    return (1.0,) * (3 - ndim) + tuple(float(v) for v in sp)


def metrics_scratch_bytes(shape, classes: int, voxelspacing=None) -> int:
    """What `metrics_device` allocates for one volume: two uint8 surface maps, two squared-distance maps (one class at a time: to the
    prediction's surface and to the ground truth's) and the int64 result [2][classes][3]; beside them, without spacing, int32 maps and
    the uint32 histograms [classes][bins]; with spacing, float64 maps and the radix select's work buffer."""
    D, H, W = _shape3(shape)
    n = D * H * W
    if voxelspacing is not None:
        return 2 * n + 2 * 8 * n + TC_METRIC_SELECT_WORK_BYTES + 8 * 2 * classes * 3
    return 2 * n + 2 * 4 * n + 4 * classes * metrics_hist_bins(shape) + 8 * 2 * classes * 3


def hd95_from_order_stats(n: int, d2_lo: int, d2_hi: int) -> float:
    """numpy.percentile(sqrt(d2), 95) of a pooled multiset of n squared distances from the two order statistics tc_metric_select returns:
    d2_lo at sorted position floor(0.95 (n-1)) and d2_hi at the next one (clamped), interpolated linearly in fp64."""
    pos = 0.95 * (n - 1)
    lo, hi = math.sqrt(d2_lo), math.sqrt(d2_hi)
    return lo + (hi - lo) * (pos - math.floor(pos))


def _label_pair(pred: torch.Tensor, label: torch.Tensor, classes: int):
    if not (pred.is_cuda and label.is_cuda):
        raise RuntimeError(NO_CPU)
    if pred.dtype != torch.uint8 or label.dtype != torch.uint8 or pred.shape != label.shape:
        raise ValueError("metrics on the device take two uint8 label volumes of one shape")
    if not 2 <= classes <= 16:
        raise ValueError("classes must be in 2..16")
    return pred.contiguous(), label.contiguous(), _shape3(pred.shape), int(pred.dim() == 3)


def surfaces_counts(pred: torch.Tensor, label: torch.Tensor, classes: int):
    """(surf_pred, surf_label, counts): per volume the uint8 map that holds label k on the surface voxels of class k and 0 elsewhere,
    and the int64 [classes,3] Dice counts (|P==k & G==k|, |P==k|, |G==k|), one launch (tc_metric_surfaces).  Nothing is synchronised."""
    pred, label, (D, H, W), zfaces = _label_pair(pred, label, classes)
    sp, sg = torch.empty_like(pred), torch.empty_like(label)
    counts = torch.zeros((classes, 3), dtype=torch.int64, device=pred.device)
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    lib().tc_metric_surfaces(pred.data_ptr(), label.data_ptr(), sp.data_ptr(), sg.data_ptr(), counts.data_ptr(), D, H, W, classes, zfaces, stream)
    return sp, sg, counts


def edt_squared(surf: torch.Tensor, k: int, out: Optional[torch.Tensor] = None, voxelspacing=None) -> torch.Tensor:
    """int32 map of the squared Euclidean distance to the nearest voxel with surf == k (TC_METRIC_NO_SOURCE everywhere if there is none).
    With `voxelspacing`: the float64 map of min (sz dz)^2 + (sy dy)^2 + (sx dx)^2 (tc_metric_edt_f64; +inf everywhere if there is none)."""
    if not surf.is_cuda:
        raise RuntimeError(NO_CPU)
    spaced = voxelspacing is not None
    spacing = _spacing3(voxelspacing, surf.dim()) if spaced else ()
    dtype = torch.float64 if spaced else torch.int32
    if out is None:
        out = torch.empty(surf.shape, dtype=dtype, device=surf.device)
    elif spaced and (out.dtype != dtype or out.shape != surf.shape or not out.is_contiguous()):
        raise ValueError("with voxelspacing `out` is a contiguous float64 map of surf's shape")
    entry = lib().tc_metric_edt_f64 if spaced else lib().tc_metric_edt
    entry(surf.contiguous().data_ptr(), k, out.data_ptr(), *_shape3(surf.shape), int(surf.dim() == 3), *spacing,
          torch.cuda.current_stream(surf.device).cuda_stream)
    return out


def metrics_order_stats(pred: torch.Tensor, label: torch.Tensor, classes: int, voxelspacing=None) -> torch.Tensor:
    """int64 [2,classes,3] on the device: [0] the Dice counts, [1] (n, d2_lo, d2_hi) per class (tc_metric_select).  Allocates
    `metrics_scratch_bytes(pred.shape, classes, voxelspacing)`; the two distance maps are reused class by class.  Nothing is synchronised.
    With `voxelspacing` d2_lo and d2_hi are doubles (tc_metric_select_f64): read them with `result[1, :, 1:].view(torch.float64)`."""
    return _class_loop(pred, label, classes, voxelspacing)[0]


def _split_stats(both: torch.Tensor, classes: int):
    """(res [2,classes,3], stats [classes,2,4]): the views of `_class_loop`'s flat int64 tensor, on the device or on the host."""
    return both[:6 * classes].view(2, classes, 3), both[6 * classes:].view(classes, 2, 4)


def _class_loop(pred: torch.Tensor, label: torch.Tensor, classes: int, voxelspacing=None, tol2: Optional[Tuple[float, ...]] = None):
    """The per-class loop of the device metrics: (res, stats, both).  `res` is `metrics_order_stats`' tensor.  With `tol2` (one squared
    tolerance per class 1..classes-1) every class's two distance maps, computed once, also feed tc_surface_stats / tc_surface_stats_f64,
    and `stats` is its int64 [classes,2,4] output (include/transception_surface.h; class 0 stays zero); `res` and `stats` are then the
    two views `_split_stats` takes of the flat int64 tensor `both`, so that one copy brings everything to the host.  Without `tol2`:
    `stats` and `both` are None and nothing else runs.  Nothing is synchronised."""
    spaced = voxelspacing is not None
    spacing = _spacing3(voxelspacing, pred.dim())[3 - pred.dim():] if spaced else None
    sp, sg, counts = surfaces_counts(pred, label, classes)
    D, H, W = _shape3(pred.shape)
    dev = pred.device
    L, stream = lib(), torch.cuda.current_stream(dev).cuda_stream
    stats = both = None
    if tol2 is not None:
        both = torch.zeros((6 + 8) * classes, dtype=torch.int64, device=dev)
        res, stats = _split_stats(both, classes)
        swork = torch.empty(TC_SURFACE_WORK_BYTES // 8, dtype=torch.int64, device=dev)
        surface_entry = L.tc_surface_stats_f64 if spaced else L.tc_surface_stats
    if spaced:
        work = torch.empty(TC_METRIC_SELECT_WORK_BYTES, dtype=torch.uint8, device=dev)
        if stats is None:
            res = torch.zeros((2, classes, 3), dtype=torch.int64, device=dev)         # class 0 is never selected: (0, 0.0, 0.0)
    else:
        nbins = metrics_hist_bins(pred.shape)
        hist = torch.zeros((classes, nbins), dtype=torch.int32, device=dev)           # uint32 to the library
        if stats is None:
            res = torch.empty((2, classes, 3), dtype=torch.int64, device=dev)         # tc_metric_select writes every class
    dp, dg = (torch.empty(pred.shape, dtype=torch.float64 if spaced else torch.int32, device=dev) for _ in range(2))
    res[0] = counts
    for k in range(1, classes):
        edt_squared(sp, k, dp, spacing)
        edt_squared(sg, k, dg, spacing)
        if spaced:
            L.tc_metric_select_f64(sp.data_ptr(), sg.data_ptr(), dp.data_ptr(), dg.data_ptr(), k, classes, D, H, W, work.data_ptr(),
                                   res[1].data_ptr(), stream)
        else:
            L.tc_metric_hist(sp.data_ptr(), sg.data_ptr(), dp.data_ptr(), dg.data_ptr(), k, hist.data_ptr(), nbins, classes, D, H, W, stream)
        if stats is not None:
            surface_entry(sp.data_ptr(), sg.data_ptr(), dp.data_ptr(), dg.data_ptr(), k, classes, D, H, W, tol2[k - 1], swork.data_ptr(),
                          stats.data_ptr(), stream)
    if not spaced:
        L.tc_metric_select(hist.data_ptr(), nbins, classes, res[1].data_ptr(), stream)
    return res, stats, both


def _order_stats_to_host(res: torch.Tensor, spaced: bool):
    """(counts, [(n, d2_lo, d2_hi)]) as Python numbers from `metrics_order_stats`' tensor: one copy."""
    res = res.cpu()
    counts, sel = res[0].tolist(), res[1].tolist()
    if spaced:
        sel = [(n, lo, hi) for (n, _, _), (lo, hi) in zip(sel, res[1, :, 1:].contiguous().view(torch.float64).tolist())]
    return counts, sel


def metrics_device(pred: torch.Tensor, label: torch.Tensor, classes: int = 9, voxelspacing=None) -> List[Tuple[float, float]]:
    """`calculate_metric_percase` (utils.py:50-60) for classes 1..classes-1 of two uint8 CUDA label volumes [D,H,W] ([H,W]: true 2-D, no z
    faces), connectivity 1: [(dice, hd95)].  Unit spacing: exact integer work on the device (csrc/metrics.hip), one copy of 6 * classes
    integers back; scratch: `metrics_scratch_bytes` (10 bytes a voxel plus the histograms).  `voxelspacing` (`pred.dim()` positive floats in
    array axis order, or a scalar): the fp64 kernels, 18 bytes a voxel.  The library takes D, H, W up to 2048 and fewer than 2^31 voxels;
    a larger volume raises `TcError`."""
    counts, sel = _order_stats_to_host(metrics_order_stats(pred, label, classes, voxelspacing), voxelspacing is not None)
    return [_percase(inter, p, g, lambda: hd95_from_order_stats(n, lo, hi)) for (inter, p, g), (n, lo, hi) in zip(counts[1:], sel[1:])]


def hd95_device(result: torch.Tensor, reference: torch.Tensor, voxelspacing=None) -> float:
    """`hd95(result, reference, voxelspacing)` (connectivity 1) for two boolean / uint8 CUDA masks, on the device."""
    if not (result.is_cuda and reference.is_cuda):
        raise RuntimeError(NO_CPU)
    counts, sel = _order_stats_to_host(metrics_order_stats((result != 0).to(torch.uint8), (reference != 0).to(torch.uint8), 2, voxelspacing),
                                       voxelspacing is not None)
    if counts[1][1] == 0 or counts[1][2] == 0:
        raise RuntimeError("surface distances need non-empty masks")
    return hd95_from_order_stats(*sel[1])


def _is_real(v) -> bool:
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


@dataclass(frozen=True)
class SurfaceMetrics:
    """The surface metrics of the evaluation beside Dice and HD95 (include/transception_surface.h has the definitions): ASD in both
    directions, ASSD, the full Hausdorff distance and the surface Dice (NSD) at `nsd_tolerance` -- one finite number >= 0 for every class, or
    a sequence with one per class 1..classes-1 (organ-specific tolerances), in the units of `voxelspacing` (voxels without it).  The
    tolerance is applied to squared distances: a surface voxel counts when d^2 <= tolerance * tolerance (the product formed once in fp64).
    The length of a sequence is checked where `classes` is known (`tolerances`)."""
    nsd_tolerance: Union[float, Tuple[float, ...]] = 1.0

    def __post_init__(self):
        t = self.nsd_tolerance
        if isinstance(t, (str, bytes, dict, set)) or (not _is_real(t) and not hasattr(t, "__iter__")):
            raise ValueError(f"nsd_tolerance must be a number >= 0 or a sequence of them, got {t!r}")
        values = (t,) if _is_real(t) else tuple(t)
        if not values or not all(_is_real(v) and math.isfinite(v) and v >= 0 for v in values):
            raise ValueError(f"nsd_tolerance must be finite numbers >= 0 (no bool, no NaN), got {t!r}")
        object.__setattr__(self, "nsd_tolerance", float(t) if _is_real(t) else tuple(float(v) for v in values))

    def tolerances(self, classes: int) -> Tuple[float, ...]:
        """One tolerance per class 1..classes-1."""
        t = self.nsd_tolerance
        if not isinstance(t, tuple):
            return (t,) * (classes - 1)
        if len(t) != classes - 1:
            raise ValueError(f"nsd_tolerance has {len(t)} values for the {classes - 1} classes 1..{classes - 1}")
        return t


def _surface_tolerances(surface, classes: int) -> Tuple[float, ...]:
    """The squared tolerances tau * tau per class 1..classes-1 of a `SurfaceMetrics`: a ValueError for anything else, before anything runs."""
    if not isinstance(surface, SurfaceMetrics):
        raise ValueError(f"surface must be a SurfaceMetrics, got {surface!r}")
    if isinstance(classes, bool) or not isinstance(classes, (int, np.integer)) or not 2 <= classes <= 16:
        raise ValueError("classes must be in 2..16")
    return tuple(t * t for t in surface.tolerances(int(classes)))


# what `surface_metrics_device` and `surface_metrics_host` return per class, beside `defined`
SURFACE_KEYS = ("dice", "jaccard", "precision", "recall", "hd95", "hd", "asd_pred", "asd_gt", "assd", "nsd")


def _percase_surface(inter: int, p: int, g: int, hd95_fn: Callable[[], float], records_fn: Callable[[], tuple]) -> Dict[str, object]:
    """The reference's rule (`_percase`, utils.py:50-60) extended to the surface metrics, for one class of one volume from |P&G|, |P|, |G|
    and, asked for only when both masks are non-empty, the two directed records (n, sum, within, max) of transception_surface.h.
    Both non-empty: the measured values, defined=True.  Only the prediction non-empty: the reference's own (1, 0) -- every overlap score and
    the surface Dice 1, every distance 0 --, defined=False.  Otherwise everything 0, defined=False."""
    dice, h95 = _percase(inter, p, g, hd95_fn)
    if p > 0 and g > 0:
        (n0, s0, w0, m0), (n1, s1, w1, m1) = records_fn()
        asd_pred, asd_gt = s0 / n0, s1 / n1
        values = (dice, inter / (p + g - inter), inter / p, inter / g, h95, math.sqrt(max(m0, m1)), asd_pred, asd_gt,
                  (asd_pred + asd_gt) / 2, (w0 + w1) / (n0 + n1))          # assd: medpy's mean of the directed means, not the pooled mean
    else:
        values = (dice,) * 4 + (0.0,) * 5 + (dice,)                        # dice is 1 or 0 here
    out = {key: float(v) for key, v in zip(SURFACE_KEYS, values)}
    out["defined"] = bool(p > 0 and g > 0)
    return out


def surface_metrics_device(pred: torch.Tensor, label: torch.Tensor, classes: int = 9, voxelspacing=None,
                           surface: SurfaceMetrics = SurfaceMetrics()) -> List[Dict[str, object]]:
    """One dict per class 1..classes-1 of two uint8 CUDA label volumes ([D,H,W], or [H,W]: true 2-D), keys SURFACE_KEYS and `defined`
    (`_percase_surface` has the rule).  `dice` and `hd95` are `metrics_device`'s, from the same launches and expressions; jaccard, precision
    and recall come from the same int64 counts; hd, asd_pred, asd_gt, assd and nsd from the directed statistics of tc_surface_stats /
    tc_surface_stats_f64 (csrc/surface.hip), one more pass per class over the surface and distance maps `metrics_device` has in memory.
    Scratch beside `metrics_scratch_bytes`: TC_SURFACE_WORK_BYTES and the [classes,2,4] result.  One copy of 14 * classes integers comes
    back, and nothing is synchronised before it."""
    tol2 = _surface_tolerances(surface, classes)
    spaced = voxelspacing is not None
    res, stats = _split_stats(_class_loop(pred, label, classes, voxelspacing, tol2)[2].cpu(), classes)
    counts, sel = _order_stats_to_host(res, spaced)
    rec = stats.tolist()
    sums = stats[:, :, 1].contiguous().view(torch.float64).tolist()
    maxs = stats[:, :, 3].contiguous().view(torch.float64).tolist() if spaced else None
    out = []
    for k in range(1, classes):
        (inter, p, g), (n, lo, hi) = counts[k], sel[k]
        records = tuple((rec[k][i][0], sums[k][i], rec[k][i][2], maxs[k][i] if spaced else rec[k][i][3]) for i in range(2))
        out.append(_percase_surface(inter, p, g, lambda: hd95_from_order_stats(n, lo, hi), lambda: records))
    return out


def surface_stats_host(pred: np.ndarray, gt: np.ndarray, voxelspacing=None, tol2: float = 1.0) -> tuple:
    """The two directed records ((n, sum, within, max) from the surface of `pred` to that of `gt`, then the reverse) of two non-empty
    boolean masks, as transception_surface.h defines them, from scipy.  The squared distances come from the feature transform: the index
    of the nearest surface voxel, then d2 = sum over the axes, in axis order, of (s_a (i_a - j_a))^2 -- exact integers (and an int `max`)
    with unit spacing, float64 with `voxelspacing`.  `sum` is math.fsum of the square roots; `within` counts d2 <= tol2."""
    from scipy.ndimage import binary_erosion, distance_transform_edt, generate_binary_structure
    pred, gt = np.atleast_1d(np.asarray(pred) > 0), np.atleast_1d(np.asarray(gt) > 0)
    if not pred.any() or not gt.any():
        raise RuntimeError("surface distances need non-empty masks")
    spacing = None if voxelspacing is None else _spacing3(voxelspacing, pred.ndim)[3 - pred.ndim:]
    footprint = generate_binary_structure(pred.ndim, 1)
    borders = [m ^ binary_erosion(m, structure=footprint, iterations=1) for m in (pred, gt)]
    records = []
    for src, dst in ((borders[0], borders[1]), (borders[1], borders[0])):
        nearest = distance_transform_edt(~dst, sampling=spacing, return_distances=False, return_indices=True)
        d2 = None
        for a, pos in enumerate(np.nonzero(src)):
            step = nearest[a][src].astype(np.int64) - pos
            term = step * step if spacing is None else (spacing[a] * step) ** 2
            d2 = term if d2 is None else d2 + term
        d2f = d2.astype(np.float64)
        records.append((int(d2.size), math.fsum(np.sqrt(d2f).tolist()), int(np.count_nonzero(d2f <= tol2)),
                        int(d2.max()) if spacing is None else float(d2.max())))
    return tuple(records)


def surface_metrics_host(pred: np.ndarray, label: np.ndarray, classes: int = 9, voxelspacing=None,
                         surface: SurfaceMetrics = SurfaceMetrics()) -> List[Dict[str, object]]:
    """`surface_metrics_device`'s structure from scipy, for the host metric path: `dice` and `hd95` are `calculate_metric_percase`'s, the
    rest comes from `surface_stats_host`.  With unit spacing the squared distances are exact integers and the tolerance test is the device's."""
    tol2 = _surface_tolerances(surface, classes)
    pred, label = np.asarray(pred), np.asarray(label)
    if pred.shape != label.shape or pred.ndim not in (2, 3):
        raise ValueError("surface metrics take two label volumes [D,H,W] or [H,W] of one shape")
    out = []
    for k in range(1, classes):
        P, G = pred == k, label == k
        out.append(_percase_surface(int(np.logical_and(P, G).sum()), int(P.sum()), int(G.sum()), lambda: hd95(P, G, voxelspacing),
                                    lambda: surface_stats_host(P, G, voxelspacing, tol2[k - 1])))       # the first two as calculate_metric_percase
    return out


POST_MODES = ("largest", "min_voxels")


@dataclass(frozen=True)
class PostProcess:
    """Connected-component post-processing of a predicted label volume, per class 1..classes-1 (include/transception_post.h):
    mode "largest" keeps the largest component of every class (a tie goes to the component that comes first in raster order),
    mode "min_voxels" every component of at least `min_voxels` voxels; the rest becomes background.  connectivity 1: face neighbours
    (scipy's generate_binary_structure(ndim, 1)), 3: the full neighbourhood (generate_binary_structure(ndim, ndim))."""
    mode: str = "largest"
    min_voxels: int = 0
    connectivity: int = 1

    def __post_init__(self):
        if self.mode not in POST_MODES:
            raise ValueError(f"mode must be one of {POST_MODES}, got {self.mode!r}")
        n = self.min_voxels
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
            raise ValueError(f"min_voxels must be an integer, got {n!r}")
        if self.mode == "min_voxels" and not 1 <= n < 2 ** 63:
            raise ValueError(f'mode "min_voxels" needs 1 <= min_voxels < 2^63, got {n!r}')
        if self.mode == "largest" and n != 0:
            raise ValueError(f'min_voxels belongs to mode "min_voxels" (leave it 0 with "largest"), got {n!r}')
        if self.connectivity not in (1, 3) or isinstance(self.connectivity, bool):
            raise ValueError(f"connectivity must be 1 (faces) or 3 (full neighbourhood), got {self.connectivity!r}")


def postprocess_scratch_bytes(shape) -> int:
    """What `postprocess_device` allocates beside its output: the int32 root and size maps, 8 bytes a voxel (the int64 [classes,2] record
    of the largest components is not counted).  0 for a shape outside the library's limits."""
    return int(lib().tc_cc_scratch_bytes(*_shape3(shape)))


def _label_volume(lab: torch.Tensor) -> Tuple[int, int, int]:
    if not lab.is_cuda:
        raise RuntimeError(NO_CPU)
    if lab.dtype != torch.uint8:
        raise ValueError("connected components on the device take a uint8 label volume")
    return _shape3(lab.shape)


def component_roots(lab: torch.Tensor, classes: int, connectivity: int = 1) -> torch.Tensor:
    """int32 map of lab's shape: for a foreground voxel (1 <= label < classes) the smallest linear index of its connected component, -1 for
    background (tc_cc_label).  Nothing is synchronised; limits and errors are the library's (`TcError`)."""
    shape = _label_volume(lab)
    root = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
    lib().tc_cc_label(lab.contiguous().data_ptr(), root.data_ptr(), *shape, classes, connectivity, torch.cuda.current_stream(lab.device).cuda_stream)
    return root


def component_sizes(lab: torch.Tensor, root: torch.Tensor, classes: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(size, best) from `component_roots`' map of the same volume: size is int32 of lab's shape, the voxel count of a component at its root
    and 0 elsewhere; best is int64 [classes,2], (voxels, root) of the largest component of every class -- a tie goes to the smaller root --
    and (0, -1) for a class without a voxel (tc_cc_sizes).  Nothing is synchronised."""
    shape = _label_volume(lab)
    if not root.is_cuda:
        raise RuntimeError(NO_CPU)
    if root.dtype != torch.int32 or root.shape != lab.shape or not root.is_contiguous():
        raise ValueError("root is the contiguous int32 map `component_roots` returned for this volume")
    size = torch.empty(lab.shape, dtype=torch.int32, device=lab.device)
    best = torch.empty((classes, 2), dtype=torch.int64, device=lab.device)
    lib().tc_cc_sizes(lab.contiguous().data_ptr(), root.data_ptr(), size.data_ptr(), best.data_ptr(), *shape, classes,
                      torch.cuda.current_stream(lab.device).cuda_stream)
    return size, best


def postprocess_device(pred: torch.Tensor, classes: int = 9, post: PostProcess = PostProcess(), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`post` applied to the uint8 CUDA label volume `pred` ([D,H,W], or [H,W]: true 2-D), on the device: a new tensor, or `out` (uint8, pred's
    shape; `out is pred` works in place).  Labels 0 and >= classes pass through unchanged.  Scratch: `postprocess_scratch_bytes`, 8 bytes
    a voxel.  Nothing is synchronised."""
    shape = _label_volume(pred)
    if out is not None and (not out.is_cuda or out.dtype != torch.uint8 or out.shape != pred.shape):
        raise ValueError("`out` is a uint8 CUDA tensor of pred's shape")
    lab = pred.contiguous()
    root = component_roots(lab, classes, post.connectivity)
    size, best = component_sizes(lab, root, classes)
    dst = out if out is not None and out.is_contiguous() else (lab if out is pred else torch.empty_like(lab))
    lib().tc_cc_keep(lab.data_ptr(), root.data_ptr(), size.data_ptr(), best.data_ptr(), dst.data_ptr(),
                     TC_CC_LARGEST if post.mode == "largest" else TC_CC_MIN_VOXELS, int(post.min_voxels), *shape, classes,
                     torch.cuda.current_stream(pred.device).cuda_stream)
    if out is None:
        return dst
    if dst is not out:
        out.copy_(dst)
    return out


def postprocess_host(pred: np.ndarray, classes: int = 9, post: PostProcess = PostProcess()) -> np.ndarray:
    """The same step on the host, with scipy.ndimage.label per class: a new array.  scipy numbers components in raster order of their first
    voxel, so numpy.argmax over their sizes picks, among equally large ones, the one with the smaller root: the device's tie rule."""
    from scipy.ndimage import generate_binary_structure, label
    pred = np.asarray(pred)
    if pred.dtype != np.uint8 or pred.ndim not in (2, 3):
        raise ValueError("post-processing takes a uint8 label volume [D,H,W] or [H,W]")
    if not 2 <= classes <= 16:
        raise ValueError("classes must be in 2..16")
    structure = generate_binary_structure(pred.ndim, 1 if post.connectivity == 1 else pred.ndim)
    out = pred.copy()
    for k in range(1, classes):
        comp, ncomp = label(pred == k, structure=structure)
        if ncomp == 0:
            continue
        sizes = np.bincount(comp.ravel(), minlength=ncomp + 1)
        if post.mode == "largest":
            keep = np.zeros(ncomp + 1, bool)
            keep[1 + int(np.argmax(sizes[1:]))] = True
        else:
            keep = sizes >= post.min_voxels
        keep[0] = True                                                   # not of class k: untouched
        out[~keep[comp]] = 0
    return out


@dataclass(frozen=True)
class TTA:
    """Test-time augmentation: the views of the input whose class probabilities are averaged (include/transception_tta.h).  A view is three
    bits -- 1: rows reversed, 2: columns reversed, 4: transpose, applied after the flips (square slices only) -- so 0..3 are the identity and
    the flips and 0..7 the eight symmetries of the square.  Views are evaluated, and their probabilities added, in the order given: another
    order may differ in the last bits of the sums."""
    views: Tuple[int, ...] = (0, 1, 2, 3)

    def __post_init__(self):
        v = self.views
        if not isinstance(v, tuple) or not v:
            raise ValueError(f"views must be a non-empty tuple of views 0..7, got {v!r}")
        if any(isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i <= 7 for i in v):
            raise ValueError(f"views must be integers in 0..7, got {v!r}")
        if len(set(int(i) for i in v)) != len(v):
            raise ValueError(f"views must be distinct, got {v!r}")

    @classmethod
    def flips(cls) -> "TTA":
        """Identity and the three flips: any slice shape."""
        return cls((0, 1, 2, 3))

    @classmethod
    def dihedral(cls) -> "TTA":
        """All eight symmetries of the square: square slices only."""
        return cls((0, 1, 2, 3, 4, 5, 6, 7))


RESAMPLE_MODES = ("labels", "scores")


# what an option of the evaluation may be: `_check_options` and `TrainConfig` apply these, each with its own message
VALID_OPTION = {"postprocess": lambda v: v is None or isinstance(v, PostProcess),
                "tta": lambda v: v is None or isinstance(v, TTA),
                "resample": lambda v: isinstance(v, str) and v in RESAMPLE_MODES,
                "surface": lambda v: v is None or isinstance(v, SurfaceMetrics),
                "calibration": lambda v: v is None or isinstance(v, Calibration)}


def _check_tta(tta, shape=None) -> None:
    """None or a TTA; with `shape` = (H, W) of the slices, a transposed view needs H == W."""
    if not VALID_OPTION["tta"](tta):
        raise ValueError(f"tta must be None or a TTA, got {tta!r}")
    if tta is not None and shape is not None and shape[0] != shape[1] and any(int(v) & TC_TTA_TRANSPOSE for v in tta.views):
        raise ValueError(f"a transposed view (>= 4) needs square slices, got {shape[0]} x {shape[1]}")


def _check_options(postprocess, tta, resample, host_zoom: bool = False, patch=None) -> None:
    """The options of `evaluate_volume` and `inference`, before anything runs; `patch`: (H, W) of the network's slices, where known."""
    if not VALID_OPTION["resample"](resample):
        raise ValueError(f"resample must be one of {RESAMPLE_MODES}, got {resample!r}")
    if resample == "scores" and host_zoom:
        raise ValueError('resample="scores" runs on the device; host_zoom=True is the reference\'s path (order-0 zoom of the labels on the host)')
    if not VALID_OPTION["postprocess"](postprocess):
        raise ValueError(f"postprocess must be None or a PostProcess, got {postprocess!r}")
    _check_tta(tta, patch)


def _check_out_size(out_size) -> Optional[Tuple[int, int]]:
    """None, or (X, Y): two integers in 1..TC_RESAMPLE_MAX_EXTENT."""
    if out_size is None:
        return None
    try:
        X, Y = out_size
        ok = all(not isinstance(v, bool) and isinstance(v, (int, np.integer)) and 1 <= v <= TC_RESAMPLE_MAX_EXTENT for v in (X, Y))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"out_size must be None or two integers in 1..{TC_RESAMPLE_MAX_EXTENT}, got {out_size!r}")
    return int(X), int(Y)


def resample_scores(src: torch.Tensor, size: Tuple[int, int], *, scores: bool = False, pred: bool = True,
                    pred_out: Optional[torch.Tensor] = None, scores_out: Optional[torch.Tensor] = None):
    """(scores, pred) of `src` [N,C,h,w] (fp32, bf16 or fp16 CUDA class scores) at `size` = (H, W): the bilinear, align_corners=False
    resampling of every class map as fp32 [N,C,H,W] (`scores`) and its first-maximum argmax as uint8 [N,H,W] (`pred`), one kernel
    (tc_resample_scores; include/transception_resample.h states the definition).  What is not asked for is None and is never written: with
    `pred` alone nothing of the size of the resampled scores exists.  `pred_out` / `scores_out`: contiguous tensors to write into.
    Nothing is synchronised."""
    if not src.is_cuda:
        raise RuntimeError(NO_CPU)
    if src.dim() != 4 or src.dtype not in TC_DTYPE:
        raise ValueError("class scores are a [N,C,h,w] tensor of float32, bfloat16 or float16")
    H, W = _check_out_size(size)
    scores, pred = scores or scores_out is not None, pred or pred_out is not None
    if not (scores or pred):
        raise ValueError("ask for the scores, the labels or both")
    src = src.contiguous()
    N, C, h, w = src.shape
    if scores and scores_out is None:
        scores_out = torch.empty((N, C, H, W), dtype=torch.float32, device=src.device)
    if pred and pred_out is None:
        pred_out = torch.empty((N, H, W), dtype=torch.uint8, device=src.device)
    for t, dt, shape in ((scores_out, torch.float32, (N, C, H, W)), (pred_out, torch.uint8, (N, H, W))):
        if t is not None and (not t.is_cuda or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError(f"an output of resample_scores is a contiguous CUDA {dt} tensor of shape {shape}")
    lib().tc_resample_scores(src.data_ptr(), TC_DTYPE[src.dtype], scores_out.data_ptr() if scores else None,
                             pred_out.data_ptr() if pred else None, N, C, h, w, H, W, torch.cuda.current_stream(src.device).cuda_stream)
    return (scores_out if scores else None), (pred_out if pred else None)


def _library_dtype(logits: torch.Tensor) -> torch.Tensor:
    """The logits as they are in a dtype the library takes, else as float32."""
    return logits if logits.dtype in TC_DTYPE else logits.float()


def _tta_view_logits(L, model, src: torch.Tensor, H: int, W: int, v: int, stream) -> torch.Tensor:
    """View `v` of the fp32 [n,H,W] batch `src`, normalised (tc_tta_view), through `model`: the logits, contiguous and in a dtype of the library."""
    n = src.shape[0]
    x = torch.empty((n, 1, W, H) if v & TC_TTA_TRANSPOSE else (n, 1, H, W), dtype=torch.float32, device=src.device)
    L.tc_tta_view(src.data_ptr(), x.data_ptr(), n, H, W, v, 0.5, 0.5, stream)
    lg = _library_dtype(model(x)).contiguous()
    if lg.shape != x.shape[:1] + lg.shape[1:2] + x.shape[2:]:
        raise ValueError(f"the model returned logits of shape {tuple(lg.shape)} for a view of shape {tuple(x.shape)}")
    return lg


@contextlib.contextmanager
def _eval_mode(model):
    """`model` in eval mode (BatchNorm by its running statistics, utils.py:78), and back to what it was."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def _view_entropy_add(L, lg: torch.Tensor, v: int, first: bool, ves: torch.Tensor, buf: torch.Tensor, stream) -> None:
    """The normalised entropy of one view's logits (tc_uncert_maps on the logits, in view coordinates, into the flat fp32 scratch `buf`),
    brought back to the un-transformed position -- the transpose undone, then the flips: plumbing on one [n,H,W] map -- and written (`first`)
    or added into `ves`."""
    n, C, Hv, Wv = lg.shape
    h = buf[:n * Hv * Wv].view(n, Hv, Wv)
    L.tc_uncert_maps(lg.data_ptr(), TC_DTYPE[lg.dtype], TC_UNCERT_LOGITS, 1.0, None, h.data_ptr(), None, None, None, n, C, Hv, Wv, stream)
    if v & TC_TTA_TRANSPOSE:
        h = h.transpose(-2, -1)
    dims = [d for d, bit in ((-2, TC_TTA_FLIP_H), (-1, TC_TTA_FLIP_W)) if v & bit]
    if dims:
        h = h.flip(dims)
    if first:
        ves.copy_(h)
    else:
        ves.add_(h)


def _predict(model, slices: torch.Tensor, batch: int, views: Optional[Tuple[int, ...]], out_size: Optional[Tuple[int, int]],
             labels: bool, ves: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The one batch loop of `predict_slices` (`labels`: uint8 [N,X,Y]) and `predict_probs` (else: the fp32 [N,C,X,Y] sums over the views), `model` in
    eval mode; (X, Y) is `out_size`, and None or (H, W) is the scores' own size.  How a batch's class scores are made: `views` None (labels
    only) -- the torch normalisation, and the scores are the logits; else per view, in the order given, tc_tta_view, `model`,
    tc_tta_accumulate.  Where they go: at their own size the labels come from tc_argmax_counts or from the last tc_tta_accumulate, and the
    sums are added in place in the returned tensor; at another size tc_resample_scores writes either.  One fp32 [batch,C,H,W] accumulator,
    allocated at the first logits, holds the views that do not go into the result: none for a single view that writes labels at its own size.
    `ves` (`predict_uncertainty` alone; fp32 [N,H,W], with `views`): every view's own normalised entropy is summed into it at the un-transformed
    position (`_view_entropy_add`: one more launch per view); None, as everywhere else: nothing more runs."""
    if not slices.is_cuda:
        raise RuntimeError(NO_CPU)
    N, H, W = slices.shape
    if out_size == (H, W):
        out_size = None
    in_place = out_size is None and not labels                   # the views are added into the returned sums themselves
    need_acc = views is not None and not in_place and (out_size is not None or len(views) > 1)
    L, stream, acc, hbuf = lib(), torch.cuda.current_stream(slices.device).cuda_stream, None, None
    out = torch.empty((N,) + (out_size or (H, W)), dtype=torch.uint8, device=slices.device) if labels else None
    with _eval_mode(model):
        for i in range(0, N, batch):
            src = slices[i:i + batch].float()
            n = src.shape[0]
            if views is None:
                scores = _library_dtype(model(((src - 0.5) / 0.5).unsqueeze(1)))
            else:
                src = src.contiguous()
                for j, v in enumerate(views):
                    lg = _tta_view_logits(L, model, src, H, W, v, stream)
                    C = lg.shape[1]
                    if need_acc and acc is None:
                        acc = torch.empty((batch, C, H, W), dtype=torch.float32, device=src.device)
                    if out is None:
                        out = torch.empty((N, C) + (out_size or (H, W)), dtype=torch.float32, device=src.device)
                    sums = out[i:i + n] if in_place else acc
                    last = labels and out_size is None and j == len(views) - 1
                    L.tc_tta_accumulate(lg.data_ptr(), TC_DTYPE[lg.dtype], sums.data_ptr() if sums is not None else None,
                                        out[i:i + n].data_ptr() if last else None, n, C, H, W, v, int(j == 0), stream)
                    if ves is not None:
                        if hbuf is None:                         # one view's entropy map: allocated once, as the accumulator is
                            hbuf = torch.empty(batch * H * W, dtype=torch.float32, device=src.device)
                        _view_entropy_add(L, lg, v, j == 0, ves[i:i + n], hbuf, stream)
                scores = acc[:n] if out_size is not None else None
            if out_size is not None:
                resample_scores(scores, out_size, pred=labels, pred_out=out[i:i + n] if labels else None, scores_out=None if labels else out[i:i + n])
            elif views is None:
                out[i:i + n] = argmax_counts(scores)[0]
            del scores                                           # a batch's logits do not live through the next batch's forward
    return out


@torch.no_grad()
def predict_slices(model, slices: torch.Tensor, batch: int = 16, tta: Optional[TTA] = None, *, out_size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """slices: float [N,H,W] in [0,1] at the network size (a multiple of 32); returns uint8 [N,H,W] labels.
    Normalisation (x-0.5)/0.5 as `transforms.Normalize([0.5],[0.5])` (utils.py:71-75); eval-mode BatchNorm (utils.py:78).
    `tta`: a `TTA`; the label is then the argmax of the class probabilities summed over its views (`views=(0,)` is softmax-then-argmax of
    the one plain pass: not bit-pinned to the path without `tta`, which takes the argmax of the logits).
    `out_size` = (X, Y) other than (H, W): uint8 [N,X,Y] labels, the argmax of the class scores resampled bilinearly to that size
    (tc_resample_scores) -- each batch's logits in their own dtype, or with `tta` the summed probabilities of all its views.  None or
    (H, W): the calls above, unchanged."""
    _check_tta(tta, tuple(slices.shape[1:]))
    return _predict(model, slices, batch, None if tta is None else tuple(map(int, tta.views)), _check_out_size(out_size), labels=True)


@torch.no_grad()
def predict_probs(model, slices: torch.Tensor, batch: int = 16, tta: Optional[TTA] = None, *, out_size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The class probabilities of `predict_slices`' input averaged over the views of `tta` (None: the single view 0): fp32 [N,C,H,W], the
    accumulator of tc_tta_accumulate divided by the number of views.  `out_size` = (X, Y) other than (H, W): fp32 [N,C,X,Y], the accumulator
    resampled bilinearly (the `scores` output of tc_resample_scores) and then divided."""
    _check_tta(tta, tuple(slices.shape[1:]))
    out_size = _check_out_size(out_size)
    if slices.shape[0] == 0:
        raise ValueError("predict_probs needs at least one slice")
    views = (0,) if tta is None else tuple(map(int, tta.views))
    out = _predict(model, slices, batch, views, out_size, labels=False)
    return out.div_(len(views)) if len(views) > 1 else out


@torch.no_grad()
def zoom_volume_to_network(vol: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """[D,X,Y] float32 slices on the GPU -> [D,size] : scipy.ndimage.zoom(slice, (size/X, size/Y), order=3) of utils.py:69-70 as the
    device spline prefilter + 4x4-tap evaluation of the input pipeline (csrc/data.hip; within 1e-6 of scipy, tests/test_data_gpu.py)."""
    L = lib()
    D, X, Y = vol.shape
    stream = torch.cuda.current_stream(vol.device).cuda_stream
    vol = vol.contiguous()
    coef = torch.empty((D, X, Y), dtype=torch.float64, device=vol.device)
    out = torch.empty((D, 1, size[0], size[1]), dtype=torch.float32, device=vol.device)
    L.tc_spline_prefilter(vol.data_ptr(), coef.data_ptr(), D, X, Y, stream)
    L.tc_zoom_normalize(coef.data_ptr(), vol.data_ptr(), None, out.data_ptr(), None, D, X, Y, size[0], size[1], 0.0, 1.0, stream)
    return out[:, 0]


@torch.no_grad()
def zoom_labels(pred: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """uint8 [D,h,w] label maps -> [D,size]: scipy.ndimage.zoom(pred, ..., order=0) of utils.py:83-84 (nearest sample at
    o (in-1)/(out-1); bit-exact integer work) through the label path of the same device kernel."""
    L = lib()
    D, h, w = pred.shape
    dev = pred.device
    stream = torch.cuda.current_stream(dev).cuda_stream
    pred = pred.contiguous()
    coef = torch.zeros(D * h * w, dtype=torch.float64, device=dev)            # the image half of the kernel is unused
    x = torch.empty((D, 1, size[0], size[1]), dtype=torch.float32, device=dev)
    y = torch.empty((D, size[0], size[1]), dtype=torch.int64, device=dev)
    L.tc_zoom_normalize(coef.data_ptr(), None, pred.data_ptr(), x.data_ptr(), y.data_ptr(), D, h, w, size[0], size[1], 0.0, 1.0, stream)
    return y.to(torch.uint8)


def _predict_volume_host(model, image: np.ndarray, dev, classes, patch_size, batch, postprocess, tta) -> np.ndarray:
    """Prediction at `image`'s resolution, as the reference makes it: scipy's zooms per slice, `postprocess` on the host.  uint8 NumPy [D,X,Y]."""
    from scipy.ndimage import zoom
    D, X, Y = image.shape
    resize = (X, Y) != tuple(patch_size)
    sl = np.stack([zoom(image[d], (patch_size[0] / X, patch_size[1] / Y), order=3) if resize else image[d] for d in range(D)])
    pred = predict_slices(model, torch.from_numpy(sl.astype(np.float32)).to(dev), batch, tta).cpu().numpy()
    if resize:
        pred = np.stack([zoom(pred[d], (X / patch_size[0], Y / patch_size[1]), order=0) for d in range(D)])
    return pred if postprocess is None else postprocess_host(pred, classes, postprocess)


def _predict_volume_device(model, image: np.ndarray, dev, classes, patch_size, batch, postprocess, tta, resample) -> torch.Tensor:
    """The same on the device: one upload, both zooms (resample="scores": the resampled class scores), `postprocess`.  uint8 CUDA tensor [D,X,Y]."""
    D, X, Y = image.shape
    resize = (X, Y) != tuple(patch_size)
    vol = torch.from_numpy(np.ascontiguousarray(image, np.float32)).to(dev)
    sl = zoom_volume_to_network(vol, tuple(patch_size)) if resize else vol
    if resize and resample == "scores":
        pred = predict_slices(model, sl, batch, tta, out_size=(X, Y))
    else:
        pred = predict_slices(model, sl, batch, tta)
        pred = zoom_labels(pred, (X, Y)) if resize else pred
    return pred if postprocess is None else postprocess_device(pred, classes, postprocess, out=pred)


def _dice_counts_host(pred: np.ndarray, label: np.ndarray, classes: int) -> np.ndarray:
    """float64 [classes,3]: (|P==k & G==k|, |P==k|, |G==k|), what `surfaces_counts` counts on the device."""
    return np.array([(np.logical_and(pred == k, label == k).sum(), (pred == k).sum(), (label == k).sum()) for k in range(classes)], dtype=np.float64)


def _score_host(pred: np.ndarray, label: np.ndarray, classes: int, with_hd95: bool, voxelspacing):
    if with_hd95:
        return [calculate_metric_percase(pred == k, label == k, voxelspacing) for k in range(1, classes)]
    return dice_from_counts(_dice_counts_host(pred, label, classes))


def _score_device(pred: torch.Tensor, label: np.ndarray, classes: int, with_hd95: bool, voxelspacing):
    label_t = torch.from_numpy(np.ascontiguousarray(label).astype(np.uint8)).to(pred.device)
    if with_hd95:
        return metrics_device(pred, label_t, classes, voxelspacing)
    return dice_from_counts(surfaces_counts(pred, label_t, classes)[2].cpu().numpy())


@torch.no_grad()
def evaluate_volume(model, image: np.ndarray, label: np.ndarray, classes: int = 9, patch_size=(224, 224),
                    batch: int = 16, with_hd95: bool = False, host_zoom: bool = False, device_metrics: bool = False, voxelspacing=None,
                    postprocess: Optional[PostProcess] = None, tta: Optional[TTA] = None, *, resample: str = "labels"):
    """`test_single_volume` for one [D,H,W] volume (utils.py:63-98): per-class Dice for classes 1..classes-1, or with
    `with_hd95` the reference's metric_list of (dice, hd95) pairs.  The volume goes to the GPU once; the order-3 zoom to the network
    size, inference, argmax and the order-0 zoom back all run there (host_zoom=True: scipy per slice, as the reference does).
    `device_metrics=True`: the prediction stays on the GPU, the label volume is uploaded once and `metrics_device` (with_hd95) or the
    counts of its first kernel (Dice only) replace the host metric; same returned structure.  `voxelspacing`: the (z, y, x) size of a voxel
    of `label`, for the HD95 of either metric path (Dice does not depend on it).  `postprocess`: a `PostProcess` applied in 3-D to the
    prediction at `label`'s resolution (after the order-0 zoom back) before either metric path: on the device wherever the prediction is
    there (host_zoom=False, whatever `device_metrics` is), else on the host; None: no such step.  `tta`: a `TTA` handed to `predict_slices`
    (both zoom paths; the views are taken at the network size, before the zoom back and `postprocess`); None: one plain pass.
    `resample`: what goes from the network size to `label`'s.  "labels": the argmax, by the reference's order-0 zoom (utils.py:83-84).
    "scores": the class scores (with `tta` the summed probabilities), bilinearly, and then the argmax -- the reference's commented-out
    `F.interpolate(outputs, ..., mode='bilinear')` (utils.py:81) -- fused in tc_resample_scores, so that only the uint8 labels exist at
    `label`'s size; `postprocess` and both metric paths follow as before.  Without a resize both values run the same calls; "scores" with
    `host_zoom=True` is a ValueError."""
    _check_options(postprocess, tta, resample, host_zoom, tuple(patch_size))
    pred = _predict_volume(model, image, classes, patch_size, batch, host_zoom, device_metrics, postprocess, tta, resample)
    return (_score_device if device_metrics else _score_host)(pred, label, classes, with_hd95, voxelspacing)


def _predict_volume(model, image: np.ndarray, classes, patch_size, batch, host_zoom, device_metrics, postprocess, tta, resample):
    """The prediction of `evaluate_volume` and `evaluate_volume_report` at `image`'s resolution, where the metric path wants it: a uint8 CUDA
    tensor with `device_metrics`, else a NumPy array."""
    dev = next(model.parameters()).device
    if device_metrics and dev.type != "cuda":
        raise RuntimeError(NO_CPU)
    if host_zoom:
        on_host = _predict_volume_host(model, image, dev, classes, patch_size, batch, postprocess, tta)
        return torch.from_numpy(on_host).to(dev) if device_metrics else on_host
    on_device = _predict_volume_device(model, image, dev, classes, patch_size, batch, postprocess, tta, resample)
    return on_device if device_metrics else on_device.cpu().numpy()


@torch.no_grad()
def evaluate_volume_report(model, image: np.ndarray, label: np.ndarray, classes: int = 9, patch_size=(224, 224), batch: int = 16,
                           host_zoom: bool = False, device_metrics: bool = False, voxelspacing=None, postprocess: Optional[PostProcess] = None,
                           tta: Optional[TTA] = None, *, resample: str = "labels", surface: SurfaceMetrics = SurfaceMetrics()):
    """`evaluate_volume`'s prediction of one [D,H,W] volume, scored with the surface metrics as well: one dict per class 1..classes-1 with the
    keys SURFACE_KEYS and `defined`, from `surface_metrics_device` (`device_metrics=True`: the prediction stays on the GPU) or
    `surface_metrics_host`.  `dice` and `hd95` are what `evaluate_volume(..., with_hd95=True)` returns; every other argument is its own."""
    _check_options(postprocess, tta, resample, host_zoom, tuple(patch_size))
    _surface_tolerances(surface, classes)
    pred = _predict_volume(model, image, classes, patch_size, batch, host_zoom, device_metrics, postprocess, tta, resample)
    if not device_metrics:
        return surface_metrics_host(pred, label, classes, voxelspacing, surface)
    label_t = torch.from_numpy(np.ascontiguousarray(label).astype(np.uint8)).to(pred.device)
    return surface_metrics_device(pred, label_t, classes, voxelspacing, surface)


def inference(model, volumes, classes: int = 9, img_size: int = 224, batch: int = 16, log=None,
              device_metrics: bool = False, voxelspacing=None, postprocess: Optional[PostProcess] = None,
              tta: Optional[TTA] = None, *, resample: str = "labels") -> Tuple[float, float]:
    """trainer.py:25-47: mean Dice and mean HD95 over `volumes` = iterable of (image [D,H,W] in [0,1], label [D,H,W], case name).
    `device_metrics`, `voxelspacing` (one spacing for every volume), `postprocess`, `tta`, `resample`: as in `evaluate_volume`."""
    _check_options(postprocess, tta, resample)
    total, n = 0.0, 0
    for i, (image, label, name) in enumerate(volumes):
        m = np.array(evaluate_volume(model, np.asarray(image), np.asarray(label), classes, (img_size, img_size), batch, with_hd95=True,
                                     device_metrics=device_metrics, voxelspacing=voxelspacing, postprocess=postprocess, tta=tta, resample=resample))
        total = total + m
        n += 1
        if log:
            log(' idx %d case %s mean_dice %f mean_hd95 %f' % (i, name, m.mean(axis=0)[0], m.mean(axis=0)[1]))
    if n == 0:
        raise ValueError("inference() needs at least one volume")
    total = total / n
    if log:
        for k in range(1, classes):
            log('Mean class %d mean_dice %f mean_hd95 %f' % (k, total[k - 1][0], total[k - 1][1]))
    performance, mean_hd95 = float(total.mean(axis=0)[0]), float(total.mean(axis=0)[1])
    if log:
        log('Testing performance in best val model: mean_dice : %f mean_hd95 : %f' % (performance, mean_hd95))
    return performance, mean_hd95



def inference_report(model, volumes, classes: int = 9, img_size: int = 224, batch: int = 16, log=None,
                     device_metrics: bool = False, voxelspacing=None, postprocess: Optional[PostProcess] = None,
                     tta: Optional[TTA] = None, *, resample: str = "labels", surface: SurfaceMetrics = SurfaceMetrics()) -> dict:
    """`inference` with the surface metrics: `evaluate_volume_report` per volume, and
        {"cases": [{"name", "classes": [dict per class]}], "mean": {key: [per class]}, "overall": {key: float}, "n_defined": [per class]}
    over the keys SURFACE_KEYS.  The means are taken over ALL cases with the values of the per-case rule (`_percase_surface`), as
    `inference` takes them, in its arithmetic: (overall["dice"], overall["hd95"]) is the pair `inference` returns.  `n_defined` counts, per
    class, the cases in which both masks were non-empty -- the cases whose distances were measured."""
    _check_options(postprocess, tta, resample)
    _surface_tolerances(surface, classes)
    cases, total = [], 0.0
    for i, (image, label, name) in enumerate(volumes):
        per_class = evaluate_volume_report(model, np.asarray(image), np.asarray(label), classes, (img_size, img_size), batch,
                                           device_metrics=device_metrics, voxelspacing=voxelspacing, postprocess=postprocess, tta=tta,
                                           resample=resample, surface=surface)
        m = np.array([[c[key] for key in SURFACE_KEYS] for c in per_class])
        total = total + m
        cases.append({"name": name, "classes": per_class})
        if log:
            case = dict(zip(SURFACE_KEYS, m.mean(axis=0)))
            log(' idx %d case %s mean_dice %f mean_hd95 %f' % (i, name, case["dice"], case["hd95"]))
            log(' idx %d case %s mean_assd %f mean_hd %f mean_nsd %f' % (i, name, case["assd"], case["hd"], case["nsd"]))
    if not cases:
        raise ValueError("inference_report() needs at least one volume")
    total = total / len(cases)
    overall = {key: float(v) for key, v in zip(SURFACE_KEYS, total.mean(axis=0))}
    if log:
        for k in range(1, classes):
            row = dict(zip(SURFACE_KEYS, total[k - 1]))
            log('Mean class %d mean_dice %f mean_hd95 %f' % (k, row["dice"], row["hd95"]))
            log('Mean class %d mean_assd %f mean_hd %f mean_nsd %f' % (k, row["assd"], row["hd"], row["nsd"]))
        log('Testing performance in best val model: mean_dice : %f mean_hd95 : %f' % (overall["dice"], overall["hd95"]))
        log('Testing performance in best val model: mean_assd : %f mean_hd : %f mean_nsd : %f' % (overall["assd"], overall["hd"], overall["nsd"]))
    return {"cases": cases, "mean": {key: total[:, j].tolist() for j, key in enumerate(SURFACE_KEYS)}, "overall": overall,
            "n_defined": [sum(bool(c["classes"][k]["defined"]) for c in cases) for k in range(classes - 1)]}


# ------------------------------------------------------------------------------------------------ uncertainty maps and calibration
UNCERT_KINDS = {"logits": TC_UNCERT_LOGITS, "prob_sums": TC_UNCERT_PROB_SUMS}


class Uncertainty(NamedTuple):
    """Per-pixel maps of `uncertainty_maps` and `predict_uncertainty` (include/transception_uncertainty.h): the uint8 label, the predictive
    entropy normalised to [0, 1] by log(classes), the maximum class probability, and the mutual information between the views (the entropy of
    the averaged probabilities minus the average of the views' entropies, >= 0).  What was not asked for, or does not exist, is None."""
    pred: Optional[torch.Tensor]
    entropy: Optional[torch.Tensor]
    confidence: Optional[torch.Tensor]
    mutual_information: Optional[torch.Tensor]


@dataclass(frozen=True)
class Calibration:
    """Calibration statistics of the evaluation (include/transception_uncertainty.h): `bins` equal-width confidence bins (1..32) of the
    reliability table behind ECE and MCE; `foreground_only`: count a pixel only where its label or its prediction is not background (class 0
    dominates a CT slice, and its confident pixels hide everything else); `ignore_index`: a label value 0..255 whose pixels are not counted
    (labels >= classes never are)."""
    bins: int = 15
    foreground_only: bool = False
    ignore_index: Optional[int] = None

    def __post_init__(self):
        b, i = self.bins, self.ignore_index
        if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 1 <= b <= TC_CALIB_MAX_BINS:
            raise ValueError(f"bins must be an integer in 1..{TC_CALIB_MAX_BINS}, got {b!r}")
        if not isinstance(self.foreground_only, (bool, np.bool_)):
            raise ValueError(f"foreground_only must be a bool, got {self.foreground_only!r}")
        if i is not None and (isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i <= 255):
            raise ValueError(f"ignore_index must be None or an integer in 0..255 (labels are uint8), got {i!r}")
        object.__setattr__(self, "bins", int(b))
        object.__setattr__(self, "foreground_only", bool(self.foreground_only))
        object.__setattr__(self, "ignore_index", None if i is None else int(i))


def _check_calibration(calibration, classes) -> None:
    if not isinstance(calibration, Calibration):
        raise ValueError(f"calibration must be a Calibration, got {calibration!r}")
    if isinstance(classes, bool) or not isinstance(classes, (int, np.integer)) or not 1 <= classes <= 16:
        raise ValueError("classes must be in 1..16")


def _check_views(views) -> float:
    """The fp32 factor (float)(1.0 / V) of V views."""
    if isinstance(views, bool) or not isinstance(views, (int, np.integer)) or views < 1:
        raise ValueError(f"views must be an integer >= 1, got {views!r}")
    return float(np.float32(1.0 / int(views)))


def _check_scores(scores: torch.Tensor, kind: str) -> torch.Tensor:
    if kind not in UNCERT_KINDS:
        raise ValueError(f"kind must be one of {tuple(UNCERT_KINDS)}, got {kind!r}")
    if not scores.is_cuda:
        raise RuntimeError(NO_CPU)
    if scores.dim() != 4 or scores.dtype not in TC_DTYPE or (kind == "prob_sums" and scores.dtype != torch.float32):
        raise ValueError("class scores are a [N,C,H,W] tensor: float32, bfloat16 or float16 logits, or float32 probability sums")
    return scores.contiguous()


def uncertainty_maps(scores: torch.Tensor, *, kind: str = "logits", views: int = 1, entropy: bool = True, confidence: bool = True,
                     pred: bool = False, view_entropy_sum: Optional[torch.Tensor] = None) -> Uncertainty:
    """The maps of tc_uncert_maps for CUDA class scores [N,C,H,W], one launch: `kind` "logits" (fp32, bf16 or fp16; softmax in registers) or
    "prob_sums" (fp32 sums of `views` probability vectors, the accumulator of tc_tta_accumulate).  `view_entropy_sum`: fp32 [N,H,W], the sum of
    the views' own normalised entropies; the mutual information `max(0, entropy - view_entropy_sum / views)` is returned with it.  What is
    not asked for is None and is never written.  Nothing is synchronised."""
    inv = _check_views(views)
    scores = _check_scores(scores, kind)
    N, C, H, W = scores.shape
    dev = scores.device
    if not (entropy or confidence or pred or view_entropy_sum is not None):
        raise ValueError("ask for at least one map")
    ves = view_entropy_sum
    if ves is not None:
        if not ves.is_cuda or ves.dtype != torch.float32 or tuple(ves.shape) != (N, H, W):
            raise ValueError(f"view_entropy_sum is a float32 CUDA tensor of shape {(N, H, W)}")
        ves = ves.contiguous()
    new = lambda dt: torch.empty((N, H, W), dtype=dt, device=dev)
    e, c = (new(torch.float32) if entropy else None), (new(torch.float32) if confidence else None)
    m, p = (new(torch.float32) if ves is not None else None), (new(torch.uint8) if pred else None)
    ptr = lambda t: None if t is None else t.data_ptr()
    lib().tc_uncert_maps(scores.data_ptr(), TC_DTYPE[scores.dtype], UNCERT_KINDS[kind], inv, ptr(ves), ptr(e), ptr(c), ptr(m), ptr(p), N, C, H, W,
                         torch.cuda.current_stream(dev).cuda_stream)
    return Uncertainty(p, e, c, m)


@torch.no_grad()
def predict_uncertainty(model, slices: torch.Tensor, batch: int = 16, tta: Optional[TTA] = None, *,
                        out_size: Optional[Tuple[int, int]] = None) -> Uncertainty:
    """`predict_probs`' batch loop and views (`_predict`), and from its accumulator the four maps of `Uncertainty`, each [N,X,Y] with
    (X, Y) = `out_size` or the slices' own size.  Per view one tc_uncert_maps on the view's logits adds that view's entropy, at the
    un-transformed position, into a view-entropy sum; after the last view one tc_uncert_maps per batch on the summed probabilities writes all
    maps.  With `out_size` the accumulator is resampled bilinearly first (tc_resample_scores), and the view-entropy sum with it, as a
    one-class map.  `mutual_information` is None with fewer than two views.  `pred` is the argmax of the summed probabilities."""
    _check_tta(tta, tuple(slices.shape[1:]))
    out_size = _check_out_size(out_size)
    if slices.shape[0] == 0:
        raise ValueError("predict_uncertainty needs at least one slice")
    views = (0,) if tta is None else tuple(map(int, tta.views))
    N, H, W = slices.shape
    ves = torch.empty((N, H, W), dtype=torch.float32, device=slices.device) if len(views) > 1 else None
    sums = _predict(model, slices, batch, views, out_size, labels=False, ves=ves)
    if ves is not None and tuple(sums.shape[2:]) != (H, W):
        ves = torch.cat([resample_scores(ves[i:i + batch].unsqueeze(1), tuple(sums.shape[2:]), scores=True, pred=False)[0][:, 0]
                         for i in range(0, N, batch)])
    parts = [uncertainty_maps(sums[i:i + batch], kind="prob_sums", views=len(views), pred=True,
                              view_entropy_sum=None if ves is None else ves[i:i + batch]) for i in range(0, N, batch)]
    return Uncertainty(*(None if part[0] is None else torch.cat(part) for part in zip(*parts)))


def calibration_stats(scores: torch.Tensor, labels: torch.Tensor, calibration: Calibration = Calibration(), *, kind: str = "logits",
                      views: int = 1, work: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw int64 slots of tc_calib_stats, on the device, for CUDA class scores [N,C,H,W] (`kind`, `views`: as `uncertainty_maps`) and
    uint8 labels [N,H,W]: [bins][3] (count, confidence sum in units of 2^-32, correct), [4] (n, NLL sum and Brier sum as the bits of doubles,
    correct), [C][3] per predicted class (count, entropy sum in units of 2^-32, correct).  Two launches, nothing synchronised.
    `decode_calibration_stats` turns them into a float64 vector that is additive over batches, volumes and ranks.  `work`: the scratch of an
    earlier call with the same bins and classes (`calibration_work`), so that a loop over batches allocates it once."""
    scores = _check_scores(scores, kind)
    inv = _check_views(views)
    N, C, H, W = scores.shape
    _check_calibration(calibration, C)
    if not labels.is_cuda:
        raise RuntimeError(NO_CPU)
    if labels.dtype != torch.uint8 or tuple(labels.shape) != (N, H, W):
        raise ValueError(f"labels are a uint8 CUDA tensor of shape {(N, H, W)}")
    labels = labels.contiguous()
    L, dev = lib(), scores.device
    if work is None:
        work = calibration_work(calibration.bins, C, dev)
    elif not work.is_cuda or work.dtype != torch.int64 or work.numel() * 8 < int(L.tc_calib_work_bytes(calibration.bins, C)) or not work.is_contiguous():
        raise ValueError("work is the int64 CUDA scratch of calibration_work(bins, classes, device)")
    out = torch.empty(int(L.tc_calib_out_slots(calibration.bins, C)), dtype=torch.int64, device=dev)
    L.tc_calib_stats(scores.data_ptr(), TC_DTYPE[scores.dtype], UNCERT_KINDS[kind], inv, labels.data_ptr(),
                     -1 if calibration.ignore_index is None else calibration.ignore_index, TC_CALIB_FOREGROUND if calibration.foreground_only else 0,
                     calibration.bins, N, C, H, W, work.data_ptr(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return out


def calibration_work(bins: int, classes: int, device) -> torch.Tensor:
    """The scratch of tc_calib_stats for `bins` and `classes` (tc_calib_work_bytes; 304 KiB at 15 and 9): it needs no initialisation."""
    return torch.empty(int(lib().tc_calib_work_bytes(bins, classes)) // 8, dtype=torch.int64, device=device)


def decode_calibration_stats(stats, bins: int):
    """The int64 slots of `calibration_stats` (a tensor, on the device or not, or a NumPy array) as a float64 vector of the same kind and layout:
    the counts as they are (exact below 2^53), the two fixed-point sums divided by 2^32, the NLL and Brier sums read as the doubles they
    are.  Decoded vectors add: over batches, volumes and ranks."""
    if isinstance(stats, torch.Tensor):
        if stats.dtype != torch.int64 or stats.dim() != 1:
            raise ValueError("raw calibration statistics are a flat int64 tensor")
        out = stats.to(torch.float64)
        out[3 * bins + 1:3 * bins + 3] = stats[3 * bins + 1:3 * bins + 3].view(torch.float64)
    else:
        stats = np.ascontiguousarray(stats)
        if stats.dtype != np.int64 or stats.ndim != 1:
            raise ValueError("raw calibration statistics are a flat int64 array")
        out = stats.astype(np.float64)
        out[3 * bins + 1:3 * bins + 3] = stats[3 * bins + 1:3 * bins + 3].view(np.float64)
    out[1:3 * bins:3] /= 2.0 ** 32
    out[3 * bins + 5::3] /= 2.0 ** 32
    return out


def calibration_from_stats(stats, bins: int, classes: int) -> dict:
    """ECE and its companions from the slots of `calibration_stats` -- raw int64, or decoded and summed float64 (`decode_calibration_stats`):
        {"ece": sum_b n_b / n |acc_b - conf_b|, "mce": max_b |acc_b - conf_b| over the non-empty bins, "nll", "brier": means over the n
         counted pixels, "accuracy", "n", "bins": [{"count", "confidence", "accuracy"}], "classes": [{"count", "entropy", "accuracy"}]}
    with the means of an empty bin or class, and everything at n = 0, equal to 0."""
    if isinstance(stats, torch.Tensor):
        stats = stats.detach().cpu().numpy()
    stats = np.asarray(stats)
    if stats.dtype == np.int64:
        stats = decode_calibration_stats(stats, bins)
    if stats.dtype != np.float64 or stats.shape != (3 * bins + 4 + 3 * classes,):
        raise ValueError(f"calibration statistics for {bins} bins and {classes} classes are {3 * bins + 4 + 3 * classes} int64 or float64 slots")
    table, (n, nll, brier, correct), per_class = stats[:3 * bins].reshape(bins, 3), stats[3 * bins:3 * bins + 4], stats[3 * bins + 4:].reshape(classes, 3)
    mean = lambda total, count: float(total / count) if count > 0 else 0.0
    rows = [{"count": int(c), "confidence": mean(s, c), "accuracy": mean(k, c)} for c, s, k in table]
    gaps = [(r["count"], abs(r["accuracy"] - r["confidence"])) for r in rows if r["count"] > 0]
    return {"ece": float(sum(c * g for c, g in gaps) / n) if n > 0 else 0.0, "mce": max((g for _, g in gaps), default=0.0),
            "nll": mean(nll, n), "brier": mean(brier, n), "accuracy": mean(correct, n), "n": int(n), "bins": rows,
            "classes": [{"count": int(c), "entropy": mean(s, c), "accuracy": mean(k, c)} for c, s, k in per_class]}


def calibration_stats_host(probs: np.ndarray, labels: np.ndarray, calibration: Calibration = Calibration()) -> np.ndarray:
    """The decoded float64 slots of `calibration_stats` from NumPy, by the definitions of include/transception_uncertainty.h for probabilities
    p [N,C,H,W] (the values as given, widened to float64) and labels [N,H,W]: the bin by the header's float32 product, the confidence sum
    by its truncation to 2^-32 (exact for float32 probabilities), entropy, NLL and Brier in float64."""
    probs, labels = np.asarray(probs), np.asarray(labels)
    if probs.ndim != 4 or labels.shape != probs.shape[:1] + probs.shape[2:]:
        raise ValueError("calibration on the host takes probabilities [N,C,H,W] and labels [N,H,W]")
    C, bins = probs.shape[1], calibration.bins
    _check_calibration(calibration, C)
    p = np.moveaxis(probs, 1, -1).reshape(-1, C)
    y = labels.reshape(-1).astype(np.int64)
    pred = p.argmax(axis=1)                                                # the first maximum
    counted = y < C
    if calibration.ignore_index is not None:
        counted &= y != calibration.ignore_index
    if calibration.foreground_only:
        counted &= (y > 0) | (pred > 0)
    p, y, pred = p[counted], y[counted], pred[counted]
    conf32 = p.max(axis=1).astype(np.float32) if len(p) else np.zeros(0, np.float32)
    b = np.minimum(bins - 1, (conf32 * np.float32(bins)).astype(np.int64))
    p = p.astype(np.float64)
    conf = np.floor(conf32.astype(np.float64) * 2.0 ** 32) / 2.0 ** 32
    with np.errstate(divide="ignore", invalid="ignore"):
        h = -np.where(p > 0, p * np.log(p), 0.0).sum(axis=1) / math.log(C) if C > 1 else np.zeros(len(p))
    h = np.clip(h, 0.0, 1.0)
    rows = np.arange(len(p))
    nll = -np.log(np.maximum(p[rows, y], float(np.finfo(np.float32).tiny)))
    onehot = np.zeros_like(p)
    onehot[rows, y] = 1.0
    brier = ((p - onehot) ** 2).sum(axis=1)
    ok = (pred == y).astype(np.float64)
    out = np.zeros(3 * bins + 4 + 3 * C, dtype=np.float64)
    for j, w in enumerate((None, conf, ok)):
        out[j:3 * bins:3] = np.bincount(b, weights=w, minlength=bins)
    out[3 * bins:3 * bins + 4] = (len(p), math.fsum(nll.tolist()), math.fsum(brier.tolist()), ok.sum())
    for j, w in enumerate((None, h, ok)):
        out[3 * bins + 4 + j::3] = np.bincount(pred, weights=w, minlength=C)
    return out


def calibration_host(probs: np.ndarray, labels: np.ndarray, calibration: Calibration = Calibration()) -> dict:
    """`calibration_from_stats`' dict from NumPy in float64 (`calibration_stats_host`), plus "stats": the counterpart of the `*_host` functions."""
    stats = calibration_stats_host(probs, labels, calibration)
    return dict(calibration_from_stats(stats, calibration.bins, np.asarray(probs).shape[1]), stats=stats)


@torch.no_grad()
def evaluate_volume_calibration(model, image: np.ndarray, label: np.ndarray, classes: int = 9, patch_size=(224, 224), batch: int = 16,
                                tta: Optional[TTA] = None, *, calibration: Calibration = Calibration()) -> dict:
    """Calibration of one [D,X,Y] volume, measured where the scores live: at the network size.  The image goes there by the order-3 zoom of
    `evaluate_volume`, the label volume by `zoom_labels`, the order-0 rule the training labels go through; the class probabilities summed
    over the views of `tta` (None: the one plain pass) are `predict_probs`' accumulator, and tc_calib_stats reads it batch by batch.  Nothing
    of the label's size times the classes is made.  Returns `calibration_from_stats`' dict plus "stats": the decoded float64 slots (NumPy),
    which add over volumes."""
    _check_calibration(calibration, classes)
    _check_tta(tta, tuple(patch_size))
    image, label = np.asarray(image), np.asarray(label)
    if image.ndim != 3 or image.shape != label.shape:
        raise ValueError("calibration takes an image volume [D,X,Y] and a label volume of the same shape")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError(NO_CPU)
    D, X, Y = image.shape
    resize = (X, Y) != tuple(patch_size)
    vol = torch.from_numpy(np.ascontiguousarray(image, np.float32)).to(dev)
    lab = torch.from_numpy(np.ascontiguousarray(label).astype(np.uint8)).to(dev)
    if resize:
        vol, lab = zoom_volume_to_network(vol, tuple(patch_size)), zoom_labels(lab, tuple(patch_size))
    views = (0,) if tta is None else tuple(map(int, tta.views))
    sums = _predict(model, vol, batch, views, None, labels=False)
    if sums.shape[1] != classes:
        raise ValueError(f"the model returned {sums.shape[1]} classes, not {classes}")
    total, work = None, calibration_work(calibration.bins, classes, dev)
    for i in range(0, D, batch):
        part = decode_calibration_stats(calibration_stats(sums[i:i + batch], lab[i:i + batch], calibration, kind="prob_sums", views=len(views),
                                                          work=work), calibration.bins)
        total = part if total is None else total.add_(part)
    stats = total.cpu().numpy()
    return dict(calibration_from_stats(stats, calibration.bins, classes), stats=stats)


def calibration_line(c: dict) -> str:
    """The figures of a `calibration_from_stats` dict as the log lines carry them."""
    return 'ece %f mce %f nll %f brier %f accuracy %f n %d' % (c["ece"], c["mce"], c["nll"], c["brier"], c["accuracy"], c["n"])


def inference_calibration(model, volumes, classes: int = 9, img_size: int = 224, batch: int = 16, log=None, tta: Optional[TTA] = None, *,
                          calibration: Calibration = Calibration()) -> dict:
    """`evaluate_volume_calibration` over `volumes` = iterable of (image, label, case name), and the calibration of the POOL: the slots of all
    volumes are added and decoded once -- ECE is defined over a test set, it is not the mean of the cases' ECEs.
        {"cases": [{"name", ...the case's dict}], "overall": {...the pool's dict, with its "stats"}}"""
    _check_calibration(calibration, classes)
    _check_tta(tta)
    cases, total = [], None
    for i, (image, label, name) in enumerate(volumes):
        c = evaluate_volume_calibration(model, np.asarray(image), np.asarray(label), classes, (img_size, img_size), batch, tta, calibration=calibration)
        total = c["stats"].copy() if total is None else total + c["stats"]
        cases.append(dict(c, name=name))
        if log:
            log(' idx %d case %s calibration %s' % (i, name, calibration_line(c)))
    if not cases:
        raise ValueError("inference_calibration() needs at least one volume")
    overall = dict(calibration_from_stats(total, calibration.bins, classes), stats=total)
    if log:
        log('Calibration over %d cases: %s' % (len(cases), calibration_line(overall)))
    return {"cases": cases, "overall": overall}

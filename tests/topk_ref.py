"""The definition of include/transception_topk.h in float64 torch with autograd; no project code.

  v_i    = w_ce[y_i] q_i^gamma (-log max(p_t, 1e-38))          per counted pixel (y_i != ignore_index), q_i = sum_{k != y_i} p_ik
  n      = number of counted pixels,  k = max(1, min(n, ceil(frac n)))  (the product once, in float64)
  t      = the k-th largest v_i,  n_gt = #{v_i > t},  n_eq = #{v_i == t},  S = sum_{v_i > t} v_i,  f = (k - n_gt) / n_eq
  TopkCE = (S + (k - n_gt) t) / k  =  sum_i s_i v_i / k       s_i = 1 above t, f at t, 0 below: constants, the selection is not differentiated
  CE     = mean over the ranks of TopkCE_r, each rank selecting among its own pixels;  n = 0: TopkCE = 0
  loss   = w_ce CE + w_dice Overlap, the overlap term (Dice or Tversky, weighted, ignoring) over ALL ranks' pixels

`reference` takes the batch of one rank; `reference_ranks` a list of them.
"""
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

EPS = 1e-5


def topk_k(frac: float, n: int) -> int:
    """k = max(1, min(n, ceil(frac n))); 0 when nothing is counted."""
    return max(1, min(n, math.ceil(float(frac) * float(n)))) if n > 0 else 0


class Select(NamedTuple):
    n: int
    k: int
    n_gt: int
    n_eq: int
    t: float
    S: float
    f: float
    ce: float                   # (S + (k - n_gt) t) / k
    gap: float                  # (k-th - (k+1)-th largest) / k-th, relative; inf when k = n


def select(v: torch.Tensor, frac: float) -> Select:
    """The selection over a 1-D float64 tensor of the counted pixels' values."""
    n = v.numel()
    k = topk_k(frac, n)
    if n == 0:
        return Select(0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, math.inf)
    srt = torch.sort(v.detach(), descending=True).values
    t = float(srt[k - 1])
    n_gt, n_eq = int((srt > t).sum()), int((srt == t).sum())
    S = math.fsum(srt[:n_gt].tolist())
    gap = (t - float(srt[k])) / t if k < n and t > 0 else math.inf
    return Select(n, k, n_gt, n_eq, t, S, (k - n_gt) / n_eq, (S + (k - n_gt) * t) / k, gap)


class Ref(NamedTuple):
    loss: float
    ce: float
    overlap: float
    grad: list                  # per rank: d loss / d logits, [B, C, HW]
    grad_ce: list               # its w_ce * CE part
    grad_overlap: list          # its w_dice * Overlap part
    sel: list                   # per rank: Select
    values: list                # per rank: [B, HW] float64, v_i at counted pixels and -1 at ignored ones


def _pixel_terms(x, labels, w_ce, ii, gamma):
    ncls = x.shape[1]
    valid = torch.ones_like(labels, dtype=torch.bool) if ii is None else labels != ii
    lab0 = torch.where(valid, labels, torch.zeros_like(labels))
    oh = F.one_hot(lab0, ncls).permute(0, 2, 1).double() * valid[:, None]
    p = torch.softmax(x, 1) * valid[:, None]
    wc = torch.ones(ncls, dtype=torch.float64) if w_ce is None else w_ce.double()
    pt = (p * oh).sum(1)
    q = (p * (1.0 - oh)).sum(1)
    q = torch.where(valid, q, torch.ones_like(q))
    nll = -torch.log(torch.clamp(torch.where(valid, pt, torch.ones_like(pt)), min=1e-38))
    mod = torch.ones_like(q) if gamma == 0 else q ** gamma
    v = wc[lab0] * mod * nll                                  # [B, HW]; 0 * ... at ignored pixels, masked below
    return v, valid, p, oh


def pixel_values(logits, labels, w_ce=None, ii=None, gamma: float = 0.0) -> torch.Tensor:
    """The value map [B, HW] in float64: v_i at counted pixels, -1 at ignored ones."""
    v, valid, _, _ = _pixel_terms(logits.detach().double().cpu(), labels.cpu(), w_ce, ii, gamma)
    return torch.where(valid, v, torch.full_like(v, -1.0))


def reference_ranks(logits, labels, frac: float, w_ce: Optional[torch.Tensor] = None, w_dice: Optional[torch.Tensor] = None,
                    ii: Optional[int] = None, gamma: float = 0.0, overlap: str = "dice", alpha: float = 0.5, beta: float = 0.5,
                    w=(0.4, 0.6)) -> Ref:
    """logits: a list (one entry per rank) of [B, C, HW] tensors of any float type, widened; labels: a list of [B, HW] int64."""
    xs = [l.detach().double().cpu().clone().requires_grad_() for l in logits]
    ncls = xs[0].shape[1]
    wd = torch.ones(ncls, dtype=torch.float64) if w_dice is None else w_dice.double()
    ce, sels, values = 0.0, [], []
    inter = ys = third = 0.0
    for x, lab in zip(xs, labels):
        v, valid, p, oh = _pixel_terms(x, lab.cpu(), w_ce, ii, gamma)
        vc = v[valid]
        sel = select(vc, frac)
        sels.append(sel)
        values.append(torch.where(valid, v.detach(), torch.full_like(v, -1.0)))
        if sel.n:
            s = torch.where(vc.detach() > sel.t, 1.0, 0.0) + torch.where(vc.detach() == sel.t, sel.f, 0.0)
            ce = ce + (s * vc).sum() / sel.k
        else:
            ce = ce + x.sum() * 0.0
        inter, ys = inter + (p * oh).sum((0, 2)), ys + oh.sum((0, 2))
        third = third + ((p * p) if overlap == "dice" else p).sum((0, 2))
    ce = ce / len(xs)
    if overlap == "dice":
        per_class = 1.0 - (2.0 * inter + EPS) / (third + ys + EPS)
    else:
        assert overlap == "tversky"
        per_class = 1.0 - (inter + EPS) / ((1.0 - alpha - beta) * inter + alpha * third + beta * ys + EPS)
    ov = (wd * per_class).sum() / ncls
    g_ce = torch.autograd.grad(w[0] * ce, xs, retain_graph=True)
    g_ov = torch.autograd.grad(w[1] * ov, xs)
    loss = w[0] * ce + w[1] * ov
    assert bool(torch.isfinite(loss)), "the reference itself is not finite"
    return Ref(loss.item(), ce.item(), ov.item(), [a + b for a, b in zip(g_ce, g_ov)], list(g_ce), list(g_ov), sels, values)


def reference(logits, labels, frac: float, w_ce=None, w_dice=None, ii=None, gamma: float = 0.0, overlap: str = "dice", alpha: float = 0.5,
              beta: float = 0.5, w=(0.4, 0.6)) -> Ref:
    """One rank: the lists of reference_ranks hold one entry each."""
    return reference_ranks([logits], [labels], frac, w_ce, w_dice, ii, gamma, overlap, alpha, beta, w)

"""The definition of include/transception_loss.h in float64 torch with autograd: softmax, the focal cross-entropy, the Dice or Tversky
overlap term, then `backward` -- once per term, so that the two parts of the gradient are known before they cancel.  `closed_form` is the
gradient as the header writes it (what the backward kernel evaluates), index for index; tests/test_focal_tversky_host.py holds it to autograd.

  q_i     = sum_{k != y_i} p_ik
  FocalCE = sum_i w_ce[y_i] q_i^gamma (-log max(p_t, 1e-38)) / sum_i w_ce[y_i]       over the counted pixels; 0 when the denominator is 0
  Dice    = sum_k w_dice[k] (1 - (2 I_k + eps) / (Z_k + Y_k + eps)) / ncls
  Tversky = sum_k w_dice[k] (1 - (I_k + eps) / ((1 - a - b) I_k + a P_k + b Y_k + eps)) / ncls
  loss    = w_ce FocalCE + w_dice Overlap
"""
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

EPS = 1e-5


class Ref(NamedTuple):
    loss: float
    ce: float
    overlap: float
    grad: torch.Tensor          # d loss / d logits, [B, C, HW]
    grad_ce: torch.Tensor       # its w_ce * FocalCE part
    grad_overlap: torch.Tensor  # its w_dice * Overlap part
    sums: torch.Tensor          # [1 + 3 C] float64: what the forward kernel accumulates (third per-class sum: Z under Dice, P under Tversky)


def _terms(x, labels, w_ce, w_dice, ii, gamma, overlap, alpha, beta):
    ncls = x.shape[1]
    valid = torch.ones_like(labels, dtype=torch.bool) if ii is None else labels != ii
    lab0 = torch.where(valid, labels, torch.zeros_like(labels))
    oh = F.one_hot(lab0, ncls).permute(0, 2, 1).double() * valid[:, None]
    p = torch.softmax(x, 1) * valid[:, None]
    wc = torch.ones(ncls, dtype=torch.float64) if w_ce is None else w_ce.double()
    wd = torch.ones(ncls, dtype=torch.float64) if w_dice is None else w_dice.double()
    pt = (p * oh).sum(1)
    q = (p * (1.0 - oh)).sum(1)
    q = torch.where(valid, q, torch.ones_like(q))             # (an ignored pixel has weight 0: keep 0^gamma out of its graph)
    nll = -torch.log(torch.clamp(torch.where(valid, pt, torch.ones_like(pt)), min=1e-38))
    mod = torch.ones_like(q) if gamma == 0 else q ** gamma
    wy = wc[lab0] * valid
    num, den = (wy * mod * nll).sum(), wy.sum()
    ce = num / den if float(den) > 0.0 else x.sum() * 0.0
    inter, ys = (p * oh).sum((0, 2)), oh.sum((0, 2))
    if overlap == "dice":
        third = (p * p).sum((0, 2))
        per_class = 1.0 - (2.0 * inter + EPS) / (third + ys + EPS)
    else:
        assert overlap == "tversky"
        third = p.sum((0, 2))
        per_class = 1.0 - (inter + EPS) / ((1.0 - alpha - beta) * inter + alpha * third + beta * ys + EPS)
    ov = (wd * per_class).sum() / ncls
    sums = torch.cat([num.reshape(1), torch.stack([inter, ys, third], 1).reshape(-1)]).detach()
    return ce, ov, sums


def reference(logits, labels, w_ce: Optional[torch.Tensor] = None, w_dice: Optional[torch.Tensor] = None, ii: Optional[int] = None,
              gamma: float = 0.0, overlap: str = "dice", alpha: float = 0.5, beta: float = 0.5, w=(0.4, 0.6)) -> Ref:
    """logits [B, C, HW] (any float type, widened), labels [B, HW] int64; w_ce / w_dice [C] or None; ii or None."""
    x = logits.detach().double().cpu().clone().requires_grad_()
    ce, ov, sums = _terms(x, labels.cpu(), w_ce, w_dice, ii, gamma, overlap, alpha, beta)
    g_ce, = torch.autograd.grad(w[0] * ce, x, retain_graph=True)
    g_ov, = torch.autograd.grad(w[1] * ov, x)
    loss = w[0] * ce + w[1] * ov
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g_ce).all()) and bool(torch.isfinite(g_ov).all()), "the reference itself is not finite"
    return Ref(loss.item(), ce.item(), ov.item(), g_ce + g_ov, g_ce, g_ov, sums)


def closed_form(logits, labels, w_ce=None, w_dice=None, ii=None, gamma=0.0, overlap="dice", alpha=0.5, beta=0.5, w=(0.4, 0.6), gscale=1.0):
    """dlogits [B, C, HW] by the formulas of the header, in float64: m_i, ca_k / cb_k from the global sums, one pass per pixel."""
    x = logits.detach().double().cpu()
    labels = labels.cpu()
    B, ncls, HW = x.shape
    with torch.no_grad():
        sums = _terms(x, labels, w_ce, w_dice, ii, gamma, overlap, alpha, beta)[2]
    inter, ys, third = sums[1::3], sums[2::3], sums[3::3]
    wc = torch.ones(ncls, dtype=torch.float64) if w_ce is None else w_ce.double()
    wd = torch.ones(ncls, dtype=torch.float64) if w_dice is None else w_dice.double()
    if overlap == "dice":
        den = third + ys + EPS
        ca = -(w[1] / ncls) * wd * 2.0 / den
        cb = (w[1] / ncls) * wd * 2.0 * (2.0 * inter + EPS) / den ** 2
    else:
        r = 1.0 - alpha - beta
        D = r * inter + alpha * third + beta * ys + EPS
        ca = -(w[1] / ncls) * wd * (D - (inter + EPS) * r) / D ** 2
        cb = (w[1] / ncls) * wd * (inter + EPS) * alpha / D ** 2
    n_eff = float((wc * ys).sum())
    cew = w[0] / n_eff if n_eff > 0.0 else 0.0
    p = torch.softmax(x, 1)
    out = torch.zeros_like(x)
    for b in range(B):
        for i in range(HW):
            t = int(labels[b, i])
            if ii is not None and t == ii:
                continue
            pi = p[b, :, i]
            delta = torch.zeros(ncls, dtype=torch.float64)
            delta[t] = 1.0
            q = float(pi.sum() - pi[t]) if ncls == 1 else float(torch.cat([pi[:t], pi[t + 1:]]).sum())
            pt = float(pi[t])
            if gamma == 0:
                m = 1.0
            elif q == 0.0:
                m = 0.0
            else:
                m = q ** (gamma - 1.0) * (q - gamma * pt * float(torch.log(pi[t])))
            g = ca * delta + (cb * pi if overlap == "dice" else cb)
            out[b, :, i] = gscale * (cew * float(wc[t]) * m * (pi - delta) + pi * (g - float((g * pi).sum())))
    return out

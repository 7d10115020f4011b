"""Host reference of the test-time augmentation (include/transception_tta.h), in float64 torch, written from the definition:

  a view v in 0..7 is three bits: 1 = rows reversed, 2 = columns reversed, 4 = transpose, applied after the flips;
  the probabilities of a view's logits are the softmax over the class axis; they are taken back to the un-transformed position and summed.

Nothing here imports the package."""
import torch

FLIP_H, FLIP_W, TRANSPOSE = 1, 2, 4


def _flip_dims(v):
    if not 0 <= v <= 7:
        raise ValueError(f"view {v!r} is outside 0..7")
    return [d for bit, d in ((FLIP_H, -2), (FLIP_W, -1)) if v & bit]


def view(a: torch.Tensor, v: int) -> torch.Tensor:
    """view_v of the last two axes of `a`: the flips chosen by bits 0 and 1, then the transpose under bit 2."""
    dims = _flip_dims(v)
    a = a.flip(dims) if dims else a
    return a.transpose(-2, -1) if v & TRANSPOSE else a


def unview(b: torch.Tensor, v: int) -> torch.Tensor:
    """The inverse: the transpose first, then the flips (each its own inverse; they act on different axes, so their order is free)."""
    dims = _flip_dims(v)
    b = b.transpose(-2, -1) if v & TRANSPOSE else b
    return b.flip(dims) if dims else b


def where_in_view(v: int, H: int, W: int, p: int, q: int):
    """The index form: (y, x) of the view at which original position (p, q) of an [H, W] map is found."""
    fp = H - 1 - p if v & FLIP_H else p
    fq = W - 1 - q if v & FLIP_W else q
    return (fq, fp) if v & TRANSPOSE else (fp, fq)


def view_probs(logits: torch.Tensor, v: int) -> torch.Tensor:
    """float64 softmax over axis 1 of the logits [N,C,h,w] of view v, at the original positions: [N,C,H,W]."""
    return unview(torch.softmax(logits.detach().cpu().double(), dim=1), v).contiguous()


def sum_probs(views, logits) -> torch.Tensor:
    """Sum over the views (in any order: float64) of `view_probs`; logits[i] belongs to views[i].  The mean is this over len(views)."""
    assert len(views) == len(logits) and len(views) > 0
    total = view_probs(logits[0], views[0])
    for v, lg in zip(views[1:], logits[1:]):
        total = total + view_probs(lg, v)
    return total

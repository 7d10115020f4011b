"""A float64 model of include/transception_uncertainty.h (torch / NumPy), a NumPy float32 emulation of its bin rule and of its entropy,
and the seeded inputs the host and the GPU tests share.  Nothing here imports the package."""
import math

import numpy as np
import torch

SHAPES = [(1, 1, 1, 1), (2, 9, 3, 5), (1, 2, 3, 130), (3, 16, 33, 33), (2, 9, 33, 47), (4, 9, 96, 96)]
PER_VIEW = 2e-6                # the project's bound on one fp32 softmax probability against float64 (tests/tta_ref.py)
ENTROPY_CAP = 2e-5             # the entropy bound is four times the worst deviation measured on the MI355X, never above this
# Measured on the MI355X: the worst |h - float64 model| over the shapes of tests/test_uncertainty_gpu.py -- logits in fp32, bf16 and fp16 at
# scales 1-3 (worst 1.84e-7, 4 x 9 x 96 x 96 fp16) and sums of three views' probabilities (worst 2.522e-7, 3 x 16 x 33 x 33) -- is 2.522e-7.
# The bound is four times that, 1.009e-6, far below the cap: a wrong formula or a missing normalisation misses by 1e-2 or more.
ENTROPY_WORST = 2.522e-7
ENTROPY_BOUND = min(4 * ENTROPY_WORST, ENTROPY_CAP)
FLT_MIN = float(np.finfo(np.float32).tiny)
TORCH_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def sums_bound(n: int, C: int) -> float:
    """The issue's bound on a sum of n NLL or Brier terms: n (entropy bound x log C + 2e-6 C)."""
    return n * (ENTROPY_BOUND * math.log(C) + PER_VIEW * C)


# ------------------------------------------------------------------------------------------------------------------ seeded inputs
def seeded_logits(shape, dtype: torch.dtype, seed: int, scale: float) -> torch.Tensor:
    """Normals x scale, STORED in `dtype`: the model reads the stored values."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale).to(dtype)


def seeded_labels(shape, seed: int, extra=()) -> torch.Tensor:
    """uint8 [N,H,W] labels in 0..C-1, with about 5 % of each value of `extra` (an ignore value, labels >= C)."""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed + 1000)
    y = torch.randint(0, C, (N, H, W), generator=g)
    for j, v in enumerate(extra):
        y[torch.rand((N, H, W), generator=g) < 0.05] = v
    return y.to(torch.uint8)


def seeded_prob_sums(shape, views: int, seed: int, scale: float = 2.0) -> torch.Tensor:
    """fp32 [N,C,H,W]: the sum of `views` float64 softmaxes of seeded normals, rounded to fp32 once."""
    g = torch.Generator().manual_seed(seed)
    t = sum(torch.softmax(torch.randn(shape, generator=g, dtype=torch.float64) * scale, dim=1) for _ in range(views))
    return t.to(torch.float32)


def dyadic_prob_sums(shape, seed: int):
    """fp32 [N,C,H,W] sums of FOUR views' probabilities that are multiples of 1/64 (so p = t / 4 is a multiple of 1/256 and every sum the
    kernel forms from it is exact), with 16 bins in mind.  Where the map has room, pixels are planted whose confidence sits exactly on every
    bin edge b / 16 and in the middle of every bin, bin 0 included: those are not normalised (a maximum below 1/16 cannot belong to 16
    probabilities that sum to 1), which the definition does not ask for.  Returns (t, planted): planted = the number of planted pixels."""
    N, C, H, W = shape
    g = np.random.default_rng(seed)
    counts = g.multinomial(256, g.dirichlet(np.full(C, 0.6), size=N * H * W))              # [pixels, C], rows sum to 256
    t = counts.astype(np.float64) / 64.0
    planted = 0
    if N * H * W >= 64:
        for b in range(16):
            for units in (16 * b + 8, 16 * b):                                             # the middle of bin b, and its lower edge
                if units == 0:
                    continue
                t[planted] = 0.0
                t[planted, b % C] = units / 64.0
                planted += 1
    t = t.reshape(N, H, W, C).transpose(0, 3, 1, 2)
    return torch.from_numpy(np.ascontiguousarray(t)).to(torch.float32), planted


# ------------------------------------------------------------------------------------------------------------------ the float64 model
def model(scores: torch.Tensor, kind: str, views: int = 1, labels: torch.Tensor = None) -> dict:
    """float64 [N,H,W] maps of the header's per-pixel quantities from the stored scores: p (float64 [N,C,H,W]), conf, pred, h, gap (between
    the two largest probabilities; 1 for one class) and, with labels, nll and brier (0 where the label is >= C)."""
    x = scores.detach().cpu().to(torch.float64)
    C = x.shape[1]
    p = torch.softmax(x, dim=1) if kind == "logits" else x / views
    conf, pred = p.max(dim=1)
    pred = p.argmax(dim=1)
    if kind == "logits":
        logp = torch.log_softmax(x, dim=1)
        H = -(p * logp).sum(dim=1)
    else:
        H = -torch.where(p > 0, p * torch.log(p.clamp(min=1e-300)), torch.zeros_like(p)).sum(dim=1)
    h = (H / math.log(C)).clamp(0.0, 1.0) if C > 1 else torch.zeros_like(H)
    top = torch.topk(p, min(2, C), dim=1).values
    out = {"p": p, "conf": conf, "pred": pred, "h": h, "gap": top[:, 0] - top[:, 1] if C > 1 else torch.ones_like(conf)}
    if labels is not None:
        y = labels.cpu().long()
        yc = y.clamp(max=C - 1).unsqueeze(1)
        py = p.gather(1, yc)[:, 0]
        out["nll"] = -logp.gather(1, yc)[:, 0] if kind == "logits" else -torch.log(py.clamp(min=FLT_MIN))
        onehot = torch.zeros_like(p).scatter_(1, yc, 1.0)
        out["brier"] = ((p - onehot) ** 2).sum(dim=1)
    return out


def counted(labels: torch.Tensor, pred: torch.Tensor, C: int, ignore_index=None, foreground=False) -> torch.Tensor:
    y = labels.cpu().long()
    keep = y < C
    if ignore_index is not None and 0 <= ignore_index <= 255:
        keep &= y != ignore_index
    if foreground:
        keep &= (y > 0) | (pred.cpu() > 0)
    return keep


def stats_model(m: dict, labels: torch.Tensor, bins: int, C: int, ignore_index=None, foreground=False, conf=None, pred=None) -> np.ndarray:
    """The decoded float64 slots from the maps of `model` (the bin from float64 conf x bins -- or from `conf`, `pred`: float64 / int64 maps given instead)."""
    conf = m["conf"] if conf is None else conf
    pred = m["pred"] if pred is None else pred
    keep = counted(labels, pred, C, ignore_index, foreground)
    y = labels.cpu().long()[keep].numpy()
    c, k = conf[keep].numpy(), pred[keep].numpy()
    b = np.minimum(bins - 1, np.floor(c * bins).astype(np.int64))
    ok = (k == y).astype(np.float64)
    out = np.zeros(3 * bins + 4 + 3 * C)
    for j, w in enumerate((None, c, ok)):
        out[j:3 * bins:3] = np.bincount(b, weights=w, minlength=bins)
    out[3 * bins:3 * bins + 4] = (len(y), m["nll"][keep].sum().item(), m["brier"][keep].sum().item(), ok.sum())
    for j, w in enumerate((None, m["h"][keep].numpy(), ok)):
        out[3 * bins + 4 + j::3] = np.bincount(k, weights=w, minlength=C)
    return out


# ------------------------------------------------------------------------------------------------------------------ float32 emulations
def emulate_prob_sums(t: torch.Tensor, views: int, labels: torch.Tensor, bins: int, ignore_index=None, foreground=False) -> dict:
    """The rule of TC_UNCERT_PROB_SUMS in NumPy float32: p = t * (float)(1.0 / V), one multiply; conf, the first maximum; the bin
    min(bins - 1, (int)(conf * (float)bins)); the confidence sum by truncation to 2^-32; brier in float32 in class order, summed in float64.
    Returns the int64 bin table [bins,3], n, n correct, the per-class (count, correct) [C,2], the Brier sum and the maps conf / pred."""
    x = t.cpu().numpy().astype(np.float32)
    C = x.shape[1]
    p = x * np.float32(1.0 / views)
    assert p.dtype == np.float32
    conf, pred = p.max(axis=1), p.argmax(axis=1)
    keep = counted(labels, torch.from_numpy(pred), C, ignore_index, foreground).numpy()
    y = labels.cpu().numpy().astype(np.int64)
    prod = conf * np.float32(bins)
    assert prod.dtype == np.float32
    b = np.minimum(bins - 1, prod.astype(np.int64))
    fixed = np.floor(conf.astype(np.float64) * 2.0 ** 32).astype(np.int64)                  # conf * 2^32 is exact in fp32: a power of two
    brier = np.zeros(conf.shape, np.float32)
    for k in range(C):
        d = p[:, k] - (y == k).astype(np.float32)
        brier = brier + d * d
    ok = pred == y
    table = np.zeros((bins, 3), np.int64)
    np.add.at(table[:, 0], b[keep], 1)
    np.add.at(table[:, 1], b[keep], fixed[keep])
    np.add.at(table[:, 2], b[keep], ok[keep].astype(np.int64))
    per_class = np.zeros((C, 2), np.int64)
    np.add.at(per_class[:, 0], pred[keep], 1)
    np.add.at(per_class[:, 1], pred[keep], ok[keep].astype(np.int64))
    return {"table": table, "n": int(keep.sum()), "correct": int(ok[keep].sum()), "per_class": per_class,
            "brier": float(brier[keep].astype(np.float64).sum()), "conf": conf, "pred": pred}


def emulate_entropy_logits(scores: torch.Tensor) -> np.ndarray:
    """h of TC_UNCERT_LOGITS in NumPy float32, operation by operation (NumPy's float32 exp / log, not the device's)."""
    l = scores.detach().cpu().to(torch.float32).numpy()
    C = l.shape[1]
    if C == 1:
        return np.zeros((l.shape[0],) + l.shape[2:], np.float32)
    m = l.max(axis=1)
    s = np.zeros_like(m)
    a = np.zeros_like(m)
    for k in range(C):
        d = l[:, k] - m
        e = np.exp(d)
        s = s + e
        a = a + e * d
    H = np.log(s) - a / s
    assert H.dtype == np.float32
    return np.minimum(np.float32(1), np.maximum(np.float32(0), H / np.log(np.float32(C))))


# ------------------------------------------------------------------------------------------------------------------ safe pixels
def safe_vector(C: int) -> torch.Tensor:
    """Logits (1, 0, 0, ...): confidence e / (e + C - 1), far from every edge of 10, 15 and 16 bins for C = 2, 9, 16 (the tests assert it)."""
    v = torch.zeros(C, dtype=torch.float64)
    v[0] = 1.0
    return v


def make_safe(logits: torch.Tensor, bins_list=(10, 15, 16), margin: float = 1e-5):
    """(logits with unsafe pixels replaced by `safe_vector`, replaced share): a pixel is unsafe when its float64 confidence lies within
    `margin` of an inner edge of any of `bins_list`, or the gap between its two largest probabilities is below `margin`."""
    m = model(logits, "logits")
    C = logits.shape[1]
    unsafe = m["gap"] < margin if C > 1 else torch.zeros_like(m["conf"], dtype=torch.bool)
    for bins in bins_list:
        pos = m["conf"] * bins
        near = (pos - pos.round()).abs() < margin * bins
        unsafe |= near & (pos.round() >= 1) & (pos.round() <= bins - 1)
    out = logits.clone()
    vec = safe_vector(C).to(logits.dtype)
    out.permute(0, 2, 3, 1)[unsafe] = vec
    return out, float(unsafe.double().mean())

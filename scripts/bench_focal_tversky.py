"""What the focal cross-entropy and the Tversky overlap cost.  Two measurements, device events around alternating blocks, medians and block
ranges, everything in one run so that the plain entries measured beside them are the yardstick.
  1. forward + backward of the tc_seg_loss_*_ft entries beside tc_seg_loss_fwd_tok / _bwd_tok and tc_seg_loss_*_w, in the captured step's form:
     bf16 token-major logits of 16 x 9 x 224 x 224 in rows padded to 16, no probability map (the backward recomputes the softmax);
     with the bytes each launch moves and the rate;
  2. the replayed training step (GraphedStep, bf16, the same batch) with the default loss and with focal_gamma = 2, Tversky(0.3, 0.7).
python scripts/bench_focal_tversky.py [--block 300] [--rounds 9] [--skip-step]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transception_amd import MSTransception
from transception_amd._lib import TC_BF16, TC_IGNORE_NONE, TC_OVERLAP_DICE, TC_OVERLAP_TVERSKY, lib
from transception_amd.seeded_init import seeded_input, seeded_labels, seeded_state_dict
from transception_amd.train import FusedSGD, GraphedStep, SegLoss, train_step

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--classes", type=int, default=9)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--block", type=int, default=300, help="launches per timed block")
ap.add_argument("--rounds", type=int, default=9, help="timed blocks per variant, alternating")
ap.add_argument("--step-block", type=int, default=10, help="replayed steps per timed block")
ap.add_argument("--skip-step", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda:0")
L = lib()
stream = torch.cuda.current_stream(dev).cuda_stream
N, C, S = args.batch, args.classes, args.size
HW, LD = S * S, 16
g = torch.Generator().manual_seed(0)


def blocks(fns, n, rounds):
    for fn in fns.values():                              # warm: code objects loaded, every shape seen
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / n)
    return ms


def summary(ms, nbytes=None):
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"median_us": med * 1e3, "min_max_us": [min(v) * 1e3, max(v) * 1e3]}
        if nbytes:
            out[k]["bytes"] = nbytes[k.split("_")[0]]
            out[k]["tb_per_s"] = out[k]["bytes"] / med / 1e9
    return out


# ------------------------------------------------------------------------------------------------ 1: the loss launches
logits = torch.zeros((N * HW, LD), dtype=torch.bfloat16, device=dev)
logits[:, :C] = (torch.randn((N * HW, C), generator=g) * 2).to(dev)
labels = torch.randint(0, C, (N, HW), generator=g).to(dev)
weights = (0.25 + 3.75 * torch.rand(2 * C, generator=g)).to(dev)
sums = torch.zeros(1 + 3 * C, dtype=torch.float32, device=dev)
L.tc_seg_loss_fwd_tok(logits.data_ptr(), LD, labels.data_ptr(), None, sums.data_ptr(), N, C, HW, TC_BF16, stream)
torch.cuda.synchronize()
fixed = sums.clone()                                     # the backward reads these; the timed forwards keep adding into `sums`
dlogits = torch.empty((N * HW, LD), dtype=torch.bfloat16, device=dev)
lp, yp, wp, sp, fp, dp = logits.data_ptr(), labels.data_ptr(), weights.data_ptr(), sums.data_ptr(), fixed.data_ptr(), dlogits.data_ptr()
npix = float(N * HW)


def ft(gamma, overlap, alpha=0.5, beta=0.5):
    return (lambda: L.tc_seg_loss_fwd_ft(lp, LD, yp, wp, TC_IGNORE_NONE, gamma, overlap, None, sp, N, C, HW, TC_BF16, stream),
            lambda: L.tc_seg_loss_bwd_ft(None, lp, LD, yp, wp, TC_IGNORE_NONE, fp, dp, LD, N, C, HW, 0.4, 0.6, gamma, overlap, alpha, beta, 1.0, None,
                                         TC_BF16, stream))


variants = {"plain": (lambda: L.tc_seg_loss_fwd_tok(lp, LD, yp, None, sp, N, C, HW, TC_BF16, stream),
                      lambda: L.tc_seg_loss_bwd_tok(None, lp, LD, yp, fp, dp, LD, N, C, HW, 0.4, 0.6, npix, 1.0, None, TC_BF16, stream)),
            "weighted": (lambda: L.tc_seg_loss_fwd_w(lp, LD, yp, wp, TC_IGNORE_NONE, None, sp, N, C, HW, TC_BF16, stream),
                         lambda: L.tc_seg_loss_bwd_w(None, lp, LD, yp, wp, TC_IGNORE_NONE, fp, dp, LD, N, C, HW, 0.4, 0.6, 1.0, None, TC_BF16, stream)),
            "focal2-dice": ft(2.0, TC_OVERLAP_DICE),
            "gamma0-tversky": ft(0.0, TC_OVERLAP_TVERSKY, 0.3, 0.7),
            "focal2-tversky": ft(2.0, TC_OVERLAP_TVERSKY, 0.3, 0.7),
            "focal0.5-tversky": ft(0.5, TC_OVERLAP_TVERSKY, 0.3, 0.7)}
fns = {f"{d}_{name}": pair[i] for name, pair in variants.items() for i, d in enumerate(("fwd", "bwd"))}
# forward: logits rows and labels read; backward: the same read, dlogits rows written
nbytes = {"fwd": N * HW * (LD * 2 + 8), "bwd": N * HW * (2 * LD * 2 + 8)}
loss = summary(blocks(fns, args.block, args.rounds), nbytes)
out = {"batch": N, "classes": C, "size": S, "row_pitch": LD, "dtype": "bf16", "launches_per_block": args.block, "blocks": args.rounds, "loss": loss}
for d in ("fwd", "bwd"):
    out[f"{d}_ratio_to_plain"] = {name: loss[f"{d}_{name}"]["median_us"] / loss[f"{d}_plain"]["median_us"] for name in variants}

# ------------------------------------------------------------------------------------------------ 2: the replayed step
if not args.skip_step:
    x = torch.from_numpy(seeded_input(N, size=S)).to(dev)
    y = torch.from_numpy(seeded_labels(N, size=S)).to(dev)
    steps = {}
    for name, kw in (("default", {}), ("focal2-tversky", dict(focal_gamma=2.0, overlap="tversky", tversky_alpha=0.3, tversky_beta=0.7))):
        m = MSTransception(num_classes=C)
        m.load_state_dict(seeded_state_dict(), strict=True)
        m.to(dev).train()
        m.set_compute_dtype(torch.bfloat16)
        lf, opt = SegLoss(C, **kw), FusedSGD(m, lr=0.01)
        train_step(m, lf, opt, x, y)
        steps[name] = GraphedStep(m, lf, opt, x, y, None, warmup=2)
    out["step"] = {"steps_per_block": args.step_block, "blocks": args.rounds,
                   **summary(blocks({k: (lambda s=s: s()) for k, s in steps.items()}, args.step_block, args.rounds))}
print(json.dumps(out))

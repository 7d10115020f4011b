"""What the top-k (hard-pixel) cross-entropy costs.  Device events around alternating blocks, medians and block ranges, everything in one
run so that the _ft entries and the default step measured beside the new ones are the yardstick.
  1. tc_seg_loss_fwd_topk beside tc_seg_loss_fwd_ft, tc_topk_select (its launches and their total time), tc_seg_loss_bwd_topk beside
     tc_seg_loss_bwd_ft, in the captured step's form: bf16 token-major logits of 16 x 9 x 224 x 224 in rows padded to 16, no probability
     map (the backward recomputes the softmax); with the bytes each launch moves and the rate;
  2. the replayed training step (GraphedStep, bf16, the same batch) with the default loss and with ce_topk = 0.1.
python scripts/bench_topk.py [--block 300] [--rounds 9] [--frac 0.1] [--skip-step]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transception_amd import MSTransception
from transception_amd._lib import TC_BF16, TC_IGNORE_NONE, TC_OVERLAP_DICE, lib
from transception_amd.seeded_init import seeded_input, seeded_labels, seeded_state_dict
from transception_amd.train import FusedSGD, GraphedStep, SegLoss, train_step

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--classes", type=int, default=9)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--frac", type=float, default=0.1)
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
SELECT_LAUNCHES = 11                                     # clear, 4 x (count, scan), sum, final: csrc/topk.hip
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
        if nbytes and k in nbytes:
            out[k]["bytes"] = nbytes[k]
            out[k]["tb_per_s"] = nbytes[k] / med / 1e9
    return out


# ------------------------------------------------------------------------------------------------ 1: the loss launches
logits = torch.zeros((N * HW, LD), dtype=torch.bfloat16, device=dev)
logits[:, :C] = (torch.randn((N * HW, C), generator=g) * 2).to(dev)
labels = torch.randint(0, C, (N, HW), generator=g).to(dev)
weights = (0.25 + 3.75 * torch.rand(2 * C, generator=g)).to(dev)
sums = torch.zeros(1 + 3 * C, dtype=torch.float32, device=dev)
values = torch.empty(N * HW, dtype=torch.float32, device=dev)
state = torch.tensor([args.frac] + [0.0] * 7, dtype=torch.float64, device=dev)
work = torch.empty((L.tc_topk_work_bytes() + 7) // 8, dtype=torch.int64, device=dev)
L.tc_seg_loss_fwd_topk(logits.data_ptr(), LD, labels.data_ptr(), weights.data_ptr(), TC_IGNORE_NONE, 0.0, TC_OVERLAP_DICE, None, sums.data_ptr(),
                       values.data_ptr(), N, C, HW, TC_BF16, stream)
L.tc_topk_select(values.data_ptr(), N * HW, state.data_ptr(), sums.data_ptr(), 1.0, work.data_ptr(), stream)
torch.cuda.synchronize()
fixed = sums.clone()                                     # the backward reads these; the timed forwards keep adding into `sums`
dlogits = torch.empty((N * HW, LD), dtype=torch.bfloat16, device=dev)
lp, yp, wp, sp, fp, dp = logits.data_ptr(), labels.data_ptr(), weights.data_ptr(), sums.data_ptr(), fixed.data_ptr(), dlogits.data_ptr()
vp, tp, kp = values.data_ptr(), state.data_ptr(), work.data_ptr()
fns = {"fwd_ft": lambda: L.tc_seg_loss_fwd_ft(lp, LD, yp, wp, TC_IGNORE_NONE, 0.0, TC_OVERLAP_DICE, None, sp, N, C, HW, TC_BF16, stream),
       "fwd_topk": lambda: L.tc_seg_loss_fwd_topk(lp, LD, yp, wp, TC_IGNORE_NONE, 0.0, TC_OVERLAP_DICE, None, sp, vp, N, C, HW, TC_BF16, stream),
       "select": lambda: L.tc_topk_select(vp, N * HW, tp, sp, 1.0, kp, stream),
       "bwd_ft": lambda: L.tc_seg_loss_bwd_ft(None, lp, LD, yp, wp, TC_IGNORE_NONE, fp, dp, LD, N, C, HW, 0.4, 0.6, 0.0, TC_OVERLAP_DICE, 0.5, 0.5, 1.0,
                                              None, TC_BF16, stream),
       "bwd_topk": lambda: L.tc_seg_loss_bwd_topk(None, lp, LD, yp, wp, TC_IGNORE_NONE, fp, dp, LD, N, C, HW, 0.4, 0.6, 0.0, TC_OVERLAP_DICE, 0.5, 0.5,
                                                  1.0, None, vp, tp, 1.0, TC_BF16, stream)}
# forward: logits rows and labels read (top-k: the value map written); select: the map read once per count pass and once for the sum;
# backward: rows and labels read, dlogits rows written (top-k: the map read)
px = N * HW
nbytes = {"fwd_ft": px * (LD * 2 + 8), "fwd_topk": px * (LD * 2 + 8 + 4), "select": px * 4 * 5, "bwd_ft": px * (2 * LD * 2 + 8),
          "bwd_topk": px * (2 * LD * 2 + 8 + 4)}
loss = summary(blocks(fns, args.block, args.rounds), nbytes)
loss["select"]["launches"] = SELECT_LAUNCHES
out = {"batch": N, "classes": C, "size": S, "row_pitch": LD, "dtype": "bf16", "frac": args.frac, "launches_per_block": args.block,
       "blocks": args.rounds, "value_map_bytes": px * 4, "work_bytes": L.tc_topk_work_bytes(), "state": state.cpu().tolist(), "loss": loss,
       "fwd_topk_over_ft": loss["fwd_topk"]["median_us"] / loss["fwd_ft"]["median_us"],
       "bwd_topk_over_ft": loss["bwd_topk"]["median_us"] / loss["bwd_ft"]["median_us"],
       "select_over_fwd_ft": loss["select"]["median_us"] / loss["fwd_ft"]["median_us"]}

# ------------------------------------------------------------------------------------------------ 2: the replayed step
if not args.skip_step:
    x = torch.from_numpy(seeded_input(N, size=S)).to(dev)
    y = torch.from_numpy(seeded_labels(N, size=S)).to(dev)
    steps = {}
    for name, kw in (("default", {}), ("ce_topk", dict(ce_topk=args.frac))):
        m = MSTransception(num_classes=C)
        m.load_state_dict(seeded_state_dict(), strict=True)
        m.to(dev).train()
        m.set_compute_dtype(torch.bfloat16)
        lf, opt = SegLoss(C, **kw), FusedSGD(m, lr=0.01)
        train_step(m, lf, opt, x, y)
        steps[name] = GraphedStep(m, lf, opt, x, y, None, warmup=2)
    out["step"] = {"steps_per_block": args.step_block, "blocks": args.rounds, "kernel_nodes": {k: s.kernel_nodes() for k, s in steps.items()},
                   **summary(blocks({k: (lambda s=s: s()) for k, s in steps.items()}, args.step_block, args.rounds))}
print(json.dumps(out))

"""What the dynamic loss scale adds to a captured step: GraphedStep replay with a static loss scale against the same step with a
train.DynamicLossScale that holds the same value (one more single-thread launch and two dependent scalar loads per step).
Two models side by side, blocks of replays alternating between them, each block timed with device events; medians, spread and the
difference as a share of the step.   python scripts/bench_loss_scale.py [--dtype f16] [--size 224] [--batch 16] [--block 50] [--rounds 12]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transception_amd import MSTransception
from transception_amd.seeded_init import seeded_input, seeded_labels, seeded_state_dict
from transception_amd.train import DynamicLossScale, FusedSGD, GraphedStep, SegLoss

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="f16", choices=["f16", "bf16"])
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--scale", type=float, default=4096.0)
ap.add_argument("--block", type=int, default=50, help="replays per timed block")
ap.add_argument("--rounds", type=int, default=12, help="timed blocks per variant, alternating")
ap.add_argument("--warmup", type=int, default=20, help="untimed replays per variant before the first block")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda:0")
x = torch.from_numpy(seeded_input(args.batch, size=args.size)).to(dev)
y = torch.from_numpy(seeded_labels(args.batch, size=args.size)).to(dev)
sd = seeded_state_dict()


def make(loss_scale):
    m = MSTransception(num_classes=9)
    m.load_state_dict(sd, strict=True)
    m.to(dev).train()
    m.set_compute_dtype({"f16": torch.float16, "bf16": torch.bfloat16}[args.dtype])
    opt = FusedSGD(m, lr=0.01)
    return GraphedStep(m, SegLoss(9, loss_scale=loss_scale), opt, x, y, None, warmup=3), opt


scaler = DynamicLossScale(init_scale=args.scale, growth_interval=10 ** 9)          # holds its value unless a step overflows
steps = {"static": make(args.scale), "dynamic": make(scaler)}
for st, _ in steps.values():
    for _ in range(args.warmup):
        st()
torch.cuda.synchronize()
ms = {k: [] for k in steps}
for _ in range(args.rounds):
    for k, (st, _) in steps.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.block):
            st()
        b.record()
        b.synchronize()
        ms[k].append(a.elapsed_time(b) / args.block)
med = {k: statistics.median(v) for k, v in ms.items()}
out = {"dtype": args.dtype, "size": args.size, "batch": args.batch, "scale": args.scale, "replays_per_block": args.block, "blocks": args.rounds,
       "static_ms": med["static"], "dynamic_ms": med["dynamic"],
       "static_ms_min_max": [min(ms["static"]), max(ms["static"])], "dynamic_ms_min_max": [min(ms["dynamic"]), max(ms["dynamic"])],
       "difference_us": (med["dynamic"] - med["static"]) * 1e3, "difference_percent_of_step": 100.0 * (med["dynamic"] - med["static"]) / med["static"],
       "kernel_nodes": {k: st.kernel_nodes() for k, (st, _) in steps.items()},
       "dynamic_scale_after": scaler.value(), "dynamic_skipped": scaler.skipped(),
       "static_last_step_skipped": steps["static"][1].last_step_skipped()}
print(json.dumps(out))

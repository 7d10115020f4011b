"""What the weight average costs.  Two measurements, each in alternating blocks timed with device events; medians and block ranges.
  1. the replayed B = 16, 224^2 training step (GraphedStep, FusedAdamW with no_decay="norm_bias") without and with a WeightEMA attached,
     two models side by side in one process on the same build.  The arm without is what the step was before the feature;
  2. the two new launches alone (tc_ema_advance + tc_ema_update_multi) on the arenas the replays left, beside tc_adam_step_multi on the
     same model, and tc_swap_f32 on the whole arena.  The update moves 12 bytes per live weight (w read, e read and written), Adam 30.
python scripts/bench_ema.py [--dtype bf16] [--size 224] [--batch 16] [--block 50] [--rounds 12] [--update-block 1000]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transception_amd import MSTransception
from transception_amd.seeded_init import seeded_input, seeded_labels, seeded_state_dict
from transception_amd._lib import lib
from transception_amd.train import FusedAdamW, GraphedStep, SegLoss, WeightEMA, train_step

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="bf16", choices=["f16", "bf16"])
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--decay", type=float, default=0.999)
ap.add_argument("--block", type=int, default=50, help="replays per timed block of the whole step")
ap.add_argument("--update-block", type=int, default=1000, help="launches per timed block of the kernels alone")
ap.add_argument("--rounds", type=int, default=12, help="timed blocks per variant, alternating")
ap.add_argument("--warmup", type=int, default=20, help="untimed replays per variant before the first block")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda:0")
x = torch.from_numpy(seeded_input(args.batch, size=args.size)).to(dev)
y = torch.from_numpy(seeded_labels(args.batch, size=args.size)).to(dev)
sd = seeded_state_dict()


def make(with_ema):
    m = MSTransception(num_classes=9)
    m.load_state_dict(sd, strict=True)
    m.to(dev).train()
    m.set_compute_dtype({"f16": torch.float16, "bf16": torch.bfloat16}[args.dtype])
    # (a learning rate small enough that hundreds of steps on one batch keep every value finite; the time does not depend on it)
    opt = FusedAdamW(m, lr=1e-5, no_decay="norm_bias")
    if with_ema:
        opt.ema = WeightEMA(m, decay=args.decay)
    loss_fn = SegLoss(9, loss_scale=4096.0 if args.dtype == "f16" else 1.0)
    train_step(m, loss_fn, opt, x, y)                    # eager: the optimiser's and the average's arenas exist before the capture
    return GraphedStep(m, loss_fn, opt, x, y, None, warmup=3), opt, m


def blocks(fns, n, rounds):
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


steps = {"plain": make(False), "ema": make(True)}
for st, _, _ in steps.values():
    for _ in range(args.warmup):
        st()
torch.cuda.synchronize()
step_ms = blocks({k: st for k, (st, _, _) in steps.items()}, args.block, args.rounds)

# the kernels alone, launched directly on the arenas the replays left
L = lib()
stream = torch.cuda.current_stream(dev).cuda_stream
_, ao, am = steps["ema"]
ema = ao.ema
n_before = ema.updates()


def ema_update():
    L.tc_ema_advance(ema._state.data_ptr(), None, ema.decay, int(ema.warmup), stream)
    L.tc_ema_update_multi(ema.shadow.data_ptr(), am._flat.data_ptr(), ema._segs_dev.data_ptr(), ema._nseg, ema._maxlen, ema._state.data_ptr(),
                          None, stream)


def adam_update():
    L.tc_adam_step_multi(am._flat.data_ptr(), am._gflat.data_ptr(), ao.m.data_ptr(), ao.v.data_ptr(), ao._segs_dev.data_ptr(),
                         ao._wd_dev.data_ptr(), ao._nseg, ao._maxlen, ao.lr, ao.lr_dev.data_ptr(), ao.betas[0], ao.betas[1], ao.eps, ao.wd, 1,
                         1.0, None, float("inf"), am._flat_lp.data_ptr(), am._tc_dtype(), None, ao._adam_state.data_ptr(), stream)


def swap():
    L.tc_swap_f32(am._flat.data_ptr(), ema.shadow.data_ptr(), am._flat.numel(), stream)


variants = {"ema": ema_update, "adamw": adam_update, "swap": swap}
for fn in variants.values():
    for _ in range(6):                                   # (an even number: the swap leaves the arenas where they were)
        fn()
torch.cuda.synchronize()
assert args.update_block % 2 == 0
upd_ms = blocks(variants, args.update_block, args.rounds)
am.invalidate_working_copy()


def summary(ms):
    return {k: {"median_ms": statistics.median(v), "min_max_ms": [min(v), max(v)]} for k, v in ms.items()}


su, ss = summary(upd_ms), summary(step_ms)
live = sum(n for _, n in ema.segments())
arena = am._flat.numel()
out = {"dtype": args.dtype, "size": args.size, "batch": args.batch, "decay": args.decay, "blocks": args.rounds,
       "live_weights": live, "arena_weights": arena, "segments": {"ema": ema._nseg, "adamw": ao._nseg},
       "step": ss, "step_per_block": args.block,
       "step_difference_us": (ss["ema"]["median_ms"] - ss["plain"]["median_ms"]) * 1e3,
       "step_difference_percent": 100.0 * (ss["ema"]["median_ms"] - ss["plain"]["median_ms"]) / ss["plain"]["median_ms"],
       "kernel_nodes": {k: st.kernel_nodes() for k, (st, _, _) in steps.items()},
       "kernels": su, "kernels_per_block": args.update_block,
       "bytes_per_weight": {"ema": 12, "adamw": 30, "swap": 16},
       "predicted_ema_gigabytes_per_step": live * 12 / 1e9,
       "tb_per_s": {"ema": live * 12 / su["ema"]["median_ms"] / 1e9, "adamw": live * 30 / su["adamw"]["median_ms"] / 1e9,
                    "swap": arena * 16 / su["swap"]["median_ms"] / 1e9},
       "ema_updates_counted_on_device": {"after_the_steps": n_before, "at_the_end": ema.updates()},
       "finite": {k: bool(torch.isfinite(m.flat_parameters()).all()) for k, (_, _, m) in steps.items()}}
print(json.dumps(out))

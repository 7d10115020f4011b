"""What AdamW costs against SGD.  Two measurements, each in alternating blocks timed with device events; medians and block ranges.
  1. the update alone on the model's real arena (16-bit working copy written; AdamW over the per-class table of no_decay="norm_bias" and
     over SGD's merged table):
     tc_adam_step_multi against tc_sgd_step_multi, launched directly on the arenas of the two models below.  The kernels move
     30 and 22 bytes per live weight, so the expected ratio is near 30 / 22 = 1.36;
  2. the replayed B = 16, 224^2 training step (GraphedStep) under each optimiser, two models side by side.
python scripts/bench_optimizer.py [--dtype bf16] [--size 224] [--batch 16] [--block 50] [--rounds 12] [--update-block 1000]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transception_amd import MSTransception
from transception_amd.seeded_init import seeded_input, seeded_labels, seeded_state_dict
from transception_amd._lib import lib
from transception_amd.train import FusedAdamW, FusedSGD, GraphedStep, SegLoss

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="bf16", choices=["f16", "bf16"])
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--block", type=int, default=50, help="replays per timed block of the whole step")
ap.add_argument("--update-block", type=int, default=1000, help="updates per timed block of the update alone")
ap.add_argument("--rounds", type=int, default=12, help="timed blocks per variant, alternating")
ap.add_argument("--warmup", type=int, default=20, help="untimed replays per variant before the first block")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda:0")
x = torch.from_numpy(seeded_input(args.batch, size=args.size)).to(dev)
y = torch.from_numpy(seeded_labels(args.batch, size=args.size)).to(dev)
sd = seeded_state_dict()


def make(kind):
    m = MSTransception(num_classes=9)
    m.load_state_dict(sd, strict=True)
    m.to(dev).train()
    m.set_compute_dtype({"f16": torch.float16, "bf16": torch.bfloat16}[args.dtype])
    # (learning rates small enough that hundreds of steps on one batch keep every value finite; the time does not depend on them)
    opt = FusedSGD(m, lr=1e-3) if kind == "sgd" else FusedAdamW(m, lr=1e-5, no_decay="norm_bias")
    return GraphedStep(m, SegLoss(9, loss_scale=4096.0 if args.dtype == "f16" else 1.0), opt, x, y, None, warmup=3), opt, m


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


steps = {k: make(k) for k in ("sgd", "adamw")}
for st, _, _ in steps.values():
    for _ in range(args.warmup):
        st()
torch.cuda.synchronize()
step_ms = blocks({k: st for k, (st, _, _) in steps.items()}, args.block, args.rounds)
# the update alone: the two kernels launched directly on the arenas the replays left (gradients of the last step, live moments, t > 0)
L = lib()
stream = torch.cuda.current_stream(dev).cuda_stream
(_, so, sm), (_, ao, am) = steps["sgd"], steps["adamw"]


def sgd_update():
    L.tc_sgd_step_multi(sm._flat.data_ptr(), sm._gflat.data_ptr(), so.buf.data_ptr(), so._segs_dev.data_ptr(), so._nseg, so._maxlen, so.lr,
                        so.lr_dev.data_ptr(), so.momentum, so.wd, 1.0, 0, None, float("inf"), sm._flat_lp.data_ptr(), sm._tc_dtype(), stream)


def adam_update(o=ao):
    L.tc_adam_step_multi(am._flat.data_ptr(), am._gflat.data_ptr(), ao.m.data_ptr(), ao.v.data_ptr(), o._segs_dev.data_ptr(),
                         o._wd_dev.data_ptr() if o._wd_dev is not None else None, o._nseg, o._maxlen, ao.lr, ao.lr_dev.data_ptr(), ao.betas[0],
                         ao.betas[1], ao.eps, ao.wd, 1, 1.0, None, float("inf"), am._flat_lp.data_ptr(), am._tc_dtype(), None,
                         ao._adam_state.data_ptr(), stream)


# the same kernel over SGD's segment table (no_decay=None: one decay, adjacent tensors merged): the grid is (blocks of the longest segment) x
# (segments), so the per-class table of no_decay launches many workgroups that find a short segment already covered and leave
one_decay = FusedAdamW(am, lr=ao.lr)
one_decay._tables(am._flat)
variants = {"sgd": sgd_update, "adamw": adam_update, "adamw_one_decay": lambda: adam_update(one_decay)}
for fn in variants.values():
    for _ in range(5):
        fn()
torch.cuda.synchronize()
upd_ms = blocks(variants, args.update_block, args.rounds)


def summary(ms):
    return {k: {"median_ms": statistics.median(v), "min_max_ms": [min(v), max(v)]} for k, v in ms.items()}


su, ss = summary(upd_ms), summary(step_ms)
live = sum(n for _, n in steps["adamw"][1]._segs())
lp_bytes = 2
out = {"dtype": args.dtype, "size": args.size, "batch": args.batch, "blocks": args.rounds,
       "live_weights": live, "segments": {"sgd": so._nseg, "adamw": ao._nseg, "adamw_one_decay": one_decay._nseg},
       "update": su, "update_per_block": args.update_block,
       "update_ratio_adamw_over_sgd": su["adamw"]["median_ms"] / su["sgd"]["median_ms"],
       "update_ratio_range": [su["adamw"]["min_max_ms"][0] / su["sgd"]["min_max_ms"][1], su["adamw"]["min_max_ms"][1] / su["sgd"]["min_max_ms"][0]],
       "update_bytes_per_weight": {"sgd": 20 + lp_bytes, "adamw": 28 + lp_bytes},
       "update_ratio_one_decay_over_sgd": su["adamw_one_decay"]["median_ms"] / su["sgd"]["median_ms"],
       "update_tb_per_s": {"sgd": live * (20 + lp_bytes) / su["sgd"]["median_ms"] / 1e9, "adamw": live * (28 + lp_bytes) / su["adamw"]["median_ms"] / 1e9,
                           "adamw_one_decay": live * (28 + lp_bytes) / su["adamw_one_decay"]["median_ms"] / 1e9},
       "step": ss, "step_per_block": args.block,
       "step_difference_us": (ss["adamw"]["median_ms"] - ss["sgd"]["median_ms"]) * 1e3,
       "step_difference_percent": 100.0 * (ss["adamw"]["median_ms"] - ss["sgd"]["median_ms"]) / ss["sgd"]["median_ms"],
       "kernel_nodes": {k: st.kernel_nodes() for k, (st, _, _) in steps.items()},
       "adam_steps_counted_on_device": steps["adamw"][1].device_step(),
       "finite": {k: bool(torch.isfinite(m.flat_parameters()).all()) for k, (_, _, m) in steps.items()}}
print(json.dumps(out))

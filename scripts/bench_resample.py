"""What evaluating at label resolution costs.  Device events around alternating blocks, medians and block ranges, everything warmed.
  1. tc_resample_scores, labels only, at 16 x 9 x 224 x 224 -> 512 x 512 with fp32 and bf16 sources, with the bytes it moves (taken from the
     shapes: the source once, the uint8 labels once) and the rate;
  2. the same result from stock torch ops in the same process -- F.interpolate(..., mode="bilinear", align_corners=False).argmax(1) -- which
     writes and re-reads the fp32 [N,C,512,512] map (its bytes likewise from the shapes); and today's path, the argmax at the network size
     followed by the order-0 zoom of the labels (tc_argmax_counts + zoom_labels), for scale;
  3. evaluate_volume (device zooms, device Dice) on one synthetic 148 x 512 x 512 volume with resample="labels" and "scores", without TTA and
     with TTA.flips().
python scripts/bench_resample.py [--dtype bf16] [--block 200] [--rounds 9] [--skip-volume]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F
from transception_amd import MSTransception
from transception_amd._lib import TC_BF16, TC_F32, lib
from transception_amd.evaluate import TTA, argmax_counts, evaluate_volume, zoom_labels
from transception_amd.seeded_init import seeded_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="bf16", choices=["f32", "f16", "bf16"], help="compute dtype of the network in the volume measurement")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--classes", type=int, default=9)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--out", type=int, default=512)
ap.add_argument("--block", type=int, default=200, help="launches per timed block")
ap.add_argument("--rounds", type=int, default=9, help="timed blocks per variant, alternating")
ap.add_argument("--volume", type=int, nargs=3, default=[148, 512, 512])
ap.add_argument("--volume-repeats", type=int, default=3)
ap.add_argument("--skip-volume", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda:0")
L = lib()
stream = torch.cuda.current_stream(dev).cuda_stream
N, C, S, O = args.batch, args.classes, args.size, args.out
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


def summary(ms, nbytes):
    out = {}
    for k, v in ms.items():
        med = statistics.median(v)
        out[k] = {"median_us": med * 1e3, "min_max_us": [min(v) * 1e3, max(v) * 1e3], "bytes": nbytes[k], "tb_per_s": nbytes[k] / med / 1e9}
    return out


# ------------------------------------------------------------------------------------------------ 1 + 2: the kernel and the torch composition
pred = torch.empty((N, O, O), dtype=torch.uint8, device=dev)
small, big = N * S * S, N * O * O
kernel = {}
for name, dt, tc in (("f32", torch.float32, TC_F32), ("bf16", torch.bfloat16, TC_BF16)):
    lg = (torch.randn((N, C, S, S), generator=g) * 4).to(dt).to(dev)
    e = lg.element_size()
    fns = {"hip_labels": lambda lg=lg, tc=tc: L.tc_resample_scores(lg.data_ptr(), tc, None, pred.data_ptr(), N, C, S, S, O, O, stream),
           "torch_interpolate_argmax": lambda lg=lg: F.interpolate(lg, size=(O, O), mode="bilinear", align_corners=False).argmax(1).to(torch.uint8),
           "today_argmax_zoom_labels": lambda lg=lg: zoom_labels(argmax_counts(lg)[0], (O, O))}
    # the composition: source read, resampled map written in the source's dtype and read again, int64 labels written, read, uint8 written
    nbytes = {"hip_labels": small * C * e + big, "torch_interpolate_argmax": small * C * e + 2 * big * C * e + big * (8 + 8 + 1),
              "today_argmax_zoom_labels": small * C * e + 2 * small + big * (8 + 8 + 1)}
    kernel[name] = summary(blocks(fns, args.block, args.rounds), nbytes)
    k = kernel[name]
    k["torch_over_hip"] = k["torch_interpolate_argmax"]["median_us"] / k["hip_labels"]["median_us"]
    ref = F.interpolate(lg.float(), size=(O, O), mode="bilinear", align_corners=False).argmax(1).to(torch.uint8)
    L.tc_resample_scores(lg.data_ptr(), tc, None, pred.data_ptr(), N, C, S, S, O, O, stream)
    k["labels_differing_from_torch_fp32"] = float((pred != ref).float().mean())       # near-ties under torch's fp32 coordinates only

out = {"batch": N, "classes": C, "size": S, "out": O, "launches_per_block": args.block, "blocks": args.rounds, "resample": kernel,
       "resampled_map_bytes_fp32": big * C * 4}

# ------------------------------------------------------------------------------------------------ 3: a whole volume
if not args.skip_volume:
    m = MSTransception(num_classes=C)
    m.load_state_dict(seeded_state_dict(), strict=True)
    m.to(dev).eval()
    m.set_compute_dtype({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype])
    rng = np.random.default_rng(0)
    D, X, Y = args.volume
    image = rng.random((D, X, Y), dtype=np.float32)
    label = rng.integers(0, C, (D, X, Y)).astype(np.uint8)
    variants = {"labels": ("labels", None), "scores": ("scores", None), "labels_flips": ("labels", TTA.flips()), "scores_flips": ("scores", TTA.flips())}
    times = {k: [] for k in variants}
    for rep in range(args.volume_repeats + 1):           # the first pass over the variants is the warm-up
        for k, (mode, tta) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate_volume(m, image, label, C, (S, S), batch=N, device_metrics=True, tta=tta, resample=mode)      # ends in a copy to the host
            torch.cuda.synchronize()
            if rep:
                times[k].append(time.perf_counter() - t0)
    out["volume"] = {"shape": [D, X, Y], "dtype": args.dtype, "repeats": args.volume_repeats,
                     "seconds": {k: {"median": statistics.median(v), "min_max": [min(v), max(v)]} for k, v in times.items()}}
print(json.dumps(out))

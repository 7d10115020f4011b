"""What test-time augmentation costs.  Three measurements, device events around alternating blocks, medians and block ranges.
  1. the two kernels alone at 16 x 9 x 224 x 224, fp32 and bf16 logits: tc_tta_view (a flip view and a transposed one) and tc_tta_accumulate as
     the first view (accumulator written), a middle view (read and written) and the last view (read, labels written), flip and transposed;
     with the bytes each moves and the rate;
  2. the same step from stock torch ops in the same process -- per view softmax, flip back, add; then divide and argmax -- which is the
     baseline: before this feature the library had no test-time augmentation;
  3. evaluate_volume (device zooms, device Dice) on one synthetic 148 x 512 x 512 volume with no TTA and with 1, 4 and 8 views.
python scripts/bench_tta.py [--dtype bf16] [--block 500] [--rounds 9] [--skip-volume]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from transception_amd import MSTransception
from transception_amd._lib import TC_BF16, TC_F32, lib
from transception_amd.evaluate import TTA, evaluate_volume
from transception_amd.seeded_init import seeded_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="bf16", choices=["f32", "f16", "bf16"], help="compute dtype of the network in the volume measurement")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--classes", type=int, default=9)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--block", type=int, default=500, help="launches per timed block")
ap.add_argument("--rounds", type=int, default=9, help="timed blocks per variant, alternating")
ap.add_argument("--volume", type=int, nargs=3, default=[148, 512, 512])
ap.add_argument("--volume-repeats", type=int, default=3)
ap.add_argument("--skip-volume", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "this measurement needs the GPU"
dev = torch.device("cuda:0")
L = lib()
stream = torch.cuda.current_stream(dev).cuda_stream
N, C, S = args.batch, args.classes, args.size
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


# ------------------------------------------------------------------------------------------------ 1 + 2: the kernels and the torch composition
src = torch.rand((N, S, S), generator=g).to(dev)
dst = torch.empty((N, S, S), dtype=torch.float32, device=dev)
acc = torch.zeros((N, C, S, S), dtype=torch.float32, device=dev)
pred = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
pix = N * S * S
kernels = {}
for name, dt, tc in (("f32", torch.float32, TC_F32), ("bf16", torch.bfloat16, TC_BF16)):
    lg = (torch.randn((N, C, S, S), generator=g) * 4).to(dt).to(dev)
    e = lg.element_size()

    def hip(view, first, last, lg=lg, tc=tc):
        return lambda: L.tc_tta_accumulate(lg.data_ptr(), tc, acc.data_ptr(), pred.data_ptr() if last else None, N, C, S, S, view, first, stream)

    def torch_view(view, lg=lg):                         # one middle view from stock ops: softmax, flip back, add
        dims = [d for bit, d in ((1, -2), (2, -1)) if view & bit]

        def run():
            p = torch.softmax(lg.float(), dim=1)
            if view & 4:
                p = p.transpose(-2, -1)
            if dims:
                p = p.flip(dims)
            acc.add_(p)
        return run

    def torch_tail():                                    # after the last view: divide, argmax
        return lambda: acc.div(8).argmax(dim=1).to(torch.uint8)

    fns = {"hip_first_flip": hip(3, 1, False), "hip_middle_flip": hip(3, 0, False), "hip_last_flip": hip(3, 0, True),
           "hip_middle_identity": hip(0, 0, False), "hip_middle_transposed": hip(7, 0, False), "hip_last_transposed": hip(7, 0, True),
           "torch_middle_flip": torch_view(3), "torch_middle_transposed": torch_view(7), "torch_tail": torch_tail()}
    nbytes = {"hip_first_flip": pix * C * (e + 4), "hip_middle_flip": pix * C * (e + 8), "hip_last_flip": pix * (C * (e + 4) + 1),
              "hip_middle_identity": pix * C * (e + 8), "hip_middle_transposed": pix * C * (e + 8), "hip_last_transposed": pix * (C * (e + 4) + 1)}
    kernels[name] = summary(blocks(fns, args.block, args.rounds), nbytes)
    acc.zero_()

view_fns = {"view_identity": lambda: L.tc_tta_view(src.data_ptr(), dst.data_ptr(), N, S, S, 0, 0.5, 0.5, stream),
            "view_flip": lambda: L.tc_tta_view(src.data_ptr(), dst.data_ptr(), N, S, S, 3, 0.5, 0.5, stream),
            "view_transposed": lambda: L.tc_tta_view(src.data_ptr(), dst.data_ptr(), N, S, S, 7, 0.5, 0.5, stream),
            "torch_view_flip": lambda: ((src - 0.5) / 0.5).flip([-2, -1]).unsqueeze(1).contiguous()}
views = summary(blocks(view_fns, args.block, args.rounds), {k: pix * 8 for k in ("view_identity", "view_flip", "view_transposed")})

out = {"batch": N, "classes": C, "size": S, "launches_per_block": args.block, "blocks": args.rounds, "accumulate": kernels, "view": views,
       "accumulator_bytes": pix * C * 4}

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
    variants = {"none": None, "views_1": TTA((0,)), "views_4": TTA.flips(), "views_8": TTA.dihedral()}
    times = {k: [] for k in variants}
    for rep in range(args.volume_repeats + 1):           # the first pass over the variants is the warm-up
        for k, tta in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            evaluate_volume(m, image, label, C, (S, S), batch=N, device_metrics=True, tta=tta)      # ends in a copy to the host
            torch.cuda.synchronize()
            if rep:
                times[k].append(time.perf_counter() - t0)
    out["volume"] = {"shape": [D, X, Y], "dtype": args.dtype, "repeats": args.volume_repeats,
                     "seconds": {k: {"median": statistics.median(v), "min_max": [min(v), max(v)]} for k, v in times.items()}}
print(json.dumps(out))

"""What the uncertainty maps and the calibration statistics cost.  Device events around alternating blocks, medians and block ranges.
  1. the two kernels alone at 16 x 9 x 224 x 224 -- tc_uncert_maps (entropy, confidence, label; with the mutual information for the sums) and
     tc_calib_stats (15 bins) on fp32 logits, bf16 logits and the fp32 accumulator of four views -- each beside the stock-torch expression
     of the same quantities in the same run, whose outputs are checked against the kernel's at this size first; with the bytes each kernel
     moves (from the shapes) and the rate;
  2. one synthetic 148 x 512 x 512 volume through evaluate_volume_calibration and predict_uncertainty, with no TTA and with four views.
python scripts/bench_uncertainty.py [--dtype bf16] [--block 200] [--rounds 9] [--skip-volume]"""
import argparse, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from transception_amd import MSTransception
from transception_amd._lib import TC_BF16, TC_F32, TC_UNCERT_LOGITS, TC_UNCERT_PROB_SUMS, lib
from transception_amd.evaluate import TTA, Calibration, evaluate_volume_calibration, predict_uncertainty, zoom_volume_to_network
from transception_amd.seeded_init import seeded_state_dict

ap = argparse.ArgumentParser()
ap.add_argument("--dtype", default="bf16", choices=["f32", "f16", "bf16"], help="compute dtype of the network in the volume measurement")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--classes", type=int, default=9)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--bins", type=int, default=15)
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
N, C, S, B = args.batch, args.classes, args.size, args.bins
g = torch.Generator().manual_seed(0)


def blocks(fns, n, rounds):
    for fn in fns.values():                              # warm: code objects loaded, every shape seen
        for _ in range(5):
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
        out[k] = {"median_us": med * 1e3, "min_max_us": [min(v) * 1e3, max(v) * 1e3]}
        if k in nbytes:
            out[k]["bytes"] = nbytes[k]
            out[k]["tb_per_s"] = nbytes[k] / med / 1e9
    return out


pix = N * S * S
ent, conf, mi = (torch.empty((N, S, S), dtype=torch.float32, device=dev) for _ in range(3))
pred = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
labels = torch.randint(0, C, (N, S, S), generator=g).to(torch.uint8).to(dev)
ves = (torch.rand((N, S, S), generator=g) * 4).to(dev)
work = torch.empty(L.tc_calib_work_bytes(B, C) // 8, dtype=torch.int64, device=dev)
stats = torch.empty(L.tc_calib_out_slots(B, C), dtype=torch.int64, device=dev)
logc = math.log(C)


def torch_maps(scores, logits, with_mi):
    """The same maps from stock ops: (entropy, confidence, label[, mutual information])."""
    if logits:
        logp = torch.log_softmax(scores.float(), dim=1)
        p = logp.exp()
        h = (-(p * logp).sum(dim=1) / logc).clamp_(0, 1)
    else:
        p = scores * 0.25
        h = (-torch.xlogy(p, p).sum(dim=1) / logc).clamp_(0, 1)
    c, k = p.max(dim=1)
    out = (h, c, k.to(torch.uint8))
    return out + ((h - ves * 0.25).clamp_(min=0),) if with_mi else out


def torch_calib(scores, logits):
    """The same statistics from stock ops, histograms on the device: (bin counts, confidence sums, correct per bin, n, nll, brier)."""
    p = torch.softmax(scores.float(), dim=1) if logits else scores * 0.25
    c, k = p.max(dim=1)
    y = labels.long()
    b = (c * B).long().clamp_(max=B - 1).flatten()
    ok = (k == y).flatten()
    py = p.gather(1, y.unsqueeze(1))[:, 0]
    brier = (p * p).sum(dim=1) - 2 * py + 1
    return (torch.bincount(b, minlength=B), torch.bincount(b, weights=c.flatten().double(), minlength=B), torch.bincount(b, weights=ok.double(), minlength=B),
            y.numel(), -torch.log(py.clamp(min=1.1754944e-38)).double().sum(), brier.double().sum())


kernels, checks = {}, {}
cases = [("logits_f32", (torch.randn((N, C, S, S), generator=g) * 3).to(dev), TC_F32, TC_UNCERT_LOGITS, 1.0),
         ("logits_bf16", (torch.randn((N, C, S, S), generator=g) * 3).to(torch.bfloat16).to(dev), TC_BF16, TC_UNCERT_LOGITS, 1.0),
         ("prob_sums_f32", sum(torch.softmax(torch.randn((N, C, S, S), generator=g) * 3, dim=1) for _ in range(4)).to(dev), TC_F32, TC_UNCERT_PROB_SUMS, 0.25)]
for name, sc, tc, kind, inv in cases:
    e, sums = sc.element_size(), kind == TC_UNCERT_PROB_SUMS

    def hip_maps(sc=sc, tc=tc, kind=kind, inv=inv, sums=sums):
        L.tc_uncert_maps(sc.data_ptr(), tc, kind, inv, ves.data_ptr() if sums else None, ent.data_ptr(), conf.data_ptr(), mi.data_ptr() if sums else None,
                         pred.data_ptr(), N, C, S, S, stream)

    def hip_calib(sc=sc, tc=tc, kind=kind, inv=inv):
        L.tc_calib_stats(sc.data_ptr(), tc, kind, inv, labels.data_ptr(), -1, 0, B, N, C, S, S, work.data_ptr(), stats.data_ptr(), stream)

    # equal outputs at this size, before anything is timed
    hip_maps()
    hip_calib()
    t = torch_maps(sc, not sums, sums)
    raw = stats.cpu().numpy()
    tb = torch_calib(sc, not sums)
    n = int(raw[3 * B])
    checks[name] = {"max_abs_entropy": float((ent - t[0]).abs().max()), "max_abs_confidence": float((conf - t[1]).abs().max()),
                    "labels_differ": int((pred != t[2]).sum()), "bin_counts_differ": int((torch.from_numpy(raw[0:3 * B:3]) != tb[0].cpu()).sum()),
                    "nll_per_pixel_diff": abs(float(raw[3 * B + 1:3 * B + 2].view(np.float64)[0]) - float(tb[4])) / n,
                    "brier_per_pixel_diff": abs(float(raw[3 * B + 2:3 * B + 3].view(np.float64)[0]) - float(tb[5])) / n, "n": n}
    if sums:
        checks[name]["max_abs_mutual_info"] = float((mi - t[3]).abs().max())
    assert checks[name]["max_abs_entropy"] < 1e-4 and checks[name]["max_abs_confidence"] < 1e-5 and n == pix == tb[3], checks[name]
    assert checks[name]["labels_differ"] <= pix // 10000 and checks[name]["bin_counts_differ"] <= 2 * B, checks[name]     # a rounding on an edge or a tie
    fns = {"hip_maps": hip_maps, "torch_maps": lambda sc=sc, sums=sums: torch_maps(sc, not sums, sums),
           "hip_calib": hip_calib, "torch_calib": lambda sc=sc, sums=sums: torch_calib(sc, not sums)}
    nbytes = {"hip_maps": pix * (C * e + 4 + 4 + 1 + (8 if sums else 0)), "hip_calib": pix * (C * e + 1)}
    kernels[name] = summary(blocks(fns, args.block, args.rounds), nbytes)

out = {"batch": N, "classes": C, "size": S, "bins": B, "launches_per_block": args.block, "blocks": args.rounds, "kernels": kernels, "checks": checks}

# ------------------------------------------------------------------------------------------------ 2: a whole volume
if not args.skip_volume:
    m = MSTransception(num_classes=C)
    m.load_state_dict(seeded_state_dict(), strict=True)
    m.to(dev).eval()
    m.set_compute_dtype({"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[args.dtype])
    rng = np.random.default_rng(0)
    D, X, Y = args.volume
    image = rng.random((D, X, Y), dtype=np.float32)
    label = rng.integers(0, C, (D, X, Y)).astype(np.uint8)
    slices = zoom_volume_to_network(torch.from_numpy(image).to(dev), (S, S))
    variants = {"calibration_none": lambda: evaluate_volume_calibration(m, image, label, C, (S, S), batch=N, calibration=Calibration(B)),
                "calibration_views_4": lambda: evaluate_volume_calibration(m, image, label, C, (S, S), batch=N, tta=TTA.flips(), calibration=Calibration(B)),
                "uncertainty_none": lambda: predict_uncertainty(m, slices, batch=N),
                "uncertainty_views_4": lambda: predict_uncertainty(m, slices, batch=N, tta=TTA.flips())}
    times = {k: [] for k in variants}
    for rep in range(args.volume_repeats + 1):           # the first pass over the variants is the warm-up
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                times[k].append(time.perf_counter() - t0)
    out["volume"] = {"shape": [D, X, Y], "dtype": args.dtype, "repeats": args.volume_repeats,
                     "seconds": {k: {"median": statistics.median(v), "min_max": [min(v), max(v)]} for k, v in times.items()}}
print(json.dumps(out))

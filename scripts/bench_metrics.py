"""Evaluation of one volume with the metric on the host (scipy, the default) against the metric on the device (device_metrics=True).

    python scripts/bench_metrics.py [--shape 148 512 512] [--reps 3] [--out profiles/metrics_device.json]
    python scripts/bench_metrics.py --metric-only            # metrics_device alone, e.g. under rocprofv3 --kernel-trace --stats
    python scripts/bench_metrics.py --spacing 3.0 0.8 0.8    # the metric alone with voxel spacing: host scipy, device unit spacing, device fp64

One seeded synthetic volume of Synapse test size with 8 organs of realistic extent, the seeded model in eval mode.  After one warm-up
of each, `evaluate_volume(..., with_hd95=True)` runs `reps` times with device_metrics off and on, alternating, under a host clock
around work that ends in a device synchronise.  The metric alone (`metrics_device` on label volumes already in HBM) is timed with
device events.  Both paths see the same prediction, and their results are compared.  Every repetition, the spread, the volume shape
and the source hash go into the json.

With `--spacing Z Y X` the metric alone is timed three ways on one pair of label volumes (the label volume and a displaced copy): the host
`calculate_metric_percase` per class with that spacing (host clock), `metrics_device` without spacing (the integer kernels) and
`metrics_device` with it (the fp64 kernels), the two device forms alternating, each run from resident label volumes to the results on the
host (host clock around a call that ends in the copy back).  After a warm-up of each; median and spread of every form, the ratio fp64 /
integer, the scratch of both forms and the largest difference between the fp64 form and the host go into the json (default
`profiles/metrics_spacing.json`)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# (centre, radii) as fractions of (D, H, W): spleen, right kidney, left kidney, gallbladder, liver, stomach, aorta, pancreas (labels 1..8)
ORGANS = [((0.55, 0.45, 0.78), (0.20, 0.09, 0.07)), ((0.40, 0.60, 0.33), (0.16, 0.06, 0.05)), ((0.40, 0.60, 0.67), (0.16, 0.06, 0.05)),
          ((0.50, 0.42, 0.38), (0.07, 0.03, 0.03)), ((0.60, 0.40, 0.30), (0.28, 0.16, 0.18)), ((0.55, 0.38, 0.62), (0.15, 0.09, 0.11)),
          ((0.50, 0.55, 0.50), (0.48, 0.025, 0.025)), ((0.45, 0.50, 0.50), (0.06, 0.035, 0.11))]


def synthetic_volume(shape, seed=0):
    g = np.random.default_rng(seed)
    D, H, W = shape
    z, y, x = np.meshgrid(np.linspace(0, 1, D, dtype=np.float32), np.linspace(0, 1, H, dtype=np.float32),
                          np.linspace(0, 1, W, dtype=np.float32), indexing="ij", sparse=True)
    label = np.zeros(shape, np.uint8)
    image = np.full(shape, 0.25, np.float32)
    for k in (5, 1, 2, 3, 4, 6, 7, 8):                                           # the liver first: the gallbladder lies inside its extent
        c, r = ORGANS[k - 1]
        wob = 1.0 + 0.15 * np.sin(9 * x + k) * np.cos(7 * y - k) + 0.1 * np.sin(11 * z + 2 * k)
        m = ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 < wob
        label[m] = k
        image[m] = 0.3 + 0.07 * k
    image = np.clip(image + g.normal(0, 0.03, shape).astype(np.float32), 0, 1)
    return image, label


def spread(ts):
    return {"runs_s": ts, "min_s": min(ts), "max_s": max(ts), "median_s": float(np.median(ts))}


def bench_spacing(a, shape, label, pred_d, lab_d):
    from provenance import source_digest
    from transception_amd.evaluate import calculate_metric_percase, metrics_device, metrics_scratch_bytes
    spacing = tuple(a.spacing)

    def device(sp):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = metrics_device(pred_d, lab_d, 9, voxelspacing=sp)                   # ends in the copy of the results to the host
        return time.perf_counter() - t0, r

    device(None), device(spacing)                                               # warm-up of both forms
    t_int, t_f64 = [], []
    for i in range(a.reps):
        t, r_int = device(None)
        t_int.append(t)
        t, r_f64 = device(spacing)
        t_f64.append(t)
        print(f"rep {i}: device unit spacing {t_int[-1]:.4f} s, device fp64 {t_f64[-1]:.4f} s", flush=True)
    pred = pred_d.cpu().numpy()
    t_host = []
    for i in range(a.host_reps):
        t0 = time.perf_counter()
        r_host = [calculate_metric_percase(pred == k, label == k, voxelspacing=spacing) for k in range(1, 9)]
        t_host.append(time.perf_counter() - t0)
        print(f"rep {i}: host scipy with spacing {t_host[-1]:.3f} s", flush=True)
    doc = {"what": "Dice / HD95 of classes 1..8 of one synthetic label volume against a displaced copy, the metric alone, seconds: host = "
                   "calculate_metric_percase per class with the spacing (scipy, host clock); device_unit = metrics_device without spacing "
                   "(integer kernels); device_fp64 = metrics_device with the spacing (fp64 kernels); device forms from resident volumes to "
                   "results on the host, alternating, host clock",
           "shape": list(shape), "spacing": list(spacing), "classes": 9, "voxels_per_label": np.bincount(label.ravel(), minlength=9).tolist(),
           "device_unit": spread(t_int), "device_fp64": spread(t_f64),
           "fp64_over_unit_median": float(np.median(t_f64) / np.median(t_int)),
           "scratch_bytes": {"unit": metrics_scratch_bytes(shape, 9), "fp64": metrics_scratch_bytes(shape, 9, spacing),
                             "largest_allocation_fp64": 8 * int(np.prod(shape))},
           "result_device_unit": r_int, "result_device_fp64": r_f64, "gpu": torch.cuda.get_device_name(0),
           "provenance": {"source_sha": source_digest()}}
    if t_host:
        diff = np.abs(np.array(r_f64) - np.array(r_host)).max(axis=0)
        doc.update({"host": spread(t_host), "host_over_fp64_median": float(np.median(t_host) / np.median(t_f64)), "result_host": r_host,
                    "max_abs_diff_fp64_vs_host": {"dice": float(diff[0]), "hd95": float(diff[1])}})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({k: doc[k] for k in ("host", "device_unit", "device_fp64", "fp64_over_unit_median", "host_over_fp64_median",
                                           "scratch_bytes", "max_abs_diff_fp64_vs_host") if k in doc}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[148, 512, 512])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--img-size", type=int, default=224)
    ap.add_argument("--out", default=None)
    ap.add_argument("--metric-only", action="store_true")
    ap.add_argument("--spacing", type=float, nargs=3, metavar=("Z", "Y", "X"), default=None,
                    help="voxel size: time the metric alone on the host and on the device with it, beside the unit-spacing device path")
    ap.add_argument("--host-reps", type=int, default=None, help="with --spacing: repetitions of the host metric (default: --reps; 0 skips it)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "metrics_spacing.json" if a.spacing else "metrics_device.json")
    if a.host_reps is None:
        a.host_reps = a.reps
    assert torch.cuda.is_available(), "bench_metrics.py measures on the MI355X"
    from provenance import source_digest
    from transception_amd import MSTransception
    from transception_amd.evaluate import evaluate_volume, metrics_device, metrics_scratch_bytes
    from transception_amd.seeded_init import seeded_state_dict
    dev = "cuda:0"
    shape = tuple(a.shape)
    image, label = synthetic_volume(shape)
    print(f"volume {shape}, voxels per label {np.bincount(label.ravel(), minlength=9).tolist()}", flush=True)

    lab_d = torch.from_numpy(label).to(dev)
    pred_d = torch.roll(lab_d, (2, 5, -4), (0, 1, 2)).contiguous()              # a displaced copy: every class has two different surfaces
    if a.spacing:
        return bench_spacing(a, shape, label, pred_d, lab_d)
    res = metrics_device(pred_d, lab_d, 9)                                      # warm-up
    ev = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = metrics_device(pred_d, lab_d, 9)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3)
    print(f"metrics_device alone (device events): {ev}", flush=True)
    if a.metric_only:
        print(res)
        return

    m = MSTransception(num_classes=9)
    m.load_state_dict(seeded_state_dict(), strict=True)
    m.to(dev).eval()

    def run(device_metrics):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = evaluate_volume(m, image, label, 9, (a.img_size, a.img_size), with_hd95=True, device_metrics=device_metrics)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    t, r_dev = run(True)
    print(f"warm-up device {t:.3f} s", flush=True)
    t, r_host = run(False)
    print(f"warm-up host {t:.3f} s", flush=True)
    diff = np.abs(np.array(r_dev) - np.array(r_host)).max(axis=0)
    print(f"max |device - host|: dice {diff[0]:.3e} hd95 {diff[1]:.3e}", flush=True)
    host, devt = [], []
    for i in range(a.reps):
        host.append(run(False)[0])
        devt.append(run(True)[0])
        print(f"rep {i}: host {host[-1]:.3f} s, device {devt[-1]:.3f} s", flush=True)
    doc = {"what": "evaluate_volume(with_hd95=True) of one synthetic volume, metric on the host (scipy) vs on the device; seconds, host clock "
                   "around a device synchronise; metric_alone = metrics_device on resident label volumes, device events",
           "shape": list(shape), "img_size": a.img_size, "classes": 9, "voxels_per_label": np.bincount(label.ravel(), minlength=9).tolist(),
           "host_metrics": spread(host), "device_metrics": spread(devt), "metric_alone": spread(ev),
           "speedup_slowest_device_vs_fastest_host": min(host) / max(devt), "accepted": max(devt) < min(host),
           "max_abs_diff": {"dice": float(diff[0]), "hd95": float(diff[1])}, "result_device": r_dev,
           "scratch_bytes": metrics_scratch_bytes(shape, 9), "gpu": torch.cuda.get_device_name(0),
           "provenance": {"source_sha": source_digest()}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({k: doc[k] for k in ("host_metrics", "device_metrics", "metric_alone", "speedup_slowest_device_vs_fastest_host", "accepted")}))


if __name__ == "__main__":
    main()

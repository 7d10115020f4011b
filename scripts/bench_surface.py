"""What the surface metrics (ASD, ASSD, surface Dice, full Hausdorff) cost beside Dice and HD95, on one volume.

    python scripts/bench_surface.py [--shape 148 512 512] [--reps 5] [--host-reps 1] [--spacing Z Y X] [--out profiles/surface_metrics.json]

The synthetic label volume of scripts/bench_metrics.py (8 organs of realistic extent at Synapse test size) against a displaced copy, both
resident on the device.  Three measurements, each after a warm-up, medians of the repetitions:
  * `metrics_device` and `surface_metrics_device`, alternating in one run, under device events around a call that ends in the copy of the
    results to the host: the difference is what the extra pass costs;
  * the statistics launch alone (tc_surface_stats, or tc_surface_stats_f64 with --spacing) per class on that class's resident maps, under
    device events, with the bytes it has to read -- the two uint8 maps and one distance per surface voxel -- and the rate that makes;
  * `surface_metrics_host` (scipy), host clock; --host-reps 0 skips it, and the json then says "not measured".
Every repetition, the shape and the source hash go into the json."""
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

from bench_metrics import spread, synthetic_volume  # noqa: E402


def timed(fn):
    """Seconds of `fn()` between two device events, and its result."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[148, 512, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--tolerance", type=float, default=2.0)
    ap.add_argument("--spacing", type=float, nargs=3, metavar=("Z", "Y", "X"), default=None, help="voxel size: the fp64 kernels")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_surface.py measures on the MI355X"
    from provenance import source_digest
    from transception_amd._lib import TC_SURFACE_WORK_BYTES, lib
    from transception_amd.evaluate import (SurfaceMetrics, edt_squared, metrics_device, metrics_scratch_bytes, surface_metrics_device,
                                           surface_metrics_host, surfaces_counts)
    dev, shape, classes = "cuda:0", tuple(a.shape), 9
    spacing = tuple(a.spacing) if a.spacing else None
    surface = SurfaceMetrics(a.tolerance)
    _, label = synthetic_volume(shape)
    lab_d = torch.from_numpy(label).to(dev)
    pred_d = torch.roll(lab_d, (2, 5, -4), (0, 1, 2)).contiguous()              # a displaced copy: every class has two different surfaces
    n = int(np.prod(shape))
    print(f"volume {shape}, voxels per label {np.bincount(label.ravel(), minlength=classes).tolist()}", flush=True)

    # 1. the whole metric, without and with the surface statistics
    metrics_device(pred_d, lab_d, classes, spacing), surface_metrics_device(pred_d, lab_d, classes, spacing, surface)        # warm-up
    t_plain, t_surface = [], []
    for i in range(a.reps):
        t, plain = timed(lambda: metrics_device(pred_d, lab_d, classes, spacing))
        t_plain.append(t)
        t, report = timed(lambda: surface_metrics_device(pred_d, lab_d, classes, spacing, surface))
        t_surface.append(t)
        print(f"rep {i}: metrics_device {t_plain[-1]:.4f} s, surface_metrics_device {t_surface[-1]:.4f} s", flush=True)
    assert [(d["dice"], d["hd95"]) for d in report] == plain

    # 2. the statistics launch alone, per class
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    entry = L.tc_surface_stats_f64 if spacing else L.tc_surface_stats
    sp, sg, _ = surfaces_counts(pred_d, lab_d, classes)
    work = torch.empty(TC_SURFACE_WORK_BYTES // 8, dtype=torch.int64, device=dev)
    out = torch.zeros((classes, 2, 4), dtype=torch.int64, device=dev)
    per_class = []
    for k in range(1, classes):
        dp, dg = edt_squared(sp, k, voxelspacing=spacing), edt_squared(sg, k, voxelspacing=spacing)

        def launch():
            entry(sp.data_ptr(), sg.data_ptr(), dp.data_ptr(), dg.data_ptr(), k, classes, *shape, a.tolerance ** 2, work.data_ptr(), out.data_ptr(), stream)

        launch()
        ts = [timed(launch)[0] for _ in range(max(a.reps, 5))]
        members = int(out[k, 0, 0]) + int(out[k, 1, 0])
        nbytes = 2 * n + dp.element_size() * members
        med = float(np.median(ts))
        per_class.append({"class": k, "surface_voxels": members, "bytes": nbytes, **spread(ts), "TB_per_s": nbytes / med * 1e-12})
        print(f"class {k}: {members} surface voxels, {nbytes} bytes, median {med * 1e6:.1f} us, {nbytes / med * 1e-12:.3f} TB/s", flush=True)

    # 3. the host
    t_host, host_report = [], None
    pred = pred_d.cpu().numpy()
    for i in range(a.host_reps):
        t0 = time.perf_counter()
        host_report = surface_metrics_host(pred, label, classes, spacing, surface)
        t_host.append(time.perf_counter() - t0)
        print(f"rep {i}: surface_metrics_host {t_host[-1]:.2f} s", flush=True)

    extra = float(np.median(t_surface) - np.median(t_plain))
    doc = {"what": "one synthetic label volume against a displaced copy, classes 1..8, seconds.  metrics_device / surface_metrics_device: from "
                   "resident volumes to the results on the host, alternating, device events; stats_launch: tc_surface_stats"
                   + ("_f64" if spacing else "") + " alone per class on resident maps (both launches of the entry), device events, bytes = the two "
                   "uint8 maps + one distance per surface voxel; host: surface_metrics_host (scipy), host clock",
           "shape": list(shape), "classes": classes, "spacing": list(spacing) if spacing else None, "nsd_tolerance": a.tolerance,
           "metrics_device": spread(t_plain), "surface_metrics_device": spread(t_surface), "extra_median_s": extra,
           "extra_over_metrics_device": extra / float(np.median(t_plain)), "stats_launch": per_class,
           "stats_launch_sum_of_medians_s": float(sum(c["median_s"] for c in per_class)),
           "host": spread(t_host) if t_host else "not measured",
           "host_over_device_median": float(np.median(t_host) / np.median(t_surface)) if t_host else "not measured",
           "scratch_bytes": {"metrics_device": metrics_scratch_bytes(shape, classes, spacing), "surface_extra": TC_SURFACE_WORK_BYTES + 8 * classes * 2 * 4},
           "result_device": report, "gpu": torch.cuda.get_device_name(0), "provenance": {"source_sha": source_digest()}}
    if host_report is not None:
        doc["max_abs_diff_device_vs_host"] = {key: max(abs(d[key] - h[key]) for d, h in zip(report, host_report)) for key in report[0] if key != "defined"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({k: doc[k] for k in ("metrics_device", "surface_metrics_device", "extra_median_s", "extra_over_metrics_device",
                                           "stats_launch_sum_of_medians_s", "host", "host_over_device_median", "max_abs_diff_device_vs_host") if k in doc}))


if __name__ == "__main__":
    main()

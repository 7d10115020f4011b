"""Connected-component post-processing of one predicted label volume on the device (evaluate.postprocess_device) against the host path a
user had before: copy the prediction to the host, evaluate.postprocess_host (scipy.ndimage.label per class), copy the result back.

    python scripts/bench_postprocess.py [--shape 148 512 512] [--reps 10] [--host-reps 2] [--islands 0.01] [--out profiles/postprocess_device.json]

One seeded synthetic 9-class volume of Synapse test size (the organs of bench_metrics.py) plus `--islands` of its voxels turned into
random island voxels of random classes, resident in HBM.  For both modes ("largest", "min_voxels" with N = 10) and both connectivities:
after one warm-up of every configuration one whole `postprocess_device` call -- four allocations from torch's caching allocator, three
C entries, seven launches and two memsets -- runs `reps` times between two device events, the configurations alternating: an end-to-end
figure of the call, which at a millisecond may hold as much of the host's launch rate as of the kernels' time, not a kernel time; the host
path runs `host-reps` times under a host clock that starts after a device synchronise and ends after the upload's synchronise.  The two
results are compared voxel by voxel.  No threshold: every repetition, the medians, their ratio, the component counts and the source hash
go into the json."""
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


def spread(ts):
    return {"runs_s": ts, "min_s": min(ts), "max_s": max(ts), "median_s": float(np.median(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[148, 512, 512])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=2, help="repetitions of the host path (0 skips it and the comparison)")
    ap.add_argument("--islands", type=float, default=0.01, help="fraction of voxels turned into random island voxels")
    ap.add_argument("--min-voxels", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postprocess_device.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_postprocess.py measures on the MI355X"
    from bench_metrics import synthetic_volume
    from provenance import source_digest
    from transception_amd.evaluate import PostProcess, component_roots, postprocess_device, postprocess_host, postprocess_scratch_bytes
    dev = "cuda:0"
    shape = tuple(a.shape)
    _, label = synthetic_volume(shape)
    g = np.random.default_rng(1)
    islands = g.random(shape) < a.islands
    label[islands] = g.integers(1, 9, int(islands.sum()))
    print(f"volume {shape}, voxels per label {np.bincount(label.ravel(), minlength=9).tolist()}", flush=True)
    pred_d = torch.from_numpy(label).to(dev)
    out_d = torch.empty_like(pred_d)

    configs = [PostProcess("largest", 0, c) for c in (1, 3)] + [PostProcess("min_voxels", a.min_voxels, c) for c in (1, 3)]
    names = [f"{p.mode}/connectivity{p.connectivity}" for p in configs]
    components = {}
    for c in (1, 3):
        root = component_roots(pred_d, 9, c)
        components[f"connectivity{c}"] = int((root == torch.arange(root.numel(), device=dev, dtype=torch.int32).view(shape)).sum())
        del root
    for p in configs:                                                           # warm-up of every configuration
        postprocess_device(pred_d, 9, p, out=out_d)
    torch.cuda.synchronize()
    t_dev = {n: [] for n in names}
    for i in range(a.reps):
        for n, p in zip(names, configs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            postprocess_device(pred_d, 9, p, out=out_d)
            e1.record()
            e1.synchronize()
            t_dev[n].append(e0.elapsed_time(e1) * 1e-3)
        print(f"rep {i}: device " + ", ".join(f"{n} {t_dev[n][-1] * 1e3:.2f} ms" for n in names), flush=True)

    t_host, t_label, equal = {n: [] for n in names}, {n: [] for n in names}, {}
    for i in range(a.host_reps):
        for n, p in zip(names, configs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h = pred_d.cpu().numpy()
            t1 = time.perf_counter()
            r = postprocess_host(h, 9, p)
            t2 = time.perf_counter()
            back = torch.from_numpy(r).to(dev)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            t_host[n].append(t3 - t0)
            t_label[n].append(t2 - t1)
            equal[n] = bool(torch.equal(back, postprocess_device(pred_d, 9, p)))
            print(f"rep {i}: host {n} {t3 - t0:.3f} s (scipy part {t2 - t1:.3f} s), device result equal: {equal[n]}", flush=True)

    doc = {"what": "connected-component post-processing of one synthetic 9-class label volume resident in HBM, seconds: device = "
                   "one whole evaluate.postprocess_device call into a preallocated output, end to end (allocations, seven launches, two memsets "
                   "between two device events; configurations alternating, after warm-up; not a kernel time); host = "
                   "copy to the host + evaluate.postprocess_host (scipy.ndimage.label per class) + copy back (host clock between device "
                   "synchronises); host_scipy_part = postprocess_host alone",
           "shape": list(shape), "classes": 9, "island_fraction": a.islands, "min_voxels": a.min_voxels,
           "voxels_per_label": np.bincount(label.ravel(), minlength=9).tolist(), "components": components,
           "scratch_bytes": postprocess_scratch_bytes(shape), "device": {n: spread(t_dev[n]) for n in names},
           "gpu": torch.cuda.get_device_name(0), "provenance": {"source_sha": source_digest()}}
    if a.host_reps:
        doc.update({"host": {n: spread(t_host[n]) for n in names}, "host_scipy_part": {n: spread(t_label[n]) for n in names},
                    "host_over_device_median": {n: float(np.median(t_host[n]) / np.median(t_dev[n])) for n in names},
                    "device_equals_host": equal})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({"device_median_ms": {n: 1e3 * doc["device"][n]["median_s"] for n in names},
                      "host_median_s": {n: doc["host"][n]["median_s"] for n in names} if a.host_reps else None,
                      "host_over_device_median": doc.get("host_over_device_median"), "device_equals_host": doc.get("device_equals_host"),
                      "components": components}))


if __name__ == "__main__":
    main()

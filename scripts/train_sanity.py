"""A few hundred captured training steps on the synthetic Synapse set (bf16 storage, loader-fed, the default kernels incl. the
hand-scheduled attention stream): the loss must fall and stay finite.  python scripts/train_sanity.py [steps] [--loss-scale {N,dynamic}]
--loss-scale switches to float16 storage: N is a static scale, `dynamic` a train.DynamicLossScale whose value each log line shows."""
import argparse, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from transception_amd import MSTransception, data as D
from transception_amd.seeded_init import seeded_state_dict
from transception_amd.train import DynamicLossScale, FusedSGD, GraphedStep, SegLoss, cosine_lr
ap = argparse.ArgumentParser()
ap.add_argument("steps", nargs="?", type=int, default=300)
ap.add_argument("--loss-scale", default=None, metavar="{N,dynamic}", help="float16 storage with a static scale N or a dynamic one")
args = ap.parse_args()
steps = args.steps
scale = None if args.loss_scale is None else DynamicLossScale() if args.loss_scale == "dynamic" else float(args.loss_scale)
dyn = isinstance(scale, DynamicLossScale)
dev = torch.device("cuda:0")
tmp = tempfile.mkdtemp()
D.write_synthetic_synapse(tmp + "/a", tmp + "/l", n_cases=4, slices_per_case=32, size=512, seed=1)
ds = D.SynapseSlices(tmp + "/a", tmp + "/l")
model = MSTransception(num_classes=9); model.load_state_dict(seeded_state_dict(), strict=True); model.to(dev).train()
model.set_compute_dtype(torch.bfloat16 if scale is None else torch.float16); model._ensure_flat(dev)
loss_fn, opt = SegLoss(9, loss_scale=1.0 if scale is None else scale), FusedSGD(model, lr=0.05, momentum=0.9, weight_decay=1e-4)
loader = D.DeviceLoader(ds, 16, device=dev, epochs=steps * 16 // len(ds) + 2, readers=8)
x0 = torch.zeros(16, 1, 224, 224, device=dev); y0 = torch.zeros(16, 224, 224, dtype=torch.int64, device=dev)
fed, hist = {}, []
t0 = time.perf_counter()
for i, slot in enumerate(loader.iter_raw()):
    if i == steps:
        break
    st = fed.get(slot["index"])
    if st is None:
        st = fed[slot["index"]] = GraphedStep(model, loss_fn, opt, x0, y0, None, warmup=1, pre=loader.slot_preprocess(slot))
    loss, ce, dice = st()
    opt.set_lr(cosine_lr(0.05, i + 1, steps))
    if i % 25 == 0 or i == steps - 1:
        hist.append((i, float(loss), float(ce), float(dice)))
        print(f"step {i:4d} loss {hist[-1][1]:.4f} ce {hist[-1][2]:.4f} dice {hist[-1][3]:.4f}"
              + (f" loss scale {scale.value():g} ({scale.skipped()} skipped)" if dyn else ""), flush=True)
torch.cuda.synchronize()
print(f"{steps} steps in {time.perf_counter() - t0:.1f} s; finite: {all(map(lambda h: h[1] == h[1] and abs(h[1]) < 1e4, hist))}; "
      f"loss {hist[0][1]:.4f} -> {hist[-1][1]:.4f}")
assert hist[-1][1] < 0.8 * hist[0][1]

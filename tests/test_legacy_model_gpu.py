"""The legacy Transception network on the MI355X against the reference's own outputs (tests/golden/legacy.npz): a train step per
constructor configuration, module cases (dilated patch embedding, fused block, stage fuse), bf16 storage, the captured step and the
evaluation path."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import check_packed, load  # noqa: E402
from transception_amd.seeded_init import schema_entries, seeded_input, seeded_labels, seeded_state_dict, seeded_tensor  # noqa: E402

DEV = "cuda:0"
CONFIGS = {"default": {}, "sk": dict(concat="sk"), "nodil": dict(dil_conv=0), "heads8": dict(head_count=8), "mix": dict(token_mlp_mode="mix")}
GRAD_TOL = dict(atol=2e-6, rtol=2e-3, sum_rtol=1e-3)


@pytest.fixture(scope="module")
def gold():
    return load("legacy.npz")


def _fresh(dtype=torch.float32, **kw):
    from transception_amd import Transception
    m = Transception(num_classes=9, **kw)
    m.load_state_dict(seeded_state_dict(schema_entries(m)), strict=True)
    return m.to(DEV).set_compute_dtype(dtype)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_train_step_vs_reference_golden(gold, cfg):
    from transception_amd.train import SegLoss
    m = _fresh(**CONFIGS[cfg]).train()
    x = torch.from_numpy(seeded_input(1)).to(DEV)
    lab = torch.from_numpy(seeded_labels(1)).to(DEV)
    logits = m(x)
    check_packed(gold, cfg + "/logits", logits.detach().cpu(), atol=1e-4)
    loss, ce, dice = SegLoss(9)(logits, lab)
    np.testing.assert_allclose([loss.item(), ce.item(), dice.item()], gold[cfg + "/loss"], rtol=0, atol=2e-5)
    loss.backward()
    named = dict(m.named_parameters())
    assert sum(1 for p in m.parameters() if p.grad is not None) == int(gold[cfg + "/n_live"][0])
    probes = [k[len(cfg) + 6:-6] for k in gold.files if k.startswith(cfg + "/grad/") and k.endswith("/shape")]
    assert len(probes) == 6
    for key in probes:
        check_packed(gold, cfg + "/grad/" + key, named[key].grad.cpu(), **GRAD_TOL)
    bufs = dict(m.named_buffers())
    for key in [k[len(cfg) + 4:-6] for k in gold.files if k.startswith(cfg + "/bn/") and k.endswith("/shape")]:
        check_packed(gold, cfg + "/bn/" + key, bufs[key].cpu(), atol=1e-5, rtol=1e-4)
    m2 = _fresh(**CONFIGS[cfg]).eval()
    with torch.no_grad():
        check_packed(gold, cfg + "/logits_eval", m2(x).cpu(), atol=1e-4)


def _tok(x):
    B, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(B * H * W, C)


def _case(gold, tag, m, shape, to_in, fn, from_out, to_gout):
    """Module case `tag` of legacy.npz through the engine in fp32: output, input gradient, every weight gradient the module touched."""
    from transception_amd.engine import Graph, Var
    m._ensure_flat(torch.device(DEV))
    m._used_views = {}
    m._gflat.zero_()
    G = Graph(torch.float32, torch.device(DEV), training=True, record=True)
    x = torch.from_numpy(seeded_tensor(f"legacy/{tag}/x0", shape))
    xv = Var(to_in(x).to(DEV).contiguous())
    out = fn(G, xv)
    y = from_out(out.data.cpu())
    check_packed(gold, f"mod/{tag}/y", y, atol=1e-4)
    g = torch.from_numpy(seeded_tensor(f"legacy/{tag}/g", tuple(y.shape)))
    r = out.root
    assert out.is_whole
    r.grad_t, r.whole_written = to_gout(g).to(DEV).contiguous().view(r.rows, r.cols), True
    G.backward()
    torch.cuda.synchronize()
    check_packed(gold, f"mod/{tag}/gx0", from_out_in(G.grad_of(xv).cpu(), x.shape, to_in), atol=1e-4, sum_rtol=1e-3)
    keys = [k[len(tag) + 8:-6] for k in gold.files if k.startswith(f"mod/{tag}/gw/") and k.endswith("/shape")]
    assert keys
    for k in keys:
        off, shp = m._index[k]
        gw = m._gflat[off:off + math.prod(shp)].view(shp).cpu()
        scale = float(np.abs(gold[f"mod/{tag}/gw/{k}/samples"]).max())
        check_packed(gold, f"mod/{tag}/gw/{k}", gw, atol=2e-6 + 1e-5 * scale, rtol=2e-3, sum_rtol=1e-3)


def from_out_in(gx, shape, to_in):
    """The gradient of the engine's input layout back in the reference's input layout."""
    if len(shape) == 4:
        B, C, H, W = shape
        return gx.view(B, H, W, C).permute(0, 3, 1, 2)
    return gx.view(*shape) if to_in is _tok3 else _branch_to_image(gx, shape)


def _tok3(t):
    return t.reshape(-1, t.shape[-1])


N1 = {1460: 676, 340: 144}


def _image_to_branch(t):
    """[B, n1+n2, C] (the reference's per-image sequence) -> branch-major rows [B*n1 | B*n2, C] (the engine's layout)."""
    B, n, C = t.shape
    n1 = N1[n]
    return torch.cat([t[:, :n1].reshape(-1, C), t[:, n1:].reshape(-1, C)])


def _branch_to_image(t, shape):
    B, n, C = shape
    n1 = N1[n]
    return torch.cat([t[:B * n1].view(B, n1, C), t[B * n1:].view(B, n - n1, C)], 1)


def test_module_cases_vs_reference_golden(gold):
    import transception_amd.legacy as LG
    B = 2
    m = _fresh().train()
    run = lambda *a: _case(gold, *a)
    run("patch_embed2_1", m, (B, 64, 56, 56), _tok,
        lambda G, x: _pe(G, m, x, B), lambda o: o.view(B, 676, 128), lambda g: g.reshape(B * 676, 128))
    run("block2_0", m, (B, 1460, 128), _image_to_branch,
        lambda G, x: LG._fuse_block(m, G, x, "backbone.block2.0", B, 26, 28), lambda o: _branch_to_image(o, (B, 1460, 128)), _image_to_branch)
    fuse = lambda mm, G, x: (G.linear(G.nearest_concat(x, B, 12, 12, 14, 14), *LG._lin(mm, G, "backbone.conv1_1_s3")) if mm.concat == "original"
                             else LG._sk_block(mm, G, G.nearest_concat(x, B, 12, 12, 14, 14), "backbone.sk_concat3", B, 196, 320))
    nchw = lambda o: o.view(B, 14, 14, 320).permute(0, 3, 1, 2)
    run("fuse3_conv", m, (B, 340, 320), _image_to_branch, lambda G, x: fuse(m, G, x), nchw, _tok)
    msk = _fresh(concat="sk").train()
    run("fuse3_sk", msk, (B, 340, 320), _image_to_branch, lambda G, x: fuse(msk, G, x), nchw, _tok)


def _pe(G, m, x, B):
    import transception_amd.legacy as LG
    out = G.new(B * 676, 128)
    LG._patch_embed(m, G, x, "backbone.patch_embed2_1", B, 56, (3, 2, 0, 2), out)
    return out


def test_bf16_step_tracks_fp32():
    from transception_amd.train import SegLoss
    x = torch.from_numpy(seeded_input(1)).to(DEV)
    lab = torch.from_numpy(seeded_labels(1)).to(DEV)
    with torch.no_grad():
        l32 = _fresh().train()(x).cpu()
    mb = _fresh(torch.bfloat16).train()
    lb = mb(x)
    d = float((lb.detach().cpu() - l32).abs().max())
    print(f"bf16 vs fp32 max |dlogit| = {d:.4f}")
    assert d <= 0.17, d
    SegLoss(9)(lb, lab)[0].backward()
    assert all(torch.isfinite(p.grad).all() for p in mb.parameters() if p.grad is not None)


def test_graphed_bf16_step_tracks_eager():
    from transception_amd.train import FusedSGD, GraphedStep, SegLoss, train_step
    x = torch.from_numpy(seeded_input(2)).to(DEV)
    lab = torch.from_numpy(seeded_labels(2)).to(DEV)
    me, mg = _fresh(torch.bfloat16).train(), _fresh(torch.bfloat16).train()
    oe, og = FusedSGD(me, lr=0.05), FusedSGD(mg, lr=0.05)
    le, lg = SegLoss(9), SegLoss(9)
    for _ in range(2):
        train_step(me, le, oe, x, lab)
    step = GraphedStep(mg, lg, og, x, lab, None, warmup=2)
    for _ in range(5):
        a = train_step(me, le, oe, x, lab)[0].item()
        b = step()[0].item()
        assert abs(a - b) < 5e-3, (a, b)
    assert torch.isfinite(mg.flat_gradients()).all()


def test_evaluate_volume_is_argmax_of_forward():
    from transception_amd.evaluate import dice_from_counts, evaluate_volume
    m = _fresh().eval()
    g = torch.Generator().manual_seed(3)
    vol = torch.rand(3, 224, 224, generator=g)
    with torch.no_grad():
        pred = m(((vol - 0.5) / 0.5).unsqueeze(1).to(DEV)).argmax(1).cpu().numpy()
    label = torch.randint(0, 9, (3, 224, 224), generator=g).numpy()
    label[:, :112] = pred[:, :112]                               # half of each slice agrees: non-trivial Dice values
    counts = np.zeros((9, 3))
    for k in range(9):
        p, t = pred == k, label == k
        counts[k] = (np.logical_and(p, t).sum(), p.sum(), t.sum())
    assert evaluate_volume(m, vol.numpy(), label, classes=9, batch=2) == dice_from_counts(counts)

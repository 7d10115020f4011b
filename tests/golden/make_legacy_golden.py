"""Generates tests/golden/legacy.npz from the imported reference's legacy network (build container only).

    python tests/golden/make_legacy_golden.py

networks/Transception.py::Transception, run on CPU in fp32 with the name-seeded weights of transception_amd/seeded_init.py loaded
strict=True (the schema is derived from the reference module itself, schema_entries).  Same `pack` conventions as make_golden.py
(shape, samples at seeded positions, float64 checksums).  Contents:

  <cfg>/schema_sha256, <cfg>/n_keys, <cfg>/keys   state_dict schema of each constructor configuration (CONFIGS)
  <cfg>/logits, <cfg>/loss, <cfg>/n_live          B=1 train-mode step: logits, [loss, ce, dice] (0.4 CE + 0.6 Dice), live gradient count
  <cfg>/grad/<name>                               gradient probes (PROBES)
  <cfg>/bn/<name>                                 BatchNorm running statistics after the step (SK configurations)
  <cfg>/logits_eval                               eval-mode logits of a fresh model with the same weights
  mod/<case>/y, gx0, gw/<name>                    module cases at B=2 with seeded inputs and upstream gradients (MODULES)
  init/keys, init/sums                            per-key float64 sums of the state_dict right after torch.manual_seed(1234); Transception()

Fixtures hold data only, never reference source.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from ref_shim import import_reference  # noqa: E402
from make_golden import pack  # noqa: E402
from transception_amd.seeded_init import seeded_input, seeded_labels, seeded_state_dict, seeded_tensor, schema_entries, schema_digest  # noqa: E402

CONFIGS = {
    "default": {},
    "sk": dict(concat="sk"),
    "nodil": dict(dil_conv=0),
    "heads8": dict(head_count=8),
    "mix": dict(token_mlp_mode="mix"),
}
PROBES = ["backbone.patch_embed2_1.proj.weight", "backbone.block2.0.attn.keys.weight", "backbone.block3.1.mlp1.fc1.weight",
          "backbone.block4.0.norm2.weight", "decoder_0.last_layer.weight"]
SK_BN = [f"backbone.sk_concat{s}.conv_bn_ac.2.running_{w}" for s in (2, 3, 4) for w in ("mean", "var")]


def _text(s: str) -> np.ndarray:
    return np.frombuffer(s.encode(), dtype=np.uint8)


def _fuse(concat_mod, seq, n1, g1, g2, sk):
    """Stage fuse of MiT_3inception.forward (Transception.py:461-476): split, maps, nearest resize of branch 1, conv1_1_sK or SK_Block."""
    b = seq.shape[0]
    m1 = seq[:, :n1].reshape(b, g1, g1, -1).permute(0, 3, 1, 2)
    m2 = seq[:, n1:].reshape(b, g2, g2, -1).permute(0, 3, 1, 2)
    m1 = F.interpolate(m1, [g2, g2])
    return concat_mod([m1, m2]) if sk else concat_mod(torch.cat((m1, m2), 1))


def config(out, RefT, Dice, name, kw):
    x = torch.from_numpy(seeded_input(1))
    y_lab = torch.from_numpy(seeded_labels(1))
    ref = RefT(num_classes=9, **kw)
    entries = schema_entries(ref)
    out[name + "/schema_sha256"] = _text(schema_digest(entries))
    out[name + "/n_keys"] = np.array([len(entries), len({c for _, _, c in entries})], dtype=np.int64)
    out[name + "/keys"] = _text("\n".join(k for k, _, _ in entries))
    sd = seeded_state_dict(entries)
    ref.load_state_dict(sd, strict=True)
    ref.train()
    logits = ref(x)
    pack(out, name + "/logits", logits)
    ce = F.cross_entropy(logits, y_lab)
    dice = Dice(9)(logits, y_lab, softmax=True)
    loss = 0.4 * ce + 0.6 * dice
    loss.backward()
    out[name + "/loss"] = np.array([loss.item(), ce.item(), dice.item()], dtype=np.float64)
    named = dict(ref.named_parameters())
    live = sorted(n for n, p in named.items() if p.grad is not None)
    out[name + "/n_live"] = np.array([len(live)], dtype=np.int64)
    sk = kw.get("concat", "original") != "original"
    for n in PROBES + (["backbone.sk_concat4.fc.weight"] if sk else ["backbone.conv1_1_s3.weight"]):
        pack(out, name + "/grad/" + n, named[n].grad)
    if sk:
        bufs = dict(ref.named_buffers())
        for n in SK_BN:
            pack(out, name + "/bn/" + n, bufs[n])
    ref2 = RefT(num_classes=9, **kw)
    ref2.load_state_dict(sd, strict=True)
    ref2.eval()
    with torch.no_grad():
        pack(out, name + "/logits_eval", ref2(x))
    print(name, "keys", len(entries), "live grads", len(live), "loss", loss.item())


def modules(out, RefT):
    """y = m(x); gx0 = d(sum(y*g))/dx, gw/<name> = d(sum(y*g))/dw for every parameter the module touched (B=2, train mode)."""
    B = 2
    refs = {}
    for cname, kw in (("default", {}), ("sk", dict(concat="sk"))):
        r = RefT(num_classes=9, **kw)
        r.load_state_dict(seeded_state_dict(schema_entries(r)), strict=True)
        r.train()
        refs[cname] = r

    def run(tag, ref, fn, shape):
        xin = torch.from_numpy(seeded_tensor(f"legacy/{tag}/x0", shape)).requires_grad_(True)
        ref.zero_grad(set_to_none=True)
        y = fn(xin)
        g = torch.from_numpy(seeded_tensor(f"legacy/{tag}/g", tuple(y.shape)))
        (y * g).sum().backward()
        pack(out, f"mod/{tag}/y", y)
        pack(out, f"mod/{tag}/gx0", xin.grad)
        nw = 0
        for n, p in ref.named_parameters():
            if p.grad is not None:
                pack(out, f"mod/{tag}/gw/{n}", p.grad)
                nw += 1
        print(tag, tuple(y.shape), f"{nw} weight gradients")

    bd, bs = refs["default"].backbone, refs["sk"].backbone
    run("patch_embed2_1", refs["default"], lambda x: bd.patch_embed2_1(x)[0], (B, 64, 56, 56))
    run("block2_0", refs["default"], lambda x: bd.block2[0](x, 676, 784, 26, 26, 28, 28), (B, 676 + 784, 128))
    run("fuse3_conv", refs["default"], lambda x: _fuse(bd.conv1_1_s3, x, 144, 12, 14, False), (B, 144 + 196, 320))
    run("fuse3_sk", refs["sk"], lambda x: _fuse(bs.sk_concat3, x, 144, 12, 14, True), (B, 144 + 196, 320))


def init_sums(out, RefT):
    torch.manual_seed(1234)
    ref = RefT()
    sd = ref.state_dict()
    out["init/keys"] = _text("\n".join(sd))
    out["init/sums"] = np.array([float(t.double().sum()) for t in sd.values()], dtype=np.float64)


if __name__ == "__main__":
    torch.set_num_threads(8)
    _, Dice = import_reference()
    from networks.Transception import Transception as RefT  # noqa: E402
    res = {}
    init_sums(res, RefT)
    for name, kw in CONFIGS.items():
        config(res, RefT, Dice, name, kw)
    modules(res, RefT)
    path = os.path.join(HERE, "legacy.npz")
    np.savez_compressed(path, **res)
    print(path, os.path.getsize(path))

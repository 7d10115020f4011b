"""Host side of the fused Adam / AdamW (train.FusedAdamW, tc_adam_advance, tc_adam_step_multi): the float64 closed form of
tests/adam_ref.py against torch.optim, the segment construction, TrainConfig's validation and the exported symbols.  No GPU."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from adam_ref import adam_ref, bias_terms

BETAS, WD, LR, EPS = (0.9, 0.999), 0.05, 1e-3, 1e-8


# ---------------------------------------------------------------------------------------------------------------- the closed form
@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam"])
def test_closed_form_is_torch_optim(decoupled):
    """Five float64 steps of torch.optim.AdamW / torch.optim.Adam on 1000 elements against five applications of adam_ref with the
    exact double betas and bias terms: parameters and both moments within 1e-14."""
    g = torch.Generator().manual_seed(3)
    w0 = torch.randn(1000, generator=g, dtype=torch.float64)
    p = torch.nn.Parameter(w0.clone())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    w, m, v = w0.numpy().copy(), np.zeros(1000), np.zeros(1000)
    worst = 0.0
    for t in range(1, 6):
        grad = torch.randn(1000, generator=g, dtype=torch.float64)
        p.grad = grad.clone()
        opt.step()
        bc1, bc2 = 1.0 - BETAS[0] ** t, math.sqrt(1.0 - BETAS[1] ** t)
        w, m, v, Am, Av, den = adam_ref(w, grad.numpy(), m, v, LR, BETAS[0], 1.0 - BETAS[0], BETAS[1], 1.0 - BETAS[1], EPS, WD, bc1, bc2, decoupled)
        st = opt.state[p]
        worst = max(worst, float(np.abs(p.detach().numpy() - w).max()))
        assert np.abs(p.detach().numpy() - w).max() <= 1e-14, (t, worst)
        assert np.abs(st["exp_avg"].numpy() - m).max() <= 1e-14 and np.abs(st["exp_avg_sq"].numpy() - v).max() <= 1e-14
        # the magnitudes the GPU bounds are stated in dominate what they bound
        assert bool((Am >= np.abs(m) * (1 - 1e-12)).all()) and bool((Av >= v * (1 - 1e-12)).all()) and bool((den > 0).all())
    print(f"adam_ref vs torch.optim.{cls.__name__}: worst parameter difference {worst:.2e}")


def test_bias_terms_are_the_float32_roundings():
    for t in (1, 2, 1000):
        bc1, bc2 = bias_terms(*BETAS, t)
        assert bc1 == float(np.float32(1.0 - 0.9 ** t)) and bc2 == float(np.float32(math.sqrt(1.0 - 0.999 ** t)))


# ---------------------------------------------------------------------------------------------------------------- segments
def _views(seed=0, n=60):
    """(name, offset, shape) of fake parameters laid out like the model's arena (every tensor padded to 8 elements), with holes where
    grad-less tensors sit, matrices and vectors mixed so that decay classes change inside contiguous runs."""
    rng = np.random.default_rng(seed)
    out, off = [], 0
    for i in range(n):
        shape = [(int(rng.integers(1, 40)),), (int(rng.integers(1, 9)), int(rng.integers(1, 30))), (3, 3, int(rng.integers(1, 12)), 2)][int(rng.integers(0, 3))]
        numel = math.prod(shape)
        if rng.random() > 0.25:                                    # (a quarter of the tensors receive no gradient: a hole)
            out.append((f"p{i}." + ("bias" if len(shape) == 1 else "weight"), off, shape))
        off += (numel + 7) // 8 * 8
    return out, off


def _sgd_table_as_it_always_was(views):
    """FusedSGD._segs's algorithm restated: pad to 8, merge adjacent views."""
    segs = []
    for off, n in sorted((off, math.prod(shape)) for _, off, shape in views):
        n8 = (n + 7) // 8 * 8
        if segs and segs[-1][0] + segs[-1][1] == off:
            segs[-1][1] += n8
        else:
            segs.append([off, n8])
    return [(o, n) for o, n in segs]


def _fake_model(views):
    return types.SimpleNamespace(_used_views={i: (off, shape) for i, (_, off, shape) in enumerate(views)},
                                 _pid={name: i for i, (name, _, _) in enumerate(views)})


def _covered(segs):
    s = set()
    for seg in segs:
        s.update(range(seg[0], seg[0] + seg[1]))
    return s


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_segments_without_a_predicate_are_the_sgd_table(seed):
    from transception_amd.train import FusedAdamW, FusedSGD, build_segments
    views, _ = _views(seed)
    want = _sgd_table_as_it_always_was(views)
    assert len(want) > 3
    pure = build_segments(sorted((off, math.prod(shape), 0.01) for _, off, shape in views))
    assert [(o, n) for o, n, _ in pure] == want and {wd for _, _, wd in pure} == {0.01}
    M = _fake_model(views)
    assert FusedSGD(M)._segs() == want
    opt = FusedAdamW(M)
    assert opt._segs() == want and opt._no_decay is None


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_norm_bias_segments_do_not_mix_classes(seed):
    from transception_amd.train import FusedAdamW
    views, total = _views(seed)
    M = _fake_model(views)
    plain, opt = FusedAdamW(M, weight_decay=0.1)._segs(), FusedAdamW(M, weight_decay=0.1, no_decay="norm_bias")
    segs = opt._segs3()
    assert len(segs) > len(plain)                                   # classes do change inside contiguous runs of this layout
    assert all(o % 8 == 0 and n % 8 == 0 and n > 0 for o, n, _ in segs) and {wd for _, _, wd in segs} == {0.0, 0.1}
    assert all(a[0] + a[1] <= b[0] for a, b in zip(segs, segs[1:]))                         # sorted, disjoint
    assert all(a[0] + a[1] < b[0] or a[2] != b[2] for a, b in zip(segs, segs[1:]))          # merged wherever the class allows
    assert _covered(segs) == _covered(plain)
    cls = np.full(total, -1.0)
    for o, n, wd in segs:
        cls[o:o + n] = wd
    for name, off, shape in views:                                  # every tensor lies in a segment of its own class
        assert set(cls[off:off + math.prod(shape)]) == {0.0 if len(shape) <= 1 else 0.1}, name
    # a predicate of the caller's: by name
    by_name = FusedAdamW(M, weight_decay=0.1, no_decay=lambda name, shape: name.endswith("bias"))._segs3()
    assert by_name == segs                                          # (in this layout the one-dimensional tensors are the biases)
    with pytest.raises(ValueError):
        FusedAdamW(M, no_decay="biases")


def test_fused_adamw_refuses_bad_hyper_parameters():
    from transception_amd.train import FusedAdamW
    M = _fake_model(_views(0)[0])
    for kw in (dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=0.0), dict(weight_decay=-1e-2)):
        with pytest.raises(ValueError):
            FusedAdamW(M, **kw)


# ---------------------------------------------------------------------------------------------------------------- TrainConfig
def test_train_config_validates_the_optimizer_fields():
    from transception_amd.trainer import TrainConfig
    ok = TrainConfig(root_path="r", list_dir="l")
    assert ok.optimizer == "sgd" and ok.weight_decay is None and ok.betas == (0.9, 0.999) and ok.adam_eps == 1e-8 and ok.no_decay is None
    TrainConfig(root_path="r", list_dir="l", optimizer="adamw", weight_decay=0.0, betas=(0.0, 0.5), no_decay="norm_bias")
    TrainConfig(root_path="r", list_dir="l", optimizer="adam", base_lr=1e-3)
    for kw in (dict(optimizer="lamb"), dict(optimizer="AdamW"), dict(optimizer="adamw", betas=(0.9, 1.0)), dict(optimizer="adamw", betas=(-0.1, 0.9)),
               dict(optimizer="adamw", betas=(0.9,)), dict(weight_decay=-1e-4), dict(optimizer="adamw", weight_decay=float("nan")),
               dict(optimizer="adamw", no_decay="bias"), dict(no_decay="norm_bias"), dict(optimizer="adam", adam_eps=0.0)):
        with pytest.raises(ValueError):
            TrainConfig(root_path="r", list_dir="l", **kw)


def test_make_optimizer_follows_the_config():
    from transception_amd.train import FusedAdamW, FusedSGD
    from transception_amd.trainer import TrainConfig, make_optimizer
    M = _fake_model(_views(0)[0])
    sgd = make_optimizer(TrainConfig(root_path="r", list_dir="l", grad_clipping=True), M)
    assert type(sgd) is FusedSGD and (sgd.lr, sgd.momentum, sgd.wd, sgd.clip_norm) == (0.05, 0.9, 1e-4, 5.0)
    a = make_optimizer(TrainConfig(root_path="r", list_dir="l", optimizer="adamw", base_lr=1e-3, no_decay="norm_bias"), M)
    assert type(a) is FusedAdamW and (a.lr, a.wd, a.decoupled, a.clip_norm, a.betas, a.eps) == (1e-3, 1e-2, True, None, (0.9, 0.999), 1e-8)
    assert a._no_decay("x", (7,)) and not a._no_decay("x", (7, 2))
    b = make_optimizer(TrainConfig(root_path="r", list_dir="l", optimizer="adam", weight_decay=0.0, betas=(0.5, 0.9)), M)
    assert (b.decoupled, b.wd, b.betas, b.lr) == (False, 0.0, (0.5, 0.9), 0.05)            # base_lr is not rescaled behind the user's back


# ---------------------------------------------------------------------------------------------------------------- exports
def test_library_exports_the_adam_entries():
    from transception_amd import _lib
    from transception_amd.build import build
    dll = ctypes.CDLL(build(verbose=False))
    for name in ("tc_adam_advance", "tc_adam_step_multi"):
        assert hasattr(dll, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["tc_adam_advance"][2:4] == [ctypes.c_double] * 2 and _lib.SIGNATURES["tc_adam_step_multi"][10:12] == [ctypes.c_double] * 2
    assert dll.tc_abi_version() == 15

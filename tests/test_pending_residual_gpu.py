"""Residual gradients that are pure copies (engine.Graph._defer_residual): where the residual branches that feed a LayerNorm's input would copy
consecutive rows of ONE tensor into that input's gradient, the copies are not made and the LayerNorm backward reads the tensor as its `dres`
rows.  Engine level, tiny maps: t1 = Linear(x0) is a `covered` root of four row groups (8, 4, 4 and 2 rows of 64); tx = LayerNorm(t1); each
group of tx feeds a Linear with that group of t1 as its residual, writing its group of t2 -- the shape of a bridge layer's norm2 + four
MixFFNs.  The kernel sees the same dy, the same x and the same addend values either way (only the addend's address differs), so every
comparison between the path and its module switch (engine._PENDING_RES) is of bit patterns, and the launch counter tells the copies."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from transception_amd import _lib  # noqa: E402
from transception_amd.seeded_init import seeded_tensor  # noqa: E402

DEV = "cuda:0"
GROUPS = [(0, 8), (8, 12), (12, 16), (16, 18)]
ROWS, CD = 18, 64


def _name(dtype):
    return str(dtype).split(".")[-1]


def vals(tag, shape, dtype, scale=1.0):
    return torch.from_numpy(seeded_tensor("pending/" + tag, shape, scale)).to(dtype).to(DEV)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))


def mkP(t):
    from transception_amd.engine import P
    return P(t, torch.zeros(t.shape, dtype=torch.float32, device=DEV))


def run(dtype, enabled, monkeypatch, apart=None, peek=False):
    """One forward + backward.  apart: the group whose consumer writes a tensor of its own instead of its rows of t2 (its gradient is then not
    adjacent to the others').  peek: a tape entry between the consumers and the LayerNorm reads the gradient of t1."""
    from transception_amd import engine
    from transception_amd.engine import Graph, Var
    monkeypatch.setattr(engine, "_PENDING_RES", enabled)
    G = Graph(dtype, torch.device(DEV), training=True, record=True)
    x0 = Var(vals("x0", (ROWS, CD), dtype))
    W0, b0 = mkP(vals("W0", (CD, CD), dtype, 0.125)), mkP(vals("b0", (CD,), dtype, 0.1))
    t1 = G.linear(x0, W0, b0, out=G.new(ROWS, CD, covered=True))
    gp, bp = mkP(vals("g", (CD,), dtype, 0.2) + 1.0), mkP(vals("b", (CD,), dtype, 0.3))
    tx = G.layernorm(t1, gp, bp, out=G.new(ROWS, CD, covered=True))
    seen = []
    if peek:
        G._rec(lambda: seen.append(G.grad_of(t1).clone()))
    t2 = G.new(ROWS, CD)
    own = G.new(GROUPS[apart][1] - GROUPS[apart][0], CD) if apart is not None else None
    Ws = [(mkP(vals(f"W{s}", (CD, CD), dtype, 0.125)), mkP(vals(f"b{s}", (CD,), dtype, 0.1))) for s in range(4)]
    for s, (a, b) in enumerate(GROUPS):
        G.linear(tx.rowslice(a, b), Ws[s][0], Ws[s][1], out=own if s == apart else t2.rowslice(a, b), residual=t1.rowslice(a, b))
    gy = vals("gy", (ROWS, CD), dtype)
    t2.root.grad_t, t2.root.whole_written = gy.clone(), True
    if own is not None:
        a, b = GROUPS[apart]
        own.root.grad_t, own.root.whole_written = gy[a:b].clone(), True
    torch.cuda.synchronize()
    calls0 = _lib._Lib.calls
    G.backward()
    torch.cuda.synchronize()
    calls = _lib._Lib.calls - calls0
    grads = [G.grad_of(t1), G.grad_of(x0), W0.grad, b0.grad, gp.grad, bp.grad] + [q.grad for pair in Ws for q in pair]
    return [g.clone() for g in grads], calls, seen, gy


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=_name)
def test_adjacent_sources_reach_the_layernorm_without_a_copy(dtype, monkeypatch):
    """Case a: the four residual gradients are the four row groups of t2's gradient: no copy launch at all."""
    off, n_off, _, _ = run(dtype, False, monkeypatch)
    on, n_on, _, _ = run(dtype, True, monkeypatch)
    assert all(same_bits(a, b) for a, b in zip(on, off))
    assert n_off - n_on == 4                                      # one tc_copy3d per residual, gone


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_name)
@pytest.mark.parametrize("apart", [1, 3])
def test_sources_that_are_not_adjacent_are_copied_in_one_launch(apart, dtype, monkeypatch):
    """Case b: one group's gradient lives in a tensor of its own: the LayerNorm backward cannot read one tensor, so the four copies are made --
    in one tc_ew_multi launch instead of four tc_copy3d."""
    off, n_off, _, _ = run(dtype, False, monkeypatch, apart=apart)
    on, n_on, _, _ = run(dtype, True, monkeypatch, apart=apart)
    assert all(same_bits(a, b) for a, b in zip(on, off))
    assert n_off - n_on == 3


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_name)
def test_a_read_between_registration_and_the_layernorm_sees_complete_data(dtype, monkeypatch):
    """Case c: grad_of on the root while the copies are pending makes them first."""
    off, n_off, seen_off, gy = run(dtype, False, monkeypatch, peek=True)
    on, n_on, seen_on, _ = run(dtype, True, monkeypatch, peek=True)
    assert len(seen_on) == len(seen_off) == 1
    assert same_bits(seen_on[0], gy) and same_bits(seen_off[0], gy)          # every row group is there: the residual gradients are t2's
    assert all(same_bits(a, b) for a, b in zip(on, off))
    assert n_off - n_on == 3

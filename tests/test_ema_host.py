"""Weight averaging without a GPU: the closed form of tests/ema_ref.py against torch.optim.swa_utils.AveragedModel, the decay schedule,
TrainConfig's three fields, the binding derived from include/transception_ema.h, and the refusals of the three entries (status -1 before
any launch)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from ema_ref import decay_at, ema_ref, f32, state_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMA_HEADER = os.path.join(ROOT, "include", "transception_ema.h")
ENTRIES = {"tc_ema_abi_version": 0, "tc_ema_advance": 5, "tc_ema_update_multi": 8, "tc_swap_f32": 4}


@pytest.fixture(scope="module")
def built():
    from transception_amd.build import build
    return build(verbose=False)


# ---------------------------------------------------------------------------------------------------------------- the closed form
def test_closed_form_matches_torch_averaged_model():
    """Six updates of a small CPU module (its weights moved between updates), warmup off, decay 0.9: AveragedModel with
    get_ema_multi_avg_fn copies at the first update and lerps afterwards.  Each of its float32 results lies within the derived bound of
    the float64 closed form applied to its own previous value; a free-running float64 chain of the closed form stays within the
    accumulated bounds of it."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    decay = 0.9
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay))
    flat = lambda mod: torch.cat([p.detach().reshape(-1) for p in mod.parameters()]).numpy().copy()
    e_prev, chain, slack = None, None, 0.0
    for n in range(1, 7):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.3 * torch.randn_like(p))
        w = flat(m)
        avg.update_parameters(m)
        got = flat(avg.module)
        _, d, omd, _ = state_words(n, decay, False)
        assert int(avg.n_averaged) == n and d == (0.0 if n == 1 else f32(decay)) and omd == f32(1.0 - (0.0 if n == 1 else decay))
        if n == 1:
            ref, bound = ema_ref(np.zeros_like(w), w, omd)
            assert np.array_equal(got.astype(np.float64), ref) and not bound.any()          # the first update copies
            chain = ref
        else:
            ref, bound = ema_ref(e_prev, w, omd)
            err = np.abs(got.astype(np.float64) - ref)
            assert (err <= bound).all(), (n, float((err / bound).max()))
            chain = chain + omd * (w.astype(np.float64) - chain)
            slack = slack * f32(decay) + float(bound.max())
            assert float(np.abs(got - chain).max()) <= slack, (n, slack)
        e_prev = got
    assert not np.array_equal(e_prev, flat(m))


def test_closed_form_copies_where_omd_is_one():
    e, w = np.float32([1e8, -3.0, 0.0]), np.float32([1.0, 2.5, -0.0])
    assert np.float32(e[0] + (w[0] - e[0])) != w[0]                       # why the kernel stores the value itself
    ref, bound = ema_ref(e, w, 1.0)
    assert np.array_equal(ref, w.astype(np.float64)) and not bound.any()
    ref, bound = ema_ref(torch.from_numpy(e), torch.from_numpy(w), 1.0)
    assert torch.equal(ref, torch.from_numpy(w).double()) and not bool(bound.any())
    ref, bound = ema_ref(torch.from_numpy(e), torch.from_numpy(w), 0.25)
    assert torch.equal(ref, torch.tensor([0.75e8 + 0.25, -1.625, 0.0], dtype=torch.float64)) and bool((bound[:2] > 0).all())


# ---------------------------------------------------------------------------------------------------------------- the schedule
def test_warmup_schedule():
    """n = 1, 2, 9, 10 and 10^5 at decay 0.999: 0, then (1 + n) / (10 + n) until it exceeds the decay."""
    want = {1: 0.0, 2: 3.0 / 12.0, 9: 10.0 / 19.0, 10: 11.0 / 20.0, 10 ** 5: 0.999}
    for n, d in want.items():
        assert decay_at(n, 0.999, True) == d, n
        assert decay_at(n, 0.999, False) == (0.0 if n == 1 else 0.999), n
        assert state_words(n, 0.999, True) == (n, f32(d), f32(1.0 - d), 0)
    assert decay_at(10 ** 5, 0.999, True) < (1.0 + 10 ** 5) / (10.0 + 10 ** 5)
    assert decay_at(8989, 0.999, True) == 8990.0 / 8999.0 < 0.999 == decay_at(8991, 0.999, True)      # where the warmup ends
    assert decay_at(5, 0.3, True) == 0.3 and state_words(1, 0.9, False) == (1, 0.0, 1.0, 0)
    with pytest.raises(ValueError):
        decay_at(0, 0.9, True)


# ---------------------------------------------------------------------------------------------------------------- TrainConfig
def test_train_config_fields():
    from transception_amd.trainer import TrainConfig
    cfg = TrainConfig("root", "lists")
    assert (cfg.ema_decay, cfg.ema_warmup, cfg.ema_eval) == (None, True, True)
    names = list(TrainConfig.__dataclass_fields__)
    assert names[-3:] == ["ema_decay", "ema_warmup", "ema_eval"] and names[-4] == "no_decay"      # appended: positional callers keep working
    for ok in (0.0, 0.5, 0.999, 0):
        assert TrainConfig("root", "lists", ema_decay=ok).ema_decay == ok
    for bad in (True, False, "0.9", 1.0, 1.5, -0.1, math.nan, math.inf, (0.9,)):
        with pytest.raises(ValueError, match="EMA decay"):
            TrainConfig("root", "lists", ema_decay=bad)


def test_weight_ema_checks_its_decay():
    from transception_amd.train import WeightEMA
    for bad in (True, "0.9", 1.0, -0.1, math.nan):
        with pytest.raises(ValueError, match="EMA decay"):
            WeightEMA(None, decay=bad)
    ema = WeightEMA(None)
    assert (ema.decay, ema.warmup, ema.updates()) == (0.999, True, 0)


# ---------------------------------------------------------------------------------------------------------------- the binding
def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(EMA_HEADER).read(), flags=re.S)
    fns = {}
    for m in re.finditer(r"\b(?:int|long long)\s+(tc_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        fns[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return fns


def test_binding_is_the_header(built):
    from transception_amd import _header, _lib
    fns = header_functions()
    assert fns == ENTRIES
    dll = ctypes.CDLL(built)
    for name in fns:
        assert hasattr(dll, name), f"{name} declared in the header but not exported by {built}"
    assert set(_lib.EMA.functions) == set(ENTRIES)
    for name, n in ENTRIES.items():
        assert len(_lib.EMA.functions[name].argtypes) == n, name
    assert {n for n, f in _lib.EMA.functions.items() if f.query} == {"tc_ema_abi_version"}
    assert _lib.EMA.functions["tc_ema_advance"].argtypes[2] is ctypes.c_double                    # decay
    assert _lib.EMA.functions["tc_ema_update_multi"].argtypes[4] is ctypes.c_longlong             # max_len
    assert _lib.EMA.functions["tc_swap_f32"].argtypes[2] is ctypes.c_longlong                     # n
    assert not _lib.EMA.structs
    assert not set(_lib.EMA.functions) & set(_lib.SIGNATURES) and not set(_lib.EMA.functions) & set(_lib.POST.functions)
    assert _lib.EMA.constants == {"TC_EMA_ABI_VERSION": 1}
    assert _header.load(EMA_HEADER).functions.keys() == fns.keys()          # self-contained: the parser refuses an #include
    assert dll.tc_ema_abi_version() == _lib.EMA_ABI_VERSION == 1
    L = _lib.lib()
    assert L.tc_ema_abi_version is L.cdll.tc_ema_abi_version                # the query is exposed raw, the three status entries checked
    for name in ("tc_ema_advance", "tc_ema_update_multi", "tc_swap_f32"):
        assert getattr(L, name).__name__ == name and getattr(L, name) is not getattr(L.cdll, name)


# ---------------------------------------------------------------------------------------------------------------- refusals
A, B, S, T = 0x10000, 0x20000, 0x30000, 0x40000        # non-null, 16-byte aligned addresses that are never dereferenced: every call below is refused


def test_entries_refuse_bad_arguments_before_any_launch(built):
    from transception_amd import _lib
    L = _lib.lib()
    bad = [("tc_ema_advance", (None, None, 0.9, 1, None)),
           ("tc_ema_advance", (None, S, 0.9, 0, None)),
           ("tc_ema_advance", (T, None, 1.0, 1, None)),
           ("tc_ema_advance", (T, None, 1.5, 1, None)),
           ("tc_ema_advance", (T, None, -1e-9, 1, None)),
           ("tc_ema_advance", (T, None, math.nan, 1, None)),
           ("tc_ema_advance", (T, None, math.inf, 0, None)),
           ("tc_ema_advance", (T, None, -math.inf, 0, None)),
           ("tc_ema_update_multi", (None, B, S, 1, 64, T, None, None)),
           ("tc_ema_update_multi", (A, None, S, 1, 64, T, None, None)),
           ("tc_ema_update_multi", (A, B, None, 1, 64, T, None, None)),
           ("tc_ema_update_multi", (A, B, S, 1, 64, None, None, None)),
           ("tc_ema_update_multi", (A, B, S, 0, 64, T, None, None)),
           ("tc_ema_update_multi", (A, B, S, -2, 64, T, None, None)),
           ("tc_ema_update_multi", (A, B, S, 65536, 64, T, None, None)),
           ("tc_ema_update_multi", (A, B, S, 1, 0, T, None, None)),
           ("tc_swap_f32", (None, B, 64, None)),
           ("tc_swap_f32", (A, None, 64, None)),
           ("tc_swap_f32", (A, A, 64, None)),
           ("tc_swap_f32", (A, B, 0, None)),
           ("tc_swap_f32", (A, B, -4, None)),
           ("tc_swap_f32", (A, B, 66, None)),
           ("tc_swap_f32", (A + 4, B, 64, None)),
           ("tc_swap_f32", (A, B + 8, 64, None))]
    for name, args in bad:
        with pytest.raises(_lib.TcError, match=f"{name} failed with status -1"):
            getattr(L, name)(*args)

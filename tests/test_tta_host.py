"""Test-time augmentation without a GPU: the views of tests/tta_ref.py against a nested loop over the index form, the number facts the
exact GPU test rests on, a float32 emulation of the kernel's arithmetic inside the bound the GPU test asserts, `TTA` and `TrainConfig.tta`,
the binding derived from include/transception_tta.h, and the refusals of the two entries (status -1 before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tta_ref import sum_probs, unview, view, where_in_view

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TTA_HEADER = os.path.join(ROOT, "include", "transception_tta.h")
ENTRIES = {"tc_tta_abi_version": 0, "tc_tta_view": 9, "tc_tta_accumulate": 11}
SHAPES = [(2, 9, 5, 7), (1, 2, 3, 130), (3, 16, 33, 33), (2, 9, 64, 64), (1, 1, 4, 4)]       # the GPU test's


@pytest.fixture(scope="module")
def built():
    from transception_amd.build import build
    return build(verbose=False)


# ---------------------------------------------------------------------------------------------------------------- the views
@pytest.mark.parametrize("H,W,views", [(5, 7, range(4)), (6, 6, range(8))])
def test_views_against_the_index_form(H, W, views):
    a = torch.arange(2 * H * W, dtype=torch.float64).reshape(2, H, W)
    seen = set()
    for v in views:
        b = view(a, v)
        assert b.shape == ((2, W, H) if v & 4 else (2, H, W))
        assert torch.equal(unview(b, v), a)
        for p in range(H):
            for q in range(W):
                y, x = where_in_view(v, H, W, p, q)
                assert b[0, y, x] == a[0, p, q] and b[1, y, x] == a[1, p, q], (v, p, q)
        seen.add(tuple(b[0].reshape(-1).tolist()))
    assert len(seen) == len(views)                                   # the views are different maps


def test_transposed_views_are_the_rotations():
    a = torch.arange(36.0).reshape(6, 6)
    assert torch.equal(view(a, 4), a.T)
    rots = {tuple(torch.rot90(a, k).reshape(-1).tolist()) for k in (1, 2, 3)}
    assert rots <= {tuple(view(a, v).reshape(-1).tolist()) for v in range(8)}
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            view(a, bad)


# ---------------------------------------------------------------------------------------------------------------- number facts
def test_one_hot_logits_are_exact_in_every_dtype():
    """What the exact geometry test on the GPU rests on: -200 is a value of all three formats, and exp(-200) rounds to 0 in fp32 (with or
    without denormals: it lies below the smallest one), so the softmax of (0, -200, ...) is (1, 0, ...) exactly."""
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert float(torch.tensor(-200.0).to(dt).float()) == -200.0
        assert float(torch.tensor(0.0).to(dt).float()) == 0.0
    assert float(torch.exp(torch.tensor(-200.0, dtype=torch.float32))) == 0.0
    assert np.exp(np.float64(-200.0)) < 2.0 ** -149 / 2                      # below half the smallest fp32 denormal
    p = torch.softmax(torch.tensor([-200.0, 0.0, -200.0]), 0)
    assert p.tolist() == [0.0, 1.0, 0.0]


def test_float32_emulation_is_inside_the_bound():
    """The kernel's arithmetic restated in float32 torch on the CPU (max, exp of the difference, the sum in class order, one division, one
    running add per view) stays below 1e-6 for all views together on the GPU test's shapes, half of the 2e-6 PER VIEW that test allows."""
    g = torch.Generator().manual_seed(11)
    worst = 0.0
    for N, C, H, W in SHAPES:
        views = list(range(8 if H == W else 4))
        for scale in (1.0, 4.0, 12.0):
            logits = [torch.randn((N, C, W, H) if v & 4 else (N, C, H, W), generator=g) * scale for v in views]
            acc = torch.zeros((N, C, H, W), dtype=torch.float32)
            for v, lg in zip(views, logits):
                e = torch.exp(lg - lg.max(dim=1, keepdim=True).values)
                s = torch.zeros_like(e[:, 0])
                for k in range(C):
                    s = s + e[:, k]
                acc = acc + unview(e / s[:, None], v)
            err = float((acc.double() - sum_probs(views, logits)).abs().max())
            worst = max(worst, err)
            assert err <= 2e-6 * len(views)
    assert worst < 1e-6, worst


# ---------------------------------------------------------------------------------------------------------------- TTA, TrainConfig
def test_tta_validation():
    from transception_amd.evaluate import TTA
    assert TTA().views == TTA.flips().views == (0, 1, 2, 3)
    assert TTA.dihedral().views == tuple(range(8))
    assert TTA((6, 0, 3)).views == (6, 0, 3)                                   # the order given is kept
    assert TTA((np.int64(5),)).views == (5,)
    for bad in ((), [0, 1], None, 3, (0, 0), (1, 2, 1), (8,), (-1,), (0, 1.0), (True,), (0, False), ("1",), (0, None)):
        with pytest.raises(ValueError):
            TTA(bad)
    with pytest.raises(Exception):                                             # frozen
        TTA().views = (0,)


def test_train_config_tta():
    from transception_amd.evaluate import TTA
    from transception_amd.trainer import TrainConfig
    assert TrainConfig("root", "lists").tta is None
    assert TrainConfig.__dataclass_fields__["tta"].default is None
    assert TrainConfig("root", "lists", tta=TTA.dihedral()).tta.views == tuple(range(8))
    for bad in ((0, 1), "flips", 4, True, [TTA()]):
        with pytest.raises(ValueError, match="tta"):
            TrainConfig("root", "lists", tta=bad)
    # keyword-only: the positional order of the other fields is what it was
    import inspect
    params = inspect.signature(TrainConfig).parameters
    assert params["tta"].kind is inspect.Parameter.KEYWORD_ONLY
    assert [n for n, p in params.items() if p.kind is not inspect.Parameter.KEYWORD_ONLY] == [n for n in TrainConfig.__dataclass_fields__ if n != "tta"]


def test_evaluate_refuses_a_bad_tta_before_anything_runs():
    """Anything but None or a TTA is a ValueError in every entry that takes `tta`, raised before the model or the device is touched (the
    model here is None); so is a transposed view with a non-square patch."""
    from transception_amd.evaluate import TTA, evaluate_volume, inference, predict_probs, predict_slices
    img, lab = np.zeros((1, 48, 64), np.float32), np.zeros((1, 48, 64), np.uint8)
    for bad in ((0, 1), "flips", 4, True):
        with pytest.raises(ValueError, match="tta"):
            predict_slices(None, torch.zeros(1, 48, 64), tta=bad)
        with pytest.raises(ValueError, match="tta"):
            predict_probs(None, torch.zeros(1, 48, 64), tta=bad)
        with pytest.raises(ValueError, match="tta"):
            evaluate_volume(None, img, lab, patch_size=(48, 64), tta=bad)
        with pytest.raises(ValueError, match="tta"):
            inference(None, [(img, lab, "case")], tta=bad)
    with pytest.raises(ValueError, match="square"):
        evaluate_volume(None, img, lab, patch_size=(48, 64), tta=TTA.dihedral())


# ---------------------------------------------------------------------------------------------------------------- the binding
def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(TTA_HEADER).read(), flags=re.S)
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
    assert set(_lib.TTA.functions) == set(ENTRIES)
    for name, n in ENTRIES.items():
        assert len(_lib.TTA.functions[name].argtypes) == n, name
    assert {n for n, f in _lib.TTA.functions.items() if f.query} == {"tc_tta_abi_version"}
    assert _lib.TTA.functions["tc_tta_view"].argtypes[6] is ctypes.c_float and _lib.TTA.functions["tc_tta_view"].argtypes[7] is ctypes.c_float
    assert _lib.TTA.functions["tc_tta_accumulate"].argtypes[1] is ctypes.c_int                    # dtype
    assert not _lib.TTA.structs
    for other in (_lib.SIGNATURES, _lib.POST.functions, _lib.EMA.functions):
        assert not set(_lib.TTA.functions) & set(other)
    assert _lib.TTA.constants == {"TC_TTA_ABI_VERSION": 1, "TC_TTA_FLIP_H": 1, "TC_TTA_FLIP_W": 2, "TC_TTA_TRANSPOSE": 4}
    assert (_lib.TC_TTA_FLIP_H, _lib.TC_TTA_FLIP_W, _lib.TC_TTA_TRANSPOSE) == (1, 2, 4)
    assert _header.load(TTA_HEADER).functions.keys() == fns.keys()          # self-contained: the parser refuses an #include
    assert dll.tc_tta_abi_version() == _lib.TTA_ABI_VERSION == 1
    L = _lib.lib()
    assert L.tc_tta_abi_version is L.cdll.tc_tta_abi_version                # the query is exposed raw, the two status entries checked
    for name in ("tc_tta_view", "tc_tta_accumulate"):
        assert getattr(L, name).__name__ == name and getattr(L, name) is not getattr(L.cdll, name)
    from transception_amd.build import SOURCES
    assert "tta.hip" in SOURCES


# ---------------------------------------------------------------------------------------------------------------- refusals
A, B, P = 0x10000, 0x20000, 0x30000        # non-null, 16-byte aligned addresses that are never dereferenced: every call below is refused
F32, BF16, F16 = 0, 1, 2


def test_entries_refuse_bad_arguments_before_any_launch(built):
    from transception_amd import _lib
    L = _lib.lib()
    assert (_lib.TC_F32, _lib.TC_BF16, _lib.TC_F16) == (F32, BF16, F16)
    bad = [("tc_tta_view", (None, B, 2, 8, 8, 0, 0.5, 0.5, None)),                 # src NULL
           ("tc_tta_view", (A, None, 2, 8, 8, 0, 0.5, 0.5, None)),                 # dst NULL
           ("tc_tta_view", (A, A, 2, 8, 8, 0, 0.5, 0.5, None)),                    # in place
           ("tc_tta_view", (A, B, 0, 8, 8, 0, 0.5, 0.5, None)),
           ("tc_tta_view", (A, B, -1, 8, 8, 0, 0.5, 0.5, None)),
           ("tc_tta_view", (A, B, 2, 0, 8, 0, 0.5, 0.5, None)),
           ("tc_tta_view", (A, B, 2, 8, -3, 0, 0.5, 0.5, None)),
           ("tc_tta_view", (A, B, 2, 8, 8, -1, 0.5, 0.5, None)),                   # view outside 0..7
           ("tc_tta_view", (A, B, 2, 8, 8, 8, 0.5, 0.5, None)),
           ("tc_tta_view", (A, B, 2, 8, 9, 4, 0.5, 0.5, None)),                    # transpose, H != W
           ("tc_tta_view", (A, B, 2, 9, 8, 7, 0.5, 0.5, None)),
           ("tc_tta_view", (A, B, 2, 8, 8, 0, 0.5, 0.0, None)),                    # stdv == 0
           ("tc_tta_view", (A, B, 2, 8, 8, 0, 0.5, -0.0, None)),
           ("tc_tta_view", (A, B, 2 ** 11, 2 ** 10, 2 ** 10, 0, 0.5, 0.5, None)),  # 2^31 elements
           ("tc_tta_view", (A, B, 2 ** 30, 2 ** 30, 2 ** 30, 0, 0.5, 0.5, None)),  # a product that wraps 64 bits
           ("tc_tta_accumulate", (None, F32, A, None, 2, 9, 8, 8, 0, 1, None)),    # logits NULL
           ("tc_tta_accumulate", (B, F32, None, None, 2, 9, 8, 8, 0, 1, None)),    # acc NULL without pred
           ("tc_tta_accumulate", (B, F32, None, None, 2, 9, 8, 8, 0, 0, None)),
           ("tc_tta_accumulate", (B, F32, None, P, 2, 9, 8, 8, 0, 0, None)),       # acc NULL with pred, but not first
           ("tc_tta_accumulate", (A, F32, A, None, 2, 9, 8, 8, 0, 1, None)),       # acc == logits
           ("tc_tta_accumulate", (A, F32, A, P, 2, 9, 8, 8, 0, 0, None)),
           ("tc_tta_accumulate", (B, F32, A, None, 2, 9, 8, 8, -1, 1, None)),      # view outside 0..7
           ("tc_tta_accumulate", (B, F32, A, None, 2, 9, 8, 8, 8, 1, None)),
           ("tc_tta_accumulate", (B, F32, A, None, 2, 9, 8, 9, 4, 1, None)),       # transpose, H != W
           ("tc_tta_accumulate", (B, BF16, A, P, 2, 9, 9, 8, 5, 0, None)),
           ("tc_tta_accumulate", (B, F32, A, None, 2, 0, 8, 8, 0, 1, None)),       # ncls outside 1..16
           ("tc_tta_accumulate", (B, F32, A, None, 2, 17, 8, 8, 0, 1, None)),
           ("tc_tta_accumulate", (B, F32, A, None, 2, -9, 8, 8, 0, 1, None)),
           ("tc_tta_accumulate", (B, F32, A, None, 0, 9, 8, 8, 0, 1, None)),       # N, H, W <= 0
           ("tc_tta_accumulate", (B, F32, A, None, 2, 9, 0, 8, 0, 1, None)),
           ("tc_tta_accumulate", (B, F32, A, None, 2, 9, 8, -8, 0, 1, None)),
           ("tc_tta_accumulate", (B, F32, A, None, 2 ** 7, 16, 2 ** 10, 2 ** 10, 0, 1, None)),     # 2^31 elements
           ("tc_tta_accumulate", (B, F16, A, P, 2 ** 30, 16, 2 ** 30, 2 ** 30, 0, 0, None)),       # a product that wraps 64 bits
           ("tc_tta_accumulate", (B, 3, A, None, 2, 9, 8, 8, 0, 1, None)),         # unknown dtype
           ("tc_tta_accumulate", (B, -1, A, P, 2, 9, 8, 8, 0, 1, None)),
           ("tc_tta_accumulate", (B, F32, A, None, 2, 9, 8, 8, 0, 2, None)),       # first outside {0, 1}
           ("tc_tta_accumulate", (B, F32, A, P, 2, 9, 8, 8, 0, -1, None))]
    for name, args in bad:
        with pytest.raises(_lib.TcError, match=f"{name} failed with status -1"):
            getattr(L, name)(*args)

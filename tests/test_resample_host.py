"""Score resampling without a GPU: the float64 reference of tests/resample_ref.py against torch's own bilinear interpolation and against
its index form, the validation of `resample=` / `out_size=` / `TrainConfig.resample`, the binding derived from
include/transception_resample.h, and the refusals of the entry (status -1 before any launch)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resample_ref import labels, resample, resample_index, tap, taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "transception_resample.h")
ENTRIES = {"tc_resample_abi_version": 0, "tc_resample_scores": 11}
DYADIC = [((7, 7), (16, 16)), ((14, 21), (32, 48)), ((5, 6), (10, 24)), ((8, 8), (32, 32)), ((64, 64), (128, 256)), ((224, 224), (512, 512)),
          ((3, 4), (3, 4))]
OTHER = [((5, 7), (7, 5)), ((9, 5), (13, 300)), ((12, 12), (5, 7))]


@pytest.fixture(scope="module")
def built():
    from transception_amd.build import build
    return build(verbose=False)


def grid_eighths(shape, seed):
    """multiples of 1/8 in [-8, 8]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-64, 65, shape, generator=g).float() / 8


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("src,dst", DYADIC, ids=lambda v: "x".join(map(str, v)))
def test_reference_equals_interpolate_on_dyadic_ratios(src, dst):
    """Every weight is a multiple of 1/32 and every input one of 1/8: all products and sums are exact in fp32, so torch's fp32 result and
    the float64 reference are the same numbers."""
    v = grid_eighths((2, 3) + src, 5)
    got = resample(v, dst)
    want = F.interpolate(v, size=dst, mode="bilinear", align_corners=False)
    assert got.dtype == torch.float64 and got.shape == want.shape
    assert torch.equal(got, want.double())
    if src == dst:
        assert torch.equal(got, v.double())


@pytest.mark.parametrize("src,dst", OTHER, ids=lambda v: "x".join(map(str, v)))
def test_reference_is_close_to_interpolate_elsewhere(src, dst):
    """Seeded normals at ratios that are no power of two: within 2^-19 max|v| (measured: 10.3 * 2^-24 max|v| at worst, which is torch's own fp32
    coordinate rounding, not the definition)."""
    v = torch.randn((2, 3) + src, generator=torch.Generator().manual_seed(7))
    got = resample(v, dst)
    want = F.interpolate(v, size=dst, mode="bilinear", align_corners=False).double()
    err = float((got - want).abs().max())
    print(f"{src}->{dst}: {err / float(v.abs().max()) * 2 ** 24:.2f} * 2^-24 max|v|")
    assert err <= 2.0 ** -19 * float(v.abs().max())


@pytest.mark.parametrize("src,dst", [s for s in DYADIC if s[1][0] <= 48] + OTHER, ids=lambda v: "x".join(map(str, v)))
def test_the_two_forms_agree(src, dst):
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        v = torch.randn((2, 3) + src, generator=torch.Generator().manual_seed(3)).to(dt)
        assert torch.equal(resample(v, dst), resample_index(v, dst))
    for n, out in ((src[0], dst[0]), (src[1], dst[1])):
        t0, t1, lam = taps(n, out)
        for o in range(out):
            assert (int(t0[o]), int(t1[o]), float(lam[o])) == tap(o, n, out)
            assert 0 <= t0[o] <= t1[o] <= n - 1 and 0.0 <= lam[o] < 1.0
        assert bool((t0[1:] >= t0[:-1]).all())                       # monotone: a tile's footprint is a rectangle


def test_first_maximum():
    s = torch.tensor([[[[1.0]], [[3.0]], [[3.0]], [[2.0]]]])
    assert labels(s).tolist() == [[[1]]] and labels(s).dtype == torch.uint8


# ---------------------------------------------------------------------------------------------------------------- validation
def test_train_config_resample():
    from transception_amd.trainer import TrainConfig
    assert TrainConfig("root", "lists").resample == "labels" and TrainConfig.resample == "labels"
    assert TrainConfig("root", "lists", resample="scores").resample == "scores"
    for bad in ("bilinear", "", None, 1, True, ("scores",), "Scores"):
        with pytest.raises(ValueError, match="resample"):
            TrainConfig("root", "lists", resample=bad)
    params = inspect.signature(TrainConfig).parameters
    assert params["resample"].kind is inspect.Parameter.KEYWORD_ONLY and params["resample"].default == "labels"
    assert list(params)[-1] == "resample"
    positional = [p.default for p in params.values() if p.kind is not inspect.Parameter.KEYWORD_ONLY][2:]
    assert TrainConfig("root", "lists", *positional).resample == "labels"
    with pytest.raises(TypeError):
        TrainConfig("root", "lists", *positional, "scores")                                   # not reachable by position


def test_new_parameters_are_keyword_only_and_last():
    from transception_amd import evaluate
    for fn, name, default in ((evaluate.predict_slices, "out_size", None), (evaluate.predict_probs, "out_size", None),
                              (evaluate.evaluate_volume, "resample", "labels"), (evaluate.inference, "resample", "labels")):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == name, fn.__name__
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default, fn.__name__
        assert [p.kind for p in params.values()].count(inspect.Parameter.KEYWORD_ONLY) == 1, fn.__name__
    assert evaluate.RESAMPLE_MODES == ("labels", "scores")


def test_evaluate_refuses_a_bad_resample_before_anything_runs():
    """The model here is None: a ValueError must come before it or the device is touched."""
    from transception_amd.evaluate import evaluate_volume, inference, predict_probs, predict_slices
    img, lab = np.zeros((1, 96, 96), np.float32), np.zeros((1, 96, 96), np.uint8)
    for bad in ("bilinear", "", None, 1, True, ("scores",)):
        with pytest.raises(ValueError, match="resample"):
            evaluate_volume(None, img, lab, patch_size=(64, 64), resample=bad)
        with pytest.raises(ValueError, match="resample"):
            inference(None, [(img, lab, "case")], resample=bad)
    with pytest.raises(ValueError, match="host_zoom"):
        evaluate_volume(None, img, lab, patch_size=(64, 64), host_zoom=True, resample="scores")
    with pytest.raises(ValueError, match="host_zoom"):
        evaluate_volume(None, img, lab, patch_size=(96, 96), host_zoom=True, resample="scores")   # also where nothing would be resized
    for bad in ((0, 8), (8, -1), (8,), (8, 8, 8), 8, "88", (8.0, 8), (True, 8), (4097, 8)):
        with pytest.raises(ValueError, match="out_size"):
            predict_slices(None, torch.zeros(1, 64, 64), out_size=bad)
        with pytest.raises(ValueError, match="out_size"):
            predict_probs(None, torch.zeros(1, 64, 64), out_size=bad)


# ---------------------------------------------------------------------------------------------------------------- the binding
def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
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
    assert set(_lib.RESAMPLE.functions) == set(ENTRIES)
    for name, n in ENTRIES.items():
        assert len(_lib.RESAMPLE.functions[name].argtypes) == n, name
    assert {n for n, f in _lib.RESAMPLE.functions.items() if f.query} == {"tc_resample_abi_version"}
    at = _lib.RESAMPLE.functions["tc_resample_scores"].argtypes
    assert all(t is ctypes.c_int for t in (at[1], *at[4:10])) and all(t is ctypes.c_void_p for t in (at[0], at[2], at[3], at[10]))
    assert not _lib.RESAMPLE.structs
    for other in (_lib.SIGNATURES, _lib.POST.functions, _lib.EMA.functions, _lib.TTA.functions):
        assert not set(_lib.RESAMPLE.functions) & set(other)
    assert _lib.RESAMPLE.constants == {"TC_RESAMPLE_ABI_VERSION": 1, "TC_RESAMPLE_MAX_EXTENT": 4096}
    assert _header.load(HEADER).functions.keys() == fns.keys()               # self-contained: the parser refuses an #include
    assert dll.tc_resample_abi_version() == _lib.RESAMPLE_ABI_VERSION == 1
    L = _lib.lib()
    assert L.tc_resample_abi_version is L.cdll.tc_resample_abi_version       # the query is exposed raw, the status entry checked
    assert L.tc_resample_scores.__name__ == "tc_resample_scores" and L.tc_resample_scores is not L.cdll.tc_resample_scores
    from transception_amd.build import SOURCES
    assert "resample.hip" in SOURCES


# ---------------------------------------------------------------------------------------------------------------- refusals
A, B, P = 0x10000, 0x20000, 0x30000        # non-null, 16-byte aligned addresses that are never dereferenced: every call below is refused
F32, BF16, F16 = 0, 1, 2


def test_entry_refuses_bad_arguments_before_any_launch(built):
    from transception_amd import _lib
    L = _lib.lib()
    assert (_lib.TC_F32, _lib.TC_BF16, _lib.TC_F16) == (F32, BF16, F16)
    #       src  dtype scores pred  N  ncls  h   w   H   W
    bad = [(None, F32, B, P, 2, 9, 8, 8, 16, 16),                   # src NULL
           (A, F32, None, None, 2, 9, 8, 8, 16, 16),                # both outputs NULL
           (A, F32, A, P, 2, 9, 8, 8, 16, 16),                      # scores aliasing src
           (A, F32, A, None, 2, 9, 8, 8, 8, 8),
           (A, BF16, B, A, 2, 9, 8, 8, 16, 16),                     # pred aliasing src
           (A, F32, None, A, 2, 9, 8, 8, 16, 16),
           (A, F32, B, P, 2, 0, 8, 8, 16, 16),                      # ncls outside 1..16
           (A, F32, B, P, 2, 17, 8, 8, 16, 16),
           (A, F32, None, P, 2, -9, 8, 8, 16, 16),
           (A, F32, B, P, 0, 9, 8, 8, 16, 16),                      # N <= 0
           (A, F32, B, P, -2, 9, 8, 8, 16, 16),
           (A, F32, B, P, 2, 9, 0, 8, 16, 16),                      # an extent <= 0
           (A, F32, B, P, 2, 9, 8, -8, 16, 16),
           (A, F32, B, P, 2, 9, 8, 8, 0, 16),
           (A, F32, None, P, 2, 9, 8, 8, 16, -1),
           (A, F32, B, P, 1, 1, 4097, 8, 16, 16),                   # an extent > 4096
           (A, F32, B, P, 1, 1, 8, 4097, 16, 16),
           (A, F32, None, P, 1, 1, 8, 8, 4097, 16),
           (A, F16, None, P, 1, 1, 8, 8, 16, 4097),
           (A, F32, None, P, 1, 1, 8, 8, 16, 2 ** 30),
           (A, F32, None, P, 8, 16, 4096, 4096, 8, 8),              # N ncls h w = 2^31
           (A, F32, None, P, 128, 1, 8, 8, 4096, 4096),             # N H W = 2^31
           (A, F32, B, P, 8, 16, 8, 8, 4096, 4096),                 # N ncls H W = 2^31 with scores ...
           (A, F32, B, None, 8, 16, 8, 8, 4096, 4096),
           (A, F32, B, P, 2 ** 30, 16, 4096, 4096, 4096, 4096),     # products far beyond 2^31
           (A, F32, None, P, 2 ** 31 - 1, 16, 4096, 4096, 4096, 4096),
           (A, 3, B, P, 2, 9, 8, 8, 16, 16),                        # unknown dtype
           (A, -1, None, P, 2, 9, 8, 8, 16, 16)]
    for args in bad:
        with pytest.raises(_lib.TcError, match="tc_resample_scores failed with status -1"):
            L.tc_resample_scores(*args, None)
    # the largest sizes are refused for the product, not one by one: every single argument above is legal somewhere
    assert _lib.TC_RESAMPLE_MAX_EXTENT == 4096

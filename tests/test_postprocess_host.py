"""Host side of the connected-component post-processing (transception_amd.evaluate.PostProcess / postprocess_host, the binding of
include/transception_post.h): `postprocess_host` against a pure-Python flood fill, argument validation, and the new C entries as far as
they answer without a GPU.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

from postprocess_util import flood_fill_post, organs_with_islands, tie_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POST_HEADER = os.path.join(ROOT, "include", "transception_post.h")

VOLUMES = [("organs3d", organs_with_islands((4, 11, 13), 3, 0.06, n_organs=5, max_label=6), 6),
           ("one-slice", organs_with_islands((1, 12, 15), 4, 0.08, n_organs=4, max_label=4), 5),
           ("2-d", organs_with_islands((13, 17), 5, 0.08, n_organs=4, max_label=9), 5),      # labels 5..9 are >= classes: background
           ("tie", tie_volume(), 4)]


@pytest.mark.parametrize("connectivity", [1, 3])
@pytest.mark.parametrize("name,lab,classes", VOLUMES, ids=[v[0] for v in VOLUMES])
def test_postprocess_host_follows_the_flood_fill(name, lab, classes, connectivity):
    from transception_amd.evaluate import PostProcess, postprocess_host
    before = lab.copy()
    posts = [PostProcess(connectivity=connectivity)] + [PostProcess("min_voxels", n, connectivity) for n in (1, 2, 5, 10 ** 9)]
    for post in posts:
        got = postprocess_host(lab, classes, post)
        assert got.dtype == np.uint8 and got.shape == lab.shape and got is not lab
        np.testing.assert_array_equal(got, flood_fill_post(lab, classes, post.mode, post.min_voxels, connectivity), err_msg=f"{name} {post}")
        np.testing.assert_array_equal(got[lab >= classes], lab[lab >= classes])
    np.testing.assert_array_equal(lab, before)                          # the input is left alone
    np.testing.assert_array_equal(postprocess_host(lab, classes, PostProcess("min_voxels", 1, connectivity)), lab)
    emptied = postprocess_host(lab, classes, PostProcess("min_voxels", 10 ** 9, connectivity))
    assert not ((emptied >= 1) & (emptied < classes)).any()


def test_tie_goes_to_the_first_component_in_raster_order():
    from transception_amd.evaluate import PostProcess, postprocess_host
    lab = tie_volume()
    got = postprocess_host(lab, 4)
    assert (got[0, 1, 1:7] == 1).all() and (got == 1).sum() == 6         # of the two 6-voxel components the first one stays
    assert (got[2, 2:4, 5:9] == 2).all() and (got == 2).sum() == 8       # the larger one wins wherever it lies
    assert postprocess_host(lab, 4, PostProcess(connectivity=3)).sum() == got.sum()
    with pytest.raises(ValueError):
        postprocess_host(lab.astype(np.int64), 4)
    with pytest.raises(ValueError):
        postprocess_host(lab, 17)


def test_postprocess_validation():
    from transception_amd.evaluate import PostProcess
    from transception_amd.trainer import TrainConfig
    p = PostProcess()
    assert (p.mode, p.min_voxels, p.connectivity) == ("largest", 0, 1)
    assert PostProcess("min_voxels", 1, 3).min_voxels == 1
    with pytest.raises(Exception):                                      # frozen
        p.mode = "min_voxels"
    for bad in (dict(mode="biggest"), dict(mode="min_voxels"), dict(mode="min_voxels", min_voxels=0), dict(mode="min_voxels", min_voxels=-4),
                dict(mode="largest", min_voxels=5), dict(mode="min_voxels", min_voxels=2.5), dict(connectivity=2), dict(connectivity=0),
                dict(connectivity=26)):
        with pytest.raises(ValueError):
            PostProcess(**bad)
    assert TrainConfig.__dataclass_fields__["postprocess"].default is None
    assert TrainConfig("root", "lists", postprocess=PostProcess("min_voxels", 10)).postprocess.min_voxels == 10
    for bad in ("largest", 5, {"mode": "largest"}):
        with pytest.raises(ValueError):
            TrainConfig("root", "lists", postprocess=bad)


def test_evaluation_refuses_what_is_no_postprocess():
    import torch
    from transception_amd.evaluate import evaluate_volume
    image, label = np.zeros((2, 32, 32), np.float32), np.zeros((2, 32, 32), np.uint8)
    with pytest.raises(ValueError, match="PostProcess"):
        evaluate_volume(torch.nn.Conv2d(1, 9, 1), image, label, 9, (32, 32), postprocess="largest")


def test_device_functions_have_no_cpu_fallback():
    import torch
    from transception_amd.evaluate import PostProcess, component_roots, component_sizes, postprocess_device
    lab = torch.zeros((2, 8, 8), dtype=torch.uint8)
    root = torch.zeros((2, 8, 8), dtype=torch.int32)
    for call in (lambda: component_roots(lab, 9), lambda: component_sizes(lab, root, 9), lambda: postprocess_device(lab, 9, PostProcess())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


@pytest.fixture(scope="module")
def built():
    from transception_amd.build import build
    return build(verbose=False)


def header_functions():
    src = re.sub(r"/\*.*?\*/", "", open(POST_HEADER).read(), flags=re.S)
    fns = {}
    for m in re.finditer(r"\b(?:int|long long)\s+(tc_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        fns[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return fns


def test_library_exports_the_post_header(built):
    from transception_amd import _header, _lib
    fns = header_functions()
    assert fns == {"tc_post_abi_version": 0, "tc_cc_scratch_bytes": 3, "tc_cc_label": 8, "tc_cc_sizes": 9, "tc_cc_keep": 12}
    dll = ctypes.CDLL(built)
    for name in fns:
        assert hasattr(dll, name), f"{name} declared in the header but not exported by {built}"
    assert set(_lib.POST.functions) == set(fns)
    for name, n in fns.items():
        assert len(_lib.POST.functions[name].argtypes) == n, name
    assert {n for n, f in _lib.POST.functions.items() if f.query} == {"tc_post_abi_version", "tc_cc_scratch_bytes"}
    assert _lib.POST.functions["tc_cc_scratch_bytes"].restype is ctypes.c_longlong
    assert _lib.POST.functions["tc_cc_keep"].argtypes[6] is ctypes.c_longlong          # min_voxels
    assert not _lib.POST.structs and not set(_lib.POST.functions) & set(_lib.SIGNATURES)
    assert _lib.POST.constants == {"TC_POST_ABI_VERSION": 1, "TC_CC_LARGEST": 0, "TC_CC_MIN_VOXELS": 1}
    assert _header.load(POST_HEADER).functions.keys() == fns.keys()          # self-contained: the parser refuses an #include
    assert dll.tc_post_abi_version() == _lib.POST_ABI_VERSION == 1


def test_queries_and_the_error_rule_without_a_gpu(built):
    from transception_amd import _lib
    from transception_amd.evaluate import postprocess_scratch_bytes
    L = _lib.lib()
    assert L.tc_post_abi_version() == 1
    assert L.tc_post_abi_version is L.cdll.tc_post_abi_version and L.tc_cc_label is not L.cdll.tc_cc_label       # raw query, checked status
    n = 148 * 512 * 512
    assert L.tc_cc_scratch_bytes(148, 512, 512) == postprocess_scratch_bytes((148, 512, 512)) == 8 * n == 310378496
    assert postprocess_scratch_bytes((5, 7)) == L.tc_cc_scratch_bytes(1, 5, 7) == 8 * 35
    assert L.tc_cc_scratch_bytes(2049, 4, 4) == 0 and L.tc_cc_scratch_bytes(0, 4, 4) == 0 and L.tc_cc_scratch_bytes(2048, 1024, 1024) == 0
    with pytest.raises(_lib.TcError, match="tc_cc_label failed with status -1"):
        L.tc_cc_label(None, None, 2, 8, 8, 9, 1, None)
    with pytest.raises(_lib.TcError, match="status -1"):
        L.tc_cc_sizes(None, None, None, None, 2, 8, 8, 9, None)
    with pytest.raises(_lib.TcError, match="status -1"):
        L.tc_cc_keep(None, None, None, None, None, _lib.TC_CC_LARGEST, 0, 2, 8, 8, 9, None)

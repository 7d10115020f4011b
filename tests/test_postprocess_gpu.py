"""Connected-component post-processing on the MI355X (csrc/postprocess.hip, transception_amd.evaluate.postprocess_device): root maps,
component sizes, the largest component per class and the two keep modes against scipy.ndimage.label plus numpy (postprocess_util.py) --
never against the code under test, and every comparison an equality."""
import functools

import numpy as np
import pytest
import torch

from metrics_util import DEV, dev as _dev, label_volume
from postprocess_util import organs_with_islands, tie_volume, want_post, want_root, want_sizes_best

pytestmark = pytest.mark.gpu

SHAPES = [(5, 12, 10), (1, 14, 12), (24, 96, 80), (3, 7, 130), (20, 26)]       # (3, 7, 130): a width that is no multiple of 64 and not below it


@functools.lru_cache(maxsize=None)
def _volume(shape):
    """9 labels (0..8) from `label_volume` plus 2 % island voxels of classes 1..11: with classes = 9 the labels 9..11 are background.
    Shared and cached: no test writes to it."""
    lab = organs_with_islands(shape, 100 + len(shape) + sum(shape), 0.02, n_organs=8, max_label=11)
    return lab


@functools.lru_cache(maxsize=None)
def _want_root(shape, connectivity):
    return want_root(_volume(shape), 9, connectivity)


@pytest.mark.parametrize("connectivity", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_root_map(shape, connectivity):
    from transception_amd.evaluate import component_roots
    lab = _volume(shape)
    if shape == (24, 96, 80):                                                      # the small ones need not hold every label
        assert (lab >= 9).any() and (lab == 0).any() and len(np.unique(lab[lab < 9])) == 9
    want = _want_root(shape, connectivity)
    got = component_roots(_dev(lab), 9, connectivity)
    assert got.dtype == torch.int32 and got.shape == lab.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert (want[(lab == 0) | (lab >= 9)] == -1).all() and (want[(lab > 0) & (lab < 9)] >= 0).all()
    assert torch.equal(component_roots(_dev(lab), 9, connectivity), got)           # bit-identical from run to run


def _serpentine():
    """One voxel wide through [1,64,65]: the even rows, joined alternately at their right and left ends -- one component whose chain is
    2000 voxels long and crosses every workgroup."""
    lab = np.zeros((1, 64, 65), np.uint8)
    lab[0, ::2] = 1
    lab[0, 1::4, -1] = 1
    lab[0, 3::4, 0] = 1
    return lab


def _comb():
    """Teeth that join only in the last row: the unions that make it one component arrive last in raster order."""
    lab = np.zeros((1, 48, 131), np.uint8)
    lab[0, :, ::2] = 1
    lab[0, -1, :] = 1
    return lab


def _checkerboard():
    z, y, x = np.meshgrid(np.arange(7), np.arange(9), np.arange(11), indexing="ij")
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def _two_combs():
    """Two interleaved combs of different labels: neighbours by geometry everywhere, never to be merged."""
    lab = np.zeros((2, 40, 70), np.uint8)
    lab[:, :-1, ::2] = 1
    lab[:, 1:, 1::2] = 2
    lab[:, 0, :] = 1
    lab[:, -1, :] = 2
    return lab


def _gap_row():
    lab = np.ones((1, 1, 70), np.uint8)
    lab[0, 0, 64] = 0
    return lab


HARD = [("serpentine", _serpentine, {1: 1, 3: 1}), ("comb", _comb, {1: 1, 3: 1}), ("checkerboard", _checkerboard, {1: 347, 3: 1}),
        ("full", lambda: np.ones((2, 300, 260), np.uint8), {1: 1, 3: 1}), ("two-combs", _two_combs, {1: 2, 3: 2}),
        ("1x1x1", lambda: np.ones((1, 1, 1), np.uint8), {1: 1, 3: 1}), ("3x1x1", lambda: np.ones((3, 1, 1), np.uint8), {1: 1, 3: 1}),
        ("1x1x70", lambda: np.ones((1, 1, 70), np.uint8), {1: 1, 3: 1}), ("1x1x70-gap", _gap_row, {1: 2, 3: 2}),
        ("background", lambda: np.zeros((3, 9, 70), np.uint8), {1: 0, 3: 0})]


@pytest.mark.parametrize("connectivity", [1, 3])
@pytest.mark.parametrize("name,make,components", HARD, ids=[h[0] for h in HARD])
def test_shapes_that_break_union_find(name, make, components, connectivity):
    from transception_amd.evaluate import PostProcess, component_roots, postprocess_device
    lab = make()
    want = want_root(lab, 3, connectivity)
    assert len(np.unique(want[want >= 0])) == components[connectivity]             # the case is what its name says
    got = component_roots(_dev(lab), 3, connectivity).cpu().numpy()
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(postprocess_device(_dev(lab), 3, PostProcess(connectivity=connectivity)).cpu().numpy(),
                                  want_post(lab, 3, "largest", 0, connectivity))


def _absent_class_volume():
    lab = np.array(_volume((24, 96, 80)))
    lab[lab == 4] = 0
    return lab


@pytest.mark.parametrize("connectivity", [1, 3])
@pytest.mark.parametrize("name,make,classes,absent", [("organs", _absent_class_volume, 9, 4), ("tie", tie_volume, 4, 3)], ids=["organs", "tie"])
def test_sizes_and_best(name, make, classes, absent, connectivity):
    from transception_amd.evaluate import component_roots, component_sizes
    lab = make()
    want_size, want_best = want_sizes_best(lab, classes, connectivity)
    d = _dev(lab)
    root = component_roots(d, classes, connectivity)
    size = torch.full(lab.shape, 77, dtype=torch.int32, device=DEV)                # OVERWRITTEN, whatever was there
    best = torch.full((classes, 2), -9, dtype=torch.int64, device=DEV)
    from transception_amd._lib import lib
    lib().tc_cc_sizes(d.data_ptr(), root.data_ptr(), size.data_ptr(), best.data_ptr(), *lab.shape, classes, torch.cuda.current_stream().cuda_stream)
    np.testing.assert_array_equal(size.cpu().numpy(), want_size)
    np.testing.assert_array_equal(best.cpu().numpy(), want_best)
    size2, best2 = component_sizes(d, root, classes)
    assert size2.dtype == torch.int32 and best2.dtype == torch.int64 and torch.equal(size2, size) and torch.equal(best2, best)
    r = root.cpu().numpy()
    assert (want_size[r != np.arange(lab.size).reshape(lab.shape)] == 0).all() and int(want_size.sum()) == int(((lab > 0) & (lab < classes)).sum())
    assert want_best[0].tolist() == [0, -1] and want_best[absent].tolist() == [0, -1]
    if name == "tie":
        assert want_best[1].tolist() == [6, 1 * 9 + 1] and want_best[2].tolist() == [8, (2 * 8 + 2) * 9 + 5]     # the first of two 6-voxel components


def _noncontiguous(lab):
    """A CUDA tensor of lab's shape and content whose memory is laid out [D,W,H]."""
    t = _dev(np.ascontiguousarray(lab.transpose(0, 2, 1))).transpose(1, 2)
    assert not t.is_contiguous() and t.shape == lab.shape
    return t


POSTS = [("largest", 0), ("min_voxels", 1), ("min_voxels", 5), ("min_voxels", 10 ** 9)]


@pytest.mark.parametrize("connectivity", [1, 3])
@pytest.mark.parametrize("shape", [(24, 96, 80), (3, 7, 130), (20, 26)], ids=str)
def test_keep(shape, connectivity):
    from transception_amd.evaluate import PostProcess, postprocess_device
    lab = _volume(shape)
    for mode, n in POSTS:
        post = PostProcess(mode, n, connectivity)
        want = want_post(lab, 9, mode, n, connectivity)
        d = _dev(lab)
        got = postprocess_device(d, 9, post)
        assert got is not d and got.dtype == torch.uint8 and torch.equal(d.cpu(), torch.from_numpy(np.array(lab)))     # the input is left alone
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str(post))
        np.testing.assert_array_equal(want[lab >= 9], lab[lab >= 9])                # labels >= classes survive
        assert postprocess_device(d, 9, post, out=d) is d                           # in place
        np.testing.assert_array_equal(d.cpu().numpy(), want, err_msg=f"in place {post}")
        if lab.ndim == 3:
            t = _noncontiguous(lab)
            np.testing.assert_array_equal(postprocess_device(t, 9, post).cpu().numpy(), want, err_msg=f"non-contiguous {post}")
            assert postprocess_device(t, 9, post, out=t) is t and not t.is_contiguous()
            np.testing.assert_array_equal(t.cpu().numpy(), want, err_msg=f"non-contiguous in place {post}")
    assert (want_post(lab, 9, "min_voxels", 1, connectivity) == lab).all()
    assert not np.isin(want_post(lab, 9, "min_voxels", 10 ** 9, connectivity), np.arange(1, 9)).any()


@pytest.mark.parametrize("connectivity", [1, 3])
def test_idempotence(connectivity):
    from transception_amd.evaluate import PostProcess, postprocess_device
    d = _dev(_volume((24, 96, 80)))
    for mode, n in POSTS:
        post = PostProcess(mode, n, connectivity)
        once = postprocess_device(d, 9, post)
        assert torch.equal(postprocess_device(once, 9, post), once), post
    assert not torch.equal(postprocess_device(d, 9, PostProcess(connectivity=connectivity)), d)


class _Binned(torch.nn.Module):
    """Logits that are the one-hot of the input intensity binned into 9 levels: an image of k / 8 is predicted as label k."""

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):                                                           # x = (image - 0.5) / 0.5 (predict_slices)
        k = torch.round((x[:, 0] * 0.5 + 0.5) * 8).long().clamp(0, 8)
        return torch.nn.functional.one_hot(k, 9).permute(0, 3, 1, 2).float().contiguous()


def _planted():
    """(pred, gt, planted classes): the ground truth's organs displaced, a few island voxels, and per planted class one 2 x 8 x 8 island in
    a corner of the volume, far from every organ (organ centres lie in the middle 60 % of every axis)."""
    shape = (6, 64, 64)
    gt = label_volume(shape, np.random.default_rng(77), 8)
    pred = np.roll(gt, (0, 2, -1), (0, 1, 2))
    g = np.random.default_rng(78)
    isl = g.random(shape) < 0.003
    pred[isl] = g.integers(1, 9, int(isl.sum()))
    present = [k for k in range(1, 9) if (gt == k).sum() > 400]
    planted = present[:2]
    corners = [(slice(0, 2), slice(0, 8), slice(0, 8)), (slice(4, 6), slice(56, 64), slice(56, 64))]
    for k, c in zip(planted, corners):
        assert (pred[c] == 0).all()
        pred[c] = k
    return pred, gt, planted


def test_through_evaluate_volume():
    """Dice within 1e-12 and HD95 within 1e-9 (the bound test_metrics_gpu.py derives: both sides interpolate in fp64 between the square
    roots of the same two integers) of `calculate_metric_percase` on the scipy-post-processed prediction, on both metric paths."""
    from transception_amd.evaluate import PostProcess, calculate_metric_percase, evaluate_volume, inference
    pred, gt, planted = _planted()
    assert len(planted) == 2
    image = pred.astype(np.float32) / 8
    m = _Binned().to(DEV)
    post = PostProcess()
    want = [calculate_metric_percase(want_post(pred, 9, "largest", 0, 1) == k, gt == k) for k in range(1, 9)]
    raw = [calculate_metric_percase(pred == k, gt == k) for k in range(1, 9)]
    run = functools.partial(evaluate_volume, m, image, gt, 9, (64, 64), batch=4, with_hd95=True)
    dev = run(device_metrics=True, postprocess=post)
    host = run(device_metrics=False, postprocess=post)
    hostform = run(host_zoom=True, postprocess=post)                                # the prediction on the host: postprocess_host
    for k, (d, h, z, w, r) in enumerate(zip(dev, host, hostform, want, raw), start=1):
        print(f"class {k}: device {d!r} host {h!r} host form {z!r} scipy {w!r} without {r!r}")
    for got in (dev, host, hostform):
        assert len(got) == 8
        for (d, h), (wd, wh) in zip(got, want):
            assert abs(d - wd) <= 1e-12 and abs(h - wh) <= 1e-9
    for a, b in zip(dev, host):
        assert abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-9
    for dm in (True, False):
        plain = run(device_metrics=dm)
        assert run(device_metrics=dm, postprocess=None) == plain                     # bit-identical to the call without the argument
        for (d, h), (wd, wh) in zip(plain, raw):
            assert abs(d - wd) <= 1e-12 and abs(h - wh) <= 1e-9
        for k in planted:
            assert (dev if dm else host)[k - 1][1] < plain[k - 1][1], k             # the island was what the HD95 measured
    dice = evaluate_volume(m, image, gt, 9, (64, 64), batch=4, device_metrics=True, postprocess=post)
    assert max(abs(a - w[0]) for a, w in zip(dice, want)) <= 1e-12
    a = inference(m, [(image, gt, "case")], 9, 64, batch=4, device_metrics=True, postprocess=post)
    assert abs(a[0] - np.mean([w[0] for w in want])) <= 1e-12 and abs(a[1] - np.mean([w[1] for w in want])) <= 1e-9


def test_bad_arguments_raise_without_launching():
    from transception_amd._lib import TC_CC_LARGEST, TC_CC_MIN_VOXELS, TcError, lib
    from transception_amd.evaluate import PostProcess, component_roots, component_sizes, postprocess_device
    L, stream = lib(), torch.cuda.current_stream().cuda_stream
    shape = (2, 8, 8)
    lab = torch.ones(shape, dtype=torch.uint8, device=DEV)
    root = torch.full(shape, 55, dtype=torch.int32, device=DEV)
    size = torch.full(shape, 66, dtype=torch.int32, device=DEV)
    best = torch.full((16, 2), 77, dtype=torch.int64, device=DEV)
    out = torch.full(shape, 88, dtype=torch.uint8, device=DEV)
    l, r, s, b, o = lab.data_ptr(), root.data_ptr(), size.data_ptr(), best.data_ptr(), out.data_ptr()
    bad = [
        lambda: L.tc_cc_label(l, r, 2, 8, 8, 1, 1, stream),                          # classes outside 2..16
        lambda: L.tc_cc_label(l, r, 2, 8, 8, 17, 1, stream),
        lambda: L.tc_cc_label(l, r, 2, 8, 8, 9, 2, stream),                          # connectivity 2
        lambda: L.tc_cc_label(l, r, 2, 8, 8, 9, 0, stream),
        lambda: L.tc_cc_label(l, r, 2049, 8, 8, 9, 1, stream),                       # D = 2049
        lambda: L.tc_cc_label(l, r, 2, 0, 8, 9, 1, stream),
        lambda: L.tc_cc_label(l, r, 2048, 1024, 1024, 9, 1, stream),                 # 2^31 voxels
        lambda: L.tc_cc_label(None, r, 2, 8, 8, 9, 1, stream),
        lambda: L.tc_cc_label(l, None, 2, 8, 8, 9, 1, stream),
        lambda: L.tc_cc_sizes(l, r, s, b, 2, 8, 8, 1, stream),
        lambda: L.tc_cc_sizes(l, r, s, b, 2, 8, 8, 17, stream),
        lambda: L.tc_cc_sizes(l, r, s, b, 2049, 8, 8, 9, stream),
        lambda: L.tc_cc_sizes(None, r, s, b, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_sizes(l, None, s, b, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_sizes(l, r, None, b, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_sizes(l, r, s, None, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_keep(l, r, s, b, o, TC_CC_LARGEST, 0, 2, 8, 8, 17, stream),
        lambda: L.tc_cc_keep(l, r, s, b, o, TC_CC_LARGEST, 0, 2, 8, 2049, 9, stream),
        lambda: L.tc_cc_keep(l, r, s, b, o, 2, 5, 2, 8, 8, 9, stream),               # no such mode
        lambda: L.tc_cc_keep(l, r, s, b, o, TC_CC_MIN_VOXELS, 0, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_keep(None, r, s, b, o, TC_CC_LARGEST, 0, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_keep(l, None, s, b, o, TC_CC_LARGEST, 0, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_keep(l, r, None, b, o, TC_CC_LARGEST, 0, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_keep(l, r, s, None, o, TC_CC_LARGEST, 0, 2, 8, 8, 9, stream),
        lambda: L.tc_cc_keep(l, r, s, b, None, TC_CC_LARGEST, 0, 2, 8, 8, 9, stream),
        lambda: component_roots(lab, 1),                                             # the same through the host interface
        lambda: component_roots(lab, 17),
        lambda: component_roots(lab, 9, connectivity=2),
        lambda: component_sizes(lab, root, 17),
        lambda: postprocess_device(lab, 1),
        lambda: postprocess_device(lab, 17, PostProcess("min_voxels", 3)),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(TcError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    torch.cuda.synchronize()
    assert int((lab != 1).sum()) == 0 and int((root != 55).sum()) == 0 and int((size != 66).sum()) == 0      # nothing ran
    assert int((best != 77).sum()) == 0 and int((out != 88).sum()) == 0
    cpu = torch.ones(shape, dtype=torch.uint8)
    for call in (lambda: component_roots(cpu, 9), lambda: component_sizes(cpu, root, 9), lambda: component_sizes(lab, root.cpu(), 9),
                 lambda: postprocess_device(cpu, 9)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError):
        component_roots(lab.int(), 9)
    with pytest.raises(ValueError):
        component_roots(torch.ones((2, 2, 2, 2), dtype=torch.uint8, device=DEV), 9)

"""The line passes of the distance transform (csrc/metrics.hip) at every tile width and on both sides of every boundary of the tile rule:
the widest of 32, 16, 8 lines per tile whose [L][TX] tile is at most 64 KB, else 8 -- int32 maps switch after L = 512 and 1024, float64
maps after 256 and 512.  Where the tile plus its flags exceed 64 KB (int32: L = 512, 1024, 2048; float64: L = 256, 512 and from 1024) the
launch raises the dynamic LDS limit first.

Surface maps are built directly: a handful of voxels of class 1 with both ends of the long axis among them, class 2 on one full row,
class 3 one voxel in the far corner (every scan runs the whole line), class 4 absent.  Against scipy.ndimage.distance_transform_edt:
the int32 map exactly, the float64 maps within 1e-12 relative element by element (the bound of test_weighted_distance_maps_against_scipy;
on these 2-D shapes a brute-force minimum over the sources differs from scipy's squared transform by at most 2.3e-16 relative)."""
import numpy as np
import pytest

from metrics_util import dev

pytestmark = pytest.mark.gpu

Y_SHAPES = [(L, 44) for L in (256, 257, 512, 513, 1024, 1025, 2048)]      # true 2-D: the y pass along L; 44 leaves a part tile at every width
Z_SHAPES = [(L, 2, 22) for L in (513, 1025)]                              # the z pass along L with inner = 44; the y pass over L slices of 2 rows
SPACINGS = {2: [(0.8, 1.25), (3.0, 0.7)], 3: [(0.8, 2.0, 1.25), (3.0, 0.5, 0.7)]}


def _surface_map(shape):
    L = shape[0]
    surf = np.zeros(shape, np.uint8)
    flat = surf.reshape(L, 44)                                            # [L][44] either way: sources in a few slices only
    for i, x in ((0, 3), (L - 1, 40), (L // 2, 17), (L // 3, 43), (L // 3 + 1, 0), (5, 21)):
        flat[i, x] = 1
    flat[7, :] = 2
    flat[L - 1, 43] = 3
    return surf


@pytest.mark.parametrize("shape", Y_SHAPES + Z_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_line_passes_at_every_tile_width(shape):
    from scipy.ndimage import distance_transform_edt
    from transception_amd._lib import TC_METRIC_NO_SOURCE
    from transception_amd.evaluate import edt_squared
    surf_h = _surface_map(shape)
    surf = dev(surf_h)
    for k in (1, 2, 3):
        d2i = edt_squared(surf, k).cpu().numpy()
        assert d2i.dtype == np.int32 and d2i.shape == shape
        np.testing.assert_array_equal(d2i, np.rint(distance_transform_edt(surf_h != k) ** 2).astype(np.int64))
        unit = edt_squared(surf, k, voxelspacing=1.0).cpu().numpy()
        assert unit.dtype == np.float64
        np.testing.assert_array_equal(unit, d2i.astype(np.float64))     # sums of squared integers are exact in fp64
        for s in SPACINGS[len(shape)]:
            d2 = edt_squared(surf, k, voxelspacing=s).cpu().numpy()
            want = distance_transform_edt(surf_h != k, sampling=s) ** 2
            err = np.abs(d2 - want)
            print(f"{shape} class {k} spacing {s}: largest relative difference from scipy {float((err / np.maximum(want, 1e-300)).max()):.3e}")
            assert (err <= 1e-12 * want).all(), (k, s)
    assert not (surf_h == 4).any()
    np.testing.assert_array_equal(edt_squared(surf, 4).cpu().numpy(), np.full(shape, TC_METRIC_NO_SOURCE, np.int32))
    for s in SPACINGS[len(shape)] + [1.0]:
        assert np.isposinf(edt_squared(surf, 4, voxelspacing=s).cpu().numpy()).all()

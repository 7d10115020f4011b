"""Seeded masks and label volumes shared by the device-metric tests (test_metrics_gpu.py, test_metrics_spacing_gpu.py, test_metrics_tile_gpu.py)."""
import numpy as np
import torch

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ellipsoid(shape, centre, radii, g=None, rough=0.0):
    """Boolean ellipsoid; `rough` perturbs the shell voxel by voxel (seeded)."""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    r2 = sum(((x - c) / r) ** 2 for x, c, r in zip(grids, centre, radii))
    if rough:
        r2 = r2 + g.uniform(-rough, rough, shape)
    return r2 < 1.0


def mask_pairs(seed, single_voxel, single_partner_centre):
    """(name, a, b) mask pairs; `single_voxel` is the one voxel of the "single-voxel" pair's first mask in a [4,9,9] array and
    `single_partner_centre` the centre of the ellipsoid it is compared with."""
    g = np.random.default_rng(seed)
    pairs = []
    for shape in [(3, 8, 8), (5, 12, 10), (8, 20, 24), (12, 30, 30)]:                          # ellipsoids with a roughened shell
        c = [(n - 1) / 2 for n in shape]
        a = ellipsoid(shape, [v + g.uniform(-1, 1) for v in c], [max(1.2, n / 3.2) for n in shape], g, 0.35)
        b = ellipsoid(shape, [v + g.uniform(-1.5, 1.5) for v in c], [max(1.2, n / 3.6) for n in shape], g, 0.35)
        pairs.append((f"rough{shape}", a, b))
    shape = (6, 16, 14)                                                                         # touching the array border
    pairs.append(("border", ellipsoid(shape, (0, 2, 3), (3, 6, 6)), ellipsoid(shape, (5, 13, 12), (4, 7, 5), g, 0.3)))
    pairs.append(("border-all", np.ones(shape, bool), ellipsoid(shape, (2, 8, 7), (2.5, 5, 4))))
    pairs.append(("one-slice", ellipsoid((1, 14, 12), (0, 6, 5), (1, 4, 4)), ellipsoid((1, 14, 12), (0, 8, 6), (1, 5, 3), g, 0.3)))
    single = np.zeros((4, 9, 9), bool)
    single[single_voxel] = True
    pairs.append(("single-voxel", single, ellipsoid((4, 9, 9), single_partner_centre, (1.5, 3, 2.5))))
    a = np.zeros((7, 10, 11), bool)
    b = np.zeros((7, 10, 11), bool)
    a[:2, :3, :3] = True
    b[-2:, -3:, -2:] = True
    pairs.append(("disjoint-corners", a, b))
    pairs.append(("2-d", ellipsoid((20, 26), (9, 12), (6, 8), g, 0.3), ellipsoid((20, 26), (11, 13), (7, 6), g, 0.3)))
    pairs.append(("2-d-border", ellipsoid((9, 70), (0, 10), (4, 9)), ellipsoid((9, 70), (8, 60), (5, 12))))
    return pairs


def label_volume(shape, g, n_organs, skip=()):
    """Seeded uint8 label volume: overlapping roughened ellipsoids, later labels painted over earlier ones.  A skipped organ draws the
    same random numbers, so two volumes from one seed differ only in the organs skipped."""
    lab = np.zeros(shape, np.uint8)
    for k in range(1, n_organs + 1):
        c = [g.uniform(0.2 * n, 0.8 * n) for n in shape]
        r = [g.uniform(0.08 * n, 0.22 * n) + 1.0 for n in shape]
        m = ellipsoid(shape, c, r, g, 0.25)
        if k not in skip:
            lab[m] = k
    return lab

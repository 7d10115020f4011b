"""References and seeded volumes shared by the post-processing tests (test_postprocess_gpu.py, test_postprocess_host.py): connected
components from scipy.ndimage.label plus numpy, and from a pure-Python flood fill -- never from the code under test."""
import numpy as np

from metrics_util import label_volume


def structure(ndim, connectivity):
    from scipy.ndimage import generate_binary_structure
    return generate_binary_structure(ndim, 1 if connectivity == 1 else ndim)


def scipy_components(lab, classes, connectivity):
    """[(k, comp, ncomp)] for every class 1..classes-1 that has a voxel: scipy's numbering, raster order of the first voxel."""
    from scipy.ndimage import label
    out = []
    for k in range(1, classes):
        comp, ncomp = label(lab == k, structure=structure(lab.ndim, connectivity))
        if ncomp:
            out.append((k, comp, ncomp))
    return out


def first_voxels(comp, ncomp):
    """[ncomp + 1]: the minimum flat index of every scipy label (entry 0: of the voxels outside the class)."""
    first = np.full(ncomp + 1, comp.size, np.int64)
    np.minimum.at(first, comp.ravel(), np.arange(comp.size, dtype=np.int64))
    return first


def want_root(lab, classes, connectivity):
    """int32 map: per component the minimum flat index, -1 for labels 0 and >= classes."""
    root = np.full(lab.shape, -1, np.int32)
    for _, comp, ncomp in scipy_components(lab, classes, connectivity):
        root[comp > 0] = first_voxels(comp, ncomp)[comp[comp > 0]]
    return root


def want_sizes_best(lab, classes, connectivity):
    """(size, best): the voxel count at every root (np.bincount of scipy's labels) and 0 elsewhere; per class (voxels, root) of the
    component np.argmax picks, (0, -1) for an absent class and for class 0."""
    size = np.zeros(lab.size, np.int32)
    best = np.tile(np.array([0, -1], np.int64), (classes, 1))
    for k, comp, ncomp in scipy_components(lab, classes, connectivity):
        counts = np.bincount(comp.ravel())[1:]
        firsts = first_voxels(comp, ncomp)[1:]
        size[firsts] = counts
        best[k] = (counts[np.argmax(counts)], firsts[np.argmax(counts)])
    return size.reshape(lab.shape), best


def want_post(lab, classes, mode, min_voxels, connectivity):
    """The post-processed volume, built from scipy's labels."""
    out = lab.copy()
    for k, comp, ncomp in scipy_components(lab, classes, connectivity):
        counts = np.bincount(comp.ravel())
        if mode == "largest":
            drop = (comp > 0) & (comp != 1 + np.argmax(counts[1:]))
        else:
            drop = (comp > 0) & (counts[comp] < min_voxels)
        out[drop] = 0
    return out


def organs_with_islands(shape, seed, fraction=0.02, n_organs=8, max_label=8):
    """`metrics_util.label_volume` organs plus `fraction` seeded random island voxels of random classes 1..max_label."""
    g = np.random.default_rng(seed)
    lab = label_volume(shape, g, n_organs)
    islands = g.random(shape) < fraction
    lab[islands] = g.integers(1, max_label + 1, int(islands.sum()))
    return lab


def tie_volume():
    """Class 1: two components of 6 voxels each (the first in raster order must win) and one of 5; class 2: one of 4 and a larger one
    later in raster order; class 3 absent."""
    lab = np.zeros((3, 8, 9), np.uint8)
    lab[0, 1, 1:7] = 1
    lab[1, 4:6, 2:5] = 1
    lab[2, 7, 0:5] = 1
    lab[0, 5, 5:9] = 2
    lab[2, 2:4, 5:9] = 2
    return lab


def flood_fill_post(lab, classes, mode, min_voxels, connectivity):
    """Pure Python: components by flood fill in raster order of their first voxel; the first largest one wins."""
    shape = (1,) * (3 - lab.ndim) + lab.shape
    l = lab.reshape(shape)
    D, H, W = shape
    offs = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) != (0, 0, 0) and (connectivity == 3 or abs(dz) + abs(dy) + abs(dx) == 1)]
    seen = np.zeros(shape, bool)
    comps = {}
    for z in range(D):
        for y in range(H):
            for x in range(W):
                k = int(l[z, y, x])
                if seen[z, y, x] or not 1 <= k < classes:
                    continue
                seen[z, y, x] = True
                stack, members = [(z, y, x)], []
                while stack:
                    p = stack.pop()
                    members.append(p)
                    for d in offs:
                        q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
                        if 0 <= q[0] < D and 0 <= q[1] < H and 0 <= q[2] < W and not seen[q] and l[q] == k:
                            seen[q] = True
                            stack.append(q)
                comps.setdefault(k, []).append(members)
    out = l.copy()
    for k, cs in comps.items():
        if mode == "largest":
            biggest = max(len(c) for c in cs)
            keep = next(i for i, c in enumerate(cs) if len(c) == biggest)
            dropped = [c for i, c in enumerate(cs) if i != keep]
        else:
            dropped = [c for c in cs if len(c) < min_voxels]
        for c in dropped:
            for p in c:
                out[p] = 0
    return out.reshape(lab.shape)

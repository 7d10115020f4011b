"""Brute-force reference of the directed surface statistics (include/transception_surface.h), independent of transception_amd.evaluate and of
scipy: surfaces by the face-neighbour definition, every surface-to-surface squared distance by exhaustive search, math.fsum for the sums.
Quadratic in the number of surface voxels: for the small shapes of tests/test_surface_host.py and tests/test_surface_gpu.py only."""
import math

import numpy as np


def surface(mask):
    """Voxels of the boolean mask ([D,H,W] or [H,W]) with at least one face neighbour (6 in 3-D, 4 in 2-D) outside the mask, the outside of
    the array counting as outside the mask."""
    m = np.asarray(mask, bool)
    padded = np.pad(m, 1)
    inner = m.copy()
    for axis in range(m.ndim):
        for shift in (-1, 1):
            inner &= np.roll(padded, shift, axis=axis)[(slice(1, -1),) * m.ndim]
    return m & ~inner


def directed_d2(src, dst, spacing=None, chunk=512):
    """For every voxel of the boolean map `src`, in raster order, the smallest squared distance to a voxel of `dst`, over ALL of them:
    int64 with unit spacing; with `spacing` (one float per axis) float64, summed over the axes in axis order as (s_a (i_a - j_a))^2.
    Empty when either map is."""
    a, b = np.argwhere(src), np.argwhere(dst)
    if len(a) == 0 or len(b) == 0:
        return np.zeros(0, np.int64 if spacing is None else np.float64)
    out = []
    for i in range(0, len(a), chunk):
        diff = a[i:i + chunk, None, :] - b[None, :, :]
        d2 = None
        for axis in range(diff.shape[-1]):
            term = diff[..., axis] ** 2 if spacing is None else (float(spacing[axis]) * diff[..., axis]) ** 2
            d2 = term if d2 is None else d2 + term
        out.append(d2.min(axis=1))
    return np.concatenate(out)


def record(d2, tol2):
    """(n, sum, within, max) of one direction; max is an int for integer squared distances, else a float; an empty direction is all zero."""
    if len(d2) == 0:
        return (0, 0.0, 0, 0)
    root = [math.sqrt(float(v)) for v in d2.tolist()]
    mx = d2.max()
    return (len(root), math.fsum(root), sum(float(v) <= tol2 for v in d2.tolist()), int(mx) if d2.dtype.kind == "i" else float(mx))


def records(pred, gt, spacing=None, tol2=1.0):
    """((n, sum, within, max) from the surface of `pred` to the surface of `gt`, the same in the other direction) of two boolean masks."""
    sp, sg = surface(pred), surface(gt)
    return record(directed_d2(sp, sg, spacing), tol2), record(directed_d2(sg, sp, spacing), tol2)


def all_d2(pred, gt, spacing=None):
    """Every squared distance of both directions, pooled (for a test that has to keep a tolerance away from all of them)."""
    sp, sg = surface(pred), surface(gt)
    return np.concatenate([directed_d2(sp, sg, spacing).astype(np.float64), directed_d2(sg, sp, spacing).astype(np.float64)])


def metrics(rec):
    """asd_pred, asd_gt, assd (medpy: the mean of the two directed means), nsd and hd from the two records of non-empty surfaces."""
    (n0, s0, w0, m0), (n1, s1, w1, m1) = rec
    asd_pred, asd_gt = s0 / n0, s1 / n1
    return {"asd_pred": asd_pred, "asd_gt": asd_gt, "assd": (asd_pred + asd_gt) / 2, "nsd": (w0 + w1) / (n0 + n1), "hd": math.sqrt(max(m0, m1))}


def sum_bound(n, total):
    """|sum - fsum| a sum of n correctly rounded square roots may have, in any order: each root within an ulp (2^-52 relative), n
    non-negative terms within (n - 1) 2^-53 relative of their exact sum."""
    return (n + 1) * 2.0 ** -52 * total

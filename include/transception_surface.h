/*
 * transception_surface.h -- directed surface-distance statistics of one class: what ASD, ASSD, the surface Dice (NSD) and the full
 * Hausdorff distance are formed from.  C ABI of libtransception_hip.so (MI355X / gfx950; csrc/surface.hip).
 *
 * A header of its own: every entry of transception_hip.h names the reference call sites it replaces, and this replaces none -- the
 * reference reports Dice and HD95 only (utils.py:50-60).  Self-contained (no #include); the conventions are those of transception_hip.h:
 * device pointers owned by the caller, `stream` a hipStream_t passed as void*, nothing allocated, freed or synchronised, every call
 * asynchronous on `stream`.  An unmarked entry returns a status with the values of transception_hip.h: 0 (TC_OK), -1 (TC_ERR_ARG),
 * -2 (TC_ERR_LAUNCH); an entry marked TC_QUERY returns a value instead.  A refused call (-1) launches nothing.
 *
 * Definitions, for class k of two label volumes [D,H,W]:
 *   S_P = { v : surf_pred[v] == k },  S_G = { v : surf_gt[v] == k }: the uint8 surface maps of tc_metric_surfaces (connectivity 1);
 *   d2_pred[v], d2_gt[v]: the squared distance of v to S_P / to S_G -- the maps of tc_metric_edt (int32, unit spacing) or of
 *     tc_metric_edt_f64 (float64, with a voxel spacing) for this k;
 *   direction 0 is the multiset { d2_gt[v]   : v in S_P }  (from the prediction's surface to the ground truth's),
 *   direction 1 is the multiset { d2_pred[v] : v in S_G }  (from the ground truth's surface to the prediction's).
 *   Members whose distance is to an empty surface are left out, as tc_metric_hist and tc_metric_select_f64 leave them out:
 *   >= TC_METRIC_NO_SOURCE (1 << 28) in the int32 maps, +inf in the float64 maps.
 * Per direction i four values:
 *   n_i      the number of members,
 *   sum_i    the sum of sqrt(d2) over the members, in fp64 (each square root correctly rounded),
 *   within_i the number of members with (double)d2 <= tol2,
 *   max_i    the largest d2 (0 for an empty direction).
 * The host forms (evaluate.surface_metrics_device):
 *   asd_pred = sum_0 / n_0,   asd_gt = sum_1 / n_1        medpy.metric.binary.asd(result, reference) and asd(reference, result)
 *   assd     = (asd_pred + asd_gt) / 2                    medpy's assd: the mean of the two directed means, NOT the pooled mean
 *   nsd      = (within_0 + within_1) / (n_0 + n_1)        surface Dice at tolerance tau, the count-based form
 *   hd       = sqrt(max(max_0, max_1))                    the full Hausdorff distance
 * The tolerance is tested on SQUARED distances: tol2 = tau * tau is formed once, in fp64, by the caller, and a member counts when
 * (double)d2 <= tol2.  With unit spacing d2 is an exact integer and so is the count.  This differs from sqrt(d2) <= tau only where a
 * rounding sits on the boundary (tau * tau or the square root rounded across it).
 *
 * tc_surface_stats / tc_surface_stats_f64: `out` is [ncls][2][4] slots of 8 bytes; a call OVERWRITES the eight slots of class k and touches
 *   no other: [direction][n, sum, within, max].  n and within are long long; sum is the bits of a double; max is a long long squared
 *   distance (tc_surface_stats) or the bits of a double (tc_surface_stats_f64).  An empty direction is (0, 0.0, 0, 0): all bits zero.
 *   `work` is TC_SURFACE_WORK_BYTES of scratch, 8-byte aligned; it needs no initialisation (every slot that is read was written by the
 *   same call) and holds nothing afterwards.  The surface maps may start at any address (they are read in 16-byte pieces from the first
 *   16-byte boundary on, the bytes before and after one by one); the distance maps are aligned to their element and are read only at
 *   surface voxels.  The inputs are not written.
 *   Deterministic: a fixed grid, every thread takes its elements in increasing order, a fixed reduction tree inside the workgroup, one
 *   slot of `work` per workgroup, and a second launch of one workgroup that adds the slots in a fixed order.  No floating-point atomics:
 *   the sums and the fp64 maximum repeat to the bit, the counts and the int32 maximum are exact.  (Which thread takes which voxel follows
 *   the surface maps' addresses modulo 16: at another alignment the same square roots are added in another order, and a sum may differ
 *   in its last bits.)
 *   -1: a NULL pointer (surf_pred, surf_gt, d2_pred, d2_gt, work, out); D, H or W outside 1..2048; D H W >= 2^31 - 1; ncls outside 1..16;
 *       k outside 1..ncls-1; tol2 negative, infinite or a NaN.
 */
#ifndef TRANSCEPTION_SURFACE_H
#define TRANSCEPTION_SURFACE_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_SURFACE_ABI_VERSION 1
#define TC_SURFACE_WORK_BYTES 131072      /* 2048 workgroups x 8 slots x 8 bytes */
#ifndef TC_QUERY
#define TC_QUERY
#endif

/* identity of this part of the library: bumped on any change to a signature below */
TC_QUERY int tc_surface_abi_version(void);
int tc_surface_stats    (const unsigned char* surf_pred, const unsigned char* surf_gt, const int*    d2_pred, const int*    d2_gt,
                         int k, int ncls, int D, int H, int W, double tol2, void* work, long long* out, void* stream);
int tc_surface_stats_f64(const unsigned char* surf_pred, const unsigned char* surf_gt, const double* d2_pred, const double* d2_gt,
                         int k, int ncls, int D, int H, int W, double tol2, void* work, long long* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_SURFACE_H */

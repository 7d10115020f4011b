/*
 * transception_uncertainty.h -- per-pixel uncertainty maps (predictive entropy, maximum-probability confidence, mutual information between
 * views) and calibration statistics (reliability table, NLL, Brier score) of class scores, one streaming pass each.
 * C ABI of libtransception_hip.so (MI355X / gfx950; csrc/uncertainty.hip).
 *
 * A header of its own: every entry of transception_hip.h names the reference call sites it replaces, and these replace none -- the
 * reference reduces its class scores to an argmax and reports Dice and HD95 only.  Self-contained (no #include); the conventions are those
 * of transception_hip.h: device pointers owned by the caller, `stream` a hipStream_t passed as void*, nothing allocated, freed or
 * synchronised, every call asynchronous on `stream`.  An unmarked entry returns a status with the values of transception_hip.h: 0 (TC_OK),
 * -1 (TC_ERR_ARG), -2 (TC_ERR_LAUNCH); an entry marked TC_QUERY returns a value instead.  A refused call (-1) launches nothing.
 *
 * Two kinds of input (`kind`):
 *   TC_UNCERT_LOGITS (0): `scores` is [N,ncls,H,W], contiguous, in `dtype` (TC_F32 0, TC_BF16 1, TC_F16 2 of transception_hip.h).  Per pixel,
 *     in fp32, exactly as tc_tta_accumulate does it: m = max_k l_k, e_k = expf(l_k - m), s = e_0 + e_1 + ... in class order, p_k = e_k / s.
 *   TC_UNCERT_PROB_SUMS (1): `scores` is fp32 [N,ncls,H,W] holding the sums t_k of V probability vectors -- the accumulator of
 *     tc_tta_accumulate, or its bilinear resampling (tc_resample_scores).  `dtype` must be TC_F32.  p_k = t_k * inv_views: one fp32 multiply,
 *     inv_views = (float)(1.0 / V) formed by the caller.
 * Per pixel, all in fp32:
 *   conf  = max_k p_k;  pred = the first maximum (torch.argmax, tc_argmax_counts).
 *   h     = min(1, max(0, H / logf((float)ncls))): the entropy normalised by that of the uniform distribution; h = 0 for ncls == 1.
 *             LOGITS:    H = logf(s) - (sum_k e_k (l_k - m)) / s, in class order: 0 log 0 is never formed.
 *             PROB_SUMS: H = -sum_k p_k logf(p_k), in class order, a term with p_k <= 0 counted as 0.
 *   nll   of a label y:  LOGITS: logf(s) - (l_y - m);  PROB_SUMS: -logf(fmaxf(p_y, FLT_MIN)).
 *   brier = sum_k (p_k - [k == y])^2, in class order.
 *
 * tc_uncert_maps: three nullable fp32 [N,H,W] outputs and one nullable uint8 [N,H,W] output, at least one of them given:
 *     entropy = h,  confidence = conf,  pred as above,
 *     mutual_info = max(0, h - view_entropy_sum[n,y,x] * inv_views), given only together with `view_entropy_sum`: fp32 [N,H,W], the sum over
 *     the views of each view's own h, already at the un-transformed position.  (mutual_info == view_entropy_sum, in place, is allowed.)
 *   One thread owns a few consecutive pixels in all their classes.  `scores` may start at any address aligned to its element: where the
 *   plane H * W is a multiple of the elements in 16 bytes, every class plane is read in 16-byte pieces from the first 16-byte boundary on
 *   and the elements before and after it one by one (otherwise all one by one); an output whose pieces fall on a 16-byte (pred: one piece's
 *   bytes) boundary is stored in pieces.  No atomics, no LDS; every output element has one owner and a run repeats to the bit.
 *   A NULL output is never written.  inv_views is read for PROB_SUMS and for mutual_info.
 *   -1: scores NULL; every output NULL; mutual_info without view_entropy_sum or the reverse; an output equal to `scores`; kind or dtype
 *       unknown; PROB_SUMS with a 16-bit dtype; inv_views not in (0, 1] (a NaN included); ncls outside 1..16; N, H or W <= 0;
 *       N * ncls * H * W >= 2^31.
 *
 * tc_calib_stats: `labels` is uint8 [N,H,W]; `bins` in 1..32; `flags`: bit 0 TC_CALIB_FOREGROUND.  A pixel is COUNTED if labels != ignore_index
 *   and labels < ncls, and under TC_CALIB_FOREGROUND also labels > 0 || pred > 0.  ignore_index outside 0..255 means none.
 *   `out` is OVERWRITTEN: tc_calib_out_slots(bins, ncls) = 3 bins + 4 + 3 ncls slots of 8 bytes,
 *     [bins][3]  (n_b, sum of conf in units of 2^-32 as int64, n_b correct) of the counted pixels of confidence bin
 *                b = min(bins - 1, (int)(conf * (float)bins)), the product in fp32; a pixel adds (long long)(conf * 4294967296.0f) to the sum:
 *                exact for conf >= 2^-8, i.e. always for the maximum of at most 16 probabilities that sum to about 1;
 *     [4]        (n, sum of nll as the bits of a double, sum of brier as the bits of a double, n correct), y = the pixel's label;
 *     [ncls][3]  per PREDICTED class among the counted pixels: (n_k, sum of h in units of 2^-32 as int64 by the same truncation, n_k correct).
 *   "correct" is pred == label.  The counts and the two fixed-point sums are integers, so the order of arrival cannot change them: they are
 *   collected with integer atomics in LDS and leave a workgroup as one set of slots in `work`.  The two fp64 sums use no atomics: a fixed
 *   grid, every thread takes its groups of pixels in increasing order, a fixed butterfly inside a wave, the waves of a workgroup added in
 *   order, one slot per workgroup in `work`, and a second launch of one workgroup that adds the workgroups' slots in a fixed order.  A run
 *   repeats to the bit.  (Which thread takes which pixel follows the address of `scores` modulo 16: at another alignment the same terms
 *   are added in another order, and an fp64 sum may differ in its last bits.)
 *   `work` is tc_calib_work_bytes(bins, ncls) of scratch, 8-byte aligned; it needs no initialisation (every slot that is read was written by
 *   the same call) and holds nothing afterwards.  tc_calib_work_bytes is 0, and tc_calib_out_slots is 0, outside the limits of bins and ncls.
 *   -1: as tc_uncert_maps for scores, kind, dtype, inv_views, ncls, N, H, W; labels, work or out NULL; bins outside 1..32; an unknown flag bit.
 */
#ifndef TRANSCEPTION_UNCERTAINTY_H
#define TRANSCEPTION_UNCERTAINTY_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_UNCERT_ABI_VERSION 1
#define TC_UNCERT_LOGITS 0
#define TC_UNCERT_PROB_SUMS 1
#define TC_CALIB_FOREGROUND 1
#define TC_CALIB_MAX_BINS 32
#ifndef TC_QUERY
#define TC_QUERY
#endif

/* identity of this part of the library: bumped on any change to a signature below */
TC_QUERY int tc_uncert_abi_version(void);
TC_QUERY long long tc_calib_work_bytes(int bins, int ncls);
TC_QUERY int tc_calib_out_slots(int bins, int ncls);
int tc_uncert_maps(const void* scores, int dtype, int kind, float inv_views, const float* view_entropy_sum, float* entropy, float* confidence,
                   float* mutual_info, unsigned char* pred, int N, int ncls, int H, int W, void* stream);
int tc_calib_stats(const void* scores, int dtype, int kind, float inv_views, const unsigned char* labels, int ignore_index, int flags, int bins,
                   int N, int ncls, int H, int W, void* work, long long* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_UNCERTAINTY_H */

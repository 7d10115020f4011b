/*
 * transception_loss.h -- focal cross-entropy and Tversky overlap in the fused segmentation loss, C ABI of libtransception_hip.so
 * (MI355X / gfx950; csrc/train.hip).
 *
 * A header of its own: every entry of transception_hip.h names the reference call sites it replaces, and these replace none -- the
 * reference's loss is 0.4 CE + 0.6 Dice (trainer.py:141-143), which tc_seg_loss_* / tc_seg_loss_*_w of transception_hip.h compute.
 * Self-contained (no #include); the conventions are those of transception_hip.h: device pointers owned by the caller, `stream` a
 * hipStream_t passed as void*, nothing allocated, freed or synchronised, every call asynchronous on `stream`.  An unmarked entry returns a
 * status with the values of transception_hip.h: 0 (TC_OK), -1 (TC_ERR_ARG), -2 (TC_ERR_LAUNCH); an entry marked TC_QUERY returns a value
 * instead.  A refused call (-1) launches nothing.
 *
 * Definition.  Per pixel i with label y_i, softmax probabilities p_ik and counted_i = (y_i != ignore_index); every sum below runs over the
 * counted pixels only.
 *   q_i     = sum_{k != y_i} p_ik                    (1 - p_t as a sum of the OTHER classes' probabilities: no cancellation as p_t -> 1)
 *   FocalCE = sum_i w_ce[y_i] q_i^gamma (-log max(p_{i,y_i}, 1e-38)) / sum_i w_ce[y_i]
 *             gamma >= 0, finite; gamma = 0 is the class-weighted CE of tc_seg_loss_*_w.  The denominator is sum_k w_ce[k] Y_k, formed
 *             from the sums; a zero denominator gives 0 with a zero gradient, never NaN.
 *   Overlap, by `overlap`:
 *     TC_OVERLAP_DICE     sum_k w_dice[k] (1 - (2 I_k + eps) / (Z_k + Y_k + eps)) / ncls       the reference's term, as in tc_seg_loss_*_w
 *     TC_OVERLAP_TVERSKY  sum_k w_dice[k] (1 - T_k) / ncls,  T_k = (I_k + eps) / D_k,  D_k = (1 - alpha - beta) I_k + alpha P_k + beta Y_k + eps
 *                         alpha, beta >= 0, finite, alpha + beta > 0 (alpha weighs the false positives P_k - I_k, beta the false
 *                         negatives Y_k - I_k).  alpha = beta = 0.5 is the LINEAR Dice, not the reference's: that one has sum p^2 in
 *                         the denominator and 2 I + eps in the numerator.  alpha and beta are read only under TC_OVERLAP_TVERSKY.
 *     with I_k = sum_i p_ik [y_i = k], Y_k = sum_i [y_i = k], Z_k = sum_i p_ik^2, P_k = sum_i p_ik and eps = 1e-5.
 *   Loss    = w_ce FocalCE + w_dice Overlap.
 *
 * Sums vector: float[1 + 3 ncls], zeroed by the caller, accumulated by the forward (wave sums, then one atomic add per workgroup and
 * element), all-reduced by the caller across ranks as the one of tc_seg_loss_fwd is.  sums[0] = sum_i w_ce[y_i] q_i^gamma nll_i;
 * sums[1 + 3k] = I_k, sums[2 + 3k] = Y_k, sums[3 + 3k] = Z_k under TC_OVERLAP_DICE and P_k under TC_OVERLAP_TVERSKY.  I, Y, Z and P are
 * unweighted.  The fp32 Y_k are whole numbers: the CE denominator is exact while the global number of counted pixels stays below 2^24.
 *
 * Gradient (tc_seg_loss_bwd_ft), at a counted pixel with t = y_i, p = p_it and delta_k = [k = t]:
 *   m_i        = q^gamma (1 - gamma p log(max(p, 1e-38)) / q), which is q^(gamma - 1) (q - gamma p log p);  1 for gamma = 0;  0 for
 *                gamma > 0 and q = 0 (0^(gamma - 1) is never evaluated)
 *   g_ik       = ca_k delta_k + cb_k p_ik   TC_OVERLAP_DICE:     ca_k = -(w_dice / ncls) w_dice[k] 2 / (Z_k + Y_k + eps),
 *                                                                cb_k = +(w_dice / ncls) w_dice[k] 2 (2 I_k + eps) / (Z_k + Y_k + eps)^2
 *   g_ik       = ca_k delta_k + cb_k        TC_OVERLAP_TVERSKY:  ca_k = -(w_dice / ncls) w_dice[k] (D_k - (I_k + eps)(1 - alpha - beta)) / D_k^2,
 *                                                                cb_k = +(w_dice / ncls) w_dice[k] (I_k + eps) alpha / D_k^2
 *   dlogits_ik = gscale [ (w_ce / sum_k w_ce[k] Y_k) w_ce[t] m_i (p_ik - delta_k) + p_ik (g_ik - sum_j g_ij p_ij) ]
 *                (p_it - 1 is taken as -q_i).  gscale is multiplied by *gscale_dev when that pointer is not NULL.
 * The clamp at 1e-38 is not differentiated: at a pixel with p_t below it the gradient is the analytic one above, as in the plain and
 * class-weighted kernels (autograd through a clamp would give the CE term no gradient there).  In both directions log p_t is taken as
 * log1p(-q_i) where q_i < 1/4: p_t rounds to 1 in fp32 for q_i below 6e-8, where its logarithm is -q_i, not 0.
 * An ignored pixel's dlogits is WRITTEN as exact zeros in every class.  ca / cb are formed once per workgroup from `sums`; the per-pixel
 * part is one pass without atomics, so dlogits is the same bit for bit from launch to launch.
 *
 * Arguments, as for tc_seg_loss_*_w: weights float[2 * ncls] on the device, CE weights then overlap weights, NULL = all ones;
 * ignore_index a label value outside [0, ncls), or TC_IGNORE_NONE (transception_hip.h: -2^31) for none; ncls <= 16; dtype TC_F32 /
 * TC_BF16 / TC_F16 storage of logits and dlogits, fp32 arithmetic.  One pair of entries serves both layouts: ld = 0 is NCHW logits /
 * dlogits [B, ncls, HW] and prob (fp32 [B, ncls, HW]) is then required; ld >= ncls is token-major rows [B * HW, ld].  16-bit rows that
 * are 16-byte aligned and padded to a multiple of 8 elements are read and written as whole 16-byte pieces, the pad elements of dlogits
 * as zeros; every other pitch is accessed element by element, padding untouched.  prob == NULL on token-major rows: the forward writes no
 * map and the backward recomputes the softmax from `logits` (row pitch ldl) with the forward's operations in the forward's order.
 * -1: a NULL pointer where one is required, B, ncls or HW out of range, B * HW >= 2^31 - 1, a pitch below ncls, gamma < 0 or not finite,
 * an `overlap` that is neither constant, under TC_OVERLAP_TVERSKY a negative or non-finite alpha or beta or alpha + beta = 0, and an
 * ignore_index inside [0, ncls).
 * The scalars are kernel arguments: a captured launch keeps the values it was captured with.
 */
#ifndef TRANSCEPTION_LOSS_H
#define TRANSCEPTION_LOSS_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_LOSS_ABI_VERSION 1
#ifndef TC_QUERY
#define TC_QUERY
#endif

enum { TC_OVERLAP_DICE = 0, TC_OVERLAP_TVERSKY = 1 };

/* identity of this part of the library: bumped on any change to a signature below */
TC_QUERY int tc_loss_abi_version(void);
int tc_seg_loss_fwd_ft(const void* logits, int ld, const long long* labels, const float* weights, int ignore_index, float gamma, int overlap,
                       float* prob, float* sums, int B, int ncls, int HW, int dtype, void* stream);
/* out3 = {w_ce FocalCE + w_dice Overlap, FocalCE, Overlap} from the (all-reduced) sums, in double on the device */
int tc_seg_loss_value_ft(const float* sums, const float* weights, int ncls, double w_ce, double w_dice, int overlap, double alpha, double beta,
                         float* out3, void* stream);
int tc_seg_loss_bwd_ft(const float* prob, const void* logits, int ldl, const long long* labels, const float* weights, int ignore_index,
                       const float* sums, void* dlogits, int ld, int B, int ncls, int HW, float w_ce, float w_dice, float gamma, int overlap,
                       float alpha, float beta, float gscale, const float* gscale_dev, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_LOSS_H */

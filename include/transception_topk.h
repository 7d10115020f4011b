/*
 * transception_topk.h -- top-k (hard-pixel) cross-entropy in the fused segmentation loss, C ABI of libtransception_hip.so
 * (MI355X / gfx950; csrc/train.hip for the loss kernels, csrc/topk.hip for the select).
 *
 * A header of its own, as transception_loss.h is and for the same reason: these entries replace no reference call site.  The loss is the
 * "TopK" cross-entropy of nnU-Net (DC_and_topk_loss, k = 10 %), also known as online hard-example mining: the cross-entropy is the mean of
 * the k largest per-pixel terms only.  Self-contained (no #include); the conventions are those of transception_hip.h: device pointers owned
 * by the caller, `stream` a hipStream_t passed as void*, nothing allocated, freed or synchronised, every call asynchronous on `stream`.  An
 * unmarked entry returns 0 (TC_OK), -1 (TC_ERR_ARG) or -2 (TC_ERR_LAUNCH); an entry marked TC_QUERY returns a value instead.  A refused
 * call (-1) launches nothing.
 *
 * Definition.  Per pixel i with label y_i, v_i is that pixel's cross-entropy term exactly as tc_seg_loss_fwd_ft (transception_loss.h) forms
 * it: v_i = w_ce[y_i] q_i^gamma (-log max(p_t, 1e-38)); with gamma = 0 the class-weighted nll, with no weights the plain nll.  Counted
 * pixels are those with y_i != ignore_index.
 *   n      = number of counted pixels ON THIS RANK
 *   k      = max(1, min(n, ceil(frac n))), the product formed once in fp64, frac a double in (0, 1]
 *   t      = the k-th largest v_i -- exact: non-negative floats order like their bit patterns
 *   n_gt   = #{v_i > t},  n_eq = #{v_i == t},  S = sum_{v_i > t} v_i in fp64
 *   TopkCE = (S + (k - n_gt) t) / k         the mean of the k largest terms
 *   s_i    = 1 for v_i > t,  f = (k - n_gt) / n_eq for v_i == t,  0 below         the selection weight of a pixel
 *   CE     = (1 / world) sum_r TopkCE_r     across ranks the selection is per rank, as nnU-Net's is under DDP
 *   Loss   = w_ce CE + w_dice Overlap       Overlap (Dice or Tversky) as in transception_loss.h, untouched and global
 * Two things to know.  (1) Whatever class weights there are, the divisor is k, not sum w: frac = 1 with class weights is the mean of the
 * weighted terms, NOT torch's weighted mean (frac = 1 without weights is the plain CE).  (2) All pixels tied at the threshold share the
 * places left there equally (f), so the loss and its gradient are functions of the values alone; torch.topk picks among ties arbitrarily.
 * n = 0: CE = 0 with a zero gradient, never NaN.
 *
 * Gradient of the CE term at a counted pixel (tc_seg_loss_bwd_topk; the overlap part and every symbol as in transception_loss.h):
 *   (w_ce / (world k)) s_i w_ce[y_i] m_i (p_ik - delta_k)
 * The selection is not differentiated.  s_i is taken from the STORED value map against the stored t and f, not recomputed: forward and
 * backward agree on the selection by construction.  An ignored pixel's dlogits is written as exact zeros.
 *
 * Value map: float[B * HW], 4 bytes per pixel, written by tc_seg_loss_fwd_topk: v_i with the sign bit cleared at a counted pixel (a NaN
 * from overflowed fp16 logits keeps a defined place, above +inf), -1.0f at an ignored one.  A counted pixel whose label is outside
 * [0, ncls) has the value 0.
 *
 * State: double[8] in device memory.  [0] = frac, written by the CALLER and read on the device by tc_topk_select: a captured step follows
 * an annealed fraction without a new capture.  [1..7] are overwritten by tc_topk_select with n, k, n_gt, n_eq, t, S, f (the counts whole
 * numbers, exact in a double; t the float widened exactly; all seven are 0 when n = 0).  The fraction never passes through an argument, so
 * no entry can refuse it: the host side validates it (SegLoss, set_topk, TrainConfig: a finite number in (0, 1]), and a word on the device
 * that is not in (0, 1] cannot index out of range: k is clamped into [1, n] (a NaN gives k = 1).
 *
 * tc_topk_select: every entry of `values` with the sign bit set is not counted.  The select is a most-significant-digit-first radix select
 * over the uint32 patterns: four passes of one 8-bit digit, each an integer histogram (per wave aggregated, then LDS atomics, then one
 * global atomic per workgroup and used bin) and a one-workgroup scan; then S through one fp64 scratch slot per workgroup and a fixed-order
 * add.  Integer atomics only, passes separated by launch boundaries: 11 launches, results the same bit for bit from run to run.  It writes
 * sums[0] = (float)(TopkCE inv_world), so the sum all-reduce of the sums vector yields the global CE in sums[0].  `work` is
 * tc_topk_work_bytes() bytes, 8-byte aligned, cleared and overwritten by the entry itself: its contents before the call do not matter.
 *
 * tc_seg_loss_fwd_topk: the arguments of tc_seg_loss_fwd_ft and `values`.  prob and sums[1..] are what tc_seg_loss_fwd_ft leaves (same
 * operations in the same order; sums zeroed by the caller); sums[0] is left alone.  Both layouts, the 16-byte path of padded 16-bit rows
 * included.  tc_seg_loss_value_topk: tc_seg_loss_value_ft with CE = sums[0].  tc_seg_loss_bwd_topk: the arguments of tc_seg_loss_bwd_ft and
 * values, state, inv_world = 1 / world; one pass, dlogits written once.
 * -1: what transception_loss.h refuses, a NULL values / state / work, n_pix out of (0, 2^31 - 1), a misaligned work or state, and an
 * inv_world that is not in (0, 1].
 */
#ifndef TRANSCEPTION_TOPK_H
#define TRANSCEPTION_TOPK_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_TOPK_ABI_VERSION 1
#ifndef TC_QUERY
#define TC_QUERY
#endif

/* identity of this part of the library: bumped on any change to a signature below */
TC_QUERY int tc_topk_abi_version(void);
/* bytes of scratch tc_topk_select needs */
TC_QUERY long long tc_topk_work_bytes(void);
int tc_seg_loss_fwd_topk(const void* logits, int ld, const long long* labels, const float* weights, int ignore_index, float gamma, int overlap,
                         float* prob, float* sums, float* values, int B, int ncls, int HW, int dtype, void* stream);
int tc_topk_select(const float* values, long long n_pix, double* state, float* sums, double inv_world, void* work, void* stream);
/* out3 = {w_ce CE + w_dice Overlap, CE, Overlap} with CE = sums[0] from the (all-reduced) sums, in double on the device */
int tc_seg_loss_value_topk(const float* sums, const float* weights, int ncls, double w_ce, double w_dice, int overlap, double alpha, double beta,
                           float* out3, void* stream);
int tc_seg_loss_bwd_topk(const float* prob, const void* logits, int ldl, const long long* labels, const float* weights, int ignore_index,
                         const float* sums, void* dlogits, int ld, int B, int ncls, int HW, float w_ce, float w_dice, float gamma, int overlap,
                         float alpha, float beta, float gscale, const float* gscale_dev, const float* values, const double* state,
                         float inv_world, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_TOPK_H */

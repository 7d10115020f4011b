/*
 * transception_tta.h -- test-time augmentation: flip / transpose views of the input, their class probabilities averaged on the device.
 * C ABI of libtransception_hip.so (MI355X / gfx950; csrc/tta.hip).
 *
 * A header of its own: every entry of transception_hip.h names the reference call sites it replaces, and these replace none -- the
 * reference scores one forward pass per slice.  Self-contained (no #include); the conventions are those of transception_hip.h:
 * device pointers owned by the caller, `stream` a hipStream_t passed as void*, nothing allocated, freed or synchronised, every call
 * asynchronous on `stream`.  An unmarked entry returns a status with the values of transception_hip.h: 0 (TC_OK), -1 (TC_ERR_ARG),
 * -2 (TC_ERR_LAUNCH); an entry marked TC_QUERY returns a value instead.  A refused call (-1) launches nothing.
 *
 * A VIEW v in 0..7 is three bits: TC_TTA_FLIP_H rows reversed, TC_TTA_FLIP_W columns reversed, TC_TTA_TRANSPOSE transpose, applied
 * after the flips (H == W required).  In torch terms view_v(a) = a.flip(<dims chosen by bits 0, 1>), then .transpose(-2, -1) under bit 2:
 * the 8 symmetries of the square.  With fh(i) = H-1-i under bit 0 (else i) and fw(i) = W-1-i under bit 1 (else i), original position
 * (p, q) is found in the view at (y, x) = (fh(p), fw(q)) without the transpose and at (fw(q), fh(p)) with it.
 *
 * tc_tta_view: dst[n] = view_v((src[n] - mean) / stdv), fp32 [N,H,W] (view [N,W,H] = [N,H,W] under bit 2), out of place; the expression is
 *   tc_zoom_normalize's `(v - mean) / stdv`, so view 0 with (0.5, 0.5) is bit-identical to the host's (x - 0.5) / 0.5.
 *   -1: src or dst NULL, src == dst, N, H or W <= 0, N*H*W >= 2^31, view outside 0..7, view >= 4 with H != W, stdv == 0.
 * tc_tta_accumulate: `logits` is [N,ncls,H,W], contiguous, in `dtype` (TC_F32 0, TC_BF16 1, TC_F16 2 of transception_hip.h): the network's
 *   output for view_v of the input.  Per pixel (y, x) of the view, in fp32: m = max_k l_k, e_k = expf(l_k - m), s = e_0 + e_1 + ... in class
 *   order, p_k = e_k / s.  At the ORIGINAL position (p, q): t_k = p_k if `first`, else acc[n,k,p,q] + p_k  (acc: fp32 [N,ncls,H,W]).
 *     pred == NULL: acc[n,k,p,q] = t_k.  With `first` set acc is overwritten, never read: it needs no memset.
 *     pred != NULL: pred[n,p,q] = argmax_k t_k as uint8, the first maximum (torch.argmax, tc_argmax_counts); acc is NOT written and may
 *                   be NULL when `first` is set.  The last view of a set: the accumulator's final write and re-read are saved.
 *   Each accumulator element is owned by one thread: no atomics, views are added in launch order, a run repeats to the bit.
 *   -1: logits NULL; acc NULL unless first && pred; acc == logits; view outside 0..7; view >= 4 with H != W; ncls outside 1..16;
 *       N, H or W <= 0; N*ncls*H*W >= 2^31; an unknown dtype; first outside {0, 1}.
 */
#ifndef TRANSCEPTION_TTA_H
#define TRANSCEPTION_TTA_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_TTA_ABI_VERSION 1
#define TC_TTA_FLIP_H 1
#define TC_TTA_FLIP_W 2
#define TC_TTA_TRANSPOSE 4
#ifndef TC_QUERY
#define TC_QUERY
#endif

/* identity of this part of the library: bumped on any change to a signature below */
TC_QUERY int tc_tta_abi_version(void);
int tc_tta_view(const float* src, float* dst, int N, int H, int W, int view, float mean, float stdv, void* stream);
int tc_tta_accumulate(const void* logits, int dtype, float* acc, unsigned char* pred, int N, int ncls, int H, int W, int view, int first,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_TTA_H */

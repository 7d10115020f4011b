/*
 * transception_resample.h -- class scores resampled bilinearly to another size, and their argmax, in one pass.
 * C ABI of libtransception_hip.so (MI355X / gfx950; csrc/resample.hip).
 *
 * A header of its own: every entry of transception_hip.h names the reference call sites it replaces, and this replaces none -- the
 * reference takes the argmax at the network size and zooms the labels (utils.py:83-84); the score resampling stands there as a
 * commented-out line (utils.py:81, trainer.py:140).  Self-contained (no #include); the conventions are those of transception_hip.h:
 * device pointers owned by the caller, `stream` a hipStream_t passed as void*, nothing allocated, freed or synchronised, every call
 * asynchronous on `stream`.  An unmarked entry returns a status with the values of transception_hip.h: 0 (TC_OK), -1 (TC_ERR_ARG),
 * -2 (TC_ERR_LAUNCH); an entry marked TC_QUERY returns a value instead.  A refused call (-1) launches nothing.
 *
 * tc_resample_scores: `src` is [N,ncls,h,w], contiguous, in `dtype` (TC_F32 0, TC_BF16 1, TC_F16 2 of transception_hip.h); a 16-bit
 *   value is widened to fp32 exactly.  `scores` (nullable) is fp32 [N,ncls,H,W], `pred` (nullable) uint8 [N,H,W]; at least one is given.
 *   Bilinear, align_corners=False, no antialiasing: torch.nn.functional.interpolate(src, (H, W), mode="bilinear", align_corners=False).
 *   The coordinates are rational, so that neither fp32 rounding nor contraction can move a tap.  For output row o:
 *       num = max((2o + 1) h - H, 0),   y0 = num / (2H) (integer division),   y1 = min(y0 + 1, h - 1),
 *       ly  = float(num mod 2H) / float(2H)              (one fp32 division)
 *   and for output column p the same with w, W: x0, x1, lx.  With v_ab = src[n, k, y_a, x_b] widened, in fp32:
 *       scores[n,k,o,p] = (1 - ly) ((1 - lx) v00 + lx v01) + ly ((1 - lx) v10 + lx v11)            (contraction allowed)
 *       pred[n,o,p]     = argmax_k scores[n,k,o,p], the first maximum (torch.argmax, tc_argmax_counts, tc_tta_accumulate).
 *   With h == H and w == W every l is 0 and the scores are the input bit for bit (v + 0: a -0 comes out as +0).  Enlarging, shrinking
 *   and different ratios per axis are all this one definition.  With `pred` alone nothing of size ncls H W is written.
 *   One thread owns an output element in all its classes: no atomics, a run repeats to the bit.
 *   -1: src NULL; scores and pred both NULL; scores or pred == src; ncls outside 1..16; N <= 0; h, w, H or W <= 0 or > 4096 (which keeps
 *       (2o + 1) h inside int32); N ncls h w >= 2^31; N H W >= 2^31; N ncls H W >= 2^31 when scores is given; an unknown dtype.
 */
#ifndef TRANSCEPTION_RESAMPLE_H
#define TRANSCEPTION_RESAMPLE_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_RESAMPLE_ABI_VERSION 1
#define TC_RESAMPLE_MAX_EXTENT 4096
#ifndef TC_QUERY
#define TC_QUERY
#endif

/* identity of this part of the library: bumped on any change to a signature below */
TC_QUERY int tc_resample_abi_version(void);
int tc_resample_scores(const void* src, int dtype, float* scores, unsigned char* pred, int N, int ncls, int h, int w, int H, int W,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_RESAMPLE_H */

/*
 * transception_bridge.h -- LayerNorm launches of the bridge layers that take the work of their neighbours along.
 * C ABI of libtransception_hip.so (MI355X / gfx950; csrc/norm.hip).
 *
 * A header of its own: these entries replace no reference call site that transception_hip.h does not already name -- they are the
 * LayerNorm of Scale_reduce (MSTr.py:2249) and of MixFFN_skip (MSTr.py:898 + 894 GELU) with the layout moves in front of them, or several
 * of them, in one launch.  Self-contained (no #include); the conventions are those of transception_hip.h: device pointers owned by the
 * caller, `stream` a hipStream_t passed as void*, nothing allocated, freed or synchronised, every call asynchronous on `stream`.  An
 * unmarked entry returns a status with the values of transception_hip.h: 0 (TC_OK), -1 (TC_ERR_ARG), -2 (TC_ERR_LAUNCH); an entry marked
 * TC_QUERY returns a value instead.  A refused call (-1) launches nothing.  dtype: TC_F32 0, TC_BF16 1, TC_F16 2.
 *
 * ---- Scale_reduce tail (MSTr.py:2236-2249): channel de-interleave of the three convolution outputs + stage-4 token copy + LayerNorm(64)
 * The normalised matrix has B images of Nk rows of 64 channels.  Row lr of an image comes from the source whose [off, off + rows) holds lr:
 *   mult >= 1  a convolution output `src` [B, P, 64 * mult], contiguous, de-interleaved: row off + g * P + pos, channel c is
 *              src[b, pos, c * mult + g]  (g < mult; the source covers mult * P rows)                                    (tc_sr_deinterleave)
 *   mult == 0  a block of `rows` rows: row off + r is src + b * sb + r * ld, 64 channels                                 (tc_copy3d)
 * The sources (at most TC_SR_LN_MAX) must tile [0, Nk) exactly.  The gathered matrix is never stored.
 * tc_sr_ln_fwd: y [B * Nk, 64] (row stride ldy), mean / rstd fp32 [B * Nk]: what tc_layernorm_fwd leaves for the gathered rows, bit for bit
 *   (the same statistics passes and lane-group sums).
 * tc_sr_ln_bwd: dy [B * Nk, 64] (row stride lddy); the normalised values are recomputed from the gathered rows and mean / rstd.  The input
 *   gradient of each row goes where the row came from, in the layout of its source: dsrc[b, pos, c * mult + g] (every element of dsrc is
 *   written once: no zero fill, no accumulate), or dsrc + b * sb + r * ld, added to what is there when `acc` is set (rounded to the storage
 *   type before the add, as a copy launch with its accumulate flag would).  Per row the arithmetic of tc_layernorm_bwd_defer; the per-workgroup
 *   dgamma / dbeta sums are left in `part` ([tc_layernorm_bwd_nblk(B * Nk, 64)][dgamma 64 | dbeta 64] floats) for tc_layernorm_fold, with the
 *   same rows in the same workgroups as tc_layernorm_bwd_defer.
 * 16-bit storage only; every pointer 16-byte aligned, ldy / lddy / ld / sb multiples of 8 elements, B * Nk < 131072 (-1 otherwise).
 * tc_sr_ln_supported: 1 where the two entries take (rows = B * Nk, C, dtype).
 *
 * ---- Several independent LayerNorm (+ GELU) forwards in one launch (the stand-alone LayerNorms of the wide MixFFN sites of a bridge layer)
 * tc_layernorm_fwd_multi: segment i is the call tc_layernorm_fwd(x, ldx, gamma, beta, y, ldy, mean, rstd, rows, C, eps, act, 1, 0, dtype,
 *   stream) and leaves what that call leaves, bit for bit; rstd == mean + 1 selects the interleaved statistics as there.  n <= TC_LN_MULTI_MAX.
 *   One launch (blockIdx.y = segment) where every segment is 16-bit with rows < 4096; otherwise one launch per segment, in order.
 *   -1 if any segment would be refused by tc_layernorm_fwd (nothing is launched then).
 */
#ifndef TRANSCEPTION_BRIDGE_H
#define TRANSCEPTION_BRIDGE_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_BRIDGE_ABI_VERSION 1
#define TC_SR_LN_MAX 4
#define TC_LN_MULTI_MAX 4
#ifndef TC_QUERY
#define TC_QUERY
#endif

/* identity of this part of the library: bumped on any change to a signature or struct below */
TC_QUERY int tc_bridge_abi_version(void);

typedef struct TcSrSrc {
    const void* src;              /* forward values */
    void* dsrc;                   /* tc_sr_ln_bwd: gradient of src, same layout (ignored by tc_sr_ln_fwd) */
    long long sb;                 /* mult == 0: batch stride, elements */
    int mult, P;                  /* mult >= 1: channel multiplier and positions per image */
    int ld, rows;                 /* mult == 0: row stride and rows per image */
    int off;                      /* first row inside an image's Nk rows */
    int acc;                      /* tc_sr_ln_bwd, mult == 0: add to dsrc */
} TcSrSrc;
TC_QUERY int tc_sr_ln_supported(int rows, int C, int dtype);
int tc_sr_ln_fwd(const TcSrSrc* srcs, int nsrc, int B, int Nk, const void* gamma, const void* beta, void* y, int ldy, float* mean,
                 float* rstd, float eps, int dtype, void* stream);
int tc_sr_ln_bwd(const TcSrSrc* srcs, int nsrc, int B, int Nk, const void* dy, int lddy, const void* gamma, const float* mean,
                 const float* rstd, float* part, long long part_floats, int dtype, void* stream);

typedef struct TcLnSeg {
    const void* x; const void* gamma; const void* beta;
    void* y; float* mean; float* rstd;
    int ldx, ldy, rows, C;
    float eps;
    int act;
} TcLnSeg;
int tc_layernorm_fwd_multi(const TcLnSeg* segs, int n, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_BRIDGE_H */

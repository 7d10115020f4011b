/*
 * transception_ema.h -- exponential moving average of the weights on the flat fp32 arenas, C ABI of libtransception_hip.so
 * (MI355X / gfx950; csrc/ema.hip).
 *
 * A header of its own: every entry of transception_hip.h names the reference call sites it replaces, and these replace none -- the
 * reference trains and evaluates the last iterate only.  Self-contained (no #include); the conventions are those of transception_hip.h:
 * device pointers owned by the caller, `stream` a hipStream_t passed as void*, nothing allocated, freed or synchronised, every call
 * asynchronous on `stream`.  An unmarked entry returns a status with the values of transception_hip.h: 0 (TC_OK), -1 (TC_ERR_ARG),
 * -2 (TC_ERR_LAUNCH); an entry marked TC_QUERY returns a value instead.  A refused call (-1) launches nothing.
 *
 * EMA state: four 32-bit words in device memory, owned by the caller, all zero before the first update.
 *   [0] int32 n      updates averaged so far (skipped ones are not counted)
 *   [1] fp32  d      the decay the update of the same step applies
 *   [2] fp32  1 - d
 *   [3] int32        reserved, written as 0
 *
 * tc_ema_advance, launched BEFORE the update kernel of the same step, one thread, ordinary loads and stores.  sumsq == NULL or *sumsq
 *   finite: n += 1 and, in double, d = 0 for n == 1 (the first update copies: torch.optim.swa_utils.AveragedModel's rule), else
 *   min(decay, (1 + n) / (10 + n)) with `warmup` set, else decay; word 1 = (float)d, word 2 = (float)(1 - d), each rounded once from
 *   double.  *sumsq inf or NaN (the optimiser's update kernel skips the same step): all four words stay exactly as they were.
 *   -1: state == NULL, decay not finite or outside [0, 1).
 * tc_ema_update_multi: one launch over the (offset, length) segment table of tc_sgd_step_multi (segs_dev: int64 [nseg][2] in device
 *   memory, max_len the longest length).  A non-finite *sumsq (sumsq may be NULL: no guard) returns before anything is touched.  Else,
 *   with omd = ema_state[2], for every element j of every segment: ema[j] = p[j] where omd == 1.0f -- the value itself, not
 *   e + (w - e) --, elsewhere ema[j] = e + omd * (w - e) in fp32 (torch's lerp_(w, 1 - d)).  p is never written; elements outside the
 *   segments are neither read nor written.  16-byte pieces where offset and length are multiples of 4 and both arenas are 16-byte
 *   aligned, single elements otherwise.  12 bytes per live weight: w read, e read and written.
 *   -1: ema, p, segs_dev or ema_state NULL, nseg <= 0 or > 65535, max_len <= 0.
 * tc_swap_f32: exchanges the contents of two DISJOINT fp32 buffers of n elements in one pass; bit patterns are preserved (NaN payloads,
 *   -0.0).  n a positive multiple of 4, both pointers 16-byte aligned (as for tc_grad_sumsq); -1 otherwise, for a NULL pointer and
 *   for a == b.
 */
#ifndef TRANSCEPTION_EMA_H
#define TRANSCEPTION_EMA_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_EMA_ABI_VERSION 1
#ifndef TC_QUERY
#define TC_QUERY
#endif

/* identity of this part of the library: bumped on any change to a signature below */
TC_QUERY int tc_ema_abi_version(void);
int tc_ema_advance(float* state, const float* sumsq, double decay, int warmup, void* stream);
int tc_ema_update_multi(float* ema, const float* p, const long long* segs_dev, int nseg, long long max_len, const float* ema_state,
                        const float* sumsq, void* stream);
int tc_swap_f32(float* a, float* b, long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_EMA_H */

/*
 * transception_hip.h -- C ABI of libtransception_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the TransCeption forward/backward hot path.  The reference
 * (xmindflow/TransCeption) is 100 % Python on PyTorch and has NO native FFI of its own
 * (SURVEY.md section 2): every arithmetic step of networks/MSTr.py::MSTransception is an ATen
 * call.  Each entry point below therefore names the reference *call sites* (file:line in
 * /root/reference) whose ATen arithmetic it replaces.  The Python host
 * (transception_amd/_lib.py, ctypes) is the binding a reference maintainer would add; see
 * INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers + sizes only; all pointers are DEVICE pointers owned by the caller;
 *  - `stream` is a hipStream_t passed as void*; the library never allocates, frees or
 *    synchronises; every call is asynchronous on `stream` and capturable in a hipGraph;
 *  - activations are token-major / NHWC: a map [B,H,W,C] is the token matrix [B*H*W, C];
 *    `ld*` arguments are row strides in ELEMENTS so that ops can read/write column slices;
 *  - `dtype` selects the storage type of activations/weights: TC_F32, TC_BF16 or TC_F16 (IEEE half); statistics,
 *    accumulators and every `float*` argument are always fp32; the 16-bit types share every kernel (one matrix-core rate),
 *    they differ in the conversion instructions and the MFMA operand type only;
 *  - return value: TC_OK (0) or a negative TC_ERR_* code; nothing throws across the ABI.  An entry marked TC_QUERY returns a value
 *    instead (a version, a yes / no, a count or a size); an unmarked entry returns a status.
 */
#ifndef TRANSCEPTION_HIP_H
#define TRANSCEPTION_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define TC_ABI_VERSION 15
#define TC_QUERY
enum { TC_OK = 0, TC_ERR_ARG = -1, TC_ERR_LAUNCH = -2, TC_ERR_UNSUPPORTED = -3 };
enum { TC_F32 = 0, TC_BF16 = 1, TC_F16 = 2 };
enum { TC_ACT_NONE = 0, TC_ACT_HSWISH = 1, TC_ACT_COORD = 2, TC_ACT_SIGMOID = 3, TC_ACT_GELU = 4,
       TC_ACT_SCALE = 5 /* tc_gemm only: C = alpha * (op(A) op(B) + bias + R), i.e. alpha applied AFTER bias and residual */,
       TC_ACT_RELU = 6  /* tc_bn_fwd / tc_bn_bwd only (SE_Block's act(bn(.)), MSTr.py:590) */ };

/* library identity: returns the ABI version (bumped on any signature change) */
TC_QUERY int tc_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * GEMM:  C[b] = alpha * op(A[b]) * op(B[b]) (+ bias) (+ R[b]) ; optional sigmoid ; optional C += .
 *   op(A) is M x K: transA=0 -> A stored [M,K] (row stride lda); transA=1 -> stored [K,M].
 *   op(B) is K x N: transB=0 -> B stored [K,N] (row stride ldb); transB=1 -> stored [N,K]
 *   (the nn.Linear / 1x1-conv weight layout).  Two batch levels: z = b1*nb2 + b2, element
 *   offsets b1*s?1 + b2*s?2.  splitk > 1 requires accumulate=1 (fp32 atomics into C).
 * Replaces: every nn.Linear / 1x1 nn.Conv2d / torch.bmm / einsum / `@` on the path --
 *   MSTr.py:109-111,136-137,141 (EfficientAttention), :856,866-871,883 (FactorAtt),
 *   :892-900 (MixFFN_skip fc1/fc2), :338,1043-1049 (pw / 1x1 convs), :1333,1342-1346 (CoordAtt),
 *   :2270-2288,2312-2350 (bridge attention), :190,218,276,281 (decoder), and their autograd
 *   backward (dX = dY*W, dW = dY^T*X).
 */
typedef struct TcGemm {
    const void* A; const void* B; void* C;
    const void* bias;            /* [N] or NULL */
    const void* R;               /* residual, same indexing as C with ldr / sR*, or NULL */
    int M, N, K;
    int lda, ldb, ldc, ldr;
    int transA, transB;
    int nb1, nb2;                /* batch counts (>=1) */
    long long sA1, sA2, sB1, sB2, sC1, sC2, sR1, sR2;
    float alpha;
    int accumulate;              /* C += result */
    int act;                     /* TC_ACT_NONE, TC_ACT_SIGMOID or TC_ACT_SCALE */
    int splitk;                  /* >=1 */
    int dtype;
    int c_f32;                   /* C (and the accumulate read) is fp32 whatever dtype is: weight gradients */
    int atomic;                  /* accumulate with fp32 atomics (batches that share one C) */
    float* rowsum;               /* optional fp32 [M]: rowsum[m] += sum_k op(A)[m,k] (bias gradient of a dW GEMM) */
    long long sBias1, sRow1;     /* level-1 batch strides of bias / rowsum (grouped weights: one weight set per batch) */
    int bgap_every;              /* > 0 (multiple of 64, transB = 0 only): op(B) is stored [K,N] in blocks of bgap_every rows with */
    long long bgap;              /* bgap extra elements (multiple of 8) between consecutive blocks -- several [N_i,K] weight matrices
                                  * separated by their biases in the parameter arena, contracted as one K = sum N_i product */
    void* ws;                    /* optional device workspace (16-byte aligned) for the in-kernel split-K fix-up; its first 16 KiB */
    long long ws_bytes;          /* are arrival counters: zero before the first use, left zero by every launch.  One workspace per
                                  * stream (launches that may overlap must not share one).  NULL: requested split-K uses atomics. */
    /* MixFFN_skip fusion hooks (MSTr.py:889-902, out = fc2(GELU(LayerNorm(d))), d = dw3x3(h) + h): the LayerNorm + GELU between the
     * depthwise convolution and fc2 never exists as a tensor, it is applied to the operand tiles of the GEMMs that consume it.
     *   TC_FFN_LN_A (forward fc2; transA = 0, K = LayerNorm width): every row of A goes through GELU(LN(.)) on its way into the
     *     product.  Row statistics are merged from the chunk partials tc_ffn_dw_fwd left in ffn_part ([rows][ffn_nchunk][2]: sum,
     *     squared deviations from the chunk mean; ffn_chunk_n channels per chunk) and written to ffn_stat ([rows][2]: mean, rstd).
     *     ffn_aout (optional, row stride ffn_ldd): the workgroups of the first N tile also store the activated rows GELU(LN(A)) there
     *     (one extra write of the hidden map, so that the weight-gradient GEMM need not recompute the GELU).
     *   TC_FFN_LN_B (weight gradient of fc2, dW = dY^T a; transA = 1, transB = 0, N = LayerNorm width): the rows of B (the stored
     *     d) go through GELU(LN(.)) with the statistics in ffn_stat -- `a` is recomputed, never stored.
     *   TC_FFN_EP (input gradient of fc2, dY W; transA = transB = 0, N = LayerNorm width, no accumulate / split): the epilogue
     *     multiplies by GELU'(u), u = xhat gamma + beta from ffn_d (the stored d, row stride ffn_ldd, rows as C) and ffn_stat, stores
     *     that product gp in C, and leaves per row and 64-column tile (sum gp gamma, sum gp gamma xhat) in ffn_part2
     *     ([rows][ceil(N/64)][2]) for tc_ffn_mid_bwd.
     * ffn_gamma / ffn_beta: the LayerNorm parameters (storage dtype).  Level-1 batches (grouped weights): statistics rows of batch b
     * start at row b * ffn_sRow1, parameters at + b * ffn_sPar1; ffn_d of batch b at + b * ffn_sRow1 * ffn_ldd. */
    int ffn_mode, ffn_nchunk, ffn_chunk_n, ffn_ldd;
    float ffn_eps;
    const float* ffn_part; float* ffn_stat; const void* ffn_gamma; const void* ffn_beta; const void* ffn_d; float* ffn_part2;
    long long ffn_sRow1, ffn_sPar1;
    void* ffn_aout;
    /* BatchNorm statistics of the OUTPUT in the epilogue (DWConv2d_BN / Conv2d_BN, MSTr.py:338-339, 394-400: a 1x1 convolution whose
     * result goes straight into a training-mode BatchNorm2d).  bn_part != NULL (16-bit storage, plain store: no batches, no split-K,
     * no accumulate, 16-byte addressable C rows, N % 8 == 0 -- anything else is TC_ERR_ARG): every 64-row tile t of C leaves
     *   bn_part[N + t*N + n]            = sum over its rows of (c[m][n] - shift[n])
     *   bn_part[N + (T + t)*N + n]      = sum over its rows of (c[m][n] - shift[n])^2        (T = ceil(M / 64) tiles)
     * computed from the ROUNDED values it stores, and bn_part[n] = shift[n] = bn_shift[n] (fp32 [N], e.g. the running mean; NULL: 0).
     * That is tc_bn_fwd's scratch layout with T chunks: pass stats_chunks = T there and the separate statistics pass is skipped. */
    float* bn_part; const float* bn_shift;
} TcGemm;
enum { TC_FFN_NONE = 0, TC_FFN_LN_A = 1, TC_FFN_LN_B = 2, TC_FFN_EP = 3 };
int tc_gemm(const TcGemm* g, void* stream);
/* The two gradient GEMMs of one Linear in ONE launch when both are small-tile bf16 problems (a: dX = dY W, row-major operands,
 * bf16 out; b: dW = dY^T X with fp32 accumulate, transA=1): their workgroups share the grid.  Any other pair: a then b. */
int tc_gemm_pair(const TcGemm* a, const TcGemm* b, void* stream);
/* n (<= 12) INDEPENDENT bf16 GEMMs of the kinds a Linear produces (forward transB=1; dX transA=transB=0; dW transA=1 with fp32 C)
 * in one grid of 64x64 tiles; each problem that uses the split-K fix-up needs its OWN workspace slice.  Anything else: one launch
 * per problem, in order. */
int tc_gemm_multi(const TcGemm* g, int n, void* stream);

/* out[c] (+)= sum_b sum_r x[b*sb + r*ldx + c]   (bias gradients; fp32 output).  Replaces the bias-gradient
 * reductions autograd performs for every Linear/Conv on the path (trainer.py:146). */
int tc_colsum(const void* x, int rows, int cols, int ldx, int nb, long long sb, float* out, int accumulate, int dtype,
              void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (C <= 4096), optionally followed by exact-erf GELU.
 * Replaces nn.LayerNorm at MSTr.py:165,170,303,898(norm1 of MixFFN_skip)+894 GELU,:932-933 (eps 1e-6),
 *   :199,225,1720,2249,2390-2391 and their backward.
 * mean/rstd: fp32 [rows] saved for backward (forward only: rstd == mean + 1 selects the interleaved [rows][2] layout that the
 * TcGemm ffn_stat consumers read).
 */
/* groups > 1: `groups` stacked row blocks of `rows` rows each, block g using gamma/beta + g*pstride (the three MB paths). */
int tc_layernorm_fwd(const void* x, int ldx, const void* gamma, const void* beta, void* y, int ldy,
                     float* mean, float* rstd, int rows, int C, float eps, int act, int groups, long long pstride,
                     int dtype, void* stream);
/* dx = d/dx ; dgamma/dbeta (fp32 [C]) are ACCUMULATED into (caller zeroes or reuses grad buffers).
 * If dres != NULL its rows (stride ldres) are added to dx (fan-in of a residual branch). */
int tc_layernorm_bwd(const void* dy, int lddy, const void* x, int ldx, const void* gamma, const void* beta,
                     const float* mean, const float* rstd, void* dx, int lddx, const void* dres, int ldres,
                     float* dgamma, float* dbeta, int rows, int C, int act, int groups, long long pstride,
                     float* scratch, long long scratch_floats, int dtype, void* stream);
/* scratch (>= tc_layernorm_bwd_scratch_floats() floats, or NULL): a per-stream workspace with the TcGemm.ws contract (its
 * first 16 KiB are arrival counters: zero before the first use, left zero).  With it the per-workgroup parameter-gradient
 * partials are folded 16 at a time inside the kernel before anything touches dgamma / dbeta atomically -- one pass over
 * x / dy for dx, dgamma and dbeta together. */
TC_QUERY long long tc_layernorm_bwd_scratch_floats(int rows, int C, int groups);
/* Deferred parameter gradients (the backward of nn.LayerNorm's weight / bias at the same reference lines): tc_layernorm_bwd_defer is
 * tc_layernorm_bwd, but instead of folding its per-workgroup column sums at its tail it leaves them in `part`
 * ([groups][tc_layernorm_bwd_nblk(rows, C)][dgamma C | dbeta C] floats, a buffer of this launch's own, kept until the fold) and returns;
 * tc_layernorm_fold adds the partials of up to 64 such launches to their dgamma / dbeta in ONE launch (the host calls it when a backward
 * sweep stops or ends).  tc_layernorm_bwd_nblk returns 0 for shapes that are not deferred (C > 1024: they fold in launches of their own). */
typedef struct {
    const float* part;            /* what tc_layernorm_bwd_defer left */
    float* dgamma; float* dbeta;  /* accumulated into (group g at + g * pstride) */
    long long pstride;
    int nblk, C, groups;
} TcLnFold;
TC_QUERY int tc_layernorm_bwd_nblk(int rows, int C);
int tc_layernorm_bwd_defer(const void* dy, int lddy, const void* x, int ldx, const void* gamma, const void* beta,
                           const float* mean, const float* rstd, void* dx, int lddx, const void* dres, int ldres,
                           float* dgamma, float* dbeta, int rows, int C, int act, int groups, long long pstride,
                           float* part, long long part_floats, int dtype, void* stream);
/* (a site is what tc_layernorm_bwd_defer parks: C % 4 == 0, C <= 1024, nblk >= 1 -- anything else is TC_ERR_ARG before the launch) */
int tc_layernorm_fold(const TcLnFold* sites, int n, void* stream);
/* dgamma / dbeta may both be NULL above (dx only); this entry then produces them as a row-parallel column reduction, so the
 * host can run it on a second stream beside the activation-gradient chain.  Same argument tests as tc_layernorm_bwd (C % 4, C <= 2048,
 * act TC_ACT_NONE or TC_ACT_GELU). */
int tc_layernorm_bwd_params(const void* dy, int lddy, const void* x, int ldx, const void* gamma, const void* beta,
                            const float* mean, const float* rstd, float* dgamma, float* dbeta, int rows, int C, int act,
                            int groups, long long pstride, int dtype, void* stream);

/* LayerNorm over the pixels of a pixel-shuffled map without the shuffle copy (PatchExpand / FinalPatchExpand_X4, MSTr.py:196-199,
 * 222-225: Linear -> rearrange 'b h w (p1 p2 c) -> b (h p1) (w p2) c' -> LayerNorm(c)): x is the UN-shuffled Linear output
 * [B*H*W, p*p*C] (row stride ldx); output row (b, h*p+p1, w*p+p2) normalises the C-wide chunk (p1*p+p2) of x row (b, h, w); y, mean,
 * rstd are indexed by output pixel.  Backward writes dx in the un-shuffled layout (row stride lddx), dgamma/dbeta accumulated,
 * scratch as in tc_layernorm_bwd. */
int tc_layernorm_ps_fwd(const void* x, int ldx, const void* gamma, const void* beta, void* y, int ldy, float* mean, float* rstd,
                        int B, int H, int W, int p, int C, float eps, int dtype, void* stream);
int tc_layernorm_ps_bwd(const void* dy, int lddy, const void* x, int ldx, const void* gamma, const void* beta, const float* mean,
                        const float* rstd, void* dx, int lddx, float* dgamma, float* dbeta, int B, int H, int W, int p, int C,
                        float* scratch, long long scratch_floats, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * The tail of the last decoder stage in one forward and one backward call (ABI 15, round 6):
 *   logits = last_layer(LayerNorm(rearrange 'b h w (p1 p2 c) -> b (h p1) (w p2) c' (x)))
 * Replaces the rearrange + self.norm of FinalPatchExpand_X4.forward (MSTr.py:222-225) and self.last_layer (Conv2d(c, n_class, 1),
 * MSTr.py:258, called at :281) -- tc_layernorm_ps_fwd + tc_gemm, and tc_gemm_pair + tc_layernorm_ps_bwd on the way back -- without
 * the normalised [B * (H p) * (W p), c] map (or its gradient) ever reaching memory.
 *   x       [B*H*W, p*p*c] the expand Linear's output (row stride ldx, un-shuffled); p = 0: x is [B*H*W, c] itself (no rearrange)
 *   Wc, bc  [ncls, c], [ncls] (the 1x1 convolution's weight / bias); gamma, beta [c]
 *   logits  [B*(H p)*(W p), ldl] token-major, ldl >= ncls; mean / rstd [rows] fp32 saved for the backward
 *   dl      the gradient of logits [rows, lddl]; read in 16-byte pieces when its rows are 16-byte aligned (lddl a multiple of 8 elements
 *           >= ncls rounded up to 8: the captured training step pads the logits' rows to that), element by element otherwise
 *   dx      written in x's layout (row stride lddx); dgamma / dbeta / dWc / dbc fp32, ADDED to
 *   scratch fp32, tc_ln_cls_scratch_floats(rows, ncls) floats (per-workgroup partial sums; folded by the call's second launch)
 * 16-bit storage, c = 64, ncls in {2, 9}: tc_ln_cls_supported; TC_ERR_ARG otherwise (callers keep the op-by-op form).
 * xn is kept in fp32 between the LayerNorm and the product (the op-by-op form rounds it to the storage type). */
TC_QUERY int tc_ln_cls_supported(int C, int ncls, int dtype);
TC_QUERY long long tc_ln_cls_scratch_floats(int rows, int ncls);
int tc_ln_cls_fwd(const void* x, int ldx, const void* gamma, const void* beta, const void* Wc, const void* bc, void* logits, int ldl,
                  float* mean, float* rstd, int B, int H, int W, int p, int C, int ncls, float eps, int dtype, void* stream);
int tc_ln_cls_bwd(const void* dl, int lddl, const void* x, int ldx, const void* gamma, const void* beta, const void* Wc, const float* mean,
                  const float* rstd, void* dx, int lddx, float* dgamma, float* dbeta, float* dWc, float* dbc, float* scratch,
                  long long scratch_floats, int B, int H, int W, int p, int C, int ncls, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Depthwise k x k convolution on NHWC maps, k in {3,5,7}, stride 1 or 2, padding (k-1)/2,
 * weight in the PyTorch layout [C,1,k,k], optional bias, optional "+ x" (stride 1 only).
 * x rows (pixels) have stride ldx elements, y rows ldy, so channel slices of wider buffers work.
 * Replaces: DWConv MSTr.py:21-31 (+ the skip add at :900), ConvPosEnc :744-752, ConvRelPosEnc
 *   depthwise 3/5/7 convs :785-797,814-816, DWConv2d_BN.dwconv :328-336, ResBlock.dwconv :1005-1013.
 */
/* groups > 1 (stride 1 only): `groups` stacked sets of B images, set g using the filters at w + g*wstride and the bias at
 * bias + g*wstride (one stride for every parameter: the distance between two MB encoders in the flat arena). */
int tc_dwconv_fwd(const void* x, int ldx, const void* w, const void* bias, void* y, int ldy,
                  int B, int H, int W, int C, int k, int stride, int add_input, int groups, long long wstride, int dtype,
                  void* stream);
/* accumulate=1: dx += result */
int tc_dwconv_bwd_input(const void* dy, int lddy, const void* w, void* dx, int lddx,
                        int B, int H, int W, int C, int k, int stride, int add_input, int accumulate, int groups,
                        long long wstride, int dtype, void* stream);
/* dw [C,1,k,k] and db [C] (fp32) are ACCUMULATED into. db may be NULL.
 * ws / ws_bytes: optional per-stream workspace with the TcGemm.ws contract (first 16 KiB = zeroed arrival counters): the
 * workgroups' sums are then folded 16 at a time before anything touches dw / db atomically. */
int tc_dwconv_bwd_weight(const void* dy, int lddy, const void* x, int ldx, float* dw, float* db,
                         int B, int H, int W, int C, int k, int stride, int groups, long long wstride, void* ws,
                         long long ws_bytes, int dtype, void* stream);
/* Both gradients of a stride-1 convolution in ONE launch (same arguments and semantics as the two entries above; falls back to them when
 * the operands do not allow the 16-byte tile kernels): the two launches read the same dy and do not depend on each other. */
/* Deferred weight gradients: with ws_bytes < 0, ws is a buffer of the caller's own (>= tc_dwconv_bwd_plan() floats, -ws_bytes bytes;
 * 0 floats: this shape cannot defer) in which tc_dwconv_bwd leaves the per-workgroup sums instead of folding them at its tail; tc_dw_fold adds
 * the sums of up to 48 such launches to their dw / db in ONE launch (the host calls it when a backward sweep stops or ends). */
typedef struct {
    const float* part; float* dw; float* db;   /* the launch's sums; its dw / db (db may be NULL), group g at + g * wstride */
    float* dgamma; float* dbeta;               /* tc_ffn_mid_bwd only (nt = k*k + 3), else NULL */
    long long wstride;
    int C, k, groups;
    int ch, chunks, gx, nt;                    /* geometry of the sums ([group * chunks + chunk][gx walkers][nt taps][ch channels]): filled by the plans */
} TcDwFold;
/* floats the launch will leave (0: this shape cannot defer); fill *site's geometry */
TC_QUERY long long tc_dwconv_bwd_plan(int B, int H, int W, int C, int k, int groups, int dtype, TcDwFold* site);
int tc_dw_fold(const TcDwFold* sites, int n, void* stream);
int tc_dwconv_bwd(const void* dy, int lddy, const void* x, int ldx, const void* w, void* dx, int lddx, float* dw, float* db, int B, int H,
                  int W, int C, int k, int add_input, int accumulate, int groups, long long wstride, void* ws, long long ws_bytes,
                  int dtype, void* stream);

/* Up to four INDEPENDENT stride-1 depthwise convolutions in ONE launch: ConvRelPosEnc's 3x3 / 5x5 / 7x7 branches on column
 * slices of one map (MSTr.py:785-816), or the four per-scale MixFFN convolutions of a bridge layer (different maps).
 * mode 0: y = conv(x) (+bias) (+x); mode 1: y (= dx) = conv^T(x (= dy)) (+x) (+y when accumulate); mode 2: dw / db += gradients
 * from x and dy; mode 3: both gradients in the one launch -- y (= dx) = conv^T(dy) (+dy) (+y when accumulate) and dw / db += gradients
 * from x and dy (tc_dwconv_bwd per segment).  Every segment carries its own geometry and row strides; groups / wstride are common (see tc_dwconv_fwd);
 * ws as in tc_dwconv_bwd_weight.  Deferred sums (ws_bytes < 0, modes 2 / 3) need every segment on the 16-byte tile kernels: with one that is
 * not, TC_ERR_ARG before anything is launched. */
typedef struct TcDwSeg {
    const void* x; const void* w; const void* bias; void* y; const void* dy; float* dw; float* db;
    int C; int k; int ldx; int ldy; int lddy; int B; int H; int W;
    float* stat;                 /* mode 0, k = 3, optional: LayerNorm chunk partials of y as tc_ffn_dw_fwd leaves them */
} TcDwSeg;
int tc_dwconv_multi(const TcDwSeg* segs, int nseg, int mode, int add_input, int accumulate, int groups, long long wstride,
                    void* ws, long long ws_bytes, int dtype, void* stream);
/* Deferred weight gradients of a mode 2 / 3 launch (ws_bytes < 0, as tc_dwconv_bwd): total floats the launch will leave (0: cannot defer);
 * sites[i] gets segment i's geometry and offs[i] its offset (floats) into the one buffer -- the caller sets part / dw / db / wstride. */
TC_QUERY long long tc_dwconv_multi_plan(const TcDwSeg* segs, int nseg, int groups, int dtype, TcDwFold* sites, long long* offs);

/* ------------------------------------------------------------------------------------------
 * MixFFN_skip middle (MSTr.py:889-902 with DWConv :21-31): between fc1 and fc2 the reference runs dw3x3(+bias) + skip, LayerNorm(4C),
 * GELU as three passes over the hidden map (and their three autograd backward passes + the conv's weight gradient).
 * Here:  forward  = tc_ffn_dw_fwd (d = dw3x3(h) + bias + h, plus LayerNorm chunk partials) -> fc2 GEMM with TC_FFN_LN_A;
 *        backward = fc2 input-gradient GEMM with TC_FFN_EP + fc2 weight-gradient GEMM with TC_FFN_LN_B -> tc_ffn_mid_bwd.
 */
/* channels per statistics chunk of tc_ffn_dw_fwd for a C-channel map of this dtype (C must be a multiple of it) */
TC_QUERY int tc_ffn_chunk(int C, int dtype);
/* y = dw3x3(x) + bias + x on `groups` stacked sets of B images (parameters of set g at + g*wstride), and
 * stat[((g*B + b)*H*W + pixel) * (C / tc_ffn_chunk) + chunk] = float2(sum, squared deviations from the chunk mean) of the chunk's channels,
 * computed from the fp32 result BEFORE it is rounded to y's storage type (in 16-bit storage they are not the statistics of the stored y).
 * stat may be NULL; with stat, C must be a multiple of tc_ffn_chunk (TC_ERR_ARG otherwise). */
int tc_ffn_dw_fwd(const void* x, int ldx, const void* w, const void* bias, void* y, int ldy, float* stat, int B, int H, int W,
                  int C, int groups, long long wstride, int dtype, void* stream);
/* One launch for up to four MixFFN sites (the four scales of a bridge layer):
 *   dd = LayerNorm backward of gp (x) gamma using stat ([rows][2] mean, rstd) and the row sums in part2 ([rows][nch2][2]),
 *   dh = dw3x3^T(dd) + dd, and ACCUMULATED into fp32: dw [C,1,3,3], db [C] (conv), dgamma / dbeta [C] (LayerNorm).
 * gp / d / h / dh: [groups*B*H*W, C] maps with row strides ld*; ws as in tc_dwconv_bwd_weight. */
typedef struct TcFfnSeg {
    const void* gp; const void* d; const void* h; void* dh; const float* stat; const float* part2; const void* w; const void* gamma;
    float* dw; float* db; float* dgamma; float* dbeta;
    int C, ldg, ldd, ldh, lddh, B, H, W, nch2;
} TcFfnSeg;
int tc_ffn_mid_bwd(const TcFfnSeg* segs, int nseg, int groups, long long wstride, void* ws, long long ws_bytes, int dtype,
                   void* stream);
/* Deferred parameter gradients of a tc_ffn_mid_bwd launch (ws_bytes < 0, as tc_dwconv_bwd): total floats it will leave (0: cannot defer);
 * sites[i] / offs[i] as tc_dwconv_multi_plan -- the caller sets part, dw, db, dgamma, dbeta and wstride, tc_dw_fold adds them. */
TC_QUERY long long tc_ffn_mid_plan(const TcFfnSeg* segs, int nseg, int groups, int dtype, TcDwFold* sites, long long* offs);

/* MixFFN_skip forward as ONE spatially tiled kernel (16-bit storage types, C = 64 or 128; see csrc/mixffn.hip):
 *   out = fc2(GELU(LayerNorm_4C(dw3x3(h) + bias + h))) + b2 + res,  h = x W1^T + b1        (MSTr.py:889-902, DWConv :21-31)
 * x [groups*B*H*W, C] (row stride ldx); parameters of weight group g at + g*wstride elements (PyTorch layouts: w1 [4C,C], wd [4C,1,3,3],
 * w2 [C,4C]); res / out: pixel row r of group g at g*sres + r*ldr / g*sout + r*ldo (row blocks or column blocks of a wider buffer).
 * Optional outputs for the backward pass, contiguous [groups*B*H*W, 4C] in the storage type: h (fc1 output), d (dw3x3(h) + bias + h),
 * a (GELU(LN(d))); stat: fp32 [rows][2] = (mean, rstd) of the LayerNorm.  The hidden maps that are not asked for never leave LDS.
 * Replaces fc1 GEMM + tc_ffn_dw_fwd + (tc_layernorm_fwd) + fc2 GEMM of the op-by-op form.
 * GELU: the 16-bit kernels evaluate the normal CDF as a clamped odd polynomial (|error| <= 1.02e-5 absolute, csrc/tc_common.h gelu_poly) in
 * every FORWARD use (here, the op-by-op LayerNorm + GELU, tc_gelu_fwd); the backward kernels and the fp32 path use the erf form.
 * Ranges (TC_ERR_ARG beyond them; both tiled directions): B * tiles per image < 2^22, H * W < 2^23, H * W * ld < 2^31 -- the kernels form
 * tile / pixel indices by fp32 floor((n + 0.5) / d) and per-image element offsets in 32 bits. */
typedef struct TcFfnFused {
    const void* x; const void* w1; const void* b1; const void* wd; const void* bd; const void* gamma; const void* beta;
    const void* w2; const void* b2; const void* res; void* out; void* h; void* d; void* a; float* stat;
    long long sres, sout, wstride;
    int ldx, ldr, ldo, C, B, H, W, groups;
    float eps;
    int tile_h, tile_w;          /* 0: the library picks the pixel tile; otherwise a forced shape (tests, tuning) */
    const void* pre_gamma; const void* pre_beta; float pre_eps;   /* optional LayerNorm(C) of x ahead of fc1 (the block's norm2, MSTr.py:168 /
                                                                    :906-907), applied as the tile is loaded; null: x is used as it is.  Same
                                                                    per-group stride (wstride) as the other parameters */
} TcFfnFused;
TC_QUERY int tc_ffn_fused_supported(int C, int dtype);
int tc_ffn_fused_fwd(const TcFfnFused* f, int dtype, void* stream);

/* MixFFN_skip backward with the hidden maps kept on the chip (16-bit storage types; see csrc/mixffn_bwd.hip): the autograd backward of
 * MSTr.py:889-902 (fc2, GELU, LayerNorm(4C), DWConv :21-31 + skip, fc1) from what tc_ffn_fused_fwd left -- d = dw3x3(h) + bias + h in
 * the storage type and stat = (mean, rstd) per pixel -- and the site's input x and output gradient dy.  Three launches:
 *   1. rows of 64 pixels: gp = (dy W2) (.) GELU'(u), u = LN(d);  LayerNorm backward -> gd (the only hidden-width map that is written);
 *      dW2 += dy^T GELU(u), db2, dgamma, dbeta as per-workgroup fp32 partials (the activation GELU(u) is recomputed, never stored);
 *   2. pixel tiles with a one-pixel halo: h = fc1(x) recomputed by MFMA, dh = dw3x3^T(gd) + gd, dx (+)= dh W1,
 *      dW1 += dh^T x, db1, dwd, dbd as per-workgroup fp32 partials (h and dh never leave LDS);
 *   3. the partials of all workgroups are added into the fp32 gradient arrays.
 * x / dy / dx rows as in TcFfnFused (x, dx: group g at g*B*H*W rows; dy: pixel row r of group g at g*sdy + r*lddy); parameters and
 * gradient arrays of weight group g at + g*wstride elements.  gd: [groups*B*H*W, 4C] scratch in the storage type; part: fp32 scratch of
 * tc_ffn_fused_bwd_scratch_floats(C, groups) floats.  acc_dx = 1 adds to dx.  Replaces {fc2 dX + dW GEMMs, tc_ffn_mid_bwd, fc1 dX + dW
 * GEMMs} of the op-by-op form, which read or write eight hidden-width maps. */
typedef struct TcFfnBwd {
    const void* x; const void* dy; const void* d; const float* stat;
    const void* w1; const void* b1; const void* wd; const void* gamma; const void* beta; const void* w2;
    void* dx; void* gd; float* part; long long part_floats;
    float* dw1; float* db1; float* dwd; float* dbd; float* dgamma; float* dbeta; float* dw2; float* db2;
    long long sdy, wstride;
    int ldx, lddy, lddx, C, B, H, W, groups, acc_dx;
    float eps;
    int tile_h, tile_w;          /* 0: the library picks the pixel tile of launch 2 */
    const void* pre_gamma; const void* pre_beta; float* dpre_gamma; float* dpre_beta; float pre_eps;
                                 /* the forward's optional LayerNorm(C) of x (TcFfnFused.pre_gamma): x is normalised again as it is loaded, dx
                                    becomes the gradient of the RAW x (LayerNorm backward applied where dx leaves launch 2) and the fp32
                                    dpre_* receive (+=) the LayerNorm's parameter gradients; null: no LayerNorm */
} TcFfnBwd;
TC_QUERY int tc_ffn_fused_bwd_supported(int C, int dtype);
TC_QUERY long long tc_ffn_fused_bwd_scratch_floats(int C, int groups);
int tc_ffn_fused_bwd(const TcFfnBwd* f, int dtype, void* stream);

/* ---- EfficientAttention block: out = t + reproj(softmax_c(Q) . (softmax_n(K)^T V)) with K | Q | V = LayerNorm(t) W^T + b ----
 * Replaces, for C = 64 and one head, MSTr.py:80-143 (EfficientAttention.forward: keys / queries / values 1x1 convolutions,
 * softmax over the tokens for the keys, over the channels for the queries, context = key @ value^T, attended = context^T @ query,
 * reprojection) together with its caller's LayerNorm and residual (MSTr.py:166-167: tx = x + attn(norm1(x))), forward and backward.
 * t / out / dout / dt: [B * N, C] token maps of the storage type with leading dimensions ldt / ldo / lddo / lddt (elements).
 * ctx [B][C][C] and kstat [B][2][C] (column maximum and sum of the keys' softmax) are fp32 outputs of the forward that the backward
 * reads; part is fp32 scratch of tc_effatt_scratch_floats(C, B, N) floats; g1 a [B * N, C] scratch map of the storage type.
 * The backward ADDS into the fp32 gradient arrays (dw* [C][C], db* / dgamma / dbeta [C]); dt is overwritten, or added to when acc_dt.
 * Seven launches in all (3 forward, 4 backward) on `stream`.  TC_ERR_ARG for anything unsupported (use tc_effatt_supported): C != 64,
 * fp32 storage, token maps or weight matrices not 16-byte aligned, leading dimensions not multiples of 8 elements. */
typedef struct TcEffAtt {
    const void* t; const void* gamma; const void* beta;
    const void* wk; const void* bk; const void* wq; const void* bq; const void* wv; const void* bv; const void* wr; const void* br;
    void* out; float* ctx; float* kstat; float* part; long long part_floats;
    const void* dout; void* dt; void* g1;
    float* dgamma; float* dbeta; float* dwk; float* dbk; float* dwq; float* dbq; float* dwv; float* dbv; float* dwr; float* dbr;
    int ldt, ldo, lddo, lddt, acc_dt, C, B, N;
    float eps;
} TcEffAtt;
TC_QUERY int tc_effatt_supported(int C, int dtype);
TC_QUERY long long tc_effatt_scratch_floats(int C, int B, int N);
int tc_effatt_fwd(const TcEffAtt* f, int dtype, void* stream);
int tc_effatt_bwd(const TcEffAtt* f, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm2d over token rows ([rows, C], statistics over rows) fused with its activation and an
 * optional residual add:  y = act((x-mean)*rstd*gamma+beta) (+ res).
 * Replaces nn.BatchNorm2d + Hardswish / silu_swish at MSTr.py:339-340,358-360 (RIPM), :376-401,1045-1049
 *   (ResBlock / Conv2d_BN), :1335-1336 (CoordAtt bn1 + act) and the residual add :1050.
 * training=1: batch statistics (biased var), running stats updated with momentum 0.1 and the unbiased
 *   variance, save_mean/save_rstd [C] written for backward.  training=0: running statistics.
 * `partial` is caller-provided fp32 scratch of at least tc_bn_scratch_floats(rows, C) floats.
 * stats_chunks > 0 (training only): `partial` ALREADY holds the shifted sums of x in stats_chunks row chunks, left there by the
 *   GEMM that produced x (TcGemm.bn_part; C * (1 + 2 * stats_chunks) floats) -- no statistics pass is launched.  0: computed here.
 */
TC_QUERY long long tc_bn_scratch_floats(int rows, int C);
int tc_bn_fwd(const void* x, int ldx, const void* gamma, const void* beta, float* running_mean,
              float* running_var, const void* res, int ldres, void* y, int ldy, float* save_mean,
              float* save_rstd, float* partial, int rows, int C, float eps, float momentum, int training,
              int stats_chunks, int act, int dtype, void* stream);
/* dgamma/dbeta ACCUMULATED into; dx written (or accumulated into when accumulate=1).
 * (The residual gradient is dy itself.) */
int tc_bn_bwd(const void* dy, int lddy, const void* x, int ldx, const void* gamma, const void* beta,
              const float* save_mean, const float* save_rstd, void* dx, int lddx, float* dgamma,
              float* dbeta, float* partial, int rows, int C, int act, int accumulate, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Softmax over one axis of a batch of [R, Ccols] matrices (row stride ld, batch stride sb).
 * axis=1: over the contiguous columns; axis=0: over the rows (per column).
 * Replaces F.softmax / .softmax at MSTr.py:118-128 (EfficientAttention: keys over N, queries over C),
 *   :865 (FactorAtt k over N), :2322-2332 (channel attention on the flat re-view), :2283 (scores).
 * axis=0 is split over row ranges (two passes through caller-provided fp32 scratch of tc_softmax_scratch_floats floats);
 * scratch may be NULL for axis=1.
 */
TC_QUERY long long tc_softmax_scratch_floats(int nb, int R, int Ccols);
int tc_softmax_fwd(const void* x, void* y, float* scratch, int nb, long long sbx, long long sby, int R, int Ccols,
                   int ldx, int ldy, int axis, int dtype, void* stream);
int tc_softmax_bwd(const void* dy, const void* y, void* dx, float* scratch, int nb, long long sbdy, long long sby,
                   long long sbdx, int R, int Ccols, int lddy, int ldy, int lddx, int axis, int accumulate,
                   int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused single-head attention with spatial-reduction K/V (the Dual Transformer Bridge core):
 *   O[b] = softmax(Q[b] K[b]^T * scale) V[b],  head dim 64, no score matrix in HBM.
 *   lse[b, q] = log-sum-exp of the scaled scores (fp32), saved for backward.
 * Replaces MSTr.py:2281-2287 (M_EfficientSelfAtten: q@k^T*scale -> softmax -> @v) and its backward.
 * tc_attn_fwd / tc_attn_bwd are the fp32 parity form: one query group per launch, exact fp32 products, dtype = TC_F32 only
 * (any other dtype is TC_ERR_ARG, before any launch).  tc_attn_fwd_seg / tc_attn_bwd_seg below run them once per segment for
 * fp32 storage; 16-bit storage goes through the _seg entries, which have their own kernels.
 */
int tc_attn_fwd(const void* Q, int ldq, long long sq, const void* K, int ldk, const void* V, int ldv,
                long long skv, void* O, int ldo, long long so, float* lse, int B, int Nq, int Nk,
                float scale, int dtype, void* stream);
/* delta: fp32 scratch [B*Nq].  dQ is written; dK/dV (row strides lddk/lddv, batch stride sdkv) are written, or
 * added to when accumulate_dkv=1 (several query groups sharing one K/V). */
int tc_attn_bwd(const void* Q, int ldq, long long sq, const void* K, int ldk, const void* V, int ldv,
                long long skv, const void* O, int ldo, long long so, const void* dO, int lddo, long long sdo,
                const float* lse, float* delta, void* dQ, int lddq, long long sdq, void* dK, int lddk,
                void* dV, int lddv, long long sdkv, int accumulate_dkv, int B, int Nq, int Nk, float scale,
                int dtype, void* stream);

/* Segmented form used by the bridge: Q / O / dO / dQ / lse are stage-major row blocks -- segment i holds B images of
 * nq[i] queries back to back, segments follow each other -- while K/V stay image-major (batch stride skv).  ONE launch
 * covers all segments (bf16 / fp16); fp32 storage runs the per-segment kernels above.  nq is a HOST array of nseg (<= 4) ints.
 * Replaces the same reference lines (MSTr.py:2281-2287) for all 6076 query tokens of every image at once.
 * 16-bit path: head dimension 64; Q, K, V (and dO) 16-byte aligned with row strides that are multiples of 8 elements; O / dQ rows
 * are written with 16-byte stores when their pointer and stride allow it (8-byte stores otherwise).  The forward kernel's softmax
 * is referenced to an integer exponent per row that is raised only when a row sum outgrows it by 2^30 (2^14 for fp16) -- the
 * result is the ordinary softmax(QK^T scale)V, lse the ordinary log-sum-exp.  The kernels use 126 KB of dynamic LDS.
 * qscaled (16-bit paths only): Q already holds q * scale * log2(e), rounded ONCE from the fp32 accumulator of the projection that
 * produced it (tc_gemm with TC_ACT_SCALE): the scores then need no multiply per element, and no second rounding of Q.  The
 * backward then takes the same scaled Q and still returns dQ = dL/dq of the UNSCALED projection output (and dK, dV as ever). */
int tc_attn_fwd_seg(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, long long skv, void* O, int ldo,
                    float* lse, int B, int nseg, const int* nq, int Nk, float scale, int qscaled, int dtype, void* stream);
/* dkv32: fp32 scratch of TC_ATTN_DKV_SPLITS * B * Nk * 128 floats (16-bit path: every query chunk of the dK/dV kernel writes its own
 * partial dK|dV there, one conversion kernel adds them; needs no initialisation); may be NULL for fp32.
 * delta: fp32 [rows], written (row sums of O dO; computed inside the dQ kernel when O / dO rows are 16-byte addressable).
 * With qscaled = 1 and 16-byte addressable rows the two kernels are the hand-scheduled streams of csrc/gen_dq_asm.py / gen_dkv_asm.py
 * (same arithmetic in the same order as the compiler-scheduled kernels, which remain for every other case and as
 * TC_ATTN_DQ_ASM=0 / TC_ATTN_DKV_ASM=0); the dK/dV stream keeps its per-tile row statistics in the LAST of the dkv32 partial buffers. */
#define TC_ATTN_DKV_SPLITS 8
int tc_attn_bwd_seg(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, long long skv, const void* O,
                    int ldo, const void* dO, int lddo, const float* lse, float* delta, float* dkv32, void* dQ, int lddq,
                    void* dK, int lddk, void* dV, int lddv, long long sdkv, int B, int nseg, const int* nq, int Nk,
                    float scale, int qscaled, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise / layout kernels.
 */
/* out = alpha*a + b*c (rows x cols, each with its own row stride).  FactorAtt merge MSTr.py:877, 821. */
int tc_fma3_fwd(const void* a, int lda, const void* b, int ldb, const void* c, int ldc, void* out, int ldo,
                int rows, int cols, float alpha, int dtype, void* stream);
/* da = alpha*dout ; db (+)= dout*c ; dc = dout*b.  db_accumulate adds into db (q receives two grads). */
int tc_fma3_bwd(const void* dout, int lddo, const void* b, int ldb, const void* c, int ldc, void* da, int ldda,
                void* db, int lddb, int db_accumulate, void* dc, int lddc, int rows, int cols, float alpha,
                int dtype, void* stream);
/* y = a + b */
int tc_add(const void* a, int lda, const void* b, int ldb, void* y, int ldy, int rows, int cols, int dtype,
           void* stream);
/* dz = dy * s * (1 - s) given s = sigmoid(z) */
int tc_sigmoid_bwd(const void* dy, const void* s, void* dz, long long n, int dtype, void* stream);
/* batched strided copy: dst[b, r, c] (+)= src[b, r, c]  (batch strides sb*, row strides ld*, in elements).
 * The torch.cat / slicing glue of MSTr.py:2231,2237 (raw stage-4 tokens into the K/V source). */
int tc_copy3d(const void* src, long long sbs, int lds, void* dst, long long sbd, int ldd, int nb, int rows, int cols,
              int accumulate, int dtype, void* stream);
/* batched transpose: dst[b, c, r] = src[b, r, c]  (logits NHWC -> NCHW, MSTr.py:281 permute) */
int tc_transpose(const void* src, void* dst, int nb, int R, int Ccols, int dtype, void* stream);

/* SE_Block (MSTr.py:571-594, the concat = "se" aggregate of MHCA_stage :1396-1397): x is [B*N, C] token rows (row stride ldx).
 *   squeeze     pooled[b, c] = mean over the image's N rows of x                      (AdaptiveAvgPool2d(1), :586)
 *   gate        y[b, n, c]   = x[b, n, c] * gate[b, c]                                (x * y.expand_as(x), :588)
 * and their gradients: dx (+)= dpooled / N;  dx (+)= dy * gate, dgate[b, c] = sum_n dy * x.  pooled / gate / dgate are [B, C], storage dtype. */
int tc_chan_pool_fwd(const void* x, int ldx, void* pooled, int B, int N, int C, int dtype, void* stream);
int tc_chan_pool_bwd(const void* dpooled, void* dx, int lddx, int B, int N, int C, int accumulate, int dtype, void* stream);
int tc_chan_gate_fwd(const void* x, int ldx, const void* gate, void* y, int ldy, int B, int N, int C, int dtype, void* stream);
int tc_chan_gate_bwd(const void* dy, int lddy, const void* x, int ldx, const void* gate, void* dx, int lddx, int dx_accumulate,
                     void* dgate, int B, int N, int C, int dtype, void* stream);
/* y = max(x, 0) and dz = dy where y > 0 (nn.ReLU of SE_Block's excitation, MSTr.py:577; after its BatchNorm the ReLU is TC_ACT_RELU) */
int tc_relu_fwd(const void* x, void* y, long long n, int dtype, void* stream);
int tc_relu_bwd(const void* dy, const void* y, void* dz, long long n, int dtype, void* stream);

/* CBAMBlock pieces (the concat = "cbam" aggregate, MSTr.py:1128-1211): x is [B*N, C] token rows.
 *   tc_chan_pool2: pooled rows 0..B-1 = max over the image's N rows (idx[b, c] = the first maximal row), rows B..2B-1 = mean    (:1141-1142)
 *   tc_pix_stats:  st[row] = (max over the C channels, mean over them), idx[row] = the first maximal channel                   (:1156-1158)
 *   tc_sa_conv:    g = sigmoid(Conv2d(2 -> 1, k x k, padding k/2)(st))  over the [B, H, W] token grid, k = 3 or 7               (:1151,1161-1163)
 *                  backward: dst, dw (fp32 [2*k*k], ACCUMULATED), db (fp32 [1], ACCUMULATED) from dg and the stored g
 *   tc_pix_gate:   y[row, c] = x[row, c] * g[row]; backward dx (+)= dy g, dg[row] = sum_c dy x                                  (:1206) */
int tc_chan_pool2_fwd(const void* x, int ldx, void* pooled, int* idx, int B, int N, int C, int dtype, void* stream);
int tc_chan_pool2_bwd(const void* dpooled, const int* idx, void* dx, int lddx, int B, int N, int C, int accumulate, int dtype, void* stream);
int tc_pix_stats_fwd(const void* x, int ldx, void* st, int* idx, int rows, int C, int dtype, void* stream);
int tc_pix_stats_bwd(const void* dst, const int* idx, void* dx, int lddx, int rows, int C, int accumulate, int dtype, void* stream);
int tc_sa_conv_fwd(const void* st, const void* w, const void* bias, void* g, int B, int H, int W, int k, int dtype, void* stream);
int tc_sa_conv_bwd(const void* dg, const void* g, const void* st, const void* w, void* dst, float* dw, float* db, int B, int H, int W, int k,
                   int dtype, void* stream);
int tc_pix_gate_fwd(const void* x, int ldx, const void* g, void* y, int ldy, int rows, int C, int dtype, void* stream);
int tc_pix_gate_bwd(const void* dy, int lddy, const void* x, int ldx, const void* g, void* dx, int lddx, int dx_accumulate, void* dg, int rows, int C,
                    int dtype, void* stream);

/* CAM_Module (the concat = "cam" aggregate, MSTr.py:464-509): x is [B*N, 4*C], the four branch maps side by side (column p*C + c).  Per image and
 * channel the 4 x 4 path energy E = x^T x over the tokens, A = softmax(rowmax(E) - E) (att: fp32 [B][C][16]), y = gamma (A x) + x.
 * tc_cam_bwd: dx (+)= the gradient through the residual, the attention-weighted sum and the energy; dgamma (fp32 [1]) ACCUMULATED; att2 is
 * fp32 scratch [B][C][16]. */
int tc_cam_att_fwd(const void* x, int ldx, float* att, int B, int N, int C, int dtype, void* stream);
int tc_cam_apply_fwd(const void* x, int ldx, const float* att, const float* gamma, void* y, int ldy, int B, int N, int C, int dtype, void* stream);
int tc_cam_bwd(const void* x, int ldx, const void* dy, int lddy, const float* att, const float* gamma, float* att2, float* dgamma, void* dx, int lddx,
               int dx_accumulate, int B, int N, int C, int dtype, void* stream);
/* y = gamma * a + x with gamma an fp32 device scalar (the residual scale of CAM_Module / CAM_Factorized_Module, MSTr.py:508, 566);
 * backward: da = gamma dy, dx (+)= dy, dgamma (fp32 [1]) += sum dy (.) a */
int tc_gamma_res_fwd(const void* a, int lda, const void* x, int ldx, const float* gamma, void* y, int ldy, int rows, int C, int dtype, void* stream);
int tc_gamma_res_bwd(const void* dy, int lddy, const void* a, int lda, const float* gamma, void* da, int ldda, void* dx, int lddx, int dx_accumulate,
                     float* dgamma, int rows, int C, int dtype, void* stream);
/* y = GELU(x) (nn.GELU(): exact erf form in fp32; bf16 / fp16 storage takes the polynomial CDF described at TcFfnFused, within 1.02e-5 |x| of
 * it) and dz = dy * GELU'(x) (erf form), elementwise (Conv3d + GELU of the "cam" aggregate, MSTr.py:625-628) */
int tc_gelu_fwd(const void* x, void* y, long long n, int dtype, void* stream);
int tc_gelu_bwd(const void* dy, const void* x, void* dz, long long n, int dtype, void* stream);

/* CoordAtt pooling MSTr.py:1327-1332.  pooled/att rows: first B*H rows (b,h) = mean over w, then B*W rows (b,w) = mean over h
 * (a row permutation of the reference's per-image cat; BatchNorm statistics over rows are unaffected). */
int tc_coord_pool_fwd(const void* x, void* pooled, int B, int H, int W, int C, int dtype, void* stream);
int tc_coord_pool_bwd(const void* dpooled, void* dx, int B, int H, int W, int C, int accumulate, int dtype,
                      void* stream);
/* CoordAtt gating MSTr.py:1345: y = x * a_w[b,w,:] * a_h[b,h,:]; att rows as for pooling ([B*H] a_h then [B*W] a_w) */
int tc_coord_gate_fwd(const void* x, const void* att, void* y, int B, int H, int W, int C, int dtype,
                      void* stream);
/* dx (+)= dy*a_w*a_h ; datt[b,h] = sum_w dy*x*a_w ; datt[b,H+w] = sum_h dy*x*a_h */
int tc_coord_gate_bwd(const void* dy, const void* x, const void* att, void* dx, int dx_accumulate,
                      void* datt, int B, int H, int W, int C, int dtype, void* stream);

/* Up to TC_EW_MULTI_MAX independent layout moves in one launch (Scale_reduce, MSTr.py:2225-2249: the three patchifies; the three
 * channel de-interleaves + the stage-4 token copy).  kind / fields (the arguments of the single-op entry points):
 *   TC_EW_PATCHIFY      a = map, sa = sb_map, lda = ld_map, b = cols, n0..n4 = B, H, W, C, k, flag = inverse      (tc_patchify)
 *   TC_EW_DEINTERLEAVE  a = in, b = out, sb = sbo, ldb = ldo, n0..n3 = B, P, C, mult, flag = inverse              (tc_sr_deinterleave)
 *   TC_EW_COPY          a = src, sa = sbs, lda = lds, b = dst, sb = sbd, ldb = ldd, n0..n2 = nb, rows, cols, flag = accumulate (tc_copy3d) */
#define TC_EW_MULTI_MAX 4
enum { TC_EW_PATCHIFY = 0, TC_EW_DEINTERLEAVE = 1, TC_EW_COPY = 2 };
typedef struct TcEwSeg {
    int kind, flag;
    const void* a; void* b;
    long long sa, sb;
    int lda, ldb, n0, n1, n2, n3, n4, reserved;
} TcEwSeg;
int tc_ew_multi(const TcEwSeg* segs, int nseg, int dtype, void* stream);

/* Pixel shuffle of PatchExpand / FinalPatchExpand_X4, MSTr.py:196-197,222-223:
 *   fwd: in [B,H,W,p*p*c] -> out [B,H*p,W*p,c] with channel index (p1*p + p2)*c + cc ; inverse=1 undoes it. */
int tc_pixel_shuffle(const void* in, void* out, int B, int H, int W, int p, int c, int inverse, int dtype,
                     void* stream);
/* Non-overlapping patch gather for the k=s patchify convs of Scale_reduce, MSTr.py:2215-2217,2233-2235:
 *   fwd: map [B,H,W,C] (batch stride sb_map, pixel stride ld_map) -> cols [B*(H/k)*(W/k), k*k*C] ordered (c,ky,kx) = the conv weight's [O, I*k*k] view;
 *   inverse=1 scatters cols back (the input gradient); inverse=2 adds them onto the map.
 *   16-bit storage with k = 2 / 4 / 8 and 16-byte aligned buffers moves whole 4 / 8 / 16-byte pieces (one filter row of a patch x four channels per thread). */
int tc_patchify(const void* map, long long sb_map, int ld_map, void* cols, int B, int H, int W, int C, int k,
                int inverse, int dtype, void* stream);
/* Channel de-interleave of Scale_reduce (Appendix C.4): out[b, g*P+pos, c] = in[b, pos, c*mult+g];
 *   out rows have stride ldo and batch stride sbo (written straight into the [B,784,64] K/V source buffer). */
int tc_sr_deinterleave(const void* in, void* out, long long sbo, int ldo, int B, int P, int C, int mult,
                       int inverse, int dtype, void* stream);
/* im2col for the 7x7 stride-4 pad-3 stem conv (MSTr.py:296,300) from an NCHW fp32/bf16 image with in_ch
 * channels (1 => the reference's x.repeat(1,3,1,1), MSTr.py:2828-2829, is folded in):
 *   cols [B*Ho*Wo, ldc] with column (ci*49 + ky*7 + kx), ci in 0..2, zero padded up to ldc. */
int tc_stem_im2col(const void* img, void* cols, int ldc, int B, int in_ch, int H, int W, int dtype, void* stream);
/* im2col / col2im of a 3x3 stride-2 pad-1 convolution -- the Conv2d_BN stem of MSViT_4Stages (Stage_3or4 = 4, MSTr.py:1793-1810; the product
 * is a tc_gemm with the [Cout, Cin*9] weight): cols [B*Ho*Wo, ldc], column c*9 + ky*3 + kx = x(b, 2 oy + ky - 1, 2 ox + kx - 1, c), zero
 * outside the map and up to ldc.  nchw != 0: x is an image [B, src_ch, H, W] (src_ch = 1 feeds every channel, MSTr.py:2828-2829), else
 * token-major rows [B*H*W, Cin] with row stride ldx.  tc_col2im3s2: dx (+)= the transposed gather of the column gradients. */
/* have_bridge = "sp" (BridgeBlock_sp, MSTr.py:2586-2757).  tc_window_rows: the window partition of SpatialAwareTrans (:2627-2640) and its
 * reverse (:2649-2658) as a row permutation between a token map [B*H*W, C] (row stride: lds / ldd) and the window-token matrix
 * [B*(H/ws)*(W/ws)*ntw, C]: pixel (b, wy ws + iy, wx ws + ix) <-> token off + iy ws + ix of window (b, wy, wx); dir 0: windows <- map,
 * dir 1: map (+)= windows.  C a multiple of 8.  tc_dropout: nn.Dropout of its MLP_FFN (:70, 75-77) in training mode, y = x keep / (1 - p) with
 * keep drawn from a counter-based generator keyed by (*seed_dev + salt, element index); the backward applies the same call to the gradient.
 * (The mask bits have no reference counterpart: torch draws them from its own generator.) */
int tc_window_rows(const void* src, int lds, void* dst, int ldd, int B, int H, int W, int ws, int ntw, int off, int C, int dir, int accumulate,
                   int dtype, void* stream);
int tc_dropout(const void* x, void* y, long long n, float p, const long long* seed_dev, unsigned salt, int dtype, void* stream);
int tc_im2col3s2(const void* x, int ldx, int nchw, int src_ch, void* cols, int ldc, int B, int Cin, int H, int W, int dtype, void* stream);
int tc_col2im3s2(const void* dcols, int ldc, void* dx, int lddx, int B, int Cin, int H, int W, int accumulate, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-step kernels (trainer.py:123-153, utils.py:11-47).
 */
/* Per-pixel softmax over classes; accumulates into sums[0]=sum CE, sums[1+3c..]=intersect_c, y_sum_c, z_sum_c.
 * logits NCHW [B,ncls,HW] (storage dtype), labels int64 [B,HW]; prob (fp32 [B,ncls,HW]) saved for backward. */
int tc_seg_loss_fwd(const void* logits, const long long* labels, float* prob, float* sums, int B, int ncls,
                    int HW, int dtype, void* stream);
/* out3 = {w_ce*CE + w_dice*Dice, CE, Dice} from the (all-reduced) forward sums, evaluated in double on the device
 * (trainer.py:141-143: loss = 0.4*loss_ce + 0.6*loss_dice; utils.py:34-47: smooth 1e-5, mean over classes).  One launch in
 * place of the sixteen scalar ones of the host expression. */
int tc_seg_loss_value(const float* sums, int ncls, double n_pix_global, double w_ce, double w_dice, float* out3, void* stream);
/* dlogits for loss = w_ce*CE_mean + w_dice*mean_c(1 - (2I+eps)/(Z+Y+eps)); sums are the (all-reduced) forward sums;
 * n_pix_global = global pixel count for the CE mean. */
int tc_seg_loss_bwd(const float* prob, const long long* labels, const float* sums, void* dlogits, int B, int ncls,
                    int HW, float w_ce, float w_dice, float n_pix_global, float gscale, const float* gscale_dev, int dtype,
                    void* stream);
/* The same two kernels on TOKEN-MAJOR logits / dlogits [B*HW, ld] (rows = pixels, ld >= ncls elements of the storage type), the layout
 * the classifier Linear (MSTr.py:281 last_layer) leaves: the captured training step skips the NHWC -> NCHW transpose and the fp32 copy
 * of the logits, and their counterparts on the way back (trainer.py:139-143 see the same values).  prob, when given, is [B, ncls, HW] fp32.
 * 16-bit rows that are 16-byte aligned and padded to a multiple of 8 elements (tc_ln_cls_fwd's padded logits) are read and written as whole
 * 16-byte pieces: the pad elements of dlogits are then written as zeros; any other row pitch is accessed element by element, padding untouched. */
int tc_seg_loss_fwd_tok(const void* logits, int ld, const long long* labels, float* prob, float* sums, int B, int ncls, int HW, int dtype,
                        void* stream);
int tc_seg_loss_bwd_tok(const float* prob, const void* logits, int ldl, const long long* labels, const float* sums, void* dlogits, int ld,
                        int B, int ncls, int HW, float w_ce, float w_dice, float n_pix_global, float gscale, const float* gscale_dev,
                        int dtype, void* stream);
/* prob may be NULL in both: the forward then only accumulates the sums, the backward recomputes the softmax from `logits` (row pitch ldl)
 * with the forward's operations in the forward's order -- 29 MB of fp32 probabilities less to write and read at B = 16, 224 x 224. */
/* The class-weighted loss with ignore_index: the arguments the reference's loss classes take beyond their defaults -- the `weight` and
 * `ignore_index` of the CrossEntropyLoss it constructs (trainer.py:123, applied at trainer.py:141) and the per-class `weight` of
 * DiceLoss.forward (utils.py:34-47: weight at :38-39, `loss += dice * weight[i]` at :46, `/ n_classes` at :47):
 *   CE   = sum_i w_ce[y_i] nll_i / sum_i w_ce[y_i]                                       over the pixels whose label is not ignore_index
 *   Dice = sum_k w_dice[k] (1 - (2 I_k + 1e-5) / (Z_k + Y_k + 1e-5)) / ncls              an ignored pixel enters none of I, Y, Z
 * weights: float[2 * ncls] on the device, CE weights then Dice weights; NULL = all ones.  ignore_index: a label value outside [0, ncls)
 * (an index inside it is TC_ERR_ARG), or TC_IGNORE_NONE for none.  ncls <= 16.
 * ONE pair of entries serves both layouts: ld = 0 is NCHW logits / dlogits [B, ncls, HW] (tc_seg_loss_fwd / _bwd; prob is then required),
 * ld >= ncls is token-major rows [B * HW, ld] (tc_seg_loss_fwd_tok / _bwd_tok, with the same 16-byte-piece path for aligned padded 16-bit
 * rows, pad elements of dlogits written as zeros, and the same prob == NULL recompute from `logits` of row pitch ldl).
 * The sums vector keeps its layout and meaning except sums[0] = sum_i w_ce[y_i] nll_i: I, Y, Z are unweighted, so ranks all-reduce the same
 * 1 + 3 ncls floats, and the CE denominator is formed from them as sum_k w_ce[k] Y_k -- no pixel count is passed.  The fp32 Y_k are whole
 * numbers: the denominator is exact only while the GLOBAL number of counted pixels stays below 2^24.
 * Zero denominator (every pixel ignored, or only zero-weight classes present): CE and its gradient are 0, NOT the NaN of torch -- a NaN
 * would read as an overflow to the loss-scale guard of tc_sgd_step_multi and skip the update silently.
 * Backward: dlogits of an ignored pixel is WRITTEN as exact zeros in every class; per pixel the CE factor is (w_ce / denominator) * w_ce[y_i]
 * in that order, so that with all-ones weights and no ignore_index dlogits and prob are bit-equal to the plain entries' (the atomically
 * accumulated sums agree to rounding).  gscale / gscale_dev as in tc_seg_loss_bwd.  A label outside [0, ncls) that is not ignore_index is
 * not supported (as in the plain entries). */
#define TC_IGNORE_NONE (-2147483647 - 1)
int tc_seg_loss_fwd_w(const void* logits, int ld, const long long* labels, const float* weights, int ignore_index, float* prob, float* sums,
                      int B, int ncls, int HW, int dtype, void* stream);
int tc_seg_loss_value_w(const float* sums, const float* weights, int ncls, double w_ce, double w_dice, float* out3, void* stream);
int tc_seg_loss_bwd_w(const float* prob, const void* logits, int ldl, const long long* labels, const float* weights, int ignore_index,
                      const float* sums, void* dlogits, int ld, int B, int ncls, int HW, float w_ce, float w_dice, float gscale,
                      const float* gscale_dev, int dtype, void* stream);
/* Fused core of FactorAtt_ConvRelPosEnc (MSTr.py:864-877), one workgroup per (image, head):
 *   o = scale * q (softmax_N(k)^T v) + q (.) convv        q, k, v: column slices (row stride ld) of the [Bt*N, 3C] qkv buffer,
 * head h owning channels [h*Ch, (h+1)*Ch); convv = crpe(v) (row stride ldc).  stats: tc_factor_att_stats_floats() floats saved for
 * the backward (column max and 1/sum of the key softmax).  Backward: dq/dk/dv share the row stride ldd (slices of the qkv
 * gradient; acc_* = add to what is there), dconvv is overwritten.  Replaces 5 forward + 7 backward launches of the unfused form. */
TC_QUERY long long tc_factor_att_stats_floats(int Bt, int heads, int Ch);
/* The attention half of an MHCABlock after norm1 in one launch (16-bit storage; C = 64 / 128 / 320 with 8 heads; N = H * W tokens per
 * image small enough for one head's tiles to sit in LDS -- ask tc_mhca_att_supported): per (image, head)
 *   q | k | v = xn Wqkv_h^T + b_h (nn.Linear(C, 3C), MSTr.py:856-862), convv = crpe_h(v) (ConvRelPosEnc, :801-823: heads 0-1 3x3, 2-4 5x5,
 *   5-7 7x7 depthwise windows, weights w3 / w5 / w7 [nh*Ch, 1, k, k] + biases), o = scale q (softmax_N(k)^T v) + q (.) convv (:864-877).
 * xn [groups*B*N, C] (row stride ldx); qkv [.., 3C], convv, o [.., C] and stats (tc_factor_att_stats_floats(groups*B, 8, C/8) floats) are
 * written as tc_gemm + tc_dwconv_multi + tc_factor_att_fwd would leave them (their backward entries apply unchanged).  Parameters of
 * weight group g (the three MB paths) at +g*gs elements. */
/* tc_mhca_att_bwd: the backward of the crpe window and the attention core for the same layout in one launch per (image, head) -- what
 * tc_factor_att_bwd followed by tc_dwconv_multi (mode 3) compute: dq | dk | dv into dqkv [.., 3C] (row stride ldd; acc_* = add to what is
 * there), the window's weight / bias gradients ADDED to dw3 / db3 / dw5 / db5 / dw7 / db7 (fp32, laid out like the weights, group g at
 * +g*gs).  go = d loss / d o.  dconvv is not materialised. */
TC_QUERY int tc_mhca_att_supported(int C, int N, int dtype);
/* tc_dw_ln_fwd: the head of an MHCABlock in one launch (16-bit storage, C = 64 / 128 / 320): t1 = x + dw3x3(x) + bias (ConvPosEnc,
 * MSTr.py:744-752), xn = LayerNorm_C(t1) (norm1, :932, 937), mean / rstd [groups*B*H*W] as tc_layernorm_fwd leaves them.  Parameters of
 * weight group g at +g*wstride (conv) / +g*gstride (norm).  Backward: tc_layernorm_bwd*, then tc_dwconv_bwd -- unchanged. */
TC_QUERY int tc_dw_ln_supported(int C, int dtype);
int tc_dw_ln_fwd(const void* x, int ldx, const void* w, const void* b, long long wstride, const void* gamma, const void* beta,
                 long long gstride, void* t1, int ldt, void* xn, int ldn, float* mean, float* rstd, int groups, int B, int H, int W,
                 int C, float eps, int dtype, void* stream);
TC_QUERY int tc_mhca_att_bwd_supported(int C, int N, int dtype);
int tc_mhca_att_bwd(const void* qkv, int ldq, const void* convv, int ldc, const void* go, int ldgo, const float* stats, void* dqkv,
                    int ldd, int acc_q, int acc_k, int acc_v, const void* w3, const void* w5, const void* w7, float* dw3, float* db3,
                    float* dw5, float* db5, float* dw7, float* db7, long long gs, int groups, int B, int H, int W, int C, float scale,
                    int dtype, void* stream);
int tc_mhca_att_fwd(const void* xn, int ldx, const void* Wqkv, const void* bqkv, const void* w3, const void* b3, const void* w5,
                    const void* b5, const void* w7, const void* b7, long long gs, void* qkv, int ldq, void* convv, int ldc,
                    void* o, int ldo, float* stats, int groups, int B, int H, int W, int C, float scale, int dtype, void* stream);
int tc_factor_att_fwd(const void* q, const void* k, const void* v, int ld, const void* convv, int ldc, void* o, int ldo,
                      float* stats, int Bt, int N, int heads, int Ch, float scale, int dtype, void* stream);
int tc_factor_att_bwd(const void* q, const void* k, const void* v, int ld, const void* convv, int ldc, const void* go, int ldgo,
                      const float* stats, void* dq, void* dk, void* dv, int ldd, int acc_q, int acc_k, int acc_v, void* dconvv,
                      int lddc, int Bt, int N, int heads, int Ch, float scale, int dtype, void* stream);

/* Evaluation (utils.py:72-76 argmax(softmax(logits)), :50-60,96-97 per-class Dice): pred[b,p] = argmax_k
 * logits[b,k,p] as uint8; with labels (int64 [B,HW]) also counts[3k..3k+2] += (|pred==k & gt==k|, |pred==k|, |gt==k|), fp32,
 * ACCUMULATED.  ncls <= 16. */
int tc_argmax_counts(const void* logits, const long long* labels, unsigned char* pred, float* counts, int B, int ncls, int HW,
                     int dtype, void* stream);

/* Evaluation metrics on the device (csrc/metrics.hip): the integer side of calculate_metric_percase (utils.py:50-60, called per class at
 * utils.py:96-98: medpy's dc and hd95 with defaults, i.e. unit voxel spacing, connectivity 1) for a predicted label volume against a
 * ground-truth one, both uint8 [D,H,W] in HBM.  Definition, as oracle.transception_oracle.eval_hd95 states it:
 *   - surface voxel of a mask = mask voxel with at least one of its 6 face neighbours outside the mask, the outside of the array counting
 *     as background (scipy binary_erosion, border_value 0), so every mask voxel of a [1,H,W] volume is on its surface;
 *   - for every surface voxel of A the Euclidean distance to the nearest surface voxel of B, and the other way round, both lists pooled;
 *   - HD95 = numpy.percentile(pooled, 95), linear interpolation between the two neighbouring order statistics;
 *   - utils.py:53-60: both masks non-empty -> (dice, hd95); only the prediction non-empty -> (1, 0); else (0, 0)  (the host applies it).
 * Squared distances are integers, so all of it is exact int32 work with integer atomics: bit-identical from run to run.
 * Limits (TC_ERR_ARG beyond them, as for null pointers; nothing is launched): D, H, W in 1..2048, D*H*W < 2^31, ncls in 1..16,
 * class k in 1..15 (and k < ncls where ncls is passed).  zfaces = 1 is a 3-D volume; zfaces = 0 treats every z-slice as a 2-D image of
 * its own (no z neighbours, no z pass): what an [H,W] pair means to hd95, passed with D = 1.
 *
 * tc_metric_surfaces: surf[v] = lab[v] if v is a surface voxel of class lab[v] (1 <= lab[v] < ncls), else 0, for both volumes (uint8
 *   [D,H,W] each, OVERWRITTEN), and counts[3k..3k+2] += (|P==k & G==k|, |P==k|, |G==k|) for k < ncls: int64, ACCUMULATED -- the caller
 *   zeroes them (the same rule as tc_argmax_counts).
 * tc_metric_edt: d2[v] = squared Euclidean distance from v to the nearest voxel with surf == k, int32 [D,H,W], OVERWRITTEN; exact
 *   (separable: nearest source within the row, then min_j f[j] + (i-j)^2 along y and z, in place).  TC_METRIC_NO_SOURCE everywhere when
 *   no voxel has surf == k (with zfaces = 0: in every slice without one).
 * tc_metric_hist: hist[k][d2_gt[v]] += 1 for every v with surf_pred[v] == k and hist[k][d2_pred[v]] += 1 for every v with
 *   surf_gt[v] == k; hist is uint32 [ncls][nbins], ACCUMULATED -- the caller zeroes it; nbins >= tc_metric_hist_bins(D,H,W) =
 *   (D-1)^2 + (H-1)^2 + (W-1)^2 + 1 (0 for a shape outside the limits).  Distances to an empty surface are not counted.
 * tc_metric_select: out[3k..3k+2] = (n, d2_lo, d2_hi), int64, OVERWRITTEN for every k < ncls: the pooled count of hist[k] and the squared
 *   distances at sorted positions floor(0.95 (n-1)) and min(that + 1, n-1); (0, 0, 0) for an empty histogram.  The host forms
 *   sqrt(d2_lo) + (sqrt(d2_hi) - sqrt(d2_lo)) * (0.95 (n-1) - floor(0.95 (n-1))) in fp64. */
#define TC_METRIC_NO_SOURCE (1 << 28)
TC_QUERY long long tc_metric_hist_bins(int D, int H, int W);
int tc_metric_surfaces(const unsigned char* pred, const unsigned char* gt, unsigned char* surf_pred, unsigned char* surf_gt,
                       long long* counts, int D, int H, int W, int ncls, int zfaces, void* stream);
int tc_metric_edt(const unsigned char* surf, int k, int* d2, int D, int H, int W, int zfaces, void* stream);
int tc_metric_hist(const unsigned char* surf_pred, const unsigned char* surf_gt, const int* d2_pred, const int* d2_gt, int k,
                   unsigned int* hist, long long nbins, int ncls, int D, int H, int W, void* stream);
int tc_metric_select(const unsigned int* hist, long long nbins, int ncls, long long* out, void* stream);

/* The same metric with anisotropic voxel spacing (sz, sy, sx), each finite and > 0, in the units of the result (medpy's voxelspacing, in
 * array axis order): distance^2 = (sz dz)^2 + (sy dy)^2 + (sx dx)^2 is no integer, so the maps are fp64 and the order statistics come
 * from a radix select over bit patterns, not from a histogram indexed by the distance.  Surfaces and counts do not depend on spacing:
 * tc_metric_surfaces serves both forms.  Same limits (D, H, W in 1..2048, fewer than 2^31 voxels, k in 1..15 and k < ncls where ncls is
 * passed), same meaning of zfaces (0: sz is not used), same error rule; a spacing that is not finite and > 0 is TC_ERR_ARG.
 *
 * tc_metric_edt_f64: d2[v] = min over voxels u with surf == k of (sz dz)^2 + (sy dy)^2 + (sx dx)^2, double [D,H,W], OVERWRITTEN
 *   (separable: (sx dx)^2 to the nearest source within the row, then min_j f[j] + (s (i-j))^2 along y and z, in place; the sum is
 *   formed in the order x, y, z, each term rounded once or fused into the add).  +inf everywhere when no voxel has surf == k (with
 *   zfaces = 0: in every slice without one).
 * tc_metric_select_f64: for ONE class k, out[3k..3k+2] = (n, d2_lo, d2_hi), OVERWRITTEN (the other classes' records are not touched):
 *   n (long long) counts the pooled multiset { d2_gt[v] : surf_pred[v] == k } + { d2_pred[v] : surf_gt[v] == k } without its +inf
 *   members (distances to an empty surface), and the next two 8-byte slots hold, AS DOUBLES, its elements at sorted positions
 *   floor(0.95 (n-1)) and min(that + 1, n-1); (0, 0.0, 0.0) for an empty multiset.  Exact: non-negative doubles order like their bit
 *   patterns, and eight passes of 8-bit integer histograms (most significant digit first) pin both elements; integer atomics only, so
 *   the result is bit-identical from run to run.  work: TC_METRIC_SELECT_WORK_BYTES of device memory, 8-byte aligned, OVERWRITTEN
 *   (zeroed by the entry; one buffer serves every class on one stream).  The host forms the percentile as for tc_metric_select. */
#define TC_METRIC_SELECT_WORK_BYTES 16448
int tc_metric_edt_f64(const unsigned char* surf, int k, double* d2, int D, int H, int W, int zfaces, double sz, double sy, double sx,
                      void* stream);
int tc_metric_select_f64(const unsigned char* surf_pred, const unsigned char* surf_gt, const double* d2_pred, const double* d2_gt, int k,
                         int ncls, int D, int H, int W, void* work, long long* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Input pipeline (datasets/dataset_synapse.py:101-112, trainer.py:89-93): a batch of raw slices
 * [B,H,W] (image fp32 in [0,1], label uint8 0..8) already in HBM -> network input.
 */
enum { TC_AUG_WARP = 1, TC_AUG_LINEAR = 2, TC_AUG_BLUR = 4, TC_AUG_PIECEWISE = 8,
       TC_AUG_SKIP = 1 << 20, TC_AUG_FROM_RAW = 1 << 21 };      /* (rounds of a chain only, see tc_slice_augment_chain) */
/* Per-slice augmentation record (DEVICE array of B).  Stage order: warp first, then the pixel stages in the order `reserved` encodes
 *   (imgaug's SomeOf(random_order=True) applies its augmenters in the drawn order, dataset_synapse.py:84-95): up to three 2-bit codes,
 *   first stage in the low bits, 1 = blur, 2 = contrast, 3 = noise; reserved = 0 means blur -> contrast -> noise.
 *   warp: source (row, col) = (m[2] + m[0] y' + m[1] x', m[5] + m[3] y' + m[4] x') of output pixel (y, x), where (y', x') = (y, x)
 *   plus, with TC_AUG_PIECEWISE, the piecewise-affine displacement of imgaug's PiecewiseAffine = skimage's PiecewiseAffineTransform
 *   (dataset_synapse.py:93): control points linspace(0, H, 4) x linspace(0, W, 4) moved by disp[(gy*4+gx)*2 + {0:dy,1:dx}] (pixels,
 *   already clipped into the image as imgaug clips them); every cell of the grid is two triangles -- bit 8 + gy*3 + gx of `flags` set:
 *   split along the top-right / bottom-left diagonal, clear: top-left / bottom-right (the host takes this from the Delaunay
 *   triangulation of the grid, as skimage does) -- and a pixel moves by the barycentric mix of its triangle's three corner displacements;
 *   image sampled order 1 (TC_AUG_LINEAR) or order 0, label always order 0, outside -> 0
 *   (scipy.ndimage mode='constant': dataset_synapse.py:48-52 rotate, :39-46 rot90/flip; imgaug Affine family :90-94).
 *   blur: Gaussian sigma 1, 9 taps, mirror border (:88).  contrast: center + alpha (v - center) (:89).
 *   noise: v += noise_sigma * N(0,1), counter-based generator keyed by (noise_seed, pixel) (:87). */
typedef struct TcSliceAug {
    double m[6];
    float disp[32];
    float alpha, center, noise_sigma;
    unsigned int noise_seed;
    int flags;
    int reserved;
} TcSliceAug;
/* img/lab [B,H,W] -> img_out/lab_out (distinct buffers).  H, W >= 9. */
int tc_slice_augment(const float* img, const unsigned char* lab, const TcSliceAug* aug_dev, float* img_out,
                     unsigned char* lab_out, int B, int H, int W, void* stream);
/* The stage chains of a batch (imgaug's SomeOf((0, 4), ..., random_order=True), dataset_synapse.py:84-95: every drawn augmenter resamples the
 * previous one's result) as rounds [first_round, rounds) of launches: aug_dev [rounds][B]; round r writes buffer a (r even) or b (r odd) and
 * reads the other one, or the raw slice where the record says TC_AUG_FROM_RAW (the first stage of a slice's chain); a record with TC_AUG_SKIP
 * does nothing (the slice's chain has not started: chains END in the last round, so that the result of every slice lies in the buffer of
 * round rounds - 1 and no identity copy is needed in between; a slice without stages is copied there once, by a plain FROM_RAW record). */
int tc_slice_augment_chain(const float* raw_img, const unsigned char* raw_lab, const TcSliceAug* aug_dev, int first_round, int rounds,
                           float* img_a, unsigned char* lab_a, float* img_b, unsigned char* lab_b, int B, int H, int W, void* stream);
/* Cubic B-spline coefficients (fp64 [B,H,W]) of fp32 slices: the prefilter half of scipy.ndimage.zoom(order=3)
 * (dataset_synapse.py:111), mirror boundaries, axis 0 then axis 1. */
int tc_spline_prefilter(const float* img, double* coef, int B, int H, int W, void* stream);
/* x[b,0,oy,ox] = (zoom3(img)[oy,ox] - mean) / std ; y[b,oy,ox] = zoom0(lab)[oy,ox] (int64) with scipy's grid
 * (source coordinate o*(in-1)/(out-1) in double; a coordinate that rounds above in-1 yields 0 for image and label -- at 512->224
 * that is the whole last row and column, as in the reference).  coef = NULL requires OH==H, OW==W and only normalises img
 * (the reference skips the zoom for equal sizes, dataset_synapse.py:109).  y/lab may be NULL. */
int tc_zoom_normalize(const double* coef, const float* img, const unsigned char* lab, float* x, long long* y, int B, int H,
                      int W, int OH, int OW, float mean, float stdv, void* stream);

/* Fused SGD with momentum and weight decay over flat fp32 buffers (torch.optim.SGD semantics, trainer.py:125):
 *   g = grad*gscale + wd*p ; buf = first ? g : mom*buf + g ; p -= lr*buf.
 * lr_dev (optional device scalar) overrides lr, so a hipGraph-captured step can follow a per-iteration schedule. */
int tc_sgd_step(float* p, const float* grad, float* buf, long long n, float lr, const float* lr_dev, float momentum,
                float wd, float gscale, int first, void* stream);
/* The same update over nseg contiguous segments of the flat arenas in ONE launch: segs_dev is a DEVICE array of
 * (offset, length) pairs (elements); max_len = longest segment.  Parameters outside the segments are untouched
 * (torch.optim.SGD skips parameters whose grad is None -- the reference's 332 grad-less tensors). */
/* clip_sumsq (optional device scalar = sum of squared gradients, see tc_grad_sumsq): gradients are additionally scaled by
 * min(1, clip_norm / (sqrt(*clip_sumsq) + 1e-6)) -- nn.utils.clip_grad_norm_(parameters, clip_norm, 2) of trainer.py:147-148 folded
 * into the update (the stored gradients themselves stay unscaled). */
/* lp (optional, lp_dtype TC_BF16 / TC_F16): the 16-bit working copy of the parameters, same indexing as p -- the updated values are
 * stored there too, so the next forward needs no cast pass over the arena. */
int tc_sgd_step_multi(float* p, const float* grad, float* buf, const long long* segs_dev, int nseg, long long max_len,
                      float lr, const float* lr_dev, float momentum, float wd, float gscale, int first, const float* clip_sumsq,
                      float clip_norm, void* lp, int lp_dtype, void* stream);
/* ---- Dynamic loss scaling for float16 storage, entirely on the device (nothing here synchronises, allocates or reads back).
 * A LOSS-SCALE STATE is four 32-bit words in device memory, owned by the caller:
 *     [0] fp32   scale                      (the loss gradient is multiplied by it: hand &state[0] to tc_seg_loss_bwd* as gscale_dev)
 *     [1] fp32   1 / scale                  (rewritten whenever the scale is)
 *     [2] int32  growth tracker: clean steps since the scale last changed
 *     [3] int32  updates skipped so far
 *
 * tc_sgd_step_multi_scaled = tc_sgd_step_multi on gradients that carry the state's scale: gscale is multiplied by state[1], and the
 * clip coefficient is min(1, clip_norm * state[0] / (sqrt(*clip_sumsq) + 1e-6)), so clip_norm bounds the norm of the TRUE gradient.
 * clip_sumsq is mandatory (TC_ERR_ARG without it; clip_norm = inf for no clipping): a non-finite *clip_sumsq leaves p, buf and lp as
 * they were, exactly as in tc_sgd_step_multi.  With scale a power of two the result is bit-equal to tc_sgd_step_multi called with
 * gscale / scale and clip_norm * scale. */
int tc_sgd_step_multi_scaled(float* p, const float* grad, float* buf, const long long* segs_dev, int nseg, long long max_len,
                             float lr, const float* lr_dev, float momentum, float wd, float gscale, int first,
                             const float* clip_sumsq, float clip_norm, void* lp, int lp_dtype, const float* scale_state, void* stream);
/* The scale's own step, launched after the update kernel of the same training step; *sumsq is what tc_grad_sumsq left.
 *     *sumsq not finite (inf or NaN):  scale = max(scale * backoff, min_scale) ; tracker = 0 ; skipped += 1
 *     *sumsq finite:                   tracker += 1 ; when it reaches interval:  scale = min(scale * growth, max_scale) ; tracker = 0
 * and state[1] = 1 / scale.  This is torch.amp.GradScaler.update's rule with the two clamps added.
 * growth >= 1, 0 < backoff < 1, interval >= 1, 0 < min_scale <= max_scale, all finite (TC_ERR_ARG otherwise). */
int tc_loss_scale_update(float* state, const float* sumsq, float growth, float backoff, int interval, float min_scale,
                         float max_scale, void* stream);
/* ---- Fused Adam / AdamW over the flat arenas, with its step count on the device (a captured kernel's scalar arguments are frozen at
 * capture, and the bias correction depends on the step number).
 * An ADAM STATE is four 32-bit words in device memory, owned by the caller (all zero before the first update):
 *     [0] int32  t: updates applied so far; skipped updates are not counted
 *     [1] fp32   1 - beta1^t
 *     [2] fp32   sqrt(1 - beta2^t)
 *     [3] int32  reserved, written as 0
 *
 * tc_adam_advance, launched BEFORE the update kernel of the same step: sumsq == NULL or *sumsq finite: t += 1 and words 1, 2 recomputed
 * in double from the double betas, each rounded once to fp32; *sumsq inf or NaN: the state stays exactly as it was (tc_adam_step_multi
 * skips the same step).  0 <= beta < 1 (TC_ERR_ARG otherwise). */
int tc_adam_advance(float* state, const float* sumsq, double beta1, double beta2, void* stream);
/* One launch over the (offset, length) segment table of tc_sgd_step_multi.  With c = gscale x the clip coefficient x (scale_state[1] if
 * given), formed exactly as in tc_sgd_step_multi(_scaled), and wd_s = wd_dev[segment] when wd_dev is given, else wd:
 *     decoupled != 0 (torch.optim.AdamW):  w1 = w * (1 - lr*wd_s) ;  gh = g*c
 *     decoupled == 0 (torch.optim.Adam):   w1 = w ;                  gh = g*c + wd_s*w
 *     m' = beta1*m + (1-beta1)*gh ;  v' = beta2*v + (1-beta2)*gh*gh
 *     w' = w1 - (lr / adam_state[1]) * m' / (sqrt(v') / adam_state[2] + eps)
 * float(beta) and float(1 - beta) are each rounded once from the double arguments; division and square root are correctly rounded.
 * adam_state must have been advanced at least once (word 1 is 0 before).  lr_dev overrides lr; a non-finite *clip_sumsq returns before
 * touching p, m, v or lp; scale_state (a loss-scale state) requires clip_sumsq, and clip_norm * scale_state[0] then bounds the norm of the
 * TRUE gradient; lp (TC_BF16 / TC_F16) receives the rounded w'; elements outside the segments are never read or written.
 * TC_ERR_ARG: a beta outside [0, 1), eps <= 0, nseg <= 0, an unknown lp_dtype with lp set, adam_state == NULL, scale_state without
 * clip_sumsq. */
int tc_adam_step_multi(float* p, const float* grad, float* m, float* v, const long long* segs_dev, const float* wd_dev, int nseg,
                       long long max_len, float lr, const float* lr_dev, double beta1, double beta2, float eps, float wd, int decoupled,
                       float gscale, const float* clip_sumsq, float clip_norm, void* lp, int lp_dtype, const float* scale_state,
                       const float* adam_state, void* stream);
/* *out += sum_i g[i]^2 over a flat fp32 buffer (n a multiple of 4, 16-byte aligned): the squared total gradient norm. */
int tc_grad_sumsq(const float* g, long long n, float* out, void* stream);
/* p[0..n) = v (fp32): resets device accumulators inside a captured step */
int tc_fill_f32(float* p, long long n, float v, void* stream);
/* dst(bf16) = src(fp32) and back, for bf16 working copies of fp32 master weights */
int tc_cast(const void* src, void* dst, long long n, int src_dtype, int dst_dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * RIPM (Patch_Embed_stage of DWConv2d_BN, MSTr.py:704-732 / 309-362): one DWConv2d_BN step per launch (16-bit storage, C = 64 / 128 / 320).
 *   bn_in = 0:  x = xin                                   (step 0: the previous stage's map, stride 2)
 *   bn_in = 1:  x = Hardswish(BatchNorm(xin))             (xin = the raw 1x1 output of the previous step; training: batch statistics folded
 *               from part_in -- tc_bn_fwd's scratch with chunks_in row chunks, as left by the previous call -- save_mean / save_rstd [C]
 *               written and running_mean / running_var updated (momentum) as tc_bn_fwd does; eval: the running statistics) and x is ALSO
 *               written to xnorm [B*Hi*Wi, C] (row stride ldn): the map the step's other consumers read;
 *   y = dw3x3(x, stride, pad 1, no bias) [B*Ho*Wo, C]   z = y wp^T [.., C] (wp = nn.Conv2d(C, C, 1) weight [C, C], no bias)
 *   part_out = shift[C] | S1[T][C] | S2[T][C], T = tc_ripm_tiles(B, Ho, Wo): sums of (z - shift) and (z - shift)^2 per 8 x 8-pixel tile
 *   (shift = shift_out[C] or 0) -- pass it to tc_bn_fwd(stats_chunks = T) / the next tc_ripm_fwd(part_in, chunks_in = T).
 * Backward: tc_bn_bwd, tc_gemm_pair, tc_dwconv_bwd* on the tensors left here -- unchanged. */
TC_QUERY int tc_ripm_supported(int C, int dtype);
TC_QUERY int tc_ripm_tiles(int B, int Ho, int Wo);
int tc_ripm_fwd(const void* xin, int ldx, int bn_in, const float* part_in, int chunks_in, const void* gamma, const void* beta,
                float* running_mean, float* running_var, float* save_mean, float* save_rstd, float eps, float momentum,
                int training, void* xnorm, int ldn, const void* wd, const void* wp, void* y, int ldy, void* z, int ldz,
                float* part_out, const float* shift_out, int B, int Hi, int Wi, int C, int stride, int dtype, void* stream);

/* Square Linear + residual + LayerNorm in one launch (16-bit storage, C = 64 / 128 / 320): t = x W^T + b + res (res may be NULL),
 * xn = LayerNorm_C(t) with mean / rstd [groups*rows] as tc_layernorm_fwd leaves them -- nn.Linear(C, C) `proj` + skip + norm2 of an MHCABlock
 * (MSTr.py:883, 940-942) and of a bridge layer (:2288, 2404-2406), `reprojection` + skip + norm2 of an EfficientTransformerBlock (:141,
 * 167-170).  `groups` row blocks of `rows` rows, group g's parameters at +g*wstride (W, b) / +g*gstride (gamma, beta).  Every pointer
 * 16-byte aligned, ld* and both strides multiples of 8 elements (TC_ERR_ARG otherwise).  Backward: tc_layernorm_bwd*, then tc_gemm_pair --
 * unchanged. */
TC_QUERY int tc_linear_ln_supported(int C, int dtype);
int tc_linear_ln_fwd(const void* x, int ldx, const void* w, const void* b, long long wstride, const void* res, int ldr, const void* gamma,
                     const void* beta, long long gstride, void* t, int ldt, void* xn, int ldn, float* mean, float* rstd, int groups,
                     int rows, int C, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------
 * Legacy Transception encoder (networks/Transception.py, MiT_3inception, :362-551).  Every pointer 16-byte aligned, every C / Cin, row
 * stride and batch stride a multiple of 8 elements (TC_ERR_ARG otherwise); channels move in 16-byte pieces.  No atomics: the adjoints
 * gather, so their results are the same run to run.
 *
 * tc_im2col_dil: patches of a k x k convolution (k in {1, 3}) with any stride / pad / dilation -- the Conv2d of each
 * OverlapPatchEmbeddings_fuse branch (EffSegformer.py:117-131; 3x3 s2 p0 d2, 3x3 s2 p1 d1 and 1x1 s2 here).  x token-major [B*H*W, Cin]
 * (row stride ldx) -> cols [B*Ho*Wo, ldc], tap-major: column (ky*k + kx)*Cin + c = x(b, oy*stride - pad + ky*dil, ox*stride - pad + kx*dil, c),
 * zero outside the map; Ho = (H + 2 pad - dil (k - 1) - 1) / stride + 1.  The product with the [Cout, Cin, k, k] weight read as
 * [Cout, k*k*Cin] is the convolution.  tc_col2im_dil: dx (+)= for each input pixel the sum of the column gradients of the taps that read it. */
int tc_im2col_dil(const void* x, int ldx, void* cols, int ldc, int B, int Cin, int H, int W, int k, int stride, int pad, int dil, int dtype, void* stream);
int tc_col2im_dil(const void* dcols, int ldc, void* dx, int lddx, int B, int Cin, int H, int W, int k, int stride, int pad, int dil, int accumulate,
                  int dtype, void* stream);
/* tc_nearest_concat_fwd: the split of the normalised two-branch sequence, F.interpolate(branch 1, [Ho, Wo]) (mode nearest:
 * src = min((int)floorf(dst * (float)in / out), in - 1) per axis) and torch.cat((branch 1, branch 2), channels) (Transception.py:432-447,
 * 461-476, 490-505) in one gather: y [B*Ho*Wo, ldy], columns [0, C) branch 1 resampled, [C, 2C) branch 2.  Token t of image b of branch 1
 * ([H1*W1] tokens) lives at x1 + b*sb1 + t*ldx, of branch 2 ([Ho*Wo] tokens) at x2 + b*sb2 + t*ldx (elements): the per-image sequence
 * [B, n1+n2, C] is x2 = x1 + n1*ldx, sb1 = sb2 = (n1+n2)*ldx; branch-major rows are x2 = x1 + B*n1*ldx, sb1 = n1*ldx, sb2 = n2*ldx.
 * y feeds conv1_1_sK as one GEMM, or SK_Block with its two column halves as the two branch maps.
 * tc_nearest_concat_bwd: dx1 (+)= per branch-1 token the sum of the dy rows of the pixels that picked it; dx2 (+)= dy's second half. */
int tc_nearest_concat_fwd(const void* x1, long long sb1, const void* x2, long long sb2, int ldx, void* y, int ldy, int B, int H1, int W1, int Ho,
                          int Wo, int C, int dtype, void* stream);
int tc_nearest_concat_bwd(const void* dy, int ldy, void* dx1, long long sb1, void* dx2, long long sb2, int lddx, int B, int H1, int W1, int Ho,
                          int Wo, int C, int accumulate, int dtype, void* stream);

/* profiling aid: an empty launch of id + 1 workgroups that marks a section boundary in a kernel trace (no reference counterpart) */
int tc_seg_marker(int id, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRANSCEPTION_HIP_H */

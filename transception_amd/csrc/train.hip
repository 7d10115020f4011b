// Reductions and training-step kernels: bias-gradient column sums, the fused CE + Dice segmentation loss
// (trainer.py:141-143, utils.py:24-47), its class-weighted / ignore_index form (nn.CrossEntropyLoss(weight, ignore_index), trainer.py:141;
// DiceLoss.forward(weight=...), utils.py:34-47) and the fused SGD-momentum update (trainer.py:125).
#include "tc_common.h"
#include "../../include/transception_loss.h"
#include "../../include/transception_topk.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T* __restrict__ x, int rows, int cols, int ldx, float* __restrict__ out,
                                                     int nb, long long sb) {
    __shared__ float red[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + tx;
    float s = 0.f;
    if (c < cols)
        for (long long r = (long long)blockIdx.x * 4 + ty; r < (long long)rows * nb; r += (long long)gridDim.x * 4)
            s += ldf<T>(x + (r / rows) * sb + (r % rows) * ldx + c);
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && c < cols) atomicAdd(out + c, red[0][tx] + red[1][tx] + red[2][tx] + red[3][tx]);
}

constexpr int MAXCLS = 16;

// a token row of up to 16 classes whose storage is 16-byte aligned and padded to a multiple of 8 elements: one or two 16-byte pieces
template <typename T> __device__ __forceinline__ void tok_row_load(const T* lp, int ncls, float* v) {
    if constexpr (sizeof(T) == 2) {
        const uint4 a = *reinterpret_cast<const uint4*>(lp);
        tc_unpack16<T>(a, v);
        if (ncls > 8) {
            const uint4 b = *reinterpret_cast<const uint4*>(lp + 8);
            tc_unpack16<T>(b, v + 8);
        }
    }
}
template <typename T> __device__ __forceinline__ void tok_row_store(T* dp, int ncls, const float* v) {
    if constexpr (sizeof(T) == 2) {
        *reinterpret_cast<uint4*>(dp) = tc_pack16<T>(v);
        if (ncls > 8) *reinterpret_cast<uint4*>(dp + 8) = tc_pack16<T>(v + 8);
    }
}

// ld = 0: logits / dlogits are [B, ncls, HW] (the module's NCHW output); ld > 0: token-major [B * HW, ld] rows as the last Linear leaves
// them (the captured training step hands them over without the transpose and the fp32 copy); prob is [B, ncls, HW] either way
//
// WEIGHTED (the class-weighted / ignoring loss, tc_seg_loss_*_w) is a compile-time variant of the same bodies: every line it adds sits under
// `if constexpr (WEIGHTED)`, so the plain instantiations keep their instruction sequence and their bits.  weights: float[2 * ncls], CE weights
// then Dice weights, NULL = all ones, staged in LDS once per workgroup; ignore: the label value whose pixels are left out of every sum and get an
// exactly zero gradient (TC_IGNORE_NONE: no such label).  The forward needs the CE weights only -- I, Y, Z stay unweighted, so the sums vector
// and its all-reduce are what they were, and the CE denominator sum_k w_ce[k] Y_k is formed from the (global) sums where it is needed.
//
// FT (focal CE and Tversky overlap, tc_seg_loss_*_ft; include/transception_loss.h has the definition) is a further variant, of the WEIGHTED
// bodies: every line it adds sits under `if constexpr (FT)`, and its scalars travel in a last kernel argument that is an empty struct in the
// other instantiations, which therefore keep their instruction sequence too.  gamma and the overlap mode are run-time values.
template <bool FT> struct LossOpts {};
template <> struct LossOpts<true> { float gamma; int tversky; float alpha, beta; };
// TOPK (the top-k cross-entropy, tc_seg_loss_*_topk; include/transception_topk.h has the definition) is a further variant, of the FT bodies, in
// the same manner: every line it adds sits under `if constexpr (TOPK)` and its pointers travel in a last argument that is empty otherwise.  The
// forward stores each pixel's CE term in a value map instead of summing it; the backward weighs the CE gradient by the pixel's selection
// weight, which it takes from the stored value against the threshold t = state[5] and the tie share f = state[7] of tc_topk_select.
template <bool TOPK> struct TopkFwd {};
template <> struct TopkFwd<true> { float* values; };
template <bool TOPK> struct TopkBwd {};
template <> struct TopkBwd<true> { const float* values; const double* state; float inv_world; };

// the focal CE factor of a pixel: q^gamma, with gamma = 0 giving 1 for every q (q = 0 included)
__device__ __forceinline__ float focal_pow(float q, float gamma) { return gamma == 0.f ? 1.f : powf(q, gamma); }
// log max(p_t, 1e-38) of the focal variant.  p_t = 1 - q, so above p_t = 3/4 it is log1p(-q): p_t rounds to 1 for q below 6e-8 and its
// logarithm to 0, where the true value is -q.  Below, the logarithm of the clamped p_t as the other variants take it
__device__ __forceinline__ float focal_log_pt(float pt, float q) { return q < 0.25f ? log1pf(-q) : logf(fmaxf(pt, 1e-38f)); }

template <typename T, bool WEIGHTED, bool FT = false, bool TOPK = false>
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const T* __restrict__ logits, const long long* __restrict__ labels,
                                                           float* __restrict__ prob, float* __restrict__ sums, int B, int ncls, int HW, int ld,
                                                           const float* __restrict__ weights, int ignore, LossOpts<FT> ft, TopkFwd<TOPK> tk) {
    static_assert(WEIGHTED || !FT, "FT extends the WEIGHTED variant");
    static_assert(FT || !TOPK, "TOPK extends the FT variant");
    __shared__ float red[4][1 + 3 * MAXCLS];
    __shared__ float wce[WEIGHTED ? MAXCLS : 1];
    if constexpr (WEIGHTED) {
        if (threadIdx.x < ncls) wce[threadIdx.x] = weights ? weights[threadIdx.x] : 1.f;
        __syncthreads();
    }
    const bool vec16 = ld > 0 && !(ld & 7) && ld >= ((ncls + 7) & ~7) && !((uintptr_t)logits & 15);
    float ce = 0.f, I[MAXCLS], Y[MAXCLS], Z[MAXCLS];
#pragma unroll
    for (int k = 0; k < MAXCLS; ++k) I[k] = Y[k] = Z[k] = 0.f;
    const long long n = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int b = (ld && !prob) ? 0 : (int)((unsigned)i / (unsigned)HW), p = (int)i - b * HW;     // (B * HW < 2^31: checked by the entry points;
                                                                                                    //  token-major without a probability map needs neither)
        const T* lp = ld ? logits + i * ld : logits + (long long)b * ncls * HW + p;
        const long long ks = ld ? 1 : HW;
        float v[MAXCLS], m = -INFINITY;
        if (sizeof(T) == 2 && vec16) {                          // padded token rows (Graph.ln_cls(pad_rows)): whole 16-byte pieces instead of ncls 2-byte loads
            tok_row_load<T>(lp, ncls, v);
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) m = fmaxf(m, v[k]);
        } else {
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) { v[k] = ldf<T>(lp + k * ks); m = fmaxf(m, v[k]); }
        }
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MAXCLS; ++k) if (k < ncls) { v[k] = expf(v[k] - m); s += v[k]; }
        const float inv = 1.f / s;
        const int lab = (int)labels[i];
        float* pp = prob + (long long)b * ncls * HW + p;
        if constexpr (FT) {
            // q = 1 - p_t as the sum of the other classes' probabilities, in class order (the backward forms it the same way); the third
            // per-class sum is P_k = sum p under Tversky, Z_k = sum p^2 under Dice
            const bool counted = lab != ignore;
            float q = 0.f, pt = 1.f;
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) {
                const float pk = v[k] * inv;
                if (prob) pp[(long long)k * HW] = pk;
                if (counted) {
                    Z[k] += ft.tversky ? pk : pk * pk;
                    if (k == lab) { I[k] += pk; Y[k] += 1.f; pt = pk; } else q += pk;
                }
            }
            if constexpr (TOPK) {
                // the pixel's term goes to the value map, sign bit cleared (a NaN keeps a place above +inf in the select's bit order);
                // -1 marks an ignored pixel; a counted pixel whose label is no class has the term 0, as it adds nothing above
                float vi = -1.f;
                if (counted) vi = (unsigned)lab < (unsigned)ncls ? wce[lab] * focal_pow(q, ft.gamma) * focal_log_pt(pt, q) : 0.f;
                tk.values[i] = counted ? __uint_as_float(__float_as_uint(vi) & 0x7fffffffu) : vi;
                continue;
            }
            if (counted && (unsigned)lab < (unsigned)ncls) ce -= wce[lab] * focal_pow(q, ft.gamma) * focal_log_pt(pt, q);
            continue;
        }
        if constexpr (WEIGHTED) {
            const bool counted = lab != ignore;                    // one test per pixel; an ignored pixel still writes its probabilities
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) {
                const float pk = v[k] * inv;
                if (prob) pp[(long long)k * HW] = pk;
                if (counted) {
                    Z[k] += pk * pk;
                    if (k == lab) { I[k] += pk; Y[k] += 1.f; ce -= wce[k] * logf(fmaxf(pk, 1e-38f)); }
                }
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < MAXCLS; ++k) if (k < ncls) {
            const float pk = v[k] * inv;
            if (prob) pp[(long long)k * HW] = pk;                  // (null: the backward recomputes the softmax from the logits)
            Z[k] += pk * pk;
            if (k == lab) { I[k] += pk; Y[k] += 1.f; ce -= logf(fmaxf(pk, 1e-38f)); }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ce = wave_sum(ce);
    if (lane == 0) red[wave][0] = ce;
#pragma unroll
    for (int k = 0; k < MAXCLS; ++k) if (k < ncls) {
        const float a = wave_sum(I[k]), b = wave_sum(Y[k]), c = wave_sum(Z[k]);
        if (lane == 0) { red[wave][1 + 3 * k] = a; red[wave][2 + 3 * k] = b; red[wave][3 + 3 * k] = c; }
    }
    __syncthreads();
    if constexpr (TOPK) { if (threadIdx.x == 0) return; }          // sums[0] is tc_topk_select's
    if (threadIdx.x < 1 + 3 * ncls)
        atomicAdd(sums + threadIdx.x, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// WEIGHTED: n_pix is not used.  The prologue forms n_eff = sum_k w_ce[k] Y_k from the sums (Y_k is the number of counted pixels of class k:
// whole numbers, exact in fp32 below 2^24 counted pixels in all) and folds w_dice[k] into ca / cb; per pixel the CE factor is
// (w_ce / n_eff) * w_ce[lab] in that order, which with all-ones weights is w_ce / n_pix to the bit.  n_eff = 0 (every pixel ignored, or only
// zero-weight classes present): the CE term has no gradient.  An ignored pixel's gradient is WRITTEN as zeros (dlogits is uninitialised memory).
//
// FT: under Tversky ca / cb are the coefficients of g_k = ca_k [k = lab] + cb_k (cb is NOT multiplied by p_k) from I, Y and P = sums[3 + 3k];
// per pixel the CE factor is additionally multiplied by m = q^gamma (1 - gamma p_t log p_t / q), and p_t - 1 is taken as -q.
//
// TOPK: the CE factor is w_ce / (world k) with k = state[2] of this rank's select (0 when nothing is counted: no CE gradient), times the
// pixel's selection weight: 1 above the threshold, the tie share at it, 0 below, by the bit patterns the select ordered.
template <typename T, bool WEIGHTED, bool FT = false, bool TOPK = false>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ prob, const long long* __restrict__ labels,
                                                           const float* __restrict__ sums, T* __restrict__ dlogits, int B, int ncls,
                                                           int HW, float w_ce, float w_dice, float n_pix, float gscale, const float* __restrict__ gscale_dev, int ld,
                                                           const T* __restrict__ logits, int ldl, const float* __restrict__ weights, int ignore,
                                                           LossOpts<FT> ft, TopkBwd<TOPK> tk) {
    static_assert(WEIGHTED || !FT, "FT extends the WEIGHTED variant");
    static_assert(FT || !TOPK, "TOPK extends the FT variant");
    if (gscale_dev) gscale *= *gscale_dev;
    const bool vin = !prob && !(ldl & 7) && ldl >= ((ncls + 7) & ~7) && !((uintptr_t)logits & 15);
    const bool vout = ld > 0 && !(ld & 7) && ld >= ((ncls + 7) & ~7) && !((uintptr_t)dlogits & 15);
    __shared__ float ca[MAXCLS], cb[MAXCLS];          // dDice/dp_c = ca[c]*onehot_c + cb[c]*p_c
    __shared__ float wce[WEIGHTED ? MAXCLS : 1], wy[WEIGHTED ? MAXCLS : 1];
    if (threadIdx.x < ncls) {
        const float I = sums[1 + 3 * threadIdx.x], Y = sums[2 + 3 * threadIdx.x], Z = sums[3 + 3 * threadIdx.x];
        const float den = Z + Y + 1e-5f, num = 2.f * I + 1e-5f;
        ca[threadIdx.x] = -w_dice / (float)ncls * 2.f / den;
        cb[threadIdx.x] = w_dice / (float)ncls * 2.f * num / (den * den);
        if constexpr (WEIGHTED) {
            const float wc = weights ? weights[threadIdx.x] : 1.f, wd = weights ? weights[ncls + threadIdx.x] : 1.f;
            ca[threadIdx.x] *= wd;
            cb[threadIdx.x] *= wd;
            wce[threadIdx.x] = wc;
            wy[threadIdx.x] = wc * Y;
            if constexpr (FT) {
                if (ft.tversky) {                                   // Z is P = sum p here
                    const float r = 1.f - ft.alpha - ft.beta, tn = I + 1e-5f;
                    const float D = r * I + ft.alpha * Z + ft.beta * Y + 1e-5f;
                    ca[threadIdx.x] = -w_dice / (float)ncls * wd * (D - tn * r) / (D * D);
                    cb[threadIdx.x] = w_dice / (float)ncls * wd * tn * ft.alpha / (D * D);
                }
            }
        }
    }
    __syncthreads();
    const long long n = (long long)B * HW;
    float cew;
    if constexpr (WEIGHTED) {
        float n_eff = 0.f;
        for (int k = 0; k < ncls; ++k) n_eff += wy[k];              // class order, the same in every thread and every workgroup
        cew = n_eff > 0.f ? w_ce / n_eff : 0.f;
        if constexpr (TOPK) cew = tk.state[2] > 0.0 ? (float)((double)w_ce * (double)tk.inv_world / tk.state[2]) : 0.f;
    } else {
        cew = w_ce / n_pix;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int b = (ld && !prob) ? 0 : (int)((unsigned)i / (unsigned)HW), p = (int)i - b * HW;
        const float* pp = prob + (long long)b * ncls * HW + p;
        const int lab = (int)labels[i];
        float pk[MAXCLS], g[MAXCLS], dot = 0.f;
        if (prob) {
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) pk[k] = pp[(long long)k * HW];
        } else {                                                // the forward's arithmetic again (same operations, same order: same bits)
            const T* lp = logits + i * ldl;
            float m = -INFINITY, ssum = 0.f;
            if (sizeof(T) == 2 && vin) {
                tok_row_load<T>(lp, ncls, pk);
#pragma unroll
                for (int k = 0; k < MAXCLS; ++k) if (k < ncls) m = fmaxf(m, pk[k]);
            } else {
#pragma unroll
                for (int k = 0; k < MAXCLS; ++k) if (k < ncls) { pk[k] = ldf<T>(lp + k); m = fmaxf(m, pk[k]); }
            }
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) { pk[k] = expf(pk[k] - m); ssum += pk[k]; }
            const float inv = 1.f / ssum;
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) pk[k] *= inv;
        }
        if constexpr (FT) {
            float q = 0.f, pt = 1.f;                               // as the forward forms them
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) {
                g[k] = (k == lab ? ca[k] : 0.f) + (ft.tversky ? cb[k] : cb[k] * pk[k]);
                dot += g[k] * pk[k];
                if (k == lab) pt = pk[k]; else q += pk[k];
            }
            // m = q^(gamma - 1) (q - gamma p_t log p_t) as q^gamma (1 - gamma p_t log p_t / q): no power of q overflows, and p_t near 1
            // has -log p_t of the order of q.  gamma = 0: 1; q = 0 under gamma > 0: 0
            float mod = 1.f;
            if (ft.gamma != 0.f) mod = q > 0.f ? powf(q, ft.gamma) * (1.f - ft.gamma * pt * focal_log_pt(pt, q) / q) : 0.f;
            const bool counted = lab != ignore;
            float cw = cew * ((unsigned)lab < (unsigned)ncls ? wce[lab] : 1.f) * mod;
            if constexpr (TOPK) {
                const unsigned vb = __float_as_uint(tk.values[i]), tb = __float_as_uint((float)tk.state[5]);
                cw *= vb > tb ? 1.f : (vb == tb ? (float)tk.state[7] : 0.f);       // (an ignored pixel's -1 is above every t; it writes zeros below)
            }
            T* dp = ld ? dlogits + i * ld : dlogits + (long long)b * ncls * HW + p;
            const long long ks = ld ? 1 : HW;
            if (sizeof(T) == 2 && vout) {
                float o[MAXCLS];
#pragma unroll
                for (int k = 0; k < MAXCLS; ++k)
                    o[k] = (k < ncls && counted) ? gscale * (cw * (k == lab ? -q : pk[k]) + pk[k] * (g[k] - dot)) : 0.f;
                tok_row_store<T>(dp, ncls, o);
            } else {
#pragma unroll
                for (int k = 0; k < MAXCLS; ++k) if (k < ncls)
                    stf<T>(dp + k * ks, counted ? gscale * (cw * (k == lab ? -q : pk[k]) + pk[k] * (g[k] - dot)) : 0.f);
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < MAXCLS; ++k) if (k < ncls) {
            g[k] = (k == lab ? ca[k] : 0.f) + cb[k] * pk[k];
            dot += g[k] * pk[k];
        }
        T* dp = ld ? dlogits + i * ld : dlogits + (long long)b * ncls * HW + p;
        const long long ks = ld ? 1 : HW;
        if constexpr (WEIGHTED) {
            // (a label outside [0, ncls) that is not `ignore` matches no class, as in the plain kernel; it takes weight 1 rather than reading past wce)
            const bool counted = lab != ignore;
            const float cw = cew * ((unsigned)lab < (unsigned)ncls ? wce[lab] : 1.f);
            if (sizeof(T) == 2 && vout) {
                float o[MAXCLS];
#pragma unroll
                for (int k = 0; k < MAXCLS; ++k)
                    o[k] = (k < ncls && counted) ? gscale * (cw * (pk[k] - (k == lab ? 1.f : 0.f)) + pk[k] * (g[k] - dot)) : 0.f;
                tok_row_store<T>(dp, ncls, o);
            } else {
#pragma unroll
                for (int k = 0; k < MAXCLS; ++k) if (k < ncls)
                    stf<T>(dp + k * ks, counted ? gscale * (cw * (pk[k] - (k == lab ? 1.f : 0.f)) + pk[k] * (g[k] - dot)) : 0.f);
            }
            continue;
        }
        if (sizeof(T) == 2 && vout) {                           // padded rows: the pad elements are written as zeros
            float o[MAXCLS];
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) o[k] = k < ncls ? gscale * (cew * (pk[k] - (k == lab ? 1.f : 0.f)) + pk[k] * (g[k] - dot)) : 0.f;
            tok_row_store<T>(dp, ncls, o);
        } else {
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls)
                stf<T>(dp + k * ks, gscale * (cew * (pk[k] - (k == lab ? 1.f : 0.f)) + pk[k] * (g[k] - dot)));
        }
    }
}

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long n, float lr,
                           float mom, float wd, float gscale, int first, const float* __restrict__ lr_dev) {
    if (lr_dev) lr = *lr_dev;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float w = p[i];
        const float d = g[i] * gscale + wd * w;
        const float b = first ? d : mom * buf[i] + d;
        buf[i] = b;
        p[i] = w - lr * b;
    }
}

// all contiguous "used" parameter segments in one launch: blockIdx.y = segment, segs[2*i] = offset, segs[2*i+1] = length
// sum of squares of a flat fp32 buffer, accumulated into *out (the total gradient norm of nn.utils.clip_grad_norm_, trainer.py:147-148:
// parameters without a gradient hold zeros in the arena)
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long long n4, float* __restrict__ out) {
    __shared__ float red[4];
    float s = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(g)[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

__global__ void sgd_multi_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, const long long* __restrict__ segs,
                                 float lr, float mom, float wd, float gscale, int first, const float* __restrict__ lr_dev,
                                 const float* __restrict__ clip_sumsq, float clip_norm, void* __restrict__ lp, int lp_dtype,
                                 const float* __restrict__ scale_state) {
    if (lr_dev) lr = *lr_dev;
    if (clip_sumsq) {
        // a non-finite gradient (float16 overflow under a loss scale): skip the update -- weights, momentum and the 16-bit copy stay as
        // they were.  Otherwise clip_grad_norm_'s coefficient, clamped to 1 (clip_norm = inf: no clipping)
        const float ss = *clip_sumsq;
        if (!(ss < __builtin_inff())) return;
        if (scale_state) {                    // dynamic loss scale (tc_sgd_step_multi_scaled): the arena holds gradients `scale` times too
            gscale *= scale_state[1];         // large, so 1 / scale takes it out again and the threshold is raised by `scale`: what is clipped
            clip_norm *= scale_state[0];      // is the norm of the TRUE gradient
        }
        gscale *= fminf(clip_norm / (sqrtf(ss) + 1e-6f), 1.0f);
    }
    const long long off = segs[2 * blockIdx.y], n = segs[2 * blockIdx.y + 1];
    if (!((off | n) & 3) && !(((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) && !((uintptr_t)lp & 7)) {
        // four elements per thread in 16-byte pieces (the arena's segments start and end on multiples of 8 elements): the scalar form
        // ran at 4.1 TB/s for the 22 bytes per weight it moves
        const long long n4 = n >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const long long j = off + 4 * i;
            const float4 w = *reinterpret_cast<const float4*>(p + j), gv = *reinterpret_cast<const float4*>(g + j);
            float4 b;
            if (first) b = make_float4(gv.x * gscale + wd * w.x, gv.y * gscale + wd * w.y, gv.z * gscale + wd * w.z, gv.w * gscale + wd * w.w);
            else {
                const float4 m = *reinterpret_cast<const float4*>(buf + j);
                b = make_float4(mom * m.x + (gv.x * gscale + wd * w.x), mom * m.y + (gv.y * gscale + wd * w.y), mom * m.z + (gv.z * gscale + wd * w.z),
                                mom * m.w + (gv.w * gscale + wd * w.w));
            }
            *reinterpret_cast<float4*>(buf + j) = b;
            const float4 wn = make_float4(w.x - lr * b.x, w.y - lr * b.y, w.z - lr * b.z, w.w - lr * b.w);
            *reinterpret_cast<float4*>(p + j) = wn;
            if (lp_dtype == TC_BF16) *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(lp) + j) = make_uint2(pack2<bf16_t>(wn.x, wn.y), pack2<bf16_t>(wn.z, wn.w));
            else if (lp_dtype == TC_F16) *reinterpret_cast<uint2*>(reinterpret_cast<f16_t*>(lp) + j) = make_uint2(pack2<f16_t>(wn.x, wn.y), pack2<f16_t>(wn.z, wn.w));
        }
        return;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long j = off + i;
        const float w = p[j];
        const float d = g[j] * gscale + wd * w;
        const float b = first ? d : mom * buf[j] + d;
        buf[j] = b;
        const float wn = w - lr * b;
        p[j] = wn;
        // the 16-bit working copy of the weights that the next forward reads (otherwise a separate cast pass over the whole arena)
        if (lp_dtype == TC_BF16) reinterpret_cast<bf16_t*>(lp)[j] = f2bf(wn);
        else if (lp_dtype == TC_F16) reinterpret_cast<f16_t*>(lp)[j] = f2h(wn);
    }
}

// The step count of an Adam state (include/transception_hip.h) and the two bias terms derived from it.  One thread: ordinary loads and
// stores.  beta^t by repeated squaring in double (at most 62 multiplications, each within 2^-53: far inside one float32 rounding of
// 1 - beta^t even at t = 1, where 1 - 0.999 cancels three digits), every word rounded once.  A non-finite *sumsq leaves all four words
// alone: adam_multi_kernel skips the same step.
__global__ void adam_advance_kernel(float* __restrict__ state, const float* __restrict__ sumsq, double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (sumsq && !(*sumsq < __builtin_inff())) return;
    int* istate = reinterpret_cast<int*>(state);
    const int t = istate[0] + 1;
    double p1 = 1.0, p2 = 1.0, s1 = beta1, s2 = beta2;
    for (unsigned k = (unsigned)t; k; k >>= 1) {
        if (k & 1) { p1 *= s1; p2 *= s2; }
        s1 *= s1;
        s2 *= s2;
    }
    istate[0] = t;
    state[1] = (float)(1.0 - p1);
    state[2] = (float)sqrt(1.0 - p2);
    istate[3] = 0;
}

// torch.optim.AdamW (decoupled) / torch.optim.Adam (coupled decay) on one element.  dk = 1 - lr wd (decoupled) or 1; wc = wd (coupled) or 0;
// step = lr / state[1]; rbc2 is state[2] itself: sqrt(v') is DIVIDED by it, as torch does.  Division and sqrtf are the correctly rounded ones.
__device__ __forceinline__ float adam_elem(float w, float g, float& m, float& v, float c, float dk, float wc, float b1, float omb1, float b2,
                                           float omb2, float step, float bc2, float eps) {
    const float gh = g * c + wc * w;
    m = b1 * m + omb1 * gh;
    v = b2 * v + (omb2 * gh) * gh;
    return w * dk - step * (m / (sqrtf(v) / bc2 + eps));
}

// The segment table, the clip / skip / loss-scale prologue, the alignment test and the two element paths are sgd_multi_kernel's.
// 30 bytes per weight with a 16-bit copy: p, g, m, v read, p, m, v and lp written.
__global__ __launch_bounds__(256) void adam_multi_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, const long long* __restrict__ segs,
                                                         const float* __restrict__ wd_dev, float lr, const float* __restrict__ lr_dev, float b1,
                                                         float omb1, float b2, float omb2, float eps, float wd, int decoupled, float gscale,
                                                         const float* __restrict__ clip_sumsq, float clip_norm, void* __restrict__ lp,
                                                         int lp_dtype, const float* __restrict__ scale_state,
                                                         const float* __restrict__ adam_state) {
    if (lr_dev) lr = *lr_dev;
    if (clip_sumsq) {
        const float ss = *clip_sumsq;
        if (!(ss < __builtin_inff())) return;     // skipped: weights, both moments and the 16-bit copy stay; adam_advance_kernel did not count it
        if (scale_state) {
            gscale *= scale_state[1];
            clip_norm *= scale_state[0];
        }
        gscale *= fminf(clip_norm / (sqrtf(ss) + 1e-6f), 1.0f);
    }
    if (wd_dev) wd = wd_dev[blockIdx.y];
    const float dk = decoupled ? 1.f - lr * wd : 1.f, wc = decoupled ? 0.f : wd;
    const float step = lr / adam_state[1], bc2 = adam_state[2];
    const long long off = segs[2 * blockIdx.y], n = segs[2 * blockIdx.y + 1];
    if (!((off | n) & 3) && !(((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) && !((uintptr_t)lp & 7)) {
        const long long n4 = n >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const long long j = off + 4 * i;
            const float4 w = *reinterpret_cast<const float4*>(p + j), gv = *reinterpret_cast<const float4*>(g + j);
            float4 mv = *reinterpret_cast<const float4*>(m + j), vv = *reinterpret_cast<const float4*>(v + j);
            float4 wn;
            wn.x = adam_elem(w.x, gv.x, mv.x, vv.x, gscale, dk, wc, b1, omb1, b2, omb2, step, bc2, eps);
            wn.y = adam_elem(w.y, gv.y, mv.y, vv.y, gscale, dk, wc, b1, omb1, b2, omb2, step, bc2, eps);
            wn.z = adam_elem(w.z, gv.z, mv.z, vv.z, gscale, dk, wc, b1, omb1, b2, omb2, step, bc2, eps);
            wn.w = adam_elem(w.w, gv.w, mv.w, vv.w, gscale, dk, wc, b1, omb1, b2, omb2, step, bc2, eps);
            *reinterpret_cast<float4*>(m + j) = mv;
            *reinterpret_cast<float4*>(v + j) = vv;
            *reinterpret_cast<float4*>(p + j) = wn;
            if (lp_dtype == TC_BF16) *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(lp) + j) = make_uint2(pack2<bf16_t>(wn.x, wn.y), pack2<bf16_t>(wn.z, wn.w));
            else if (lp_dtype == TC_F16) *reinterpret_cast<uint2*>(reinterpret_cast<f16_t*>(lp) + j) = make_uint2(pack2<f16_t>(wn.x, wn.y), pack2<f16_t>(wn.z, wn.w));
        }
        return;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long j = off + i;
        float mj = m[j], vj = v[j];
        const float wn = adam_elem(p[j], g[j], mj, vj, gscale, dk, wc, b1, omb1, b2, omb2, step, bc2, eps);
        m[j] = mj;
        v[j] = vj;
        p[j] = wn;
        if (lp_dtype == TC_BF16) reinterpret_cast<bf16_t*>(lp)[j] = f2bf(wn);
        else if (lp_dtype == TC_F16) reinterpret_cast<f16_t*>(lp)[j] = f2h(wn);
    }
}

// Evaluation (utils.py:72-76,96-97): pred = argmax_k logits[b,k,p] (softmax is monotone; first maximum wins like torch.argmax) and,
// when labels are given, per-class voxel counts  counts[3k..3k+2] += (|pred==k & gt==k|, |pred==k|, |gt==k|)  for the Dice of
// calculate_metric_percase (utils.py:50-60).  Counts are exact in fp32 up to 2^24 per launch; the host accumulates in float64.
template <typename T>
__global__ __launch_bounds__(256) void argmax_counts_kernel(const T* __restrict__ logits, const long long* __restrict__ labels,
                                                            unsigned char* __restrict__ pred, float* __restrict__ counts, int B, int ncls,
                                                            int HW) {
    __shared__ float red[4][3 * MAXCLS];
    float cnt[3 * MAXCLS];
#pragma unroll
    for (int k = 0; k < 3 * MAXCLS; ++k) cnt[k] = 0.f;
    const long long n = (long long)B * HW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / HW), p = (int)(i % HW);
        const T* lp = logits + (long long)b * ncls * HW + p;
        float m = ldf<T>(lp);
        int arg = 0;
#pragma unroll
        for (int k = 1; k < MAXCLS; ++k) if (k < ncls) { const float v = ldf<T>(lp + (long long)k * HW); if (v > m) { m = v; arg = k; } }
        pred[i] = (unsigned char)arg;
        if (labels) {
            const int lab = (int)labels[i];
#pragma unroll
            for (int k = 0; k < MAXCLS; ++k) if (k < ncls) {
                cnt[3 * k] += (arg == k && lab == k) ? 1.f : 0.f;
                cnt[3 * k + 1] += (arg == k) ? 1.f : 0.f;
                cnt[3 * k + 2] += (lab == k) ? 1.f : 0.f;
            }
        }
    }
    if (!labels) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 3 * MAXCLS; ++k) if (k < 3 * ncls) { const float a = wave_sum(cnt[k]); if (lane == 0) red[wave][k] = a; }
    __syncthreads();
    if (threadIdx.x < 3 * ncls) atomicAdd(counts + threadIdx.x, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// torch.amp.GradScaler.update's rule on the four words of a loss-scale state (include/transception_hip.h), with two clamps added.
// One thread: four loads, a handful of flops, four ordinary stores.
__global__ void loss_scale_update_kernel(float* __restrict__ state, const float* __restrict__ sumsq, float growth, float backoff, int interval,
                                         float min_scale, float max_scale) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int* istate = reinterpret_cast<int*>(state);
    float scale = state[0];
    int tracker = istate[2], skipped = istate[3];
    if (!(*sumsq < __builtin_inff())) {                           // inf or NaN: the update kernel skipped this step
        scale = fmaxf(scale * backoff, min_scale);
        tracker = 0;
        ++skipped;
    } else if (++tracker >= interval) {                           // (== for a tracker that counts up from 0; >= so that a loaded tracker beyond
        scale = fminf(scale * growth, max_scale);                 //  the interval grows at once instead of counting round the integers)
        tracker = 0;
    }
    state[0] = scale;
    state[1] = 1.f / scale;
    istate[2] = tracker;
    istate[3] = skipped;
}

__global__ void zero_floats_kernel(float* __restrict__ p, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

}  // namespace

extern "C" int tc_colsum(const void* x, int rows, int cols, int ldx, int nb, long long sb, float* out, int accumulate, int dtype,
                         void* stream) {
    if (!x || !out || rows <= 0 || cols <= 0 || nb <= 0) return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    // (a kernel, not hipMemsetAsync: memset NODES of a captured single-stream graph were observed to run out of order on ROCm 7.2)
    if (!accumulate) hipLaunchKernelGGL(zero_floats_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, out, cols);
    dim3 grid(tc_blocks((long long)rows * nb, 4 * 32, 256), (cols + 63) / 64);
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((colsum_kernel<T>), grid, dim3(256), 0, s, (const T*)x, rows, cols, ldx, out, nb, sb));
    return tc_launch_status();
}

extern "C" int tc_seg_loss_fwd(const void* logits, const long long* labels, float* prob, float* sums, int B, int ncls, int HW,
                               int dtype, void* stream) {
    if (!logits || !labels || !prob || !sums || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 || (long long)B * HW >= 0x7fffffffLL) return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_fwd_kernel<T, false>), dim3(tc_blocks((long long)B * HW, 256, 1024)), dim3(256), 0, s,
                                                (const T*)logits, labels, prob, sums, B, ncls, HW, 0, (const float*)nullptr, 0, LossOpts<false>{}, TopkFwd<false>{}));
    return tc_launch_status();
}

extern "C" int tc_seg_loss_fwd_tok(const void* logits, int ld, const long long* labels, float* prob, float* sums, int B, int ncls, int HW,
                                   int dtype, void* stream) {
    if (!logits || !labels || !sums || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 || ld < ncls || (long long)B * HW >= 0x7fffffffLL) return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_fwd_kernel<T, false>), dim3(tc_blocks((long long)B * HW, 256, 1024)), dim3(256), 0, s,
                                                (const T*)logits, labels, prob, sums, B, ncls, HW, ld, (const float*)nullptr, 0, LossOpts<false>{}, TopkFwd<false>{}));
    return tc_launch_status();
}

// loss, CE and Dice from the (all-reduced) sums, in double like the host expression it replaces (sixteen scalar launches between the
// forward and the backward of every step).  trainer.py:141-143, utils.py:34-47.
__global__ void seg_loss_value_kernel(const float* __restrict__ sums, int ncls, double n_pix, double w_ce, double w_dice,
                                      float* __restrict__ out3) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double ce = (double)sums[0] / n_pix;
    double acc = 0.0;
    for (int c = 0; c < ncls; ++c) {
        const double inter = sums[1 + 3 * c], ysum = sums[2 + 3 * c], zsum = sums[3 + 3 * c];
        acc += 1.0 - (2.0 * inter + 1e-5) / (zsum + ysum + 1e-5);
    }
    const double dice = acc / (double)ncls;
    out3[0] = (float)(w_ce * ce + w_dice * dice);
    out3[1] = (float)ce;
    out3[2] = (float)dice;
}

extern "C" int tc_seg_loss_value(const float* sums, int ncls, double n_pix, double w_ce, double w_dice, float* out3, void* stream) {
    if (!sums || !out3 || ncls <= 0 || ncls > MAXCLS || !(n_pix > 0.0)) return TC_ERR_ARG;
    hipLaunchKernelGGL(seg_loss_value_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, ncls, n_pix, w_ce, w_dice, out3);
    return tc_launch_status();
}

// The same from the sums of the class-weighted / ignoring forward: sums[0] = sum_i w_ce[y_i] nll_i over the counted pixels, so
// CE = sums[0] / sum_k w_ce[k] Y_k (nn.CrossEntropyLoss(weight, ignore_index), mean reduction) -- 0, not NaN, when that denominator is 0 --
// and Dice = sum_k w_dice[k] (1 - (2 I_k + eps) / (Z_k + Y_k + eps)) / ncls (DiceLoss.forward(weight=...), utils.py:42-46).
__global__ void seg_loss_value_w_kernel(const float* __restrict__ sums, const float* __restrict__ weights, int ncls, double w_ce, double w_dice,
                                        float* __restrict__ out3) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double acc = 0.0, n_eff = 0.0;
    for (int c = 0; c < ncls; ++c) {
        const double inter = sums[1 + 3 * c], ysum = sums[2 + 3 * c], zsum = sums[3 + 3 * c];
        const double wc = weights ? (double)weights[c] : 1.0, wd = weights ? (double)weights[ncls + c] : 1.0;
        n_eff += wc * ysum;
        acc += wd * (1.0 - (2.0 * inter + 1e-5) / (zsum + ysum + 1e-5));
    }
    const double ce = n_eff > 0.0 ? (double)sums[0] / n_eff : 0.0;
    const double dice = acc / (double)ncls;
    out3[0] = (float)(w_ce * ce + w_dice * dice);
    out3[1] = (float)ce;
    out3[2] = (float)dice;
}

extern "C" int tc_seg_loss_value_w(const float* sums, const float* weights, int ncls, double w_ce, double w_dice, float* out3, void* stream) {
    if (!sums || !out3 || ncls <= 0 || ncls > MAXCLS) return TC_ERR_ARG;
    hipLaunchKernelGGL(seg_loss_value_w_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, weights, ncls, w_ce, w_dice, out3);
    return tc_launch_status();
}

// ld = 0: NCHW logits (prob is then required, as in tc_seg_loss_fwd); ld >= ncls: token-major rows (tc_seg_loss_fwd_tok)
extern "C" int tc_seg_loss_fwd_w(const void* logits, int ld, const long long* labels, const float* weights, int ignore_index, float* prob,
                                 float* sums, int B, int ncls, int HW, int dtype, void* stream) {
    if (!logits || !labels || !sums || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 || (ld != 0 && ld < ncls) || (ld == 0 && !prob) ||
        (ignore_index >= 0 && ignore_index < ncls) || (long long)B * HW >= 0x7fffffffLL)
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_fwd_kernel<T, true>), dim3(tc_blocks((long long)B * HW, 256, 1024)), dim3(256), 0, s,
                                                (const T*)logits, labels, prob, sums, B, ncls, HW, ld, weights, ignore_index, LossOpts<false>{}, TopkFwd<false>{}));
    return tc_launch_status();
}

// ld = 0: NCHW dlogits from the probability map (tc_seg_loss_bwd); ld >= ncls: token-major rows, prob or -- prob == NULL -- the softmax
// recomputed from the token-major logits of row pitch ldl (tc_seg_loss_bwd_tok)
extern "C" int tc_seg_loss_bwd_w(const float* prob, const void* logits, int ldl, const long long* labels, const float* weights, int ignore_index,
                                 const float* sums, void* dlogits, int ld, int B, int ncls, int HW, float w_ce, float w_dice, float gscale,
                                 const float* gscale_dev, int dtype, void* stream) {
    if ((!prob && (!logits || ldl < ncls || ld == 0)) || !labels || !sums || !dlogits || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 ||
        (ld != 0 && ld < ncls) || (ignore_index >= 0 && ignore_index < ncls) || (long long)B * HW >= 0x7fffffffLL)
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_bwd_kernel<T, true>), dim3(tc_blocks((long long)B * HW, 256, 2048)), dim3(256), 0, s,
                                                prob, labels, sums, (T*)dlogits, B, ncls, HW, w_ce, w_dice, 0.f, gscale, gscale_dev, ld,
                                                (const T*)logits, ldl, weights, ignore_index, LossOpts<false>{}, TopkBwd<false>{}));
    return tc_launch_status();
}

// ---- focal CE and Tversky overlap (include/transception_loss.h): the FT variant of the two kernels above and a value kernel of its own
extern "C" int tc_loss_abi_version(void) { return TC_LOSS_ABI_VERSION; }

// gamma >= 0 and finite; an overlap constant; under Tversky alpha, beta >= 0, finite and not both 0 (the comparisons are false for a NaN)
static bool loss_opts_ok(double gamma, int overlap, double alpha, double beta) {
    if (!(gamma >= 0.0 && gamma < (double)INFINITY)) return false;
    if (overlap == TC_OVERLAP_DICE) return true;
    return overlap == TC_OVERLAP_TVERSKY && alpha >= 0.0 && alpha < (double)INFINITY && beta >= 0.0 && beta < (double)INFINITY && alpha + beta > 0.0;
}

extern "C" int tc_seg_loss_fwd_ft(const void* logits, int ld, const long long* labels, const float* weights, int ignore_index, float gamma,
                                  int overlap, float* prob, float* sums, int B, int ncls, int HW, int dtype, void* stream) {
    if (!logits || !labels || !sums || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 || (ld != 0 && ld < ncls) || (ld == 0 && !prob) ||
        (ignore_index >= 0 && ignore_index < ncls) || (long long)B * HW >= 0x7fffffffLL || !loss_opts_ok(gamma, overlap, 0.5, 0.5))
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const LossOpts<true> ft{gamma, overlap == TC_OVERLAP_TVERSKY, 0.f, 0.f};
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_fwd_kernel<T, true, true>), dim3(tc_blocks((long long)B * HW, 256, 1024)), dim3(256), 0, s,
                                                (const T*)logits, labels, prob, sums, B, ncls, HW, ld, weights, ignore_index, ft, TopkFwd<false>{}));
    return tc_launch_status();
}

// tc_seg_loss_value_w's expression with the overlap term chosen by `overlap`; sums[0] already carries the focal factor
// TOPK (tc_seg_loss_value_topk): sums[0] IS the cross-entropy, the mean over ranks of each rank's top-k mean
template <bool TOPK = false>
__global__ void seg_loss_value_ft_kernel(const float* __restrict__ sums, const float* __restrict__ weights, int ncls, double w_ce, double w_dice,
                                         int tversky, double alpha, double beta, float* __restrict__ out3) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double acc = 0.0, n_eff = 0.0;
    for (int c = 0; c < ncls; ++c) {
        const double inter = sums[1 + 3 * c], ysum = sums[2 + 3 * c], zsum = sums[3 + 3 * c];      // zsum: P = sum p under Tversky
        const double wc = weights ? (double)weights[c] : 1.0, wd = weights ? (double)weights[ncls + c] : 1.0;
        n_eff += wc * ysum;
        if (tversky) acc += wd * (1.0 - (inter + 1e-5) / ((1.0 - alpha - beta) * inter + alpha * zsum + beta * ysum + 1e-5));
        else acc += wd * (1.0 - (2.0 * inter + 1e-5) / (zsum + ysum + 1e-5));
    }
    const double ce = TOPK ? (double)sums[0] : n_eff > 0.0 ? (double)sums[0] / n_eff : 0.0;
    const double ov = acc / (double)ncls;
    out3[0] = (float)(w_ce * ce + w_dice * ov);
    out3[1] = (float)ce;
    out3[2] = (float)ov;
}

extern "C" int tc_seg_loss_value_ft(const float* sums, const float* weights, int ncls, double w_ce, double w_dice, int overlap, double alpha,
                                    double beta, float* out3, void* stream) {
    if (!sums || !out3 || ncls <= 0 || ncls > MAXCLS || !loss_opts_ok(0.0, overlap, alpha, beta)) return TC_ERR_ARG;
    hipLaunchKernelGGL(seg_loss_value_ft_kernel<false>, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, weights, ncls, w_ce, w_dice,
                       (int)(overlap == TC_OVERLAP_TVERSKY), alpha, beta, out3);
    return tc_launch_status();
}

extern "C" int tc_seg_loss_bwd_ft(const float* prob, const void* logits, int ldl, const long long* labels, const float* weights, int ignore_index,
                                  const float* sums, void* dlogits, int ld, int B, int ncls, int HW, float w_ce, float w_dice, float gamma,
                                  int overlap, float alpha, float beta, float gscale, const float* gscale_dev, int dtype, void* stream) {
    if ((!prob && (!logits || ldl < ncls || ld == 0)) || !labels || !sums || !dlogits || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 ||
        (ld != 0 && ld < ncls) || (ignore_index >= 0 && ignore_index < ncls) || (long long)B * HW >= 0x7fffffffLL ||
        !loss_opts_ok(gamma, overlap, alpha, beta))
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const bool tv = overlap == TC_OVERLAP_TVERSKY;
    const LossOpts<true> ft{gamma, tv, tv ? alpha : 0.f, tv ? beta : 0.f};
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_bwd_kernel<T, true, true>), dim3(tc_blocks((long long)B * HW, 256, 2048)), dim3(256), 0, s,
                                                prob, labels, sums, (T*)dlogits, B, ncls, HW, w_ce, w_dice, 0.f, gscale, gscale_dev, ld,
                                                (const T*)logits, ldl, weights, ignore_index, ft, TopkBwd<false>{}));
    return tc_launch_status();
}

// ---- top-k cross-entropy (include/transception_topk.h): the TOPK variant of the FT kernels; the select between them is csrc/topk.hip
extern "C" int tc_seg_loss_fwd_topk(const void* logits, int ld, const long long* labels, const float* weights, int ignore_index, float gamma,
                                    int overlap, float* prob, float* sums, float* values, int B, int ncls, int HW, int dtype, void* stream) {
    if (!logits || !labels || !sums || !values || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 || (ld != 0 && ld < ncls) || (ld == 0 && !prob) ||
        (ignore_index >= 0 && ignore_index < ncls) || (long long)B * HW >= 0x7fffffffLL || !loss_opts_ok(gamma, overlap, 0.5, 0.5))
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const LossOpts<true> ft{gamma, overlap == TC_OVERLAP_TVERSKY, 0.f, 0.f};
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_fwd_kernel<T, true, true, true>), dim3(tc_blocks((long long)B * HW, 256, 1024)), dim3(256), 0, s,
                                                (const T*)logits, labels, prob, sums, B, ncls, HW, ld, weights, ignore_index, ft, TopkFwd<true>{values}));
    return tc_launch_status();
}

extern "C" int tc_seg_loss_value_topk(const float* sums, const float* weights, int ncls, double w_ce, double w_dice, int overlap, double alpha,
                                      double beta, float* out3, void* stream) {
    if (!sums || !out3 || ncls <= 0 || ncls > MAXCLS || !loss_opts_ok(0.0, overlap, alpha, beta)) return TC_ERR_ARG;
    hipLaunchKernelGGL(seg_loss_value_ft_kernel<true>, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, weights, ncls, w_ce, w_dice,
                       (int)(overlap == TC_OVERLAP_TVERSKY), alpha, beta, out3);
    return tc_launch_status();
}

extern "C" int tc_seg_loss_bwd_topk(const float* prob, const void* logits, int ldl, const long long* labels, const float* weights, int ignore_index,
                                    const float* sums, void* dlogits, int ld, int B, int ncls, int HW, float w_ce, float w_dice, float gamma,
                                    int overlap, float alpha, float beta, float gscale, const float* gscale_dev, const float* values,
                                    const double* state, float inv_world, int dtype, void* stream) {
    if ((!prob && (!logits || ldl < ncls || ld == 0)) || !labels || !sums || !dlogits || !values || !state || ((uintptr_t)state & 7) || B <= 0 ||
        ncls <= 0 || ncls > MAXCLS || HW <= 0 || (ld != 0 && ld < ncls) || (ignore_index >= 0 && ignore_index < ncls) ||
        (long long)B * HW >= 0x7fffffffLL || !loss_opts_ok(gamma, overlap, alpha, beta) || !(inv_world > 0.f && inv_world <= 1.f))
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const bool tv = overlap == TC_OVERLAP_TVERSKY;
    const LossOpts<true> ft{gamma, tv, tv ? alpha : 0.f, tv ? beta : 0.f};
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_bwd_kernel<T, true, true, true>), dim3(tc_blocks((long long)B * HW, 256, 2048)), dim3(256), 0, s,
                                                prob, labels, sums, (T*)dlogits, B, ncls, HW, w_ce, w_dice, 0.f, gscale, gscale_dev, ld,
                                                (const T*)logits, ldl, weights, ignore_index, ft, TopkBwd<true>{values, state, inv_world}));
    return tc_launch_status();
}

extern "C" int tc_argmax_counts(const void* logits, const long long* labels, unsigned char* pred, float* counts, int B, int ncls, int HW,
                                int dtype, void* stream) {
    if (!logits || !pred || (labels && !counts) || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0) return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((argmax_counts_kernel<T>), dim3(tc_blocks((long long)B * HW, 256, 512)), dim3(256), 0, s,
                                                (const T*)logits, labels, pred, counts, B, ncls, HW));
    return tc_launch_status();
}

extern "C" int tc_seg_loss_bwd(const float* prob, const long long* labels, const float* sums, void* dlogits, int B, int ncls, int HW,
                               float w_ce, float w_dice, float n_pix_global, float gscale, const float* gscale_dev, int dtype, void* stream) {
    if (!prob || !labels || !sums || !dlogits || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 || (long long)B * HW >= 0x7fffffffLL) return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_bwd_kernel<T, false>), dim3(tc_blocks((long long)B * HW, 256, 2048)), dim3(256), 0, s,
                                                prob, labels, sums, (T*)dlogits, B, ncls, HW, w_ce, w_dice, n_pix_global, gscale, gscale_dev, 0, (const T*)nullptr, 0,
                                                (const float*)nullptr, 0, LossOpts<false>{}, TopkBwd<false>{}));
    return tc_launch_status();
}

extern "C" int tc_seg_loss_bwd_tok(const float* prob, const void* logits, int ldl, const long long* labels, const float* sums, void* dlogits, int ld,
                                   int B, int ncls, int HW, float w_ce, float w_dice, float n_pix_global, float gscale, const float* gscale_dev,
                                   int dtype, void* stream) {
    if ((!prob && (!logits || ldl < ncls)) || !labels || !sums || !dlogits || B <= 0 || ncls <= 0 || ncls > MAXCLS || HW <= 0 || ld < ncls ||
        (long long)B * HW >= 0x7fffffffLL)
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((seg_loss_bwd_kernel<T, false>), dim3(tc_blocks((long long)B * HW, 256, 2048)), dim3(256), 0, s,
                                                prob, labels, sums, (T*)dlogits, B, ncls, HW, w_ce, w_dice, n_pix_global, gscale, gscale_dev, ld, (const T*)logits, ldl,
                                                (const float*)nullptr, 0, LossOpts<false>{}, TopkBwd<false>{}));
    return tc_launch_status();
}

extern "C" int tc_sgd_step(float* p, const float* grad, float* buf, long long n, float lr, const float* lr_dev, float momentum, float wd,
                           float gscale, int first, void* stream) {
    if (!p || !grad || !buf || n <= 0) return TC_ERR_ARG;
    hipLaunchKernelGGL(sgd_kernel, dim3(tc_blocks(n, 256 * 4, 4096)), dim3(256), 0, (hipStream_t)stream, p, grad, buf, n, lr, momentum, wd,
                       gscale, first, lr_dev);
    return tc_launch_status();
}

extern "C" int tc_sgd_step_multi(float* p, const float* grad, float* buf, const long long* segs_dev, int nseg, long long max_len, float lr,
                                 const float* lr_dev, float momentum, float wd, float gscale, int first, const float* clip_sumsq,
                                 float clip_norm, void* lp, int lp_dtype, void* stream) {
    if (!p || !grad || !buf || !segs_dev || nseg <= 0 || nseg > 65535 || max_len <= 0 || (clip_sumsq && !(clip_norm > 0.f)) ||
        (lp && lp_dtype != TC_BF16 && lp_dtype != TC_F16))
        return TC_ERR_ARG;
    hipLaunchKernelGGL(sgd_multi_kernel, dim3(tc_blocks(max_len, 256 * 8, 256), nseg), dim3(256), 0, (hipStream_t)stream, p, grad, buf, segs_dev,
                       lr, momentum, wd, gscale, first, lr_dev, clip_sumsq, clip_norm, lp, lp ? lp_dtype : -1, (const float*)nullptr);
    return tc_launch_status();
}

extern "C" int tc_sgd_step_multi_scaled(float* p, const float* grad, float* buf, const long long* segs_dev, int nseg, long long max_len, float lr,
                                        const float* lr_dev, float momentum, float wd, float gscale, int first, const float* clip_sumsq,
                                        float clip_norm, void* lp, int lp_dtype, const float* scale_state, void* stream) {
    if (!p || !grad || !buf || !segs_dev || nseg <= 0 || nseg > 65535 || max_len <= 0 || !clip_sumsq || !scale_state || !(clip_norm > 0.f) ||
        (lp && lp_dtype != TC_BF16 && lp_dtype != TC_F16))
        return TC_ERR_ARG;
    hipLaunchKernelGGL(sgd_multi_kernel, dim3(tc_blocks(max_len, 256 * 8, 256), nseg), dim3(256), 0, (hipStream_t)stream, p, grad, buf, segs_dev,
                       lr, momentum, wd, gscale, first, lr_dev, clip_sumsq, clip_norm, lp, lp ? lp_dtype : -1, scale_state);
    return tc_launch_status();
}

extern "C" int tc_adam_advance(float* state, const float* sumsq, double beta1, double beta2, void* stream) {
    if (!state || !(beta1 >= 0.0) || !(beta1 < 1.0) || !(beta2 >= 0.0) || !(beta2 < 1.0)) return TC_ERR_ARG;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, sumsq, beta1, beta2);
    return tc_launch_status();
}

extern "C" int tc_adam_step_multi(float* p, const float* grad, float* m, float* v, const long long* segs_dev, const float* wd_dev, int nseg,
                                  long long max_len, float lr, const float* lr_dev, double beta1, double beta2, float eps, float wd,
                                  int decoupled, float gscale, const float* clip_sumsq, float clip_norm, void* lp, int lp_dtype,
                                  const float* scale_state, const float* adam_state, void* stream) {
    if (!p || !grad || !m || !v || !segs_dev || !adam_state || nseg <= 0 || nseg > 65535 || max_len <= 0 || !(beta1 >= 0.0) || !(beta1 < 1.0) ||
        !(beta2 >= 0.0) || !(beta2 < 1.0) || !(eps > 0.f) || (clip_sumsq && !(clip_norm > 0.f)) || (scale_state && !clip_sumsq) ||
        (lp && lp_dtype != TC_BF16 && lp_dtype != TC_F16))
        return TC_ERR_ARG;
    // float(beta) and float(1 - beta): each rounded once from double, here on the host side of the launch
    hipLaunchKernelGGL(adam_multi_kernel, dim3(tc_blocks(max_len, 256 * 8, 256), nseg), dim3(256), 0, (hipStream_t)stream, p, grad, m, v, segs_dev,
                       wd_dev, lr, lr_dev, (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), eps, wd, decoupled ? 1 : 0,
                       gscale, clip_sumsq, clip_norm, lp, lp ? lp_dtype : -1, scale_state, adam_state);
    return tc_launch_status();
}

extern "C" int tc_loss_scale_update(float* state, const float* sumsq, float growth, float backoff, int interval, float min_scale,
                                    float max_scale, void* stream) {
    if (!state || !sumsq || !(growth >= 1.f) || !(growth < __builtin_inff()) || !(backoff > 0.f) || !(backoff < 1.f) || interval < 1 ||
        !(min_scale > 0.f) || !(max_scale >= min_scale) || !(max_scale < __builtin_inff()))
        return TC_ERR_ARG;
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, sumsq, growth, backoff, interval, min_scale,
                       max_scale);
    return tc_launch_status();
}

__global__ void fill_f32_kernel(float* __restrict__ p, long long n, float v) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) p[i] = v;
}
extern "C" int tc_fill_f32(float* p, long long n, float v, void* stream) {
    if (!p || n <= 0) return TC_ERR_ARG;
    hipLaunchKernelGGL(fill_f32_kernel, dim3(tc_blocks(n, 256 * 4, 2048)), dim3(256), 0, (hipStream_t)stream, p, n, v);
    return tc_launch_status();
}

extern "C" int tc_grad_sumsq(const float* g, long long n, float* out, void* stream) {
    if (!g || !out || n <= 0 || (n & 3) || (uintptr_t)g % 16) return TC_ERR_ARG;
    hipLaunchKernelGGL(sumsq_kernel, dim3(tc_blocks(n / 4, 256 * 8, 1024)), dim3(256), 0, (hipStream_t)stream, g, n / 4, out);
    return tc_launch_status();
}

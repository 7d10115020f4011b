// Uncertainty maps and calibration statistics of class scores (include/transception_uncertainty.h has the definitions): per pixel the
// normalised predictive entropy, the maximum-probability confidence, the mutual information between views and the label; over a batch the
// reliability table, the NLL and Brier sums and the per-predicted-class entropy sums.  The scores are the network's logits (softmax in
// registers, the arithmetic of csrc/tta.hip) or the fp32 sums of the views' probabilities that tc_tta_accumulate leaves.
//
// Both kernels stream [N,ncls,H,W] once: one thread owns a GROUP of consecutive pixels of one image in all their classes.  With P = H * W a
// multiple of the elements in 16 bytes (4 fp32, 8 of a 16-bit type) every class plane starts at the same offset from a 16-byte boundary as
// `scores` itself, so an image is `head` single pixels up to the first boundary, `pieces` groups of one 16-byte load per class (every class
// loaded before the arithmetic starts) and `tail` single pixels; any other P is taken pixel by pixel.  Groups are numbered per image --
// the pieces first, then the head and tail pixels -- and spread over the grid with a stride loop.  The [N,H,W] maps (view-entropy sum, labels,
// outputs) move in pieces of the same pixels where their own address allows it (a host-computed bit each), else element by element.
//
// tc_uncert_maps: no LDS, no atomics, one owner per output element.
// tc_calib_stats: the integer slots (counts, fixed-point sums) are added with 64-bit integer atomics in LDS -- count and correct-count packed in one
// word -- and leave the workgroup as plain stores to its column of `work` ([slot][workgroup]); the two fp64 sums go thread -> wave (xor
// butterfly) -> workgroup (thread 0, waves in order) -> `work`.  calib_final_kernel, one workgroup of 16 waves, adds the columns: a wave per
// slot, lane l takes workgroups l, l + 64, ... in increasing order, then the same butterfly.  No floating-point atomics anywhere.
// Plain C++; the arithmetic of one pixel (uc_pixel) is the same function on every path of both entries.
#include "tc_common.h"
#include "../../include/transception_uncertainty.h"

#include <cfloat>

namespace {

constexpr int kMaxCls = 16;
constexpr int kMaxBins = TC_CALIB_MAX_BINS;
constexpr int kThreads = 256;
constexpr int kMapBlocks = 2048;                 // 256 CUs x 8 workgroups
constexpr int kCalibBlocks = 512;                // 256 CUs x 2: a column of `work` per workgroup
constexpr int kFinalThreads = 1024;

struct UcGeom {
    long long plane;                             // H * W
    long long groups;                            // N * per_image
    int head, pieces, tail;                      // single pixels in front of the first 16-byte boundary, 16-byte pieces, single pixels behind
    int per_image;                               // pieces + head + tail
};

struct UcPixel {
    float conf, h, nll, brier;
    int pred;
};

// One pixel, in registers.  l[0 .. ncls): its logits (KIND 0) or its probability sums (KIND 1) in fp32; y: its label where STATS, which asks
// for nll and brier too.  The loops run to kMaxCls with k < ncls tested inside: fully unrolled, the arrays stay in registers.
template <int KIND, bool STATS>
__device__ __forceinline__ UcPixel uc_pixel(const float (&l)[kMaxCls], int ncls, float inv_views, float logc, int y) {
    UcPixel o;
    o.conf = 0.f; o.pred = 0; o.brier = 0.f; o.nll = 0.f;
    float H;
    if constexpr (KIND == TC_UNCERT_LOGITS) {
        float m = l[0];
#pragma unroll
        for (int k = 1; k < kMaxCls; ++k)
            if (k < ncls) m = fmaxf(m, l[k]);
        float e[kMaxCls], s = 0.f, a = 0.f, dy = 0.f;
#pragma unroll
        for (int k = 0; k < kMaxCls; ++k)
            if (k < ncls) {
                const float d = l[k] - m;
                e[k] = expf(d);
                s += e[k];
                a += e[k] * d;
                if (STATS && k == y) dy = d;
            }
        const float logs = logf(s);
        H = logs - a / s;
        o.nll = logs - dy;
#pragma unroll
        for (int k = 0; k < kMaxCls; ++k)
            if (k < ncls) {
                const float p = e[k] / s;
                if (k == 0 || p > o.conf) { o.conf = p; o.pred = k; }
                if (STATS) { const float d = p - (k == y ? 1.f : 0.f); o.brier += d * d; }
            }
    } else {
        float a = 0.f, py = 0.f;
#pragma unroll
        for (int k = 0; k < kMaxCls; ++k)
            if (k < ncls) {
                const float p = l[k] * inv_views;
                if (k == 0 || p > o.conf) { o.conf = p; o.pred = k; }
                a += p > 0.f ? p * logf(p) : 0.f;
                if (STATS) {
                    const float d = p - (k == y ? 1.f : 0.f);
                    o.brier += d * d;
                    if (k == y) py = p;
                }
            }
        H = -a;
        o.nll = -logf(fmaxf(py, FLT_MIN));
    }
    o.h = ncls == 1 ? 0.f : fminf(1.f, fmaxf(0.f, H / logc));
    return o;
}

// PX consecutive pixels of every class plane of one image: PX = 1, or the elements of one 16-byte piece, kept as loaded
template <typename T, int PX> struct UcTile {
    uint4 raw[kMaxCls];
    __device__ __forceinline__ void load(int k, const T* p) { raw[k] = *reinterpret_cast<const uint4*>(p); }
    __device__ __forceinline__ float get(int k, int j) const {
        const unsigned w[4] = {raw[k].x, raw[k].y, raw[k].z, raw[k].w};
        if constexpr (std::is_same<T, float>::value) return __uint_as_float(w[j]);
        else {
            float lo, hi;
            unpack2<T>(w[j >> 1], lo, hi);
            return (j & 1) ? hi : lo;
        }
    }
};
template <typename T> struct UcTile<T, 1> {
    float v[kMaxCls];
    __device__ __forceinline__ void load(int k, const T* p) { v[k] = ldf<T>(p); }
    __device__ __forceinline__ float get(int k, int) const { return v[k]; }
};

// PX elements of an [N,H,W] map: in 16-byte (floats) / PX-byte (bytes) pieces where `vec`, else one by one
template <int PX> __device__ __forceinline__ void uc_load_f(const float* p, float (&v)[PX], bool vec) {
    if constexpr (PX > 1) {
        if (vec) {
#pragma unroll
            for (int q = 0; q < PX / 4; ++q) {
                const float4 t = *reinterpret_cast<const float4*>(p + 4 * q);
                v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) v[j] = p[j];
}
template <int PX> __device__ __forceinline__ void uc_store_f(float* p, const float (&v)[PX], bool vec) {
    if constexpr (PX > 1) {
        if (vec) {
#pragma unroll
            for (int q = 0; q < PX / 4; ++q) *reinterpret_cast<float4*>(p + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) p[j] = v[j];
}
template <int PX> __device__ __forceinline__ void uc_load_b(const unsigned char* p, int (&v)[PX], bool vec) {
    if constexpr (PX > 1) {
        if (vec) {
#pragma unroll
            for (int q = 0; q < PX / 4; ++q) {
                const unsigned w = reinterpret_cast<const unsigned*>(p)[q];
#pragma unroll
                for (int b = 0; b < 4; ++b) v[4 * q + b] = (int)((w >> (8 * b)) & 255u);
            }
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) v[j] = p[j];
}
template <int PX> __device__ __forceinline__ void uc_store_b(unsigned char* p, const int (&v)[PX], bool vec) {
    if constexpr (PX > 1) {
        if (vec) {
#pragma unroll
            for (int q = 0; q < PX / 4; ++q)
                reinterpret_cast<unsigned*>(p)[q] = (unsigned)v[4 * q] | ((unsigned)v[4 * q + 1] << 8) | ((unsigned)v[4 * q + 2] << 16) | ((unsigned)v[4 * q + 3] << 24);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) p[j] = (unsigned char)v[j];
}

// group i of the grid-stride loop -> (image, first pixel, whether it is a 16-byte piece)
__device__ __forceinline__ bool uc_group(const UcGeom& g, long long i, int vec, long long& n, int& p0) {
    n = i / g.per_image;
    const int r = (int)(i - n * g.per_image);
    if (r < g.pieces) { p0 = g.head + r * vec; return true; }
    const int s = r - g.pieces;
    p0 = s < g.head ? s : (int)g.plane - g.tail + (s - g.head);
    return false;
}

enum { UC_VES = 1, UC_ENT = 2, UC_CONF = 4, UC_MI = 8, UC_PRED = 16, UC_LABELS = 1 };     // the bits of `aligned`

template <typename T, int KIND, int PX>
__device__ __forceinline__ void uc_maps_group(const T* __restrict__ scores, const float* ves, float* ent, float* conf, float* mi,
                                              unsigned char* pred, long long plane, long long n, int p0, int ncls, float inv_views, float logc,
                                              unsigned aligned) {
    const T* src = scores + n * ncls * plane + p0;
    const long long pix = n * plane + p0;
    UcTile<T, PX> tile;
#pragma unroll
    for (int k = 0; k < kMaxCls; ++k)
        if (k < ncls) tile.load(k, src + k * plane);
    float vs[PX];
    if (ves) uc_load_f<PX>(ves + pix, vs, aligned & UC_VES);
    float h[PX], c[PX], m[PX];
    int lab[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        float l[kMaxCls];
#pragma unroll
        for (int k = 0; k < kMaxCls; ++k) l[k] = k < ncls ? tile.get(k, j) : 0.f;
        const UcPixel px = uc_pixel<KIND, false>(l, ncls, inv_views, logc, -1);
        h[j] = px.h; c[j] = px.conf; lab[j] = px.pred;
        m[j] = ves ? fmaxf(0.f, px.h - vs[j] * inv_views) : 0.f;
    }
    if (ent) uc_store_f<PX>(ent + pix, h, aligned & UC_ENT);
    if (conf) uc_store_f<PX>(conf + pix, c, aligned & UC_CONF);
    if (mi) uc_store_f<PX>(mi + pix, m, aligned & UC_MI);
    if (pred) uc_store_b<PX>(pred + pix, lab, aligned & UC_PRED);
}

template <typename T, int KIND> __global__ __launch_bounds__(kThreads)
void uncert_maps_kernel(const T* __restrict__ scores, const float* ves, float* ent, float* conf, float* mi, unsigned char* pred, UcGeom g, int ncls,
                        float inv_views, unsigned aligned) {
    constexpr int VEC = TcVec16<T>::N;
    const float logc = logf((float)ncls);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < g.groups; i += (long long)gridDim.x * kThreads) {
        long long n;
        int p0;
        if (uc_group(g, i, VEC, n, p0)) uc_maps_group<T, KIND, VEC>(scores, ves, ent, conf, mi, pred, g.plane, n, p0, ncls, inv_views, logc, aligned);
        else uc_maps_group<T, KIND, 1>(scores, ves, ent, conf, mi, pred, g.plane, n, p0, ncls, inv_views, logc, 0u);
    }
}

struct UcSums {
    double nll, brier;
};

template <typename T, int KIND, int PX>
__device__ __forceinline__ void uc_calib_group(const T* __restrict__ scores, const unsigned char* __restrict__ labels, long long plane, long long n,
                                               int p0, int ncls, float inv_views, float logc, int ignore_index, bool fg, int bins, unsigned aligned,
                                               unsigned long long* tab, UcSums& acc) {
    const T* src = scores + n * ncls * plane + p0;
    UcTile<T, PX> tile;
#pragma unroll
    for (int k = 0; k < kMaxCls; ++k)
        if (k < ncls) tile.load(k, src + k * plane);
    int y[PX];
    uc_load_b<PX>(labels + n * plane + p0, y, aligned & UC_LABELS);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        if (y[j] == ignore_index || y[j] >= ncls) continue;
        float l[kMaxCls];
#pragma unroll
        for (int k = 0; k < kMaxCls; ++k) l[k] = k < ncls ? tile.get(k, j) : 0.f;
        const UcPixel px = uc_pixel<KIND, true>(l, ncls, inv_views, logc, y[j]);
        if (fg && y[j] == 0 && px.pred == 0) continue;
        const int b = max(0, min(bins - 1, (int)(px.conf * (float)bins)));
        const unsigned long long one = 1ull | ((unsigned long long)(px.pred == y[j]) << 32);     // (count, correct) in one word
        atomicAdd(&tab[2 * b], one);
        atomicAdd(&tab[2 * b + 1], (unsigned long long)(long long)(px.conf * 4294967296.0f));
        atomicAdd(&tab[2 * kMaxBins + 2 * px.pred], one);
        atomicAdd(&tab[2 * kMaxBins + 2 * px.pred + 1], (unsigned long long)(long long)(px.h * 4294967296.0f));
        acc.nll += (double)px.nll;
        acc.brier += (double)px.brier;
    }
}

// slot s of `out` from a workgroup's LDS table: (n, fixed-point sum, correct) per bin, then per class behind the four totals
__device__ __forceinline__ long long uc_table_slot(const unsigned long long* tab, int row, int c) {
    const unsigned long long counts = tab[2 * row];
    return c == 0 ? (long long)(counts & 0xffffffffull) : c == 1 ? (long long)tab[2 * row + 1] : (long long)(counts >> 32);
}

template <typename T, int KIND> __global__ __launch_bounds__(kThreads)
void calib_stats_kernel(const T* __restrict__ scores, const unsigned char* __restrict__ labels, UcGeom g, int ncls, float inv_views, int ignore_index,
                        int fg, int bins, unsigned aligned, long long* __restrict__ work) {
    constexpr int VEC = TcVec16<T>::N;
    __shared__ unsigned long long tab[2 * kMaxBins + 2 * kMaxCls];        // [bins] then [ncls]: (count | correct << 32, fixed-point sum)
    __shared__ double part[kThreads / 64][2];
    for (int i = threadIdx.x; i < 2 * kMaxBins + 2 * kMaxCls; i += kThreads) tab[i] = 0ull;
    __syncthreads();
    const float logc = logf((float)ncls);
    UcSums acc = {0.0, 0.0};
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < g.groups; i += (long long)gridDim.x * kThreads) {
        long long n;
        int p0;
        if (uc_group(g, i, VEC, n, p0))
            uc_calib_group<T, KIND, VEC>(scores, labels, g.plane, n, p0, ncls, inv_views, logc, ignore_index, fg != 0, bins, aligned, tab, acc);
        else
            uc_calib_group<T, KIND, 1>(scores, labels, g.plane, n, p0, ncls, inv_views, logc, ignore_index, fg != 0, bins, 0u, tab, acc);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {                               // a + b == b + a: every lane holds the same bits
        acc.nll += __shfl_xor(acc.nll, off, 64);
        acc.brier += __shfl_xor(acc.brier, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = acc.nll; part[threadIdx.x >> 6][1] = acc.brier; }
    __syncthreads();                                                       // the table is complete, the waves' sums are in `part`
    const int s = threadIdx.x, totals = 3 * bins, slots = totals + 4 + 3 * ncls;
    if (s >= slots) return;
    long long v;
    if (s < totals) v = uc_table_slot(tab, s / 3, s % 3);
    else if (s >= totals + 4) v = uc_table_slot(tab, kMaxBins + (s - totals - 4) / 3, (s - totals - 4) % 3);
    else if (s == totals || s == totals + 3) {                             // n, n correct: over the bins
        long long t = 0;
        for (int b = 0; b < bins; ++b) t += uc_table_slot(tab, b, s == totals ? 0 : 2);
        v = t;
    } else {                                                               // the fp64 sums: the waves in order
        double t = part[0][s - totals - 1];
        for (int w = 1; w < kThreads / 64; ++w) t += part[w][s - totals - 1];
        v = __double_as_longlong(t);
    }
    work[(long long)s * gridDim.x + blockIdx.x] = v;
}

// one workgroup: column sums of `work` [slots][blocks] into `out`; slots f64 and f64 + 1 hold doubles
__global__ __launch_bounds__(kFinalThreads)
void calib_final_kernel(const long long* __restrict__ work, int blocks, int slots, int f64, long long* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int s = threadIdx.x >> 6; s < slots; s += kFinalThreads / 64) {   // wave-uniform
        const long long* col = work + (long long)s * blocks;
        long long v;
        if (s == f64 || s == f64 + 1) {
            double a = 0.0;
            for (int b = lane; b < blocks; b += 64) a += __longlong_as_double(col[b]);
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) a += __shfl_xor(a, off, 64);
            v = __double_as_longlong(a);
        } else {
            long long a = 0;
            for (int b = lane; b < blocks; b += 64) a += col[b];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) a += __shfl_xor(a, off, 64);
            v = a;
        }
        if (lane == 0) out[s] = v;
    }
}

// a * b * c < 2^31 for positive ints, without overflow on the way
bool uc_below_2g(int a, int b, int c) {
    const long long ab = (long long)a * b;
    return ab <= 0x7fffffffLL && ab * c <= 0x7fffffffLL;
}

// what both entries refuse about the scores
bool uc_scores_ok(const void* scores, int dtype, int kind, float inv_views, int N, int ncls, int H, int W) {
    if (!scores || N <= 0 || H <= 0 || W <= 0 || ncls < 1 || ncls > kMaxCls) return false;
    if (kind != TC_UNCERT_LOGITS && kind != TC_UNCERT_PROB_SUMS) return false;
    if (dtype != TC_F32 && dtype != TC_BF16 && dtype != TC_F16) return false;
    if (kind == TC_UNCERT_PROB_SUMS && dtype != TC_F32) return false;
    if (!(inv_views > 0.f && inv_views <= 1.f)) return false;                                  // !(...): false for a NaN
    return uc_below_2g(N, ncls, H) && uc_below_2g(N * ncls * H, W, 1);
}

template <typename T> UcGeom uc_geom(const void* scores, int N, int H, int W) {
    constexpr int VEC = TcVec16<T>::N;
    UcGeom g;
    g.plane = (long long)H * W;
    const uintptr_t a = (uintptr_t)scores;
    g.head = (int)g.plane;                                                                     // every pixel on its own
    if (g.plane % VEC == 0 && a % sizeof(T) == 0) g.head = (int)(((16 - a % 16) % 16) / sizeof(T));   // < VEC <= plane
    g.pieces = (int)((g.plane - g.head) / VEC);
    g.tail = (int)(g.plane - g.head - (long long)g.pieces * VEC);
    g.per_image = g.pieces + g.head + g.tail;
    g.groups = (long long)N * g.per_image;
    return g;
}

// an [N,H,W] map of `elem`-byte elements moves in pieces of `bytes` bytes: its first piece, `head` elements in, sits on such a boundary
bool uc_aligned(const void* p, int head, int elem, int bytes) { return p && ((uintptr_t)p + (uintptr_t)head * elem) % bytes == 0; }

template <typename T, int KIND>
void uc_maps_launch(const void* scores, float inv_views, const float* ves, float* ent, float* conf, float* mi, unsigned char* pred, int N, int ncls,
                    int H, int W, hipStream_t s) {
    constexpr int VEC = TcVec16<T>::N;
    const UcGeom g = uc_geom<T>(scores, N, H, W);
    const unsigned aligned = (uc_aligned(ves, g.head, 4, 16) ? UC_VES : 0) | (uc_aligned(ent, g.head, 4, 16) ? UC_ENT : 0) |
                             (uc_aligned(conf, g.head, 4, 16) ? UC_CONF : 0) | (uc_aligned(mi, g.head, 4, 16) ? UC_MI : 0) |
                             (uc_aligned(pred, g.head, 1, VEC) ? UC_PRED : 0);
    hipLaunchKernelGGL((uncert_maps_kernel<T, KIND>), dim3(tc_blocks(g.groups, kThreads, kMapBlocks)), dim3(kThreads), 0, s, (const T*)scores, ves, ent,
                       conf, mi, pred, g, ncls, inv_views, aligned);
}

template <typename T, int KIND>
void uc_calib_launch(const void* scores, float inv_views, const unsigned char* labels, int ignore_index, int flags, int bins, int N, int ncls, int H,
                     int W, long long* work, long long* out, hipStream_t s) {
    constexpr int VEC = TcVec16<T>::N;
    const UcGeom g = uc_geom<T>(scores, N, H, W);
    const unsigned aligned = uc_aligned(labels, g.head, 1, VEC) ? UC_LABELS : 0;
    const int blocks = tc_blocks(g.groups, kThreads, kCalibBlocks), slots = 3 * bins + 4 + 3 * ncls;
    hipLaunchKernelGGL((calib_stats_kernel<T, KIND>), dim3(blocks), dim3(kThreads), 0, s, (const T*)scores, labels, g, ncls, inv_views,
                       ignore_index >= 0 && ignore_index <= 255 ? ignore_index : -1, flags & TC_CALIB_FOREGROUND, bins, aligned, work);
    hipLaunchKernelGGL(calib_final_kernel, dim3(1), dim3(kFinalThreads), 0, s, (const long long*)work, blocks, slots, 3 * bins + 1, out);
}

}  // namespace

extern "C" int tc_uncert_abi_version(void) { return TC_UNCERT_ABI_VERSION; }

extern "C" int tc_calib_out_slots(int bins, int ncls) {
    return bins < 1 || bins > kMaxBins || ncls < 1 || ncls > kMaxCls ? 0 : 3 * bins + 4 + 3 * ncls;
}

extern "C" long long tc_calib_work_bytes(int bins, int ncls) { return (long long)kCalibBlocks * 8 * tc_calib_out_slots(bins, ncls); }

extern "C" int tc_uncert_maps(const void* scores, int dtype, int kind, float inv_views, const float* view_entropy_sum, float* entropy, float* confidence,
                              float* mutual_info, unsigned char* pred, int N, int ncls, int H, int W, void* stream) {
    if (!uc_scores_ok(scores, dtype, kind, inv_views, N, ncls, H, W) || (!entropy && !confidence && !mutual_info && !pred) ||
        (mutual_info != nullptr) != (view_entropy_sum != nullptr) || (const void*)entropy == scores || (const void*)confidence == scores ||
        (const void*)mutual_info == scores || (const void*)pred == scores)
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (kind == TC_UNCERT_PROB_SUMS)
        uc_maps_launch<float, TC_UNCERT_PROB_SUMS>(scores, inv_views, view_entropy_sum, entropy, confidence, mutual_info, pred, N, ncls, H, W, s);
    else
        TC_DISPATCH_DTYPE(dtype, (uc_maps_launch<T, TC_UNCERT_LOGITS>(scores, inv_views, view_entropy_sum, entropy, confidence, mutual_info, pred, N,
                                                                      ncls, H, W, s)));
    return tc_launch_status();
}

extern "C" int tc_calib_stats(const void* scores, int dtype, int kind, float inv_views, const unsigned char* labels, int ignore_index, int flags,
                              int bins, int N, int ncls, int H, int W, void* work, long long* out, void* stream) {
    if (!uc_scores_ok(scores, dtype, kind, inv_views, N, ncls, H, W) || !labels || !work || !out || bins < 1 || bins > kMaxBins ||
        (flags & ~TC_CALIB_FOREGROUND))
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (kind == TC_UNCERT_PROB_SUMS)
        uc_calib_launch<float, TC_UNCERT_PROB_SUMS>(scores, inv_views, labels, ignore_index, flags, bins, N, ncls, H, W, (long long*)work, out, s);
    else
        TC_DISPATCH_DTYPE(dtype, (uc_calib_launch<T, TC_UNCERT_LOGITS>(scores, inv_views, labels, ignore_index, flags, bins, N, ncls, H, W,
                                                                       (long long*)work, out, s)));
    return tc_launch_status();
}

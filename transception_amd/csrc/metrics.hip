// Evaluation metrics on the device: the device side of calculate_metric_percase (utils.py:50-60, called per class at utils.py:96-98) --
// per-class Dice counts and the exact HD95 order statistics of a predicted label volume against a ground-truth one, both uint8 [D,H,W].
//
//   surface voxel of a mask  = mask voxel with at least one of its 6 face neighbours outside the mask, the outside of the array counting as
//                              background (scipy binary_erosion, connectivity 1, border_value 0);
//   distance                 = Euclidean, from every surface voxel of one mask to the nearest surface voxel of the other, both directions
//                              pooled; with a voxel spacing (sz, sy, sx) the squared distance is (sz dz)^2 + (sy dy)^2 + (sx dx)^2;
//   HD95                     = numpy.percentile(pooled, 95).
//
// (1) One pass writes a surface map per label volume (a voxel has one label, so surf[v] = lab[v] on the surface of class lab[v], else 0,
// holds every class) and the Dice counts; (2) the squared Euclidean distance transform to {surf == k} is separable: the distance to the
// nearest source inside the row, then out[i] = min_j f[j] + (s (i-j))^2 along y and along z -- one body per pass, instantiated for int32
// maps (unit spacing: every squared distance is an integer) and for float64 maps; then the two order statistics around position
// 0.95 (n-1) of the squared distances met on the other mask's surface: (3, 4) with unit spacing from a histogram indexed by the squared
// distance, (5) with a spacing by a radix select over the doubles.  Integer atomics only, so no result depends on arrival order.  The
// host takes two square roots.
#include "tc_common.h"

#define MT_MAXCLS 16
#define MT_MAXDIM 2048                    // longest line: a [L][8] tile is 64 KB (int32) or 128 KB (float64) of the 160 KB LDS, and 3 * 2047^2 + 2^28 stays far inside int32
#define MT_INF TC_METRIC_NO_SOURCE

// ---- (1) surfaces and counts -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned char mt_surface(const unsigned char* __restrict__ lab, int v, int z, int y, int x, int D, int H, int W,
                                                    int ncls, int zfaces) {
    const unsigned char c = lab[v];
    if (c == 0 || c >= ncls) return 0;
    bool edge = x == 0 || x == W - 1 || y == 0 || y == H - 1 || (zfaces && (z == 0 || z == D - 1));
    if (!edge) {                                                                   // all six neighbours are inside the array
        edge = lab[v - 1] != c || lab[v + 1] != c || lab[v - W] != c || lab[v + W] != c;
        if (zfaces) edge = edge || lab[v - H * W] != c || lab[v + H * W] != c;
        return edge ? c : 0;
    }
    bool out = (x == 0 || lab[v - 1] != c) || (x == W - 1 || lab[v + 1] != c) || (y == 0 || lab[v - W] != c) || (y == H - 1 || lab[v + W] != c);
    if (zfaces) out = out || (z == 0 || lab[v - H * W] != c) || (z == D - 1 || lab[v + H * W] != c);
    return out ? c : 0;
}

// counts[3k..3k+2] += (|P==k & G==k|, |P==k|, |G==k|): per class one ballot + popcount per wave and voxel batch (wave-uniform partial sums),
// then one LDS add per wave and one global atomic per workgroup and counter.
__global__ __launch_bounds__(256) void metric_surfaces_kernel(const unsigned char* __restrict__ P, const unsigned char* __restrict__ G,
                                                              unsigned char* __restrict__ sP, unsigned char* __restrict__ sG,
                                                              unsigned long long* __restrict__ counts, int D, int H, int W, int ncls, int zfaces) {
    __shared__ int lc[3 * MT_MAXCLS];
    if (threadIdx.x < 3 * MT_MAXCLS) lc[threadIdx.x] = 0;
    __syncthreads();
    const int n = D * H * W, HW = H * W, lane = threadIdx.x & 63;
    int ci[MT_MAXCLS], cp[MT_MAXCLS], cg[MT_MAXCLS];
#pragma unroll
    for (int k = 0; k < MT_MAXCLS; ++k) ci[k] = cp[k] = cg[k] = 0;
    // every lane of a wave runs the same number of iterations (the ballots need the whole wave); `ok` masks the tail
    for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); base < n; base += (long long)gridDim.x * 256) {
        const long long vv = base + lane;
        const bool ok = vv < n;
        const int v = ok ? (int)vv : 0;
        const int z = v / HW, r = v - z * HW, y = r / W, x = r - y * W;
        const int p = ok ? P[v] : 255, g = ok ? G[v] : 255;
        if (ok) {
            sP[v] = mt_surface(P, v, z, y, x, D, H, W, ncls, zfaces);
            sG[v] = mt_surface(G, v, z, y, x, D, H, W, ncls, zfaces);
        }
#pragma unroll
        for (int k = 0; k < MT_MAXCLS; ++k) {
            if (k < ncls) {
                const unsigned long long mp = __ballot(p == k), mg = __ballot(g == k);
                cp[k] += __popcll(mp); cg[k] += __popcll(mg); ci[k] += __popcll(mp & mg);
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < MT_MAXCLS; ++k) {
            if (k < ncls) {
                if (ci[k]) atomicAdd(&lc[3 * k], ci[k]);
                if (cp[k]) atomicAdd(&lc[3 * k + 1], cp[k]);
                if (cg[k]) atomicAdd(&lc[3 * k + 2], cg[k]);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * ncls && lc[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)lc[threadIdx.x]);
}

// ---- (2) exact squared Euclidean distance transform ---------------------------------------------------------------------------------
// What the element type of a map decides: the value where there is no source, the squared length of d steps of size s, and the minimum.
template <typename T> struct MtElem;
template <> struct MtElem<int> {
    static __device__ __forceinline__ int none() { return MT_INF; }
    static __device__ __forceinline__ int sq(double, int d) { return d * d; }                  // unit spacing
    static __device__ __forceinline__ int min(int a, int b) { return ::min(a, b); }
};
template <> struct MtElem<double> {
    static __device__ __forceinline__ double none() { return __builtin_huge_val(); }
    static __device__ __forceinline__ double sq(double s, int d) { const double t = s * d; return t * t; }
    static __device__ __forceinline__ double min(double a, double b) { return fmin(a, b); }
};

// x: one wave per row.  The row's sources become one 64-bit ballot per 64 voxels; a voxel finds the nearest set bit on either side with
// clz / ffs, walking whole words where its own has none: d2 = (sx dx)^2, "no source" in a row without one.
template <typename T>
__global__ __launch_bounds__(256) void metric_edt_x_kernel(const unsigned char* __restrict__ surf, int k, T* __restrict__ d2, int rows, int W, double sx) {
    __shared__ unsigned long long masks[4][MT_MAXDIM / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    const bool live = row < rows;
    const int nch = (W + 63) >> 6;
    const unsigned char* s = surf + (long long)(live ? row : 0) * W;
    unsigned long long any = 0;
    for (int c = 0; c < nch; ++c) {
        const int x = c * 64 + lane;
        const unsigned long long m = __ballot(live && x < W && s[x] == k);
        if (lane == 0) masks[wave][c] = m;
        any |= m;
    }
    __syncthreads();
    if (!live) return;
    T* o = d2 + (long long)row * W;
    for (int c0 = 0; c0 < nch; ++c0) {
        const int x = c0 * 64 + lane;
        if (x >= W) break;
        T best = MtElem<T>::none();
        if (any) {
            int near = MT_MAXDIM, c = c0;
            unsigned long long m = masks[wave][c] & (~0ull >> (63 - lane));          // sources at or left of x
            while (m == 0 && c > 0) m = masks[wave][--c];
            if (m) near = x - (c * 64 + 63 - __clzll((long long)m));
            c = c0;
            m = masks[wave][c] & (~0ull << lane);                                     // sources at or right of x
            while (m == 0 && c < nch - 1) m = masks[wave][++c];
            if (m) near = min(near, c * 64 + __ffsll((unsigned long long)m) - 1 - x);
            best = MtElem<T>::sq(sx, near);
        }
        o[x] = best;
    }
}

// y and z: the array is [outer][L][inner] with the pass along L (y: outer = D, inner = W; z: outer = 1, inner = H*W) and out[i] =
// min_j f[j] + (s (i-j))^2.  A workgroup stages TX neighbouring lines in LDS ([L][TX], lanes along the contiguous axis so global accesses
// stay coalesced; a half-wave reads whole neighbouring rows of the tile, 128 or 256 contiguous bytes: conflict-free, and every lane of a
// wave is at the same step d of its scan) and, for every output i, scans j outwards from i until (s (i-j))^2 can no longer beat the best
// found.  In place: a workgroup reads its whole tile before it writes, and no other workgroup touches those lines.  A line without any
// finite value is left as it is (min_j of "no source" + (s (i-j))^2 is "no source" at j = i: 2^28 or +inf), so only lines that the
// earlier passes reached are scanned.
template <typename T, int TX>
__global__ __launch_bounds__(256) void metric_edt_line_kernel(T* __restrict__ d2, int L, long long inner, double s) {
    extern __shared__ double mt_lds[];                                              // one declaration for both element types, 8-byte aligned
    T* tile = (T*)mt_lds;
    constexpr int NY = 256 / TX;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const long long col = (long long)blockIdx.x * TX + tx;
    const bool ok = col < inner;
    T* base = d2 + (long long)blockIdx.y * L * inner + (ok ? col : 0);
    int* col_finite = (int*)(tile + L * TX);                                        // a line without a source stays as it is: nothing to scan for
    if (threadIdx.x < TX) col_finite[threadIdx.x] = 0;
    __syncthreads();
    const T none = MtElem<T>::none();
    int finite = 0;
    for (int i = ty; i < L; i += NY) {
        const T v = ok ? base[i * inner] : none;
        tile[i * TX + tx] = v;
        finite |= v < none;
    }
    if (finite) col_finite[tx] = 1;
    if (!__syncthreads_or(finite)) return;
    if (!col_finite[tx]) return;                                                    // (no barrier follows)
    for (int i = ty; i < L; i += NY) {
        T best = tile[i * TX + tx];
        const int far = max(i, L - 1 - i);
        for (int d = 1; d <= far; ++d) {
            const T dd = MtElem<T>::sq(s, d);
            if (!(dd < best)) break;
            if (i - d >= 0) best = MtElem<T>::min(best, tile[(i - d) * TX + tx] + dd);
            if (i + d < L) best = MtElem<T>::min(best, tile[(i + d) * TX + tx] + dd);
        }
        if (ok) base[i * inner] = best;
    }
}

// TX is the widest of 32, 16, 8 lines whose [L][TX] tile is at most 64 KB (so two workgroups share a compute unit), else 8: 32 / 16 / 8
// for L <= 512 / 1024 / 2048 on int32 and for L <= 256 / 512 / 2048 on float64 -- at L = 512, 1024, 2048 (int32) and 256, 512, 2048
// (float64) that is 32, 16, 8.  Behind the tile lies one flag per line: up to 64 KB + 128 B (int32), 128 KB + 32 B (float64).
template <typename T>
static int mt_line_pass(T* d2, int outer, int L, long long inner, double sp, hipStream_t s) {
    if (L <= 1) return TC_OK;
    const size_t fits = 64 * 1024 / sizeof(T);
    const int tx = (size_t)L * 32 <= fits ? 32 : ((size_t)L * 16 <= fits ? 16 : 8);
    const size_t smem = (size_t)L * tx * sizeof(T) + tx * sizeof(int);
    const dim3 grid((unsigned)((inner + tx - 1) / tx), (unsigned)outer);
    void (*fn)(T*, int, long long, double) = tx == 32 ? metric_edt_line_kernel<T, 32> : (tx == 16 ? metric_edt_line_kernel<T, 16> : metric_edt_line_kernel<T, 8>);
    if (smem > 64 * 1024 && hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) return TC_ERR_LAUNCH;
    hipLaunchKernelGGL(fn, grid, dim3(256), smem, s, d2, L, inner, sp);
    return tc_launch_status();
}

template <typename T>
static int mt_edt(const unsigned char* surf, int k, T* d2, int D, int H, int W, int zfaces, double sz, double sy, double sx, hipStream_t s) {
    const int rows = D * H;
    hipLaunchKernelGGL(metric_edt_x_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, s, surf, k, d2, rows, W, sx);
    int rc = tc_launch_status();
    if (rc == TC_OK) rc = mt_line_pass(d2, D, H, W, sy, s);
    if (rc == TC_OK && zfaces) rc = mt_line_pass(d2, 1, D, (long long)H * W, sz, s);
    return rc;
}

// ---- (3) histogram of squared distances ----------------------------------------------------------------------------------------------
// The pooled multiset of class k: d2_gt on the prediction's surface and d2_pred on the ground truth's, each value handed to `f`.
template <typename T, typename F>
__device__ __forceinline__ void mt_for_pooled(const unsigned char* __restrict__ sP, const unsigned char* __restrict__ sG, const T* __restrict__ d2P,
                                              const T* __restrict__ d2G, int k, int n, F f) {
    for (long long v = (long long)blockIdx.x * 256 + threadIdx.x; v < n; v += (long long)gridDim.x * 256) {
        if (sP[v] == k) f(d2G[v]);
        if (sG[v] == k) f(d2P[v]);
    }
}

__global__ __launch_bounds__(256) void metric_hist_kernel(const unsigned char* __restrict__ sP, const unsigned char* __restrict__ sG,
                                                          const int* __restrict__ d2P, const int* __restrict__ d2G, int k,
                                                          unsigned int* __restrict__ hist, long long nbins, int n) {
    mt_for_pooled(sP, sG, d2P, d2G, k, n, [&](int d) { if (d < nbins) atomicAdd(&hist[d], 1u); });    // d >= nbins only when the other surface is empty
}

// ---- (4) order statistics --------------------------------------------------------------------------------------------------------------
// One workgroup per class: every thread sums one contiguous run of bins, thread 0 walks the 256 partial sums to the run that holds each
// wanted position and then that run.
__global__ __launch_bounds__(256) void metric_select_kernel(const unsigned int* __restrict__ hist, long long nbins, long long* __restrict__ out) {
    __shared__ unsigned long long part[256];
    const unsigned int* h = hist + (long long)blockIdx.x * nbins;
    const long long run = (nbins + 255) / 256, b0 = threadIdx.x * run, b1 = b0 + run < nbins ? b0 + run : nbins;
    unsigned long long sum = 0;
    for (long long b = b0; b < b1; ++b) sum += h[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long n = 0;
    for (int t = 0; t < 256; ++t) n += part[t];
    long long* o = out + 3 * blockIdx.x;
    o[0] = (long long)n; o[1] = 0; o[2] = 0;
    if (n == 0) return;
    // the host forms the same IEEE fp64 product 0.95 * (n-1) (evaluate.hd95_from_order_stats), so its floor and fraction belong to these positions
    const unsigned long long lo = (unsigned long long)floor(0.95 * (double)(n - 1)), hi = lo + 1 < n ? lo + 1 : n - 1;
    const unsigned long long want[2] = {lo, hi};
    for (int w = 0; w < 2; ++w) {
        unsigned long long before = 0;
        int t = 0;
        while (before + part[t] <= want[w]) before += part[t++];                      // terminates: want < n = sum of part
        long long b = t * run;
        while (before + h[b] <= want[w]) before += h[b++];                            // and the run's bins sum to part[t]
        o[1 + w] = b;
    }
}

// ---- (5) order statistics of float64 maps -----------------------------------------------------------------------------------------------
// With a spacing a squared distance is no integer any more, so there is no histogram to index with it.  The two order statistics come from
// a most-significant-digit radix select over the bit patterns (non-negative doubles order like their bits read as uint64): integer
// histograms of one 8-bit digit per pass, eight passes.
#define MT_F64_INF_BITS 0x7ff0000000000000ull
#define MT_SEL_PASSES 8
#define MT_SEL_HIST_WORDS (MT_SEL_PASSES * 2 * 256)       // uint32 [pass][wanted position][digit], then one MtSelState
struct MtSelState { unsigned long long prefix[2], rank[2], n; };   // per wanted position: the digits fixed so far and the position among the values that share them
static_assert(MT_SEL_HIST_WORDS * 4 + sizeof(MtSelState) <= TC_METRIC_SELECT_WORK_BYTES, "the header's work size");

// One pass of the radix select over the pooled multiset (+inf, the distance to an empty surface, is not counted).  Of the values whose
// leading 8 * pass bits equal the prefix fixed for a wanted position, the next 8-bit digit is counted: in LDS first, then one global atomic
// per workgroup and used bin.  While both positions share their prefix (always in pass 0) only row 0 is filled.
__global__ __launch_bounds__(256) void metric_select_count_kernel(const unsigned char* __restrict__ sP, const unsigned char* __restrict__ sG,
                                                                  const double* __restrict__ d2P, const double* __restrict__ d2G, int k,
                                                                  unsigned int* __restrict__ work, int pass, int n) {
    __shared__ unsigned int lh[2][256];
    lh[0][threadIdx.x] = 0; lh[1][threadIdx.x] = 0;
    const MtSelState* st = (const MtSelState*)(work + MT_SEL_HIST_WORDS);
    const unsigned long long p0 = pass ? st->prefix[0] : 0, p1 = pass ? st->prefix[1] : 0;
    const int shift = 56 - 8 * pass;
    __syncthreads();
    auto count = [&](double x) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(x);
        if (b >= MT_F64_INF_BITS) return;
        const unsigned long long lead = pass ? b >> (shift + 8) : 0;
        const int digit = (int)(b >> shift) & 255;
        if (lead == p0) atomicAdd(&lh[0][digit], 1u);
        else if (lead == p1) atomicAdd(&lh[1][digit], 1u);
    };
    mt_for_pooled(sP, sG, d2P, d2G, k, n, count);
    __syncthreads();
    unsigned int* hist = work + pass * 512;
    if (lh[0][threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[0][threadIdx.x]);
    if (lh[1][threadIdx.x]) atomicAdd(&hist[256 + threadIdx.x], lh[1][threadIdx.x]);
}

// One workgroup: an inclusive scan over the 256 bins of each wanted position, and the thread whose bin holds the position appends its
// digit to the prefix and keeps the position inside the bin.  Pass 0 also fixes n and the two positions; the last pass writes the result.
__global__ __launch_bounds__(256) void metric_select_scan_kernel(unsigned int* __restrict__ work, int pass, long long* __restrict__ out) {
    __shared__ unsigned long long inc[2][256];
    MtSelState* st = (MtSelState*)(work + MT_SEL_HIST_WORDS);
    const unsigned int* hist = work + pass * 512;
    const int t = threadIdx.x;
    const unsigned long long p[2] = {pass ? st->prefix[0] : 0, pass ? st->prefix[1] : 0};
    unsigned long long rank[2] = {pass ? st->rank[0] : 0, pass ? st->rank[1] : 0}, n = pass ? st->n : 0;
    const unsigned long long h[2] = {hist[t], p[0] != p[1] ? hist[256 + t] : hist[t]};
    inc[0][t] = h[0]; inc[1][t] = h[1];
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned long long a = t >= off ? inc[0][t - off] : 0, b = t >= off ? inc[1][t - off] : 0;
        __syncthreads();
        inc[0][t] += a; inc[1][t] += b;
        __syncthreads();
    }
    if (pass == 0) {
        n = inc[0][255];
        if (n) {
            // the host forms the same IEEE fp64 product 0.95 * (n-1) (evaluate.hd95_from_order_stats), so its floor and fraction belong to these positions
            rank[0] = (unsigned long long)floor(0.95 * (double)(n - 1));
            rank[1] = rank[0] + 1 < n ? rank[0] + 1 : n - 1;
        }
        if (t == 0) st->n = n;
    }
    if (n == 0) {                                                                    // (uniform) an empty multiset: (0, 0.0, 0.0)
        if (t == 0 && pass == MT_SEL_PASSES - 1) { out[0] = 0; out[1] = 0; out[2] = 0; }
        return;
    }
    for (int w = 0; w < 2; ++w) {
        const unsigned long long before = inc[w][t] - h[w];
        if (h[w] && before <= rank[w] && rank[w] < inc[w][t]) {                      // exactly one thread: rank < the bins' total
            const unsigned long long q = (p[w] << 8) | (unsigned long long)t;
            st->prefix[w] = q; st->rank[w] = rank[w] - before;
            if (pass == MT_SEL_PASSES - 1) out[1 + w] = (long long)q;                // all 64 bits: the double itself
        }
    }
    if (t == 0 && pass == MT_SEL_PASSES - 1) out[0] = (long long)n;
}

// ---- entries ------------------------------------------------------------------------------------------------------------------------------
static bool mt_shape_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && D <= MT_MAXDIM && H <= MT_MAXDIM && W <= MT_MAXDIM && (long long)D * H * W < 0x7fffffffLL;
}

extern "C" long long tc_metric_hist_bins(int D, int H, int W) {
    if (!mt_shape_ok(D, H, W)) return 0;
    return (long long)(D - 1) * (D - 1) + (long long)(H - 1) * (H - 1) + (long long)(W - 1) * (W - 1) + 1;
}

extern "C" int tc_metric_surfaces(const unsigned char* pred, const unsigned char* gt, unsigned char* surf_pred, unsigned char* surf_gt,
                                  long long* counts, int D, int H, int W, int ncls, int zfaces, void* stream) {
    if (!pred || !gt || !surf_pred || !surf_gt || !counts || !mt_shape_ok(D, H, W) || ncls <= 0 || ncls > MT_MAXCLS) return TC_ERR_ARG;
    hipLaunchKernelGGL(metric_surfaces_kernel, dim3(tc_blocks((long long)D * H * W, 256, 2048)), dim3(256), 0, (hipStream_t)stream,
                       pred, gt, surf_pred, surf_gt, (unsigned long long*)counts, D, H, W, ncls, zfaces ? 1 : 0);
    return tc_launch_status();
}

extern "C" int tc_metric_edt(const unsigned char* surf, int k, int* d2, int D, int H, int W, int zfaces, void* stream) {
    if (!surf || !d2 || !mt_shape_ok(D, H, W) || k <= 0 || k >= MT_MAXCLS) return TC_ERR_ARG;
    return mt_edt(surf, k, d2, D, H, W, zfaces, 1.0, 1.0, 1.0, (hipStream_t)stream);
}

extern "C" int tc_metric_hist(const unsigned char* surf_pred, const unsigned char* surf_gt, const int* d2_pred, const int* d2_gt, int k,
                              unsigned int* hist, long long nbins, int ncls, int D, int H, int W, void* stream) {
    if (!surf_pred || !surf_gt || !d2_pred || !d2_gt || !hist || !mt_shape_ok(D, H, W) || ncls <= 0 || ncls > MT_MAXCLS || k <= 0 || k >= ncls ||
        nbins < tc_metric_hist_bins(D, H, W))
        return TC_ERR_ARG;
    hipLaunchKernelGGL(metric_hist_kernel, dim3(tc_blocks((long long)D * H * W, 256, 2048)), dim3(256), 0, (hipStream_t)stream,
                       surf_pred, surf_gt, d2_pred, d2_gt, k, hist + (long long)k * nbins, nbins, D * H * W);
    return tc_launch_status();
}

extern "C" int tc_metric_select(const unsigned int* hist, long long nbins, int ncls, long long* out, void* stream) {
    if (!hist || !out || nbins <= 0 || ncls <= 0 || ncls > MT_MAXCLS) return TC_ERR_ARG;
    hipLaunchKernelGGL(metric_select_kernel, dim3(ncls), dim3(256), 0, (hipStream_t)stream, hist, nbins, out);
    return tc_launch_status();
}

static bool mt_spacing_ok(double v) { return v > 0.0 && v < __builtin_huge_val(); }       // finite and > 0 (false for a NaN)

extern "C" int tc_metric_edt_f64(const unsigned char* surf, int k, double* d2, int D, int H, int W, int zfaces, double sz, double sy, double sx,
                                 void* stream) {
    if (!surf || !d2 || !mt_shape_ok(D, H, W) || k <= 0 || k >= MT_MAXCLS || !mt_spacing_ok(sz) || !mt_spacing_ok(sy) || !mt_spacing_ok(sx))
        return TC_ERR_ARG;
    return mt_edt(surf, k, d2, D, H, W, zfaces, sz, sy, sx, (hipStream_t)stream);
}

extern "C" int tc_metric_select_f64(const unsigned char* surf_pred, const unsigned char* surf_gt, const double* d2_pred, const double* d2_gt, int k,
                                    int ncls, int D, int H, int W, void* work, long long* out, void* stream) {
    if (!surf_pred || !surf_gt || !d2_pred || !d2_gt || !work || !out || !mt_shape_ok(D, H, W) || ncls <= 0 || ncls > MT_MAXCLS || k <= 0 || k >= ncls)
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(work, 0, TC_METRIC_SELECT_WORK_BYTES, s) != hipSuccess) return TC_ERR_LAUNCH;
    const int n = D * H * W, blocks = tc_blocks(n, 256, 2048);
    for (int pass = 0; pass < MT_SEL_PASSES; ++pass) {
        hipLaunchKernelGGL(metric_select_count_kernel, dim3(blocks), dim3(256), 0, s, surf_pred, surf_gt, d2_pred, d2_gt, k, (unsigned int*)work, pass, n);
        hipLaunchKernelGGL(metric_select_scan_kernel, dim3(1), dim3(256), 0, s, (unsigned int*)work, pass, out + 3 * k);
        const int rc = tc_launch_status();
        if (rc != TC_OK) return rc;
    }
    return TC_OK;
}

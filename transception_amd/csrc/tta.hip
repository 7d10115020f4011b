// Test-time augmentation (include/transception_tta.h has the definition): the views of the input, and the softmax of a view's logits
// folded into an fp32 accumulator -- or, for the last view of a set, into the label -- at the un-transformed position.
//
// A view is three bits: rows reversed (1), columns reversed (2), then transpose (4).  Original position (p, q) is found in the view at
//   (fh(p), fw(q))          without the transpose,
//   (fw(q), fh(p))          with it (H == W),           fh(i) = H-1-i under bit 0, fw(i) = W-1-i under bit 1, else i.
//
// Every kernel is mapped on its OUTPUT: the accumulator (or label) for tta_accumulate_*, the view for tta_view_*.  One thread owns an
// output element in all its classes, so nothing is atomic, the views are added in launch order and a run repeats to the bit.
//   flip views       lanes walk a row of the output; the source row is the same piece forwards or backwards: coalesced both ways.
//                    Where W % 4 == 0 and the pointers are 16-byte aligned a lane owns 4 consecutive columns (16-byte fp32 / 8-byte 16-bit
//                    loads; the reversed piece [W-4-q, W-q) starts at a multiple of 4 too and is reversed in registers), and the
//                    accumulator moves in 16-byte pieces, every class loaded before the arithmetic starts.
//   transpose views  a 32 x 32 pixel tile of the output needs a 32 x 32 tile of the source with rows and columns exchanged.  The source tile
//                    is loaded with lanes along ITS rows (128-byte fp32 pieces), parked in LDS as fp32 [class][32][33] and read back with
//                    lanes along the output's rows: lane stride 33 words, 33 mod 32 = 1, so the 32 lanes of a ds_read_b32 group hit 32
//                    banks; the writes have lane stride 1.  Neither global side is strided by H.
//                    LDS: ncls * 32 * 33 * 4 bytes = 67,584 at ncls = 16 (two 256-thread workgroups per CU), 38,016 at ncls = 9 (four);
//                    the view kernel's tile is one plane, 4,224 bytes.
// Plain C++; the arithmetic of one pixel (tta_pixel) is the same function on every path.
#include "tc_common.h"
#include "../../include/transception_tta.h"

namespace {

constexpr int kMaxCls = 16;
constexpr int kTile = 32;                        // pixels per tile edge of the transposed paths
constexpr int kPitch = kTile + 1;                // LDS row pitch in words: the pad that spreads a tile column over the banks
constexpr int kMaxBlocks = 2048;                 // 256 CUs x 8 workgroups; larger maps take more trips of the grid-stride loops (tiles: twice as many)

__device__ __forceinline__ int tta_flip(int i, int n, bool on) { return on ? n - 1 - i : i; }

// One pixel, in registers.  l[0 .. ncls) are its logits in fp32; t[0 .. ncls) holds acc[n, ., p, q] on entry (anything when `first`) and
// t on exit: m = max l, e_k = expf(l_k - m), s = sum in class order, p_k = e_k / s; t_k = p_k (first) or acc_k + p_k.  Returns the first
// maximum of t.  The loops run to kMaxCls with k < ncls tested inside: fully unrolled, the arrays stay in registers (a run-time trip
// count would index scratch).
__device__ __forceinline__ int tta_pixel(const float (&l)[kMaxCls], float (&t)[kMaxCls], int ncls, bool first) {
    float m = l[0];
#pragma unroll
    for (int k = 1; k < kMaxCls; ++k)
        if (k < ncls) m = fmaxf(m, l[k]);
    float e[kMaxCls], s = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxCls; ++k)
        if (k < ncls) { e[k] = expf(l[k] - m); s += e[k]; }
    int best = 0;
    float tbest = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxCls; ++k)
        if (k < ncls) {
            const float pk = e[k] / s;
            t[k] = first ? pk : t[k] + pk;
            if (k == 0 || t[k] > tbest) { tbest = t[k]; best = k; }
        }
    return best;
}

// PX consecutive elements of a row, the first at p, as floats; PX = 4: p is aligned to 4 elements
template <typename T, int PX> __device__ __forceinline__ void tta_load(const T* p, float* o) {
    if constexpr (PX == 1) o[0] = ldf<T>(p);
    else { const float4 v = ld4<T>(p); o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
}

// Flip views (view < 4).  A thread owns PX consecutive columns of one accumulator row: `groups` = N * H * (W / PX) of them, grid-stride.
template <typename T, int PX, bool PRED> __global__ __launch_bounds__(256)
void tta_accumulate_flip_kernel(const T* __restrict__ logits, float* __restrict__ acc, unsigned char* __restrict__ pred, long long groups, int ncls,
                                int H, int W, int view, int first) {
    const int wg = W / PX;
    const long long plane = (long long)H * W;
    const bool rh = view & TC_TTA_FLIP_H, rw = view & TC_TTA_FLIP_W;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const int q0 = (int)(g % wg) * PX;
        const long long row = g / wg;                                             // n * H + p
        const int p = (int)(row % H);
        const long long n = row / H;
        // the source piece: columns fw(q0 + PX - 1) .. fw(q0) when reversed, which start at W - PX - q0
        const T* src = logits + n * ncls * plane + (long long)tta_flip(p, H, rh) * W + (rw ? W - PX - q0 : q0);
        const long long pix = row * W + q0 - n * plane;                           // p * W + q0
        float* a = acc + n * ncls * plane + pix;                                  // (not dereferenced where acc is NULL: first && PRED)
        // every load of the trip is issued before the arithmetic: the logits, and the accumulator's PX columns of every class as one piece
        float v[kMaxCls][PX], av[kMaxCls][PX];
#pragma unroll
        for (int k = 0; k < kMaxCls; ++k)
            if (k < ncls) {
                tta_load<T, PX>(src + k * plane, v[k]);
                if (!first) tta_load<float, PX>(a + k * plane, av[k]);
            }
        unsigned char lab[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            float l[kMaxCls], t[kMaxCls];
#pragma unroll
            for (int k = 0; k < kMaxCls; ++k) {
                l[k] = k < ncls ? v[k][rw ? PX - 1 - j : j] : 0.f;
                t[k] = k < ncls && !first ? av[k][j] : 0.f;
            }
            lab[j] = (unsigned char)tta_pixel(l, t, ncls, first);
#pragma unroll
            for (int k = 0; k < kMaxCls; ++k) av[k][j] = t[k];
        }
        if (PRED) {
            unsigned char* o = pred + n * plane + pix;
            if constexpr (PX == 4) *reinterpret_cast<uchar4*>(o) = make_uchar4(lab[0], lab[1], lab[2], lab[3]);
            else o[0] = lab[0];
        } else {
#pragma unroll
            for (int k = 0; k < kMaxCls; ++k)
                if (k < ncls) {
                    if constexpr (PX == 4) *reinterpret_cast<float4*>(a + k * plane) = make_float4(av[k][0], av[k][1], av[k][2], av[k][3]);
                    else a[k * plane] = av[k][0];
                }
        }
    }
}

// Transpose views (view >= 4, H == W == S).  A block owns 32 x 32 pixel tiles of the accumulator, `tiles` = N * ts * ts of them, block-stride
// (every thread of a block takes the same trips, so the barriers are uniform).  Thread t: lane column t % 32, rows t / 32 + 8 j.
//   load   tile[k][a][b] = logits[n, k, fw(q0 + a), fh(p0 + b)], lanes along b: the source row piece, forwards or backwards
//   use    pixel (p0 + pp, q0 + qq) reads tile[k][qq][pp], lanes along qq: word stride 33
template <typename T, bool PRED> __global__ __launch_bounds__(256)
void tta_accumulate_tr_kernel(const T* __restrict__ logits, float* __restrict__ acc, unsigned char* __restrict__ pred, long long tiles, int ts,
                              int ncls, int S, int view, int first) {
    extern __shared__ __align__(16) float tile[];                                 // [ncls][kTile][kPitch]
    const long long plane = (long long)S * S;
    const bool rh = view & TC_TTA_FLIP_H, rw = view & TC_TTA_FLIP_W;
    const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;                 // ly in 0..7
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int q0 = (int)(t % ts) * kTile, p0 = (int)((t / ts) % ts) * kTile;
        const long long n = t / ((long long)ts * ts);
        const T* src = logits + n * ncls * plane;
        if (p0 + lx < S) {
            const int x = tta_flip(p0 + lx, S, rh);
            for (int a = ly; a < kTile && q0 + a < S; a += 8) {
                const long long o = (long long)tta_flip(q0 + a, S, rw) * S + x;
#pragma unroll
                for (int k = 0; k < kMaxCls; ++k)
                    if (k < ncls) tile[(k * kTile + a) * kPitch + lx] = ldf<T>(src + k * plane + o);
            }
        }
        __syncthreads();
        if (q0 + lx < S) {
            for (int pp = ly; pp < kTile && p0 + pp < S; pp += 8) {
                const long long pix = (long long)(p0 + pp) * S + q0 + lx;
                float* a = acc + n * ncls * plane + pix;                          // (not dereferenced where acc is NULL: first && PRED)
                float l[kMaxCls], t[kMaxCls];
#pragma unroll
                for (int k = 0; k < kMaxCls; ++k) {
                    l[k] = k < ncls ? tile[(k * kTile + lx) * kPitch + pp] : 0.f;
                    t[k] = k < ncls && !first ? a[k * plane] : 0.f;
                }
                const int lab = tta_pixel(l, t, ncls, first);
                if (PRED) pred[n * plane + pix] = (unsigned char)lab;
                else {
#pragma unroll
                    for (int k = 0; k < kMaxCls; ++k)
                        if (k < ncls) a[k * plane] = t[k];
                }
            }
        }
        __syncthreads();                                                          // the tile is free before the next trip fills it
    }
}

// dst[n, y, x] = (src[n, fh(y), fw(x)] - mean) / stdv: a thread owns PX consecutive columns of a row of the view
template <int PX> __global__ __launch_bounds__(256)
void tta_view_flip_kernel(const float* __restrict__ src, float* __restrict__ dst, long long groups, int H, int W, int view, float mean, float stdv) {
    const int wg = W / PX;
    const bool rh = view & TC_TTA_FLIP_H, rw = view & TC_TTA_FLIP_W;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)gridDim.x * 256) {
        const int x0 = (int)(g % wg) * PX;
        const long long row = g / wg;
        const int y = (int)(row % H);
        const long long n = row / H;
        float v[PX];
        tta_load<float, PX>(src + (n * H + tta_flip(y, H, rh)) * W + (rw ? W - PX - x0 : x0), v);
        float o[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) o[j] = (v[rw ? PX - 1 - j : j] - mean) / stdv;
        float* d = dst + row * W + x0;
        if constexpr (PX == 4) *reinterpret_cast<float4*>(d) = make_float4(o[0], o[1], o[2], o[3]);
        else d[0] = o[0];
    }
}

// dst[n, y, x] = (src[n, fh(x), fw(y)] - mean) / stdv, H == W == S: the view tile (y0, x0) is the source tile with rows fh(x0 + .) and
// columns fw(y0 + .); loaded with lanes along the source's columns, read with lanes along the view's
__global__ __launch_bounds__(256)
void tta_view_tr_kernel(const float* __restrict__ src, float* __restrict__ dst, long long tiles, int ts, int S, int view, float mean, float stdv) {
    __shared__ float tile[kTile * kPitch];
    const long long plane = (long long)S * S;
    const bool rh = view & TC_TTA_FLIP_H, rw = view & TC_TTA_FLIP_W;
    const int lx = threadIdx.x % kTile, ly = threadIdx.x / kTile;
    for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int x0 = (int)(t % ts) * kTile, y0 = (int)((t / ts) % ts) * kTile;
        const long long n = t / ((long long)ts * ts);
        if (y0 + lx < S) {
            const int c = tta_flip(y0 + lx, S, rw);
            for (int a = ly; a < kTile && x0 + a < S; a += 8)
                tile[a * kPitch + lx] = src[n * plane + (long long)tta_flip(x0 + a, S, rh) * S + c];
        }
        __syncthreads();
        if (x0 + lx < S)
            for (int yy = ly; yy < kTile && y0 + yy < S; yy += 8)
                dst[n * plane + (long long)(y0 + yy) * S + x0 + lx] = (tile[lx * kPitch + yy] - mean) / stdv;
        __syncthreads();
    }
}

// a * b * c < 2^31 for positive ints, without overflow on the way
bool tta_below_2g(int a, int b, int c) {
    const long long ab = (long long)a * b;
    return ab <= 0x7fffffffLL && ab * c <= 0x7fffffffLL;
}

// false: the launch was not made (the LDS limit of the kernel could not be raised)
template <typename T, bool PRED>
bool tta_accumulate_launch(const T* logits, float* acc, unsigned char* pred, int N, int ncls, int H, int W, int view, int first, hipStream_t s) {
    if (view & TC_TTA_TRANSPOSE) {
        const int ts = (H + kTile - 1) / kTile;
        const long long tiles = (long long)N * ts * ts;
        const size_t smem = (size_t)ncls * kTile * kPitch * sizeof(float);
        if (smem > 64 * 1024 && hipFuncSetAttribute((const void*)tta_accumulate_tr_kernel<T, PRED>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                    (int)smem) != hipSuccess)
            return false;
        hipLaunchKernelGGL((tta_accumulate_tr_kernel<T, PRED>), dim3(tc_blocks(tiles, 1, 2 * kMaxBlocks)), dim3(256), smem, s, logits, acc, pred, tiles, ts,
                           ncls, H, view, first);
        return true;
    }
    // 4 columns a thread where every row piece is aligned: logits 4 elements of T, the accumulator 16 bytes, the labels 4
    const bool vec = W % 4 == 0 && (uintptr_t)logits % (4 * sizeof(T)) == 0 && (uintptr_t)acc % 16 == 0 && (uintptr_t)pred % 4 == 0;
    const long long groups = (long long)N * H * (vec ? W / 4 : W);
    const dim3 grid(tc_blocks(groups, 256, kMaxBlocks));
    if (vec)
        hipLaunchKernelGGL((tta_accumulate_flip_kernel<T, 4, PRED>), grid, dim3(256), 0, s, logits, acc, pred, groups, ncls, H, W, view, first);
    else
        hipLaunchKernelGGL((tta_accumulate_flip_kernel<T, 1, PRED>), grid, dim3(256), 0, s, logits, acc, pred, groups, ncls, H, W, view, first);
    return true;
}

}  // namespace

extern "C" int tc_tta_abi_version(void) { return TC_TTA_ABI_VERSION; }

extern "C" int tc_tta_view(const float* src, float* dst, int N, int H, int W, int view, float mean, float stdv, void* stream) {
    if (!src || !dst || src == dst || N <= 0 || H <= 0 || W <= 0 || view < 0 || view > 7 || ((view & TC_TTA_TRANSPOSE) && H != W) ||
        stdv == 0.f || !tta_below_2g(N, H, W))
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (view & TC_TTA_TRANSPOSE) {
        const int ts = (H + kTile - 1) / kTile;
        const long long tiles = (long long)N * ts * ts;
        hipLaunchKernelGGL(tta_view_tr_kernel, dim3(tc_blocks(tiles, 1, 2 * kMaxBlocks)), dim3(256), 0, s, src, dst, tiles, ts, H, view, mean, stdv);
    } else {
        const bool vec = W % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
        const long long groups = (long long)N * H * (vec ? W / 4 : W);
        const dim3 grid(tc_blocks(groups, 256, kMaxBlocks));
        if (vec) hipLaunchKernelGGL(tta_view_flip_kernel<4>, grid, dim3(256), 0, s, src, dst, groups, H, W, view, mean, stdv);
        else hipLaunchKernelGGL(tta_view_flip_kernel<1>, grid, dim3(256), 0, s, src, dst, groups, H, W, view, mean, stdv);
    }
    return tc_launch_status();
}

extern "C" int tc_tta_accumulate(const void* logits, int dtype, float* acc, unsigned char* pred, int N, int ncls, int H, int W, int view,
                                 int first, void* stream) {
    if (!logits || (first != 0 && first != 1) || (!acc && !(first && pred)) || (const void*)acc == logits || N <= 0 || H <= 0 || W <= 0 ||
        ncls < 1 || ncls > kMaxCls || view < 0 || view > 7 || ((view & TC_TTA_TRANSPOSE) && H != W) ||
        !tta_below_2g(N, ncls, H) || !tta_below_2g(N * ncls * H, W, 1))
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    bool launched = false;
    if (pred) TC_DISPATCH_DTYPE(dtype, launched = tta_accumulate_launch<T, true>((const T*)logits, acc, pred, N, ncls, H, W, view, first, s));
    else TC_DISPATCH_DTYPE(dtype, launched = tta_accumulate_launch<T, false>((const T*)logits, acc, nullptr, N, ncls, H, W, view, first, s));
    return launched ? tc_launch_status() : TC_ERR_LAUNCH;
}

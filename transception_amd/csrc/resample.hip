// Class scores resampled bilinearly (align_corners=False) to another size and their argmax, one pass (include/transception_resample.h has
// the definition).  The small score maps are read once; what leaves is the uint8 label at full resolution and, only where asked for, the
// fp32 scores.
//
// Mapped on the OUTPUT.  A 256-thread block owns a tile of 8 rows x 128 columns of one image, a thread 4 consecutive columns of one row in
// all classes: a wave is two rows of 32 threads, labels leave as one 4-byte store a thread (128 contiguous bytes a row), score rows as
// 16-byte stores (512 contiguous bytes a row and class).  The thread's row tap (y0, y1, ly) and four column taps (x0, x1, lx) are worked out
// once -- five integer divisions by a run-time 2H / 2W, five fp32 divisions -- and the class loop holds only the four lerps and the running
// best value and index of each column, in registers.  No atomics; an output element has one owner.
//
// Source.  The taps are monotone in the output coordinate, so the tile's source footprint is the rectangle from the first row's / column's
// lower tap to the last one's upper tap: at most (8-1) h/H + 3 rows and (128-1) w/W + 3 columns.  The block stages it in LDS as fp32
// [class][row][pitch] and every tap is a ds_read_b32.  Why LDS and not L1/L2: each source element is used by (H/h)(W/w) ~ 5 output pixels,
// and a thread's taps start at an arbitrary element, so reading them straight from memory means sixteen scalar loads a class and thread
// (2 rows x 4 columns x 2 taps), or 16-byte loads followed by a chain of selects to pick the taps out of registers (a run-time register index
// is scratch).  Staged, the global side is the footprint's rows in aligned 16-byte pieces, each element once a block, and the arbitrary
// offsets fall on the LDS, where lanes 0..31 of a row walk ~56 consecutive words at the workload's 7/16 ratio: about two lanes a bank.
//   MODE 0  staged, 16-byte source pieces: base 16-byte aligned and w a multiple of the piece (4 fp32 / 8 16-bit elements), so every row is;
//           the footprint's column range is widened to whole pieces.
//   MODE 1  staged, element-wise source loads: any base, any w.
//   MODE 2  unstaged, taps read from memory: a footprint that does not fit the LDS budget even one class at a time (strong shrinking).
// Where all classes of the footprint exceed the budget (32 KiB: four blocks a CU and more) they are staged in chunks of as many classes as
// fit, with the running best carried across chunks.  At 9 x 224^2 -> 512^2 one chunk holds 9 x 6 x 64 words = 13.5 KiB.
// Plain C++.
#include <algorithm>

#include "tc_common.h"
#include "../../include/transception_resample.h"

namespace {

constexpr int kMaxCls = 16;
constexpr int kThreads = 256;
constexpr int kPX = 4;                            // output columns a thread
constexpr int kTileH = 8, kTileW = 128;           // output tile of a block: 8 rows of 32 threads
constexpr int kLdsWords = 8192;                   // staging budget, fp32 words (32 KiB)

// lower tap and weight of output coordinate o: in = source extent, out2 = 2 * output extent
__device__ __forceinline__ void rs_tap(int o, int in, int out2, int& t0, float& l) {
    const int num = max((2 * o + 1) * in - (out2 >> 1), 0);
    t0 = num / out2;
    l = (float)(num - t0 * out2) / (float)out2;
}
__device__ __forceinline__ int rs_tap0(int o, int in, int out2) { return max((2 * o + 1) * in - (out2 >> 1), 0) / out2; }

template <typename T, int MODE> __global__ __launch_bounds__(kThreads)
void resample_kernel(const T* __restrict__ src, float* __restrict__ scores, unsigned char* __restrict__ pred, int ncls, int h, int w, int H, int W,
                     int tilesx, int tilesy, int kc, int pitch, int vout) {
    constexpr int P = MODE == 0 ? (int)(16 / sizeof(T)) : 1;                       // elements of a staged source piece
    extern __shared__ __align__(16) float lds[];                                  // [classes of a chunk][fr][pitch]
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tilesx, ty = (blockIdx.x / tilesx) % tilesy;
    const long long n = blockIdx.x / (tilesx * tilesy);
    const int X0 = tx * kTileW, Y0 = ty * kTileH;
    // the tile's source footprint: rows ya .. ya + fr - 1, columns xa .. xa + fc - 1 (whole pieces in MODE 0: w % P == 0)
    const int ya = rs_tap0(Y0, h, 2 * H), yb = min(rs_tap0(min(Y0 + kTileH, H) - 1, h, 2 * H) + 1, h - 1);
    const int xa = rs_tap0(X0, w, 2 * W) / P * P, xb = min(rs_tap0(min(X0 + kTileW, W) - 1, w, 2 * W) + 1, w - 1);
    const int fr = yb - ya + 1, fc = (xb - xa + P) / P * P;

    // this thread's outputs: row Y, columns X .. X + 3
    const int Y = Y0 + tid / (kTileW / kPX), X = X0 + tid % (kTileW / kPX) * kPX;
    const bool active = Y < H && X < W;
    int y0 = 0, x0[kPX], x1[kPX];
    float ly = 0.f, lx[kPX];
    rs_tap(min(Y, H - 1), h, 2 * H, y0, ly);
    const int y1 = min(y0 + 1, h - 1);
#pragma unroll
    for (int j = 0; j < kPX; ++j) {
        rs_tap(min(X + j, W - 1), w, 2 * W, x0[j], lx[j]);
        x1[j] = min(x0[j] + 1, w - 1);
    }
    const float my = 1.0f - ly;
    float best[kPX];
    int lab[kPX];
#pragma unroll
    for (int j = 0; j < kPX; ++j) { best[j] = 0.f; lab[j] = 0; }
    const long long plane = (long long)H * W, splane = (long long)h * w;
    const T* img = src + n * ncls * splane;
    float* so = scores ? scores + n * ncls * plane + (long long)Y * W + X : nullptr;

    for (int k0 = 0; k0 < ncls; k0 += kc) {
        const int nk = min(kc, ncls - k0);
        if constexpr (MODE != 2) {
            if (k0) __syncthreads();                                              // the last chunk's taps are read before it is overwritten
            const int pieces = fc / P;
            for (int R = tid >> 5; R < nk * fr; R += kThreads >> 5) {             // LDS row R = (class of the chunk) * fr + (row of the footprint)
                const int k = R / fr, rr = R - k * fr;
                const T* g = img + (k0 + k) * splane + (long long)(ya + rr) * w + xa;
                float* l = lds + R * pitch;
                for (int pc = tid & 31; pc < pieces; pc += 32) {
                    if constexpr (MODE == 0) {
                        float v[P];
                        tc_unpack16<T>(*reinterpret_cast<const uint4*>(g + pc * P), v);
#pragma unroll
                        for (int i = 0; i < P; i += 4) *reinterpret_cast<float4*>(l + pc * P + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
                    } else l[pc] = ldf<T>(g + pc);
                }
            }
            __syncthreads();
        }
        if (active) {
            for (int k = 0; k < nk; ++k) {
                float v[kPX];
                if constexpr (MODE != 2) {
                    const int b0 = (k * fr + y0 - ya) * pitch - xa, b1 = (k * fr + y1 - ya) * pitch - xa;
#pragma unroll
                    for (int j = 0; j < kPX; ++j) {
                        const float mx = 1.0f - lx[j];
                        v[j] = my * (mx * lds[b0 + x0[j]] + lx[j] * lds[b0 + x1[j]]) + ly * (mx * lds[b1 + x0[j]] + lx[j] * lds[b1 + x1[j]]);
                    }
                } else {
                    const T* r0 = img + (k0 + k) * splane + (long long)y0 * w;
                    const T* r1 = img + (k0 + k) * splane + (long long)y1 * w;
#pragma unroll
                    for (int j = 0; j < kPX; ++j) {
                        const float mx = 1.0f - lx[j];
                        v[j] = my * (mx * ldf<T>(r0 + x0[j]) + lx[j] * ldf<T>(r0 + x1[j])) + ly * (mx * ldf<T>(r1 + x0[j]) + lx[j] * ldf<T>(r1 + x1[j]));
                    }
                }
#pragma unroll
                for (int j = 0; j < kPX; ++j)
                    if (k0 + k == 0 || v[j] > best[j]) { best[j] = v[j]; lab[j] = k0 + k; }
                if (so) {
                    float* o = so + (k0 + k) * plane;
                    if (vout) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                    else {
#pragma unroll
                        for (int j = 0; j < kPX; ++j)
                            if (X + j < W) o[j] = v[j];
                    }
                }
            }
        }
    }
    if (active && pred) {
        unsigned char* o = pred + n * plane + (long long)Y * W + X;
        if (vout) *reinterpret_cast<uchar4*>(o) = make_uchar4(lab[0], lab[1], lab[2], lab[3]);
        else {
#pragma unroll
            for (int j = 0; j < kPX; ++j)
                if (X + j < W) o[j] = (unsigned char)lab[j];
        }
    }
}

// a * b * c < 2^31 for positive ints, without overflow on the way
bool rs_below_2g(long long a, int b, int c) {
    const long long ab = a * b;
    return ab <= 0x7fffffffLL && ab * c <= 0x7fffffffLL;
}

template <typename T>
void resample_launch(const T* src, float* scores, unsigned char* pred, int N, int ncls, int h, int w, int H, int W, hipStream_t s) {
    constexpr int P = 16 / sizeof(T);
    const bool vec = (uintptr_t)src % 16 == 0 && w % P == 0;
    // the bound of the footprint: the lower taps of a tile's first and last coordinate are at most floor((tile - 1) in / out) + 1 apart, the upper
    // tap adds one, whole pieces up to P - 1 in front (the end is rounded up inside the row: w % P == 0)
    const int fr = (int)std::min((long long)h, (long long)(kTileH - 1) * h / H + 3);
    const int p = vec ? P : 1;
    const int pitch = (int)(std::min((long long)w, (long long)(kTileW - 1) * w / W + 3 + (p - 1)) + p - 1) / p * p;
    const long long words = (long long)fr * pitch;
    const int tilesx = (W + kTileW - 1) / kTileW, tilesy = (H + kTileH - 1) / kTileH;
    const dim3 grid((unsigned)((long long)N * tilesx * tilesy));                  // < 2^31: N H W is
    // 4-column stores where every thread's piece is whole and aligned: the labels 4 bytes, the scores 16
    const int vout = W % kPX == 0 && (uintptr_t)pred % 4 == 0 && (uintptr_t)scores % 16 == 0;
    if (words > kLdsWords)
        hipLaunchKernelGGL((resample_kernel<T, 2>), grid, dim3(kThreads), 0, s, src, scores, pred, ncls, h, w, H, W, tilesx, tilesy, ncls, 0, vout);
    else {
        const int kc = (int)std::min((long long)ncls, kLdsWords / words);
        const size_t smem = (size_t)kc * words * sizeof(float);
        if (vec) hipLaunchKernelGGL((resample_kernel<T, 0>), grid, dim3(kThreads), smem, s, src, scores, pred, ncls, h, w, H, W, tilesx, tilesy, kc, pitch, vout);
        else hipLaunchKernelGGL((resample_kernel<T, 1>), grid, dim3(kThreads), smem, s, src, scores, pred, ncls, h, w, H, W, tilesx, tilesy, kc, pitch, vout);
    }
}

}  // namespace

extern "C" int tc_resample_abi_version(void) { return TC_RESAMPLE_ABI_VERSION; }

extern "C" int tc_resample_scores(const void* src, int dtype, float* scores, unsigned char* pred, int N, int ncls, int h, int w, int H, int W,
                                  void* stream) {
    const int E = TC_RESAMPLE_MAX_EXTENT;
    if (!src || (!scores && !pred) || (const void*)scores == src || (const void*)pred == src || ncls < 1 || ncls > kMaxCls || N <= 0 ||
        h <= 0 || w <= 0 || H <= 0 || W <= 0 || h > E || w > E || H > E || W > E || (dtype != TC_F32 && dtype != TC_BF16 && dtype != TC_F16) ||
        !rs_below_2g((long long)N * ncls, h, w) || !rs_below_2g(N, H, W) || (scores && !rs_below_2g((long long)N * ncls, H, W)))
        return TC_ERR_ARG;
    TC_DISPATCH_DTYPE(dtype, resample_launch<T>((const T*)src, scores, pred, N, ncls, h, w, H, W, (hipStream_t)stream));
    return tc_launch_status();
}

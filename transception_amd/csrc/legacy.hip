// Gather kernels of the legacy Transception encoder (networks/Transception.py, MiT_3inception: stages 2-4 with two patch-embedding
// branches).  Every thread moves one 16-byte channel piece (4 fp32 or 8 16-bit elements); the forward gathers copy bits, the adjoints
// gather (no atomics: each output element is written by one thread, its sum taken in a fixed order in fp32).
#include "tc_common.h"

namespace {

#define TC_GRID_STRIDE(i, n) for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)(n); i += gridDim.x * blockDim.x)

template <typename T> __device__ __forceinline__ void ld_piece(const T* p, float* v) { tc_unpack16<T>(*reinterpret_cast<const uint4*>(p), v); }
template <typename T> __device__ __forceinline__ void st_piece(T* p, const float* v) { *reinterpret_cast<uint4*>(p) = tc_pack16<T>(v); }

// im2col of a k x k convolution (stride s, padding p, dilation d) over a token-major map x [B*H*W, Cin] (row stride ldx):
// cols[(b, oy, ox), (ky*k + kx)*Cin + c] = x(b, oy*s - p + ky*d, ox*s - p + kx*d, c), zero outside the map.  Tap-major columns keep
// the channels of a tap contiguous; the weight is handed to the GEMM as [Cout, k*k*Cin] (engine.Graph.permuted_weight).
template <typename T>
__global__ void im2col_dil_kernel(const T* __restrict__ x, int ldx, T* __restrict__ cols, int ldc, int B, int Cin, int H, int W, int Ho, int Wo,
                                  int k, int s, int p, int d) {
    constexpr int V = TcVec16<T>::N;
    const int cp = Cin / V, taps = k * k;
    const long long n = (long long)B * Ho * Wo * taps * cp;
    TC_GRID_STRIDE(i, n) {
        const int q = (int)(i % cp); unsigned t = i / cp;
        const int tap = (int)(t % taps); t /= taps;
        const int ox = (int)(t % Wo); t /= Wo; const int oy = (int)(t % Ho); const int b = (int)(t / Ho);
        const int ky = tap / k, kx = tap - ky * k;
        const int iy = oy * s - p + ky * d, ix = ox * s - p + kx * d;
        T* dst = cols + (long long)((b * Ho + oy) * Wo + ox) * ldc + tap * Cin + q * V;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W)
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(x + (long long)((b * H + iy) * W + ix) * ldx + q * V);
        else
            *reinterpret_cast<uint4*>(dst) = make_uint4(0u, 0u, 0u, 0u);
    }
}

// dx(b, y, x, c) (+)= the sum, over the taps (ky, kx) in order, of the column gradient of the output pixel that read (b, y, x) through that tap
template <typename T>
__global__ void col2im_dil_kernel(const T* __restrict__ dcols, int ldc, T* __restrict__ dx, int lddx, int B, int Cin, int H, int W, int Ho, int Wo,
                                  int k, int s, int p, int d, int accumulate) {
    constexpr int V = TcVec16<T>::N;
    const int cp = Cin / V;
    const long long n = (long long)B * H * W * cp;
    TC_GRID_STRIDE(i, n) {
        const int q = (int)(i % cp); unsigned t = i / cp;
        const int x_ = (int)(t % W); t /= W; const int y = (int)(t % H); const int b = (int)(t / H);
        float a[V], v[V];
#pragma unroll
        for (int e = 0; e < V; ++e) a[e] = 0.f;
        for (int ky = 0; ky < k; ++ky) {
            const int sy = y + p - ky * d;                       // = oy * s
            if (sy < 0 || sy % s) continue;
            const int oy = sy / s;
            if (oy >= Ho) continue;
            for (int kx = 0; kx < k; ++kx) {
                const int sx = x_ + p - kx * d;
                if (sx < 0 || sx % s) continue;
                const int ox = sx / s;
                if (ox >= Wo) continue;
                ld_piece<T>(dcols + (long long)((b * Ho + oy) * Wo + ox) * ldc + (ky * k + kx) * Cin + q * V, v);
#pragma unroll
                for (int e = 0; e < V; ++e) a[e] += v[e];
            }
        }
        T* dst = dx + (long long)((b * H + y) * W + x_) * lddx + q * V;
        if (accumulate) {
            ld_piece<T>(dst, v);
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] += v[e];
        }
        st_piece<T>(dst, a);
    }
}

// PyTorch's nearest rule (F.interpolate, mode "nearest", no scale factor): src = min((int)floorf(dst * (float)in / out), in - 1)
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) { return min((int)floorf((float)dst * scale), in - 1); }

// y[(b, oy, ox), 0:C) = branch-1 token (nearest(oy), nearest(ox)) of image b; y[(b, oy, ox), C:2C) = branch-2 token (oy, ox)
template <typename T>
__global__ void nearest_concat_fwd_kernel(const T* __restrict__ x1, long long sb1, const T* __restrict__ x2, long long sb2, int ldx,
                                          T* __restrict__ y, int ldy, int B, int H1, int W1, int Ho, int Wo, int C, float sy, float sx) {
    constexpr int V = TcVec16<T>::N;
    const int cp = C / V, cp2 = 2 * cp;
    const long long n = (long long)B * Ho * Wo * cp2;
    TC_GRID_STRIDE(i, n) {
        const int q = (int)(i % cp2); unsigned t = i / cp2;
        const int ox = (int)(t % Wo); t /= Wo; const int oy = (int)(t % Ho); const int b = (int)(t / Ho);
        const T* src = q < cp ? x1 + b * sb1 + (long long)(nearest_src(oy, sy, H1) * W1 + nearest_src(ox, sx, W1)) * ldx + q * V
                              : x2 + b * sb2 + (long long)(oy * Wo + ox) * ldx + (q - cp) * V;
        *reinterpret_cast<uint4*>(y + (long long)((b * Ho + oy) * Wo + ox) * ldy + q * V) = *reinterpret_cast<const uint4*>(src);
    }
}

// dx1(b, iy, ix) (+)= sum of dy[(b, oy, ox), 0:C) over the output pixels whose nearest source is (iy, ix), row-major order;
// dx2(b, oy, ox) (+)= dy[(b, oy, ox), C:2C)
template <typename T>
__global__ void nearest_concat_bwd_kernel(const T* __restrict__ dy, int ldy, T* __restrict__ dx1, long long sb1, T* __restrict__ dx2, long long sb2,
                                          int lddx, int B, int H1, int W1, int Ho, int Wo, int C, float sy, float sx, int accumulate) {
    constexpr int V = TcVec16<T>::N;
    const int cp = C / V, n1 = H1 * W1, nt = n1 + Ho * Wo;
    const long long n = (long long)B * nt * cp;
    TC_GRID_STRIDE(i, n) {
        const int q = (int)(i % cp); unsigned t = i / cp;
        const int tok = (int)(t % nt); const int b = (int)(t / nt);
        float a[V], v[V];
        T* dst;
        if (tok < n1) {
            const int iy = tok / W1, ix = tok - iy * W1;
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] = 0.f;
            // the outputs that pick iy lie in [floor(iy / scale) - 1, ceil((iy + 1) / scale) + 1): test each with the forward's rule
            const int y0 = max(0, (int)floorf((float)iy / sy) - 1), y1 = min(Ho, (int)ceilf((float)(iy + 1) / sy) + 1);
            const int x0 = max(0, (int)floorf((float)ix / sx) - 1), x1 = min(Wo, (int)ceilf((float)(ix + 1) / sx) + 1);
            for (int oy = y0; oy < y1; ++oy) {
                if (nearest_src(oy, sy, H1) != iy) continue;
                for (int ox = x0; ox < x1; ++ox) {
                    if (nearest_src(ox, sx, W1) != ix) continue;
                    ld_piece<T>(dy + (long long)((b * Ho + oy) * Wo + ox) * ldy + q * V, v);
#pragma unroll
                    for (int e = 0; e < V; ++e) a[e] += v[e];
                }
            }
            dst = dx1 + b * sb1 + (long long)tok * lddx + q * V;
        } else {
            ld_piece<T>(dy + (long long)(b * Ho * Wo + tok - n1) * ldy + C + q * V, a);
            dst = dx2 + b * sb2 + (long long)(tok - n1) * lddx + q * V;
        }
        if (accumulate) {
            ld_piece<T>(dst, v);
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] += v[e];
        }
        st_piece<T>(dst, a);
    }
}

inline dim3 g1(long long n) { return n < 0x7fffffffLL ? dim3(tc_blocks(n, 256, 8192)) : dim3(0); }     // (an empty grid is a launch error: reported)
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define TC_S ((hipStream_t)stream)

static bool dil_geometry(int H, int W, int k, int s, int p, int d, int& Ho, int& Wo) {
    if ((k != 1 && k != 3) || s <= 0 || p < 0 || d <= 0) return false;
    Ho = (H + 2 * p - d * (k - 1) - 1) / s + 1;
    Wo = (W + 2 * p - d * (k - 1) - 1) / s + 1;
    return H + 2 * p - d * (k - 1) - 1 >= 0 && W + 2 * p - d * (k - 1) - 1 >= 0;
}

extern "C" int tc_im2col_dil(const void* x, int ldx, void* cols, int ldc, int B, int Cin, int H, int W, int k, int stride, int pad, int dil,
                             int dtype, void* stream) {
    int Ho, Wo;
    if (!x || !cols || B <= 0 || Cin <= 0 || (Cin & 7) || H <= 0 || W <= 0 || !dil_geometry(H, W, k, stride, pad, dil, Ho, Wo) || ldx < Cin
        || (ldx & 7) || ldc < k * k * Cin || (ldc & 7) || !al16(x) || !al16(cols))
        return TC_ERR_ARG;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((im2col_dil_kernel<T>), g1((long long)B * Ho * Wo * k * k * (Cin / TcVec16<T>::N)), dim3(256), 0, TC_S,
                                                (const T*)x, ldx, (T*)cols, ldc, B, Cin, H, W, Ho, Wo, k, stride, pad, dil));
    return tc_launch_status();
}

extern "C" int tc_col2im_dil(const void* dcols, int ldc, void* dx, int lddx, int B, int Cin, int H, int W, int k, int stride, int pad, int dil,
                             int accumulate, int dtype, void* stream) {
    int Ho, Wo;
    if (!dcols || !dx || B <= 0 || Cin <= 0 || (Cin & 7) || H <= 0 || W <= 0 || !dil_geometry(H, W, k, stride, pad, dil, Ho, Wo) || lddx < Cin
        || (lddx & 7) || ldc < k * k * Cin || (ldc & 7) || !al16(dcols) || !al16(dx))
        return TC_ERR_ARG;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((col2im_dil_kernel<T>), g1((long long)B * H * W * (Cin / TcVec16<T>::N)), dim3(256), 0, TC_S,
                                                (const T*)dcols, ldc, (T*)dx, lddx, B, Cin, H, W, Ho, Wo, k, stride, pad, dil, accumulate));
    return tc_launch_status();
}

extern "C" int tc_nearest_concat_fwd(const void* x1, long long sb1, const void* x2, long long sb2, int ldx, void* y, int ldy, int B, int H1, int W1,
                                     int Ho, int Wo, int C, int dtype, void* stream) {
    if (!x1 || !x2 || !y || B <= 0 || H1 <= 0 || W1 <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || (C & 7) || ldx < C || (ldx & 7) || ldy < 2 * C
        || (ldy & 7) || (sb1 & 7) || (sb2 & 7) || !al16(x1) || !al16(x2) || !al16(y))
        return TC_ERR_ARG;
    const float sy = (float)H1 / (float)Ho, sx = (float)W1 / (float)Wo;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((nearest_concat_fwd_kernel<T>), g1((long long)B * Ho * Wo * 2 * (C / TcVec16<T>::N)), dim3(256), 0, TC_S,
                                                (const T*)x1, sb1, (const T*)x2, sb2, ldx, (T*)y, ldy, B, H1, W1, Ho, Wo, C, sy, sx));
    return tc_launch_status();
}

extern "C" int tc_nearest_concat_bwd(const void* dy, int ldy, void* dx1, long long sb1, void* dx2, long long sb2, int lddx, int B, int H1, int W1,
                                     int Ho, int Wo, int C, int accumulate, int dtype, void* stream) {
    if (!dy || !dx1 || !dx2 || B <= 0 || H1 <= 0 || W1 <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || (C & 7) || lddx < C || (lddx & 7) || ldy < 2 * C
        || (ldy & 7) || (sb1 & 7) || (sb2 & 7) || !al16(dy) || !al16(dx1) || !al16(dx2))
        return TC_ERR_ARG;
    const float sy = (float)H1 / (float)Ho, sx = (float)W1 / (float)Wo;
    TC_DISPATCH_DTYPE(dtype, hipLaunchKernelGGL((nearest_concat_bwd_kernel<T>), g1((long long)B * (H1 * W1 + Ho * Wo) * (C / TcVec16<T>::N)), dim3(256),
                                                0, TC_S, (const T*)dy, ldy, (T*)dx1, sb1, (T*)dx2, sb2, lddx, B, H1, W1, Ho, Wo, C, sy, sx, accumulate));
    return tc_launch_status();
}

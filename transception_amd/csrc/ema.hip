// Exponential moving average of the weights on the flat fp32 arenas (include/transception_ema.h has the definition): the shadow arena
// follows the parameter arena inside the captured step, after the optimiser's update kernel, under the same skip.
//
// The pattern is the fused AdamW's (train.hip): a four-word state in device memory, a one-thread advance launch that leaves the state
// alone on a skipped step, one streaming launch over the segment table.  A captured kernel's scalar arguments are frozen at capture, so
// the count and the decay derived from it live in the state and are read from there.
// Plain C++ with 16-byte loads and stores; no atomics, no LDS, no communication between threads.
#include "tc_common.h"
#include "../../include/transception_ema.h"

namespace {

// One thread: ordinary loads and stores.  d in double, each float word rounded once.  A non-finite *sumsq leaves all four words alone:
// ema_multi_kernel and the optimiser's update kernel skip the same step.
__global__ void ema_advance_kernel(float* __restrict__ state, const float* __restrict__ sumsq, double decay, int warmup) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (sumsq && !(*sumsq < __builtin_inff())) return;
    int* istate = reinterpret_cast<int*>(state);
    const int n = istate[0] + 1;
    double d = decay;
    if (n == 1) d = 0.0;                                          // the first update copies (AveragedModel)
    else if (warmup) d = fmin(decay, (1.0 + (double)n) / (10.0 + (double)n));
    istate[0] = n;
    state[1] = (float)d;
    state[2] = (float)(1.0 - d);
    istate[3] = 0;
}

// torch's lerp_(w, omd) on one element: e + omd (w - e)
__device__ __forceinline__ float ema_elem(float e, float w, float omd) { return e + omd * (w - e); }

// The segment table, the skip, the alignment test and the two element paths are adam_multi_kernel's: blockIdx.y = segment,
// segs[2 i] = offset, segs[2 i + 1] = length.  12 bytes per live weight: w read, e read and written (8 on a copying update: e is not read).
__global__ __launch_bounds__(256) void ema_multi_kernel(float* __restrict__ ema, const float* __restrict__ p, const long long* __restrict__ segs,
                                                        const float* __restrict__ ema_state, const float* __restrict__ sumsq) {
    if (sumsq && !(*sumsq < __builtin_inff())) return;           // skipped: the shadow stays; ema_advance_kernel did not count it
    const float omd = ema_state[2];
    const bool copy = omd == 1.0f;                                // d = 0: the value itself, e + (w - e) need not equal w
    const long long off = segs[2 * blockIdx.y], n = segs[2 * blockIdx.y + 1];
    if (!((off | n) & 3) && !(((uintptr_t)ema | (uintptr_t)p) & 15)) {
        const long long n4 = n >> 2;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
            const long long j = off + 4 * i;
            float4 w = *reinterpret_cast<const float4*>(p + j);
            if (!copy) {
                const float4 e = *reinterpret_cast<const float4*>(ema + j);
                w = make_float4(ema_elem(e.x, w.x, omd), ema_elem(e.y, w.y, omd), ema_elem(e.z, w.z, omd), ema_elem(e.w, w.w, omd));
            }
            *reinterpret_cast<float4*>(ema + j) = w;
        }
        return;
    }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long j = off + i;
        const float w = p[j];
        ema[j] = copy ? w : ema_elem(ema[j], w, omd);
    }
}

// Both buffers in 16-byte pieces, each piece read and written by one thread: a and b are disjoint, so nothing is read after it was written.
__global__ __launch_bounds__(256) void swap_f32_kernel(uint4* __restrict__ a, uint4* __restrict__ b, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const uint4 va = a[i], vb = b[i];
        a[i] = vb;
        b[i] = va;
    }
}

}  // namespace

extern "C" int tc_ema_abi_version(void) { return TC_EMA_ABI_VERSION; }

extern "C" int tc_ema_advance(float* state, const float* sumsq, double decay, int warmup, void* stream) {
    if (!state || !(decay >= 0.0) || !(decay < 1.0)) return TC_ERR_ARG;                  // (a NaN fails both comparisons)
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, sumsq, decay, warmup ? 1 : 0);
    return tc_launch_status();
}

extern "C" int tc_ema_update_multi(float* ema, const float* p, const long long* segs_dev, int nseg, long long max_len, const float* ema_state,
                                   const float* sumsq, void* stream) {
    if (!ema || !p || !segs_dev || !ema_state || nseg <= 0 || nseg > 65535 || max_len <= 0) return TC_ERR_ARG;
    // one decay class: the table holds a few long segments, so the x extent carries the parallelism (a block past its segment's end returns)
    hipLaunchKernelGGL(ema_multi_kernel, dim3(tc_blocks(max_len, 256 * 8, 1024), nseg), dim3(256), 0, (hipStream_t)stream, ema, p, segs_dev,
                       ema_state, sumsq);
    return tc_launch_status();
}

extern "C" int tc_swap_f32(float* a, float* b, long long n, void* stream) {
    if (!a || !b || a == b || n <= 0 || (n & 3) || (uintptr_t)a % 16 || (uintptr_t)b % 16) return TC_ERR_ARG;
    hipLaunchKernelGGL(swap_f32_kernel, dim3(tc_blocks(n / 4, 256 * 4, 2048)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<uint4*>(a),
                       reinterpret_cast<uint4*>(b), n / 4);
    return tc_launch_status();
}

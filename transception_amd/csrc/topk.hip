// The select of the top-k (hard-pixel) cross-entropy (include/transception_topk.h): the k-th largest entry of a per-pixel value map, the
// counts around it and the sum above it, on the device and the same bit for bit from run to run.
//
// A most-significant-digit radix select over the uint32 patterns, as metric_select_count_kernel / metric_select_scan_kernel (metrics.hip) do
// it for doubles: non-negative floats order like their bits, so the k-th largest value is found digit by digit from integer histograms, four
// passes of 8 bits.  Entries with the sign bit set (an ignored pixel's -1.0f) are not counted.  Integer atomics only; the fp64 sum S goes
// through one scratch slot per workgroup and a fixed-order add, as in surface.hip.  Every step is a launch of its own: no grid barrier, no
// ticket, no loop that runs until something converges.
#include "tc_common.h"
#include "../../include/transception_topk.h"

namespace {

constexpr int TK_PASSES = 4;
constexpr int TK_MAX_BLOCKS = 1024;                     // the grid cap of the loss forward (the sum pass): one fp64 slot each
// The count passes end in one global atomic per workgroup and used bin, and atomics on one address serialise: at 1024 workgroups they were
// the larger part of a pass (16 x 9 x 224 x 224, a pass whose digits spread over all 256 bins: 22 us).  So those passes run on 256
// workgroups, one per compute unit, and each thread keeps four loads in flight instead.
constexpr int TK_COUNT_BLOCKS = 256;
constexpr int TK_UNROLL = 4;
struct TkSel {
    unsigned int hist[TK_PASSES][256];                  // [pass][digit]
    unsigned long long n, k, rank, n_eq;                // rank: the wanted position (1 = largest) among the values that share `prefix`
    unsigned int prefix, pad;                           // the digits fixed so far
    double part[TK_MAX_BLOCKS];                         // S, per workgroup
};

__global__ __launch_bounds__(256) void topk_clear_kernel(TkSel* __restrict__ w) {
    unsigned int* p = reinterpret_cast<unsigned int*>(w);
    for (int i = threadIdx.x; i < (int)(offsetof(TkSel, part) / 4); i += 256) p[i] = 0u;
}

// One pass: of the counted values whose leading 8 * pass bits equal the prefix, the next 8-bit digit is counted.  Loss values crowd into a
// few exponent bins, and lanes of one wave that hit the same LDS word serialise: four rounds peel a digit each -- the first remaining lane's
// digit, counted for all lanes that share it by ONE atomic of the popcount -- and only what is left after them goes lane by lane.
__global__ __launch_bounds__(256) void topk_count_kernel(const float* __restrict__ values, long long n, TkSel* __restrict__ w, int pass) {
    __shared__ unsigned int lh[256];
    lh[threadIdx.x] = 0;
    const unsigned int prefix = pass ? w->prefix : 0u;
    const int shift = 24 - 8 * pass;
    const int lane = threadIdx.x & 63;
    __syncthreads();
    // (the trip count is uniform per workgroup: the ballots see whole waves.  Four loads in flight per thread: the grid is small, see the entry)
    for (long long base = (long long)blockIdx.x * (256 * TK_UNROLL); base < n; base += (long long)gridDim.x * (256 * TK_UNROLL)) {
        unsigned int bits[TK_UNROLL];
#pragma unroll
        for (int j = 0; j < TK_UNROLL; ++j) {
            const long long i = base + j * 256 + threadIdx.x;
            bits[j] = i < n ? __float_as_uint(values[i]) : 0x80000000u;
        }
#pragma unroll
        for (int j = 0; j < TK_UNROLL; ++j) {
            const unsigned int b = bits[j];
            bool todo = !(b >> 31) && (pass == 0 || (b >> (shift + 8)) == prefix);
            const int digit = (int)(b >> shift) & 255;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const unsigned long long act = __ballot(todo);
                const int leader = (__ffsll((long long)act) - 1) & 63;
                const int d = __shfl(digit, leader, 64);
                const bool mine = todo && digit == d;
                const unsigned long long grp = __ballot(mine);
                if (mine && lane == leader) atomicAdd(&lh[d], (unsigned int)__popcll(grp));
                todo = todo && !mine;
            }
            if (todo) atomicAdd(&lh[digit], 1u);
        }
    }
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&w->hist[pass][threadIdx.x], lh[threadIdx.x]);
}

// One workgroup.  Thread t owns digit 255 - t, so an inclusive scan over t counts the values at or above a digit; the thread whose bin
// holds the wanted position appends its digit to the prefix and keeps the position inside the bin.  Pass 0 also fixes n and k.
__global__ __launch_bounds__(256) void topk_scan_kernel(TkSel* __restrict__ w, const double* __restrict__ state, int pass) {
    __shared__ unsigned long long inc[256];
    const int t = threadIdx.x, digit = 255 - t;
    const unsigned long long h = w->hist[pass][digit];
    unsigned long long n = pass ? w->n : 0, rank = pass ? w->rank : 0;
    const unsigned int prefix = pass ? w->prefix : 0u;
    inc[t] = h;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned long long a = t >= off ? inc[t - off] : 0;
        __syncthreads();
        inc[t] += a;
        __syncthreads();
    }
    if (pass == 0) {
        n = inc[255];
        // k = max(1, min(n, ceil(frac n))), the product once in fp64; the comparisons send a NaN and anything below 1 to 1
        const double kd = ceil(state[0] * (double)n);
        unsigned long long k = 1;
        if (kd >= (double)n) k = n;
        else if (kd >= 1.0) k = (unsigned long long)kd;
        rank = k;
        if (t == 0) { w->n = n; w->k = n ? k : 0; }
    }
    if (n == 0) return;                                                               // (uniform) nothing counted: prefix and rank stay 0
    const unsigned long long before = inc[t] - h;
    if (h && before < rank && rank <= inc[t]) {                                       // exactly one thread: 1 <= rank <= the bins' total
        w->prefix = (prefix << 8) | (unsigned int)digit;
        w->rank = rank - before;
        if (pass == TK_PASSES - 1) w->n_eq = h;
    }
}

// S = sum of the values above the threshold, in double: per thread, then a fixed tree over the workgroup, one slot per workgroup
__global__ __launch_bounds__(256) void topk_sum_kernel(const float* __restrict__ values, long long n, TkSel* __restrict__ w) {
    __shared__ double red[256];
    const unsigned int tb = w->prefix;
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = values[i];
        const unsigned int b = __float_as_uint(v);
        if (!(b >> 31) && b > tb) s += (double)v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) w->part[blockIdx.x] = red[0];
}

// One workgroup: the slots in a fixed order, then the state and the rank's share of the cross-entropy
__global__ __launch_bounds__(256) void topk_final_kernel(const TkSel* __restrict__ w, int nblk, double* __restrict__ state,
                                                         float* __restrict__ sums, double inv_world) {
    __shared__ double red[256];
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += w->part[b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const unsigned long long n = w->n, k = w->k;
    if (n == 0) {
        for (int j = 1; j < 8; ++j) state[j] = 0.0;
        sums[0] = 0.f;
        return;
    }
    const unsigned long long n_gt = k - w->rank, n_eq = w->n_eq;
    const double t = (double)__uint_as_float(w->prefix), S = red[0], left = (double)(k - n_gt);
    state[1] = (double)n; state[2] = (double)k; state[3] = (double)n_gt; state[4] = (double)n_eq;
    state[5] = t; state[6] = S; state[7] = left / (double)n_eq;
    sums[0] = (float)((S + left * t) / (double)k * inv_world);
}

}  // namespace

extern "C" int tc_topk_abi_version(void) { return TC_TOPK_ABI_VERSION; }
extern "C" long long tc_topk_work_bytes(void) { return (long long)sizeof(TkSel); }

extern "C" int tc_topk_select(const float* values, long long n_pix, double* state, float* sums, double inv_world, void* work, void* stream) {
    if (!values || !state || !sums || !work || n_pix <= 0 || n_pix >= 0x7fffffffLL || ((uintptr_t)work & 7) || ((uintptr_t)state & 7) ||
        !(inv_world > 0.0 && inv_world <= 1.0))
        return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    TkSel* w = (TkSel*)work;
    const int blocks = tc_blocks(n_pix, 256, TK_MAX_BLOCKS), cblocks = tc_blocks(n_pix, 256 * TK_UNROLL, TK_COUNT_BLOCKS);
    // (a kernel, not hipMemsetAsync: see tc_colsum)
    hipLaunchKernelGGL(topk_clear_kernel, dim3(1), dim3(256), 0, s, w);
    for (int pass = 0; pass < TK_PASSES; ++pass) {
        hipLaunchKernelGGL(topk_count_kernel, dim3(cblocks), dim3(256), 0, s, values, n_pix, w, pass);
        hipLaunchKernelGGL(topk_scan_kernel, dim3(1), dim3(256), 0, s, w, (const double*)state, pass);
    }
    hipLaunchKernelGGL(topk_sum_kernel, dim3(blocks), dim3(256), 0, s, values, n_pix, w);
    hipLaunchKernelGGL(topk_final_kernel, dim3(1), dim3(256), 0, s, (const TkSel*)w, blocks, state, sums, inv_world);
    return tc_launch_status();
}

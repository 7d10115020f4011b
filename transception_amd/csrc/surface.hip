// Directed surface-distance statistics of one class (include/transception_surface.h has the definition): per direction the number of
// surface voxels, the sum of their distances to the other surface, how many lie within a tolerance and the largest squared distance --
// what ASD, ASSD, the surface Dice and the full Hausdorff distance are formed from on the host.  One more pass over maps that the HD95
// path (csrc/metrics.hip) has in memory already: the two uint8 surface maps of tc_metric_surfaces and the two squared-distance maps of
// tc_metric_edt / tc_metric_edt_f64 of class k.
//
// Bound by reading the two uint8 maps: surface voxels are sparse, and a distance map is touched only where the surface map holds k.  Each
// map is scanned on its own, so each has its own alignment: the bytes up to the first 16-byte boundary one by one, then 16-byte pieces (one
// global_load_dwordx4 a thread and iteration; a 32-bit word of a piece is skipped with the has-zero-byte test on word ^ k k k k), then the
// bytes left over.  Two independent scans instead of one loop over both maps cost nothing -- every byte is read once either way -- and
// let the two maps start at different offsets.
//
// No floating-point atomics, and no atomics at all.  The grid is tc_blocks(n, 256, 2048), a function of the shape alone; a thread takes its
// head byte, its pieces p = tid, tid + threads, ... and its tail byte in that (increasing) order, the bytes of a piece in increasing order;
// a wave is reduced by a fixed xor butterfly of shuffles, the four waves by thread 0 in order through LDS, and the workgroup's eight values
// go to its own slot of `work`.  A second launch of one workgroup adds the slots: thread t takes workgroups t, t + 256, ... in increasing
// order, then a fixed binary tree over the 256 threads.  So the fp64 sums repeat to the bit, and `work` needs no zeroing.
// Plain C++.
#include "tc_common.h"
#include "../../include/transception_surface.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;
constexpr int kMaxCls = 16, kMaxDim = 2048;                     // the limits of csrc/metrics.hip (MT_MAXCLS, MT_MAXDIM)
static_assert(kMaxBlocks * 8 * 8 == TC_SURFACE_WORK_BYTES, "the header's work size");

template <typename T> struct SfAcc {                           // one direction
    long long n, within;
    double sum;
    T mx;
};

// a distance to an empty surface is no member: >= TC_METRIC_NO_SOURCE in the int32 maps, +inf in the float64 maps
__device__ __forceinline__ bool sf_member(int d) { return d < TC_METRIC_NO_SOURCE; }
__device__ __forceinline__ bool sf_member(double d) { return d < __builtin_huge_val(); }

template <typename T> __device__ __forceinline__ void sf_take(SfAcc<T>& a, T d, double tol2) {
    if (!sf_member(d)) return;
    a.n += 1;
    a.sum += sqrt((double)d);
    a.within += (double)d <= tol2 ? 1 : 0;
    a.mx = d > a.mx ? d : a.mx;
}

template <typename T> __device__ __forceinline__ void sf_merge(SfAcc<T>& a, const SfAcc<T>& b) {
    a.n += b.n;
    a.within += b.within;
    a.sum += b.sum;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
}

// d2[v] of every v with surf[v] == k into `a`: this thread's share of the map, in increasing order of v
template <typename T>
__device__ __forceinline__ void sf_scan(const unsigned char* __restrict__ surf, const T* __restrict__ d2, int k, int n, double tol2, SfAcc<T>& a) {
    const int tid = blockIdx.x * kThreads + threadIdx.x, threads = gridDim.x * kThreads;      // <= 2048 * 256
    const int head = min(n, (int)((16u - (unsigned)((uintptr_t)surf & 15u)) & 15u));          // bytes in front of the first 16-byte boundary
    const int pieces = (n - head) >> 4, tail = head + (pieces << 4);
    if (tid < head && surf[tid] == k) sf_take(a, d2[tid], tol2);
    const uint4* __restrict__ body = reinterpret_cast<const uint4*>(surf + head);
    const unsigned kkkk = (unsigned)k * 0x01010101u;
    for (int p = tid; p < pieces; p += threads) {                                              // p + threads < 2^27 + 2^19
        const uint4 q = body[p];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        const int v0 = head + (p << 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned x = w[j] ^ kkkk;                                                    // a zero byte where surf == k
            if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (((x >> (8 * b)) & 255u) == 0) sf_take(a, d2[v0 + 4 * j + b], tol2);
        }
    }
    if (tid < n - tail && surf[tail + tid] == k) sf_take(a, d2[tail + tid], tol2);             // fewer than 16 bytes are left
}

template <typename T> __device__ __forceinline__ void sf_wave_reduce(SfAcc<T>& a) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        SfAcc<T> b;
        b.n = __shfl_xor(a.n, off, 64);
        b.within = __shfl_xor(a.within, off, 64);
        b.sum = __shfl_xor(a.sum, off, 64);
        b.mx = __shfl_xor(a.mx, off, 64);
        sf_merge(a, b);                                                                        // a + b == b + a: every lane holds the same bits
    }
}

__device__ __forceinline__ long long sf_bits(int v) { return (long long)v; }
__device__ __forceinline__ long long sf_bits(double v) { return __double_as_longlong(v); }
__device__ __forceinline__ void sf_from_bits(long long b, int& v) { v = (int)b; }
__device__ __forceinline__ void sf_from_bits(long long b, double& v) { v = __longlong_as_double(b); }

// [n, sum, within, max] of one direction, the layout of `out` and of a slot of `work`
template <typename T> __device__ __forceinline__ void sf_store(long long* o, const SfAcc<T>& a) {
    o[0] = a.n; o[1] = __double_as_longlong(a.sum); o[2] = a.within; o[3] = sf_bits(a.mx);
}
template <typename T> __device__ __forceinline__ void sf_load(const long long* o, SfAcc<T>& a) {
    a.n = o[0]; a.sum = __longlong_as_double(o[1]); a.within = o[2]; sf_from_bits(o[3], a.mx);
}

template <typename T> __global__ __launch_bounds__(kThreads)
void surface_stats_kernel(const unsigned char* __restrict__ sP, const unsigned char* __restrict__ sG, const T* __restrict__ d2P,
                          const T* __restrict__ d2G, int k, int n, double tol2, long long* __restrict__ work) {
    __shared__ long long part[kThreads / 64][8];
    SfAcc<T> a[2] = {{0, 0, 0.0, (T)0}, {0, 0, 0.0, (T)0}};
    sf_scan(sP, d2G, k, n, tol2, a[0]);                        // direction 0: from the prediction's surface to the ground truth's
    sf_scan(sG, d2P, k, n, tol2, a[1]);                        // direction 1
    sf_wave_reduce(a[0]);
    sf_wave_reduce(a[1]);
    if ((threadIdx.x & 63) == 0) {
        sf_store(part[threadIdx.x >> 6], a[0]);
        sf_store(part[threadIdx.x >> 6] + 4, a[1]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kThreads / 64; ++w)
        for (int i = 0; i < 2; ++i) {
            SfAcc<T> b;
            sf_load(part[w] + 4 * i, b);
            sf_merge(a[i], b);
        }
    sf_store(work + 8 * blockIdx.x, a[0]);
    sf_store(work + 8 * blockIdx.x + 4, a[1]);
}

// one workgroup: the `blocks` slots of `work` into the eight slots of class k
template <typename T> __global__ __launch_bounds__(kThreads)
void surface_final_kernel(const long long* __restrict__ work, int blocks, long long* __restrict__ out) {
    __shared__ long long tree[kThreads][8];
    const int t = threadIdx.x;
    SfAcc<T> a[2] = {{0, 0, 0.0, (T)0}, {0, 0, 0.0, (T)0}};
    for (int b = t; b < blocks; b += kThreads)
        for (int i = 0; i < 2; ++i) {
            SfAcc<T> s;
            sf_load(work + 8 * b + 4 * i, s);
            sf_merge(a[i], s);
        }
    sf_store(tree[t], a[0]);
    sf_store(tree[t] + 4, a[1]);
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (t < off)
            for (int i = 0; i < 2; ++i) {
                SfAcc<T> s;
                sf_load(tree[t + off] + 4 * i, s);
                sf_merge(a[i], s);
                sf_store(tree[t] + 4 * i, a[i]);
            }
        __syncthreads();
    }
    if (t == 0) {
        sf_store(out, a[0]);
        sf_store(out + 4, a[1]);
    }
}

template <typename T>
int surface_stats(const unsigned char* surf_pred, const unsigned char* surf_gt, const T* d2_pred, const T* d2_gt, int k, int ncls, int D, int H, int W,
                  double tol2, void* work, long long* out, void* stream) {
    if (!surf_pred || !surf_gt || !d2_pred || !d2_gt || !work || !out || D <= 0 || H <= 0 || W <= 0 || D > kMaxDim || H > kMaxDim || W > kMaxDim ||
        (long long)D * H * W >= 0x7fffffffLL || ncls <= 0 || ncls > kMaxCls || k <= 0 || k >= ncls || !(tol2 >= 0.0 && tol2 < __builtin_huge_val()))
        return TC_ERR_ARG;                                                                     // !(...): false for a NaN
    const int n = D * H * W, blocks = tc_blocks(n, kThreads, kMaxBlocks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((surface_stats_kernel<T>), dim3(blocks), dim3(kThreads), 0, s, surf_pred, surf_gt, d2_pred, d2_gt, k, n, tol2, (long long*)work);
    hipLaunchKernelGGL((surface_final_kernel<T>), dim3(1), dim3(kThreads), 0, s, (const long long*)work, blocks, out + 8 * k);
    return tc_launch_status();
}

}  // namespace

extern "C" int tc_surface_abi_version(void) { return TC_SURFACE_ABI_VERSION; }

extern "C" int tc_surface_stats(const unsigned char* surf_pred, const unsigned char* surf_gt, const int* d2_pred, const int* d2_gt, int k, int ncls,
                                int D, int H, int W, double tol2, void* work, long long* out, void* stream) {
    return surface_stats<int>(surf_pred, surf_gt, d2_pred, d2_gt, k, ncls, D, H, W, tol2, work, out, stream);
}

extern "C" int tc_surface_stats_f64(const unsigned char* surf_pred, const unsigned char* surf_gt, const double* d2_pred, const double* d2_gt, int k,
                                    int ncls, int D, int H, int W, double tol2, void* work, long long* out, void* stream) {
    return surface_stats<double>(surf_pred, surf_gt, d2_pred, d2_gt, k, ncls, D, H, W, tol2, work, out, stream);
}

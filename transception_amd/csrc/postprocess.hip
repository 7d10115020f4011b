// Connected-component post-processing of a predicted label volume on the device (include/transception_post.h has the definition): per
// class keep the largest component, or every component of at least N voxels.  uint8 [D,H,W] in, uint8 [D,H,W] out.
//
// One lock-free union-find over the whole volume serves every class at once: a voxel has one label, so two neighbours are joined only
// when their labels are equal and foreground (the trick of the surface map in metrics.hip).  parent[] is int32 [D,H,W]:
//   (a) init      parent[v] = first voxel of v's run of equal labels inside its row and its wave, -1 for background;
//   (b) merge     every foreground voxel unions itself with the backward half of its neighbourhood that carries its label;
//   (c) compress  root[v] = find(v), in place;
//   (d) sizes     size[root] by integer atomic adds, then per class one 64-bit atomic max over a key ordered by (size, smaller root);
//   (e) keep      the two modes.
//
// The invariants that make this safe on a shared machine (each is repeated at the loop it is about):
//   I1  parent[x] <= x at all times, and parent[x] only ever decreases (init writes <= x; afterwards only atomicMin and compress's
//       store of an ancestor write it);
//   I2  parent[x] is always a voxel of x's own component, whatever age the value read has;
//   I3  so every find walks strictly downward and ends after at most x steps, and a stale value costs steps, never correctness;
//   I4  no loop waits for another thread's write: no spin-wait, no lock, no grid barrier.  The only communication between workgroups
//       inside a launch is the atomic min of (b); everything else is ordered by launch boundaries on one stream.
// Integer atomics only; with "root = smallest index" and the tie rule every output is independent of the order of arrival.
#include "tc_common.h"
#include "../../include/transception_post.h"

#define CC_MAXCLS 16
#define CC_MAXDIM 2048

__device__ __forceinline__ bool cc_fg(int c, int ncls) { return c >= 1 && c < ncls; }

// ---- (a) init -------------------------------------------------------------------------------------------------------------------------
// A wave holds 64 consecutive voxels.  A lane starts a run if it is the wave's first, the row's first, or its left neighbour's label
// differs; a voxel's parent is the nearest run start at or left of it: one ballot and a clz replace most unions along x.  I1: start <= v.
// I2: every voxel between the start and v carries v's label in v's row.  Every lane of a wave runs the same number of iterations (the
// ballot needs the whole wave); `ok` masks the tail.
__global__ __launch_bounds__(256) void cc_init_kernel(const unsigned char* __restrict__ lab, int* __restrict__ parent, int n, int W, int ncls) {
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); base < n; base += (long long)gridDim.x * 256) {
        const long long vv = base + lane;
        const bool ok = vv < n;
        const int v = ok ? (int)vv : 0;
        const int c = ok ? lab[v] : 0;
        const int left = __shfl_up(c, 1, 64);
        const unsigned long long starts = __ballot(lane == 0 || v % W == 0 || left != c);           // bit 0 is always set
        const int start = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
        if (ok) parent[v] = cc_fg(c, ncls) ? (int)base + start : -1;
    }
}

// ---- (b) merge ------------------------------------------------------------------------------------------------------------------------
// Reads of parent[] here are relaxed device-scope atomic loads.  What that guarantees: the compiler may not hoist them out of a loop or
// reuse an earlier value, and they bypass the compute unit's L1.  They are still served from the XCD's own L2, so the value may be
// STALE: another XCD's atomic min may have lowered the word since.  Stale is harmless here (I2: an old parent is still a voxel of the
// same component, and the atomic min below decides); it only lengthens the walk, and by I3 and the argument at cc_union no stale value
// can keep a loop going.  What the project measured about scopes of atomics across XCDs: profiles/r4_atomic_scope.txt.
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// I3: p = parent[x] <= x (I1), and the loop goes on only while p < x: x strictly decreases, so it ends after at most x steps whatever
// values it reads.  It waits for nothing (I4): if no other thread ever wrote again it would still end.
__device__ __forceinline__ int cc_find(const int* parent, int x) {
    for (int p = cc_load(parent + x); p != x; p = cc_load(parent + x)) x = p;
    return x;
}

// The standard lock-free union: find both roots, make a > b, old = atomicMin(&parent[a], b); done if old == a (a was still a root and now
// hangs under b).  Otherwise another thread hung a under old < a in the meantime; parent[a] is now min(old, b), both of a's component
// (I2), and what is left to do is to join old with b.  I1 holds: the only write is a min with b < a.  It ends: after a failed round
// find(old) <= old < a and find(b) <= b < a, so max(a, b) strictly decreases from round to round and is bounded by 0 -- again whatever
// the other threads do, and without waiting for any of them (I4).
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

// FULL = false: the backward face neighbours x-1, y-1, z-1; FULL = true: the 13 backward neighbours of the 3 x 3 x 3 block.
// x-1 is already joined by (a) unless v is the first lane of its wave there (v % 64 == 0: the grid-stride bases of (a) are multiples of
// 64).  Faces: the union with y-1 is skipped where v-1 and v-1-W carry the label too -- v ~ v-1 along x, v-1 ~ v-1-W is v-1's own
// union (or skipped for the same reason, down to the run's first voxel, which never skips), v-1-W ~ v-W along x; likewise z-1.
template <bool FULL>
__global__ __launch_bounds__(256) void cc_merge_kernel(const unsigned char* __restrict__ lab, int* parent, int D, int H, int W, int ncls) {
    const int HW = H * W, n = D * HW;
    for (long long vv = (long long)blockIdx.x * 256 + threadIdx.x; vv < n; vv += (long long)gridDim.x * 256) {
        const int v = (int)vv;
        const int c = lab[v];
        if (!cc_fg(c, ncls)) continue;
        const int z = v / HW, r = v - z * HW, y = r / W, x = r - y * W;
        const bool xl = x > 0 && lab[v - 1] == c;
        if (xl && (v & 63) == 0) cc_union(parent, v, v - 1);
        if (!FULL) {
            if (y > 0 && lab[v - W] == c && !(xl && lab[v - W - 1] == c)) cc_union(parent, v, v - W);
            if (z > 0 && lab[v - HW] == c && !(xl && lab[v - HW - 1] == c)) cc_union(parent, v, v - HW);
        } else {
            for (int dz = -1; dz <= 0; ++dz) {
                if (z + dz < 0) continue;
                for (int dy = -1; dy <= (dz ? 1 : 0); ++dy) {
                    if (y + dy < 0 || y + dy >= H) continue;
                    for (int dx = -1; dx <= 1; ++dx) {
                        if ((dz == 0 && dy == 0) || x + dx < 0 || x + dx >= W) continue;     // (0, 0, -1) is the x-1 case above
                        const int u = v + (dz * H + dy) * W + dx;
                        if (lab[u] == c) cc_union(parent, v, u);
                    }
                }
            }
        }
    }
}

// ---- (c) compress ---------------------------------------------------------------------------------------------------------------------
// root[v] = find(v), in place.  Every union is behind a launch boundary, so plain loads see the finished forest; the only writes in this
// launch store a voxel's own root over its parent -- an ancestor, so I1 and I2 hold and a walk that meets either value ends at the same
// root (I3).  The walk reads a new address at every step: there is nothing to hoist.
__global__ __launch_bounds__(256) void cc_compress_kernel(int* parent, int n) {
    for (long long vv = (long long)blockIdx.x * 256 + threadIdx.x; vv < n; vv += (long long)gridDim.x * 256) {
        int x = parent[vv];
        if (x < 0) continue;
        for (int p = parent[x]; p != x; p = parent[x]) x = p;                            // strictly downward: p < x
        parent[vv] = x;
    }
}

// ---- (d) sizes and best ---------------------------------------------------------------------------------------------------------------
// size[root[v]] += 1.  The 64 consecutive voxels of a wave lie in a handful of components, so each round takes the first lane still to do,
// counts the lanes with its root by ballot and lets that lane add the count: one atomic per distinct root of the wave.  `left` is
// wave-uniform and loses at least the leader's bit per round: at most 64 rounds, in lockstep, waiting for no memory (I4).
__global__ __launch_bounds__(256) void cc_count_kernel(const int* __restrict__ root, int* __restrict__ size, int n) {
    const int lane = threadIdx.x & 63;
    for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); base < n; base += (long long)gridDim.x * 256) {
        const long long vv = base + lane;
        const int r = vv < n ? root[vv] : -1;
        bool todo = r >= 0 && r < n;                                                     // (a root map from elsewhere cannot send an add outside size[])
        unsigned long long left = __ballot(todo);
        while (left) {
            const int leader = __ffsll(left) - 1;
            const int rl = __shfl(r, leader, 64);
            const unsigned long long same = __ballot(todo && r == rl);
            if (lane == leader) atomicAdd(size + rl, __popcll(same));
            todo = todo && r != rl;
            left &= ~same;
        }
    }
}

// The key of a component: size in the high bits, 2^31 - 1 - root below, so the greatest key is the greatest size and, among equal sizes,
// the smallest root.  size < 2^31 and 0 <= root < 2^31 - 1: 62 bits.  A class's maximum is taken in LDS first, then one global atomic max
// per workgroup and class; keys[2k] is best[k][0] until cc_unpack_kernel has run.
#define CC_ROOT_BITS 31
#define CC_ROOT_MASK 0x7fffffffull
__global__ __launch_bounds__(256) void cc_best_kernel(const unsigned char* __restrict__ lab, const int* __restrict__ root, const int* __restrict__ size,
                                                      unsigned long long* __restrict__ keys, int n, int ncls) {
    __shared__ unsigned long long lk[CC_MAXCLS];
    if (threadIdx.x < CC_MAXCLS) lk[threadIdx.x] = 0;
    __syncthreads();
    for (long long vv = (long long)blockIdx.x * 256 + threadIdx.x; vv < n; vv += (long long)gridDim.x * 256) {
        const int c = lab[vv];
        if (root[vv] != (int)vv || !cc_fg(c, ncls)) continue;                            // roots only; a root is foreground
        atomicMax(&lk[c], ((unsigned long long)size[vv] << CC_ROOT_BITS) | (CC_ROOT_MASK - (unsigned long long)vv));
    }
    __syncthreads();
    if (threadIdx.x < ncls && lk[threadIdx.x]) atomicMax(&keys[2 * threadIdx.x], lk[threadIdx.x]);
}

__global__ void cc_unpack_kernel(long long* __restrict__ best, int ncls) {
    const int k = threadIdx.x;
    if (k >= ncls) return;
    const unsigned long long key = (unsigned long long)best[2 * k];
    best[2 * k] = (long long)(key >> CC_ROOT_BITS);
    best[2 * k + 1] = key ? (long long)(CC_ROOT_MASK - (key & CC_ROOT_MASK)) : -1;      // a component has size >= 1: key != 0
}

// ---- (e) keep -------------------------------------------------------------------------------------------------------------------------
// out may be lab: a thread reads and writes its own voxel only (so neither pointer is __restrict__).
__global__ __launch_bounds__(256) void cc_keep_kernel(const unsigned char* lab, const int* __restrict__ root, const int* __restrict__ size,
                                                      const long long* __restrict__ best, unsigned char* out, int mode, long long min_voxels,
                                                      int n, int ncls) {
    for (long long vv = (long long)blockIdx.x * 256 + threadIdx.x; vv < n; vv += (long long)gridDim.x * 256) {
        const int c = lab[vv];
        bool keep = true;
        if (cc_fg(c, ncls)) {
            const int r = root[vv];
            keep = mode == TC_CC_LARGEST ? (long long)r == best[2 * c + 1] : (r >= 0 && r < n && (long long)size[r] >= min_voxels);
        }
        out[vv] = keep ? (unsigned char)c : (unsigned char)0;
    }
}

// ---- entries --------------------------------------------------------------------------------------------------------------------------
static bool cc_shape_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && D <= CC_MAXDIM && H <= CC_MAXDIM && W <= CC_MAXDIM && (long long)D * H * W < 0x7fffffffLL;
}
static bool cc_ncls_ok(int ncls) { return ncls >= 2 && ncls <= CC_MAXCLS; }

extern "C" int tc_post_abi_version(void) { return TC_POST_ABI_VERSION; }

extern "C" long long tc_cc_scratch_bytes(int D, int H, int W) { return cc_shape_ok(D, H, W) ? 8LL * D * H * W : 0; }

extern "C" int tc_cc_label(const unsigned char* lab, int* root, int D, int H, int W, int ncls, int connectivity, void* stream) {
    if (!lab || !root || !cc_shape_ok(D, H, W) || !cc_ncls_ok(ncls) || (connectivity != 1 && connectivity != 3)) return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int n = D * H * W, blocks = tc_blocks(n, 256, 4096);
    hipLaunchKernelGGL(cc_init_kernel, dim3(blocks), dim3(256), 0, s, lab, root, n, W, ncls);
    if (connectivity == 1) hipLaunchKernelGGL(cc_merge_kernel<false>, dim3(blocks), dim3(256), 0, s, lab, root, D, H, W, ncls);
    else hipLaunchKernelGGL(cc_merge_kernel<true>, dim3(blocks), dim3(256), 0, s, lab, root, D, H, W, ncls);
    hipLaunchKernelGGL(cc_compress_kernel, dim3(blocks), dim3(256), 0, s, root, n);
    return tc_launch_status();
}

extern "C" int tc_cc_sizes(const unsigned char* lab, const int* root, int* size, long long* best, int D, int H, int W, int ncls, void* stream) {
    if (!lab || !root || !size || !best || !cc_shape_ok(D, H, W) || !cc_ncls_ok(ncls)) return TC_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int n = D * H * W, blocks = tc_blocks(n, 256, 4096);
    if (hipMemsetAsync(size, 0, (size_t)n * sizeof(int), s) != hipSuccess) return TC_ERR_LAUNCH;
    if (hipMemsetAsync(best, 0, (size_t)ncls * 2 * sizeof(long long), s) != hipSuccess) return TC_ERR_LAUNCH;
    hipLaunchKernelGGL(cc_count_kernel, dim3(blocks), dim3(256), 0, s, root, size, n);
    hipLaunchKernelGGL(cc_best_kernel, dim3(blocks), dim3(256), 0, s, lab, root, size, (unsigned long long*)best, n, ncls);
    hipLaunchKernelGGL(cc_unpack_kernel, dim3(1), dim3(64), 0, s, best, ncls);
    return tc_launch_status();
}

extern "C" int tc_cc_keep(const unsigned char* lab, const int* root, const int* size, const long long* best, unsigned char* out, int mode,
                          long long min_voxels, int D, int H, int W, int ncls, void* stream) {
    if (!lab || !root || !size || !best || !out || !cc_shape_ok(D, H, W) || !cc_ncls_ok(ncls) ||
        !(mode == TC_CC_LARGEST || (mode == TC_CC_MIN_VOXELS && min_voxels >= 1)))
        return TC_ERR_ARG;
    const int n = D * H * W;
    hipLaunchKernelGGL(cc_keep_kernel, dim3(tc_blocks(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, lab, root, size, best, out, mode,
                       min_voxels, n, ncls);
    return tc_launch_status();
}

// rgcn_sort_scan.h -- the integer building blocks the device-side builders share (rgcn_plan.hip: graph plans; rgcn_summary.hip:
// node partitions and quotient graphs; rgcn_sample.hip: in-edge index and fan-out hops; rgcn_minibatch.hip: block indices; rgcn_linkpred.hip: triple indices): a stable
// LSD radix sort of (u64 key, u32 value) pairs, an exclusive scan of u32, head flags / run ids over sorted keys, and the host
// plumbing of a builder: carving a workspace (Arena, take_sort_bufs), the other pair of the sort buffers (from_pair), the one read-back of a
// build's scalars (read_back).  gfx950 only.  Everything has internal linkage: every including source gets its own copy of the kernels.
//
//   sort      LSD radix sort, 8-bit digits, stable: per wave-segment digit histograms -> one exclusive scan -> scatter
//             with wave-level multi-split ranking (ballots), no cross-wave traffic inside a pass
//
// All byte / integer work: bound by HBM traffic (about 35 B per key and sort pass), nothing here touches MFMA.
#ifndef RGCN_SORT_SCAN_H
#define RGCN_SORT_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rgcn_sort_scan {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kSortItems = 32;                 // keys per lane of one wave segment
constexpr int kSegKeys = 64 * kSortItems;      // 2,048 keys per wave segment
constexpr int kSortThreads = 256;              // four independent wave segments per workgroup
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;
constexpr int kScanBlock = kScanThreads * kScanItems;   // 2,048 elements per scan workgroup

__host__ __device__ inline int bits_for(u64 max_value) {   // bits needed to hold 0 .. max_value (at least 1)
    int b = 1;
    while ((max_value >> b) != 0 && b < 64) ++b;
    return b;
}

// splitmix64's finaliser: the one mixing step of the counter-based generators (rgcn_sample.hip: fan-out draws; rgcn_linkpred.hip:
// negatives).  A draw is a pure function of its key, never of launch geometry.
__host__ __device__ inline u64 mix(u64 z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// ------------------------------------------------------------------------------------------------
// exclusive scan of u32 (two levels: workgroup sums -> one workgroup scans the sums -> apply)
// ------------------------------------------------------------------------------------------------
__device__ inline u32 block_exclusive_scan(u32 v, u32* lds_wave_tot, u32& block_total) {
    // v: this thread's value; returns the exclusive prefix over the 256 threads of the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u32 inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) lds_wave_tot[wave] = inc;
    __syncthreads();
    u32 before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
        const u32 t = lds_wave_tot[w];
        if (w < wave) before += t;
        tot += t;
    }
    __syncthreads();
    block_total = tot;
    return before + inc - v;
}

static __global__ void scan_reduce_kernel(const u32* __restrict__ in, u32 n, u32* __restrict__ sums) {
    __shared__ u32 wt[kScanThreads / 64];
    const size_t base = (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * kScanItems;
    u32 s = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (base + j < n) s += in[base + j];
    u32 tot;
    block_exclusive_scan(s, wt, tot);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

// one workgroup: sums[0 .. m) -> exclusive scan in place, grand total -> sums[m]
static __global__ void scan_top_kernel(u32* __restrict__ sums, u32 m) {
    __shared__ u32 wt[kScanThreads / 64];
    u32 carry = 0;
    for (u32 c0 = 0; c0 < m; c0 += kScanBlock) {
        const u32 base = c0 + threadIdx.x * kScanItems;
        u32 v[kScanItems], s = 0;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            v[j] = base + j < m ? sums[base + j] : 0u;
            s += v[j];
        }
        u32 tot;
        u32 ex = block_exclusive_scan(s, wt, tot) + carry;
#pragma unroll
        for (int j = 0; j < kScanItems; ++j) {
            if (base + j < m) sums[base + j] = ex;
            ex += v[j];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) sums[m] = carry;
}

static __global__ void scan_apply_kernel(const u32* __restrict__ in, u32* __restrict__ out, u32 n, const u32* __restrict__ sums) {
    __shared__ u32 wt[kScanThreads / 64];
    const size_t base = (size_t)blockIdx.x * kScanBlock + (size_t)threadIdx.x * kScanItems;
    u32 v[kScanItems], s = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        v[j] = base + j < n ? in[base + j] : 0u;
        s += v[j];
    }
    u32 tot;
    u32 ex = block_exclusive_scan(s, wt, tot) + sums[blockIdx.x];
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (base + j < n) out[base + j] = ex;
        ex += v[j];
    }
}

// out[i] = sum of in[0 .. i); the grand total lands in sums[nblocks] (device).  in may equal out.
static u32 scan_blocks(u32 n) { return (n + kScanBlock - 1) / kScanBlock; }
static void exclusive_scan(const u32* in, u32* out, u32 n, u32* sums, hipStream_t s) {
    const u32 nb = scan_blocks(n);
    if (nb == 0) {
        (void)hipMemsetAsync(sums, 0, sizeof(u32), s);
        return;
    }
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(nb), dim3(kScanThreads), 0, s, in, n, sums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(kScanThreads), 0, s, sums, nb);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nb), dim3(kScanThreads), 0, s, in, out, n, sums);
}

// ------------------------------------------------------------------------------------------------
// stable LSD radix sort of (u64 key, u32 value) pairs, 8 bits per pass
// ------------------------------------------------------------------------------------------------
__device__ inline u32 digit_of(u64 k, int shift) { return (u32)(k >> shift) & 255u; }

// hist[d * nseg + seg] = keys of wave segment `seg` whose digit is d
static __global__ void radix_hist_kernel(const u64* __restrict__ keys, u32 n, int shift, u32 nseg, u32* __restrict__ hist) {
    __shared__ u32 cnt[kSortThreads / 64][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 seg = blockIdx.x * (kSortThreads / 64) + wave;
    for (int d = lane; d < 256; d += 64) cnt[wave][d] = 0;
    __syncthreads();
    if (seg < nseg) {
        const size_t base = (size_t)seg * kSegKeys;
        for (int r = 0; r < kSortItems; ++r) {
            const size_t i = base + (size_t)r * 64 + lane;
            if (i < n) atomicAdd(&cnt[wave][digit_of(keys[i], shift)], 1u);
        }
    }
    __syncthreads();
    if (seg < nseg)
        for (int d = lane; d < 256; d += 64) hist[(size_t)d * nseg + seg] = cnt[wave][d];
}

// offs = exclusive scan of hist in memory order (digit-major, segment-minor): where this segment's keys of digit d
// start in the output.  A wave ranks its 64 keys of a round by wave-level multi-split: eight ballots give every lane
// the set of lanes holding the same digit; its rank among them keeps the input order (stable), the first of them
// advances the segment's running offset of that digit in LDS.
static __global__ void radix_scatter_kernel(const u64* __restrict__ kin, const u32* __restrict__ vin, u64* __restrict__ kout,
                                     u32* __restrict__ vout, u32 n, int shift, u32 nseg, const u32* __restrict__ offs) {
    __shared__ u32 cnt_s[kSortThreads / 64][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 seg = blockIdx.x * (kSortThreads / 64) + wave;
    volatile u32* cnt = cnt_s[wave];
    if (seg < nseg)
        for (int d = lane; d < 256; d += 64) cnt[d] = offs[(size_t)d * nseg + seg];
    __syncthreads();
    if (seg >= nseg) return;
    const size_t base = (size_t)seg * kSegKeys;
    const u64 below = (1ull << lane) - 1ull;
    for (int r = 0; r < kSortItems; ++r) {
        const size_t i = base + (size_t)r * 64 + lane;
        const bool valid = i < n;
        const u64 k = valid ? kin[i] : 0ull;
        const u32 v = valid ? vin[i] : 0u;
        const u32 dg = digit_of(k, shift);
        u64 peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (dg >> b) & 1u;
            const u64 m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const u32 rank = (u32)__popcll(peers & below);
        const int leader = valid ? (__ffsll((long long)peers) - 1) : lane;
        u32 off = 0;
        if (valid && lane == leader) {
            off = cnt[dg];
            cnt[dg] = off + (u32)__popcll(peers);
        }
        __builtin_amdgcn_wave_barrier();
        off = __shfl(off, leader);
        if (valid) {
            kout[(size_t)off + rank] = k;
            vout[(size_t)off + rank] = v;
        }
    }
}

struct SortBufs {
    u64* k[2];
    u32* v[2];
    u32* hist;   // 256 * nseg + 1
    u32* sums;   // scan_blocks(256 * nseg) + 1
};

static u32 sort_segments(u32 n) { return (n + kSegKeys - 1) / kSegKeys; }

// sorts by the low `bits` bits of the key; data starts in (k[0], v[0]); returns the index of the pair holding the result
static int radix_sort_pairs(const SortBufs& b, u32 n, int bits, hipStream_t s) {
    int cur = 0;
    if (n <= 1) return cur;
    const u32 nseg = sort_segments(n);
    const u32 nblk = (nseg + kSortThreads / 64 - 1) / (kSortThreads / 64);
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3(nblk), dim3(kSortThreads), 0, s, b.k[cur], n, shift, nseg, b.hist);
        exclusive_scan(b.hist, b.hist, 256u * nseg, b.sums, s);
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(nblk), dim3(kSortThreads), 0, s, b.k[cur], b.v[cur], b.k[cur ^ 1],
                           b.v[cur ^ 1], n, shift, nseg, b.hist);
        cur ^= 1;
    }
    return cur;
}

// flag[i] = 1 where element i starts a run of equal (key >> shift)
static __global__ void head_flags_kernel(const u64* __restrict__ keys, u32 n, int shift, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || (keys[i] >> shift) != (keys[i - 1] >> shift)) ? 1u : 0u;
}

// ex = exclusive scan of the head flags: for the head of a run that is the run's index, for the other elements of the
// run it is the index + 1 (their head is already counted).  id[i] = ex[i] + flag[i] - 1 is the run index of EVERY element.
static __global__ void run_ids_kernel(u32* __restrict__ ex, const u32* __restrict__ flag, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ex[i] = ex[i] + flag[i] - 1u;
}

static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
static u32 grid_for(u64 n, int threads = 256) { return (u32)((n + threads - 1) / threads); }

// ids[i] = index of the run of equal (key >> shift) that element i of the sorted keys lies in; flag keeps the head flags, the
// number of runs lands in sums[scan_blocks(n)] (device)
static void run_ids(const u64* keys, u32 n, int shift, u32* flag, u32* ids, u32* sums, hipStream_t s) {
    hipLaunchKernelGGL(head_flags_kernel, dim3(grid_for(n)), dim3(256), 0, s, keys, n, shift, flag);
    exclusive_scan(flag, ids, n, sums, s);
    hipLaunchKernelGGL(run_ids_kernel, dim3(grid_for(n)), dim3(256), 0, s, ids, flag, n);
}

// the SortBufs whose pair 0 is pair `cur` of b: where a sort left its result becomes the next sort's input
static SortBufs from_pair(const SortBufs& b, int cur) {
    SortBufs r = b;
    r.k[0] = b.k[cur];
    r.k[1] = b.k[cur ^ 1];
    r.v[0] = b.v[cur];
    r.v[1] = b.v[cur ^ 1];
    return r;
}

// A workspace handed out front to back in 256-byte aligned pieces.  A null base sizes it: every take is nullptr, bytes() the total.
struct Arena {
    char* base;
    size_t off = 0;
    explicit Arena(void* b) : base((char*)b) {}
    template <class T>
    T* take(size_t count) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += align_up(count * sizeof(T));
        return p;
    }
    size_t bytes() const { return off; }
};

constexpr u64 kMaxKeys = 0xFFFF0000ull;      // the sort counts keys in u32, rounded up to whole 2,048-key segments

// The buffers of a sort of n keys, in this order; sums also serves the caller's own scans of up to longest_scan elements.
static SortBufs take_sort_bufs(Arena& ar, u64 n, u64 longest_scan = 0) {
    SortBufs b;
    const u32 nseg = sort_segments((u32)n);
    b.k[0] = ar.take<u64>(n);
    b.k[1] = ar.take<u64>(n);
    b.v[0] = ar.take<u32>(n);
    b.v[1] = ar.take<u32>(n);
    b.hist = ar.take<u32>((size_t)256 * nseg + 1);
    const u64 scan_len = longest_scan > (u64)256 * nseg ? longest_scan : (u64)256 * nseg;
    b.sums = ar.take<u32>((size_t)scan_blocks((u32)scan_len) + 2);
    return b;
}

// *host = *dev once the stream's work is done: the copy and the synchronisation of a builder's scalars
template <class T>
static int read_back(const T* dev, T* host, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(host, dev, sizeof(T), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return (int)e;
}

}  // namespace rgcn_sort_scan

#endif  // RGCN_SORT_SCAN_H

// rgcn_transfer.hip -- the glue between training on summaries and training on the original graph, behind the C ABI rgcn_tr_* of
// include/rgcn_mi355x.h: the fractional labels of a node partition and the transferred embedding of every original node, on
// tensors alone.  gfx950 only.  DESIGN.md section 19 has the semantics.
//
//   rgcn_tr_block_labels   size[b] = nodes of block b; cnt[b][c] = sum of y[i][c] over the training rows i whose node lies in b
//                          (int32, vector integer atomics); y_sum[b][c] = float(double(cnt) / double(max(1, size))), the double
//                          quotient rounded once -- graphs.Dataset.make_training_data's v[c] / max(1, len(org_nodes)) bit for bit.
//     tr_size_kernel       a wave counts kSizeChunks chunks of 64 consecutive nodes, loaded up front.  Equal ids of a chunk are
//                          combined before the atomic: up to kLeaderRounds times the first lane left takes its id, a ballot finds
//                          the lanes that hold the same one, the leader adds their count and they all retire; what is left after
//                          that holds more than kLeaderRounds distinct ids per chunk and adds 1 per lane.  A chunk that is ONE id
//                          is counted in a register that reaches memory when the id changes or the wave ends: the one-block
//                          partition costs one atomic per 1,024 nodes, not one per node.
//     tr_count_kernel      one lane per (training row, class): a non-zero count is added to cnt[block[node]][class]
//     tr_finish_kernel     one lane per block: the quotients of its row, and nonzero[b]
//   rgcn_tr_gather         out row j (node = nodes[j], or j) from S summary tables through S node maps: a mapped piece is the
//                          table row, an unmapped one a uniform draw in [0, 1) that is a pure function of (seed, s, node, column).
//     tr_gather_kernel     a unit is G = min(ceil(E / 4), 64) lanes of one wave (one 16-byte piece each, several passes beyond 256
//                          columns), 64 / G units per wave; the unit's first lane loads the node id and, per table, the map value and
//                          hands them to the others.  STACK / CONCAT store every piece where it belongs, SUM adds the S pieces
//                          in table order in a register (0 + t_0 + t_1 ...: Python's sum) and stores once.  Pieces that are not
//                          whole, and every piece when a stride or a base is not 16-byte aligned, go element by element.  The
//                          16-byte stores of a whole table (no node list) are non-temporal.
// Bandwidth bound: the tables are small and stay in cache, the output is the traffic.  Every row address is a 64-bit element
// offset on plain pointers ([S, N, E] passes 2^32 bytes at N = 10M).  An id out of range is never used as an address: it sets a
// bit of the caller's `bad` word (integer atomic).  No float atomics: the same inputs give the same bits.
#include "rgcn_common.h"
#include "rgcn_sort_scan.h"

namespace rgcn_tr {

using namespace rgcn_sort_scan;
using rgcn::f32x4;

constexpr int kLeaderRounds = 8;
constexpr int kSizeChunks = 16;                   // chunks of 64 nodes one wave of tr_size_kernel counts
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;
constexpr int64_t kMaxCount = 0x7FFFFFFFll;       // nodes, blocks, training rows: int32 on the device
constexpr int kMaxClasses = 65536;
constexpr u64 kMaxCells = 1ull << 38;             // (row, class) cells of y and of the counts: one lane each, 2^31 workgroups at most

// ---- labels --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tr_size_kernel(const int64_t* __restrict__ block, u32 n, int64_t num_blocks,
                                                      int32_t* __restrict__ size, int32_t* __restrict__ bad) {
    // (the grid covers n rounded up to whole waves of kSizeChunks chunks: no early return before the ballots)
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const u64 base = wave * (u64)(64 * kSizeChunks) + (u64)lane;
    int64_t ids[kSizeChunks];
#pragma unroll
    for (int k = 0; k < kSizeChunks; ++k) {      // all loads first: one round trip per wave
        const u64 i = base + (u64)(64 * k);
        ids[k] = i < (u64)n ? block[i] : -1;
    }
    int64_t carry_id = -1;                       // wave-uniform: whole chunks of one id are counted here ...
    int32_t carry = 0;
#pragma unroll
    for (int k = 0; k < kSizeChunks; ++k) {
        int64_t b = ids[k];
        if (base + (u64)(64 * k) < (u64)n && (b < 0 || b >= num_blocks)) {
            if (bad != nullptr) atomicOr(bad, RGCN_TR_BAD_BLOCK);
            b = -1;
        }
        bool left = b >= 0;
        for (int round = 0; round < kLeaderRounds; ++round) {
            const u64 todo = __ballot(left);
            if (todo == 0ull) break;
            const int leader = __ffsll((long long)todo) - 1;
            const int64_t lb = __shfl(b, leader);
            const bool same = left && b == lb;
            const int32_t peers = (int32_t)__popcll(__ballot(same));
            if (round == 0 && peers == 64) {     // ... and reach memory once per run of such chunks
                if (lb != carry_id) {
                    if (carry > 0 && lane == 0) atomicAdd(&size[carry_id], carry);
                    carry_id = lb;
                    carry = 0;
                }
                carry += 64;
            } else if (lane == leader) {
                atomicAdd(&size[lb], peers);
            }
            left = left && !same;
        }
        if (left) atomicAdd(&size[b], 1);
    }
    if (carry > 0 && lane == 0) atomicAdd(&size[carry_id], carry);
}

__global__ void __launch_bounds__(256) tr_count_kernel(const int64_t* __restrict__ block, int64_t num_nodes, int64_t num_blocks,
                                                       const int64_t* __restrict__ train_idx, const int64_t* __restrict__ y, u64 n_elems,
                                                       int classes, int64_t ldy, int32_t* __restrict__ cnt, int32_t* __restrict__ bad) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_elems) return;
    const u64 i = e / (u64)classes;
    const int c = (int)(e - i * (u64)classes);
    const int64_t node = train_idx[i];
    if (node < 0 || node >= num_nodes) {
        if (c == 0 && bad != nullptr) atomicOr(bad, RGCN_TR_BAD_NODE);
        return;
    }
    const int64_t b = block[node];
    if (b < 0 || b >= num_blocks) return;      // (tr_size_kernel has set the bit)
    const int64_t v = y[(int64_t)i * ldy + c];
    if (v != 0) atomicAdd(&cnt[b * (int64_t)classes + c], (int32_t)v);
}

__global__ void __launch_bounds__(256) tr_finish_kernel(const int32_t* __restrict__ cnt, const int32_t* __restrict__ size, u32 num_blocks,
                                                        int classes, float* __restrict__ y_sum, int64_t ld, int32_t* __restrict__ nonzero) {
    const u32 b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= num_blocks) return;
    const int32_t sz = size[b];
    const double div = (double)(sz > 1 ? sz : 1);
    const int32_t* row = cnt + (int64_t)b * classes;
    float* out = y_sum + (int64_t)b * ld;
    int64_t total = 0;
    for (int c = 0; c < classes; ++c) {
        const int32_t v = row[c];
        total += v;
        out[c] = (float)((double)v / div);
    }
    nonzero[b] = total != 0 ? 1 : 0;
}

// ---- gather --------------------------------------------------------------------------------------------------------------------
struct GatherArgs {
    const float* table[RGCN_TR_MAX_TABLES];
    const int64_t* map[RGCN_TR_MAX_TABLES];
    int64_t rows[RGCN_TR_MAX_TABLES];
    u64 key[RGCN_TR_MAX_TABLES];          // mix(seed + GOLDEN (s + 1))
    int ld[RGCN_TR_MAX_TABLES];
    const int64_t* nodes;                 // NULL: row j is node j
    float* out;
    int32_t* bad;                         // may be NULL
    int64_t num_nodes, ld_out, plane_stride;
    u64 n_out;
    int num_tables, width, width4, group, rows_per_wave;
    int vec;                              // 1: whole pieces move as 16 bytes
};

// the uniform draw of (table key, node, column): the top 24 bits of the mixed counter
__device__ __forceinline__ float tr_draw(u64 key, u64 node, int width, int col) {
    return (float)(u32)(mix(key + node * (u64)width + (u64)col) >> 40) * 0x1p-24f;
}

// NT: the whole table is written (no node list): gigabytes nobody reads back soon, stored non-temporally -- measured 3 to 21 % faster
// than plain stores at 0.26 to 7.7 GB (profiles/transfer_timing.txt).  The rows of a node list are read by the very next kernel and
// take plain stores (their time did not change with the hint).
template <bool NT>
__device__ __forceinline__ void store16(float* dst, f32x4 v) {
    if (NT)
        __builtin_nontemporal_store(v, (f32x4*)dst);
    else
        *(f32x4*)dst = v;
}

template <int MODE, bool NT>
__global__ void __launch_bounds__(256) tr_gather_kernel(const GatherArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int sub = lane / a.group;
    if (sub >= a.rows_per_wave) return;
    const u64 unit = wave * (u64)a.rows_per_wave + (u64)sub;
    if (unit >= a.n_out) return;
    // every lane left is one of a whole group: the group's first lane reads the ids
    const int piece0 = lane - sub * a.group, first = sub * a.group;
    int64_t node = 0;
    if (piece0 == 0) {
        node = a.nodes != nullptr ? a.nodes[unit] : (int64_t)unit;
        if (node < 0 || node >= a.num_nodes) {
            if (a.bad != nullptr) atomicOr(a.bad, RGCN_TR_BAD_NODE);
            node = -1;
        }
    }
    node = __shfl(node, first);
    for (int p = piece0; p < a.width4; p += a.group) {
        const int c0 = 4 * p;
        const bool whole = a.vec && c0 + 4 <= a.width;
        const int cend = c0 + 4 < a.width ? c0 + 4 : a.width;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < a.num_tables; ++s) {
            // -1: not mapped (a draw); -2: nothing to read (zeros)
            int64_t row = -2;
            if (piece0 == 0 && node >= 0) {
                row = a.map[s][node];
                if (row < -1 || row >= a.rows[s]) {
                    if (p == 0 && a.bad != nullptr) atomicOr(a.bad, RGCN_TR_BAD_MAP);
                    row = -2;
                }
            }
            row = __shfl(row, first);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row >= 0) {
                const float* src = a.table[s] + row * (int64_t)a.ld[s] + c0;
                if (whole) {
                    v = *(const f32x4*)src;
                } else {
                    for (int c = c0; c < cend; ++c) v[c - c0] = src[c - c0];
                }
            } else if (row == -1) {
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = tr_draw(a.key[s], (u64)node, a.width, c0 + c);
            }
            if (MODE == RGCN_TR_SUM) {
                acc += v;
            } else {
                float* dst = MODE == RGCN_TR_STACK ? a.out + (int64_t)s * a.plane_stride + (int64_t)unit * a.ld_out + c0
                                                   : a.out + (int64_t)unit * a.ld_out + (int64_t)s * a.width + c0;
                if (whole) {
                    store16<NT>(dst, v);
                } else {
                    for (int c = c0; c < cend; ++c) dst[c - c0] = v[c - c0];
                }
            }
        }
        if (MODE == RGCN_TR_SUM) {
            float* dst = a.out + (int64_t)unit * a.ld_out + c0;
            if (whole) {
                store16<NT>(dst, acc);
            } else {
                for (int c = c0; c < cend; ++c) dst[c - c0] = acc[c - c0];
            }
        }
    }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

static bool labels_args_ok(int64_t num_nodes, int64_t num_blocks, int64_t n_train, int classes) {
    return num_nodes >= 0 && num_blocks >= 1 && n_train >= 0 && classes >= 1;
}

static bool labels_sizes_ok(int64_t num_nodes, int64_t num_blocks, int64_t n_train, int classes) {
    return num_nodes <= kMaxCount && num_blocks <= kMaxCount && n_train <= kMaxCount && classes <= kMaxClasses &&
           (u64)n_train * (u64)classes <= kMaxCells && (u64)num_blocks * (u64)classes <= kMaxCells;
}

}  // namespace rgcn_tr

using namespace rgcn_tr;

extern "C" size_t rgcn_tr_block_labels_workspace_bytes(int64_t num_nodes, int64_t num_blocks, int64_t n_train, int classes) {
    if (!labels_args_ok(num_nodes, num_blocks, n_train, classes) || !labels_sizes_ok(num_nodes, num_blocks, n_train, classes)) return 0;
    Arena ar(nullptr);
    ar.take<int32_t>((size_t)num_blocks * (size_t)classes);
    return ar.bytes();
}

extern "C" int rgcn_tr_block_labels(const int64_t* block, int64_t num_nodes, int64_t num_blocks, const int64_t* train_idx,
                                    const int64_t* y, int64_t ldy, int64_t n_train, int classes, int32_t* size, float* y_sum, int64_t ld,
                                    int32_t* nonzero, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!size || !y_sum || !nonzero) return RGCN_ERR_NULL;
    if (num_nodes > 0 && !block) return RGCN_ERR_NULL;
    if (n_train > 0 && (!train_idx || !y)) return RGCN_ERR_NULL;
    if (!labels_args_ok(num_nodes, num_blocks, n_train, classes) || ld < classes || ldy < classes) return RGCN_ERR_ARG;
    if (!labels_sizes_ok(num_nodes, num_blocks, n_train, classes)) return RGCN_ERR_PLAN;
    Arena ar(workspace);
    int32_t* cnt = ar.take<int32_t>((size_t)num_blocks * (size_t)classes);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(size, 0, (size_t)num_blocks * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, (size_t)num_blocks * (size_t)classes * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    if (num_nodes > 0) {
        const u32 waves = (u32)((num_nodes + 64 * kSizeChunks - 1) / (64 * kSizeChunks));
        hipLaunchKernelGGL(tr_size_kernel, dim3((waves + 3) / 4), dim3(256), 0, s, block, (u32)num_nodes, num_blocks, size, bad);
    }
    const u64 n_elems = (u64)n_train * (u64)classes;
    if (n_elems > 0)
        hipLaunchKernelGGL(tr_count_kernel, dim3(grid_for(n_elems)), dim3(256), 0, s, block, num_nodes, num_blocks, train_idx, y, n_elems,
                           classes, ldy, cnt, bad);
    hipLaunchKernelGGL(tr_finish_kernel, dim3(grid_for((u64)num_blocks)), dim3(256), 0, s, cnt, size, (u32)num_blocks, classes, y_sum, ld,
                       nonzero);
    return (int)hipGetLastError();
}

extern "C" int rgcn_tr_gather(const float* const* tables, const int32_t* lds, const int64_t* rows, const int64_t* const* maps,
                              int num_tables, int width, int64_t num_nodes, const int64_t* nodes, int64_t n_out, int mode, int64_t seed,
                              float* out, int64_t ld_out, int64_t plane_stride, int32_t* bad, void* stream) {
    if (!tables || !lds || !rows || !maps) return RGCN_ERR_NULL;
    if (num_tables < 1 || num_tables > RGCN_TR_MAX_TABLES || width < 1 || num_nodes < 0 || n_out < 0 || seed < 0) return RGCN_ERR_ARG;
    if (mode != RGCN_TR_STACK && mode != RGCN_TR_CONCAT && mode != RGCN_TR_SUM) return RGCN_ERR_ARG;
    if (nodes == nullptr && n_out != num_nodes) return RGCN_ERR_ARG;
    for (int s = 0; s < num_tables; ++s) {
        if (rows[s] < 0) return RGCN_ERR_ARG;
        if (lds[s] < width) return RGCN_ERR_STRIDE;
        if ((rows[s] > 0 && !tables[s]) || (num_nodes > 0 && !maps[s])) return RGCN_ERR_NULL;
    }
    const int64_t row_floats = mode == RGCN_TR_CONCAT ? (int64_t)num_tables * width : (int64_t)width;
    if (ld_out < row_floats) return RGCN_ERR_STRIDE;
    if (mode == RGCN_TR_STACK && num_tables > 1 && plane_stride < n_out * ld_out) return RGCN_ERR_STRIDE;
    if (num_nodes > kMaxCount || n_out > kMaxCount) return RGCN_ERR_PLAN;
    if (n_out == 0) return RGCN_OK;
    if (!out) return RGCN_ERR_NULL;
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    GatherArgs a;
    bool vec = aligned16(out) && ld_out % 4 == 0 && (mode != RGCN_TR_STACK || num_tables == 1 || plane_stride % 4 == 0) &&
               (mode != RGCN_TR_CONCAT || width % 4 == 0);
    for (int s = 0; s < RGCN_TR_MAX_TABLES; ++s) {
        const bool used = s < num_tables;
        a.table[s] = used ? tables[s] : nullptr;
        a.map[s] = used ? maps[s] : nullptr;
        a.rows[s] = used ? rows[s] : 0;
        a.ld[s] = used ? lds[s] : 0;
        a.key[s] = mix((u64)seed + kGolden * (u64)(s + 1));
        if (used && (lds[s] % 4 != 0 || !aligned16(tables[s]))) vec = false;
    }
    a.nodes = nodes;
    a.out = out;
    a.bad = bad;
    a.num_nodes = num_nodes;
    a.ld_out = ld_out;
    a.plane_stride = plane_stride;
    a.n_out = (u64)n_out;
    a.num_tables = num_tables;
    a.width = width;
    a.width4 = (width + 3) / 4;
    a.group = a.width4 < 64 ? a.width4 : 64;
    a.rows_per_wave = 64 / a.group;
    a.vec = vec ? 1 : 0;
    const u64 waves = (a.n_out + (u64)a.rows_per_wave - 1) / (u64)a.rows_per_wave;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const bool nt = nodes == nullptr;
    auto kernel = mode == RGCN_TR_STACK    ? (nt ? tr_gather_kernel<RGCN_TR_STACK, true> : tr_gather_kernel<RGCN_TR_STACK, false>)
                  : mode == RGCN_TR_CONCAT ? (nt ? tr_gather_kernel<RGCN_TR_CONCAT, true> : tr_gather_kernel<RGCN_TR_CONCAT, false>)
                                           : (nt ? tr_gather_kernel<RGCN_TR_SUM, true> : tr_gather_kernel<RGCN_TR_SUM, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a);
    return (int)hipGetLastError();
}

// rgcn_minibatch.hip -- a bipartite R-GCN layer straight from a sampled block (sampling.Block), behind the C ABI rgcn_mb_* of
// include/rgcn_mi355x.h: one light index per block that serves forward, dX and d_weight; no TilePlan, no GraphPlans, no plan cache.
// gfx950 only.  DESIGN.md section 15 has the semantics.  ("block" in the C ABI already means block-diagonal weights: hence "mb".)
//
// The root term is relation R with one pseudo edge i -> i per destination (a block's destinations are its first n_dst source
// rows), so d_root and the root's part of dX fall out of the same kernels as the relations'.
//
// Index (rgcn_mb_index_build; integer work on rgcn_sort_scan.h), M = E_b + n_dst edges:
//   keys      (relation, destination) per edge, sources counted by integer atomics; ids out of range set an error bit
//   sort      one stable sort by (relation, destination): position p of the sorted list is what every array below refers to
//   runs      head flags + scan: runs of equal (relation, destination); a run's length is the mean's divisor
//   rows      a run is cut into rows of at most 256 consecutive positions; scale = 1 / run length (mean) or 1 (sum)
//   tiles     rows relation-major in tiles of 16 that never straddle a relation: tile_ptr[R + 2] by a scan of the per-relation
//             row counts (a search in the sorted keys, no counter); row slot = 16 * tile_ptr[rel] + (row - first row of rel);
//             the slots that pad a relation's last tile are empty
//   dst list  the row slots sorted stably by destination: ascending relation within a destination
//   src list  (row slot, scale) of every position, sorted stably by source
//   read      error bits, rows and tiles: the one copy and the one synchronisation of a build
//
// Layer:
//   mb_transform_kernel   one wave per tile.  Forward: a lane sums its row's source rows of x in index order, scales, stores the
//                         aggregated tile H (kept for d_weight) and multiplies by W_rel on v_mfma_f32_16x16x4_f32 (exact fp32; the
//                         fragments of rgcn_pack_weights come straight from L2: consecutive tiles share a relation) -> Z.
//                         Backward: the same tiles, A = g[destination of the row], operand W_rel^T -> dH.
//   mb_sum_kernel         out[i] = bias + sum of Z[row] over the rows of destination i / dx[s] = sum of scale_e dH[row_e] over the
//                         positions of source s: one lane group per output row, index order, no atomics
//   mb_dw_kernel          dW[rel] = H_rel^T g[destinations of rel's rows] on the same MFMA; a relation's tiles in S slabs (S fixed
//                         per launch), slabs added in slab order by mb_dw_reduce_kernel
// No float atomics anywhere: the same block and inputs give the same bits.
#include <initializer_list>
#include "rgcn_common.h"
#include "rgcn_launch.h"
#include "rgcn_sort_scan.h"

namespace rgcn_mb {

using namespace rgcn_sort_scan;
using rgcn::f32x4;

constexpr u32 kErrRange = 1u, kErrInternal = 2u;
constexpr int64_t kMaxRelations = 65536;
constexpr u32 kRowEdges = 256;               // most positions of one row
constexpr int kMaxSlabs = 64;
constexpr size_t kMaxSlabFloats = (size_t)1 << 24;      // 64 MiB of d_weight partials at the most

struct Results {        // device-resident scalars of one build: what the host reads back in one copy
    u32 error;          // kErr* bits
    u32 n_rows;         // rows (non-empty slots)
    u32 n_tiles;
    u32 reserved;
};

// ------------------------------------------------------------------------------------------------
// index
// ------------------------------------------------------------------------------------------------
// An id out of range sets the error bit and the key of (relation 0, destination 0, source 0): everything later stays inside
// its arrays whatever the input holds.  Edges E .. M-1 are the root's pseudo edges i -> i of relation R.
__global__ void mb_keys_kernel(const int64_t* __restrict__ src, int64_t src_stride, const int64_t* __restrict__ dst, int64_t dst_stride,
                               const int64_t* __restrict__ typ, int64_t typ_stride, u32 num_edges, u32 total, u32 n_src, u32 n_dst,
                               u32 num_rel, int dst_bits, u64* __restrict__ keys, u32* __restrict__ vals, u32* __restrict__ esrc,
                               u32* __restrict__ src_cnt, Results* __restrict__ res) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    u32 s, d, r;
    if (e < num_edges) {
        const int64_t sv = src[(u64)e * src_stride], dv = dst[(u64)e * dst_stride], t = typ[(u64)e * typ_stride];
        const bool bad = t < 0 || t >= (int64_t)num_rel || sv < 0 || sv >= (int64_t)n_src || dv < 0 || dv >= (int64_t)n_dst;
        if (bad) atomicOr(&res->error, kErrRange);
        s = bad ? 0u : (u32)sv;
        d = bad ? 0u : (u32)dv;
        r = bad ? 0u : (u32)t;
    } else {
        s = d = e - num_edges;
        r = num_rel;
    }
    keys[e] = ((u64)r << dst_bits) | (u64)d;
    vals[e] = e;
    esrc[e] = s;
    atomicAdd(&src_cnt[s], 1u);
}

// run_start[run] = first position of the run; run_start[number of runs] = total
__global__ void mb_run_start_kernel(const u32* __restrict__ flag, const u32* __restrict__ run_id, u32 total, u32* __restrict__ run_start) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    if (flag[p]) run_start[run_id[p]] = p;
    if (p == total - 1u) run_start[run_id[p] + 1u] = total;
}

// row heads: every 256th position of a run; counts rows per destination
__global__ void mb_row_flags_kernel(const u64* __restrict__ keys, const u32* __restrict__ run_id, const u32* __restrict__ run_start,
                                    u32 total, int dst_bits, u32* __restrict__ flag, u32* __restrict__ dst_cnt) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const bool head = ((p - run_start[run_id[p]]) & (kRowEdges - 1u)) == 0u;
    flag[p] = head ? 1u : 0u;
    if (head) atomicAdd(&dst_cnt[(u32)(keys[p] & ((1ull << dst_bits) - 1ull))], 1u);
}

// rows of the relations below `rel`: the row of the first sorted position whose relation is at least rel (such a position starts
// a run, hence a row); no atomics -- thousands of row heads of one relation would queue on one counter
__device__ inline u32 rows_below(const u64* __restrict__ keys, const u32* __restrict__ row_id, u32 total, int dst_bits, u32 rel) {
    u32 lo = 0, hi = total;      // first position in [0, total] with relation >= rel
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if ((u32)(keys[mid] >> dst_bits) < rel) lo = mid + 1u;
        else hi = mid;
    }
    return lo < total ? row_id[lo] : row_id[total - 1u] + 1u;
}

// one workgroup: rel_start = rows before every relation, tile_ptr = exclusive scan of the relations' tiles of 16
__global__ void mb_rel_scan_kernel(const u64* __restrict__ keys, const u32* __restrict__ row_id, u32 total, int dst_bits, u32 nrel,
                                   u32* __restrict__ rel_start, u32* __restrict__ tile_ptr, Results* __restrict__ res) {
    __shared__ u32 wt[kScanThreads / 64];
    u32 carry_t = 0;
    for (u32 c0 = 0; c0 < nrel; c0 += kScanThreads) {
        const u32 i = c0 + threadIdx.x;
        const u32 b = i < nrel ? rows_below(keys, row_id, total, dst_bits, i) : 0u;
        const u32 c = i < nrel ? rows_below(keys, row_id, total, dst_bits, i + 1u) - b : 0u;
        const u32 t = (c + 15u) >> 4;
        u32 tot_t;
        const u32 ex_t = block_exclusive_scan(t, wt, tot_t);
        if (i < nrel) {
            rel_start[i] = b;
            tile_ptr[i] = carry_t + ex_t;
        }
        carry_t += tot_t;
    }
    if (threadIdx.x == 0) {
        tile_ptr[nrel] = carry_t;
        res->n_rows = row_id[total - 1u] + 1u;
        res->n_tiles = carry_t;
    }
}

struct FillArgs {
    const u64* keys;          // sorted
    const u32* vals;          // sorted: the edge of a position
    const u32* run_id;
    const u32* run_start;
    const u32* row_id;        // the row of a position, counted over the whole sorted list
    const u32* rel_start;
    const u32* tile_ptr;
    const u32* esrc;
    u32* row_beg;
    u32* row_cnt;
    u32* row_dst;
    float* row_scale;
    u32* edge_src;
    u32* pos_slot;
    float* pos_scale;
    u32* row_slot;            // row -> slot
    Results* res;
    u32 total, rows_cap;
    int dst_bits, mean;
};

__global__ void mb_fill_kernel(const FillArgs a) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.total) return;
    const u64 k = a.keys[p];
    const u32 rel = (u32)(k >> a.dst_bits), dst = (u32)(k & ((1ull << a.dst_bits) - 1ull));
    const u32 run = a.run_id[p], rs = a.run_start[run], len = a.run_start[run + 1u] - rs;
    const u32 row = a.row_id[p];
    const u64 slot64 = (u64)a.tile_ptr[rel] * 16ull + (u64)(row - a.rel_start[rel]);
    a.edge_src[p] = a.esrc[a.vals[p]];
    if (slot64 >= (u64)a.rows_cap) {      // (cannot happen: the tiles of R + 1 relations hold at most M / 16 + R + 1 of them)
        atomicOr(&a.res->error, kErrInternal);
        a.pos_slot[p] = 0u;
        a.pos_scale[p] = 0.f;
        return;
    }
    const u32 slot = (u32)slot64;
    const float scale = a.mean ? __fdiv_rn(1.f, (float)len) : 1.f;
    a.pos_slot[p] = slot;
    a.pos_scale[p] = scale;
    const u32 off = p - rs;
    if ((off & (kRowEdges - 1u)) == 0u) {
        a.row_beg[slot] = p;
        a.row_cnt[slot] = len - off < kRowEdges ? len - off : kRowEdges;
        a.row_dst[slot] = dst;
        a.row_scale[slot] = scale;
        a.row_slot[row] = slot;
    }
}

// the second sort's pairs: (destination, slot) of every row in relation-major order; entries past the rows sort behind them
__global__ void mb_dst_pairs_kernel(const u32* __restrict__ row_slot, const u32* __restrict__ row_dst, const Results* __restrict__ res,
                                    u32 total, u32 n_dst, u64* __restrict__ keys, u32* __restrict__ vals) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const bool live = j < res->n_rows;
    const u32 slot = live ? row_slot[j] : 0u;
    keys[j] = live ? (u64)row_dst[slot] : (u64)n_dst;
    vals[j] = slot;
}

__global__ void mb_copy_kernel(const u32* __restrict__ in, u32 n, u32* __restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i];
}

__global__ void mb_src_pairs_kernel(const u32* __restrict__ edge_src, u32 total, u64* __restrict__ keys, u32* __restrict__ vals) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    keys[p] = (u64)edge_src[p];
    vals[p] = p;
}

__global__ void mb_src_list_kernel(const u32* __restrict__ vals, const u32* __restrict__ pos_slot, const float* __restrict__ pos_scale,
                                   u32 total, u32* __restrict__ src_row, float* __restrict__ src_scale) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const u32 p = vals[q];
    src_row[q] = pos_slot[p];
    src_scale[q] = pos_scale[p];
}

struct Sizes {
    u64 total;         // M = E_b + n_dst
    u64 rows_cap;      // slots the row arrays hold: 16 * (M / 16 + R + 1)
};

static int check_sizes(int64_t num_edges, int64_t n_src, int64_t n_dst, int64_t num_rel, Sizes* sz) {
    if (num_edges < 0 || n_src < 0 || n_dst < 0 || n_dst > n_src) return RGCN_ERR_ARG;
    if (num_rel <= 0 || num_rel > kMaxRelations || n_src >= (1ll << 31) || n_dst >= (1ll << 31)) return RGCN_ERR_PLAN;
    if ((u64)num_edges > kMaxKeys || (u64)num_edges + (u64)n_dst > kMaxKeys) return RGCN_ERR_PLAN;
    sz->total = (u64)num_edges + (u64)n_dst;
    sz->rows_cap = 16ull * (sz->total / 16ull + (u64)num_rel + 1ull);
    if (sz->rows_cap > 0xFFFFFFFFull) return RGCN_ERR_PLAN;      // slots are 32-bit
    return RGCN_OK;
}

struct IndexArrays {
    u32 *tile_ptr, *row_beg, *row_cnt, *row_dst;
    float* row_scale;
    u32 *edge_src, *dst_ptr, *dst_rows, *src_ptr, *src_row;
    float* src_scale;
    size_t bytes;
};

static IndexArrays carve_arrays(void* base, const Sizes& sz, u64 n_src, u64 n_dst, u64 num_rel) {
    IndexArrays w;
    Arena ar(base);
    w.tile_ptr = ar.take<u32>(num_rel + 2);
    w.row_beg = ar.take<u32>(sz.rows_cap);
    w.row_cnt = ar.take<u32>(sz.rows_cap);
    w.row_dst = ar.take<u32>(sz.rows_cap);
    w.row_scale = ar.take<float>(sz.rows_cap);
    w.edge_src = ar.take<u32>(sz.total);
    w.dst_ptr = ar.take<u32>(n_dst + 1);
    w.dst_rows = ar.take<u32>(sz.total);
    w.src_ptr = ar.take<u32>(n_src + 1);
    w.src_row = ar.take<u32>(sz.total);
    w.src_scale = ar.take<float>(sz.total);
    w.bytes = ar.bytes();
    return w;
}

struct BuildWorkspace {
    Results* res;
    SortBufs sb;
    u32 *flag, *run_id, *run_start, *row_id, *esrc, *pos_slot, *row_slot, *rel_start;
    float* pos_scale;
    size_t bytes;
};

static BuildWorkspace carve_build(void* base, const Sizes& sz, u64 n_src, u64 n_dst, u64 num_rel) {
    BuildWorkspace w;
    Arena ar(base);
    const u64 m = sz.total;
    w.res = ar.take<Results>(1);
    u64 scan_len = m;
    if (n_src + 1 > scan_len) scan_len = n_src + 1;
    if (n_dst + 1 > scan_len) scan_len = n_dst + 1;
    w.sb = take_sort_bufs(ar, m, scan_len);
    w.flag = ar.take<u32>(m);
    w.run_id = ar.take<u32>(m);
    w.run_start = ar.take<u32>(m + 1);
    w.row_id = ar.take<u32>(m);
    w.esrc = ar.take<u32>(m);
    w.pos_slot = ar.take<u32>(m);
    w.pos_scale = ar.take<float>(m);
    w.row_slot = ar.take<u32>(m);
    w.rel_start = ar.take<u32>(num_rel + 2);
    w.bytes = ar.bytes();
    return w;
}

// ------------------------------------------------------------------------------------------------
// layer
// ------------------------------------------------------------------------------------------------
struct TransformArgs {
    const u32* tile_ptr;
    const u32* row_beg;
    const u32* row_cnt;
    const u32* row_dst;
    const float* row_scale;
    const u32* edge_src;
    const float* x;        // forward: the layer input [n_src][ldx]; backward: g [n_dst][ldx]
    const float* wp;       // rgcn_pack_weights: fp32 MFMA fragment order, relation R = the root
    float* h;              // forward: the aggregated rows [16 n_tiles][ldh]; backward: unused
    float* z;              // [16 n_tiles][ldz]
    u32 nrel, n_tiles;     // nrel = R + 1
    int ldx, k4, ldh, ldz, n4;      // k4 / n4: 16-byte pieces of a gathered row / of a stored row
};

// One wave per tile of 16 rows.  A lane holds columns 16 j + 4 kq .. + 3 of row (lane & 15): the B operand of Z^T = W^T H^T, so
// that it ends with four consecutive columns of its row (csrc/rgcn_ep.hip).
template <int KP, int NP, bool BWD>
__global__ void __launch_bounds__(256) mb_transform_kernel(const TransformArgs a) {
    constexpr int KT = KP / 16, NT = NP / 16;
    const int lane = threadIdx.x & 63;
    const u32 tile = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)));
    if (tile >= a.n_tiles) return;
    // the relation of the tile: the last r with tile_ptr[r] <= tile (tile_ptr[nrel] = n_tiles > tile)
    u32 lo = 0, hi = a.nrel;
    while (hi - lo > 1u) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (a.tile_ptr[mid] <= tile) lo = mid;
        else hi = mid;
    }
    const u32 rel = lo;
    const int row = lane & 15, kq = lane >> 4;
    const size_t slot = (size_t)tile * 16 + row;
    const u32 cnt = a.row_cnt[slot];
    f32x4 cur[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) cur[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (!BWD) {
        const u32* es = a.edge_src + a.row_beg[slot];
        u32 q = 0;
        for (; q + 2 <= cnt; q += 2) {      // two rows in flight, added in index order
            const float* r0 = a.x + (size_t)es[q] * a.ldx + 4 * kq;
            const float* r1 = a.x + (size_t)es[q + 1] * a.ldx + 4 * kq;
            f32x4 v0[KT], v1[KT];
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                v0[j] = v1[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (4 * j + kq < a.k4) {
                    v0[j] = *(const f32x4*)(r0 + 16 * j);
                    v1[j] = *(const f32x4*)(r1 + 16 * j);
                }
            }
#pragma unroll
            for (int j = 0; j < KT; ++j) cur[j] = (cur[j] + v0[j]) + v1[j];
        }
        if (q < cnt) {
            const float* r0 = a.x + (size_t)es[q] * a.ldx + 4 * kq;
#pragma unroll
            for (int j = 0; j < KT; ++j)
                if (4 * j + kq < a.k4) cur[j] += *(const f32x4*)(r0 + 16 * j);
        }
        const float sc = a.row_scale[slot];
        float* hr = a.h + slot * (size_t)a.ldh + 4 * kq;
#pragma unroll
        for (int j = 0; j < KT; ++j) {
            cur[j] *= sc;
            if (4 * j + kq < a.k4) *(f32x4*)(hr + 16 * j) = cur[j];
        }
    } else if (cnt != 0u) {
        const float* r0 = a.x + (size_t)a.row_dst[slot] * a.ldx + 4 * kq;
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (4 * j + kq < a.k4) cur[j] = *(const f32x4*)(r0 + 16 * j);
    }
    const f32x4* wp4 = (const f32x4*)a.wp + lane;
    f32x4 acc[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < KT; ++j)
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const f32x4 b4 = wp4[((size_t)(rel * NT + s) * KT + j) * 64];
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[tt], cur[j][tt], acc[s], 0, 0, 0);
        }
    float* zr = a.z + slot * (size_t)a.ldz + 4 * kq;
#pragma unroll
    for (int s = 0; s < NT; ++s)
        if (4 * s + kq < a.n4) *(f32x4*)(zr + 16 * s) = acc[s];
}

// out[i][c] = bias[c] + sum over q in [ptr[i], ptr[i + 1]) of w[q] * in[idx[q]][c] (w == NULL: 1): G lanes per output row (one
// 16-byte piece each), 64 / G rows per wave; the rows are added in index order, four in flight.
struct SumArgs {
    const float* in;
    const u32* ptr;
    const u32* idx;
    const float* w;
    const float* bias;
    float* out;
    int ldin, ldo, width, width4;
    u32 n_out;
};

template <int G>
__global__ void __launch_bounds__(256) mb_sum_kernel(const SumArgs a) {
    constexpr int SPW = 64 / G;
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const u64 seg = wave * SPW + lane / G;
    const int piece = lane % G;
    if (seg >= a.n_out || piece >= a.width4) return;
    const u32 q0 = a.ptr[seg], q1 = a.ptr[seg + 1];
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    auto rowv = [&](u32 q) {
        const f32x4 v = *(const f32x4*)(a.in + (size_t)a.idx[q] * a.ldin + 4 * piece);
        return a.w != nullptr ? v * a.w[q] : v;
    };
    u32 q = q0;
    for (; q + 4 <= q1; q += 4) {
        const f32x4 v0 = rowv(q), v1 = rowv(q + 1), v2 = rowv(q + 2), v3 = rowv(q + 3);
        s = (((s + v0) + v1) + v2) + v3;
    }
    for (; q < q1; ++q) s += rowv(q);
    if (a.bias != nullptr) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * piece + c < a.width) s[c] += a.bias[4 * piece + c];
    }
    *(f32x4*)(a.out + (size_t)seg * a.ldo + 4 * piece) = s;
}

static int launch_sum(const SumArgs& a, hipStream_t s) {
    return rgcn::launch_row_groups(a.width4, a.n_out, [&](auto g, dim3 grid) {
        hipLaunchKernelGGL(mb_sum_kernel<decltype(g)::value>, grid, dim3(256), 0, s, a);
        return (int)hipGetLastError();
    });
}

template <bool BWD>
static int launch_transform(int KP, int NP, const TransformArgs& a, hipStream_t s) {
    const dim3 grid((a.n_tiles + 3u) / 4u), block(256);
    return rgcn::for_padded_width(KP, [&](auto kp) {
        return rgcn::for_padded_width(NP, [&](auto np) {
            hipLaunchKernelGGL((mb_transform_kernel<decltype(kp)::value, decltype(np)::value, BWD>), grid, block, 0, s, a);
            return (int)hipGetLastError();
        });
    });
}

// d_weight.  Workgroup (relation, slab): its four waves share the row tiles of the slab and split the 16 x 16 tiles of the
// [in, out] result (tile o of wave o % 4); a row tile is four MFMA steps of four rows, A = H^T, B = g[destination].
struct DwArgs {
    const u32* tile_ptr;
    const u32* row_cnt;
    const u32* row_dst;
    const float* h;
    const float* g;
    float* part;       // slabs > 1: [R + 1][slabs][din * dout]
    float* d_weight;   // [R][din][dout] or NULL
    float* d_root;     // [din][dout] or NULL
    u32 nrel;          // R + 1
    int slabs, ldh, ldg, din, dout, din4, dout4;
};

template <int KP, int NP>
__global__ void __launch_bounds__(256) mb_dw_kernel(const DwArgs a) {
    constexpr int KT = KP / 16, NT = NP / 16, OT = KT * NT, OPW = (OT + 3) / 4;
    const u32 rel = blockIdx.x / (u32)a.slabs, slab = blockIdx.x % (u32)a.slabs;
    float* own = rel + 1u < a.nrel ? (a.d_weight ? a.d_weight + (size_t)rel * a.din * a.dout : nullptr) : a.d_root;
    if (own == nullptr) return;
    float* dest = a.slabs > 1 ? a.part + ((size_t)rel * a.slabs + slab) * a.din * a.dout : own;
    const u32 t0 = a.tile_ptr[rel], t1 = a.tile_ptr[rel + 1];
    const u32 per = (t1 - t0 + (u32)a.slabs - 1u) / (u32)a.slabs;
    const u32 tb = t0 + slab * per < t1 ? t0 + slab * per : t1;
    const u32 te = tb + per < t1 ? tb + per : t1;
    const int lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    f32x4 acc[OPW];
#pragma unroll
    for (int oi = 0; oi < OPW; ++oi) acc[oi] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (u32 t = tb; t < te; ++t) {
#pragma unroll
        for (int step = 0; step < 4; ++step) {
            const size_t slot = (size_t)t * 16 + 4 * step + kq;
            const bool live = a.row_cnt[slot] != 0u;
            const float* hr = a.h + slot * (size_t)a.ldh;
            const float* gr = a.g + (size_t)a.row_dst[slot] * a.ldg;
#pragma unroll
            for (int oi = 0; oi < OPW; ++oi) {
                const int o = 4 * oi + wave;
                if (o < OT) {
                    const int kc = 16 * (o / NT) + m, nc = 16 * (o % NT) + m;
                    const float av = (live && kc < 4 * a.din4) ? hr[kc] : 0.f;
                    const float bv = (live && nc < 4 * a.dout4) ? gr[nc] : 0.f;
                    acc[oi] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[oi], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int oi = 0; oi < OPW; ++oi) {
        const int o = 4 * oi + wave;
        if (o < OT) {
            const int n = 16 * (o % NT) + m;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = 16 * (o / NT) + 4 * kq + i;
                if (k < a.din && n < a.dout) dest[(size_t)k * a.dout + n] = acc[oi][i];
            }
        }
    }
}

// d_W[rel] = the slabs' partial results added in slab order
__global__ void mb_dw_reduce_kernel(const DwArgs a) {
    const size_t per = (size_t)a.din * a.dout, total = (size_t)a.nrel * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const u32 rel = (u32)(i / per);
        const size_t e = i - (size_t)rel * per;
        float* own = rel + 1u < a.nrel ? (a.d_weight ? a.d_weight + (size_t)rel * per : nullptr) : a.d_root;
        if (own == nullptr) continue;
        const float* p = a.part + (size_t)rel * a.slabs * per + e;
        float v = 0.f;
        for (int s = 0; s < a.slabs; ++s) v += p[(size_t)s * per];
        own[e] = v;
    }
}

// slabs per relation of a d_weight launch: about eight tiles per workgroup, at most 64, the partials at most 64 MiB
static int dw_slabs(int64_t n_tiles, int64_t nrel, int din, int dout) {
    int64_t s = (n_tiles + 8 * nrel - 1) / (8 * nrel);
    const int64_t room = (int64_t)(kMaxSlabFloats / ((size_t)nrel * din * dout));
    if (s > room) s = room;
    if (s > kMaxSlabs) s = kMaxSlabs;
    return s < 1 ? 1 : (int)s;
}

static int check_index(const rgcn_mb_index_t* ix) {
    if (ix == nullptr) return RGCN_ERR_NULL;
    Sizes sz;
    const int st = check_sizes(ix->num_edges, ix->n_src, ix->n_dst, ix->num_relations, &sz);
    if (st != RGCN_OK) return st;
    if (ix->n_tiles < 0 || ix->n_rows < 0 || (u64)ix->n_tiles * 16ull > sz.rows_cap || ix->n_rows > (int64_t)ix->n_tiles * 16) return RGCN_ERR_PLAN;
    if (!ix->tile_ptr || !ix->src_ptr || !ix->dst_ptr) return RGCN_ERR_NULL;
    if (ix->n_tiles > 0 && (!ix->row_beg || !ix->row_cnt || !ix->row_dst || !ix->row_scale || !ix->edge_src || !ix->dst_rows ||
                            !ix->src_row || !ix->src_scale))
        return RGCN_ERR_NULL;
    return RGCN_OK;
}

// what the three layer entries check first, in this order: the index, the widths, then every (leading dimension, width) pair
struct Stride {
    int ld, width;
};
static int check_layer(const rgcn_mb_index_t* ix, int din, int dout, std::initializer_list<Stride> strides) {
    int st = check_index(ix);
    if (st != RGCN_OK) return st;
    if (din < 1 || din > RGCN_MAX_WIDTH || dout < 1 || dout > RGCN_MAX_WIDTH) return RGCN_ERR_PLAN;
    for (const Stride& t : strides)
        if ((st = rgcn::check_stride(t.ld, t.width)) != RGCN_OK) return st;
    return RGCN_OK;
}

// the fields of TransformArgs that come from the index: the same for both directions
static TransformArgs transform_args(const rgcn_mb_index_t* ix) {
    TransformArgs a;
    a.tile_ptr = (const u32*)ix->tile_ptr;
    a.row_beg = ix->row_beg;
    a.row_cnt = (const u32*)ix->row_cnt;
    a.row_dst = (const u32*)ix->row_dst;
    a.row_scale = ix->row_scale;
    a.edge_src = (const u32*)ix->edge_src;
    a.nrel = (u32)ix->num_relations + 1u;
    a.n_tiles = (u32)ix->n_tiles;
    return a;
}

}  // namespace rgcn_mb

using namespace rgcn_mb;

extern "C" size_t rgcn_mb_index_bytes(int64_t num_edges, int64_t n_src, int64_t n_dst, int32_t num_relations) {
    Sizes sz;
    if (check_sizes(num_edges, n_src, n_dst, num_relations, &sz) != RGCN_OK) return 0;
    return carve_arrays(nullptr, sz, (u64)n_src, (u64)n_dst, (u64)num_relations).bytes;
}

extern "C" size_t rgcn_mb_index_workspace_bytes(int64_t num_edges, int64_t n_src, int64_t n_dst, int32_t num_relations) {
    Sizes sz;
    if (check_sizes(num_edges, n_src, n_dst, num_relations, &sz) != RGCN_OK) return 0;
    return carve_build(nullptr, sz, (u64)n_src, (u64)n_dst, (u64)num_relations).bytes;
}

extern "C" int rgcn_mb_index_build(const int64_t* src, int64_t src_stride, const int64_t* dst, int64_t dst_stride, const int64_t* type,
                                   int64_t type_stride, int64_t num_edges, int64_t n_src, int64_t n_dst, int32_t num_relations,
                                   int mean, void* index_mem, size_t index_bytes, void* workspace, size_t workspace_bytes,
                                   rgcn_mb_index_t* index_out, void* stream) {
    if (index_out == nullptr) return RGCN_ERR_NULL;
    Sizes sz;
    int st = check_sizes(num_edges, n_src, n_dst, num_relations, &sz);
    if (st != RGCN_OK) return st;
    if (num_edges > 0 && (!src || !dst || !type)) return RGCN_ERR_NULL;
    if (!index_mem || !workspace) return RGCN_ERR_NULL;
    const u32 E = (u32)num_edges, M = (u32)sz.total, ns = (u32)n_src, nd = (u32)n_dst, R = (u32)num_relations;
    const IndexArrays ia = carve_arrays(index_mem, sz, ns, nd, R);
    BuildWorkspace ws = carve_build(workspace, sz, ns, nd, R);
    if (index_bytes < ia.bytes || workspace_bytes < ws.bytes) return RGCN_ERR_WORKSPACE;
    if (nd == 0 && E > 0) return RGCN_ERR_GRAPH;      // (no destination: every edge's destination is out of range)
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    rgcn_mb_index_t ix;
    ix.tile_ptr = (const int32_t*)ia.tile_ptr;
    ix.row_beg = ia.row_beg;
    ix.row_cnt = (const int32_t*)ia.row_cnt;
    ix.row_dst = (const int32_t*)ia.row_dst;
    ix.row_scale = ia.row_scale;
    ix.edge_src = (const int32_t*)ia.edge_src;
    ix.dst_ptr = ia.dst_ptr;
    ix.dst_rows = ia.dst_rows;
    ix.src_ptr = ia.src_ptr;
    ix.src_row = ia.src_row;
    ix.src_scale = ia.src_scale;
    ix.num_edges = num_edges;
    ix.n_rows = 0;
    ix.n_src = (int32_t)ns;
    ix.n_dst = (int32_t)nd;
    ix.num_relations = num_relations;
    ix.mean = mean ? 1 : 0;
    ix.n_tiles = 0;
    ix.reserved = 0;
    hipError_t e = hipMemsetAsync(ia.tile_ptr, 0, ((size_t)R + 2) * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(ia.src_ptr, 0, ((size_t)ns + 1) * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(ia.dst_ptr, 0, ((size_t)nd + 1) * 4, s);
    if (e != hipSuccess) return (int)e;
    if (M == 0) {      // no destination, no edge: an index without rows
        *index_out = ix;
        return RGCN_OK;
    }
    e = hipMemsetAsync(ws.res, 0, sizeof(Results), s);
    // the four row arrays are one range of the arena (carve_arrays): empty slots read as (0, 0, 0, 0.f)
    if (e == hipSuccess) e = hipMemsetAsync(ia.row_beg, 0, (size_t)((char*)ia.edge_src - (char*)ia.row_beg), s);
    if (e != hipSuccess) return (int)e;
    const int db = bits_for(nd - 1u);
    const dim3 gm(grid_for(M)), blk(256);
    hipLaunchKernelGGL(mb_keys_kernel, gm, blk, 0, s, src, src_stride, dst, dst_stride, type, type_stride, E, M, ns, nd, R, db,
                       ws.sb.k[0], ws.sb.v[0], ws.esrc, ia.src_ptr, ws.res);
    const int c = radix_sort_pairs(ws.sb, M, bits_for((u64)R) + db, s);
    const u64* keys = ws.sb.k[c];
    run_ids(keys, M, 0, ws.flag, ws.run_id, ws.sb.sums, s);
    hipLaunchKernelGGL(mb_run_start_kernel, gm, blk, 0, s, ws.flag, ws.run_id, M, ws.run_start);
    hipLaunchKernelGGL(mb_row_flags_kernel, gm, blk, 0, s, keys, ws.run_id, ws.run_start, M, db, ws.flag, ia.dst_ptr);
    exclusive_scan(ws.flag, ws.row_id, M, ws.sb.sums, s);
    hipLaunchKernelGGL(run_ids_kernel, gm, blk, 0, s, ws.row_id, ws.flag, M);
    hipLaunchKernelGGL(mb_rel_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, keys, ws.row_id, M, db, R + 1u, ws.rel_start, ia.tile_ptr,
                       ws.res);
    FillArgs fa;
    fa.keys = keys;
    fa.vals = ws.sb.v[c];
    fa.run_id = ws.run_id;
    fa.run_start = ws.run_start;
    fa.row_id = ws.row_id;
    fa.rel_start = ws.rel_start;
    fa.tile_ptr = ia.tile_ptr;
    fa.esrc = ws.esrc;
    fa.row_beg = ia.row_beg;
    fa.row_cnt = ia.row_cnt;
    fa.row_dst = ia.row_dst;
    fa.row_scale = ia.row_scale;
    fa.edge_src = ia.edge_src;
    fa.pos_slot = ws.pos_slot;
    fa.pos_scale = ws.pos_scale;
    fa.row_slot = ws.row_slot;
    fa.res = ws.res;
    fa.total = M;
    fa.rows_cap = (u32)sz.rows_cap;
    fa.dst_bits = db;
    fa.mean = ix.mean;
    hipLaunchKernelGGL(mb_fill_kernel, gm, blk, 0, s, fa);
    // the later sorts start in the pair the first one did not end in (nothing reads the first sort's pairs after the fill)
    const SortBufs sb2 = from_pair(ws.sb, c ^ 1);
    hipLaunchKernelGGL(mb_dst_pairs_kernel, gm, blk, 0, s, ws.row_slot, ia.row_dst, ws.res, M, nd, sb2.k[0], sb2.v[0]);
    const int c2 = radix_sort_pairs(sb2, M, bits_for((u64)nd), s);
    hipLaunchKernelGGL(mb_copy_kernel, gm, blk, 0, s, sb2.v[c2], M, ia.dst_rows);
    exclusive_scan(ia.dst_ptr, ia.dst_ptr, nd + 1u, ws.sb.sums, s);
    hipLaunchKernelGGL(mb_src_pairs_kernel, gm, blk, 0, s, ia.edge_src, M, sb2.k[0], sb2.v[0]);
    const int c3 = radix_sort_pairs(sb2, M, bits_for((u64)ns - 1u), s);
    hipLaunchKernelGGL(mb_src_list_kernel, gm, blk, 0, s, sb2.v[c3], ws.pos_slot, ws.pos_scale, M, ia.src_row, ia.src_scale);
    exclusive_scan(ia.src_ptr, ia.src_ptr, ns + 1u, ws.sb.sums, s);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    Results r;
    if ((st = read_back(ws.res, &r, s)) != 0) return st;
    if (r.error & kErrRange) return RGCN_ERR_GRAPH;
    if (r.error & kErrInternal) return RGCN_ERR_PLAN;
    ix.n_rows = (int64_t)r.n_rows;
    ix.n_tiles = (int32_t)r.n_tiles;
    *index_out = ix;
    return RGCN_OK;
}

extern "C" int rgcn_mb_fwd(const rgcn_mb_index_t* index, const float* x, int ldx, int din, const float* packed_w, const float* bias,
                           float* h, int ldh, float* z, int ldz, float* out, int ldo, int dout, void* stream) {
    int st = check_layer(index, din, dout, {{ldx, din}, {ldh, din}, {ldz, dout}, {ldo, dout}});
    if (st != RGCN_OK) return st;
    if (index->n_dst == 0) return RGCN_OK;
    if (!x || !packed_w || !h || !z || !out) return RGCN_ERR_NULL;
    if (index->n_tiles <= 0) return RGCN_ERR_PLAN;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    TransformArgs a = transform_args(index);
    a.x = x;
    a.wp = packed_w;
    a.h = h;
    a.z = z;
    a.ldx = ldx;
    a.k4 = (din + 3) / 4;
    a.ldh = ldh;
    a.ldz = ldz;
    a.n4 = (dout + 3) / 4;
    if ((st = launch_transform<false>(rgcn::padded_width(din), rgcn::padded_width(dout), a, s)) != 0) return st;
    SumArgs sa;
    sa.in = z;
    sa.ptr = index->dst_ptr;
    sa.idx = index->dst_rows;
    sa.w = nullptr;
    sa.bias = bias;
    sa.out = out;
    sa.ldin = ldz;
    sa.ldo = ldo;
    sa.width = dout;
    sa.width4 = (dout + 3) / 4;
    sa.n_out = (u32)index->n_dst;
    return launch_sum(sa, s);
}

extern "C" int rgcn_mb_bwd_dx(const rgcn_mb_index_t* index, const float* g, int ldg, int dout, const float* packed_wt, float* dh,
                              int lddh, float* dx, int lddx, int din, void* stream) {
    int st = check_layer(index, din, dout, {{ldg, dout}, {lddh, din}, {lddx, din}});
    if (st != RGCN_OK) return st;
    if (index->n_src == 0) return RGCN_OK;
    if (!dx) return RGCN_ERR_NULL;
    if (index->n_tiles > 0 && (!g || !packed_wt || !dh)) return RGCN_ERR_NULL;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    if (index->n_tiles > 0) {
        TransformArgs a = transform_args(index);
        a.x = g;
        a.wp = packed_wt;
        a.h = nullptr;
        a.z = dh;
        a.ldx = ldg;
        a.k4 = (dout + 3) / 4;
        a.ldh = 0;
        a.ldz = lddh;
        a.n4 = (din + 3) / 4;
        if ((st = launch_transform<true>(rgcn::padded_width(dout), rgcn::padded_width(din), a, s)) != 0) return st;
    }
    // (without a destination the source lists are empty: src_ptr is all zeros and every row of dx a zero)
    SumArgs sa;
    sa.in = dh;
    sa.ptr = index->src_ptr;
    sa.idx = index->src_row;
    sa.w = index->src_scale;
    sa.bias = nullptr;
    sa.out = dx;
    sa.ldin = lddh;
    sa.ldo = lddx;
    sa.width = din;
    sa.width4 = (din + 3) / 4;
    sa.n_out = (u32)index->n_src;
    return launch_sum(sa, s);
}

extern "C" size_t rgcn_mb_bwd_dw_workspace_bytes(const rgcn_mb_index_t* index, int din, int dout) {
    if (check_index(index) != RGCN_OK || din < 1 || din > RGCN_MAX_WIDTH || dout < 1 || dout > RGCN_MAX_WIDTH) return 0;
    const int64_t nrel = (int64_t)index->num_relations + 1;
    const int slabs = dw_slabs(index->n_tiles, nrel, din, dout);
    return slabs > 1 ? (size_t)nrel * slabs * din * dout * sizeof(float) : 0;
}

extern "C" int rgcn_mb_bwd_dw(const rgcn_mb_index_t* index, const float* h, int ldh, int din, const float* g, int ldg, int dout,
                              float* d_weight, float* d_root, void* workspace, size_t workspace_bytes, void* stream) {
    int st = check_layer(index, din, dout, {{ldh, din}, {ldg, dout}});
    if (st != RGCN_OK) return st;
    if (!d_weight && !d_root) return RGCN_OK;
    if (index->n_tiles > 0 && (!h || !g)) return RGCN_ERR_NULL;
    const int64_t nrel = (int64_t)index->num_relations + 1;
    const int slabs = dw_slabs(index->n_tiles, nrel, din, dout);
    const size_t need = slabs > 1 ? (size_t)nrel * slabs * din * dout * sizeof(float) : 0;
    if (need > 0 && !workspace) return RGCN_ERR_NULL;
    if (workspace_bytes < need) return RGCN_ERR_WORKSPACE;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    DwArgs a;
    a.tile_ptr = (const u32*)index->tile_ptr;
    a.row_cnt = (const u32*)index->row_cnt;
    a.row_dst = (const u32*)index->row_dst;
    a.h = h;
    a.g = g;
    a.part = (float*)workspace;
    a.d_weight = d_weight;
    a.d_root = d_root;
    a.nrel = (u32)nrel;
    a.slabs = slabs;
    a.ldh = ldh;
    a.ldg = ldg;
    a.din = din;
    a.dout = dout;
    a.din4 = (din + 3) / 4;
    a.dout4 = (dout + 3) / 4;
    // (an index without tiles has tile_ptr all zeros: every workgroup stores its zeros)
    const dim3 grid(a.nrel * (u32)a.slabs), block(256);
    st = rgcn::for_padded_width(rgcn::padded_width(din), [&](auto kp) {
        return rgcn::for_padded_width(rgcn::padded_width(dout), [&](auto np) {
            hipLaunchKernelGGL((mb_dw_kernel<decltype(kp)::value, decltype(np)::value>), grid, block, 0, s, a);
            return (int)hipGetLastError();
        });
    });
    if (st != 0 || slabs == 1) return st;
    const size_t total = (size_t)nrel * din * dout;
    const unsigned blocks = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(mb_dw_reduce_kernel, dim3(blocks), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

// rgcn_lp_shared.h -- what the link-prediction decoders share (rgcn_linkpred.hip: DistMult; rgcn_kge.hip: ComplEx, TransE): the lane
// groups of a row, pad masking and id checks, the relation-chunk kernels of the backward (functions of the index and of partial rows,
// not of the decoder), the fp32-MFMA ranking pass behind a query image (lp_rank_body: sweep, targets, filter lists and the count
// reduction in ONE copy), and the host-side argument checks.  Moved here from rgcn_linkpred.hip unchanged, as `mix` moved to
// rgcn_sort_scan.h: rgcn_lp_* keeps its bits.  gfx950 only; everything has internal linkage (each including source gets its own
// copy of the kernels).  DESIGN.md sections 18 and 22.
#ifndef RGCN_LP_SHARED_H
#define RGCN_LP_SHARED_H

#include "rgcn_common.h"
#include "rgcn_launch.h"
#include "rgcn_sort_scan.h"

namespace rgcn_lp {

using namespace rgcn_sort_scan;
using rgcn::f32x4;

constexpr int kBadNode = 1, kBadRel = 2;     // bits of the `bad` word (RGCN_LP_BAD_*)
constexpr u32 kRelChunk = 256;               // triples per chunk of a relation's gradient

// lanes of a row, rows of a wave, the first step of the shuffle tree over a row's lanes
struct Group {
    int width, width4, lanes, per_wave, half;
};

static Group group_of(int width) {
    Group g;
    g.width = width;
    g.width4 = (width + 3) / 4;
    g.lanes = g.width4;
    g.per_wave = 64 / g.lanes;
    int p = 1;
    while (p < g.lanes) p <<= 1;
    g.half = p >> 1;
    return g;
}

__device__ __forceinline__ f32x4 mask_pad(f32x4 v, int c0, int width) {
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c0 + e >= width) v[e] = 0.f;
    return v;
}

__device__ __forceinline__ f32x4 piece(const float* base, int64_t row, int ld, int c0) {
    return *(const f32x4*)(base + row * (int64_t)ld + c0);
}

__device__ __forceinline__ int id_flags(int64_t s, int64_t r, int64_t o, int n, int nrel) {
    return ((s < 0 || s >= (int64_t)n || o < 0 || o >= (int64_t)n) ? kBadNode : 0) | ((r < 0 || r >= (int64_t)nrel) ? kBadRel : 0);
}

// ------------------------------------------------------------------------------------------------
// backward: what does not depend on the decoder
// ------------------------------------------------------------------------------------------------
struct BwdArgs {
    const float* z;
    const float* rel;
    const int64_t* s;
    const int64_t* r;
    const int64_t* o;
    const float* g;
    const u32* node_ptr;
    const u32* node_slot;
    const u32* rel_ptr;
    const u32* rel_triple;
    const u32* chunk_ptr;
    float* partial;         // [chunks][4 width4]
    float* dz;
    float* drel;
    u32 max_chunks;
    int num_nodes, num_relations, ldz, ldr, lddz, lddrel;
    Group gr;
};

// chunk_ptr[r] = chunks of kRelChunk triples of the relations before r; one workgroup
static __global__ void __launch_bounds__(kScanThreads) lp_chunk_ptr_kernel(const u32* __restrict__ rel_ptr, int num_relations, u32* __restrict__ chunk_ptr) {
    __shared__ u32 wt[kScanThreads / 64];
    const int per = (num_relations + kScanThreads - 1) / kScanThreads;
    const int r0 = threadIdx.x * per, r1 = r0 + per < num_relations ? r0 + per : num_relations;
    u32 mine = 0;
    for (int r = r0; r < r1; ++r) mine += (rel_ptr[r + 1] - rel_ptr[r] + kRelChunk - 1) / kRelChunk;
    u32 tot;
    u32 ex = block_exclusive_scan(mine, wt, tot);
    for (int r = r0; r < r1; ++r) {
        chunk_ptr[r] = ex;
        ex += (rel_ptr[r + 1] - rel_ptr[r] + kRelChunk - 1) / kRelChunk;
    }
    if (threadIdx.x == 0) chunk_ptr[num_relations] = tot;
}

// the chunk of kRelChunk triples that is unit `unit` of the relation-chunk launch: its relation's sorted range [beg, end)
__device__ __forceinline__ void lp_chunk_range(const BwdArgs& a, u32 unit, u32& beg, u32& end) {
    int lo = 0, hi = a.num_relations - 1;
    while (lo < hi) {                                    // the relation whose chunks hold `unit`
        const int mid = (lo + hi) >> 1;
        if (a.chunk_ptr[mid + 1] <= unit) lo = mid + 1; else hi = mid;
    }
    beg = a.rel_ptr[lo] + (unit - a.chunk_ptr[lo]) * kRelChunk;
    end = beg + kRelChunk < a.rel_ptr[lo + 1] ? beg + kRelChunk : a.rel_ptr[lo + 1];
}

// group 0 of a chunk's wave adds the lane groups' sums in the order 1, 2, .., U - 1 and stores the chunk's partial row
__device__ __forceinline__ void lp_chunk_store(const BwdArgs& a, u32 unit, f32x4 acc, int sub, int p) {
    for (int u = 1; u < a.gr.per_wave; ++u) {
        const int from = (p + u * a.gr.lanes) & 63;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float w = __shfl(acc[e], from);
            if (sub == 0) acc[e] += w;               // (the other groups keep what they summed: group 0 still has to read it)
        }
    }
    if (sub == 0) *(f32x4*)(a.partial + ((size_t)unit * a.gr.width4 + p) * 4) = acc;
}

static __global__ void __launch_bounds__(256) lp_drel_sum_kernel(const BwdArgs a) {
    const int lane = threadIdx.x & 63;
    const u32 wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int sub = lane / a.gr.lanes;
    if (sub >= a.gr.per_wave) return;
    const u32 r = wave * (u32)a.gr.per_wave + (u32)sub;
    if (r >= (u32)a.num_relations) return;
    const int p = lane - sub * a.gr.lanes, c0 = 4 * p;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const u32 end = a.chunk_ptr[r + 1];
    for (u32 c = a.chunk_ptr[r]; c < end; ++c) acc += *(const f32x4*)(a.partial + ((size_t)c * a.gr.width4 + p) * 4);
    *(f32x4*)(a.drel + (int64_t)r * a.lddrel + c0) = mask_pad(acc, c0, a.gr.width);
}

// ------------------------------------------------------------------------------------------------
// ranks on v_mfma_f32_16x16x4_f32
// ------------------------------------------------------------------------------------------------
constexpr int kRankThreads = 512;
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kRankQueries = 64;                 // query rows of a workgroup: four MFMA tiles
constexpr int kRankTiles = kRankQueries / 16;
constexpr int kRankBlocks = 1024;                // workgroups a launch aims at: four per CU

struct RankArgs {
    const float* z;
    const float* rel;
    const int64_t* a;
    const int64_t* r;
    const int64_t* e;
    const int64_t* fptr;       // NULL: raw ranks
    const int64_t* fidx;
    int64_t flen;
    float* tscore;             // [Q] (workspace): the targets' scores
    u64* greater;
    u64* equal;
    int64_t nq;
    int num_nodes, num_relations, width, ldz, ldr, k16;
};

// The MFMA's k index is permuted (a sum does not care): lane (rl, kq) holds the four consecutive columns 16 c + 4 kq + j of its
// row and feeds element j to step (c, j).  The query image in LDS is laid out for exactly that read: q4[(4 c + kq) * 64 + query]
// is the 16-byte piece 4 c + kq of a query row, so sixteen lanes read sixteen consecutive pieces (no bank conflict).
//
// lp_rank_rows: the B operand, the pieces of row `row` of z (row < 0: zeros); pad columns masked.
template <int KT>
__device__ __forceinline__ void lp_rank_rows(f32x4 (&zf)[KT], const RankArgs& a, int64_t row, int kq) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KT; ++c) {
        const int col = 16 * c + 4 * kq;
        zf[c] = (row >= 0 && col < a.width) ? mask_pad(piece(a.z, row, a.ldz, col), col, a.width) : zero;
    }
}

// lp_score_tile: THE score of the ranking pass.  acc[r] of lane (rl, kq) = score(query 16 qt + 4 kq + r, the row lane rl loaded).
// Every element of the tile is its own chain of MFMA steps over (c, j) in that order: the bits of a (query, entity) score depend on
// the two rows alone, not on where in a tile the pair sits or which rows share the tile.
template <int KT>
__device__ __forceinline__ f32x4 lp_score_tile(const f32x4* q4, int qt, int rl, int kq, const f32x4 (&zf)[KT], int k16) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < KT; ++c) {
        if (c < k16) {
            const f32x4 qa = q4[(4 * c + kq) * kRankQueries + 16 * qt + rl];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[j], zf[c][j], acc, 0, 0, 0);
        }
    }
    return acc;
}

__device__ __forceinline__ float pick4(const f32x4& v, int r) {
    const float lo = (r & 1) ? v[1] : v[0], hi = (r & 1) ? v[3] : v[2];
    return (r & 2) ? hi : lo;
}

// The body of a ranking kernel of kRankThreads threads.  `query(anchor, relation, col)` is the decoder's part: the 16-byte piece at
// column col of the query row of (anchor, relation), ids in range; the body masks its pad columns.  TARGETS: the workgroup scores its
// 64 queries' targets into a.tscore and ends.  Otherwise grid (query blocks, entity slices): the sweep over this slice's entity
// tiles, then the filter lists and the target's own count, dealt over the slices' waves.
template <int KT, bool TARGETS, class Query>
__device__ __forceinline__ void lp_rank_body(const RankArgs& a, Query query) {
    __shared__ f32x4 q4[KT * 4 * kRankQueries];
    __shared__ float ts_l[kRankQueries];
    __shared__ int ok_l[kRankQueries];
    __shared__ u32 cnt_l[2][kRankQueries];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kRankQueries;

    // the query rows, zero where the query is past the end or has an id out of range
    for (int i = tid; i < KT * 4 * kRankQueries; i += kRankThreads) {
        const int pc = i / kRankQueries, qi = i - pc * kRankQueries, col = 4 * pc;
        const int64_t q = q0 + qi;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < a.nq && col < a.width) {
            const int64_t an = a.a[q], rn = a.r[q], en = a.e[q];
            if (id_flags(an, rn, en, a.num_nodes, a.num_relations) == 0) v = mask_pad(query(an, rn, col), col, a.width);
        }
        q4[i] = v;
    }
    if (tid < kRankQueries) {
        const int64_t q = q0 + tid;
        const bool ok = q < a.nq && id_flags(a.a[q], a.r[q], a.e[q], a.num_nodes, a.num_relations) == 0;
        ok_l[tid] = ok ? 1 : 0;
        if (!TARGETS) ts_l[tid] = ok ? a.tscore[q] : __builtin_inff();      // +inf: nothing is greater, nothing equal
        cnt_l[0][tid] = 0;
        cnt_l[1][tid] = 0;
    }
    __syncthreads();

    f32x4 zf[KT];
    if (TARGETS) {
        if (wave < kRankTiles) {                 // wave = query tile; column rl of the tile is the target of query 16 wave + rl
            const int qi = 16 * wave + rl;
            lp_rank_rows(zf, a, ok_l[qi] ? a.e[q0 + qi] : (int64_t)-1, kq);
            const f32x4 acc = lp_score_tile(q4, wave, rl, kq, zf, a.k16);
            if (kq == (rl >> 2) && q0 + qi < a.nq) a.tscore[q0 + qi] = pick4(acc, rl & 3);      // the diagonal
        }
        return;
    }

    // ---- sweep: this slice's entity tiles, 16 rows per wave and step; counts per lane in integer registers
    float tg[kRankTiles][4];
    u32 cg[kRankTiles][4], ce[kRankTiles][4];
#pragma unroll
    for (int qt = 0; qt < kRankTiles; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            tg[qt][r] = ts_l[16 * qt + 4 * kq + r];
            cg[qt][r] = 0;
            ce[qt][r] = 0;
        }
    }
    const int64_t tiles = ((int64_t)a.num_nodes + 15) / 16;
    const int64_t step = (int64_t)gridDim.y * kRankWaves;
    for (int64_t t = (int64_t)blockIdx.y * kRankWaves + wave; t < tiles; t += step) {
        const int64_t row = t * 16 + rl;
        const bool valid = row < (int64_t)a.num_nodes;
        lp_rank_rows(zf, a, valid ? row : (int64_t)-1, kq);
#pragma unroll
        for (int qt = 0; qt < kRankTiles; ++qt) {
            const f32x4 acc = lp_score_tile(q4, qt, rl, kq, zf, a.k16);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                cg[qt][r] += (valid && acc[r] > tg[qt][r]) ? 1u : 0u;
                ce[qt][r] += (valid && acc[r] == tg[qt][r]) ? 1u : 0u;
            }
        }
    }
    // the sixteen lanes that share kq hold the counts of the same four queries per tile: add them, then the waves in LDS
#pragma unroll
    for (int qt = 0; qt < kRankTiles; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            u32 g = cg[qt][r], e = ce[qt][r];
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) {
                g += __shfl_xor(g, m);
                e += __shfl_xor(e, m);
            }
            if (rl == 0) {
                if (g) atomicAdd(&cnt_l[0][16 * qt + 4 * kq + r], g);
                if (e) atomicAdd(&cnt_l[1][16 * qt + 4 * kq + r], e);
            }
        }
    }
    __syncthreads();
    if (tid < kRankQueries && q0 + tid < a.nq) {
        if (cnt_l[0][tid]) atomicAdd(&a.greater[q0 + tid], (u64)cnt_l[0][tid]);
        if (cnt_l[1][tid]) atomicAdd(&a.equal[q0 + tid], (u64)cnt_l[1][tid]);
    }

    // ---- listed entities and the target itself: taken off again, scored by the same function on rows gathered by list.  An entry
    // that is the target is skipped (the target is taken off once, below); an entry out of range counts nothing.
    const int gw = (int)blockIdx.y * kRankWaves + wave, nw = (int)gridDim.y * kRankWaves;
    for (int qi = gw; qi < kRankQueries; qi += nw) {
        const int64_t q = q0 + qi;
        if (q >= a.nq) break;
        if (!ok_l[qi]) {                         // an id out of range: both counts -1 (the sweep counted nothing against +inf)
            if (lane == 0) {
                atomicAdd(&a.greater[q], ~0ull);
                atomicAdd(&a.equal[q], ~0ull);
            }
            continue;
        }
        const float ts = ts_l[qi];
        const int64_t target = a.e[q];
        u64 ng = 0, ne = (ts == ts) ? 1ull : 0ull;      // the target's own score equals itself in the sweep (unless it is a NaN)
        if (a.fptr != nullptr) {
            int64_t beg = a.fptr[q], end = a.fptr[q + 1];
            if (beg < 0) beg = 0;
            if (end > a.flen) end = a.flen;
            for (int64_t base = beg; base < end; base += 16) {
                int64_t id = -1;
                if (base + rl < end) id = a.fidx[base + rl];
                const bool ok = id >= 0 && id < (int64_t)a.num_nodes && id != target;
                lp_rank_rows(zf, a, ok ? id : (int64_t)-1, kq);
                const f32x4 acc = lp_score_tile(q4, qi >> 4, rl, kq, zf, a.k16);
                const float v = pick4(acc, qi & 3);
                const bool mine = ok && kq == ((qi & 15) >> 2);
                ng += (u64)__popcll(__ballot(mine && v > ts));
                ne += (u64)__popcll(__ballot(mine && v == ts));
            }
        }
        if (lane == 0) {
            if (ng) atomicAdd(&a.greater[q], (u64)0 - ng);
            if (ne) atomicAdd(&a.equal[q], (u64)0 - ne);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// host: the checks every entry point shares
// ------------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// z / rel and their strides, the conventions every entry point shares
static int check_tables(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations) {
    int st;
    if ((st = rgcn::check_stride(ldz, width)) != RGCN_OK) return st;
    if (rel != nullptr && (st = rgcn::check_stride(ldr, width)) != RGCN_OK) return st;
    if (!aligned16(z) || !aligned16(rel)) return RGCN_ERR_STRIDE;
    if (num_nodes < 0 || num_relations < 0) return RGCN_ERR_ARG;
    if (num_relations > 65536) return RGCN_ERR_PLAN;
    return RGCN_OK;
}

static bool triples_fit(int64_t n) { return n >= 0 && 2ull * (u64)n <= kMaxKeys; }

struct BwdBufs {
    u32* chunk_ptr;
    float* partial;
    u32 max_chunks;
};

static BwdBufs take_bwd_bufs(Arena& ar, int64_t n, int32_t num_relations, int width) {
    BwdBufs b;
    b.max_chunks = (u32)((u64)n / kRelChunk) + (u32)num_relations;
    b.chunk_ptr = ar.take<u32>((size_t)num_relations + 1);
    b.partial = ar.take<float>((size_t)b.max_chunks * (size_t)((width + 3) / 4) * 4);
    return b;
}

// grid.y of a ranking sweep whose waves take `rows_per_wave` entity rows a step, `waves` waves per workgroup
static int64_t rank_slices(int64_t qblocks, int32_t num_nodes, int rows_per_wave, int waves) {
    const int64_t tiles = ((int64_t)num_nodes + rows_per_wave - 1) / rows_per_wave;
    int64_t slices = (kRankBlocks + qblocks - 1) / qblocks;
    const int64_t most = (tiles + waves - 1) / waves;
    if (slices > most) slices = most;
    return slices < 1 ? 1 : slices;
}

}  // namespace rgcn_lp

#endif

// rgcn_linkpred.hip -- link prediction behind the C ABI rgcn_lp_* of include/rgcn_mi355x.h: the DistMult decoder (score, an index
// that makes its backward atomic-free, the backward), negative sampling and filtered ranking.  gfx950 only.  DESIGN.md section 18
// has the semantics and the summation orders.
//
//   z [N][ldz], rel [R][ldr] fp32, widths 1..128, strides multiples of 4 and at least the width (so a row's last 16-byte piece lies
//   inside the row), bases 16-byte aligned.  Pad columns are masked out of every sum, whatever they hold.
//
//   lp_score_kernel      a triple is G = ceil(width / 4) lanes of one wave (one 16-byte piece of each of the three rows per lane),
//                        64 / G triples per wave; the lane's four products are added as (p0 + p1) + (p2 + p3), the lanes by a
//                        shuffle tree.  Nothing of size T x E is written.
//   index build          2T (node, slot = 2t + side) pairs and T (relation, t) pairs, each sorted stably on rgcn_sort_scan.h; the
//                        pointers from an integer count and a scan.  A triple with an id out of range gets the key behind every row
//                        and is not counted: the backward never meets it.
//   lp_dz_kernel         a node is G lanes; it walks its slots in sorted (= position) order.  Every row is written.
//   lp_drel_*            a relation's triples in chunks of kRelChunk: one wave per chunk (its 64 / G lane groups take every
//                        (64 / G)-th triple, then the groups are added in order), then one lane group per relation adds the chunks
//                        in order.
//   lp_corrupt_kernel    counter-based: the draw of (i, j) is mix(mix(seed + GOLDEN (i + 1)) + RELMUL (j + 1)), nothing else.
//   lp_rank_kernel       64 query rows z[a] o rel[r] in LDS, entity rows streamed 16 per wave, a [16 queries x 16 entities] tile on
//                        v_mfma_f32_16x16x4_f32, compared with the targets' scores and counted in integers.  lp_score_tile is the
//                        ONE function that makes a tile: the sweep (consecutive rows), the targets (rows by index) and the filter
//                        lists (rows by list) all go through it, so a (query, entity) pair has the same bits wherever it is scored.
// No float atomics anywhere; integer atomics in the counts and the `bad` word.
#include "rgcn_common.h"
#include "rgcn_launch.h"
#include "rgcn_sort_scan.h"

namespace rgcn_lp {

using namespace rgcn_sort_scan;
using rgcn::f32x4;

constexpr int kBadNode = 1, kBadRel = 2;     // bits of the `bad` word (RGCN_LP_BAD_*)
constexpr u32 kRelChunk = 256;               // triples per chunk of a relation's gradient
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull, kNegMul = 0xD1B54A32D192ED03ull, kSideMul = 0x2545F4914F6CDD1Dull;

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
// a. score
// ------------------------------------------------------------------------------------------------
struct ScoreArgs {
    const float* z;
    const float* rel;
    const int64_t* s;
    const int64_t* r;
    const int64_t* o;
    float* score;
    int32_t* bad;
    u64 n;
    int num_nodes, num_relations, ldz, ldr;
    Group g;
};

__global__ void __launch_bounds__(256) lp_score_kernel(const ScoreArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int sub = lane / a.g.lanes;
    if (sub >= a.g.per_wave) return;
    const u64 t = wave * (u64)a.g.per_wave + (u64)sub;
    if (t >= a.n) return;
    // every lane left is one of a whole group
    const int p = lane - sub * a.g.lanes, c0 = 4 * p;
    const int64_t s = a.s[t], r = a.r[t], o = a.o[t];
    const int flags = id_flags(s, r, o, a.num_nodes, a.num_relations);
    float v = 0.f;
    if (flags == 0) {
        const f32x4 q = mask_pad(piece(a.z, s, a.ldz, c0) * piece(a.rel, r, a.ldr, c0) * piece(a.z, o, a.ldz, c0), c0, a.g.width);
        v = (q[0] + q[1]) + (q[2] + q[3]);
    } else if (p == 0 && a.bad != nullptr) {
        atomicOr(a.bad, flags);
    }
    for (int d = a.g.half; d >= 1; d >>= 1) {
        const float w = __shfl_down(v, d);
        if (p + d < a.g.lanes) v += w;
    }
    if (p == 0) a.score[t] = v;
}

// ------------------------------------------------------------------------------------------------
// b. index
// ------------------------------------------------------------------------------------------------
// NODE: one key per (triple, side), the node of that side; else one key per triple, its relation.  `limit` (N or R) is the key of a
// triple that has an id out of range: it sorts behind every row and is not counted.
template <bool NODE>
__global__ void lp_keys_kernel(const int64_t* __restrict__ s, const int64_t* __restrict__ r, const int64_t* __restrict__ o, u32 n_keys,
                               int num_nodes, int num_relations, u64* __restrict__ keys, u32* __restrict__ vals, u32* __restrict__ count,
                               int32_t* __restrict__ bad) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_keys) return;
    const u32 t = NODE ? (i >> 1) : i;
    const int64_t sv = s[t], rv = r[t], ov = o[t];
    const int flags = id_flags(sv, rv, ov, num_nodes, num_relations);
    u64 key = NODE ? (u64)num_nodes : (u64)num_relations;
    if (flags == 0) {
        key = NODE ? (u64)((i & 1u) ? ov : sv) : (u64)rv;
        atomicAdd(&count[key], 1u);
    } else if ((!NODE || (i & 1u) == 0) && bad != nullptr) {
        atomicOr(bad, flags);
    }
    keys[i] = key;
    vals[i] = i;
}

// chunk_ptr[r] = chunks of kRelChunk triples of the relations before r; one workgroup
__global__ void __launch_bounds__(kScanThreads) lp_chunk_ptr_kernel(const u32* __restrict__ rel_ptr, int num_relations, u32* __restrict__ chunk_ptr) {
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

// ------------------------------------------------------------------------------------------------
// c. backward
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

__global__ void __launch_bounds__(256) lp_dz_kernel(const BwdArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int sub = lane / a.gr.lanes;
    if (sub >= a.gr.per_wave) return;
    const u64 v = wave * (u64)a.gr.per_wave + (u64)sub;
    if (v >= (u64)a.num_nodes) return;
    const int c0 = 4 * (lane - sub * a.gr.lanes);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const u32 end = a.node_ptr[v + 1];
    for (u32 j = a.node_ptr[v]; j < end; ++j) {
        const u32 slot = a.node_slot[j], t = slot >> 1;
        const int64_t other = (slot & 1u) ? a.s[t] : a.o[t];
        acc += (a.g[t] * piece(a.rel, a.r[t], a.ldr, c0)) * piece(a.z, other, a.ldz, c0);
    }
    *(f32x4*)(a.dz + (int64_t)v * a.lddz + c0) = mask_pad(acc, c0, a.gr.width);      // the pad columns of the last piece: +0.0
}

// one wave per chunk: lane group u takes the chunk's triples u, u + U, u + 2U, .. in order (U = 64 / G groups), then the groups
// are added in order 0, 1, .., U - 1
__global__ void __launch_bounds__(256) lp_drel_chunk_kernel(const BwdArgs a) {
    const int lane = threadIdx.x & 63;
    const u32 unit = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (unit >= a.max_chunks || unit >= a.chunk_ptr[a.num_relations]) return;      // (wave-uniform)
    int lo = 0, hi = a.num_relations - 1;
    while (lo < hi) {                                    // the relation whose chunks hold `unit`
        const int mid = (lo + hi) >> 1;
        if (a.chunk_ptr[mid + 1] <= unit) lo = mid + 1; else hi = mid;
    }
    const u32 beg = a.rel_ptr[lo] + (unit - a.chunk_ptr[lo]) * kRelChunk;
    const u32 end = beg + kRelChunk < a.rel_ptr[lo + 1] ? beg + kRelChunk : a.rel_ptr[lo + 1];
    const int sub = lane / a.gr.lanes, p = lane - sub * a.gr.lanes, c0 = 4 * p;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (sub < a.gr.per_wave) {
        for (u32 j = beg + (u32)sub; j < end; j += (u32)a.gr.per_wave) {
            const u32 t = a.rel_triple[j];
            acc += (a.g[t] * piece(a.z, a.s[t], a.ldz, c0)) * piece(a.z, a.o[t], a.ldz, c0);
        }
    }
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

__global__ void __launch_bounds__(256) lp_drel_sum_kernel(const BwdArgs a) {
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
// d. negatives
// ------------------------------------------------------------------------------------------------
__global__ void lp_corrupt_kernel(const int64_t* __restrict__ s, const int64_t* __restrict__ r, const int64_t* __restrict__ o, u64 total,
                                  u32 k, u64 num_nodes, u64 seed, int64_t* __restrict__ so, int64_t* __restrict__ ro,
                                  int64_t* __restrict__ oo) {
    const u64 step = (u64)gridDim.x * blockDim.x;
    for (u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += step) {
        const u64 i = idx / k, j = idx - i * k;
        const u64 draw = mix(mix(seed + kGolden * (i + 1ull)) + kNegMul * (j + 1ull));
        const int64_t id = (int64_t)__umul64hi(draw, num_nodes);
        const bool object_side = (mix(draw + kSideMul) >> 63) != 0ull;
        so[idx] = object_side ? s[i] : id;
        ro[idx] = r[i];
        oo[idx] = object_side ? id : o[i];
    }
}

// ------------------------------------------------------------------------------------------------
// e. ranks
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

// TARGETS: the workgroup scores its 64 queries' targets into a.tscore and ends.  Otherwise grid (query blocks, entity slices): the
// sweep over this slice's entity tiles, then the filter lists and the target's own count, dealt over the slices' waves.
template <int KT, bool TARGETS>
__global__ void __launch_bounds__(kRankThreads) lp_rank_kernel(const RankArgs a) {
    __shared__ f32x4 q4[KT * 4 * kRankQueries];
    __shared__ float ts_l[kRankQueries];
    __shared__ int ok_l[kRankQueries];
    __shared__ u32 cnt_l[2][kRankQueries];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kRankQueries;

    // the query rows z[a] o rel[r], zero where the query is past the end or has an id out of range
    for (int i = tid; i < KT * 4 * kRankQueries; i += kRankThreads) {
        const int pc = i / kRankQueries, qi = i - pc * kRankQueries, col = 4 * pc;
        const int64_t q = q0 + qi;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < a.nq && col < a.width) {
            const int64_t an = a.a[q], rn = a.r[q], en = a.e[q];
            if (id_flags(an, rn, en, a.num_nodes, a.num_relations) == 0)
                v = mask_pad(piece(a.z, an, a.ldz, col) * piece(a.rel, rn, a.ldr, col), col, a.width);
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

}  // namespace rgcn_lp

using namespace rgcn_lp;

extern "C" int rgcn_lp_score(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                             const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, float* score, int32_t* bad,
                             void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_triples > 0 && (!s || !r || !o || !score)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if (n_triples < 0) return RGCN_ERR_ARG;
    if (!triples_fit(n_triples)) return RGCN_ERR_PLAN;
    if (n_triples == 0) return RGCN_OK;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    ScoreArgs a;
    a.z = z;
    a.rel = rel;
    a.s = s;
    a.r = r;
    a.o = o;
    a.score = score;
    a.bad = bad;
    a.n = (u64)n_triples;
    a.num_nodes = num_nodes;
    a.num_relations = num_relations;
    a.ldz = ldz;
    a.ldr = ldr;
    a.g = group_of(width);
    const u64 waves = (a.n + (u64)a.g.per_wave - 1) / (u64)a.g.per_wave;
    hipLaunchKernelGGL(lp_score_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_lp_index_workspace_bytes(int64_t n_triples, int32_t num_nodes, int32_t num_relations) {
    if (n_triples <= 0 || num_nodes < 0 || num_relations < 0 || num_relations > 65536 || !triples_fit(n_triples)) return 0;
    Arena ar(nullptr);
    const u64 longest = (u64)(num_nodes > num_relations ? num_nodes : num_relations) + 1;
    take_sort_bufs(ar, 2ull * (u64)n_triples, longest);
    return ar.bytes();
}

extern "C" int rgcn_lp_index_build(const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, int32_t num_nodes,
                                   int32_t num_relations, uint32_t* node_ptr, uint32_t* node_slot, uint32_t* rel_ptr,
                                   uint32_t* rel_triple, int32_t* bad, void* workspace, size_t workspace_bytes, void* stream) {
    if (!node_ptr && !rel_ptr) return RGCN_ERR_NULL;      // (one half may be left out: node_ptr NULL or rel_ptr NULL)
    if (n_triples > 0 && (!s || !r || !o || (node_ptr && !node_slot) || (rel_ptr && !rel_triple))) return RGCN_ERR_NULL;
    if (n_triples < 0 || num_nodes < 0 || num_relations < 0) return RGCN_ERR_ARG;
    if (num_relations > 65536 || !triples_fit(n_triples)) return RGCN_ERR_PLAN;
    if (n_triples == 0) return RGCN_OK;
    Arena ar(workspace);
    const u64 longest = (u64)(num_nodes > num_relations ? num_nodes : num_relations) + 1;
    const SortBufs sb = take_sort_bufs(ar, 2ull * (u64)n_triples, longest);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    hipStream_t q = (hipStream_t)stream;
    const u32 n2 = (u32)(2 * n_triples), n1 = (u32)n_triples;
    if (node_ptr) {      // 2T (node, slot) pairs
        (void)hipMemsetAsync(node_ptr, 0, sizeof(u32) * ((size_t)num_nodes + 1), q);
        hipLaunchKernelGGL(lp_keys_kernel<true>, dim3(grid_for(n2)), dim3(256), 0, q, s, r, o, n2, (int)num_nodes, (int)num_relations,
                           sb.k[0], sb.v[0], node_ptr, bad);
        const int c = radix_sort_pairs(sb, n2, bits_for((u64)num_nodes), q);
        (void)hipMemcpyAsync(node_slot, sb.v[c], sizeof(u32) * (size_t)n2, hipMemcpyDeviceToDevice, q);
        exclusive_scan(node_ptr, node_ptr, (u32)num_nodes + 1u, sb.sums, q);
    }
    if (rel_ptr) {       // T (relation, triple) pairs, in the same buffers
        (void)hipMemsetAsync(rel_ptr, 0, sizeof(u32) * ((size_t)num_relations + 1), q);
        hipLaunchKernelGGL(lp_keys_kernel<false>, dim3(grid_for(n1)), dim3(256), 0, q, s, r, o, n1, (int)num_nodes, (int)num_relations,
                           sb.k[0], sb.v[0], rel_ptr, node_ptr ? (int32_t*)nullptr : bad);
        const int c = radix_sort_pairs(sb, n1, bits_for((u64)num_relations), q);
        (void)hipMemcpyAsync(rel_triple, sb.v[c], sizeof(u32) * (size_t)n1, hipMemcpyDeviceToDevice, q);
        exclusive_scan(rel_ptr, rel_ptr, (u32)num_relations + 1u, sb.sums, q);
    }
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_lp_backward_workspace_bytes(int64_t n_triples, int32_t num_relations, int width) {
    if (n_triples <= 0 || num_relations < 0 || num_relations > 65536 || width < 1 || width > RGCN_MAX_WIDTH || !triples_fit(n_triples))
        return 0;
    Arena ar(nullptr);
    take_bwd_bufs(ar, n_triples, num_relations, width);
    return ar.bytes();
}

extern "C" int rgcn_lp_backward(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                                const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, const float* g,
                                const uint32_t* node_ptr, const uint32_t* node_slot, const uint32_t* rel_ptr, const uint32_t* rel_triple,
                                float* dz, int lddz, float* drel, int lddrel, void* workspace, size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_triples > 0 && (!s || !r || !o || !g)) return RGCN_ERR_NULL;
    if (n_triples > 0 && dz && (!node_ptr || !node_slot)) return RGCN_ERR_NULL;
    if (n_triples > 0 && drel && (!rel_ptr || !rel_triple)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if (dz && (st = rgcn::check_stride(lddz, width)) != RGCN_OK) return st;
    if (drel && (st = rgcn::check_stride(lddrel, width)) != RGCN_OK) return st;
    if (!aligned16(dz) || !aligned16(drel)) return RGCN_ERR_STRIDE;
    if (n_triples < 0) return RGCN_ERR_ARG;
    if (!triples_fit(n_triples)) return RGCN_ERR_PLAN;
    if (n_triples == 0 || (!dz && !drel)) return RGCN_OK;
    BwdBufs bb{};
    if (drel && num_relations > 0) {
        Arena ar(workspace);
        bb = take_bwd_bufs(ar, n_triples, num_relations, width);
        if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
        if (!workspace) return RGCN_ERR_NULL;
    }
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t q = (hipStream_t)stream;
    BwdArgs a;
    a.z = z;
    a.rel = rel;
    a.s = s;
    a.r = r;
    a.o = o;
    a.g = g;
    a.node_ptr = node_ptr;
    a.node_slot = node_slot;
    a.rel_ptr = rel_ptr;
    a.rel_triple = rel_triple;
    a.chunk_ptr = bb.chunk_ptr;
    a.partial = bb.partial;
    a.dz = dz;
    a.drel = drel;
    a.max_chunks = bb.max_chunks;
    a.num_nodes = num_nodes;
    a.num_relations = num_relations;
    a.ldz = ldz;
    a.ldr = ldr;
    a.lddz = lddz;
    a.lddrel = lddrel;
    a.gr = group_of(width);
    auto row_grid = [&](u64 rows) { return dim3((unsigned)(((rows + (u64)a.gr.per_wave - 1) / (u64)a.gr.per_wave + 3) / 4)); };
    if (dz && num_nodes > 0) hipLaunchKernelGGL(lp_dz_kernel, row_grid((u64)num_nodes), dim3(256), 0, q, a);
    if (drel && num_relations > 0) {
        hipLaunchKernelGGL(lp_chunk_ptr_kernel, dim3(1), dim3(kScanThreads), 0, q, rel_ptr, (int)num_relations, bb.chunk_ptr);
        hipLaunchKernelGGL(lp_drel_chunk_kernel, dim3((bb.max_chunks + 3) / 4), dim3(256), 0, q, a);
        hipLaunchKernelGGL(lp_drel_sum_kernel, row_grid((u64)num_relations), dim3(256), 0, q, a);
    }
    return (int)hipGetLastError();
}

extern "C" int rgcn_lp_corrupt(const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, int32_t num_nodes,
                               int32_t num_negatives, int64_t seed, int64_t* s_out, int64_t* r_out, int64_t* o_out, void* stream) {
    if (n_triples > 0 && (!s || !r || !o || !s_out || !r_out || !o_out)) return RGCN_ERR_NULL;
    if (n_triples < 0 || num_nodes < 1 || num_negatives < 1 || seed < 0) return RGCN_ERR_ARG;
    if ((u64)n_triples > kMaxKeys / (u64)num_negatives) return RGCN_ERR_PLAN;
    if (n_triples == 0) return RGCN_OK;
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    const u64 total = (u64)n_triples * (u64)num_negatives;
    const u64 want = (total + 255) / 256;
    hipLaunchKernelGGL(lp_corrupt_kernel, dim3((unsigned)(want > 65536 ? 65536 : want)), dim3(256), 0, (hipStream_t)stream, s, r, o, total,
                       (u32)num_negatives, (u64)num_nodes, (u64)seed, s_out, r_out, o_out);
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_lp_rank_workspace_bytes(int64_t n_queries, int32_t num_nodes, int width) {
    if (n_queries <= 0 || num_nodes < 0 || width < 1 || width > RGCN_MAX_WIDTH || (u64)n_queries > kMaxKeys) return 0;
    Arena ar(nullptr);
    ar.take<float>((size_t)n_queries);
    return ar.bytes();
}

extern "C" int rgcn_lp_rank(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                            const int64_t* anchor, const int64_t* r, const int64_t* target, int64_t n_queries, const int64_t* filter_ptr,
                            const int64_t* filter_idx, int64_t filter_len, int64_t* greater, int64_t* equal, void* workspace,
                            size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!anchor || !r || !target || !greater || !equal)) return RGCN_ERR_NULL;
    if (filter_ptr != nullptr && filter_len > 0 && !filter_idx) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if (n_queries < 0 || filter_len < 0) return RGCN_ERR_ARG;
    if ((u64)n_queries > kMaxKeys) return RGCN_ERR_PLAN;
    if (n_queries == 0) return RGCN_OK;
    Arena ar(workspace);
    float* tscore = ar.take<float>((size_t)n_queries);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t q = (hipStream_t)stream;
    RankArgs a;
    a.z = z;
    a.rel = rel;
    a.a = anchor;
    a.r = r;
    a.e = target;
    a.fptr = filter_ptr;
    a.fidx = filter_idx;
    a.flen = filter_len;
    a.tscore = tscore;
    a.greater = (u64*)greater;
    a.equal = (u64*)equal;
    a.nq = n_queries;
    a.num_nodes = num_nodes;
    a.num_relations = num_relations;
    a.width = width;
    a.ldz = ldz;
    a.ldr = ldr;
    a.k16 = (width + 15) / 16;
    (void)hipMemsetAsync(greater, 0, sizeof(int64_t) * (size_t)n_queries, q);
    (void)hipMemsetAsync(equal, 0, sizeof(int64_t) * (size_t)n_queries, q);
    const int64_t qblocks = (n_queries + kRankQueries - 1) / kRankQueries;
    const int64_t tiles = ((int64_t)num_nodes + 15) / 16;
    int64_t slices = (kRankBlocks + qblocks - 1) / qblocks;
    const int64_t most = (tiles + kRankWaves - 1) / kRankWaves;
    if (slices > most) slices = most;
    if (slices < 1) slices = 1;
    return rgcn::for_padded_width(rgcn::padded_width(width), [&](auto kp) {
        constexpr int KT = decltype(kp)::value / 16;
        hipLaunchKernelGGL((lp_rank_kernel<KT, true>), dim3((unsigned)qblocks), dim3(kRankThreads), 0, q, a);
        hipLaunchKernelGGL((lp_rank_kernel<KT, false>), dim3((unsigned)qblocks, (unsigned)slices), dim3(kRankThreads), 0, q, a);
        return (int)hipGetLastError();
    });
}

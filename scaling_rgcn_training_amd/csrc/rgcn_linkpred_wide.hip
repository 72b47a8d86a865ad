// rgcn_linkpred_wide.hip -- link prediction on rows of up to 512 columns behind the C ABI rgcn_lpw_* of include/rgcn_mi355x.h: the
// DistMult score, its backward and the filtered ranking pass.  gfx950 only.  DESIGN.md section 21 has the work split and the
// summation orders; the conventions are section 18's (rgcn_linkpred.hip), whose index build and negatives serve both families.
//
//   z [N][ldz], rel [R][ldr] fp32, widths 1..512, strides multiples of 4 and at least the width, bases 16-byte aligned.  Pad columns
//   are masked out of every sum, whatever they hold.  A row is up to 128 16-byte pieces: lane l of a wave owns pieces l and l + 64.
//
//   lpw_score_kernel     one wave per triple; a lane adds its pieces in ascending order, the lanes by a fixed shuffle tree.
//   lpw_dz_kernel        one wave per node; it walks the node's slots in sorted (= position) order.  Every row is written.
//   lpw_drel_*           a relation's triples in chunks of kRelChunk; a chunk is one workgroup of kChunkWaves waves (wave w takes the
//                        triples w, w + W, ..), whose rows are added in wave order through LDS; then one wave per relation adds the
//                        chunk rows in order.
//   lpw_rank_kernel      QW (64 or 32) query rows z[a] o rel[r] in dynamic LDS, sized by the width; entity rows streamed 16 per wave
//                        in slabs of 128 columns (eight f32x4 per lane), the next slab's loads issued before this slab's
//                        v_mfma_f32_16x16x4_f32 steps, the accumulators of the QW / 16 query tiles live across the slabs.
//                        lpw_tile_step is the ONE function that makes a score: the sweep, the targets and the filter lists all run
//                        it over (slab, c, j) in the same order, so a (query, entity) pair has the same bits wherever it is scored.
// No float atomics anywhere; integer atomics in the counts and the `bad` word.
#include "rgcn_common.h"
#include "rgcn_kernels_shared.h"
#include "rgcn_sort_scan.h"

namespace rgcn_lpw {

using namespace rgcn_sort_scan;
using rgcn::f32x4;

constexpr int kBadNode = 1, kBadRel = 2;     // bits of the `bad` word (RGCN_LP_BAD_*)
constexpr u32 kRelChunk = 256;               // triples per chunk of a relation's gradient
constexpr int kChunkWaves = 4;               // waves that share a chunk
constexpr int kMaxPieces = RGCN_XWIDE_MAX_WIDTH / 4;

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

// what the score and the backward read
struct Triples {
    const float* z;
    const float* rel;
    const int64_t* s;
    const int64_t* r;
    const int64_t* o;
    int num_nodes, num_relations, width, width4, ldz, ldr;
};

// ------------------------------------------------------------------------------------------------
// a. score
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lpw_score_kernel(const Triples a, u64 n, float* __restrict__ score, int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const u64 t = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= n) return;                      // (wave-uniform)
    const int64_t s = a.s[t], r = a.r[t], o = a.o[t];
    const int flags = id_flags(s, r, o, a.num_nodes, a.num_relations);
    float v = 0.f;
    if (flags == 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h, c0 = 4 * p;
            if (p < a.width4) {
                const f32x4 q = mask_pad(piece(a.z, s, a.ldz, c0) * piece(a.rel, r, a.ldr, c0) * piece(a.z, o, a.ldz, c0), c0, a.width);
                v += (q[0] + q[1]) + (q[2] + q[3]);
            }
        }
    } else if (lane == 0 && bad != nullptr) {
        atomicOr(bad, flags);
    }
    // lane 0 ends with ((((v0 + v32) + (v16 + v48)) + ..): the same tree at every width, lanes without a piece add 0
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) score[t] = v;
}

// ------------------------------------------------------------------------------------------------
// b. backward
// ------------------------------------------------------------------------------------------------
struct BwdArgs {
    Triples t;
    const float* g;
    const u32* node_ptr;
    const u32* node_slot;
    const u32* rel_ptr;
    const u32* rel_triple;
    const u32* chunk_ptr;
    float* partial;         // [chunks][4 width4]
    float* dz;
    float* drel;
    int lddz, lddrel;
};

__global__ void __launch_bounds__(256) lpw_dz_kernel(const BwdArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 v = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= (u64)a.t.num_nodes) return;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const u32 end = a.node_ptr[v + 1];
    for (u32 j = a.node_ptr[v]; j < end; ++j) {
        const u32 slot = a.node_slot[j], t = slot >> 1;
        const int64_t other = (slot & 1u) ? a.t.s[t] : a.t.o[t], r = a.t.r[t];
        const float gt = a.g[t];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            if (p < a.t.width4) acc[h] += (gt * piece(a.t.rel, r, a.t.ldr, 4 * p)) * piece(a.t.z, other, a.t.ldz, 4 * p);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;      // the pad columns of the last piece: +0.0
        if (p < a.t.width4) *(f32x4*)(a.dz + (int64_t)v * a.lddz + 4 * p) = mask_pad(acc[h], 4 * p, a.t.width);
    }
}

// chunk_ptr[r] = chunks of kRelChunk triples of the relations before r; one workgroup
__global__ void __launch_bounds__(kScanThreads) lpw_chunk_ptr_kernel(const u32* __restrict__ rel_ptr, int num_relations,
                                                                     u32* __restrict__ chunk_ptr) {
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

// one workgroup per chunk: wave w takes the chunk's triples w, w + W, w + 2W, .. in order, then piece p of the chunk's row is
// wave 0's + wave 1's + .. + wave W-1's, added by thread p
__global__ void __launch_bounds__(64 * kChunkWaves) lpw_drel_chunk_kernel(const BwdArgs a) {
    __shared__ f32x4 part[kChunkWaves][kMaxPieces];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 unit = blockIdx.x;
    if (unit >= a.chunk_ptr[a.t.num_relations]) return;      // (uniform over the workgroup)
    int lo = 0, hi = a.t.num_relations - 1;
    while (lo < hi) {                                        // the relation whose chunks hold `unit`
        const int mid = (lo + hi) >> 1;
        if (a.chunk_ptr[mid + 1] <= unit) lo = mid + 1; else hi = mid;
    }
    const u32 beg = a.rel_ptr[lo] + (unit - a.chunk_ptr[lo]) * kRelChunk;
    const u32 end = beg + kRelChunk < a.rel_ptr[lo + 1] ? beg + kRelChunk : a.rel_ptr[lo + 1];
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (u32 j = beg + (u32)wave; j < end; j += (u32)kChunkWaves) {
        const u32 t = a.rel_triple[j];
        const int64_t s = a.t.s[t], o = a.t.o[t];
        const float gt = a.g[t];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            if (p < a.t.width4) acc[h] += (gt * piece(a.t.z, s, a.t.ldz, 4 * p)) * piece(a.t.z, o, a.t.ldz, 4 * p);
        }
    }
    part[wave][lane] = acc[0];
    part[wave][lane + 64] = acc[1];
    __syncthreads();
    if (tid < a.t.width4) {
        f32x4 sum = part[0][tid];
#pragma unroll
        for (int w = 1; w < kChunkWaves; ++w) sum += part[w][tid];
        *(f32x4*)(a.partial + ((size_t)unit * a.t.width4 + tid) * 4) = sum;
    }
}

// one wave per relation: its chunks' rows in ascending chunk order
__global__ void __launch_bounds__(256) lpw_drel_sum_kernel(const BwdArgs a) {
    const int lane = threadIdx.x & 63;
    const u32 r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (u32)a.t.num_relations) return;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const u32 end = a.chunk_ptr[r + 1];
    for (u32 c = a.chunk_ptr[r]; c < end; ++c) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            if (p < a.t.width4) acc[h] += *(const f32x4*)(a.partial + ((size_t)c * a.t.width4 + p) * 4);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        if (p < a.t.width4) *(f32x4*)(a.drel + (int64_t)r * a.lddrel + 4 * p) = mask_pad(acc[h], 4 * p, a.t.width);
    }
}

// ------------------------------------------------------------------------------------------------
// c. ranks
// ------------------------------------------------------------------------------------------------
constexpr int kRankThreads = 512;
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kRankBlocks = 1024;                // workgroups a launch aims at: four per CU
constexpr int kSlabSteps = 8;                    // a slab: eight steps of 16 columns, 128 columns, eight f32x4 per lane
constexpr int kSplitWidth = 256;                 // rows wider than this: 32 queries per workgroup (measured)

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

// The MFMA's k index is permuted as in lp_rank_kernel: lane (rl, kq) holds the four consecutive columns 16 c + 4 kq + j of its row
// and feeds element j to step (c, j); q4[(4 c + kq) * QW + query] is the 16-byte piece 4 c + kq of a query row.
//
// lpw_load_slab: the B operand of slab `sl`, the pieces 128 sl + 16 c + 4 kq of row `row` of z, ISSUED and not waited for
// (rgcn::prefetch16: a load the compiler can neither sink below the MFMAs it should overlap nor wait for early); nothing touches zf
// before lpw_wait_slab.  No lane is predicated: `row` is a row of z (the callers clamp; what a clamped lane scores is never
// counted) and a piece behind the row's last one is read from the last one (never multiplied, or zeroed by lpw_wait_slab).
__device__ __forceinline__ void lpw_load_slab(f32x4 (&zf)[kSlabSteps], const RankArgs& a, int64_t row, int kq, int sl) {
    const float* base = a.z + row * (int64_t)a.ldz;
    const int cmax = 4 * ((a.width + 3) / 4 - 1);
#pragma unroll
    for (int c = 0; c < kSlabSteps; ++c) {
        const int col = 16 * (kSlabSteps * sl + c) + 4 * kq;
        rgcn::prefetch16<0>(zf[c], (const f32x4*)(base + (col < cmax ? col : cmax)));
    }
}

// lpw_wait_slab: every load this wave has issued has landed (the slab's registers are operands, so that no use of them is
// scheduled above the wait), and the operand is made what the sums need: step k16 - 1 is the only one of a row that can hold pad
// columns or lie partly behind the width (the steps behind it are never multiplied), so its pad elements become zeros here.
__device__ __forceinline__ void lpw_wait_slab(f32x4 (&zf)[kSlabSteps], const RankArgs& a, int kq, int sl) {
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(zf[0]), "+v"(zf[1]), "+v"(zf[2]), "+v"(zf[3]), "+v"(zf[4]), "+v"(zf[5]), "+v"(zf[6]), "+v"(zf[7])::"memory");
    if (kSlabSteps * (sl + 1) < a.k16) return;   // (wave-uniform) the row's last step lies in a later slab
#pragma unroll
    for (int c = 0; c < kSlabSteps; ++c) {
        const int cc = kSlabSteps * sl + c, col = 16 * cc + 4 * kq;
        if (cc == a.k16 - 1) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            zf[c] = col < a.width ? mask_pad(zf[c], col, a.width) : zero;
        }
    }
}

// lpw_tile_step: THE score of the ranking pass, one slab of it.  acc[r] of lane (rl, kq) = score(query 16 qt + 4 kq + r, the row
// lane rl loaded), continued over slab `sl`.  Every element of the tile is its own chain of MFMA steps over (sl, c, j) in that
// order: its bits depend on the two rows alone, not on where in a tile the pair sits or which rows share the tile.
template <int QW>
__device__ __forceinline__ void lpw_tile_step(f32x4& acc, const f32x4* q4, int qt, int sl, int rl, int kq, const f32x4 (&zf)[kSlabSteps],
                                              int k16) {
    const f32x4* q = q4 + (4 * kSlabSteps * sl + kq) * QW + 16 * qt + rl;
    if (kSlabSteps * (sl + 1) <= k16) {          // (wave-uniform) a whole slab
#pragma unroll
        for (int c = 0; c < kSlabSteps; ++c) {
            const f32x4 qa = q[4 * c * QW];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[j], zf[c][j], acc, 0, 0, 0);
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < kSlabSteps; ++c) {
        if (kSlabSteps * sl + c < k16) {
            const f32x4 qa = q[4 * c * QW];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[j], zf[c][j], acc, 0, 0, 0);
        }
    }
}

// a tile of rows gathered by index (the targets, a filter list): slab by slab through lpw_tile_step.  row < 0: a lane whose score
// the caller does not use; it reads row 0 (the callers have num_nodes > 0).
template <int QW>
__device__ __forceinline__ f32x4 lpw_score_rows(const f32x4* q4, int qt, const RankArgs& a, int64_t row, int rl, int kq) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    f32x4 zf[kSlabSteps];
    const int ns = (a.k16 + kSlabSteps - 1) / kSlabSteps;
#pragma unroll 1
    for (int sl = 0; sl < ns; ++sl) {
        lpw_load_slab(zf, a, row < 0 ? 0 : row, kq, sl);
        lpw_wait_slab(zf, a, kq, sl);
        lpw_tile_step<QW>(acc, q4, qt, sl, rl, kq, zf, a.k16);
    }
    return acc;
}

__device__ __forceinline__ float pick4(const f32x4& v, int r) {
    const float lo = (r & 1) ? v[1] : v[0], hi = (r & 1) ? v[3] : v[2];
    return (r & 2) ? hi : lo;
}

// QW queries per workgroup (32: two workgroups share a CU's registers and LDS).  TARGETS: the workgroup scores its queries' targets
// into a.tscore, clears their counts and ends.  Otherwise grid (query blocks, entity slices): the sweep over this slice's entity
// tiles, then the filter lists and the target's own count, dealt over the slices' waves.
template <int QW, bool TARGETS>
__global__ void __launch_bounds__(kRankThreads) __attribute__((amdgpu_waves_per_eu(QW == 32 ? 4 : 2))) lpw_rank_kernel(const RankArgs a) {
    constexpr int QT = QW / 16;
    // all LDS is dynamic (rgcn::allow_full_lds raises the dynamic limit to the whole CU's): the query image, then per query the
    // target's score, the ok flag and the two counts
    extern __shared__ f32x4 q4[];                // [4 k16][QW]
    float* ts_l = (float*)(q4 + 4 * a.k16 * QW);
    int* ok_l = (int*)(ts_l + QW);
    u32(*cnt_l)[QW] = (u32(*)[QW])(ok_l + QW);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * QW;

    // the query rows z[a] o rel[r], zero where the query is past the end or has an id out of range
    for (int i = tid; i < a.k16 * 4 * QW; i += kRankThreads) {
        const int pc = i / QW, qi = i - pc * QW, col = 4 * pc;
        const int64_t q = q0 + qi;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < a.nq && col < a.width) {
            const int64_t an = a.a[q], rn = a.r[q], en = a.e[q];
            if (id_flags(an, rn, en, a.num_nodes, a.num_relations) == 0)
                v = mask_pad(piece(a.z, an, a.ldz, col) * piece(a.rel, rn, a.ldr, col), col, a.width);
        }
        q4[i] = v;
    }
    if (tid < QW) {
        const int64_t q = q0 + tid;
        const bool ok = q < a.nq && id_flags(a.a[q], a.r[q], a.e[q], a.num_nodes, a.num_relations) == 0;
        ok_l[tid] = ok ? 1 : 0;
        if (!TARGETS) ts_l[tid] = ok ? a.tscore[q] : __builtin_inff();      // +inf: nothing is greater, nothing equal
        cnt_l[0][tid] = 0;
        cnt_l[1][tid] = 0;
        if (TARGETS && q < a.nq) {
            a.greater[q] = 0;
            a.equal[q] = 0;
        }
    }
    __syncthreads();

    if (TARGETS) {
        if (wave < QT && a.num_nodes > 0) {      // wave = query tile; column rl of the tile is the target of query 16 wave + rl
            const int qi = 16 * wave + rl;
            const f32x4 acc = lpw_score_rows<QW>(q4, wave, a, ok_l[qi] ? a.e[q0 + qi] : (int64_t)-1, rl, kq);
            if (kq == (rl >> 2) && q0 + qi < a.nq) a.tscore[q0 + qi] = pick4(acc, rl & 3);      // the diagonal
        }
        return;
    }

    // ---- sweep: this slice's entity tiles, 16 rows per wave and step, slab by slab; counts per lane in integer registers
    float tg[QT][4];
    u32 cg[QT][4], ce[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            tg[qt][r] = ts_l[16 * qt + 4 * kq + r];
            cg[qt][r] = 0;
            ce[qt][r] = 0;
        }
    }
    const int64_t tiles = ((int64_t)a.num_nodes + 15) / 16;
    const int64_t step = (int64_t)gridDim.y * kRankWaves;
    // the row of tile t this lane loads: past the last row or the last tile it loads row 0 again, and counts nothing
    auto row_of = [&](int64_t t) { return (t < tiles && t * 16 + rl < (int64_t)a.num_nodes) ? t * 16 + rl : (int64_t)0; };
    const int ns = (a.k16 + kSlabSteps - 1) / kSlabSteps;
    f32x4 cur[kSlabSteps], nxt[kSlabSteps];
    int64_t t = (int64_t)blockIdx.y * kRankWaves + wave;
    if (t < tiles) {
        lpw_load_slab(cur, a, row_of(t), kq, 0);
        lpw_wait_slab(cur, a, kq, 0);
    }
    for (; t < tiles; t += step) {
        const bool valid = t * 16 + rl < (int64_t)a.num_nodes;
        f32x4 acc[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int sl = 0; sl < ns; ++sl) {
            // the next slab of this tile, or the first of the wave's next tile, is on its way while this one is multiplied
            const bool more = sl + 1 < ns;
            lpw_load_slab(nxt, a, row_of(more ? t : t + step), kq, more ? sl + 1 : 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {    // (fenced per tile: the eight LDS reads of one tile ahead of its MFMAs, not all QT x 8)
                lpw_tile_step<QW>(acc[qt], q4, qt, sl, rl, kq, cur, a.k16);
                __builtin_amdgcn_sched_barrier(0);
            }
            lpw_wait_slab(nxt, a, kq, more ? sl + 1 : 0);
#pragma unroll
            for (int c = 0; c < kSlabSteps; ++c) cur[c] = nxt[c];
        }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                cg[qt][r] += (valid && acc[qt][r] > tg[qt][r]) ? 1u : 0u;
                ce[qt][r] += (valid && acc[qt][r] == tg[qt][r]) ? 1u : 0u;
            }
        }
    }
    // the sixteen lanes that share kq hold the counts of the same four queries per tile: add them, then the waves in LDS
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
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
    if (tid < QW && q0 + tid < a.nq) {
        if (cnt_l[0][tid]) atomicAdd(&a.greater[q0 + tid], (u64)cnt_l[0][tid]);
        if (cnt_l[1][tid]) atomicAdd(&a.equal[q0 + tid], (u64)cnt_l[1][tid]);
    }

    // ---- listed entities and the target itself: taken off again, scored by the same function on rows gathered by list.  An entry
    // that is the target is skipped (the target is taken off once, below); an entry out of range counts nothing.
    const int gw = (int)blockIdx.y * kRankWaves + wave, nw = (int)gridDim.y * kRankWaves;
    for (int qi = gw; qi < QW; qi += nw) {
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
                const f32x4 acc = lpw_score_rows<QW>(q4, qi >> 4, a, ok ? id : (int64_t)-1, rl, kq);
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
// host
// ------------------------------------------------------------------------------------------------
static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

static int check_stride(int ld, int width) {
    if (width < 1 || width > RGCN_XWIDE_MAX_WIDTH) return RGCN_ERR_WIDTH;
    if ((ld % 4) != 0 || ld < ((width + 3) / 4) * 4) return RGCN_ERR_STRIDE;
    return RGCN_OK;
}

// z / rel and their strides, the conventions every entry point shares
static int check_tables(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations) {
    int st;
    if ((st = check_stride(ldz, width)) != RGCN_OK) return st;
    if ((st = check_stride(ldr, width)) != RGCN_OK) return st;
    if (!aligned16(z) || !aligned16(rel)) return RGCN_ERR_STRIDE;
    if (num_nodes < 0 || num_relations < 0) return RGCN_ERR_ARG;
    if (num_relations > 65536) return RGCN_ERR_PLAN;
    return RGCN_OK;
}

static bool triples_fit(int64_t n) { return n >= 0 && 2ull * (u64)n <= kMaxKeys; }

static Triples triples_of(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                          const int64_t* s, const int64_t* r, const int64_t* o) {
    Triples t;
    t.z = z;
    t.rel = rel;
    t.s = s;
    t.r = r;
    t.o = o;
    t.num_nodes = num_nodes;
    t.num_relations = num_relations;
    t.width = width;
    t.width4 = (width + 3) / 4;
    t.ldz = ldz;
    t.ldr = ldr;
    return t;
}

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

template <int QW>
static int launch_rank(const RankArgs& a, int64_t n_queries, hipStream_t q) {
    const size_t lds = sizeof(f32x4) * 4 * (size_t)a.k16 * QW + 4 * sizeof(float) * QW;
    if (lds > 64 * 1024) {
        hipError_t e = rgcn::allow_full_lds<lpw_rank_kernel<QW, true>>();
        if (e == hipSuccess) e = rgcn::allow_full_lds<lpw_rank_kernel<QW, false>>();
        if (e != hipSuccess) return (int)e;
    }
    const int64_t qblocks = (n_queries + QW - 1) / QW;
    const int64_t tiles = ((int64_t)a.num_nodes + 15) / 16;
    int64_t slices = (kRankBlocks + qblocks - 1) / qblocks;
    const int64_t most = (tiles + kRankWaves - 1) / kRankWaves;
    if (slices > most) slices = most;
    if (slices < 1) slices = 1;
    hipLaunchKernelGGL((lpw_rank_kernel<QW, true>), dim3((unsigned)qblocks), dim3(kRankThreads), lds, q, a);
    hipLaunchKernelGGL((lpw_rank_kernel<QW, false>), dim3((unsigned)qblocks, (unsigned)slices), dim3(kRankThreads), lds, q, a);
    return (int)hipGetLastError();
}

}  // namespace rgcn_lpw

using namespace rgcn_lpw;

extern "C" int rgcn_lpw_score(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
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
    const Triples t = triples_of(z, ldz, rel, ldr, width, num_nodes, num_relations, s, r, o);
    hipLaunchKernelGGL(lpw_score_kernel, dim3((unsigned)(((u64)n_triples + 3) / 4)), dim3(256), 0, (hipStream_t)stream, t, (u64)n_triples,
                       score, bad);
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_lpw_backward_workspace_bytes(int64_t n_triples, int32_t num_relations, int width) {
    if (n_triples <= 0 || num_relations < 0 || num_relations > 65536 || width < 1 || width > RGCN_XWIDE_MAX_WIDTH ||
        !triples_fit(n_triples))
        return 0;
    Arena ar(nullptr);
    take_bwd_bufs(ar, n_triples, num_relations, width);
    return ar.bytes();
}

extern "C" int rgcn_lpw_backward(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                                 const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, const float* g,
                                 const uint32_t* node_ptr, const uint32_t* node_slot, const uint32_t* rel_ptr, const uint32_t* rel_triple,
                                 float* dz, int lddz, float* drel, int lddrel, void* workspace, size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_triples > 0 && (!s || !r || !o || !g)) return RGCN_ERR_NULL;
    if (n_triples > 0 && dz && (!node_ptr || !node_slot)) return RGCN_ERR_NULL;
    if (n_triples > 0 && drel && (!rel_ptr || !rel_triple)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if (dz && (st = check_stride(lddz, width)) != RGCN_OK) return st;
    if (drel && (st = check_stride(lddrel, width)) != RGCN_OK) return st;
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
    a.t = triples_of(z, ldz, rel, ldr, width, num_nodes, num_relations, s, r, o);
    a.g = g;
    a.node_ptr = node_ptr;
    a.node_slot = node_slot;
    a.rel_ptr = rel_ptr;
    a.rel_triple = rel_triple;
    a.chunk_ptr = bb.chunk_ptr;
    a.partial = bb.partial;
    a.dz = dz;
    a.drel = drel;
    a.lddz = lddz;
    a.lddrel = lddrel;
    if (dz && num_nodes > 0) hipLaunchKernelGGL(lpw_dz_kernel, dim3(((unsigned)num_nodes + 3u) / 4u), dim3(256), 0, q, a);
    if (drel && num_relations > 0) {
        hipLaunchKernelGGL(lpw_chunk_ptr_kernel, dim3(1), dim3(kScanThreads), 0, q, rel_ptr, (int)num_relations, bb.chunk_ptr);
        hipLaunchKernelGGL(lpw_drel_chunk_kernel, dim3(bb.max_chunks), dim3(64 * kChunkWaves), 0, q, a);
        hipLaunchKernelGGL(lpw_drel_sum_kernel, dim3(((unsigned)num_relations + 3u) / 4u), dim3(256), 0, q, a);
    }
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_lpw_rank_workspace_bytes(int64_t n_queries, int32_t num_nodes, int width) {
    if (n_queries <= 0 || num_nodes < 0 || width < 1 || width > RGCN_XWIDE_MAX_WIDTH || (u64)n_queries > kMaxKeys) return 0;
    Arena ar(nullptr);
    ar.take<float>((size_t)n_queries);
    return ar.bytes();
}

extern "C" int rgcn_lpw_rank(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                             const int64_t* anchor, const int64_t* r, const int64_t* target, int64_t n_queries, const int64_t* filter_ptr,
                             const int64_t* filter_idx, int64_t filter_len, int64_t* greater, int64_t* equal, int wg_queries,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!anchor || !r || !target || !greater || !equal)) return RGCN_ERR_NULL;
    if (filter_ptr != nullptr && filter_len > 0 && !filter_idx) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if (n_queries < 0 || filter_len < 0 || (wg_queries != 0 && wg_queries != 32 && wg_queries != 64)) return RGCN_ERR_ARG;
    if ((u64)n_queries > kMaxKeys) return RGCN_ERR_PLAN;
    if (n_queries == 0) return RGCN_OK;
    Arena ar(workspace);
    float* tscore = ar.take<float>((size_t)n_queries);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
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
    if (wg_queries == 0) wg_queries = width > kSplitWidth ? 32 : 64;
    return wg_queries == 32 ? launch_rank<32>(a, n_queries, (hipStream_t)stream) : launch_rank<64>(a, n_queries, (hipStream_t)stream);
}

// rgcn_kge.hip -- the asymmetric link-prediction decoders behind the C ABI rgcn_kge_* of include/rgcn_mi355x.h: ComplEx and TransE
// (L1): score, backward and filtered ranking.  gfx950 only.  DESIGN.md section 22 has the formulas, the work splits and the summation
// orders; the conventions, the index (rgcn_lp_index_build), the negatives and the relation-chunk scheme are section 18's
// (rgcn_linkpred.hip), shared through rgcn_lp_shared.h.
//
//   z [N][ldz], rel [R][ldr] fp32, widths 1..128 (ComplEx: even), strides multiples of 4 and at least the width, bases 16-byte
//   aligned.  Pad columns are masked out of every sum, whatever they hold.
//
//   ComplEx   columns 2k, 2k + 1 are the real and imaginary part of component k, so a 16-byte piece is two whole complex numbers and
//             a lane never needs a second piece of a row.  score = Re sum_k s_k r_k conj(o_k).  Complex products are written as one
//             multiply and one fma per part (cmul / cmulc below), so their bits do not hang on the compiler's contraction.
//   TransE    score = -sum_k |(s_k + r_k) - o_k|, sign(0) = 0 in the gradients.
//
//   kge_score_kernel     lp_score_kernel's shape: a triple is G = ceil(width / 4) lanes, one piece of each of the three rows per
//                        lane, a fixed shuffle tree over the lanes.
//   kge_dz_kernel        a node is G lanes and walks its slots in sorted order; the slot's parity picks the formula (subject end:
//                        d score / d s, object end: d score / d o).  Every row is written.
//   kge_drel_chunk_kernel  one wave per chunk of 256 triples of a relation, lane groups dealt round robin and added in order; then
//                        lp_drel_sum_kernel adds the chunks in order.
//   kge_complex_rank_kernel   the query rows s o r (object side) or conj(r) o o (subject side) as the LDS image of lp_rank_body: from
//                        there DistMult's permuted-k v_mfma_f32_16x16x4_f32 sweep, targets, lists and counts, one copy of the code.
//   kge_transe_rank_kernel    no matrix instruction fits an L1 norm: a VALU sweep with a work split of its own, described at te_tile,
//                        THE function that makes every TransE ranking score (sweep, targets, listed entities).
// No float atomics anywhere; integer atomics in the counts and the `bad` word.
#include "rgcn_lp_shared.h"

namespace rgcn_kge {

using namespace rgcn_lp;

constexpr int kComplex = RGCN_KGE_COMPLEX, kTransE = RGCN_KGE_TRANSE_L1;

// ---- the decoders' arithmetic on 16-byte pieces ------------------------------------------------------------------------
// x o y on two interleaved complex numbers: (a + bi)(c + di) = (ac - bd) + (ad + bc) i
__device__ __forceinline__ f32x4 cmul(f32x4 x, f32x4 y) {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        v[k] = __builtin_fmaf(x[k], y[k], -(x[k + 1] * y[k + 1]));
        v[k + 1] = __builtin_fmaf(x[k], y[k + 1], x[k + 1] * y[k]);
    }
    return v;
}

// conj(x) o y: (a - bi)(c + di) = (ac + bd) + (ad - bc) i
__device__ __forceinline__ f32x4 cmulc(f32x4 x, f32x4 y) {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        v[k] = __builtin_fmaf(x[k], y[k], x[k + 1] * y[k + 1]);
        v[k + 1] = __builtin_fmaf(x[k], y[k + 1], -(x[k + 1] * y[k]));
    }
    return v;
}

// sign((s + r) - o) per column, sign(0) = 0
__device__ __forceinline__ f32x4 te_sign(f32x4 s, f32x4 r, f32x4 o) {
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d = (s[e] + r[e]) - o[e];
        v[e] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    }
    return v;
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

// A lane's share of a score.  ComplEx: q = s o r, then the real dot product with o, the piece's two components added as p0 + p1.
// TransE: (|d0| + |d1|) + (|d2| + |d3|); the kernel negates the sum of the lanes.
template <int DEC>
__device__ __forceinline__ float score_piece(f32x4 s, f32x4 r, f32x4 o, int c0, int width) {
    if (DEC == kComplex) {
        const f32x4 q = cmul(s, r);
        const float p0 = __builtin_fmaf(q[0], o[0], q[1] * o[1]), p1 = __builtin_fmaf(q[2], o[2], q[3] * o[3]);
        return (c0 < width ? p0 : 0.f) + (c0 + 2 < width ? p1 : 0.f);
    }
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = c0 + e < width ? __builtin_fabsf((s[e] + r[e]) - o[e]) : 0.f;
    return (d[0] + d[1]) + (d[2] + d[3]);
}

template <int DEC>
__global__ void __launch_bounds__(256) kge_score_kernel(const ScoreArgs a) {
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
        v = score_piece<DEC>(piece(a.z, s, a.ldz, c0), piece(a.rel, r, a.ldr, c0), piece(a.z, o, a.ldz, c0), c0, a.g.width);
    } else if (p == 0 && a.bad != nullptr) {
        atomicOr(a.bad, flags);
    }
    for (int d = a.g.half; d >= 1; d >>= 1) {
        const float w = __shfl_down(v, d);
        if (p + d < a.g.lanes) v += w;
    }
    if (p == 0) a.score[t] = (DEC == kTransE && flags == 0) ? -v : v;
}

// ------------------------------------------------------------------------------------------------
// b. backward, on the index of rgcn_lp_index_build
// ------------------------------------------------------------------------------------------------
// dz[v] = sum over v's slots in sorted order of g_t * (d score_t / d that end).  Slot 2 t + side: side 0 is the subject end of t,
// side 1 the object end -- with DistMult both ends had one formula, here they do not:
//   ComplEx   subject: conj(r) o o      object: s o r
//   TransE    subject: -sign(d)         object: +sign(d),   d = (s + r) - o in that order
template <int DEC>
__global__ void __launch_bounds__(256) kge_dz_kernel(const BwdArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int sub = lane / a.gr.lanes;
    if (sub >= a.gr.per_wave) return;
    const u64 v = wave * (u64)a.gr.per_wave + (u64)sub;
    if (v >= (u64)a.num_nodes) return;
    const int c0 = 4 * (lane - sub * a.gr.lanes);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const f32x4 own = piece(a.z, (int64_t)v, a.ldz, c0);      // (TransE: the row of this node is one end of every d)
    const u32 end = a.node_ptr[v + 1];
    for (u32 j = a.node_ptr[v]; j < end; ++j) {
        const u32 slot = a.node_slot[j], t = slot >> 1;
        const bool object_end = (slot & 1u) != 0;
        const f32x4 other = piece(a.z, object_end ? a.s[t] : a.o[t], a.ldz, c0), rl = piece(a.rel, a.r[t], a.ldr, c0);
        const float g = a.g[t];
        if (DEC == kComplex)
            acc += g * (object_end ? cmul(other, rl) : cmulc(rl, other));
        else
            acc += (object_end ? g : -g) * (object_end ? te_sign(other, rl, own) : te_sign(own, rl, other));
    }
    *(f32x4*)(a.dz + (int64_t)v * a.lddz + c0) = mask_pad(acc, c0, a.gr.width);      // the pad columns of the last piece: +0.0
}

// drel: ComplEx conj(s) o o, TransE -sign(d).  One wave per chunk: lane group u takes the chunk's triples u, u + U, u + 2U, .. in
// order (U = 64 / G groups), then the groups are added in order 0, 1, .., U - 1 (lp_chunk_store)
template <int DEC>
__global__ void __launch_bounds__(256) kge_drel_chunk_kernel(const BwdArgs a) {
    const int lane = threadIdx.x & 63;
    const u32 unit = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (unit >= a.max_chunks || unit >= a.chunk_ptr[a.num_relations]) return;      // (wave-uniform)
    u32 beg, end;
    lp_chunk_range(a, unit, beg, end);
    const int sub = lane / a.gr.lanes, p = lane - sub * a.gr.lanes, c0 = 4 * p;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (sub < a.gr.per_wave) {
        for (u32 j = beg + (u32)sub; j < end; j += (u32)a.gr.per_wave) {
            const u32 t = a.rel_triple[j];
            const f32x4 s = piece(a.z, a.s[t], a.ldz, c0), o = piece(a.z, a.o[t], a.ldz, c0);
            if (DEC == kComplex)
                acc += a.g[t] * cmulc(s, o);
            else
                acc += -a.g[t] * te_sign(s, piece(a.rel, a.r[t], a.ldr, c0), o);
        }
    }
    lp_chunk_store(a, unit, acc, sub, p);
}

// ------------------------------------------------------------------------------------------------
// c. ranks
// ------------------------------------------------------------------------------------------------
struct KgeRankArgs {
    RankArgs b;
    int side;                  // 0: (s, r, ?), the anchor is the subject; 1: (?, r, o), the anchor is the object
};

__global__ void kge_clear_kernel(u64* __restrict__ greater, u64* __restrict__ equal, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        greater[i] = 0;
        equal[i] = 0;
    }
}

// ComplEx: score(q, c) is the real dot product of the query row and z[c] on either side, so everything behind the query image is
// lp_rank_body.  Object side: s o r.  Subject side: conj(r) o o.
template <int KT, bool TARGETS>
__global__ void __launch_bounds__(kRankThreads) kge_complex_rank_kernel(const KgeRankArgs a) {
    lp_rank_body<KT, TARGETS>(a.b, [&](int64_t an, int64_t rn, int col) {
        const f32x4 x = piece(a.b.z, an, a.b.ldz, col), y = piece(a.b.rel, rn, a.b.ldr, col);
        return a.side == 0 ? cmul(x, y) : cmulc(y, x);
    });
}

// ---- TransE: the VALU sweep ------------------------------------------------------------------------------------------------
// A workgroup is 4 waves and 64 queries.  The query rows (s + r on the object side, o - r on the subject side, pad columns and
// queries out of range zero) lie in LDS as 16-byte pieces, qT[piece * kTeStride + query]; wave w owns the REGISTER TILE of the 16
// queries 16 w .. 16 w + 15 and streams the slice's entity rows past them, 64 rows a step.
//   lanes          lane (rl, kq) = (lane & 15, lane >> 4) holds the pieces 4 c + kq (columns 16 c + 4 kq .. + 3) of the FOUR entity
//                  rows rl, rl + 16, rl + 32, rl + 48 of the step: the four lanes of a row read 64 consecutive bytes of it.  Only ONE
//                  16-column slab of the four rows is in registers at a time (4 x f32x4), the slab behind it -- or slab 0 of the next
//                  64 rows -- is loaded before the arithmetic of this one, so the width costs no registers.
//   accumulators   4 rows x 16 queries = 64 fp32 registers per lane, live across the slabs.
//   query pieces   one ds_read_b128 per (slab, query): the sixteen lanes that share kq read one address (a broadcast), the four kq
//                  read four pieces kTeStride = 65 pieces apart (bank groups 0, 4, 8, 12 apart: no conflict).  A piece read serves
//                  4 rows x 4 columns = 32 VALU lane-ops (one v_sub_f32 and one v_add_f32 with |x| on its source per column), so
//                  the LDS pipe issues one instruction per 32 VALU instructions.
//   order          the score of a (query, entity) pair: each kq adds its columns 16 c + 4 kq + j in ascending (c, j) order into
//                  one chain that starts at +0 -- pad columns add |0 - 0| = +0 and change nothing -- then the four chains are added
//                  as (k0 + k1) + (k2 + k3) (two xor shuffles; fp32 addition commutes, so all four lanes hold the same bits), and
//                  the sum is negated.  A function of the two rows and the width alone: not of the row's place in the step, not of
//                  the other rows or queries of the tile.
//   counts         every lane compares its 64 sums with the 16 target scores; the lanes kq = 0 count, in integer registers.
constexpr int kTeThreads = 256;
constexpr int kTeWaves = kTeThreads / 64;
constexpr int kTeRows = 64;                  // entity rows of a wave's step
constexpr int kTeStride = kRankQueries + 1;  // pieces between two consecutive pieces of one query in LDS

// the slab c of four rows (rows[j] < 0: zeros); pad columns masked
__device__ __forceinline__ void te_slab(f32x4 (&ent)[4], const RankArgs& a, const int64_t (&rows)[4], int c, int kq) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const int col = 16 * c + 4 * kq;
#pragma unroll
    for (int j = 0; j < 4; ++j) ent[j] = (rows[j] >= 0 && col < a.width) ? mask_pad(piece(a.z, rows[j], a.ldz, col), col, a.width) : zero;
}

// te_tile: THE score of the TransE ranking pass.  acc[j][q] of every lane = score(query 16 qt + q, row rows[j]).  `ent` holds slab 0
// of `rows` on entry and slab 0 of `next_rows` on return.
__device__ __forceinline__ void te_tile(float (&acc)[4][16], const f32x4* qT, int qt, int kq, const RankArgs& a, f32x4 (&ent)[4],
                                        const int64_t (&rows)[4], const int64_t (&next_rows)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;
    for (int c = 0; c < a.k16; ++c) {
        f32x4 cur[4], nxt[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = ent[j];
        if (c + 1 < a.k16) te_slab(nxt, a, rows, c + 1, kq); else te_slab(nxt, a, next_rows, 0, kq);
        const f32x4* qp = qT + (4 * c + kq) * kTeStride + 16 * qt;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const f32x4 qa = qp[q];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][q] += __builtin_fabsf(qa[e] - cur[j][e]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) ent[j] = nxt[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            float v = acc[j][q];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            acc[j][q] = -v;
        }
}

// TARGETS: the workgroup scores its 64 queries' targets into a.b.tscore and ends.  Otherwise grid (query blocks, entity slices).
template <bool TARGETS>
__global__ void __launch_bounds__(kTeThreads) kge_transe_rank_kernel(const KgeRankArgs ka) {
    __shared__ f32x4 qT[(RGCN_MAX_WIDTH / 4) * kTeStride];
    __shared__ float ts_l[kRankQueries];
    __shared__ int ok_l[kRankQueries];
    const RankArgs& a = ka.b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kRankQueries;
    const int64_t none[4] = {-1, -1, -1, -1};

    for (int i = tid; i < 4 * a.k16 * kRankQueries; i += kTeThreads) {
        const int pc = i / kRankQueries, qi = i - pc * kRankQueries, col = 4 * pc;
        const int64_t q = q0 + qi;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < a.nq && col < a.width) {
            const int64_t an = a.a[q], rn = a.r[q], en = a.e[q];
            if (id_flags(an, rn, en, a.num_nodes, a.num_relations) == 0) {
                const f32x4 x = piece(a.z, an, a.ldz, col), y = piece(a.rel, rn, a.ldr, col);
                v = mask_pad(ka.side == 0 ? x + y : x - y, col, a.width);
            }
        }
        qT[pc * kTeStride + qi] = v;
    }
    if (tid < kRankQueries) {
        const int64_t q = q0 + tid;
        const bool ok = q < a.nq && id_flags(a.a[q], a.r[q], a.e[q], a.num_nodes, a.num_relations) == 0;
        ok_l[tid] = ok ? 1 : 0;
        if (!TARGETS) ts_l[tid] = ok ? a.tscore[q] : __builtin_inff();      // +inf: nothing is greater, nothing equal
    }
    __syncthreads();

    float acc[4][16];
    f32x4 ent[4];
    if (TARGETS) {                               // wave = register tile; row slot (0, rl) is the target of query 16 wave + rl
        const int qi = 16 * wave + rl;
        const int64_t rows[4] = {ok_l[qi] ? a.e[q0 + qi] : (int64_t)-1, -1, -1, -1};
        te_slab(ent, a, rows, 0, kq);
        te_tile(acc, qT, wave, kq, a, ent, rows, none);
        // the diagonal.  (Sixteen predicated stores of registers named at compile time: an accumulator picked by a lane-dependent
        // index would send the whole tile through scratch memory.)
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (kq == 0 && rl == q && q0 + qi < a.nq) a.tscore[q0 + qi] = acc[0][q];
        return;
    }

    // ---- sweep: wave w compares the slice's rows with its 16 queries
    float tg[16];
    u32 cg[16], ce[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        tg[q] = ts_l[16 * wave + q];
        cg[q] = 0;
        ce[q] = 0;
    }
    const int64_t n = (int64_t)a.num_nodes, tiles = (n + kTeRows - 1) / kTeRows, step = (int64_t)gridDim.y;
    auto rows_of = [&](int64_t t, int64_t (&rows)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t row = t * kTeRows + 16 * j + rl;
            rows[j] = (t < tiles && row < n) ? row : (int64_t)-1;
        }
    };
    int64_t rows[4], next_rows[4];
    rows_of((int64_t)blockIdx.y, rows);
    te_slab(ent, a, rows, 0, kq);
    for (int64_t t = (int64_t)blockIdx.y; t < tiles; t += step) {
        rows_of(t + step, next_rows);
        te_tile(acc, qT, wave, kq, a, ent, rows, next_rows);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool mine = kq == 0 && rows[j] >= 0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                cg[q] += (mine && acc[j][q] > tg[q]) ? 1u : 0u;
                ce[q] += (mine && acc[j][q] == tg[q]) ? 1u : 0u;
            }
            rows[j] = next_rows[j];
        }
    }
    // the wave's counts of a query (only the lanes kq = 0 hold any), then one global integer atomic per query and wave
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        u32 g = cg[q], e = ce[q];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            g += __shfl_xor(g, m);
            e += __shfl_xor(e, m);
        }
        const int64_t qq = q0 + 16 * wave + q;
        if (lane == 0 && qq < a.nq) {
            if (g) atomicAdd(&a.greater[qq], (u64)g);
            if (e) atomicAdd(&a.equal[qq], (u64)e);
        }
    }

    // ---- listed entities and the target itself: taken off again, scored by te_tile on rows gathered by list, 64 entries a step.
    // An entry that is the target is skipped (the target is taken off once, below); an entry out of range counts nothing.
    const int gw = (int)blockIdx.y * kTeWaves + wave, nw = (int)gridDim.y * kTeWaves;
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
            for (int64_t base = beg; base < end; base += kTeRows) {
                int64_t ids[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t at = base + 16 * j + rl;
                    const int64_t id = at < end ? a.fidx[at] : (int64_t)-1;
                    ids[j] = (id >= 0 && id < n && id != target) ? id : (int64_t)-1;
                }
                te_slab(ent, a, ids, 0, kq);
                te_tile(acc, qT, qi >> 4, kq, a, ent, ids, none);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (q != (qi & 15)) continue;          // (wave-uniform; the register is named at compile time, as above)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool mine = kq == 0 && ids[j] >= 0;
                        ng += (u64)__popcll(__ballot(mine && acc[j][q] > ts));
                        ne += (u64)__popcll(__ballot(mine && acc[j][q] == ts));
                    }
                }
            }
        }
        if (lane == 0) {
            if (ng) atomicAdd(&a.greater[q], (u64)0 - ng);
            if (ne) atomicAdd(&a.equal[q], (u64)0 - ne);
        }
    }
}

static bool decoder_known(int decoder) { return decoder == kComplex || decoder == kTransE; }

// the width of a decoder's rows: ComplEx needs whole complex numbers
static int check_decoder(int decoder, int width) {
    if (!decoder_known(decoder)) return RGCN_ERR_ARG;
    if (decoder == kComplex && width >= 1 && width <= RGCN_MAX_WIDTH && (width & 1)) return RGCN_ERR_WIDTH;
    return RGCN_OK;
}

}  // namespace rgcn_kge

using namespace rgcn_kge;

extern "C" int rgcn_kge_score(int decoder, const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes,
                              int32_t num_relations, const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples,
                              float* score, int32_t* bad, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_triples > 0 && (!s || !r || !o || !score)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if ((st = check_decoder(decoder, width)) != RGCN_OK) return st;
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
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (decoder == kComplex)
        hipLaunchKernelGGL(kge_score_kernel<kComplex>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(kge_score_kernel<kTransE>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_kge_backward_workspace_bytes(int decoder, int64_t n_triples, int32_t num_relations, int width) {
    if (n_triples <= 0 || num_relations < 0 || num_relations > 65536 || width < 1 || width > RGCN_MAX_WIDTH || !triples_fit(n_triples) ||
        check_decoder(decoder, width) != RGCN_OK)
        return 0;
    Arena ar(nullptr);
    take_bwd_bufs(ar, n_triples, num_relations, width);
    return ar.bytes();
}

extern "C" int rgcn_kge_backward(int decoder, const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes,
                                 int32_t num_relations, const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples,
                                 const float* g, const uint32_t* node_ptr, const uint32_t* node_slot, const uint32_t* rel_ptr,
                                 const uint32_t* rel_triple, float* dz, int lddz, float* drel, int lddrel, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_triples > 0 && (!s || !r || !o || !g)) return RGCN_ERR_NULL;
    if (n_triples > 0 && dz && (!node_ptr || !node_slot)) return RGCN_ERR_NULL;
    if (n_triples > 0 && drel && (!rel_ptr || !rel_triple)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if ((st = check_decoder(decoder, width)) != RGCN_OK) return st;
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
    const bool cx = decoder == kComplex;
    if (dz && num_nodes > 0) {
        if (cx)
            hipLaunchKernelGGL(kge_dz_kernel<kComplex>, row_grid((u64)num_nodes), dim3(256), 0, q, a);
        else
            hipLaunchKernelGGL(kge_dz_kernel<kTransE>, row_grid((u64)num_nodes), dim3(256), 0, q, a);
    }
    if (drel && num_relations > 0) {
        const dim3 chunks((bb.max_chunks + 3) / 4);
        hipLaunchKernelGGL(lp_chunk_ptr_kernel, dim3(1), dim3(kScanThreads), 0, q, rel_ptr, (int)num_relations, bb.chunk_ptr);
        if (cx)
            hipLaunchKernelGGL(kge_drel_chunk_kernel<kComplex>, chunks, dim3(256), 0, q, a);
        else
            hipLaunchKernelGGL(kge_drel_chunk_kernel<kTransE>, chunks, dim3(256), 0, q, a);
        hipLaunchKernelGGL(lp_drel_sum_kernel, row_grid((u64)num_relations), dim3(256), 0, q, a);
    }
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_kge_rank_workspace_bytes(int decoder, int64_t n_queries, int32_t num_nodes, int width) {
    if (n_queries <= 0 || num_nodes < 0 || width < 1 || width > RGCN_MAX_WIDTH || (u64)n_queries > kMaxKeys ||
        check_decoder(decoder, width) != RGCN_OK)
        return 0;
    Arena ar(nullptr);
    ar.take<float>((size_t)n_queries);
    return ar.bytes();
}

extern "C" int rgcn_kge_rank(int decoder, int side, const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes,
                             int32_t num_relations, const int64_t* anchor, const int64_t* r, const int64_t* target, int64_t n_queries,
                             const int64_t* filter_ptr, const int64_t* filter_idx, int64_t filter_len, int64_t* greater, int64_t* equal,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!anchor || !r || !target || !greater || !equal)) return RGCN_ERR_NULL;
    if (filter_ptr != nullptr && filter_len > 0 && !filter_idx) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if ((st = check_decoder(decoder, width)) != RGCN_OK) return st;
    if (n_queries < 0 || filter_len < 0 || (side != 0 && side != 1)) return RGCN_ERR_ARG;
    if ((u64)n_queries > kMaxKeys) return RGCN_ERR_PLAN;
    if (n_queries == 0) return RGCN_OK;
    Arena ar(workspace);
    float* tscore = ar.take<float>((size_t)n_queries);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t q = (hipStream_t)stream;
    KgeRankArgs a;
    a.b.z = z;
    a.b.rel = rel;
    a.b.a = anchor;
    a.b.r = r;
    a.b.e = target;
    a.b.fptr = filter_ptr;
    a.b.fidx = filter_idx;
    a.b.flen = filter_len;
    a.b.tscore = tscore;
    a.b.greater = (u64*)greater;
    a.b.equal = (u64*)equal;
    a.b.nq = n_queries;
    a.b.num_nodes = num_nodes;
    a.b.num_relations = num_relations;
    a.b.width = width;
    a.b.ldz = ldz;
    a.b.ldr = ldr;
    a.b.k16 = (width + 15) / 16;
    a.side = side;
    hipLaunchKernelGGL(kge_clear_kernel, dim3(grid_for((u64)n_queries)), dim3(256), 0, q, a.b.greater, a.b.equal, n_queries);
    const int64_t qblocks = (n_queries + kRankQueries - 1) / kRankQueries;
    if (decoder == kTransE) {
        const unsigned slices = (unsigned)rank_slices(qblocks, num_nodes, kTeRows, 1);      // (every wave of a workgroup takes every step)
        hipLaunchKernelGGL(kge_transe_rank_kernel<true>, dim3((unsigned)qblocks), dim3(kTeThreads), 0, q, a);
        hipLaunchKernelGGL(kge_transe_rank_kernel<false>, dim3((unsigned)qblocks, slices), dim3(kTeThreads), 0, q, a);
        return (int)hipGetLastError();
    }
    const unsigned slices = (unsigned)rank_slices(qblocks, num_nodes, 16, kRankWaves);
    return rgcn::for_padded_width(rgcn::padded_width(width), [&](auto kp) {
        constexpr int KT = decltype(kp)::value / 16;
        hipLaunchKernelGGL((kge_complex_rank_kernel<KT, true>), dim3((unsigned)qblocks), dim3(kRankThreads), 0, q, a);
        hipLaunchKernelGGL((kge_complex_rank_kernel<KT, false>), dim3((unsigned)qblocks, slices), dim3(kRankThreads), 0, q, a);
        return (int)hipGetLastError();
    });
}

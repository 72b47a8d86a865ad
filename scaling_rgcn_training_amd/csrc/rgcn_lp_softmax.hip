// rgcn_lp_softmax.hip -- the softmax (1-N, "1vsAll") link-prediction loss behind the C ABI rgcn_lpsm_* of include/rgcn_mi355x.h:
//   loss_i = logsumexp_n <q_i, z_n> - <q_i, z_target_i>     over ALL N entities, and its gradient, with no [Q, N] matrix anywhere.
// gfx950 only.  DESIGN.md section 23 has the work splits, the register and LDS budgets and the summation orders; the conventions, the
// index and the relation-chunk scheme are section 18's, the query rows section 22's, shared through rgcn_lp_shared.h.
//
//   lpsm_query_kernel     the decoder's query row of (anchor, r) as a row of qrows: a triple is G = ceil(width / 4) lanes, one 16-byte
//                         piece per lane (lp_score_kernel's shape).  DistMult z[a] o rel[r]; ComplEx s o r / conj(r) o o.
//   lpsm_sweep_kernel     lp_rank_body's geometry: 64 query rows in LDS, grid (query blocks, entity slices), 16 entity rows per wave
//                         and step on lp_score_tile.  Where the rank kernel counts, a lane keeps an online (max, sum) pair per
//                         accumulator element; pairs are merged in fixed order (lanes, waves, then the slices in lpsm_finish_kernel).
//   lpsm_grad_kernel      ONE body for dq (queries stationary, entities streamed) and dz (entities stationary, queries streamed):
//                         S^T = streamed . stationary^T on v_mfma_f32_16x16x4_f32, w from S^T on the VALU, acc += w . streamed on the
//                         same instruction.  The first product is computed TRANSPOSED so that its C layout is the second product's A
//                         layout (no LDS round trip for w); the streamed tile is read a second time, by column, for the B operand.
//   lpsm_dz_kernel / lpsm_drel_chunk_kernel    lp_dz_kernel and lp_drel_chunk_kernel with a row of dq where they have a scalar g.
// No float atomics anywhere (one integer atomicOr into the `bad` word): the same inputs give the same bits.
#include "rgcn_lp_shared.h"

namespace rgcn_lpsm {

using namespace rgcn_lp;

constexpr int kComplex = RGCN_KGE_COMPLEX, kDistMult = RGCN_LPSM_DISTMULT;

// x o y and conj(x) o y on two interleaved complex numbers, written as in rgcn_kge.hip (one multiply and one fma per part)
__device__ __forceinline__ f32x4 cmul(f32x4 x, f32x4 y) {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        v[k] = __builtin_fmaf(x[k], y[k], -(x[k + 1] * y[k + 1]));
        v[k + 1] = __builtin_fmaf(x[k], y[k + 1], x[k + 1] * y[k]);
    }
    return v;
}

__device__ __forceinline__ f32x4 cmulc(f32x4 x, f32x4 y) {
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
        v[k] = __builtin_fmaf(x[k], y[k], x[k + 1] * y[k + 1]);
        v[k + 1] = __builtin_fmaf(x[k], y[k + 1], -(x[k + 1] * y[k]));
    }
    return v;
}

// ------------------------------------------------------------------------------------------------
// a. query rows
// ------------------------------------------------------------------------------------------------
struct QueryArgs {
    const float* z;
    const float* rel;
    const int64_t* a;
    const int64_t* r;
    const int64_t* e;
    float* q;
    int64_t* qtarget;
    int32_t* bad;
    u64 n;
    int num_nodes, num_relations, ldz, ldr, ldq, decoder, side;
    Group g;
};

__global__ void __launch_bounds__(256) lpsm_query_kernel(const QueryArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int sub = lane / a.g.lanes;
    if (sub >= a.g.per_wave) return;
    const u64 t = wave * (u64)a.g.per_wave + (u64)sub;
    if (t >= a.n) return;
    const int p = lane - sub * a.g.lanes, c0 = 4 * p;
    const int64_t an = a.a[t], rn = a.r[t], en = a.e[t];
    const int flags = id_flags(an, rn, en, a.num_nodes, a.num_relations);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (flags == 0) {
        const f32x4 x = piece(a.z, an, a.ldz, c0), y = piece(a.rel, rn, a.ldr, c0);
        v = mask_pad(a.decoder == kDistMult ? x * y : (a.side == 0 ? cmul(x, y) : cmulc(y, x)), c0, a.g.width);
    } else if (p == 0 && a.bad != nullptr) {
        atomicOr(a.bad, flags);
    }
    *(f32x4*)(a.q + (int64_t)t * a.ldq + c0) = v;
    if (p == 0) a.qtarget[t] = flags == 0 ? en : (int64_t)-1;
}

// ------------------------------------------------------------------------------------------------
// b. forward: online log-sum-exp behind lp_score_tile
// ------------------------------------------------------------------------------------------------
// 64 rows of a table as the q4 image of lp_score_tile (rgcn_lp_shared.h): rows past `rows` and pad columns zero
template <int KT>
__device__ __forceinline__ void load_image(f32x4* q4, const float* tab, int ld, int64_t rows, int64_t row0, int width) {
    for (int i = threadIdx.x; i < KT * 4 * kRankQueries; i += blockDim.x) {
        const int pc = i / kRankQueries, qi = i - pc * kRankQueries, col = 4 * pc;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + qi < rows && col < width) v = mask_pad(piece(tab, row0 + qi, ld, col), col, width);
        q4[i] = v;
    }
}

// (ma, sa) <- the pair of the union of two sets of logits: max and sum of exp(. - max).  Symmetric in its arguments bit for bit (no
// contraction: two rounded products, one rounded sum), so both lanes of a butterfly step hold the same pair.  An empty set is
// (-inf, 0): its factor is taken as 1 when both are empty (-inf - -inf is not a number) and is exp(-inf) = 0 otherwise.
__device__ __forceinline__ void merge_pair(float& ma, float& sa, float mb, float sb) {
    const float m = __builtin_fmaxf(ma, mb);
    const float ea = ma == m ? 1.f : expf(ma - m), eb = mb == m ? 1.f : expf(mb - m);
    sa = __fadd_rn(__fmul_rn(sa, ea), __fmul_rn(sb, eb));
    ma = m;
}

struct FwdArgs {
    RankArgs b;                // z, ldz, width, k16, num_nodes, nq (what lp_rank_rows / lp_score_tile read)
    const float* q;
    const int64_t* target;
    float2* part;              // [slices][qpad] (workspace): (max, sum) of a (query, slice)
    float* lse;
    float* tlogit;
    float* loss;
    int64_t qpad;
    int ldq, slices;
};

template <int KT>
__global__ void __launch_bounds__(kRankThreads) lpsm_sweep_kernel(const FwdArgs a) {
    __shared__ f32x4 q4[KT * 4 * kRankQueries];
    __shared__ float wm[kRankWaves][kRankQueries], wsum[kRankWaves][kRankQueries];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kRankQueries;
    load_image<KT>(q4, a.q, a.ldq, a.b.nq, q0, a.b.width);
    __syncthreads();

    const float ninf = -__builtin_inff();
    float m[kRankTiles][4], s[kRankTiles][4];
#pragma unroll
    for (int qt = 0; qt < kRankTiles; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            m[qt][r] = ninf;
            s[qt][r] = 0.f;
        }
    }
    f32x4 zf[KT];
    const int64_t tiles = ((int64_t)a.b.num_nodes + 15) / 16;
    const int64_t step = (int64_t)gridDim.y * kRankWaves;
    for (int64_t t = (int64_t)blockIdx.y * kRankWaves + wave; t < tiles; t += step) {
        const int64_t row = t * 16 + rl;
        const bool valid = row < (int64_t)a.b.num_nodes;      // a row past N is no logit at all (not a logit of 0)
        lp_rank_rows(zf, a.b, valid ? row : (int64_t)-1, kq);
#pragma unroll
        for (int qt = 0; qt < kRankTiles; ++qt) {
            const f32x4 acc = lp_score_tile(q4, qt, rl, kq, zf, a.b.k16);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // one exp per logit: e = exp(-|v - m|) rescales the sum when the max rises and is the new term when it does not
                const float d = acc[r] - m[qt][r], e = expf(-__builtin_fabsf(d));
                const float up = d > 0.f ? __builtin_fmaf(s[qt][r], e, 1.f) : s[qt][r] + e;
                s[qt][r] = valid ? up : s[qt][r];
                m[qt][r] = valid ? __builtin_fmaxf(m[qt][r], acc[r]) : m[qt][r];
            }
        }
    }
    // the sixteen lanes that share kq hold pairs of the same four queries per tile: a butterfly over them, then the waves in LDS
#pragma unroll
    for (int qt = 0; qt < kRankTiles; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mm = m[qt][r], ss = s[qt][r];
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) {
                const float om = __shfl_xor(mm, x), os = __shfl_xor(ss, x);
                merge_pair(mm, ss, om, os);
            }
            if (rl == 0) {
                wm[wave][16 * qt + 4 * kq + r] = mm;
                wsum[wave][16 * qt + 4 * kq + r] = ss;
            }
        }
    }
    __syncthreads();
    if (tid < kRankQueries) {
        float mm = ninf, ss = 0.f;
        for (int w = 0; w < kRankWaves; ++w) merge_pair(mm, ss, wm[w][tid], wsum[w][tid]);      // waves in order
        a.part[(int64_t)blockIdx.y * a.qpad + q0 + tid] = make_float2(mm, ss);
    }
}

// one workgroup of four waves per 64 queries: the targets' logits by lp_rank_body's TARGETS form (wave = query tile, column rl of the
// tile is the target of query 16 wave + rl, the diagonal is kept), then the slices' pairs in slice order
template <int KT>
__global__ void __launch_bounds__(256) lpsm_finish_kernel(const FwdArgs a) {
    __shared__ f32x4 q4[KT * 4 * kRankQueries];
    __shared__ float tl[kRankQueries];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kRankQueries;
    load_image<KT>(q4, a.q, a.ldq, a.b.nq, q0, a.b.width);
    __syncthreads();
    {
        const int qi = 16 * wave + rl;
        const int64_t tg = q0 + qi < a.b.nq ? a.target[q0 + qi] : (int64_t)-1;
        f32x4 zf[KT];
        lp_rank_rows(zf, a.b, (tg >= 0 && tg < (int64_t)a.b.num_nodes) ? tg : (int64_t)-1, kq);
        const f32x4 acc = lp_score_tile(q4, wave, rl, kq, zf, a.b.k16);
        if (kq == (rl >> 2)) tl[qi] = pick4(acc, rl & 3);
    }
    __syncthreads();
    const int64_t q = q0 + tid;
    if (tid < kRankQueries && q < a.b.nq) {
        float mm = -__builtin_inff(), ss = 0.f;
        for (int y = 0; y < a.slices; ++y) {
            const float2 p = a.part[(int64_t)y * a.qpad + q];
            merge_pair(mm, ss, p.x, p.y);
        }
        const float lse = mm + logf(ss);
        const int64_t tg = a.target[q];
        const bool ok = tg >= 0 && tg < (int64_t)a.b.num_nodes;       // (a void query: loss 0, and the backward gives it no weight)
        a.lse[q] = lse;
        a.tlogit[q] = ok ? tl[tid] : 0.f;
        a.loss[q] = ok ? lse - tl[tid] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------
// c. gradient sweep: acc[64 stationary rows][width] += w . streamed, w a function of stationary . streamed^T
// ------------------------------------------------------------------------------------------------
struct GradArgs {
    const float* a;            // stationary table [na][lda]: qrows (QSTAT) or z
    const float* b;            // streamed table [nb][ldb]: z (QSTAT) or qrows
    const float* lse;          // per query
    const float* g;
    const int64_t* target;
    float* out;                // [na][ldo], or slice y's partial rows at out + y slice_stride
    int64_t na, nb, nq;
    size_t slice_stride;
    int lda, ldb, ldo, width, k16, num_nodes;
};

// the weight of (query, entity n) up to the exp: g of a query that is void (target out of range) or past the end is 0
__device__ __forceinline__ void query_weights(const GradArgs& a, int64_t i, float& g, float& lse, int64_t& tg) {
    g = 0.f;
    lse = 0.f;
    tg = -1;
    if (i < a.nq) {
        tg = a.target[i];
        if (tg >= 0 && tg < (int64_t)a.num_nodes) {
            g = a.g[i];
            lse = a.lse[i];
        }
    }
}

__device__ __forceinline__ float weight(float s, float g, float lse, bool hit) {
    return g == 0.f ? 0.f : g * (expf(s - lse) - (hit ? 1.f : 0.f));
}

// Lane (rl, kq) of a wave, per streamed tile of 16 rows:
//   zf[c]        the pieces 4 c + kq of streamed row rl: the A operand of S^T = streamed . stationary^T, whose B operand is the q4 image
//                read exactly as lp_score_tile reads it.  st[r] = S^T[streamed 4 kq + r][stationary 16 qt + rl].
//   w[r]         from st[r]: it already lies as the A operand of the second product (row rl = stationary, k = kq), step r, with the
//                k index permuted to streamed row 4 kq + r.
//   bc[r]        column 16 ct + rl of streamed row 4 kq + r: the B operand of that step, read from memory a second time (the first
//                read left the line in cache; sixteen lanes read 64 consecutive bytes), one 16-column slab ct at a time.
//   acc[qt][ct]  rows 16 qt + 4 kq + r, column 16 ct + rl of the workgroup's 64 x width result; lives for the whole sweep.
template <int KT, bool QSTAT>
__global__ void __launch_bounds__(kRankThreads) lpsm_grad_kernel(const GradArgs a) {
    constexpr int kStride = KT * 16 + 4;         // floats between two rows of the waves' sum (4 kq rows apart: 16 banks apart)
    __shared__ __attribute__((aligned(16))) float smem[kRankQueries * kStride];
    f32x4* q4 = (f32x4*)smem;                    // the stationary image during the sweep, the sum of the waves after it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * kRankQueries;
    load_image<KT>(q4, a.a, a.lda, a.na, r0, a.width);
    __syncthreads();

    float sg[kRankTiles], sl[kRankTiles];
    int64_t stg[kRankTiles];
    if (QSTAT) {
#pragma unroll
        for (int qt = 0; qt < kRankTiles; ++qt) query_weights(a, r0 + 16 * qt + rl, sg[qt], sl[qt], stg[qt]);
    }
    f32x4 acc[kRankTiles][KT];
#pragma unroll
    for (int qt = 0; qt < kRankTiles; ++qt)
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) acc[qt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int64_t tiles = (a.nb + 15) / 16;
    const int64_t step = (int64_t)gridDim.y * kRankWaves;
    for (int64_t t = (int64_t)blockIdx.y * kRankWaves + wave; t < tiles; t += step) {
        f32x4 zf[KT];
        const int64_t row = t * 16 + rl;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            const int col = 16 * c + 4 * kq;
            zf[c] = (row < a.nb && col < a.width) ? mask_pad(piece(a.b, row, a.ldb, col), col, a.width) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        float tg_[4], tl_[4];
        int64_t ttg[4];
        if (!QSTAT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) query_weights(a, t * 16 + 4 * kq + r, tg_[r], tl_[r], ttg[r]);
        }
        // first product and the weights of all four stationary tiles (zf dies here) ...
        float w[kRankTiles][4];
#pragma unroll
        for (int qt = 0; qt < kRankTiles; ++qt) {
            f32x4 st = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < KT; ++c) {
                if (c < a.k16) {
                    const f32x4 qa = q4[(4 * c + kq) * kRankQueries + 16 * qt + rl];
#pragma unroll
                    for (int j = 0; j < 4; ++j) st = __builtin_amdgcn_mfma_f32_16x16x4f32(zf[c][j], qa[j], st, 0, 0, 0);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (QSTAT) {
                    const int64_t n = t * 16 + 4 * kq + r;
                    w[qt][r] = n < a.nb ? weight(st[r], sg[qt], sl[qt], n == stg[qt]) : 0.f;
                } else {
                    w[qt][r] = weight(st[r], tg_[r], tl_[r], ttg[r] == r0 + 16 * qt + rl);
                }
            }
        }
        // ... then the second product, one 16-column slab of the streamed tile at a time: four registers of B, not 4 KT
#pragma unroll
        for (int ct = 0; ct < KT; ++ct) {
            if (ct < a.k16) {
                float bc[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t brow = t * 16 + 4 * kq + r;
                    const int col = 16 * ct + rl;
                    bc[r] = (brow < a.nb && col < a.width) ? a.b[brow * (int64_t)a.ldb + col] : 0.f;
                }
#pragma unroll
                for (int qt = 0; qt < kRankTiles; ++qt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[qt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[qt][r], bc[r], acc[qt][ct], 0, 0, 0);
            }
        }
    }

    // the waves' accumulators, added in wave order over the image's LDS
    __syncthreads();
    for (int w = 0; w < kRankWaves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int qt = 0; qt < kRankTiles; ++qt)
#pragma unroll
                for (int ct = 0; ct < KT; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* at = smem + (16 * qt + 4 * kq + r) * kStride + 16 * ct + rl;
                        *at = w == 0 ? acc[qt][ct][r] : *at + acc[qt][ct][r];
                    }
        }
        __syncthreads();
    }
    const int w4 = (a.width + 3) / 4;
    float* out = a.out + (size_t)blockIdx.y * a.slice_stride;
    for (int i = tid; i < kRankQueries * w4; i += kRankThreads) {
        const int row = i / w4, p = i - row * w4;
        if (r0 + row < a.na) *(f32x4*)(out + (r0 + row) * (int64_t)a.ldo + 4 * p) = mask_pad(*(const f32x4*)(smem + row * kStride + 4 * p), 4 * p, a.width);
    }
}

// out[row] = the slices' partial rows added in slice order; one 16-byte piece per thread
__global__ void __launch_bounds__(256) lpsm_slice_sum_kernel(const float* __restrict__ part, int slices, int64_t rows, int w4,
                                                             float* __restrict__ out, int ldo) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * w4) return;
    const int64_t row = i / w4;
    const int p = (int)(i - row * w4);
    f32x4 acc = *(const f32x4*)(part + i * 4);
    for (int y = 1; y < slices; ++y) acc += *(const f32x4*)(part + ((int64_t)y * rows * w4 + i) * 4);
    *(f32x4*)(out + row * (int64_t)ldo + 4 * p) = acc;
}

// ------------------------------------------------------------------------------------------------
// d. from dq to the anchor rows and the relation rows, on the index of rgcn_lp_index_build
// ------------------------------------------------------------------------------------------------
struct QbArgs {
    BwdArgs b;                 // (g unused: the gradient of a triple is a row of dq)
    const float* dq;
    int lddq, decoder, side;
};

// dz[v] += sum over v's slots whose parity is the anchor end, in sorted order, of d q_t / d anchor applied to dq_t
__global__ void __launch_bounds__(256) lpsm_dz_kernel(const QbArgs a) {
    const BwdArgs& b = a.b;
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int sub = lane / b.gr.lanes;
    if (sub >= b.gr.per_wave) return;
    const u64 v = wave * (u64)b.gr.per_wave + (u64)sub;
    if (v >= (u64)b.num_nodes) return;
    const int c0 = 4 * (lane - sub * b.gr.lanes);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    bool any = false;
    const u32 end = b.node_ptr[v + 1];
    for (u32 j = b.node_ptr[v]; j < end; ++j) {
        const u32 slot = b.node_slot[j], t = slot >> 1;
        if ((int)(slot & 1u) != a.side) continue;
        const f32x4 d = piece(a.dq, t, a.lddq, c0), rl = piece(b.rel, b.r[t], b.ldr, c0);
        acc += a.decoder == kDistMult ? d * rl : (a.side == 0 ? cmulc(rl, d) : cmul(d, rl));
        any = true;
    }
    if (any) {
        float* at = b.dz + (int64_t)v * b.lddz + c0;
        *(f32x4*)at = mask_pad(*(const f32x4*)at + acc, c0, b.gr.width);
    }
}

// lp_drel_chunk_kernel's walk: DistMult dq o z[a]; ComplEx conj(s) o dq (side 0), conj(dq) o o (side 1)
__global__ void __launch_bounds__(256) lpsm_drel_chunk_kernel(const QbArgs a) {
    const BwdArgs& b = a.b;
    const int lane = threadIdx.x & 63;
    const u32 unit = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (unit >= b.max_chunks || unit >= b.chunk_ptr[b.num_relations]) return;      // (wave-uniform)
    u32 beg, end;
    lp_chunk_range(b, unit, beg, end);
    const int sub = lane / b.gr.lanes, p = lane - sub * b.gr.lanes, c0 = 4 * p;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (sub < b.gr.per_wave) {
        for (u32 j = beg + (u32)sub; j < end; j += (u32)b.gr.per_wave) {
            const u32 t = b.rel_triple[j];
            const f32x4 d = piece(a.dq, t, a.lddq, c0), x = piece(b.z, a.side == 0 ? b.s[t] : b.o[t], b.ldz, c0);
            acc += a.decoder == kDistMult ? d * x : (a.side == 0 ? cmulc(x, d) : cmulc(d, x));
        }
    }
    lp_chunk_store(b, unit, acc, sub, p);
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static int check_decoder(int decoder, int width) {
    if (decoder != kComplex && decoder != kDistMult) return RGCN_ERR_ARG;
    if (decoder == kComplex && width >= 1 && width <= RGCN_MAX_WIDTH && (width & 1)) return RGCN_ERR_WIDTH;
    return RGCN_OK;
}

static bool queries_fit(int64_t n) { return n >= 0 && n <= 0x7FFFFFFFll; }      // (a table of queries is streamed like one of nodes)

static int ld4(int width) { return (width + 3) / 4 * 4; }

static int64_t blocks_of(int64_t rows) { return (rows + kRankQueries - 1) / kRankQueries; }

// slices of the sweep whose stationary table has `stat` rows and whose streamed table has `streamed`
static int64_t slices_of(int64_t stat, int64_t streamed) { return rank_slices(blocks_of(stat), (int32_t)streamed, 16, kRankWaves); }

static float2* take_fwd_bufs(Arena& ar, int64_t nq, int32_t num_nodes) {
    return ar.take<float2>((size_t)slices_of(nq, num_nodes) * (size_t)blocks_of(nq) * kRankQueries);
}

struct GradBufs {
    float* pq;                 // [slices_q][nq][ld4]: only when the dq sweep is sliced
    float* pz;                 // [slices_z][num_nodes][ld4]: only when dz is wanted and its sweep is sliced
};

static GradBufs take_grad_bufs(Arena& ar, int64_t nq, int32_t num_nodes, int width, bool want_dz) {
    GradBufs b{};
    const int64_t sq = slices_of(nq, num_nodes), sz = slices_of(num_nodes, nq);
    if (sq > 1) b.pq = ar.take<float>((size_t)sq * (size_t)nq * ld4(width));
    if (want_dz && sz > 1) b.pz = ar.take<float>((size_t)sz * (size_t)num_nodes * ld4(width));
    return b;
}

template <bool QSTAT>
static int launch_grad(GradArgs a, float* final_out, int final_ld, float* partial, hipStream_t q) {
    const int64_t slices = slices_of(a.na, a.nb);
    if (slices > 1) {
        a.out = partial;
        a.ldo = ld4(a.width);
        a.slice_stride = (size_t)a.na * a.ldo;
    } else {
        a.out = final_out;
        a.ldo = final_ld;
        a.slice_stride = 0;
    }
    const dim3 grid((unsigned)blocks_of(a.na), (unsigned)slices);
    const int st = rgcn::for_padded_width(rgcn::padded_width(a.width), [&](auto kp) {
        constexpr int KT = decltype(kp)::value / 16;
        hipLaunchKernelGGL((lpsm_grad_kernel<KT, QSTAT>), grid, dim3(kRankThreads), 0, q, a);
        return (int)hipGetLastError();
    });
    if (st != RGCN_OK || slices == 1) return st;
    const int w4 = ld4(a.width) / 4;
    hipLaunchKernelGGL(lpsm_slice_sum_kernel, dim3(grid_for((u64)a.na * w4)), dim3(256), 0, q, partial, (int)slices, a.na, w4, final_out, final_ld);
    return (int)hipGetLastError();
}

}  // namespace rgcn_lpsm

using namespace rgcn_lpsm;

extern "C" int rgcn_lpsm_query(int decoder, int side, const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes,
                               int32_t num_relations, const int64_t* anchor, const int64_t* r, const int64_t* target, int64_t n_queries,
                               float* qrows, int ldq, int64_t* qtarget, int32_t* bad, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!anchor || !r || !target || !qrows || !qtarget)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if ((st = check_decoder(decoder, width)) != RGCN_OK) return st;
    if ((st = rgcn::check_stride(ldq, width)) != RGCN_OK) return st;
    if (!aligned16(qrows)) return RGCN_ERR_STRIDE;
    if (n_queries < 0 || (side != 0 && side != 1)) return RGCN_ERR_ARG;
    if (!queries_fit(n_queries)) return RGCN_ERR_PLAN;
    if (n_queries == 0) return RGCN_OK;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    QueryArgs a;
    a.z = z;
    a.rel = rel;
    a.a = anchor;
    a.r = r;
    a.e = target;
    a.q = qrows;
    a.qtarget = qtarget;
    a.bad = bad;
    a.n = (u64)n_queries;
    a.num_nodes = num_nodes;
    a.num_relations = num_relations;
    a.ldz = ldz;
    a.ldr = ldr;
    a.ldq = ldq;
    a.decoder = decoder;
    a.side = side;
    a.g = group_of(width);
    const u64 waves = (a.n + (u64)a.g.per_wave - 1) / (u64)a.g.per_wave;
    hipLaunchKernelGGL(lpsm_query_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_lpsm_forward_workspace_bytes(int64_t n_queries, int32_t num_nodes, int width) {
    if (n_queries <= 0 || num_nodes < 0 || width < 1 || width > RGCN_MAX_WIDTH || !queries_fit(n_queries)) return 0;
    Arena ar(nullptr);
    take_fwd_bufs(ar, n_queries, num_nodes);
    return ar.bytes();
}

extern "C" int rgcn_lpsm_forward(const float* qrows, int ldq, const float* z, int ldz, int width, int32_t num_nodes,
                                 const int64_t* target, int64_t n_queries, float* lse, float* tlogit, float* loss, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!z) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!qrows || !target || !lse || !tlogit || !loss)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, qrows, ldq, width, num_nodes, 0);
    if (st != RGCN_OK) return st;
    if (n_queries < 0) return RGCN_ERR_ARG;
    if (!queries_fit(n_queries)) return RGCN_ERR_PLAN;
    if (n_queries == 0) return RGCN_OK;
    Arena ar(workspace);
    float2* part = take_fwd_bufs(ar, n_queries, num_nodes);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t q = (hipStream_t)stream;
    FwdArgs a{};
    a.b.z = z;
    a.b.nq = n_queries;
    a.b.num_nodes = num_nodes;
    a.b.width = width;
    a.b.ldz = ldz;
    a.b.k16 = (width + 15) / 16;
    a.q = qrows;
    a.target = target;
    a.part = part;
    a.lse = lse;
    a.tlogit = tlogit;
    a.loss = loss;
    a.qpad = blocks_of(n_queries) * kRankQueries;
    a.ldq = ldq;
    a.slices = (int)slices_of(n_queries, num_nodes);
    const dim3 grid((unsigned)blocks_of(n_queries), (unsigned)a.slices);
    return rgcn::for_padded_width(rgcn::padded_width(width), [&](auto kp) {
        constexpr int KT = decltype(kp)::value / 16;
        hipLaunchKernelGGL(lpsm_sweep_kernel<KT>, grid, dim3(kRankThreads), 0, q, a);
        hipLaunchKernelGGL(lpsm_finish_kernel<KT>, dim3(grid.x), dim3(256), 0, q, a);
        return (int)hipGetLastError();
    });
}

extern "C" size_t rgcn_lpsm_backward_workspace_bytes(int64_t n_queries, int32_t num_nodes, int width, int want_dz) {
    if (n_queries <= 0 || num_nodes < 0 || width < 1 || width > RGCN_MAX_WIDTH || !queries_fit(n_queries)) return 0;
    Arena ar(nullptr);
    take_grad_bufs(ar, n_queries, num_nodes, width, want_dz != 0);
    return ar.bytes();
}

extern "C" int rgcn_lpsm_backward(const float* qrows, int ldq, const float* z, int ldz, int width, int32_t num_nodes,
                                  const int64_t* target, int64_t n_queries, const float* lse, const float* g, float* dq, int lddq,
                                  float* dz, int lddz, void* workspace, size_t workspace_bytes, void* stream) {
    if (!z) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!qrows || !target || !lse || !g || !dq)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, qrows, ldq, width, num_nodes, 0);
    if (st != RGCN_OK) return st;
    if ((st = rgcn::check_stride(lddq, width)) != RGCN_OK) return st;
    if (dz && (st = rgcn::check_stride(lddz, width)) != RGCN_OK) return st;
    if (!aligned16(dq) || !aligned16(dz)) return RGCN_ERR_STRIDE;
    if (n_queries < 0) return RGCN_ERR_ARG;
    if (!queries_fit(n_queries)) return RGCN_ERR_PLAN;
    if (n_queries == 0) return RGCN_OK;
    Arena ar(workspace);
    const GradBufs gb = take_grad_bufs(ar, n_queries, num_nodes, width, dz != nullptr);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (ar.bytes() > 0 && !workspace) return RGCN_ERR_NULL;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t q = (hipStream_t)stream;
    GradArgs a{};
    a.lse = lse;
    a.g = g;
    a.target = target;
    a.nq = n_queries;
    a.width = width;
    a.k16 = (width + 15) / 16;
    a.num_nodes = num_nodes;
    a.a = qrows;
    a.lda = ldq;
    a.na = n_queries;
    a.b = z;
    a.ldb = ldz;
    a.nb = num_nodes;
    if ((st = launch_grad<true>(a, dq, lddq, gb.pq, q)) != RGCN_OK) return st;
    if (!dz || num_nodes == 0) return RGCN_OK;
    a.a = z;
    a.lda = ldz;
    a.na = num_nodes;
    a.b = qrows;
    a.ldb = ldq;
    a.nb = n_queries;
    return launch_grad<false>(a, dz, lddz, gb.pz, q);
}

extern "C" size_t rgcn_lpsm_query_backward_workspace_bytes(int decoder, int64_t n_triples, int32_t num_relations, int width) {
    if (n_triples <= 0 || num_relations < 0 || num_relations > 65536 || width < 1 || width > RGCN_MAX_WIDTH || !triples_fit(n_triples) ||
        check_decoder(decoder, width) != RGCN_OK)
        return 0;
    Arena ar(nullptr);
    take_bwd_bufs(ar, n_triples, num_relations, width);
    return ar.bytes();
}

extern "C" int rgcn_lpsm_query_backward(int decoder, int side, const float* z, int ldz, const float* rel, int ldr, int width,
                                        int32_t num_nodes, int32_t num_relations, const int64_t* s, const int64_t* r, const int64_t* o,
                                        int64_t n_triples, const float* dq, int lddq, const uint32_t* node_ptr, const uint32_t* node_slot,
                                        const uint32_t* rel_ptr, const uint32_t* rel_triple, float* dz, int lddz, float* drel, int lddrel,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_triples > 0 && (!s || !r || !o || !dq)) return RGCN_ERR_NULL;
    if (n_triples > 0 && dz && (!node_ptr || !node_slot)) return RGCN_ERR_NULL;
    if (n_triples > 0 && drel && (!rel_ptr || !rel_triple)) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if ((st = check_decoder(decoder, width)) != RGCN_OK) return st;
    if ((st = rgcn::check_stride(lddq, width)) != RGCN_OK) return st;
    if (dz && (st = rgcn::check_stride(lddz, width)) != RGCN_OK) return st;
    if (drel && (st = rgcn::check_stride(lddrel, width)) != RGCN_OK) return st;
    if (!aligned16(dq) || !aligned16(dz) || !aligned16(drel)) return RGCN_ERR_STRIDE;
    if (n_triples < 0 || (side != 0 && side != 1)) return RGCN_ERR_ARG;
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
    QbArgs a{};
    a.b.z = z;
    a.b.rel = rel;
    a.b.s = s;
    a.b.r = r;
    a.b.o = o;
    a.b.node_ptr = node_ptr;
    a.b.node_slot = node_slot;
    a.b.rel_ptr = rel_ptr;
    a.b.rel_triple = rel_triple;
    a.b.chunk_ptr = bb.chunk_ptr;
    a.b.partial = bb.partial;
    a.b.dz = dz;
    a.b.drel = drel;
    a.b.max_chunks = bb.max_chunks;
    a.b.num_nodes = num_nodes;
    a.b.num_relations = num_relations;
    a.b.ldz = ldz;
    a.b.ldr = ldr;
    a.b.lddz = lddz;
    a.b.lddrel = lddrel;
    a.b.gr = group_of(width);
    a.dq = dq;
    a.lddq = lddq;
    a.decoder = decoder;
    a.side = side;
    auto row_grid = [&](u64 rows) { return dim3((unsigned)(((rows + (u64)a.b.gr.per_wave - 1) / (u64)a.b.gr.per_wave + 3) / 4)); };
    if (dz && num_nodes > 0) hipLaunchKernelGGL(lpsm_dz_kernel, row_grid((u64)num_nodes), dim3(256), 0, q, a);
    if (drel && num_relations > 0) {
        hipLaunchKernelGGL(lp_chunk_ptr_kernel, dim3(1), dim3(kScanThreads), 0, q, rel_ptr, (int)num_relations, bb.chunk_ptr);
        hipLaunchKernelGGL(lpsm_drel_chunk_kernel, dim3((bb.max_chunks + 3) / 4), dim3(256), 0, q, a);
        hipLaunchKernelGGL(lp_drel_sum_kernel, row_grid((u64)num_relations), dim3(256), 0, q, a.b);
    }
    return (int)hipGetLastError();
}

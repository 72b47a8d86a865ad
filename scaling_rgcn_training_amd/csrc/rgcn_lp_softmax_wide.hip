// rgcn_lp_softmax_wide.hip -- the softmax (1-N) link-prediction loss of rgcn_lp_softmax.hip on DistMult rows of up to 512 columns,
// behind the C ABI rgcn_lpsmw_* of include/rgcn_mi355x.h.  gfx950 only.  DESIGN.md section 24 has the work split, the LDS and register
// budgets and the summation orders; the conventions are section 18's, the row layout and the slab geometry section 21's, the online
// pair and the transposed first product section 23's.
//
//   lpsmw_query_kernel    qrows = z[anchor] o rel[r]: one wave per row, lane l owns the 16-byte pieces l and l + 64.
//   lpsmw_sweep_kernel    SW (64 up to 256 columns, 32 above) query rows in dynamic LDS; entity rows streamed 16 per wave in slabs of
//                         128 columns, the next slab's loads issued before this slab's v_mfma_f32_16x16x4_f32 steps; an online
//                         (max, sum) pair per accumulator element; pairs merged lanes -> waves -> slices (lpsmw_finish_kernel, which
//                         also scores the targets by the same chain of steps).
//   lpsmw_grad_kernel     ONE body for dq (queries stationary) and dz (entity rows stationary).  A workgroup step covers 8 streamed
//                         tiles in two phases: each wave contracts ITS tile with the SW stationary rows over all slabs (transposed, so
//                         the result lies as the second product's A operand), makes the weights and writes them to its LDS slab; after
//                         a barrier each wave multiplies ALL eight weight slabs by ITS eighth of the columns of the 128 streamed rows.
//                         A wave's accumulator is SW x (width / 8) for the whole sweep and is stored by the wave itself.
//   lpsmw_dz_kernel / lpsmw_drel_*    lpw_dz_kernel / lpw_drel_* of rgcn_linkpred_wide.hip with a row of dq where they have a scalar g.
// No float atomics anywhere (one integer atomicOr into the `bad` word): the same inputs give the same bits.
#include "rgcn_kernels_shared.h"
#include "rgcn_lp_shared.h"

namespace rgcn_lpsmw {

using namespace rgcn_lp;

constexpr int kMaxWidth = RGCN_XWIDE_MAX_WIDTH;
constexpr int kMaxPieces = kMaxWidth / 4;
constexpr int kChunkWaves = 4;               // waves that share a chunk of a relation's triples
constexpr int kSlabSteps = 8;                // a slab: eight steps of 16 columns, 128 columns, eight f32x4 per lane
constexpr int kSplitWidth = 256;             // rows wider than this: 32 stationary rows per workgroup

// a table of fp32 rows as the sweeps read it
struct Table {
    const float* base;
    int ld, width, k16;
};

static Table table_of(const float* base, int ld, int width) { return Table{base, ld, width, (width + 15) / 16}; }

// ------------------------------------------------------------------------------------------------
// the slab helpers of rgcn_linkpred_wide.hip, re-stated on a Table
// ------------------------------------------------------------------------------------------------
// load_slab: the pieces 128 sl + 16 c + 4 kq of row `row`, ISSUED and not waited for (rgcn::prefetch16); nothing touches zf before
// wait_slab.  No lane is predicated: `row` is a row of the table (the callers clamp; what a clamped lane computes is never used) and
// a piece behind the row's last one is read from the last one (never multiplied, or zeroed by wait_slab).
__device__ __forceinline__ void load_slab(f32x4 (&zf)[kSlabSteps], const Table& t, int64_t row, int kq, int sl) {
    const float* base = t.base + row * (int64_t)t.ld;
    const int cmax = 4 * ((t.width + 3) / 4 - 1);
#pragma unroll
    for (int c = 0; c < kSlabSteps; ++c) {
        const int col = 16 * (kSlabSteps * sl + c) + 4 * kq;
        rgcn::prefetch16<0>(zf[c], (const f32x4*)(base + (col < cmax ? col : cmax)));
    }
}

// wait_slab: every load this wave has issued has landed; step k16 - 1 is the only one of a row that can hold pad columns or lie
// partly behind the width, so its pad elements become zeros here.
__device__ __forceinline__ void wait_slab(f32x4 (&zf)[kSlabSteps], const Table& t, int kq, int sl) {
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(zf[0]), "+v"(zf[1]), "+v"(zf[2]), "+v"(zf[3]), "+v"(zf[4]), "+v"(zf[5]), "+v"(zf[6]), "+v"(zf[7])::"memory");
    if (kSlabSteps * (sl + 1) < t.k16) return;   // (wave-uniform) the row's last step lies in a later slab
#pragma unroll
    for (int c = 0; c < kSlabSteps; ++c) {
        const int cc = kSlabSteps * sl + c, col = 16 * cc + 4 * kq;
        if (cc == t.k16 - 1) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            zf[c] = col < t.width ? mask_pad(zf[c], col, t.width) : zero;
        }
    }
}

// tile_step: THE logit, one slab of it.  Every element of the 16 x 16 tile is its own chain of MFMA steps over (sl, c, j) in that
// order.  Forward form: acc[r] = logit(stationary 16 qt + 4 kq + r, the streamed row lane rl loaded).  TRANSPOSED (the gradient
// sweep): the operands swapped, acc[r] = logit(stationary 16 qt + rl, streamed row 4 kq + r), the same chain per element.
template <int SW, bool TRANSPOSED>
__device__ __forceinline__ void tile_step(f32x4& acc, const f32x4* q4, int qt, int sl, int rl, int kq, const f32x4 (&zf)[kSlabSteps],
                                          int k16) {
    const f32x4* q = q4 + (4 * kSlabSteps * sl + kq) * SW + 16 * qt + rl;
#pragma unroll
    for (int c = 0; c < kSlabSteps; ++c) {
        if (kSlabSteps * sl + c < k16) {         // (wave-uniform)
            const f32x4 qa = q[4 * c * SW];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc = TRANSPOSED ? __builtin_amdgcn_mfma_f32_16x16x4f32(zf[c][j], qa[j], acc, 0, 0, 0)
                                 : __builtin_amdgcn_mfma_f32_16x16x4f32(qa[j], zf[c][j], acc, 0, 0, 0);
        }
    }
}

// SW rows of a table as the q4 image: q4[(4 c + kq) * SW + row] is the 16-byte piece 4 c + kq of a row; rows past `rows` and pad
// columns zero
template <int SW>
__device__ __forceinline__ void load_image(f32x4* q4, const Table& t, int64_t rows, int64_t row0) {
    for (int i = threadIdx.x; i < t.k16 * 4 * SW; i += blockDim.x) {
        const int pc = i / SW, qi = i - pc * SW, col = 4 * pc;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + qi < rows && col < t.width) v = mask_pad(piece(t.base, row0 + qi, t.ld, col), col, t.width);
        q4[i] = v;
    }
}

// section 23's merge of two (max, sum) pairs: symmetric bit for bit (two rounded products, one rounded sum); an empty set is (-inf, 0)
__device__ __forceinline__ void merge_pair(float& ma, float& sa, float mb, float sb) {
    const float m = __builtin_fmaxf(ma, mb);
    const float ea = ma == m ? 1.f : expf(ma - m), eb = mb == m ? 1.f : expf(mb - m);
    sa = __fadd_rn(__fmul_rn(sa, ea), __fmul_rn(sb, eb));
    ma = m;
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
    int num_nodes, num_relations, ldz, ldr, ldq, width, width4;
};

__global__ void __launch_bounds__(256) lpsmw_query_kernel(const QueryArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 t = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.n) return;                        // (wave-uniform)
    const int64_t an = a.a[t], rn = a.r[t], en = a.e[t];
    const int flags = id_flags(an, rn, en, a.num_nodes, a.num_relations);
    if (flags != 0 && lane == 0 && a.bad != nullptr) atomicOr(a.bad, flags);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h, c0 = 4 * p;
        if (p < a.width4) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (flags == 0) v = mask_pad(piece(a.z, an, a.ldz, c0) * piece(a.rel, rn, a.ldr, c0), c0, a.width);
            *(f32x4*)(a.q + (int64_t)t * a.ldq + c0) = v;
        }
    }
    if (lane == 0) a.qtarget[t] = flags == 0 ? en : (int64_t)-1;
}

// ------------------------------------------------------------------------------------------------
// b. forward: online log-sum-exp over the slab sweep
// ------------------------------------------------------------------------------------------------
struct FwdArgs {
    Table z, q;
    const int64_t* target;
    float2* part;              // [slices][qpad] (workspace): (max, sum) of a (query, slice)
    float* lse;
    float* tlogit;
    float* loss;
    int64_t nq, qpad;
    int num_nodes, slices;
};

template <int SW>
__global__ void __launch_bounds__(kRankThreads) __attribute__((amdgpu_waves_per_eu(SW == 32 ? 4 : 2))) lpsmw_sweep_kernel(const FwdArgs a) {
    constexpr int QT = SW / 16;
    extern __shared__ f32x4 q4[];                // [4 k16][SW]; after the sweep the waves' pairs, [2][kRankWaves][SW] floats
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * SW;
    load_image<SW>(q4, a.q, a.nq, q0);
    __syncthreads();

    const float ninf = -__builtin_inff();
    float m[QT][4], s[QT][4];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            m[qt][r] = ninf;
            s[qt][r] = 0.f;
        }
    }
    const int64_t tiles = ((int64_t)a.num_nodes + 15) / 16;
    const int64_t step = (int64_t)gridDim.y * kRankWaves;
    // the row of tile t this lane loads: past the last row or the last tile it loads row 0 again, and is no logit
    auto row_of = [&](int64_t t) { return (t < tiles && t * 16 + rl < (int64_t)a.num_nodes) ? t * 16 + rl : (int64_t)0; };
    const int ns = (a.z.k16 + kSlabSteps - 1) / kSlabSteps;
    f32x4 cur[kSlabSteps], nxt[kSlabSteps];
    int64_t t = (int64_t)blockIdx.y * kRankWaves + wave;
    if (t < tiles) {
        load_slab(cur, a.z, row_of(t), kq, 0);
        wait_slab(cur, a.z, kq, 0);
    }
    for (; t < tiles; t += step) {
        const bool valid = t * 16 + rl < (int64_t)a.num_nodes;       // a row past N is no logit at all (not a logit of 0)
        f32x4 acc[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int sl = 0; sl < ns; ++sl) {
            // the next slab of this tile, or the first of the wave's next tile, is on its way while this one is multiplied
            const bool more = sl + 1 < ns;
            load_slab(nxt, a.z, row_of(more ? t : t + step), kq, more ? sl + 1 : 0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                tile_step<SW, false>(acc[qt], q4, qt, sl, rl, kq, cur, a.z.k16);
                __builtin_amdgcn_sched_barrier(0);
            }
            wait_slab(nxt, a.z, kq, more ? sl + 1 : 0);
#pragma unroll
            for (int c = 0; c < kSlabSteps; ++c) cur[c] = nxt[c];
        }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                // one exp per logit: e = exp(-|v - m|) rescales the sum when the max rises and is the new term when it does not
                const float d = acc[qt][r] - m[qt][r], e = expf(-__builtin_fabsf(d));
                const float up = d > 0.f ? __builtin_fmaf(s[qt][r], e, 1.f) : s[qt][r] + e;
                s[qt][r] = valid ? up : s[qt][r];
                m[qt][r] = valid ? __builtin_fmaxf(m[qt][r], acc[qt][r]) : m[qt][r];
            }
        }
    }
    // the sixteen lanes that share kq hold pairs of the same four queries per tile: a butterfly over them, then the waves in LDS,
    // over the image (every wave has left the sweep)
    __syncthreads();
    float* wm = (float*)q4;
    float* wsum = wm + kRankWaves * SW;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float mm = m[qt][r], ss = s[qt][r];
#pragma unroll
            for (int x = 1; x < 16; x <<= 1) {
                const float om = __shfl_xor(mm, x), os = __shfl_xor(ss, x);
                merge_pair(mm, ss, om, os);
            }
            if (rl == 0) {
                wm[wave * SW + 16 * qt + 4 * kq + r] = mm;
                wsum[wave * SW + 16 * qt + 4 * kq + r] = ss;
            }
        }
    }
    __syncthreads();
    if (tid < SW) {
        float mm = ninf, ss = 0.f;
        for (int w = 0; w < kRankWaves; ++w) merge_pair(mm, ss, wm[w * SW + tid], wsum[w * SW + tid]);      // waves in order
        a.part[(int64_t)blockIdx.y * a.qpad + q0 + tid] = make_float2(mm, ss);
    }
}

// one workgroup of four waves per SW queries: the targets' logits (wave = query tile, column rl of the tile is the target of query
// 16 wave + rl, the diagonal is kept) slab by slab through tile_step, then the slices' pairs in slice order
template <int SW>
__global__ void __launch_bounds__(256) lpsmw_finish_kernel(const FwdArgs a) {
    constexpr int QT = SW / 16;
    extern __shared__ f32x4 q4[];
    float* tl = (float*)(q4 + 4 * a.z.k16 * SW);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * SW;
    load_image<SW>(q4, a.q, a.nq, q0);
    __syncthreads();
    if (wave < QT && a.num_nodes > 0) {
        const int qi = 16 * wave + rl;
        const int64_t tg = q0 + qi < a.nq ? a.target[q0 + qi] : (int64_t)-1;
        const int64_t row = (tg >= 0 && tg < (int64_t)a.num_nodes) ? tg : (int64_t)0;      // (a void query's logit is not used)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        f32x4 zf[kSlabSteps];
        const int ns = (a.z.k16 + kSlabSteps - 1) / kSlabSteps;
#pragma unroll 1
        for (int sl = 0; sl < ns; ++sl) {
            load_slab(zf, a.z, row, kq, sl);
            wait_slab(zf, a.z, kq, sl);
            tile_step<SW, false>(acc, q4, wave, sl, rl, kq, zf, a.z.k16);
        }
        if (kq == (rl >> 2)) tl[qi] = pick4(acc, rl & 3);
    }
    __syncthreads();
    const int64_t q = q0 + tid;
    if (tid < SW && q < a.nq) {
        float mm = -__builtin_inff(), ss = 0.f;
        for (int y = 0; y < a.slices; ++y) {
            const float2 p = a.part[(int64_t)y * a.qpad + q];
            merge_pair(mm, ss, p.x, p.y);
        }
        const float lse = mm + logf(ss);
        const int64_t tg = a.target[q];
        const bool ok = tg >= 0 && tg < (int64_t)a.num_nodes;       // (a void query: loss 0, and the backward gives it no weight)
        a.lse[q] = lse;
        a.tlogit[q] = ok ? tl[tid] : 0.f;
        a.loss[q] = ok ? lse - tl[tid] : 0.f;
    }
}

// ------------------------------------------------------------------------------------------------
// c. gradient sweep: acc[SW stationary rows][width] += w . streamed, w a function of stationary . streamed^T
// ------------------------------------------------------------------------------------------------
struct GradArgs {
    Table a;                   // stationary table [na]: qrows (QSTAT) or z
    Table b;                   // streamed table [nb]: z (QSTAT) or qrows
    const float* lse;          // per query
    const float* g;
    const int64_t* target;
    float* out;                // [na][ldo], or slice y's partial rows at out + y slice_stride
    int64_t na, nb, nq;
    size_t slice_stride;
    int ldo, num_nodes;
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

// A workgroup step is the eight streamed tiles 8 T .. 8 T + 7; lane (rl, kq) of wave v:
//   phase 1   st[qt][r] = logit(stationary 16 qt + rl, row 4 kq + r of tile 8 T + v) by tile_step's TRANSPOSED form over all slabs;
//             w[qt][r] from it on the VALU.  w[qt] already lies as the A operand of the second product (row rl = stationary, k = kq,
//             step r <-> streamed row 4 kq + r): the lane writes it as ONE 16-byte piece to slab v, wslab[(v QT + qt) 64 + lane], and
//             the same lane of every wave reads it back from there (lane-linear both ways: no bank conflict).  A wave whose tile
//             lies past the table writes zeros.
//   phase 2   the wave owns the column tiles ct0 .. ct0 + nct - 1 (a contiguous eighth of the k16 tiles of 16 columns; at most CT).
//             For each tile u of the step: bc[ct][r] = column 16 (ct0 + ct) + rl of row 4 kq + r of tile u, read from L1 / L2 by
//             column (sixteen lanes read 64 consecutive bytes), and acc[qt][ct] += w_u[qt][r] x bc[ct][r] over r.
//   acc[qt][ct]  rows 16 qt + 4 kq + r, column 16 (ct0 + ct) + rl of the workgroup's SW x width result; lives for the whole sweep and
//             is stored by this wave: no merge of accumulators across the waves.
// Two barriers per step (after the weights are written, after they are read); the slabs are not double-buffered.  One workgroup per
// CU in both SW classes: under 128 VGPRs the SW = 32 body spilled 49 registers.
template <int SW, bool QSTAT>
__global__ void __launch_bounds__(kRankThreads) __attribute__((amdgpu_waves_per_eu(2))) lpsmw_grad_kernel(const GradArgs a) {
    constexpr int QT = SW / 16, CT = SW == 64 ? kSplitWidth / 16 / kRankWaves : kMaxWidth / 16 / kRankWaves;      // 2 column tiles, or 4
    extern __shared__ f32x4 q4[];                // [4 k16][SW], then the weight slabs [kRankWaves][QT][64]
    f32x4* wslab = q4 + 4 * a.a.k16 * SW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * SW;
    const int k16 = a.a.k16, width = a.a.width;
    load_image<SW>(q4, a.a, a.na, r0);
    __syncthreads();

    float sg[QT], sl_[QT];
    int64_t stg[QT];
    if (QSTAT) {
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) query_weights(a, r0 + 16 * qt + rl, sg[qt], sl_[qt], stg[qt]);
    }
    const int ct0 = wave * k16 / kRankWaves, nct = (wave + 1) * k16 / kRankWaves - ct0;
    f32x4 acc[QT][CT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[qt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int64_t tiles = (a.nb + 15) / 16, steps = (tiles + kRankWaves - 1) / kRankWaves;
    const int ns = (k16 + kSlabSteps - 1) / kSlabSteps;
    for (int64_t T = blockIdx.y; T < steps; T += gridDim.y) {        // (uniform over the workgroup: every wave meets every barrier)
        // ---- phase 1: this wave's tile against the stationary rows
        const int64_t t = T * kRankWaves + wave;
        f32x4 w[QT];
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) w[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < tiles) {                         // (wave-uniform)
            const int64_t row = t * 16 + rl;
            const int64_t rowc = row < a.nb ? row : (int64_t)0;      // (what a clamped lane loads only meets rows whose weight is 0)
            f32x4 st[QT];
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) st[qt] = f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 cur[kSlabSteps], nxt[kSlabSteps];
            load_slab(cur, a.b, rowc, kq, 0);
            wait_slab(cur, a.b, kq, 0);
#pragma unroll 1
            for (int sl = 0; sl < ns; ++sl) {
                const bool more = sl + 1 < ns;
                if (more) load_slab(nxt, a.b, rowc, kq, sl + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int qt = 0; qt < QT; ++qt) {
                    tile_step<SW, true>(st[qt], q4, qt, sl, rl, kq, cur, k16);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (more) {
                    wait_slab(nxt, a.b, kq, sl + 1);
#pragma unroll
                    for (int c = 0; c < kSlabSteps; ++c) cur[c] = nxt[c];
                }
            }
            if (QSTAT) {
#pragma unroll
                for (int qt = 0; qt < QT; ++qt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t n = t * 16 + 4 * kq + r;
                        w[qt][r] = n < a.nb ? weight(st[qt][r], sg[qt], sl_[qt], n == stg[qt]) : 0.f;
                    }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float tg_, tl_;
                    int64_t ttg;
                    query_weights(a, t * 16 + 4 * kq + r, tg_, tl_, ttg);
#pragma unroll
                    for (int qt = 0; qt < QT; ++qt) w[qt][r] = weight(st[qt][r], tg_, tl_, ttg == r0 + 16 * qt + rl);
                }
            }
        }
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) wslab[(wave * QT + qt) * 64 + lane] = w[qt];
        __syncthreads();

        // ---- phase 2: all eight weight slabs against this wave's columns of the 128 streamed rows
#pragma unroll 1
        for (int u = 0; u < kRankWaves; ++u) {
            const int64_t brow = (T * kRankWaves + u) * 16 + 4 * kq;
            if (brow - 4 * kq >= a.nb) break;    // (uniform) the tiles from here on lie past the table: their slabs hold zeros
            float bc[CT][4];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = 16 * (ct0 + ct) + rl;
                    bc[ct][r] = (ct < nct && brow + r < a.nb && col < width) ? a.b.base[(brow + r) * (int64_t)a.b.ld + col] : 0.f;
                }
            }
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
                const f32x4 wa = wslab[(u * QT + qt) * 64 + lane];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    if (ct < nct) {              // (wave-uniform)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[qt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[r], bc[ct][r], acc[qt][ct], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }

    // each wave stores its own columns; the pad columns of the last 16-byte piece +0, nothing behind it
    const int wpad = (width + 3) / 4 * 4;
    float* out = a.out + (size_t)blockIdx.y * a.slice_stride;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = r0 + 16 * qt + 4 * kq + r;
                const int col = 16 * (ct0 + ct) + rl;
                if (ct < nct && row < a.na && col < wpad) out[row * (int64_t)a.ldo + col] = col < width ? acc[qt][ct][r] : 0.f;
            }
}

// out[row] = the slices' partial rows added in slice order; one 16-byte piece per thread
__global__ void __launch_bounds__(256) lpsmw_slice_sum_kernel(const float* __restrict__ part, int slices, int64_t rows, int w4,
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
// d. from dq to the anchor rows and the relation rows, on the index of rgcn_lp_index_build (DESIGN.md 21b's walks)
// ------------------------------------------------------------------------------------------------
struct QbArgs {
    BwdArgs b;                 // (g and gr unused: the gradient of a triple is a row of dq, a row is two pieces per lane)
    const float* dq;
    int lddq, side, width, width4;
};

// one wave per node: dz[v] += sum over v's slots whose parity is the anchor end, in sorted order, of dq_t o rel[r_t]
__global__ void __launch_bounds__(256) lpsmw_dz_kernel(const QbArgs a) {
    const BwdArgs& b = a.b;
    const int lane = threadIdx.x & 63;
    const u64 v = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= (u64)b.num_nodes) return;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    bool any = false;
    const u32 end = b.node_ptr[v + 1];
    for (u32 j = b.node_ptr[v]; j < end; ++j) {
        const u32 slot = b.node_slot[j], t = slot >> 1;
        if ((int)(slot & 1u) != a.side) continue;
        const int64_t r = b.r[t];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            if (p < a.width4) acc[h] += piece(a.dq, t, a.lddq, 4 * p) * piece(b.rel, r, b.ldr, 4 * p);
        }
        any = true;
    }
    if (!any) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        if (p < a.width4) {
            float* at = b.dz + (int64_t)v * b.lddz + 4 * p;
            *(f32x4*)at = mask_pad(*(const f32x4*)at + acc[h], 4 * p, a.width);
        }
    }
}

// one workgroup per chunk: wave w takes the chunk's triples w, w + W, .. in order, then piece p of the chunk's row is wave 0's +
// wave 1's + .. + wave W-1's, added by thread p
__global__ void __launch_bounds__(64 * kChunkWaves) lpsmw_drel_chunk_kernel(const QbArgs a) {
    __shared__ f32x4 part[kChunkWaves][kMaxPieces];
    const BwdArgs& b = a.b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u32 unit = blockIdx.x;
    if (unit >= b.chunk_ptr[b.num_relations]) return;        // (uniform over the workgroup)
    u32 beg, end;
    lp_chunk_range(b, unit, beg, end);
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (u32 j = beg + (u32)wave; j < end; j += (u32)kChunkWaves) {
        const u32 t = b.rel_triple[j];
        const int64_t an = a.side == 0 ? b.s[t] : b.o[t];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            if (p < a.width4) acc[h] += piece(a.dq, t, a.lddq, 4 * p) * piece(b.z, an, b.ldz, 4 * p);
        }
    }
    part[wave][lane] = acc[0];
    part[wave][lane + 64] = acc[1];
    __syncthreads();
    if (tid < a.width4) {
        f32x4 sum = part[0][tid];
#pragma unroll
        for (int w = 1; w < kChunkWaves; ++w) sum += part[w][tid];
        *(f32x4*)(b.partial + ((size_t)unit * a.width4 + tid) * 4) = sum;
    }
}

// one wave per relation: its chunks' rows in ascending chunk order
__global__ void __launch_bounds__(256) lpsmw_drel_sum_kernel(const QbArgs a) {
    const BwdArgs& b = a.b;
    const int lane = threadIdx.x & 63;
    const u32 r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (u32)b.num_relations) return;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const u32 end = b.chunk_ptr[r + 1];
    for (u32 c = b.chunk_ptr[r]; c < end; ++c) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int p = lane + 64 * h;
            if (p < a.width4) acc[h] += *(const f32x4*)(b.partial + ((size_t)c * a.width4 + p) * 4);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int p = lane + 64 * h;
        if (p < a.width4) *(f32x4*)(b.drel + (int64_t)r * b.lddrel + 4 * p) = mask_pad(acc[h], 4 * p, a.width);
    }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static int check_stride_w(int ld, int width) {
    if (width < 1 || width > kMaxWidth) return RGCN_ERR_WIDTH;
    if ((ld % 4) != 0 || ld < ((width + 3) / 4) * 4) return RGCN_ERR_STRIDE;
    return RGCN_OK;
}

// two tables and their strides (the second may be NULL), the conventions every entry point shares
static int check_tables_w(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations) {
    int st;
    if ((st = check_stride_w(ldz, width)) != RGCN_OK) return st;
    if (rel != nullptr && (st = check_stride_w(ldr, width)) != RGCN_OK) return st;
    if (!aligned16(z) || !aligned16(rel)) return RGCN_ERR_STRIDE;
    if (num_nodes < 0 || num_relations < 0) return RGCN_ERR_ARG;
    if (num_relations > 65536) return RGCN_ERR_PLAN;
    return RGCN_OK;
}

static bool queries_fit(int64_t n) { return n >= 0 && n <= 0x7FFFFFFFll; }      // (a table of queries is streamed like one of nodes)
static bool width_ok(int width) { return width >= 1 && width <= kMaxWidth; }
static int ld4(int width) { return (width + 3) / 4 * 4; }
static int sw_of(int width) { return width > kSplitWidth ? 32 : 64; }
static int64_t blocks_of(int64_t rows, int sw) { return (rows + sw - 1) / sw; }

// slices of the sweep whose stationary table has `stat` rows and whose streamed table has `streamed`: a workgroup's step is eight
// tiles of 16 streamed rows in the forward and in the gradient sweep alike
static int64_t slices_of(int64_t stat, int64_t streamed, int sw) { return rank_slices(blocks_of(stat, sw), (int32_t)streamed, 16, kRankWaves); }

static size_t image_bytes(int width, int sw) { return sizeof(f32x4) * 4 * (size_t)((width + 15) / 16) * sw; }

static float2* take_fwd_bufs(Arena& ar, int64_t nq, int32_t num_nodes, int width) {
    const int sw = sw_of(width);
    return ar.take<float2>((size_t)slices_of(nq, num_nodes, sw) * (size_t)blocks_of(nq, sw) * sw);
}

struct GradBufs {
    float* pq;                 // [slices_q][nq][ld4]: only when the dq sweep is sliced
    float* pz;                 // [slices_z][num_nodes][ld4]: only when dz is wanted and its sweep is sliced
};

static GradBufs take_grad_bufs(Arena& ar, int64_t nq, int32_t num_nodes, int width, bool want_dz) {
    GradBufs b{};
    const int sw = sw_of(width);
    const int64_t sq = slices_of(nq, num_nodes, sw), sz = slices_of(num_nodes, nq, sw);
    if (sq > 1) b.pq = ar.take<float>((size_t)sq * (size_t)nq * ld4(width));
    if (want_dz && sz > 1) b.pz = ar.take<float>((size_t)sz * (size_t)num_nodes * ld4(width));
    return b;
}

template <int SW>
static int launch_forward(const FwdArgs& a, hipStream_t q) {
    const size_t lds = image_bytes(a.z.width, SW), lds_finish = lds + sizeof(float) * SW;
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024) e = rgcn::allow_full_lds<lpsmw_sweep_kernel<SW>>();
    if (e == hipSuccess && lds_finish > 64 * 1024) e = rgcn::allow_full_lds<lpsmw_finish_kernel<SW>>();
    if (e != hipSuccess) return (int)e;
    const dim3 grid((unsigned)blocks_of(a.nq, SW), (unsigned)a.slices);
    hipLaunchKernelGGL(lpsmw_sweep_kernel<SW>, grid, dim3(kRankThreads), lds, q, a);
    hipLaunchKernelGGL(lpsmw_finish_kernel<SW>, dim3(grid.x), dim3(256), lds_finish, q, a);
    return (int)hipGetLastError();
}

template <int SW, bool QSTAT>
static int launch_grad(GradArgs a, float* final_out, int final_ld, float* partial, hipStream_t q) {
    const int width = a.a.width;
    const int64_t slices = slices_of(a.na, a.nb, SW);
    if (slices > 1) {
        a.out = partial;
        a.ldo = ld4(width);
        a.slice_stride = (size_t)a.na * a.ldo;
    } else {
        a.out = final_out;
        a.ldo = final_ld;
        a.slice_stride = 0;
    }
    const size_t lds = image_bytes(width, SW) + sizeof(f32x4) * kRankWaves * (SW / 16) * 64;
    if (lds > 64 * 1024) {
        const hipError_t e = rgcn::allow_full_lds<lpsmw_grad_kernel<SW, QSTAT>>();
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)blocks_of(a.na, SW), (unsigned)slices);
    hipLaunchKernelGGL((lpsmw_grad_kernel<SW, QSTAT>), grid, dim3(kRankThreads), lds, q, a);
    const int st = (int)hipGetLastError();
    if (st != RGCN_OK || slices == 1) return st;
    const int w4 = ld4(width) / 4;
    hipLaunchKernelGGL(lpsmw_slice_sum_kernel, dim3(grid_for((u64)a.na * w4)), dim3(256), 0, q, partial, (int)slices, a.na, w4, final_out, final_ld);
    return (int)hipGetLastError();
}

template <int SW>
static int launch_backward(GradArgs a, const float* qrows, int ldq, const float* z, int ldz, int width, int32_t num_nodes, int64_t nq,
                           float* dq, int lddq, float* dz, int lddz, const GradBufs& gb, hipStream_t q) {
    a.a = table_of(qrows, ldq, width);
    a.na = nq;
    a.b = table_of(z, ldz, width);
    a.nb = num_nodes;
    const int st = launch_grad<SW, true>(a, dq, lddq, gb.pq, q);
    if (st != RGCN_OK || !dz || num_nodes == 0) return st;
    a.a = table_of(z, ldz, width);
    a.na = num_nodes;
    a.b = table_of(qrows, ldq, width);
    a.nb = nq;
    return launch_grad<SW, false>(a, dz, lddz, gb.pz, q);
}

}  // namespace rgcn_lpsmw

using namespace rgcn_lpsmw;

extern "C" int rgcn_lpsmw_query(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                                const int64_t* anchor, const int64_t* r, const int64_t* target, int64_t n_queries, float* qrows, int ldq,
                                int64_t* qtarget, int32_t* bad, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!anchor || !r || !target || !qrows || !qtarget)) return RGCN_ERR_NULL;
    int st = check_tables_w(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if ((st = check_stride_w(ldq, width)) != RGCN_OK) return st;
    if (!aligned16(qrows)) return RGCN_ERR_STRIDE;
    if (n_queries < 0) return RGCN_ERR_ARG;
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
    a.width = width;
    a.width4 = (width + 3) / 4;
    hipLaunchKernelGGL(lpsmw_query_kernel, dim3((unsigned)((a.n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_lpsmw_forward_workspace_bytes(int64_t n_queries, int32_t num_nodes, int width) {
    if (n_queries <= 0 || num_nodes < 0 || !width_ok(width) || !queries_fit(n_queries)) return 0;
    Arena ar(nullptr);
    take_fwd_bufs(ar, n_queries, num_nodes, width);
    return ar.bytes();
}

extern "C" int rgcn_lpsmw_forward(const float* qrows, int ldq, const float* z, int ldz, int width, int32_t num_nodes,
                                  const int64_t* target, int64_t n_queries, float* lse, float* tlogit, float* loss, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (!z) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!qrows || !target || !lse || !tlogit || !loss)) return RGCN_ERR_NULL;
    int st = check_tables_w(z, ldz, qrows, ldq, width, num_nodes, 0);
    if (st != RGCN_OK) return st;
    if (n_queries < 0) return RGCN_ERR_ARG;
    if (!queries_fit(n_queries)) return RGCN_ERR_PLAN;
    if (n_queries == 0) return RGCN_OK;
    Arena ar(workspace);
    float2* part = take_fwd_bufs(ar, n_queries, num_nodes, width);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    const int sw = sw_of(width);
    FwdArgs a{};
    a.z = table_of(z, ldz, width);
    a.q = table_of(qrows, ldq, width);
    a.target = target;
    a.part = part;
    a.lse = lse;
    a.tlogit = tlogit;
    a.loss = loss;
    a.nq = n_queries;
    a.qpad = blocks_of(n_queries, sw) * sw;
    a.num_nodes = num_nodes;
    a.slices = (int)slices_of(n_queries, num_nodes, sw);
    return sw == 32 ? launch_forward<32>(a, (hipStream_t)stream) : launch_forward<64>(a, (hipStream_t)stream);
}

extern "C" size_t rgcn_lpsmw_backward_workspace_bytes(int64_t n_queries, int32_t num_nodes, int width, int want_dz) {
    if (n_queries <= 0 || num_nodes < 0 || !width_ok(width) || !queries_fit(n_queries)) return 0;
    Arena ar(nullptr);
    take_grad_bufs(ar, n_queries, num_nodes, width, want_dz != 0);
    return ar.bytes();
}

extern "C" int rgcn_lpsmw_backward(const float* qrows, int ldq, const float* z, int ldz, int width, int32_t num_nodes,
                                   const int64_t* target, int64_t n_queries, const float* lse, const float* g, float* dq, int lddq,
                                   float* dz, int lddz, void* workspace, size_t workspace_bytes, void* stream) {
    if (!z) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!qrows || !target || !lse || !g || !dq)) return RGCN_ERR_NULL;
    int st = check_tables_w(z, ldz, qrows, ldq, width, num_nodes, 0);
    if (st != RGCN_OK) return st;
    if ((st = check_stride_w(lddq, width)) != RGCN_OK) return st;
    if (dz && (st = check_stride_w(lddz, width)) != RGCN_OK) return st;
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
    a.num_nodes = num_nodes;
    return sw_of(width) == 32 ? launch_backward<32>(a, qrows, ldq, z, ldz, width, num_nodes, n_queries, dq, lddq, dz, lddz, gb, q)
                              : launch_backward<64>(a, qrows, ldq, z, ldz, width, num_nodes, n_queries, dq, lddq, dz, lddz, gb, q);
}

extern "C" size_t rgcn_lpsmw_query_backward_workspace_bytes(int64_t n_triples, int32_t num_relations, int width) {
    if (n_triples <= 0 || num_relations < 0 || num_relations > 65536 || !width_ok(width) || !triples_fit(n_triples)) return 0;
    Arena ar(nullptr);
    take_bwd_bufs(ar, n_triples, num_relations, width);
    return ar.bytes();
}

extern "C" int rgcn_lpsmw_query_backward(int side, const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes,
                                         int32_t num_relations, const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples,
                                         const float* dq, int lddq, const uint32_t* node_ptr, const uint32_t* node_slot,
                                         const uint32_t* rel_ptr, const uint32_t* rel_triple, float* dz, int lddz, float* drel, int lddrel,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_triples > 0 && (!s || !r || !o || !dq)) return RGCN_ERR_NULL;
    if (n_triples > 0 && dz && (!node_ptr || !node_slot)) return RGCN_ERR_NULL;
    if (n_triples > 0 && drel && (!rel_ptr || !rel_triple)) return RGCN_ERR_NULL;
    int st = check_tables_w(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if ((st = check_stride_w(lddq, width)) != RGCN_OK) return st;
    if (dz && (st = check_stride_w(lddz, width)) != RGCN_OK) return st;
    if (drel && (st = check_stride_w(lddrel, width)) != RGCN_OK) return st;
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
    a.dq = dq;
    a.lddq = lddq;
    a.side = side;
    a.width = width;
    a.width4 = (width + 3) / 4;
    if (dz && num_nodes > 0) hipLaunchKernelGGL(lpsmw_dz_kernel, dim3(((unsigned)num_nodes + 3u) / 4u), dim3(256), 0, q, a);
    if (drel && num_relations > 0) {
        hipLaunchKernelGGL(lp_chunk_ptr_kernel, dim3(1), dim3(kScanThreads), 0, q, rel_ptr, (int)num_relations, bb.chunk_ptr);
        hipLaunchKernelGGL(lpsmw_drel_chunk_kernel, dim3(bb.max_chunks), dim3(64 * kChunkWaves), 0, q, a);
        hipLaunchKernelGGL(lpsmw_drel_sum_kernel, dim3(((unsigned)num_relations + 3u) / 4u), dim3(256), 0, q, a);
    }
    return (int)hipGetLastError();
}

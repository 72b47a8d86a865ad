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
// The lane groups, the relation-chunk kernels, the ranking body and the host checks live in rgcn_lp_shared.h, which rgcn_kge.hip
// (ComplEx, TransE) includes too.
#include "rgcn_lp_shared.h"

namespace rgcn_lp {

constexpr u64 kGolden = 0x9E3779B97F4A7C15ull, kNegMul = 0xD1B54A32D192ED03ull, kSideMul = 0x2545F4914F6CDD1Dull;

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

// (lp_chunk_ptr_kernel: rgcn_lp_shared.h)

// ------------------------------------------------------------------------------------------------
// c. backward (BwdArgs, lp_chunk_range / lp_chunk_store and lp_drel_sum_kernel: rgcn_lp_shared.h)
// ------------------------------------------------------------------------------------------------
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
    u32 beg, end;
    lp_chunk_range(a, unit, beg, end);
    const int sub = lane / a.gr.lanes, p = lane - sub * a.gr.lanes, c0 = 4 * p;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (sub < a.gr.per_wave) {
        for (u32 j = beg + (u32)sub; j < end; j += (u32)a.gr.per_wave) {
            const u32 t = a.rel_triple[j];
            acc += (a.g[t] * piece(a.z, a.s[t], a.ldz, c0)) * piece(a.z, a.o[t], a.ldz, c0);
        }
    }
    lp_chunk_store(a, unit, acc, sub, p);
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
// e. ranks (lp_rank_body: rgcn_lp_shared.h); DistMult's query row is z[a] o rel[r]
// ------------------------------------------------------------------------------------------------
template <int KT, bool TARGETS>
__global__ void __launch_bounds__(kRankThreads) lp_rank_kernel(const RankArgs a) {
    lp_rank_body<KT, TARGETS>(a, [&](int64_t an, int64_t rn, int col) { return piece(a.z, an, a.ldz, col) * piece(a.rel, rn, a.ldr, col); });
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

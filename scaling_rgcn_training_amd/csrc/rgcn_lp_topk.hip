// rgcn_lp_topk.hip -- the k best entities of every query (anchor, r, ?) / (?, r, anchor) behind the C ABI rgcn_lp_topk (DistMult) and
// rgcn_kge_topk (ComplEx) of include/rgcn_mi355x.h, with no [Q, N] score matrix anywhere.  gfx950 only.  DESIGN.md section 25 has the
// key order, the selection scheme and the argument why nothing is dropped and nothing hangs; the sweep's geometry, the query image and
// THE score function (lp_rank_rows, lp_score_tile) are section 18's, through rgcn_lp_shared.h: a returned score has the bits the rank
// kernels compare.
//
//   key                  one u64 per candidate: orderable(score) << 32 | (0xFFFFFFFF - id).  orderable is the monotone map of float
//                        bits to unsigned (-0 made +0 first), so a larger key is a better score or, at equal scores, a smaller id.
//                        Keys of different entities differ.  0 is the empty slot: below every real key (orderable(-inf) = 0x007FFFFF).
//                        EVERY ordering decision of both kernels compares keys; a NaN score makes no key.
//   topk_sweep_kernel    grid (query blocks of 64, entity slices), 8 waves, 16 entity rows per wave and step, as the rank sweep.  Per
//                        query in LDS: the k best keys so far, sorted (list), and a buffer of kBuf = 64 keys with an integer count.
//                        A lane compares its sixteen scores of a step with its queries' thresholds (the k-th key of the list, 0 until
//                        the list is full); a key above it is looked up in the query's filter list (a binary search), then takes a
//                        buffer slot by an LDS atomicAdd.  A slot at or past kBuf leaves the candidate PENDING in the lane's registers
//                        (the step's scores and a bit mask): its wave sweeps no further until the next round.  A round is at most
//                        kSteps steps, then the workgroup meets: barrier, every wave sorts list + buffer of the queries 8 apart that
//                        have a non-empty buffer (128 keys, two per lane, a bitonic network on shuffles), keeps the best k, clears
//                        the count; a second barrier that also ORs "tiles left or candidates pending" over the workgroup decides the
//                        exit for all waves at once.  Then the pending candidates retry against the risen thresholds.
//   topk_merge_kernel    one wave per query: the slices' lists, 64 keys at a time through the same network, to the final k; decodes
//                        ids and scores, writes the (-1, -inf) tails.
// No float atomics, no waiting on another wave but at the workgroup barriers, the same number of barriers in every wave.
#include "rgcn_lp_shared.h"

namespace rgcn_topk {

using namespace rgcn_lp;

constexpr int kComplex = RGCN_KGE_COMPLEX;
constexpr int kMaxK = 64;
constexpr int kBuf = 64;                     // buffered keys per query between two rounds: list + buffer is one wave's 128 keys
constexpr int kSteps = 8;                    // sweep steps of a round
constexpr u64 kNever = ~0ull;                // the threshold of a query that takes no candidate (past the end, an id out of range)

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

// ---- keys --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 make_key(float score, u32 low) {
    const u32 b = __float_as_uint(score + 0.0f);             // -0 -> +0
    const u32 ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((u64)ord << 32) | (u64)low;
}

__device__ __forceinline__ void decode_key(u64 key, int64_t& id, float& score) {
    const u32 ord = (u32)(key >> 32);
    id = key ? (int64_t)(0xFFFFFFFFu - (u32)key) : (int64_t)-1;
    score = key ? __uint_as_float((ord & 0x80000000u) ? (ord ^ 0x80000000u) : ~ord) : -__builtin_inff();
}

// The 128 keys (e0 of lane l: index l; e1: index 64 + l) of a wave, sorted descending over the index: a bitonic network, the partner
// of index i at distance j is i ^ j -- the lane's other register at j = 64, a shuffle below.
__device__ __forceinline__ void sort128(u64& e0, u64& e1, int lane) {
    for (int size = 2; size <= 128; size <<= 1) {
        for (int j = size >> 1; j >= 1; j >>= 1) {
            if (j == 64) {                       // (size 128: descending everywhere)
                const u64 hi = e0 > e1 ? e0 : e1, lo = e0 > e1 ? e1 : e0;
                e0 = hi;
                e1 = lo;
            } else {
                const u64 o0 = __shfl_xor(e0, j), o1 = __shfl_xor(e1, j);
                const bool lower = (lane & j) == 0;
                const bool max0 = lower == ((lane & size) == 0);                 // index lane
                const bool max1 = lower == (((64 + lane) & size) == 0);          // index 64 + lane
                e0 = ((e0 > o0) == max0) ? e0 : o0;
                e1 = ((e1 > o1) == max1) ? e1 : o1;
            }
        }
    }
}

struct TopkArgs {
    RankArgs b;                // z, rel, a, r, fptr, fidx, flen, nq, sizes and strides (e, tscore, greater, equal unused)
    u64* part;                 // [nq][slices][k] (workspace): the sorted list of a (query, slice)
    int64_t* ids;
    float* scores;
    int k, slices, side;
};

// The lane's candidates `pend` (bit 4 qt + r: query 16 qt + 4 kq + r, score sc[qt][r], entity 0xFFFFFFFF - low) go to their queries'
// buffers; the bits that found no slot come back.  A candidate at or below the threshold, or on the query's filter list, is gone.
// (The query tiles are unrolled so that sc stays in registers.)
__device__ __forceinline__ u32 place(const RankArgs& a, u32 pend, const f32x4 (&sc)[kRankTiles], u32 low, int kq, int64_t q0,
                                     const u64* thr_l, int* cnt_l, u64* buf) {
    u32 left = 0;
#pragma unroll
    for (int qt = 0; qt < kRankTiles; ++qt) {
        u32 m = (pend >> (4 * qt)) & 15u;
        while (m) {
            const int r = __ffs(m) - 1;
            m &= m - 1;
            const int qi = 16 * qt + 4 * kq + r;
            const u64 key = make_key(pick4(sc[qt], r), low);
            if (key <= thr_l[qi]) continue;
            if (a.fptr != nullptr) {
                const int64_t id = (int64_t)(0xFFFFFFFFu - low);
                int64_t lo = a.fptr[q0 + qi], end = a.fptr[q0 + qi + 1];
                if (lo < 0) lo = 0;
                if (end > a.flen) end = a.flen;
                int64_t hi = end;
                while (lo < hi) {
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (a.fidx[mid] < id) lo = mid + 1; else hi = mid;
                }
                if (lo < end && a.fidx[lo] == id) continue;
            }
            const int slot = atomicAdd(&cnt_l[qi], 1);
            if (slot < kBuf) buf[qi * kBuf + slot] = key; else left |= 1u << (4 * qt + r);
        }
    }
    return left;
}

template <int KT, class Query>
__device__ __forceinline__ void topk_body(const TopkArgs& ta, Query query) {
    __shared__ f32x4 q4[KT * 4 * kRankQueries];
    __shared__ u64 thr_l[kRankQueries];
    __shared__ int cnt_l[kRankQueries];
    extern __shared__ u64 keys_l[];              // list [64][k], then buffer [64][kBuf]
    const RankArgs& a = ta.b;
    const int k = ta.k;
    u64* list = keys_l;
    u64* buf = keys_l + kRankQueries * k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * kRankQueries;

    // the query rows, as lp_rank_body lays them out; the anchor is the only node id of a query
    for (int i = tid; i < KT * 4 * kRankQueries; i += kRankThreads) {
        const int pc = i / kRankQueries, qi = i - pc * kRankQueries, col = 4 * pc;
        const int64_t q = q0 + qi;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < a.nq && col < a.width) {
            const int64_t an = a.a[q], rn = a.r[q];
            if (id_flags(an, rn, an, a.num_nodes, a.num_relations) == 0) v = mask_pad(query(an, rn, col), col, a.width);
        }
        q4[i] = v;
    }
    for (int i = tid; i < kRankQueries * k; i += kRankThreads) list[i] = 0;
    if (tid < kRankQueries) {
        const int64_t q = q0 + tid;
        const bool ok = q < a.nq && id_flags(a.a[q], a.r[q], a.a[q], a.num_nodes, a.num_relations) == 0;
        thr_l[tid] = ok ? 0ull : kNever;
        cnt_l[tid] = 0;
    }
    __syncthreads();

    const int64_t tiles = ((int64_t)a.num_nodes + 15) / 16;
    const int64_t step = (int64_t)gridDim.y * kRankWaves;
    int64_t t = (int64_t)blockIdx.y * kRankWaves + wave;
    f32x4 zf[KT], zn[KT], sc[kRankTiles];
    u32 pend = 0, low = 0;
    if (t < tiles) lp_rank_rows(zn, a, t * 16 + rl < (int64_t)a.num_nodes ? t * 16 + rl : (int64_t)-1, kq);
    for (;;) {
        // ---- a round: the thresholds of this lane's sixteen queries, the pending candidates, then up to kSteps steps
        u64 th[kRankTiles][4];
#pragma unroll
        for (int qt = 0; qt < kRankTiles; ++qt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) th[qt][r] = thr_l[16 * qt + 4 * kq + r];
        }
        if (pend) pend = place(a, pend, sc, low, kq, q0, thr_l, cnt_l, buf);
        for (int s = 0; s < kSteps; ++s) {
            if (t >= tiles || __any((int)pend)) break;        // (t is the wave's: the branch is wave-uniform)
            const int64_t row = t * 16 + rl;
            const bool valid = row < (int64_t)a.num_nodes;
#pragma unroll
            for (int c = 0; c < KT; ++c) zf[c] = zn[c];
            t += step;
            if (t < tiles) lp_rank_rows(zn, a, t * 16 + rl < (int64_t)a.num_nodes ? t * 16 + rl : (int64_t)-1, kq);     // the next step's rows
            low = 0xFFFFFFFFu - (u32)row;
#pragma unroll
            for (int qt = 0; qt < kRankTiles; ++qt) {
                sc[qt] = lp_score_tile(q4, qt, rl, kq, zf, a.k16);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = sc[qt][r];
                    if (valid && v == v && make_key(v, low) > th[qt][r]) pend |= 1u << (4 * qt + r);
                }
            }
            if (pend) pend = place(a, pend, sc, low, kq, q0, thr_l, cnt_l, buf);
        }
        const int more = (t < tiles || pend != 0) ? 1 : 0;
        __syncthreads();
        // ---- the workgroup's meeting: list + buffer -> list, for the queries that buffered something
        for (int qi = wave; qi < kRankQueries; qi += kRankWaves) {
            const int n = cnt_l[qi] < kBuf ? cnt_l[qi] : kBuf;
            if (n == 0) continue;
            u64 e0 = lane < k ? list[qi * k + lane] : 0ull;
            u64 e1 = lane < n ? buf[qi * kBuf + lane] : 0ull;
            sort128(e0, e1, lane);
            if (lane < k) list[qi * k + lane] = e0;
            if (lane == k - 1) thr_l[qi] = e0;               // 0 while fewer than k candidates were seen
            if (lane == 0) cnt_l[qi] = 0;
        }
        if (!__syncthreads_or(more)) break;
    }
    for (int i = tid; i < kRankQueries * k; i += kRankThreads) {
        const int qi = i / k, j = i - qi * k;
        if (q0 + qi < a.nq) ta.part[((u64)(q0 + qi) * (u64)ta.slices + blockIdx.y) * (u64)k + (u64)j] = list[i];
    }
}

template <int KT>
__global__ void __launch_bounds__(kRankThreads) lp_topk_sweep_kernel(const TopkArgs a) {
    topk_body<KT>(a, [&](int64_t an, int64_t rn, int col) { return piece(a.b.z, an, a.b.ldz, col) * piece(a.b.rel, rn, a.b.ldr, col); });
}

// ComplEx's query row as kge_complex_rank_kernel builds it.  Object side: s o r.  Subject side: conj(r) o o.
template <int KT>
__global__ void __launch_bounds__(kRankThreads) kge_topk_sweep_kernel(const TopkArgs a) {
    topk_body<KT>(a, [&](int64_t an, int64_t rn, int col) {
        const f32x4 x = piece(a.b.z, an, a.b.ldz, col), y = piece(a.b.rel, rn, a.b.ldr, col);
        return a.side == 0 ? cmul(x, y) : cmulc(y, x);
    });
}

// one wave per query; a chunk of 64 keys that holds nothing above the k-th key so far is passed over
__global__ void __launch_bounds__(256) topk_merge_kernel(const TopkArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= a.b.nq) return;
    const int64_t total = (int64_t)a.slices * a.k;
    const u64* p = a.part + (u64)q * (u64)total;
    u64 e0 = 0;
    for (int64_t base = 0; base < total; base += 64) {
        u64 e1 = base + lane < total ? p[base + lane] : 0ull;
        const u64 thr = __shfl(e0, a.k - 1);
        if (!__any(e1 > thr ? 1 : 0)) continue;
        sort128(e0, e1, lane);
    }
    if (lane < a.k) decode_key(e0, a.ids[q * a.k + lane], a.scores[q * a.k + lane]);
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// kge: the call has a decoder argument (rgcn_kge_topk); rgcn_lp_topk is DistMult
static int check_decoder(bool kge, int decoder, int width) {
    if (!kge) return RGCN_OK;
    if (decoder != kComplex) return RGCN_ERR_ARG;           // RGCN_KGE_TRANSE_L1 too: its sweep is not this one
    if (width >= 1 && width <= RGCN_MAX_WIDTH && (width & 1)) return RGCN_ERR_WIDTH;
    return RGCN_OK;
}

static unsigned slices_of(int64_t n_queries, int32_t num_nodes) {
    return (unsigned)rank_slices((n_queries + kRankQueries - 1) / kRankQueries, num_nodes, 16, kRankWaves);
}

static size_t workspace_bytes_of(bool kge, int decoder, int64_t n_queries, int32_t num_nodes, int width, int k) {
    if (n_queries <= 0 || num_nodes < 0 || width < 1 || width > RGCN_MAX_WIDTH || (u64)n_queries > kMaxKeys || k < 1 || k > kMaxK ||
        check_decoder(kge, decoder, width) != RGCN_OK)
        return 0;
    Arena ar(nullptr);
    ar.take<u64>((size_t)n_queries * slices_of(n_queries, num_nodes) * (size_t)k);
    return ar.bytes();
}

static int topk(bool kge, int decoder, int side, const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes,
                int32_t num_relations, const int64_t* anchor, const int64_t* r, int64_t n_queries, int k, const int64_t* filter_ptr,
                const int64_t* filter_idx, int64_t filter_len, int64_t* ids_out, float* scores_out, void* workspace,
                size_t workspace_bytes, void* stream) {
    if (!z || !rel) return RGCN_ERR_NULL;
    if (n_queries > 0 && (!anchor || !r || !ids_out || !scores_out)) return RGCN_ERR_NULL;
    if (filter_ptr != nullptr && filter_len > 0 && !filter_idx) return RGCN_ERR_NULL;
    int st = check_tables(z, ldz, rel, ldr, width, num_nodes, num_relations);
    if (st != RGCN_OK) return st;
    if ((st = check_decoder(kge, decoder, width)) != RGCN_OK) return st;
    if (n_queries < 0 || filter_len < 0 || (side != 0 && side != 1) || k < 1 || k > kMaxK) return RGCN_ERR_ARG;
    if ((u64)n_queries > kMaxKeys) return RGCN_ERR_PLAN;
    if (n_queries == 0) return RGCN_OK;
    const unsigned slices = slices_of(n_queries, num_nodes);
    Arena ar(workspace);
    u64* part = ar.take<u64>((size_t)n_queries * slices * (size_t)k);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    if ((st = rgcn::check_device()) != RGCN_OK) return st;
    hipStream_t q = (hipStream_t)stream;
    TopkArgs a;
    a.b.z = z;
    a.b.rel = rel;
    a.b.a = anchor;
    a.b.r = r;
    a.b.e = nullptr;
    a.b.fptr = filter_ptr;
    a.b.fidx = filter_idx;
    a.b.flen = filter_len;
    a.b.tscore = nullptr;
    a.b.greater = nullptr;
    a.b.equal = nullptr;
    a.b.nq = n_queries;
    a.b.num_nodes = num_nodes;
    a.b.num_relations = num_relations;
    a.b.width = width;
    a.b.ldz = ldz;
    a.b.ldr = ldr;
    a.b.k16 = (width + 15) / 16;
    a.part = part;
    a.ids = ids_out;
    a.scores = scores_out;
    a.k = k;
    a.slices = (int)slices;
    a.side = side;
    const dim3 grid((unsigned)((n_queries + kRankQueries - 1) / kRankQueries), slices);
    const size_t lds = sizeof(u64) * (size_t)kRankQueries * (size_t)(k + kBuf);
    auto launch = [&](auto kern, size_t image) -> int {
        hipError_t e = hipSuccess;
        if (image + lds + 1024 > 64 * 1024) e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(kern, grid, dim3(kRankThreads), lds, q, a);
        hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((n_queries + 3) / 4)), dim3(256), 0, q, a);
        return (int)hipGetLastError();
    };
    return rgcn::for_padded_width(rgcn::padded_width(width), [&](auto kp) {
        constexpr int KT = decltype(kp)::value / 16;
        constexpr size_t image = sizeof(f32x4) * KT * 4 * kRankQueries;
        return kge ? launch(kge_topk_sweep_kernel<KT>, image) : launch(lp_topk_sweep_kernel<KT>, image);
    });
}

}  // namespace rgcn_topk

using namespace rgcn_topk;

extern "C" size_t rgcn_lp_topk_workspace_bytes(int64_t n_queries, int32_t num_nodes, int width, int k) {
    return workspace_bytes_of(false, 0, n_queries, num_nodes, width, k);
}

extern "C" int rgcn_lp_topk(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                            const int64_t* anchor, const int64_t* r, int64_t n_queries, int k, const int64_t* filter_ptr,
                            const int64_t* filter_idx, int64_t filter_len, int64_t* ids_out, float* scores_out, void* workspace,
                            size_t workspace_bytes, void* stream) {
    return topk(false, 0, 0, z, ldz, rel, ldr, width, num_nodes, num_relations, anchor, r, n_queries, k, filter_ptr, filter_idx,
                filter_len, ids_out, scores_out, workspace, workspace_bytes, stream);
}

extern "C" size_t rgcn_kge_topk_workspace_bytes(int decoder, int64_t n_queries, int32_t num_nodes, int width, int k) {
    return workspace_bytes_of(true, decoder, n_queries, num_nodes, width, k);
}

extern "C" int rgcn_kge_topk(int decoder, int side, const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes,
                             int32_t num_relations, const int64_t* anchor, const int64_t* r, int64_t n_queries, int k,
                             const int64_t* filter_ptr, const int64_t* filter_idx, int64_t filter_len, int64_t* ids_out,
                             float* scores_out, void* workspace, size_t workspace_bytes, void* stream) {
    return topk(true, decoder, side, z, ldz, rel, ldr, width, num_nodes, num_relations, anchor, r, n_queries, k, filter_ptr, filter_idx,
                filter_len, ids_out, scores_out, workspace, workspace_bytes, stream);
}

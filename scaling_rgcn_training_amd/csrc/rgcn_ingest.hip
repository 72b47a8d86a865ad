// rgcn_ingest.hip -- N-Triples ingest behind the C ABI rgcn_nt_* of include/rgcn_mi355x.h: the bytes of an .nt file -> term
// (offset, length) triples -> node / relation / class ids in bytewise term order -> int64 COO, labelled nodes, multi-hot rows and
// the three term tables.  gfx950 only.  DESIGN.md section 20 has the contract (graphs.py's) and the phases.
//
//   rgcn_nt_lines      nt_count_kernel      16 bytes per lane: '\n' per 4,096-byte block, the first NUL, the last byte
//   rgcn_nt_tokenize   nt_count_kernel -> scan of the block counts -> nt_newlines_kernel (positions of the '\n' bytes) ->
//                      nt_tokenize_kernel   a wave per line: drops one '\r', skips lines of <= 2 bytes, cuts 2 bytes, finds the
//                                           first two spaces by ballots over 64-byte pieces (it stops at the second one: the
//                                           object, where the long literals are, is never walked)
//                      -> scan of the kept lines -> nt_compact_kernel: occurrence 3 t + role = (offset, length)
//   rgcn_nt_build      nt_hash_kernel       8 lanes per occurrence, 8 folded bytes per lane and step: sum of mix(piece + position)
//                      radix_sort_pairs by the low hash_bits bits, run ids = provisional term ids
//                      nt_verify_kernel     8 lanes per occurrence: length and bytes against the head of its run; any difference
//                                           is a collision: the call answers RGCN_ERR_COLLISION and merges nothing
//                      rank rounds          round j sorts the active terms by (group << 32 | folded bytes [4 j, 4 j + 4), big
//                                           endian, zero padded); a group id is the bytewise rank of the group's first term, a
//                                           run of equal keys becomes group + its offset inside the group, a run of one is final
//                                           and leaves the active set.  One read-back (the active count) per round.
//                      roles                integer atomics on per-rank flags, scans in rank order -> node / relation / class
//                                           ids; scan of the non-type triples; label flags per node id + scan
//   rgcn_nt_emit       edges in file order (forward 2 i, inverse 2 i + 1), tables, labelled ids, multi-hot rows.  No read-back.
// No id depends on the hash: it only groups candidates, verified byte by byte.  No float math.  All offsets are u32
// (num_bytes <= 0xFFFF0000); an (offset, length) pair that leaves the text is never used as an address.
#include "rgcn_common.h"
#include "rgcn_sort_scan.h"

namespace rgcn_nt {

using namespace rgcn_sort_scan;

constexpr int kByteItems = 16;                         // bytes per lane of the byte passes (one 16-byte load)
constexpr int kByteBlock = 256 * kByteItems;           // 4,096 bytes per workgroup
constexpr int kGroup = 8;                              // lanes per occurrence in the hash / verify kernels
constexpr u32 kNone = 0xFFFFFFFFu;
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;
constexpr u32 kPredRdfType = 1, kPredType = 2;         // pred_kind values; 0: a message-passing predicate
constexpr u32 kStatusCollision = 1, kStatusBadOcc = 2;

__constant__ char kRdfType[] = "<http://www.w3.org/1999/02/22-rdf-syntax-ns#type>";
__constant__ char kType[] = "<type>";
__constant__ char kOntology[] = "http://swrc.ontoware.org/ontology";
constexpr u32 kRdfTypeLen = 49, kTypeLen = 6, kOntologyLen = 33;

__device__ __forceinline__ u32 fold(u32 b) { return b + ((b - 65u) < 26u ? 32u : 0u); }      // 'A'..'Z' -> 'a'..'z'

// device words of the tokenizer / of a build
struct TokInfo { u32 newlines, nul_pos, last_is_nl, bad_line, nul_line, max_len, triples, pad; };
struct BuildInfo { u32 status, distinct, nodes, relations, classes, half_edges, labelled, pad; };

// ---- lines ---------------------------------------------------------------------------------------------------------------------
// 16 consecutive bytes of the text as four little-endian words; bytes past the end read as 0x01 (neither '\n' nor NUL)
__device__ __forceinline__ void load16(const uint8_t* __restrict__ text, u64 base, u64 n, int vec, u32 w[4]) {
    if (vec && base + kByteItems <= n) {
        const uint4 v = *(const uint4*)(text + base);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u32 x = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const u64 i = base + (u64)(4 * q + k);
                x |= (i < n ? (u32)text[i] : 1u) << (8 * k);
            }
            w[q] = x;
        }
    }
}

__device__ __forceinline__ u32 byte_of(const u32 w[4], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

// block_cnt[b] = '\n' bytes of block b (may be NULL); info: newlines, the first NUL, whether the last byte is '\n'
__global__ void __launch_bounds__(256) nt_count_kernel(const uint8_t* __restrict__ text, u64 n, int vec, u32* __restrict__ block_cnt,
                                                       TokInfo* __restrict__ info) {
    __shared__ u32 wt[kScanThreads / 64];
    const u64 base = (u64)blockIdx.x * kByteBlock + (u64)threadIdx.x * kByteItems;
    u32 w[4];
    load16(text, base, n, vec, w);
    u32 cnt = 0, nul = kNone;
#pragma unroll
    for (int k = kByteItems - 1; k >= 0; --k) {
        const u32 b = byte_of(w, k);
        cnt += b == 10u ? 1u : 0u;
        if (b == 0u) nul = (u32)(base + k);
    }
    if (nul != kNone) atomicMin(&info->nul_pos, nul);
    if (base < n && base + kByteItems >= n && byte_of(w, (int)(n - 1 - base)) == 10u) info->last_is_nl = 1u;
    u32 tot;
    block_exclusive_scan(cnt, wt, tot);
    if (threadIdx.x == 0) {
        if (block_cnt != nullptr) block_cnt[blockIdx.x] = tot;
        if (tot != 0u) atomicAdd(&info->newlines, tot);
    }
}

// nl_pos[i] = byte offset of the i-th '\n' (i < cap); block_base = exclusive scan of the block counts
__global__ void __launch_bounds__(256) nt_newlines_kernel(const uint8_t* __restrict__ text, u64 n, int vec,
                                                          const u32* __restrict__ block_base, u32* __restrict__ nl_pos, u32 cap) {
    __shared__ u32 wt[kScanThreads / 64];
    const u64 base = (u64)blockIdx.x * kByteBlock + (u64)threadIdx.x * kByteItems;
    u32 w[4];
    load16(text, base, n, vec, w);
    u32 cnt = 0;
#pragma unroll
    for (int k = 0; k < kByteItems; ++k) cnt += byte_of(w, k) == 10u ? 1u : 0u;
    u32 tot;
    u32 at = block_exclusive_scan(cnt, wt, tot) + block_base[blockIdx.x];
    if (cnt == 0u) return;
#pragma unroll
    for (int k = 0; k < kByteItems; ++k)
        if (byte_of(w, k) == 10u) {
            if (at < cap) nl_pos[at] = (u32)(base + k);
            ++at;
        }
}

// ---- tokens --------------------------------------------------------------------------------------------------------------------
// a wave per line.  tok[4 l ..] = start, first space, second space, end (after the cut); keep[l] = 1 for a triple
__global__ void __launch_bounds__(256) nt_tokenize_kernel(const uint8_t* __restrict__ text, u64 n, const u32* __restrict__ nl_pos,
                                                          u32 num_lines, u32* __restrict__ tok, u32* __restrict__ keep,
                                                          TokInfo* __restrict__ info) {
    const int lane = threadIdx.x & 63;
    const u64 line = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (line >= (u64)num_lines) return;                    // (whole waves leave together)
    const u32 l = (u32)line;
    const u32 nnl = info->newlines < num_lines ? info->newlines : num_lines;
    u32 kept = 0;
    if (l <= nnl) {                                        // (a line count that does not match the text: the ABI call refuses after)
        const u64 start = l == 0 ? 0ull : (u64)nl_pos[l - 1] + 1ull;
        u64 end = l < nnl ? (u64)nl_pos[l] : n;
        const u64 past = l < nnl ? end + 1ull : end;       // the line with its '\n'
        const u64 nul = info->nul_pos;
        if (lane == 0 && info->nul_pos != kNone && nul >= start && nul < past) atomicMin(&info->nul_line, l + 1u);
        if (end > start && text[end - 1] == 13u) --end;
        if (end > start + 2ull) {
            end -= 2ull;
            u64 sp1 = ~0ull, sp2 = ~0ull;
            for (u64 c = start; c < end && sp2 == ~0ull; c += 64ull) {
                const u64 i = c + (u64)lane;
                u64 m = __ballot(i < end && text[i] == 32u);
                if (sp1 == ~0ull && m != 0ull) {
                    sp1 = c + (u64)(__ffsll((long long)m) - 1);
                    m &= m - 1ull;
                }
                if (sp1 != ~0ull && m != 0ull) sp2 = c + (u64)(__ffsll((long long)m) - 1);
            }
            if (sp2 == ~0ull) {
                if (lane == 0) atomicMin(&info->bad_line, l + 1u);
            } else {
                kept = 1;
                if (lane == 0) {
                    tok[4 * (size_t)l] = (u32)start;
                    tok[4 * (size_t)l + 1] = (u32)sp1;
                    tok[4 * (size_t)l + 2] = (u32)sp2;
                    tok[4 * (size_t)l + 3] = (u32)end;
                    const u64 a = sp1 - start, b = sp2 - sp1 - 1ull, c = end - sp2 - 1ull;
                    const u64 mx = a > b ? (a > c ? a : c) : (b > c ? b : c);
                    atomicMax(&info->max_len, (u32)mx);
                }
            }
        }
    }
    if (lane == 0) keep[l] = kept;
}

__global__ void __launch_bounds__(256) nt_compact_kernel(const u32* __restrict__ tok, const u32* __restrict__ keep,
                                                         const u32* __restrict__ pos, u32 num_lines, u32* __restrict__ occ_off,
                                                         u32* __restrict__ occ_len) {
    const u32 l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= num_lines || keep[l] == 0u) return;
    const size_t t = pos[l];                               // (< num_lines: the outputs hold 3 num_lines entries)
    const u32 start = tok[4 * (size_t)l], sp1 = tok[4 * (size_t)l + 1], sp2 = tok[4 * (size_t)l + 2], end = tok[4 * (size_t)l + 3];
    occ_off[3 * t] = start;
    occ_len[3 * t] = sp1 - start;
    occ_off[3 * t + 1] = sp1 + 1u;
    occ_len[3 * t + 1] = sp2 - sp1 - 1u;
    occ_off[3 * t + 2] = sp2 + 1u;
    occ_len[3 * t + 2] = end - sp2 - 1u;
}

__global__ void nt_store_kernel(const u32* __restrict__ src, u32* __restrict__ dst) { *dst = *src; }

// ---- distinct terms ------------------------------------------------------------------------------------------------------------
struct Text {
    const uint8_t* p;
    u64 n;
};

// the (offset, length) of occurrence o; a pair that leaves the text becomes the empty term and sets kStatusBadOcc
__device__ __forceinline__ void occ_load(const Text tx, const u32* __restrict__ occ_off, const u32* __restrict__ occ_len, u32 o,
                                         u32& off, u32& len, u32* status) {
    off = occ_off[o];
    len = occ_len[o];
    if ((u64)off + (u64)len > tx.n) {
        if (status != nullptr) atomicOr(status, kStatusBadOcc);
        off = 0;
        len = 0;
    }
}

// 8 folded bytes of a term from byte `at`, little endian, zero padded past the end
__device__ __forceinline__ u64 piece8(const uint8_t* __restrict__ t, u32 len, u32 at) {
    u64 w = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const u32 i = at + (u32)k;
        if (i < len) w |= (u64)fold(t[i]) << (8 * k);
    }
    return w;
}

// 4 folded bytes of a term from byte `at`, BIG endian (integer order = bytewise order), zero padded past the end
__device__ __forceinline__ u32 piece4_be(const uint8_t* __restrict__ t, u32 len, u64 at) {
    u32 w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u64 i = at + (u64)k;
        w = (w << 8) | (i < (u64)len ? fold(t[i]) : 0u);
    }
    return w;
}

// (the grids of the two group kernels cover n_occ rounded up to whole waves: no early return before the shuffles)
__global__ void __launch_bounds__(256) nt_hash_kernel(const Text tx, const u32* __restrict__ occ_off, const u32* __restrict__ occ_len,
                                                      u32 n_occ, u64 seed_key, u64 mask, u64* __restrict__ keys, u32* __restrict__ vals,
                                                      u32* __restrict__ status) {
    const u64 unit = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    const int g = threadIdx.x & (kGroup - 1);
    const bool live = unit < (u64)n_occ;
    u32 off = 0, len = 0;
    if (live) occ_load(tx, occ_off, occ_len, (u32)unit, off, len, g == 0 ? status : nullptr);
    const uint8_t* t = tx.p + off;
    u64 acc = 0;
    for (u32 at = 8u * (u32)g; at < len; at += 8u * kGroup) acc += mix(piece8(t, len, at) + seed_key + kGolden * (u64)(at / 8u + 1u));
#pragma unroll
    for (int d = 1; d < kGroup; d <<= 1) acc += __shfl_xor(acc, d);
    if (live && g == 0) {
        keys[unit] = mix(acc + seed_key + (u64)len) & mask;
        vals[unit] = (u32)unit;
    }
}

// heads of the sorted runs: rep[run] = the run's first occurrence (the earliest in the file: the sort is stable)
__global__ void __launch_bounds__(256) nt_rep_kernel(const u32* __restrict__ vals, const u32* __restrict__ flag,
                                                     const u32* __restrict__ ids, u32 n_occ, u32* __restrict__ rep) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_occ && flag[p] != 0u) rep[ids[p]] = vals[p];
}

__global__ void __launch_bounds__(256) nt_verify_kernel(const Text tx, const u32* __restrict__ occ_off, const u32* __restrict__ occ_len,
                                                        const u32* __restrict__ vals, const u32* __restrict__ ids,
                                                        const u32* __restrict__ rep, u32 n_occ, u32* __restrict__ term_of_occ,
                                                        u32* __restrict__ status) {
    const u64 unit = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
    const int g = threadIdx.x & (kGroup - 1);
    if (unit >= (u64)n_occ) return;                        // (no cross-lane traffic below)
    const u32 o = vals[unit], id = ids[unit];
    if (o >= n_occ) return;
    const u32 h = rep[id];
    if (g == 0) term_of_occ[o] = id;
    if (h == o || h >= n_occ) return;
    u32 off_a, len_a, off_b, len_b;
    occ_load(tx, occ_off, occ_len, o, off_a, len_a, nullptr);
    occ_load(tx, occ_off, occ_len, h, off_b, len_b, nullptr);
    bool differ = len_a != len_b;
    if (!differ) {
        const uint8_t *a = tx.p + off_a, *b = tx.p + off_b;
        for (u32 at = 8u * (u32)g; at < len_a && !differ; at += 8u * kGroup) differ = piece8(a, len_a, at) != piece8(b, len_a, at);
    }
    if (differ) atomicOr(status, kStatusCollision);
}

// ---- bytewise ranks ------------------------------------------------------------------------------------------------------------
// per distinct term: its representative's (offset, length), whether it is one of the two type predicates, whether the class
// filter fires on it as a subject, and its key of round 0
__global__ void __launch_bounds__(256) nt_terms_kernel(const Text tx, const u32* __restrict__ occ_off, const u32* __restrict__ occ_len,
                                                       const u32* __restrict__ rep, u32 n_terms, u32 n_occ, u32* __restrict__ term_off,
                                                       u32* __restrict__ term_len, u32* __restrict__ pred_kind, u32* __restrict__ onto,
                                                       u64* __restrict__ keys, u32* __restrict__ vals) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_terms) return;
    const u32 o = rep[i];
    u32 off = 0, len = 0;
    if (o < n_occ) occ_load(tx, occ_off, occ_len, o, off, len, nullptr);
    const uint8_t* t = tx.p + off;
    term_off[i] = off;
    term_len[i] = len;
    u32 kind = 0;
    if (len == kRdfTypeLen) {
        bool eq = true;
        for (u32 k = 0; k < kRdfTypeLen && eq; ++k) eq = fold(t[k]) == (u32)(uint8_t)kRdfType[k];
        if (eq) kind = kPredRdfType;
    } else if (len == kTypeLen) {
        bool eq = true;
        for (u32 k = 0; k < kTypeLen && eq; ++k) eq = fold(t[k]) == (u32)(uint8_t)kType[k];
        if (eq) kind = kPredType;
    }
    pred_kind[i] = kind;
    // s.split("#")[0] == ONTOLOGY_PREFIX: the prefix, then the end of the term or '#'
    bool on = len >= kOntologyLen && (len == kOntologyLen || t[kOntologyLen] == 35u);
    for (u32 k = 0; k < kOntologyLen && on; ++k) on = fold(t[k]) == (u32)(uint8_t)kOntology[k];
    onto[i] = on ? 1u : 0u;
    keys[i] = (u64)piece4_be(t, len, 0);
    vals[i] = i;
}

// head flags of the sorted active set by the whole key (a run of equal terms so far) and by the group alone
__global__ void __launch_bounds__(256) nt_round_flags_kernel(const u64* __restrict__ keys, u32 m, u32* __restrict__ flag_k,
                                                             u32* __restrict__ flag_g) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const u64 k = keys[p], q = p == 0 ? 0ull : keys[p - 1];
    flag_k[p] = (p == 0 || k != q) ? 1u : 0u;
    flag_g[p] = (p == 0 || (k >> 32) != (q >> 32)) ? 1u : 0u;
}

// ex_k / ex_g: exclusive scans of the flags: for a head that is its run's index
__global__ void __launch_bounds__(256) nt_round_heads_kernel(const u32* __restrict__ flag_k, const u32* __restrict__ flag_g,
                                                             const u32* __restrict__ ex_k, const u32* __restrict__ ex_g, u32 m,
                                                             u32* __restrict__ head_k, u32* __restrict__ head_g) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    if (flag_k[p] != 0u) head_k[ex_k[p]] = p;
    if (flag_g[p] != 0u) head_g[ex_g[p]] = p;
}

// new group = old group + offset of the run's head inside its group; a run of one term is final: rank[term] = new group
__global__ void __launch_bounds__(256) nt_round_assign_kernel(const u64* __restrict__ keys, const u32* __restrict__ vals,
                                                              const u32* __restrict__ flag_k, const u32* __restrict__ flag_g,
                                                              const u32* __restrict__ ex_k, const u32* __restrict__ ex_g,
                                                              const u32* __restrict__ head_k, const u32* __restrict__ head_g, u32 m,
                                                              u32 n_terms, u32* __restrict__ group, u32* __restrict__ keep,
                                                              u32* __restrict__ rank) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const u32 fk = flag_k[p];
    const u32 rk = ex_k[p] + fk - 1u, rg = ex_g[p] + flag_g[p] - 1u;
    const u32 ng = (u32)(keys[p] >> 32) + (head_k[rk] - head_g[rg]);
    const bool single = fk != 0u && (p + 1u == m || flag_k[p + 1u] != 0u);
    group[p] = ng;
    keep[p] = single ? 0u : 1u;
    const u32 term = vals[p];
    if (single && term < n_terms && ng < n_terms) rank[term] = ng;
}

__global__ void __launch_bounds__(256) nt_round_compact_kernel(const Text tx, const u32* __restrict__ vals, const u32* __restrict__ group,
                                                               const u32* __restrict__ keep, const u32* __restrict__ pos, u32 m,
                                                               u32 n_terms, const u32* __restrict__ term_off,
                                                               const u32* __restrict__ term_len, u64 at, u64* __restrict__ keys_out,
                                                               u32* __restrict__ vals_out) {
    const u32 p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m || keep[p] == 0u) return;
    const u32 term = vals[p], q = pos[p];
    u32 w = 0;
    if (term < n_terms) w = piece4_be(tx.p + term_off[term], term_len[term], at);
    keys_out[q] = ((u64)group[p] << 32) | (u64)w;
    vals_out[q] = term;
}

// ---- roles, ids ----------------------------------------------------------------------------------------------------------------
struct State {                 // the carve of a build's workspace: what rgcn_nt_emit reads is written by rgcn_nt_build
    SortBufs sb;
    u32 *flag, *ids, *rep, *term_of_occ;                               // 3 T: occurrences
    u32 *term_off, *term_len, *pred_kind, *onto, *rank;                // U <= 3 T: distinct terms, by provisional id
    u32 *flag_g, *ex_g, *head_k, *head_g, *group, *keep, *pos;         // rounds
    u32 *is_node, *is_rel, *is_cls, *node_id, *rel_id, *cls_id;        // by rank
    u32 *msg, *msg_pos;                                                // T: 1 for a message-passing triple, its index
    u32 *lab, *lab_pos;                                                // 2 T >= N: labelled node flags, their positions
    BuildInfo* info;
};

static State carve(Arena& ar, u64 triples) {
    State s;
    const u64 n = 3 * triples;
    s.sb = take_sort_bufs(ar, n, n);
    u32** occ[] = {&s.flag, &s.ids, &s.rep, &s.term_of_occ, &s.term_off, &s.term_len, &s.pred_kind, &s.onto, &s.rank, &s.flag_g, &s.ex_g,
                   &s.head_k, &s.head_g, &s.group, &s.keep, &s.pos, &s.is_node, &s.is_rel, &s.is_cls, &s.node_id, &s.rel_id, &s.cls_id};
    for (u32** p : occ) *p = ar.take<u32>(n);
    s.msg = ar.take<u32>(triples);
    s.msg_pos = ar.take<u32>(triples);
    s.lab = ar.take<u32>(2 * triples);
    s.lab_pos = ar.take<u32>(2 * triples);
    s.info = ar.take<BuildInfo>(1);
    return s;
}

// a lane per triple: the flags of its three terms, by rank (integer atomics: many triples share a term)
__global__ void __launch_bounds__(256) nt_roles_kernel(const u32* __restrict__ term_of_occ, const u32* __restrict__ rank,
                                                       const u32* __restrict__ pred_kind, const u32* __restrict__ onto, u32 triples,
                                                       u32 n_terms, u32* __restrict__ is_node, u32* __restrict__ is_rel,
                                                       u32* __restrict__ is_cls, u32* __restrict__ msg) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= triples) return;
    const u32 ts = term_of_occ[3 * (size_t)t], tp = term_of_occ[3 * (size_t)t + 1], to = term_of_occ[3 * (size_t)t + 2];
    u32 m = 0;
    if (ts < n_terms && tp < n_terms && to < n_terms) {
        const u32 rs = rank[ts], rp = rank[tp], ro = rank[to];
        if (rs < n_terms && rp < n_terms && ro < n_terms) {
            atomicOr(&is_node[rs], 1u);
            atomicOr(&is_node[ro], 1u);
            const u32 kind = pred_kind[tp];
            if (kind == 0u) {
                atomicOr(&is_rel[rp], 1u);
                m = 1;
            } else if (kind == kPredRdfType && onto[ts] == 0u) {
                atomicOr(&is_cls[ro], 1u);
            }
        }
    }
    msg[t] = m;
}

__global__ void __launch_bounds__(256) nt_label_flags_kernel(const u32* __restrict__ term_of_occ, const u32* __restrict__ rank,
                                                             const u32* __restrict__ pred_kind, const u32* __restrict__ onto,
                                                             const u32* __restrict__ node_id, u32 triples, u32 n_terms,
                                                             u32* __restrict__ lab) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= triples) return;
    const u32 ts = term_of_occ[3 * (size_t)t], tp = term_of_occ[3 * (size_t)t + 1];
    if (ts >= n_terms || tp >= n_terms || pred_kind[tp] != kPredRdfType || onto[ts] != 0u) return;
    const u32 rs = rank[ts];
    if (rs >= n_terms) return;
    const u32 node = node_id[rs];
    if (node < 2u * triples) atomicOr(&lab[node], 1u);
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------
struct Counts { u32 terms, nodes, rels, classes, half_edges, labelled; };

__global__ void __launch_bounds__(256) nt_edges_kernel(const State s, u32 triples, const Counts c, int64_t* __restrict__ edge_index,
                                                       int64_t* __restrict__ edge_type) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= triples || s.msg[t] == 0u) return;
    const u32 i = s.msg_pos[t];
    const u32 ts = s.term_of_occ[3 * (size_t)t], tp = s.term_of_occ[3 * (size_t)t + 1], to = s.term_of_occ[3 * (size_t)t + 2];
    if (i >= c.half_edges || ts >= c.terms || tp >= c.terms || to >= c.terms) return;
    const u32 rs = s.rank[ts], rp = s.rank[tp], ro = s.rank[to];
    if (rs >= c.terms || rp >= c.terms || ro >= c.terms) return;
    const int64_t a = s.node_id[rs], b = s.node_id[ro], r = s.rel_id[rp];
    const size_t e = 2 * (size_t)c.half_edges, at = 2 * (size_t)i;
    edge_index[at] = a;
    edge_index[at + 1] = b;
    edge_index[e + at] = b;
    edge_index[e + at + 1] = a;
    edge_type[at] = 2 * r;
    edge_type[at + 1] = 2 * r + 1;
}

struct Tables { u32 *node_off, *node_len, *rel_off, *rel_len, *cls_off, *cls_len; };

__global__ void __launch_bounds__(256) nt_tables_kernel(const State s, const Counts c, const Tables tb) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.terms) return;
    const u32 r = s.rank[i];
    if (r >= c.terms) return;
    const u32 off = s.term_off[i], len = s.term_len[i];
    if (s.is_node[r] != 0u && s.node_id[r] < c.nodes) {
        tb.node_off[s.node_id[r]] = off;
        tb.node_len[s.node_id[r]] = len;
    }
    if (s.is_rel[r] != 0u && s.rel_id[r] < c.rels) {
        tb.rel_off[s.rel_id[r]] = off;
        tb.rel_len[s.rel_id[r]] = len;
    }
    if (s.is_cls[r] != 0u && s.cls_id[r] < c.classes) {
        tb.cls_off[s.cls_id[r]] = off;
        tb.cls_len[s.cls_id[r]] = len;
    }
}

__global__ void __launch_bounds__(256) nt_labelled_kernel(const State s, const Counts c, int64_t* __restrict__ labelled_idx) {
    const u32 n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= c.nodes || s.lab[n] == 0u) return;
    const u32 j = s.lab_pos[n];
    if (j < c.labelled) labelled_idx[j] = (int64_t)n;
}

__global__ void __launch_bounds__(256) nt_labels_kernel(const State s, u32 triples, const Counts c, int64_t* __restrict__ labels) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= triples) return;
    const u32 ts = s.term_of_occ[3 * (size_t)t], tp = s.term_of_occ[3 * (size_t)t + 1], to = s.term_of_occ[3 * (size_t)t + 2];
    if (ts >= c.terms || tp >= c.terms || to >= c.terms || s.pred_kind[tp] != kPredRdfType || s.onto[ts] != 0u) return;
    const u32 rs = s.rank[ts], ro = s.rank[to];
    if (rs >= c.terms || ro >= c.terms) return;
    const u32 node = s.node_id[rs], cls = s.cls_id[ro];
    if (node >= c.nodes || cls >= c.classes) return;
    const u32 j = s.lab_pos[node];
    if (j < c.labelled) atomicOr((u64*)&labels[(size_t)j * c.classes + cls], 1ull);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
constexpr int64_t kMaxBytes = 0xFFFF0000ll;
constexpr int64_t kMaxTriples = (int64_t)(kMaxKeys / 3);

static u32 byte_blocks(int64_t num_bytes) { return (u32)((num_bytes + kByteBlock - 1) / kByteBlock); }
static int vec_ok(const void* p) { return ((uintptr_t)p & 15u) == 0 ? 1 : 0; }

struct TokState {
    u32 *block_cnt, *nl_pos, *tok, *keep, *pos, *sums;
    TokInfo* info;
};

static TokState carve_tok(Arena& ar, int64_t num_bytes, int64_t num_lines) {
    TokState s;
    const u64 nb = byte_blocks(num_bytes), nl = (u64)num_lines;
    s.block_cnt = ar.take<u32>(nb + 1);
    s.nl_pos = ar.take<u32>(nl + 1);
    s.tok = ar.take<u32>(4 * nl);
    s.keep = ar.take<u32>(nl + 1);
    s.pos = ar.take<u32>(nl + 1);
    s.sums = ar.take<u32>((size_t)scan_blocks((u32)(nb > nl ? nb : nl)) + 2);
    s.info = ar.take<TokInfo>(1);
    return s;
}

static hipError_t reset_tok_info(TokInfo* info, hipStream_t s) {
    hipError_t e = hipMemsetAsync(info, 0, sizeof(TokInfo), s);
    if (e == hipSuccess) e = hipMemsetAsync(&info->nul_pos, 0xFF, sizeof(u32), s);
    if (e == hipSuccess) e = hipMemsetAsync(&info->bad_line, 0xFF, 2 * sizeof(u32), s);      // bad_line, nul_line
    return e;
}

}  // namespace rgcn_nt

using namespace rgcn_nt;

extern "C" size_t rgcn_nt_lines_workspace_bytes(int64_t num_bytes) {
    if (num_bytes < 0 || num_bytes > kMaxBytes) return 0;
    Arena ar(nullptr);
    ar.take<TokInfo>(1);
    return ar.bytes();
}

extern "C" int rgcn_nt_lines(const uint8_t* text, int64_t num_bytes, void* workspace, size_t workspace_bytes, int64_t* num_lines,
                             void* stream) {
    if (!num_lines || (num_bytes > 0 && !text)) return RGCN_ERR_NULL;
    if (num_bytes < 0) return RGCN_ERR_ARG;
    if (num_bytes > kMaxBytes) return RGCN_ERR_PLAN;
    Arena ar(workspace);
    TokInfo* info = ar.take<TokInfo>(1);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    *num_lines = 0;
    if (num_bytes == 0) return RGCN_OK;
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = reset_tok_info(info, s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(nt_count_kernel, dim3(byte_blocks(num_bytes)), dim3(256), 0, s, text, (u64)num_bytes, vec_ok(text), (u32*)nullptr,
                       info);
    TokInfo h;
    st = read_back(info, &h, s);
    if (st != 0) return st;
    *num_lines = (int64_t)h.newlines + (h.last_is_nl ? 0 : 1);
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_nt_tokenize_workspace_bytes(int64_t num_bytes, int64_t num_lines) {
    if (num_bytes < 0 || num_bytes > kMaxBytes || num_lines < 0 || num_lines > num_bytes) return 0;
    Arena ar(nullptr);
    carve_tok(ar, num_bytes, num_lines);
    return ar.bytes();
}

extern "C" int rgcn_nt_tokenize(const uint8_t* text, int64_t num_bytes, int64_t num_lines, uint32_t* occ_off, uint32_t* occ_len,
                                void* workspace, size_t workspace_bytes, int64_t* info_out, void* stream) {
    if (!info_out || (num_bytes > 0 && !text) || (num_lines > 0 && (!occ_off || !occ_len))) return RGCN_ERR_NULL;
    if (num_bytes < 0 || num_lines < 0 || num_lines > num_bytes) return RGCN_ERR_ARG;
    if (num_bytes > kMaxBytes) return RGCN_ERR_PLAN;
    Arena ar(workspace);
    TokState ts = carve_tok(ar, num_bytes, num_lines);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    info_out[0] = info_out[1] = info_out[2] = info_out[3] = 0;
    if (num_lines == 0) return num_bytes == 0 ? RGCN_OK : RGCN_ERR_ARG;
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = reset_tok_info(ts.info, s);
    if (e != hipSuccess) return (int)e;
    const u32 nb = byte_blocks(num_bytes), nl = (u32)num_lines;
    const int vec = vec_ok(text);
    hipLaunchKernelGGL(nt_count_kernel, dim3(nb), dim3(256), 0, s, text, (u64)num_bytes, vec, ts.block_cnt, ts.info);
    exclusive_scan(ts.block_cnt, ts.block_cnt, nb, ts.sums, s);
    hipLaunchKernelGGL(nt_newlines_kernel, dim3(nb), dim3(256), 0, s, text, (u64)num_bytes, vec, ts.block_cnt, ts.nl_pos, nl);
    hipLaunchKernelGGL(nt_tokenize_kernel, dim3((nl + 3) / 4), dim3(256), 0, s, text, (u64)num_bytes, ts.nl_pos, nl, ts.tok, ts.keep,
                       ts.info);
    exclusive_scan(ts.keep, ts.pos, nl, ts.sums, s);
    hipLaunchKernelGGL(nt_store_kernel, dim3(1), dim3(1), 0, s, ts.sums + scan_blocks(nl), &ts.info->triples);
    hipLaunchKernelGGL(nt_compact_kernel, dim3(grid_for(nl)), dim3(256), 0, s, ts.tok, ts.keep, ts.pos, nl, occ_off, occ_len);
    TokInfo h;
    st = read_back(ts.info, &h, s);
    if (st != 0) return st;
    if ((int64_t)h.newlines + (h.last_is_nl ? 0 : 1) != num_lines) return RGCN_ERR_ARG;      // not this text's line count
    info_out[0] = h.triples;
    info_out[1] = h.bad_line == kNone ? 0 : (int64_t)h.bad_line;
    info_out[2] = h.nul_line == kNone ? 0 : (int64_t)h.nul_line;
    info_out[3] = h.max_len;
    if (info_out[1] != 0 || info_out[2] != 0) return RGCN_ERR_GRAPH;
    return (int)hipGetLastError();
}

extern "C" size_t rgcn_nt_workspace_bytes(int64_t num_triples) {
    if (num_triples < 0 || num_triples > kMaxTriples) return 0;
    Arena ar(nullptr);
    carve(ar, (u64)num_triples);
    return ar.bytes();
}

extern "C" int rgcn_nt_build(const uint8_t* text, int64_t num_bytes, const uint32_t* occ_off, const uint32_t* occ_len,
                             int64_t num_triples, int64_t max_term_len, int hash_bits, int64_t seed, void* workspace,
                             size_t workspace_bytes, int64_t* counts, void* stream) {
    if (!counts || (num_bytes > 0 && !text) || (num_triples > 0 && (!occ_off || !occ_len))) return RGCN_ERR_NULL;
    if (num_bytes < 0 || num_triples < 0 || max_term_len < 0 || seed < 0 || hash_bits < 1 || hash_bits > 64) return RGCN_ERR_ARG;
    if (num_bytes > kMaxBytes || num_triples > kMaxTriples) return RGCN_ERR_PLAN;
    Arena ar(workspace);
    const State w = carve(ar, (u64)num_triples);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    for (int i = 0; i < 8; ++i) counts[i] = 0;
    if (num_triples == 0) return RGCN_OK;
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    const Text tx = {text, (u64)num_bytes};
    const u32 triples = (u32)num_triples, n_occ = 3u * triples;
    hipError_t e = hipMemsetAsync(w.info, 0, sizeof(BuildInfo), s);
    if (e != hipSuccess) return (int)e;

    // distinct terms: hash, sort, run ids, verification
    const u64 mask = hash_bits == 64 ? ~0ull : ((1ull << hash_bits) - 1ull);
    const u32 group_grid = grid_for((u64)n_occ * kGroup);
    hipLaunchKernelGGL(nt_hash_kernel, dim3(group_grid), dim3(256), 0, s, tx, occ_off, occ_len, n_occ, mix((u64)seed + kGolden), mask,
                       w.sb.k[0], w.sb.v[0], &w.info->status);
    const int cur = radix_sort_pairs(w.sb, n_occ, hash_bits, s);
    run_ids(w.sb.k[cur], n_occ, 0, w.flag, w.ids, w.sb.sums, s);
    hipLaunchKernelGGL(nt_store_kernel, dim3(1), dim3(1), 0, s, w.sb.sums + scan_blocks(n_occ), &w.info->distinct);
    hipLaunchKernelGGL(nt_rep_kernel, dim3(grid_for(n_occ)), dim3(256), 0, s, w.sb.v[cur], w.flag, w.ids, n_occ, w.rep);
    hipLaunchKernelGGL(nt_verify_kernel, dim3(group_grid), dim3(256), 0, s, tx, occ_off, occ_len, w.sb.v[cur], w.ids, w.rep, n_occ,
                       w.term_of_occ, &w.info->status);
    BuildInfo h;
    st = read_back(w.info, &h, s);
    if (st != 0) return st;
    counts[0] = h.distinct;
    counts[6] = h.status;
    if (h.status & kStatusBadOcc) return RGCN_ERR_GRAPH;
    if (h.status & kStatusCollision) return RGCN_ERR_COLLISION;
    const u32 n_terms = h.distinct;
    if (n_terms == 0 || n_terms > n_occ) return RGCN_ERR_GRAPH;

    // bytewise ranks by refinement rounds
    SortBufs sb = w.sb;
    hipLaunchKernelGGL(nt_terms_kernel, dim3(grid_for(n_terms)), dim3(256), 0, s, tx, occ_off, occ_len, w.rep, n_terms, n_occ, w.term_off,
                       w.term_len, w.pred_kind, w.onto, sb.k[0], sb.v[0]);
    e = hipMemsetAsync(w.rank, 0xFF, (size_t)n_terms * sizeof(u32), s);
    if (e != hipSuccess) return (int)e;
    const int sort_bits = 32 + bits_for((u64)n_terms - 1);
    const int64_t max_rounds = max_term_len / 4 + 2;
    u32 m = n_terms;
    int64_t round = 0;
    for (; m > 0 && round < max_rounds; ++round) {
        const int c = radix_sort_pairs(sb, m, sort_bits, s);
        const dim3 grid(grid_for(m)), block(256);
        hipLaunchKernelGGL(nt_round_flags_kernel, grid, block, 0, s, sb.k[c], m, w.flag, w.flag_g);
        exclusive_scan(w.flag, w.ids, m, sb.sums, s);
        exclusive_scan(w.flag_g, w.ex_g, m, sb.sums, s);
        hipLaunchKernelGGL(nt_round_heads_kernel, grid, block, 0, s, w.flag, w.flag_g, w.ids, w.ex_g, m, w.head_k, w.head_g);
        hipLaunchKernelGGL(nt_round_assign_kernel, grid, block, 0, s, sb.k[c], sb.v[c], w.flag, w.flag_g, w.ids, w.ex_g, w.head_k, w.head_g,
                           m, n_terms, w.group, w.keep, w.rank);
        exclusive_scan(w.keep, w.pos, m, sb.sums, s);
        hipLaunchKernelGGL(nt_round_compact_kernel, grid, block, 0, s, tx, sb.v[c], w.group, w.keep, w.pos, m, n_terms, w.term_off,
                           w.term_len, (u64)(4 * (round + 1)), sb.k[c ^ 1], sb.v[c ^ 1]);
        u32 left = 0;
        st = read_back(sb.sums + scan_blocks(m), &left, s);
        if (st != 0) return st;
        if (left > m) return RGCN_ERR_GRAPH;
        sb = from_pair(sb, c ^ 1);
        m = left;
    }
    counts[7] = round;
    if (m != 0) return RGCN_ERR_GRAPH;          // max_term_len is not this text's: terms still tie after their last byte

    // roles -> ids in rank order; message-passing triples; labelled nodes
    e = hipMemsetAsync(w.is_node, 0, (size_t)n_terms * sizeof(u32), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.is_rel, 0, (size_t)n_terms * sizeof(u32), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.is_cls, 0, (size_t)n_terms * sizeof(u32), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.lab, 0, 2 * (size_t)triples * sizeof(u32), s);
    if (e != hipSuccess) return (int)e;
    const dim3 tgrid(grid_for(triples)), block(256);
    hipLaunchKernelGGL(nt_roles_kernel, tgrid, block, 0, s, w.term_of_occ, w.rank, w.pred_kind, w.onto, triples, n_terms, w.is_node,
                       w.is_rel, w.is_cls, w.msg);
    const u32* const flags[4] = {w.is_node, w.is_rel, w.is_cls, w.msg};
    u32* const ids[4] = {w.node_id, w.rel_id, w.cls_id, w.msg_pos};
    u32* const totals[4] = {&w.info->nodes, &w.info->relations, &w.info->classes, &w.info->half_edges};
    for (int i = 0; i < 4; ++i) {
        const u32 n = i == 3 ? triples : n_terms;
        exclusive_scan(flags[i], ids[i], n, w.sb.sums, s);
        hipLaunchKernelGGL(nt_store_kernel, dim3(1), dim3(1), 0, s, w.sb.sums + scan_blocks(n), totals[i]);
    }
    hipLaunchKernelGGL(nt_label_flags_kernel, tgrid, block, 0, s, w.term_of_occ, w.rank, w.pred_kind, w.onto, w.node_id, triples, n_terms,
                       w.lab);
    exclusive_scan(w.lab, w.lab_pos, 2 * triples, w.sb.sums, s);
    hipLaunchKernelGGL(nt_store_kernel, dim3(1), dim3(1), 0, s, w.sb.sums + scan_blocks(2 * triples), &w.info->labelled);
    st = read_back(w.info, &h, s);
    if (st != 0) return st;
    counts[1] = h.nodes;
    counts[2] = h.relations;
    counts[3] = h.classes;
    counts[4] = 2 * (int64_t)h.half_edges;
    counts[5] = h.labelled;
    return (int)hipGetLastError();
}

extern "C" int rgcn_nt_emit(int64_t num_triples, const int64_t* counts, int64_t* edge_index, int64_t* edge_type, int64_t* labelled_idx,
                            int64_t* labels, uint32_t* node_off, uint32_t* node_len, uint32_t* rel_off, uint32_t* rel_len,
                            uint32_t* cls_off, uint32_t* cls_len, void* workspace, size_t workspace_bytes, void* stream) {
    if (!counts) return RGCN_ERR_NULL;
    if (num_triples < 0) return RGCN_ERR_ARG;
    if (num_triples > kMaxTriples) return RGCN_ERR_PLAN;
    const int64_t terms = counts[0], nodes = counts[1], rels = counts[2], classes = counts[3], edges = counts[4], labelled = counts[5];
    if (terms < 0 || terms > 3 * num_triples || nodes < 0 || nodes > terms || nodes > 2 * num_triples || rels < 0 || rels > terms ||
        classes < 0 || classes > terms || edges < 0 || (edges & 1) || edges > 2 * num_triples || labelled < 0 || labelled > nodes)
        return RGCN_ERR_ARG;
    if ((edges > 0 && (!edge_index || !edge_type)) || (labelled > 0 && (!labelled_idx || (classes > 0 && !labels))) ||
        (nodes > 0 && (!node_off || !node_len)) || (rels > 0 && (!rel_off || !rel_len)) || (classes > 0 && (!cls_off || !cls_len)))
        return RGCN_ERR_NULL;
    Arena ar(workspace);
    const State w = carve(ar, (u64)num_triples);
    if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
    if (!workspace) return RGCN_ERR_NULL;
    if (num_triples == 0 || terms == 0) return RGCN_OK;
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    const u32 triples = (u32)num_triples;
    const Counts c = {(u32)terms, (u32)nodes, (u32)rels, (u32)classes, (u32)(edges / 2), (u32)labelled};
    const dim3 tgrid(grid_for(triples)), block(256);
    if (edges > 0) hipLaunchKernelGGL(nt_edges_kernel, tgrid, block, 0, s, w, triples, c, edge_index, edge_type);
    const Tables tb = {node_off, node_len, rel_off, rel_len, cls_off, cls_len};
    hipLaunchKernelGGL(nt_tables_kernel, dim3(grid_for(c.terms)), block, 0, s, w, c, tb);
    if (labelled > 0) {
        hipLaunchKernelGGL(nt_labelled_kernel, dim3(grid_for(c.nodes)), block, 0, s, w, c, labelled_idx);
        if (classes > 0) {
            hipError_t e = hipMemsetAsync(labels, 0, (size_t)labelled * (size_t)classes * sizeof(int64_t), s);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL(nt_labels_kernel, tgrid, block, 0, s, w, triples, c, labels);
        }
    }
    return (int)hipGetLastError();
}

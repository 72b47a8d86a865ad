// rgcn_summary.hip -- graph summaries built ON THE DEVICE behind the C ABI (include/rgcn_mi355x.h: rgcn_summary_round,
// rgcn_summary_quotient): k-bisimulation partition refinement of the nodes and the quotient graph of a partition, on the
// same strided int64 COO the layer and the plan builder take.  gfx950 only.  DESIGN.md section 13 has the semantics.
//
// One refinement round  b -> b'  (b'[i] == b'[j]  iff  b[i] == b[j] and S(i) == S(j), S the SET of (direction, type, block of
// the neighbour) over the edges of the node):
//   keys      one 64-bit key per edge (two for in_out): (owner, [dir,] type, b[neighbour]), fields bits_for() wide
//   sort      route 1: one stable sort over the bits used; route 2 (the fields pass 64 bits): sort by (dir, type, block),
//             replace that element by its rank among the distinct elements (32 bits), then sort stably by owner
//   sig       every DISTINCT key adds two fmix64 words of its element into the 128-bit signature of its owner: lanes of a
//             wave holding one owner are summed with shuffles, the first lane of the run issues the two 64-bit atomic adds
//             (integer sums: exact, order-free); the node's own block is folded in last
//   renumber  sort (sig_lo, node), then stably (sig_hi, node); runs of equal 128 bits are blocks, the first node of a run is
//             its smallest; a scan over the nodes of the first-member flags numbers the blocks by smallest member
//   B         read back through a host pointer: the one copy and the one synchronisation of a round
//
// All byte / integer work, bound by HBM traffic like the plan builder; nothing here touches MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/rgcn_mi355x.h"
#include "rgcn_sort_scan.h"

namespace rgcn_summary {

using namespace rgcn_sort_scan;

constexpr u32 kErrType = 1u, kErrNode = 2u, kErrBlock = 4u;
constexpr u32 kNoOwner = 0xFFFFFFFFu;      // owner of the lanes past the last key (node ids stay below 2^31)

struct Results {        // device-resident scalars of one call: what the host reads back in one copy
    u32 error;          // kErr* bits
    u32 count;          // blocks of the new partition / distinct triples of the quotient
};

__host__ __device__ inline u64 fmix64(u64 x) {      // MurmurHash3's 64-bit finaliser: a bijection of the 64-bit words
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}
constexpr u64 kSeedA = 0x9E3779B97F4A7C15ull, kSeedB = 0xD1B54A32D192ED03ull;
__host__ __device__ inline u64 elem_word_a(u64 e) { return fmix64(e + kSeedA); }
__host__ __device__ inline u64 elem_word_b(u64 e) { return fmix64(fmix64(e ^ kSeedB) + kSeedA); }
// The words of a node's OWN block come from seeds of their own.  With the elements' words a node of block x whose one element is
// the integer y and a node of block y whose one element is x -- two nodes that point at each other's block -- had one signature:
// word(y) ^ word(x) and word(y) + word(x) do not tell which of the two is the block.
constexpr u64 kSeedOwnA = 0xA0761D6478BD642Full, kSeedOwnB = 0xE7037ED1A0B428DBull;
__host__ __device__ inline u64 own_word_a(u64 b) { return fmix64(b + kSeedOwnA); }
__host__ __device__ inline u64 own_word_b(u64 b) { return fmix64(fmix64(b ^ kSeedOwnB) + kSeedOwnA); }

// ------------------------------------------------------------------------------------------------
// keys of a refinement round
// ------------------------------------------------------------------------------------------------
struct RoundKeys {
    int block_bits, type_bits, dir_bits, node_bits;
    __host__ __device__ int elem_bits() const { return block_bits + type_bits + dir_bits; }
    __host__ __device__ int total() const { return elem_bits() + node_bits; }
    __host__ __device__ u64 elem(u32 dir, u32 type, u32 blk) const { return ((((u64)dir << type_bits) | type) << block_bits) | blk; }
};

// Key i of an edge list of `num_edges` edges: out / in give one key per edge, in_out two (2e: the edge seen from its source,
// dir 0; 2e + 1: from its target, dir 1).  Route 1 writes (owner << elem_bits | element); route 2 writes the element as the key
// and the owner as the value.  An id out of range sets its error bit and the key of node 0 / type 0 / block 0: everything the
// later kernels index with a key field stays inside its array whatever the input holds.
__global__ void round_keys_kernel(const int64_t* __restrict__ src, int64_t src_stride, const int64_t* __restrict__ dst,
                                  int64_t dst_stride, const int64_t* __restrict__ typ, int64_t typ_stride,
                                  const int32_t* __restrict__ block, u64 num_keys, int direction, u32 n_nodes, u32 num_rel,
                                  u32 num_blocks, RoundKeys kl, int two_sorts, u64* __restrict__ keys, u32* __restrict__ vals,
                                  Results* __restrict__ res) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_keys) return;
    const u64 e = direction == 2 ? i >> 1 : i;
    const u32 dir = direction == 2 ? (u32)(i & 1u) : 0u;
    const bool from_source = direction == 0 || (direction == 2 && dir == 0u);
    const int64_t sv = src[e * src_stride], dv = dst[e * dst_stride], t = typ[e * typ_stride];
    u32 err = 0, owner = 0, type = 0, blk = 0;
    if (t < 0 || t >= (int64_t)num_rel) err |= kErrType;
    if (sv < 0 || sv >= (int64_t)n_nodes || dv < 0 || dv >= (int64_t)n_nodes) err |= kErrNode;
    if (!err) {
        const int32_t b = block[from_source ? dv : sv];
        if (b < 0 || (u32)b >= num_blocks) {
            err |= kErrBlock;
        } else {
            owner = (u32)(from_source ? sv : dv);
            type = (u32)t;
            blk = (u32)b;
        }
    }
    if (err) atomicOr(&res->error, err);
    const u64 el = err ? 0ull : kl.elem(dir, type, blk);
    if (two_sorts) {
        keys[i] = el;
        vals[i] = owner;
    } else {
        keys[i] = ((u64)owner << kl.elem_bits()) | el;
        vals[i] = 0u;
    }
}

// route 2, between its sorts: (rank of the element among the distinct elements << 32 | owner), rank = run id of the first sort.
// The owner sits in the LOW bits, the ones radix_sort_pairs sorts: the second sort runs over the owner's bits alone and, being
// stable, keeps the ranks of one owner in order.
__global__ void rank_keys_kernel(const u32* __restrict__ owner, const u32* __restrict__ rank, u32 n, u64* __restrict__ keys,
                                 u32* __restrict__ vals) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = ((u64)rank[i] << 32) | owner[i];
    vals[i] = 0u;
}

// ------------------------------------------------------------------------------------------------
// signatures
// ------------------------------------------------------------------------------------------------
// keys sorted by (owner, element).  Route 1 (elem_bits > 0): owner = key >> elem_bits, element = the bits below; route 2
// (elem_bits == 0): owner = low word, element = high word.  A key equal to the one before it is a
// duplicate edge and adds nothing.  The lanes of a wave that hold one owner are contiguous: a segmented suffix sum over them
// (five shuffle steps per word) leaves the run's total in its first lane, which alone adds it to sig[owner] -- one pair of
// atomics per (wave, owner) run, 1 / 64 of a hub's edges.  A run cut by a wave boundary adds its parts separately; the sums are
// integers, so neither the cut nor the order of arrival changes them.
__global__ void signature_kernel(const u64* __restrict__ keys, u32 n, int elem_bits, u64* __restrict__ sig_lo,
                                 u64* __restrict__ sig_hi) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;      // (the grid covers n rounded up to whole waves: no early return)
    const int lane = threadIdx.x & 63;
    const bool valid = i < n;
    const u64 k = valid ? keys[i] : 0ull;
    const bool distinct = valid && (i == 0 || keys[i - 1] != k);
    const u32 owner = !valid ? kNoOwner : (elem_bits ? (u32)(k >> elem_bits) : (u32)k);
    const u64 el = elem_bits ? k & ((1ull << elem_bits) - 1ull) : k >> 32;
    u64 a = distinct ? elem_word_a(el) : 0ull;
    u64 b = distinct ? elem_word_b(el) : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 ta = __shfl_down(a, d), tb = __shfl_down(b, d);
        const u32 to = __shfl_down(owner, d);
        if (lane + d < 64 && to == owner) {      // lane + d continues this lane's run, and so does every lane between them
            a += ta;
            b += tb;
        }
    }
    const u32 before = __shfl_up(owner, 1);
    const bool first = valid && (lane == 0 || before != owner);
    if (first && (a | b) != 0ull) {
        atomicAdd((unsigned long long*)&sig_lo[owner], (unsigned long long)a);
        atomicAdd((unsigned long long*)&sig_hi[owner], (unsigned long long)b);
    }
}

// the node's own block joins its signature; (sig_lo, node) is the first renumbering sort's input
__global__ void fold_kernel(u64* __restrict__ sig_lo, u64* __restrict__ sig_hi, const int32_t* __restrict__ block, u32 n_nodes,
                            u64* __restrict__ keys, u32* __restrict__ vals) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const u64 own = (u64)(u32)block[i];
    const u64 lo = fmix64(sig_lo[i] ^ own_word_a(own)), hi = fmix64(sig_hi[i] + own_word_b(own));
    sig_lo[i] = lo;
    sig_hi[i] = hi;
    keys[i] = lo;
    vals[i] = i;
}

// ------------------------------------------------------------------------------------------------
// renumbering
// ------------------------------------------------------------------------------------------------
__global__ void gather_words_kernel(const u64* __restrict__ words, const u32* __restrict__ node, u32 n, u64* __restrict__ keys) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = words[node[i]];
}

// nodes sorted by (sig_hi, sig_lo, node): flag the first node of every run of equal 128 bits
__global__ void block_heads_kernel(const u64* __restrict__ hi_sorted, const u64* __restrict__ sig_lo, const u32* __restrict__ node,
                                   u32 n, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = (i == 0 || hi_sorted[i] != hi_sorted[i - 1] || sig_lo[node[i]] != sig_lo[node[i - 1]]) ? 1u : 0u;
}

// ex = exclusive scan of flag.  The head of run r = ex[i] is the run's smallest node: remember it, and mark it among the nodes
__global__ void block_first_kernel(const u32* __restrict__ flag, const u32* __restrict__ ex, const u32* __restrict__ node, u32 n,
                                   u32* __restrict__ run_first, u32* __restrict__ is_first) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    run_first[ex[i]] = node[i];
    is_first[node[i]] = 1u;
}

// cid = exclusive scan over the NODES of is_first: at a first member, the blocks whose smallest member is smaller -- its id
__global__ void block_ids_kernel(const u32* __restrict__ flag, const u32* __restrict__ ex, const u32* __restrict__ node, u32 n,
                                 const u32* __restrict__ run_first, const u32* __restrict__ cid, int32_t* __restrict__ block_out,
                                 const u32* __restrict__ total, Results* __restrict__ res) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) res->count = *total;
    if (i >= n) return;
    block_out[node[i]] = (int32_t)cid[run_first[ex[i] + flag[i] - 1u]];
}

// ------------------------------------------------------------------------------------------------
// quotient graph
// ------------------------------------------------------------------------------------------------
struct QuotKeys {
    int block_bits, type_bits;
    __host__ __device__ int total() const { return 2 * block_bits + type_bits; }
};

// route 1: key = (type, b[dst], b[src]); route 2: key = b[src] and the value carries the edge, whose (type, b[dst]) the second
// sort gathers.  Errors as in round_keys_kernel.
__global__ void quot_keys_kernel(const int64_t* __restrict__ src, int64_t src_stride, const int64_t* __restrict__ dst,
                                 int64_t dst_stride, const int64_t* __restrict__ typ, int64_t typ_stride,
                                 const int32_t* __restrict__ block, u64 num_edges, u32 n_nodes, u32 num_rel, u32 num_blocks,
                                 QuotKeys kl, int two_sorts, u64* __restrict__ keys, u32* __restrict__ vals,
                                 Results* __restrict__ res) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= num_edges) return;
    const int64_t sv = src[e * src_stride], dv = dst[e * dst_stride], t = typ[e * typ_stride];
    u32 err = 0, bs = 0, bd = 0;
    if (t < 0 || t >= (int64_t)num_rel) err |= kErrType;
    if (sv < 0 || sv >= (int64_t)n_nodes || dv < 0 || dv >= (int64_t)n_nodes) err |= kErrNode;
    if (!err) {
        const int32_t b0 = block[sv], b1 = block[dv];
        if (b0 < 0 || (u32)b0 >= num_blocks || b1 < 0 || (u32)b1 >= num_blocks) err |= kErrBlock;
        else { bs = (u32)b0; bd = (u32)b1; }
    }
    if (err) atomicOr(&res->error, err);
    const u64 td = err ? 0ull : (((u64)t << kl.block_bits) | bd);
    keys[e] = two_sorts ? (u64)bs : ((td << kl.block_bits) | bs);
    vals[e] = (u32)e;
}

// route 2, between its sorts: the edges are sorted by b[src]; key = (type, b[dst]) of the edge, b[src] moves to the side array
__global__ void quot_second_keys_kernel(const u64* __restrict__ bsrc_sorted, const u32* __restrict__ edge, u32 n,
                                        const int64_t* __restrict__ dst, int64_t dst_stride, const int64_t* __restrict__ typ,
                                        int64_t typ_stride, const int32_t* __restrict__ block, u32 n_nodes, u32 num_rel,
                                        u32 num_blocks, QuotKeys kl, u64* __restrict__ keys, u32* __restrict__ vals,
                                        u32* __restrict__ bsrc_of_edge) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 e = edge[i];
    const int64_t dv = dst[(u64)e * dst_stride], t = typ[(u64)e * typ_stride];
    u64 td = 0;
    if (t >= 0 && t < (int64_t)num_rel && dv >= 0 && dv < (int64_t)n_nodes) {      // (else: the error bit is set already)
        const int32_t b1 = block[dv];
        if (b1 >= 0 && (u32)b1 < num_blocks) td = ((u64)t << kl.block_bits) | (u32)b1;
    }
    keys[i] = td;
    vals[i] = e;
    bsrc_of_edge[e] = (u32)bsrc_sorted[i];
}

__global__ void quot_heads_kernel(const u64* __restrict__ keys, const u32* __restrict__ edge, const u32* __restrict__ bsrc_of_edge,
                                  u32 n, u32* __restrict__ flag) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool head = i == 0 || keys[i] != keys[i - 1];
    if (!head && bsrc_of_edge != nullptr) head = bsrc_of_edge[edge[i]] != bsrc_of_edge[edge[i - 1]];
    flag[i] = head ? 1u : 0u;
}

// the head of run u = ex[i] writes the run's triple and where it starts
__global__ void quot_emit_kernel(const u64* __restrict__ keys, const u32* __restrict__ edge, const u32* __restrict__ bsrc_of_edge,
                                 const u32* __restrict__ flag, const u32* __restrict__ ex, u32 n, QuotKeys kl,
                                 int64_t* __restrict__ src_out, int64_t* __restrict__ dst_out, int64_t* __restrict__ type_out,
                                 u32* __restrict__ start) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const u32 u = ex[i];
    const u64 k = keys[i], bmask = (1ull << kl.block_bits) - 1ull;
    u64 td, bs;
    if (bsrc_of_edge != nullptr) {
        td = k;
        bs = bsrc_of_edge[edge[i]];
    } else {
        td = k >> kl.block_bits;
        bs = k & bmask;
    }
    src_out[u] = (int64_t)bs;
    dst_out[u] = (int64_t)(td & bmask);
    type_out[u] = (int64_t)(td >> kl.block_bits);
    start[u] = i;
}

__global__ void quot_mult_kernel(const u32* __restrict__ start, u32 n_runs, u32 n, int64_t* __restrict__ mult_out) {
    const u32 u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n_runs) mult_out[u] = (int64_t)((u + 1u < n_runs ? start[u + 1] : n) - start[u]);
}

__global__ void publish_count_kernel(const u32* __restrict__ total, Results* __restrict__ res) { res->count = *total; }

// ------------------------------------------------------------------------------------------------
// workspace
// ------------------------------------------------------------------------------------------------
struct Workspace {
    SortBufs sb;         // kmax keys (edges; both directions of every edge for in_out) or n_nodes signatures, whichever is more
    u32* scan_a;         // kmax + 1
    u32* scan_b;         // kmax + 1
    u32* scan_c;         // kmax + 1
    u64* sig_lo;         // n_nodes
    u64* sig_hi;         // n_nodes
    u32* node_a;         // n_nodes + 1
    u32* node_b;         // n_nodes + 1
    Results* res;
    size_t bytes;
};

static Workspace carve(void* base, u64 num_keys, u64 n_nodes) {
    Workspace w;
    Arena ar(base);
    const u64 kmax = num_keys > n_nodes ? num_keys : n_nodes;
    w.res = ar.take<Results>(1);
    w.sb = take_sort_bufs(ar, kmax, kmax + 1);
    w.scan_a = ar.take<u32>(kmax + 1);
    w.scan_b = ar.take<u32>(kmax + 1);
    w.scan_c = ar.take<u32>(kmax + 1);
    w.sig_lo = ar.take<u64>(n_nodes);
    w.sig_hi = ar.take<u64>(n_nodes);
    w.node_a = ar.take<u32>(n_nodes + 1);
    w.node_b = ar.take<u32>(n_nodes + 1);
    w.bytes = ar.bytes();
    return w;
}

constexpr int32_t kMaxRelations = 65536;

static int check_graph(const rgcn_graph_t* g) {
    if (g == nullptr) return RGCN_ERR_NULL;
    if (g->num_edges < 0 || g->num_nodes <= 0 || g->num_relations <= 0 || g->num_relations > kMaxRelations) return RGCN_ERR_PLAN;
    if (g->num_edges > 0 && (!g->src || !g->dst || !g->type)) return RGCN_ERR_NULL;
    return RGCN_OK;
}

}  // namespace rgcn_summary

using namespace rgcn_summary;

static u64 round_keys(int64_t num_edges, int direction) { return (u64)num_edges * (direction == 2 ? 2u : 1u); }

extern "C" size_t rgcn_summary_workspace_bytes(int64_t num_edges, int32_t num_nodes, int direction) {
    if (num_edges < 0 || num_nodes <= 0 || direction < 0 || direction > 2) return 0;
    if ((u64)num_edges > kMaxKeys || round_keys(num_edges, direction) > kMaxKeys) return 0;
    return carve(nullptr, round_keys(num_edges, direction), (u64)num_nodes).bytes;
}

extern "C" int rgcn_summary_round(const rgcn_graph_t* g, int direction, const int32_t* block_in, int32_t num_blocks_in, int route,
                                  int32_t* block_out, void* workspace, size_t workspace_bytes, int32_t* num_blocks_out,
                                  void* stream) {
    int st = check_graph(g);
    if (st != RGCN_OK) return st;
    if (!block_in || !block_out || !workspace || !num_blocks_out) return RGCN_ERR_NULL;
    if (direction < 0 || direction > 2 || num_blocks_in < 1 || route < 0 || route > 2) return RGCN_ERR_PLAN;
    if ((u64)g->num_edges > kMaxKeys || round_keys(g->num_edges, direction) > kMaxKeys) return RGCN_ERR_PLAN;
    RoundKeys kl;
    kl.block_bits = bits_for((u64)num_blocks_in - 1);
    kl.type_bits = bits_for((u64)g->num_relations - 1);
    kl.dir_bits = direction == 2 ? 1 : 0;
    kl.node_bits = bits_for((u64)g->num_nodes - 1);
    if (route == 1 && kl.total() > 64) return RGCN_ERR_PLAN;
    const bool two_sorts = route == 2 || (route == 0 && kl.total() > 64);
    const u32 M = (u32)round_keys(g->num_edges, direction), N = (u32)g->num_nodes;
    Workspace ws = carve(workspace, M, N);
    if (workspace_bytes < ws.bytes) return RGCN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(ws.res, 0, sizeof(Results), s);
    if (e == hipSuccess) e = hipMemsetAsync(ws.sig_lo, 0, (size_t)N * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(ws.sig_hi, 0, (size_t)N * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(ws.node_b, 0, ((size_t)N + 1) * 4, s);
    if (e != hipSuccess) return (int)e;

    if (M > 0) {
        hipLaunchKernelGGL(round_keys_kernel, dim3(grid_for(M)), dim3(256), 0, s, g->src, g->src_stride, g->dst, g->dst_stride,
                           g->type, g->type_stride, block_in, (u64)M, direction, N, (u32)g->num_relations, (u32)num_blocks_in, kl,
                           two_sorts ? 1 : 0, ws.sb.k[0], ws.sb.v[0], ws.res);
        const u64* sorted;
        int elem_bits;
        if (!two_sorts) {
            sorted = ws.sb.k[radix_sort_pairs(ws.sb, M, kl.total(), s)];
            elem_bits = kl.elem_bits();      // (1 .. 63: the owner has at least one bit)
        } else {
            const int c1 = radix_sort_pairs(ws.sb, M, kl.elem_bits(), s);
            run_ids(ws.sb.k[c1], M, 0, ws.scan_a, ws.scan_b, ws.sb.sums, s);
            // the owners sit in v[c1]; the second sort's input goes to the other pair
            hipLaunchKernelGGL(rank_keys_kernel, dim3(grid_for(M)), dim3(256), 0, s, ws.sb.v[c1], ws.scan_b, M, ws.sb.k[c1 ^ 1],
                               ws.sb.v[c1 ^ 1]);
            const SortBufs sb2 = from_pair(ws.sb, c1 ^ 1);
            sorted = sb2.k[radix_sort_pairs(sb2, M, kl.node_bits, s)];
            elem_bits = 0;
        }
        const u32 waves = (M + 63u) / 64u;
        hipLaunchKernelGGL(signature_kernel, dim3((waves + 3u) / 4u), dim3(256), 0, s, sorted, M, elem_bits, ws.sig_lo, ws.sig_hi);
    }
    hipLaunchKernelGGL(fold_kernel, dim3(grid_for(N)), dim3(256), 0, s, ws.sig_lo, ws.sig_hi, block_in, N, ws.sb.k[0], ws.sb.v[0]);
    const int c1 = radix_sort_pairs(ws.sb, N, 64, s);
    hipLaunchKernelGGL(gather_words_kernel, dim3(grid_for(N)), dim3(256), 0, s, ws.sig_hi, ws.sb.v[c1], N, ws.sb.k[c1]);
    const SortBufs sb2 = from_pair(ws.sb, c1);
    const int c2 = radix_sort_pairs(sb2, N, 64, s);
    const u64* hi_sorted = sb2.k[c2];
    const u32* node = sb2.v[c2];
    hipLaunchKernelGGL(block_heads_kernel, dim3(grid_for(N)), dim3(256), 0, s, hi_sorted, ws.sig_lo, node, N, ws.scan_a);
    exclusive_scan(ws.scan_a, ws.scan_b, N, ws.sb.sums, s);
    hipLaunchKernelGGL(block_first_kernel, dim3(grid_for(N)), dim3(256), 0, s, ws.scan_a, ws.scan_b, node, N, ws.node_a, ws.node_b);
    u32* cid = (u32*)ws.sig_hi;      // (dead since the second sort's keys were gathered: N u64 hold N + 1 u32)
    exclusive_scan(ws.node_b, cid, N, ws.sb.sums, s);
    hipLaunchKernelGGL(block_ids_kernel, dim3(grid_for(N)), dim3(256), 0, s, ws.scan_a, ws.scan_b, node, N, ws.node_a, cid, block_out,
                       ws.sb.sums + scan_blocks(N), ws.res);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    Results r;
    if ((st = read_back(ws.res, &r, s)) != 0) return st;
    if (r.error) return RGCN_ERR_GRAPH;
    *num_blocks_out = (int32_t)r.count;
    return RGCN_OK;
}

extern "C" int rgcn_summary_quotient(const rgcn_graph_t* g, const int32_t* block, int32_t num_blocks, int route, int64_t* src_out,
                                     int64_t* dst_out, int64_t* type_out, int64_t* mult_out, void* workspace, size_t workspace_bytes,
                                     int64_t* num_edges_out, void* stream) {
    int st = check_graph(g);
    if (st != RGCN_OK) return st;
    if (!block || !workspace || !num_edges_out) return RGCN_ERR_NULL;
    if (g->num_edges > 0 && (!src_out || !dst_out || !type_out || !mult_out)) return RGCN_ERR_NULL;
    if (num_blocks < 1 || route < 0 || route > 2) return RGCN_ERR_PLAN;
    if ((u64)g->num_edges > kMaxKeys) return RGCN_ERR_PLAN;
    QuotKeys kl;
    kl.block_bits = bits_for((u64)num_blocks - 1);
    kl.type_bits = bits_for((u64)g->num_relations - 1);
    if (route == 1 && kl.total() > 64) return RGCN_ERR_PLAN;
    const bool two_sorts = route == 2 || (route == 0 && kl.total() > 64);
    const u32 E = (u32)g->num_edges, N = (u32)g->num_nodes;
    Workspace ws = carve(workspace, E, N);
    if (workspace_bytes < ws.bytes) return RGCN_ERR_WORKSPACE;
    if (E == 0) {
        *num_edges_out = 0;
        return RGCN_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(ws.res, 0, sizeof(Results), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(quot_keys_kernel, dim3(grid_for(E)), dim3(256), 0, s, g->src, g->src_stride, g->dst, g->dst_stride, g->type,
                       g->type_stride, block, (u64)E, N, (u32)g->num_relations, (u32)num_blocks, kl, two_sorts ? 1 : 0, ws.sb.k[0],
                       ws.sb.v[0], ws.res);
    const u64* sorted;
    const u32* edge;
    const u32* bsrc_of_edge = nullptr;
    u32* spare_vals;      // the value buffer the last sort pass read from: dead, and E words wide
    if (!two_sorts) {
        const int c = radix_sort_pairs(ws.sb, E, kl.total(), s);
        sorted = ws.sb.k[c];
        edge = ws.sb.v[c];
        spare_vals = ws.sb.v[c ^ 1];
    } else {
        const int c1 = radix_sort_pairs(ws.sb, E, kl.block_bits, s);
        hipLaunchKernelGGL(quot_second_keys_kernel, dim3(grid_for(E)), dim3(256), 0, s, ws.sb.k[c1], ws.sb.v[c1], E, g->dst,
                           g->dst_stride, g->type, g->type_stride, block, N, (u32)g->num_relations, (u32)num_blocks, kl,
                           ws.sb.k[c1 ^ 1], ws.sb.v[c1 ^ 1], ws.scan_c);
        const SortBufs sb2 = from_pair(ws.sb, c1 ^ 1);
        const int c2 = radix_sort_pairs(sb2, E, kl.type_bits + kl.block_bits, s);
        sorted = sb2.k[c2];
        edge = sb2.v[c2];
        spare_vals = sb2.v[c2 ^ 1];
        bsrc_of_edge = ws.scan_c;
    }
    hipLaunchKernelGGL(quot_heads_kernel, dim3(grid_for(E)), dim3(256), 0, s, sorted, edge, bsrc_of_edge, E, ws.scan_a);
    exclusive_scan(ws.scan_a, ws.scan_b, E, ws.sb.sums, s);
    hipLaunchKernelGGL(publish_count_kernel, dim3(1), dim3(1), 0, s, ws.sb.sums + scan_blocks(E), ws.res);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    Results r;
    if ((st = read_back(ws.res, &r, s)) != 0) return st;
    if (r.error) return RGCN_ERR_GRAPH;
    const u32 n_runs = r.count;      // 1 .. E
    hipLaunchKernelGGL(quot_emit_kernel, dim3(grid_for(E)), dim3(256), 0, s, sorted, edge, bsrc_of_edge, ws.scan_a, ws.scan_b, E, kl,
                       src_out, dst_out, type_out, spare_vals);
    hipLaunchKernelGGL(quot_mult_kernel, dim3(grid_for(n_runs)), dim3(256), 0, s, spare_vals, n_runs, E, mult_out);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    *num_edges_out = (int64_t)n_runs;
    return RGCN_OK;
}

// rgcn_sample.hip -- neighbour sampling ON THE DEVICE behind the C ABI (include/rgcn_mi355x.h: rgcn_sample_index_build,
// rgcn_sample_hop, and for one fan-out per relation rgcn_sample_rel_index_build, rgcn_sample_hop_rel): an in-edge index of a
// graph and one fan-out hop that turns a set of destination nodes into a relabelled bipartite block for
// RGCNConv((x_src, x_dst), ...).  gfx950 only.  DESIGN.md sections 14 and 17 have the semantics.
//
// Both indices and both hops are one skeleton with two front halves.  What they share:
//
// Index (once per graph):
//   keys      a key and the edge id per edge; ids out of range set an error bit
//   sort      one stable sort by the key: the edges of a key keep the input order
//   gather    src (and type) of the sorted edges as int32
//   ptr       exclusive scan of a per-node count (num_nodes + 1 entries)
//
// Hop (once per layer and step), every launch sized on the host -- by the destinations, by the worst-case edge count `cap`
// (grid-stride, bounded by the count on the device) or by the 32-node words of the graph:
//   mark      map[dst_nodes[i]] = i in the caller's persistent num_nodes-entry map; range check
//   ...       the front half: the edge offsets of the sampling units (the total is E_b) and, in sel, the positions Floyd chose
//   expand    one thread per block edge (take-all units need no wave): unit by binary search in the offsets, the in-edge's
//             source and type from the index; a source the map does not hold sets its bit in a num_nodes-bit set
//   frontier  popcount per word, scan: the rank of a set bit IS the ascending order of the new sources -- no sort, no second
//             count to read back; every bit writes src_nodes and its map entry
//   relabel   edge sources through the map
//   reset     the map entries written (destinations, new sources) go back to "none"
//   read      error bits, E_b and the number of new sources: the one copy and the one synchronisation of a hop
//
// One fan-out (section 14): the key is dst, the keys kernel counts the in-degrees that become ptr, the sampling unit is a
// destination.
//   count     min(d, k) per destination; a node listed twice lost one map entry: error, and it counts nothing
//   scan      offsets of every destination's edges
//   floyd     one wave per SAMPLED destination (d > k): Floyd's k-subset, a dependency chain of k draws; the chosen positions sit
//             in registers (ceil(k / 64) per lane), the membership test is one compare per register and a ballot; the wave then
//             ranks its positions (k broadcasts) and stores them in ascending order
//
// One fan-out per relation (section 17): the key is dst * R + type over bits_for(N-1) + bits_for(R-1) bits, so the edges of a
// (dst, type) run keep the input order; between sort and gather
//   heads     head flags over the sorted keys, scan: a head's run number; it writes run_beg / run_type and counts its node's
//             runs, which become run_ptr
// and the sampling unit is a (destination position, run) pair:
//   units     runs per destination (a node listed twice: error, counts nothing) -> scan -> unit offsets, U units
//   count     one thread per unit: min(d, k[type]); its destination and run, kept for the steps below; the units with d > k > 0
//             go to the work list (one atomic per tile of 1,024 units) -> scan -> edge offsets
//   floyd     waves stride over the WORK LIST only: a unit taken whole never sees a wave.  floyd_wave<REGS>, REGS from the
//             largest positive fan-out, the unit's own k a run-time value; the key also mixes the relation
//
// All integer work: no float, no waiting between workgroups, every loop bounded by k, d or the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/rgcn_mi355x.h"
#include "rgcn_sort_scan.h"

namespace rgcn_sample {

using namespace rgcn_sort_scan;

constexpr u32 kErrRange = 1u, kErrDuplicate = 2u;
constexpr u32 kNone = 0xFFFFFFFFu;           // map entry of a node outside the block
constexpr int32_t kMaxRelations = 65536;
constexpr int kMaxFanout = 256;
constexpr u32 kEdgeGridMax = 16384;          // workgroups of an edge-parallel launch: beyond that the threads stride

struct Results {        // device-resident scalars of one call: what the host reads back in one copy
    u32 error;          // kErr* bits
    u32 num_edges;      // E_b
    u32 num_new;        // sources that are no destination
    u32 aux;            // relation index build: the number of runs; per-relation hop: the number of sampled units
};

constexpr u64 kRelMul = 0xD1B54A32D192ED03ull;      // the per-relation term of the generator's key

// ------------------------------------------------------------------------------------------------
// index
// ------------------------------------------------------------------------------------------------
// An id out of range sets the error bit and the key 0: everything later stays inside its arrays whatever the input holds.
// REL: the key is dst * R + type; else it is dst, and deg counts the in-degrees.
template <bool REL>
__global__ void index_keys_kernel(const int64_t* __restrict__ src, int64_t src_stride, const int64_t* __restrict__ dst,
                                  int64_t dst_stride, const int64_t* __restrict__ typ, int64_t typ_stride, u32 num_edges,
                                  u32 n_nodes, u32 num_rel, u64* __restrict__ keys, u32* __restrict__ vals, u32* __restrict__ deg,
                                  Results* __restrict__ res) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= num_edges) return;
    const int64_t sv = src[(u64)e * src_stride], dv = dst[(u64)e * dst_stride], t = typ[(u64)e * typ_stride];
    const bool bad = t < 0 || t >= (int64_t)num_rel || sv < 0 || sv >= (int64_t)n_nodes || dv < 0 || dv >= (int64_t)n_nodes;
    if (bad) atomicOr(&res->error, kErrRange);
    vals[e] = e;
    if (REL) {
        keys[e] = bad ? 0ull : (u64)dv * num_rel + (u64)t;
    } else {
        const u32 v = bad ? 0u : (u32)dv;
        keys[e] = v;
        atomicAdd(&deg[v], 1u);
    }
}

// ids[i]: the run of sorted edge i (run_ids).  run_cnt has num_nodes + 1 zeroed entries; run_beg num_runs + 1 <= E + 1.
__global__ void rel_heads_kernel(const u64* __restrict__ keys, const u32* __restrict__ flag, const u32* __restrict__ ids,
                                 u32 num_edges, u32 num_rel, u32* __restrict__ run_cnt, u32* __restrict__ run_beg,
                                 int32_t* __restrict__ run_type, Results* __restrict__ res) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_edges) return;
    const u32 q = ids[i];
    if (flag[i] != 0u) {
        const u64 key = keys[i];
        const u64 v = key / num_rel;      // (< n_nodes: the key kernel checked the ranges)
        run_beg[q] = i;
        run_type[q] = (int32_t)(key - v * num_rel);
        atomicAdd(&run_cnt[v], 1u);
    }
    if (i == num_edges - 1u) {
        run_beg[q + 1u] = num_edges;
        res->aux = q + 1u;
    }
}

// TYPES: type_sorted is written too; else the type arguments go unread and type_sorted may be null.
template <bool TYPES>
__global__ void index_gather_kernel(const u32* __restrict__ edge, u32 num_edges, const int64_t* __restrict__ src, int64_t src_stride,
                                    const int64_t* __restrict__ typ, int64_t typ_stride, u32 n_nodes, u32 num_rel,
                                    int32_t* __restrict__ src_sorted, int32_t* __restrict__ type_sorted) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_edges) return;
    const u32 e = edge[i];
    const int64_t sv = src[(u64)e * src_stride];
    src_sorted[i] = (sv < 0 || sv >= (int64_t)n_nodes) ? 0 : (int32_t)sv;      // (else: the error bit is set already)
    if (TYPES) {
        const int64_t t = typ[(u64)e * typ_stride];
        type_sorted[i] = (t < 0 || t >= (int64_t)num_rel) ? 0 : (int32_t)t;
    }
}

struct IndexWorkspace {
    SortBufs sb;      // (relation index: after the sort the pair that does not hold the result holds flags and run ids)
    Results* res;
    size_t bytes;
};

// sums serves the scan over the nodes; rel: also run_ids over the edges
static IndexWorkspace carve_index(void* base, u64 num_edges, u64 n_nodes, bool rel) {
    IndexWorkspace w;
    Arena ar(base);
    w.res = ar.take<Results>(1);
    w.sb = take_sort_bufs(ar, num_edges, rel && num_edges > n_nodes + 1 ? num_edges : n_nodes + 1);
    w.bytes = ar.bytes();
    return w;
}

// what both index builds ask of their graph, before their own outputs
static int check_graph(const rgcn_graph_t* g) {
    if (g == nullptr) return RGCN_ERR_NULL;
    if (g->num_edges < 0 || g->num_nodes <= 0 || g->num_relations <= 0 || g->num_relations > kMaxRelations) return RGCN_ERR_PLAN;
    if ((u64)g->num_edges > kMaxKeys) return RGCN_ERR_PLAN;
    if (g->num_edges > 0 && (!g->src || !g->dst || !g->type)) return RGCN_ERR_NULL;
    return RGCN_OK;
}

// The two builds between their key kernel and their gather: memsets before, node scan, last error, read-back and decode after.
// `mid(c)` is what a build launches between the sort (result in pair c) and the gather.
template <bool REL, class Mid>
static int index_build(const rgcn_graph_t* g, u32* node_cnt, int32_t* src_out, int32_t* type_out, const IndexWorkspace& ws,
                       hipStream_t s, Results* r, Mid&& mid) {
    const u32 E = (u32)g->num_edges, N = (u32)g->num_nodes, R = (u32)g->num_relations;
    hipError_t e = hipMemsetAsync(ws.res, 0, sizeof(Results), s);
    if (e == hipSuccess) e = hipMemsetAsync(node_cnt, 0, ((size_t)N + 1) * 4, s);
    if (e != hipSuccess) return (int)e;
    if (E > 0) {
        hipLaunchKernelGGL(index_keys_kernel<REL>, dim3(grid_for(E)), dim3(256), 0, s, g->src, g->src_stride, g->dst, g->dst_stride,
                           g->type, g->type_stride, E, N, R, ws.sb.k[0], ws.sb.v[0], node_cnt, ws.res);
        const int c = radix_sort_pairs(ws.sb, E, bits_for((u64)N - 1) + (REL ? bits_for((u64)R - 1) : 0), s);
        mid(c);
        hipLaunchKernelGGL(index_gather_kernel<!REL>, dim3(grid_for(E)), dim3(256), 0, s, ws.sb.v[c], E, g->src, g->src_stride, g->type,
                           g->type_stride, N, R, src_out, type_out);
    }
    exclusive_scan(node_cnt, node_cnt, N + 1u, ws.sb.sums, s);      // counts per node -> ptr / run_ptr, its last entry the total
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    const int st = read_back(ws.res, r, s);
    if (st != 0) return st;
    return r->error ? RGCN_ERR_GRAPH : RGCN_OK;
}

// ------------------------------------------------------------------------------------------------
// hop
// ------------------------------------------------------------------------------------------------
// A destination out of range marks nothing.  src_nodes starts with the destinations.
__global__ void hop_mark_kernel(const int64_t* __restrict__ dst_nodes, u32 n_dst, u32 n_nodes, u32* __restrict__ map,
                                int64_t* __restrict__ src_nodes, Results* __restrict__ res) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_dst) return;
    const int64_t v = dst_nodes[i];
    src_nodes[i] = v;
    if (v < 0 || v >= (int64_t)n_nodes) {
        atomicOr(&res->error, kErrRange);
        return;
    }
    map[v] = i;
}

// cnt has n_dst + 1 entries (the last one 0: its scan is E_b).  Of a node listed twice one position lost the map entry: it counts
// nothing, so the counts add up to at most the edges of the graph -- and of `cap` -- whatever the list holds.
__global__ void hop_count_kernel(const int64_t* __restrict__ dst_nodes, u32 n_dst, u32 n_nodes, const u32* __restrict__ ptr,
                                 int fanout, const u32* __restrict__ map, u32* __restrict__ cnt, Results* __restrict__ res) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_dst) return;
    u32 c = 0u;
    if (i < n_dst) {
        const int64_t v = dst_nodes[i];
        if (v >= 0 && v < (int64_t)n_nodes) {
            if (map[v] != i) {
                atomicOr(&res->error, kErrDuplicate);
            } else {
                const u32 d = ptr[v + 1] - ptr[v];
                c = (fanout < 0 || d <= (u32)fanout) ? d : (u32)fanout;
            }
        }
    }
    cnt[i] = c;
}

// Floyd's k-subset of the positions 0 .. d-1 (d > k >= 1) by one wave, stored ascending at out[0 .. k-1]: for j = d-k .. d-1:
// t = draw(j) in [0, j]; add j if t is chosen already, else t.  Slot t (0 .. k-1) of the chosen set lives in register t / 64 of
// lane t % 64 (k <= 64 * REGS, a run-time value); the membership test is one compare per register and a ballot; the rank of a
// chosen position = chosen positions below it (k broadcasts).  Every lane of the wave must call it with the same d, k, kv.
template <int REGS>
__device__ inline void floyd_wave(u32 d, u32 k, u64 kv, u32 lane, u32* __restrict__ out) {
    u32 c[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) c[r] = kNone;      // (positions stay below 0xFFFF0000: no position equals an empty slot)
    for (u32 t = 0; t < k; ++t) {
        const u32 j = d - k + t;
        const u64 rnd = mix(kv + (u64)j);
        const u32 draw = (u32)(((rnd >> 32) * ((u64)j + 1ull)) >> 32);
        bool hit = false;
#pragma unroll
        for (int r = 0; r < REGS; ++r) hit = hit || c[r] == draw;
        const u32 val = __ballot(hit) != 0ull ? j : draw;
#pragma unroll
        for (int r = 0; r < REGS; ++r)
            if ((u32)r == (t >> 6) && lane == (t & 63u)) c[r] = val;
    }
    u32 rank[REGS];
#pragma unroll
    for (int r = 0; r < REGS; ++r) rank[r] = 0u;
#pragma unroll
    for (int q = 0; q < REGS; ++q) {
        if ((u32)q * 64u >= k) break;
        const u32 in_reg = k - (u32)q * 64u < 64u ? k - (u32)q * 64u : 64u;      // slots of register q in use
        for (u32 l = 0; l < in_reg; ++l) {
            const u32 b = (u32)__shfl((int)c[q], (int)l);
#pragma unroll
            for (int r = 0; r < REGS; ++r) rank[r] += b < c[r] ? 1u : 0u;
        }
    }
#pragma unroll
    for (int r = 0; r < REGS; ++r)
        if ((u32)r * 64u + lane < k) out[rank[r]] = c[r];
}

// One wave per destination; a wave whose destination is taken whole (or counts nothing) leaves at once: off[i + 1] - off[i] is k
// exactly where d > k.  The block's edges of a destination ascend by in-edge position.
template <int REGS>
__global__ void hop_floyd_kernel(const int64_t* __restrict__ dst_nodes, u32 n_dst, const u32* __restrict__ ptr, u32 k,
                                 u64 key, const u32* __restrict__ off, u32* __restrict__ sel) {
    const u32 i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const u32 lane = threadIdx.x & 63u;
    if (i >= n_dst) return;
    const u32 base = off[i];
    if (off[i + 1] - base != k) return;
    const int64_t v = dst_nodes[i];      // (in range and listed once: it has edges)
    const u32 d = ptr[v + 1] - ptr[v];
    if (d <= k) return;
    floyd_wave<REGS>(d, k, mix(key + (u64)v), lane, sel + base);
}

// destination position of block edge e: the last i with off[i] <= e (off has n_dst + 1 entries, off[n_dst] = E_b > e)
__device__ inline u32 owner_of(const u32* __restrict__ off, u32 n_dst, u32 e) {
    u32 lo = 0, hi = n_dst;      // answer in [lo, hi)
    while (hi - lo > 1u) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// What expand_kernel asks of the sampling units, by value: count() of them hold edges, off has their edge offsets and off[last()]
// the block's edge total; unit(u): where in the index its edges begin, how many there are, its destination position and run
// (one fan-out: none); type(u, p): the type of its edge at position p.
struct Unit { u32 begin, d, dst, run; };

struct NodeUnits {      // one fan-out: unit i is destination i, its edges the in-edges of the node
    const int64_t* __restrict__ dst_nodes;
    const u32* __restrict__ ptr;
    const int32_t* __restrict__ type_sorted;
    const u32* __restrict__ off;
    u32 n_dst;
    __device__ u32 count() const { return n_dst; }
    __device__ u32 last() const { return n_dst; }
    __device__ Unit unit(u32 i) const {
        const int64_t v = dst_nodes[i];      // (in range: it has edges)
        return {ptr[v], ptr[v + 1] - ptr[v], i, 0u};
    }
    __device__ int32_t type(const Unit& u, u32 p) const { return type_sorted[(u64)u.begin + p]; }
};

struct RunUnits {      // one fan-out per relation: unit u is run urun[u] of destination udst[u]
    const u32* __restrict__ uoff;
    u32 n_dst, ucap;
    const u32* __restrict__ run_beg;
    const int32_t* __restrict__ run_type;
    const u32* __restrict__ off;
    const u32* __restrict__ udst;
    const u32* __restrict__ urun;
    __device__ u32 count() const { return uoff[n_dst] < ucap ? uoff[n_dst] : ucap; }
    __device__ u32 last() const { return ucap; }
    __device__ Unit unit(u32 u) const {
        const u32 q = urun[u];
        return {run_beg[q], run_beg[q + 1] - run_beg[q], udst[u], q};
    }
    __device__ int32_t type(const Unit& u, u32) const { return run_type[u.run]; }
};

// sel[e]: in: the position in its unit of a sampled unit's edge (the floyd kernels); out: the edge's GLOBAL source
template <class Units>
__global__ void expand_kernel(const Units units, const int32_t* __restrict__ src_sorted, const u32* __restrict__ map,
                              u32* __restrict__ sel, u32* __restrict__ bits, int64_t* __restrict__ edge_dst,
                              int64_t* __restrict__ edge_type, Results* __restrict__ res) {
    const u32 n_units = units.count(), total = units.off[units.last()];
    const u64 stride = (u64)gridDim.x * blockDim.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) res->num_edges = total;
    for (u64 e64 = (u64)blockIdx.x * blockDim.x + threadIdx.x; e64 < total; e64 += stride) {
        const u32 e = (u32)e64;
        const u32 i = owner_of(units.off, n_units, e);      // (off[n_units] = E_b > e)
        const u32 first = units.off[i], count = units.off[i + 1] - first;
        const Unit u = units.unit(i);
        const u32 p = count == u.d ? e - first : sel[e];
        const u32 s = (u32)src_sorted[(u64)u.begin + p];
        edge_dst[e] = (int64_t)u.dst;
        edge_type[e] = (int64_t)units.type(u, p);
        sel[e] = s;
        if (map[s] == kNone) atomicOr(&bits[s >> 5], 1u << (s & 31u));
    }
}

__global__ void hop_popcount_kernel(const u32* __restrict__ bits, u32 n_words, u32* __restrict__ wcnt) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w > n_words) return;
    wcnt[w] = w < n_words ? (u32)__popc(bits[w]) : 0u;      // (n_words + 1 entries: the scan of the last one is the total)
}

// woff = exclusive scan of the popcounts: bit b of word w is new source number woff[w] + (set bits of w below b)
__global__ void hop_frontier_kernel(const u32* __restrict__ bits, u32 n_words, const u32* __restrict__ woff, u32 n_dst,
                                    u32* __restrict__ map, int64_t* __restrict__ src_nodes, Results* __restrict__ res) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w == 0) res->num_new = woff[n_words];
    if (w >= n_words) return;
    u32 m = bits[w], r = n_dst + woff[w];
    while (m != 0u) {      // at most 32 trips
        const u32 b = (u32)__ffs((int)m) - 1u;
        m &= m - 1u;
        const u32 s = w * 32u + b;
        src_nodes[r] = (int64_t)s;
        map[s] = r;
        ++r;
    }
}

__global__ void hop_relabel_kernel(const u32* __restrict__ off, u32 n_dst, const u32* __restrict__ sel, const u32* __restrict__ map,
                                   int64_t* __restrict__ edge_src) {
    const u32 total = off[n_dst];
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) edge_src[e] = (int64_t)map[sel[e]];
}

__global__ void hop_reset_dst_kernel(const int64_t* __restrict__ dst_nodes, u32 n_dst, u32 n_nodes, u32* __restrict__ map) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_dst) return;
    const int64_t v = dst_nodes[i];
    if (v >= 0 && v < (int64_t)n_nodes) map[v] = kNone;
}

__global__ void hop_reset_new_kernel(const u32* __restrict__ bits, u32 n_words, u32* __restrict__ map) {
    const u32 w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n_words) return;
    u32 m = bits[w];
    while (m != 0u) {
        const u32 b = (u32)__ffs((int)m) - 1u;
        m &= m - 1u;
        map[w * 32u + b] = kNone;
    }
}

// f(std::integral_constant<int, REGS>{}) with the REGS of floyd_wave that hold kmax (1 .. 256) chosen positions
template <class F>
static void for_floyd_regs(int kmax, F&& f) {
    if (kmax <= 64) f(std::integral_constant<int, 1>{});
    else if (kmax <= 128) f(std::integral_constant<int, 2>{});
    else if (kmax <= 192) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 4>{});
}

// the most edges a block (units a hop) can hold: `each` per destination, never more than the index has
static u64 at_most(int64_t num_dst, u64 each, int64_t in_index) {
    const u64 c = (u64)num_dst * each;
    return c < (u64)in_index ? c : (u64)in_index;
}

static u32 edge_grid(u64 cap) {      // workgroups of a launch that strides over the block's edges
    const u32 g = grid_for(cap);
    return g < kEdgeGridMax ? g : kEdgeGridMax;
}

// ---- what a hop does whichever its sampling unit: arguments, workspace tail, first and last launches ------------------------------
struct HopArgs {      // the arguments rgcn_sample_hop and rgcn_sample_hop_rel share
    const int64_t* dst_nodes;
    int64_t num_dst, seed;
    int hop;
    u32* node_map;
    int64_t *edge_src_out, *edge_dst_out, *edge_type_out, *src_nodes_out;
    void* workspace;
    size_t workspace_bytes;
    int64_t *num_edges_out, *num_src_out;
    hipStream_t s;
};

struct HopShared {      // the part of a hop's workspace every hop has
    Results* res;
    u32* sel;       // cap
    u32* bits;      // n_words
    u32* wcnt;      // n_words + 1: popcounts, scanned in place
    u32* sums;
    size_t bytes;
};

// the last takes of a hop's workspace; longest_scan: the hop's own longest scan
static void take_hop_tail(Arena& ar, HopShared& w, u64 cap, u64 n_nodes, u64 longest_scan) {
    const u64 n_words = (n_nodes + 31) / 32;
    w.sel = ar.take<u32>(cap);
    w.bits = ar.take<u32>(n_words);
    w.wcnt = ar.take<u32>(n_words + 1);
    const u64 scan_len = longest_scan > n_words + 1 ? longest_scan : n_words + 1;
    w.sums = ar.take<u32>((size_t)scan_blocks((u32)scan_len) + 2);
    w.bytes = ar.bytes();
}

// A hop's first part, after its own checks of sizes and fan-outs: the checks every hop makes, then the scalars and the bit set
// zeroed and the destinations marked.  index_ok: the index has the arrays its edge count asks for; cap: the hop's edge bound (cap
// and ws are read once the scalars they come from have passed); *key: the generator's key of (seed, hop).  A hop without
// destinations is done here: its caller returns.
static int hop_begin(const HopArgs& a, const HopShared& ws, int32_t num_nodes, bool index_ok, u64 cap, u64* key) {
    if (a.seed < 0 || a.hop < 0 || a.num_dst < 0 || a.num_dst > (int64_t)num_nodes) return RGCN_ERR_ARG;
    if (!index_ok || !a.node_map || !a.workspace || !a.num_edges_out || !a.num_src_out) return RGCN_ERR_NULL;
    if (a.num_dst > 0 && (!a.dst_nodes || !a.src_nodes_out)) return RGCN_ERR_NULL;
    if (cap > 0 && (!a.edge_src_out || !a.edge_dst_out || !a.edge_type_out)) return RGCN_ERR_NULL;
    if (a.workspace_bytes < ws.bytes) return RGCN_ERR_WORKSPACE;
    if (a.num_dst == 0) {
        *a.num_edges_out = 0;
        *a.num_src_out = 0;
        return RGCN_OK;
    }
    const u32 N = (u32)num_nodes, nd = (u32)a.num_dst;
    hipError_t e = hipMemsetAsync(ws.res, 0, sizeof(Results), a.s);
    if (e == hipSuccess) e = hipMemsetAsync(ws.bits, 0, (size_t)((N + 31u) / 32u) * 4, a.s);
    if (e != hipSuccess) return (int)e;
    *key = mix((u64)a.seed + 0x9E3779B97F4A7C15ull * ((u64)a.hop + 1ull));
    hipLaunchKernelGGL(hop_mark_kernel, dim3(grid_for(nd)), dim3(256), 0, a.s, a.dst_nodes, nd, N, a.node_map, a.src_nodes_out, ws.res);
    return RGCN_OK;
}

// Everything after expand.  edges: the block can hold edges and expand ran; off[n_off]: the block's edge total.  Every return
// waits for the stream first (the per-relation hop's host fan-outs are copied on it) and reports a failed launch second.
static int hop_finish(const HopArgs& a, const HopShared& ws, u32 N, bool edges, u64 cap, const u32* off, u32 n_off) {
    const u32 nd = (u32)a.num_dst, n_words = (N + 31u) / 32u;
    hipStream_t s = a.s;
    if (edges) {
        hipLaunchKernelGGL(hop_popcount_kernel, dim3(grid_for((u64)n_words + 1)), dim3(256), 0, s, ws.bits, n_words, ws.wcnt);
        exclusive_scan(ws.wcnt, ws.wcnt, n_words + 1u, ws.sums, s);
        hipLaunchKernelGGL(hop_frontier_kernel, dim3(grid_for(n_words)), dim3(256), 0, s, ws.bits, n_words, ws.wcnt, nd, a.node_map,
                           a.src_nodes_out, ws.res);
        hipLaunchKernelGGL(hop_relabel_kernel, dim3(edge_grid(cap)), dim3(256), 0, s, off, n_off, ws.sel, a.node_map, a.edge_src_out);
        hipLaunchKernelGGL(hop_reset_new_kernel, dim3(grid_for(n_words)), dim3(256), 0, s, ws.bits, n_words, a.node_map);
    }
    hipLaunchKernelGGL(hop_reset_dst_kernel, dim3(grid_for(nd)), dim3(256), 0, s, a.dst_nodes, nd, N, a.node_map);
    const hipError_t e = hipGetLastError();
    Results r;
    const int st = read_back(ws.res, &r, s);
    if (e != hipSuccess) return (int)e;
    if (st != 0) return st;
    if (r.error & kErrRange) return RGCN_ERR_GRAPH;
    if (r.error & kErrDuplicate) return RGCN_ERR_ARG;
    *a.num_edges_out = (int64_t)r.num_edges;
    *a.num_src_out = (int64_t)nd + (int64_t)r.num_new;
    return RGCN_OK;
}

struct HopWorkspace : HopShared {      // one fan-out
    u32* cnt;       // n_dst + 1: counts, scanned in place into offsets
};

static HopWorkspace carve_hop(void* base, u64 n_dst, u64 cap, u64 n_nodes) {
    HopWorkspace w;
    Arena ar(base);
    w.res = ar.take<Results>(1);
    w.cnt = ar.take<u32>(n_dst + 1);
    take_hop_tail(ar, w, cap, n_nodes, n_dst + 1);
    return w;
}

// ---- one fan-out per relation: the hop's own kernels and workspace ------------------------------------------------
struct RelFanouts {      // what the host learns from a fan-out vector before any launch
    int kmax;           // the largest positive entry (0: none)
    bool any_all;       // an entry is -1
    u64 sum;            // sum of max(k[t], 0)
};

static int check_rel_fanouts(const int32_t* fanouts, int32_t num_rel, RelFanouts* f) {
    f->kmax = 0;
    f->any_all = false;
    f->sum = 0;
    for (int32_t t = 0; t < num_rel; ++t) {
        const int32_t k = fanouts[t];
        if (k < -1 || k > kMaxFanout) return RGCN_ERR_ARG;
        if (k == -1) f->any_all = true;
        if (k > 0) f->sum += (u64)k;
        if (k > f->kmax) f->kmax = k;
    }
    return RGCN_OK;
}

static u64 rel_cap(int64_t num_dst, const RelFanouts& f, int64_t num_edges) {
    return f.any_all ? (u64)num_edges : at_most(num_dst, f.sum, num_edges);
}

// ucnt has n_dst + 1 entries (the last one 0: its scan is U).  A node has at most R runs and the runs of distinct nodes are
// distinct: U <= ucap whatever the list holds.
__global__ void rel_units_kernel(const int64_t* __restrict__ dst_nodes, u32 n_dst, u32 n_nodes, const u32* __restrict__ run_ptr,
                                 const u32* __restrict__ map, u32* __restrict__ ucnt, Results* __restrict__ res) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n_dst) return;
    u32 c = 0u;
    if (i < n_dst) {
        const int64_t v = dst_nodes[i];
        if (v >= 0 && v < (int64_t)n_nodes) {
            if (map[v] != i) atomicOr(&res->error, kErrDuplicate);
            else c = run_ptr[v + 1] - run_ptr[v];
        }
    }
    ucnt[i] = c;
}

// ecnt has ucap + 1 entries, the ones from U on 0 (its scan's last entry is E_b).  A workgroup walks tiles of 1,024 units, four per
// thread, and appends the tile's sampled units to the work list with ONE atomic: ballots number them inside a wave, LDS across the
// waves.  (One atomic per wave was measured first: on 889,245 units of which 13,490 are sampled this kernel took 108 us, 90 of them
// the 12,000 returning atomics on one word)  The order of the work list is arbitrary, what it leads to is not.
constexpr int kCountItems = 4;
constexpr u32 kCountTile = 256u * kCountItems;
__global__ void rel_count_kernel(const int64_t* __restrict__ dst_nodes, u32 n_dst, const u32* __restrict__ run_ptr,
                                 const u32* __restrict__ run_beg, const int32_t* __restrict__ run_type,
                                 const int32_t* __restrict__ fan, const u32* __restrict__ uoff, u32 ucap, u32* __restrict__ ecnt,
                                 u32* __restrict__ udst, u32* __restrict__ urun, u32* __restrict__ work, Results* __restrict__ res) {
    __shared__ u32 wave_tot[4];
    __shared__ u32 tile_base;
    const u32 units = uoff[n_dst] < ucap ? uoff[n_dst] : ucap;
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 below = (1ull << lane) - 1ull;
    for (u64 tile = (u64)blockIdx.x * kCountTile; tile <= ucap; tile += (u64)gridDim.x * kCountTile) {      // (uniform per workgroup)
        u32 slot[kCountItems], in_wave = 0u;
        bool sampled[kCountItems];
#pragma unroll
        for (int j = 0; j < kCountItems; ++j) {
            const u64 u = tile + (u64)j * 256u + threadIdx.x;
            u32 c = 0u;
            sampled[j] = false;
            if (u < units) {
                const u32 i = owner_of(uoff, n_dst, (u32)u);
                const int64_t v = dst_nodes[i];      // (in range and listed once: it has runs)
                const u32 q = run_ptr[v] + ((u32)u - uoff[i]);
                const u32 d = run_beg[q + 1] - run_beg[q];
                const int32_t k = fan[run_type[q]];
                c = (k < 0 || d <= (u32)k) ? d : (u32)k;
                sampled[j] = k > 0 && d > (u32)k;
                udst[u] = i;
                urun[u] = q;
            }
            if (u <= ucap) ecnt[u] = c;
            const u64 m = __ballot(sampled[j]);
            slot[j] = in_wave + (u32)__popcll(m & below);
            in_wave += (u32)__popcll(m);
        }
        if (lane == 0u) wave_tot[wave] = in_wave;
        __syncthreads();
        if (threadIdx.x == 0u) {
            const u32 tot = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
            tile_base = tot != 0u ? atomicAdd(&res->aux, tot) : 0u;
        }
        __syncthreads();
        u32 base = tile_base;
        for (u32 w = 0; w < wave; ++w) base += wave_tot[w];
#pragma unroll
        for (int j = 0; j < kCountItems; ++j)
            if (sampled[j]) work[base + slot[j]] = (u32)(tile + (u64)j * 256u + threadIdx.x);
        __syncthreads();      // (the next tile writes wave_tot and tile_base again)
    }
}

// The waves of the grid stride over the work list: only units with d > k > 0 are on it.
template <int REGS>
__global__ void rel_floyd_kernel(const int64_t* __restrict__ dst_nodes, const u32* __restrict__ run_beg,
                                 const int32_t* __restrict__ run_type, const int32_t* __restrict__ fan, u64 key,
                                 const u32* __restrict__ udst, const u32* __restrict__ urun, const u32* __restrict__ eoff,
                                 const u32* __restrict__ work, u32 ucap, const Results* __restrict__ res, u32* __restrict__ sel) {
    const u32 n_work = res->aux < ucap ? res->aux : ucap;
    const u64 waves = (u64)gridDim.x * (blockDim.x >> 6);
    const u32 lane = threadIdx.x & 63u;
    for (u64 w = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); w < n_work; w += waves) {
        const u32 u = work[w], q = urun[u];
        const u64 v = (u64)dst_nodes[udst[u]];
        const u32 d = run_beg[q + 1] - run_beg[q];
        const u32 t = (u32)run_type[q];
        const u32 k = (u32)fan[t];
        const u64 kv = mix(mix(key + v) + kRelMul * ((u64)t + 1ull));
        floyd_wave<REGS>(d, k, kv, lane, sel + eoff[u]);
    }
}

constexpr u32 kFloydGridMax = 4096;      // workgroups (of four waves) that stride over the work list

struct HopRelWorkspace : HopShared {
    int32_t* fan;   // R: the fan-out vector
    u32* ucnt;      // n_dst + 1: runs per destination, scanned in place into unit offsets
    u32* ecnt;      // ucap + 1: edges per unit, scanned in place into edge offsets
    u32* udst;      // ucap: destination position of a unit
    u32* urun;      // ucap: run of a unit
    u32* work;      // ucap: the sampled units
};

static HopRelWorkspace carve_hop_rel(void* base, u64 n_dst, u64 ucap, u64 cap, u64 n_nodes, u64 num_rel) {
    HopRelWorkspace w;
    Arena ar(base);
    w.res = ar.take<Results>(1);
    w.fan = ar.take<int32_t>(num_rel);
    w.ucnt = ar.take<u32>(n_dst + 1);
    w.ecnt = ar.take<u32>(ucap + 1);
    w.udst = ar.take<u32>(ucap);
    w.urun = ar.take<u32>(ucap);
    w.work = ar.take<u32>(ucap);
    take_hop_tail(ar, w, cap, n_nodes, n_dst + 1 > ucap + 1 ? n_dst + 1 : ucap + 1);
    return w;
}

static int check_rel_sizes(int64_t num_edges, int64_t num_runs, int32_t num_nodes, int32_t num_rel) {
    if (num_nodes <= 0 || num_edges < 0 || (u64)num_edges > kMaxKeys || num_runs < 0 || num_runs > num_edges) return RGCN_ERR_PLAN;
    if (num_rel <= 0 || num_rel > kMaxRelations) return RGCN_ERR_PLAN;
    return RGCN_OK;
}

}  // namespace rgcn_sample

using namespace rgcn_sample;

extern "C" size_t rgcn_sample_index_workspace_bytes(int64_t num_edges, int32_t num_nodes) {
    if (num_edges < 0 || num_nodes <= 0 || (u64)num_edges > kMaxKeys) return 0;
    return carve_index(nullptr, (u64)num_edges, (u64)num_nodes, false).bytes;
}

extern "C" int rgcn_sample_index_build(const rgcn_graph_t* g, uint32_t* ptr_out, int32_t* src_out, int32_t* type_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    const int st = check_graph(g);
    if (st != RGCN_OK) return st;
    if (g->num_edges > 0 && (!src_out || !type_out)) return RGCN_ERR_NULL;
    if (!ptr_out || !workspace) return RGCN_ERR_NULL;
    const IndexWorkspace ws = carve_index(workspace, (u64)g->num_edges, (u64)g->num_nodes, false);
    if (workspace_bytes < ws.bytes) return RGCN_ERR_WORKSPACE;
    Results r;
    return index_build<false>(g, ptr_out, src_out, type_out, ws, (hipStream_t)stream, &r, [](int) {});      // in-degrees -> ptr
}

extern "C" size_t rgcn_sample_hop_workspace_bytes(int64_t num_dst, int fanout, int64_t num_edges, int32_t num_nodes) {
    if (num_edges < 0 || num_nodes <= 0 || (u64)num_edges > kMaxKeys || num_dst < 0 || num_dst > (int64_t)num_nodes) return 0;
    if (fanout != -1 && (fanout < 1 || fanout > kMaxFanout)) return 0;
    const u64 cap = fanout < 0 ? (u64)num_edges : at_most(num_dst, (u64)fanout, num_edges);
    return carve_hop(nullptr, (u64)num_dst, cap, (u64)num_nodes).bytes;
}

extern "C" int rgcn_sample_hop(const rgcn_sample_index_t* ix, const int64_t* dst_nodes, int64_t num_dst, int fanout, int64_t seed,
                               int hop, uint32_t* node_map, int64_t* edge_src_out, int64_t* edge_dst_out, int64_t* edge_type_out,
                               int64_t* src_nodes_out, void* workspace, size_t workspace_bytes, int64_t* num_edges_out,
                               int64_t* num_src_out, void* stream) {
    const HopArgs a = {dst_nodes, num_dst, seed, hop, node_map, edge_src_out, edge_dst_out, edge_type_out, src_nodes_out, workspace,
                       workspace_bytes, num_edges_out, num_src_out, (hipStream_t)stream};
    if (ix == nullptr) return RGCN_ERR_NULL;
    if (ix->num_nodes <= 0 || ix->num_edges < 0 || (u64)ix->num_edges > kMaxKeys) return RGCN_ERR_PLAN;
    if (fanout != -1 && (fanout < 1 || fanout > kMaxFanout)) return RGCN_ERR_ARG;
    const u64 cap = fanout < 0 ? (u64)ix->num_edges : at_most(num_dst, (u64)fanout, ix->num_edges);
    const u32 N = (u32)ix->num_nodes, nd = (u32)num_dst;
    const HopWorkspace ws = carve_hop(workspace, nd, cap, N);
    u64 key;
    const int st = hop_begin(a, ws, ix->num_nodes, ix->ptr && (ix->num_edges == 0 || (ix->src && ix->type)), cap, &key);
    if (st != RGCN_OK || nd == 0) return st;
    hipStream_t s = a.s;
    hipLaunchKernelGGL(hop_count_kernel, dim3(grid_for((u64)nd + 1)), dim3(256), 0, s, dst_nodes, nd, N, ix->ptr, fanout, node_map,
                       ws.cnt, ws.res);
    exclusive_scan(ws.cnt, ws.cnt, nd + 1u, ws.sums, s);
    if (cap > 0) {
        if (fanout > 0) {
            const dim3 grid(grid_for((u64)nd, 4)), block(256);      // four waves, four destinations per workgroup
            for_floyd_regs(fanout, [&](auto regs) {
                hipLaunchKernelGGL(hop_floyd_kernel<decltype(regs)::value>, grid, block, 0, s, dst_nodes, nd, ix->ptr, (u32)fanout, key,
                                   ws.cnt, ws.sel);
            });
        }
        const NodeUnits units = {dst_nodes, ix->ptr, ix->type, ws.cnt, nd};
        hipLaunchKernelGGL(expand_kernel<NodeUnits>, dim3(edge_grid(cap)), dim3(256), 0, s, units, ix->src, node_map, ws.sel, ws.bits,
                           edge_dst_out, edge_type_out, ws.res);
    }
    return hop_finish(a, ws, N, cap > 0, cap, ws.cnt, nd);
}

extern "C" size_t rgcn_sample_rel_index_workspace_bytes(int64_t num_edges, int32_t num_nodes) {
    if (num_edges < 0 || num_nodes <= 0 || (u64)num_edges > kMaxKeys) return 0;
    return carve_index(nullptr, (u64)num_edges, (u64)num_nodes, true).bytes;
}

extern "C" int rgcn_sample_rel_index_build(const rgcn_graph_t* g, uint32_t* run_ptr_out, uint32_t* run_beg_out, int32_t* run_type_out,
                                           int32_t* src_out, void* workspace, size_t workspace_bytes, int64_t* num_runs_out,
                                           void* stream) {
    int st = check_graph(g);
    if (st != RGCN_OK) return st;
    if (g->num_edges > 0 && (!run_type_out || !src_out)) return RGCN_ERR_NULL;
    if (!run_ptr_out || !run_beg_out || !workspace || !num_runs_out) return RGCN_ERR_NULL;
    const u32 E = (u32)g->num_edges, R = (u32)g->num_relations;
    const IndexWorkspace ws = carve_index(workspace, E, (u64)g->num_nodes, true);
    if (workspace_bytes < ws.bytes) return RGCN_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const hipError_t e = hipMemsetAsync(run_beg_out, 0, 4, s);      // (a graph without edges: run_beg = [0])
    if (e != hipSuccess) return (int)e;
    Results r;
    st = index_build<true>(g, run_ptr_out, src_out, nullptr, ws, s, &r, [&](int c) {      // runs per node -> run_ptr
        u32* flag = (u32*)ws.sb.k[c ^ 1];      // the pair the sort left free: 8 B per edge
        u32* ids = flag + E;
        run_ids(ws.sb.k[c], E, 0, flag, ids, ws.sb.sums, s);
        hipLaunchKernelGGL(rel_heads_kernel, dim3(grid_for(E)), dim3(256), 0, s, ws.sb.k[c], flag, ids, E, R, run_ptr_out, run_beg_out,
                           run_type_out, ws.res);
    });
    if (st == RGCN_OK) *num_runs_out = (int64_t)r.aux;
    return st;
}

extern "C" size_t rgcn_sample_hop_rel_workspace_bytes(int64_t num_dst, const int32_t* fanouts, int32_t num_relations,
                                                      int64_t num_edges, int64_t num_runs, int32_t num_nodes) {
    if (check_rel_sizes(num_edges, num_runs, num_nodes, num_relations) != RGCN_OK || !fanouts) return 0;
    if (num_dst < 0 || num_dst > (int64_t)num_nodes) return 0;
    RelFanouts f;
    if (check_rel_fanouts(fanouts, num_relations, &f) != RGCN_OK) return 0;
    return carve_hop_rel(nullptr, (u64)num_dst, at_most(num_dst, (u64)num_relations, num_runs), rel_cap(num_dst, f, num_edges),
                         (u64)num_nodes, (u64)num_relations).bytes;
}

extern "C" int rgcn_sample_hop_rel(const rgcn_sample_rel_index_t* ix, const int64_t* dst_nodes, int64_t num_dst,
                                   const int32_t* fanouts, int64_t seed, int hop, uint32_t* node_map, int64_t* edge_src_out,
                                   int64_t* edge_dst_out, int64_t* edge_type_out, int64_t* src_nodes_out, void* workspace,
                                   size_t workspace_bytes, int64_t* num_edges_out, int64_t* num_src_out, void* stream) {
    const HopArgs a = {dst_nodes, num_dst, seed, hop, node_map, edge_src_out, edge_dst_out, edge_type_out, src_nodes_out, workspace,
                       workspace_bytes, num_edges_out, num_src_out, (hipStream_t)stream};
    if (ix == nullptr || fanouts == nullptr) return RGCN_ERR_NULL;
    int st = check_rel_sizes(ix->num_edges, ix->num_runs, ix->num_nodes, ix->num_relations);
    if (st != RGCN_OK) return st;
    RelFanouts f;
    if ((st = check_rel_fanouts(fanouts, ix->num_relations, &f)) != RGCN_OK) return st;
    const u64 cap = rel_cap(num_dst, f, ix->num_edges);
    const u32 N = (u32)ix->num_nodes, nd = (u32)num_dst, ucap = (u32)at_most(num_dst, (u64)ix->num_relations, ix->num_runs);
    const HopRelWorkspace ws = carve_hop_rel(workspace, nd, ucap, cap, N, (u64)ix->num_relations);
    u64 key;
    st = hop_begin(a, ws, ix->num_nodes, ix->run_ptr && ix->run_beg && (ix->num_edges == 0 || (ix->run_type && ix->src)), cap, &key);
    if (st != RGCN_OK || nd == 0) return st;
    hipStream_t s = a.s;
    // the fan-outs: one copy; every return below goes through hop_finish, which waits for the stream: the caller's array outlives it
    const hipError_t e = hipMemcpyAsync(ws.fan, fanouts, (size_t)ix->num_relations * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        (void)hop_finish(a, ws, N, false, cap, ws.ecnt, ucap);      // (the marks go back)
        return (int)e;
    }
    hipLaunchKernelGGL(rel_units_kernel, dim3(grid_for((u64)nd + 1)), dim3(256), 0, s, dst_nodes, nd, N, ix->run_ptr, node_map, ws.ucnt,
                       ws.res);
    const bool edges = cap > 0 && ucap > 0;      // (an index with edges has runs; every grid below has at least one workgroup)
    if (edges) {
        exclusive_scan(ws.ucnt, ws.ucnt, nd + 1u, ws.sums, s);
        u32 ug = grid_for((u64)ucap + 1, (int)kCountTile);      // one workgroup per tile of 1,024 units
        if (ug > kEdgeGridMax) ug = kEdgeGridMax;
        hipLaunchKernelGGL(rel_count_kernel, dim3(ug), dim3(256), 0, s, dst_nodes, nd, ix->run_ptr, ix->run_beg, ix->run_type, ws.fan,
                           ws.ucnt, ucap, ws.ecnt, ws.udst, ws.urun, ws.work, ws.res);
        exclusive_scan(ws.ecnt, ws.ecnt, ucap + 1u, ws.sums, s);
        if (f.kmax > 0) {
            u32 fg = grid_for((u64)ucap, 4);      // four waves per workgroup, one unit of the work list per wave and trip
            if (fg > kFloydGridMax) fg = kFloydGridMax;
            for_floyd_regs(f.kmax, [&](auto regs) {
                hipLaunchKernelGGL(rel_floyd_kernel<decltype(regs)::value>, dim3(fg), dim3(256), 0, s, dst_nodes, ix->run_beg,
                                   ix->run_type, ws.fan, key, ws.udst, ws.urun, ws.ecnt, ws.work, ucap, ws.res, ws.sel);
            });
        }
        const RunUnits units = {ws.ucnt, nd, ucap, ix->run_beg, ix->run_type, ws.ecnt, ws.udst, ws.urun};
        hipLaunchKernelGGL(expand_kernel<RunUnits>, dim3(edge_grid(cap)), dim3(256), 0, s, units, ix->src, node_map, ws.sel, ws.bits,
                           edge_dst_out, edge_type_out, ws.res);
    }
    return hop_finish(a, ws, N, edges, cap, ws.ecnt, ucap);
}

// rgcn_featureless.hip -- rgcn_featureless_* of include/rgcn_mi355x.h: RGCNConv in PyG's FEATURELESS mode (x absent or an
// int64 node-index vector), where every weight table W_r [in, out] is a trainable per-node embedding:
//   out[i] = bias + root[x_i] + sum_r sum_{j -> i in r} w_e * W_r[x_j]            (x = None: x_j = j)
//   basis:  W_r[row] = sum_b comp[r, b] * V_b[row]   -- composed per gathered row, [R, in, out] never exists.
// No contraction, so no MFMA: a weighted row gather and a weighted segment sum, HBM-bound (DESIGN.md "Featureless layers").
//
// Kernels (one wave per workgroup, one workgroup per plan tile, accumulator of tile x round4(out) floats in LDS):
//   fl_fwd_kernel      walks the tile's chunks of a layout-0 FORWARD plan; per pass S = 64 / L slots of one 16-slot row tile
//                      (L lanes per slot, 4 columns per lane) gather their table rows, a segmented shuffle scan adds the rows
//                      of equal destination (a row tile is sorted by destination), the last lane of every run adds the run's
//                      sum into the LDS row.  One wave walks the passes in plan order: a fixed summation order, no atomics.
//   fl_bwd_kernel      walks the tile's chunks of the TRANSPOSED plan relation by relation (chunks of a tile are relation-
//                      ascending, root last): G_r[j] = sum w * g[i] in LDS, then full weights store G_r into d_weight[r] rows
//                      (zeros for relations without edges in the tile: the dense gradient needs no memset), bases add
//                      comp[r, b] * G_r into B LDS accumulators and keep per-chunk partials of d_comp in a slab.
//   fl_index_reduce    integer x: the per-node rows the walk wrote to the workspace are summed per table row through the
//                      inverted index of x (rows with no node get zeros), in index order.
//   fl_bias_reduce / fl_comp_reduce   fixed-order reductions of the per-tile d_bias and per-chunk d_comp slabs.
// Tables are addressed with 64-bit offsets: rel * in * out passes 2^32 floats on real graphs (AM, full weights: 28 GB).
#include "rgcn_kernels_shared.h"

namespace rgcn {

namespace {

constexpr int kFlLanes = 64;
constexpr int kFlMaxTile = 128;

struct FlArgs {
    // plan
    const int* tile_ptr;
    const int* chunk_rel;
    const int* chunk_cnt;
    const int* slot_src;
    const float* slot_w;
    const int* slot_row;
    int n_nodes, n_tiles, tile, chunk, num_rel;
    // tables: weight [R, in, out] or bases [B, in, out] (+ comp [R, B]); root [in, out] or NULL
    const int64_t* x_index;
    const float* weight;
    const float* comp;
    const float* root;
    int num_bases;
    long in_rows;
    int dout, d4;
    // forward
    const float* bias;
    float* out;
    int ldo;
    // backward
    const float* g;
    int ldg;
    float* d_weight;       // full: [R, in, out]; basis: d_bases [B, in, out]; NULL: not wanted
    float* d_root;
    float* ws_rows;        // integer x: [(T + 1) * n_nodes, 4 * d4] per-node rows (T = R or B, the last block: root)
    float* comp_slab;      // [n_chunks * B] or NULL
    float* bias_slab;      // [n_tiles * 4 * d4] or NULL
};

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }

// four columns 4 c4 .. 4 c4 + 3 of row `row` of a [rows, dout] table (64-bit offsets; beyond dout: zeros)
template <bool VEC>
__device__ __forceinline__ f32x4 table_row(const float* t, long row, int dout, int c4) {
    const float* p = t + (size_t)row * (size_t)dout + 4 * c4;
    if (VEC) return *(const f32x4*)p;
    f32x4 v = zero4();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * c4 + k < dout) v[k] = p[k];
    return v;
}

template <bool VEC>
__device__ __forceinline__ void table_store(float* t, long row, int dout, int c4, f32x4 v) {
    float* p = t + (size_t)row * (size_t)dout + 4 * c4;
    if (VEC) {
        *(f32x4*)p = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * c4 + k < dout) p[k] = v[k];
}

__device__ __forceinline__ f32x4 shfl_up4(f32x4 v, int d) {
    return f32x4{__shfl_up(v[0], d), __shfl_up(v[1], d), __shfl_up(v[2], d), __shfl_up(v[3], d)};
}
__device__ __forceinline__ f32x4 shfl_down4(f32x4 v, int d) {
    return f32x4{__shfl_down(v[0], d), __shfl_down(v[1], d), __shfl_down(v[2], d), __shfl_down(v[3], d)};
}

// Walk one chunk into the LDS accumulator acc [(tile + 1) * d4] (row `tile`: never written).  value(src, w, rowl, c4, slot)
// returns the weighted 16-byte piece of the slot's row.  Slots of a pass lie in one 16-slot row tile (S <= 16), sorted by
// destination: a Hillis-Steele scan over slot positions restricted to equal destinations leaves every run's sum on its last slot.
template <int L, typename F>
__device__ __forceinline__ void walk_chunk(const FlArgs& a, int c, int r0, f32x4* acc, F&& value) {
    constexpr int S = kFlLanes / L;
    const int lane = threadIdx.x;
    const int sp = lane / L, c4 = lane % L;
    const int cnt = __builtin_amdgcn_readfirstlane(ldc(a.chunk_cnt, c));
    const long base = (long)c * a.chunk;
    const int passes = cnt / S;
    for (int p0 = 0; p0 < passes; p0 += 4) {
        f32x4 v[4];
        int dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = zero4();
            dst[u] = a.tile;
            if (p0 + u < passes) {
                const long s = base + (long)(p0 + u) * S + sp;
                const float w = a.slot_w[s];
                const int src = a.slot_src[s];
                if (w != 0.f && (unsigned)src < (unsigned)a.n_nodes) {
                    dst[u] = a.slot_row[s] - r0;
                    if (c4 < a.d4) v[u] = value(src, w, dst[u], c4, s);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (p0 + u >= passes) break;
#pragma unroll
            for (int d = 1; d < S; d <<= 1) {
                const f32x4 up = shfl_up4(v[u], d * L);
                const int dup = __shfl_up(dst[u], d * L);
                if (sp >= d && dup == dst[u]) v[u] += up;
            }
            const int nxt = __shfl_down(dst[u], L);
            const bool end = sp == S - 1 || nxt != dst[u];
            if (end && (unsigned)dst[u] < (unsigned)a.tile && c4 < a.d4) acc[dst[u] * a.d4 + c4] += v[u];
        }
    }
}

__device__ __forceinline__ void zero_rows(f32x4* p, int n4) {
    for (int i = threadIdx.x; i < n4; i += kFlLanes) p[i] = zero4();
}

template <int L, bool VEC, bool BASIS>
__global__ void __launch_bounds__(64) fl_fwd_kernel(const FlArgs a) {
    extern __shared__ f32x4 fl_lds[];
    f32x4* acc = fl_lds;
    const int t = blockIdx.x;
    const int r0 = t * a.tile;
    const int nrows = min(a.tile, a.n_nodes - r0);
    zero_rows(acc, (a.tile + 1) * a.d4);
    __syncthreads();
    const int c0 = ldc(a.tile_ptr, t), c1 = ldc(a.tile_ptr, t + 1);
    for (int c = c0; c < c1; ++c) {
        const int rel = __builtin_amdgcn_readfirstlane(ldc(a.chunk_rel, c));
        const bool is_root = rel >= a.num_rel;
        if (is_root && a.root == nullptr) continue;
        auto value = [&](int src, float w, int, int c4, long) -> f32x4 {
            const long row = a.x_index ? (long)a.x_index[src] : (long)src;
            if ((unsigned long)row >= (unsigned long)a.in_rows) return zero4();
            if (is_root) return w * table_row<VEC>(a.root, row, a.dout, c4);
            if (!BASIS) return w * table_row<VEC>(a.weight + (size_t)rel * (size_t)a.in_rows * a.dout, row, a.dout, c4);
            f32x4 s = zero4();
            for (int b = 0; b < a.num_bases; ++b)
                s += a.comp[(long)rel * a.num_bases + b] * table_row<VEC>(a.weight + (size_t)b * (size_t)a.in_rows * a.dout, row, a.dout, c4);
            return w * s;
        };
        walk_chunk<L>(a, c, r0, acc, value);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nrows * a.d4; i += kFlLanes) {
        const int row = i / a.d4, c4 = i % a.d4;
        f32x4 v = acc[i];
        if (a.bias != nullptr) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * c4 + k < a.dout) v[k] += a.bias[4 * c4 + k];
        }
        *(f32x4*)(a.out + (size_t)(r0 + row) * a.ldo + 4 * c4) = v;
    }
}

// rows [r0, r0 + nrows) of the LDS matrix `m` into table `t` (dout columns) or, integer x, into the workspace block `blk`
template <bool VEC>
__device__ __forceinline__ void store_rows(const FlArgs& a, const f32x4* m, float* t, long blk, int r0, int nrows) {
    for (int i = threadIdx.x; i < nrows * a.d4; i += kFlLanes) {
        const int row = i / a.d4, c4 = i % a.d4;
        const f32x4 v = m ? m[i] : zero4();
        if (a.x_index) *(f32x4*)(a.ws_rows + ((size_t)blk * a.n_nodes + r0 + row) * (size_t)(4 * a.d4) + 4 * c4) = v;
        else table_store<VEC>(t, r0 + row, a.dout, c4, v);
    }
}

template <int L, bool VEC, bool BASIS>
__global__ void __launch_bounds__(64) fl_bwd_kernel(const FlArgs a) {
    extern __shared__ f32x4 fl_lds[];
    const int T4 = a.tile * a.d4;
    f32x4* G = fl_lds;                                   // [(tile + 1) * d4]
    f32x4* dV = fl_lds + T4 + a.d4;                      // basis: [B][tile * d4]
    float* cp = (float*)(dV + (BASIS ? a.num_bases * T4 : 0));   // basis: [B][64] per-lane d_comp partials
    const int lane = threadIdx.x;
    const int t = blockIdx.x;
    const int r0 = t * a.tile;
    const int nrows = min(a.tile, a.n_nodes - r0);
    const int B = a.num_bases;
    const size_t tab = (size_t)a.in_rows * a.dout;
    if (BASIS) {
        zero_rows(dV, B * T4);
        for (int i = lane; i < B * kFlLanes; i += kFlLanes) cp[i] = 0.f;
    }
    // d_bias: this tile's rows of g, fixed tree over the row groups
    if (a.bias_slab != nullptr) {
        constexpr int S = kFlLanes / L;
        const int sp = lane / L, c4 = lane % L;
        f32x4 s = zero4();
        if (c4 < a.d4)
            for (int r = sp; r < nrows; r += S) s += *(const f32x4*)(a.g + (size_t)(r0 + r) * a.ldg + 4 * c4);
#pragma unroll
        for (int d = S / 2; d >= 1; d >>= 1) s += shfl_down4(s, d * L);
        if (sp == 0 && c4 < a.d4) *(f32x4*)(a.bias_slab + ((size_t)t * a.d4 + c4) * 4) = s;
    }
    int c = ldc(a.tile_ptr, t);
    const int c1 = ldc(a.tile_ptr, t + 1);
    auto gather_g = [&](int src, float w, int, int c4, long) -> f32x4 {
        return w * *(const f32x4*)(a.g + (size_t)src * a.ldg + 4 * c4);
    };
    const bool want_w = a.d_weight != nullptr || (BASIS && a.comp_slab != nullptr);
    for (int rel = 0; rel <= a.num_rel; ++rel) {
        const bool is_root = rel == a.num_rel;
        if (is_root && a.d_root == nullptr) break;
        if (!is_root && !want_w) {
            rel = a.num_rel - 1;            // straight to the root chunks
            while (c < c1 && ldc(a.chunk_rel, c) < a.num_rel) ++c;
            continue;
        }
        const bool has = c < c1 && ldc(a.chunk_rel, c) == rel;
        if (!has) {
            if (is_root) store_rows<VEC>(a, nullptr, a.d_root, BASIS ? B : a.num_rel, r0, nrows);
            else if (!BASIS && a.d_weight) store_rows<VEC>(a, nullptr, a.d_weight + (size_t)rel * tab, rel, r0, nrows);
            continue;
        }
        zero_rows(G, T4 + a.d4);
        __syncthreads();
        for (; c < c1 && ldc(a.chunk_rel, c) == rel; ++c) {
            if (BASIS && !is_root && a.comp_slab != nullptr) {
                // d_comp[rel, b] partial of this chunk: sum over its slots of < w g[i], V_b[x_j] >
                auto value = [&](int src, float w, int rowl, int c4, long) -> f32x4 {
                    const f32x4 gv = w * *(const f32x4*)(a.g + (size_t)src * a.ldg + 4 * c4);
                    const long j = r0 + rowl;
                    const long row = a.x_index ? (long)a.x_index[j] : j;
                    if ((unsigned long)row < (unsigned long)a.in_rows)
                        for (int b = 0; b < B; ++b) {
                            const f32x4 vb = table_row<VEC>(a.weight + (size_t)b * tab, row, a.dout, c4);
                            cp[b * kFlLanes + lane] += (gv[0] * vb[0] + gv[1] * vb[1]) + (gv[2] * vb[2] + gv[3] * vb[3]);
                        }
                    return gv;
                };
                walk_chunk<L>(a, c, r0, G, value);
                __syncthreads();
                for (int b = lane; b < B; b += kFlLanes) {
                    float s = 0.f;
                    for (int k = 0; k < kFlLanes; ++k) {
                        s += cp[b * kFlLanes + k];
                        cp[b * kFlLanes + k] = 0.f;
                    }
                    a.comp_slab[(size_t)c * B + b] = s;
                }
                __syncthreads();
            } else {
                walk_chunk<L>(a, c, r0, G, gather_g);
            }
        }
        __syncthreads();
        if (is_root) {
            store_rows<VEC>(a, G, a.d_root, BASIS ? B : a.num_rel, r0, nrows);
        } else if (!BASIS) {
            if (a.d_weight) store_rows<VEC>(a, G, a.d_weight + (size_t)rel * tab, rel, r0, nrows);
        } else if (a.d_weight) {
            for (int i = lane; i < nrows * a.d4; i += kFlLanes) {
                const f32x4 gi = G[i];
                for (int b = 0; b < B; ++b) dV[b * T4 + i] += a.comp[(long)rel * B + b] * gi;
            }
        }
        __syncthreads();
    }
    if (BASIS && a.d_weight) {
        __syncthreads();
        for (int b = 0; b < B; ++b) store_rows<VEC>(a, dV + b * T4, a.d_weight + (size_t)b * tab, b, r0, nrows);
    }
}

// out[t][v] = sum of the workspace rows ws[t][idx[q]], q in [ptr[v], ptr[v + 1]), in index order; tables t < n_tab
template <bool VEC>
__global__ void __launch_bounds__(256) fl_index_reduce(const float* ws, long n_nodes, int d4, const int* ptr, const int* idx,
                                                       long in_rows, int dout, int n_tab, float* out, int first_blk) {
    const long total = (long)n_tab * in_rows * d4;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int c4 = (int)(e % d4);
        const long v = (e / d4) % in_rows;
        const int t = (int)(e / ((long)d4 * in_rows));
        const long blk = first_blk + t;
        const float* src = ws + (size_t)blk * n_nodes * (4 * d4) + 4 * c4;
        f32x4 s = zero4();
        for (int q = ptr[v]; q < ptr[v + 1]; ++q) s += *(const f32x4*)(src + (size_t)idx[q] * (4 * d4));
        float* o = out + (size_t)t * in_rows * dout;
        table_store<VEC>(o, v, dout, c4, s);
    }
}

__global__ void __launch_bounds__(256) fl_bias_reduce(const float* slab, int n_tiles, int d4, int dout, float* d_bias) {
    __shared__ float red[256];
    const int col = blockIdx.x;          // 0 .. 4 d4 - 1
    float s = 0.f;
    for (int t = threadIdx.x; t < n_tiles; t += 256) s += slab[(size_t)t * 4 * d4 + col];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0 && col < dout) d_bias[col] = red[0];
}

// d_comp[r, b]: the chunk partials of relation r in rel_order order (sorted by (relation, tile)); a chunk's first unit stands for it
__global__ void __launch_bounds__(256) fl_comp_reduce(const float* slab, const int* rel_order, int n_units, const int* chunk_rel,
                                                      int upc, int B, float* d_comp) {
    __shared__ float red[256];
    const int r = blockIdx.x / B, b = blockIdx.x % B;
    int lo = 0, hi = n_units;              // first unit of relation >= r
    while (lo < hi) {
        const int m = (lo + hi) / 2;
        if (chunk_rel[rel_order[m] / upc] < r) lo = m + 1; else hi = m;
    }
    int e = lo, hi2 = n_units;              // first unit of relation > r
    while (e < hi2) {
        const int m = (e + hi2) / 2;
        if (chunk_rel[rel_order[m] / upc] <= r) e = m + 1; else hi2 = m;
    }
    float s = 0.f;
    for (int p = lo + threadIdx.x; p < e; p += 256) {
        const int u = rel_order[p];
        if (u % upc == 0) s += slab[(size_t)(u / upc) * B + b];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) d_comp[(long)r * B + b] = red[0];
}

int lanes_per_slot(int d4) { return d4 <= 4 ? 4 : (d4 <= 8 ? 8 : (d4 <= 16 ? 16 : 32)); }

size_t fwd_lds(int tile, int d4) { return (size_t)(tile + 1) * d4 * 16; }
size_t bwd_lds(int tile, int d4, int B) { return (size_t)(tile + 1) * d4 * 16 + (size_t)B * tile * d4 * 16 + (size_t)B * kFlLanes * 4; }

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

int check_fl_plan(const rgcn_plan_t* p) {
    int st = check_plan(p);
    if (st != RGCN_OK) return st;
    // featureless kernels walk layout 0 only, and the whole node range (slot_row is then the node id)
    if (p->layout != 0 || p->n_owned != p->n_nodes) return RGCN_ERR_PLAN;
    return RGCN_OK;
}

FlArgs plan_args(const rgcn_plan_t* p) {
    FlArgs a;
    memset(&a, 0, sizeof(a));
    a.tile_ptr = p->tile_ptr;
    a.chunk_rel = p->chunk_rel;
    a.chunk_cnt = p->chunk_cnt;
    a.slot_src = p->slot_src;
    a.slot_w = p->slot_w;
    a.slot_row = p->slot_row;
    a.n_nodes = p->n_nodes;
    a.n_tiles = p->n_tiles;
    a.tile = p->tile;
    a.chunk = p->chunk;
    a.num_rel = p->num_relations;
    return a;
}

struct WsLayout {
    size_t bias, comp, rows, total;
};

WsLayout ws_layout(const rgcn_plan_t* p, int dout, int num_bases, int indexed) {
    const int d4 = (dout + 3) / 4;
    WsLayout w;
    w.bias = 0;
    w.comp = align256((size_t)p->n_tiles * d4 * 16);
    w.rows = w.comp + align256(num_bases > 0 ? (size_t)p->n_chunks * num_bases * 4 : 0);
    const size_t tabs = (size_t)(num_bases > 0 ? num_bases : p->num_relations) + 1;
    w.total = w.rows + align256(indexed ? tabs * (size_t)p->n_nodes * d4 * 16 : 0);
    return w;
}

#define FL_DISPATCH(KERN, L, VEC, BASIS, ...)                                                             \
    do {                                                                                               \
        auto launch = [&](auto kern) -> int {                                                          \
            hipError_t e = hipSuccess;                                                                 \
            if (lds > 64 * 1024) e = hipFuncSetAttribute((const void*)kern,                             \
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes); \
            if (e != hipSuccess) return (int)e;                                                        \
            hipLaunchKernelGGL(kern, dim3(a.n_tiles), dim3(64), lds, s, a);                            \
            return (int)hipGetLastError();                                                             \
        };                                                                                             \
        switch ((L) * 4 + ((VEC) ? 2 : 0) + ((BASIS) ? 1 : 0)) {                                       \
            case 16: return launch(KERN<4, false, false>);  case 17: return launch(KERN<4, false, true>);  \
            case 18: return launch(KERN<4, true, false>);   case 19: return launch(KERN<4, true, true>);   \
            case 32: return launch(KERN<8, false, false>);  case 33: return launch(KERN<8, false, true>);  \
            case 34: return launch(KERN<8, true, false>);   case 35: return launch(KERN<8, true, true>);   \
            case 64: return launch(KERN<16, false, false>); case 65: return launch(KERN<16, false, true>); \
            case 66: return launch(KERN<16, true, false>);  case 67: return launch(KERN<16, true, true>);  \
            case 128: return launch(KERN<32, false, false>); case 129: return launch(KERN<32, false, true>); \
            case 130: return launch(KERN<32, true, false>); default: return launch(KERN<32, true, true>);  \
        }                                                                                              \
    } while (0)

}  // namespace
}  // namespace rgcn

using namespace rgcn;

extern "C" int rgcn_featureless_geometry(int32_t n_nodes, int dout, int num_bases, int* tile, int* chunk) {
    if (!tile || !chunk) return RGCN_ERR_NULL;
    if (dout < 1 || dout > RGCN_MAX_WIDTH) return RGCN_ERR_WIDTH;
    if (n_nodes <= 0 || num_bases < 0) return RGCN_ERR_PLAN;
    const int d4 = (dout + 3) / 4;
    // about 4096 tiles (one wave each) where the graph has the nodes, never more than kFlMaxTile rows, and at most 20 KiB of
    // LDS per workgroup where 16 rows allow it (eight one-wave workgroups per CU at least)
    int t = (n_nodes / 4096) / 16 * 16;
    t = t < 16 ? 16 : (t > kFlMaxTile ? kFlMaxTile : t);
    while (t > 16 && bwd_lds(t, d4, num_bases) > 20 * 1024) t -= 16;
    if (bwd_lds(t, d4, num_bases) > (size_t)kLdsBytes) return RGCN_ERR_LDS;
    *tile = t;
    *chunk = 64;
    return RGCN_OK;
}

extern "C" int rgcn_featureless_fwd(const rgcn_plan_t* plan, const int64_t* x_index, int64_t in_rows, const float* weight,
                                    const float* comp, int num_bases, const float* root, const float* bias, float* out, int ldo,
                                    int dout, void* stream) {
    if (!plan || !weight || !out) return RGCN_ERR_NULL;
    if ((num_bases > 0) != (comp != nullptr) || num_bases < 0) return comp ? RGCN_ERR_PLAN : RGCN_ERR_NULL;
    if (dout < 1 || dout > RGCN_MAX_WIDTH) return RGCN_ERR_WIDTH;
    int st;
    if ((st = check_stride(ldo, dout)) != RGCN_OK) return st;
    if ((st = check_fl_plan(plan)) != RGCN_OK) return st;
    if (in_rows <= 0 || (!x_index && in_rows != plan->n_nodes)) return RGCN_ERR_PLAN;
    const int d4 = (dout + 3) / 4;
    const size_t lds = fwd_lds(plan->tile, d4);
    if (lds > (size_t)kLdsBytes) return RGCN_ERR_LDS;
    if ((st = check_device()) != RGCN_OK) return st;
    FlArgs a = plan_args(plan);
    a.x_index = x_index;
    a.weight = weight;
    a.comp = comp;
    a.root = root;
    a.num_bases = num_bases;
    a.in_rows = in_rows;
    a.dout = dout;
    a.d4 = d4;
    a.bias = bias;
    a.out = out;
    a.ldo = ldo;
    hipStream_t s = (hipStream_t)stream;
    FL_DISPATCH(fl_fwd_kernel, lanes_per_slot(d4), dout % 4 == 0, num_bases > 0);
}

extern "C" size_t rgcn_featureless_bwd_workspace_bytes(const rgcn_plan_t* plan_t, int dout, int num_bases, int indexed) {
    if (check_fl_plan(plan_t) != RGCN_OK || dout < 1 || dout > RGCN_MAX_WIDTH || num_bases < 0) return 0;
    return ws_layout(plan_t, dout, num_bases, indexed).total;
}

extern "C" int rgcn_featureless_bwd(const rgcn_plan_t* plan_t, const int64_t* x_index, const int32_t* inv_ptr,
                                    const int32_t* inv_idx, int64_t in_rows, const float* g, int ldg, int dout, const float* weight,
                                    const float* comp, int num_bases, void* workspace, size_t workspace_bytes, float* d_weight,
                                    float* d_comp, float* d_root, float* d_bias, void* stream) {
    if (!plan_t || !g || !workspace) return RGCN_ERR_NULL;
    if (num_bases < 0 || (num_bases > 0 && !comp)) return RGCN_ERR_NULL;
    if (d_comp && (num_bases == 0 || !weight)) return num_bases == 0 ? RGCN_ERR_PLAN : RGCN_ERR_NULL;
    if (x_index && (!inv_ptr || !inv_idx)) return RGCN_ERR_NULL;
    if (dout < 1 || dout > RGCN_MAX_WIDTH) return RGCN_ERR_WIDTH;
    int st;
    if ((st = check_stride(ldg, dout)) != RGCN_OK) return st;
    if ((st = check_fl_plan(plan_t)) != RGCN_OK) return st;
    if (in_rows <= 0 || (!x_index && in_rows != plan_t->n_nodes)) return RGCN_ERR_PLAN;
    const int d4 = (dout + 3) / 4;
    const WsLayout wl = ws_layout(plan_t, dout, num_bases, x_index != nullptr);
    if (workspace_bytes < wl.total) return RGCN_ERR_WORKSPACE;
    const size_t lds = num_bases > 0 ? bwd_lds(plan_t->tile, d4, num_bases) : fwd_lds(plan_t->tile, d4);
    if (lds > (size_t)kLdsBytes) return RGCN_ERR_LDS;
    if ((st = check_device()) != RGCN_OK) return st;
    if (!d_weight && !d_comp && !d_root && !d_bias) return RGCN_OK;
    char* ws = (char*)workspace;
    FlArgs a = plan_args(plan_t);
    a.x_index = x_index;
    a.weight = weight;
    a.comp = comp;
    a.num_bases = num_bases;
    a.in_rows = in_rows;
    a.dout = dout;
    a.d4 = d4;
    a.g = g;
    a.ldg = ldg;
    a.d_weight = d_weight;
    a.d_root = d_root;
    a.ws_rows = x_index ? (float*)(ws + wl.rows) : nullptr;
    a.comp_slab = d_comp ? (float*)(ws + wl.comp) : nullptr;
    a.bias_slab = d_bias ? (float*)(ws + wl.bias) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    auto walk = [&]() -> int {
        FL_DISPATCH(fl_bwd_kernel, lanes_per_slot(d4), dout % 4 == 0, num_bases > 0);
    };
    if ((st = walk()) != RGCN_OK) return st;
    const bool vec = dout % 4 == 0;
    // the per-node rows of an integer x, summed per table row through the inverted index of x
    if (x_index) {
        const int T = num_bases > 0 ? num_bases : plan_t->num_relations;
        auto reduce = [&](float* o, int n_tab, int first) -> int {
            const long total = (long)n_tab * in_rows * d4;
            const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 65536L);
            if (vec) hipLaunchKernelGGL(fl_index_reduce<true>, dim3(blocks), dim3(256), 0, s, a.ws_rows, (long)plan_t->n_nodes, d4,
                                        inv_ptr, inv_idx, (long)in_rows, dout, n_tab, o, first);
            else hipLaunchKernelGGL(fl_index_reduce<false>, dim3(blocks), dim3(256), 0, s, a.ws_rows, (long)plan_t->n_nodes, d4,
                                    inv_ptr, inv_idx, (long)in_rows, dout, n_tab, o, first);
            return (int)hipGetLastError();
        };
        if (d_weight && (st = reduce(d_weight, T, 0)) != RGCN_OK) return st;
        if (d_root && (st = reduce(d_root, 1, T)) != RGCN_OK) return st;
    }
    if (d_bias) {
        hipLaunchKernelGGL(fl_bias_reduce, dim3(4 * d4), dim3(256), 0, s, (const float*)(ws + wl.bias), plan_t->n_tiles, d4, dout,
                           d_bias);
        if ((st = (int)hipGetLastError()) != RGCN_OK) return st;
    }
    if (d_comp) {
        hipLaunchKernelGGL(fl_comp_reduce, dim3(plan_t->num_relations * num_bases), dim3(256), 0, s, (const float*)(ws + wl.comp),
                           plan_t->rel_order, plan_t->n_units, plan_t->chunk_rel, plan_t->chunk / 64, num_bases, d_comp);
        if ((st = (int)hipGetLastError()) != RGCN_OK) return st;
    }
    return RGCN_OK;
}

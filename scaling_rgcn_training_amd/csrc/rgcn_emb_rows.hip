// rgcn_emb_rows.hip -- a row-wise Adam step on the embedding rows a mini-batch gathered, behind the C ABI rgcn_emb_adam_rows of
// include/rgcn_mi355x.h: the optimizer's traffic is what the batch read, not what the table holds.  gfx950 only.  DESIGN.md
// section 16 has the semantics.
//
// A table is `planes` planes of [num_nodes][ld] floats (1: an nn.Embedding weight; S: the attention model's [S, N, emb]), its two
// moments lie the same way, row_step [num_nodes] counts the steps of every row (shared by the planes).  For every node n that
// `nodes` lists:  g = the gradient rows of the positions that list n, added in ascending position order, + weight_decay p;
// t = ++row_step[n];  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps):
// torch's dense Adam on that row alone, with the row's own step count.  Rows that are not listed are neither read nor written.
//
//   assume_unique   one unit per position, no workspace: the caller promises distinct ids (a sampler's src_nodes)
//   otherwise       emb_keys_kernel: (id, position) pairs, ids out of range get the key num_nodes and sort behind every row;
//                   one stable sort by id on rgcn_sort_scan.h (as many key bits as num_nodes needs): equal ids lie together in
//                   ascending position; the unit at the head of a run of equal ids walks the run, the others exit.  Nothing is
//                   read back: the call stays asynchronous.
//   emb_adam_rows_kernel   a unit is G = ceil(width / 4) lanes of one wave (one 16-byte piece each), 64 / G units per wave (one
//                   unit of 64 lanes and several passes beyond 256 columns); the group's first lane advances row_step and hands
//                   t to the others.  Pieces that are not whole, and every piece when a stride or a base is not 16-byte aligned,
//                   go element by element.  1 - b^t = -expm1f(t ln b) with ln b from the host in double: a plain fp32
//                   1 - powf(b, t) loses four digits at b = 0.999, t = 1.
// Purely bandwidth bound: four reads and three writes of 16 bytes per lane.  Every row address is a 64-bit element offset on plain
// pointers (S = 3, N = 10M, emb = 64 is 1.9e9 elements: no buffer descriptor spans it).  An id outside [0, num_nodes) writes nothing
// and adds 1 to *bad_ids (integer atomic).  No float atomics: the same inputs give the same bits.
#include <math.h>
#include "rgcn_common.h"
#include "rgcn_sort_scan.h"

namespace rgcn_emb {

using namespace rgcn_sort_scan;
using rgcn::f32x4;

struct RowArgs {
    float* table;
    float* exp_avg;
    float* exp_avg_sq;
    int32_t* row_step;
    const int64_t* nodes;      // assume_unique: the id of every position
    const u64* keys;           // otherwise: the sorted ids (num_nodes: out of range) ...
    const u32* vals;           // ... and their positions
    const float* grad;
    int32_t* bad_ids;          // may be NULL
    int64_t plane_stride, grad_plane_stride;
    u64 n_rows;
    int planes, num_nodes, width, width4, ld, ldg;
    int group, rows_per_wave;  // lanes of a unit, units of a wave
    int vec;                   // 1: whole pieces move as 16 bytes
    float lr, beta1, beta2, eps, weight_decay;
    double ln_beta1, ln_beta2;
};

__global__ void emb_keys_kernel(const int64_t* __restrict__ nodes, u32 n, int num_nodes, u64* __restrict__ keys, u32* __restrict__ vals,
                                int32_t* __restrict__ bad_ids) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t id = nodes[i];
    const bool bad = id < 0 || id >= (int64_t)num_nodes;
    if (bad && bad_ids != nullptr) atomicAdd(bad_ids, 1);
    keys[i] = bad ? (u64)num_nodes : (u64)id;
    vals[i] = i;
}

// the moments of one element, or of four at once
template <class T>
__device__ __forceinline__ void adam_moments(const T& p, T& m, T& v, T g, const RowArgs& a) {
    g += a.weight_decay * p;
    m = a.beta1 * m + (1.f - a.beta1) * g;
    v = a.beta2 * v + (1.f - a.beta2) * (g * g);
}

// what leaves p; c1 / c2: 1 - beta^t
__device__ __forceinline__ float adam_step(float m, float v, const RowArgs& a, float c1, float c2) {
    return a.lr * (m / c1) / (sqrtf(v / c2) + a.eps);
}

template <bool UNIQUE>
__global__ void __launch_bounds__(256) emb_adam_rows_kernel(const RowArgs a) {
    const int lane = threadIdx.x & 63;
    const u64 wave = (u64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int sub = lane / a.group;
    if (sub >= a.rows_per_wave) return;
    const u64 unit = wave * (u64)a.rows_per_wave + (u64)sub;
    if (unit >= a.n_rows) return;
    const int piece0 = lane - sub * a.group;
    int64_t node;
    u64 run_end = unit + 1;
    if (UNIQUE) {
        node = a.nodes[unit];
        if (node < 0 || node >= (int64_t)a.num_nodes) {
            if (piece0 == 0 && a.bad_ids != nullptr) atomicAdd(a.bad_ids, 1);
            return;
        }
    } else {
        const u64 key = a.keys[unit];
        if (unit > 0 && a.keys[unit - 1] == key) return;      // not the head of its run
        if (key >= (u64)a.num_nodes) return;                  // the ids out of range (counted by emb_keys_kernel)
        node = (int64_t)key;
        while (run_end < a.n_rows && a.keys[run_end] == key) ++run_end;
    }
    // every lane left is one of a whole group: the group's first lane owns the row's step count
    int t = 0;
    if (piece0 == 0) {
        t = a.row_step[node] + 1;
        a.row_step[node] = t;
    }
    t = __shfl(t, sub * a.group);
    const float c1 = -expm1f((float)((double)t * a.ln_beta1)), c2 = -expm1f((float)((double)t * a.ln_beta2));
    auto position = [&](u64 j) -> u64 { return UNIQUE ? j : (u64)a.vals[j]; };
    for (int pl = 0; pl < a.planes; ++pl) {
        const int64_t off = (int64_t)pl * a.plane_stride + node * (int64_t)a.ld;
        float* pr = a.table + off;
        float* mr = a.exp_avg + off;
        float* vr = a.exp_avg_sq + off;
        const float* gp = a.grad + (int64_t)pl * a.grad_plane_stride;
        for (int piece = piece0; piece < a.width4; piece += a.group) {
            const int c0 = 4 * piece;
            if (a.vec && c0 + 4 <= a.width) {
                f32x4 g = *(const f32x4*)(gp + (int64_t)position(unit) * a.ldg + c0);
                for (u64 j = unit + 1; j < run_end; ++j) g += *(const f32x4*)(gp + (int64_t)position(j) * a.ldg + c0);
                f32x4 p = *(const f32x4*)(pr + c0), m = *(const f32x4*)(mr + c0), v = *(const f32x4*)(vr + c0);
                adam_moments(p, m, v, g, a);
#pragma unroll
                for (int c = 0; c < 4; ++c) p[c] -= adam_step(m[c], v[c], a, c1, c2);
                *(f32x4*)(pr + c0) = p;
                *(f32x4*)(mr + c0) = m;
                *(f32x4*)(vr + c0) = v;
            } else {
                const int c1e = c0 + 4 < a.width ? c0 + 4 : a.width;
                for (int c = c0; c < c1e; ++c) {
                    float g = gp[(int64_t)position(unit) * a.ldg + c];
                    for (u64 j = unit + 1; j < run_end; ++j) g += gp[(int64_t)position(j) * a.ldg + c];
                    float p = pr[c], m = mr[c], v = vr[c];
                    adam_moments(p, m, v, g, a);
                    p -= adam_step(m, v, a, c1, c2);
                    pr[c] = p;
                    mr[c] = m;
                    vr[c] = v;
                }
            }
        }
    }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace rgcn_emb

using namespace rgcn_emb;

extern "C" size_t rgcn_emb_adam_rows_workspace_bytes(int64_t n_rows, int32_t num_nodes) {
    if (n_rows <= 0 || num_nodes < 0 || (u64)n_rows > kMaxKeys) return 0;
    Arena ar(nullptr);
    take_sort_bufs(ar, (u64)n_rows);
    return ar.bytes();
}

extern "C" int rgcn_emb_adam_rows(float* table, float* exp_avg, float* exp_avg_sq, int32_t* row_step, int planes, int64_t plane_stride,
                                  int32_t num_nodes, int width, int ld, const int64_t* nodes, int64_t n_rows, const float* grad,
                                  int64_t grad_plane_stride, int ldg, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  int assume_unique, int32_t* bad_ids, void* workspace, size_t workspace_bytes, void* stream) {
    if (!table || !exp_avg || !exp_avg_sq || !row_step) return RGCN_ERR_NULL;
    if (n_rows > 0 && (!nodes || !grad)) return RGCN_ERR_NULL;
    if (planes < 1 || num_nodes < 0 || n_rows < 0 || plane_stride < 0 || grad_plane_stride < 0) return RGCN_ERR_ARG;
    if (width < 1 || width > ld || width > ldg) return RGCN_ERR_ARG;
    // (written so that a NaN is refused too)
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(lr >= 0.f) || !(weight_decay >= 0.f))
        return RGCN_ERR_ARG;
    if ((u64)n_rows > kMaxKeys) return RGCN_ERR_PLAN;
    if (n_rows == 0) return RGCN_OK;
    SortBufs sb{};
    if (!assume_unique) {
        Arena ar(workspace);
        sb = take_sort_bufs(ar, (u64)n_rows);
        if (workspace_bytes < ar.bytes()) return RGCN_ERR_WORKSPACE;
        if (!workspace) return RGCN_ERR_NULL;
    }
    int st = rgcn::check_device();
    if (st != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    RowArgs a;
    a.table = table;
    a.exp_avg = exp_avg;
    a.exp_avg_sq = exp_avg_sq;
    a.row_step = row_step;
    a.nodes = nodes;
    a.keys = nullptr;
    a.vals = nullptr;
    a.grad = grad;
    a.bad_ids = bad_ids;
    a.plane_stride = plane_stride;
    a.grad_plane_stride = grad_plane_stride;
    a.n_rows = (u64)n_rows;
    a.planes = planes;
    a.num_nodes = num_nodes;
    a.width = width;
    a.width4 = (width + 3) / 4;
    a.ld = ld;
    a.ldg = ldg;
    a.group = a.width4 < 64 ? a.width4 : 64;
    a.rows_per_wave = 64 / a.group;
    a.vec = (ld % 4 == 0 && ldg % 4 == 0 && aligned16(table) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(grad) &&
             (planes == 1 || (plane_stride % 4 == 0 && grad_plane_stride % 4 == 0)))
                ? 1
                : 0;
    a.lr = lr;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.eps = eps;
    a.weight_decay = weight_decay;
    a.ln_beta1 = log((double)beta1);      // (-inf at beta = 0: 1 - 0^t = 1)
    a.ln_beta2 = log((double)beta2);
    const u64 waves = (a.n_rows + (u64)a.rows_per_wave - 1) / (u64)a.rows_per_wave;
    const dim3 grid((unsigned)((waves + 3) / 4)), block(256);
    if (assume_unique) {
        hipLaunchKernelGGL(emb_adam_rows_kernel<true>, grid, block, 0, s, a);
    } else {
        const u32 n = (u32)n_rows;
        hipLaunchKernelGGL(emb_keys_kernel, dim3(grid_for(n)), dim3(256), 0, s, nodes, n, (int)num_nodes, sb.k[0], sb.v[0], bad_ids);
        const int c = radix_sort_pairs(sb, n, bits_for((u64)num_nodes), s);
        a.keys = sb.k[c];
        a.vals = sb.v[c];
        hipLaunchKernelGGL(emb_adam_rows_kernel<false>, grid, block, 0, s, a);
    }
    return (int)hipGetLastError();
}

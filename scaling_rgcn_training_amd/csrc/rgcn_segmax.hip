// rgcn_segmax.hip -- max aggregation of the R-GCN layer (RGCNConv(aggr="max")) for gfx950: the entry points
// rgcn_segment_max / rgcn_segment_max_bwd of include/rgcn_mi355x.h.
//
// PyG 2.3.1 aggregates x before the transform: H_r[i] = max over the edges e into i of relation r of x[src_e] (torch
// scatter_reduce "amax", include_self = False), out[i] = sum_r H_r[i] W_r + x[i] root + bias.  Here (scaling_rgcn_training_amd/
// eplan.py MaxPlan) every (destination, relation) segment is a heavy segment of the edge-parallel plan:
//   rgcn_segment_max_kernel      H[seg][c] = max of in[row][c] over the rows of the segment, and T[seg][c] = the sum of the
//                                rows' tie weights (their multiplicities) over the rows that attain it: G lanes per segment,
//                                one 16-byte piece each, rows combined in index order.  Long segments go through levels
//                                exactly as rgcn_ep_segment_sum's: a level's (max, T) pairs combine as the larger max, or the
//                                sum of T for equal maxima -- T holds small integers, which fp32 adds exactly, so H and T do
//                                not depend on the cut.  The pseudo rows of the segments then go through rgcn_ep_transform.
//   rgcn_segment_max_bwd_kernel  C[q][c] = [x[src_q][c] == H[seg_q][c]] * w_q * dH[seg_q][c] / N[seg_q][c] for every segment
//                                row q, N = T + [H == 0]: the gradient of a max split evenly among the rows that attain it as
//                                torch's amax backward splits it -- with include_self = False torch still counts the zero its
//                                output starts from as one more tie when the max is exactly 0 (PyG 2.3.1 inherits that), so
//                                N = T + 1 there.  One row per lane group, no ownership; rgcn_ep_segment_sum adds C per source.
// Bytes per segment row: 16 (indices, weight) + width * 4 gathered in the forward; + 3 width * 4 read and width * 4 written in
// the backward.  No atomics, no LDS; rows are addressed with 64-bit offsets (any number of rows).
#include "rgcn_kernels_shared.h"
#include "rgcn_launch.h"

namespace rgcn {

struct SegMaxArgs {
    const float* in;
    const float* in_t;       // tie weights of the rows (the T of the level before), or NULL: seg_w[q] (1 without seg_w)
    const int* seg_ptr;
    const int* seg_idx;
    const float* seg_w;
    float* out;
    float* out_t;            // NULL: T is not written
    int ldin, ldo, width, width4, n_out;
};

// (m, t) <- (m, t) combined with (v, w): a larger value (or a NaN, which then stays: torch's amax propagates it) replaces the
// max and its tie weight, an equal one (-0 == +0 included) adds its weight
__device__ __forceinline__ void max_step(f32x4& m, f32x4& t, const f32x4 v, const f32x4 w) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (v[c] > m[c] || v[c] != v[c]) {
            m[c] = v[c];
            t[c] = w[c];
        } else if (v[c] == m[c]) {
            t[c] += w[c];
        }
    }
}

template <int G>
__global__ void __launch_bounds__(256) rgcn_segment_max_kernel(const SegMaxArgs a) {
    constexpr int SPW = 64 / G;                 // segments per wave
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long seg = wave * SPW + lane / G;
    const int piece = lane % G;
    if (seg >= a.n_out || piece >= a.width4) return;      // pieces beyond round4(width): nothing to read or write
    const int q0 = a.seg_ptr[seg], q1 = a.seg_ptr[seg + 1];
    auto off = [&](int q) { return (size_t)(a.seg_idx ? a.seg_idx[q] : q) * a.ldin + 4 * piece; };
    auto tie = [&](int q, size_t o) -> f32x4 {
        const float sw = a.seg_w ? a.seg_w[q] : 1.f;
        if (a.in_t == nullptr) return f32x4{sw, sw, sw, sw};
        return *(const f32x4*)(a.in_t + o) * sw;
    };
    f32x4 m = {0.f, 0.f, 0.f, 0.f}, t = m;        // an empty segment: H = 0 (PyG's zero fill), T = 0
    int q = q0;
    if (q < q1) {
        const size_t o = off(q);
        m = *(const f32x4*)(a.in + o);
        t = tie(q, o);
        ++q;
    }
    // four rows in flight; they are combined one after the other in index order
    for (; q + 4 <= q1; q += 4) {
        const size_t o0 = off(q), o1 = off(q + 1), o2 = off(q + 2), o3 = off(q + 3);
        const f32x4 v0 = *(const f32x4*)(a.in + o0), v1 = *(const f32x4*)(a.in + o1), v2 = *(const f32x4*)(a.in + o2),
                    v3 = *(const f32x4*)(a.in + o3);
        const f32x4 w0 = tie(q, o0), w1 = tie(q + 1, o1), w2 = tie(q + 2, o2), w3 = tie(q + 3, o3);
        max_step(m, t, v0, w0);
        max_step(m, t, v1, w1);
        max_step(m, t, v2, w2);
        max_step(m, t, v3, w3);
    }
    for (; q < q1; ++q) {
        const size_t o = off(q);
        max_step(m, t, *(const f32x4*)(a.in + o), tie(q, o));
    }
    const size_t oo = (size_t)seg * a.ldo + 4 * piece;
    *(f32x4*)(a.out + oo) = m;
    if (a.out_t != nullptr) {
        // the pad columns [width, round4(width)) hold +0.0 as every output's do (x's pad columns are zeros that all tie: their
        // count is not part of T)
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (4 * piece + c >= a.width) t[c] = 0.f;
        *(f32x4*)(a.out_t + oo) = t;
    }
}

struct SegMaxBwdArgs {
    const float* x;
    const float* h;
    const float* t;
    const float* dh;
    const int* row_src;
    const int* row_seg;
    const int* seg_dh;       // row of dH of every segment, or NULL: the segment id itself
    const float* row_w;      // NULL: 1
    float* c;
    long n_rows;
    int ldx, ldh, lddh, ldc, width4;
};

template <int G>
__global__ void __launch_bounds__(256) rgcn_segment_max_bwd_kernel(const SegMaxBwdArgs a) {
    constexpr int RPW = 64 / G;                 // rows per wave
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long q = wave * RPW + lane / G;
    const int piece = lane % G;
    if (q >= a.n_rows || piece >= a.width4) return;
    const int src = a.row_src[q], seg = a.row_seg[q];
    const int d = a.seg_dh ? a.seg_dh[seg] : seg;
    const float w = a.row_w ? a.row_w[q] : 1.f;
    const f32x4 xv = *(const f32x4*)(a.x + (size_t)src * a.ldx + 4 * piece);
    const size_t oh = (size_t)seg * a.ldh + 4 * piece;
    const f32x4 hv = *(const f32x4*)(a.h + oh), tv = *(const f32x4*)(a.t + oh);
    const f32x4 dv = *(const f32x4*)(a.dh + (size_t)d * a.lddh + 4 * piece);
    f32x4 r;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float n = tv[c] + (hv[c] == 0.f ? 1.f : 0.f);        // torch counts its zero-filled start when the max is 0
        r[c] = (xv[c] == hv[c] && n != 0.f) ? w * dv[c] / n : 0.f;
    }
    *(f32x4*)(a.c + (size_t)q * a.ldc + 4 * piece) = r;
}

}  // namespace rgcn

using namespace rgcn;

extern "C" int rgcn_segment_max(const float* in, const float* in_t, int ldin, const int32_t* seg_ptr, const int32_t* seg_idx,
                                const float* seg_w, int n_out, int width, float* out, float* out_t, int ldo, void* stream) {
    if (!in || !seg_ptr || !out) return RGCN_ERR_NULL;
    if (n_out < 0) return RGCN_ERR_PLAN;
    int st;
    if ((st = check_stride(ldin, width)) != RGCN_OK) return st;
    if ((st = check_stride(ldo, width)) != RGCN_OK) return st;
    if ((st = check_device()) != RGCN_OK) return st;
    if (n_out == 0) return RGCN_OK;
    SegMaxArgs a;
    a.in = in;
    a.in_t = in_t;
    a.seg_ptr = seg_ptr;
    a.seg_idx = seg_idx;
    a.seg_w = seg_w;
    a.out = out;
    a.out_t = out_t;
    a.ldin = ldin;
    a.ldo = ldo;
    a.width = width;
    a.width4 = (width + 3) / 4;
    a.n_out = n_out;
    hipStream_t s = (hipStream_t)stream;
    return launch_row_groups(a.width4, n_out, [&](auto g, dim3 grid) {
        hipLaunchKernelGGL(rgcn_segment_max_kernel<decltype(g)::value>, grid, dim3(256), 0, s, a);
        return (int)hipGetLastError();
    });
}

extern "C" int rgcn_segment_max_bwd(const float* x, int ldx, const float* h, const float* t, int ldh, const float* dh, int lddh,
                                    const int32_t* row_src, const int32_t* row_seg, const int32_t* seg_dh, const float* row_w,
                                    int64_t n_rows, int width, float* c, int ldc, void* stream) {
    if (!x || !h || !t || !dh || !row_src || !row_seg || !c) return RGCN_ERR_NULL;
    if (n_rows < 0 || n_rows > INT32_MAX) return RGCN_ERR_PLAN;     // (C rows are addressed by int32 segment indices)
    int st;
    if ((st = check_stride(ldx, width)) != RGCN_OK) return st;
    if ((st = check_stride(ldh, width)) != RGCN_OK) return st;
    if ((st = check_stride(lddh, width)) != RGCN_OK) return st;
    if ((st = check_stride(ldc, width)) != RGCN_OK) return st;
    if ((st = check_device()) != RGCN_OK) return st;
    if (n_rows == 0) return RGCN_OK;
    SegMaxBwdArgs a;
    a.x = x;
    a.h = h;
    a.t = t;
    a.dh = dh;
    a.row_src = row_src;
    a.row_seg = row_seg;
    a.seg_dh = seg_dh;
    a.row_w = row_w;
    a.c = c;
    a.n_rows = (long)n_rows;
    a.ldx = ldx;
    a.ldh = ldh;
    a.lddh = lddh;
    a.ldc = ldc;
    a.width4 = (width + 3) / 4;
    hipStream_t s = (hipStream_t)stream;
    return launch_row_groups(a.width4, a.n_rows, [&](auto g, dim3 grid) {
        hipLaunchKernelGGL(rgcn_segment_max_bwd_kernel<decltype(g)::value>, grid, dim3(256), 0, s, a);
        return (int)hipGetLastError();
    });
}

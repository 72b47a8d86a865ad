// rgcn_rows.hip -- the root term of a BIPARTITE R-GCN layer for gfx950 (MI355X), plan-free: the rows of x_dst pair up one to
// one with the rows of the output, so `x_dst @ root` and its gradient towards x_dst are dense products over rows with one small
// matrix (PyG 2.3.1 rgcn_conv.py: `out = out + x_r @ root` with x = (x_l, x_r)).
//   rgcn_rows_transform : y = add + x @ W + bias   (forward: W = root; d_x_dst = g @ root^T: W = root^T, read from root itself)
// (d_root = x_dst^T g is rgcn_rows_dw, on the streaming kernel of rgcn_dw_root.hip.)
// Exact fp32 (v_mfma_f32_16x16x4_f32), no atomics, fixed summation orders: bit-reproducible.
#include "rgcn_common.h"
#include "rgcn_launch.h"

namespace rgcn {

// ------------------------------------------------------------------------------------------------
// y[i, :] = add[i, :] + x[i, :] @ W + bias
// ------------------------------------------------------------------------------------------------
// W (at most 128 x 128) sits in LDS, zero padded to multiples of 16 per side, rows 4 floats longer than the padded width so
// that the four k-quarters of a wave read four different bank groups.  A wave owns 16 rows at a time and computes y^T = W^T x^T:
// the MFMA's M index is the output column, its N index the row, so lane (row, kq) ends up with FOUR CONSECUTIVE columns
// 16 nt + 4 kq + r of its row -- one 16-byte load of `add` and one 16-byte store of y per lane and 16-column tile.  The k index
// of an MFMA step is permuted (a sum does not care): lane (row, kq) loads x[row][16 c + 4 kq .. + 3] with one 16-byte load and
// feeds element j to step (c, j), whose W operand is row 16 c + 4 kq + j of the LDS image.
// Persistent workgroups of 8 waves, two per CU; up to 64 gathered columns the x rows of the next tile are loaded before the
// current one is multiplied (at 128 the second set of fragments would not fit 128 VGPRs: four waves per SIMD hide the load).
constexpr int kRowsTfThreads = 512;
constexpr int kRowsTfWaves = kRowsTfThreads / 64;
constexpr int kRowsTfMaxBlocks = 512;            // two workgroups per CU

struct RowsTfArgs {
    const float* x;
    const float* w;
    const float* add;      // may alias y: a lane reads exactly the 16 bytes it stores later
    const float* bias;
    float* y;
    long rows;
    int ldx, lda, ldy, din, dout, transpose;
    int k16, n16;          // 16-wide pieces of din / dout
    int ldw;               // floats per row of the LDS image: 16 n16 + 4
};

template <int KT>
__global__ void __launch_bounds__(kRowsTfThreads, 4) rgcn_rows_transform_kernel(const RowsTfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // W [16 k16][ldw], then bias [16 n16]
    const int tid = threadIdx.x;
    const int krows = 16 * a.k16, ncols = 16 * a.n16;
    float* bias_l = lds + krows * a.ldw;
    if (!a.transpose) {
        for (int i = tid; i < krows * ncols; i += kRowsTfThreads) {
            const int k = i / ncols, n = i - k * ncols;
            lds[k * a.ldw + n] = (k < a.din && n < a.dout) ? a.w[(size_t)k * a.dout + n] : 0.f;
        }
    } else {                                     // w is [dout][din]: W[k][n] = w[n][k]
        for (int i = tid; i < krows * ncols; i += kRowsTfThreads) {
            const int n = i / krows, k = i - n * krows;
            lds[k * a.ldw + n] = (k < a.din && n < a.dout) ? a.w[(size_t)n * a.din + k] : 0.f;
        }
    }
    for (int n = tid; n < ncols; n += kRowsTfThreads) bias_l[n] = (a.bias != nullptr && n < a.dout) ? a.bias[n] : 0.f;
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int din4 = (a.din + 3) / 4 * 4, dout4 = (a.dout + 3) / 4 * 4;
    const long tiles = (a.rows + 15) / 16;
    const long step = (long)gridDim.x * kRowsTfWaves;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    f32x4 xa[KT], xn[KT];
    auto load_x = [&](f32x4(&dst)[KT], long tile) {
        const long row = tile * 16 + rl;
#pragma unroll
        for (int c = 0; c < KT; ++c) {
            const int col = 16 * c + 4 * kq;
            dst[c] = (row < a.rows && col < din4) ? *(const f32x4*)(a.x + (size_t)row * a.ldx + col) : zero;
        }
    };
    long t = (long)blockIdx.x * kRowsTfWaves + wave;
    load_x(xa, t);
    constexpr bool kAhead = KT <= 4;
    for (; t < tiles; t += step) {
        if (kAhead) load_x(xn, t + step);
        const long row = t * 16 + rl;
        for (int nt = 0; nt < a.n16; ++nt) {
            const int col = 16 * nt + 4 * kq;
            const bool mine = row < a.rows && col < dout4;
            f32x4 acc = zero;
            if (a.add != nullptr && mine) acc = *(const f32x4*)(a.add + (size_t)row * a.lda + col);
            const float* wl = lds + (4 * kq) * a.ldw + 16 * nt + rl;
#pragma unroll
            for (int c = 0; c < KT; ++c) {
                if (c < a.k16) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wl[(16 * c + j) * a.ldw], xa[c][j], acc, 0, 0, 0);
                }
            }
            if (mine) {
                acc += *(const f32x4*)(bias_l + col);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (col + e >= a.dout) acc[e] = 0.f;             // the pad columns of y: +0.0
                *(f32x4*)(a.y + (size_t)row * a.ldy + col) = acc;
            }
        }
        if (kAhead) {
#pragma unroll
            for (int c = 0; c < KT; ++c) xa[c] = xn[c];
        } else {
            load_x(xa, t + step);
        }
    }
}

}  // namespace rgcn

using namespace rgcn;

extern "C" int rgcn_rows_transform(const float* x, int ldx, int din, const float* w, int transpose, const float* add, int lda,
                                   const float* bias, float* y, int ldy, int dout, long rows, void* stream) {
    int st;
    if (!x || !w || !y) return RGCN_ERR_NULL;
    if ((st = check_stride(ldx, din)) != RGCN_OK) return st;
    if ((st = check_stride(ldy, dout)) != RGCN_OK) return st;
    if (add != nullptr && (st = check_stride(lda, dout)) != RGCN_OK) return st;
    if (rows < 0) return RGCN_ERR_PLAN;
    if (rows == 0) return RGCN_OK;
    if ((st = check_device()) != RGCN_OK) return st;
    RowsTfArgs a;
    a.x = x;
    a.w = w;
    a.add = add;
    a.bias = bias;
    a.y = y;
    a.rows = rows;
    a.ldx = ldx;
    a.lda = lda;
    a.ldy = ldy;
    a.din = din;
    a.dout = dout;
    a.transpose = transpose != 0;
    a.k16 = (din + 15) / 16;
    a.n16 = (dout + 15) / 16;
    a.ldw = 16 * a.n16 + 4;
    const size_t lds = sizeof(float) * ((size_t)16 * a.k16 * a.ldw + 16 * a.n16);
    const long tiles = (rows + 15) / 16;
    const long want = (tiles + kRowsTfWaves - 1) / kRowsTfWaves;
    const int blocks = (int)(want > kRowsTfMaxBlocks ? kRowsTfMaxBlocks : want);
    hipStream_t s = (hipStream_t)stream;
    auto launch = [&](auto kern) -> int {
        hipError_t e = hipSuccess;
        if (lds > 64 * 1024) e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(kRowsTfThreads), lds, s, a);
        return (int)hipGetLastError();
    };
    return for_padded_width(padded_width(din), [&](auto kp) { return launch(rgcn_rows_transform_kernel<decltype(kp)::value / 16>); });
}

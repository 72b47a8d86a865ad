// rgcn_rows.hip -- the root term of a BIPARTITE R-GCN layer for gfx950 (MI355X), plan-free: the rows of x_dst pair up one to
// one with the rows of the output, so `x_dst @ root` and its two gradients are dense products over rows with one small matrix
// (PyG 2.3.1 rgcn_conv.py: `out = out + x_r @ root` with x = (x_l, x_r)).
//   rgcn_rows_transform : y = add + x @ W + bias   (forward: W = root; d_x_dst = g @ root^T: W = root^T, read from root itself)
//   rgcn_rows_dw        : d_w = x^T g              (d_root)
// Exact fp32 (v_mfma_f32_16x16x4_f32), no atomics, fixed summation orders: bit-reproducible.
#include "rgcn_common.h"

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

// ------------------------------------------------------------------------------------------------
// d_w [din, dout] = x^T g
// ------------------------------------------------------------------------------------------------
// rgcn_dw_root_kernel's streaming product (both operands straight from memory in MFMA layout, no LDS: a k-step is 4 rows, lane
// (ml, kq) loads 16 bytes of x[row + kq] and 16 of g[row + kq]) with the output split over waves: one wave holds a 64 x 64
// accumulator in 64 VGPRs, so a product of up to 128 x 128 is cut into qi x qj quadrants of 64 x 64 and a wave takes ONE quadrant
// of ONE row range -- the quadrants of a range are neighbouring waves of one workgroup, which read the same rows together.  Every
// wave writes one slab; rgcn_rows_dw_reduce_kernel sums the slabs of a quadrant in range order (fixed: bit-reproducible).
constexpr int kRowsDwBatch = 8;                  // k-steps per register batch (two batches in flight)
constexpr int kRowsDwMaxWaves = 2048;            // two waves per SIMD of the chip
constexpr int kRowsDwSlabFloats = 64 * 64;

struct RowsDwArgs {
    const float* x;
    const float* g;
    float* slabs;          // [parts][qi * qj][64 * 64]
    long rows;
    int ldx, ldg, din4, dout4;     // (widths in 16-byte pieces)
    int parts, qi, qj;
};

__global__ void __launch_bounds__(256, 2) rgcn_rows_dw_kernel(const RowsDwArgs a) {
    constexpr int B = kRowsDwBatch;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));     // wave-uniform
    const int nq = a.qi * a.qj;
    if (w >= a.parts * nq) return;
    const int p = w / nq, q = w - p * nq;
    const int wi = q / a.qj, wj = q - wi * a.qj;
    const int ml = lane & 15, kq = lane >> 4;
    const long ksteps = (a.rows + 3) / 4;
    const long k0 = ksteps * p / a.parts, k1 = ksteps * (p + 1) / a.parts;
    // the wave's rows of its two column halves through buffer descriptors (base = first row of the range at the quadrant's first
    // column, num_records = bytes from there to the end of the range): a k-step past the range, a row past the matrix and a
    // 16-byte piece beyond the width read zeros from the hardware range check
    const long r0 = 4 * k0;
    long rcnt = (4 * k1 < a.rows ? 4 * k1 : a.rows) - r0;
    if (rcnt < 0) rcnt = 0;
    const long xrec = rcnt * a.ldx - 64 * wi, grec = rcnt * a.ldg - 64 * wj;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(a.x + (size_t)r0 * a.ldx + 64 * wi, xrec > 0 ? (unsigned)(xrec * 4) : 0u);
    const __amdgpu_buffer_rsrc_t rg = make_rsrc(a.g + (size_t)r0 * a.ldg + 64 * wj, grec > 0 ? (unsigned)(grec * 4) : 0u);
    const bool xin = 16 * wi + ml < a.din4, gin = 16 * wj + ml < a.dout4;
    const unsigned xstep = xin ? 16u * (unsigned)a.ldx : 0u, gstep = gin ? 16u * (unsigned)a.ldg : 0u;
    unsigned xo = xin ? (unsigned)(kq * a.ldx + 4 * ml) * 4u : 0xFFFFFFF0u;
    unsigned go = gin ? (unsigned)(kq * a.ldg + 4 * ml) * 4u : 0xFFFFFFF0u;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    f32x4 acc[4][4];
#pragma unroll
    for (int ia = 0; ia < 4; ++ia)
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) acc[ia][jb] = zero;

    f32x4 xa[2][B], ga[2][B];
    auto load_batch = [&](int buf) {
#pragma unroll
        for (int s = 0; s < B; ++s) {
            xa[buf][s] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, (int)xo, 0, 0));
            ga[buf][s] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rg, (int)go, 0, 0));
            xo += xstep;
            go += gstep;
        }
    };
    auto compute_batch = [&](int buf) {
#pragma unroll
        for (int s = 0; s < B; ++s)
#pragma unroll
            for (int ia = 0; ia < 4; ++ia)
#pragma unroll
                for (int jb = 0; jb < 4; ++jb)
                    acc[ia][jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[buf][s][ia], ga[buf][s][jb], acc[ia][jb], 0, 0, 0);
    };
    load_batch(0);
    for (long k = k0; k < k1; k += 2 * B) {
        load_batch(1);
        compute_batch(0);
        load_batch(0);
        compute_batch(1);
    }
    // D of v_mfma_f32_16x16x4_f32: lane (ml, kq) holds D[m = 4 kq + r][n = ml]; m stands for x column 4 m + ia of the quadrant,
    // n for g column 4 ml + jb
    float* slab = a.slabs + (size_t)w * kRowsDwSlabFloats;
#pragma unroll
    for (int ia = 0; ia < 4; ++ia)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            f32x4 v;
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) v[jb] = acc[ia][jb][r];
            *(f32x4*)(slab + (4 * (4 * kq + r) + ia) * 64 + 4 * ml) = v;
        }
}

// d_w[k][n] = sum over the row ranges' slabs of the quadrant that holds (k, n): 16 strided partial sums (range s, s + 16, ...)
// folded in order s = 0..15.  grid = (din, qj) workgroups x 1024 threads; no range at all (rows = 0) writes zeros.
__global__ void __launch_bounds__(1024) rgcn_rows_dw_reduce_kernel(const float* __restrict__ slabs, int parts, int qi, int qj,
                                                                   int din, int dout, float* __restrict__ d_w) {
    __shared__ float part[16][64];
    const int n = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int k = blockIdx.x, bj = blockIdx.y;
    const int nq = qi * qj, q = (k >> 6) * qj + bj;
    float sum = 0.f;
    for (int p = s; p < parts; p += 16) sum += slabs[((size_t)p * nq + q) * kRowsDwSlabFloats + (k & 63) * 64 + n];
    part[s][n] = sum;
    __syncthreads();
    if (s != 0 || 64 * bj + n >= dout) return;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += part[i][n];
    d_w[(size_t)k * dout + 64 * bj + n] = t;
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
    switch (padded_width(din)) {
        case 16: return launch(rgcn_rows_transform_kernel<1>);
        case 32: return launch(rgcn_rows_transform_kernel<2>);
        case 64: return launch(rgcn_rows_transform_kernel<4>);
        default: return launch(rgcn_rows_transform_kernel<8>);
    }
}

extern "C" size_t rgcn_rows_dw_workspace_bytes(int din, int dout) {
    if (din < 1 || din > RGCN_MAX_WIDTH || dout < 1 || dout > RGCN_MAX_WIDTH) return 0;
    return sizeof(float) * (size_t)kRowsDwMaxWaves * kRowsDwSlabFloats;
}

extern "C" int rgcn_rows_dw(const float* x, int ldx, int din, const float* g, int ldg, int dout, long rows, void* workspace,
                            size_t workspace_bytes, float* d_w, void* stream) {
    int st;
    if (!workspace || !d_w || (rows != 0 && (!x || !g))) return RGCN_ERR_NULL;      // (no rows: x and g are not read)
    if ((st = check_stride(ldx, din)) != RGCN_OK) return st;
    if ((st = check_stride(ldg, dout)) != RGCN_OK) return st;
    if (rows < 0) return RGCN_ERR_PLAN;
    if (workspace_bytes < rgcn_rows_dw_workspace_bytes(din, dout)) return RGCN_ERR_WORKSPACE;
    RowsDwArgs a;
    a.x = x;
    a.g = g;
    a.slabs = (float*)workspace;
    a.rows = rows;
    a.ldx = ldx;
    a.ldg = ldg;
    a.din4 = (din + 3) / 4;
    a.dout4 = (dout + 3) / 4;
    a.qi = (din + 63) / 64;
    a.qj = (dout + 63) / 64;
    const int nq = a.qi * a.qj;
    const long ksteps = (rows + 3) / 4;
    const long want = (ksteps + 2 * kRowsDwBatch - 1) / (2 * kRowsDwBatch);      // at least one double batch per range
    a.parts = (int)(want > kRowsDwMaxWaves / nq ? kRowsDwMaxWaves / nq : want);
    if (a.parts > 0) {
        // a wave addresses its row range (and the batches it loads past the end of it) through 32-bit buffer offsets, below the
        // out-of-range marker at the top of that range
        const long rows_per_wave = 4 * ((ksteps + a.parts - 1) / a.parts + 1 + 3 * kRowsDwBatch);
        if ((unsigned long long)rows_per_wave * (unsigned long long)(ldx > ldg ? ldx : ldg) * 4ull >= 0xFFFFFF00ull) return RGCN_ERR_STRIDE;
    }
    if ((st = check_device()) != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    if (a.parts > 0) {
        hipLaunchKernelGGL(rgcn_rows_dw_kernel, dim3((a.parts * nq + 3) / 4), dim3(256), 0, s, a);
        if ((st = (int)hipGetLastError()) != 0) return st;
    }
    hipLaunchKernelGGL(rgcn_rows_dw_reduce_kernel, dim3(din, a.qj), dim3(1024), 0, s, a.slabs, a.parts, a.qi, a.qj, din, dout, d_w);
    return (int)hipGetLastError();
}

// rgcn_dw_root.hip -- the root part of the R-GCN weight gradients for gfx950 (MI355X), plan-free: d_root = X^T G and
// d_bias = sum of the rows of G, one streaming kernel behind two entry points.
//   rgcn_bwd_dw_root : d_root and d_bias of a layer whose root rows are its own nodes, widths up to 64.  Replaces what autograd
//                      computes for RGCNConv's `root` / `bias` at /root/reference/model/modelTrainer.py:66 (the layer's
//                      `x @ root + bias` term: PyG 2.3.1 rgcn_conv.py, called from model/layers.py:21,23).
//   rgcn_rows_dw     : d_w = x^T g, widths up to 128: d_root of a BIPARTITE layer (`out = out + x_r @ root` with x = (x_l, x_r);
//                      the forward product and d_x_dst are rgcn_rows_transform, rgcn_rows.hip).
// Exact fp32 (v_mfma_f32_16x16x4_f32), no atomics, fixed summation orders: bit-reproducible.
#include "rgcn_common.h"

namespace rgcn {

// ------------------------------------------------------------------------------------------------
// d_w = X^T G (and the column sums of G) -- a dense [in x rows] x [rows x out] product
// ------------------------------------------------------------------------------------------------
// The "gathered" rows of the self-loop relation are the node's own: no indices, no plan.  A wave streams a contiguous
// range of rows (one MFMA k-step = 4 rows: lane (ml, kq) loads 16 bytes of x[row + kq] and 16 of g[row + kq], 1 KiB
// coalesced per instruction), two batches of kDwRootBatch k-steps in registers, 16 MFMAs per k-step into a 64 x 64
// accumulator in 64 VGPRs (the output tiles are strided column sets, as in rgcn_dw_direct_kernel), and writes ONE slab;
// rgcn_dw_root_reduce_kernel sums the slabs in range order (bit-reproducible).  No LDS and few enough registers that its
// workgroups fit a CU NEXT TO a workgroup of rgcn_tile_kernel: 5 GB of streaming reads and a tenth of a launch's MFMAs,
// which the host runs on a side stream under the MFMA-bound dX launch instead of after it.
//   BIAS = true  (rgcn_bwd_dw_root): one 64 x 64 output, wave w is range w; it also sums its rows of g, and the slab holds
//                the four row-quarters' sums behind the accumulator.
//   BIAS = false (rgcn_rows_dw): a product of up to 128 x 128 is cut into qi x qj quadrants of 64 x 64 and a wave takes ONE
//                quadrant of ONE range -- the quadrants of a range are neighbouring waves of one workgroup, which read the
//                same rows together.
constexpr int kDwRootBatch = 8;                  // k-steps per register batch (two batches in flight)
constexpr int kRootMaxWaves = 1024;              // rgcn_bwd_dw_root: one wave per SIMD of the chip
constexpr int kRowsDwMaxWaves = 2048;            // rgcn_rows_dw: two
constexpr int kDwRootSlabFloats = 64 * 64;       // the accumulator; the four bias sums of 64 floats follow it under BIAS
constexpr int dw_root_slab_floats(bool bias) { return kDwRootSlabFloats + (bias ? 4 * 64 : 0); }

struct DwRootArgs {
    const float* x;
    const float* g;
    float* slabs;          // [parts][qi * qj][dw_root_slab_floats(BIAS)]
    long rows;
    int ldx, ldg, din4, dout4;     // (widths in 16-byte pieces)
    int parts, qi, qj;             // row ranges, quadrants per side (BIAS: 1 x 1)
};

template <bool BIAS>
__global__ void __launch_bounds__(256, 2) rgcn_dw_root_kernel(const DwRootArgs a) {
    constexpr int B = kDwRootBatch;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));     // wave-uniform (scalar registers)
    const int nq = BIAS ? 1 : a.qi * a.qj;
    if (w >= a.parts * nq) return;
    const int p = w / nq, q = w - p * nq;
    const int wi = BIAS ? 0 : q / a.qj, wj = BIAS ? 0 : q - wi * a.qj;
    const int ml = lane & 15, kq = lane >> 4;
    const long ksteps = (a.rows + 3) / 4;
    const long k0 = ksteps * p / a.parts, k1 = ksteps * (p + 1) / a.parts;
    // Each wave addresses ITS rows through two buffer descriptors (base = first row of the range at the quadrant's first
    // column, num_records = bytes from there to the end of the range): a k-step past the end of the range, a row past the end
    // of the matrix or a 16-byte column piece beyond the width is out of range and the hardware range check feeds zeros -- no
    // branch, no select.  Per load one v_add of the lane's running offset (a lane beyond the width keeps the out-of-range
    // marker: its step is 0).
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
    f32x4 bsum = zero;

    f32x4 xa[2][B], ga[2][B];
    auto load_batch = [&](int buf) {                 // the next B k-steps of the range
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
        for (int s = 0; s < B; ++s) {
            if (BIAS) bsum += ga[buf][s];
#pragma unroll
            for (int ia = 0; ia < 4; ++ia)
#pragma unroll
                for (int jb = 0; jb < 4; ++jb)
                    acc[ia][jb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[buf][s][ia], ga[buf][s][jb], acc[ia][jb], 0, 0, 0);
        }
    };
    load_batch(0);
    for (long k = k0; k < k1; k += 2 * B) {
        load_batch(1);
        compute_batch(0);
        load_batch(0);
        compute_batch(1);
    }
    // D layout of v_mfma_f32_16x16x4_f32: lane (ml, kq) holds D[m = 4 kq + r][n = ml]; m stands for x column 4 m + ia of the
    // quadrant, n for g column 4 ml + jb
    float* slab = a.slabs + (size_t)w * dw_root_slab_floats(BIAS);
#pragma unroll
    for (int ia = 0; ia < 4; ++ia)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            f32x4 v;
#pragma unroll
            for (int jb = 0; jb < 4; ++jb) v[jb] = acc[ia][jb][r];
            *(f32x4*)(slab + (4 * (4 * kq + r) + ia) * 64 + 4 * ml) = v;
        }
    if (BIAS) *(f32x4*)(slab + kDwRootSlabFloats + kq * 64 + 4 * ml) = bsum;
}

// d_w[k][n] = sum over the row ranges' slabs of the quadrant that holds (k, n); block row k = din (there when d_bias is asked
// for; BIAS slabs, one quadrant): d_bias[n] = sum over slabs and row quarters.  Fixed order: 16 strided partial sums (range
// s, s + 16, ...) folded in order s = 0..15.  grid = (din [+ 1], qj) workgroups x 1024 threads; no range at all writes zeros.
__global__ void __launch_bounds__(1024) rgcn_dw_root_reduce_kernel(const float* __restrict__ slabs, int parts, int nq, int qj,
                                                                   int slab_floats, int din, int dout, float* __restrict__ d_w,
                                                                   float* __restrict__ d_bias) {
    __shared__ float part[16][64];
    const int n = threadIdx.x & 63, s = threadIdx.x >> 6;
    const int k = blockIdx.x, bj = blockIdx.y;
    float sum = 0.f;
    if (k < din) {
        const int q = (k >> 6) * qj + bj;
        for (int p = s; p < parts; p += 16) sum += slabs[((size_t)p * nq + q) * slab_floats + (k & 63) * 64 + n];
    } else {
        for (int p = s; p < parts; p += 16) {
            const float* b = slabs + (size_t)p * slab_floats + kDwRootSlabFloats + n;
            sum += (b[0] + b[64]) + (b[128] + b[192]);
        }
    }
    part[s][n] = sum;
    __syncthreads();
    if (s != 0 || 64 * bj + n >= dout) return;
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += part[i][n];
    if (k < din) {
        if (d_w != nullptr) d_w[(size_t)k * dout + 64 * bj + n] = t;
    } else {
        d_bias[n] = t;
    }
}

// The launches behind both entry points, whose own argument checks have passed: `parts` row ranges, each a wave per quadrant.
template <bool BIAS>
int dw_root_launch(const float* x, int ldx, int din, const float* g, int ldg, int dout, long rows, int parts, void* workspace,
                   float* d_w, float* d_bias, void* stream) {
    int st;
    DwRootArgs a;
    a.x = x;
    a.g = g;
    a.slabs = (float*)workspace;
    a.rows = rows;
    a.ldx = ldx;
    a.ldg = ldg;
    a.din4 = (din + 3) / 4;
    a.dout4 = (dout + 3) / 4;
    a.parts = parts;
    a.qi = (din + 63) / 64;
    a.qj = (dout + 63) / 64;
    const int nq = a.qi * a.qj;
    if (parts > 0) {
        // a wave addresses its row range (and the batches it loads past the end of it) through 32-bit buffer offsets, below the
        // out-of-range marker at the top of that range
        const long ksteps = (rows + 3) / 4;
        const long rows_per_wave = 4 * ((ksteps + parts - 1) / parts + 1 + 3 * kDwRootBatch);
        if ((unsigned long long)rows_per_wave * (unsigned long long)(ldx > ldg ? ldx : ldg) * 4ull >= 0xFFFFFF00ull) return RGCN_ERR_STRIDE;
    }
    if ((st = check_device()) != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    if (parts > 0) {
        hipLaunchKernelGGL(rgcn_dw_root_kernel<BIAS>, dim3((parts * nq + 3) / 4), dim3(256), 0, s, a);
        if ((st = (int)hipGetLastError()) != 0) return st;
    }
    hipLaunchKernelGGL(rgcn_dw_root_reduce_kernel, dim3(din + (d_bias != nullptr ? 1 : 0), a.qj), dim3(1024), 0, s, a.slabs, parts,
                       nq, a.qj, dw_root_slab_floats(BIAS), din, dout, d_w, d_bias);
    return (int)hipGetLastError();
}

}  // namespace rgcn

using namespace rgcn;

extern "C" size_t rgcn_bwd_dw_root_workspace_bytes(void) { return sizeof(float) * (size_t)kRootMaxWaves * dw_root_slab_floats(true); }

// d_root = x^T g, d_bias = column sums of g over `rows` rows: the self-loop part of the weight gradients, plan-free
extern "C" int rgcn_bwd_dw_root(const float* x, int ldx, int din, const float* g, int ldg, int dout, long rows, void* workspace,
                                size_t workspace_bytes, float* d_root, float* d_bias, void* stream) {
    int st;
    if (!x || !g || !workspace) return RGCN_ERR_NULL;
    if (!d_root && !d_bias) return RGCN_ERR_NULL;
    if ((st = check_stride(ldx, din)) != RGCN_OK) return st;
    if ((st = check_stride(ldg, dout)) != RGCN_OK) return st;
    if (din > 64 || dout > 64) return RGCN_ERR_WIDTH;
    if (rows <= 0) return RGCN_ERR_PLAN;
    if (workspace_bytes < rgcn_bwd_dw_root_workspace_bytes()) return RGCN_ERR_WORKSPACE;
    const long ksteps = (rows + 3) / 4;
    const long want = (ksteps + 2 * kDwRootBatch - 1) / (2 * kDwRootBatch);      // at least one double batch per wave
    const int waves = (int)(want < 4 ? 4 : (want > kRootMaxWaves ? kRootMaxWaves : want));
    return dw_root_launch<true>(x, ldx, din, g, ldg, dout, rows, waves, workspace, d_root, d_bias, stream);
}

extern "C" size_t rgcn_rows_dw_workspace_bytes(int din, int dout) {
    if (din < 1 || din > RGCN_MAX_WIDTH || dout < 1 || dout > RGCN_MAX_WIDTH) return 0;
    return sizeof(float) * (size_t)kRowsDwMaxWaves * dw_root_slab_floats(false);
}

// d_w = x^T g over `rows` rows, widths up to 128 per side; no rows: zeros
extern "C" int rgcn_rows_dw(const float* x, int ldx, int din, const float* g, int ldg, int dout, long rows, void* workspace,
                            size_t workspace_bytes, float* d_w, void* stream) {
    int st;
    if (!workspace || !d_w || (rows != 0 && (!x || !g))) return RGCN_ERR_NULL;      // (no rows: x and g are not read)
    if ((st = check_stride(ldx, din)) != RGCN_OK) return st;
    if ((st = check_stride(ldg, dout)) != RGCN_OK) return st;
    if (rows < 0) return RGCN_ERR_PLAN;
    if (workspace_bytes < rgcn_rows_dw_workspace_bytes(din, dout)) return RGCN_ERR_WORKSPACE;
    const int nq = ((din + 63) / 64) * ((dout + 63) / 64);
    const long ksteps = (rows + 3) / 4;
    const long want = (ksteps + 2 * kDwRootBatch - 1) / (2 * kDwRootBatch);      // at least one double batch per range
    const int parts = (int)(want > kRowsDwMaxWaves / nq ? kRowsDwMaxWaves / nq : want);
    return dw_root_launch<false>(x, ldx, din, g, ldg, dout, rows, parts, workspace, d_w, nullptr, stream);
}

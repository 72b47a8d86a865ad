// rgcn_xwide.hip -- rgcn_xwide_* of include/rgcn_mi355x.h: forward, dX and weight gradients of R-GCN layers with 1..512 features
// per side (the other kernels stop at 128), in exact fp32 on v_mfma_f32_16x16x4_f32.  Same arithmetic as rgcn_fwd / rgcn_bwd_dx /
// rgcn_bwd_dw on the same layout-0 plans (DESIGN.md §10 "Layers wider than 128").
//
// Kernels:
//   xw_tile_kernel<NB>  forward (forward plan, W_r) and dX (transposed plan, W_r^T): one 256-thread workgroup per (plan tile, block
//                       of NB output columns).  It walks the tile's chunks; per chunk the gathered, weighted rows come in K-slices of
//                       32 columns through LDS (so a 512-wide row never has to fit whole) next to the matching 32 x NB slice of W,
//                       staged through registers one slice ahead.  Each wave owns NB / 4 columns and keeps a 16 x 16 fp32 MFMA
//                       accumulator per (16-slot row tile, 16 columns) of the chunk in registers.  After the chunk's last slice a
//                       segmented scan over the 16 rows of every row tile (sorted by destination) sums the runs of equal
//                       destination, and the lane holding a run's last row adds it into the tile's LDS accumulator: one writer per
//                       (row, column) at a time, in plan order -- deterministic, no atomics.  Epilogue: bias, activation, ReLU mask.
//   xw_dw_kernel        d_W_r = H_r^T g (and d_root: relation R') on a relation-major walk of the forward plan's 64-slot units
//                       (rel_order): workgroup (piece p, block of K x N: 128 x 128, or 64 x 256 / 256 x 64 when a side is at most
//                       64), 4 waves with a 64 x 64 accumulator each in registers.  A relation wholly inside the piece is stored
//                       straight into its output; the partials of the relations a piece shares with its neighbours go to a
//                       workspace slab, which xw_dw_reduce sums in piece order.
//   xw_bias_partial / xw_bias_reduce   d_bias = column sums of g: fixed row blocks, then the block sums in order.
// Every row offset is 64-bit: a 512-wide fp32 matrix passes 4 GiB at 2,097,152 rows.
#include <type_traits>
#include "rgcn_kernels_shared.h"

namespace rgcn {

namespace {

constexpr int kXwThreads = 256;
constexpr int kXwKS = 32;              // gathered columns per K-slice of the forward / dX kernel
constexpr int kXwAS = kXwKS + 4;       // row stride (floats) of the gathered slice in LDS: 16 rows of a fragment read hit 16 bank groups
constexpr int kXwMaxRT = 8;            // 16-slot row tiles per chunk (128-slot chunks)
constexpr int kXwDwB = 128;            // d_W block: 128 x 128 outputs per workgroup
constexpr int kXwBiasRows = 256;       // rows per block of the d_bias partial sums (at most 1024 blocks)
constexpr int kXwDwWorkgroups = 512;   // workgroups of one d_W launch (pieces x blocks), about two per CU

struct XwTileArgs {
    const int* tile_ptr;
    const int* chunk_rel;
    const int* chunk_cnt;
    const int* slot_src;
    const float* slot_w;
    const int* slot_row;
    int n_nodes, n_owned, tile, chunk;
    const float* a;      // gathered matrix [n_nodes, lda]: x (forward) or g (dX)
    long lda;
    int K;               // its width
    const float* w;      // [R' + 1, K, N] row-major, root last
    int N;               // output width
    const float* bias;   // [N] or NULL
    int act;
    const float* mask;   // [n_owned, ldm] or NULL (dX of a ReLU input)
    long ldm;
    float* out;          // [n_owned, ldo]
    long ldo;
};

size_t tile_lds_bytes(int tile, int nb, int chunk) {
    return (size_t)chunk * kXwAS * 4 + (size_t)kXwKS * (nb + 16) * 4 + (size_t)chunk * 4 + (size_t)tile * nb * 4;
}

// registers for two workgroups per CU: the LDS of tiles up to 64 rows allows two (60 KiB at NB 128); the 192-row tiles of large
// graphs (123 KiB) run one per CU
template <int NB>
__global__ void __launch_bounds__(kXwThreads, 2) xw_tile_kernel(const XwTileArgs a) {
    constexpr int WS = NB + 16;         // W-slice row stride: the 4 k-rows of a B fragment hit 4 bank groups
    constexpr int NW = NB / 64;         // 16-column MFMA blocks per wave
    constexpr int WI = NB * kXwKS / kXwThreads;   // W-slice elements staged per thread
    extern __shared__ float xw_lds[];
    float* As = xw_lds;                               // [chunk][kXwAS]   weighted gathered rows, one K-slice
    float* Ws = As + (size_t)a.chunk * kXwAS;         // [kXwKS][WS]      W_rel rows k0 .. k0 + 31, columns n0 .. n0 + NB - 1
    int* Ds = (int*)(Ws + kXwKS * WS);                // [chunk]          destination row in the tile (tile: padding)
    float* acc = (float*)(Ds + a.chunk);              // [tile][NB]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x;
    const int n0 = blockIdx.y * NB;
    const long r0 = (long)t * a.tile;
    const int nrows = (int)min((long)a.tile, (long)a.n_owned - r0);
    const int K4 = (a.K + 3) & ~3, N4 = (a.N + 3) & ~3;
    const int nslices = (a.K + kXwKS - 1) / kXwKS;
    const int wcol = wave * (NB / 4);                 // this wave's first column in the block
    const bool wave_live = n0 + wcol < a.N;
    for (int i = tid; i < a.tile * NB; i += kXwThreads) acc[i] = 0.f;
    const int c1_ = ldc(a.tile_ptr, t + 1);

    // Loads are unconditional (invalid rows and columns read the 16 zero bytes of g_zero16) and nothing is computed on their
    // results before the stage that consumes them, so no wait sits in front of the MFMAs.  The slot indices of a chunk are
    // loaded while the chunk before it is walked: a row load never waits for its index.
    f32x4 ra[4];
    float rw[WI];
    int isrc[4], jsrc[4], irow = a.tile, jrow = a.tile;    // i: the chunk whose rows are fetched; j: the chunk after it
    float iw[4], jw[4];
    auto load_idx = [&](int c, int* src, float* wt, int& row_d) {
        const bool have = c < c1_;
        const int cnt = have ? ldc(a.chunk_cnt, c) : 0;
        const long base = (long)c * a.chunk;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int slot = (tid + kXwThreads * u) >> 3;
            const bool in = slot < cnt;
            src[u] = in ? a.slot_src[base + slot] : a.n_nodes;
            wt[u] = in ? a.slot_w[base + slot] : 0.f;
        }
        const int row = (have && tid < cnt) ? a.slot_row[base + tid] : a.n_owned;
        row_d = row < a.n_owned ? (int)(row - r0) : a.tile;
    };
    auto fetch = [&](int c, int s) {
        const int rel = ldc(a.chunk_rel, c);
        const int k0 = s * kXwKS;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = k0 + 4 * ((tid + kXwThreads * u) & 7);
            const bool ok = iw[u] != 0.f && (unsigned)isrc[u] < (unsigned)a.n_nodes && col < K4;
            ra[u] = *(const f32x4*)(ok ? a.a + (size_t)isrc[u] * a.lda + col : g_zero16);
        }
        const float* wr = a.w + (size_t)rel * a.K * a.N;
#pragma unroll
        for (int u = 0; u < WI; ++u) {
            const int i = tid + kXwThreads * u;
            const int k = k0 + i / NB, n = n0 + i % NB;
            rw[u] = *((k < a.K && n < a.N) ? wr + (size_t)k * a.N + n : g_zero16);
        }
    };
    auto stage = [&](int s) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = tid + kXwThreads * u;
            if ((i >> 3) < a.chunk) *(f32x4*)(As + (i >> 3) * kXwAS + 4 * (i & 7)) = iw[u] * ra[u];
        }
#pragma unroll
        for (int u = 0; u < WI; ++u) {
            const int i = tid + kXwThreads * u;
            Ws[(i / NB) * WS + i % NB] = rw[u];
        }
        if (s == 0 && tid < a.chunk) Ds[tid] = irow;
    };

    f32x4 cacc[kXwMaxRT][NW];
    const int c0 = ldc(a.tile_ptr, t), c1 = c1_;
    if (c0 < c1) {
        load_idx(c0, isrc, iw, irow);
        load_idx(c0 + 1, jsrc, jw, jrow);
        fetch(c0, 0);
    }
    int c = c0, s = 0;
    while (c < c1) {
        const int cnt = ldc(a.chunk_cnt, c);
        const int nrt = cnt >> 4;
        __syncthreads();                 // the previous item's MFMAs and scatter are done with As / Ws / Ds
        stage(s);
        __syncthreads();
        int cn = c, sn = s + 1;
        if (sn == nslices) {
            cn = c + 1;
            sn = 0;
        }
        if (cn != c && cn < c1) {        // the fetch moves to the next chunk: its indices are here, load the one after it
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                isrc[u] = jsrc[u];
                iw[u] = jw[u];
            }
            irow = jrow;
            load_idx(cn + 1, jsrc, jw, jrow);
        }
        if (cn < c1) fetch(cn, sn);      // in flight under this item's MFMAs
        if (s == 0) {
#pragma unroll
            for (int rt = 0; rt < kXwMaxRT; ++rt)
#pragma unroll
                for (int j = 0; j < NW; ++j) cacc[rt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (wave_live) {
            // one fully unrolled MFMA walk per row-tile count: LDS offsets are immediates, no per-tile branch
            const int ksteps = min(kXwKS, K4 - s * kXwKS) >> 2;
            const float* ab = As + (lane & 15) * kXwAS + (lane >> 4);
            const float* bb = Ws + (lane >> 4) * WS + wcol + (lane & 15);
            auto slice = [&](auto nrt_c) {
                constexpr int R = decltype(nrt_c)::value;
#pragma unroll
                for (int kk = 0; kk < kXwKS / 4; ++kk) {
                    if (kk >= ksteps) break;
                    float bv[NW];
#pragma unroll
                    for (int j = 0; j < NW; ++j) bv[j] = bb[kk * 4 * WS + j * 16];
#pragma unroll
                    for (int rt = 0; rt < R; ++rt) {
                        const float av = ab[rt * 16 * kXwAS + kk * 4];
#pragma unroll
                        for (int j = 0; j < NW; ++j) cacc[rt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], cacc[rt][j], 0, 0, 0);
                    }
                }
            };
            switch (nrt) {
                case 1: slice(std::integral_constant<int, 1>{}); break;
                case 2: slice(std::integral_constant<int, 2>{}); break;
                case 3: slice(std::integral_constant<int, 3>{}); break;
                case 4: slice(std::integral_constant<int, 4>{}); break;
                case 5: slice(std::integral_constant<int, 5>{}); break;
                case 6: slice(std::integral_constant<int, 6>{}); break;
                case 7: slice(std::integral_constant<int, 7>{}); break;
                default: slice(std::integral_constant<int, 8>{}); break;
            }
        }
        if (s == nslices - 1 && wave_live) {
            // scatter: lane holds rows 4 q + 0..3 (q = lane / 16) of column lane % 16 of every 16 x 16 block; rows of a row tile are
            // sorted by destination, so the runs of equal destination are contiguous
            const int q = lane >> 4;
#pragma unroll
            for (int rt = 0; rt < kXwMaxRT; ++rt) {
                if (rt >= nrt) break;
                const int4 d = *(const int4*)(Ds + rt * 16 + 4 * q);
                const int dprev = __shfl_up(d.w, 16);
                const int dnext = __shfl_down(d.x, 16);
                const bool join = q > 0 && dprev == d.x;        // the group's first run continues the previous group's last
                const bool full = d.x == d.w;
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    f32x4 v = cacc[rt][j];
                    if (d.y == d.x) v[1] += v[0];
                    if (d.z == d.y) v[2] += v[1];
                    if (d.w == d.z) v[3] += v[2];
                    float tail = v[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const float up = __shfl_up(tail, 16);
                        tail = v[3] + ((full && join) ? up : 0.f);
                    }
                    const float carry = __shfl_up(tail, 16);
                    if (join) {
                        v[0] += carry;
                        if (d.y == d.x) v[1] += carry;
                        if (d.z == d.x) v[2] += carry;
                        if (d.w == d.x) v[3] += carry;
                    }
                    const int col = wcol + j * 16 + (lane & 15);
                    if (d.y != d.x && d.x < a.tile) acc[d.x * NB + col] += v[0];
                    if (d.z != d.y && d.y < a.tile) acc[d.y * NB + col] += v[1];
                    if (d.w != d.z && d.z < a.tile) acc[d.z * NB + col] += v[2];
                    if ((q == 3 || dnext != d.w) && d.w < a.tile) acc[d.w * NB + col] += v[3];
                }
            }
        }
        c = cn;
        s = sn;
    }
    __syncthreads();
    for (int i = tid; i < nrows * (NB / 4); i += kXwThreads) {
        const int row = i / (NB / 4), c4 = i % (NB / 4);
        const int col = n0 + 4 * c4;
        if (col >= N4) continue;
        f32x4 v = *(const f32x4*)(acc + row * NB + 4 * c4);
        f32x4 m = {1.f, 1.f, 1.f, 1.f};
        if (a.mask != nullptr) m = *(const f32x4*)(a.mask + (size_t)(r0 + row) * a.ldm + col);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (col + k >= a.N) {
                v[k] = 0.f;
                continue;
            }
            if (a.bias != nullptr) v[k] += a.bias[col + k];
            if (a.act == RGCN_ACT_RELU) v[k] = v[k] > 0.f ? v[k] : 0.f;
            else if (a.act == RGCN_ACT_SIGMOID) v[k] = 1.f / (1.f + expf(-v[k]));
            if (a.mask != nullptr && !(m[k] > 0.f)) v[k] = 0.f;
        }
        *(f32x4*)(a.out + (size_t)(r0 + row) * a.ldo + col) = v;
    }
}

struct XwDwArgs {
    const int* rel_order;
    const int* chunk_rel;
    const int* chunk_cnt;
    const int* slot_src;
    const float* slot_w;
    const int* slot_row;
    int n_nodes, n_owned, num_rel, n_units, upc, pieces;
    const float* x;
    long ldx;
    int K;
    const float* g;
    long ldg;
    int N;
    float* d_weight;     // [R', K, N] or NULL
    float* d_root;       // [K, N] or NULL
    float* slab;         // [pieces][2][K][N]
};

__device__ __forceinline__ int unit_rel(const XwDwArgs& a, long u) { return ldc(a.chunk_rel, ldc(a.rel_order, u) / a.upc); }
__device__ __forceinline__ long piece_start(long p, long n_units, long pieces) { return p * n_units / pieces; }
__device__ __forceinline__ float* rel_out(const XwDwArgs& a, int rel) {
    return rel < a.num_rel ? (a.d_weight ? a.d_weight + (size_t)rel * a.K * a.N : nullptr) : a.d_root;
}

template <int BM, int BN>
__global__ void __launch_bounds__(kXwThreads) xw_dw_kernel(const XwDwArgs a) {
    constexpr int SM = BM + 16, SN = BN + 16;   // LDS row strides: the 4 slot rows of a fragment read hit 4 bank groups
    constexpr int WN = BN / 64;                 // waves along N (4 / WN along M)
    constexpr int XC = BM / 4, GC = BN / 4;     // 16-byte pieces per staged row
    constexpr int XI = 64 * XC / kXwThreads, GI = 64 * GC / kXwThreads;
    extern __shared__ float xw_lds[];
    float* Xs = xw_lds;                   // [64 slots][SM]  w * x[src], columns m0 .. m0 + BM - 1
    float* Gs = Xs + 64 * SM;             // [64 slots][SN]  g[dst],     columns n0 .. n0 + BN - 1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p = blockIdx.x;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.z * BN;
    const int wm = m0 + (wave / WN) * 64, wn = n0 + (wave % WN) * 64;   // this wave's 64 x 64 output block
    const int K4 = (a.K + 3) & ~3, N4 = (a.N + 3) & ~3;
    const long u0 = piece_start(p, a.n_units, a.pieces), u1 = piece_start(p + 1, a.n_units, a.pieces);
    if (u0 >= u1) return;
    const int rel_first = unit_rel(a, u0), rel_last = unit_rel(a, u1 - 1);
    const bool cont_in = u0 > 0 && unit_rel(a, u0 - 1) == rel_first;
    const bool cont_out = u1 < a.n_units && unit_rel(a, u1) == rel_last;

    // the slot indices of unit u + 2 are loaded while the rows of unit u + 1 are, under the MFMAs of unit u; loads are
    // unconditional (g_zero16 for padding) and the edge weight is applied when the rows are staged
    f32x4 rx[XI], rg[GI];
    int isrc[XI], irow[GI];
    float iw[XI], sw[XI];
    auto load_idx = [&](long u) {
        const bool have = u < u1;
        const int unit = have ? ldc(a.rel_order, u) : 0;
        const long base = (long)unit * 64;
        const bool live = have && rel_out(a, ldc(a.chunk_rel, unit / a.upc)) != nullptr;
#pragma unroll
        for (int v = 0; v < XI; ++v) {
            const int slot = (tid + kXwThreads * v) / XC;
            isrc[v] = live ? a.slot_src[base + slot] : a.n_nodes;
            iw[v] = live ? a.slot_w[base + slot] : 0.f;
        }
#pragma unroll
        for (int v = 0; v < GI; ++v) irow[v] = live ? a.slot_row[base + (tid + kXwThreads * v) / GC] : a.n_owned;
    };
    auto fetch = [&]() {
#pragma unroll
        for (int v = 0; v < XI; ++v) {
            const int c4 = 4 * ((tid + kXwThreads * v) % XC);
            const bool ok = m0 + c4 < K4 && iw[v] != 0.f && (unsigned)isrc[v] < (unsigned)a.n_nodes;
            rx[v] = *(const f32x4*)(ok ? a.x + (size_t)isrc[v] * a.ldx + m0 + c4 : g_zero16);
            sw[v] = ok ? iw[v] : 0.f;
        }
#pragma unroll
        for (int v = 0; v < GI; ++v) {
            const int c4 = 4 * ((tid + kXwThreads * v) % GC);
            const bool ok = n0 + c4 < N4 && (unsigned)irow[v] < (unsigned)a.n_owned;
            rg[v] = *(const f32x4*)(ok ? a.g + (size_t)irow[v] * a.ldg + n0 + c4 : g_zero16);
        }
    };
    f32x4 acc[4][4];
    auto zero_acc = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto flush = [&](int rel) {
        float* o = rel_out(a, rel);
        if (o == nullptr) return;
        if ((rel == rel_first && cont_in) || (rel == rel_last && cont_out))
            o = a.slab + ((size_t)p * 2 + (rel == rel_first ? 0 : 1)) * a.K * a.N;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int m = wm + i * 16 + 4 * (lane >> 4) + k, n = wn + j * 16 + (lane & 15);
                    if (m < a.K && n < a.N) o[(size_t)m * a.N + n] = acc[i][j][k];
                }
    };

    zero_acc();
    int cur = rel_first;
    load_idx(u0);
    fetch();
    load_idx(u0 + 1);
    for (long u = u0; u < u1; ++u) {
        const int unit = ldc(a.rel_order, u);
        const int rel = ldc(a.chunk_rel, unit / a.upc);
        if (rel != cur) {
            flush(cur);
            zero_acc();
            cur = rel;
        }
        const int used = min(64, ldc(a.chunk_cnt, unit / a.upc) - 64 * (unit % a.upc));
        __syncthreads();
#pragma unroll
        for (int v = 0; v < XI; ++v) {
            const int i = tid + kXwThreads * v;
            *(f32x4*)(Xs + (i / XC) * SM + 4 * (i % XC)) = sw[v] * rx[v];
        }
#pragma unroll
        for (int v = 0; v < GI; ++v) {
            const int i = tid + kXwThreads * v;
            *(f32x4*)(Gs + (i / GC) * SN + 4 * (i % GC)) = rg[v];
        }
        __syncthreads();
        if (u + 1 < u1) {
            fetch();
            load_idx(u + 2);
        }
        if (rel_out(a, rel) == nullptr || wm >= K4 || wn >= N4) continue;
        const float* xb = Xs + (lane >> 4) * SM + (wm - m0) + (lane & 15);
        const float* gbp = Gs + (lane >> 4) * SN + (wn - n0) + (lane & 15);
        bool mv[4], nv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mv[i] = wm + i * 16 < K4;
            nv[i] = wn + i * 16 < N4;
        }
        for (int k16 = 0; k16 < (used >> 4); ++k16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r4 = (k16 * 4 + q) * 4;
                float xa[4], gb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) xa[i] = xb[r4 * SM + i * 16];
#pragma unroll
                for (int j = 0; j < 4; ++j) gb[j] = gbp[r4 * SN + j * 16];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (mv[i] && nv[j]) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[i], gb[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    flush(cur);
}

// relation r (R' = root) of d_W: zeros when the plan has no unit of r; the piece partials in piece order when r spans pieces
__global__ void __launch_bounds__(256) xw_dw_reduce(const XwDwArgs a) {
    const int r = blockIdx.y;
    float* o = rel_out(a, r);
    if (o == nullptr) return;
    long lo = 0, hi = a.n_units;                   // first unit of relation >= r
    while (lo < hi) {
        const long m = (lo + hi) / 2;
        if (unit_rel(a, m) < r) lo = m + 1; else hi = m;
    }
    long e = lo, hi2 = a.n_units;                  // first unit of relation > r
    while (e < hi2) {
        const long m = (e + hi2) / 2;
        if (unit_rel(a, m) <= r) e = m + 1; else hi2 = m;
    }
    auto piece_of = [&](long u) -> long {          // the last piece whose range starts at or before u
        long l = 0, h = a.pieces - 1;
        while (l < h) {
            const long m = (l + h + 1) / 2;
            if (piece_start(m, a.n_units, a.pieces) <= u) l = m; else h = m - 1;
        }
        return l;
    };
    const size_t kn = (size_t)a.K * a.N;
    long p_lo = 0, p_hi = 0;
    if (lo < e) {
        p_lo = piece_of(lo);
        p_hi = piece_of(e - 1);
        if (p_lo == p_hi) return;                  // stored by its piece
    }
    const int first_slot = (lo < e && piece_start(p_lo, a.n_units, a.pieces) == lo) ? 0 : 1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < kn; i += (size_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        if (lo < e) {
            s = a.slab[((size_t)p_lo * 2 + first_slot) * kn + i];
            for (long p = p_lo + 1; p <= p_hi; ++p)
                if (piece_start(p, a.n_units, a.pieces) < piece_start(p + 1, a.n_units, a.pieces)) s += a.slab[(size_t)p * 2 * kn + i];
        }
        o[i] = s;
    }
}

__global__ void __launch_bounds__(256) xw_bias_partial(const float* g, long ldg, int n_owned, int N, int rows_per_block, float* slab) {
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = min((long)n_owned, r0 + rows_per_block);
    for (int col = threadIdx.x; col < N; col += 256) {
        float s = 0.f;
        for (long r = r0; r < r1; ++r) s += g[(size_t)r * ldg + col];
        slab[(size_t)blockIdx.x * N + col] = s;
    }
}

__global__ void __launch_bounds__(256) xw_bias_reduce(const float* slab, int nblk, int N, float* d_bias) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= N) return;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += slab[(size_t)b * N + col];
    d_bias[col] = s;
}

int xw_nb(int n) { return n <= 64 ? 64 : 128; }

int check_xw_width(int w) { return (w >= 1 && w <= RGCN_XWIDE_MAX_WIDTH) ? RGCN_OK : RGCN_ERR_WIDTH; }

int check_xw_stride(int ld, int width) {
    if (check_xw_width(width) != RGCN_OK) return RGCN_ERR_WIDTH;
    if ((ld % 4) != 0 || ld < ((width + 3) / 4) * 4) return RGCN_ERR_STRIDE;
    return RGCN_OK;
}

int check_xw_plan(const rgcn_plan_t* p) {
    const int st = check_plan(p);
    if (st != RGCN_OK) return st;
    // layout 0 only, chunks holding `chunk` rows
    if (p->layout != 0 || (p->chunk_rows != 0 && p->chunk_rows != p->chunk)) return RGCN_ERR_PLAN;
    return RGCN_OK;
}

// d_W block shape: 64 x 256 when din <= 64, 256 x 64 when dout <= 64 (so that all four waves own columns), else 128 x 128
int dw_shape(int din, int dout) { return din <= 64 && dout > 64 ? 1 : (dout <= 64 && din > 64 ? 2 : 0); }

int dw_pieces(const rgcn_plan_t* p, int din, int dout) {
    const int shape = dw_shape(din, dout);
    const int bm = shape == 1 ? 64 : (shape == 2 ? 256 : kXwDwB), bn = shape == 1 ? 256 : (shape == 2 ? 64 : kXwDwB);
    const int blocks = ((din + bm - 1) / bm) * ((dout + bn - 1) / bn);
    const int want = kXwDwWorkgroups / blocks;
    return std::max(1, std::min(p->n_units, want));
}

int bias_blocks(const rgcn_plan_t* p) { return std::min(1024, (p->n_owned + kXwBiasRows - 1) / kXwBiasRows); }

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

struct XwWs {
    size_t slab, bias, total;
};

XwWs dw_ws(const rgcn_plan_t* p, int din, int dout) {
    XwWs w;
    w.slab = 0;
    w.bias = align256((size_t)dw_pieces(p, din, dout) * 2 * din * dout * 4);
    w.total = w.bias + align256((size_t)bias_blocks(p) * dout * 4);
    return w;
}

template <int NB>
int launch_tile(const XwTileArgs& a, int n_tiles, size_t lds, hipStream_t s) {
    hipError_t e = allow_full_lds<xw_tile_kernel<NB>>();
    if (e != hipSuccess) return (int)e;
    const int ncb = (a.N + NB - 1) / NB;
    hipLaunchKernelGGL(xw_tile_kernel<NB>, dim3(n_tiles, ncb), dim3(kXwThreads), lds, s, a);
    return (int)hipGetLastError();
}

int tile_pass(const rgcn_plan_t* p, const float* a_mat, int lda, int K, const float* w, const float* bias, int act, const float* mask,
              int ldm, float* out, int ldo, int N, void* stream) {
    XwTileArgs a;
    memset(&a, 0, sizeof(a));
    a.tile_ptr = p->tile_ptr;
    a.chunk_rel = p->chunk_rel;
    a.chunk_cnt = p->chunk_cnt;
    a.slot_src = p->slot_src;
    a.slot_w = p->slot_w;
    a.slot_row = p->slot_row;
    a.n_nodes = p->n_nodes;
    a.n_owned = p->n_owned;
    a.tile = p->tile;
    a.chunk = p->chunk;
    a.a = a_mat;
    a.lda = lda;
    a.K = K;
    a.w = w;
    a.N = N;
    a.bias = bias;
    a.act = act;
    a.mask = mask;
    a.ldm = ldm;
    a.out = out;
    a.ldo = ldo;
    const int nb = xw_nb(N);
    const size_t lds = tile_lds_bytes(p->tile, nb, p->chunk);
    hipStream_t s = (hipStream_t)stream;
    return nb == 64 ? launch_tile<64>(a, p->n_tiles, lds, s) : launch_tile<128>(a, p->n_tiles, lds, s);
}

}  // namespace
}  // namespace rgcn

using namespace rgcn;

extern "C" int rgcn_xwide_geometry(int32_t n_nodes, int din, int dout, int* tile, int* chunk) {
    if (!tile || !chunk) return RGCN_ERR_NULL;
    if (check_xw_width(din) != RGCN_OK || check_xw_width(dout) != RGCN_OK) return RGCN_ERR_WIDTH;
    if (n_nodes <= 0) return RGCN_ERR_PLAN;
    // about a thousand tiles or more where the graph has the nodes: 192 rows from 196,608 nodes (larger (tile, relation) groups:
    // fewer W slices and padded row tiles per edge -- 1M nodes, 256 x 256: forward 51 -> 43 ms, d_W 35 -> 21 ms against tile 64),
    // 64 from 65,536, 32 from 32,768, else 16
    int t = n_nodes >= 196608 ? 192 : (n_nodes >= 65536 ? 64 : (n_nodes >= 32768 ? 32 : 16));
    const int nb = std::max(xw_nb(din), xw_nb(dout));     // the forward and the dX plan share the tile
    if (tile_lds_bytes(t, nb, 64) > (size_t)kLdsBytes) return RGCN_ERR_LDS;
    *tile = t;
    *chunk = 64;
    return RGCN_OK;
}

extern "C" int rgcn_xwide_fwd(const rgcn_plan_t* plan, const float* x, int ldx, int din, const float* weight, const float* bias,
                              float* out, int ldo, int dout, int act, void* stream) {
    if (!plan || !x || !weight || !out) return RGCN_ERR_NULL;
    if (check_xw_width(din) != RGCN_OK || check_xw_width(dout) != RGCN_OK) return RGCN_ERR_WIDTH;
    int st;
    if ((st = check_xw_stride(ldx, din)) != RGCN_OK) return st;
    if ((st = check_xw_stride(ldo, dout)) != RGCN_OK) return st;
    if (act != RGCN_ACT_NONE && act != RGCN_ACT_RELU && act != RGCN_ACT_SIGMOID) return RGCN_ERR_ACT;
    if ((st = check_xw_plan(plan)) != RGCN_OK) return st;
    if (tile_lds_bytes(plan->tile, xw_nb(dout), plan->chunk) > (size_t)kLdsBytes) return RGCN_ERR_LDS;
    if ((st = check_device()) != RGCN_OK) return st;
    return tile_pass(plan, x, ldx, din, weight, bias, act, nullptr, 0, out, ldo, dout, stream);
}

extern "C" int rgcn_xwide_bwd_dx(const rgcn_plan_t* plan_t, const float* g, int ldg, int dout, const float* weight_t, float* dx,
                                 int lddx, int din, const float* relu_of, int ldr, void* stream) {
    if (!plan_t || !g || !weight_t || !dx) return RGCN_ERR_NULL;
    if (check_xw_width(din) != RGCN_OK || check_xw_width(dout) != RGCN_OK) return RGCN_ERR_WIDTH;
    int st;
    if ((st = check_xw_stride(ldg, dout)) != RGCN_OK) return st;
    if ((st = check_xw_stride(lddx, din)) != RGCN_OK) return st;
    if (relu_of && (st = check_xw_stride(ldr, din)) != RGCN_OK) return st;
    if ((st = check_xw_plan(plan_t)) != RGCN_OK) return st;
    if (tile_lds_bytes(plan_t->tile, xw_nb(din), plan_t->chunk) > (size_t)kLdsBytes) return RGCN_ERR_LDS;
    if ((st = check_device()) != RGCN_OK) return st;
    return tile_pass(plan_t, g, ldg, dout, weight_t, nullptr, RGCN_ACT_NONE, relu_of, ldr, dx, lddx, din, stream);
}

extern "C" size_t rgcn_xwide_bwd_dw_workspace_bytes(const rgcn_plan_t* plan, int din, int dout) {
    if (check_xw_plan(plan) != RGCN_OK || check_xw_width(din) != RGCN_OK || check_xw_width(dout) != RGCN_OK) return 0;
    return dw_ws(plan, din, dout).total;
}

extern "C" int rgcn_xwide_bwd_dw(const rgcn_plan_t* plan, const float* x, int ldx, int din, const float* g, int ldg, int dout,
                                 void* workspace, size_t workspace_bytes, float* d_weight, float* d_root, float* d_bias, void* stream) {
    if (!plan || !x || !g || !workspace) return RGCN_ERR_NULL;
    if (check_xw_width(din) != RGCN_OK || check_xw_width(dout) != RGCN_OK) return RGCN_ERR_WIDTH;
    int st;
    if ((st = check_xw_stride(ldx, din)) != RGCN_OK) return st;
    if ((st = check_xw_stride(ldg, dout)) != RGCN_OK) return st;
    if ((st = check_xw_plan(plan)) != RGCN_OK) return st;
    const XwWs wl = dw_ws(plan, din, dout);
    if (workspace_bytes < wl.total) return RGCN_ERR_WORKSPACE;
    if ((st = check_device()) != RGCN_OK) return st;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (d_weight || d_root) {
        XwDwArgs a;
        memset(&a, 0, sizeof(a));
        a.rel_order = plan->rel_order;
        a.chunk_rel = plan->chunk_rel;
        a.chunk_cnt = plan->chunk_cnt;
        a.slot_src = plan->slot_src;
        a.slot_w = plan->slot_w;
        a.slot_row = plan->slot_row;
        a.n_nodes = plan->n_nodes;
        a.n_owned = plan->n_owned;
        a.num_rel = plan->num_relations;
        a.n_units = plan->n_units;
        a.upc = plan->chunk / 64;
        a.pieces = dw_pieces(plan, din, dout);
        a.x = x;
        a.ldx = ldx;
        a.K = din;
        a.g = g;
        a.ldg = ldg;
        a.N = dout;
        a.d_weight = d_weight;
        a.d_root = d_root;
        a.slab = (float*)(ws + wl.slab);
        const int shape = dw_shape(din, dout);
        const int bm = shape == 1 ? 64 : (shape == 2 ? 256 : kXwDwB), bn = shape == 1 ? 256 : (shape == 2 ? 64 : kXwDwB);
        const size_t lds = (size_t)64 * ((bm + 16) + (bn + 16)) * 4;
        const dim3 grid(a.pieces, (din + bm - 1) / bm, (dout + bn - 1) / bn);
        hipError_t e;
        if (shape == 1) {
            if ((e = allow_full_lds<xw_dw_kernel<64, 256>>()) != hipSuccess) return (int)e;
            hipLaunchKernelGGL((xw_dw_kernel<64, 256>), grid, dim3(kXwThreads), lds, s, a);
        } else if (shape == 2) {
            if ((e = allow_full_lds<xw_dw_kernel<256, 64>>()) != hipSuccess) return (int)e;
            hipLaunchKernelGGL((xw_dw_kernel<256, 64>), grid, dim3(kXwThreads), lds, s, a);
        } else {
            if ((e = allow_full_lds<xw_dw_kernel<kXwDwB, kXwDwB>>()) != hipSuccess) return (int)e;
            hipLaunchKernelGGL((xw_dw_kernel<kXwDwB, kXwDwB>), grid, dim3(kXwThreads), lds, s, a);
        }
        if ((st = (int)hipGetLastError()) != RGCN_OK) return st;
        const size_t kn = (size_t)din * dout;
        const unsigned gx = (unsigned)std::min<size_t>((kn + 255) / 256, 1024);
        hipLaunchKernelGGL(xw_dw_reduce, dim3(gx, plan->num_relations + 1), dim3(256), 0, s, a);
        if ((st = (int)hipGetLastError()) != RGCN_OK) return st;
    }
    if (d_bias) {
        const int nblk = bias_blocks(plan);
        float* slab = (float*)(ws + wl.bias);
        hipLaunchKernelGGL(xw_bias_partial, dim3(nblk), dim3(256), 0, s, g, (long)ldg, plan->n_owned, dout,
                           (plan->n_owned + nblk - 1) / nblk, slab);
        if ((st = (int)hipGetLastError()) != RGCN_OK) return st;
        hipLaunchKernelGGL(xw_bias_reduce, dim3((dout + 255) / 256), dim3(256), 0, s, (const float*)slab, nblk, dout, d_bias);
        if ((st = (int)hipGetLastError()) != RGCN_OK) return st;
    }
    return RGCN_OK;
}

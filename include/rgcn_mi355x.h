/*
 * rgcn_mi355x.h -- C ABI of librgcn_mi355x.so: the R-GCN layer hot path (forward + backward of
 * the per-relation sparse message passing  out = sum_r D_r^-1 A_r X W_r + X root + b) as
 * hand-written HIP kernels for gfx950 (MI355X).
 *
 * What each entry point replaces in the reference (paths relative to /root/reference):
 *   - the arithmetic of torch_geometric.nn.RGCNConv (torch_geometric==2.3.1, requirements.txt:7),
 *     which the reference reaches from model/layers.py:21,23 (Emb_Layers.forward), :62,64
 *     (Emb_ATT_Layers.forward) and :108,110 (Emb_MLP_Layers.forward), and differentiates through at
 *     model/modelTrainer.py:66 (output.backward()).
 * The reference has no FFI of its own (it is pure Python); INTEGRATION.md shows the ctypes stub a
 * maintainer would add.
 *
 * Conventions (SURVEY.md 8b "C ABI"):
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless stated otherwise;
 *   - every function returns an int status (0 = RGCN_OK, negative = argument error, positive =
 *     hipError_t of a failed launch); nothing throws;
 *   - nothing allocates: workspaces are sized by the *_bytes / *_floats queries and owned by the caller;
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream); no host synchronisation, no global mutable state -> re-entrant on distinct streams
 *     and capturable into a hipGraph.
 *   - float32 features, int32 indices.  Feature row strides (ld*) are in ELEMENTS, must be multiples
 *     of 4 (16-byte rows) and >= the feature width; columns between the width and the width rounded
 *     up to a multiple of 4 must hold zeros (the Python host pads when needed).
 *   - feature widths 1..128 per side (rgcn_xwide_*: 1..RGCN_XWIDE_MAX_WIDTH).
 */
#ifndef RGCN_MI355X_H
#define RGCN_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGCN_ABI_VERSION 19
#define RGCN_UNIT 64 /* edge slots per unit of the weight-gradient walk (rel_order); a chunk is 1 or 2 units */
#define RGCN_CHUNK_MAX 128 /* plan->chunk is 64 or 128 edge slots (rows of one LDS ring slot of the forward / dX kernel) */
#define RGCN_MAX_WIDTH 128
#define RGCN_XWIDE_MAX_WIDTH 512 /* rgcn_xwide_*: feature widths 1..512 per side */
#define RGCN_DW_WALKERS 2048 /* waves that walk rel_order side by side in the largest relation-major dW launch (512 workgroups x 4) */

/* activation fused into rgcn_fwd's store (reference model/layers.py:22 F.relu, :24 activation = torch.sigmoid) */
enum rgcn_act { RGCN_ACT_NONE = 0, RGCN_ACT_RELU = 1, RGCN_ACT_SIGMOID = 2 };

/* per-call options (bit mask); 0 = let the library choose */
#define RGCN_FLAG_POINTER_GATHER 1u /* address gathered rows with 64-bit pointers even where a buffer descriptor fits */
#define RGCN_FLAG_DW_RING 2u        /* rgcn_bwd_dw: LDS-ring kernels whatever the size */
#define RGCN_FLAG_DW_DIRECT 4u      /* rgcn_bwd_dw: direct-gather kernel whenever the widths allow (64 x 64) */
#define RGCN_FLAG_DW_ROOT_ONLY 16u   /* rgcn_bwd_dw: d_root and d_bias only (the relations went to rgcn_bwd_dw_tiles) */
#define RGCN_FLAG_SPLIT_PRODUCERS 32u /* rgcn_fwd / rgcn_bwd_dx: the bf16 x 3 kernel whose PRODUCER waves split the gathered rows
                                       * (fp32-equivalent: 24 significant bits on both operands, six bf16 products): 64 x 64 layers,
                                       * 128-slot chunks, tile <= 224 (layout-1 plans too, walked like layout 0); other shapes take the exact-fp32 kernel.
                                       * rgcn_bwd_dw_tiles: the same walk with both operands split into three bf16 pieces in registers
                                       * (six bf16 products, fp32 accumulation; same fp32-equivalence) */
#define RGCN_FLAG_EXACT_FP32 8u     /* rgcn_fwd / rgcn_bwd_dx: the exact-fp32 MFMA kernel whatever else the flags ask for */

enum rgcn_status {
    RGCN_OK = 0,
    RGCN_ERR_NULL = -1,      /* a required pointer is NULL */
    RGCN_ERR_WIDTH = -2,     /* feature width outside 1..128 */
    RGCN_ERR_STRIDE = -3,    /* a row stride is not a multiple of 4 or smaller than the width */
    RGCN_ERR_PLAN = -4,      /* inconsistent plan (sizes <= 0, tile not a multiple of 16, ...) */
    RGCN_ERR_LDS = -5,       /* plan tile too large for the 160 KiB LDS at these widths */
    RGCN_ERR_WORKSPACE = -6, /* workspace smaller than the *_workspace_bytes query */
    RGCN_ERR_DEVICE = -7,    /* current device is not gfx950 / no device */
    RGCN_ERR_ACT = -8,       /* unknown activation code */
    RGCN_ERR_GRAPH = -9,     /* rgcn_plan_build, rgcn_sample_*, rgcn_mb_index_build: an edge_index / edge_type value is out of range */
    RGCN_ERR_ADDRESS = -10,  /* rgcn_bwd_dw_tiles: a gathered matrix cannot be addressed through a buffer descriptor (2^24 rows or
                              * 4 GiB and more): use rgcn_bwd_dw, whose kernels fall back to 64-bit pointers */
    RGCN_ERR_ARG = -11,      /* rgcn_sample_*: a scalar argument outside its domain (fan-out, seed, hop, number of destinations),
                              * or a destination listed twice */
    RGCN_ERR_COLLISION = -12 /* rgcn_nt_build: two different terms share their hash_bits hash bits: nothing was merged; call again
                              * with more bits or another seed */
};

/* Graph plan in HBM, built once per graph (scaling_rgcn_training_amd/plan.py documents the layout;
 * PyG rebuilds the per-relation masks and counts on every forward call instead).
 * Rows scattered into are the plan's OWNED node range, numbered from 0 (= node_begin). */
typedef struct rgcn_plan {
    int32_t n_nodes;       /* rows of the gathered matrix (whole graph) */
    int32_t n_owned;       /* output rows (node_end - node_begin) */
    int32_t num_relations; /* R'; the self-loop ("root") is relation id R' */
    int32_t tile;          /* output nodes per tile (multiple of 16) */
    int32_t n_tiles;
    int32_t n_chunks;
    int32_t chunk;         /* edge slots per chunk: 64 or 128 (rows of one LDS ring slot of the forward / dX kernel) */
    int32_t n_units;       /* entries of rel_order */
    int32_t layout;        /* 0: the rows of a (tile, relation) group are dealt over all its row tiles; 1 (chunk = 128): TEAM
                            * placement -- a chunk's rows are cut at a change of destination into part A on its first
                            * ceil(nt / 2) row tiles and part B on the others, so the two parts scatter into disjoint rows
                            * (chunk_flags bit 8: they do not); every kernel that takes layout 0 walks it the same way;
                            * same chunks and row-tile counts as layout 0;
                            * 2: no tiles -- dense relation-major units for rgcn_bwd_dw only (rgcn_edge_units);
                            * 3 (chunk = 128): layout 0 with the rows of a (destination, relation) run on ONE slot where a chunk is
                            * a whole (tile, relation) group with runs of at most 3 rows: heads on slots 0 .. H-1, second rows on
                            * row tile 7 - h / 16 (place h % 16), third rows on the row tile below those (6 or 5); chunk_cnt counts the head row tiles,
                            * chunk_flags bits 20-23 repeat every chunk's row-tile count, bits 16-17 / 18 count the row tiles of
                            * second / third rows, bit 19 "the rows of a run differ in
                            * weight" (a shadow slot's slot_acc then holds the float weight / head's weight).  Walked by rgcn_fwd / rgcn_bwd_dx with RGCN_FLAG_SPLIT_PRODUCERS on 64 x 64 layers only (the
                            * producer waves add a run's rows before they cut them: aggregate, then transform); every other
                            * entry point answers RGCN_ERR_PLAN;
                            * 5 (chunk = 64; the plan rgcn_bwd_dw_tiles walks): layout 0 with PAIRS of rows of one (destination, relation,
                            * weight) on one slot in the (tile, relation) groups of at most two chunks, see slot_src2; n_units / rel_order
                            * hold the units that are left (its rgcn_plan_build_finish synchronises the stream to count them);
                            * the heads of one relation inside one of rgcn_dw_tiles_geometry's tile ranges are then packed densely
                            * across tile boundaries: a unit may hold rows of chunk_tile (its earliest row's tile) AND of the tile
                            * after it, chunk_flags bit 28 / 29: half 0 / half 1 (slots 0..31 / 32..63) holds rows of both, bit 30:
                            * half 1 holds rows of the later tile only and half 0 of the earlier only (all three 0: one tile);
                            * rgcn_bwd_dw, rgcn_fwd and rgcn_bwd_dx answer RGCN_ERR_PLAN.
                            * Any other value, and layouts 1 / 3 with 64-slot chunks, is refused by every entry point (RGCN_ERR_PLAN) */
    int32_t chunk_rows;    /* rows a chunk may hold: = chunk, or 112 (chunk = 128: seven row tiles of rows, the eighth free for shadow
                            * rows; built by rgcn_plan_build_begin(chunk = 112)): what rgcn_tile3p_kernel's 42 KiB ring slots hold,
                            * which leaves its accumulator room for tiles up to 272.  0 is read as `chunk`; any other value is
                            * refused (RGCN_ERR_PLAN).  max(chunk_cnt) <= chunk_rows is a caller promise like every other array
                            * content: the entry points check header fields only.  The builders keep it */
    const int32_t* tile_ptr;   /* [n_tiles + 1] tile-major chunk ranges */
    const int32_t* chunk_rel;  /* [n_chunks] relation id, R' for root chunks */
    const int32_t* chunk_cnt;  /* [n_chunks] slots of the chunk's used 16-slot MFMA row tiles (16, 32, ... chunk);
                                * padding slots sit at the end of every row tile */
    const int32_t* chunk_tile; /* [n_chunks] */
    const int32_t* chunk_flags; /* [n_chunks] bit t: row tile t holds a repeated destination (needs the run-sum); layout 1: bit 8;
                                 * layout 3: bits 16-19, layout 5: bits 28-30, see `layout` */
    const int32_t* rel_order;  /* [n_units] the weight-gradient walk: non-empty 64-slot units (unit u = slots
                                * [64 u, 64 u + 64), chunk u / (chunk / 64)) sorted by (relation, tile) */
    const int32_t* slot_src;   /* [n_chunks * chunk] row to gather; padding = n_nodes (one past the last row) */
    const float* slot_w;       /* [n_chunks * chunk] edge weight 1/max(1,c[dst,rel]), 0 = padding */
    const int32_t* slot_row;   /* [n_chunks * chunk] row of the owned range the slot scatters into (tile * tile_size + row
                                * in tile), ascending inside a 16-slot row tile; padding = n_owned */
    const int32_t* slot_acc;   /* [n_chunks * chunk] forward run-sum metadata per slot: (position 0..15 in the 16-slot
                                * MFMA row tile of the slot ending this slot's run of equal destinations) << 24 |
                                * (accumulator row written); the row is the slot's row in the tile if the slot
                                * ends its run, else `tile` (dummy row) */
    const int32_t* slot_src2;  /* layout 5 only (else NULL): [n_chunks * 8] the SECOND gathered row of the slots 0..3 and 32..35 of
                                * every 64-slot unit (padding = n_nodes): rgcn_bwd_dw_tiles adds it to the slot's first row before
                                * the contraction -- two rows with one (destination, relation) and one weight on ONE slot */
} rgcn_plan_t;

int rgcn_abi_version(void);
const char* rgcn_status_string(int status);

/* ---- graph plan, built on the device ---------------------------------------------------------------------------
 * The COO the reference's Graph.init_graph produces and hands to every forward call (graphs/graph.py:55-69):
 * int64, unsorted, duplicate triples kept, forward / inverse edges interleaved.  edge_index[0] / [1] / edge_type
 * are rows of a TRANSPOSED [E, 3] tensor there, hence the element strides.  PyG rebuilds per-relation masks and
 * counts from it on every call; here it is laid out once. */
typedef struct rgcn_graph {
    const int64_t* src;  /* edge_index[0]: source j of edge j -> i */
    const int64_t* dst;  /* edge_index[1]: target i */
    const int64_t* type; /* edge_type, 0 .. num_relations - 1 */
    int64_t src_stride, dst_stride, type_stride; /* in elements */
    int64_t num_edges;
    int32_t num_nodes;
    int32_t num_relations;
} rgcn_graph_t;

/* What rgcn_plan_build_begin found: sizes of the arrays the caller allocates for rgcn_plan_build_finish. */
typedef struct rgcn_plan_sizes {
    int32_t n_tiles;  /* tile_ptr: n_tiles + 1 */
    int32_t n_chunks; /* chunk_rel / chunk_cnt / chunk_tile / chunk_flags */
    int32_t n_units;  /* rel_order */
    int32_t reserved;
    int64_t n_slots;  /* slot_src / slot_w / slot_row / slot_acc: n_chunks * chunk */
    int64_t n_edges;  /* edges placed (scatter node inside the owned range), before duplicate triples are merged */
    uint64_t opaque[16]; /* state handed from _begin to _finish */
} rgcn_plan_sizes_t;

/* Bytes of scratch for rgcn_edge_weights / rgcn_plan_build_* on a graph of num_edges edges whose plan owns n_owned
 * output nodes (0 on bad arguments).  The same workspace serves all three; it is dead after _finish. */
size_t rgcn_plan_workspace_bytes(int64_t num_edges, int32_t n_owned, int32_t num_relations, int32_t tile);

/* w[e] = 1 / max(1, c[dst_e, type_e]) for aggr = mean (c counts duplicates: PyG's scatter-mean normaliser), 1 for
 * aggr = sum (aggr_sum != 0); float32, in input edge order.  Shared by the forward and the transposed plan.
 * SYNCHRONISES the stream (reads a data-dependent count back); RGCN_ERR_GRAPH on out-of-range ids. */
int rgcn_edge_weights(const rgcn_graph_t* graph, int aggr_sum, float* w, void* workspace, size_t workspace_bytes, void* stream);

/* Plan of the edges scattering into nodes [node_begin, node_end) (node_begin a multiple of tile).
 * transposed = 0: forward plan (gather source rows, scatter into targets) for rgcn_fwd / rgcn_bwd_dw;
 * transposed = 1: the plan rgcn_bwd_dx runs on (gather target rows, scatter into sources), same weights w.
 * _begin sorts, merges duplicate triples and sizes the plan (SYNCHRONISES the stream: the sizes are data-dependent);
 * the caller then allocates the ten device arrays of `plan` (sizes above; nothing in this library allocates) and
 * _finish fills them and the scalar fields, asynchronously on `stream`.  tile: output nodes per tile (multiple of
 * 16), chunk: 64 or 128 -- or 112 (layouts 0 and 3): a plan of 128-slot chunks that hold at most 112 rows, see rgcn_plan.chunk_rows --,
 * layout: 0, 2 (chunk = 64) or (chunk = 128) 1 / 3, see struct rgcn_plan.  Replaces scaling_rgcn_training_amd/plan.py (torch tensor ops), which stays as the test
 * oracle: all arrays are bit-identical. */
int rgcn_plan_build_begin(const rgcn_graph_t* graph, const float* w, int transposed, int32_t node_begin, int32_t node_end,
                          int32_t tile, int32_t chunk, int32_t layout, void* workspace, size_t workspace_bytes,
                          rgcn_plan_sizes_t* sizes, void* stream);
int rgcn_plan_build_finish(const rgcn_plan_sizes_t* sizes, void* workspace, size_t workspace_bytes, rgcn_plan_t* plan,
                           void* stream);

/* Widths are padded to 16/32/64/128 inside the kernels; returns that padded value (0 if unsupported). */
int rgcn_padded_width(int width);

/* Floats of the MFMA-fragment-ordered weight pack: (R' + 1) * pad(K) * pad(N), plus for 64 x 64 layers the bf16 x 3 split
 * of the same weights ((R' + 1) * 6144 floats) that the split-precision kernel reads. */
size_t rgcn_packed_weight_floats(int num_relations, int din, int dout);

/* Pack weight[R', din, dout] (+ root[din, dout], may be NULL = zeros) into B-fragment order.
 * transpose = 0: B_r = W_r (K = din, N = dout), used by rgcn_fwd;
 * transpose = 1: B_r = W_r^T (K = dout, N = din), used by rgcn_bwd_dx.
 * Replaces nothing in PyG (it indexes weight[i] directly); cost O(R' * din * dout) per call. */
int rgcn_pack_weights(const float* weight, const float* root, int num_relations, int din, int dout,
                      int transpose, float* packed, void* stream);
/* The same pack for PyG's two weight decompositions (BASELINE.json configs[2]: num_bases = 30),
 * composed inside the packer -- [R', din, dout] is never materialised:
 *   basis: W_r = sum_b comp[r, b] * bases[b], bases [B, din, dout], comp [R', B]  (torch: comp @ weight.view(B, -1));
 *   block: W_r = blockdiag(blocks[r, 0 .. nb - 1]), blocks [R', nb, din / nb, dout / nb]. */
int rgcn_pack_weights_basis(const float* bases, const float* comp, const float* root, int num_relations, int num_bases,
                            int din, int dout, int transpose, float* packed, void* stream);
int rgcn_pack_weights_block(const float* blocks, const float* root, int num_relations, int num_blocks, int din, int dout,
                            int transpose, float* packed, void* stream);
/* Gradients of the decomposition's parameters from the dense d_w [R', din, dout] that rgcn_bwd_dw / rgcn_bwd_dw_tiles
 * produce (a scratch buffer, not an autograd tensor): d_bases[b] = sum_r comp[r, b] d_w[r], d_comp[r, b] = <d_w[r], bases[b]>
 * (either may be NULL); d_blocks = the diagonal blocks of d_w.  Fixed summation orders: bit-reproducible. */
int rgcn_basis_backward(const float* d_w, const float* bases, const float* comp, int num_relations, int num_bases, int din,
                        int dout, float* d_bases, float* d_comp, void* stream);
int rgcn_block_backward(const float* d_w, int num_relations, int num_blocks, int din, int dout, float* d_blocks, void* stream);

/* Forward of RGCNConv.forward (aggr mean/sum folded into the plan's edge weights):
 *   out[i, :] = act(bias + sum_{slots scattering into i} w_e * x[src_e, :] @ W_{rel_e})   (root = rel R')
 * x: [plan->n_nodes, ldx]; out: [plan->n_owned, ldo]; packed_w from rgcn_pack_weights(transpose=0);
 * bias: [dout] or NULL.  Columns dout..roundup4(dout) of out are written as zeros.
 * act: RGCN_ACT_* applied in the tile store -- what model/layers.py:22 (F.relu) and :24 (activation) run as
 * separate elementwise kernels over [N, out]. */
int rgcn_fwd(const rgcn_plan_t* plan, const float* x, int ldx, int din, const float* packed_w,
             const float* bias, float* out, int ldo, int dout, int act, unsigned flags, void* stream);

/* dX of the layer (autograd of index_select/scatter-mean/matmul in PyG's loop), atomics-free:
 *   dx[j, :] = sum_{edges j->i, r} w_e * g[i, :] @ W_r^T + g[j, :] @ root^T
 * `plan_t` is the TRANSPOSED plan (edges grouped by source); g: [plan_t->n_nodes, ldg] upstream
 * gradient; packed_wt from rgcn_pack_weights(transpose=1); dx: [plan_t->n_owned, lddx].
 * relu_of (NULL or [plan_t->n_owned, ldr], the rows of the layer INPUT that dx belongs to): when the input was
 * produced by a ReLU (the previous layer's fused RGCN_ACT_RELU), dx is stored as dx * (relu_of > 0), i.e. the
 * gradient w.r.t. the previous layer's pre-activation: autograd's relu backward never runs as a kernel. */
int rgcn_bwd_dx(const rgcn_plan_t* plan_t, const float* g, int ldg, int dout, const float* packed_wt,
                float* dx, int lddx, int din, const float* relu_of, int ldr, unsigned flags, void* stream);

/* dz = da * act'(a) for an output a = act(z) of rgcn_fwd: relu -> da * (a > 0), sigmoid -> da * a * (1 - a).
 * a, da, dz: [rows, ld] (dz may alias da).  For layers whose consumer cannot fold the mask (rgcn_bwd_dx relu_of). */
int rgcn_act_backward(const float* a, const float* da, float* dz, long rows, int ld, int act, void* stream);

/* Weight gradients: d_weight[r] = H_r^T g, d_root = X^T g, d_bias = column sums of g, over the
 * plan's owned rows (g: [plan->n_owned, ldg] is the upstream gradient of those rows).
 * Any of d_weight / d_root / d_bias may be NULL (frozen parameter, model/layers.py:33-46).
 * Deterministic: per-workgroup partial slabs in `workspace` are summed in a fixed order. */
size_t rgcn_bwd_dw_workspace_bytes(const rgcn_plan_t* plan, int din, int dout);
int rgcn_bwd_dw(const rgcn_plan_t* plan, const float* x, int ldx, int din, const float* g, int ldg,
                int dout, void* workspace, size_t workspace_bytes, float* d_weight, float* d_root,
                float* d_bias, unsigned flags, void* stream);

/* d_weight alone, tile-major (64 x 64 layers with at most 32 relations on large graphs): every wave owns one relation and
 * keeps its 64 x 64 accumulator in registers for the whole launch, the upstream-gradient rows of a tile are staged in LDS
 * once per relation quarter instead of being gathered per edge (37 GB instead of 55 GB moved at the headline config).
 * `plan`: a FORWARD-direction plan built with the geometry rgcn_dw_tiles_geometry reports (tile = 320, chunk = 64, layout
 * 0); walk_ptr: int32 [num_relations][walkers + 1], walk_ptr[r][p] = first position in plan->rel_order of relation r
 * whose tile is >= p * n_tiles / walkers (integer division), walk_ptr[r][walkers] = end of relation r; filled by
 * rgcn_dw_tiles_walk (once per plan; walk_ptr: device memory, num_relations * (walkers + 1) int32).
 * d_root / d_bias: rgcn_bwd_dw(..., RGCN_FLAG_DW_ROOT_ONLY) on any forward plan of the same graph. */
int rgcn_dw_tiles_geometry(int* tile, int* walkers, int* max_relations);
int rgcn_dw_tiles_walk(const rgcn_plan_t* plan, int32_t* walk_ptr, void* stream);
size_t rgcn_bwd_dw_tiles_workspace_bytes(int num_relations);
int rgcn_bwd_dw_tiles(const rgcn_plan_t* plan, const int32_t* walk_ptr, const float* x, int ldx, int din, const float* g,
                      int ldg, int dout, void* workspace, size_t workspace_bytes, float* d_weight, unsigned flags,
                      void* stream);

/* d_root = x^T g and d_bias = column sums of g over rows [0, rows) of the two matrices -- the self-loop ("root") part of
 * autograd's backward of RGCNConv (reference model/modelTrainer.py:66), which needs no plan: the rows the root relation
 * "gathers" are the nodes' own.  Widths up to 64 per side (RGCN_ERR_WIDTH beyond: use rgcn_bwd_dw with
 * RGCN_FLAG_DW_ROOT_ONLY).  A streaming kernel without LDS whose workgroups fit a CU next to rgcn_bwd_dx's: enqueue it on a
 * second stream beside the dX launch.  d_root or d_bias may be NULL (not both).  Bit-reproducible.  The kernel is the one
 * behind rgcn_rows_dw (csrc/rgcn_dw_root.hip), here on one 64 x 64 output with the bias sums: where both entry points cut the
 * rows into the same ranges their products agree bit for bit.  A row count whose share per wave cannot be addressed with
 * 32-bit offsets is RGCN_ERR_STRIDE. */
size_t rgcn_bwd_dw_root_workspace_bytes(void);
int rgcn_bwd_dw_root(const float* x, int ldx, int din, const float* g, int ldg, int dout, long rows, void* workspace,
                     size_t workspace_bytes, float* d_root, float* d_bias, void* stream);

/* ---- edge-parallel path (scaling_rgcn_training_amd/eplan.py) ---------------------------------------------------
 * The same layer arithmetic for graphs on which the tile-major plan is the wrong shape -- the reference's own datasets
 * (model/modelTrainer.py:78,92: 45 .. ~267 relation ids, hubs of in-degree 10^4 on 8k nodes): rows (merged edges + one
 * root pseudo edge per node) sorted RELATION-MAJOR and packed into dense 64-slot units; rgcn_ep_transform writes
 * Z[slot] = w_slot * (x[src_slot] @ W_rel) for every slot, rgcn_ep_segment_sum adds the rows of every destination in a
 * fixed order and applies bias / activation / ReLU mask.  dX: the same two calls on the transposed units with W^T.
 * The units double as a dense relation-major walk for rgcn_bwd_dw (a rgcn_plan_t with layout = 2, chunk = 64, rel_order
 * = 0 .. n_units - 1, chunk_rel / chunk_cnt = unit_rel / unit_cnt: rgcn_fwd / rgcn_bwd_dx refuse it). */
typedef struct rgcn_edge_units {
    int32_t n_nodes;           /* rows of the gathered matrix (padding slots gather row n_nodes -> zeros) */
    int32_t n_units;           /* 64-slot units */
    int32_t num_relations;     /* R' (the root pseudo relation is id R') */
    int32_t reserved;
    const int32_t* unit_rel;   /* [n_units] relation of the unit, ascending */
    const int32_t* unit_cnt;   /* [n_units] used slots rounded up to 16 (whole MFMA row tiles): 16 .. 64 */
    const int32_t* slot_src;   /* [n_units * 64] */
    const float* slot_w;       /* [n_units * 64] edge weight, 0 = padding */
} rgcn_edge_units_t;

/* The unit arrays come from the plan builder itself: rgcn_plan_build_begin / _finish with layout = 2, chunk = 64 (tile is
 * ignored) lay the owned range out as ONE tile, i.e. relation-major: chunk_rel / chunk_cnt are unit_rel / unit_cnt, slot_src /
 * slot_w the slots, slot_row the destination row of every slot (n_owned = padding), rel_order = 0 .. n_units - 1 -- the same
 * rgcn_plan_t is what rgcn_bwd_dw walks.  rgcn_eplan_segments then sorts the slots by destination: seg_idx [n_slots] (its first
 * seg_ptr[n_owned] entries are the real slots ordered by (destination row, slot)), seg_ptr [n_owned + 1].  Workspace:
 * rgcn_plan_workspace_bytes(n_slots, 0, 1, 16).  Destinations with more than a few hundred rows are summed in levels: cut
 * [seg_ptr[i], seg_ptr[i + 1]) into pieces of at most P rows (scaling_rgcn_training_amd/eplan.py segment_levels, P = 256). */
int rgcn_eplan_segments(const int32_t* slot_row, int64_t n_slots, int32_t n_owned, void* workspace, size_t workspace_bytes,
                        int32_t* seg_ptr, int32_t* seg_idx, void* stream);
/* z: [n_units * 64, ldz] (rows of unused row tiles are left untouched); packed_w: rgcn_pack_weights(..., transpose).
 * flags & RGCN_FLAG_SPLIT_PRODUCERS: 64 x 64 layers multiply on bf16 MFMAs over three-way split operands (fp32-equivalent, as
 * rgcn_fwd under the same flag): the exact-fp32 MFMA rate binds the transform at that width. */
int rgcn_ep_transform(const rgcn_edge_units_t* units, const float* x, int ldx, int din, const float* packed_w, float* z,
                      int ldz, int dout, unsigned flags, void* stream);
/* out[i] = sum of rows seg_idx[q] (q itself when seg_idx is NULL) of `in` -- times seg_w[q] when seg_w is given -- for q in
 * [seg_ptr[i], seg_ptr[i + 1]), i < n_out, added in index order; final_level != 0: + bias (may be NULL), activation (RGCN_ACT_*), then out *= (mask > 0) when mask
 * is given (rows of the layer input when it is a ReLU output, as rgcn_bwd_dx's relu_of).  Long segments are summed in
 * levels: pieces first (final_level = 0, seg_idx of the first level only), the pieces of a segment last. */
int rgcn_ep_segment_sum(const float* in, int ldin, const int32_t* seg_ptr, const int32_t* seg_idx, const float* seg_w, int n_out,
                        int width, const float* bias, int act, const float* mask, int ldm, int final_level, float* out, int ldo,
                        void* stream);

/* ---- max aggregation (RGCNConv(aggr="max"); scaling_rgcn_training_amd/csrc/rgcn_segmax.hip, eplan.py MaxPlan) ---------------
 * PyG 2.3.1 with aggr="max": H_r[i] = max over the edges e into i of relation r of x[src_e] (torch scatter_reduce "amax",
 * include_self = 0: all-negative rows give a negative max), out[i] = sum_r H_r[i] W_r + x[i] root + bias.  Every (destination,
 * relation) segment is a heavy segment of the edge-parallel plan: its rows are reduced by rgcn_segment_max, its pseudo row goes
 * through rgcn_ep_transform and rgcn_ep_segment_sum as a sum layer's would.
 * rgcn_segment_max: out[i] = max of rows seg_idx[q] (q itself when seg_idx is NULL) of `in` over q in [seg_ptr[i], seg_ptr[i + 1]),
 * per column; an empty segment gives 0.  out_t (may be NULL) [n_out, ldo]: the TIE WEIGHT of every column, the sum over the
 * rows equal to the max (-0 == +0) of their weight -- seg_w[q] (1 when seg_w is NULL), times in_t[row] when in_t is given.  Long
 * segments are reduced in levels as with rgcn_ep_segment_sum: level 0 over the gathered rows with in_t = NULL, each further
 * level over the (out, out_t) of the level before (in_t = its out_t, seg_idx = seg_w = NULL); equal maxima add their weights, so
 * both outputs are the same for every cut.  A NaN in a column makes its max NaN (its tie weight is unspecified).  in and in_t
 * share the stride ldin, out and out_t the stride ldo.
 * rgcn_segment_max_bwd: for q < n_rows, c[q] = (x[row_src[q]] == h[s]) * row_w[q] * dh[seg_dh[s]] / n[s] per column, s =
 * row_seg[q], n = t + (h == 0 ? 1 : 0) (row_w NULL: 1; seg_dh NULL: dh[s]; n == 0: 0) -- the gradient of a max split evenly
 * among the rows that attain it, as torch's scatter_reduce "amax" backward splits it: with include_self = 0 torch still counts
 * the zero its output starts from as one more tie when the max is exactly 0.  rgcn_ep_segment_sum then adds c per source.  h
 * and t share the stride ldh.
 * Both: widths 1..128, no workspace, no atomics, fixed orders (bit-reproducible); rows addressed with 64-bit offsets.  Inputs
 * hold zeros in their pad columns [width, roundup4(width)) (the rule of every operand); out, out_t and c are written as +0.0
 * there (out_t too: the zeros of the inputs' pad columns all tie, and their count is not part of the tie weights). */
int rgcn_segment_max(const float* in, const float* in_t, int ldin, const int32_t* seg_ptr, const int32_t* seg_idx,
                     const float* seg_w, int n_out, int width, float* out, float* out_t, int ldo, void* stream);
int rgcn_segment_max_bwd(const float* x, int ldx, const float* h, const float* t, int ldh, const float* dh, int lddh,
                         const int32_t* row_src, const int32_t* row_seg, const int32_t* seg_dh, const float* row_w,
                         int64_t n_rows, int width, float* c, int ldc, void* stream);

/* ---- featureless layers (scaling_rgcn_training_amd/csrc/rgcn_featureless.hip) -----------------------------------------------
 * PyG's RGCNConv with x = None or an int64 node-index vector: the weight tables are per-node embeddings,
 *   out[i] = bias + root[x_i] + sum_{slots j -> i} w_e * W_{rel}[x_j]     (x_index NULL: x_j = j, and in_rows = plan->n_nodes)
 * weight: full [R', in_rows, dout] (comp NULL, num_bases 0) or bases [B, in_rows, dout] with comp [R', B]: W_r = sum_b comp[r, b] V_b,
 * composed per gathered row ([R', in_rows, dout] is never formed).  Tables have row stride dout (any dout in 1..128) and are
 * addressed with 64-bit offsets.  Plans: layout 0 over the whole node range (n_owned = n_nodes), chunk 64 or 128, tile from
 * rgcn_featureless_geometry; layouts 1 / 2 / 3 / 5 answer RGCN_ERR_PLAN.  x_index values outside [0, in_rows) read zeros (the
 * Python host refuses them once per index vector).  Deterministic: fixed summation orders, no atomics. */
/* (tile, chunk) of the featureless plans of a graph of n_nodes nodes; RGCN_ERR_LDS when B bases of that width do not fit */
int rgcn_featureless_geometry(int32_t n_nodes, int dout, int num_bases, int* tile, int* chunk);
/* out: [plan->n_nodes, ldo], columns dout .. roundup4(dout) written as zeros; root / bias may be NULL (zeros). */
int rgcn_featureless_fwd(const rgcn_plan_t* plan, const int64_t* x_index, int64_t in_rows, const float* weight, const float* comp,
                         int num_bases, const float* root, const float* bias, float* out, int ldo, int dout, void* stream);
/* Gradients from g [plan_t->n_nodes, ldg] on the TRANSPOSED plan: d_weight [R', in_rows, dout] (every row written, zeros where no
 * edge gathers it), or with bases d_weight = d_bases [B, in_rows, dout] and d_comp [R', B]; d_root [in_rows, dout]; d_bias [dout].
 * Any of them may be NULL.  x_index given: inv_ptr [in_rows + 1] / inv_idx [n_nodes] is its inverted index (the node ids sorted by
 * x value, inv_ptr[v] the first of value v); the per-node rows go through `workspace` and are summed per value in index order.
 * indexed != 0 in the query: the size for an x_index call. */
size_t rgcn_featureless_bwd_workspace_bytes(const rgcn_plan_t* plan_t, int dout, int num_bases, int indexed);
int rgcn_featureless_bwd(const rgcn_plan_t* plan_t, const int64_t* x_index, const int32_t* inv_ptr, const int32_t* inv_idx,
                         int64_t in_rows, const float* g, int ldg, int dout, const float* weight, const float* comp, int num_bases,
                         void* workspace, size_t workspace_bytes, float* d_weight, float* d_comp, float* d_root, float* d_bias,
                         void* stream);

/* ---- layers wider than 128 (scaling_rgcn_training_amd/csrc/rgcn_xwide.hip) ---------------------------------------------------
 * The same layer arithmetic as rgcn_fwd / rgcn_bwd_dx / rgcn_bwd_dw (exact fp32 MFMAs) for 1..RGCN_XWIDE_MAX_WIDTH features per
 * side; narrower widths are accepted too.  Plans: layout 0, chunk 64 or 128 (rows = chunk), from rgcn_plan_build_* at the
 * geometry below; layouts 1 / 2 / 3 / 5 answer RGCN_ERR_PLAN.  The weight operand is caller-owned and plain row-major
 * fp32 [R' + 1, K, N]: block r at r * K * N, the root last (zeros when the layer has none):
 *   forward: K = din, N = dout, block r = W_r;      dX: K = dout, N = din, block r = W_r^T.
 * Rows are addressed with 64-bit offsets (no 4 GiB / 2^24-row limit).  Deterministic: fixed summation orders, no atomics.  The
 * entry points take no flags. */
/* (tile, chunk) of the forward and transposed plans of a layer din -> dout on a graph of n_nodes nodes (160 KiB of LDS) */
int rgcn_xwide_geometry(int32_t n_nodes, int din, int dout, int* tile, int* chunk);
/* out[i] = act(bias + sum_{slots -> i} w_e * x[src_e] @ W_rel) as rgcn_fwd; x [plan->n_nodes, ldx], out [plan->n_owned, ldo],
 * columns dout .. roundup4(dout) of out written as zeros; bias [dout] or NULL; act RGCN_ACT_*. */
int rgcn_xwide_fwd(const rgcn_plan_t* plan, const float* x, int ldx, int din, const float* weight, const float* bias, float* out,
                   int ldo, int dout, int act, void* stream);
/* dX on the TRANSPOSED plan with the transposed operand, as rgcn_bwd_dx (relu_of: NULL or [plan_t->n_owned, ldr]). */
int rgcn_xwide_bwd_dx(const rgcn_plan_t* plan_t, const float* g, int ldg, int dout, const float* weight_t, float* dx, int lddx,
                      int din, const float* relu_of, int ldr, void* stream);
/* d_weight [R', din, dout], d_root [din, dout], d_bias [dout] on the FORWARD plan, as rgcn_bwd_dw; any of them may be NULL.
 * Partial slabs in `workspace` are summed in a fixed order.  The query answers 0 on bad arguments. */
size_t rgcn_xwide_bwd_dw_workspace_bytes(const rgcn_plan_t* plan, int din, int dout);
int rgcn_xwide_bwd_dw(const rgcn_plan_t* plan, const float* x, int ldx, int din, const float* g, int ldg, int dout, void* workspace,
                      size_t workspace_bytes, float* d_weight, float* d_root, float* d_bias, void* stream);

/* ---- bipartite layers: the root term (csrc/rgcn_rows.hip, rgcn_rows_dw: csrc/rgcn_dw_root.hip) ------------------
 * RGCNConv with x = (x_src, x_dst) (PyG 2.3.1): `root` is [in_dst, out] and multiplies x_dst, whose rows pair up one to one
 * with the output rows -- a different matrix of a different width than the rows the plans gather, so the plans' root relation
 * is packed as zeros and the term and its two gradients are dense, plan-free products over rows.  Widths 1..128 per side
 * (RGCN_ERR_WIDTH), strides multiples of 4 and at least the width rounded up to 4 (RGCN_ERR_STRIDE), pad columns of the inputs
 * zero; every argument check is answered without a device.  Exact fp32, no atomics, fixed summation orders: bit-reproducible.
 * Row offsets are 64-bit: rows x ld may pass 2^31.
 *
 * rgcn_rows_transform: y[i, :] = add[i, :] + x[i, :] @ W + bias, i < rows.
 *   x [rows, ldx], din columns.
 *   transpose == 0: w is row-major [din, dout] and W = w.
 *   transpose != 0: w is row-major [dout, din] and W = w^T (d_x = g @ root^T reads root itself).
 *   add: NULL (zeros), or [rows, lda]; add may alias y.
 *   bias: NULL or [dout].
 *   Columns dout..roundup4(dout) of y are written as +0.0.  rows == 0 touches nothing.
 * rgcn_rows_dw: d_w [din, dout] (dense, no padding) = x^T g over rows [0, rows).  rows == 0 writes zeros (x and g may then be NULL).
 *   The streaming kernel of rgcn_bwd_dw_root with the output cut into quadrants of 64 x 64, one per wave, and no bias sums.
 *   Per-wave partial slabs in `workspace` (the query answers 0 on bad widths), summed in a fixed order.  A row count whose
 *   share per wave cannot be addressed with 32-bit offsets (beyond 2^31 rows at 128 columns) is RGCN_ERR_STRIDE. */
int rgcn_rows_transform(const float* x, int ldx, int din, const float* w, int transpose, const float* add, int lda,
                        const float* bias, float* y, int ldy, int dout, long rows, void* stream);
size_t rgcn_rows_dw_workspace_bytes(int din, int dout);
int rgcn_rows_dw(const float* x, int ldx, int din, const float* g, int ldg, int dout, long rows, void* workspace,
                 size_t workspace_bytes, float* d_w, void* stream);

/* ---- graph summaries: k-bisimulation node partitions and quotient graphs (csrc/rgcn_summary.hip) --------------
 * The step that makes the summary graphs the method trains on first, on the same strided int64 COO (struct rgcn_graph) the
 * plan builder takes.  A partition is an int32 block id per node.  One refinement round maps a partition b to b':
 * b'[i] == b'[j] iff b[i] == b[j] and S(i) == S(j), where S is a SET (duplicates and order ignored) over the node's edges:
 *   RGCN_DIR_OUT:    S(i) = {(type_e, b[dst_e]) : src_e = i}
 *   RGCN_DIR_IN:     S(i) = {(type_e, b[src_e]) : dst_e = i}
 *   RGCN_DIR_IN_OUT: S(i) = {(0, type_e, b[dst_e]) : src_e = i} u {(1, type_e, b[src_e]) : dst_e = i}
 * b' is numbered canonically: ids 0 .. B' - 1 in the order of the smallest node of every block.  From the all-zero partition
 * round 1 is the reference's attribute summary over relation ids (graphs/createAttributeSum.py), rounds 2 .. k the
 * k-bisimulation; a round that returns B' == B (B the number of DISTINCT ids in b) changed nothing: the fixpoint.
 * Sets are compared through 128-bit signatures (sums of two 64-bit mixes per distinct element, the node's own block folded
 * in); block ids do not depend on the hash.  Limits: num_relations <= 65536, num_edges (twice that for RGCN_DIR_IN_OUT)
 * <= 0xFFFF0000 (RGCN_ERR_PLAN beyond).  Both entry points SYNCHRONISE the stream once, to read one data-dependent count back
 * into the HOST pointer they take last but one; they allocate nothing.  An edge_index / edge_type value out of range, or a
 * block id outside [0, num_blocks), is RGCN_ERR_GRAPH (found on the device: outputs are then unspecified, nothing is written
 * outside them).  route: 0 = the library chooses; 1 = one stable sort over a single packed 64-bit key (RGCN_ERR_PLAN when the
 * fields do not fit 64 bits); 2 = two stable sorts (always possible; what route 0 falls back to). */
enum rgcn_summary_direction { RGCN_DIR_OUT = 0, RGCN_DIR_IN = 1, RGCN_DIR_IN_OUT = 2 };

/* Bytes of scratch for rgcn_summary_round on num_edges edges and num_nodes nodes in `direction` (0 on bad arguments);
 * rgcn_summary_quotient needs the RGCN_DIR_OUT size.  A larger workspace serves a smaller call. */
size_t rgcn_summary_workspace_bytes(int64_t num_edges, int32_t num_nodes, int direction);

/* One refinement round.  block_in [num_nodes] with ids in [0, num_blocks_in), num_blocks_in >= 1 (the ids need not be
 * canonical nor all in use: num_blocks_in only sizes the key field); block_out [num_nodes] (may alias block_in);
 * *num_blocks_out (host) = B'.  A graph without edges is allowed (src / dst / type may then be NULL): the call then numbers
 * block_in canonically. */
int rgcn_summary_round(const rgcn_graph_t* graph, int direction, const int32_t* block_in, int32_t num_blocks_in, int route,
                       int32_t* block_out, void* workspace, size_t workspace_bytes, int32_t* num_blocks_out, void* stream);

/* The quotient graph of a partition: the distinct (block[src], type, block[dst]) triples sorted by (type, block[dst],
 * block[src]), with the number of edges behind each.  src_out / dst_out / type_out / mult_out: int64 [num_edges] each (the
 * worst case; may be NULL when num_edges == 0), of which the first *num_edges_out (host) are written. */
int rgcn_summary_quotient(const rgcn_graph_t* graph, const int32_t* block, int32_t num_blocks, int route, int64_t* src_out,
                          int64_t* dst_out, int64_t* type_out, int64_t* mult_out, void* workspace, size_t workspace_bytes,
                          int64_t* num_edges_out, void* stream);

/* ---- neighbour sampling: the in-edge index and one fan-out hop (csrc/rgcn_sample.hip) ----------------------------
 * What makes the (x_src, x_dst) blocks a mini-batch step walks, on the same strided int64 COO (struct rgcn_graph).
 * Index: the edges sorted stably by destination; ptr[v] .. ptr[v + 1] are the in-edges of v in input order (duplicate triples stay
 * distinct in-edges), src / type the sorted edges' sources and relations.  Limits: num_edges <= 0xFFFF0000, num_relations <= 65536
 * (RGCN_ERR_PLAN beyond).
 * Hop: for destination v = dst_nodes[i] (unique, in [0, num_nodes)) with in-degree d: fanout == -1 or d <= fanout takes all d
 * in-edges, otherwise a uniform fanout-subset of the positions 0 .. d-1 by Floyd's algorithm (S = {}; for j = d-k .. d-1:
 * t = draw(j); add j if t is in S, else t) on a counter-based generator, arithmetic mod 2^64:
 *   mix(z):  z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31
 *   key      = mix(seed + 0x9E3779B97F4A7C15 * (hop + 1))
 *   r        = mix(mix(key + v) + j)
 *   draw(j)  = ((r >> 32) * (j + 1)) >> 32
 * so the choice depends on (seed, hop, v) alone.  The block: src_nodes = dst_nodes followed by the ascending distinct sampled
 * sources that are no destination; edges ordered by destination position, then by ascending in-edge position, relabelled to
 * positions in src_nodes (edge_src) and in dst_nodes (edge_dst).  A pure function of its arguments.
 * cap, the most edges a block can hold: num_edges for fanout == -1, else min(num_edges, num_dst * fanout).
 * Both calls allocate nothing and SYNCHRONISE the stream once: the index build to read its error word, the hop to read the error
 * word, E_b and n_src back.  An edge_index / edge_type value or a destination out of range is RGCN_ERR_GRAPH, a destination listed
 * twice RGCN_ERR_ARG (both found on the device: outputs are then unspecified, nothing is written outside them, node_map is reset);
 * a fan-out outside {-1} u [1, 256], seed < 0, hop < 0, num_dst < 0 or > num_nodes: RGCN_ERR_ARG, answered before any launch. */
typedef struct rgcn_sample_index {
    const uint32_t* ptr;   /* [num_nodes + 1] */
    const int32_t* src;    /* [num_edges] (may be NULL when num_edges == 0) */
    const int32_t* type;   /* [num_edges] */
    int64_t num_edges;
    int32_t num_nodes;
    int32_t num_relations;
} rgcn_sample_index_t;

/* Bytes of scratch for rgcn_sample_index_build / rgcn_sample_hop (0 on bad arguments).  A larger workspace serves a smaller call. */
size_t rgcn_sample_index_workspace_bytes(int64_t num_edges, int32_t num_nodes);
size_t rgcn_sample_hop_workspace_bytes(int64_t num_dst, int fanout, int64_t num_edges, int32_t num_nodes);

/* ptr_out [num_nodes + 1], src_out / type_out [num_edges] (may be NULL when num_edges == 0). */
int rgcn_sample_index_build(const rgcn_graph_t* graph, uint32_t* ptr_out, int32_t* src_out, int32_t* type_out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* One hop.  node_map [num_nodes]: the caller's persistent scratch, every entry 0xFFFFFFFF on entry; the call writes the entries of
 * the block's nodes and resets exactly those before it returns.  edge_src_out / edge_dst_out / edge_type_out: int64 [cap] each,
 * src_nodes_out: int64 [num_dst + min(cap, num_nodes)]; the first *num_edges_out / *num_src_out (host) entries are written.
 * num_dst == 0 is an empty block and launches nothing. */
int rgcn_sample_hop(const rgcn_sample_index_t* index, const int64_t* dst_nodes, int64_t num_dst, int fanout, int64_t seed, int hop,
                    uint32_t* node_map, int64_t* edge_src_out, int64_t* edge_dst_out, int64_t* edge_type_out, int64_t* src_nodes_out,
                    void* workspace, size_t workspace_bytes, int64_t* num_edges_out, int64_t* num_src_out, void* stream);

/* ---- neighbour sampling with one fan-out PER RELATION (csrc/rgcn_sample.hip) ------------------------------------
 * RGCNConv normalises per (destination, relation), so the sampling unit here is the RUN: the in-edges of one destination v with
 * one relation t.  Additions to the calls above, which are unchanged; RGCN_ABI_VERSION stays.
 * Relation index: the edges sorted stably by (destination, relation); a run is the maximal group of sorted edges with one (v, t),
 * its edges in input order (duplicate triples stay distinct).  run_ptr[v] .. run_ptr[v + 1] are the runs of v, ascending in t;
 * run_beg[q] .. run_beg[q + 1] the positions of run q in the sorted edge list, run_type[q] its relation; src the sorted edges'
 * sources.  Limits as above: num_edges <= 0xFFFF0000, num_relations <= 65536 (RGCN_ERR_PLAN beyond).
 * Hop: fanouts is a HOST array of num_relations entries, each in {-1, 0} u [1, 256]: -1 takes a run whole, 0 takes nothing of
 * that relation.  A run of length d of destination v and relation t is taken whole when fanouts[t] == -1 or d <= fanouts[t],
 * otherwise a uniform fanouts[t]-subset of its positions 0 .. d-1 by the Floyd loop above, the generator keyed per relation too:
 *   key      = mix(seed + 0x9E3779B97F4A7C15 * (hop + 1))
 *   kv       = mix(mix(key + v) + 0xD1B54A32D192ED03 * (t + 1))
 *   r        = mix(kv + j);   draw(j) = ((r >> 32) * (j + 1)) >> 32
 * so the choice depends on (seed, hop, v, t) alone -- not on the batch, not on the other entries of fanouts.  The block:
 * src_nodes as above; edges ordered by destination position, then relation, then ascending position in the run.
 * cap, the most edges a block can hold: num_edges if any entry is -1, else min(num_edges, num_dst * sum of the positive entries).
 * Both calls allocate nothing and synchronise the stream once.  Errors as above: an id or a destination out of range
 * RGCN_ERR_GRAPH, a destination listed twice RGCN_ERR_ARG (found on the device: outputs unspecified, nothing written outside them,
 * node_map reset); a fan-out entry outside its domain, seed < 0, hop < 0, num_dst < 0 or > num_nodes: RGCN_ERR_ARG before any
 * launch. */
typedef struct rgcn_sample_rel_index {
    const uint32_t* run_ptr;   /* [num_nodes + 1] */
    const uint32_t* run_beg;   /* [num_runs + 1] */
    const int32_t* run_type;   /* [num_runs] (may be NULL when num_edges == 0) */
    const int32_t* src;        /* [num_edges] (may be NULL when num_edges == 0) */
    int64_t num_edges;
    int64_t num_runs;
    int32_t num_nodes;
    int32_t num_relations;
} rgcn_sample_rel_index_t;

/* Bytes of scratch (0 on bad arguments, a fan-out entry outside its domain included). */
size_t rgcn_sample_rel_index_workspace_bytes(int64_t num_edges, int32_t num_nodes);
size_t rgcn_sample_hop_rel_workspace_bytes(int64_t num_dst, const int32_t* fanouts, int32_t num_relations, int64_t num_edges,
                                           int64_t num_runs, int32_t num_nodes);

/* run_ptr_out [num_nodes + 1]; run_beg_out [num_edges + 1] and run_type_out [num_edges] (the worst case: every edge a run of its
 * own), of which num_runs + 1 / num_runs entries are written; src_out [num_edges]; *num_runs_out (host).  run_type_out / src_out
 * may be NULL when num_edges == 0. */
int rgcn_sample_rel_index_build(const rgcn_graph_t* graph, uint32_t* run_ptr_out, uint32_t* run_beg_out, int32_t* run_type_out,
                                int32_t* src_out, void* workspace, size_t workspace_bytes, int64_t* num_runs_out, void* stream);

/* One hop; node_map and the outputs as rgcn_sample_hop, sized by this call's cap. */
int rgcn_sample_hop_rel(const rgcn_sample_rel_index_t* index, const int64_t* dst_nodes, int64_t num_dst, const int32_t* fanouts,
                        int64_t seed, int hop, uint32_t* node_map, int64_t* edge_src_out, int64_t* edge_dst_out,
                        int64_t* edge_type_out, int64_t* src_nodes_out, void* workspace, size_t workspace_bytes,
                        int64_t* num_edges_out, int64_t* num_src_out, void* stream);

/* ---- mini-batch layers: a bipartite R-GCN layer straight from a sampled block (csrc/rgcn_minibatch.hip) ----------
 * ("block" in this header already means block-diagonal weights: hence rgcn_mb_.)  For a block of E_b edges (strided int64 src /
 * dst / type, src in [0, n_src), dst in [0, n_dst), type in [0, R)) whose destinations are its first n_dst source rows
 * (n_dst <= n_src) and x [n_src, in]:  out[i] = bias + x[i] root + sum_r aggregate over the edges of relation r into i of x[src] W_r,
 * mean (divided by the number of edges of the (destination, relation) pair, duplicates counted) or sum.  No graph plan: ONE index
 * per block serves forward, dX and d_weight.  No order is required of the edges.
 * Index.  The root is relation R with one pseudo edge i -> i per destination: M = E_b + n_dst edges, sorted stably by (relation,
 * destination); everything below refers to POSITIONS in that order.  A run of equal (relation, destination) is cut into rows of at
 * most 256 consecutive positions, each with scale = 1 / run length (mean) or 1 (sum).  Rows lie relation-major in tiles of 16 row
 * slots that never straddle a relation: the tiles of relation r are tile_ptr[r] .. tile_ptr[r + 1], its rows fill their slots from
 * the first on, the slots left over in its last tile are empty (row_cnt == 0, row_scale == 0).  n_tiles = tile_ptr[R + 1]; row
 * slot = 16 * tile + (0 .. 15).
 *   edge_src [M]            source of every position
 *   row_beg / row_cnt       [16 n_tiles] first position and number of positions (1 .. 256; 0: empty) of a slot's row
 *   row_dst / row_scale     [16 n_tiles] its destination and scale
 *   dst_ptr [n_dst + 1], dst_rows [n_rows]   the row slots of every destination, ascending relation within it
 *   src_ptr [n_src + 1], src_row / src_scale [M]   row slot and scale of every position, grouped by source, ascending position
 * Limits: n_src, n_dst < 2^31, E_b + n_dst <= 0xFFFF0000, R <= 65536, 16 (M / 16 + R + 1) < 2^32, widths 1..128: RGCN_ERR_PLAN
 * beyond; negative counts or n_dst > n_src: RGCN_ERR_ARG; an id out of range (found on the device): RGCN_ERR_GRAPH.  A refused
 * call launches nothing.
 * The build allocates nothing and SYNCHRONISES the stream once, to read the error word, the row count and the tile count back;
 * the three layer calls are asynchronous.  No float atomics: the same block and inputs give the same bits. */
typedef struct rgcn_mb_index {
    const int32_t* tile_ptr;   /* [num_relations + 2] */
    const uint32_t* row_beg;   /* [16 n_tiles] */
    const int32_t* row_cnt;
    const int32_t* row_dst;
    const float* row_scale;
    const int32_t* edge_src;   /* [num_edges + n_dst] */
    const uint32_t* dst_ptr;   /* [n_dst + 1] */
    const uint32_t* dst_rows;  /* [n_rows] */
    const uint32_t* src_ptr;   /* [n_src + 1] */
    const uint32_t* src_row;   /* [num_edges + n_dst] */
    const float* src_scale;
    int64_t num_edges;         /* E_b */
    int64_t n_rows;            /* non-empty row slots */
    int32_t n_src, n_dst, num_relations;
    int32_t mean;              /* 1: mean, 0: sum */
    int32_t n_tiles;
    int32_t reserved;
} rgcn_mb_index_t;

/* Bytes of the index arena / of the build's scratch (0 on arguments the build would refuse).  Larger buffers serve. */
size_t rgcn_mb_index_bytes(int64_t num_edges, int64_t n_src, int64_t n_dst, int32_t num_relations);
size_t rgcn_mb_index_workspace_bytes(int64_t num_edges, int64_t n_src, int64_t n_dst, int32_t num_relations);

/* Builds the index into the caller's arena `index_mem` and fills *index_out (host) with pointers into it and the counts.  src / dst /
 * type may be NULL when num_edges == 0.  n_dst == 0 (then num_edges must be 0) gives an index without tiles and reads nothing back. */
int rgcn_mb_index_build(const int64_t* src, int64_t src_stride, const int64_t* dst, int64_t dst_stride, const int64_t* type,
                        int64_t type_stride, int64_t num_edges, int64_t n_src, int64_t n_dst, int32_t num_relations, int mean,
                        void* index_mem, size_t index_bytes, void* workspace, size_t workspace_bytes, rgcn_mb_index_t* index_out,
                        void* stream);

/* Forward.  packed_w: rgcn_pack_weights* of the layer (relation R = root, zeros without one).  h [16 n_tiles][ldh] receives the
 * aggregated rows (keep it for rgcn_mb_bwd_dw), z [16 n_tiles][ldz] their products, out [n_dst][ldo] the layer output; bias
 * [out] or NULL.  n_dst == 0 launches nothing. */
int rgcn_mb_fwd(const rgcn_mb_index_t* index, const float* x, int ldx, int din, const float* packed_w, const float* bias, float* h,
                int ldh, float* z, int ldz, float* out, int ldo, int dout, void* stream);

/* dX [n_src][lddx] from g [n_dst][ldg] = dL/d out: the root's g root^T included in the first n_dst rows, zeros in rows no edge
 * reads.  packed_wt: the transposed pack.  dh [16 n_tiles][lddh]: scratch. */
int rgcn_mb_bwd_dx(const rgcn_mb_index_t* index, const float* g, int ldg, int dout, const float* packed_wt, float* dh, int lddh,
                   float* dx, int lddx, int din, void* stream);

/* d_weight [R][din][dout] (dense) and d_root [din][dout], either may be NULL, from the forward's h.  A relation's tiles are cut
 * into a number of slabs fixed by (n_tiles, R, din, dout) and the slabs added in order; the query gives the slabs' bytes (0: none). */
size_t rgcn_mb_bwd_dw_workspace_bytes(const rgcn_mb_index_t* index, int din, int dout);
int rgcn_mb_bwd_dw(const rgcn_mb_index_t* index, const float* h, int ldh, int din, const float* g, int ldg, int dout, float* d_weight,
                   float* d_root, void* workspace, size_t workspace_bytes, void* stream);

/* ---- sparse embedding rows: a row-wise Adam step on the rows a mini-batch gathered (csrc/rgcn_emb_rows.hip) -------
 * table / exp_avg / exp_avg_sq: `planes` planes of [num_nodes][ld] floats, plane_stride ELEMENTS apart (planes = 1: an nn.Embedding
 * weight; planes = S: a stacked [S, N, emb] parameter); row_step [num_nodes]: the steps every row has taken, shared by the planes.
 * nodes [n_rows]: int64 node ids; grad: `planes` planes of [n_rows][ldg], grad_plane_stride elements apart: one gradient row per
 * position of `nodes`.  For every node n that `nodes` lists:
 *   g = the sum of the gradient rows of every position that lists n, added in ascending position order;  g += weight_decay * p
 *   t = ++row_step[n];   m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2
 *   p -= lr * (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps)
 * which is torch.optim.Adam (L2 weight decay, no amsgrad) applied to that row alone with the row's own step count: a row listed on
 * every step evolves as under the dense optimizer.  Rows that are not listed are NOT READ AND NOT WRITTEN: no momentum carry-over
 * and no weight decay for them.  1 - beta^t is accurate to fp32 rounding (-expm1f(t ln beta), ln beta taken in double).
 * assume_unique != 0: the caller guarantees distinct ids (a sampler's src_nodes); no sort, no workspace.  With duplicates the
 *   result for those rows is unspecified, but nothing outside the listed rows is written.
 * assume_unique == 0: (id, position) pairs are sorted by id in `workspace` (rgcn_emb_adam_rows_workspace_bytes) and every run of
 *   equal ids is one update.
 * An id outside [0, num_nodes) writes nothing and adds 1 to *bad_ids (a device word the caller zeroes and reads when it next
 * synchronises; may be NULL).  The call is asynchronous: it allocates nothing and reads nothing back.  No float atomics: the same
 * inputs give the same bits.  All row addressing is in 64-bit element offsets on plain pointers (planes * num_nodes * ld may pass
 * 2^31).  Whole 16-byte pieces of a row move as such when ld, ldg, the plane strides and the four float bases are 16-byte
 * aligned; anything else goes element by element.
 * Refusals, before any launch: NULL table / moments / row_step (or nodes / grad with n_rows > 0): RGCN_ERR_NULL; width outside
 * 1 .. ld or > ldg, planes < 1, a negative count or stride, beta outside [0, 1), eps <= 0, lr < 0, weight_decay < 0:
 * RGCN_ERR_ARG; n_rows > 0xFFFF0000: RGCN_ERR_PLAN; with assume_unique == 0 a workspace smaller than the query:
 * RGCN_ERR_WORKSPACE.  n_rows == 0 launches nothing. */
size_t rgcn_emb_adam_rows_workspace_bytes(int64_t n_rows, int32_t num_nodes);   /* 0 on bad arguments; 0 is also right for assume_unique callers */
int rgcn_emb_adam_rows(float* table, float* exp_avg, float* exp_avg_sq, int32_t* row_step, int planes, int64_t plane_stride,
                       int32_t num_nodes, int width, int ld, const int64_t* nodes, int64_t n_rows, const float* grad,
                       int64_t grad_plane_stride, int ldg, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int assume_unique, int32_t* bad_ids, void* workspace, size_t workspace_bytes, void* stream);

/* ---- link prediction: DistMult decoder, negatives, filtered ranks (csrc/rgcn_linkpred.hip) ------------------------
 * Additions; RGCN_ABI_VERSION stays.  Conventions of every entry point below:
 *   z [num_nodes][ldz] and rel [num_relations][ldr] fp32; width 1..128 (RGCN_ERR_WIDTH); strides multiples of 4 and at least the
 *   width, bases 16-byte aligned (RGCN_ERR_STRIDE); pad columns behind `width` never enter a sum, whatever they hold.  s / r / o
 *   (anchor / r / target) are contiguous int64 device vectors.  Limits: num_nodes < 2^31, num_relations <= 65536,
 *   2 n_triples <= 0xFFFF0000, n_queries <= 0xFFFF0000: RGCN_ERR_PLAN beyond.  NULL pointers (RGCN_ERR_NULL), negative counts
 *   (RGCN_ERR_ARG) and small workspaces (RGCN_ERR_WORKSPACE) are answered before any launch; n_triples == 0 / n_queries == 0
 *   launches nothing and writes nothing.  Every *_workspace_bytes answers 0 on arguments its call would refuse.
 *   rgcn_lp_score / _index_build / _backward / _corrupt are asynchronous: no allocation, no read-back, no synchronisation.  A
 *   triple with an id out of range scores 0, gets and gives no gradient, and sets RGCN_LP_BAD_NODE / RGCN_LP_BAD_REL in the
 *   caller-owned device word `bad` (may be NULL; the caller zeroes it and reads it when it next synchronises).
 *   No float atomics: the same inputs give the same bits. */
#define RGCN_LP_BAD_NODE 1
#define RGCN_LP_BAD_REL 2

/* score[t] = sum_k z[s_t][k] rel[r_t][k] z[o_t][k].  A triple is ceil(width / 4) lanes, each adds its four products as
 * (p0 + p1) + (p2 + p3), the lanes are added by a shuffle tree. */
int rgcn_lp_score(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                  const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, float* score, int32_t* bad, void* stream);

/* The index of one batch of triples, a function of (s, r, o) alone, into caller buffers: node_slot [2 n_triples] holds the slots
 * 2 t + side (side 0: s_t, 1: o_t) sorted stably by their node, node_ptr [num_nodes + 1] where each node's slots begin;
 * rel_triple [n_triples] the triples sorted stably by relation, rel_ptr [num_relations + 1].  Triples with an id out of range lie
 * behind node_ptr[num_nodes] / rel_ptr[num_relations] and set `bad`.  One half may be left out (node_ptr NULL: no node half, which
 * only dz needs; rel_ptr NULL: no relation half, which only drel needs). */
size_t rgcn_lp_index_workspace_bytes(int64_t n_triples, int32_t num_nodes, int32_t num_relations);
int rgcn_lp_index_build(const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, int32_t num_nodes,
                        int32_t num_relations, uint32_t* node_ptr, uint32_t* node_slot, uint32_t* rel_ptr, uint32_t* rel_triple,
                        int32_t* bad, void* workspace, size_t workspace_bytes, void* stream);

/* dz [num_nodes][lddz] and / or drel [num_relations][lddrel] (NULL: not wanted) from g [n_triples] = dL/d score and the index of
 * the same (s, r, o).  dz[v] = sum over v's slots in sorted order of (g_t rel[r_t]) o z[other end]; EVERY row is written (zeros
 * where a node has no triple; the pad columns of the last 16-byte piece are +0, columns behind it are not touched); s_t == o_t
 * contributes twice.  drel[r] = sum_t (g_t z[s_t]) o z[o_t]: the relation's triples in sorted order in chunks of 256, a chunk's
 * triples dealt round robin to the 64 / ceil(width / 4) lane groups of a wave and the groups added in order, then the chunks in
 * order.  The workspace is needed for drel only. */
size_t rgcn_lp_backward_workspace_bytes(int64_t n_triples, int32_t num_relations, int width);
int rgcn_lp_backward(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                     const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, const float* g,
                     const uint32_t* node_ptr, const uint32_t* node_slot, const uint32_t* rel_ptr, const uint32_t* rel_triple,
                     float* dz, int lddz, float* drel, int lddrel, void* workspace, size_t workspace_bytes, void* stream);

/* Negatives: position i * num_negatives + j of the outputs holds triple i with ONE end replaced by a node id in [0, num_nodes):
 *   d = mix(mix(seed + 0x9E3779B97F4A7C15 (i + 1)) + 0xD1B54A32D192ED03 (j + 1));   id = (d * num_nodes) >> 64;
 *   the object is replaced when the top bit of mix(d + 0x2545F4914F6CDD1D) is set, else the subject
 * (mix as in the sampler, arithmetic mod 2^64): a pure function of (seed, i, j, num_nodes).  Ids of s / o pass through unchecked.
 * Negatives are not filtered against true triples.  num_nodes < 1, num_negatives < 1 or seed < 0: RGCN_ERR_ARG;
 * n_triples * num_negatives > 0xFFFF0000: RGCN_ERR_PLAN. */
int rgcn_lp_corrupt(const int64_t* s, const int64_t* r, const int64_t* o, int64_t n_triples, int32_t num_nodes, int32_t num_negatives,
                    int64_t seed, int64_t* s_out, int64_t* r_out, int64_t* o_out, void* stream);

/* Ranks.  For query q the candidate e scores (z[anchor_q] o rel[r_q]) . z[e]; over all e in [0, num_nodes) that are neither in
 * filter_idx[filter_ptr[q] .. filter_ptr[q + 1]) nor the target, greater[q] counts the scores strictly above the target's and
 * equal[q] those with exactly the target's bits.  filter_ptr NULL: raw ranks.  A list holds distinct ids (an id listed twice is taken
 * off twice); entries out of range are ignored.  Every score of the call -- sweep, target, listed -- comes from one device function,
 * so the counts are exact integers; the scores need not be rgcn_lp_score's bits.  A query with an id out of range gets -1 / -1.
 * Scores are never written: the workspace is n_queries floats, whatever num_nodes is.  Integer atomics in the counts. */
size_t rgcn_lp_rank_workspace_bytes(int64_t n_queries, int32_t num_nodes, int width);
int rgcn_lp_rank(const float* z, int ldz, const float* rel, int ldr, int width, int32_t num_nodes, int32_t num_relations,
                 const int64_t* anchor, const int64_t* r, const int64_t* target, int64_t n_queries, const int64_t* filter_ptr,
                 const int64_t* filter_idx, int64_t filter_len, int64_t* greater, int64_t* equal, void* workspace,
                 size_t workspace_bytes, void* stream);

/* ---- summaries -> original graph on tensors: block labels, transferred embeddings (csrc/rgcn_transfer.hip) ----------
 * Additions; RGCN_ABI_VERSION stays.  Both calls are asynchronous: no allocation, no read-back, no synchronisation, everything on
 * `stream`.  Argument checks come before the device is looked at.  An id out of range is never used as an address: it sets one of
 * the bits below in the caller-owned device word `bad` (may be NULL; the caller zeroes it and reads it when it next synchronises).
 * Integer atomics only: the same inputs give the same bits. */
#define RGCN_TR_BAD_BLOCK 1 /* a block id outside [0, num_blocks) */
#define RGCN_TR_BAD_NODE 2  /* a train_idx / nodes entry outside [0, num_nodes) */
#define RGCN_TR_BAD_MAP 4   /* a map value < -1 or >= the table's rows */
#define RGCN_TR_MAX_TABLES 16
#define RGCN_TR_STACK 0  /* out [S][n_out][width]: one plane per table (plane_stride floats apart) */
#define RGCN_TR_CONCAT 1 /* out [n_out][S width]: the tables side by side */
#define RGCN_TR_SUM 2    /* out [n_out][width]: ((0 + t_0) + t_1) + ... in fp32, in table order */

/* The fractional labels of a node partition.  block [num_nodes] holds ids in [0, num_blocks); train_idx [n_train] distinct node
 * ids; y [n_train][ldy] int64 counts (the multi-hot rows of the training nodes).  Out: size [num_blocks] = nodes per block;
 * y_sum[b][c] = (float)((double)(sum of y[i][c] over the rows i with block[train_idx[i]] == b) / (double)max(1, size[b])) in rows
 * of ld floats (columns behind `classes` are not touched); nonzero[b] = 1 where the integer sum of the row is not 0.  The sums are
 * int32.  Equal block ids of a wave are combined before they reach memory, so the one-block partition is one atomic per wave.
 * A node whose block id is out of range counts nowhere (RGCN_TR_BAD_BLOCK), a training row whose node is out of range adds
 * nothing (RGCN_TR_BAD_NODE).  workspace: num_blocks x classes int32.
 * Refusals: NULL size / y_sum / nonzero / workspace (block with num_nodes > 0, train_idx / y with n_train > 0): RGCN_ERR_NULL;
 * num_blocks < 1, classes < 1, a negative count, ld < classes, ldy < classes: RGCN_ERR_ARG; num_nodes, num_blocks or n_train
 * >= 2^31, classes > 65536, n_train x classes or num_blocks x classes > 2^38: RGCN_ERR_PLAN; a small workspace:
 * RGCN_ERR_WORKSPACE.  The query answers 0 on arguments the call refuses. */
size_t rgcn_tr_block_labels_workspace_bytes(int64_t num_nodes, int64_t num_blocks, int64_t n_train, int classes);
int rgcn_tr_block_labels(const int64_t* block, int64_t num_nodes, int64_t num_blocks, const int64_t* train_idx, const int64_t* y,
                         int64_t ldy, int64_t n_train, int classes, int32_t* size, float* y_sum, int64_t ld, int32_t* nonzero,
                         int32_t* bad, void* workspace, size_t workspace_bytes, void* stream);

/* The transferred embedding of the nodes `nodes` [n_out] (repeats allowed; NULL: all num_nodes nodes in order, n_out ==
 * num_nodes) from S = num_tables summary tables.  tables / lds / rows / maps are HOST arrays of S entries: table s is fp32
 * [rows[s]][lds[s]] on the device, maps[s] int64 [num_nodes] on the device with the row of every node in table s, or -1 where the
 * node is not mapped.  A mapped node's piece is the table row; an unmapped node's piece is uniform in [0, 1):
 *   bits = mix(mix(seed + 0x9E3779B97F4A7C15 (s + 1)) + node * width + column);   value = (bits >> 40) * 2^-24
 * (mix as in the sampler, arithmetic mod 2^64): a pure function of (seed, s, node, column), never of the launch, n_out, the node's
 * position or the mode.  A nodes entry outside [0, num_nodes) gives a row of zeros (RGCN_TR_BAD_NODE), a map value < -1 or >=
 * rows[s] a piece of zeros (RGCN_TR_BAD_MAP).  ld_out: floats between output rows; plane_stride: floats between the planes of
 * RGCN_TR_STACK (ignored otherwise).  Whole 16-byte pieces move as such when every lds[s], ld_out (and plane_stride, and width for
 * RGCN_TR_CONCAT) is a multiple of 4 and every base is 16-byte aligned; anything else goes element by element.  Rows are addressed
 * by 64-bit element offsets.  No workspace.
 * Refusals: NULL arrays, a NULL table with rows, a NULL map with nodes, NULL out with n_out > 0: RGCN_ERR_NULL; num_tables outside
 * 1 .. 16, width < 1, an unknown mode, a negative count or seed, nodes == NULL with n_out != num_nodes: RGCN_ERR_ARG; lds[s] <
 * width, ld_out smaller than an output row, overlapping planes: RGCN_ERR_STRIDE; num_nodes or n_out >= 2^31: RGCN_ERR_PLAN.
 * n_out == 0 launches nothing. */
int rgcn_tr_gather(const float* const* tables, const int32_t* lds, const int64_t* rows, const int64_t* const* maps, int num_tables,
                   int width, int64_t num_nodes, const int64_t* nodes, int64_t n_out, int mode, int64_t seed, float* out,
                   int64_t ld_out, int64_t plane_stride, int32_t* bad, void* stream);

/* ---- N-Triples ingest: file bytes -> COO tensors and term tables (csrc/rgcn_ingest.hip) -------------------------
 * Additions; RGCN_ABI_VERSION stays.  The contract is graphs.py's: lines end at '\n' (one '\r' before it is dropped, the last line
 * need not end in '\n'); a line of at most 2 bytes is skipped; every other line loses its last 2 bytes and splits at its first two
 * spaces into subject, predicate, object (the object keeps further spaces; a term may be empty); 'A'..'Z' are folded to lower case
 * wherever bytes are compared.  Terms are ordered bytewise.  Node ids are the ranks among the terms that occur as subject or
 * object, relation ids the ranks among the predicates other than "<http://www.w3.org/1999/02/22-rdf-syntax-ns#type>" and "<type>",
 * class ids the ranks among the objects of the rdf-syntax type triples whose subject's bytes up to its first '#' are not
 * "http://swrc.ontoware.org/ontology".  The i-th other triple, in file order, is edge 2 i = (s, o, 2 rel) and edge 2 i + 1 =
 * (o, s, 2 rel + 1).  The subjects of the class triples are the labelled nodes; labels[j][c] = 1 iff labelled_idx[j] has class c.
 *
 * `text` is a device pointer to num_bytes <= 0xFFFF0000 bytes (RGCN_ERR_PLAN beyond; offsets are 32-bit); at most 0x55550000
 * triples.  Four calls, each on `stream`, each with a caller-owned workspace; the library allocates nothing.  A call SYNCHRONISES
 * the stream only for the read-backs named below, into the host pointers given.  Argument errors (RGCN_ERR_NULL, _ARG, _PLAN,
 * _WORKSPACE, in this order of checks) are answered before any launch; the size queries answer 0 on arguments the call refuses and
 * multiples of 256 otherwise.
 *
 *   rgcn_nt_lines      *num_lines = lines of the text (one read-back).
 *   rgcn_nt_tokenize   num_lines as rgcn_nt_lines answered (another count: RGCN_ERR_ARG).  Occurrence 3 t + role (role 0 / 1 / 2:
 *                      subject / predicate / object of the t-th triple, in file order) -> occ_off / occ_len [3 num_lines entries
 *                      each, the first 3 T written].  One read-back into info[4] (host): T, the 1-based number of the first line
 *                      with fewer than two spaces after the cut (0: none), that of the first line with a NUL byte (0: none), the
 *                      longest term.  RGCN_ERR_GRAPH when either line number is set; occ_off / occ_len are then unspecified.
 *   rgcn_nt_build      distinct terms by a hash_bits-bit hash (1 .. 64, else RGCN_ERR_ARG; seed >= 0) and a stable sort; EVERY
 *                      occurrence is then compared, length and bytes, with the first of its run: a difference answers
 *                      RGCN_ERR_COLLISION, and no id ever depends on the hash.  Bytewise ranks by refinement rounds over 4 bytes a
 *                      round (one read-back per round), roles, ids.  counts[8] (host): U distinct terms, N nodes, R relations (the
 *                      COO has 2 R edge types), C classes, E edges, L labelled nodes, the device status word, rounds.
 *                      max_term_len as rgcn_nt_tokenize answered; occ pairs that leave the text: RGCN_ERR_GRAPH.
 *   rgcn_nt_emit       the same workspace, untouched since rgcn_nt_build answered RGCN_OK, and that call's counts: edge_index
 *                      int64 [2][E], edge_type [E], labelled_idx [L] ascending, labels [L][C], and (offset, length) into the text of
 *                      one occurrence of every node / relation / class, in id order.  Asynchronous, no read-back.  Counts that
 *                      do not fit num_triples: RGCN_ERR_ARG; nothing is ever written outside the sizes the counts give. */
size_t rgcn_nt_lines_workspace_bytes(int64_t num_bytes);
int rgcn_nt_lines(const uint8_t* text, int64_t num_bytes, void* workspace, size_t workspace_bytes, int64_t* num_lines, void* stream);
size_t rgcn_nt_tokenize_workspace_bytes(int64_t num_bytes, int64_t num_lines);
int rgcn_nt_tokenize(const uint8_t* text, int64_t num_bytes, int64_t num_lines, uint32_t* occ_off, uint32_t* occ_len, void* workspace,
                     size_t workspace_bytes, int64_t* info, void* stream);
size_t rgcn_nt_workspace_bytes(int64_t num_triples);
int rgcn_nt_build(const uint8_t* text, int64_t num_bytes, const uint32_t* occ_off, const uint32_t* occ_len, int64_t num_triples,
                  int64_t max_term_len, int hash_bits, int64_t seed, void* workspace, size_t workspace_bytes, int64_t* counts,
                  void* stream);
int rgcn_nt_emit(int64_t num_triples, const int64_t* counts, int64_t* edge_index, int64_t* edge_type, int64_t* labelled_idx,
                 int64_t* labels, uint32_t* node_off, uint32_t* node_len, uint32_t* rel_off, uint32_t* rel_len, uint32_t* cls_off,
                 uint32_t* cls_len, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RGCN_MI355X_H */

// lgcn_kernels.h -- the launcher boundary of lgcn_device.hip (not installed): the argument structs of the training kernels, the
// constants the plan builder and the step driver read, and ONE declaration per launch.  The host files (lgcn_graph.cpp,
// lgcn_train.cpp) fill in a struct and call a launcher; the grid arithmetic and the choice of instantiation live beside the kernel,
// in lgcn_device.hip.  Nothing here is device code.
#ifndef LGCN_KERNELS_H
#define LGCN_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lgcn_hip.h"

typedef __bf16 bf16_t;

#ifndef LGCN_GATHER_U
#define LGCN_GATHER_U 8      /* max row gathers in flight per lane (8 x 16 B raw = 32 VGPRs) */
#endif

// the edge-dropout mask of one step (the hash and its rule: lgcn_device.hip; make_drop in lgcn_internal.h fills this in)
struct DropArgs { uint32_t k0, k1, thr; float inv; int32_t tr; int32_t on; };

// ---------------------------------------------------------------------------------
// Work plan of one graph (built on the host at lgcn_graph_create).
//
// The processing order of the rows is cut into 8 slices, one per XCD (hardware deals
// workgroups round-robin over the 8 XCDs -- speed-only observation -- so block b works on
// slice b & 7).  A slice's rows mostly gather rows of the same part of the graph
// (reorder.py), so the part of the table an XCD touches is a fraction of the whole and
// lives in that XCD's 4 MiB L2.  Inside a slice:
//   * rows with more than LONG_T (= one 64-entry tile) non-zeros run as independent waves at
//     the FRONT of the slice (they start first: their serial tile walk overlaps everything
//     else).  Rows up to LONG_CH non-zeros are finished by one wave; longer rows are cut into
//     chunks of LONG_CH (a single wave walking Gowalla's 1415-nnz row = 23 serial tiles was
//     the critical path = the entire 57 us of an un-split launch): each chunk writes a partial
//     row and takes a ticket, and the LAST arriver sums the partials in chunk order (fixed
//     order: bitwise reproducible whoever is last) and runs the epilogue.  The hand-off is not
//     free (write-through stores, a drain, an atomic round trip, an L1 invalidate), which is
//     why the chunk is 512 and not one tile.  Long rows stay in the slice of their part of the
//     graph: they are 29 % of Gowalla's non-zeros, and dealt round-robin over the XCDs (round 1)
//     they alone produced half of the L2 misses.
//   * the other rows go NPW at a time per wave, ONE ROW PER LANE GROUP (NPW = 64 / lanes per row:
//     4 fp32 rows or 8 bf16 rows at d = 64), 4 waves per workgroup, in order.  The plan sorts every
//     window of SHORT_WIN consecutive short rows by length, so the rows of a pack are about equally
//     long (the window is far smaller than what an XCD has in flight: locality is unaffected).
// ---------------------------------------------------------------------------------
#define LONG_T 64             /* rows with more non-zeros than one tile leave the short path */
#define SLICE_PAD 64          /* short rows of a slice are padded to a multiple of this (>= rows per workgroup of every variant) */
#ifndef SHORT_WIN
#define SHORT_WIN 2048        /* window of the length sort (measured 128 / 512 / 1024 / 2048 / 4096 / 8192: 6082 / 6330 / 6403 / 6400 / 6378 / 6329 steps/s) */
#endif
#ifndef LONG_CH
#define LONG_CH 512           /* measured on Gowalla: 64 -> 58 us, 128 -> 40, 256 -> 34, 512 -> 32.5, 768 -> 39, none -> 57 */
#endif
#define XCDS 8
// The (col,val) pairs of the planned rows are kept a second time as ONE packed stream of 8-byte entries in
// plan order (chunks of a slice, then its short rows): the rows of a pack are contiguous there, so a wave
// loads a whole pack's index tiles with one or two 512-byte instructions instead of two 4-byte loads per
// row.  What bounds these kernels is the number of vector-memory instructions a CU retires (a 13-lane index
// load holds its address/return path as long as a 64-lane 1-KiB row gather, 26-30 cycles per instruction
// measured on both the fp32 and the bf16 table), so every instruction saved is time saved.
struct LongPlan {
    const int4 *chunks;           // [n_chunk_slots] (index o into long_row | -1 = padding, first entry, end entry in the stream, ordinal in row)
    const int32_t *long_row;      // [n_long] row ids with nnz > LONG_T
    const int32_t *long_nch;      // [n_long] chunks of that row
    float *partials;              // [n_chunk_slots, D]  (slot = position in `chunks`)
    int32_t *counters;            // [n_long] arrival tickets (zero between launches)
    int32_t n_long, n_chunk_slots;
};
struct SlicePlan {                // per XCD slice x: chunk blocks [cblk[x], cblk[x+1]) then short rows [rows[x], rows[x+1]) of rowinfo
    int32_t cblk[XCDS + 1];
    int32_t rows[XCDS + 1];       // multiples of SLICE_PAD
};

struct SpmmArgs {
    const int2 *pk;               // packed (col, val bits) stream in plan order
    const int4 *rowinfo;          // short rows of the slices, padded per slice: (row | -1, first entry in the stream, count, 0)
    LongPlan lp; SlicePlan sp;
    const void *X; void *Y;
    int64_t n_rows;               // rows of X (picks 32- or 64-bit gather offsets)
    long long *G64; uint32_t *bitmap; float div;   // sparse gradient rows (fixed point), K+1
    const float *G32;             // their fp32 copy Gs = G64 / 2^50 / (K+1), valid on the flagged rows (k_g32)
    float *P; float *M; float *V;
    bf16_t *Pb;                   // optional bf16 shadow of P written by the Adam epilogue
    void *Pq;                     // optional fp8 shadow of P (rows + scales), same
    // last kernel of a step (K >= 2): its epilogue zeroes the G64 rows / bitmap bits it consumes and one
    // wave reduces the per-triplet loss terms, so no separate clean-up launch is needed
    int clear;
    const float *terms; const float *gathered; float *loss_out; int32_t B, shard; float decay;
    float ent_coeff;              // popularity gate: coefficient of the gates' entropy term in the loss (0: no gate)
    int64_t blk;                  // data parallel: floats per rank in `gathered` (0: the default layout 3*shard*D + 2*shard)
    float step_size, bc2_sqrt, w1, beta2, omb2, eps;
    int remap;
    const float *selfX;           // M_ADDSELF: Y[row] = selfX[row] + (A X)[row]  (item-item smoothing, model.py:228-229)
    int32_t *cnt; float lam;      // reg_ego: slots of the batch naming each row (zeroed as consumed), decay / B: grad += lam * cnt[row] * P[row]
    DropArgs dr;                  // edge dropout of the step (dr.on: the DROP instantiation is launched); behind the older fields, so that every one of them keeps its offset
    float w_in, w_add;            // M_WTS launches only (layer weights): Y = w_add * G[row] + w_in * (A X)[row]
    int32_t wt;                   // LGCN_STORE_ARG_* bits: which of the launch's row stores go write-through (0: all plain).
                                  //   A run-time, wave-uniform field and no template axis: the instantiations stay what they were
};

enum { M_SPARSE = 1, M_ADDG = 2, M_ADAM = 4, M_ADDSELF = 8, M_WTS = 16 };

//   M_SPARSE: X is Gs, read from the fp32 copy G32 for rows flagged in `bitmap`
//   M_ADDG  : add Gs[row] where flagged (Horner term)
//   M_ADAM  : apply torch.optim.Adam to P/M/V with grad = result, else store to Y
//   M_WTS   : layer weights are set (lgcn_ctx_set_layer_weights): G32 holds the UNSCALED gradient rows and the launch carries the
//             two coefficients of its Horner step, h_{k-1} = w_{k-1} G + A h_k with h_K = w_K G.  The first backward layer gathers
//             G itself, so its product takes w_in = w_K and its Horner term w_add = w_{K-1}; every later layer has w_in = 1.
//             A MODE bit and not a run-time test: the instantiations without it are what they were
// Y = [Gs +] A_hat X on the graph's plan.  `mode` is one of the ten the library launches: 0, M_ADDSELF (fp32 tables only), and
// M_ADDG and M_SPARSE | M_ADDG, each with and without M_ADAM and with and without M_WTS; any other value is error 3
int lgcn_spmm_launch(const SpmmArgs &a, int mode, int d, int x_dtype, int y_dtype, hipStream_t st);

struct MeanArgs {
    const float *X0; const void *Xl[LGCN_MAX_LAYERS + 1]; int K;
    float *out; int64_t n4;      // number of 4-element pieces
    int32_t d; int64_t N;        // row width and rows of the tables (fp8 tables: where a piece's row scale lies)
    float w[LGCN_MAX_LAYERS + 1];   // WTS instantiations only (lgcn_propagate_weighted): out = sum_k w[k] X_k
};
void lgcn_layer_mean_launch(const MeanArgs &m, int act_dtype, bool wts, hipStream_t st);

void lgcn_to_bf16_launch(const float *src, bf16_t *dst, int64_t n, hipStream_t st);
int lgcn_to_fp8_launch(const float *src, void *dst, int64_t n_rows, int d, hipStream_t st);

// BPR on the batch: k_triplet, k_triplet_dense, k_cols_finish
#ifndef TRIPLET_HUB_NNZ
#define TRIPLET_HUB_NNZ 131072  /* rows longer than this get their last-layer row from the hub plan (whole chip) instead of one workgroup
                                  (10M x 1M graph, ms per step: off 264, 8192: 242, 32768: 236, 65536: 239, 131072: 228, 262144: 231, 524288: 244) */
#endif
#ifndef TRIPLET_HUB_CHUNK
#define TRIPLET_HUB_CHUNK 2048   /* non-zeros per chunk of the hub plan's rows */
#endif
struct BprArgs {
    const int32_t *indptr; const int32_t *indices; const float *vals;
    const float *X0; const void *Xl[LGCN_MAX_LAYERS + 1]; int K;
    int32_t n_users; int64_t N;
    const int32_t *users; const int32_t *pos; const int32_t *neg;   // already offset to the local shard
    int32_t B_local;      // triplets handled by this launch
    int32_t shard;        // row stride of the contrib block (>= B_local)
    float inv_B;          // 1 / global batch
    float lam;            // decay / global batch
    long long *G64;       // if non-null: atomics
    uint32_t *bitmap;
    uint32_t *stale_bitmap; int64_t bitmap_words;   // last step's bitmap: zeroed here (plain stores)
    uint32_t *item_bitmap;  // item-item smoothing: bit i = item i is named by the batch (or NULL)
    float *contrib;       // exchange block [3*shard*D | shard | shard] (data parallel)
    int32_t exchange;     // write the gradient rows and loss terms to `contrib` (instead of / besides the atomics)
    const float *Xhub; int32_t hub_nnz;     // rows with more than hub_nnz non-zeros: X_K[row] is read from Xhub (0: none)
    float *terms;         // atomics mode: [2*terms_stride] (loss terms | reg terms), this launch at terms_off
    int32_t terms_off, terms_stride;
    int32_t *err;
    int32_t dense_last;   // X_K exists densely (Xl[K]): the slot rows are read, not gathered
    int32_t reg_ego;      // L2 term on the tables' own rows X0[row] (upstream LightGCN) instead of the propagated rows (the fork)
    int32_t *cnt;         // reg_ego: per-row count of the batch slots naming the row (bumped where the row is flagged), or NULL
    // column-sharded data parallelism: this rank holds D of the table's columns.  cols_phase 1: the batch-row kernel stops after
    // the slot rows -- it writes them to erows [3][B_local][D] and the PARTIAL dot products / squared norms over its columns to
    // colsum [3][B_local] (pos score, neg score, reg term); the ranks all-reduce colsum; k_cols_finish does the rest.
    int32_t cols_phase; float *erows; float *colsum;
    DropArgs dr;          // edge dropout of the step (dr.on: k_triplet's DROP instantiation gathers the last layer); behind the older fields: their offsets stay
    float w[LGCN_MAX_LAYERS + 1];   // WTS instantiations only (layer weights): slot row e = sum_k w[k] X_k[row] instead of the mean
    // The fold of k_g32 into this launch (lgcn_train_epoch's single-GPU steps): mult != NULL.  mult[c * B_local + b]
    // = slots of THIS batch that name slot (c, b)'s row (k_slot_mult, once per call); the workgroup that completes a row writes
    // its fp32 copy G32[row] = (float)(G64[row] * 2^-50) / gdiv itself.  arrive: [N] arrival tickets of the shared rows, zero between steps
    const uint16_t *mult; float *G32; float gdiv; int32_t *arrive;
};
// The batch-row launch of a.B_local > 0 triplets: k_cols_finish under a.cols_phase == 2, else k_triplet_dense under a.dense_last,
// else k_triplet (big: 64-bit gather offsets; a.dr.on: its dropout form; wts: the weighted slot rows, which come first)
int lgcn_triplet_launch(const BprArgs &a, int d, int act_dtype, bool wts, bool big, hipStream_t st);

// The popularity gate: k_triplet_gate, k_gate_rank_total, k_gate_adam
#define GATE_TPB 8            /* triplets per workgroup (two per wave) */
#define GATE_HMAX 64          /* pop_hidden, gate_hidden <= 64 (lane = hidden unit) */
struct GateArgs {
    const float *E;               // [N,d] final propagated table (layer mean, item-item smoothing applied)
    const float *item_pop;        // [m_items]
    const float *params;          // flat: W1[Hp] b1[Hp] W2[d*Hp] b2[d] V1[Hg*2d] c1[Hg] V2[Hg] c2[1]  (torch.nn.Linear layouts)
    long long *partials;          // [grid, P] per-workgroup parameter-gradient sums, FIXED POINT (2^50): every slot's contribution is
                                  // converted before it is added, so the total is independent of how slots fall into workgroups and
                                  // ranks (integer sums are associative) -- the data-parallel step equals the single-GPU step bit for bit
    int32_t Hp, Hg, P;
    float inv_temp, ent_scale;    // 1 / pop_gate_temp ; gate_entropy_coeff / (2 B)
    int32_t n_users; int64_t N;
    const int32_t *users; const int32_t *pos; const int32_t *neg;
    int32_t B; float inv_B, lam;
    long long *G64; uint32_t *bitmap; uint32_t *item_bitmap;      // item_bitmap: bit i = item i named by the batch (or NULL)
    uint32_t *stale_bitmap; int64_t bitmap_words;
    float *terms; int32_t terms_stride;
    int32_t *err;
    float *contrib; int32_t shard; int32_t exchange;   // data parallel: gradient rows and loss terms of this rank's shard go to the exchange
                                                        // block [3*shard*D | shard | shard | shard] (besides / instead of the atomics)
};
int lgcn_gate_launch(const GateArgs &g, int d, hipStream_t st);
void lgcn_gate_rank_total_launch(const long long *partials, int32_t n_part, int32_t P, long long *out, hipStream_t st);
struct GateAdamArgs {
    const long long *src; int32_t n_src; int64_t stride; int32_t P;      // n_src vectors of P sums, `stride` int64 apart
    float *params, *m, *v, *grad_out;
    float step_size, bc2_sqrt, w1, beta2, omb2, eps;
};
void lgcn_gate_adam_launch(const GateAdamArgs &a, hipStream_t st);

struct MeanSplitArgs {
    const float *X0; const void *Xl[LGCN_MAX_LAYERS + 1]; int K;
    float *out_u, *out_i; int64_t n4_users, n4;      // 4-element pieces: of the user block, of the whole table
};
void lgcn_mean_layers_launch(const MeanSplitArgs &m, int act_dtype, hipStream_t st);
void lgcn_flag_range_launch(uint32_t *bm, int64_t lo, int64_t hi, hipStream_t st);

// The slot kernels over the 3 B slots of a batch: k_scatter, k_g32, k_flag_rows, k_finish
struct SlotArgs {
    const int32_t *users; const int32_t *pos; const int32_t *neg;
    int32_t B; int32_t n_users; int64_t N;
    long long *G64; uint32_t *bitmap;
    float *G32; float div;                                 // k_g32: fp32 copy of the flagged rows, K+1
    const float *gathered; int32_t shard; int32_t world;   // DP scatter
    int32_t skip_rank;                                     // DP scatter: this rank's own block is in G64 already (-1: none)
    const float *terms; float *loss_out; float decay;
    float ent_coeff;
    int64_t blk;                                           // floats per rank in `gathered` (0: default layout)
    uint32_t *item_bitmap;                                 // DP scatter with item-item smoothing: items named by the global batch
    int32_t *cnt;                                          // reg_ego: per-row slot counts (k_scatter / k_flag_rows bump, k_finish clears), or NULL
};
int lgcn_scatter_launch(const SlotArgs &s, int d, hipStream_t st);
int lgcn_g32_launch(const SlotArgs &s, int d, hipStream_t st);
int lgcn_finish_launch(const SlotArgs &s, int d, hipStream_t st);
void lgcn_flag_rows_launch(const SlotArgs &s, hipStream_t st);
// ... and their siblings over the (2 + R) B slots of a batch with several negatives per positive
struct SlotArgsMulti {
    SlotArgs s;                    // users / pos / B / tables / loss reduction as in the three-slot kernels (s.neg unused)
    const int32_t *negs; int64_t neg_stride; int32_t R;
};
int lgcn_g32_multi_launch(const SlotArgsMulti &s, int d, hipStream_t st);
int lgcn_finish_multi_launch(const SlotArgsMulti &s, int d, hipStream_t st);

// k_slot_mult: the slot multiplicities of the batches of B of the triplets [0, T) (the fold of k_g32)
#define SLOT_MULT_HMAX 16384        /* hash slots, 8 bytes each: 128 KiB of a CU's 160 KiB; batches up to B = 4096 */
#define SLOT_MULT_THREADS 1024
struct SlotMultArgs {
    const int32_t *users; const int32_t *pos; const int32_t *neg;
    int64_t T; int32_t B; int32_t n_users; int64_t N;
    uint16_t *out; int32_t H;
};
// hash slots for batches of B triplets: a power of two with 3 B <= 3/4 H, or 0 where that exceeds the LDS budget
static inline int32_t slot_mult_hash(int32_t B) {
    if (B <= 0) return 0;
    int64_t H = 64;
    while (3 * H < 12 * (int64_t)B) H <<= 1;
    return H <= SLOT_MULT_HMAX ? (int32_t)H : 0;
}
int lgcn_slot_mult_launch(const int32_t *users, const int32_t *pos, const int32_t *neg, int64_t T, int32_t B, int32_t n_users,
                          int64_t N, uint16_t *out, hipStream_t st);

void lgcn_apply_perm_launch(const int32_t *S, int cols, const int64_t *perm, int64_t T, int32_t *users, int32_t *pos, int32_t *neg,
                            hipStream_t st);
void lgcn_apply_perm_multi_launch(const int32_t *S, int cols, const int64_t *perm, int64_t T, int32_t *users, int32_t *pos,
                                  int32_t *negs, int32_t R, hipStream_t st);

// what lgcn_graph_create and lgcn_dropout_mask run on the device: k_index_range and k_pack_stream (on the null stream), k_dropout_mask
void lgcn_index_range_launch(const int32_t *indices, int64_t nnz, int32_t n_rows, int32_t *bad);
void lgcn_pack_stream_launch(const int4 *items, int64_t n_items, const int32_t *indices, const float *vals, int2 *pk);
void lgcn_dropout_mask_launch(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t nnz, uint32_t k0, uint32_t k1,
                              uint64_t thr, uint8_t *keep_out, hipStream_t st);
#endif

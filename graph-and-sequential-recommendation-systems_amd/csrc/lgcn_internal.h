// lgcn_internal.h -- declarations shared by the translation units of liblgcn_hip.so (not installed).
#ifndef LGCN_INTERNAL_H
#define LGCN_INTERNAL_H
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>       // types only: RCCL is resolved with dlopen at run time, never linked
#include <math.h>
#include <stdio.h>
#include "lgcn_hip.h"
#include "lgcn_kernels.h"      // (every unit gets its macros -- XCDS, LONG_T, GATE_TPB, ... -- with it: keep such names out of the other files)

extern "C" void lgcn_set_error(const char *msg);   // lgcn_host.cpp
// 0 under LGCN_LOSS_BPR; else rc 3 and the message "<who>: the ... loss ... is implemented for ... only" (lgcn_ctx.cpp): ONE wording
// for every entry point that does not train the loss set on the context.  The same callers cannot train hard negatives
// (lgcn_ctx_set_hard_neg) either: while those are set it returns 3 and names them, whatever the loss
int lgcn_refuse_loss(const lgcn_ctx *x, const char *who);

#define HIP_OK(expr)                                                            \
    do {                                                                        \
        hipError_t e_ = (expr);                                                 \
        if (e_ != hipSuccess) {                                                 \
            char buf_[256];                                                     \
            snprintf(buf_, sizeof buf_, "%s failed: %s", #expr, hipGetErrorString(e_)); \
            lgcn_set_error(buf_);                                               \
            return 10;                                                          \
        }                                                                       \
    } while (0)

// ---------------------------------------------------------------------------------
// What lgcn_graph.cpp (graph object, propagation) and the training units (lgcn_ctx.cpp, lgcn_train.cpp, lgcn_train_dp.cpp) share
// ---------------------------------------------------------------------------------
// graph object: device CSR (borrowed) + the long-row plan and its scratch (owned)
struct lgcn_graph {
    const int32_t *indptr; const int32_t *indices; const float *vals; const int4 *rowinfo;
    const int2 *pk;       // the planned rows' (col,val) pairs, packed, in plan order
    int64_t n_rows, nnz;
    int32_t d_max;
    LongPlan lp; SlicePlan sp;
    void *owned;          // one device allocation holding plan arrays, partials and counters
    // The long-row scratch (partials, tickets) is shared by every launch on this graph: launches
    // are ordered.  A launch on another stream than the previous one first waits for it.
    mutable hipStream_t last_stream; mutable bool used; mutable hipEvent_t order_ev;
};
// long_ch: non-zeros per chunk of a split row (LONG_CH for the propagation plans; the hub plan of k_triplet, whose rows
// have 10^4 .. 10^6 non-zeros, takes longer chunks so that a row's last arriver has hundreds, not thousands, of partials to add)
int lgcn_graph_create_impl(const int32_t *indptr, const int32_t *indices, const float *vals,
                           int64_t n_rows, int64_t nnz, int32_t d_max, const int32_t *row_order,
                           int64_t n_order, const int64_t *xcd_start, int32_t long_ch, lgcn_graph **out);
int lgcn_check_layer_weights(const char *who, const float *w, int n, int K);
int64_t lgcn_fold_segment_steps();      // lgcn_ctx.cpp

// a launch on `st` is about to use the graph's scratch: order it behind the previous user
static inline int graph_acquire(const lgcn_graph *g, hipStream_t st) {
    if (g->used && g->last_stream != st) {
        HIP_OK(hipEventRecord(g->order_ev, g->last_stream));
        HIP_OK(hipStreamWaitEvent(st, g->order_ev, 0));
    }
    g->used = true; g->last_stream = st;
    return 0;
}
static inline SpmmArgs graph_spmm(const lgcn_graph *g) {
    SpmmArgs a{};
    a.pk = g->pk; a.rowinfo = g->rowinfo; a.lp = g->lp; a.sp = g->sp; a.n_rows = g->n_rows;
    return a;
}
// gathered tables of 4 GiB or more need 64-bit offsets (priced at the fp32 row size whatever the table type)
static inline bool big_table(int64_t n_rows, int d) { return n_rows * (int64_t)d * 4 >= (1ll << 32); }
// bytes of one [N,d] table of a storage type (fp8: rows + fp32 row scales, padded so that the next table stays 256-byte aligned)
static inline size_t table_bytes(int64_t N, int d, int dtype) {
    if (dtype == LGCN_FP8) return (((size_t)N * d + (size_t)N * 4) + 255) & ~(size_t)255;
    return (size_t)N * d * (dtype == LGCN_BF16 ? 2 : 4);
}
static inline int check_dtype(int t) {
    if (t != LGCN_F32 && t != LGCN_BF16 && t != LGCN_FP8) { lgcn_set_error("dtype must be LGCN_F32, LGCN_BF16 or LGCN_FP8"); return 3; }
    return 0;
}
// edge dropout: the step's keys (the hash itself: lgcn_device.hip); hard negatives: the step's picks (lgcn_hn_rank below, which
// the kernel calls too)
static __host__ __device__ inline uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline bool drop_prob_ok(float keep_prob) { return keep_prob > 0.f && keep_prob <= 1.f; }      // (NaN fails both)
// floor(keep_prob * 2^32): exact in double; 2^32 itself (keep_prob = 1) means "keep everything"
static inline uint64_t drop_threshold(float keep_prob) { return (uint64_t)floor((double)keep_prob * 4294967296.0); }
// the mask of one step; keep_prob in (0, 1): at 1 there is nothing to drop and on stays 0 (the launch is the plain one)
static inline DropArgs make_drop(float keep_prob, uint64_t seed, int64_t step, int transposed) {
    DropArgs d{};
    if (!(keep_prob < 1.f)) return d;
    const uint64_t k = splitmix64(splitmix64(seed) + (uint64_t)step);
    d.k0 = (uint32_t)k; d.k1 = (uint32_t)(k >> 32);
    d.thr = (uint32_t)drop_threshold(keep_prob); d.inv = 1.0f / keep_prob; d.tr = transposed ? 1 : 0; d.on = 1;
    return d;
}

// The RCCL entry points the data-parallel path uses.  Resolved once, preferring the librccl that is
// already mapped into the process (PyTorch-ROCm ships its own copy; two RCCL instances in one process
// would each build their own topology/IPC state), else LGCN_RCCL_PATH, else the system librccl.so.1.
struct RcclApi {
    ncclResult_t (*GetUniqueId)(ncclUniqueId *);
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*GroupStart)();
    ncclResult_t (*GroupEnd)();
    const char *(*GetErrorString)(ncclResult_t);
};
const RcclApi *lgcn_rccl();      // nullptr (+ error text) if RCCL cannot be found

struct lgcn_dp {
    ncclComm_t comm;
    int world, rank;
    const RcclApi *api;      // the collectives this communicator runs on: RCCL (lgcn_dp.cpp) or the in-process loopback
    bool loopback;
};
void lgcn_dp_loopback_release(lgcn_dp *dp);      // lgcn_dp_loopback.hip
void lgcn_dp_loopback_abort(lgcn_dp *dp);        // a rank failed outside a collective: wake every waiter, all later collectives fail

// The batch-row launch for samples with several negatives (lgcn_multineg.hip; lgcn_train_step_multi fills this in).
// Sample b = (users[b], pos[b], negs[r * neg_stride + b] for r < R); dense-last form: Xl[1..K] are all tables of the storage type.
struct MultiNegArgs {
    const float *X0; const void *Xl[LGCN_MAX_LAYERS + 1]; int K;
    int32_t n_users; int64_t N;
    const int32_t *users; const int32_t *pos; const int32_t *negs; int64_t neg_stride;
    int32_t R, B;
    float inv_BR, inv_R;          // 1 / (B R), 1 / R
    float lam, lam_n;             // decay / B (user, positive rows), decay / (B R) (a negative's row)
    long long *G64; uint32_t *bitmap;
    uint32_t *stale_bitmap; int64_t bitmap_words;      // last step's bitmap: zeroed by the launch (plain stores)
    float *terms; int32_t terms_stride;                // [2 * terms_stride]: per-sample loss term | reg term
    int32_t *err;
    int32_t reg_ego; int32_t *cnt;                     // reg_ego: cnt[row] += R per user / positive slot, 1 per negative slot
    float w[LGCN_MAX_LAYERS + 1];                      // wts launches only: the layer weights
    // the loss (lgcn_ctx_set_loss): LGCN_LOSS_BPR, or LGCN_LOSS_SOFTMAX with z_r = -x_r / tau and gb_r = -q_r * inv_tauB,
    // inv_tauB = 1 / (tau B) (inv_BR is then unused)
    int32_t loss; float tau, inv_tauB;
};
int lgcn_multineg_launch(const MultiNegArgs &a, int d, int act_dtype, bool wts, hipStream_t st);

// Hard negatives, DNS(M, N) (lgcn_hardneg.hip; lgcn_ctx_set_hard_neg).  H: which of the M hardest candidates sample b
// of a step trains on, 0..M-1.  Keyed as the dropout mask of the step is -- splitmix64(splitmix64(seed) + step), `step` the Adam
// step counter as it stands BEFORE the step (0 for the first step of a fresh context), make_drop's convention -- then moved into
// a stream of its own by a domain constant and mixed with the sample index: at equal seeds the dropout mask and the picks share
// no state.  The high word goes into the modulus (M <= 16: the bias of 2^32 mod M is below 4e-9).  ONE definition: the kernel
// calls it, lgcn_hard_neg_rank exports it, tests/hard_neg_restatement.py restates it.
#define LGCN_HN_DOMAIN 0x4841524E45473031ull      /* "HARNEG01" */
static __host__ __device__ inline uint32_t lgcn_hn_rank(uint64_t seed, int64_t step, int32_t b, int32_t M) {
    const uint64_t k = splitmix64(splitmix64(seed) + (uint64_t)step);
    const uint64_t v = splitmix64((k ^ LGCN_HN_DOMAIN) + (uint64_t)(uint32_t)b);
    return M > 1 ? (uint32_t)(v >> 32) % (uint32_t)M : 0u;
}
// `m` carries what the batch-row launch of the multi-negative step carries (inv_BR, inv_R, lam_n, loss, tau are unused: every one of
// the three slots weighs 1 and the divisor is B)
struct HardNegArgs {
    MultiNegArgs m;
    float inv_B;                  // 1 / B
    int32_t top_m;                // M, 1..R
    uint64_t seed; int64_t step;  // the arguments of lgcn_hn_rank (step: the counter before the step)
    int32_t *sel_id;              // [B] the selected ITEM id of each sample (-1: void) -- the negative column of the backward's three-slot kernels
    int32_t *sel_out;             // [B] the selected index r (-1: void), or NULL
};
int lgcn_hardneg_launch(const HardNegArgs &h, int d, int act_dtype, bool wts, hipStream_t st);

// The in-batch sampled softmax (lgcn_inbatch.hip; lgcn_train_step_inbatch fills this in).  Sample b = (users[b],
// pos[b]); every user of the batch scores against every positive of the batch.  `m` carries what the batch-row launch of the
// other losses carries (tables, ids, G64, bitmaps, terms, err, cnt, layer weights, tau, inv_tauB; negs / R / inv_BR / lam_n
// are unused, loss = LGCN_LOSS_INBATCH).  The workspace is the context's: `cap` rows (a multiple of 32, >= B rounded up to 32).
#define LGCN_INBATCH_PART_TILES 8      /* 32-row tiles of the swept side one workgroup covers: the sweep split */
struct InBatchArgs {
    MultiNegArgs m;
    float *U, *P;                 // [cap][d] fp32: the users' / positives' output-table rows, zero rows for void samples and padding
    float *sbb;                   // [cap] s_{b,b}
    int32_t *uid, *pid;           // [cap] the sample's ids, -1 / -1 for a void sample or padding (uid >= 0 is the sound flag)
    float *part;                  // [parts][Bp][2] partial (m, r) of a user over one part of the item sweep: sum = exp(m) (1 + r)
    float *mrg;                   // [cap][2] merged (M, 1 + Zm1) of a user
    int32_t cap;
    // the score options (lgcn_ctx_set_inbatch_scores), behind everything the default launches read.  Their three
    // [cap] vectors lie behind `part` (the largest part count): invu, invp = 1 / |e_u|, 1 / |e_p| of the sample under cosine, lqb =
    // item_logq[p_b] under logq; 0 for a void sample and for padding (and inv = 0 for a row of norm 0)
    int32_t score;                // LGCN_SCORE_DOT, or LGCN_SCORE_COSINE: U, P then hold the rows over their norms
    const float *item_logq;       // [m_items] log Q(item), or NULL: no correction
    // mixed negatives (lgcn_train_step_inbatch_mix), behind everything the other launches read.  mix != 0: m.negs /
    // neg_stride / R / inv_R / lam_n are set, the item side has (1 + R) Bp rows -- pool row (r, c) is row Bp (1 + r) + c of P and
    // of pid (-1: sample c is void or padding), part holds lgcn_inbatch_mix_parts(B, R) parts -- and the three vectors of the
    // score options are these, the item-side ones over the same (1 + R) Bp rows
    int32_t mix, icap;            // icap: item rows of P / pid / xinvp / xlq in the workspace (>= (1 + R) Bp)
    float *xinvu, *xinvp, *xlq;
};
static __host__ __device__ inline int32_t lgcn_inbatch_rows(int32_t B) { return (B + 31) & ~31; }                          // Bp: B padded to whole tiles
static __host__ __device__ inline int32_t lgcn_inbatch_parts(int32_t B) { return (lgcn_inbatch_rows(B) / 32 + LGCN_INBATCH_PART_TILES - 1) / LGCN_INBATCH_PART_TILES; }
// parts of the (1 + R) Bp-row item sweep of a mixed step
static __host__ __device__ inline int32_t lgcn_inbatch_mix_parts(int32_t B, int32_t R) {
    return ((1 + R) * (lgcn_inbatch_rows(B) / 32) + LGCN_INBATCH_PART_TILES - 1) / LGCN_INBATCH_PART_TILES;
}
int lgcn_inbatch_launch(const InBatchArgs &a, int d, int act_dtype, bool wts, hipStream_t st);

// The alignment-and-uniformity loss (lgcn_directau.hip; lgcn_train_step_directau fills this in).  Sample b = (users[b],
// pos[b]); `m` carries what the batch-row launch of the other losses carries (negs / R / inv_BR / lam_n / tau / inv_tauB are unused,
// loss = LGCN_LOSS_DIRECTAU).  The workspace is the context's own: `cap` rows (a multiple of 32, >= B rounded up to 32), the rows
// and the sweep split of the in-batch step (lgcn_inbatch_rows, lgcn_inbatch_parts, LGCN_INBATCH_PART_TILES).
struct DirectAuArgs {
    MultiNegArgs m;
    float *X, *Y;                 // [cap][d] fp32: the users' / positives' output-table rows over their norms; zero rows for void samples and padding
    float *invx, *invy;           // [cap] 1 / |e_u|, 1 / |e_p| (0 for a row of norm 0, a void sample, padding)
    float *qx, *qy;               // [cap] the fp32 sum of squares of the stored x_b, y_b (1 up to rounding; 0 for a zero row)
    float *al;                    // [cap] |x_b - y_b|^2 (0 for a void sample and padding)
    int32_t *uid, *pid;           // [cap] the sample's ids, -1 / -1 for a void sample or padding (uid >= 0 is the sound flag)
    float *part;                  // [2][parts][tiles] partial sums of k over (side, part of the sweep, owner tile)
    float *scal;                  // [2] the coefficients 2 gamma / Z_X, 2 gamma / Z_Y of the step (0: no pair, or gamma = 0)
    int32_t cap;
    float gamma;
};
int lgcn_directau_launch(const DirectAuArgs &a, int d, int act_dtype, bool wts, hipStream_t st);
#endif

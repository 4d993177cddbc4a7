// lgcn_ctx.h -- the training context and what the three host units that work on it share: lgcn_ctx.cpp (create / destroy, setters,
// getters, refusals), lgcn_train.cpp (the single-GPU step driver) and lgcn_train_dp.cpp (the data-parallel forms).  Host only: no
// .hip unit includes this file, so a change of the context rebuilds no device code.
#ifndef LGCN_CTX_H
#define LGCN_CTX_H
#include <algorithm>

#include "lgcn_internal.h"

// ---------------------------------------------------------------------------------
// training context
// ---------------------------------------------------------------------------------
struct lgcn_ctx {
    lgcn_train_config c;
    int64_t step;
    int64_t N;
    int64_t bm_words;             // words per bitmap; cfg.bitmap holds two, used alternately
    int flip;
    void *act[LGCN_MAX_LAYERS + 1];   // act[k] = X_k storage for k = 1..K-1 (K with dense_last; also reused for H)
    int fwd_layers;               // dense forward layers per step: K-1, or K with dense_last
    float *g32;                   // [N,d] fp32 copy of the step's flagged gradient rows (library-owned; k_g32)
    bf16_t *e0b;                  // [N,d] bf16 copy of E0 (library-owned; bf16 activation storage with K >= 2 only)
    void *e0q;                    // fp8 copy of E0, rows + scales (library-owned; fp8 activation storage with K >= 2 only); e0b_fresh covers it too
    bool e0b_fresh;               // e0b == bf16(E0) right now (set by the Adam epilogue inside a multi-step call)
    bool in_loop;                 // inside lgcn_train_epoch / lgcn_train_epoch_dp: the Adam epilogue keeps e0b current
    lgcn_graph *hub_graph;        // plan over the rows with more than hub_nnz non-zeros (or NULL): their last-layer rows are
    int32_t hub_nnz;              //   computed by k_spmm into g32 before k_triplet instead of by the one workgroup of a triplet
    int64_t hub_rows;             // rows in that plan
    bool dp_local;                // data parallel (rows): part 1 also adds this rank's own rows into G64, part 2 scatters the others'
    int dp_rank;                  // rank of the last part 1
    // optional branches of the fork (popularity gate / item-item smoothing): the step runs on ONE final table
    bool variant;                 // either branch is on
    float *tvar;                  // [N,d] fp32 final propagated table T (library-owned)
    uint32_t *item_bitmap;        // [ceil(m_items/32)] items named by the batch (item-item backward), library-owned
    long long *gate_partials;     // [n_wg, P] parameter-gradient partial sums, fixed point (library-owned)
    long long *gate_total;        // [P] this rank's sum of them, all-reduced by the dense data-parallel form (behind gate_partials)
    int32_t gate_P, gate_wgs;
    int32_t *cnt;                 // reg_ego: [N] slots of the running step naming each row (library-owned, zero between steps)
    float *colsum;                // [3 * max_batch] partial scores / reg terms of a column-sharded step (library-owned)
    // edge dropout (lgcn_ctx_set_dropout): drop_keep < 1 = on.  dr is the mask of the running step, made by lgcn_train_step from
    // the step counter as it stands BEFORE the step; forward, batch rows and backward all read it (dr.on = 0: off)
    float drop_keep; uint64_t drop_seed; DropArgs dr;
    // layer weights (lgcn_ctx_set_layer_weights): lw_n = K + 1 values in lw, or 0 = the mean
    int32_t lw_n; float lw[LGCN_MAX_LAYERS + 1];
    // the fold of k_g32 into k_triplet (lgcn_ctx_set_fold_g32): lgcn_train_epoch computes the slot multiplicities
    // of its steps (k_slot_mult) into `mult` and points fold_mult at the running step's slice; NULL everywhere else
    bool fold_g32;                // the setter's switch (default on)
    uint16_t *mult; int64_t mult_cap;     // library-owned, grown when a call needs more (elements)
    const uint16_t *fold_mult;    // multiplicities of the running step's slots, or NULL: the step launches k_g32
    int32_t *arrive;              // [N] arrival tickets of the rows several slots name (library-owned, zero between steps; allocated by the first call that folds)
    int64_t folded_steps;         // steps run with the fold since the context was created
    // the (2 + R) B slot form of the running step (SlotScope): on only while a multi-negative step (R >= 1), an
    // in-batch step (R = 0, no negatives) or a mixed one (R >= 1) runs -- its backward enumerates (2 + R) B slots (negative column
    // r at negs + r * stride) and, with R > 0, the reg_ego epilogue takes decay / (B R)
    struct SlotForm { const int32_t *negs; int64_t stride; int32_t R; bool on; } mn;
    // the loss of the multi-negative step (lgcn_ctx_set_loss): LGCN_LOSS_BPR launches the BPR instantiations of k_multineg,
    // LGCN_LOSS_SOFTMAX the softmax ones with the temperature loss_temp; the three-slot and rank-splitting entry points refuse
    int32_t loss_kind; float loss_temp;
    // the in-batch softmax (LGCN_LOSS_INBATCH): the workspace of its launches, allocated by the first lgcn_ctx_set_loss
    // that accepts the loss (ib_cap = max_batch rounded up to 32 rows) and freed with the context; ONE allocation, carved up
    void *ib_ws; int32_t ib_cap;
    // its score options (lgcn_ctx_set_inbatch_scores): independent of loss_kind, (LGCN_SCORE_DOT, NULL) by default
    int32_t ib_score; const float *ib_logq;
    // mixed negatives (lgcn_ctx_set_inbatch_mix): ib_mix = R_max (0: off).  While it is on, ib_ws is large enough for
    // both carvings: the plain step's (the one above, unchanged) and the mixed step's with (1 + R_max) ib_cap item rows
    int32_t ib_mix;
    // the store policy (lgcn_ctx_set_store_policy): LGCN_STORE_* bits, and the SpmmArgs::wt the last +Adam launch and
    // the last forward launch of the deepest layer carried (the getter reports them)
    int32_t store_policy, wt_adam, wt_fwd;
    // hard negatives (lgcn_ctx_set_hard_neg): hn_m = M (0: off).  While it is on, the multi-negative step launches
    // k_hardneg, which writes the selected item of each sample to hn_sel (library-owned [max_batch], allocated by the first setter
    // that turns it on) -- the negative column of the backward's three-slot kernels -- and its index to hn_out (the caller's, or NULL)
    int32_t hn_m; uint64_t hn_seed; int32_t *hn_sel, *hn_out;
    // the alignment-and-uniformity loss (LGCN_LOSS_DIRECTAU; lgcn_ctx_set_directau): gamma, and the workspace of its
    // launches (DirectAuWs over au_cap = max_batch rounded up to 32 rows), allocated by the first setter call that accepts and freed
    // with the context
    float au_gamma; void *au_ws; int32_t au_cap;
};
// a multi-step call: nobody but this library touches E0 between its steps
struct LoopScope {
    lgcn_ctx *x;
    explicit LoopScope(lgcn_ctx *x_) : x(x_) { x->in_loop = true; x->e0b_fresh = false; }
    ~LoopScope() { x->in_loop = false; x->e0b_fresh = false; }
};
// a slot-form step: the loss launch, the backward's slot kernels and the reg_ego epilogue read x->mn; cleared on every way out
struct SlotScope {
    lgcn_ctx *x;
    SlotScope(lgcn_ctx *x_, const int32_t *negs, int64_t stride, int32_t R) : x(x_) { x->mn = {negs, stride, R, true}; }
    ~SlotScope() { x->mn = {}; }
};
// THE carving of the in-batch workspace for `cap` rows of dim d, in floats from its start:
//   U | P | sbb | uid | pid | mrg | part | invu | invp | lq      with icap = (1 + R_max) cap item rows in P, pid, invp and lq
// R_max = 0 is the plain step's carving, R_max >= 1 the mixed step's; both live in ONE allocation of `words` floats, which is
// never smaller than the plain carving's.  The plain kernels do not take the three score vectors as arguments: ib_invu() in
// lgcn_inbatch.hip finds them at part + 2 cap lgcn_inbatch_parts(cap), which is where `invu` lands here -- `part` holds exactly
// that many floats under R_max = 0 and invu, invp, lq ([cap] each) are the next blocks
struct InBatchWs {
    size_t U, P, sbb, uid, pid, mrg, part, invu, invp, lq, words, icap;
    InBatchWs(int32_t cap_, int d, int32_t R_max) {
        const size_t cap = (size_t)cap_;
        const size_t parts = (size_t)(R_max ? lgcn_inbatch_mix_parts(cap_, R_max) : lgcn_inbatch_parts(cap_));
        size_t at = 0;
        auto take = [&at](size_t n) { const size_t o = at; at += n; return o; };
        icap = (size_t)(1 + R_max) * cap;
        U = take(cap * d); P = take(icap * d); sbb = take(cap); uid = take(cap); pid = take(icap); mrg = take(2 * cap);
        part = take(2 * cap * parts); invu = take(cap); invp = take(icap); lq = take(icap);
        words = at;
        if (R_max) words = std::max(words, InBatchWs(cap_, d, 0).words);
    }
};
// THE carving of the workspace of the alignment-and-uniformity loss for `cap` rows of dim d, in floats from its start
struct DirectAuWs {
    size_t X, Y, invx, invy, qx, qy, al, uid, pid, part, scal, words;
    DirectAuWs(int32_t cap_, int d) {
        const size_t cap = (size_t)cap_;
        size_t at = 0;
        auto take = [&at](size_t n) { const size_t o = at; at += n; return o; };
        X = take(cap * d); Y = take(cap * d); invx = take(cap); invy = take(cap); qx = take(cap); qy = take(cap); al = take(cap);
        uid = take(cap); pid = take(cap); part = take(2 * (size_t)lgcn_inbatch_parts(cap_) * (cap / 32)); scal = take(4);
        words = at;
    }
};

// The ids of a global batch and the slice of it a launch works on: triplets [b_off, b_off + B_local) of B_global, in shards of
// `shard` triplets over `world` ranks.  The shard arithmetic of every data-parallel form lives in of_rank() and nowhere else
struct BatchView {
    const int32_t *users, *pos, *neg;
    int32_t B_global, b_off, B_local, shard, world;
    // rank `rank` of `world`: shards of ceil(B_global / world); a short last batch leaves trailing ranks with B_local = 0
    static BatchView of_rank(const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B_global, int32_t world, int32_t rank) {
        const int32_t shard = (B_global + world - 1) / world;
        const int32_t b_off = rank * shard;
        int32_t B_local = B_global - b_off;
        if (B_local > shard) B_local = shard;
        if (B_local < 0) B_local = 0;
        return {users, pos, neg, B_global, b_off, B_local, shard, world};
    }
    static BatchView whole(const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B) { return {users, pos, neg, B, 0, B, B, 1}; }
};

// Where the loss launch puts the rows of its slice.  atomics: into G64 and the row flags; exchange: into the exchange block
// (cfg.contrib); count_slots: reg_ego's slot counts are taken by this launch (with atomics only); cols_phase: 0, or part 1 / 2 of
// the column-sharded step.  These five are every combination there is
struct LossPlace { bool atomics, exchange, count_slots; int cols_phase; };
constexpr LossPlace PLACE_STEP{true, false, true, 0};                // the single-GPU step: everything lands on this GPU
constexpr LossPlace PLACE_EXCHANGE{false, true, true, 0};            // the exchange block only: k_scatter adds every rank's rows
constexpr LossPlace PLACE_EXCHANGE_AND_G64{true, true, true, 0};     // dp_local: the block, and this rank's own rows at once
constexpr LossPlace PLACE_DENSE{true, false, false, 0};              // this rank's G64, all-reduced later; k_flag_rows counts the slots
constexpr LossPlace PLACE_COLS_SCORES{false, false, false, 1};       // column shard, part 1: slot rows + partial scores
constexpr LossPlace PLACE_COLS_ROWS{true, false, true, 2};           // column shard, part 2: the rows, from the all-reduced scores

// ---------------------------------------------------------------------------------
// What lgcn_ctx.cpp and lgcn_train.cpp define and lgcn_train_dp.cpp calls too
// ---------------------------------------------------------------------------------
int lgcn_refuse_dropout(const lgcn_ctx *x, const char *who);             // lgcn_ctx.cpp
int lgcn_refuse_layer_weights(const lgcn_ctx *x, const char *who);
int train_check_batch(const lgcn_ctx *x, const void *u, const void *p, const void *n, int32_t B);      // lgcn_train.cpp, as all below
SpmmArgs train_base_spmm(const lgcn_ctx *x);
int train_forward(lgcn_ctx *x, hipStream_t st);
int train_bpr(lgcn_ctx *x, const BatchView &v, LossPlace at, hipStream_t st);
int train_variant_loss(lgcn_ctx *x, const BatchView &v, LossPlace at, hipStream_t st);
int64_t train_dp_block_floats(const lgcn_ctx *x, int64_t S);
int64_t train_dp_block_tail(const lgcn_ctx *x, int64_t S);
SlotArgs train_slot_args(const lgcn_ctx *x, const BatchView &v, const float *gathered, float *loss_out);
void *train_bwd_buffer(const lgcn_ctx *x, int k);
int train_backward_layer(lgcn_ctx *x, int k, const BatchView &v, const float *gathered, float *loss_out, bool fused_finish, hipStream_t st);
int train_backward(lgcn_ctx *x, const BatchView &v, const float *gathered, float *loss_out, hipStream_t st, bool gate_reduced);
#endif

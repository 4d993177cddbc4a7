// lgcn_train.cpp -- host side of training: the training context, its setters and refusals, the step driver (forward layers,
// the loss launch of the step's form, the backward chain with Adam) and the data-parallel forms, behind the C ABI of
// include/lgcn_hip.h.  No kernels and no launches here: the driver fills in the args structs of lgcn_kernels.h and calls
// their launchers, which live beside the kernels in lgcn_device.hip.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

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
// The policy of a new context: LGCN_STORE_POLICY (0..3) or the default below; -1: the variable is set and is neither.
// Default: what the alternating runs of profiles/store_policy/README.md adopted.
#ifndef LGCN_STORE_POLICY_DEFAULT
#define LGCN_STORE_POLICY_DEFAULT LGCN_STORE_ADAM
#endif
static int store_policy_initial() {
    const char *e = getenv("LGCN_STORE_POLICY");
    if (!e) return LGCN_STORE_POLICY_DEFAULT;
    if (e[0] < '0' || e[0] > '0' + (LGCN_STORE_ADAM | LGCN_STORE_XLAST) || e[1] != '\0') return -1;
    return e[0] - '0';
}
// steps whose multiplicities one launch computes (and the context's buffer holds): 1024 steps = 3 * B * 1024 uint16 = 12 MiB at
// B = 2048, 24 MiB at the largest batch that folds.  LGCN_FOLD_SEGMENT: for tests only (a call longer than a small segment)
int64_t lgcn_fold_segment_steps() {
    const char *e = getenv("LGCN_FOLD_SEGMENT");
    const long v = e ? atol(e) : 0;
    return v > 0 ? (int64_t)v : 1024;
}
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

extern "C" int lgcn_ctx_create(const lgcn_train_config *cfg, lgcn_ctx **out) {
    if (!cfg || !out) { lgcn_set_error("lgcn_ctx_create: null argument"); return 3; }
    const lgcn_train_config &c = *cfg;
    if (!c.graph || !c.E0 || !c.adam_m || !c.adam_v || !c.G64 ||
        !c.bitmap || !c.terms || !c.err) { lgcn_set_error("lgcn_ctx_create: null buffer"); return 3; }
    if (c.K < 1 || c.K > LGCN_MAX_LAYERS) { lgcn_set_error("lgcn_ctx_create: K out of range"); return 3; }
    if ((c.K > 1 || c.dense_last) && !c.act) { lgcn_set_error("lgcn_ctx_create: activation workspace missing"); return 3; }
    if (c.d != 32 && c.d != 64 && c.d != 128 && c.d != 256) { lgcn_set_error("embedding dim must be 32, 64, 128 or 256"); return 3; }
    if (check_dtype(c.act_dtype)) return 3;
    if (c.act_dtype == LGCN_FP8 && c.d < 64) { lgcn_set_error("lgcn_ctx_create: fp8 activation storage needs an embedding dim of 64, 128 or 256"); return 3; }
    if (c.act_dtype == LGCN_FP8 && (c.item_pop || c.i2i)) { lgcn_set_error("lgcn_ctx_create: fp8 activation storage is implemented for the default model, not with the optional branches"); return 3; }
    if (c.n_users <= 0 || c.n_users >= c.graph->n_rows || c.max_batch <= 0) { lgcn_set_error("lgcn_ctx_create: bad sizes"); return 3; }
    if (c.d > c.graph->d_max) { lgcn_set_error("lgcn_ctx_create: d exceeds the graph's d_max"); return 3; }
    const bool gate = c.item_pop != nullptr, smooth = c.i2i != nullptr;
    if (gate || smooth) {
        if (!c.dense_last) { lgcn_set_error("lgcn_ctx_create: the optional branches need dense_last = 1 (every layer propagated densely)"); return 3; }
        const int64_t m_items = c.graph->n_rows - c.n_users;
        if (smooth && (!c.i2i_t || c.i2i->n_rows != m_items || c.i2i_t->n_rows != m_items || c.i2i->d_max < c.d || c.i2i_t->d_max < c.d)) {
            lgcn_set_error("lgcn_ctx_create: i2i / i2i_t must be [m_items, m_items] graphs with d_max >= d"); return 3; }
        if (gate && (!c.gate_params || !c.gate_adam_m || !c.gate_adam_v || !c.gate_grad || c.pop_hidden < 1 || c.pop_hidden > GATE_HMAX ||
                     c.gate_hidden < 1 || c.gate_hidden > GATE_HMAX || c.d > 128 || !(c.pop_gate_temp > 0.f))) {
            lgcn_set_error("lgcn_ctx_create: popularity gate needs its parameter / Adam buffers, hidden sizes in 1..64, d <= 128, temperature > 0"); return 3; }
    }
    if (c.reg_ego && (gate || smooth)) { lgcn_set_error("lgcn_ctx_create: reg_ego (upstream's L2 term) is defined for the default model only, not with the optional branches"); return 3; }
    const int policy = store_policy_initial();
    if (policy < 0) { lgcn_set_error("lgcn_ctx_create: LGCN_STORE_POLICY must be one of 0, 1, 2, 3 (LGCN_STORE_* bits)"); return 3; }
    lgcn_ctx *x = new (std::nothrow) lgcn_ctx;
    if (!x) { lgcn_set_error("out of memory"); return 4; }
    x->store_policy = policy; x->wt_adam = 0; x->wt_fwd = 0;
    x->c = c; x->step = 0; x->N = c.graph->n_rows; x->cnt = nullptr; x->colsum = nullptr;
    x->drop_keep = 1.f; x->drop_seed = 0; x->dr = DropArgs{};
    x->lw_n = 0; for (int k = 0; k <= LGCN_MAX_LAYERS; k++) x->lw[k] = 0.f;
    x->fold_g32 = true; x->mult = nullptr; x->mult_cap = 0; x->fold_mult = nullptr; x->arrive = nullptr; x->folded_steps = 0;
    x->mn = {};
    x->loss_kind = LGCN_LOSS_BPR; x->loss_temp = 1.f; x->ib_ws = nullptr; x->ib_cap = 0;
    x->ib_score = LGCN_SCORE_DOT; x->ib_logq = nullptr; x->ib_mix = 0;
    x->hn_m = 0; x->hn_seed = 0; x->hn_sel = nullptr; x->hn_out = nullptr;
    x->au_gamma = 0.f; x->au_ws = nullptr; x->au_cap = 0;
    x->bm_words = (x->N + 31) / 32; x->flip = 0;
    const size_t stride = table_bytes(x->N, c.d, c.act_dtype);
    for (int k = 0; k <= LGCN_MAX_LAYERS; k++) x->act[k] = nullptr;
    x->fwd_layers = c.dense_last ? c.K : c.K - 1;
    for (int k = 1; k <= x->fwd_layers; k++) x->act[k] = (char *)c.act + (size_t)(k - 1) * stride;
    // rows that are never flagged are never read; zero-filled so that the zero-weight padding reads of row 0 stay finite
    x->g32 = nullptr; x->e0b = nullptr; x->e0q = nullptr; x->e0b_fresh = false; x->in_loop = false; x->dp_local = false; x->dp_rank = -1;
    x->hub_graph = nullptr; x->hub_nnz = 0; x->hub_rows = 0;
    x->variant = gate || smooth; x->tvar = nullptr; x->item_bitmap = nullptr; x->gate_partials = nullptr; x->gate_total = nullptr; x->gate_P = 0; x->gate_wgs = 0;
    const size_t gbytes = (size_t)x->N * c.d * sizeof(float);
    bool ok = hipMalloc((void **)&x->g32, gbytes) == hipSuccess && hipMemset(x->g32, 0, gbytes) == hipSuccess;
    if (ok) ok = hipMalloc((void **)&x->colsum, sizeof(float) * 3 * (size_t)c.max_batch) == hipSuccess;
    if (ok && c.reg_ego) ok = hipMalloc((void **)&x->cnt, sizeof(int32_t) * (size_t)x->N) == hipSuccess && hipMemset(x->cnt, 0, sizeof(int32_t) * (size_t)x->N) == hipSuccess;
    if (ok && x->variant) ok = hipMalloc((void **)&x->tvar, gbytes) == hipSuccess;
    if (ok && smooth) {
        const size_t wb = sizeof(uint32_t) * (size_t)((x->N - c.n_users + 31) / 32);
        ok = hipMalloc((void **)&x->item_bitmap, wb) == hipSuccess && hipMemset(x->item_bitmap, 0, wb) == hipSuccess;
    }
    if (ok && gate) {
        x->gate_P = 2 * c.pop_hidden + c.d * c.pop_hidden + c.d + 2 * c.d * c.gate_hidden + 2 * c.gate_hidden + 1;
        x->gate_wgs = (c.max_batch + GATE_TPB - 1) / GATE_TPB;
        ok = hipMalloc((void **)&x->gate_partials, sizeof(long long) * ((size_t)x->gate_wgs + 1) * x->gate_P) == hipSuccess;
        if (ok) x->gate_total = x->gate_partials + (size_t)x->gate_wgs * x->gate_P;
    }
    if (ok && c.act_dtype == LGCN_BF16 && c.K >= 2) ok = hipMalloc((void **)&x->e0b, gbytes / 2) == hipSuccess;
    if (ok && c.act_dtype == LGCN_FP8 && c.K >= 2) ok = hipMalloc(&x->e0q, table_bytes(x->N, c.d, LGCN_FP8)) == hipSuccess;
    if (ok && !c.dense_last) {
        // Rows too long for one workgroup (a 800 000-neighbour item of the 10M x 1M graph kept ONE k_triplet workgroup busy
        // for 37 ms, several times per batch): a plan over just those rows; k_spmm computes their last-layer rows for
        // the whole chip to share, once per step, before k_triplet.
        const int32_t thr = c.hub_nnz == 0 ? TRIPLET_HUB_NNZ : c.hub_nnz;
        if (thr > 0) {
            std::vector<int32_t> ip((size_t)x->N + 1), hubs;
            ok = hipMemcpy(ip.data(), c.graph->indptr, sizeof(int32_t) * ip.size(), hipMemcpyDeviceToHost) == hipSuccess;
            for (int64_t r = 0; ok && r < x->N; r++) if (ip[(size_t)r + 1] - ip[(size_t)r] > thr) hubs.push_back((int32_t)r);
            if (ok && !hubs.empty()) {
                int32_t *dh = nullptr;
                ok = hipMalloc((void **)&dh, sizeof(int32_t) * hubs.size()) == hipSuccess &&
                     hipMemcpy(dh, hubs.data(), sizeof(int32_t) * hubs.size(), hipMemcpyHostToDevice) == hipSuccess;
                const int32_t hub_chunk = c.hub_chunk > 0 ? c.hub_chunk : TRIPLET_HUB_CHUNK;
                if (ok) ok = lgcn_graph_create_impl(c.graph->indptr, c.graph->indices, c.graph->vals, x->N, c.graph->nnz, c.d, dh,
                                               (int64_t)hubs.size(), nullptr, hub_chunk, &x->hub_graph) == 0;
                if (dh) (void)hipFree(dh);
                x->hub_nnz = thr; x->hub_rows = (int64_t)hubs.size();
            }
        }
    }
    if (!ok) {
        if (x->g32) (void)hipFree(x->g32);
        if (x->colsum) (void)hipFree(x->colsum);
        if (x->cnt) (void)hipFree(x->cnt);
        if (x->arrive) (void)hipFree(x->arrive);
        if (x->tvar) (void)hipFree(x->tvar);
        if (x->item_bitmap) (void)hipFree(x->item_bitmap);
        if (x->gate_partials) (void)hipFree(x->gate_partials);
        if (x->e0b) (void)hipFree(x->e0b);
        if (x->e0q) (void)hipFree(x->e0q);
        if (x->hub_graph) lgcn_graph_destroy(x->hub_graph);
        delete x;
        lgcn_set_error("lgcn_ctx_create: cannot allocate the library-owned tables (N*d*4 bytes fp32 gradient rows, N*d*2 bf16 parameters)");
        return 4;
    }
    *out = x;
    return 0;
}
extern "C" void lgcn_ctx_destroy(lgcn_ctx *ctx) {
    if (!ctx) return;
    if (ctx->g32) (void)hipFree(ctx->g32);
    if (ctx->colsum) (void)hipFree(ctx->colsum);
    if (ctx->cnt) (void)hipFree(ctx->cnt);
    if (ctx->arrive) (void)hipFree(ctx->arrive);
    if (ctx->mult) (void)hipFree(ctx->mult);
    if (ctx->ib_ws) (void)hipFree(ctx->ib_ws);
    if (ctx->hn_sel) (void)hipFree(ctx->hn_sel);
    if (ctx->au_ws) (void)hipFree(ctx->au_ws);
    if (ctx->tvar) (void)hipFree(ctx->tvar);
    if (ctx->item_bitmap) (void)hipFree(ctx->item_bitmap);
    if (ctx->gate_partials) (void)hipFree(ctx->gate_partials);
    if (ctx->e0b) (void)hipFree(ctx->e0b);
    if (ctx->e0q) (void)hipFree(ctx->e0q);
    if (ctx->hub_graph) lgcn_graph_destroy(ctx->hub_graph);
    delete ctx;
}
extern "C" int lgcn_ctx_set_dp_local(lgcn_ctx *ctx, int on) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_dp_local: null context"); return 3; }
    ctx->dp_local = on != 0; ctx->dp_rank = -1;
    return 0;
}
extern "C" int lgcn_ctx_set_fold_g32(lgcn_ctx *ctx, int on) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_fold_g32: null context"); return 3; }
    ctx->fold_g32 = on != 0;
    return 0;
}
extern "C" int64_t lgcn_ctx_folded_steps(const lgcn_ctx *ctx) { return ctx ? ctx->folded_steps : -1; }
extern "C" int lgcn_ctx_set_store_policy(lgcn_ctx *ctx, int bits) {
    if (bits & ~(LGCN_STORE_ADAM | LGCN_STORE_XLAST)) { lgcn_set_error("lgcn_ctx_set_store_policy: unknown store policy bits (LGCN_STORE_ADAM | LGCN_STORE_XLAST)"); return 3; }
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_store_policy: null context"); return 3; }
    ctx->store_policy = bits;
    return 0;
}
extern "C" int lgcn_ctx_get_store_policy(const lgcn_ctx *ctx, int32_t *launch_out) {
    if (launch_out) { launch_out[0] = ctx ? ctx->wt_adam : 0; launch_out[1] = ctx ? ctx->wt_fwd : 0; }
    return ctx ? ctx->store_policy : store_policy_initial();
}
extern "C" int lgcn_ctx_copy_arrivals(const lgcn_ctx *ctx, int32_t *dst_host, int64_t n) {
    if (!ctx || !dst_host) { lgcn_set_error("lgcn_ctx_copy_arrivals: null argument"); return 3; }
    if (ctx->variant || n < 0 || n > ctx->N) { lgcn_set_error("lgcn_ctx_copy_arrivals: the context has no arrival array of that size"); return 3; }
    if (!ctx->arrive) { memset(dst_host, 0, sizeof(int32_t) * (size_t)n); return 0; }       // no call has folded yet: nothing was ever counted
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(dst_host, ctx->arrive, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int64_t lgcn_ctx_get_step(const lgcn_ctx *ctx) { return ctx ? ctx->step : -1; }
extern "C" int64_t lgcn_ctx_hub_rows(const lgcn_ctx *ctx) { return (ctx && ctx->hub_graph) ? ctx->hub_rows : 0; }
extern "C" void lgcn_ctx_set_step(lgcn_ctx *ctx, int64_t s) { if (ctx) ctx->step = s; }
extern "C" void lgcn_ctx_set_lr(lgcn_ctx *ctx, double lr) { if (ctx) ctx->c.lr = lr; }
extern "C" int lgcn_ctx_set_dropout(lgcn_ctx *ctx, float keep_prob, uint64_t seed) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_dropout: null context"); return 3; }
    if (!drop_prob_ok(keep_prob)) { lgcn_set_error("lgcn_ctx_set_dropout: dropout keep_prob must be in (0, 1]"); return 3; }
    if (ctx->c.act_dtype == LGCN_FP8) { lgcn_set_error("lgcn_ctx_set_dropout: edge dropout is not implemented for LGCN_FP8 activation storage"); return 3; }
    if (ctx->variant) { lgcn_set_error("lgcn_ctx_set_dropout: edge dropout is not implemented with the optional branches (item-item smoothing / popularity gate)"); return 3; }
    if (ctx->lw_n && keep_prob < 1.f) { lgcn_set_error("lgcn_ctx_set_dropout: edge dropout is not implemented together with layer weights (lgcn_ctx_set_layer_weights)"); return 3; }
    ctx->drop_keep = keep_prob; ctx->drop_seed = seed; ctx->dr = DropArgs{};
    return 0;
}
// the entry points that split a step over ranks have no dropout form: say so instead of training undropped
static int refuse_dropout(const lgcn_ctx *x, const char *who) {
    if (!x || !(x->drop_keep < 1.f)) return 0;
    char buf[192];
    snprintf(buf, sizeof buf, "%s: edge dropout (lgcn_ctx_set_dropout) is implemented for the single-GPU step only", who);
    lgcn_set_error(buf);
    return 3;
}

extern "C" int lgcn_ctx_set_layer_weights(lgcn_ctx *ctx, const float *w_host, int32_t n) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_layer_weights: null context"); return 3; }
    if (!w_host || n == 0) { ctx->lw_n = 0; return 0; }            // back to the mean: the step launches what it always launched
    if (n < 0 || n > LGCN_MAX_LAYERS + 1) n = -1;                    // (reported as a wrong count)
    if (int rc = lgcn_check_layer_weights("lgcn_ctx_set_layer_weights", w_host, n, ctx->c.K)) return rc;
    if (ctx->c.act_dtype == LGCN_FP8) { lgcn_set_error("lgcn_ctx_set_layer_weights: layer weights are not implemented for LGCN_FP8 activation storage"); return 3; }
    if (ctx->variant) { lgcn_set_error("lgcn_ctx_set_layer_weights: layer weights are not implemented with the optional branches (item-item smoothing / popularity gate)"); return 3; }
    if (ctx->drop_keep < 1.f) { lgcn_set_error("lgcn_ctx_set_layer_weights: layer weights are not implemented together with edge dropout (lgcn_ctx_set_dropout)"); return 3; }
    for (int k = 0; k < n; k++) ctx->lw[k] = w_host[k];
    ctx->lw_n = n;
    return 0;
}
extern "C" int32_t lgcn_ctx_get_layer_weights(const lgcn_ctx *ctx, float *w_out) {
    if (!ctx || !ctx->lw_n) return 0;
    if (w_out) for (int k = 0; k < ctx->lw_n; k++) w_out[k] = ctx->lw[k];
    return ctx->lw_n;
}
// ... nor a weighted form: say so instead of training the mean
static int refuse_layer_weights(const lgcn_ctx *x, const char *who) {
    if (!x || !x->lw_n) return 0;
    char buf[192];
    snprintf(buf, sizeof buf, "%s: layer weights (lgcn_ctx_set_layer_weights) are implemented for the single-GPU step only", who);
    lgcn_set_error(buf);
    return 3;
}

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

// the conditions of the two softmax losses (`what`: the loss as the messages name it, `slots`: its slot form)
static int refuse_loss_config(const lgcn_ctx *ctx, float temperature, const char *what, const char *slots) {
    char buf[256];
    const char *fmt = nullptr;
    if (!(temperature > 0.f) || !isfinite(temperature)) fmt = "lgcn_ctx_set_loss: %s needs a finite temperature > 0";
    else if (ctx->c.act_dtype == LGCN_FP8) fmt = "lgcn_ctx_set_loss: %s is not implemented for LGCN_FP8 activation storage";
    else if (ctx->variant) fmt = "lgcn_ctx_set_loss: %s is not implemented with the optional branches (item-item smoothing / popularity gate)";
    else if (!ctx->c.dense_last) fmt = "lgcn_ctx_set_loss: %s needs a context with dense_last = 1 (the gathered last layer has no %s slot form)";
    if (!fmt) return 0;
    snprintf(buf, sizeof buf, fmt, what, slots);
    lgcn_set_error(buf);
    return 3;
}

extern "C" int lgcn_ctx_set_loss(lgcn_ctx *ctx, int32_t kind, float temperature) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_loss: null context"); return 3; }
    if (kind == LGCN_LOSS_BPR) { ctx->loss_kind = LGCN_LOSS_BPR; ctx->loss_temp = 1.f; return 0; }      // the step launches what it always launched
    if (kind == LGCN_LOSS_DIRECTAU) { lgcn_set_error("lgcn_ctx_set_loss: the alignment-and-uniformity loss (directau) takes gamma, not a temperature: set it with lgcn_ctx_set_directau"); return 3; }
    if (kind != LGCN_LOSS_SOFTMAX && kind != LGCN_LOSS_INBATCH) { lgcn_set_error("lgcn_ctx_set_loss: unknown loss kind (LGCN_LOSS_BPR, LGCN_LOSS_SOFTMAX or LGCN_LOSS_INBATCH)"); return 3; }
    if (ctx->hn_m) { lgcn_set_error("lgcn_ctx_set_loss: hard negatives (lgcn_ctx_set_hard_neg) are set on this context and train the BPR loss only"); return 3; }
    const bool inbatch = kind == LGCN_LOSS_INBATCH;
    if (int rc = refuse_loss_config(ctx, temperature, inbatch ? "the in-batch softmax loss (inbatch)" : "the sampled-softmax loss", inbatch ? "2 B" : "2 + R")) return rc;
    if (inbatch && !ctx->ib_ws) {       // the workspace is allocated once, before anything is changed
        const int32_t cap = lgcn_inbatch_rows(ctx->c.max_batch);
        void *ws = nullptr;
        if (hipMalloc(&ws, sizeof(float) * InBatchWs(cap, ctx->c.d, 0).words) != hipSuccess) {
            (void)hipGetLastError();
            lgcn_set_error("lgcn_ctx_set_loss: cannot allocate the workspace of the in-batch softmax loss (inbatch): 2 * max_batch * d * 4 bytes and a few vectors");
            return 4;
        }
        ctx->ib_ws = ws; ctx->ib_cap = cap;
    }
    ctx->loss_kind = kind; ctx->loss_temp = temperature;
    return 0;
}
extern "C" int lgcn_ctx_set_inbatch_scores(lgcn_ctx *ctx, int score, const float *item_logq) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_inbatch_scores: null context"); return 3; }
    if (score != LGCN_SCORE_DOT && score != LGCN_SCORE_COSINE) {
        lgcn_set_error("lgcn_ctx_set_inbatch_scores: unknown score kind (LGCN_SCORE_DOT or LGCN_SCORE_COSINE)"); return 3; }
    ctx->ib_score = score; ctx->ib_logq = item_logq;
    return 0;
}
extern "C" int lgcn_ctx_get_inbatch_scores(const lgcn_ctx *ctx, const float **item_logq) {
    if (!ctx) return -1;
    if (item_logq) *item_logq = ctx->ib_logq;
    return ctx->ib_score;
}
extern "C" int lgcn_ctx_set_inbatch_mix(lgcn_ctx *ctx, int32_t R_max) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_inbatch_mix: null context"); return 3; }
    if (R_max == 0) { ctx->ib_mix = 0; return 0; }      // off: the workspace stays (the plain step carves the same allocation)
    if (R_max < 1 || R_max > LGCN_MAX_NEG_RATIO) {
        char buf[160];
        snprintf(buf, sizeof buf, "lgcn_ctx_set_inbatch_mix: R_max = %d is out of range (0 = off, or 1..%d)", (int)R_max, LGCN_MAX_NEG_RATIO);
        lgcn_set_error(buf); return 3;
    }
    if (ctx->loss_kind != LGCN_LOSS_INBATCH || !ctx->ib_ws) {
        lgcn_set_error("lgcn_ctx_set_inbatch_mix: mixed negatives need the in-batch softmax loss (inbatch) set on the context first (lgcn_ctx_set_loss with LGCN_LOSS_INBATCH)");
        return 3;
    }
    if (R_max > ctx->ib_mix) {      // grow only: the new block first, so a failure changes nothing
        HIP_OK(hipDeviceSynchronize());     // steps in flight still read the old block
        void *ws = nullptr;
        if (hipMalloc(&ws, sizeof(float) * InBatchWs(ctx->ib_cap, ctx->c.d, R_max).words) != hipSuccess) {
            (void)hipGetLastError();
            lgcn_set_error("lgcn_ctx_set_inbatch_mix: cannot allocate the workspace of the mixed in-batch step: (2 + R_max) * max_batch * d * 4 bytes and a few vectors");
            return 4;
        }
        (void)hipFree(ctx->ib_ws);
        ctx->ib_ws = ws;
    }
    ctx->ib_mix = R_max;
    return 0;
}
extern "C" int32_t lgcn_ctx_get_inbatch_mix(const lgcn_ctx *ctx) { return ctx ? ctx->ib_mix : -1; }
extern "C" int32_t lgcn_ctx_get_loss(const lgcn_ctx *ctx, float *temperature_out) {
    if (!ctx) return -1;
    if (temperature_out) *temperature_out = ctx->loss_temp;
    return ctx->loss_kind;
}
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
// The alignment-and-uniformity loss: refused where the in-batch loss is, in the same words; the workspace first
extern "C" int lgcn_ctx_set_directau(lgcn_ctx *ctx, float gamma) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_directau: null context"); return 3; }
    const char *what = "the alignment-and-uniformity loss (directau)";
    char buf[256];
    const char *fmt = nullptr;
    if (!(gamma >= 0.f) || !isfinite(gamma)) fmt = "lgcn_ctx_set_directau: %s needs a finite gamma >= 0";
    else if (ctx->hn_m) fmt = "lgcn_ctx_set_directau: hard negatives (lgcn_ctx_set_hard_neg) are set on this context and train the BPR loss only, not %s";
    else if (ctx->ib_mix) fmt = "lgcn_ctx_set_directau: mixed negatives (lgcn_ctx_set_inbatch_mix) are set on this context and belong to the in-batch softmax loss, not to %s";
    else if (ctx->c.act_dtype == LGCN_FP8) fmt = "lgcn_ctx_set_directau: %s is not implemented for LGCN_FP8 activation storage";
    else if (ctx->variant) fmt = "lgcn_ctx_set_directau: %s is not implemented with the optional branches (item-item smoothing / popularity gate)";
    else if (!ctx->c.dense_last) fmt = "lgcn_ctx_set_directau: %s needs a context with dense_last = 1 (the gathered last layer has no 2 B slot form)";
    if (fmt) { snprintf(buf, sizeof buf, fmt, what); lgcn_set_error(buf); return 3; }
    if (!ctx->au_ws) {                  // the workspace is allocated once, before anything is changed
        const int32_t cap = lgcn_inbatch_rows(ctx->c.max_batch);
        void *ws = nullptr;
        if (hipMalloc(&ws, sizeof(float) * DirectAuWs(cap, ctx->c.d).words) != hipSuccess) {
            (void)hipGetLastError();
            lgcn_set_error("lgcn_ctx_set_directau: cannot allocate the workspace of the alignment-and-uniformity loss (directau): 2 * max_batch * d * 4 bytes and a few vectors");
            return 4;
        }
        ctx->au_ws = ws; ctx->au_cap = cap;
    }
    ctx->loss_kind = LGCN_LOSS_DIRECTAU; ctx->loss_temp = 1.f; ctx->au_gamma = gamma;
    return 0;
}
extern "C" int lgcn_ctx_get_directau(const lgcn_ctx *ctx, float *gamma) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_get_directau: null context"); return 3; }
    if (ctx->loss_kind != LGCN_LOSS_DIRECTAU) { lgcn_set_error("lgcn_ctx_get_directau: the alignment-and-uniformity loss (directau) is not set on this context (lgcn_ctx_set_directau)"); return 3; }
    if (gamma) *gamma = ctx->au_gamma;
    return 0;
}
// Hard negatives, DNS(M, N).  Everything is checked before anything changes; top_m = 0 leaves the allocation in
// place and restores exactly the launches of a context that was never told.
extern "C" int lgcn_ctx_set_hard_neg(lgcn_ctx *ctx, int32_t top_m, uint64_t seed, int32_t *sel_out) {
    if (!ctx) { lgcn_set_error("lgcn_ctx_set_hard_neg: null context"); return 3; }
    if (top_m == 0) { ctx->hn_m = 0; ctx->hn_seed = 0; ctx->hn_out = nullptr; return 0; }
    char buf[256];
    const char *fmt = nullptr;
    if (top_m < 0 || top_m > LGCN_MAX_NEG_RATIO) fmt = "lgcn_ctx_set_hard_neg: hard negatives: top_m = %d is out of range (0 = off, or 1..%d)";
    else if (ctx->loss_kind != LGCN_LOSS_BPR) fmt = "lgcn_ctx_set_hard_neg: hard negatives train the BPR loss only, and another loss is set on this context (lgcn_ctx_set_loss)";
    else if (ctx->c.act_dtype == LGCN_FP8) fmt = "lgcn_ctx_set_hard_neg: hard negatives are not implemented for LGCN_FP8 activation storage";
    else if (ctx->variant) fmt = "lgcn_ctx_set_hard_neg: hard negatives are not implemented with the optional branches (item-item smoothing / popularity gate)";
    else if (!ctx->c.dense_last) fmt = "lgcn_ctx_set_hard_neg: hard negatives need a context with dense_last = 1 (the gathered last layer has no 2 + R slot form)";
    if (fmt) { snprintf(buf, sizeof buf, fmt, (int)top_m, LGCN_MAX_NEG_RATIO); lgcn_set_error(buf); return 3; }
    if (!ctx->hn_sel && hipMalloc((void **)&ctx->hn_sel, sizeof(int32_t) * (size_t)ctx->c.max_batch) != hipSuccess) {
        (void)hipGetLastError();
        ctx->hn_sel = nullptr;
        lgcn_set_error("lgcn_ctx_set_hard_neg: cannot allocate the selected ids of hard negatives (max_batch * 4 bytes)");
        return 4;
    }
    ctx->hn_m = top_m; ctx->hn_seed = seed; ctx->hn_out = sel_out;
    return 0;
}
extern "C" int32_t lgcn_ctx_get_hard_neg(const lgcn_ctx *ctx) { return ctx ? ctx->hn_m : -1; }
extern "C" uint32_t lgcn_hard_neg_rank(uint64_t seed, int64_t step, int32_t b, int32_t M) { return lgcn_hn_rank(seed, step, b, M); }
// today's three-slot kernels, and every form that splits a step over ranks, compute BPR: say so instead of training another
// loss.  The in-batch loss trains through its own two entry points only, so lgcn_train_step_multi / _epoch_multi refuse it too.
// (Declared in lgcn_internal.h: lgcn_train_step_i64 in lgcn_ids.hip refuses in the same words.)
// Hard negatives (lgcn_ctx_set_hard_neg) train through lgcn_train_step_multi / _epoch_multi only: the same callers refuse them here.
int lgcn_refuse_loss(const lgcn_ctx *x, const char *who) {
    if (!x || (x->loss_kind == LGCN_LOSS_BPR && !x->hn_m)) return 0;
    char buf[256];
    if (x->hn_m)
        snprintf(buf, sizeof buf, "%s: hard negatives (lgcn_ctx_set_hard_neg) are implemented for lgcn_train_step_multi / lgcn_train_epoch_multi only", who);
    else if (x->loss_kind == LGCN_LOSS_INBATCH)
        snprintf(buf, sizeof buf, "%s: the in-batch softmax loss (inbatch; lgcn_ctx_set_loss) is implemented for lgcn_train_step_inbatch / lgcn_train_epoch_inbatch only", who);
    else if (x->loss_kind == LGCN_LOSS_DIRECTAU)
        snprintf(buf, sizeof buf, "%s: the alignment-and-uniformity loss (directau; lgcn_ctx_set_directau) is implemented for lgcn_train_step_directau / lgcn_train_epoch_directau only", who);
    else
        snprintf(buf, sizeof buf, "%s: the sampled-softmax loss (lgcn_ctx_set_loss) is implemented for lgcn_train_step_multi / lgcn_train_epoch_multi only", who);
    lgcn_set_error(buf);
    return 3;
}

static SpmmArgs base_spmm(const lgcn_ctx *x) {
    SpmmArgs a = graph_spmm(x->c.graph);
    a.G64 = (long long *)x->c.G64; a.G32 = x->g32; a.bitmap = x->c.bitmap + x->flip * x->bm_words;
    a.div = (float)(x->c.K + 1); a.remap = x->c.xcd_remap;
    return a;
}

// forward layers X_1..X_{K-1}
static int run_forward(lgcn_ctx *x, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    { int rc0 = graph_acquire(c.graph, st); if (rc0) return rc0; }
    const void *prev = c.E0; int prev_dt = LGCN_F32;
    if (x->e0b && x->fwd_layers >= 1) {                 // bf16 activation storage: layer 1 gathers bf16(E0)
        if (!x->in_loop) x->e0b_fresh = false;          // a single-step call: E0 may have been written by anybody since
        if (!x->e0b_fresh) lgcn_to_bf16_launch(c.E0, x->e0b, x->N * c.d, st);
        x->e0b_fresh = true;
        prev = x->e0b; prev_dt = LGCN_BF16;
    }
    if (x->e0q && x->fwd_layers >= 1) {                 // fp8 activation storage: layer 1 gathers fp8(E0)
        if (!x->in_loop) x->e0b_fresh = false;
        if (!x->e0b_fresh) { int rc = lgcn_to_fp8_launch(c.E0, x->e0q, x->N, c.d, st); if (rc) return rc; }
        x->e0b_fresh = true;
        prev = x->e0q; prev_dt = LGCN_FP8;
    }
    for (int k = 1; k <= x->fwd_layers; k++) {
        SpmmArgs a = base_spmm(x);
        a.X = prev; a.Y = x->act[k]; a.dr = x->dr;
        if (k == x->fwd_layers) {
            // X_{K-1} of the gathered last layer: only the batch-row launch gathers it, and its workgroups have no slice affinity
            // (a dense last layer is read by slot, and the lower layers are gathered by the next one: plain.  fp8 tables: plain too,
            //  the forward instantiations there have no registers to spare for the second store form -- RowStore, lgcn_device.hip)
            if ((x->store_policy & LGCN_STORE_XLAST) && !c.dense_last && c.act_dtype != LGCN_FP8) a.wt = LGCN_STORE_ARG_Y;
            x->wt_fwd = a.wt;
        }
        int rc = lgcn_spmm_launch(a, 0, c.d, prev_dt, c.act_dtype, st);
        if (rc) return rc;
        prev = x->act[k]; prev_dt = c.act_dtype;
    }
    return 0;
}

static int run_bpr(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                   int32_t B_global, int32_t b_off, int32_t B_local, int32_t shard, bool atomics, bool exchange, hipStream_t st,
                   bool count_slots = true, int cols_phase = 0) {
    const lgcn_train_config &c = x->c;
    BprArgs a{};
    a.reg_ego = c.reg_ego; a.cnt = (atomics && count_slots) ? x->cnt : nullptr;
    a.dr = x->dr;
    const bool wts = x->lw_n != 0;
    for (int k = 0; k < x->lw_n; k++) a.w[k] = x->lw[k];
    a.cols_phase = cols_phase; a.erows = c.contrib; a.colsum = x->colsum;
    a.indptr = c.graph->indptr; a.indices = c.graph->indices; a.vals = c.graph->vals; a.X0 = c.E0; a.K = c.K;
    for (int k = 1; k <= x->fwd_layers; k++) a.Xl[k] = x->act[k];
    a.dense_last = c.dense_last;
    a.n_users = c.n_users; a.N = x->N;
    a.users = users + b_off; a.pos = pos + b_off; a.neg = neg + b_off;
    a.B_local = B_local; a.shard = shard;
    a.inv_B = 1.0f / (float)B_global; a.lam = c.decay / (float)B_global;
    a.G64 = atomics ? (long long *)c.G64 : nullptr; a.bitmap = c.bitmap + x->flip * x->bm_words;
    a.stale_bitmap = c.bitmap + (x->flip ^ 1) * x->bm_words; a.bitmap_words = x->bm_words;
    a.contrib = c.contrib; a.terms = c.terms; a.err = c.err; a.exchange = exchange ? 1 : 0;
    a.terms_off = exchange ? 0 : b_off; a.terms_stride = B_global;
    if (x->fold_mult && atomics && !exchange && cols_phase == 0 && b_off == 0 && B_local == B_global) {
        // a step of lgcn_train_epoch with the fold: the launch below also writes the fp32 copies of its gradient rows
        a.mult = x->fold_mult; a.G32 = x->g32; a.gdiv = x->lw_n ? 1.f : (float)(c.K + 1); a.arrive = x->arrive;
    }
    if (cols_phase == 2)        // column shard, after the all-reduce: loss terms + gradient scatter from the stored slot rows
        return B_local <= 0 ? 0 : lgcn_triplet_launch(a, c.d, c.act_dtype, wts, false, st);
    if (x->hub_graph && !c.dense_last && B_local > 0) {
        // last layer of the hub rows, X_K[hub] = (A_hat X_{K-1})[hub] in fp32, into the library's [N,d] table (free until k_g32)
        { int rc0 = graph_acquire(x->hub_graph, st); if (rc0) return rc0; }
        SpmmArgs h = graph_spmm(x->hub_graph);
        h.X = c.K == 1 ? (const void *)c.E0 : x->act[c.K - 1]; h.Y = x->g32; h.remap = c.xcd_remap; h.dr = x->dr;
        int rc = lgcn_spmm_launch(h, 0, c.d, c.K == 1 ? LGCN_F32 : c.act_dtype, LGCN_F32, st);
        if (rc) return rc;
        a.Xhub = x->g32; a.hub_nnz = x->hub_nnz;
    }
    if (B_local <= 0) {
        // a rank whose shard of a short last batch is empty launches nothing, but the row bitmap of
        // two steps ago still has to be cleared (k_triplet / k_triplet_dense does it on the other ranks)
        HIP_OK(hipMemsetAsync(a.stale_bitmap, 0, sizeof(uint32_t) * (size_t)x->bm_words, st));
        return 0;
    }
    return lgcn_triplet_launch(a, c.d, c.act_dtype, wts, big_table(x->N, c.d), st);
}

// floats per rank of the data-parallel exchange block for a shard of S triplets: [3*S*d gradient rows | S loss | S reg terms], with
// the popularity gate also [S entropy terms | pad to an even count | 2*P floats = P int64: the rank's fixed-point MLP gradient sums]
static int64_t dp_block_floats(const lgcn_ctx *x, int64_t S) {
    int64_t n = 3 * S * x->c.d + 2 * S;
    if (x->variant && x->c.item_pop) { n += S; n += n & 1; n += 2 * (int64_t)x->gate_P; }
    return n;
}
static int64_t dp_block_tail(const lgcn_ctx *x, int64_t S) {          // float offset of the int64 tail inside a block
    int64_t n = 3 * S * x->c.d + 3 * S;
    return n + (n & 1);
}
extern "C" int64_t lgcn_dp_block_floats(const lgcn_ctx *x, int32_t B_global, int32_t world) {
    if (!x || B_global <= 0 || world < 1) return 0;
    return dp_block_floats(x, (B_global + world - 1) / world);
}

// The optional branches' forward tail and loss: T = mean of the K+1 dense layers, item-item smoothing, then the loss on the
// ONE final table (popularity gate inside k_triplet_gate).  The batch slice [b_off, b_off + B_local) of a global batch of
// B_global triplets (single GPU: the whole batch); atomics: into G64 / the row flags; exchange: into the exchange block.
static int run_variant_loss(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B_global,
                            int32_t b_off, int32_t B_local, int32_t shard, bool atomics, bool exchange, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    const int64_t m_items = x->N - c.n_users;
    float *items_mean = c.i2i ? x->g32 : x->tvar;           // with smoothing the item block of T is an SpMM input first
    MeanSplitArgs m{};
    m.X0 = c.E0; m.K = c.K; m.out_u = x->tvar; m.out_i = items_mean;
    for (int k = 1; k <= c.K; k++) m.Xl[k] = x->act[k];
    m.n4_users = (int64_t)c.n_users * c.d / 4; m.n4 = x->N * c.d / 4;
    lgcn_mean_layers_launch(m, c.act_dtype, st);
    if (c.i2i) {            // items = T_items + (alpha I2I) T_items   (model.py:228-229)
        { int rc0 = graph_acquire(c.i2i, st); if (rc0) return rc0; }
        SpmmArgs h = graph_spmm(c.i2i);
        h.X = x->g32 + (int64_t)c.n_users * c.d; h.selfX = (const float *)h.X; h.Y = x->tvar + (int64_t)c.n_users * c.d; h.remap = c.xcd_remap;
        int rc = lgcn_spmm_launch(h, M_ADDSELF, c.d, LGCN_F32, LGCN_F32, st);
        if (rc) return rc;
        HIP_OK(hipMemsetAsync(x->item_bitmap, 0, sizeof(uint32_t) * (size_t)((m_items + 31) / 32), st));
    }
    uint32_t *bm = c.bitmap + x->flip * x->bm_words, *stale = c.bitmap + (x->flip ^ 1) * x->bm_words;
    const int64_t tail = dp_block_tail(x, shard);
    if (B_local <= 0) {     // an empty shard: nothing to launch, but the stale bitmap must go and the block's MLP sums must read zero
        HIP_OK(hipMemsetAsync(stale, 0, sizeof(uint32_t) * (size_t)x->bm_words, st));
        if (exchange && c.item_pop) HIP_OK(hipMemsetAsync(c.contrib + tail, 0, sizeof(long long) * (size_t)x->gate_P, st));
        return 0;
    }
    if (c.item_pop) {
        GateArgs g{};
        g.E = x->tvar; g.item_pop = c.item_pop; g.params = c.gate_params; g.partials = x->gate_partials;
        g.Hp = c.pop_hidden; g.Hg = c.gate_hidden; g.P = x->gate_P;
        g.inv_temp = 1.0f / c.pop_gate_temp; g.ent_scale = c.gate_entropy_coeff / (float)(2 * B_global);
        g.n_users = c.n_users; g.N = x->N; g.users = users + b_off; g.pos = pos + b_off; g.neg = neg + b_off; g.B = B_local;
        g.inv_B = 1.0f / (float)B_global; g.lam = c.decay / (float)B_global;
        g.G64 = atomics ? (long long *)c.G64 : nullptr; g.bitmap = bm; g.item_bitmap = c.i2i ? x->item_bitmap : nullptr;
        g.stale_bitmap = stale; g.bitmap_words = x->bm_words; g.terms = c.terms + (exchange ? 0 : b_off); g.terms_stride = B_global; g.err = c.err;
        g.contrib = c.contrib; g.shard = shard; g.exchange = exchange ? 1 : 0;
        if (int rc = lgcn_gate_launch(g, c.d, st)) return rc;
        if (exchange)       // this rank's MLP gradient sums into the tail of its exchange block
            lgcn_gate_rank_total_launch((const long long *)x->gate_partials, (int32_t)((B_local + GATE_TPB - 1) / GATE_TPB), x->gate_P,
                                        (long long *)(c.contrib + tail), st);
    } else {
        BprArgs a{};
        a.X0 = x->tvar; a.K = 0; a.dense_last = 1;            // e = the row of the final table
        a.n_users = c.n_users; a.N = x->N; a.users = users + b_off; a.pos = pos + b_off; a.neg = neg + b_off; a.B_local = B_local; a.shard = shard;
        a.inv_B = 1.0f / (float)B_global; a.lam = c.decay / (float)B_global;
        a.G64 = atomics ? (long long *)c.G64 : nullptr; a.bitmap = bm; a.stale_bitmap = stale; a.bitmap_words = x->bm_words;
        a.item_bitmap = x->item_bitmap; a.terms = c.terms; a.err = c.err; a.terms_off = exchange ? 0 : b_off; a.terms_stride = B_global;
        a.contrib = c.contrib; a.exchange = exchange ? 1 : 0;
        return lgcn_triplet_launch(a, c.d, LGCN_F32, false, false, st);
    }
    return 0;
}

static SlotArgs slot_args(const lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B,
                          const float *gathered, int32_t shard, int32_t world, float *loss_out) {
    const lgcn_train_config &c = x->c;
    SlotArgs s{};
    s.users = users; s.pos = pos; s.neg = neg; s.B = B; s.n_users = c.n_users; s.N = x->N;
    s.G64 = (long long *)c.G64; s.G32 = x->g32; s.div = x->lw_n ? 1.f : (float)(c.K + 1);      // layer weights: G32 = G, the launches scale it
    s.bitmap = c.bitmap + x->flip * x->bm_words; s.gathered = gathered; s.shard = shard; s.world = world;
    s.terms = c.terms; s.loss_out = loss_out; s.decay = c.decay; s.skip_rank = -1;
    s.ent_coeff = c.item_pop ? c.gate_entropy_coeff : 0.f;
    s.blk = gathered ? dp_block_floats(x, shard) : 0;
    s.item_bitmap = (x->variant && c.i2i) ? x->item_bitmap : nullptr;
    s.cnt = x->cnt;
    return s;
}
static SlotArgsMulti slot_args_multi(const lgcn_ctx *x, const int32_t *users, const int32_t *pos, int32_t B, float *loss_out) {
    SlotArgsMulti m{};
    m.s = slot_args(x, users, pos, nullptr, B, nullptr, B, 1, loss_out);
    m.negs = x->mn.negs; m.neg_stride = x->mn.stride; m.R = x->mn.R;
    return m;
}
// buffer the backward layer k writes (k > 1): ping-pong inside the activation workspace (forward
// activations are dead by then)
static void *bwd_buffer(const lgcn_ctx *x, int k) {
    return (x->c.K == 2) ? x->act[1] : x->act[1 + ((x->c.K - k) & 1)];
}

// One layer of the Horner chain h_{k-1} = Gs + A h_k (k = K: sparse input Gs; k = 1: feeds Adam).
// fused_finish: the Adam launch also zeroes the G64 rows it consumes and reduces the loss (single-GPU
// and batch-sharded steps, where every rank runs every row); the row-sharded step finishes separately.
static int backward_layer(lgcn_ctx *x, int k, const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B,
                          const float *gathered, int32_t shard, float *loss_out, bool fused_finish, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    const bool first = (k == c.K), last = (k == 1);
    if (first) {        // every contribution is in G64 by now: convert the batch rows once (the fold: k_triplet has done it)
        if (x->mn.on) {     // several negatives per positive, or the in-batch loss (R = 0): (2 + R) B slots, never folded
            SlotArgsMulti s = slot_args_multi(x, users, pos, B, loss_out);
            if (int rc = lgcn_g32_multi_launch(s, c.d, st)) return rc;
        } else if (!x->fold_mult) {
            SlotArgs s = slot_args(x, users, pos, neg, B, gathered, shard, 1, loss_out);
            if (int rc = lgcn_g32_launch(s, c.d, st)) return rc;
        }
        if (x->variant && c.i2i) {
            // backward of the smoothing: Gs_items <- Gs_items + (alpha I2I)^T Gs_items, a sparse-input SpMM on the item block; the
            // result is dense, so every item row of Gs counts as non-zero from here on
            { int rc0 = graph_acquire(c.i2i_t, st); if (rc0) return rc0; }
            const int64_t ioff = (int64_t)c.n_users * c.d, m_items = x->N - c.n_users;
            SpmmArgs h = graph_spmm(c.i2i_t);
            h.G32 = x->g32 + ioff; h.bitmap = x->item_bitmap; h.Y = x->tvar + ioff; h.div = (float)(c.K + 1); h.remap = c.xcd_remap;
            int rc = lgcn_spmm_launch(h, M_SPARSE | M_ADDG, c.d, LGCN_F32, LGCN_F32, st);
            if (rc) return rc;
            HIP_OK(hipMemcpyAsync(x->g32 + ioff, x->tvar + ioff, sizeof(float) * (size_t)m_items * c.d, hipMemcpyDeviceToDevice, st));
            lgcn_flag_range_launch(c.bitmap + x->flip * x->bm_words, (int64_t)c.n_users, x->N, st);
        }
    }
    SpmmArgs a = base_spmm(x);
    a.dr = x->dr; a.dr.tr = 1;           // the chain multiplies by A_drop^T: the entry stored at (i, j) carries keep(j, i)
    a.X = first ? nullptr : bwd_buffer(x, k + 1);
    if (!last) a.Y = bwd_buffer(x, k);
    else {
        const double bc1 = 1.0 - pow(c.beta1, (double)x->step);
        const double bc2 = 1.0 - pow(c.beta2, (double)x->step);
        a.P = c.E0; a.M = c.adam_m; a.V = c.adam_v;
        a.cnt = x->cnt; a.lam = c.decay / (float)B;
        if (x->mn.R > 0) a.lam = c.decay / (float)((int64_t)B * x->mn.R);      // the counts are R per user / positive slot, 1 per negative slot
        // inside a multi-step call on replicated tables the epilogue keeps the bf16 copy of E0 current (row-sharded steps
        // update only the owned rows and convert again after the exchange)
        a.Pb = (x->e0b && x->in_loop && fused_finish) ? x->e0b : nullptr;
        a.Pq = (x->e0q && x->in_loop && fused_finish) ? x->e0q : nullptr;
        x->e0b_fresh = a.Pb != nullptr || a.Pq != nullptr;
        // nothing gathers M or V; P is gathered (layer 1, with slice affinity) unless this launch keeps a shadow for that
        if (x->store_policy & LGCN_STORE_ADAM) a.wt = LGCN_STORE_ARG_MV | ((a.Pb || a.Pq) ? LGCN_STORE_ARG_P : 0);
        x->wt_adam = a.wt;
        a.step_size = (float)(c.lr / bc1); a.bc2_sqrt = (float)sqrt(bc2);
        a.w1 = (float)(1.0 - c.beta1); a.beta2 = (float)c.beta2; a.omb2 = (float)(1.0 - c.beta2); a.eps = (float)c.eps;
        if (!first && fused_finish) {       // K >= 2: this launch also cleans the workspace and reduces the loss
            a.clear = 1; a.terms = c.terms; a.gathered = gathered; a.loss_out = loss_out;
            a.B = B; a.shard = shard; a.decay = c.decay; a.ent_coeff = c.item_pop ? c.gate_entropy_coeff : 0.f;
            a.blk = gathered ? dp_block_floats(x, shard) : 0;
        }
    }
    const int prev_dt = first ? LGCN_F32 : c.act_dtype;
    int mode = M_ADDG | (first ? M_SPARSE : 0) | (last ? M_ADAM : 0);
    if (x->lw_n) {      // layer weights: h_{k-1} = w_{k-1} G + A h_k, h_K = w_K G (G32 is G unscaled; the first layer gathers it)
        a.w_in = first ? x->lw[c.K] : 1.f; a.w_add = x->lw[k - 1];
        mode |= M_WTS;
    }
    return lgcn_spmm_launch(a, mode, c.d, prev_dt, last ? LGCN_F32 : c.act_dtype, st);
}

// [DP scatter] + backward chain + Adam + finish
// gate_reduced: the MLP gradient of the global batch is the all-reduced gate_total (dense data-parallel form)
static int run_backward(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B,
                        const float *gathered, int32_t shard, int32_t world, float *loss_out, hipStream_t st, bool gate_reduced = false) {
    const lgcn_train_config &c = x->c;
    { int rc0 = graph_acquire(c.graph, st); if (rc0) return rc0; }
    SlotArgs s = slot_args(x, users, pos, neg, B, gathered, shard, world, loss_out);
    if (gathered) {
        s.skip_rank = x->dp_local ? x->dp_rank : -1;       // part 1 already added this rank's own rows
        if (int rc = lgcn_scatter_launch(s, c.d, st)) return rc;
    }
    x->step += 1;
    // Horner: h_{K-1} = Gs + A Gs (sparse input); h_{k-1} = Gs + A h_k; last one feeds Adam
    for (int k = c.K; k >= 1; k--) {
        int rc = backward_layer(x, k, users, pos, neg, B, gathered, shard, loss_out, true, st);
        if (rc) return rc;
    }
    if (x->variant && c.item_pop) {          // torch.optim.Adam on the gate's MLP parameters, same step count as the tables
        GateAdamArgs ga{};
        if (gathered) {      // data parallel: the ranks' totals sit in the tails of their exchange blocks
            ga.src = (const long long *)(gathered + dp_block_tail(x, shard)); ga.n_src = world; ga.stride = dp_block_floats(x, shard) / 2;
        } else if (gate_reduced) {             // dense form: the all-reduced total
            ga.src = x->gate_total; ga.n_src = 1; ga.stride = x->gate_P;
        } else { ga.src = x->gate_partials; ga.n_src = (B + GATE_TPB - 1) / GATE_TPB; ga.stride = x->gate_P; }
        ga.P = x->gate_P;
        ga.params = c.gate_params; ga.m = c.gate_adam_m; ga.v = c.gate_adam_v; ga.grad_out = c.gate_grad;
        const double bc1 = 1.0 - pow(c.beta1, (double)x->step), bc2 = 1.0 - pow(c.beta2, (double)x->step);
        ga.step_size = (float)(c.lr / bc1); ga.bc2_sqrt = (float)sqrt(bc2);
        ga.w1 = (float)(1.0 - c.beta1); ga.beta2 = (float)c.beta2; ga.omb2 = (float)(1.0 - c.beta2); ga.eps = (float)c.eps;
        lgcn_gate_adam_launch(ga, st);
    }
    if (c.K >= 2) { x->flip ^= 1; return 0; }       // next step flags rows in the other bitmap
    if (x->mn.on) {
        SlotArgsMulti sm = slot_args_multi(x, users, pos, B, loss_out);
        return lgcn_finish_multi_launch(sm, c.d, st);
    }
    if (int rc = lgcn_finish_launch(s, c.d, st)) return rc;
    if (x->variant && c.i2i) {
        // K = 1 keeps ONE bitmap (k_finish clears the batch rows' words); the smoothing's backward flagged EVERY item row in it
        // and zeroed nothing of G64 beyond the batch rows, which k_finish has just done: clear the whole bitmap
        HIP_OK(hipMemsetAsync(c.bitmap + x->flip * x->bm_words, 0, sizeof(uint32_t) * (size_t)x->bm_words, st));
    }
    return 0;
}

// What the batch-row launch of every slot-form step takes (lgcn_multineg.hip, lgcn_inbatch.hip), from the context and the slot
// form of the running step (x->mn).  Without negatives (the plain in-batch step) inv_BR, inv_R and lam_n stay 0; under
// LGCN_LOSS_BPR tau and inv_tauB do
static MultiNegArgs multineg_args(const lgcn_ctx *x, const int32_t *users, const int32_t *pos, int32_t B) {
    const lgcn_train_config &c = x->c;
    MultiNegArgs a{};
    a.X0 = c.E0; a.K = c.K;
    for (int k = 1; k <= x->fwd_layers; k++) a.Xl[k] = x->act[k];
    a.n_users = c.n_users; a.N = x->N;
    a.users = users; a.pos = pos; a.negs = x->mn.negs; a.neg_stride = x->mn.stride; a.R = x->mn.R; a.B = B;
    a.lam = c.decay / (float)B;
    if (x->mn.R > 0) {
        const float BR = (float)((int64_t)B * x->mn.R);
        a.inv_BR = 1.0f / BR; a.inv_R = 1.0f / (float)x->mn.R; a.lam_n = c.decay / BR;
    }
    a.G64 = (long long *)c.G64; a.bitmap = c.bitmap + x->flip * x->bm_words;
    a.stale_bitmap = c.bitmap + (x->flip ^ 1) * x->bm_words; a.bitmap_words = x->bm_words;
    a.terms = c.terms; a.terms_stride = B; a.err = c.err;
    a.reg_ego = c.reg_ego; a.cnt = x->cnt;
    for (int k = 0; k < x->lw_n; k++) a.w[k] = x->lw[k];
    a.loss = x->loss_kind;
    if (x->loss_kind != LGCN_LOSS_BPR) {       // the same rows, flags and terms; another coefficient per negative
        a.tau = x->loss_temp; a.inv_tauB = (float)(1.0 / ((double)x->loss_temp * (double)B));
    }
    return a;
}

// The four launches of lgcn_inbatch.hip: the plain step on the plain carving of the workspace, a step with
// negatives on the mixed carving for the context's R_max, with the pool's (1 + R_max) cap item rows
static int run_inbatch(lgcn_ctx *x, const int32_t *users, const int32_t *pos, int32_t B, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    const bool mix = x->mn.R > 0;
    const InBatchWs ws(x->ib_cap, c.d, mix ? x->ib_mix : 0);
    float *w = (float *)x->ib_ws;
    InBatchArgs ia{};
    ia.m = multineg_args(x, users, pos, B);
    ia.cap = x->ib_cap;
    ia.U = w + ws.U; ia.P = w + ws.P; ia.sbb = w + ws.sbb;
    ia.uid = (int32_t *)(w + ws.uid); ia.pid = (int32_t *)(w + ws.pid);
    ia.mrg = w + ws.mrg; ia.part = w + ws.part;
    if (mix) { ia.mix = 1; ia.icap = (int32_t)ws.icap; ia.xinvu = w + ws.invu; ia.xinvp = w + ws.invp; ia.xlq = w + ws.lq; }
    ia.score = x->ib_score; ia.item_logq = x->ib_logq;
    return lgcn_inbatch_launch(ia, c.d, c.act_dtype, x->lw_n != 0, st);
}

// The four launches of lgcn_directau.hip on the context's own workspace
static int run_directau(lgcn_ctx *x, const int32_t *users, const int32_t *pos, int32_t B, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    const DirectAuWs ws(x->au_cap, c.d);
    float *w = (float *)x->au_ws;
    DirectAuArgs da{};
    da.m = multineg_args(x, users, pos, B);
    da.m.tau = 0.f; da.m.inv_tauB = 0.f;      // (no temperature in this loss)
    da.cap = x->au_cap; da.gamma = x->au_gamma;
    da.X = w + ws.X; da.Y = w + ws.Y; da.invx = w + ws.invx; da.invy = w + ws.invy; da.qx = w + ws.qx; da.qy = w + ws.qy; da.al = w + ws.al;
    da.uid = (int32_t *)(w + ws.uid); da.pid = (int32_t *)(w + ws.pid); da.part = w + ws.part; da.scal = w + ws.scal;
    return lgcn_directau_launch(da, c.d, c.act_dtype, x->lw_n != 0, st);
}

// One training step on one GPU: the drop mask, the forward layers, the loss launch of the step's form -- three slots (BPR or
// the optional branches) unless a SlotScope is open, else the batch-row launch of the context's loss -- and the backward
static int run_step(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B, float *loss_out, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    int rc;
    x->dr = make_drop(x->drop_keep, x->drop_seed, x->step, 0);        // ONE mask per step, from the counter before the step
    if ((rc = run_forward(x, st))) return rc;
    if (!x->mn.on) rc = x->variant ? run_variant_loss(x, users, pos, neg, B, 0, B, B, true, false, st) : run_bpr(x, users, pos, neg, B, 0, B, B, true, false, st);
    else if (x->loss_kind == LGCN_LOSS_INBATCH) rc = run_inbatch(x, users, pos, B, st);
    else if (x->loss_kind == LGCN_LOSS_DIRECTAU) rc = run_directau(x, users, pos, B, st);
    else if (x->hn_m) {
        // hard negatives: the launch picks one candidate per sample and from there on the step IS the three-slot step on (users,
        // pos, hn_sel) -- its slot kernels, cnt slots of weight 1, decay / B -- so the slot form ends here.  k_g32 is launched,
        // never folded: which rows the batch touches is not known ahead
        HardNegArgs h{};
        h.m = multineg_args(x, users, pos, B);
        h.inv_B = 1.0f / (float)B; h.top_m = x->hn_m; h.seed = x->hn_seed; h.step = x->step;      // the counter before the step, as the drop mask's
        h.sel_id = x->hn_sel; h.sel_out = x->hn_out;
        rc = lgcn_hardneg_launch(h, c.d, c.act_dtype, x->lw_n != 0, st);
        x->mn = {};
        neg = x->hn_sel;
    }
    else rc = lgcn_multineg_launch(multineg_args(x, users, pos, B), c.d, c.act_dtype, x->lw_n != 0, st);
    if (rc) return rc;
    if ((rc = run_backward(x, users, pos, neg, B, nullptr, B, 1, loss_out, st))) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

static int check_batch(const lgcn_ctx *x, const void *u, const void *p, const void *n, int32_t B) {
    if (!x || !u || !p || !n) { lgcn_set_error("train step: null argument"); return 3; }
    if (B <= 0 || B > x->c.max_batch) { lgcn_set_error("train step: batch size out of range (0 < B <= max_batch)"); return 3; }
    return 0;
}

extern "C" int lgcn_train_step(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                               int32_t B, float *loss_out, void *stream) {
    int rc = check_batch(x, users, pos, neg, B);
    if (rc) return rc;
    if ((rc = lgcn_refuse_loss(x, "lgcn_train_step"))) return rc;
    if (!loss_out) { lgcn_set_error("train step: loss_out is null"); return 3; }
    return run_step(x, users, pos, neg, B, loss_out, (hipStream_t)stream);
}

extern "C" int lgcn_train_epoch(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                int64_t T, int32_t B, float *loss_out, void *stream) {
    if (T <= 0) return 0;
    if (!x) { lgcn_set_error("train epoch: null context"); return 3; }
    if (int rc = lgcn_refuse_loss(x, "lgcn_train_epoch")) return rc;
    LoopScope scope(x);
    // The fold of k_g32: the call's triplets are all here, so how many slots of each batch name a row is known
    // before the first step -- one k_slot_mult launch per segment of steps, into the context's buffer -- and k_triplet writes
    // the fp32 copies of the gradient rows itself.  Not with the optional branches (they run another loss kernel), not with a
    // hub plan (its rows live in the same table until k_g32), not where a batch's row ids do not fit the LDS hash
    const bool fold = x->fold_g32 && !x->variant && !x->hub_graph && users && pos && neg &&
                      B > 0 && B <= x->c.max_batch && x->N <= 0x7fffffffLL && slot_mult_hash(B) != 0;
    const int64_t seg = lgcn_fold_segment_steps();
    if (fold) {
        if (!x->arrive) {         // the first call that folds: every other path leaves the context's footprint as it was
            HIP_OK(hipMalloc((void **)&x->arrive, sizeof(int32_t) * (size_t)x->N));
            HIP_OK(hipMemsetAsync(x->arrive, 0, sizeof(int32_t) * (size_t)x->N, (hipStream_t)stream));
        }
        // room for a whole segment of the context's largest batch that folds, whatever this call's length: a longer call
        // later (an epoch after a few warm-up steps) finds the buffer in place, and only a larger segment grows it
        const int64_t bmax = x->c.max_batch < 4096 ? x->c.max_batch : 4096;
        const int64_t need = 3 * (B > bmax ? (int64_t)B : bmax) * seg;
        if (x->mult_cap < need) {
            if (x->mult) (void)hipFree(x->mult);
            x->mult = nullptr; x->mult_cap = 0;
            HIP_OK(hipMalloc((void **)&x->mult, sizeof(uint16_t) * (size_t)need));
            x->mult_cap = need;
        }
    }
    int64_t i = 0, seg_t0 = 0;
    for (int64_t t = 0; t < T; t += B, i++) {
        const int32_t b = (int32_t)((T - t) < B ? (T - t) : B);
        if (fold) {
            if (i % seg == 0) {       // the next segment's multiplicities (the steps that read the last one's are ahead on the stream)
                seg_t0 = t;
                const int64_t Ts = (T - t) < seg * B ? (T - t) : seg * B;
                int rc = lgcn_slot_mult_launch(users + t, pos + t, neg + t, Ts, B, x->c.n_users, x->N, x->mult, (hipStream_t)stream);
                if (rc) return rc;
            }
            x->fold_mult = x->mult + 3 * (t - seg_t0);
        }
        int rc = lgcn_train_step(x, users + t, pos + t, neg + t, b, loss_out + 3 * i, stream);
        x->fold_mult = nullptr;
        if (rc) return rc;
        if (fold) x->folded_steps += 1;
    }
    return 0;
}

// The slot-form steps: several negatives per positive under BPR or the sampled softmax (SLOT_MULTI), the
// in-batch softmax over (users, pos) alone (SLOT_INBATCH; 4.19, 4.20: R = 0, no negatives) and the in-batch softmax with the
// batch's sampled negatives as a shared pool (SLOT_MIX; 4.21).  Everything is checked before anything is launched or counted: a
// refusal leaves the outputs, the step counter and the workspace as they were.
enum SlotKind { SLOT_MULTI, SLOT_INBATCH, SLOT_MIX, SLOT_DIRECTAU };
static int check_slot_step(const lgcn_ctx *x, SlotKind kind, const void *u, const void *p, const void *n, const void *loss_out,
                           int32_t R, int32_t B, int64_t neg_stride, const char *who) {
    char buf[256];
    auto refuse = [&](const char *fmt, int v0 = 0, int v1 = 0) { snprintf(buf, sizeof buf, fmt, who, v0, v1); lgcn_set_error(buf); return 3; };
    const bool negs = kind != SLOT_INBATCH && kind != SLOT_DIRECTAU;
    if (!x || !u || !p || (negs && !n) || !loss_out) return refuse("%s: null argument");
    if (kind == SLOT_MULTI) {
        if (x->loss_kind == LGCN_LOSS_INBATCH || x->loss_kind == LGCN_LOSS_DIRECTAU) return lgcn_refuse_loss(x, who);
        if (R < 1 || R > LGCN_MAX_NEG_RATIO) return refuse("%s: the negative ratio R = %d is out of range (1..%d)", R, LGCN_MAX_NEG_RATIO);
        if (!x->c.dense_last) return refuse("%s: a negative ratio above the three-slot step's needs a context with dense_last = 1 (the gathered last layer has no 2 + R slot form)");
        if (x->c.act_dtype == LGCN_FP8) return refuse("%s: the negative ratio (several negatives per positive) is not implemented for LGCN_FP8 activation storage");
        if (x->variant) return refuse("%s: the negative ratio (several negatives per positive) is not implemented with the optional branches (item-item smoothing / popularity gate)");
        if (x->hn_m && (R < 2 || x->hn_m > R))
            return refuse("%s: hard negatives pick among the M = %d hardest of R >= 2 candidates with M <= R: the negative ratio R = %d does not fit (lgcn_ctx_set_hard_neg)", x->hn_m, R);
    } else if (kind == SLOT_DIRECTAU) {
        if (x->hn_m) return lgcn_refuse_loss(x, who);
        if (x->loss_kind != LGCN_LOSS_DIRECTAU || !x->au_ws) return refuse("%s: the alignment-and-uniformity loss (directau) is not set on this context (lgcn_ctx_set_directau)");
    } else {
        if (x->hn_m || x->loss_kind == LGCN_LOSS_DIRECTAU) return lgcn_refuse_loss(x, who);
        if (x->loss_kind != LGCN_LOSS_INBATCH || !x->ib_ws) return refuse("%s: the in-batch softmax loss (inbatch) is not set on this context (lgcn_ctx_set_loss with LGCN_LOSS_INBATCH)");
        if (kind == SLOT_MIX && x->ib_mix < 1) return refuse("%s: mixed negatives are not set on this context (lgcn_ctx_set_inbatch_mix)");
        if (kind == SLOT_MIX && (R < 1 || R > x->ib_mix)) return refuse("%s: the negative ratio R = %d is out of range (1..%d, the R_max of lgcn_ctx_set_inbatch_mix)", R, x->ib_mix);
    }
    if (B <= 0 || B > x->c.max_batch) return refuse("%s: batch size out of range (0 < B <= max_batch)");
    if (negs && neg_stride < B) return refuse("%s: neg_stride must be at least B (negative ratio columns would overlap)");
    return 0;
}

static int slot_step(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *negs, int64_t neg_stride, int32_t R,
                     int32_t B, float *loss_out, void *stream) {
    SlotScope scope(x, negs, neg_stride, R);
    return run_step(x, users, pos, negs, B, loss_out, (hipStream_t)stream);
}
// T samples in batches of B (a short last one), negative column r at negs + r * T (or no negatives); stops at the first failure
static int slot_epoch(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *negs, int32_t R, int64_t T, int32_t B,
                      float *loss_out, void *stream) {
    LoopScope scope(x);
    int64_t i = 0;
    for (int64_t t = 0; t < T; t += B, i++) {
        const int32_t b = (int32_t)((T - t) < B ? (T - t) : B);
        if (int rc = slot_step(x, users + t, pos + t, negs ? negs + t : nullptr, negs ? T : 0, R, b, loss_out + 3 * i, stream)) return rc;
    }
    return 0;
}

extern "C" int lgcn_train_step_multi(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *negs, int64_t neg_stride,
                                     int32_t R, int32_t B, float *loss_out, void *stream) {
    if (int rc = check_slot_step(x, SLOT_MULTI, users, pos, negs, loss_out, R, B, neg_stride, "lgcn_train_step_multi")) return rc;
    return slot_step(x, users, pos, negs, neg_stride, R, B, loss_out, stream);
}
extern "C" int lgcn_train_epoch_multi(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *negs, int32_t R,
                                      int64_t T, int32_t B, float *loss_out, void *stream) {
    if (T <= 0) return 0;
    if (int rc = check_slot_step(x, SLOT_MULTI, users, pos, negs, loss_out, R, B, T < B ? (int64_t)B : T, "lgcn_train_epoch_multi")) return rc;
    return slot_epoch(x, users, pos, negs, R, T, B, loss_out, stream);
}

extern "C" int lgcn_train_step_inbatch(lgcn_ctx *x, const int32_t *users, const int32_t *pos, int32_t B, float *loss_out, void *stream) {
    if (int rc = check_slot_step(x, SLOT_INBATCH, users, pos, nullptr, loss_out, 0, B, 0, "lgcn_train_step_inbatch")) return rc;
    return slot_step(x, users, pos, nullptr, 0, 0, B, loss_out, stream);
}
extern "C" int lgcn_train_epoch_inbatch(lgcn_ctx *x, const int32_t *users, const int32_t *pos, int64_t T, int32_t B, float *loss_out,
                                        void *stream) {
    if (T <= 0) return 0;
    if (int rc = check_slot_step(x, SLOT_INBATCH, users, pos, nullptr, loss_out, 0, B, 0, "lgcn_train_epoch_inbatch")) return rc;
    return slot_epoch(x, users, pos, nullptr, 0, T, B, loss_out, stream);
}

extern "C" int lgcn_train_step_directau(lgcn_ctx *x, const int32_t *users, const int32_t *pos, int32_t B, float *loss_out, void *stream) {
    if (int rc = check_slot_step(x, SLOT_DIRECTAU, users, pos, nullptr, loss_out, 0, B, 0, "lgcn_train_step_directau")) return rc;
    return slot_step(x, users, pos, nullptr, 0, 0, B, loss_out, stream);
}
extern "C" int lgcn_train_epoch_directau(lgcn_ctx *x, const int32_t *users, const int32_t *pos, int64_t T, int32_t B, float *loss_out,
                                         void *stream) {
    if (T <= 0) return 0;
    if (int rc = check_slot_step(x, SLOT_DIRECTAU, users, pos, nullptr, loss_out, 0, B, 0, "lgcn_train_epoch_directau")) return rc;
    return slot_epoch(x, users, pos, nullptr, 0, T, B, loss_out, stream);
}

extern "C" int lgcn_train_step_inbatch_mix(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *negs, int64_t neg_stride,
                                           int32_t R, int32_t B, float *loss_out, void *stream) {
    if (int rc = check_slot_step(x, SLOT_MIX, users, pos, negs, loss_out, R, B, neg_stride, "lgcn_train_step_inbatch_mix")) return rc;
    return slot_step(x, users, pos, negs, neg_stride, R, B, loss_out, stream);
}
extern "C" int lgcn_train_epoch_inbatch_mix(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *negs, int32_t R,
                                            int64_t T, int32_t B, float *loss_out, void *stream) {
    if (T <= 0) return 0;
    if (int rc = check_slot_step(x, SLOT_MIX, users, pos, negs, loss_out, R, B, T < B ? (int64_t)B : T, "lgcn_train_epoch_inbatch_mix")) return rc;
    return slot_epoch(x, users, pos, negs, R, T, B, loss_out, stream);
}

extern "C" int lgcn_train_step_dp_part1(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                        int32_t B_global, int32_t world, int32_t rank, void *stream) {
    int rc = check_batch(x, users, pos, neg, B_global);
    if (rc) return rc;
    if ((rc = refuse_dropout(x, "lgcn_train_step_dp_part1"))) return rc;
    if ((rc = refuse_layer_weights(x, "lgcn_train_step_dp_part1"))) return rc;
    if ((rc = lgcn_refuse_loss(x, "lgcn_train_step_dp_part1"))) return rc;
    if (!x->c.contrib) { lgcn_set_error("dp step: cfg.contrib exchange buffer missing"); return 3; }
    if (world < 1 || rank < 0 || rank >= world) { lgcn_set_error("dp step: bad world/rank"); return 3; }
    const int32_t shard = (B_global + world - 1) / world;
    const int32_t b_off = rank * shard;
    int32_t B_local = B_global - b_off;
    if (B_local > shard) B_local = shard;
    if (B_local < 0) B_local = 0;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = run_forward(x, st))) return rc;
    // with dp_local the rank's own rows go into G64 here (atomics) AND into the exchange block; part 2 scatters the others'
    if (x->variant) rc = run_variant_loss(x, users, pos, neg, B_global, b_off, B_local, shard, x->dp_local, true, st);
    else rc = run_bpr(x, users, pos, neg, B_global, b_off, B_local, shard, x->dp_local, true, st);
    if (rc) return rc;
    x->dp_rank = rank;
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lgcn_train_step_dp_dense_part1(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                              int32_t B_global, int32_t world, int32_t rank, void *stream) {
    int rc = check_batch(x, users, pos, neg, B_global);
    if (rc) return rc;
    if ((rc = refuse_dropout(x, "lgcn_train_step_dp_dense_part1"))) return rc;
    if ((rc = refuse_layer_weights(x, "lgcn_train_step_dp_dense_part1"))) return rc;
    if ((rc = lgcn_refuse_loss(x, "lgcn_train_step_dp_dense_part1"))) return rc;
    if (world < 1 || rank < 0 || rank >= world) { lgcn_set_error("dp step: bad world/rank"); return 3; }
    const int32_t shard = (B_global + world - 1) / world;
    const int32_t b_off = rank * shard;
    int32_t B_local = B_global - b_off;
    if (B_local > shard) B_local = shard;
    if (B_local < 0) B_local = 0;
    hipStream_t st = (hipStream_t)stream;
    const bool gate = x->variant && x->c.item_pop;
    // this rank owns positions [b_off, b_off+B_local) of the global loss-term arrays (loss | reg | with the gate: entropy);
    // the rest must be zero
    HIP_OK(hipMemsetAsync(x->c.terms, 0, sizeof(float) * (gate ? 3 : 2) * (size_t)B_global, st));
    if ((rc = run_forward(x, st))) return rc;
    if (x->variant) {
        // optional branches: the shard's rows go into this rank's G64 by atomics like the default model's; the MLP
        // parameter gradients of the shard are summed (fixed point: any order) into gate_total, one more all-reduce
        if ((rc = run_variant_loss(x, users, pos, neg, B_global, b_off, B_local, shard, true, false, st))) return rc;
        if (gate) {
            if (B_local > 0)
                lgcn_gate_rank_total_launch((const long long *)x->gate_partials, (int32_t)((B_local + GATE_TPB - 1) / GATE_TPB), x->gate_P, x->gate_total, st);
            else HIP_OK(hipMemsetAsync(x->gate_total, 0, sizeof(long long) * (size_t)x->gate_P, st));
        }
    } else if ((rc = run_bpr(x, users, pos, neg, B_global, b_off, B_local, shard, true, false, st, false))) return rc;
    SlotArgs s{};
    s.users = users; s.pos = pos; s.neg = neg; s.B = B_global; s.n_users = x->c.n_users; s.N = x->N;
    s.bitmap = x->c.bitmap + x->flip * x->bm_words; s.cnt = x->cnt;
    s.item_bitmap = (x->variant && x->c.i2i) ? x->item_bitmap : nullptr;      // the smoothing's backward reads the items of the GLOBAL batch
    lgcn_flag_rows_launch(s, st);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lgcn_ctx_gate_total(const lgcn_ctx *x, void **buf, int32_t *count) {
    if (!x || !buf || !count) { lgcn_set_error("lgcn_ctx_gate_total: null argument"); return 3; }
    *buf = x->gate_total; *count = x->gate_total ? x->gate_P : 0;
    return 0;
}

extern "C" int lgcn_train_step_dp_part2(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                        int32_t B_global, int32_t world, const float *gathered, float *loss_out,
                                        void *stream) {
    int rc = check_batch(x, users, pos, neg, B_global);
    if (rc) return rc;
    if ((rc = refuse_dropout(x, "lgcn_train_step_dp_part2"))) return rc;
    if ((rc = refuse_layer_weights(x, "lgcn_train_step_dp_part2"))) return rc;
    if ((rc = lgcn_refuse_loss(x, "lgcn_train_step_dp_part2"))) return rc;
    if (!loss_out || world < 1) { lgcn_set_error("dp step part 2: invalid argument"); return 3; }
    const int32_t shard = (B_global + world - 1) / world;
    // gathered == NULL is the dense form: G64, the terms and (popularity gate) gate_total hold the reduced sums of the global batch
    if ((rc = run_backward(x, users, pos, neg, B_global, gathered, shard, world, loss_out, (hipStream_t)stream, gathered == nullptr))) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------
// Column-sharded data parallelism: rank r holds columns [r d/W, (r+1) d/W) of E0, of the Adam state and of every activation --
// its context is an ordinary context of width d / W over the same graph.  Propagation, the gradient scatter, the backward
// chain and Adam are independent per column; the one thing that is not is the score of a triplet, a dot product over ALL
// columns.  So the step is: part 1 (forward + slot rows + PARTIAL scores / reg terms of this rank's columns), ONE all-reduce
// of 3 B floats, part 2 (loss terms, gradient rows of this rank's columns, backward, Adam).  Per-rank SpMM work falls with
// the world size (rows of d / W elements), which batch sharding cannot offer.  Not bitwise equal to the single-GPU step: the
// dot products are summed in another order (W partial sums); everything else is.
// ---------------------------------------------------------------------------------
extern "C" int lgcn_train_step_cols_part1(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                          int32_t B, float **partials, void *stream) {
    int rc = check_batch(x, users, pos, neg, B);
    if (rc) return rc;
    if ((rc = refuse_dropout(x, "lgcn_train_step_cols_part1"))) return rc;
    if ((rc = refuse_layer_weights(x, "lgcn_train_step_cols_part1"))) return rc;
    if ((rc = lgcn_refuse_loss(x, "lgcn_train_step_cols_part1"))) return rc;
    if (x->variant) { lgcn_set_error("column-sharded step: the popularity gate / item-item smoothing mix columns (MLPs over the row): not supported"); return 3; }
    if (!x->c.contrib) { lgcn_set_error("column-sharded step: cfg.contrib (3*max_batch*d floats: the batch's slot rows) missing"); return 3; }
    hipStream_t st = (hipStream_t)stream;
    if ((rc = run_forward(x, st))) return rc;
    if ((rc = run_bpr(x, users, pos, neg, B, 0, B, B, false, false, st, false, 1))) return rc;
    if (partials) *partials = x->colsum;
    HIP_OK(hipGetLastError());
    return 0;
}
extern "C" int lgcn_train_step_cols_part2(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                          int32_t B, float *loss_out, void *stream) {
    int rc = check_batch(x, users, pos, neg, B);
    if (rc) return rc;
    if ((rc = refuse_dropout(x, "lgcn_train_step_cols_part2"))) return rc;
    if ((rc = refuse_layer_weights(x, "lgcn_train_step_cols_part2"))) return rc;
    if ((rc = lgcn_refuse_loss(x, "lgcn_train_step_cols_part2"))) return rc;
    if (!loss_out) { lgcn_set_error("column-sharded step part 2: loss_out is null"); return 3; }
    hipStream_t st = (hipStream_t)stream;
    if ((rc = run_bpr(x, users, pos, neg, B, 0, B, B, true, false, st, true, 2))) return rc;
    if ((rc = run_backward(x, users, pos, neg, B, nullptr, B, 1, loss_out, st))) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------
// Row-sharded propagation (SURVEY 8e "beyond the contract"; the analogue of the reference's A_split
// row folds, dataloader.py:192-201): the context's graph plan holds only the rows this rank owns; a
// phase computes those rows of one layer, and the owners' rows are exchanged before the next phase.
// ---------------------------------------------------------------------------------
extern "C" int lgcn_rs_phase(lgcn_ctx *x, int32_t phase, int32_t k, const int32_t *users, const int32_t *pos, const int32_t *neg,
                             int32_t B_global, int32_t world, int32_t rank, const float *gathered, float *loss_out, void *stream) {
    int rc = check_batch(x, users, pos, neg, B_global);
    if (rc) return rc;
    if ((rc = refuse_dropout(x, "lgcn_rs_phase"))) return rc;
    if ((rc = refuse_layer_weights(x, "lgcn_rs_phase"))) return rc;
    if ((rc = lgcn_refuse_loss(x, "lgcn_rs_phase"))) return rc;
    if (x->variant) { lgcn_set_error("lgcn_rs_phase: the popularity gate / item-item smoothing run on one GPU only"); return 3; }
    const lgcn_train_config &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    if (world < 1 || rank < 0 || rank >= world) { lgcn_set_error("lgcn_rs_phase: bad world/rank"); return 3; }
    const int32_t shard = (B_global + world - 1) / world;
    if ((rc = graph_acquire(c.graph, st))) return rc;
    switch (phase) {
    case LGCN_RS_FWD: {                               // X_k[owned] = (A X_{k-1})[owned], k = 1..K-1
        if (k < 1 || k > x->fwd_layers) { lgcn_set_error("lgcn_rs_phase: forward layer out of range"); return 3; }
        SpmmArgs a = base_spmm(x);
        // bf16 / fp8 activation storage: layer 1 gathers bf16(E0) / fp8(E0), converted after every exchange of the owners' Adam rows
        const bool shadow = k == 1 && (x->e0b != nullptr || x->e0q != nullptr);
        if (shadow) {
            if (x->e0b) lgcn_to_bf16_launch(c.E0, x->e0b, x->N * c.d, st);
            else if ((rc = lgcn_to_fp8_launch(c.E0, x->e0q, x->N, c.d, st))) return rc;
            x->e0b_fresh = false;
        }
        a.X = k == 1 ? (shadow ? (x->e0b ? (const void *)x->e0b : (const void *)x->e0q) : (const void *)c.E0) : x->act[k - 1]; a.Y = x->act[k];
        rc = lgcn_spmm_launch(a, 0, c.d, k == 1 && !shadow ? LGCN_F32 : c.act_dtype, c.act_dtype, st);
        break;
    }
    case LGCN_RS_BPR: {                               // this rank's batch shard -> cfg.contrib
        if (!c.contrib) { lgcn_set_error("lgcn_rs_phase: cfg.contrib exchange buffer missing"); return 3; }
        const int32_t b_off = rank * shard;
        int32_t B_local = B_global - b_off;
        if (B_local > shard) B_local = shard;
        if (B_local < 0) B_local = 0;
        rc = run_bpr(x, users, pos, neg, B_global, b_off, B_local, shard, false, true, st);
        break;
    }
    case LGCN_RS_SCATTER: {                           // all ranks' gradient rows -> G64 + row flags
        if (!gathered) { lgcn_set_error("lgcn_rs_phase: gathered blocks missing"); return 3; }
        SlotArgs s = slot_args(x, users, pos, neg, B_global, gathered, shard, world, loss_out);
        rc = lgcn_scatter_launch(s, c.d, st);
        break;
    }
    case LGCN_RS_BWD:                                 // h_{k-1}[owned] = Gs + (A h_k)[owned], k = K..1; k = 1: Adam on the owned rows
        if (k < 1 || k > c.K) { lgcn_set_error("lgcn_rs_phase: backward layer out of range"); return 3; }
        if (k == c.K) x->step += 1;
        rc = backward_layer(x, k, users, pos, neg, B_global, gathered, shard, loss_out, false, st);
        break;
    case LGCN_RS_FINISH: {                            // zero the batch rows of G64 + their flags, reduce the loss
        if (!loss_out) { lgcn_set_error("lgcn_rs_phase: loss_out is null"); return 3; }
        SlotArgs s = slot_args(x, users, pos, neg, B_global, gathered, shard, world, loss_out);
        rc = lgcn_finish_launch(s, c.d, st);
        break;
    }
    default: lgcn_set_error("lgcn_rs_phase: unknown phase"); return 3;
    }
    if (rc) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

// what a phase wrote and the owners must exchange: buffer + element type
extern "C" int lgcn_rs_buffer(const lgcn_ctx *x, int32_t phase, int32_t k, void **buf, int32_t *dtype) {
    if (!x || !buf || !dtype) { lgcn_set_error("lgcn_rs_buffer: null argument"); return 3; }
    const lgcn_train_config &c = x->c;
    if (phase == LGCN_RS_FWD && k >= 1 && k <= x->fwd_layers) { *buf = x->act[k]; *dtype = c.act_dtype; return 0; }
    if (phase == LGCN_RS_BWD && k > 1 && k <= c.K) { *buf = bwd_buffer(x, k); *dtype = c.act_dtype; return 0; }
    if (phase == LGCN_RS_BWD && k == 1) { *buf = c.E0; *dtype = LGCN_F32; return 0; }
    lgcn_set_error("lgcn_rs_buffer: this phase exchanges nothing");
    return 3;
}

// every owner broadcasts its two row ranges (users, items) of `buf` in place; one RCCL group
// (an fp8 table: the rows are d bytes each and the owners' row scales, fp32 behind the rows, travel with them)
static int rs_exchange(const RcclApi *api, lgcn_dp *dp, void *buf, int dtype, int d, int64_t n_rows, const int64_t *ranges, hipStream_t st) {
    const size_t es = dtype == LGCN_BF16 ? 2 : dtype == LGCN_FP8 ? 1 : 4;
    const ncclDataType_t nt = dtype == LGCN_BF16 ? ncclBfloat16 : dtype == LGCN_FP8 ? ncclUint8 : ncclFloat32;
    float *scales = dtype == LGCN_FP8 ? (float *)((char *)buf + (size_t)n_rows * d) : nullptr;
    ncclResult_t r = api->GroupStart();
    for (int q = 0; q < dp->world && r == ncclSuccess; q++)
        for (int part = 0; part < 2 && r == ncclSuccess; part++) {
            const int64_t lo = ranges[4 * q + 2 * part], hi = ranges[4 * q + 2 * part + 1];
            if (hi <= lo) continue;
            char *p = (char *)buf + (size_t)lo * d * es;
            r = api->Broadcast(p, p, (size_t)(hi - lo) * d, nt, q, dp->comm, st);
            if (scales && r == ncclSuccess) r = api->Broadcast(scales + lo, scales + lo, (size_t)(hi - lo), ncclFloat32, q, dp->comm, st);
        }
    if (r == ncclSuccess) r = api->GroupEnd(); else (void)api->GroupEnd();
    if (r != ncclSuccess) { lgcn_set_error("RCCL broadcast of owned rows failed"); return 11; }
    return 0;
}

// A whole data-parallel epoch from ONE host call: per global batch, part 1 -> RCCL collective on the
// SAME stream (no host synchronisation, no Python between the kernels and the collective) -> part 2.
static int train_epoch_dp_impl(lgcn_ctx *x, lgcn_dp *dp, const int32_t *users, const int32_t *pos, const int32_t *neg,
                               int64_t T, int32_t B_global, int32_t reduce, const int64_t *row_ranges, float *gathered,
                               float *loss_out, void *stream) {
    if (!x || !dp || !users || !pos || !neg || !loss_out) { lgcn_set_error("lgcn_train_epoch_dp: null argument"); return 3; }
    if (reduce != LGCN_DP_ROWS && reduce != LGCN_DP_DENSE && reduce != LGCN_DP_ROW_SHARDED && reduce != LGCN_DP_COLS) { lgcn_set_error("lgcn_train_epoch_dp: unknown reduce mode"); return 3; }
    if (reduce == LGCN_DP_ROW_SHARDED && !row_ranges) { lgcn_set_error("lgcn_train_epoch_dp: row_ranges missing"); return 3; }
    if (reduce != LGCN_DP_DENSE && reduce != LGCN_DP_COLS && !gathered) { lgcn_set_error("lgcn_train_epoch_dp: gathered workspace missing"); return 3; }
    if (B_global <= 0 || B_global > x->c.max_batch) { lgcn_set_error("lgcn_train_epoch_dp: batch size out of range"); return 3; }
    const RcclApi *api = dp->api;             // RCCL, or the in-process loopback of the tests
    if (!api) { lgcn_set_error("lgcn_train_epoch_dp: communicator without collectives"); return 12; }
    hipStream_t st = (hipStream_t)stream;
    const int world = dp->world, rank = dp->rank;
    LoopScope scope(x);
    struct LocalScope {         // batch-sharded rows mode: every rank adds its own rows itself, k_scatter the other ranks'
        lgcn_ctx *x; bool was;
        LocalScope(lgcn_ctx *x_, bool on) : x(x_), was(x_->dp_local) { x->dp_local = on; x->dp_rank = -1; }
        ~LocalScope() { x->dp_local = was; x->dp_rank = -1; }
    } local_scope(x, reduce == LGCN_DP_ROWS);
    int64_t i = 0;
    for (int64_t t = 0; t < T; t += B_global, i++) {
        const int32_t b = (int32_t)((T - t) < B_global ? (T - t) : B_global);
        int rc;
        ncclResult_t r;
        if (reduce == LGCN_DP_COLS) {
            if ((rc = lgcn_train_step_cols_part1(x, users + t, pos + t, neg + t, b, nullptr, stream))) return rc;
            r = api->AllReduce(x->colsum, x->colsum, (size_t)3 * b, ncclFloat32, ncclSum, dp->comm, st);
            if (r != ncclSuccess) { lgcn_set_error("ncclAllReduce failed"); return 11; }
            if ((rc = lgcn_train_step_cols_part2(x, users + t, pos + t, neg + t, b, loss_out + 3 * i, stream))) return rc;
        } else if (reduce == LGCN_DP_ROW_SHARDED) {
            const int32_t K = x->c.K, d = x->c.d;
            const int32_t *u = users + t, *p = pos + t, *n = neg + t;
            void *buf; int32_t dt;
            for (int k = 1; k <= x->fwd_layers; k++) {
                if ((rc = lgcn_rs_phase(x, LGCN_RS_FWD, k, u, p, n, b, world, rank, nullptr, nullptr, stream))) return rc;
                if ((rc = lgcn_rs_buffer(x, LGCN_RS_FWD, k, &buf, &dt))) return rc;
                if ((rc = rs_exchange(api, dp, buf, dt, d, x->N, row_ranges, st))) return rc;
            }
            if ((rc = lgcn_rs_phase(x, LGCN_RS_BPR, 0, u, p, n, b, world, rank, nullptr, nullptr, stream))) return rc;
            const int64_t S = (b + world - 1) / world, blk = 3 * S * d + 2 * S;
            r = api->AllGather(x->c.contrib, gathered, (size_t)blk, ncclFloat32, dp->comm, st);
            if (r != ncclSuccess) { lgcn_set_error("ncclAllGather failed"); return 11; }
            if ((rc = lgcn_rs_phase(x, LGCN_RS_SCATTER, 0, u, p, n, b, world, rank, gathered, nullptr, stream))) return rc;
            for (int k = K; k >= 1; k--) {
                if ((rc = lgcn_rs_phase(x, LGCN_RS_BWD, k, u, p, n, b, world, rank, gathered, nullptr, stream))) return rc;
                if ((rc = lgcn_rs_buffer(x, LGCN_RS_BWD, k, &buf, &dt))) return rc;
                if ((rc = rs_exchange(api, dp, buf, dt, d, x->N, row_ranges, st))) return rc;
            }
            if ((rc = lgcn_rs_phase(x, LGCN_RS_FINISH, 0, u, p, n, b, world, rank, gathered, loss_out + 3 * i, stream))) return rc;
        } else if (reduce == LGCN_DP_ROWS) {
            if ((rc = lgcn_train_step_dp_part1(x, users + t, pos + t, neg + t, b, world, rank, stream))) return rc;
            const int64_t S = (b + world - 1) / world, blk = dp_block_floats(x, S);
            r = api->AllGather(x->c.contrib, gathered, (size_t)blk, ncclFloat32, dp->comm, st);
            if (r != ncclSuccess) { lgcn_set_error("ncclAllGather failed"); return 11; }
            if ((rc = lgcn_train_step_dp_part2(x, users + t, pos + t, neg + t, b, world, gathered, loss_out + 3 * i, stream))) return rc;
        } else {
            if ((rc = lgcn_train_step_dp_dense_part1(x, users + t, pos + t, neg + t, b, world, rank, stream))) return rc;
            r = api->AllReduce(x->c.G64, x->c.G64, (size_t)x->N * x->c.d, ncclInt64, ncclSum, dp->comm, st);
            const bool gate = x->variant && x->c.item_pop;
            if (r == ncclSuccess) r = api->AllReduce(x->c.terms, x->c.terms, (size_t)(gate ? 3 : 2) * b, ncclFloat32, ncclSum, dp->comm, st);
            if (r == ncclSuccess && gate) r = api->AllReduce(x->gate_total, x->gate_total, (size_t)x->gate_P, ncclInt64, ncclSum, dp->comm, st);
            if (r != ncclSuccess) { lgcn_set_error("ncclAllReduce failed"); return 11; }
            if ((rc = lgcn_train_step_dp_part2(x, users + t, pos + t, neg + t, b, world, nullptr, loss_out + 3 * i, stream))) return rc;
        }
    }
    return 0;
}

extern "C" int lgcn_train_epoch_dp(lgcn_ctx *x, lgcn_dp *dp, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                   int64_t T, int32_t B_global, int32_t reduce, const int64_t *row_ranges, float *gathered,
                                   float *loss_out, void *stream) {
    if (refuse_dropout(x, "lgcn_train_epoch_dp") || refuse_layer_weights(x, "lgcn_train_epoch_dp") || lgcn_refuse_loss(x, "lgcn_train_epoch_dp")) return 3;         // (every rank's context says the same: nobody waits in a collective)
    const int rc = train_epoch_dp_impl(x, dp, users, pos, neg, T, B_global, reduce, row_ranges, gathered, loss_out, stream);
    // a rank that leaves the loop early never reaches its next collective: release the loopback ranks waiting for it
    // (RCCL has its own abort / timeout machinery)
    if (rc && dp && dp->loopback) lgcn_dp_loopback_abort(dp);
    return rc;
}

extern "C" int lgcn_ctx_check(lgcn_ctx *x, void *stream) {
    if (!x) { lgcn_set_error("null context"); return 3; }
    int32_t flag = 0;
    HIP_OK(hipMemcpyAsync(&flag, x->c.err, sizeof flag, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    if (flag) {
        HIP_OK(hipMemsetAsync(x->c.err, 0, sizeof flag, (hipStream_t)stream));
        lgcn_set_error("device flagged an out-of-range user/item id in a batch");
    }
    return flag;
}

// lgcn_ctx.cpp -- the training context (lgcn_ctx.h) behind the C ABI of include/lgcn_hip.h: create and destroy, the setters and
// getters, and the refusals the entry points share.  No kernels, no launches and no step here: the driver is lgcn_train.cpp.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>

#include "lgcn_ctx.h"

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
int lgcn_refuse_dropout(const lgcn_ctx *x, const char *who) {
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
int lgcn_refuse_layer_weights(const lgcn_ctx *x, const char *who) {
    if (!x || !x->lw_n) return 0;
    char buf[192];
    snprintf(buf, sizeof buf, "%s: layer weights (lgcn_ctx_set_layer_weights) are implemented for the single-GPU step only", who);
    lgcn_set_error(buf);
    return 3;
}
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
extern "C" int lgcn_ctx_gate_total(const lgcn_ctx *x, void **buf, int32_t *count) {
    if (!x || !buf || !count) { lgcn_set_error("lgcn_ctx_gate_total: null argument"); return 3; }
    *buf = x->gate_total; *count = x->gate_total ? x->gate_P : 0;
    return 0;
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

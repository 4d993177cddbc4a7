// lgcn_train_dp.cpp -- the four data-parallel forms of the training step, behind the C ABI of include/lgcn_hip.h: the row
// exchange (part 1 / all-gather / part 2), the dense all-reduce, column shards and row-sharded propagation, and the C loop that
// runs a whole epoch of any of them with the collectives on the kernels' stream.  Every form is the driver of lgcn_train.cpp on
// a slice of the global batch (BatchView, lgcn_ctx.h) with another place for the loss launch's rows (LossPlace).  No kernels and
// no launches here.
#include <stdint.h>
#include <stdio.h>

#include "lgcn_ctx.h"

// What every data-parallel entry point checks first: the batch, then the features that have no form split over ranks
static int dp_guard(const lgcn_ctx *x, const char *who, const void *users, const void *pos, const void *neg, int32_t B) {
    int rc = train_check_batch(x, users, pos, neg, B);
    if (rc) return rc;
    if ((rc = lgcn_refuse_dropout(x, who))) return rc;
    if ((rc = lgcn_refuse_layer_weights(x, who))) return rc;
    return lgcn_refuse_loss(x, who);
}

extern "C" int64_t lgcn_dp_block_floats(const lgcn_ctx *x, int32_t B_global, int32_t world) {
    if (!x || B_global <= 0 || world < 1) return 0;
    return train_dp_block_floats(x, BatchView::of_rank(nullptr, nullptr, nullptr, B_global, world, 0).shard);
}
extern "C" int lgcn_train_step_dp_part1(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                        int32_t B_global, int32_t world, int32_t rank, void *stream) {
    int rc = dp_guard(x, "lgcn_train_step_dp_part1", users, pos, neg, B_global);
    if (rc) return rc;
    if (!x->c.contrib) { lgcn_set_error("dp step: cfg.contrib exchange buffer missing"); return 3; }
    if (world < 1 || rank < 0 || rank >= world) { lgcn_set_error("dp step: bad world/rank"); return 3; }
    const BatchView v = BatchView::of_rank(users, pos, neg, B_global, world, rank);
    hipStream_t st = (hipStream_t)stream;
    if ((rc = train_forward(x, st))) return rc;
    // with dp_local the rank's own rows go into G64 here (atomics) AND into the exchange block; part 2 scatters the others'
    const LossPlace at = x->dp_local ? PLACE_EXCHANGE_AND_G64 : PLACE_EXCHANGE;
    rc = x->variant ? train_variant_loss(x, v, at, st) : train_bpr(x, v, at, st);
    if (rc) return rc;
    x->dp_rank = rank;
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lgcn_train_step_dp_dense_part1(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                              int32_t B_global, int32_t world, int32_t rank, void *stream) {
    int rc = dp_guard(x, "lgcn_train_step_dp_dense_part1", users, pos, neg, B_global);
    if (rc) return rc;
    if (world < 1 || rank < 0 || rank >= world) { lgcn_set_error("dp step: bad world/rank"); return 3; }
    const BatchView v = BatchView::of_rank(users, pos, neg, B_global, world, rank);
    hipStream_t st = (hipStream_t)stream;
    const bool gate = x->variant && x->c.item_pop;
    // this rank owns positions [b_off, b_off+B_local) of the global loss-term arrays (loss | reg | with the gate: entropy);
    // the rest must be zero
    HIP_OK(hipMemsetAsync(x->c.terms, 0, sizeof(float) * (gate ? 3 : 2) * (size_t)B_global, st));
    if ((rc = train_forward(x, st))) return rc;
    if (x->variant) {
        // optional branches: the shard's rows go into this rank's G64 by atomics like the default model's; the MLP
        // parameter gradients of the shard are summed (fixed point: any order) into gate_total, one more all-reduce
        if ((rc = train_variant_loss(x, v, PLACE_DENSE, st))) return rc;
        if (gate) {
            if (v.B_local > 0)
                lgcn_gate_rank_total_launch((const long long *)x->gate_partials, (int32_t)((v.B_local + GATE_TPB - 1) / GATE_TPB), x->gate_P, x->gate_total, st);
            else HIP_OK(hipMemsetAsync(x->gate_total, 0, sizeof(long long) * (size_t)x->gate_P, st));
        }
    } else if ((rc = train_bpr(x, v, PLACE_DENSE, st))) return rc;
    SlotArgs s{};
    s.users = users; s.pos = pos; s.neg = neg; s.B = B_global; s.n_users = x->c.n_users; s.N = x->N;
    s.bitmap = x->c.bitmap + x->flip * x->bm_words; s.cnt = x->cnt;
    s.item_bitmap = (x->variant && x->c.i2i) ? x->item_bitmap : nullptr;      // the smoothing's backward reads the items of the GLOBAL batch
    lgcn_flag_rows_launch(s, st);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lgcn_train_step_dp_part2(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                        int32_t B_global, int32_t world, const float *gathered, float *loss_out,
                                        void *stream) {
    int rc = dp_guard(x, "lgcn_train_step_dp_part2", users, pos, neg, B_global);
    if (rc) return rc;
    if (!loss_out || world < 1) { lgcn_set_error("dp step part 2: invalid argument"); return 3; }
    // every rank runs the same backward over the global batch: the view's own slice (rank 0's here) is not read
    const BatchView v = BatchView::of_rank(users, pos, neg, B_global, world, 0);
    // gathered == NULL is the dense form: G64, the terms and (popularity gate) gate_total hold the reduced sums of the global batch
    if ((rc = train_backward(x, v, gathered, loss_out, (hipStream_t)stream, gathered == nullptr))) return rc;
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
    int rc = dp_guard(x, "lgcn_train_step_cols_part1", users, pos, neg, B);
    if (rc) return rc;
    if (x->variant) { lgcn_set_error("column-sharded step: the popularity gate / item-item smoothing mix columns (MLPs over the row): not supported"); return 3; }
    if (!x->c.contrib) { lgcn_set_error("column-sharded step: cfg.contrib (3*max_batch*d floats: the batch's slot rows) missing"); return 3; }
    hipStream_t st = (hipStream_t)stream;
    if ((rc = train_forward(x, st))) return rc;
    if ((rc = train_bpr(x, BatchView::whole(users, pos, neg, B), PLACE_COLS_SCORES, st))) return rc;
    if (partials) *partials = x->colsum;
    HIP_OK(hipGetLastError());
    return 0;
}
extern "C" int lgcn_train_step_cols_part2(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                                          int32_t B, float *loss_out, void *stream) {
    int rc = dp_guard(x, "lgcn_train_step_cols_part2", users, pos, neg, B);
    if (rc) return rc;
    if (!loss_out) { lgcn_set_error("column-sharded step part 2: loss_out is null"); return 3; }
    hipStream_t st = (hipStream_t)stream;
    const BatchView v = BatchView::whole(users, pos, neg, B);
    if ((rc = train_bpr(x, v, PLACE_COLS_ROWS, st))) return rc;
    if ((rc = train_backward(x, v, nullptr, loss_out, st, false))) return rc;
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
    int rc = dp_guard(x, "lgcn_rs_phase", users, pos, neg, B_global);
    if (rc) return rc;
    if (x->variant) { lgcn_set_error("lgcn_rs_phase: the popularity gate / item-item smoothing run on one GPU only"); return 3; }
    const lgcn_train_config &c = x->c;
    hipStream_t st = (hipStream_t)stream;
    if (world < 1 || rank < 0 || rank >= world) { lgcn_set_error("lgcn_rs_phase: bad world/rank"); return 3; }
    const BatchView v = BatchView::of_rank(users, pos, neg, B_global, world, rank);
    if ((rc = graph_acquire(c.graph, st))) return rc;
    switch (phase) {
    case LGCN_RS_FWD: {                               // X_k[owned] = (A X_{k-1})[owned], k = 1..K-1
        if (k < 1 || k > x->fwd_layers) { lgcn_set_error("lgcn_rs_phase: forward layer out of range"); return 3; }
        SpmmArgs a = train_base_spmm(x);
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
    case LGCN_RS_BPR:                                 // this rank's batch shard -> cfg.contrib
        if (!c.contrib) { lgcn_set_error("lgcn_rs_phase: cfg.contrib exchange buffer missing"); return 3; }
        rc = train_bpr(x, v, PLACE_EXCHANGE, st);
        break;
    case LGCN_RS_SCATTER: {                           // all ranks' gradient rows -> G64 + row flags
        if (!gathered) { lgcn_set_error("lgcn_rs_phase: gathered blocks missing"); return 3; }
        SlotArgs s = train_slot_args(x, v, gathered, loss_out);
        rc = lgcn_scatter_launch(s, c.d, st);
        break;
    }
    case LGCN_RS_BWD:                                 // h_{k-1}[owned] = Gs + (A h_k)[owned], k = K..1; k = 1: Adam on the owned rows
        if (k < 1 || k > c.K) { lgcn_set_error("lgcn_rs_phase: backward layer out of range"); return 3; }
        if (k == c.K) x->step += 1;
        rc = train_backward_layer(x, k, v, gathered, loss_out, false, st);
        break;
    case LGCN_RS_FINISH: {                            // zero the batch rows of G64 + their flags, reduce the loss
        if (!loss_out) { lgcn_set_error("lgcn_rs_phase: loss_out is null"); return 3; }
        SlotArgs s = train_slot_args(x, v, gathered, loss_out);
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
    if (phase == LGCN_RS_BWD && k > 1 && k <= c.K) { *buf = train_bwd_buffer(x, k); *dtype = c.act_dtype; return 0; }
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
        // floats of a rank's exchange block (the all-gathers of the rows and row-sharded forms)
        const size_t blk = (size_t)train_dp_block_floats(x, BatchView::of_rank(users + t, pos + t, neg + t, b, world, rank).shard);
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
            r = api->AllGather(x->c.contrib, gathered, blk, ncclFloat32, dp->comm, st);
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
            r = api->AllGather(x->c.contrib, gathered, blk, ncclFloat32, dp->comm, st);
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
    if (lgcn_refuse_dropout(x, "lgcn_train_epoch_dp") || lgcn_refuse_layer_weights(x, "lgcn_train_epoch_dp") || lgcn_refuse_loss(x, "lgcn_train_epoch_dp")) return 3;         // (every rank's context says the same: nobody waits in a collective)
    const int rc = train_epoch_dp_impl(x, dp, users, pos, neg, T, B_global, reduce, row_ranges, gathered, loss_out, stream);
    // a rank that leaves the loop early never reaches its next collective: release the loopback ranks waiting for it
    // (RCCL has its own abort / timeout machinery)
    if (rc && dp && dp->loopback) lgcn_dp_loopback_abort(dp);
    return rc;
}

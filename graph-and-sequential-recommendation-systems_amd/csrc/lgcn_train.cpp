// lgcn_train.cpp -- host side of training: the step driver (forward layers, the loss launch of the step's form, the backward
// chain with Adam) and the single-GPU step and epoch entry points of every step form, behind the C ABI of include/lgcn_hip.h.
// The context is lgcn_ctx.cpp's, the data-parallel forms are lgcn_train_dp.cpp's.  No kernels and no launches here: the driver
// fills in the args structs of lgcn_kernels.h and calls their launchers, which live beside the kernels in lgcn_device.hip.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "lgcn_ctx.h"

SpmmArgs train_base_spmm(const lgcn_ctx *x) {
    SpmmArgs a = graph_spmm(x->c.graph);
    a.G64 = (long long *)x->c.G64; a.G32 = x->g32; a.bitmap = x->c.bitmap + x->flip * x->bm_words;
    a.div = (float)(x->c.K + 1); a.remap = x->c.xcd_remap;
    return a;
}

// forward layers X_1..X_{K-1}
int train_forward(lgcn_ctx *x, hipStream_t st) {
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
        SpmmArgs a = train_base_spmm(x);
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

// The loss launch of the three-slot step on the slice `v` of a global batch; `at`: where its rows go (LossPlace)
int train_bpr(lgcn_ctx *x, const BatchView &v, LossPlace at, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    BprArgs a{};
    a.reg_ego = c.reg_ego; a.cnt = (at.atomics && at.count_slots) ? x->cnt : nullptr;
    a.dr = x->dr;
    const bool wts = x->lw_n != 0;
    for (int k = 0; k < x->lw_n; k++) a.w[k] = x->lw[k];
    a.cols_phase = at.cols_phase; a.erows = c.contrib; a.colsum = x->colsum;
    a.indptr = c.graph->indptr; a.indices = c.graph->indices; a.vals = c.graph->vals; a.X0 = c.E0; a.K = c.K;
    for (int k = 1; k <= x->fwd_layers; k++) a.Xl[k] = x->act[k];
    a.dense_last = c.dense_last;
    a.n_users = c.n_users; a.N = x->N;
    a.users = v.users + v.b_off; a.pos = v.pos + v.b_off; a.neg = v.neg + v.b_off;
    a.B_local = v.B_local; a.shard = v.shard;
    a.inv_B = 1.0f / (float)v.B_global; a.lam = c.decay / (float)v.B_global;
    a.G64 = at.atomics ? (long long *)c.G64 : nullptr; a.bitmap = c.bitmap + x->flip * x->bm_words;
    a.stale_bitmap = c.bitmap + (x->flip ^ 1) * x->bm_words; a.bitmap_words = x->bm_words;
    a.contrib = c.contrib; a.terms = c.terms; a.err = c.err; a.exchange = at.exchange ? 1 : 0;
    a.terms_off = at.exchange ? 0 : v.b_off; a.terms_stride = v.B_global;
    if (x->fold_mult && at.atomics && !at.exchange && at.cols_phase == 0 && v.b_off == 0 && v.B_local == v.B_global) {
        // a step of lgcn_train_epoch with the fold: the launch below also writes the fp32 copies of its gradient rows
        a.mult = x->fold_mult; a.G32 = x->g32; a.gdiv = x->lw_n ? 1.f : (float)(c.K + 1); a.arrive = x->arrive;
    }
    if (at.cols_phase == 2)     // column shard, after the all-reduce: loss terms + gradient scatter from the stored slot rows
        return v.B_local <= 0 ? 0 : lgcn_triplet_launch(a, c.d, c.act_dtype, wts, false, st);
    if (x->hub_graph && !c.dense_last && v.B_local > 0) {
        // last layer of the hub rows, X_K[hub] = (A_hat X_{K-1})[hub] in fp32, into the library's [N,d] table (free until k_g32)
        { int rc0 = graph_acquire(x->hub_graph, st); if (rc0) return rc0; }
        SpmmArgs h = graph_spmm(x->hub_graph);
        h.X = c.K == 1 ? (const void *)c.E0 : x->act[c.K - 1]; h.Y = x->g32; h.remap = c.xcd_remap; h.dr = x->dr;
        int rc = lgcn_spmm_launch(h, 0, c.d, c.K == 1 ? LGCN_F32 : c.act_dtype, LGCN_F32, st);
        if (rc) return rc;
        a.Xhub = x->g32; a.hub_nnz = x->hub_nnz;
    }
    if (v.B_local <= 0) {
        // a rank whose shard of a short last batch is empty launches nothing, but the row bitmap of
        // two steps ago still has to be cleared (k_triplet / k_triplet_dense does it on the other ranks)
        HIP_OK(hipMemsetAsync(a.stale_bitmap, 0, sizeof(uint32_t) * (size_t)x->bm_words, st));
        return 0;
    }
    return lgcn_triplet_launch(a, c.d, c.act_dtype, wts, big_table(x->N, c.d), st);
}

// floats per rank of the data-parallel exchange block for a shard of S triplets: [3*S*d gradient rows | S loss | S reg terms], with
// the popularity gate also [S entropy terms | pad to an even count | 2*P floats = P int64: the rank's fixed-point MLP gradient sums]
int64_t train_dp_block_floats(const lgcn_ctx *x, int64_t S) {
    int64_t n = 3 * S * x->c.d + 2 * S;
    if (x->variant && x->c.item_pop) { n += S; n += n & 1; n += 2 * (int64_t)x->gate_P; }
    return n;
}
int64_t train_dp_block_tail(const lgcn_ctx *x, int64_t S) {          // float offset of the int64 tail inside a block
    int64_t n = 3 * S * x->c.d + 3 * S;
    return n + (n & 1);
}

// The optional branches' forward tail and loss: T = mean of the K+1 dense layers, item-item smoothing, then the loss on the
// ONE final table (popularity gate inside k_triplet_gate).  The slice `v` of a global batch (single GPU: the whole batch); of
// `at` this launch reads atomics (into G64 / the row flags) and exchange (into the exchange block).
int train_variant_loss(lgcn_ctx *x, const BatchView &v, LossPlace at, hipStream_t st) {
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
    const int64_t tail = train_dp_block_tail(x, v.shard);
    if (v.B_local <= 0) {   // an empty shard: nothing to launch, but the stale bitmap must go and the block's MLP sums must read zero
        HIP_OK(hipMemsetAsync(stale, 0, sizeof(uint32_t) * (size_t)x->bm_words, st));
        if (at.exchange && c.item_pop) HIP_OK(hipMemsetAsync(c.contrib + tail, 0, sizeof(long long) * (size_t)x->gate_P, st));
        return 0;
    }
    if (c.item_pop) {
        GateArgs g{};
        g.E = x->tvar; g.item_pop = c.item_pop; g.params = c.gate_params; g.partials = x->gate_partials;
        g.Hp = c.pop_hidden; g.Hg = c.gate_hidden; g.P = x->gate_P;
        g.inv_temp = 1.0f / c.pop_gate_temp; g.ent_scale = c.gate_entropy_coeff / (float)(2 * v.B_global);
        g.n_users = c.n_users; g.N = x->N; g.users = v.users + v.b_off; g.pos = v.pos + v.b_off; g.neg = v.neg + v.b_off; g.B = v.B_local;
        g.inv_B = 1.0f / (float)v.B_global; g.lam = c.decay / (float)v.B_global;
        g.G64 = at.atomics ? (long long *)c.G64 : nullptr; g.bitmap = bm; g.item_bitmap = c.i2i ? x->item_bitmap : nullptr;
        g.stale_bitmap = stale; g.bitmap_words = x->bm_words; g.terms = c.terms + (at.exchange ? 0 : v.b_off); g.terms_stride = v.B_global; g.err = c.err;
        g.contrib = c.contrib; g.shard = v.shard; g.exchange = at.exchange ? 1 : 0;
        if (int rc = lgcn_gate_launch(g, c.d, st)) return rc;
        if (at.exchange)    // this rank's MLP gradient sums into the tail of its exchange block
            lgcn_gate_rank_total_launch((const long long *)x->gate_partials, (int32_t)((v.B_local + GATE_TPB - 1) / GATE_TPB), x->gate_P,
                                        (long long *)(c.contrib + tail), st);
    } else {
        BprArgs a{};
        a.X0 = x->tvar; a.K = 0; a.dense_last = 1;            // e = the row of the final table
        a.n_users = c.n_users; a.N = x->N; a.users = v.users + v.b_off; a.pos = v.pos + v.b_off; a.neg = v.neg + v.b_off; a.B_local = v.B_local; a.shard = v.shard;
        a.inv_B = 1.0f / (float)v.B_global; a.lam = c.decay / (float)v.B_global;
        a.G64 = at.atomics ? (long long *)c.G64 : nullptr; a.bitmap = bm; a.stale_bitmap = stale; a.bitmap_words = x->bm_words;
        a.item_bitmap = x->item_bitmap; a.terms = c.terms; a.err = c.err; a.terms_off = at.exchange ? 0 : v.b_off; a.terms_stride = v.B_global;
        a.contrib = c.contrib; a.exchange = at.exchange ? 1 : 0;
        return lgcn_triplet_launch(a, c.d, LGCN_F32, false, false, st);
    }
    return 0;
}

// what the slot kernels of the backward (k_g32, k_scatter, k_finish) take: the whole global batch of `v`
SlotArgs train_slot_args(const lgcn_ctx *x, const BatchView &v, const float *gathered, float *loss_out) {
    const lgcn_train_config &c = x->c;
    SlotArgs s{};
    s.users = v.users; s.pos = v.pos; s.neg = v.neg; s.B = v.B_global; s.n_users = c.n_users; s.N = x->N;
    s.G64 = (long long *)c.G64; s.G32 = x->g32; s.div = x->lw_n ? 1.f : (float)(c.K + 1);      // layer weights: G32 = G, the launches scale it
    s.bitmap = c.bitmap + x->flip * x->bm_words; s.gathered = gathered; s.shard = v.shard; s.world = v.world;
    s.terms = c.terms; s.loss_out = loss_out; s.decay = c.decay; s.skip_rank = -1;
    s.ent_coeff = c.item_pop ? c.gate_entropy_coeff : 0.f;
    s.blk = gathered ? train_dp_block_floats(x, v.shard) : 0;
    s.item_bitmap = (x->variant && c.i2i) ? x->item_bitmap : nullptr;
    s.cnt = x->cnt;
    return s;
}
static SlotArgsMulti slot_args_multi(const lgcn_ctx *x, const BatchView &v, float *loss_out) {
    SlotArgsMulti m{};
    m.s = train_slot_args(x, BatchView::whole(v.users, v.pos, nullptr, v.B_global), nullptr, loss_out);
    m.negs = x->mn.negs; m.neg_stride = x->mn.stride; m.R = x->mn.R;
    return m;
}
// buffer the backward layer k writes (k > 1): ping-pong inside the activation workspace (forward
// activations are dead by then)
void *train_bwd_buffer(const lgcn_ctx *x, int k) {
    return (x->c.K == 2) ? x->act[1] : x->act[1 + ((x->c.K - k) & 1)];
}

// Adam's scalars of step `step` (1-based), in double as torch.optim.Adam computes them; SpmmArgs (the +Adam launch of the tables)
// and GateAdamArgs (the gate's MLP parameters) name them alike
template <class Args> static void adam_scalars(Args &a, const lgcn_train_config &c, int64_t step) {
    const double bc1 = 1.0 - pow(c.beta1, (double)step);
    const double bc2 = 1.0 - pow(c.beta2, (double)step);
    a.step_size = (float)(c.lr / bc1); a.bc2_sqrt = (float)sqrt(bc2);
    a.w1 = (float)(1.0 - c.beta1); a.beta2 = (float)c.beta2; a.omb2 = (float)(1.0 - c.beta2); a.eps = (float)c.eps;
}

// One layer of the Horner chain h_{k-1} = Gs + A h_k (k = K: sparse input Gs; k = 1: feeds Adam).
// fused_finish: the Adam launch also zeroes the G64 rows it consumes and reduces the loss (single-GPU
// and batch-sharded steps, where every rank runs every row); the row-sharded step finishes separately.
int train_backward_layer(lgcn_ctx *x, int k, const BatchView &v, const float *gathered, float *loss_out, bool fused_finish, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    const int32_t B = v.B_global;
    const bool first = (k == c.K), last = (k == 1);
    if (first) {        // every contribution is in G64 by now: convert the batch rows once (the fold: k_triplet has done it)
        if (x->mn.on) {     // several negatives per positive, or the in-batch loss (R = 0): (2 + R) B slots, never folded
            SlotArgsMulti s = slot_args_multi(x, v, loss_out);
            if (int rc = lgcn_g32_multi_launch(s, c.d, st)) return rc;
        } else if (!x->fold_mult) {
            SlotArgs s = train_slot_args(x, v, gathered, loss_out);
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
    SpmmArgs a = train_base_spmm(x);
    a.dr = x->dr; a.dr.tr = 1;           // the chain multiplies by A_drop^T: the entry stored at (i, j) carries keep(j, i)
    a.X = first ? nullptr : train_bwd_buffer(x, k + 1);
    if (!last) a.Y = train_bwd_buffer(x, k);
    else {
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
        adam_scalars(a, c, x->step);
        if (!first && fused_finish) {       // K >= 2: this launch also cleans the workspace and reduces the loss
            a.clear = 1; a.terms = c.terms; a.gathered = gathered; a.loss_out = loss_out;
            a.B = B; a.shard = v.shard; a.decay = c.decay; a.ent_coeff = c.item_pop ? c.gate_entropy_coeff : 0.f;
            a.blk = gathered ? train_dp_block_floats(x, v.shard) : 0;
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
int train_backward(lgcn_ctx *x, const BatchView &v, const float *gathered, float *loss_out, hipStream_t st, bool gate_reduced) {
    const lgcn_train_config &c = x->c;
    { int rc0 = graph_acquire(c.graph, st); if (rc0) return rc0; }
    SlotArgs s = train_slot_args(x, v, gathered, loss_out);
    if (gathered) {
        s.skip_rank = x->dp_local ? x->dp_rank : -1;       // part 1 already added this rank's own rows
        if (int rc = lgcn_scatter_launch(s, c.d, st)) return rc;
    }
    x->step += 1;
    // Horner: h_{K-1} = Gs + A Gs (sparse input); h_{k-1} = Gs + A h_k; last one feeds Adam
    for (int k = c.K; k >= 1; k--) {
        int rc = train_backward_layer(x, k, v, gathered, loss_out, true, st);
        if (rc) return rc;
    }
    if (x->variant && c.item_pop) {          // torch.optim.Adam on the gate's MLP parameters, same step count as the tables
        GateAdamArgs ga{};
        if (gathered) {      // data parallel: the ranks' totals sit in the tails of their exchange blocks
            ga.src = (const long long *)(gathered + train_dp_block_tail(x, v.shard)); ga.n_src = v.world; ga.stride = train_dp_block_floats(x, v.shard) / 2;
        } else if (gate_reduced) {             // dense form: the all-reduced total
            ga.src = x->gate_total; ga.n_src = 1; ga.stride = x->gate_P;
        } else { ga.src = x->gate_partials; ga.n_src = (v.B_global + GATE_TPB - 1) / GATE_TPB; ga.stride = x->gate_P; }
        ga.P = x->gate_P;
        ga.params = c.gate_params; ga.m = c.gate_adam_m; ga.v = c.gate_adam_v; ga.grad_out = c.gate_grad;
        adam_scalars(ga, c, x->step);
        lgcn_gate_adam_launch(ga, st);
    }
    if (c.K >= 2) { x->flip ^= 1; return 0; }       // next step flags rows in the other bitmap
    if (x->mn.on) {
        SlotArgsMulti sm = slot_args_multi(x, v, loss_out);
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
static int run_step(lgcn_ctx *x, BatchView v, float *loss_out, hipStream_t st) {
    const lgcn_train_config &c = x->c;
    const int32_t *users = v.users, *pos = v.pos;
    const int32_t B = v.B_global;
    int rc;
    x->dr = make_drop(x->drop_keep, x->drop_seed, x->step, 0);        // ONE mask per step, from the counter before the step
    if ((rc = train_forward(x, st))) return rc;
    if (!x->mn.on) rc = x->variant ? train_variant_loss(x, v, PLACE_STEP, st) : train_bpr(x, v, PLACE_STEP, st);
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
        v.neg = x->hn_sel;
    }
    else rc = lgcn_multineg_launch(multineg_args(x, users, pos, B), c.d, c.act_dtype, x->lw_n != 0, st);
    if (rc) return rc;
    if ((rc = train_backward(x, v, nullptr, loss_out, st, false))) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

int train_check_batch(const lgcn_ctx *x, const void *u, const void *p, const void *n, int32_t B) {
    if (!x || !u || !p || !n) { lgcn_set_error("train step: null argument"); return 3; }
    if (B <= 0 || B > x->c.max_batch) { lgcn_set_error("train step: batch size out of range (0 < B <= max_batch)"); return 3; }
    return 0;
}

extern "C" int lgcn_train_step(lgcn_ctx *x, const int32_t *users, const int32_t *pos, const int32_t *neg,
                               int32_t B, float *loss_out, void *stream) {
    int rc = train_check_batch(x, users, pos, neg, B);
    if (rc) return rc;
    if ((rc = lgcn_refuse_loss(x, "lgcn_train_step"))) return rc;
    if (!loss_out) { lgcn_set_error("train step: loss_out is null"); return 3; }
    return run_step(x, BatchView::whole(users, pos, neg, B), loss_out, (hipStream_t)stream);
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
    return run_step(x, BatchView::whole(users, pos, negs, B), loss_out, (hipStream_t)stream);
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

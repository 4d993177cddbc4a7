// lgcn_graph.cpp -- host side of the graph object and of propagation: the plan builder of lgcn_graph_create, the SpMM,
// edge-dropout, conversion, propagation and permutation entry points of the C ABI (include/lgcn_hip.h).  No kernels and no
// launches here: every launch goes through a launcher of lgcn_kernels.h, defined beside its kernel in lgcn_device.hip.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <array>
#include <new>
#include <vector>

#include "lgcn_internal.h"

extern "C" int lgcn_device_available(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n > 0;
}

// ---------------------------------------------------------------------------------
// graph object: device CSR (borrowed) + the long-row plan and its scratch (owned)
// ---------------------------------------------------------------------------------
extern "C" int lgcn_graph_create(const int32_t *indptr, const int32_t *indices, const float *vals,
                                 int64_t n_rows, int64_t nnz, int32_t d_max, const int32_t *row_order,
                                 int64_t n_order, const int64_t *xcd_start, lgcn_graph **out) {
    return lgcn_graph_create_impl(indptr, indices, vals, n_rows, nnz, d_max, row_order, n_order, xcd_start, LONG_CH, out);
}
int lgcn_graph_create_impl(const int32_t *indptr, const int32_t *indices, const float *vals,
                           int64_t n_rows, int64_t nnz, int32_t d_max, const int32_t *row_order,
                           int64_t n_order, const int64_t *xcd_start, int32_t long_ch, lgcn_graph **out) {
    if (!indptr || !indices || !vals || !out || n_rows <= 0 || nnz < 0 || nnz > 0x7fffffffLL ||
        n_rows >= 0x7fffffffLL) { lgcn_set_error("lgcn_graph_create: invalid argument"); return 3; }
    if (d_max != 32 && d_max != 64 && d_max != 128 && d_max != 256) { lgcn_set_error("lgcn_graph_create: d_max must be 32, 64, 128 or 256"); return 3; }
    std::vector<int32_t> ip((size_t)n_rows + 1);
    HIP_OK(hipMemcpy(ip.data(), indptr, sizeof(int32_t) * ip.size(), hipMemcpyDeviceToHost));
    if (ip[0] != 0 || (int64_t)ip[(size_t)n_rows] != nnz) { lgcn_set_error("lgcn_graph_create: indptr does not match nnz"); return 3; }
    if (nnz > 0) {               // a bad column index would become an out-of-bounds row gather
        int32_t *bad = nullptr, hbad = 0;
        HIP_OK(hipMalloc((void **)&bad, sizeof(int32_t)));
        hipError_t e0 = hipMemset(bad, 0, sizeof(int32_t));
        if (e0 == hipSuccess) {
            lgcn_index_range_launch(indices, nnz, (int32_t)n_rows, bad);
            e0 = hipMemcpy(&hbad, bad, sizeof(int32_t), hipMemcpyDeviceToHost);
        }
        (void)hipFree(bad);
        if (e0 != hipSuccess) { lgcn_set_error("lgcn_graph_create: index check failed to run"); return 10; }
        if (hbad) { lgcn_set_error("lgcn_graph_create: column index out of range [0, n_rows)"); return 3; }
    }
    std::vector<int32_t> ord;
    if (!row_order) n_order = n_rows;
    if (n_order < 0 || n_order > n_rows) { lgcn_set_error("lgcn_graph_create: n_order out of range"); return 3; }
    if (row_order) {             // a permutation of 0..n_rows-1, or a subset of the rows without repetition
        ord.resize((size_t)n_order);
        if (n_order) HIP_OK(hipMemcpy(ord.data(), row_order, sizeof(int32_t) * ord.size(), hipMemcpyDeviceToHost));
        std::vector<char> seen((size_t)n_rows, 0);
        for (int64_t i = 0; i < n_order; i++) {
            const int32_t r = ord[(size_t)i];
            if (r < 0 || r >= n_rows || seen[(size_t)r]) { lgcn_set_error("lgcn_graph_create: row_order is not a permutation / repeats a row"); return 3; }
            seen[(size_t)r] = 1;
        }
    }
    for (int64_t r = 0; r < n_rows; r++)
        if (ip[(size_t)r + 1] < ip[(size_t)r]) { lgcn_set_error("lgcn_graph_create: indptr not monotone"); return 3; }
    // ---- slices of the processing order, one per XCD
    int64_t xs[XCDS + 1];
    if (xcd_start) {
        for (int x = 0; x <= XCDS; x++) xs[x] = xcd_start[x];
        bool ok = xs[0] == 0 && xs[XCDS] == n_order;
        for (int x = 0; x < XCDS; x++) ok = ok && xs[x] <= xs[x + 1];
        if (!ok) { lgcn_set_error("lgcn_graph_create: xcd_start must be 9 non-decreasing positions from 0 to n_order"); return 3; }
    } else {                     // balance the work: non-zeros plus a per-row constant (see reorder.py _row_cost)
        const double ROW_COST = 4.0;           // small per-row term (measured: 0..16 equal on Gowalla, larger is slower)
        double total = ROW_COST * (double)n_order;
        for (int64_t p = 0; p < n_order; p++) {
            const int32_t r = row_order ? ord[(size_t)p] : (int32_t)p;
            total += (double)(ip[(size_t)r + 1] - ip[(size_t)r]);
        }
        double acc = 0.0; int x = 1;
        xs[0] = 0;
        for (int64_t p = 0; p < n_order && x < XCDS; p++) {
            const int32_t r = row_order ? ord[(size_t)p] : (int32_t)p;
            acc += (double)(ip[(size_t)r + 1] - ip[(size_t)r]) + ROW_COST;
            while (x < XCDS && acc >= total * x / XCDS) xs[x++] = p + 1;
        }
        while (x <= XCDS) xs[x++] = n_order;
        xs[XCDS] = n_order;
    }
    // ---- per slice: chunks of its long rows (padded to whole workgroups), then its short rows; the
    //      planned rows' entries go into the packed stream in exactly that order
    std::vector<int32_t> long_row, long_nch, chunks, rowinfo, copyplan;
    SlicePlan sp{};
    rowinfo.reserve((size_t)n_order * 4 + 4 * SLICE_PAD * XCDS);
    copyplan.reserve((size_t)n_order * 4);
    int64_t n_pk = 0;
    for (int x = 0; x < XCDS; x++) {
        sp.cblk[x] = (int32_t)(chunks.size() / 16); sp.rows[x] = (int32_t)(rowinfo.size() / 4);
        const size_t slice_begin = rowinfo.size();
        for (int64_t p = xs[x]; p < xs[x + 1]; p++) {
            const int32_t r = row_order ? ord[(size_t)p] : (int32_t)p;
            const int32_t s0 = ip[(size_t)r], deg = ip[(size_t)r + 1] - s0;
            if (deg > LONG_T) {
                const int nch = (deg + long_ch - 1) / long_ch;
                const int32_t lb = (int32_t)n_pk;
                for (int k = 0; k < nch; k++) {
                    const int32_t c0 = k * long_ch, c1 = c0 + long_ch < deg ? c0 + long_ch : deg;
                    const int32_t e[4] = {(int32_t)long_row.size(), lb + c0, lb + c1, k};
                    chunks.insert(chunks.end(), e, e + 4);
                }
                const int32_t cp[4] = {s0, lb, deg, 0};
                copyplan.insert(copyplan.end(), cp, cp + 4);
                n_pk += deg;
                long_row.push_back(r); long_nch.push_back(nch);
            } else {
                const int32_t e[4] = {r, s0, deg, 0};
                rowinfo.insert(rowinfo.end(), e, e + 4);
            }
        }
        // rows of a pack run in lock step: sort every window of SHORT_WIN short rows by length (stable)
        for (size_t w0 = slice_begin; w0 < rowinfo.size(); w0 += 4 * SHORT_WIN) {
            const size_t w1 = std::min(rowinfo.size(), w0 + 4 * (size_t)SHORT_WIN), n = (w1 - w0) / 4;
            std::vector<std::array<int32_t, 4>> tmp(n);
            for (size_t i = 0; i < n; i++) for (int k = 0; k < 4; k++) tmp[i][k] = rowinfo[w0 + 4 * i + k];
            std::stable_sort(tmp.begin(), tmp.end(), [](const std::array<int32_t, 4> &p, const std::array<int32_t, 4> &q) { return p[2] > q[2]; });
            for (size_t i = 0; i < n; i++) for (int k = 0; k < 4; k++) rowinfo[w0 + 4 * i + k] = tmp[i][k];
        }
        // stream positions of the short rows, in their final order
        for (size_t i = slice_begin; i < rowinfo.size(); i += 4) {
            const int32_t cp[4] = {rowinfo[i + 1], (int32_t)n_pk, rowinfo[i + 2], 0};
            if (cp[2] > 0) copyplan.insert(copyplan.end(), cp, cp + 4);
            rowinfo[i + 1] = (int32_t)n_pk;
            n_pk += rowinfo[i + 2];
        }
        const int32_t pad[4] = {-1, 0, 0, 0};
        while ((chunks.size() / 4) % 4) chunks.insert(chunks.end(), pad, pad + 4);
        while ((rowinfo.size() / 4) % SLICE_PAD) rowinfo.insert(rowinfo.end(), pad, pad + 4);
    }
    sp.cblk[XCDS] = (int32_t)(chunks.size() / 16); sp.rows[XCDS] = (int32_t)(rowinfo.size() / 4);
    lgcn_graph *g = new (std::nothrow) lgcn_graph;
    if (!g) { lgcn_set_error("out of memory"); return 4; }
    g->indptr = indptr; g->indices = indices; g->vals = vals; g->rowinfo = nullptr; g->pk = nullptr;
    g->n_rows = n_rows; g->nnz = nnz; g->d_max = d_max;
    g->owned = nullptr; g->lp = LongPlan{}; g->sp = sp;
    g->used = false; g->last_stream = nullptr; g->order_ev = nullptr;
    if (hipEventCreateWithFlags(&g->order_ev, hipEventDisableTiming) != hipSuccess) { delete g; lgcn_set_error("lgcn_graph_create: hipEventCreate failed"); return 10; }
    const size_t n_long = long_row.size(), n_slots = chunks.size() / 4, n_info = rowinfo.size() / 4;
    {
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_info = 0, o_chk = up(o_info + 16 * n_info), o_row = up(o_chk + 16 * n_slots),
                     o_nch = up(o_row + 4 * n_long), o_cnt = up(o_nch + 4 * n_long),
                     o_par = up(o_cnt + 4 * n_long), o_pk = up(o_par + n_slots * (size_t)d_max * 4),
                     total = o_pk + 8 * (size_t)n_pk + 256;
        char *base = nullptr;
        if (hipMalloc((void **)&base, total) != hipSuccess) { (void)hipEventDestroy(g->order_ev); delete g; lgcn_set_error("lgcn_graph_create: hipMalloc failed"); return 4; }
        g->owned = base;
        hipError_t e1 = hipMemset(base, 0, total);
        if (e1 == hipSuccess && n_info) e1 = hipMemcpy(base + o_info, rowinfo.data(), 16 * n_info, hipMemcpyHostToDevice);
        if (e1 == hipSuccess && n_long) {
            e1 = hipMemcpy(base + o_chk, chunks.data(), 16 * n_slots, hipMemcpyHostToDevice);
            if (e1 == hipSuccess) e1 = hipMemcpy(base + o_row, long_row.data(), 4 * n_long, hipMemcpyHostToDevice);
            if (e1 == hipSuccess) e1 = hipMemcpy(base + o_nch, long_nch.data(), 4 * n_long, hipMemcpyHostToDevice);
        }
        if (e1 == hipSuccess && !copyplan.empty()) {        // fill the packed stream on the device
            int4 *items = nullptr;
            e1 = hipMalloc((void **)&items, copyplan.size() * 4);
            if (e1 == hipSuccess) e1 = hipMemcpy(items, copyplan.data(), copyplan.size() * 4, hipMemcpyHostToDevice);
            if (e1 == hipSuccess) {
                lgcn_pack_stream_launch(items, (int64_t)(copyplan.size() / 4), indices, vals, (int2 *)(base + o_pk));
                e1 = hipDeviceSynchronize();
            }
            if (items) (void)hipFree(items);
        }
        if (e1 != hipSuccess) { (void)hipFree(base); (void)hipEventDestroy(g->order_ev); delete g; lgcn_set_error("lgcn_graph_create: plan upload failed"); return 10; }
        g->rowinfo = (const int4 *)(base + o_info);
        g->pk = (const int2 *)(base + o_pk);
        if (n_long) {
            g->lp.chunks = (const int4 *)(base + o_chk);
            g->lp.long_row = (const int32_t *)(base + o_row); g->lp.long_nch = (const int32_t *)(base + o_nch);
            g->lp.counters = (int32_t *)(base + o_cnt);
            g->lp.partials = (float *)(base + o_par);
            g->lp.n_long = (int32_t)n_long; g->lp.n_chunk_slots = (int32_t)n_slots;
        }
    }
    *out = g;
    return 0;
}

extern "C" void lgcn_graph_destroy(lgcn_graph *g) {
    if (!g) return;
    if (g->owned) (void)hipFree(g->owned);
    if (g->order_ev) (void)hipEventDestroy(g->order_ev);
    delete g;
}

extern "C" int lgcn_spmm_csr(const lgcn_graph *g, const void *X, int x_dtype, void *Y, int y_dtype, int d, void *stream) {
    if (!g || !X || !Y) { lgcn_set_error("lgcn_spmm_csr: null/invalid argument"); return 3; }
    if (check_dtype(x_dtype) || check_dtype(y_dtype)) return 3;
    if (d > g->d_max) { lgcn_set_error("lgcn_spmm_csr: d exceeds the graph's d_max"); return 3; }
    SpmmArgs a = graph_spmm(g);
    a.X = X; a.Y = Y; a.remap = 1;
    int rc = graph_acquire(g, (hipStream_t)stream);
    if (rc) return rc;
    rc = lgcn_spmm_launch(a, 0, d, x_dtype, y_dtype, (hipStream_t)stream);
    if (rc) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------
// edge dropout: the step's keys, the exported mask, the masked SpMM
// ---------------------------------------------------------------------------------

extern "C" int lgcn_dropout_mask(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t nnz,
                                 float keep_prob, uint64_t seed, int64_t step, uint8_t *keep_out, void *stream) {
    if (!indptr || n_rows <= 0 || nnz < 0 || (nnz > 0 && (!indices || !keep_out))) { lgcn_set_error("lgcn_dropout_mask: invalid argument"); return 3; }
    if (!drop_prob_ok(keep_prob)) { lgcn_set_error("lgcn_dropout_mask: dropout keep_prob must be in (0, 1]"); return 3; }
    if (nnz == 0) return 0;
    const uint64_t k = splitmix64(splitmix64(seed) + (uint64_t)step);
    lgcn_dropout_mask_launch(indptr, indices, n_rows, nnz, (uint32_t)k, (uint32_t)(k >> 32), drop_threshold(keep_prob), keep_out, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lgcn_spmm_csr_drop(const lgcn_graph *g, const void *X, int x_dtype, void *Y, int y_dtype, int d,
                                  float keep_prob, uint64_t seed, int64_t step, int transposed, void *stream) {
    if (!g || !X || !Y) { lgcn_set_error("lgcn_spmm_csr_drop: null/invalid argument"); return 3; }
    if (check_dtype(x_dtype) || check_dtype(y_dtype)) return 3;
    if (x_dtype == LGCN_FP8 || y_dtype == LGCN_FP8) { lgcn_set_error("lgcn_spmm_csr_drop: edge dropout is not implemented for fp8 tables"); return 3; }
    if (!drop_prob_ok(keep_prob)) { lgcn_set_error("lgcn_spmm_csr_drop: dropout keep_prob must be in (0, 1]"); return 3; }
    if (d > g->d_max) { lgcn_set_error("lgcn_spmm_csr_drop: d exceeds the graph's d_max"); return 3; }
    SpmmArgs a = graph_spmm(g);
    a.X = X; a.Y = Y; a.remap = 1; a.dr = make_drop(keep_prob, seed, step, transposed);
    int rc = graph_acquire(g, (hipStream_t)stream);
    if (rc) return rc;
    rc = lgcn_spmm_launch(a, 0, d, x_dtype, y_dtype, (hipStream_t)stream);
    if (rc) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int64_t lgcn_table_bytes(int64_t n_rows, int32_t d, int32_t dtype) { return n_rows > 0 && d > 0 ? (int64_t)table_bytes(n_rows, d, dtype) : 0; }
extern "C" int lgcn_to_fp8(const float *src, void *dst, int64_t n_rows, int32_t d, void *stream) {
    if (!src || !dst || n_rows <= 0) { lgcn_set_error("lgcn_to_fp8: invalid argument"); return 3; }
    int rc = lgcn_to_fp8_launch(src, dst, n_rows, d, (hipStream_t)stream);
    if (rc) return rc;
    HIP_OK(hipGetLastError());
    return 0;
}

// Layer weights w_0..w_K: fp32 values taken as they are.  n values for a model of K layers; finite, not all zero.
int lgcn_check_layer_weights(const char *who, const float *w, int n, int K) {
    char buf[192];
    bool ok = w && n == K + 1, any = false;
    for (int k = 0; ok && k < n; k++) { ok = isfinite(w[k]); any = any || w[k] != 0.f; }
    if (ok && any) return 0;
    snprintf(buf, sizeof buf, "%s: layer weights must be K + 1 = %d finite fp32 values that are not all zero (got %d)", who, K + 1, n);
    lgcn_set_error(buf);
    return 3;
}

// w: NULL = the mean (lgcn_propagate_mean), else K + 1 layer weights (lgcn_propagate_weighted)
static int propagate_impl(const char *who, const lgcn_graph *g, const float *E0, int K, int d, int act_dtype, void *work,
                          const float *w, float *out, void *stream) {
    char buf[160];
    if (!g || !E0 || !out || K < 1 || K > LGCN_MAX_LAYERS) { snprintf(buf, sizeof buf, "%s: invalid argument", who); lgcn_set_error(buf); return 3; }
    if (K > 1 && !work) { snprintf(buf, sizeof buf, "%s: workspace required for K > 1", who); lgcn_set_error(buf); return 3; }
    if (check_dtype(act_dtype)) return 3;
    if (d > g->d_max) { snprintf(buf, sizeof buf, "%s: d exceeds the graph's d_max", who); lgcn_set_error(buf); return 3; }
    hipStream_t st = (hipStream_t)stream;
    { int rc0 = graph_acquire(g, st); if (rc0) return rc0; }
    const int64_t N = g->n_rows;
    MeanArgs m{};
    m.X0 = E0; m.K = K; m.out = out; m.n4 = N * d / 4; m.d = d; m.N = N;
    const size_t stride = table_bytes(N, d, act_dtype);
    const void *prev = E0; int prev_dtype = LGCN_F32;
    if (act_dtype == LGCN_BF16 && K >= 2) {
        // the same rule as the training step: with bf16 activation storage layer 1 reads bf16(E0).  `out` is free until
        // the last layer writes it (K >= 2): its memory holds the 2-byte copy meanwhile
        lgcn_to_bf16_launch(E0, (bf16_t *)out, N * d, st);
        prev = out; prev_dtype = LGCN_BF16;
    }
    if (act_dtype == LGCN_FP8 && K >= 2) {                 // the same with fp8 storage: rows + scales fit the fp32 `out`
        int rc = lgcn_to_fp8_launch(E0, out, N, d, st);
        if (rc) return rc;
        prev = out; prev_dtype = LGCN_FP8;
    }
    for (int k = 1; k <= K; k++) {
        const bool last = (k == K);
        void *y = last ? (void *)out : (void *)((char *)work + (size_t)(k - 1) * stride);
        SpmmArgs a = graph_spmm(g);
        a.X = prev; a.Y = y; a.remap = 1;
        int rc = lgcn_spmm_launch(a, 0, d, prev_dtype, last ? LGCN_F32 : act_dtype, st);
        if (rc) return rc;
        if (!last) { m.Xl[k] = y; prev = y; prev_dtype = act_dtype; }
    }
    if (w) for (int k = 0; k <= K; k++) m.w[k] = w[k];
    lgcn_layer_mean_launch(m, act_dtype, w != nullptr, st);
    HIP_OK(hipGetLastError());
    return 0;
}
extern "C" int lgcn_propagate_mean(const lgcn_graph *g, const float *E0, int K, int d, int act_dtype, void *work,
                                   float *out, void *stream) {
    return propagate_impl("lgcn_propagate_mean", g, E0, K, d, act_dtype, work, nullptr, out, stream);
}
extern "C" int lgcn_propagate_weighted(const lgcn_graph *g, const float *E0, int K, int d, int act_dtype, void *work,
                                       const float *w_host, float *out, void *stream) {
    if (K < 1 || K > LGCN_MAX_LAYERS) { lgcn_set_error("lgcn_propagate_weighted: invalid argument"); return 3; }
    if (act_dtype == LGCN_FP8) { lgcn_set_error("lgcn_propagate_weighted: layer weights are not implemented for LGCN_FP8 activation storage"); return 3; }
    if (int rc = lgcn_check_layer_weights("lgcn_propagate_weighted", w_host, K + 1, K)) return rc;
    return propagate_impl("lgcn_propagate_weighted", g, E0, K, d, act_dtype, work, w_host, out, stream);
}

extern "C" int lgcn_apply_perm(const int32_t *S, int s_cols, const int64_t *perm, int64_t T,
                               int32_t *users, int32_t *pos, int32_t *neg, void *stream) {
    if (!S || !users || !pos || !neg || s_cols < 3 || T < 0) { lgcn_set_error("lgcn_apply_perm: invalid argument"); return 3; }
    if (T == 0) return 0;
    lgcn_apply_perm_launch(S, s_cols, perm, T, users, pos, neg, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lgcn_apply_perm_multi(const int32_t *S, int s_cols, const int64_t *perm, int64_t T,
                                     int32_t *users, int32_t *pos, int32_t *negs, int32_t R, void *stream) {
    if (R < 1 || R > LGCN_MAX_NEG_RATIO) { lgcn_set_error("lgcn_apply_perm_multi: the negative ratio R must be in 1..16"); return 3; }
    if (!S || !users || !pos || !negs || s_cols < 2 + R || T < 0) { lgcn_set_error("lgcn_apply_perm_multi: invalid argument (s_cols >= 2 + R)"); return 3; }
    if (T == 0) return 0;
    lgcn_apply_perm_multi_launch(S, s_cols, perm, T, users, pos, negs, R, (hipStream_t)stream);
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lgcn_slot_multiplicity(const int32_t *users, const int32_t *pos, const int32_t *neg, int64_t T, int32_t B,
                                      int32_t n_users, int64_t N, uint16_t *mult_out, void *stream) {
    if (T <= 0) return 0;
    if (!users || !pos || !neg || !mult_out) { lgcn_set_error("lgcn_slot_multiplicity: null argument"); return 3; }
    if (B <= 0 || n_users <= 0 || N <= n_users || N > 0x7fffffffLL) { lgcn_set_error("lgcn_slot_multiplicity: bad sizes (0 < B, 0 < n_users < N < 2^31)"); return 3; }
    if (!slot_mult_hash(B)) { lgcn_set_error("lgcn_slot_multiplicity: the row ids of a batch of B triplets do not fit the LDS hash (B <= 4096)"); return 3; }
    const int64_t seg = lgcn_fold_segment_steps() * B;          // triplets per launch
    for (int64_t t = 0; t < T; t += seg) {
        int rc = lgcn_slot_mult_launch(users + t, pos + t, neg + t, (T - t) < seg ? (T - t) : seg, B, n_users, N, mult_out + 3 * t, (hipStream_t)stream);
        if (rc) return rc;
    }
    HIP_OK(hipGetLastError());
    return 0;
}

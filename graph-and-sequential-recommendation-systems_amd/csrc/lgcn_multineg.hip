// lgcn_multineg.hip -- the batch-row launch of the fused LightGCN step for samples with SEVERAL negatives per positive
// (--neg_ratio R, --loss; lgcn_train_step_multi / lgcn_train_epoch_multi), gfx950 (wave64).
//
// A sample is (u, p, n_1..n_R).  With e the rows of the model's output table (layer mean, or the weighted sum):
//   x_r  = e_u.e_p - e_u.e_{n_r}
//   reg  = 0.5/B sum_b ( |e_u|^2 + |e_p|^2 + 1/R sum_r |e_{n_r}|^2 )      (reg_ego: on the tables' own rows E0[.])
//   lam  = decay / B
//   g_u = sum_r gb_r (e_p - e_{n_r}) + lam e_u ;  g_p = (sum_r gb_r) e_u + lam e_p ;  g_{n_r} = -gb_r e_u + lam/R e_{n_r}
// and the loss (lgcn_ctx_set_loss) decides the term of the sample and the coefficient gb_r of a negative:
//   LGCN_LOSS_BPR      bpr = -1/(B R) sum_b sum_r logsigmoid(x_{b,r}),   gb_r = -sigmoid(-x_r) / (B R)
//                      term for term the loss of the three-slot step on the flattened batch of B R triplets (u, p, n_r)
//   LGCN_LOSS_SOFTMAX  z_r = -x_r / tau (tau > 0),  l = log(1 + sum_r exp(z_r)),  sm = 1/B sum_b l_b,
//                      q_r = exp(z_r) / (1 + sum_j exp(z_j)),  gb_r = -q_r / (tau B);  terms[b] = -l, so the single-wave
//                      reduction with 1/B yields sm
// Either way the user row and the positive row are read once and added to G64 once: 2 + R slot rows and 2 + R fixed-point
// row adds per sample instead of 3 R.
//
// k_multineg<D, TI, WTS, LOSS> (the dense-last form: every layer X_1..X_K exists as a table): one lane group of min(D, 64)
// lanes per sample, lane = column (mod 64), 256 / min(D, 64) samples per workgroup -- the geometry of k_triplet_dense, so
// every load and every 64-bit atomic wave-instruction covers min(D, 64) contiguous elements.  The negatives are STREAMED:
// the row of negative r + 1 is in flight while negative r is worked on, and only sum_r gb_r and sum_r gb_r e_{n_r} stay in
// registers, so neither the register count nor anything else grows with R (#pragma unroll 1 over r; no LDS).
// Lanes 0..R-1 of the group hold the negatives' ids (R <= 16 <= the smallest group), lanes R and R + 1 the user's and the
// positive's row: one ballot voids a sample, the row flags and the reg_ego slot counts of all 2 + R rows are ONE atomic
// instruction each.  That prologue -- geometry, stale-bitmap loop, id check and ballot, user / positive pair, flag and count -- is
// lgcn_batch_rows.h's, shared with k_hardneg, k_inbatch_rows and k_directau_rows.  LOSS is a compile-time axis, so an instantiation holds the code of its own loss only:
//   BPR      one pass over the negatives: a negative's gradient row goes out as soon as its score is known.
//   softmax  q_r needs ALL R scores of the sample before any gradient row can leave, so two passes with a step between:
//     score      z_r stays in lane r of the group, the reg squares are summed.  No gradient leaves.
//     normalise  m = max(0, max_r z_r) and the sum over lanes < R with shuffles;  with the one term that equals exp(0)
//                taken out of the sum (the positive's when m = 0, the first maximal negative's otherwise)
//                    l = m + log1p(Zm1),  q_r = exp(z_r - m) / (1 + Zm1)
//                so no exp of a positive argument occurs and l keeps its relative accuracy where it is tiny.
//     emit       the negatives' rows are streamed a SECOND time (they were read by this workgroup a moment ago): g_{n_r}
//                and sum_r gb_r e_{n_r} need the row and gb_r together.
// The two softmax passes are one function (softmax_pass); the BPR pass stays written out in the kernel, so a fix to the
// streaming loop or to the emit of a gradient row is made in BOTH places.  Reason: the library is built with floating-point
// contraction on, and which multiply-add pairs hipcc fuses follows the shape of the code -- a BPR pass shared with softmax
// moved low bits of the gradient rows (profiles/batch_row_merge/README.md).  Keep the declaration order of sgb / sl / srn and
// the row buffers for the same reason, and compare the compiler's resource report with the previous one after an edit.
// Everything downstream consumes what the three-slot kernels write: G64 (2^50 fixed point), the row bitmap, cnt, terms, err.
#include "lgcn_batch_rows.h"      // RowsGeo and the sample prologue (bitmap loop, id check, user / positive pair, flag and count), DISPATCH_ROWS

// (slot_row, the output-table row of a slot, lives in lgcn_device_common.h: the in-batch launch gathers its rows through it too)

// One of the two passes of the softmax loss over the R negatives of a sample (their ids are in lanes 0..R-1 of the group), the
// rows of negative r + 1 in flight while negative r is worked on.  Score pass (!EMIT): z_r into lane r of zq, the squares into
// srn; no gradient leaves.  Emit pass: zq holds q_r in lane r, the coefficient of negative r is gb_r = -inv_tauB q_r.
// The score pass reads ps / ego and writes srn / zq only; the emit pass reads lam_n / zq and writes acc / sgb only (one
// signature so that the loop exists once: the arguments a pass does not use cost nothing after inlining).
// n, n0, nn, nn0: the kernel's row buffers (this and the next negative's slot_row).
template <int D, typename TI, bool WTS, bool EMIT>
__device__ __forceinline__ void softmax_pass(const MultiNegArgs &a, int32_t id, int l, const float *u, float ps, bool ego, float lam_n,
                                             float *acc, float &sgb, float &srn, float &zq, float *n, float *n0, float *nn, float *nn0) {
    constexpr int LPT = RowsGeo<D>::LPT, CPT = RowsGeo<D>::CPT;
    const int R = a.R;
    int64_t rn = (int64_t)__shfl(id, 0, LPT) + a.n_users;
    slot_row<D, TI, WTS>(a, rn, l, n, n0);
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const int64_t rnext = (int64_t)__shfl(id, r + 1 < R ? r + 1 : r, LPT) + a.n_users;
        if (r + 1 < R) slot_row<D, TI, WTS>(a, rnext, l, nn, nn0);
        if constexpr (!EMIT) {
            float ns = 0.f;
#pragma unroll
            for (int j = 0; j < CPT; j++) { const float v = ego ? n0[j] : n[j]; ns += u[j] * n[j]; srn += v * v; }
            ns = group_sum<LPT>(ns);
            const float zr = -(ps - ns) / a.tau;
            if (l == r) zq = zr;
        } else {
            const float gb = -a.inv_tauB * __shfl(zq, r, LPT);
            sgb += gb;
#pragma unroll
            for (int j = 0; j < CPT; j++) {
                acc[j] += gb * n[j];
                const float g = (-gb) * u[j] + lam_n * n[j];
                fixed_add(a.G64 + rn * D + j * LPT + l, g);
            }
        }
        if (r + 1 < R) {
#pragma unroll
            for (int j = 0; j < CPT; j++) { n[j] = nn[j]; n0[j] = nn0[j]; }
            rn = rnext;
        }
    }
}

template <int D, typename TI, bool WTS, int LOSS>
__global__ void __launch_bounds__(256) k_multineg(MultiNegArgs a) {
    ROWS_ZERO_STALE_BITMAP(a);
    ROWS_GEOMETRY(D);
    if (b >= a.B) return;                       // whole lane groups leave together
    const int R = a.R;
    ROWS_LOAD_IDS(a, ROWS_NEGS_FIRST, true, true);      // lane r < R holds negative r, lanes R / R + 1 the user / positive
    const int64_t myrow = l == R ? (int64_t)id : (int64_t)id + a.n_users;      // (meaningful on lanes 0 .. R + 1)
    if (bad) {                                  // an out-of-range id voids the whole sample: err flag, zero terms, no gradient
        if (l == 0) { atomicExch(a.err, 1); a.terms[b] = 0.f; a.terms[a.terms_stride + b] = 0.f; }
        return;
    }
    const int64_t ru = (int64_t)__shfl(id, R, LPT), rp = (int64_t)__shfl(id, R + 1, LPT) + a.n_users;
    const bool ego = a.reg_ego != 0;
    const float lam = ego ? 0.f : a.lam, lam_n = ego ? 0.f : a.lam_n;
    float u[CPT], p[CPT], acc[CPT];             // acc = sum_r gb_r e_{n_r}
    float ps = 0.f, ru2 = 0.f, rp2 = 0.f;
    ROWS_PAIR(ps += u[j] * p[j]; acc[j] = 0.f)
    ps = group_sum<LPT>(ps);
    float sgb = 0.f, sl = 0.f, srn = 0.f;       // sum_r gb_r, the loss term (BPR: sum_r logsigmoid(x_r)), sum_r |n_r|^2 (this lane's columns)
    float n[CPT], n0[CPT], nn[CPT], nn0[CPT];
    if constexpr (LOSS == LGCN_LOSS_BPR) {
        int64_t rn = (int64_t)__shfl(id, 0, LPT) + a.n_users;
        slot_row<D, TI, WTS>(a, rn, l, n, n0);
#pragma unroll 1
        for (int r = 0; r < R; r++) {
            const int64_t rnext = (int64_t)__shfl(id, r + 1 < R ? r + 1 : r, LPT) + a.n_users;
            if (r + 1 < R) slot_row<D, TI, WTS>(a, rnext, l, nn, nn0);      // the next negative's rows fly while this one is scored
            float ns = 0.f;
#pragma unroll
            for (int j = 0; j < CPT; j++) { const float v = ego ? n0[j] : n[j]; ns += u[j] * n[j]; srn += v * v; }
            ns = group_sum<LPT>(ns);
            const float x = ps - ns;
            const float gb = -a.inv_BR * sigmoid_neg_f(x);
            sl += logsigmoid_f(x);
            sgb += gb;
#pragma unroll
            for (int j = 0; j < CPT; j++) {
                acc[j] += gb * n[j];
                const float g = (-gb) * u[j] + lam_n * n[j];
                fixed_add(a.G64 + rn * D + j * LPT + l, g);
            }
            if (r + 1 < R) {
#pragma unroll
                for (int j = 0; j < CPT; j++) { n[j] = nn[j]; n0[j] = nn0[j]; }
                rn = rnext;
            }
        }
    } else {
        // ---- score.  z_r into lane r; lanes >= R keep 0, the positive's own exponent (LPT >= 32 > R: there is one)
        float z = 0.f;
        softmax_pass<D, TI, WTS, false>(a, id, l, u, ps, ego, lam_n, acc, sgb, srn, z, n, n0, nn, nn0);
        // ---- normalise.  m = max(0, max_r z_r); every exponent below is <= 0
        const float m = group_max<LPT>(z);
        const bool mine = l < R;
        // the term that is exp(0) = 1 exactly is left out of the sum: the positive's where m = 0, else the first maximal negative's
        const unsigned long long atmax = ROWS_VOTES(mine && z == m);
        const int first = m > 0.f ? __ffsll(atmax) - 1 : -1;
        const float ev = mine ? expf(z - m) : 0.f;
        const float zm1 = group_sum<LPT>(l == first ? 0.f : ev) + (m > 0.f ? expf(-m) : 0.f);      // Z - 1
        float q = ev / (1.f + zm1);             // q_r in lane r (0 on lanes >= R)
        sl = -(m + log1pf(zm1));
        // ---- emit.  the negatives' rows a second time, now with their coefficients
        softmax_pass<D, TI, WTS, true>(a, id, l, u, ps, ego, lam_n, acc, sgb, srn, q, n, n0, nn, nn0);
    }
    const float rr = group_sum<LPT>(ru2 + rp2 + srn * a.inv_R);
    if (l == 0) { a.terms[b] = LOSS == LGCN_LOSS_SOFTMAX ? sl : sl * a.inv_R; a.terms[a.terms_stride + b] = rr; }
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const float gu = (sgb * p[j] - acc[j]) + lam * u[j];
        const float gp = sgb * u[j] + lam * p[j];
        fixed_add(a.G64 + ru * D + j * LPT + l, gu);
        fixed_add(a.G64 + rp * D + j * LPT + l, gp);
    }
    if (l < R + 2) {                            // the 2 + R rows of the sample: one lane each
        ROWS_FLAG(a, myrow, l < R ? 1 : R);     // a negative slot weighs 1/R of a user / positive slot (epilogue: decay / (B R))
    }
}

template <int D, int LOSS>
static void launch_d(const MultiNegArgs &a, int act_dtype, bool wts, hipStream_t st) {
    constexpr int SPB = RowsGeo<D>::SPB;
    const dim3 grid((unsigned)((a.B + SPB - 1) / SPB)), block(256);
    DISPATCH_ROWS(act_dtype, wts, hipLaunchKernelGGL((k_multineg<D, TI, WTS, LOSS>), grid, block, 0, st, a));
}

int lgcn_multineg_launch(const MultiNegArgs &a, int d, int act_dtype, bool wts, hipStream_t st) {
    const bool softmax = a.loss == LGCN_LOSS_SOFTMAX;
    if (a.B <= 0 || a.R < 1 || a.R > LGCN_MAX_NEG_RATIO || a.neg_stride < a.B || (!softmax && a.loss != LGCN_LOSS_BPR) ||
        (softmax && !(a.tau > 0.f)) || (act_dtype != LGCN_F32 && act_dtype != LGCN_BF16)) {
        lgcn_set_error("multi-negative batch rows: bad launch arguments (negative ratio 1..16, neg_stride >= B, loss bpr or softmax "
                       "with temperature > 0, fp32 / bf16 tables)");
        return 3;
    }
    DISPATCH_D(d, {
        if (softmax) launch_d<D, LGCN_LOSS_SOFTMAX>(a, act_dtype, wts, st);
        else launch_d<D, LGCN_LOSS_BPR>(a, act_dtype, wts, st);
    });
    return 0;
}

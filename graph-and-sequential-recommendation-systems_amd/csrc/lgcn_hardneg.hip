// lgcn_hardneg.hip -- the batch-row launch of the fused LightGCN step with HARD NEGATIVES, DNS(M, N) (--hard_neg M with --neg_ratio R;
// lgcn_ctx_set_hard_neg), gfx950 (wave64).
//
// A sample is (u, p, n_1..n_R), R >= 2.  With e the rows of the model's output table (slot_row: the expression every batch-row
// launch of the dense-last form reads its rows through):
//   s_r   = e_u.e_{n_r}                                   the candidates' scores under the current model
//   rank  : s descending, ties by r ascending (duplicate ids inside a sample tie exactly)
//   j_b   = lgcn_hn_rank(seed, step, b, M)                a counter-based pick in 0..M-1 (lgcn_internal.h; M = 1: the hardest)
//   sel_b = the candidate of rank j_b
// and the step is the BPR step on the B triplets (u_b, p_b, n_sel(b)) -- what k_triplet_dense computes on that batch:
//   x = e_u.e_p - s_sel,  terms[b] = logsigmoid(x),  terms[B + b] = |e_u|^2 + |e_p|^2 + |e_sel|^2     (reg_ego: the tables' own rows)
//   gb = -sigmoid(-x) / B,  lam = decay / B (0 under reg_ego)
//   g_u = gb (e_p - e_sel) + lam e_u ;  g_p = gb e_u + lam e_p ;  g_sel = -gb e_u + lam e_sel
// THREE gradient rows, three row flags and three cnt slots of weight 1 per sample; the divisor is B.  (k_multineg weighs a
// negative slot 1 / R in cnt and lam_n and divides by B R: none of that here.)  The R - 1 unselected candidates get nothing.
//
// k_hardneg<D, TI, WTS>: the geometry of k_multineg -- one lane group of min(D, 64) lanes per sample, lane = column (mod 64), 256 /
// min(D, 64) samples per workgroup; lanes 0..R-1 of the group hold the candidates' ids (R <= 16 <= the smallest group), lanes R
// and R + 1 the user's and the positive's; no LDS; #pragma unroll 1 over r, so the registers do not grow with R.
//   score   one pass over the R rows, the row of candidate r + 1 in flight while candidate r is scored: s_r into lane r.
//   select  lane r < R counts the candidates that beat it (s_r' > s_r, or s_r' == s_r and r' < r): R shuffles.  The counts of
//           finite scores are a permutation of 0..R-1, so exactly one lane holds j_b; lanes >= R never vote.  (A NaN score
//           compares false both ways and may leave several lanes or none at a count: the lowest voting lane wins, candidate 0 if
//           none -- in range, deterministic.)
//   emit    the ONE selected row is read again (this workgroup read it a moment ago); its score is the one lane sel holds.
// The selected item id goes to sel_id[b] (library-owned): the backward chain's slot kernels (k_g32, k_finish) then run their
// three-slot forms on (users, pos, sel_id).  sel_out[b] (the caller's, may be NULL) gets the selected INDEX r.  A sample with an
// out-of-range id is void as in k_multineg (err flag, zero terms, nothing else) and stores -1 to both.
// The sample prologue (geometry, stale-bitmap loop, id check, user / positive pair, flag and count) is lgcn_batch_rows.h's, the one
// k_multineg opens with; the score pass and the emit are this kernel's own.  This file stays a translation unit of its own: the
// kernel shares no pass with k_multineg, and a unit per loss keeps one loss's edit out of the other's compilation.
#include "lgcn_batch_rows.h"      // RowsGeo and the sample prologue (bitmap loop, id check, user / positive pair, flag and count), DISPATCH_ROWS

template <int D, typename TI, bool WTS>
__global__ void __launch_bounds__(256) k_hardneg(HardNegArgs h) {
    const MultiNegArgs &a = h.m;
    ROWS_ZERO_STALE_BITMAP(a);
    ROWS_GEOMETRY(D);
    if (b >= a.B) return;                       // whole lane groups leave together
    const int R = a.R;
    ROWS_LOAD_IDS(a, ROWS_NEGS_FIRST, true, true);      // lane r < R holds candidate r, lanes R / R + 1 the user / positive
    if (bad) {                                  // an out-of-range id voids the whole sample: err flag, zero terms, no gradient
        if (l == 0) {
            atomicExch(a.err, 1); a.terms[b] = 0.f; a.terms[a.terms_stride + b] = 0.f;
            h.sel_id[b] = -1;
            if (h.sel_out) h.sel_out[b] = -1;
        }
        return;
    }
    const int64_t ru = (int64_t)__shfl(id, R, LPT), rp = (int64_t)__shfl(id, R + 1, LPT) + a.n_users;
    const bool ego = a.reg_ego != 0;
    const float lam = ego ? 0.f : a.lam;
    float u[CPT], p[CPT];
    float ps = 0.f, ru2 = 0.f, rp2 = 0.f;
    ROWS_PAIR(ps += u[j] * p[j])
    ps = group_sum<LPT>(ps);
    // ---- score.  s_r into lane r; the next candidate's rows fly while this one is scored.  The pass reads ONE row per candidate,
    // the output-table row.  slot_row also hands back the table's own row (n0 / nn0): that is the first term of e, loaded either
    // way, and the score pass does not keep it -- only the emit below needs n0, for the one selected row
    float s = 0.f;
    float n[CPT], n0[CPT], nn[CPT], nn0[CPT];
    {
        int64_t rn = (int64_t)__shfl(id, 0, LPT) + a.n_users;
        slot_row<D, TI, WTS>(a, rn, l, n, n0);
#pragma unroll 1
        for (int r = 0; r < R; r++) {
            const int64_t rnext = (int64_t)__shfl(id, r + 1 < R ? r + 1 : r, LPT) + a.n_users;
            if (r + 1 < R) slot_row<D, TI, WTS>(a, rnext, l, nn, nn0);
            float ns = 0.f;
#pragma unroll
            for (int j = 0; j < CPT; j++) ns += u[j] * n[j];
            ns = group_sum<LPT>(ns);
            if (l == r) s = ns;
            if (r + 1 < R) {
#pragma unroll
                for (int j = 0; j < CPT; j++) n[j] = nn[j];
            }
        }
    }
    // ---- select.  beaten = candidates that rank before this lane's; the lane at count j_b is the selection
    int beaten = 0;
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const float sr = __shfl(s, r, LPT);
        beaten += (sr > s || (sr == s && r < l)) ? 1 : 0;
    }
    const int jb = (int)lgcn_hn_rank(h.seed, h.step, b, h.top_m);
    const unsigned long long votes = ROWS_VOTES(l < R && beaten == jb);
    const int sel = votes ? __ffsll(votes) - 1 : 0;
    const int32_t nid = __shfl(id, sel, LPT);
    const int64_t rn = (int64_t)nid + a.n_users;
    const float ns = __shfl(s, sel, LPT);
    // ---- emit.  the BPR triplet (u, p, n_sel)
    slot_row<D, TI, WTS>(a, rn, l, n, n0);
    float rn2 = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; j++) { const float v = ego ? n0[j] : n[j]; rn2 += v * v; }
    const float rr = group_sum<LPT>(ru2 + rp2 + rn2);
    const float x = ps - ns;
    const float gb = -h.inv_B * sigmoid_neg_f(x);
    if (l == 0) {
        a.terms[b] = logsigmoid_f(x); a.terms[a.terms_stride + b] = rr;
        h.sel_id[b] = nid;
        if (h.sel_out) h.sel_out[b] = sel;
    }
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const float gu = gb * (p[j] - n[j]) + lam * u[j];
        const float gp = gb * u[j] + lam * p[j];
        const float gn = (-gb) * u[j] + lam * n[j];
        fixed_add(a.G64 + ru * D + j * LPT + l, gu);
        fixed_add(a.G64 + rp * D + j * LPT + l, gp);
        fixed_add(a.G64 + rn * D + j * LPT + l, gn);
    }
    if (l < 3) {                                // the three rows of the triplet: one lane each, every slot weighs 1
        const int64_t myrow = l == 0 ? ru : (l == 1 ? rp : rn);
        ROWS_FLAG(a, myrow, 1);
    }
}

template <int D>
static void launch_d(const HardNegArgs &h, int act_dtype, bool wts, hipStream_t st) {
    constexpr int SPB = RowsGeo<D>::SPB;
    const dim3 grid((unsigned)((h.m.B + SPB - 1) / SPB)), block(256);
    DISPATCH_ROWS(act_dtype, wts, hipLaunchKernelGGL((k_hardneg<D, TI, WTS>), grid, block, 0, st, h));
}

int lgcn_hardneg_launch(const HardNegArgs &h, int d, int act_dtype, bool wts, hipStream_t st) {
    const MultiNegArgs &a = h.m;
    if (a.B <= 0 || a.R < 2 || a.R > LGCN_MAX_NEG_RATIO || h.top_m < 1 || h.top_m > a.R || a.neg_stride < a.B || !h.sel_id ||
        (act_dtype != LGCN_F32 && act_dtype != LGCN_BF16)) {
        lgcn_set_error("hard-negative batch rows: bad launch arguments (negative ratio 2..16, hard negatives 1..R, neg_stride >= B, "
                       "fp32 / bf16 tables)");
        return 3;
    }
    DISPATCH_D(d, launch_d<D>(h, act_dtype, wts, st));
    return 0;
}

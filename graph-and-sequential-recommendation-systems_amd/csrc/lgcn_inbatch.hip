// lgcn_inbatch.hip -- the in-batch sampled softmax of the fused LightGCN step (--loss inbatch; lgcn_train_step_inbatch /
// lgcn_train_epoch_inbatch), gfx950 (wave64).
//
// A batch is B samples (u_b, p_b).  With e the rows of the model's output table (layer mean, or the weighted sum):
//   s_{b,c} = e_{u_b}.e_{p_c}                                  for sound b, c (both ids of the sample in range)
//   A_b     = { c sound, c != b, p_c != p_b, u_c != u_b }       the competitors of sample b
//   z_{b,c} = (s_{b,c} - s_{b,b}) / tau,  l_b = log(1 + sum_{c in A_b} exp(z_{b,c})),  sm = 1/B sum_b l_b,  terms[b] = -l_b
//   q_{b,c} = exp(z_{b,c}) / (1 + sum_j exp(z_{b,j})),  Q_b = sum_c q_{b,c}
//   W[b,c] = q_{b,c} / (tau B) (c in A_b),  W[b,b] = -Q_b / (tau B),  0 otherwise
//   g_{u_b} = sum_c W[b,c] e_{p_c} + lam e_{u_b},   g_{p_c} = sum_b W[b,c] e_{u_b} + lam e_{p_c},   lam = decay / B
//
// Four launches between the forward and the backward of the step, over a workspace of Bp = B rounded up to 32 rows:
//   k_inbatch_rows   one lane group of min(D, 64) lanes per sample (the sample prologue of lgcn_batch_rows.h).  Gathers e_u
//                    and e_p through slot_row -- the expression every loss uses -- into dense fp32 U[Bp][D], P[Bp][D] (zero
//                    rows for void samples and for the padding b >= B), writes s_{b,b}, the reg term, the ids (-1: void),
//                    zeroes the stale bitmap, flags the two rows, counts them and adds the lam terms to G64.
//   k_inbatch_norm   one wave per (32 users, part of the item sweep).  The score tile is P.U^T on the fp32-input MFMA
//                    (v_mfma_f32_32x32x2_f32: exact fp32, a k-ordered fmaf chain), so a lane holds ONE user (column) and 16
//                    items (rows) of the tile: the running (m, r) of the user -- sum of exponentials = exp(m) (1 + r), the
//                    first maximal term being the 1 -- lives in the lane, the two lane halves are merged with one shuffle and
//                    one partial per part leaves.  No atomics on floats, no LDS.
//   k_inbatch_diag   one lane group per sample again: merges the parts in ascending order (m_b = max(0, max z): no exp of a
//                    positive argument; the term that equals exp(0) stays out of the sum, so a tiny l_b keeps its relative
//                    accuracy), writes terms[b] and the merged (M_b, 1 + Zm1_b), and adds the diagonal W[b,b] to both rows.
//   k_inbatch_grad   one wave per (32 owned rows, part of the sweep, role, 128-column block).  Role "users" recomputes the
//                    tile as P.U^T (user on the lane), role "items" as U.P^T (item on the lane); W is formed elementwise in
//                    the 16 accumulator registers and register i IS the A operand of the next 32x32x2 MFMA (output row =
//                    lane & 31 = the owned index, k = lane half = tile rows r and r + 4 of register i): W^T.Other accumulates
//                    into 32 x 128 fp32 with no lane movement and no LDS.  The partial rows go to G64 with fixed_add, so the
//                    split of the sweep has no ordering effect.
// s_{b,c} has the same bits in all three places: the same k order (lane half h walks columns h D/2 .. h D/2 + D/2 - 1 of both
// operands) and fp32 products commute, so exp(z - M) <= 1 everywhere and q, Q_b are consistent.
// The sweep itself -- part bounds, operand forms, the second product, the projected epilogue -- is lgcn_inbatch_tile.h's, shared with
// lgcn_directau.hip; k_inbatch_norm and k_inbatch_grad hold the roles, the masks and the weights.
// Operands: up to D = 64 (IB_REG_D) a lane keeps its row of the owned side in registers for the whole sweep and loads the swept
// side's NEXT tile (and this tile's ids, normalisers and second-product operands) while the score MFMAs of this tile run; above
// that the rows are streamed from L2 in chunks of 8 columns per lane half (128 floats per operand would not fit beside the
// 64-register gradient accumulator).  Measured (profiles/inbatch/README.md): the passes are bound by the vector ALU work on
// the 16 scores of a lane (a division, an expf, the mask compares), not by the matrix pipe.
// The sweep split: LGCN_INBATCH_PART_TILES = 8 tiles (256 rows) per workgroup -- 64 owner tiles x 8 parts (x 2 roles) at
// B = 2048.  Ragged B and every D are handled by the zero rows of the workspace and the id -1 of a void row, never by a
// branch in the MFMA loop.
//
// Two options (lgcn_ctx_set_inbatch_scores), compile-time axes COS / LQ of the same four launches; the (false, false)
// instantiations are the kernels above and hold no other code:
//   COS  s_{b,c} = e^_{u_b}.e^_{p_c}, e^ = e inv(e), inv(e) = 1 / |e| (0 for |e| = 0; sqrtf of the fp32 sum of squares and an IEEE
//        division).  k_inbatch_rows writes U^, P^ into U, P, inv into invu / invp and takes s_bb from the normalised values; the
//        reg term and lam e stay on the raw rows.  The chain through the normalisation is a projection,
//        g_o = inv_o (sum_x W[x,o] other^_x - t_o own^_o), t_o = sum_x W[x,o] s[x,o]: k_inbatch_grad sums t_o over the 16
//        accumulator registers in which it forms W from the scores (per lane, the two halves added with one shuffle) and applies
//        the projection to its partial rows in the epilogue -- it is linear, so the parts of the sweep still meet order-free in
//        G64; k_inbatch_diag adds the diagonal's inv_u W[b,b] (p^_b - s_bb u^_b) and its mirror.
//   LQ   z_{b,c} = (s_{b,c} - s_{b,b}) / tau - (lq_{p_c} - lq_{p_b}): k_inbatch_rows gathers lq[p_b] into lqb (after the id check;
//        0 for void rows and padding), the two tile passes load the lane's and the tile rows' lq where s_bb and the ids are
//        loaded; fl(lq_c - lq_b) has the same bits in all three places.
//
// Mixed negative sampling (lgcn_train_step_inbatch_mix), a third compile-time axis MIX of the same four launches; the
// MIX = false instantiations are the kernels above.  A sample carries R negatives n_{b,1..R}; the B R negatives of the sound samples
// are a pool shared by the whole batch, extra columns of every sample's score row in the same log-sum-exp:
//   z_{b,(c,r)} = (e^_{u_b}.e^_{n_{c,r}} - s_{b,b}) / tau - (lq_{n_{c,r}} - lq_{p_b}),  masked only where n_{c,r} = p_b
//   g_{n_{c,r}} = sum_b W[b,(c,r)] e^_{u_b} + lam / R e_{n_{c,r}}  (through its own normalisation under cosine), no diagonal
// The item side grows from Bp to (1 + R) Bp rows: pool row (r, c) is row Bp (1 + r) + c of P and of pid (id -1 and a zero row where
// sample c is void or padding), its lq / inv in the launch's own vectors over the same rows.
//   k_inbatch_rows  the negatives' ids sit in lanes 2 .. R + 1 of the group and are checked in the same ballot; the R rows are streamed
//                   through slot_row one at a time (the register count does not grow with R), written to the pool region, regularised
//                   (lam / R e to G64, 1 / R |e|^2 to the reg term) and flagged / counted as k_multineg counts them (R, R, 1).
//   k_inbatch_norm  sweeps (1 + R) Bp / 32 item tiles; the mask rule follows the tile's kind, which is uniform: no divergence.
//   k_inbatch_diag  merges the larger number of parts.
//   k_inbatch_grad  role "users" owns Bp / 32 tiles and sweeps all item tiles, role "items" owns (1 + R) Bp / 32 tiles and sweeps the
//                   user tiles: both extents differ, so the grid is flat (the users' workgroups first).
#include "lgcn_batch_rows.h"        // RowsGeo and the sample prologue, DISPATCH_ROWS
#include "lgcn_inbatch_tile.h"      // the score tile (ib_scores, IbRow / ib_load / ib_scores_reg, IB_REG_D) and the pieces of the sweep round it

// the three [cap] vectors of the score options, carved behind `part` in the context's workspace
__device__ __forceinline__ float *ib_invu(const InBatchArgs &ia) { return ia.part + 2 * (int64_t)ia.cap * lgcn_inbatch_parts(ia.cap); }
__device__ __forceinline__ float *ib_invp(const InBatchArgs &ia) { return ib_invu(ia) + ia.cap; }
__device__ __forceinline__ float *ib_lqb(const InBatchArgs &ia) { return ib_invu(ia) + 2 * (int64_t)ia.cap; }

// the same three vectors of a mixed launch: its own pointers, the item-side ones over the (1 + R) Bp item rows
template <bool MIX> __device__ __forceinline__ float *ibx_invu(const InBatchArgs &ia) { if constexpr (MIX) return ia.xinvu; else return ib_invu(ia); }
template <bool MIX> __device__ __forceinline__ float *ibx_invp(const InBatchArgs &ia) { if constexpr (MIX) return ia.xinvp; else return ib_invp(ia); }
template <bool MIX> __device__ __forceinline__ float *ibx_lq(const InBatchArgs &ia) { if constexpr (MIX) return ia.xlq; else return ib_lqb(ia); }

// (m, r) <- (m, r) + (m2, r2), each standing for the sum exp(m) (1 + r) (m = -inf: the empty sum); every exponent is <= 0
__device__ __forceinline__ void ib_merge(float &m, float &r, float m2, float r2) {
    if (m2 == -INFINITY) return;
    if (m == -INFINITY) { m = m2; r = r2; return; }
    if (m >= m2) r = r + (1.f + r2) * expf(m2 - m);
    else { r = r2 + (1.f + r) * expf(m - m2); m = m2; }
}

template <int D, typename TI, bool WTS, bool COS, bool LQ, bool MIX>
__global__ void __launch_bounds__(256) k_inbatch_rows(InBatchArgs ia) {
    const MultiNegArgs &a = ia.m;
    ROWS_ZERO_STALE_BITMAP(a);
    ROWS_GEOMETRY(D);
    const int Bp = lgcn_inbatch_rows(a.B);
    if (b >= Bp) return;                        // whole lane groups leave together
    // lane 0 holds the user, lane 1 the positive, with MIX lanes 2 .. R + 1 the sample's negatives; the padding b >= B is bad too
    ROWS_LOAD_IDS(a, ROWS_PAIR_FIRST, MIX, b < a.B);
    if (bad) {          // padding, or an out-of-range id: a zero row and a zero column of the score matrix, masked by uid = -1
#pragma unroll
        for (int j = 0; j < CPT; j++) { ia.U[(int64_t)b * D + j * LPT + l] = 0.f; ia.P[(int64_t)b * D + j * LPT + l] = 0.f; }
        if (l == 0) {
            ia.uid[b] = -1; ia.pid[b] = -1; ia.sbb[b] = 0.f; ia.mrg[2 * b] = 0.f; ia.mrg[2 * b + 1] = 1.f;
            if constexpr (COS) { ibx_invu<MIX>(ia)[b] = 0.f; ibx_invp<MIX>(ia)[b] = 0.f; }
            if constexpr (LQ) ibx_lq<MIX>(ia)[b] = 0.f;
            if (b < a.B) { atomicExch(a.err, 1); a.terms[b] = 0.f; a.terms[a.terms_stride + b] = 0.f; }
        }
        if constexpr (MIX) {                    // no pool column either: R zero rows with id -1
            for (int r = 0; r < a.R; r++) {
                const int64_t x = (int64_t)Bp * (1 + r) + b;
#pragma unroll
                for (int j = 0; j < CPT; j++) ia.P[x * D + j * LPT + l] = 0.f;
                if (l == 0) {
                    ia.pid[x] = -1;
                    if constexpr (COS) ia.xinvp[x] = 0.f;
                    if constexpr (LQ) ia.xlq[x] = 0.f;
                }
            }
        }
        return;
    }
    const int32_t iu = __shfl(id, 0, LPT), ip = __shfl(id, 1, LPT);
    const int64_t ru = (int64_t)iu, rp = (int64_t)ip + a.n_users;
    const bool ego = a.reg_ego != 0;
    const float lam = ego ? 0.f : a.lam;
    float u[CPT], p[CPT];
    float ps = 0.f, ru2 = 0.f, rp2 = 0.f;
    ROWS_PAIR(ps += u[j] * p[j])
    ps = group_sum<LPT>(ps);
    float rr = group_sum<LPT>(ru2 + rp2);
    if constexpr (MIX) {
        // the sample's R negatives become pool rows Bp (1 + r) + b of P (normalised under cosine), streamed one at a time
        const float lam_n = ego ? 0.f : a.lam_n;
        float srn = 0.f;
#pragma unroll 1
        for (int r = 0; r < a.R; r++) {
            const int32_t in = __shfl(id, 2 + r, LPT);
            const int64_t rn = (int64_t)in + a.n_users, x = (int64_t)Bp * (1 + r) + b;
            float n[CPT], n0[CPT];
            slot_row<D, TI, WTS>(a, rn, l, n, n0);
            float inv_n = 1.f;
            if constexpr (COS) {
                float nn = 0.f;
#pragma unroll
                for (int j = 0; j < CPT; j++) nn += n[j] * n[j];
                nn = group_sum<LPT>(nn);
                inv_n = rows_inv_norm(nn);
            }
#pragma unroll
            for (int j = 0; j < CPT; j++) {
                const float v = ego ? n0[j] : n[j];
                srn += v * v;
                if constexpr (COS) ia.P[x * D + j * LPT + l] = n[j] * inv_n; else ia.P[x * D + j * LPT + l] = n[j];
                if (lam_n != 0.f) fixed_add(a.G64 + rn * D + j * LPT + l, lam_n * n[j]);
            }
            if (l == 0) {
                ia.pid[x] = in;
                if constexpr (COS) ia.xinvp[x] = inv_n;
                if constexpr (LQ) ia.xlq[x] = ia.item_logq[in];         // (in passed the id check above)
            }
        }
        rr = group_sum<LPT>(ru2 + rp2 + srn * a.inv_R);
    }
    if constexpr (COS) {
        // |e| = sqrtf of the fp32 sum of squares, inv = 1 / |e| by an IEEE division (0 for a row of norm 0): two roundings.
        // U, P and s_bb are those of the rows over their norms; the reg term and lam e stay on the rows themselves
        float nu = 0.f, np = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; j++) { nu += u[j] * u[j]; np += p[j] * p[j]; }
        nu = group_sum<LPT>(nu); np = group_sum<LPT>(np);
        const float inv_u = rows_inv_norm(nu), inv_p = rows_inv_norm(np);
        ps = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            const float uh = u[j] * inv_u, ph = p[j] * inv_p;
            ps += uh * ph;
            ia.U[(int64_t)b * D + j * LPT + l] = uh;
            ia.P[(int64_t)b * D + j * LPT + l] = ph;
            if (lam != 0.f) {
                fixed_add(a.G64 + ru * D + j * LPT + l, lam * u[j]);
                fixed_add(a.G64 + rp * D + j * LPT + l, lam * p[j]);
            }
        }
        ps = group_sum<LPT>(ps);
        if (l == 0) { ibx_invu<MIX>(ia)[b] = inv_u; ibx_invp<MIX>(ia)[b] = inv_p; }
    } else {
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            ia.U[(int64_t)b * D + j * LPT + l] = u[j];
            ia.P[(int64_t)b * D + j * LPT + l] = p[j];
            if (lam != 0.f) {
                fixed_add(a.G64 + ru * D + j * LPT + l, lam * u[j]);
                fixed_add(a.G64 + rp * D + j * LPT + l, lam * p[j]);
            }
        }
    }
    if (l == 0) { ia.uid[b] = iu; ia.pid[b] = ip; ia.sbb[b] = ps; a.terms[a.terms_stride + b] = rr; }
    if constexpr (LQ) { if (l == 0) ibx_lq<MIX>(ia)[b] = ia.item_logq[ip]; }          // (ip passed the id check above)
    if constexpr (MIX) {
        if (l < 2 + a.R) {                      // the 2 + R rows of the sample: one lane each, counted as k_multineg counts them
            const int64_t myrow = l == 0 ? ru : (int64_t)id + a.n_users;
            ROWS_FLAG(a, myrow, l < 2 ? a.R : 1);
        }
    } else if (l < 2) {                         // the 2 rows of the sample: one lane each
        const int64_t myrow = l == 0 ? ru : rp;
        ROWS_FLAG(a, myrow, 1);
    }
}

template <int D, bool LQ, bool MIX>
__global__ void __launch_bounds__(64) k_inbatch_norm(InBatchArgs ia) {
    const int l = threadIdx.x, j = l & 31, h = l >> 5;
    const int Bp = lgcn_inbatch_rows(ia.m.B);
    int nT = Bp / 32;                           // item tiles of the sweep
    if constexpr (MIX) nT = (1 + ia.m.R) * nT;  // ... the pool's behind the batch's own
    const int b = blockIdx.x * 32 + j;          // this lane's user (a column of the tile)
    IB_PART_BOUNDS(blockIdx.y, nT);
    const int32_t ub = ia.uid[b], pb = ia.pid[b];
    const float sbb = ia.sbb[b], tau = ia.m.tau;
    float lqb = 0.f;                            // log Q of the lane's own positive
    if constexpr (LQ) lqb = ibx_lq<MIX>(ia)[b];
    const float *brow = ia.U + (int64_t)b * D + h * (D / 2);
    float m = -INFINITY, r = 0.f;
    IB_SWEEP_BEGIN(D, own, ia.P, t0, true)
#pragma unroll 1
    for (int t = t0; t < t1; t++) {
        // this tile's ids and the next tile's rows are in flight while this tile is multiplied
        int32_t ucs[16], pcs[16];
        bool pool = false;                      // the tile's kind (uniform): a pool tile has no users and its own mask rule
        if constexpr (MIX) pool = t >= Bp / 32;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int c = t * 32 + mfma32_row(reg, h);
            if constexpr (MIX) ucs[reg] = pool ? 0 : ia.uid[c]; else ucs[reg] = ia.uid[c];
            pcs[reg] = ia.pid[c];
        }
        float lqs[LQ ? 16 : 1];
        if constexpr (LQ) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) lqs[reg] = ibx_lq<MIX>(ia)[t * 32 + mfma32_row(reg, h)];
        }
        f32x16 acc;
        IB_SWEEP_SCORES(D, acc, own, ia.P, t);
        float z[16], tmax = -INFINITY;
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int c = t * 32 + mfma32_row(reg, h);
            const int32_t uc = ucs[reg], pc = pcs[reg];
            bool ok = ub >= 0 && uc >= 0 && c != b && pc != pb && uc != ub;
            if constexpr (MIX) { if (pool) ok = ub >= 0 && pc >= 0 && pc != pb; }
            if constexpr (LQ) z[reg] = ok ? (acc[reg] - sbb) / tau - (lqs[reg] - lqb) : -INFINITY;
            else z[reg] = ok ? (acc[reg] - sbb) / tau : -INFINITY;
            tmax = fmaxf(tmax, z[reg]);
        }
        bool excl = false;                      // a new maximum: its first occurrence becomes the 1 of (1 + r)
        if (tmax > m) { r = (1.f + r) * expf(m - tmax); m = tmax; excl = true; }
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            if (z[reg] == -INFINITY) continue;
            if (excl && z[reg] == m) excl = false;
            else r += expf(z[reg] - m);
        }
    }
    const float m2 = __shfl_xor(m, 32), r2 = __shfl_xor(r, 32);
    if (h == 0) {                               // half 0 first, then half 1: a fixed order
        ib_merge(m, r, m2, r2);
        float *o = ia.part + ((int64_t)blockIdx.y * Bp + b) * 2;
        o[0] = m; o[1] = r;
    }
}

template <int D, bool COS, bool MIX>
__global__ void __launch_bounds__(256) k_inbatch_diag(InBatchArgs ia) {
    const MultiNegArgs &a = ia.m;
    ROWS_GEOMETRY(D);
    if (b >= a.B) return;
    const int32_t iu = ia.uid[b], ip = ia.pid[b];
    if (iu < 0) return;                         // void: k_inbatch_rows wrote its zero terms
    const int Bp = lgcn_inbatch_rows(a.B);
    int NP = lgcn_inbatch_parts(a.B);
    if constexpr (MIX) NP = lgcn_inbatch_mix_parts(a.B, a.R);
    float m = -INFINITY, r = 0.f;               // every lane of the group merges the same parts in the same order
    for (int p = 0; p < NP; p++) { const float *q = ia.part + ((int64_t)p * Bp + b) * 2; ib_merge(m, r, q[0], q[1]); }
    // with the positive's own exp(0): 1 + sum_c exp(z_c) = exp(M) (1 + Zm1), M = max(0, m)
    float M = 0.f, zm1 = 0.f, Q = 0.f;
    if (m > 0.f) { M = m; zm1 = r + expf(-m); Q = (1.f + r) / (1.f + zm1); }          // the 1 is the first maximal competitor's term
    else if (m != -INFINITY) { zm1 = expf(m) * (1.f + r); Q = zm1 / (1.f + zm1); }    // the 1 is the positive's term
    if (l == 0) { a.terms[b] = -(M + log1pf(zm1)); ia.mrg[2 * b] = M; ia.mrg[2 * b + 1] = 1.f + zm1; }
    if (Q == 0.f) return;                       // no competitor (B = 1, everything masked): only the regulariser moves the rows
    const float wd = -(Q * a.inv_tauB);         // W[b,b]
    const int64_t ru = (int64_t)iu, rp = (int64_t)ip + a.n_users;
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const int64_t o = (int64_t)b * D + j * LPT + l;
        if constexpr (COS) {                    // the diagonal through the normalisation: inv W[b,b] (other^ - s_bb own^)
            const float uh = ia.U[o], ph = ia.P[o], sbb = ia.sbb[b];
            fixed_add(a.G64 + ru * D + j * LPT + l, ibx_invu<MIX>(ia)[b] * (wd * (ph - sbb * uh)));
            fixed_add(a.G64 + rp * D + j * LPT + l, ibx_invp<MIX>(ia)[b] * (wd * (uh - sbb * ph)));
        } else {
            fixed_add(a.G64 + ru * D + j * LPT + l, wd * ia.P[o]);
            fixed_add(a.G64 + rp * D + j * LPT + l, wd * ia.U[o]);
        }
    }
}

template <int D, bool COS, bool LQ, bool MIX>
__global__ void __launch_bounds__(64) k_inbatch_grad(InBatchArgs ia) {
    constexpr int CB = ib_grad_blocks(D);        // 32-column blocks of the output this workgroup accumulates
    const int l = threadIdx.x, j = l & 31, h = l >> 5;
    const int Bp = lgcn_inbatch_rows(ia.m.B);
    int nT = Bp / 32;                           // tiles of the swept side
    int role = blockIdx.z & 1, col0 = (blockIdx.z >> 1) * 128;              // role 0: the owned rows are users, 1: items
    int bx = blockIdx.x, by = blockIdx.y;       // the owned tile, the part of the sweep
    bool pool_o = false;                        // mixed: the owned tile is a pool tile (role 1 only; uniform)
    if constexpr (MIX) {
        // the two roles differ in both extents -- users: Bp / 32 owned tiles x the parts of the (1 + R) Bp / 32 item tiles; items:
        // (1 + R) Bp / 32 owned tiles x the parts of the Bp / 32 user tiles -- so the grid is flat: the users' workgroups first
        const int nTI = (1 + ia.m.R) * nT, nb0 = nT * lgcn_inbatch_mix_parts(ia.m.B, ia.m.R);
        const int i = (int)blockIdx.x;
        col0 = blockIdx.z * 128;
        if (i < nb0) { role = 0; bx = i % nT; by = i / nT; nT = nTI; }
        else { role = 1; bx = (i - nb0) % nTI; by = (i - nb0) / nTI; pool_o = bx >= nT; }
    }
    const float *own = role == 0 ? ia.U : ia.P, *oth = role == 0 ? ia.P : ia.U;
    const int o = bx * 32 + j;                  // this lane's owned index (a column of the score tile)
    IB_PART_BOUNDS(by, nT);
    int32_t uo, po = ia.pid[o];
    float sbb_o, M_o, den_o;
    if constexpr (MIX) {                        // an owned item index may lie in the pool: no user, no s_bb, no merged pair there
        uo = pool_o ? 0 : ia.uid[o];
        sbb_o = role == 0 ? ia.sbb[o] : 0.f; M_o = role == 0 ? ia.mrg[2 * o] : 0.f; den_o = role == 0 ? ia.mrg[2 * o + 1] : 1.f;
    } else { uo = ia.uid[o]; sbb_o = ia.sbb[o]; M_o = ia.mrg[2 * o]; den_o = ia.mrg[2 * o + 1]; }
    const float tau = ia.m.tau, inv_tauB = ia.m.inv_tauB;
    float lq_o = 0.f;                           // log Q of the owned sample's positive
    if constexpr (LQ) lq_o = ibx_lq<MIX>(ia)[o];
    float tproj = 0.f;                          // cosine: sum_x W[x][o] s[x][o] over this lane's 16 rows of every tile
    const float *brow = own + (int64_t)o * D + h * (D / 2);
    IB_GRAD_ZERO();
    IB_SWEEP_BEGIN(D, ownr, oth, t0, true)
#pragma unroll 1
    for (int t = t0; t < t1; t++) {
        // what the tile needs besides its scores is in flight while the scores are multiplied: the rows' ids, the users' s_bb and
        // merged (M, 1 + Zm1) under role 1 (under role 0 they are the lane's own), the B operands of the second product and,
        // in the register form, the next tile's rows
        int32_t uxs[16], pxs[16];
        float sbs[16], Ms[16], dens[16], ob[16][CB], lqd[LQ ? 16 : 1];
        bool pool = false;                      // mixed: the pairs of this tile are (user, pool column) -- uniform
        if constexpr (MIX) pool = pool_o || (role == 0 && t >= Bp / 32);
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int x = t * 32 + mfma32_row(reg, h);          // the other side's index (a row of the tile)
            if constexpr (MIX) uxs[reg] = (role == 0 && pool) ? 0 : ia.uid[x]; else uxs[reg] = ia.uid[x];
            pxs[reg] = ia.pid[x];
            // the USER of the pair owns s_bb and the merged (M, 1 + Zm1): the lane's under role 0, the row's under role 1
            sbs[reg] = role == 0 ? sbb_o : ia.sbb[x];
            Ms[reg] = role == 0 ? M_o : ia.mrg[2 * x]; dens[reg] = role == 0 ? den_o : ia.mrg[2 * x + 1];
            // lq of the pair's ITEM less lq of the pair's user's own positive: the row's less the lane's under role 0
            if constexpr (LQ) { const float lq_x = ibx_lq<MIX>(ia)[x]; lqd[reg] = role == 0 ? lq_x - lq_o : lq_o - lq_x; }
            IB_GRAD_PREFETCH(D, oth, x);
        }
        f32x16 w;
        IB_SWEEP_SCORES(D, w, ownr, oth, t);
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int x = t * 32 + mfma32_row(reg, h);
            bool ok = uo >= 0 && uxs[reg] >= 0 && x != o && pxs[reg] != po && uxs[reg] != uo;
            // a pool pair: a sound user, a pool column that exists, another item than the user's positive
            if constexpr (MIX) { if (pool) ok = (role == 0 ? uo >= 0 && pxs[reg] >= 0 : uxs[reg] >= 0 && po >= 0) && pxs[reg] != po; }
            float z;
            if constexpr (LQ) z = (w[reg] - sbs[reg]) / tau - lqd[reg]; else z = (w[reg] - sbs[reg]) / tau;
            if constexpr (COS) {
                const float s = w[reg];
                w[reg] = ok ? expf(z - Ms[reg]) / dens[reg] * inv_tauB : 0.f;
                tproj += w[reg] * s;
            } else {
                w[reg] = ok ? expf(z - Ms[reg]) / dens[reg] * inv_tauB : 0.f;
            }
        }
        IB_GRAD_PRODUCT(D, oth, t);              // g[owned][col] += sum_x W[x][owned] Other[x][col]
    }
    if constexpr (COS) IB_GRAD_TPROJ_COMBINE();
    // rows of g: owned index blockIdx.x * 32 + mfma32_row(reg, h); columns col0 + cb * 32 + j
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
        const int ob = bx * 32 + mfma32_row(reg, h);
        float t_row = 0.f;
        if constexpr (COS) t_row = IB_GRAD_TPROJ_ROW(reg);          // (every lane takes part: before the skip)
        int32_t us;
        if constexpr (MIX) us = role == 0 ? ia.uid[ob] : ia.pid[ob]; else us = ia.uid[ob];        // (a pool row has only its item id)
        if (us < 0) continue;                   // void or padding: no row to add to (its W is zero)
        int64_t row;
        if constexpr (MIX) row = role == 0 ? (int64_t)us : (int64_t)us + ia.m.n_users;
        else row = role == 0 ? (int64_t)us : (int64_t)ia.pid[ob] + ia.m.n_users;
        if constexpr (COS) {
            // the chain through the normalisation, per part (it is linear): inv_o (sum_x W own-side^ - t own^), DESIGN 4.20
            const float inv_o = (role == 0 ? ibx_invu<MIX>(ia) : ibx_invp<MIX>(ia))[ob];
            IB_GRAD_ADD_PROJECTED(D, ia.m.G64, own, inv_o);
        } else {
#pragma unroll
            for (int cb = 0; cb < CB; cb++) fixed_add(ia.m.G64 + row * D + col0 + cb * 32 + j, g[cb][reg]);
        }
    }
}

template <int D, bool COS, bool LQ, bool MIX>
static void launch_d(const InBatchArgs &a, int act_dtype, bool wts, hipStream_t st) {
    constexpr int SPB = RowsGeo<D>::SPB;
    const int Bp = lgcn_inbatch_rows(a.m.B), NP = lgcn_inbatch_parts(a.m.B);
    const dim3 rows_grid((unsigned)((Bp + SPB - 1) / SPB)), diag_grid((unsigned)((a.m.B + SPB - 1) / SPB));
    DISPATCH_ROWS(act_dtype, wts, hipLaunchKernelGGL((k_inbatch_rows<D, TI, WTS, COS, LQ, MIX>), rows_grid, dim3(256), 0, st, a));
    if constexpr (MIX) {
        // the item sweep is (1 + R) times as long; the gradient's grid is flat (users' workgroups, then the items')
        const int nT = Bp / 32, nTI = (1 + a.m.R) * nT, NPX = lgcn_inbatch_mix_parts(a.m.B, a.m.R);
        hipLaunchKernelGGL((k_inbatch_norm<D, LQ, true>), dim3((unsigned)nT, (unsigned)NPX), dim3(64), 0, st, a);
        hipLaunchKernelGGL((k_inbatch_diag<D, COS, true>), diag_grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL((k_inbatch_grad<D, COS, LQ, true>), dim3((unsigned)(nT * NPX + nTI * NP), 1u, (unsigned)(D > 128 ? D / 128 : 1)), dim3(64), 0, st, a);
    } else {
        hipLaunchKernelGGL((k_inbatch_norm<D, LQ, false>), dim3((unsigned)(Bp / 32), (unsigned)NP), dim3(64), 0, st, a);
        hipLaunchKernelGGL((k_inbatch_diag<D, COS, false>), diag_grid, dim3(256), 0, st, a);
        hipLaunchKernelGGL((k_inbatch_grad<D, COS, LQ, false>), dim3((unsigned)(Bp / 32), (unsigned)NP, 2u * (D > 128 ? D / 128 : 1)), dim3(64), 0, st, a);
    }
}

// the two options are compile-time axes: (dot, no logq) are the instantiations a context that was never told launches
template <int D, bool MIX>
static void launch_opts(const InBatchArgs &a, int act_dtype, bool wts, hipStream_t st) {
    const bool cosine = a.score == LGCN_SCORE_COSINE, lq = a.item_logq != nullptr;
    if (cosine) { if (lq) launch_d<D, true, true, MIX>(a, act_dtype, wts, st); else launch_d<D, true, false, MIX>(a, act_dtype, wts, st); }
    else { if (lq) launch_d<D, false, true, MIX>(a, act_dtype, wts, st); else launch_d<D, false, false, MIX>(a, act_dtype, wts, st); }
}

int lgcn_inbatch_launch(const InBatchArgs &a, int d, int act_dtype, bool wts, hipStream_t st) {
    if (a.m.B <= 0 || a.m.loss != LGCN_LOSS_INBATCH || !(a.m.tau > 0.f) || !(a.m.inv_tauB > 0.f) ||
        (act_dtype != LGCN_F32 && act_dtype != LGCN_BF16) || !a.U || !a.P || !a.sbb || !a.uid || !a.pid || !a.part || !a.mrg ||
        a.cap % 32 != 0 || a.m.B > a.cap || !a.m.users || !a.m.pos || !a.m.G64 || !a.m.terms || a.m.terms_stride < a.m.B) {
        lgcn_set_error("in-batch softmax rows: bad launch arguments (0 < B <= the workspace's rows, loss inbatch with temperature > 0, "
                       "fp32 / bf16 tables, a workspace of a multiple of 32 rows)");
        return 3;
    }
    if (a.score != LGCN_SCORE_DOT && a.score != LGCN_SCORE_COSINE) {
        lgcn_set_error("in-batch softmax rows: bad launch arguments (score dot or cosine)");
        return 3;
    }
    if (a.mix) {        // the mixed step: the pool's rows must fit the item side of the workspace
        const int64_t rows = (1 + (int64_t)a.m.R) * lgcn_inbatch_rows(a.m.B);
        if (a.m.R < 1 || a.m.R > LGCN_MAX_NEG_RATIO || !a.m.negs || a.m.neg_stride < a.m.B || rows > a.icap || !a.xinvu || !a.xinvp || !a.xlq) {
            lgcn_set_error("in-batch softmax rows: bad launch arguments (mixed negatives: negative ratio 1..16 within the workspace's item rows, "
                           "neg_stride >= B)");
            return 3;
        }
        DISPATCH_D(d, (launch_opts<D, true>(a, act_dtype, wts, st)));
        return 0;
    }
    DISPATCH_D(d, (launch_opts<D, false>(a, act_dtype, wts, st)));
    return 0;
}

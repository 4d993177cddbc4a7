// lgcn_directau.hip -- the alignment-and-uniformity loss of the fused LightGCN step (--loss directau; lgcn_train_step_directau /
// lgcn_train_epoch_directau), gfx950 (wave64).  DirectAU (Wang et al., KDD 2022): no negatives at all.
//
// A batch is B samples (u_b, p_b).  With e the rows of the model's output table (layer mean, or the weighted sum),
// e^ = e inv(e), inv(e) = 1 / |e| (0 for |e| = 0: the cosine option's definition), x_b = e^_{u_b}, y_b = e^_{p_b}:
//   align   = 1/B sum_b |x_b - y_b|^2
//   k_{b,c} = exp(-2 |x_b - x_c|^2)  for sound b != c BY POSITION,   Z_X = sum_{b<c} k_{b,c},   unif(X) = log(Z_X / (B (B - 1) / 2))
//   loss    = align + gamma (unif(X) + unif(Y)) / 2 + decay reg            (Z = 0 -- fewer than two sound samples: unif = 0)
//   g_{x_b} = 2/B (x_b - y_b) + sum_{c != b} W[b,c] (x_c - x_b),  W[b,c] = (2 gamma / Z_X) k_{b,c}   (symmetric);  its mirror for y
//   g_{e}   = inv(e) (g_x - (g_x.x) x) + lam e,   lam = decay / B         (the projection of the cosine in-batch step)
// |x_b - x_c|^2 is evaluated as (q_b + q_c) - 2 s_{b,c} with s the MFMA score and q_b = the fp32 sum of squares of the stored x_b
// (1 up to rounding; 0 for a row of norm 0, which keeps its exact distance to every other row).
//
// Four launches between the forward and the backward of the step, over a workspace of Bp = B rounded up to 32 rows (the in-batch
// step's conventions: zero rows and id -1 for void samples and for the padding, no branch in the MFMA loop for raggedness):
//   k_directau_rows   one lane group of min(D, 64) lanes per sample (the sample prologue of lgcn_batch_rows.h): gathers
//                     e_u, e_p through slot_row, writes x, y, inv, q, the ids and the alignment term |x - y|^2, the reg term, zeroes
//                     the stale bitmap, flags the two rows, counts them and adds the lam terms to G64.
//   k_directau_norm   one wave per (side, owner tile I, part of the sweep).  The score tile is T.T^T of ONE table on the fp32-input
//                     MFMA (the k order of ib_scores); k is formed in the 16 accumulator registers, masked by position (only c > b
//                     counts: tiles J < I are skipped, the diagonal tile keeps its upper triangle -- half the pass) and by the ids
//                     (a zero padding row would add exp(-4) per pair), summed per lane in register order, then over the wave
//                     with an xor-shuffle tree: one partial per (side, part, tile).  No atomics on floats, no LDS.
//   k_directau_merge  one lane group per sample.  Every wave sums the partials of both sides in ONE fixed order (lane-strided, then
//                     the same tree), so every wave holds the same Z_X, Z_Y; writes terms[b] = -(|x_b - y_b|^2 + gamma (unif(X) +
//                     unif(Y)) / 2) for every b < B (the existing single-wave reduction with 1 / B then yields the "bpr" slot; a void
//                     sample carries the constant alone), the two coefficients 2 gamma / Z_side where the next launch reads them
//                     (no host synchronisation inside a step), and adds the alignment gradient of both rows through the projection.
//   k_directau_grad   one wave per (side, 32 owned rows, part of the sweep, 128-column block).  Recomputes the tile with the same
//                     operands in the same k order -- s and hence k have the bits the normaliser summed -- forms W = coef k in the
//                     accumulator registers, sums t_b = sum_c W[b,c] s_{b,c} there, and register i IS the A operand of the second
//                     MFMA (k_inbatch_grad's scheme); the projection inv_b (sum_c W x_c - t_b x_b) is applied to the partial rows in
//                     the epilogue (it is linear) and they go to G64 with fixed_add: the split of the sweep has no ordering effect.
// k in [e^-8, 1]: no maximum is subtracted and nothing underflows.  Operands up to D = 64 (IB_REG_D) live in registers with the
// next tile prefetched, above that they are streamed: the sweep of lgcn_inbatch_tile.h, shared with lgcn_inbatch.hip.
#include "lgcn_batch_rows.h"        // RowsGeo and the sample prologue, DISPATCH_ROWS
#include "lgcn_inbatch_tile.h"      // the score tile and the pieces of the sweep round it

#ifndef LGCN_DIRECTAU_NORM_FULL
#define LGCN_DIRECTAU_NORM_FULL 0     /* 1 (A/B only, profiles/directau/README.md): the normaliser sweeps every tile and counts every pair
                                         twice -- (b, c) and (c, b) have the same bits -- and the merge halves the sums (exact) */
#endif

// k_{b,c} from the score and the two squared norms: ONE expression for the normaliser and the gradient (an explicit fmaf: the
// same bits whatever the compiler contracts around it; q_b + q_c commutes, so k is symmetric bit for bit)
__device__ __forceinline__ float au_k(float qb, float qc, float s) { return expf(-2.f * fmaf(-2.f, s, qb + qc)); }

template <int D, typename TI, bool WTS>
__global__ void __launch_bounds__(256) k_directau_rows(DirectAuArgs da) {
    const MultiNegArgs &a = da.m;
    ROWS_ZERO_STALE_BITMAP(a);
    ROWS_GEOMETRY(D);
    const int Bp = lgcn_inbatch_rows(a.B);
    if (b >= Bp) return;                        // whole lane groups leave together
    ROWS_LOAD_IDS(a, ROWS_PAIR_FIRST, false, b < a.B);      // lane 0 holds the user, lane 1 the positive; the padding b >= B is bad too
    if (bad) {          // padding, or an out-of-range id: zero rows, masked in every pair by uid = -1
#pragma unroll
        for (int j = 0; j < CPT; j++) { da.X[(int64_t)b * D + j * LPT + l] = 0.f; da.Y[(int64_t)b * D + j * LPT + l] = 0.f; }
        if (l == 0) {
            da.uid[b] = -1; da.pid[b] = -1; da.al[b] = 0.f;
            da.invx[b] = 0.f; da.invy[b] = 0.f; da.qx[b] = 0.f; da.qy[b] = 0.f;
            if (b < a.B) { atomicExch(a.err, 1); a.terms[a.terms_stride + b] = 0.f; }
        }
        return;
    }
    const int32_t iu = __shfl(id, 0, LPT), ip = __shfl(id, 1, LPT);
    const int64_t ru = (int64_t)iu, rp = (int64_t)ip + a.n_users;
    const bool ego = a.reg_ego != 0;
    const float lam = ego ? 0.f : a.lam;
    float u[CPT], p[CPT];
    float ru2 = 0.f, rp2 = 0.f;
    ROWS_PAIR((void)0)
    const float rr = group_sum<LPT>(ru2 + rp2);
    // |e| = sqrtf of the fp32 sum of squares, inv = 1 / |e| by an IEEE division (0 for a row of norm 0): k_inbatch_rows' COS form.
    // The reg term and lam e stay on the rows themselves
    float nu = 0.f, np = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; j++) { nu += u[j] * u[j]; np += p[j] * p[j]; }
    nu = group_sum<LPT>(nu); np = group_sum<LPT>(np);
    const float inv_u = rows_inv_norm(nu), inv_p = rows_inv_norm(np);
    float qx = 0.f, qy = 0.f, al = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const float xh = u[j] * inv_u, yh = p[j] * inv_p, dd = xh - yh;
        qx += xh * xh; qy += yh * yh; al += dd * dd;
        da.X[(int64_t)b * D + j * LPT + l] = xh;
        da.Y[(int64_t)b * D + j * LPT + l] = yh;
        if (lam != 0.f) {
            fixed_add(a.G64 + ru * D + j * LPT + l, lam * u[j]);
            fixed_add(a.G64 + rp * D + j * LPT + l, lam * p[j]);
        }
    }
    qx = group_sum<LPT>(qx); qy = group_sum<LPT>(qy); al = group_sum<LPT>(al);
    if (l == 0) {
        da.uid[b] = iu; da.pid[b] = ip; da.al[b] = al;
        da.invx[b] = inv_u; da.invy[b] = inv_p; da.qx[b] = qx; da.qy[b] = qy;
        a.terms[a.terms_stride + b] = rr;
    }
    if (l < 2) {                                // the 2 rows of the sample: one lane each
        const int64_t myrow = l == 0 ? ru : rp;
        ROWS_FLAG(a, myrow, 1);
    }
}

template <int D>
__global__ void __launch_bounds__(64) k_directau_norm(DirectAuArgs da) {
    const int l = threadIdx.x, j = l & 31, h = l >> 5;
    const int Bp = lgcn_inbatch_rows(da.m.B), nT = Bp / 32, NP = lgcn_inbatch_parts(da.m.B);
    const int bx = blockIdx.x, by = blockIdx.y, side = blockIdx.z;
    const float *T = side == 0 ? da.X : da.Y, *q = side == 0 ? da.qx : da.qy;
    const int b = bx * 32 + j;                  // this lane's owned index (a column of the tile)
    IB_PART_BOUNDS(by, nT);
    const int ts = LGCN_DIRECTAU_NORM_FULL ? t0 : (t0 > bx ? t0 : bx);      // pairs are counted once, as (b, c > b): tiles below the owner's hold none
    const int32_t sb = da.uid[b];               // >= 0: the sample is sound
    const float qb = q[b];
    const float *brow = T + (int64_t)b * D + h * (D / 2);
    float z = 0.f;
    IB_SWEEP_BEGIN(D, own, T, ts, ts < t1)
#pragma unroll 1
    for (int t = ts; t < t1; t++) {
        int32_t ids[16];
        float qc[16];
#pragma unroll
        for (int reg = 0; reg < 16; reg++) { const int c = t * 32 + mfma32_row(reg, h); ids[reg] = da.uid[c]; qc[reg] = q[c]; }
        f32x16 acc;
        IB_SWEEP_SCORES(D, acc, own, T, t);
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {    // register order: part of the result
            const int c = t * 32 + mfma32_row(reg, h);
            const bool ok = sb >= 0 && ids[reg] >= 0 && (LGCN_DIRECTAU_NORM_FULL ? c != b : c > b);
            const float k = au_k(qb, qc[reg], acc[reg]);
            z += ok ? k : 0.f;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off);
    if (l == 0) da.part[((int64_t)side * NP + by) * nT + bx] = z;
}

template <int D>
__global__ void __launch_bounds__(256) k_directau_merge(DirectAuArgs da) {
    const MultiNegArgs &a = da.m;
    ROWS_GEOMETRY(D);
    // Z_X, Z_Y: every wave of the launch adds the same partials in the same order (lane-strided, then the tree)
    const int n = (lgcn_inbatch_rows(a.B) / 32) * lgcn_inbatch_parts(a.B);
    float zx = 0.f, zy = 0.f;
    for (int i = threadIdx.x & 63; i < n; i += 64) { zx += da.part[i]; zy += da.part[n + i]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { zx += __shfl_xor(zx, off); zy += __shfl_xor(zy, off); }
    if (LGCN_DIRECTAU_NORM_FULL) { zx *= 0.5f; zy *= 0.5f; }
    // fewer than two sound samples: Z = 0 exactly (every k >= exp(-8) > 0), no log is taken and no coefficient leaves
    const float npairs = (float)(0.5 * (double)a.B * (double)(a.B - 1));
    const float ux = zx > 0.f ? logf(zx / npairs) : 0.f, uy = zy > 0.f ? logf(zy / npairs) : 0.f;
    const float cst = da.gamma * (ux + uy) * 0.5f;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        da.scal[0] = zx > 0.f ? 2.f * da.gamma / zx : 0.f;
        da.scal[1] = zy > 0.f ? 2.f * da.gamma / zy : 0.f;
    }
    if (b >= a.B) return;
    const int32_t iu = da.uid[b], ip = da.pid[b];
    if (l == 0) a.terms[b] = -(da.al[b] + cst);         // (al = 0 for a void sample: it carries the batch's constant alone)
    if (iu < 0) return;
    // the alignment gradient 2/B (x - y) of x and its mirror of y, through the normalisation: inv (g - (g.own^) own^)
    float xs[CPT], ys[CPT], sxy = 0.f;
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const int64_t o = (int64_t)b * D + j * LPT + l;
        xs[j] = da.X[o]; ys[j] = da.Y[o];
        sxy += xs[j] * ys[j];
    }
    sxy = group_sum<LPT>(sxy);
    const float w = 2.f / (float)a.B, tx = da.qx[b] - sxy, ty = da.qy[b] - sxy, inv_u = da.invx[b], inv_p = da.invy[b];
    const int64_t ru = (int64_t)iu, rp = (int64_t)ip + a.n_users;
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const float dd = xs[j] - ys[j];
        fixed_add(a.G64 + ru * D + j * LPT + l, inv_u * (w * (dd - tx * xs[j])));
        fixed_add(a.G64 + rp * D + j * LPT + l, inv_p * (w * (-dd - ty * ys[j])));
    }
}

template <int D>
__global__ void __launch_bounds__(64) k_directau_grad(DirectAuArgs da) {
    constexpr int CB = ib_grad_blocks(D);        // 32-column blocks of the output this workgroup accumulates
    const int l = threadIdx.x, j = l & 31, h = l >> 5;
    const int Bp = lgcn_inbatch_rows(da.m.B), nT = Bp / 32;
    const int side = blockIdx.z & 1, col0 = (blockIdx.z >> 1) * 128;
    const int bx = blockIdx.x, by = blockIdx.y; // the owned tile, the part of the sweep
    const float coef = da.scal[side];           // 2 gamma / Z_side; 0: gamma = 0 or no pair -- nothing to add (uniform)
    if (coef == 0.f) return;
    const float *T = side == 0 ? da.X : da.Y, *q = side == 0 ? da.qx : da.qy;
    const int o = bx * 32 + j;                  // this lane's owned index (a column of the score tile)
    IB_PART_BOUNDS(by, nT);
    const int32_t so = da.uid[o];
    const float qo = q[o];
    float tproj = 0.f;                          // sum_x W[x][o] s[x][o] over this lane's 16 rows of every tile
    const float *brow = T + (int64_t)o * D + h * (D / 2);
    IB_GRAD_ZERO();
    IB_SWEEP_BEGIN(D, ownr, T, t0, true)
#pragma unroll 1
    for (int t = t0; t < t1; t++) {
        // the rows' ids and squared norms, the B operands of the second product and, in the register form, the next tile's rows are
        // in flight while the scores are multiplied
        int32_t ids[16];
        float qc[16], ob[16][CB];
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int x = t * 32 + mfma32_row(reg, h);          // the other index (a row of the tile)
            ids[reg] = da.uid[x]; qc[reg] = q[x];
            IB_GRAD_PREFETCH(D, T, x);
        }
        f32x16 w;
        IB_SWEEP_SCORES(D, w, ownr, T, t);
#pragma unroll
        for (int reg = 0; reg < 16; reg++) {
            const int x = t * 32 + mfma32_row(reg, h);
            const bool ok = so >= 0 && ids[reg] >= 0 && x != o;
            const float s = w[reg];
            w[reg] = ok ? coef * au_k(qo, qc[reg], s) : 0.f;
            tproj += w[reg] * s;
        }
        IB_GRAD_PRODUCT(D, T, t);                // g[owned][col] += sum_x W[x][owned] T[x][col]
    }
    IB_GRAD_TPROJ_COMBINE();
    // rows of g: owned index bx * 32 + mfma32_row(reg, h); columns col0 + cb * 32 + j
    const int32_t *rid = side == 0 ? da.uid : da.pid;
    const float *inv = side == 0 ? da.invx : da.invy;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) {
        const int ob = bx * 32 + mfma32_row(reg, h);
        const float t_row = IB_GRAD_TPROJ_ROW(reg);       // (every lane takes part: before the skip)
        const int32_t us = rid[ob];
        if (us < 0) continue;                   // void or padding: no row to add to (its W is zero)
        const int64_t row = side == 0 ? (int64_t)us : (int64_t)us + da.m.n_users;
        const float inv_o = inv[ob];
        IB_GRAD_ADD_PROJECTED(D, da.m.G64, T, inv_o);
    }
}

template <int D>
static void launch_d(const DirectAuArgs &a, int act_dtype, bool wts, hipStream_t st) {
    constexpr int SPB = RowsGeo<D>::SPB;
    const int Bp = lgcn_inbatch_rows(a.m.B), NP = lgcn_inbatch_parts(a.m.B);
    const dim3 rows_grid((unsigned)((Bp + SPB - 1) / SPB)), merge_grid((unsigned)((a.m.B + SPB - 1) / SPB));
    DISPATCH_ROWS(act_dtype, wts, hipLaunchKernelGGL((k_directau_rows<D, TI, WTS>), rows_grid, dim3(256), 0, st, a));
    hipLaunchKernelGGL((k_directau_norm<D>), dim3((unsigned)(Bp / 32), (unsigned)NP, 2u), dim3(64), 0, st, a);
    hipLaunchKernelGGL((k_directau_merge<D>), merge_grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL((k_directau_grad<D>), dim3((unsigned)(Bp / 32), (unsigned)NP, 2u * (D > 128 ? D / 128 : 1)), dim3(64), 0, st, a);
}

int lgcn_directau_launch(const DirectAuArgs &a, int d, int act_dtype, bool wts, hipStream_t st) {
    if (a.m.B <= 0 || a.m.loss != LGCN_LOSS_DIRECTAU || !(a.gamma >= 0.f) || !isfinite(a.gamma) ||
        (act_dtype != LGCN_F32 && act_dtype != LGCN_BF16) || !a.X || !a.Y || !a.invx || !a.invy || !a.qx || !a.qy || !a.al ||
        !a.uid || !a.pid || !a.part || !a.scal || a.cap % 32 != 0 || a.m.B > a.cap || !a.m.users || !a.m.pos || !a.m.G64 ||
        !a.m.terms || a.m.terms_stride < a.m.B) {
        lgcn_set_error("alignment-and-uniformity rows: bad launch arguments (0 < B <= the workspace's rows, loss directau with a finite "
                       "gamma >= 0, fp32 / bf16 tables, a workspace of a multiple of 32 rows)");
        return 3;
    }
    DISPATCH_D(d, (launch_d<D>(a, act_dtype, wts, st)));
    return 0;
}

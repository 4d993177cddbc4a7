// lgcn_multineg.hip -- the batch-row launch of the fused LightGCN step for samples with SEVERAL negatives per positive
// (--neg_ratio R; lgcn_train_step_multi / lgcn_train_epoch_multi), gfx950 (wave64).
//
// A sample is (u, p, n_1..n_R).  With e the rows of the model's output table (layer mean, or the weighted sum):
//   x_r  = e_u.e_p - e_u.e_{n_r}
//   bpr  = -1/(B R) sum_b sum_r logsigmoid(x_{b,r})
//   reg  = 0.5/B sum_b ( |e_u|^2 + |e_p|^2 + 1/R sum_r |e_{n_r}|^2 )      (reg_ego: on the tables' own rows E0[.])
//   gb_r = -sigmoid(-x_r) / (B R),  lam = decay / B
//   g_u = sum_r gb_r (e_p - e_{n_r}) + lam e_u ;  g_p = (sum_r gb_r) e_u + lam e_p ;  g_{n_r} = -gb_r e_u + lam/R e_{n_r}
// which is term for term the loss of the three-slot step on the flattened batch of B R triplets (u, p, n_r) -- but the user
// row and the positive row are read once and added to G64 once: 2 + R slot rows and 2 + R fixed-point row adds per sample
// instead of 3 R.
//
// k_multineg_dense (the dense-last form: every layer X_1..X_K exists as a table): one lane group of min(D, 64) lanes per
// sample, lane = column (mod 64), 256 / min(D, 64) samples per workgroup -- the geometry of k_triplet_dense, so every load
// and every 64-bit atomic wave-instruction covers min(D, 64) contiguous elements.  The negatives are STREAMED: the row of
// negative r + 1 is in flight while negative r is scored, its gradient row goes out as soon as its score is known, and only
// sum_r gb_r and sum_r gb_r e_{n_r} stay in registers, so neither the register count nor anything else grows with R (no LDS).
// Lanes 0..R-1 of the group hold the negatives' ids (R <= 16 <= the smallest group), lanes R and R + 1 the user's and the
// positive's row: the row flags and the reg_ego slot counts of all 2 + R rows are ONE atomic instruction each.
// Everything downstream consumes what the three-slot kernels write: G64 (2^50 fixed point), the row bitmap, cnt, terms, err.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lgcn_hip.h"
#include "lgcn_internal.h"

#define MN_FIXED_SCALE 1125899906842624.0     /* 2^50, the scale of G64 everywhere in this library */

typedef __bf16 mn_bf16_t;

template <typename TI> __device__ __forceinline__ float mn_elem(const void *tab, int64_t o);
template <> __device__ __forceinline__ float mn_elem<float>(const void *tab, int64_t o) { return ((const float *)tab)[o]; }
template <> __device__ __forceinline__ float mn_elem<mn_bf16_t>(const void *tab, int64_t o) { return (float)((const mn_bf16_t *)tab)[o]; }

// the arithmetic of the three-slot kernels, restated so that their file is not touched
__device__ __forceinline__ float mn_logsigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float mn_sigmoid_neg(float x) {
    const float z = expf(-fabsf(x));
    return x < 0.f ? 1.f / (1.f + z) : z / (1.f + z);
}

// e[j] = the output-table row `row` at columns j * LPT + l (mean over the K + 1 layers, or the weighted sum); e0[j] = E0's
template <int D, typename TI, bool WTS>
__device__ __forceinline__ void mn_slot_row(const MultiNegArgs &a, int64_t row, int l, float *e, float *e0) {
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT;
    const float div = (float)(a.K + 1);
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const int64_t o = row * D + j * LPT + l;
        float s = a.X0[o];
        e0[j] = s;
        if constexpr (WTS) {
            s *= a.w[0];
            for (int k = 1; k <= a.K; k++) s += a.w[k] * mn_elem<TI>(a.Xl[k], o);
            e[j] = s;
        } else {
            for (int k = 1; k <= a.K; k++) s += mn_elem<TI>(a.Xl[k], o);
            e[j] = s / div;
        }
    }
}

template <int LPT> __device__ __forceinline__ float mn_group_sum(float v) {
#pragma unroll
    for (int off = 1; off < LPT; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

template <int D, typename TI, bool WTS>
__global__ void __launch_bounds__(256) k_multineg_dense(MultiNegArgs a) {
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT, SPB = 256 / LPT;     // lanes per sample, samples per workgroup
    // last step's row bitmap is dead: zero it here with plain stores (the two bitmaps alternate per step)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.bitmap_words; i += (int64_t)gridDim.x * 256)
        a.stale_bitmap[i] = 0u;
    const int b = blockIdx.x * SPB + threadIdx.x / LPT, l = threadIdx.x % LPT;
    if (b >= a.B) return;                       // whole lane groups leave together
    const int R = a.R;
    // every id is checked before anything is addressed with it: lane r < R holds negative r, lanes R / R + 1 the user / positive
    int32_t id = 0;
    bool idbad = false;
    if (l < R) { id = a.negs[(int64_t)l * a.neg_stride + b]; idbad = id < 0 || (int64_t)id + a.n_users >= a.N; }
    else if (l == R) { id = a.users[b]; idbad = id < 0 || id >= a.n_users; }
    else if (l == R + 1) { id = a.pos[b]; idbad = id < 0 || (int64_t)id + a.n_users >= a.N; }
    const int64_t myrow = l == R ? (int64_t)id : (int64_t)id + a.n_users;      // (meaningful on lanes 0 .. R + 1)
    constexpr unsigned long long GROUP = LPT == 64 ? ~0ull : ((1ull << (LPT & 63)) - 1ull);
    const bool bad = (__ballot(idbad) & (GROUP << ((threadIdx.x & 63) / LPT * LPT))) != 0ull;
    if (bad) {                                  // an out-of-range id voids the whole sample: err flag, zero terms, no gradient
        if (l == 0) { atomicExch(a.err, 1); a.terms[b] = 0.f; a.terms[a.terms_stride + b] = 0.f; }
        return;
    }
    const int64_t ru = (int64_t)__shfl(id, R, LPT), rp = (int64_t)__shfl(id, R + 1, LPT) + a.n_users;
    const bool ego = a.reg_ego != 0;
    const float lam = ego ? 0.f : a.lam, lam_n = ego ? 0.f : a.lam_n;
    float u[CPT], p[CPT], t0[CPT], acc[CPT];    // acc = sum_r gb_r e_{n_r}
    float ps = 0.f, ru2 = 0.f, rp2 = 0.f;
    mn_slot_row<D, TI, WTS>(a, ru, l, u, t0);
#pragma unroll
    for (int j = 0; j < CPT; j++) { const float v = ego ? t0[j] : u[j]; ru2 += v * v; }
    mn_slot_row<D, TI, WTS>(a, rp, l, p, t0);
#pragma unroll
    for (int j = 0; j < CPT; j++) { const float v = ego ? t0[j] : p[j]; ps += u[j] * p[j]; rp2 += v * v; acc[j] = 0.f; }
    ps = mn_group_sum<LPT>(ps);
    float sgb = 0.f, sl = 0.f, srn = 0.f;       // sum_r gb_r, sum_r logsigmoid(x_r), sum_r |n_r|^2 (this lane's columns)
    float n[CPT], n0[CPT], nn[CPT], nn0[CPT];
    int64_t rn = (int64_t)__shfl(id, 0, LPT) + a.n_users;
    mn_slot_row<D, TI, WTS>(a, rn, l, n, n0);
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const int64_t rnext = (int64_t)__shfl(id, r + 1 < R ? r + 1 : r, LPT) + a.n_users;
        if (r + 1 < R) mn_slot_row<D, TI, WTS>(a, rnext, l, nn, nn0);      // the next negative's rows fly while this one is scored
        float ns = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; j++) { const float v = ego ? n0[j] : n[j]; ns += u[j] * n[j]; srn += v * v; }
        ns = mn_group_sum<LPT>(ns);
        const float x = ps - ns;
        const float gb = -a.inv_BR * mn_sigmoid_neg(x);
        sl += mn_logsigmoid(x);
        sgb += gb;
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            acc[j] += gb * n[j];
            const float g = (-gb) * u[j] + lam_n * n[j];
            atomicAdd((unsigned long long *)(a.G64 + rn * D + j * LPT + l), (unsigned long long)__double2ll_rn((double)g * MN_FIXED_SCALE));
        }
        if (r + 1 < R) {
#pragma unroll
            for (int j = 0; j < CPT; j++) { n[j] = nn[j]; n0[j] = nn0[j]; }
            rn = rnext;
        }
    }
    const float rr = mn_group_sum<LPT>(ru2 + rp2 + srn * a.inv_R);
    if (l == 0) { a.terms[b] = sl * a.inv_R; a.terms[a.terms_stride + b] = rr; }
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const float gu = (sgb * p[j] - acc[j]) + lam * u[j];
        const float gp = sgb * u[j] + lam * p[j];
        atomicAdd((unsigned long long *)(a.G64 + ru * D + j * LPT + l), (unsigned long long)__double2ll_rn((double)gu * MN_FIXED_SCALE));
        atomicAdd((unsigned long long *)(a.G64 + rp * D + j * LPT + l), (unsigned long long)__double2ll_rn((double)gp * MN_FIXED_SCALE));
    }
    if (l < R + 2) {                            // the 2 + R rows of the sample: one lane each
        atomicOr(a.bitmap + (myrow >> 5), 1u << (myrow & 31));
        if (a.cnt) atomicAdd(a.cnt + myrow, l < R ? 1 : R);     // a negative slot weighs 1/R of a user / positive slot (epilogue: decay / (B R))
    }
}

template <int D>
static void mn_launch_d(const MultiNegArgs &a, int act_dtype, bool wts, hipStream_t st) {
    constexpr int SPB = 256 / (D < 64 ? D : 64);
    const dim3 grid((unsigned)((a.B + SPB - 1) / SPB)), block(256);
    if (act_dtype == LGCN_F32) {
        if (wts) hipLaunchKernelGGL((k_multineg_dense<D, float, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_multineg_dense<D, float, false>), grid, block, 0, st, a);
    } else {
        if (wts) hipLaunchKernelGGL((k_multineg_dense<D, mn_bf16_t, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_multineg_dense<D, mn_bf16_t, false>), grid, block, 0, st, a);
    }
}

int lgcn_multineg_launch(const MultiNegArgs &a, int d, int act_dtype, bool wts, hipStream_t st) {
    if (a.B <= 0 || a.R < 1 || a.R > LGCN_MAX_NEG_RATIO || a.neg_stride < a.B || (act_dtype != LGCN_F32 && act_dtype != LGCN_BF16)) {
        lgcn_set_error("multi-negative batch rows: bad launch arguments (negative ratio 1..16, neg_stride >= B, fp32 / bf16 tables)");
        return 3;
    }
    switch (d) {
    case 32: mn_launch_d<32>(a, act_dtype, wts, st); break;
    case 64: mn_launch_d<64>(a, act_dtype, wts, st); break;
    case 128: mn_launch_d<128>(a, act_dtype, wts, st); break;
    case 256: mn_launch_d<256>(a, act_dtype, wts, st); break;
    default: lgcn_set_error("multi-negative batch rows: embedding dim must be 32, 64, 128 or 256"); return 3;
    }
    return 0;
}

// lgcn_softmax.hip -- the batch-row launch of the multi-negative step under the sampled-softmax loss (--loss softmax;
// lgcn_ctx_set_loss), gfx950 (wave64).
//
// A sample is (u, p, n_1..n_R).  With e the rows of the model's output table and the temperature tau > 0:
//   x_r  = e_u.e_p - e_u.e_{n_r},   z_r = -x_r / tau
//   l    = log(1 + sum_r exp(z_r))                          sm = 1/B sum_b l_b       (one term per sample)
//   q_r  = exp(z_r) / (1 + sum_j exp(z_j)),   gb_r = -q_r / (tau B)
//   g_u = sum_r gb_r (e_p - e_{n_r}) + lam e_u ;  g_p = (sum_r gb_r) e_u + lam e_p ;  g_{n_r} = -gb_r e_u + lam/R e_{n_r}
// reg, lam, the reg_ego slot counts and everything downstream are those of lgcn_multineg.hip; terms[b] = -l, so the
// single-wave reduction with 1/B yields sm.
//
// k_multineg_softmax keeps the geometry of k_multineg_dense (one lane group of min(D, 64) lanes per sample, lane = column
// mod 64, ids on lanes 0..R+1, one ballot voids a sample, one atomicOr / atomicAdd for the 2 + R row flags / counts), but
// q_r needs ALL R scores of the sample before any gradient row can leave, so it runs in three phases:
//   1. score      the negatives are streamed as there (the next row in flight while this one is scored); z_r stays in lane r
//                 of the group (R <= 16 <= the smallest group), the reg squares are summed.  No gradient leaves.
//   2. normalise  m = max(0, max_r z_r) and the sum over lanes < R with shuffles;  with the one term that equals exp(0) taken
//                 out of the sum (the positive's when m = 0, the first maximal negative's otherwise)
//                     l = m + log1p(Zm1),  q_r = exp(z_r - m) / (1 + Zm1)
//                 so no exp of a positive argument occurs and l keeps its relative accuracy where it is tiny.
//   3. emit       the negatives' rows are streamed a SECOND time (they were read by this workgroup a moment ago): g_{n_r} and
//                 acc = sum_r gb_r e_{n_r} need the row and gb_r together.  2 + R fixed-point row adds per sample, as there.
// Registers do not grow with R (#pragma unroll 1 over r), no LDS.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lgcn_hip.h"
#include "lgcn_internal.h"

#define SX_FIXED_SCALE 1125899906842624.0     /* 2^50, the scale of G64 everywhere in this library */

typedef __bf16 sx_bf16_t;

template <typename TI> __device__ __forceinline__ float sx_elem(const void *tab, int64_t o);
template <> __device__ __forceinline__ float sx_elem<float>(const void *tab, int64_t o) { return ((const float *)tab)[o]; }
template <> __device__ __forceinline__ float sx_elem<sx_bf16_t>(const void *tab, int64_t o) { return (float)((const sx_bf16_t *)tab)[o]; }

// e[j] = the output-table row `row` at columns j * LPT + l (mean over the K + 1 layers, or the weighted sum); e0[j] = E0's
// (the arithmetic of mn_slot_row, restated so that its file is not touched)
template <int D, typename TI, bool WTS>
__device__ __forceinline__ void sx_slot_row(const MultiNegArgs &a, int64_t row, int l, float *e, float *e0) {
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT;
    const float div = (float)(a.K + 1);
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const int64_t o = row * D + j * LPT + l;
        float s = a.X0[o];
        e0[j] = s;
        if constexpr (WTS) {
            s *= a.w[0];
            for (int k = 1; k <= a.K; k++) s += a.w[k] * sx_elem<TI>(a.Xl[k], o);
            e[j] = s;
        } else {
            for (int k = 1; k <= a.K; k++) s += sx_elem<TI>(a.Xl[k], o);
            e[j] = s / div;
        }
    }
}

template <int LPT> __device__ __forceinline__ float sx_group_sum(float v) {
#pragma unroll
    for (int off = 1; off < LPT; off <<= 1) v += __shfl_xor(v, off);
    return v;
}
template <int LPT> __device__ __forceinline__ float sx_group_max(float v) {
#pragma unroll
    for (int off = 1; off < LPT; off <<= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

template <int D, typename TI, bool WTS>
__global__ void __launch_bounds__(256) k_multineg_softmax(SoftmaxArgs sa) {
    const MultiNegArgs &a = sa.m;
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
    const int gshift = (threadIdx.x & 63) / LPT * LPT;                          // this group's first lane in the wave
    const bool bad = (__ballot(idbad) & (GROUP << gshift)) != 0ull;
    if (bad) {                                  // an out-of-range id voids the whole sample: err flag, zero terms, no gradient
        if (l == 0) { atomicExch(a.err, 1); a.terms[b] = 0.f; a.terms[a.terms_stride + b] = 0.f; }
        return;
    }
    const int64_t ru = (int64_t)__shfl(id, R, LPT), rp = (int64_t)__shfl(id, R + 1, LPT) + a.n_users;
    const bool ego = a.reg_ego != 0;
    const float lam = ego ? 0.f : a.lam, lam_n = ego ? 0.f : a.lam_n;
    float u[CPT], p[CPT], t0[CPT], acc[CPT];    // acc = sum_r gb_r e_{n_r}
    float ps = 0.f, ru2 = 0.f, rp2 = 0.f;
    sx_slot_row<D, TI, WTS>(a, ru, l, u, t0);
#pragma unroll
    for (int j = 0; j < CPT; j++) { const float v = ego ? t0[j] : u[j]; ru2 += v * v; }
    sx_slot_row<D, TI, WTS>(a, rp, l, p, t0);
#pragma unroll
    for (int j = 0; j < CPT; j++) { const float v = ego ? t0[j] : p[j]; ps += u[j] * p[j]; rp2 += v * v; acc[j] = 0.f; }
    ps = sx_group_sum<LPT>(ps);
    float n[CPT], n0[CPT], nn[CPT], nn0[CPT];
    // ---- phase 1: score.  z_r into lane r; lanes >= R keep 0, the positive's own exponent (LPT >= 32 > R: there is one)
    float z = 0.f, srn = 0.f;                   // srn = sum_r |n_r|^2 (this lane's columns)
    int64_t rn = (int64_t)__shfl(id, 0, LPT) + a.n_users;
    sx_slot_row<D, TI, WTS>(a, rn, l, n, n0);
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const int64_t rnext = (int64_t)__shfl(id, r + 1 < R ? r + 1 : r, LPT) + a.n_users;
        if (r + 1 < R) sx_slot_row<D, TI, WTS>(a, rnext, l, nn, nn0);      // the next negative's rows fly while this one is scored
        float ns = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; j++) { const float v = ego ? n0[j] : n[j]; ns += u[j] * n[j]; srn += v * v; }
        ns = sx_group_sum<LPT>(ns);
        const float zr = -(ps - ns) / sa.tau;
        if (l == r) z = zr;
        if (r + 1 < R) {
#pragma unroll
            for (int j = 0; j < CPT; j++) { n[j] = nn[j]; n0[j] = nn0[j]; }
        }
    }
    // ---- phase 2: normalise.  m = max(0, max_r z_r); every exponent below is <= 0
    const float m = sx_group_max<LPT>(z);
    const bool mine = l < R;
    // the term that is exp(0) = 1 exactly is left out of the sum: the positive's where m = 0, else the first maximal negative's
    const unsigned long long atmax = (__ballot(mine && z == m) >> gshift) & GROUP;
    const int first = m > 0.f ? __ffsll(atmax) - 1 : -1;
    const float ev = mine ? expf(z - m) : 0.f;
    const float zm1 = sx_group_sum<LPT>(l == first ? 0.f : ev) + (m > 0.f ? expf(-m) : 0.f);      // Z - 1
    const float q = ev / (1.f + zm1);           // q_r in lane r (0 on lanes >= R)
    const float lterm = m + log1pf(zm1);
    // ---- phase 3: emit.  the negatives' rows a second time, now with their coefficients
    float sgb = 0.f;
    rn = (int64_t)__shfl(id, 0, LPT) + a.n_users;
    sx_slot_row<D, TI, WTS>(a, rn, l, n, n0);
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const int64_t rnext = (int64_t)__shfl(id, r + 1 < R ? r + 1 : r, LPT) + a.n_users;
        if (r + 1 < R) sx_slot_row<D, TI, WTS>(a, rnext, l, nn, nn0);
        const float gb = -sa.inv_tauB * __shfl(q, r, LPT);
        sgb += gb;
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            acc[j] += gb * n[j];
            const float g = (-gb) * u[j] + lam_n * n[j];
            atomicAdd((unsigned long long *)(a.G64 + rn * D + j * LPT + l), (unsigned long long)__double2ll_rn((double)g * SX_FIXED_SCALE));
        }
        if (r + 1 < R) {
#pragma unroll
            for (int j = 0; j < CPT; j++) n[j] = nn[j];
            rn = rnext;
        }
    }
    const float rr = sx_group_sum<LPT>(ru2 + rp2 + srn * a.inv_R);
    if (l == 0) { a.terms[b] = -lterm; a.terms[a.terms_stride + b] = rr; }
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const float gu = (sgb * p[j] - acc[j]) + lam * u[j];
        const float gp = sgb * u[j] + lam * p[j];
        atomicAdd((unsigned long long *)(a.G64 + ru * D + j * LPT + l), (unsigned long long)__double2ll_rn((double)gu * SX_FIXED_SCALE));
        atomicAdd((unsigned long long *)(a.G64 + rp * D + j * LPT + l), (unsigned long long)__double2ll_rn((double)gp * SX_FIXED_SCALE));
    }
    if (l < R + 2) {                            // the 2 + R rows of the sample: one lane each
        atomicOr(a.bitmap + (myrow >> 5), 1u << (myrow & 31));
        if (a.cnt) atomicAdd(a.cnt + myrow, l < R ? 1 : R);     // a negative slot weighs 1/R of a user / positive slot (epilogue: decay / (B R))
    }
}

template <int D>
static void sx_launch_d(const SoftmaxArgs &a, int act_dtype, bool wts, hipStream_t st) {
    constexpr int SPB = 256 / (D < 64 ? D : 64);
    const dim3 grid((unsigned)((a.m.B + SPB - 1) / SPB)), block(256);
    if (act_dtype == LGCN_F32) {
        if (wts) hipLaunchKernelGGL((k_multineg_softmax<D, float, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_multineg_softmax<D, float, false>), grid, block, 0, st, a);
    } else {
        if (wts) hipLaunchKernelGGL((k_multineg_softmax<D, sx_bf16_t, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_multineg_softmax<D, sx_bf16_t, false>), grid, block, 0, st, a);
    }
}

int lgcn_softmax_launch(const SoftmaxArgs &a, int d, int act_dtype, bool wts, hipStream_t st) {
    if (a.m.B <= 0 || a.m.R < 1 || a.m.R > LGCN_MAX_NEG_RATIO || a.m.neg_stride < a.m.B || !(a.tau > 0.f) ||
        (act_dtype != LGCN_F32 && act_dtype != LGCN_BF16)) {
        lgcn_set_error("sampled-softmax batch rows: bad launch arguments (negative ratio 1..16, neg_stride >= B, temperature > 0, fp32 / bf16 tables)");
        return 3;
    }
    switch (d) {
    case 32: sx_launch_d<32>(a, act_dtype, wts, st); break;
    case 64: sx_launch_d<64>(a, act_dtype, wts, st); break;
    case 128: sx_launch_d<128>(a, act_dtype, wts, st); break;
    case 256: sx_launch_d<256>(a, act_dtype, wts, st); break;
    default: lgcn_set_error("sampled-softmax batch rows: embedding dim must be 32, 64, 128 or 256"); return 3;
    }
    return 0;
}

// lgcn_mf.hip -- matrix factorisation trained with BPR (upstream LightGCN's PureMF, --model mf): BPRLoss.stageOne on a model
// with no graph and no propagation, in two launches for gfx950 (wave64).
//
//   x_b  = <U_b, Nn_b> - <U_b, P_b>          rows of the tables themselves
//   loss = mean_b softplus(x_b) + decay * 1/2 (|U|^2 + |P|^2 + |Nn|^2) / B
//   grad : row u += (s_b (Nn_b - P_b) + decay U_b) / B,  row p += (-s_b U_b + decay P_b) / B,
//          row n += ( s_b U_b + decay Nn_b) / B,          s_b = sigmoid(x_b); repeated ids sum
//   torch.optim.Adam on the DENSE gradient: every row moves every step (rows outside the batch have g = 0: their moments
//   decay and their parameters still follow them).
//
//   k_mf_triplet  one lane group of d/4 lanes per triplet (8 / 4 / 2 / 1 triplets per wave at d = 32 / 64 / 128 / 256): one
//                 16-byte load per row and lane, the two dot products and the squared norms reduced inside the lane group on the
//                 VALU (DPP inside a 16-lane row, v_permlane16_swap / v_permlane32_swap across rows), loss terms into terms[2B],
//                 the three gradient rows into G64 with the 2^50 fixed-point int64 atomics (order-free: bitwise reproducible),
//                 the rows flagged in this step's bitmap.
//   k_mf_adam     a chip-wide stream over all N rows, 16 bytes of P / M / V per lane: a flagged row takes its gradient from G64
//                 and zeroes it, any other row has g = 0; last step's bitmap is zeroed with plain stores (the two bitmaps
//                 alternate per step, as in the LightGCN step); one extra workgroup reduces the loss terms in the fixed order
//                 of the LightGCN step's reduction.
// The Adam arithmetic is that of the LightGCN step's epilogue (lerp, mul / addcmul, sqrt(v) / bc2_sqrt + eps, step_size) on
// 16-byte pieces of a dense stream.
#include <new>

#include "lgcn_device_common.h"

#define MF_ADAM_BLOCKS_MAX 16384              /* workgroups of the Adam stream: one 16-byte piece per lane up to here, grid-stride beyond */

struct lgcn_mf {
    lgcn_mf_config c;
    int64_t N;            // n_users + m_items
    int64_t bm_words;     // words per bitmap; c.bitmap holds two, used alternately
    int64_t step;         // torch Adam state['step']
    int flip;             // which bitmap the next step flags
};

// v + the value `CTRL` names inside the 16-lane row (all lanes of a wave execute this: no lane reads a disabled one)
template <int CTRL> __device__ __forceinline__ float mf_add_dpp(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// Sum over the G = 8 / 16 / 32 / 64 consecutive lanes of a lane group; every lane of the group ends with the SAME bits (each
// stage adds two values that the partner lane adds in the other order).  VALU only.
template <int G> __device__ __forceinline__ float mf_group_sum(float v) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    v = mf_add_dpp<0xB1>(v);                 // quad_perm [1,0,3,2]: lane ^ 1
    v = mf_add_dpp<0x4E>(v);                 // quad_perm [2,3,0,1]: lane ^ 2
    v = mf_add_dpp<0x141>(v);                // row_half_mirror: the other quad of the 8 lanes
    if (G >= 16) v = mf_add_dpp<0x140>(v);   // row_mirror: the other half of the row
    if (G >= 32) { const unsigned a = __float_as_uint(v); const u32x2 r = __builtin_amdgcn_permlane16_swap(a, a, false, false); v = __uint_as_float(r.x) + __uint_as_float(r.y); }
    if (G >= 64) { const unsigned a = __float_as_uint(v); const u32x2 r = __builtin_amdgcn_permlane32_swap(a, a, false, false); v = __uint_as_float(r.x) + __uint_as_float(r.y); }
    return v;
}

struct MfTripletArgs {
    const float *E;                       // [N, D] the table
    const int32_t *users, *pos, *neg;
    int32_t B, n_users, m_items;
    float decay, Bf;                      // Bf = (float)B
    long long *G64; uint32_t *bitmap;
    float *terms;                         // [2B]: softplus(x_b) | |U_b|^2 + |P_b|^2 + |Nn_b|^2
    int32_t *err;
};

template <int D>
__global__ void __launch_bounds__(256) k_mf_triplet(MfTripletArgs a) {
    constexpr int G = D / 4, TPB = 256 / G;                  // lanes per triplet, triplets per workgroup
    const int l = (int)threadIdx.x % G;
    const int64_t b = (int64_t)blockIdx.x * TPB + (int)threadIdx.x / G;
    const bool in = b < a.B;
    int32_t iu = 0, ip = 0, in_ = 0;
    if (in) { iu = a.users[b]; ip = a.pos[b]; in_ = a.neg[b]; }
    // every id is checked before anything is addressed with it; an out-of-range id voids its triplet
    const bool bad = in && (iu < 0 || iu >= a.n_users || ip < 0 || ip >= a.m_items || in_ < 0 || in_ >= a.m_items);
    const bool ok = in && !bad;
    const int64_t ru = (int64_t)iu, rp = (int64_t)ip + a.n_users, rn = (int64_t)in_ + a.n_users;
    f32x4 u = {0.f, 0.f, 0.f, 0.f}, p = u, n = u;
    if (ok) {
        u = *reinterpret_cast<const f32x4 *>(a.E + ru * D + 4 * l);
        p = *reinterpret_cast<const f32x4 *>(a.E + rp * D + 4 * l);
        n = *reinterpret_cast<const f32x4 *>(a.E + rn * D + 4 * l);
    }
    float ps = 0.f, ns = 0.f, rr = 0.f;
#pragma unroll
    for (int i = 0; i < 4; i++) { ps += u[i] * p[i]; ns += u[i] * n[i]; rr += u[i] * u[i] + p[i] * p[i] + n[i] * n[i]; }
    // (lanes of void or absent triplets carry zeros through the reduction: all 64 lanes stay in it)
    ps = mf_group_sum<G>(ps); ns = mf_group_sum<G>(ns); rr = mf_group_sum<G>(rr);
    if (!in) return;
    if (bad) {
        if (l == 0) { atomicExch(a.err, 1); a.terms[b] = 0.f; a.terms[a.B + b] = 0.f; }
        return;
    }
    const float x = ns - ps;
    const float e = expf(-fabsf(x));                          // in (0, 1]: neither form below overflows, |x| of hundreds gives e = 0
    const float s = (x >= 0.f ? 1.f : e) / (1.f + e);         // sigmoid(x)
    if (l == 0) {
        a.terms[b] = fmaxf(x, 0.f) + log1pf(e);               // softplus(x) = -logsigmoid(pos - neg)
        a.terms[a.B + b] = rr;
    }
    long long *gu = a.G64 + ru * D + 4 * l, *gp = a.G64 + rp * D + 4 * l, *gn = a.G64 + rn * D + 4 * l;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const float du = (s * (n[i] - p[i]) + a.decay * u[i]) / a.Bf;
        const float dp = (a.decay * p[i] - s * u[i]) / a.Bf;
        const float dn = (s * u[i] + a.decay * n[i]) / a.Bf;
        fixed_add(gu + i, du);
        fixed_add(gp + i, dp);
        fixed_add(gn + i, dn);
    }
    if (l == 0) {
        atomicOr(a.bitmap + (ru >> 5), 1u << (ru & 31));
        atomicOr(a.bitmap + (rp >> 5), 1u << (rp & 31));
        atomicOr(a.bitmap + (rn >> 5), 1u << (rn & 31));
    }
}

struct MfAdamArgs {
    float *P, *M, *V;
    long long *G64; const uint32_t *bitmap;
    uint32_t *stale_bitmap; int64_t bitmap_words;      // last step's bitmap: dead, zeroed here with plain stores
    int64_t n_vec;                                       // N * D / 4: 16-byte pieces of a table
    const float *terms; float *loss_out; int32_t B; float decay;
    float step_size, bc2_sqrt, w1, beta2, omb2, eps;
};

// the loss of the step from its per-triplet terms, by ONE wave in a fixed order: every lane adds its terms b = lane, lane + 64, ...
// in that order, then an xor-shuffle tree
__device__ __forceinline__ void mf_reduce_loss_wave(const MfAdamArgs &a, int lane) {
    float fl = 0.f, fr = 0.f;
#pragma unroll 8
    for (int b = lane; b < a.B; b += 64) { fl += a.terms[b]; fr += a.terms[a.B + b]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { fl += __shfl_xor(fl, off); fr += __shfl_xor(fr, off); }
    if (lane == 0) {
        const float bpr = fl / (float)a.B;
        const float reg = (0.5f * fr) / (float)a.B;
        a.loss_out[0] = bpr + a.decay * reg; a.loss_out[1] = bpr; a.loss_out[2] = reg;
    }
}

template <int D>
__global__ void __launch_bounds__(256) k_mf_adam(MfAdamArgs a) {
    if (blockIdx.x == gridDim.x - 1) {                 // the extra workgroup: nothing but the loss
        if (threadIdx.x < 64) mf_reduce_loss_wave(a, (int)threadIdx.x);
        return;
    }
    constexpr int G = D / 4;                           // 16-byte pieces per row
    const int64_t stride = (int64_t)(gridDim.x - 1) * 256;
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = t0; i < a.bitmap_words; i += stride) a.stale_bitmap[i] = 0u;
    for (int64_t i = t0; i < a.n_vec; i += stride) {
        const int64_t row = i / G;
        const uint32_t word = a.bitmap[row >> 5];
        f32x4 p = *reinterpret_cast<const f32x4 *>(a.P + 4 * i);
        f32x4 m = *reinterpret_cast<const f32x4 *>(a.M + 4 * i);
        f32x4 v = *reinterpret_cast<const f32x4 *>(a.V + 4 * i);
        f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if ((word >> (row & 31)) & 1u) {               // a row of the batch: its gradient, consumed (G64 is all zero after the step)
            i64x2 *q = reinterpret_cast<i64x2 *>(a.G64 + 4 * i);
            const i64x2 q0 = q[0], q1 = q[1];
            g[0] = (float)((double)q0.x * FIXED_INV); g[1] = (float)((double)q0.y * FIXED_INV);
            g[2] = (float)((double)q1.x * FIXED_INV); g[3] = (float)((double)q1.y * FIXED_INV);
            q[0] = i64x2{0, 0}; q[1] = i64x2{0, 0};
        }
        m = m + a.w1 * (g - m);                         // exp_avg.lerp_(grad, 1-beta1)
        v = v * a.beta2 + (a.omb2 * g) * g;             // mul_(beta2).addcmul_(g,g,1-beta2)
        f32x4 denom;
#pragma unroll
        for (int k = 0; k < 4; k++) denom[k] = sqrtf(v[k]) / a.bc2_sqrt + a.eps;
        p = p - a.step_size * (m / denom);              // addcdiv_(exp_avg, denom, -step_size)
        *reinterpret_cast<f32x4 *>(a.P + 4 * i) = p;
        *reinterpret_cast<f32x4 *>(a.M + 4 * i) = m;
        *reinterpret_cast<f32x4 *>(a.V + 4 * i) = v;
    }
}

extern "C" int lgcn_mf_create(const lgcn_mf_config *cfg, lgcn_mf **out) {
    if (!cfg || !out) { lgcn_set_error("lgcn_mf_create: null argument"); return 3; }
    const lgcn_mf_config &c = *cfg;
    if (c.d != 32 && c.d != 64 && c.d != 128 && c.d != 256) { lgcn_set_error("lgcn_mf_create: d must be 32, 64, 128 or 256"); return 3; }
    if (c.n_users <= 0 || c.m_items <= 0) { lgcn_set_error("lgcn_mf_create: n_users and m_items must be positive"); return 3; }
    if ((int64_t)c.n_users + (int64_t)c.m_items >= ((int64_t)1 << 31)) { lgcn_set_error("lgcn_mf_create: n_users + m_items must stay below 2^31"); return 3; }
    if (c.max_batch < 1) { lgcn_set_error("lgcn_mf_create: max_batch must be at least 1"); return 3; }
    if (!c.E0 || !c.adam_m || !c.adam_v || !c.G64 || !c.bitmap || !c.terms || !c.err) { lgcn_set_error("lgcn_mf_create: null buffer"); return 3; }
    lgcn_mf *x = new (std::nothrow) lgcn_mf();
    if (!x) { lgcn_set_error("lgcn_mf_create: out of host memory"); return 4; }
    x->c = c; x->N = (int64_t)c.n_users + c.m_items; x->bm_words = (x->N + 31) / 32; x->step = 0; x->flip = 0;
    *out = x;
    return 0;
}

extern "C" void lgcn_mf_destroy(lgcn_mf *mf) { delete mf; }
extern "C" int64_t lgcn_mf_get_step(const lgcn_mf *mf) { return mf ? mf->step : -1; }
extern "C" void lgcn_mf_set_step(lgcn_mf *mf, int64_t step) { if (mf) mf->step = step; }
extern "C" void lgcn_mf_set_lr(lgcn_mf *mf, double lr) { if (mf) mf->c.lr = lr; }

static int mf_check_batch(const lgcn_mf *x, const void *u, const void *p, const void *n, const void *loss_out, int32_t B, const char *who) {
    char buf[160];
    if (!x || !u || !p || !n || !loss_out) { snprintf(buf, sizeof buf, "%s: null argument", who); lgcn_set_error(buf); return 3; }
    if (B < 1 || B > x->c.max_batch) { snprintf(buf, sizeof buf, "%s: batch size out of range (1 <= B <= max_batch)", who); lgcn_set_error(buf); return 3; }
    return 0;
}

static int mf_step(lgcn_mf *x, const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B, float *loss_out, hipStream_t st) {
    const lgcn_mf_config &c = x->c;
    uint32_t *bm = c.bitmap + x->flip * x->bm_words, *stale = c.bitmap + (x->flip ^ 1) * x->bm_words;
    MfTripletArgs t{};
    t.E = c.E0; t.users = users; t.pos = pos; t.neg = neg; t.B = B; t.n_users = c.n_users; t.m_items = c.m_items;
    t.decay = c.decay; t.Bf = (float)B; t.G64 = (long long *)c.G64; t.bitmap = bm; t.terms = c.terms; t.err = c.err;
    x->step += 1;
    const double bc1 = 1.0 - pow(c.beta1, (double)x->step), bc2 = 1.0 - pow(c.beta2, (double)x->step);
    MfAdamArgs a{};
    a.P = c.E0; a.M = c.adam_m; a.V = c.adam_v; a.G64 = (long long *)c.G64; a.bitmap = bm; a.stale_bitmap = stale; a.bitmap_words = x->bm_words;
    a.n_vec = x->N * (c.d / 4); a.terms = c.terms; a.loss_out = loss_out; a.B = B; a.decay = c.decay;
    a.step_size = (float)(c.lr / bc1); a.bc2_sqrt = (float)sqrt(bc2);
    a.w1 = (float)(1.0 - c.beta1); a.beta2 = (float)c.beta2; a.omb2 = (float)(1.0 - c.beta2); a.eps = (float)c.eps;
    int64_t blocks = (a.n_vec + 255) / 256;
    if (blocks > MF_ADAM_BLOCKS_MAX) blocks = MF_ADAM_BLOCKS_MAX;
    DISPATCH_D(c.d, {
        constexpr int TPB = 256 / (D / 4);
        hipLaunchKernelGGL((k_mf_triplet<D>), dim3((unsigned)(((int64_t)B + TPB - 1) / TPB)), dim3(256), 0, st, t);
        hipLaunchKernelGGL((k_mf_adam<D>), dim3((unsigned)blocks + 1), dim3(256), 0, st, a);
    });
    x->flip ^= 1;                  // the next step flags rows in the other bitmap (this launch has just zeroed it)
    HIP_OK(hipGetLastError());
    return 0;
}

extern "C" int lgcn_mf_train_step(lgcn_mf *mf, const int32_t *users, const int32_t *pos, const int32_t *neg, int32_t B,
                                  float *loss_out, void *stream) {
    if (int rc = mf_check_batch(mf, users, pos, neg, loss_out, B, "lgcn_mf_train_step")) return rc;
    return mf_step(mf, users, pos, neg, B, loss_out, (hipStream_t)stream);
}

extern "C" int lgcn_mf_train_epoch(lgcn_mf *mf, const int32_t *users, const int32_t *pos, const int32_t *neg, int64_t T, int32_t B,
                                   float *loss_out, void *stream) {
    if (int rc = mf_check_batch(mf, users, pos, neg, loss_out, B, "lgcn_mf_train_epoch")) return rc;
    int64_t i = 0;
    for (int64_t t = 0; t < T; t += B, i++) {
        const int32_t b = (int32_t)((T - t) < B ? (T - t) : B);
        if (int rc = mf_step(mf, users + t, pos + t, neg + t, b, loss_out + 3 * i, (hipStream_t)stream)) return rc;
    }
    return 0;
}

extern "C" int lgcn_mf_check(lgcn_mf *mf, void *stream) {
    if (!mf) { lgcn_set_error("lgcn_mf_check: null context"); return 3; }
    int32_t flag = 0;
    HIP_OK(hipMemcpyAsync(&flag, mf->c.err, sizeof flag, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    if (flag) {
        HIP_OK(hipMemsetAsync(mf->c.err, 0, sizeof flag, (hipStream_t)stream));
        lgcn_set_error("device flagged an out-of-range user/item id in a batch");
    }
    return flag;
}

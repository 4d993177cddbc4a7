// lgcn_eval_sweep.h -- what the units of the fused evaluation share (not installed).  k_eval_topk (lgcn_eval.hip)
// and k_eval_ranks (lgcn_eval_ranks.hip) run the same item sweep: a workgroup of NW waves x 32 users, the users' rows in registers
// as the B operand, item tiles of 32 rows staged through LDS, a user on a lane pair with 16 of the tile's scores in each lane's
// registers.  ONE definition here of the exact bf16 split and its MFMA, the geometry of an LDS tile, the user operand with its
// score tile, the tile stage, the lower-bound search of a CSR row and the launcher of the per-user sums.  (The accumulator type
// and its row formula: lgcn_device_common.h.)  k_eval_ranks runs the sweep from here; k_eval_topk still spells the operand, the
// stage and the score tile itself, because with these definitions its instantiations do not keep their instruction mix
// (profiles/eval_sweep/README.md): a change to the layout or the plane order is made here AND there.
#ifndef LGCN_EVAL_SWEEP_H
#define LGCN_EVAL_SWEEP_H
#include "lgcn_device_common.h"

// SPLIT3: the fp32 product on the bf16 matrix cores.  Every fp32 value is EXACTLY the sum of three bf16 values
// (x = h + m + l: 8 + 8 + 8 significant bits, by truncation: h = x & 0xffff0000, m = (x - h) & 0xffff0000, l = x - h - m,
// every subtraction exact), and every bf16 x bf16 product is exact in fp32, so
//     a . b = sum_k (ah + am + al)(bh + bm + bl)
// is accumulated from the six product planes hh, hm, mh, hl, lh, mm (smallest first) by v_mfma_f32_32x32x16_bf16 -- 24 MFMAs of
// 8 passes per 32 x 32 x 64 block instead of 32 of 16 passes.  The three planes left out (ml, lm, ll) are below 2^-23 of
// |a_k b_k| per term: the rounding an fp32 dot product of this length carries anyway (the ranking is fp32-accurate, not
// bit-identical to any one fp32 summation order -- neither is the reference's sgemm).
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
struct Planes2 { uint32_t h, m, l; };                        // two consecutive values, bf16 pairs (low half = first value)
__device__ __forceinline__ Planes2 split3(float x0, float x1) {
    const uint32_t M = 0xffff0000u;
    const float h0 = __uint_as_float(__float_as_uint(x0) & M), h1 = __uint_as_float(__float_as_uint(x1) & M);
    const float r0 = x0 - h0, r1 = x1 - h1;
    const float m0 = __uint_as_float(__float_as_uint(r0) & M), m1 = __uint_as_float(__float_as_uint(r1) & M);
    const float l0 = r0 - m0, l1 = r1 - m1;
    Planes2 o;
    o.h = (__float_as_uint(h0) >> 16) | __float_as_uint(h1);
    o.m = (__float_as_uint(m0) >> 16) | __float_as_uint(m1);
    o.l = (__float_as_uint(l0) >> 16) | (__float_as_uint(l1) & M);
    return o;
}
__device__ __forceinline__ f32x16 mfma_bf16(const u32x4 &a, const u32x4 &b, const f32x16 &c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// One item tile in LDS: 32 rows of D floats, the row stride RS padded by 16 B so the ds_read_b128 of 32 lanes at the same column
// hit different banks.  SPLIT3: three bf16 planes per tile, rows of D + 8 bf16 (144 bytes at d = 64: the 16-byte reads of 16
// lanes at one column start 36 banks apart and cover the 64 banks once).
template <int D, bool SPLIT3> struct SweepGeo {
    static constexpr int HALF = D / 2, RS = D + 4;
    static constexpr int RSB = D + 8, NCH = D / 16, PLANE_B = 32 * RSB * 2;
    static constexpr int TILE_F = SPLIT3 ? 3 * PLANE_B / 4 : 32 * RS;       // floats per item tile
};


// The user operand and the score tile.  Lane (j, h) holds half of user j's row as the B operand, in registers for the whole sweep
// (the k order inside a dot product is free, so each half-row is one contiguous run): fp32, elements [h D/2, (h + 1) D/2);
// SPLIT3, k = 16 c + 8 h + [0, 8) of MFMA step c as three bf16 planes.  scores(tile, j, h): 32 items x 32 users,
// scores[item i][user j] = sum_k I[i][k] U[j][k] from one LDS tile; the A operand of lane (i = j, h) is item i's half row, the
// accumulator puts user j on the lane and the item rows mfma32_row(reg, h) in its 16 registers.  SPLIT3 adds the product planes
// in the order mm; hl, lh; hm, mh; hh.
template <int D, bool SPLIT3> struct SweepUser;
template <int D> struct SweepUser<D, false> {
    using G = SweepGeo<D, false>;
    float b[D / 2];
    __device__ __forceinline__ void load(const float *row, int h) {
        const float *up = row + h * (D / 2);
#pragma unroll
        for (int s = 0; s < D / 2; s += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(up + s);
            b[s] = v.x; b[s + 1] = v.y; b[s + 2] = v.z; b[s + 3] = v.w;
        }
    }
    __device__ __forceinline__ f32x16 scores(const float *tile, int j, int h) const {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float *arow = &tile[j * G::RS + h * G::HALF];
#pragma unroll
        for (int s = 0; s < G::HALF; s += 4) {
            const f32x4 av = *reinterpret_cast<const f32x4 *>(arow + s);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b[s + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b[s + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b[s + 3], acc, 0, 0, 0);
        }
        return acc;
    }
};
template <int D> struct SweepUser<D, true> {
    using G = SweepGeo<D, true>;
    static constexpr int NCH = G::NCH, PLANE_B = G::PLANE_B;
    u32x4 bh[NCH], bm[NCH], bl[NCH];
    __device__ __forceinline__ void load(const float *row, int h) {
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const float *up = row + 16 * c + 8 * h;
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(up), v1 = *reinterpret_cast<const f32x4 *>(up + 4);
            const Planes2 p0 = split3(v0.x, v0.y), p1 = split3(v0.z, v0.w), p2 = split3(v1.x, v1.y), p3 = split3(v1.z, v1.w);
            bh[c] = u32x4{p0.h, p1.h, p2.h, p3.h}; bm[c] = u32x4{p0.m, p1.m, p2.m, p3.m}; bl[c] = u32x4{p0.l, p1.l, p2.l, p3.l};
        }
    }
    __device__ __forceinline__ f32x16 scores(const float *tile, int j, int h) const {
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const char *arow = reinterpret_cast<const char *>(tile) + (j * G::RSB + 8 * h) * 2;
        u32x4 ah[NCH], am[NCH], al[NCH];
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            am[c] = *reinterpret_cast<const u32x4 *>(arow + PLANE_B + 32 * c);
            ah[c] = *reinterpret_cast<const u32x4 *>(arow + 32 * c);
            al[c] = *reinterpret_cast<const u32x4 *>(arow + 2 * PLANE_B + 32 * c);
        }
#pragma unroll
        for (int c = 0; c < NCH; c++) acc = mfma_bf16(am[c], bm[c], acc);
#pragma unroll
        for (int c = 0; c < NCH; c++) { acc = mfma_bf16(ah[c], bl[c], acc); acc = mfma_bf16(al[c], bh[c], acc); }
#pragma unroll
        for (int c = 0; c < NCH; c++) { acc = mfma_bf16(ah[c], bm[c], acc); acc = mfma_bf16(am[c], bh[c], acc); }
#pragma unroll
        for (int c = 0; c < NCH; c++) acc = mfma_bf16(ah[c], bh[c], acc);
        return acc;
    }
};

// The tile stage of a workgroup of NT threads: tile t from the item table (rows past the table: zeros) into each thread's
// registers (coalesced 16-byte loads), and from there into LDS tile buffer `buf`.  Piece p of a tile: item row p / (D/4), 16-byte
// column p % (D/4).  (tid by reference, as the lambdas these functions were captured it: by value the compiler shares the column
// arithmetic of the two and every instantiation comes out a few instructions different from what was measured.)
template <int D, int NT> struct SweepStage {
    static constexpr int LPT = 32 * D * 4 / 16 / NT;           // 16-byte pieces per thread per item tile
    static_assert(LPT >= 1, "tile smaller than the workgroup");
    f32x4 pre[LPT];
};
template <int D, int NT>
__device__ __forceinline__ void sweep_load_tile(SweepStage<D, NT> &st, const float *items, int32_t m_items, int t, const int &tid) {
#pragma unroll
    for (int q = 0; q < SweepStage<D, NT>::LPT; q++) {
        const int p = tid + q * NT, r = p / (D / 4), c = p % (D / 4);
        const int64_t item = (int64_t)t * 32 + r;
        st.pre[q] = item < m_items ? *reinterpret_cast<const f32x4 *>(items + item * D + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}
template <int D, bool SPLIT3, int NT, int NBUF>
__device__ __forceinline__ void sweep_store_tile(const SweepStage<D, NT> &st, float (&tiles)[NBUF][SweepGeo<D, SPLIT3>::TILE_F], int buf, const int &tid) {
    using G = SweepGeo<D, SPLIT3>;
#pragma unroll
    for (int q = 0; q < SweepStage<D, NT>::LPT; q++) {
        const int p = tid + q * NT, r = p / (D / 4), c = p % (D / 4);
        if constexpr (SPLIT3) {                             // split once per workgroup, not once per wave
            const Planes2 p0 = split3(st.pre[q].x, st.pre[q].y), p1 = split3(st.pre[q].z, st.pre[q].w);
            char *dst = reinterpret_cast<char *>(tiles[buf]) + (r * G::RSB + 4 * c) * 2;
            *reinterpret_cast<uint2 *>(dst) = make_uint2(p0.h, p1.h);
            *reinterpret_cast<uint2 *>(dst + G::PLANE_B) = make_uint2(p0.m, p1.m);
            *reinterpret_cast<uint2 *>(dst + 2 * G::PLANE_B) = make_uint2(p0.l, p1.l);
        } else {
            *reinterpret_cast<f32x4 *>(&tiles[buf][r * G::RS + c * 4]) = st.pre[q];
        }
    }
}

// first position in idx[lo, hi) whose value is >= v (idx ascending: a row of a CSR)
__device__ __forceinline__ int64_t csr_lower_bound(const int32_t *idx, int64_t lo, int64_t hi, int32_t v) {
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (idx[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

// sums[c] = the sum of per_user[s * width + c] over the n_eval slots, in a fixed order (k_eval_sum, lgcn_eval.hip)
void lgcn_eval_sum_launch(const double *per_user, int32_t n_eval, int32_t width, double *sums, hipStream_t stream);
#endif

// lgcn_inbatch_tile.h -- the 32 x 32 score tile on the fp32-input MFMA (v_mfma_f32_32x32x2_f32) that the in-batch softmax
// (lgcn_inbatch.hip) and the alignment-and-uniformity loss (lgcn_directau.hip) both sweep: the accumulator
// layout, the k order of a score and the register form of its operands.  ONE definition of each (not installed); the functions
// stand here word for word as lgcn_inbatch.hip held them, so every instantiation of that file is the code it was.
#ifndef LGCN_INBATCH_TILE_H
#define LGCN_INBATCH_TILE_H
#include "lgcn_device_common.h"

// (the accumulator type f32x16 and its row formula mfma32_row: lgcn_device_common.h)

// 32 x 32 scores acc[i][j] = sum_k A[i][k] B[j][k]: arow / brow point at this lane's row (lane & 31) of each operand, at column
// h D/2.  MFMA number t multiplies columns (t, D/2 + t): the k order every score of this file is summed in.
template <int D>
__device__ __forceinline__ f32x16 ib_scores(const float *arow, const float *brow) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
    for (int s = 0; s < D / 2; s += 8) {
        const f32x4 a0 = *reinterpret_cast<const f32x4 *>(arow + s), a1 = *reinterpret_cast<const f32x4 *>(arow + s + 4);
        const f32x4 b0 = *reinterpret_cast<const f32x4 *>(brow + s), b1 = *reinterpret_cast<const f32x4 *>(brow + s + 4);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b0.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b0.w, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b1.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b1.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b1.w, acc, 0, 0, 0);
    }
    return acc;
}

// The same scores from operands already in registers (D <= 64: D / 2 floats per operand and lane): the owned side is loaded once
// per workgroup and the swept side's NEXT tile is loaded while this one is multiplied.  Same k order as ib_scores: the same bits.
template <int D> struct IbRow { f32x4 v[D / 8]; };
template <int D>
__device__ __forceinline__ void ib_load(IbRow<D> &r, const float *row) {
#pragma unroll
    for (int i = 0; i < D / 8; i++) r.v[i] = *reinterpret_cast<const f32x4 *>(row + 4 * i);
}
template <int D>
__device__ __forceinline__ f32x16 ib_scores_reg(const IbRow<D> &a, const IbRow<D> &b) {
    f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < D / 8; i++) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[i].x, b.v[i].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[i].y, b.v[i].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[i].z, b.v[i].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[i].w, b.v[i].w, acc, 0, 0, 0);
    }
    return acc;
}
constexpr int IB_REG_D = 64;      // up to this D the operands of a tile live in registers (and the next tile's are prefetched)
#endif

// lgcn_inbatch_tile.h -- the sweep over 32 x 32 score tiles on the fp32-input MFMA (v_mfma_f32_32x32x2_f32) that the in-batch
// softmax (lgcn_inbatch.hip) and the alignment-and-uniformity loss (lgcn_directau.hip) both run (DESIGN
// 4.29): the accumulator layout and the k order of a score, the part bounds, the owned operand with the swept one in its register
// or streamed form, and the gradient accumulator with its second product, the cosine projection's scalar and the projected
// epilogue into G64.  ONE definition of each (not installed).  A kernel of the four that sweep (k_inbatch_norm, k_inbatch_grad,
// k_directau_norm, k_directau_grad) holds what differs: which table is owned and which is swept, where the sweep starts, the mask
// and the weight of a register, and what happens to the partial.  The k order of a score and the register order of every sum are
// part of the result.  The score products are functions, word for word as lgcn_inbatch.hip held them; the pieces of the sweep
// round them are MACROS for the reason lgcn_batch_rows.h gives: as members of a struct they changed registers and selects of the
// sweeping kernels (profiles/loss_sweep/README.md), as macros every instantiation is the code it was.  Each macro lists every name
// of the kernel it reads beyond its arguments and every name it declares; j = lane & 31 and h = lane >> 5 throughout.  A macro that
// declares nothing is one statement (do { } while (0)).
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

// the tiles [t0, t1) of part `part` of a sweep over nT tiles: LGCN_INBATCH_PART_TILES per part, the last part what is left.
// Declares t0, t1; reads nothing
#define IB_PART_BOUNDS(part, nT)                                                                                                  \
    const int t0 = (part) * LGCN_INBATCH_PART_TILES, t1 = t0 + LGCN_INBATCH_PART_TILES < (nT) ? t0 + LGCN_INBATCH_PART_TILES : (nT)

// this lane's row of a table for tile t: row t * 32 + j at column h D/2.  Reads j, h
#define IB_TILE_ROW(D, tab, t) ((tab) + (int64_t)((t) * 32 + j) * D + h * (D / 2))

// The operands of a sweep from tile ts.  Up to IB_REG_D both live in registers: OWN is this lane's row of the owned table (brow)
// for the whole sweep, cur the swept table's tile ts, loaded if `nonempty` (ts < t1 where the sweep may be empty, true where it
// cannot: a part of the grid holds a tile).  Above IB_REG_D nothing is loaded here.  Declares RD, OWN, cur, nxt; reads brow (this
// lane's row of the owned table at column h D/2), j, h.
#define IB_SWEEP_BEGIN(D, OWN, swept, ts, nonempty)                                                                               \
    constexpr int RD = D <= IB_REG_D ? D : 8;   /* (the register form's types at a size that costs nothing where it is not used) */ \
    IbRow<RD> OWN, cur, nxt;                                                                                                      \
    if constexpr (D <= IB_REG_D) { ib_load(OWN, brow); if (nonempty) ib_load(cur, IB_TILE_ROW(D, swept, ts)); }

// ACC = the scores of tile t.  Register form: the NEXT tile's rows are loaded while this one is multiplied, clamped at the part's
// end (the last tile is loaded again, never one from t1 on).  Streamed form: ib_scores from L2.  Reads t1, brow, j, h and
// IB_SWEEP_BEGIN's RD, cur, nxt.
#define IB_SWEEP_SCORES(D, ACC, OWN, swept, t)                                                                                    \
    do {                                                                                                                          \
        if constexpr (D <= IB_REG_D) {                                                                                            \
            const int tn = (t) + 1 < t1 ? (t) + 1 : (t);                                                                          \
            ib_load(nxt, IB_TILE_ROW(D, swept, tn));                                                                              \
            ACC = ib_scores_reg<RD>(cur, OWN);                                                                                    \
            cur = nxt;                                                                                                            \
        } else {                                                                                                                  \
            ACC = ib_scores<D>(IB_TILE_ROW(D, swept, t), brow);                                                                   \
        }                                                                                                                         \
    } while (0)

// The gradient of a sweep: g[owned][col] += sum_x W[x][owned] Other[x][col] over the 32-column blocks from col0.
// ib_grad_blocks(D): the blocks a workgroup accumulates, the kernel's CB.  IB_GRAD_ZERO declares the accumulator g[CB], zeroed; reads CB.
constexpr int ib_grad_blocks(int D) { return D < 128 ? D / 32 : 4; }
#define IB_GRAD_ZERO()                                                                                                            \
    f32x16 g[CB];                                                                                                                 \
    _Pragma("unroll") for (int cb = 0; cb < CB; cb++)                                                                             \
        _Pragma("unroll") for (int reg = 0; reg < 16; reg++) g[cb][reg] = 0.f
// register form: the B operands of the second product for register reg (tile row x), in flight while the scores are multiplied.
// Reads ob (the kernel's float [16][CB] of this tile), reg, col0, j, CB
#define IB_GRAD_PREFETCH(D, oth, x)                                                                                               \
    do {                                                                                                                          \
        if constexpr (D <= IB_REG_D) {                                                                                            \
            _Pragma("unroll") for (int cb = 0; cb < CB; cb++) ob[reg][cb] = (oth)[(int64_t)(x) * D + col0 + j + cb * 32];         \
        }                                                                                                                         \
    } while (0)
// the second product of tile t: register i of the weights w IS the A operand (output row = lane & 31 = the owned index, k = lane
// half = tile rows r and r + 4 of register i), so W^T.Other accumulates with no lane movement and no LDS.  Reads w (the f32x16 of
// weights), g, ob, col0, j, h, CB
#define IB_GRAD_PRODUCT(D, oth, t)                                                                                                \
    do {                                                                                                                          \
        _Pragma("unroll") for (int reg = 0; reg < 16; reg++) {                                                                    \
            const float *orow = (oth) + (int64_t)((t) * 32 + mfma32_row(reg, h)) * D + col0 + j;                                  \
            _Pragma("unroll") for (int cb = 0; cb < CB; cb++) {                                                                   \
                float bv;                                                                                                         \
                if constexpr (D <= IB_REG_D) bv = ob[reg][cb]; else bv = orow[cb * 32];                                           \
                g[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[reg], bv, g[cb], 0, 0, 0);                                         \
            }                                                                                                                     \
        }                                                                                                                         \
    } while (0)
// the scalar of the chain through a cosine normalisation, t_o = sum_x W[x][o] s[x][o], summed per lane where W is formed: both
// lane halves (lane r and lane r + 32 hold owned row r's), then the scalar of register reg's row, on every lane (before any skip).
// Both read the kernel's float tproj; IB_GRAD_TPROJ_ROW reads h
#define IB_GRAD_TPROJ_COMBINE() tproj += __shfl_xor(tproj, 32)
#define IB_GRAD_TPROJ_ROW(reg) __shfl(tproj, mfma32_row(reg, h))
// register reg's row (owned index ob) into G64 row `row` through the projection inv_o (g - t_row own^): it is linear, so the parts
// of the sweep still meet order-free in G64.  Reads g, reg, ob (here the owned index of register reg's row), row (its G64 row),
// t_row (IB_GRAD_TPROJ_ROW(reg)), col0, j, CB
#define IB_GRAD_ADD_PROJECTED(D, G64, own, inv_o)                                                                                 \
    do {                                                                                                                          \
        _Pragma("unroll") for (int cb = 0; cb < CB; cb++) {                                                                       \
            const float oh = (own)[(int64_t)ob * D + col0 + cb * 32 + j];                                                         \
            fixed_add((G64) + row * D + col0 + cb * 32 + j, inv_o * (g[cb][reg] - t_row * oh));                                   \
        }                                                                                                                         \
    } while (0)
#endif

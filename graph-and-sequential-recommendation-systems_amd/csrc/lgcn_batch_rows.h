// lgcn_batch_rows.h -- what the batch-row kernels of the slot-form losses share (not installed): k_multineg
// (lgcn_multineg.hip), k_hardneg (lgcn_hardneg.hip), k_inbatch_rows (lgcn_inbatch.hip) and k_directau_rows (lgcn_directau.hip) all
// open with the same sample prologue over MultiNegArgs.  ONE definition of each piece, so every loss agrees on which samples are
// void and on what the reg term is.  What a void sample writes is each loss's own business and stays in the kernels.
//
// The pieces that hold statements are MACROS, not functions, and that is deliberate: the library is built with floating-point
// contraction on, and which multiply-add pairs hipcc fuses follows the shape of the code (profiles/batch_row_merge/README.md).  As
// __forceinline__ functions the id check alone -- integer code -- moved the fused pairs of the BPR pass of k_multineg at d 32 / 64,
// and the bitmap loop and the flag changed the scalar loads of every instantiation (profiles/loss_sweep/README.md).  A macro leaves
// the kernel the token sequence it had: every instantiation of the four kernels is the parent's code, byte for byte.  Each macro
// lists in its comment every name of the kernel it reads beyond its arguments ("reads") and every name it declares; a piece is
// used once per kernel, at the place the text stood.  A macro that declares nothing is one statement (do { } while (0)).
#ifndef LGCN_BATCH_ROWS_H
#define LGCN_BATCH_ROWS_H
#include "lgcn_device_common.h"

// One lane group of min(D, 64) lanes per sample, lane = column (mod 64), 256 / min(D, 64) samples per workgroup (the geometry
// of k_triplet_dense): every load and every 64-bit atomic wave-instruction covers min(D, 64) contiguous elements.
template <int D> struct RowsGeo {
    static constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT, SPB = 256 / LPT;     // lanes per sample, columns per lane, samples per workgroup
    static constexpr unsigned long long GROUP = LPT == 64 ? ~0ull : ((1ull << (LPT & 63)) - 1ull);      // the lanes of a group, from bit 0
};

// The kernel's names for the geometry, its sample b and its lane l in the sample's group.  Declares LPT, CPT, SPB, b, l; reads nothing
#define ROWS_GEOMETRY(D)                                                                                                          \
    constexpr int LPT = RowsGeo<D>::LPT, CPT = RowsGeo<D>::CPT, SPB = RowsGeo<D>::SPB;                                            \
    const int b = blockIdx.x * SPB + threadIdx.x / LPT, l = threadIdx.x % LPT

// last step's row bitmap is dead: zero it here with plain stores (the two bitmaps alternate per step).  Reads nothing but a
#define ROWS_ZERO_STALE_BITMAP(a)                                                                                                 \
    do {                                                                                                                          \
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (a).bitmap_words; i += (int64_t)gridDim.x * 256)            \
            (a).stale_bitmap[i] = 0u;                                                                                             \
    } while (0)

// Every id is checked before anything is addressed with it: user in [0, n_users), item with id + n_users < N.  Declares id (this
// lane's, 0 where the lane holds none), GROUP, gshift (this group's first lane in the wave) and bad: an out-of-range id voids the
// whole sample, and so does live == false (the padding of a workspace).  Declares id, idbad, GROUP, gshift, bad; reads b, l, LPT and the
// kernel's D.  A layout is a macro (a, NEGS) over id, idbad, b, l; NEGS: the sample has negatives (ROWS_NEGS_FIRST always has them and
// takes the argument only so that both layouts are called alike).  Two lane layouts; the ids only route rows:
//   ROWS_NEGS_FIRST  lanes 0..R-1 the negatives, lanes R / R + 1 the user / positive (k_multineg, k_hardneg; R <= 16 <= the smallest group)
//   ROWS_PAIR_FIRST  lane 0 / 1 the user / positive and, with NEGS, lanes 2..R+1 the negatives (k_inbatch_rows, k_directau_rows)
#define ROWS_ITEM_BAD(a, id) ((id) < 0 || (int64_t)(id) + (a).n_users >= (a).N)
#define ROWS_NEGS_FIRST(a, NEGS)                                                                                                 \
    if (l < (a).R) { id = (a).negs[(int64_t)l * (a).neg_stride + b]; idbad = ROWS_ITEM_BAD(a, id); }                              \
    else if (l == (a).R) { id = (a).users[b]; idbad = id < 0 || id >= (a).n_users; }                                              \
    else if (l == (a).R + 1) { id = (a).pos[b]; idbad = ROWS_ITEM_BAD(a, id); }
#define ROWS_PAIR_FIRST(a, NEGS)                                                                                                 \
    if (l == 0) { id = (a).users[b]; idbad = id < 0 || id >= (a).n_users; }                                                       \
    else if (l == 1) { id = (a).pos[b]; idbad = ROWS_ITEM_BAD(a, id); }                                                           \
    if constexpr (NEGS) {                                                                                                         \
        if (l >= 2 && l < 2 + (a).R) { id = (a).negs[(int64_t)(l - 2) * (a).neg_stride + b]; idbad = ROWS_ITEM_BAD(a, id); }      \
    }
#define ROWS_LOAD_IDS(a, LAYOUT, NEGS, live)                                                                                     \
    int32_t id = 0;                                                                                                               \
    bool idbad = false;                                                                                                           \
    if (live) { LAYOUT(a, NEGS) }                                                                                                 \
    constexpr unsigned long long GROUP = RowsGeo<D>::GROUP;                                                                       \
    const int gshift = (threadIdx.x & 63) / LPT * LPT;                                                                            \
    const bool bad = !(live) || (__ballot(idbad) & (GROUP << gshift)) != 0ull
// a vote of the group's lanes, lane 0 of the group at bit 0 (reads GROUP, gshift)
#define ROWS_VOTES(v) ((__ballot(v) >> gshift) & GROUP)

// The user's and the positive's output-table rows u[], p[] (slot_row) with the squares of the reg term (reg_ego: of the tables' own
// rows) summed over this lane's columns into ru2 / rp2.  PS_STMT runs per column beside the positive's square: `ps += u[j] * p[j]`
// where the loss wants the score.  Declares t0; reads a, ru, rp, l, ego, u, p, ru2, rp2, CPT and the kernel's D, TI, WTS; PS_STMT
// sees the column j and v.
#define ROWS_PAIR(PS_STMT)                                                                                                        \
    float t0[CPT];                                                                                                                \
    slot_row<D, TI, WTS>(a, ru, l, u, t0);                                                                                        \
    _Pragma("unroll") for (int j = 0; j < CPT; j++) { const float v = ego ? t0[j] : u[j]; ru2 += v * v; }                         \
    slot_row<D, TI, WTS>(a, rp, l, p, t0);                                                                                        \
    _Pragma("unroll") for (int j = 0; j < CPT; j++) { const float v = ego ? t0[j] : p[j]; PS_STMT; rp2 += v * v; }

// the end of the prologue: flag this lane's row and count it with weight w (the backward's epilogue turns cnt into the reg_ego
// term).  Reads nothing but its arguments
#define ROWS_FLAG(a, myrow, w)                                                                                                    \
    do {                                                                                                                          \
        atomicOr((a).bitmap + ((myrow) >> 5), 1u << ((myrow) & 31));                                                              \
        if ((a).cnt) atomicAdd((a).cnt + (myrow), w);                                                                             \
    } while (0)

// inv(e) = 1 / |e| from nn = the fp32 sum of squares of a row (0 for |e| = 0): sqrtf and an IEEE division, two roundings.  (The sum
// itself stays in the kernels: as part of this function its multiply-adds fused differently at d 128 / 256.)
__device__ __forceinline__ float rows_inv_norm(float nn) { return nn > 0.f ? 1.f / sqrtf(nn) : 0.f; }

// runs the statement with the storage type TI (float | bf16_t) and WTS (layer weights) compile-time: the ladder of a rows kernel
#define DISPATCH_ROWS(act_dtype, wts, ...)                                         \
    do {                                                                           \
        if ((act_dtype) == LGCN_F32) {                                             \
            if (wts) { using TI = float; constexpr bool WTS = true; __VA_ARGS__; } \
            else { using TI = float; constexpr bool WTS = false; __VA_ARGS__; }    \
        } else {                                                                   \
            if (wts) { using TI = bf16_t; constexpr bool WTS = true; __VA_ARGS__; } \
            else { using TI = bf16_t; constexpr bool WTS = false; __VA_ARGS__; }   \
        }                                                                          \
    } while (0)
#endif

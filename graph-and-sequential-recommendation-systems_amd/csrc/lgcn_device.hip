// lgcn_device.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the LightGCN/BPR
// training hot path: kernels and their launchers (lgcn_kernels.h).  The host side -- the graph
// object and its plan, the training context and the step driver -- is lgcn_graph.cpp and
// lgcn_train.cpp; build.kernel_hash() is the hash of this file.
//
// The path is sparse and HBM/cache-bandwidth bound (<= 0.5 flop/byte): no MFMA.
// What matters here: 16-byte (fp32) / 8-byte (bf16) per-lane row gathers that
// cover whole 128/256-byte embedding rows, fp32 accumulation, wavefront
// (ds_swizzle/DPP) reductions, fused epilogues so that no dense [N,d]
// intermediate is written twice, and a launch geometry of >> 256 workgroups.
//
// Reference semantics (LightGCN_work/code): model.py:201-231 (computer),
// model.py:162-183 (bpr_loss), utils.py:53-64 (stageOne = fwd + backward + Adam).
//
// Algebra used (exact restructuring):
//  * forward needs dense X_1..X_{K-1} only; the last layer X_K and the layer mean
//    are evaluated on the <= 3B rows the batch gathers (k_triplet).
//  * backward is the Horner chain h_{k-1} = Gs + A h_k, Gs = G/(K+1); Gs has
//    <= 3B non-zero rows, so the first backward SpMM skips zero rows by bitmap
//    and gathers the flagged rows from a fp32 copy made once per step (k_g32).
//  * the last backward SpMM applies Adam in its epilogue (no dense grad buffer).
//  * with layer weights (lgcn_ctx_set_layer_weights) the mean becomes sum_k w_k X_k and the chain
//    h_K = w_K G, h_{k-1} = w_{k-1} G + A h_k: Gs is then G unscaled and every backward launch carries its two
//    coefficients (M_WTS); the weighted forms are compile-time axes, so the kernels of the mean are what they were.
//  * the scatter-add of per-triplet gradient rows uses 64-bit fixed-point integer
//    atomics (scale 2^50): integer addition is associative, so the result is
//    bitwise reproducible and independent of batch sharding.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <math.h>

#include "lgcn_device_common.h"      // (through lgcn_internal.h: lgcn_kernels.h, the args structs and the constants the host shares)

typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(16))) __bf16 bf16x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
// LGCN_FP8: a table of n rows is  n * D bytes of OCP E4M3 values  followed by  n fp32 ROW SCALES  (value = scale * fp8): one
// pointer names both.  Scales are powers of two with max|row| / scale in [64, 128) (inside the range of both E4M3 flavours;
// a division by a power of two is exact, so the quantisation is a pure fp8 rounding the tests restate bit for bit).
// The columns of an fp8 row are CHUNK-INTERLEAVED: with L = D / 16 lanes per row, the 16 bytes at l*16 hold the four 4-column
// chunks q = j*L + l (j = 0..3): byte l*16 + 4j + e = column (j*L + l)*4 + e.  A lane that gathers 16 bytes therefore owns four
// float4 chunks that lie L chunks apart, and the fp32 side of every epilogue (G32, P / M / V, fp32 outputs) is four fully
// coalesced float4 accesses per row instead of 64 contiguous bytes per lane (measured on the 10M x 1M graph: Adam's operands of
// the fp8 step streamed at 4.0 TB/s with the natural order against 6.6 TB/s in the fp32 step).  The table is an opaque blob of
// the ABI (lgcn_to_fp8 writes it, the kernels read it); lgcn_fp8_col_of_byte gives the order for anyone who decodes it.
struct fp8_t { uint8_t v; };
__host__ __device__ __forceinline__ int fp8_byte_of_col(int c, int D) { const int L = D / 16, q = c >> 2; return (q % L) * 16 + 4 * (q / L) + (c & 3); }
__device__ __forceinline__ const float *fp8_scales(const void *tab, int64_t n_rows, int D) { return (const float *)((const char *)tab + n_rows * D); }
__device__ __forceinline__ float *fp8_scales(void *tab, int64_t n_rows, int D) { return (float *)((char *)tab + n_rows * D); }

// C fp32 values per lane (C = 4: 16 B of fp32 / 8 B of bf16; C = 8: 32 B of fp32 / 16 B of bf16)
template <int C> struct VecF;
template <> struct VecF<4> { typedef f32x4 T; typedef bf16x4 B; };
template <> struct VecF<8> { typedef f32x8 T; typedef bf16x8 B; };
template <> struct VecF<16> { typedef f32x16 T; typedef bf16x16 B; };

template <int C> __device__ __forceinline__ typename VecF<C>::T zerov() {
    typename VecF<C>::T z;
#pragma unroll
    for (int i = 0; i < C; i++) z[i] = 0.f;
    return z;
}
template <int C> __device__ __forceinline__ typename VecF<C>::T loadv(const float *p) {
    return *reinterpret_cast<const typename VecF<C>::T *>(p);
}
template <int C> __device__ __forceinline__ typename VecF<C>::T loadv(const bf16_t *p) {
    return __builtin_convertvector(*reinterpret_cast<const typename VecF<C>::B *>(p), typename VecF<C>::T);
}
template <int C> __device__ __forceinline__ void storev(float *p, typename VecF<C>::T v) {
    *reinterpret_cast<typename VecF<C>::T *>(p) = v;
}
template <int C> __device__ __forceinline__ void storev(bf16_t *p, typename VecF<C>::T v) {
    *reinterpret_cast<typename VecF<C>::B *>(p) = __builtin_convertvector(v, typename VecF<C>::B);
}
__device__ __forceinline__ f32x4 load4(const float *p) { return loadv<4>(p); }
__device__ __forceinline__ f32x4 load4(const bf16_t *p) { return loadv<4>(p); }
__device__ __forceinline__ void store4(float *p, f32x4 v) { storev<4>(p, v); }
__device__ __forceinline__ void store4(bf16_t *p, f32x4 v) { storev<4>(p, v); }
// A lane's 16-byte piece at p + OFF bytes, stored WRITE-THROUGH (the vector store with sc1): the bytes go on to memory and the
// line is dropped from this XCD's L2 instead of staying there dirty.  For rows that nobody gathers and the next reader takes row
// by row; SpmmArgs::wt says which stores of a launch take this form.  A 16-byte sc1 store costs what the plain one
// costs (narrower ones do not), so this is the one form.  p: a global address, 16-byte aligned with OFF.  The trailing s_nop 1:
// a store of more than 8 bytes reads its data registers late, and nothing outside the string is padded for it.
template <int OFF> __device__ __forceinline__ void store16_wt(void *p, f32x4 v) {
    static_assert(OFF >= 0 && OFF < 4096 && OFF % 16 == 0, "immediate offset of a global store");
    asm volatile("global_store_dwordx4 %0, %1, off offset:%2 sc1\n\ts_nop 1" : : "v"(p), "v"(v), "n"(OFF) : "memory");
}
// C consecutive fp32 values (C / 4 pieces) / 8 bf16 values (one piece) of a lane, write-through
template <int C> __device__ __forceinline__ void storev_wt(float *p, typename VecF<C>::T v) {
    store16_wt<0>(p, f32x4{v[0], v[1], v[2], v[3]});
    if constexpr (C >= 8) store16_wt<16>(p, f32x4{v[4], v[5], v[6], v[7]});
    if constexpr (C == 16) { store16_wt<32>(p, f32x4{v[8], v[9], v[10], v[11]}); store16_wt<48>(p, f32x4{v[12], v[13], v[14], v[15]}); }
}
__device__ __forceinline__ void storev_wt(bf16_t *p, f32x8 v) {
    union { bf16x8 b; f32x4 f; } u; u.b = __builtin_convertvector(v, bf16x8);
    store16_wt<0>(p, u.f);
}
// one fp8 element of a table, decoded (k_triplet's lower-layer rows: lane = column): the fp8 form of the header's tab_elem
__device__ __forceinline__ float fp8_decode(uint8_t b) { return __builtin_amdgcn_cvt_pk_f32_fp8((int)b, false)[0]; }
template <> __device__ __forceinline__ float tab_elem<fp8_t>(const void *tab, int64_t n_rows, int D, int64_t row, int col) {
    return fp8_scales(tab, n_rows, D)[row] * fp8_decode(((const uint8_t *)tab)[row * D + fp8_byte_of_col(col, D)]);
}
// scale of a row whose largest magnitude is amax: 2^(e - 6) for amax = 1.f * 2^e  ->  amax / scale in [64, 128); rows
// below 2^-100 (and zero rows) are stored as zeros with scale 1; every other finite row, up to the top of fp32, is scaled
__device__ __forceinline__ void fp8_row_scale(float amax, float &scale, float &inv) {
    const uint32_t E = __float_as_uint(amax) >> 23;           // biased exponent (amax >= 0)
    if (E < 27u || E == 255u) { scale = 1.f; inv = E == 255u ? 1.f : 0.f; return; }      // (inf / NaN rows stay inf / NaN)
    scale = __uint_as_float((E - 6u) << 23); inv = __uint_as_float((260u - E) << 23);
}
// Store one row piece of C values per lane as fp8: the row's LPR = D / C lanes (contiguous, aligned, all active) agree on
// the row maximum through xor shuffles, every lane quantises its piece, lane l == 0 writes the scale.
// IL: v holds the lane's four interleaved chunks (an fp8 table was gathered: C = 16) -- its 16 bytes are contiguous at l*16;
// otherwise v holds C consecutive columns (an fp32 / bf16 table was gathered) and every 4-column chunk goes to its own word.
template <int D, int C, bool IL>
__device__ __forceinline__ void store_row_fp8(void *tab, int64_t n_rows, int64_t row, int l, typename VecF<C>::T v) {
    static_assert(!IL || C == 16, "interleaved accumulators come from fp8 gathers: 16 per lane");
    constexpr int LPR = D / C;
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < C; i++) amax = fmaxf(amax, fabsf(v[i]));
#pragma unroll
    for (int o = 1; o < LPR; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    float scale, inv;
    fp8_row_scale(amax, scale, inv);
    uint32_t w[C / 4];
#pragma unroll
    for (int i = 0; i < C / 4; i++) {
        int p = 0;
        p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i] * inv, v[4 * i + 1] * inv, p, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i + 2] * inv, v[4 * i + 3] * inv, p, true);
        w[i] = (uint32_t)p;
    }
    if (IL) {
        uint32_t *dst = (uint32_t *)((char *)tab + row * D + l * 16);
#pragma unroll
        for (int i = 0; i < C / 4; i++) dst[i] = w[i];
    } else {
#pragma unroll
        for (int i = 0; i < C / 4; i++) *(uint32_t *)((char *)tab + row * D + fp8_byte_of_col((l * (C / 4) + i) * 4, D)) = w[i];
    }
    if (l == 0) fp8_scales(tab, n_rows, D)[row] = scale;
}
// row piece store by output type
// a lane's piece of an fp32 row: C consecutive columns at l*C, or (IL: the accumulators of an fp8 gather) the four float4 chunks j*L + l
template <int D, int C, bool IL> __device__ __forceinline__ typename VecF<C>::T row_load(const float *base, int64_t row, int l) {
    if constexpr (!IL) return loadv<C>(base + row * D + l * C);
    else {
        typename VecF<C>::T r;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const f32x4 t = load4(base + row * D + (j * (D / 16) + l) * 4);
            r[4 * j] = t.x; r[4 * j + 1] = t.y; r[4 * j + 2] = t.z; r[4 * j + 3] = t.w;
        }
        return r;
    }
}
// wt (wave-uniform): the pieces go write-through (store16_wt)
template <int D, int C, bool IL> __device__ __forceinline__ void row_store(float *base, int64_t row, int l, typename VecF<C>::T v, bool wt = false) {
    if constexpr (!IL) {
        if (wt) storev_wt<C>(base + row * D + l * C, v);
        else storev<C>(base + row * D + l * C, v);
    } else if (wt) {      // the four chunks lie D / 16 pieces = D bytes apart
        float *p = base + row * D + l * 4;
        store16_wt<0>(p, f32x4{v[0], v[1], v[2], v[3]}); store16_wt<D>(p, f32x4{v[4], v[5], v[6], v[7]});
        store16_wt<2 * D>(p, f32x4{v[8], v[9], v[10], v[11]}); store16_wt<3 * D>(p, f32x4{v[12], v[13], v[14], v[15]});
    } else {
#pragma unroll
        for (int j = 0; j < 4; j++) store4(base + row * D + (j * (D / 16) + l) * 4, f32x4{v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]});
    }
}
// (wt: honoured for fp32 and bf16 outputs whose piece per lane is 16 bytes or a multiple -- what a forward launch on fp32 / bf16
//  tables writes; the 8-byte bf16 pieces of a launch that gathered fp32 rows stay plain.  A launch that gathered an fp8 table
//  ignores it: its instantiations are budgeted at 4-5 waves per SIMD, and the second store form took the forward ones from
//  88-94 to 126-128 VGPRs -- lgcn_train.cpp does not ask for it there)
template <int D, int C, typename TO, bool IL> struct RowStore {
    static __device__ __forceinline__ void put(void *Y, int64_t, int64_t row, int l, typename VecF<C>::T v, bool wt = false) {
        static_assert(!IL, "an fp8 gather writes fp32 or fp8");
        if constexpr (C == 8) { if (wt) { storev_wt((TO *)Y + row * D + l * C, v); return; } }
        storev<C>((TO *)Y + row * D + l * C, v); }
};
template <int D, int C, bool IL> struct RowStore<D, C, float, IL> {
    static __device__ __forceinline__ void put(void *Y, int64_t, int64_t row, int l, typename VecF<C>::T v, bool wt = false) { row_store<D, C, IL>((float *)Y, row, l, v, IL ? false : wt); }
};
template <int D, int C, bool IL> struct RowStore<D, C, fp8_t, IL> {
    static __device__ __forceinline__ void put(void *Y, int64_t n_rows, int64_t row, int l, typename VecF<C>::T v, bool = false) { store_row_fp8<D, C, IL>(Y, n_rows, row, l, v); }
};
__device__ __forceinline__ bool bit_set(const uint32_t *bm, int i) { return (bm[i >> 5] >> (i & 31)) & 1u; }

// fixed-point gradient row -> fp32 Gs row:  (float)(q * 2^-50) / (K+1)
template <int C> __device__ __forceinline__ typename VecF<C>::T loadv_fixed(const long long *p, float div) {
    typedef __attribute__((ext_vector_type(2))) long long i64x2_;
    typename VecF<C>::T r;
#pragma unroll
    for (int i = 0; i < C; i += 2) {
        const i64x2_ a = *reinterpret_cast<const i64x2_ *>(p + i);
        r[i] = (float)((double)a.x * FIXED_INV) / div; r[i + 1] = (float)((double)a.y * FIXED_INV) / div;
    }
    return r;
}

// ---------------------------------------------------------------------------------
// Edge dropout of one training step (upstream LightGCN's __dropout_x): every stored non-zero (i, j) of A_hat is
// kept when  H(seed, step, i, j) < thr = floor(keep_prob * 2^32)  and the survivors are scaled by 1 / keep_prob.  H is a
// counter-based hash of the adjacency's own row and column ids and of nothing else -- not of where the entry lies in the CSR
// arrays, the plan's packed stream or the launch -- so every kernel that meets the entry decides alike:
//     (k0, k1) = low / high word of  splitmix64(splitmix64(seed) + step)        (host, once per step)
//     H        = fmix32( fmix32(i ^ k0) ^ (j * 0x9E3779B1) ^ k1 )               (fmix32: MurmurHash3's 32-bit finaliser)
// 32-bit multiplies, shifts and xors on the VALU (about two dozen instructions per staged entry, five of them multiplies), no table, no LDS.  The mask is applied
// where an entry is STAGED (tile_stage's callers, the pack path of k_spmm): its weight becomes val * (1 / keep_prob) or zero;
// gather loops, epilogues and the chunk hand-off never see it.  tr: the launch computes A_drop^T h (backward), where the
// entry stored at (row, col) stands for A_drop[col, row] and carries keep(col, row).  (DropArgs: lgcn_kernels.h)
// ---------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t drop_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__host__ __device__ __forceinline__ uint32_t drop_hash(uint32_t k0, uint32_t k1, uint32_t i, uint32_t j) {
    return drop_fmix32(drop_fmix32(i ^ k0) ^ (j * 0x9E3779B1u) ^ k1);
}
// is the entry the launch reads at (row, col) of the stored matrix alive this step?
__device__ __forceinline__ bool drop_live(const DropArgs &d, int row, int col) {
    const uint32_t i = (uint32_t)(d.tr ? col : row), j = (uint32_t)(d.tr ? row : col);
    return drop_hash(d.k0, d.k1, i, j) < d.thr;
}

struct GatherSrc {           // what a row gather reads
    const float *S;          // fp8 table: its row scales (an entry's weight is multiplied by S[col] when it is staged), else NULL
    const void *X;           // [N,D] of TI; SPARSE: the fp32 copy of the flagged gradient rows (k_g32)
    const uint32_t *bm;      // SPARSE: non-zero-row bitmap (global, or the workgroup's LDS copy)
    float div;               // unused by the gathers (K+1; the epilogues take it from SpmmArgs)
    DropArgs dr;             // DROP instantiations only: the step's edge-dropout mask
};

// Raw (unconverted) piece of a gathered row: 16 bytes per lane for fp32 AND bf16 tables (4 / 8
// columns), so one wave-instruction always moves 1 KiB = 4 fp32 rows / 8 bf16 rows at d = 64 and the
// bf16 table needs HALF the gather instructions of the fp32 one (with 8 B per lane the bf16 kernel
// issued as many gathers as the fp32 one and was instruction-bound: +15 % for half the bytes).
// The conversion to fp32 is kept OUT of the load block: hipcc otherwise waits vmcnt(0) inside every
// block and the U gathers serialise (measured: bf16 SpMM 2x slower than fp32).
struct fixed4 { i64x2 a, b; };
template <typename TI, bool SPARSE> struct Raw;
template <> struct Raw<float, false> {
    static constexpr int CPL = 4;
    typedef f32x4 T;
    // BIG = false (table under 4 GiB): uniform base + ONE 32-bit byte offset per gather (v_lshl_add_u32, SGPR-base
    // addressing) instead of a sign extension, a 64-bit shift and a 64-bit add per gathered row
    template <bool BIG> static __device__ __forceinline__ T load(const GatherSrc &s, int col, int D, int l) {
        if (BIG) return *reinterpret_cast<const T *>((const float *)s.X + (int64_t)col * D + l * 4);
        return *reinterpret_cast<const T *>((const char *)s.X + ((uint32_t)col * (uint32_t)(D * 4) + (uint32_t)(l * 16))); }
    static __device__ __forceinline__ f32x4 cvt(const T &r, float) { return r; }
};
template <> struct Raw<bf16_t, false> {
    static constexpr int CPL = 8;
    typedef bf16x8 T;
    template <bool BIG> static __device__ __forceinline__ T load(const GatherSrc &s, int col, int D, int l) {
        if (BIG) return *reinterpret_cast<const T *>((const bf16_t *)s.X + (int64_t)col * D + l * 8);
        return *reinterpret_cast<const T *>((const char *)s.X + ((uint32_t)col * (uint32_t)(D * 2) + (uint32_t)(l * 16))); }
    static __device__ __forceinline__ f32x8 cvt(const T &r, float) { return __builtin_convertvector(r, f32x8); }
};
template <> struct Raw<fp8_t, false> {
    static constexpr int CPL = 16;
    typedef u32x4 T;
    template <bool BIG> static __device__ __forceinline__ T load(const GatherSrc &s, int col, int D, int l) {
        if (BIG) return *reinterpret_cast<const T *>((const char *)s.X + (int64_t)col * D + l * 16);
        return *reinterpret_cast<const T *>((const char *)s.X + ((uint32_t)col * (uint32_t)D + (uint32_t)(l * 16))); }
    // the row scale is NOT applied here: the entry's weight was multiplied by it when the entry was staged
    static __device__ __forceinline__ f32x16 cvt(const T &r, float) {
        f32x16 o;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[i], false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[i], true);
            o[4 * i] = a[0]; o[4 * i + 1] = a[1]; o[4 * i + 2] = b[0]; o[4 * i + 3] = b[1];
        }
        return o;
    }
};
// SPARSE: the flagged rows of Gs, converted once per step from the fixed-point accumulator to fp32 by k_g32
// (gathering the 512-byte int64 rows and converting every gathered copy -- int64 -> fp64 -> fp32 and a
// division per element -- made this launch cost as much as a dense layer for a quarter of its gathers)
template <typename TI> struct Raw<TI, true> : Raw<float, false> {};
// geometry of one kernel instance: columns per lane, lanes per row, neighbour rows per wave-instruction
template <int D, typename TI, bool SPARSE> struct Geo {
    static constexpr int CPL = Raw<TI, SPARSE>::CPL, LPR = D / CPL, NPW = 64 / LPR;
    typedef typename VecF<CPL>::T Acc;
};

// ---------------------------------------------------------------------------------
// One CSR row segment [start,end) of  A_hat * X  computed by one wavefront.
//
// The segment is walked in tiles of 64 non-zeros.  Per tile: every lane loads one
// (col,val) pair -- one coalesced 256-byte read of each CSR stream -- and the tile is
// staged in a wave-private LDS slot.  Then LPR lanes cover one embedding row with 16
// bytes each and the wave's NPW = 64/LPR lane groups take the staged neighbours
// interleaved, U deep, so every lane has up to U independent row gathers in flight
// behind ONE index round trip.  SPARSE: only neighbours whose row is flagged in the
// bitmap are staged (ballot + prefix-popcount compaction), the rest cost no gather.
// Partial sums are combined across the lane groups in a fixed order: deterministic,
// and identical wherever this function is used.
// ---------------------------------------------------------------------------------
// stage one tile of n <= 64 (col,val) pairs held one per lane; returns the staged count.  The tile is followed by
// zero-weight entries (column 0) up to TILE_PAD positions past its end, so that the gather batches below read
// past-the-end slots WITHOUT a per-gather clamp / compare / select (3 vector instructions per gathered row):
// positions [cnt, 64) are written here, positions [64, 64 + TILE_PAD) once per wave by tile_pad_init().
#define TILE_PAD 64           /* >= 4 * NPW of every geometry (d = 32 with a bf16 table: NPW = 16) */
#define TILE_ST (64 + TILE_PAD)
__device__ __forceinline__ void tile_pad_init(int2 *stage, int lane) { stage[64 + lane] = make_int2(0, 0); }
// live: edge dropout kept the entry (its weight is already scaled; a dropped entry's is zero).  SPARSE treats a dropped
// entry as unflagged, so the compaction skips its gather; the dense form stages it with its zero weight.
template <bool SPARSE>
__device__ __forceinline__ int tile_stage(int col, float val, int n, const GatherSrc &src, int lane, int2 *stage, bool live = true) {
    if (!SPARSE) {
        stage[lane] = lane < n ? make_int2(col, __float_as_int(val)) : make_int2(0, 0);
        return n;
    }
    const bool act = (lane < n) && live && bit_set(src.bm, col);
    const unsigned long long mask = __ballot(act);
    const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
    const int cnt = __popcll(mask);
    // flagged entries at their compacted position, the others behind them as zero-weight padding: all 64 slots written
    stage[act ? below : cnt + (lane - below)] = act ? make_int2(col, __float_as_int(val)) : make_int2(0, 0);
    return cnt;
}

// One batch of U gathers per lane: entries j0+g, j0+g+NPW, ... of the staged tile (past the end: zero-weight padding).
template <int D, typename TI, bool SPARSE, int U, bool BIG>
__device__ __forceinline__ void gather_batch(const int2 *stage, int j0, const GatherSrc &src, int lane,
                                             typename Geo<D, TI, SPARSE>::Acc &acc) {
    typedef Geo<D, TI, SPARSE> G;
    typedef Raw<TI, SPARSE> R;
    const int g = lane / G::LPR, l = lane % G::LPR;
    int2 cv[U]; typename R::T x[U];
    const int2 *p = stage + j0 + g;
#pragma unroll
    for (int u = 0; u < U; u++) cv[u] = p[u * G::NPW];                   // all LDS reads first (one base, immediate offsets)
#pragma unroll
    for (int u = 0; u < U; u++) x[u] = R::template load<BIG>(src, cv[u].x, D, l);      // U gathers in flight
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; u++) acc += __int_as_float(cv[u].y) * R::cvt(x[u], src.div);
}

// Gather-accumulate the staged tile.  The batch depth follows the (wave-uniform) number of staged
// neighbours instead of always issuing the deepest batch: a 64-lane gather instruction costs the
// CU's address path the same whether 1 or all of its row slots are useful.
template <int D, typename TI, bool SPARSE, bool BIG, int UCAP = LGCN_GATHER_U>
__device__ __forceinline__ void tile_gather(const int2 *stage, int cnt, const GatherSrc &src, int lane,
                                            typename Geo<D, TI, SPARSE>::Acc &acc) {
    constexpr int NPW = Geo<D, TI, SPARSE>::NPW, UMAX = SPARSE ? 4 : UCAP;
    static_assert(4 * NPW <= TILE_PAD, "the padding behind a tile must cover the deepest batch's overshoot");
    cnt = __builtin_amdgcn_readfirstlane(cnt);
    int j = 0;
    if (UMAX >= 8) for (; cnt - j > 4 * NPW; j += 8 * NPW) gather_batch<D, TI, SPARSE, (UMAX >= 8 ? 8 : UMAX), BIG>(stage, j, src, lane, acc);
    if (UMAX >= 4) for (; cnt - j > 2 * NPW; j += 4 * NPW) gather_batch<D, TI, SPARSE, (UMAX >= 4 ? 4 : UMAX), BIG>(stage, j, src, lane, acc);
    for (; cnt - j > NPW; j += 2 * NPW) gather_batch<D, TI, SPARSE, 2, BIG>(stage, j, src, lane, acc);
    if (cnt - j > 0) gather_batch<D, TI, SPARSE, 1, BIG>(stage, j, src, lane, acc);
}

// Sum over the lanes that hold the same columns (lane % LPR equal): every lane ends with the full
// sum.  VALU only -- v_permlane32_swap / v_permlane16_swap (gfx950) exchange wave halves / 16-lane rows
// without the LDS crossbar, DPP row rotations finish inside a row.  Fixed order: bitwise reproducible.
__device__ __forceinline__ float sum_xor32(float v) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    const unsigned a = __float_as_uint(v);
    const u32x2 r = __builtin_amdgcn_permlane32_swap(a, a, false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ float sum_xor16(float v) {
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    const unsigned a = __float_as_uint(v);
    const u32x2 r = __builtin_amdgcn_permlane16_swap(a, a, false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
template <int ROT> __device__ __forceinline__ float sum_ror(float v) {      // + the lane ROT positions lower in the 16-lane row (cyclic)
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + ROT, 0xf, 0xf, false));
}
template <int LPR, typename Acc>
__device__ __forceinline__ Acc reduce_groups(Acc acc) {
    constexpr int C = sizeof(Acc) / sizeof(float);
#pragma unroll
    for (int i = 0; i < C; i++) {
        float v = acc[i];
        if (LPR <= 32) v = sum_xor32(v);
        if (LPR <= 16) v = sum_xor16(v);
        if (LPR <= 8) v = sum_ror<8>(v);
        if (LPR <= 4) v = sum_ror<4>(v);
        acc[i] = v;
    }
    return acc;   // every lane group holds the full sum for its columns
}

// where a wave reads the (col,val) pairs of a row segment from: the CSR arrays (two 4-byte loads per
// entry) or the graph plan's packed stream (one 8-byte load)
struct CsrSrc {
    const int32_t *indices; const float *vals;
    __device__ __forceinline__ int2 at(int64_t i) const { return make_int2(indices[i], __float_as_int(vals[i])); }
};
struct PackedSrc {
    const int2 *pk;
    __device__ __forceinline__ int2 at(int64_t i) const { return pk[i]; }
};

// the staged weight of an entry of row `row` under edge dropout: val / keep_prob (as val * inv) or zero; returns whether it lives
__device__ __forceinline__ bool drop_apply(const DropArgs &d, int row, int2 &cv) {
    const bool live = drop_live(d, row, cv.x);
    cv.y = live ? __float_as_int(__int_as_float(cv.y) * d.inv) : 0;
    return live;
}

// DROP: edge dropout is on (src.dr); `row` is the id of the row the segment belongs to (unused otherwise)
template <int D, typename TI, bool SPARSE, bool BIG, bool DROP = false, typename ES>
__device__ __forceinline__ typename Geo<D, TI, SPARSE>::Acc
row_gather(const ES &es, int64_t start, int64_t end, const GatherSrc &src, int lane, int2 *stage, int row = 0) {
    typedef Geo<D, TI, SPARSE> G;
    typename G::Acc acc = zerov<G::CPL>();
    tile_pad_init(stage, lane);
    // the next tile's (col,val) pairs are in flight while this tile gathers
    int2 cv = make_int2(0, 0);
    if (start + lane < end) cv = es.at(start + lane);
    for (int64_t base = start; base < end; base += 64) {
        const int n = (int)min((int64_t)64, end - base);
        if (!SPARSE && src.S) cv.y = __float_as_int(__int_as_float(cv.y) * src.S[cv.x]);     // fp8 table: weight x row scale of the column
        bool live = true;
        if constexpr (DROP) live = drop_apply(src.dr, row, cv);
        const int cnt = tile_stage<SPARSE>(cv.x, __int_as_float(cv.y), n, src, lane, stage, live);
        __builtin_amdgcn_wave_barrier();
        cv = make_int2(0, 0);
        if (base + 64 + lane < end) cv = es.at(base + 64 + lane);
        tile_gather<D, TI, SPARSE, BIG>(stage, cnt, src, lane, acc);
        __builtin_amdgcn_wave_barrier();
    }
    return reduce_groups<G::LPR>(acc);
}

// (The work plan of a graph -- its slices, long-row chunks and packed stream -- with LongPlan, SlicePlan, SpmmArgs and the M_* mode
//  bits of k_spmm: lgcn_kernels.h, beside the constants the plan builder reads.)
// Adam's operands of one row piece, fetched under the LAST gather batch of a pack (see pack_batch)
template <int C> struct AdamPre { typename VecF<C>::T p, m, v; bool have; };

// IL: the accumulators are the four interleaved chunks of an fp8 gather (see fp8_t): the fp32 rows are addressed chunk by chunk
template <int D, typename TO, int MODE, int C, bool IL = false>
__device__ __forceinline__ void spmm_epilogue(const SpmmArgs &a, int64_t row, int l, typename VecF<C>::T acc, bool flagged,
                                              const AdamPre<C> *pre = nullptr) {
    typedef typename VecF<C>::T V;
    const int64_t off = row * D + l * C;
    if (MODE & M_ADDSELF) acc = row_load<D, C, IL>(a.selfX, row, l) + acc;
    if (MODE & M_WTS) acc = a.w_in * acc;
    if ((MODE & M_ADDG) && flagged) {      // (the row's bitmap word was fetched before the gathers -- a dependent load here measured +0.3-0.6 % on the step)
        V g = row_load<D, C, IL>(a.G32, row, l);          // = (float)(G64 * 2^-50) / (K+1), converted once by k_g32
        if (MODE & M_WTS) g = a.w_add * g;               // (there G32 is G unscaled)
        acc = g + acc;
        if ((MODE & M_ADAM) && !(MODE & M_SPARSE) && a.clear) {      // consumed: leave the workspace clean
            // (the bitmap is NOT cleared here: an atomic on words that every row's epilogue reads keeps
            //  dropping those lines from L2 -- measured +22 us; the two bitmaps alternate per step and
            //  k_triplet of the next step zeroes the stale one with plain stores)
            if constexpr (IL) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    i64x2 *q = reinterpret_cast<i64x2 *>(a.G64 + row * D + (j * (D / 16) + l) * 4);
                    q[0] = i64x2{0, 0}; q[1] = i64x2{0, 0};
                }
            } else {
                i64x2 *q = reinterpret_cast<i64x2 *>(a.G64 + off);
#pragma unroll
                for (int i = 0; i < C / 2; i++) q[i] = i64x2{0, 0};
            }
        }
    }
    if (MODE & M_ADAM) {
        V p, m, v;
        if (pre && pre->have) { p = pre->p; m = pre->m; v = pre->v; }
        else { p = row_load<D, C, IL>(a.P, row, l); m = row_load<D, C, IL>(a.M, row, l); v = row_load<D, C, IL>(a.V, row, l); }
        if ((MODE & M_ADDG) && a.cnt && flagged) {
            // upstream LightGCN's L2 term (cfg.reg_ego): d(decay * reg)/dE0[row] = decay/B * (slots naming the row) * E0[row],
            // added to the propagated gradient here, where E0[row] is in registers anyway
            const int n_slots = a.cnt[row];
            acc = acc + (a.lam * (float)n_slots) * p;
            if (l == 0) a.cnt[row] = 0;                 // consumed (all lanes of the row belong to this wave: read before write)
        }
        m = m + a.w1 * (acc - m);                       // exp_avg.lerp_(grad, 1-beta1)
        v = v * a.beta2 + (a.omb2 * acc) * acc;         // mul_(beta2).addcmul_(g,g,1-beta2)
        V denom;
#pragma unroll
        for (int i = 0; i < C; i++) denom[i] = sqrtf(v[i]) / a.bc2_sqrt + a.eps;
        p = p - a.step_size * (m / denom);              // addcdiv_(exp_avg, denom, -step_size)
        // M and V are read next by this epilogue of the next step, P (where a shadow is gathered in its place) by that and by the
        // batch rows: under a.wt they go write-through.  The shadows are gathered with slice affinity and stay plain
        row_store<D, C, IL>(a.P, row, l, p, (a.wt & LGCN_STORE_ARG_P) != 0);
        row_store<D, C, IL>(a.M, row, l, m, (a.wt & LGCN_STORE_ARG_MV) != 0); row_store<D, C, IL>(a.V, row, l, v, (a.wt & LGCN_STORE_ARG_MV) != 0);
        // (a sparse-input launch that feeds Adam is the whole backward of K = 1: no forward layer, so no shadow -- lgcn_spmm_launch
        //  refuses one; the four pointer registers pay for the store field in the instantiations that sit at a register boundary)
        if constexpr (!(MODE & M_SPARSE)) {
            if (a.Pb) storev<C>(a.Pb + off, p);          // (bf16 shadow: only with bf16 tables, never IL)
            if (a.Pq) store_row_fp8<D, C, IL>(a.Pq, a.n_rows, row, l, p);
        }
    } else {
        RowStore<D, C, TO, IL>::put(a.Y, a.n_rows, row, l, acc, (a.wt & LGCN_STORE_ARG_Y) != 0);
    }
}

// deterministic reduction of the per-triplet loss / reg terms by ONE wave (fixed strided
// partials, then an xor-shuffle tree): loss_out = {bpr + decay*reg, bpr, reg}   (model.py:168-173)
__device__ __forceinline__ void reduce_loss_wave(const float *terms, const float *gathered, int B, int shard,
                                                 int D, float decay, float *loss_out, int lane, float ent_coeff = 0.f, int64_t blk_in = 0) {
    // Every lane adds its terms b = lane, lane + 64, ... in that order (the order is part of the result).
    float fl = 0.f, fr = 0.f, fe = 0.f;
    if (ent_coeff != 0.f) {        // popularity gate: entropy of the 2B gates, one sum per triplet (model.py:176-181)
        if (!gathered) { for (int b = lane; b < B; b += 64) fe += terms[2 * B + b]; }
        else for (int b = lane; b < B; b += 64) fe += gathered[(int64_t)(b / shard) * blk_in + (int64_t)3 * shard * D + 2 * shard + b % shard];
    }
    if (!gathered) {
        // one GPU: the plain loop (deeper explicit batches made the launch it rides in slower: 3214-3278 steps/s at
        // B = 8192 for 32 ... 4 loads in flight, 3296 for this form)
#pragma unroll 8
        for (int b = lane; b < B; b += 64) { fl += terms[b]; fr += terms[B + b]; }
    } else {
        // data parallel: the terms of the GLOBAL batch lie in the ranks' blocks.  16 loads in flight: with one load per
        // round trip a 16 384-triplet batch (8 ranks) took 100 us and held the +Adam launch back (38 -> 108 us).
        // (r, i) = (block, position in it) of this lane's next term, advanced without divisions.
        constexpr int UL = 16;
        const int64_t blk = blk_in ? blk_in : (int64_t)3 * shard * D + 2 * shard;
        int r = lane / shard, i = lane % shard;
        for (int b0 = 0; b0 < B; b0 += 64 * UL) {
            float tl[UL], tr[UL];
#pragma unroll
            for (int u = 0; u < UL; u++) {
                const bool in = b0 + u * 64 + lane < B;
                const float *t = gathered + (in ? r : 0) * blk + (int64_t)3 * shard * D;      // past the end: a valid address, weight 0
                const int ii = in ? i : 0;
                tl[u] = t[ii]; tr[u] = t[shard + ii];
                i += 64;
                while (i >= shard) { i -= shard; r++; }
            }
#pragma unroll
            for (int u = 0; u < UL; u++) {
                const bool in = b0 + u * 64 + lane < B;
                fl += in ? tl[u] : 0.f; fr += in ? tr[u] : 0.f;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { fl += __shfl_xor(fl, off); fr += __shfl_xor(fr, off); fe += __shfl_xor(fe, off); }
    if (lane == 0) {
        const float bpr = -(fl / (float)B) - ent_coeff * (fe / (float)(2 * B));       // loss - coeff * entropy.mean()
        const float reg = (0.5f * fr) / (float)B;
        loss_out[0] = bpr + decay * reg; loss_out[1] = bpr; loss_out[2] = reg;
    }
}

// Y = [Gs +] A_hat X.  256-thread workgroups = 4 waves.  Block b works on slice b & 7 (b >> 3 -th
// block of it): first the slice's long-row chunks, one per wave, then its short rows.
//   M_SPARSE: X is Gs, read from the fixed-point table G64 for rows flagged in `bitmap`
#ifndef SPMM_MIN_WAVES
#define SPMM_MIN_WAVES 6      /* waves per SIMD the register allocation must allow (<= 80 VGPRs): a wave keeps up to
                                 NPW x 8 row gathers in flight, so residency is not what hides the latency */
#endif
#ifndef SPMM_MIN_WAVES_ADAM
#define SPMM_MIN_WAVES_ADAM 5    /* the fp32 +Adam variant holds P/M/V pieces across its last batch: 84 VGPRs */
#endif
#ifndef SPMM_ADAM_PREFETCH
#define SPMM_ADAM_PREFETCH 1   /* Adam's P/M/V of a short row are loaded under the pack's last gather batch */
#endif
#ifndef SPMM_U_SP
#define SPMM_U_SP 4           /* the same for the sparse first backward layer (few flagged neighbours per row) */
#endif
#ifndef SPMM_U
#define SPMM_U 8              /* gathers in flight per lane in the short-row path */
#endif
// One batch of U gathers of a lane group walking ITS OWN row: the next U of its entries, p[0], p[GPR], ... (GPR lane
// groups share a row and take alternate entries).  Past the row's end the staged row continues with zero-weight
// entries (written once per pack), so a gather costs its address, its load and its multiply-adds and nothing else
// (before: clamp, select, compare, select, LDS address and a 64-bit address per gathered row -- 9 of the 12 / 21 vector
// instructions per fp32 / bf16 gather; loads are unconditional either way: a predicated load makes hipcc wait).
template <int D, typename TI, bool SPARSE, int U, int GPR, bool PRE, bool BIG, int PC>
__device__ __forceinline__ void pack_batch(const int2 *p, const GatherSrc &src, int l,
                                           typename Geo<D, TI, SPARSE>::Acc &acc,
                                           const SpmmArgs *a, int64_t off, bool final_batch,
                                           AdamPre<PC> *pre) {
    typedef Raw<TI, SPARSE> R;
    int2 cv[U]; typename R::T xr[U];
#pragma unroll
    for (int u = 0; u < U; u++) cv[u] = p[u * GPR];
#pragma unroll
    for (int u = 0; u < U; u++) xr[u] = R::template load<BIG>(src, cv[u].x, D, l);
    if (PRE && final_batch && off >= 0) {       // the pack's last gathers are in flight: Adam's operands ride the same round trip
        pre->p = loadv<PC>(a->P + off); pre->m = loadv<PC>(a->M + off); pre->v = loadv<PC>(a->V + off);
        pre->have = true;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < U; u++) acc += __int_as_float(cv[u].y) * R::cvt(xr[u], src.div);
}

// rows per workgroup of a kernel variant: 4 waves x PACKS packs x NPW rows
#ifndef SPMM_WAVE_ROWS
#define SPMM_WAVE_ROWS 1      /* a wave walks packs one after the other until it has done this many rows (1: one pack per wave --
                                 measured: 4 -> 1 takes the d = 128 layer from 221 to 199 us; more, shorter waves win) */
#endif
#ifndef SPMM_WPB
#define SPMM_WPB 1            /* waves per workgroup (1, 2 or 4; the plan pads a slice's chunks to 4 and its rows to 64).  One-wave
                                 workgroups measured best: 4 -> 2 -> 1 = 5650 -> 5890 -> 5965 steps/s, dense layer 28.7 -> 27.5 -> 26.6 us */
#endif
template <int NPW> struct PackGeo { static constexpr int PACKS = NPW >= SPMM_WAVE_ROWS ? 1 : SPMM_WAVE_ROWS / NPW, RPW = NPW * PACKS, RPB = SPMM_WPB * RPW; };
// lane groups that share one short row.  A bf16 table row is 8 lanes wide, so 8 rows fit a wave -- but more,
// shorter waves are what this kernel wants (measured): two groups per bf16 row = 4 rows per wave like fp32.
#ifndef SPMM_GPR_BF16
#define SPMM_GPR_BF16 2
#endif
#ifndef SPMM_SCALAR_ROWINFO
#define SPMM_SCALAR_ROWINFO 1  /* a pack's row descriptors and bitmap words through the scalar cache instead of vector loads + readlane */
#endif
#ifndef SPMM_ADAM_SPLIT
#define SPMM_ADAM_SPLIT 1     /* bf16 tables: the two lane groups of a row share its Adam epilogue (see k_spmm) */
#endif
#ifndef SPMM_ADAM_PREFETCH_BF16
#define SPMM_ADAM_PREFETCH_BF16 0
#endif
#ifndef SPMM_GPR_F32
#define SPMM_GPR_F32 1
#endif
template <int D, typename TI, bool SP> struct RowGeo {
    static constexpr int NPW = Geo<D, TI, SP>::NPW;
    // (an fp8 row is D / 16 lanes wide: NPW / 4 groups per row keep 4 rows per wave at every d)
    static constexpr int WANT = SP ? 1 : (Geo<D, TI, SP>::CPL == 16 ? (NPW >= 4 ? NPW / 4 : 1) : Geo<D, TI, SP>::CPL == 8 ? SPMM_GPR_BF16 : SPMM_GPR_F32);
    static constexpr int GPR = NPW >= WANT ? WANT : NPW;
    static constexpr int RPK = NPW / GPR;          // rows of a pack
};
// v[lane] + v[lane ^ O], VALU only
template <int O> __device__ __forceinline__ float sum_xor(float v, int lane) {
    if (O == 32) return sum_xor32(v);
    if (O == 16) return sum_xor16(v);
    if (O == 8) return sum_ror<8>(v);
    // O == 4: row_ror moves data to HIGHER lanes (lane i receives lane i - n): the partner is 4 below or 4 above
    const float dn = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + 4, 0xf, 0xf, false));
    const float up = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x120 + 12, 0xf, 0xf, false));
    return v + ((lane & 4) ? dn : up);
}
// sum over the GPR lane groups of a row (groups LPR lanes apart): every one of them ends with the total
template <int LPR, int GPR> __device__ __forceinline__ float sum_row_groups(float v, int lane) {
    if (GPR >= 2) v = sum_xor<LPR>(v, lane);
    if (GPR >= 4) v = sum_xor<(2 * LPR > 32 ? 32 : 2 * LPR)>(v, lane);
    return v;
}

template <int D, typename TI, typename TO, int MODE, bool BIG, bool DROP = false>
// (fp8 tables: 16 accumulators per lane and, with Adam, 3 x 16 operands: a 128-register budget, 4 waves per SIMD)
// DROP: edge dropout (a.dr) -- a compile-time axis, so that the instantiations without it are what they were
__global__ void __launch_bounds__(64 * SPMM_WPB, sizeof(TI) == 1 ? 4 : ((MODE & M_ADAM) && sizeof(TI) == 4) ? SPMM_MIN_WAVES_ADAM : SPMM_MIN_WAVES) k_spmm(SpmmArgs a) {
    constexpr bool SP = (MODE & M_SPARSE) != 0;
    typedef Geo<D, TI, SP> G;
    typedef typename G::Acc Acc;
    typedef Raw<TI, SP> R;
    constexpr int LPR = G::LPR, NPW = G::NPW, C = G::CPL;
    constexpr bool IL = !SP && sizeof(TI) == 1;        // accumulators of an fp8 gather: chunk-interleaved columns
    constexpr int GPR = RowGeo<D, TI, SP>::GPR, RPK = RowGeo<D, TI, SP>::RPK;
    static_assert(GPR == 1 || GPR == 2 || GPR == 4, "one, two or four lane groups per row");
    static_assert(LPR * GPR <= 64 && (GPR == 1 || LPR >= 4), "lane groups of a row must fit the wave");
    constexpr int PACKS = PackGeo<RPK>::PACKS, RPW = PackGeo<RPK>::RPW, RPB = PackGeo<RPK>::RPB;
    // stage row stride (entries): a row's <= 64 entries + the zero-weight tail the deepest batch may read (3 per lane
    // group of the row); lane groups reading the same position of different rows hit different banks (76 * 2 mod 64 = 24)
    constexpr int ST = 76;
    static_assert(64 + 3 * GPR <= ST, "staged row + padding");
    constexpr int U = SP ? SPMM_U_SP : (C == 16 ? 4 : SPMM_U);      // fp8: 16 accumulators per lane; 4 x 16 B in flight per lane
    __shared__ int2 stage_lds[SPMM_WPB][(RPK * ST > TILE_ST ? RPK * ST : TILE_ST)];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    GatherSrc src;
    src.X = SP ? (const void *)a.G32 : a.X; src.bm = a.bitmap; src.div = a.div;
    src.S = (!SP && sizeof(TI) == 1) ? fp8_scales(a.X, a.n_rows, D) : nullptr;
    if constexpr (DROP) src.dr = a.dr;
    // (a per-workgroup LDS copy of the row bitmap -- 9 KiB on Gowalla -- was measured: no gain, the copy's
    //  own round trip per workgroup costs what the per-neighbour tests save once a pack's tests are batched)
    // (block 0 is dispatched first: the reduction overlaps the whole launch; on the last block it
    //  sat on the tail and cost +25 us)
    if ((MODE & M_ADAM) && !SP && a.clear && blockIdx.x == 0 && wid == SPMM_WPB - 1)
        reduce_loss_wave(a.terms, a.gathered, a.B, a.shard, D, a.decay, a.loss_out, lane, a.ent_coeff, a.blk);
    int x, j;
    if (a.remap) { x = blockIdx.x & (XCDS - 1); j = blockIdx.x >> 3; }
    else {        // slices as contiguous block ranges (placement-independent either way: speed only)
        x = 0; j = blockIdx.x;
        while (x < XCDS - 1) {
            const int nb = (a.sp.cblk[x + 1] - a.sp.cblk[x]) * (4 / SPMM_WPB) + (a.sp.rows[x + 1] - a.sp.rows[x]) / RPB;
            if (j < nb) break;
            j -= nb; x++;
        }
    }
    const int ncb = (a.sp.cblk[x + 1] - a.sp.cblk[x]) * (4 / SPMM_WPB);      // the plan counts groups of 4 chunks
    if (j < ncb) {
        // ---- one chunk of a long row, the whole wave on it ----
        const int c = a.sp.cblk[x] * 4 + j * SPMM_WPB + wid;
#if SPMM_SCALAR_ROWINFO
        // (the chunk's descriptor, its row and the row's bitmap word are wave-uniform plan data: scalar loads, as for the packs below)
        typedef int i32x4c_ __attribute__((ext_vector_type(4)));
        const i32x4c_ chv = ((const __attribute__((address_space(4))) i32x4c_ *)a.lp.chunks)[c];
        const int4 ch = make_int4(chv.x, chv.y, chv.z, chv.w);
        const int o = ch.x;
        if (o < 0) return;
        const int64_t row = ((const __attribute__((address_space(4))) int32_t *)a.lp.long_row)[o];
        const int nch = ((const __attribute__((address_space(4))) int32_t *)a.lp.long_nch)[o];
        const bool rflag = (MODE & M_ADDG) ? ((((const __attribute__((address_space(4))) uint32_t *)a.bitmap)[row >> 5] >> (row & 31)) & 1u) != 0u : false;
#else
        const int4 ch = a.lp.chunks[c];
        const int o = ch.x;
        if (o < 0) return;
        const int64_t row = a.lp.long_row[o];
        const int nch = a.lp.long_nch[o];
        const bool rflag = (MODE & M_ADDG) ? bit_set(a.bitmap, (int)row) : false;
#endif
        Acc acc = row_gather<D, TI, SP, BIG, DROP>(PackedSrc{a.pk}, ch.y, ch.z, src, lane, stage_lds[wid], (int)row);
        if (nch == 1) {                                   // LONG_T < nnz <= LONG_CH: one wave, no hand-off
            if (lane < LPR) spmm_epilogue<D, TO, MODE, C, IL>(a, row, lane, acc, rflag);
            return;
        }
        // Publish the partial WRITE-THROUGH (sc1: 8-byte agent-scope stores, no release fence -- a
        // release would write back this XCD's whole dirty L2, measured 2x on the launch), drain, take
        // a ticket; the last arriver invalidates its L1 once and reads the partials with sc1 loads
        // (cdna guide G16: R1 form with a counter, both the acquire AND the sc1-load variant).
        typedef __attribute__((address_space(1))) unsigned long long gu64;
        if (lane < LPR) {
            union { Acc v; unsigned long long q[C / 2]; } pk; pk.v = acc;
            gu64 *dst = (gu64 *)(a.lp.partials + (int64_t)c * D + lane * C);
#pragma unroll
            for (int i = 0; i < C / 2; i++) __hip_atomic_store(dst + i, pk.q[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        int ticket = 0;
        if (lane == 0) ticket = __hip_atomic_fetch_add(a.lp.counters + o, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ticket = __builtin_amdgcn_readfirstlane(ticket);
        if (ticket != nch - 1) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(a.lp.counters + o, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next launch
        if (lane >= LPR) return;
        const int first = c - ch.w;
        Acc tot = zerov<C>();
        for (int k = 0; k < nch; k++) {
            union { Acc v; unsigned long long q[C / 2]; } pk;
            gu64 *sp_ = (gu64 *)(a.lp.partials + (int64_t)(first + k) * D + lane * C);
#pragma unroll
            for (int i = 0; i < C / 2; i++) pk.q[i] = __hip_atomic_load(sp_ + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == 0) tot = pk.v; else tot += pk.v;
        }
        spmm_epilogue<D, TO, MODE, C, IL>(a, row, lane, tot, rflag);
        return;
    }
    // ---- short rows (<= 64 non-zeros): a pack of NPW rows at a time, ONE ROW PER LANE GROUP.  All
    //      index tiles of the pack are loaded back to back, then every group walks its own row U
    //      gathers deep: NPW x U row gathers in flight per wave (32 at d = 64 fp32, 64 with a bf16
    //      table) instead of one row's worth, no cross-group reduction, no divergence (the trip
    //      count is the pack's longest row; shorter rows pad with zero-weight re-reads of their
    //      last entry, and the plan sorts windows of rows by length so there is little to pad).
    //      A row is summed in CSR order by one accumulator chain -- the reference's own order.
    const int t = j - ncb;
    if (t >= (a.sp.rows[x + 1] - a.sp.rows[x]) / RPB) return;
    const int g = lane / LPR, l = lane % LPR;
    int2 *stage = stage_lds[wid];
#pragma unroll 1
    for (int pk = 0; pk < PACKS; pk++) {
        const int64_t pos0 = (int64_t)a.sp.rows[x] + (int64_t)t * RPB + (wid * PACKS + pk) * RPK;
        int off[RPK + 1];
        off[0] = 0;
#if SPMM_SCALAR_ROWINFO
        // The pack's row descriptors (row id, first entry, count) are the same for every lane and constant during the launch:
        // SCALAR loads (constant address space -> s_load_dwordx4), no vector-memory instruction and no readlane for them -- these
        // kernels are bound by the vector-memory instructions a CU retires (experiments.txt run 29-31).  The rows' bitmap words
        // likewise (k_spmm only reads the bitmap).
        typedef int i32x4_ __attribute__((ext_vector_type(4)));          // (a plain vector type: HIP's int4 is a class on the host pass)
        typedef const __attribute__((address_space(4))) i32x4_ *kint4p;
        typedef const __attribute__((address_space(4))) uint32_t *ku32p;
        const kint4p rip = (kint4p)(a.rowinfo + pos0);
        int row_s[RPK];
        int64_t base = 0;
#pragma unroll
        for (int r = 0; r < RPK; r++) {
            const i32x4_ ri = rip[r];
            row_s[r] = ri.x; off[r + 1] = off[r] + ri.z;
            if (r == 0) base = ri.y;
        }
        if (row_s[0] < 0) break;                                   // padding is at the end of a slice
        uint32_t fw_s[RPK];
#pragma unroll
        for (int r = 0; r < RPK; r++) fw_s[r] = ((MODE & M_ADDG) && row_s[r] >= 0) ? ((ku32p)a.bitmap)[row_s[r] >> 5] : 0u;
        const int tot = off[RPK];
#else
        // lane r < RPK fetches (row id, first entry, count) of row r with ONE 16-byte load from the plan
        int my_row = -1, my_s = 0, my_n = 0;
        if (lane < RPK) {
            const int4 ri = a.rowinfo[pos0 + lane];
            my_row = ri.x; my_s = ri.y; my_n = ri.z;
        }
        uint32_t my_fw = 0u;           // bitmap word of this lane's row, in flight under the stream loads
        if ((MODE & M_ADDG) && my_row >= 0) my_fw = a.bitmap[my_row >> 5];
        if (__builtin_amdgcn_readlane(my_row, 0) < 0) break;       // padding is at the end of a slice
#pragma unroll
        for (int r = 0; r < RPK; r++) off[r + 1] = off[r] + __builtin_amdgcn_readlane(my_n, r);
        const int tot = off[RPK];
        const int64_t base = __builtin_amdgcn_readlane(my_s, 0);
#endif
        // the pack's rows are contiguous in the stream: entry e of the pack belongs to the row r with
        // off[r] <= e < off[r+1]; whole 512-byte loads, all issued before the first is staged
        int2 cvr[RPK];
#pragma unroll
        for (int it = 0; it < RPK; it++) {
            cvr[it] = make_int2(0, 0);
            if (it * 64 < tot) { const int e = it * 64 + lane; if (e < tot) cvr[it] = a.pk[base + e]; }
        }
        const int myr = g / GPR, sub = g % GPR;      // this lane group's row of the pack, and its share of it
        int maxcnt = 0;
        if (!SP && sizeof(TI) == 1) {                // fp8 table: weight x row scale of the column (padding entries: column 0, weight 0)
#pragma unroll
            for (int it = 0; it < RPK; it++)
                if (it * 64 < tot) cvr[it].y = __float_as_int(__int_as_float(cvr[it].y) * src.S[cvr[it].x]);
        }
        // edge dropout: a lane learns the row of the entry it stages from the pack's prefix `off` (scalar registers), scales the
        // weight of a kept entry and zeroes a dropped one; the sparse form below also leaves a dropped entry out of its compaction
        bool live[RPK];
#pragma unroll
        for (int it = 0; it < RPK; it++) live[it] = true;
        if constexpr (DROP) {
#pragma unroll
            for (int it = 0; it < RPK; it++) {
                if (it * 64 < tot) {
                    const int e = it * 64 + lane;
#if SPMM_SCALAR_ROWINFO
                    int rid = row_s[0];
#pragma unroll
                    for (int k = 1; k < RPK; k++) rid = (e >= off[k]) ? row_s[k] : rid;
#else
                    int r = 0;
#pragma unroll
                    for (int k = 1; k < RPK; k++) r += (e >= off[k]) ? 1 : 0;
                    const int rid = __shfl(my_row, r);
#endif
                    live[it] = drop_apply(src.dr, rid, cvr[it]);
                }
            }
        }
        if (!SP) {
#pragma unroll
            for (int it = 0; it < RPK; it++) {
                if (it * 64 < tot) {
                    const int e = it * 64 + lane;
                    int r = 0;
#pragma unroll
                    for (int k = 1; k < RPK; k++) r += (e >= off[k]) ? 1 : 0;
                    int o_r = 0;
#pragma unroll
                    for (int k = 1; k < RPK; k++) o_r = (e >= off[k]) ? off[k] : o_r;
                    if (e < tot) stage[r * ST + (e - o_r)] = cvr[it];
                }
            }
#pragma unroll
            for (int r = 0; r < RPK; r++) maxcnt = max(maxcnt, (off[r + 1] - off[r] + GPR - 1) / GPR);
            // zero-weight tail of every row up to what the longest row's batches read (see pack_batch)
            const int padto = GPR * (maxcnt + 3);
#pragma unroll
            for (int r = 0; r < RPK; r++)
                for (int q = off[r + 1] - off[r] + lane; q < padto; q += 64) stage[r * ST + q] = make_int2(0, 0);
        } else {
            // keep only the neighbours whose row is flagged.  The bitmap words of ALL the pack's entries are
            // fetched in one round trip straight from the registers the stream landed in, and every entry is
            // staged at its compacted position in one pass: ballot, popcount of the flagged lanes below it
            // inside its own row's lane range, plus the row's count from the earlier 64-entry pieces (uniform).
            uint32_t w[RPK];
#pragma unroll
            for (int it = 0; it < RPK; it++) w[it] = (it * 64 < tot) ? src.bm[cvr[it].x >> 5] : 0u;      // col 0 past the end: valid
            int cntr[RPK];
#pragma unroll
            for (int r = 0; r < RPK; r++) cntr[r] = 0;
#pragma unroll
            for (int it = 0; it < RPK; it++) {
                if (it * 64 < tot) {
                    const int e = it * 64 + lane;
                    const bool flag = e < tot && live[it] && ((w[it] >> (cvr[it].x & 31)) & 1u);
                    const unsigned long long m = __ballot(flag);
                    int r = 0, o_r = 0, before = cntr[0];
#pragma unroll
                    for (int k = 1; k < RPK; k++) { const bool ge = e >= off[k]; r += ge ? 1 : 0; o_r = ge ? off[k] : o_r; before = ge ? cntr[k] : before; }
                    const int lo = max(o_r - it * 64, 0);                 // first lane of this lane's row in this piece (<= lane)
                    const unsigned long long below = m & ((1ull << lane) - 1ull) & ~((1ull << lo) - 1ull);
                    if (flag) stage[r * ST + before + __popcll(below)] = cvr[it];
#pragma unroll
                    for (int k = 0; k < RPK; k++) {
                        const int lk = min(max(off[k] - it * 64, 0), 64), hk = min(max(off[k + 1] - it * 64, 0), 64);
                        const unsigned long long mk = (hk >= 64 ? ~0ull : (1ull << hk) - 1ull) & ~(lk >= 64 ? ~0ull : (1ull << lk) - 1ull);
                        cntr[k] += __popcll(m & mk);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < RPK; r++) maxcnt = max(maxcnt, cntr[r]);
            const int padto = GPR * (maxcnt + 3);
#pragma unroll
            for (int r = 0; r < RPK; r++)
                for (int q = cntr[r] + lane; q < padto; q += 64) stage[r * ST + q] = make_int2(0, 0);
        }
        __builtin_amdgcn_wave_barrier();
        maxcnt = __builtin_amdgcn_readfirstlane(maxcnt);
        const int2 *mystage = stage + myr * ST + sub;
        Acc acc = zerov<C>();
        // batch depth follows the pack's longest row (8 / 4 / 2 / 1 gathers per lane): a padded gather costs
        // the address path as much as a useful one
#if SPMM_SCALAR_ROWINFO
        int mrow = row_s[0];
        uint32_t mfw = fw_s[0];
#pragma unroll
        for (int r = 1; r < RPK; r++) { mrow = myr == r ? row_s[r] : mrow; mfw = myr == r ? fw_s[r] : mfw; }
#else
        const int mrow = __shfl(my_row, myr);
        const uint32_t mfw = (MODE & M_ADDG) ? (uint32_t)__shfl((int)my_fw, myr) : 0u;
#endif
        // (fp32 tables only: with a bf16 table the kernel is already at its register budget and the operands spill --
        //  measured 6940 vs 7420 steps/s; fp32: 6339 vs 6306)
        //  with the two lane groups of a bf16 row sharing the epilogue -- SPLIT below -- the operands are 12 registers, not 24)
        constexpr bool SPLIT = SPMM_ADAM_SPLIT && (MODE & M_ADAM) != 0 && C == 8 && GPR == 2 && !IL;
        constexpr bool PRE = SPMM_ADAM_PREFETCH && (MODE & M_ADAM) != 0 && (sizeof(TI) == 4 || (SPLIT && SPMM_ADAM_PREFETCH_BF16));
        constexpr int PC = SPLIT ? 4 : C;
        AdamPre<PC> pre; pre.have = false;
        const int64_t poff = (PRE && mrow >= 0 && (SPLIT || sub == 0)) ? (int64_t)mrow * D + (SPLIT ? (2 * l + sub) * 4 : l * C) : -1;
        int u0 = 0;
#define PACK_BATCH(UU) pack_batch<D, TI, SP, UU, GPR, PRE, BIG, PC>(mystage + GPR * u0, src, l, acc, &a, poff, maxcnt - u0 <= UU, &pre)
        if (U >= 8) for (; maxcnt - u0 > 4; u0 += 8) PACK_BATCH((U >= 8 ? 8 : U));
        if (U >= 4) for (; maxcnt - u0 > 2; u0 += 4) PACK_BATCH((U >= 4 ? 4 : U));
        for (; maxcnt - u0 > 1; u0 += 2) PACK_BATCH(2);
        if (maxcnt - u0 > 0) PACK_BATCH(1);
#undef PACK_BATCH
        if (GPR > 1) {
#pragma unroll
            for (int i = 0; i < C; i++) acc[i] = sum_row_groups<LPR, GPR>(acc[i], lane);     // fixed order: bitwise reproducible
        }
        const bool mflag = (MODE & M_ADDG) ? ((mfw >> (mrow & 31)) & 1u) != 0u : false;
        if constexpr (SPLIT) {
            // bf16 table, Adam: both lane groups of the row hold its sums, so BOTH run the fp32 epilogue, group `sub`
            // on the 4-column chunk 2l + sub.  One float4 per operand and lane, whole 64-byte lines per instruction
            // (8 columns per lane = two instructions that each touch every line of the row and use half of it);
            // the same arithmetic per element, so the same bits.
            if (mrow >= 0) {
                const f32x4 h = sub ? f32x4{acc[4], acc[5], acc[6], acc[7]} : f32x4{acc[0], acc[1], acc[2], acc[3]};
                spmm_epilogue<D, TO, MODE, 4, false>(a, mrow, 2 * l + sub, h, mflag, PRE ? &pre : nullptr);
            }
        } else
        if (mrow >= 0 && sub == 0) spmm_epilogue<D, TO, MODE, C, IL>(a, mrow, l, acc, mflag, PRE ? &pre : nullptr);
        if (PACKS > 1) __builtin_amdgcn_wave_barrier();
    }
}

// out = (X_0 + X_1 + ... + X_{K-1} + out) / (K+1), `out` holding X_K on entry -- the stack + mean of
// computer() (model.py:221-222) as one streaming pass.  The K-th layer itself runs through k_spmm
// like the others, so evaluation gets the split long rows too.
// piece i (4 consecutive elements) of an [N,d] table of TI
template <typename TI> __device__ __forceinline__ f32x4 tab_load4(const void *tab, int64_t i, int d, int64_t N) { return load4((const TI *)tab + i * 4); }
template <> __device__ __forceinline__ f32x4 tab_load4<fp8_t>(const void *tab, int64_t i, int d, int64_t N) {
    const int64_t row = (i * 4) / d;
    const int w = *(const int *)((const char *)tab + row * d + fp8_byte_of_col((int)(i * 4 - row * d), d));      // a 4-column chunk is one aligned word
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8(w, false), b = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
    const float sc = ((const float *)((const char *)tab + N * d))[row];
    return f32x4{a[0] * sc, a[1] * sc, b[0] * sc, b[1] * sc};
}

template <typename TI, bool WTS = false>
__global__ void __launch_bounds__(256) k_layer_mean(MeanArgs a) {
    const float div = (float)(a.K + 1);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += (int64_t)gridDim.x * 256) {
        if constexpr (WTS) {         // the weighted combination, in the same layer order
            f32x4 s = a.w[0] * load4(a.X0 + i * 4);
            for (int k = 1; k < a.K; k++) s += a.w[k] * tab_load4<TI>(a.Xl[k], i, a.d, a.N);
            s += a.w[a.K] * load4(a.out + i * 4);
            store4(a.out + i * 4, s);
        } else {
            f32x4 s = load4(a.X0 + i * 4);
            for (int k = 1; k < a.K; k++) s += tab_load4<TI>(a.Xl[k], i, a.d, a.N);
            s += load4(a.out + i * 4);
            store4(a.out + i * 4, s / div);
        }
    }
}
void lgcn_layer_mean_launch(const MeanArgs &m, int act_dtype, bool wts, hipStream_t st) {
    const int64_t blocks = (m.n4 + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 2048 ? blocks : 2048);
    if (wts) {          // (no fp8 form: lgcn_propagate_weighted refuses it)
        if (act_dtype == LGCN_F32) hipLaunchKernelGGL((k_layer_mean<float, true>), dim3(grid), dim3(256), 0, st, m);
        else hipLaunchKernelGGL((k_layer_mean<bf16_t, true>), dim3(grid), dim3(256), 0, st, m);
    } else if (act_dtype == LGCN_F32) hipLaunchKernelGGL((k_layer_mean<float>), dim3(grid), dim3(256), 0, st, m);
    else if (act_dtype == LGCN_BF16) hipLaunchKernelGGL((k_layer_mean<bf16_t>), dim3(grid), dim3(256), 0, st, m);
    else hipLaunchKernelGGL((k_layer_mean<fp8_t>), dim3(grid), dim3(256), 0, st, m);
}

// bf16 copy of the parameter table: with bf16 activation storage (K >= 2) layer 1 gathers THIS instead of the fp32
// rows -- every SpMM input is then a 2-byte table.  Made at the start of a training call and kept current by the
// Adam epilogue (SpmmArgs::Pb) inside a multi-step call; evaluation (lgcn_propagate_mean) makes its own.
__global__ void __launch_bounds__(256) k_to_bf16(const float *src, bf16_t *dst, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
        store4(dst + i * 4, load4(src + i * 4));
}
// fp8 copy of an fp32 table (rows + row scales): the input of layer 1 with fp8 activation storage.  One lane group of
// d / 16 lanes per row (64 B read, 16 B written per lane).
template <int D>
__global__ void __launch_bounds__(256) k_to_fp8(const float *src, void *dst, int64_t n_rows) {
    constexpr int LPR = D / 16, RPB = 256 / LPR;
    const int l = threadIdx.x % LPR;
    const int64_t rows_pad = (n_rows + RPB - 1) / RPB * RPB;          // whole lane groups stay together (the shuffles need them)
    for (int64_t r = (int64_t)blockIdx.x * RPB + threadIdx.x / LPR; r < rows_pad; r += (int64_t)gridDim.x * RPB) {
        const int64_t row = r < n_rows ? r : n_rows - 1;
        const f32x16 v = row_load<D, 16, true>(src, row, l);          // the lane's four chunks j*L + l: coalesced float4 loads
        if (r < n_rows) store_row_fp8<D, 16, true>(dst, n_rows, row, l, v);
        else { float amax = 0.f; for (int o = 1; o < LPR; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o)); }   // (keep the group's shuffles matched)
    }
}
int lgcn_to_fp8_launch(const float *src, void *dst, int64_t n_rows, int d, hipStream_t st) {
    const int64_t blocks = (n_rows * (d / 16) + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 8192 ? (blocks > 0 ? blocks : 1) : 8192);
    switch (d) {
    case 64: hipLaunchKernelGGL((k_to_fp8<64>), dim3(grid), dim3(256), 0, st, src, dst, n_rows); return 0;
    case 128: hipLaunchKernelGGL((k_to_fp8<128>), dim3(grid), dim3(256), 0, st, src, dst, n_rows); return 0;
    case 256: hipLaunchKernelGGL((k_to_fp8<256>), dim3(grid), dim3(256), 0, st, src, dst, n_rows); return 0;
    }
    lgcn_set_error("fp8 storage needs an embedding dim of 64, 128 or 256");
    return 3;
}
void lgcn_to_bf16_launch(const float *src, bf16_t *dst, int64_t n, hipStream_t st) {
    const int64_t n4 = n / 4, blocks = (n4 + 255) / 256;
    hipLaunchKernelGGL(k_to_bf16, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, src, dst, n4);
}

// ---------------------------------------------------------------------------------
// BPR on the batch.
//
// k_triplet (default): ONE 256-thread workgroup per triplet does everything the batch needs from it:
//   the three slot rows e = mean_k X_k[row] (user, positive, negative item; the last layer
//   X_K[row] = (A_hat X_{K-1})[row] is gathered on the fly), then the loss terms and the three gradient
//   rows (triplet_loss_regs).  A row is cut into units of ROWS_UNIT_TILES 64-entry tiles; unit u of slot c
//   belongs to wave (c + u) mod 4: a typical triplet costs one unit per slot on waves 0-2 and wave 3 ends at
//   once, while a hub positive (sampled proportionally to popularity: 1000-neighbour rows are common) is
//   shared by all four waves.  Partial rows meet in LDS in a fixed order; wave 0 finishes the triplet.
//   (Round 1/2 history: one workgroup per SLOT + a loss launch = 24.6K waves of which 18K ended after reading
//   two indices; the launch skeleton alone -- ids, indptr, nothing else -- measured 7.3 of its 16.7 us, and
//   the slot rows made a round trip through HBM to the 6.7 us loss launch.)
// k_triplet_dense: the same when the last layer was propagated densely (cfg.dense_last).  (BprArgs: lgcn_kernels.h)
// ---------------------------------------------------------------------------------
__device__ __forceinline__ bool triplet_bad(const BprArgs &a, int b) {
    const int u = a.users[b], p = a.pos[b], n = a.neg[b];
    return u < 0 || u >= a.n_users || p < 0 || (int64_t)p + a.n_users >= a.N || n < 0 || (int64_t)n + a.n_users >= a.N;
}

// Loss terms and the three gradient rows of ONE triplet by one lane group.  Lane = column (mod 64): every
// load, store and atomic wave-instruction covers min(D,64) contiguous elements -- 512 contiguous bytes
// per 64-bit atomic instruction at d = 64.  (With 4 columns per lane the same atomics were 16 lanes x 8 B
// at a 32-byte stride and cost 9 of a 13.7 us kernel.)  x = e_u.e_p - e_u.e_n ; l = logsigmoid(x) ;
// r = |e_u|^2+|e_p|^2+|e_n|^2 ; gradient rows w.r.t. the propagated table -> fixed-point
// atomics into G64 + row flags (single GPU / dense DP) or the exchange block (DP rows).
template <int D>
__device__ __forceinline__ void triplet_finish(const BprArgs &a, int b, int l, const float *u, const float *p, const float *n,
                                               float ps, float ns, float rr);
// reg_ego: u0 / p0 / n0 = the slots' rows of the table itself; the L2 term is theirs and its gradient never enters G
// (the Adam epilogue adds it from the slot counts), so the gradient rows carry no lam term.
template <int D>
__device__ __forceinline__ void triplet_loss_regs(const BprArgs &a, int b, int l, const float *u, const float *p, const float *n,
                                                  const float *u0 = nullptr, const float *p0 = nullptr, const float *n0 = nullptr) {
    constexpr int LPT = D < 64 ? D : 64, CPL = D / LPT;
    float ps = 0.f, ns = 0.f, ru = 0.f, rp = 0.f, rn = 0.f;
    const bool ego = a.reg_ego != 0;
    const float lam = ego ? 0.f : a.lam;
#pragma unroll
    for (int j = 0; j < CPL; j++) {
        ps += u[j] * p[j]; ns += u[j] * n[j];
        const float ur = ego ? u0[j] : u[j], pr = ego ? p0[j] : p[j], nr = ego ? n0[j] : n[j];
        ru += ur * ur; rp += pr * pr; rn += nr * nr;
    }
    float rr = ru + rp + rn;
#pragma unroll
    for (int off = 1; off < LPT; off <<= 1) {
        ps += __shfl_xor(ps, off); ns += __shfl_xor(ns, off); rr += __shfl_xor(rr, off);
    }
    if (a.cols_phase == 1) {                    // column shard: rows + partial sums out, the all-reduce comes next
        const bool bad1 = triplet_bad(a, b);
        if (l == 0) { a.colsum[b] = bad1 ? 0.f : ps; a.colsum[a.B_local + b] = bad1 ? 0.f : ns; a.colsum[2 * a.B_local + b] = bad1 ? 0.f : rr; }
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            a.erows[((int64_t)0 * a.B_local + b) * D + j * LPT + l] = u[j];
            a.erows[((int64_t)1 * a.B_local + b) * D + j * LPT + l] = p[j];
            a.erows[((int64_t)2 * a.B_local + b) * D + j * LPT + l] = n[j];
        }
        return;
    }
    triplet_finish<D>(a, b, l, u, p, n, ps, ns, rr);
}

#ifndef FOLD_TICKET_ALL
#define FOLD_TICKET_ALL 0      /* the fold of k_g32: 0 = a row named by ONE slot of the batch is written to G32 directly (no G64 atomics,
                                  no ticket); 1 = every row goes through G64 and the ticket (A/B form: profiles/fold_g32/README.md) */
#endif
// The fold's hand-off for the rows of a triplet that m > 1 slots of the batch name (a.mult): this lane group has just added its
// three gradient rows (m[c] > 1: into G64[row]).  It drains those atomics ONCE and takes its tickets with ONE instruction -- lane
// c of the group adds 1 to the arrival counter of slot c's row -- so a triplet pays one drain and one atomic round trip however
// many of its rows are shared (one of each per slot was slower: the chain sits at the end of every workgroup; profiles/fold_g32/README.md).
// The group whose ticket on a row is m - 1 is the last one there; every other group's adds were drained before its own ticket,
// so it reads the complete fixed-point row (agent-scope loads behind an agent acquire: the hand-off of k_spmm's split rows, with
// atomics as the payload stores; the acquiring wave's own loads need no wait for the invalidate), converts it exactly as k_g32
// does and leaves the counter zero for the next step.  Nobody waits: a group that is not last just goes on.  A triplet whose
// positive and negative are one row takes two tickets on it (two lanes, two values).  The lane group is LPT lanes of one wave.
template <int D>
__device__ __forceinline__ void fold_close_rows(const BprArgs &a, const int64_t (&rows)[3], const int (&m)[3], int l) {
    constexpr int LPT = D < 64 ? D : 64, CPL = D / LPT, MIN_SHARED = FOLD_TICKET_ALL ? 1 : 2;
    typedef __attribute__((address_space(1))) unsigned long long gu64;
    if (m[0] < MIN_SHARED && m[1] < MIN_SHARED && m[2] < MIN_SHARED) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int ml = l == 0 ? m[0] : (l == 1 ? m[1] : m[2]);
    const int64_t rl = l == 0 ? rows[0] : (l == 1 ? rows[1] : rows[2]);
    int ticket = -1;
    if (l < 3 && ml >= MIN_SHARED) ticket = __hip_atomic_fetch_add(a.arrive + rl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool last[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int t = LPT == 64 ? __builtin_amdgcn_readlane(ticket, c) : __shfl(ticket, c, LPT);
        last[c] = m[c] >= MIN_SHARED && t == m[c] - 1;
    }
    if (!(last[0] || last[1] || last[2])) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    if (l < 3 && ml >= MIN_SHARED && ticket == ml - 1) __hip_atomic_store(a.arrive + rl, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // next step
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (!last[c]) continue;
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            const long long q = (long long)__hip_atomic_load((gu64 *)(a.G64 + rows[c] * D + j * LPT + l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.G32[rows[c] * D + j * LPT + l] = (float)((double)q * FIXED_INV) / a.gdiv;
        }
    }
}

// loss terms + the three gradient rows of one triplet from its slot rows and its (complete) dot products
template <int D>
__device__ __forceinline__ void triplet_finish(const BprArgs &a, int b, int l, const float *u, const float *p, const float *n,
                                               float ps, float ns, float rr) {
    constexpr int LPT = D < 64 ? D : 64, CPL = D / LPT;
    const float lam = a.reg_ego ? 0.f : a.lam;
    const bool tbad = triplet_bad(a, b);        // an out-of-range id voids the whole triplet
    const float x = ps - ns;
    const float gb = tbad ? 0.f : -a.inv_B * sigmoid_neg_f(x);
    if (l == 0) {
        float *lt = a.exchange ? a.contrib + (int64_t)3 * a.shard * D : a.terms + a.terms_off;
        const int stride = a.exchange ? a.shard : a.terms_stride;
        lt[b] = tbad ? 0.f : logsigmoid_f(x);
        lt[stride + b] = tbad ? 0.f : rr;
    }
    if (tbad && !a.exchange) return;
    const int64_t rows[3] = {(int64_t)a.users[b], (int64_t)a.pos[b] + a.n_users, (int64_t)a.neg[b] + a.n_users};
    int mm[3] = {0, 0, 0};
    if (a.mult) {
#pragma unroll
        for (int c = 0; c < 3; c++) mm[c] = (int)a.mult[c * a.B_local + b];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        // the fold of k_g32: m = slots of the batch naming this row (0: no fold, the row is converted by k_g32).  A row that
        // only this slot names is complete with this one term: its fp32 copy is the one-term sum's, bit for bit
        const int m = mm[c];
        const bool direct = !FOLD_TICKET_ALL && m == 1;
#pragma unroll
        for (int j = 0; j < CPL; j++) {
            float g = c == 0 ? gb * (p[j] - n[j]) + lam * u[j] : (c == 1 ? gb * u[j] + lam * p[j] : (-gb) * u[j] + lam * n[j]);
            if (a.G64 && !tbad) {
                const long long q = __double2ll_rn((double)g * FIXED_SCALE);
                if (direct) a.G32[rows[c] * D + j * LPT + l] = (float)((double)q * FIXED_INV) / a.gdiv;
                else atomicAdd((unsigned long long *)(a.G64 + rows[c] * D + j * LPT + l), (unsigned long long)q);
            }
            if (a.exchange) a.contrib[((int64_t)c * a.shard + b) * D + j * LPT + l] = tbad ? 0.f : g;
        }
        if (a.G64 && !tbad && l == 0) {
            atomicOr(a.bitmap + (rows[c] >> 5), 1u << (rows[c] & 31));
            if (a.cnt) atomicAdd(a.cnt + rows[c], 1);
            if (a.item_bitmap && c > 0) { const int64_t it = rows[c] - a.n_users; atomicOr(a.item_bitmap + (it >> 5), 1u << (it & 31)); }
        }
    }
    if (a.G64 && !tbad && a.mult) fold_close_rows<D>(a, rows, mm, l);
}

#ifndef TRIPLET_MIN_WAVES
#define TRIPLET_MIN_WAVES 4    /* bf16 tables: a 64-VGPR cap spills (7290 vs 7610 steps/s); fp32 tables fit 64 without (8 workgroups per CU, +0.4 %) */
#endif
#ifndef TRIPLET_MIN_WAVES_F32
#define TRIPLET_MIN_WAVES_F32 7 /* fp32 tables: 72 registers without scratch; the 64-register budget of round 2 (8 workgroups per CU) spills 20 bytes
                                   since the gather offsets became 32-bit + SGPR base (k_triplet 20.0 -> 21.9 us) */
#endif
#ifndef TRIPLET_U
#define TRIPLET_U LGCN_GATHER_U   /* gathers in flight per lane in k_triplet */
#endif
#ifndef TRIPLET_WAVES
#define TRIPLET_WAVES 4        /* waves per k_triplet workgroup: 4 = three gathering waves + one that reads the lower layers' rows; 3 = every wave
                                  reads the lower-layer rows of its own slot before it gathers (more workgroups resident per CU) */
#endif
#ifndef TRIPLET_WAVES_BF16
#define TRIPLET_WAVES_BF16 3   /* bf16 tables: three (measured again in run 27: Gowalla bf16 8 312 / 8 260 -> 8 398 / 8 417 steps/s; fp32 tables
                                  6 572 / 6 523 vs 6 518 / 6 560: no difference, four stays) */
#endif
// waves per k_triplet workgroup for a table type
template <typename TI> struct TripletGeo { static constexpr int NW = sizeof(TI) == 2 ? TRIPLET_WAVES_BF16 : TRIPLET_WAVES; };
#ifndef ROWS_UNIT_TILES
#define ROWS_UNIT_TILES 2      /* 64-entry tiles per unit of a slot row */
#endif
// units u_first, u_first + NW, ... of the row [start, start + n): one wave's share of a slot row.  The next
// tile's (col,val) pairs are in flight while this tile gathers, across the unit boundaries too.
template <int D, typename TG, bool BIG, int NW, bool DROP = false, typename ES>
__device__ __forceinline__ typename Geo<D, TG, false>::Acc
units_gather(const ES &es, int64_t start, int n, int u_first, const GatherSrc &src, int lane, int2 *stage, int row = 0) {
    typedef Geo<D, TG, false> G;
    constexpr int UT = ROWS_UNIT_TILES;
    typename G::Acc acc = zerov<G::CPL>();
    const int ntiles = (n + 63) >> 6;
    int t = u_first * UT;
    if (t >= ntiles) return acc;
    int2 cv = make_int2(0, 0);
    if (t * 64 + lane < n) cv = es.at(start + t * 64 + lane);
    for (;;) {
        if (src.S) cv.y = __float_as_int(__int_as_float(cv.y) * src.S[cv.x]);      // fp8 table: weight x row scale of the column
        if constexpr (DROP) drop_apply(src.dr, row, cv);                            // edge dropout: scaled or zero weight
        const int cnt = tile_stage<false>(cv.x, __int_as_float(cv.y), min(64, n - t * 64), src, lane, stage);
        __builtin_amdgcn_wave_barrier();
        int tn = t + 1;
        if (tn % UT == 0) tn += (NW - 1) * UT;
        const bool more = tn < ntiles;
        cv = make_int2(0, 0);
        if (more && tn * 64 + lane < n) cv = es.at(start + tn * 64 + lane);
        tile_gather<D, TG, false, BIG, TRIPLET_U>(stage, cnt, src, lane, acc);
        __builtin_amdgcn_wave_barrier();
        if (!more) break;
        t = tn;
    }
    return reduce_groups<G::LPR>(acc);
}

// TG: type of the table the last layer gathers from (X_{K-1}; E0 itself when K == 1)
// WTS: layer weights (a.w) instead of the mean -- every form of a slot row takes them: the lower layers' rows as they are summed
// (spare wave or three-wave form), the gathered / hub last layer where wave 0 joins the parts
template <int D, typename TG, typename TI, bool BIG, bool DROP = false, bool WTS = false>
__device__ __forceinline__ void triplet_body(const BprArgs &a, const void *Xg, int2 *stage, float (*part)[TripletGeo<TI>::NW][D], float (*base)[D], float (*ego)[D]) {
    constexpr int NW = TripletGeo<TI>::NW;
    typedef Geo<D, TG, false> G;
    constexpr int C = G::CPL, LPR = G::LPR, UN = 64 * ROWS_UNIT_TILES;
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT;      // lane = column (mod 64) layout of the finishing steps
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.x;
    const bool bad = triplet_bad(a, b);                 // an out-of-range id voids the whole triplet (err flag; zero terms)
    if (bad && threadIdx.x == 0) atomicExch(a.err, 1);
    // everything below is wave-uniform (scalar registers)
    const int64_t row0 = bad ? 0 : (int64_t)a.users[b], row1 = bad ? 0 : (int64_t)a.pos[b] + a.n_users, row2 = bad ? 0 : (int64_t)a.neg[b] + a.n_users;
    const int st0 = a.indptr[row0], st1 = a.indptr[row1], st2 = a.indptr[row2];
    const int n0 = a.indptr[row0 + 1] - st0, n1 = a.indptr[row1 + 1] - st1, n2 = a.indptr[row2 + 1] - st2;
    // the K lower layers' rows of a slot, summed in layer order (lane = column)
    auto base_row = [&](int c) {
        const int64_t row = c == 0 ? row0 : (c == 1 ? row1 : row2);
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            const int col = j * LPT + lane;
            float s = a.X0[row * D + col];
            if (a.reg_ego) ego[c][col] = s;
            if constexpr (WTS) {
                s *= a.w[0];
                for (int k = 1; k < a.K; k++) s += a.w[k] * tab_elem<TI>(a.Xl[k], a.N, D, row, col);
            } else
                for (int k = 1; k < a.K; k++) s += tab_elem<TI>(a.Xl[k], a.N, D, row, col);
            base[c][col] = s;
        }
    };
    if (NW == 4 && w == 3 && lane < LPT) {              // the spare wave does all three while waves 0-2 gather
#pragma unroll
        for (int c = 0; c < 3; c++) base_row(c);
    }
    GatherSrc src; src.bm = nullptr; src.div = 1.f; src.X = Xg;
    src.S = sizeof(TG) == 1 ? fp8_scales(Xg, a.N, D) : nullptr;
    if constexpr (DROP) src.dr = a.dr;
    tile_pad_init(stage, threadIdx.x & 63);
    bool any = NW == 3 || (w == 0 || w == 3);
#pragma unroll 1
    for (int c = 0; c < 3; c++) {                       // (not unrolled: three inlined copies of the gather loop cost 20 VGPRs)
        const int stc = c == 0 ? st0 : (c == 1 ? st1 : st2), nc = c == 0 ? n0 : (c == 1 ? n1 : n2);
        const int u0 = NW == 4 ? ((w - c + 4) & 3) : ((w - c + 3) % 3), units = (a.hub_nnz && nc > a.hub_nnz) ? 0 : (nc + UN - 1) / UN;      // a hub row: computed by the hub plan
        if (u0 < units) {
            const typename G::Acc x = units_gather<D, TG, BIG, NW, DROP>(CsrSrc{a.indices, a.vals}, stc, nc, u0, src, lane, stage,
                                                                         (int)(c == 0 ? row0 : (c == 1 ? row1 : row2)));
            if (lane < LPR) {
                if constexpr (sizeof(TG) == 1) {       // an fp8 gather: the lane's values are the chunks j*LPR + lane (see fp8_t)
#pragma unroll
                    for (int j = 0; j < 4; j++) store4(&part[c][w][(j * LPR + lane) * 4], f32x4{x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]});
                } else storev<C>(&part[c][w][lane * C], x);
            }
            any = true;
        }
    }
    if (NW == 3 && lane < LPT) base_row(w);             // three-wave form: wave w owns slot w's lower-layer rows (behind its gathers)
    if (!any) return;                  // s_barrier counts only the surviving waves
    __syncthreads();
    if (w != 0 || lane >= LPT) return;
    // wave 0: finish the three rows and the triplet
    const float div = (float)(a.K + 1);
    float e[3][CPT];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int nc = c == 0 ? n0 : (c == 1 ? n1 : n2);
        const bool hub = a.hub_nnz && nc > a.hub_nnz;
        const int units = hub ? 0 : (nc + UN - 1) / UN;
        const int64_t rowc = c == 0 ? row0 : (c == 1 ? row1 : row2);
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            const int col = j * LPT + lane;
            float xk = hub ? a.Xhub[rowc * D + col] : 0.f;
#pragma unroll
            for (int i = 0; i < NW; i++) if (i < units) xk += part[c][(c + i) % NW][col];     // unit 0's wave first
            if constexpr (WTS) e[c][j] = base[c][col] + a.w[a.K] * xk;
            else e[c][j] = (base[c][col] + xk) / div;
        }
    }
    if (a.reg_ego) {
        float e0[3][CPT];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
            for (int j = 0; j < CPT; j++) e0[c][j] = ego[c][j * LPT + lane];
        triplet_loss_regs<D>(a, b, lane, e[0], e[1], e[2], e0[0], e0[1], e0[2]);
    } else triplet_loss_regs<D>(a, b, lane, e[0], e[1], e[2]);
}

template <int D, typename TI, bool BIG, bool DROP = false, bool WTS = false>
__global__ void __launch_bounds__(64 * TripletGeo<TI>::NW, sizeof(TI) == 4 ? TRIPLET_MIN_WAVES_F32 : TRIPLET_MIN_WAVES) k_triplet(BprArgs a) {
    constexpr int NW = TripletGeo<TI>::NW;
    __shared__ int2 stage_lds[NW][TILE_ST];
    __shared__ __attribute__((aligned(32))) float part_lds[3][NW][D];
    __shared__ float base_lds[3][D];
    __shared__ float ego_lds[3][D];          // reg_ego: the slots' rows of the table itself
    // last step's row bitmap is dead: zero it here with plain stores (the two bitmaps alternate per step)
    for (int64_t i = (int64_t)blockIdx.x * (64 * NW) + threadIdx.x; i < a.bitmap_words; i += (int64_t)gridDim.x * (64 * NW))
        a.stale_bitmap[i] = 0u;
    int2 *stage = stage_lds[threadIdx.x >> 6];
    if (a.K == 1) triplet_body<D, float, TI, BIG, DROP, WTS>(a, a.X0, stage, part_lds, base_lds, ego_lds);
    else triplet_body<D, TI, TI, BIG, DROP, WTS>(a, a.Xl[a.K - 1], stage, part_lds, base_lds, ego_lds);
}

// The same when the last layer was propagated densely (cfg.dense_last): e = mean_k X_k[row] is K+1 row reads per slot,
// so one lane group (lane = column mod 64) does a whole triplet: 3 x (K+1) coalesced row reads, loss, atomics.  On graphs
// whose positives concentrate on hub items (a popularity-weighted mean item degree in the thousands: the synthetic Yelp /
// Amazon shapes) the slots together hold several times the graph's non-zeros -- one more dense SpMM is then far cheaper
// than per-slot gathers (236 -> ~50 us at B = 8192).  (Until run 56 this was two launches with the slot rows in HBM between.)
template <int D, typename TI, bool WTS = false>
__global__ void __launch_bounds__(256) k_triplet_dense(BprArgs a) {
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT, TPB = 256 / LPT;     // lanes per triplet, triplets per workgroup
    // last step's row bitmap is dead: zero it here with plain stores (the two bitmaps alternate per step)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.bitmap_words; i += (int64_t)gridDim.x * 256)
        a.stale_bitmap[i] = 0u;
    const int b = blockIdx.x * TPB + threadIdx.x / LPT, l = threadIdx.x % LPT;
    if (b >= a.B_local) return;                 // whole lane groups leave together
    const bool bad = triplet_bad(a, b);
    if (bad && l == 0) atomicExch(a.err, 1);
    const int64_t rows[3] = {bad ? 0 : (int64_t)a.users[b], bad ? 0 : (int64_t)a.pos[b] + a.n_users, bad ? 0 : (int64_t)a.neg[b] + a.n_users};
    const float div = (float)(a.K + 1);
    float e[3][CPT], e0[3][CPT];
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            const int64_t o = rows[c] * D + j * LPT + l;
            float s = a.X0[o];
            e0[c][j] = s;
            if constexpr (WTS) {        // layer weights: e = sum_k w[k] X_k[row]
                s *= a.w[0];
                for (int k = 1; k <= a.K; k++) s += a.w[k] * tab_elem<TI>(a.Xl[k], a.N, D, rows[c], j * LPT + l);
                e[c][j] = s;
            } else {
                for (int k = 1; k <= a.K; k++) s += tab_elem<TI>(a.Xl[k], a.N, D, rows[c], j * LPT + l);
                e[c][j] = s / div;
            }
        }
    }
    triplet_loss_regs<D>(a, b, l, e[0], e[1], e[2], e0[0], e0[1], e0[2]);
}

// Column-sharded step, after the all-reduce of the partial sums: one lane group per triplet reads its three slot rows (this rank's
// columns) and the COMPLETE scores / reg term, writes the loss terms and scatters the gradient rows of its columns.
template <int D>
__global__ void __launch_bounds__(256) k_cols_finish(BprArgs a) {
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT, TPB = 256 / LPT;
    const int b = blockIdx.x * TPB + threadIdx.x / LPT, l = threadIdx.x % LPT;
    if (b >= a.B_local) return;
    float e[3][CPT];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int j = 0; j < CPT; j++) e[c][j] = a.erows[((int64_t)c * a.B_local + b) * D + j * LPT + l];
    triplet_finish<D>(a, b, l, e[0], e[1], e[2], a.colsum[b], a.colsum[a.B_local + b], a.colsum[2 * a.B_local + b]);
}

// The instantiations of the batch-row launch for one width and table type.  The holes are the launcher's: an fp8 table has no
// DROP and no WTS form, WTS and DROP never meet (the setters refuse the pair; WTS comes first), the dense form has neither a
// BIG nor a DROP axis.
template <int D, typename TI, bool DROP, bool WTS>
static void launch_triplet_gathered(const BprArgs &a, bool big, hipStream_t st) {
    const dim3 grid(a.B_local), block(64 * TripletGeo<TI>::NW);
    if (big) hipLaunchKernelGGL((k_triplet<D, TI, true, DROP, WTS>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_triplet<D, TI, false, DROP, WTS>), grid, block, 0, st, a);
}
template <int D, typename TI>
static void launch_triplet_t(const BprArgs &a, bool wts, bool big, hipStream_t st) {
    constexpr bool AXES = sizeof(TI) != 1;          // fp8: the plain instantiations only
    if (a.dense_last) {
        constexpr int tpb = 256 / (D < 64 ? D : 64);
        const dim3 grid((unsigned)((a.B_local + tpb - 1) / tpb));
        if constexpr (AXES) if (wts) { hipLaunchKernelGGL((k_triplet_dense<D, TI, true>), grid, dim3(256), 0, st, a); return; }
        hipLaunchKernelGGL((k_triplet_dense<D, TI>), grid, dim3(256), 0, st, a);
        return;
    }
    if constexpr (AXES) {
        if (wts) return launch_triplet_gathered<D, TI, false, true>(a, big, st);
        if (a.dr.on) return launch_triplet_gathered<D, TI, true, false>(a, big, st);      // edge dropout: the last layer's gathers take the step's mask
    }
    launch_triplet_gathered<D, TI, false, false>(a, big, st);
}
int lgcn_triplet_launch(const BprArgs &a, int d, int act_dtype, bool wts, bool big, hipStream_t st) {
    DISPATCH_D(d, {
        if (a.cols_phase == 2) {      // column shard, after the all-reduce: loss terms + gradient scatter from the stored slot rows
            const int tpb = 256 / (D < 64 ? D : 64);
            hipLaunchKernelGGL((k_cols_finish<D>), dim3((unsigned)((a.B_local + tpb - 1) / tpb)), dim3(256), 0, st, a);
        } else if (act_dtype == LGCN_FP8) {
            if constexpr (D >= 64) launch_triplet_t<D, fp8_t>(a, wts, big, st);
        } else if (act_dtype == LGCN_F32) launch_triplet_t<D, float>(a, wts, big, st);
        else launch_triplet_t<D, bf16_t>(a, wts, big, st);
    });
    return 0;
}

// ---------------------------------------------------------------------------------
// The fork's optional branches in the fused step.
//
// Popularity gate (model.py:66-96,139-157,176-181).  For an item i with propagated row e_i and popularity scalar s_i:
//     a      = relu(W1 s_i + b1)                      pop_mlp[0]: Linear(1, Hp)
//     pv     = W2 a + b2                               pop_mlp[2]: Linear(Hp, d)
//     h      = relu(V1 [e_i ; pv] + c1)                gate_mlp[0]: Linear(2d, Hg)
//     g      = sigmoid((V2 h + c2) / T)                gate_mlp[2]: Linear(Hg, 1)
//     f_i    = g e_i + (1 - g) pv                      the row bpr_loss scores with
//     loss   = bpr(u, f_p, f_n) - coeff * mean over the 2B gates of H(clamp(g, 1e-6, 1 - 1e-6))
// bpr_loss reads f only on the 2B item slots of the batch, so the gate and its backward run on those slots: one wave per
// triplet (lane = column for the row work, lane = hidden unit for the two MLPs), the MLP weights in LDS (V1 and W2 row
// padded by one float: conflict-free both for "lane = unit walks a row" and "lane = column walks a column"), the
// gradient rows w.r.t. e_u, e_p, e_n scattered with the same fixed-point atomics as k_triplet, and the parameter
// gradients summed in two deterministic stages: per workgroup over its slots (phase 2 below, fixed slot order),
// then over the workgroups in index order inside k_gate_adam, which also applies torch.optim.Adam to the MLP parameters.
// ---------------------------------------------------------------------------------
#define GATE_S (2 * GATE_TPB) /* item slots per workgroup */
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int D>
__global__ void __launch_bounds__(256) k_triplet_gate(GateArgs a) {
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT, D2 = 2 * D, V1S = D2 + 1;
    extern __shared__ __attribute__((aligned(16))) float gsm[];
    const int Hp = a.Hp, Hg = a.Hg, W2S = Hp + 1;
    // LDS carve-up
    float *V1p = gsm;                                  // [Hg][2d + 1]
    float *W2p = V1p + GATE_HMAX * V1S;                // [d][Hp + 1]
    float *W1 = W2p + D * (GATE_HMAX + 1);             // [Hp]
    float *b1 = W1 + GATE_HMAX, *b2 = b1 + GATE_HMAX;  // [Hp], [d]
    float *c1 = b2 + D, *V2 = c1 + GATE_HMAX;          // [Hg], [Hg]
    float *IN = V2 + GATE_HMAX;                        // [S][2d]  gate input [e ; pv]
    float *DH = IN + GATE_S * D2;                      // [S][Hmax] d loss / d (pre-activation of the gate's hidden layer)
    float *HR = DH + GATE_S * GATE_HMAX;               // [S][Hmax] relu(h)
    float *DPV = HR + GATE_S * GATE_HMAX;              // [S][d]   d loss / d pv
    float *AA = DPV + GATE_S * D;                      // [S][Hmax] relu(a)
    float *DA = AA + GATE_S * GATE_HMAX;               // [S][Hmax] d loss / d (pre-activation of the pop hidden layer)
    float *SC = DA + GATE_S * GATE_HMAX;               // [S] popularity scalar
    float *DLOG = SC + GATE_S;                         // [S] d loss / d logit
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < a.bitmap_words; i += (int64_t)gridDim.x * 256) a.stale_bitmap[i] = 0u;
    const int oW2 = 2 * Hp, ob2 = oW2 + D * Hp, oV1 = ob2 + D, oc1 = oV1 + Hg * D2, oV2 = oc1 + Hg, oc2 = oV2 + Hg;
    // (the weight copies are unrolled: with one load per round trip the 8 192 + 2 048 words took a third of the launch)
#pragma unroll 16
    for (int i = tid; i < Hg * D2; i += 256) V1p[(i / D2) * V1S + i % D2] = a.params[oV1 + i];
#pragma unroll 8
    for (int i = tid; i < D * Hp; i += 256) W2p[(i / Hp) * W2S + i % Hp] = a.params[oW2 + i];
    if (tid < Hp) { W1[tid] = a.params[tid]; b1[tid] = a.params[Hp + tid]; }
    for (int i = tid; i < D; i += 256) b2[i] = a.params[ob2 + i];
    if (tid < Hg) { c1[tid] = a.params[oc1 + tid]; V2[tid] = a.params[oV2 + tid]; }
    const float c2 = a.params[oc2];
    // records of slots that end up unused (batch tail, bad ids) must read as zero in phase 2
    for (int i = tid; i < GATE_S * GATE_HMAX; i += 256) { DH[i] = 0.f; HR[i] = 0.f; AA[i] = 0.f; DA[i] = 0.f; }
    for (int i = tid; i < GATE_S * D; i += 256) DPV[i] = 0.f;
    for (int i = tid; i < GATE_S * D2; i += 256) IN[i] = 0.f;
    if (tid < GATE_S) { SC[tid] = 0.f; DLOG[tid] = 0.f; }
    __syncthreads();
    // ---- phase 1: one wave per triplet
    for (int tt = w; tt < GATE_TPB; tt += 4) {
        const int b = blockIdx.x * GATE_TPB + tt;
        if (b >= a.B) break;
        const int iu = a.users[b], ip = a.pos[b], in_ = a.neg[b];
        const bool bad = iu < 0 || iu >= a.n_users || ip < 0 || (int64_t)ip + a.n_users >= a.N || in_ < 0 || (int64_t)in_ + a.n_users >= a.N;
        float *lt = a.exchange ? a.contrib + (int64_t)3 * a.shard * D : a.terms;
        const int lts = a.exchange ? a.shard : a.terms_stride;
        if (bad) {
            if (lane == 0) { atomicExch(a.err, 1); lt[b] = 0.f; lt[lts + b] = 0.f; lt[2 * lts + b] = 0.f; }
            if (a.exchange && lane < LPT)
                for (int c3 = 0; c3 < 3; c3++)
                    for (int j = 0; j < CPT; j++) a.contrib[((int64_t)c3 * a.shard + b) * D + j * LPT + lane] = 0.f;
            continue;
        }
        const bool col = lane < LPT;
        float u[CPT], e[2][CPT], pv[2][CPT], f[2][CPT], g[2], ent[2];
        const int item[2] = {ip, in_};
#pragma unroll
        for (int j = 0; j < CPT; j++) u[j] = col ? a.E[(int64_t)iu * D + j * LPT + lane] : 0.f;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int sidx = 2 * tt + q;
            const int64_t row = (int64_t)item[q] + a.n_users;
#pragma unroll
            for (int j = 0; j < CPT; j++) e[q][j] = col ? a.E[row * D + j * LPT + lane] : 0.f;
            const float sc = a.item_pop[item[q]];
            if (lane < Hp) AA[sidx * GATE_HMAX + lane] = fmaxf(W1[lane] * sc + b1[lane], 0.f);
            if (lane == 0) SC[sidx] = sc;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < CPT; j++) {
                const int c = j * LPT + lane;
                float acc = 0.f;
                if (col) {
                    acc = b2[c];
#pragma unroll 8
                    for (int k = 0; k < Hp; k++) acc += W2p[c * W2S + k] * AA[sidx * GATE_HMAX + k];
                }
                pv[q][j] = acc;
                if (col) { IN[sidx * D2 + c] = e[q][j]; IN[sidx * D2 + D + c] = acc; }
            }
            __builtin_amdgcn_wave_barrier();
            float hr = 0.f;
            if (lane < Hg) {
                float h = c1[lane];
#pragma unroll 16
                for (int c = 0; c < D2; c++) h += V1p[lane * V1S + c] * IN[sidx * D2 + c];       // (16 LDS reads in flight, one accumulator chain)
                hr = fmaxf(h, 0.f);
                HR[sidx * GATE_HMAX + lane] = hr;
            }
            const float logit = (wave_sum(lane < Hg ? V2[lane] * hr : 0.f) + c2) * a.inv_temp;
            g[q] = 1.f / (1.f + expf(-logit));                                 // torch.sigmoid
            const float gc = fminf(fmaxf(g[q], 1e-6f), 1.f - 1e-6f);           // torch.clamp(gates, 1e-6, 1 - 1e-6)
            ent[q] = -(gc * logf(gc) + (1.f - gc) * logf(1.f - gc));
#pragma unroll
            for (int j = 0; j < CPT; j++) f[q][j] = g[q] * e[q][j] + (1.f - g[q]) * pv[q][j];
        }
        // loss terms (model.py:168-173 on the fused rows)
        float ps = 0.f, ns = 0.f, rr = 0.f;
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            ps += u[j] * f[0][j]; ns += u[j] * f[1][j];
            rr += u[j] * u[j] + f[0][j] * f[0][j] + f[1][j] * f[1][j];
        }
        ps = wave_sum(ps); ns = wave_sum(ns); rr = wave_sum(rr);
        const float x = ps - ns;
        const float gb = -a.inv_B * sigmoid_neg_f(x);
        if (lane == 0) { lt[b] = logsigmoid_f(x); lt[lts + b] = rr; lt[2 * lts + b] = ent[0] + ent[1]; }
        // backward: user row
        const int64_t urow = iu;
#pragma unroll
        for (int j = 0; j < CPT; j++) {
            if (col) {
                const float du = gb * (f[0][j] - f[1][j]) + a.lam * u[j];
                if (a.G64) fixed_add(a.G64 + urow * D + j * LPT + lane, du);
                if (a.exchange) a.contrib[((int64_t)0 * a.shard + b) * D + j * LPT + lane] = du;
            }
        }
        if (a.G64 && lane == 0) atomicOr(a.bitmap + (urow >> 5), 1u << (urow & 31));
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int sidx = 2 * tt + q;
            const int64_t row = (int64_t)item[q] + a.n_users;
            float dF[CPT], part = 0.f;
#pragma unroll
            for (int j = 0; j < CPT; j++) {
                dF[j] = (q == 0 ? gb : -gb) * u[j] + a.lam * f[q][j];
                part += dF[j] * (e[q][j] - pv[q][j]);
            }
            const bool inside = g[q] > 1e-6f && g[q] < 1.f - 1e-6f;            // the clamp passes gradient only inside its range
            const float dent = inside ? a.ent_scale * (logf(g[q]) - logf(1.f - g[q])) : 0.f;
            const float dlogit = (wave_sum(part) + dent) * g[q] * (1.f - g[q]) * a.inv_temp;
            if (lane < Hg) DH[sidx * GATE_HMAX + lane] = HR[sidx * GATE_HMAX + lane] > 0.f ? dlogit * V2[lane] : 0.f;
            if (lane == 0) DLOG[sidx] = dlogit;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int j = 0; j < CPT; j++) {
                const int c = j * LPT + lane;
                float die = 0.f, dip = 0.f;
                if (col) {
#pragma unroll 8
                    for (int k = 0; k < Hg; k++) { const float dh = DH[sidx * GATE_HMAX + k]; die += V1p[k * V1S + c] * dh; dip += V1p[k * V1S + D + c] * dh; }
                }
                const float de = g[q] * dF[j] + die, dpv = (1.f - g[q]) * dF[j] + dip;
                if (col) {
                    DPV[sidx * D + c] = dpv;
                    if (a.G64) fixed_add(a.G64 + row * D + c, de);
                    if (a.exchange) a.contrib[((int64_t)(1 + q) * a.shard + b) * D + c] = de;
                }
            }
            if (a.G64 && lane == 0) {
                atomicOr(a.bitmap + (row >> 5), 1u << (row & 31));
                if (a.item_bitmap) atomicOr(a.item_bitmap + (item[q] >> 5), 1u << (item[q] & 31));
            }
            __builtin_amdgcn_wave_barrier();
            if (lane < Hp) {
                float da = 0.f;
#pragma unroll 16
                for (int c = 0; c < D; c++) da += W2p[c * W2S + lane] * DPV[sidx * D + c];
                DA[sidx * GATE_HMAX + lane] = AA[sidx * GATE_HMAX + lane] > 0.f ? da : 0.f;
            }
        }
    }
    __syncthreads();
    // ---- phase 2: this workgroup's parameter-gradient sums over its slots.  The two item slots of a triplet (2 tt, 2 tt + 1) are
    //      added in fp32 -- the same pair on every rank whatever the shard -- and each triplet's term enters the sum in fixed point:
    //      the total does not depend on which triplets share a workgroup or a rank (half the conversions of one per slot)
    long long *out = a.partials + (int64_t)blockIdx.x * a.P;
    auto fx = [](float v) { return __double2ll_rn((double)v * FIXED_SCALE); };
#define GATE_SUM(EXPR) _Pragma("unroll") for (int w2 = 0; w2 < GATE_S; w2 += 2) { float pr_; { const int sI = w2; pr_ = (EXPR); } { const int sI = w2 + 1; pr_ += (EXPR); } v += fx(pr_); }
    for (int i = tid; i < a.P; i += 256) {
        long long v = 0;
        if (i < Hp) { GATE_SUM(DA[sI * GATE_HMAX + i] * SC[sI]) }
        else if (i < oW2) { const int k = i - Hp; GATE_SUM(DA[sI * GATE_HMAX + k]) }
        else if (i < ob2) { const int c = (i - oW2) / Hp, k = (i - oW2) % Hp; GATE_SUM(DPV[sI * D + c] * AA[sI * GATE_HMAX + k]) }
        else if (i < oV1) { const int c = i - ob2; GATE_SUM(DPV[sI * D + c]) }
        else if (i < oc1) { const int jj = (i - oV1) / D2, c = (i - oV1) % D2; GATE_SUM(DH[sI * GATE_HMAX + jj] * IN[sI * D2 + c]) }
        else if (i < oV2) { const int jj = i - oc1; GATE_SUM(DH[sI * GATE_HMAX + jj]) }
        else if (i < oc2) { const int jj = i - oV2; GATE_SUM(DLOG[sI] * HR[sI * GATE_HMAX + jj]) }
        else { GATE_SUM(DLOG[sI]) }
        out[i] = v;
    }
#undef GATE_SUM
}
static size_t gate_lds_bytes(int D) {
    const size_t fl = (size_t)GATE_HMAX * (2 * D + 1) + (size_t)D * (GATE_HMAX + 1) + 2 * GATE_HMAX + D + 2 * GATE_HMAX
                    + (size_t)GATE_S * 2 * D + 2 * GATE_S * GATE_HMAX + (size_t)GATE_S * D + 2 * GATE_S * GATE_HMAX + 2 * GATE_S;
    return fl * sizeof(float);
}
int lgcn_gate_launch(const GateArgs &g, int d, hipStream_t st) {
    const unsigned grid = (unsigned)((g.B + GATE_TPB - 1) / GATE_TPB);
    const size_t lds = gate_lds_bytes(d);
    switch (d) {
    case 32: HIP_OK(hipFuncSetAttribute((const void *)k_triplet_gate<32>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
             hipLaunchKernelGGL((k_triplet_gate<32>), dim3(grid), dim3(256), lds, st, g); break;
    case 64: HIP_OK(hipFuncSetAttribute((const void *)k_triplet_gate<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
             hipLaunchKernelGGL((k_triplet_gate<64>), dim3(grid), dim3(256), lds, st, g); break;
    case 128: HIP_OK(hipFuncSetAttribute((const void *)k_triplet_gate<128>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
             hipLaunchKernelGGL((k_triplet_gate<128>), dim3(grid), dim3(256), lds, st, g); break;
    default: lgcn_set_error("popularity gate: embedding dim must be 32, 64 or 128"); return 3;
    }
    return 0;
}

// sum of the fixed-point partial sums (of the workgroups on one GPU; of the ranks' totals in the exchange blocks under data
// parallelism -- integer sums: any grouping gives the same bits) + torch.optim.Adam on the MLP parameters (same arithmetic as
// spmm_epilogue's); grad_out keeps the reduced gradient (tests, inspection)
__global__ void __launch_bounds__(256) k_gate_adam(GateAdamArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    long long q = 0;
    for (int q0 = 0; q0 < a.n_src; q0 += 32) {               // 32 loads in flight per round trip
        long long t[32];
#pragma unroll
        for (int u = 0; u < 32; u++) t[u] = q0 + u < a.n_src ? a.src[(int64_t)(q0 + u) * a.stride + i] : 0;
#pragma unroll
        for (int u = 0; u < 32; u++) q += t[u];
    }
    const float g = (float)((double)q * FIXED_INV);
    a.grad_out[i] = g;
    float m = a.m[i], v = a.v[i], p = a.params[i];
    m = m + a.w1 * (g - m);
    v = v * a.beta2 + (a.omb2 * g) * g;
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);
    a.params[i] = p; a.m[i] = m; a.v[i] = v;
}
// data parallel: this rank's total (sum of its workgroups' partial sums) into the tail of its exchange block
__global__ void __launch_bounds__(256) k_gate_rank_total(const long long *partials, int32_t n_part, int32_t P, long long *out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    long long q = 0;
    for (int w = 0; w < n_part; w++) q += partials[(int64_t)w * P + i];
    out[i] = q;
}
void lgcn_gate_adam_launch(const GateAdamArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_gate_adam, dim3((unsigned)((a.P + 255) / 256)), dim3(256), 0, st, a);
}
void lgcn_gate_rank_total_launch(const long long *partials, int32_t n_part, int32_t P, long long *out, hipStream_t st) {
    hipLaunchKernelGGL(k_gate_rank_total, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, partials, n_part, P, out);
}

// T = mean of the K+1 layers (the stack + mean of computer(), model.py:221-222): user rows to out_u, item rows to out_i
// (two destinations: with item-item smoothing the item block is an SpMM input and its result lands beside the users)
template <typename TI>
__global__ void __launch_bounds__(256) k_mean_layers(MeanSplitArgs a) {
    const float div = (float)(a.K + 1);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.n4; i += (int64_t)gridDim.x * 256) {
        f32x4 s = load4(a.X0 + i * 4);
        for (int k = 1; k <= a.K; k++) s += load4((const TI *)a.Xl[k] + i * 4);
        store4((i < a.n4_users ? a.out_u : a.out_i) + i * 4, s / div);
    }
}
// flag the rows [lo, hi) in a row bitmap (item-item smoothing makes every item row of Gs non-zero)
__global__ void __launch_bounds__(256) k_flag_range(uint32_t *bm, int64_t lo, int64_t hi) {
    const int64_t wlo = lo >> 5, whi = (hi + 31) >> 5;
    for (int64_t wd = wlo + (int64_t)blockIdx.x * 256 + threadIdx.x; wd < whi; wd += (int64_t)gridDim.x * 256) {
        uint32_t m = 0xffffffffu;
        if (wd == (lo >> 5)) m &= 0xffffffffu << (lo & 31);
        if (wd == (hi >> 5)) m &= (hi & 31) ? (0xffffffffu >> (32 - (hi & 31))) : 0u;
        if (m == 0xffffffffu) bm[wd] = m; else if (m) atomicOr(bm + wd, m);
    }
}
void lgcn_mean_layers_launch(const MeanSplitArgs &m, int act_dtype, hipStream_t st) {
    const int64_t blocks = (m.n4 + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 2048 ? blocks : 2048);
    if (act_dtype == LGCN_F32) hipLaunchKernelGGL((k_mean_layers<float>), dim3(grid), dim3(256), 0, st, m);
    else hipLaunchKernelGGL((k_mean_layers<bf16_t>), dim3(grid), dim3(256), 0, st, m);
}
void lgcn_flag_range_launch(uint32_t *bm, int64_t lo, int64_t hi, hipStream_t st) {
    const int64_t words = (hi + 31) / 32;         // (of the whole bitmap up to hi: 64 workgroups at the most)
    hipLaunchKernelGGL(k_flag_range, dim3((unsigned)((words + 255) / 256 < 64 ? (words + 255) / 256 : 64)), dim3(256), 0, st, bm, lo, hi);
}

// slot -> destination row of the global batch (-1: the slot's triplet has a bad id)
__device__ __forceinline__ int64_t slot_row(int c, int b, const int32_t *users, const int32_t *pos,
                                            const int32_t *neg, int32_t n_users, int64_t N) {
    const int u = users[b], p = pos[b], n = neg[b];
    if (u < 0 || u >= n_users || p < 0 || (int64_t)p + n_users >= N || n < 0 || (int64_t)n + n_users >= N) return -1;
    return c == 0 ? (int64_t)u : (int64_t)(c == 1 ? p : n) + n_users;
}

// DP: order-independent scatter of every rank's gradient rows into G64 (+ row flags)
template <int D>
__global__ void __launch_bounds__(256) k_scatter(SlotArgs a) {
    // lane = column (mod 64), like triplet_loss: every 64-bit atomic wave-instruction covers 512 contiguous bytes.
    // (4 columns per lane -- 16 lanes x 8 B at a 32-byte stride per instruction -- ran at 0.24 TB/s of added bytes:
    //  12.9 us per 2048 triplets, 84 us for an 8-rank batch.)
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT, SPB = 256 / LPT;
    const int s = blockIdx.x * SPB + threadIdx.x / LPT, l = threadIdx.x % LPT;
    if (s >= 3 * a.B) return;
    const int c = s / a.B, b = s % a.B;
    const int64_t row = slot_row(c, b, a.users, a.pos, a.neg, a.n_users, a.N);
    if (row < 0) return;
    const int r = b / a.shard, i = b % a.shard;
    if (r == a.skip_rank) return;
    const int64_t blk = a.blk ? a.blk : (int64_t)3 * a.shard * D + 2 * a.shard;
    const float *src = a.gathered + r * blk + ((int64_t)c * a.shard + i) * D;
#pragma unroll
    for (int j = 0; j < CPT; j++)
        fixed_add(a.G64 + row * D + j * LPT + l, src[j * LPT + l]);
    if (l == 0) {
        atomicOr(a.bitmap + (row >> 5), 1u << (row & 31));
        if (a.cnt) atomicAdd(a.cnt + row, 1);
        if (a.item_bitmap && c > 0) { const int64_t it = row - a.n_users; atomicOr(a.item_bitmap + (it >> 5), 1u << (it & 31)); }
    }
}

// Gs rows of the batch, once per step: G32[row] = (float)(G64[row] * 2^-50) / (K+1) for every slot's row, after
// ALL contributions are in (k_triplet / k_scatter / the all-reduce).  Slots that share a row write the same
// bytes.  The first backward layer gathers these 4-byte rows (and every Horner epilogue adds them) instead of
// converting the fixed-point rows per gathered copy.
template <int D>
__global__ void __launch_bounds__(256) k_g32(SlotArgs a) {
    constexpr int LPR = D / 4, SPB = 256 / LPR;
    const int s = blockIdx.x * SPB + threadIdx.x / LPR, l = threadIdx.x % LPR;
    if (s >= 3 * a.B) return;
    const int64_t row = slot_row(s / a.B, s % a.B, a.users, a.pos, a.neg, a.n_users, a.N);
    if (row < 0) return;
    store4(a.G32 + row * D + l * 4, loadv_fixed<4>(a.G64 + row * D + l * 4, a.div));
}

// Slot multiplicities of a whole multi-step call (the fold of k_g32 into k_triplet).  The call's triplets
// [0, T) are cut into consecutive batches of B (the last one shorter); for batch i of b_i triplets and its slot
// s = c * b_i + b, out[3 * i * B + s] = how many slots of THAT batch name slot s's destination row -- 0 for the three
// slots of a triplet with an out-of-range id (slot_row's rule, which is triplet_bad's).  It depends on the ids alone, so one
// launch ahead of the loop serves every step.  One workgroup per batch: an open-addressing hash (linear probing) of the
// batch's row ids in LDS, H slots of key + count with 3 * B <= 3/4 H, so every probe sequence ends within H steps.
__global__ void __launch_bounds__(SLOT_MULT_THREADS) k_slot_mult(SlotMultArgs a) {
    // One thread per triplet (tid, tid + 1024, ...): its three ids are one round trip and its three rows follow from them.  The
    // loops are NOT unrolled: the launch runs once per call with a cold instruction cache, and an unrolled body (four triplets
    // x three rows x two passes, 9 KB of code) took tens of microseconds per launch, as did a slot-by-slot walk with its twelve
    // dependent id reads (profiles/fold_g32/README.md); the second pass re-reads the ids, which are cache hits by then.
    extern __shared__ int32_t slot_mult_lds[];          // keys [H] (-1: empty) | counts [H]
    int32_t *keys = slot_mult_lds, *cnts = slot_mult_lds + a.H;
    const int64_t t0 = (int64_t)blockIdx.x * a.B;
    const int bn = (int)((a.T - t0) < a.B ? (a.T - t0) : a.B);
    const int32_t *users = a.users + t0, *pos = a.pos + t0, *neg = a.neg + t0;
    const uint32_t mask = (uint32_t)a.H - 1u;
    for (int i = threadIdx.x; i < a.H; i += SLOT_MULT_THREADS) { keys[i] = -1; cnts[i] = 0; }
    __syncthreads();
#pragma unroll 1
    for (int b = threadIdx.x; b < bn; b += SLOT_MULT_THREADS) {
        const int32_t r0 = (int32_t)slot_row(0, b, users, pos, neg, a.n_users, a.N);
        if (r0 < 0) continue;                            // a void triplet: none of its slots counts
        const int32_t r1 = pos[b] + a.n_users, r2 = neg[b] + a.n_users;
#pragma unroll 1
        for (int c = 0; c < 3; c++) {
            const int32_t row = c == 0 ? r0 : (c == 1 ? r1 : r2);
            uint32_t h = drop_fmix32((uint32_t)row) & mask;
            for (int probe = 0; probe < a.H; probe++, h = (h + 1u) & mask) {
                const int32_t old = atomicCAS(&keys[h], -1, row);
                if (old == -1 || old == row) { atomicAdd(&cnts[h], 1); break; }
            }
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int b = threadIdx.x; b < bn; b += SLOT_MULT_THREADS) {
        const int32_t r0 = (int32_t)slot_row(0, b, users, pos, neg, a.n_users, a.N);
        const int32_t r1 = pos[b] + a.n_users, r2 = neg[b] + a.n_users;
#pragma unroll 1
        for (int c = 0; c < 3; c++) {
            const int32_t row = c == 0 ? r0 : (c == 1 ? r1 : r2);
            int m = 0;
            if (r0 >= 0) {
                uint32_t h = drop_fmix32((uint32_t)row) & mask;
                for (int probe = 0; probe < a.H; probe++, h = (h + 1u) & mask)
                    if (keys[h] == row) { m = cnts[h]; break; }
            }
            a.out[3 * t0 + (int64_t)c * bn + b] = (uint16_t)m;
        }
    }
}
int lgcn_slot_mult_launch(const int32_t *users, const int32_t *pos, const int32_t *neg, int64_t T, int32_t B, int32_t n_users,
                          int64_t N, uint16_t *out, hipStream_t st) {
    SlotMultArgs a{};
    a.users = users; a.pos = pos; a.neg = neg; a.T = T; a.B = B; a.n_users = n_users; a.N = N; a.out = out; a.H = slot_mult_hash(B);
    const size_t lds = sizeof(int32_t) * 2 * (size_t)a.H;
    // (once per device, for the largest hash: the call sits on the host path ahead of the first launch of every folded call)
    static bool attr_set[64] = {};
    int dev = 0;
    HIP_OK(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        HIP_OK(hipFuncSetAttribute((const void *)k_slot_mult, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(int32_t) * 2 * SLOT_MULT_HMAX)));
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL(k_slot_mult, dim3((unsigned)((T + B - 1) / B)), dim3(SLOT_MULT_THREADS), lds, st, a);
    return 0;
}
// dense data-parallel form: flag the rows of the WHOLE global batch (every rank knows all ids), so the
// row bitmap needs no collective (RCCL has no bitwise-OR reduction)
__global__ void __launch_bounds__(256) k_flag_rows(SlotArgs a) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= 3 * a.B) return;
    const int64_t row = slot_row(s / a.B, s % a.B, a.users, a.pos, a.neg, a.n_users, a.N);
    if (row >= 0) {
        atomicOr(a.bitmap + (row >> 5), 1u << (row & 31));
        if (a.cnt) atomicAdd(a.cnt + row, 1);          // dense form: every rank counts the whole global batch itself (part 1 does not)
        if (a.item_bitmap && s >= a.B) { const int64_t it = row - a.n_users; atomicOr(a.item_bitmap + (it >> 5), 1u << (it & 31)); }
    }
}

// End of step: zero what the step touched (G64 rows, bitmap words of the batch rows);
// block 0 also reduces the per-triplet loss terms in a fixed order.
template <int D>
__global__ void __launch_bounds__(256) k_finish(SlotArgs a) {
    constexpr int LPR = D / 4, SPB = 256 / LPR;
    const int s = blockIdx.x * SPB + threadIdx.x / LPR, l = threadIdx.x % LPR;
    if (s < 3 * a.B) {
        const int c = s / a.B, b = s % a.B;
        const int64_t row = slot_row(c, b, a.users, a.pos, a.neg, a.n_users, a.N);
        if (row >= 0) {
                    i64x2 *q = reinterpret_cast<i64x2 *>(a.G64 + row * D + l * 4);
            q[0] = i64x2{0, 0}; q[1] = i64x2{0, 0};
            if (l == 0) { a.bitmap[row >> 5] = 0u; if (a.cnt) a.cnt[row] = 0; }
        }
    }
    // the same single-wave, fixed-order reduction as the fused finish of the last SpMM: identical bits
    if (blockIdx.x == 0 && threadIdx.x < 64)
        reduce_loss_wave(a.terms, a.gathered, a.B, a.shard, D, a.decay, a.loss_out, (int)threadIdx.x, a.ent_coeff, a.blk);
}
// k_scatter: one lane group of min(d, 64) lanes per slot; k_g32, k_finish: d / 4 lanes per slot
static unsigned scatter_grid(int d, int32_t B) {
    const int spb = 256 / (d < 64 ? d : 64);
    return (unsigned)((3 * (int64_t)B + spb - 1) / spb);
}
static unsigned slot_grid(int d, int64_t slots_per_sample, int32_t B) {
    const int spb = 256 / (d / 4);
    return (unsigned)((slots_per_sample * B + spb - 1) / spb);
}
int lgcn_scatter_launch(const SlotArgs &s, int d, hipStream_t st) {
    DISPATCH_D(d, hipLaunchKernelGGL((k_scatter<D>), dim3(scatter_grid(d, s.B)), dim3(256), 0, st, s));
    return 0;
}
int lgcn_g32_launch(const SlotArgs &s, int d, hipStream_t st) {
    DISPATCH_D(d, hipLaunchKernelGGL((k_g32<D>), dim3(slot_grid(d, 3, s.B)), dim3(256), 0, st, s));
    return 0;
}
int lgcn_finish_launch(const SlotArgs &s, int d, hipStream_t st) {
    DISPATCH_D(d, hipLaunchKernelGGL((k_finish<D>), dim3(slot_grid(d, 3, s.B)), dim3(256), 0, st, s));
    return 0;
}
void lgcn_flag_rows_launch(const SlotArgs &s, hipStream_t st) {
    hipLaunchKernelGGL(k_flag_rows, dim3((3 * s.B + 255) / 256), dim3(256), 0, st, s);
}

__global__ void __launch_bounds__(256) k_apply_perm(const int32_t *S, int cols, const int64_t *perm, int64_t T,
                                                   int32_t *users, int32_t *pos, int32_t *neg) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int64_t j = perm ? perm[t] : t;
    users[t] = S[j * cols]; pos[t] = S[j * cols + 1]; neg[t] = S[j * cols + 2];
}
void lgcn_apply_perm_launch(const int32_t *S, int cols, const int64_t *perm, int64_t T, int32_t *users, int32_t *pos, int32_t *neg,
                            hipStream_t st) {
    hipLaunchKernelGGL(k_apply_perm, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, S, cols, perm, T, users, pos, neg);
}

// Several negatives per positive (lgcn_train_step_multi): the slot kernels' siblings over the (2 + R) B slots of a
// batch of B samples.  Slot s = c * B + b: c = 0 the user, 1 the positive, 2 + r negative r, read from negs + r * neg_stride.
// The three-slot launches above receive what they always received.
// slot -> destination row (-1: the slot's sample has an out-of-range id among its 2 + R: the whole sample is void)
__device__ __forceinline__ int64_t slot_row_multi(const SlotArgsMulti &a, int c, int b) {
    const int u = a.s.users[b], p = a.s.pos[b];
    bool bad = u < 0 || u >= a.s.n_users || p < 0 || (int64_t)p + a.s.n_users >= a.s.N;
    int nc = 0;
    for (int r = 0; r < a.R; r++) {
        const int n = a.negs[(int64_t)r * a.neg_stride + b];
        bad = bad || n < 0 || (int64_t)n + a.s.n_users >= a.s.N;
        if (r == c - 2) nc = n;
    }
    if (bad) return -1;
    return c == 0 ? (int64_t)u : (int64_t)(c == 1 ? p : nc) + a.s.n_users;
}
template <int D>
__global__ void __launch_bounds__(256) k_g32_multi(SlotArgsMulti a) {
    constexpr int LPR = D / 4, SPB = 256 / LPR;
    const int64_t s = (int64_t)blockIdx.x * SPB + threadIdx.x / LPR;
    const int l = threadIdx.x % LPR;
    if (s >= (int64_t)(2 + a.R) * a.s.B) return;
    const int64_t row = slot_row_multi(a, (int)(s / a.s.B), (int)(s % a.s.B));
    if (row < 0) return;
    store4(a.s.G32 + row * D + l * 4, loadv_fixed<4>(a.s.G64 + row * D + l * 4, a.s.div));
}
template <int D>
__global__ void __launch_bounds__(256) k_finish_multi(SlotArgsMulti a) {
    constexpr int LPR = D / 4, SPB = 256 / LPR;
    const int64_t s = (int64_t)blockIdx.x * SPB + threadIdx.x / LPR;
    const int l = threadIdx.x % LPR;
    if (s < (int64_t)(2 + a.R) * a.s.B) {
        const int64_t row = slot_row_multi(a, (int)(s / a.s.B), (int)(s % a.s.B));
        if (row >= 0) {
            i64x2 *q = reinterpret_cast<i64x2 *>(a.s.G64 + row * D + l * 4);
            q[0] = i64x2{0, 0}; q[1] = i64x2{0, 0};
            if (l == 0) { a.s.bitmap[row >> 5] = 0u; if (a.s.cnt) a.s.cnt[row] = 0; }
        }
    }
    // the per-sample terms are scaled so that the three-slot step's reduction with 1 / B yields the loss (same wave, same order)
    if (blockIdx.x == 0 && threadIdx.x < 64)
        reduce_loss_wave(a.s.terms, nullptr, a.s.B, a.s.shard, D, a.s.decay, a.s.loss_out, (int)threadIdx.x, 0.f, 0);
}
int lgcn_g32_multi_launch(const SlotArgsMulti &s, int d, hipStream_t st) {
    DISPATCH_D(d, hipLaunchKernelGGL((k_g32_multi<D>), dim3(slot_grid(d, 2 + (int64_t)s.R, s.s.B)), dim3(256), 0, st, s));
    return 0;
}
int lgcn_finish_multi_launch(const SlotArgsMulti &s, int d, hipStream_t st) {
    DISPATCH_D(d, hipLaunchKernelGGL((k_finish_multi<D>), dim3(slot_grid(d, 2 + (int64_t)s.R, s.s.B)), dim3(256), 0, st, s));
    return 0;
}
__global__ void __launch_bounds__(256) k_apply_perm_multi(const int32_t *S, int cols, const int64_t *perm, int64_t T,
                                                         int32_t *users, int32_t *pos, int32_t *negs, int32_t R) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    const int64_t j = perm ? perm[t] : t;
    users[t] = S[j * cols]; pos[t] = S[j * cols + 1];
    for (int r = 0; r < R; r++) negs[(int64_t)r * T + t] = S[j * cols + 2 + r];
}
void lgcn_apply_perm_multi_launch(const int32_t *S, int cols, const int64_t *perm, int64_t T, int32_t *users, int32_t *pos,
                                  int32_t *negs, int32_t R, hipStream_t st) {
    hipLaunchKernelGGL(k_apply_perm_multi, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, st, S, cols, perm, T, users, pos, negs, R);
}

// column indices must address rows of X: flag any index outside [0, n_rows)
__global__ void __launch_bounds__(256) k_index_range(const int32_t *indices, int64_t nnz, int32_t n_rows, int32_t *bad) {
    bool b = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * 256) {
        const int32_t c = indices[i];
        b |= (c < 0 || c >= n_rows);
    }
    if (__ballot(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}
void lgcn_index_range_launch(const int32_t *indices, int64_t nnz, int32_t n_rows, int32_t *bad) {
    const int64_t blocks = (nnz + 255) / 256;
    hipLaunchKernelGGL(k_index_range, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, 0, indices, nnz, n_rows, bad);
}

// copy the planned rows' CSR segments into the packed stream: items = (first CSR entry, first stream entry, count, 0)
__global__ void __launch_bounds__(256) k_pack_stream(const int4 *items, int64_t n_items, const int32_t *indices,
                                                     const float *vals, int2 *pk) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t i = wave; i < n_items; i += nwaves) {
        const int4 it = items[i];
        for (int e = lane; e < it.z; e += 64)
            pk[(int64_t)it.y + e] = make_int2(indices[(int64_t)it.x + e], __float_as_int(vals[(int64_t)it.x + e]));
    }
}
void lgcn_pack_stream_launch(const int4 *items, int64_t n_items, const int32_t *indices, const float *vals, int2 *pk) {
    const int64_t blocks = (n_items + 3) / 4;
    hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, 0, items, n_items, indices, vals, pk);
}

// keep_out[p] = keep(row of p, indices[p]): one wave per row, its lanes over the row's entries
__global__ void __launch_bounds__(256) k_dropout_mask(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t nnz,
                                                      uint32_t k0, uint32_t k1, uint64_t thr, uint8_t *keep_out) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t row = wave; row < n_rows; row += nwaves) {
        const int64_t s = max((int64_t)indptr[row], (int64_t)0), e = min((int64_t)indptr[row + 1], nnz);      // never past the arrays
        for (int64_t p = s + lane; p < e; p += 64)
            keep_out[p] = (uint64_t)drop_hash(k0, k1, (uint32_t)row, (uint32_t)indices[p]) < thr ? 1 : 0;
    }
}
void lgcn_dropout_mask_launch(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t nnz, uint32_t k0, uint32_t k1,
                              uint64_t thr, uint8_t *keep_out, hipStream_t st) {
    const int64_t blocks = (n_rows + 3) / 4;
    hipLaunchKernelGGL(k_dropout_mask, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st,
                       indptr, indices, n_rows, nnz, k0, k1, thr, keep_out);
}

// ---------------------------------------------------------------------------------
// launch helpers
// ---------------------------------------------------------------------------------
template <int D, typename TI, typename TO, int MODE, bool DROP = false>
static void launch_spmm_t(const SpmmArgs &a, hipStream_t st) {
    constexpr int RPB = PackGeo<RowGeo<D, TI, (MODE & M_SPARSE) != 0>::RPK>::RPB;
    static_assert(SLICE_PAD % RPB == 0, "slice padding must hold whole workgroups of every variant");
    unsigned grid = 0, widest = 0;
    for (int x = 0; x < XCDS; x++) {
        const unsigned nb = (unsigned)((a.sp.cblk[x + 1] - a.sp.cblk[x]) * (4 / SPMM_WPB) + (a.sp.rows[x + 1] - a.sp.rows[x]) / RPB);
        grid += nb; widest = nb > widest ? nb : widest;
    }
    if (a.remap) grid = widest * XCDS;
    if (grid == 0) return;
    if (big_table(a.n_rows, D)) hipLaunchKernelGGL((k_spmm<D, TI, TO, MODE, true, DROP>), dim3(grid), dim3(64 * SPMM_WPB), 0, st, a);
    else hipLaunchKernelGGL((k_spmm<D, TI, TO, MODE, false, DROP>), dim3(grid), dim3(64 * SPMM_WPB), 0, st, a);
}

template <int D, int MODE>
static int launch_spmm_d(const SpmmArgs &a, int x_dtype, int y_dtype, hipStream_t st) {
    if (MODE & M_SPARSE) x_dtype = LGCN_F32;           // source is the fixed-point table; TI unused
    if (MODE & M_ADAM) y_dtype = LGCN_F32;
    if (x_dtype == LGCN_FP8 || y_dtype == LGCN_FP8) {
        if (a.dr.on) { lgcn_set_error("edge dropout is not implemented for fp8 tables"); return 3; }
        // fp8 tables: 16 elements per lane, so d >= 64; fp8 <-> bf16 conversions are not instantiated
        if constexpr (D >= 64) {
            if (x_dtype == LGCN_FP8 && y_dtype == LGCN_FP8) { launch_spmm_t<D, fp8_t, fp8_t, MODE>(a, st); return 0; }
            if (x_dtype == LGCN_FP8 && y_dtype == LGCN_F32) { launch_spmm_t<D, fp8_t, float, MODE>(a, st); return 0; }
            if (x_dtype == LGCN_F32 && y_dtype == LGCN_FP8) { launch_spmm_t<D, float, fp8_t, MODE>(a, st); return 0; }
        }
        lgcn_set_error("fp8 tables: embedding dim 64, 128 or 256, and fp8 <-> fp32 only (no fp8 <-> bf16 launch)");
        return 3;
    }
    // every MODE that comes through here (0, ADDG, ADDG|ADAM, SPARSE|ADDG, SPARSE|ADDG|ADAM) is one the dropout step launches;
    // M_ADDSELF is launched by lgcn_spmm_launch itself and has no DROP instantiation
    static_assert(!(MODE & M_ADDSELF), "item-item smoothing never takes the dropout branch");
    if (a.dr.on) {
        // edge dropout: its own instantiations, and only the type pairs a launch can ask for (a sparse input is fp32, Adam writes fp32)
        if (x_dtype == LGCN_F32 && y_dtype == LGCN_F32) launch_spmm_t<D, float, float, MODE, true>(a, st);
        else if constexpr ((MODE & M_SPARSE) != 0) {
            if constexpr (!(MODE & M_ADAM)) launch_spmm_t<D, float, bf16_t, MODE, true>(a, st);
        } else if constexpr ((MODE & M_ADAM) != 0) launch_spmm_t<D, bf16_t, float, MODE, true>(a, st);
        else if (x_dtype == LGCN_F32) launch_spmm_t<D, float, bf16_t, MODE, true>(a, st);
        else if (y_dtype == LGCN_F32) launch_spmm_t<D, bf16_t, float, MODE, true>(a, st);
        else launch_spmm_t<D, bf16_t, bf16_t, MODE, true>(a, st);
        return 0;
    }
    if (x_dtype == LGCN_F32 && y_dtype == LGCN_F32) launch_spmm_t<D, float, float, MODE>(a, st);
    else if (x_dtype == LGCN_F32 && y_dtype == LGCN_BF16) launch_spmm_t<D, float, bf16_t, MODE>(a, st);
    else if (x_dtype == LGCN_BF16 && y_dtype == LGCN_F32) launch_spmm_t<D, bf16_t, float, MODE>(a, st);
    else launch_spmm_t<D, bf16_t, bf16_t, MODE>(a, st);
    return 0;
}

// Layer weights (M_WTS): the four launches of the weighted Horner chain and only the type pairs they can ask for (a sparse input
// is fp32, Adam writes fp32, a middle layer reads and writes the activation type); no fp8, no dropout
template <int D, int MODE>
static int launch_spmm_wts(const SpmmArgs &a, int x_dtype, int y_dtype, hipStream_t st) {
    static_assert((MODE & M_ADDG) && !(MODE & M_ADDSELF), "the weighted forms are the Horner launches");
    if (MODE & M_SPARSE) x_dtype = LGCN_F32;
    if (MODE & M_ADAM) y_dtype = LGCN_F32;
    if (x_dtype == LGCN_FP8 || y_dtype == LGCN_FP8 || a.dr.on) { lgcn_set_error("layer weights are not implemented for fp8 tables or with edge dropout"); return 3; }
    if (x_dtype == LGCN_F32 && y_dtype == LGCN_F32) launch_spmm_t<D, float, float, MODE>(a, st);
    else if constexpr ((MODE & M_SPARSE) != 0) {
        if constexpr (!(MODE & M_ADAM)) launch_spmm_t<D, float, bf16_t, MODE>(a, st);
    } else if constexpr ((MODE & M_ADAM) != 0) launch_spmm_t<D, bf16_t, float, MODE>(a, st);
    else if (x_dtype == LGCN_BF16 && y_dtype == LGCN_BF16) launch_spmm_t<D, bf16_t, bf16_t, MODE>(a, st);
    else { lgcn_set_error("layer weights: no such launch"); return 3; }
    return 0;
}
template <int D, int MODE>
static int launch_spmm_dm(const SpmmArgs &a, int x_dtype, int y_dtype, hipStream_t st) {
    if constexpr ((MODE & M_WTS) != 0) return launch_spmm_wts<D, MODE>(a, x_dtype, y_dtype, st);
    else return launch_spmm_d<D, MODE>(a, x_dtype, y_dtype, st);
}

template <int MODE>
static int launch_spmm(const SpmmArgs &a, int d, int x_dtype, int y_dtype, hipStream_t st) {
    DISPATCH_D(d, return (launch_spmm_dm<D, MODE>(a, x_dtype, y_dtype, st)));
}

int lgcn_spmm_launch(const SpmmArgs &a, int mode, int d, int x_dtype, int y_dtype, hipStream_t st) {
    if ((mode & M_SPARSE) && (mode & M_ADAM) && (a.Pb || a.Pq)) { lgcn_set_error("spmm: a sparse-input launch keeps no shadow of P"); return 3; }
    switch (mode) {
    case 0: return launch_spmm<0>(a, d, x_dtype, y_dtype, st);
    case M_ADDSELF:       // Y = selfX + A X on fp32 tables (item-item smoothing): only the fp32 instance exists
        DISPATCH_D(d, launch_spmm_t<D, float, float, M_ADDSELF>(a, st));
        return 0;
    case M_ADDG: return launch_spmm<M_ADDG>(a, d, x_dtype, y_dtype, st);
    case M_ADDG | M_ADAM: return launch_spmm<M_ADDG | M_ADAM>(a, d, x_dtype, y_dtype, st);
    case M_SPARSE | M_ADDG: return launch_spmm<M_SPARSE | M_ADDG>(a, d, x_dtype, y_dtype, st);
    case M_SPARSE | M_ADDG | M_ADAM: return launch_spmm<M_SPARSE | M_ADDG | M_ADAM>(a, d, x_dtype, y_dtype, st);
    case M_ADDG | M_WTS: return launch_spmm<M_ADDG | M_WTS>(a, d, x_dtype, y_dtype, st);
    case M_ADDG | M_ADAM | M_WTS: return launch_spmm<M_ADDG | M_ADAM | M_WTS>(a, d, x_dtype, y_dtype, st);
    case M_SPARSE | M_ADDG | M_WTS: return launch_spmm<M_SPARSE | M_ADDG | M_WTS>(a, d, x_dtype, y_dtype, st);
    case M_SPARSE | M_ADDG | M_ADAM | M_WTS: return launch_spmm<M_SPARSE | M_ADDG | M_ADAM | M_WTS>(a, d, x_dtype, y_dtype, st);
    }
    lgcn_set_error("spmm: no such launch");
    return 3;
}

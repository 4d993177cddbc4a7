// lgcn_device_common.h -- what the device translation units of liblgcn_hip.so share (not installed): the 2^50 fixed point of
// G64, the vector typedefs, the switch over the embedding dim, and the few device functions that more than one file needs.  ONE
// definition of each lives here; build.kernel_hash() covers lgcn_device.hip alone, so code that another file needs too belongs
// in this header, not in a copy.
#ifndef LGCN_DEVICE_COMMON_H
#define LGCN_DEVICE_COMMON_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "lgcn_hip.h"
#include "lgcn_internal.h"      // HIP_OK, the launchers' error macro, comes from there (the host files use it too)

// G64 holds gradient rows as 64-bit fixed point: integer addition is associative, so a row's sum is order-free
#define FIXED_SCALE 1125899906842624.0   /* 2^50 */
#define FIXED_INV   8.8817841970012523e-16 /* 2^-50 */

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;        // the accumulator of a 32 x 32 MFMA
typedef __attribute__((ext_vector_type(2))) long long i64x2;      // (bf16_t: lgcn_kernels.h, whose args structs name it)

// runs the statement with D a compile-time constant; any other d is the caller's error 3
#define DISPATCH_D(d, ...)                                                       \
    switch (d) {                                                                 \
    case 32: { constexpr int D = 32; __VA_ARGS__; } break;                       \
    case 64: { constexpr int D = 64; __VA_ARGS__; } break;                       \
    case 128: { constexpr int D = 128; __VA_ARGS__; } break;                     \
    case 256: { constexpr int D = 256; __VA_ARGS__; } break;                     \
    default: lgcn_set_error("embedding dim must be 32, 64, 128 or 256"); return 3; \
    }

__device__ __forceinline__ float logsigmoid_f(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid_neg_f(float x) {
    const float z = expf(-fabsf(x));
    return x < 0.f ? 1.f / (1.f + z) : z / (1.f + z);
}

// element o of a table of the storage type TI, and the same by row and column (lgcn_device.hip adds the fp8 form of tab_elem)
template <typename TI> __device__ __forceinline__ float tab_at(const void *tab, int64_t o) { return (float)((const TI *)tab)[o]; }
template <typename TI> __device__ __forceinline__ float tab_elem(const void *tab, int64_t n_rows, int D, int64_t row, int col);
template <> __device__ __forceinline__ float tab_elem<float>(const void *tab, int64_t, int D, int64_t row, int col) { return tab_at<float>(tab, row * D + col); }
template <> __device__ __forceinline__ float tab_elem<bf16_t>(const void *tab, int64_t, int D, int64_t row, int col) { return tab_at<bf16_t>(tab, row * D + col); }

// sum / max over the LPT consecutive lanes of a lane group (xor-shuffle tree: every lane ends with the same bits)
template <int LPT> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = 1; off < LPT; off <<= 1) v += __shfl_xor(v, off);
    return v;
}
template <int LPT> __device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int off = 1; off < LPT; off <<= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// The output-table row of a slot of the dense-last batch-row launches (k_multineg, k_inbatch_rows): e[j] = the row `row` at
// columns j * LPT + l (mean over the K + 1 layers, or the weighted sum); e0[j] = E0's.  ONE expression for every loss, so a row
// has the same bits whichever loss reads it.
template <int D, typename TI, bool WTS>
__device__ __forceinline__ void slot_row(const MultiNegArgs &a, int64_t row, int l, float *e, float *e0) {
    constexpr int LPT = D < 64 ? D : 64, CPT = D / LPT;
    const float div = (float)(a.K + 1);
#pragma unroll
    for (int j = 0; j < CPT; j++) {
        const int64_t o = row * D + j * LPT + l;
        float s = a.X0[o];
        e0[j] = s;
        if constexpr (WTS) {
            s *= a.w[0];
            for (int k = 1; k <= a.K; k++) s += a.w[k] * tab_at<TI>(a.Xl[k], o);
            e[j] = s;
        } else {
            for (int k = 1; k <= a.K; k++) s += tab_at<TI>(a.Xl[k], o);
            e[j] = s / div;
        }
    }
}

// tile row of accumulator register `reg` on lane half h (C/D layout of the 32x32 MFMAs; the column is lane & 31)
__device__ __forceinline__ int mfma32_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// *g64 += g in the fixed point of G64
__device__ __forceinline__ void fixed_add(long long *g64, float g) {
    atomicAdd((unsigned long long *)g64, (unsigned long long)__double2ll_rn((double)g * FIXED_SCALE));
}
#endif

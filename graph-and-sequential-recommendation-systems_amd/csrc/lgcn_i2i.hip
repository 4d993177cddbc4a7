// lgcn_i2i.hip -- the item-item co-occurrence graph on the GPU.
//
// Restates build_item_item of the reference's preprocess_instacart_i2i.py (:61-170): a dict-of-dicts loop over every pair of
// every basket, a weighting (cooc / jaccard / pmi, fp64), heapq.nlargest(topk) per item, maximum(A, A^T), D^-1/2 A D^-1/2.
// Two stages so that each can be tested alone:
//
//   lgcn_i2i_topk    baskets (CSR) -> per item the topk best neighbours in rank order.  The count c[i][j] is the sparse product
//                    R^T R, never materialised whole: a workgroup takes an item i, walks i's baskets from a device-built
//                    item -> basket transpose and every other item j of each basket, and accumulates (count, first basket) per
//                    j with integer add / integer min -- order-independent, so the result is bitwise reproducible whatever
//                    the order the atomics land in.  Two accumulators, chosen per row by the bound  sum_{b holds i} (|b| - 1)
//                    on the row's distinct neighbours: an LDS hash table (4096 slots, rows of <= 3072 neighbours) and a dense
//                    pair of arrays in a pooled global scratch (one per workgroup, cleared by walking the row's own list).
//                    The fp64 weight and the tie rule make one 128-bit key per neighbour,
//                        ~bits(weight) | first basket | j        (ascending = weight down, first basket up, j up)
//                    which is a TOTAL order -- exactly the order heapq.nlargest leaves a dict filled by
//                    combinations(sorted(items), 2) in.  The k-th key is found by an MSB-first radix select (16 passes of 8
//                    bits, a 256-bin LDS histogram each), the <= 256 keys at or below it are ranked by counting.
//   lgcn_i2i_finish  both orientations of every kept pair -> rocPRIM radix sort by (row, column) -> duplicates merged by
//                    maximum -> fp32 row sums -> v * deg_i^-1/2 * deg_j^-1/2.
//
// Temporaries are library-owned and stream-ordered (hipMallocAsync / hipFreeAsync; rc 4 if the runtime has no such pool).
// Each stage synchronises ONCE, at its end, to read the device's verdict (rc; finish: the nnz): every kernel that writes an
// output reads the error word first, so a refused call leaves the outputs as they were.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "lgcn_hip.h"
#include "lgcn_internal.h"

#define I2I_SLOTS 4096            /* LDS hash table: 3 x 4 bytes x 4096 = 48 KiB -> three workgroups per CU (160 KiB) */
#define I2I_LDS_CAP 3072          /* rows whose neighbour bound is <= this use it (load factor <= 0.75, linear probing) */
#define I2I_EMPTY (-1)
#define I2I_TOPK_MAX 256
#define I2I_WG_SMALL 768          /* 256 CUs x 3 resident workgroups */
#define I2I_WG_LARGE 256
#define I2I_PAD (~0ull)

namespace {

struct I2IStat {
    int err;                      // bit 0: indptr malformed, bit 1: item id out of range, bit 2: finish capacity too small
    int total;                    // kept baskets
    int n_small, n_large;         // rows per accumulator form
    int next_small, next_large;   // work counters of the row kernels
    unsigned long long sumlen;    // finish: sum of len
    long long nnz;                // finish: entries written
};

typedef unsigned long long u64;

struct I2IArgs {
    const int64_t *indptr; const int32_t *idx;
    const int64_t *tptr; const int32_t *tb; const int32_t *deg;
    I2IStat *st; const int32_t *list;
    int32_t m, topk, weight;
    ulonglong2 *keys; size_t keys_stride;
    int32_t *dcnt, *dmin, *dlist;             // dense form: [workgroups][m] each
    int32_t *cols; float *w; int32_t *len;
};

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

// ---- stage 1: checks, degrees, transpose, bins ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_i2i_check(const int64_t *indptr, int64_t nb, int64_t nnz, int32_t min_basket, I2IStat *st) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    int bad = 0, kept = 0;
    if (t == 0 && (indptr[0] != 0 || indptr[nb] != nnz)) bad |= 1;
    for (int64_t b = t; b < nb; b += stride) {
        const int64_t s = indptr[b + 1] - indptr[b];
        if (s < 0) bad |= 1;
        kept += s >= (int64_t)min_basket ? 1 : 0;
    }
    if (bad) atomicOr(&st->err, bad);
    for (int o = 32; o > 0; o >>= 1) kept += __shfl_down(kept, o);          // total = kept baskets: one atomic per wave
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(&st->total, kept);
}
// (second kernel: the ids are read only once the offsets are known to stay inside indices[0, nnz))
__global__ void __launch_bounds__(256) k_i2i_check_ids(const int32_t *idx, int64_t nnz, int32_t m, I2IStat *st) {
    if (st->err) return;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    int bad = 0;
    for (int64_t e = t; e < nnz; e += stride) { const int32_t j = idx[e]; if (j < 0 || j >= m) bad = 2; }
    if (bad) atomicOr(&st->err, bad);
}

// one wave per basket.  FILL = false: deg[j] += 1, nbound[j] += |b| - 1 over the kept baskets; FILL = true: the transpose.
// (the number of kept baskets comes from k_i2i_check: an atomic per basket on one word was most of this kernel's time)
template <bool FILL>
__global__ void __launch_bounds__(256) k_i2i_baskets(const int64_t *indptr, const int32_t *idx, int64_t nb, int32_t min_basket, I2IStat *st,
                                                     int32_t *deg, u64 *nbound, const int64_t *tptr, int32_t *cursor, int32_t *tb) {
    if (st->err) return;
    const int lane = threadIdx.x & 63;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < nb; b += (int64_t)gridDim.x * 4) {
        const int64_t s0 = indptr[b], s1 = indptr[b + 1];
        if (s1 - s0 < (int64_t)min_basket) continue;
        for (int64_t e = s0 + lane; e < s1; e += 64) {
            const int32_t j = idx[e];
            if (FILL) tb[tptr[j] + atomicAdd(&cursor[j], 1)] = (int32_t)b;
            else { atomicAdd(&deg[j], 1); atomicAdd(&nbound[j], (u64)(s1 - s0 - 1)); }
        }
    }
}

__global__ void __launch_bounds__(256) k_i2i_bin(const int32_t *deg, const u64 *nbound, int32_t m, I2IStat *st, int32_t *small, int32_t *large, int32_t *len) {
    if (st->err) return;
    const int32_t i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = i < m;
    if (in) len[i] = 0;
    const u64 nbd = in && deg[i] != 0 ? nbound[i] : 0;
    const bool sm = nbd != 0 && nbd <= I2I_LDS_CAP, lg = nbd > I2I_LDS_CAP;
    const u64 ms = __ballot(sm), ml = __ballot(lg);                         // one atomic per wave and list
    int bs = 0, bl = 0;
    if (lane == 0) { if (ms) bs = atomicAdd(&st->n_small, __popcll(ms)); if (ml) bl = atomicAdd(&st->n_large, __popcll(ml)); }
    bs = __shfl(bs, 0); bl = __shfl(bl, 0);
    const u64 below = (1ull << lane) - 1ull;
    if (sm) small[bs + __popcll(ms & below)] = i;
    if (lg) large[bl + __popcll(ml & below)] = i;
}

__global__ void __launch_bounds__(256) k_i2i_init(const I2IStat *st, int64_t n, int32_t *cols, float *w) {
    if (st->err) return;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) { cols[t] = -1; w[t] = 0.0f; }
}

// ---- stage 1: one row per workgroup ----------------------------------------------------------------------------------------
__device__ __forceinline__ ulonglong2 i2i_key(int weight, int c, int di, int dj, double total, int mb, int j) {
    double w;
    if (weight == LGCN_I2I_COOC) w = (double)c;
    else if (weight == LGCN_I2I_JACCARD) {
        const long long den = (long long)di + (long long)dj - (long long)c;
        w = den <= 0 ? 0.0 : (double)c / (double)den;
    } else {
        const double den = (double)di * (double)dj;
        w = den <= 0.0 ? 0.0 : log(((double)c * total) / den + 1e-12);
        w = w > 0.0 ? w : 0.0;
    }
    ulonglong2 k;
    k.x = ~(u64)__double_as_longlong(w);          // w >= +0: its bit pattern orders as the value does
    k.y = ((u64)(uint32_t)mb << 32) | (u64)(uint32_t)j;
    return k;
}
// byte p (0 = most significant) of the 128-bit key, and whether the bytes above it equal those of P
__device__ __forceinline__ unsigned i2i_byte(ulonglong2 k, int p) {
    return p < 8 ? (unsigned)(k.x >> (56 - 8 * p)) & 255u : (unsigned)(k.y >> (56 - 8 * (p - 8))) & 255u;
}
__device__ __forceinline__ bool i2i_match(ulonglong2 k, ulonglong2 P, int p) {
    if (p == 0) return true;
    if (p < 8) return (k.x >> (64 - 8 * p)) == (P.x >> (64 - 8 * p));
    if (k.x != P.x) return false;
    return p == 8 || (k.y >> (64 - 8 * (p - 8))) == (P.y >> (64 - 8 * (p - 8)));
}
__device__ __forceinline__ bool i2i_less(ulonglong2 a, ulonglong2 b) { return a.x < b.x || (a.x == b.x && a.y < b.y); }

template <bool LDSF>
__global__ void __launch_bounds__(256) k_i2i_rows(I2IArgs a) {
    __shared__ int t_key[LDSF ? I2I_SLOTS : 1], t_cnt[LDSF ? I2I_SLOTS : 1], t_min[LDSF ? I2I_SLOTS : 1];
    __shared__ unsigned hist[256];
    __shared__ ulonglong2 sel[I2I_TOPK_MAX];
    __shared__ int s_row, s_n, s_m, s_bin;
    __shared__ unsigned s_need;
    if (a.st->err) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    ulonglong2 *keys = a.keys + (size_t)blockIdx.x * a.keys_stride;
    int32_t *dcnt = LDSF ? nullptr : a.dcnt + (size_t)blockIdx.x * a.m;
    int32_t *dmin = LDSF ? nullptr : a.dmin + (size_t)blockIdx.x * a.m;
    int32_t *dlist = LDSF ? nullptr : a.dlist + (size_t)blockIdx.x * a.m;
    const int n_rows = LDSF ? a.st->n_small : a.st->n_large;
    const double total = a.st->total > 0 ? (double)a.st->total : 1.0;
    for (;;) {
        __syncthreads();
        if (tid == 0) { s_row = atomicAdd(LDSF ? &a.st->next_small : &a.st->next_large, 1); s_n = 0; s_m = 0; }
        if (LDSF) for (int s = tid; s < I2I_SLOTS; s += 256) { t_key[s] = I2I_EMPTY; t_cnt[s] = 0; t_min[s] = INT_MAX; }
        __syncthreads();
        if (s_row >= n_rows) break;
        const int32_t i = a.list[s_row];
        // accumulate (count, first basket) per neighbour: a wave per basket of i
        const int64_t p1 = a.tptr[i + 1];
        for (int64_t p = a.tptr[i] + wv; p < p1; p += 4) {
            const int32_t b = a.tb[p];
            const int64_t e1 = a.indptr[b + 1];
            for (int64_t e = a.indptr[b] + lane; e < e1; e += 64) {
                const int32_t j = a.idx[e];
                if (j == i) continue;
                if (LDSF) {
                    unsigned h = ((unsigned)j * 2654435761u) >> 20;           // 12 bits
                    for (;;) {                                                // ends: <= 3072 distinct keys in 4096 slots
                        const int prev = atomicCAS(&t_key[h], I2I_EMPTY, j);
                        if (prev == I2I_EMPTY || prev == j) { atomicAdd(&t_cnt[h], 1); atomicMin(&t_min[h], b); break; }
                        h = (h + 1) & (I2I_SLOTS - 1);
                    }
                } else {
                    if (atomicAdd(&dcnt[j], 1) == 0) dlist[atomicAdd(&s_n, 1)] = j;      // < m distinct neighbours
                    atomicMin(&dmin[j], b);
                }
            }
        }
        __syncthreads();
        // one key per neighbour; the dense accumulator is cleared as it is read
        const int di = a.deg[i];
        if (LDSF) {
            for (int s = tid; s < I2I_SLOTS; s += 256) {
                const int j = t_key[s];
                if (j != I2I_EMPTY) keys[atomicAdd(&s_n, 1)] = i2i_key(a.weight, t_cnt[s], di, a.deg[j], total, t_min[s], j);
            }
        } else {
            const int n0 = s_n;
            for (int q = tid; q < n0; q += 256) {
                const int j = __hip_atomic_load(&dlist[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int c = __hip_atomic_load(&dcnt[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const int mb = __hip_atomic_load(&dmin[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                keys[q] = i2i_key(a.weight, c, di, a.deg[j], total, mb, j);
                __hip_atomic_store(&dcnt[j], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&dmin[j], INT_MAX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();
        const int n = s_n;
        const int kk = n < a.topk ? n : a.topk;
        ulonglong2 P; P.x = I2I_PAD; P.y = I2I_PAD;
        if (n > a.topk) {
            // the kk-th smallest key, a byte per pass from the top
            P.x = 0; P.y = 0;
            unsigned need = (unsigned)kk;
            for (int p = 0; p < 16; p++) {
                hist[tid] = 0;
                __syncthreads();
                for (int q = tid; q < n; q += 256) { const ulonglong2 k = keys[q]; if (i2i_match(k, P, p)) atomicAdd(&hist[i2i_byte(k, p)], 1u); }
                __syncthreads();
                if (wv == 0) {
                    const unsigned a0 = hist[4 * lane], a1 = hist[4 * lane + 1], a2 = hist[4 * lane + 2], a3 = hist[4 * lane + 3];
                    const unsigned s = a0 + a1 + a2 + a3;
                    unsigned incl = s;
                    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o); if (lane >= o) incl += t; }
                    const unsigned excl = incl - s;
                    if (excl < need && need <= incl) {
                        unsigned c = excl; int u = 0;
                        if (need > c + a0) { c += a0; u = 1; if (need > c + a1) { c += a1; u = 2; if (need > c + a2) { c += a2; u = 3; } } }
                        s_bin = 4 * lane + u; s_need = need - c;
                    }
                }
                __syncthreads();
                const u64 bin = (u64)s_bin;
                need = s_need;
                if (p < 8) P.x |= bin << (56 - 8 * p); else P.y |= bin << (56 - 8 * (p - 8));
            }
        }
        for (int q = tid; q < n; q += 256) {
            const ulonglong2 k = keys[q];
            if (!i2i_less(P, k)) { const int pos = atomicAdd(&s_m, 1); if (pos < I2I_TOPK_MAX) sel[pos] = k; }
        }
        __syncthreads();
        if (tid < kk) {
            const ulonglong2 k = sel[tid];
            int rank = 0;
            for (int u = 0; u < kk; u++) rank += i2i_less(sel[u], k) ? 1 : 0;
            const int64_t o = (int64_t)i * a.topk + rank;
            a.cols[o] = (int32_t)(uint32_t)(k.y & 0xffffffffull);
            a.w[o] = (float)__longlong_as_double((long long)~k.x);
        }
        if (tid == 0) a.len[i] = kk;
    }
}

// ---- stage 2 ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fin_sum(const int32_t *len, int32_t m, int32_t topk, I2IStat *st) {
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    int l = i < m ? len[i] : 0;
    l = l < 0 ? 0 : (l > topk ? topk : l);
    for (int o = 32; o > 0; o >>= 1) l += __shfl_down(l, o);
    if ((threadIdx.x & 63) == 0 && l) atomicAdd(&st->sumlen, (u64)l);
}
__global__ void k_fin_guard(I2IStat *st, int64_t capacity) {
    if (2ull * st->sumlen > (u64)capacity) st->err = 4;
}
__global__ void __launch_bounds__(256) k_fin_emit(const int32_t *cols, const float *w, const int32_t *len, int32_t m, int32_t topk, u64 *keys, float *vals) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)m * topk) return;
    const int32_t i = (int32_t)(t / topk), r = (int32_t)(t % topk);
    u64 k0 = I2I_PAD, k1 = I2I_PAD;
    float v = 0.0f;
    if (r < len[i]) {
        const int32_t j = cols[t];
        v = w[t];
        if (j >= 0 && j < m && v > 0.0f) { k0 = ((u64)(uint32_t)i << 32) | (uint32_t)j; k1 = ((u64)(uint32_t)j << 32) | (uint32_t)i; }
    }
    keys[2 * t] = k0; keys[2 * t + 1] = k1;
    vals[2 * t] = v; vals[2 * t + 1] = v;
}
__global__ void __launch_bounds__(256) k_fin_flag(const u64 *keys, int64_t n, int32_t *flag) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n) flag[p] = (keys[p] != I2I_PAD && (p == 0 || keys[p] != keys[p - 1])) ? 1 : 0;
}
__global__ void __launch_bounds__(256) k_fin_write(const u64 *keys, const float *vals, const int32_t *flag, const int32_t *pos, int64_t n, int64_t capacity,
                                                   I2IStat *st, int32_t *rows, int32_t *indices, float *raw) {
    if (st->err) return;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    if (p == n - 1) st->nnz = (long long)pos[p] + flag[p];
    if (!flag[p]) return;
    const int64_t o = pos[p];
    if (o >= capacity) return;
    float v = vals[p];
    for (int64_t q = p + 1; q < n && keys[q] == keys[p]; q++) v = fmaxf(v, vals[q]);      // maximum(A, A^T)
    rows[o] = (int32_t)(keys[p] >> 32);
    indices[o] = (int32_t)(uint32_t)(keys[p] & 0xffffffffull);
    raw[o] = v;
}
__global__ void __launch_bounds__(256) k_fin_indptr(const I2IStat *st, const int32_t *rows, int32_t m, int64_t n, int32_t *indptr) {
    if (st->err) return;
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nnz = st->nnz;
    if (o > nnz || o > n) return;
    const int32_t hi = o < nnz ? rows[o] : m, lo = o > 0 ? rows[o - 1] + 1 : 0;
    for (int32_t r = lo; r <= hi; r++) indptr[r] = (int32_t)o;
}
// a wave per row: fp32 row sum in a fixed order -> deg^-1/2 (0 -> 1)
__global__ void __launch_bounds__(256) k_fin_rowsum(const I2IStat *st, const int32_t *indptr, const float *raw, int32_t m, float *isq) {
    if (st->err) return;
    const int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= m) return;
    float s = 0.0f;
    for (int32_t o = indptr[r] + lane; o < indptr[r + 1]; o += 64) s += raw[o];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if (lane == 0) { if (s == 0.0f) s = 1.0f; isq[r] = 1.0f / sqrtf(s); }
}
__global__ void __launch_bounds__(256) k_fin_scale(const I2IStat *st, const int32_t *rows, const int32_t *indices, const float *raw, const float *isq, float *vals) {
    if (st->err) return;
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o < st->nnz) vals[o] = (raw[o] * isq[rows[o]]) * isq[indices[o]];
}

namespace {
struct Tmp {
    void *p = nullptr;
    int alloc(size_t bytes, hipStream_t st) {                  // stream-ordered pool only: no allocation that would need a second synchronise
        if (hipMallocAsync(&p, bytes, st) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return 4; }
        return 0;
    }
    void release(hipStream_t st) { if (p) (void)hipFreeAsync(p, st); p = nullptr; }
};
inline unsigned nblk(int64_t n, int64_t cap = 1 << 24) { int64_t b = (n + 255) / 256; if (b < 1) b = 1; if (b > cap) b = cap; return (unsigned)b; }
}  // namespace

extern "C" int lgcn_i2i_topk(const int64_t *indptr, const int32_t *indices, int64_t n_baskets, int64_t nnz, int32_t m_items,
                             int32_t topk, int32_t weight, int32_t min_basket, int32_t *cols, float *w, int32_t *len, void *stream) {
    if (topk < 1 || topk > I2I_TOPK_MAX) { lgcn_set_error("lgcn_i2i_topk: topk must be in 1..256"); return 3; }
    if (weight != LGCN_I2I_COOC && weight != LGCN_I2I_JACCARD && weight != LGCN_I2I_PMI) { lgcn_set_error("lgcn_i2i_topk: unknown weight"); return 3; }
    if (min_basket < 0) { lgcn_set_error("lgcn_i2i_topk: min_basket must be >= 0"); return 3; }
    if (n_baskets <= 0 || nnz <= 0 || m_items <= 0 || n_baskets > 0x7f000000LL || nnz > 0x7f000000LL) {
        lgcn_set_error("lgcn_i2i_topk: n_baskets, nnz and m_items must be positive (and at most 0x7f000000)"); return 3; }
    if ((int64_t)m_items * topk * 2 > 0x7ffffff0LL) { lgcn_set_error("lgcn_i2i_topk: 2 m_items topk must stay below 2^31"); return 3; }
    if (!indptr || !indices || !cols || !w || !len) { lgcn_set_error("lgcn_i2i_topk: null pointer"); return 3; }
    hipStream_t st = (hipStream_t)stream;
    const size_t m = (size_t)m_items;
    const int wg_small = (int)(m < I2I_WG_SMALL ? m : I2I_WG_SMALL);
    size_t wl = ((size_t)512 << 20) / (32 * m);
    const int wg_large = (int)(wl < 1 ? 1 : (wl > I2I_WG_LARGE ? I2I_WG_LARGE : wl));
    size_t scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, (const int32_t *)nullptr, (int64_t *)nullptr, (int64_t)0, m + 1, rocprim::plus<int64_t>(), st);
    // layout; everything up to o_zero_end is cleared
    size_t o = 0;
    const size_t o_stat = o; o = up256(o + sizeof(I2IStat));
    const size_t o_deg = o; o = up256(o + (m + 1) * 4);
    const size_t o_nb = o; o = up256(o + m * 8);
    const size_t o_cur = o; o = up256(o + m * 4);
    const size_t o_dcnt = o; o = up256(o + (size_t)wg_large * m * 4);
    const size_t o_zero_end = o;
    const size_t o_dmin = o; o = up256(o + (size_t)wg_large * m * 4);
    const size_t o_dmin_end = o;
    const size_t o_dlist = o; o = up256(o + (size_t)wg_large * m * 4);
    const size_t o_tptr = o; o = up256(o + (m + 1) * 8);
    const size_t o_tb = o; o = up256(o + (size_t)nnz * 4);
    const size_t o_small = o; o = up256(o + m * 4);
    const size_t o_large = o; o = up256(o + m * 4);
    const size_t o_scan = o; o = up256(o + scan_bytes);
    const size_t o_ks = o; o = up256(o + (size_t)wg_small * I2I_LDS_CAP * 16);
    const size_t o_kl = o; o = up256(o + (size_t)wg_large * m * 16);
    Tmp tmp;
    if (tmp.alloc(o, st)) { lgcn_set_error("lgcn_i2i_topk: cannot allocate the temporaries"); return 4; }
    char *base = (char *)tmp.p;
    I2IStat *stat = (I2IStat *)(base + o_stat);
    int32_t *deg = (int32_t *)(base + o_deg), *cursor = (int32_t *)(base + o_cur), *tb = (int32_t *)(base + o_tb);
    u64 *nbound = (u64 *)(base + o_nb);
    int64_t *tptr = (int64_t *)(base + o_tptr);
    int32_t *small = (int32_t *)(base + o_small), *large = (int32_t *)(base + o_large);
    int rc = 0;
    if (hipMemsetAsync(base, 0, o_zero_end, st) != hipSuccess || hipMemsetAsync(base + o_dmin, 0x7f, o_dmin_end - o_dmin, st) != hipSuccess) {
        tmp.release(st); lgcn_set_error("lgcn_i2i_topk: memset failed"); return 10; }
    hipLaunchKernelGGL(k_i2i_check, dim3(nblk(n_baskets, 4096)), dim3(256), 0, st, indptr, n_baskets, nnz, min_basket, stat);
    hipLaunchKernelGGL(k_i2i_check_ids, dim3(nblk(nnz, 4096)), dim3(256), 0, st, indices, nnz, m_items, stat);
    const unsigned bb = nblk(n_baskets * 64, 8192);
    hipLaunchKernelGGL(k_i2i_baskets<false>, dim3(bb), dim3(256), 0, st, indptr, indices, n_baskets, min_basket, stat, deg, nbound,
                       (const int64_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
    if (rocprim::exclusive_scan(base + o_scan, scan_bytes, (const int32_t *)deg, tptr, (int64_t)0, m + 1, rocprim::plus<int64_t>(), st) != hipSuccess) {
        tmp.release(st); lgcn_set_error("lgcn_i2i_topk: scan failed"); return 10; }
    hipLaunchKernelGGL(k_i2i_baskets<true>, dim3(bb), dim3(256), 0, st, indptr, indices, n_baskets, min_basket, stat, deg, nbound,
                       (const int64_t *)tptr, cursor, tb);
    hipLaunchKernelGGL(k_i2i_bin, dim3(nblk(m_items)), dim3(256), 0, st, (const int32_t *)deg, (const u64 *)nbound, m_items, stat, small, large, len);
    hipLaunchKernelGGL(k_i2i_init, dim3(nblk((int64_t)m * topk)), dim3(256), 0, st, (const I2IStat *)stat, (int64_t)m * topk, cols, w);
    I2IArgs a{indptr, indices, tptr, tb, deg, stat, large, m_items, topk, weight,
              (ulonglong2 *)(base + o_kl), m, (int32_t *)(base + o_dcnt), (int32_t *)(base + o_dmin), (int32_t *)(base + o_dlist), cols, w, len};
    hipLaunchKernelGGL(k_i2i_rows<false>, dim3(wg_large), dim3(256), 0, st, a);      // the long rows first
    a.list = small; a.keys = (ulonglong2 *)(base + o_ks); a.keys_stride = I2I_LDS_CAP;
    hipLaunchKernelGGL(k_i2i_rows<true>, dim3(wg_small), dim3(256), 0, st, a);
    I2IStat h{};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, stat, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { lgcn_set_error("lgcn_i2i_topk: kernels failed"); rc = 10; }
    tmp.release(st);
    if (rc) return rc;
    if (h.err & 1) { lgcn_set_error("lgcn_i2i_topk: basket offsets are not a CSR over nnz entries"); return 6; }
    if (h.err & 2) { lgcn_set_error("lgcn_i2i_topk: item id outside [0, m_items)"); return 5; }
    return 0;
}

extern "C" int lgcn_i2i_finish(const int32_t *cols, const float *w, const int32_t *len, int32_t m_items, int32_t topk, int64_t capacity,
                               int32_t *indptr, int32_t *indices, float *vals, int64_t *nnz_out, void *stream) {
    if (topk < 1 || topk > I2I_TOPK_MAX) { lgcn_set_error("lgcn_i2i_finish: topk must be in 1..256"); return 3; }
    if (m_items <= 0 || capacity <= 0 || (int64_t)m_items * topk * 2 > 0x7ffffff0LL) {
        lgcn_set_error("lgcn_i2i_finish: m_items and capacity must be positive, 2 m_items topk below 2^31"); return 3; }
    if (!cols || !w || !len || !indptr || !indices || !vals || !nnz_out) { lgcn_set_error("lgcn_i2i_finish: null pointer"); return 3; }
    hipStream_t st = (hipStream_t)stream;
    const size_t m = (size_t)m_items, n = 2 * m * (size_t)topk;
    size_t sort_bytes = 0, scan_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, (const u64 *)nullptr, (u64 *)nullptr, (const float *)nullptr, (float *)nullptr, n, 0, 64, st);
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, n, rocprim::plus<int32_t>(), st);
    const size_t lib_bytes = sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
    size_t o = 0;
    const size_t o_stat = o; o = up256(o + sizeof(I2IStat));
    const size_t o_k0 = o; o = up256(o + n * 8);
    const size_t o_k1 = o; o = up256(o + n * 8);
    const size_t o_v0 = o; o = up256(o + n * 4);
    const size_t o_v1 = o; o = up256(o + n * 4);
    const size_t o_flag = o; o = up256(o + n * 4);
    const size_t o_pos = o; o = up256(o + n * 4);
    const size_t o_rows = o; o = up256(o + n * 4);
    const size_t o_raw = o; o = up256(o + n * 4);
    const size_t o_isq = o; o = up256(o + m * 4);
    const size_t o_lib = o; o = up256(o + lib_bytes);
    Tmp tmp;
    if (tmp.alloc(o, st)) { lgcn_set_error("lgcn_i2i_finish: cannot allocate the temporaries"); return 4; }
    char *base = (char *)tmp.p;
    I2IStat *stat = (I2IStat *)(base + o_stat);
    u64 *k0 = (u64 *)(base + o_k0), *k1 = (u64 *)(base + o_k1);
    float *v0 = (float *)(base + o_v0), *v1 = (float *)(base + o_v1), *raw = (float *)(base + o_raw), *isq = (float *)(base + o_isq);
    int32_t *flag = (int32_t *)(base + o_flag), *pos = (int32_t *)(base + o_pos), *rows = (int32_t *)(base + o_rows);
    int rc = 0;
    if (hipMemsetAsync(stat, 0, sizeof(I2IStat), st) != hipSuccess) { tmp.release(st); lgcn_set_error("lgcn_i2i_finish: memset failed"); return 10; }
    hipLaunchKernelGGL(k_fin_sum, dim3(nblk(m_items)), dim3(256), 0, st, len, m_items, topk, stat);
    hipLaunchKernelGGL(k_fin_guard, dim3(1), dim3(1), 0, st, stat, capacity);
    hipLaunchKernelGGL(k_fin_emit, dim3(nblk((int64_t)(n / 2))), dim3(256), 0, st, cols, w, len, m_items, topk, k0, v0);
    if (rocprim::radix_sort_pairs(base + o_lib, sort_bytes, (const u64 *)k0, k1, (const float *)v0, v1, n, 0, 64, st) != hipSuccess) {
        tmp.release(st); lgcn_set_error("lgcn_i2i_finish: radix sort failed"); return 10; }
    hipLaunchKernelGGL(k_fin_flag, dim3(nblk((int64_t)n)), dim3(256), 0, st, (const u64 *)k1, (int64_t)n, flag);
    if (rocprim::exclusive_scan(base + o_lib, scan_bytes, (const int32_t *)flag, pos, (int32_t)0, n, rocprim::plus<int32_t>(), st) != hipSuccess) {
        tmp.release(st); lgcn_set_error("lgcn_i2i_finish: scan failed"); return 10; }
    hipLaunchKernelGGL(k_fin_write, dim3(nblk((int64_t)n)), dim3(256), 0, st, (const u64 *)k1, (const float *)v1, (const int32_t *)flag, (const int32_t *)pos,
                       (int64_t)n, capacity, stat, rows, indices, raw);
    hipLaunchKernelGGL(k_fin_indptr, dim3(nblk((int64_t)n + 1)), dim3(256), 0, st, (const I2IStat *)stat, (const int32_t *)rows, m_items, (int64_t)n, indptr);
    hipLaunchKernelGGL(k_fin_rowsum, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, (const I2IStat *)stat, (const int32_t *)indptr, (const float *)raw, m_items, isq);
    hipLaunchKernelGGL(k_fin_scale, dim3(nblk((int64_t)n)), dim3(256), 0, st, (const I2IStat *)stat, (const int32_t *)rows, (const int32_t *)indices,
                       (const float *)raw, (const float *)isq, vals);
    I2IStat h{};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h, stat, sizeof h, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) { lgcn_set_error("lgcn_i2i_finish: kernels failed"); rc = 10; }
    tmp.release(st);
    if (rc) return rc;
    if (h.err) { lgcn_set_error("lgcn_i2i_finish: output capacity below 2 * sum(len)"); return 7; }
    *nnz_out = (int64_t)h.nnz;
    return 0;
}

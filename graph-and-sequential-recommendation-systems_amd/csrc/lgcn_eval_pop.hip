// lgcn_eval_pop.hip -- popularity-aware evaluation for gfx950: from the ranked lists lgcn_eval_topk_ex wrote, recall split by
// item-popularity group, the share of every group in the lists, the average popularity of the recommended items, catalogue
// coverage and the Gini index of item exposure, at up to 8 cut-offs (lgcn_eval_pop_metrics; definitions: include/lgcn_hip.h,
// DESIGN 4.27).  Nothing here scores anything: the lists are the input.
//
// Four launches behind one memset of the temporaries:
//   k_pop_slots  a lane group (32 lanes for K <= 32, else a wave) per evaluation slot, the lanes striding over the list
//                positions: the row is one coalesced load, each lane searches its entry in the slot's test list and gathers the
//                entry's packed item word; the per-(cut-off, group) hit and list counts are population counts of ballots
//                against the lane masks r < ks[q].  Lane (q, g) of the group owns that pair's counts and quotients.  ONE
//                integer atomic per list entry goes to the exposure bucket of the smallest cut-off above its position.
//   k_pop_sum    the workgroups' partial sums merged in a fixed order (float64 quotients, int64 counts).
//   k_pop_items  per item the prefix over the buckets = the exposure e_k[i], counted into the histogram H of the exposure values.
//   k_pop_gini   per cut-off one scan over the histogram: covered items, sum of e, and sum_v v H[v] (2 R_v + H[v] - m),
//                R_v = #{items exposed < v}.
// Every sum across lanes, slots or items is an integer sum (order-free) except the two quotient sums, and those are added in
// an order fixed by n_eval and K alone: all outputs are bitwise reproducible, with or without per_slot.  No float atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lgcn_device_common.h"

namespace {

#define POP_WG_MAX 1024                 /* workgroups of k_pop_slots (each loops over its slots): the number of partial sums */
#define POP_FW 128                      /* float64 partials of a workgroup: [8 cut-offs][recall_share | recall_by_group][8 groups] */
#define POP_IW 80                       /* int64 partials: list counts [8][8] | popularity per bucket [8] | slots with t_g > 0 [8] */
#define POP_HB 256                      /* exposure values below this are counted in LDS first (k_pop_items) */

typedef unsigned long long u64;

struct PopArgs {
    const int32_t *topk; int32_t n_eval, K;
    const int64_t *test_ptr; const int32_t *test_idx;
    const uint32_t *info; int32_t m_items, n_groups;
    int32_t ks[8], sk[8], n_ks;         // the cut-offs as given, and sorted ascending (duplicates kept)
    int32_t *bucket;                    // [n_ks, m_items], zero on entry: bucket[b][i] = entries of item i at positions sk[b-1] <= r < sk[b]
    double *per_slot;                   // [n_eval, n_ks, 2, n_groups] or NULL
    double *part_f;                     // [workgroups, POP_FW]
    u64 *part_i;                        // [workgroups, POP_IW]
};

// ---- the per-slot pass.  Per-group arrays hold 8 columns and the group is `word & 7`: no item word can index past them.
template <int LG>
__global__ void __launch_bounds__(256) k_pop_slots(PopArgs a) {
    constexpr int GPW = 64 / LG, NSUB = 4 * GPW, NP = 64 / LG, QS = LG / 8;      // lane (q0, g) owns the pairs (q0 + j QS, g), j < NP
    constexpr uint64_t GMASK = LG == 64 ? ~0ull : ((1ull << (LG & 63)) - 1ull);
    __shared__ double red_f[NSUB][POP_FW];
    __shared__ u64 red_i[NSUB][64];
    __shared__ u64 red_n[NSUB][8];
    __shared__ u64 pop_b[8];
    __shared__ int32_t ks_l[8], sk_l[8];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int grp = lane / LG, l = lane % LG, sub = wid * GPW + grp;
    const int g = l & 7, q0 = l >> 3;
    if (tid < 8) { pop_b[tid] = 0ull; ks_l[tid] = tid < a.n_ks ? a.ks[tid] : 0; sk_l[tid] = tid < a.n_ks ? a.sk[tid] : 0x7fffffff; }
    __syncthreads();
    double fs[NP], fg[NP];
    u64 lc[NP], ns = 0ull;
#pragma unroll
    for (int j = 0; j < NP; j++) { fs[j] = 0.0; fg[j] = 0.0; lc[j] = 0ull; }

    const int64_t per_pass = (int64_t)gridDim.x * NSUB;
    for (int64_t base = (int64_t)blockIdx.x * NSUB; base < a.n_eval; base += per_pass) {      // (workgroup-uniform trip count)
        const int64_t s = base + sub;
        const bool have = s < a.n_eval;
        int64_t tb = 0, te = 0;
        if (have) { tb = a.test_ptr[s]; te = a.test_ptr[s + 1]; if (te < tb) te = tb; }
        const int64_t len = te - tb;
        // ---- t_{s,g}: one walk over the test list, a ballot per group
        int64_t wlen = len;
        if constexpr (LG < 64) { const int64_t o = __shfl_xor(wlen, 32); wlen = o > wlen ? o : wlen; }
        uint32_t tg = 0;
        for (int64_t p = 0; p < wlen; p += LG) {                                              // (wave-uniform)
            int gi = 8;
            if (p + l < len) {
                const int32_t id = a.test_idx[tb + p + l];
                if ((uint32_t)id < (uint32_t)a.m_items) gi = (int)(a.info[id] & 7u);
            }
            uint64_t mine = 0ull;
#pragma unroll
            for (int x = 0; x < 8; x++) { const uint64_t b = __ballot(gi == x); if (g == x) mine = b; }
            tg += (uint32_t)__popcll((mine >> (grp * LG)) & GMASK);
        }
        // ---- the list: positions c0 + l
        uint32_t hq[NP], cq[NP];
#pragma unroll
        for (int j = 0; j < NP; j++) { hq[j] = 0u; cq[j] = 0u; }
        for (int c0 = 0; c0 < a.K; c0 += LG) {                                                // (uniform)
            const int r = c0 + l;
            int gi = 8;
            bool hit = false;
            if (have && r < a.K) {
                const int32_t id = a.topk[s * a.K + r];
                if ((uint32_t)id < (uint32_t)a.m_items) {                                     // (the -1 padding counts nowhere)
                    const uint32_t w = a.info[id];
                    gi = (int)(w & 7u);
                    int64_t lo = tb, hi = te;
                    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.test_idx[mid] < id) lo = mid + 1; else hi = mid; }
                    hit = lo < te && a.test_idx[lo] == id;
                    int b = 0;
                    while (b < 8 && sk_l[b] <= r) b++;                                        // the smallest sorted cut-off above r
                    if (b < a.n_ks) {
                        atomicAdd(a.bucket + (int64_t)b * a.m_items + id, 1);
                        atomicAdd(&pop_b[b], (u64)(w >> 3));
                    }
                }
            }
            uint64_t mh = 0ull, ml = 0ull;
#pragma unroll
            for (int x = 0; x < 8; x++) {
                const uint64_t bl = __ballot(gi == x), bh = __ballot(hit && gi == x);
                if (g == x) { ml = bl; mh = bh; }
            }
            ml = (ml >> (grp * LG)) & GMASK;
            mh = (mh >> (grp * LG)) & GMASK;
#pragma unroll
            for (int j = 0; j < NP; j++) {
                const int rem = ks_l[q0 + j * QS] - c0;                                       // lanes of this chunk below the cut-off
                const uint64_t below = rem <= 0 ? 0ull : rem >= LG ? GMASK : ((1ull << rem) - 1ull);
                hq[j] += (uint32_t)__popcll(mh & below);
                cq[j] += (uint32_t)__popcll(ml & below);
            }
        }
        // ---- the pair's quotients: one correctly rounded division each
#pragma unroll
        for (int j = 0; j < NP; j++) {
            const int q = q0 + j * QS;
            if (have && q < a.n_ks) {
                const double h = (double)hq[j];
                const double share = len > 0 ? h / (double)len : 0.0;
                const double byg = tg > 0u ? h / (double)tg : 0.0;
                fs[j] += share; fg[j] += byg; lc[j] += cq[j];
                if (a.per_slot && g < a.n_groups) {
                    double *o = a.per_slot + (s * a.n_ks + q) * 2 * a.n_groups;
                    o[g] = share; o[a.n_groups + g] = byg;
                }
            }
        }
        if (have && q0 == 0 && tg > 0u) ns += 1ull;
    }
    // ---- the workgroup's partials: its lane groups in a fixed order
#pragma unroll
    for (int j = 0; j < NP; j++) {
        const int q = q0 + j * QS;
        red_f[sub][(q * 2) * 8 + g] = fs[j]; red_f[sub][(q * 2 + 1) * 8 + g] = fg[j]; red_i[sub][q * 8 + g] = lc[j];
    }
    if (q0 == 0) red_n[sub][g] = ns;
    __syncthreads();
    if (tid < POP_FW) {
        double acc = 0.0;
        for (int x = 0; x < NSUB; x++) acc += red_f[x][tid];
        a.part_f[(int64_t)blockIdx.x * POP_FW + tid] = acc;
    }
    if (tid < 64) {
        u64 acc = 0ull;
        for (int x = 0; x < NSUB; x++) acc += red_i[x][tid];
        a.part_i[(int64_t)blockIdx.x * POP_IW + tid] = acc;
    } else if (tid < 72) {
        a.part_i[(int64_t)blockIdx.x * POP_IW + tid] = pop_b[tid - 64];
    } else if (tid < 80) {
        u64 acc = 0ull;
        for (int x = 0; x < NSUB; x++) acc += red_n[x][tid - 72];
        a.part_i[(int64_t)blockIdx.x * POP_IW + tid] = acc;
    }
}

// ---- the partials of the nwg workgroups, merged in a fixed order (one workgroup: 8 strided runs per column, then the 8 in order)
__global__ void __launch_bounds__(1024) k_pop_sum(PopArgs a, int32_t nwg, double *sums, int64_t *counts, int64_t *group_slots) {
    __shared__ double f[8][POP_FW];
    __shared__ u64 iv[8][POP_IW];
    __shared__ u64 tot[POP_IW];
    const int tid = threadIdx.x;
    {                                                       // (eight loads in flight, then added in their order: an absent row adds +0.0)
        const int c = tid & (POP_FW - 1), j = tid >> 7;
        double acc = 0.0;
        for (int w0 = j; w0 < nwg; w0 += 64) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const int w = w0 + 8 * u; v[u] = w < nwg ? a.part_f[(int64_t)w * POP_FW + c] : 0.0; }
#pragma unroll
            for (int u = 0; u < 8; u++) acc += v[u];
        }
        f[j][c] = acc;
    }
    if (tid < 8 * POP_IW) {
        const int c = tid % POP_IW, j = tid / POP_IW;
        u64 acc = 0ull;
        for (int w0 = j; w0 < nwg; w0 += 64) {
            u64 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) { const int w = w0 + 8 * u; v[u] = w < nwg ? a.part_i[(int64_t)w * POP_IW + c] : 0ull; }
#pragma unroll
            for (int u = 0; u < 8; u++) acc += v[u];
        }
        iv[j][c] = acc;
    }
    __syncthreads();
    const int G = a.n_groups;
    if (tid < POP_FW) {
        double acc = 0.0;
        for (int j = 0; j < 8; j++) acc += f[j][tid];
        const int q = tid >> 4, half = (tid >> 3) & 1, g = tid & 7;
        if (q < a.n_ks && g < G) sums[(q * 2 + half) * G + g] = acc;
    }
    if (tid < POP_IW) {
        u64 acc = 0ull;
        for (int j = 0; j < 8; j++) acc += iv[j][tid];
        tot[tid] = acc;
    }
    __syncthreads();
    if (tid < a.n_ks) {
        const int q = tid;
        int64_t *o = counts + (int64_t)q * (G + 5);
        u64 valid = 0ull, pop = 0ull;
        for (int g = 0; g < 8; g++) { valid += tot[q * 8 + g]; if (g < G) o[g] = (int64_t)tot[q * 8 + g]; }
        for (int b = 0; b < a.n_ks; b++) if (a.sk[b] <= a.ks[q]) pop += tot[64 + b];
        o[G] = (int64_t)valid; o[G + 1] = (int64_t)pop;
    }
    if (tid < G) group_slots[tid] = (int64_t)tot[72 + tid];
}

// ---- per item: e_k[i] = the buckets of the cut-offs up to k, and the histogram hist[q][v] of the exposure values (zero on entry, v in
//      1..n_eval: an item nobody was shown needs no counter).  Most exposed items share a few small values, so a workgroup counts the
//      values below POP_HB in LDS and adds each of its non-empty bins to the global histogram once.
__global__ void __launch_bounds__(256) k_pop_items(PopArgs a, int32_t *exposure, int32_t *hist) {
    __shared__ int32_t lh[8 * POP_HB];
    for (int t = threadIdx.x; t < 8 * POP_HB; t += 256) lh[t] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t hs = (int64_t)a.n_eval + 1;
    if (i < a.m_items) {
        int32_t bk[8];
#pragma unroll
        for (int b = 0; b < 8; b++) bk[b] = b < a.n_ks ? a.bucket[(int64_t)b * a.m_items + i] : 0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            if (q >= a.n_ks) break;
            int64_t e = 0;
#pragma unroll
            for (int b = 0; b < 8; b++) if (b < a.n_ks && a.sk[b] <= a.ks[q]) e += bk[b];
            if (exposure) exposure[(int64_t)q * a.m_items + i] = (int32_t)e;      // (may be the bucket array itself: all of it was read above)
            if (e > 0 && e < POP_HB) atomicAdd(&lh[q * POP_HB + (int)e], 1);
            else if (e >= POP_HB && e <= a.n_eval) atomicAdd(hist + q * hs + e, 1);
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < a.n_ks * POP_HB; t += 256) {
        const int q = t / POP_HB, v = t % POP_HB, c = lh[t];
        if (c && v <= a.n_eval) atomicAdd(hist + q * hs + v, c);                  // (v > n_eval only if a list repeats an id: dropped)
    }
}

// ---- per cut-off (one workgroup each): counts[q][G + 2 ..] = covered | sum of e | Gini numerator, all from the histogram H:
//      covered = sum_v H[v], sum of e = sum_v v H[v], numerator = sum_v v H[v] (2 R_v + H[v] - m) with R_v = (m - covered) + sum_{0<w<v} H[w].
//      A thread takes a run of consecutive values; R at the start of its run comes from a scan of the runs' item counts.  int64, exact.
__global__ void __launch_bounds__(1024) k_pop_gini(PopArgs a, const int32_t *hist, int64_t *counts) {
    __shared__ long long sc[2][1024];
    __shared__ u64 tot[2];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int64_t n = a.n_eval, m = a.m_items;
    const int32_t *H = hist + (int64_t)q * (n + 1);
    const int64_t run = (n + 1023) / 1024;
    const int64_t v0 = 1 + tid * run, v1 = v0 + run - 1 < n ? v0 + run - 1 : n;
    long long mine = 0;
    for (int64_t v = v0; v <= v1; v++) mine += H[v];
    sc[0][tid] = mine;
    if (tid < 2) tot[tid] = 0ull;
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < 1024; off <<= 1) {              // inclusive scan, double-buffered: one barrier per step
        long long v = sc[cur][tid];
        if (tid >= off) v += sc[cur][tid - off];
        sc[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    const long long covered = sc[cur][1023];
    long long R = (m - covered) + sc[cur][tid] - mine, sum = 0, se = 0;
    for (int64_t v = v0; v <= v1; v++) {
        const long long h = H[v];
        if (h) { sum += v * h * (2 * R + h - m); se += v * h; R += h; }
    }
    if (se) { atomicAdd(&tot[0], (u64)se); atomicAdd(&tot[1], (u64)sum); }      // (two's complement: the order of integer additions is free)
    __syncthreads();
    if (tid == 0) {
        int64_t *o = counts + (int64_t)q * (a.n_groups + 5) + a.n_groups + 2;
        o[0] = (int64_t)covered; o[1] = (int64_t)tot[0]; o[2] = (int64_t)tot[1];
    }
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" int lgcn_eval_pop_metrics(const int32_t *topk_items, int32_t n_eval, int32_t K,
                                     const int64_t *test_indptr, const int32_t *test_items_sorted,
                                     const uint32_t *item_info, int32_t m_items, int32_t n_groups,
                                     const int32_t *ks, int32_t n_ks,
                                     double *sums_f64, int64_t *counts_i64, int64_t *group_slots,
                                     int32_t *exposure, double *per_slot, void *stream) {
    if (n_groups < 1 || n_groups > 8) { lgcn_set_error("lgcn_eval_pop_metrics: n_groups must be in 1..8"); return 3; }
    if (n_ks < 1 || n_ks > 8) { lgcn_set_error("lgcn_eval_pop_metrics: n_ks must be in 1..8"); return 3; }
    if (K < 1 || K > lgcn_eval_kmax()) { lgcn_set_error("lgcn_eval_pop_metrics: K must be in 1..lgcn_eval_kmax()"); return 3; }
    if (n_eval < 0) { lgcn_set_error("lgcn_eval_pop_metrics: n_eval is negative"); return 3; }
    if (m_items < 1) { lgcn_set_error("lgcn_eval_pop_metrics: m_items must be positive"); return 3; }
    if (!ks) { lgcn_set_error("lgcn_eval_pop_metrics: ks is NULL"); return 3; }
    if (!topk_items) { lgcn_set_error("lgcn_eval_pop_metrics: topk_items is NULL"); return 3; }
    if (!test_indptr) { lgcn_set_error("lgcn_eval_pop_metrics: test_indptr is NULL"); return 3; }
    if (!test_items_sorted) { lgcn_set_error("lgcn_eval_pop_metrics: test_items_sorted is NULL"); return 3; }
    if (!item_info) { lgcn_set_error("lgcn_eval_pop_metrics: item_info is NULL"); return 3; }
    if (!sums_f64) { lgcn_set_error("lgcn_eval_pop_metrics: sums_f64 is NULL"); return 3; }
    if (!counts_i64) { lgcn_set_error("lgcn_eval_pop_metrics: counts_i64 is NULL"); return 3; }
    if (!group_slots) { lgcn_set_error("lgcn_eval_pop_metrics: group_slots is NULL"); return 3; }
    PopArgs a{};
    for (int q = 0; q < n_ks; q++) {
        if (ks[q] < 1 || ks[q] > K) { lgcn_set_error("lgcn_eval_pop_metrics: a cut-off in ks is outside 1..K"); return 3; }
        a.ks[q] = ks[q];
        int b = q;                                          // insertion into the sorted copy
        while (b > 0 && a.sk[b - 1] > ks[q]) { a.sk[b] = a.sk[b - 1]; b--; }
        a.sk[b] = ks[q];
    }
    // the Gini numerator is at most m_items * sum of e <= m_items * n_eval * K: refused where that could leave int64
    if (n_eval > 0 && (int64_t)n_eval * K > ((((int64_t)1) << 62) - 1) / m_items) {
        lgcn_set_error("lgcn_eval_pop_metrics: n_eval * K * m_items reaches 2^62"); return 3;
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t sums_b = sizeof(double) * (size_t)n_ks * 2 * n_groups, counts_b = sizeof(int64_t) * (size_t)n_ks * (n_groups + 5);
    const size_t expo_b = sizeof(int32_t) * (size_t)n_ks * (size_t)m_items;
    if (n_eval == 0) {
        if (hipMemsetAsync(sums_f64, 0, sums_b, st) != hipSuccess || hipMemsetAsync(counts_i64, 0, counts_b, st) != hipSuccess ||
            hipMemsetAsync(group_slots, 0, sizeof(int64_t) * (size_t)n_groups, st) != hipSuccess ||
            (exposure && hipMemsetAsync(exposure, 0, expo_b, st) != hipSuccess)) {
            (void)hipGetLastError();
            lgcn_set_error("lgcn_eval_pop_metrics: memset failed"); return 10;
        }
        return 0;
    }
    const int LG = K <= 32 ? 32 : 64, nsub = 4 * (64 / LG);
    int64_t nwg64 = ((int64_t)n_eval + nsub - 1) / nsub;
    const int nwg = (int)(nwg64 > POP_WG_MAX ? POP_WG_MAX : nwg64);
    // one stream-ordered allocation: the histogram (zeroed) | the buckets when the caller keeps no exposure (zeroed) | partials
    const size_t hist_b = up256(sizeof(int32_t) * (size_t)n_ks * ((size_t)n_eval + 1));
    const size_t bucket_b = exposure ? 0 : up256(expo_b);
    const size_t pf_b = up256(sizeof(double) * (size_t)nwg * POP_FW), pi_b = up256(sizeof(u64) * (size_t)nwg * POP_IW);
    char *tmp = nullptr;
    if (hipMallocAsync((void **)&tmp, hist_b + bucket_b + pf_b + pi_b, st) != hipSuccess) {
        (void)hipGetLastError();
        lgcn_set_error("lgcn_eval_pop_metrics: cannot allocate the temporaries"); return 4;
    }
    int32_t *hist = (int32_t *)tmp;
    a.bucket = exposure ? exposure : (int32_t *)(tmp + hist_b);
    a.part_f = (double *)(tmp + hist_b + bucket_b);
    a.part_i = (u64 *)(tmp + hist_b + bucket_b + pf_b);
    a.topk = topk_items; a.n_eval = n_eval; a.K = K; a.test_ptr = test_indptr; a.test_idx = test_items_sorted;
    a.info = item_info; a.m_items = m_items; a.n_groups = n_groups; a.n_ks = n_ks; a.per_slot = per_slot;
    int rc = 0;
    if (hipMemsetAsync(tmp, 0, hist_b + bucket_b, st) != hipSuccess || (exposure && hipMemsetAsync(exposure, 0, expo_b, st) != hipSuccess)) {
        (void)hipGetLastError();
        lgcn_set_error("lgcn_eval_pop_metrics: memset failed"); rc = 10;
    } else {
        if (LG == 32) hipLaunchKernelGGL(k_pop_slots<32>, dim3((unsigned)nwg), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_pop_slots<64>, dim3((unsigned)nwg), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_pop_sum, dim3(1), dim3(1024), 0, st, a, (int32_t)nwg, sums_f64, counts_i64, group_slots);
        hipLaunchKernelGGL(k_pop_items, dim3((unsigned)(((int64_t)m_items + 255) / 256)), dim3(256), 0, st, a, exposure, hist);
        hipLaunchKernelGGL(k_pop_gini, dim3((unsigned)n_ks), dim3(1024), 0, st, a, (const int32_t *)hist, counts_i64);
        if (hipGetLastError() != hipSuccess) { lgcn_set_error("lgcn_eval_pop_metrics: launch failed"); rc = 10; }
    }
    (void)hipFreeAsync(tmp, st);
    return rc;
}

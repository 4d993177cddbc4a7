// lgcn_eval_ranks.hip -- rank-based fused evaluation for gfx950: for every (evaluation slot, test item) the number of
// candidate items that score above it / equal to it, and from those counts precision / recall / NDCG at ANY cut-off, AUC
// (utils.AUC, utils.py:203-209) and MRR.
//
// The item sweep is lgcn_eval_sweep.h's: a workgroup of NW waves x 32 users, the users' rows in registers as the B operand, item
// tiles of 32 rows double-buffered through LDS, a user on a lane pair with 16 of the tile's scores in each lane's registers.
// It is the sweep of k_eval_topk with another consumer: no list, no insertion, no merge.  A user's test scores and two int32
// counters per test item live in LDS; per tile a lane compares its 16 unmasked scores with each test score of its user.
// The counts are integers, added in any order: the result does not depend on the split of the sweep and is bitwise
// reproducible.  The cost does not depend on a cut-off.
//
// Definitions (slot s, user u, train positives P_u, test list T_u ascending, L_u[j] = <E[u], E[n_users + j]> or -1024 for
// j in P_u -- Procedure.py:177-181):
//   score[t] = L_u[t]                                     (k_eval_test_scores)
//   gt[t]    = #{ j not in P_u or T_u : L_u[j] >  score[t] }      (k_eval_ranks)
//   eq[t]    = #{ j not in P_u or T_u : L_u[j] == score[t] }
// Everything else is closed form on these plus |P_u \ T_u| (those items sit at -1024) and compares among score[] itself, so
// the two kernels never need bitwise-equal arithmetic (k_eval_rank_metrics).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "lgcn_eval_sweep.h"

namespace {

#define RANKS_NEG_INF (-3.0e38f)
#ifndef EVAL_RANKS_TB
#define EVAL_RANKS_TB 64                /* test items of a user held in LDS per pass of the sweep (the LDS budget per user) */
#endif
#define RANKS_TB EVAL_RANKS_TB
#ifndef EVAL_RANKS_PARTS
#define EVAL_RANKS_PARTS 0              /* workgroups per user block (0: from the grid size, see lgcn_eval_ranks) */
#endif
#define RANKS_MAX_PARTS 32
#define RANKS_LDS_BYTES (160 * 1024)

struct RankArgs {
    const float *E; int32_t n_users, m_items, d;
    const int32_t *users; int32_t n_eval;
    const int64_t *train_ptr; const int32_t *train_idx;
    const int64_t *test_ptr; const int32_t *test_idx; int64_t n_test;
    float *score; int32_t *gt, *eq;
};

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

// ---- score[t] for every (slot, test item): 16 lanes per pair, each a contiguous run of d / 16 elements summed in order, then a
//      fixed xor tree over the 16 partial sums; -1024 when t is also a train positive (binary search of the sorted CSR row)
__global__ void __launch_bounds__(256) k_eval_test_scores(RankArgs a) {
    const int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int l = threadIdx.x & 15;
    const bool live = p < a.n_test;
    float acc = 0.f;
    bool masked = true;
    if (live) {
        int64_t lo = 0, hi = a.n_eval;                       // the slot: the last s with test_ptr[s] <= p
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.test_ptr[mid + 1] <= p) lo = mid + 1; else hi = mid; }
        const int32_t item = a.test_idx[p];
        if (lo < a.n_eval && item >= 0 && item < a.m_items) {
            const int32_t u = a.users[lo];
            const int64_t pb = a.train_ptr[u], pe = a.train_ptr[u + 1];
            const int64_t q = csr_lower_bound(a.train_idx, pb, pe, item);
            masked = q < pe && a.train_idx[q] == item;
            const int run = a.d / 16;
            const float *up = a.E + (int64_t)u * a.d + l * run, *ip = a.E + ((int64_t)a.n_users + item) * a.d + l * run;
            for (int k = 0; k < run; k++) acc = fmaf(up[k], ip[k], acc);
        }
    }
    for (int off = 8; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 16);
    if (live && l == 0) a.score[p] = masked ? -1024.0f : acc;            // Procedure.py:181
}

template <int D, bool SPLIT3, int NW> struct RankShape {
    static constexpr int TILE_F = SweepGeo<D, SPLIT3>::TILE_F;
    static constexpr int lds = 2 * TILE_F * 4 + 32 * NW * ((RANKS_TB + 1) + (2 * RANKS_TB + 1)) * 4 + 64;
};

// ---- the sweep.  gt / eq must be zero on entry: every workgroup ADDS its counts (integer atomics, no merge kernel).
template <int D, bool SPLIT3, int NW>
__global__ void __launch_bounds__(64 * NW, 1) k_eval_ranks(RankArgs a) {
    constexpr int NT = 64 * NW, NU = 32 * NW, TB = RANKS_TB;
    static_assert(RankShape<D, SPLIT3, NW>::lds <= RANKS_LDS_BYTES, "test scores + counters + item tiles exceed the LDS of a CU");
    constexpr int TILE_F = SweepGeo<D, SPLIT3>::TILE_F;
    __shared__ __attribute__((aligned(16))) float tile_lds[2][TILE_F];
    __shared__ float ts_lds[NU][TB + 1];                    // the user's test scores of this pass (odd stride: no bank conflict)
    __shared__ uint32_t cnt_lds[NU][2 * TB + 1];            // [2 k] = gt, [2 k + 1] = eq of test item k of this pass
    __shared__ int32_t wmax_lds[NW];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const float *items = a.E + (int64_t)a.n_users * D;

    const int64_t slot = (int64_t)blockIdx.x * NU + wid * 32 + j;
    const bool have = slot < a.n_eval;
    const int32_t uid = have ? a.users[slot] : 0;
    SweepUser<D, SPLIT3> ub;                                // this lane's user: half a row in registers (B operand)
    ub.load(a.E + (int64_t)uid * D, h);
    // ---- the user's test list, and the passes the workgroup needs: ceil(longest list / TB)
    int64_t tb0 = 0, te0 = 0;
    if (have) { tb0 = clamp64(a.test_ptr[slot], 0, a.n_test); te0 = clamp64(a.test_ptr[slot + 1], tb0, a.n_test); }
    const int64_t len64 = te0 - tb0;
    const int32_t len = len64 > 0x7fffffff ? 0x7fffffff : (int32_t)len64;
    int32_t wmax = len;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int32_t o = __shfl_xor(wmax, off); wmax = o > wmax ? o : wmax; }
    if (lane == 0) wmax_lds[wid] = wmax;
    __syncthreads();
    int32_t gmax = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) gmax = wmax_lds[w] > gmax ? wmax_lds[w] : gmax;
    const int npass = (int)(((int64_t)gmax + TB - 1) / TB);
    // ---- the exclusion cursors: the lower lane of a pair walks the user's train positives, the upper one its test list
    const int32_t *cl = h == 0 ? a.train_idx : a.test_idx;
    int64_t c_begin = 0, c_end = 0;
    if (have) {
        if (h == 0) { c_begin = a.train_ptr[uid]; c_end = a.train_ptr[uid + 1]; }
        else { c_begin = tb0; c_end = te0; }
    }
    const int ntiles_all = (a.m_items + 31) / 32;
    const int t_begin = (int)((int64_t)ntiles_all * blockIdx.y / gridDim.y), t_end = (int)((int64_t)ntiles_all * (blockIdx.y + 1) / gridDim.y);
    if (t_begin >= t_end) return;
    const int ul = wid * 32 + j;

    SweepStage<D, NT> stage;
    for (int pass = 0; pass < npass; pass++) {
        const int32_t p0 = pass * TB;
        const int32_t mine = len - p0 < 0 ? 0 : len - p0 > TB ? TB : len - p0;          // my user's test items of this pass
        const int32_t trip = wmax - p0 < 0 ? 0 : wmax - p0 > TB ? TB : wmax - p0;       // the wave's compare loop
        for (int k = h; k < TB; k += 2) {
            ts_lds[ul][k] = k < mine ? a.score[tb0 + p0 + k] : 3.0e38f;                 // (nothing is above or equal to the filler)
            cnt_lds[ul][2 * k] = 0u; cnt_lds[ul][2 * k + 1] = 0u;
        }
        int64_t cp = c_begin;
        if (t_begin > 0) cp = csr_lower_bound(cl, c_begin, c_end, t_begin * 32);
        int32_t nid = cp < c_end ? cl[cp] : 0x7fffffff;
        sweep_load_tile(stage, items, a.m_items, t_begin, tid);
        sweep_store_tile<D, SPLIT3>(stage, tile_lds, t_begin & 1, tid);
        __syncthreads();
        for (int t = t_begin; t < t_end; t++) {
            const int buf = t & 1;
            if (t + 1 < t_end) sweep_load_tile(stage, items, a.m_items, t + 1, tid);                // in flight under this tile's work
            const int base = t * 32;
            if (trip > 0) {                                     // (wave-uniform: a wave whose lists are done only moves tiles)
                // ---- the tile's exclusion word of my user: P_u | T_u
                uint32_t m1 = 0;
                while (nid < base + 32) {
                    if (nid >= base) m1 |= 1u << (nid - base);
                    cp++;
                    nid = cp < c_end ? cl[cp] : 0x7fffffff;
                }
                const u32x2 mm = __builtin_amdgcn_permlane32_swap(m1, m1, false, false);
                const uint32_t mask = mm.x | mm.y;
                // ---- 32 items x 32 users
                f32x16 acc = ub.scores(tile_lds[buf], j, h);
                // ---- my 16 scores (item row = mfma32_row(reg, h)): excluded items and rows past the table drop
                //      below every test score, once per tile; the compare loop itself is then two compares per score
                const bool edge = base + 32 > a.m_items;
                if (edge || __any(mask != 0u)) {
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) {
                        const int row = mfma32_row(reg, h);
                        if (((mask >> row) & 1u) || base + row >= a.m_items) acc[reg] = RANKS_NEG_INF;
                    }
                }
                for (int k = 0; k < trip; k++) {
                    const float ts = ts_lds[ul][k];
                    uint32_t g = 0, e = 0;
#pragma unroll
                    for (int reg = 0; reg < 16; reg++) { g += acc[reg] > ts ? 1u : 0u; e += acc[reg] == ts ? 1u : 0u; }
                    // the pair's counts: the lower lane adds gt, the upper one eq -- no two lanes touch one counter
                    const uint32_t v = g | (e << 8);
                    const u32x2 vv = __builtin_amdgcn_permlane32_swap(v, v, false, false);
                    const uint32_t sum = vv.x + vv.y;
                    const uint32_t add = h ? sum >> 8 : sum & 0xffu;
                    if (add) cnt_lds[ul][2 * k + h] += add;
                }
            }
            if (t + 1 < t_end) sweep_store_tile<D, SPLIT3>(stage, tile_lds, buf ^ 1, tid);
            __syncthreads();
        }
        // ---- this pass's counts into the global counters (each lane its own entries: written by this lane alone)
        for (int k = 0; k < mine; k++) {
            const uint32_t c = cnt_lds[ul][2 * k + h];
            if (c) atomicAdd((h ? a.eq : a.gt) + tb0 + p0 + k, (int32_t)c);
        }
        __syncthreads();
    }
}

// ---- metrics from (score, gt, eq): one workgroup per slot.
//   pos[t] = gt[t] + eq[t]                        a tie with a non-test item goes against the test item
//          + |P_u \ T_u| if score[t] <= -1024     the train positives sit at -1024
//          + c[t],  c[t] = #{t' in T_u : score[t'] > score[t], or equal with a lower id}      ties among test items: lower id first
// c[] is a permutation of 0..n-1 (the test items in ranked order), so pos is scattered to sorted[c[t]] and one thread adds the
// hits, DCG and ideal DCG rank by rank -- the additions of k_eval_metrics_ex in its order.
struct RankMetricArgs {
    int32_t n_eval, m_items;
    const int32_t *users; const int64_t *train_ptr; const int32_t *train_idx;
    const int64_t *test_ptr; const int32_t *test_idx; int64_t n_test;
    const float *score; const int32_t *gt, *eq;
    int32_t ks[8]; int32_t n_ks;
    int32_t *sorted;                                        // [n_test] temporary
    double *per_user;                                       // [n_eval, 3 n_ks + 2]: precision | recall | ndcg | auc | mrr
};

__global__ void __launch_bounds__(256) k_eval_rank_metrics(RankMetricArgs a) {
    const int64_t s = blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ int32_t inter;
    __shared__ unsigned long long auc2;
    const int64_t b = clamp64(a.test_ptr[s], 0, a.n_test), e = clamp64(a.test_ptr[s + 1], b, a.n_test);
    const int64_t n = e - b, m = a.m_items;
    const int32_t u = a.users[s];
    const int64_t pb = a.train_ptr[u], pe = a.train_ptr[u + 1];
    if (tid == 0) { inter = 0; auc2 = 0ull; }
    __syncthreads();
    int32_t mine = 0;
    for (int64_t i = tid; i < n; i += 256) {
        const int32_t it = a.test_idx[b + i];
        const int64_t q = csr_lower_bound(a.train_idx, pb, pe, it);
        mine += q < pe && a.train_idx[q] == it;
    }
    if (mine) atomicAdd(&inter, mine);
    __syncthreads();
    const int64_t pnt = (pe - pb) - inter;                  // |P_u \ T_u|
    const int64_t rest = m - n - pnt;                       // the items the sweep counted over
    unsigned long long part2 = 0ull;
    for (int64_t i = tid; i < n; i += 256) {
        const float sc = a.score[b + i];
        const int64_t g = a.gt[b + i], q = a.eq[b + i];
        int64_t c = 0;
        for (int64_t i2 = 0; i2 < n; i2++) { const float s2 = a.score[b + i2]; c += (s2 > sc || (s2 == sc && i2 < i)) ? 1 : 0; }
        const int64_t pos = g + q + (sc <= -1024.0f ? pnt : 0) + c;
        a.sorted[b + c] = (int32_t)pos;
        const int64_t less = rest - g - q + (sc > -1024.0f ? pnt : 0), same = q + (sc == -1024.0f ? pnt : 0);
        part2 += (unsigned long long)(2 * less + same);
    }
    if (part2) atomicAdd(&auc2, part2);
    __syncthreads();
    if (tid != 0) return;
    const int W = 3 * a.n_ks + 2;
    double *o = a.per_user + s * W;
    for (int q = 0; q < a.n_ks; q++) {
        const int64_t k = a.ks[q];
        double right = 0.0, dcg = 0.0, idcg = 0.0;
        for (int64_t i = 0; i < n; i++) {
            const int64_t p = a.sorted[b + i];
            if (p >= k) break;
            right += 1.0; dcg += 1.0 / log2((double)(p + 2));
        }
        const int64_t top = n < k ? n : k;
        for (int64_t r = 0; r < top; r++) idcg += 1.0 / log2((double)(r + 2));
        if (idcg == 0.0) idcg = 1.0;
        o[q] = right / (double)k;                           // utils.py:173-187
        o[a.n_ks + q] = n > 0 ? right / (double)n : 0.0;
        o[2 * a.n_ks + q] = dcg / idcg;                     // utils.py:190-203
    }
    // roc_auc_score(r_all, L_u): Mann-Whitney with ties counted half, over the n (m - n) (test, non-test) pairs
    o[3 * a.n_ks] = (n > 0 && n < m) ? (double)auc2 / (2.0 * (double)n * (double)(m - n)) : 0.0;
    o[3 * a.n_ks + 1] = n > 0 ? 1.0 / (1.0 + (double)a.sorted[b]) : 0.0;
}

template <int D, bool SPLIT3, int NW>
void launch_ranks(const RankArgs &a, int parts, hipStream_t st) {
    const dim3 grid((unsigned)((a.n_eval + 32 * NW - 1) / (32 * NW)), (unsigned)parts);
    hipLaunchKernelGGL((k_eval_ranks<D, SPLIT3, NW>), grid, dim3(64 * NW), 0, st, a);
}

}  // namespace

extern "C" int lgcn_eval_ranks(const float *E, int32_t n_users, int32_t m_items, int32_t d, const int32_t *users, int32_t n_eval,
                               const int64_t *train_indptr, const int32_t *train_indices,
                               const int64_t *test_indptr, const int32_t *test_items_sorted, int64_t n_test,
                               float *test_scores, int32_t *gt, int32_t *eq, int32_t flags, void *stream) {
    if (n_users <= 0 || m_items <= 0 || n_eval < 0 || n_test < 0 || (flags & ~LGCN_EVAL_FP32)) {
        lgcn_set_error("lgcn_eval_ranks: invalid argument"); return 3;
    }
    if (d != 32 && d != 64 && d != 128 && d != 256) { lgcn_set_error("embedding dim must be 32, 64, 128 or 256"); return 3; }
    if (n_test > (int64_t)n_eval * m_items) { lgcn_set_error("lgcn_eval_ranks: n_test exceeds n_eval * m_items"); return 3; }
    if (!E || !users || !train_indptr || !train_indices || !test_indptr || (n_test > 0 && (!test_items_sorted || !test_scores || !gt || !eq))) {
        lgcn_set_error("lgcn_eval_ranks: invalid argument"); return 3;
    }
    if (n_eval == 0 || n_test == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    RankArgs a{E, n_users, m_items, d, users, n_eval, train_indptr, train_indices, test_indptr, test_items_sorted, n_test, test_scores, gt, eq};
    if (hipMemsetAsync(gt, 0, sizeof(int32_t) * (size_t)n_test, st) != hipSuccess || hipMemsetAsync(eq, 0, sizeof(int32_t) * (size_t)n_test, st) != hipSuccess) {
        lgcn_set_error("lgcn_eval_ranks: memset failed"); return 10;
    }
    hipLaunchKernelGGL(k_eval_test_scores, dim3((unsigned)((n_test + 15) / 16)), dim3(256), 0, st, a);
    // One workgroup per CU (the counters and test scores of 128 users are ~97 KB of LDS), and the work of a workgroup is
    // (passes of its longest list) x (tiles) x (its waves' longest lists): uneven by an order of magnitude between user blocks.
    // So the sweep is cut into many parts of >= 32 tiles (<= 32 parts) and the hardware's workgroup scheduler balances them;
    // the parts add into the same global counters.  (Gowalla, measured: 1 / 2 / 4 parts = 92 / 50 / 27 ms with the slots by list
    // length -- the kernel's time was its heaviest workgroup's.)
    const int ntiles = (m_items + 31) / 32;
    int parts = EVAL_RANKS_PARTS;
    if (parts <= 0) parts = ntiles / 32;
    if (parts > RANKS_MAX_PARTS) parts = RANKS_MAX_PARTS;
    if (parts > ntiles) parts = ntiles;
    if (parts < 1) parts = 1;
    const bool split3 = !(flags & LGCN_EVAL_FP32);
    switch (d) {
    case 32: if (split3) launch_ranks<32, true, 4>(a, parts, st); else launch_ranks<32, false, 4>(a, parts, st); break;
    case 64: if (split3) launch_ranks<64, true, 4>(a, parts, st); else launch_ranks<64, false, 4>(a, parts, st); break;
    case 128: if (split3) launch_ranks<128, true, 4>(a, parts, st); else launch_ranks<128, false, 4>(a, parts, st); break;
    default: launch_ranks<256, false, 2>(a, parts, st); break;      // (six planes of both operands: more than 512 registers)
    }
    if (hipGetLastError() != hipSuccess) { lgcn_set_error("lgcn_eval_ranks: launch failed"); return 10; }
    return 0;
}

extern "C" int lgcn_eval_rank_metrics(int32_t n_eval, int32_t m_items, const int32_t *users,
                                      const int64_t *train_indptr, const int32_t *train_indices,
                                      const int64_t *test_indptr, const int32_t *test_items_sorted, int64_t n_test,
                                      const float *test_scores, const int32_t *gt, const int32_t *eq,
                                      const int32_t *ks, int32_t n_ks, double *per_user, double *sums, void *stream) {
    if (n_eval < 0 || m_items <= 0 || n_test < 0 || n_ks < 1 || n_ks > 8 || !ks) { lgcn_set_error("lgcn_eval_rank_metrics: invalid argument"); return 3; }
    if (n_test > (int64_t)n_eval * m_items) { lgcn_set_error("lgcn_eval_rank_metrics: n_test exceeds n_eval * m_items"); return 3; }
    RankMetricArgs a{};
    for (int q = 0; q < n_ks; q++) {
        if (ks[q] < 1 || ks[q] > m_items) { lgcn_set_error("lgcn_eval_rank_metrics: a cut-off outside 1..m_items"); return 3; }
        a.ks[q] = ks[q];
    }
    if (!users || !train_indptr || !train_indices || !test_indptr || !per_user || !sums ||
        (n_test > 0 && (!test_items_sorted || !test_scores || !gt || !eq))) {
        lgcn_set_error("lgcn_eval_rank_metrics: invalid argument"); return 3;
    }
    a.n_eval = n_eval; a.m_items = m_items; a.users = users; a.train_ptr = train_indptr; a.train_idx = train_indices;
    a.test_ptr = test_indptr; a.test_idx = test_items_sorted; a.n_test = n_test; a.score = test_scores; a.gt = gt; a.eq = eq;
    a.n_ks = n_ks; a.per_user = per_user;
    hipStream_t st = (hipStream_t)stream;
    void *tmp = nullptr;
    if (n_eval > 0) {
        if (hipMallocAsync(&tmp, sizeof(int32_t) * (size_t)(n_test > 0 ? n_test : 1), st) != hipSuccess) {
            (void)hipGetLastError();
            lgcn_set_error("lgcn_eval_rank_metrics: cannot allocate the ranked positions"); return 4;
        }
        a.sorted = (int32_t *)tmp;
        hipLaunchKernelGGL(k_eval_rank_metrics, dim3((unsigned)n_eval), dim3(256), 0, st, a);
        (void)hipFreeAsync(tmp, st);
    }
    lgcn_eval_sum_launch(per_user, n_eval, 3 * n_ks + 2, sums, st);
    if (hipGetLastError() != hipSuccess) { lgcn_set_error("lgcn_eval_rank_metrics: launch failed"); return 10; }
    return 0;
}

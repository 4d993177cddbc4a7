// lgcn_eval.hip -- fused full-ranking evaluation for gfx950.
//
// Replaces, for one launch over all test users (reference: LightGCN_work/code):
//   model.py:114-123      getUsersRating: rating = U_b . I^T  (the reference re-propagates per 100 users;
//                         here the propagated table comes in once from lgcn_propagate_mean)
//   Procedure.py:177-181  rating[train positives] = -(1<<10)
//   Procedure.py:183      torch.topk(rating, k=max(topks))
//   Procedure.py:89-121 + utils.py:173-217   per-user hits, precision / recall / NDCG, summed over users
// without ever materialising the [users, m_items] score matrix.
//
// k_eval_topk: the one dense contraction of the system -> matrix cores.  fp32 in / fp32 accumulate
// (v_mfma_f32_32x32x2_f32: exact f32, 64 FLOP/clk/SIMD) so the ranking is the reference's fp32 ranking.
//   * workgroup = 4 waves x 32 users; the users' rows are the B operand and stay in registers for the
//     whole item sweep (D/2 VGPRs per lane: lane (j, h) holds elements [h*D/2, (h+1)*D/2) of user j --
//     the k order inside a dot product is free, so each half-row is one contiguous run);
//   * items stream through LDS in tiles of 32 rows (coalesced 16-byte global loads, double buffered,
//     rows padded by 16 B so the ds_read_b128 of 32 lanes at the same column hit different banks);
//     every wave multiplies the same item tile with its own users: D/2 MFMAs per 32 x 32 scores;
//   * the accumulator layout puts a user on a lane (col = lane & 31) and 16 of the tile's items in its
//     registers, so the train-positive mask is a 32-bit word per user (built one tile ahead from the
//     sorted train CSR by a cursor whose next entry is always already loaded) and the running top-K
//     is per lane: a threshold compare per score marks the candidates of a tile, and only those touch the
//     lane's list in LDS (replace the minimum, rescan for the new minimum), one per round for all lanes
//     together.  The lists of the two lanes of a user are merged and sorted once at the end.
//     Order of the result: (score descending, item id ascending).  The list's key is the score alone: the entry replaced is
//     the FIRST slot holding the minimum, whatever its id, so of several items tying EXACTLY at the K-th score any may be
//     the ones kept (every item strictly above that score is kept).  Making (score, id) the key was measured and costs
//     3-13 % of the sweep (profiles/eval_topk_exact).
// What this file shares with lgcn_eval_ranks.hip is defined in lgcn_eval_sweep.h: the bf16 split, the tile geometry, the CSR search, the
// sums' launcher.  The operand, the tile stage and the score tile of k_eval_topk are still spelled below, and again in that header
// for k_eval_ranks (why: profiles/eval_sweep/README.md).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "lgcn_eval_sweep.h"

#define EVAL_KMAX 64
#define EVAL_NEG_INF (-3.0e38f)
#ifndef EVAL_PARTS
#define EVAL_PARTS 3          /* workgroups per user block (<= 4) = workgroups that fit a CU with the compact lists */
#endif
// Ids in the per-lane lists: int32 item ids, or (compact form) 16-bit offsets from the first item of the workgroup's
// part of the sweep -- 10 KB less LDS per workgroup, which is what lets a third workgroup share the CU.
template <typename IDT> struct ListId;
template <> struct ListId<int32_t> { static constexpr int32_t EMPTY = -1; static constexpr int PAD = 1; };
template <> struct ListId<uint16_t> { static constexpr uint16_t EMPTY = 0xffffu; static constexpr int PAD = 0; };
#ifndef EVAL_NBUF
#define EVAL_NBUF 2
#endif
#ifndef EVAL_PUB_TILES
#define EVAL_PUB_TILES 16        /* tiles between two exchanges of the parts' K-th best (a power of two; 0: never) */
#endif
#ifndef EVAL_SPLIT3
#define EVAL_SPLIT3 1          /* compact form: fp32 scores from six bf16 product planes (0: fp32 matrix instructions) */
#endif
#define EVAL_ID16_MAX_TILES 2047        /* 2047 * 32 + 31 < 0xffff */
#define EVAL_KMAX_EX 256                /* lgcn_eval_topk_ex: 64 < K <= 256 take the large-K sweep */
#define EVAL_LDS_BYTES (160 * 1024)     /* LDS of one CU */
#ifndef EVAL_BIG_PARTS
#define EVAL_BIG_PARTS 0                /* large-K sweep: parts per user block (0: from the grid size, see eval_topk_big) */
#endif

// LDS shape of one k_eval_topk instantiation: NW waves = 32 NW users, one list of KS slots per user, NBUF item tiles.
// The large-K lists (KS > 64) pad each score row by 16 bytes, so the 16-byte reads of 16 lanes at one column start 4 banks
// apart; the K <= 64 lists keep their shape.
template <int D, int KS, typename IDT, int NW, bool SPLIT3> struct EvalShape {
    static constexpr int TILE_F = SweepGeo<D, SPLIT3>::TILE_F;              // floats per item tile
    static constexpr int KSP = (KS + 7) / 8 * 8;
    static constexpr int KSPP = KS > EVAL_KMAX ? KSP + 4 : KSP;             // score row stride (floats)
    static constexpr int USERS = 32 * NW;
    static constexpr int lds(int nbuf) {
        return nbuf * TILE_F * 4 + USERS * KSPP * 4 + USERS * (KS + (sizeof(IDT) == 4 ? 1 : 0)) * (int)sizeof(IDT);
    }
};

struct EvalArgs {
    const float *E; int32_t n_users, m_items;
    const int32_t *users; int32_t n_eval;
    const int64_t *train_ptr; const int32_t *train_idx;
    int32_t K;
    int32_t *out_items; float *out_scores;
    // the item sweep split over gridDim.y workgroups per user block (two co-resident workgroups per CU overlap
    // one's list maintenance with the other's MFMAs): each writes its sorted partial list here, k_eval_merge picks
    int32_t *part_items; float *part_scores;      // [n_eval, gridDim.y, K] or NULL (gridDim.y == 1: straight to out_*)
    // The parts of a user's sweep tell each other their K-th best so far ([gridDim.y][n_eval], NaN = nothing yet; or NULL):
    // K items at or above a part's K-th best exist, so every other part may use it as a floor for what it still inserts.
    // Any value ever published is valid, however stale -- the exchange only prunes, it never decides.
    float *thr_pub;
    // Optional: the train-positive masks precomputed once per dataset (lgcn_eval_build_masks): masks[t * mask_stride + slot] =
    // bit i set when item 32 t + i is a train positive of the user in evaluation slot `slot`.  With them the item sweep holds no
    // global load besides the tile stream and one coalesced 128-byte mask load per wave and tile, issued a tile ahead (the
    // cursor over the sorted train CSR costs a dependent load and a wait inside the loop).  NULL: the cursor.
    const uint32_t *masks; int64_t mask_stride;
};

// c ? hi : lo.  The empty asm keeps the compiler from folding a tree of these over vector elements into ONE dynamically
// indexed element, which it lowers through scratch memory or an LDS copy of the vector.
static __device__ __forceinline__ float pick(bool c, float hi, float lo) {
    asm volatile("" : "+v"(hi), "+v"(lo));
    return c ? hi : lo;
}

template <int D, int KS, typename IDT, int WGS, int NBUF = 2, bool SPLIT3 = false, bool MASKS = false, int NW = 4>
                                                                // KS: list slots per lane (a multiple of 4, >= K); WGS: workgroups per CU;
                                                                // NBUF: item tile buffers in LDS (1: one more barrier per tile); NW: waves
__global__ void __launch_bounds__(64 * NW, WGS) k_eval_topk(EvalArgs a) {
    constexpr int NT = 64 * NW, NU = 32 * NW;          // threads, users of the workgroup
    static_assert(EvalShape<D, KS, IDT, NW, SPLIT3>::lds(NBUF) <= EVAL_LDS_BYTES, "lists + item tiles exceed the LDS of a CU");
    using G = SweepGeo<D, SPLIT3>;
    constexpr int HALF = G::HALF, RS = G::RS, RSB = G::RSB, NCH = G::NCH, PLANE_B = G::PLANE_B, TILE_F = G::TILE_F;
    constexpr int LPT = 32 * D * 4 / 16 / NT;           // 16-byte pieces per thread per item tile
    static_assert(LPT >= 1, "tile smaller than the workgroup");
    __shared__ __attribute__((aligned(16))) float tile_lds[NBUF][TILE_F];
    // per-lane candidate lists: KS slots (slots >= K hold +inf: never the minimum, never output),
    // 16-byte aligned rows so the minimum scan is KS/4 independent ds_read_b128
    // (row stride KS floats = 80 / 128 bytes: 16 lanes' 16-byte reads start 20 / 32 banks apart and cover the 64 banks once)
    constexpr int KSP = (KS + 7) / 8 * 8, KH = KSP / 2;       // slots padded so that each of a user's two lanes scans KH of them
    __shared__ __attribute__((aligned(16))) float list_s[NU][EvalShape<D, KS, IDT, NW, SPLIT3>::KSPP];
    __shared__ IDT list_i[NU][KS + ListId<IDT>::PAD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int K = a.K;
    const float *items = a.E + (int64_t)a.n_users * D;

    // ---- this lane's user: half a row in registers (B operand)
    const int64_t slot = (int64_t)blockIdx.x * NU + wid * 32 + j;
    const bool have = slot < a.n_eval;
    const int32_t uid = have ? a.users[slot] : 0;
    float b[SPLIT3 ? 1 : HALF];
    u32x4 bh[SPLIT3 ? NCH : 1], bm[SPLIT3 ? NCH : 1], bl[SPLIT3 ? NCH : 1];   // SPLIT3: k = 16 c + 8 h + [0, 8) of MFMA step c
    if constexpr (SPLIT3) {
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const float *up = a.E + (int64_t)uid * D + 16 * c + 8 * h;
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(up), v1 = *reinterpret_cast<const f32x4 *>(up + 4);
            const Planes2 p0 = split3(v0.x, v0.y), p1 = split3(v0.z, v0.w), p2 = split3(v1.x, v1.y), p3 = split3(v1.z, v1.w);
            bh[c] = u32x4{p0.h, p1.h, p2.h, p3.h}; bm[c] = u32x4{p0.m, p1.m, p2.m, p3.m}; bl[c] = u32x4{p0.l, p1.l, p2.l, p3.l};
        }
    } else {
        const float *up = a.E + (int64_t)uid * D + h * HALF;
#pragma unroll
        for (int s = 0; s < HALF; s += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(up + s);
            b[s] = v.x; b[s + 1] = v.y; b[s + 2] = v.z; b[s + 3] = v.w;
        }
    }
    // ---- train-positive cursor (lower lane of the pair walks it; the mask is shared with the upper one)
    int64_t tp = 0, tend = 0;
    int32_t nid = 0x7fffffff, nnid = 0x7fffffff;
    const int ntiles_all = (a.m_items + 31) / 32;
    const int t_begin = (int)((int64_t)ntiles_all * blockIdx.y / gridDim.y), t_end = (int)((int64_t)ntiles_all * (blockIdx.y + 1) / gridDim.y);
    uint32_t mask_next = 0;        // MASKS: this user's word of the NEXT tile, in flight under this tile's work
    const uint32_t slot32 = (uint32_t)slot;     // (uniform row base + one 32-bit lane offset: slots past n_eval read their padding column, zeros)
    if (MASKS) { if (t_begin < t_end) mask_next = (a.masks + (int64_t)t_begin * a.mask_stride)[slot32]; }
    else if (have && h == 0) {
        tp = a.train_ptr[uid]; tend = a.train_ptr[uid + 1];
        if (t_begin > 0 && tp < tend) tp = csr_lower_bound(a.train_idx, tp, tend, t_begin * 32);       // first train positive inside this workgroup's item range
        if (tp < tend) nid = a.train_idx[tp];
        if (tp + 1 < tend) nnid = a.train_idx[tp + 1];
    }
    const int ul = wid * 32 + j;                               // the user's list (shared by its two lanes)
    if (h == 0) for (int k = 0; k < KSP; k++) { list_s[ul][k] = k < K ? EVAL_NEG_INF : 3.0e38f; if (k < KS) list_i[ul][k] = ListId<IDT>::EMPTY; }
    const int id0 = sizeof(IDT) == 2 ? t_begin * 32 : 0;       // list ids are stored relative to this
    float thr = EVAL_NEG_INF;      // the user's K-th best so far (the same value in both lanes), or the other parts' if that is higher
    int pmin = 0;                  // where it sits in the list

    // piece p of a tile: item row p / (D/4), 16-byte column p % (D/4)
    f32x4 pre[LPT];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int q = 0; q < LPT; q++) {
            const int p = tid + q * NT, r = p / (D / 4), c = p % (D / 4);
            const int64_t item = (int64_t)t * 32 + r;
            pre[q] = item < a.m_items ? *reinterpret_cast<const f32x4 *>(items + item * D + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_tile = [&](int buf) {
#pragma unroll
        for (int q = 0; q < LPT; q++) {
            const int p = tid + q * NT, r = p / (D / 4), c = p % (D / 4);
            if constexpr (SPLIT3) {                             // split once per workgroup, not once per wave
                const Planes2 p0 = split3(pre[q].x, pre[q].y), p1 = split3(pre[q].z, pre[q].w);
                char *dst = reinterpret_cast<char *>(tile_lds[buf]) + (r * RSB + 4 * c) * 2;
                *reinterpret_cast<uint2 *>(dst) = make_uint2(p0.h, p1.h);
                *reinterpret_cast<uint2 *>(dst + PLANE_B) = make_uint2(p0.m, p1.m);
                *reinterpret_cast<uint2 *>(dst + 2 * PLANE_B) = make_uint2(p0.l, p1.l);
            } else {
                *reinterpret_cast<f32x4 *>(&tile_lds[buf][r * RS + c * 4]) = pre[q];
            }
        }
    };
    load_tile(t_begin);
    store_tile(NBUF == 2 ? t_begin & 1 : 0);
    __syncthreads();
    typedef __attribute__((address_space(1))) float gf32;
    for (int t = t_begin; t < t_end; t++) {
        const int buf = NBUF == 2 ? t & 1 : 0;
        if (a.thr_pub && have && ((t - t_begin) & (EVAL_PUB_TILES - 1)) == EVAL_PUB_TILES - 1) {
            // (agent-scope accesses: the parts run on different XCDs, whose L2s do not see each other's plain stores)
            if (h == 0) __hip_atomic_store((gf32 *)(a.thr_pub + (int64_t)blockIdx.y * a.n_eval + slot), thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int q = 0; q < (int)gridDim.y; q++)
                if (q != (int)blockIdx.y)
                    thr = fmaxf(thr, __hip_atomic_load((gf32 *)(a.thr_pub + (int64_t)q * a.n_eval + slot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));   // fmaxf drops a NaN
        }
        if (t + 1 < t_end) load_tile(t + 1);                   // in flight under this tile's MFMAs
        // ---- mask of this tile's train positives for my user
        const int base = t * 32;
        uint32_t mask = 0;
        if (MASKS) {
            mask = mask_next;                                   // both lanes of the user load the same word
            if (t + 1 < t_end) mask_next = (a.masks + (int64_t)(t + 1) * a.mask_stride)[slot32];
        } else {
            while (nid < base + 32) {                           // nid >= base always: tiles ascend
                mask |= 1u << (nid - base);
                nid = nnid; tp++;
                nnid = (tp + 1 < tend) ? a.train_idx[tp + 1] : 0x7fffffff;
            }
            mask = __shfl(mask, j);                             // lane j (h = 0) holds the user's mask
        }
        // ---- 32 items x 32 users: scores[item i][user j] = sum_k I[i][k] U[j][k]
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if constexpr (SPLIT3) {
            const char *arow = reinterpret_cast<const char *>(tile_lds[buf]) + (j * RSB + 8 * h) * 2;   // lane (i = j, h): k = 16 c + 8 h + [0, 8)
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
        } else {
            const float *arow = &tile_lds[buf][j * RS + h * HALF];  // A operand: lane (i = j, h) holds item i's half row
#pragma unroll
            for (int s = 0; s < HALF; s += 4) {
                const f32x4 av = *reinterpret_cast<const f32x4 *>(arow + s);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b[s], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b[s + 1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b[s + 2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b[s + 3], acc, 0, 0, 0);
            }
        }
        if (NBUF == 1) {                                        // every wave has read the tile: the next one may overwrite it
            __syncthreads();
            if (t + 1 < t_end) store_tile(0);
        }
        // ---- my 16 scores: item row = mfma32_row(reg, h).  First only MARK the ones that can
        //      enter the user's top K: above this lane's K-th best AND not below the partner lane's (the other
        //      half of the user's items: K items at or above that score already exist).  Then the marked scores
        //      are inserted one per round, all lanes together: the rounds of a tile are the LARGEST number of
        //      marked scores any lane of the workgroup has (the waves meet at the tile's barrier), not the number
        //      of score positions where some lane inserts -- mid-sweep that is 1-2 rounds instead of 5-10.
        uint32_t pend = 0;
        // The reference's semantics (a train positive's score IS -1024 and competes, Procedure.py:181; rows past the table do
        // not exist) cost three instructions per score.  They can only matter while some user with a train positive in this
        // tile has no K scores above -1024 yet, or in the table's last tile: everywhere else a train positive is simply
        // never marked.
        const bool exact_mask = base + 32 > a.m_items || __any(mask != 0u && !(thr >= -1024.0f));
        if (exact_mask) {
#pragma unroll
            for (int reg = 0; reg < 16; reg++) {
                const int row = mfma32_row(reg, h);
                float sc = acc[reg];
                if ((mask >> row) & 1u) sc = -1024.0f;                      // Procedure.py:181
                if (base + row >= a.m_items) sc = EVAL_NEG_INF;             // past the table
                acc[reg] = sc;
                if (sc > thr) pend |= 1u << reg;
            }
        } else {
#pragma unroll
            for (int reg = 0; reg < 16; reg++)
                if (acc[reg] > thr) pend |= 1u << reg;
            // my rows' bits of the train-positive mask, in register order: nibble g of the result = rows 8 g + 4 h + [0, 4)
            const uint32_t m2 = mask >> (4 * h);
            pend &= ~((m2 & 0xfu) | ((m2 >> 4) & 0xf0u) | ((m2 >> 8) & 0xf00u) | ((m2 >> 12) & 0xf000u));
        }
        // One list per USER: of its two lanes (the two halves of the tile's rows) at most one inserts per round, the lower
        // one first; then BOTH rescan half of the list each for the new K-th best and combine through v_permlane32_swap
        // (no LDS round trip, and neither lane idles during the scan).
        while (__any(pend != 0u)) {
            const uint32_t mine = pend != 0u ? 1u : 0u;
            const u32x2 mm = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);      // .x: lower lane's, .y: upper lane's
            const bool act = mine && (h == 0 || mm.x == 0u);
            uint32_t did = 0u;
            if (act) {
                const int reg = __builtin_ctz(pend);
                pend &= pend - 1u;
                // acc[reg] for a per-lane reg: a binary select tree (4 bit tests + 15 selects; a linear chain is 15 + 15)
                const bool b0 = reg & 1, b1 = reg & 2, b2 = reg & 4, b3 = reg & 8;
                const float e0 = pick(b0, acc[1], acc[0]), e1 = pick(b0, acc[3], acc[2]), e2 = pick(b0, acc[5], acc[4]), e3 = pick(b0, acc[7], acc[6]);
                const float e4 = pick(b0, acc[9], acc[8]), e5 = pick(b0, acc[11], acc[10]), e6 = pick(b0, acc[13], acc[12]), e7 = pick(b0, acc[15], acc[14]);
                const float f0 = pick(b1, e1, e0), f1 = pick(b1, e3, e2), f2 = pick(b1, e5, e4), f3 = pick(b1, e7, e6);
                const float sc = pick(b3, pick(b2, f3, f2), pick(b2, f1, f0));
                if (sc > thr) {                                         // thr may have risen since the marking
                    const int row = mfma32_row(reg, h);
                    list_s[ul][pmin] = sc; list_i[ul][pmin] = (IDT)(base + row - id0);
                    did = 1u;
                }
            }
            const u32x2 dd = __builtin_amdgcn_permlane32_swap(did, did, false, false);
            if (dd.x | dd.y) {
                // (the wave's LDS accesses execute in program order: the partner's write above is visible to these reads)
                f32x4 q[KH / 4];
#pragma unroll
                for (int k4 = 0; k4 < KH / 4; k4++) q[k4] = *reinterpret_cast<const f32x4 *>(&list_s[ul][h * KH + 4 * k4]);
                float m = q[0].x; int pm = 0;
                if constexpr (KS > EVAL_KMAX) {
                    // large K: four independent chains (one per vector component: slots 4 k4 + c), then the first slot of the
                    // smallest -- the serial scan's answer with a quarter of its dependent chain
                    float mc[4]; int pc[4];
#pragma unroll
                    for (int c = 0; c < 4; c++) { mc[c] = q[0][c]; pc[c] = c; }
#pragma unroll
                    for (int k4 = 1; k4 < KH / 4; k4++)
#pragma unroll
                        for (int c = 0; c < 4; c++) { const float v = q[k4][c]; if (v < mc[c]) { mc[c] = v; pc[c] = 4 * k4 + c; } }
                    m = mc[0]; pm = pc[0];
#pragma unroll
                    for (int c = 1; c < 4; c++) if (mc[c] < m || (mc[c] == m && pc[c] < pm)) { m = mc[c]; pm = pc[c]; }
                } else {
#pragma unroll
                    for (int k = 1; k < KH; k++) { const float v = q[k / 4][k % 4]; if (v < m) { m = v; pm = k; } }
                }
                pm += h * KH;
                const u32x2 mv = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
                const u32x2 pv = __builtin_amdgcn_permlane32_swap((uint32_t)pm, (uint32_t)pm, false, false);
                const float m0 = __uint_as_float(mv.x), m1 = __uint_as_float(mv.y);
                const bool lower = m0 <= m1;                            // ties: the first slot, as one lane's scan would
                thr = fmaxf(lower ? m0 : m1, thr);          // (thr never falls: it may already stand above the list's minimum, on another part's word)
                pmin = (int)(lower ? pv.x : pv.y);
            }
        }
        if (NBUF == 2 && t + 1 < t_end) store_tile(buf ^ 1);
        __syncthreads();
    }
    // ---- sort the user's list descending (ties: lower item id first)
    __syncthreads();
    if constexpr (KS > EVAL_KMAX) {
        // large K: every entry's place is the number of entries ahead of it (score, then lower id), each of the user's two
        // lanes placing half of them -- K^2 / 2 compares per lane instead of the selection sort's K^2.  Entries of one part are
        // distinct items, so the places are a permutation; the empty slots (a part with fewer than K items) keep their
        // EVAL_NEG_INF, below every inserted score, and their places are filled with -1 after the entries.
        if (have) {
            int n_full = 0;
            for (int k = 0; k < K; k++) n_full += list_i[ul][k] != ListId<IDT>::EMPTY;
            for (int k = h; k < K; k += 2) {
                const IDT raw = list_i[ul][k];
                if (raw == ListId<IDT>::EMPTY) continue;
                const float v = list_s[ul][k];
                const int id = id0 + (int)raw;
                int r = 0;
                for (int k2 = 0; k2 < K; k2++) {
                    const float v2 = list_s[ul][k2];
                    r += (v2 > v || (v2 == v && id0 + (int)list_i[ul][k2] < id)) ? 1 : 0;
                }
                if (a.part_items) {
                    const int64_t o = (slot * gridDim.y + blockIdx.y) * K + r;
                    a.part_items[o] = id; a.part_scores[o] = v;
                } else {
                    a.out_items[slot * K + r] = id;
                    if (a.out_scores) a.out_scores[slot * K + r] = v;
                }
            }
            for (int r = n_full + h; r < K; r += 2) {
                if (a.part_items) {
                    const int64_t o = (slot * gridDim.y + blockIdx.y) * K + r;
                    a.part_items[o] = -1; a.part_scores[o] = EVAL_NEG_INF * 2.0f;
                } else {
                    a.out_items[slot * K + r] = -1;
                    if (a.out_scores) a.out_scores[slot * K + r] = EVAL_NEG_INF * 2.0f;
                }
            }
        }
    } else if (h == 0 && have) {
        for (int r = 0; r < K; r++) {
            float best = EVAL_NEG_INF * 2.0f; int bi = 0x7fffffff, bk = -1;
            for (int k = 0; k < K; k++) {
                const float v = list_s[ul][k]; const IDT raw = list_i[ul][k];
                const int id = id0 + (int)raw;
                if (raw != ListId<IDT>::EMPTY && (v > best || (v == best && id < bi))) { best = v; bi = id; bk = k; }
            }
            if (bk >= 0) list_i[ul][bk] = ListId<IDT>::EMPTY;   // taken
            if (a.part_items) {
                const int64_t o = (slot * gridDim.y + blockIdx.y) * K + r;
                a.part_items[o] = bk >= 0 ? bi : -1; a.part_scores[o] = best;
            } else {
                a.out_items[slot * K + r] = bk >= 0 ? bi : -1;
                if (a.out_scores) a.out_scores[slot * K + r] = best;
            }
        }
    }
}

// top K of a user's P sorted partial lists (descending, ties: lower item id first): a P-way merge by one thread
__global__ void __launch_bounds__(256) k_eval_merge(EvalArgs a, int P) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_eval) return;
    const int K = a.K;
    int cur[4] = {0, 0, 0, 0};
    for (int r = 0; r < K; r++) {
        float best = EVAL_NEG_INF * 2.0f; int bi = 0x7fffffff, bp = -1;
        for (int p = 0; p < P; p++) {
            if (cur[p] >= K) continue;
            const int64_t o = (s * P + p) * K + cur[p];
            const int id = a.part_items[o]; const float v = a.part_scores[o];
            if (id >= 0 && (v > best || (v == best && id < bi))) { best = v; bi = id; bp = p; }
        }
        if (bp >= 0) cur[bp]++;
        a.out_items[s * K + r] = bp >= 0 ? bi : -1;
        if (a.out_scores) a.out_scores[s * K + r] = best;
    }
}

// per-user metrics from the ranked ids: r_j = [id_j in the user's test list] (sorted: binary search)
struct MetricArgs {
    const int32_t *topk; int32_t n_eval, K;
    const int64_t *test_ptr; const int32_t *test_idx;      // per evaluated slot, ids ascending
    int32_t ks[8]; int32_t n_ks;
    double *per_user;                                        // [n_eval, 3 * n_ks]: precision | recall | ndcg
};

// Running sums of hits, DCG and ideal DCG over the ranks, read out when the rank reaches a cut-off (any K: no hit mask).
__global__ void __launch_bounds__(256) k_eval_metrics_ex(MetricArgs a, int32_t kmax) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_eval) return;
    const int64_t b = a.test_ptr[s], e = a.test_ptr[s + 1];
    const int len = (int)(e - b);
    double right = 0.0, dcg = 0.0, idcg = 0.0;
    double *o = a.per_user + s * 3 * a.n_ks;
    for (int r = 0; r < kmax; r++) {
        const int32_t id = a.topk[s * a.K + r];
        const int64_t lo = csr_lower_bound(a.test_idx, b, e, id);
        const double disc = 1.0 / log2((double)(r + 2));
        if (lo < e && a.test_idx[lo] == id) { right += 1.0; dcg += disc; }
        if (r < len) idcg += disc;
        for (int q = 0; q < a.n_ks; q++) {
            if (a.ks[q] != r + 1) continue;
            const int k = a.ks[q];
            o[q] = right / (double)k;                     // utils.py:173-187
            o[a.n_ks + q] = len > 0 ? right / (double)len : 0.0;
            o[2 * a.n_ks + q] = dcg / (idcg == 0.0 ? 1.0 : idcg);      // utils.py:190-203
        }
    }
}

// sums over users in a fixed order (one workgroup: deterministic)
__global__ void __launch_bounds__(256) k_eval_sum(const double *per_user, int32_t n_eval, int32_t width, double *sums) {
    __shared__ double part[256];
    for (int c = 0; c < width; c++) {
        double acc = 0.0;
        for (int64_t s = threadIdx.x; s < n_eval; s += 256) acc += per_user[s * width + c];
        part[threadIdx.x] = acc;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) sums[c] = part[0];
        __syncthreads();
    }
}

// masks[t * stride + slot]: one wave per evaluation slot walks the user's train positives
__global__ void __launch_bounds__(256) k_eval_masks(const int32_t *users, int32_t n_eval, const int64_t *train_ptr, const int32_t *train_idx,
                                                    int32_t m_items, uint32_t *masks, int64_t stride) {
    const int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (slot >= n_eval) return;
    const int32_t u = users[slot];
    const int64_t b = train_ptr[u], e = train_ptr[u + 1];
    for (int64_t i = b + (threadIdx.x & 63); i < e; i += 64) {
        const int32_t it = train_idx[i];
        if (it >= 0 && it < m_items) atomicOr(masks + (int64_t)(it >> 5) * stride + slot, 1u << (it & 31));
    }
}

void lgcn_eval_sum_launch(const double *per_user, int32_t n_eval, int32_t width, double *sums, hipStream_t stream) {
    hipLaunchKernelGGL(k_eval_sum, dim3(1), dim3(256), 0, stream, per_user, n_eval, width, sums);
}

static inline int64_t eval_mask_stride(int32_t n_eval) { return ((int64_t)n_eval + 127) / 128 * 128; }

extern "C" int64_t lgcn_eval_mask_words(int32_t m_items, int32_t n_eval) {
    if (m_items <= 0 || n_eval <= 0) return 0;
    return (int64_t)((m_items + 31) / 32) * eval_mask_stride(n_eval);
}

extern "C" int lgcn_eval_build_masks(const int32_t *users, int32_t n_eval, const int64_t *train_indptr, const int32_t *train_indices,
                                     int32_t m_items, uint32_t *masks, void *stream) {
    if (!users || !train_indptr || !train_indices || !masks || m_items <= 0 || n_eval < 0) { lgcn_set_error("lgcn_eval_build_masks: invalid argument"); return 3; }
    if (n_eval == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t stride = eval_mask_stride(n_eval);
    if (hipMemsetAsync(masks, 0, sizeof(uint32_t) * (size_t)lgcn_eval_mask_words(m_items, n_eval), st) != hipSuccess) { lgcn_set_error("lgcn_eval_build_masks: memset failed"); return 10; }
    hipLaunchKernelGGL(k_eval_masks, dim3((unsigned)((n_eval + 3) / 4)), dim3(256), 0, st, users, n_eval, train_indptr, train_indices, m_items, masks, stride);
    if (hipGetLastError() != hipSuccess) { lgcn_set_error("lgcn_eval_build_masks: launch failed"); return 10; }
    return 0;
}

// A sweep in `parts` parts per user block, and the merge of their lists.  parts > 1: the partial lists and the block the parts
// publish their K-th best in (NaN = nothing published) are one stream-ordered allocation, or a plain one freed after a
// synchronise where the runtime has no pool; it is freed on every path.  `who` is the entry point the messages name.
template <typename Sweep>
static int sweep_in_parts(const char *who, EvalArgs &a, int parts, hipStream_t st, Sweep sweep) {
    char msg[96];
    void *tmp = nullptr;
    bool tmp_sync = false, ok = true;
    if (parts > 1) {
        const size_t n = (size_t)a.n_eval * parts * a.K;
        const size_t lists = (n * (sizeof(int32_t) + sizeof(float)) + 255) & ~(size_t)255;
        const size_t pub = EVAL_PUB_TILES > 0 ? (size_t)parts * a.n_eval * sizeof(float) : 0;
        if (hipMallocAsync(&tmp, lists + pub, st) != hipSuccess) {
            (void)hipGetLastError();
            tmp = nullptr;
            if (hipMalloc(&tmp, lists + pub) != hipSuccess) {
                snprintf(msg, sizeof msg, "%s: cannot allocate the partial lists", who); lgcn_set_error(msg); return 4;
            }
            tmp_sync = true;       // no stream-ordered pool on this runtime: plain allocation, freed after a synchronise
        }
        a.part_items = (int32_t *)tmp; a.part_scores = (float *)((int32_t *)tmp + n);
        if (pub) {
            a.thr_pub = (float *)((char *)tmp + lists);
            ok = hipMemsetAsync(a.thr_pub, 0xff, pub, st) == hipSuccess;
        }
    }
    if (ok) {
        sweep(a);
        if (parts > 1) hipLaunchKernelGGL(k_eval_merge, dim3((unsigned)((a.n_eval + 255) / 256)), dim3(256), 0, st, a, parts);
    }
    if (tmp) {
        if (tmp_sync) { (void)hipStreamSynchronize(st); (void)hipFree(tmp); }
        else (void)hipFreeAsync(tmp, st);
    }
    if (!ok) { snprintf(msg, sizeof msg, "%s: memset failed", who); lgcn_set_error(msg); return 10; }
    if (hipGetLastError() != hipSuccess) { snprintf(msg, sizeof msg, "%s: launch failed", who); lgcn_set_error(msg); return 10; }
    return 0;
}

// ---- K <= 64: 128 users per workgroup.  The compact forms (16-bit ids; the split bf16 product or the fp32 matrix instructions)
//      where the parts are short enough for them, else the generic form: int32 ids, one workgroup per CU, fp32 matrix instructions.
template <int D, int KS, typename IDT, int WGS, int NBUF, bool SPLIT3>
static void launch_small(const EvalArgs &a, int parts, bool mk, hipStream_t st) {
    const dim3 grid((unsigned)((a.n_eval + 127) / 128), (unsigned)parts);
    if (mk) hipLaunchKernelGGL((k_eval_topk<D, KS, IDT, WGS, NBUF, SPLIT3, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_eval_topk<D, KS, IDT, WGS, NBUF, SPLIT3, false>), grid, dim3(256), 0, st, a);
}

template <int D>
static void launch_small_generic(const EvalArgs &a, int parts, bool mk, hipStream_t st) {
    if (a.K <= 20) launch_small<D, 20, int32_t, 1, 2, false>(a, parts, mk, st);
    else if (a.K <= 32) launch_small<D, 32, int32_t, 1, 2, false>(a, parts, mk, st);
    else launch_small<D, 64, int32_t, 1, (D >= 256 ? 1 : 2), false>(a, parts, mk, st);     // (d = 256: 64 slots leave room for one tile)
}

template <int D>
static void launch_small_d(const EvalArgs &a, int parts, bool id16, bool split3, bool mk, hipStream_t st) {
    const bool small = a.K <= 20;
    if constexpr (D <= 64) {
        if (id16 && small && split3) { launch_small<D, 20, uint16_t, EVAL_PARTS, EVAL_NBUF, true>(a, parts, mk, st); return; }
        if (id16 && small) { launch_small<D, 20, uint16_t, EVAL_PARTS, EVAL_NBUF, false>(a, parts, mk, st); return; }
        if (id16 && split3) { launch_small<D, 64, uint16_t, 2, 2, true>(a, parts, mk, st); return; }
        if (id16) { launch_small<D, 64, uint16_t, 2, 2, false>(a, parts, mk, st); return; }
    } else if constexpr (D == 128) {        // 256 registers: two workgroups per CU, K <= 20 alone; the six planes leave LDS for one tile
        if (id16 && small && split3) { launch_small<D, 20, uint16_t, 2, 1, true>(a, parts, mk, st); return; }
        if (id16 && small) { launch_small<D, 20, uint16_t, 2, 2, false>(a, parts, mk, st); return; }
    }
    launch_small_generic<D>(a, parts, mk, st);
}

static int eval_topk(const float *E, int32_t n_users, int32_t m_items, int32_t d,
                     const int32_t *users, int32_t n_eval,
                     const int64_t *train_indptr, const int32_t *train_indices,
                     int32_t K, int32_t *topk_items, float *topk_scores, const uint32_t *masks, void *stream, bool split3) {
    if (!E || !users || !train_indptr || !train_indices || !topk_items || n_users <= 0 || m_items <= 0 || n_eval < 0) {
        lgcn_set_error("lgcn_eval_topk: invalid argument"); return 3;
    }
    if (K < 1 || K > EVAL_KMAX || K > m_items) { lgcn_set_error("lgcn_eval_topk: K must be in 1..64 and <= m_items"); return 3; }
    if (n_eval == 0) return 0;
    if (d != 32 && d != 64 && d != 128 && d != 256) { lgcn_set_error("embedding dim must be 32, 64, 128 or 256"); return 3; }
    EvalArgs a{E, n_users, m_items, users, n_eval, train_indptr, train_indices, K, topk_items, topk_scores, nullptr, nullptr, nullptr,
               masks, eval_mask_stride(n_eval)};
    hipStream_t st = (hipStream_t)stream;
    // The item sweep is split over `parts` workgroups per user block, as many as fit a CU together, so that one's list
    // maintenance runs under the others' MFMAs.  Compact lists (16-bit ids relative to the part's first item: d <= 64,
    // at most 2047 tiles per part) make that three for K <= 20 and two for K <= 64 (the lists grow with K); d = 128: two
    // for K <= 20; otherwise one workgroup per CU with int32 ids and the fp32 matrix instructions.
    // (measured on Gowalla with int32 ids, two per CU: 1 / 2 / 3 / 4 parts = 3.40 / 2.54 / 2.79 / 2.70 ms)
    const int ntiles = (m_items + 31) / 32;
    const bool small = K <= 20;
    const bool split = m_items >= 4096 && ((d <= 128 && small) || d <= 64);
    const int want = (d <= 64 && small) ? EVAL_PARTS : 2;      // d = 128: 256 registers; K > 20: 64-slot lists -- two workgroups per CU
    const bool id16 = split && (ntiles + want - 1) / want + 1 <= EVAL_ID16_MAX_TILES;
    const int parts = id16 ? want : (split && small) ? 2 : 1;
    const bool mk = masks != nullptr;
    return sweep_in_parts("lgcn_eval_topk", a, parts, st, [&](const EvalArgs &ea) {
        switch (d) {
        case 32: launch_small_d<32>(ea, parts, id16, split3, mk, st); break;
        case 64: launch_small_d<64>(ea, parts, id16, split3, mk, st); break;
        case 128: launch_small_d<128>(ea, parts, id16, split3, mk, st); break;
        default: launch_small_d<256>(ea, parts, id16, split3, mk, st); break;
        }
    });
}

extern "C" int lgcn_eval_topk(const float *E, int32_t n_users, int32_t m_items, int32_t d, const int32_t *users, int32_t n_eval,
                              const int64_t *train_indptr, const int32_t *train_indices, int32_t K, int32_t *topk_items,
                              float *topk_scores, void *stream) {
    return eval_topk(E, n_users, m_items, d, users, n_eval, train_indptr, train_indices, K, topk_items, topk_scores, nullptr, stream, EVAL_SPLIT3 != 0);
}

extern "C" int lgcn_eval_topk_masked(const float *E, int32_t n_users, int32_t m_items, int32_t d, const int32_t *users, int32_t n_eval,
                                     const int64_t *train_indptr, const int32_t *train_indices, int32_t K, int32_t *topk_items,
                                     float *topk_scores, const uint32_t *masks, void *stream) {
    return eval_topk(E, n_users, m_items, d, users, n_eval, train_indptr, train_indices, K, topk_items, topk_scores, masks, stream, EVAL_SPLIT3 != 0);
}

extern "C" int lgcn_eval_topk_fp32(const float *E, int32_t n_users, int32_t m_items, int32_t d, const int32_t *users, int32_t n_eval,
                                   const int64_t *train_indptr, const int32_t *train_indices, int32_t K, int32_t *topk_items,
                                   float *topk_scores, void *stream) {
    return eval_topk(E, n_users, m_items, d, users, n_eval, train_indptr, train_indices, K, topk_items, topk_scores, nullptr, stream, false);
}

extern "C" int lgcn_eval_metrics(const int32_t *topk_items, int32_t n_eval, int32_t K,
                                 const int64_t *test_indptr, const int32_t *test_items_sorted,
                                 const int32_t *ks, int32_t n_ks, double *per_user, double *sums, void *stream) {
    if (!topk_items || !test_indptr || !test_items_sorted || !ks || !per_user || !sums || n_eval < 0) {
        lgcn_set_error("lgcn_eval_metrics: invalid argument"); return 3;
    }
    if (n_ks < 1 || n_ks > 8 || K < 1 || K > 64) { lgcn_set_error("lgcn_eval_metrics: 1..8 cut-offs, K <= 64"); return 3; }
    MetricArgs a{};
    a.topk = topk_items; a.n_eval = n_eval; a.K = K; a.test_ptr = test_indptr; a.test_idx = test_items_sorted;
    a.n_ks = n_ks; a.per_user = per_user;
    int32_t kmax = 0;
    for (int q = 0; q < n_ks; q++) {
        if (ks[q] < 1 || ks[q] > K) { lgcn_set_error("lgcn_eval_metrics: a cut-off exceeds K"); return 3; }
        a.ks[q] = ks[q];
        kmax = ks[q] > kmax ? ks[q] : kmax;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_eval > 0) hipLaunchKernelGGL(k_eval_metrics_ex, dim3((unsigned)((n_eval + 255) / 256)), dim3(256), 0, st, a, kmax);
    lgcn_eval_sum_launch(per_user, n_eval, 3 * n_ks, sums, st);
    if (hipGetLastError() != hipSuccess) { lgcn_set_error("lgcn_eval_metrics: launch failed"); return 10; }
    return 0;
}

// ---- large K (64 < K <= 256): the same sweep with longer lists and fewer users per workgroup
//
// One workgroup per CU (the lists alone are ~96-130 KB): KS = 128 with 4 waves (128 users), KS = 256 with 2 waves (64 users),
// halved again where int32 ids and a wide fp32 tile would not fit; two tile buffers where they fit, else one.  The split bf16
// product with 16-bit ids at d <= 128; int32 ids and d = 256 take the fp32 matrix instructions.
template <int D, int KS, typename IDT, bool SPLIT3> struct BigForm {
    template <int NW> using S = EvalShape<D, KS, IDT, NW, SPLIT3>;
    static constexpr int NW = S<KS <= 128 ? 4 : 2>::lds(1) <= EVAL_LDS_BYTES ? (KS <= 128 ? 4 : 2)
                            : S<KS <= 128 ? 2 : 1>::lds(1) <= EVAL_LDS_BYTES ? (KS <= 128 ? 2 : 1) : 0;
    static_assert(NW > 0, "no large-K form fits the LDS");
    static constexpr int NBUF = S<NW>::lds(2) <= EVAL_LDS_BYTES ? 2 : 1;
};

template <int D, int KS, typename IDT, bool SPLIT3>
static void launch_big(const EvalArgs &a, int parts, bool mk, hipStream_t st) {
    using F = BigForm<D, KS, IDT, SPLIT3>;
    const dim3 grid((unsigned)((a.n_eval + 32 * F::NW - 1) / (32 * F::NW)), (unsigned)parts);
    if (mk) hipLaunchKernelGGL((k_eval_topk<D, KS, IDT, 1, F::NBUF, SPLIT3, true, F::NW>), grid, dim3(64 * F::NW), 0, st, a);
    else hipLaunchKernelGGL((k_eval_topk<D, KS, IDT, 1, F::NBUF, SPLIT3, false, F::NW>), grid, dim3(64 * F::NW), 0, st, a);
}

template <int D, int KS>
static void launch_big_d(const EvalArgs &a, int parts, bool id16, bool split3, bool mk, hipStream_t st) {
    if constexpr (D <= 128) {       // (d = 256: the six planes of both operands need more than 512 registers)
        if (id16 && split3) { launch_big<D, KS, uint16_t, true>(a, parts, mk, st); return; }
    }
    if (id16) launch_big<D, KS, uint16_t, false>(a, parts, mk, st);
    else launch_big<D, KS, int32_t, false>(a, parts, mk, st);          // int32 ids: the fp32 matrix instructions, as the generic form
}

template <int KS>
static void launch_big_k(int32_t d, const EvalArgs &a, int parts, bool id16, bool split3, bool mk, hipStream_t st) {
    switch (d) {
    case 32: launch_big_d<32, KS>(a, parts, id16, split3, mk, st); break;
    case 64: launch_big_d<64, KS>(a, parts, id16, split3, mk, st); break;
    case 128: launch_big_d<128, KS>(a, parts, id16, split3, mk, st); break;
    default: launch_big_d<256, KS>(a, parts, id16, split3, mk, st); break;
    }
}

static int eval_topk_big(const float *E, int32_t n_users, int32_t m_items, int32_t d, const int32_t *users, int32_t n_eval,
                         const int64_t *train_indptr, const int32_t *train_indices, int32_t K, int32_t *topk_items,
                         float *topk_scores, const uint32_t *masks, void *stream, bool split3) {
    if (d != 32 && d != 64 && d != 128 && d != 256) { lgcn_set_error("embedding dim must be 32, 64, 128 or 256"); return 3; }
    if (n_eval == 0) return 0;
    EvalArgs a{E, n_users, m_items, users, n_eval, train_indptr, train_indices, K, topk_items, topk_scores, nullptr, nullptr, nullptr,
               masks, eval_mask_stride(n_eval)};
    hipStream_t st = (hipStream_t)stream;
    // One workgroup per CU whatever the split, so the parts trade spreading the user blocks over the 256 CUs (whole rounds of
    // workgroups: ceil(blocks * parts / 256)) against list work that each part repeats (~K (1 + ln(items per part / K)) insertions
    // per user and part).  The part count minimises rounds x (tiles per part + 0.53 K (1 + ln(items per part / K))), the weight
    // fitted to the measured 1 / 2 / 4-part sweeps (Gowalla: 1 part; 300 000 items x 20 000 users: 3 parts at K = 100, 2 at
    // K = 256).  At most 4 parts (k_eval_merge); a part covers >= 1024 items (catalogues of >= 4096), so it always holds K of them.
    // 16-bit ids (and the split bf16 product) when a part spans at most 2047 tiles; else int32 ids.
    const int ntiles = (m_items + 31) / 32;
    const int64_t nu0 = K <= 128 ? 128 : 64;
    const int64_t blocks0 = (n_eval + nu0 - 1) / nu0;
    int parts = 1;
    if (m_items >= 4096) {
        if (EVAL_BIG_PARTS > 0) parts = EVAL_BIG_PARTS;
        else {
            double best = 0.0;
            for (int p = 1; p <= 4; p++) {
                const double rounds = (double)((blocks0 * p + 255) / 256);
                const double cost = rounds * ((double)ntiles / p + 0.53 * K * (1.0 + log((double)m_items / p / K)));
                if (p == 1 || cost < best) { best = cost; parts = p; }
            }
        }
    }
    const bool id16 = (ntiles + parts - 1) / parts + 1 <= EVAL_ID16_MAX_TILES;
    const bool mk = masks != nullptr;
    return sweep_in_parts("lgcn_eval_topk_ex", a, parts, st, [&](const EvalArgs &ea) {
        if (K <= 128) launch_big_k<128>(d, ea, parts, id16, split3, mk, st);
        else launch_big_k<256>(d, ea, parts, id16, split3, mk, st);
    });
}

extern "C" int32_t lgcn_eval_kmax(void) { return EVAL_KMAX_EX; }

extern "C" int lgcn_eval_topk_ex(const float *E, int32_t n_users, int32_t m_items, int32_t d, const int32_t *users, int32_t n_eval,
                                 const int64_t *train_indptr, const int32_t *train_indices, const uint32_t *masks,
                                 int32_t K, int32_t *topk_items, float *topk_scores, int64_t out_capacity,
                                 int32_t flags, void *stream) {
    if (!E || !users || !train_indptr || !train_indices || !topk_items || n_users <= 0 || m_items <= 0 || n_eval < 0 || (flags & ~LGCN_EVAL_FP32)) {
        lgcn_set_error("lgcn_eval_topk_ex: invalid argument"); return 3;
    }
    if (K < 1 || K > EVAL_KMAX_EX || K > m_items) { lgcn_set_error("lgcn_eval_topk_ex: K must be in 1..lgcn_eval_kmax() and <= m_items"); return 3; }
    if (out_capacity < 0 || (int64_t)n_eval * K > out_capacity) { lgcn_set_error("lgcn_eval_topk_ex: output buffers hold fewer than n_eval * K elements"); return 3; }
    const bool split3 = EVAL_SPLIT3 != 0 && !(flags & LGCN_EVAL_FP32);
    if (K <= EVAL_KMAX)        // the K <= 64 sweep itself: bitwise lgcn_eval_topk_masked / lgcn_eval_topk_fp32
        return eval_topk(E, n_users, m_items, d, users, n_eval, train_indptr, train_indices, K, topk_items, topk_scores, masks, stream, split3);
    return eval_topk_big(E, n_users, m_items, d, users, n_eval, train_indptr, train_indices, K, topk_items, topk_scores, masks, stream, split3);
}

extern "C" int lgcn_eval_metrics_ex(const int32_t *topk_items, int32_t n_eval, int32_t K,
                                    const int64_t *test_indptr, const int32_t *test_items_sorted,
                                    const int32_t *ks, int32_t n_ks, double *per_user, double *sums, void *stream) {
    if (!topk_items || !test_indptr || !test_items_sorted || !ks || !per_user || !sums || n_eval < 0) {
        lgcn_set_error("lgcn_eval_metrics_ex: invalid argument"); return 3;
    }
    if (n_ks < 1 || n_ks > 8 || K < 1 || K > EVAL_KMAX_EX) { lgcn_set_error("lgcn_eval_metrics_ex: 1..8 cut-offs, K <= lgcn_eval_kmax()"); return 3; }
    MetricArgs a{};
    a.topk = topk_items; a.n_eval = n_eval; a.K = K; a.test_ptr = test_indptr; a.test_idx = test_items_sorted;
    a.n_ks = n_ks; a.per_user = per_user;
    int32_t kmax = 0;
    for (int q = 0; q < n_ks; q++) {
        if (ks[q] < 1 || ks[q] > K) { lgcn_set_error("lgcn_eval_metrics_ex: a cut-off exceeds K"); return 3; }
        a.ks[q] = ks[q];
        kmax = ks[q] > kmax ? ks[q] : kmax;
    }
    hipStream_t st = (hipStream_t)stream;
    if (n_eval > 0) hipLaunchKernelGGL(k_eval_metrics_ex, dim3((unsigned)((n_eval + 255) / 256)), dim3(256), 0, st, a, kmax);
    lgcn_eval_sum_launch(per_user, n_eval, 3 * n_ks, sums, st);
    if (hipGetLastError() != hipSuccess) { lgcn_set_error("lgcn_eval_metrics_ex: launch failed"); return 10; }
    return 0;
}

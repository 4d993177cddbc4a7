/*
 * lgcn_hip.h -- C ABI of the MI355X-native LightGCN/BPR training hot path.
 *
 * One shared library (liblgcn_hip.so, built from
 * graph-and-sequential-recommendation-systems_amd/csrc by hipcc for gfx950).
 * Plain C types only: device buffers are raw pointers (e.g. torch
 * `tensor.data_ptr()`), streams are `hipStream_t` passed as void*.  Every
 * device entry point is asynchronous on the given stream, never allocates,
 * never synchronises, and is therefore hipGraph-capturable.  Return value:
 * 0 = ok, non-zero = error (text via lgcn_last_error()).
 *
 * Each entry point names the reference interface it replaces; paths are
 * relative to LightGCN_work/code in saamiya225/Graph-and-sequential-recommendation-systems.
 * The reference's only FFI on this path is the pybind11 module `sampling`
 * (sources/sampling.cpp:95-106); everything else replaces PyTorch library
 * calls made from model.py / utils.py.  INTEGRATION.md shows the bindings.
 */
#ifndef LGCN_HIP_H
#define LGCN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LGCN_ABI_VERSION 13
#define LGCN_MAX_LAYERS 8

/* storage type of propagated activations (accumulation is always fp32) */
enum { LGCN_F32 = 0, LGCN_BF16 = 1, LGCN_FP8 = 2 };
/* LGCN_FP8: a table of n rows is n*d bytes of OCP E4M3 values FOLLOWED BY n fp32 row scales (value = scale * fp8), one pointer
 * for both; scales are powers of two with max|row| / scale in [64, 128).  d must be 64, 128 or 256.  The bytes of a row are
 * CHUNK-INTERLEAVED (an opaque layout: lgcn_to_fp8 writes it, the kernels read it): with L = d/16, byte l*16 + 4j + e holds
 * column (j*L + l)*4 + e, so that a lane gathering 16 bytes owns four float4 chunks L chunks apart and the fp32 side of every
 * epilogue is coalesced.  Accumulation is fp32 as
 * with every storage type.  lgcn_table_bytes: bytes of one [n_rows, d] table of a storage type (fp8: rows + scales, padded
 * to 256); lgcn_to_fp8: quantise an fp32 table (device pointers).                                                     */
int64_t lgcn_table_bytes(int64_t n_rows, int32_t d, int32_t dtype);
int lgcn_to_fp8(const float *src, void *dst, int64_t n_rows, int32_t d, void *stream);

int lgcn_abi_version(void);
const char *lgcn_last_error(void);
/* 1 if a HIP device is usable from this process, else 0 (never throws) */
int lgcn_device_available(void);

/* ------------------------------------------------------------------------ */
/* Host: BPR triplet sampler -- replaces the pybind11 module `sampling`      */
/* ------------------------------------------------------------------------ */
/* sampling.seed(seed)            sources/sampling.cpp:88-91,101  (srand)     */
void lgcn_sampling_seed(unsigned int seed);
/* sampling.randint(end)          sources/sampling.cpp:22-25,100  (rand()%end) */
int lgcn_sampling_randint(int end);
/* sampling.sample_negative(user_num,item_num,train_num,allPos,neg_num)
 *                                sources/sampling.cpp:27-56,102-103
 * allPos is passed zero-copy as the CSR (indptr[user_num+1], indices) of
 * UserItemNet (dataloader.py:133-136,178-180; columns sorted ascending).
 * S_out: int32 [user_num*(train_num/user_num), 2+neg_num], row-major.
 * Bit-exact glibc rand() stream.  Returns 2 (no crash) if a user has no
 * positives, where the reference dies with SIGFPE on rand()%0. */
int lgcn_sample_negative(int user_num, int item_num, int64_t train_num,
                         const int64_t *indptr, const int32_t *indices,
                         int neg_num, int32_t *S_out);
/* sampling.sample_negative_ByUser(users,item_num,allPos,neg_num)
 *                                sources/sampling.cpp:58-86,104-105          */
int lgcn_sample_negative_by_user(const int32_t *users, int n_users_listed, int item_num,
                                 const int64_t *indptr, const int32_t *indices,
                                 int neg_num, int32_t *S_out);

/* The same sampler on the GPU (neg_num = 1): identical rows from the identical rand() stream, written
 * to DEVICE memory (d_S int32 [user_num*(train_num/user_num), 3]); the host generator is then moved
 * past the draws the device consumed (jump-ahead), so host and device calls can be mixed freely.
 * h_indptr: host copy of the CSR row pointers (degree checks); d_indptr/d_indices: device CSR;
 * workspace: device bytes from lgcn_sample_negative_device_workspace().  Synchronises `stream`. */
int64_t lgcn_sample_negative_device_workspace(int user_num, int64_t train_num);
int lgcn_sample_negative_device(int user_num, int item_num, int64_t train_num,
                                const int64_t *h_indptr, const int64_t *d_indptr, const int32_t *d_indices,
                                int32_t *d_S, void *workspace, int64_t workspace_bytes, void *stream);
/* TEST HOOK: the device sampler expands 2 draws per triplet + T / divisor + fixed more (default 50, 65536) and
 * returns 5 -- host generator untouched -- when an epoch's rejections need more.  A test makes the margin small to
 * drive the segmented path into the end of the stream; values <= 0 restore the defaults.  Affects the workspace size. */
void lgcn_sampler_test_margin(int64_t divisor, int64_t fixed);
/* The device sampler for neg_num = R negatives per positive, 1 <= R <= LGCN_MAX_NEG_RATIO: the rows of
 * lgcn_sample_negative(..., neg_num, S) as d_S int32 [user_num*(train_num/user_num), 2+neg_num] in DEVICE memory, from the
 * same rand() stream, the host generator left where the host loop leaves it.  Arguments as lgcn_sample_negative_device;
 * the workspace query takes neg_num (monotone in it; at 1 it is the three-slot query).  The stream margin is
 * neg_num * (T / divisor) + fixed draws beyond the 1 + neg_num per sample (lgcn_sampler_test_margin sets both calls').
 * Returns 3 (nothing touched) for an invalid argument, a short workspace or neg_num outside 1..16, 2 (nothing written) for
 * a user without positives or positive on every item, 5 (generator not advanced) when the margin is exceeded, 10 for a
 * failed launch or copy.  Synchronises `stream`. */
int64_t lgcn_sample_negative_device_multi_workspace(int user_num, int64_t train_num, int neg_num);
int lgcn_sample_negative_device_multi(int user_num, int item_num, int64_t train_num,
                                      const int64_t *h_indptr, const int64_t *d_indptr, const int32_t *d_indices,
                                      int neg_num, int32_t *d_S, void *workspace, int64_t workspace_bytes, void *stream);

/* numpy legacy global RandomState stream (MT19937), used by the reference for
 * the fallback sampler and the epoch shuffle.                                 */
/* utils.set_seed -> np.random.seed(seed)                    utils.py:114-120 */
void lgcn_np_seed(uint32_t seed);
/* The generator's whole state, as numpy's RandomState.get_state() / set_state() name it: key[624] (the untempered MT19937
 * words) and the read position pos in 0..624 (624: the next draw twists first; larger values are taken as 624).          */
void lgcn_np_get_state(uint32_t key[624], uint32_t *pos);
void lgcn_np_set_state(const uint32_t key[624], uint32_t pos);
/* utils.UniformSample_original_python                      utils.py:84-110
 * S_out: int64 [train_num,3]; returns the number of rows written (users with no
 * positives are skipped), or -1 on error.                                      */
int64_t lgcn_sample_python(int n_users, int m_items, int64_t train_num,
                           const int64_t *indptr, const int32_t *indices, int64_t *S_out);
/* utils.shuffle: idx = arange(n); np.random.shuffle(idx)    utils.py:148-149 */
int lgcn_np_shuffle_perm(int64_t n, int64_t *perm_out);

/* ------------------------------------------------------------------------ */
/* Host: graph builder -- replaces Loader.getSparseGraph dataloader.py:218-234 */
/* ------------------------------------------------------------------------ */
/* COO interactions (dataloader.py:133-136) -> UserItemNet CSR with sorted,
 * de-duplicated columns (values = multiplicity).  Call with indices==NULL to get
 * the de-duplicated nnz in *nnz_out first.                                     */
int lgcn_build_user_item_csr(int n_users, int m_items, int64_t n_inter,
                             const int64_t *train_user, const int64_t *train_item,
                             int64_t *indptr, int32_t *indices, float *vals, int64_t *nnz_out);
/* fp32 row sums of A=[[0,R],[R^T,0]]                        dataloader.py:230 */
int lgcn_adj_rowsum(int n_users, int m_items, const int64_t *r_indptr, const int32_t *r_indices,
                    const float *r_vals, float *rowsum);
/* A_hat = D^-1/2 A D^-1/2 as CSR (int32 indptr[N+1], indices[2E], fp32 data[2E]),
 * value = fl32(fl32(d_inv[i]*a_ij)*d_inv[j]); d_inv is supplied by the caller
 * (the host mirror computes it with numpy.power exactly as dataloader.py:231). */
int lgcn_build_norm_adj(int n_users, int m_items, const int64_t *r_indptr, const int32_t *r_indices,
                        const float *r_vals, const float *d_inv,
                        int32_t *indptr, int32_t *indices, float *data);

/* ------------------------------------------------------------------------ */
/* Device: graph object + single kernels                                      */
/* ------------------------------------------------------------------------ */
/* The device-resident A_hat (what Loader.getSparseGraph returns, dataloader.py:203-246,
 * here as CSR: int32 indptr[n_rows+1], int32 indices[nnz] sorted per row, fp32 vals[nnz]).
 * The arrays are borrowed (must outlive the graph).  Creation is synchronous: it reads
 * indptr back once to plan the splitting of long rows and allocates that plan's scratch
 * (d_max = largest embedding dim that will be used with this graph).  Column indices are
 * range-checked here (rc 3), so no later launch can gather out of bounds.  Launches on one
 * graph share its scratch: the library orders them (a launch on another stream than the
 * previous one first waits for it).
 * row_order (DEVICE int32[n_order], may be NULL = natural order of all rows) is an optional
 * PROCESSING order of the rows -- a permutation chosen for L2 locality (n_order = n_rows), or
 * a SUBSET of the rows without repetition (n_order < n_rows: launches then compute only those
 * rows and leave the others of Y untouched -- a rank's share of a row-sharded job);
 * xcd_start (HOST int64[9], may be NULL) cuts that order into the 8 slices the 8 XCDs work on
 * (NULL: 8 slices of equal work).  Neither changes the memory layout or any result bit.   */
typedef struct lgcn_graph lgcn_graph;   /* opaque */
int lgcn_graph_create(const int32_t *indptr, const int32_t *indices, const float *vals,
                      int64_t n_rows, int64_t nnz, int32_t d_max, const int32_t *row_order,
                      int64_t n_order, const int64_t *xcd_start, lgcn_graph **out);
void lgcn_graph_destroy(lgcn_graph *g);

/* Y = A_hat X  -- replaces torch.sparse.mm(g, x)                model.py:217
 * (and its autograd backward A^T g: A_hat is symmetric).  X,Y: [n_rows,d]
 * row-major, fp32 or bf16 (x_dtype / y_dtype); d in {32,64,128,256}.           */
int lgcn_spmm_csr(const lgcn_graph *g, const void *X, int x_dtype, void *Y, int y_dtype, int d,
                  void *stream);

/* Edge dropout (upstream LightGCN's __dropout_x, which the fork left as a TODO in computer()).  For one optimiser step
 * `step` and a 64-bit seed every stored non-zero (i, j) of A_hat is kept when
 *     H(seed, step, i, j) < floor(keep_prob * 2^32)
 * and the survivors are scaled by 1 / keep_prob (fp32).  H is a 32-bit counter-based hash of the seed, the step and the row
 * and column ids of the [N, N] adjacency only (DESIGN 4 spells it out): not of CSR positions, plans or kernels.  keep(i, j)
 * and keep(j, i) are independent draws; for fixed (seed, step) the kept set grows with keep_prob.  keep_prob in (0, 1].
 *
 * lgcn_dropout_mask: keep_out[p] (device uint8[nnz]) = keep(row of p, indices[p]) for CSR position p.  Device pointers.   */
int lgcn_dropout_mask(const int32_t *indptr, const int32_t *indices, int64_t n_rows, int64_t nnz,
                      float keep_prob, uint64_t seed, int64_t step, uint8_t *keep_out, void *stream);
/* Y = A_drop X (transposed = 0) or, at row i, the sum over the stored (i, j) of keep(j, i) * v / keep_prob * X[j]
 * (transposed = 1: A_drop^T X with A_hat's own values, as every backward here uses them): lgcn_spmm_csr with the step's
 * mask; fp32 / bf16 tables, the same dims.  keep_prob = 1 is lgcn_spmm_csr itself.                                       */
int lgcn_spmm_csr_drop(const lgcn_graph *g, const void *X, int x_dtype, void *Y, int y_dtype, int d,
                       float keep_prob, uint64_t seed, int64_t step, int transposed, void *stream);

/* out[N,d] fp32 = mean(X_0, A X_0, ..., A^K X_0) -- replaces LightGCN.computer()
 * model.py:201-231 (cat + K sparse.mm + stack + mean).  work: (K-1)*N*d elements
 * of act_dtype (may be NULL for K == 1).                                       */
int lgcn_propagate_mean(const lgcn_graph *g, const float *E0, int K, int d, int act_dtype,
                        void *work, float *out, void *stream);
/* The same with layer weights: out = sum_k w_host[k] * A^k X_0 for the K + 1 fp32 values w_host[0..K] (host memory), used
 * as they are (no normalisation).  LGCN_F32 / LGCN_BF16 storage.  rc 3: a non-finite weight, all weights zero, LGCN_FP8.     */
int lgcn_propagate_weighted(const lgcn_graph *g, const float *E0, int K, int d, int act_dtype,
                            void *work, const float *w_host, float *out, void *stream);

/* The same permutation from the same stream, produced ON THE DEVICE (d_perm: device int64[n]): one wave twists MT19937 in LDS
 * and aligns the draws to the Fisher-Yates steps as it generates them (64 per pass), then the swaps are resolved as sorted chains +
 * pointer doubling (csrc/lgcn_shuffle.hip).  The host generator is set to where the device stopped, so host and device calls mix
 * freely.  workspace: device bytes from lgcn_np_shuffle_perm_device_workspace(n).  Returns 3 for n >= 2^31 - 16 (the caller then
 * uses lgcn_np_shuffle_perm).  Synchronises `stream`. */
int64_t lgcn_np_shuffle_perm_device_workspace(int64_t n);
int lgcn_np_shuffle_perm_device(int64_t n, int64_t *d_perm, void *workspace, int64_t workspace_bytes, void *stream);
/* TEST HOOK: the swap resolution of lgcn_np_shuffle_perm_device alone (keys, sort, parents, pointer doubling, output -- the same
 * launches, the same workspace layout and size) on targets the caller chooses: d_perm (device int64[n]) = the result of
 * x = arange(n); for i = n-1 .. 1: swap(x[i], x[J[i]]).  J_host: HOST uint32[n] with J[0] == 0 and J[i] <= i, checked before
 * anything is launched (rc 3 otherwise, as for a short workspace or n >= 2^31 - 16).  Draws from MT19937 give chains about
 * log n deep; a test reaches deep chains and long runs of equal targets only through here.  The host generator is neither
 * read nor written.  Synchronises `stream`. */
int lgcn_fy_resolve_device(const uint32_t *J_host, int64_t n, int64_t *d_perm, void *workspace, int64_t workspace_bytes, void *stream);
/* users/pos/neg[T] = S[perm[t], 0..2] -- the device side of utils.shuffle
 * (utils.py:150) applied to the sampler output (main.py:217-220).            */
int lgcn_apply_perm(const int32_t *S, int s_cols, const int64_t *perm, int64_t T,
                    int32_t *users, int32_t *pos, int32_t *neg, void *stream);

/* The same for rows of 2 + R ids (the sampler's output with neg_num = R): users/pos[T] = S[perm[t], 0..1], and negative
 * column r of the result, negs + r * T, holds S[perm[t], 2 + r] -- the [R][T] layout lgcn_train_epoch_multi reads.
 * 1 <= R <= LGCN_MAX_NEG_RATIO, s_cols >= 2 + R.  For R = 1 it writes what lgcn_apply_perm writes.                 */
int lgcn_apply_perm_multi(const int32_t *S, int s_cols, const int64_t *perm, int64_t T,
                          int32_t *users, int32_t *pos, int32_t *negs /* [R][T] */, int32_t R, void *stream);

/* ------------------------------------------------------------------------ */
/* Device: fused training step -- replaces BPRLoss.stageOne   utils.py:53-64  */
/*   = LightGCN.bpr_loss (model.py:162-183) + loss.backward() (autograd of     */
/*     model.py:201-231) + torch.optim.Adam.step (utils.py:51,62)              */
/* ------------------------------------------------------------------------ */
typedef struct lgcn_ctx lgcn_ctx;   /* opaque */

typedef struct {
    const lgcn_graph *graph;    /* A_hat, N = n_users + m_items rows */
    int32_t n_users;
    int32_t d;                  /* latent_dim_rec: 32/64/128/256 */
    int32_t K;                  /* lightGCN_n_layers: 1..LGCN_MAX_LAYERS */
    int32_t act_dtype;          /* LGCN_F32 | LGCN_BF16 | LGCN_FP8: storage of layer activations (forward X_k and backward h_k) */
    /* parameters + Adam state, fp32 [N,d]: rows [0,n_users) = embedding_user.weight,
     * rows [n_users,N) = embedding_item.weight (model.py:57-60) */
    float *E0;
    float *adam_m;
    float *adam_v;
    /* workspace, caller-allocated, zero-initialised before the first step */
    void *act;                  /* max(1, dense_last ? K : K-1) tables of lgcn_table_bytes(N, d, act_dtype) bytes each */
    int64_t *G64;               /* [N,d] fixed-point (2^50) accumulator of the sparse-row gradient */
    uint32_t *bitmap;           /* [2*ceil(N/32)] rows of G64 that are non-zero (two, used alternately) */
    float *terms;               /* [2*max_batch] per-triplet loss / reg terms */
    float *contrib;             /* [3*max_batch*d + 2*max_batch] (data-parallel exchange buffer) or NULL */
    int32_t *err;               /* [1] device error flag */
    int32_t max_batch;
    /* hyper-parameters (utils.py:47-51, torch.optim.Adam defaults) */
    float decay;                /* config['decay'] */
    double lr, beta1, beta2, eps;
    int32_t xcd_remap;          /* 1: contiguous row ranges per XCD */
    int32_t dense_last;         /* 1: propagate the LAST layer densely too and read the batch rows from it (needs K
                                   activation buffers); 0: compute it only on the 3B batch rows (K-1 buffers).  Pays
                                   when the batch rows together hold more non-zeros than the graph (hub-heavy data) */
    /* hub plan of the batch-row kernel (dense_last = 0): rows with more than hub_nnz non-zeros get their last-layer row
     * from a whole-chip SpMM over just those rows, once per step, instead of from the one workgroup of each triplet
     * that names them.  0 = library default (131072), < 0 = no hub plan.  hub_chunk: non-zeros per chunk of those
     * rows (0 = default 2048).  Neither changes the algorithm, only who sums a hub row (fp32 summation order). */
    int32_t hub_nnz;
    int32_t hub_chunk;
    /* ---- the fork's optional branches (all NULL / 0: the default model).  With either one on, the step propagates every
     * layer densely (dense_last must be 1), forms the layer mean T, and runs the loss on ONE final table.
     * Item-item smoothing, model.py:99-109,228-229: items = T_items + alpha * (I2I @ T_items).  i2i / i2i_t: graphs over the
     * m_items item rows ([m_items, m_items]) holding alpha * I2I and its transpose (the caller scales the values).      */
    const lgcn_graph *i2i;
    const lgcn_graph *i2i_t;
    /* Popularity gate, model.py:66-96,139-157,176-181.  gate_params: ONE fp32 buffer holding the eight tensors of pop_mlp
     * and gate_mlp back to back in torch's named_parameters order and torch.nn.Linear layouts:
     *   pop_mlp.0.weight [Hp,1] | pop_mlp.0.bias [Hp] | pop_mlp.2.weight [d,Hp] | pop_mlp.2.bias [d] |
     *   gate_mlp.0.weight [Hg,2d] | gate_mlp.0.bias [Hg] | gate_mlp.2.weight [1,Hg] | gate_mlp.2.bias [1]
     * (P = 2 Hp + d Hp + d + 2 d Hg + 2 Hg + 1 floats); gate_adam_m / gate_adam_v / gate_grad: [P] each (Adam state of those
     * parameters, zero-initialised; the last reduced gradient, for inspection).  Hp, Hg <= 64, d <= 128.
     * terms must then hold 3 * max_batch floats (third block: the gates' entropy per triplet).                         */
    const float *item_pop;      /* [m_items] item_pop_scalar, or NULL: no gate */
    float *gate_params;
    float *gate_adam_m;
    float *gate_adam_v;
    float *gate_grad;
    int32_t pop_hidden;         /* Hp */
    int32_t gate_hidden;        /* Hg */
    float gate_entropy_coeff;
    float pop_gate_temp;
    /* Which rows the L2 term of the loss is taken on.  0 (default) = the reference: the PROPAGATED rows of the batch
     * (model.py:173: u.norm(2), pos_e.norm(2), neg_e.norm(2) of getEmbedding's outputs).  1 = UPSTREAM LightGCN, the code the
     * reference forked and whose recorded 1000-epoch run / README table it keeps (code/runs/07-10-17h52m32s--lgn,
     * LightGCN_work/README.md:88-95): the embedding tables' OWN rows of the batch (userEmb0 / posEmb0 / negEmb0), whose
     * gradient decay/B * count(row) * E0[row] does not pass through the propagation -- the Adam epilogue adds it from a
     * per-row slot count.  Not available together with the optional branches.                                        */
    int32_t reg_ego;
} lgcn_train_config;

/* Besides the caller's workspace the context owns device allocations made here with hipMalloc and released by
 * lgcn_ctx_destroy: N*d*4 bytes (fp32 copy of the step's sparse gradient rows) and, with act_dtype = LGCN_BF16 and
 * K >= 2, N*d*2 bytes (bf16 copy of E0: the input of layer 1 in that mode).  Returns 4 if they cannot be had. */
int lgcn_ctx_create(const lgcn_train_config *cfg, lgcn_ctx **out);
void lgcn_ctx_destroy(lgcn_ctx *ctx);
/* optimizer step counter (torch Adam state['step']) for checkpoint/resume */
int64_t lgcn_ctx_get_step(const lgcn_ctx *ctx);
/* number of rows in the context's hub plan (0: none was built) */
int64_t lgcn_ctx_hub_rows(const lgcn_ctx *ctx);
void lgcn_ctx_set_step(lgcn_ctx *ctx, int64_t step);
void lgcn_ctx_set_lr(lgcn_ctx *ctx, double lr);
/* Edge dropout in the training step (--dropout 1 --keepprob p): lgcn_train_step / _i64 / lgcn_train_epoch then draw ONE mask
 * per step from (seed, lgcn_ctx_get_step() before the step) and use A_drop in all K forward layers, on the batch rows and
 * (transposed) in the whole backward; the layer mean still includes X_0.  A step is bitwise reproducible for a given
 * (seed, step), and a resumed run replays the same masks.  Evaluation entry points never drop.  keep_prob in (0, 1];
 * 1.0 = off (the step then launches exactly the kernels it launches without this call).  rc 3: out of range, or the context
 * uses LGCN_FP8 storage or an optional branch (i2i / popularity gate).  While dropout is on, every entry point that splits
 * a step over ranks (lgcn_train_step_dp_* / _cols_*, lgcn_rs_phase, lgcn_train_epoch_dp) returns 3 and says so.          */
int lgcn_ctx_set_dropout(lgcn_ctx *ctx, float keep_prob, uint64_t seed);
/* Layer weights in the training step (--layer_weights): the model's output becomes  out = sum_k w_k X_k  (X_0 = E0,
 * X_k = A_hat X_{k-1}) instead of the mean, for the n = K + 1 fp32 values w_host[0..K] (host memory), used exactly as given.
 * lgcn_train_step / _i64 / lgcn_train_epoch then form the weighted rows of the batch and run the backward chain
 *     h_K = w_K G,   h_{k-1} = w_{k-1} G + A_hat h_k,   gradient = h_0        (G = d loss / d out)
 * with the same launches as the mean (the weights travel as kernel arguments).  reg_ego is untouched by the weights; the
 * default L2 term is taken on the weighted rows.  w_host == NULL or n == 0 restores the mean: the step then launches exactly
 * the kernels it launches without this call, with the same arguments.  rc 3 (the error text names the layer weights):
 * n != K + 1, a non-finite value, all zeros, LGCN_FP8 storage, an optional branch (i2i / popularity gate), dropout on.
 * While weights are set lgcn_ctx_set_dropout refuses, and every entry point that splits a step over ranks
 * (lgcn_train_step_dp_* / _cols_*, lgcn_rs_phase, lgcn_train_epoch_dp) returns 3 and says so.                             */
int lgcn_ctx_set_layer_weights(lgcn_ctx *ctx, const float *w_host, int32_t n);
/* The weights in force: writes them to w_out (room for LGCN_MAX_LAYERS + 1 floats; may be NULL) and returns their count;
 * 0 = the mean.                                                                                                          */
int32_t lgcn_ctx_get_layer_weights(const lgcn_ctx *ctx, float *w_out);
/* Data parallel, rows mode: 1 = part 1 of a step also adds this rank's OWN gradient rows into its G64 (besides writing
 * them to the exchange block) and part 2 scatters only the other ranks' blocks -- what lgcn_train_epoch_dp does itself;
 * 0 (default) = part 2 scatters every block (one context may then play several ranks, as the emulation tests do). */
int lgcn_ctx_set_dp_local(lgcn_ctx *ctx, int on);

/* One full stageOne on a batch of B triplets (device int32 ids).
 * loss_out[0..2] (device) = {bpr + decay*reg, bpr, reg}.  No host sync.        */
int lgcn_train_step(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, const int32_t *neg,
                    int32_t B, float *loss_out, void *stream);

/* The same step for ids as the reference passes them -- torch.long (int64) device tensors (main.py:217-225): one launch narrows the
 * three arrays into ids_scratch (device int32 [3*B], caller-owned) and the step follows on the same stream; an id outside int32
 * is flagged like any out-of-range id.                                                                                       */
int lgcn_train_step_i64(lgcn_ctx *ctx, const int64_t *users, const int64_t *pos, const int64_t *neg,
                        int32_t B, int32_t *ids_scratch, float *loss_out, void *stream);

/* A whole epoch: the loop of main.py:223-225 over ceil(T/B) consecutive batches
 * of the (already shuffled) device arrays.  loss_out: [3*ceil(T/B)].           */
int lgcn_train_epoch(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, const int32_t *neg,
                     int64_t T, int32_t B, float *loss_out, void *stream);

/* Several negatives per positive (--neg_ratio R).  A batch is B samples (u_b, p_b, n_{b,1..R}); negative column r
 * of the batch is negs + r * neg_stride (device int32, neg_stride >= B).  With e the rows of the model's output table:
 *   x_{b,r} = e_u.e_p - e_u.e_{n_r}
 *   bpr = -1/(B R) sum_b sum_r logsigmoid(x_{b,r})
 *   reg = 0.5/B sum_b ( |e_u|^2 + |e_p|^2 + 1/R sum_r |e_{n_r}|^2 )      (reg_ego: the same on the tables' own rows)
 *   loss_out = {bpr + decay * reg, bpr, reg}
 * -- term for term the loss of lgcn_train_step on the flattened batch of B R triplets (u_b, p_b, n_{b,r}), but the batch-row
 * launch reads 2 + R slot rows per sample and adds 2 + R gradient rows instead of 3 R.  Forward, backward chain and the Adam
 * epilogue are those of lgcn_train_step; edge dropout and layer weights set on the context apply.  B <= max_batch.
 * rc 3, with a message that names the negative ratio and with outputs, step counter and workspace untouched: R outside
 * 1..LGCN_MAX_NEG_RATIO, neg_stride < B, a context with dense_last = 0, LGCN_FP8 storage, or an optional branch (i2i /
 * popularity gate).  The data-parallel entry points stay three-slot.                                                          */
#define LGCN_MAX_NEG_RATIO 16
int lgcn_train_step_multi(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos,
                          const int32_t *negs, int64_t neg_stride, int32_t R,
                          int32_t B, float *loss_out, void *stream);
/* A whole epoch of such steps: ceil(T/B) consecutive batches of the (already shuffled) arrays, negative column r of the
 * epoch at negs + r * T (what lgcn_apply_perm_multi writes).  loss_out: [3*ceil(T/B)].  The same refusals.                  */
int lgcn_train_epoch_multi(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos,
                           const int32_t *negs /* [R][T]: column r at negs + r*T */, int32_t R,
                           int64_t T, int32_t B, float *loss_out, void *stream);
/* The loss of the multi-negative step (--loss).  LGCN_LOSS_BPR (the default) is the definition above.  With
 * LGCN_LOSS_SOFTMAX the positive competes against all R negatives of its sample inside one log-sum-exp at temperature tau:
 *   z_{b,r} = -x_{b,r} / tau,   l_b = log(1 + sum_r exp(z_{b,r})),   sm = 1/B sum_b l_b        (one term per sample: 1/B, not 1/(B R))
 *   loss_out = {sm + decay * reg, sm, reg}      (reg as above)
 *   gb_r = -q_{b,r} / (tau B),  q_{b,r} = exp(z_{b,r}) / (1 + sum_j exp(z_{b,j}))      (evaluated with the maximum subtracted: no
 *                                                                                       exp of a positive argument, any finite score)
 * lgcn_train_step_multi / lgcn_train_epoch_multi then run the softmax form of the batch-row launch (k_multineg) for every R in
 * 1..LGCN_MAX_NEG_RATIO; forward, backward chain, Adam epilogue, edge dropout, layer weights and reg_ego are untouched.  At
 * R = 1, tau = 1 it is the BPR step.  lgcn_ctx_set_loss(ctx, LGCN_LOSS_BPR, anything) restores exactly the launches of a
 * context that was never told otherwise.  rc 3, with a message that names the loss and nothing changed: an unknown kind, tau
 * not finite or <= 0, LGCN_FP8 storage, an optional branch (i2i / popularity gate), dense_last = 0.  While the softmax loss is
 * set every three-slot and every rank-splitting entry point (lgcn_train_step / _i64, lgcn_train_epoch, lgcn_train_step_dp_* /
 * _cols_*, lgcn_rs_phase, lgcn_train_epoch_dp) returns 3 and says so: their kernels compute BPR.                              */
#define LGCN_LOSS_BPR 0
#define LGCN_LOSS_SOFTMAX 1
int lgcn_ctx_set_loss(lgcn_ctx *ctx, int32_t kind, float temperature);
/* The loss in force (-1: null context); its temperature goes to temperature_out (may be NULL; 1 under LGCN_LOSS_BPR).       */
int32_t lgcn_ctx_get_loss(const lgcn_ctx *ctx, float *temperature_out);

/* The in-batch sampled softmax (--loss inbatch).  A batch is B samples (u_b, p_b); every user of the batch scores
 * against every positive of the batch and the other samples' positives are the negatives.  With e the output-table rows:
 *   s_{b,c} = e_{u_b}.e_{p_c},   A_b = { c : c != b, p_c != p_b, u_c != u_b }      (the false negatives the batch itself reveals)
 *   z_{b,c} = (s_{b,c} - s_{b,b}) / tau,   l_b = log(1 + sum_{c in A_b} exp(z_{b,c})),   sm = 1/B sum_b l_b
 *   reg = 0.5/B sum_b ( |e_u|^2 + |e_p|^2 )      (reg_ego: the same on the tables' own rows)
 *   loss_out = {sm + decay * reg, sm, reg}
 * A sample with an out-of-range id is void (err flag, zero terms, no gradient, neither a row nor a column of the score
 * matrix); B in the normalisation stays B.  lgcn_ctx_set_loss(ctx, LGCN_LOSS_INBATCH, tau) is accepted and refused exactly as
 * LGCN_LOSS_SOFTMAX is, and allocates the library-owned workspace (two [max_batch, d] fp32 row tables and a few vectors) once.
 * While it is set, ONLY the two entry points below train: every other training entry point returns 3 and says so, and these
 * two return 3 unless it is set.  Forward, backward chain (over the 2 B slots), Adam epilogue, edge dropout, layer weights and
 * reg_ego are those of lgcn_train_step.  Everything is checked before anything is launched or counted.                        */
#define LGCN_LOSS_INBATCH 2
int lgcn_train_step_inbatch(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, int32_t B, float *loss_out, void *stream);
/* ceil(T/B) consecutive batches of the (already shuffled) arrays; loss_out: [3*ceil(T/B)].                                   */
int lgcn_train_epoch_inbatch(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, int64_t T, int32_t B, float *loss_out,
                             void *stream);

/* Two options of the in-batch step (--score, --inbatch_logq), read by the two entry points above only:
 *   score:      LGCN_SCORE_DOT     e^ = e
 *               LGCN_SCORE_COSINE  e^ = e inv(e),  inv(e) = 1 / |e| if |e| > 0 else 0   (|e| = sqrtf of the fp32 sum of squares)
 *               s_{b,c} = e^_{u_b}.e^_{p_c}
 *   item_logq:  lq, one finite fp32 per item (log of the item's sampling probability up to a constant: the constant cancels),
 *               or NULL = no correction;   z_{b,c} = (s_{b,c} - s_{b,b}) / tau - (lq_{p_c} - lq_{p_b})
 * l_b, sm, q, W are those of the in-batch loss, from this z.  Under cosine the gradient goes through the normalisation:
 *   g_{u_b} = inv(e_u) ( sum_c W[b,c] e^_{p_c} - (sum_c W[b,c] s_{b,c}) e^_{u_b} ) + lam e_{u_b}     (c over A_b and b itself)
 * and its mirror for the items; the reg term and lam e stay on the raw rows, and a row of norm 0 scores 0 and receives no score
 * gradient.  The state is independent of lgcn_ctx_set_loss; a context that is never told holds (LGCN_SCORE_DOT, NULL) and runs
 * the launches it always ran.  item_logq is caller-owned DEVICE memory, [m_items], alive while the context trains.
 * Returns 3 (nothing changed) for a null context or an unknown score kind.                                                    */
#define LGCN_SCORE_DOT 0
#define LGCN_SCORE_COSINE 1
int lgcn_ctx_set_inbatch_scores(lgcn_ctx *ctx, int score, const float *item_logq);
/* The score kind in force (-1: null context); the logq vector goes to item_logq (may be NULL).                                */
int lgcn_ctx_get_inbatch_scores(const lgcn_ctx *ctx, const float **item_logq);

/* Mixed negative sampling for the in-batch step (--inbatch_mix).  A sample carries R sampled negatives
 * n_{b,1..R} (the layouts of lgcn_train_step_multi / lgcn_train_epoch_multi); the B R negatives of the sound samples are a pool
 * SHARED by the whole batch: extra columns of every sample's score row, in the same log-sum-exp.
 *   N_b         = { (c, r) : c sound, n_{c,r} != p_b }        (nothing else is masked; the train graph is not consulted)
 *   z_{b,(c,r)} = (e^_{u_b}.e^_{n_{c,r}} - s_{b,b}) / tau - (lq_{n_{c,r}} - lq_{p_b})
 *   l_b = log(1 + sum_{c in A_b} exp z_{b,c} + sum_{(c,r) in N_b} exp z_{b,(c,r)}),   sm = 1/B sum_b l_b
 *   g_{n_{c,r}} = sum_b W[b,(c,r)] e^_{u_b} + lam/R e_{n_{c,r}}   (cosine: through the pool row's own normalisation)
 *   reg = 0.5/B sum_b ( |e_u|^2 + |e_p|^2 + 1/R sum_r |e_{n_{b,r}}|^2 )
 * An item that is a positive of the batch and named by the pool, or named twice by the pool, counts once per occurrence.  A
 * sample is sound when all 2 + R ids are in range; a void sample contributes no row, no in-batch column and no pool column.
 * At B = 1 the loss is LGCN_LOSS_SOFTMAX's at the same R and tau; with an empty pool it is the in-batch loss above.
 * lgcn_ctx_set_inbatch_mix(ctx, R_max): 0 = off (the default); 1..LGCN_MAX_NEG_RATIO while LGCN_LOSS_INBATCH is set allocates the
 * library-owned workspace again, for (1 + R_max) item rows per sample -- never inside a step.  Returns 3 (nothing changed) for
 * a null context, R_max out of range, or a context whose loss is not LGCN_LOSS_INBATCH; 4 if the workspace cannot be allocated.
 * The two entry points return 3, naming the cause, before anything is launched or counted: loss not inbatch, mixing not set,
 * R < 1 or R > R_max, neg_stride < B, a null pointer, B > max_batch.  lgcn_train_step_inbatch on the same context stays the
 * step it is on a context that was never told (bit for bit); every other entry point refuses as before.                      */
int lgcn_ctx_set_inbatch_mix(lgcn_ctx *ctx, int32_t R_max);
/* R_max in force (0: off; -1: null context).                                                                                  */
int32_t lgcn_ctx_get_inbatch_mix(const lgcn_ctx *ctx);
int lgcn_train_step_inbatch_mix(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, const int32_t *negs, int64_t neg_stride,
                                int32_t R, int32_t B, float *loss_out, void *stream);
/* negs: [R][T]; ceil(T/B) consecutive batches; loss_out: [3*ceil(T/B)].                                                       */
int lgcn_train_epoch_inbatch_mix(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, const int32_t *negs, int32_t R,
                                 int64_t T, int32_t B, float *loss_out, void *stream);

/* The alignment-and-uniformity loss (--loss directau): DirectAU (Wang et al., KDD 2022), training with no negatives.
 * A batch is B samples (u_b, p_b).  With e the output-table rows, e^ = e inv(e) (inv as under LGCN_SCORE_COSINE), x_b = e^_{u_b},
 * y_b = e^_{p_b}:
 *   align   = 1/B sum_b |x_b - y_b|^2
 *   unif(X) = log( 1/npairs sum_{b<c} exp(-2 |x_b - x_c|^2) ),   npairs = B (B - 1) / 2      (pairs BY POSITION: two samples naming
 *                                                                  the same user are a pair of distance 0; torch.pdist over the batch)
 *   reg     = 0.5/B sum_b ( |e_u|^2 + |e_p|^2 )      (on the raw rows; reg_ego: the same on the tables' own rows)
 *   loss_out = {au + decay * reg, au, reg},   au = align + gamma (unif(X) + unif(Y)) / 2
 * A sample with an out-of-range id is void (err flag, no alignment term, part of no pair, no gradient); the divisors stay B and
 * B (B - 1) / 2.  With fewer than two sound samples (B = 1 included) both unif terms are 0 and contribute no gradient: no log of 0
 * is taken.  The gradient goes through the normalisation as under LGCN_SCORE_COSINE; the reg term and lam e stay on the raw rows.
 * lgcn_ctx_set_directau(ctx, gamma), gamma finite and >= 0, sets the loss (lgcn_ctx_get_loss then returns LGCN_LOSS_DIRECTAU) and
 * allocates the library-owned workspace (two [max_batch, d] fp32 row tables and a few vectors) once, before anything is changed.
 * rc 3, with a message naming directau and nothing changed: a null context, a bad gamma, LGCN_FP8 storage, an optional branch,
 * dense_last = 0, hard negatives set, mixed negatives set; rc 4 if the workspace cannot be allocated.  lgcn_ctx_set_loss(ctx,
 * LGCN_LOSS_BPR, anything) leaves the loss; lgcn_ctx_set_loss(ctx, LGCN_LOSS_DIRECTAU, anything) returns 3 and names this setter.
 * While it is set, ONLY the two entry points below train: every other training entry point returns 3 and says so, and these two
 * return 3 unless it is set.  Forward, backward chain (over the 2 B slots), Adam epilogue, edge dropout, layer weights and reg_ego
 * are those of lgcn_train_step_inbatch.  Everything is checked before anything is launched or counted.                         */
#define LGCN_LOSS_DIRECTAU 4
int lgcn_ctx_set_directau(lgcn_ctx *ctx, float gamma);
/* 0, and gamma to *gamma (may be NULL), while the loss is set; 3 (and *gamma untouched) for a null context or another loss.    */
int lgcn_ctx_get_directau(const lgcn_ctx *ctx, float *gamma);
int lgcn_train_step_directau(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, int32_t B, float *loss_out, void *stream);
/* ceil(T/B) consecutive batches of the (already shuffled) arrays; loss_out: [3*ceil(T/B)].                                   */
int lgcn_train_epoch_directau(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, int64_t T, int32_t B, float *loss_out,
                              void *stream);

/* Hard negatives for the multi-negative step: dynamic negative sampling, DNS(M, N) (--hard_neg M).  A sample is
 * (u_b, p_b, n_{b,1..R}) in the layouts of lgcn_train_step_multi / lgcn_train_epoch_multi, R >= 2.  The step scores the R
 * candidates with the current model, s_r = e_u.e_{n_r}, ranks them by s descending (ties: r ascending), picks rank
 *   j_b = lgcn_hard_neg_rank(seed, step, b, M)        (step: the Adam step counter BEFORE the step, as the dropout mask's)
 * and is then exactly lgcn_train_step's BPR step on the B triplets (u_b, p_b, n_sel(b)):
 *   bpr = -1/B sum_b logsigmoid(e_u.e_p - e_u.e_sel),   reg = 0.5/B sum_b (|e_u|^2 + |e_p|^2 + |e_sel|^2)   (reg_ego: own rows)
 * Gradient rows, row flags and reg_ego slot counts go to u, p and n_sel only, each of weight 1; the divisor is B.  The R - 1
 * unselected candidates receive nothing.  M = 1 trains the hardest candidate, M = R a uniform one.  Forward, backward chain,
 * Adam epilogue, edge dropout, layer weights and reg_ego are the multi-negative step's; the gradient-row conversion is never
 * folded (the touched rows are not known ahead).  A sample with an out-of-range id is void as before.
 * lgcn_ctx_set_hard_neg(ctx, top_m, seed, sel_out): top_m = 0 (the default) restores exactly the launches of a context that
 * was never told.  sel_out: caller-owned DEVICE memory [max_batch], alive while it is set, or NULL; every step stores the
 * selected index r of sample b to sel_out[b] (-1: void sample).  rc 3 with a message naming hard negatives and nothing changed:
 * top_m outside 0..LGCN_MAX_NEG_RATIO, a loss other than LGCN_LOSS_BPR in force, LGCN_FP8 storage, an optional branch,
 * dense_last = 0; rc 4 if the [max_batch] ids cannot be allocated.  While it is set: lgcn_ctx_set_loss to another loss returns
 * 3; lgcn_train_step_multi / lgcn_train_epoch_multi return 3, naming R and M, for R < 2 or M > R (outputs, step counter and
 * workspace untouched); every three-slot, in-batch and rank-splitting entry point returns 3 and says so.                      */
int lgcn_ctx_set_hard_neg(lgcn_ctx *ctx, int32_t top_m, uint64_t seed, int32_t *sel_out);
/* M in force (0: off; -1: null context).                                                                                      */
int32_t lgcn_ctx_get_hard_neg(const lgcn_ctx *ctx);
/* The pick j_b in 0..M-1 on the host (no GPU): the function the kernel calls.  M <= 1 gives 0.                                */
uint32_t lgcn_hard_neg_rank(uint64_t seed, int64_t step, int32_t b, int32_t M);

/* The fold of the gradient-row conversion into the batch-row launch.  lgcn_train_epoch holds all triplets of
 * the call before its first step, so it computes once (per segment of 1024 steps) how many slots of each batch name each
 * destination row; the batch-row kernel then writes the fp32 copy of a gradient row itself -- directly where one slot names
 * the row, from the workgroup that adds last (an arrival ticket, nobody waits) where several do -- and the step launches no
 * k_g32.  The results are bit for bit those of the unfolded step.  On by default; it engages in lgcn_train_epoch only, for
 * the default model (no i2i / popularity gate), without a hub plan (lgcn_ctx_hub_rows() == 0) and for B <= 4096.  Every other
 * entry point, and lgcn_train_epoch with the switch off, launches what it launched before.                                  */
int lgcn_ctx_set_fold_g32(lgcn_ctx *ctx, int on);
/* steps run with the fold since the context was created (tests: did it engage?) */
int64_t lgcn_ctx_folded_steps(const lgcn_ctx *ctx);
/* debug: copies the first n entries of the fold's per-row arrival counters to HOST memory after a device synchronise; they
 * are zero between steps (the array is allocated by the first lgcn_train_epoch call that folds; before that, zeros are
 * written).  rc 3: no such array (optional branches) or n > N.                                                              */
int lgcn_ctx_copy_arrivals(const lgcn_ctx *ctx, int32_t *dst_host, int64_t n);

/* The store policy of outputs that are read once, row by row, and never gathered.  A plain store keeps its
 * line dirty in the writing XCD's L2; a write-through store (16 bytes per lane, sc1) sends it on and drops the line, so the
 * launch ends with that much less to write back and the write-once lines do not compete with the table the launch gathers.
 *   LGCN_STORE_ADAM  (bit 0): the Adam epilogue writes the rows of M and V write-through, and those of P where a bf16 / fp8
 *                             shadow of P is maintained by the same epilogue (fp32 tables gather P itself: plain).
 *   LGCN_STORE_XLAST (bit 1): the forward launch whose output only the batch-row kernel gathers (X_{K-1} of a context with the
 *                             gathered last layer) writes it write-through.  fp32 and bf16 tables; fp8 tables keep plain stores.
 * Arithmetic, and every result, is bit for bit the same under every policy.  Any other bit: rc 3.  A new context takes
 * LGCN_STORE_POLICY from the environment (0..3, read at lgcn_ctx_create; anything else makes the create fail with rc 3) or,
 * without it, the library's default.                                                                                          */
#define LGCN_STORE_ADAM 1
#define LGCN_STORE_XLAST 2
int lgcn_ctx_set_store_policy(lgcn_ctx *ctx, int bits);
/* -> the context's policy bits.  launch_out (or NULL): [2] the store field the last +Adam launch and the last forward launch of
 * the deepest layer carried (LGCN_STORE_ARG_* bits; 0 before the first step).  ctx == NULL: what a context created now would
 * start with (-1: LGCN_STORE_POLICY is set and is not one of 0..3).                                                            */
#define LGCN_STORE_ARG_MV 1     /* M and V rows write-through */
#define LGCN_STORE_ARG_P 2      /* P rows write-through */
#define LGCN_STORE_ARG_Y 4      /* the launch's output table write-through */
int lgcn_ctx_get_store_policy(const lgcn_ctx *ctx, int32_t *launch_out);
/* Slot multiplicities of a multi-step call: the triplets [0, T) (device int32 ids) are cut into consecutive batches of B, the
 * last one shorter; for batch i of b_i triplets and slot s = c * b_i + b (c = 0 user, 1 positive, 2 negative),
 * mult_out[3 * i * B + s] = the number of slots of batch i whose destination row is slot s's (user u -> row u, item j -> row
 * n_users + j), counting only triplets whose three ids are in range; the three slots of a triplet with an out-of-range id
 * get 0.  mult_out: device, 3 * T values of 16 bits (a batch that fits has at most 12 288 slots).  rc 3 where the row ids of
 * a batch do not fit the kernel's LDS hash (B > 4096) or N >= 2^31.  No host sync.                                          */
int lgcn_slot_multiplicity(const int32_t *users, const int32_t *pos, const int32_t *neg, int64_t T, int32_t B,
                           int32_t n_users, int64_t N, uint16_t *mult_out, void *stream);

/* Data-parallel split of the same step (replicated tables, batch sharded):
 *   part 1  forward propagation + per-triplet loss terms and gradient rows for this
 *           rank's shard [rank*S, min((rank+1)*S, B_global)), S = ceil(B_global/world),
 *           written to cfg.contrib as [3*S*d gradient rows | S loss | S reg terms];
 *   (caller: RCCL all-gather of that block over the ranks into `gathered`)
 *   part 2  order-independent reduction of all ranks' rows, backward propagation
 *           and Adam -- bitwise identical on every rank and to lgcn_train_step.  */
/* Floats per rank of the exchange block for a global batch of B_global triplets over `world` ranks (S = ceil(B_global/world)):
 * 3*S*d + 2*S for the default model; with the popularity gate 3*S*d + 3*S (third term block: the gates' entropy), padded to
 * an even count, + 2*P floats holding P int64 = the rank's fixed-point sums of the MLP parameter gradients.  cfg.contrib must
 * hold that many floats for the largest batch, `gathered` world times as many.  The optional branches are supported in the
 * gradient-row exchange (LGCN_DP_ROWS) only.                                                                      */
int64_t lgcn_dp_block_floats(const lgcn_ctx *ctx, int32_t B_global, int32_t world);
int lgcn_train_step_dp_part1(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos,
                             const int32_t *neg, int32_t B_global, int32_t world, int32_t rank,
                             void *stream);
/* The literal north_star form (dense gradient all-reduce), kept as an alternative:
 *   dense part 1  forward + this rank's shard accumulated into ITS OWN G64 / bitmap / loss terms
 *                 (1/B and decay/B of the global batch);
 *   (caller: RCCL all-reduce SUM of G64 [N*d int64] and of terms [2*B_global fp32]; the row bitmap
 *    is flagged for the whole global batch on every rank and needs no collective)
 *   part 2 with gathered == NULL: backward + Adam from the reduced G64.
 * Integer sums commute, so this is again bitwise equal to lgcn_train_step -- but it moves
 * N*d*8 bytes per step (Gowalla 36 MB) instead of 1.6 MB.
 * With the popularity gate on, terms carries a third block (the gates' entropy: all-reduce 3*B_global
 * floats) and the rank's fixed-point sums of the MLP parameter gradients sit in the buffer
 * lgcn_ctx_gate_total names (int64[count]): all-reduce SUM it too before part 2.
 * (the reference trains on one device: model.py:139-157,176-181 define what is summed)      */
int lgcn_train_step_dp_dense_part1(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos,
                                   const int32_t *neg, int32_t B_global, int32_t world, int32_t rank,
                                   void *stream);
int lgcn_ctx_gate_total(const lgcn_ctx *ctx, void **buf, int32_t *count);   /* count 0 without the gate */
int lgcn_train_step_dp_part2(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos,
                             const int32_t *neg, int32_t B_global, int32_t world,
                             const float *gathered, float *loss_out, void *stream);

/* Column-sharded data parallelism (LGCN_DP_COLS): rank r holds columns [r*d/W, (r+1)*d/W) of the tables -- its context is an
 * ordinary context of width d/W (32/64/128/256) over the same graph, cfg.contrib holding 3*max_batch*(d/W) floats.  Every rank
 * sees the WHOLE batch.  part 1: forward + the batch's slot rows + the PARTIAL scores / reg terms over this rank's columns
 * (*partials = device float[3*B]: pos score | neg score | reg term); the caller all-reduces (SUM) those 3*B floats over the
 * ranks IN PLACE; part 2: loss terms, gradient rows of this rank's columns, backward, Adam.  One 3*B-float collective per
 * step and per-rank SpMM work that falls with W.  Equal to lgcn_train_step up to the summation order of the dot products
 * (W partial sums).  lgcn_train_epoch_dp(reduce = LGCN_DP_COLS) runs the loop with the all-reduce on the communicator.     */
int lgcn_train_step_cols_part1(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, const int32_t *neg,
                               int32_t B, float **partials, void *stream);
int lgcn_train_step_cols_part2(lgcn_ctx *ctx, const int32_t *users, const int32_t *pos, const int32_t *neg,
                               int32_t B, float *loss_out, void *stream);

/* ------------------------------------------------------------------------ */
/* Device: fused full-ranking evaluation -- replaces the body of Procedure.Test  */
/* ------------------------------------------------------------------------ */
/* For every listed user: scores against ALL items (model.getUsersRating, model.py:114-123:
 * U_b . I^T on the propagated table E[N,d] -- matrix cores, fp32 accumulate, fp32-accurate), train positives
 * set to -(1<<10) (Procedure.py:177-181; CSR with int64 indptr[n_users+1] and ascending int32
 * indices = dataset.allPos), top-K (Procedure.py:183) -- in one kernel, the [users, m_items]
 * score matrix is never materialised.  topk_items [n_eval,K] int32, ordered by (score descending, item id
 * ascending).  Every item scoring strictly above the K-th score is returned; WHICH of several items whose scores tie
 * EXACTLY at the K-th score are returned is unspecified, for every catalogue size (as torch.topk's choice is) -- the
 * ones returned are distinct and in id order;
 * topk_scores [n_eval,K] or NULL.  1 <= K <= 64 (Procedure.py:183 takes k = max(topks)).          */
int lgcn_eval_topk(const float *E, int32_t n_users, int32_t m_items, int32_t d,
                   const int32_t *users, int32_t n_eval,
                   const int64_t *train_indptr, const int32_t *train_indices,
                   int32_t K, int32_t *topk_items, float *topk_scores, void *stream);
/* The same with the train-positive masks precomputed ONCE per dataset instead of walked from the CSR inside the sweep:
 * masks = lgcn_eval_mask_words(m_items, n_eval) uint32 words filled by lgcn_eval_build_masks (word [t * stride + slot],
 * stride = n_eval rounded up to 128: bit i = item 32 t + i is a train positive of users[slot]).  The sweep then holds
 * no global load besides the item tiles and one coalesced mask load per wave and tile.  Same results.          */
int64_t lgcn_eval_mask_words(int32_t m_items, int32_t n_eval);
int lgcn_eval_build_masks(const int32_t *users, int32_t n_eval, const int64_t *train_indptr, const int32_t *train_indices,
                          int32_t m_items, uint32_t *masks, void *stream);
int lgcn_eval_topk_masked(const float *E, int32_t n_users, int32_t m_items, int32_t d,
                          const int32_t *users, int32_t n_eval,
                          const int64_t *train_indptr, const int32_t *train_indices,
                          int32_t K, int32_t *topk_items, float *topk_scores, const uint32_t *masks, void *stream);
/* The same, with every score produced by the fp32 matrix instructions (v_mfma_f32_32x32x2_f32).  lgcn_eval_topk itself
 * computes the fp32 product on the bf16 matrix cores where it can (d <= 64, at most 65 K items per part of the catalogue: three parts for
 * K <= 20, two for K <= 64; d = 128 with K <= 20): both operands split EXACTLY into three bf16 values each, six of the nine product planes accumulated in
 * fp32 -- the planes left out are below the rounding of an fp32 dot product, so both entry points are fp32-accurate and
 * may differ only where two scores tie within that rounding.  This one is the slower cross-check.          */
int lgcn_eval_topk_fp32(const float *E, int32_t n_users, int32_t m_items, int32_t d,
                        const int32_t *users, int32_t n_eval,
                        const int64_t *train_indptr, const int32_t *train_indices,
                        int32_t K, int32_t *topk_items, float *topk_scores, void *stream);
/* Per-user precision / recall / NDCG at the cut-offs ks[n_ks] (Procedure.test_one_batch,
 * Procedure.py:89-121; utils.RecallPrecision_ATk / NDCGatK_r / getLabel, utils.py:173-217) from the
 * ranked ids and the users' test lists (CSR over the n_eval slots, ids ASCENDING per slot), in
 * float64; per_user [n_eval, 3*n_ks] = precision | recall | ndcg, sums [3*n_ks] = their sums over
 * the users in a fixed order (the reference averages them, Procedure.py:191-192).        */
int lgcn_eval_metrics(const int32_t *topk_items, int32_t n_eval, int32_t K,
                      const int64_t *test_indptr, const int32_t *test_items_sorted,
                      const int32_t *ks, int32_t n_ks, double *per_user, double *sums, void *stream);
/* Evaluation past K = 64 (the entry points above keep their 1..64 contract).  lgcn_eval_kmax: the largest K the _ex forms
 * take (256; a larger max(topks) stays with the caller's own ranking).  lgcn_eval_topk_ex ranks as lgcn_eval_topk_masked
 * (same semantics, same tie caveat; a user with fewer than K items that are not train positives gets train positives at -(1<<10)
 * in the tail -- which of them, when more are left than places, is such a tie): 1 <= K <= lgcn_eval_kmax(), K <= m_items; topk_items and topk_scores (or NULL) are [n_eval, K] contiguous and
 * out_capacity is the number of elements each of them holds -- rc 3, and nothing launched, if n_eval * K > out_capacity.
 * masks: as lgcn_eval_topk_masked, or NULL (the cursor over the train CSR).  flags: LGCN_EVAL_FP32 = every score from the fp32
 * matrix instructions (the cross-check, as lgcn_eval_topk_fp32), else the split bf16 product where the sweep supports it.
 * K <= 64 runs the very sweep of lgcn_eval_topk_masked / lgcn_eval_topk_fp32 (bitwise the same output); 64 < K <= 256 a
 * sweep with 128- or 256-slot lists and 128 or 64 users per workgroup.
 * lgcn_eval_metrics_ex: lgcn_eval_metrics for K <= lgcn_eval_kmax() (cut-offs in any order), same outputs; for K <= 64
 * bitwise those of lgcn_eval_metrics.                                                                                 */
#define LGCN_EVAL_FP32 1
int32_t lgcn_eval_kmax(void);
int lgcn_eval_topk_ex(const float *E, int32_t n_users, int32_t m_items, int32_t d,
                      const int32_t *users, int32_t n_eval,
                      const int64_t *train_indptr, const int32_t *train_indices, const uint32_t *masks,
                      int32_t K, int32_t *topk_items, float *topk_scores, int64_t out_capacity,
                      int32_t flags, void *stream);
int lgcn_eval_metrics_ex(const int32_t *topk_items, int32_t n_eval, int32_t K,
                         const int64_t *test_indptr, const int32_t *test_items_sorted,
                         const int32_t *ks, int32_t n_ks, double *per_user, double *sums, void *stream);
/* Rank-based evaluation: any cut-off up to m_items, AUC (utils.AUC, utils.py:203-209) and MRR, from one item sweep whose
 * cost does not depend on a cut-off (additive to ABI 13; the entry points above are unchanged).
 * For evaluation slot s with user u = users[s], train positives P_u (the sorted CSR), test list T_u (test_indptr over the
 * n_eval slots, ids ASCENDING per slot, n_test = test_indptr[n_eval] entries in all) and the reference's row
 * L_u[j] = <E[u], E[n_users + j]> in fp32 accuracy, or -(1<<10) for j in P_u (Procedure.py:177-181), lgcn_eval_ranks writes
 * per test entry t (three arrays of n_test elements, in the order of test_items_sorted):
 *   test_scores[t] = L_u[t]                                   (so -1024 when t is also a train positive)
 *   gt[t] = #{ j not in P_u or T_u : L_u[j] >  test_scores[t] }
 *   eq[t] = #{ j not in P_u or T_u : L_u[j] == test_scores[t] }
 * The counts are integers added in any order: bitwise reproducible, whatever the split of the sweep.  flags: LGCN_EVAL_FP32
 * = every score from the fp32 matrix instructions, else the split bf16 product (d <= 128).
 * lgcn_eval_rank_metrics derives, per slot, pos[t] = the position of t in L_u sorted best first:
 *   TIE RULES: a tie between a test item and a non-test item goes AGAINST the test item (the non-test item ranks first: a
 *   constant table scores nothing); a tie among test items goes to the LOWER id.  The train positives outside T_u sit at
 *   -1024 and rank above a test item whose score is <= -1024.
 * and from it hit@K = [pos[t] < K] for any cut-off 1 <= ks[q] <= m_items (ks: HOST pointer, 1..8 cut-offs, any order),
 * precision / recall / NDCG by the formulas of lgcn_eval_metrics_ex (same additions, same order),
 *   AUC_u = sum_t (#{j not in T_u : L_u[j] < score[t]} + 1/2 #{j not in T_u : L_u[j] == score[t]}) / (n (m_items - n)),
 *           = roc_auc_score(r_all, L_u); 0 for a slot with n = 0 or n = m_items,
 *   MRR_u = 1 / (1 + min_t pos[t]); 0 for an empty list.
 * per_user [n_eval, 3*n_ks + 2] = precision | recall | ndcg | auc | mrr in float64, sums [3*n_ks + 2] their sums over the
 * slots in a fixed order.  n_test sizes the temporaries (stream-ordered; nothing synchronises) and bounds every access to
 * the per-entry arrays: entries at or past n_test are never read or written.
 * rc 3, nothing launched and no output written: d outside {32, 64, 128, 256}, a negative size, n_test > n_eval * m_items, a
 * NULL array, an unknown flag, a cut-off outside [1, m_items].                                                          */
int lgcn_eval_ranks(const float *E, int32_t n_users, int32_t m_items, int32_t d,
                    const int32_t *users, int32_t n_eval,
                    const int64_t *train_indptr, const int32_t *train_indices,
                    const int64_t *test_indptr, const int32_t *test_items_sorted, int64_t n_test,
                    float *test_scores, int32_t *gt, int32_t *eq, int32_t flags, void *stream);
int lgcn_eval_rank_metrics(int32_t n_eval, int32_t m_items, const int32_t *users,
                           const int64_t *train_indptr, const int32_t *train_indices,
                           const int64_t *test_indptr, const int32_t *test_items_sorted, int64_t n_test,
                           const float *test_scores, const int32_t *gt, const int32_t *eq,
                           const int32_t *ks, int32_t n_ks, double *per_user, double *sums, void *stream);
/* Popularity-aware evaluation from the ranked lists (additive to ABI 13; csrc/lgcn_eval_pop.hip): which items
 * the lists hold.  Inputs: topk_items [n_eval, K] as lgcn_eval_topk_ex wrote it (the ids of a list DISTINCT; an id outside
 * [0, m_items), the -1 padding, counts nowhere), the test CSR over the slots as lgcn_eval_metrics_ex takes it (ids ascending,
 * test_indptr[n_eval] entries; a test id outside [0, m_items) belongs to no group), and one packed word per item,
 * item_info[i] = pop_i * 8 + g_i: pop_i < 2^28 the item's train interactions, g_i its popularity group (0 = the most popular).
 * The group is read as `word & 7` and every per-group array in the kernels holds 8 columns, so no content of item_info can
 * index out of bounds; an item with g_i >= n_groups is counted in `valid`, the popularity sum and the exposures, and in no
 * reported group column.  ks: HOST pointer, 1..8 cut-offs in 1..K, any order, duplicates allowed.
 * With L_s the list and T_s the test list of slot s, h[s,g,k] = #{r < k : L_s[r] in T_s, g(L_s[r]) = g}, t[s,g] = #{i in T_s :
 * g_i = g}, e_k[i] = #{s : i among the first k entries of L_s} (the exposure):
 *   sums_f64 [n_ks, 2, n_groups]   [q][0][g] = sum_s h[s,g,k] / |T_s|  (a slot with an empty T_s adds 0; over g and / n_eval: Recall@k)
 *                                  [q][1][g] = sum_{s : t[s,g] > 0} h[s,g,k] / t[s,g]     (recall on the group's test items)
 *   group_slots [n_groups]         #{s : t[s,g] > 0}
 *   counts_i64 [n_ks, n_groups+5]  [q][g] = list entries of group g among the first k | [n_groups] valid entries among the first
 *                                  k | [n_groups+1] sum of pop over them | [n_groups+2] #{i : e_k[i] > 0} | [n_groups+3] sum_i e_k[i]
 *                                  | [n_groups+4] sum_{i<j} |e_k[i] - e_k[j]|, the Gini numerator (Gini = it / (m_items sum_i e_k[i]))
 *   exposure [n_ks, m_items] or NULL   e_k[i] (when given it also serves as the kernels' bucket array: no temporary of that size)
 *   per_slot [n_eval, n_ks, 2, n_groups] or NULL   the two quotients of every slot, each one correctly rounded division
 * Every count is an integer sum (order-free, exact); the two float64 sums are added in an order that depends on n_eval and K
 * alone (per-workgroup partials merged in a fixed order): all outputs are bitwise reproducible, with or without per_slot.  A list
 * entry costs ONE integer atomic add (into the exposure bucket of the smallest cut-off above its position); the Gini numerator is
 * sum_v v H[v] (2 R_v + H[v] - m_items) over the histogram H of the exposure values, R_v = sum_{w<v} H[w]: no sort, no floats.
 * The temporaries come from the stream-ordered pool; nothing synchronises.  n_eval == 0: the outputs are zeroed, nothing else runs.
 *   rc 3  nothing launched, no output written: n_groups or n_ks outside 1..8, K outside 1..lgcn_eval_kmax(), a cut-off outside
 *         1..K, n_eval < 0, m_items < 1, a NULL array other than exposure / per_slot, n_eval * K * m_items >= 2^62 (the Gini
 *         numerator could leave int64); the message names the argument
 *   rc 4  the temporaries cannot be allocated: nothing launched                                                           */
int lgcn_eval_pop_metrics(const int32_t *topk_items, int32_t n_eval, int32_t K,
                          const int64_t *test_indptr, const int32_t *test_items_sorted,
                          const uint32_t *item_info, int32_t m_items, int32_t n_groups,
                          const int32_t *ks, int32_t n_ks,
                          double *sums_f64, int64_t *counts_i64, int64_t *group_slots,
                          int32_t *exposure, double *per_slot, void *stream);

/* ------------------------------------------------------------------------ */
/* Item-item co-occurrence graph (preprocess_instacart_i2i.py:61-170)         */
/* ------------------------------------------------------------------------ */
/* build_item_item on the device, in two stages.  UNLIKE the entry points above these two own their
 * temporaries (stream-ordered allocations) and synchronise `stream` ONCE, at the end, to read the device's verdict; every
 * kernel that writes an output reads that verdict first, so a refused call leaves all outputs as they were.  All pointers
 * are device pointers except nnz_out.
 * The first stage (topk): baskets as a CSR (indptr[n_baskets + 1] with indptr[n_baskets] == nnz, indices[nnz]; the items of
 * a basket DISTINCT, in any order); baskets are numbered in input order, one with fewer than min_basket items is skipped.
 * c[i][j] = kept baskets holding both, deg[i] = kept baskets holding i, total = kept baskets (1.0 if none); weight in fp64:
 * LGCN_I2I_COOC c | LGCN_I2I_JACCARD c / (deg_i + deg_j - c) (0 if that is <= 0) | LGCN_I2I_PMI max(log(c total / (deg_i
 * deg_j) + 1e-12), 0).  Per item the topk best by (weight descending, first kept basket holding both ascending, j ascending)
 * -- the order heapq.nlargest leaves the reference's dict in -- in RANK order: cols [m_items, topk] padded with -1,
 * w [m_items, topk] = (float)weight padded with 0, len [m_items].  Bitwise reproducible.
 *   rc 3  topk outside 1..256, unknown weight, min_basket < 0, n_baskets / nnz / m_items <= 0 (or above 0x7f000000),
 *         2 m_items topk >= 2^31, a null pointer: nothing launched
 *   rc 4  the temporaries cannot be allocated from the stream-ordered pool: nothing launched
 *   rc 5  an item id outside [0, m_items)      } found on the device before anything is counted;
 *   rc 6  indptr not ascending from 0 to nnz   } cols / w / len untouched
 *   rc 10 a runtime call failed
 * The second stage (finish): entry (i, j) exists if j is in i's list or i in j's (weight = the maximum; weights <= 0 are
 * not stored), deg = fp32 row sum (0 -> 1), value = (v * deg_i^-1/2) * deg_j^-1/2 in fp32 -> CSR with ascending columns:
 * indptr [m_items + 1], indices / vals [capacity], *nnz_out (HOST) = entries written.  cols of a row must be distinct.
 *   rc 3  topk outside 1..256, m_items <= 0, capacity <= 0, 2 m_items topk >= 2^31, a null pointer: nothing launched
 *   rc 4  the temporaries cannot be allocated from the stream-ordered pool: nothing launched
 *   rc 7  capacity < 2 * sum(len) (summed on the device): indptr / indices / vals / *nnz_out untouched
 *   rc 10 a runtime call failed                                                                                        */
enum { LGCN_I2I_COOC = 0, LGCN_I2I_JACCARD = 1, LGCN_I2I_PMI = 2 };
int lgcn_i2i_topk(const int64_t *indptr, const int32_t *indices, int64_t n_baskets, int64_t nnz, int32_t m_items,
                  int32_t topk, int32_t weight, int32_t min_basket, int32_t *cols, float *w, int32_t *len, void *stream);
int lgcn_i2i_finish(const int32_t *cols, const float *w, const int32_t *len, int32_t m_items, int32_t topk, int64_t capacity,
                    int32_t *indptr, int32_t *indices, float *vals, int64_t *nnz_out, void *stream);

/* ------------------------------------------------------------------------ */
/* Data parallel over RCCL (no counterpart in the reference: SURVEY 2, north_star) */
/* ------------------------------------------------------------------------ */
/* RCCL is resolved at run time (dlopen of the librccl already mapped into the process, else
 * $LGCN_RCCL_PATH, else the system one); the library itself does not link it.  One communicator
 * per process / GPU.  Rank 0 creates the 128-byte id (ncclGetUniqueId) and the caller hands it to
 * every rank through any channel it has (torch.distributed store, MPI, a file).             */
#define LGCN_DP_ID_BYTES 128
enum { LGCN_DP_ROWS = 0, LGCN_DP_DENSE = 1, LGCN_DP_ROW_SHARDED = 2, LGCN_DP_COLS = 3 };
typedef struct lgcn_dp lgcn_dp;   /* opaque */
int lgcn_dp_available(void);                         /* 1 if RCCL could be resolved */
int lgcn_dp_unique_id(void *id128);
int lgcn_dp_init(const void *id128, int world, int rank, lgcn_dp **out);   /* on the current HIP device */
/* TEST HOOK, no RCCL involved: `world` communicators for `world` THREADS OF THIS PROCESS on the current device
 * (out[world]; destroy each with lgcn_dp_destroy).  Their collectives meet on a host barrier and move the blocks
 * with hipMemcpyAsync on the calling rank's stream, so lgcn_train_epoch_dp's world > 1 control flow can run -- and
 * be compared bit for bit with the single-GPU epoch -- on a one-GPU machine: every thread calls
 * lgcn_train_epoch_dp with its own context, tables, stream and communicator.  Synchronous by construction. */
int lgcn_dp_init_loopback(int world, lgcn_dp **out);
void lgcn_dp_destroy(lgcn_dp *dp);
/* In-place SUM all-reduce of n device floats over the communicator, on `stream` (no host sync).  bench.py counts the ranks
 * RCCL itself sees with it (an all-reduce of 1.0 per rank), independent of torch.distributed's WORLD_SIZE. */
int lgcn_dp_allreduce_sum_f32(lgcn_dp *dp, float *buf, int64_t n, void *stream);
int lgcn_dp_world(const lgcn_dp *dp);
int lgcn_dp_rank(const lgcn_dp *dp);
/* A whole data-parallel epoch in one host call: the loop of main.py:223-225 over ceil(T/B_global)
 * global batches (arrays identical on every rank); per batch: part 1, the collective on `stream`
 * (reduce = LGCN_DP_ROWS: ncclAllGather of cfg.contrib blocks into `gathered`
 * [world * (3*S*d + 2*S)] floats, S = ceil(B_global/world); LGCN_DP_DENSE: ncclAllReduce of G64 and
 * of the loss terms, `gathered` unused), part 2.  No host synchronisation.  loss_out: [3*steps].
 * LGCN_DP_ROW_SHARDED: the row-sharded step below, every exchange one grouped in-place
 * ncclBroadcast of the owners' row ranges; row_ranges = HOST int64[world][4] = {user rows lo, hi,
 * item rows lo, hi} (row ids of the [N,d] tables) owned by each rank, else NULL.          */
int lgcn_train_epoch_dp(lgcn_ctx *ctx, lgcn_dp *dp, const int32_t *users, const int32_t *pos,
                        const int32_t *neg, int64_t T, int32_t B_global, int32_t reduce,
                        const int64_t *row_ranges, float *gathered, float *loss_out, void *stream);

/* Row-sharded propagation (SURVEY 8e "beyond the contract"; analogue of the reference's A_split row
 * folds, dataloader.py:192-201).  Tables stay replicated in layout; the graph handed to the context was
 * created with row_order = ONLY the rows this rank owns (n_order < n_rows), so every SpMM phase
 * computes 1/world of a layer and the owners' rows are exchanged before the next phase:
 *   FWD k = 1..K-1   X_k[owned] = (A X_{k-1})[owned]                       -> exchange lgcn_rs_buffer(FWD,k)
 *   BPR              this rank's batch shard -> cfg.contrib (as dp part 1)  -> all-gather of the blocks
 *   SCATTER          all ranks' gradient rows -> G64 + row flags (every rank, identical)
 *   BWD k = K..1     h_{k-1}[owned] = Gs + (A h_k)[owned]; k = 1: Adam on the owned rows
 *                                                                          -> exchange lgcn_rs_buffer(BWD,k)
 *   FINISH           zero the batch rows of G64 and their flags, reduce the loss
 * Every row is computed by the same code in the same order wherever it runs, so the result is
 * bitwise identical to lgcn_train_step.  Adam state (m, v) of a row lives on its owner only.
 * An exchanged buffer of dtype LGCN_FP8 is an fp8 table (lgcn_table_bytes): a caller running the
 * phases itself moves the owners' rows (d bytes each) AND their row scales (fp32, behind the rows).   */
enum { LGCN_RS_FWD = 0, LGCN_RS_BPR = 1, LGCN_RS_SCATTER = 2, LGCN_RS_BWD = 3, LGCN_RS_FINISH = 4 };
int lgcn_rs_phase(lgcn_ctx *ctx, int32_t phase, int32_t k, const int32_t *users, const int32_t *pos,
                  const int32_t *neg, int32_t B_global, int32_t world, int32_t rank,
                  const float *gathered, float *loss_out, void *stream);
int lgcn_rs_buffer(const lgcn_ctx *ctx, int32_t phase, int32_t k, void **buf, int32_t *dtype);

/* reads and clears the device error flag (synchronises the stream): 0 = none,
 * 1 = id out of range in users/pos/neg.                                        */
int lgcn_ctx_check(lgcn_ctx *ctx, void *stream);

/* ------------------------------------------------------------------------ */
/* Device: matrix factorisation (--model mf) -- replaces BPRLoss.stageOne    */
/*   utils.py:53-64 on upstream LightGCN's PureMF (the model the reference's */
/*   register.py:43-44 registers "if it exists"):                            */
/*   = PureMF.bpr_loss (embedding lookups, softplus(neg - pos).mean(), the    */
/*     L2 term on the looked-up rows) + loss.backward() + torch.optim.Adam    */
/*     .step on the DENSE gradient of both tables (utils.py:51,62)            */
/* ------------------------------------------------------------------------ */
/* No graph and no propagation: the scores are dot products of the tables' own rows.  For a batch of B triplets (u, p, n)
 * with rows U, P, Nn:   x_b = <U_b, Nn_b> - <U_b, P_b>,   bpr = mean_b softplus(x_b),   reg = 1/2 (|U|^2 + |P|^2 + |Nn|^2) / B,
 * loss = bpr + decay * reg.  With s_b = sigmoid(x_b) row u receives (s_b (Nn_b - P_b) + decay U_b) / B, row p
 * (-s_b U_b + decay P_b) / B and row n (s_b U_b + decay Nn_b) / B; repeated ids sum (2^50 fixed point: in any order, bit for
 * bit).  Adam is torch's dense one: EVERY row is updated every step, rows outside the batch with g = 0.
 * Two launches per step (k_mf_triplet, k_mf_adam), no host sync, no allocation; after a step G64 is all zero again.      */
typedef struct lgcn_mf lgcn_mf;   /* opaque */

typedef struct {
    int32_t n_users;
    int32_t m_items;            /* N = n_users + m_items < 2^31 */
    int32_t d;                  /* latent_dim_rec: 32/64/128/256 */
    /* parameters + Adam state, fp32 [N,d]: rows [0,n_users) = embedding_user.weight,
     * rows [n_users,N) = embedding_item.weight */
    float *E0;
    float *adam_m;
    float *adam_v;
    /* workspace, caller-allocated, zero-initialised before the first step */
    int64_t *G64;               /* [N,d] fixed-point (2^50) accumulator of the batch rows' gradient */
    uint32_t *bitmap;           /* [2*ceil(N/32)] rows of G64 that are non-zero (two, used alternately) */
    float *terms;               /* [2*max_batch] per-triplet loss / reg terms */
    int32_t *err;               /* [1] device error flag */
    int32_t max_batch;
    /* hyper-parameters (utils.py:47-51, torch.optim.Adam defaults) */
    float decay;                /* config['decay'] */
    double lr, beta1, beta2, eps;
} lgcn_mf_config;

/* rc 3 (nothing allocated): a null pointer, d outside {32, 64, 128, 256}, n_users or m_items < 1, N >= 2^31, max_batch < 1.
 * The context owns no device memory. */
int lgcn_mf_create(const lgcn_mf_config *cfg, lgcn_mf **out);
void lgcn_mf_destroy(lgcn_mf *mf);
/* optimizer step counter (torch Adam state['step']) for checkpoint/resume, and the learning rate of the next step */
int64_t lgcn_mf_get_step(const lgcn_mf *mf);
void lgcn_mf_set_step(lgcn_mf *mf, int64_t step);
void lgcn_mf_set_lr(lgcn_mf *mf, double lr);

/* One full stageOne on a batch of B triplets (device int32 ids): replaces PureMF.bpr_loss + backward + Adam.step.
 * loss_out[0..2] (device) = {bpr + decay*reg, bpr, reg}.  No host sync.  An id outside its table raises the device error
 * flag (lgcn_mf_check) and its triplet contributes nothing (zero terms, no gradient); the step still divides by B.
 * rc 3, with nothing launched and nothing written: a null pointer, B < 1, B > max_batch.                                  */
int lgcn_mf_train_step(lgcn_mf *mf, const int32_t *users, const int32_t *pos, const int32_t *neg,
                       int32_t B, float *loss_out, void *stream);

/* A whole epoch: the loop of main.py:223-225 over ceil(T/B) consecutive batches of the (already shuffled) device arrays,
 * the last one short.  loss_out: [3*ceil(T/B)].  Bit for bit the loop of lgcn_mf_train_step.  Same rc 3 cases.           */
int lgcn_mf_train_epoch(lgcn_mf *mf, const int32_t *users, const int32_t *pos, const int32_t *neg,
                        int64_t T, int32_t B, float *loss_out, void *stream);

/* reads and clears the device error flag (synchronises the stream): 0 = none,
 * 1 = id out of range in users/pos/neg.                                        */
int lgcn_mf_check(lgcn_mf *mf, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LGCN_HIP_H */

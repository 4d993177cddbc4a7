"""float64 restatement of the fused step with hard negatives, DNS(M, N) (--hard_neg M with --neg_ratio R; lgcn_ctx_set_hard_neg,
csrc/lgcn_hardneg.hip), and the cases its tests share.  Test infrastructure: tests/test_hard_neg_host.py pins it
(the exported hash, torch autograd of LightGCN.bpr_loss); tests/test_gpu_hard_neg.py uses the cases and the bound.

A sample is (u, p, n_1..n_R).  With e the rows of the output table (tests/multineg_restatement.py: propagate):
    s_r   = e_u.e_{n_r},  ranked descending, ties by r ascending (a stable sort)
    j_b   = H(seed, step, b) mod M          (rank below: lgcn_hn_rank of csrc/lgcn_internal.h in Python integers)
    sel_b = the candidate of rank j_b
and the step is multineg_restatement.step on the R = 1 batch (u_b, p_b, n_sel(b)): the BPR step, every slot of weight 1, divisor B.

THE SCORE BOUND (u = 2^-24, gamma_n = n u / (1 - n u)).  The kernel forms s_r as a d-term fp32 dot product (per-lane partial sums,
then a shuffle tree; multiply-add pairs may be contracted): whatever the order, |fl(s_r) - s_r| <= gamma_d sum_j |u_j| |n_rj| on the
fp32 rows it read; gamma_{d+2} is what the issue writes and is what is used.  The rows themselves are formed in the kernel from the
K + 1 stored tables (slot_row): the mean adds K values and divides once, the weighted form makes K + 1 products and K additions --
at most K + 2 roundings of partial sums no larger than T = sum_k |w_k X_k[row]|, so a row is delta_e = (K + 2) u T (with the mean's
1 / (K + 1) inside w_k) from the float64 combination of the same stored tables, the figure of tests/storage_cases.py, and the
score moves by at most sum_j (delta_u_j |n_rj| + |u_j| delta_n_rj) more.  Together, for sample b,
    bound_b = max_r ( gamma_{d+2} sum_j |u_j| |n_rj| + sum_j (delta_u_j |n_rj| + |u_j| delta_n_rj) ).
Every fp32 score is within bound_b of its float64 value; order statistics are 1-Lipschitz in the sup norm, so the j-th largest fp32
score is within bound_b of the j-th largest float64 score, and the fp32 score of the kernel's selection IS the j-th largest fp32
score: |s64[sel_b] - s64_sorted[j_b]| <= 2 bound_b for every sample, and where the gaps around the picked order statistic exceed
2 bound_b the choice itself is forced.  Nothing here is tuned."""
import numpy as np
import torch

import multineg_restatement as MN
import storage_cases as SC

MASK = (1 << 64) - 1
DOMAIN = 0x4841524E45473031
U = 2.0 ** -24
SEED = SC.DROP_SEED                       # world's default --seed: what model.LightGCN hands to lgcn_ctx_set_hard_neg


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def rank(seed, step, b, M):
    """j_b in Python integers.  step: the Adam step counter BEFORE the step (0 for the first step), as the dropout mask's key."""
    k = splitmix64((splitmix64(seed & MASK) + (step & MASK)) & MASK)
    v = splitmix64(((k ^ DOMAIN) + (b & 0xFFFFFFFF)) & MASK)
    return (v >> 32) % M if M > 1 else 0


def ranks(seed, step, B, M):
    return np.array([rank(seed, step, b, M) for b in range(B)], np.int64)


def scores(E, n_users, batch):
    """float64 s [B, R] of the candidates on an output table E (torch or numpy [N, d])."""
    E = torch.as_tensor(np.asarray(E, np.float64)) if not torch.is_tensor(E) else E.to(MN.F64)
    u, _, negs = (torch.from_numpy(np.asarray(t, np.int64)) for t in batch)
    return (E[u][:, None, :] * E[n_users + negs]).sum(2).numpy()


def select(s, j):
    """s [B, R], j [B] -> (sel [B], s sorted descending [B, R]): ties by r ascending."""
    order = np.argsort(-s, axis=1, kind="stable")
    return order[np.arange(len(j)), j], np.take_along_axis(s, order, axis=1)


def selected_batch(batch, sel):
    """(u, p, negs [B, R]), sel [B] -> the R = 1 batch (u, p, n_sel [B, 1]) of multineg_restatement.step."""
    u, p, negs = (np.asarray(t, np.int64) for t in batch)
    return u, p, negs[np.arange(len(u)), np.asarray(sel, np.int64)][:, None]


def step(A, n_users, K, decay, table, batch, sel, reg_ego=False, w=None, B_norm=None):
    """The step given the selection: multineg_restatement.step on the selected triplets."""
    return MN.step(A, n_users, K, decay, table, selected_batch(batch, sel), reg_ego, w, B_norm=B_norm)


def score_bound(tables, wk, n_users, batch, d):
    """bound_b [B] of the module docstring.  tables: the K + 1 float64 [N, d] tables X_0..X_K the rows are combined from (torch or
    numpy), wk: their K + 1 coefficients (the mean: 1 / (K + 1) each).  Also -> the float64 combination E [N, d]."""
    K = len(wk) - 1
    Xs = [np.asarray(t, np.float64) for t in tables]
    E = sum(float(wk[k]) * Xs[k] for k in range(K + 1))
    T = sum(abs(float(wk[k])) * np.abs(Xs[k]) for k in range(K + 1))
    dE = (K + 2) * U * T
    u, _, negs = (np.asarray(t, np.int64) for t in batch)
    au, an = np.abs(E[u])[:, None, :], np.abs(E[n_users + negs])
    du, dn = dE[u][:, None, :], dE[n_users + negs]
    n = d + 2
    gamma = n * U / (1.0 - n * U)
    return (gamma * (au * an).sum(2) + (du * an + au * dn).sum(2)).max(1), E


def float64_tables(A, table, K):
    """X_0..X_K in float64 (no storage rounding): what the host condition below is computed from."""
    X = torch.from_numpy(np.asarray(table, np.float64))
    out = [X.numpy()]
    for _ in range(K):
        X = A.to(MN.F64) @ X
        out.append(X.numpy())
    return out


def tight_share(s_sorted, j, bound):
    """Share of the samples whose picked order statistic lies within 2 bound_b of a neighbouring one."""
    B, R = s_sorted.shape
    rows = np.arange(B)
    gap = np.full(B, np.inf)
    up, dn = j > 0, j < R - 1
    gap[up] = np.minimum(gap[up], (s_sorted[rows, np.maximum(j - 1, 0)] - s_sorted[rows, j])[up])
    gap[dn] = np.minimum(gap[dn], (s_sorted[rows, j] - s_sorted[rows, np.minimum(j + 1, R - 1)])[dn])
    return float((gap < 2.0 * bound).mean())


# ---- cases -----------------------------------------------------------------------------------------------------------------
# (mode, d, K, R, M, reg_rows, feature): a covering subset of d 32..256 x K 1, 2 x R 2, 5, 16 x M 1, 2, R x fp32 / bf16 x reg_rows;
# d = 32 with R = 16 (18 id lanes of a 32-lane group) and d = 256 (four columns per lane) are in it; feature: None, ("drop", keep)
# (--dropout 1) or ("w", "exp") (--layer_weights exp).  Each case steps the batches of 64, 37 and 1 samples of its sequence.
CASES = [("fp32", 32, 1, 16, 1, "propagated", None), ("bf16", 32, 2, 16, 16, "ego", None),
         ("fp32", 64, 2, 5, 2, "propagated", None), ("bf16", 64, 1, 2, 2, "propagated", None),
         ("fp32", 128, 2, 5, 5, "ego", None), ("bf16", 128, 1, 16, 2, "propagated", None),
         ("fp32", 256, 1, 2, 1, "propagated", None), ("bf16", 256, 2, 5, 1, "ego", None),
         ("fp32", 64, 2, 5, 2, "propagated", ("drop", 0.6)), ("fp32", 64, 2, 5, 2, "propagated", ("w", "exp"))]
# Seed of a case's batches: 0 unless tests/test_hard_neg_host.py::test_the_reference_alone_discriminates fails there -- the
# condition involves the float64 table and the bound only, never the code under test (the device of storage_cases.BATCH_SEED)
BATCH_SEED = {}
TIGHT_SHARE = 0.05
# Batches of MN.LARGE_BATCH_SIZES = 65 and 300 samples (the loss reduction's second addition per lane, which no batch of CASES
# reaches), at R = 2 and R = 16 with M = 1 and M = R; K in {1, 3}, every width, both storages, both reg rows.  The same condition
# on the seed (tests/test_hard_neg_host.py::test_the_reference_alone_discriminates runs over both lists).
LARGE_CASES = [("fp32", 32, 1, 2, 1, "propagated", None), ("bf16", 64, 3, 16, 16, "ego", None),
               ("fp32", 128, 3, 2, 2, "propagated", None), ("bf16", 256, 1, 16, 1, "ego", None)]
assert not set(LARGE_CASES) & set(CASES) and {c[1] for c in LARGE_CASES} == set(MN.DS) and {c[2] for c in LARGE_CASES} == {1, 3}
assert {(c[3], c[4]) for c in LARGE_CASES} == {(R, M) for R in MN.LARGE_RS for M in (1, R)}
assert {c[0] for c in LARGE_CASES} == {"fp32", "bf16"} and {c[5] for c in LARGE_CASES} == {"propagated", "ego"}


def case_id(c):
    mode, d, K, R, M, reg, feat = c
    return f"{mode}-d{d}-K{K}-R{R}-M{M}" + ("-ego" if reg == "ego" else "") + ("" if feat is None else f"-{feat[0]}{feat[1]}")


def case_batches(c, seed=None):
    """The batches of 64, 37 and 1 samples of a case (multineg_restatement.make_batches: a user in several samples, the same item
    twice among one sample's candidates, the hub rows, the isolated item, the last table row, the hand-set rows)."""
    mode, d, K, R, M, reg, feat = c
    seed = BATCH_SEED.get(case_id(c), 0) if seed is None else seed
    if c in LARGE_CASES:                                                   # the batches of 65 and 300 samples
        return MN.make_batches(d, K, R, seed, sizes=MN.LARGE_BATCH_SIZES)
    seq = MN.make_batches(d, K, R, seed)
    return [seq[0], seq[2], seq[3]]

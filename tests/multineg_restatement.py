"""float64 restatement of the fused step on samples with several negatives per positive (--neg_ratio R; lgcn_train_step_multi,
csrc/lgcn_multineg.hip), and the batches its tests share.  Test infrastructure: tests/test_multineg_host.py pins
it (torch autograd, its own R = 1 run on the flattened batch, oracle.Trainer on the flattened batch); tests/test_gpu_multineg.py
uses the batches.

A batch is B samples (u_b, p_b, n_{b,1..R}).  With e the rows of the output table (mean of X_0 .. X_K, X_k = A X_{k-1}, or
sum_k w_k X_k):
    x_{b,r} = e_u.e_p - e_u.e_{n_r}
    bpr     = -1/(B R) sum_b sum_r logsigmoid(x_{b,r})
    reg     = 0.5/B sum_b (|e_u|^2 + |e_p|^2 + 1/R sum_r |e_{n_r}|^2)          (reg_ego: on the rows E0[.] of the table itself)
    loss    = bpr + decay reg
Gradient rows with gb_r = -sigmoid(-x_r) / (B R), lam = decay / B (0 in the rows with reg_ego):
    g_u = sum_r gb_r (e_p - e_{n_r}) + lam e_u,   g_p = (sum_r gb_r) e_u + lam e_p,   g_{n_r} = -gb_r e_u + lam/R e_{n_r}
reg_ego: the gradient of the L2 term goes to the table directly, decay/(B R) cnt[row] E0[row] with cnt = R per user / positive
slot and 1 per negative slot.  Backward: grad E0 = sum_k w_k A^k G (A symmetric; w_k = 1/(K+1) for the mean)."""
import numpy as np
import torch

import storage_cases as SC

F64 = torch.float64


def flatten(batch):
    """(u [B], p [B], negs [B, R]) -> the B R triplets (u_b, p_b, n_{b,r}), sample-major."""
    u, p, negs = (np.asarray(t, np.int64) for t in batch)
    R = negs.shape[1]
    return np.repeat(u, R), np.repeat(p, R), negs.reshape(-1)


def layer_weights(K, w=None):
    return [1.0 / (K + 1)] * (K + 1) if w is None else [float(np.float32(x)) for x in w]


def propagate(A, E0, K, w=None):
    wk = layer_weights(K, w)
    X, out = E0, wk[0] * E0
    for k in range(1, K + 1):
        X = A @ X
        out = out + wk[k] * X
    return out


def loss(E, E0, n_users, batch, decay, reg_ego=False):
    """The written loss on an output table E (autograd-capable) -> (loss, bpr, reg)."""
    u, p, negs = (torch.from_numpy(np.asarray(t, np.int64)) for t in batch)
    B, R = negs.shape
    eu, ep, en = E[u], E[n_users + p], E[n_users + negs]                     # [B, d], [B, d], [B, R, d]
    x = (eu * ep).sum(1)[:, None] - (eu[:, None, :] * en).sum(2)
    bpr = -torch.nn.functional.logsigmoid(x).sum() / float(B * R)
    if reg_ego:
        eu, ep, en = E0[u], E0[n_users + p], E0[n_users + negs]
    reg = 0.5 * ((eu * eu).sum() + (ep * ep).sum() + (en * en).sum() / float(R)) / float(B)
    return bpr + decay * reg, bpr, reg


def step(A, n_users, K, decay, table, batch, reg_ego=False, w=None, B_norm=None):
    """One step at the parameters `table` (numpy) in float64, by the formulas of the module docstring (no autograd) -> dict
    (B_norm: the batch size the step normalises by, where `batch` holds only the sound samples of a batch with voided ones):
    e_u, e_p [B, d], e_n [B, R, d], x [B, R], term, regterm [B] (what the kernel writes per sample), gb [B, R],
    g_u, g_p [B, d], g_n [B, R, d], G [N, d], cnt [N], g_final [N, d], loss_out (loss, bpr, reg)."""
    E0 = torch.from_numpy(np.asarray(table, np.float64))
    A = A.to(F64)
    u, p, negs = (torch.from_numpy(np.asarray(t, np.int64)) for t in batch)
    nb, R = negs.shape
    B = nb if B_norm is None else int(B_norm)
    N, d = E0.shape
    E = propagate(A, E0, K, w)
    eu, ep, en = E[u], E[n_users + p], E[n_users + negs]
    x = (eu * ep).sum(1)[:, None] - (eu[:, None, :] * en).sum(2)
    term = torch.nn.functional.logsigmoid(x).sum(1) / float(R)
    ru, rp, rn = (E0[u], E0[n_users + p], E0[n_users + negs]) if reg_ego else (eu, ep, en)
    regterm = (ru * ru).sum(1) + (rp * rp).sum(1) + (rn * rn).sum((1, 2)) / float(R)
    bpr = -term.sum() / float(B)
    reg = 0.5 * regterm.sum() / float(B)
    gb = -torch.sigmoid(-x) / float(B * R)
    lam = 0.0 if reg_ego else decay / float(B)
    g_u = (gb[:, :, None] * (ep[:, None, :] - en)).sum(1) + lam * eu
    g_p = gb.sum(1)[:, None] * eu + lam * ep
    g_n = -gb[:, :, None] * eu[:, None, :] + (lam / float(R)) * en
    G = torch.zeros(N, d, dtype=F64)
    G.index_add_(0, u, g_u)
    G.index_add_(0, n_users + p, g_p)
    G.index_add_(0, (n_users + negs).reshape(-1), g_n.reshape(-1, d))
    cnt = torch.zeros(N, dtype=F64)
    cnt.index_add_(0, u, torch.full((nb,), float(R), dtype=F64))
    cnt.index_add_(0, n_users + p, torch.full((nb,), float(R), dtype=F64))
    cnt.index_add_(0, (n_users + negs).reshape(-1), torch.ones(nb * R, dtype=F64))
    wk = layer_weights(K, w)
    h = wk[K] * G                                                            # Horner: h_{k-1} = w_{k-1} G + A h_k
    for k in range(K, 0, -1):
        h = wk[k - 1] * G + A @ h
    if reg_ego:
        h = h + (decay / float(B * R)) * cnt[:, None] * E0
    return dict(e_u=eu, e_p=ep, e_n=en, x=x, term=term, regterm=regterm, gb=gb, g_u=g_u, g_p=g_p, g_n=g_n, G=G, cnt=cnt,
                g_final=h, loss_out=(bpr + decay * reg, bpr, reg), E=E, E0=E0)


def adam(p, m, v, g, step_no, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's single-tensor step in float64 on numpy arrays -> (p', m', v')."""
    m2 = m + (1.0 - b1) * (g - m)
    v2 = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step_no, 1.0 - b2 ** step_no
    return p - (lr / bc1) * m2 / (np.sqrt(v2) / np.sqrt(bc2) + eps), m2, v2


# ---- cases -----------------------------------------------------------------------------------------------------------------
DS = (32, 64, 128, 256)
KS = (1, 2, 3)
RS = (2, 5, 16)
BATCH_SIZES = SC.BATCH_SIZES              # 64, 64, 37, 1
# Seed of a case's batches in the comparisons with the oracle: 0 unless the condition of
# tests/test_multineg_host.py::test_the_oracle_can_judge_at_its_yardstick fails there (the device of storage_cases.BATCH_SEED).
# The oracle is fp32: its reg term is a sequential sum of 3 d squares per triplet, and with reg_rows = ego at d >= 128 (reg about
# 0.015 d) the B = 1 step, where no averaging over samples helps, leaves it up to 3e-6 from float64 -- the whole yardstick.  A case
# whose oracle is further than HALF the yardstick (1.5e-6) from float64 on its own trajectory takes the first seed at which it is
# not; the condition involves the oracle and float64 only, never the code under test.
ORACLE_ROOM = 1.5e-6
BATCH_SEED = {(128, 3, 16, "ego"): 1, (256, 1, 5, "ego"): 1, (256, 1, 16, "ego"): 2, (256, 2, 2, "ego"): 2, (256, 2, 16, "ego"): 1,
              (256, 3, 2, "ego"): 1, (256, 3, 5, "ego"): 1, (256, 3, 16, "ego"): 9}


def case_batches(d, K, R, reg):
    """The batches of a case of the oracle comparisons (BATCH_SEED)."""
    return make_batches(d, K, R, BATCH_SEED.get((d, K, R, reg), 0))


# reduce_loss_wave adds terms[lane], terms[lane + 64], ..: with B <= 64 the per-sample terms of the multi-negative, softmax and
# hard-negative steps (scaled by inv_R, read with terms_stride) never take the second addition.  65: one lane takes it; 300: every
# lane takes four or five.  Both also leave a last 64-sample block that is not full.
LARGE_BATCH_SIZES = (65, 300)
LARGE_RS = (2, 16)
assert all(-(-B // 64) >= 2 for B in LARGE_BATCH_SIZES) and all(-(-B // 64) == 1 for B in BATCH_SIZES)


def make_batches(d, K, R, seed=0, sizes=BATCH_SIZES):
    """Batches of 64, 64, 37 and 1 samples (u [B], p [B], negs [B, R]) on the graph of tests/storage_cases.py (or of `sizes`
    samples).  Every batch sequence holds: a user in several samples, an item that is one sample's positive and another's
    negative, the same item twice among one sample's negatives, the isolated item and the last table row as negatives, the hub
    user and the hub item, the hand-set rows."""
    rng = np.random.Generator(np.random.PCG64(100000 * seed + 1000 * R + d + K))
    out = []
    for nb in sizes:
        u = rng.integers(1, SC.N_USERS, nb); p = rng.integers(1, SC.M_ITEMS, nb); n = rng.integers(1, SC.M_ITEMS, (nb, R))
        for a in (p, n):                                          # the big row propagates, no slot names it (no saturated sigmoid)
            a[(a == SC.BIG_ITEM) | (a == SC.ISOLATED_ITEM)] = 20
        if nb > 8:
            u[:4] = u[0]                                          # a user in several samples
            p[:6] = 21                                            # a row named by many slots
            n[6, 0] = p[6]                                        # pos = neg inside a sample
            n[7, R - 1] = p[8]                                    # the positive of one sample, a negative of another
            n[9, 0] = n[9, 1] = 33                                # the same item twice among one sample's negatives
            u[10] = SC.HUB_USER; p[11] = SC.HUB_ITEM; n[12, R // 2] = SC.HUB_ITEM
            n[13, 1] = SC.ISOLATED_ITEM                           # the isolated item as a negative
            n[14, R - 1] = SC.M_ITEMS - 1                         # the last table row as a negative
            u[15] = SC.ZERO_USER; u[16] = SC.TINY_USER; p[17] = SC.OUTLIER_ITEM; n[18, 0] = SC.SUBNORMAL_ITEM; u[19] = SC.N_USERS - 1
        else:
            n[0, R - 1] = SC.M_ITEMS - 1                          # B = 1: the last table row, and a repeated negative
            n[0, 0] = n[0, 1]
        out.append((u, p, n))
    return out

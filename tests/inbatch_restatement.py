"""float64 restatement of the fused step under the in-batch sampled softmax (--loss inbatch; lgcn_train_step_inbatch,
csrc/lgcn_inbatch.hip), in the manner of tests/softmax_restatement.py, whose propagate, adam and layer_weights
(tests/multineg_restatement.py) and graph (tests/storage_cases.py) it uses.  Test infrastructure: tests/test_inbatch_host.py
pins it (torch autograd of the loss written with torch.logsumexp and an explicit mask; the sampled softmax at B = 2);
tests/test_gpu_inbatch.py judges the device against it.

A batch is B samples (u_b, p_b), e the rows of the output table, tau > 0 the temperature:
    s_{b,c} = e_{u_b}.e_{p_c}
    A_b     = { c != b, p_c != p_b, u_c != u_b }                               (the competitors of sample b)
    z_{b,c} = (s_{b,c} - s_{b,b}) / tau,   l_b = log(1 + sum_{c in A_b} exp(z_{b,c})),   sm = 1/B sum_b l_b
    reg     = 0.5/B sum_b (|e_u|^2 + |e_p|^2)                                  (reg_ego: on the rows E0[.] of the table itself)
    loss    = sm + decay reg
Gradient rows with q_{b,c} = exp(z_{b,c}) / (1 + sum_j exp(z_{b,j})), Q_b = sum_c q_{b,c}, lam = decay / B (0 with reg_ego):
    W[b,c] = q_{b,c} / (tau B) (c in A_b),  W[b,b] = -Q_b / (tau B),  0 otherwise
    g_{u_b} = sum_c W[b,c] e_{p_c} + lam e_{u_b},   g_{p_c} = sum_b W[b,c] e_{u_b} + lam e_{p_c}
reg_ego, the backward chain and Adam are those of tests/multineg_restatement.py (two slots per sample, weight 1 each).  l and q
are evaluated with the maximum m = max(0, max_c z_c) subtracted, so any finite score is fine in float64 too."""
import numpy as np
import torch

import multineg_restatement as MN
import storage_cases as SC

F64 = torch.float64
propagate, adam, layer_weights = MN.propagate, MN.adam, MN.layer_weights


def as_samples(batch):
    """(u [B], p [B][, anything]) -> int64 arrays (u, p): the sampled negatives of a triplet batch are not used."""
    return np.asarray(batch[0], np.int64).reshape(-1), np.asarray(batch[1], np.int64).reshape(-1)


def competitors(u, p):
    """keep[b, c] = c in A_b, from the ids alone (torch bool [B, B])."""
    u, p = torch.as_tensor(u), torch.as_tensor(p)
    return (p[None, :] != p[:, None]) & (u[None, :] != u[:, None])           # (u_c != u_b leaves c = b out)


def loss(E, E0, n_users, batch, decay, tau, reg_ego=False):
    """The written loss on an output table E (autograd-capable), with torch.logsumexp over (0, z_c for c in A_b) and an explicit
    mask -> (loss, sm, reg)."""
    u, p = (torch.from_numpy(t) for t in as_samples(batch))
    B = len(u)
    eu, ep = E[u], E[n_users + p]
    s = eu @ ep.t()
    z = (s - torch.diagonal(s)[:, None]) / float(tau)
    z = torch.where(competitors(u, p), z, torch.full_like(z, float("-inf")))
    sm = torch.logsumexp(torch.cat([torch.zeros(B, 1, dtype=z.dtype), z], dim=1), dim=1).sum() / float(B)
    if reg_ego:
        eu, ep = E0[u], E0[n_users + p]
    reg = 0.5 * ((eu * eu).sum() + (ep * ep).sum()) / float(B)
    return sm + decay * reg, sm, reg


def step(A, n_users, K, decay, tau, table, batch, reg_ego=False, w=None, B_norm=None, A_bwd=None):
    """One step at the parameters `table` (numpy) in float64, by the formulas of the module docstring (no autograd) -> dict
    (B_norm: the batch size the step normalises by, where `batch` holds only the sound samples of a batch with voided ones;
    A_bwd: the matrix of the backward chain where A is not symmetric -- edge dropout: A = A_drop, A_bwd = A_drop^T):
    e_u, e_p [B, d], s, z, q, W [B, B] (z = -inf, q = 0 outside A_b; W with its diagonal), keep [B, B], m, lterm, Q [B],
    term (= -lterm: what the kernel writes), regterm [B], g_u, g_p [B, d], G [N, d], cnt [N], g_final [N, d],
    loss_out (loss, sm, reg), E, E0."""
    E0 = torch.from_numpy(np.asarray(table, np.float64))
    A = A.to(F64)
    u, p = (torch.from_numpy(t) for t in as_samples(batch))
    nb = len(u)
    B = nb if B_norm is None else int(B_norm)
    N, d = E0.shape
    E = propagate(A, E0, K, w)
    eu, ep = E[u], E[n_users + p]
    s = eu @ ep.t()
    keep = competitors(u, p)
    z = torch.where(keep, (s - torch.diagonal(s)[:, None]) / float(tau), torch.full_like(s, float("-inf")))
    m = torch.clamp(z.max(1).values, min=0.0)
    ez = torch.exp(z - m[:, None])                                           # every exponent <= 0; exp(-inf) = 0 outside A_b
    Z = torch.exp(-m) + ez.sum(1)
    # l = m + log1p(Z - 1): where m = 0 the 1 of Z is the positive's term and is never added, so a tiny l keeps its relative
    # accuracy in float64 too (log(1 + 4e-12) would be good to 3e-5 only); where m > 0 the sum holds a term that is exactly 1
    Zm1 = torch.where(m > 0, torch.exp(-m) + (ez.sum(1) - 1.0), ez.sum(1))
    lterm = torch.where(keep.any(1), m + torch.log1p(Zm1), torch.zeros_like(m))  # no competitor: exactly 0
    q = ez / Z[:, None]
    Q = q.sum(1)
    ru, rp = (E0[u], E0[n_users + p]) if reg_ego else (eu, ep)
    regterm = (ru * ru).sum(1) + (rp * rp).sum(1)
    sm = lterm.sum() / float(B)
    reg = 0.5 * regterm.sum() / float(B)
    W = q / (float(tau) * float(B))
    W = W - torch.diag(Q / (float(tau) * float(B)))
    lam = 0.0 if reg_ego else decay / float(B)
    g_u = W @ ep + lam * eu
    g_p = W.t() @ eu + lam * ep
    G = torch.zeros(N, d, dtype=F64)
    G.index_add_(0, u, g_u)
    G.index_add_(0, n_users + p, g_p)
    cnt = torch.zeros(N, dtype=F64)
    cnt.index_add_(0, u, torch.ones(nb, dtype=F64))
    cnt.index_add_(0, n_users + p, torch.ones(nb, dtype=F64))
    wk = layer_weights(K, w)
    h = wk[K] * G                                                            # Horner: h_{k-1} = w_{k-1} G + A h_k
    At = A if A_bwd is None else A_bwd.to(F64)
    for k in range(K, 0, -1):
        h = wk[k - 1] * G + At @ h
    if reg_ego:
        h = h + (decay / float(B)) * cnt[:, None] * E0
    return dict(e_u=eu, e_p=ep, s=s, z=z, keep=keep, m=m, q=q, Q=Q, W=W, lterm=lterm, term=-lterm, regterm=regterm, g_u=g_u,
                g_p=g_p, G=G, cnt=cnt, g_final=h, loss_out=(sm + decay * reg, sm, reg), E=E, E0=E0)


# ---- cases -----------------------------------------------------------------------------------------------------------------
# The sweep split of csrc/lgcn_inbatch.hip is LGCN_INBATCH_PART_TILES = 8 tiles of 32 rows: B = 260 is 9 tiles, two parts.
PART_ROWS = 256
SPLIT_B = 260
BATCH_SIZES = (1, 2, 31, 32, 33, 65, 100, SPLIT_B)
# The sizes at which code runs that no batch of BATCH_SIZES reaches: 513 is 17 tiles = THREE parts, the third one tile with one
# live row (the merge loop over the parts, the blockIdx.y extent and the per-part addressing beyond two parts); 2048 is the
# default --bpr_batch: 64 tiles, eight full parts.
MANY_PARTS_B = 513
LARGE_BATCH_SIZES = (MANY_PARTS_B, 2048)


def parts(B):
    """The part count of the sweep over a batch of B samples (lgcn_inbatch_parts)."""
    return (((B + 31) // 32) + 7) // 8


def last_part_rows(B):
    """The rows of the last part of the sweep: from PART_ROWS (parts - 1) to B - 1."""
    return np.arange(PART_ROWS * (parts(B) - 1), B)


def make_batch(B, seed=0):
    """One batch (u [B], p [B]) on the graph of tests/storage_cases.py: unmasked at B <= 2; from B = 31 on a user in several
    samples and a positive drawn twice inside the first tile, the hub rows, the hand-set rows and the last table rows; from
    B = 65 on the same user and the same positive also ACROSS two tiles; from B = 513 (three parts of the sweep) on the same user
    and the same positive also across PARTS: one sample in rows 0..255, one in the last part (row B - 1: at B = 513 the last part
    is that row alone), and one pair across parts 0 / 1.  (300 users: a batch of 100 repeats users by itself.)"""
    rng = np.random.Generator(np.random.PCG64(7000 * seed + B))
    u = rng.integers(20, SC.N_USERS, B); p = rng.integers(30, SC.M_ITEMS - 10, B)
    p[(p == SC.BIG_ITEM) | (p == SC.ISOLATED_ITEM)] = 40
    if B == 2:
        u[1] = u[0] - 1; p[1] = p[0] + 1                          # no mask: the B = 2 identity
    if B >= 31:
        u[1] = u[0]; u[3] = u[0]                                  # one user, three samples (one tile)
        p[5] = p[4]                                               # one positive, two samples (one tile)
        u[6] = SC.HUB_USER; p[7] = SC.HUB_ITEM; u[8] = SC.ZERO_USER; u[9] = SC.TINY_USER; p[10] = SC.OUTLIER_ITEM
        p[11] = SC.SUBNORMAL_ITEM; u[12] = SC.N_USERS - 1; p[13] = SC.M_ITEMS - 1; p[14] = SC.ISOLATED_ITEM
    if B >= 65:
        u[40] = u[2]; p[50] = p[15]                               # across tiles 0 / 1
        u[64] = u[16]; p[B - 1] = p[17]                           # across tiles 0 / 2 (.. the last)
    if B >= MANY_PARTS_B:
        u[B - 1] = u[18]                                          # across parts 0 / the last (the positive: p[B - 1] = p[17] above)
        u[300] = u[19]; p[400] = p[20]                            # across parts 0 / 1
    return u, p


def kept_share(u, p):
    """The smallest share of its B - 1 possible competitors that a sample of the batch keeps (300 users, 560 items: a large batch
    masks some pairs by itself)."""
    B = len(u)
    return float(competitors(u, p).sum(1).min()) / max(B - 1, 1)


def make_batches(B, steps=3, seed=0):
    """`steps` consecutive batches of B samples."""
    return [make_batch(B, seed * 100 + i) for i in range(steps)]


def one_user_batch(B, seed=0):
    """Every sample names the same user: no competitors at all."""
    u, p = make_batch(B, seed)
    return np.full_like(u, u[0]), p


def duplicated_positive_batch(B=8, seed=0):
    """Distinct users and positives, except that samples 2 and 5 share their positive."""
    rng = np.random.Generator(np.random.PCG64(99 + seed))
    u = 20 + rng.permutation(SC.N_USERS - 20)[:B]; p = 30 + rng.permutation(SC.M_ITEMS - 40)[:B]
    p[(p == SC.BIG_ITEM) | (p == SC.ISOLATED_ITEM)] = 29
    p[5] = p[2]
    return u.astype(np.int64), p.astype(np.int64)


# ---- the saturation batch ----------------------------------------------------------------------------------------------------
SAT_TAU, SAT_D, SAT_K = 0.05, 256, 1
# As in tests/softmax_restatement.py the storage table reaches the condition as it stands (the BIG_ITEM row is 2^6 times an
# N(0, 0.1) row): no scaling is needed.  The condition (some z > 100, some sample with all z < -100) is checked in float64 by
# tests/test_inbatch_host.py and never involves the code under test.


def saturation_batch(E, B=40):
    """B samples of distinct users and positives on an output table E (float64 [N, d]): BIG_ITEM is the positive of sample 2 and
    of no other; the users of samples 0 / 2 are the ones that score BIG_ITEM highest, those of samples 1 / 3 the ones that score
    it lowest.  So samples 0 and 3 meet a dominating (q one-hot) and sample 1 a dominated competitor (column 2), and sample 2 has
    all z << 0 (a tiny l)."""
    E = np.asarray(E, np.float64)
    s = E[:SC.N_USERS] @ E[SC.N_USERS + SC.BIG_ITEM]
    s[[SC.ZERO_USER, SC.TINY_USER]] = 0.0
    hi, lo = np.argsort(-s)[:2], np.argsort(s)[:2]
    rng = np.random.Generator(np.random.PCG64(4243))
    rest = np.setdiff1d(np.arange(20, SC.N_USERS), np.concatenate([hi, lo]))
    u = rest[rng.permutation(len(rest))[:B]].astype(np.int64)
    p = (30 + rng.permutation(SC.M_ITEMS - 40)[:B]).astype(np.int64)
    p[(p == SC.BIG_ITEM) | (p == SC.ISOLATED_ITEM)] = 29
    u[0], u[1], u[2], u[3] = hi[0], lo[0], hi[1], lo[1]
    p[2] = SC.BIG_ITEM
    return u, p


TINY_Z = 30.0


def tiny_l_batch(E, B=40):
    """(u, p, tau): the saturation batch at the temperature tau = s_{2,2} / TINY_Z.  Sample 2 (the user that scores BIG_ITEM high,
    BIG_ITEM its positive) then has every z near -30: l_2 = log(1 + sum exp z) is about 39 e^-30 = 4e-12 -- tiny, NOT zero, and a
    normal fp32 number, so that its relative accuracy can be judged (log1p of the sum that never had the 1 added).  The other
    samples' z are ordinary at this temperature, except column 2."""
    E = np.asarray(E, np.float64)
    u, p = saturation_batch(E, B)
    return u, p, float(E[u[2]] @ E[SC.N_USERS + p[2]]) / TINY_Z

"""float64 restatement of the fused step under the sampled-softmax loss (--loss softmax; lgcn_ctx_set_loss,
csrc/lgcn_multineg.hip), in the manner of tests/multineg_restatement.py, whose propagate, adam, make_batches and
graph (tests/storage_cases.py) it uses.  Test infrastructure: tests/test_softmax_host.py pins it (torch autograd, the BPR
restatement at R = 1 and tau = 1); tests/test_gpu_softmax.py judges the device against it.

A batch is B samples (u_b, p_b, n_{b,1..R}), e the rows of the output table, tau > 0 the temperature:
    x_{b,r} = e_u.e_p - e_u.e_{n_r},   z_{b,r} = -x_{b,r} / tau
    l_b     = log(1 + sum_r exp(z_{b,r}))
    sm      = 1/B sum_b l_b                                                    (one term per sample: 1/B, not 1/(B R))
    reg     = 0.5/B sum_b (|e_u|^2 + |e_p|^2 + 1/R sum_r |e_{n_r}|^2)          (reg_ego: on the rows E0[.] of the table itself)
    loss    = sm + decay reg
Gradient rows with q_{b,r} = exp(z_{b,r}) / (1 + sum_j exp(z_{b,j})), gb_r = -q_{b,r} / (tau B), lam = decay / B (0 with reg_ego):
    g_u = sum_r gb_r (e_p - e_{n_r}) + lam e_u,   g_p = (sum_r gb_r) e_u + lam e_p,   g_{n_r} = -gb_r e_u + lam/R e_{n_r}
reg_ego, the backward chain and Adam are those of tests/multineg_restatement.py.  l and q are evaluated with the maximum
m = max(0, max_r z_r) subtracted, so any finite score is fine in float64 too."""
import numpy as np
import torch

import multineg_restatement as MN
import storage_cases as SC

F64 = torch.float64
propagate, adam, make_batches, layer_weights = MN.propagate, MN.adam, MN.make_batches, MN.layer_weights


def as_samples(batch):
    """(u [B], p [B], negs [B] or [B, R]) -> int64 arrays with negs [B, R] (1-D negatives: R = 1)."""
    u, p, negs = (np.asarray(t, np.int64) for t in batch)
    return u, p, negs.reshape(len(u), -1)


def loss(E, E0, n_users, batch, decay, tau, reg_ego=False):
    """The written loss on an output table E (autograd-capable), with torch.logsumexp over (0, z_1..z_R) -> (loss, sm, reg)."""
    u, p, negs = (torch.from_numpy(t) for t in as_samples(batch))
    B, R = negs.shape
    eu, ep, en = E[u], E[n_users + p], E[n_users + negs]
    x = (eu * ep).sum(1)[:, None] - (eu[:, None, :] * en).sum(2)
    z = -x / float(tau)
    sm = torch.logsumexp(torch.cat([torch.zeros(B, 1, dtype=z.dtype), z], dim=1), dim=1).sum() / float(B)
    if reg_ego:
        eu, ep, en = E0[u], E0[n_users + p], E0[n_users + negs]
    reg = 0.5 * ((eu * eu).sum() + (ep * ep).sum() + (en * en).sum() / float(R)) / float(B)
    return sm + decay * reg, sm, reg


def step(A, n_users, K, decay, tau, table, batch, reg_ego=False, w=None, B_norm=None, A_bwd=None):
    """One step at the parameters `table` (numpy) in float64, by the formulas of the module docstring (no autograd) -> dict
    (B_norm: the batch size the step normalises by, where `batch` holds only the sound samples of a batch with voided ones;
    A_bwd: the matrix of the backward chain where A is not symmetric -- edge dropout: A = A_drop, A_bwd = A_drop^T):
    e_u, e_p [B, d], e_n [B, R, d], x, z, q, gb [B, R], m, lterm [B], term (= -lterm: what the kernel writes), regterm [B],
    g_u, g_p [B, d], g_n [B, R, d], G [N, d], cnt [N], g_final [N, d], loss_out (loss, sm, reg), E, E0."""
    E0 = torch.from_numpy(np.asarray(table, np.float64))
    A = A.to(F64)
    u, p, negs = (torch.from_numpy(t) for t in as_samples(batch))
    nb, R = negs.shape
    B = nb if B_norm is None else int(B_norm)
    N, d = E0.shape
    E = propagate(A, E0, K, w)
    eu, ep, en = E[u], E[n_users + p], E[n_users + negs]
    x = (eu * ep).sum(1)[:, None] - (eu[:, None, :] * en).sum(2)
    z = -x / float(tau)
    m = torch.clamp(z.max(1).values, min=0.0)
    ez = torch.exp(z - m[:, None])                                           # every exponent <= 0
    Z = torch.exp(-m) + ez.sum(1)
    lterm = m + torch.log(Z)
    q = ez / Z[:, None]
    ru, rp, rn = (E0[u], E0[n_users + p], E0[n_users + negs]) if reg_ego else (eu, ep, en)
    regterm = (ru * ru).sum(1) + (rp * rp).sum(1) + (rn * rn).sum((1, 2)) / float(R)
    sm = lterm.sum() / float(B)
    reg = 0.5 * regterm.sum() / float(B)
    gb = -q / (float(tau) * float(B))
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
    At = A if A_bwd is None else A_bwd.to(F64)
    for k in range(K, 0, -1):
        h = wk[k - 1] * G + At @ h
    if reg_ego:
        h = h + (decay / float(B * R)) * cnt[:, None] * E0
    return dict(e_u=eu, e_p=ep, e_n=en, x=x, z=z, m=m, q=q, lterm=lterm, term=-lterm, regterm=regterm, gb=gb, g_u=g_u, g_p=g_p,
                g_n=g_n, G=G, cnt=cnt, g_final=h, loss_out=(sm + decay * reg, sm, reg), E=E, E0=E0)


# ---- the saturation batch ----------------------------------------------------------------------------------------------------
SAT_TAU, SAT_D, SAT_K = 0.05, 256, 1
# The storage table reaches the condition as it stands (the BIG_ITEM row is 2^6 times an N(0, 0.1) row and K = 1 puts it into
# its neighbours' rows): no scaling of that row is needed -- the factor is 1.  The condition (some z > 100, some sample with all
# z < -100; fp32 expf overflows at 88.7) is checked in float64 by tests/test_softmax_host.py and never involves the code under test.


def saturation_batch(E, R=4):
    """8 samples on an output table E (float64 [N, d]): BIG_ITEM is a negative of samples 0 and 1 and the
    positive of samples 2 and 3 (with ordinary negatives); samples 4..7 are ordinary.  The users of samples 0 / 2 are the ones
    that score BIG_ITEM highest, those of samples 1 / 3 the ones that score it lowest (most negative), so that both signs of a
    saturated exponent occur on each side: chosen from E alone."""
    E = np.asarray(E, np.float64)
    s = E[:SC.N_USERS] @ E[SC.N_USERS + SC.BIG_ITEM]
    s[[SC.ZERO_USER, SC.TINY_USER]] = 0.0
    hi, lo = np.argsort(-s)[:2], np.argsort(s)[:2]
    rng = np.random.Generator(np.random.PCG64(4242))
    u = rng.integers(20, SC.N_USERS, 8); p = rng.integers(30, SC.M_ITEMS - 10, 8); n = rng.integers(30, SC.M_ITEMS - 10, (8, R))
    u[0], u[1], u[2], u[3] = hi[0], lo[0], hi[1], lo[1]
    n[0, 1] = SC.BIG_ITEM; n[1, R - 1] = SC.BIG_ITEM                          # dominating (u = hi) / dominated (u = lo) negative
    p[2] = SC.BIG_ITEM; p[3] = SC.BIG_ITEM                                    # all z << 0 (u = hi) / all z >> 0 (u = lo)
    return u, p, n

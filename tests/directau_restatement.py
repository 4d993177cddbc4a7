"""float64 restatement of the fused step under the alignment-and-uniformity loss (--loss directau; lgcn_train_step_directau,
csrc/lgcn_directau.hip), with the call shape of tests/inbatch_scores_restatement.py, whose unit (and, through
tests/inbatch_restatement.py, propagate, adam, layer_weights, as_samples) it uses.  Test infrastructure:
tests/test_directau_host.py pins it (torch float64 autograd of the loss written independently with F.normalize and torch.pdist);
tests/test_gpu_directau.py judges the device against it.

A batch is B samples (u_b, p_b), e the rows of the output table, e^ = e inv(e), inv(e) = 1 / |e| (0 for a row of norm 0),
x_b = e^_{u_b}, y_b = e^_{p_b}, gamma >= 0:
    align   = 1/B sum_b |x_b - y_b|^2
    k_{b,c} = exp(-2 |x_b - x_c|^2) for b != c BY POSITION,   Z_X = sum_{b<c} k_{b,c},   unif(X) = log(Z_X / (B (B - 1) / 2))
    au      = align + gamma (unif(X) + unif(Y)) / 2,   reg = 0.5/B sum_b (|e_u|^2 + |e_p|^2)   (reg_ego: on the rows E0[.])
    loss    = au + decay reg
With fewer than two samples in `batch` both unif are 0 and contribute no gradient.  `batch` holds the SOUND samples of a call;
B_norm is the call's B: the divisors B and B (B - 1) / 2 are the call's (void samples drop out of the pairs, not of the divisors).
Gradient rows, lam = decay / B (0 with reg_ego), W_X[b,c] = (2 gamma / Z_X) k_{b,c} (zero diagonal; symmetric):
    g_{x_b} = 2/B (x_b - y_b) + sum_c W_X[b,c] (x_c - x_b),   g_{y_b} = -2/B (x_b - y_b) + sum_c W_Y[b,c] (y_c - y_b)
    g_{u_b} = inv(e_{u_b}) (g_x - (g_x.x_b) x_b) + lam e_{u_b},   and its mirror for the item row
The per-sample term the kernel writes is -(|x_b - y_b|^2 + gamma (unif(X) + unif(Y)) / 2), for EVERY sample of the call (a void
one carries the constant alone), so that the reduction with 1 / B yields au."""
import numpy as np
import torch
import torch.nn.functional as Fn

import inbatch_restatement as IB
import inbatch_scores_restatement as IS

F64 = IB.F64
unit = IS.unit


def npairs(B):
    return 0.5 * float(B) * float(B - 1)


def loss(E, E0, n_users, batch, decay, gamma, reg_ego=False, B_norm=None):
    """The written loss on an output table E (autograd-capable; rows of non-zero norm), independently of step(): F.normalize and
    torch.pdist -> (loss, au, reg)."""
    u, p = (torch.from_numpy(t) for t in IB.as_samples(batch))
    nb = len(u)
    B = nb if B_norm is None else int(B_norm)
    eu, ep = E[u], E[n_users + p]
    x, y = Fn.normalize(eu, dim=1, eps=0.0), Fn.normalize(ep, dim=1, eps=0.0)
    au = (x - y).pow(2).sum() / float(B)
    if nb >= 2:
        for t in (x, y):
            au = au + 0.5 * float(gamma) * torch.log(torch.exp(-2.0 * torch.pdist(t, p=2).pow(2)).sum() / npairs(B))
    if reg_ego:
        eu, ep = E0[u], E0[n_users + p]
    reg = 0.5 * ((eu * eu).sum() + (ep * ep).sum()) / float(B)
    return au + decay * reg, au, reg


def side(x, gamma, B):
    """One side of the uniformity term on unit rows x [nb, d] -> (k [nb, nb] with a zero diagonal, Z, unif, W)."""
    nb = len(x)
    if nb < 2:
        z = torch.zeros(nb, nb, dtype=F64)
        return z, torch.zeros((), dtype=F64), torch.zeros((), dtype=F64), z
    # (in blocks of rows: the same operations on the same operands, element for element, without a [nb, nb, d] array at nb = 2048)
    d2 = torch.cat([((x[i:i + 64, None, :] - x[None, :, :]) ** 2).sum(2) for i in range(0, nb, 64)], dim=0)
    k = torch.exp(-2.0 * d2) * (1.0 - torch.eye(nb, dtype=F64))
    Z = torch.triu(k, 1).sum()
    return k, Z, torch.log(Z / npairs(B)), (2.0 * float(gamma) / Z) * k


def step(A, n_users, K, decay, gamma, table, batch, reg_ego=False, w=None, B_norm=None, A_bwd=None):
    """One step at the parameters `table` (numpy) in float64, by the formulas of the module docstring (no autograd) -> dict:
    e_u, e_p (the RAW rows), x, y, inv_u, inv_p, al [nb], k_x, k_y, W_x, W_y [nb, nb], Z_x, Z_y, unif_x, unif_y, cst (gamma (unif(X) +
    unif(Y)) / 2), term [nb] (what the kernel writes for a sound sample), regterm [nb], ga_u, ga_p (the alignment part of the
    gradient rows), gu_u, gu_p (the uniformity part), t_x, t_y, g_u, g_p (with lam e), G [N, d], cnt [N], g_final [N, d],
    loss_out (loss, au, reg), E, E0."""
    E0 = torch.from_numpy(np.asarray(table, np.float64))
    A = A.to(F64)
    u, p = (torch.from_numpy(t) for t in IB.as_samples(batch))
    nb = len(u)
    B = nb if B_norm is None else int(B_norm)
    N, d = E0.shape
    E = IB.propagate(A, E0, K, w)
    eu, ep = E[u], E[n_users + p]
    (x, inv_u), (y, inv_p) = unit(eu), unit(ep)
    al = ((x - y) ** 2).sum(1)
    k_x, Z_x, unif_x, W_x = side(x, gamma, B)
    k_y, Z_y, unif_y, W_y = side(y, gamma, B)
    cst = 0.5 * float(gamma) * (unif_x + unif_y)
    lam = 0.0 if reg_ego else decay / float(B)

    def project(g, own, inv):
        return inv[:, None] * (g - (g * own).sum(1)[:, None] * own)
    ga_x = (2.0 / float(B)) * (x - y)
    gu_x = W_x @ x - W_x.sum(1)[:, None] * x
    gu_y = W_y @ y - W_y.sum(1)[:, None] * y
    ga_u, ga_p = project(ga_x, x, inv_u), project(-ga_x, y, inv_p)
    gu_u, gu_p = project(gu_x, x, inv_u), project(gu_y, y, inv_p)
    g_u = ga_u + gu_u + lam * eu
    g_p = ga_p + gu_p + lam * ep
    ru, rp = (E0[u], E0[n_users + p]) if reg_ego else (eu, ep)
    regterm = (ru * ru).sum(1) + (rp * rp).sum(1)
    au = al.sum() / float(B) + cst
    reg = 0.5 * regterm.sum() / float(B)
    G = torch.zeros(N, d, dtype=F64)
    G.index_add_(0, u, g_u)
    G.index_add_(0, n_users + p, g_p)
    cnt = torch.zeros(N, dtype=F64)
    cnt.index_add_(0, u, torch.ones(nb, dtype=F64))
    cnt.index_add_(0, n_users + p, torch.ones(nb, dtype=F64))
    wk = IB.layer_weights(K, w)
    h = wk[K] * G                                                            # Horner: h_{k-1} = w_{k-1} G + A h_k
    At = A if A_bwd is None else A_bwd.to(F64)
    for k in range(K, 0, -1):
        h = wk[k - 1] * G + At @ h
    if reg_ego:
        h = h + (decay / float(B)) * cnt[:, None] * E0
    return dict(e_u=eu, e_p=ep, x=x, y=y, inv_u=inv_u, inv_p=inv_p, al=al, k_x=k_x, k_y=k_y, W_x=W_x, W_y=W_y, Z_x=Z_x, Z_y=Z_y,
                unif_x=unif_x, unif_y=unif_y, cst=cst, term=-(al + cst), regterm=regterm, ga_u=ga_u, ga_p=ga_p, gu_u=gu_u, gu_p=gu_p,
                t_x=(W_x * (x @ x.t())).sum(1), t_y=(W_y * (y @ y.t())).sum(1), g_u=g_u, g_p=g_p, G=G, cnt=cnt, g_final=h,
                loss_out=(au + decay * reg, au, reg), E=E, E0=E0)


# ---- cases -----------------------------------------------------------------------------------------------------------------
import storage_cases as SC  # noqa: E402


def make_batch(B, seed=0):
    """One batch (u [B], p [B]) on the graph of tests/storage_cases.py, on rows of ordinary norm only (the hand-set zero, tiny,
    subnormal and outlier rows of the storage table are left out: the loss normalises every row).  From B = 7 on a repeated user,
    a repeated item and a sample that is another's mirror in position (same user AND same item: a pair of distance 0 on both
    sides); from B = 65 on the same user and item also across tiles; from B = 513 (three parts of the sweep) on the same user and
    the same item also across PARTS: rows 0..255 / the last part (row B - 1), rows 0..255 / part 1, and a mirror across parts."""
    rng = np.random.Generator(np.random.PCG64(9100 * seed + B))
    special_u = {SC.ZERO_USER, SC.TINY_USER}
    special_p = {SC.BIG_ITEM, SC.ISOLATED_ITEM, SC.OUTLIER_ITEM, SC.SUBNORMAL_ITEM}
    us = np.array([i for i in range(20, SC.N_USERS) if i not in special_u])
    ps = np.array([i for i in range(30, SC.M_ITEMS - 10) if i not in special_p])
    u = us[rng.integers(0, len(us), B)]; p = ps[rng.integers(0, len(ps), B)]
    if B == 2:
        u[1] = u[0] - 1 if u[0] > 20 else u[0] + 1               # two users: one pair of non-zero distance
    if B >= 7:
        u[1] = u[0]                                                # a repeated user
        p[3] = p[2]                                                # a repeated item
        u[5], p[5] = u[4], p[4]                                    # a mirror: zero distance on both sides
        u[6] = SC.HUB_USER
    if B >= 33:
        p[7] = SC.HUB_ITEM; u[12] = SC.N_USERS - 1; p[13] = SC.M_ITEMS - 1
        u[B - 1] = u[2]                                            # across tiles 0 / the last
    if B >= 65:
        u[40] = u[8]; p[50] = p[15]                                # across tiles 0 / 1
    if B >= IB.MANY_PARTS_B:
        p[B - 1] = p[9]                                            # across parts 0 / the last (the user: u[B - 1] = u[2] above)
        u[300] = u[10]; p[400] = p[11]                             # across parts 0 / 1
        u[500], p[500] = u[14], p[14]                              # a mirror across parts 0 / 1
    return u.astype(np.int64), p.astype(np.int64)


# The sizes at which code runs that no smaller batch reaches (csrc/lgcn_directau.hip): k_directau_merge adds n = tiles * parts
# partials per side, lane-strided over 64 lanes -- a lane adds a SECOND partial only from n > 64, which 22 tiles x 3 parts = 66
# are the first to reach.  705 is 23 tiles x 3 parts = 69 with one live row in the last tile; 736 is the same count with full
# tiles; 2048 is the default --bpr_batch (64 x 8 = 512 partials, eight per lane).
MERGE_B = 705
LARGE_BATCH_SIZES = (MERGE_B, 736, 2048)


def partials(B):
    """The partials per side that k_directau_merge adds: tiles x parts."""
    return ((B + 31) // 32) * IB.parts(B)


def skipped_parts(B):
    """The (owner tile, part) workgroups of the symmetric sweep whose whole part lies below the owner tile (ts = max(t0, bx) >= t1)
    although the part is neither the first nor the last one: a hole in the middle of the sweep."""
    nT, NP = (B + 31) // 32, IB.parts(B)
    return [(bx, by) for bx in range(nT) for by in range(1, NP - 1) if max(by * 8, bx) >= min(by * 8 + 8, nT)]


def make_batches(B, steps=3, seed=0):
    return [make_batch(B, seed * 100 + i) for i in range(steps)]

"""float64 restatement of the in-batch step with mixed negative sampling (--inbatch_mix 1; DESIGN 4.21;
lgcn_train_step_inbatch_mix, csrc/lgcn_inbatch.hip), built on tests/inbatch_scores_restatement.py (imported, not edited), whose
unit rows, competitors, propagate and backward chain it uses.  Test infrastructure: tests/test_inbatch_mix_host.py pins it
(array-equal to inbatch_scores_restatement.step with no pool; the sampled softmax at B = 1; torch autograd of the written loss);
tests/test_gpu_inbatch_mix.py judges the device against it.

A batch is B samples (u_b, p_b, n_{b,1..R}).  Everything not restated is inbatch_scores_restatement's.  The columns of sample
b's score row are the in-batch columns c in A_b and the pool columns (c, r) of ALL samples c (here: column B + r B + c):
    N_b         = { (c, r) : n_{c,r} != p_b }
    s_{b,(c,r)} = e^_{u_b}.e^_{n_{c,r}}
    z_{b,(c,r)} = (s_{b,(c,r)} - s_{b,b}) / tau - (lq_{n_{c,r}} - lq_{p_b})
    l_b = log(1 + sum_{A_b} exp z + sum_{N_b} exp z),  q, Q_b over both kinds of column,  W[b,.] = q / (tau B),  W[b,b] = -Q_b / (tau B)
    g_{u_b} += sum_{(c,r)} W[b,(c,r)] e^_{n_{c,r}},   g_{n_{c,r}} = sum_b W[b,(c,r)] e^_{u_b} + lam/R e_{n_{c,r}}
    cosine: every row through its own normalisation, t_{u_b} over both kinds of column, a pool row with its own t and inv
    reg = 0.5/B sum_b ( |e_u|^2 + |e_p|^2 + 1/R sum_r |e_{n_{b,r}}|^2 );  reg_ego: cnt = R per user / positive slot, 1 per negative
    slot, and the last link adds decay / (B R) cnt E0                               (the convention of tests/softmax_restatement.py)
With no pool (negs None, or R = 0) every operation below is inbatch_scores_restatement.step's on the same operands in the same
order: the results are array-equal, which tests/test_inbatch_mix_host.py asserts."""
import numpy as np
import torch
import torch.nn.functional as Fn

import inbatch_restatement as IB
import inbatch_scores_restatement as IS
import storage_cases as SC

F64 = IB.F64


def as_samples(batch):
    """(u [B], p [B][, negs [B] or [B, R] or None]) -> int64 arrays (u, p, negs [B, R]); R = 0 without negatives."""
    u, p = IB.as_samples(batch)
    negs = batch[2] if len(batch) > 2 else None
    negs = np.zeros((len(u), 0), np.int64) if negs is None else np.asarray(negs, np.int64).reshape(len(u), -1)
    return u, p, negs


def pool_ids(negs):
    """negs [B, R] -> the pool's item ids in column order r B + c."""
    return np.ascontiguousarray(np.asarray(negs, np.int64).T).reshape(-1)


def item_logq_mix(items_D, B, R):
    """What Python hands the library under --inbatch_logq 1 with mixing on: the log of the expected number of times item i stands
    among a sample's competitors, (B - 1) deg_i / sum deg + B R / m_items, in float64, rounded once to fp32."""
    deg = np.asarray(items_D, np.float64)
    return np.log((B - 1) * deg / deg.sum() + float(B) * R / len(deg)).astype(np.float32)


def keep_mask(u, p, n):
    """keep[b, j] over the B in-batch columns and the pool columns n (torch bool [B, B + len(n)])."""
    u, p, n = torch.as_tensor(u), torch.as_tensor(p), torch.as_tensor(n)
    return torch.cat([IB.competitors(u, p), n[None, :] != p[:, None]], dim=1)


def loss(E, E0, n_users, batch, decay, tau, reg_ego=False, score="dot", logq=None, B_norm=None):
    """The written loss on an output table E (autograd-capable; rows of non-zero norm under cosine), with torch.logsumexp over the
    masked [B, 1 + B + B R] logits -> (loss, sm, reg).  B_norm: see step."""
    cosine = IS._check(score)
    u, p, negs = as_samples(batch)
    R = negs.shape[1]
    u, p, n = torch.from_numpy(u), torch.from_numpy(p), torch.from_numpy(pool_ids(negs))
    nb = len(u)
    B = nb if B_norm is None else int(B_norm)
    eu, ep, en = E[u], E[n_users + p], E[n_users + n]
    items = torch.cat([ep, en], dim=0)
    s = Fn.normalize(eu, dim=1, eps=0.0) @ Fn.normalize(items, dim=1, eps=0.0).t() if cosine else eu @ items.t()
    z = (s - torch.diagonal(s[:, :nb])[:, None]) / float(tau)
    if logq is not None:
        lq = torch.from_numpy(np.asarray(logq, np.float64))
        z = z - (torch.cat([lq[p], lq[n]])[None, :] - lq[p][:, None])
    z = torch.where(keep_mask(u, p, n), z, torch.full_like(z, float("-inf")))
    sm = torch.logsumexp(torch.cat([torch.zeros(nb, 1, dtype=z.dtype), z], dim=1), dim=1).sum() / float(B)
    if reg_ego:
        eu, ep, en = E0[u], E0[n_users + p], E0[n_users + n]
    reg = (eu * eu).sum() + (ep * ep).sum()
    if R:
        reg = reg + (en * en).sum() / float(R)
    reg = 0.5 * reg / float(B)
    return sm + decay * reg, sm, reg


def rows(eu, ep, en, u, p, n, tau, B, score="dot", lqb=None, lqn=None, lam=0.0, lam_n=0.0):
    """The batch-row part of a step on the output rows eu, ep [nb, d] and the pool's rows en [P, d] (float64 tensors), normalised by
    B -> dict: inbatch_scores_restatement.rows' keys with s, z, keep, q, W over the nb + P columns (the in-batch block first), and
    eh_n, inv_n, t_n, gs_n, g_n for the pool."""
    cosine = IS._check(score)
    nb = len(eu)
    if cosine:
        (ehu, inv_u), (ehp, inv_p), (ehn, inv_n) = IS.unit(eu), IS.unit(ep), IS.unit(en)
    else:
        ehu, ehp, ehn = eu, ep, en
        inv_u, inv_p, inv_n = torch.ones(nb, dtype=F64), torch.ones(len(ep), dtype=F64), torch.ones(len(en), dtype=F64)
    ehi = torch.cat([ehp, ehn], dim=0)
    s = ehu @ ehi.t()
    keep = keep_mask(u, p, n)
    zz = (s - torch.diagonal(s[:, :nb])[:, None]) / float(tau)
    if lqb is not None:
        zz = zz - (torch.cat([lqb, lqn])[None, :] - lqb[:, None])
    z = torch.where(keep, zz, torch.full_like(s, float("-inf")))
    m = torch.clamp(z.max(1).values, min=0.0)
    ez = torch.exp(z - m[:, None])
    Z = torch.exp(-m) + ez.sum(1)
    Zm1 = torch.where(m > 0, torch.exp(-m) + (ez.sum(1) - 1.0), ez.sum(1))
    lterm = torch.where(keep.any(1), m + torch.log1p(Zm1), torch.zeros_like(m))
    q = ez / Z[:, None]
    Q = q.sum(1)
    W = q / (float(tau) * float(B))
    W = W - torch.cat([torch.diag(Q / (float(tau) * float(B))), torch.zeros(nb, len(en), dtype=F64)], dim=1)
    Wp, Wn = W[:, :nb], W[:, nb:]
    if cosine:
        t_u, t_i = (W * s).sum(1), (W * s).sum(0)
        t_p, t_n = t_i[:nb], t_i[nb:]
        gs_u = inv_u[:, None] * (W @ ehi - t_u[:, None] * ehu)
        gs_p = inv_p[:, None] * (Wp.t() @ ehu - t_p[:, None] * ehp)
        gs_n = inv_n[:, None] * (Wn.t() @ ehu - t_n[:, None] * ehn)
        g_u = gs_u + lam * eu
        g_p = gs_p + lam * ep
        g_n = gs_n + lam_n * en
    else:
        t_u, t_p, t_n = torch.zeros(nb, dtype=F64), torch.zeros(len(ep), dtype=F64), torch.zeros(len(en), dtype=F64)
        items = torch.cat([ep, en], dim=0)
        gs_u, gs_p, gs_n = W @ items, Wp.t() @ eu, Wn.t() @ eu
        g_u = W @ items + lam * eu
        g_p = Wp.t() @ eu + lam * ep
        g_n = Wn.t() @ eu + lam_n * en
    return dict(eh_u=ehu, eh_p=ehp, eh_n=ehn, inv_u=inv_u, inv_p=inv_p, inv_n=inv_n, s=s, z=z, keep=keep, m=m, q=q, Q=Q, W=W, lterm=lterm,
                term=-lterm, t_u=t_u, t_p=t_p, t_n=t_n, gs_u=gs_u, gs_p=gs_p, gs_n=gs_n, g_u=g_u, g_p=g_p, g_n=g_n)


def step(A, n_users, K, decay, tau, table, batch, reg_ego=False, w=None, B_norm=None, A_bwd=None, score="dot", logq=None):
    """inbatch_scores_restatement.step on (u, p, negs) -> its dict, s / z / keep / q / W over the B + B R columns, and the pool's
    n [P] (item ids, column order r B + c), e_n, eh_n, inv_n, lq_n, t_n, gs_n, g_n.  `batch` holds the sound samples only."""
    E0 = torch.from_numpy(np.asarray(table, np.float64))
    A = A.to(F64)
    u, p, negs = as_samples(batch)
    R = negs.shape[1]
    u, p, n = torch.from_numpy(u), torch.from_numpy(p), torch.from_numpy(pool_ids(negs))
    nb = len(u)
    B = nb if B_norm is None else int(B_norm)
    N, d = E0.shape
    E = IB.propagate(A, E0, K, w)
    eu, ep, en = E[u], E[n_users + p], E[n_users + n]
    lqv = None if logq is None else torch.from_numpy(np.asarray(logq, np.float64))
    lqb, lqn = (None, None) if lqv is None else (lqv[p], lqv[n])
    lam = 0.0 if reg_ego else decay / float(B)
    lam_n = lam / float(R) if R else 0.0
    r = rows(eu, ep, en, u, p, n, tau, B, score, lqb, lqn, lam, lam_n)
    ru, rp, rn = (E0[u], E0[n_users + p], E0[n_users + n]) if reg_ego else (eu, ep, en)
    regterm = (ru * ru).sum(1) + (rp * rp).sum(1)
    if R:
        regterm = regterm + (rn * rn).sum(1).reshape(R, nb).sum(0) / float(R)
    sm = r["lterm"].sum() / float(B)
    reg = 0.5 * regterm.sum() / float(B)
    G = torch.zeros(N, d, dtype=F64)
    G.index_add_(0, u, r["g_u"])
    G.index_add_(0, n_users + p, r["g_p"])
    G.index_add_(0, n_users + n, r["g_n"])
    slot = float(R) if R else 1.0                                            # a negative slot weighs 1 / R of a user / positive slot
    cnt = torch.zeros(N, dtype=F64)
    cnt.index_add_(0, u, torch.full((nb,), slot, dtype=F64))
    cnt.index_add_(0, n_users + p, torch.full((nb,), slot, dtype=F64))
    cnt.index_add_(0, n_users + n, torch.ones(len(n), dtype=F64))
    wk = IB.layer_weights(K, w)
    h = wk[K] * G                                                            # Horner: h_{k-1} = w_{k-1} G + A h_k
    At = A if A_bwd is None else A_bwd.to(F64)
    for k in range(K, 0, -1):
        h = wk[k - 1] * G + At @ h
    if reg_ego:
        h = h + (decay / float(B * R if R else B)) * cnt[:, None] * E0
    r.update(e_u=eu, e_p=ep, e_n=en, n=n, R=R, lq=torch.zeros(nb, dtype=F64) if lqb is None else lqb,
             lq_n=torch.zeros(len(n), dtype=F64) if lqn is None else lqn, regterm=regterm, G=G, cnt=cnt, g_final=h,
             loss_out=(sm + decay * reg, sm, reg), E=E, E0=E0)
    return r


# ---- cases -----------------------------------------------------------------------------------------------------------------
def make_batch(B, R, seed=0, plain=False):
    """One batch (u [B], p [B], negs [B, R]) on the graph of tests/storage_cases.py: (u, p) is inbatch_restatement.make_batch's,
    the negatives are uniform; unless `plain`: a duplicate pool id inside one sample (R >= 2) and across samples (B >= 3), the
    hub / hand-set item rows in the pool (B >= 31), and (B R >= 2) negs[1 % B, R - 1] = p_0 -- a pool id that is masked for sample 0
    and, being another sample's positive, stands twice among the columns of every other sample; from B = 513 on (three parts of
    the user sweep; (u, p) then repeat a user and a positive across parts) a positive of rows 0..255 as a negative of the last
    part, and a pool id twice across parts 0 / 1."""
    u, p = IB.make_batch(B, seed)
    rng = np.random.Generator(np.random.PCG64(9000 * seed + 16 * B + R))
    negs = rng.integers(30, SC.M_ITEMS - 10, (B, R))
    negs[(negs == SC.BIG_ITEM) | (negs == SC.ISOLATED_ITEM)] = 41
    if plain:
        negs[negs == p[:, None]] = 42
        assert not (negs == p[:, None]).any()
        return u, p, negs
    if R >= 2:
        negs[0, 1] = negs[0, 0]
    if B >= 3:
        negs[2, 0] = negs[0, 0]
    if B >= 31:
        negs[3, 0] = SC.HUB_ITEM; negs[4, R - 1] = SC.OUTLIER_ITEM; negs[5, 0] = SC.SUBNORMAL_ITEM; negs[6, R - 1] = SC.M_ITEMS - 1
    if B * R >= 2:                                                          # (never the only pool id: the pool would be empty)
        negs[1 % B, R - 1] = p[0]
    if B >= IB.MANY_PARTS_B:                                                # the pool across the PARTS of the user sweep (a pool row
        negs[B - 1, 0] = p[21]                                              #   sweeps the users): a positive of part 0 as a negative of
        negs[300, R - 1] = negs[8, 0]                                       #   the last part; a duplicate across parts 0 / 1
    return u, p, negs


def make_batches(B, R, steps=3, seed=0):
    return [make_batch(B, R, seed * 100 + i) for i in range(steps)]

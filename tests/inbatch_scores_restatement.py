"""float64 restatement of the in-batch step with its two score options (--score cosine, --inbatch_logq 1; DESIGN 4.20;
lgcn_ctx_set_inbatch_scores, csrc/lgcn_inbatch.hip), built on tests/inbatch_restatement.py (imported, not edited), whose
propagate, competitors, batches and backward chain it uses.  Test infrastructure: tests/test_inbatch_scores_host.py pins it
(array-equal to inbatch_restatement.step with both options off; torch autograd of the written loss with F.normalize and the lq
difference for the three new combinations); tests/test_gpu_inbatch_scores.py judges the device against it.

Everything not restated here is inbatch_restatement's (A_b, lam, the reg term on the RAW rows, reg_ego, B_norm, A_bwd):
    dot:     e^ = e
    cosine:  e^ = e inv(e),  inv(e) = 1 / |e| if |e| > 0 else 0
    s_{b,c} = e^_{u_b}.e^_{p_c}
    z_{b,c} = (s_{b,c} - s_{b,b}) / tau - (lq_{p_c} - lq_{p_b})        (lq: one value per item, None = 0)
    l, sm, q, Q, W from this z, as before
    cosine:  t_u[b] = sum_c W[b,c] s_{b,c},  t_p[c] = sum_b W[b,c] s_{b,c}                  (c, b over A and the diagonal)
             g_{u_b} = inv(e_{u_b}) (sum_c W[b,c] e^_{p_c} - t_u[b] e^_{u_b}) + lam e_{u_b}
             g_{p_c} = inv(e_{p_c}) (sum_b W[b,c] e^_{u_b} - t_p[c] e^_{p_c}) + lam e_{p_c}
With score = 'dot' and logq = None every operation below is inbatch_restatement.step's, in its order: the results are
array-equal, which tests/test_inbatch_scores_host.py asserts."""
import numpy as np
import torch
import torch.nn.functional as Fn

import inbatch_restatement as IB

F64 = IB.F64
SCORES = ("dot", "cosine")
# the three new combinations (score, logq on?)
NEW_OPTIONS = (("cosine", False), ("dot", True), ("cosine", True))


def item_logq(items_D):
    """What Python hands the library: log of the train degree in float64, rounded once to fp32 (numpy [m_items])."""
    return np.log(np.asarray(items_D, np.float64)).astype(np.float32)


def unit(e):
    """rows e [n, d] -> (e^, inv): inv = 1 / |e| (0 for a row of norm 0)."""
    n = torch.sqrt((e * e).sum(1))
    inv = torch.where(n > 0, 1.0 / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n))
    return e * inv[:, None], inv


def _check(score):
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    return score == "cosine"


def loss(E, E0, n_users, batch, decay, tau, reg_ego=False, score="dot", logq=None):
    """The written loss on an output table E (autograd-capable; rows of non-zero norm under cosine, where e^ is F.normalize),
    with torch.logsumexp over (0, z_c for c in A_b) and an explicit mask -> (loss, sm, reg)."""
    cosine = _check(score)
    u, p = (torch.from_numpy(t) for t in IB.as_samples(batch))
    B = len(u)
    eu, ep = E[u], E[n_users + p]
    s = Fn.normalize(eu, dim=1, eps=0.0) @ Fn.normalize(ep, dim=1, eps=0.0).t() if cosine else eu @ ep.t()
    z = (s - torch.diagonal(s)[:, None]) / float(tau)
    if logq is not None:
        lq = torch.from_numpy(np.asarray(logq, np.float64))[p]
        z = z - (lq[None, :] - lq[:, None])
    z = torch.where(IB.competitors(u, p), z, torch.full_like(z, float("-inf")))
    sm = torch.logsumexp(torch.cat([torch.zeros(B, 1, dtype=z.dtype), z], dim=1), dim=1).sum() / float(B)
    if reg_ego:
        eu, ep = E0[u], E0[n_users + p]
    reg = 0.5 * ((eu * eu).sum() + (ep * ep).sum()) / float(B)
    return sm + decay * reg, sm, reg


def rows(eu, ep, u, p, tau, B, score="dot", lqb=None, lam=0.0):
    """The batch-row part of a step on the samples' output rows eu, ep [nb, d] (float64 tensors), normalised by B -> dict:
    eh_u, eh_p, inv_u, inv_p, s, z, keep, m, q, Q, W, lterm, t_u, t_p (zeros under dot), gs_u, gs_p (the score part of the gradient
    rows), g_u, g_p (with lam e)."""
    cosine = _check(score)
    if cosine:
        (ehu, inv_u), (ehp, inv_p) = unit(eu), unit(ep)
    else:
        ehu, ehp = eu, ep
        inv_u, inv_p = torch.ones(len(eu), dtype=F64), torch.ones(len(ep), dtype=F64)
    s = ehu @ ehp.t()
    keep = IB.competitors(u, p)
    zz = (s - torch.diagonal(s)[:, None]) / float(tau)
    if lqb is not None:
        zz = zz - (lqb[None, :] - lqb[:, None])
    z = torch.where(keep, zz, torch.full_like(s, float("-inf")))
    m = torch.clamp(z.max(1).values, min=0.0)
    ez = torch.exp(z - m[:, None])
    Z = torch.exp(-m) + ez.sum(1)
    Zm1 = torch.where(m > 0, torch.exp(-m) + (ez.sum(1) - 1.0), ez.sum(1))
    lterm = torch.where(keep.any(1), m + torch.log1p(Zm1), torch.zeros_like(m))
    q = ez / Z[:, None]
    Q = q.sum(1)
    W = q / (float(tau) * float(B))
    W = W - torch.diag(Q / (float(tau) * float(B)))
    if cosine:
        t_u, t_p = (W * s).sum(1), (W * s).sum(0)
        gs_u = inv_u[:, None] * (W @ ehp - t_u[:, None] * ehu)
        gs_p = inv_p[:, None] * (W.t() @ ehu - t_p[:, None] * ehp)
        g_u = gs_u + lam * eu
        g_p = gs_p + lam * ep
    else:
        t_u, t_p = torch.zeros(len(eu), dtype=F64), torch.zeros(len(ep), dtype=F64)
        gs_u, gs_p = W @ ep, W.t() @ eu
        g_u = W @ ep + lam * eu
        g_p = W.t() @ eu + lam * ep
    return dict(eh_u=ehu, eh_p=ehp, inv_u=inv_u, inv_p=inv_p, s=s, z=z, keep=keep, m=m, q=q, Q=Q, W=W, lterm=lterm, term=-lterm,
                t_u=t_u, t_p=t_p, gs_u=gs_u, gs_p=gs_p, g_u=g_u, g_p=g_p)


def step(A, n_users, K, decay, tau, table, batch, reg_ego=False, w=None, B_norm=None, A_bwd=None, score="dot", logq=None):
    """inbatch_restatement.step with the two options -> its dict (e_u, e_p: the RAW rows) and eh_u, eh_p, inv_u, inv_p, lq [nb],
    t_u, t_p, gs_u, gs_p.  logq: numpy [m_items] (the fp32 vector the library is given), or None."""
    E0 = torch.from_numpy(np.asarray(table, np.float64))
    A = A.to(F64)
    u, p = (torch.from_numpy(t) for t in IB.as_samples(batch))
    nb = len(u)
    B = nb if B_norm is None else int(B_norm)
    N, d = E0.shape
    E = IB.propagate(A, E0, K, w)
    eu, ep = E[u], E[n_users + p]
    lqb = None if logq is None else torch.from_numpy(np.asarray(logq, np.float64))[p]
    lam = 0.0 if reg_ego else decay / float(B)
    r = rows(eu, ep, u, p, tau, B, score, lqb, lam)
    ru, rp = (E0[u], E0[n_users + p]) if reg_ego else (eu, ep)
    regterm = (ru * ru).sum(1) + (rp * rp).sum(1)
    sm = r["lterm"].sum() / float(B)
    reg = 0.5 * regterm.sum() / float(B)
    G = torch.zeros(N, d, dtype=F64)
    G.index_add_(0, u, r["g_u"])
    G.index_add_(0, n_users + p, r["g_p"])
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
    r.update(e_u=eu, e_p=ep, lq=torch.zeros(nb, dtype=F64) if lqb is None else lqb, regterm=regterm, G=G, cnt=cnt, g_final=h,
             loss_out=(sm + decay * reg, sm, reg), E=E, E0=E0)
    return r

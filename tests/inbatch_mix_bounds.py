"""The cases and the error bounds of tests/test_gpu_inbatch_mix.py (mixed negative sampling for the in-batch softmax),
in a module without a device so that tests/test_inbatch_mix_host.py can evaluate the SAME bound on the CPU: for every GPU case
it asserts that a step which ignored the pool would miss the bound on `terms` (the sensitivity check).  Test infrastructure.

BOUNDS (u = 2^-24; per element, first order in u unless said otherwise; magnitudes from the restatement).  The lines are those
of tests/test_gpu_inbatch.py and tests/test_gpu_inbatch_scores.py (forward, slot rows, score, sum of squares / sqrtf / division,
lq in z, normalise, W, g, the scalar t, projected row, diagonal, reg term, reg_ego, backward, loss_out) and are not repeated.  They are
applied to the B + B R columns of a sample's score row; what changes (Bp = B rounded up to 32, CPT = d / min(d, 64)):
  NP            the part count of the (1 + R) Bp-row item sweep, NP = ceil((1 + R) (Bp / 32) / 8), in kZ = 172 + 5 NP (the lane
                still adds at most 16 * 8 terms per part, the parts are merged in ascending order) and in the fixed-point line.
  user row      one partial row per part of the item sweep: NP partial adds, the diagonal and lam e: (NP + 2) 2^-51.  Per part an
                fmaf chain of at most n_u = min((1 + R) Bp, 256) terms.
  positive row  as before: it sweeps the user side, NPu = ceil((Bp / 32) / 8) parts of at most n_i = min(Bp, 256) terms, the
                diagonal and lam e: (NPu + 2) 2^-51.
  pool row      the user side's parts too, NO diagonal: the g line / the projected-row line without their diagonal terms, lam / R
                in place of lam (fl(decay / (B R)), one rounding like fl(decay / B)): (NPu + 1) 2^-51 <= (NPu + 2) 2^-51.
                Its own inv and t under cosine (the sum-of-squares / sqrtf / division lines on its own row).
  z             a pool column's z has the lq line with lq_{n_{c,r}} in place of lq_{p_c}; s_bb is the sample's own.
  reg term      gains 1/R sum_r |e_{n_r}|^2: the R CPT squares of a lane are summed in ONE chain (R CPT + 1 roundings with the
                square), the product with fl(1 / R) (2), the two additions to the user's and the positive's sums (2) and the 6 of
                the lane-group tree, against (2 CPT + 1 + 6) for the two other sums:
                delta_reg = (4 CPT + 12) u (|e_u|^2 + |e_p|^2) + (R CPT + 11) u / R sum_r |e_n|^2 + 2 sum |e| delta_e  (the /R on negatives)
  reg_ego       the last launch adds fl(decay / (B R)) cnt E0 (cnt = R per user / positive slot, 1 per negative slot): 4 u of
                it and 2 u of the sum, as in tests/test_gpu_softmax.py.
Nothing here is fitted to an observed error; the shares every test prints are recorded in profiles/inbatch_mix/README.md."""
import numpy as np

import inbatch_mix_restatement as IM
import inbatch_restatement as IB
import multineg_restatement as MN
import storage_cases as SC
from conftest import spmm_sum_bound

U = SC.U
MIN_N2 = 2.0 ** -60

# ---- the cases of test_steps_equal_the_restatement: (B, R, d, K, storage, reg rows, tau, (score, logq on)) ---------------------
BS, RS, DS, KS, MS, REGS, TS = (1, 2, 33, 65, 260), (1, 2, 16), (32, 64, 128, 256), (1, 2), ("fp32", "bf16"), ("propagated", "ego"), (0.2, 0.1)
OS = (("dot", False), ("cosine", True))
# Not the full product: every value of every axis meets at least two values of each other axis (tests/test_gpu_inbatch.py's
# _uncovered, asserted by both test files).  (65, 16): 51 item tiles = SEVEN parts, the last one ragged (3 tiles), the pool's
# padding rows 65..95 of every negative column; (260, 1): 18 item tiles, three parts; (1, .) and (2, .): a pool no larger than a
# tile's padding; d = 64: the register form's limit; 128 / 256: streamed operands, 256: two column workgroups per owned tile.
CASES = [
    (1, 1, 64, 1, "fp32", "propagated", 0.2, ("dot", False)),
    (1, 2, 32, 2, "bf16", "ego", 0.1, ("cosine", True)),
    (1, 16, 256, 1, "bf16", "ego", 0.2, ("cosine", True)),
    (2, 1, 128, 2, "bf16", "ego", 0.1, ("dot", False)),
    (2, 2, 64, 1, "fp32", "propagated", 0.2, ("cosine", True)),
    (2, 16, 32, 2, "fp32", "propagated", 0.1, ("dot", False)),
    (33, 1, 256, 2, "fp32", "propagated", 0.1, ("cosine", True)),
    (33, 2, 128, 1, "fp32", "ego", 0.2, ("dot", False)),
    (33, 16, 64, 2, "bf16", "propagated", 0.2, ("cosine", True)),
    (65, 16, 128, 1, "fp32", "propagated", 0.1, ("cosine", True)),
    (65, 1, 32, 1, "bf16", "ego", 0.2, ("dot", False)),
    (65, 2, 256, 2, "bf16", "propagated", 0.1, ("dot", False)),
    (65, 16, 64, 2, "fp32", "ego", 0.2, ("dot", False)),
    (260, 1, 64, 1, "bf16", "propagated", 0.1, ("cosine", True)),
    (260, 1, 128, 2, "fp32", "ego", 0.2, ("dot", False)),
    (260, 2, 32, 1, "fp32", "ego", 0.1, ("cosine", True)),
    (260, 16, 256, 2, "bf16", "propagated", 0.2, ("dot", False)),
]
AXES = (BS, RS, DS, KS, MS, REGS, TS, OS)
STEPS = 2
# The batch sizes the loss is trained and timed at (tests/test_gpu_inbatch_mix.py, section 1b).  CASES reaches many parts only
# through the ITEM tiles; the user side of the step (the pool rows' and the positives' sweep over the users, NPu parts) never has
# more than two there.  (2048, 1): the default --bpr_batch, 128 item tiles = 16 parts, EIGHT user parts; (545, 16): 18 user tiles
# = three user parts, the third ragged (two tiles, the last with one live row), 17 x 18 = 306 item tiles = 39 parts, the last
# ragged.  K in {1, 3}; every width twice; both storages on the register form (d <= 64) and on the streamed one (d >= 128).
LARGE_BRS = ((2048, 1), (545, 16))
LARGE_CASES = [
    (2048, 1, 64, 1, "bf16", "propagated", 0.1, ("cosine", True)),
    (2048, 1, 128, 3, "fp32", "ego", 0.2, ("dot", False)),
    (2048, 1, 32, 3, "fp32", "propagated", 0.2, ("dot", False)),
    (2048, 1, 256, 1, "bf16", "ego", 0.1, ("cosine", True)),
    (545, 16, 32, 1, "bf16", "ego", 0.1, ("cosine", True)),
    (545, 16, 256, 3, "fp32", "propagated", 0.2, ("dot", False)),
    (545, 16, 64, 3, "fp32", "ego", 0.2, ("cosine", True)),
    (545, 16, 128, 1, "bf16", "propagated", 0.1, ("dot", False)),
]


def case_id(c):
    return f"B{c[0]}-R{c[1]}-d{c[2]}-K{c[3]}-{c[4]}-{c[5]}-tau{c[6]}-{c[7][0]}{'-logq' if c[7][1] else ''}"


def case_batches(c):
    return IM.make_batches(c[0], c[1], STEPS, seed=c[2] + c[3])


def tau32(tau):
    return float(np.float32(tau))


def parts_items(B, R):
    return ((1 + R) * ((B + 31) // 32) + 7) // 8


def parts_users(B):
    return (((B + 31) // 32) + 7) // 8


def _c(n):
    return int(np.ceil(n / 64.0)) + 8


def _check_large_cases():
    """What LARGE_CASES must reach, asserted at import (no device)."""
    cs = LARGE_CASES
    assert {(c[0], c[1]) for c in cs} == set(LARGE_BRS)
    assert {parts_users(c[0]) for c in cs} == {3, 8} and all(parts_items(c[0], c[1]) > parts_users(c[0]) for c in cs)
    assert all(sum(c[2] == d for c in cs) >= 2 for d in DS) and {c[3] for c in cs} == {1, 3}
    assert all({c[4] for c in cs if ok(c[2])} == set(MS) for ok in (lambda d: d <= 64, lambda d: d >= 128))
    assert {c[5] for c in cs} == set(REGS) and {c[7] for c in cs} == set(OS)
    for c in cs:
        for u, p, negs in case_batches(c):
            B = len(u)
            assert negs.shape == (c[0], c[1]) and IB.kept_share(u, p) > 0.5
            assert u[B - 1] in u[:IB.PART_ROWS] and p[B - 1] in p[:IB.PART_ROWS] and negs[B - 1, 0] in p[:IB.PART_ROWS]      # across parts


_check_large_cases()


def bounds(adj, r, batch, B, K, d, mode, ego, tau, cosine, lq, only_term=False):
    """The bounds of the module docstring from a restatement r (inbatch_mix_restatement.step) of the sound samples `batch` of a
    step normalised by B, on the graph adj (scipy CSR of A_hat) -> dict: term, regterm [b], loss (3), g_final [N, d], rho."""
    fwd = adj.astype(np.float64)
    af = abs(fwd).tocsr()
    wk = MN.layer_weights(K, None)
    E0 = r["E0"].numpy()
    R = int(r["R"])
    # ---- forward tables and slot rows (tests/test_gpu_softmax.py)
    X = E0
    T = abs(wk[0]) * np.abs(E0)
    dX = SC.stored_bound(E0, 0.0, "bf16") if (mode == "bf16" and K >= 2) else np.zeros_like(E0)
    dE = np.zeros_like(E0)
    for k in range(1, K + 1):
        pre = af @ dX + spmm_sum_bound(af.indptr, af.data, af.indices, np.abs(X) + dX, extra_terms=2)
        X = fwd @ X
        dX = SC.stored_bound(X, pre, "bf16") if mode == "bf16" else pre
        T = T + abs(wk[k]) * np.abs(X)
        dE = dE + abs(wk[k]) * dX
    dE = dE + (K + 2) * U * T
    T = T + dE
    u_, p_, negs = IM.as_samples(batch)
    n_ = r["n"].numpy()
    nb, P = len(u_), len(n_)
    ui, pi, ni = u_, SC.N_USERS + p_, SC.N_USERS + n_
    ii = np.concatenate([pi, ni])                                           # the item side: positives, then the pool
    au, ai, du, di = T[ui], T[ii], dE[ui], dE[ii]
    NP, NPu = parts_items(B, R), parts_users(B)
    kZ = 172 + 5 * NP
    CPT = d // min(d, 64)
    # ---- the rows the score is formed from
    rho_u, rho_i = np.zeros(nb), np.zeros(nb + P)
    inv_u, inv_i = np.ones(nb), np.ones(nb + P)
    hu, hi, dhu, dhi = au, ai, du, di
    if cosine:
        def hat(a, de, inv, eh):
            n2 = 1.0 / inv ** 2
            assert (inv > 0).all() and (n2 >= MIN_N2).all()
            dn2 = (CPT + 7) * U * (a * a).sum(1) + (2 * a * de).sum(1) + d * 2.0 ** -149
            eps = dn2 / n2
            assert (eps < 0.25).all(), float(eps.max())
            rho = 0.5 * eps * (1.0 - eps) ** -1.5 + 2 * U
            dh = np.abs(eh) * (rho + U)[:, None] + de * (inv * (1 + rho))[:, None]
            return np.abs(eh) + dh, dh, rho, inv * (1 + rho)
        hu, dhu, rho_u, inv_u = hat(au, du, r["inv_u"].numpy(), r["eh_u"].numpy())
        hi, dhi, rho_i, inv_i = hat(ai, di, np.concatenate([r["inv_p"].numpy(), r["inv_n"].numpy()]),
                                    np.concatenate([r["eh_p"].numpy(), r["eh_n"].numpy()]))
    # ---- scores and z over the nb + P columns
    Sabs = hu @ hi.T
    opd = dhu @ hi.T + hu @ dhi.T
    ds = (d + 1) * U * Sabs + opd
    dsbb = (d + 2) * U * np.diag(Sabs[:, :nb]) + np.diag(opd[:, :nb])
    keep = r["keep"].numpy()
    z = np.where(keep, r["z"].numpy(), 0.0)
    lqb, lqi = r["lq"].numpy(), np.concatenate([r["lq"].numpy(), r["lq_n"].numpy()])
    dl = (lqi[None, :] - lqb[:, None]) if lq else np.zeros_like(z)
    mm, q, l, Q = r["m"].numpy(), r["q"].numpy(), r["lterm"].numpy(), r["Q"].numpy()
    dz = np.where(keep, (ds + dsbb[:, None]) / tau + 2 * U * np.abs(z + dl) + (U * (np.abs(dl) + np.abs(z)) if lq else 0.0), 0.0)
    a = np.where(keep, np.abs(z - mm[:, None]), 0.0)
    q0 = np.where(mm > 0, 1.0 - Q, 0.0)
    Pm = np.minimum(Q + q0, 1.0)
    qd = (q * (dz + U * a)).sum(1)
    rho = kZ * U * Pm + qd
    out = {"term": rho + 3 * U * l + 1e-37, "rho": float(max(rho_u.max(), rho_i.max()))}
    if only_term:
        return out
    dq = np.where(keep, q * (4 * U + dz + U * a + rho[:, None]) + 2.0 ** -140, 0.0)
    dQ = Q * (kZ + 6) * U + qd + 2.0 ** -140 * (Q > 0)
    itb = 1.0 / (tau * B)
    Wabs = q * itb
    dW = 2 * U * Wabs + dq * itb
    Wd = Q * itb
    dWd = 2 * U * Wd + dQ * itb
    # ---- reg term (raw rows)
    sq = lambda x: x.reshape(R, nb, -1).sum((0, 2)) if R else np.zeros(nb)      # pool order r B + c -> per sample
    if ego:
        e0 = np.abs(E0)
        reg_up, reg_n = (e0[ui] ** 2).sum(1) + (e0[pi] ** 2).sum(1), sq(e0[ni] ** 2)
        d_regx = 0.0
    else:
        reg_up, reg_n = (au * au).sum(1) + (ai[:nb] * ai[:nb]).sum(1), sq(ai[nb:] * ai[nb:])
        d_regx = 2.0 * ((au * du).sum(1) + (ai[:nb] * di[:nb]).sum(1) + sq(ai[nb:] * di[nb:]) / max(R, 1))
    regterm = reg_up + reg_n / max(R, 1)
    out["regterm"] = (4 * CPT + 12) * U * reg_up + (R * CPT + 11) * U * reg_n / max(R, 1) + d_regx + 1e-37
    cB = _c(B) * U
    b_sm = out["term"].sum() / B + cB * l.sum() / B
    b_reg = 0.5 * (out["regterm"].sum() / B + cB * regterm.sum() / B)
    lo = [float(v) for v in r["loss_out"]]
    out["loss"] = (b_sm + SC.DECAY * b_reg + 4 * U * (abs(lo[1]) + SC.DECAY * abs(lo[2])), b_sm, b_reg)
    # ---- gradient rows
    Bp = ((B + 31) // 32) * 32
    lam = 0.0 if ego else SC.DECAY / B
    lam_i = np.concatenate([np.full(nb, lam), np.full(P, lam / max(R, 1))])
    n_u, n_i = min((1 + R) * Bp, IB.PART_ROWS), min(Bp, IB.PART_ROWS)
    fx_u, fx_i = (NP + 2) * 2.0 ** -51, (NPu + 2) * 2.0 ** -51
    Wf = Wabs + dW
    ap, dp = hi[:nb], dhi[:nb]                                              # the positives' rows (the diagonal's operands)
    pad = lambda x: np.concatenate([x, np.zeros((P,) + x.shape[1:])])      # the diagonal exists on the positives' rows only
    if cosine:
        sf = np.abs(r["s"].numpy()) + ds
        sbb = np.abs(np.diag(r["s"].numpy()[:, :nb])) + dsbb

        def off(Wm, dWm, own, down, oth, doth, inv, rho_o, sfm, dsm, n_chain):
            G_abs = Wm @ oth
            dg = (n_chain + 1) * U * G_abs + dWm @ oth + Wm @ doth
            t_abs = (Wm * sfm).sum(1)
            dt = (n_chain + 1) * U * t_abs + (dWm * sfm).sum(1) + (Wm * dsm).sum(1)
            return inv[:, None] * (dg + dt[:, None] * own + t_abs[:, None] * down + (3 * U + rho_o)[:, None] * (G_abs + t_abs[:, None] * own))

        def dia(own, down, oth, doth, inv, rho_o):
            m_ = oth + sbb[:, None] * own
            return inv[:, None] * (dWd[:, None] * m_ + Wd[:, None] * (doth + dsbb[:, None] * own + sbb[:, None] * down)
                                   + (Wd * (4 * U + rho_o))[:, None] * m_)
        d_gu = off(Wf, dW, hu, dhu, hi, dhi, inv_u, rho_u, sf, ds, n_u) + dia(hu, dhu, ap, dp, inv_u, rho_u) + 6 * U * lam * au + lam * du + fx_u
        d_gi = (off(Wf.T, dW.T, hi, dhi, hu, dhu, inv_i, rho_i, sf.T, ds.T, n_i) + pad(dia(ap, dp, hu, dhu, inv_i[:nb], rho_i[:nb]))
                + 6 * U * lam_i[:, None] * ai + lam_i[:, None] * di + fx_i)
    else:
        d_gu = ((n_u + 1) * U * (Wf @ ai) + dW @ ai + Wf @ di + 2 * U * Wd[:, None] * ap + dWd[:, None] * ap + (Wd + dWd)[:, None] * dp
                + 6 * U * lam * au + lam * du + fx_u)
        d_gi = ((n_i + 1) * U * (Wf.T @ au) + dW.T @ au + Wf.T @ du + pad(2 * U * Wd[:, None] * au + dWd[:, None] * au + (Wd + dWd)[:, None] * du)
                + 6 * U * lam_i[:, None] * ai + lam_i[:, None] * di + fx_i)
    dG = np.zeros_like(T)
    np.add.at(dG, ui, d_gu); np.add.at(dG, ii, d_gi)
    div = float(K + 1)
    Gref = r["G"].numpy()
    Gs = np.abs(Gref) / div
    dGs = dG / div + 2 * U * Gs
    # ---- backward chain (tests/test_gpu_softmax.py)
    cw = [abs(x) * div for x in wk]
    v = cw[K] * (Gref / div)
    h, dh = np.abs(v), cw[K] * dGs
    D = dh
    for i in range(K):
        k = K - i
        Ah = af @ h
        D = cw[k - 1] * dGs + af @ dh + spmm_sum_bound(af.indptr, af.data, af.indices, h + dh, extra_terms=2) + 2 * U * (cw[k - 1] * Gs + Ah)
        v = (wk[k - 1] * div) * (Gref / div) + fwd @ v
        if i < K - 1 and mode == "bf16":
            D = SC.stored_bound(v, D, "bf16")
        h, dh = np.abs(v), D
    if ego:
        D = D + 4 * U * (SC.DECAY / (B * max(R, 1))) * r["cnt"].numpy()[:, None] * np.abs(E0) + 2 * U * np.abs(r["g_final"].numpy())
    out["g_final"] = D
    return out


def sensitivity(adj, A, table, batch, B, K, d, mode, ego, tau, score, logq, B_norm=None):
    """How far a step that ignored the pool would miss: max over the samples of |term with the pool - term without| / the bound on
    the term (with the pool) -> (that share, the restatement with the pool, its term bound)."""
    Bn = B if B_norm is None else B_norm
    r = IM.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, ego, None, B_norm=Bn, score=score, logq=logq)
    r0 = IM.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch[:2], ego, None, B_norm=Bn, score=score, logq=logq)
    bd = bounds(adj, r, batch, Bn, K, d, mode, ego, tau, score == "cosine", logq is not None, only_term=True)
    return float((np.abs(r["term"].numpy() - r0["term"].numpy()) / bd["term"]).max()), r, bd

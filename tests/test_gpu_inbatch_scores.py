"""The two score options of the in-batch softmax (--score cosine, --inbatch_logq 1; lgcn_ctx_set_inbatch_scores,
csrc/lgcn_inbatch.hip) on the GPU (-m gpu), on the graph and table rows of tests/storage_cases.py with the batches of
tests/inbatch_restatement.py, against the float64 restatement tests/inbatch_scores_restatement.py.  Every step is judged from the
GPU's OWN state before the step.

BOUNDS (u = 2^-24; per element, first order in u unless said otherwise; magnitudes from the restatement).  The forward / slot
rows / score / normalise / W / g / reg term / reg_ego / backward / loss_out lines are those of tests/test_gpu_inbatch.py (and,
through it, tests/test_gpu_softmax.py) and are not repeated: they are applied to the rows e^ the score is formed from and to
the z below.  New (e a raw output row with its bound delta_e, CPT = d / min(d, 64)):
  sum of squares  n2 = sum_k e_k^2: CPT fmaf terms in the lane, 6 additions in the lane-group tree, all terms >= 0:
                  delta_n2 = (CPT + 7) u n2 + sum_k (2 |e_k| delta_e_k + delta_e_k^2) + d 2^-149      (a subnormal square)
                  The tests assert, in float64, n2 >= 2^-60 for every row of a sound sample: far from the underflow of a square.
  sqrtf           correctly rounded: |e| (1 + eps)^(1/2) (1 + u), eps = delta_n2 / n2
  the division    inv = 1 / |e|, correctly rounded.  Together, NOT first order in eps (bf16 rows: eps is a few 1e-3):
                  rho = delta_inv / inv = (eps / 2) (1 - eps)^(-3/2) + 2 u                               (two roundings)
  e . inv         e^_k = e_k inv: delta_e^_k = |e^_k| (rho + u) + delta_e_k inv (1 + rho)
                  s_{b,c}, s_{b,b} and their deltas: the score line of tests/test_gpu_inbatch.py on e^, delta_e^.
  lq in z         lq is the same fp32 vector on both sides (exact).  z = z0 - fl(lq_c - lq_b), z0 = (s_bc - s_bb) / tau:
                  delta_z = (delta_s_bc + delta_s_bb) / tau + 2 u |z0| + u |lq_c - lq_b| + u |z|
  the scalar t    t_o = sum_x W[x,o] s[x,o] over the off-diagonal rows of one part: at most n = min(Bp, 256) / 2 fmaf terms in
                  the lane and one addition for the other lane half, bounded by the (n + 1) of the g line:
                  delta_t = (n + 1) u sum |W| |s| + sum (delta_W |s| + |W| delta_s)
  projected row   per part inv_o (g - t o^), g the g line of tests/test_gpu_inbatch.py on e^ (without diagonal and lam):
                  the product t o^ and the subtraction (2 u, 1 if contracted), the product with inv (u), inv itself (rho):
                  delta = inv (1 + rho) [ delta_g + delta_t |o^| + |t| delta_o^ + (3 u + rho) (sum |W| |e^| + sum |W| |s| |o^|) ]
                  The bound is linear in the sums, so the parts' bounds add up to the bound of the whole sweep.
  the diagonal    inv_u W_bb (p^_b - s_bb u^_b) with W_bb of the W line (delta_W_bb) and the s_bb of the rows launch:
                  delta = inv (1 + rho) [ delta_W_bb m + |W_bb| (delta_p^ + delta_s_bb |u^| + |s_bb| delta_u^) + (4 u + rho) |W_bb| m ],
                  m = |p^_b| + |s_bb| |u^_b|; the mirror for the item row.
  lam e, reg      on the raw rows: the lines of tests/test_gpu_inbatch.py unchanged.  Fixed point: (NP + 2) 2^-51 per row.
Every test prints the largest share of each bound it used (recorded in profiles/inbatch_scores/README.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import inbatch_restatement as IB
import inbatch_scores_restatement as IS
import multineg_restatement as MN
import storage_cases as SC
from conftest import spmm_sum_bound
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)
from test_gpu_gate_shapes import W1, _adam_checks
from test_gpu_inbatch import _G, _c, _dev, _model, _parts, _same, _snapshot, _state, _tau32, _uncovered
from test_gpu_inbatch import _LARGE_CASES as _PLAIN_LARGE_CASES, check_large_cases, large_batches

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = SC.U
MIN_N2 = 2.0 ** -60
_LQ = {}


def _logq(ds):
    if "lq" not in _LQ:
        _LQ["lq"] = IS.item_logq(ds.items_D)
    return _LQ["lq"]


def _cfg(tau, score, lq_on, **more):
    return dict(loss='inbatch', softmax_temp=tau, score=score, inbatch_logq=int(lq_on), **more)


def _bounds(r, batch, B, K, d, mode, ego, w, tau, cosine, lq):
    """The bounds of the module docstring (and of tests/test_gpu_inbatch.py, whose _bounds this follows line by line) from a
    restatement r of the sound samples `batch` of a step normalised by B -> dict: term, regterm [b], loss (3), g_final [N, d],
    rho (the largest relative bound of an inv)."""
    adj = _G["adj"]
    fwd = adj.astype(np.float64)
    af = abs(fwd).tocsr()
    wk = MN.layer_weights(K, w)
    E0 = r["E0"].numpy()
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
    dE = dE + ((K + 2) if w is None else 2 * (K + 2)) * U * T
    T = T + dE
    u_, p_ = IB.as_samples(batch)
    ui, pi = u_, SC.N_USERS + p_
    au, ap, du, dp = T[ui], T[pi], dE[ui], dE[pi]
    NP = _parts(B)
    kZ = 172 + 5 * NP
    CPT = d // min(d, 64)
    # ---- the rows the score is formed from
    rho_u = rho_p = np.zeros(len(u_))
    inv_u = inv_p = np.ones(len(u_))
    hu, hp, dhu, dhp = au, ap, du, dp
    if cosine:
        def hat(a, de, inv, eh):
            n2 = 1.0 / inv ** 2
            assert (inv > 0).all() and (n2 >= MIN_N2).all()
            dn2 = (CPT + 7) * U * (a * a).sum(1) + (2 * a * de).sum(1) + d * 2.0 ** -149      # a = |e| + delta_e: 2 a de >= 2 |e| de + de^2
            eps = dn2 / n2
            assert (eps < 0.25).all(), float(eps.max())
            rho = 0.5 * eps * (1.0 - eps) ** -1.5 + 2 * U
            dh = np.abs(eh) * (rho + U)[:, None] + de * (inv * (1 + rho))[:, None]
            return np.abs(eh) + dh, dh, rho, inv * (1 + rho)
        hu, dhu, rho_u, inv_u = hat(au, du, r["inv_u"].numpy(), r["eh_u"].numpy())
        hp, dhp, rho_p, inv_p = hat(ap, dp, r["inv_p"].numpy(), r["eh_p"].numpy())
    # ---- scores (tests/test_gpu_inbatch.py on e^) and z
    Sabs = hu @ hp.T
    opd = dhu @ hp.T + hu @ dhp.T
    ds = (d + 1) * U * Sabs + opd
    dsbb = (d + 2) * U * np.diag(Sabs) + np.diag(opd)
    keep = r["keep"].numpy()
    z = np.where(keep, r["z"].numpy(), 0.0)
    lqb = r["lq"].numpy()
    dl = (lqb[None, :] - lqb[:, None]) if lq else np.zeros_like(z)
    mm, q, l, Q = r["m"].numpy(), r["q"].numpy(), r["lterm"].numpy(), r["Q"].numpy()
    dz = np.where(keep, (ds + dsbb[:, None]) / tau + 2 * U * np.abs(z + dl) + (U * (np.abs(dl) + np.abs(z)) if lq else 0.0), 0.0)
    a = np.where(keep, np.abs(z - mm[:, None]), 0.0)
    q0 = np.where(mm > 0, 1.0 - Q, 0.0)
    P = np.minimum(Q + q0, 1.0)
    qd = (q * (dz + U * a)).sum(1)
    rho = kZ * U * P + qd
    out = {"term": rho + 3 * U * l + 1e-37, "rho": float(max(rho_u.max(), rho_p.max()))}
    dq = np.where(keep, q * (4 * U + dz + U * a + rho[:, None]) + 2.0 ** -140, 0.0)
    dQ = Q * (kZ + 6) * U + qd + 2.0 ** -140 * (Q > 0)
    itb = 1.0 / (tau * B)
    Wabs = q * itb
    dW = 2 * U * Wabs + dq * itb
    Wd = Q * itb
    dWd = 2 * U * Wd + dQ * itb
    # ---- reg term (raw rows)
    if ego:
        e0 = np.abs(E0)
        regterm = (e0[ui] ** 2).sum(1) + (e0[pi] ** 2).sum(1)
        d_regx = 0.0
    else:
        regterm = (au * au).sum(1) + (ap * ap).sum(1)
        d_regx = 2.0 * ((au * du).sum(1) + (ap * dp).sum(1))
    out["regterm"] = (4 * CPT + 12) * U * regterm + d_regx + 1e-37
    cB = _c(B) * U
    b_sm = out["term"].sum() / B + cB * l.sum() / B
    b_reg = 0.5 * (out["regterm"].sum() / B + cB * regterm.sum() / B)
    lo = [float(v) for v in r["loss_out"]]
    out["loss"] = (b_sm + SC.DECAY * b_reg + 4 * U * (abs(lo[1]) + SC.DECAY * abs(lo[2])), b_sm, b_reg)
    # ---- gradient rows
    lam = 0.0 if ego else SC.DECAY / B
    n_chain = min(((B + 31) // 32) * 32, IB.PART_ROWS)
    fx = (NP + 2) * 2.0 ** -51
    Wf = Wabs + dW
    if cosine:
        sf = np.abs(r["s"].numpy()) + ds
        sbb = np.abs(np.diag(r["s"].numpy())) + dsbb

        def side(Wm, dWm, own, down, oth, doth, inv, rho_o, sfm, dsm):
            G_abs = Wm @ oth
            dg = (n_chain + 1) * U * G_abs + dWm @ oth + Wm @ doth
            t_abs = (Wm * sfm).sum(1)
            dt = (n_chain + 1) * U * t_abs + (dWm * sfm).sum(1) + (Wm * dsm).sum(1)
            off = inv[:, None] * (dg + dt[:, None] * own + t_abs[:, None] * down + (3 * U + rho_o)[:, None] * (G_abs + t_abs[:, None] * own))
            m_ = oth + sbb[:, None] * own
            dia = inv[:, None] * (dWd[:, None] * m_ + Wd[:, None] * (doth + dsbb[:, None] * own + sbb[:, None] * down)
                                  + (Wd * (4 * U + rho_o))[:, None] * m_)
            return off + dia
        d_gu = side(Wf, dW, hu, dhu, hp, dhp, inv_u, rho_u, sf, ds) + 6 * U * lam * au + lam * du + fx
        d_gp = side(Wf.T, dW.T, hp, dhp, hu, dhu, inv_p, rho_p, sf.T, ds.T) + 6 * U * lam * ap + lam * dp + fx
    else:
        d_gu = ((n_chain + 1) * U * (Wf @ ap) + dW @ ap + Wf @ dp + 2 * U * Wd[:, None] * ap + dWd[:, None] * ap + (Wd + dWd)[:, None] * dp
                + 6 * U * lam * au + lam * du + fx)
        d_gp = ((n_chain + 1) * U * (Wf.T @ au) + dW.T @ au + Wf.T @ du + 2 * U * Wd[:, None] * au + dWd[:, None] * au + (Wd + dWd)[:, None] * du
                + 6 * U * lam * ap + lam * dp + fx)
    dG = np.zeros_like(T)
    np.add.at(dG, ui, d_gu); np.add.at(dG, pi, d_gp)
    div = 1.0 if w is not None else float(K + 1)
    Gref = r["G"].numpy()
    Gs = np.abs(Gref) / div
    dGs = dG / div + 2 * U * Gs
    # ---- backward chain (tests/test_gpu_softmax.py)
    cw = [abs(x) * div for x in wk]
    v = cw[K] * (Gref / div)
    h, dh = np.abs(v), cw[K] * dGs + (U * cw[K] * Gs if w is not None else 0.0)
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
        D = D + 4 * U * (SC.DECAY / B) * r["cnt"].numpy()[:, None] * np.abs(E0) + 2 * U * np.abs(r["g_final"].numpy())
    out["g_final"] = D
    return out


def _judge(pkg, ds, m, batch, K, d, mode, reg, tau, step_no, tag, score, lq_on, void=()):
    """One fused step from the GPU's own state -> ({link: share of its bound}, restatement, raw outputs)."""
    A = _G["A"]
    ego = reg == "ego"
    B = len(batch[0])
    st = m._state(max_batch=max(B, int(m.config.get('bpr_batch_size', B))), need_ctx=True)
    lib = pkg._lib.load()
    got_lq = C.c_void_p(0)
    kind = lib.lgcn_ctx_get_inbatch_scores(st['ctx'], C.byref(got_lq))
    assert kind == (pkg._lib.SCORE_COSINE if score == "cosine" else pkg._lib.SCORE_DOT)
    assert (got_lq.value == st['item_logq'].data_ptr()) if lq_on else (got_lq.value is None)
    lq = _logq(ds) if lq_on else None
    if lq_on:
        assert np.array_equal(st['item_logq'].cpu().numpy(), lq)
    assert m.adam_step == step_no - 1
    before = _state(m)
    neg = np.zeros(B, np.int64)                                             # accepted and ignored
    out = m.fused_step(_dev(batch[0]), _dev(batch[1]), _dev(neg)).cpu().numpy().astype(np.float64)
    after = _state(m)
    t = m._dev['terms'].cpu().numpy().astype(np.float64)
    term, regt = t[:B], t[B:2 * B]
    sound = np.ones(B, bool)
    for v_ in void:
        sound[v_] = False
        assert term[v_] == 0.0 and regt[v_] == 0.0
    sb = tuple(np.asarray(a_)[sound] for a_ in batch[:2])
    r = IS.step(A, SC.N_USERS, K, SC.DECAY, tau, before["table"], sb, ego, None, B_norm=B, score=score, logq=lq)
    if score == "cosine":       # far from a zero norm and from the underflow of a square, in float64 and never from the device
        assert float((r["e_u"] ** 2).sum(1).min()) >= MIN_N2 and float((r["e_p"] ** 2).sum(1).min()) >= MIN_N2
    bd = _bounds(r, sb, B, K, d, mode, ego, None, tau, score == "cosine", lq_on)
    assert np.isfinite(out).all() and np.isfinite(t[:2 * B]).all() and np.isfinite(after["M"]).all()
    share = {}
    share["term"] = float((np.abs(term[sound] - r["term"].numpy()) / bd["term"]).max())
    share["regterm"] = float((np.abs(regt[sound] - r["regterm"].numpy()) / bd["regterm"]).max())
    for j in range(3):
        share[f"loss{j}"] = abs(out[j] - float(r["loss_out"][j])) / bd["loss"][j]
    slack = 2.0 ** -21 * (np.abs(before["M"]) + np.abs(after["M"])) / W1
    g_rec = before["M"] + (after["M"] - before["M"]) / W1
    g_ref = r["g_final"].numpy()
    assert float(np.abs(g_rec).max()) > 0.0
    share["grad"] = float((np.abs(g_rec - g_ref) / (bd["g_final"] + slack + 1e-300)).max())
    share["adam"] = _adam_checks((tag, "table"), before["table"], before["M"], before["V"], after["table"], after["M"], after["V"],
                                 g_rec, slack, step_no, False)
    # how tight: the bound of the gradient against the gradient itself, over the rows the batch names
    rows_ = np.unique(np.concatenate([sb[0], SC.N_USERS + sb[1]]))
    tight = float(np.median(bd["g_final"][rows_].max(1) / (np.abs(g_ref[rows_]).max(1) + 1e-300)))
    print(f"[inbatch_scores] {tag}: shares " + " ".join(f"{k}={v:.3f}" for k, v in share.items()) + f" | rho_inv {bd['rho']:.2e} bound/|g| median {tight:.2e}")
    return share, r, (term, regt, g_rec, slack, bd, out)


def _run(pkg, path, mode, d, K, B, tau, reg, score, lq_on, batches=None):
    try:
        ds, m = _model(pkg, path, mode, d, K, reg, dl=0, batch=B, **_cfg(tau, score, lq_on))
        top, bad = {}, []
        for i, batch in enumerate(batches or IB.make_batches(B, 3, seed=d + K)):
            tag = f"{score}{'+logq' if lq_on else ''} {mode} d{d} K{K} tau{tau} {reg} step {i + 1} B={len(batch[0])}"
            share = _judge(pkg, ds, m, batch, K, d, mode, reg, _tau32(tau), i + 1, tag, score, lq_on)[0]
            for k_, v in share.items():
                top[k_] = max(top.get(k_, 0.0), v)
                if not v <= 1.0:
                    bad.append((tag, k_, v))
            m.check_device_errors()
            assert not bool(m._dev['G64'].any()) and m.adam_step == i + 1
        print(f"[inbatch_scores] {score}{'+logq' if lq_on else ''} {mode} d{d} K{K} B{B} tau{tau} {reg} TOP: " + " ".join(f"{k_}={v:.3f}" for k_, v in top.items()))
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
    finally:
        pkg.world.configure([])


# ---- 1. three steps against the float64 restatement ------------------------------------------------------------------------
_BS, _DS, _KS, _MS, _RS, _TS = (1, 2, 33, 65, 260), (32, 64, 128, 256), (1, 2), ("fp32", "bf16"), ("propagated", "ego"), (0.2, 0.1)
_OS = IS.NEW_OPTIONS
# Not the full product: every value of every axis meets at least two values of each other axis (checked below).  B = 1: no
# competitor; 2: the smallest batch with one; 33: two tiles, padded rows; 65: three tiles, duplicates across tiles; 260: two parts
# of the sweep (the projection per part, merged in G64).  d = 32: one column block, 32-lane groups; 64: the register form's limit;
# 128: streamed operands, four column blocks; 256: two workgroups per owned tile recompute t.  The last row is both at once.
_CASES = [
    (1, 64, 2, 'bf16', 'ego', 0.1, ('dot', True)),
    (1, 32, 1, 'bf16', 'propagated', 0.2, ('cosine', False)),
    (1, 256, 1, 'fp32', 'ego', 0.1, ('cosine', True)),
    (2, 128, 2, 'fp32', 'ego', 0.2, ('cosine', False)),
    (2, 64, 1, 'fp32', 'propagated', 0.1, ('dot', True)),
    (2, 256, 1, 'bf16', 'ego', 0.2, ('cosine', True)),
    (33, 64, 1, 'bf16', 'propagated', 0.2, ('cosine', True)),
    (33, 32, 2, 'bf16', 'ego', 0.1, ('cosine', False)),
    (33, 256, 2, 'fp32', 'propagated', 0.2, ('dot', True)),
    (65, 128, 2, 'bf16', 'propagated', 0.2, ('cosine', True)),
    (65, 64, 1, 'bf16', 'ego', 0.1, ('dot', True)),
    (65, 32, 1, 'fp32', 'propagated', 0.2, ('cosine', False)),
    (260, 128, 1, 'bf16', 'ego', 0.1, ('dot', True)),
    (260, 64, 2, 'bf16', 'propagated', 0.2, ('cosine', False)),
    (260, 32, 2, 'fp32', 'ego', 0.1, ('cosine', True)),
    (260, 256, 1, 'fp32', 'propagated', 0.2, ('cosine', True)),
]
assert not _uncovered(_CASES), _uncovered(_CASES)
assert all({c[a] for c in _CASES} == set(ax) for a, ax in enumerate((_BS, _DS, _KS, _MS, _RS, _TS, _OS)))


@pytest.mark.parametrize("B,d,K,mode,reg,tau,opt", [pytest.param(*c, id=f"B{c[0]}-d{c[1]}-K{c[2]}-{c[3]}-{c[4]}-tau{c[5]}-{c[6][0]}{'-logq' if c[6][1] else ''}") for c in _CASES])
def test_steps_equal_the_restatement(pkg, storage_graph, B, d, K, mode, reg, tau, opt):
    """Per-sample terms, loss_out, the gradient recovered from Adam's first moment and Adam itself, each within the bound derived
    in the module docstring, over three consecutive batches of B samples."""
    _run(pkg, storage_graph, mode, d, K, B, tau, reg, opt[0], opt[1])


# ---- 1b. the batch sizes the loss is trained and timed at ----------------------------------------------------------------------
# tests/test_gpu_inbatch.py section 1b for the three new score options: B = 513 (three parts, the third one tile with one live
# row) and B = 2048 (eight parts).  The projection runs per part and the parts meet in G64, so cosine reaches the per-part
# addressing of t and of the partial rows beyond two parts here first.  The bounds are section 1's, unchanged (functions of B
# through NP, n = min(Bp, 256) and c(B)).  With the four dot cases of tests/test_gpu_inbatch.py every width stands twice.
_LARGE_CASES = [
    (513, 64, 1, 'bf16', 'propagated', 0.2, ('cosine', False)),
    (513, 256, 3, 'fp32', 'ego', 0.1, ('dot', True)),
    (2048, 32, 3, 'fp32', 'propagated', 0.1, ('cosine', True)),
    (2048, 128, 1, 'bf16', 'ego', 0.2, ('cosine', True)),
]
check_large_cases(_LARGE_CASES, lambda c: large_batches(c[0], c[1], c[2]))
assert {c[6] for c in _LARGE_CASES} == set(_OS)
assert sorted(c[1] for c in _LARGE_CASES + _PLAIN_LARGE_CASES) == [32, 32, 64, 64, 128, 128, 256, 256]


@pytest.mark.parametrize("B,d,K,mode,reg,tau,opt", [pytest.param(*c, id=f"B{c[0]}-d{c[1]}-K{c[2]}-{c[3]}-{c[4]}-tau{c[5]}-{c[6][0]}{'-logq' if c[6][1] else ''}") for c in _LARGE_CASES])
def test_steps_equal_the_restatement_at_the_training_batch_sizes(pkg, storage_graph, B, d, K, mode, reg, tau, opt):
    """Section 1 at B = 513 and B = 2048: the same links within the same derived bounds, over two consecutive batches that repeat
    a user and a positive across parts."""
    _run(pkg, storage_graph, mode, d, K, B, tau, reg, opt[0], opt[1], batches=large_batches(B, d, K))


# ---- 2. masks and voids ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score,lq_on", _OS)
def test_duplicates_inside_one_tile_and_across_tiles(pkg, storage_graph, score, lq_on):
    """The batch of 65 (three tiles): the same user and the same positive inside tile 0, across tiles 0 / 1 and 0 / 2: repeated
    ids sum, each sample projected with its own t."""
    u, p = IB.make_batch(65, seed=3)
    keep = IB.competitors(u, p).numpy()
    assert not keep[0, 1] and not keep[4, 5] and not keep[2, 40] and not keep[15, 50] and not keep[16, 64] and not keep[17, 64]
    _run(pkg, storage_graph, "fp32", 64, 2, 65, 0.2, "propagated", score, lq_on, batches=[(u, p)])


@pytest.mark.parametrize("what", ["user", "pos", "both"])
def test_voided_samples(pkg, storage_graph, what):
    """An out-of-range user, positive, or both, at the first, a middle and the last position of a batch of 65, cosine + logq:
    err is set, the id check precedes the lq gather (an out-of-range positive is never an index), the samples are void as rows
    and as columns, the others are the restatement of the sound samples normalised by the original B."""
    try:
        d, K, B = 64, 1, 65
        u, p = IB.make_batch(B, seed=5)
        u, p = u.copy(), p.copy()
        void = (0, 33, B - 1)
        for i, v_ in enumerate(void):
            if what in ("user", "both"):
                u[v_] = SC.N_USERS + i if i != 1 else -1
            if what in ("pos", "both"):
                p[v_] = SC.M_ITEMS + i if i != 1 else -3
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **_cfg(0.2, "cosine", True))
        share = _judge(pkg, ds, m, (u, p), K, d, "fp32", "propagated", _tau32(0.2), 1, f"void {what}", "cosine", True, void=void)[0]
        assert all(v <= 1.0 for v in share.values()), share
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


def test_voided_samples_in_the_last_part(pkg, storage_graph):
    """test_voided_samples ("both") at B = 513, cosine + logq: the bad ids at row 0, in part 1 (row 300) and in the last part,
    whose only live row (512) is then void."""
    try:
        d, K, B = 64, 1, IB.MANY_PARTS_B
        u, p = IB.make_batch(B, seed=5)
        u, p = u.copy(), p.copy()
        void = (0, 300, B - 1)
        assert IB.last_part_rows(B).tolist() == [B - 1]
        for i, v_ in enumerate(void):
            u[v_] = SC.N_USERS + i if i != 1 else -1
            p[v_] = SC.M_ITEMS + i if i != 1 else -3
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **_cfg(0.2, "cosine", True))
        share = _judge(pkg, ds, m, (u, p), K, d, "fp32", "propagated", _tau32(0.2), 1, f"void both B={B}", "cosine", True, void=void)[0]
        assert all(v <= 1.0 for v in share.values()), share
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("B,score,lq_on", [(33, "cosine", False), (260, "cosine", True), (33, "dot", True)])
def test_one_user_batch_has_no_loss(pkg, storage_graph, B, score, lq_on):
    """Every sample names one user: loss_out[1] is exactly 0.0, every term exactly -0 / 0, and only the regulariser moves rows."""
    try:
        d, K = 32, 2
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **_cfg(0.2, score, lq_on))
        batch = IB.one_user_batch(B)
        share, r, (term, regt, g_rec, slack, bd, out) = _judge(pkg, ds, m, batch, K, d, "fp32", "propagated", _tau32(0.2), 1,
                                                               f"one user B={B} {score} logq{int(lq_on)}", score, lq_on)
        m.check_device_errors()
        assert out[1] == 0.0 and (term == 0.0).all() and float(r["loss_out"][1]) == 0.0 and float(r["W"].abs().max()) == 0.0
        assert all(v <= 1.0 for v in share.values()), share
    finally:
        pkg.world.configure([])


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,d", [("fp32", 260, 64), ("bf16", 100, 256)])
def test_the_same_step_twice_is_bitwise_the_same(pkg, storage_graph, mode, B, d):
    try:
        res = []
        for _ in range(2):
            _, m = _model(pkg, storage_graph, mode, d, 2, batch=B, **_cfg(0.1, "cosine", True))
            outs = [m.fused_step(_dev(u), _dev(p), _dev(u)).clone() for u, p in IB.make_batches(B, 2, seed=9)]
            m.check_device_errors()
            res.append(outs + [m._table.detach().clone(), m._dev['adam_m'].clone(), m._dev['adam_v'].clone(), m._dev['terms'].clone()])
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("mode,K,score,lq_on", [("fp32", 1, "cosine", True), ("bf16", 2, "cosine", False), ("fp32", 2, "dot", True)])
def test_epoch_equals_the_loop_of_steps_bitwise(pkg, storage_graph, mode, K, score, lq_on):
    """lgcn_train_epoch_inbatch over T = 165 (batches of 64, 64, 37) against the loop of lgcn_train_step_inbatch: loss rows, table,
    both Adam moments bit for bit."""
    try:
        B, T, d = 64, 165, 64
        cfg = _cfg(0.2, score, lq_on)
        u, p = IB.make_batch(T, seed=1)
        _, a = _model(pkg, storage_graph, mode, d, K, **cfg)
        want = a.fused_epoch(_dev(u), _dev(p), _dev(u), B)
        a.check_device_errors()
        _, b = _model(pkg, storage_graph, mode, d, K, **cfg)
        first = b._table.detach().clone()
        got = [b.fused_step(_dev(u[t:t + B]), _dev(p[t:t + B]), _dev(u[t:t + B])) for t in range(0, T, B)]
        b.check_device_errors()
        assert a.adam_step == b.adam_step == 3 and want.shape == (3, 3)
        assert torch.equal(torch.stack(got), want), (torch.stack(got), want)
        assert torch.equal(a._table, b._table), int((a._table != b._table).sum())
        assert torch.equal(a._dev['adam_m'], b._dev['adam_m']) and torch.equal(a._dev['adam_v'], b._dev['adam_v'])
        assert not bool(a._dev['G64'].any()) and not bool(b._dev['G64'].any())
        assert float((b._table - first).abs().max()) > 1e-4                 # (it trained)
    finally:
        pkg.world.configure([])


# ---- 4. the defaults are the parent's path; refusals -------------------------------------------------------------------------
@pytest.mark.parametrize("mode,d", [("fp32", 64), ("bf16", 128)])
def test_dot_without_logq_told_or_never_told_is_bitwise_the_same(pkg, storage_graph, mode, d):
    """A context given (LGCN_SCORE_DOT, NULL) explicitly -- after having held (COSINE, lq) -- and a context never told: tables,
    moments and losses bit for bit over three steps."""
    try:
        L = pkg._lib
        lib = L.load()
        B, res = 100, []
        for told in (True, False):
            ds, m = _model(pkg, storage_graph, mode, d, 2, batch=B, loss='inbatch', softmax_temp=0.2)
            st = m._state(max_batch=B, need_ctx=True)
            got = C.c_void_p(5)
            assert lib.lgcn_ctx_get_inbatch_scores(st['ctx'], C.byref(got)) == L.SCORE_DOT and got.value is None
            if told:
                lq = _dev(_logq(ds), torch.float32)
                L.check(lib.lgcn_ctx_set_inbatch_scores(st['ctx'], L.SCORE_COSINE, L.tp(lq)), "set")
                assert lib.lgcn_ctx_get_inbatch_scores(st['ctx'], C.byref(got)) == L.SCORE_COSINE and got.value == lq.data_ptr()
                L.check(lib.lgcn_ctx_set_inbatch_scores(st['ctx'], L.SCORE_DOT, None), "set")
                assert lib.lgcn_ctx_get_inbatch_scores(st['ctx'], C.byref(got)) == L.SCORE_DOT and got.value is None
            outs = [m.fused_step(_dev(u), _dev(p), _dev(u)).clone() for u, p in IB.make_batches(B, 3, seed=4)]
            m.check_device_errors()
            assert m.adam_step == 3
            res.append(outs + [m._table.detach().clone(), st['adam_m'].clone(), st['adam_v'].clone(), st['terms'].clone()])
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


def test_the_options_are_independent_of_set_loss(pkg, storage_graph):
    """The setter before lgcn_ctx_set_loss, on a context whose loss is BPR: accepted and kept; the in-batch entry points still
    refuse until the loss is set, and a BPR step on that context is the step of a context never told."""
    try:
        L = pkg._lib
        lib = L.load()
        res = []
        for told in (True, False):
            ds, m = _model(pkg, storage_graph, "fp32", 64, 2)
            st = m._state(max_batch=64, need_ctx=True)
            u, p = IB.make_batch(64)
            if told:
                lq = _dev(_logq(ds), torch.float32)
                L.check(lib.lgcn_ctx_set_inbatch_scores(st['ctx'], L.SCORE_COSINE, L.tp(lq)), "set")
                loss = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
                assert lib.lgcn_train_step_inbatch(st['ctx'], L.tp(_dev(u)), L.tp(_dev(p)), 64, L.tp(loss), L.current_stream()) == 3
                assert "inbatch" in lib.lgcn_last_error().decode() and bool((loss == -7.0).all())
                assert lib.lgcn_ctx_get_inbatch_scores(st['ctx'], None) == L.SCORE_COSINE
            out = m.fused_step(_dev(u), _dev(p), _dev(p[::-1].copy())).clone()
            m.check_device_errors()
            res.append((out, m._table.detach().clone(), st['adam_m'].clone()))
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


def test_refusals_leave_everything_untouched(pkg, storage_graph):
    try:
        L = pkg._lib
        lib = L.load()
        ds, m = _model(pkg, storage_graph, "fp32", 64, 2, **_cfg(0.2, "cosine", True))
        st = m._state(max_batch=64, need_ctx=True)
        ctx = st['ctx']
        u, p = IB.make_batch(64)
        m.fused_step(_dev(u), _dev(p), _dev(u))
        m.check_device_errors()
        before = _snapshot(lib, m, st)
        other = torch.zeros(SC.M_ITEMS, dtype=torch.float32, device=DEV)
        for kind in (2, -1, 7, 1 << 20):
            rc = lib.lgcn_ctx_set_inbatch_scores(ctx, kind, L.tp(other))
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "score" in msg and "lgcn_ctx_set_inbatch_scores" in msg, (kind, rc, msg)
        rc = lib.lgcn_ctx_set_inbatch_scores(None, L.SCORE_DOT, None)
        assert rc == 3 and "null context" in lib.lgcn_last_error().decode()
        got = C.c_void_p(0)
        assert lib.lgcn_ctx_get_inbatch_scores(ctx, C.byref(got)) == L.SCORE_COSINE and got.value == st['item_logq'].data_ptr()
        torch.cuda.synchronize()
        _same(before, _snapshot(lib, m, st))
        # ... and the same context takes a sound call afterwards, the one a context that saw no refusal takes
        o1 = m.fused_step(_dev(u), _dev(p), _dev(u)).clone()
        m.check_device_errors()
        _, m2 = _model(pkg, storage_graph, "fp32", 64, 2, **_cfg(0.2, "cosine", True))
        m2.fused_step(_dev(u), _dev(p), _dev(u))
        o2 = m2.fused_step(_dev(u), _dev(p), _dev(u)).clone()
        assert torch.equal(o1, o2) and torch.equal(m._table, m2._table)
    finally:
        pkg.world.configure([])


# ---- 5. evaluation ranks what was trained ------------------------------------------------------------------------------------
def test_evaluation_under_cosine(pkg, storage_graph):
    """After two cosine steps: rating_table() is the row-normalised propagated table (memoised, dropped by invalidate_cache),
    getUsersRating is U^ P^^T, and Procedure.Test returns the same recall / ndcg through the fused kernels (--eval_fused 1),
    through the rank-based ones (--rank_metrics 1) and through the torch harness (--eval_fused 0): 1e-6, the tolerance of
    tests/test_gpu_layer_weights.py::test_evaluation_scores_with_the_weighted_table for that comparison."""
    w = pkg.world
    old_topks = list(w.topks)
    try:
        ds, m = _model(pkg, storage_graph, "fp32", 64, 2, **_cfg(0.1, "cosine", True))
        for u, p in IB.make_batches(64, 2, seed=2):
            m.fused_step(_dev(u), _dev(p), _dev(u))
        m.check_device_errors()
        m.eval()
        with torch.no_grad():
            E = m.propagated_table()
            R = m.rating_table()
            assert R is m.rating_table() and R is not E
            ref = IS.unit(E.double().cpu())[0]
            assert float((R.double().cpu() - ref).abs().max()) <= 4 * U
            r = m.getUsersRating(torch.arange(8, device=DEV))
            assert float((r.double().cpu() - ref[:8] @ ref[SC.N_USERS:].t()).abs().max()) <= 1e-6
            m.invalidate_cache()
            assert m._cosine_cache is None and m.rating_table() is not R and torch.equal(m.rating_table(), R)
        assert set(m.state_dict()) == {"embedding_user.weight", "embedding_item.weight"}
        w.topks = [20]
        res = {}
        for name, fused, ranks in (("fused", 1, 0), ("ranks", 1, 1), ("torch", 0, 0)):
            w.config['eval_fused'], w.config['rank_metrics'] = fused, ranks
            res[name] = pkg.Procedure.Test(ds, m, 0)
        print("[inbatch_scores] evaluation under cosine: " + " ".join(f"{n}: recall {float(v['recall'][0]):.6f} ndcg {float(v['ndcg'][0]):.6f}" for n, v in res.items()))
        assert float(res["torch"]["recall"][0]) > 0.0
        for name in ("fused", "ranks"):
            for k in ("recall", "ndcg"):
                assert abs(float(res[name][k][0]) - float(res["torch"][k][0])) < 1e-6, (name, k, res)
        m.check_device_errors()
    finally:
        w.topks = old_topks
        w.config['eval_fused'], w.config['rank_metrics'] = 1, 0
        pkg.world.configure([])

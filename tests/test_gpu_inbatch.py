"""The in-batch sampled softmax in the fused step (--loss inbatch; lgcn_train_step_inbatch, csrc/lgcn_inbatch.hip) on
the GPU (-m gpu), on the graph and table rows of tests/storage_cases.py with the batches of tests/inbatch_restatement.py,
against the float64 restatement in that file.  Every step is judged from the GPU's OWN state before the step.

BOUNDS (u = 2^-24; per element, first order in u; all magnitudes from the restatement; tau below is the fp32 value the library
holds, which the restatement is given).  The forward / slot rows / G, Gs / backward / last link / loss_out lines are those of
tests/test_gpu_softmax.py (same launches, same expressions) and are not repeated here.  New:
  score         s_{b,c} = sum_k U[b][k] P[c][k], a d-term fmaf chain on the fp32-input MFMA (one rounding per term), S_{b,c} =
                sum |u_k p_k|:   delta_s_bc = (d + 1) u S_bc + sum_k (delta_e_u |p| + |u| delta_e_p).
                s_{b,b} is the lane-group dot product of the rows kernel (any order): (d + 2) u S_bb + the operand deltas.
                z_bc = (s_bc - s_bb) / tau, a subtraction and a correctly rounded division:
                delta_z_bc = (delta_s_bc + delta_s_bb) / tau + 2 u |z_bc|.
  normalise     1 + sum_c exp(z_c) = exp(M) (1 + Zm1), M = max(0, max_c z_c).  The kernel keeps a sum as exp(m) (1 + r) and
                moves m upwards only: a term that entered at the running maximum m_1 and was rescaled at m_2 < .. < M carries
                the roundings of the differences z_c - m_1, m_1 - m_2, .., whose absolute sum is |z_c - M| = a_c: u a_c in the
                exponent, as for one shift.  Per term the relative roundings are its own expf (2 u), one per addition it passes
                through and 4 per rescaling event (expf, 1 + r, the product, the addition).  The tiling (LGCN_INBATCH_PART_TILES
                = 8 tiles of 32 rows per part, 16 rows per lane and tile) gives at most 16 * 8 = 128 additions in the lane, 1
                for the other lane half, NP for the parts (NP = ceil(ceil(B / 32) / 8), merged in ascending order) and 1 for
                the positive's term: 130 + NP additions; and at most 8 + 1 + NP + 1 rescaling events:
                kZ = 2 + (130 + NP) + 4 (10 + NP) = 172 + 5 NP    (182 at B = 260, NP = 2; 177 below).
                With q_c = exp(z_c - M) / Z, q_0 = exp(-M) / Z (evaluated only where M > 0: where M = 0 the kernel's Zm1 =
                expf(m) (1 + r) never adds the positive's 1, so every rounding sits on Zm1 itself),
                P = sum q_c + [M > 0] q_0 <= 1:
                rho = delta_Z / Z = kZ u P + sum_c q_c (delta_z_c + u a_c)
                delta_l = rho + 2 u log1p(Zm1) + u |l| <= rho + 3 u l                       (terms[b] = -l)
                Where M = 0, P = Q <= l (1 + l), so the bound is RELATIVE to a tiny l: l (kZ u + 3 u) + sum q_c (delta_z_c + u a_c).
                delta_q_c = q_c (4 u + delta_z_c + u a_c + rho) + 2^-140          (expf, the division, 1 + Zm1; subnormal results)
                Q = S / (S + e_0) with S the competitors' sum: |dQ| <= Q (dS / S + de_0 / e_0), so
                delta_Q = Q (kZ + 6) u + sum_c q_c (delta_z_c + u a_c) + 2^-140.
  W             W_bc = q_bc * fl(1 / (tau B)): delta_W = 2 u |W| + delta_q / (tau B); the diagonal likewise from delta_Q.
  g_u, g_p      g_{u_b} = sum_c W_bc e_{p_c} (+ the diagonal term, + lam e_u), g_{p_c} = sum_b W_bc e_{u_b} (+ ..): per part an
                fmaf chain of at most n = min(Bp, 256) terms on the MFMA, the parts added in fixed point (exact, 2^-51 each,
                NP + 2 adds per row with the diagonal and lam terms).  In any order:
                delta_g = (n + 1) u sum |W| |e| + sum (delta_W |e| + |W| delta_e) + 2 u |W_bb| |e| + 6 u lam |e| + lam delta_e
                          + (NP + 2) 2^-51.
  reg term      two sums of squares: 2 CPT roundings each in the lane (CPT = d / min(d, 64)), one addition, 6 in the lane-group
                sum: delta_reg = (4 CPT + 12) u regterm + 2 sum |e| delta_e               (reg_ego: delta_e = 0).
  reg_ego       the last launch adds fl(decay / B) cnt E0 (cnt = 1 per slot): 4 u of it and 2 u of the sum.
Every test prints the largest share of each bound it used (recorded in profiles/inbatch/README.md)."""
import os

import numpy as np
import pytest
import torch

import inbatch_restatement as IB
import multineg_restatement as MN
import storage_cases as SC
import storage_restatement as S
from conftest import spmm_sum_bound
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)
from test_gpu_gate_shapes import W1, _adam_checks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = SC.U
_G = {}


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _tau32(tau):
    return float(np.float32(tau))


def _model(pkg, path, mode, d, K, reg="propagated", dl=1, batch=64, **cfg):
    """A fresh GPU model of the storage graph (seed SC.MODEL_SEED, hand-set rows); cfg goes into world.config first."""
    w = SC.configure(pkg, (mode, d, K, dl, -1, reg), path, batch)
    w.config.update(cfg)
    ds = pkg.dataloader.Loader(w.config, path=path)
    pkg.utils.set_seed(SC.MODEL_SEED)
    m = pkg.model.LightGCN(w.config, ds)
    SC.set_rows(m._table)
    m = m.to(DEV)
    m.train()
    if "adj" not in _G:
        _G["adj"] = ds.getSparseGraphCSR()
        _G["A"] = S.dense_adj(_G["adj"])
    return ds, m


def _state(m):
    st = m._dev
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in (("table", m._table), ("M", st['adam_m']), ("V", st['adam_v']))}


def _c(n):
    return int(np.ceil(n / 64.0)) + 8


def _parts(B):
    return (((B + 31) // 32) + 7) // 8


def _drop_matrices(pkg, m, keep, step):
    """(A_drop, A_drop^T) of the step whose counter stands at `step` before it, as scipy float64 CSR, from the exported mask
    (lgcn_dropout_mask on the CSR of A_hat itself: the mask is a function of (row, column))."""
    import scipy.sparse as sp
    L = pkg._lib
    adj = _G["adj"]
    out = torch.full((adj.nnz,), 7, dtype=torch.uint8, device=DEV)
    ip, ix = _dev(adj.indptr.astype(np.int32)), _dev(adj.indices.astype(np.int32))
    L.check(L.load().lgcn_dropout_mask(L.tp(ip), L.tp(ix), adj.shape[0], adj.nnz, keep, int(m.config.get('seed', 2020)), step, L.tp(out),
                                       L.current_stream()), "lgcn_dropout_mask")
    mk = out.cpu().numpy().astype(np.float64)
    assert np.isin(mk, (0.0, 1.0)).all() and 0.0 < mk.mean() < 1.0
    A64 = sp.csr_matrix((adj.data.astype(np.float64), adj.indices, adj.indptr), shape=adj.shape)
    M = sp.csr_matrix((mk, adj.indices, adj.indptr), shape=adj.shape)
    fwd = (A64.multiply(M).tocsr() / keep).tocsr()
    return fwd, fwd.T.tocsr()


def _bounds(r, batch, B, K, d, mode, ego, w, tau, fwd=None, bwd=None):
    """The bounds of the module docstring from a restatement r of the sound samples `batch` of a step normalised by B ->
    dict: term, regterm [b], loss (3), g_final [N, d].  fwd / bwd: scipy CSR of the forward / backward matrix (default A_hat)."""
    adj = _G["adj"]
    extra = 2 if fwd is None else 4
    fwd = adj.astype(np.float64) if fwd is None else fwd
    bwd = fwd if bwd is None else bwd
    af, ab = abs(fwd).tocsr(), abs(bwd).tocsr()
    wk = MN.layer_weights(K, w)
    E0 = r["E0"].numpy()
    # ---- forward tables and slot rows (tests/test_gpu_softmax.py)
    X = E0
    T = abs(wk[0]) * np.abs(E0)
    dX = SC.stored_bound(E0, 0.0, "bf16") if (mode == "bf16" and K >= 2) else np.zeros_like(E0)     # the input of layer 1
    dE = np.zeros_like(E0)
    for k in range(1, K + 1):
        pre = af @ dX + spmm_sum_bound(af.indptr, af.data, af.indices, np.abs(X) + dX, extra_terms=extra)
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
    # ---- scores
    Sabs = au @ ap.T
    opd = du @ ap.T + au @ dp.T
    ds = (d + 1) * U * Sabs + opd
    dsbb = (d + 2) * U * np.diag(Sabs) + np.diag(opd)
    keep = r["keep"].numpy()
    z = np.where(keep, r["z"].numpy(), 0.0)
    mm, q, l, Q = r["m"].numpy(), r["q"].numpy(), r["lterm"].numpy(), r["Q"].numpy()
    dz = np.where(keep, (ds + dsbb[:, None]) / tau + 2 * U * np.abs(z), 0.0)
    a = np.where(keep, np.abs(z - mm[:, None]), 0.0)
    q0 = np.where(mm > 0, 1.0 - Q, 0.0)                                    # exp(-M) / Z = 1 - Q, counted only where M > 0
    P = np.minimum(Q + q0, 1.0)                                             # (as tests/test_gpu_softmax.py: P = Q where M = 0)
    qd = (q * (dz + U * a)).sum(1)
    rho = kZ * U * P + qd
    out = {"term": rho + 3 * U * l + 1e-37}
    dq = np.where(keep, q * (4 * U + dz + U * a + rho[:, None]) + 2.0 ** -140, 0.0)
    dQ = Q * (kZ + 6) * U + qd + 2.0 ** -140 * (Q > 0)
    itb = 1.0 / (tau * B)
    Wabs = q * itb                                                          # off the diagonal (q = 0 on it and outside A_b)
    dW = 2 * U * Wabs + dq * itb
    Wd = Q * itb
    dWd = 2 * U * Wd + dQ * itb
    # ---- reg term
    CPT = d // min(d, 64)
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
    # ---- backward chain: the float64 values v_i of the launches and their bounds (tests/test_gpu_softmax.py)
    cw = [abs(x) * div for x in wk]                                       # the chain on Gs: mean 1, 1, ..; weights w_k
    v = cw[K] * (Gref / div)
    h, dh = np.abs(v), cw[K] * dGs + (U * cw[K] * Gs if w is not None else 0.0)
    D = dh
    for i in range(K):
        k = K - i
        Ah = ab @ h
        D = cw[k - 1] * dGs + ab @ dh + spmm_sum_bound(ab.indptr, ab.data, ab.indices, h + dh, extra_terms=extra) + 2 * U * (cw[k - 1] * Gs + Ah)
        v = (wk[k - 1] * div) * (Gref / div) + bwd @ v
        if i < K - 1 and mode == "bf16":
            D = SC.stored_bound(v, D, "bf16")
        h, dh = np.abs(v), D
    if ego:
        D = D + 4 * U * (SC.DECAY / B) * r["cnt"].numpy()[:, None] * np.abs(E0) + 2 * U * np.abs(r["g_final"].numpy())
    out["g_final"] = D
    return out


def _judge(pkg, m, batch, K, d, mode, reg, tau, step_no, tag, w=None, keep=None, void=()):
    """One fused step from the GPU's own state -> {link: share of its bound}.  void: indices of the samples whose ids are bad in
    `batch`: their terms must be zero and the step is the restatement of the sound samples with B_norm = B."""
    A = _G["A"]
    ego = reg == "ego"
    B = len(batch[0])
    m._state(max_batch=max(B, int(m.config.get('bpr_batch_size', B))), need_ctx=True)      # (the context fused_step would make)
    assert m.adam_step == step_no - 1
    before = _state(m)
    fwd = bwd = None
    Af, Ab = A, None
    if keep is not None:
        fwd, bwd = _drop_matrices(pkg, m, keep, step_no - 1)
        Af, Ab = torch.from_numpy(fwd.toarray()), torch.from_numpy(bwd.toarray())
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
    r = IB.step(Af, SC.N_USERS, K, SC.DECAY, tau, before["table"], sb, ego, w, B_norm=B, A_bwd=Ab)
    bd = _bounds(r, sb, B, K, d, mode, ego, w, tau, fwd, bwd)
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
    print(f"[inbatch] {tag}: shares " + " ".join(f"{k}={v:.3f}" for k, v in share.items()))
    return share, r, (term, regt, g_rec, slack, bd, out)


def _run(pkg, path, mode, d, K, B, tau, reg="propagated", w=None, keep=None, batches=None):
    try:
        cfg = {'loss': 'inbatch', 'softmax_temp': tau}
        if w is not None:
            cfg['layer_weights'] = str(list(w))
        if keep is not None:
            cfg.update({'dropout': 1, 'keep_prob': keep, 'seed': 2020})
        _, m = _model(pkg, path, mode, d, K, reg, dl=0, batch=B, **cfg)      # --dense_last 0: _make_ctx must force the dense last layer
        top, bad = {}, []
        for i, batch in enumerate(batches or IB.make_batches(B, 3, seed=d + K)):
            tag = f"{mode} d{d} K{K} tau{tau} {reg}" + (" wts" if w is not None else "") + (f" keep{keep}" if keep else "") + f" step {i + 1} B={len(batch[0])}"
            share = _judge(pkg, m, batch, K, d, mode, reg, _tau32(tau), i + 1, tag, w=w, keep=keep)[0]
            for k_, v in share.items():
                top[k_] = max(top.get(k_, 0.0), v)
                if not v <= 1.0:
                    bad.append((tag, k_, v))
            m.check_device_errors()
            assert not bool(m._dev['G64'].any()) and m.adam_step == i + 1
        assert m._dev['dense_last'] is True
        lib = pkg._lib.load()
        assert lib.lgcn_ctx_get_loss(m._dev['ctx'], None) == pkg._lib.LOSS_INBATCH
        print(f"[inbatch] {mode} d{d} K{K} B{B} tau{tau} {reg} TOP: " + " ".join(f"{k_}={v:.3f}" for k_, v in top.items()))
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
    finally:
        pkg.world.configure([])


# ---- 1. three steps against the float64 restatement ------------------------------------------------------------------------
_BS, _DS, _KS, _MS, _RS, _TS = IB.BATCH_SIZES, (32, 64, 128, 256), (1, 2, 3), ("fp32", "bf16"), ("propagated", "ego"), (1.0, 0.2)


def _cases():
    """Not the full product: every value of every axis meets at least two values of each other axis (checked below).
    B = 260 is IB.SPLIT_B: 9 tiles, more than the LGCN_INBATCH_PART_TILES = 8 of one part of the sweep."""
    out = []
    for i, B in enumerate(_BS):
        for s in (0, 1, 2):
            out.append((B, _DS[(i + s) % 4], _KS[(i + 2 * s + i // 3) % 3], _MS[(i // 2 + s) % 2], _RS[(i + s // 2 + i // 4) % 2],
                        _TS[(i // 4 + s) % 2]))
    return out


def _uncovered(cs):
    axes = list(zip(*cs))
    return [(a, v, b) for a in range(len(axes)) for b in range(len(axes)) if a != b for v in set(axes[a])
            if len({c[b] for c in cs if c[a] == v}) < 2]


assert not _uncovered(_cases()), _uncovered(_cases())
assert all({c[a] for c in _cases()} == set(ax) for a, ax in enumerate((_BS, _DS, _KS, _MS, _RS, _TS)))


@pytest.mark.parametrize("B,d,K,mode,reg,tau", [pytest.param(*c, id=f"B{c[0]}-d{c[1]}-K{c[2]}-{c[3]}-{c[4]}-tau{c[5]}") for c in _cases()])
def test_steps_equal_the_restatement(pkg, storage_graph, B, d, K, mode, reg, tau):
    """Per-sample terms, loss_out, the gradient recovered from Adam's first moment and Adam itself, each within the bound derived
    in the module docstring, over three consecutive batches of B samples."""
    _run(pkg, storage_graph, mode, d, K, B, tau, reg)


# ---- 1b. the batch sizes the loss is trained and timed at ----------------------------------------------------------------------
# IB.LARGE_BATCH_SIZES: 513 = 17 tiles = three parts of the sweep, the third a single tile with one live row; 2048 = the default
# --bpr_batch, eight full parts.  No batch of section 1 has more than two parts, so the merge loop of k_inbatch_diag over the
# parts, the blockIdx.y extent of k_inbatch_norm / k_inbatch_grad beyond 2 and the addressing part + (by * Bp + b) * 2 for by >= 2
# run here first.  The bounds are section 1's, unchanged: every line is a function of B through NP (kZ, the fixed-point line),
# n = min(Bp, 256) (the chain of one part) and c(B) (the loss reduction: ceil(B / 64) = 32 additions in the lane at 2048).
# Together with tests/test_gpu_inbatch_scores.py (the other three score options) every width stands twice among the in-batch
# cases of these sizes; two steps per case: the float64 restatement decides the time.
LARGE_STEPS = 2
_LARGE_CASES = [
    (513, 32, 1, 'fp32', 'ego', 0.2),
    (513, 128, 3, 'bf16', 'propagated', 1.0),
    (2048, 64, 3, 'bf16', 'ego', 1.0),
    (2048, 256, 1, 'fp32', 'propagated', 0.2),
]


def large_batches(B, d, K):
    return IB.make_batches(B, LARGE_STEPS, seed=d + K)


def check_large_cases(cases, batches_of):
    """What a list of (B, d, K, mode, reg, ..) cases at the large sizes must reach (asserted at import, without a device)."""
    assert {c[0] for c in cases} == set(IB.LARGE_BATCH_SIZES)
    assert {_parts(c[0]) for c in cases} >= {3, 8}
    assert all(any(_parts(c[0]) >= 3 and ok(c[1]) for c in cases) for ok in (lambda d: d <= 64, lambda d: d >= 128))
    assert {c[2] for c in cases} == {1, 3} and {c[3] for c in cases} == {"fp32", "bf16"}
    assert {c[4] for c in cases if c[0] >= IB.MANY_PARTS_B} == {"propagated", "ego"}
    for c in cases:
        for u, p in (b[:2] for b in batches_of(c)):
            B, last = len(u), IB.last_part_rows(len(u))
            assert B == c[0] and IB.kept_share(u, p) > 0.5, (c, IB.kept_share(u, p))
            assert last[0] >= IB.PART_ROWS and u[B - 1] in u[:IB.PART_ROWS] and p[B - 1] in p[:IB.PART_ROWS]      # across parts


check_large_cases(_LARGE_CASES, lambda c: large_batches(c[0], c[1], c[2]))


@pytest.mark.parametrize("B,d,K,mode,reg,tau", [pytest.param(*c, id=f"B{c[0]}-d{c[1]}-K{c[2]}-{c[3]}-{c[4]}-tau{c[5]}") for c in _LARGE_CASES])
def test_steps_equal_the_restatement_at_the_training_batch_sizes(pkg, storage_graph, B, d, K, mode, reg, tau):
    """Section 1 at B = 513 and B = 2048 (three and eight parts of the sweep): per-sample terms, loss_out, the gradient recovered
    from Adam's first moment and Adam itself within the same derived bounds, over two consecutive batches that repeat a user and
    a positive across parts (rows 0..255 / the last part)."""
    _run(pkg, storage_graph, mode, d, K, B, tau, reg, batches=large_batches(B, d, K))


# ---- 2. masks and voids ------------------------------------------------------------------------------------------------------
def test_duplicates_inside_one_tile_and_across_tiles(pkg, storage_graph):
    """The batch of 65 (three tiles): the same user and the same positive inside tile 0, across tiles 0 / 1 and 0 / 2."""
    u, p = IB.make_batch(65, seed=3)
    keep = IB.competitors(u, p).numpy()
    assert not keep[0, 1] and not keep[4, 5] and not keep[2, 40] and not keep[15, 50] and not keep[16, 64] and not keep[17, 64]
    assert keep[20, 21] and keep[20, 64]
    _run(pkg, storage_graph, "fp32", 64, 2, 65, 0.2, batches=[(u, p)])


@pytest.mark.parametrize("B", [33, 260])
def test_one_user_batch_has_no_loss(pkg, storage_graph, B):
    """Every sample names one user: loss_out[1] is exactly 0.0, every term exactly -0 / 0, and only the regulariser moves rows."""
    try:
        d, K = 32, 2
        _, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, loss='inbatch', softmax_temp=0.2)
        batch = IB.one_user_batch(B)
        share, r, (term, regt, g_rec, slack, bd, out) = _judge(pkg, m, batch, K, d, "fp32", "propagated", _tau32(0.2), 1, f"one user B={B}")
        m.check_device_errors()
        assert out[1] == 0.0 and (term == 0.0).all() and float(r["loss_out"][1]) == 0.0
        assert all(v <= 1.0 for v in share.values()), share
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("what", ["user", "pos", "both"])
def test_voided_samples(pkg, storage_graph, what):
    """An out-of-range user, positive, or both, at the first, a middle and the last position of a batch of 65 (the last one alone
    in its tile): err is set, the samples are void as rows and as columns, the others are the restatement of the sound samples
    normalised by the original B."""
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
        _, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, loss='inbatch', softmax_temp=0.2)
        share = _judge(pkg, m, (u, p), K, d, "fp32", "propagated", _tau32(0.2), 1, f"void {what}", void=void)[0]
        assert all(v <= 1.0 for v in share.values()), share
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("what", ["user", "pos", "both"])
def test_voided_samples_in_the_last_part(pkg, storage_graph, what):
    """test_voided_samples at B = 513: the bad ids at row 0, in part 1 (row 300) and in the last part, whose only live row (512) is
    then void -- a part with no sound sample at all.  The samples are void as rows and as columns of every part."""
    try:
        d, K, B = 64, 1, IB.MANY_PARTS_B
        u, p = IB.make_batch(B, seed=5)
        u, p = u.copy(), p.copy()
        void = (0, 300, B - 1)
        assert IB.last_part_rows(B).tolist() == [B - 1]
        for i, v_ in enumerate(void):
            if what in ("user", "both"):
                u[v_] = SC.N_USERS + i if i != 1 else -1
            if what in ("pos", "both"):
                p[v_] = SC.M_ITEMS + i if i != 1 else -3
        _, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, loss='inbatch', softmax_temp=0.2)
        share = _judge(pkg, m, (u, p), K, d, "fp32", "propagated", _tau32(0.2), 1, f"void {what} B={B}", void=void)[0]
        assert all(v <= 1.0 for v in share.values()), share
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


# ---- 3. the saturation batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_saturation_batch(pkg, storage_graph, mode):
    """tests/test_inbatch_host.py::test_saturation_batch_exists: z beyond +100 and a sample with all z below -100 (tau = 0.05,
    d = 256, K = 1).  Every output is finite, terms and the recovered gradient lie within the derived bounds -- the bound of a
    term is relative to l where l is tiny, and q is one-hot within delta_q where one competitor dominates."""
    try:
        d, K, tau = IB.SAT_D, IB.SAT_K, IB.SAT_TAU
        _, m = _model(pkg, storage_graph, mode, d, K, loss='inbatch', softmax_temp=tau, batch=40)
        E = IB.propagate(_G["A"], torch.from_numpy(m._table.cpu().numpy().astype(np.float64)), K).numpy()
        batch = IB.saturation_batch(E)
        share, r, (term, regt, g_rec, slack, bd, out) = _judge(pkg, m, batch, K, d, mode, "propagated", _tau32(tau), 1, f"saturation {mode}")
        m.check_device_errors()
        z, keep, q = r["z"].numpy(), r["keep"].numpy(), r["q"].numpy()
        assert (z[keep] > 100.0).any() and (np.where(keep, z, -np.inf) < -100.0).all(1).any()
        assert np.isfinite(m._table.cpu().numpy()).all() and np.isfinite(term).all() and np.isfinite(out).all()
        assert all(v <= 1.0 for v in share.values()), share
        dead = np.where((np.where(keep, z, -np.inf) < -100.0).all(1))[0]      # all competitors dominated: l underflows
        assert len(dead) >= 1
        for b in dead:                                                        # (a tiny NON-zero l: test_tiny_loss_term_keeps_its_relative_accuracy)
            assert abs(term[b]) <= 2.0 ** -126 and abs(term[b] - float(r["term"][b])) <= bd["term"][b]
        # q one-hot on the DEVICE: sample 0 (distinct ids: its user row is named by this slot alone) is dominated by column 2, so
        # the step's gradient on that row is what W[0,2] = 1 / (tau B) = -W[0,0] gives, within the bound (K = 1: g = (G + A G) / 2)
        u_, p_ = IB.as_samples(batch)
        B, row = len(u_), int(u_[0])
        assert float(q[0, 2]) > 1.0 - 1e-9 and (u_ == row).sum() == 1
        tb = _tau32(tau) * B
        g_onehot = (r["e_p"][2] - r["e_p"][0]).numpy() / tb + (SC.DECAY / B) * r["e_u"][0].numpy()
        assert float(np.abs(r["G"][row].numpy() - g_onehot).max()) <= 1e-9 * float(np.abs(g_onehot).max())
        want = 0.5 * (g_onehot + (_G["A"] @ r["G"])[row].numpy())
        one_hot_share = float((np.abs(g_rec[row] - want) / (bd["g_final"][row] + slack[row] + 1e-300)).max())
        print(f"[inbatch] saturation {mode}: one-hot gradient row share {one_hot_share:.3f}")
        assert one_hot_share <= 1.0
    finally:
        pkg.world.configure([])


def test_tiny_loss_term_keeps_its_relative_accuracy(pkg, storage_graph):
    """tests/test_inbatch_host.py::test_tiny_l_batch_exists: sample 2 has every z near -30, so l_2 is about 4e-12 -- far below
    u = 6e-8, non-zero, a normal fp32 number -- and M_2 = 0.  Its bound (module docstring, M = 0) is relative to l: asserted to be
    below 1e-2 l (d = 256: delta_z is a few 1e-4 in fp32), and the device's term must lie within it.  A logf(1 + Zm1), or a sum
    that has the positive's 1 added to it, returns 0 or a multiple of u here.  fp32 storage only: with bf16 rows delta_z = delta_s /
    tau is no longer small against 1 at |z| = 30, and a first-order bound of exp is not a statement about l any more."""
    try:
        d, K = IB.SAT_D, IB.SAT_K
        _, m = _model(pkg, storage_graph, "fp32", d, K, loss='inbatch', softmax_temp=1.0, batch=40)
        E = IB.propagate(_G["A"], torch.from_numpy(m._table.cpu().numpy().astype(np.float64)), K).numpy()
        u, p, tau = IB.tiny_l_batch(E)
        tau = _tau32(tau)
        m.softmax_temp = tau                     # (read when the context is made, which _judge does)
        share, r, (term, regt, g_rec, slack, bd, out) = _judge(pkg, m, (u, p), K, d, "fp32", "propagated", tau, 1, "tiny l")
        m.check_device_errors()
        import ctypes as C
        t_ = C.c_float(0.0)
        assert pkg._lib.load().lgcn_ctx_get_loss(m._dev['ctx'], C.byref(t_)) == pkg._lib.LOSS_INBATCH and t_.value == np.float32(tau)
        l2, b2 = float(r["lterm"][2]), float(bd["term"][2])
        rel = abs(-term[2] - l2) / l2
        print(f"[inbatch] tiny l: l_2 = {l2:.3e}, device {-term[2]:.3e}, relative error {rel:.2e}, relative bound {b2 / l2:.2e}, share {abs(-term[2] - l2) / b2:.3f}")
        assert 2.0 ** -100 < l2 < 1e-6 and float(r["m"][2]) == 0.0
        assert b2 <= 1e-2 * l2 and abs(-term[2] - l2) <= b2
        assert all(v <= 1.0 for v in share.values()), share
    finally:
        pkg.world.configure([])


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B", [("fp32", 260), ("bf16", 100)])
def test_the_same_step_twice_is_bitwise_the_same(pkg, storage_graph, mode, B):
    try:
        res = []
        for _ in range(2):
            _, m = _model(pkg, storage_graph, mode, 64, 2, batch=B, loss='inbatch', softmax_temp=0.2)
            outs = [m.fused_step(_dev(u), _dev(p), _dev(u)).clone() for u, p in IB.make_batches(B, 2, seed=9)]
            m.check_device_errors()
            res.append(outs + [m._table.detach().clone(), m._dev['adam_m'].clone(), m._dev['adam_v'].clone(), m._dev['terms'].clone()])
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


# ---- 5. composition ----------------------------------------------------------------------------------------------------------
def test_steps_with_layer_weights(pkg, storage_graph):
    _run(pkg, storage_graph, "fp32", 128, 3, 65, 1.0, w=[0.4, 0.1, 0.3, 0.2])


def test_steps_with_edge_dropout(pkg, storage_graph):
    """keep 0.8: the restatement runs on A_drop (forward) and A_drop^T (backward) of each step, from the exported mask."""
    _run(pkg, storage_graph, "fp32", 64, 2, 65, 1.0, keep=0.8)


def test_steps_with_reg_rows_ego(pkg, storage_graph):
    """reg_ego: one count per slot with decay / B in the epilogue."""
    _run(pkg, storage_graph, "bf16", 64, 2, 100, 0.2, reg="ego")


# ---- 6. lifecycle and refusals -----------------------------------------------------------------------------------------------
def _snapshot(lib, m, st):
    return (m._table.detach().clone(), st['adam_m'].clone(), st['adam_v'].clone(), int(lib.lgcn_ctx_get_step(st['ctx'])),
            st['G64'].clone(), st['terms'].clone())


def _same(before, after):
    for a, b in zip(before, after):
        assert (a == b) if isinstance(a, int) else torch.equal(a, b)


def test_loss_bpr_after_inbatch_is_the_parents_path(pkg, storage_graph):
    """set INBATCH -> an in-batch step -> set BPR on one context; a context never told otherwise runs a BPR multi step in place of
    the in-batch one (so that both stand at the same step count).  From equal tables onwards a three-slot step and a multi step
    are bit for bit the same on both; lgcn_ctx_get_loss reports kind and temperature."""
    import ctypes as C
    try:
        L = pkg._lib
        lib = L.load()
        d, K, R = 64, 2, 5
        u, p, n = MN.make_batches(d, K, R)[0]
        B = len(u)
        res = []
        for told in (True, False):
            _, m = _model(pkg, storage_graph, "fp32", d, K, neg_ratio=R)
            st = m._state(max_batch=64, need_ctx=True)
            ctx = st['ctx']
            tau = C.c_float(-1.0)
            assert lib.lgcn_ctx_get_loss(ctx, C.byref(tau)) == L.LOSS_BPR and tau.value == 1.0
            loss = torch.zeros(3, dtype=torch.float32, device=DEV)
            du_, dp_ = _dev(u), _dev(p)
            if told:
                L.check(lib.lgcn_ctx_set_loss(ctx, L.LOSS_INBATCH, 0.25), "set_loss")
                assert lib.lgcn_ctx_get_loss(ctx, C.byref(tau)) == L.LOSS_INBATCH and tau.value == 0.25
                L.check(lib.lgcn_train_step_inbatch(ctx, L.tp(du_), L.tp(dp_), B, L.tp(loss), L.current_stream()), "inbatch")
                torch.cuda.synchronize()
                assert bool(torch.isfinite(loss).all()) and float(loss[1]) > 0.0
                L.check(lib.lgcn_ctx_set_loss(ctx, L.LOSS_BPR, float("nan")), "set_loss")
                assert lib.lgcn_ctx_get_loss(ctx, C.byref(tau)) == L.LOSS_BPR and tau.value == 1.0
            else:
                m.fused_step(du_, dp_, _dev(n))
            m.check_device_errors()
            assert m.adam_step == 1 and not bool(st['G64'].any())
            # the same state on both from here: the told context's tables are overwritten with the other's start
            res.append((m, st))
        (ma, sa), (mb, sb) = res
        for key in ('adam_m', 'adam_v'):
            sa[key].copy_(sb[key])
        ma._table.data.copy_(mb._table.data)
        outs = []
        for m in (ma, mb):
            o1 = m.fused_step(_dev(u), _dev(p), _dev(n)).clone()
            o2 = m.fused_step(_dev(u), _dev(p), _dev(n[:, 0])).clone()          # the three-slot step (lgcn_train_step)
            m.check_device_errors()
            assert m.adam_step == 3
            outs.append((o1, o2, m._table.detach().clone(), m._dev['adam_m'].clone(), m._dev['adam_v'].clone()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


def test_refusals_leave_everything_untouched(pkg, storage_graph):
    import ctypes as C
    try:
        L = pkg._lib
        lib = L.load()
        B = 8
        u = _dev(np.arange(B)); p = _dev(np.arange(B)); n = _dev(np.arange(B) + 1)
        u64, p64, n64 = (t.long() for t in (u, p, n))
        scratch = torch.full((3 * 64,), -5, dtype=torch.int32, device=DEV)
        loss = torch.full((6,), -7.0, dtype=torch.float32, device=DEV)
        stream = L.current_stream()
        # (a) while inbatch is set, every other training entry point
        _, m = _model(pkg, storage_graph, "fp32", 64, 2, loss='inbatch', softmax_temp=0.5)
        st = m._state(max_batch=64, need_ctx=True)
        ctx = st['ctx']
        before = _snapshot(lib, m, st)
        calls = {
            "lgcn_train_step": lambda: lib.lgcn_train_step(ctx, L.tp(u), L.tp(p), L.tp(n), B, L.tp(loss), stream),
            "lgcn_train_step_i64": lambda: lib.lgcn_train_step_i64(ctx, L.tp(u64), L.tp(p64), L.tp(n64), B, L.tp(scratch), L.tp(loss), stream),
            "lgcn_train_epoch": lambda: lib.lgcn_train_epoch(ctx, L.tp(u), L.tp(p), L.tp(n), B, B, L.tp(loss), stream),
            "lgcn_train_step_multi": lambda: lib.lgcn_train_step_multi(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, B, L.tp(loss), stream),
            "lgcn_train_epoch_multi": lambda: lib.lgcn_train_epoch_multi(ctx, L.tp(u), L.tp(p), L.tp(n), 1, B, B, L.tp(loss), stream),
            "lgcn_train_step_dp_part1": lambda: lib.lgcn_train_step_dp_part1(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, 0, stream),
            "lgcn_train_step_dp_dense_part1": lambda: lib.lgcn_train_step_dp_dense_part1(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, 0, stream),
            "lgcn_train_step_dp_part2": lambda: lib.lgcn_train_step_dp_part2(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, None, L.tp(loss), stream),
            "lgcn_train_step_cols_part1": lambda: lib.lgcn_train_step_cols_part1(ctx, L.tp(u), L.tp(p), L.tp(n), B, None, stream),
            "lgcn_train_step_cols_part2": lambda: lib.lgcn_train_step_cols_part2(ctx, L.tp(u), L.tp(p), L.tp(n), B, L.tp(loss), stream),
            "lgcn_rs_phase": lambda: lib.lgcn_rs_phase(ctx, 0, 1, L.tp(u), L.tp(p), L.tp(n), B, 1, 0, None, L.tp(loss), stream),
            "lgcn_train_epoch_dp": lambda: lib.lgcn_train_epoch_dp(ctx, None, L.tp(u), L.tp(p), L.tp(n), B, B, 0, None, None, L.tp(loss), stream),
        }
        for name, call in calls.items():
            rc = call()
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "inbatch" in msg and name in msg, (name, rc, msg)
        # (b) the in-batch entry points: B out of range, null pointers
        for name, call in {
            "B=0": lambda: lib.lgcn_train_step_inbatch(ctx, L.tp(u), L.tp(p), 0, L.tp(loss), stream),
            "B>max": lambda: lib.lgcn_train_step_inbatch(ctx, L.tp(u), L.tp(p), 65, L.tp(loss), stream),
            "null users": lambda: lib.lgcn_train_step_inbatch(ctx, None, L.tp(p), B, L.tp(loss), stream),
            "null pos": lambda: lib.lgcn_train_step_inbatch(ctx, L.tp(u), None, B, L.tp(loss), stream),
            "null loss": lambda: lib.lgcn_train_step_inbatch(ctx, L.tp(u), L.tp(p), B, None, stream),
            "epoch B>max": lambda: lib.lgcn_train_epoch_inbatch(ctx, L.tp(u), L.tp(p), B, 65, L.tp(loss), stream),
            "epoch null": lambda: lib.lgcn_train_epoch_inbatch(ctx, L.tp(u), None, B, 4, L.tp(loss), stream),
        }.items():
            rc = call()
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "inbatch" in msg, (name, rc, msg)
        # (c) a temperature that is no temperature, an unknown kind: refused, the loss in force stays
        for kind, tau in ((L.LOSS_INBATCH, 0.0), (L.LOSS_INBATCH, -1.0), (L.LOSS_INBATCH, float("nan")), (L.LOSS_INBATCH, float("inf")), (7, 1.0), (3, 1.0)):
            rc = lib.lgcn_ctx_set_loss(ctx, kind, tau)
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and ("inbatch" in msg or "loss" in msg), (kind, tau, rc, msg)
        t_ = C.c_float(0.0)
        assert lib.lgcn_ctx_get_loss(ctx, C.byref(t_)) == L.LOSS_INBATCH and t_.value == 0.5
        torch.cuda.synchronize()
        _same(before, _snapshot(lib, m, st))
        assert bool((loss == -7.0).all()) and bool((scratch == -5).all())
        # ... and the same context takes a sound call afterwards
        bu, bp = IB.make_batch(64)
        out = m.fused_step(_dev(bu), _dev(bp), _dev(bu))
        m.check_device_errors()
        assert bool(torch.isfinite(out).all()) and m.adam_step == 1
        # (d) the in-batch entry points on a context whose loss is not set (bpr, softmax)
        for cfg in ({}, {'loss': 'softmax', 'softmax_temp': 0.5}):
            _, mo = _model(pkg, storage_graph, "fp32", 64, 2, **cfg)
            so = mo._state(max_batch=64, need_ctx=True)
            b0 = _snapshot(lib, mo, so)
            for name, call in (("lgcn_train_step_inbatch", lambda: lib.lgcn_train_step_inbatch(so['ctx'], L.tp(u), L.tp(p), B, L.tp(loss), stream)),
                               ("lgcn_train_epoch_inbatch", lambda: lib.lgcn_train_epoch_inbatch(so['ctx'], L.tp(u), L.tp(p), B, 4, L.tp(loss), stream))):
                rc = call()
                msg = lib.lgcn_last_error().decode()
                assert rc == 3 and "inbatch" in msg and name in msg, (name, rc, msg)
            torch.cuda.synchronize()
            _same(b0, _snapshot(lib, mo, so))
        # (e) contexts that cannot run it: fp8 storage, dense_last = 0
        for mode, dl in (("fp8", 1), ("fp32", 0)):
            _, mo = _model(pkg, storage_graph, mode, 64, 2, dl=dl)
            so = mo._state(max_batch=64, need_ctx=True)
            assert bool(so['dense_last']) == bool(dl)
            b0 = _snapshot(lib, mo, so)
            rc = lib.lgcn_ctx_set_loss(so['ctx'], L.LOSS_INBATCH, 1.0)
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "inbatch" in msg and ("FP8" in msg if mode == "fp8" else "dense_last" in msg), (mode, dl, rc, msg)
            assert lib.lgcn_ctx_get_loss(so['ctx'], None) == L.LOSS_BPR
            _same(b0, _snapshot(lib, mo, so))
    finally:
        pkg.world.configure([])


# ---- 7. through the module surface -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,K", [("fp32", 1), ("bf16", 2)])
def test_epoch_equals_the_loop_of_steps_bitwise(pkg, storage_graph, mode, K):
    """lgcn_train_epoch_inbatch over T = 165 (batches of 64, 64, 37) against the loop of lgcn_train_step_inbatch: loss rows,
    table, both Adam moments bit for bit; G64 zero and no device error afterwards."""
    try:
        B, T, d = 64, 165, 64
        cfg = dict(loss='inbatch', softmax_temp=0.2)
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


def test_training_epoch_through_procedure(pkg, oracle, storage_graph, tmp_path):
    """--loss inbatch --softmax_temp 0.2 --sampler cpp, one Procedure.BPR_train_original epoch (the sampler, the epoch permutation,
    lgcn_apply_perm, lgcn_train_epoch_inbatch) against the float64 restatement stepping the same sampled and shuffled rows (fp32
    state between steps, as the device holds it).  Tolerances as in tests/test_gpu_softmax.py::test_training_epoch_through_procedure:
    3e-6 for the mean loss and for the table, widened only by the derived per-step bounds.  The RNG streams end where the
    reference leaves them."""
    import csv
    try:
        B, d, K, tau = 256, 64, 2, 0.2
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, loss='inbatch', softmax_temp=tau, prefetch_epoch=0,
                       sampler='cpp', checkpoint_dir=os.path.join(str(tmp_path), "ckpt"))
        pkg.world.tensorboard = 0
        indptr, indices = pkg.utils._pos_csr(ds)
        oracle.srand(31); oracle.np_seed(32)
        S_ = oracle.sample_negative(ds.n_users, ds.m_items, ds.trainDataSize, indptr, indices, neg_num=1)
        T = len(S_)
        S_ = S_[oracle.np_shuffle_arange(T)]
        prm = m._table.cpu().numpy().astype(np.float64)
        mom, var = np.zeros_like(prm), np.zeros_like(prm)
        ref, ref_rows, row_tol, widen_loss, widen_tab = [], [], [], 0.0, np.zeros_like(prm)
        for i, t in enumerate(range(0, T, B)):
            batch = (S_[t:t + B, 0], S_[t:t + B, 1])
            r = IB.step(_G["A"], SC.N_USERS, K, SC.DECAY, _tau32(tau), prm, batch)
            ref.append(float(r["loss_out"][0]))
            bl = _bounds(r, batch, len(batch[0]), K, d, "fp32", False, None, _tau32(tau))["loss"]
            widen_loss += bl[0]
            ref_rows.append([float(v) for v in r["loss_out"]]); row_tol.append([3e-6 + float(v) for v in bl])
            widen_tab += 4 * U * (np.abs(prm) + 4 * SC.LR)
            prm, mom, var = IB.adam(prm, mom, var, r["g_final"].numpy(), i + 1, SC.LR)
            prm, mom, var = (x.astype(np.float32).astype(np.float64) for x in (prm, mom, var))
        pkg.sampling.seed(31); pkg.utils.set_seed(32)
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        rows_seen, fused_epoch = [], m.fused_epoch                          # the per-step rows Procedure receives and reduces
        m.fused_epoch = lambda *a_, **k_: rows_seen.append(fused_epoch(*a_, **k_)) or rows_seen[-1]
        info = pkg.Procedure.BPR_train_original(ds, m, bpr, 1)
        m.fused_epoch = fused_epoch
        assert info.startswith("loss")
        assert m.adam_step == len(ref) == (T + B - 1) // B
        # every step's (loss, sm, reg) against the restatement epoch: the project's 3e-6 (the states differ by what the earlier
        # steps' roundings left) widened by the step's own derived bound
        got_rows = rows_seen[0].cpu().numpy().astype(np.float64)
        assert len(rows_seen) == 1 and got_rows.shape == (len(ref), 3)
        step_share = np.abs(got_rows - np.asarray(ref_rows)) / np.asarray(row_tol)
        print(f"[inbatch] procedure: per-step |loss, sm, reg| largest share of 3e-6 + the step bound: {step_share.max(0)}")
        assert (step_share <= 1.0).all(), step_share
        with open(os.path.join(pkg.world.config['checkpoint_dir'], 'train_epoch_metrics.csv')) as f:
            rows = list(csv.reader(f))
        got_mean = float(rows[-1][1])
        nb = T // B + 1                                                     # Procedure's divisor (Procedure.py: total_batch)
        want_mean = float(np.sum(ref)) / nb
        tol_loss = 3e-6 + widen_loss / nb
        err_t = np.abs(m._table.cpu().numpy().astype(np.float64) - prm)
        tol_t = 3e-6 + widen_tab
        print(f"[inbatch] procedure: |mean loss| {abs(got_mean - want_mean):.2e} of {tol_loss:.2e} (3e-6 + {widen_loss / nb:.2e}); "
              f"|table| share {float((err_t / tol_t).max()):.3f} (3e-6 + at most {float(widen_tab.max()):.2e}, raw {float(err_t.max()):.2e})")
        assert abs(got_mean - want_mean) < tol_loss and (err_t <= tol_t).all()
        assert pkg.sampling.randint(10 ** 6) == oracle.randint(10 ** 6)
        out = bpr.stageOne(_dev(S_[:B, 0]), _dev(S_[:B, 1]), _dev(S_[:B, 2]))
        assert np.isfinite(out) and m.adam_step == len(ref) + 1
    finally:
        pkg.world.configure([])

"""The sampled-softmax loss in the fused step (--loss softmax; lgcn_ctx_set_loss, csrc/lgcn_multineg.hip) on the GPU
(-m gpu), on the graph, table rows and batch shapes of tests/storage_cases.py with the batches of tests/multineg_restatement.py,
against the float64 restatement tests/softmax_restatement.py.  Every step is judged from the GPU's OWN state before the step.

BOUNDS (u = 2^-24; per element, first order in u; all magnitudes from the restatement; tau below is the fp32 value the library
holds, which the restatement is given):
  forward       fp32 storage: X_k = A X_{k-1}; delta_X_0 = 0, delta_X_k = |A| delta_X_{k-1} + spmm_sum_bound(A, X_{k-1}) (conftest;
                covers an fp32 evaluation in any order twice over; edge dropout: A = A_drop, whose entries carry one more product,
                a / keep: two extra terms).  bf16 storage: layer 1 reads bf16(E0) when K >= 2 (half a bf16 ulp: stored_bound(E0, 0)),
                and every table is stored in bf16: delta_X_k = stored_bound(X_k, delta_pre_k) (tests/storage_cases.py).
  slot rows     mean: K additions and one division of terms whose absolute sum is (K + 1) T, T = sum_k |w_k X_k[row]|:
                delta_e = (K + 2) u T + sum_k |w_k| delta_X_k.  Layer weights: a product and an addition per layer:
                delta_e = 2 (K + 2) u T + sum_k |w_k| delta_X_k.  X_0 is read in fp32 (delta 0) in both storages.
  score         x_r = u.p - u.n_r, two d-term dot products in any order and a subtraction (S_p = sum |u_j p_j|, S_r alike):
                delta_x_r = (d + 2) u (S_p + S_r) + sum_j (delta_e_u (|p| + |n_r|) + |u| (delta_e_p + delta_e_n)).
                z_r = -x_r / tau, one correctly rounded division: delta_z_r = delta_x_r / tau + u |z_r|.
  normalise     l = m + log1p(Zm1) is the same function of the z_r for EVERY shift m, so the kernel's m (an fp32 number it picked
                exactly) is no source of error; a_r = z_r - m rounds once (u |a_r|); expf and log1pf are the HIP library's, 1 ulp
                = 2 u each (tests/storage_cases.py, log-sigmoid); the sum Zm1 of at most R + 1 non-negative terms over the lane
                group: one rounding per addition, at most 7 additions and the final 1 + Zm1: 8 u relative.  With q_r =
                exp(z_r - m) / Z, q_0 = exp(-m) / Z (only where m > 0 is it evaluated), P = sum_r q_r + [m > 0] q_0 <= 1:
                rho = delta_Z / Z = 10 u P + sum_r q_r (delta_z_r + u |a_r|)
                delta_l = rho + 2 u log1p(Zm1) + u |l| <= rho + 3 u l                     (terms[b] = -l)
                delta_q_r = q_r (4 u + delta_z_r + u |a_r| + rho) + 2^-140        (expf, the division, 1 + Zm1; subnormal results)
  gb            gb_r = -q_r * fl(1 / (tau B)): delta_gb_r = 2 u |gb_r| + delta_q_r / (tau B).
  g_n           fl(fl(-gb_r u) + fl(lam_n n)), lam_n = fl(fl(decay) / (float)(B R)) against decay / (B R) in float64 (2 u):
                delta_gn = 4 u (|gb_r| |u| + lam_n |n_r|) + 2 u lam_n |n_r| + delta_gb_r |u| + |gb_r| delta_e_u + lam_n delta_e_n + 2^-51.
  g_p           fl(fl(sgb u) + fl(lam p)), sgb the fp32 sum of the R gb_r (one sign: R - 1 relative roundings):
                delta_gp = (R + 3) u sum_r |gb_r| |u| + 6 u lam |p| + sum_r (delta_gb_r |u| + |gb_r| delta_e_u) + lam delta_e_p + 2^-51.
  g_u           fl(fl(fl(sgb p) - acc) + fl(lam u)), acc the fp32 sum of the R products gb_r n_r:
                delta_gu = (R + 4) u sum_r |gb_r| (|p| + |n_r|) + 6 u lam |u| + sum_r (delta_gb_r (|p| + |n_r|) + |gb_r| (delta_e_p +
                delta_e_n)) + lam delta_e_u + 2^-51.
  G, Gs         the fixed-point sum over the slots naming a row is exact: delta_G[row] = the sum of its slots' deltas; the
                conversion to fp32 and the division by K + 1: delta_Gs = delta_G / div + 2 u |Gs| (div = 1 with layer weights).
  backward      launch i computes c_add Gs + A h: D = c_add delta_Gs + |A| delta_h + spmm_sum_bound(A, |h| + delta_h) + 2 u (|c_add
                Gs| + |A| |h|); every launch but the last is stored: stored_bound(value, D) with bf16 storage.  reg_ego: the last
                launch adds fl(lam_e cnt) E0: 4 u of it and 2 u of the sum.  Edge dropout: A = A_drop^T here.
  last link     the gradient is read from Adam's first moment, g_rec = M + (M' - M) / w1, good to 2^-21 (|M| + |M'|) / w1; the table
                and the second moment by test_gpu_gate_shapes._adam_checks.
  reg term      sums of squares, every rounding relative; the longest chain is a negative's: 2 R CPT roundings in the lane (CPT =
                d / min(d, 64)), times fl(1 / R) (2 u), 2 additions, 6 in the lane-group sum:
                delta_reg = (2 (R + 2) CPT + 12) u regterm + 2 sum |e| delta_e       (reg_ego: the rows are exact, delta_e = 0).
  loss_out      one wave: c(B) = ceil(B / 64) + 8 roundings of partial sums <= sum |term| (tests/test_gpu_multineg.py):
                delta_sm = mean_b delta_l + c(B) u mean_b l; delta_reg_out = 0.5 (mean delta_reg + c(B) u mean regterm);
                delta_0 = delta_sm + decay delta_reg_out + 4 u (|sm| + decay |reg|).
Every test prints the largest share of each bound it used."""
import os

import numpy as np
import pytest
import torch

import multineg_restatement as MN
import softmax_restatement as SM
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


def _bounds(r, batch, B, R, K, d, mode, ego, w, tau, fwd=None, bwd=None):
    """The bounds of the module docstring from a restatement r of the sound samples `batch` of a step normalised by B ->
    dict: term, regterm [b], loss (3), g_final [N, d].  fwd / bwd: scipy CSR of the forward / backward matrix (default A_hat)."""
    adj = _G["adj"]
    extra = 2 if fwd is None else 4
    fwd = adj.astype(np.float64) if fwd is None else fwd
    bwd = fwd if bwd is None else bwd
    af, ab = abs(fwd).tocsr(), abs(bwd).tocsr()
    wk = MN.layer_weights(K, w)
    E0 = r["E0"].numpy()
    # ---- forward tables and slot rows
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
    u_, p_, n_ = SM.as_samples(batch)
    ui, pi, ni = u_, SC.N_USERS + p_, SC.N_USERS + n_
    au, ap, an = T[ui], T[pi], T[ni]
    du, dp, dn = dE[ui], dE[pi], dE[ni]
    Sp, Sr = (au * ap).sum(1), (au[:, None, :] * an).sum(2)
    dx = (d + 2) * U * (Sp[:, None] + Sr) + (du[:, None, :] * (ap[:, None, :] + an) + au[:, None, :] * (dp[:, None, :] + dn)).sum(2)
    z, mm, q, l = r["z"].numpy(), r["m"].numpy(), r["q"].numpy(), r["lterm"].numpy()
    dz = dx / tau + U * np.abs(z)
    a = np.abs(z - mm[:, None])
    q0 = np.where(mm > 0, np.exp(-mm) / (np.exp(-mm) + np.exp(z - mm[:, None]).sum(1)), 0.0)
    P = np.minimum(q.sum(1) + q0, 1.0)
    rho = 10 * U * P + (q * (dz + U * a)).sum(1)
    out = {"term": rho + 3 * U * l + 1e-37}
    dq = q * (4 * U + dz + U * a + rho[:, None]) + 2.0 ** -140
    gb = np.abs(r["gb"].numpy())
    dgb = 2 * U * gb + dq / (tau * B)
    gb = gb + dgb
    # ---- reg term
    CPT = d // min(d, 64)
    if ego:
        e0 = np.abs(E0)
        regterm = (e0[ui] ** 2).sum(1) + (e0[pi] ** 2).sum(1) + (e0[ni] ** 2).sum((1, 2)) / R
        d_regx = 0.0
    else:
        regterm = (au * au).sum(1) + (ap * ap).sum(1) + (an * an).sum((1, 2)) / R
        d_regx = 2.0 * ((au * du).sum(1) + (ap * dp).sum(1) + (an * dn).sum((1, 2)) / R)
    out["regterm"] = (2 * (R + 2) * CPT + 12) * U * regterm + d_regx + 1e-37
    cB = _c(B) * U
    b_sm = out["term"].sum() / B + cB * l.sum() / B
    b_reg = 0.5 * (out["regterm"].sum() / B + cB * regterm.sum() / B)
    lo = [float(v) for v in r["loss_out"]]
    out["loss"] = (b_sm + SC.DECAY * b_reg + 4 * U * (abs(lo[1]) + SC.DECAY * abs(lo[2])), b_sm, b_reg)
    # ---- gradient rows
    lam = 0.0 if ego else SC.DECAY / B
    lam_n = lam / R
    fx = 2.0 ** -51
    gbc, dgbc = gb[:, :, None], dgb[:, :, None]
    d_gn = 4 * U * (gbc * au[:, None, :] + lam_n * an) + 2 * U * lam_n * an + dgbc * au[:, None, :] + gbc * du[:, None, :] + lam_n * dn + fx
    d_gp = (R + 3) * U * gb.sum(1)[:, None] * au + 6 * U * lam * ap + dgb.sum(1)[:, None] * au + gb.sum(1)[:, None] * du + lam * dp + fx
    pn = ap[:, None, :] + an
    d_gu = (R + 4) * U * (gbc * pn).sum(1) + 6 * U * lam * au + (dgbc * pn).sum(1) + (gbc * (dp[:, None, :] + dn)).sum(1) + lam * du + fx
    dG = np.zeros_like(T)
    np.add.at(dG, ui, d_gu); np.add.at(dG, pi, d_gp); np.add.at(dG, ni.reshape(-1), d_gn.reshape(-1, d))
    div = 1.0 if w is not None else float(K + 1)
    Gref = r["G"].numpy()
    Gs = np.abs(Gref) / div
    dGs = dG / div + 2 * U * Gs
    # ---- backward chain: the float64 values v_i of the launches and their bounds
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
        D = D + 4 * U * (SC.DECAY / (B * R)) * r["cnt"].numpy()[:, None] * np.abs(E0) + 2 * U * np.abs(r["g_final"].numpy())
    out["g_final"] = D
    return out


def _judge(pkg, m, batch, R, K, d, mode, reg, tau, step_no, tag, w=None, keep=None, void=None):
    """One fused step from the GPU's own state -> {link: share of its bound}.  void: index of a sample whose id is bad in
    `batch`: its terms must be zero and the step is the restatement of the sound samples with B_norm = B."""
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
    out = m.fused_step(_dev(batch[0]), _dev(batch[1]), _dev(batch[2])).cpu().numpy().astype(np.float64)
    after = _state(m)
    t = m._dev['terms'].cpu().numpy().astype(np.float64)
    term, regt = t[:B], t[B:2 * B]
    sound = np.ones(B, bool)
    if void is not None:
        sound[void] = False
        assert term[void] == 0.0 and regt[void] == 0.0
    sb = tuple(np.asarray(a)[sound] for a in batch)
    r = SM.step(Af, SC.N_USERS, K, SC.DECAY, tau, before["table"], sb, ego, w, B_norm=B, A_bwd=Ab)
    bd = _bounds(r, sb, B, R, K, d, mode, ego, w, tau, fwd, bwd)
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
    print(f"[softmax] {tag}: shares " + " ".join(f"{k}={v:.3f}" for k, v in share.items()))
    return share, r, (term, regt, g_rec, slack, bd)


def _run(pkg, path, mode, d, K, R, tau, reg="propagated", w=None, keep=None, sizes=MN.BATCH_SIZES):
    try:
        cfg = {'loss': 'softmax', 'softmax_temp': tau, 'neg_ratio': R}
        if w is not None:
            cfg['layer_weights'] = str(list(w))
        if keep is not None:
            cfg.update({'dropout': 1, 'keep_prob': keep, 'seed': 2020})
        _, m = _model(pkg, path, mode, d, K, reg, dl=0, batch=max(sizes), **cfg)      # --dense_last 0: _make_ctx must force the dense last layer
        top, bad = {}, []
        for i, batch in enumerate(SM.make_batches(d, K, R, sizes=sizes)):
            tag = f"{mode} d{d} K{K} R{R} tau{tau} {reg}" + (" wts" if w is not None else "") + (f" keep{keep}" if keep else "") + f" step {i + 1} B={len(batch[0])}"
            share = _judge(pkg, m, batch, R, K, d, mode, reg, _tau32(tau), i + 1, tag, w=w, keep=keep)[0]
            for k_, v in share.items():
                top[k_] = max(top.get(k_, 0.0), v)
                if not v <= 1.0:
                    bad.append((tag, k_, v))
            m.check_device_errors()
            assert not bool(m._dev['G64'].any()) and m.adam_step == i + 1
        assert m._dev['dense_last'] is True
        lib = pkg._lib.load()
        assert lib.lgcn_ctx_get_loss(m._dev['ctx'], None) == pkg._lib.LOSS_SOFTMAX
        print(f"[softmax] {mode} d{d} K{K} R{R} tau{tau} {reg} TOP: " + " ".join(f"{k_}={v:.3f}" for k_, v in top.items()))
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
    finally:
        pkg.world.configure([])


# ---- 1. four steps against the float64 restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 16])
@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_steps_equal_the_restatement(pkg, storage_graph, d, R):
    """fp32 storage, K = 3, tau = 1: per-sample terms, loss_out, the gradient recovered from Adam's first moment, Adam itself,
    each within the bound derived in the module docstring, over batches of 64 / 64 / 37 / 1 samples."""
    _run(pkg, storage_graph, "fp32", d, 3, R, 1.0)


# The per-sample terms of this step are scaled by inv_R and reduced by reduce_loss_wave, which adds terms[lane], terms[lane + 64],
# ..: no batch above has more than 64 samples, so the second addition is first taken here (MN.LARGE_BATCH_SIZES = 65, 300; the
# bound's c(B) = ceil(B / 64) + 8 counts it).  Every width, both storages, K in {1, 3}, both reg rows, R = 2 and 16.
_LARGE_CASES = [(32, 1, 2, "bf16", "propagated", 1.0), (64, 3, 16, "fp32", "ego", 0.2), (128, 3, 2, "fp32", "propagated", 0.2), (256, 1, 16, "bf16", "ego", 1.0)]
assert {c[0] for c in _LARGE_CASES} == set(MN.DS) and {c[1] for c in _LARGE_CASES} == {1, 3} and {c[2] for c in _LARGE_CASES} == set(MN.LARGE_RS)
assert {c[3] for c in _LARGE_CASES} == {"fp32", "bf16"} and {c[4] for c in _LARGE_CASES} == {"propagated", "ego"}
assert all(_c(B) - 8 >= 2 for B in MN.LARGE_BATCH_SIZES)


@pytest.mark.parametrize("d,K,R,mode,reg,tau", [pytest.param(*c, id=f"d{c[0]}-K{c[1]}-R{c[2]}-{c[3]}-{c[4]}-tau{c[5]}") for c in _LARGE_CASES])
def test_steps_equal_the_restatement_beyond_one_wave_of_terms(pkg, storage_graph, d, K, R, mode, reg, tau):
    """Batches of 65 and 300 samples in a context of 300: the links of test_steps_equal_the_restatement within the same bounds."""
    _run(pkg, storage_graph, mode, d, K, R, tau, reg, sizes=MN.LARGE_BATCH_SIZES)


@pytest.mark.parametrize("K", [1, 2])
def test_steps_at_a_low_temperature(pkg, storage_graph, K):
    _run(pkg, storage_graph, "fp32", 64, K, 5, 0.2)


@pytest.mark.parametrize("d", [32, 128])
def test_steps_with_bf16_storage(pkg, storage_graph, d):
    _run(pkg, storage_graph, "bf16", d, 2, 5, 1.0)


@pytest.mark.parametrize("d", [64, 256])
def test_steps_with_reg_rows_ego(pkg, storage_graph, d):
    """reg_ego: the slot counts (R per user / positive slot, 1 per negative slot) with decay / (B R) in the epilogue."""
    _run(pkg, storage_graph, "fp32", d, 2, 5, 0.2, reg="ego")


def test_steps_with_layer_weights(pkg, storage_graph):
    _run(pkg, storage_graph, "fp32", 128, 3, 5, 1.0, w=[0.4, 0.1, 0.3, 0.2])


def test_steps_with_edge_dropout(pkg, storage_graph):
    """keep 0.8: the restatement runs on A_drop (forward) and A_drop^T (backward) of each step, from the exported mask."""
    _run(pkg, storage_graph, "fp32", 64, 2, 5, 1.0, keep=0.8)


# ---- 2. R = 1, tau = 1 against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K,reg", [(32, 3, "propagated"), (64, 3, "propagated"), (128, 3, "propagated"), (256, 3, "propagated"), (64, 1, "ego")])
def test_one_negative_at_temperature_one_is_the_oracles_bpr_step(pkg, oracle, storage_graph, d, K, reg):
    """--loss softmax --neg_ratio 1 --softmax_temp 1 with 1-D negatives: fused_step routes to lgcn_train_step_multi at R = 1 and
    the new kernel computes the BPR step: loss triple and table against oracle.Trainer on the same triplets at the project's
    oracle yardstick 3e-6, after each of four steps (the triplets of tests/storage_cases.py)."""
    try:
        ds, m = _model(pkg, storage_graph, "fp32", d, K, reg, dl=0, loss='softmax', softmax_temp=1.0, neg_ratio=1)
        adj = _G["adj"]
        csr = (adj.indptr, adj.indices, adj.data)
        tr = oracle.Trainer(SC.N_USERS, adj.indptr, adj.indices, adj.data, m._table.cpu().numpy(), K, SC.DECAY, SC.LR, reg_rows=reg)
        worst, bad = 0.0, []
        for i, (u, p, n) in enumerate(SC.make_batches(("fp32", d, K, 1, -1, reg))):
            E = oracle.propagate(*csr, tr.e0, tr.K)
            bpr, rg = (oracle.bpr_ego(E, tr.e0, SC.N_USERS, u, p, n, SC.DECAY) if reg == "ego" else oracle.bpr(E, SC.N_USERS, u, p, n, SC.DECAY))[:2]
            ref = (tr.stageOne(u, p, n), bpr, rg)
            out = m.fused_step(_dev(u), _dev(p), _dev(n)).cpu().numpy().astype(np.float64)
            errs = [abs(out[j] - ref[j]) for j in range(3)] + [float(np.abs(m._table.cpu().numpy().astype(np.float64) - tr.e0).max())]
            worst = max(worst, max(errs))
            print(f"[softmax] oracle d{d} K{K} {reg} step {i + 1} B={len(u)}: |loss| {errs[0]:.2e} |sm| {errs[1]:.2e} |reg| {errs[2]:.2e} |table| {errs[3]:.2e}")
            bad += [(i + 1, name, float(e)) for name, e in zip(("loss", "sm", "reg", "table"), errs) if not e < 3e-6]
            m.check_device_errors()
            assert m.adam_step == i + 1 and not bool(m._dev['G64'].any())
        assert m._dev['dense_last'] is True
        print(f"[softmax] oracle d{d} K{K} {reg} TOP share of 3e-6: {worst / 3e-6:.3f}")
        assert not bad, ("beyond 3e-6 of the oracle (step, quantity, distance)", bad)
    finally:
        pkg.world.configure([])


# ---- 3. the saturation batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_saturation_batch(pkg, storage_graph, mode):
    """tests/test_softmax_host.py::test_saturation_batch_exists: z beyond +100 and samples with all z below -100 (tau = 0.05,
    d = 256, K = 1).  Every output is finite, terms and the recovered gradient lie within the derived bounds, and a dominated
    negative's q underflows: its G row, where no other slot names it, is lam_n e_n alone -- the step's gradient on that row is
    what the restatement gives with that q set to zero, to the bound.  Without the maximum subtracted the sums are inf / nan."""
    try:
        d, K, R, tau = SM.SAT_D, SM.SAT_K, 4, SM.SAT_TAU
        _, m = _model(pkg, storage_graph, mode, d, K, loss='softmax', softmax_temp=tau, neg_ratio=R, batch=8)
        E = SM.propagate(_G["A"], torch.from_numpy(m._table.cpu().numpy().astype(np.float64)), K).numpy()
        batch = SM.saturation_batch(E, R)
        share, r, (term, regt, g_rec, slack, bd) = _judge(pkg, m, batch, R, K, d, mode, "propagated", _tau32(tau), 1, f"saturation {mode}")
        m.check_device_errors()
        z, q = r["z"].numpy(), r["q"].numpy()
        assert (z > 100.0).any() and (z < -100.0).all(1).any()
        assert np.isfinite(m._table.cpu().numpy()).all() and np.isfinite(term).all()
        assert all(v <= 1.0 for v in share.values()), share
        # the dominated sample (all z << 0): its term is exactly -0 or a subnormal away, its negatives get lam_n e_n only
        dead = np.where((z < -110.0).all(1))[0]
        assert len(dead) >= 1
        lam_n = SC.DECAY / (8 * R)
        for b in dead:
            assert abs(term[b]) <= 2.0 ** -126 and float(q[b].max()) < 1e-45
            for j in range(R):
                row = SC.N_USERS + int(batch[2][b, j])
                named = (batch[0] == row).sum() + (SC.N_USERS + batch[1] == row).sum() + (SC.N_USERS + batch[2] == row).sum()
                if named == 1 and K == 1:
                    # g_final[row] = 0.5 (G + A G)[row]; G[row] = lam_n e_n exactly as far as this slot goes
                    want = 0.5 * (lam_n * r["e_n"][b, j].numpy() + (_G["A"] @ r["G"])[row].numpy())
                    assert (np.abs(g_rec[row] - want) <= bd["g_final"][row] + slack[row] + 1e-300).all()
                    assert float(np.abs(r["G"][row].numpy() - lam_n * r["e_n"][b, j].numpy()).max()) <= 1e-15 * lam_n * float(r["e_n"][b, j].abs().max())
    finally:
        pkg.world.configure([])


# ---- 4. the epoch call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,K", [("fp32", 1), ("bf16", 2)])
def test_epoch_equals_the_loop_of_steps_bitwise(pkg, storage_graph, mode, K):
    """lgcn_train_epoch_multi over T = 165 (batches of 64, 64, 37, column stride T) against the loop of lgcn_train_step_multi under
    the softmax loss: loss rows, table, both Adam moments bit for bit; G64 zero and no device error afterwards."""
    try:
        R, B, T, d = 5, 64, 165, 64
        cfg = dict(loss='softmax', softmax_temp=0.2, neg_ratio=R)
        seq = SM.make_batches(d, K, R)[:3]
        u = np.concatenate([b[0] for b in seq]); p = np.concatenate([b[1] for b in seq]); n = np.concatenate([b[2] for b in seq])
        assert len(u) == T
        _, a = _model(pkg, storage_graph, mode, d, K, **cfg)
        want = a.fused_epoch(_dev(u), _dev(p), _dev(np.ascontiguousarray(n.T)), B)
        a.check_device_errors()
        _, b = _model(pkg, storage_graph, mode, d, K, **cfg)
        first = b._table.detach().clone()
        got = [b.fused_step(_dev(u[t:t + B]), _dev(p[t:t + B]), _dev(n[t:t + B])) for t in range(0, T, B)]
        b.check_device_errors()
        assert a.adam_step == b.adam_step == 3 and want.shape == (3, 3)
        assert torch.equal(torch.stack(got), want), (torch.stack(got), want)
        assert torch.equal(a._table, b._table), int((a._table != b._table).sum())
        assert torch.equal(a._dev['adam_m'], b._dev['adam_m']) and torch.equal(a._dev['adam_v'], b._dev['adam_v'])
        assert not bool(a._dev['G64'].any()) and not bool(b._dev['G64'].any())
        assert float((b._table - first).abs().max()) > 1e-4                 # (it trained)
        # ... and it is another loss than --loss bpr on the same samples
        _, c = _model(pkg, storage_graph, mode, d, K, neg_ratio=R)
        other = c.fused_epoch(_dev(u), _dev(p), _dev(np.ascontiguousarray(n.T)), B)
        assert float((other[:, 1] - want[:, 1]).abs().min()) > 1e-3
    finally:
        pkg.world.configure([])


# ---- 5. a voided sample ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,R", [(32, 16), (64, 2)])
def test_voided_sample(pkg, storage_graph, d, R):
    """One sample with ONE out-of-range negative (K = 1; d = 32, R = 16: the lane group is exactly 32 lanes wide with 18 id
    lanes): the err flag, zero terms for that sample, and the other samples' step is the restatement with B_norm = B."""
    try:
        K, void = 1, 3
        u, p, n = SM.make_batches(d, K, R)[0]
        nbad = n.copy(); nbad[void, R - 1] = SC.M_ITEMS
        _, m = _model(pkg, storage_graph, "fp32", d, K, loss='softmax', softmax_temp=1.0, neg_ratio=R)
        share = _judge(pkg, m, (u, p, nbad), R, K, d, "fp32", "propagated", 1.0, 1, f"void d{d} R{R}", void=void)[0]
        assert all(v <= 1.0 for v in share.values()), share
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


# ---- 6. --loss bpr is the parent's path --------------------------------------------------------------------------------------
def test_loss_bpr_is_the_parents_path(pkg, storage_graph):
    """lgcn_ctx_set_loss(SOFTMAX) then (BPR) on a context: a multi step at R = 5 and a three-slot step are bit for bit those of a
    context that was never told; lgcn_ctx_get_loss reports what was set."""
    import ctypes as C
    try:
        L = pkg._lib
        lib = L.load()
        d, K, R = 64, 2, 5
        u, p, n = SM.make_batches(d, K, R)[0]
        res = []
        for told in (True, False):
            _, m = _model(pkg, storage_graph, "fp32", d, K, neg_ratio=R)
            ctx = m._state(max_batch=64, need_ctx=True)['ctx']
            tau = C.c_float(-1.0)
            assert lib.lgcn_ctx_get_loss(ctx, C.byref(tau)) == L.LOSS_BPR and tau.value == 1.0
            if told:
                L.check(lib.lgcn_ctx_set_loss(ctx, L.LOSS_SOFTMAX, 0.25), "set_loss")
                assert lib.lgcn_ctx_get_loss(ctx, C.byref(tau)) == L.LOSS_SOFTMAX and tau.value == 0.25
                L.check(lib.lgcn_ctx_set_loss(ctx, L.LOSS_BPR, float("nan")), "set_loss")
                assert lib.lgcn_ctx_get_loss(ctx, C.byref(tau)) == L.LOSS_BPR and tau.value == 1.0
            o1 = m.fused_step(_dev(u), _dev(p), _dev(n)).clone()
            o2 = m.fused_step(_dev(u), _dev(p), _dev(n[:, 0])).clone()          # the three-slot step (lgcn_train_step)
            m.check_device_errors()
            assert m.adam_step == 2
            res.append((o1, o2, m._table.detach().clone(), m._dev['adam_m'].clone(), m._dev['adam_v'].clone()))
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def _snapshot(lib, m, st):
    return (m._table.detach().clone(), st['adam_m'].clone(), st['adam_v'].clone(), int(lib.lgcn_ctx_get_step(st['ctx'])),
            st['G64'].clone(), st['terms'].clone())


def _same(before, after):
    for a, b in zip(before, after):
        assert (a == b) if isinstance(a, int) else torch.equal(a, b)


def test_refusals_leave_everything_untouched(pkg, storage_graph):
    import ctypes as C
    try:
        L = pkg._lib
        lib = L.load()
        B = 8
        u = _dev(np.arange(B)); p = _dev(np.arange(B)); n = _dev(np.arange(B) + 1)
        u64, p64, n64 = (t.long() for t in (u, p, n))
        scratch = torch.full((3 * 64,), -5, dtype=torch.int32, device=DEV)
        loss = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
        stream = L.current_stream()
        # (a) while softmax is set, every three-slot and rank-splitting entry point
        _, m = _model(pkg, storage_graph, "fp32", 64, 2, loss='softmax', softmax_temp=0.5, neg_ratio=4)
        st = m._state(max_batch=64, need_ctx=True)
        ctx = st['ctx']
        before = _snapshot(lib, m, st)
        calls = {
            "lgcn_train_step": lambda: lib.lgcn_train_step(ctx, L.tp(u), L.tp(p), L.tp(n), B, L.tp(loss), stream),
            "lgcn_train_step_i64": lambda: lib.lgcn_train_step_i64(ctx, L.tp(u64), L.tp(p64), L.tp(n64), B, L.tp(scratch), L.tp(loss), stream),
            "lgcn_train_epoch": lambda: lib.lgcn_train_epoch(ctx, L.tp(u), L.tp(p), L.tp(n), B, B, L.tp(loss), stream),
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
            assert rc == 3 and "softmax" in msg and name in msg, (name, rc, msg)
        torch.cuda.synchronize()
        _same(before, _snapshot(lib, m, st))
        assert bool((loss == -7.0).all()) and bool((scratch == -5).all())
        # (b) a temperature that is no temperature, an unknown kind: refused, the loss in force stays
        for kind, tau in ((L.LOSS_SOFTMAX, 0.0), (L.LOSS_SOFTMAX, -1.0), (L.LOSS_SOFTMAX, float("nan")), (L.LOSS_SOFTMAX, float("inf")), (7, 1.0)):
            rc = lib.lgcn_ctx_set_loss(ctx, kind, tau)
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and ("softmax" in msg or "loss" in msg), (kind, tau, rc, msg)
        t_ = C.c_float(0.0)
        assert lib.lgcn_ctx_get_loss(ctx, C.byref(t_)) == L.LOSS_SOFTMAX and t_.value == 0.5
        _same(before, _snapshot(lib, m, st))
        # ... and the same context takes a sound call afterwards
        bu, bp, bn = SM.make_batches(64, 2, 2)[0]
        out = m.fused_step(_dev(bu), _dev(bp), _dev(bn))
        m.check_device_errors()
        assert bool(torch.isfinite(out).all()) and m.adam_step == 1
        # (c) contexts that cannot run it: fp8 storage, dense_last = 0
        for mode, dl in (("fp8", 1), ("fp32", 0)):
            _, mo = _model(pkg, storage_graph, mode, 64, 2, dl=dl)
            so = mo._state(max_batch=64, need_ctx=True)
            assert bool(so['dense_last']) == bool(dl)
            b0 = _snapshot(lib, mo, so)
            rc = lib.lgcn_ctx_set_loss(so['ctx'], L.LOSS_SOFTMAX, 1.0)
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and "softmax" in msg and ("FP8" in msg if mode == "fp8" else "dense_last" in msg), (mode, dl, rc, msg)
            assert lib.lgcn_ctx_get_loss(so['ctx'], None) == L.LOSS_BPR
            _same(b0, _snapshot(lib, mo, so))
    finally:
        pkg.world.configure([])


# ---- 8. through the module surface -------------------------------------------------------------------------------------------
def test_training_epoch_through_procedure(pkg, oracle, storage_graph, tmp_path):
    """--loss softmax --neg_ratio 5 --softmax_temp 0.2 --sampler cpp, one Procedure.BPR_train_original epoch (host sampler with
    neg_num = 5, the epoch permutation, lgcn_apply_perm_multi, lgcn_train_epoch_multi) against the float64 restatement stepping
    the same sampled and shuffled rows (fp32 state between steps, as the device holds it).  Tolerances: those of
    tests/test_gpu_multineg.py::test_training_epoch_through_procedure (3e-6 for the mean loss and for the table), widened only by
    the derived per-step bounds: the mean over the steps of delta_0 (module docstring) for the mean loss, and per element the sum
    over the steps of the parameter bound of _adam_checks, 4 u (|p| + 4 lr), for the table.  Both sums are printed."""
    import csv
    try:
        R, B, d, K, tau = 5, 256, 64, 2, 0.2
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, neg_ratio=R, loss='softmax', softmax_temp=tau, prefetch_epoch=0,
                       sampler='cpp', checkpoint_dir=os.path.join(str(tmp_path), "ckpt"))
        pkg.world.tensorboard = 0
        indptr, indices = pkg.utils._pos_csr(ds)
        oracle.srand(31); oracle.np_seed(32)
        S_ = oracle.sample_negative(ds.n_users, ds.m_items, ds.trainDataSize, indptr, indices, neg_num=R)
        T = len(S_)
        S_ = S_[oracle.np_shuffle_arange(T)]
        prm = m._table.cpu().numpy().astype(np.float64)
        mom, var = np.zeros_like(prm), np.zeros_like(prm)
        ref, widen_loss, widen_tab = [], 0.0, np.zeros_like(prm)
        for i, t in enumerate(range(0, T, B)):
            batch = (S_[t:t + B, 0], S_[t:t + B, 1], S_[t:t + B, 2:])
            r = SM.step(_G["A"], SC.N_USERS, K, SC.DECAY, _tau32(tau), prm, batch)
            ref.append(float(r["loss_out"][0]))
            widen_loss += _bounds(r, batch, len(batch[0]), R, K, d, "fp32", False, None, _tau32(tau))["loss"][0]
            widen_tab += 4 * U * (np.abs(prm) + 4 * SC.LR)
            prm, mom, var = SM.adam(prm, mom, var, r["g_final"].numpy(), i + 1, SC.LR)
            prm, mom, var = (x.astype(np.float32).astype(np.float64) for x in (prm, mom, var))
        pkg.sampling.seed(31); pkg.utils.set_seed(32)
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        info = pkg.Procedure.BPR_train_original(ds, m, bpr, 1)
        assert info.startswith("loss")
        assert m.adam_step == len(ref) == (T + B - 1) // B
        with open(os.path.join(pkg.world.config['checkpoint_dir'], 'train_epoch_metrics.csv')) as f:
            rows = list(csv.reader(f))
        got_mean = float(rows[-1][1])
        nb = T // B + 1                                                     # Procedure's divisor (Procedure.py: total_batch)
        want_mean = float(np.sum(ref)) / nb
        tol_loss = 3e-6 + widen_loss / nb
        err_t = np.abs(m._table.cpu().numpy().astype(np.float64) - prm)
        tol_t = 3e-6 + widen_tab
        print(f"[softmax] procedure: |mean loss| {abs(got_mean - want_mean):.2e} of {tol_loss:.2e} (3e-6 + {widen_loss / nb:.2e}); "
              f"|table| share {float((err_t / tol_t).max()):.3f} (3e-6 + at most {float(widen_tab.max()):.2e}, raw {float(err_t.max()):.2e})")
        assert abs(got_mean - want_mean) < tol_loss and (err_t <= tol_t).all()
        assert pkg.sampling.randint(10 ** 6) == oracle.randint(10 ** 6)
        # the sampler's rows as they come, [T, R], and 1-D negatives (R = 1) go through stageOne too
        out = bpr.stageOne(_dev(S_[:B, 0]), _dev(S_[:B, 1]), _dev(S_[:B, 2:]))
        assert np.isfinite(out) and m.adam_step == len(ref) + 1
        out = bpr.stageOne(_dev(S_[:B, 0]), _dev(S_[:B, 1]), _dev(S_[:B, 2]))
        assert np.isfinite(out) and m.adam_step == len(ref) + 2
    finally:
        pkg.world.configure([])

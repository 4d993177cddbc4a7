"""Several negatives per positive in the fused step (--neg_ratio; lgcn_train_step_multi / _epoch_multi, csrc/lgcn_multineg.hip,
DESIGN 4.17) on the GPU (-m gpu), on the graph, table rows and batch shapes of tests/storage_cases.py with the batches of
tests/multineg_restatement.py.

The specification is an identity: the step on B samples (u, p, n_1..n_R) is the three-slot step on the flattened batch of B R
triplets (u, p, n_r).  So the references are (1) oracle.Trainer stepping the flattened batches, at the project's yardstick for
oracle comparisons (atol 3e-6, test_fused_step_vs_oracle), and (2) the EXISTING fused step on the flattened batch, from the same
state with dense_last = 1 on both sides: the forward tables are then the same bits and only the batch-row arithmetic differs.

BOUND of (2) (u = 2^-24; per element, first order in u; N = the new kernel k_multineg_dense, O = k_triplet_dense on the
flattened batch; |e| below is T = sum_k |w_k X_k[row]| >= |e|, from the float64 restatement, times 1 + 2^-6 for the storage
roundings the restatement does not make; S_p = sum_j |u_j p_j|, S_r = sum_j |u_j n_rj|):
  slot rows     the mean form adds K + 1 loaded values in layer order and divides once in both kernels: no product, nothing to
                contract, the same bits (delta_e = 0).  Layer weights: s = w_0 x_0, s += w_k x_k -- either kernel may or may not
                contract a step into an fma: delta_e = 2 (K + 2) u T.
  score         x_r = u.p - u.n_r: each evaluation of a d-term dot product in any order and with any contraction errs by at
                most (d + 1) u S, the subtraction by u (S_p + S_r): two evaluations,
                delta_x_r = 2 (d + 2) u (S_p + S_r) + sum_j (delta_e_u (|p| + |n_r|) + |u| (delta_e_p + delta_e_n)).
  log-sigmoid   tests/storage_cases.py: one evaluation 8 u |t| at its own x, d t / d x = sigmoid(-x) = s:
                |t_N,r - t_O,r| <= 16 u |t_r| + s_r delta_x_r.  N adds the R terms in fp32 (R - 1 roundings of partial sums
                <= sum |t_r|) and multiplies by fl(1 / R) (2 u):
                delta_term = (sum_r (16 u |t_r| + s_r delta_x_r) + (R + 1) u sum_r |t_r|) / R      against mean_r t_O,r.
  reg term      sums of squares, all terms >= 0, so every rounding is relative.  N: a lane adds R CPT squares of negatives
                (CPT = d / min(d, 64) columns per lane; product + addition each), times fl(1 / R) (2 u), + |u|^2 + |p|^2 (2 CPT
                + 2), the 6 additions of the lane-group sum: (2 (R + 1) CPT + 10) u.  O per triplet: (2 CPT + 8) u.
                delta_reg = (2 (R + 2) CPT + 18) u regterm + 2 sum |e| delta_e.
  loss_out      one wave: a lane adds ceil(n / 64) terms in order, 6 more additions in the tree, a division, the sign:
                c(n) = ceil(n / 64) + 8 roundings of partial sums <= sum |term|.  N reduces B terms, O reduces B R:
                delta_bpr = (c(B) + c(B R)) u mean |t| + mean_b delta_term; the reg line the same with the factor 0.5;
                loss_out[0] = bpr + decay reg: delta_0 = delta_bpr + decay delta_reg + 4 u (|bpr| + decay |reg|).
  gb            tests/storage_cases.py: 8 u |gb| per evaluation, |d gb / d x| <= |gb|: delta_gb_r = 16 u |gb_r| + |gb_r| delta_x_r.
                Both kernels multiply by the same fl(1 / (float)(B R)).
  g_n           the same expression in both kernels, (-gb) u + lam_n n with lam_n = fl(decay / (float)(B R)) on both sides:
                two evaluations of <= 3 roundings and ONE fixed-point rounding each:
                delta_gn = 4 u (|gb_r| |u| + lam_n |n_r|) + delta_gb_r |u| + |gb_r| delta_e_u + lam_n delta_e_n + 2 * 2^-51.
  g_p           N: fl(fl(sgb u) + fl(lam p)), sgb = the fp32 sum of the R gb_r (R - 1 roundings), lam = fl(decay / (float) B),
                ONE fixed-point rounding.  O: R terms fl(gb_r u + lam_n p), each rounded to fixed point and summed exactly --
                THE difference the issue names: N rounds sum_r in fp32 before one fixed-point add of 2^-51, O rounds each term
                to fixed point and sums exactly.  |lam - R lam_n| <= 2 u lam.
                delta_gp = (R + 3) u sum_r |gb_r| |u| + 6 u lam |p| + sum_r (delta_gb_r |u| + |gb_r| delta_e_u) + lam delta_e_p
                           + (R + 1) 2^-51.
  g_u           N: fl(fl(fl(sgb p) - acc) + fl(lam u)), acc = the fp32 sum of the R products gb_r n_r: (R + 4) u sum_r |gb_r|
                (|p| + |n_r|) + 2 u lam |u| + 2^-51.  O: R terms fl(gb_r (p - n_r) + lam_n u) -> 3 u |gb_r| (|p| + |n_r|) + 2 u
                lam_n |u| + 2^-51 each.
                delta_gu = (R + 7) u sum_r |gb_r| (|p| + |n_r|) + 6 u lam |u| + sum_r (delta_gb_r (|p| + |n_r|) + |gb_r|
                           (delta_e_p + delta_e_n)) + lam delta_e_u + (R + 1) 2^-51.
  G, Gs         delta_G[row] = the sum of the deltas of the slots naming the row; the conversion to fp32 and the division by
                K + 1 in each run: delta_Gs = delta_G / div + 4 u |Gs|  (div = K + 1; 1 with layer weights).
  backward      both runs launch the same kernels on inputs delta apart: launch i computes c_add Gs + A h.  Its outputs differ by
                c_add delta_Gs + |A| delta_h (the exact map), + spmm_sum_bound(A, h) (conftest: covers the two fp32 evaluations),
                + 2 u (|c_add Gs| + |A| |h|) for the additions and the weight products.  bf16 storage rounds every launch but the
                last: each value moves by at most half a bf16 ulp, <= 2^-8 of its size (tests/storage_cases.py), so two values D
                apart are stored at most D + 2 * 2^-8 (|v| + D) apart (one may cross a rounding boundary).
                reg_ego: the epilogue adds the SAME fl(lam_e cnt) E0 in both runs (equal inputs), rounding the sum: 2 u more of
                |g_final|.  With edge dropout the bound uses |A| / keep (a kept entry is scaled by 1 / keep).
  last link     Adam's first moment of each run: g_rec = M + (M' - M) / w1, good to 2^-21 (|M| + |M'|) / w1: both slacks.
Every test prints the largest share of each bound it used."""
import os

import numpy as np
import pytest
import torch

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


def _model(pkg, path, mode, d, K, reg="propagated", dl=1, batch=64, **cfg):
    """A fresh GPU model of the storage graph (seed SC.MODEL_SEED, hand-set rows); cfg goes into world.config first."""
    w = SC.configure(pkg, (mode, d, K, dl, -1, reg), path, batch)
    for key in cfg.pop('_without', ()):
        w.config.pop(key)
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


def _oracle_losses(oracle, tr, batch, reg):
    """(loss, bpr, reg) of the oracle on the flattened batch at the trainer's current table, then its step."""
    adj = _G["adj"]
    csr = (adj.indptr, adj.indices, adj.data)
    fu, fp, fn = MN.flatten(batch)
    E = oracle.propagate(*csr, tr.e0, tr.K)
    if reg == "ego":
        bpr, rg = oracle.bpr_ego(E, tr.e0, SC.N_USERS, fu, fp, fn, SC.DECAY)[:2]
    else:
        bpr, rg = oracle.bpr(E, SC.N_USERS, fu, fp, fn, SC.DECAY)[:2]
    return tr.stageOne(fu, fp, fn), bpr, rg


# ---- 1. against the flattened batch on the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("reg", ["propagated", "ego"])
@pytest.mark.parametrize("R", MN.RS)
@pytest.mark.parametrize("K", MN.KS)
@pytest.mark.parametrize("d", MN.DS)
def test_steps_equal_the_oracle_on_the_flattened_batch(pkg, oracle, storage_graph, d, K, R, reg):
    """Four steps (64 / 64 / 37 / 1 samples) of fused_step with [B, R] negatives, fp32 storage, against oracle.Trainer stepping the
    flattened B R batches: the loss triple and the table at 3e-6.  The model is configured with --dense_last 0 and
    neg_ratio = R: _make_ctx must force the dense last layer.

    The batches are multineg_restatement.case_batches: seed 0 unless the oracle itself is more than half the yardstick from
    float64 on them (tests/test_multineg_host.py::test_the_oracle_can_judge_at_its_yardstick; eight reg_rows = ego cases at
    d >= 128, where its sequential fp32 sum of 3 d squares errs by up to 3e-6 on the B = 1 step)."""
    try:
        ds, m = _model(pkg, storage_graph, "fp32", d, K, reg, dl=0, neg_ratio=R)
        adj = _G["adj"]
        tr = oracle.Trainer(SC.N_USERS, adj.indptr, adj.indices, adj.data, m._table.cpu().numpy(), K, SC.DECAY, SC.LR, reg_rows=reg)
        worst, bad = 0.0, []
        for i, batch in enumerate(MN.case_batches(d, K, R, reg)):
            ref = _oracle_losses(oracle, tr, batch, reg)
            out = m.fused_step(_dev(batch[0]), _dev(batch[1]), _dev(batch[2])).cpu().numpy().astype(np.float64)
            err_t = float(np.abs(m._table.cpu().numpy().astype(np.float64) - tr.e0).max())
            errs = [abs(out[j] - ref[j]) for j in range(3)] + [err_t]
            worst = max(worst, max(errs))
            print(f"[multineg] oracle d{d} K{K} R{R} {reg} step {i + 1} B={len(batch[0])}: |loss| {errs[0]:.2e} |bpr| {errs[1]:.2e} |reg| {errs[2]:.2e} |table| {errs[3]:.2e}")
            bad += [(i + 1, name, float(e)) for name, e in zip(("loss", "bpr", "reg", "table"), errs) if not e < 3e-6]
            m.check_device_errors()
            assert m.adam_step == i + 1 and not bool(m._dev['G64'].any())
        assert m._dev['dense_last'] is True
        print(f"[multineg] oracle d{d} K{K} R{R} {reg} TOP share of 3e-6: {worst / 3e-6:.3f}")
        assert not bad, ("beyond 3e-6 of the oracle (step, quantity, distance)", bad)
    finally:
        pkg.world.configure([])


# ---- 2. against the existing fused step on the flattened batch --------------------------------------------------------------
def _c(n):
    return int(np.ceil(n / 64.0)) + 8


def _judge_pair(pkg, mN, mO, batch, R, K, d, mode, reg, step_no, tag, w=None, keep=1.0, void=None):
    """One step of both models from the SAME state -> {link: share of its bound}.  void: index of a sample that is voided in
    both runs (its id is bad in `batch`); the bounds then come from the sound samples."""
    adj, A = _G["adj"], _G["A"]
    ego = reg == "ego"
    B = len(batch[0])
    BR = B * R
    # one state: O takes N's table and moments (in place: the contexts keep their pointers), same step counter
    with torch.no_grad():
        mO._table.copy_(mN._table); mO._dev['adam_m'].copy_(mN._dev['adam_m']); mO._dev['adam_v'].copy_(mN._dev['adam_v'])
    assert mN.adam_step == mO.adam_step == step_no - 1
    before = _state(mN)
    fu, fp, fn = MN.flatten(batch)
    if void is not None:
        fn = fn.copy(); fn[void * R:(void + 1) * R] = SC.M_ITEMS              # every triplet of the voided sample is void for O
    outN = mN.fused_step(_dev(batch[0]), _dev(batch[1]), _dev(batch[2])).cpu().numpy().astype(np.float64)
    outO = mO.fused_step(_dev(fu), _dev(fp), _dev(fn)).cpu().numpy().astype(np.float64)
    afterN, afterO = _state(mN), _state(mO)
    tN = mN._dev['terms'].cpu().numpy().astype(np.float64)
    tO = mO._dev['terms'].cpu().numpy().astype(np.float64)
    termN, regN = tN[:B], tN[B:2 * B]
    termO, regO = tO[:BR].reshape(B, R).mean(1), tO[BR:2 * BR].reshape(B, R).mean(1)
    sound = np.ones(B, bool)
    if void is not None:
        sound[void] = False
        assert termN[void] == 0.0 and regN[void] == 0.0 and not tO[:BR].reshape(B, R)[void].any()
    sb = tuple(np.asarray(t)[sound] for t in batch)
    r = MN.step(A, SC.N_USERS, K, SC.DECAY, before["table"], sb, ego, w, B_norm=B)
    # ---- magnitudes
    wk = MN.layer_weights(K, w)
    X, T = r["E0"], abs(wk[0]) * r["E0"].abs()
    for k in range(1, K + 1):
        X = A @ X
        T = T + abs(wk[k]) * X.abs()
    T = T.numpy() * (1.0 + 2.0 ** -6)                                   # [N, d] >= |e| (storage roundings included)
    dE = 2 * (K + 2) * U * T if w is not None else np.zeros_like(T)
    ui, pi, ni = sb[0].astype(np.int64), SC.N_USERS + sb[1].astype(np.int64), SC.N_USERS + sb[2].astype(np.int64)
    au, ap, an = T[ui], T[pi], T[ni]                                     # [b, d], [b, d], [b, R, d]
    du, dp, dn = dE[ui], dE[pi], dE[ni]
    Sp, Sr = (au * ap).sum(1), (au[:, None, :] * an).sum(2)             # [b], [b, R]
    dx = 2 * (d + 2) * U * (Sp[:, None] + Sr) + (du[:, None, :] * (ap[:, None, :] + an) + au[:, None, :] * (dp[:, None, :] + dn)).sum(2)
    x = r["x"].numpy()
    t = np.abs(torch.nn.functional.logsigmoid(r["x"]).numpy()) * (1.0 + 2.0 ** -6) + dx      # |t_r| (at either run's x)
    s = 1.0 / (1.0 + np.exp(x))
    d_term = ((16 * U * t + s * dx).sum(1) + (R + 1) * U * t.sum(1)) / R + 1e-37
    CPT = d // min(d, 64)
    regterm = ((au * au).sum(1) + (ap * ap).sum(1) + (an * an).sum((1, 2)) / R)
    if ego:
        e0 = np.abs(r["E0"].numpy())
        regterm = (e0[ui] ** 2).sum(1) + (e0[pi] ** 2).sum(1) + (e0[ni] ** 2).sum((1, 2)) / R
        d_regx = 0.0
    else:
        d_regx = 2.0 * ((au * du).sum(1) + (ap * dp).sum(1) + (an * dn).sum((1, 2)) / R)
    d_reg = (2 * (R + 2) * CPT + 18) * U * regterm + d_regx + 1e-37
    share = {}
    share["term"] = float((np.abs(termN - termO)[sound] / d_term).max())
    share["regterm"] = float((np.abs(regN - regO)[sound] / d_reg).max())
    # ---- loss_out
    cc = (_c(B) + _c(BR)) * U
    b_bpr = cc * t.mean(1).sum() / B + d_term.sum() / B
    b_reg = 0.5 * (cc * regterm.sum() / B + d_reg.sum() / B)
    decay = float(np.float32(SC.DECAY))
    b_tot = b_bpr + decay * b_reg + 4 * U * (abs(outO[1]) + decay * abs(outO[2]))
    share["loss1"], share["loss2"], share["loss0"] = abs(outN[1] - outO[1]) / b_bpr, abs(outN[2] - outO[2]) / b_reg, abs(outN[0] - outO[0]) / b_tot
    # ---- gradient rows
    gb = np.abs(r["gb"].numpy()) * (1.0 + 2.0 ** -6)
    dgb = 16 * U * gb + gb * dx
    lam = 0.0 if ego else SC.DECAY / B
    lam_n = lam / R
    fx = 2.0 ** -51
    gbc, dgbc = gb[:, :, None], dgb[:, :, None]
    d_gn = 4 * U * (gbc * au[:, None, :] + lam_n * an) + dgbc * au[:, None, :] + gbc * du[:, None, :] + lam_n * dn + 2 * fx
    d_gp = ((R + 3) * U * gb.sum(1)[:, None] * au + 6 * U * lam * ap + dgb.sum(1)[:, None] * au + gb.sum(1)[:, None] * du + lam * dp + (R + 1) * fx)
    pn = ap[:, None, :] + an
    d_gu = ((R + 7) * U * (gbc * pn).sum(1) + 6 * U * lam * au + (dgbc * pn).sum(1) + (gbc * (dp[:, None, :] + dn)).sum(1) + lam * du + (R + 1) * fx)
    dG = np.zeros_like(T)
    np.add.at(dG, ui, d_gu); np.add.at(dG, pi, d_gp); np.add.at(dG, ni.reshape(-1), d_gn.reshape(-1, d))
    div = 1.0 if w is not None else float(K + 1)
    G = np.abs(r["G"].numpy()) * (1.0 + 2.0 ** -6) + dG
    Gs = G / div
    dGs = dG / div + 4 * U * Gs
    aabs = abs(adj).astype(np.float64) / keep
    absadj = aabs.tocsr()
    h, dh = (abs(wk[K]) * div if w is not None else 1.0) * Gs, None
    D = None
    for i in range(K):
        k = K - i                                                        # launch i computes w_{k-1} G + A h_k
        c_add = abs(wk[k - 1]) * div if w is not None else 1.0
        if i == 0:
            cin = abs(wk[K]) if w is not None else 1.0
            h, dh = cin * Gs, cin * dGs + (2 * U * cin * Gs if w is not None else 0.0)
        Ah = absadj @ h
        D = c_add * dGs + absadj @ dh + spmm_sum_bound(absadj.indptr, absadj.data, absadj.indices, h) + 2 * U * (c_add * Gs + Ah)
        v = c_add * Gs + Ah
        if i < K - 1 and mode == "bf16":
            D = D + 2.0 ** -7 * (v + D)
        h, dh = v + D, D
    g_abs = h
    if ego:
        D = D + 2 * U * (g_abs + (SC.DECAY / BR) * r["cnt"].numpy()[:, None] * np.abs(r["E0"].numpy()))
    slack = 2.0 ** -21 * (np.abs(before["M"]) + np.abs(afterN["M"])) / W1 + 2.0 ** -21 * (np.abs(before["M"]) + np.abs(afterO["M"])) / W1
    gN = before["M"] + (afterN["M"] - before["M"]) / W1
    gO = before["M"] + (afterO["M"] - before["M"]) / W1
    share["grad"] = float((np.abs(gN - gO) / (D + slack + 1e-300)).max())
    assert float(np.abs(gN).max()) > 0.0
    slackN = 2.0 ** -21 * (np.abs(before["M"]) + np.abs(afterN["M"])) / W1
    share["adam"] = _adam_checks((tag, "table"), before["table"], before["M"], before["V"], afterN["table"], afterN["M"], afterN["V"],
                                 gN, slackN, step_no, False)
    print(f"[multineg] pair {tag}: shares " + " ".join(f"{k}={v:.3f}" for k, v in share.items()))
    return share


def _run_pair(pkg, path, mode, d, K, R, reg="propagated", w=None, dropout=None, sizes=MN.BATCH_SIZES):
    try:
        cfg = {}
        if w is not None:
            cfg['layer_weights'] = str(list(w))
        if dropout is not None:
            cfg.update({'dropout': 1, 'keep_prob': dropout, 'seed': 2020})
        cap = max(sizes)
        _, mN = _model(pkg, path, mode, d, K, reg, dl=1, batch=cap, neg_ratio=R, **cfg)
        mN._state(max_batch=cap, need_ctx=True)
        _, mO = _model(pkg, path, mode, d, K, reg, dl=1, batch=cap * R, **cfg)
        mO._state(max_batch=cap * R, need_ctx=True)
        assert mN._dev['dense_last'] and mO._dev['dense_last']
        top, bad = {}, []
        for i, batch in enumerate(MN.make_batches(d, K, R, sizes=sizes)):
            tag = f"{mode} d{d} K{K} R{R} {reg}" + (" wts" if w is not None else "") + (f" keep{dropout}" if dropout else "") + f" step {i + 1} B={len(batch[0])}"
            share = _judge_pair(pkg, mN, mO, batch, R, K, d, mode, reg, i + 1, tag, w=w, keep=dropout or 1.0)
            for k_, v in share.items():
                top[k_] = max(top.get(k_, 0.0), v)
                if not v <= 1.0:
                    bad.append((tag, k_, v))
            mN.check_device_errors(); mO.check_device_errors()
            assert not bool(mN._dev['G64'].any()) and mN.adam_step == mO.adam_step == i + 1
        print(f"[multineg] pair {mode} d{d} K{K} R{R} {reg} TOP: " + " ".join(f"{k_}={v:.3f}" for k_, v in top.items()))
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
@pytest.mark.parametrize("R", MN.RS)
@pytest.mark.parametrize("K", MN.KS)
@pytest.mark.parametrize("d", MN.DS)
def test_steps_equal_the_existing_step_on_the_flattened_batch(pkg, storage_graph, d, K, R, mode):
    """Per-sample terms, loss_out, the gradient recovered from Adam's first moment and Adam itself, new kernel against
    k_triplet_dense on the flattened batch from one state, each within the bound derived in the module docstring."""
    _run_pair(pkg, storage_graph, mode, d, K, R)


# N reduces B per-sample terms, scaled by inv_R, with reduce_loss_wave (terms[lane], terms[lane + 64], ..): no batch above has
# more than 64 samples, so its second addition is first taken here (MN.LARGE_BATCH_SIZES = 65, 300; c(B) in the loss_out line
# counts it).  O reduces B R terms as before.  Every width, both storages, K in {1, 3}, both reg rows, R = 2 and 16.
_LARGE_CASES = [(32, 3, 16, "fp32", "propagated"), (64, 1, 2, "bf16", "ego"), (128, 1, 16, "bf16", "propagated"), (256, 3, 2, "fp32", "ego")]
assert {c[0] for c in _LARGE_CASES} == set(MN.DS) and {c[1] for c in _LARGE_CASES} == {1, 3} and {c[2] for c in _LARGE_CASES} == set(MN.LARGE_RS)
assert {c[3] for c in _LARGE_CASES} == {"fp32", "bf16"} and {c[4] for c in _LARGE_CASES} == {"propagated", "ego"}
assert all(_c(B) - 8 >= 2 for B in MN.LARGE_BATCH_SIZES)


@pytest.mark.parametrize("d,K,R,mode,reg", [pytest.param(*c, id=f"d{c[0]}-K{c[1]}-R{c[2]}-{c[3]}-{c[4]}") for c in _LARGE_CASES])
def test_pair_beyond_one_wave_of_terms(pkg, storage_graph, d, K, R, mode, reg):
    """Batches of 65 and 300 samples (contexts of 300 and 300 R): the links of
    test_steps_equal_the_existing_step_on_the_flattened_batch within the same bounds."""
    _run_pair(pkg, storage_graph, mode, d, K, R, reg, sizes=MN.LARGE_BATCH_SIZES)


def test_pair_with_reg_rows_ego(pkg, storage_graph):
    """reg_ego: the slot counts (R per user / positive slot, 1 per negative slot) with decay / (B R) in the epilogue."""
    _run_pair(pkg, storage_graph, "fp32", 64, 2, 5, reg="ego")


def test_pair_with_layer_weights(pkg, storage_graph):
    _run_pair(pkg, storage_graph, "fp32", 64, 3, 5, w=[0.4, 0.1, 0.3, 0.2])


def test_pair_with_edge_dropout(pkg, storage_graph):
    """keep 0.6, same seed and step counter on both models: the same masks in the SpMMs, nothing in the batch-row kernel."""
    _run_pair(pkg, storage_graph, "fp32", 64, 3, 5, dropout=0.6)


# ---- 3. the epoch call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,K,reg", [("fp32", 1, "ego"), ("fp32", 3, "propagated"), ("bf16", 2, "propagated")])
def test_epoch_equals_the_loop_of_steps_bitwise(pkg, storage_graph, mode, K, reg):
    """lgcn_train_epoch_multi over T = 165 (batches of 64, 64, 37, column stride T) against the loop of lgcn_train_step_multi:
    loss rows, table, both Adam moments bit for bit; G64 zero and no device error afterwards."""
    try:
        R, B, T, d = 5, 64, 165, 64
        seq = MN.make_batches(d, K, R)[:3]
        u = np.concatenate([b[0] for b in seq]); p = np.concatenate([b[1] for b in seq]); n = np.concatenate([b[2] for b in seq])
        assert len(u) == T
        negs_rt = _dev(np.ascontiguousarray(n.T))                           # [R, T]
        _, a = _model(pkg, storage_graph, mode, d, K, reg, neg_ratio=R)
        want = a.fused_epoch(_dev(u), _dev(p), negs_rt, B)
        a.check_device_errors()
        _, b = _model(pkg, storage_graph, mode, d, K, reg, neg_ratio=R)
        first = b._table.detach().clone()
        got = [b.fused_step(_dev(u[t:t + B]), _dev(p[t:t + B]), _dev(n[t:t + B])) for t in range(0, T, B)]
        b.check_device_errors()
        assert a.adam_step == b.adam_step == 3 and want.shape == (3, 3)
        assert torch.equal(torch.stack(got), want), (torch.stack(got), want)
        assert torch.equal(a._table, b._table), int((a._table != b._table).sum())
        assert torch.equal(a._dev['adam_m'], b._dev['adam_m']) and torch.equal(a._dev['adam_v'], b._dev['adam_v'])
        assert not bool(a._dev['G64'].any()) and not bool(b._dev['G64'].any())
        assert float((b._table - first).abs().max()) > 1e-4                 # (it trained)
        # the [T, R] layout (the sampler's S[:, 2:]) is the same call
        _, c = _model(pkg, storage_graph, mode, d, K, reg, neg_ratio=R)
        assert torch.equal(c.fused_epoch(_dev(u), _dev(p), _dev(n), B), want) and torch.equal(c._table, a._table)
    finally:
        pkg.world.configure([])


# ---- 4. lgcn_apply_perm_multi -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 5])
def test_apply_perm_multi(pkg, R):
    L = pkg._lib
    lib = L.load()
    T, cols = 1000, 2 + R
    rng = np.random.Generator(np.random.PCG64(R))
    S_ = rng.integers(0, 10 ** 6, (T, cols)).astype(np.int32)
    perm = rng.permutation(T).astype(np.int64)
    dS, dperm = _dev(S_), _dev(perm, torch.int64)
    users = torch.empty(T, dtype=torch.int32, device=DEV); pos = torch.empty_like(users)
    negs = torch.empty(R, T, dtype=torch.int32, device=DEV)
    L.check(lib.lgcn_apply_perm_multi(L.tp(dS), cols, L.tp(dperm), T, L.tp(users), L.tp(pos), L.tp(negs), R, L.current_stream()), "lgcn_apply_perm_multi")
    want = S_[perm]
    assert np.array_equal(users.cpu().numpy(), want[:, 0]) and np.array_equal(pos.cpu().numpy(), want[:, 1])
    for r in range(R):
        assert np.array_equal(negs[r].cpu().numpy(), want[:, 2 + r]), r
    if R == 1:
        u1 = torch.empty_like(users); p1 = torch.empty_like(users); n1 = torch.empty_like(users)
        L.check(lib.lgcn_apply_perm(L.tp(dS), cols, L.tp(dperm), T, L.tp(u1), L.tp(p1), L.tp(n1), L.current_stream()), "lgcn_apply_perm")
        assert torch.equal(u1, users) and torch.equal(p1, pos) and torch.equal(n1, negs[0])
    # no permutation: the rows in order
    L.check(lib.lgcn_apply_perm_multi(L.tp(dS), cols, None, T, L.tp(users), L.tp(pos), L.tp(negs), R, L.current_stream()), "lgcn_apply_perm_multi")
    assert np.array_equal(negs[R - 1].cpu().numpy(), S_[:, 1 + R])


# ---- 5. a voided sample -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2])
def test_voided_sample(pkg, storage_graph, K):
    """One sample with ONE out-of-range negative: zero terms, and the step is the existing step with that sample's R triplets
    voided (zero gradient from all of its 2 + R rows), within the bound of the pair comparison; the other samples' terms are
    the bits of the clean run; check_device_errors() raises on both."""
    try:
        R, d, void = 5, 64, 3
        u, p, n = MN.make_batches(d, K, R)[0]
        nbad = n.copy(); nbad[void, 2] = SC.M_ITEMS
        _, clean = _model(pkg, storage_graph, "fp32", d, K, neg_ratio=R)
        clean.fused_step(_dev(u), _dev(p), _dev(n))
        t_clean = clean._dev['terms'].cpu().numpy().copy()
        _, mN = _model(pkg, storage_graph, "fp32", d, K, neg_ratio=R)
        mN._state(max_batch=64, need_ctx=True)
        _, mO = _model(pkg, storage_graph, "fp32", d, K, batch=64 * R)
        mO._state(max_batch=64 * R, need_ctx=True)
        share = _judge_pair(pkg, mN, mO, (u, p, nbad), R, K, d, "fp32", "propagated", 1, f"void K{K}", void=void)
        assert all(v <= 1.0 for v in share.values()), share
        t_void = mN._dev['terms'].cpu().numpy()
        keep = np.arange(64) != void
        assert np.array_equal(t_void[:64][keep], t_clean[:64][keep]) and np.array_equal(t_void[64:128][keep], t_clean[64:128][keep])
        for m in (mN, mO):
            with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
                m.check_device_errors()
        assert not bool(mN._dev['G64'].any())
    finally:
        pkg.world.configure([])


# ---- 6. R = 1 is untouched --------------------------------------------------------------------------------------------------
def test_neg_ratio_one_is_the_parents_path(pkg, storage_graph):
    """neg_ratio 1 and 1-D negatives: fused_epoch calls lgcn_train_epoch, the fold engages, and the result is bit for bit that of a
    model built without the config key; [T, 1] negatives take the same path."""
    try:
        d, K, B = 64, 2, 64
        rng = np.random.Generator(np.random.PCG64(5))
        T = 165
        u = rng.integers(0, SC.N_USERS, T); p = rng.integers(0, SC.M_ITEMS, T); n = rng.integers(0, SC.M_ITEMS, T)
        res = []
        for form in ("key", "nokey", "2d"):
            _, m = _model(pkg, storage_graph, "fp32", d, K, dl=0, **({'_without': ('neg_ratio',)} if form == "nokey" else {'neg_ratio': 1}))
            assert ('neg_ratio' in m.config) == (form != "nokey")
            lib = pkg._lib.load()
            losses = m.fused_epoch(_dev(u), _dev(p), _dev(n[:, None]) if form == "2d" else _dev(n), B)
            m.check_device_errors()
            assert m._dev['dense_last'] is False
            assert int(lib.lgcn_ctx_folded_steps(m._dev['ctx'])) == 3, form          # lgcn_train_epoch ran, folded
            res.append((losses.clone(), m._table.detach().clone(), m._dev['adam_m'].clone(), m._dev['adam_v'].clone()))
        for other in res[1:]:
            for a, b in zip(res[0], other):
                assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def _refused(pkg, m, R=4, B=8):
    """Both new calls on the model's context -> asserts rc 3 naming the negative ratio and an untouched state."""
    L = pkg._lib
    lib = L.load()
    st = m._state(max_batch=64, need_ctx=True)
    before = (m._table.detach().clone(), st['adam_m'].clone(), st['adam_v'].clone(), int(lib.lgcn_ctx_get_step(st['ctx'])),
              st['G64'].clone(), st['terms'].clone())
    u = _dev(np.arange(B)); p = _dev(np.arange(B)); negs = _dev(np.arange(max(R, 1) * B).reshape(max(R, 1), B) % SC.M_ITEMS)
    loss = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
    for call in ("step", "epoch"):
        if call == "step":
            rc = lib.lgcn_train_step_multi(st['ctx'], L.tp(u), L.tp(p), L.tp(negs), B, R, B, L.tp(loss), L.current_stream())
        else:
            rc = lib.lgcn_train_epoch_multi(st['ctx'], L.tp(u), L.tp(p), L.tp(negs), R, B, B, L.tp(loss), L.current_stream())
        msg = lib.lgcn_last_error().decode()
        assert rc == 3 and "negative ratio" in msg, (call, rc, msg)
    torch.cuda.synchronize()
    after = (m._table, st['adam_m'], st['adam_v'], int(lib.lgcn_ctx_get_step(st['ctx'])), st['G64'], st['terms'])
    for a, b in zip(before, after):
        assert (a == b) if isinstance(a, int) else torch.equal(a, b)
    assert bool((loss == -7.0).all())
    m.check_device_errors()


def test_refusals_leave_everything_untouched(pkg, storage_graph):
    try:
        _, m = _model(pkg, storage_graph, "fp32", 64, 2, dl=0)
        _refused(pkg, m)                                                    # dense_last = 0
        _, m = _model(pkg, storage_graph, "fp8", 64, 2, dl=1)
        _refused(pkg, m)                                                    # fp8 storage
        _, m = _model(pkg, storage_graph, "fp32", 64, 2, dl=1, use_pop_gate=True)
        _refused(pkg, m)                                                    # the popularity gate
        _, m = _model(pkg, storage_graph, "fp32", 64, 2, dl=1, use_item_item=True, i2i_build='cooc', i2i_alpha=0.5)
        assert m.i2i_active
        _refused(pkg, m)                                                    # item-item smoothing
        _, m = _model(pkg, storage_graph, "fp32", 64, 2, dl=1)
        _refused(pkg, m, R=0)
        _refused(pkg, m, R=17)
        # ... and the same context takes a sound call afterwards
        u, p, n = MN.make_batches(64, 2, 2)[0]
        out = m.fused_step(_dev(u), _dev(p), _dev(n))
        m.check_device_errors()
        assert bool(torch.isfinite(out).all()) and m.adam_step == 1
    finally:
        pkg.world.configure([])


# ---- 8. through the module surface ------------------------------------------------------------------------------------------
def test_training_epoch_through_procedure(pkg, oracle, storage_graph, tmp_path):
    """world.config['neg_ratio'] = 4, one Procedure.BPR_train_original epoch (host sampler with neg_num = 4, the epoch permutation,
    lgcn_apply_perm_multi, lgcn_train_epoch_multi) against the flattened-batch oracle fed the same sampled and shuffled rows, at
    3e-6; the sampler's rand() stream stands where the oracle sampler's stands."""
    import csv
    try:
        R, B, d, K = 4, 256, 64, 2
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, neg_ratio=R, prefetch_epoch=0, sampler='cpp',
                       checkpoint_dir=os.path.join(str(tmp_path), "ckpt"))
        pkg.world.tensorboard = 0
        adj = _G["adj"]
        tr = oracle.Trainer(SC.N_USERS, adj.indptr, adj.indices, adj.data, m._table.cpu().numpy(), K, SC.DECAY, SC.LR)
        indptr, indices = pkg.utils._pos_csr(ds)
        oracle.srand(31); oracle.np_seed(32)
        S_ = oracle.sample_negative(ds.n_users, ds.m_items, ds.trainDataSize, indptr, indices, neg_num=R)
        T = len(S_)
        S_ = S_[oracle.np_shuffle_arange(T)]
        ref = [tr.stageOne(*MN.flatten((S_[t:t + B, 0], S_[t:t + B, 1], S_[t:t + B, 2:]))) for t in range(0, T, B)]
        pkg.sampling.seed(31); pkg.utils.set_seed(32)
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        info = pkg.Procedure.BPR_train_original(ds, m, bpr, 1)
        assert info.startswith("loss")
        assert m.adam_step == len(ref) == (T + B - 1) // B
        with open(os.path.join(pkg.world.config['checkpoint_dir'], 'train_epoch_metrics.csv')) as f:
            rows = list(csv.reader(f))
        got_mean = float(rows[-1][1])
        want_mean = float(np.sum(ref)) / (T // B + 1)
        err_t = float(np.abs(m._table.cpu().numpy().astype(np.float64) - tr.e0).max())
        print(f"[multineg] procedure: |mean loss| {abs(got_mean - want_mean):.2e} |table| {err_t:.2e}")
        assert abs(got_mean - want_mean) < 3e-6 and err_t <= 3e-6
        assert pkg.sampling.randint(10 ** 6) == oracle.randint(10 ** 6)
        # the sampler's rows as they come, [T, R], go through stageOne too
        out = bpr.stageOne(_dev(S_[:B, 0]), _dev(S_[:B, 1]), _dev(S_[:B, 2:]))
        assert np.isfinite(out) and m.adam_step == len(ref) + 1
    finally:
        pkg.world.configure([])

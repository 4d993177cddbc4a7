"""Several negatives per positive (--neg_ratio) without a device: the float64 restatement of the step
(tests/multineg_restatement.py) is pinned to torch autograd of the written loss, to its own R = 1 run on the flattened batch and
to oracle.Trainer on the flattened batch; the C ABI, the flag, the refusals that need no device and the host sampler."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multineg_restatement as MN                # noqa: E402
import storage_cases as SC                       # noqa: E402
import storage_restatement as S                  # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import REPO                        # noqa: E402

_CACHE = {}
CASES = [(32, 1, 2, "propagated"), (64, 2, 5, "ego"), (32, 3, 16, "propagated"), (64, 3, 5, "propagated"), (32, 2, 2, "ego")]


def _inputs(pkg, path, d):
    """(dataset, adjacency CSR, dense float64 A, initial fp32 table with the hand-set rows) for an embedding width"""
    try:
        if ("tab", d) not in _CACHE:
            ds, m = SC.make_model(pkg, ("bf16", d, 1, 1, -1, "propagated"), path)
            if "adj" not in _CACHE:
                adj = ds.getSparseGraphCSR()
                _CACHE["adj"], _CACHE["A"], _CACHE["ds"] = adj, S.dense_adj(adj), ds
            _CACHE[("tab", d)] = m._table.detach().numpy().copy()
        return _CACHE["ds"], _CACHE["adj"], _CACHE["A"], _CACHE[("tab", d)]
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("d,K,R,reg", CASES)
def test_restatement_is_the_autograd_of_the_written_loss(pkg, storage_graph, d, K, R, reg):
    """The three kinds of gradient rows, the backward chain and the reg_ego term against torch float64 autograd on a dense A_hat;
    with layer weights on one case."""
    _, _, A, table = _inputs(pkg, storage_graph, d)
    for w in (None, [0.4, 0.1, 0.3, 0.2][:K + 1]) if (d, K) == (64, 3) else (None,):
        for batch in MN.make_batches(d, K, R):
            r = MN.step(A, SC.N_USERS, K, SC.DECAY, table, batch, reg == "ego", w)
            E0 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
            E = MN.propagate(A, E0, K, w)
            E.retain_grad()
            loss, bpr, reg_l = MN.loss(E, E0, SC.N_USERS, batch, SC.DECAY, reg == "ego")
            loss.backward()
            for got, ref in zip(r["loss_out"], (loss.detach(), bpr.detach(), reg_l.detach())):
                assert abs(float(got) - float(ref)) <= 1e-13 * max(1.0, abs(float(ref)))
            scale = float(E0.grad.abs().max())
            assert float((r["G"] - E.grad).abs().max()) <= 1e-12 * scale
            assert float((r["g_final"] - E0.grad).abs().max()) <= 1e-12 * scale
            B = len(batch[0])          # the per-sample terms are scaled for the three-slot step's reduction with 1 / B
            assert abs(-float(r["term"].sum()) / B - float(bpr.detach())) <= 1e-13 and abs(0.5 * float(r["regterm"].sum()) / B - float(reg_l.detach())) <= 1e-13


@pytest.mark.parametrize("d,K,R,reg", CASES)
def test_restatement_is_its_own_flattened_run(pkg, storage_graph, d, K, R, reg):
    """The specification: the step on (u, p, n_1..n_R) is the R = 1 step on the B R triplets (u, p, n_r), to float64 round-off --
    loss triple, gradient table, reg_ego counts (R flattened slots = one slot of weight R), the final gradient."""
    _, _, A, table = _inputs(pkg, storage_graph, d)
    for batch in MN.make_batches(d, K, R):
        r = MN.step(A, SC.N_USERS, K, SC.DECAY, table, batch, reg == "ego")
        fu, fp, fn = MN.flatten(batch)
        f = MN.step(A, SC.N_USERS, K, SC.DECAY, table, (fu, fp, fn[:, None]), reg == "ego")
        for got, ref in zip(r["loss_out"], f["loss_out"]):
            assert abs(float(got) - float(ref)) <= 1e-13 * max(1.0, abs(float(ref)))
        scale = float(f["g_final"].abs().max())
        assert float((r["G"] - f["G"]).abs().max()) <= 1e-12 * scale
        assert float((r["g_final"] - f["g_final"]).abs().max()) <= 1e-12 * scale
        assert torch.equal(r["cnt"], f["cnt"])


@pytest.mark.parametrize("d,K,R,reg", CASES)
def test_restatement_is_the_oracle_on_the_flattened_batch(pkg, oracle, storage_graph, d, K, R, reg):
    """oracle.Trainer steps the flattened B R batches; the restatement steps the samples (fp32 state between steps, as the
    device holds it): loss and table at the project's yardstick for oracle comparisons, atol 3e-6 (test_fused_step_vs_oracle)."""
    _, adj, A, table = _inputs(pkg, storage_graph, d)
    tr = oracle.Trainer(SC.N_USERS, adj.indptr, adj.indices, adj.data, table, K, SC.DECAY, SC.LR, reg_rows=reg)
    p = table.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for i, batch in enumerate(MN.case_batches(d, K, R, reg)):
        r = MN.step(A, SC.N_USERS, K, SC.DECAY, p, batch, reg == "ego")
        l_ref = tr.stageOne(*MN.flatten(batch))
        assert abs(float(r["loss_out"][0]) - l_ref) < 3e-6, (i, float(r["loss_out"][0]), l_ref)
        p, m, v = MN.adam(p, m, v, r["g_final"].numpy(), i + 1, SC.LR)
        p, m, v = (t.astype(np.float32).astype(np.float64) for t in (p, m, v))
        np.testing.assert_allclose(p, tr.e0, rtol=0, atol=3e-6)


def _oracle_triple(oracle, tr, adj, batch, reg):
    """(loss, bpr, reg) of the oracle on the flattened batch at the trainer's table, then its step."""
    csr = (adj.indptr, adj.indices, adj.data)
    fu, fp, fn = MN.flatten(batch)
    E = oracle.propagate(*csr, tr.e0, tr.K)
    if reg == "ego":
        bpr, rg = oracle.bpr_ego(E, tr.e0, SC.N_USERS, fu, fp, fn, SC.DECAY)[:2]
    else:
        bpr, rg = oracle.bpr(E, SC.N_USERS, fu, fp, fn, SC.DECAY)[:2]
    return tr.stageOne(fu, fp, fn), bpr, rg


@pytest.mark.parametrize("reg", ["propagated", "ego"])
@pytest.mark.parametrize("R", MN.RS)
@pytest.mark.parametrize("K", MN.KS)
@pytest.mark.parametrize("d", MN.DS)
def test_the_oracle_can_judge_at_its_yardstick(pkg, oracle, storage_graph, d, K, R, reg):
    """The condition behind multineg_restatement.BATCH_SEED, for every case tests/test_gpu_multineg.py compares with the oracle at
    3e-6: on the oracle's own trajectory over the case's batches, its fp32 loss triple is within half that yardstick of the float64
    restatement at the same table -- else the comparison would measure the oracle's rounding.  A seed is above 0 only where seed 0
    fails this."""
    _, adj, A, table = _inputs(pkg, storage_graph, d)

    def oracle_error(seed):
        tr = oracle.Trainer(SC.N_USERS, adj.indptr, adj.indices, adj.data, table, K, SC.DECAY, SC.LR, reg_rows=reg)
        worst = 0.0
        for batch in MN.make_batches(d, K, R, seed):
            r = MN.step(A, SC.N_USERS, K, SC.DECAY, tr.e0, batch, reg == "ego")          # (before the trainer's step)
            ref = _oracle_triple(oracle, tr, adj, batch, reg)
            worst = max(worst, max(abs(float(a) - b) for a, b in zip(r["loss_out"], ref)))
        return worst

    seed = MN.BATCH_SEED.get((d, K, R, reg), 0)
    assert oracle_error(seed) <= MN.ORACLE_ROOM, (seed, oracle_error(seed))
    for lower in range(seed):
        assert oracle_error(lower) > MN.ORACLE_ROOM, ("a lower seed meets the condition", lower)


def test_batches_hold_the_cases_the_kernel_can_get_wrong():
    for d, K, R, seed in [(64, 2, R, 0) for R in MN.RS] + [(*key[:3], seed) for key, seed in MN.BATCH_SEED.items()]:
        seq = MN.make_batches(d, K, R, seed)
        assert [len(b[0]) for b in seq] == [64, 64, 37, 1]
        negs = np.concatenate([b[2].reshape(-1) for b in seq])
        assert SC.ISOLATED_ITEM in negs and SC.M_ITEMS - 1 in negs
        for u, p, n in seq:
            assert n.shape == (len(u), R)
            assert any(len(set(row.tolist())) < R for row in n)                      # the same item twice in one sample's negatives
            if len(u) > 8:
                assert len(set(u.tolist())) < len(u)                                 # a user in several samples
                assert any(p[b] in n[np.arange(len(u)) != b] for b in range(len(u)))  # a positive that is another sample's negative


# ---- the C ABI, the flag, the refusals ------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lgcn_apply_perm_multi", "lgcn_train_step_multi", "lgcn_train_epoch_multi")


def test_new_symbols_are_declared_bound_and_exported_with_abi_13(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lgcn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", hdr))
    lib = pkg._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lgcn_abi_version() == pkg._lib.ABI_VERSION == 13
    assert pkg._lib.MAX_NEG_RATIO == int(re.search(r"#define\s+LGCN_MAX_NEG_RATIO\s+(\d+)", hdr).group(1)) == 16


def test_entry_points_refuse_before_touching_anything(pkg):
    """What the host can refuse with no device: null arguments and a negative ratio out of range (rc 3, the message names it)."""
    lib = pkg._lib.load()
    one = np.zeros(8, np.int32)
    for R in (0, 17):
        rc = lib.lgcn_apply_perm_multi(pkg._lib.npp(one), 2 + max(R, 0), None, 1, pkg._lib.npp(one), pkg._lib.npp(one), pkg._lib.npp(one), R, None)
        assert rc == 3 and b"negative ratio" in lib.lgcn_last_error()
    assert lib.lgcn_apply_perm_multi(pkg._lib.npp(one), 3, None, 1, pkg._lib.npp(one), pkg._lib.npp(one), pkg._lib.npp(one), 2, None) == 3      # s_cols < 2 + R
    assert lib.lgcn_train_step_multi(None, None, None, None, 1, 2, 1, None, None) == 3
    assert lib.lgcn_train_epoch_multi(None, None, None, None, 2, 1, 1, None, None) == 3


def test_neg_ratio_flag(pkg):
    w = pkg.world
    try:
        w.configure([])
        assert w.config['neg_ratio'] == 1
        w.configure(['--neg_ratio', '4'])
        assert w.config['neg_ratio'] == 4
        with pytest.raises(SystemExit):
            w.configure(['--neg_ratio', 'many'])
    finally:
        w.configure([])


def _model_with(pkg, path, cls="LightGCN", **cfg):
    w = SC.configure(pkg, ("fp32", 32, 2, 1, -1, "propagated"), path)
    w.config.update(cfg)
    ds = pkg.dataloader.Loader(w.config, path=path)
    return ds, getattr(pkg.model, cls)(w.config, ds)


def test_refusals_that_need_no_device_name_the_flag(pkg, storage_graph):
    try:
        for cfg in ({'act_dtype': 'fp8', 'latent_dim_rec': 64}, {'use_pop_gate': True}, {'use_item_item': True}):
            with pytest.raises(pkg._lib.LgcnError, match="--neg_ratio"):
                _model_with(pkg, storage_graph, neg_ratio=4, **cfg)
        with pytest.raises(pkg._lib.LgcnError, match="--neg_ratio"):
            _model_with(pkg, storage_graph, cls="PureMF", neg_ratio=2)
        for bad in (0, 17):
            with pytest.raises(ValueError, match="--neg_ratio"):
                _model_with(pkg, storage_graph, neg_ratio=bad)
        ds, m = _model_with(pkg, storage_graph, neg_ratio=4)
        assert m.neg_ratio == 4
        with pytest.raises(RuntimeError, match="--neg_ratio"):
            pkg.parallel.DataParallelBPR(m, pkg.world.config)
        # the reference's Python sampler draws one negative: --sampler python with R > 1 is an error, not three columns
        pkg.world.config['sampler'] = 'python'
        with pytest.raises(pkg._lib.LgcnError, match="--neg_ratio"):
            pkg.Procedure.sample_epoch_to_device(ds, "cpu")
        # neg_ratio 1 builds what it always built
        _, m1 = _model_with(pkg, storage_graph)
        assert m1.neg_ratio == 1
    finally:
        pkg.world.configure([])


def test_autograd_loss_accepts_two_dimensional_negatives_on_the_host_tables(pkg, storage_graph):
    """LightGCN.bpr_loss with [B, R] negatives is the written loss (the propagation itself needs the device: the embeddings are
    injected here, which is all getEmbedding adds to them)."""
    try:
        ds, m = _model_with(pkg, storage_graph, neg_ratio=5)
        _, _, A, _ = _inputs(pkg, storage_graph, 32)
        SC.configure(pkg, ("fp32", 32, 2, 1, -1, "propagated"), storage_graph)
        E0 = m._table.detach().double()
        E = MN.propagate(A, E0, 2)
        m.computer = lambda: (E[:SC.N_USERS].float(), E[SC.N_USERS:].float())
        u, p, n = MN.make_batches(32, 2, 5)[0]
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
        bpr, reg = m.bpr_loss(t(u), t(p), t(n))
        _, bpr_ref, reg_ref = MN.loss(E, E0, SC.N_USERS, (u, p, n), SC.DECAY)
        assert abs(float(bpr) - float(bpr_ref)) < 1e-6 and abs(float(reg) - float(reg_ref)) < 1e-6
        bpr_t, reg_t = m.bpr_loss(t(u), t(p), t(n).t().contiguous())                 # the [R, B] layout
        assert abs(float(bpr_t) - float(bpr)) < 1e-6 and abs(float(reg_t) - float(reg)) < 1e-6      # (fp32 sums in another order)
    finally:
        pkg.world.configure([])


# ---- the host sampler -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 5])
def test_host_sampler_rows_of_two_plus_r_ids(pkg, oracle, storage_graph, R):
    try:
        ds, _, _, _ = _inputs(pkg, storage_graph, 32)
        pkg.world.configure([])
        pkg.world.config['sampler'] = 'cpp'
        pkg.sampling.seed(77)
        S_ = pkg.utils.UniformSample_original(ds, R)
        per = ds.trainDataSize // ds.n_users
        assert S_.shape == (ds.n_users * per, 2 + R)
        indptr, indices = pkg.utils._pos_csr(ds)
        oracle.srand(77)
        ref = oracle.sample_negative(ds.n_users, ds.m_items, ds.trainDataSize, indptr, indices, neg_num=R)
        assert np.array_equal(np.asarray(S_), ref)                                   # row for row
        assert pkg.sampling.randint(10 ** 6) == oracle.randint(10 ** 6)               # and the stream stands where the oracle's stands
        for row in np.asarray(S_)[:: max(1, len(S_) // 400)]:
            pos = set(ds.allPos[int(row[0])].tolist())
            assert int(row[1]) in pos and not (set(row[2:].tolist()) & pos)
    finally:
        pkg.world.configure([])

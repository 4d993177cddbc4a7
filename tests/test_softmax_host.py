"""The sampled-softmax loss (--loss softmax) without a device: the float64 restatement of the step
(tests/softmax_restatement.py) is pinned to torch autograd of the written loss and, at R = 1 and tau = 1, to the BPR
restatement (tests/multineg_restatement.py); the package's autograd loss; the saturation batch of the GPU tests; the flags,
the refusals that need no device and the C ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multineg_restatement as MN                # noqa: E402
import softmax_restatement as SM                 # noqa: E402
import storage_cases as SC                       # noqa: E402
import storage_restatement as S                  # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import REPO                        # noqa: E402

_CACHE = {}


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


# ---- 1. the restatement is the autograd of the written loss ------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1.0, 0.2])
@pytest.mark.parametrize("R", [1, 2, 16])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("d", [32, 256])
def test_restatement_is_the_autograd_of_the_written_loss(pkg, storage_graph, d, K, R, tau):
    """g_final, G and the loss triple against torch float64 autograd of the loss written with torch.logsumexp, both reg rows,
    with and without layer weights, on the first and the last (B = 1) batch: 1e-12 relative, float64 against float64."""
    _, _, A, table = _inputs(pkg, storage_graph, d)
    batches = SM.make_batches(d, K, max(R, 2))
    for reg in ("propagated", "ego"):
        for w in (None, [0.4, 0.1, 0.3, 0.2][:K + 1]):
            for batch in (batches[0], batches[3]):
                batch = (batch[0], batch[1], batch[2][:, :R])
                r = SM.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg == "ego", w)
                E0 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
                E = SM.propagate(A, E0, K, w)
                E.retain_grad()
                loss, sm, reg_l = SM.loss(E, E0, SC.N_USERS, batch, SC.DECAY, tau, reg == "ego")
                loss.backward()
                for got, ref in zip(r["loss_out"], (loss.detach(), sm.detach(), reg_l.detach())):
                    assert abs(float(got) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
                scale = float(E0.grad.abs().max())
                assert float((r["G"] - E.grad).abs().max()) <= 1e-12 * scale
                assert float((r["g_final"] - E0.grad).abs().max()) <= 1e-12 * scale
                B = len(batch[0])          # the per-sample terms are scaled for the single-wave reduction with 1 / B
                assert abs(-float(r["term"].sum()) / B - float(sm.detach())) <= 1e-12
                assert abs(0.5 * float(r["regterm"].sum()) / B - float(reg_l.detach())) <= 1e-12
                assert float((r["q"].sum(1) - 1.0).max()) < 0.0 and float(r["q"].min()) >= 0.0


# ---- 2. R = 1, tau = 1 is the BPR step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,K,reg", [(32, 1, "propagated"), (64, 3, "ego"), (256, 2, "propagated")])
def test_one_negative_at_temperature_one_is_the_bpr_step(pkg, storage_graph, d, K, reg):
    """log(1 + exp(-x)) = -logsigmoid(x) and q = sigmoid(-x): the restatement at R = 1, tau = 1 against
    multineg_restatement.step on the same triplets, to 1e-13."""
    _, _, A, table = _inputs(pkg, storage_graph, d)
    for u, p, n in SM.make_batches(d, K, 2):
        batch = (u, p, n[:, :1])
        r = SM.step(A, SC.N_USERS, K, SC.DECAY, 1.0, table, batch, reg == "ego")
        f = MN.step(A, SC.N_USERS, K, SC.DECAY, table, batch, reg == "ego")
        for got, ref in zip(r["loss_out"], f["loss_out"]):
            assert abs(float(got) - float(ref)) <= 1e-13 * max(1.0, abs(float(ref)))
        scale = float(f["g_final"].abs().max())
        assert float((r["gb"] - f["gb"]).abs().max()) <= 1e-13 * float(f["gb"].abs().max())
        assert float((r["term"] - f["term"]).abs().max()) <= 1e-13 * max(1.0, float(f["term"].abs().max()))
        assert float((r["G"] - f["G"]).abs().max()) <= 1e-13 * scale
        assert float((r["g_final"] - f["g_final"]).abs().max()) <= 1e-13 * scale
        assert torch.equal(r["cnt"], f["cnt"])
        # 1-D negatives are R = 1
        r1 = SM.step(A, SC.N_USERS, K, SC.DECAY, 1.0, table, (u, p, n[:, 0]), reg == "ego")
        assert torch.equal(r1["g_final"], r["g_final"])


# ---- 3. the package's autograd loss ------------------------------------------------------------------------------------------
def _model_with(pkg, path, cls="LightGCN", **cfg):
    w = SC.configure(pkg, ("fp32", 32, 2, 1, -1, "propagated"), path)
    w.config.update(cfg)
    ds = pkg.dataloader.Loader(w.config, path=path)
    return ds, getattr(pkg.model, cls)(w.config, ds)


@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_package_autograd_loss_is_the_restatement(pkg, storage_graph, reg):
    """LightGCN.bpr_loss with loss = softmax on the host tables (the embeddings injected, as in
    test_autograd_loss_accepts_two_dimensional_negatives_on_the_host_tables, and at its fp32-vs-float64 tolerance 1e-6):
    [B, R], [R, B] and 1-D negatives (R = 1)."""
    try:
        tau = 0.2
        ds, m = _model_with(pkg, storage_graph, neg_ratio=5, loss='softmax', softmax_temp=tau, reg_rows=reg)
        assert m.loss_kind == 'softmax' and m.softmax_temp == tau
        _, _, A, _ = _inputs(pkg, storage_graph, 32)
        SC.configure(pkg, ("fp32", 32, 2, 1, -1, reg), storage_graph)
        E0 = m._table.detach().double()
        E = SM.propagate(A, E0, 2)
        m.computer = lambda: (E[:SC.N_USERS].float(), E[SC.N_USERS:].float())
        u, p, n = SM.make_batches(32, 2, 5)[0]
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
        r = SM.step(A, SC.N_USERS, 2, SC.DECAY, tau, E0.numpy(), (u, p, n), reg == "ego")
        sm, rg = m.bpr_loss(t(u), t(p), t(n))
        assert abs(float(sm.detach()) - float(r["loss_out"][1])) < 1e-6 and abs(float(rg.detach()) - float(r["loss_out"][2])) < 1e-6
        sm_t, rg_t = m.bpr_loss(t(u), t(p), t(n).t().contiguous())
        assert abs(float(sm_t) - float(sm)) < 1e-6 and abs(float(rg_t) - float(rg)) < 1e-6
        r1 = SM.step(A, SC.N_USERS, 2, SC.DECAY, tau, E0.numpy(), (u, p, n[:, 0]), reg == "ego")
        sm1, rg1 = m.bpr_loss(t(u), t(p), t(n[:, 0]))
        assert abs(float(sm1) - float(r1["loss_out"][1])) < 1e-6 and abs(float(rg1) - float(r1["loss_out"][2])) < 1e-6
        assert abs(float(sm1) - float(sm)) > 1e-3                                   # (another loss than the five-negative one)
    finally:
        pkg.world.configure([])


# ---- 4. the saturation batch -------------------------------------------------------------------------------------------------
def test_saturation_batch_exists(pkg, storage_graph):
    """The batch of tests/test_gpu_softmax.py::test_saturation_batch, from the restatement alone: some z beyond +100 (fp32 expf
    overflows at 88.7: without the maximum subtracted the sum is inf) and some sample with all z below -100 (every exponent
    underflows).  The storage table reaches both as it stands: the BIG_ITEM row is not scaled (factor 1)."""
    _, _, A, table = _inputs(pkg, storage_graph, SM.SAT_D)
    E = SM.propagate(A, torch.from_numpy(table.astype(np.float64)), SM.SAT_K)
    u, p, n = batch = SM.saturation_batch(E.numpy())
    z = SM.step(A, SC.N_USERS, SM.SAT_K, SC.DECAY, SM.SAT_TAU, table, batch)["z"].numpy()
    print(f"[softmax] saturation batch: z in [{z.min():.1f}, {z.max():.1f}], per sample max {np.round(z.max(1), 1)}")
    assert len(u) == 8 and SC.BIG_ITEM in n[0] and SC.BIG_ITEM in n[1] and p[2] == p[3] == SC.BIG_ITEM
    assert SC.BIG_ITEM not in n[2:] and SC.BIG_ITEM not in p[[0, 1, 4, 5, 6, 7]]
    assert (z > 100.0).any() and (z < -100.0).all(1).any(), (z.max(), z.max(1).min())
    assert z[0].max() > 100.0 and (z[2] < -100.0).all() and (z[3] > 100.0).all()     # a dominating negative / all dominated / all dominating
    assert z[1].min() < -100.0                                                        # one dominated negative among ordinary ones
    assert np.isfinite(z).all()


# ---- 5. surface and refusals -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lgcn_ctx_set_loss", "lgcn_ctx_get_loss")


def test_new_symbols_are_declared_bound_and_exported_with_abi_13(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lgcn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", hdr))
    lib = pkg._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lgcn_abi_version() == pkg._lib.ABI_VERSION == 13
    assert pkg._lib.LOSS_BPR == int(re.search(r"#define\s+LGCN_LOSS_BPR\s+(\d+)", hdr).group(1)) == 0
    assert pkg._lib.LOSS_SOFTMAX == int(re.search(r"#define\s+LGCN_LOSS_SOFTMAX\s+(\d+)", hdr).group(1)) == 1
    assert "lgcn_multineg.hip" in [os.path.basename(s) for s in pkg.build.SOURCES]
    assert all(os.path.exists(s) for s in pkg.build.SOURCES), [s for s in pkg.build.SOURCES if not os.path.exists(s)]
    # what the host can refuse with no device
    assert lib.lgcn_ctx_set_loss(None, 1, 1.0) == 3 and b"lgcn_ctx_set_loss" in lib.lgcn_last_error()
    assert lib.lgcn_ctx_get_loss(None, None) == -1


def test_loss_flags(pkg):
    w = pkg.world
    try:
        w.configure([])
        assert w.config['loss'] == 'bpr' and w.config['softmax_temp'] == 1.0
        w.configure(['--loss', 'softmax', '--softmax_temp', '0.2', '--neg_ratio', '1'])
        assert w.config['loss'] == 'softmax' and w.config['softmax_temp'] == 0.2 and w.config['neg_ratio'] == 1
        with pytest.raises(SystemExit):
            w.configure(['--loss', 'hinge'])
        with pytest.raises(SystemExit):
            w.configure(['--softmax_temp', 'warm'])
    finally:
        w.configure([])


def test_refusals_that_need_no_device_name_the_flag(pkg, storage_graph):
    try:
        for cfg in ({'act_dtype': 'fp8', 'latent_dim_rec': 64}, {'use_pop_gate': True}, {'use_item_item': True}):
            with pytest.raises(pkg._lib.LgcnError, match="--loss"):
                _model_with(pkg, storage_graph, loss='softmax', **cfg)
        with pytest.raises(pkg._lib.LgcnError, match="--loss"):
            _model_with(pkg, storage_graph, cls="PureMF", loss='softmax')
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="--softmax_temp"):
                _model_with(pkg, storage_graph, loss='softmax', softmax_temp=bad)
        with pytest.raises(ValueError, match="--loss"):
            _model_with(pkg, storage_graph, loss='hinge')
        ds, m = _model_with(pkg, storage_graph, loss='softmax', softmax_temp=0.5, neg_ratio=1)      # --neg_ratio 1 is legal
        assert m.loss_kind == 'softmax' and m.neg_ratio == 1
        with pytest.raises(RuntimeError, match="--loss"):
            pkg.parallel.DataParallelBPR(m, pkg.world.config)
        # the default builds what it always built; a temperature without --loss softmax is not looked at
        _, m1 = _model_with(pkg, storage_graph, softmax_temp=0.0)
        assert m1.loss_kind == 'bpr'
        _, mf = _model_with(pkg, storage_graph, cls="PureMF")
        assert type(mf).__name__ == 'PureMF'
    finally:
        pkg.world.configure([])

"""The in-batch sampled softmax (--loss inbatch) without a device: the float64 restatement of the step
(tests/inbatch_restatement.py) is pinned to torch autograd of the loss written with torch.logsumexp and an explicit mask and,
at B = 2, to the sampled-softmax restatement (tests/softmax_restatement.py); the exact zeros of the masked batches; the
package's autograd loss; the saturation batch of the GPU tests; the flags, the refusals that need no device and the C ABI."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inbatch_restatement as IB                 # noqa: E402
import softmax_restatement as SM                 # noqa: E402
import storage_cases as SC                       # noqa: E402
import storage_restatement as S                  # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import REPO                        # noqa: E402

_CACHE = {}


def _inputs(pkg, path, d):
    """(dense float64 A, initial fp32 table with the hand-set rows) for an embedding width"""
    try:
        if ("tab", d) not in _CACHE:
            ds, m = SC.make_model(pkg, ("bf16", d, 1, 1, -1, "propagated"), path)
            if "A" not in _CACHE:
                _CACHE["A"] = S.dense_adj(ds.getSparseGraphCSR())
            _CACHE[("tab", d)] = m._table.detach().numpy().copy()
        return _CACHE["A"], _CACHE[("tab", d)]
    finally:
        pkg.world.configure([])


# ---- 1. the restatement is the autograd of the written loss ------------------------------------------------------------------
@pytest.mark.parametrize("tau", [1.0, 0.2])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("d", [32, 64])
def test_restatement_is_the_autograd_of_the_written_loss(pkg, storage_graph, d, K, tau):
    """g_final, G and the loss triple against torch float64 autograd of the loss written with torch.logsumexp and an explicit
    mask, both reg rows, with and without layer weights, on a masked batch of 65, the split batch and B = 1: 1e-12 relative,
    float64 against float64 (the level tests/test_softmax_host.py uses for the same comparison)."""
    A, table = _inputs(pkg, storage_graph, d)
    for reg in ("propagated", "ego"):
        for w in (None, [0.4, 0.1, 0.3, 0.2][:K + 1]):
            for batch in (IB.make_batch(65), IB.make_batch(IB.SPLIT_B), IB.make_batch(1)):
                r = IB.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg == "ego", w)
                E0 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
                E = IB.propagate(A, E0, K, w)
                E.retain_grad()
                loss, sm, reg_l = IB.loss(E, E0, SC.N_USERS, batch, SC.DECAY, tau, reg == "ego")
                loss.backward()
                for got, ref in zip(r["loss_out"], (loss.detach(), sm.detach(), reg_l.detach())):
                    assert abs(float(got) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
                scale = float(E0.grad.abs().max())
                assert float((r["G"] - E.grad).abs().max()) <= 1e-12 * scale
                assert float((r["g_final"] - E0.grad).abs().max()) <= 1e-12 * scale
                B = len(batch[0])          # the per-sample terms are scaled for the single-wave reduction with 1 / B
                assert abs(-float(r["term"].sum()) / B - float(sm.detach())) <= 1e-12
                assert abs(0.5 * float(r["regterm"].sum()) / B - float(reg_l.detach())) <= 1e-12
                assert float(r["q"].min()) >= 0.0 and float((r["Q"] - 1.0).max()) < 0.0
                assert float(r["W"].sum(1).abs().max()) <= 1e-15                     # every row of W sums to zero


def _pin(r, loss_fn, A, table, K, w, B):
    """A restatement r against torch float64 autograd of loss_fn(E, E0) -> (loss, sm, reg) at 1e-12 relative."""
    E0 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
    E = IB.propagate(A, E0, K, w)
    E.retain_grad()
    loss, sm, reg_l = loss_fn(E, E0)
    loss.backward()
    for got, ref in zip(r["loss_out"], (loss.detach(), sm.detach(), reg_l.detach())):
        assert abs(float(got) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
    scale = float(E0.grad.abs().max())
    assert float((r["G"] - E.grad).abs().max()) <= 1e-12 * scale
    assert float((r["g_final"] - E0.grad).abs().max()) <= 1e-12 * scale
    assert abs(-float(r["term"].sum()) / B - float(sm.detach())) <= 1e-12
    assert abs(0.5 * float(r["regterm"].sum()) / B - float(reg_l.detach())) <= 1e-12


@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_restatement_is_the_autograd_of_the_written_loss_across_three_parts(pkg, storage_graph, reg):
    """The same pin at B = 705 (23 tiles, three parts of the sweep; a user and a positive repeated across parts), d = 64, K = 3,
    tau = 0.2: the restatement judges the device at B = 513 and B = 2048 (tests/test_gpu_inbatch.py, section 1b), so it is not
    only pinned at B <= 260.  1e-12 relative, as above.  Every sample of the large batches keeps more than half of its B - 1
    possible competitors (300 users and 560 items mask some pairs by themselves)."""
    A, table = _inputs(pkg, storage_graph, 64)
    B, K, tau = 705, 3, 0.2
    batch = IB.make_batch(B)
    u, p = batch
    assert IB.parts(B) == 3 and u[B - 1] in u[:256] and p[B - 1] in p[:256] and u[300] in u[:256] and p[400] in p[:256]
    for w in (None, [0.4, 0.1, 0.3, 0.2]):
        r = IB.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg == "ego", w)
        _pin(r, lambda E, E0: IB.loss(E, E0, SC.N_USERS, batch, SC.DECAY, tau, reg == "ego"), A, table, K, w, B)
        assert float(r["W"].sum(1).abs().max()) <= 1e-15
    for Bl in IB.LARGE_BATCH_SIZES + (705,):
        assert IB.kept_share(*IB.make_batch(Bl)) > 0.5


# ---- 2. B = 2 is the sampled softmax with each other's positive as the negative ------------------------------------------------
@pytest.mark.parametrize("d,K,tau", [(32, 1, 1.0), (64, 3, 0.2)])
def test_two_samples_are_the_sampled_softmax_of_each_others_positive(pkg, storage_graph, d, K, tau):
    A, table = _inputs(pkg, storage_graph, d)
    u, p = IB.make_batch(2)
    assert u[0] != u[1] and p[0] != p[1]
    r = IB.step(A, SC.N_USERS, K, SC.DECAY, tau, table, (u, p))
    E0 = torch.from_numpy(table.astype(np.float64))
    E = SM.propagate(A, E0, K)
    _, sm, _ = SM.loss(E, E0, SC.N_USERS, (u, p, p[::-1].copy()), SC.DECAY, tau)
    assert abs(float(r["loss_out"][1]) - float(sm)) <= 1e-13 * max(1.0, abs(float(sm)))


# ---- 3. the exact zeros ------------------------------------------------------------------------------------------------------
def test_one_sample_and_one_user_batches_have_no_competitors(pkg, storage_graph):
    """B = 1, and a batch whose samples all share one user: sm is exactly 0.0 and the gradient is the regulariser's."""
    A, table = _inputs(pkg, storage_graph, 32)
    for batch in (IB.make_batch(1), IB.one_user_batch(33)):
        r = IB.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, batch)
        assert float(r["loss_out"][1]) == 0.0 and not bool(r["keep"].any()) and float(r["W"].abs().max()) == 0.0
        u, p = (torch.from_numpy(t) for t in IB.as_samples(batch))
        lam = SC.DECAY / len(u)
        G = torch.zeros_like(r["G"])
        G.index_add_(0, u, lam * r["e_u"]); G.index_add_(0, SC.N_USERS + p, lam * r["e_p"])
        assert torch.equal(G, r["G"])


def test_a_duplicated_positive_masks_its_two_columns_from_each_other_only(pkg, storage_graph):
    A, table = _inputs(pkg, storage_graph, 32)
    u, p = IB.duplicated_positive_batch()
    assert p[5] == p[2] and len(set(u)) == len(u) and len(set(p)) == len(p) - 1
    r = IB.step(A, SC.N_USERS, 1, SC.DECAY, 0.2, table, (u, p))
    want = ~torch.eye(len(u), dtype=torch.bool)
    want[2, 5] = want[5, 2] = False
    assert torch.equal(r["keep"], want)
    assert float(r["q"][2, 5]) == 0.0 and float(r["q"][5, 2]) == 0.0 and float(r["q"][want].min()) > 0.0


# ---- 4. the package's autograd loss ------------------------------------------------------------------------------------------
def _model_with(pkg, path, cls="LightGCN", **cfg):
    w = SC.configure(pkg, ("fp32", 32, 2, 1, -1, "propagated"), path)
    w.config.update(cfg)
    ds = pkg.dataloader.Loader(w.config, path=path)
    return ds, getattr(pkg.model, cls)(w.config, ds)


@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_package_autograd_loss_is_the_restatement(pkg, storage_graph, reg):
    """LightGCN.bpr_loss with loss = inbatch on the host tables (the embeddings injected, as in tests/test_softmax_host.py, and
    at its fp32-vs-float64 tolerance 1e-6); the negatives are accepted and ignored."""
    try:
        tau = 0.2
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=tau, reg_rows=reg)
        assert m.loss_kind == 'inbatch' and m.softmax_temp == tau
        A, _ = _inputs(pkg, storage_graph, 32)
        SC.configure(pkg, ("fp32", 32, 2, 1, -1, reg), storage_graph)
        E0 = m._table.detach().double()
        E = IB.propagate(A, E0, 2)
        m.computer = lambda: (E[:SC.N_USERS].float(), E[SC.N_USERS:].float())
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
        for batch in (IB.make_batch(65), IB.make_batch(2), IB.make_batch(1)):
            u, p = batch
            r = IB.step(A, SC.N_USERS, 2, SC.DECAY, tau, E0.numpy(), batch, reg == "ego")
            sm, rg = m.bpr_loss(t(u), t(p), t(p[::-1].copy()))
            assert abs(float(sm.detach()) - float(r["loss_out"][1])) < 1e-6 and abs(float(rg.detach()) - float(r["loss_out"][2])) < 1e-6
            sm2, _ = m.bpr_loss(t(u), t(p), t(u) * 0)
            assert float(sm2) == float(sm)
    finally:
        pkg.world.configure([])


# ---- 5. the saturation batch -------------------------------------------------------------------------------------------------
def test_saturation_batch_exists(pkg, storage_graph):
    """The batch of tests/test_gpu_inbatch.py::test_saturation_batch, from the restatement alone: some z beyond +100 (fp32 expf
    overflows at 88.7) and a sample with all z below -100."""
    A, table = _inputs(pkg, storage_graph, IB.SAT_D)
    E = IB.propagate(A, torch.from_numpy(table.astype(np.float64)), IB.SAT_K)
    u, p = batch = IB.saturation_batch(E.numpy())
    r = IB.step(A, SC.N_USERS, IB.SAT_K, SC.DECAY, IB.SAT_TAU, table, batch)
    z, keep = r["z"].numpy(), r["keep"].numpy()
    zk = np.where(keep, z, np.nan)
    print(f"[inbatch] saturation batch: z in [{np.nanmin(zk):.1f}, {np.nanmax(zk):.1f}]")
    assert len(set(u)) == len(u) and len(set(p)) == len(p) and p[2] == SC.BIG_ITEM
    assert keep.sum() == len(u) * (len(u) - 1)
    assert zk[0, 2] > 100.0 and zk[1, 2] < -100.0 and np.nanmax(zk[2]) < -100.0
    q = r["q"].numpy()
    assert q[0, 2] > 1.0 - 1e-9 and float(r["lterm"][2]) < 1e-40                  # a one-hot row, a tiny l
    assert np.isfinite(z[keep]).all() and np.isfinite(r["g_final"].numpy()).all()


def test_tiny_l_batch_exists(pkg, storage_graph):
    """The batch of tests/test_gpu_inbatch.py::test_tiny_loss_term_keeps_its_relative_accuracy, from the restatement alone: sample 2
    has all z in [-60, -20], so its l is tiny, non-zero in float64 and a normal fp32 number, and its maximum stays at M = 0."""
    A, table = _inputs(pkg, storage_graph, IB.SAT_D)
    E = IB.propagate(A, torch.from_numpy(table.astype(np.float64)), IB.SAT_K)
    u, p, tau = IB.tiny_l_batch(E.numpy())
    tau = float(np.float32(tau))
    r = IB.step(A, SC.N_USERS, IB.SAT_K, SC.DECAY, tau, table, (u, p))
    z2 = r["z"].numpy()[2][r["keep"].numpy()[2]]
    l2 = float(r["lterm"][2])
    print(f"[inbatch] tiny-l batch: tau {tau:.4f}, z_2 in [{z2.min():.2f}, {z2.max():.2f}], l_2 = {l2:.3e}")
    assert len(z2) == len(u) - 1 and -60.0 < z2.min() and z2.max() < -20.0
    assert 2.0 ** -100 < l2 < 1e-6 and float(r["m"][2]) == 0.0 and abs(float(r["Q"][2]) / l2 - 1.0) < 1e-6


# ---- 6. surface and refusals -------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lgcn_train_step_inbatch", "lgcn_train_epoch_inbatch")


def test_new_symbols_are_declared_bound_and_exported_with_abi_13(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lgcn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", hdr))
    lib = pkg._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lgcn_abi_version() == pkg._lib.ABI_VERSION == 13
    assert pkg._lib.LOSS_INBATCH == int(re.search(r"#define\s+LGCN_LOSS_INBATCH\s+(\d+)", hdr).group(1)) == 2
    assert "lgcn_inbatch.hip" in [os.path.basename(s) for s in pkg.build.SOURCES]
    assert all(os.path.exists(s) for s in pkg.build.SOURCES), [s for s in pkg.build.SOURCES if not os.path.exists(s)]
    # what the host can refuse with no device
    assert lib.lgcn_ctx_set_loss(None, pkg._lib.LOSS_INBATCH, 1.0) == 3 and b"lgcn_ctx_set_loss" in lib.lgcn_last_error()
    assert lib.lgcn_train_step_inbatch(None, None, None, 4, None, None) == 3 and b"lgcn_train_step_inbatch" in lib.lgcn_last_error()
    assert lib.lgcn_train_epoch_inbatch(None, None, None, 8, 4, None, None) == 3 and b"lgcn_train_epoch_inbatch" in lib.lgcn_last_error()
    assert lib.lgcn_train_epoch_inbatch(None, None, None, 0, 4, None, None) == 0          # an empty epoch is no call


def test_loss_flags(pkg):
    w = pkg.world
    try:
        w.configure(['--loss', 'inbatch', '--softmax_temp', '0.2'])
        assert w.config['loss'] == 'inbatch' and w.config['softmax_temp'] == 0.2 and w.config['neg_ratio'] == 1
        assert pkg.model.resolve_loss(w.config) == ('inbatch', 0.2)
        with pytest.raises(SystemExit):
            w.configure(['--loss', 'hinge'])
    finally:
        w.configure([])


def test_refusals_that_need_no_device_name_the_flag(pkg, storage_graph):
    try:
        for cfg in ({'act_dtype': 'fp8', 'latent_dim_rec': 64}, {'use_pop_gate': True}, {'use_item_item': True}):
            with pytest.raises(pkg._lib.LgcnError, match="--loss inbatch"):
                _model_with(pkg, storage_graph, loss='inbatch', **cfg)
        with pytest.raises(pkg._lib.LgcnError, match="--loss"):
            _model_with(pkg, storage_graph, cls="PureMF", loss='inbatch')
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="--softmax_temp"):
                _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=bad)
        with pytest.raises(ValueError, match="--loss"):
            _model_with(pkg, storage_graph, loss='hinge')
        with pytest.raises(pkg._lib.LgcnError, match=r"--loss inbatch.*--neg_ratio"):
            _model_with(pkg, storage_graph, loss='inbatch', neg_ratio=2)
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.5)
        assert m.loss_kind == 'inbatch' and m.neg_ratio == 1
        with pytest.raises(RuntimeError, match="--loss inbatch"):
            pkg.parallel.DataParallelBPR(m, pkg.world.config)
    finally:
        pkg.world.configure([])

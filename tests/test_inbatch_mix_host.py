"""Mixed negative sampling for the in-batch softmax (--inbatch_mix 1) without a device: the float64 restatement
(tests/inbatch_mix_restatement.py) is (a) array-equal to tests/inbatch_scores_restatement.py with no pool, (b) the sampled
softmax of tests/softmax_restatement.py at B = 1 and (c) pinned to torch autograd of the written loss; (d) the mixture's logQ
against a direct count; (e) the flags, the defaults and the refusals that need no device; (f) the C ABI; (g) for every case of
tests/test_gpu_inbatch_mix.py a step that ignored the pool would miss that test's bound on `terms`."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inbatch_mix_bounds as MB                  # noqa: E402
import inbatch_mix_restatement as IM             # noqa: E402
import inbatch_restatement as IB                 # noqa: E402
import inbatch_scores_restatement as IS          # noqa: E402
import softmax_restatement as SM                 # noqa: E402
import storage_cases as SC                       # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import REPO                        # noqa: E402
from test_gpu_inbatch import _uncovered          # noqa: E402
from test_inbatch_host import _inputs, _model_with, _pin   # noqa: E402

_C = {}
OPTIONS = (("dot", False), ("cosine", True), ("cosine", False))


def _ds(pkg, path):
    if "ds" not in _C:
        try:
            ds, _ = SC.make_model(pkg, ("fp32", 32, 1, 1, -1, "propagated"), path)
            _C["ds"], _C["adj"] = ds, ds.getSparseGraphCSR()
        finally:
            pkg.world.configure([])
    return _C["ds"]


def _logq(pkg, path, B, R):
    lq = IM.item_logq_mix(_ds(pkg, path).items_D, B, R)
    assert lq.dtype == np.float32 and len(lq) == SC.M_ITEMS and np.isfinite(lq).all()
    return lq


# ---- (a) no pool: the parent's restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("score,lq_on", OPTIONS)
def test_without_a_pool_it_is_the_scores_restatement_array_equal(pkg, storage_graph, score, lq_on):
    A, table = _inputs(pkg, storage_graph, 32)
    lq = IS.item_logq(_ds(pkg, storage_graph).items_D) if lq_on else None
    for K, w in ((1, None), (3, [0.4, 0.1, 0.3, 0.2])):
        for reg in (False, True):
            for batch in (IB.make_batch(65), IB.duplicated_positive_batch(), IB.one_user_batch(33), IB.make_batch(1)):
                a = IS.step(A, SC.N_USERS, K, SC.DECAY, 0.2, table, batch, reg, w, score=score, logq=lq)
                for b in (IM.step(A, SC.N_USERS, K, SC.DECAY, 0.2, table, batch, reg, w, score=score, logq=lq),
                          IM.step(A, SC.N_USERS, K, SC.DECAY, 0.2, table, batch + (None,), reg, w, score=score, logq=lq)):
                    for key, v in a.items():
                        if key == "loss_out":
                            assert all(float(x) == float(y) for x, y in zip(v, b[key]))
                        else:
                            assert np.array_equal(v.numpy(), b[key].numpy(), equal_nan=True), key
    v = IS.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, IB.make_batch(33), B_norm=40, score=score, logq=lq)
    g = IM.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, IB.make_batch(33), B_norm=40, score=score, logq=lq)
    assert np.array_equal(v["g_final"].numpy(), g["g_final"].numpy())


# ---- (b) B = 1: the sampled softmax ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 16])
@pytest.mark.parametrize("tau", [0.2, 0.1])
def test_one_sample_is_the_sampled_softmax(pkg, storage_graph, R, tau):
    """loss, reg and every gradient row against tests/softmax_restatement.py at the same R and tau: 1e-12 relative."""
    A, table = _inputs(pkg, storage_graph, 64)
    for reg in (False, True):
        for K, w in ((1, None), (2, [0.5, 0.2, 0.3])):
            batch = IM.make_batch(1, R, seed=R, plain=True)
            a = IM.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg, w)
            b = SM.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg, w)
            for x, y in zip(a["loss_out"], b["loss_out"]):
                assert abs(float(x) - float(y)) <= 1e-12 * max(1.0, abs(float(y)))
            assert abs(float(a["regterm"][0]) - float(b["regterm"][0])) <= 1e-12 * float(b["regterm"][0])
            for key in ("G", "g_final"):
                assert float((a[key] - b[key]).abs().max()) <= 1e-12 * float(b[key].abs().max()), key
            assert float((a["g_n"] - b["g_n"].reshape(-1, 64)).abs().max()) <= 1e-12 * float(b["g_n"].abs().max())
            assert np.array_equal(a["cnt"].numpy(), b["cnt"].numpy())


# ---- (c) the autograd of the written loss ------------------------------------------------------------------------------------
def _pin_batch():
    """65 samples, R = 3, with everything the loss has to get right; sample 33 is void (the restatement is given the sound ones)."""
    u, p, negs = IM.make_batch(65, 3, seed=2)
    assert negs[1, 2] == p[0] and negs[0, 1] == negs[0, 0] and negs[2, 0] == negs[0, 0]      # masked / another's positive; duplicates
    sound = np.ones(65, bool); sound[33] = False
    return (u[sound], p[sound], negs[sound]), 65


@pytest.mark.parametrize("tau", [0.2, 0.1])
@pytest.mark.parametrize("score,lq_on", OPTIONS)
@pytest.mark.parametrize("d,K", [(32, 1), (64, 3)])
def test_restatement_is_the_autograd_of_the_written_loss(pkg, storage_graph, d, K, score, lq_on, tau):
    """g_final, G and the loss triple against torch float64 autograd of the loss written with F.normalize, the lq difference,
    torch.logsumexp and an explicit mask over the [B, 1 + B + B R] logits: 1e-12 relative, float64 against float64 -- the
    tolerance of tests/test_inbatch_scores_host.py for the same comparison."""
    A, table = _inputs(pkg, storage_graph, d)
    lq = _logq(pkg, storage_graph, 65, 3) if lq_on else None
    (bu, bp, bn), Bn = _pin_batch()
    cases = [((bu, bp, bn), Bn), (IM.make_batch(2, 2), None), (IM.make_batch(1, 1), None), (IM.make_batch(33, 16), None)]
    for reg in ("propagated", "ego"):
        for w in (None, [0.4, 0.1, 0.3, 0.2][:K + 1]):
            for batch, B_norm in cases:
                r = IM.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg == "ego", w, B_norm=B_norm, score=score, logq=lq)
                assert float(r["inv_u"].min()) > 0.0 and float(r["inv_p"].min()) > 0.0 and float(r["inv_n"].min()) > 0.0
                E0 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
                E = IB.propagate(A, E0, K, w)
                E.retain_grad()
                loss, sm, reg_l = IM.loss(E, E0, SC.N_USERS, batch, SC.DECAY, tau, reg == "ego", score=score, logq=lq, B_norm=B_norm)
                loss.backward()
                for got, ref in zip(r["loss_out"], (loss.detach(), sm.detach(), reg_l.detach())):
                    assert abs(float(got) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
                scale = float(E0.grad.abs().max())
                assert float((r["G"] - E.grad).abs().max()) <= 1e-12 * scale
                assert float((r["g_final"] - E0.grad).abs().max()) <= 1e-12 * scale
                assert float(r["W"].sum(1).abs().max()) <= 1e-15                     # every row of W sums to zero
    r = IM.step(A, SC.N_USERS, K, SC.DECAY, tau, table, (bu, bp, bn), B_norm=Bn, score=score, logq=lq)
    keep = r["keep"].numpy()
    nb = len(bu)
    assert not keep[0, nb + 2 * nb + 1] and keep[5, nb + 2 * nb + 1] and keep[5, 0]      # n_{1,2} = p_0: masked for sample 0 only
    assert float(r["q"][5, nb + 0]) > 0.0 and float(r["q"][5, nb + nb + 0]) > 0.0      # the duplicate n_{0,0} = n_{0,1}: both count


@pytest.mark.parametrize("score,lq_on", [("dot", False), ("cosine", True)])
def test_restatement_is_the_autograd_of_the_written_loss_across_three_parts(pkg, storage_graph, score, lq_on):
    """The same pin at (B, R) = (545, 16) -- three parts on the user side, 39 on the item side; a case of
    inbatch_mix_bounds.LARGE_CASES -- d = 64, K = 3, tau = 0.2, both reg rows: the restatement judges the device at that size and at
    (2048, 1) (tests/test_gpu_inbatch_mix.py, section 1b).  1e-12 relative, as above."""
    A, table = _inputs(pkg, storage_graph, 64)
    B, R, K, tau = 545, 16, 3, 0.2
    assert (B, R) in MB.LARGE_BRS and MB.parts_users(B) == 3
    lq = _logq(pkg, storage_graph, B, R) if lq_on else None
    batch = IM.make_batch(B, R)
    u, p, negs = batch
    assert u[B - 1] in u[:256] and p[B - 1] in p[:256] and negs[B - 1, 0] in p[:256]      # across the parts of the user sweep
    for reg in ("propagated", "ego"):
        r = IM.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg == "ego", None, score=score, logq=lq)
        assert float(r["inv_u"].min()) > 0.0 and float(r["inv_p"].min()) > 0.0 and float(r["inv_n"].min()) > 0.0
        _pin(r, lambda E, E0: IM.loss(E, E0, SC.N_USERS, batch, SC.DECAY, tau, reg == "ego", score=score, logq=lq), A, table, K, None, B)
        assert float(r["W"].sum(1).abs().max()) <= 1e-15


def test_the_pool_changes_the_step(pkg, storage_graph):
    A, table = _inputs(pkg, storage_graph, 32)
    u, p, negs = IM.make_batch(65, 2)
    base = IS.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, (u, p))
    r = IM.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, (u, p, negs))
    assert float(r["loss_out"][1]) > float(base["loss_out"][1]) + 0.1 and float(r["loss_out"][2]) > float(base["loss_out"][2])
    assert bool((r["lterm"] >= base["lterm"]).all())                                  # more competitors, never fewer


# ---- (d) the mixture's logQ --------------------------------------------------------------------------------------------------
def test_mixture_logq_is_the_expected_count_of_competitors(pkg):
    """A tiny graph, counted directly: (B - 1) other samples each draw their positive with probability deg_i / sum deg (an edge
    drawn uniformly), and the B R pool ids are uniform over the items."""
    edges = [(0, 0), (0, 1), (1, 1), (2, 1), (2, 2), (3, 1), (3, 3), (4, 0)]      # (user, item); item 4 has no edge: the loader's 1
    m_items = 5
    deg = np.ones(m_items)
    for i in range(m_items):
        deg[i] = max(1, sum(1 for _, it in edges if it == i))
    B, R = 6, 3
    expected = np.array([(B - 1) * deg[i] / deg.sum() + B * R * (1.0 / m_items) for i in range(m_items)])
    want = np.log(expected).astype(np.float32)
    assert np.array_equal(pkg.model.item_logq_mix(deg, B, R), want) and np.array_equal(IM.item_logq_mix(deg, B, R), want)
    assert pkg.model.item_logq_mix(deg, B, R).dtype == np.float32
    # B = 1: no in-batch competitor, the uniform pool alone -- a constant, which cancels in z
    assert len(set(pkg.model.item_logq_mix(deg, 1, 2).tolist())) == 1
    for bad in ((0, 1), (4, 0)):
        with pytest.raises(ValueError, match="--inbatch_mix"):
            pkg.model.item_logq_mix(deg, *bad)
    with pytest.raises(ValueError, match="degrees"):
        pkg.model.item_logq_mix(np.array([1.0, 0.0]), 4, 1)


# ---- (e) flags, defaults, refusals -------------------------------------------------------------------------------------------
def test_flag_and_defaults(pkg):
    w = pkg.world
    try:
        w.configure([])
        assert w.config['inbatch_mix'] == 0
        assert pkg.model.resolve_inbatch_mix(w.config, 'bpr') is False and pkg.model.resolve_inbatch_mix({}, 'softmax') is False
        w.configure(['--loss', 'inbatch', '--inbatch_mix', '1', '--neg_ratio', '4', '--softmax_temp', '0.1'])
        assert w.config['inbatch_mix'] == 1 and pkg.model.resolve_inbatch_mix(w.config, 'inbatch') is True
        with pytest.raises(SystemExit):
            w.configure(['--inbatch_mix', '2'])
        helps = {a.dest: a.help for a in pkg.parse.build_parser()._actions}
        assert helps['inbatch_mix'].startswith('NEW') and '--neg_ratio' in helps['inbatch_mix']
        with pytest.raises(ValueError, match="--inbatch_mix"):
            pkg.model.resolve_inbatch_mix({'inbatch_mix': 2}, 'inbatch')
    finally:
        w.configure([])


def test_refusals_that_need_no_device_name_the_flag(pkg, storage_graph):
    try:
        for loss in ('bpr', 'softmax'):
            with pytest.raises(pkg._lib.LgcnError, match="--inbatch_mix 1 is implemented for --loss inbatch only"):
                _model_with(pkg, storage_graph, loss=loss, inbatch_mix=1)
        with pytest.raises(pkg._lib.LgcnError, match="--inbatch_mix"):
            _model_with(pkg, storage_graph, cls="PureMF", inbatch_mix=1)
        # with 0 nothing changes: today's refusal of --neg_ratio > 1 and its message
        with pytest.raises(pkg._lib.LgcnError, match="--loss inbatch is not implemented together with --neg_ratio 4"):
            _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.2, neg_ratio=4)
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.2)
        assert m.inbatch_mix is False
        for R in (1, 4, 16):
            ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.2, inbatch_mix=1, neg_ratio=R)
            assert m.inbatch_mix is True and m.neg_ratio == R and m._item_logq is None
        with pytest.raises(ValueError, match="--neg_ratio"):
            _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.2, inbatch_mix=1, neg_ratio=17)
        # the logQ vector: the mixture's with mixing on (B = --bpr_batch), log(deg) with it off
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.1, inbatch_logq=1, inbatch_mix=1, neg_ratio=4)
        B = int(pkg.world.config['bpr_batch_size'])
        assert np.array_equal(m._item_logq.numpy(), IM.item_logq_mix(ds.items_D, B, 4))
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.1, inbatch_logq=1)
        assert np.array_equal(m._item_logq.numpy(), IS.item_logq(ds.items_D))
        # data parallelism refuses by name before it looks at anything else
        with pytest.raises(RuntimeError, match="--inbatch_mix 1 is implemented for single-GPU training only"):
            class _M:
                inbatch_mix = True
            pkg.parallel.DataParallelBPR(_M(), {'inbatch_mix': 1})
    finally:
        pkg.world.configure([])


# ---- (f) surface -------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lgcn_ctx_set_inbatch_mix", "lgcn_ctx_get_inbatch_mix", "lgcn_train_step_inbatch_mix", "lgcn_train_epoch_inbatch_mix")


def test_new_symbols_are_declared_bound_and_exported_with_abi_13(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lgcn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", hdr))
    lib = pkg._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lgcn_abi_version() == pkg._lib.ABI_VERSION == 13
    # what the host can refuse with no device: a null context, by name
    assert lib.lgcn_ctx_set_inbatch_mix(None, 1) == 3 and b"lgcn_ctx_set_inbatch_mix" in lib.lgcn_last_error()
    assert lib.lgcn_ctx_get_inbatch_mix(None) == -1
    assert lib.lgcn_train_step_inbatch_mix(None, None, None, None, 1, 1, 1, None, None) == 3
    assert b"lgcn_train_step_inbatch_mix" in lib.lgcn_last_error()
    assert lib.lgcn_train_epoch_inbatch_mix(None, None, None, None, 1, 5, 1, None, None) == 3
    assert b"lgcn_train_epoch_inbatch_mix" in lib.lgcn_last_error()


@pytest.mark.parametrize("score,lq_on", [("dot", False), ("cosine", True)])
@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_package_autograd_loss_is_the_restatement(pkg, storage_graph, reg, score, lq_on):
    """LightGCN.bpr_loss of a CPU model with mixing on, the embeddings injected, at the fp32-vs-float64 tolerance 1e-6 of
    tests/test_inbatch_scores_host.py::test_package_autograd_loss_is_the_restatement; neg as [B, R], [R, B] and (R = 1) [B]."""
    try:
        tau, R = 0.2, 3
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=tau, reg_rows=reg, score=score, inbatch_logq=int(lq_on),
                            inbatch_mix=1, neg_ratio=R)
        lq = m._item_logq.numpy() if lq_on else None
        A, _ = _inputs(pkg, storage_graph, 32)
        SC.configure(pkg, ("fp32", 32, 2, 1, -1, reg), storage_graph)
        E0 = m._table.detach().double()
        E = IB.propagate(A, E0, 2)
        Ef = E.float().requires_grad_(True)
        m.computer = lambda: (Ef[:SC.N_USERS], Ef[SC.N_USERS:])
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
        for batch in (IM.make_batch(65, R), IM.make_batch(2, R), IM.make_batch(1, R), IM.make_batch(33, 1)):
            u, p, negs = batch
            r = IM.step(A, SC.N_USERS, 2, SC.DECAY, tau, E0.numpy(), batch, reg == "ego", score=score, logq=lq)
            shapes = [t(negs), t(negs.T.copy())] if len(u) != negs.shape[1] else [t(negs)]
            if negs.shape[1] == 1:
                shapes.append(t(negs.reshape(-1)))
            for ng in shapes:
                sm, rg = m.bpr_loss(t(u), t(p), ng)
                assert abs(float(sm.detach()) - float(r["loss_out"][1])) < 1e-6 and abs(float(rg.detach()) - float(r["loss_out"][2])) < 1e-6
        u, p, negs = IM.make_batch(65, R)
        r = IM.step(A, SC.N_USERS, 2, 0.0, tau, E0.numpy(), (u, p, negs), False, score=score, logq=lq)
        sm, _ = m.bpr_loss(t(u), t(p), t(negs))
        sm.backward()
        assert float((Ef.grad.double() - r["G"]).abs().max()) < 1e-6 * max(1.0, float(r["G"].abs().max()))
    finally:
        pkg.world.configure([])


# ---- (g) the GPU cases are sensitive to the pool -----------------------------------------------------------------------------
def test_the_gpu_cases_cover_the_axes():
    assert not _uncovered(MB.CASES), _uncovered(MB.CASES)
    assert all({c[a] for c in MB.CASES} == set(ax) for a, ax in enumerate(MB.AXES))
    assert (65, 16) in {c[:2] for c in MB.CASES} and (260, 1) in {c[:2] for c in MB.CASES}
    assert MB.parts_items(65, 16) == 7 and (1 + 16) * 3 % 8 != 0 and MB.parts_items(260, 1) == 3


_SEEN = {}


@pytest.mark.parametrize("case", [pytest.param(c, id=MB.case_id(c)) for c in MB.CASES])
def test_a_step_that_ignored_the_pool_would_miss_the_bound(pkg, storage_graph, case):
    """From the initial table of the GPU case (its first step; the GPU test repeats the check from the device's own state at
    every step): the terms with and without the pool differ by more than the GPU test's bound on a term for at least one sample."""
    B, R, d, K, mode, reg, tau, (score, lq_on) = case
    A, table = _inputs(pkg, storage_graph, d)
    _ds(pkg, storage_graph)
    lq = _logq(pkg, storage_graph, B, R) if lq_on else None
    batch = MB.case_batches(case)[0]
    share, r, bd = MB.sensitivity(_C["adj"], A, table, batch, B, K, d, mode, reg == "ego", MB.tau32(tau), score, lq)
    print(f"[inbatch_mix] {MB.case_id(case)}: ignoring the pool moves a term by {share:.3g} times its bound")
    assert share > 1.0, share
    z, m = r["z"].numpy(), r["m"].numpy()
    top = z.argmax(1)
    nb = len(batch[0])
    for key, hit in (("pool", (m > 0) & (top >= nb)), ("inbatch", (m > 0) & (top < nb)), ("M0", (m == 0) & r["keep"].numpy().any(1))):
        _SEEN[key] = _SEEN.get(key, False) or bool(hit.any())
    masked = ~r["keep"].numpy()[:, nb:]
    _SEEN["masked"] = _SEEN.get("masked", False) or bool(masked.any())


def test_the_gpu_cases_hold_every_kind_of_row(pkg, storage_graph):
    """Over the first steps of the cases: a row whose maximum lies in the pool, one whose maximum lies in an in-batch column, one
    where no competitor exceeds the positive (M = 0), and a masked pool id.  (Computed here if the cases above did not run.)"""
    if len(_SEEN) < 4:
        for case in MB.CASES:
            test_a_step_that_ignored_the_pool_would_miss_the_bound(pkg, storage_graph, case)
    assert all(_SEEN.get(k) for k in ("pool", "inbatch", "M0", "masked")), _SEEN

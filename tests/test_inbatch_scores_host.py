"""The two score options of the in-batch softmax (--score cosine, --inbatch_logq 1) without a device: the float64
restatement (tests/inbatch_scores_restatement.py) is (a) array-equal to tests/inbatch_restatement.py with both options off and
(b) pinned to torch autograd of the written loss (F.normalize, the lq difference) for the three new combinations; (c) a
constant lq changes nothing; (d) cosine scores do not see the length of a row and the score gradient of a row is orthogonal to
it; (e) the flags, the defaults, the refusals that need no device, the C ABI and the package's autograd loss."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inbatch_restatement as IB                 # noqa: E402
import inbatch_scores_restatement as IS          # noqa: E402
import storage_cases as SC                       # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import REPO                        # noqa: E402
from test_inbatch_host import _inputs, _model_with, _pin   # noqa: E402

_LQ = {}


def _logq(pkg, path):
    """The fp32 vector the package hands the library on the storage graph: log(items_D)."""
    if "lq" not in _LQ:
        try:
            ds, _ = SC.make_model(pkg, ("fp32", 32, 1, 1, -1, "propagated"), path)
            _LQ["lq"] = IS.item_logq(ds.items_D)
            assert np.array_equal(_LQ["lq"], pkg.model.item_logq(ds.items_D)) and _LQ["lq"].dtype == np.float32
            assert len(_LQ["lq"]) == SC.M_ITEMS and np.isfinite(_LQ["lq"]).all() and len(set(_LQ["lq"].tolist())) > 3
        finally:
            pkg.world.configure([])
    return _LQ["lq"]


def _batches():
    return (IB.make_batch(65), IB.duplicated_positive_batch(), IB.one_user_batch(33), IB.make_batch(IB.SPLIT_B), IB.make_batch(1))


# ---- (a) both options off: the parent's restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("d,K", [(32, 1), (64, 3)])
def test_dot_without_logq_is_the_in_batch_restatement_array_equal(pkg, storage_graph, d, K):
    A, table = _inputs(pkg, storage_graph, d)
    for reg in (False, True):
        for w in (None, [0.4, 0.1, 0.3, 0.2][:K + 1]):
            for batch in _batches():
                a = IB.step(A, SC.N_USERS, K, SC.DECAY, 0.2, table, batch, reg, w)
                b = IS.step(A, SC.N_USERS, K, SC.DECAY, 0.2, table, batch, reg, w, score="dot", logq=None)
                for key, v in a.items():
                    if key == "loss_out":
                        assert all(float(x) == float(y) for x, y in zip(v, b[key]))
                    else:
                        assert np.array_equal(v.numpy(), b[key].numpy(), equal_nan=True), key
    v = IB.step(A, SC.N_USERS, K, SC.DECAY, 0.2, table, IB.make_batch(33)[0:2], B_norm=40)
    g = IS.step(A, SC.N_USERS, K, SC.DECAY, 0.2, table, IB.make_batch(33)[0:2], B_norm=40)
    assert np.array_equal(v["g_final"].numpy(), g["g_final"].numpy())


# ---- (b) the three new combinations are the autograd of the written loss --------------------------------------------------------
@pytest.mark.parametrize("tau", [0.2, 0.1])
@pytest.mark.parametrize("score,lq_on", IS.NEW_OPTIONS)
@pytest.mark.parametrize("d,K", [(32, 1), (64, 3)])
def test_restatement_is_the_autograd_of_the_written_loss(pkg, storage_graph, d, K, score, lq_on, tau):
    """g_final, G and the loss triple against torch float64 autograd of the loss written with F.normalize, the lq difference,
    torch.logsumexp and an explicit mask: 1e-12 relative, float64 against float64 -- the tolerance of
    tests/test_inbatch_host.py::test_restatement_is_the_autograd_of_the_written_loss for the same comparison."""
    A, table = _inputs(pkg, storage_graph, d)
    lq = _logq(pkg, storage_graph) if lq_on else None
    for reg in ("propagated", "ego"):
        for w in (None, [0.4, 0.1, 0.3, 0.2][:K + 1]):
            for batch in _batches():
                r = IS.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg == "ego", w, score=score, logq=lq)
                assert float(r["inv_u"].min()) > 0.0 and float(r["inv_p"].min()) > 0.0      # the torch pin uses non-zero rows
                E0 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
                E = IB.propagate(A, E0, K, w)
                E.retain_grad()
                loss, sm, reg_l = IS.loss(E, E0, SC.N_USERS, batch, SC.DECAY, tau, reg == "ego", score=score, logq=lq)
                loss.backward()
                for got, ref in zip(r["loss_out"], (loss.detach(), sm.detach(), reg_l.detach())):
                    assert abs(float(got) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
                scale = float(E0.grad.abs().max())
                assert float((r["G"] - E.grad).abs().max()) <= 1e-12 * scale
                assert float((r["g_final"] - E0.grad).abs().max()) <= 1e-12 * scale
                assert float(r["W"].sum(1).abs().max()) <= 1e-15                     # every row of W sums to zero


@pytest.mark.parametrize("score,lq_on", IS.NEW_OPTIONS)
def test_restatement_is_the_autograd_of_the_written_loss_across_three_parts(pkg, storage_graph, score, lq_on):
    """The same pin at B = 705 (three parts of the sweep), d = 64, K = 3, tau = 0.1, both reg rows: the restatement judges the device
    at B = 513 and B = 2048 (tests/test_gpu_inbatch_scores.py, section 1b).  1e-12 relative, as above."""
    A, table = _inputs(pkg, storage_graph, 64)
    lq = _logq(pkg, storage_graph) if lq_on else None
    B, K, tau = 705, 3, 0.1
    batch = IB.make_batch(B)
    assert IB.parts(B) == 3
    for reg in ("propagated", "ego"):
        r = IS.step(A, SC.N_USERS, K, SC.DECAY, tau, table, batch, reg == "ego", None, score=score, logq=lq)
        assert float(r["inv_u"].min()) > 0.0 and float(r["inv_p"].min()) > 0.0
        _pin(r, lambda E, E0: IS.loss(E, E0, SC.N_USERS, batch, SC.DECAY, tau, reg == "ego", score=score, logq=lq), A, table, K, None, B)
        assert float(r["W"].sum(1).abs().max()) <= 1e-15


def test_the_options_change_the_step(pkg, storage_graph):
    """(so that the comparisons above are not between two copies of the plain loss)"""
    A, table = _inputs(pkg, storage_graph, 32)
    batch = IB.make_batch(65)
    base = IB.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, batch)
    for score, lq_on in IS.NEW_OPTIONS:
        r = IS.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, batch, score=score, logq=_logq(pkg, storage_graph) if lq_on else None)
        assert abs(float(r["loss_out"][1]) - float(base["loss_out"][1])) > 1e-3
        assert float((r["g_final"] - base["g_final"]).abs().max()) > 1e-6
        assert float(r["loss_out"][2]) == float(base["loss_out"][2])                # the reg term stays on the raw rows


# ---- (c) a constant lq cancels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score", IS.SCORES)
def test_a_constant_logq_changes_nothing(pkg, storage_graph, score):
    """lq_{p_c} - lq_{p_b} is exactly 0 for a constant vector, and z - 0 is z: array-equal."""
    A, table = _inputs(pkg, storage_graph, 32)
    for batch in _batches():
        a = IS.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, batch, score=score, logq=None)
        b = IS.step(A, SC.N_USERS, 2, SC.DECAY, 0.2, table, batch, score=score, logq=np.full(SC.M_ITEMS, 3.25, np.float32))
        for key in ("z", "q", "W", "g_final", "lterm"):
            assert np.array_equal(a[key].numpy(), b[key].numpy()), key


# ---- (d) cosine ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lq_on", [False, True])
def test_cosine_ignores_the_length_of_a_row_and_its_gradient_is_orthogonal(pkg, storage_graph, lq_on):
    A, table = _inputs(pkg, storage_graph, 64)
    u, p = IB.make_batch(65)
    ut, pt = torch.from_numpy(u), torch.from_numpy(p)
    E = IB.propagate(A, torch.from_numpy(table.astype(np.float64)), 2)
    eu, ep = E[ut], E[SC.N_USERS + pt]
    lqb = torch.from_numpy(_logq(pkg, storage_graph).astype(np.float64))[pt] if lq_on else None
    B, tau = len(u), 0.2
    r = IS.rows(eu, ep, ut, pt, tau, B, "cosine", lqb)
    sm = float(r["lterm"].sum()) / B
    assert sm > 0.1
    for side, i, c in (("u", 0, 3.0), ("u", 20, 1e-3), ("p", 7, 64.0), ("p", 64, 0.25)):
        eu2, ep2 = eu.clone(), ep.clone()
        (eu2 if side == "u" else ep2)[i] *= c
        r2 = IS.rows(eu2, ep2, ut, pt, tau, B, "cosine", lqb)
        assert abs(float(r2["lterm"].sum()) / B - sm) <= 1e-13 * sm, (side, i, c)
    # the score part of each gradient row is orthogonal to its row: inv |e| = 1, so |gs.e| is a rounding of sum |W| |s| + |t|
    for gs, e, eh, oh, t, Wm in ((r["gs_u"], eu, r["eh_u"], r["eh_p"], r["t_u"], r["W"]), (r["gs_p"], ep, r["eh_p"], r["eh_u"], r["t_p"], r["W"].t())):
        scale = ((Wm.abs() @ oh.abs()) * eh.abs()).sum(1) + t.abs()
        dot = (gs * e).sum(1).abs()
        assert float(gs.abs().max()) > 0.0 and bool((dot <= 1e-12 * scale).all()), float((dot / scale).max())
    # a row of norm 0 scores 0 and receives no score gradient
    eu0 = eu.clone(); eu0[20] = 0.0
    r0 = IS.rows(eu0, ep, ut, pt, tau, B, "cosine", lqb, lam=1e-4)
    assert float(r0["inv_u"][20]) == 0.0 and float(r0["s"][20].abs().max()) == 0.0 and float(r0["gs_u"][20].abs().max()) == 0.0
    assert np.isfinite(r0["g_p"].numpy()).all() and np.isfinite(r0["lterm"].numpy()).all()


# ---- (e) surface -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lgcn_ctx_set_inbatch_scores", "lgcn_ctx_get_inbatch_scores")


def test_new_symbols_are_declared_bound_and_exported_with_abi_13(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lgcn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", hdr))
    lib = pkg._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lgcn_abi_version() == pkg._lib.ABI_VERSION == 13
    assert pkg._lib.SCORE_DOT == int(re.search(r"#define\s+LGCN_SCORE_DOT\s+(\d+)", hdr).group(1)) == 0
    assert pkg._lib.SCORE_COSINE == int(re.search(r"#define\s+LGCN_SCORE_COSINE\s+(\d+)", hdr).group(1)) == 1
    # what the host can refuse with no device: a null context, by name
    assert lib.lgcn_ctx_set_inbatch_scores(None, pkg._lib.SCORE_COSINE, None) == 3 and b"lgcn_ctx_set_inbatch_scores" in lib.lgcn_last_error()
    out = C.c_void_p(17)
    assert lib.lgcn_ctx_get_inbatch_scores(None, C.byref(out)) == -1 and out.value == 17


def test_score_flags_and_defaults(pkg):
    w = pkg.world
    try:
        w.configure([])
        assert w.config['score'] == 'dot' and w.config['inbatch_logq'] == 0
        assert pkg.model.resolve_inbatch_scores(w.config, 'bpr') == ('dot', False)
        assert pkg.model.resolve_inbatch_scores({}, 'softmax') == ('dot', False)
        w.configure(['--loss', 'inbatch', '--score', 'cosine', '--inbatch_logq', '1', '--softmax_temp', '0.1'])
        assert w.config['score'] == 'cosine' and w.config['inbatch_logq'] == 1
        assert pkg.model.resolve_inbatch_scores(w.config, 'inbatch') == ('cosine', True)
        for bad in (['--score', 'angle'], ['--inbatch_logq', '2']):
            with pytest.raises(SystemExit):
                w.configure(bad)
        helps = {a.dest: a.help for a in pkg.parse.build_parser()._actions}
        assert helps['score'].startswith('NEW') and helps['inbatch_logq'].startswith('NEW') and '--softmax_temp' in helps['score']
        with pytest.raises(ValueError, match="--score"):
            pkg.model.resolve_inbatch_scores({'score': 'angle'}, 'inbatch')
        with pytest.raises(ValueError, match="--inbatch_logq"):
            pkg.model.resolve_inbatch_scores({'inbatch_logq': 2}, 'inbatch')
    finally:
        w.configure([])


def test_refusals_that_need_no_device_name_the_flag(pkg, storage_graph):
    try:
        for loss in ('bpr', 'softmax'):
            with pytest.raises(pkg._lib.LgcnError, match="--score cosine"):
                _model_with(pkg, storage_graph, loss=loss, score='cosine')
            with pytest.raises(pkg._lib.LgcnError, match="--inbatch_logq 1"):
                _model_with(pkg, storage_graph, loss=loss, inbatch_logq=1)
        with pytest.raises(pkg._lib.LgcnError, match="--score"):
            _model_with(pkg, storage_graph, cls="PureMF", score='cosine')
        with pytest.raises(pkg._lib.LgcnError, match="--inbatch_logq"):
            _model_with(pkg, storage_graph, cls="PureMF", inbatch_logq=1)
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.5)
        assert m.score_kind == 'dot' and m.inbatch_logq is False and m._item_logq is None
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.1, score='cosine', inbatch_logq=1)
        assert m.score_kind == 'cosine' and m.inbatch_logq is True
        assert np.array_equal(m._item_logq.numpy(), _logq(pkg, storage_graph))
        ds, m = _model_with(pkg, storage_graph, cls="PureMF")                       # the defaults pass
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("score,lq_on", IS.NEW_OPTIONS)
@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_package_autograd_loss_is_the_restatement(pkg, storage_graph, reg, score, lq_on):
    """LightGCN.bpr_loss of a CPU model with the options on, the embeddings injected, at the fp32-vs-float64 tolerance 1e-6 of
    tests/test_inbatch_host.py::test_package_autograd_loss_is_the_restatement; and its gradient reaches the rows."""
    try:
        tau = 0.2
        ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=tau, reg_rows=reg, score=score, inbatch_logq=int(lq_on))
        lq = _logq(pkg, storage_graph) if lq_on else None
        A, _ = _inputs(pkg, storage_graph, 32)
        SC.configure(pkg, ("fp32", 32, 2, 1, -1, reg), storage_graph)
        E0 = m._table.detach().double()
        E = IB.propagate(A, E0, 2)
        Ef = E.float().requires_grad_(True)
        m.computer = lambda: (Ef[:SC.N_USERS], Ef[SC.N_USERS:])
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
        for batch in (IB.make_batch(65), IB.make_batch(2), IB.make_batch(1)):
            u, p = batch
            r = IS.step(A, SC.N_USERS, 2, SC.DECAY, tau, E0.numpy(), batch, reg == "ego", score=score, logq=lq)
            sm, rg = m.bpr_loss(t(u), t(p), t(p[::-1].copy()))
            assert abs(float(sm.detach()) - float(r["loss_out"][1])) < 1e-6 and abs(float(rg.detach()) - float(r["loss_out"][2])) < 1e-6
        u, p = IB.make_batch(65)
        r = IS.step(A, SC.N_USERS, 2, 0.0, tau, E0.numpy(), (u, p), False, score=score, logq=lq)
        sm, _ = m.bpr_loss(t(u), t(p), t(u))
        sm.backward()
        assert float((Ef.grad.double() - r["G"]).abs().max()) < 1e-6 * max(1.0, float(r["G"].abs().max()))
    finally:
        pkg.world.configure([])


def test_evaluation_ranks_the_normalised_rows_under_cosine(pkg, storage_graph):
    """getUsersRating of a CPU model under --score cosine is U^ P^^T of the propagated table; under dot it is U P^T as before."""
    try:
        A, _ = _inputs(pkg, storage_graph, 32)
        users = torch.arange(0, SC.N_USERS, 7)
        for score in ("dot", "cosine"):
            ds, m = _model_with(pkg, storage_graph, loss='inbatch', softmax_temp=0.2, score=score)
            E = IB.propagate(A, m._table.detach().double(), 2)
            m.computer = lambda: (E[:SC.N_USERS].float(), E[SC.N_USERS:].float())
            got = m.getUsersRating(users).double()
            Eu, Ep = E[:SC.N_USERS], E[SC.N_USERS:]
            if score == "cosine":
                Eu, Ep = IS.unit(Eu)[0], IS.unit(Ep)[0]
            want = Eu[users] @ Ep.t()
            assert float((got - want).abs().max()) < 1e-5
            if score == "cosine":
                assert float(got.abs().max()) <= 1.0 + 1e-5
    finally:
        pkg.world.configure([])

"""The alignment-and-uniformity loss (--loss directau) without a device: the float64 restatement
(tests/directau_restatement.py) is (a) pinned to torch float64 autograd of the loss written independently with F.normalize and
torch.pdist, (b) checked for its conventions (B = 1, one sound sample, gamma = 0, void samples against the divisors, what a lost
mask would cost); (c) the flags, the defaults, the refusals that need no device, the C ABI and the package's autograd loss."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import directau_restatement as DA               # noqa: E402
import inbatch_restatement as IB                 # noqa: E402
import storage_cases as SC                       # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import REPO                        # noqa: E402
from test_inbatch_host import _inputs, _model_with, _pin   # noqa: E402


def _batches():
    return (DA.make_batch(2), DA.make_batch(7), DA.make_batch(33), DA.make_batch(67))


# ---- (a) the restatement is the autograd of the written loss ------------------------------------------------------------------
@pytest.mark.parametrize("gamma", [1.0, 0.3])
@pytest.mark.parametrize("d,K", [(32, 1), (64, 2), (64, 3)])
def test_restatement_is_the_autograd_of_the_written_loss(pkg, storage_graph, d, K, gamma):
    """g_final, G and the loss triple against torch float64 autograd of the loss written with F.normalize and torch.pdist, both
    reg rows, mean and weighted layers, batches of 2, 7 (a repeated user, a repeated item, a mirror), 33 and 67: 1e-12 relative,
    float64 against float64 -- the tolerance of tests/test_inbatch_scores_host.py for its own restatement-against-autograd
    comparison."""
    A, table = _inputs(pkg, storage_graph, d)
    for reg in ("propagated", "ego"):
        for w in (None, [0.4, 0.1, 0.3, 0.2][:K + 1]):
            for batch in _batches():
                u, p = batch
                if len(u) >= 7:
                    assert u[1] == u[0] and p[3] == p[2] and (u[5], p[5]) == (u[4], p[4])
                r = DA.step(A, SC.N_USERS, K, SC.DECAY, gamma, table, batch, reg == "ego", w)
                assert float(r["inv_u"].min()) > 0.0 and float(r["inv_p"].min()) > 0.0      # the torch pin uses non-zero rows
                E0 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
                E = IB.propagate(A, E0, K, w)
                E.retain_grad()
                loss, au, reg_l = DA.loss(E, E0, SC.N_USERS, batch, SC.DECAY, gamma, reg == "ego")
                loss.backward()
                for got, ref in zip(r["loss_out"], (loss.detach(), au.detach(), reg_l.detach())):
                    assert abs(float(got) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
                scale = float(E0.grad.abs().max())
                assert float((r["G"] - E.grad).abs().max()) <= 1e-12 * scale
                assert float((r["g_final"] - E0.grad).abs().max()) <= 1e-12 * scale
                # the projected parts are orthogonal to their rows
                for g, e in ((r["ga_u"] + r["gu_u"], r["e_u"]), (r["ga_p"] + r["gu_p"], r["e_p"])):
                    assert float(((g * e).sum(1)).abs().max()) <= 1e-12 * float(g.abs().max() + 1e-300) * float(e.abs().max()) * d


@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_restatement_is_the_autograd_of_the_written_loss_across_three_parts(pkg, storage_graph, reg):
    """The same pin at B = 705 (23 tiles x 3 parts = 69 partials of the normaliser; a user, an item and a mirror repeated across
    parts), d = 64, K = 3, gamma = 1: the restatement judges the device at B = 705, 736 and 2048 (tests/test_gpu_directau.py,
    section 1b).  1e-12 relative, as above."""
    A, table = _inputs(pkg, storage_graph, 64)
    B, K = DA.MERGE_B, 3
    batch = DA.make_batch(B)
    u, p = batch
    assert DA.partials(B) == 69 and u[B - 1] in u[:256] and p[B - 1] in p[:256] and (u[500], p[500]) == (u[14], p[14])
    for w in (None, [0.4, 0.1, 0.3, 0.2]):
        r = DA.step(A, SC.N_USERS, K, SC.DECAY, 1.0, table, batch, reg == "ego", w)
        assert float(r["inv_u"].min()) > 0.0 and float(r["inv_p"].min()) > 0.0
        _pin(r, lambda E, E0: DA.loss(E, E0, SC.N_USERS, batch, SC.DECAY, 1.0, reg == "ego"), A, table, K, w, B)


def test_the_blocked_distance_matrix_is_the_whole_one(pkg, storage_graph):
    """directau_restatement.side forms the squared distances in blocks of 64 rows: array-equal to the one-expression form."""
    A, table = _inputs(pkg, storage_graph, 32)
    x = DA.unit(torch.from_numpy(table[20:277].astype(np.float64)))[0]
    k = DA.side(x, 1.0, len(x))[0]
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    assert torch.equal(k, torch.exp(-2.0 * d2) * (1.0 - torch.eye(len(x), dtype=DA.F64)))


# ---- (b) the conventions ------------------------------------------------------------------------------------------------------
def test_one_sample_and_one_sound_sample_have_no_uniformity(pkg, storage_graph):
    A, table = _inputs(pkg, storage_graph, 32)
    u, p = DA.make_batch(7)
    for B_norm in (1, 5):           # B = 1; one sound sample among five (four void)
        r = DA.step(A, SC.N_USERS, 2, SC.DECAY, 1.0, table, (u[:1], p[:1]), B_norm=B_norm)
        assert float(r["unif_x"]) == 0.0 and float(r["unif_y"]) == 0.0 and float(r["cst"]) == 0.0
        assert float(r["gu_u"].abs().max()) == 0.0 and float(r["gu_p"].abs().max()) == 0.0 and float(r["ga_u"].abs().max()) > 0.0
        assert abs(float(r["loss_out"][1]) - float(r["al"][0]) / B_norm) <= 1e-15
        assert np.isfinite(r["g_final"].numpy()).all()


def test_gamma_zero_is_the_alignment_loss_alone(pkg, storage_graph):
    A, table = _inputs(pkg, storage_graph, 32)
    batch = DA.make_batch(33)
    r = DA.step(A, SC.N_USERS, 2, SC.DECAY, 0.0, table, batch)
    assert float(r["cst"]) == 0.0 and float(r["W_x"].abs().max()) == 0.0 and float(r["gu_u"].abs().max()) == 0.0
    assert abs(float(r["loss_out"][1]) - float(r["al"].sum()) / 33) <= 1e-15
    r1 = DA.step(A, SC.N_USERS, 2, SC.DECAY, 1.0, table, batch)
    assert abs(float(r1["loss_out"][1]) - float(r["loss_out"][1])) > 1e-2           # (the term is not small on these inputs)
    assert np.array_equal(r["ga_u"].numpy(), r1["ga_u"].numpy())


def test_void_samples_leave_the_pairs_and_not_the_divisors(pkg, storage_graph):
    """Three samples of 33 void: the loss is that of the 30 sound ones with the divisors 33 and 33 * 32 / 2."""
    A, table = _inputs(pkg, storage_graph, 32)
    u, p = DA.make_batch(33)
    keep = np.ones(33, bool); keep[[0, 17, 32]] = False
    r = DA.step(A, SC.N_USERS, 2, SC.DECAY, 1.0, table, (u[keep], p[keep]), B_norm=33)
    s = DA.step(A, SC.N_USERS, 2, SC.DECAY, 1.0, table, (u[keep], p[keep]))
    assert abs(float(r["unif_x"]) - (float(s["unif_x"]) + np.log(DA.npairs(30) / DA.npairs(33)))) <= 1e-13
    assert abs(float(r["al"].sum()) / 33 + float(r["cst"]) - float(r["loss_out"][1])) <= 1e-15
    # the uniformity gradient does not see the divisor (it cancels in W = 2 gamma k / Z); the alignment gradient does
    assert float((r["gu_u"] - s["gu_u"]).abs().max()) <= 1e-15 and float((r["ga_u"] * 33 - s["ga_u"] * 30).abs().max()) <= 1e-13


@pytest.mark.parametrize("B", [7, 33])
def test_a_lost_mask_is_far_outside_the_bound_of_z(pkg, storage_graph, B):
    """What ONE zero row that is not masked would add to Z -- exp(-4) per pair with a unit row (|0 - x|^2 = 1 under the kernel's
    (q_b + q_c) - 2 s) -- against the Z line of tests/directau_bounds.py for the inputs of
    tests/test_gpu_directau.py::test_void_samples_and_padding_are_masked (fp32 tables, d = 64, K = 1, gamma = 1, the storage
    table): more than 10 times the bound on both sides, so the bound of the terms and of the gradient cannot hide it."""
    import directau_bounds as DB
    try:
        ds, m = SC.make_model(pkg, ("fp32", 64, 1, 1, -1, "propagated"), storage_graph)
        adj = ds.getSparseGraphCSR()
    finally:
        pkg.world.configure([])
    A, table = _inputs(pkg, storage_graph, 64)
    u, p = DA.make_batch(B, seed=5)
    keep = np.ones(B, bool); keep[[0, B - 1]] = False
    sb = (u[keep], p[keep])
    r = DA.step(A, SC.N_USERS, 1, SC.DECAY, 1.0, table, sb, B_norm=B)
    bd = DB.bounds(adj, r, sb, B, 1, 64, "fp32", False, None, 1.0)
    lost = (B - 2) * np.exp(-4.0)
    assert lost > 10 * bd["dZ"][0] and lost > 10 * bd["dZ"][1], (lost, bd["dZ"])
    # ... and in the loss: the constant moves by more than 10 times its bound
    for Z in (float(r["Z_x"]), float(r["Z_y"])):
        assert 0.5 * np.log1p(lost / Z) > 10 * bd["void_term"]


# ---- (c) surface -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("lgcn_ctx_set_directau", "lgcn_ctx_get_directau", "lgcn_train_step_directau", "lgcn_train_epoch_directau")


def test_new_symbols_are_declared_bound_and_exported_with_abi_13(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lgcn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", hdr))
    lib = pkg._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lgcn_abi_version() == pkg._lib.ABI_VERSION == 13
    assert pkg._lib.LOSS_DIRECTAU == int(re.search(r"#define\s+LGCN_LOSS_DIRECTAU\s+(\d+)", hdr).group(1)) == 4
    # what the host can refuse with no device: a null context, by name
    assert lib.lgcn_ctx_set_directau(None, 1.0) == 3 and b"lgcn_ctx_set_directau" in lib.lgcn_last_error()
    g = C.c_float(17.0)
    assert lib.lgcn_ctx_get_directau(None, C.byref(g)) == 3 and g.value == 17.0 and b"lgcn_ctx_get_directau" in lib.lgcn_last_error()
    buf = (C.c_int32 * 4)()
    out = (C.c_float * 3)(-7.0, -7.0, -7.0)
    assert lib.lgcn_train_step_directau(None, buf, buf, 4, out, None) == 3 and b"lgcn_train_step_directau" in lib.lgcn_last_error()
    assert lib.lgcn_train_epoch_directau(None, buf, buf, 4, 4, out, None) == 3 and b"lgcn_train_epoch_directau" in lib.lgcn_last_error()
    assert list(out) == [-7.0, -7.0, -7.0]
    assert lib.lgcn_ctx_set_loss(None, pkg._lib.LOSS_DIRECTAU, 1.0) == 3


def test_flags_and_defaults(pkg):
    w = pkg.world
    try:
        w.configure([])
        assert w.config['loss'] == 'bpr' and w.config['au_gamma'] == 1.0
        assert pkg.model.resolve_loss(w.config) == ('bpr', 1.0) and pkg.model.resolve_loss({})[0] == 'bpr'
        w.configure(['--loss', 'directau'])
        assert w.config['loss'] == 'directau' and w.config['au_gamma'] == 1.0
        assert pkg.model.resolve_loss(w.config)[0] == 'directau' and pkg.model.resolve_au_gamma(w.config, 'directau') == 1.0
        w.configure(['--loss', 'directau', '--au_gamma', '0.5', '--softmax_temp', '-3'])       # the temperature is not looked at
        assert w.config['au_gamma'] == 0.5 and pkg.model.resolve_loss(w.config) == ('directau', 1.0)
        with pytest.raises(SystemExit):
            w.configure(['--loss', 'au'])
        helps = {a.dest: a.help for a in pkg.parse.build_parser()._actions}
        assert helps['au_gamma'].startswith('NEW') and 'directau' in helps['loss'] and '--loss directau' in helps['au_gamma']
        for bad in (float('nan'), float('inf'), -1.0):
            with pytest.raises(ValueError, match="--au_gamma"):
                pkg.model.resolve_au_gamma({'au_gamma': bad}, 'directau')
        assert pkg.model.resolve_au_gamma({'au_gamma': float('nan')}, 'bpr') == 1.0           # not looked at under another loss
        with pytest.raises(ValueError, match="--loss"):
            pkg.model.resolve_loss({'loss': 'au'})
    finally:
        w.configure([])


def test_refusals_that_need_no_device_name_the_flag(pkg, storage_graph):
    try:
        ds, m = _model_with(pkg, storage_graph)
        assert m.loss_kind == 'bpr'
        ds, m = _model_with(pkg, storage_graph, loss='directau', au_gamma=0.5, softmax_temp=-1.0)
        assert m.loss_kind == 'directau' and m.au_gamma == 0.5
        assert ('lgcn_ctx_set_directau', (0.5,)) in m._ctx_setters({}, 0) and not any(n == 'lgcn_ctx_set_loss' for n, _ in m._ctx_setters({}, 0))
        for bad in (float('nan'), float('inf'), -1.0):
            with pytest.raises(ValueError, match="--au_gamma"):
                _model_with(pkg, storage_graph, loss='directau', au_gamma=bad)
        for cfg, flag in ((dict(neg_ratio=4), "--neg_ratio 4"), (dict(neg_ratio=4, hard_neg=2), "--hard_neg 2"),
                          (dict(inbatch_mix=1), "--inbatch_mix 1"), (dict(score='cosine'), "--score cosine"),
                          (dict(inbatch_logq=1), "--inbatch_logq 1"), (dict(act_dtype='fp8'), "fp8"),
                          (dict(use_pop_gate=True), "--use_pop_gate"), (dict(use_item_item=True), "--use_item_item")):
            with pytest.raises(pkg._lib.LgcnError, match=flag) as e:
                _model_with(pkg, storage_graph, loss='directau', **cfg)
            assert "directau" in str(e.value), (cfg, str(e.value))
        with pytest.raises(pkg._lib.LgcnError, match="--loss directau"):
            _model_with(pkg, storage_graph, cls="PureMF", loss='directau')
        ds, m = _model_with(pkg, storage_graph, loss='directau')
        with pytest.raises(RuntimeError, match="--loss directau"):
            pkg.parallel.DataParallelBPR(m, pkg.world.config)
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_package_autograd_loss_is_the_restatement(pkg, storage_graph, reg):
    """LightGCN.bpr_loss under --loss directau on a CPU model, the embeddings injected, at the fp32-vs-float64 tolerance 1e-6 of
    tests/test_inbatch_host.py::test_package_autograd_loss_is_the_restatement; and its gradient reaches the rows."""
    try:
        gamma = 0.7
        ds, m = _model_with(pkg, storage_graph, loss='directau', au_gamma=gamma, reg_rows=reg)
        A, _ = _inputs(pkg, storage_graph, 32)
        SC.configure(pkg, ("fp32", 32, 2, 1, -1, reg), storage_graph)
        E0 = m._table.detach().double()
        E = IB.propagate(A, E0, 2)
        Ef = E.float().requires_grad_(True)
        m.computer = lambda: (Ef[:SC.N_USERS], Ef[SC.N_USERS:])
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
        for batch in (DA.make_batch(67), DA.make_batch(2), DA.make_batch(1)):
            u, p = batch
            r = DA.step(A, SC.N_USERS, 2, SC.DECAY, gamma, E0.numpy(), batch, reg == "ego")
            au, rg = m.bpr_loss(t(u), t(p), t(p[::-1].copy()))
            assert abs(float(au.detach()) - float(r["loss_out"][1])) < 1e-6 and abs(float(rg.detach()) - float(r["loss_out"][2])) < 1e-6
        u, p = DA.make_batch(67)
        r = DA.step(A, SC.N_USERS, 2, 0.0, gamma, E0.numpy(), (u, p), False)
        au, _ = m.bpr_loss(t(u), t(p), t(u))
        au.backward()
        assert float((Ef.grad.double() - r["G"]).abs().max()) < 1e-6 * max(1.0, float(r["G"].abs().max()))
    finally:
        pkg.world.configure([])

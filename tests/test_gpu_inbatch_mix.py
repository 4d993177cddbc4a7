"""Mixed negative sampling for the in-batch softmax (--inbatch_mix 1; lgcn_train_step_inbatch_mix, csrc/lgcn_inbatch.hip, DESIGN
4.21) on the GPU (-m gpu), on the graph and table rows of tests/storage_cases.py, against the float64 restatement
tests/inbatch_mix_restatement.py.  Every step is judged from the GPU's OWN state before the step: per-sample terms, loss_out, the
gradient recovered from Adam's first moment, and Adam itself.

BOUNDS: derived in the docstring of tests/inbatch_mix_bounds.py (to first order in u = 2^-24 from the lines of
tests/test_gpu_inbatch.py and tests/test_gpu_inbatch_scores.py: NP is the part count of the (1 + R) Bp-row item sweep in kZ and
in the fixed-point line, a user row takes that many partial adds and a pool row the user side's, the reg line gains the 1/R
terms), in a module without a device because tests/test_inbatch_mix_host.py evaluates the same bound on the CPU: a step that
ignored the pool would miss the bound on `terms` in every case below.  The same check is repeated here at every step, from the
device's own state.  Every test prints the largest share of each bound it used (recorded in profiles/inbatch_mix/README.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import inbatch_mix_bounds as MB
import inbatch_mix_restatement as IM
import inbatch_restatement as IB
import storage_cases as SC
import test_gpu_softmax as SMT
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)
from test_gpu_gate_shapes import W1, _adam_checks
from test_gpu_inbatch import _G, _dev, _model, _same, _snapshot, _state, _uncovered

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = SC.U

assert not _uncovered(MB.CASES), _uncovered(MB.CASES)
assert all({c[a] for c in MB.CASES} == set(ax) for a, ax in enumerate(MB.AXES))


def _cfg(tau, R, score="dot", lq_on=False, **more):
    return dict(loss='inbatch', softmax_temp=tau, score=score, inbatch_logq=int(lq_on), inbatch_mix=1, neg_ratio=R, **more)


def _judge(pkg, ds, m, batch, K, d, mode, reg, tau, step_no, tag, score, lq_on, void=()):
    """One fused mixed step from the GPU's own state -> ({link: share of its bound}, restatement, raw outputs)."""
    A = _G["A"]
    ego = reg == "ego"
    u, p, negs = batch
    B, R = negs.shape
    st = m._state(max_batch=max(B, int(m.config.get('bpr_batch_size', B))), need_ctx=True)
    lib = pkg._lib.load()
    assert lib.lgcn_ctx_get_inbatch_mix(st['ctx']) == m.neg_ratio >= R
    lq = st['item_logq'].cpu().numpy() if lq_on else None
    if lq_on:       # the mixture's vector at B = --bpr_batch, R = --neg_ratio
        assert np.array_equal(lq, IM.item_logq_mix(ds.items_D, int(m.config['bpr_batch_size']), m.neg_ratio))
    assert m.adam_step == step_no - 1
    before = _state(m)
    out = m.fused_step(_dev(u), _dev(p), _dev(negs)).cpu().numpy().astype(np.float64)
    after = _state(m)
    t = m._dev['terms'].cpu().numpy().astype(np.float64)
    term, regt = t[:B], t[B:2 * B]
    sound = np.ones(B, bool)
    for v_ in void:
        sound[v_] = False
        assert term[v_] == 0.0 and regt[v_] == 0.0
    sb = (np.asarray(u)[sound], np.asarray(p)[sound], np.asarray(negs)[sound])
    # the restatement with the pool, the one without it, and how far the latter misses the bound on a term
    sens, r, _ = MB.sensitivity(_G["adj"], A, before["table"], sb, B, K, d, mode, ego, tau, score, lq, B_norm=B)
    assert sens > 1.0, (tag, sens)
    if score == "cosine":
        assert min(float((r[k] ** 2).sum(1).min()) for k in ("e_u", "e_p", "e_n")) >= MB.MIN_N2
    bd = MB.bounds(_G["adj"], r, sb, B, K, d, mode, ego, tau, score == "cosine", lq_on)
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
    z, mm = r["z"].numpy(), r["m"].numpy()
    nb = len(sb[0])
    kinds = (int(((mm > 0) & (z.argmax(1) >= nb)).sum()), int(((mm > 0) & (z.argmax(1) < nb)).sum()), int((mm == 0).sum()), int((~r["keep"].numpy()[:, nb:]).sum()))
    print(f"[inbatch_mix] {tag}: shares " + " ".join(f"{k}={v:.3f}" for k, v in share.items())
          + f" | without the pool {sens:.3g} bounds off | rows with the maximum in the pool / in the batch / M = 0: {kinds[0]} / {kinds[1]} / {kinds[2]}, masked pool pairs {kinds[3]}")
    return share, r, (term, regt, g_rec, slack, bd, out)


def _run(pkg, path, mode, d, K, B, R, tau, reg, score, lq_on, batches):
    try:
        ds, m = _model(pkg, path, mode, d, K, reg, dl=0, batch=B, **_cfg(tau, R, score, lq_on))
        top, bad = {}, []
        for i, batch in enumerate(batches):
            tag = f"{score}{'+logq' if lq_on else ''} {mode} d{d} K{K} R{R} tau{tau} {reg} step {i + 1} B={len(batch[0])}"
            share = _judge(pkg, ds, m, batch, K, d, mode, reg, MB.tau32(tau), i + 1, tag, score, lq_on)[0]
            for k_, v in share.items():
                top[k_] = max(top.get(k_, 0.0), v)
                if not v <= 1.0:
                    bad.append((tag, k_, v))
            m.check_device_errors()
            assert not bool(m._dev['G64'].any()) and m.adam_step == i + 1
        assert m._dev['dense_last'] is True
        print(f"[inbatch_mix] {score}{'+logq' if lq_on else ''} {mode} d{d} K{K} B{B} R{R} tau{tau} {reg} TOP: " + " ".join(f"{k_}={v:.3f}" for k_, v in top.items()))
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
    finally:
        pkg.world.configure([])


# ---- 1. steps against the float64 restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id=MB.case_id(c)) for c in MB.CASES])
def test_steps_equal_the_restatement(pkg, storage_graph, case):
    """Per-sample terms, loss_out, the gradient recovered from Adam's first moment and Adam itself, each within the bound derived
    in tests/inbatch_mix_bounds.py, over consecutive batches; the batches hold a masked pool id, a pool id that is another
    sample's positive and duplicate pool ids (tests/inbatch_mix_restatement.py::make_batch)."""
    B, R, d, K, mode, reg, tau, (score, lq_on) = case
    _run(pkg, storage_graph, mode, d, K, B, R, tau, reg, score, lq_on, MB.case_batches(case))


# ---- 1b. the batch sizes the loss is trained and timed at ----------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id=MB.case_id(c)) for c in MB.LARGE_CASES])
def test_steps_equal_the_restatement_at_the_training_batch_sizes(pkg, storage_graph, case):
    """Section 1 at (B, R) = (2048, 1) and (545, 16) (inbatch_mix_bounds.LARGE_CASES): eight and three parts on the USER side of the
    step, which section 1 never takes beyond two; the same links within the same derived bounds (functions of B and R through
    NP, NPu, the chain lengths and c(B)), over two consecutive batches that repeat a user, a positive and a pool id across parts."""
    B, R, d, K, mode, reg, tau, (score, lq_on) = case
    _run(pkg, storage_graph, mode, d, K, B, R, tau, reg, score, lq_on, MB.case_batches(case))


# ---- 2. voids ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("score,lq_on", MB.OS)
def test_an_out_of_range_negative_in_the_last_part_voids_the_sample(pkg, storage_graph, score, lq_on):
    """test_an_out_of_range_negative_voids_the_sample at B = 513 (three user parts, the third one tile with one live row): the bad
    negatives in part 1 (row 300) and in row 512, after which the last user part holds no sound sample at all."""
    try:
        d, K, B, R = 64, 1, IB.MANY_PARTS_B, 2
        u, p, negs = IM.make_batch(B, R, seed=5)
        negs = negs.copy()
        void = (300, B - 1)
        assert IB.last_part_rows(B).tolist() == [B - 1]
        negs[B - 1, 1] = SC.M_ITEMS + 2
        negs[300, 0] = -1
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **_cfg(0.2, R, score, lq_on))
        share = _judge(pkg, ds, m, (u, p, negs), K, d, "fp32", "propagated", MB.tau32(0.2), 1, f"void negative {score} B={B}", score, lq_on, void=void)[0]
        assert all(v <= 1.0 for v in share.values()), share
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])



@pytest.mark.parametrize("score,lq_on", MB.OS)
def test_an_out_of_range_negative_voids_the_sample(pkg, storage_graph, score, lq_on):
    """One negative id beyond the items (and one below zero) in a batch of 65, R = 2: err is set, the id check precedes the lq
    gather, the sample is void as row, as in-batch column and as pool columns -- its SOUND negative of the other column is no
    pool column either -- and the rest is the restatement of the sound samples normalised by the original B."""
    try:
        d, K, B, R = 64, 1, 65, 2
        u, p, negs = IM.make_batch(B, R, seed=5)
        negs = negs.copy()
        void = (7, 33)
        negs[7, 1] = SC.M_ITEMS + 2
        negs[33, 0] = -1
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **_cfg(0.2, R, score, lq_on))
        share = _judge(pkg, ds, m, (u, p, negs), K, d, "fp32", "propagated", MB.tau32(0.2), 1, f"void negative {score}", score, lq_on, void=void)[0]
        assert all(v <= 1.0 for v in share.values()), share
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert not bool(m._dev['G64'].any())
    finally:
        pkg.world.configure([])


# ---- 3. B = 1 is the sampled softmax -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,d,mode", [(1, 64, "fp32"), (16, 32, "bf16"), (5, 256, "fp32")])
def test_one_sample_agrees_with_the_sampled_softmax_step(pkg, storage_graph, R, d, mode):
    """lgcn_train_step_inbatch_mix at B = 1 against lgcn_train_step_multi under LGCN_LOSS_SOFTMAX from the same state: the two
    restatements are one (tests/test_inbatch_mix_host.py, 1e-12), so the outputs agree within the SUM of the two tests' bounds."""
    try:
        K, tau = 2, 0.2
        batch = IM.make_batch(1, R, seed=R, plain=True)
        _, ms = SMT._model(pkg, storage_graph, mode, d, K, batch=1, loss='softmax', softmax_temp=tau, neg_ratio=R)
        _, _, (term_s, regt_s, g_s, slack_s, bd_s) = SMT._judge(pkg, ms, batch, R, K, d, mode, "propagated", MB.tau32(tau), 1, f"softmax B=1 R={R}")
        ds, mx = _model(pkg, storage_graph, mode, d, K, batch=1, **_cfg(tau, R))
        share, r, (term_m, regt_m, g_m, slack_m, bd_m, out_m) = _judge(pkg, ds, mx, batch, K, d, mode, "propagated", MB.tau32(tau), 1,
                                                                       f"mix B=1 R={R} {mode} d{d}", "dot", False)
        assert all(v <= 1.0 for v in share.values()), share
        assert abs(term_m[0] - term_s[0]) <= bd_m["term"][0] + bd_s["term"][0]
        assert abs(regt_m[0] - regt_s[0]) <= bd_m["regterm"][0] + bd_s["regterm"][0]
        assert bool((np.abs(g_m - g_s) <= bd_m["g_final"] + bd_s["g_final"] + slack_m + slack_s).all())
        assert float(np.abs(g_m).max()) > 0.0
    finally:
        pkg.world.configure([])


# ---- 4. determinism, the epoch entry -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,B,R,d", [("fp32", 260, 2, 64), ("bf16", 100, 16, 256)])
def test_the_same_step_twice_is_bitwise_the_same(pkg, storage_graph, mode, B, R, d):
    try:
        res = []
        for _ in range(2):
            _, m = _model(pkg, storage_graph, mode, d, 2, batch=B, **_cfg(0.1, R, "cosine", True))
            outs = [m.fused_step(_dev(u), _dev(p), _dev(n)).clone() for u, p, n in IM.make_batches(B, R, 2, seed=9)]
            m.check_device_errors()
            res.append(outs + [m._table.detach().clone(), m._dev['adam_m'].clone(), m._dev['adam_v'].clone(), m._dev['terms'].clone()])
        for a, b in zip(*res):
            assert torch.equal(a, b)
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("mode,K,R,score,lq_on", [("fp32", 1, 1, "cosine", True), ("bf16", 2, 3, "dot", False)])
def test_epoch_equals_the_loop_of_steps_bitwise(pkg, storage_graph, mode, K, R, score, lq_on):
    """lgcn_train_epoch_inbatch_mix over T = 165 (batches of 64, 64, 37; negs [R][T]) against the loop of
    lgcn_train_step_inbatch_mix: loss rows, table, both Adam moments bit for bit."""
    try:
        B, T, d = 64, 165, 64
        cfg = _cfg(0.2, R, score, lq_on)
        u, p, negs = IM.make_batch(T, R, seed=1)
        _, a = _model(pkg, storage_graph, mode, d, K, **cfg)
        want = a.fused_epoch(_dev(u), _dev(p), _dev(negs if R > 1 else negs.reshape(-1)), B)
        a.check_device_errors()
        _, b = _model(pkg, storage_graph, mode, d, K, **cfg)
        first = b._table.detach().clone()
        got = [b.fused_step(_dev(u[t:t + B]), _dev(p[t:t + B]), _dev(negs[t:t + B].T.copy())) for t in range(0, T, B)]
        b.check_device_errors()
        assert a.adam_step == b.adam_step == 3 and want.shape == (3, 3)
        assert torch.equal(torch.stack(got), want), (torch.stack(got), want)
        assert torch.equal(a._table, b._table), int((a._table != b._table).sum())
        assert torch.equal(a._dev['adam_m'], b._dev['adam_m']) and torch.equal(a._dev['adam_v'], b._dev['adam_v'])
        assert not bool(a._dev['G64'].any()) and not bool(b._dev['G64'].any())
        assert float((b._table - first).abs().max()) > 1e-4                 # (it trained)
    finally:
        pkg.world.configure([])


# ---- 5. the plain step on a context with mixing set ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,d,score,lq_on", [("fp32", 64, "dot", False), ("bf16", 128, "cosine", True)])
def test_the_plain_step_after_a_mixed_step_is_that_of_a_fresh_context(pkg, storage_graph, mode, d, score, lq_on):
    """Workspace isolation: a context with mixing set runs a mixed step and then plain lgcn_train_step_inbatch steps; a context
    never told runs a plain step in place of the mixed one and is then handed the first context's state.  From equal tables
    onwards the plain steps are bit for bit the same -- nothing of the mixed step's workspace reaches them."""
    try:
        L = pkg._lib
        lib = L.load()
        B, R, K = 100, 4, 2
        plain_cfg = dict(loss='inbatch', softmax_temp=0.2, score=score, inbatch_logq=int(lq_on))
        _, a = _model(pkg, storage_graph, mode, d, K, batch=B, **plain_cfg)
        sa = a._state(max_batch=B, need_ctx=True)
        assert lib.lgcn_ctx_get_inbatch_mix(sa['ctx']) == 0
        L.check(lib.lgcn_ctx_set_inbatch_mix(sa['ctx'], R), "lgcn_ctx_set_inbatch_mix")
        assert lib.lgcn_ctx_get_inbatch_mix(sa['ctx']) == R
        u, p, negs = IM.make_batch(B, R, seed=3)
        du, dp, nt = _dev(u), _dev(p), _dev(negs.T.copy())                  # (held: the launches read them after the call returns)
        loss = torch.empty(3, dtype=torch.float32, device=DEV)
        L.check(lib.lgcn_train_step_inbatch_mix(sa['ctx'], L.tp(du), L.tp(dp), L.tp(nt), B, R, B, L.tp(loss), L.current_stream()), "mixed step")
        a.check_device_errors()
        _, b = _model(pkg, storage_graph, mode, d, K, batch=B, **plain_cfg)
        sb = b._state(max_batch=B, need_ctx=True)
        b.fused_step(_dev(u), _dev(p), _dev(u))                              # (one plain step: the same step count, both bitmaps used)
        b.check_device_errors()
        with torch.no_grad():
            b._table.copy_(a._table); sb['adam_m'].copy_(sa['adam_m']); sb['adam_v'].copy_(sa['adam_v'])
        assert a.adam_step == b.adam_step == 1
        for i, (u2, p2) in enumerate(IB.make_batches(B, 2, seed=6)):
            oa = a.fused_step(_dev(u2), _dev(p2), _dev(u2)).clone()          # mixing is set on the context, not on the model: the plain entry
            ob = b.fused_step(_dev(u2), _dev(p2), _dev(u2)).clone()
            assert torch.equal(oa, ob), (i, oa, ob)
        a.check_device_errors(); b.check_device_errors()
        assert torch.equal(a._table, b._table) and torch.equal(sa['adam_m'], sb['adam_m']) and torch.equal(sa['adam_v'], sb['adam_v'])
        assert torch.equal(sa['terms'][:2 * B], sb['terms'][:2 * B])
    finally:
        pkg.world.configure([])


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched(pkg, storage_graph):
    try:
        L = pkg._lib
        lib = L.load()
        B, R = 64, 3
        ds, m = _model(pkg, storage_graph, "fp32", 64, 2, batch=B, **_cfg(0.2, R))
        st = m._state(max_batch=B, need_ctx=True)
        ctx = st['ctx']
        u, p, negs = IM.make_batch(B, R)
        du, dp, dn = _dev(u), _dev(p), _dev(negs.T.copy())
        m.fused_step(du, dp, dn)
        m.check_device_errors()
        before = _snapshot(lib, m, st)
        loss = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
        s = L.current_stream()

        def refused(rc, *words):
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and all(w in msg for w in words), (rc, msg, words)

        step, epoch = lib.lgcn_train_step_inbatch_mix, lib.lgcn_train_epoch_inbatch_mix
        for R_bad in (0, -1, R + 1, 17):
            refused(step(ctx, L.tp(du), L.tp(dp), L.tp(dn), B, R_bad, B, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "negative ratio")
            refused(epoch(ctx, L.tp(du), L.tp(dp), L.tp(dn), R_bad, B, B, L.tp(loss), s), "lgcn_train_epoch_inbatch_mix", "negative ratio")
        refused(step(ctx, L.tp(du), L.tp(dp), L.tp(dn), B - 1, R, B, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "neg_stride")
        refused(step(ctx, L.tp(du), L.tp(dp), L.tp(dn), B, R, B + 1, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "max_batch")
        refused(step(ctx, L.tp(du), L.tp(dp), L.tp(dn), B, R, 0, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "batch size")
        refused(epoch(ctx, L.tp(du), L.tp(dp), L.tp(dn), R, B, B + 1, L.tp(loss), s), "lgcn_train_epoch_inbatch_mix", "max_batch")
        for args in ((None, L.tp(dp), L.tp(dn)), (L.tp(du), None, L.tp(dn)), (L.tp(du), L.tp(dp), None)):
            refused(step(ctx, *args, B, R, B, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "null")
            refused(epoch(ctx, *args, R, B, B, L.tp(loss), s), "lgcn_train_epoch_inbatch_mix", "null")
        refused(step(ctx, L.tp(du), L.tp(dp), L.tp(dn), B, R, B, None, s), "lgcn_train_step_inbatch_mix", "null")
        # the setter: out of range by name, nothing changed
        for bad in (-1, 17, 1 << 20):
            refused(lib.lgcn_ctx_set_inbatch_mix(ctx, bad), "lgcn_ctx_set_inbatch_mix", "R_max")
        assert lib.lgcn_ctx_get_inbatch_mix(ctx) == R
        # every other entry point keeps refusing as before
        refused(lib.lgcn_train_step(ctx, L.tp(du), L.tp(dp), L.tp(dn), B, L.tp(loss), s), "lgcn_train_step", "inbatch")
        refused(lib.lgcn_train_step_multi(ctx, L.tp(du), L.tp(dp), L.tp(dn), B, R, B, L.tp(loss), s), "lgcn_train_step_multi", "inbatch")
        # mixing off: the mixed entry points refuse, the setter wants the in-batch loss
        L.check(lib.lgcn_ctx_set_inbatch_mix(ctx, 0), "off")
        refused(step(ctx, L.tp(du), L.tp(dp), L.tp(dn), B, R, B, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "lgcn_ctx_set_inbatch_mix")
        L.check(lib.lgcn_ctx_set_inbatch_mix(ctx, R), "on again")
        L.check(lib.lgcn_ctx_set_loss(ctx, L.LOSS_SOFTMAX, 0.2), "softmax")
        refused(step(ctx, L.tp(du), L.tp(dp), L.tp(dn), B, R, B, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "inbatch")
        refused(lib.lgcn_ctx_set_inbatch_mix(ctx, 2), "lgcn_ctx_set_inbatch_mix", "inbatch")
        assert lib.lgcn_ctx_get_inbatch_mix(ctx) == R
        L.check(lib.lgcn_ctx_set_loss(ctx, L.LOSS_INBATCH, 0.2), "inbatch again")
        torch.cuda.synchronize()
        assert bool((loss == -7.0).all())
        _same(before, _snapshot(lib, m, st))
        # ... and the same context takes a sound call afterwards, the one a context that saw no refusal takes
        o1 = m.fused_step(du, dp, dn).clone()
        m.check_device_errors()
        _, m2 = _model(pkg, storage_graph, "fp32", 64, 2, batch=B, **_cfg(0.2, R))
        m2.fused_step(du, dp, dn)
        o2 = m2.fused_step(du, dp, dn).clone()
        assert torch.equal(o1, o2) and torch.equal(m._table, m2._table)
        # a context whose loss was never inbatch
        _, m3 = _model(pkg, storage_graph, "fp32", 64, 2, batch=B)
        st3 = m3._state(max_batch=B, need_ctx=True)
        refused(lib.lgcn_ctx_set_inbatch_mix(st3['ctx'], 2), "lgcn_ctx_set_inbatch_mix", "inbatch")
        refused(step(st3['ctx'], L.tp(du), L.tp(dp), L.tp(dn), B, R, B, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "inbatch")
    finally:
        pkg.world.configure([])


# ---- 7. the Python path ------------------------------------------------------------------------------------------------------
def test_fused_step_fused_epoch_and_autograd_agree(pkg, storage_graph):
    """One batch of 33, R = 2, cosine + logq: fused_step and a one-batch fused_epoch are bit for bit the same, with neg given as
    [B, R] and as [R, B]; bpr_loss (autograd, fp32) returns the fused step's (sm, reg) and its gradient is the one the fused step
    fed Adam with, both at the fp32-vs-float64 tolerance 1e-6 the host tests use for bpr_loss against the restatement."""
    try:
        B, R, d, K, tau = 33, 2, 64, 2, 0.2
        cfg = _cfg(tau, R, "cosine", True)
        u, p, negs = IM.make_batch(B, R, seed=4)
        res = []
        for how in ("step", "step_rt", "epoch"):
            ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **cfg)
            m._state(max_batch=B, need_ctx=True)
            before = _state(m)
            if how == "epoch":
                out = m.fused_epoch(_dev(u), _dev(p), _dev(negs), B)[0]
            else:
                out = m.fused_step(_dev(u), _dev(p), _dev(negs if how == "step" else negs.T.copy()))
            m.check_device_errors()
            res.append((out.clone(), m._table.detach().clone(), m._dev['adam_m'].clone()))
        for other in res[1:]:
            for x, y in zip(res[0], other):
                assert torch.equal(x, y)
        ds, m = _model(pkg, storage_graph, "fp32", d, K, batch=B, **cfg)
        m._state(max_batch=B, need_ctx=True)
        t = lambda a_: torch.from_numpy(np.asarray(a_, np.int64)).to(DEV)
        sm, reg = m.bpr_loss(t(u), t(p), t(negs))
        out = res[0][0].double().cpu().numpy()
        assert abs(float(sm.detach()) - out[1]) < 1e-6 and abs(float(reg.detach()) - out[2]) < 1e-6
        (sm + SC.DECAY * reg).backward()
        g_auto = torch.cat([m.embedding_user.weight.grad, m.embedding_item.weight.grad]).double().cpu().numpy()
        g_rec = before["M"] + (res[0][2].double().cpu().numpy() - before["M"]) / W1
        assert float(np.abs(g_auto).max()) > 0.0
        assert float(np.abs(g_auto - g_rec).max()) < 1e-6 * max(1.0, float(np.abs(g_rec).max()))
    finally:
        pkg.world.configure([])

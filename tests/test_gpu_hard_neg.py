"""Hard negatives, DNS(M, N), in the fused step (--hard_neg M with --neg_ratio R; lgcn_ctx_set_hard_neg, csrc/lgcn_hardneg.hip,
DESIGN 4.25) on the GPU (-m gpu), on the graph and table rows of tests/storage_cases.py with the cases of
tests/hard_neg_restatement.py.

A  the selection is valid: the candidates' float64 scores are formed from the tables the kernel read -- the forward tables made
   with the public calls on the model's own graph (tests/test_gpu_storage_step.py: the same launches on the same plan, the same
   bits; bf16 storage: the stored bf16 tables), combined as slot_row combines them -- and |s64[sel_b] - s64_sorted[j_b]| <= 2 bound_b
   for EVERY sample, bound_b derived in tests/hard_neg_restatement.py.  tests/test_hard_neg_host.py shows that on these fixtures the
   bound forces the exact choice for at least 95 % of the samples.
B  the step is the BPR step on the selection: given the device's sel, test_gpu_multineg._judge_pair at R = 1 judges the step
   from the same state, link by link.  The per-sample terms, the loss triple and the gradient recovered from Adam's first moment
   are judged against the EXISTING THREE-SLOT STEP on the triplets (u, p, n_sel), not against float64 directly: the bounds of
   that module's docstring are bounds between two fp32 evaluations, computed from the float64 restatement of the step on
   (u, p, n_sel) (R = 1: both sides add one negative), and the three-slot step itself is pinned to float64 and to the oracle by
   tests/test_gpu_storage_step.py and tests/test_gpu_parity.py.  Only Adam (table and both moments) is compared with float64 here.
   Rows that no touched row reaches have an exactly zero gradient: they keep their bits and their zero moments.
C  ties and edges, D determinism and composition, E off means off."""
import numpy as np
import pytest
import torch

import hard_neg_restatement as HN
import multineg_restatement as MN
import storage_cases as SC
import storage_restatement as S
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)
from test_gpu_multineg import _G, _judge_pair      # (_G: the judge reads the graph from its module's cache)
from test_gpu_storage_step import _forward_tables

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _sc_case(case):
    mode, d, K, R, M, reg, feat = case
    return (mode, d, K, 1, -1, reg) + ((feat,) if feat is not None and feat[0] == "drop" else ())


def _model(pkg, path, case, hard=True, batch=64, **cfg):
    """A fresh GPU model of a case (seed SC.MODEL_SEED, hand-set rows); hard = False: the plain three-slot model of the same
    configuration (what the selected triplets are stepped on)."""
    mode, d, K, R, M, reg, feat = case
    w = SC.configure(pkg, _sc_case(case), path, batch)
    if feat is not None and feat[0] == "w":
        w.config['layer_weights'] = feat[1]
    if hard:
        w.config.update({'neg_ratio': R, 'hard_neg': M, 'hard_neg_record': 1})
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
    m._state(max_batch=batch, need_ctx=True)
    return m


def _snapshot(m):
    st = m._dev
    return m._table.detach().clone(), st['adam_m'].clone(), st['adam_v'].clone(), m.adam_step


def _restore(m, snap):
    with torch.no_grad():
        m._table.copy_(snap[0]); m._dev['adam_m'].copy_(snap[1]); m._dev['adam_v'].copy_(snap[2])
    m.set_adam_step(snap[3])
    m.invalidate_cache()


def _step(m, batch):
    """One fused step with [B, R] candidates -> (loss_out, sel [B]) on the host."""
    out = m.fused_step(_dev(batch[0]), _dev(batch[1]), _dev(batch[2]))
    return out.cpu().numpy(), m.last_selection()[:len(batch[0])].cpu().numpy().astype(np.int64)


class _Full:
    """The hard-negative model as _judge_pair steps it: fused_step trains on the full [B, R] candidates whatever triplets the
    judge passes (those are the selected ones, for the other side); everything else is the model's own."""

    def __init__(self, m, batch):
        self._m, self._batch = m, batch

    def __getattr__(self, name):
        return getattr(self._m, name)

    def fused_step(self, u, p, n):
        return self._m.fused_step(_dev(self._batch[0]), _dev(self._batch[1]), _dev(self._batch[2]))


def _tables_read(pkg, m, case):
    """float64 X_0..X_K as the kernel of the NEXT step reads them (the public calls on the model's graph, from the table as it stands)."""
    E0 = m._table.detach().clone()
    _, fwd = _forward_tables(pkg, m, _sc_case(case), E0)
    return [E0.double().cpu().numpy()] + [fwd[k].float().double().cpu().numpy() for k in sorted(fwd)]


# ---- A + B ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HN.CASES, ids=HN.case_id)
def test_selection_is_valid_and_the_step_is_the_bpr_step_on_it(pkg, storage_graph, case):
    _selection_and_step(pkg, storage_graph, case)


@pytest.mark.parametrize("case", HN.LARGE_CASES, ids=HN.case_id)
def test_selection_and_step_beyond_one_wave_of_terms(pkg, storage_graph, case):
    """A and B on batches of 65 and 300 samples (HN.LARGE_CASES) in contexts of 300: reduce_loss_wave's second addition per lane,
    which no batch of HN.CASES reaches, on this step's scaled terms; the same assertions."""
    _selection_and_step(pkg, storage_graph, case, cap=max(MN.LARGE_BATCH_SIZES))


def _selection_and_step(pkg, storage_graph, case, cap=64):
    mode, d, K, R, M, reg, feat = case
    try:
        mN = _model(pkg, storage_graph, case, batch=cap)
        mO = _model(pkg, storage_graph, case, hard=False, batch=cap)
        assert mN._dev['dense_last'] and mO._dev['dense_last'] and mN.hard_neg == M
        assert pkg._lib.load().lgcn_ctx_get_hard_neg(mN._dev['ctx']) == M and pkg._lib.load().lgcn_ctx_get_hard_neg(mO._dev['ctx']) == 0
        w = None if mN.layer_weights is None else [float(v) for v in mN.layer_weights]
        keep = feat[1] if feat is not None and feat[0] == "drop" else 1.0
        wk = MN.layer_weights(K, w)
        bad, exact, total = [], 0, 0
        for i, batch in enumerate(HN.case_batches(case)):
            B, tag = len(batch[0]), f"{HN.case_id(case)} step {i + 1} B={len(batch[0])}"
            assert mN.adam_step == i
            snap = _snapshot(mN)
            tables = _tables_read(pkg, mN, case)
            assert len(tables) == K + 1
            out1, sel = _step(mN, batch)
            mN.check_device_errors()
            # ---- A
            bound, E = HN.score_bound(tables, wk, SC.N_USERS, batch, d)
            s64 = HN.scores(E, SC.N_USERS, batch)
            j = HN.ranks(HN.SEED, i, B, M)                                 # step: the counter before the step
            ref_sel, srt = HN.select(s64, j)
            assert ((sel >= 0) & (sel < R)).all()
            err = np.abs(s64[np.arange(B), sel] - srt[np.arange(B), j])
            print(f"[hard_neg] A {tag}: max |s[sel] - s_(j)| / (2 bound) = {float((err / (2 * bound + 1e-300)).max()):.3f}, "
                  f"sel == float64 choice on {int((sel == ref_sel).sum())} of {B}, tight share {HN.tight_share(srt, j, bound):.3f}")
            assert (err <= 2.0 * bound).all(), (tag, np.nonzero(err > 2.0 * bound)[0].tolist())
            exact += int((sel == ref_sel).sum()); total += B
            after1 = _snapshot(mN)
            # ---- B: the same step again from the same state (D: the same bits, sel included), judged against the three-slot step
            _restore(mN, snap)
            share = _judge_pair(pkg, _Full(mN, batch), mO, HN.selected_batch(batch, sel), 1, K, d, mode, reg, i + 1, "hard_neg " + tag,
                                w=w, keep=keep)
            bad += [(tag, k_, v) for k_, v in share.items() if not v <= 1.0]
            sel2 = mN.last_selection()[:B].cpu().numpy()
            assert np.array_equal(sel2, sel), (tag, "sel of the repeated step")
            for a, b in zip(after1[:3], _snapshot(mN)[:3]):
                assert torch.equal(a, b), (tag, "the repeated step is not bitwise the first")
            mN.check_device_errors(); mO.check_device_errors()
            assert not bool(mN._dev['G64'].any()) and mN.adam_step == mO.adam_step == i + 1
            if i == 0:      # rows with an exactly zero gradient (nothing touched reaches them) keep their bits; moments stay zero
                r = HN.step(_G["A"], SC.N_USERS, K, SC.DECAY, snap[0].cpu().numpy(), batch, sel, reg == "ego", w)
                if keep == 1.0:
                    still = ~SC.reach(_G["adj"], np.concatenate([batch[0], SC.N_USERS + batch[1], SC.N_USERS + HN.selected_batch(batch, sel)[2][:, 0]]), K)
                    assert not r["g_final"].numpy()[still].any()
                    idx = torch.from_numpy(np.nonzero(still)[0]).to(DEV)
                    assert torch.equal(mN._table[idx], snap[0][idx]) and not bool(mN._dev['adam_m'][idx].any()) and not bool(mN._dev['adam_v'][idx].any())
                    unsel = np.setdiff1d(SC.N_USERS + np.asarray(batch[2]).reshape(-1), np.nonzero(~still)[0])
                    print(f"[hard_neg] B {tag}: {int(still.sum())} rows outside the reach, {len(unsel)} of them unselected candidates")
        print(f"[hard_neg] {HN.case_id(case)}: the float64 choice on {exact} of {total} samples")
        assert exact >= (1.0 - HN.TIGHT_SHARE) * total - 1e-9
        assert not bad, ("beyond the bound (step, link, share of the bound)", bad)
    finally:
        pkg.world.configure([])


def test_unselected_candidates_get_nothing(pkg, storage_graph):
    """B = 1, K = 1, a user of degree 1 and R = 5 distinct candidates that the user does not hold: the unselected candidates have
    no touched neighbour, so their gradient is exactly zero -- rows bit for bit, both moments zero -- while the three touched rows move."""
    case = ("fp32", 64, 1, 5, 1, "propagated", None)
    try:
        m = _model(pkg, storage_graph, case)
        adj = _G["adj"]
        u = SC.N_USERS - 4
        held = set((adj.indices[adj.indptr[u]:adj.indptr[u + 1]] - SC.N_USERS).tolist())
        assert len(held) == 1
        cand = [i for i in (30, 31, 32, 34, 35, 36, 37) if i not in held][:5]
        batch = (np.array([u]), np.array([40]), np.array([cand]))
        first = m._table.detach().clone()
        out, sel = _step(m, batch)
        m.check_device_errors()
        assert sel.shape == (1,) and 0 <= sel[0] < 5 and np.isfinite(out).all()
        rows = SC.N_USERS + np.array(cand)
        others = torch.from_numpy(np.delete(rows, sel[0])).to(DEV)
        assert torch.equal(m._table[others], first[others])
        assert not bool(m._dev['adam_m'][others].any()) and not bool(m._dev['adam_v'][others].any())
        for row in (u, SC.N_USERS + 40, int(rows[sel[0]])):
            assert bool((m._table[row] != first[row]).any()) and bool(m._dev['adam_v'][row].any())
        assert not bool(m._dev['G64'].any()) and not bool(m._dev['bitmap'].any())
    finally:
        pkg.world.configure([])


# ---- C. ties and edges ------------------------------------------------------------------------------------------------------
def _edge_batch(E, R):
    """B = 8 samples of R candidates on the float64 output table E: sample 0 names ONE id R times; sample 1 has its user's best
    item at r = 1 and r = 3 and its worst items elsewhere; sample 2 has an out-of-range candidate; the rest are random."""
    rng = np.random.Generator(np.random.PCG64(4))
    B = 8
    u = rng.integers(20, SC.N_USERS - 10, B); p = rng.integers(20, SC.M_ITEMS - 10, B); n = rng.integers(20, SC.M_ITEMS - 10, (B, R))
    n[0, :] = 77
    s = E[SC.N_USERS:] @ E[u[1]]
    s[[SC.BIG_ITEM, SC.ISOLATED_ITEM]] = np.median(s)           # (never at either end: no slot names these two rows)
    order = np.argsort(s)
    n[1, :] = order[:R]                                           # the lowest scores ...
    if R >= 4:
        n[1, 1] = n[1, 3] = order[-1]                             # ... and the highest twice
    n[2, R - 1] = SC.M_ITEMS
    return u, p, n


@pytest.mark.parametrize("mode,d,R,M", [("fp32", 64, 5, 1), ("bf16", 32, 5, 2), ("fp32", 128, 5, 5), ("bf16", 256, 16, 16), ("fp32", 32, 2, 2), ("fp32", 64, 2, 1)])
def test_ties_and_edges(pkg, storage_graph, mode, d, R, M):
    """R copies of one id: sel = j_b under every M (ties rank by r).  The hardest item at r = 1 and r = 3, M = 1: sel = 1.  An
    out-of-range id: sel = -1, the error flag, zero terms -- the voiding of the multi-negative step.  M = R at R = 2."""
    case = (mode, d, 2, R, M, "propagated", None)
    try:
        m = _model(pkg, storage_graph, case)
        E = MN.propagate(_G["A"], torch.from_numpy(m._table.detach().cpu().numpy().astype(np.float64)), 2).numpy()
        batch = _edge_batch(E, R)
        B = len(batch[0])
        first = m._table.detach().clone()
        out, sel = _step(m, batch)
        j = HN.ranks(HN.SEED, 0, B, M)
        assert sel[0] == j[0], (sel, j)
        if R >= 4 and M == 1:
            assert sel[1] == 1
        assert sel[2] == -1
        terms = m._dev['terms'].cpu().numpy()
        assert terms[2] == 0.0 and terms[B + 2] == 0.0 and (terms[:B][np.arange(B) != 2] != 0.0).all()
        with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
            m.check_device_errors()
        assert np.isfinite(out).all() and not bool(m._dev['G64'].any()) and m.adam_step == 1
        assert ((sel[np.arange(B) != 2] >= 0) & (sel[np.arange(B) != 2] < R)).all()
        assert float((m._table - first).abs().max()) > 1e-4                 # (it trained)
        if mode == "fp32":      # the voided sample contributes nothing: the loss is that of the batch without it, normalised by the same B
            r = HN.step(_G["A"], SC.N_USERS, 2, SC.DECAY, first.cpu().numpy(), tuple(np.delete(t, 2, axis=0) for t in batch), np.delete(sel, 2), B_norm=B)
            assert abs(out[1] - float(r["loss_out"][1])) < 3e-6 and abs(out[2] - float(r["loss_out"][2])) < 3e-6      # (the project's yardstick against float64)
    finally:
        pkg.world.configure([])


# ---- D. determinism and composition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,K,reg,M", [("fp32", 1, "ego", 2), ("bf16", 2, "propagated", 1)])
def test_epoch_equals_the_loop_of_steps_bitwise(pkg, storage_graph, mode, K, reg, M):
    """lgcn_train_epoch_multi over T = 165 (batches of 64, 64, 37: a ragged last one) against the loop of lgcn_train_step_multi
    under hard negatives: loss rows, table, both moments and the last batch's sel bit for bit."""
    try:
        R, B, T, d = 5, 64, 165, 64
        case = (mode, d, K, R, M, reg, None)
        seq = MN.make_batches(d, K, R)[:3]
        u = np.concatenate([b[0] for b in seq]); p = np.concatenate([b[1] for b in seq]); n = np.concatenate([b[2] for b in seq])
        a = _model(pkg, storage_graph, case)
        want = a.fused_epoch(_dev(u), _dev(p), _dev(np.ascontiguousarray(n.T)), B)
        a.check_device_errors()
        b = _model(pkg, storage_graph, case)
        first = b._table.detach().clone()
        got = [b.fused_step(_dev(u[t:t + B]), _dev(p[t:t + B]), _dev(n[t:t + B])) for t in range(0, T, B)]
        b.check_device_errors()
        assert a.adam_step == b.adam_step == 3 and want.shape == (3, 3)
        assert torch.equal(torch.stack(got), want), (torch.stack(got), want)
        assert torch.equal(a._table, b._table) and torch.equal(a._dev['adam_m'], b._dev['adam_m']) and torch.equal(a._dev['adam_v'], b._dev['adam_v'])
        assert torch.equal(a.last_selection()[:37], b.last_selection()[:37])
        assert not bool(a._dev['G64'].any()) and float((b._table - first).abs().max()) > 1e-4
        assert int(pkg._lib.load().lgcn_ctx_folded_steps(a._dev['ctx'])) == 0      # never folded
    finally:
        pkg.world.configure([])


def test_seeds_move_the_selection_only_where_there_is_a_choice(pkg, storage_graph):
    """M = 3 of R = 5: another --seed gives another sel, in exactly the samples whose pick j_b the host hash moves (the scores are
    the same bits and distinct ranks are distinct candidates); M = 1: the same sel whatever the seed."""
    try:
        batch = MN.make_batches(64, 2, 5)[0]
        sels = {}
        for M in (3, 1):
            for seed in (2020, 2021):
                m = _model(pkg, storage_graph, ("fp32", 64, 2, 5, M, "propagated", None), seed=seed)
                sels[M, seed] = _step(m, batch)[1]
                m.check_device_errors()
        assert np.array_equal(sels[1, 2020], sels[1, 2021])
        moved = HN.ranks(2020, 0, 64, 3) != HN.ranks(2021, 0, 64, 3)
        assert moved.any() and np.array_equal(sels[3, 2020] != sels[3, 2021], moved)
    finally:
        pkg.world.configure([])


# ---- E. off means off, and the refusals on a context ------------------------------------------------------------------------
def test_off_restores_the_multi_negative_step_and_refusals_leave_everything_untouched(pkg, storage_graph):
    try:
        L = pkg._lib
        lib = L.load()
        R, B, d, K = 5, 64, 64, 2
        batch = MN.make_batches(d, K, R)[0]
        case = ("fp32", d, K, R, 2, "propagated", None)
        plain = _model(pkg, storage_graph, case, hard=False, neg_ratio=R)
        want = plain.fused_step(_dev(batch[0]), _dev(batch[1]), _dev(batch[2]))
        m = _model(pkg, storage_graph, case)
        ctx, s = m._dev['ctx'], L.current_stream()
        u, p, n = _dev(batch[0]), _dev(batch[1]), _dev(np.ascontiguousarray(batch[2].T))
        loss = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
        st = m._dev
        before = (m._table.detach().clone(), st['adam_m'].clone(), st['adam_v'].clone(), st['G64'].clone(), st['terms'].clone())

        def refused(rc, *words):
            msg = lib.lgcn_last_error().decode()
            assert rc == 3 and all(wd in msg for wd in words), (rc, msg)

        # R < 2, M > R (a context set to M = 5 stepping R = 4), and every entry point that is not the multi-negative one
        refused(lib.lgcn_train_step_multi(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, B, L.tp(loss), s), "hard negatives", "M = 2", "R = 1")
        refused(lib.lgcn_train_epoch_multi(ctx, L.tp(u), L.tp(p), L.tp(n), 1, B, B, L.tp(loss), s), "hard negatives", "M = 2", "R = 1")
        L.check(lib.lgcn_ctx_set_hard_neg(ctx, 5, 2020, None), "set")
        refused(lib.lgcn_train_step_multi(ctx, L.tp(u), L.tp(p), L.tp(n), B, 4, B, L.tp(loss), s), "hard negatives", "M = 5", "R = 4")
        refused(lib.lgcn_train_step(ctx, L.tp(u), L.tp(p), L.tp(n), B, L.tp(loss), s), "lgcn_train_step", "hard negatives")
        refused(lib.lgcn_train_epoch(ctx, L.tp(u), L.tp(p), L.tp(n), B, B, L.tp(loss), s), "lgcn_train_epoch", "hard negatives")
        refused(lib.lgcn_train_step_inbatch(ctx, L.tp(u), L.tp(p), B, L.tp(loss), s), "lgcn_train_step_inbatch", "hard negatives")
        refused(lib.lgcn_train_step_inbatch_mix(ctx, L.tp(u), L.tp(p), L.tp(n), B, R, B, L.tp(loss), s), "lgcn_train_step_inbatch_mix", "hard negatives")
        refused(lib.lgcn_train_step_dp_part1(ctx, L.tp(u), L.tp(p), L.tp(n), B, 1, 0, s), "lgcn_train_step_dp_part1", "hard negatives")
        refused(lib.lgcn_train_step_cols_part1(ctx, L.tp(u), L.tp(p), L.tp(n), B, None, s), "lgcn_train_step_cols_part1", "hard negatives")
        refused(lib.lgcn_ctx_set_loss(ctx, L.LOSS_SOFTMAX, 0.5), "lgcn_ctx_set_loss", "hard negatives")
        refused(lib.lgcn_ctx_set_hard_neg(ctx, 17, 2020, None), "hard negatives", "17")
        refused(lib.lgcn_ctx_set_hard_neg(ctx, -1, 2020, None), "hard negatives")
        assert lib.lgcn_ctx_get_hard_neg(ctx) == 5 and lib.lgcn_ctx_get_loss(ctx, None) == L.LOSS_BPR
        torch.cuda.synchronize()
        for a, b in zip(before, (m._table, st['adam_m'], st['adam_v'], st['G64'], st['terms'])):
            assert torch.equal(a, b)
        assert bool((loss == -7.0).all()) and m.adam_step == 0
        m.check_device_errors()
        # off: the same context runs the multi-negative step of a context that was never told, bit for bit
        L.check(lib.lgcn_ctx_set_hard_neg(ctx, 0, 0, None), "off")
        assert lib.lgcn_ctx_get_hard_neg(ctx) == 0
        got = m._fused_call("lgcn_train_step_multi", (L.tp(u), L.tp(p), L.tp(n), B, R, B), B)
        assert torch.equal(got, want) and torch.equal(m._table, plain._table) and torch.equal(st['adam_m'], plain._dev['adam_m'])
        assert bool((m.last_selection() == -1).all())                      # nothing was ever recorded
        # the contexts that cannot take it say so and stay as they were
        L.check(lib.lgcn_ctx_set_loss(ctx, L.LOSS_SOFTMAX, 0.5), "softmax")
        refused(lib.lgcn_ctx_set_hard_neg(ctx, 2, 2020, None), "hard negatives", "loss")
        for mode, dl, cfg, word in (("fp8", 1, {}, "FP8"), ("fp32", 0, {}, "dense_last"), ("fp32", 1, {'use_pop_gate': True}, "optional")):
            w = SC.configure(pkg, (mode, 64, 2, dl, -1, "propagated"), storage_graph)
            w.config.update(cfg)
            ds = pkg.dataloader.Loader(w.config, path=storage_graph)
            o = pkg.model.LightGCN(w.config, ds).to(DEV)
            octx = o._state(max_batch=64, need_ctx=True)['ctx']
            refused(lib.lgcn_ctx_set_hard_neg(octx, 2, 2020, None), "hard negatives", word)
            assert lib.lgcn_ctx_get_hard_neg(octx) == 0
    finally:
        pkg.world.configure([])


def test_training_epoch_through_procedure(pkg, storage_graph, tmp_path):
    """world.config['hard_neg'] = 2 with neg_ratio 4, one Procedure.BPR_train_original epoch: the sampler, the shuffle and
    lgcn_train_epoch_multi as they were; the loss is finite, the steps were counted and a selection was recorded."""
    import os
    try:
        case = ("fp32", 64, 2, 4, 2, "propagated", None)
        m = _model(pkg, storage_graph, case, batch=256, prefetch_epoch=0, sampler='cpp', checkpoint_dir=os.path.join(str(tmp_path), "ckpt"))
        pkg.world.tensorboard = 0
        ds = m.dataset
        pkg.sampling.seed(31); pkg.utils.set_seed(32)
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        info = pkg.Procedure.BPR_train_original(ds, m, bpr, 1)
        m.check_device_errors()
        assert info.startswith("loss") and m.adam_step >= ds.trainDataSize // ds.n_users * ds.n_users // 256
        sel = m.last_selection().cpu().numpy()
        assert ((sel >= -1) & (sel < 4)).all() and (sel >= 0).any()
    finally:
        pkg.world.configure([])

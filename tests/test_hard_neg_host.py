"""Hard negatives, DNS(M, N) (--hard_neg M) without a device: the exported hash against its two Python restatements,
the float64 restatement (tests/hard_neg_restatement.py) against torch autograd of LightGCN.bpr_loss, the flag, the refusals that
need no device, the C ABI, and the condition under which the GPU fixtures can tell a right selection from a wrong one."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hard_neg_restatement as HN                # noqa: E402
import multineg_restatement as MN                # noqa: E402
import storage_cases as SC                       # noqa: E402
import storage_restatement as S                  # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import REPO                        # noqa: E402

_CACHE = {}


def _inputs(pkg, path, d):
    """(adjacency CSR, dense float64 A, initial fp32 table with the hand-set rows) for an embedding width"""
    try:
        if ("tab", d) not in _CACHE:
            ds, m = SC.make_model(pkg, ("bf16", d, 1, 1, -1, "propagated"), path)
            if "adj" not in _CACHE:
                adj = ds.getSparseGraphCSR()
                _CACHE["adj"], _CACHE["A"] = adj, S.dense_adj(adj)
            _CACHE[("tab", d)] = m._table.detach().numpy().copy()
        return _CACHE["adj"], _CACHE["A"], _CACHE[("tab", d)]
    finally:
        pkg.world.configure([])


# ---- 1. the hash ------------------------------------------------------------------------------------------------------------
def test_exported_hash_is_the_python_restatement(pkg):
    """lgcn_hard_neg_rank (the function the kernel calls) == model.hard_neg_rank (NumPy uint64, what bpr_loss uses) == the Python
    integers of tests/hard_neg_restatement.py on 10 000 (seed, step, b, M) tuples with the edges in: M = 1 (always 0), M = 16,
    step 0, b = 2^31 - 1, seeds and steps at the ends of their ranges."""
    lib = pkg._lib.load()
    rng = np.random.Generator(np.random.PCG64(25))
    tuples = [(2020, 0, 0, 1), (2020, 0, 0, 16), (2020, 0, 2 ** 31 - 1, 4), (0, 0, 0, 2), (2 ** 64 - 1, 2 ** 62, 2 ** 31 - 1, 16),
              (2 ** 63, 1, 1, 3), (1, 0, 5, 1)]
    while len(tuples) < 10000:
        tuples.append((int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 31)),
                       int(rng.integers(1, 17))))
    for seed, step, b, M in tuples:
        got = int(lib.lgcn_hard_neg_rank(seed, step, b, M))
        assert got == HN.rank(seed, step, b, M) == int(pkg.model.hard_neg_rank(seed, step, [b], M)[0]), (seed, step, b, M)
        assert 0 <= got < M and (M > 1 or got == 0)
    # the vectorised form, and M <= 1
    assert np.array_equal(pkg.model.hard_neg_rank(2020, 3, np.arange(500), 5), HN.ranks(2020, 3, 500, 5))
    assert lib.lgcn_hard_neg_rank(7, 7, 7, 0) == 0 and not pkg.model.hard_neg_rank(7, 7, np.arange(9), 1).any()


def test_hash_is_uniform_and_keyed(pkg):
    """Over b = 0..99 999 at M = 4 each value occurs within 1 % of a quarter; another step or seed gives another stream; the
    dropout key of the same (seed, step) is not the stream's key (the domain constant)."""
    j = pkg.model.hard_neg_rank(2020, 0, np.arange(100000), 4)
    counts = np.bincount(j, minlength=4)
    assert counts.sum() == 100000 and (np.abs(counts / 100000.0 - 0.25) <= 0.01 * 0.25).all(), counts
    for other in (pkg.model.hard_neg_rank(2020, 1, np.arange(100000), 4), pkg.model.hard_neg_rank(2021, 0, np.arange(100000), 4)):
        assert 0.70 < float((other != j).mean()) < 0.80          # independent picks among 4 differ 3 times in 4
    k = HN.splitmix64((HN.splitmix64(2020) + 0) & HN.MASK)       # make_drop's key of (seed 2020, step 0)
    undomained = np.array([(HN.splitmix64((k + b) & HN.MASK) >> 32) % 4 for b in range(2000)])
    assert 0.70 < float((undomained != j[:2000]).mean()) < 0.80


# ---- 2. the restatement is the autograd of LightGCN.bpr_loss ----------------------------------------------------------------
def _model_with(pkg, path, cls="LightGCN", d=32, K=2, **cfg):
    w = SC.configure(pkg, ("fp32", d, K, 1, -1, "propagated"), path)
    w.config.update(cfg)
    ds = pkg.dataloader.Loader(w.config, path=path)
    return ds, getattr(pkg.model, cls)(w.config, ds)


@pytest.mark.parametrize("d,K,R,M,step", [(32, 1, 2, 1, 0), (32, 2, 5, 2, 3), (64, 3, 16, 16, 1), (64, 2, 5, 5, 0), (32, 3, 16, 1, 7)])
def test_restatement_is_the_autograd_of_bpr_loss(pkg, storage_graph, d, K, R, M, step):
    """propagate, select, then multineg_restatement.step on the R = 1 batch of the selected triplets, against torch float64
    autograd of LightGCN.bpr_loss with [B, R] negatives and hard_neg = M (the propagation needs the device, so a float64
    computer() over the same dense A_hat is injected: everything after it is the model's own code): the selection equal, the
    loss triple at 1e-13 and the gradient at 1e-12 of its scale -- the bounds of tests/test_multineg_host.py."""
    try:
        _, A, table = _inputs(pkg, storage_graph, d)
        ds, m = _model_with(pkg, storage_graph, d=d, K=K, neg_ratio=R, hard_neg=M)
        assert m.hard_neg == M
        m.hard_neg_step = step
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
        for batch in MN.make_batches(d, K, R):
            B = len(batch[0])
            E0 = torch.from_numpy(table.astype(np.float64)).requires_grad_(True)
            E = MN.propagate(A, E0, K)
            m.computer = lambda: (E[:SC.N_USERS], E[SC.N_USERS:])
            j = HN.ranks(HN.SEED, step, B, M)
            sel, _ = HN.select(HN.scores(E.detach(), SC.N_USERS, batch), j)
            got_sel = m.hard_neg_select(t(batch[0]), t(batch[2])).numpy()
            assert np.array_equal(got_sel, sel)
            bpr, reg = m.bpr_loss(t(batch[0]), t(batch[1]), t(batch[2]))
            bpr_t, reg_t = m.bpr_loss(t(batch[0]), t(batch[1]), t(batch[2]).t().contiguous()) if B != R else (bpr, reg)      # the [R, B] layout
            assert float(bpr_t.detach()) == float(bpr.detach()) and float(reg_t.detach()) == float(reg.detach())
            loss = bpr + SC.DECAY * reg
            loss.backward()
            r = HN.step(A, SC.N_USERS, K, SC.DECAY, table, batch, sel)
            for got, ref in zip(r["loss_out"], (loss.detach(), bpr.detach(), reg.detach())):
                assert abs(float(got) - float(ref)) <= 1e-13 * max(1.0, abs(float(ref)))
            scale = float(E0.grad.abs().max())
            assert float((r["g_final"] - E0.grad).abs().max()) <= 1e-12 * scale
            # three rows per sample, each slot of weight 1: nothing of an unselected candidate
            assert float(r["cnt"].sum()) == 3 * B and r["e_n"].shape == (B, 1, d)
            unsel = np.setdiff1d(SC.N_USERS + np.asarray(batch[2]).reshape(-1),
                                 np.concatenate([batch[0], SC.N_USERS + batch[1], SC.N_USERS + HN.selected_batch(batch, sel)[2][:, 0]]))
            assert not r["G"][unsel].any()
    finally:
        pkg.world.configure([])


def test_selection_rule_on_ties(pkg, storage_graph):
    """model.hard_neg_select on injected tables whose scores are known exactly (users = the first unit vector, an item's first
    column = its score): equal scores rank by r ascending, so R copies of one id rank 0..R-1 and the selection is j_b itself;
    two equal maxima are ranks 0 and 1 in the order of r; over 8 step counters every rank of M = 4 is picked somewhere."""
    try:
        _, m = _model_with(pkg, storage_graph, neg_ratio=4, hard_neg=4)
        U = torch.zeros(SC.N_USERS, 32, dtype=torch.float64); U[:, 0] = 1.0
        I = torch.zeros(SC.M_ITEMS, 32, dtype=torch.float64)
        I[:, 0] = torch.tensor([0.5, 0.1, 0.9, 0.3, 0.2] + [0.0] * (SC.M_ITEMS - 5), dtype=torch.float64)
        m.computer = lambda: (U, I)
        neg = torch.tensor([[0, 0, 0, 0], [1, 2, 3, 2], [4, 1, 4, 3]])          # scores .5 .5 .5 .5 | .1 .9 .3 .9 | .2 .1 .2 .3
        users = torch.tensor([3, 4, 5])
        by_rank = [[0, 1, 2, 3], [1, 3, 2, 0], [3, 0, 2, 1]]                     # the candidate of rank 0, 1, 2, 3 of each sample
        seen = set()
        for step in range(8):
            m.hard_neg_step = step
            j = HN.ranks(HN.SEED, step, 3, 4)
            sel = m.hard_neg_select(users, neg).tolist()
            assert sel == [by_rank[b][j[b]] for b in range(3)], (step, j, sel)
            assert sel[0] == j[0]
            ref, srt = HN.select(I[neg, 0].numpy(), j)
            assert ref.tolist() == sel and (np.diff(srt, axis=1) <= 0).all()
            seen |= set(j.tolist())
        assert seen == {0, 1, 2, 3}
    finally:
        pkg.world.configure([])


# ---- 3. the flag, the refusals, the C ABI -----------------------------------------------------------------------------------
NEW_SYMBOLS = ("lgcn_ctx_set_hard_neg", "lgcn_ctx_get_hard_neg", "lgcn_hard_neg_rank")


def test_new_symbols_are_declared_bound_and_exported_with_abi_13(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "lgcn_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lgcn_[a-z0-9_]+)\s*\(", hdr))
    lib = pkg._lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lgcn_abi_version() == pkg._lib.ABI_VERSION == 13
    assert "lgcn_hardneg.hip" in [os.path.basename(s) for s in pkg.build.SOURCES]


def test_null_context_return_codes(pkg):
    lib = pkg._lib.load()
    assert lib.lgcn_ctx_set_hard_neg(None, 2, 2020, None) == 3 and b"lgcn_ctx_set_hard_neg" in lib.lgcn_last_error()
    assert lib.lgcn_ctx_set_hard_neg(None, 0, 0, None) == 3
    assert lib.lgcn_ctx_get_hard_neg(None) == -1
    assert lib.lgcn_hard_neg_rank(2020, 0, 0, 1) == 0


def test_hard_neg_flag(pkg):
    w = pkg.world
    try:
        w.configure([])
        assert w.config['hard_neg'] == 0
        w.configure(['--hard_neg', '2', '--neg_ratio', '8'])
        assert w.config['hard_neg'] == 2 and w.config['neg_ratio'] == 8
        with pytest.raises(SystemExit):
            w.configure(['--hard_neg', 'hardest'])
    finally:
        w.configure([])


def test_refusals_that_need_no_device_name_the_flag(pkg, storage_graph):
    try:
        refused = ({'neg_ratio': 1}, {'neg_ratio': 4, 'hard_neg': 5}, {'neg_ratio': 4, 'loss': 'softmax'}, {'neg_ratio': 1, 'loss': 'inbatch'},
                   {'neg_ratio': 4, 'act_dtype': 'fp8', 'latent_dim_rec': 64}, {'neg_ratio': 4, 'use_pop_gate': True},
                   {'neg_ratio': 4, 'use_item_item': True})
        for cfg in refused:
            with pytest.raises(pkg._lib.LgcnError, match="--hard_neg"):
                _model_with(pkg, storage_graph, **{'hard_neg': 2, **cfg})
        for bad in (-1, 17, 'two'):
            with pytest.raises(ValueError, match="--hard_neg"):
                _model_with(pkg, storage_graph, neg_ratio=4, hard_neg=bad)
        with pytest.raises(pkg._lib.LgcnError, match="--hard_neg"):
            _model_with(pkg, storage_graph, cls="PureMF", hard_neg=1, neg_ratio=2)
        ds, m = _model_with(pkg, storage_graph, neg_ratio=4, hard_neg=2)
        assert m.hard_neg == 2 and m.neg_ratio == 4
        with pytest.raises(RuntimeError, match="--hard_neg"):
            pkg.parallel.DataParallelBPR(m, pkg.world.config)
        with pytest.raises(pkg._lib.LgcnError, match="last_selection"):
            m.last_selection()
        with pytest.raises(ValueError, match="--hard_neg"):       # fewer candidates in the batch than M
            m.hard_neg_select(torch.zeros(3, dtype=torch.int64), torch.zeros(3, 1, dtype=torch.int64))
    finally:
        pkg.world.configure([])


def test_hard_neg_zero_builds_what_was_built_before(pkg, storage_graph):
    """--hard_neg 0, and no key at all: no setter in the context's list, the same refusal order, the multi-negative loss."""
    try:
        for cfg in ({'hard_neg': 0}, {}):
            ds, m = _model_with(pkg, storage_graph, neg_ratio=5, **cfg)
            if not cfg:
                m.config.pop('hard_neg')
                m = pkg.model.LightGCN(m.config, ds)
            assert m.hard_neg == 0
            assert [e for e, _ in m._ctx_setters({}, 0)] == ['lgcn_ctx_set_step']
            with pytest.raises(pkg._lib.LgcnError, match="--neg_ratio"):       # the parent's message, not a --hard_neg one
                _model_with(pkg, storage_graph, neg_ratio=5, act_dtype='fp8', latent_dim_rec=64, **cfg)
        _, on = _model_with(pkg, storage_graph, neg_ratio=5, hard_neg=2, seed=77)
        setters = dict(on._ctx_setters({}, 0))
        assert setters['lgcn_ctx_set_hard_neg'] == (2, 77, None)
        # the autograd path with the flag off is the multi-negative loss, untouched
        _, A, table = _inputs(pkg, storage_graph, 32)
        _, off = _model_with(pkg, storage_graph, neg_ratio=5)
        E = MN.propagate(A, torch.from_numpy(table.astype(np.float64)), 2)
        off.computer = lambda: (E[:SC.N_USERS], E[SC.N_USERS:])
        u, p, n = MN.make_batches(32, 2, 5)[0]
        t = lambda a: torch.from_numpy(np.asarray(a, np.int64))
        bpr, _ = off.bpr_loss(t(u), t(p), t(n))
        assert abs(float(bpr) - float(MN.loss(E, E, SC.N_USERS, (u, p, n), SC.DECAY)[1])) <= 1e-13
    finally:
        pkg.world.configure([])


# ---- 4. the GPU fixtures can discriminate -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", HN.CASES + HN.LARGE_CASES, ids=HN.case_id)
def test_the_reference_alone_discriminates(pkg, storage_graph, case):
    """For every fixture of tests/test_gpu_hard_neg.py, from the float64 table alone (the case's initial table, float64 layers, no
    storage rounding): over the case's samples at most 5 % have a gap below 2 bound_b between the picked order statistic and a
    neighbouring one -- elsewhere the bound of test A forces the exact choice, so A can fail.  (The batches carry one deliberate
    exact tie per batch, the same item twice among a sample's candidates.)  A seed in HN.BATCH_SEED is above 0 only where the
    lower seeds fail this."""
    mode, d, K, R, M, reg, feat = case
    _, A, table = _inputs(pkg, storage_graph, d)
    wk = MN.layer_weights(K, None if feat is None or feat[0] != "w" else [float(v) for v in _exp_weights(pkg, K)])
    tables = HN.float64_tables(A, table, K)

    def share(seed):
        tight, total = 0.0, 0
        for step, batch in enumerate(HN.case_batches(case, seed)):
            B = len(batch[0])
            bound, E = HN.score_bound(tables, wk, SC.N_USERS, batch, d)
            _, srt = HN.select(HN.scores(E, SC.N_USERS, batch), HN.ranks(HN.SEED, step, B, M))
            tight += HN.tight_share(srt, HN.ranks(HN.SEED, step, B, M), bound) * B
            total += B
        return tight / total

    seed = HN.BATCH_SEED.get(HN.case_id(case), 0)
    print(f"[hard_neg] {HN.case_id(case)}: seed {seed}, share of samples within 2 bound of a neighbour {share(seed):.4f}")
    assert share(seed) <= HN.TIGHT_SHARE, (seed, share(seed))
    for lower in range(seed):
        assert share(lower) > HN.TIGHT_SHARE, ("a lower seed meets the condition", lower)


def _exp_weights(pkg, K):
    """--layer_weights exp at --layer K as the model resolves it."""
    cfg = dict(pkg.world.config)
    cfg['layer_weights'] = 'exp'
    return pkg.model.resolve_layer_weights(cfg, K)

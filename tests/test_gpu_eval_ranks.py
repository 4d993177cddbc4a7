"""Rank-based fused evaluation on the GPU (lgcn_eval_ranks / lgcn_eval_rank_metrics): exact agreement on integer tables where
every product and sum is exact in fp32 and in the split bf16 product; rounding-aware interval bounds on Gaussian tables against
fp64; a catalogue large enough for a multi-part sweep; Procedure.Test with --rank_metrics 1 on the LastFM fixture; and the
refusals, which must leave pre-filled outputs untouched.  The metric restatement is the one of test_eval_ranks_host."""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import EPS32
from test_eval_ranks_host import restate

DEV = "cuda:0"
gpu = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _csr(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate(rows).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, idx


def _lists(rng, m_items, n_users, users, lens, full_slot=None):
    """Train positives clustered inside a tile, at ids 31/32/33 and at m - 1 (some users none); per slot a test list of the
    given length drawn from the user's other items, every fifth slot with one train positive added to it."""
    ntiles = (m_items + 31) // 32
    train = []
    for u in range(n_users):
        c = set(rng.integers(0, m_items, int(rng.integers(0, 25))).tolist())
        t0 = int(rng.integers(0, ntiles - 1)) * 32
        c |= set(range(t0 + 3, min(m_items, t0 + 3 + int(rng.integers(5, 29)))))          # inside one tile
        if u % 2:
            c |= {31, 32, 33}
        if u % 3 == 0:
            c |= {m_items - 1}
        if u % 11 == 0:
            c = set()
        train.append(np.array(sorted(c), np.int32))
    test = []
    for s, u in enumerate(users.tolist()):
        free = np.setdiff1d(np.arange(m_items, dtype=np.int32), train[u])
        n = len(free) if s == full_slot else min(lens[s % len(lens)], len(free))
        t = rng.choice(free, n, replace=False) if n < len(free) else free
        if s % 5 == 0 and n and len(train[u]) and s != full_slot:
            t = np.union1d(t, train[u][len(train[u]) // 2:][:1])                           # a test item that is a train positive
        test.append(np.sort(t).astype(np.int32))
    return train, test


class Problem:
    def __init__(self, E, n_users, users, train, test):
        self.E, self.n_users, self.users, self.train, self.test = E, n_users, users, train, test
        self.m_items, self.d = E.shape[0] - n_users, E.shape[1]
        self.train_ptr, self.train_idx = _csr(train)
        self.test_ptr, self.test_idx = _csr(test)
        self.pnt = np.array([len(np.setdiff1d(train[u], test[s])) for s, u in enumerate(users.tolist())], np.int64)

    def device(self):
        idx = self.train_idx if len(self.train_idx) else np.zeros(1, np.int32)
        return (_dev(self.E), _dev(self.users), _dev(self.train_ptr), _dev(idx), _dev(self.test_ptr), _dev(self.test_idx))

    def rows64(self):
        """The reference's rows in float64, -1024 at the train positives: [n_eval, m_items]."""
        S = self.E[:self.n_users][self.users].astype(np.float64) @ self.E[self.n_users:].astype(np.float64).T
        for s, u in enumerate(self.users.tolist()):
            S[s, self.train[u]] = -1024.0
        return S

    def candidates(self, s):
        cand = np.ones(self.m_items, bool)
        cand[self.train[self.users[s]]] = False
        cand[self.test[s]] = False
        return cand


def _run(pkg, prob, dev, fp32=False):
    L = pkg._lib
    Ed, ud, tp_, ti, sp, si = dev
    score, gt, eq = L.eval_ranks(Ed, prob.n_users, ud, tp_, ti, sp, si, fp32=fp32)
    torch.cuda.synchronize()
    return score, gt, eq


# ---------------------------------------------------------------------------------------------------------------------------
# 1. exact
EXACT = [(300, 32), (3001, 64), (10007, 128), (3001, 256)]
EXACT_LENS = [0, 1, 2, 63, 64, 65, 200, 200]


@functools.lru_cache(maxsize=None)
def _exact_problem(m_items, d):
    """Integer tables in {-3..3}: every dot product is an integer below 2^24 -- exact whatever the order or the number format.
    Returns the problem and its int64 reference (score, gt, eq), computed once."""
    rng = np.random.Generator(np.random.PCG64(1000 * d + m_items))
    n_users, n_eval = 120, 257
    E = rng.integers(-3, 4, (n_users + m_items, d)).astype(np.float32)
    E[5] = 0.0                                                       # a user whose row is zero: every score ties at 0
    users = rng.integers(0, n_users, n_eval).astype(np.int32)        # unsorted, repeating
    users[:4] = [5, 7, 5, 0]
    train, test = _lists(rng, m_items, n_users, users, EXACT_LENS, full_slot=7)     # slot 7: every non-train item
    prob = Problem(E, n_users, users, train, test)
    S = prob.rows64().astype(np.int64)
    score, gt, eq = [], [], []
    for s in range(n_eval):
        c = np.sort(S[s, prob.candidates(s)])
        st = S[s, test[s]]
        hi, lo = np.searchsorted(c, st, 'right'), np.searchsorted(c, st, 'left')
        score.append(st); gt.append(len(c) - hi); eq.append(hi - lo)
    return prob, np.concatenate(score), np.concatenate(gt), np.concatenate(eq)


@gpu
@pytest.mark.parametrize("m_items,d", EXACT)
def test_ranks_exact(pkg, m_items, d):
    prob, score, gt, eq = _exact_problem(m_items, d)
    lens = np.diff(prob.test_ptr)
    assert {0, 1, 2, 63, 64, 65, 200} <= set(lens.tolist()) | set((lens - 1).tolist()) and lens.max() >= min(m_items - 80, 9000)
    dev = prob.device()
    first = None
    for fp32 in (False, True):
        for rep in range(2):
            got = [t.cpu().numpy() for t in _run(pkg, prob, dev, fp32=fp32)]
            assert np.array_equal(got[0].astype(np.int64), score)
            assert np.array_equal(got[1].astype(np.int64), gt)
            assert np.array_equal(got[2].astype(np.int64), eq)
            if first is None:
                first = got
            assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(first, got))       # bitwise, run to run


@gpu
@pytest.mark.parametrize("m_items,d", EXACT)
def test_rank_metrics_equal_the_restatement(pkg, m_items, d):
    prob, score, gt, eq = _exact_problem(m_items, d)
    L = pkg._lib
    Ed, ud, tp_, ti, sp, si = prob.device()
    ks = [20, 1, m_items, 64, 300]
    per_user, sums = L.eval_rank_metrics(m_items, ud, tp_, ti, sp, si, _dev(score.astype(np.float32)), _dev(gt.astype(np.int32)),
                                         _dev(eq.astype(np.int32)), ks)
    per_user, sums = per_user.cpu().numpy(), sums.cpu().numpy()
    nk = len(ks)
    assert per_user.shape == (len(prob.users), 3 * nk + 2)
    for s in range(len(prob.users)):
        b, e = prob.test_ptr[s], prob.test_ptr[s + 1]
        r = restate(score[b:e], gt[b:e], eq[b:e], prob.pnt[s], m_items, ks)
        want = np.concatenate([r['precision'], r['recall'], r['ndcg'], [r['auc'], r['mrr']]])
        np.testing.assert_allclose(per_user[s], want, rtol=0, atol=1e-12, err_msg=f"slot {s} (n = {e - b})")
    np.testing.assert_allclose(sums, per_user.sum(0), rtol=0, atol=1e-9)
    _, sums2 = L.eval_rank_metrics(m_items, ud, tp_, ti, sp, si, _dev(score.astype(np.float32)), _dev(gt.astype(np.int32)),
                                   _dev(eq.astype(np.int32)), ks)
    assert np.array_equal(sums2.cpu().numpy(), sums)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. rounding-aware.  b = 2 sqrt(d) 2^-24 |u| max|i| bounds the distance of any fp32 evaluation of a score from its exact
# value (the bound of the top-K tests), so two fp32 scores can compare differently from their fp64 values only when those lie
# within 2 b: with fp64 scores S, any correct count satisfies  #{S_j > S_t + 2b} <= gt  and  gt + eq <= #{S_j >= S_t - 2b}.
ROUNDING = [(3001, 32), (10007, 64), (10007, 128), (3001, 256)]
ROUND_LENS = [0, 1, 2, 5, 20, 63, 64, 65, 100, 200, 9, 33]
KS = [20, 300, 1000]


class Bounds:
    """Per test entry: lo <= gt, gt + eq <= hi; positions in [pos_lo, pos_hi]; the fp64 metrics."""

    def __init__(self, prob):
        S = prob.rows64()
        E64 = prob.E.astype(np.float64)
        inorm = np.linalg.norm(E64[prob.n_users:], axis=1).max()
        lo, hi, plo, phi, flip = [], [], [], [], []
        self.auc64, self.recall64, self.inv_n = [], [], []
        for s, u in enumerate(prob.users.tolist()):
            t = prob.test[s]
            n = len(t)
            b2 = 2.0 * (2.0 * np.sqrt(prob.d) * EPS32 * np.linalg.norm(E64[u]) * inorm)
            c = np.sort(S[s, prob.candidates(s)])
            st = S[s, t]
            l = len(c) - np.searchsorted(c, st + b2, 'right')
            h = len(c) - np.searchsorted(c, st - b2, 'left')
            in_p = np.isin(t, prob.train[u])
            pnt = int(prob.pnt[s])
            near = (~in_p) & (np.abs(st + 1024.0) <= b2)              # a score within rounding of the train positives' -1024
            t_lo = (st[None, :] > st[:, None] + b2).sum(1)
            t_hi = (st[None, :] >= st[:, None] - b2).sum(1) - 1
            lo.append(l); hi.append(h); flip.append(near * pnt)
            plo.append(l + t_lo + np.where(st + b2 < -1024.0, pnt, 0) + np.where(in_p, pnt, 0))
            phi.append(h + t_hi + np.where(st - b2 <= -1024.0, pnt, 0))
            ex = np.sort(S[s, prob.candidates(s)])
            g64 = len(ex) - np.searchsorted(ex, st, 'right')
            e64 = np.searchsorted(ex, st, 'right') - np.searchsorted(ex, st, 'left')
            r = restate(st, g64, e64, pnt, prob.m_items, KS)
            self.auc64.append(r['auc']); self.recall64.append(r['recall']); self.inv_n.append(np.full(n, 1.0 / max(n, 1)))
        self.lo, self.hi, self.flip = np.concatenate(lo), np.concatenate(hi), np.concatenate(flip)
        self.pos_lo, self.pos_hi = np.concatenate(plo), np.concatenate(phi)
        self.auc64, self.recall64, self.inv_n = np.array(self.auc64), np.array(self.recall64), np.concatenate(self.inv_n)
        self.prob = prob

    def check_counts(self, gt, eq):
        gt, eq = gt.astype(np.int64), eq.astype(np.int64)
        bad = (self.lo > gt) | (gt + eq > self.hi) | (eq < 0)
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4].tolist(), self.lo[bad][:4], gt[bad][:4], eq[bad][:4], self.hi[bad][:4])

    def check_auc(self, auc):
        p = self.prob
        n = np.diff(p.test_ptr)
        cs = np.concatenate([[0], np.cumsum(self.hi - self.lo + self.flip)])
        slack = cs[p.test_ptr[1:]] - cs[p.test_ptr[:-1]]
        tol = slack / np.maximum(n * (p.m_items - n), 1) + 1e-12
        err = np.abs(auc - self.auc64)
        assert (err <= tol).all(), (int((err > tol).sum()), float(err.max()), float(tol[np.argmax(err)]))
        return tol


@functools.lru_cache(maxsize=None)
def _gauss_problem(m_items, d, n_eval=257):
    rng = np.random.Generator(np.random.PCG64(7 * d + m_items))
    n_users = 150
    E = (0.1 * rng.standard_normal((n_users + m_items, d))).astype(np.float32)
    users = rng.integers(0, n_users, n_eval).astype(np.int32)
    train, test = _lists(rng, m_items, n_users, users, ROUND_LENS)
    prob = Problem(E, n_users, users, train, test)
    return prob, Bounds(prob)


def _metrics(pkg, prob, dev, score, gt, eq, ks):
    Ed, ud, tp_, ti, sp, si = dev
    per_user, sums = pkg._lib.eval_rank_metrics(prob.m_items, ud, tp_, ti, sp, si, score, gt, eq, ks)
    return per_user.cpu().numpy(), sums.cpu().numpy()


@gpu
@pytest.mark.parametrize("m_items,d", ROUNDING)
def test_ranks_rounding_aware(pkg, m_items, d):
    prob, bd = _gauss_problem(m_items, d)
    share = float((bd.lo != bd.hi).mean())
    print(f"m={m_items} d={d}: {100 * share:.1f} % of the intervals are non-trivial")
    assert share <= 0.25                                              # the bounds pin most counts exactly: not a vacuous test
    dev = prob.device()
    nk = len(KS)
    for fp32 in (False, True):
        score, gt, eq = _run(pkg, prob, dev, fp32=fp32)
        bd.check_counts(gt.cpu().numpy(), eq.cpu().numpy())
        per_user, sums = _metrics(pkg, prob, dev, score, gt, eq, KS)
        bd.check_auc(per_user[:, 3 * nk])
        for q, k in enumerate(KS):
            straddle = (bd.pos_lo < k) & (bd.pos_hi >= k)             # hit@k undecided within rounding
            tol = float(bd.inv_n[straddle].sum()) + 1e-9              # each moves its user's recall by 1 / n  (<= their count)
            got, want = float(sums[nk + q]), float(bd.recall64[:, q].sum())
            print(f"  fp32={fp32} recall@{k}: {got:.9f} vs {want:.9f}, {int(straddle.sum())} straddling")
            assert abs(got - want) <= tol, (k, got, want, tol)
            assert abs(float(per_user[:, nk + q].sum()) - got) < 1e-9


# ---------------------------------------------------------------------------------------------------------------------------
# 3. a catalogue that takes a multi-part sweep and large counters
@gpu
def test_ranks_catalogue_split(pkg):
    prob, bd = _gauss_problem(70001, 64, n_eval=97)
    print(f"{100 * float((bd.lo != bd.hi).mean()):.1f} % of the intervals are non-trivial")
    dev = prob.device()
    score, gt, eq = _run(pkg, prob, dev)
    bd.check_counts(gt.cpu().numpy(), eq.cpu().numpy())
    again = _run(pkg, prob, dev)
    assert torch.equal(again[1], gt) and torch.equal(again[2], eq) and torch.equal(again[0], score)
    per_user, _ = _metrics(pkg, prob, dev, score, gt, eq, [20, 70001])
    bd.check_auc(per_user[:, 6])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. Procedure.Test
def _make_model(pkg, g, tmp_path):
    d = os.path.join(str(tmp_path), g.name)
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(g.dir, f), os.path.join(d, f))
    w = pkg.world
    w.configure([])
    w.dataset = g.name
    w.config.update({'lightGCN_n_layers': g.K, 'latent_dim_rec': g.d, 'bpr_batch_size': g.B, 'act_dtype': 'fp32',
                     'decay': g.meta["decay"], 'lr': g.meta["lr"], 'row_order': 'cocluster', 'reg_rows': 'propagated'})
    w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=d)
    pkg.sampling.seed(w.seed)
    pkg.utils.set_seed(w.seed)
    return ds, pkg.model.LightGCN(w.config, ds).to(DEV)


@gpu
def test_procedure_test_rank_metrics(pkg, lastfm, tmp_path):
    g = lastfm
    ds, m = _make_model(pkg, g, tmp_path)
    users, pos, neg = pkg.Procedure.sample_epoch_to_device(ds, DEV)
    m.fused_epoch(users, pos, neg, g.B)
    m.eval()
    w = pkg.world
    old_topks = list(w.topks)
    try:
        # ---- flag off: what Test was -- three keys, the values of _test_fused (that code is unchanged)
        assert w.config['rank_metrics'] == 0
        w.topks = [20]
        r_off = pkg.Procedure.Test(ds, m, 0)
        assert sorted(r_off) == ['ndcg', 'precision', 'recall']
        ev = ds._lgcn_eval_index
        with torch.no_grad():
            direct, _ = pkg.Procedure._test_fused(m, ev, 20)
        for name in direct:
            assert np.array_equal(r_off[name], direct[name])
        # ---- flag on
        w.topks = KS
        w.config['rank_metrics'] = 1
        r_on = pkg.Procedure.Test(ds, m, 0)
        assert sorted(r_on) == ['auc', 'mrr', 'ndcg', 'precision', 'recall']
        w.config['rank_metrics'] = 0
        w.config['eval_fused'] = 0
        r_torch = pkg.Procedure.Test(ds, m, 0)
        assert sorted(r_torch) == ['ndcg', 'precision', 'recall']
    finally:
        w.topks = old_topks
        w.config['rank_metrics'] = 0
        w.config['eval_fused'] = 1
    with torch.no_grad():
        E = m.rating_table().cpu().numpy()
    eval_users = ev.users.astype(np.int32)
    train = [np.asarray(ds.allPos[u], np.int32) for u in range(ds.n_users)]
    train = [np.sort(t) for t in train]
    test = [np.sort(np.asarray(ds.testDict[u], np.int32)) for u in eval_users.tolist()]
    prob = Problem(E, ds.n_users, eval_users, train, test)
    bd = Bounds(prob)
    n = len(eval_users)
    for q, k in enumerate(KS):
        straddle = int(((bd.pos_lo < k) & (bd.pos_hi >= k)).sum())
        print(f"@{k}: {straddle} test items straddle; rank {[r_on[x][q] for x in ('precision', 'recall', 'ndcg')]}")
        tol = straddle / n + 1e-9                                     # an undecided hit moves one user's metric by at most 1
        for name in ('precision', 'recall', 'ndcg'):
            assert abs(float(r_on[name][q]) - float(r_torch[name][q])) <= tol, (k, name, r_on[name][q], r_torch[name][q], tol)
    # auc: the harness's own rows (model.getUsersRating, fp32) masked to -1024, through utils.AUC
    with torch.no_grad():
        rating = m.getUsersRating(torch.from_numpy(ev.users).to(DEV)).cpu().numpy()
    aucs = []
    for s, u in enumerate(eval_users.tolist()):
        rating[s, train[u]] = -1024.0
        aucs.append(pkg.utils.AUC(rating[s], ds, test[s].tolist()))
    nn = np.diff(prob.test_ptr)
    slack = np.array([(bd.hi - bd.lo + bd.flip)[prob.test_ptr[s]:prob.test_ptr[s + 1]].sum() for s in range(n)])
    bound = float((slack / np.maximum(nn * (prob.m_items - nn), 1)).mean()) + 1e-12      # both counts lie in [lo, hi]
    print(f"auc {r_on['auc']:.12f} vs harness {np.mean(aucs):.12f}, bound {bound:.3e}; mrr {r_on['mrr']:.12f}")
    assert abs(r_on['auc'] - float(np.mean(aucs))) <= bound
    # mrr: the restatement on the kernel's own counts
    L = pkg._lib
    score, gt, eq = L.eval_ranks(m.rating_table(), ds.n_users, ev.users32, ev.train_ptr, ev.train_idx32, ev.test_ptr, ev.test_sorted32)
    score, gt, eq = score.cpu().numpy(), gt.cpu().numpy(), eq.cpu().numpy()
    mrr = np.mean([restate(score[prob.test_ptr[s]:prob.test_ptr[s + 1]], gt[prob.test_ptr[s]:prob.test_ptr[s + 1]],
                           eq[prob.test_ptr[s]:prob.test_ptr[s + 1]], prob.pnt[s], prob.m_items, KS)['mrr'] for s in range(n)])
    assert abs(r_on['mrr'] - float(mrr)) < 1e-12
    rows = open(os.path.join(w.config['checkpoint_dir'], 'valid_epoch_metrics.csv')).read().strip().splitlines()
    assert rows[0] == 'epoch,precision,recall,ndcg' and all(len(r.split(',')) == 4 for r in rows)     # the CSV keeps its columns


# ---------------------------------------------------------------------------------------------------------------------------
# 5. refusals: nothing launched, outputs untouched
@gpu
def test_ranks_refusals_leave_outputs_untouched(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    prob, _, _, _ = _exact_problem(300, 32)
    Ed, ud, tp_, ti, sp, si = prob.device()
    n, n_test = len(prob.users), len(prob.test_idx)
    score = torch.full((n_test,), 7.0, dtype=torch.float32, device=DEV)
    gt = torch.full((n_test,), -7, dtype=torch.int32, device=DEV)
    eq = torch.full((n_test,), -7, dtype=torch.int32, device=DEV)
    per_user = torch.full((n, 5), 7.0, dtype=torch.float64, device=DEV)
    sums = torch.full((5,), 7.0, dtype=torch.float64, device=DEV)

    def c_ranks(d=32, n_eval=n, nt=n_test, flags=0, m_items=prob.m_items):
        return lib.lgcn_eval_ranks(L.tp(Ed), prob.n_users, m_items, d, L.tp(ud), n_eval, L.tp(tp_), L.tp(ti), L.tp(sp), L.tp(si), nt,
                                   L.tp(score), L.tp(gt), L.tp(eq), flags, L.current_stream())
    for kw in ({'d': 48}, {'d': 16}, {'n_eval': -1}, {'nt': -1}, {'flags': 4}, {'m_items': 0}, {'nt': n * prob.m_items + 1}):
        assert c_ranks(**kw) == 3, kw

    def c_metrics(ks, m_items=prob.m_items, nt=n_test):
        ks = np.asarray(ks, np.int32)
        return lib.lgcn_eval_rank_metrics(n, m_items, L.tp(ud), L.tp(tp_), L.tp(ti), L.tp(sp), L.tp(si), nt, L.tp(score), L.tp(gt),
                                          L.tp(eq), L.npp(ks), len(ks), L.tp(per_user), L.tp(sums), L.current_stream())
    assert c_metrics([20, prob.m_items + 1]) == 3
    assert c_metrics([0]) == 3
    assert c_metrics([]) == 3
    assert c_metrics([20], nt=-1) == 3
    # the wrappers refuse buffers that do not hold n_test entries, wrong types and cut-offs past the catalogue
    for bad in ({'scores': score[:-1]}, {'gt': gt[:-1].clone()}, {'eq': eq.long()}, {'gt': gt.cpu()}):
        with pytest.raises(ValueError):
            L.eval_ranks(Ed, prob.n_users, ud, tp_, ti, sp, si, **{'scores': score, 'gt': gt, 'eq': eq, **bad})
    with pytest.raises(ValueError):
        L.eval_ranks(Ed, prob.n_users, ud, tp_, ti, sp[:-1], si, scores=score, gt=gt, eq=eq)
    with pytest.raises(ValueError):
        L.eval_ranks(Ed[:, :16].contiguous(), prob.n_users, ud, tp_, ti, sp, si, scores=score, gt=gt, eq=eq)
    with pytest.raises(ValueError):
        L.eval_rank_metrics(prob.m_items, ud, tp_, ti, sp, si, score, gt, eq, [20, prob.m_items + 1], per_user=per_user, sums=sums)
    with pytest.raises(ValueError):
        L.eval_rank_metrics(prob.m_items, ud, tp_, ti, sp, si, score, gt[:-1], eq, [20], per_user=per_user, sums=sums)
    with pytest.raises(ValueError):
        L.eval_rank_metrics(prob.m_items, ud, tp_, ti, sp, si, score, gt, eq, [20], per_user=per_user[:, :4].contiguous(), sums=sums)
    torch.cuda.synchronize()
    assert bool((score == 7.0).all()) and bool((gt == -7).all()) and bool((eq == -7).all())
    assert bool((per_user == 7.0).all()) and bool((sums == 7.0).all())

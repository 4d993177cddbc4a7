"""Rank-based evaluation, host side (no GPU): the new symbols in the header, the binding and the library with the ABI still
13; the --rank_metrics flag; utils.AUC against brute-force pair counting; the refusals of the two C entry points (null
pointers suffice: every check precedes any launch); and a numpy restatement of pos / hit@K / AUC / MRR from
(score, gt, eq), checked here against a direct sort of the reference's row and reused by the GPU tests."""
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# The contract, restated in numpy.  One evaluation slot: the reference's row L (fp, -1024 at the train positives), the train
# positives P and the test list T (ascending ids).
def counts_from_row(L, P, T):
    """(score, gt, eq) of a slot from its full row L: score[t] = L[t]; gt / eq count the items outside P and T above / level."""
    L = np.asarray(L)
    T = np.asarray(T, np.int64)
    cand = np.ones(len(L), bool)
    cand[np.asarray(P, np.int64)] = False
    cand[T] = False
    c = L[cand]
    score = L[T]
    gt = np.array([(c > s).sum() for s in score], np.int64)
    eq = np.array([(c == s).sum() for s in score], np.int64)
    return score, gt, eq


def positions(score, gt, eq, n_train_not_test):
    """pos[t]: the place of test item t in the row sorted best first.  A tie with a non-test item goes against the test item;
    a tie among test items goes to the lower id (score[] is in ascending id order).  The n_train_not_test train positives
    outside T sit at -1024."""
    score = np.asarray(score, np.float64)
    n = len(score)
    c = np.empty(n, np.int64)                            # test items ahead of t: higher score, or the same score and a lower id
    c[np.lexsort((np.arange(n), -score))] = np.arange(n)
    return np.asarray(gt, np.int64) + np.asarray(eq, np.int64) + (score <= -1024.0) * int(n_train_not_test) + c


def restate(score, gt, eq, n_train_not_test, m_items, ks):
    """Per-slot metrics from (score, gt, eq): dict with precision / recall / ndcg arrays over ks, auc, mrr, pos."""
    score = np.asarray(score, np.float64)
    gt, eq = np.asarray(gt, np.int64), np.asarray(eq, np.int64)
    n, m, pnt = len(score), int(m_items), int(n_train_not_test)
    out = {'precision': np.zeros(len(ks)), 'recall': np.zeros(len(ks)), 'ndcg': np.zeros(len(ks)), 'auc': 0.0, 'mrr': 0.0,
           'pos': np.zeros(0, np.int64)}
    if n == 0:
        return out
    pos = positions(score, gt, eq, pnt)
    out['pos'] = pos
    for q, k in enumerate(ks):
        hit = np.sort(pos[pos < k])
        right = float(len(hit))
        dcg = float(np.sum(1.0 / np.log2(hit + 2.0)))
        idcg = float(np.sum(1.0 / np.log2(np.arange(min(k, n)) + 2.0)))
        out['precision'][q] = right / k
        out['recall'][q] = right / n
        out['ndcg'][q] = dcg / (idcg if idcg != 0.0 else 1.0)
    if n < m:
        rest = m - n - pnt
        less = rest - gt - eq + (score > -1024.0) * pnt
        same = eq + (score == -1024.0) * pnt
        out['auc'] = float((2 * less + same).sum()) / (2.0 * n * (m - n))
    out['mrr'] = 1.0 / (1.0 + float(pos.min()))
    return out


def brute_force(L, T, ks):
    """The same metrics from a direct sort of the row: key (score descending, non-test before test, id ascending)."""
    L = np.asarray(L, np.float64)
    m, T = len(L), np.asarray(T, np.int64)
    is_t = np.zeros(m, bool)
    is_t[T] = True
    order = np.lexsort((np.arange(m), is_t, -L))
    place = np.empty(m, np.int64)
    place[order] = np.arange(m)
    pos = place[T]
    n = len(T)
    out = {'pos': pos, 'precision': np.zeros(len(ks)), 'recall': np.zeros(len(ks)), 'ndcg': np.zeros(len(ks)), 'auc': 0.0, 'mrr': 0.0}
    if n == 0:
        return out
    for q, k in enumerate(ks):
        r = is_t[order[:k]].astype(np.float64)
        disc = 1.0 / np.log2(np.arange(2, k + 2))
        idcg = disc[:min(k, n)].sum()
        out['precision'][q] = r.sum() / k
        out['recall'][q] = r.sum() / n
        out['ndcg'][q] = (r * disc).sum() / (idcg if idcg != 0.0 else 1.0)
    if n < m:
        neg = L[~is_t]
        out['auc'] = sum(float((neg < s).sum()) + 0.5 * float((neg == s).sum()) for s in L[T]) / (n * (m - n))
    out['mrr'] = 1.0 / (1.0 + pos.min())
    return out


def _rows(seed):
    """Rows with ties (integer scores), -1024 entries, a test item that is a train positive, a constant row."""
    rng = np.random.Generator(np.random.PCG64(seed))
    m = 200
    for case in range(12):
        L = rng.integers(-3, 4, m).astype(np.float64)
        if case == 0:
            L[:] = 1.0
        P = np.sort(rng.choice(m, int(rng.integers(0, 30)), replace=False))
        n = [0, 1, 2, 17, 60, m][case % 6]
        T = np.sort(rng.choice(m, n, replace=False))
        if case % 3 == 1 and len(P) and n < m:
            T = np.union1d(T, P[:1])
        L[P] = -1024.0
        yield L, P, T


def test_restatement_agrees_with_a_direct_sort():
    ks = [1, 5, 20, 150, 200]
    for seed in range(3):
        for L, P, T in _rows(seed):
            score, gt, eq = counts_from_row(L, P, T)
            pnt = len(np.setdiff1d(P, T))
            a, b = restate(score, gt, eq, pnt, len(L), ks), brute_force(L, T, ks)
            assert np.array_equal(a['pos'], b['pos'])
            for name in ('precision', 'recall', 'ndcg'):
                np.testing.assert_allclose(a[name], b[name], rtol=0, atol=1e-12)
            assert abs(a['auc'] - b['auc']) < 1e-12 and abs(a['mrr'] - b['mrr']) < 1e-15


def test_constant_table_does_not_score():
    L = np.zeros(50)
    score, gt, eq = counts_from_row(L, [], [3, 7])
    r = restate(score, gt, eq, 0, 50, [20])
    assert r['pos'].tolist() == [48, 49] and r['recall'][0] == 0.0 and r['auc'] == 0.5


def test_utils_auc_equals_pair_counting(pkg):
    class DS:
        m_items = 200
    for seed in range(3):
        for L, P, T in _rows(seed + 10):
            got = pkg.utils.AUC(L, DS, T.tolist())
            n = len(T)
            if n == 0 or n == len(L):
                assert got == 0.0
                continue
            neg = np.delete(L, T)
            want = sum(float((neg < s).sum()) + 0.5 * float((neg == s).sum()) for s in L[T]) / (n * (len(L) - n))
            assert abs(got - want) <= 1e-15, (got, want)
    src = open(os.path.join(REPO, pkg.__name__, "utils.py")).read()
    assert not re.search(r"^\s*(import|from)\s+sklearn", src, flags=re.M)


def test_symbols_in_header_binding_and_library(pkg):
    header = open(os.path.join(REPO, "include", "lgcn_hip.h")).read()
    assert int(re.search(r"#define\s+LGCN_ABI_VERSION\s+(\d+)", header).group(1)) == 13 == pkg._lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = pkg._lib.load()
    assert lib.lgcn_abi_version() == 13
    for name in ("lgcn_eval_ranks", "lgcn_eval_rank_metrics"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in pkg._lib.SIGNATURES and hasattr(lib, name)
    assert callable(pkg._lib.eval_ranks) and callable(pkg._lib.eval_rank_metrics)
    assert "tie" in header.lower() and "against the test item" in header.lower()
    assert lib.lgcn_eval_kmax() == 256                                   # the list-based path keeps its limit
    assert any(s.endswith("lgcn_eval_ranks.hip") for s in pkg.build.SOURCES)


def test_flag_reaches_the_config(pkg):
    w = pkg.world
    try:
        assert w.configure([])['rank_metrics'] == 0
        assert w.configure(['--rank_metrics', '1'])['rank_metrics'] == 1
    finally:
        w.configure([])


def test_refusals_c_level(pkg):
    """rc 3 with nothing launched: every pointer below is fake or null and is never dereferenced."""
    L, lib = pkg._lib, pkg._lib.load()
    fake = L._vp(256)

    def ranks(d=64, n_users=50, m_items=1000, n_eval=10, n_test=40, flags=0, E=fake, gt=fake):
        return lib.lgcn_eval_ranks(E, n_users, m_items, d, fake, n_eval, fake, fake, fake, fake, n_test, fake, gt, fake, flags, None)
    for d in (0, 16, 48, 96, 512, -64):
        assert ranks(d=d) == 3
    assert ranks(n_eval=-1) == 3
    assert ranks(n_test=-1) == 3
    assert ranks(m_items=0) == 3
    assert ranks(n_users=0) == 3
    assert ranks(flags=2) == 3
    assert ranks(n_test=10 * 1000 + 1) == 3                  # more entries than n_eval full lists hold
    assert ranks(E=None) == 3
    assert ranks(gt=None) == 3
    assert ranks(n_eval=0, n_test=0) == 0                    # nothing to rank: nothing launched, success
    assert ranks(n_test=0) == 0

    def metrics(ks, n_ks=None, n_eval=10, m_items=1000, n_test=40, per_user=fake):
        ks = np.asarray(ks, np.int32)
        return lib.lgcn_eval_rank_metrics(n_eval, m_items, fake, fake, fake, fake, fake, n_test, fake, fake, fake,
                                          L.npp(ks), len(ks) if n_ks is None else n_ks, per_user, fake, None)
    assert metrics([20, 1001]) == 3                          # a cut-off past the catalogue
    assert metrics([0]) == 3
    assert metrics([20], n_ks=0) == 3
    assert metrics([1] * 9) == 3
    assert metrics([20], n_eval=-1) == 3
    assert metrics([20], n_test=-1) == 3
    assert metrics([20], m_items=0) == 3
    assert metrics([20], per_user=None) == 3
    assert lib.lgcn_last_error()

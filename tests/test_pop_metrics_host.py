"""Popularity-aware evaluation, host side (no GPU): the numpy restatement of lgcn_eval_pop_metrics on a case worked out by hand,
the closed forms of the Gini index, its sums against utils.RecallPrecision_ATk, utils.popularity_groups / pack_item_info /
pop_results, the three flags, the symbol in header, binding and library (ABI still 13), the C-level refusals (fake pointers
suffice: every check precedes any launch) and the refusals of Procedure.Test, which raise before anything touches a GPU."""
import os
import re

import numpy as np
import pytest

import pop_metrics_restatement as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------------
# 3 slots, 6 items, K = 3, G = 2.  pop = 5 4 3 2 1 0, head = items {0, 1}.
#   slot 0: list 0 2 4,  test {2, 4}      slot 1: list 1 0 5,  test {0}      slot 2: list 0 3 -1,  test {1, 3}
HAND = dict(topk=[[0, 2, 4], [1, 0, 5], [0, 3, -1]], test_ptr=[0, 2, 3, 5], test_items=[2, 4, 0, 1, 3],
            pop=[5, 4, 3, 2, 1, 0], groups=[0, 0, 1, 1, 1, 1], G=2, ks=[1, 3])


def test_restatement_on_a_case_worked_by_hand():
    r = pr.restate(**HAND)
    # k = 1: the first entries 0, 1, 0 hit nothing.  k = 3: slot 0 hits 2 and 4 (tail, 2 of its 2 test items, both tail); slot 1
    # hits 0 (head, its only test item); slot 2 hits 3 (tail; 1 of 2 test items, 1 of its 1 tail test items), misses head item 1.
    assert r['sums'].tolist() == [[[0.0, 0.0], [0.0, 0.0]], [[1.0, 1.5], [1.0, 2.0]]]
    assert r['group_slots'].tolist() == [2, 2]               # head test items: slots 1, 2; tail: slots 0, 2
    # list entries per group | valid | sum of pop | covered | sum of e | Gini numerator
    #   k = 1: e = 2 1 0 0 0 0 -> |2-1| + 4 |2-0| + 4 |1-0| = 13;  k = 3: e = 3 1 1 1 1 1 -> 5 |3-1| = 10
    assert r['counts'].tolist() == [[3, 0, 3, 14, 2, 3, 13], [4, 4, 8, 25, 6, 8, 10]]
    assert r['exposure'].tolist() == [[2, 1, 0, 0, 0, 0], [3, 1, 1, 1, 1, 1]]
    assert r['per_slot'][2, 1].tolist() == [[0.0, 0.5], [0.0, 1.0]]
    assert r['recall_share'].tolist() == [[0.0, 1.0 / 3], [0.0, 0.5]]
    assert r['recall_by_group'].tolist() == [[0.0, 0.5], [0.0, 1.0]]
    assert r['list_share'].tolist() == [[1.0, 0.5], [0.0, 0.5]]
    assert r['arp'].tolist() == [14 / 3, 25 / 8]
    assert r['coverage'].tolist() == [2 / 6, 1.0]
    assert r['gini'].tolist() == [13 / (6 * 3), 10 / (6 * 8)]


def test_pop_results_divides_as_the_restatement(pkg):
    r = pr.restate(**HAND)
    got = pkg.utils.pop_results(r['sums'], r['counts'], r['group_slots'], 3, 6)
    for name in ('recall_share', 'recall_by_group', 'list_share', 'arp', 'coverage', 'gini', 'group_users'):
        assert np.array_equal(got[name], r[name]), name
        assert np.asarray(got[name]).shape == np.asarray(r[name]).shape
    # an empty group, no valid entry, nobody exposed: zeros, no NaN
    z = pkg.utils.pop_results(np.zeros((1, 2, 2)), np.zeros((1, 7), np.int64), np.zeros(2, np.int64), 0, 6)
    assert all(np.all(np.asarray(v) == 0) for v in z.values())


def test_gini_closed_forms():
    m = 7
    assert pr.gini_numerator(np.full(m, 4)) == 0                             # all items equally exposed
    one = np.zeros(m, np.int64); one[3] = 9
    assert pr.gini_numerator(one) == 9 * (m - 1)                             # one item holds all exposure: Gini = (m - 1) / m
    assert pr.gini_numerator(one) / (m * one.sum()) == (m - 1) / m
    assert pr.gini_numerator(np.zeros(m, np.int64)) == 0                     # nobody exposed
    r = pr.restate([[-1, -1]], [0, 0], [], [1, 1, 1], [0, 0, 0], 1, [2])
    assert r['gini'].tolist() == [0.0] and r['coverage'].tolist() == [0.0] and r['arp'].tolist() == [0.0]
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(20):
        e = rng.integers(0, 6, int(rng.integers(1, 40)))
        assert pr.gini_numerator(e) == pr.gini_numerator_pairs(e)
        # the histogram form the kernel uses: sum_v v H[v] (2 R_v + H[v] - m)
        H = np.bincount(e)
        R = np.cumsum(H) - H
        assert int(np.sum(np.arange(len(H)) * H * (2 * R + H - len(e)))) == pr.gini_numerator(e)


def _random_case(seed, n=40, m=60, K=12, G=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    topk = np.stack([rng.permutation(m)[:K] for _ in range(n)])
    topk[::7, K - 2:] = -1
    lens = rng.integers(0, 9, n)
    lens[0] = 0
    test = [np.sort(rng.choice(m, int(l), replace=False)) for l in lens]
    ptr = np.zeros(n + 1, np.int64); np.cumsum(lens, out=ptr[1:])
    pop = rng.integers(0, 50, m)
    groups = rng.integers(0, G, m)
    return topk, ptr, (np.concatenate(test) if ptr[-1] else np.zeros(0, np.int64)), pop, groups, G, test


def test_group_sums_equal_recall_and_shares_sum_to_one(pkg):
    ks = [5, 1, 12]
    for seed in range(3):
        topk, ptr, items, pop, groups, G, test = _random_case(seed)
        r = pr.restate(topk, ptr, items, pop, groups, G, ks)
        keep = [s for s in range(len(test)) if len(test[s])]                 # (RecallPrecision_ATk divides by |T_s|)
        lab = np.array([[1.0 if x in test[s] else 0.0 for x in topk[s]] for s in keep])
        for q, k in enumerate(ks):
            want = pkg.utils.RecallPrecision_ATk([test[s] for s in keep], lab, k)['recall'] / len(test)
            assert abs(r['recall_share'][:, q].sum() - want) <= 4 * 2.0 ** -53 * max(want, 1e-300) * len(test)
            assert abs(r['list_share'][:, q].sum() - 1.0) <= 4 * 2.0 ** -53
        assert r['counts'][:, :G].sum(axis=1).tolist() == r['counts'][:, G].tolist()


def test_popularity_groups(pkg):
    pg = pkg.utils.popularity_groups
    pop = np.array([3, 9, 3, 0, 9, 1, 3, 0, 2, 5])
    # ranked by (pop descending, id ascending): 1 4 9 0 2 6 8 5 3 7
    assert pg(pop, [0.2]).tolist() == [1, 0, 1, 1, 0, 1, 1, 1, 1, 1] and pg(pop, [0.2]).dtype == np.int32
    assert pg(pop, [0.3, 0.5]).tolist() == [1, 0, 1, 2, 0, 2, 2, 2, 2, 0]        # ties at pop 3 broken by id: items 0, 2 are ranks 4, 5; item 6 is not
    g = pg(pop, [0.3, 0.6])                                                      # ranks 1-3 | 4-6 | 7-10
    assert g.tolist() == [1, 0, 1, 2, 0, 2, 1, 2, 2, 0]
    # all degrees equal: the id decides
    assert pg(np.full(10, 4), [0.2, 0.5]).tolist() == [0, 0, 1, 1, 1, 2, 2, 2, 2, 2]
    # by interactions: 35 in all; cumulative 9 18 23 26 29 32 34 35 35 35 along the ranking; boundaries 17.5 and 28
    gi = pg(pop, [0.5, 0.8], by='interactions')
    assert gi.tolist() == [1, 0, 2, 2, 1, 2, 2, 2, 2, 1]
    # an empty group is legal
    assert pg(np.array([5, 1]), [0.1, 0.5]).tolist() == [1, 2]
    assert pg(np.zeros(0, np.int64), [0.2]).tolist() == []
    for bad in ([0.0], [1.0], [0.5, 0.5], [0.6, 0.2], [float('nan')], [0.1] * 8, "nonsense(", "{'a': 1}", [[0.2]], ["0.2"]):
        with pytest.raises(ValueError, match="pop_groups"):
            pg(pop, bad)
    with pytest.raises(ValueError, match="pop_group_by"):
        pg(pop, [0.2], by='users')
    with pytest.raises(ValueError, match="pop must"):
        pg(np.array([1, -1]), [0.2])
    assert pkg.utils.pop_fractions("[0.2, 0.5]") == [0.2, 0.5] and pkg.utils.pop_fractions("[]") == []


def test_pack_item_info(pkg):
    pack = pkg.utils.pack_item_info
    w = pack([0, 5, (1 << 28) - 1], [0, 1, 7])
    assert w.dtype == np.int32 and w.view(np.uint32).tolist() == [0, 41, 0x7fffffff]
    with pytest.raises(ValueError, match="2\\^28"):
        pack([1 << 28], [0])
    with pytest.raises(ValueError, match="2\\^28"):
        pack([-1], [0])
    with pytest.raises(ValueError, match="groups"):
        pack([1], [8])
    with pytest.raises(ValueError):
        pack([1, 2], [0])


def test_item_popularity_counts_train_interactions(pkg):
    class DS:
        m_items = 6

        def pos_csr(self):
            return np.array([0, 2, 5]), np.array([1, 4, 0, 1, 4])
    assert pkg.utils.item_popularity(DS()).tolist() == [1, 2, 0, 0, 2, 0]        # a cold item has 0


def test_flags_reach_the_config(pkg):
    w = pkg.world
    try:
        c = w.configure([])
        assert (c['pop_metrics'], c['pop_groups'], c['pop_group_by']) == (0, "[0.2]", 'items')
        c = w.configure(['--pop_metrics', '1', '--pop_groups', '[0.1, 0.5]', '--pop_group_by', 'interactions'])
        assert (c['pop_metrics'], c['pop_groups'], c['pop_group_by']) == (1, "[0.1, 0.5]", 'interactions')
        with pytest.raises(SystemExit):
            pkg.parse.parse_args(['--pop_group_by', 'users'])
    finally:
        w.configure([])


def test_symbol_in_header_binding_and_library(pkg):
    header = open(os.path.join(REPO, "include", "lgcn_hip.h")).read()
    assert int(re.search(r"#define\s+LGCN_ABI_VERSION\s+(\d+)", header).group(1)) == 13 == pkg._lib.ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = pkg._lib.load()
    assert lib.lgcn_abi_version() == 13
    assert re.search(r"\blgcn_eval_pop_metrics\s*\(", code)
    assert "lgcn_eval_pop_metrics" in pkg._lib.SIGNATURES and hasattr(lib, "lgcn_eval_pop_metrics")
    assert callable(pkg._lib.eval_pop_metrics)
    assert "lgcn_eval_pop.hip" in [os.path.basename(s) for s in pkg.build.SOURCES]
    assert all(os.path.exists(s) for s in pkg.build.SOURCES)


def test_refusals_c_level(pkg):
    """rc 3 with nothing launched: every pointer below is fake or null and is never dereferenced."""
    L, lib = pkg._lib, pkg._lib.load()
    fake = L._vp(256)

    def call(ks=(20,), n_ks=None, n_eval=10, K=20, m_items=1000, G=2, topk=fake, tptr=fake, tidx=fake, info=fake, sums=fake,
             counts=fake, slots=fake, ks_null=False):
        ks = np.asarray(ks, np.int32)
        return lib.lgcn_eval_pop_metrics(topk, n_eval, K, tptr, tidx, info, m_items, G, None if ks_null else L.npp(ks),
                                         len(ks) if n_ks is None else n_ks, sums, counts, slots, None, None, None)
    for kw, word in ((dict(G=0), "n_groups"), (dict(G=9), "n_groups"), (dict(n_ks=0), "n_ks"), (dict(ks=[1] * 9), "n_ks"),
                     (dict(ks=[0]), "cut-off"), (dict(ks=[5, 21]), "cut-off"), (dict(K=0), "K"), (dict(K=257, ks=[257]), "K"),
                     (dict(n_eval=-1), "n_eval"), (dict(m_items=-5), "m_items"), (dict(m_items=0), "m_items"),
                     (dict(topk=None), "topk_items"), (dict(tptr=None), "test_indptr"), (dict(tidx=None), "test_items_sorted"),
                     (dict(info=None), "item_info"), (dict(sums=None), "sums_f64"), (dict(counts=None), "counts_i64"),
                     (dict(slots=None), "group_slots"), (dict(ks_null=True), "ks"),
                     (dict(n_eval=1 << 30, K=256, m_items=1 << 24), "2^62")):
        assert call(**kw) == 3, kw
        assert word in lib.lgcn_last_error().decode(), (kw, lib.lgcn_last_error())
    assert lib.lgcn_eval_kmax() == 256


def test_procedure_test_refusals_raise_before_any_gpu_work(pkg):
    """Each raises by name; dataset and model are None, so anything past the checks would fail differently."""
    w = pkg.world
    old_topks = list(w.topks)
    try:
        w.configure(['--pop_metrics', '1', '--rank_metrics', '1'])
        w.topks = [20]
        with pytest.raises(ValueError, match="--rank_metrics"):
            pkg.Procedure.Test(None, None, 0)
        w.configure(['--pop_metrics', '1', '--eval_fused', '0'])
        w.topks = [20]
        with pytest.raises(ValueError, match="--eval_fused"):
            pkg.Procedure.Test(None, None, 0)
        w.configure(['--pop_metrics', '1'])
        w.topks = [20, 300]
        with pytest.raises(ValueError, match="lgcn_eval_kmax"):
            pkg.Procedure.Test(None, None, 0)
        w.configure(['--pop_metrics', '1', '--pop_groups', '[0.7, 0.2]'])
        w.topks = [20]
        with pytest.raises(ValueError, match="pop_groups"):
            pkg.Procedure.Test(None, None, 0)
    finally:
        w.configure([])
        w.topks = old_topks


def test_finish_test_adds_pop_scalars_and_keeps_the_csv(pkg, tmp_path):
    class Writer:
        def __init__(self):
            self.tags = []

        def add_scalars(self, tag, values, epoch):
            self.tags.append(tag)

        def add_scalar(self, tag, value, epoch):
            self.tags.append(tag)
    w = pkg.world
    old_topks, old_tb = list(w.topks), w.tensorboard
    try:
        w.configure(['--checkpoint_dir', str(tmp_path)])
        w.topks, w.tensorboard = [1, 3], True
        r = pr.restate(**HAND)
        res = {m: np.array([0.1, 0.2]) for m in ('precision', 'recall', 'ndcg')}
        plain, with_pop = Writer(), Writer()
        pkg.Procedure._finish_test(dict(res), 0, plain)
        res.update(pkg.utils.pop_results(r['sums'], r['counts'], r['group_slots'], 3, 6))
        pkg.Procedure._finish_test(res, 1, with_pop)
    finally:
        w.configure([])
        w.topks, w.tensorboard = old_topks, old_tb
    assert not any(t.startswith('Test/Pop') for t in plain.tags) and len(plain.tags) == 3
    pop_tags = [t for t in with_pop.tags if t.startswith('Test/Pop/')]
    assert len(pop_tags) == 3 * 2 + 3 and with_pop.tags[:3] == plain.tags
    assert {'Test/Pop/arp@[1, 3]', 'Test/Pop/recall_share/group1@[1, 3]'} <= set(pop_tags)
    rows = open(os.path.join(str(tmp_path), 'valid_epoch_metrics.csv')).read().split()
    assert rows[0] == 'epoch,precision,recall,ndcg' and all(len(x.split(',')) == 4 for x in rows) and len(rows) == 3

"""lgcn_eval_pop_metrics on the GPU against the numpy restatement (tests/pop_metrics_restatement.py): every integer output and
the exposures exactly, the float64 sums within (n_eval + 2) 2^-53 relative (one rounding per quotient, at most n_eval - 1
additions of non-negative terms in any order), per-slot quotients exactly (one correctly rounded division of two small integers),
bitwise repeatability with and without per_slot, n_eval = 0, the refusals, item words whose group bits exceed n_groups, and
Procedure.Test with --pop_metrics 1 on the LastFM fixture.  The kernel takes any lists, so no model and no sweep is needed except
in the last test."""
import functools
import os
import shutil

import numpy as np
import pytest
import torch

import pop_metrics_restatement as pr

gpu = pytest.mark.gpu
DEV = "cuda:0"
M_ITEMS = 3001
HOT = 7                                 # the item placed first in every list: e = n_eval, every slot adds to one counter
LENS = (0, 1, 2, 63, 64, 65, 200)
KS = {1: [1, 1], 20: [20, 5, 1, 5], 64: [64, 10, 33, 10, 1], 65: [65, 1, 64, 32, 64], 256: [100, 256, 64, 65, 100, 1, 255, 32]}
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _case(n_eval, K, G, m=M_ITEMS, seed=0):
    """(inputs as host arrays, restatement), computed once and shared.  Distinct ids per list; HOT first in every list; the last
    min(K - 1, 3) entries of a few lists are -1; test-list lengths from LENS; slot 6 repeats slot 5's user (the same test list);
    for G >= 2 no test item lies in group G - 1 (n_g = 0 there); the most popular item carries pop = 2^28 - 1."""
    rng = np.random.Generator(np.random.PCG64(1000 * K + 10 * G + seed + n_eval))
    pop = rng.integers(0, 5000, m).astype(np.int64)
    pop[HOT] = (1 << 28) - 1
    fr = [(g + 1) / (G + 1) for g in range(G - 1)]
    order = np.lexsort((np.arange(m), -pop))
    groups = np.empty(m, np.int64)
    groups[order] = np.searchsorted(np.asarray(fr) * m, np.arange(1, m + 1), side='left')
    topk = np.empty((n_eval, K), np.int64)
    for s in range(n_eval):
        row = rng.permutation(m)[:K]
        if HOT in row:
            row[row == HOT] = row[0]
        row[0] = HOT
        topk[s] = row
    tail = min(K - 1, 3)
    if tail:
        topk[3::50, K - tail:] = -1
    allowed = np.flatnonzero(groups != G - 1) if G >= 2 else np.arange(m)
    lens = rng.choice(LENS, n_eval)
    lens[:min(n_eval, len(LENS))] = LENS[:min(n_eval, len(LENS))]
    if n_eval == 1:
        lens[0] = 65
    test = [np.sort(rng.choice(allowed, int(l), replace=False)) for l in lens]
    if n_eval == 1:                                      # the only slot hits its list: HOT and up to two more
        test[0] = np.unique(np.concatenate([test[0], topk[0, :3][np.isin(topk[0, :3], allowed)]])).astype(np.int64)
    if n_eval > 6:
        test[6] = test[5]
        for s in range(8, min(n_eval, 40)):          # hits are rare among random lists: plant some, and HOT in a few test lists
            if len(test[s]) and K > 1:
                cand = topk[s, 1:][np.isin(topk[s, 1:], allowed)][:3]
                test[s] = np.unique(np.concatenate([test[s], cand, [HOT] if s % 2 else []])).astype(np.int64)      # (HOT is in group 0)
    ptr = np.zeros(n_eval + 1, np.int64)
    np.cumsum([len(t) for t in test], out=ptr[1:])
    items = np.concatenate(test).astype(np.int64) if ptr[-1] else np.zeros(0, np.int64)
    ks = KS[K]
    ref = pr.restate(topk, ptr, items, pop, groups, G, ks)
    return dict(topk=topk, ptr=ptr, items=items, pop=pop, groups=groups, G=G, ks=ks, n=n_eval, m=m, K=K), ref


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def _info(pkg, pop, groups):
    return torch.from_numpy(pkg.utils.pack_item_info(pop, groups)).to(DEV)


def _run(pkg, c, per_slot=True, exposure=True, info=None):
    n, nk, G = c['n'], len(c['ks']), c['G']
    ps = torch.full((n, nk, 2, G), -7.0, dtype=torch.float64, device=DEV) if per_slot else None
    out = pkg._lib.eval_pop_metrics(_dev(c['topk'], np.int32), _dev(c['ptr'], np.int64), _dev(c['items'], np.int32),
                                    _info(pkg, c['pop'], c['groups']) if info is None else info, G, c['ks'],
                                    per_slot=ps, want_exposure=exposure)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _judge(got, ref, n, what):
    assert np.array_equal(got['counts'], ref['counts']), (what, got['counts'].tolist(), ref['counts'].tolist())
    assert np.array_equal(got['group_slots'], ref['group_slots']), what
    if got['exposure'] is not None:
        assert np.array_equal(got['exposure'], ref['exposure']), what
    err = np.abs(got['sums'] - ref['sums'])
    bound = (n + 2) * U * np.abs(ref['sums'])
    print(what, "max |sum - restatement| / bound:", float((err / np.maximum(bound, 1e-300)).max()), "max rel:",
          float((err / np.maximum(np.abs(ref['sums']), 1e-300)).max()))
    assert np.all(err <= bound), (what, float(err.max()))
    if got['per_slot'] is not None:
        assert np.array_equal(got['per_slot'], ref['per_slot']), what


@gpu
@pytest.mark.parametrize("G", [1, 2, 8])
@pytest.mark.parametrize("K", [1, 20, 64, 65, 256])
def test_pop_metrics_equal_the_restatement(pkg, K, G):
    c, ref = _case(257, K, G)
    assert ref['exposure'][:, HOT].tolist() == [257] * len(c['ks'])
    if G >= 2:
        assert ref['group_slots'][G - 1] == 0 and ref['group_slots'][0] > 0
    if K > 1:
        assert ref['sums'].max() > 0                                         # the case does hold hits
    a = _run(pkg, c)
    _judge(a, ref, 257, f"K={K} G={G}")
    b = _run(pkg, c)                                                         # run to run: bitwise
    for k in ('sums', 'counts', 'group_slots', 'exposure', 'per_slot'):
        assert a[k].tobytes() == b[k].tobytes(), k
    d = _run(pkg, c, per_slot=False, exposure=False)                         # without the optional outputs: bitwise
    assert d['per_slot'] is None and d['exposure'] is None
    for k in ('sums', 'counts', 'group_slots'):
        assert a[k].tobytes() == d[k].tobytes(), k


@gpu
def test_pop_metrics_many_workgroups(pkg):
    """n_eval = 4099 at K = 65: more lane groups than the 1024 workgroups hold at once, so the workgroups loop over their slots and
    the partial sums of all of them are merged."""
    c, ref = _case(4099, 65, 2)
    a = _run(pkg, c)
    _judge(a, ref, 4099, "n_eval=4099")
    d = _run(pkg, c, per_slot=False, exposure=False)
    for k in ('sums', 'counts', 'group_slots'):
        assert a[k].tobytes() == d[k].tobytes(), k


@gpu
@pytest.mark.parametrize("K", [20, 65])
def test_pop_metrics_one_slot(pkg, K):
    c, ref = _case(1, K, 2)
    _judge(_run(pkg, c), ref, 1, f"n_eval=1 K={K}")


@gpu
def test_pop_metrics_no_slot_zeroes_the_outputs(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    m, G, ks = 100, 2, np.array([3, 5], np.int32)
    sums = torch.full((2, 2, G), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((2, G + 5), -7, dtype=torch.int64, device=DEV)
    slots = torch.full((G,), -7, dtype=torch.int64, device=DEV)
    expo = torch.full((2, m), -7, dtype=torch.int32, device=DEV)
    topk = torch.zeros(1, 5, dtype=torch.int32, device=DEV)
    ptr = torch.zeros(1, dtype=torch.int64, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    info = torch.zeros(m, dtype=torch.int32, device=DEV)
    rc = lib.lgcn_eval_pop_metrics(L.tp(topk), 0, 5, L.tp(ptr), L.tp(idx), L.tp(info), m, G, L.npp(ks), 2, L.tp(sums), L.tp(counts),
                                   L.tp(slots), L.tp(expo), None, L.current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert not sums.any() and not counts.any() and not slots.any() and not expo.any()


@gpu
def test_pop_metrics_refusals_leave_outputs_untouched(pkg):
    L, lib = pkg._lib, pkg._lib.load()
    c, _ = _case(257, 20, 2)
    n, K, m, G = c['n'], c['K'], c['m'], c['G']
    topk, ptr, idx = _dev(c['topk'], np.int32), _dev(c['ptr'], np.int64), _dev(c['items'], np.int32)
    info = _info(pkg, c['pop'], c['groups'])
    sums = torch.full((8, 2, 8), -7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((8, 13), -7, dtype=torch.int64, device=DEV)
    slots = torch.full((8,), -7, dtype=torch.int64, device=DEV)
    expo = torch.full((8, m), -7, dtype=torch.int32, device=DEV)
    per = torch.full((n, 8, 2, 8), -7.0, dtype=torch.float64, device=DEV)

    def call(ks=(20, 5), n_ks=None, n_eval=n, K_=K, m_=m, G_=G, topk_=topk, ptr_=ptr, idx_=idx, info_=info, sums_=sums,
             counts_=counts, slots_=slots, ks_null=False):
        ks = np.asarray(ks, np.int32)
        return lib.lgcn_eval_pop_metrics(L.tp(topk_), n_eval, K_, L.tp(ptr_), L.tp(idx_), L.tp(info_), m_, G_,
                                         None if ks_null else L.npp(ks), len(ks) if n_ks is None else n_ks, L.tp(sums_),
                                         L.tp(counts_), L.tp(slots_), L.tp(expo), L.tp(per), L.current_stream())
    for kw in (dict(G_=0), dict(G_=9), dict(n_ks=0), dict(ks=[1] * 9), dict(ks=[0]), dict(ks=[5, 21]), dict(K_=0),
               dict(K_=257, ks=[257]), dict(n_eval=-1), dict(m_=-1), dict(topk_=None), dict(ptr_=None), dict(idx_=None),
               dict(info_=None), dict(sums_=None), dict(counts_=None), dict(slots_=None), dict(ks_null=True),
               dict(n_eval=1 << 30, K_=256, ks=[256], m_=1 << 24)):
        assert call(**kw) == 3, kw
        assert lib.lgcn_last_error()
    torch.cuda.synchronize()
    assert bool((sums == -7.0).all()) and bool((counts == -7).all()) and bool((slots == -7).all())
    assert bool((expo == -7).all()) and bool((per == -7.0).all())
    # the checked wrapper refuses before any pointer leaves Python
    ev = pkg._lib.eval_pop_metrics
    with pytest.raises(ValueError, match="n_groups"):
        ev(topk, ptr, idx, info, 9, [20])
    with pytest.raises(ValueError, match="cut-offs"):
        ev(topk, ptr, idx, info, 2, [21])
    with pytest.raises(ValueError, match="test_ptr"):
        ev(topk, ptr[:-1], idx, info, 2, [20])
    with pytest.raises(ValueError, match="item_info"):
        ev(topk, ptr, idx, info.to(torch.int64), 2, [20])
    with pytest.raises(ValueError, match="topk"):
        ev(topk.cpu(), ptr, idx, info, 2, [20])
    with pytest.raises(ValueError, match="contiguous"):
        ev(topk.t().contiguous().t(), ptr, idx, info, 2, [20])
    with pytest.raises(ValueError, match="per_slot"):
        ev(topk, ptr, idx, info, 2, [20], per_slot=torch.empty(n, 1, 2, 3, dtype=torch.float64, device=DEV))


@gpu
def test_pop_metrics_group_bits_past_n_groups(pkg):
    """Ordinary input: item words whose group is >= n_groups.  Such an item is in no reported group column; valid entries,
    popularity, exposures, coverage and Gini do not move."""
    c, ref = _case(257, 65, 2)
    rng = np.random.Generator(np.random.PCG64(5))
    wild = dict(c)
    wild['groups'] = np.where(rng.random(c['m']) < 0.5, rng.integers(2, 8, c['m']), c['groups'])
    ref_w = pr.restate(wild['topk'], wild['ptr'], wild['items'], wild['pop'], wild['groups'], 2, wild['ks'])
    info = torch.from_numpy((c['pop'] * 8 + wild['groups']).astype(np.uint32).view(np.int32)).to(DEV)
    got = _run(pkg, wild, info=info)
    _judge(got, ref_w, 257, "group bits past n_groups")
    G = 2
    assert np.array_equal(got['counts'][:, G:], ref['counts'][:, G:]) and np.array_equal(got['exposure'], ref['exposure'])
    assert (got['counts'][:, :G].sum(axis=1) < got['counts'][:, G]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# Procedure.Test
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
def test_procedure_test_pop_metrics(pkg, lastfm, tmp_path):
    g = lastfm
    ds, m = _make_model(pkg, g, tmp_path)
    users, pos, neg = pkg.Procedure.sample_epoch_to_device(ds, DEV)
    m.fused_epoch(users, pos, neg, g.B)
    m.eval()
    w = pkg.world
    old_topks = list(w.topks)
    try:
        w.topks = [5, 20]
        assert w.config['pop_metrics'] == 0
        r_off = pkg.Procedure.Test(ds, m, 0)
        assert sorted(r_off) == ['ndcg', 'precision', 'recall']
        w.config['pop_metrics'] = 1
        r_on = pkg.Procedure.Test(ds, m, 0)
        ev = ds._lgcn_eval_index
        with torch.no_grad():
            _, topk = pkg.Procedure._test_fused(m, ev, 20)
        csv_head = open(os.path.join(w.config['checkpoint_dir'], 'valid_epoch_metrics.csv')).readline().strip()
    finally:
        w.topks = old_topks
        w.config['pop_metrics'] = 0
    new = ['arp', 'coverage', 'gini', 'group_users', 'list_share', 'recall_by_group', 'recall_share']
    assert sorted(r_on) == sorted(new + ['ndcg', 'precision', 'recall'])
    assert csv_head == 'epoch,precision,recall,ndcg'
    for name in ('precision', 'recall', 'ndcg'):
        assert np.asarray(r_on[name]).tobytes() == np.asarray(r_off[name]).tobytes(), name
    eval_users = ev.users.tolist()
    test = [np.sort(np.asarray(ds.testDict[u], np.int64)) for u in eval_users]
    ptr = np.zeros(len(test) + 1, np.int64)
    np.cumsum([len(t) for t in test], out=ptr[1:])
    pop = np.bincount(np.concatenate([np.asarray(ds.allPos[u], np.int64) for u in range(ds.n_users)]), minlength=ds.m_items)
    groups = pkg.utils.popularity_groups(pop, [0.2])
    ref = pr.restate(topk.cpu().numpy(), ptr, np.concatenate(test), pop, groups, 2, [5, 20])
    n = len(test)
    for name in ('list_share', 'arp', 'coverage', 'gini', 'group_users'):
        assert np.array_equal(np.asarray(r_on[name]), ref[name]), (name, r_on[name], ref[name])
    for name in ('recall_share', 'recall_by_group'):
        err = np.abs(np.asarray(r_on[name]) - ref[name])
        print(name, "max rel err:", float((err / np.maximum(ref[name], 1e-300)).max()), "bound", (n + 3) * U)
        assert np.all(err <= (n + 3) * U * ref[name]), name              # (the sum's bound + the division by n or n_g)
        assert np.asarray(r_on[name]).shape == (2, 2)
    assert ref['recall_share'].sum() > 0 and 0 < ref['coverage'][1] <= 1 and 0 < ref['gini'][1] < 1
    total = np.asarray(r_on['recall_share']).sum(axis=0)
    rel = np.abs(total - r_on['recall']) / r_on['recall']
    print("sum_g recall_share vs recall, relative:", rel.tolist(), "bound", 4 * U)
    assert np.all(rel <= 4 * U)

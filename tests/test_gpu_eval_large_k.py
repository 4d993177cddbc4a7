"""Fused evaluation past K = 64 (lgcn_eval_topk_ex / lgcn_eval_metrics_ex, ABI 12): the large-K item sweep against torch in
fp64, the -(1<<10) tail of users with fewer than K unmasked items, bitwise identity with the K <= 64 entry points, the metrics
at large cut-offs against the Python harness and the oracle, Procedure.Test end to end at --topks "[20, 50, 100]", and the
refusals (bad K, too small an output) that launch nothing."""
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import EPS32
from eval_cases import csr as _csr, problem as _problem

DEV = "cuda:0"
gpu = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run_ex(pkg, E, n_users, users, ptr, idx, K, masks=None, flags=0, cap=None):
    L, lib = pkg._lib, pkg._lib.load()
    n = len(users)
    m_items = E.shape[0] - n_users
    topk = torch.full((n, K), -7, dtype=torch.int32, device=DEV)
    sc = torch.full((n, K), 7.0, dtype=torch.float32, device=DEV)
    rc = lib.lgcn_eval_topk_ex(L.tp(E), n_users, m_items, int(E.shape[1]), L.tp(users), n, L.tp(ptr), L.tp(idx),
                               L.tp(masks), K, L.tp(topk), L.tp(sc), n * K if cap is None else cap, flags, L.current_stream())
    torch.cuda.synchronize()
    return rc, topk, sc


def _masks(pkg, users, ptr, idx, m_items):
    L, lib = pkg._lib, pkg._lib.load()
    n = int(users.numel())
    masks = torch.empty(int(lib.lgcn_eval_mask_words(m_items, n)), dtype=torch.int32, device=DEV)
    L.check(lib.lgcn_eval_build_masks(L.tp(users), n, L.tp(ptr), L.tp(idx), m_items, L.tp(masks), L.current_stream()),
            "lgcn_eval_build_masks")
    return masks


def _check_vs_torch(E, n_users, users, rows, topk, sc, K, same_ids=True):
    m_items = E.shape[0] - n_users
    d = E.shape[1]
    exact = E[:n_users][users.long()].double() @ E[n_users:].double().t()        # fp64: no summation order
    for s, u in enumerate(users.tolist()):
        if len(rows[u]):
            exact[s, torch.from_numpy(rows[u]).long().to(DEV)] = -(1 << 10)
    want_sc, want = torch.topk(exact, K)
    got = topk.long()
    assert int(got.min()) >= 0 and int(got.max()) < m_items
    for row in got.cpu().numpy():
        assert len(np.unique(row)) == K
    got_exact = torch.gather(exact, 1, got)
    # fp32 rounding of a d-term dot product in any order, taken twice (as test_eval_topk_every_sweep_form_vs_torch)
    tol = 2.0 * np.sqrt(d) * EPS32 * float(E[:n_users].norm(dim=1).max()) * float(E[n_users:].norm(dim=1).max())
    assert float((got_exact - sc.double()).abs().max()) < tol                    # reported scores are those items' scores
    assert float((got_exact - want_sc).abs().max()) < tol                        # rank by rank the same score
    assert float((got_exact[:, -1] - want_sc[:, -1]).abs().max()) < max(tol, 1e-6)      # the K-th score
    if same_ids:
        assert float((got == want).float().mean()) > 0.999                       # ids differ only inside fp32 ties
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())                                 # descending
    return exact


CASES = [  # (m_items, d): under 4096 items (one part), ~10 000 (parts, 16-bit ids), >= 270 000 (parts with int32 ids)
    (3001, 32), (3001, 256), (10007, 64), (10007, 128), (10007, 256), (270001, 32), (270001, 128), (270001, 256),
]


@gpu
@pytest.mark.parametrize("m_items,d", CASES)
@pytest.mark.parametrize("K", [65, 100, 128, 200, 256])
def test_eval_topk_ex_large_k_vs_torch(pkg, m_items, d, K):
    """Every large-K sweep form against torch matmul + mask + topk in fp64; masks on and off bitwise equal; the split bf16
    product and the fp32 matrix instructions agree up to fp32 ties."""
    n_eval = 97 if m_items > 100000 else 257
    E, users, rows = _problem(m_items, d, n_eval=n_eval, seed=K)
    ptr, idx = _csr(rows)
    Ed, ud, pd, idd = _dev(E), _dev(users), _dev(ptr), _dev(idx)
    rc, topk, sc = _run_ex(pkg, Ed, 300, ud, pd, idd, K)
    assert rc == 0, pkg._lib.load().lgcn_last_error()
    _check_vs_torch(Ed, 300, ud, rows, topk, sc, K)
    masks = _masks(pkg, ud, pd, idd, m_items)
    rc, topk_m, sc_m = _run_ex(pkg, Ed, 300, ud, pd, idd, K, masks=masks)
    assert rc == 0
    assert torch.equal(topk_m, topk) and torch.equal(sc_m, sc)
    rc, topk32, sc32 = _run_ex(pkg, Ed, 300, ud, pd, idd, K, flags=pkg._lib.EVAL_FP32)
    assert rc == 0
    _check_vs_torch(Ed, 300, ud, rows, topk32, sc32, K)
    rc, topk32m, sc32m = _run_ex(pkg, Ed, 300, ud, pd, idd, K, masks=masks, flags=pkg._lib.EVAL_FP32)
    assert rc == 0
    assert torch.equal(topk32m, topk32) and torch.equal(sc32m, sc32)


@gpu
@pytest.mark.parametrize("m_items,K", [(300, 256), (5000, 200), (4100, 128)])
def test_eval_topk_ex_minus_1024_tail(pkg, m_items, K):
    """Users whose train positives cover all but K/2 items: the K/2 unmasked items first, then train positives at -(1<<10)
    (Procedure.py:181 + torch.topk) -- any of them, as they tie exactly at the K-th score, listed in id order."""
    d, n_users = 64, 200
    E, users, rows = _problem(m_items, d, n_users=n_users, n_eval=150, seed=5)
    rng = np.random.Generator(np.random.PCG64(9))
    dense = set()
    for u in range(0, n_users, 3):
        keep = rng.choice(m_items, K // 2, replace=False)
        rows[u] = np.setdiff1d(np.arange(m_items), keep).astype(np.int32)
        dense.add(u)
    ptr, idx = _csr(rows)
    Ed, ud, pd, idd = _dev(E), _dev(users), _dev(ptr), _dev(idx)
    for masks in (None, _masks(pkg, ud, pd, idd, m_items)):
        rc, topk, sc = _run_ex(pkg, Ed, n_users, ud, pd, idd, K, masks=masks)
        assert rc == 0
        _check_vs_torch(Ed, n_users, ud, rows, topk, sc, K, same_ids=False)      # (which positives tie at -1024: unspecified)
        got, scores = topk.cpu().numpy(), sc.cpu().numpy()
        for s, u in enumerate(users.tolist()):
            if u not in dense:
                continue
            free = np.setdiff1d(np.arange(m_items), rows[u])
            assert np.array_equal(np.sort(got[s, :K // 2]), free)                      # every non-positive, above ...
            assert np.all(scores[s, K // 2:] == -1024.0)                               # ... the train positives at -1024
            assert np.all(np.isin(got[s, K // 2:], rows[u]))
            assert np.array_equal(got[s, K // 2:], np.sort(got[s, K // 2:]))           # equal scores: in id order (which ids: unspecified)


@gpu
@pytest.mark.parametrize("m_items,d", [(3001, 32), (10007, 64), (10007, 128), (10007, 256), (70001, 64)])
def test_eval_topk_ex_small_k_is_the_k64_sweep(pkg, m_items, d):
    """K <= 64 through lgcn_eval_topk_ex is bitwise lgcn_eval_topk_masked / lgcn_eval_topk_fp32 (and _ex's metrics are bitwise
    lgcn_eval_metrics)."""
    L, lib = pkg._lib, pkg._lib.load()
    E, users, rows = _problem(m_items, d, n_eval=300, seed=1)
    ptr, idx = _csr(rows)
    Ed, ud, pd, idd = _dev(E), _dev(users), _dev(ptr), _dev(idx)
    n, n_users = len(users), 300
    masks = _masks(pkg, ud, pd, idd, m_items)
    rng = np.random.Generator(np.random.PCG64(3))
    test_rows = [np.sort(rng.choice(m_items, int(rng.integers(0, 30)), replace=False)).astype(np.int32) for _ in range(n)]
    tptr, tidx = _csr(test_rows)
    tpd, tid = _dev(tptr), _dev(tidx)
    for K in (7, 20, 50, 64):
        ref = torch.full((n, K), -7, dtype=torch.int32, device=DEV)
        ref_sc = torch.empty(n, K, dtype=torch.float32, device=DEV)
        L.check(lib.lgcn_eval_topk_masked(L.tp(Ed), n_users, m_items, d, L.tp(ud), n, L.tp(pd), L.tp(idd), K, L.tp(ref),
                                          L.tp(ref_sc), L.tp(masks), L.current_stream()), "masked")
        rc, got, got_sc = _run_ex(pkg, Ed, n_users, ud, pd, idd, K, masks=masks)
        assert rc == 0 and torch.equal(got, ref) and torch.equal(got_sc, ref_sc)
        ref32 = torch.full((n, K), -7, dtype=torch.int32, device=DEV)
        ref32_sc = torch.empty(n, K, dtype=torch.float32, device=DEV)
        L.check(lib.lgcn_eval_topk_fp32(L.tp(Ed), n_users, m_items, d, L.tp(ud), n, L.tp(pd), L.tp(idd), K, L.tp(ref32),
                                        L.tp(ref32_sc), L.current_stream()), "fp32")
        rc, got32, got32_sc = _run_ex(pkg, Ed, n_users, ud, pd, idd, K, flags=L.EVAL_FP32)
        assert rc == 0 and torch.equal(got32, ref32) and torch.equal(got32_sc, ref32_sc)
        ks = [k for k in (K, 1, 5, 20, 50) if k <= K]
        ks_h = torch.tensor(ks, dtype=torch.int32)
        pu = torch.empty(n, 3 * len(ks), dtype=torch.float64, device=DEV)
        sums = torch.empty(3 * len(ks), dtype=torch.float64, device=DEV)
        L.check(lib.lgcn_eval_metrics(L.tp(ref), n, K, L.tp(tpd), L.tp(tid), L.tp(ks_h), len(ks), L.tp(pu), L.tp(sums),
                                      L.current_stream()), "metrics")
        pu_ex, sums_ex = L.eval_metrics(ref, tpd, tid, ks)
        torch.cuda.synchronize()
        assert torch.equal(pu_ex, pu) and torch.equal(sums_ex, sums)


@gpu
@pytest.mark.parametrize("ks", [[20, 50, 100, 256], [256, 20, 100, 50], [100, 1, 256]])
def test_eval_metrics_ex_large_k(pkg, oracle, ks):
    """lgcn_eval_metrics_ex at cut-offs up to 256, in any order, against the harness's formulas in float64 (1e-12),
    Procedure._batch_metrics itself (to its float32 rounding) and oracle.test on the same table (1e-8)."""
    L = pkg._lib
    rng = np.random.Generator(np.random.PCG64(len(ks)))
    n_users, m_items, d, K = 180, 2000, 32, 256
    E = rng.standard_normal((n_users + m_items, d)).astype(np.float32)
    users = np.arange(n_users, dtype=np.int32)
    train = [np.sort(rng.choice(m_items, int(rng.integers(1, 40)), replace=False)).astype(np.int32) for _ in range(n_users)]
    test_dict = {}
    for u in range(n_users):
        rest = np.setdiff1d(np.arange(m_items), train[u])
        test_dict[u] = np.sort(rng.choice(rest, int(rng.integers(1, 30)), replace=False)).tolist()
    ptr, idx = _csr(train)
    Ed, ud, pd, idd = _dev(E), _dev(users), _dev(ptr), _dev(idx)
    topk = torch.empty(n_users, K, dtype=torch.int32, device=DEV)
    L.eval_topk(Ed, n_users, ud, pd, idd, K, topk, fp32=True)
    tptr, tidx = _csr([np.array(test_dict[u], np.int32) for u in range(n_users)])
    pu, sums = L.eval_metrics(topk, _dev(tptr), _dev(tidx), ks)
    pu = pu.cpu().numpy()
    top = topk.cpu().numpy()
    hits = np.array([np.isin(top[s], test_dict[s]) for s in range(n_users)]).astype(np.float64)
    gt_len = np.array([len(test_dict[u]) for u in range(n_users)])
    bm = pkg.Procedure._batch_metrics(hits, gt_len, ks)
    # _batch_metrics divides float32 hit counts (its precision / recall are float32-rounded): the same formulas in float64 beside it
    disc = 1.0 / np.log2(np.arange(2, K + 2))
    f64 = {"precision": np.stack([hits[:, :k].sum(1) / k for k in ks], 1),
           "recall": np.stack([hits[:, :k].sum(1) / gt_len for k in ks], 1),
           "ndcg": np.stack([(hits[:, :k] * disc[:k]).sum(1) / (disc[:k] * (np.arange(k) < np.minimum(k, gt_len)[:, None])).sum(1)
                             for k in ks], 1)}
    nk = len(ks)
    for j, name in enumerate(("precision", "recall", "ndcg")):
        np.testing.assert_allclose(pu[:, j * nk:(j + 1) * nk], f64[name], rtol=0, atol=1e-12)
        np.testing.assert_allclose(pu[:, j * nk:(j + 1) * nk], bm[name], rtol=1e-7, atol=1e-12)
        np.testing.assert_allclose(sums.cpu().numpy()[j * nk:(j + 1) * nk], f64[name].sum(0), rtol=0, atol=1e-9)
    r_indptr = ptr.astype(np.int64)
    for j, k in enumerate(ks):
        ref = oracle.test(E, n_users, r_indptr, idx, test_dict, k)
        for q, name in enumerate(("precision", "recall", "ndcg")):
            assert abs(float(sums[q * nk + j]) / n_users - ref[name]) < 1e-8, (k, name, float(sums[q * nk + j]) / n_users, ref[name])


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
@pytest.mark.parametrize("topks", [[20, 50, 100], [100, 20]])
def test_procedure_test_fused_large_k(pkg, oracle, lastfm, tmp_path, topks, monkeypatch):
    """Procedure.Test at max(topks) = 100 takes the fused path (asserted) and matches the torch harness (1e-9) and the
    oracle (1e-8) at every cut-off."""
    g = lastfm
    ds, m = _make_model(pkg, g, tmp_path)
    users, pos, neg = pkg.Procedure.sample_epoch_to_device(ds, DEV)
    m.fused_epoch(users, pos, neg, g.B)
    m.eval()
    w = pkg.world
    old_topks = list(w.topks)
    calls = []
    real = pkg.Procedure._test_fused

    def spy(*a, **k):
        calls.append(a[2])
        return real(*a, **k)
    monkeypatch.setattr(pkg.Procedure, "_test_fused", spy)
    try:
        w.topks = topks
        w.config['eval_fused'] = 1
        r_fused = pkg.Procedure.Test(ds, m, 0)
        assert calls == [max(topks)]
        w.config['eval_fused'] = 0
        r_torch = pkg.Procedure.Test(ds, m, 0)
        assert calls == [max(topks)]
    finally:
        w.topks = old_topks
        w.config['eval_fused'] = 1
    with torch.no_grad():
        E = m.propagated_table().cpu().numpy()
    for j, k in enumerate(topks):
        ref = oracle.test(E, ds.n_users, ds._r_indptr, ds._r_indices, ds.testDict, k)
        for name in ("precision", "recall", "ndcg"):
            assert abs(float(r_fused[name][j]) - float(r_torch[name][j])) < 1e-9, (k, name, r_fused[name], r_torch[name])
            assert abs(float(r_fused[name][j]) - ref[name]) < 1e-8, (k, name, r_fused[name][j], ref[name])


def test_eval_ex_refusals_c_level(pkg):
    """rc 3, and nothing launched (null pointers suffice: the checks come first), for K > lgcn_eval_kmax(), K > m_items, an
    output smaller than n_eval * K, and unknown flags.  No device needed."""
    L, lib = pkg._lib, pkg._lib.load()
    assert lib.lgcn_eval_kmax() == 256 and L.eval_kmax() == 256
    fake = L._vp(256)                  # never dereferenced: every refusal precedes any launch or device access
    def call(K, m_items=1000, n_eval=10, cap=None, flags=0):
        return lib.lgcn_eval_topk_ex(fake, 50, m_items, 64, fake, n_eval, fake, fake, None, K, fake, None,
                                     n_eval * K if cap is None else cap, flags, None)
    assert call(257) == 3
    assert call(0) == 3
    assert call(200, m_items=150) == 3
    assert call(100, cap=10 * 100 - 1) == 3
    assert call(20, cap=10 * 20 - 1) == 3
    assert call(20, flags=2) == 3
    assert call(100, n_eval=0) == 0                       # nothing to rank: nothing launched, success
    k20, ks = np.array([20], np.int32), np.array([20, 300], np.int32)
    assert lib.lgcn_eval_metrics_ex(fake, 10, 257, fake, fake, L.npp(k20), 1, fake, fake, None) == 3
    assert lib.lgcn_eval_metrics_ex(fake, 10, 256, fake, fake, L.npp(ks), 2, fake, fake, None) == 3     # a cut-off > K
    assert lib.lgcn_eval_metrics_ex(fake, 10, 256, fake, fake, L.npp(ks), 0, fake, fake, None) == 3     # no cut-off


@gpu
def test_eval_ex_refusals_wrapper(pkg):
    """The Python wrappers raise ValueError before launching: wrong output shape, dtype, contiguity, K out of range."""
    L = pkg._lib
    n_users, m_items, d, n, K = 50, 500, 32, 10, 100
    E = torch.zeros(n_users + m_items, d, dtype=torch.float32, device=DEV)
    users = torch.arange(n, dtype=torch.int32, device=DEV)
    ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    for bad in (torch.empty(n, K - 1, dtype=torch.int32, device=DEV),
                torch.empty(n, K, dtype=torch.int64, device=DEV),
                torch.empty(K, n, dtype=torch.int32, device=DEV).t(),
                torch.empty(n, K, dtype=torch.int32)):
        with pytest.raises(ValueError):
            L.eval_topk(E, n_users, users, ptr, idx, K, bad)
    out = torch.empty(n, 257, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        L.eval_topk(E, n_users, users, ptr, idx, 257, out)
    with pytest.raises(ValueError):
        L.eval_topk(E[:n_users + 99], n_users, users, ptr, idx, K, torch.empty(n, K, dtype=torch.int32, device=DEV))   # K > m_items
    with pytest.raises(ValueError):
        L.eval_topk(E, n_users, users, ptr, idx, K, torch.empty(n, K, dtype=torch.int32, device=DEV),
                    out_scores=torch.empty(n, K, dtype=torch.float64, device=DEV))
    topk = torch.zeros(n, K, dtype=torch.int32, device=DEV)
    tptr = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        L.eval_metrics(topk, tptr, idx, [20, 101])
    with pytest.raises(ValueError):
        L.eval_metrics(topk, tptr[:-1], idx, [20])
    with pytest.raises(ValueError):
        L.eval_metrics(topk.t(), tptr, idx, [5])

"""The item-item graph builder on the GPU (lgcn_i2i_topk / lgcn_i2i_finish, ABI 13; -m gpu) against the reference's recorded
matrices (tests/golden/*/i2i_*.npz) and the numpy restatement of its semantics (tests/i2i_restatement.py, pinned to the same
fixtures by tests/test_i2i_restatement.py).

cooc / jaccard: exact arithmetic on both sides (integers; one IEEE division), so lists and structure must be equal exactly.
pmi: the device log is not libm's.  A row may differ from the restatement only in entries whose restated fp64 weight is within
4 fp64 ulp of that row's cut weight (the restated weight at rank topk): every entry the GPU admitted that the restatement cut,
and every entry it cut that the restatement kept, is checked against the cut weight itself.  The order INSIDE the list is held
position by position to the same 4 ulp (the GPU's entry at rank t against the restated weight at rank t), which a chain of
near-ties could not stretch: each position is compared with the restatement's own weight there, not with its neighbour.  At
most 0.1 % of a case's rows may use the allowance.  Values of the final matrix: within
(n_i + n_j + 16) 2^-24 |ref| (i2i_restatement.value_bound)."""
import ctypes as C
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import i2i_restatement as R                     # noqa: E402
from conftest import GOLDEN                     # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS_CAP = 3072            # neighbour bound up to which a row uses the LDS accumulator (csrc/lgcn_i2i.hip)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to(DEV)


def gpu_topk(pkg, indptr, indices, n_items, topk, weight, min_basket=1):
    cols, w, length = pkg._lib.i2i_topk(_dev(indptr, np.int64), _dev(indices, np.int32), n_items, topk, weight, min_basket)
    return cols, w, length


def check_lists(r, cols, w, length, items, weight, topk, what):
    """GPU lists (numpy) of `items` against the restatement, rank order included.  Returns the rows that needed the pmi allowance."""
    used = 0
    for i in items:
        j, w64, _ = r.row(int(i), weight)
        k = min(topk, len(j))
        assert int(length[i]) == k, (what, i, int(length[i]), k)
        g = cols[i, :k].astype(np.int64)
        assert (cols[i, k:] == -1).all() and (w[i, k:] == 0).all(), (what, i, "padding")
        if weight != "pmi":
            assert np.array_equal(g, j[:k]), (what, i, g[:8], j[:8])
            assert np.array_equal(w[i, :k], w64[:k].astype(np.float32)), (what, i)
            continue
        if not np.array_equal(g, j[:k]):
            used += 1
            pos = {int(c): t for t, c in enumerate(j)}
            assert len(set(g.tolist())) == k and all(int(c) in pos for c in g), (what, i, "not neighbours")
            wg = np.asarray([w64[pos[int(c)]] for c in g])
            ulp = np.spacing(np.maximum(np.abs(w64[:k]), np.abs(wg)))
            assert (np.abs(wg - w64[:k]) <= 4 * ulp).all(), (what, i, "differs beyond 4 ulp of a near-tie")
            cut = w64[k - 1]                                   # the row's cut weight: what was swapped across the cut lies within 4 ulp of it
            kept = set(j[:k].tolist())
            swapped = [w64[pos[int(c)]] for c in g if int(c) not in kept] + [w64[t] for t in range(k) if int(j[t]) not in set(g.tolist())]
            assert all(abs(x - cut) <= 4 * np.spacing(max(abs(x), abs(cut))) for x in swapped), (what, i, "beyond 4 ulp of the cut weight")
        np.testing.assert_allclose(w[i, :k], w64[:k].astype(np.float32), rtol=3e-7, atol=0, err_msg=f"{what} {i}")
    return used


def finish_of(cols, w, length, n_items):
    """scipy's maximum / row sums / scaling over the GPU's own lists."""
    k = cols.shape[1]
    m = np.arange(k)[None, :] < length[:, None]
    rows = np.repeat(np.arange(n_items), length)
    return R.finish(rows, cols[m], w[m], n_items)


def gpu_finish(pkg, cols, w, length, n_items):
    ip, ix, v, nnz = pkg._lib.i2i_finish(cols, w, length)
    return R.Csr(ip.cpu().numpy(), ix[:nnz].cpu().numpy(), v[:nnz].cpu().numpy()), nnz


# ---- 1. fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,weight,topk,min_basket", R.FIXTURES, ids=lambda v: str(v))
def test_build_item_item_matches_reference_fixture(pkg, name, weight, topk, min_basket):
    z = np.load(R.fixture_path(GOLDEN, name, weight, topk, min_basket))
    train = os.path.join(GOLDEN, name, "train.txt")
    n_items = int(z["n_items"])
    what = f"{name} {weight} topk={topk} min_basket={min_basket}"
    m = pkg.preprocess_instacart_i2i.build_item_item(train, n_items=n_items, topk=topk, weight=weight, min_basket=min_basket)
    assert m.shape == (n_items, n_items) and m.data.dtype == np.float32 and m.indices.dtype == np.int32
    ref = R.Csr(z["indptr"], z["indices"], z["data"])
    if weight != "pmi":
        R.assert_csr_close(m, ref, what)
        return
    indptr, indices = R.baskets_csr(R.read_baskets(train))
    cols, w, length = gpu_topk(pkg, indptr, indices, n_items, topk, weight, min_basket)
    cols, w, length = cols.cpu().numpy(), w.cpu().numpy(), length.cpu().numpy()
    used = check_lists(R.Restatement(indptr, indices, n_items, min_basket), cols, w, length, range(n_items), weight, topk, what)
    print(f"[i2i] {what}: rows using the pmi near-tie allowance: {used} of {n_items}")
    assert used <= 0.001 * n_items
    R.assert_csr_close(m, ref if used == 0 else finish_of(cols, w, length, n_items), what)


# ---- 2. the first stage alone, on data made for the boundaries -------------------------------------------------------------
def directed_baskets():
    """Hub item 0 in every basket (more distinct neighbours than the LDS form holds); three long baskets (3072, 3073, 3074 items,
    unsorted) whose private items have neighbour bounds LDS_CAP - 1, LDS_CAP, LDS_CAP + 1; short random baskets; baskets of one
    item; an item that co-occurs with nothing (12000) and items in no basket (>= 12001; n_items = 12500)."""
    rng = np.random.Generator(np.random.PCG64(13))
    baskets, nxt = [], 2000
    for size in (LDS_CAP, LDS_CAP + 1, LDS_CAP + 2):
        b = np.concatenate([[0], np.arange(nxt, nxt + size - 1)])
        nxt += size - 1
        baskets.append(rng.permutation(b))
    for _ in range(400):
        b = np.concatenate([[0], rng.choice(np.arange(1, 2000), size=int(rng.integers(1, 12)), replace=False)])
        baskets.append(rng.permutation(b))
    baskets += [np.array([12000]), np.array([0]), np.array([7]), np.array([8, 9]), np.array([9, 8])]
    order = rng.permutation(len(baskets))
    baskets = [baskets[t] for t in order]
    assert nxt < 12000
    return baskets, 12500


@pytest.mark.parametrize("weight,min_basket", [("cooc", 1), ("jaccard", 1), ("pmi", 1), ("cooc", 0), ("jaccard", 3), ("cooc", 2)])
def test_topk_stage_on_directed_baskets(pkg, weight, min_basket):
    baskets, n_items = directed_baskets()
    indptr, indices = R.baskets_csr(baskets)
    r = R.Restatement(indptr, indices, n_items, min_basket)
    assert r.work[0] > LDS_CAP and max(len(b) for b in baskets) >= 1024
    bounds = sorted(set(r.work[2000:12000].tolist()))
    assert {LDS_CAP - 1, LDS_CAP, LDS_CAP + 1} <= set(bounds)                      # the bin boundary and both neighbours
    topk = 20
    cols, w, length = gpu_topk(pkg, indptr, indices, n_items, topk, weight, min_basket)
    cols, w, length = cols.cpu().numpy(), w.cpu().numpy(), length.cpu().numpy()
    rng = np.random.Generator(np.random.PCG64(5))
    special = [0, 7, 8, 9, 12000, 12001, 12499, 1999, 2000]
    for b in (LDS_CAP - 1, LDS_CAP, LDS_CAP + 1):
        special += np.flatnonzero(r.work == b)[:3].tolist()
    items = special + rng.choice(n_items, 400, replace=False).tolist()
    used = check_lists(r, cols, w, length, items, weight, topk, f"directed {weight} mb={min_basket}")
    print(f"[i2i] directed {weight} mb={min_basket}: rows using the pmi near-tie allowance: {used} of {len(items)}")
    assert used <= 0.001 * len(items)
    assert length[12000] == 0 and length[12001:].max() == 0 and (cols[12000:] == -1).all()
    empty = np.flatnonzero(r.deg == 0)
    assert (length[empty] == 0).all()
    # both stages: empty rows get degree 1, the matrix is the restatement's
    got, nnz = gpu_finish(pkg, torch.from_numpy(cols).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(length).to(DEV), n_items)
    R.assert_csr_close(got, finish_of(cols, w, length, n_items), f"directed finish {weight} mb={min_basket}")


def plane_baskets(p=11):
    """The lines of the affine plane over Z_p as baskets: every pair of the p*p items shares exactly ONE basket, so every count is 1
    and every cut is decided by the first basket, then the column.  Basket order and the order inside a basket are shuffled."""
    rng = np.random.Generator(np.random.PCG64(3))
    lines = [np.array([x * p + (m * x + c) % p for x in range(p)]) for m in range(p) for c in range(p)]
    lines += [np.array([x * p + y for y in range(p)]) for x in range(p)]
    return [rng.permutation(lines[t]) for t in rng.permutation(len(lines))], p * p + 9      # n_items above the largest id


@pytest.mark.parametrize("weight", R.WEIGHTS)
@pytest.mark.parametrize("topk", [7, 256])
def test_topk_stage_when_every_count_is_one(pkg, weight, topk):
    baskets, n_items = plane_baskets()
    indptr, indices = R.baskets_csr(baskets)
    r = R.Restatement(indptr, indices, n_items)
    j, w64, first = r.row(17, "cooc")
    assert len(j) == 120 and (w64 == 1.0).all() and len(set(first.tolist())) == 12
    cols, w, length = gpu_topk(pkg, indptr, indices, n_items, topk, weight)
    cols, w, length = cols.cpu().numpy(), w.cpu().numpy(), length.cpu().numpy()
    assert check_lists(r, cols, w, length, range(n_items), weight, topk, f"plane {weight} {topk}") == 0    # equal weights: exact ties
    assert (length[:121] == min(topk, 120)).all() and (length[121:] == 0).all()                # topk = 256 exceeds every row


# ---- 3. Gowalla ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gowalla():
    z = np.load(os.path.join(GOLDEN, "gowalla", "gowalla.npz"))
    indptr, indices = z["train_ptr"].astype(np.int64), z["train_items"].astype(np.int32)
    n_items = int(max(indices.max(), z["test_items"].max())) + 1
    return indptr, indices, n_items, R.Restatement(indptr, indices, n_items)


@pytest.mark.parametrize("weight", R.WEIGHTS)
def test_gowalla_both_stages(pkg, gowalla, weight):
    indptr, indices, n_items, r = gowalla
    topk = 50
    c_d, w_d, l_d = gpu_topk(pkg, indptr, indices, n_items, topk, weight)
    cols, w, length = c_d.cpu().numpy(), w_d.cpu().numpy(), l_d.cpu().numpy()
    rng = np.random.Generator(np.random.PCG64(2020))
    by_work = np.argsort(r.work, kind="stable")
    cut = int(np.searchsorted(r.work[by_work], LDS_CAP, side="right"))
    assert 32 <= cut <= n_items - 32                                               # both accumulator forms run on this data
    items = np.concatenate([rng.choice(n_items, 512, replace=False), by_work[-64:], by_work[cut - 32:cut + 32]])
    used = check_lists(r, cols, w, length, items, weight, topk, f"gowalla {weight}")
    print(f"[i2i] gowalla {weight}: rows using the pmi near-tie allowance: {used} of {len(items)}; rows in the dense form: {n_items - cut}")
    assert used <= 0.001 * len(items)
    got, nnz = gpu_finish(pkg, c_d, w_d, l_d, n_items)
    assert nnz <= 2 * int(length.sum())
    R.assert_csr_close(got, finish_of(cols, w, length, n_items), f"gowalla finish {weight}")
    # the whole build again: bitwise identical
    c2, w2, l2 = gpu_topk(pkg, indptr, indices, n_items, topk, weight)
    assert torch.equal(c2, c_d) and torch.equal(w2.view(torch.int32), w_d.view(torch.int32)) and torch.equal(l2, l_d)
    got2, nnz2 = gpu_finish(pkg, c2, w2, l2, n_items)
    assert nnz2 == nnz and np.array_equal(got2.indptr, got.indptr) and np.array_equal(got2.indices, got.indices)
    assert np.array_equal(got2.data.view(np.int32), got.data.view(np.int32))


# ---- 4. the model hook -------------------------------------------------------------------------------------------------------
def test_model_builds_the_graph_it_was_not_given(pkg, tiny, tmp_path):
    gz = np.load(os.path.join(tiny.dir, "golden_i2i.npz"))
    meta = json.load(open(os.path.join(tiny.dir, "golden_i2i.json")))
    d = os.path.join(str(tmp_path), "tiny")
    os.makedirs(d)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(tiny.dir, f), os.path.join(d, f))
    w = pkg.world
    base = ['--layer', str(meta["K"]), '--recdim', str(meta["d"]), '--bpr_batch', str(meta["B"]), '--decay', str(meta["decay"]),
            '--lr', str(meta["lr"]), '--tensorboard', '0', '--dataset', 'tiny', '--use_item_item', '--i2i_alpha', '0.3']

    def run(extra):
        w.configure(base + extra)
        w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
        ds = pkg.dataloader.Loader(w.config, path=d)
        pkg.utils.set_seed(meta["seed"])
        m = pkg.model.LightGCN(w.config, ds).to(DEV)
        m.train()
        return m, ds

    m, ds = run(['--i2i_build', 'jaccard', '--i2i_topk', '5'])
    z = np.load(R.fixture_path(GOLDEN, "tiny", "jaccard", 5))
    assert m.i2i_active and m._i2i.shape == (ds.m_items, ds.m_items)
    R.assert_csr_close(m._i2i, R.Csr(z["indptr"], z["indices"], z["data"]), "model._i2i")
    out = pkg.preprocess_instacart_i2i.main(['--data_root', d, '--weight', 'jaccard', '--topk', '5', '--out', 'i2i_cli.npz'])
    b = gz["batches"]

    def steps(model):
        bpr = pkg.utils.BPRLoss(model, w.config)
        losses = [bpr.stageOne(*(torch.from_numpy(b[t + 1, c]).to(DEV) for c in range(3))) for t in range(3)]
        model.check_device_errors()
        return np.asarray([float(l) for l in losses], np.float64), {k: v.cpu().numpy() for k, v in model.state_dict().items()}
    l1, p1 = steps(m)
    m2, _ = run(['--i2i_path', out])
    assert m2.i2i_active and np.array_equal(m2._i2i.indices, m._i2i.indices) and np.array_equal(m2._i2i.data.view(np.int32), m._i2i.data.view(np.int32))
    l2, p2 = steps(m2)
    assert np.array_equal(l1.view(np.int64), l2.view(np.int64)), (l1, l2)
    for k in p1:
        assert p1[k].tobytes() == p2[k].tobytes(), k
    assert np.isfinite(l1).all() and l1[0] != l1[2]
    m3, _ = run([])                                                                # --i2i_build none, no path: the branch stays off
    assert m3._i2i is None and not m3.i2i_active
    w.configure([])


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(pkg):
    L = pkg._lib
    lib = L.load()
    st = L.current_stream()
    baskets = [np.array([0, 1, 2]), np.array([2, 3]), np.array([1, 3, 4, 5])]
    indptr, indices = R.baskets_csr(baskets)
    m_items, topk = 6, 4
    ip, ix = _dev(indptr, np.int64), _dev(indices, np.int32)
    cols = torch.full((m_items, topk), 77, dtype=torch.int32, device=DEV)
    w = torch.full((m_items, topk), 7.5, dtype=torch.float32, device=DEV)
    length = torch.full((m_items,), 77, dtype=torch.int32, device=DEV)

    def topk_rc(ip_=ip, ix_=ix, nb=3, nnz=9, m=m_items, k=topk, wt=0, mb=1):
        return lib.lgcn_i2i_topk(L.tp(ip_), L.tp(ix_), nb, nnz, m, k, wt, mb, L.tp(cols), L.tp(w), L.tp(length), st)

    def untouched():
        torch.cuda.synchronize()
        return bool((cols == 77).all()) and bool((w == 7.5).all()) and bool((length == 77).all())
    for kw in ({"k": 0}, {"k": 257}, {"wt": 3}, {"wt": -1}, {"mb": -1}, {"nb": 0}, {"nnz": 0}, {"m": 0}, {"nb": -2},
               {"m": 2 ** 23, "k": 256}):                                          # 2 m_items topk past 2^31
        assert topk_rc(**kw) == 3, kw
        assert lib.lgcn_last_error()
    assert untouched()
    for bad in (6, -1):                                                            # an item id outside [0, m_items)
        ixb = indices.copy(); ixb[4] = bad
        assert topk_rc(ix_=_dev(ixb, np.int32)) == 5 and untouched()
    assert topk_rc(m=5) == 5 and untouched()                                       # id 5 with m_items 5
    ipb = indptr.copy(); ipb[1], ipb[2] = 5, 3
    assert topk_rc(ip_=_dev(ipb, np.int64)) == 6 and untouched()                   # offsets not ascending
    assert topk_rc(nnz=8) == 6 and untouched()                                     # indptr[n] != nnz
    with pytest.raises(L.LgcnError, match="item id"):
        L.i2i_topk(ip, _dev(np.where(indices == 5, 9, indices), np.int32), m_items, topk, cols=cols, w=w, length=length)
    assert untouched()
    assert topk_rc() == 0 and not untouched()
    r = R.Restatement(indptr, indices, m_items)
    check_lists(r, cols.cpu().numpy(), w.cpu().numpy(), length.cpu().numpy(), range(m_items), "cooc", topk, "small")
    total = int(length.sum())
    # finish
    op = torch.full((m_items + 1,), 55, dtype=torch.int32, device=DEV)
    oi = torch.full((2 * total,), 55, dtype=torch.int32, device=DEV)
    ov = torch.full((2 * total,), 5.5, dtype=torch.float32, device=DEV)
    nnz = C.c_int64(-9)

    def fin_rc(m=m_items, k=topk, cap=2 * total):
        return lib.lgcn_i2i_finish(L.tp(cols), L.tp(w), L.tp(length), m, k, cap, L.tp(op), L.tp(oi), L.tp(ov), C.byref(nnz), st)

    def fin_untouched():
        torch.cuda.synchronize()
        return bool((op == 55).all()) and bool((oi == 55).all()) and bool((ov == 5.5).all()) and nnz.value == -9
    for kw in ({"k": 0}, {"k": 257}, {"m": 0}, {"cap": 0}, {"cap": -4}):
        assert fin_rc(**kw) == 3 and fin_untouched(), kw
    assert fin_rc(cap=2 * total - 1) == 7 and fin_untouched()
    with pytest.raises(L.LgcnError, match="capacity"):
        L.i2i_finish(cols, w, length, capacity=2 * total - 1, indptr=op, indices=oi[:2 * total - 1].clone(), vals=ov[:2 * total - 1].clone())
    assert fin_untouched()
    assert fin_rc() == 0 and 0 < nnz.value <= 2 * total
    ref = finish_of(cols.cpu().numpy(), w.cpu().numpy(), length.cpu().numpy(), m_items)
    R.assert_csr_close(R.Csr(op.cpu().numpy(), oi[:nnz.value].cpu().numpy(), ov[:nnz.value].cpu().numpy()), ref, "small finish")
    # the wrappers' own checks, on the device
    for bad in (dict(cols=cols[:, :3]), dict(w=w.double()), dict(length=length[:5]), dict(cols=cols.t().contiguous().t())):
        args = dict(cols=cols, w=w, length=length)
        args.update(bad)
        with pytest.raises(ValueError):
            L.i2i_topk(ip, ix, m_items, topk, **args)
    with pytest.raises(ValueError):
        L.i2i_topk(ip, ix.to(torch.int64), m_items, topk)
    with pytest.raises(ValueError):
        L.i2i_finish(cols, w[:, :3], length)
    with pytest.raises(ValueError):
        L.i2i_finish(cols, w, length, capacity=0)
    with pytest.raises(ValueError):
        L.i2i_finish(cols, w, length, indices=oi[:5])
    with pytest.raises(ValueError, match="weight"):
        pkg.preprocess_instacart_i2i.build_from_csr(indptr, indices, m_items, weight="cosine")

"""The fold of the gradient-row conversion into the batch-row launch (lgcn_ctx_set_fold_g32).

lgcn_train_epoch computes, for all steps of the call at once, how many slots of each batch name each destination row
(lgcn_slot_multiplicity); k_triplet / k_triplet_dense then write the fp32 copy of a gradient row themselves and the step
launches no k_g32.  Two contracts:

 * the multiplicities equal a numpy restatement (np.unique per batch, with slot_row's validity rule);
 * the folded step is the unfolded one BIT FOR BIT (integer sums and the identical conversion): losses, the embedding table
   and Adam's moments are compared with torch.equal, never with a tolerance.

The graph is synthetic: 300 users x 200 items, about 3 000 interactions, so batches of 64 hold rows named once and rows named
several times, and batches of 256 hold mostly shared rows."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_USERS, M_ITEMS = 300, 200
N = N_USERS + M_ITEMS


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


# ---- multiplicities ---------------------------------------------------------------------------------------------------------
def _mult_ref(u, p, n, B, n_users, n_rows):
    """numpy restatement: per batch, np.unique counts of the destination rows of the slots of valid triplets; 0 for the rest"""
    T = len(u)
    out = np.zeros(3 * T, np.int64)
    for t0 in range(0, T, B):
        uu, pp, nn = (x[t0:t0 + B].astype(np.int64) for x in (u, p, n))
        b = len(uu)
        ok = (uu >= 0) & (uu < n_users) & (pp >= 0) & (pp + n_users < n_rows) & (nn >= 0) & (nn + n_users < n_rows)
        rows = np.concatenate([uu, pp + n_users, nn + n_users])
        valid = np.tile(ok, 3)
        _, inv, cnt = np.unique(rows[valid], return_inverse=True, return_counts=True)
        m = np.zeros(3 * b, np.int64)
        m[valid] = cnt[inv]
        out[3 * t0:3 * t0 + 3 * b] = m
    return out


def _mult_gpu(pkg, u, p, n, B, n_users, n_rows):
    L = pkg._lib
    U, P, Nn = (_dev(x, torch.int32) for x in (u, p, n))
    out = torch.full((3 * len(u),), -1, dtype=torch.int16, device=DEV)
    rc = L.load().lgcn_slot_multiplicity(L.tp(U), L.tp(P), L.tp(Nn), len(u), B, n_users, n_rows, L.tp(out), L.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy().view(np.uint16).astype(np.int64)


def _mult_batches(B=64):
    """six batches: all rows distinct | one user in every triplet | 5 items in total | one out-of-range id | random | short"""
    rng = np.random.Generator(np.random.PCG64(5))
    ar = np.arange(B)
    bs = [(ar, ar, ar + B),
          (np.full(B, 7), rng.integers(0, M_ITEMS, B), rng.integers(0, M_ITEMS, B)),
          (rng.integers(0, N_USERS, B), rng.integers(0, 5, B), rng.integers(0, 5, B))]
    u, p, n = rng.integers(0, N_USERS, B), rng.integers(0, M_ITEMS, B), rng.integers(0, M_ITEMS, B)
    u[3], p[3], n[3] = u[9], M_ITEMS, n[9]             # triplet 3 is void: its in-range ids must not count for triplet 9's rows
    p[11] = -1
    bs.append((u, p, n))
    bs.append((rng.integers(0, N_USERS, B), rng.integers(0, M_ITEMS, B), rng.integers(0, M_ITEMS, B)))
    bs.append((rng.integers(0, N_USERS, 17), rng.integers(0, M_ITEMS, 17), rng.integers(0, M_ITEMS, 17)))
    return tuple(np.concatenate([b[i] for b in bs]).astype(np.int32) for i in range(3))


@pytest.mark.parametrize("segment", [None, "4", "1"])
def test_multiplicities_vs_numpy(pkg, monkeypatch, segment):
    """the six batches of _mult_batches in one call, with the default segment (one launch) and with segments of 4 steps and of
    1 step (several launches into the one output)"""
    if segment is None:
        monkeypatch.delenv("LGCN_FOLD_SEGMENT", raising=False)
    else:
        monkeypatch.setenv("LGCN_FOLD_SEGMENT", segment)
    u, p, n = _mult_batches()
    want = _mult_ref(u, p, n, 64, N_USERS, N)
    assert (want[:3 * 64] == 1).all() and (want[3 * 64:4 * 64] == 64).all() and want[6 * 64 + 64:6 * 64 + 192].min() >= 2
    assert (want[9 * 64 + np.array([3, 64 + 3, 128 + 3, 11, 64 + 11, 128 + 11])] == 0).all()
    rc, got = _mult_gpu(pkg, u, p, n, 64, N_USERS, N)
    assert rc == 0, pkg._lib.load().lgcn_last_error()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()


def test_multiplicities_large_batches(pkg, monkeypatch):
    """B = 2048 (the headline batch; 8 192 hash slots) on 1 000 users x 700 items and B = 4096, the largest batch that fits,
    on ids wide enough that most rows are distinct (12 288 keys in 16 384 slots); B = 4097 is refused"""
    monkeypatch.delenv("LGCN_FOLD_SEGMENT", raising=False)
    rng = np.random.Generator(np.random.PCG64(6))
    for B, T, nu, mi in ((2048, 2 * 2048 + 100, 1000, 700), (4096, 4096 + 5, 200000, 300000)):
        u, p, n = (rng.integers(0, hi, T).astype(np.int32) for hi in (nu, mi, mi))
        rc, got = _mult_gpu(pkg, u, p, n, B, nu, nu + mi)
        assert rc == 0, pkg._lib.load().lgcn_last_error()
        assert np.array_equal(got, _mult_ref(u, p, n, B, nu, nu + mi)), B
    rc, _ = _mult_gpu(pkg, u, p, n, 4097, nu, nu + mi)
    assert rc == 3 and b"do not fit" in pkg._lib.load().lgcn_last_error()


# ---- the fold, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph_dir(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("foldgraph")), "foldgraph")
    os.makedirs(path)
    rng = np.random.Generator(np.random.PCG64(4321))
    total = 0
    with open(os.path.join(path, "train.txt"), "w") as f, open(os.path.join(path, "test.txt"), "w") as ft:
        for u in range(N_USERS):
            k = 60 if u == 0 else int(rng.integers(1, 19))
            items = np.sort(rng.choice(M_ITEMS - 1, size=k, replace=False))
            total += k
            f.write(f"{u} " + " ".join(map(str, items.tolist())) + "\n")
            ft.write(f"{u} {M_ITEMS - 1}\n")
    assert 2500 <= total <= 3500
    return path


def _model(pkg, path, K, d, act, dense_last, B, fold, flags=(), extra=None):
    w = pkg.world
    w.configure(["--dataset", "foldgraph", "--tensorboard", "0", "--layer", str(K), "--recdim", str(d), "--bpr_batch", str(B),
                 "--act_dtype", act] + list(flags))
    w.config.update({'dense_last': str(dense_last), 'row_order': 'rcm', 'fold_g32': fold})
    if extra:
        w.config.update(extra)
    w.config['checkpoint_dir'] = os.path.join(os.path.dirname(path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=path)
    pkg.utils.set_seed(11)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    m.train()
    assert (ds.n_users, ds.m_items) == (N_USERS, M_ITEMS)
    return m


def _triplets(B, seed, one_user=False):
    """5 batches of B and one of 37: T is no multiple of B.  one_user: user 7 fills every triplet of batch 2 (the longest ticket
    chain a batch can have: multiplicity B)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = 5 * B + 37
    u, p, n = rng.integers(0, N_USERS, T), rng.integers(0, M_ITEMS, T), rng.integers(0, M_ITEMS, T)
    n[5] = p[5]                                        # a triplet whose positive and negative are one row
    if one_user:
        u[2 * B:3 * B] = 7
    return tuple(_dev(x, torch.int32) for x in (u, p, n))


def _state(m):
    st = m._dev
    torch.cuda.synchronize()
    return m._table.detach().clone(), st['adam_m'].clone(), st['adam_v'].clone()


def _clean(pkg, m):
    """after the last step: G64 all zero, the arrival tickets all zero"""
    arr = np.full(N, -1, np.int32)
    pkg._lib.check(pkg._lib.load().lgcn_ctx_copy_arrivals(m._dev['ctx'], arr.ctypes.data_as(C.c_void_p), N), "arrivals")
    assert not arr.any() and not bool(m._dev['G64'].any())


def _on_off(pkg, path, K, d, act, dense_last, B, flags=(), extra=None, one_user=False, seed=1, bad=False):
    lib = pkg._lib.load()
    U, P, Nn = _triplets(B, seed, one_user)
    if bad:
        P = P.clone()
        P[B + 2] = M_ITEMS                             # one void triplet in batch 1
    out = []
    for fold in (1, 0):
        m = _model(pkg, path, K, d, act, dense_last, B, fold, flags, extra)
        init = m._table.detach().clone()
        losses = m.fused_epoch(U, P, Nn, B)
        assert losses.shape == (6, 3)
        assert lib.lgcn_ctx_hub_rows(m._dev['ctx']) == 0
        assert lib.lgcn_ctx_folded_steps(m._dev['ctx']) == (6 if fold else 0)
        out.append((losses.clone(),) + _state(m))
        _clean(pkg, m)
        if bad:
            with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
                m.check_device_errors()
        else:
            m.check_device_errors()
    for name, a, b in zip(("losses", "table", "adam_m", "adam_v"), out[0], out[1]):
        assert torch.equal(a, b), (name, int((a != b).sum()))
    assert torch.isfinite(out[0][0]).all() and not torch.equal(out[0][1], init)          # ... and the steps did train


def _cases():
    """every (d, K, storage, dense_last) the step accepts; the batch size alternates so that each value of each axis meets
    both B = 64 and B = 256"""
    out = []
    for d in (32, 64, 128):
        for K in (1, 2, 3):
            for ai, act in enumerate(("fp32", "bf16", "fp8")):
                if act == "fp8" and d < 64:
                    continue
                for dl in (0, 1):
                    B = 256 if (d // 32 + K + ai + dl) % 2 else 64
                    out.append(pytest.param(d, K, act, dl, B, id=f"d{d}-K{K}-{act}-dl{dl}-B{B}"))
    return out


@pytest.mark.parametrize("d,K,act,dense_last,B", _cases())
def test_fold_is_bitwise_the_unfolded_epoch(pkg, graph_dir, monkeypatch, d, K, act, dense_last, B):
    """6 steps of fused_epoch with the fold on and off from one seed: losses, table, Adam's m and v torch.equal; G64 and the
    arrival tickets zero afterwards; the fold engaged in all 6 steps of the one and in none of the other"""
    monkeypatch.delenv("LGCN_FOLD_SEGMENT", raising=False)
    _on_off(pkg, graph_dir, K, d, act, dense_last, B, seed=d + K)


@pytest.mark.parametrize("what", ["layer_weights", "dropout", "reg_ego", "one_user", "one_user_dense", "segments", "bad_id"])
def test_fold_special_cases(pkg, graph_dir, monkeypatch, what):
    """K = 3, d = 64: layer weights (G32 unscaled), edge dropout (the DROP instantiation), reg_ego (slot counts), a batch one
    user fills (multiplicity B = 64 / 256: the longest ticket chain) in both batch-row kernels, a call that spans two
    multiplicity segments, and a void triplet (its slots have multiplicity 0 and must neither store nor take a ticket)"""
    monkeypatch.delenv("LGCN_FOLD_SEGMENT", raising=False)
    if what == "layer_weights":
        _on_off(pkg, graph_dir, 3, 64, "bf16", 0, 64, flags=["--layer_weights", "[0.4,0.3,0.2,0.1]"])
    elif what == "dropout":
        _on_off(pkg, graph_dir, 3, 64, "fp32", 0, 64, flags=["--dropout", "1", "--keepprob", "0.7"])
    elif what == "reg_ego":
        _on_off(pkg, graph_dir, 3, 64, "fp32", 0, 256, extra={'reg_rows': 'ego'})
    elif what == "one_user":
        _on_off(pkg, graph_dir, 3, 64, "bf16", 0, 256, one_user=True)
    elif what == "one_user_dense":
        _on_off(pkg, graph_dir, 2, 32, "fp32", 1, 64, one_user=True)
    elif what == "segments":
        monkeypatch.setenv("LGCN_FOLD_SEGMENT", "4")
        _on_off(pkg, graph_dir, 3, 64, "bf16", 0, 64)
    else:
        _on_off(pkg, graph_dir, 3, 64, "fp32", 0, 64, bad=True)


def test_per_step_call_is_untouched(pkg, graph_dir):
    """fused_step (lgcn_train_step) never folds: the switch changes nothing and no step is counted"""
    lib = pkg._lib.load()
    U, P, Nn = _triplets(64, 3)
    out = []
    for fold in (1, 0):
        m = _model(pkg, graph_dir, 3, 64, "bf16", 0, 64, fold)
        ls = [m.fused_step(U[i * 64:(i + 1) * 64], P[i * 64:(i + 1) * 64], Nn[i * 64:(i + 1) * 64]).clone() for i in range(3)]
        assert lib.lgcn_ctx_folded_steps(m._dev['ctx']) == 0
        out.append((torch.stack(ls),) + _state(m))
        _clean(pkg, m)
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)


def test_variant_model_is_untouched(pkg, tiny, tmp_path):
    """a model with the popularity gate and item-item smoothing (the fused step's optional branches) runs another loss kernel:
    fused_epoch does not fold there, whatever the switch says"""
    lib = pkg._lib.load()
    meta = json.load(open(os.path.join(tiny.dir, "golden_gate_i2i.json")))
    d = os.path.join(str(tmp_path), "tiny_fold")
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(tiny.dir, f), os.path.join(d, f))
    w = pkg.world
    B = 44
    rng = np.random.Generator(np.random.PCG64(9))
    T = 2 * B + 5
    U, P, Nn = (_dev(rng.integers(0, hi, T), torch.int32) for hi in (tiny.n_users, tiny.m_items, tiny.m_items))
    out = []
    try:
        for fold in (1, 0):
            w.configure([])
            w.dataset = "tiny"
            w.config.update({'lightGCN_n_layers': meta["K"], 'latent_dim_rec': meta["d"], 'bpr_batch_size': B, 'decay': meta["decay"],
                             'lr': meta["lr"], 'use_pop_gate': meta["use_pop_gate"], 'use_item_item': meta["use_item_item"],
                             'i2i_path': os.path.join(tiny.dir, "i2i_tiny.npz") if meta["use_item_item"] else None,
                             'i2i_alpha': meta["i2i_alpha"], 'fused_variants': 1, 'fold_g32': fold})
            w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
            ds = pkg.dataloader.Loader(w.config, path=d)
            pkg.utils.set_seed(meta["seed"])
            m = pkg.model.LightGCN(w.config, ds).to(DEV)
            m.train()
            assert m.has_variants and m.fused_variants
            losses = m.fused_epoch(U, P, Nn, B)
            assert lib.lgcn_ctx_folded_steps(m._dev['ctx']) == 0
            torch.cuda.synchronize()
            out.append([losses.clone()] + [v.detach().clone() for v in m.state_dict().values()])
            m.check_device_errors()
    finally:
        w.configure([])
    assert len(out[0]) == len(out[1]) and all(torch.equal(a, b) for a, b in zip(out[0], out[1]))

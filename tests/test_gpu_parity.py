"""Parity tests proper (-m gpu): the HIP path, called through the C ABI, against the CPU
oracle on the same seeded inputs, against the golden fixtures captured from the reference,
and -- at full Gowalla size -- through size-independent properties.

Tolerances (fp32 path): the GPU sums a CSR row in 4 interleaved partial sums with FMA, the
oracle/reference sequentially without, so single SpMM outputs agree to ~1e-6 relative;
per-step losses to 5e-6 absolute; parameters after an epoch to 1e-5 absolute; Recall/NDCG
to 1e-4 (BASELINE.json north_star).  Integer work (sampler, shuffle, permutation apply) is
bit-exact.  bf16 activation storage is a separate, looser mode (2e-2 relative on rows)."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import EPS32, GOLDEN, assert_rows_close, spmm_sum_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def _spmm(pkg, indptr, indices, vals, X, x_dtype=0, y_dtype=0):
    g = pkg._lib.Graph(_dev(indptr.astype(np.int32)), _dev(indices.astype(np.int32)), _dev(vals.astype(np.float32)),
                       d_max=X.shape[1])
    x = _dev(X.astype(np.float32))
    if x_dtype == 1:
        x = x.to(torch.bfloat16)
    y = g.spmm(x, y_dtype)
    torch.cuda.synchronize()
    g.close()
    return y.float().cpu().numpy()


def _random_graph(rng, n, avg_deg, heavy=0):
    deg = rng.poisson(avg_deg, n).astype(np.int64)
    deg[rng.integers(0, n, max(1, n // 50))] = 0            # empty rows
    for _ in range(heavy):
        deg[rng.integers(0, n)] = min(n - 1, 40 * avg_deg)   # a few very long rows
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in deg] + [np.zeros(0, np.int64)]).astype(np.int32)
    vals = rng.uniform(0.01, 0.4, len(indices)).astype(np.float32)
    return indptr, indices, vals


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_spmm_vs_oracle_random(pkg, oracle, d):
    rng = np.random.Generator(np.random.PCG64(d))
    indptr, indices, vals = _random_graph(rng, 3001, 9, heavy=3)      # heavy rows take the split-row path
    X = rng.normal(0, 0.1, (3001, d)).astype(np.float32)
    ref = oracle.spmm(indptr, indices, vals, X)
    got = _spmm(pkg, indptr, indices, vals, X)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-6)
    # bf16 storage of the gathered table and of the output: fp32 accumulate
    Xb = torch.from_numpy(X).to(torch.bfloat16).float().numpy()
    refb = oracle.spmm(indptr, indices, vals, Xb)
    gotb = _spmm(pkg, indptr, indices, vals, X, x_dtype=1, y_dtype=0)
    np.testing.assert_allclose(gotb, refb, rtol=2e-5, atol=1e-6)
    gotbb = _spmm(pkg, indptr, indices, vals, X, x_dtype=1, y_dtype=1)
    np.testing.assert_allclose(gotbb, refb, rtol=1e-2, atol=1e-4)


def test_spmm_edge_cases(pkg, oracle):
    # single row, empty matrix rows only, one neighbour
    X = np.arange(2 * 64, dtype=np.float32).reshape(2, 64)
    got = _spmm(pkg, np.array([0, 0, 0]), np.zeros(0, np.int32), np.zeros(0, np.float32), X)
    assert np.array_equal(got, np.zeros_like(X))
    got = _spmm(pkg, np.array([0, 1, 1]), np.array([1], np.int32), np.array([0.5], np.float32), X)
    assert np.array_equal(got[0], 0.5 * X[1]) and np.all(got[1] == 0)
    L = pkg._lib
    assert L.load().lgcn_spmm_csr(None, None, 0, None, 0, 64, None) != 0
    assert b"null" in L.load().lgcn_last_error()
    x = torch.zeros(4, 48, device=DEV)
    g = L.Graph(torch.zeros(5, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                torch.zeros(0, device=DEV), d_max=64)
    assert L.load().lgcn_spmm_csr(g.handle, L.tp(x), 0, L.tp(x), 0, 48, None) == 3          # unsupported dim
    with pytest.raises(L.LgcnError):
        L.Graph(torch.tensor([0, 2, 1], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                torch.zeros(1, device=DEV))                                               # non-monotone indptr


def _make_model(pkg, g, tmp_path, act_dtype="fp32", K=None, B=None, row_order="cocluster", reg_rows="propagated", dim=None):
    d = os.path.join(str(tmp_path), g.name + act_dtype)
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(g.dir, f), os.path.join(d, f))
    w = pkg.world
    w.configure([])
    w.dataset = g.name
    w.config.update({'lightGCN_n_layers': K or g.K, 'latent_dim_rec': dim or g.d, 'bpr_batch_size': B or g.B,
                     'act_dtype': act_dtype, 'decay': g.meta["decay"], 'lr': g.meta["lr"], 'row_order': row_order,
                     'reg_rows': reg_rows})
    w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=d)
    pkg.sampling.seed(w.seed)
    pkg.utils.set_seed(w.seed)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    return ds, m


def test_computer_vs_golden_and_oracle(pkg, oracle, tiny, lastfm, tmp_path):
    for g in (tiny, lastfm):
        ds, m = _make_model(pkg, g, tmp_path)
        assert np.array_equal(m._table.cpu().numpy(), g.e0())                    # seed-2020 init, bit-exact
        with torch.no_grad():
            au, ai = m.computer()
        got = torch.cat([au, ai]).cpu().numpy()
        ref = oracle.propagate(g.z["adj_indptr"], g.z["adj_indices"], g.z["adj_data"], g.e0(), g.K)
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-7)
        gold = np.concatenate([g.z["computer_users"], g.z["computer_items"]], 0)
        np.testing.assert_allclose(np.concatenate([got[:g.n_users][::g.stride], got[g.n_users:][::g.stride]]),
                                   gold, rtol=2e-5, atol=2e-7)


def test_unfused_bpr_loss_autograd_vs_golden(pkg, tiny, tmp_path):
    """model.bpr_loss + loss.backward() (the reference's own stageOne recipe) through the
    custom autograd Function: loss, reg and both parameter gradients."""
    g = tiny
    ds, m = _make_model(pkg, g, tmp_path)
    m.train()
    loss, reg = m.bpr_loss(_dev(g.z["b_users"]), _dev(g.z["b_pos"]), _dev(g.z["b_neg"]))
    assert abs(float(loss) - g.meta["b_loss"]) < 2e-6 and abs(float(reg) - g.meta["b_reg"]) < 2e-6
    (loss + reg * g.meta["decay"]).backward()
    np.testing.assert_allclose(m.embedding_user.weight.grad.cpu().numpy(), g.z["b_grad_user"], rtol=2e-4, atol=2e-9)
    np.testing.assert_allclose(m.embedding_item.weight.grad.cpu().numpy(), g.z["b_grad_item"], rtol=2e-4, atol=2e-9)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_fused_step_vs_oracle(pkg, oracle, tiny, tmp_path, K):
    """One fused stageOne vs the oracle's stageOne for every layer count (K=1 exercises the
    sparse-input + Adam kernel, K=2 the single-buffer chain, K=4 the ping-pong)."""
    g = tiny
    ds, m = _make_model(pkg, g, tmp_path, K=K)
    A = (g.z["adj_indptr"], g.z["adj_indices"], g.z["adj_data"])
    tr = oracle.Trainer(g.n_users, *A, g.e0(), K, g.meta["decay"], g.meta["lr"])
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    rng = np.random.Generator(np.random.PCG64(K))
    for step in range(3):
        nb = [64, 17, 1][step]
        u = rng.integers(0, g.n_users, nb); p = rng.integers(0, g.m_items, nb); n = rng.integers(0, g.m_items, nb)
        if step == 0:
            u[:8] = u[0]; p[:8] = p[0]; n[8:12] = p[0]          # duplicates / pos-neg collisions
        l_ref = tr.stageOne(u, p, n)
        l_got = bpr.stageOne(_dev(u), _dev(p), _dev(n))
        assert abs(l_got - l_ref) < 3e-6, (step, l_got, l_ref)
        np.testing.assert_allclose(m._table.cpu().numpy(), tr.e0, rtol=0, atol=3e-6)
    st = m._dev
    np.testing.assert_allclose(st['adam_m'].cpu().numpy(), tr.m, rtol=2e-3, atol=1e-9)
    np.testing.assert_allclose(st['adam_v'].cpu().numpy(), tr.v, rtol=2e-3, atol=1e-13)
    # workspace is clean again after the step
    assert int(st['G64'].abs().sum()) == 0          # (the row bitmaps alternate; the stale one is zeroed by the next step)
    m.check_device_errors()


@pytest.mark.parametrize("dense_last", ["0", "1"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_upstream_loss_fused_step_vs_oracle(pkg, oracle, tiny, tmp_path, K, dense_last):
    """--reg_rows ego: UPSTREAM LightGCN's bpr_loss (L2 term on the embedding tables' own rows of the batch -- the loss behind the
    recorded 1000-epoch run and README table the reference keeps; this fork moved the term to the propagated rows, model.py:173).
    In the fused step the term's gradient decay/B * count(row) * E0[row] bypasses the propagation: k_triplet counts the slots
    per row, the Adam epilogue adds count * lam * P[row].  Three steps (duplicated users / items, pos-neg collisions, B = 1) vs
    oracle.Trainer(reg_rows='ego') -- whose gradient algebra test_oracle checks against torch autograd -- for K = 1 (sparse +
    Adam in one launch), 2, 3 and both last-layer forms; and the unfused autograd path of model.bpr_loss on the same batch."""
    g = tiny
    ds, m = _make_model(pkg, g, tmp_path, K=K, reg_rows="ego")
    m.config['dense_last'] = dense_last
    A = (g.z["adj_indptr"], g.z["adj_indices"], g.z["adj_data"])
    tr = oracle.Trainer(g.n_users, *A, g.e0(), K, g.meta["decay"], g.meta["lr"], reg_rows="ego")
    rng = np.random.Generator(np.random.PCG64(100 + K))
    u = rng.integers(0, g.n_users, 64); p = rng.integers(0, g.m_items, 64); n = rng.integers(0, g.m_items, 64)
    u[:8] = u[0]; p[:8] = p[0]; n[8:12] = p[0]
    # unfused: model.bpr_loss + autograd (the reference's call shape) against the oracle's loss / reg of the same batch
    E = oracle.propagate(*A, g.e0(), K)
    l_o, r_o, G_o, Gego_o = oracle.bpr_ego(E, g.e0(), g.n_users, u, p, n, g.meta["decay"])
    m.train()
    loss, reg = m.bpr_loss(_dev(u), _dev(p), _dev(n))
    assert abs(float(loss) - l_o) < 2e-6 and abs(float(reg) - r_o) < 2e-6 * max(1.0, r_o)
    (loss + g.meta["decay"] * reg).backward()
    grad = torch.cat([m.embedding_user.weight.grad, m.embedding_item.weight.grad]).cpu().numpy()
    want = oracle.propagate_bwd(*A, G_o, K) + Gego_o
    np.testing.assert_allclose(grad, want, rtol=2e-4, atol=2e-9)
    m.zero_grad(set_to_none=True)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    for step in range(3):
        nb = [64, 17, 1][step]
        if step:
            u = rng.integers(0, g.n_users, nb); p = rng.integers(0, g.m_items, nb); n = rng.integers(0, g.m_items, nb)
        l_ref = tr.stageOne(u, p, n)
        l_got = bpr.stageOne(_dev(u), _dev(p), _dev(n))
        assert abs(l_got - l_ref) < 3e-6, (step, l_got, l_ref)
        np.testing.assert_allclose(m._table.cpu().numpy(), tr.e0, rtol=0, atol=3e-6)
    st = m._dev
    assert int(st['G64'].abs().sum()) == 0
    # and it IS another loss: the fork's gradient on the first batch differs (test_oracle compares whole steps)
    _, _, G_fork = oracle.bpr(E, g.n_users, g.z["b_users"], g.z["b_pos"], g.z["b_neg"], g.meta["decay"])
    _, _, G_up, _ = oracle.bpr_ego(E, g.e0(), g.n_users, g.z["b_users"], g.z["b_pos"], g.z["b_neg"], g.meta["decay"])
    assert np.abs(G_fork - G_up).max() > 1e-9
    m.check_device_errors()


@pytest.mark.parametrize("mode", ["rows", "dense", "row_sharded"])
@pytest.mark.parametrize("world", [2, 3])
def test_upstream_loss_dp_epoch_loopback(pkg, tiny, tmp_path, world, mode):
    """--reg_rows ego under data parallelism, the C loop at world 2 / 3 through the loopback communicator in all three exchange
    modes: the per-row slot counts are integers (own shard in part 1 + the other ranks' in k_scatter; the whole batch in
    k_flag_rows for the dense form; k_scatter alone for row-sharded), so every rank ends bit for bit where the single-GPU
    epoch ends -- and three epochs in a row leave the counts clean (a stale count would change the next epoch)."""
    import threading
    g = tiny
    rng = np.random.Generator(np.random.PCG64(23 * world + len(mode)))
    B = 48
    T = 3 * B + 1
    u = rng.integers(0, g.n_users, T); p = rng.integers(0, g.m_items, T); n = rng.integers(0, g.m_items, T)
    u[5] = u[40]; p[7] = p[30]; n[9] = p[30]
    U, P, Nn = (_dev(x, torch.int32) for x in (u, p, n))
    ds, ref = _make_model(pkg, g, tmp_path, B=B, reg_rows="ego")
    L, lib = pkg._lib, pkg._lib.load()
    models = [_make_model(pkg, g, tmp_path, B=B, reg_rows="ego")[1] for _ in range(world)]
    par = pkg.parallel
    ranges = par.row_ranges(models[0]._adj.indptr, models[0].n_users, world) if mode == "row_sharded" else None
    states = [mm._state(max_batch=B, need_ctx=True, dp_world=world,
                        row_subset=par.owned_rows(ranges, r) if ranges is not None else None) for r, mm in enumerate(models)]
    comms = (C.c_void_p * world)()
    L.check(lib.lgcn_dp_init_loopback(world, comms), "loopback")
    code = {"rows": 0, "dense": 1, "row_sharded": 2}[mode]
    steps = (T + B - 1) // B
    streams = [torch.cuda.Stream() for _ in range(world)]
    gathered = [torch.empty(world * par.block_numel(B, world, g.d), device=DEV) for _ in range(world)]
    losses = [torch.empty(steps, 3, device=DEV) for _ in range(world)]
    rr = np.ascontiguousarray(ranges, np.int64) if ranges is not None else None
    for epoch in range(3):
        want_loss = ref.fused_epoch(U, P, Nn, B).cpu().numpy()
        want = ref._table.cpu().numpy().view(np.uint32)
        torch.cuda.synchronize()
        rcs, errs = [None] * world, [None] * world

        def rank_main(r):
            rcs[r] = lib.lgcn_train_epoch_dp(states[r]['ctx'], comms[r], L.tp(U), L.tp(P), L.tp(Nn), T, B, code,
                                             L.npp(rr) if rr is not None else None, L.tp(gathered[r]), L.tp(losses[r]),
                                             C.c_void_p(streams[r].cuda_stream))
            if rcs[r]:
                errs[r] = lib.lgcn_last_error()
        threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
        assert not any(t.is_alive() for t in threads), "a rank did not come back from lgcn_train_epoch_dp"
        torch.cuda.synchronize()
        assert rcs == [0] * world, (rcs, errs)
        for r, mm in enumerate(models):
            assert np.array_equal(losses[r].cpu().numpy(), want_loss), (mode, world, r, epoch)
            assert np.array_equal(mm._table.cpu().numpy().view(np.uint32), want), (mode, world, r, epoch)
            mm.check_device_errors()
    for r in range(world):
        lib.lgcn_dp_destroy(comms[r])


def test_stage_one_call_shapes(pkg, oracle, tiny, tmp_path):
    """BPRLoss.stageOne the way the reference calls it -- torch.long device tensors, a Python float back (utils.py:53-64) -- goes through
    lgcn_train_step_i64 (one launch narrows the ids inside the step); int32 tensors, numpy arrays, non-contiguous views and the
    --lazy_loss 1 DeferredLoss take the same step: identical losses and parameters whatever the call shape; an id beyond int32 in a
    torch.long tensor is flagged like any out-of-range id."""
    g = tiny
    A = (g.z["adj_indptr"], g.z["adj_indices"], g.z["adj_data"])
    rng = np.random.Generator(np.random.PCG64(77))
    batches = [(rng.integers(0, g.n_users, b), rng.integers(0, g.m_items, b), rng.integers(0, g.m_items, b)) for b in (64, 17, 1)]
    results = {}
    for shape in ("int64", "int32", "numpy", "strided", "deferred"):
        ds, m = _make_model(pkg, g, tmp_path)
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        bpr.deferred = shape == "deferred"
        losses = []
        for (u, p, n) in batches:
            if shape in ("int64", "deferred"):
                args = tuple(torch.from_numpy(x.astype(np.int64)).to(DEV) for x in (u, p, n))
            elif shape == "int32":
                args = tuple(torch.from_numpy(x.astype(np.int32)).to(DEV) for x in (u, p, n))
            elif shape == "numpy":
                args = (u, p, n)
            else:
                args = tuple(torch.from_numpy(np.repeat(x.astype(np.int64), 2)).to(DEV)[::2] for x in (u, p, n))
            r = bpr.stageOne(*args)
            assert isinstance(r, pkg.utils.DeferredLoss) if shape == "deferred" else isinstance(r, float)
            losses.append(float(r))
        results[shape] = (losses, m._table.detach().cpu().numpy().copy())
        m.check_device_errors()
    tr = oracle.Trainer(g.n_users, *A, g.e0(), g.K, g.meta["decay"], g.meta["lr"])
    want = [tr.stageOne(u, p, n) for (u, p, n) in batches]
    for shape, (losses, table) in results.items():
        assert losses == results["int64"][0] and np.array_equal(table, results["int64"][1]), shape
    assert np.abs(np.asarray(results["int64"][0]) - np.asarray(want)).max() < 3e-6
    np.testing.assert_allclose(results["int64"][1], tr.e0, rtol=0, atol=3e-6)
    # an id that does not fit int32
    ds, m = _make_model(pkg, g, tmp_path)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    u = torch.tensor([1, (1 << 40) + 3], dtype=torch.int64, device=DEV); p = torch.tensor([2, 3], dtype=torch.int64, device=DEV)
    bpr.stageOne(u, p, p.clone())
    with pytest.raises(pkg._lib.LgcnError):
        m.check_device_errors()


def test_epochs_tiny_vs_golden(pkg, tiny, tmp_path):
    """Two epochs driven exactly like main.py:215-225 through the product's own sampler,
    shuffle and fused step: triplets bit-exact, losses / parameters / Adam state vs the
    reference's."""
    g = tiny
    ds, m = _make_model(pkg, g, tmp_path)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    for e in (1, 2):
        S = pkg.utils.UniformSample_original(ds)
        assert np.array_equal(S, g.z[f"S_epoch{e}"])
        users, pos, neg = (torch.tensor(S[:, c], dtype=torch.long, device=DEV) for c in range(3))
        users, pos, neg = pkg.utils.shuffle(users, pos, neg)
        assert np.array_equal(users.cpu().numpy(), g.z[f"shuf_users_epoch{e}"])
        assert np.array_equal(neg.cpu().numpy(), g.z[f"shuf_neg_epoch{e}"])
        losses = [bpr.stageOne(bu, bp, bn) for (bu, bp, bn) in pkg.utils.minibatch(users, pos, neg, batch_size=g.B)]
        np.testing.assert_allclose(losses, g.z[f"losses_epoch{e}"], rtol=0, atol=3e-6)
        P = np.concatenate([g.z[f"P_user_epoch{e}"], g.z[f"P_item_epoch{e}"]], 0)
        np.testing.assert_allclose(m._table.cpu().numpy(), P, rtol=0, atol=6e-6)
    sd = bpr.opt.state_dict()
    assert int(sd['state'][0]['step']) == 2 * g.meta["adam_step_epoch1"]
    assert sd['param_groups'][0]['lr'] == g.meta["lr"]


def test_procedure_epoch_lastfm_vs_golden(pkg, lastfm, tmp_path):
    """Config C1 (LastFM, K=2, python-mode sampler): Procedure.BPR_train_original + Test vs the
    reference's per-step losses and Recall/NDCG/Precision@20 before and after one epoch."""
    g = lastfm
    ds, m = _make_model(pkg, g, tmp_path)
    pkg.world.tensorboard = 0
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    r0 = pkg.Procedure.Test(ds, m, 0)
    for k in ("precision", "recall", "ndcg"):
        assert abs(r0[k][0] - g.meta["test_epoch0"][k][0]) < 1e-7, k
    # same epoch twice: once step by step (losses), once through the epoch procedure
    users, pos, neg = pkg.Procedure.sample_epoch_to_device(ds, DEV)
    assert np.array_equal(users.cpu().numpy(), g.z["shuf_users_epoch1"])
    losses = m.fused_epoch(users, pos, neg, g.B)[:, 0].cpu().numpy()
    np.testing.assert_allclose(losses, g.z["losses_epoch1"], rtol=0, atol=5e-6)
    r1 = pkg.Procedure.Test(ds, m, 1)
    for k in ("precision", "recall", "ndcg"):
        assert abs(r1[k][0] - g.meta["test_epoch1"][k][0]) < 1e-4, (k, r1[k], g.meta["test_epoch1"][k])
    out = pkg.Procedure.BPR_train_original(ds, m, bpr, 2)
    assert out.startswith("loss0.") and "|Sample:" in out
    r2 = pkg.Procedure.Test(ds, m, 2)
    for k in ("precision", "recall", "ndcg"):
        assert abs(r2[k][0] - g.meta["test_epoch2"][k][0]) < 1e-4, (k, r2[k], g.meta["test_epoch2"][k])
    assert os.path.exists(os.path.join(pkg.world.config['checkpoint_dir'], 'train_epoch_metrics.csv'))


def test_bitwise_reproducible_and_dp_split(pkg, tiny, tmp_path):
    """(a) two runs of the same steps give identical bits (fixed-point gradient reduction);
    (b) the data-parallel split (part1 per rank -> concatenated blocks -> part2) equals the
    single-GPU step bit for bit, for world = 2 and 3 with a ragged last shard."""
    g = tiny
    rng = np.random.Generator(np.random.PCG64(1))
    batches = [(rng.integers(0, g.n_users, b), rng.integers(0, g.m_items, b), rng.integers(0, g.m_items, b))
               for b in (64, 64, 37)]

    def run(world):
        ds, m = _make_model(pkg, g, tmp_path)
        L, lib = pkg._lib, pkg._lib.load()
        losses = []
        for (u, p, n) in batches:
            u, p, n = (_dev(x, torch.int32) for x in (u, p, n))
            B = len(u)
            if world == 1:
                losses.append(m.fused_step(u, p, n).cpu().numpy())
                continue
            st = m._state(max_batch=64, need_ctx=True, dp_world=world)
            nblk = pkg.parallel.block_numel(B, world, g.d)
            blocks = []
            for r in range(world):
                L.check(lib.lgcn_train_step_dp_part1(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, r,
                                                     L.current_stream()), "part1")
                blocks.append(st['contrib'][:nblk].clone())
            gathered = torch.cat(blocks)
            out = torch.empty(3, device=DEV)
            L.check(lib.lgcn_train_step_dp_part2(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, L.tp(gathered),
                                                 L.tp(out), L.current_stream()), "part2")
            losses.append(out.cpu().numpy())
        return m._table.cpu().numpy().copy(), np.array(losses)

    def run_dense(world):
        """dense (all-reduce) form emulated on one GPU: every rank's part 1 accumulates into the same
        G64 / bitmap / terms, which is exactly what the SUM / BOR all-reduces produce."""
        ds, m = _make_model(pkg, g, tmp_path)
        L, lib = pkg._lib, pkg._lib.load()
        losses = []
        for (u, p, n) in batches:
            u, p, n = (_dev(x, torch.int32) for x in (u, p, n))
            B = len(u)
            st = m._state(max_batch=64, need_ctx=True, dp_world=world)
            acc_terms = torch.zeros(2 * B, device=DEV)
            for r in range(world):
                L.check(lib.lgcn_train_step_dp_dense_part1(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, r,
                                                           L.current_stream()), "dense part1")
                acc_terms += st['terms'][:2 * B]
            st['terms'][:2 * B].copy_(acc_terms)
            out = torch.empty(3, device=DEV)
            L.check(lib.lgcn_train_step_dp_part2(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, None,
                                                 L.tp(out), L.current_stream()), "part2")
            losses.append(out.cpu().numpy())
        return m._table.cpu().numpy().copy(), np.array(losses)

    p1, l1 = run(1)
    p1b, l1b = run(1)
    assert np.array_equal(p1.view(np.uint32), p1b.view(np.uint32)) and np.array_equal(l1, l1b)
    for world in (2, 3):
        pw, lw = run(world)
        assert np.array_equal(p1.view(np.uint32), pw.view(np.uint32)), world
        np.testing.assert_allclose(lw, l1, rtol=0, atol=1e-6)
        pd, ld = run_dense(world)
        assert np.array_equal(p1.view(np.uint32), pd.view(np.uint32)), ("dense", world)
        np.testing.assert_allclose(ld, l1, rtol=0, atol=1e-6)


@pytest.mark.parametrize("local", [0, 1])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_dp_rows_one_model_per_rank(pkg, tiny, tmp_path, world, local):
    """The batch-sharded step the way the ranks really run it: W separate models (same seed), each rank's part 1 on ITS
    model, the blocks concatenated in rank order (the all-gather), each rank's part 2 on its model.  local = 1 is what
    lgcn_train_epoch_dp does: part 1 also adds the rank's own rows into its G64 and part 2 scatters only the others'.
    Every model must end bit for bit where the single-GPU model ends; ragged last shard, duplicate ids across ranks."""
    g = tiny
    rng = np.random.Generator(np.random.PCG64(5 + world))
    batches = [(rng.integers(0, g.n_users, b), rng.integers(0, g.m_items, b), rng.integers(0, 12, b)) for b in (64, 41, 64)]
    ds, ref = _make_model(pkg, g, tmp_path)
    for (u, p, n) in batches:
        ref.fused_step(_dev(u, torch.int32), _dev(p, torch.int32), _dev(n, torch.int32))
    want = ref._table.cpu().numpy().view(np.uint32)
    L, lib = pkg._lib, pkg._lib.load()
    models = [_make_model(pkg, g, tmp_path)[1] for _ in range(world)]
    states = [m._state(max_batch=64, need_ctx=True, dp_world=world) for m in models]
    for st in states:
        L.check(lib.lgcn_ctx_set_dp_local(st['ctx'], local), "set_dp_local")
    for (u, p, n) in batches:
        u, p, n = (_dev(x, torch.int32) for x in (u, p, n))
        B = len(u)
        nblk = pkg.parallel.block_numel(B, world, g.d)
        blocks = []
        for r, st in enumerate(states):
            L.check(lib.lgcn_train_step_dp_part1(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, r, L.current_stream()), "part1")
            blocks.append(st['contrib'][:nblk].clone())
        gathered = torch.cat(blocks)
        outs = []
        for st in states:
            out = torch.empty(3, device=DEV)
            L.check(lib.lgcn_train_step_dp_part2(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, L.tp(gathered), L.tp(out),
                                                 L.current_stream()), "part2")
            outs.append(out.cpu().numpy())
        assert all(np.array_equal(outs[0], o) for o in outs[1:])
    for r, m in enumerate(models):
        assert np.array_equal(m._table.cpu().numpy().view(np.uint32), want), (world, local, r)
        assert int(m._dev['G64'].abs().sum()) == 0
        m.check_device_errors()


@pytest.mark.parametrize("act", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", ["rows", "dense", "row_sharded"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_dp_epoch_c_loop_world_gt_1_loopback(pkg, tiny, lastfm, tmp_path, world, mode, act):
    """lgcn_train_epoch_dp ITSELF at world > 1 on one GPU: W threads of this process, each with its own model, context,
    stream and loopback communicator (lgcn_dp_init_loopback: the collectives meet on a host barrier and move the blocks
    with hipMemcpyAsync -- no RCCL, no second process), run the C loop of a whole epoch in all three exchange modes:
    gradient-row all-gather (LocalScope: own rows added in part 1), dense all-reduce of the fixed-point table, and
    row-sharded propagation (rs_exchange's grouped in-place broadcasts, owned-row plans).  T is not a multiple of the
    batch and the last batch leaves trailing ranks EMPTY.  Every rank must end bit for bit where the single-GPU
    epoch ends, with the same per-step losses."""
    import threading
    g = tiny if mode != "row_sharded" or world < 4 else lastfm
    rng = np.random.Generator(np.random.PCG64(17 * world + len(mode)))
    B = 48
    T = 3 * B + (2 if world > 2 else 1)                       # last global batch: 1-2 triplets -> trailing ranks get none
    u = rng.integers(0, g.n_users, T); p = rng.integers(0, g.m_items, T); n = rng.integers(0, g.m_items, T)
    u[5] = u[40]; p[7] = p[30]                                 # the same rows named by different ranks' shards
    U, P, Nn = (_dev(x, torch.int32) for x in (u, p, n))
    ds, ref = _make_model(pkg, g, tmp_path, act_dtype=act, B=B)
    want_loss = ref.fused_epoch(U, P, Nn, B).cpu().numpy()
    want = ref._table.cpu().numpy().view(np.uint32)
    L, lib = pkg._lib, pkg._lib.load()
    models = [_make_model(pkg, g, tmp_path, act_dtype=act, B=B)[1] for _ in range(world)]
    par = pkg.parallel
    ranges = par.row_ranges(models[0]._adj.indptr, models[0].n_users, world) if mode == "row_sharded" else None
    states = [m._state(max_batch=B, need_ctx=True, dp_world=world,
                       row_subset=par.owned_rows(ranges, r) if ranges is not None else None) for r, m in enumerate(models)]
    comms = (C.c_void_p * world)()
    L.check(lib.lgcn_dp_init_loopback(world, comms), "loopback")
    code = {"rows": 0, "dense": 1, "row_sharded": 2}[mode]
    steps = (T + B - 1) // B
    streams = [torch.cuda.Stream() for _ in range(world)]
    gathered = [torch.empty(world * par.block_numel(B, world, g.d), device=DEV) for _ in range(world)]
    losses = [torch.empty(steps, 3, device=DEV) for _ in range(world)]
    rr = np.ascontiguousarray(ranges, np.int64) if ranges is not None else None
    torch.cuda.synchronize()
    rcs, errs = [None] * world, [None] * world

    def rank_main(r):
        rcs[r] = lib.lgcn_train_epoch_dp(states[r]['ctx'], comms[r], L.tp(U), L.tp(P), L.tp(Nn), T, B, code,
                                         L.npp(rr) if rr is not None else None, L.tp(gathered[r]), L.tp(losses[r]),
                                         C.c_void_p(streams[r].cuda_stream))
        if rcs[r]:
            errs[r] = lib.lgcn_last_error()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank did not come back from lgcn_train_epoch_dp"
    torch.cuda.synchronize()
    assert rcs == [0] * world, (rcs, errs)
    for r, m in enumerate(models):
        assert np.array_equal(losses[r].cpu().numpy(), want_loss), (mode, world, r)
        assert np.array_equal(m._table.cpu().numpy().view(np.uint32), want), (mode, world, r)
        assert not bool(m._dev['G64'].any())
        m.check_device_errors()
    for r in range(world):
        lib.lgcn_dp_destroy(comms[r])


@pytest.mark.parametrize("world,d,act,reg_rows", [(2, 64, "fp32", "propagated"), (2, 64, "bf16", "propagated"), (4, 128, "fp32", "propagated"),
                                                  (2, 128, "fp32", "ego"), (8, 256, "fp32", "propagated")])
def test_dp_cols_epoch_loopback(pkg, tiny, tmp_path, world, d, act, reg_rows):
    """Column-sharded data parallelism (shard='cols', LGCN_DP_COLS): rank r holds columns [r d/W, (r+1) d/W) of the tables as an
    ordinary model of width d / W (parallel.column_shard: the full seed-2020 table, sliced); the C loop of lgcn_train_epoch_dp runs
    part 1 -> ONE all-reduce of 3*B partial scores / reg terms -> part 2, on W threads through the loopback communicator.  The ranks'
    tables, concatenated, against the single-GPU epoch of the full-width model, and every rank's per-step losses against its: NOT
    bitwise -- a score is now the sum of W partial dot products (fp32: <= ~W * 2^-24 relative on the score, which moves the
    gradient rows, hence Adam's steps, by as much); with bf16 storage such a difference can also land on the other side of a
    bf16 rounding of a backward row element (2^-9 of it)."""
    import threading
    g = tiny
    rng = np.random.Generator(np.random.PCG64(31 * world + d))
    B = 48
    T = 3 * B + 5
    u = rng.integers(0, g.n_users, T); p = rng.integers(0, g.m_items, T); n = rng.integers(0, g.m_items, T)
    u[5] = u[40]; p[7] = p[30]; n[9] = p[30]
    U, P, Nn = (_dev(x, torch.int32) for x in (u, p, n))
    ds, ref = _make_model(pkg, g, tmp_path, act_dtype=act, B=B, reg_rows=reg_rows, dim=d)
    E0_full = ref._table.detach().clone()
    want_loss = ref.fused_epoch(U, P, Nn, B).cpu().numpy()
    want = ref._table.detach().cpu().numpy()
    L, lib = pkg._lib, pkg._lib.load()
    par = pkg.parallel
    models = []
    for r in range(world):
        pkg.utils.set_seed(pkg.world.seed)                          # column_shard draws the FULL table as LightGCN.__init__ does
        models.append(par.column_shard(pkg.model.LightGCN, pkg.world.config, ds, world, r, DEV))
        lo, hi = par.column_range(d, world, r)
        assert models[-1].latent_dim == d // world and torch.equal(models[-1]._table.detach(), E0_full[:, lo:hi])
    states = [mm._state(max_batch=B, need_ctx=True, dp_world=1) for mm in models]
    comms = (C.c_void_p * world)()
    L.check(lib.lgcn_dp_init_loopback(world, comms), "loopback")
    steps = (T + B - 1) // B
    streams = [torch.cuda.Stream() for _ in range(world)]
    losses = [torch.empty(steps, 3, device=DEV) for _ in range(world)]
    torch.cuda.synchronize()
    rcs, errs = [None] * world, [None] * world

    def rank_main(r):
        rcs[r] = lib.lgcn_train_epoch_dp(states[r]['ctx'], comms[r], L.tp(U), L.tp(P), L.tp(Nn), T, B, 3, None, None,
                                         L.tp(losses[r]), C.c_void_p(streams[r].cuda_stream))
        if rcs[r]:
            errs[r] = lib.lgcn_last_error()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    torch.cuda.synchronize()
    assert rcs == [0] * world, (rcs, errs)
    got = torch.cat([mm._table.detach() for mm in models], dim=1).cpu().numpy()
    ltol, ptol = (2e-6, 2e-6) if act == "fp32" else (2e-5, 2e-4)
    for r in range(world):
        assert np.array_equal(losses[r].cpu().numpy(), losses[0].cpu().numpy())     # every rank reduces the same complete terms
        models[r].check_device_errors()
        assert not bool(models[r]._dev['G64'].any())
    np.testing.assert_allclose(losses[0].cpu().numpy(), want_loss, rtol=0, atol=ltol)
    np.testing.assert_allclose(got, want, rtol=0, atol=ptol)
    assert np.abs(got - E0_full.cpu().numpy()).max() > 1e-4                          # (it trained)
    for r in range(world):
        lib.lgcn_dp_destroy(comms[r])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("tag", ["gate", "i2i", "gate_i2i"])
def test_dp_epoch_optional_branches_loopback(pkg, tiny, tmp_path, tag, world, mode):
    """The popularity gate / item-item smoothing under data parallelism -- mode 0: gradient-row exchange; mode 1: the dense form
    (all-reduce of G64, of the loss / reg / ENTROPY terms and of the fixed-point MLP gradient sums).  W threads, each with its own model
    (own MLP parameter buffer, own item-item graphs), context, stream and loopback communicator run lgcn_train_epoch_dp; the exchange
    block carries the gradient rows, the loss / reg / ENTROPY terms and the rank's fixed-point sums of the MLP parameter gradients.
    Ragged shards (the batch is not a multiple of the world, nor the shard of the 8 triplets a gate workgroup handles) and an empty
    trailing rank in the last batch: every rank's tables, MLP parameters and per-step losses end bit for bit where the single-GPU
    fused epoch ends."""
    import threading
    meta = json.load(open(os.path.join(tiny.dir, f"golden_{tag}.json")))
    d = os.path.join(str(tmp_path), "tiny_dp_" + tag)
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(tiny.dir, f), os.path.join(d, f))
    w = pkg.world
    w.configure([])
    w.dataset = "tiny"
    B = 44
    w.config.update({'lightGCN_n_layers': meta["K"], 'latent_dim_rec': meta["d"], 'bpr_batch_size': B, 'decay': meta["decay"], 'lr': meta["lr"],
                     'use_pop_gate': meta["use_pop_gate"], 'use_item_item': meta["use_item_item"],
                     'i2i_path': os.path.join(tiny.dir, "i2i_tiny.npz") if meta["use_item_item"] else None, 'i2i_alpha': meta["i2i_alpha"],
                     'fused_variants': 1})
    w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=d)

    def fresh():
        pkg.utils.set_seed(meta["seed"])
        m = pkg.model.LightGCN(w.config, ds).to(DEV)
        m.train()
        return m
    rng = np.random.Generator(np.random.PCG64(3 * world + len(tag)))
    T = 3 * B + 1                                              # last global batch: one triplet -> trailing ranks get none
    u = rng.integers(0, ds.n_users, T); p = rng.integers(0, ds.m_items, T); n = rng.integers(0, ds.m_items, T)
    p[:5] = p[5]; n[9] = p[5]; u[20] = u[30]
    U, P, Nn = (_dev(x, torch.int32) for x in (u, p, n))
    ref = fresh()
    want_loss = ref.fused_epoch(U, P, Nn, B).cpu().numpy()
    want = {k: v.detach().cpu().numpy().copy() for k, v in ref.state_dict().items()}
    L, lib = pkg._lib, pkg._lib.load()
    models = [fresh() for _ in range(world)]
    states = [m._state(max_batch=B, need_ctx=True, dp_world=world) for m in models]
    comms = (C.c_void_p * world)()
    L.check(lib.lgcn_dp_init_loopback(world, comms), "loopback")
    steps = (T + B - 1) // B
    streams = [torch.cuda.Stream() for _ in range(world)]
    nblk = int(lib.lgcn_dp_block_floats(states[0]['ctx'], B, world))
    assert nblk > pkg.parallel.block_numel(B, world, meta["d"]) or not meta["use_pop_gate"]
    gathered = [torch.empty(world * nblk, device=DEV) for _ in range(world)]
    losses = [torch.empty(steps, 3, device=DEV) for _ in range(world)]
    torch.cuda.synchronize()
    rcs, errs = [None] * world, [None] * world

    def rank_main(r):
        rcs[r] = lib.lgcn_train_epoch_dp(states[r]['ctx'], comms[r], L.tp(U), L.tp(P), L.tp(Nn), T, B, mode, None, L.tp(gathered[r]),
                                         L.tp(losses[r]), C.c_void_p(streams[r].cuda_stream))
        if rcs[r]:
            errs[r] = lib.lgcn_last_error()
    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads)
    torch.cuda.synchronize()
    assert rcs == [0] * world, (rcs, errs)
    for r, m in enumerate(models):
        assert np.array_equal(losses[r].cpu().numpy(), want_loss), (tag, world, r, losses[r].cpu().numpy(), want_loss)
        for k, v in m.state_dict().items():
            assert np.array_equal(v.detach().cpu().numpy().view(np.uint32), want[k].view(np.uint32)), (tag, world, r, k)
        assert not bool(m._dev['G64'].any())
        m.check_device_errors()
    for r in range(world):
        lib.lgcn_dp_destroy(comms[r])
    # row-sharded and column-sharded propagation refuse a context with a branch on
    st = models[0]._dev
    assert lib.lgcn_rs_phase(st['ctx'], 0, 1, L.tp(U), L.tp(P), L.tp(Nn), B, world, 0, None, None, L.current_stream()) != 0
    assert lib.lgcn_train_step_cols_part1(st['ctx'], L.tp(U), L.tp(P), L.tp(Nn), B, None, L.current_stream()) != 0
    gp, gn = C.c_void_p(), C.c_int32()
    L.check(lib.lgcn_ctx_gate_total(st['ctx'], C.byref(gp), C.byref(gn)), "gate_total")
    assert (gn.value > 0 and gp.value) if meta["use_pop_gate"] else gn.value == 0
    w.configure([])


def test_out_of_range_ids_are_flagged_not_faulting(pkg, tiny, tmp_path):
    ds, m = _make_model(pkg, tiny, tmp_path)
    before = m._table.clone()
    m.fused_step(_dev(np.array([0, tiny.n_users + 5]), torch.int32), _dev(np.array([1, 2]), torch.int32),
                 _dev(np.array([tiny.m_items, 3]), torch.int32))
    with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
        m.check_device_errors()
    m.check_device_errors()          # flag is cleared
    assert torch.isfinite(m._table).all() and before.shape == m._table.shape


def test_apply_perm_bit_exact(pkg):
    rng = np.random.Generator(np.random.PCG64(3))
    T = 100003
    S = rng.integers(0, 1 << 30, (T, 3)).astype(np.int32)
    perm = rng.permutation(T).astype(np.int64)
    L = pkg._lib
    Sd, pd = _dev(S), _dev(perm)
    u, p, n = (torch.empty(T, dtype=torch.int32, device=DEV) for _ in range(3))
    L.check(L.load().lgcn_apply_perm(L.tp(Sd), 3, L.tp(pd), T, L.tp(u), L.tp(p), L.tp(n), L.current_stream()), "perm")
    assert np.array_equal(u.cpu().numpy(), S[perm, 0]) and np.array_equal(n.cpu().numpy(), S[perm, 2])


def test_bf16_activation_mode(pkg, oracle, tiny, tmp_path):
    g = tiny
    ds, m = _make_model(pkg, g, tmp_path, act_dtype="bf16")
    with torch.no_grad():
        au, ai = m.computer()
    ref = oracle.propagate(g.z["adj_indptr"], g.z["adj_indices"], g.z["adj_data"], g.e0(), g.K)
    np.testing.assert_allclose(torch.cat([au, ai]).cpu().numpy(), ref, rtol=2e-2, atol=2e-4)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    l = bpr.stageOne(_dev(g.z["b_users"]), _dev(g.z["b_pos"]), _dev(g.z["b_neg"]))
    assert abs(l - g.meta["b_total"]) < 5e-4


def test_gowalla_full_size_properties_and_known_answer(pkg, oracle, tmp_path):
    """BASELINE configs[1] size (N = 70 839, nnz = 1 620 256): adjacency hashes, seed-2020 init
    hash, the reference's OWN epoch-0 known answer (tfevents 0.000188/0.000537/0.000408),
    first step losses, and size-independent properties of the SpMM (linearity, symmetry
    <y, A x> = <A y, x>, A 1 = rowsum) on the real graph."""
    npz = os.path.join(GOLDEN, "gowalla", "gowalla.npz")
    meta = json.load(open(os.path.join(GOLDEN, "gowalla", "golden_long.json")))
    zl = np.load(os.path.join(GOLDEN, "gowalla", "golden_long.npz"))
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import materialize_gowalla
    d = materialize_gowalla(npz, os.path.join(str(tmp_path), "gowalla"))
    w = pkg.world
    w.configure([]); w.dataset = "gowalla"; w.tensorboard = 0
    w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=d)
    adj = ds.getSparseGraphCSR()
    import hashlib
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert sha(adj.indptr) == meta["adj_sha256"]["indptr"] and sha(adj.indices) == meta["adj_sha256"]["indices"]
    assert sha(adj.data) == meta["adj_sha256"]["data"]                     # A_hat bit-exact at full size
    pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    assert sha(m.embedding_user.weight.detach().cpu().numpy()) == meta["E0_sha256"]["user"]
    with torch.no_grad():
        au, ai = m.computer()
    np.testing.assert_allclose(au[:8].cpu().numpy(), zl["computer_users_head"], rtol=2e-5, atol=2e-7)
    np.testing.assert_allclose(ai[:8].cpu().numpy(), zl["computer_items_head"], rtol=2e-5, atol=2e-7)
    assert abs(float(au.double().sum()) - meta["computer_sum"][0]) < 1e-2
    r0 = pkg.Procedure.Test(ds, m, 0)
    for k in ("precision", "recall", "ndcg"):
        assert abs(r0[k][0] - meta["test_epoch0"][k][0]) < 1e-8, (k, r0[k])
    # properties
    N = ds.n_users + ds.m_items
    gen = torch.Generator(device="cpu"); gen.manual_seed(5)
    x = torch.randn(N, 64, generator=gen).to(DEV); y = torch.randn(N, 64, generator=gen).to(DEV)
    Ax, Ay = m._spmm(x), m._spmm(y)
    lin = m._spmm(2.0 * x - 0.5 * y)
    assert torch.allclose(lin, 2.0 * Ax - 0.5 * Ay, rtol=1e-4, atol=1e-5)
    assert abs(float((y.double() * Ax.double()).sum() - (Ay.double() * x.double()).sum())) < 1e-6 * N
    ones = m._spmm(torch.ones(N, 64, device=DEV))
    rs = np.asarray(adj.sum(axis=1)).ravel()
    np.testing.assert_allclose(ones[:, 0].cpu().numpy(), rs, rtol=1e-5, atol=1e-6)
    # first steps of epoch 1 vs the reference's recorded per-step losses
    bpr = pkg.utils.BPRLoss(m, w.config)
    users, pos, neg = pkg.Procedure.sample_epoch_to_device(ds, DEV)
    assert users[:5].cpu().tolist() == meta["trajectory"][0]["shuf_users_head"]
    losses = m.fused_epoch(users[:2048 * 20], pos[:2048 * 20], neg[:2048 * 20], 2048)[:, 0].cpu().numpy()
    np.testing.assert_allclose(losses, zl["losses_epoch1"][:20], rtol=0, atol=5e-6)
    m.check_device_errors()


def test_row_order_changes_no_bit(pkg, lastfm, tmp_path):
    """The processing order is a pure scheduling choice: SpMM output, a whole training step and
    the propagated table are bit-identical for natural / rcm / cocluster orders."""
    g = lastfm
    outs = []
    for order in ("natural", "rcm", "cocluster"):
        ds, m = _make_model(pkg, g, tmp_path, row_order=order)
        x = torch.from_numpy(g.e0()).to(DEV)
        y = m._spmm(x).cpu().numpy()
        m.fused_step(_dev(g.z["b_users"], torch.int32), _dev(g.z["b_pos"], torch.int32), _dev(g.z["b_neg"], torch.int32))
        with torch.no_grad():
            au, ai = m.computer()
        outs.append((y, m._table.cpu().numpy().copy(), au.cpu().numpy()))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("act_dtype", ["fp32", "bf16"])
def test_gowalla_10_epoch_trajectory_vs_reference(pkg, tmp_path, act_dtype):
    """BASELINE.json north_star: Recall@20 / NDCG@20 within 1e-4 of the reference on the same seed.
    Ten full Gowalla epochs (3 940 steps) through Procedure.BPR_train_original + Procedure.Test
    against the trajectory captured by importing the reference (golden_long.json: cpp-mode
    sampler, seed 2020): average epoch loss and the metrics after epochs 1, 2, 5 and 10.
    fp32 activations reproduce the reference's Recall/NDCG to < 1e-8; bf16 activation storage
    stays within 1e-4 too (measured 7e-6 after 10 epochs)."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import materialize_gowalla
    meta = json.load(open(os.path.join(GOLDEN, "gowalla", "golden_long.json")))
    d = materialize_gowalla(os.path.join(GOLDEN, "gowalla", "gowalla.npz"), os.path.join(str(tmp_path), "gowalla"))
    w = pkg.world
    w.configure(["--dataset", "gowalla", "--tensorboard", "0", "--act_dtype", act_dtype,
                 "--checkpoint_dir", os.path.join(str(tmp_path), "ckpt")])
    ds = pkg.dataloader.Loader(w.config, path=d)
    pkg.sampling.seed(w.seed); pkg.utils.set_seed(w.seed)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    bpr = pkg.utils.BPRLoss(m, w.config)
    tol_loss = 2e-5 if act_dtype == "fp32" else 2e-4
    for rec in meta["trajectory"]:
        e = rec["epoch"]
        info = pkg.Procedure.BPR_train_original(ds, m, bpr, e)
        losses_path = os.path.join(w.config['checkpoint_dir'], 'train_epoch_metrics.csv')
        last = open(losses_path).read().strip().splitlines()[-1].split(",")
        # the reference averages over the true step count; the Procedure divides by len//B+1 (same for 394 steps)
        assert abs(float(last[1]) - rec["avg_loss"]) < tol_loss, (e, last, rec["avg_loss"])
        if "test" in rec:
            r = pkg.Procedure.Test(ds, m, e)
            for k in ("precision", "recall", "ndcg"):
                assert abs(float(r[k][0]) - rec["test"][k][0]) < 1e-4, (act_dtype, e, k, r[k], rec["test"][k])
            if act_dtype == "fp32":
                assert abs(float(r["recall"][0]) - rec["test"]["recall"][0]) < 1e-6


def _write_synth(path, n_users, m_items, seed, max_deg):
    rng = np.random.Generator(np.random.PCG64(seed))
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "train.txt"), "w") as f, open(os.path.join(path, "test.txt"), "w") as ft:
        for u in range(n_users):
            k = int(rng.integers(1, max_deg)) if u % 37 else min(m_items - 1, 6 * max_deg)      # some long rows
            items = np.sort(rng.choice(m_items, size=k, replace=False))
            f.write(f"{u} " + " ".join(map(str, items.tolist())) + "\n")
            ft.write(f"{u} {int(rng.integers(0, m_items))}\n")
        f.write(f"{n_users - 1} {m_items - 1}\n") if False else None


@pytest.mark.parametrize("d,K,act", [(32, 2, "fp32"), (128, 4, "fp32"), (256, 3, "fp32"), (128, 3, "bf16")])
def test_fused_steps_other_dims_vs_oracle(pkg, oracle, tmp_path, d, K, act):
    """BASELINE configs[3]/[4] shapes in miniature: dim 128 (4 layers) and 256, plus dim 32, on a
    synthetic bipartite graph with split (long) rows: 3 fused steps vs the oracle's stageOne."""
    path = os.path.join(str(tmp_path), f"synth{d}")
    _write_synth(path, 700, 900, d, 24)
    w = pkg.world
    w.configure(["--dataset", "synth", "--tensorboard", "0", "--layer", str(K), "--recdim", str(d),
                 "--bpr_batch", "256", "--act_dtype", act, "--row_order", "rcm"])
    ds = pkg.dataloader.Loader(w.config, path=path)
    pkg.utils.set_seed(7)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    adj = ds.getSparseGraphCSR()
    e0 = m._table.cpu().numpy().copy()
    tr = oracle.Trainer(ds.n_users, adj.indptr, adj.indices, adj.data, e0, K, w.config['decay'], w.config['lr'])
    bpr = pkg.utils.BPRLoss(m, w.config)
    rng = np.random.Generator(np.random.PCG64(1))
    tol = 3e-6 if act == "fp32" else 3e-4
    for step in range(3):
        nb = [256, 256, 100][step]
        u = rng.integers(0, ds.n_users, nb); p = rng.integers(0, ds.m_items, nb); n = rng.integers(0, ds.m_items, nb)
        l_ref = tr.stageOne(u, p, n)
        l_got = bpr.stageOne(_dev(u), _dev(p), _dev(n))
        assert abs(l_got - l_ref) < tol * 10, (step, l_got, l_ref)
        np.testing.assert_allclose(m._table.cpu().numpy(), tr.e0, rtol=0, atol=tol if act == "fp32" else 2e-3)
    with torch.no_grad():
        au, ai = m.computer()
    ref = oracle.propagate(adj.indptr, adj.indices, adj.data, tr.e0, K)
    np.testing.assert_allclose(torch.cat([au, ai]).cpu().numpy(), ref, rtol=2e-5 if act == "fp32" else 3e-2,
                               atol=2e-6 if act == "fp32" else 3e-3)
    m.check_device_errors()


@pytest.mark.parametrize("hub", [0, 200])
@pytest.mark.parametrize("d,K,act", [(64, 3, "fp32"), (32, 1, "fp32"), (256, 2, "fp32"), (128, 3, "bf16")])
def test_triplet_kernel_unit_boundaries(pkg, oracle, tmp_path, d, K, act, hub):
    """k_triplet cuts a slot row into units of 128 non-zeros dealt to the workgroup's four waves: batches whose user /
    positive / negative rows sit exactly on and around every unit and wave-wrap boundary (1 ... 1300 non-zeros,
    item hubs of 350 / 700 / 1400), duplicates of the same hub in one batch, vs the oracle's stageOne."""
    # hub = 200: rows with more than 200 non-zeros take the hub plan (k_spmm computes their last-layer rows for k_triplet to
    # read) -- the production threshold is 131 072 and only the 10M x 1M graph crosses it (tests/test_gpu_large.py runs that)
    lens = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 640, 1025, 1300]
    n_users = m_items = 1400
    path = os.path.join(str(tmp_path), f"units{d}")
    os.makedirs(path, exist_ok=True)
    rng = np.random.Generator(np.random.PCG64(d + K))
    with open(os.path.join(path, "train.txt"), "w") as f, open(os.path.join(path, "test.txt"), "w") as ft:
        for u in range(n_users):
            if u < len(lens):
                items = np.arange(lens[u])                                  # exactly lens[u] non-zeros, hub items included
            else:
                base = [0, 1] + ([2] if u % 2 == 0 else []) + ([3] if u % 4 == 0 else [])
                extra = 4 + rng.choice(m_items - 4, size=int(rng.integers(1, 20)), replace=False)
                items = np.unique(np.concatenate([np.asarray(base, dtype=np.int64), extra]))
            f.write(f"{u} " + " ".join(map(str, items.tolist())) + "\n")
            ft.write(f"{u} {int(rng.integers(0, m_items))}\n")
    w = pkg.world
    w.configure(["--dataset", "units", "--tensorboard", "0", "--layer", str(K), "--recdim", str(d),
                 "--bpr_batch", "128", "--act_dtype", act, "--dense_last", "0", "--hub_nnz", str(hub if hub else -1)])
    ds = pkg.dataloader.Loader(w.config, path=path)
    pkg.utils.set_seed(3)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    adj = ds.getSparseGraphCSR()
    deg = np.diff(adj.indptr)
    assert sorted(set(deg[:len(lens)].tolist())) == sorted(lens) and deg[n_users] >= 1380 and 650 < deg[n_users + 2] < 760
    tr = oracle.Trainer(ds.n_users, adj.indptr, adj.indices, adj.data, m._table.cpu().numpy().copy(), K, w.config['decay'], w.config['lr'])
    bpr = pkg.utils.BPRLoss(m, w.config)
    tol = 3e-6 if act == "fp32" else 3e-4
    for step in range(3):
        u = np.concatenate([np.arange(len(lens)), rng.integers(0, n_users, 108 - len(lens) + 20 * (step == 0))])[:128 if step else 100]
        p = np.concatenate([np.asarray([0, 0, 1, 2, 3, 2, 0, 3]), rng.integers(0, m_items, len(u) - 8)])      # hub positives, duplicated
        n = np.concatenate([rng.integers(0, m_items, len(u) - 4), np.asarray([1, 2, 3, 0])])
        l_ref = tr.stageOne(u, p, n)
        l_got = bpr.stageOne(_dev(u), _dev(p), _dev(n))
        assert abs(l_got - l_ref) < tol * 10, (step, l_got, l_ref)
        np.testing.assert_allclose(m._table.cpu().numpy(), tr.e0, rtol=0, atol=tol if act == "fp32" else 2e-3)
    m.check_device_errors()


@pytest.mark.parametrize("path", ["fused", "autograd"])
@pytest.mark.parametrize("tag", ["gate", "i2i", "gate_i2i", "gate_i2i_k1", "gate_i2i_k2", "gate_i2i_k4"])
def test_optional_branches_vs_reference_golden(pkg, tiny, tmp_path, tag, path):
    """the fork's popularity gate (model.py:66-96,139-157,176-181) and item-item smoothing
    (model.py:99-109,228-229) against fixtures captured from the reference itself on the tiny dataset
    (tests/golden/make_golden.py tiny_gate / tiny_i2i / tiny_gate_i2i at K = 3, and tiny_gate_i2i_k1 / _k2 / _k4: both branches at the other
    depths -- K = 1 keeps one row bitmap and ends in k_finish, 2 / 4 alternate two): initial parameters bit for bit (same
    modules built in the same order from seed 2020), computer(), ratings, Test metrics, bpr_loss and the
    gradient of EVERY parameter, then three stageOne steps and the metrics after.
    path = "fused": the branches run INSIDE the fused HIP step (k_mean_layers, the item-item SpMMs, k_triplet_gate,
    k_gate_adam): loss / reg of the reference's first batch, the gradient of every MLP parameter (the step's reduced
    gradient buffer) against the reference's autograd gradients, the three steps' losses and EVERY parameter after them,
    optimizer state in torch-Adam format.  path = "autograd": --fused_variants 0, the reference's own sequence (torch
    MLPs, torch Adam) around the HIP propagation kernels."""
    gz = np.load(os.path.join(tiny.dir, f"golden_{tag}.npz"))
    meta = json.load(open(os.path.join(tiny.dir, f"golden_{tag}.json")))
    d = os.path.join(str(tmp_path), "tiny_" + tag)
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(tiny.dir, f), os.path.join(d, f))
    w = pkg.world
    w.configure([])
    w.dataset = "tiny"
    w.config.update({'lightGCN_n_layers': meta["K"], 'latent_dim_rec': meta["d"], 'bpr_batch_size': meta["B"], 'decay': meta["decay"],
                     'lr': meta["lr"], 'use_pop_gate': meta["use_pop_gate"], 'use_item_item': meta["use_item_item"],
                     'i2i_path': os.path.join(tiny.dir, "i2i_tiny.npz") if meta["use_item_item"] else None, 'i2i_alpha': meta["i2i_alpha"],
                     'eval_fused': 1, 'fused_variants': 1 if path == "fused" else 0})
    w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=d)

    def fresh():
        pkg.utils.set_seed(meta["seed"])
        return pkg.model.LightGCN(w.config, ds).to(DEV)
    m = fresh()
    assert m.has_variants and m.fused_variants == (path == "fused")
    sd = m.state_dict()
    assert sorted(sd) == sorted(k[3:] for k in gz.files if k.startswith("P0."))          # the reference's keys
    for k, v in sd.items():
        assert np.array_equal(v.cpu().numpy(), gz["P0." + k]), k
    m.eval()
    with torch.no_grad():
        au, ai = m.computer()
        np.testing.assert_allclose(au.cpu().numpy(), gz["computer_users"], rtol=2e-5, atol=2e-7)
        np.testing.assert_allclose(ai.cpu().numpy(), gz["computer_items"], rtol=2e-5, atol=2e-7)
        np.testing.assert_allclose(m.getUsersRating(torch.arange(10, device=DEV)).cpu().numpy(), gz["rating_users_0_9"], rtol=1e-4, atol=2e-6)
    for fused in (1, 0):                       # the MFMA top-K kernels and the torch harness both see the final item table
        w.config['eval_fused'] = fused
        r = pkg.Procedure.Test(ds, m, 0)
        for k in ("precision", "recall", "ndcg"):
            np.testing.assert_allclose(np.asarray(r[k], np.float64), meta["test_epoch0"][k], rtol=0, atol=1e-6)
    m.train()
    b = gz["batches"]
    if path == "autograd":
        loss, reg = m.bpr_loss(_dev(b[0, 0]), _dev(b[0, 1]), _dev(b[0, 2]))
        assert abs(float(loss) - meta["b_loss"]) < 2e-6 and abs(float(reg) - meta["b_reg"]) < 2e-6
        m.zero_grad()
        (loss + reg * meta["decay"]).backward()
        for k, prm in m.named_parameters():
            np.testing.assert_allclose(prm.grad.cpu().numpy(), gz["G0." + k], rtol=5e-4, atol=2e-8, err_msg=k)
        m.zero_grad()
    else:
        # the reference's first batch through the fused step: loss, reg and the MLP gradients the step itself reduced
        out = m.fused_step(_dev(b[0, 0]), _dev(b[0, 1]), _dev(b[0, 2])).cpu().numpy()
        assert abs(float(out[1]) - meta["b_loss"]) < 2e-6 and abs(float(out[2]) - meta["b_reg"]) < 2e-6 and abs(float(out[0]) - meta["b_total"]) < 2e-6, (out, meta["b_loss"], meta["b_reg"])
        if meta["use_pop_gate"]:
            gg = m._dev['gate_grad'].cpu().numpy()
            off = 0
            for k, prm in m.named_parameters():
                if k.startswith("embedding"):
                    continue
                want = gz["G0." + k]
                np.testing.assert_allclose(gg[off:off + want.size].reshape(want.shape), want, rtol=5e-4, atol=2e-8, err_msg=k)
                off += want.size
            assert off == gg.size
        m.check_device_errors()
        assert not bool(m._dev['G64'].any())
        m = fresh()                            # the three recorded steps start from the initial parameters
        m.train()
    bpr = pkg.utils.BPRLoss(m, w.config)
    assert bpr.fused == (path == "fused")
    for i in range(3):
        l = bpr.stageOne(_dev(b[i + 1, 0]), _dev(b[i + 1, 1]), _dev(b[i + 1, 2]))
        assert abs(l - meta["step_losses"][i]) < 5e-6, (i, l, meta["step_losses"][i])
    for k, v in m.state_dict().items():
        np.testing.assert_allclose(v.cpu().numpy(), gz["P3." + k], rtol=0, atol=2e-5, err_msg=k)
    r = pkg.Procedure.Test(ds, m, 0)
    for k in ("precision", "recall", "ndcg"):
        np.testing.assert_allclose(np.asarray(r[k], np.float64), meta["test_after3"][k], rtol=0, atol=1e-4)
    if path == "fused":
        m.check_device_errors()
        osd = bpr.opt.state_dict()            # torch-Adam format over ALL parameters, step = 3
        names = [k for k, _ in m.named_parameters()]
        assert len(osd['state']) == len(names)
        for i, k in enumerate(names):
            assert int(osd['state'][i]['step']) == 3 and tuple(osd['state'][i]['exp_avg'].shape) == tuple(gz["P0." + k].shape), k
            assert float(osd['state'][i]['exp_avg_sq'].abs().sum()) > 0, k
    else:
        with pytest.raises(RuntimeError):
            m.fused_step(_dev(b[0, 0]), _dev(b[0, 1]), _dev(b[0, 2]))
    w.configure([])


@pytest.mark.parametrize("act", ["fp32", "bf16"])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("tag", ["gate", "i2i", "gate_i2i"])
def test_optional_branches_fused_vs_autograd_other_depths(pkg, tiny, tmp_path, tag, K, act):
    """The reference's fixtures pin the optional branches at K = 3, fp32.  Other depths -- K = 1 keeps ONE row bitmap and ends
    in k_finish, K = 2 / 4 alternate two -- and bf16 activation storage: the fused step against the autograd path (the
    reference's own sequence around the HIP propagation kernels, itself pinned at K = 3), same seed, same five batches with
    duplicated ids: every step's loss and EVERY parameter afterwards, G64 left clean."""
    meta = json.load(open(os.path.join(tiny.dir, f"golden_{tag}.json")))
    d = os.path.join(str(tmp_path), f"tiny_{tag}_{K}")
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(tiny.dir, f), os.path.join(d, f))
    w = pkg.world
    rng = np.random.Generator(np.random.PCG64(31 * K + len(tag)))
    ds0 = None
    batches = None
    out = {}
    for fused in (1, 0):
        w.configure([])
        w.dataset = "tiny"
        w.config.update({'lightGCN_n_layers': K, 'latent_dim_rec': meta["d"], 'bpr_batch_size': 64, 'decay': meta["decay"], 'lr': meta["lr"],
                         'use_pop_gate': meta["use_pop_gate"], 'use_item_item': meta["use_item_item"], 'act_dtype': act,
                         'i2i_path': os.path.join(tiny.dir, "i2i_tiny.npz") if meta["use_item_item"] else None, 'i2i_alpha': meta["i2i_alpha"],
                         'fused_variants': fused})
        w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
        ds = pkg.dataloader.Loader(w.config, path=d)
        if batches is None:
            batches = []
            for nb in (64, 64, 33, 64, 1):
                u = rng.integers(0, ds.n_users, nb); p = rng.integers(0, ds.m_items, nb); n = rng.integers(0, ds.m_items, nb)
                if nb > 8:
                    p[:4] = p[4]; n[5] = p[4]; u[7] = u[6]
                batches.append((u, p, n))
        pkg.utils.set_seed(meta["seed"])
        m = pkg.model.LightGCN(w.config, ds).to(DEV)
        m.train()
        bpr = pkg.utils.BPRLoss(m, w.config)
        assert bpr.fused == bool(fused)
        losses = [bpr.stageOne(_dev(u), _dev(p), _dev(n)) for (u, p, n) in batches]
        if fused:
            m.check_device_errors()
            assert not bool(m._dev['G64'].any())
        out[fused] = (losses, {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()})
        del bpr, m
    ltol, ptol = (5e-6, 2e-5) if act == "fp32" else (2e-3, 2e-3)       # bf16: the two paths round different layers to 2 bytes
    for a, b in zip(out[1][0], out[0][0]):
        assert abs(a - b) < ltol, (tag, K, act, out[1][0], out[0][0])
    for k in out[1][1]:
        np.testing.assert_allclose(out[1][1][k], out[0][1][k], rtol=0, atol=ptol, err_msg=f"{tag} K={K} {act} {k}")
    w.configure([])


def test_checkpoint_resume_roundtrip(pkg, tiny, tmp_path):
    """Checkpoint surface of main.py:56-87: model.state_dict() (keys embedding_user/item.weight) +
    bpr.opt.state_dict() (torch-Adam format: step / exp_avg / exp_avg_sq) saved after 2 steps,
    loaded into a fresh model, third step bitwise equal to the uninterrupted run."""
    g = tiny
    rng = np.random.Generator(np.random.PCG64(9))
    batches = [tuple(_dev(rng.integers(0, hi, 64), torch.int32) for hi in (g.n_users, g.m_items, g.m_items)) for _ in range(3)]
    ds, m = _make_model(pkg, g, tmp_path)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    for b in batches[:2]:
        bpr.stageOne(*b)
    ckpt = os.path.join(str(tmp_path), "last.pth.tar")
    torch.save({'epoch': 1, 'model_state': m.state_dict(), 'optimizer_state': bpr.opt.state_dict()}, ckpt + ".tmp")
    os.replace(ckpt + ".tmp", ckpt)
    l3 = bpr.stageOne(*batches[2])
    want = m._table.cpu().numpy().copy()
    sd = torch.load(ckpt, weights_only=True)
    assert list(sd['model_state'].keys()) == ['embedding_user.weight', 'embedding_item.weight']
    st = sd['optimizer_state']['state']
    assert int(st[0]['step']) == 2 and st[0]['exp_avg'].shape == (g.n_users, g.d) and st[1]['exp_avg_sq'].shape == (g.m_items, g.d)
    ds2, m2 = _make_model(pkg, g, tmp_path)
    bpr2 = pkg.utils.BPRLoss(m2, pkg.world.config)
    m2.load_state_dict(sd['model_state'])
    bpr2.opt.load_state_dict(sd['optimizer_state'])
    assert m2.adam_step == 2
    l3b = bpr2.stageOne(*batches[2])
    assert l3 == l3b and np.array_equal(m2._table.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a plain torch Adam can read the same state (interchange with the reference's optimizer)
    ref_opt = torch.optim.Adam(m2.parameters(), lr=pkg.world.config['lr'])
    ref_opt.load_state_dict(bpr2.opt.state_dict())
    assert int(ref_opt.state_dict()['state'][0]['step']) == 3


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_spmm_row_length_boundaries(pkg, oracle, d):
    """Row lengths on both sides of every internal boundary of the SpMM kernel, derived from its
    constants LONG_T = 64 (one index tile: the short-row path) and LONG_CH = 512 (one chunk): rows of
    65..512 non-zeros are finished by one wave, 513.. go through the partial-row hand-off with 2, 3 and
    4 chunks (1023/1024/1025, 1537), plus empty rows, in every position of the 4-rows-per-wave /
    4-waves-per-workgroup tiling, for the natural order, a random order and a random order with an
    explicit (deliberately uneven) XCD cut."""
    rng = np.random.Generator(np.random.PCG64(100 + d))
    lens = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193,
            255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 1537, 0, 64, 65, 512, 513, 7, 7, 7]
    n = 1600
    deg = np.array([lens[i % len(lens)] for i in range(n)], np.int64)
    deg = deg[rng.permutation(n)]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in deg]).astype(np.int32)
    vals = rng.uniform(0.01, 0.4, len(indices)).astype(np.float32)
    X = rng.normal(0, 0.1, (n, d)).astype(np.float32)
    ref = oracle.spmm(indptr, indices, vals, X)
    bound = spmm_sum_bound(indptr, vals, indices, X)
    first = None
    cut = np.array([0, 10, 10, 300, 700, 701, 1200, 1599, 1600], np.int64)
    for order, xs in ((None, None), (rng.permutation(n).astype(np.int32), None), (rng.permutation(n).astype(np.int32), cut)):
        g = pkg._lib.Graph(_dev(indptr), _dev(indices), _dev(vals), d_max=d, row_order=order, xcd_start=xs)
        got = g.spmm(_dev(X)).cpu().numpy()
        # bound per row = (2 n + 2) * 2^-24 * sum |v x|: two fp32 summation orders of the same n terms (conftest.spmm_sum_bound)
        assert_rows_close(got, ref, bound, "first launch")
        again = g.spmm(_dev(2.0 * X)).cpu().numpy()    # other data through the same scratch: tickets were reset, no stale partial
        assert_rows_close(again, 2.0 * ref, 2.0 * bound, "doubled data")
        third = g.spmm(_dev(X)).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), third.view(np.uint32))
        if first is None:
            first = got
        assert np.array_equal(first.view(np.uint32), got.view(np.uint32))      # order / XCD cut change no bit
        g.close()
    assert np.array_equal(got[deg == 0], np.zeros_like(got[deg == 0]))
    with pytest.raises(pkg._lib.LgcnError):
        pkg._lib.Graph(_dev(indptr), _dev(indices), _dev(vals), d_max=d, xcd_start=np.array([0, 5, 4, 9, 9, 9, 9, 9, n]))
    bad = indices.copy(); bad[3] = n
    with pytest.raises(pkg._lib.LgcnError, match="column index"):
        pkg._lib.Graph(_dev(indptr), _dev(bad), _dev(vals), d_max=d)
    g = pkg._lib.Graph(_dev(indptr), _dev(indices), _dev(vals), d_max=d)
    with pytest.raises(pkg._lib.LgcnError):
        g.spmm(_dev(X[:-1]))                                                       # short X
    g.close()


@pytest.mark.parametrize("d,bf16", [(64, False), (64, True), (128, False), (256, True), (32, False)])
def test_spmm_hub_rows_forty_chunks(pkg, oracle, d, bf16):
    """Heavy-tail rows (the synthetic Yelp/Amazon shapes have 19-45-chunk rows): rows of 20 500 and
    9 700 non-zeros = 41 and 19 chunks of 512 whose partial rows meet through the write-through
    hand-off on different XCDs, checked against the oracle with DIFFERENT data on every launch (a
    stale or missed partial cannot hide behind identical values), 6 launches back to back."""
    rng = np.random.Generator(np.random.PCG64(7 + d))
    n = 24000
    deg = rng.poisson(6, n).astype(np.int64)
    deg[[5, 11000, 23999]] = [20500, 9700, 513]
    indptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(n, size=k, replace=False)) for k in deg]).astype(np.int32)
    vals = rng.uniform(0.001, 0.05, len(indices)).astype(np.float32)
    g = pkg._lib.Graph(_dev(indptr), _dev(indices), _dev(vals), d_max=d, row_order=rng.permutation(n).astype(np.int32))
    for it in range(6):
        X = rng.normal(0, 0.1, (n, d)).astype(np.float32)
        x = _dev(X)
        if bf16:
            x = x.to(torch.bfloat16)
            X = x.float().cpu().numpy()
        got = g.spmm(x, 0).cpu().numpy()
        ref = oracle.spmm(indptr, indices, vals, X)
        np.testing.assert_allclose(got, ref, rtol=3e-5, atol=2e-6, err_msg=f"launch {it}")
    g.close()


def _synthetic_model(pkg, name, act="fp32", row_order="xcd"):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    n_users, m_items, E, K, d, B = bench.WORKLOADS[name][:6]
    w = pkg.world
    w.configure(["--dataset", name, "--tensorboard", "0", "--layer", str(K), "--recdim", str(d), "--bpr_batch", str(B),
                 "--act_dtype", act, "--row_order", row_order])
    ds = bench.synthetic_dataset(pkg, name, w.config, DEV)
    pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    return ds, m, K, d, B


@pytest.mark.parametrize("name", ["yelp2018-shaped", "amazon-book-shaped"])
def test_full_shape_synthetic_configs_vs_oracle(pkg, oracle, name):
    """BASELINE configs[2] (Yelp2018 shape: 31 668 x 38 048, E = 1 237 259, K = 3, d = 64, B = 8192) and
    configs[3] (Amazon-Book shape: 52 643 x 91 599, E = 2 380 730, K = 4, d = 128, B = 2048) at FULL
    size on the seeded synthetic graph (the real train splits are absent from the reference checkout):
    native sampler triplets, 3 fused steps vs the oracle's stageOne (loss 5e-6, parameters 1e-5), the
    propagated table vs the oracle, a second identical run bit for bit, and the data-parallel split
    (world = 2, 4, 8 emulated on one GPU) bit for bit.  These graphs have 19-45-chunk hub rows."""
    ds, m, K, d, B = _synthetic_model(pkg, name)
    adj = ds.getSparseGraphCSR()
    assert np.diff(adj.indptr).max() > 19 * 512
    e0 = m._table.cpu().numpy().copy()
    S = pkg.utils.UniformSample_original(ds)[:3 * B]
    assert S.shape == (3 * B, 3) and S.dtype == np.int32
    tr = oracle.Trainer(ds.n_users, adj.indptr, adj.indices, adj.data, e0, K, pkg.world.config['decay'], pkg.world.config['lr'])
    batches = [tuple(_dev(np.ascontiguousarray(S[i * B:(i + 1) * B, c]), torch.int32) for c in range(3)) for i in range(3)]
    losses = []
    for i, (u, p, n) in enumerate(batches):
        l_ref = tr.stageOne(S[i * B:(i + 1) * B, 0], S[i * B:(i + 1) * B, 1], S[i * B:(i + 1) * B, 2])
        l_got = m.fused_step(u, p, n).cpu().numpy()
        losses.append(l_got.copy())
        assert abs(float(l_got[0]) - l_ref) < 5e-6, (i, l_got, l_ref)
        np.testing.assert_allclose(m._table.cpu().numpy(), tr.e0, rtol=0, atol=1e-5)
    with torch.no_grad():
        au, ai = m.computer()
    ref = oracle.propagate(adj.indptr, adj.indices, adj.data, tr.e0, K)
    np.testing.assert_allclose(torch.cat([au, ai]).cpu().numpy(), ref, rtol=3e-5, atol=3e-7)
    m.check_device_errors()
    want = m._table.cpu().numpy().copy()

    L, lib = pkg._lib, pkg._lib.load()
    for world in (1, 2, 4, 8):
        ds2, m2, *_ = _synthetic_model(pkg, name)
        assert np.array_equal(m2._table.cpu().numpy(), e0)
        for i, (u, p, n) in enumerate(batches):
            if world == 1:
                out = m2.fused_step(u, p, n)
            else:
                st = m2._state(max_batch=B, need_ctx=True, dp_world=world)
                nblk = pkg.parallel.block_numel(B, world, d)
                blocks = []
                for r in range(world):
                    L.check(lib.lgcn_train_step_dp_part1(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, r, L.current_stream()), "part1")
                    blocks.append(st['contrib'][:nblk].clone())
                out = torch.empty(3, device=DEV)
                L.check(lib.lgcn_train_step_dp_part2(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, L.tp(torch.cat(blocks)),
                                                     L.tp(out), L.current_stream()), "part2")
            np.testing.assert_allclose(out.cpu().numpy(), losses[i], rtol=0, atol=1e-6)
        assert np.array_equal(m2._table.cpu().numpy().view(np.uint32), want.view(np.uint32)), world
        del m2, ds2


def test_dp_empty_trailing_shard(pkg, tiny, tmp_path):
    """A short last batch can leave trailing ranks without triplets (B = 2 on 3 ranks: shard 1, rank 2
    empty).  Such a rank launches no BPR kernel but must still clear the row bitmap of two steps ago;
    its tables and bitmaps stay identical to the other ranks' and to the single-GPU run."""
    g = tiny
    rng = np.random.Generator(np.random.PCG64(4))
    batches = [(rng.integers(0, g.n_users, b), rng.integers(0, g.m_items, b), rng.integers(0, g.m_items, b)) for b in (64, 64, 2, 2)]
    L, lib = pkg._lib, pkg._lib.load()
    ds, ref = _make_model(pkg, g, tmp_path)
    for (u, p, n) in batches:
        ref.fused_step(_dev(u, torch.int32), _dev(p, torch.int32), _dev(n, torch.int32))
    world = 3
    ranks = [_make_model(pkg, g, tmp_path)[1] for _ in range(world)]
    for (u, p, n) in batches:
        u, p, n = (_dev(x, torch.int32) for x in (u, p, n))
        B = len(u)
        nblk = pkg.parallel.block_numel(B, world, g.d)
        sts = [m._state(max_batch=64, need_ctx=True, dp_world=world) for m in ranks]
        blocks = []
        for r, st in enumerate(sts):
            L.check(lib.lgcn_train_step_dp_part1(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, r, L.current_stream()), "part1")
            blocks.append(st['contrib'][:nblk].clone() if r * pkg.parallel.shard_size(B, world) < B else torch.zeros(nblk, device=DEV))
        gathered = torch.cat(blocks)
        for st in sts:
            out = torch.empty(3, device=DEV)
            L.check(lib.lgcn_train_step_dp_part2(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, L.tp(gathered), L.tp(out),
                                                 L.current_stream()), "part2")
    torch.cuda.synchronize()
    for m in ranks:
        assert np.array_equal(m._table.cpu().numpy().view(np.uint32), ref._table.cpu().numpy().view(np.uint32))
        assert torch.equal(m._dev['bitmap'], ranks[0]._dev['bitmap'])
        assert int(m._dev['G64'].abs().sum()) == 0


@pytest.mark.parametrize("m_items,d,K,n_eval", [(5000, 64, 20, 300), (4100, 32, 7, 130), (200000, 64, 20, 160), (9000, 64, 25, 129),
                                                (6000, 128, 20, 200), (9000, 64, 50, 200), (7000, 32, 64, 129), (3000, 64, 50, 140),
                                                (6000, 128, 50, 130), (150000, 64, 50, 130)])
def test_eval_topk_every_sweep_form_vs_torch(pkg, m_items, d, K, n_eval):
    """lgcn_eval_topk on synthetic tables, one case per form of the item sweep: three workgroups per user block with compact
    lists (16-bit ids relative to the part's first item; d <= 64, K <= 20), two with int32 ids (parts too long for 16 bits),
    one (d > 64 with K > 20, or a catalogue under 4096 items); K = 25 / 50 / 64 (Procedure.py:183 takes k = max(topks): --topks "[20,50]")
    on two workgroups per block with 64-slot lists, and on the generic form at d = 128 and on 150 000 items.  Every case also
    through lgcn_eval_topk_masked (train-positive masks precomputed by lgcn_eval_build_masks instead of the in-sweep cursor):
    bit-identical lists.  Train positives clustered inside single 32-item tiles, at the part boundaries and at the table's
    end; an unsorted, repeating user list.  Against torch matmul + mask + topk: same ids in the same order except where two
    scores tie within fp32 rounding, masked items never returned."""
    L, lib = pkg._lib, pkg._lib.load()
    rng = np.random.Generator(np.random.PCG64(m_items + d + K))
    n_users = 400
    E = torch.from_numpy(rng.standard_normal((n_users + m_items, d)).astype(np.float32)).to(DEV)
    users = rng.integers(0, n_users, n_eval).astype(np.int32)
    ntiles = (m_items + 31) // 32
    rows = []
    for u in range(n_users):
        c = set(rng.integers(0, m_items, rng.integers(0, 40)).tolist())
        t0 = int(rng.integers(0, ntiles - 1)) * 32
        c |= set(range(t0 + int(rng.integers(0, 8)), min(m_items, t0 + 32 + int(rng.integers(0, 20)))))      # a cluster across a tile edge
        for parts in (2, 3):
            b = (ntiles * (u % parts) // parts) * 32                                                     # around a part boundary
            c |= {min(m_items - 1, max(0, b - 1)), min(m_items - 1, b), min(m_items - 1, b + 1)}
        if u % 7 == 0:
            c |= {m_items - 1, m_items - 2}
        if u % 11 == 0:
            c = set()
        rows.append(np.array(sorted(c), np.int32))
    ptr = np.zeros(n_users + 1, np.int64); ptr[1:] = np.cumsum([len(r) for r in rows])
    idx = np.concatenate(rows).astype(np.int32)
    topk = torch.full((n_eval, K), -7, dtype=torch.int32, device=DEV)
    sc = torch.empty(n_eval, K, dtype=torch.float32, device=DEV)
    d_users, d_ptr, d_idx = _dev(users), _dev(ptr), _dev(idx)        # (named: a temporary's memory is reused by the next allocation)
    assert d_users.dtype == torch.int32 and d_ptr.dtype == torch.int64 and d_idx.dtype == torch.int32
    assert int(d_users.max()) < n_users and int(d_ptr[-1]) == d_idx.numel() and int(d_idx.max()) < m_items and E.shape == (n_users + m_items, d)
    L.check(lib.lgcn_eval_topk(L.tp(E), n_users, m_items, d, L.tp(d_users), n_eval, L.tp(d_ptr), L.tp(d_idx), K,
                               L.tp(topk), L.tp(sc), L.current_stream()), "lgcn_eval_topk")
    torch.cuda.synchronize()
    exact = (E[:n_users][torch.from_numpy(users).long().to(DEV)].double() @ E[n_users:].double().t())   # fp64: no summation order
    for s, u in enumerate(users):
        exact[s, torch.from_numpy(rows[u]).long().to(DEV)] = -(1 << 10)
    want_sc, want = torch.topk(exact, K)
    got = topk.long()
    assert int(got.min()) >= 0 and int(got.max()) < m_items
    got_exact = torch.gather(exact, 1, got)
    # fp32 rounding of a d-term dot product accumulated in any order: <= d eps sum|a_k b_k| in the worst case; sqrt(d) of it for
    # rounding errors of random sign, taken twice (measured: 0.3 of this bound)
    tol = 2.0 * np.sqrt(d) * EPS32 * float(E[:n_users].norm(dim=1).max()) * float(E[n_users:].norm(dim=1).max())
    assert float((got_exact - sc.double()).abs().max()) < tol                      # the scores it reports are those items' scores
    assert bool((got_exact > -1000).all())                                         # no train positive returned (K << unmasked items)
    # rank by rank the same score up to that rounding (ids may swap only inside such a tie)
    assert float((got_exact - want_sc).abs().max()) < tol
    assert float((got == want).float().mean()) > 0.999
    assert bool((sc[:, :-1] >= sc[:, 1:]).all())
    for s in range(n_eval):
        assert len(set(got[s].tolist())) == K
    # the cross-check entry point (every score from the fp32 matrix instructions): the same lists up to ties within rounding
    topk32 = torch.full((n_eval, K), -7, dtype=torch.int32, device=DEV)
    sc32 = torch.empty(n_eval, K, dtype=torch.float32, device=DEV)
    L.check(lib.lgcn_eval_topk_fp32(L.tp(E), n_users, m_items, d, L.tp(d_users), n_eval, L.tp(d_ptr), L.tp(d_idx), K,
                                    L.tp(topk32), L.tp(sc32), L.current_stream()), "lgcn_eval_topk_fp32")
    assert float((topk32 == topk).float().mean()) > 0.999
    assert float((sc32.double() - sc.double()).abs().max()) < tol
    assert float((torch.gather(exact, 1, topk32.long()) - want_sc).abs().max()) < tol
    # precomputed train-positive masks instead of the cursor: the same kernel arithmetic, so the same bits
    words = int(lib.lgcn_eval_mask_words(m_items, n_eval))
    assert words == ((m_items + 31) // 32) * ((n_eval + 127) // 128 * 128)
    masks = torch.full((words,), -1, dtype=torch.int32, device=DEV)          # (build must zero it)
    L.check(lib.lgcn_eval_build_masks(L.tp(d_users), n_eval, L.tp(d_ptr), L.tp(d_idx), m_items, L.tp(masks), L.current_stream()), "masks")
    stride = (n_eval + 127) // 128 * 128
    mk = masks.view(ntiles, stride).cpu().numpy().view(np.uint32)
    for s_ in (0, n_eval // 2, n_eval - 1):
        want_bits = np.zeros(ntiles, np.uint32)
        for it in rows[users[s_]]:
            want_bits[it >> 5] |= np.uint32(1) << np.uint32(it & 31)
        assert np.array_equal(mk[:, s_], want_bits)
    assert not mk[:, n_eval:].any()
    topk_m = torch.full((n_eval, K), -7, dtype=torch.int32, device=DEV)
    sc_m = torch.empty(n_eval, K, dtype=torch.float32, device=DEV)
    L.check(lib.lgcn_eval_topk_masked(L.tp(E), n_users, m_items, d, L.tp(d_users), n_eval, L.tp(d_ptr), L.tp(d_idx), K,
                                      L.tp(topk_m), L.tp(sc_m), L.tp(masks), L.current_stream()), "lgcn_eval_topk_masked")
    assert torch.equal(sc_m, sc)
    assert float((topk_m == topk).float().mean()) > 0.9999          # (the parts' threshold exchange is timing dependent: an exact tie at the K-th place may pick the other id)


@pytest.mark.parametrize("which", ["lastfm", "tiny"])
def test_fused_eval_kernels_vs_torch_and_oracle(pkg, oracle, tiny, lastfm, tmp_path, which):
    """Procedure.Test through the fused kernels (fp32 matrix-core scores + train mask + running top-20,
    metrics on device) against (a) the torch matmul/topk harness on the same table: identical top-20
    SETS per user, scores of the ranked items within fp32 rounding, (b) the CPU oracle's full-ranking
    evaluation (Procedure.py:162-192 restated): precision / recall / NDCG to 1e-8."""
    g = lastfm if which == "lastfm" else tiny
    ds, m = _make_model(pkg, g, tmp_path)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    users, pos, neg = pkg.Procedure.sample_epoch_to_device(ds, DEV)
    m.fused_epoch(users, pos, neg, g.B)                     # a trained table separates the scores
    m.eval()
    pkg.world.config['eval_fused'] = 1
    r_fused = pkg.Procedure.Test(ds, m, 0)
    ev = ds._lgcn_eval_index
    with torch.no_grad():
        res, topk = pkg.Procedure._test_fused(m, ev, 20)
        E = m.propagated_table()
        rating = E[:ds.n_users][torch.from_numpy(ev.users).to(DEV)] @ E[ds.n_users:].t()
        row, p = ev._expand(ev.train_ptr, torch.from_numpy(ev.users).to(DEV))
        rating[row, ev.train_idx[p]] = -(1 << 10)
        sc, ref_topk = torch.topk(rating, 20)
    got = np.sort(topk.cpu().numpy(), axis=1); want = np.sort(ref_topk.cpu().numpy(), axis=1)
    same = (got == want).all(axis=1)
    # a differing set is legitimate only for a tie at the cut (20th vs 21st score within fp32 rounding)
    for u in np.flatnonzero(~same):
        s_u = rating[u]
        a_ = s_u[topk[u].long()].min().item(); b_ = sc[u].min().item()
        assert abs(a_ - b_) <= 1e-6 * max(1.0, abs(b_)), (u, a_, b_)
    assert same.mean() > 0.999
    got_sc = torch.gather(rating, 1, topk.long())
    assert torch.all(got_sc[:, :-1] >= got_sc[:, 1:] - 1e-6)                      # ranked best first
    pkg.world.config['eval_fused'] = 0
    r_torch = pkg.Procedure.Test(ds, m, 0)
    pkg.world.config['eval_fused'] = 1
    ref = oracle.test(E.cpu().numpy(), ds.n_users, ds._r_indptr, ds._r_indices, ds.testDict, 20)
    for k in ("precision", "recall", "ndcg"):
        assert abs(float(r_fused[k][0]) - float(r_torch[k][0])) < 1e-9, (k, r_fused[k], r_torch[k])
        assert abs(float(r_fused[k][0]) - ref[k]) < 1e-8, (k, r_fused[k], ref[k])
    # argument checks
    L = pkg._lib
    assert L.load().lgcn_eval_topk(L.tp(E), ds.n_users, ds.m_items, g.d, L.tp(ev.users32), len(ev.users), L.tp(ev.train_ptr),
                                   L.tp(ev.train_idx32), 65, L.tp(topk), None, L.current_stream()) == 3      # K <= 64


def test_procedure_test_masks_on_off_and_two_cutoffs(pkg, lastfm, tmp_path):
    """Procedure.Test through the fused kernels with the train-positive masks precomputed (default) and with the in-sweep cursor
    (--eval_masks 0): identical metrics; and with --topks "[20, 50]" (k = 50 stays on the fused path since round 4) against the
    torch harness."""
    g = lastfm
    ds, m = _make_model(pkg, g, tmp_path)
    users, pos, neg = pkg.Procedure.sample_epoch_to_device(ds, DEV)
    m.fused_epoch(users, pos, neg, g.B)
    m.eval()
    w = pkg.world
    res = {}
    for masks in (1, 0):
        w.config['eval_masks'] = masks
        ds._lgcn_eval_index = None
        res[masks] = pkg.Procedure.Test(ds, m, 0)
        assert (ds._lgcn_eval_index.masks is not None) == bool(masks)
    for k in ("precision", "recall", "ndcg"):
        assert float(res[1][k][0]) == float(res[0][k][0]), k
    w.config['eval_masks'] = 1
    old_topks = list(w.topks)
    try:
        w.topks = [20, 50]
        ds._lgcn_eval_index = None
        w.config['eval_fused'] = 1
        r_f = pkg.Procedure.Test(ds, m, 0)
        w.config['eval_fused'] = 0
        r_t = pkg.Procedure.Test(ds, m, 0)
        for k in ("precision", "recall", "ndcg"):
            assert r_f[k].shape == (2,) and np.abs(np.asarray(r_f[k], np.float64) - np.asarray(r_t[k], np.float64)).max() < 1e-9, (k, r_f[k], r_t[k])
            assert abs(float(r_f[k][0]) - float(res[1][k][0])) < 1e-12
    finally:
        w.topks = old_topks
        w.config['eval_fused'] = 1


@pytest.mark.parametrize("which,world", [("tiny", 2), ("tiny", 3), ("lastfm", 4)])
def test_row_sharded_step_bitwise_equals_unsharded(pkg, tiny, lastfm, tmp_path, which, world):
    """Row-sharded propagation (SURVEY 8e "beyond the contract") emulated on one GPU: `world` training
    contexts share ONE set of device buffers (what the in-place RCCL broadcasts of the owners' row ranges
    produce on every rank) but each holds a graph plan of only its own rows; the phases of
    include/lgcn_hip.h run rank after rank.  Three steps, tables + Adam state + losses identical to the
    unsharded single-GPU step bit for bit; the owned ranges partition the rows and balance the non-zeros."""
    g = tiny if which == "tiny" else lastfm
    L, lib = pkg._lib, pkg._lib.load()
    rng = np.random.Generator(np.random.PCG64(world))
    B = 64
    batches = [tuple(_dev(rng.integers(0, hi, b), torch.int32) for hi in (g.n_users, g.m_items, g.m_items)) for b in (B, B, 37)]
    ds, ref = _make_model(pkg, g, tmp_path)
    ref_losses = [ref.fused_step(*b).cpu().numpy().copy() for b in batches]
    ds, m = _make_model(pkg, g, tmp_path)
    adj = ds.getSparseGraphCSR()
    ranges = pkg.parallel.row_ranges(adj.indptr, ds.n_users, world)
    own = [pkg.parallel.owned_rows(ranges, r) for r in range(world)]
    assert np.array_equal(np.sort(np.concatenate(own)), np.arange(ds.n_users + ds.m_items))
    nnz_r = np.array([np.diff(adj.indptr)[o].sum() for o in own], np.float64)
    assert nnz_r.max() < 1.6 * nnz_r.mean()
    st = m._state(max_batch=B, need_ctx=True, dp_world=world)          # buffers (shared by the emulated ranks)
    full = st['graph']
    graphs = [L.Graph(full.indptr, full.indices, full.vals, d_max=g.d, row_order=o) for o in own]
    ctxs = []
    for r in range(world):
        cfg = L.TrainConfig()
        cfg.graph = graphs[r].handle
        cfg.n_users, cfg.d, cfg.K, cfg.act_dtype = ds.n_users, g.d, g.K, 0
        cfg.E0, cfg.adam_m, cfg.adam_v = m._table.data_ptr(), st['adam_m'].data_ptr(), st['adam_v'].data_ptr()
        cfg.act, cfg.G64, cfg.bitmap = st['act'].data_ptr(), st['G64'].data_ptr(), st['bitmap'].data_ptr()
        cfg.terms, cfg.contrib = st['terms'].data_ptr(), st['contrib'].data_ptr()
        cfg.err, cfg.max_batch, cfg.decay = st['err'].data_ptr(), B, float(g.meta["decay"])
        cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.xcd_remap = float(g.meta["lr"]), 0.9, 0.999, 1e-8, 1
        cfg.dense_last = int(st['dense_last'])               # same last-layer mode as the reference run
        h = C.c_void_p()
        L.check(lib.lgcn_ctx_create(C.byref(cfg), C.byref(h)), "ctx")
        ctxs.append(h)
    K = g.K
    fwd_layers = K if st['dense_last'] else K - 1
    FWD, BPR, SCATTER, BWD, FINISH = 0, 1, 2, 3, 4
    stream = L.current_stream()
    for i, (u, p, n) in enumerate(batches):
        b = len(u)

        def phase(r, ph, k, gathered=None, loss=None):
            L.check(lib.lgcn_rs_phase(ctxs[r], ph, k, L.tp(u), L.tp(p), L.tp(n), b, world, r,
                                      L.tp(gathered) if gathered is not None else None,
                                      L.tp(loss) if loss is not None else None, stream), f"phase {ph} {k}")
        for k in range(1, fwd_layers + 1):
            for r in range(world):
                phase(r, FWD, k)
        nblk = pkg.parallel.block_numel(b, world, g.d)
        blocks = []
        for r in range(world):
            phase(r, BPR, 0)
            blocks.append(st['contrib'][:nblk].clone())
        gathered = torch.cat(blocks)
        phase(0, SCATTER, 0, gathered)                       # G64 / bitmap are shared: once
        for k in range(K, 0, -1):
            for r in range(world):
                phase(r, BWD, k, gathered)
        loss = torch.empty(3, device=DEV)
        phase(0, FINISH, 0, gathered, loss)
        torch.cuda.synchronize()
        assert np.array_equal(loss.cpu().numpy().view(np.uint32), ref_losses[i].view(np.uint32)), (i, loss, ref_losses[i])
    assert np.array_equal(m._table.cpu().numpy().view(np.uint32), ref._table.cpu().numpy().view(np.uint32))
    for key in ('adam_m', 'adam_v'):
        assert torch.equal(st[key], ref._dev[key])
    assert int(st['G64'].abs().sum()) == 0 and int(st['bitmap'].abs().sum()) == 0
    for h in ctxs:
        lib.lgcn_ctx_destroy(h)
    for gr in graphs:
        gr.close()


def test_gpu_sampler_bit_exact(pkg, oracle, tiny, tmp_path):
    """The device sampler (block-parallel glibc stream by jump-ahead + speculative triplets with
    first-rejection fix-up) against the host restatement of sampling.cpp on the same seed: identical
    int32 rows for two consecutive epochs (the host generator is moved past the draws the device used),
    on a graph DENSE enough that rejections are frequent (deg/m = 25 %), on the tiny fixture (whose rows
    the reference itself produced) and at Gowalla size against the reference's recorded hashes."""
    import hashlib
    S = pkg.sampling
    rng = np.random.Generator(np.random.PCG64(12))
    n_users, m_items = 700, 160
    rows = [np.sort(rng.choice(m_items, size=int(rng.integers(1, 60)), replace=False)).astype(np.int32) for _ in range(n_users)]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows)
    train_num = 13 * n_users + 5
    S.seed(77)
    want = [S.sample_negative(n_users, m_items, train_num, (indptr, indices), 1) for _ in range(2)]
    tail_host = [S.randint(1000) for _ in range(4)]
    S.seed(77)
    got = [S.sample_negative_device(n_users, m_items, train_num, (indptr, indices), DEV).cpu().numpy() for _ in range(2)]
    tail_dev = [S.randint(1000) for _ in range(4)]
    for w_, g_ in zip(want, got):
        assert g_.dtype == np.int32 and np.array_equal(w_, g_)
    assert tail_host == tail_dev                                    # stream position after the device epochs
    # tiny fixture: rows captured from the reference's own compiled plugin
    ds, m = _make_model(pkg, tiny, tmp_path)
    pkg.sampling.seed(pkg.world.seed)
    for e in (1, 2):
        got_e = S.sample_negative_device(ds.n_users, ds.m_items, ds.trainDataSize, ds.pos_csr(), DEV).cpu().numpy()
        assert np.array_equal(got_e, tiny.z[f"S_epoch{e}"])
    # Gowalla: the reference's recorded sha256 prefixes
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import materialize_gowalla
    d = materialize_gowalla(os.path.join(GOLDEN, "gowalla", "gowalla.npz"), os.path.join(str(tmp_path), "gowalla"))
    pkg.world.configure(["--dataset", "gowalla", "--tensorboard", "0"])
    gds = pkg.dataloader.Loader(pkg.world.config, path=d)
    pkg.sampling.seed(2020)
    for prefix in ("978d20809083cea5", "dcfb3021bcc6755a"):
        Sg = S.sample_negative_device(gds.n_users, gds.m_items, gds.trainDataSize, gds.pos_csr(), DEV).cpu().numpy()
        assert Sg.shape == (806166, 3) and hashlib.sha256(Sg.tobytes()).hexdigest().startswith(prefix)


def test_gpu_sampler_segments_heavy_tail_bit_exact(pkg):
    """The segmented device sampler (rejecting (position, user) pairs on all CUs, the event walk in LDS, triplets emitted in
    parallel) where its capacities and shortcuts are under stress: power-law degrees, hub users positive on 25-50 % of the items
    next to each other (blocks full of pairs, segments ending early on the extra-draw budget), two users positive on 99 % of the
    items (rejection runs longer than the budget: the walk leaves the pair list and asks the row; the one-workgroup kernel
    finishes what the segment launches did not reach).  Rows identical to the host restatement of sampling.cpp for three
    consecutive epochs, and the host generator ends at the same stream position."""
    S = pkg.sampling
    rng = np.random.Generator(np.random.PCG64(2024))
    n_users, m_items = 3000, 2000
    deg = np.minimum(m_items // 4, np.maximum(1, (30.0 / rng.random(n_users) ** 0.7).astype(np.int64) // 8))
    deg[100:108] = m_items // 2                 # adjacent hubs
    deg[1500] = deg[1501] = m_items - 20        # 99 % positive
    deg[2999] = m_items // 3                    # the last user
    rows = [np.sort(rng.choice(m_items, size=int(k), replace=False)).astype(np.int32) for k in deg]
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate(rows)
    train_num = 15 * n_users + 7
    S.seed(31)
    want = [S.sample_negative(n_users, m_items, train_num, (indptr, indices), 1) for _ in range(3)]
    tail_host = [S.randint(1 << 20) for _ in range(4)]
    S.seed(31)
    got = [S.sample_negative_device(n_users, m_items, train_num, (indptr, indices), DEV).cpu().numpy() for _ in range(3)]
    tail_dev = [S.randint(1 << 20) for _ in range(4)]
    for e, (w_, g_) in enumerate(zip(want, got)):
        bad = np.flatnonzero((w_ != g_).any(axis=1))
        assert g_.dtype == np.int32 and bad.size == 0, (e, bad[:5], w_[bad[:3]], g_[bad[:3]])
    assert tail_host == tail_dev


def test_device_shuffle_bit_exact(pkg):
    """lgcn_np_shuffle_perm_device: np.random.shuffle(arange(n)) (utils.py:148-149, numpy's legacy MT19937 + masked-rejection
    Fisher-Yates) computed on the GPU -- ONE wave twists MT19937 in LDS and aligns the draws to the steps as it generates them,
    64 draws per pass or a whole block of 624 on the fast path, with no stream buffer in memory; the swaps as sorted chains +
    pointer doubling -- against the host restatement lgcn_np_shuffle_perm (which test_oracle / test_host pin to numpy itself):
    identical permutations for one and two steps, sizes around the serial tail at 1024 and around powers of two, Gowalla's epoch
    and sizes in the millions, every call starting wherever the last one left the generator block, and the generator left exactly
    where the host loop leaves it (host and device calls interleaved draw the same stream).  The sizes here descend through every
    mask boundary at whatever block offset the stream gives them (1279..1281 and 65536 +- 255..257 date from a first form that
    aligned 256 draws at a time and mark nothing in this kernel); the hand-overs between the kernel's paths (the fast guard
    i - 624 >= max(1024, low), the pass guard i - 64 >= low, the serial stretches) are started deliberately, from chosen read
    positions, in tests/test_gpu_shuffle.py, and its swap resolution is fed deep chains there."""
    U = pkg.utils
    sizes = [1, 2, 3, 7, 64, 255, 256, 257, 1000, 1023, 1024, 1025, 1279, 1280, 1281, 1535, 1536, 2047, 2048, 2049, 4095, 4097, 5000,
             65535, 65536, 65537, 65536 + 255, 65536 + 256, 65536 + 257, 70000, 131071, 131072 + 300, 806166, 810128,
             (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 255, (1 << 20) + 256, (1 << 20) + 700]
    for seed in (2020, 7):
        U.set_seed(seed)
        want = [U.shuffle_indices(n) for n in sizes]
        tail_host = U.shuffle_indices(50)
        U.set_seed(seed)
        for n, w_ in zip(sizes, want):
            got = U.shuffle_indices_device(n, DEV).cpu().numpy()
            assert got.dtype == np.int64 and np.array_equal(got, w_), (seed, n, np.flatnonzero(got != w_)[:5])
        assert np.array_equal(U.shuffle_indices(50), tail_host), seed          # same stream position afterwards
    # interleaved: host, device, host, device ... on one stream
    U.set_seed(99)
    want = [U.shuffle_indices(n) for n in (5000, 300, 70001, 9, 2500)]
    U.set_seed(99)
    got = [U.shuffle_indices(5000), U.shuffle_indices_device(300, DEV).cpu().numpy(), U.shuffle_indices(70001),
           U.shuffle_indices_device(9, DEV).cpu().numpy(), U.shuffle_indices_device(2500, DEV).cpu().numpy()]
    for a_, b_ in zip(want, got):
        assert np.array_equal(a_, b_)
    # and it is a permutation numpy itself produces
    rs = np.random.RandomState(5); ref = np.arange(4097); rs.shuffle(ref)
    U.set_seed(5)
    assert np.array_equal(U.shuffle_indices_device(4097, DEV).cpu().numpy(), ref)
    # random sizes, one continuous stream (every call starts wherever the last one left the generator block)
    rng = np.random.Generator(np.random.PCG64(123))
    sizes = [int(x) for x in np.concatenate([rng.integers(2, 5000, 12), rng.integers(5000, 3_000_000, 12)])]
    U.set_seed(31)
    want = [U.shuffle_indices(n) for n in sizes]
    U.set_seed(31)
    for n, w_ in zip(sizes, want):
        assert np.array_equal(U.shuffle_indices_device(n, DEV).cpu().numpy(), w_), n


def test_epoch_triplets_device_shuffle_equals_host_shuffle(pkg, tiny, tmp_path):
    """Procedure.sample_epoch_to_device with --gpu_shuffle 1 (default) and 0: the same shuffled triplets, three epochs in a row."""
    out = []
    for flag in (1, 0):
        ds, m = _make_model(pkg, tiny, tmp_path)
        pkg.world.config['gpu_shuffle'] = flag
        pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
        out.append([tuple(t.cpu().numpy() for t in pkg.Procedure.sample_epoch_to_device(ds, DEV)) for _ in range(3)])
    pkg.world.config['gpu_shuffle'] = 1
    for e in range(3):
        for c in range(3):
            assert np.array_equal(out[0][e][c], out[1][e][c]), (e, c)


def test_gpu_sampler_segments_reach_the_end_of_the_stream(pkg):
    """a MID-density dataset (2.5 % of the items positive per user: the segments complete, none overflows a
    capacity) whose rejections need more draws than the stream margin holds.  The segment kernels skip positions past the
    expanded stream and emit without bound checks, so before the fix the call returned 0 with garbage in the last triplets
    and moved the host generator by a wrong count.  With the margin made small through the test hook, EVERY margin must
    end in one of two ways: rc 5 with the host generator untouched, or rc 0 with the host sampler's rows bit for bit and
    the generator at the host's position -- and both outcomes must occur over the sweep."""
    S = pkg.sampling
    lib = pkg._lib.load()
    rng = np.random.Generator(np.random.PCG64(77))
    n_users, m_items, deg = 4000, 2000, 50
    rows = [np.sort(rng.choice(m_items, size=deg, replace=False)).astype(np.int32) for _ in range(n_users)]
    indptr = (np.arange(n_users + 1, dtype=np.int64) * deg)
    indices = np.concatenate(rows)
    train_num = n_users * deg
    S.seed(5)
    want = S.sample_negative(n_users, m_items, train_num, (indptr, indices), 1)
    tail_host = [S.randint(1 << 20) for _ in range(4)]
    outcomes = []
    try:
        for fixed in (1, 1500, 3000, 4000, 4600, 5000, 5400, 6000, 8000, 12000, 20000):
            lib.lgcn_sampler_test_margin(1 << 40, fixed)
            S._DEVICE_CSR.clear()
            S.seed(5)
            try:
                got = S.sample_negative_device(n_users, m_items, train_num, (indptr, indices), DEV).cpu().numpy()
            except pkg._lib.LgcnError as e:
                assert "(rc=5)" in str(e), str(e)
                # the host generator has not moved: the host sampler now draws the epoch the reference draws
                assert np.array_equal(S.sample_negative(n_users, m_items, train_num, (indptr, indices), 1), want), fixed
                outcomes.append(5)
                continue
            bad = np.flatnonzero((want != got).any(axis=1))
            assert bad.size == 0, (fixed, bad[:5], want[bad[:3]], got[bad[:3]])
            assert [S.randint(1 << 20) for _ in range(4)] == tail_host, fixed
            outcomes.append(0)
    finally:
        lib.lgcn_sampler_test_margin(0, 0)
        S._DEVICE_CSR.clear()
    assert 5 in outcomes and 0 in outcomes, outcomes
    assert outcomes == sorted(outcomes, reverse=True), outcomes        # small margins fail, large ones pass


def test_gpu_sampler_margin_falls_back_to_host(pkg, tmp_path):
    """A dense dataset (every user holds 90 % of the items: ~9 rejected negatives per triplet) exceeds the device sampler's
    stream margin (T/50 + 65536 draws): lgcn_sample_negative_device returns rc 5 WITHOUT advancing the host generator
    and Procedure.sample_epoch_to_device hands that epoch to the bit-exact host sampler -- the epoch's triplets are
    the ones --gpu_sampler 0 produces, and training goes on."""
    n_users, m_items, keep = 2000, 200, 180
    rng = np.random.Generator(np.random.PCG64(4))
    path = os.path.join(str(tmp_path), "dense")
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "train.txt"), "w") as f, open(os.path.join(path, "test.txt"), "w") as ft:
        for u in range(n_users):
            items = np.sort(rng.choice(m_items, size=keep, replace=False))
            f.write(f"{u} " + " ".join(map(str, items.tolist())) + "\n")
            ft.write(f"{u} {int(rng.integers(0, m_items))}\n")
    w = pkg.world
    out = []
    for gpu in (1, 0):
        w.configure(["--dataset", "dense", "--tensorboard", "0", "--gpu_sampler", str(gpu), "--prefetch_epoch", "0"])
        ds = pkg.dataloader.Loader(w.config, path=path)
        pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
        if gpu:
            with pytest.raises(pkg._lib.LgcnError, match="rc=5"):
                pkg.sampling.sample_negative_device(ds.n_users, ds.m_items, ds.trainDataSize, ds.pos_csr(), DEV)
        epochs = [tuple(t.cpu().numpy() for t in pkg.Procedure.sample_epoch_to_device(ds, DEV)) for _ in range(2)]
        out.append(epochs)
    for e in range(2):
        for c in range(3):
            assert np.array_equal(out[0][e][c], out[1][e][c]), (e, c)
    assert len(out[0][0][0]) == n_users * keep
    w.configure([])


@pytest.mark.parametrize("K", [1, 3])
def test_dense_last_layer_option_vs_oracle(pkg, oracle, tiny, tmp_path, K):
    """cfg.dense_last = 1 (last layer propagated densely, batch rows read from it -- what 'auto' picks on
    hub-heavy graphs): three fused steps vs the oracle, and against the default path on the same inputs
    (same result up to fp32 summation order)."""
    g = tiny
    rng = np.random.Generator(np.random.PCG64(20 + K))
    batches = [(rng.integers(0, g.n_users, b), rng.integers(0, g.m_items, b), rng.integers(0, g.m_items, b)) for b in (64, 64, 9)]
    A = (g.z["adj_indptr"], g.z["adj_indices"], g.z["adj_data"])
    tables = {}
    for mode in ("1", "0"):
        ds, m = _make_model(pkg, g, tmp_path, K=K)
        m.config['dense_last'] = mode
        tr = oracle.Trainer(g.n_users, *A, g.e0(), K, g.meta["decay"], g.meta["lr"])
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        for (u, p, n) in batches:
            l_ref = tr.stageOne(u, p, n)
            l_got = bpr.stageOne(_dev(u), _dev(p), _dev(n))
            assert abs(l_got - l_ref) < 3e-6, (mode, l_got, l_ref)
            np.testing.assert_allclose(m._table.cpu().numpy(), tr.e0, rtol=0, atol=3e-6)
        assert m._dev['dense_last'] == (mode == "1")
        assert int(m._dev['G64'].abs().sum()) == 0
        tables[mode] = m._table.cpu().numpy().copy()
    np.testing.assert_allclose(tables["1"], tables["0"], rtol=0, atol=2e-6)

"""Weighted layer combination in the fused step (--layer_weights).

The contract: for fp32 weights w_0..w_K, used exactly as given,  out = sum_k w_k X_k  (X_0 = E0, X_k = A_hat X_{k-1}) in the
training rows and in evaluation, and with G = d loss / d out the backward chain  h_K = w_K G,  h_{k-1} = w_{k-1} G + A_hat h_k,
gradient = h_0.  Every reference here is independent of the kernels: scipy float64 for the propagation, torch autograd on the
CPU (fp32, and float64 as the guard of that reference) for the step.

The graph and the batches are test_gpu_dropout's: user 0 with 600 items (two chunks and the ticket hand-off), user 1 with 100
(two tiles), the others 1..12 (the pack path), ten empty item rows; three steps of 64 / 17 / 1 triplets with duplicated users,
pos = neg collisions and the long rows in every batch -- the smallest shape at which every row form of k_triplet and k_spmm
exists.  All weight sets lie in [0, 1] and sum to at most 1, so rows keep the magnitude of the mean and the project's
tolerances apply unchanged."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_gpu_dropout import DEV, M_ITEMS, N_USERS, _batches, _bits, _dev, _graph, _rows_of, _write_graph

pytestmark = pytest.mark.gpu


def _f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def weight_set(name, K):
    """the named sets at K = 3 and their analogues (the first K + 1 entries where that keeps the set's point)"""
    k = np.arange(K + 1, dtype=np.float64)
    if name == "exp":
        w = 0.5 ** k
        return _f32(w / w.sum())
    if name == "ppr":
        w = 0.15 * 0.85 ** k
        return _f32(w / w.sum())
    if name == "last":
        return _f32([0.0] * K + [1.0])
    if name == "first":
        return _f32([1.0] + [0.0] * K)
    if name == "literal":
        return _f32([0.5, 0.25, 0.15, 0.07, 0.03][:K + 1])
    if name == "midzero":           # an interior zero from K = 2 on (K = 1 has no interior: its zero is the last layer's)
        return _f32({1: [0.6, 0.0], 2: [0.6, 0.0, 0.1], 3: [0.6, 0.0, 0.1, 0.3], 4: [0.6, 0.0, 0.1, 0.0, 0.3]}[K])
    if name == "uniform":
        return _f32([1.0 / (K + 1)] * (K + 1))
    raise KeyError(name)


SETS = ("exp", "ppr", "last", "first", "literal", "midzero")


def _lw(w):
    return None if w is None else "[" + ",".join(repr(float(v)) for v in w) + "]"


def _model(pkg, tmp_path, K=3, d=64, act="fp32", w=None, dense_last="0", reg_rows="propagated", hub=None, extra=None, spec=None):
    path = os.path.join(str(tmp_path), "dropgraph")
    if not os.path.exists(os.path.join(path, "train.txt")):
        _write_graph(path)
    wd = pkg.world
    wd.configure(["--dataset", "dropgraph", "--tensorboard", "0", "--layer", str(K), "--recdim", str(d), "--bpr_batch", "64",
                  "--act_dtype", act] + (["--layer_weights", spec or _lw(w)] if (w is not None or spec) else []))
    wd.config.update({'dense_last': dense_last, 'reg_rows': reg_rows, 'row_order': 'rcm'})
    if hub is not None:
        wd.config.update({'hub_nnz': hub, 'hub_chunk': 256})
    if extra:
        wd.config.update(extra)
    wd.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
    ds = pkg.dataloader.Loader(wd.config, path=path)
    pkg.utils.set_seed(7)
    m = pkg.model.LightGCN(wd.config, ds).to(DEV)
    assert (ds.n_users, ds.m_items) == (N_USERS, M_ITEMS)
    if w is not None:
        assert np.array_equal(m.layer_weights, np.asarray(w, np.float32))        # a literal list arrives bit for bit
    return ds, m


@pytest.fixture(scope="module")
def adj(pkg, tmp_path_factory):
    """A_hat of the test graph (scipy CSR, fp32, sorted) -- built once, never modified."""
    ds, m = _model(pkg, tmp_path_factory.mktemp("adj"))
    a = m._adj.copy()
    deg = np.diff(a.indptr)
    assert deg[0] == 600 and deg[1] == 100 and deg[2:N_USERS].max() <= 12 and (deg[N_USERS:] == 0).sum() >= 10
    return a


def _a64(a):
    import scipy.sparse as sp
    return sp.csr_matrix((a.data.astype(np.float64), a.indices, a.indptr), shape=a.shape)


def _weighted_table64(a, e0, w):
    A, x = _a64(a), np.asarray(e0, np.float64)
    out = float(w[0]) * x
    for k in range(1, len(w)):
        x = A @ x
        out = out + float(w[k]) * x
    return out


def _bf16(x):
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).double().numpy()


def _propagate(pkg, g, e0, K, d, act, w):
    L = pkg._lib
    N = e0.shape[0]
    work = torch.zeros(max(K - 1, 1), N, d, device=DEV, dtype=torch.float32 if act == L.F32 else torch.bfloat16)
    out = torch.full((N, d), 7.0, device=DEV)
    wp = None if w is None else np.ascontiguousarray(w, np.float32)
    if w is None:
        rc = L.load().lgcn_propagate_mean(g.handle, L.tp(e0), K, d, act, L.tp(work), L.tp(out), L.current_stream())
    else:
        rc = L.load().lgcn_propagate_weighted(g.handle, L.tp(e0), K, d, act, L.tp(work), wp.ctypes.data_as(C.c_void_p), L.tp(out),
                                              L.current_stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_propagate_weighted_vs_scipy(pkg, adj, d):
    """lgcn_propagate_weighted on the test graph's A_hat, K in {1, 3}, every weight set, against scipy float64.  fp32 storage at
    test_spmm_vs_oracle_random's fp32 bound (rtol 2e-5, atol 1e-6).  bf16 storage at that test's bound for bf16 tables (1e-2 /
    1e-4), against the float64 reference of what bf16 storage stores, as there: layer 1 reads bf16(E0) and the layers below the
    last are kept in bf16 (K >= 2); X_0 in the sum stays fp32."""
    L = pkg._lib
    rng = np.random.Generator(np.random.PCG64(100 + d))
    X = rng.normal(0, 0.1, (adj.shape[0], d)).astype(np.float32)
    e0 = _dev(X)
    g = _graph(pkg, adj, d_max=d)
    A = _a64(adj)
    for K in (1, 3):
        for name in SETS + ("uniform",):
            w = weight_set(name, K)
            rc, got = _propagate(pkg, g, e0, K, d, L.F32, w)
            assert rc == 0, (K, name, L.load().lgcn_last_error())
            np.testing.assert_allclose(got.cpu().numpy(), _weighted_table64(adj, X, w), rtol=2e-5, atol=1e-6, err_msg=f"fp32 K={K} {name}")
            if name == "uniform":      # explicit uniform weights = the mean
                rc, mean = _propagate(pkg, g, e0, K, d, L.F32, None)
                assert rc == 0
                np.testing.assert_allclose(got.cpu().numpy(), mean.cpu().numpy(), rtol=2e-5, atol=1e-6, err_msg=f"uniform vs mean K={K}")
            # bf16 storage
            rc, gotb = _propagate(pkg, g, e0, K, d, L.BF16, w)
            assert rc == 0, (K, name, L.load().lgcn_last_error())
            x = _bf16(X) if K >= 2 else X.astype(np.float64)
            ref = float(w[0]) * X.astype(np.float64)
            for k in range(1, K + 1):
                x = A @ x
                if k < K:
                    x = _bf16(x)
                ref = ref + float(w[k]) * x
            np.testing.assert_allclose(gotb.cpu().numpy(), ref, rtol=1e-2, atol=1e-4, err_msg=f"bf16 K={K} {name}")
    # the argument checks
    lib = L.load()
    work = torch.zeros(2, adj.shape[0], d, device=DEV)
    out = torch.zeros(adj.shape[0], d, device=DEV)
    ok = weight_set("exp", 3)
    # (the entry point takes K + 1 values from a bare pointer: a wrong COUNT is checked where a count is passed, by
    #  lgcn_ctx_set_layer_weights in test_refusals_on_the_device)
    for what, w in (("nan", np.array([0.5, np.nan, 0.1, 0.1], np.float32)), ("inf", np.array([0.5, np.inf, 0.1, 0.1], np.float32)),
                    ("zeros", np.zeros(4, np.float32))):
        rc = lib.lgcn_propagate_weighted(g.handle, L.tp(e0), 3, d, L.F32, L.tp(work), w.ctypes.data_as(C.c_void_p), L.tp(out), L.current_stream())
        assert rc == 3 and b"layer weights" in lib.lgcn_last_error(), what
    assert lib.lgcn_propagate_weighted(g.handle, L.tp(e0), 3, d, L.F32, L.tp(work), None, L.tp(out), L.current_stream()) == 3
    assert b"layer weights" in lib.lgcn_last_error()
    assert lib.lgcn_propagate_weighted(g.handle, L.tp(e0), 3, d, L.FP8, L.tp(work), ok.ctypes.data_as(C.c_void_p), L.tp(out), L.current_stream()) == 3
    assert b"layer weights" in lib.lgcn_last_error()
    torch.cuda.synchronize()
    g.close()


class _WeightedRef:
    """The model's bpr_loss algebra with torch autograd on the CPU (test_gpu_dropout's _TorchRef with acc = sum_k w_k x_k):
    sparse A_hat, K propagations, the weighted combination, BPR + L2 term (either choice of rows), torch.optim.Adam.  dtype
    float32 is the reference; float64 with the same fp32 inputs is its guard."""

    def __init__(self, a, e0, w, decay, lr, reg_rows, dtype=torch.float32):
        self.K, self.decay, self.reg_rows = len(w) - 1, decay, reg_rows
        self.w = [float(v) for v in np.asarray(w, np.float32)]
        self.E = torch.tensor(np.asarray(e0, np.float32), dtype=dtype, requires_grad=True)
        self.opt = torch.optim.Adam([self.E], lr=lr)
        idx = torch.stack([torch.from_numpy(_rows_of(a).astype(np.int64)), torch.from_numpy(a.indices.astype(np.int64))])
        self.A = torch.sparse_coo_tensor(idx, torch.from_numpy(a.data.astype(np.float32)).to(dtype), a.shape).coalesce()

    def step(self, u, p, n):
        x = self.E
        out = self.w[0] * x
        for k in range(1, self.K + 1):
            x = torch.sparse.mm(self.A, x)
            out = out + self.w[k] * x
        u, p, n = (torch.from_numpy(np.asarray(t, np.int64)) for t in (u, p, n))
        ue, pe, ne = out[u], out[N_USERS + p], out[N_USERS + n]
        bpr = -torch.mean(torch.nn.functional.logsigmoid((ue * pe).sum(1) - (ue * ne).sum(1)))
        if self.reg_rows == "ego":
            ue, pe, ne = self.E[u], self.E[N_USERS + p], self.E[N_USERS + n]
        reg = 0.5 * (ue.pow(2).sum() + pe.pow(2).sum() + ne.pow(2).sum()) / float(len(u))
        loss = bpr + self.decay * reg
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return float(loss.detach())

    def table(self):
        return self.E.detach().double().numpy()


_REFS = {}


def reference_run(a, e0, w, decay, lr, reg_rows, batch_seed):
    """Three reference steps in fp32 and in float64 -> (fp32 losses, fp32 tables after each step, guard = max |fp32 - float64|
    over the tables).  Computed once per (weights, reg_rows, batches) and shared by the cases that differ only in how the
    kernels are launched (dense_last, hub plan)."""
    key = (tuple(np.asarray(w, np.float32).tolist()), reg_rows, batch_seed)
    if key not in _REFS:
        r32, r64 = _WeightedRef(a, e0, w, decay, lr, reg_rows), _WeightedRef(a, e0, w, decay, lr, reg_rows, torch.float64)
        losses, tables, guard = [], [], 0.0
        for (u, p, n) in _batches(batch_seed):
            losses.append(r32.step(u, p, n))
            r64.step(u, p, n)
            tables.append(r32.table().copy())
            guard = max(guard, float(np.abs(r32.table() - r64.table()).max()))
        _REFS[key] = (losses, tables, guard)
    return _REFS[key]


# (K, weight set, dense_last, reg_rows, hub, seed of the batches).  The batches' seed is K (test_gpu_dropout's) unless the guard
# of that reference -- fp32 against float64 to 1e-6 on the tables -- fails there: Adam normalises near-zero gradients, so a
# reference can disagree with itself, and such a case gets another seed (it is not loosened or skipped).
def _cases():
    out = []
    for dl in ("0", "1"):
        for name in SETS:
            out.append((3, name, dl, "propagated", None))
        for name in ("exp", "midzero"):
            out.append((3, name, dl, "ego", None))
        for K in (1, 2, 4):
            for name in ("exp", "last", "midzero", "first"):
                out.append((K, name, dl, "propagated", None))
            out.append((K, "exp", dl, "ego", None))
    for name in ("exp", "last", "midzero"):
        out.append((3, name, "0", "propagated", 64))
    out += [(1, "exp", "0", "ego", 64), (2, "midzero", "0", "propagated", 64), (4, "last", "0", "propagated", 64)]
    return out


# cases whose reference fails its guard with the batches of seed K (measured on the CPU, fp32 vs float64 tables: 2.6e-6, 3.1e-6,
# 2.4e-6, 9.7e-6 in this order; every other case is at or below 5.5e-7): seed 11, where they measure 1.9e-7 / 2.8e-8 / 1.9e-7 / 1.9e-7
BATCH_SEED = {(3, "first", "propagated"): 11, (1, "midzero", "propagated"): 11, (1, "first", "propagated"): 11,
              (2, "first", "propagated"): 11}


def _seed_of(K, name, reg_rows):
    return BATCH_SEED.get((K, name, reg_rows), K)


def _run_vs_ref(pkg, tmp_path, adj, K, w, dense_last, reg_rows, hub, batch_seed, tag, set_weights=True):
    ds, m = _model(pkg, tmp_path, K=K, w=w if set_weights else None, dense_last=dense_last, reg_rows=reg_rows, hub=hub)
    st = m._state(max_batch=64, need_ctx=True)
    lib = pkg._lib.load()
    if hub is not None and dense_last == "0":
        assert lib.lgcn_ctx_hub_rows(st['ctx']) == 2                  # users 0 and 1 go through the hub plan
    got_w = np.zeros(pkg._lib.MAX_LAYERS + 1, np.float32)
    n_set = lib.lgcn_ctx_get_layer_weights(st['ctx'], got_w.ctypes.data_as(C.c_void_p))
    assert n_set == (K + 1 if set_weights else 0) and (not set_weights or np.array_equal(got_w[:K + 1], w))
    wd = pkg.world
    losses, tables, guard = reference_run(adj, m._table.cpu().numpy().copy(), w, wd.config['decay'], wd.config['lr'], reg_rows, batch_seed)
    print(f"{tag} K={K} w={w.tolist()} reg={reg_rows} seed={batch_seed}: guard (fp32 vs float64 reference) {guard:.2e}")
    assert guard <= 1e-6, ("the reference disagrees with itself: pick another batch seed for this case", tag, guard)
    bpr = pkg.utils.BPRLoss(m, wd.config)
    for step, (u, p, n) in enumerate(_batches(batch_seed)):
        assert m.adam_step == step
        l_got = bpr.stageOne(_dev(u), _dev(p), _dev(n))
        err = float(np.abs(m._table.cpu().numpy() - tables[step]).max())
        print(f"{tag} K={K} dense_last={dense_last} reg={reg_rows} hub={hub} step {step}: loss {l_got:.7f} ref {losses[step]:.7f} max|dP| {err:.2e}")
        assert abs(l_got - losses[step]) < 3e-6, (tag, step, l_got, losses[step])
        np.testing.assert_allclose(m._table.cpu().numpy(), tables[step], rtol=0, atol=3e-6)
    assert int(m._dev['G64'].abs().sum()) == 0
    m.check_device_errors()
    return m


@pytest.mark.parametrize("K,name,dense_last,reg_rows,hub", _cases())
def test_fused_step_with_weights_vs_torch_autograd(pkg, adj, tmp_path, K, name, dense_last, reg_rows, hub):
    """Three fused steps with layer weights (fp32 storage) against torch autograd on the CPU: loss and tables at the project's
    yardstick for this comparison (3e-6, test_fused_step_vs_oracle).  A scale left in G32, the two coefficients of the first
    backward layer swapped, a row form of k_triplet that still takes the mean: each misses it."""
    _run_vs_ref(pkg, tmp_path, adj, K, weight_set(name, K), dense_last, reg_rows, hub, _seed_of(K, name, reg_rows), name)


@pytest.mark.parametrize("K,dense_last,reg_rows,hub", [
    (1, "0", "propagated", None), (2, "1", "propagated", None), (3, "0", "propagated", None), (3, "1", "ego", None),
    (4, "0", "ego", None), (3, "0", "propagated", 64)])
def test_uniform_reference_vs_weights_off_step(pkg, adj, tmp_path, K, dense_last, reg_rows, hub):
    """The same reference with uniform weights against the step that never heard of weights (no setter call), so that a flaw of
    the reference shows apart from one of the feature -- and against the step with uniform weights set."""
    w = weight_set("uniform", K)
    seed = _seed_of(K, "uniform", reg_rows)
    _run_vs_ref(pkg, tmp_path, adj, K, w, dense_last, reg_rows, hub, seed, "off", set_weights=False)
    _run_vs_ref(pkg, tmp_path, adj, K, w, dense_last, reg_rows, hub, seed, "uniform")


@pytest.mark.parametrize("dense_last", ["0", "1"])
def test_first_layer_only_is_matrix_factorisation(pkg, tmp_path, dense_last):
    """Known answer: w = [1, 0, 0, 0] with the L2 term on the propagated rows is matrix factorisation -- after one step every
    table row that is not a slot of the batch, and its Adam state, is bit-identical to its initial value.  Any A_hat term that
    leaks into the chain moves the neighbours of the batch rows."""
    ds, m = _model(pkg, tmp_path, K=3, w=weight_set("first", 3), dense_last=dense_last)
    before = _bits(m)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    u, p, n = _batches(3)[0]
    bpr.stageOne(_dev(u), _dev(p), _dev(n))
    after = _bits(m)
    slots = np.unique(np.concatenate([u, N_USERS + p, N_USERS + n]))
    others = np.setdiff1d(np.arange(N_USERS + M_ITEMS), slots)
    assert len(slots) > 100 and len(others) > 700
    assert np.array_equal(after[others], before[others])
    for key in ('adam_m', 'adam_v'):
        st = m._dev[key].cpu().numpy().view(np.uint32)
        assert not st[others].any(), key                                          # Adam state: still +0.0, bit for bit
        assert st[slots].any(axis=1).all(), key
    assert (after[slots] != before[slots]).any(axis=1).all()                      # ... and every slot row moved
    m.check_device_errors()


def _steps(pkg, m, seed=3):
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    losses = [bpr.stageOne(_dev(u), _dev(p), _dev(n)) for (u, p, n) in _batches(seed)]
    m.check_device_errors()
    return bpr, losses


def test_bf16_storage(pkg, tmp_path):
    """bf16 activation storage, K = 3, exp: against the fp32-storage run on the same batches, at the bounds
    test_fused_steps_other_dims_vs_oracle uses for bf16 (loss 3e-3, tables 2e-3) -- and the two are not equal."""
    out = {}
    for act in ("fp32", "bf16"):
        ds, m = _model(pkg, tmp_path, K=3, act=act, w=weight_set("exp", 3))
        _, losses = _steps(pkg, m)
        out[act] = (losses, m._table.cpu().numpy().copy())
    for a, b in zip(out["fp32"][0], out["bf16"][0]):
        assert abs(a - b) < 3e-3, out
    np.testing.assert_allclose(out["bf16"][1], out["fp32"][1], rtol=0, atol=2e-3)
    assert not np.array_equal(out["bf16"][1], out["fp32"][1])


def test_off_means_off(pkg, tmp_path):
    """Weights set and cleared again (NULL) = the run that never set them, bit for bit; --layer_weights mean makes no setter
    call; exp moves the tables by more than 1e-4 from the mean run in three steps (a CPU trial of the reference saw 5e-3)."""
    L = pkg._lib
    lib = L.load()
    ds, m0 = _model(pkg, tmp_path, K=3)
    assert m0.layer_weights is None
    st = m0._state(max_batch=64, need_ctx=True)
    assert lib.lgcn_ctx_get_layer_weights(st['ctx'], None) == 0
    _, l0 = _steps(pkg, m0)
    ds, mm = _model(pkg, tmp_path, K=3, spec="mean")
    assert mm.layer_weights is None
    st = mm._state(max_batch=64, need_ctx=True)
    assert lib.lgcn_ctx_get_layer_weights(st['ctx'], None) == 0
    _, lm = _steps(pkg, mm)
    ds, m1 = _model(pkg, tmp_path, K=3)
    st = m1._state(max_batch=64, need_ctx=True)
    w = weight_set("exp", 3)
    assert lib.lgcn_ctx_set_layer_weights(st['ctx'], w.ctypes.data_as(C.c_void_p), 4) == 0
    assert lib.lgcn_ctx_get_layer_weights(st['ctx'], None) == 4
    assert lib.lgcn_ctx_set_layer_weights(st['ctx'], None, 0) == 0
    assert lib.lgcn_ctx_get_layer_weights(st['ctx'], None) == 0
    _, l1 = _steps(pkg, m1)
    assert l0 == l1 == lm and np.array_equal(_bits(m0), _bits(m1)) and np.array_equal(_bits(m0), _bits(mm))
    ds, me = _model(pkg, tmp_path, K=3, spec="exp")
    assert np.array_equal(me.layer_weights, w)
    _, le = _steps(pkg, me)
    diff = float(np.abs(me._table.cpu().numpy() - m0._table.cpu().numpy()).max())
    print(f"exp vs mean after three steps: max |dP| {diff:.2e}")
    assert le != l0 and diff > 1e-4


def test_epoch_call_and_resume(pkg, tmp_path):
    """model.fused_epoch / lgcn_train_epoch = the loop of stageOne calls, bit for bit (the epoch call cuts equal batches and a
    short last one: three of 64 and one of 17 here); a model rebuilt from a checkpoint with the same flags continues bit for
    bit."""
    w = weight_set("exp", 3)
    rng = np.random.Generator(np.random.PCG64(77))
    batches = [tuple(_dev(rng.integers(0, hi, 64), torch.int32) for hi in (N_USERS, M_ITEMS, M_ITEMS)) for _ in range(3)]
    batches.append(tuple(t[:17].clone() for t in batches[0]))                     # a short last batch
    ds, ma = _model(pkg, tmp_path, K=3, w=w)
    bpra = pkg.utils.BPRLoss(ma, pkg.world.config)
    la = [bpra.stageOne(*b) for b in batches]
    ds, mf = _model(pkg, tmp_path, K=3, w=w)
    u, p, n = (torch.cat([b[i] for b in batches]) for i in range(3))
    lf = mf.fused_epoch(u, p, n, 64)
    assert [float(x) for x in lf[:, 0].cpu()] == la and np.array_equal(_bits(mf), _bits(ma))
    # 2 steps, save, load into a fresh model with the same flags, 2 more steps
    ds, md = _model(pkg, tmp_path, K=3, w=w)
    bprd = pkg.utils.BPRLoss(md, pkg.world.config)
    ld = [bprd.stageOne(*b) for b in batches[:2]]
    ckpt = os.path.join(str(tmp_path), "last.pth.tar")
    torch.save({'model_state': md.state_dict(), 'optimizer_state': bprd.opt.state_dict()}, ckpt)
    sd = torch.load(ckpt, weights_only=True)
    ds, me = _model(pkg, tmp_path, K=3, w=w)
    bpre = pkg.utils.BPRLoss(me, pkg.world.config)
    me.load_state_dict(sd['model_state'])
    bpre.opt.load_state_dict(sd['optimizer_state'])
    assert me.adam_step == 2
    le = [bpre.stageOne(*b) for b in batches[2:]]
    assert ld + le == la and np.array_equal(_bits(me), _bits(ma))
    for m in (ma, mf, md, me):
        m.check_device_errors()


def test_evaluation_scores_with_the_weighted_table(pkg, adj, tmp_path):
    """After two steps, propagated_table() / computer() / getUsersRating use the weighted table of the current parameters
    (float64 reference; test_evaluation_never_drops's tolerance for the ratings), and Procedure.Test returns the same recall /
    ndcg through the fused kernels (--eval_fused 1) and through the torch harness (--eval_fused 0)."""
    w = weight_set("exp", 3)
    ds, m = _model(pkg, tmp_path, K=3, w=w)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    for (u, p, n) in _batches(3)[:2]:
        bpr.stageOne(_dev(u), _dev(p), _dev(n))
    m.eval()
    ref = _weighted_table64(adj, m._table.cpu().numpy(), w)
    with torch.no_grad():
        got = m.propagated_table()
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=2e-5, atol=1e-6)
        au, ai = m.computer()
        assert torch.equal(torch.cat([au, ai]), got)
        r = m.getUsersRating(torch.arange(8, device=DEV))
    want = ref[:8] @ ref[N_USERS:].T                                              # the float64 weighted table's product
    err = np.abs(r.cpu().numpy().astype(np.float64) - want)
    print(f"getUsersRating vs float64 product: max |err| {err.max():.2e}, max |err| - 1e-6 |want| {(err - 1e-6 * np.abs(want)).max():.2e}")
    np.testing.assert_allclose(r.cpu().numpy(), want, rtol=1e-6, atol=1e-7)
    mean = _weighted_table64(adj, m._table.cpu().numpy(), weight_set("uniform", 3))
    assert np.abs(got.cpu().numpy() - mean).max() > 1e-2                          # not the mean
    wd = pkg.world
    old_topks = list(wd.topks)
    res = {}
    try:
        wd.topks = [20]
        for fused in (1, 0):
            wd.config['eval_fused'] = fused
            res[fused] = pkg.Procedure.Test(ds, m, 0)
    finally:
        wd.topks = old_topks
        wd.config['eval_fused'] = 1
    for k in ("recall", "ndcg"):
        assert abs(float(res[1][k][0]) - float(res[0][k][0])) < 1e-6, (k, res)
    m.check_device_errors()


def test_autograd_path_trains_the_same_model(pkg, tmp_path):
    """bpr_loss + torch.optim.Adam through computer() (lgcn_propagate_weighted forward, the weighted chain through
    lgcn_spmm_csr backward) for three steps against the fused step: 3e-6, K = 3, exp."""
    w = weight_set("exp", 3)
    ds, mf = _model(pkg, tmp_path, K=3, w=w)
    _, lf = _steps(pkg, mf)
    ds, ma = _model(pkg, tmp_path, K=3, w=w)
    ma.train()
    wd = pkg.world
    opt = torch.optim.Adam(ma.parameters(), lr=wd.config['lr'])
    la = []
    for (u, p, n) in _batches(3):
        loss, reg = ma.bpr_loss(_dev(u), _dev(p), _dev(n))
        loss = loss + wd.config['decay'] * reg
        opt.zero_grad()
        loss.backward()
        opt.step()
        ma.invalidate_cache()
        la.append(float(loss.detach()))
    for a, b in zip(la, lf):
        assert abs(a - b) < 3e-6, (la, lf)
    np.testing.assert_allclose(ma._table.cpu().numpy(), mf._table.cpu().numpy(), rtol=0, atol=3e-6)


def test_refusals_on_the_device(pkg, tmp_path):
    """No silent mean: contexts that have no weighted form refuse the setter, weights and dropout refuse each other, and with
    weights set an entry point that splits a step over ranks returns 3.  Each message names the layer weights; nothing runs."""
    L = pkg._lib
    lib = L.load()
    w = weight_set("exp", 3)
    wp = w.ctypes.data_as(C.c_void_p)
    import scipy.sparse as sp
    i2i_file = os.path.join(str(tmp_path), "i2i.npz")
    sp.save_npz(i2i_file, sp.random(M_ITEMS, M_ITEMS, density=0.01, format="csr", dtype=np.float32, random_state=3))
    i2i = {'use_item_item': True, 'i2i_alpha': 0.1, 'i2i_path': i2i_file}
    for tag, kw in (("fp8", dict(act="fp8")), ("gate", dict(dense_last="1", extra={'use_pop_gate': True})),
                    ("i2i", dict(dense_last="1", extra=i2i))):
        ds, m = _model(pkg, tmp_path, **kw)
        st = m._state(max_batch=64, need_ctx=True)
        before = _bits(m)
        assert lib.lgcn_ctx_set_layer_weights(st['ctx'], wp, 4) == 3 and b"layer weights" in lib.lgcn_last_error(), tag
        assert lib.lgcn_ctx_get_layer_weights(st['ctx'], None) == 0 and np.array_equal(_bits(m), before)
    # dropout on: the setter refuses
    ds, m = _model(pkg, tmp_path, extra={'dropout': 1, 'keep_prob': 0.6})
    st = m._state(max_batch=64, need_ctx=True)
    assert lib.lgcn_ctx_set_layer_weights(st['ctx'], wp, 4) == 3 and b"layer weights" in lib.lgcn_last_error()
    # weights set: bad arguments, dropout and the data-parallel entry points refuse
    ds, m = _model(pkg, tmp_path, w=w)
    st = m._state(max_batch=64, need_ctx=True)
    ctx = st['ctx']
    before = _bits(m)
    for bad, n in ((w, 3), (w, 5), (np.array([0.5, np.nan, 0.1, 0.1], np.float32), 4), (np.zeros(4, np.float32), 4)):
        assert lib.lgcn_ctx_set_layer_weights(ctx, bad.ctypes.data_as(C.c_void_p), n) == 3 and b"layer weights" in lib.lgcn_last_error()
    assert lib.lgcn_ctx_get_layer_weights(ctx, None) == 4                         # a refused call changes nothing
    assert lib.lgcn_ctx_set_dropout(ctx, C.c_float(0.6), 1) == 3 and b"layer weights" in lib.lgcn_last_error()
    u, p, n = (torch.zeros(64, dtype=torch.int32, device=DEV) for _ in range(3))
    assert lib.lgcn_train_step_dp_part1(ctx, L.tp(u), L.tp(p), L.tp(n), 64, 2, 0, L.current_stream()) == 3
    msg = lib.lgcn_last_error()
    assert b"layer weights" in msg and b"lgcn_train_step_dp_part1" in msg
    torch.cuda.synchronize()
    assert m.adam_step == 0 and np.array_equal(_bits(m), before)                  # nothing ran
    m.check_device_errors()

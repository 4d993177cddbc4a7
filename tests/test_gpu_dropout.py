"""Edge dropout in the fused training step (--dropout 1 --keepprob p; DESIGN 4 "Edge dropout").

The contract: for one optimiser step t and a 64-bit seed, keep(i, j) = H(seed, t, i, j) < floor(p * 2^32) with H a hash of the
adjacency's row and column ids only; A_drop[i, j] = keep(i, j) ? A[i, j] / p : 0; ONE mask per step, used by all K forward
layers, the batch rows and -- transposed -- the whole backward.  The mask is exported (lgcn_dropout_mask), so every test here
compares against references built from the exported mask (scipy float64 / torch autograd on the CPU), never against the
kernels' own output.

The graph is written by the tests so that every row form of the kernels exists at the smallest size: user 0 has 600 items
(> LONG_CH = 512: two chunks and the ticket hand-off), user 1 has 100 (two 64-entry tiles, one wave), the other users 1..12
(the pack path), and ten items have no interaction (empty rows).  `tiny` has no long rows."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from dropout_restatement import _fmix32, _keep_host, _rows_of, _splitmix64, a_scaled  # noqa: F401  (the hash, restated on the host from DESIGN 4: the mask is "exported and checkable")

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_USERS, M_ITEMS = 300, 700
SEED = 2020            # world's default --seed: what model.LightGCN hands to lgcn_ctx_set_dropout


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def _write_graph(path):
    rng = np.random.Generator(np.random.PCG64(12345))
    os.makedirs(path, exist_ok=True)
    used = M_ITEMS - 10                              # items 690..699 never interact: empty rows of A_hat
    with open(os.path.join(path, "train.txt"), "w") as f, open(os.path.join(path, "test.txt"), "w") as ft:
        for u in range(N_USERS):
            k = 600 if u == 0 else 100 if u == 1 else int(rng.integers(1, 13))
            items = np.sort(rng.choice(used, size=k, replace=False))
            f.write(f"{u} " + " ".join(map(str, items.tolist())) + "\n")
            ft.write(f"{u} {M_ITEMS - 1 - (u % 10)}\n")          # the test split names the empty items: m_items = 700


def _model(pkg, tmp_path, tag, K=3, d=64, act="fp32", dropout=1, keep=0.6, dense_last="0", reg_rows="propagated", hub=None,
           seed=SEED, extra=None):
    path = os.path.join(str(tmp_path), "dropgraph")
    if not os.path.exists(os.path.join(path, "train.txt")):
        _write_graph(path)
    w = pkg.world
    w.configure(["--dataset", "dropgraph", "--tensorboard", "0", "--layer", str(K), "--recdim", str(d), "--bpr_batch", "64",
                 "--act_dtype", act, "--dropout", str(dropout), "--keepprob", str(keep), "--seed", str(seed)])
    w.config.update({'dense_last': dense_last, 'reg_rows': reg_rows, 'row_order': 'rcm'})
    if hub is not None:
        w.config.update({'hub_nnz': hub, 'hub_chunk': 256})
    if extra:
        w.config.update(extra)
    w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=path)
    pkg.utils.set_seed(7)                            # the tables' initial values (NOT the dropout seed, which is --seed)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    assert (ds.n_users, ds.m_items) == (N_USERS, M_ITEMS)
    return ds, m


@pytest.fixture(scope="module")
def adj(pkg, tmp_path_factory):
    """A_hat of the test graph (scipy CSR, fp32, sorted) -- built once, never modified."""
    ds, m = _model(pkg, tmp_path_factory.mktemp("adj"), "adj", dropout=0)
    a = m._adj.copy()
    deg = np.diff(a.indptr)
    assert deg[0] == 600 and deg[1] == 100 and deg[2:N_USERS].max() <= 12 and (deg[N_USERS:] == 0).sum() >= 10
    return a


def _graph(pkg, a, d_max=256):
    return pkg._lib.Graph(_dev(a.indptr.astype(np.int32)), _dev(a.indices.astype(np.int32)), _dev(a.data.astype(np.float32)), d_max=d_max)


def _mask(pkg, a, keep, seed, step):
    """lgcn_dropout_mask on a scipy CSR (the raw entry point: no graph plan, any entry order inside a row)"""
    L = pkg._lib
    ip, ix = _dev(a.indptr.astype(np.int32)), _dev(a.indices.astype(np.int32))
    out = torch.full((a.nnz,), 7, dtype=torch.uint8, device=DEV)
    L.check(L.load().lgcn_dropout_mask(L.tp(ip), L.tp(ix), a.shape[0], a.nnz, keep, seed, step, L.tp(out), L.current_stream()), "mask")
    mk = out.cpu().numpy()
    assert np.isin(mk, (0, 1)).all()                 # every position written
    return mk.astype(bool)


def test_mask_statistics_and_structure(pkg, adj):
    """lgcn_dropout_mask on the test graph's A_hat (n = nnz entries, n / 2 symmetric pairs), p in {0.6, 0.9}, seeds 2020 and 1.
    Every bound is 5 sigma of the binomial it names and deterministic for a fixed hash."""
    import scipy.sparse as sp
    a = adj
    n = a.nnz
    rows = _rows_of(a)
    masks = {}
    for p in (0.6, 0.9):
        mk = masks[p] = _mask(pkg, a, p, SEED, 0)
        frac = mk.mean()
        print(f"p={p}: n={n} kept {frac:.4f} (bound {5 * np.sqrt(p * (1 - p) / n):.4f})")
        assert abs(frac - p) <= 5 * np.sqrt(p * (1 - p) / n)
        # keep(i, j) and keep(j, i) are independent draws: they differ on 2p(1-p) of the pairs
        M = sp.csr_matrix((mk.astype(np.float64) + 1.0, a.indices, a.indptr), shape=a.shape)          # 1 = dropped, 2 = kept
        Mt = M.T.tocsr(); Mt.sort_indices()
        assert np.array_equal(Mt.indices, a.indices) and np.array_equal(Mt.indptr, a.indptr)           # A_hat's structure is symmetric
        upper = rows < a.indices
        q = 2 * p * (1 - p)
        asym = (M.data[upper] != Mt.data[upper]).mean()
        sig = np.sqrt(q * (1 - q) / (n / 2))
        print(f"p={p}: asymmetric pairs {asym:.4f} (expected {q:.4f}, 5 sigma {5 * sig:.4f})")
        assert upper.sum() == n // 2 and abs(asym - q) <= 5 * sig
        # a fresh mask every step, another mask for another seed
        sig_n = np.sqrt(q * (1 - q) / n)
        for what, other in (("step t+1", _mask(pkg, a, p, SEED, 1)), ("seed 1", _mask(pkg, a, p, 1, 0))):
            ch = (mk != other).mean()
            print(f"p={p}: changed against {what}: {ch:.4f} (expected {q:.4f}, 5 sigma {5 * sig_n:.4f})")
            assert abs(ch - q) <= 5 * sig_n
        # the exported mask IS the documented hash of (seed, step, row id, column id)
        assert np.array_equal(mk, _keep_host(rows, a.indices, p, SEED, 0))
    assert not (masks[0.6] & ~masks[0.9]).any()                       # kept at 0.6  =>  kept at 0.9
    assert _mask(pkg, a, 1.0, SEED, 0).all()                          # keep_prob = 1 keeps everything
    # ids, not positions.  (1) the entries of every row in another order: the mask moves with the entries.
    rng = np.random.Generator(np.random.PCG64(5))
    perm = np.concatenate([s + rng.permutation(e - s) for s, e in zip(a.indptr[:-1], a.indptr[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
    b = sp.csr_matrix((a.data[perm], a.indices[perm], a.indptr), shape=a.shape)
    assert np.array_equal(_mask(pkg, b, 0.6, SEED, 0), masks[0.6][perm])
    # (2) the rows themselves permuted (row r of the copy holds the columns of row rp[r]): every CSR position moves and the
    # row ids of the entries change with it -- the mask is the hash of the NEW (row, column) ids, whatever the position
    rp = rng.permutation(a.shape[0])
    c = a[rp].tocsr()
    got = _mask(pkg, c, 0.6, SEED, 0)
    assert np.array_equal(got, _keep_host(_rows_of(c), c.indices, 0.6, SEED, 0))
    # ... and where a row keeps its id (fixed points of rp are rare; force some) its mask is the original row's
    rp2 = np.arange(a.shape[0]); rp2[2:N_USERS] = 2 + rng.permutation(N_USERS - 2)                     # rows 0, 1 and the items stay
    c2 = a[rp2].tocsr()
    got2 = _mask(pkg, c2, 0.6, SEED, 0)
    stay = np.isin(_rows_of(c2), np.flatnonzero(rp2 == np.arange(a.shape[0])))
    assert stay.sum() > 700 and np.array_equal(got2[stay], masks[0.6][np.isin(rows, np.flatnonzero(rp2 == np.arange(a.shape[0])))])


@pytest.mark.parametrize("d", [32, 64, 128, 256])
def test_masked_spmm_vs_scipy(pkg, adj, d):
    """lgcn_spmm_csr_drop, plain and transposed, fp32 and bf16 input, against scipy float64 (mask o A / keep) @ X with the mask
    read back from lgcn_dropout_mask.  mask != mask^T on ~48 % of the pairs, so a wrong transposition cannot pass.  Tolerances:
    test_spmm_vs_oracle_random's (rtol 2e-5, atol 1e-6 -- the fp32 atol scaled by 1 / keep, as the weights are; bf16 output 1e-2 / 1e-4, unscaled)."""
    import scipy.sparse as sp
    a = adj
    keep, step = 0.6, 3
    rng = np.random.Generator(np.random.PCG64(d))
    X = rng.normal(0, 0.1, (a.shape[0], d)).astype(np.float32)
    Xb = torch.from_numpy(X).to(torch.bfloat16).float().numpy()
    g = _graph(pkg, a, d_max=d)
    mk = g.dropout_mask(keep, SEED, step).cpu().numpy().astype(np.float64)
    A64 = sp.csr_matrix((a.data.astype(np.float64), a.indices, a.indptr), shape=a.shape)
    M = sp.csr_matrix((mk, a.indices, a.indptr), shape=a.shape)
    W = {0: A64.multiply(M).tocsr() / keep, 1: A64.multiply(M.T.tocsr()).tocsr() / keep}      # stored (i, j) carries keep(i, j) / keep(j, i)
    assert abs(W[0] - W[1]).sum() > 0
    x32, x16 = _dev(X), _dev(X).to(torch.bfloat16)
    for tr in (0, 1):
        ref, refb = W[tr] @ X.astype(np.float64), W[tr] @ Xb.astype(np.float64)
        got = g.spmm_drop(x32, keep, SEED, step, transposed=bool(tr)).cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-6 / keep, err_msg=f"fp32 tr={tr}")
        gotb = g.spmm_drop(x16, keep, SEED, step, transposed=bool(tr), y_dtype=pkg._lib.F32).cpu().numpy()
        np.testing.assert_allclose(gotb, refb, rtol=2e-5, atol=1e-6 / keep, err_msg=f"bf16 in tr={tr}")
        gotbb = g.spmm_drop(x16, keep, SEED, step, transposed=bool(tr)).float().cpu().numpy()
        np.testing.assert_allclose(gotbb, refb, rtol=1e-2, atol=1e-4, err_msg=f"bf16 in/out tr={tr}")
        # the other orientation is NOT within tolerance: the check above can tell them apart
        assert np.abs(got - (W[1 - tr] @ X.astype(np.float64))).max() > 1e-3
    # keep_prob = 1 is the plain product, bit for bit
    assert torch.equal(g.spmm_drop(x32, 1.0, SEED, step), g.spmm(x32))
    L = pkg._lib
    y = torch.empty_like(x32)
    for bad in (0.0, 1.5, float("nan")):
        assert L.load().lgcn_spmm_csr_drop(g.handle, L.tp(x32), 0, L.tp(y), 0, d, C.c_float(bad), SEED, step, 0, L.current_stream()) == 3
        assert b"dropout" in L.load().lgcn_last_error()
    torch.cuda.synchronize()
    g.close()


def _batches(K):
    """three steps (64 / 17 / 1 triplets) with duplicated users, pos-neg collisions and the long rows in every batch"""
    rng = np.random.Generator(np.random.PCG64(K))
    out = []
    for step, nb in enumerate((64, 17, 1)):
        u = rng.integers(0, N_USERS, nb); p = rng.integers(0, M_ITEMS, nb); n = rng.integers(0, M_ITEMS, nb)
        if step == 0:
            u[:8] = u[0]; p[:8] = p[0]; n[8:12] = p[0]          # duplicates / pos-neg collisions
            u[12:15] = 0; u[15] = 1                             # the chunked row (three times) and the two-tile row
        elif step == 1:
            u[0] = 1; u[1] = 0
        else:
            u[0] = 0
        out.append((u, p, n))
    return out


class _TorchRef:
    """The model's bpr_loss algebra with torch autograd on the CPU: fp32 sparse A_drop rebuilt from the exported mask of each
    step, K propagations, the layer mean including X_0, BPR + L2 term (either choice of rows), torch.optim.Adam."""

    def __init__(self, a, e0, K, decay, lr, reg_rows):
        self.a, self.K, self.decay, self.reg_rows = a, K, decay, reg_rows
        self.E = torch.tensor(e0, dtype=torch.float32, requires_grad=True)
        self.opt = torch.optim.Adam([self.E], lr=lr)
        self.rows = torch.from_numpy(_rows_of(a).astype(np.int64))
        self.cols = torch.from_numpy(a.indices.astype(np.int64))

    def step(self, mask, keep, u, p, n):
        vals = np.where(mask, a_scaled(self.a.data, keep), np.float32(0)).astype(np.float32)
        A = torch.sparse_coo_tensor(torch.stack([self.rows, self.cols]), torch.from_numpy(vals), self.a.shape).coalesce()
        x = acc = self.E
        for _ in range(self.K):
            x = torch.sparse.mm(A, x)
            acc = acc + x
        out = acc / float(self.K + 1)
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
        return float(loss)


def _run_vs_ref(pkg, tmp_path, adj, K, keep, dense_last, reg_rows, hub, tag):
    ds, m = _model(pkg, tmp_path, tag, K=K, dropout=1, keep=keep, dense_last=dense_last, reg_rows=reg_rows, hub=hub)
    m._state(max_batch=64, need_ctx=True)
    if hub is not None and dense_last == "0":
        assert pkg._lib.load().lgcn_ctx_hub_rows(m._dev['ctx']) == 2          # users 0 and 1 go through the hub plan
    w = pkg.world
    ref = _TorchRef(adj, m._table.cpu().numpy().copy(), K, w.config['decay'], w.config['lr'], reg_rows)
    bpr = pkg.utils.BPRLoss(m, w.config)
    for step, (u, p, n) in enumerate(_batches(K)):
        assert m.adam_step == step
        mask = m._dev['graph'].dropout_mask(keep, SEED, m.adam_step).cpu().numpy().astype(bool)
        if keep < 1.0:
            assert 0.5 < mask.mean() < 0.7
        l_ref = ref.step(mask, keep, u, p, n)
        l_got = bpr.stageOne(_dev(u), _dev(p), _dev(n))
        err = float(np.abs(m._table.cpu().numpy() - ref.E.detach().numpy()).max())
        print(f"{tag} K={K} keep={keep} dense_last={dense_last} reg={reg_rows} hub={hub} step {step}: loss {l_got:.7f} ref {l_ref:.7f} max|dP| {err:.2e}")
        assert abs(l_got - l_ref) < 3e-6, (tag, step, l_got, l_ref)
        np.testing.assert_allclose(m._table.cpu().numpy(), ref.E.detach().numpy(), rtol=0, atol=3e-6)
    assert int(m._dev['G64'].abs().sum()) == 0
    m.check_device_errors()
    return m


@pytest.mark.parametrize("K,dense_last,reg_rows,hub", [
    (1, "0", "propagated", None), (1, "1", "propagated", None),
    (2, "0", "propagated", None), (2, "1", "propagated", None),
    (3, "0", "propagated", None), (3, "1", "propagated", None),
    (3, "0", "ego", None), (3, "1", "ego", None),
    (3, "0", "propagated", 64), (1, "0", "ego", 64),
])
def test_fused_step_with_dropout_vs_torch_autograd(pkg, adj, tmp_path, K, dense_last, reg_rows, hub):
    """Three fused steps with dropout (keep 0.6, fp32 storage) against torch autograd on the CPU over the A_drop of each step's
    exported mask: loss and tables at the project's yardstick for this comparison (3e-6, test_fused_step_vs_oracle).  A mask
    applied untransposed in the backward, a second mask per step, or a layer that forgets the mask all miss it.  The same
    reference at keep_prob = 1 against the dropout-off step, so that a flaw of the reference shows apart from one of the feature."""
    _run_vs_ref(pkg, tmp_path, adj, K, 1.0, dense_last, reg_rows, hub, "off")
    _run_vs_ref(pkg, tmp_path, adj, K, 0.6, dense_last, reg_rows, hub, "drop")


def test_fused_step_with_dropout_bf16_storage(pkg, adj, tmp_path):
    """bf16 activation storage, K = 3: against the fp32-storage dropout run on the same batches and masks, at the bound the
    bf16 step tests use (test_fused_steps_other_dims_vs_oracle: loss 3e-3, tables 2e-3)."""
    out = {}
    for act in ("fp32", "bf16"):
        ds, m = _model(pkg, tmp_path, act, K=3, act=act, keep=0.6)
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        losses = [bpr.stageOne(_dev(u), _dev(p), _dev(n)) for (u, p, n) in _batches(3)]
        m.check_device_errors()
        out[act] = (losses, m._table.cpu().numpy().copy())
    for a, b in zip(out["fp32"][0], out["bf16"][0]):
        assert abs(a - b) < 3e-3, out
    np.testing.assert_allclose(out["bf16"][1], out["fp32"][1], rtol=0, atol=2e-3)
    assert not np.array_equal(out["bf16"][1], out["fp32"][1])


def _train(pkg, tmp_path, tag, steps, **kw):
    ds, m = _model(pkg, tmp_path, tag, **kw)
    bpr = pkg.utils.BPRLoss(m, pkg.world.config)
    rng = np.random.Generator(np.random.PCG64(77))
    batches = [tuple(_dev(rng.integers(0, hi, 64), torch.int32) for hi in (N_USERS, M_ITEMS, M_ITEMS)) for _ in range(4)]
    losses = [bpr.stageOne(*b) for b in batches[:steps]]
    return m, bpr, batches, losses


def _bits(m):
    return m._table.cpu().numpy().view(np.uint32).copy()


def test_off_means_off(pkg, tmp_path):
    """--dropout 1 --keepprob 1.0 and --dropout 0 (no setter call at all: the step as it was before this feature) give the same
    bits over 3 steps -- and dropout at 0.6 does not."""
    m0, _, _, l0 = _train(pkg, tmp_path, "d0", 3, dropout=0)
    m1, _, _, l1 = _train(pkg, tmp_path, "d1", 3, dropout=1, keep=1.0)
    m6, _, _, l6 = _train(pkg, tmp_path, "d6", 3, dropout=1, keep=0.6)
    assert l0 == l1 and np.array_equal(_bits(m0), _bits(m1))
    assert l0 != l6 and not np.array_equal(_bits(m0), _bits(m6))
    for m in (m0, m1, m6):
        m.check_device_errors()


def test_reproducible_resumable_and_epoch_call(pkg, tmp_path):
    ma, bpra, batches, la = _train(pkg, tmp_path, "a", 4)
    mb, _, _, lb = _train(pkg, tmp_path, "b", 4)
    assert la == lb and np.array_equal(_bits(ma), _bits(mb))                   # same seed: same bits
    mc, _, _, lc = _train(pkg, tmp_path, "c", 4, seed=1)
    assert not np.array_equal(_bits(ma), _bits(mc))                            # another seed: another run
    # 2 steps, save, load into a fresh model, 2 more steps (test_checkpoint_resume_roundtrip with dropout on)
    md, bprd, _, ld = _train(pkg, tmp_path, "d", 2)
    ckpt = os.path.join(str(tmp_path), "last.pth.tar")
    torch.save({'model_state': md.state_dict(), 'optimizer_state': bprd.opt.state_dict()}, ckpt)
    sd = torch.load(ckpt, weights_only=True)
    ds2, me = _model(pkg, tmp_path, "e")
    bpre = pkg.utils.BPRLoss(me, pkg.world.config)
    me.load_state_dict(sd['model_state'])
    bpre.opt.load_state_dict(sd['optimizer_state'])
    assert me.adam_step == 2
    le = [bpre.stageOne(*b) for b in batches[2:]]
    assert ld + le == la and np.array_equal(_bits(me), _bits(ma))
    # lgcn_train_epoch over the 4 batches = 4 lgcn_train_step calls
    ds3, mf = _model(pkg, tmp_path, "f")
    u, p, n = (torch.cat([b[i] for b in batches]) for i in range(3))
    lf = mf.fused_epoch(u, p, n, 64)
    assert [float(x) for x in lf[:, 0].cpu()] == la and np.array_equal(_bits(mf), _bits(ma))
    for m in (ma, mb, mc, md, me, mf):
        m.check_device_errors()


def test_evaluation_never_drops(pkg, adj, tmp_path):
    """After training with dropout, propagated_table() is lgcn_propagate_mean over the FULL graph of the current tables."""
    m, _, _, _ = _train(pkg, tmp_path, "ev", 2)
    m.eval()
    got = m.propagated_table()
    L = pkg._lib
    g = _graph(pkg, adj, d_max=64)
    N, d, K = N_USERS + M_ITEMS, 64, 3
    work = torch.zeros(K - 1, N, d, device=DEV)
    out = torch.empty(N, d, device=DEV)
    L.check(L.load().lgcn_propagate_mean(g.handle, L.tp(m._table), K, d, L.F32, L.tp(work), L.tp(out), L.current_stream()), "propagate")
    assert torch.equal(got, out)
    with torch.no_grad():
        au, ai = m.computer()
        assert torch.equal(torch.cat([au, ai]), out)
        r = m.getUsersRating(torch.arange(8, device=DEV))
    assert torch.allclose(r, out[:8] @ out[N_USERS:].t(), rtol=1e-6, atol=1e-7)
    m.check_device_errors()
    g.close()


def test_refusals_on_the_device(pkg, tmp_path):
    """No silent undropped path: contexts that cannot drop refuse the setter, and with dropout on every entry point that splits
    a step over ranks returns 3 and says why."""
    L = pkg._lib
    lib = L.load()
    for tag, kw in (("fp8", dict(act="fp8")), ("gate", dict(dense_last="1", extra={'use_pop_gate': True}))):
        ds, m = _model(pkg, tmp_path, tag, dropout=0, **kw)
        st = m._state(max_batch=64, need_ctx=True)
        assert lib.lgcn_ctx_set_dropout(st['ctx'], C.c_float(0.6), 1) == 3 and b"dropout" in lib.lgcn_last_error(), tag
    ds, m = _model(pkg, tmp_path, "dp", keep=0.6)
    st = m._state(max_batch=64, need_ctx=True)
    ctx = st['ctx']
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        assert lib.lgcn_ctx_set_dropout(ctx, C.c_float(bad), 1) == 3 and b"dropout" in lib.lgcn_last_error()
    u, p, n = (torch.zeros(64, dtype=torch.int32, device=DEV) for _ in range(3))
    loss = torch.zeros(3, device=DEV)
    gathered = torch.zeros(8, device=DEV)
    s = L.current_stream()
    part = C.c_void_p()
    calls = {
        "lgcn_train_step_dp_part1": lambda: lib.lgcn_train_step_dp_part1(ctx, L.tp(u), L.tp(p), L.tp(n), 64, 2, 0, s),
        "lgcn_train_step_dp_dense_part1": lambda: lib.lgcn_train_step_dp_dense_part1(ctx, L.tp(u), L.tp(p), L.tp(n), 64, 2, 0, s),
        "lgcn_train_step_dp_part2": lambda: lib.lgcn_train_step_dp_part2(ctx, L.tp(u), L.tp(p), L.tp(n), 64, 2, L.tp(gathered), L.tp(loss), s),
        "lgcn_train_step_cols_part1": lambda: lib.lgcn_train_step_cols_part1(ctx, L.tp(u), L.tp(p), L.tp(n), 64, C.byref(part), s),
        "lgcn_train_step_cols_part2": lambda: lib.lgcn_train_step_cols_part2(ctx, L.tp(u), L.tp(p), L.tp(n), 64, L.tp(loss), s),
        "lgcn_rs_phase": lambda: lib.lgcn_rs_phase(ctx, 0, 1, L.tp(u), L.tp(p), L.tp(n), 64, 2, 0, None, None, s),
        "lgcn_train_epoch_dp": lambda: lib.lgcn_train_epoch_dp(ctx, None, L.tp(u), L.tp(p), L.tp(n), 64, 64, 0, None, L.tp(gathered), L.tp(loss), s),
    }
    before = _bits(m)
    for name, call in calls.items():
        assert call() == 3, name
        msg = lib.lgcn_last_error()
        assert b"dropout" in msg and name.encode() in msg, (name, msg)
    assert m.adam_step == 0 and np.array_equal(_bits(m), before)             # nothing ran
    # switched off again, the same context trains like one that never heard of dropout
    assert lib.lgcn_ctx_set_dropout(ctx, C.c_float(1.0), 1) == 0
    assert lib.lgcn_train_step_dp_dense_part1(ctx, L.tp(u), L.tp(p), L.tp(n), 64, 1, 0, s) == 0
    assert lib.lgcn_train_step_dp_part2(ctx, L.tp(u), L.tp(p), L.tp(n), 64, 1, None, L.tp(loss), s) == 0
    torch.cuda.synchronize()
    m.check_device_errors()

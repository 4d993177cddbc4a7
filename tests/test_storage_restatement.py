"""CPU side of tests/test_gpu_storage_step.py: the float64 restatement of the default fused step with explicit storage points
(tests/storage_restatement.py) is the oracle's step when the quantiser is the identity, its backward is the straight-through
gradient, its bf16 / fp8 roundings are torch's casts bit for bit -- so the restatement IS the model before a kernel is judged
by it.  Then the cases of the GPU test (tests/storage_cases.py): the conditions on graph, table and batches, the byte-agreement
conditions met by the float32 twin alone, and the K = 4 allowance against an exact backward chain with stored tables.

Every step of a case starts from the float64 trajectory (restated gradient, restated Adam) rounded to fp32."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import storage_cases as SC                       # noqa: E402
import storage_restatement as S                  # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)

_CACHE = {}


def _inputs(pkg, case, path):
    """(adjacency CSR, dense float64 A, initial fp32 table) of a case; the graph objects once per session."""
    try:
        ds, m = SC.make_model(pkg, case, path)
        if "adj" not in _CACHE:
            adj = ds.getSparseGraphCSR()
            _CACHE["adj"], _CACHE["A"] = adj, S.dense_adj(adj)
        return _CACHE["adj"], _CACHE["A"], m._table.detach().numpy().copy()
    finally:
        pkg.world.configure([])


def _trajectory(A, case, table):
    """-> per step (fp32 table before it, float64 restatement at it)."""
    mode, d, K, dl, hub, reg = case
    p = table.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for i, batch in enumerate(SC.make_batches(case)):
        r = S.step(A, SC.N_USERS, K, SC.DECAY, p, batch, mode, bool(dl), reg == "ego")
        out.append((p.astype(np.float32), batch, r))
        p, m, v = S.adam(p, m, v, SC.np64(r["g_final"]), i + 1, SC.LR)
        p, m, v = (t.astype(np.float32).astype(np.float64) for t in (p, m, v))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_identity_quantiser_is_the_oracle_step(oracle, tiny, K, reg):
    """mode fp32 on the tiny fixture: loss (3e-6), the gradient the oracle's bpr + propagation gives (1e-5 of its max), the
    table after the oracle's first Adam step (3e-6: smoke()'s tolerances)."""
    z = tiny.z
    A = (z["adj_indptr"], z["adj_indices"], z["adj_data"])
    import scipy.sparse as sp
    adj = sp.csr_matrix((z["adj_data"], z["adj_indices"], z["adj_indptr"]), shape=(len(z["adj_indptr"]) - 1,) * 2)
    e0 = tiny.e0()
    u, p, n = z["b_users"], z["b_pos"], z["b_neg"]
    for dl in (False, True):
        r = S.step(S.dense_adj(adj), tiny.n_users, K, tiny.meta["decay"], e0, (u, p, n), "fp32", dl, reg == "ego")
        tr = oracle.Trainer(tiny.n_users, *A, e0, K, tiny.meta["decay"], tiny.meta["lr"], reg_rows=reg)
        l_ref = tr.stageOne(u, p, n)
        assert abs(float(r["loss_out"][0]) - l_ref) < 3e-6
        E = oracle.propagate(*A, e0, K)
        if reg == "ego":
            _, _, G, Gego = oracle.bpr_ego(E, e0, tiny.n_users, u, p, n, tiny.meta["decay"])
            g_ref = oracle.propagate_bwd(*A, G, K).astype(np.float64) + Gego
        else:
            g_ref = oracle.propagate_bwd(*A, oracle.bpr(E, tiny.n_users, u, p, n, tiny.meta["decay"])[2], K).astype(np.float64)
        g = SC.np64(r["g_final"])
        assert np.abs(g - g_ref).max() <= 1e-5 * np.abs(g_ref).max()
        p2 = S.adam(e0.astype(np.float64), 0.0 * g, 0.0 * g, g, 1, tiny.meta["lr"])[0]
        assert np.abs(p2 - tr.e0).max() < 3e-6


def test_identity_quantiser_is_the_oracle_step_on_the_case_graph(pkg, oracle, storage_graph):
    """The same on the graph of the storage cases (hub rows, an empty row, the hand-set table rows), K = 3, d = 64."""
    case = ("bf16", 64, 3, 0, -1, "propagated")
    adj, A, table = _inputs(pkg, case, storage_graph)
    batch = SC.make_batches(case)[0]
    r = S.step(A, SC.N_USERS, 3, SC.DECAY, table, batch, "fp32")
    csr = (adj.indptr, adj.indices, adj.data)
    tr = oracle.Trainer(SC.N_USERS, *csr, table, 3, SC.DECAY, SC.LR)
    assert abs(float(r["loss_out"][0]) - tr.stageOne(*batch)) < 3e-6
    g_ref = oracle.propagate_bwd(*csr, oracle.bpr(oracle.propagate(*csr, table, 3), SC.N_USERS, *batch, SC.DECAY)[2], 3).astype(np.float64)
    assert np.abs(SC.np64(r["g_final"]) - g_ref).max() <= 1e-5 * np.abs(g_ref).max()


@pytest.mark.parametrize("mode", ["bf16", "fp8"])
@pytest.mark.parametrize("K,dl", [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (4, 0)])
@pytest.mark.parametrize("reg", ["propagated", "ego"])
def test_backward_is_the_straight_through_gradient(pkg, storage_graph, mode, K, dl, reg):
    """torch autograd in float64 through the forward with Q as a straight-through function == the restated chain (no backward
    storage), to 1e-12."""
    case = (mode, 64, K, dl, -1, reg)
    adj, A, table = _inputs(pkg, case, storage_graph)
    batch = SC.make_batches(case)[2]
    r = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, mode, bool(dl), reg == "ego", q_bwd=False)
    E0 = torch.from_numpy(table).to(S.F64).requires_grad_(True)
    rows = S.slots(batch, SC.N_USERS)
    f = S.forward(A, E0, K, mode, bool(dl), rows, q=S.ste)
    b = S.bpr(f["e"], E0[rows.reshape(-1)].reshape(f["e"].shape), E0.shape[0], rows, K, SC.DECAY, reg == "ego")
    # the loss whose gradient the rows are: train_bpr's own fp32 constants inv_B = fl(1 / B) and lam = fl(decay / B), which differ
    # from the 1 / B and decay / B of loss_out in the last bit of an fp32 number (3e-8 for B = 37)
    inv_B, lam = S.constants(SC.DECAY, len(batch[0]))
    (-(inv_B * b["term"].sum()) + lam * 0.5 * b["regterm"].sum()).backward()
    assert abs(float(b["loss_out"][0].detach()) - float(r["loss_out"][0])) < 1e-15
    assert torch.equal(f["e"].detach(), r["e"])
    assert float((E0.grad - r["g_final"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("d", [64, 256])
def test_roundings_are_torchs_casts(d):
    """bf16_round / fp8_parts in float64 on fp32-representable input == torch's bfloat16 / float8_e4m3fn casts behind
    quantise_rows, bit for bit, zero / tiny / outlier / subnormal rows and exact ties included."""
    from test_gpu_fp8 import quantise_rows
    rng = np.random.Generator(np.random.PCG64(d))
    X = rng.normal(0, 0.1, (500, d)).astype(np.float32)
    X *= np.exp(rng.uniform(-30, 10, 500)).astype(np.float32)[:, None]
    X[5] = 0.0; X[6] = 1e-35; X[7, 3] = 7.0; X[7, 4:] *= 1e-6; X[8] *= np.float32(2.0 ** -20); X[9] /= 50.0; X[9, 1] = 0.1
    X[10] = (np.arange(d) + 0.5).astype(np.float32) * np.float32(2.0 ** -9)         # ties of the subnormal step (row max / scale in [64, 128) for d = 256)
    X[11] = np.float32(1.0) + np.arange(d).astype(np.float32) * np.float32(2.0 ** -9)      # bf16 ties
    x64 = torch.from_numpy(X).to(S.F64)
    assert torch.equal(S.bf16_round(x64), torch.from_numpy(X).to(torch.bfloat16).to(S.F64))
    b, s, dec = S.fp8_parts(x64)
    wb, ws = quantise_rows(X)
    assert np.array_equal(s, ws.astype(np.float64)) and np.array_equal(b, wb)
    b32, s32, dec32 = S.fp8_parts(torch.from_numpy(X))
    assert np.array_equal(dec.numpy(), dec32.numpy().astype(np.float64))
    assert s[5] == 1.0 and s[6] == 1.0 and not b[5].any() and not b[6].any()


def test_graph_and_table_conditions(pkg, storage_graph):
    case = SC.CASES[0]
    adj, A, table = _inputs(pkg, case, storage_graph)
    deg = np.diff(adj.indptr)
    assert adj.shape[0] == SC.N_USERS + SC.M_ITEMS
    assert deg[SC.HUB_USER] == SC.HUB_USER_DEG > 512 and deg[SC.N_USERS + SC.HUB_ITEM] == SC.HUB_ITEM_DEG
    assert deg[SC.N_USERS + SC.ISOLATED_ITEM] == 0 and (deg[SC.N_USERS - 10:SC.N_USERS] == 1).all()
    assert deg[SC.ZERO_USER] > 0 and not table[SC.ZERO_USER].any()
    for r, col in ((SC.N_USERS + SC.OUTLIER_ITEM, 3), (SC.N_USERS + SC.SUBNORMAL_ITEM, table.shape[1] - 2)):
        rest = np.delete(np.abs(table[r]), col)
        assert abs(table[r, col]) >= 50 * np.median(rest)
    b, s = S.fp8_parts(torch.from_numpy(table).to(S.F64))[:2]
    sub = b[SC.N_USERS + SC.SUBNORMAL_ITEM] & 0x7f
    assert (np.delete(sub, table.shape[1] - 2) < 8).all() and (sub > 0).sum() > 4          # exponent field 0: fp8 subnormals, not all flushed
    assert np.abs(table[SC.TINY_USER]).max() < 2.0 ** -20 and np.abs(table[SC.N_USERS + SC.BIG_ITEM]).max() > 6.4
    assert table[-1, 0] == np.float32(-0.2) and table[-1, -1] == np.float32(0.2) and deg[-1] > 0
    for c in SC.CASES + SC.K4_CASES:
        for (u, p, n) in SC.make_batches(c)[:3]:
            assert np.bincount(p).max() >= 6 and (p == n).any() and (u == SC.HUB_USER).sum() >= 2
            assert (p == SC.HUB_ITEM).any() and (n == SC.HUB_ITEM).any() and (n == SC.ISOLATED_ITEM).any()


@pytest.mark.parametrize("case", SC.CASES + SC.K4_CASES, ids=SC.case_id)
def test_case_conditions_and_twin(pkg, storage_graph, case):
    """Per step of the case's float64 trajectory: no sigmoid is saturated; every stored table rounds elements both ways; rows
    outside the batch's reach exist for K <= 2 (one-triplet batch); fp8: the float32 twin, restated link by link on the float64
    chain's stored tables, meets the byte-agreement conditions (scale equal on > 99.5 % of the rows, bytes on > 99.9 % of their
    elements) for every stored table; and it stays within every derived bound, so the bounds admit an honest fp32 evaluation."""
    mode, d, K, dl, hub, reg = case
    adj, A, table = _inputs(pkg, case, storage_graph)
    for i, (p, batch, r) in enumerate(_trajectory(A, case, table)):
        s = torch.sigmoid(-r["x"])
        assert 0.01 < float(s.min()) and float(s.max()) < 0.99, (i, float(s.min()), float(s.max()))
        stored = [(r["fwd_pre"][k], r["fwd"][k]) for k in r["fwd"]] + [(r["bwd_pre"][j], r["bwd"][j]) for j in r["bwd"]]
        for pre, q in stored:
            live = pre != 0
            up = float((q > pre)[live].double().mean())
            assert 0.1 < up < 0.9, (i, up)
        if K <= 2 and len(batch[0]) == 1:
            assert not SC.reach(adj, r["rows"], K).all()
        custody = {"e0s": r["e0s"].float(), "fwd": {k: t.float() for k, t in r["fwd"].items()}, "bwd": {j: t.float() for j, t in r["bwd"].items()}}
        t = S.step(A, SC.N_USERS, K, SC.DECAY, p, batch, mode, bool(dl), reg == "ego", dtype=S.F32, custody=custody)
        dl_ = SC.step_deltas(adj, r, K, bool(dl), reg == "ego")
        for key in ("term", "regterm", "gb"):
            assert (np.abs(SC.np64(t[key]) - SC.np64(r[key])) <= dl_[key]).all(), (i, key)
        assert (np.abs(SC.np64(t["g_final"]) - SC.np64(r["g_final"])) <= dl_["g_final"]).all(), i
        pairs = [(t["fwd_pre"][k], r["fwd_pre"][k], SC.spmm_delta(adj, SC.np64(r["e0s"] if k == 1 else r["fwd"][k - 1]))) for k in r["fwd"]]
        pairs += [(t["bwd_pre"][j], r["bwd_pre"][j], dl_["bwd_pre"][j]) for j in r["bwd"]]
        for got, ref, delta in pairs:
            assert (np.abs(SC.np64(S.quantise(got, mode)) - SC.np64(ref)) <= SC.stored_bound(SC.np64(ref), delta, mode)).all(), i
            if mode == "fp8":
                gb_, gs_, _ = S.fp8_parts(got)
                rb_, rs_, _ = S.fp8_parts(ref)
                rows_ok, bytes_ok = SC.bytes_agree(gb_, gs_, rb_, rs_)
                assert rows_ok > 0.995 and bytes_ok > 0.999, (i, rows_ok, bytes_ok, "change the case's batch seed (BATCH_SEED)")


@pytest.mark.parametrize("case", SC.K4_CASES, ids=SC.case_id)
def test_k4_allowance_holds_against_the_exact_chain(pkg, storage_graph, case):
    """The four-layer backward chain with stored tables (three of them, ping-ponging over two buffers on the GPU) against the
    chain without storage: within k4_allowance element by element, and the allowance is not idle (some element uses > 1 %)."""
    mode, d, K, dl, hub, reg = case
    adj, A, table = _inputs(pkg, case, storage_graph)
    for batch in SC.make_batches(case):
        on = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, mode)
        off = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, mode, q_bwd=False)
        assert torch.equal(on["G"], off["G"])
        allow = SC.k4_allowance(adj, SC.np64(off["G"]), K, mode)
        err = np.abs(SC.np64(on["g_final"]) - SC.np64(off["g_final"]))
        assert (err <= allow).all(), float((err / np.maximum(allow, 1e-300)).max())
        assert (err > 0.01 * allow).any()


# ---- the two features: layer weights and edge dropout (storage_cases.FEATURE_CASES) ---------------------------------------
def _rel(a, b):
    a, b = SC.np64(a), SC.np64(b)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _autograd64(a, table, w, batch, reg, exact_w=None):
    """One step of test_gpu_layer_weights._WeightedRef in float64 on the CSR `a` (explicit zeros allowed) -> (loss, gradient,
    table after torch.optim.Adam's first step).  The batch has 64 triplets and decay is fl32(DECAY), so that train_bpr's fp32
    constants inv_B = fl32(1 / B) and lam = fl32(fl32(decay) / B) ARE the reference's 1 / B and decay / B (a power of two divides
    exactly) and the two sides differ by float64 rounding alone.  exact_w: weights that are no fp32 numbers (the mean's 1 / (K + 1))."""
    import test_gpu_layer_weights as LW
    assert LW.N_USERS == SC.N_USERS and len(batch[0]) == 64
    ref = LW._WeightedRef(a, table, w, float(np.float32(SC.DECAY)), SC.LR, reg, torch.float64)
    if exact_w is not None:
        ref.w = list(exact_w)
    loss = ref.step(*batch)
    return loss, ref.E.grad.detach().clone(), ref.table()


def _against_autograd(r, table, loss, grad, after):
    g = SC.np64(r["g_final"])
    p2 = S.adam(table.astype(np.float64), 0.0 * g, 0.0 * g, g, 1, SC.LR)[0]
    return abs(float(r["loss_out"][0]) - loss) / abs(loss), _rel(g, grad), _rel(p2, after)


# measured on the CPU, the largest over both parametrisations below, relative to the largest element: loss equal in every digit
# (so: ten float64 roundings, 2.2e-16 each), gradient 1.8e-15, table after Adam 2.2e-16; each bound keeps a factor of 10
AUTOGRAD_BOUND = {"loss": 2.2e-15, "grad": 1.8e-14, "table": 2.2e-15}


def _assert_autograd(errs, what):
    for (k, bound), e in zip(AUTOGRAD_BOUND.items(), errs):
        assert e <= bound, (what, k, e)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["exp", "midzero", "last", "first"])
def test_weights_identity_quantiser_is_float64_autograd(pkg, storage_graph, K, name):
    """weights = w, mode fp32, on the storage graph (d = 64, the first batch): loss, gradient and the table after one Adam step
    against torch autograd in float64 through test_gpu_layer_weights._WeightedRef's algebra (out = sum_k w_k X_k), both reg_rows
    and both dense_last.  float64 against float64; measured: loss equal, gradient 1.8e-15, table 2.2e-16 (AUTOGRAD_BOUND keeps a
    factor of 10)."""
    from test_gpu_layer_weights import weight_set
    case = ("fp32", 64, K, 0, -1, "propagated")
    adj, A, table = _inputs(pkg, case, storage_graph)
    batch = SC.make_batches(case)[0]
    w = weight_set(name, K)
    worst = [0.0, 0.0, 0.0]
    for reg in ("propagated", "ego"):
        loss, grad, after = _autograd64(adj, table, w, batch, reg)
        for dl in (False, True):
            r = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, "fp32", dl, reg == "ego", weights=w)
            assert torch.equal(r["Gs"], r["G"])                                    # unscaled
            errs = _against_autograd(r, table, loss, grad, after)
            _assert_autograd(errs, (K, name, reg, dl))
            worst = [max(a, b) for a, b in zip(worst, errs)]
    print(f"[storage_restatement] weights K={K} {name}: loss {worst[0]:.1e} grad {worst[1]:.1e} table {worst[2]:.1e}")


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_uniform_weights_are_the_mean(pkg, storage_graph, K):
    """weights = 1 / (K + 1) (the float64 quotient) give the mean restatement: slot rows, loss and gradient to float64 rounding
    (measured 4.9e-16 relative at most; asserted 5e-15), with storage on (bf16 forward tables are the same numbers: Q sits behind A X)."""
    case = ("bf16", 64, K, 0, -1, "propagated")
    adj, A, table = _inputs(pkg, case, storage_graph)
    batch = SC.make_batches(case)[1]
    for dl in (False, True):
        for reg in (False, True):
            a = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, "bf16", dl, reg, q_bwd=False)
            b = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, "bf16", dl, reg, q_bwd=False, weights=[1.0 / (K + 1)] * (K + 1))
            for k in a["fwd"]:
                assert torch.equal(a["fwd"][k], b["fwd"][k])
            errs = (_rel(b["e"], a["e"]), abs(float(b["loss_out"][0]) - float(a["loss_out"][0])) / abs(float(a["loss_out"][0])), _rel(b["g_final"], a["g_final"]))
            print(f"[storage_restatement] uniform K={K} dl={dl} ego={reg}: e {errs[0]:.1e} loss {errs[1]:.1e} grad {errs[2]:.1e}")
            assert max(errs) <= 5e-15, errs


def test_stored_weights_are_symmetric_and_keep_one_is_the_default_step(pkg, storage_graph):
    """(1) A_hat's fp32 values are symmetric bit for bit, so the matrix the backward launches read (the weight stored at (i, j)
    under keep(j, i)) IS the explicit transpose of A_drop, and the two are not equal; (2) keep = 1 -- a_scaled and _keep_host
    evaluated, not short-cut -- gives A itself and the default restatement bit for bit, every output."""
    import dropout_restatement as DR
    import scipy.sparse as sp
    case = ("bf16", 64, 3, 0, -1, "propagated")
    adj, A, table = _inputs(pkg, case, storage_graph)
    assert (adj != adj.T).nnz == 0
    fwd, bwd = DR.dropped_graphs(adj, 0.6, SC.DROP_SEED, 2)
    assert (bwd != fwd.T.tocsr()).nnz == 0 and (bwd != fwd).nnz > 0.3 * adj.nnz
    kept = fwd.data != 0
    assert abs(kept.mean() - 0.6) < 0.05 and np.array_equal(fwd.data[kept], DR.a_scaled(adj.data, 0.6)[kept])
    rows = DR._rows_of(adj)
    assert DR._keep_host(rows, adj.indices, 1.0, SC.DROP_SEED, 2).all() and np.array_equal(DR.a_scaled(adj.data, 1.0), adj.data)
    one = S.dense_adj(sp.csr_matrix((np.where(DR._keep_host(rows, adj.indices, 1.0, SC.DROP_SEED, 2), DR.a_scaled(adj.data, 1.0), np.float32(0)),
                                     adj.indices, adj.indptr), shape=adj.shape))
    for batch in SC.make_batches(case)[:2]:
        a = S.step(A, SC.N_USERS, 3, SC.DECAY, table, batch, "bf16")
        b = S.step(A, SC.N_USERS, 3, SC.DECAY, table, batch, "bf16", A_fwd=one, A_bwd=one.t().contiguous())
        for k in ("e", "G", "Gs", "g_final", "term", "regterm", "terms_abs"):
            assert torch.equal(a[k], b[k]), k
        for k in ("fwd", "fwd_pre", "bwd", "bwd_pre"):
            assert all(torch.equal(a[k][j], b[k][j]) for j in a[k]), k
        assert all(float(x) == float(y) for x, y in zip(a["loss_out"], b["loss_out"]))


@pytest.mark.parametrize("K", [1, 2, 3])
def test_dropout_identity_quantiser_is_float64_autograd(pkg, storage_graph, K):
    """A_fwd = A_drop, A_bwd = A_drop^T from _keep_host (keep 0.6, step 1), mode fp32: loss, gradient and table after Adam against
    torch autograd in float64 over the sparse A_drop (test_gpu_dropout._TorchRef's algebra: the layer mean), both reg_rows and
    both dense_last, within AUTOGRAD_BOUND (measured: loss equal, gradient 4.4e-16, table 3.0e-17).  And the transpose is REQUIRED: the same
    restatement with A_bwd = A_fwd misses the gradient by more than 1e-2 of its largest element (measured 0.257 at least),
    twelve orders of magnitude beyond the bound -- so a kernel that forgets dr.tr cannot pass the GPU test."""
    case = ("fp32", 64, K, 0, -1, "propagated")
    adj, A, table = _inputs(pkg, case, storage_graph)
    batch = SC.make_batches(case)[0]
    fwd, bwd = SC.case_graphs(adj, case + (("drop", 0.6),), 1)
    Af, Ab = S.dense_adj(fwd), S.dense_adj(bwd)
    for reg in ("propagated", "ego"):
        loss, grad, after = _autograd64(fwd, table, np.ones(K + 1, np.float32), batch, reg, exact_w=[1.0 / (K + 1)] * (K + 1))
        for dl in (False, True):
            r = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, "fp32", dl, reg == "ego", A_fwd=Af, A_bwd=Ab)
            errs = _against_autograd(r, table, loss, grad, after)
            print(f"[storage_restatement] dropout K={K} {reg} dl={dl}: loss {errs[0]:.1e} grad {errs[1]:.1e} table {errs[2]:.1e}")
            _assert_autograd(errs, (K, reg, dl))
            wrong = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, "fp32", dl, reg == "ego", A_fwd=Af, A_bwd=Af)
            miss = _rel(wrong["g_final"], grad)
            print(f"[storage_restatement] dropout K={K} {reg} dl={dl}: untransposed backward misses by {miss:.2e}")
            assert miss > 1e-2
            plain = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, "fp32", dl, reg == "ego")
            assert _rel(plain["g_final"], grad) > 1e-2                            # (and so does the undropped step)


def _feature_trajectory(adj, A, case, table):
    """_trajectory for a case with a feature -> per step (fp32 table before it, batch, float64 restatement, weights, (forward CSR,
    backward CSR), their dense forms)."""
    mode, d, K, dl, hub, reg = case[:6]
    w = SC.case_weights(case)
    p = table.astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    out = []
    for i, batch in enumerate(SC.make_batches(case)):
        fwd, bwd = SC.case_graphs(adj, case, i)
        Af, Ab = (A, A) if fwd is adj else (S.dense_adj(fwd), S.dense_adj(bwd))
        r = S.step(A, SC.N_USERS, K, SC.DECAY, p, batch, mode, bool(dl), reg == "ego", weights=w, A_fwd=Af, A_bwd=Ab)
        out.append((p.astype(np.float32), batch, r, w, (fwd, bwd), (Af, Ab)))
        p, m, v = S.adam(p, m, v, SC.np64(r["g_final"]), i + 1, SC.LR)
        p, m, v = (t.astype(np.float32).astype(np.float64) for t in (p, m, v))
    return out


def test_feature_batches_hold_every_row_form():
    """test_graph_and_table_conditions' conditions on the batches, for the cases with a feature."""
    for c in SC.FEATURE_CASES + SC.FEATURE_K4_CASES:
        for (u, p, n) in SC.make_batches(c)[:3]:
            assert np.bincount(p).max() >= 6 and (p == n).any() and (u == SC.HUB_USER).sum() >= 2
            assert (p == SC.HUB_ITEM).any() and (n == SC.HUB_ITEM).any() and (n == SC.ISOLATED_ITEM).any()
    ids = [SC.case_id(c) for c in SC.CASES + SC.K4_CASES + SC.FEATURE_CASES + SC.FEATURE_K4_CASES]
    assert len(set(ids)) == len(ids)


@pytest.mark.parametrize("case", SC.FEATURE_CASES + SC.FEATURE_K4_CASES, ids=SC.case_id)
def test_feature_case_conditions_and_twin(pkg, storage_graph, case):
    """test_case_conditions_and_twin for the cases with layer weights or dropout, per step of the case's float64 trajectory: no
    sigmoid is saturated; every bf16 table that is not zero by construction (weights `first`: the backward tables are 0 G + 0 A G)
    rounds elements both ways; rows outside the reach of the backward's own graph exist for K <= 2 (one-triplet batch); under
    dropout the kept share is keep +- 0.05 and the long rows lose entries; and the float32 twin, restated link by link on the
    float64 chain's stored tables, stays within every derived bound, so the bounds admit an honest fp32 evaluation."""
    mode, d, K, dl, hub, reg = case[:6]
    adj, A, table = _inputs(pkg, case, storage_graph)
    for i, (p, batch, r, w, (fwd, bwd), (Af, Ab)) in enumerate(_feature_trajectory(adj, A, case, table)):
        s = torch.sigmoid(-r["x"])
        assert 0.01 < float(s.min()) and float(s.max()) < 0.99, (i, float(s.min()), float(s.max()), "change the case's batch seed (BATCH_SEED)")
        if SC.case_keep(case) < 1.0:
            kept = fwd.data != 0
            assert abs(kept.mean() - SC.case_keep(case)) <= 0.05
            hub_row = slice(adj.indptr[SC.HUB_USER], adj.indptr[SC.HUB_USER + 1])
            assert 0 < (~kept[hub_row]).sum() < SC.HUB_USER_DEG and (bwd != fwd).nnz > 0
        stored = [(r["fwd_pre"][k], r["fwd"][k]) for k in r["fwd"]] + [(r["bwd_pre"][j], r["bwd"][j]) for j in r["bwd"]]
        for pre, q in stored:
            live = pre != 0
            if mode == "bf16" and bool(live.any()):
                up = float((q > pre)[live].double().mean())
                assert 0.1 < up < 0.9, (i, up)
            elif mode == "bf16":
                assert w is not None and SC.feature(case)[1] == "first"
        if K <= 2 and len(batch[0]) == 1:
            assert not SC.reach(bwd, r["rows"], K).all()
        custody = {"e0s": r["e0s"].float(), "fwd": {k: t.float() for k, t in r["fwd"].items()}, "bwd": {j: t.float() for j, t in r["bwd"].items()}}
        t = S.step(A, SC.N_USERS, K, SC.DECAY, p, batch, mode, bool(dl), reg == "ego", dtype=S.F32, custody=custody, weights=w, A_fwd=Af, A_bwd=Ab)
        dl_ = SC.step_deltas(fwd, r, K, bool(dl), reg == "ego", w, bwd)
        for key in ("term", "regterm", "gb"):
            assert (np.abs(SC.np64(t[key]) - SC.np64(r[key])) <= dl_[key]).all(), (i, key)
        assert (np.abs(SC.np64(t["g_final"]) - SC.np64(r["g_final"])) <= dl_["g_final"]).all(), i
        pairs = [(t["fwd_pre"][k], r["fwd_pre"][k], SC.spmm_delta(fwd, SC.np64(r["e0s"] if k == 1 else r["fwd"][k - 1]))) for k in r["fwd"]]
        pairs += [(t["bwd_pre"][j], r["bwd_pre"][j], dl_["bwd_pre"][j]) for j in r["bwd"]]
        for got, ref, delta in pairs:
            assert (np.abs(SC.np64(S.quantise(got, mode)) - SC.np64(ref)) <= SC.stored_bound(SC.np64(ref), delta, mode)).all(), i


@pytest.mark.parametrize("case", SC.FEATURE_K4_CASES, ids=SC.case_id)
def test_feature_k4_allowance_holds_against_the_exact_chain(pkg, storage_graph, case):
    """test_k4_allowance_holds_against_the_exact_chain with the chain's own coefficients and the backward's own matrix."""
    mode, d, K, dl, hub, reg = case[:6]
    adj, A, table = _inputs(pkg, case, storage_graph)
    w = SC.case_weights(case)
    for i, batch in enumerate(SC.make_batches(case)):
        fwd, bwd = SC.case_graphs(adj, case, i)
        kw = dict(weights=w, A_fwd=S.dense_adj(fwd), A_bwd=S.dense_adj(bwd))
        on = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, mode, **kw)
        off = S.step(A, SC.N_USERS, K, SC.DECAY, table, batch, mode, q_bwd=False, **kw)
        assert torch.equal(on["G"], off["G"])
        allow = SC.feature_k4_allowance(bwd, SC.np64(off["G"]), K, w)
        err = np.abs(SC.np64(on["g_final"]) - SC.np64(off["g_final"]))
        assert (err <= allow).all(), float((err / np.maximum(allow, 1e-300)).max())
        assert (err > 0.01 * allow).any()
    uni = SC.feature_k4_allowance(adj, SC.np64(off["G"]), K)
    assert np.allclose(uni, SC.k4_allowance(adj, SC.np64(off["G"]), K, "bf16"), rtol=1e-12, atol=0)          # the mean's coefficients: storage_allowance

"""The store policy of the outputs nobody gathers (lgcn_ctx_set_store_policy).

Under LGCN_STORE_ADAM the Adam epilogue writes M and V (and P, where a bf16 / fp8 shadow is gathered in its place) with
write-through stores; under LGCN_STORE_XLAST the forward launch of X_{K-1} does the same for the table only the batch-row kernel
gathers.  Only HOW the bytes leave the chip changes, so the contract is identity: loss_out of every step, P, M, V and the error
flag under the policies 0, 1 and 3 are compared with torch.equal, never with a tolerance -- in one lgcn_train_epoch call of
three steps and in three lgcn_train_step calls.

The graph: 1 150 users x 350 items = 1 500 rows.  User rows of 1, 8, 9, 63 and 64 non-zeros (the pack boundaries of the short
path), item 1 with 300 users (a long row one wave finishes) and item 0 with 1 100 (three chunks of LONG_CH = 512: the epilogue
runs in the last arriver)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the 300 x 600 graph, written once per session)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_USERS, M_ITEMS = 1150, 350
N = N_USERS + M_ITEMS
SPECIAL = {1100: 1, 1101: 8, 1102: 9, 1103: 63, 1104: 64}       # user -> number of items
DS, ACTS, KS, BS = (32, 64, 128, 256), ("fp32", "bf16", "fp8"), (1, 2, 3), (1, 7, 67)
STEPS = 3
POLICIES = (0, 1, 3)


@pytest.fixture(scope="module")
def graph_dir(tmp_path_factory):
    path = os.path.join(str(tmp_path_factory.mktemp("storegraph")), "storegraph")
    os.makedirs(path)
    rng = np.random.Generator(np.random.PCG64(2424))
    with open(os.path.join(path, "train.txt"), "w") as f, open(os.path.join(path, "test.txt"), "w") as ft:
        for u in range(N_USERS):
            if u in SPECIAL:
                items = 2 + rng.choice(M_ITEMS - 3, size=SPECIAL[u], replace=False)
            else:
                items = 2 + rng.choice(M_ITEMS - 3, size=int(rng.integers(1, 7)), replace=False)
                if u < 1100:
                    items = np.append(items, 0)
                if u < 300:
                    items = np.append(items, 1)
            f.write(f"{u} " + " ".join(map(str, np.sort(items).tolist())) + "\n")
            ft.write(f"{u} {M_ITEMS - 1}\n")
    return path


def _model(pkg, path, d, act, K, B, dense_last=0, flags=()):
    w = pkg.world
    w.configure(["--dataset", "storegraph", "--tensorboard", "0", "--layer", str(K), "--recdim", str(d), "--bpr_batch", str(B),
                 "--act_dtype", act] + list(flags))
    w.config.update({'dense_last': str(dense_last), 'row_order': 'rcm'})
    w.config['checkpoint_dir'] = os.path.join(os.path.dirname(path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=path)
    pkg.utils.set_seed(23)
    m = pkg.model.LightGCN(w.config, ds).to(DEV)
    m.train()
    assert (ds.n_users, ds.m_items) == (N_USERS, M_ITEMS)
    m.set_adam_step(0)                                 # makes the training context
    return m


def test_graph_has_the_rows_the_cases_need(pkg, graph_dir):
    try:
        m = _model(pkg, graph_dir, 32, "fp32", 1, 7)
        deg = np.diff(m._adj.indptr)
    finally:
        pkg.world.configure([])
    assert len(deg) == N
    assert [int(deg[u]) for u in SPECIAL] == [1, 8, 9, 63, 64]
    assert deg[N_USERS] == 1100 and deg[N_USERS + 1] == 300          # 2 < 1100 / 512 <= 3 chunks; 64 < 300 <= 512: one wave
    assert sorted(deg)[-3] <= 64                                        # every other row takes the short path


def _triplets(B, seed):
    """ids of 3 batches of B; the special users and both long items are named in every batch that has room"""
    rng = np.random.Generator(np.random.PCG64(seed))
    T = STEPS * B
    u, p, n = rng.integers(0, N_USERS, T), rng.integers(0, M_ITEMS, T), rng.integers(0, M_ITEMS, T)
    if B >= 7:
        for s in range(STEPS):
            u[s * B:s * B + 5] = list(SPECIAL)
            p[s * B + 5], n[s * B + 6] = 0, 1
    return tuple(torch.from_numpy(x).to(torch.int32).to(DEV) for x in (u, p, n))


def _set_policy(pkg, m, bits):
    pkg._lib.check(pkg._lib.load().lgcn_ctx_set_store_policy(m._dev['ctx'], bits), "lgcn_ctx_set_store_policy")


def _get_policy(pkg, m):
    out = (C.c_int32 * 2)(-1, -1)
    bits = pkg._lib.load().lgcn_ctx_get_store_policy(m._dev['ctx'], out)
    return bits, out[0], out[1]


def _reset(pkg, m, init):
    """the model as it was made: the table, zero moments, step 0"""
    with torch.no_grad():
        m._table.copy_(init)
    m._dev['adam_m'].zero_()
    m._dev['adam_v'].zero_()
    m.invalidate_cache()
    pkg._lib.load().lgcn_ctx_set_step(m._dev['ctx'], 0)


def _err(pkg, m):
    try:
        m.check_device_errors()
        return 0
    except pkg._lib.LgcnError:
        return 1


def _snapshot(pkg, m, losses):
    torch.cuda.synchronize()
    return (losses.clone(), m._table.detach().clone(), m._dev['adam_m'].clone(), m._dev['adam_v'].clone(), _err(pkg, m))


def _run(pkg, m, init, ids, B, bits, epoch):
    _reset(pkg, m, init)
    _set_policy(pkg, m, bits)
    U, P, Nn = ids
    if epoch:
        losses = m.fused_epoch(U, P, Nn, B)
    else:
        losses = torch.stack([m.fused_step(U[s * B:(s + 1) * B], P[s * B:(s + 1) * B], Nn[s * B:(s + 1) * B]).clone() for s in range(STEPS)])
    assert tuple(losses.shape) == (STEPS, 3)
    return _snapshot(pkg, m, losses)


def _same(a, b, what):
    for name, x, y in zip(("loss_out", "P", "M", "V"), a[:4], b[:4]):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, name, int((x != y).sum()))
    assert a[4] == b[4] == 0, (what, "error flag")


def _identity(pkg, path, d, act, K, B, flags=()):
    try:
        m = _model(pkg, path, d, act, K, B, flags=flags)
        init = m._table.detach().clone()
        ids = _triplets(B, 100 * d + 10 * K + B)
        for epoch in (True, False):
            ref = _run(pkg, m, init, ids, B, 0, epoch)
            assert torch.isfinite(ref[0]).all() and not torch.equal(ref[1], init) and bool(ref[2].any()) and bool(ref[3].any())
            for bits in POLICIES[1:]:
                got = _run(pkg, m, init, ids, B, bits, epoch)
                pol, wt_adam, wt_fwd = _get_policy(pkg, m)
                L = pkg._lib
                assert pol == bits and (wt_adam & L.STORE_ARG_MV)                           # the launches did carry the policy
                assert bool(wt_adam & L.STORE_ARG_P) == (epoch and act != "fp32" and K >= 2)
                assert wt_fwd == (L.STORE_ARG_Y if (bits & L.STORE_XLAST) and K >= 2 and act != "fp8" else 0)
                _same(ref, got, f"policy {bits} {'epoch' if epoch else 'steps'}")
    finally:
        pkg.world.configure([])


def _cases():
    """every (d, storage, K); B rotates so that every (storage, K) pair meets 1, 7 and 67 over its widths"""
    out = []
    for di, d in enumerate(DS):
        for ai, act in enumerate(ACTS):
            if act == "fp8" and d < 64:
                continue
            for ki, K in enumerate(KS):
                out.append((d, act, K, BS[(di + ai + ki) % 3]))
    return out


def test_case_rotation_covers_every_pair():
    cs = _cases()
    for act in ACTS:
        for K in KS:
            at = [c for c in cs if c[1] == act and c[2] == K]
            assert {c[0] for c in at} == {d for d in DS if act != "fp8" or d >= 64}, (act, K)
            assert {c[3] for c in at} == set(BS), (act, K)


@pytest.mark.parametrize("d,act,K,B", [pytest.param(*c, id=f"d{c[0]}-{c[1]}-K{c[2]}-B{c[3]}") for c in _cases()])
def test_policies_are_bitwise_identical(pkg, graph_dir, d, act, K, B):
    """policies 0, 1 and 3 from one state: 3 steps in one lgcn_train_epoch call, and 3 lgcn_train_step calls"""
    _identity(pkg, graph_dir, d, act, K, B)


@pytest.mark.parametrize("what", ["dropout", "layer_weights"])
def test_policies_with_the_other_instantiations(pkg, graph_dir, what):
    """the DROP and the M_WTS instantiations share the epilogue"""
    if what == "dropout":
        _identity(pkg, graph_dir, 64, "bf16", 3, 67, flags=["--dropout", "1", "--keepprob", "0.7"])
    else:
        _identity(pkg, graph_dir, 128, "fp32", 3, 67, flags=["--layer_weights", "[0.4,0.3,0.2,0.1]"])


@pytest.mark.parametrize("act", ["fp32", "bf16", "fp8"])
def test_written_through_rows_are_visible_to_everyone(pkg, graph_dir, act):
    """after a policy-3 call P, M and V are read from another stream and through .cpu(); one more step under policy 0 on the
    same context then gives what four policy-0 steps give"""
    d, K, B = 64, 3, 67
    try:
        m = _model(pkg, graph_dir, d, act, K, B)
        init = m._table.detach().clone()
        ids = _triplets(B, 77)
        rng = np.random.Generator(np.random.PCG64(78))
        extra = tuple(torch.from_numpy(rng.integers(0, hi, B)).to(torch.int32).to(DEV) for hi in (N_USERS, M_ITEMS, M_ITEMS))
        ref3 = _run(pkg, m, init, ids, B, 0, True)
        ref4 = _snapshot(pkg, m, m.fused_step(*extra).clone().reshape(1, 3))
        _reset(pkg, m, init)
        _set_policy(pkg, m, 3)
        losses = m.fused_epoch(*ids, B)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream())
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            side.wait_event(done)
            seen = [t.detach().clone() for t in (m._table, m._dev['adam_m'], m._dev['adam_v'])]
        side.synchronize()
        host = [t.detach().cpu() for t in (m._table, m._dev['adam_m'], m._dev['adam_v'])]
        for name, want, s, h in zip("PMV", ref3[1:4], seen, host):
            assert torch.equal(want, s), (name, "other stream")
            assert torch.equal(want.cpu(), h), (name, ".cpu()")
        assert torch.equal(ref3[0], losses)
        _set_policy(pkg, m, 0)
        got4 = _snapshot(pkg, m, m.fused_step(*extra).clone().reshape(1, 3))
        _same(ref4, got4, "policy 0 after policy 3")
    finally:
        pkg.world.configure([])


def test_launch_arguments_follow_the_tables(pkg, graph_dir):
    """fp32 tables gather P itself: under policy 1 its stores stay plain; a dense last layer is read by slot, not gathered: plain"""
    L = pkg._lib
    B = 7
    try:
        for act, dense_last, bits, epoch, want_adam, want_fwd in (
                ("fp32", 0, 1, True, L.STORE_ARG_MV, 0),
                ("fp32", 0, 3, True, L.STORE_ARG_MV, L.STORE_ARG_Y),
                ("bf16", 0, 1, True, L.STORE_ARG_MV | L.STORE_ARG_P, 0),
                ("bf16", 0, 1, False, L.STORE_ARG_MV, 0),             # a single step keeps no shadow: the next one converts P
                ("fp8", 0, 3, True, L.STORE_ARG_MV | L.STORE_ARG_P, 0),   # fp8 tables: X_{K-1} stays plain (no registers to spare)
                ("bf16", 1, 3, True, L.STORE_ARG_MV | L.STORE_ARG_P, 0),
                ("bf16", 0, 2, True, 0, L.STORE_ARG_Y),
                ("bf16", 0, 0, True, 0, 0)):
            m = _model(pkg, graph_dir, 64, act, 3, B, dense_last=dense_last)
            assert _get_policy(pkg, m)[1:] == (0, 0)                  # nothing launched yet
            _run(pkg, m, m._table.detach().clone(), _triplets(B, 5), B, bits, epoch)
            assert _get_policy(pkg, m) == (bits, want_adam, want_fwd), (act, dense_last, bits, epoch)
        assert L.load().lgcn_ctx_set_store_policy(m._dev['ctx'], 4) == 3 and _get_policy(pkg, m)[0] == 0
    finally:
        pkg.world.configure([])


def test_failed_setter_leaves_no_context(pkg, storage_graph):
    """config['store_policy'] = 8, an unknown bit: the library refuses the last setter of the context builder with rc 3.  The
    error is _lib.check's, the half-made context is destroyed, and the same model then trains under a known policy.  PureMF's
    builder has no setter that can fail: the same construction there, a plain step."""
    import storage_cases as SC
    d, K, B = 32, 2, 7
    rng = np.random.Generator(np.random.PCG64(8))
    ids = tuple(torch.from_numpy(rng.integers(1, hi, B)).to(torch.int32).to(DEV) for hi in (SC.N_USERS, SC.M_ITEMS - 2, SC.M_ITEMS - 2))
    try:
        w = SC.configure(pkg, ("fp32", d, K, 0, -1, "propagated"), storage_graph, B)
        ds = pkg.dataloader.Loader(w.config, path=storage_graph)
        pkg.utils.set_seed(SC.MODEL_SEED)
        m = pkg.model.LightGCN(w.config, ds).to(DEV)
        m.train()
        m.config['store_policy'] = 8
        with pytest.raises(pkg._lib.LgcnError, match=r"^lgcn_ctx_set_store_policy failed \(rc=3\)"):
            m.fused_step(*ids)
        assert m._dev is not None and m._dev['ctx'] is None and m.adam_step == 0
        m.config['store_policy'] = 1
        loss = m.fused_step(*ids)
        torch.cuda.synchronize()
        assert m._dev['ctx'] is not None and m.adam_step == 1 and bool(torch.isfinite(loss).all())
        assert _get_policy(pkg, m)[0] == 1
        m.check_device_errors()
        m.config['store_policy'] = 8                       # (PureMF's contexts have no store policy: not looked at)
        pkg.utils.set_seed(SC.MODEL_SEED)
        mf = pkg.model.PureMF(w.config, ds).to(DEV)
        loss = mf.fused_step(*ids)
        torch.cuda.synchronize()
        assert mf._dev['ctx'] is not None and mf.adam_step == 1 and bool(torch.isfinite(loss).all())
        mf.check_device_errors()
    finally:
        pkg.world.configure([])

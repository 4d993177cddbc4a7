"""The DEFAULT fused step with bf16 and fp8 activation storage, launch by launch against float64 (-m gpu): every embedding width
the kernels are built for (bf16 32 / 64 / 128 / 256, fp8 64 / 128 / 256) x K = 1, 2, 3 x the batch-row and the dense last layer,
the hub plan, reg_rows = ego, K = 4 end to end, and lgcn_train_epoch against single steps -- on the graph, table rows and
batches of tests/storage_cases.py, against the restatement of tests/storage_restatement.py, which
tests/test_storage_restatement.py pins to the oracle on the CPU.

CHAIN OF CUSTODY.  A float64 chain that quantises on its own drifts from the GPU wherever an fp32 sum lands across a rounding
boundary (6 % of an fp8 element per flip), so no link is judged on restated tables: every step starts from the state the GPU
held (table and Adam moments read back), and every link is restated in float64 on the numbers the GPU itself stored --
  forward tables   made with the public calls on the model's own Graph object (to_fp8 / .to(bfloat16), spmm / spmm_fp8: the
                   instantiations of launch_spmm<0> the step runs, on the same plan), asserted torch.equal to st['act'][k]
                   wherever the step leaves a forward table intact (the backward ping-pongs over act[1], act[2]: X_2 with K = 2
                   and dense_last, X_1 with K = 1 and dense_last, X_3 with K = 3 / 4).  No call exposes the step's own bf16 / fp8
                   copy of E0; that equality (X_2 = A A Q(E0) bit for bit) is what shows torch's bfloat16 cast to be
                   launch_to_bf16's rounding and to_fp8 to be the step's conversion.
  backward tables  read from st['act'] after the step (K = 2: act[1]; K = 3: act[1] the first launch, act[2] the second).
  last link        Adam's first moment: g_rec = M + (M' - M) / w1, good to 2^-21 (|M| + |M'|) / w1.
Checked per step, each against the bound derived in tests/storage_cases.py: the fp8 copy of E0 (bytes and scales, exactly);
every stored table (element bound; fp8: scale equal on > 99.5 % of the rows, bytes on > 99.9 % of their elements, against the
quantiser restated on the float64 value); the per-triplet log-sigmoid and reg terms of st['terms']; loss_out against the sums
of the GPU's own terms; rows outside the batch's reach (stored backward tables exactly zero, scale 1; g_rec zero to the
recovery slack); the recovered gradient; Adam (test_gpu_gate_shapes._adam_checks, from the GPU's own p, m, v, g); G64 all zero,
check_device_errors() clean, the step counter.  Every test prints the largest share of each bound it used
(profiles/storage_step/README.md).

_judge_step / _run_case / _epoch_vs_steps also serve the cases with layer weights or edge dropout (a seventh field of the case;
tests/test_gpu_storage_features.py, whose docstring says what a feature changes in the judgement); a case without one is judged
exactly as before."""
import numpy as np
import pytest
import torch

import storage_cases as SC
import storage_restatement as S
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)
from test_gpu_fp8 import decode, table_parts
from test_gpu_gate_shapes import W1, _adam_checks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ADJ = {}


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _gpu_model(pkg, case, path):
    ds, m = SC.make_model(pkg, case, path)
    m = m.to(DEV)
    m.train()
    if "adj" not in _ADJ:
        _ADJ["adj"] = ds.getSparseGraphCSR()
        _ADJ["A"] = S.dense_adj(_ADJ["adj"])
    m._state(max_batch=64, need_ctx=True)
    return ds, m


def _parts(pkg, raw, mode, N, d):
    """A stored table as the GPU holds it -> (decoded float64 torch [N, d], bytes in column order or None, scales or None)"""
    if mode != "fp8":
        return raw.float().cpu().to(S.F64), None, None
    b, s = table_parts(pkg, raw, N, d)
    return torch.from_numpy(decode(b, s)).to(S.F64), b.copy(), s.copy()


def _forward_tables(pkg, m, case, E0):
    """Q(E0) and X_1 .. X_fwd_layers with the public calls on the model's own graph -> (e0s raw or None, {k: raw}).  fp32 storage
    has no copy of E0 (layer 1 gathers the table itself); under dropout every layer is Graph.spmm_drop with the step's own
    (keep, seed, step counter)."""
    mode, d, K, dl = case[:4]
    L, g = pkg._lib, m._dev['graph']
    fwd_layers = K if dl else K - 1
    keep = SC.case_keep(case)
    ydt = {"fp8": L.FP8, "bf16": L.BF16, "fp32": L.F32}[mode]
    e0s, out = None, {}
    if K >= 2 and mode != "fp32":
        e0s = g.to_fp8(E0) if mode == "fp8" else E0.to(torch.bfloat16)
    prev = e0s
    for k in range(1, fwd_layers + 1):
        if keep < 1.0:
            out[k] = g.spmm_drop(E0 if prev is None else prev, keep, SC.DROP_SEED, step=m.adam_step, y_dtype=ydt)
        elif prev is None:
            out[k] = g.spmm(E0, ydt)
        else:
            out[k] = g.spmm_fp8(prev, d, L.FP8) if mode == "fp8" else g.spmm(prev)
        prev = out[k]
    return e0s, out


def _step_graphs(pkg, case, m):
    """(forward CSR, backward CSR, their dense float64 forms, layer weights) of the step the model is about to run.  Dropout:
    the mask of the step counter, exported on the model's own graph, IS the host restatement's (tests/dropout_restatement.py)
    and keeps keep +- 0.05 of the entries; A_drop and its explicit transpose are built from the restatement."""
    adj, A = _ADJ["adj"], _ADJ["A"]
    w, keep = SC.case_weights(case), SC.case_keep(case)
    if w is not None:
        assert np.array_equal(m.layer_weights, w)
    if not keep < 1.0:
        return adj, adj, A, A, w
    from dropout_restatement import _keep_host, _rows_of
    g = m._dev['graph']
    assert np.array_equal(g.indices.cpu().numpy(), adj.indices) and np.array_equal(g.indptr.cpu().numpy(), adj.indptr)
    mask = g.dropout_mask(keep, SC.DROP_SEED, m.adam_step).cpu().numpy().astype(bool)
    assert np.array_equal(mask, _keep_host(_rows_of(adj), adj.indices, keep, SC.DROP_SEED, m.adam_step)), "exported mask != host restatement"
    assert abs(mask.mean() - keep) <= 0.05, mask.mean()
    fwd, bwd = SC.case_graphs(adj, case, m.adam_step)
    assert np.array_equal(fwd.data != 0, mask)
    return fwd, bwd, S.dense_adj(fwd), S.dense_adj(bwd), w


def _bwd_buffer(K, k):
    return 1 if K == 2 else 1 + ((K - k) & 1)          # train_bwd_buffer() of csrc/lgcn_train.cpp: the table launch k > 1 writes


def _share(err, bound):
    return float((err / bound).max()) if err.size else 0.0


def _state(m):
    st = m._dev
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in (("table", m._table), ("M", st['adam_m']), ("V", st['adam_v']))}


def _judge_step(pkg, case, m, batch, step_no, tag, end_to_end=False):
    """One fused step from the GPU's own state -> ({link: largest share of its bound}, [(tag, link, share)] beyond 1)."""
    mode, d, K, dl, hub, reg = case[:6]
    ego, N, B = reg == "ego", SC.N_USERS + SC.M_ITEMS, len(batch[0])
    A, st = _ADJ["A"], m._dev
    adj, adj_bwd, A_fwd, A_bwd, w = _step_graphs(pkg, case, m)          # adj: the forward's CSR from here on
    feat = SC.feature(case)[0] is not None
    nbytes = N * d + 4 * N if mode == "fp8" else None
    body = (lambda t: t[:nbytes]) if mode == "fp8" else (lambda t: t)
    before = _state(m)
    E0 = m._table.detach().clone()
    e0s_raw, fwd_raw = _forward_tables(pkg, m, case, E0)
    out = m.fused_step(*(_dev(t) for t in batch)).cpu().numpy().astype(np.float64)
    after = _state(m)
    act = st['act']
    terms = st['terms'].cpu().numpy().astype(np.float64)
    share, cond, used = {}, {}, {}
    # forward tables: the step's own wherever it leaves them intact
    written = {_bwd_buffer(K, k) for k in range(2, K + 1)}
    for k, raw in fwd_raw.items():
        if k not in written:
            assert torch.equal(body(act[k - 1]), body(raw)), (tag, "forward table", k, "differs from the public calls' table")
    custody = {"fwd": {}, "bwd": {}}
    if e0s_raw is not None:
        custody["e0s"], b8, s8 = _parts(pkg, e0s_raw, mode, N, d)
        if mode == "fp8":
            rb, rs, _ = S.fp8_parts(E0.cpu().to(S.F64))
            assert np.array_equal(s8, rs) and np.array_equal(b8, rb), (tag, "fp8(E0)")
    stored = {}
    for k, raw in fwd_raw.items():
        custody["fwd"][k], b8, s8 = _parts(pkg, raw, mode, N, d)
        stored[("fwd", k)] = (custody["fwd"][k], b8, s8)
    if not end_to_end:
        for i in range(K - 1):
            custody["bwd"][i], b8, s8 = _parts(pkg, act[_bwd_buffer(K, K - i) - 1], mode, N, d)
            stored[("bwd", i)] = (custody["bwd"][i], b8, s8)
    if feat:
        r = S.step(A, SC.N_USERS, K, SC.DECAY, before["table"], batch, mode, bool(dl), ego, custody=custody, q_bwd=not end_to_end,
                   weights=w, A_fwd=A_fwd, A_bwd=A_bwd)
        dl_ = SC.step_deltas(adj, r, K, bool(dl), ego, w, adj_bwd)
    else:
        r = S.step(A, SC.N_USERS, K, SC.DECAY, before["table"], batch, mode, bool(dl), ego, custody=custody, q_bwd=not end_to_end)
        dl_ = SC.step_deltas(adj, r, K, bool(dl), ego)
    # stored tables
    for (kind, j), (dec, b8, s8) in stored.items():
        ref = SC.np64(r[kind + "_pre"][j])
        if kind == "fwd":
            delta = SC.spmm_delta(adj, SC.np64(E0.cpu() if (j == 1 and "e0s" not in custody) else (custody["e0s"] if j == 1 else custody["fwd"][j - 1])))
        else:
            delta = dl_["bwd_pre"][j]
        err = np.abs(SC.np64(dec) - ref)
        share[f"{kind}{j}"] = _share(err, SC.stored_bound(ref, delta, mode))
        used[f"{kind}{j}"] = _share(np.maximum(err - SC.half_ulp(ref, mode), 0.0), delta + 1e-37)      # (printed only: how much of delta a stored element needed)
        if mode == "fp8":
            rb, rs, _ = S.fp8_parts(r[kind + "_pre"][j])
            cond[f"{kind}{j}"] = SC.bytes_agree(b8, s8, rb, rs)
        if kind == "bwd":
            outside = ~SC.reach(adj_bwd, r["rows"], j + 1)
            if mode == "fp8":
                assert not b8[outside].any() and (s8[outside] == 1.0).all(), (tag, "stored backward rows outside the reach", j)
            else:
                assert not SC.np64(dec)[outside].any(), (tag, "stored backward rows outside the reach", j)
    # per-triplet terms, loss_out from the GPU's own terms
    share["term"] = _share(np.abs(terms[:B] - SC.np64(r["term"])), dl_["term"])
    share["regterm"] = _share(np.abs(terms[B:2 * B] - SC.np64(r["regterm"])), dl_["regterm"])
    bpr, reg = -terms[:B].sum() / B, 0.5 * terms[B:2 * B].sum() / B
    f_bpr = SC.loss_floor(terms[:B]) / B + SC.U * abs(bpr)
    f_reg = 0.5 * SC.loss_floor(terms[B:2 * B]) / B + SC.U * abs(reg)
    share["loss1"], share["loss2"] = abs(out[1] - bpr) / f_bpr, abs(out[2] - reg) / f_reg
    decay = float(np.float32(SC.DECAY))
    share["loss0"] = abs(out[0] - (out[1] + decay * out[2])) / (2 * SC.U * (abs(out[1]) + decay * abs(out[2])))
    # last link
    Mb, Ma = before["M"], after["M"]
    slack = 2.0 ** -21 * (np.abs(Mb) + np.abs(Ma)) / W1
    g_rec = Mb + (Ma - Mb) / W1
    G = SC.np64(r["g_final"])
    bound = dl_["g_final"] + slack
    info = ""
    if end_to_end:
        chain = dl_["bwd_pre"][0]
        aabs = abs(adj_bwd).astype(np.float64)
        for i in range(1, K):
            chain = (dl_["bwd_pre"][i] if i < K - 1 else dl_["g_final"]) + aabs @ chain
        allow = SC.feature_k4_allowance(adj_bwd, SC.np64(r["G"]), K, w) if feat else SC.k4_allowance(adj, SC.np64(r["G"]), K, mode)
        bound = chain + slack + allow
        info = f" raw {float(np.abs(g_rec - G).max() / np.abs(G).max()):.1e} allowance-share {_share(np.abs(g_rec - G), allow + slack + 1e-300):.2f}"
    share["grad"] = _share(np.abs(g_rec - G), bound + 1e-300)
    outside = ~SC.reach(adj_bwd, r["rows"], K)
    assert not G[outside].any()
    assert (np.abs(g_rec[outside]) <= slack[outside]).all(), (tag, "a row outside the batch's reach has a gradient")
    if B == 1 and K <= 2:
        assert outside.sum() > 0
    share["adam"] = _adam_checks((tag, "table"), before["table"], Mb, before["V"], after["table"], Ma, after["V"], g_rec, slack, step_no, False)
    print(f"[storage_step] {SC.case_id(case)} {tag}: shares " + " ".join(f"{k}={v:.2f}" for k, v in share.items())
          + "".join(f" {k}:rows={a:.4f},bytes={b:.5f}" for k, (a, b) in cond.items()) + " delta-used " + " ".join(f"{k}={v:.2f}" for k, v in used.items()) + f" outside={int(outside.sum())}" + info)
    bad = [(tag, k, v) for k, v in share.items() if not v <= 1.0]
    bad += [(tag, k + " byte agreement", v) for k, v in cond.items() if not (v[0] > 0.995 and v[1] > 0.999)]
    return share, bad


def _run_case(pkg, path, case, end_to_end=False):
    try:
        ds, m = _gpu_model(pkg, case, path)
        assert not m.has_variants and m._dev['dense_last'] == bool(case[3])
        if case[4] > 0:
            assert int(pkg._lib.load().lgcn_ctx_hub_rows(m._dev['ctx'])) == 2          # the hub user and the hub item
        bad, top = [], {}
        for i, batch in enumerate(SC.make_batches(case)):
            share, b = _judge_step(pkg, case, m, batch, i + 1, f"step {i + 1} B={len(batch[0])}", end_to_end)
            bad += b
            for k, v in share.items():
                top[k] = max(top.get(k, 0.0), v)
            m.check_device_errors()
            assert not bool(m._dev['G64'].any()) and m.adam_step == i + 1
        print(f"[storage_step] {SC.case_id(case)} TOP: " + " ".join(f"{k}={v:.2f}" for k, v in top.items()))
        assert not bad, (SC.case_id(case), "beyond the bound (step, link, share of the bound | byte-agreement shares)", bad)
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_step_launch_by_launch(pkg, storage_graph, case):
    """Every link of four steps (64 / 64 / 37 / 1 triplets) on the GPU's own stored numbers (module docstring)."""
    _run_case(pkg, storage_graph, case)


@pytest.mark.parametrize("case", SC.K4_CASES, ids=SC.case_id)
def test_four_layers_end_to_end(pkg, storage_graph, case):
    """K = 4: the first backward table is overwritten before the step ends (the ping-pong's job), so the recovered gradient is
    compared with the float64 gradient on the GPU's own forward tables through the chain WITHOUT backward storage, within
    storage_cases.k4_allowance + the chained fp32 bounds; everything else as in the launch-by-launch test."""
    _run_case(pkg, storage_graph, case, end_to_end=True)


@pytest.mark.parametrize("case", SC.EPOCH_CASES, ids=SC.case_id)
def test_epoch_equals_single_steps_bitwise(pkg, storage_graph, case):
    """lgcn_train_epoch keeps the bf16 / fp8 copy of E0 current in the Adam epilogue (a.Pb / a.Pq), a single-step call converts
    E0 afresh: six steps (5 x 64 + 37 triplets) both ways from fresh models -- losses, table and both Adam moments bit for bit.
    The only observer of the epilogue's shadow rows: a shadow one step stale, or laid out otherwise than to_fp8 lays it out,
    changes layer 1 of the next step."""
    _epoch_vs_steps(pkg, storage_graph, case)


def _epoch_vs_steps(pkg, storage_graph, case):
    try:
        B, T = 64, 5 * 64 + 37
        rng = np.random.Generator(np.random.PCG64(7 + case[1] + case[2]))
        u = rng.integers(0, SC.N_USERS, T); p = rng.integers(0, SC.M_ITEMS, T); n = rng.integers(0, SC.M_ITEMS, T)
        p[:6] = 21; n[6] = p[6]; u[70] = SC.HUB_USER; p[71] = SC.HUB_ITEM; n[72] = SC.ISOLATED_ITEM; u[130] = SC.ZERO_USER; p[131] = SC.SUBNORMAL_ITEM
        ds, a = _gpu_model(pkg, case, storage_graph)
        want_loss = a.fused_epoch(_dev(u), _dev(p), _dev(n), B)
        a.check_device_errors()
        ds, b = _gpu_model(pkg, case, storage_graph)
        first = b._table.detach().clone()
        got = [b.fused_step(_dev(u[t:t + B]), _dev(p[t:t + B]), _dev(n[t:t + B])) for t in range(0, T, B)]
        b.check_device_errors()
        assert a.adam_step == b.adam_step == 6
        assert torch.equal(torch.stack(got), want_loss), (torch.stack(got), want_loss)
        assert torch.equal(a._table, b._table), int((a._table != b._table).sum())
        assert torch.equal(a._dev['adam_m'], b._dev['adam_m']) and torch.equal(a._dev['adam_v'], b._dev['adam_v'])
        assert not bool(a._dev['G64'].any()) and not bool(b._dev['G64'].any())
        assert float((b._table - first).abs().max()) > 1e-3          # (it trained)
    finally:
        pkg.world.configure([])

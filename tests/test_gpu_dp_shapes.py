"""The four data-parallel exchange forms at every width, storage type and shard edge (-m gpu): the cases and batches of
tests/dp_cases.py on the 300 x 600 graph and the hand-set rows of tests/storage_cases.py; tests/test_dp_shapes_host.py pins on the
CPU what makes a case worth running (ragged and empty shards, row ids shared between ranks, hub rows on different ranks, shards
that are no multiple of k_scatter's slots per workgroup, B > 64 and > 128 for the reduction wave).

(a) test_row_exchange_steps_bitwise   W models, part 1 on each rank's own, the blocks concatenated in rank order, part 2 on every
    model, dp_local 0 and 1 -- after EVERY step every rank equals the single-GPU model stepped with fused_step bit for bit: table,
    both Adam moments (they show a gradient scaled by a constant, which Adam's normalisation nearly hides in the table), the three
    loss floats, both bitmaps, G64 all zero.  reg_rows = ego: a second identical epoch of steps (a stale slot count changes it).
(b) test_c_loop_bitwise   lgcn_train_epoch_dp through the loopback communicator, forms rows / dense / row_sharded, three epochs on
    the same models: T = the five batches concatenated at B = 300 (a short last batch), then the 5-triplet and the 1-triplet batch
    as epochs of their own.  The reference is fused_epoch, which folds k_g32 where it can while the data-parallel loop never does:
    the equality is a check of the fold at these shapes too.  Table, both moments and the per-step losses, bit for bit, after each
    epoch; under row sharding Adam's state of a row lives on its owner only, so there every moment row is compared on
    the rank that owns it and must be untouched zeros on the others.  The row-sharded hub cases run on dp_cases.rotate_item_ranges (rank 0
    owns the hub user, rank 1 the hub item: parallel.row_ranges itself gives both to rank 0 on this graph); a row-sharded context's
    plan holds the owned rows only, its hub plan every hub row (lgcn_ctx_create builds it from the graph's CSR arrays).
(c) test_column_shards_step_by_step   rank models from parallel.column_shard (the hand-set rows copied in), ONE step per call of
    lgcn_train_epoch_dp in mode 3, P / M / V of every rank read before and after and concatenated by columns; each step judged the
    way tests/test_gpu_storage_step.py judges an end-to-end step: g_rec = M + (M' - M) / w1 against the float64 gradient of
    storage_restatement.step at the concatenated table the GPU held, on the GPU's own forward tables (public calls on each rank's
    graph, decoded and concatenated; equal to the step's own where the step leaves them), within storage_cases.step_deltas' chain
    + the 2^-21 (|M| + |M'|) / w1 read-back + the storage allowance of the backward tables (gate_cases.storage_allowance for bf16,
    storage_cases.k4_allowance's fp8 form; none for fp32); V', P' and the rows outside the batch's reach by _adam_checks; the
    per-triplet terms and the three loss floats by that file's bounds.

    THE SCORE UNDER COLUMN SHARDS.  Read from triplet_loss_regs (cols_phase 1), lb_all_reduce / k_sum_ranks and k_cols_finish: a
    rank's partial dot product is CPL products added serially per lane and an xor-shuffle tree over min(d / W, 64) lanes; the
    all-reduce adds the W partials in rank order, s = src[0]; s += src[q]; x = ps - ns is formed once from the complete sums.  A
    product therefore passes through (CPL - 1) + log2(LPT) + (W - 1) <= d - 1 additions: one of the orders of a d-term fp32 dot
    product, which storage_cases' score bound (d + 2) u sum |u_j p_j| holds for in ANY order.  The reg term is 3 d products; a
    product passes through (CPL - 1) + 2 (ru + rp + rn per lane) + log2(LPT) + (W - 1) additions, at most d / W + W + 1 <= d + 2
    for every (W, d) here, inside the (d + 3) u of the single-GPU bound.  Nothing else is rounded: colsum and the slot rows travel
    as fp32 and x, the loss terms and the gradient rows are computed after the all-reduce exactly as on one GPU.  So no term is
    added to the bounds.  fp8 storage under column shards is ACCEPTED by the library (no entry point refuses it; a rank's context
    is an ordinary fp8 context of width d / W >= 64, its row scale the rank's own): the two fp8 cases are judged under the fp8
    bounds, the stored tables rank by rank (each rank's row maximum), the allowance with the full row's (which is no smaller).
(d) test_refusals   dropout, layer weights or a non-BPR loss on the context: every data-parallel entry point returns 3, names
    itself and the feature, and moves nothing.
Every case of (c) prints the largest share of each bound it used (profiles/dp_shapes/README.md)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import dp_cases as D
import storage_cases as SC
import storage_restatement as S
import test_gpu_storage_step as TS
from storage_cases import storage_graph  # noqa: F401  (fixture: the graph, written once per session)
from test_gpu_gate_shapes import W1, _adam_checks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ADJ = {}


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _models(pkg, case, path, n):
    """n fresh models of a case on the GPU (storage_cases.make_model, the hand-set rows in) and the dataset; the caller resets
    world's config."""
    ds, first = SC.make_model(pkg, D.storage_case(case), path, batch=D.MAX_BATCH)
    out = [first]
    for _ in range(n - 1):
        pkg.utils.set_seed(SC.MODEL_SEED)
        m = pkg.model.LightGCN(pkg.world.config, ds)
        SC.set_rows(m._table)
        out.append(m)
    assert all(torch.equal(m._table, first._table) for m in out[1:])
    if "adj" not in _ADJ:
        _ADJ["adj"] = ds.getSparseGraphCSR()
        _ADJ["A"] = S.dense_adj(_ADJ["adj"])
    out = [m.to(DEV) for m in out]
    for m in out:
        m.train()
    return ds, out


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _assert_rank_equals(ref, m, what, bitmaps=True, owned=None):
    """owned (row-sharded ranks): Adam runs on the rows a rank owns and only the table rows are exchanged, so a rank's moments are
    the single-GPU model's on its OWN rows -- every row is compared on its owner -- and untouched zeros everywhere else."""
    for key, a, b in (("table", ref._table, m._table), ("adam_m", ref._dev['adam_m'], m._dev['adam_m']), ("adam_v", ref._dev['adam_v'], m._dev['adam_v'])):
        if owned is not None and key != "table":
            other = torch.ones(b.shape[0], dtype=torch.bool, device=b.device)
            other[owned] = False
            assert not bool(_bits(b[other]).any()), (what, key, "a row-sharded rank wrote moments of rows it does not own")
            a, b = a[owned], b[owned]
        assert _same(a, b), (what, key, int((_bits(a) != _bits(b)).sum()), float((a - b).abs().max()))
    assert not bool(m._dev['G64'].any()), (what, "G64")
    if bitmaps:
        assert torch.equal(ref._dev['bitmap'], m._dev['bitmap']), (what, "bitmaps")
    assert m.adam_step == ref.adam_step, (what, "step counter")


def _run_ranks(lib, world, fn):
    """The thread pattern of test_gpu_parity.test_dp_epoch_c_loop_world_gt_1_loopback: fn(rank) -> rc on W threads."""
    rcs, errs = [None] * world, [None] * world

    def rank_main(r):
        rcs[r] = fn(r)
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


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.STEP_CASES, ids=D.case_id)
def test_row_exchange_steps_bitwise(pkg, storage_graph, case):
    mode, d, K, dl, hub, reg, world, form, cap = case
    L, lib, par = pkg._lib, pkg._lib.load(), pkg.parallel
    try:
        ds, models = _models(pkg, case, storage_graph, world + 1)
        ref, ranks = models[0], models[1:]
        first = ref._table.detach().clone()
        ref._state(max_batch=cap, need_ctx=True)
        states = [m._state(max_batch=cap, need_ctx=True, dp_world=world) for m in ranks]
        for m in models:
            assert not m.has_variants and m._dev['dense_last'] == bool(dl)
            assert int(lib.lgcn_ctx_hub_rows(m._dev['ctx'])) == (2 if hub > 0 else 0)
        for st in states:
            L.check(lib.lgcn_ctx_set_dp_local(st['ctx'], 1 if form == "rows1" else 0), "set_dp_local")
        stream = L.current_stream()
        batches = D.make_batches(case)
        step_no = 0
        for epoch in range(2 if reg == "ego" else 1):
            for (u, p, n) in batches:
                u, p, n = (_dev(x) for x in (u, p, n))
                B = int(u.numel())
                step_no += 1
                what = (D.case_id(case), "epoch", epoch, "step", step_no, "B", B)
                want = ref.fused_step(u, p, n)
                nblk = par.block_numel(B, world, d)
                blocks = []
                for r, st in enumerate(states):
                    assert int(lib.lgcn_dp_block_floats(st['ctx'], B, world)) == nblk, what
                    L.check(lib.lgcn_train_step_dp_part1(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, r, stream), "part1")
                    blocks.append(st['contrib'][:nblk].clone())          # (an empty rank's block is whatever it held: nobody reads it)
                gathered = torch.cat(blocks)
                for r, (m, st) in enumerate(zip(ranks, states)):
                    out = torch.empty(3, device=DEV)
                    L.check(lib.lgcn_train_step_dp_part2(st['ctx'], L.tp(u), L.tp(p), L.tp(n), B, world, L.tp(gathered), L.tp(out), stream), "part2")
                    assert _same(out, want), (what, "rank", r, "loss", out.tolist(), want.tolist())
                    _assert_rank_equals(ref, m, what + ("rank", r))
                assert not bool(ref._dev['G64'].any()) and ref.adam_step == step_no
        for m in models:
            m.check_device_errors()
        assert float((ref._table - first).abs().max()) > 1e-4          # (it trained)
    finally:
        pkg.world.configure([])


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.LOOP_CASES, ids=D.case_id)
def test_c_loop_bitwise(pkg, storage_graph, case):
    mode, d, K, dl, hub, reg, world, form, B = case
    L, lib, par = pkg._lib, pkg._lib.load(), pkg.parallel
    comms = None
    try:
        ds, models = _models(pkg, case, storage_graph, world + 1)
        ref, ranks = models[0], models[1:]
        first = ref._table.detach().clone()
        batches = D.make_batches(case)
        epochs = [tuple(np.concatenate([b[i] for b in batches]) for i in range(3)), batches[3], batches[4]]
        assert [len(e[0]) for e in epochs] == [408, 5, 1]
        ranges = None
        if form == "row_sharded":
            ranges = par.row_ranges(ranks[0]._adj.indptr, ranks[0].n_users, world)
            if hub > 0:
                ranges = D.rotate_item_ranges(ranges)
                own = [set(par.owned_rows(ranges, r).tolist()) for r in range(world)]
                assert SC.HUB_USER in own[0] and SC.N_USERS + SC.HUB_ITEM in own[1]
        ref._state(max_batch=B, need_ctx=True)
        states = [m._state(max_batch=B, need_ctx=True, dp_world=world, row_subset=par.owned_rows(ranges, r) if ranges is not None else None)
                  for r, m in enumerate(ranks)]
        for m in models:
            assert m._dev['dense_last'] == bool(dl) and int(lib.lgcn_ctx_hub_rows(m._dev['ctx'])) == (2 if hub > 0 else 0)
        comms = (C.c_void_p * world)()
        L.check(lib.lgcn_dp_init_loopback(world, comms), "loopback")
        code = {"rows1": 0, "dense": 1, "row_sharded": 2}[form]
        streams = [torch.cuda.Stream() for _ in range(world)]
        gathered = [torch.empty(world * par.block_numel(B, world, d), device=DEV) for _ in range(world)]
        rr = np.ascontiguousarray(ranges, np.int64) if ranges is not None else None
        owned = [_dev(par.owned_rows(ranges, r), torch.int64) for r in range(world)] if ranges is not None else None
        for e, (u, p, n) in enumerate(epochs):
            U, P, Nn = (_dev(x) for x in (u, p, n))
            T = int(U.numel())
            steps = (T + B - 1) // B
            want = ref.fused_epoch(U, P, Nn, B)
            losses = [torch.empty(steps, 3, device=DEV) for _ in range(world)]
            torch.cuda.synchronize()
            _run_ranks(lib, world, lambda r: lib.lgcn_train_epoch_dp(
                states[r]['ctx'], comms[r], L.tp(U), L.tp(P), L.tp(Nn), T, B, code, L.npp(rr) if rr is not None else None,
                L.tp(gathered[r]), L.tp(losses[r]), C.c_void_p(streams[r].cuda_stream)))
            for r, m in enumerate(ranks):
                what = (D.case_id(case), "epoch", e, "T", T, "rank", r)
                assert _same(losses[r], want), (what, "losses", losses[r].tolist(), want.tolist())
                _assert_rank_equals(ref, m, what, bitmaps=False, owned=owned[r] if ranges is not None else None)
        for m in models:
            m.check_device_errors()
        assert ref.adam_step == 4 and float((ref._table - first).abs().max()) > 1e-4
    finally:
        if comms is not None:
            for r in range(world):
                if comms[r]:
                    lib.lgcn_dp_destroy(comms[r])
        pkg.world.configure([])


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def _cols_models(pkg, case, path):
    """The rank models of a column-sharded case: parallel.column_shard's, with the case's own full table (hand-set rows in) copied
    into the slices -> (rank models, [(lo, hi)], full CPU table)."""
    mode, d, K, dl, hub, reg, world = case[:7]
    par = pkg.parallel
    ds, full = SC.make_model(pkg, D.storage_case(case), path, batch=D.MAX_BATCH)
    if "adj" not in _ADJ:
        _ADJ["adj"] = ds.getSparseGraphCSR()
        _ADJ["A"] = S.dense_adj(_ADJ["adj"])
    table = full._table.detach().clone()
    ranks, cuts = [], []
    for r in range(world):
        pkg.utils.set_seed(SC.MODEL_SEED)
        m = par.column_shard(pkg.model.LightGCN, pkg.world.config, ds, world, r, DEV)
        lo, hi = par.column_range(d, world, r)
        assert m.latent_dim == d // world == hi - lo and m.col_range == (lo, hi, d)
        with torch.no_grad():
            m._table.copy_(table[:, lo:hi].to(DEV))
        m.train()
        ranks.append(m)
        cuts.append((lo, hi))
    return ranks, cuts, table


def _cat(ranks, get):
    return torch.cat([get(m).detach().float() for m in ranks], dim=1).cpu().numpy().astype(np.float64)


def _cols_state(ranks):
    return {"table": _cat(ranks, lambda m: m._table), "M": _cat(ranks, lambda m: m._dev['adam_m']), "V": _cat(ranks, lambda m: m._dev['adam_v'])}


def _judge_cols_step(pkg, case, ranks, cuts, run_step, batch, step_no, tag):
    """One column-sharded step from the GPU's own state -> {link: largest share of its bound}."""
    mode, d, K, dl, hub, reg, world = case[:7]
    ego, N, B, w = reg == "ego", SC.N_USERS + SC.M_ITEMS, len(batch[0]), d // world
    adj, A = _ADJ["adj"], _ADJ["A"]
    rank_case = (mode, w, K, dl, hub, reg)
    nbytes = N * w + 4 * N
    body = (lambda t: t[:nbytes]) if mode == "fp8" else (lambda t: t)
    before = _cols_state(ranks)
    # the forward tables, rank by rank with the public calls on the rank's own graph
    per_rank = [TS._forward_tables(pkg, m, rank_case, m._table.detach().clone()) for m in ranks]
    out = run_step(batch)                                                   # [W, 3] float64
    after = _cols_state(ranks)
    assert all(np.array_equal(out[r].view(np.uint64), out[0].view(np.uint64)) for r in range(world)), (tag, "the ranks' losses differ", out)
    out = out[0]
    written = {TS._bwd_buffer(K, k) for k in range(2, K + 1)}
    for m, (e0s_raw, fwd_raw) in zip(ranks, per_rank):
        for k, raw in fwd_raw.items():
            if k not in written:
                assert torch.equal(body(m._dev['act'][k - 1]), body(raw)), (tag, "forward table", k, "differs from the public calls' table")
    dec = lambda raw: TS._parts(pkg, raw, mode, N, w)[0]      # noqa: E731
    custody = {"fwd": {}, "bwd": {}}
    if per_rank[0][0] is not None:
        custody["e0s"] = torch.cat([dec(e0s) for e0s, _ in per_rank], dim=1)
    for k in per_rank[0][1]:
        custody["fwd"][k] = torch.cat([dec(f[k]) for _, f in per_rank], dim=1)
    r = S.step(A, SC.N_USERS, K, SC.DECAY, before["table"], batch, mode, bool(dl), ego, custody=custody, q_bwd=False)
    dl_ = SC.step_deltas(adj, r, K, bool(dl), ego)
    share = {}
    # stored forward tables, judged rank by rank (fp8: the row scale is the rank's own)
    for k, got in custody["fwd"].items():
        src = before["table"] if (k == 1 and "e0s" not in custody) else SC.np64(custody["e0s"] if k == 1 else custody["fwd"][k - 1])
        ref, delta = SC.np64(r["fwd_pre"][k]), SC.spmm_delta(adj, src)
        err = np.abs(SC.np64(got) - ref)
        share[f"fwd{k}"] = max(TS._share(err[:, lo:hi], SC.stored_bound(ref[:, lo:hi], delta[:, lo:hi], mode)) for lo, hi in cuts)
    # per-triplet terms (identical on every rank: they come from the all-reduced sums), loss_out from the GPU's own terms
    terms = ranks[0]._dev['terms'][:2 * B].cpu().numpy().astype(np.float64)
    for m in ranks[1:]:
        assert _same(m._dev['terms'][:2 * B], ranks[0]._dev['terms'][:2 * B]), (tag, "the ranks' loss terms differ")
    share["term"] = TS._share(np.abs(terms[:B] - SC.np64(r["term"])), dl_["term"])
    share["regterm"] = TS._share(np.abs(terms[B:] - SC.np64(r["regterm"])), dl_["regterm"])
    bpr, regl = -terms[:B].sum() / B, 0.5 * terms[B:].sum() / B
    f_bpr = SC.loss_floor(terms[:B]) / B + SC.U * abs(bpr)
    f_reg = 0.5 * SC.loss_floor(terms[B:]) / B + SC.U * abs(regl)
    share["loss1"], share["loss2"] = abs(out[1] - bpr) / f_bpr, abs(out[2] - regl) / f_reg
    decay = float(np.float32(SC.DECAY))
    share["loss0"] = abs(out[0] - (out[1] + decay * out[2])) / (2 * SC.U * (abs(out[1]) + decay * abs(out[2])))
    # the gradient, end to end
    Mb, Ma = before["M"], after["M"]
    slack = 2.0 ** -21 * (np.abs(Mb) + np.abs(Ma)) / W1
    g_rec = Mb + (Ma - Mb) / W1
    G = SC.np64(r["g_final"])
    if K == 1:
        chain = dl_["g_final"]
    else:
        chain = dl_["bwd_pre"][0]
        aabs = abs(adj).astype(np.float64)
        for i in range(1, K):
            chain = (dl_["bwd_pre"][i] if i < K - 1 else dl_["g_final"]) + aabs @ chain
    allow = 0.0 if (mode == "fp32" or K == 1) else SC.k4_allowance(adj, SC.np64(r["G"]), K, mode)
    share["grad"] = TS._share(np.abs(g_rec - G), chain + slack + allow + 1e-300)
    share["grad_fp32_part"] = TS._share(np.abs(g_rec - G), chain + slack + 1e-300)          # (printed only: > 1 where the allowance is needed)
    outside = ~SC.reach(adj, r["rows"], K)
    assert not G[outside].any()
    assert (np.abs(g_rec[outside]) <= slack[outside]).all(), (tag, "a row outside the batch's reach has a gradient")
    if B == 1 and K <= 2:
        assert outside.sum() > 0
    share["adam"] = _adam_checks((tag, "table"), before["table"], Mb, before["V"], after["table"], Ma, after["V"], g_rec, slack, step_no, False)
    print(f"[dp_shapes] {D.case_id(case)} {tag}: shares " + " ".join(f"{k}={v:.2f}" for k, v in share.items()) + f" outside={int(outside.sum())}")
    return share


def _run_cols_case(pkg, path, case):
    mode, d, K, dl, hub, reg, world, form, cap = case
    L, lib = pkg._lib, pkg._lib.load()
    comms = None
    try:
        ranks, cuts, table0 = _cols_models(pkg, case, path)
        states = [m._state(max_batch=cap, need_ctx=True, dp_world=1) for m in ranks]
        for m in ranks:
            assert m._dev['dense_last'] == bool(dl) and int(lib.lgcn_ctx_hub_rows(m._dev['ctx'])) == (2 if hub > 0 else 0)
        comms = (C.c_void_p * world)()
        L.check(lib.lgcn_dp_init_loopback(world, comms), "loopback")
        streams = [torch.cuda.Stream() for _ in range(world)]

        def run_step(batch):
            U, P, Nn = (_dev(x) for x in batch)
            B = int(U.numel())
            losses = [torch.empty(1, 3, device=DEV) for _ in range(world)]
            torch.cuda.synchronize()
            _run_ranks(lib, world, lambda r: lib.lgcn_train_epoch_dp(states[r]['ctx'], comms[r], L.tp(U), L.tp(P), L.tp(Nn), B, B, 3, None, None,
                                                                     L.tp(losses[r]), C.c_void_p(streams[r].cuda_stream)))
            return np.stack([l[0].cpu().numpy().astype(np.float64) for l in losses])
        top = {}
        for i, batch in enumerate(D.make_batches(case)):
            share = _judge_cols_step(pkg, case, ranks, cuts, run_step, batch, i + 1, f"step {i + 1} B={len(batch[0])}")
            for k, v in share.items():
                top[k] = max(top.get(k, 0.0), v)
            for m in ranks:
                m.check_device_errors()
                assert not bool(m._dev['G64'].any()) and m.adam_step == i + 1
        print(f"[dp_shapes] {D.case_id(case)} TOP: " + " ".join(f"{k}={v:.2f}" for k, v in top.items()))
        bad = {k: v for k, v in top.items() if k != "grad_fp32_part" and not v <= 1.0}
        assert not bad, (D.case_id(case), "beyond the bound (link: largest share)", bad)
        got = torch.cat([m._table.detach() for m in ranks], dim=1).cpu()
        assert float((got - table0).abs().max()) > 1e-4                 # (it trained)
    finally:
        if comms is not None:
            for r in range(world):
                if comms[r]:
                    lib.lgcn_dp_destroy(comms[r])
        pkg.world.configure([])


@pytest.mark.parametrize("case", D.COLS_CASES, ids=D.case_id)
def test_column_shards_step_by_step(pkg, storage_graph, case):
    _run_cols_case(pkg, storage_graph, case)


@pytest.mark.parametrize("case", D.COLS_FP8_CASES, ids=D.case_id)
def test_column_shards_fp8_accepted(pkg, storage_graph, case):
    """fp8 storage under column shards: no entry point of csrc/lgcn_train_dp.cpp and nothing in model.py refuses it -- a rank is an
    ordinary fp8 context of width 64 / 128 -- so it is judged, under the fp8 bounds (module docstring)."""
    _run_cols_case(pkg, storage_graph, case)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
def _set_dropout(L, lib, ctx):
    L.check(lib.lgcn_ctx_set_dropout(ctx, 0.6, SC.DROP_SEED), "set_dropout")


def _set_weights(L, lib, ctx):
    from test_gpu_layer_weights import weight_set
    w = np.ascontiguousarray(weight_set("literal", 2), np.float32)
    L.check(lib.lgcn_ctx_set_layer_weights(ctx, L.npp(w), 3), "set_layer_weights")


def _set_loss(L, lib, ctx):
    L.check(lib.lgcn_ctx_set_loss(ctx, L.LOSS_SOFTMAX, 0.5), "set_loss")


@pytest.mark.parametrize("feature,setter,names", [("dropout", _set_dropout, b"edge dropout (lgcn_ctx_set_dropout)"),
                                                   ("layer_weights", _set_weights, b"layer weights (lgcn_ctx_set_layer_weights)"),
                                                   ("loss", _set_loss, b"sampled-softmax loss (lgcn_ctx_set_loss)")])
def test_refusals(pkg, storage_graph, feature, setter, names):
    """One context per feature at d = 64, K = 2 (dense_last = 1: the softmax loss asks for it), stepped once so that the moments,
    the flagged bitmap and the step counter are not trivial; then every data-parallel entry point must return 3, name itself and
    the feature, and leave table, moments, G64, bitmaps and the step counter as they were."""
    case = D._case("fp32", 64, 2, 1, 2, "rows0")
    L, lib = pkg._lib, pkg._lib.load()
    comms = None
    try:
        ds, (m,) = _models(pkg, case, storage_graph, 1)
        st = m._state(max_batch=D.MAX_BATCH, need_ctx=True, dp_world=2)
        u, p, n = (_dev(x) for x in D.make_batches(case)[2])
        B = int(u.numel())
        m.fused_step(u, p, n)
        assert m._dev is st and m._dev['ctx'] == st['ctx']
        setter(L, lib, st['ctx'])
        keys = ('adam_m', 'adam_v', 'G64', 'bitmap')
        held = {k: st[k].clone() for k in keys}
        held['table'] = m._table.detach().clone()
        assert bool(held['adam_m'].any()) and bool(held['bitmap'].any()) and int(lib.lgcn_ctx_get_step(st['ctx'])) == 1
        comms = (C.c_void_p * 1)()
        L.check(lib.lgcn_dp_init_loopback(1, comms), "loopback")
        stream = L.current_stream()
        ids = (L.tp(u), L.tp(p), L.tp(n))
        out, gathered, ptr = torch.zeros(3, device=DEV), torch.zeros(2 * pkg.parallel.block_numel(B, 2, 64), device=DEV), C.c_void_p()
        rr = np.ascontiguousarray(pkg.parallel.row_ranges(m._adj.indptr, m.n_users, 2), np.int64)
        calls = [("lgcn_train_step_dp_part1", lambda: lib.lgcn_train_step_dp_part1(st['ctx'], *ids, B, 2, 0, stream)),
                 ("lgcn_train_step_dp_dense_part1", lambda: lib.lgcn_train_step_dp_dense_part1(st['ctx'], *ids, B, 2, 1, stream)),
                 ("lgcn_train_step_dp_part2", lambda: lib.lgcn_train_step_dp_part2(st['ctx'], *ids, B, 2, L.tp(gathered), L.tp(out), stream)),
                 ("lgcn_train_step_cols_part1", lambda: lib.lgcn_train_step_cols_part1(st['ctx'], *ids, B, C.byref(ptr), stream)),
                 ("lgcn_train_step_cols_part2", lambda: lib.lgcn_train_step_cols_part2(st['ctx'], *ids, B, L.tp(out), stream))]
        calls += [("lgcn_rs_phase", (lambda ph, k: lambda: lib.lgcn_rs_phase(st['ctx'], ph, k, *ids, B, 2, 0, L.tp(gathered), L.tp(out), stream))(ph, k))
                  for ph, k in ((0, 1), (1, 0), (2, 0), (3, 2), (4, 0))]
        calls += [("lgcn_train_epoch_dp", (lambda code: lambda: lib.lgcn_train_epoch_dp(st['ctx'], comms[0], *ids, B, B, code, L.npp(rr), L.tp(gathered),
                                                                                        L.tp(out), stream))(code)) for code in (0, 1, 2, 3)]
        for name, call in calls:
            rc = call()
            msg = lib.lgcn_last_error() or b""
            assert rc == 3, (feature, name, rc, msg)
            assert name.encode() in msg and names in msg, (feature, name, msg)
            torch.cuda.synchronize()
            assert all(torch.equal(st[k], held[k]) for k in keys) and _same(m._table, held['table']), (feature, name, "something moved")
            assert int(lib.lgcn_ctx_get_step(st['ctx'])) == 1 and not bool(out.any())
        m.check_device_errors()
    finally:
        if comms is not None and comms[0]:
            lib.lgcn_dp_destroy(comms[0])
        pkg.world.configure([])

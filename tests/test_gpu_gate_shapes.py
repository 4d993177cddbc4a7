"""The gated / smoothed fused step (k_mean_layers, the item-item SpMMs, k_triplet_gate<32 / 64 / 128> or the K = 0 form of
k_triplet_dense, k_gate_adam, k_flag_range, k_gate_rank_total) beyond the d = 64 fixture of tests/golden/tiny: every embedding
width the gate kernel is built for, hidden widths that are no power of two / are 1 / are 64 for both MLPs, temperatures other
than 1, an entropy coefficient large enough to see, saturated gates, two bitmap geometries, sparse item-item matrices with
empty rows and unnamed items -- against the float64 restatement of tests/gate_restatement.py, which
tests/test_gate_restatement.py pins to the reference's fixtures.  Shapes, seeds and the conditions on the inputs are those of
tests/test_gate_restatement.py (CASES; checked there on the CPU, asserted here again at the GPU's own states).

Every step is judged from the state the GPU itself held before it (table, MLP parameters and all Adam moments read back before
and after), so there is no trajectory to drift:
  (a) loss_out[1], [2], [0] against bpr - coeff * entropy, reg and their total at the pre-step parameters;
  (b) the step's reduced MLP gradient (gate_grad, named_parameters order) against the float64 gradient of each tensor;
  (c) the table gradient, recovered as g_rec = M + (M' - M) / w1 (w1 = float32(0.1)), against the float64 one over all N rows;
      the recovery itself is good to 2^-21 (|M| + |M'|) / w1 (two fp32 roundings in M', as in test_gpu_mf.py), which is added
      element by element.  Without smoothing, rows outside the batch's K-hop reach must be zero to that recovery error (exactly
      zero where M = 0); with smoothing every item row is live;
  (d) Adam, from the GPU's own p, m, v and its own gradient, in float64: v' within 2^-22 v' + 2 (1 - beta2) |g| slack + 2^-126
      (two roundings; the recovery's slack for the table, none for the MLPs whose gradient is read directly), the MLP's m'
      within 2^-23 (|m| + |g|) (three roundings of terms no larger than |m| + |g|), p' within 4 * 2^-24 (|p| + 4 lr) of
      p - step_size m' / (sqrt(v') / bc2_sqrt + eps)  from the GPU's m', v' (test_gpu_mf.py's bound for the same statement);
  (e) check_device_errors() clean, G64 all zero, the step counter.
Tolerances of (a) - (c), step by step: e32 = the fp32 twin's distance from float64 in THIS step (the same restatement run in
float32; for a gradient max |.| over the tensor as a fraction of the float64 tensor's max); the GPU may be 8 e32 away (it sums
2d-term dot products in one chain, reduces across lanes and rounds each contribution once to 2^-50 fixed point: reorderings of
the twin's fp32 work), and never more than the project's tolerance for the quantity on this path (2e-6 loss / reg, 5e-4 of the
tensor's max for gradients).  A quantity that is ONE fp32 number has a floor under 8 e32, derived in gate_cases.step_bounds:
(1 + ceil(log2 n)) 2^-24 sum |terms| for a sum of n fp32 terms (B triplets for loss / reg / total, 2B slots for a one-element gradient).  bf16 activation
storage adds (K - 1) 2^-8 (M |G|)_i under every element of the table gradient (gate_cases.storage_allowance: one bf16 rounding
errs by 2^-8; tests/test_gate_restatement.py holds it against an exact backward chain with bf16 tables).  Every step prints
e32 / the GPU's distance / their ratio / the share of the bound used (profiles/gate_shapes/README.md)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

import gate_restatement as R
from gate_cases import (BAD_ID_CASES, BAD_IDS, CASES, LR, bad_id_batch, case_id, make_batches, make_model, mean_abs_prop, model_inputs,
                        references, step_bounds, storage_allowance)
from gate_cases import graph_dirs  # noqa: F401  (fixture: both graphs, written once per session)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B1, B2, EPS = 0.9, 0.999, 1e-8
W1 = float(np.float32(1.0 - B1))
F_B2, F_OMB2, F_EPS = float(np.float32(B2)), float(np.float32(1.0 - B2)), float(np.float32(EPS))
U32, TINY32 = 2.0 ** -24, 2.0 ** -126


def _dev(a, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _gpu_model(pkg, case, path, fused=1, batch=64):
    ds, m = make_model(pkg, case, path, fused, batch)
    m = m.to(DEV)
    m.train()
    return ds, m


def _shapes(case):
    d, _, Hp, Hg = case[:4]
    return [(Hp, 1), (Hp,), (d, Hp), (d,), (Hg, 2 * d), (Hg,), (1, Hg), (1,)]


def _unpack(flat, case):
    out, off = [], 0
    for s in _shapes(case):
        n = int(np.prod(s))
        out.append(flat[off:off + n].reshape(s).copy())
        off += n
    assert off == flat.size
    return out


def _state(m, gate):
    st = m._dev
    s = {"table": m._table, "M": st['adam_m'], "V": st['adam_v']}
    if gate:
        s.update(mlp=m._gate_flat, gm=st['gate_m'], gv=st['gate_v'])
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in s.items()}


def _adam_checks(what, p, m, v, p2, m2, v2, g, slack, step_no, m_exact):
    """(d) of the module docstring; returns the largest share of the parameter bound used."""
    v_ref = F_B2 * v + F_OMB2 * g * g
    tol_v = 2.0 ** -22 * v2 + 2.0 * F_OMB2 * np.abs(g) * slack + TINY32
    assert (np.abs(v2 - v_ref) <= tol_v).all(), (what, "v", float((np.abs(v2 - v_ref) / tol_v).max()))
    if m_exact:
        m_ref = m + W1 * (g - m)
        tol_m = 2.0 ** -23 * (np.abs(m) + np.abs(g)) + TINY32
        assert (np.abs(m2 - m_ref) <= tol_m).all(), (what, "m", float((np.abs(m2 - m_ref) / tol_m).max()))
    bc1, bc2 = 1.0 - B1 ** step_no, 1.0 - B2 ** step_no
    step_size, bc2_sqrt = float(np.float32(LR / bc1)), float(np.float32(np.sqrt(bc2)))
    p_ref = p - step_size * m2 / (np.sqrt(v2) / bc2_sqrt + F_EPS)
    tol_p = 4.0 * U32 * (np.abs(p) + 4.0 * LR)
    share = float((np.abs(p2 - p_ref) / tol_p).max())
    assert share <= 1.0, (what, "p", share)
    return share


def _judge_step(case, inp, m, batch, step_no, tag, scale=1.0, ref_batch=None):
    """One fused step from the GPU's own state -> the quantities beyond their bound [(tag, quantity, GPU's distance, bound)].
    scale / ref_batch: the bad-id test compares with the restatement of the sound triplets, scaled."""
    gate, K, n_users = case[6], case[1], inp["n_users"]
    before = _state(m, gate)
    out = m.fused_step(*(_dev(t) for t in batch)).cpu().numpy().astype(np.float64)
    after = _state(m, gate)
    mlp_b = _unpack(before["mlp"], case) if gate else None
    r64, e32, info = references(case, inp, before["table"], mlp_b, ref_batch or batch, step_no)
    what = (case_id(case), step_no, len(batch[0]))
    dist = {"loss": abs(out[1] - scale * r64["loss"]), "reg": abs(out[2] - scale * r64["reg"]), "total": abs(out[0] - scale * r64["total"])}
    # (c)
    Mb, Ma = before["M"], after["M"]
    slack = 2.0 ** -21 * (np.abs(Mb) + np.abs(Ma)) / W1
    g_rec = Mb + (Ma - Mb) / W1
    G = scale * r64["grad_table"]
    allow = slack
    if inp["act_bf16"]:
        allow = allow + storage_allowance(inp["adj"], scale * r64["grad_final"], K)
        info["table_raw"] = f"{float(np.abs(g_rec - G).max() / np.abs(G).max()):.1e}"
    dist["table"] = float(np.maximum(np.abs(g_rec - G) - allow, 0.0).max() / np.abs(G).max())
    if inp["i2i"] is None:
        named = np.zeros((g_rec.shape[0], 1))
        named[np.asarray((ref_batch or batch)[0])] = 1.0
        named[n_users + np.concatenate([(ref_batch or batch)[1], (ref_batch or batch)[2]])] = 1.0
        outside = mean_abs_prop(inp["adj"], named, K)[:, 0] == 0.0
        assert (G[outside] == 0.0).all()
        assert (np.abs(g_rec[outside]) <= slack[outside]).all(), (what, "a row outside the batch's reach has a gradient")
        if len(batch[0]) == 1:
            assert outside.sum() > 0
        info["outside"] = int(outside.sum())
    else:
        assert (np.abs(G[n_users:]).max(axis=1) > 0).mean() > 0.9          # smoothing: the item rows are live
    share = _adam_checks(what + ("table",), before["table"], Mb, before["V"], after["table"], Ma, after["V"], g_rec, slack, step_no, False)
    # (b)
    dist["mlp"] = []
    if gate:
        gg = m._dev['gate_grad'].cpu().numpy().astype(np.float64)
        for got, ref in zip(_unpack(gg, case), r64["grad_mlp"]):
            dist["mlp"].append(R.rel_max(got, scale * ref))
        share = max(share, _adam_checks(what + ("mlp",), before["mlp"], before["gm"], before["gv"], after["mlp"], after["gm"], after["gv"],
                                        gg, 0.0, step_no, True))
    info["adam"] = f"{share:.2f}"
    # (a) - (c) against this step's own bounds; everything is printed before anything is asserted
    bound = step_bounds(e32, r64, len((ref_batch or batch)[0]))
    ratio = lambda got, ref: got / ref if ref > 0 else (0.0 if got == 0 else float("inf"))      # noqa: E731
    cell = lambda k: f"{k} {e32[k]:.1e}/{dist[k]:.1e}/{ratio(dist[k], e32[k]):.2f}/{ratio(dist[k], bound[k]):.2f}"      # noqa: E731
    print(f"[gate_shapes] {case_id(case)} {tag}: e32/GPU/ratio/share-of-bound  " + "  ".join(cell(k) for k in ("loss", "reg", "total", "table")) + "  mlp "
          + " ".join(f"{a:.1e}/{g:.1e}/{ratio(g, a):.2f}/{ratio(g, bd):.2f}" for a, g, bd in zip(e32["mlp"], dist["mlp"], bound["mlp"]))
          + "  | " + " ".join(f"{k}={v}" for k, v in info.items()))
    bad = [(tag, k, dist[k], bound[k]) for k in ("loss", "reg", "total", "table") if dist[k] > bound[k]]
    bad += [(tag, R.MLP_NAMES[j], g, bd) for j, (g, bd) in enumerate(zip(dist["mlp"], bound["mlp"])) if g > bd]
    return bad


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_step_against_float64_per_step(pkg, graph_dirs, case):
    """(a) - (e) of the module docstring on four steps of 64 / 37 / 9 / 1 triplets."""
    try:
        ds, m = _gpu_model(pkg, case, graph_dirs[case[8]])
        assert m.has_variants and m.fused_variants and m.use_pop_gate == case[6] and m.i2i_active == case[7]
        inp = model_inputs(case, ds, m)
        m._state(max_batch=64, need_ctx=True)
        bad = []
        for i, batch in enumerate(make_batches(case, ds.n_users, ds.m_items)):
            bad += _judge_step(case, inp, m, batch, i + 1, f"step {i + 1} B={len(batch[0])}")
            m.check_device_errors()
            assert not bool(m._dev['G64'].any()) and m.adam_step == i + 1
        assert not bad, (case_id(case), "beyond the step's bound (step, quantity, GPU's distance, bound)", bad)
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("case", BAD_ID_CASES, ids=case_id)
def test_bad_ids_through_the_gate_kernel(pkg, graph_dirs, case):
    """An out-of-range id in slot 5 of a 16-triplet batch -- a user id of n_users, a positive of m_items, a negative of -1, each
    from fresh parameters: the step runs, the id is reported once, the triplet contributes nothing (its two slot records stay
    zero for the kernel's parameter-gradient phase) and the step is the one of the 15 sound triplets, still divided by B = 16,
    within the bounds of that step."""
    try:
        bad = []
        for which, (name, _, _) in enumerate(BAD_IDS):
            ds, m = _gpu_model(pkg, case, graph_dirs[case[8]])
            inp = model_inputs(case, ds, m)
            m._state(max_batch=64, need_ctx=True)
            batch, sound = bad_id_batch(case, which)
            bad += _judge_step(case, inp, m, batch, 1, name, scale=15.0 / 16.0, ref_batch=sound)
            with pytest.raises(pkg._lib.LgcnError, match="out-of-range"):
                m.check_device_errors()
            m.check_device_errors()
            assert not bool(m._dev['G64'].any()) and m.adam_step == 1
            assert torch.isfinite(m._table).all() and torch.isfinite(m._gate_flat).all()
            del m
        assert not bad, (case_id(case), "beyond the step's bound (bad id, quantity, GPU's distance, bound)", bad)
    finally:
        pkg.world.configure([])


DP_CASES = [(32, 2, 32, 64, 1.0, 1e-4, True, True, "A", "fp32"), (128, 3, 32, 64, 1.0, 0.05, True, True, "A", "fp32")]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("case", DP_CASES, ids=case_id)
def test_dp_epoch_equals_single_gpu_bitwise(pkg, graph_dirs, case, world, mode):
    """test_dp_epoch_optional_branches_loopback's mechanism at d = 32 (half a wave per row) and d = 128 (two columns per lane: the
    exchange block's rows are written at j * 64 + lane): lgcn_train_epoch_dp over loopback ranks, gate + smoothing, a ragged last
    batch whose trailing ranks get nothing -- tables, MLP parameters and per-step losses bit for bit the single-GPU fused epoch's."""
    try:
        B = 44
        ds, ref = _gpu_model(pkg, case, graph_dirs["A"], batch=B)
        rng = np.random.Generator(np.random.PCG64(3 * world + case[0]))
        T = 3 * B + 1
        u = rng.integers(0, ds.n_users, T); p = rng.integers(0, ds.m_items, T); n = rng.integers(0, ds.m_items, T)
        p[:5] = p[5]; n[9] = p[5]; u[20] = u[30]
        U, P, Nn = _dev(u), _dev(p), _dev(n)
        want_loss = ref.fused_epoch(U, P, Nn, B).cpu().numpy()
        want = {k: v.detach().cpu().numpy().copy() for k, v in ref.state_dict().items()}
        L, lib = pkg._lib, pkg._lib.load()
        models = [_gpu_model(pkg, case, graph_dirs["A"], batch=B)[1] for _ in range(world)]
        states = [mm._state(max_batch=B, need_ctx=True, dp_world=world) for mm in models]
        comms = (C.c_void_p * world)()
        L.check(lib.lgcn_dp_init_loopback(world, comms), "loopback")
        steps = (T + B - 1) // B
        streams = [torch.cuda.Stream() for _ in range(world)]
        nblk = int(lib.lgcn_dp_block_floats(states[0]['ctx'], B, world))
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
        for r, mm in enumerate(models):
            assert np.array_equal(losses[r].cpu().numpy(), want_loss), (world, mode, r, losses[r].cpu().numpy(), want_loss)
            for k, v in mm.state_dict().items():
                assert np.array_equal(v.detach().cpu().numpy().view(np.uint32), want[k].view(np.uint32)), (world, mode, r, k)
            assert not bool(mm._dev['G64'].any())
            mm.check_device_errors()
        for r in range(world):
            lib.lgcn_dp_destroy(comms[r])
        fresh = _gpu_model(pkg, case, graph_dirs["A"], batch=B)[1]
        assert np.abs(want["embedding_item.weight"] - fresh.state_dict()["embedding_item.weight"].cpu().numpy()).max() > 1e-4      # (it trained)
    finally:
        pkg.world.configure([])


@pytest.mark.parametrize("case", [CASES[1], CASES[5]], ids=case_id)
def test_fused_equals_autograd_at_the_new_shapes(pkg, graph_dirs, case):
    """--fused_variants 0 (the reference's own sequence around the HIP propagation kernels, what the reference's fixtures pin) on
    the same batches, at the tolerances of test_optional_branches_fused_vs_autograd_other_depths: losses 5e-6, parameters 2e-5."""
    try:
        out = {}
        for fused in (1, 0):
            ds, m = _gpu_model(pkg, case, graph_dirs[case[8]], fused=fused)
            bpr = pkg.utils.BPRLoss(m, pkg.world.config)
            assert bpr.fused == bool(fused)
            losses = [bpr.stageOne(_dev(u, torch.int64), _dev(p, torch.int64), _dev(n, torch.int64))
                      for (u, p, n) in make_batches(case, ds.n_users, ds.m_items)]
            if fused:
                m.check_device_errors()
                assert not bool(m._dev['G64'].any())
            out[fused] = (losses, {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()})
            del bpr, m
        for a, b in zip(out[1][0], out[0][0]):
            assert abs(a - b) < 5e-6, (case_id(case), out[1][0], out[0][0])
        for k in out[1][1]:
            np.testing.assert_allclose(out[1][1][k], out[0][1][k], rtol=0, atol=2e-5, err_msg=f"{case_id(case)} {k}")
    finally:
        pkg.world.configure([])

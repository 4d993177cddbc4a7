"""Matrix factorisation on the GPU (--model mf; csrc/lgcn_mf.hip): lgcn_mf_train_step / _epoch and model.PureMF
against the float64 restatement and the bounds of tests/test_mf_host.py.

Every step is judged from the state the GPU itself held before it (P, M, V read back before, P', M', V' after), so Adam's
lr / eps amplification never enters a tolerance:
  (a) loss_out within the bpr / reg bounds of the float64 values at P;
  (b) g_rec = M + (M' - M) / w1, w1 = float32(0.1), within  bound + 2^-21 (|M| + |M'|) / w1  of the float64 gradient at P
      (lost terms, a lost 1/B, a lost decay or a lost duplicate all land far outside);
  (c) V' within  2^-22 V' + 2 (1 - beta2) |g_rec| 2^-21 (|M| + |M'|) / w1  of  beta2 V + (1 - beta2) g_rec^2;
  (d) P' within  4 u (|P| + 4 lr)  of  P - step_size M' / (sqrt(V') / bc2_sqrt + eps)  in float64 from the GPU's own M', V';
  (e) rows the batch does not name: (c) and (d) with g = 0 and M' = M - w1 M to 1 ulp -- torch's dense Adam;
  (f) G64 all zero after every step;  (g) both bitmaps consistent: the next step still passes.
Shapes: N = 37 + 94 = 131 (no multiple of 32 or 64) and 3 + 5; every d; batch sizes at every lane-group packing boundary
(8 / 4 / 2 / 1 triplets per wave, 32 / 16 / 8 / 4 per workgroup) and a ragged last wave."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from test_mf_host import (EVAL_K, EVAL_SEED, U32, eval_lists, eval_margins, eval_metrics64, mf_batch, mf_model, mf_ref64)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (32, 64, 128, 256)
BATCHES = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 300)
SHAPES = ((37, 94), (3, 5))
LR, DECAY, B1, B2, EPS = 1e-3, 1e-4, 0.9, 0.999, 1e-8
W1 = float(np.float32(1.0 - B1))
F_B2, F_OMB2, F_EPS = float(np.float32(B2)), float(np.float32(1.0 - B2)), float(np.float32(EPS))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


class Ctx:
    """An lgcn_mf context over buffers of its own (the C ABI, without the model)."""

    def __init__(self, pkg, E, n_users, max_batch, decay=DECAY, lr=LR):
        self.L = pkg._lib
        self.lib = pkg._lib.load()
        N, d = E.shape
        self.n_users, self.m_items, self.d, self.max_batch = n_users, N - n_users, d, max_batch
        self.P = _dev(E.astype(np.float32))
        self.M = torch.zeros(N, d, device=DEV)
        self.V = torch.zeros(N, d, device=DEV)
        self.G64 = torch.zeros(N, d, dtype=torch.int64, device=DEV)
        self.bitmap = torch.zeros(2 * ((N + 31) // 32), dtype=torch.int32, device=DEV)
        self.terms = torch.zeros(2 * max_batch, device=DEV)
        self.err = torch.zeros(1, dtype=torch.int32, device=DEV)
        c = self.L.MfConfig()
        c.n_users, c.m_items, c.d, c.max_batch = n_users, N - n_users, d, max_batch
        c.E0, c.adam_m, c.adam_v = self.P.data_ptr(), self.M.data_ptr(), self.V.data_ptr()
        c.G64, c.bitmap, c.terms, c.err = self.G64.data_ptr(), self.bitmap.data_ptr(), self.terms.data_ptr(), self.err.data_ptr()
        c.decay, c.lr, c.beta1, c.beta2, c.eps = decay, lr, B1, B2, EPS
        self.h = C.c_void_p()
        self.L.check(self.lib.lgcn_mf_create(C.byref(c), C.byref(self.h)), "lgcn_mf_create")

    def close(self):
        if self.h:
            self.lib.lgcn_mf_destroy(self.h)
            self.h = None

    __del__ = close

    def step_rc(self, u, p, n, loss=None, B=None):
        u, p, n = (_dev(t, torch.int32) if not torch.is_tensor(t) else t for t in (u, p, n))
        loss = torch.full((3,), -7.0, device=DEV) if loss is None else loss
        rc = self.lib.lgcn_mf_train_step(self.h, self.L.tp(u), self.L.tp(p), self.L.tp(n), int(u.numel()) if B is None else B,
                                         self.L.tp(loss), self.L.current_stream())
        torch.cuda.synchronize()
        return rc, loss

    def step(self, u, p, n):
        rc, loss = self.step_rc(u, p, n)
        assert rc == 0, self.lib.lgcn_last_error()
        return loss.cpu().numpy().astype(np.float64)

    def epoch(self, u, p, n, B):
        u, p, n = (_dev(t, torch.int32) for t in (u, p, n))
        T = int(u.numel())
        losses = torch.full(((T + B - 1) // B, 3), -7.0, device=DEV)
        rc = self.lib.lgcn_mf_train_epoch(self.h, self.L.tp(u), self.L.tp(p), self.L.tp(n), T, B, self.L.tp(losses), self.L.current_stream())
        torch.cuda.synchronize()
        assert rc == 0, self.lib.lgcn_last_error()
        return losses.cpu().numpy()

    def state(self):
        return tuple(t.cpu().numpy().copy() for t in (self.P, self.M, self.V))

    def set_state(self, P, M, V, step):
        for t, a in ((self.P, P), (self.M, M), (self.V, V)):
            t.copy_(torch.from_numpy(a))
        self.lib.lgcn_mf_set_step(self.h, step)

    @property
    def step_count(self):
        return int(self.lib.lgcn_mf_get_step(self.h))


def _table(rng, n_users, m_items, d, scale):
    return (scale * rng.standard_normal((n_users + m_items, d))).astype(np.float32)


def check_step(before, after, loss, ref, step, what, lr=LR):
    """(a) - (e) of the module docstring for one step; returns the largest share of each bound used."""
    P, M, V = (a.astype(np.float64) for a in before)
    P2, M2, V2 = (a.astype(np.float64) for a in after)
    # (a)
    assert abs(loss[1] - ref["bpr"]) <= ref["bpr_bound"], (what, "bpr", loss[1], ref["bpr"], ref["bpr_bound"])
    assert abs(loss[2] - ref["reg"]) <= ref["reg_bound"], (what, "reg", loss[2], ref["reg"], ref["reg_bound"])
    total = ref["bpr"] + DECAY * ref["reg"]
    assert abs(loss[0] - total) <= ref["bpr_bound"] + DECAY * ref["reg_bound"] + 2 * U32 * abs(total), (what, "loss", loss[0], total)
    # (b)
    slack = 2.0 ** -21 * (np.abs(M) + np.abs(M2)) / W1
    g_rec = M + (M2 - M) / W1
    err = np.abs(g_rec - ref["G"])
    tol = ref["G_bound"] + slack
    assert (err <= tol).all(), (what, "gradient", int((err > tol).sum()), float((err / tol).max()), np.argwhere(err > tol)[:4].tolist())
    # (c)
    v_ref = F_B2 * V + F_OMB2 * g_rec * g_rec
    tol_v = 2.0 ** -22 * V2 + 2.0 * F_OMB2 * np.abs(g_rec) * slack
    assert (np.abs(V2 - v_ref) <= tol_v).all(), (what, "v", float((np.abs(V2 - v_ref) - tol_v).max()))
    # (d)
    bc1, bc2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    step_size, bc2_sqrt = float(np.float32(lr / bc1)), float(np.float32(np.sqrt(bc2)))
    p_ref = P - step_size * M2 / (np.sqrt(V2) / bc2_sqrt + F_EPS)
    tol_p = 4.0 * U32 * (np.abs(P) + 4.0 * lr)
    assert (np.abs(P2 - p_ref) <= tol_p).all(), (what, "p", float((np.abs(P2 - p_ref) / tol_p).max()))
    # (e) rows outside the batch: dense Adam with g = 0
    out = ~ref["named"]
    if out.any():
        ulp = np.spacing(np.abs(after[1][out])).astype(np.float64)
        assert (np.abs(M2[out] - (M[out] - W1 * M[out])) <= ulp).all(), (what, "m of an unnamed row")
        assert (np.abs(V2[out] - F_B2 * V[out]) <= 2.0 ** -22 * V2[out]).all(), (what, "v of an unnamed row")
        moving = out[:, None] & (M2 != 0)
        assert (P2[moving] != P[moving]).mean() > 0.9 if moving.any() else True, (what, "rows outside the batch still move")
    return float((err / tol).max())


@pytest.mark.parametrize("scale", [1.0, 0.1])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("d", DIMS)
def test_step_against_float64_per_step(pkg, d, shape, scale):
    n_users, m_items = shape
    rng = np.random.default_rng(17 * d + n_users + int(10 * scale))
    cx = Ctx(pkg, _table(rng, n_users, m_items, d, scale), n_users, max(BATCHES))
    before = cx.state()
    worst = 0.0
    for B in BATCHES:
        for rep in range(5):
            u, p, n = mf_batch(rng, n_users, m_items, B)
            ref = mf_ref64(before[0], n_users, u, p, n, DECAY)
            loss = cx.step(u, p, n)
            after = cx.state()
            worst = max(worst, check_step(before, after, loss, ref, cx.step_count, (d, shape, scale, B, rep)))
            assert int(cx.G64.abs().max()) == 0, ("(f) G64 must be all zero after a step", B, rep)
            # (g) exactly one bitmap carries this step's rows, the other is clear
            words = (n_users + m_items + 31) // 32
            bm = cx.bitmap.cpu().numpy().view(np.uint32).reshape(2, words)
            want = np.zeros(words, np.uint32)
            rows = np.flatnonzero(ref["named"])
            np.bitwise_or.at(want, rows >> 5, (np.uint32(1) << (rows & 31).astype(np.uint32)))
            cur = (cx.step_count - 1) & 1
            assert np.array_equal(bm[cur], want) and not bm[cur ^ 1].any(), ("(g) bitmaps", B, rep)
            before = after
    assert cx.step_count == 5 * len(BATCHES) and int(cx.err.item()) == 0
    print(f"d={d} {shape} scale={scale}: largest share of the gradient tolerance used {worst:.3f}")
    cx.close()


@pytest.mark.parametrize("d", DIMS)
def test_repeatable_and_order_free(pkg, d):
    """The same step from the same state twice: bitwise equal tables, moments and loss.  A permuted batch: bitwise equal tables
    and moments (fixed-point sums commute), the loss within its bound."""
    n_users, m_items, B = 37, 94, 300
    rng = np.random.default_rng(5 + d)
    cx = Ctx(pkg, _table(rng, n_users, m_items, d, 1.0), n_users, B)
    for _ in range(2):                                   # non-trivial moments first
        cx.step(*mf_batch(rng, n_users, m_items, B))
    s0 = cx.state()
    u, p, n = mf_batch(rng, n_users, m_items, B)
    ref = mf_ref64(s0[0], n_users, u, p, n, DECAY)
    l1 = cx.step(u, p, n)
    s1 = cx.state()
    cx.set_state(*s0, step=2)
    l2 = cx.step(u, p, n)
    s2 = cx.state()
    assert all(np.array_equal(a, b) for a, b in zip(s1, s2)) and np.array_equal(l1, l2)
    perm = rng.permutation(B)
    cx.set_state(*s0, step=2)
    l3 = cx.step(u[perm], p[perm], n[perm])
    s3 = cx.state()
    assert all(np.array_equal(a, b) for a, b in zip(s1, s3))
    assert abs(l3[1] - ref["bpr"]) <= ref["bpr_bound"] and abs(l3[2] - ref["reg"]) <= ref["reg_bound"]
    cx.close()


@pytest.mark.parametrize("d", DIMS)
def test_epoch_is_the_loop_of_steps(pkg, d):
    n_users, m_items, B = 37, 94, 64
    T = 5 * B + 17
    rng = np.random.default_rng(11 + d)
    E = _table(rng, n_users, m_items, d, 1.0)
    u, p, n = mf_batch(rng, n_users, m_items, T)
    a, b = Ctx(pkg, E, n_users, B), Ctx(pkg, E, n_users, B)
    la = a.epoch(u, p, n, B)
    lb = np.stack([b.step(u[t:t + B], p[t:t + B], n[t:t + B]) for t in range(0, T, B)]).astype(np.float32)
    assert la.shape == (6, 3) and np.array_equal(la, lb)
    assert all(np.array_equal(x, y) for x, y in zip(a.state(), b.state()))
    assert a.step_count == b.step_count == 6 and int(a.G64.abs().max()) == 0
    a.close(); b.close()


def test_refusals_and_bad_ids(pkg):
    n_users, m_items, d, MB = 37, 94, 64, 16
    rng = np.random.default_rng(2)
    cx = Ctx(pkg, _table(rng, n_users, m_items, d, 1.0), n_users, MB)
    u, p, n = mf_batch(rng, n_users, m_items, MB + 1)
    s0 = cx.state()
    rc, loss = cx.step_rc(u, p, n)                         # B = max_batch + 1: rc 3, pre-filled outputs untouched
    assert rc == 3 and (loss.cpu().numpy() == -7.0).all() and cx.step_count == 0
    assert all(np.array_equal(a, b) for a, b in zip(s0, cx.state())) and int(cx.bitmap.abs().max()) == 0
    rc, loss = cx.step_rc(u[:MB], p[:MB], n[:MB])          # B = max_batch passes
    assert rc == 0 and np.isfinite(loss.cpu().numpy()).all() and cx.step_count == 1
    # an out-of-range id: flagged once, its triplet contributes nothing, the tables stay finite
    s1 = cx.state()
    for which, bad in ((0, n_users), (1, m_items), (2, -1), (2, 2 ** 31 - 1)):
        ids = [u[:MB].copy(), p[:MB].copy(), n[:MB].copy()]
        ids[which][5] = bad
        cx.set_state(*s1, step=1)
        rc, loss = cx.step_rc(*ids)
        assert rc == 0
        assert cx.lib.lgcn_mf_check(cx.h, cx.L.current_stream()) == 1
        assert b"out-of-range" in cx.lib.lgcn_last_error()
        assert cx.lib.lgcn_mf_check(cx.h, cx.L.current_stream()) == 0
        after = cx.state()
        assert all(np.isfinite(a).all() for a in after) and np.isfinite(loss.cpu().numpy()).all()
        # the step is the one of the 15 sound triplets, still divided by B = 16
        keep = np.arange(MB) != 5
        ref = mf_ref64(s1[0], n_users, u[:MB][keep], p[:MB][keep], n[:MB][keep], DECAY)
        g_rec = s1[1].astype(np.float64) + (after[1].astype(np.float64) - s1[1]) / W1
        scale = (MB - 1) / MB
        tol = scale * ref["G_bound"] + 2.0 ** -21 * (np.abs(s1[1]) + np.abs(after[1])) / W1
        assert (np.abs(g_rec - scale * ref["G"]) <= tol).all()
        assert int(cx.G64.abs().max()) == 0
    cx.close()


# ---------------------------------------------------------------------------------------------------------------------------
# the model
def _gpu_model(pkg, tmp_path, **kw):
    ds, m = mf_model(pkg, tmp_path, **kw)
    pkg.world.config.update({'lr': LR, 'decay': DECAY})
    return ds, m.to(DEV)


def test_fused_step_against_autograd_and_oracle(pkg, oracle, tmp_path):
    try:
        ds, m = _gpu_model(pkg, tmp_path)
        rng = np.random.default_rng(8)
        nu = ds.n_users
        E = m._table.cpu().numpy().copy()
        Mo, Vo = np.zeros_like(E), np.zeros_like(E)
        for step in range(1, 6):
            u, p, n = mf_batch(rng, nu, ds.m_items, 64 if step < 5 else 17)
            before = m._table.cpu().numpy().copy()
            Mb = m._dev['adam_m'].cpu().numpy().copy() if m._dev else np.zeros_like(before)
            # torch autograd of PureMF.bpr_loss on the same table, in float64 on the CPU
            _, m64 = mf_model(pkg, tmp_path)
            pkg.world.config.update({'lr': LR, 'decay': DECAY})
            m64.load_state_dict({'embedding_user.weight': torch.from_numpy(before[:nu]), 'embedding_item.weight': torch.from_numpy(before[nu:])})
            m64 = m64.double()
            loss, reg = m64.bpr_loss(torch.from_numpy(u), torch.from_numpy(p), torch.from_numpy(n))
            (loss + DECAY * reg).backward()
            g_auto = torch.cat([m64.embedding_user.weight.grad, m64.embedding_item.weight.grad]).numpy()
            ref = mf_ref64(before, nu, u, p, n, DECAY)
            # the restatement IS upstream's loss (torch's softplus is linear above its threshold 20: e^-20 = 2.1e-9 of a term)
            assert np.abs(g_auto - ref["G"]).max() <= 3e-9 * max(1.0, np.abs(ref["G"]).max())
            out = m.fused_step(torch.from_numpy(u).long().to(DEV), torch.from_numpy(p).long().to(DEV), torch.from_numpy(n).long().to(DEV))
            got = out.cpu().numpy().astype(np.float64)
            Ma = m._dev['adam_m'].cpu().numpy()
            g_rec = Mb.astype(np.float64) + (Ma.astype(np.float64) - Mb) / W1
            tol = ref["G_bound"] + 2.0 ** -21 * (np.abs(Mb) + np.abs(Ma)) / W1
            assert (np.abs(g_rec - g_auto) <= tol).all(), (step, float((np.abs(g_rec - g_auto) / tol).max()))
            assert abs(got[1] - loss.item()) <= ref["bpr_bound"] and abs(got[2] - reg.item()) <= ref["reg_bound"]
            # the oracle's fp32 sequence on its own trajectory: the short-run bar of the project
            bo, ro, Go = oracle.bpr(E, nu, u, p, n, DECAY)
            oracle.adam(E, Go, Mo, Vo, step, lr=LR)
            assert abs(got[0] - (bo + DECAY * ro)) <= 1e-4, (step, got[0], bo + DECAY * ro)
        assert m.adam_step == 5
    finally:
        pkg.world.configure([])


def test_checkpoint_resume_is_bitwise(pkg, tmp_path):
    try:
        rng = np.random.default_rng(21)
        ds, a = _gpu_model(pkg, tmp_path)
        batches = [tuple(torch.from_numpy(t).to(DEV) for t in mf_batch(rng, ds.n_users, ds.m_items, 64)) for _ in range(5)]
        bpr_a = pkg.utils.BPRLoss(a, pkg.world.config)
        la = [bpr_a.stageOne(*b) for b in batches]
        ds, b = _gpu_model(pkg, tmp_path)
        bpr_b = pkg.utils.BPRLoss(b, pkg.world.config)
        lb = [bpr_b.stageOne(*bt) for bt in batches[:3]]
        ck = os.path.join(str(tmp_path), "mf.pth.tar")
        torch.save({'model': b.state_dict(), 'opt': bpr_b.opt.state_dict()}, ck)
        ds, c = _gpu_model(pkg, tmp_path, seed=99)                 # a fresh model with other weights
        bpr_c = pkg.utils.BPRLoss(c, pkg.world.config)
        sd = torch.load(ck, map_location=DEV)
        c.load_state_dict(sd['model'])
        bpr_c.opt.load_state_dict(sd['opt'])
        assert c.adam_step == 3
        lb += [bpr_c.stageOne(*bt) for bt in batches[3:]]
        assert la == lb
        assert torch.equal(a._table, c._table)
        assert torch.equal(a._dev['adam_m'], c._dev['adam_m']) and torch.equal(a._dev['adam_v'], c._dev['adam_v'])
        st = bpr_c.opt.state_dict()['state']
        assert len(st) == 2 and all(float(s['step']) == 5.0 for s in st.values())
        with pytest.raises(RuntimeError, match="fused"):
            bpr_c.opt.step()
    finally:
        pkg.world.configure([])


def test_procedure_test_ranks_the_raw_scores(pkg, tmp_path):
    w = pkg.world
    old_topks = list(w.topks)
    try:
        ds, m = _gpu_model(pkg, tmp_path, seed=EVAL_SEED)
        E = m._table.cpu().numpy()
        users, train, test = eval_lists(ds)
        assert (eval_margins(E, ds.n_users, users, train, test) > 0).all()          # decided in fp32 (checked on the CPU as well)
        want = eval_metrics64(E, ds.n_users, ds.m_items, users, train, test)
        w.topks = [EVAL_K]
        fused = pkg.Procedure.Test(ds, m, 0)
        w.config['rank_metrics'] = 1
        ranks = pkg.Procedure.Test(ds, m, 0)
        w.config['rank_metrics'] = 0
        w.config['eval_fused'] = 0
        harness = pkg.Procedure.Test(ds, m, 0)                                       # torch, on getUsersRating = the sigmoid
        assert sorted(fused) == ['ndcg', 'precision', 'recall'] and sorted(ranks) == ['auc', 'mrr', 'ndcg', 'precision', 'recall']
        for name in ('precision', 'recall', 'ndcg'):
            assert abs(float(fused[name][0]) - want[name]) <= 1e-12, (name, fused[name], want[name])
            assert abs(float(ranks[name][0]) - want[name]) <= 1e-12, (name, ranks[name], want[name])
            assert 0.0 <= float(harness[name][0]) <= 1.0
        for name in ('auc', 'mrr'):
            assert abs(float(ranks[name]) - want[name]) <= 1e-12, (name, ranks[name], want[name])
        with torch.no_grad():
            r = m.getUsersRating(torch.arange(4, device=DEV))
            assert float(r.min()) >= 0.0 and float(r.max()) <= 1.0
    finally:
        w.topks = old_topks
        w.configure([])


def test_bpr_train_original_runs_and_learns(pkg, tmp_path):
    try:
        ds, m = _gpu_model(pkg, tmp_path)
        pkg.world.config.update({'lr': 0.01, 'prefetch_epoch': 0})
        pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        bpr.opt.param_groups[0]['lr'] = 0.01
        losses = []
        for epoch in range(3):
            info = pkg.Procedure.BPR_train_original(ds, m, bpr, epoch)
            assert info.startswith("loss")
            losses.append(float(info[4:].split("-")[0]))
        assert losses[2] < losses[0], losses
        assert m.adam_step == 3 * ((ds.trainDataSize + 63) // 64) and torch.isfinite(m._table).all()
        rows = open(os.path.join(pkg.world.config['checkpoint_dir'], 'train_epoch_metrics.csv')).read().strip().splitlines()
        assert rows[0] == 'epoch,loss' and len(rows) == 4
    finally:
        pkg.world.configure([])

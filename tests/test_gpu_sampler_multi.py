"""The device sampler for several negatives per positive (lgcn_sample_negative_device_multi; DESIGN 4 *Sampler*) on the GPU.
The judge everywhere is the host sampler sampling.sample_negative(..., R), which tests/test_host.py pins to the reference's
compiled plugin; equality is exact: the same int32 rows, the same position of the rand() stream afterwards."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import storage_cases as SC                       # noqa: E402
from storage_cases import storage_graph          # noqa: E402,F401  (fixture: the graph, written once per session)
from conftest import GOLDEN, REPO                # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _csr(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.concatenate(rows)


def _assert_rows(want, got, tag):
    assert got.dtype == np.int32 and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    bad = np.flatnonzero((want != got).any(axis=1))
    assert bad.size == 0, (tag, bad.size, bad[:5], want[bad[:3]], got[bad[:3]])


def _epochs(S, shape, csr, R, seed, n, device=None):
    """n consecutive epochs and four draws behind them, from the host sampler or from a device call"""
    S.seed(seed)
    if device is None:
        rows = [S.sample_negative(*shape, csr, R) for _ in range(n)]
    else:
        rows = [device(*shape, csr, DEV, R).cpu().numpy() for _ in range(n)]
    return rows, [S.randint(1 << 20) for _ in range(4)]


def _dense_small():
    """the graph of test_gpu_sampler_bit_exact: 700 users, 160 items, degrees 1..59"""
    rng = np.random.Generator(np.random.PCG64(12))
    n_users, m_items = 700, 160
    rows = [np.sort(rng.choice(m_items, size=int(rng.integers(1, 60)), replace=False)).astype(np.int32) for _ in range(n_users)]
    return (n_users, m_items, 13 * n_users + 5), _csr(rows)


# ---- 1. a dense small graph: most samples hold a rejection, often several in different slots -----------------------------------
@pytest.mark.parametrize("R", [1, 2, 3, 5, 16])
def test_dense_small_graph_bit_exact(pkg, R):
    S = pkg.sampling
    shape, csr = _dense_small()
    W, T = 1 + R, shape[0] * (shape[2] // shape[0])
    want, tail_host = _epochs(S, shape, csr, R, 77, 2)
    assert want[0].shape == (T, 2 + R)
    # not vacuous: the draws the host consumed for the first epoch, found in the expanded stream
    S.seed(77)
    S.sample_negative(*shape, csr, R)
    mark = [S.randint(1 << 20) for _ in range(4)]
    S.seed(77)
    stream = np.array([S.randint(1 << 20) for _ in range(2 * W * T + 4)])
    hit = np.flatnonzero((stream[:-3] == mark[0]) & (stream[1:-2] == mark[1]) & (stream[2:-1] == mark[2]) & (stream[3:] == mark[3]))
    assert hit.size == 1
    extra = int(hit[0]) - W * T
    print(f"[sampler_multi] dense R={R}: {extra} rejected draws in {T} samples")
    assert extra > T // 10 and (R < 5 or extra > T)              # at R >= 5 more rejections than samples
    got, tail_dev = _epochs(S, shape, csr, R, 77, 2, S.sample_negative_device_multi)
    for e in range(2):
        _assert_rows(want[e], got[e], (R, e))
    assert tail_dev == tail_host                                  # the stream position after the device epochs
    if R == 1:
        old, tail_old = _epochs(S, shape, csr, 1, 77, 2, lambda *a: S.sample_negative_device(*a[:5]))
        for e in range(2):
            _assert_rows(old[e], got[e], ("three-slot entry point", e))
        assert tail_old == tail_host
    else:                                                         # neg_num of the public call reaches the same entry point
        S.seed(77)
        _assert_rows(want[0], S.sample_negative_device(*shape, csr, DEV, neg_num=R).cpu().numpy(), (R, "neg_num="))


# ---- 2. heavy tail: runs longer than SAMP_DMAX inside one sample, events in consecutive slots, the finisher taking over ----------
@pytest.mark.parametrize("R", [4, 8])
def test_heavy_tail_bit_exact(pkg, R):
    """the generator of test_gpu_sampler_segments_heavy_tail_bit_exact"""
    S = pkg.sampling
    rng = np.random.Generator(np.random.PCG64(2024))
    n_users, m_items = 3000, 2000
    deg = np.minimum(m_items // 4, np.maximum(1, (30.0 / rng.random(n_users) ** 0.7).astype(np.int64) // 8))
    deg[100:108] = m_items // 2                 # adjacent hubs
    deg[1500] = deg[1501] = m_items - 20        # 99 % positive
    deg[2999] = m_items // 3                    # the last user
    csr = _csr([np.sort(rng.choice(m_items, size=int(k), replace=False)).astype(np.int32) for k in deg])
    shape = (n_users, m_items, 15 * n_users + 7)
    want, tail_host = _epochs(S, shape, csr, R, 31, 2)
    got, tail_dev = _epochs(S, shape, csr, R, 31, 2, S.sample_negative_device_multi)
    for e in range(2):
        _assert_rows(want[e], got[e], (R, e))
    assert tail_dev == tail_host


# ---- 3. few interactions per user: the one-workgroup kernel alone --------------------------------------------------------------
@pytest.mark.parametrize("per_user,extra", [(5, 3), (1, 3), (7, 0)])
def test_few_interactions_per_user_bit_exact(pkg, per_user, extra):
    S = pkg.sampling
    rng = np.random.Generator(np.random.PCG64(5 + per_user))
    n_users, m_items, R = 2500, 300, 3
    csr = _csr([np.sort(rng.choice(m_items, size=int(rng.integers(1, 90)), replace=False)).astype(np.int32) for _ in range(n_users)])
    shape = (n_users, m_items, per_user * n_users + extra)
    assert shape[2] // n_users == per_user < 8
    want, tail_host = _epochs(S, shape, csr, R, 11, 2)
    got, tail_dev = _epochs(S, shape, csr, R, 11, 2, S.sample_negative_device_multi)
    for e in range(2):
        _assert_rows(want[e], got[e], (per_user, e))
    assert tail_dev == tail_host


# ---- 4. the end of the stream --------------------------------------------------------------------------------------------------
def test_segments_reach_the_end_of_the_stream(pkg):
    """The mid-density generator of test_gpu_sampler_segments_reach_the_end_of_the_stream (4000 users x 50 of 2000 items) at
    R = 3 with the margin made small through the test hook.  Expected extra draws X = R T p / (1 - p) = 15 385 with p = 50 / 2000
    (standard deviation ~ 125); the stream is whole blocks of 4 092 draws, so the margins at or below X / 2 must end in rc 5,
    those at or above 2 X in rc 0, and the outcome of those within ~4 100 draws of X is not fixed -- but every margin ends in
    one of the two ways and the sequence is monotone."""
    S = pkg.sampling
    lib = pkg._lib.load()
    rng = np.random.Generator(np.random.PCG64(77))
    n_users, m_items, deg, R = 4000, 2000, 50, 3
    rows = [np.sort(rng.choice(m_items, size=deg, replace=False)).astype(np.int32) for _ in range(n_users)]
    csr = (np.arange(n_users + 1, dtype=np.int64) * deg, np.concatenate(rows))
    shape = (n_users, m_items, n_users * deg)
    T, p = n_users * deg, deg / m_items
    X = R * T * p / (1 - p)
    want, tail_host = _epochs(S, shape, csr, R, 5, 1)
    want = want[0]
    margins = [1, 2000, int(X / 4), int(X / 2), int(X) - 3000, int(X) - 1000, int(X), int(X) + 1000, int(X) + 3000, int(2 * X), int(3 * X), int(5 * X)]
    assert margins == sorted(margins)
    outcomes = []
    try:
        for fixed in margins:
            lib.lgcn_sampler_test_margin(1 << 40, fixed)
            S._DEVICE_CSR.clear()
            S.seed(5)
            try:
                got = S.sample_negative_device_multi(*shape, csr, DEV, R).cpu().numpy()
            except pkg._lib.LgcnError as e:
                assert "(rc=5)" in str(e), str(e)
                # the host generator has not moved: the host sampler now draws the epoch the reference draws
                _assert_rows(want, S.sample_negative(*shape, csr, R), (fixed, "host after rc 5"))
                outcomes.append(5)
                continue
            _assert_rows(want, got, fixed)
            assert [S.randint(1 << 20) for _ in range(4)] == tail_host, fixed
            outcomes.append(0)
    finally:
        lib.lgcn_sampler_test_margin(0, 0)
        S._DEVICE_CSR.clear()
    print(f"[sampler_multi] end of stream: X = {X:.0f}, margins {margins} -> {outcomes}")
    assert outcomes == sorted(outcomes, reverse=True), outcomes        # small margins fail, large ones pass
    assert all(o == 5 for m_, o in zip(margins, outcomes) if m_ <= X / 2), outcomes
    assert all(o == 0 for m_, o in zip(margins, outcomes) if m_ >= 2 * X), outcomes
    assert 5 in outcomes and 0 in outcomes


# ---- 5. the fallback in Procedure ----------------------------------------------------------------------------------------------
def test_margin_falls_back_to_host_in_procedure(pkg, tmp_path):
    """The dense dataset of test_gpu_sampler_margin_falls_back_to_host (every user holds 90 % of the items) with --neg_ratio 2:
    the device call raises rc 5 and Procedure.sample_epoch_to_device returns what --gpu_sampler 0 returns, two epochs."""
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
    try:
        for gpu in (1, 0):
            w.configure(["--dataset", "dense", "--tensorboard", "0", "--gpu_sampler", str(gpu), "--prefetch_epoch", "0", "--neg_ratio", "2"])
            ds = pkg.dataloader.Loader(w.config, path=path)
            pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
            if gpu:
                with pytest.raises(pkg._lib.LgcnError, match="rc=5"):
                    pkg.sampling.sample_negative_device(ds.n_users, ds.m_items, ds.trainDataSize, ds.pos_csr(), DEV, neg_num=2)
            out.append([tuple(t.cpu().numpy() for t in pkg.Procedure.sample_epoch_to_device(ds, DEV)) for _ in range(2)])
    finally:
        w.configure([])
    for e in range(2):
        for c in range(3):
            assert np.array_equal(out[0][e][c], out[1][e][c]), (e, c)
    assert out[0][0][0].shape == (n_users * keep,) and out[0][0][2].shape == (2, n_users * keep)


# ---- 6. Gowalla ----------------------------------------------------------------------------------------------------------------
def test_gowalla_epoch_bit_exact(pkg, tmp_path):
    sys.path.insert(0, REPO)
    from bench import materialize_gowalla
    S = pkg.sampling
    d = materialize_gowalla(os.path.join(GOLDEN, "gowalla", "gowalla.npz"), os.path.join(str(tmp_path), "gowalla"))
    try:
        pkg.world.configure(["--dataset", "gowalla", "--tensorboard", "0"])
        gds = pkg.dataloader.Loader(pkg.world.config, path=d)
    finally:
        pkg.world.configure([])
    shape, csr = (gds.n_users, gds.m_items, gds.trainDataSize), gds.pos_csr()
    want, tail_host = _epochs(S, shape, csr, 4, 2020, 1)
    got, tail_dev = _epochs(S, shape, csr, 4, 2020, 1, S.sample_negative_device_multi)
    assert got[0].shape == (806166, 6)
    _assert_rows(want[0], got[0], "gowalla")
    assert tail_dev == tail_host


# ---- 7. host and device calls interleaved on one stream ------------------------------------------------------------------------
def test_host_and_device_calls_interleaved(pkg):
    S = pkg.sampling
    shape, csr = _dense_small()
    S.seed(123)
    want = [S.sample_negative(*shape, csr, R) for R in (2, 3, 1, 3)]
    tail_host = [S.randint(1 << 20) for _ in range(4)]
    S.seed(123)
    got = [S.sample_negative(*shape, csr, 2),
           S.sample_negative_device(*shape, csr, DEV, neg_num=3).cpu().numpy(),
           S.sample_negative_device(*shape, csr, DEV).cpu().numpy(),                 # the three-slot entry point
           S.sample_negative(*shape, csr, 3)]
    for i, (w_, g_) in enumerate(zip(want, got)):
        _assert_rows(w_, g_, i)
    assert [S.randint(1 << 20) for _ in range(4)] == tail_host


# ---- 8. one training epoch -----------------------------------------------------------------------------------------------------
def test_training_epoch_is_the_host_samplers_epoch_bitwise(pkg, storage_graph, tmp_path, monkeypatch):
    """One Procedure.BPR_train_original epoch on the storage graph with --neg_ratio 3, the rows drawn on the device
    (--gpu_sampler 1) and on the host (0): the per-step losses and the final table are equal bit for bit."""
    runs, calls = [], []
    real = pkg.sampling.sample_negative_device_multi
    monkeypatch.setattr(pkg.sampling, "sample_negative_device_multi", lambda *a, **k: (calls.append(a[-1]), real(*a, **k))[1])
    try:
        for gpu in (1, 0):
            w = SC.configure(pkg, ("fp32", 64, 2, 1, -1, "propagated"), storage_graph, 256)
            w.config.update(neg_ratio=3, prefetch_epoch=0, sampler='cpp', gpu_sampler=gpu,
                            checkpoint_dir=os.path.join(str(tmp_path), f"ckpt{gpu}"))
            w.tensorboard = 0
            ds = pkg.dataloader.Loader(w.config, path=storage_graph)
            pkg.utils.set_seed(SC.MODEL_SEED)
            m = pkg.model.LightGCN(w.config, ds)
            SC.set_rows(m._table)
            m = m.to(DEV)
            m.train()
            losses = []
            fused = m.fused_epoch
            m.fused_epoch = lambda *a, **k: (losses.append(fused(*a, **k)), losses[-1])[1]
            pkg.sampling.seed(31); pkg.utils.set_seed(32)
            n_calls = len(calls)
            info = pkg.Procedure.BPR_train_original(ds, m, pkg.utils.BPRLoss(m, w.config), 1)
            assert info.startswith("loss") and len(losses) == 1
            assert len(calls) - n_calls == gpu and (not gpu or calls[-1] == 3)      # the device sampler ran exactly where asked
            runs.append((losses[0].cpu().numpy().copy(), m._table.detach().cpu().numpy().copy(), pkg.sampling.randint(1 << 20)))
    finally:
        pkg.world.configure([])
    assert runs[0][0].shape[0] > 1
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    assert np.array_equal(runs[0][1].view(np.uint32), runs[1][1].view(np.uint32))
    assert runs[0][2] == runs[1][2]

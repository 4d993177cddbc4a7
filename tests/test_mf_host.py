"""Matrix factorisation (--model mf, model.PureMF): everything that needs no device -- the registry, the
initial weights, the state_dict surface, the refusals, the C ABI additions -- and the float64 restatement of the step with its
rounding bounds, which tests/test_gpu_mf.py imports.  The last test holds the bounds against the project's fp32 oracle
(oracle.bpr on the table itself IS an fp32 MF step): they must contain a plain fp32 evaluation with room to spare.

The restatement (upstream LightGCN's PureMF.bpr_loss), for B triplets (u, p, n) with rows U, P, Nn of the table:
    x_b = <U_b, Nn_b> - <U_b, P_b>,  bpr = mean_b softplus(x_b),  reg = 1/2 (|U|^2 + |P|^2 + |Nn|^2) / B,
    row u += (s_b (Nn_b - P_b) + decay U_b) / B,  row p += (-s_b U_b + decay P_b) / B,  row n += (s_b U_b + decay Nn_b) / B.

The bounds, per element, u = 2^-24, A_b = sum_k |U_bk| (|P_bk| + |Nn_bk|):
    bpr : u [(d + 4) mean_b A_b + (B + 4) mean_b softplus(x_b)]       d products and sums per score, a few roundings in
                                                                        softplus, B terms in the mean
    reg : u (3 d + B + 4) reg
    grad: es_b = (d + 2) u A_b / 4 + 4 u bounds the error of s_b (|sigmoid'| <= 1/4 times the error of x_b, plus its own
          roundings); a contribution of triplet b to (row r, column k) errs by at most
          [es_b |coef_bk| + 4 u (|s_b coef_bk| + decay |own_bk|)] / B  (user row: coef = Nn - P, own = U; item row: coef = U,
          own = the row), and the sum of count_r contributions plus the fp32 conversion by (count_r + 1) u sum|contribution|;
          1e-14 covers the 2^-50 fixed-point quantum of each contribution."""
import importlib
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, PKG_NAME

U32 = 2.0 ** -24
MF_SYMBOLS = {
    "lgcn_mf_create": "int lgcn_mf_create(const lgcn_mf_config *cfg, lgcn_mf **out);",
    "lgcn_mf_destroy": "void lgcn_mf_destroy(lgcn_mf *mf);",
    "lgcn_mf_get_step": "int64_t lgcn_mf_get_step(const lgcn_mf *mf);",
    "lgcn_mf_set_step": "void lgcn_mf_set_step(lgcn_mf *mf, int64_t step);",
    "lgcn_mf_set_lr": "void lgcn_mf_set_lr(lgcn_mf *mf, double lr);",
    "lgcn_mf_train_step": "int lgcn_mf_train_step(lgcn_mf *mf, const int32_t *users, const int32_t *pos, const int32_t *neg, "
                          "int32_t B, float *loss_out, void *stream);",
    "lgcn_mf_train_epoch": "int lgcn_mf_train_epoch(lgcn_mf *mf, const int32_t *users, const int32_t *pos, const int32_t *neg, "
                           "int64_t T, int32_t B, float *loss_out, void *stream);",
    "lgcn_mf_check": "int lgcn_mf_check(lgcn_mf *mf, void *stream);",
}
MF_CONFIG_FIELDS = ["n_users", "m_items", "d", "E0", "adam_m", "adam_v", "G64", "bitmap", "terms", "err", "max_batch", "decay",
                    "lr", "beta1", "beta2", "eps"]


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 restatement and its bounds (shared with tests/test_gpu_mf.py)
def mf_ref64(E, n_users, users, pos, neg, decay):
    """-> dict: bpr, reg, G [N, d] (float64) and the bounds bpr_bound, reg_bound, G_bound [N, d] of the module docstring."""
    E = np.asarray(E, np.float64)
    N, d = E.shape
    users, pos, neg = (np.asarray(t, np.int64) for t in (users, pos, neg))
    B = len(users)
    ru, rp, rn = users, pos + n_users, neg + n_users
    U, P, Nn = E[ru], E[rp], E[rn]
    x = (U * Nn).sum(1) - (U * P).sum(1)
    sp = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
    s = np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
    bpr = sp.mean()
    reg = 0.5 * ((U * U).sum() + (P * P).sum() + (Nn * Nn).sum()) / B
    A = (np.abs(U) * (np.abs(P) + np.abs(Nn))).sum(1)
    es = (d + 2) * U32 * A / 4.0 + 4.0 * U32
    G = np.zeros((N, d))
    S = np.zeros((N, d))                  # sum of |contribution|
    Eb = np.zeros((N, d))                 # sum of the contributions' own error bounds
    cnt = np.zeros(N)
    for rows, coef, sign, own in ((ru, Nn - P, 1.0, U), (rp, U, -1.0, P), (rn, U, 1.0, Nn)):
        c = (sign * s[:, None] * coef + decay * own) / B
        np.add.at(G, rows, c)
        np.add.at(S, rows, np.abs(c))
        np.add.at(Eb, rows, (es[:, None] * np.abs(coef) + 4.0 * U32 * (np.abs(s[:, None] * coef) + decay * np.abs(own))) / B)
        np.add.at(cnt, rows, 1.0)
    return {"bpr": bpr, "reg": reg, "G": G, "x": x,
            "bpr_bound": U32 * ((d + 4) * A.mean() + (B + 4) * sp.mean()),
            "reg_bound": U32 * (3 * d + B + 4) * reg,
            "G_bound": Eb + (cnt[:, None] + 1.0) * U32 * S + 1e-14,
            "named": cnt > 0}


def mf_batch(rng, n_users, m_items, B):
    """B triplets holding, as far as B allows: one user three times, an item that is one triplet's positive and another's
    negative, a repeated positive, and the first and last row of both blocks."""
    u = rng.integers(0, n_users, B)
    p = rng.integers(0, m_items, B)
    n = rng.integers(0, m_items, B)
    if B >= 3:
        u[0:3] = u[0]
    if B >= 2:
        n[1] = p[0]
    if B >= 4:
        p[3] = p[2]
    if B >= 6:
        u[-2], p[-2], n[-2] = 0, 0, m_items - 1
    u[-1], p[-1], n[-1] = n_users - 1, m_items - 1, 0
    return u.astype(np.int32), p.astype(np.int32), n.astype(np.int32)


def tiny_dir(tmp_path):
    d = os.path.join(str(tmp_path), "tiny")
    os.makedirs(d, exist_ok=True)
    for f in ("train.txt", "test.txt"):
        shutil.copyfile(os.path.join(GOLDEN, "tiny", f), os.path.join(d, f))
    return d


def mf_model(pkg, tmp_path, args=(), extra=None, d=64, batch=64, seed=2020):
    """(dataset, PureMF on the CPU) on the tiny fixture, built under torch.manual_seed(seed)."""
    path = tiny_dir(tmp_path)
    w = pkg.world
    w.configure(["--model", "mf", "--dataset", "tiny", "--tensorboard", "0", "--recdim", str(d), "--bpr_batch", str(batch)] + list(args))
    if extra:
        w.config.update(extra)
    w.config['checkpoint_dir'] = os.path.join(str(tmp_path), "ckpt")
    ds = pkg.dataloader.Loader(w.config, path=path)
    torch.manual_seed(seed)
    return ds, pkg.model.PureMF(w.config, ds)


# ---- Procedure.Test on a PureMF: the float64 ranking of the raw scores and the seed whose ranking no fp32 rounding can move
EVAL_SEED = 2020
EVAL_K = 20


def eval_lists(ds):
    users = np.fromiter(ds.testDict.keys(), dtype=np.int64, count=len(ds.testDict))
    train = [np.sort(np.asarray(ds.allPos[u], np.int64)) for u in range(ds.n_users)]
    test = [np.asarray(ds.testDict[u], np.int64) for u in users.tolist()]
    return users, train, test


def eval_margins(E, n_users, users, train, test, k=EVAL_K):
    """For every evaluated user: (distance of the nearest test item's raw score from the k-th best candidate score, nearest
    distance of a test item's score from any OTHER candidate's score) minus 2 b each, b = 2 sqrt(d) 2^-24 |u| max|i| (the
    bound tests/test_gpu_eval_ranks.py uses for the distance of any fp32 score from its exact value).  Both positive: every
    comparison a ranking of the test items needs comes out as in float64."""
    E = np.asarray(E, np.float64)
    d = E.shape[1]
    inorm = np.linalg.norm(E[n_users:], axis=1).max()
    out = []
    for s, u in enumerate(users.tolist()):
        sc = E[u] @ E[n_users:].T
        cand = np.setdiff1d(np.arange(E.shape[0] - n_users), train[u])
        t = np.setdiff1d(test[s], train[u])
        b2 = 2.0 * (2.0 * np.sqrt(d) * U32 * np.linalg.norm(E[u]) * inorm)
        kth = np.sort(sc[cand])[::-1][k - 1]
        gap_k = np.abs(sc[t] - kth)
        gap_k = gap_k[gap_k > 0].min() if (gap_k > 0).any() else np.inf       # (a test item that IS the k-th best is judged below)
        gap_any = min(np.abs(sc[i] - np.delete(sc[cand], np.searchsorted(cand, i))).min() for i in t.tolist()) if len(t) else np.inf
        out.append((gap_k - b2, gap_any - b2))
    return np.asarray(out)


def eval_metrics64(E, n_users, m_items, users, train, test, k=EVAL_K):
    """precision / recall / ndcg at k, auc (utils.AUC's Mann-Whitney form) and mrr of the float64 ranking of the raw scores,
    train positives masked to -1024 as Procedure.Test does; means over the evaluated users."""
    E = np.asarray(E, np.float64)
    disc = 1.0 / np.log2(np.arange(2, k + 2))
    acc = {m: [] for m in ("precision", "recall", "ndcg", "auc", "mrr")}
    for s, u in enumerate(users.tolist()):
        sc = E[u] @ E[n_users:].T
        sc[train[u]] = -1024.0
        order = np.argsort(-sc, kind="stable")
        rank = np.empty(m_items, np.int64)
        rank[order] = np.arange(m_items)
        t = test[s]
        hits = np.isin(order[:k], t).astype(np.float64)
        acc["precision"].append(hits.sum() / k)
        acc["recall"].append(hits.sum() / len(t))
        idcg = disc[:min(k, len(t))].sum()
        acc["ndcg"].append((hits * disc).sum() / idcg)
        n = len(t)
        below = np.array([(sc < sc[i]).sum() + 0.5 * ((sc == sc[i]).sum() - 1) for i in t.tolist()])
        pos_below = np.array([(sc[t] < sc[i]).sum() + 0.5 * ((sc[t] == sc[i]).sum() - 1) for i in t.tolist()])
        acc["auc"].append(0.0 if n == 0 or n == m_items else float((below - pos_below).sum() / (n * (m_items - n))))
        acc["mrr"].append(1.0 / (rank[t].min() + 1.0))
    return {m: float(np.mean(v)) for m, v in acc.items()}


# ---------------------------------------------------------------------------------------------------------------------------
def test_registry_picks_up_puremf(pkg, tmp_path):
    w = pkg.world
    old_data_path = w.DATA_PATH
    tiny_dir(tmp_path)
    try:
        w.configure(["--model", "mf", "--dataset", "tiny", "--tensorboard", "0", "--data_path", str(tmp_path)])
        assert w.model_name == "mf"
        sys.modules.pop(PKG_NAME + ".register", None)
        reg = importlib.import_module(PKG_NAME + ".register")
        assert reg.MODELS["mf"] is pkg.model.PureMF and reg.MODELS["lgn"] is pkg.model.LightGCN
        assert os.path.basename(pkg.utils.getFileName()) == "mf-tiny-64.pth.tar"
        m = reg.MODELS[w.model_name](w.config, reg.dataset)
        assert isinstance(m, pkg.model.PureMF) and (m.n_users, m.m_items, m.latent_dim) == (50, 80, 64)
    finally:
        sys.modules.pop(PKG_NAME + ".register", None)
        w.configure([])
        w.DATA_PATH = old_data_path


def test_initial_weights_and_state_dict(pkg, tmp_path):
    try:
        for d in (32, 64):
            ds, m = mf_model(pkg, tmp_path, d=d)
            torch.manual_seed(2020)
            eu = torch.nn.Embedding(ds.n_users, d)          # nn.Embedding's own N(0, 1): no normal_(std=0.1)
            ei = torch.nn.Embedding(ds.m_items, d)
            assert torch.equal(m.embedding_user.weight.data, eu.weight.data) and torch.equal(m.embedding_item.weight.data, ei.weight.data)
            assert 0.9 < float(m._table.std()) < 1.1
            assert list(m.state_dict().keys()) == ["embedding_user.weight", "embedding_item.weight"]
            assert [n for n, _ in m.named_parameters()] == ["embedding_user.weight", "embedding_item.weight"]
            # ONE contiguous [N, d] fp32 table, users first
            assert m._table.shape == (ds.n_users + ds.m_items, d) and m._table.dtype == torch.float32 and m._table.is_contiguous()
            assert m.embedding_user.weight.data_ptr() == m._table.data_ptr()
            assert m.embedding_item.weight.data_ptr() == m._table.data_ptr() + ds.n_users * d * 4
            assert m.propagated_table() is m._table and m.rating_table() is m._table and m.has_variants is False
            cu, ci = m.computer()
            assert cu is m.embedding_user.weight and ci is m.embedding_item.weight
            # a load_state_dict round trip keeps the one-table binding
            sd = {k: v.clone() for k, v in m.state_dict().items()}
            ds2, m2 = mf_model(pkg, tmp_path, d=d, seed=7)
            assert not torch.equal(m2._table, m._table)
            m2.load_state_dict(sd)
            m2._check_table()
            assert torch.equal(m2._table, m._table)
            assert m2.embedding_user.weight.data_ptr() == m2._table.data_ptr()
            assert m2.embedding_item.weight.data_ptr() == m2._table.data_ptr() + ds.n_users * d * 4
    finally:
        pkg.world.configure([])


def test_no_graph_is_built(pkg, tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("PureMF must not build or load the graph")
    try:
        for name in ("getSparseGraph", "getSparseGraphCSR"):
            monkeypatch.setattr(pkg.dataloader.Loader, name, boom, raising=False)
        ds, m = mf_model(pkg, tmp_path, args=["--layer", "7"])          # --layer is ignored
        u = torch.tensor([0, 3, 49]); i = torch.tensor([0, 79, 5])
        with torch.no_grad():
            r = m.getUsersRating(u)
            E = m._table.double()
            assert r.shape == (3, ds.m_items)
            assert torch.allclose(r.double(), torch.sigmoid(E[u] @ E[ds.n_users:].T), atol=1e-6)
            assert torch.allclose(m(u, i).double(), torch.sigmoid((E[u] * E[ds.n_users + i]).sum(1)), atol=1e-6)
        # bpr_loss is plain torch on the views and differentiable: its gradient is the restatement's
        uu, pp, nn_ = mf_batch(np.random.default_rng(3), ds.n_users, ds.m_items, 9)
        loss, reg = m.bpr_loss(torch.from_numpy(uu), torch.from_numpy(pp), torch.from_numpy(nn_))
        (loss + 1e-4 * reg).backward()
        ref = mf_ref64(m._table.detach().numpy(), ds.n_users, uu, pp, nn_, 1e-4)
        g = torch.cat([m.embedding_user.weight.grad, m.embedding_item.weight.grad]).numpy()
        assert abs(loss.item() - ref["bpr"]) <= ref["bpr_bound"] and abs(reg.item() - ref["reg"]) <= ref["reg_bound"]
        assert (np.abs(g - ref["G"]) <= ref["G_bound"]).all()
    finally:
        pkg.world.configure([])


def test_refusals(pkg, tmp_path):
    L = pkg._lib
    try:
        for args, extra, flag in (
                (["--use_pop_gate"], None, "--use_pop_gate"),
                (["--use_item_item"], None, "--use_item_item"),
                (["--dropout", "1"], None, "--dropout 1"),
                (["--layer_weights", "exp"], None, "--layer_weights"),
                (["--layer_weights", "[0.5,0.5]"], None, "--layer_weights"),
                (["--use_ppr_weights"], None, "--use_ppr_weights"),
                (["--act_dtype", "bf16"], None, "--act_dtype"),
                (["--act_dtype", "fp8"], None, "--act_dtype")):
            with pytest.raises(L.LgcnError, match=re.escape(flag) + ".*--model mf"):
                mf_model(pkg, tmp_path, args=args, extra=extra)
        with pytest.raises(ValueError, match="latent_dim_rec"):
            mf_model(pkg, tmp_path, d=48)
        for reg_rows in ("propagated", "ego"):                      # both mean the same thing here
            mf_model(pkg, tmp_path, args=["--reg_rows", reg_rows])
        ds, m = mf_model(pkg, tmp_path)
        with pytest.raises(RuntimeError, match="--model mf"):       # before torch.distributed is even looked at
            pkg.parallel.DataParallelBPR(m, pkg.world.config)
        # the optimizer surface needs no device until a step or a load
        bpr = pkg.utils.BPRLoss(m, pkg.world.config)
        assert bpr.fused and isinstance(bpr.opt, pkg.utils._AdamView) and m.adam_step == 0
        assert bpr.opt.state_dict()['state'] == {}
    finally:
        pkg.world.configure([])


def _norm(s):
    return re.sub(r"\s+", " ", s).strip()


def test_abi_additions(pkg):
    import ctypes as C
    hdr = open(os.path.join(REPO, "include", "lgcn_hip.h")).read()
    assert int(re.search(r"#define\s+LGCN_ABI_VERSION\s+(\d+)", hdr).group(1)) == 13 == pkg._lib.ABI_VERSION       # additive
    bare = _norm(re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    lib = pkg._lib.load()
    assert lib.lgcn_abi_version() == 13
    for name, decl in MF_SYMBOLS.items():
        assert _norm(decl) in bare, name
        assert name in pkg._lib.SIGNATURES and hasattr(lib, name), name
    assert "typedef struct lgcn_mf lgcn_mf;" in bare
    body = re.search(r"typedef struct \{([^}]*)\} lgcn_mf_config;", bare).group(1)
    fields = [f for decl in body.split(";") if decl.strip() for f in re.findall(r"\*?\s*([A-Za-z_0-9]+)\s*(?:,|$)", decl.split(None, 1)[1])]
    assert fields == MF_CONFIG_FIELDS == [n for n, _ in pkg._lib.MfConfig._fields_]
    with open(os.path.join(REPO, PKG_NAME, "csrc", "lgcn_device.hip"), "rb") as f:
        import hashlib
        assert hashlib.sha256(f.read()).hexdigest() == pkg.build.kernel_hash()
    assert any(s.endswith("lgcn_mf.hip") for s in pkg.build.SOURCES)

    # argument checks that touch no device: rc 3, nothing launched, nothing written
    assert lib.lgcn_mf_create(None, None) == 3
    assert lib.lgcn_mf_get_step(None) == -1 and lib.lgcn_mf_check(None, None) == 3
    assert lib.lgcn_mf_train_step(None, None, None, None, 4, None, None) == 3
    assert lib.lgcn_mf_train_epoch(None, None, None, None, 100, 4, None, None) == 3

    def cfg(**kw):
        c = pkg._lib.MfConfig()
        c.n_users, c.m_items, c.d, c.max_batch = 37, 94, 64, 8
        for f in ("E0", "adam_m", "adam_v", "G64", "bitmap", "terms", "err"):
            setattr(c, f, 4096)              # never dereferenced by the calls below
        c.decay, c.lr, c.beta1, c.beta2, c.eps = 1e-4, 1e-3, 0.9, 0.999, 1e-8
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    h = C.c_void_p()
    for bad in ({"d": 48}, {"d": 0}, {"d": 512}, {"n_users": 2 ** 30, "m_items": 2 ** 30}, {"n_users": 2 ** 31 - 1, "m_items": 1},
                {"n_users": 0}, {"m_items": 0}, {"max_batch": 0}, {"E0": None}, {"adam_m": None}, {"adam_v": None}, {"G64": None},
                {"bitmap": None}, {"terms": None}, {"err": None}):
        assert lib.lgcn_mf_create(C.byref(cfg(**bad)), C.byref(h)) == 3 and not h.value, bad
        assert lib.lgcn_last_error().startswith(b"lgcn_mf_create")
    assert lib.lgcn_mf_create(C.byref(cfg()), None) == 3
    assert lib.lgcn_mf_create(C.byref(cfg()), C.byref(h)) == 0 and h.value
    try:
        assert lib.lgcn_mf_get_step(h) == 0
        lib.lgcn_mf_set_step(h, 41)
        assert lib.lgcn_mf_get_step(h) == 41
        ids = C.c_void_p(4096)
        for B in (0, -1, 9, 2 ** 31 - 1):
            assert lib.lgcn_mf_train_step(h, ids, ids, ids, B, ids, None) == 3
            assert lib.lgcn_mf_train_epoch(h, ids, ids, ids, 100, B, ids, None) == 3
        for hole in range(4):
            a = [ids, ids, ids, ids]
            a[hole] = None
            assert lib.lgcn_mf_train_step(h, a[0], a[1], a[2], 4, a[3], None) == 3
            assert lib.lgcn_mf_train_epoch(h, a[0], a[1], a[2], 100, 4, a[3], None) == 3
        assert lib.lgcn_mf_get_step(h) == 41                 # a refused call is no step
    finally:
        lib.lgcn_mf_destroy(h)


def test_eval_seed_is_decided_in_fp32(pkg, tmp_path):
    """The seed tests/test_gpu_mf.py evaluates with: on its N(0, 1) table no test item of any user lies within 2 b of that
    user's 20th best score, nor of any other candidate's score, so every metric of the fp32 kernels must equal the float64 one."""
    try:
        ds, m = mf_model(pkg, tmp_path, seed=EVAL_SEED)
        users, train, test = eval_lists(ds)
        mg = eval_margins(m._table.numpy(), ds.n_users, users, train, test)
        assert len(users) > 0 and (mg > 0).all(), (mg.min(0), np.argwhere(mg <= 0)[:4].tolist())
        r = eval_metrics64(m._table.numpy(), ds.n_users, ds.m_items, users, train, test)
        assert 0.0 < r["recall"] < 1.0 and 0.0 < r["auc"] < 1.0 and 0.0 < r["mrr"] <= 1.0
        # the AUC restatement is utils.AUC's
        u0 = int(users[0])
        sc = m._table.double().numpy()[u0] @ m._table.double().numpy()[ds.n_users:].T
        sc[train[u0]] = -1024.0
        one = eval_metrics64(m._table.numpy(), ds.n_users, ds.m_items, users[:1], train, test[:1])
        assert abs(one["auc"] - pkg.utils.AUC(sc, ds, test[0].tolist())) < 1e-12
    finally:
        pkg.world.configure([])


BOUND_DIMS = (32, 64, 128, 256)
BOUND_BATCHES = (1, 5, 65, 300, 2049)


def test_bounds_hold_the_fp32_oracle(oracle):
    """At every shape the fp32 oracle (oracle.bpr on the table itself) must lie inside the bounds the GPU tests use, measured
    against the float64 restatement; the shares used are printed."""
    n_users, m_items, decay = 37, 94, 1e-4
    worst = {"G": 0.0, "bpr": 0.0, "reg": 0.0}
    for d in BOUND_DIMS:
        for B in BOUND_BATCHES:
            for scale in (0.1, 1.0):
                for seed in range(4):
                    rng = np.random.default_rng(1000 * seed + d + B)
                    E = (scale * rng.standard_normal((n_users + m_items, d))).astype(np.float32)
                    u, p, n = mf_batch(rng, n_users, m_items, B)
                    ref = mf_ref64(E, n_users, u, p, n, decay)
                    bpr, reg, G = oracle.bpr(E, n_users, u, p, n, decay)
                    share = {"G": float((np.abs(G.astype(np.float64) - ref["G"]) / ref["G_bound"]).max()),
                             "bpr": abs(bpr - ref["bpr"]) / ref["bpr_bound"], "reg": abs(reg - ref["reg"]) / ref["reg_bound"]}
                    for k in worst:
                        worst[k] = max(worst[k], share[k])
                        assert share[k] < 1.0, (k, d, B, scale, seed, share[k])
                    assert (G[~ref["named"]] == 0).all()
    print("largest share of the bound the fp32 oracle uses:", worst)

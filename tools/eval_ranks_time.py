#!/usr/bin/env python3
"""GPU: the rank-based evaluation on Gowalla (29 858 test users x 40 981 items, d = 64, HIP events, mean of 10 calls).
  * lgcn_eval_ranks and lgcn_eval_rank_metrics, with the slots in dataset order and ordered by test-list length;
  * beside them, in the same process, lgcn_eval_topk_ex at K = 20 and K = 256 (train-positive masks on);
  * the only other way to the same quantities without the rank kernels: a chunked argsort of the masked score matrix in torch,
    the test items' positions gathered from the inverse permutation;
  * a whole Procedure.Test at --topks "[20,1000]" with --rank_metrics on and off (off: the torch harness, 1000 > 256).
One JSON line.
    python tools/eval_ranks_time.py [--kernels-only]       (LGCN_LIB_PATH selects a build variant: -DEVAL_RANKS_PARTS=n,
                                                            -DEVAL_RANKS_TB=n through tools/build_variants.py)"""
import contextlib, importlib, io, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
import bench

kernels_only = "--kernels-only" in sys.argv
sys.argv = [sys.argv[0]]
pkg = importlib.import_module(bench.PKG)
L, lib = pkg._lib, pkg._lib.load()
w = pkg.world
w.configure(["--tensorboard", "0", "--checkpoint_dir", "/tmp/lgcn_eval_ranks_ckpt"])
dev = torch.device("cuda", 0)


def kernel_ms(fn, reps=10):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / reps, 4)


out = {"lib": os.path.basename(L._build.LIB_PATH)}
data = bench.materialize_gowalla(bench.GOWALLA_NPZ, "/tmp/lgcn_bench_data/gowalla_r0")
with contextlib.redirect_stdout(io.StringIO()):
    ds = pkg.dataloader.Loader(w.config, path=data)
    pkg.utils.set_seed(2020)
    m = pkg.model.LightGCN(w.config, ds).to(dev)
    m.eval()
    w.topks = [20]
    pkg.Procedure.Test(ds, m, 0)                           # builds the evaluation index (and its masks) once
ev = ds._lgcn_eval_index
with torch.no_grad():
    E = m.rating_table()
n, n_users, m_items, d = len(ev.users), m.n_users, m.m_items, m.latent_dim
lens = ev.test_len
out["shape"] = {"users": n, "items": m_items, "d": d, "test_items": int(lens.sum()), "longest_list": int(lens.max()),
                "lists_over_64": int((lens > 64).sum())}


def ordered(perm):
    """The evaluation slots in the order perm: (users32, test_ptr, test_sorted32)."""
    ptr = ev.test_ptr.cpu().numpy()
    items = ev.test_sorted32.cpu().numpy()
    ptr2 = np.zeros(n + 1, np.int64)
    np.cumsum(lens[perm], out=ptr2[1:])
    items2 = np.concatenate([items[ptr[s]:ptr[s + 1]] for s in perm.tolist()]) if n else items
    return (ev.users32[torch.from_numpy(perm).to(dev)].contiguous(), torch.from_numpy(ptr2).to(dev), torch.from_numpy(items2).to(dev))


ks = [20, 1000]
res = {}
for name, perm in (("dataset order", np.arange(n)), ("by list length", np.argsort(-lens, kind="stable"))):
    users32, tptr, tidx = ordered(perm)
    nt = int(tidx.numel())
    sc = torch.empty(nt, dtype=torch.float32, device=dev)
    gt = torch.empty(nt, dtype=torch.int32, device=dev)
    eq = torch.empty(nt, dtype=torch.int32, device=dev)
    row = {"lgcn_eval_ranks_ms": kernel_ms(lambda: L.eval_ranks(E, n_users, users32, ev.train_ptr, ev.train_idx32, tptr, tidx, sc, gt, eq)),
           "lgcn_eval_ranks_fp32_ms": kernel_ms(lambda: L.eval_ranks(E, n_users, users32, ev.train_ptr, ev.train_idx32, tptr, tidx, sc, gt, eq, fp32=True))}
    L.eval_ranks(E, n_users, users32, ev.train_ptr, ev.train_idx32, tptr, tidx, sc, gt, eq)
    row["lgcn_eval_rank_metrics_ms"] = kernel_ms(lambda: L.eval_rank_metrics(m_items, users32, ev.train_ptr, ev.train_idx32, tptr, tidx, sc, gt, eq, ks))
    _, sums = L.eval_rank_metrics(m_items, users32, ev.train_ptr, ev.train_idx32, tptr, tidx, sc, gt, eq, ks)
    row["means"] = [float(x) / n for x in sums.cpu().numpy()]
    row["TFLOP/s"] = round(2.0 * n * m_items * d / (row["lgcn_eval_ranks_ms"] * 1e-3) / 1e12, 2)
    res[name] = row
out["ranks"] = res
for K in (20, 256):
    topk = torch.empty(n, K, dtype=torch.int32, device=dev)
    out[f"lgcn_eval_topk_ex_K{K}_ms"] = kernel_ms(lambda: L.eval_topk(E, n_users, ev.users32, ev.train_ptr, ev.train_idx32, K, topk, masks=ev.masks))

if not kernels_only:
    def torch_argsort():
        """Positions of the test items from a full argsort of every masked row, 2048 users at a time."""
        users = torch.from_numpy(ev.users).to(dev)
        pos = []
        for s in range(0, n, 2048):
            rows = torch.arange(s, min(s + 2048, n), device=dev)
            rating = E[users[rows]] @ E[n_users:].t()
            ex_row, ex_pos = ev._expand(ev.train_ptr, users[rows])
            rating[ex_row, ev.train_idx[ex_pos]] = -(1 << 10)
            order = torch.argsort(rating, dim=1, descending=True)
            place = torch.empty_like(order)
            place.scatter_(1, order, torch.arange(m_items, device=dev).expand_as(order))
            gt_row, gt_pos = ev._expand(ev.test_ptr, rows)
            pos.append(place[gt_row, ev.test_idx[gt_pos]])
        return torch.cat(pos)
    with torch.no_grad():
        out["torch_chunked_argsort_ms"] = kernel_ms(torch_argsort, reps=3)
    tests = {}
    w.topks = ks
    for flag in (1, 0):
        w.config['rank_metrics'] = flag
        with contextlib.redirect_stdout(io.StringIO()):
            pkg.Procedure.Test(ds, m, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                r = pkg.Procedure.Test(ds, m, 0)
            torch.cuda.synchronize()
        tests["rank_metrics_ms" if flag else "torch_harness_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
        tests["result_rank" if flag else "result_torch"] = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in r.items()}
    w.config['rank_metrics'] = 0
    out["Procedure.Test [20,1000]"] = tests
print(json.dumps(out))

#!/usr/bin/env python3
"""GPU: the fused evaluation past K = 64.  On Gowalla (29 858 test users x 40 981 items, d = 64): kernel time and fp32-equivalent
TFLOP/s (2 * users * items * d / time) of lgcn_eval_topk_ex (train-positive masks, as Procedure.Test runs it) at
K in {20, 64, 65, 100, 128, 200, 256}, lgcn_eval_topk at K = 20 beside it, and one whole Procedure.Test at --topks [20],
[20,50,100] and [20,100,200], fused and with eval_fused=0, in the same process.  Then one synthetic shape past the 16-bit
list ids (300 000 items).  One JSON line.
    python tools/eval_large_k.py [--kernels-only]       (LGCN_LIB_PATH selects a build variant)"""
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
w.configure(["--tensorboard", "0", "--checkpoint_dir", "/tmp/lgcn_eval_large_k_ckpt"])
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
    return e0.elapsed_time(e1) / reps


def sweep(E, n_users, users, ptr, idx, masks, Ks):
    n, m_items, d = int(users.numel()), int(E.shape[0]) - n_users, int(E.shape[1])
    res = {}
    for K in Ks:
        topk = torch.empty(n, K, dtype=torch.int32, device=dev)
        ms = kernel_ms(lambda: L.eval_topk(E, n_users, users, ptr, idx, K, topk, masks=masks))
        res[str(K)] = {"ms": round(ms, 4), "TFLOP/s": round(2.0 * n * m_items * d / (ms * 1e-3) / 1e12, 2)}
    return res


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
g = {"users": len(ev.users), "items": m.m_items, "d": m.latent_dim}
g["lgcn_eval_topk_ex"] = sweep(E, m.n_users, ev.users32, ev.train_ptr, ev.train_idx32, ev.masks, (20, 64, 65, 100, 128, 200, 256))
topk20 = torch.empty(len(ev.users), 20, dtype=torch.int32, device=dev)
ms = kernel_ms(lambda: L.check(lib.lgcn_eval_topk(L.tp(E), m.n_users, m.m_items, m.latent_dim, L.tp(ev.users32), len(ev.users),
                                                  L.tp(ev.train_ptr), L.tp(ev.train_idx32), 20, L.tp(topk20), None,
                                                  L.current_stream()), "lgcn_eval_topk"))
g["lgcn_eval_topk_K20_ms"] = round(ms, 4)
if not kernels_only:
    tests = {}
    for topks in ([20], [20, 50, 100], [20, 100, 200]):
        row = {}
        for fused in (1, 0):
            w.topks = topks
            w.config['eval_fused'] = fused
            with contextlib.redirect_stdout(io.StringIO()):
                pkg.Procedure.Test(ds, m, 0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    r = pkg.Procedure.Test(ds, m, 0)
                torch.cuda.synchronize()
            row["fused_ms" if fused else "torch_ms"] = round((time.perf_counter() - t0) / 5 * 1e3, 3)
            row["recall_fused" if fused else "recall_torch"] = [float(x) for x in r["recall"]]
        row["speedup"] = round(row["torch_ms"] / row["fused_ms"], 2)
        tests[str(topks)] = row
    w.config['eval_fused'] = 1
    g["Procedure.Test"] = tests
out["gowalla"] = g

# past the 16-bit list ids: 300 000 items (per part more than 2047 tiles -> int32 ids, fp32 matrix instructions)
nu, mi, d = 20000, 300000, 64
gen = torch.Generator(device=dev); gen.manual_seed(1)
Es = torch.randn(nu + mi, d, device=dev, generator=gen) * 0.1
rng = np.random.Generator(np.random.PCG64(3))
deg = rng.integers(5, 90, nu)
ptr = np.zeros(nu + 1, np.int64); ptr[1:] = np.cumsum(deg)
idx = np.concatenate([np.sort(rng.choice(mi, size=int(k), replace=False)) for k in deg]).astype(np.int32)
users = torch.arange(nu, dtype=torch.int32, device=dev)
d_ptr, d_idx = torch.from_numpy(ptr).to(dev), torch.from_numpy(idx).to(dev)
masks = torch.empty(int(lib.lgcn_eval_mask_words(mi, nu)), dtype=torch.int32, device=dev)
L.check(lib.lgcn_eval_build_masks(L.tp(users), nu, L.tp(d_ptr), L.tp(d_idx), mi, L.tp(masks), L.current_stream()), "masks")
out["synthetic"] = {"users": nu, "items": mi, "d": d,
                    "lgcn_eval_topk_ex": sweep(Es, nu, users, d_ptr, d_idx, masks, (20, 100, 256))}
print(json.dumps(out))

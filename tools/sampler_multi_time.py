#!/usr/bin/env python3
"""GPU: the sampler for several negatives per positive, device against host, end to end (DESIGN 4 *Sampler*).

  sampler (default)   one call each way, timed on the host clock around work that ends in a device synchronise:
                        device = sampling.sample_negative_device(..., neg_num=R): the block histories on the host and their
                                 upload, the stream expansion, the segment kernels, the read-back of the result;
                        host   = sampling.sample_negative(..., R) + the upload of its [T, 2 + R] int32 rows.
                      Gowalla at --ratios (default 1,2,4,8,16), the Yelp2018-shaped graph at R = 4 (--big: the 10 M x 1 M
                      graph at R = 4 instead).  min / median / max of --reps runs (one untimed run first).
  --epoch             a whole Gowalla epoch through Procedure.BPR_train_original (K = 3, d = 64, B = 2048, --neg_ratio 4) with
                      --prefetch_epoch 0 and 1, the rows from the device (--gpu_sampler 1) and from the host loop (0: the only
                      path before the device sampler took R > 1); the four configurations interleaved over --reps rounds.
Prints one JSON line and, with --out, writes it there."""
import argparse
import contextlib
import importlib
import io
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
ap = argparse.ArgumentParser()
ap.add_argument("--ratios", default="1,2,4,8,16")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--big", action="store_true")
ap.add_argument("--epoch", action="store_true")
ap.add_argument("--no-host", action="store_true", help="device calls only (for a kernel trace)")
ap.add_argument("--out", default="")
ap.add_argument("--tmp", default="/tmp/lgcn_sampler_multi_time")
a = ap.parse_args()
sys.argv = [sys.argv[0]]                                 # world parses sys.argv on import: this tool's flags are not the package's
import torch                                             # noqa: E402
import bench                                             # noqa: E402

pkg = importlib.import_module(bench.PKG)
w = pkg.world
dev = torch.device("cuda", 0)


def summary(ms):
    return {"min": min(ms), "median": statistics.median(ms), "max": max(ms), "n": len(ms)}


def time_sampler(ds, R, reps):
    S = pkg.sampling
    csr = ds.pos_csr()
    shape = (ds.n_users, ds.m_items, ds.trainDataSize)
    S.seed(2020)
    res = {"samples": int(ds.n_users * (ds.trainDataSize // ds.n_users))}
    dev_ms, host_ms, loop_ms = [], [], []
    for i in range(reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        S.sample_negative_device(*shape, csr, dev, neg_num=R)
        torch.cuda.synchronize()
        dev_ms.append((time.perf_counter() - t0) * 1e3)
    res["device_ms"] = summary(dev_ms[1:])
    if R == 1:                                               # neg_num = 1 above is the three-slot entry point; the slot kernels at W = 2:
        slot_ms = []
        for i in range(reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            S.sample_negative_device_multi(*shape, csr, dev, 1)
            torch.cuda.synchronize()
            slot_ms.append((time.perf_counter() - t0) * 1e3)
        res["device_slot_kernels_ms"] = summary(slot_ms[1:])
    if not a.no_host:
        for i in range(reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            rows = S.sample_negative(*shape, csr, R)
            t1 = time.perf_counter()
            torch.from_numpy(rows).to(dev)
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3); loop_ms.append((t1 - t0) * 1e3)
        res["host_ms"] = summary(host_ms[1:]); res["host_loop_ms"] = summary(loop_ms[1:])
        res["upload_MB"] = rows.nbytes / 1e6
    return res


def sampler():
    w.configure(["--tensorboard", "0", "--checkpoint_dir", os.path.join(a.tmp, "ckpt")])
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        if a.big:
            sets = [("synthetic-10m", bench.synthetic_dataset(pkg, "synthetic-10m", w.config, dev), [4])]
        else:
            d = bench.materialize_gowalla(bench.GOWALLA_NPZ, os.path.join(a.tmp, "gowalla"))
            sets = [("gowalla", pkg.dataloader.Loader(w.config, path=d), [int(x) for x in a.ratios.split(",")])]
            if not a.no_host:
                sets.append(("yelp2018-shaped", bench.synthetic_dataset(pkg, "yelp2018-shaped", w.config, dev), [4]))
    for name, ds, ratios in sets:
        for R in ratios:
            out[f"{name} R{R}"] = time_sampler(ds, R, 2 if a.big else a.reps)
            print(f"{name} R{R}: {json.dumps(out[f'{name} R{R}'])}", flush=True)
    return out


def epoch():
    R, B = 4, 2048
    d = bench.materialize_gowalla(bench.GOWALLA_NPZ, os.path.join(a.tmp, "gowalla"))
    cfgs = [(pre, gpu) for pre in (0, 1) for gpu in (1, 0)]
    w.configure(["--dataset", "gowalla", "--tensorboard", "0", "--layer", "3", "--recdim", "64", "--bpr_batch", str(B), "--row_order", "xcd",
                 "--sampler", "cpp", "--neg_ratio", str(R), "--checkpoint_dir", os.path.join(a.tmp, "ckpt")])
    w.tensorboard = 0
    with contextlib.redirect_stdout(io.StringIO()):
        sets = {c: pkg.dataloader.Loader(w.config, path=d) for c in cfgs}
        m = pkg.model.LightGCN(w.config, sets[cfgs[0]]).to(w.device)
    bpr = pkg.utils.BPRLoss(m, w.config)
    pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
    ms = {c: [] for c in cfgs}
    for rnd in range(a.reps + 1):
        for c in cfgs:
            w.config['prefetch_epoch'], w.config['gpu_sampler'] = c
            for e in range(3):                               # the first epoch of a visit fills the prefetch: not timed
                torch.cuda.synchronize(); t0 = time.perf_counter()
                pkg.Procedure.BPR_train_original(sets[c], m, bpr, e)
                torch.cuda.synchronize()
                if rnd and e:
                    ms[c].append((time.perf_counter() - t0) * 1e3)
            sets[c]._lgcn_next_epoch = None                  # the next visit samples afresh
    return {f"prefetch_epoch {pre} gpu_sampler {gpu}": dict(summary(v), all=[round(x, 2) for x in v]) for (pre, gpu), v in ms.items()}


res = {"epoch_ms gowalla K=3 d=64 B=2048 neg_ratio=4": epoch()} if a.epoch else sampler()
print(json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)

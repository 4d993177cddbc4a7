#!/usr/bin/env python3
"""One Gowalla training run of --loss directau at one --au_gamma -- or, with --loss bpr, the BPR run of the same
length -- with the settings of profiles/inbatch/README.md (K = 3, d = 64, B = 2048, --reg_rows ego, seed 2020, fp32 storage, lr
1e-3, decay 1e-4, --sampler cpp): Procedure.BPR_train_original epochs, Procedure.Test at the marks; one JSON line per mark.  A
record for profiles/directau/README.md, not a gate.  In the shape of tools/inbatch_scores_quality.py."""
import argparse
import contextlib
import importlib
import io
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bench import materialize_gowalla, GOWALLA_NPZ  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--loss", default="directau", choices=["directau", "bpr"])
ap.add_argument("--gamma", type=float, default=1.0, help="--au_gamma")
ap.add_argument("--epochs", type=int, default=50)
ap.add_argument("--marks", default="10,50")
ap.add_argument("--act_dtype", default="fp32")
ap.add_argument("--tmp", default="/tmp/lgcn_directau_quality")
a = ap.parse_args()
sys.argv = [sys.argv[0]]
import torch  # noqa: E402

pkg = importlib.import_module("graph-and-sequential-recommendation-systems_amd")
w = pkg.world
w.configure(["--dataset", "gowalla", "--tensorboard", "0", "--act_dtype", a.act_dtype, "--reg_rows", "ego", "--sampler", "cpp",
             "--loss", a.loss, "--au_gamma", str(a.gamma), "--checkpoint_dir", os.path.join(a.tmp, "ckpt")])
d = materialize_gowalla(GOWALLA_NPZ, os.path.join(a.tmp, "gowalla"))
marks = sorted(int(x) for x in a.marks.split(","))
with contextlib.redirect_stdout(io.StringIO()):
    ds = pkg.dataloader.Loader(w.config, path=d)
    pkg.sampling.seed(w.seed); pkg.utils.set_seed(w.seed)
    model = pkg.model.LightGCN(w.config, ds).to(w.device)
    bpr = pkg.utils.BPRLoss(model, w.config)
t0 = time.time()
for e in range(1, a.epochs + 1):
    with contextlib.redirect_stdout(io.StringIO()):
        info = pkg.Procedure.BPR_train_original(ds, model, bpr, e)
    if e in marks:
        with contextlib.redirect_stdout(io.StringIO()):
            r = pkg.Procedure.Test(ds, model, e)
        torch.cuda.synchronize()
        print("RESULT " + json.dumps({"loss": a.loss, "gamma": a.gamma, "epoch": e, "info": info,
                                      "recall": float(r["recall"][0]), "ndcg": float(r["ndcg"][0]), "seconds": time.time() - t0}), flush=True)
model.check_device_errors()

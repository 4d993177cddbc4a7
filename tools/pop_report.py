#!/usr/bin/env python3
"""What the popularity knobs do to the head and the tail, and what --pop_metrics 1 costs.

Without --run / --time this is the driver: one child process per training configuration (Gowalla, K = 3, d = 64, B = 2048,
--reg_rows ego, seed 2020, fp32 storage, lr 1e-3, decay 1e-4, --sampler cpp: the settings of profiles/inbatch/README.md), each
training --epochs epochs and ending in one Procedure.Test with --pop_metrics 1 at --topks [20]; before them the timing children (a
Procedure.Test on Gowalla with the flag off in --parent's tree if given, with the flag off and on in this tree, alternating over
--rounds rounds; --rounds 0 and --prior keep the rows of an earlier call).  Writes <out>/pop_metrics.json and <out>/README.md.  One seed: a record, not a claim.

  --run NAME    one training configuration in this process, one RESULT line
  --time POP    one timing window in this process (POP = 0 | 1), one RESULT line; --tree picks the tree whose package is timed"""
import argparse
import contextlib
import importlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "graph-and-sequential-recommendation-systems_amd"
CONFIGS = {
    "bpr": ["--loss", "bpr"],
    "inbatch cosine": ["--loss", "inbatch", "--softmax_temp", "0.2", "--score", "cosine"],
    "inbatch cosine + logQ": ["--loss", "inbatch", "--softmax_temp", "0.2", "--score", "cosine", "--inbatch_logq", "1"],
    "directau (gamma 1)": ["--loss", "directau", "--au_gamma", "1"],
    # the gate is defined with the fork's own L2 term only (--reg_rows propagated), so it gets a baseline of its own
    "bpr, --reg_rows propagated": ["--loss", "bpr", "--reg_rows", "propagated"],
    "bpr, --reg_rows propagated, --use_pop_gate": ["--loss", "bpr", "--reg_rows", "propagated", "--use_pop_gate"],
}

ap = argparse.ArgumentParser()
ap.add_argument("--run", default=None, choices=sorted(CONFIGS))
ap.add_argument("--time", default=None, choices=["0", "1"])
ap.add_argument("--tree", default=HERE)
ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built: timed with the flag off")
ap.add_argument("--epochs", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tests", type=int, default=200, help="Procedure.Test calls per timing window")
ap.add_argument("--only", default=None, help="configuration names separated by ';' (default: all)")
ap.add_argument("--prior", default=None, help="a pop_metrics.json of an earlier call: its rows are kept for what this call does not run again")
ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pop_metrics"))
ap.add_argument("--tmp", default="/tmp/lgcn_pop_report")
a = ap.parse_args()
sys.argv = [sys.argv[0]]


def _setup(flags):
    sys.path.insert(0, a.tree)
    from bench import materialize_gowalla, GOWALLA_NPZ
    pkg = importlib.import_module(PKG)
    w = pkg.world
    w.configure(["--dataset", "gowalla", "--tensorboard", "0", "--act_dtype", "fp32", "--reg_rows", "ego", "--sampler", "cpp",
                 "--topks", "[20]", "--checkpoint_dir", os.path.join(a.tmp, "ckpt")] + flags)
    d = materialize_gowalla(GOWALLA_NPZ, os.path.join(a.tmp, "gowalla"))
    with contextlib.redirect_stdout(io.StringIO()):
        ds = pkg.dataloader.Loader(w.config, path=d)
        pkg.sampling.seed(w.seed); pkg.utils.set_seed(w.seed)
        model = pkg.model.LightGCN(w.config, ds).to(w.device)
    return pkg, w, ds, model


def run_one(name):
    import torch
    pkg, w, ds, model = _setup(CONFIGS[name] + ["--pop_metrics", "1", "--pop_groups", "[0.2]"])
    with contextlib.redirect_stdout(io.StringIO()):
        bpr = pkg.utils.BPRLoss(model, w.config)
    t0 = time.time()
    for e in range(1, a.epochs + 1):
        with contextlib.redirect_stdout(io.StringIO()):
            pkg.Procedure.BPR_train_original(ds, model, bpr, e)
    with contextlib.redirect_stdout(io.StringIO()):
        r = pkg.Procedure.Test(ds, model, a.epochs)
    torch.cuda.synchronize()
    model.check_device_errors()
    row = {"config": name, "flags": CONFIGS[name], "epochs": a.epochs, "seconds": time.time() - t0}
    for k, v in r.items():
        row[k] = v.tolist() if hasattr(v, "tolist") else v
    print("RESULT " + json.dumps(row), flush=True)


def time_one(pop):
    import torch
    pkg, w, ds, model = _setup(["--pop_metrics", str(pop)] if pop else [])
    model.eval()
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(10):
            pkg.Procedure.Test(ds, model, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.tests):
            pkg.Procedure.Test(ds, model, 0)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.tests * 1e3
        # the device side alone: the launches of _test_fused between two events (no host copy in between)
        ev = ds._lgcn_eval_index
        info = ev.item_info(ds) if pop else None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        args = (model, ev, 20, info) if pop else (model, ev, 20)
        for _ in range(5):
            pkg.Procedure._test_fused(*args)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(50):
            pkg.Procedure._test_fused(*args)
        e1.record(); torch.cuda.synchronize()
    print("RESULT " + json.dumps({"pop_metrics": pop, "tree": "this tree" if os.path.abspath(a.tree) == HERE else "parent", "ms_per_Test": ms, "ms_per_test_fused": e0.elapsed_time(e1) / 50,
                                  "tests": a.tests}), flush=True)


def child(args, tree=HERE):
    cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--epochs", str(a.epochs), "--tests", str(a.tests), "--tmp", a.tmp] + args
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    rows = [json.loads(l[7:]) for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    if out.returncode != 0 or not rows:
        sys.stderr.write(out.stdout[-4000:])
        raise SystemExit(f"child {args} failed (exit {out.returncode}): nothing more is started")
    return rows[0]


def spread(v):
    return f"{statistics.median(v):.3f} ({min(v):.3f}..{max(v):.3f})"


def driver():
    os.makedirs(a.out, exist_ok=True)
    names = [n for n in CONFIGS if a.only is None or n in a.only.split(";")]
    sides = ([("parent, flag off", a.parent, "0")] if a.parent else []) + [("this tree, flag off", HERE, "0"), ("this tree, flag on", HERE, "1")]
    timing = {s[0]: [] for s in sides}
    prior = json.load(open(a.prior)) if a.prior else {}
    if a.rounds == 0:
        timing = prior.get("timing", timing)
    for _ in range(a.rounds):                                # alternating: every side once per round
        for label, tree, pop in sides:
            timing[label].append(child(["--time", pop], tree))
            print(label, json.dumps(timing[label][-1]), flush=True)
    quality = [r for r in prior.get("quality", []) if r["config"] not in names]
    for n in names:
        quality.append(child(["--run", n]))
        print(json.dumps(quality[-1]), flush=True)
        with open(os.path.join(a.out, "pop_metrics.json"), "w") as f:       # (kept as it grows: a later child may fail)
            json.dump({"quality": quality, "timing": timing, "epochs": a.epochs}, f, indent=1)
    with open(os.path.join(a.out, "pop_metrics.json"), "w") as f:
        json.dump({"quality": quality, "timing": timing, "epochs": a.epochs, "rounds": max(len(v) for v in timing.values()), "tests_per_window": a.tests}, f, indent=1)
    L = ["# `--pop_metrics 1`: what the lists hold (DESIGN §4.27)", "",
         f"Written by `python tools/pop_report.py --parent <checkout of the parent commit> --epochs {a.epochs}`; raw numbers in `pop_metrics.json`. One MI355X (gfx950).", "",
         "## Head and tail at `[20]` (one seed: a record, not a claim)", "",
         f"Gowalla, K = 3, d = 64, B = 2048, `--reg_rows ego`, seed 2020, fp32 storage, lr 1e-3, decay 1e-4, `--sampler cpp`, {a.epochs} epochs, "
         "one process per run; `--pop_groups \"[0.2]\"`: head = the 20 % most popular items by train interactions, tail = the other 80 %. "
         "`share` = the group's part of Recall@20 (the two sum to it), `in group` = recall on the group's own test items, `list` = the group's "
         "part of the recommended entries, ARP = mean train popularity of a recommended item.", "",
         "| run | Recall@20 | NDCG@20 | share head | share tail | in group head | in group tail | list head | list tail | ARP | coverage | Gini |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in quality:
        L.append(f"| {r['config']} | {r['recall'][0]:.4f} | {r['ndcg'][0]:.4f} | {r['recall_share'][0][0]:.4f} | {r['recall_share'][1][0]:.4f} | "
                 f"{r['recall_by_group'][0][0]:.4f} | {r['recall_by_group'][1][0]:.4f} | {r['list_share'][0][0]:.4f} | {r['list_share'][1][0]:.4f} | "
                 f"{r['arp'][0]:.1f} | {r['coverage'][0]:.4f} | {r['gini'][0]:.4f} |")
    L += ["", "## What the flag costs", "",
          f"`Procedure.Test` on Gowalla (29 858 evaluated users, 40 981 items, `--topks [20]`, random-init table), one process per window, the sides "
          f"alternating over {max(len(v) for v in timing.values())} rounds; a window is 10 warm-up calls and then {a.tests} calls between two host clocks ending in a device "
          "synchronise (`Test` itself reads its sums back, so every call is complete). `_test_fused` = its launches alone, 50 calls between two "
          "device events. Median (min..max) of the rounds, in ms.", "",
          "| side | `Procedure.Test` | `_test_fused` launches |", "|---|---|---|"]
    for label, rows in timing.items():
        L.append(f"| {label} | {spread([r['ms_per_Test'] for r in rows])} | {spread([r['ms_per_test_fused'] for r in rows])} |")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(L) + "\n")
    print("wrote", a.out)


if a.run:
    run_one(a.run)
elif a.time is not None:
    time_one(int(a.time))
else:
    driver()

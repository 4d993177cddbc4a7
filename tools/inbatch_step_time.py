#!/usr/bin/env python3
"""Step time of the in-batch sampled softmax (--loss inbatch) against the sampled softmax at one negative per
positive (--loss softmax --neg_ratio 1), whose path the in-batch loss does not touch: Gowalla, K = 3, d = 64,
B = 2048 samples per step, fp32 and bf16 storage, the same sampled and shuffled (u, p) rows on both sides -- steps/s of the
one-C-call epochs
  (a) softmax   lgcn_train_epoch_multi at R = 1 under lgcn_ctx_set_loss(LGCN_LOSS_SOFTMAX, tau) -- the baseline;
  (b) inbatch   lgcn_train_epoch_inbatch under lgcn_ctx_set_loss(LGCN_LOSS_INBATCH, tau): the negatives are not read;
and the per-launch device times of one epoch of each form (torch.profiler's kernel records, summed by kernel name: the four
k_inbatch_* launches, the batch-row launch of the baseline, the SpMM layers and the rest).

Driver (default): one CHILD PROCESS per configuration, each under its own time limit, the two forms alternating inside every
storage and over --rounds rounds, so that a drift of the machine does not land on one of them; stops at the first child that
fails.  A child runs in a session of its own, and at its time limit the whole process group is killed.  Results: a JSON file
under --out.

Child (--one): builds the model, samples one epoch with the host sampler, runs one warm-up epoch, then times --repeats windows
of --epochs epochs each (host clock around work that ends in a device synchronise), then profiles one more epoch, and prints
one JSON line."""
import argparse
import contextlib
import importlib
import io
import json
import os
import signal
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 2048
FORMS = ("softmax", "inbatch")


def kernel_times(fn, steps):
    """{kernel name (template arguments cut): microseconds per step} of the device kernels fn() launches."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA"):          # a record of the device's own timeline: a kernel or a copy
            name = ev.name.split("<")[0].split("(")[0].replace("void ", "")
            out[name] = out.get(name, 0.0) + ev.time_range.elapsed_us() / steps
    return out


def child(a):
    sys.path.insert(0, REPO)
    sys.argv = [sys.argv[0]]                                 # world parses sys.argv on import: this tool's flags are not the package's
    from bench import materialize_gowalla, GOWALLA_NPZ
    import torch
    pkg = importlib.import_module("graph-and-sequential-recommendation-systems_amd")
    w, L = pkg.world, pkg._lib
    args = ["--dataset", "gowalla", "--tensorboard", "0", "--layer", "3", "--recdim", "64", "--bpr_batch", str(B), "--act_dtype", a.act,
            "--row_order", "xcd", "--sampler", "cpp", "--neg_ratio", "1", "--dense_last", "1", "--loss", a.form, "--softmax_temp", str(a.temp)]
    w.configure(args)
    d = materialize_gowalla(a.npz or GOWALLA_NPZ, os.path.join(a.tmp, "gowalla"))
    with contextlib.redirect_stdout(io.StringIO()):
        ds = pkg.dataloader.Loader(w.config, path=d)
        pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
        w.config['gpu_sampler'] = 0                          # the host sampler: the same rows in both forms
        u, p, neg = pkg.Procedure.sample_epoch_to_device(ds, w.device)
        m = pkg.model.LightGCN(w.config, ds).to(w.device)
    steps = len(u) // B
    if a.max_steps:
        steps = min(steps, a.max_steps)
    T = steps * B
    u, p, neg = u[:T].contiguous(), p[:T].contiguous(), neg.reshape(-1)[:T].contiguous()
    st = m._state(max_batch=B, need_ctx=True)
    lib = L.load()
    assert st['dense_last'] and lib.lgcn_ctx_get_loss(st['ctx'], None) == (L.LOSS_INBATCH if a.form == "inbatch" else L.LOSS_SOFTMAX)
    losses = torch.empty(steps, 3, dtype=torch.float32, device=u.device)

    def epoch():
        if a.form == "inbatch":
            L.check(lib.lgcn_train_epoch_inbatch(st['ctx'], L.tp(u), L.tp(p), T, B, L.tp(losses), L.current_stream()), "lgcn_train_epoch_inbatch")
        else:
            L.check(lib.lgcn_train_epoch_multi(st['ctx'], L.tp(u), L.tp(p), L.tp(neg), 1, T, B, L.tp(losses), L.current_stream()), "lgcn_train_epoch_multi")

    epoch()                                                  # warm-up: every kernel of the timed window has run
    torch.cuda.synchronize()
    first = float(losses[0, 0])
    rates = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        for _ in range(a.epochs):
            epoch()
        torch.cuda.synchronize()
        rates.append(a.epochs * steps / (time.perf_counter() - t0))
    m.check_device_errors()
    launches = kernel_times(epoch, steps)
    print("RESULT " + json.dumps({"form": a.form, "act": a.act, "temp": a.temp, "steps_per_window": a.epochs * steps, "steps_per_s": rates,
                                  "first_loss": first, "last_loss": float(losses[-1, 0]), "launch_us_per_step": launches}))


def run_child(form, act, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--one", "--form", form, "--act", act, "--temp", str(a.temp),
           "--repeats", str(a.repeats), "--epochs", str(a.epochs), "--max-steps", str(a.max_steps), "--tmp", a.tmp, "--npz", a.npz]
    p = subprocess.Popen(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = p.communicate(timeout=a.child_timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        out, _ = p.communicate()
        sys.stderr.write(out[-4000:])
        raise SystemExit(f"child timed out after {a.child_timeout} s, process group killed: {' '.join(cmd)}")
    if p.returncode != 0:
        sys.stderr.write(out[-4000:])
        raise SystemExit(f"child failed (rc {p.returncode}): {' '.join(cmd)}")
    for line in out.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit("child printed no result: " + out[-2000:])


def summary(rates):
    return {"median": statistics.median(rates), "min": min(rates), "max": max(rates), "n": len(rates)}


def driver(a):
    sys.path.insert(0, REPO)
    from bench import GOWALLA_NPZ
    a.npz = a.npz or GOWALLA_NPZ
    os.makedirs(a.out, exist_ok=True)
    rates, info = {}, {}
    for rnd in range(a.rounds):
        for act in a.acts.split(","):
            for form in FORMS:
                res = run_child(form, act, a)
                key = f"{act} {form}"
                rates.setdefault(key, []).extend(res["steps_per_s"])
                info[key] = {"first_loss": res["first_loss"], "last_loss": res["last_loss"], "launch_us_per_step": res["launch_us_per_step"]}
                print(f"round {rnd} {key}: " + " ".join(f"{x:.0f}" for x in res["steps_per_s"]), flush=True)
    out = {"workload": f"gowalla K=3 d=64 dense_last=1, {B} samples per step, lgcn_train_epoch_multi (R = 1, softmax) / lgcn_train_epoch_inbatch, steps/s",
           "temperature": a.temp, "rounds": a.rounds, "repeats": a.repeats, "epochs_per_window": a.epochs,
           "configs": {k: dict(summary(v), all=v, **info[k]) for k, v in rates.items()}}
    out["pairs"] = {}
    us = lambda r: 1e6 / r                                   # microseconds per step
    for act in a.acts.split(","):
        cs, ci = out["configs"][f"{act} softmax"], out["configs"][f"{act} inbatch"]
        out["pairs"][act] = {
            "inbatch/softmax": ci["median"] / cs["median"],
            "t_softmax_us": us(cs["median"]), "t_inbatch_us": us(ci["median"]),
            "spread_us": max(us(cs["min"]) - us(cs["max"]), us(ci["min"]) - us(ci["max"]))}
    with open(os.path.join(a.out, "inbatch_step_time.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "all"} for k, v in out["configs"].items()}, indent=1))
    print(json.dumps(out["pairs"], indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true", help="child: measure one configuration in this process")
    ap.add_argument("--form", default="inbatch", choices=FORMS)
    ap.add_argument("--act", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--acts", default="fp32,bf16")
    ap.add_argument("--temp", type=float, default=0.2, help="temperature of both forms")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=2, help="epochs (395 steps each) per timed window")
    ap.add_argument("--max-steps", type=int, default=0, help="cut the epoch to this many steps")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds each child may take")
    ap.add_argument("--npz", default="", help="Gowalla interaction lists (default: tests/golden/gowalla/gowalla.npz of this tree)")
    ap.add_argument("--tmp", default="/tmp/lgcn_inbatch_time")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "inbatch"))
    a = ap.parse_args()
    child(a) if a.one else driver(a)

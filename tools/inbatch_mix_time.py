#!/usr/bin/env python3
"""Step time of the in-batch sampled softmax with mixed negative sampling (--inbatch_mix 1 at --neg_ratio 1, 4, 16)
beside the plain in-batch step and --loss softmax --neg_ratio 16: Gowalla, K = 3, d = 64, B = 2048 samples per step, fp32 and bf16
storage -- steps/s of the one-C-call epoch (lgcn_train_epoch_inbatch_mix / _inbatch / _multi) and the per-launch device times of
one epoch (torch.profiler's kernel records, summed by kernel name).  In the manner of tools/inbatch_scores_time.py; a sibling
because the forms differ in the entry point and in the sampled rows (R negatives per positive).

The form `plain` needs nothing this tool's tree adds beyond the flags of DESIGN 4.20, so the same file run from a checkout of
the parent commit (python tools/inbatch_mix_time.py --forms plain, copied there) times the parent's step: the mix-off
comparison of profiles/inbatch_mix/README.md.

Driver (default): one CHILD PROCESS per configuration, each under its own time limit, the forms alternating inside every storage
and over --rounds rounds; stops at the first child that fails.  Child (--one): builds the model, samples one epoch with the host
sampler (neg_num = R), runs one warm-up epoch, times --repeats windows of --epochs epochs each, profiles one more epoch, and
prints one JSON line."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
B = 2048
FORMS = ("plain", "mix1", "mix4", "mix16", "softmax16")


def child(a):
    from inbatch_step_time import kernel_times
    sys.path.insert(0, REPO)
    sys.argv = [sys.argv[0]]                                 # world parses sys.argv on import: this tool's flags are not the package's
    from bench import materialize_gowalla, GOWALLA_NPZ
    import torch
    pkg = importlib.import_module("graph-and-sequential-recommendation-systems_amd")
    w, L = pkg.world, pkg._lib
    mix = a.form.startswith("mix")
    R = int(a.form[3:]) if mix else (int(a.form[7:]) if a.form.startswith("softmax") else 1)
    args = ["--dataset", "gowalla", "--tensorboard", "0", "--layer", "3", "--recdim", "64", "--bpr_batch", str(B), "--act_dtype", a.act,
            "--row_order", "xcd", "--sampler", "cpp", "--neg_ratio", str(R), "--dense_last", "1", "--softmax_temp", str(a.temp)]
    if a.form.startswith("softmax"):
        args += ["--loss", "softmax"]
    else:
        args += ["--loss", "inbatch", "--score", a.opts.split("+")[0], "--inbatch_logq", str(int(a.opts.endswith("+logq")))]
        if mix:
            args += ["--inbatch_mix", "1"]
    w.configure(args)
    d = materialize_gowalla(a.npz or GOWALLA_NPZ, os.path.join(a.tmp, "gowalla"))
    with contextlib.redirect_stdout(io.StringIO()):
        ds = pkg.dataloader.Loader(w.config, path=d)
        pkg.sampling.seed(2020); pkg.utils.set_seed(2020)
        w.config['gpu_sampler'] = 0                          # the host sampler
        u, p, n = pkg.Procedure.sample_epoch_to_device(ds, w.device)
        m = pkg.model.LightGCN(w.config, ds).to(w.device)
    steps = len(u) // B
    if a.max_steps:
        steps = min(steps, a.max_steps)
    T = steps * B
    u, p = u[:T].contiguous(), p[:T].contiguous()
    n = (n[:, :T] if n.dim() == 2 else n[:T].reshape(1, -1)).contiguous()      # [R, T]
    assert n.shape == (R, T)
    st = m._state(max_batch=B, need_ctx=True)
    lib = L.load()
    losses = torch.empty(steps, 3, dtype=torch.float32, device=u.device)
    if mix:
        assert lib.lgcn_ctx_get_inbatch_mix(st['ctx']) == R

        def epoch():
            L.check(lib.lgcn_train_epoch_inbatch_mix(st['ctx'], L.tp(u), L.tp(p), L.tp(n), R, T, B, L.tp(losses), L.current_stream()), "lgcn_train_epoch_inbatch_mix")
    elif a.form == "plain":
        def epoch():
            L.check(lib.lgcn_train_epoch_inbatch(st['ctx'], L.tp(u), L.tp(p), T, B, L.tp(losses), L.current_stream()), "lgcn_train_epoch_inbatch")
    else:
        def epoch():
            L.check(lib.lgcn_train_epoch_multi(st['ctx'], L.tp(u), L.tp(p), L.tp(n), R, T, B, L.tp(losses), L.current_stream()), "lgcn_train_epoch_multi")

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
    launches = kernel_times(epoch, steps) if a.profile else {}
    print("RESULT " + json.dumps({"form": a.form, "act": a.act, "temp": a.temp, "steps_per_window": a.epochs * steps, "steps_per_s": rates,
                                  "first_loss": first, "last_loss": float(losses[-1, 0]), "launch_us_per_step": launches}))


def driver(a):
    sys.path.insert(0, REPO)
    from bench import GOWALLA_NPZ
    a.npz = a.npz or GOWALLA_NPZ
    os.makedirs(a.out, exist_ok=True)
    rates, info = {}, {}

    def run(form, act):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", "--form", form, "--act", act, "--temp", str(a.temp), "--opts", a.opts,
               "--repeats", str(a.repeats), "--epochs", str(a.epochs), "--max-steps", str(a.max_steps), "--tmp", a.tmp, "--npz", a.npz,
               "--profile", str(a.profile)]
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

    for rnd in range(a.rounds):
        for act in a.acts.split(","):
            for form in a.forms.split(","):
                res = run(form, act)
                key = f"{act} {form}"
                rates.setdefault(key, []).extend(res["steps_per_s"])
                info[key] = {"first_loss": res["first_loss"], "last_loss": res["last_loss"], "launch_us_per_step": res["launch_us_per_step"]}
                print(f"round {rnd} {key}: " + " ".join(f"{x:.0f}" for x in res["steps_per_s"]), flush=True)
    out = {"workload": f"gowalla K=3 d=64 dense_last=1, {B} samples per step, one-C-call epochs, steps/s; in-batch options {a.opts}",
           "temperature": a.temp, "rounds": a.rounds, "repeats": a.repeats, "epochs_per_window": a.epochs,
           "configs": {k: dict({"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}, all=v, **info[k]) for k, v in rates.items()}}
    with open(os.path.join(a.out, a.json), "w") as f:
        json.dump(out, f, indent=1)
    for k, v in out["configs"].items():
        ib = {n: round(t, 1) for n, t in v["launch_us_per_step"].items() if n.startswith(("k_inbatch", "k_multineg"))}
        print(f"{k}: median {v['median']:.0f} steps/s ({1e6 / v['median']:.1f} us), {v['min']:.0f}..{v['max']:.0f}; launches {ib}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true", help="child: measure one configuration in this process")
    ap.add_argument("--form", default="plain", choices=FORMS)
    ap.add_argument("--forms", default=",".join(FORMS))
    ap.add_argument("--opts", default="cosine+logq", choices=["dot", "dot+logq", "cosine", "cosine+logq"], help="score options of the in-batch forms")
    ap.add_argument("--act", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--acts", default="fp32,bf16")
    ap.add_argument("--temp", type=float, default=0.1, help="temperature")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=2, help="epochs (395 steps each) per timed window")
    ap.add_argument("--max-steps", type=int, default=0, help="cut the epoch to this many steps")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--profile", type=int, default=1, help="1: per-launch times of one more epoch (torch.profiler)")
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds each child may take")
    ap.add_argument("--npz", default="", help="Gowalla interaction lists (default: tests/golden/gowalla/gowalla.npz of this tree)")
    ap.add_argument("--tmp", default="/tmp/lgcn_inbatch_mix_time")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "inbatch_mix"))
    ap.add_argument("--json", default="inbatch_mix_time.json")
    a = ap.parse_args()
    child(a) if a.one else driver(a)

"""Measure the ensemble (R seeds trained at once) against the same seeds trained one after another.
Reported, not gated (bench.py measures the flagship workload and is not involved).

    python tools/ensemble_bench.py [--out DIR] [--runs 3] [--only update|loop] [--quick]

Update loop   DI at B = 128 and the manipulator at B = 64, K = 1000 updates per call, R in
              {1, 2, 4, 8, 10, 16}: aggregate updates/s (R * K * calls / seconds) of
              Ensemble.update_rows_n (cacto_ensemble_update); baseline: R back-to-back
              RL_AC.update_rows_n (cacto_update_n) calls in the same process on the same library.
Whole loop    cacto_amd.main.train_ensemble on the double integrator, --to-path wave, three loops,
              R in {1, 4, 10}: seconds per loop; baseline: R solo cacto_amd.main.train runs in
              sequence (their seconds added, per loop).

Every variant runs `--runs` times, each in a fresh child process, the variants alternating
(ens, base, ens, base, ...); the table gives the range over the runs. A timed window is a host clock
around work that ends in a device synchronise, after a warm-up of the same shapes. Each child's
result line is appended to <out>/ensemble_bench.jsonl as soon as it exists; the driver stops at the
first child that fails. Needs the GPU: there is no CPU path.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UPDATE_CASES = (("double_integrator", 128), ("manipulator", 64))
UPDATE_R = (1, 2, 4, 8, 10, 16)
LOOP_R = (1, 4, 10)
K = 1000
CALLS = 5
N_ROWS = 8192
W_S = 1e-2


def _rows(conf, n, rng):
    """Replay rows [s, R, s', dVdx, d, term] drawn inside the conf's initial-state box."""
    import numpy as np
    ns = conf.nb_state
    lo, hi = np.array(conf.x_init_min, dtype=float), np.array(conf.x_init_max, dtype=float)
    S, Sn = rng.uniform(lo, hi, size=(n, ns)), rng.uniform(lo, hi, size=(n, ns))
    return np.concatenate([S, rng.normal(size=(n, 1)) * 0.5, Sn, rng.normal(size=(n, ns)) * 0.3,
                           (rng.uniform(size=(n, 1)) < 0.3).astype(float),
                           (rng.uniform(size=(n, 1)) < 0.2).astype(float)], axis=1)


def child_update(variant, quick):
    import numpy as np
    import torch
    from cacto_amd.confs import load_conf
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.rl import RL_AC, Ensemble
    out = {}
    k = 50 if quick else K
    for system, B in UPDATE_CASES:
        conf = load_conf(system, fresh=True)
        conf.BATCH_SIZE = B
        env = make_env(conf)
        for R in UPDATE_R:
            learners = []
            for s in range(R):
                rl = RL_AC(env, NN(env, conf, W_S, seed=s), conf)
                rl.setup_model()
                learners.append(rl)
            rng = np.random.default_rng(7)
            storages = [torch.as_tensor(_rows(conf, N_ROWS, rng), device="cuda") for _ in range(R)]
            idx = torch.as_tensor(rng.integers(0, N_ROWS, size=(R, k, B)).astype(np.int32), device="cuda")
            if variant == "ens":
                ens = Ensemble(learners)

                def run():
                    ens.update_rows_n(storages, idx)
            else:
                def run():
                    for r, rl in enumerate(learners):
                        rl.update_rows_n(storages[r], idx[r])
            run()                                               # warm-up: the same shapes
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(CALLS):
                run()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out["%s B=%d R=%d" % (system, B, R)] = R * k * CALLS / dt
            if variant == "ens":
                ens.close()
    return out


def child_loop(variant, quick):
    import numpy as np
    import torch
    from cacto_amd import main as M
    from cacto_amd.confs import load_conf
    out = {}
    loops = 3
    kw = dict(w_S=W_S, to_cfg=dict(path="wave"), accept_maxiter=True, n_loops=loops, log=lambda *_: None)

    def conf():
        c = load_conf("double_integrator", fresh=True)
        if quick:
            c.EP_UPDATE, c.UPDATE_LOOPS = 8, np.array([20, 20, 20])
        return c
    M.train(conf(), seed=1000, **dict(kw, n_loops=1))          # warm-up: code objects, allocator
    torch.cuda.synchronize()
    for R in LOOP_R:
        seeds = list(range(R))
        t0 = time.perf_counter()
        if variant == "ens":
            M.train_ensemble(conf(), seeds, **kw)
        else:
            for s in seeds:
                M.train(conf(), seed=s, N_try=s, **kw)
        torch.cuda.synchronize()
        out["R=%d" % R] = (time.perf_counter() - t0) / loops
    return out


def table(records, what, unit, fmt):
    keys = []
    for r in records:
        if r["what"] == what:
            keys += [k for k in r["result"] if k not in keys]
    lines = ["| %s | ensemble (%s) | baseline (%s) | ranges apart |" % (what, unit, unit), "|---|---|---|---|"]
    for k in keys:
        v = {var: [r["result"][k] for r in records if r["what"] == what and r["variant"] == var and k in r["result"]]
             for var in ("ens", "base")}
        if not v["ens"] or not v["base"]:
            continue
        e, b = (min(v["ens"]), max(v["ens"])), (min(v["base"]), max(v["base"]))
        better = e[0] > b[1] if what == "update" else e[1] < b[0]
        worse = e[1] < b[0] if what == "update" else e[0] > b[1]
        lines.append("| %s | %s - %s | %s - %s | %s |" % (k, fmt % e[0], fmt % e[1], fmt % b[0], fmt % b[1],
                                                       "ensemble better" if better else "ensemble worse" if worse
                                                       else "overlap"))
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "bench_outputs"))
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--only", choices=["update", "loop"], default=None)
    p.add_argument("--quick", action="store_true", help="tiny sizes: a rehearsal of the tool, not a measurement")
    p.add_argument("--child", nargs=2, metavar=("WHAT", "VARIANT"), default=None)
    a = p.parse_args()
    if a.child:
        what, variant = a.child
        res = (child_update if what == "update" else child_loop)(variant, a.quick)
        print("RESULT " + json.dumps(dict(what=what, variant=variant, result=res)))
        return 0
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "ensemble_bench.jsonl")
    records = []
    for what, limit in (("update", 300), ("loop", 900)):
        if a.only and a.only != what:
            continue
        for run in range(a.runs):
            for variant in ("ens", "base"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", what, variant] + (["--quick"] * a.quick)
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
                except subprocess.TimeoutExpired:
                    print("child %s/%s run %d passed its %d s limit: stopping" % (what, variant, run, limit))
                    return 1
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
                    print("child %s/%s run %d failed (rc %d): stopping" % (what, variant, run, r.returncode))
                    return 1
                rec = dict(json.loads(line[-1][7:]), run=run)
                records.append(rec)
                with open(path, "a") as f:
                    f.write(json.dumps(rec) + "\n")
                print("%s %s run %d done" % (what, variant, run), flush=True)
    text = "\n\n".join(t for t in (
        table(records, "update", "updates/s", "%.0f") if a.only != "loop" else "",
        table(records, "loop", "s per loop", "%.2f") if a.only != "update" else "") if t)
    with open(os.path.join(a.out, "ensemble_bench.md"), "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Compare TO configs by what the networks learn from them, with the validation stage as the
instrument: cacto_amd.main.train_ensemble(validate=True) on one system for a list of TO configs,
and per config and loop the mean +- std over the seeds of every validation metric.

    python tools/validate_modes.py [--system-id double_integrator] [--seeds 0,1,2,3] [--loops 3]
                                   [--modes "default;hessian=psd;bounds=conf;bounds=conf,labels=bounded"]
                                   [--w-S 1e-2] [--to-path wave] [--out FILE.json]
    python tools/validate_modes.py --cost double_integrator,car [--runs 3] [--to-path default]

A mode is a comma-separated list of key=value pairs over cacto_amd.to.DEFAULT_CFG ("default": none),
e.g. "starts=4" or "starts=4,start_sigma=0.25,start_hold=4" for several warm starts per TO episode;
such a mode's rows also carry the loop's rescued and improved episodes.

What is comparable across modes: gap_* and warm / to costs (the solver's own cost of the actor's
roll-out against its solution) and value_* (V against the reward-to-go of the trajectory) measure
the networks against the trajectories themselves. grad_* and sobolev_loss are measured against each
mode's OWN labels (labels=bounded and hessian=psd change the labels), so they say how well a critic
fits its labels, not which labels are better. With bounds=conf the trajectories obey the limits, so
their cost is that of another problem: compare gaps, not costs, between bounded and unbounded modes.

--cost: the price of the stage. Per system, the shipped conf (its EP_UPDATE episodes), one learner:
RL_AC.compute_samples with and without validate, alternating in one process after a warm-up of each,
`--runs` timed runs each, a host clock around the call and a device synchronise; and the stage alone
(validate_samples between two synchronises: its launches, its three small copies to the host and the
host arithmetic). Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_MODES = "default;hessian=psd;bounds=conf;bounds=conf,labels=bounded"
METRICS = ("rows", "value_rmse", "value_r2", "grad_rmse", "grad_rel", "sobolev_loss", "actor_rmse_u",
           "warm_cost_mean", "to_cost_mean", "gap_mean", "gap_rel_median")
NUMERIC = dict(starts=int, start_hold=int, start_seed=int, start_sigma=float)
MULTISTART = ("rescued", "improved")     # per loop, of a mode with starts=N > 1 (train's `multistart` records)


def parse_mode(text):
    cfg = {}
    if text.strip() not in ("", "default"):
        for part in text.split(","):
            k, v = part.split("=")
            k, v = k.strip(), v.strip()
            # the multi-start keys are numbers ("starts=4", "start_sigma=0.25", "start_hold=4"); the rest are names
            cfg[k] = NUMERIC[k](v) if k in NUMERIC else v
    return cfg


def run_modes(args):
    import numpy as np
    from cacto_amd.confs import load_conf
    from cacto_amd.main import train_ensemble
    seeds = [int(s) for s in args.seeds.split(",")]
    table = []
    for mode in args.modes.split(";"):
        conf = load_conf(args.system_id, fresh=True)
        conf.NNs_path = None
        cfg = dict(parse_mode(mode), path=args.to_path)
        outs = train_ensemble(conf, seeds, w_S=args.w_S, to_cfg=cfg, accept_maxiter=args.accept_maxiter,
                              n_loops=args.loops, log=lambda *_: None, validate=True)
        for ep in range(len(outs[0]["validation"])):
            row = dict(mode=mode.strip() or "default", ep=ep, warm=outs[0]["validation"][ep]["warm"])
            for k in METRICS:
                vals = [o["validation"][ep][k] for o in outs]
                if any(v is None for v in vals):
                    row[k] = None
                else:
                    row[k] = (float(np.mean(vals)), float(np.std(vals)))
            for k in MULTISTART:
                vals = [o["multistart"][ep][k] for o in outs if len(o["multistart"]) > ep]
                row[k] = (float(np.mean(vals)), float(np.std(vals))) if vals else None
            table.append(row)
    print("system %s, seeds %s, w_S %g, to-path %s, accept_maxiter %s: mean +- std over the seeds"
          % (args.system_id, seeds, args.w_S, args.to_path, args.accept_maxiter))
    print("| mode | loop | warm | " + " | ".join(METRICS + MULTISTART) + " |")
    print("|" + "---|" * (3 + len(METRICS + MULTISTART)))
    for row in table:
        cells = ["-" if row[k] is None else "%.4g ± %.2g" % row[k] for k in METRICS + MULTISTART]
        print("| %s | %d | %s | %s |" % (row["mode"], row["ep"], row["warm"], " | ".join(cells)))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(system=args.system_id, seeds=seeds, w_S=args.w_S, to_path=args.to_path, table=table), f,
                      indent=1)


def run_cost(args):
    import random

    import numpy as np
    import torch
    from cacto_amd.confs import load_conf
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.replay_buffer import ReplayBuffer
    from cacto_amd.rl import RL_AC
    from cacto_amd.to import TO
    for system in args.cost.split(","):
        conf = load_conf(system, fresh=True)
        random.seed(0)
        np.random.seed(0)
        env = make_env(conf)
        rl = RL_AC(env, NN(env, conf, args.w_S, seed=0), conf)
        rl.setup_model()
        to = TO(env, conf, args.w_S)
        ics = [env.reset() for _ in range(conf.EP_UPDATE)]
        cfg = dict(path=args.to_path)

        stage = []
        real = rl.validate_samples

        def timed_stage(*a, **k):                        # the stage alone: a synchronise on either side
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = real(*a, **k)
            torch.cuda.synchronize()
            stage.append(time.perf_counter() - t0)
            return out
        rl.validate_samples = timed_stage

        def once(validate):
            buf = ReplayBuffer(conf)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = rl.compute_samples(1, ics, to, buf, cfg=cfg, accept_maxiter=True, validate=validate)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, res["rows"]
        once(False), once(True)                          # warm-up of both shapes
        del stage[:]
        secs = {False: [], True: []}
        for _ in range(args.runs):
            for v in (False, True):
                t, rows = once(v)
                secs[v].append(t)
        fmt = lambda x: "%.1f-%.1f ms" % (min(x) * 1e3, max(x) * 1e3)
        print("%s: %d episodes, %d rows, to-path %s: compute_samples %s, with validate %s (%d runs each, alternating); "
              "validate_samples alone %.2f-%.2f ms"
              % (system, conf.EP_UPDATE, rows, args.to_path, fmt(secs[False]), fmt(secs[True]), args.runs,
                 min(stage) * 1e3, max(stage) * 1e3))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--system-id", default="double_integrator")
    p.add_argument("--seeds", default="0,1,2,3")
    p.add_argument("--loops", type=int, default=3)
    p.add_argument("--modes", default=DEFAULT_MODES)
    p.add_argument("--w-S", type=float, default=1e-2)
    p.add_argument("--to-path", default=None, help="default: wave for the modes, default for --cost")
    p.add_argument("--accept-maxiter", action="store_true")
    p.add_argument("--out", default=None)
    p.add_argument("--cost", default=None, help="comma-separated systems: time compute_samples with / without validate")
    p.add_argument("--runs", type=int, default=3)
    args = p.parse_args(argv)
    if args.cost:
        args.to_path = args.to_path or "default"
        run_cost(args)
    else:
        args.to_path = args.to_path or "wave"
        run_modes(args)


if __name__ == "__main__":
    main()

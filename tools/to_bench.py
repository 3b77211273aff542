"""Throughput of the batched iLQR trajectory optimiser (cacto_to_solve) on the double integrator:
full-length episodes from Env.reset (the reference's main.py:225-230 draws), zero warm start, the
full-solve settings of the tests (gtol 1e-4, max_iter 400, max_ls 10, armijo 1e-4, mu x10 / /10
from 1e-6). Prints one JSON line: episodes/s, mean and max backward passes, the share per status.

    python tools/to_bench.py [--system double_integrator] [--episodes 4096] [--path default|wave] [--repeat 3]
                             [--hessian exact|psd] [--bounds none|conf] [--helper 8]
                             [--starts 1,2,4,8 [--start-sigma 0.5] [--start-hold 8] [--accept-maxiter]]

--starts with anything but 1 measures the multi-start solve (TO.solve_multistart) instead and prints
one JSON line with a row per value, starts = 1 (the plain solve) timed in the same rotation.

--path wave runs the one-workgroup-per-episode persistent kernel (cacto_to_cfg.path; not the
manipulator and UR5, which have none):
the path for per-episode calls (--episodes 1) and batches of the reference's size (EP_UPDATE: 200).
The result carries the plan of the config (cacto_to_solve_plan: on_device, block_threads, lds_bytes,
launches_per_iter) beside the figures.

--hessian psd solves with every node's l_xx projected onto the positive semidefinite cone
(cacto_to_opts.hessian); the result line carries the mode.

--bounds conf solves under the conf's u_min / u_max as hard limits (cacto_to_box, control-limited
DDP); the result line carries the mode and the share of the returned controls that sit on a bound.

--helper N also times tests/ilqr_ref.py (numpy, one core) on the first N of those episodes and
reports its seconds per episode. Reported, not gated: there is no earlier figure to compare with,
and the reference's IPOPT solve cannot run without CasADi.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="double_integrator")
    ap.add_argument("--episodes", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--helper", type=int, default=0)
    ap.add_argument("--poll-every", type=int, default=8)
    ap.add_argument("--path", default="default", choices=["default", "wave"])
    ap.add_argument("--hessian", default="exact", choices=["exact", "psd"])
    ap.add_argument("--bounds", default="none", choices=["none", "conf"])
    ap.add_argument("--helper-only", action="store_true", help="time the helper alone (needs no GPU)")
    ap.add_argument("--starts", default=[1], type=lambda s: [int(v) for v in s.split(",")],
                    help="warm starts per episode, or a list timed in rotation, e.g. 1,2,4,8 (multistart below)")
    ap.add_argument("--start-sigma", type=float, default=0.5)
    ap.add_argument("--start-hold", type=int, default=8)
    ap.add_argument("--accept-maxiter", action="store_true", help="with --starts: MAXITER counts as kept")
    args = ap.parse_args()

    import ilqr_ref as R
    from cacto_amd.confs import load_conf
    from oracle import env as oenv

    conf = load_conf(args.system)
    rng = random.Random(0)
    oe = oenv.make_env(conf)
    S0 = np.array([oe.reset(rng) for _ in range(args.episodes)], dtype=np.float64)
    Te = np.array([conf.NSTEPS - int(s[-1] / conf.dt) for s in S0], dtype=np.int32)
    if args.helper_only:
        print(json.dumps(dict(metric="to_helper_seconds_per_episode", system=args.system, **helper(R, args, S0, Te))))
        return
    import torch
    from cacto_amd.environment import make_env
    from cacto_amd.to import TO
    to = TO(make_env(conf), conf)
    cfg = dict(R.SOLVE_CFG, poll_every=args.poll_every, path=args.path, hessian=args.hessian)
    if args.bounds != "none":       # the key only when asked for: a library of an older revision has no such entry
        cfg["bounds"] = args.bounds
    from cacto_amd import _lib
    # a library of an older revision (CACTO_HIP_LIB with CACTO_LIB_PARTIAL=1, cacto_amd/_lib.py: A/B runs)
    # has no plan entry
    plan = to.solve_plan(cfg) if hasattr(_lib.lib().dll, "cacto_to_solve_plan") else None
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    S0_d, Te_d = dev(S0), dev(Te)
    U0_d = torch.zeros(args.episodes, max(int(Te.max()), 1), conf.nb_action, dtype=torch.float64, device="cuda")
    if args.starts != [1]:
        print(json.dumps(multistart(args, R, to, cfg, plan, S0_d, U0_d, Te_d, Te)))
        return
    times = []
    for _ in range(args.repeat + 1):        # the first run warms up (workspace, code objects)
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = to.solve_batch(S0_d, U0_d, Te_d, cfg=cfg)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    best = min(times[1:])
    status, iters = out["status"].cpu().numpy(), out["iters"].cpu().numpy()
    J = out["J"].cpu().numpy()
    U = out["U"].cpu().numpy()
    mask = np.arange(U.shape[1])[None, :, None] < Te[:, None, None]
    at_bound = ((U == conf.u_min) | (U == conf.u_max)) & mask
    outside = ((U < conf.u_min) | (U > conf.u_max)) & mask
    n_ctrl = max(int(mask.sum()) * conf.nb_action, 1)
    res = dict(metric="to_solve_episodes_per_s", system=args.system, path=args.path, hessian=args.hessian,
               bounds=args.bounds, controls_at_bound=float(at_bound.sum() / n_ctrl),
               controls_outside=float(outside.sum() / n_ctrl), episodes=args.episodes,
               mean_steps=float(Te.mean()), seconds=best, seconds_all=times[1:], episodes_per_s=args.episodes / best,
               iters_mean=float(iters.mean()), iters_max=int(iters.max()),
               status_share=dict(converged=float((status == R.CONVERGED).mean()),
                                 maxiter=float((status == R.MAXITER).mean()), failed=float((status == R.FAILED).mean())),
               monotone=bool((J[:, 1] <= J[:, 0]).all()), plan=plan)
    if args.helper > 0:
        res.update(helper(R, args, S0, Te))
        res["gpu_status_same_episodes"] = status[:args.helper].tolist()
        res["gpu_iters_same_episodes"] = iters[:args.helper].tolist()
    print(json.dumps(res))


def multistart(args, R, to, cfg, plan, S0_d, U0_d, Te_d, Te):
    """--starts N[,N..]: TO.solve_multistart for every N of the list on the same episodes, timed in
    rotation (each round runs every N once, in the list's order; the first round warms up), so that
    starts = 1 — solve_batch itself — is the baseline of the same run. Per N: the best seconds, the
    share of kept episodes (CONVERGED, or MAXITER with --accept-maxiter), the mean final cost of the
    kept ones, and rl.multistart_stats (rescued, improved, won_by, gain_rel_median). The warm start
    is zero, so there is no all-zero candidate: every candidate past 0 is a perturbation."""
    import torch
    from cacto_amd.rl import multistart_stats
    times = {N: [] for N in args.starts}
    outs = {}
    for _ in range(args.repeat + 1):
        for N in args.starts:
            c = dict(cfg, starts=N, start_sigma=args.start_sigma, start_hold=args.start_hold)
            torch.cuda.synchronize()
            t = time.perf_counter()
            outs[N] = to.solve_multistart(S0_d, U0_d, Te_d, cfg=c, seed=0, zero_start=False,
                                          accept_maxiter=args.accept_maxiter)
            torch.cuda.synchronize()
            times[N].append(time.perf_counter() - t)
    rows = []
    for N in args.starts:
        status, J = outs[N]["status"].cpu().numpy(), outs[N]["J"].cpu().numpy()
        keep = (status == R.CONVERGED) | (args.accept_maxiter & (status == R.MAXITER))
        row = dict(starts=N, seconds=min(times[N][1:]), seconds_all=times[N][1:], kept_share=float(keep.mean()),
                   kept_cost_mean=float(J[keep, 1].mean()) if keep.any() else None,
                   status_share=dict(converged=float((status == R.CONVERGED).mean()),
                                     maxiter=float((status == R.MAXITER).mean()),
                                     failed=float((status == R.FAILED).mean())))
        if N > 1:
            row.update(multistart_stats(outs[N], np.where(keep, Te, -1), args.accept_maxiter))
        rows.append(row)
    return dict(metric="to_multistart", system=args.system, path=args.path, hessian=args.hessian, bounds=args.bounds,
                episodes=args.episodes, mean_steps=float(Te.mean()), accept_maxiter=bool(args.accept_maxiter),
                start_sigma=args.start_sigma, start_hold=args.start_hold, plan=plan, rows=rows)


def helper(R, args, S0, Te):
    P = R.Problem(args.system)
    n = max(args.helper, 1)
    t = time.perf_counter()
    hs, hi = [], []
    for e in range(n):
        r = P.solve(S0[e], np.zeros((max(int(Te[e]), 1), P.m)), int(Te[e]))
        hs.append(int(r["status"]))
        hi.append(int(r["iters"]))
    return dict(helper_seconds_per_episode=(time.perf_counter() - t) / n, helper_status=hs, helper_iters=hi,
                helper_steps=[int(v) for v in Te[:n]])


if __name__ == "__main__":
    main()

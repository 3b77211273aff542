"""Throughput of the sample-collection stage (RL_AC.compute_samples: main.py:174-195 for every initial
state of an iteration + the buffer.add of main.py:240), or of the per-episode shim loop it replaces
(create_TO_init -> TO_Solve -> RL_Solve per episode, one buffer.add), on the same seeded Env.reset
states. Prints one JSON line: episodes/s, the counters, and for the stage its split by device
events (roll-out, solve, labels, ring write).

    python tools/collect_bench.py --system double_integrator --episodes 200 [--path wave] [--per-episode]
                                  [--ep 1] [--weights di_seed0_final] [--w-S 1e-2] [--repeat 1] [--root DIR]

Every shape is warmed by one untimed run; each timed run starts from an empty buffer and ends in a
device synchronise. --ep 0 solves from the zero warm start (no actor), --ep 1 from the roll-out of
the actor of --weights (a fixture of tests/golden/weights; fresh initial weights without it).
--root DIR imports cacto_amd from another checkout (built there): the per-episode loop uses only
the reference-signature shims, so it also times a revision from before the stage existed.
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_weights(root, tag):
    z = np.load(os.path.join(root, "tests", "golden", "weights", tag + ".npz"))
    get = lambda k, n: [z["%s_%d" % (k, i)] for i in range(n)]  # noqa: E731
    out = {"actor": get("actor", 6), "critic": get("critic", 10)}
    if "target_0" in z:
        out["target"] = get("target", 10)
    return out


def per_episode(rl, to, buffer, ep, ICS_list, cfg, accept_maxiter):
    """main.py:174-195 per episode, :236-240 once."""
    tmp = []
    for ICS in ICS_list:
        init, states, controls, T, ok = rl.create_TO_init(ep, ICS)
        if ok == 0:
            continue
        U, X, flag, ee, step_cost, dVdx = to.TO_Solve(init, states, controls, T, cfg=cfg, accept_maxiter=accept_maxiter)
        if flag == 0:
            continue
        state_arr, partial, total, s_next, done, rwrd, term, ep_return, ee_rl = rl.RL_Solve(U, X, step_cost)
        tmp.append((dVdx, state_arr.tolist(), partial, s_next, done, term, ep_return))
    if tmp:
        dVdx, state_arr, partial, s_next, done, term, ep_return = zip(*tmp)
        buffer.add(state_arr, partial, s_next, dVdx, done, term)
    return dict(n_kept=len(tmp), rows=int(buffer.next_idx))


def stage_split(torch, rl, to, buffer, ep, ICS, cfg, accept_maxiter):
    """The stage's calls one by one with device events between them (milliseconds per part)."""
    from cacto_amd import _lib as L
    from cacto_amd.system import dptr, stream
    E = len(ICS)
    ns_ = np.array([rl.nsteps_sh(s) for s in ICS], dtype=np.int32)
    T = int(ns_.max())
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    inputs = rl.rollout_inputs(ICS, ns_)
    S0_d, n_d = inputs[0], inputs[1]
    marks[0].record()
    roll = rl.rollout_batch(ICS, ns_, T, ep=ep, want=("S", "A"), inputs=inputs)
    warm = roll["A"].double() if ep != 0 else torch.zeros(E, T, rl.conf.nb_action, dtype=torch.float64, device="cuda")
    live = torch.where((roll["status"] == 0) & (n_d > 0), n_d, torch.full_like(n_d, -1))
    marks[1].record()
    sol = to.solve_batch(S0_d, warm, live, cfg=cfg)
    marks[2].record()
    kept_d = torch.empty(E, dtype=torch.int32, device="cuda")
    off_d = torch.empty(E + 1, dtype=torch.int64, device="cuda")
    counts_d = torch.empty(8, dtype=torch.int64, device="cuda")
    L.lib().call("cacto_collect_plan", dptr(n_d), dptr(roll["status"]), dptr(sol["status"]), int(accept_maxiter), E,
                 dptr(kept_d), dptr(off_d), dptr(counts_d), stream())
    rows = int(counts_d[0].item())
    dVdx = to.backward_pass_batch(sol["S"], sol["U"], kept_d) if to.w_S != 0 else None
    marks[3].record()
    if rl.conf.env_RL:
        S_rows, R_rows, _ = rl.env_rl_episodes(S0_d, sol["U"], kept_d, T + 1)
    else:
        S_rows, R_rows = sol["S"], -sol["step_cost"]
    buffer.add_episodes_planned(S_rows, R_rows, off_d, rows, T, dVdx=dVdx)
    marks[4].record()
    torch.cuda.synchronize()
    # labels_ms: the plan, the copy of its counters and the label pass; ring_write_ms: the env_RL
    # re-simulation (when conf.env_RL) and cacto_rl_solve_add
    names = ("rollout_ms", "solve_ms", "labels_ms", "ring_write_ms")
    return {n: marks[i].elapsed_time(marks[i + 1]) for i, n in enumerate(names)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--system", default="double_integrator")
    ap.add_argument("--episodes", type=int, default=200)
    ap.add_argument("--path", default="default", choices=["default", "wave"])
    ap.add_argument("--per-episode", action="store_true", help="time the per-episode shim loop instead of the stage")
    ap.add_argument("--ep", type=int, default=0)
    ap.add_argument("--weights", default=None)
    ap.add_argument("--w-S", type=float, default=1e-2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--accept-maxiter", action="store_true")
    ap.add_argument("--root", default=HERE, help="the checkout to import cacto_amd from")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [root]

    import torch
    from cacto_amd.confs import load_conf
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.replay_buffer import PrioritizedReplayBuffer, ReplayBuffer
    from cacto_amd.rl import RL_AC
    from cacto_amd.to import TO

    conf = load_conf(args.system, fresh=True)
    env = make_env(conf)
    rl = RL_AC(env, NN(env, conf, args.w_S), conf, 0)
    rl.setup_model(weights=load_weights(root, args.weights) if args.weights else None)
    to = TO(env, conf, args.w_S)
    cfg = dict(path=args.path)
    random.seed(args.seed)
    ICS = [env.reset() for _ in range(args.episodes)]
    new_buffer = lambda: (ReplayBuffer(conf) if conf.prioritized_replay_alpha == 0  # noqa: E731
                          else PrioritizedReplayBuffer(conf))

    def run(buffer):
        if args.per_episode:
            return per_episode(rl, to, buffer, args.ep, ICS, cfg, args.accept_maxiter)
        res = rl.compute_samples(args.ep, ICS, to, buffer, cfg=cfg, accept_maxiter=args.accept_maxiter)
        return {k: v for k, v in res.items() if k not in ("kept", "ep_return", "dev")}

    run(new_buffer())                               # warms every shape, sizes the workspaces
    torch.cuda.synchronize()
    times, counters = [], None
    for _ in range(args.repeat):
        buffer = new_buffer()
        torch.cuda.synchronize()
        t = time.perf_counter()
        counters = run(buffer)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    res = dict(metric="collect_episodes_per_s", mode="per_episode" if args.per_episode else "stage",
               system=args.system, path=args.path, episodes=args.episodes, ep=args.ep, w_S=args.w_S,
               seconds=min(times), seconds_all=times, episodes_per_s=args.episodes / min(times), counters=counters,
               own_checkout=root == HERE)
    if not args.per_episode:
        res["split"] = stage_split(torch, rl, to, new_buffer(), args.ep, np.asarray(ICS), cfg, args.accept_maxiter)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

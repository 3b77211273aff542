"""The CACTO training loop (main.py:145-165, :216-262, :276) on the device, without the plots.

    python -m cacto_amd.main --system-id double_integrator --w-S 1e-2

Per loop: EP_UPDATE initial states from Env.reset (the host's `random`, as the reference), one
RL_AC.compute_samples (roll-outs -> batched TO -> filter -> labels -> RL_Solve + ring write, all on
the device), one RL_AC.learn_and_update. No CasADi, no per-episode host work.
"""
import argparse
import os
import random

import numpy as np

from .confs import SYSTEM_MAP, load_conf


def parse_args(argv=None):
    """The reference's options (main.py:18-46) that have a meaning here, plus --nb-loops (stop after
    that many loops), --to-path (which kernels solve the TO batch, cacto_amd.to.PATHS) and
    --accept-maxiter (keep episodes whose solve stopped at max_iter). Returns a dict."""
    p = argparse.ArgumentParser(prog="python -m cacto_amd.main", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--test-n", type=int, default=0, help="Test number")
    p.add_argument("--seed", type=int, default=0, help="random and numpy.random seed")
    p.add_argument("--system-id", type=str, default="single_integrator", choices=sorted(SYSTEM_MAP),
                   help="System-id")
    p.add_argument("--recover-training-flag", action="store_true", help="Flag to recover training")
    p.add_argument("--w-S", type=float, default=0, help="Sobolev training - weight of the value related error")
    p.add_argument("--nb-loops", type=int, default=None, help="Stop after this many loops (default: conf.NLOOPS)")
    p.add_argument("--to-path", type=str, default="default", choices=["default", "wave"],
                   help="Kernels of the batched trajectory optimiser")
    p.add_argument("--accept-maxiter", action="store_true",
                   help="Keep episodes whose TO solve stopped at max_iter without converging")
    return vars(p.parse_args(argv))


def train_kwargs(args):
    """parse_args' dict -> (system_id, keyword arguments of train)."""
    return args["system_id"], dict(seed=args["seed"], N_try=args["test_n"], w_S=args["w_S"],
                                   to_cfg=dict(path=args["to_path"]), accept_maxiter=args["accept_maxiter"],
                                   n_loops=args["nb_loops"], recover=args["recover_training_flag"])


def train(conf, seed=0, N_try=0, w_S=0.0, to_cfg=None, accept_maxiter=False, n_loops=None, weights=None,
          recover_training=None, log=print):
    """main.py:145-165, :216-262, :276. `to_cfg`: a dict over cacto_amd.to.DEFAULT_CFG; `weights`:
    setup_model's dict of initial weights; `recover_training`: (path, N_try, step) of checkpoints to
    start from (the update counter starts at step). A loop in which no episode is kept raises
    RuntimeError (the reference fails there too, on zip(*tmp)). Returns dict(update_step_counter,
    ep_reward_arr, counts_per_loop, RLAC, buffer)."""
    from .environment import make_env
    from .neural_network import NN
    from .replay_buffer import PrioritizedReplayBuffer, ReplayBuffer
    from .rl import RL_AC
    from .to import TO
    random.seed(seed)
    np.random.seed(seed)
    env = make_env(conf)
    NN_inst = NN(env, conf, w_S, seed=seed)
    TrOp = TO(env, conf, w_S)
    RLAC = RL_AC(env, NN_inst, conf, N_try)
    buffer = ReplayBuffer(conf) if conf.prioritized_replay_alpha == 0 else PrioritizedReplayBuffer(conf)
    if getattr(conf, "NNs_path", None):
        os.makedirs(os.path.join(conf.NNs_path, "N_try_%s" % N_try), exist_ok=True)
    update_step_counter = 0
    if recover_training is not None:
        update_step_counter = int(recover_training[2])
    RLAC.setup_model(recover_training=recover_training, weights=weights)
    if getattr(conf, "NNs_path", None):
        RLAC.RL_save_weights(update_step_counter)

    # NLOOPS and NEPISODES (conf_*.py) from the schedule itself, so a conf whose UPDATE_LOOPS or
    # EP_UPDATE was changed after import is read consistently
    n_sched = len(conf.UPDATE_LOOPS)
    loops = n_sched if n_loops is None else min(int(n_loops), n_sched)
    ep_arr_idx = 0
    ep_reward_arr = np.zeros(int(conf.EP_UPDATE) * n_sched) * np.nan
    counts_per_loop = []
    for ep in range(loops):
        init_rand_state = [env.reset() for _ in range(conf.EP_UPDATE)]
        res = RLAC.compute_samples(ep, init_rand_state, TrOp, buffer, cfg=to_cfg, accept_maxiter=accept_maxiter)
        counts_per_loop.append({k: res[k] for k in ("rows", "n_kept", "zero_length", "nan_rollouts", "converged",
                                                    "maxiter", "failed")})
        n = res["n_kept"]
        if n == 0:
            raise RuntimeError("loop %d: no episode of %d was kept (%s)" % (ep, conf.EP_UPDATE, counts_per_loop[-1]))
        update_step_counter = RLAC.learn_and_update(update_step_counter, buffer, ep)
        ep_return = res["ep_return"]
        ep_reward_arr[ep_arr_idx:ep_arr_idx + n] = ep_return
        ep_arr_idx += n
        for i in range(n):
            log("Episode  {}  --->   Return = {}".format(ep * n + i, ep_return[i]))
        if hasattr(conf, "NUPDATES") and update_step_counter > conf.NUPDATES:
            break
    if getattr(conf, "NNs_path", None):
        RLAC.RL_save_weights()
    return dict(update_step_counter=update_step_counter, ep_reward_arr=ep_reward_arr, counts_per_loop=counts_per_loop,
                RLAC=RLAC, buffer=buffer)


def main(argv=None):
    system_id, kw = train_kwargs(parse_args(argv))
    conf = load_conf(system_id)
    if not getattr(conf, "NNs_path", None):
        conf.NNs_path = os.path.join(os.getcwd(), "Results " + system_id, "NNs")
    recover = None
    if kw.pop("recover"):
        recover = (conf.NNs_path_rec, conf.N_try_rec, conf.update_step_counter_rec)
    log = print
    log("System: {} - N_try = {}".format(conf.system_id, kw["N_try"]))
    out = train(conf, recover_training=recover, log=log, **kw)
    log("Updates: {}  kept per loop: {}".format(out["update_step_counter"],
                                                [c["n_kept"] for c in out["counts_per_loop"]]))
    return out


if __name__ == "__main__":
    main()
